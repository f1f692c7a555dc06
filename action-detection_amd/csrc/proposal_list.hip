// The proposal-list stage for a BATCH of videos: what the reference does per video in Python loops between the score
// pickle and the list file the trainers read
//   exponential sliding windows       /root/reference/ops/sequence_funcs.py:37-54 (gen_exponential_sw_proposal)
//   the integer columns of the list   /root/reference/ops/io.py:109-127 (dump_window_list: spans in seconds -> frame numbers)
// Naming (tag.hip) and recall (eval.hip) read the windows this file writes where it wrote them.  All arithmetic is fp64 or
// int32, every fp64 result is ONE IEEE operation (a division, a multiplication, a subtraction; nothing to contract, and
// contraction is off), so the numbers are the reference's bit for bit.  Launches per call do not depend on the number of
// videos.
#include "ssn_common.h"

#pragma clang fp contract(off)

namespace {

constexpr int SW_MAX_LEVELS = 31;          // spans 2^0 ... 2^30
constexpr int SW_MAX_CANDIDATES = 1 << 30;

struct SwLevels {
    int n;
    int span[SW_MAX_LEVELS];
    int step[SW_MAX_LEVELS];
};

// the largest i with off[i] <= w (off non-decreasing, off[0] = 0 <= w < off[n])
__device__ __forceinline__ int pl_find(const int* off, int n, int w) {
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (off[mid] <= w) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// `min(duration, s + t_span) - s >= 1` as the reference writes it (Python's min: the first argument unless the second is smaller)
__device__ __forceinline__ bool sw_valid(double duration, long k, int step, int span) {
    const double s = (double)(k * step);                 // k * step < 2^53: exact, as numpy's start + k * delta is
    const double e = s + (double)span;
    const double clipped = e < duration ? e : duration;
    return clipped - s >= 1.0;
}

// One lane per (video, level).  np.arange(0, duration, step) has ceil(duration / step) entries k * step (none when the
// duration is not positive); the windows that keep at least one second inside the video are a PREFIX in k: while
// s + t_span <= duration the clipped length is t_span >= 1, afterwards it is duration - s, which only shrinks -- a binary
// search over the predicate itself finds the prefix length without restating it.
__global__ __launch_bounds__(256) void sw_count_kernel(const double* durations, int V, SwLevels lv, int* counts) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= V * lv.n) return;
    const int v = i / lv.n, l = i - v * lv.n;
    const double d = durations[v];
    const int step = lv.step[l], span = lv.span[l];
    int kept = 0;
    if (d > 0.0) {
        const double c = ceil(d / (double)step);
        const long cand = c < (double)SW_MAX_CANDIDATES ? (long)c : (long)SW_MAX_CANDIDATES;      // (inf -> the cap; the host refuses it)
        long lo = 0, hi = cand;                         // kept prefix length lies in [lo, hi]
        while (lo < hi) {
            const long mid = (lo + hi + 1) >> 1;        // are the first `mid` windows kept, i.e. is window mid - 1?
            if (sw_valid(d, mid - 1, step, span)) lo = mid;
            else hi = mid - 1;
        }
        kept = (int)lo;
    }
    counts[i] = kept;
}

// One lane per window: row w of (video, level) i = the largest i with off[i] <= w is the window k = w - off[i] of that
// level, (k * step, k * step + t_span).  Rows are level ascending, start ascending inside a video -- the reference's order.
__global__ __launch_bounds__(256) void sw_fill_kernel(const int* off, int VL, SwLevels lv, int W, double* windows) {
    const int w = blockIdx.x * 256 + threadIdx.x;
    if (w >= W) return;
    const int i = pl_find(off, VL, w);
    const int l = i % lv.n;
    const long k = (long)w - off[i];
    if (k < 0 || k >= SW_MAX_CANDIDATES) return;        // tables and W disagree: leave the row (zero-filled by the caller)
    const double s = (double)(k * lv.step[l]);
    windows[2 * (long)w] = s;
    windows[2 * (long)w + 1] = s + (double)lv.span[l];
}

// int(x) of Python for a product that fits int32; anything else (NaN, inf, out of range) reports and yields 0
__device__ __forceinline__ int pl_trunc(double x, bool& bad) {
    if (!(x > -2147483649.0 && x < 2147483648.0)) {
        bad = true;
        return 0;
    }
    return (int)x;                                       // (truncation toward zero)
}

// One lane per span, ground truth first, proposals behind it: (int(start * real_fps), int(end * real_fps)) with
// real_fps = float(frame_cnt) / float(duration) of the span's video.
__global__ __launch_bounds__(256) void pl_rows_kernel(const double* gt_span, const int* gt_off, int G, const double* prop,
                                                      const int* prop_off, int P, const int* frame_cnt,
                                                      const double* durations, int V, int* gt_frames, int* frames,
                                                      int* status) {
    const long r = (long)blockIdx.x * 256 + threadIdx.x;
    if (r >= (long)G + P) return;
    const bool is_gt = r < G;
    const int j = (int)(is_gt ? r : r - G);
    const int v = pl_find(is_gt ? gt_off : prop_off, V, j);
    const double real_fps = (double)frame_cnt[v] / durations[v];
    const double* src = (is_gt ? gt_span : prop) + 2 * (long)j;
    int* dst = (is_gt ? gt_frames : frames) + 2 * (long)j;
    bool bad = false;
    dst[0] = pl_trunc(src[0] * real_fps, bad);
    dst[1] = pl_trunc(src[1] * real_fps, bad);
    if (bad) atomicOr(&status[v], is_gt ? 1 : 2);
}

int sw_levels(const int* h_spans, const int* h_steps, int L, SwLevels* lv, const char* who) {
    SSN_CHECK_ARG(h_spans && h_steps, "%s: null pointer", who);
    SSN_CHECK_ARG(L >= 1 && L <= SW_MAX_LEVELS, "%s: %d levels, 1 ... %d supported", who, L, SW_MAX_LEVELS);
    lv->n = L;
    for (int l = 0; l < SW_MAX_LEVELS; ++l) {
        lv->span[l] = l < L ? h_spans[l] : 1;
        lv->step[l] = l < L ? h_steps[l] : 1;
        SSN_CHECK_ARG(lv->span[l] >= 1 && lv->step[l] >= 1, "%s: level %d has span %d and step %d, both must be at least 1", who,
                      l, lv->span[l], lv->step[l]);
    }
    return SSN_OK;
}

}  // namespace

// Counting phase of the sliding windows: durations [V] fp64 (device), h_spans / h_steps [L] int32 on the HOST (t_span and
// step of every level, validated here before any launch) -> counts [V][L] int32 (device): windows of every (video, level).
extern "C" int ssn_sw_count(const double* durations, int V, const int* h_spans, const int* h_steps, int L, int* counts,
                            hipStream_t stream) {
    SwLevels lv;
    if (int rc = sw_levels(h_spans, h_steps, L, &lv, "sw_count")) return rc;
    SSN_CHECK_ARG(V >= 1 && (long)V * L < (1L << 30), "sw_count: bad sizes");
    SSN_CHECK_ARG(durations && counts, "sw_count: null pointer");
    hipLaunchKernelGGL(sw_count_kernel, dim3((unsigned)((V * L + 255) / 256)), dim3(256), 0, stream, durations, V, lv, counts);
    SSN_CHECK_LAUNCH("sw_count");
    return SSN_OK;
}

// Filling phase: offsets [V * L + 1] int32 (device) = exclusive prefix sums of the counts, W = their total -> windows
// [W][2] fp64 (device).  A row the tables do not cover is left as it was.
extern "C" int ssn_sw_fill(const int* offsets, int V, const int* h_spans, const int* h_steps, int L, int W, double* windows,
                           hipStream_t stream) {
    SwLevels lv;
    if (int rc = sw_levels(h_spans, h_steps, L, &lv, "sw_fill")) return rc;
    SSN_CHECK_ARG(V >= 1 && (long)V * L < (1L << 30) && W >= 0 && W < (1 << 30), "sw_fill: bad sizes");
    SSN_CHECK_ARG(offsets, "sw_fill: null pointer");
    if (W == 0) return SSN_OK;
    SSN_CHECK_ARG(windows, "sw_fill: null pointer");
    hipLaunchKernelGGL(sw_fill_kernel, dim3((unsigned)((W + 255) / 256)), dim3(256), 0, stream, offsets, V * L, lv, W, windows);
    SSN_CHECK_LAUNCH("sw_fill");
    return SSN_OK;
}

// Frame-number columns of a batch of list records: gt_span [G][2] fp64 ragged by gt_off [V + 1], prop [P][2] fp64 ragged
// by prop_off [V + 1], frame_cnt [V] int32, durations [V] fp64 (all device) -> gt_frames [G][2], frames [P][2] int32 and
// status [V] int32 (zeroed here): bit 0 a ground-truth product, bit 1 a proposal product of the video that is not finite
// or does not fit int32 (0 is written in its place).
extern "C" int ssn_proposal_list_rows(const double* gt_span, const int* gt_off, int G, const double* prop, const int* prop_off,
                                      int P, const int* frame_cnt, const double* durations, int V, int* gt_frames, int* frames,
                                      int* status, hipStream_t stream) {
    SSN_CHECK_ARG(V >= 1 && V < (1 << 30) && G >= 0 && P >= 0 && G < (1 << 30) && P < (1 << 30), "proposal_list_rows: bad sizes");
    SSN_CHECK_ARG(gt_off && prop_off && frame_cnt && durations && status, "proposal_list_rows: null pointer");
    SSN_CHECK_ARG((G == 0 || (gt_span && gt_frames)) && (P == 0 || (prop && frames)), "proposal_list_rows: null pointer");
    if (hipMemsetAsync(status, 0, sizeof(int) * (size_t)V, stream) != hipSuccess) {
        ssn_set_error("proposal_list_rows: memset failed");
        return SSN_ERR_LAUNCH;
    }
    if (G + P == 0) return SSN_OK;
    hipLaunchKernelGGL(pl_rows_kernel, dim3((unsigned)(((long)G + P + 255) / 256)), dim3(256), 0, stream, gt_span, gt_off, G, prop,
                       prop_off, P, frame_cnt, durations, V, gt_frames, frames, status);
    SSN_CHECK_LAUNCH("proposal_list_rows");
    return SSN_OK;
}
