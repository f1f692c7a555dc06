// Detection post-processing of ALL videos of a subset in one pass: the arithmetic of detect.hip (same device helpers,
// detect_common.h, so the results are bit-identical to the per-video call) in a number of launches that does not depend
// on the number of videos, ending in flat, compact detection rows -- what the evaluator (eval.hip) consumes -- instead
// of one padded [C][P][5] block per video.
//   scores    one pass over the rows of all videos                    eval_detection_results.py:91-128
//   select    top-k over the (proposal, class) pairs of each video    :113-128, one workgroup per video
//   nms       temporal NMS, one workgroup per (video, class)          ops/utils.py:56-82
//   offsets   exclusive scan of the kept counts
//   fill      regression and the five columns of every kept row       eval_detection_results.py:167-178
// The videos stand one after the other: video v owns rows p_off[v] ... p_off[v + 1] of act / comp / reg / rel_prop.
#include "detect_common.h"

namespace {

constexpr int DETB_SMALL = 256;   // candidates per class of the small NMS form (one wave, 6.5 KB of LDS)

// rows [p0, p0 + P) of video v; a table entry that cannot be right (the kernels bound what they read from device
// tables) makes the video empty
__device__ __forceinline__ void detb_video(const int* p_off, int v, long total_p, long& p0, int& P) {
    const long a = p_off[v], b = p_off[v + 1];
    const bool ok = a >= 0 && b >= a && b <= total_p;
    p0 = ok ? a : 0;
    P = ok ? (int)(b - a) : 0;
}

// sel[v] = {threshold key, cut lo, cut hi, -} of video v's P_v * C fused scores; flat indices count from the video's
// first pair.  top_k >= P_v * C (or an empty video): the word that keeps everything.
__global__ __launch_bounds__(1024) void detb_topk_kernel(const float* combined, const int* p_off, long total_p, int C, long k,
                                                         uint32_t* sel) {
    const int v = blockIdx.x;
    long p0;
    int P;
    detb_video(p_off, v, total_p, p0, P);
    const long n = (long)P * C;
    uint32_t* out = sel + 4 * (long)v;
    if (k <= 0 || k >= n) {          // (uniform over the workgroup)
        if (threadIdx.x == 0) out[0] = out[1] = out[2] = 0;
        return;
    }
    det_topk_select(combined + p0 * C, n, k, out);
}

struct DetBatchArgs {
    const double* rel_prop;        // [total_p][2]
    const float* combined;         // [total_p][C]
    const int* p_off;              // [V + 1]
    const unsigned char* report;   // [V][C] or nullptr: every class
    const uint32_t* sel;           // [V][4] or nullptr: keep every pair
    const long* big_off;           // [V + 1]: first workspace entry of a video with P > DET_MAXN
    uint32_t* g_key;               // [big_entries] each
    int* g_idx;
    unsigned char* g_supp;
    long big_entries;
    int* kept;                     // [total_p * C]: class c of video v at p_off[v] * C + c * P_v
    int* counts;                   // [V * C]
    long total_p, pairs;           // pairs = V * C
    int C;
    int p_lo, p_hi;                // this launch owns the videos with p_lo <= P_v <= p_hi
    double nms_thresh;
};

// One workgroup per (video, class): det_nms_kernel of detect.hip with the survivors written as proposal indices.
// CAP > 0: candidate arrays of CAP entries in LDS; CAP == 0: in the workspace (pow2(P_v) entries per class).
template <int CAP, int NT>
__global__ __launch_bounds__(NT) void detb_nms_kernel(DetBatchArgs a) {
    constexpr int LN = CAP > 0 ? CAP : 1;
    constexpr bool IN_LDS = CAP > 0;
    __shared__ uint32_t l_key[LN];
    __shared__ int l_idx[LN];
    __shared__ double l_t1[LN], l_t2[LN];
    __shared__ unsigned char l_supp[LN];
    __shared__ int s_n, s_keep;
    const long pair = blockIdx.x;
    const int tid = threadIdx.x;
    if (pair >= a.pairs) return;
    const int v = (int)(pair / a.C), c = (int)(pair - (long)v * a.C);
    long p0;
    int P;
    detb_video(a.p_off, v, a.total_p, p0, P);
    if (P < a.p_lo || P > a.p_hi) return;            // another launch's video
    if (P == 0 || (a.report && !a.report[pair])) {   // nothing to do, or a class the video does not report
        if (tid == 0) a.counts[pair] = 0;
        return;
    }
    int cap = CAP;
    uint32_t* key = l_key;
    int* idx = l_idx;
    unsigned char* supp = l_supp;
    if (!IN_LDS) {
        cap = 1;
        while (cap < P) cap <<= 1;
        const long off = a.big_off[v] + (long)c * cap;
        if (a.big_off[v] < 0 || off + cap > a.big_entries) {      // a table that does not fit the workspace
            if (tid == 0) a.counts[pair] = 0;
            return;
        }
        key = a.g_key + off;
        idx = a.g_idx + off;
        supp = a.g_supp + off;
    }
    const double* rel = a.rel_prop + 2 * p0;
    const float* comb = a.combined + p0 * a.C;
    uint32_t thr = 0;
    long cut = 0;
    if (a.sel) {
        const uint32_t* s = a.sel + 4 * (long)v;
        thr = s[0];
        cut = (long)(((unsigned long)s[2] << 32) | s[1]);
    }
    if (tid == 0) {
        s_n = 0;
        s_keep = 0;
    }
    __syncthreads();
    // candidates of this class, in any order (the sort's order is total)
    for (int p = tid; p < P; p += NT) {
        const long flat = (long)p * a.C + c;
        const uint32_t kk = det_key(comb[flat]);
        if (det_selected(kk, flat, thr, cut)) {
            const int slot = atomicAdd(&s_n, 1);
            if (slot < cap) {
                key[slot] = kk;
                idx[slot] = p;
            }
        }
    }
    __syncthreads();
    int n = s_n;
    if (n > cap) n = cap;             // cannot happen: cap >= P_v (the launch's p_hi, or pow2(P_v))
    int n2 = 1;
    while (n2 < n) n2 <<= 1;
    for (int i = n + tid; i < n2; i += NT) {
        key[i] = 0;                   // below every real key, and behind every real entry on a key tie (detect.hip)
        idx[i] = -1;
    }
    __syncthreads();
    for (int k = 2; k <= n2; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = tid; i < n2; i += NT) {
                const int l = i ^ j;
                if (l > i) {
                    const bool desc = (i & k) == 0;
                    const uint32_t ki = key[i], kl = key[l];
                    const int ii = idx[i], il = idx[l];
                    if (desc != det_before(ki, ii, kl, il)) {
                        key[i] = kl;
                        key[l] = ki;
                        idx[i] = il;
                        idx[l] = ii;
                    }
                }
            }
            __syncthreads();
        }
    for (int i = tid; i < n; i += NT) {
        int p = idx[i];
        if (p < 0 || p >= P) p = 0;            // defensive: never index outside the video's proposals
        if (IN_LDS) {
            l_t1[i] = rel[2 * (long)p];
            l_t2[i] = rel[2 * (long)p + 1];
        }
        idx[i] = p;
        supp[i] = 0;
    }
    __syncthreads();
    // greedy NMS in score order; a barrier is only needed behind a box that survives (detect.hip)
    int* kept = a.kept + p0 * a.C + (long)c * P;
    for (int i = 0; i < n; ++i) {
        if (supp[i]) continue;       // uniform: supp[i] was settled before the last barrier
        const int pi = idx[i];
        const double a1 = IN_LDS ? l_t1[i] : rel[2 * (long)pi];
        const double a2 = IN_LDS ? l_t2[i] : rel[2 * (long)pi + 1];
        for (int j = i + 1 + tid; j < n; j += NT) {
            const double b1 = IN_LDS ? l_t1[j] : rel[2 * (long)idx[j]];
            const double b2 = IN_LDS ? l_t2[j] : rel[2 * (long)idx[j] + 1];
            if (det_suppresses(a1, a2, b1, b2, a.nms_thresh)) supp[j] = 1;
        }
        if (tid == 0) {
            const int o = s_keep++;
            if (o < P) kept[o] = pi;
        }
        __syncthreads();
    }
    if (tid == 0) a.counts[pair] = s_keep < P ? s_keep : P;
}

// row_off [n + 1] = exclusive prefix sums of counts [n], one workgroup, tiles of 1024 x 16 entries: every thread sums 16
// contiguous entries, the wave scans its 64 sums by shuffles, the 16 wave totals go through LDS, and the running base
// moves on to the next tile (two barriers per tile).
constexpr int DETB_SCAN_ITEMS = 16;
typedef int detb_i4 __attribute__((ext_vector_type(4)));

__global__ __launch_bounds__(1024) void detb_scan_kernel(const int* counts, long n, int* row_off) {
    __shared__ int wave_tot[16];
    __shared__ int s_base;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const bool aligned = ((uintptr_t)counts & 15) == 0;
    if (tid == 0) s_base = 0;
    __syncthreads();
    for (long t0 = 0; t0 < n; t0 += 1024L * DETB_SCAN_ITEMS) {
        const long b = t0 + (long)tid * DETB_SCAN_ITEMS;
        int x[DETB_SCAN_ITEMS];
        if (aligned && b + DETB_SCAN_ITEMS <= n) {
#pragma unroll
            for (int j = 0; j < DETB_SCAN_ITEMS; j += 4) {
                const detb_i4 q = *(const detb_i4*)(counts + b + j);
                x[j] = q[0];
                x[j + 1] = q[1];
                x[j + 2] = q[2];
                x[j + 3] = q[3];
            }
        } else {
#pragma unroll
            for (int j = 0; j < DETB_SCAN_ITEMS; ++j) x[j] = b + j < n ? counts[b + j] : 0;
        }
        int sum = 0;
#pragma unroll
        for (int j = 0; j < DETB_SCAN_ITEMS; ++j) sum += x[j];
        int incl = sum;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const int y = __shfl(incl, lane >= off ? lane - off : lane, 64);      // (every lane takes part)
            if (lane >= off) incl += y;
        }
        if (lane == 63) wave_tot[w] = incl;
        __syncthreads();
        int run = s_base + incl - sum;
        for (int k = 0; k < w; ++k) run += wave_tot[k];
#pragma unroll
        for (int j = 0; j < DETB_SCAN_ITEMS; ++j) {
            if (b + j < n) row_off[b + j] = run;
            run += x[j];
        }
        __syncthreads();
        if (tid == 1023) s_base = run;      // (read again only behind the next tile's first barrier)
    }
    __syncthreads();
    if (tid == 0) row_off[n] = s_base;
}

// One lane per output row r: its (video, class) pair is the last one whose offset is <= r; its proposal is the
// (r - offset)-th survivor of that pair.
__global__ __launch_bounds__(256) void detb_fill_kernel(const double* rel_prop, const float* combined, const float* reg,
                                                        const int* p_off, const int* kept, const int* row_off, long pairs, int C,
                                                        long total_p, long N, int regress, double* rows, int* cls, int* vid,
                                                        int* prop) {
    const long r = (long)blockIdx.x * 256 + threadIdx.x;
    if (r >= N) return;
    long lo = 0, hi = pairs;          // row_off[lo] <= r (row_off[0] = 0); every pair from hi on starts behind r
    while (hi - lo > 1) {
        const long mid = (lo + hi) >> 1;
        if ((long)row_off[mid] <= r) lo = mid;
        else hi = mid;
    }
    const int v = (int)(lo / C), c = (int)(lo - (long)v * C);
    const long o = r - row_off[lo];
    long p0;
    int P;
    detb_video(p_off, v, total_p, p0, P);
    int pi = -1;
    if (o >= 0 && o < P && r < (long)row_off[lo + 1]) pi = kept[p0 * C + (long)c * P + o];
    double* d = rows + r * 5;
    if (pi < 0 || pi >= P) {          // N or a table that does not belong to these counts: an all-zero row, no access
        d[0] = d[1] = d[2] = d[3] = d[4] = 0.0;
        cls[r] = vid[r] = prop[r] = 0;
        return;
    }
    const long q = p0 + pi;
    det_write_row(d, rel_prop[2 * q], rel_prop[2 * q + 1], combined, reg, q * C + c, regress);
    cls[r] = c;
    vid[r] = v;
    prop[r] = pi;
}

inline size_t detb_round16(size_t b) { return (b + 15) & ~(size_t)15; }

}  // namespace

// Device scratch of ssn_detections_batch: one selection word per video, plus key / index / flag arrays of big_entries
// entries, big_entries = sum over the videos with P_v > 2048 of C * pow2(P_v).
extern "C" size_t ssn_detections_batch_workspace_bytes(int V, long big_entries) {
    if (V < 0 || big_entries < 0) return 0;
    return detb_round16((size_t)V * 16) + detb_round16((size_t)big_entries * 4) * 2 + detb_round16((size_t)big_entries);
}

// Stages scores, select, nms, offsets.  act [total_p][C+1], comp [total_p][C] fp32, rel_prop [total_p][2] fp64, p_off
// [V + 1] int32 (a host copy that is validated here, and the device copy the kernels read), report [V][C] uint8 or NULL,
// big_off [V + 1] int64 (device): first workspace entry of every video with P_v > 2048 (exclusive prefix sums of C *
// pow2(P_v) over those videos, 0 for the others), big_entries its last entry.  Out: combined [total_p][C] fp32, kept
// [total_p * C] int32, counts [V * C] int32, row_off [V * C + 1] int32.  include_bg and top_k as in ssn_detections.
extern "C" int ssn_detections_batch(const float* act, const float* comp, const double* rel_prop, const int* h_p_off,
                                    const int* d_p_off, const unsigned char* report, const long* big_off, long big_entries, int V,
                                    int C, int top_k, int include_bg, double nms_thresh, float* combined, int* kept, int* counts,
                                    int* row_off, void* workspace, size_t ws_bytes, hipStream_t stream) {
    SSN_CHECK_ARG(V >= 1 && C >= 1, "detections_batch: bad sizes");
    SSN_CHECK_ARG(h_p_off && d_p_off && big_off && counts && row_off && workspace, "detections_batch: null pointer");
    SSN_CHECK_ARG(h_p_off[0] == 0, "detections_batch: offsets must start at 0");
    SSN_CHECK_ARG((long)V * C < (1L << 31), "detections_batch: %d videos x %d classes do not fit int32, split the batch", V, C);
    bool small = false, mid = false, big = false;
    long want_big = 0;
    for (int v = 0; v < V; ++v) {
        const long p = (long)h_p_off[v + 1] - h_p_off[v];
        SSN_CHECK_ARG(p >= 0, "detections_batch: offsets must not decrease (video %d)", v);
        if (p <= DETB_SMALL) {
            small = true;
        } else if (p <= DET_MAXN) {
            mid = true;
        } else {
            big = true;
            want_big += (long)C * det_pow2((int)p);
        }
    }
    const long total_p = h_p_off[V];
    SSN_CHECK_ARG(total_p * C < (1L << 31), "detections_batch: %ld proposals x %d classes do not fit int32, split the batch",
                  total_p, C);
    SSN_CHECK_ARG(big_entries == want_big, "detections_batch: big_entries is %ld, the offsets give %ld", big_entries, want_big);
    SSN_CHECK_ARG(total_p == 0 || (act && comp && rel_prop && combined && kept), "detections_batch: null pointer");
    if (ws_bytes < ssn_detections_batch_workspace_bytes(V, big_entries)) {
        ssn_set_error("detections_batch: workspace of %zu bytes, %zu needed", ws_bytes,
                      ssn_detections_batch_workspace_bytes(V, big_entries));
        return SSN_ERR_WORKSPACE;
    }
    const long pairs = (long)V * C;
    if (total_p > 0)
        hipLaunchKernelGGL(det_scores_kernel, dim3((unsigned)((total_p + 3) / 4)), dim3(256), 0, stream, act, comp, combined,
                           (int)total_p, C, include_bg);
    char* w = (char*)workspace;
    uint32_t* sel = (uint32_t*)w;
    w += detb_round16((size_t)V * 16);
    if (top_k > 0)
        hipLaunchKernelGGL(detb_topk_kernel, dim3((unsigned)V), dim3(1024), 0, stream, (const float*)combined, d_p_off, total_p, C,
                           (long)top_k, sel);
    DetBatchArgs a;
    a.rel_prop = rel_prop;
    a.combined = combined;
    a.p_off = d_p_off;
    a.report = report;
    a.sel = top_k > 0 ? sel : nullptr;
    a.big_off = big_off;
    a.g_key = (uint32_t*)w;
    a.g_idx = (int*)(w + detb_round16((size_t)big_entries * 4));
    a.g_supp = (unsigned char*)(w + 2 * detb_round16((size_t)big_entries * 4));
    a.big_entries = big_entries;
    a.kept = kept;
    a.counts = counts;
    a.total_p = total_p;
    a.pairs = pairs;
    a.C = C;
    a.nms_thresh = nms_thresh;
    // every (video, class) pair belongs to exactly one of up to three launches, by the size of its video alone; a launch
    // whose size class no video of the batch has is left out
    const dim3 grid((unsigned)pairs);
    if (small) {
        a.p_lo = 0;
        a.p_hi = DETB_SMALL;
        hipLaunchKernelGGL((detb_nms_kernel<DETB_SMALL, 64>), grid, dim3(64), 0, stream, a);
    }
    if (mid) {
        a.p_lo = DETB_SMALL + 1;
        a.p_hi = DET_MAXN;
        hipLaunchKernelGGL((detb_nms_kernel<DET_MAXN, 256>), grid, dim3(256), 0, stream, a);
    }
    if (big) {
        a.p_lo = DET_MAXN + 1;
        a.p_hi = 0x7fffffff;
        hipLaunchKernelGGL((detb_nms_kernel<0, 256>), grid, dim3(256), 0, stream, a);
    }
    hipLaunchKernelGGL(detb_scan_kernel, dim3(1), dim3(1024), 0, stream, (const int*)counts, pairs, row_off);
    SSN_CHECK_LAUNCH("detections_batch");
    return SSN_OK;
}

// Stage fill, after the caller has read N = row_off[V * C] (the one sizing read).  reg [total_p][C][2] fp32 or NULL; regress 0
// keeps the proposals' own spans.  rows [N][5] fp64 = (start, end, score, loc, dur) -- the values ssn_detections writes
// into dets -- and cls / vid / prop [N] int32, in the order video, class, kept order (descending score).
extern "C" int ssn_detections_batch_fill(const double* rel_prop, const float* combined, const float* reg, const int* p_off,
                                         const int* kept, const int* row_off, int V, int C, long total_p, long N, int regress,
                                         double* rows, int* cls, int* vid, int* prop, hipStream_t stream) {
    SSN_CHECK_ARG(V >= 1 && C >= 1 && total_p >= 0 && N >= 0, "detections_batch_fill: bad sizes");
    SSN_CHECK_ARG(total_p * C < (1L << 31) && (long)V * C < (1L << 31),
                  "detections_batch_fill: sizes do not fit int32, split the batch");
    SSN_CHECK_ARG(N <= total_p * C, "detections_batch_fill: %ld rows from %ld pairs", N, total_p * C);
    if (N == 0) return SSN_OK;
    SSN_CHECK_ARG(rel_prop && combined && p_off && kept && row_off && rows && cls && vid && prop,
                  "detections_batch_fill: null pointer");
    hipLaunchKernelGGL(detb_fill_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, stream, rel_prop, combined, reg, p_off,
                       kept, row_off, (long)V * C, C, total_p, N, regress, rows, cls, vid, prop);
    SSN_CHECK_LAUNCH("detections_batch_fill");
    return SSN_OK;
}
