// Proposal evaluation for a whole subset on the GPU: average recall against the average number of proposals per video
// (AR-AN), its area under the curve and recall against tIoU -- the measure of the TAG / SSN papers and of the ActivityNet
// proposal task (the toolkit's average_recall_vs_avg_nr_proposals; the toolkit is a submodule that is empty in the
// reference tree, the algorithm is restated in DESIGN.md and in tests/proposal_eval_referee.py).
// Ground truth and proposals of all videos come flat and ragged, as for ssn_eval_recall; the proposals of a video are in
// rank order, or `order` says so.  Passes: (rank by score: keys + per-video sort) -> first hit per (ground truth, threshold),
// one wave per ground-truth row, which also drops the hit into the histogram of curve points -> prefix sums, recall,
// average recall, proposals per video and the area, one workgroup.  Launches do not depend on the number of videos.
// What is exact: the tIoU is fp64 `inter / ((ge - gs) + (e - s) - inter)` in that order, as in eval.hip; the curve point
// of a hit comes from the host's own expression `min(int(nr * pcn[j]), nr)` in fp64; counts are integers; a recall is one
// fp64 division of integers; proposals_per_video is one fp64 product.  Only the sums of avg_recall and auc are this file's.
#include "eval_common.h"

#pragma clang fp contract(off)

namespace {

constexpr int PEVAL_MAX_J = 4096;      // curve points per call

// keys of the per-video sort: entry k of video v's pow2 range is its k-th proposal (the key holds the flat index, so
// the sorted order is that of (descending score, lower flat index) whatever the slot)
__global__ __launch_bounds__(256) void peval_fill_kernel(const double* score, const int* prop_off, int P, int V,
                                                         const long* sort_off, long sort_entries, u64* hi, u64* lo) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= P) return;
    const int v = eval_find(prop_off, V, i);
    const long sb = sort_off[v], se = sort_off[v + 1];
    const int k = i - prop_off[v];
    if (sb < 0 || se > sort_entries || k < 0 || sb + k >= se) return;      // tables disagree: drop the row
    hi[sb + k] = ~eval_key(score[i]);                                      // ascending ~key = descending score
    lo[sb + k] = ((u64)(uint32_t)i << 32) | (uint32_t)v;
}

// the number of proposals video v shows at curve point j: min(int(nr * pcn[j]), nr), the product in fp64
__device__ __forceinline__ int peval_shown(int nr, double pcn) {
    const double x = (double)nr * pcn;
    return x >= (double)nr ? nr : (x > 0.0 ? (int)x : 0);
}

struct PevalArgs {
    const double* gt;          // [G][2]
    const int* gt_off;         // [V + 1]
    const double* prop;        // [P][2]
    const int* prop_off;       // [V + 1]
    const int* nr;             // [V]: proposals of the video that exist after the truncation
    const int* order;          // [P] or null: rank r of video v is row order[prop_off[v] + r]
    const double* thr;         // [T]
    const double* pcn;         // [J]
    int* first_hit;            // [G][T]
    int* hist;                 // [T][J], zeroed
    int G, P, V, T, J;
};

// One wave per ground-truth row.  The lanes take 64 consecutive ranks; each computes its tIoU once and leaves the
// thresholds it reaches as a bit mask in LDS.  Every lane then walks the 64 masks in rank order: lane t keeps the first
// rank that reaches threshold t, and all lanes keep the union, so that the wave leaves -- uniformly -- after the first
// chunk that settles every threshold.  Lane t then finds the first curve point that shows its rank and counts there.
__global__ __launch_bounds__(64) void peval_first_hit_kernel(PevalArgs a) {
    __shared__ unsigned s_mask[64];
    const int lane = threadIdx.x, g = blockIdx.x;
    const int v = eval_find(a.gt_off, a.V, g);
    int p0 = a.prop_off[v], m = a.prop_off[v + 1] - p0;
    if (p0 < 0 || m < 0 || (long)p0 + m > a.P) m = 0;
    int n = a.nr[v];
    n = n < m ? n : m;
    const double gs = a.gt[2 * (long)g], ge = a.gt[2 * (long)g + 1];
    const unsigned full = a.T >= 32 ? 0xffffffffu : ((1u << a.T) - 1u);
    unsigned seen = 0;
    int fh = -1;
    for (int base = 0; base < n && seen != full; base += 64) {
        unsigned mask = 0;
        const int r = base + lane;
        if (r < n) {
            const int p = a.order ? a.order[p0 + r] : p0 + r;
            if (p >= 0 && p < a.P) {
                const double s = a.prop[2 * (long)p], e = a.prop[2 * (long)p + 1];
                const double inter = fmax(0.0, fmin(e, ge) - fmax(s, gs));
                const double uni = (ge - gs) + (e - s) - inter;
                const double iou = inter / uni;
                for (int t = 0; t < a.T; ++t)
                    if (iou >= a.thr[t]) mask |= 1u << t;
            }
        }
        s_mask[lane] = mask;
        __syncthreads();
        for (int l = 0; l < 64; ++l) {
            const unsigned ml = s_mask[l];
            if (fh < 0 && ((ml >> (lane & 31)) & 1u)) fh = base + l;
            seen |= ml;
        }
        __syncthreads();
    }
    if (lane >= a.T) return;
    a.first_hit[(long)g * a.T + lane] = fh;
    if (fh < 0) return;
    // k(j) = peval_shown(n, pcn[j]) does not decrease with j: the smallest j with k(j) > fh
    int lo = 0, hi = a.J;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (peval_shown(n, a.pcn[mid]) > fh) hi = mid;
        else lo = mid + 1;
    }
    if (lo < a.J) atomicAdd(&a.hist[(long)lane * a.J + lo], 1);
}

// inclusive scan over the 64 lanes of a wave
__device__ __forceinline__ int peval_wave_scan(int v, int lane) {
    for (int d = 1; d < 64; d <<= 1) {
        const int o = __shfl(v, lane >= d ? lane - d : lane, 64);
        if (lane >= d) v += o;
    }
    return v;
}

// One workgroup.  hist [T][J] -> matches in place (prefix sums over j, one wave per row), then per curve point the
// recalls, their mean over the thresholds and the proposals per video; the trapezoid terms are summed per thread and
// the 256 partial sums in thread order.  out: recall [T][J], avg_recall [J], proposals_per_video [J], auc [1].
__global__ __launch_bounds__(256) void peval_finish_kernel(int* hist, const double* pcn, int T, int J, int positives,
                                                           double per_video, double* out) {
    __shared__ double s_acc[256];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    for (int t = w; t < T; t += 4) {
        int* row = hist + (long)t * J;
        int carry = 0;
        for (int base = 0; base < J; base += 64) {
            const int j = base + lane;
            const int incl = peval_wave_scan(j < J ? row[j] : 0, lane);
            if (j < J) row[j] = carry + incl;
            carry += __shfl(incl, 63, 64);
        }
    }
    __syncthreads();
    double* recall = out;
    double* avg = out + (long)T * J;
    double* ppv = avg + J;
    for (int j = tid; j < J; j += 256) {
        double sum = 0.0;
        for (int t = 0; t < T; ++t) {
            const double r = (double)hist[(long)t * J + j] / (double)positives;
            recall[(long)t * J + j] = r;
            sum += r;
        }
        avg[j] = sum / (double)T;
        ppv[j] = pcn[j] * per_video;
    }
    __syncthreads();
    double acc = 0.0;
    for (int j = tid; j + 1 < J; j += 256) acc += (ppv[j + 1] - ppv[j]) * (avg[j + 1] + avg[j]) / 2.0;
    s_acc[tid] = acc;
    __syncthreads();
    if (tid == 0) {
        double sum = 0.0;
        for (int i = 0; i < 256; ++i) sum += s_acc[i];
        out[(long)T * J + 2 * (long)J] = sum / ppv[J - 1];
    }
}

}  // namespace

// The largest number of curve points (J) of one call.
extern "C" int ssn_proposal_eval_max_points(void) { return PEVAL_MAX_J; }

// Device scratch of ssn_proposal_eval_rank: 16 bytes per sort entry.
extern "C" size_t ssn_proposal_eval_workspace_bytes(long sort_entries) {
    return sort_entries < 0 ? 0 : 16 + 16 * (size_t)sort_entries;
}

// Rank the proposals of every video by score: score [P] fp64 (finite; the caller checks), prop_off [V + 1] int32,
// sort_off [V + 1] int64 = exclusive prefix sums of the videos' proposal counts rounded up to a power of two (0 stays 0).
// -> order [P] int32: the flat indices video by video in descending score, equal scores lower index first.
extern "C" int ssn_proposal_eval_rank(const double* score, const int* prop_off, int P, int V, const long* sort_off,
                                      long sort_entries, int* order, void* workspace, size_t ws_bytes, hipStream_t stream) {
    SSN_CHECK_ARG(V >= 1 && P >= 0 && sort_entries >= P && sort_entries < (1L << 31), "proposal_eval_rank: bad sizes");
    SSN_CHECK_ARG(prop_off && sort_off && workspace, "proposal_eval_rank: null pointer");
    SSN_CHECK_ARG(P == 0 || (score && order), "proposal_eval_rank: null pointer");
    if (ws_bytes < ssn_proposal_eval_workspace_bytes(sort_entries)) {
        ssn_set_error("proposal_eval_rank: workspace of %zu bytes, %zu needed", ws_bytes,
                      ssn_proposal_eval_workspace_bytes(sort_entries));
        return SSN_ERR_WORKSPACE;
    }
    if (P == 0) return SSN_OK;
    u64* hi = (u64*)workspace;
    u64* lo = hi + sort_entries;
    if (hipMemsetAsync(hi, 0xff, 16 * (size_t)sort_entries, stream) != hipSuccess) {
        ssn_set_error("proposal_eval_rank: memset failed");
        return SSN_ERR_LAUNCH;
    }
    hipLaunchKernelGGL(peval_fill_kernel, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, stream, score, prop_off, P, V, sort_off,
                       sort_entries, hi, lo);
    hipLaunchKernelGGL(eval_sort_kernel, dim3((unsigned)V), dim3(256), 0, stream, hi, lo, sort_off, sort_entries, prop_off, P,
                       order);
    SSN_CHECK_LAUNCH("proposal_eval_rank");
    return SSN_OK;
}

// AR-AN of a batch.  gt_span [G][2] fp64 ragged by gt_off [V + 1], prop [P][2] fp64 ragged by prop_off [V + 1] (both
// int32), nr [V] int32 (proposals of each video that exist after the truncation; 0 for a video without ground truth),
// thresholds [T] fp64 (T <= 32), pcn [J] fp64 ascending (J <= ssn_proposal_eval_max_points()), order [P] int32 or null
// (null: the rows of a video are in rank order).  per_video = double(sum nr) / counted videos.  Out: first_hit [G][T]
// int32 (the smallest rank < nr whose tIoU with the row is >= the threshold, -1: none), matches [T][J] int32,
// curves [T * J + 2 J + 1] fp64 = recall [T][J], avg_recall [J], proposals_per_video [J], auc.  All pointers device memory.
extern "C" int ssn_proposal_eval_ar_an(const double* gt_span, const int* gt_off, int G, const double* prop, const int* prop_off,
                                       int P, int V, const int* nr, const int* order, const double* thresholds, int T,
                                       const double* pcn, int J, double per_video, int* first_hit, int* matches, double* curves,
                                       hipStream_t stream) {
    SSN_CHECK_ARG(T >= 1 && T <= EVAL_MAX_T, "proposal_eval_ar_an: %d thresholds, at most %d in one call", T, EVAL_MAX_T);
    SSN_CHECK_ARG(J >= 1 && J <= PEVAL_MAX_J, "proposal_eval_ar_an: %d curve points, at most %d in one call", J, PEVAL_MAX_J);
    SSN_CHECK_ARG(V >= 1 && G >= 1 && P >= 0 && (long)G * T < (1L << 31), "proposal_eval_ar_an: bad sizes");
    SSN_CHECK_ARG(gt_span && gt_off && prop_off && nr && thresholds && pcn && first_hit && matches && curves,
                  "proposal_eval_ar_an: null pointer");
    SSN_CHECK_ARG(P == 0 || prop, "proposal_eval_ar_an: null pointer");
    if (hipMemsetAsync(matches, 0, sizeof(int) * (size_t)T * (size_t)J, stream) != hipSuccess) {
        ssn_set_error("proposal_eval_ar_an: memset failed");
        return SSN_ERR_LAUNCH;
    }
    PevalArgs a;
    a.gt = gt_span;
    a.gt_off = gt_off;
    a.prop = prop;
    a.prop_off = prop_off;
    a.nr = nr;
    a.order = order;
    a.thr = thresholds;
    a.pcn = pcn;
    a.first_hit = first_hit;
    a.hist = matches;
    a.G = G;
    a.P = P;
    a.V = V;
    a.T = T;
    a.J = J;
    hipLaunchKernelGGL(peval_first_hit_kernel, dim3((unsigned)G), dim3(64), 0, stream, a);
    hipLaunchKernelGGL(peval_finish_kernel, dim3(1), dim3(256), 0, stream, matches, pcn, T, J, G, per_video, curves);
    SSN_CHECK_LAUNCH("proposal_eval_ar_an");
    return SSN_OK;
}
