// Detection evaluation for a whole dataset on the GPU: the last stage of the reference's evaluation script
//   average precision per (class, tIoU threshold)      /root/reference/eval_detection_results.py:188-237 (the ActivityNet
//                                                       toolkit's compute_average_precision_detection, restated in DESIGN.md)
//   proposal recall                                     /root/reference/ops/detection_metrics.py:7-51 (temporal_iou, temporal_recall)
// which the reference runs as pandas loops in a pool of 32 processes.  Predictions of all classes and videos come flat
// ([N] start / end / score fp64, class / video int32); every kernel covers the whole dataset, so launches per call do not
// depend on the number of classes or videos.  Passes: scatter into per-class segments + sort by (score descending, flat
// index) -> greedy matching, one wave per (class, video) group that has ground truth -> scan / running maximum / sum per
// (class, threshold).  What is exact: the IoU is fp64 `inter / ((ge - gs) + (e - s) - inter)` in that order (no multiply,
// nothing to contract; IEEE subtraction and division round as numpy's do), so the tp flags are numpy's; cumulative
// counts are integers; a precision is one fp64 division of integers.  Only the final sum's order is this file's own.
#include "eval_common.h"

#pragma clang fp contract(off)

namespace {

constexpr int EVAL_LDS_GT = 256;       // ground-truth rows of one (class, video) group matched out of LDS; more take the workspace
// (EVAL_SORT_LDS, EVAL_MAX_T, the score key, the offset search and the segment sort: eval_common.h)

// rows per class; counts[C] = rows that cannot be evaluated (class out of range or score not finite)
__global__ __launch_bounds__(256) void eval_count_kernel(const double* score, const int* cls, int n, int C, int* counts) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int c = cls[i];
    const bool ok = c >= 0 && c < C && eval_finite(score[i]);
    atomicAdd(&counts[ok ? c : C], 1);
}

// scatter into the class segments of the sort buffer.  The slot inside the segment is whatever the atomic hands out:
// the key holds the flat index, so the sorted order does not depend on it.
__global__ __launch_bounds__(256) void eval_fill_kernel(const double* score, const int* cls, const int* vid, int n, int C,
                                                        const long* sort_off, long sort_entries, int* cursor, u64* hi, u64* lo) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int c = cls[i];
    if (c < 0 || c >= C) return;
    const long sb = sort_off[c], se = sort_off[c + 1];
    const int k = atomicAdd(&cursor[c], 1);
    if (sb < 0 || se > sort_entries || k < 0 || sb + k >= se) return;      // tables and rows disagree: drop the row
    hi[sb + k] = ~eval_key(score[i]);                                      // ascending ~key = descending score
    lo[sb + k] = ((u64)(uint32_t)i << 32) | (uint32_t)vid[i];
}

struct EvalMatchArgs {
    const double* pred_seg;    // [N][2]
    const u64* lo;             // sorted entries: flat index << 32 | video
    const double* gt_seg;      // [G][2], the rows of one group next to each other
    const int* groups;         // [NG][5]: class, video, first row, rows, offset into `big` (8-byte units; LDS groups: unused)
    const double* thr;         // [T]
    const int* pred_off;       // [C + 1]
    const long* sort_off;      // [C + 1]
    double* big;               // per group above EVAL_LDS_GT: rows fp64 IoUs, then 32 * ceil(rows / 64) lock words
    unsigned char* tp;         // [T][N], zeroed
    int N, G, T, C;
    long sort_entries, big_units;
};

// Greedy matching, one wave per (class, video) group with ground truth.  The wave walks its class's sorted segment in
// chunks of 64; the entries of its video are visited in order.  Per prediction: lanes compute the IoUs with the
// group's rows, then lane t < T takes for threshold t the FREE row of highest IoU (first on ties) and, if that IoU is
// at least the threshold, locks it and sets tp -- the same outcome as the toolkit's walk over the rows by descending
// IoU that stops below the threshold and skips locked rows.
template <bool IN_LDS>
__global__ __launch_bounds__(64) void eval_match_kernel(EvalMatchArgs a) {
    constexpr int LN = IN_LDS ? EVAL_LDS_GT : 1;
    __shared__ double l_g[2 * LN], l_iou[LN];
    __shared__ u64 l_lock[EVAL_MAX_T * ((LN + 63) / 64)];
    __shared__ int s_mask[2], s_idx[64];
    const int lane = threadIdx.x;
    const int* gr = a.groups + 5 * (long)blockIdx.x;
    const int c = gr[0], v = gr[1], g0 = gr[2], ng = gr[3];
    if (c < 0 || c >= a.C || ng < 1 || g0 < 0 || (long)g0 + ng > a.G || (ng <= EVAL_LDS_GT) != IN_LDS) return;
    const int words = (ng + 63) >> 6;
    const double* gp = a.gt_seg + 2 * (long)g0;
    double* iou = l_iou;
    u64* lock = l_lock;
    if (!IN_LDS) {
        const long boff = gr[4];
        if (boff < 0 || boff + ng + (long)EVAL_MAX_T * words > a.big_units) return;
        iou = a.big + boff;
        lock = reinterpret_cast<u64*>(a.big + boff + ng);
    } else {
        for (int i = lane; i < 2 * ng; i += 64) l_g[i] = gp[i];
        gp = l_g;
    }
    for (int i = lane; i < EVAL_MAX_T * words; i += 64) lock[i] = 0;
    const long sb = a.sort_off[c];
    const int pb = a.pred_off[c], n = a.pred_off[c + 1] - pb;
    if (sb < 0 || n < 0 || sb + n > a.sort_entries || pb < 0 || (long)pb + n > a.N) return;
    const double th = lane < a.T ? a.thr[lane] : 0.0;
    u64* my_lock = lock + (lane < a.T ? lane : 0) * (long)words;
    for (int base = 0; base < n; base += 64) {
        if (lane < 2) s_mask[lane] = 0;
        __syncthreads();
        if (base + lane < n) {
            const u64 e = a.lo[sb + base + lane];
            const uint32_t idx = (uint32_t)(e >> 32);
            if ((int)(uint32_t)e == v && idx < (uint32_t)a.N) {
                s_idx[lane] = (int)idx;
                atomicOr(&s_mask[lane >> 5], (int)(1u << (lane & 31)));
            }
        }
        __syncthreads();
        u64 m = (u64)(uint32_t)s_mask[0] | ((u64)(uint32_t)s_mask[1] << 32);      // (uniform)
        while (m) {
            const int j = __builtin_ctzll(m);
            m &= m - 1;
            const long p = s_idx[j];
            const double s = a.pred_seg[2 * p], e = a.pred_seg[2 * p + 1];
            for (int g = lane; g < ng; g += 64) {
                const double gs = gp[2 * g], ge = gp[2 * g + 1];
                const double inter = fmax(0.0, fmin(e, ge) - fmax(s, gs));
                const double uni = (ge - gs) + (e - s) - inter;
                iou[g] = inter / uni;
            }
            __syncthreads();
            if (lane < a.T) {
                double best = -1.0;
                int bi = -1;
                for (int w = 0; w < words; ++w) {
                    const u64 taken = my_lock[w];
                    const int gend = ng - 64 * w < 64 ? ng - 64 * w : 64;
                    for (int b = 0; b < gend; ++b) {
                        const double x = iou[64 * w + b];
                        if (!((taken >> b) & 1) && x > best) {
                            best = x;
                            bi = 64 * w + b;
                        }
                    }
                }
                if (bi >= 0 && best >= th) {
                    my_lock[bi >> 6] |= 1ull << (bi & 63);
                    a.tp[(long)lane * a.N + pb + base + j] = 1;
                }
            }
            __syncthreads();
        }
    }
}

// inclusive scans over the 256 threads of the workgroup (+ the value of the last thread)
__device__ __forceinline__ int eval_scan_sum(int v, int* s_wave, int& total) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    for (int d = 1; d < 64; d <<= 1) {
        const int o = __shfl(v, lane >= d ? lane - d : lane, 64);
        if (lane >= d) v += o;
    }
    __syncthreads();
    if (lane == 63) s_wave[w] = v;
    __syncthreads();
    total = 0;
    for (int j = 0; j < 4; ++j) {
        if (j < w) v += s_wave[j];
        total += s_wave[j];
    }
    return v;
}

__device__ __forceinline__ double eval_shfl(double x, int src) {
    const u64 b = __builtin_bit_cast(u64, x);
    const uint32_t lo = (uint32_t)__shfl((int)(uint32_t)b, src, 64), hi = (uint32_t)__shfl((int)(b >> 32), src, 64);
    return __builtin_bit_cast(double, ((u64)hi << 32) | lo);
}

__device__ __forceinline__ double eval_scan_max(double v, double* s_wave, double& total) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    for (int d = 1; d < 64; d <<= 1) {
        const double o = eval_shfl(v, lane >= d ? lane - d : lane);
        if (lane >= d) v = fmax(v, o);
    }
    __syncthreads();
    if (lane == 63) s_wave[w] = v;
    __syncthreads();
    total = 0.0;
    for (int j = 0; j < 4; ++j) {
        if (j < w) v = fmax(v, s_wave[j]);
        total = fmax(total, s_wave[j]);
    }
    return v;
}

// One workgroup per (class, threshold).  tp flags of the class in score order -> total, then ONE pass from the end:
// cumulative tp at position i = total - (tp behind i), precision = cum / (i + 1), its running maximum from the end
// (the toolkit's "make precision non-increasing"), summed at the true positives; AP = sum / npos (0 / 0 = NaN for a
// class without ground truth).  Each thread sums its own positions, the 256 partial sums are added in thread order.
__global__ __launch_bounds__(256) void eval_ap_kernel(const unsigned char* tp, const int* pred_off, const int* npos, int N,
                                                      int T, double* ap) {
    __shared__ int s_i[4];
    __shared__ double s_d[4], s_acc[256];
    const int c = blockIdx.x / T, t = blockIdx.x - c * T, tid = threadIdx.x;
    const int pb = pred_off[c];
    int n = pred_off[c + 1] - pb;
    if (pb < 0 || n < 0 || (long)pb + n > N) n = 0;
    const unsigned char* f = tp + (long)t * N + pb;
    int cnt = 0, total;
    for (int i = tid; i < n; i += 256) cnt += f[i];
    eval_scan_sum(cnt, s_i, total);
    int behind = 0;
    double tail_max = 0.0, acc = 0.0;
    for (int end = n; end > 0; end -= 256) {
        const int i = end - 1 - tid;               // thread 0 takes the last position of the chunk
        const int fi = i >= 0 ? f[i] : 0;
        int chunk_tp;
        const int incl = eval_scan_sum(fi, s_i, chunk_tp);
        const int cum = total - behind - (incl - fi);
        const double prec = i >= 0 ? (double)cum / (double)(i + 1) : 0.0;
        double chunk_max;
        const double m = fmax(eval_scan_max(prec, s_d, chunk_max), tail_max);
        if (fi) acc += m;
        behind += chunk_tp;
        tail_max = fmax(tail_max, chunk_max);
    }
    s_acc[tid] = acc;
    __syncthreads();
    if (tid == 0) {
        double sum = 0.0;
        for (int j = 0; j < 256; ++j) sum += s_acc[j];
        ap[blockIdx.x] = sum / (double)npos[c];
    }
}

// Python's two-argument max / min: the first argument unless the second compares greater / smaller
__device__ __forceinline__ double eval_pymax(double x, double y) { return y > x ? y : x; }
__device__ __forceinline__ double eval_pymin(double x, double y) { return y < x ? y : x; }

// temporal_recall (detection_metrics.py:31-51) for every video and threshold, one lane per ground-truth span: the
// largest temporal_iou (:7-20, intersection over the HULL, 0 when the intersection is empty) with a proposal of its
// video; the span is hit at threshold t when that IoU is strictly greater.
__global__ __launch_bounds__(256) void eval_recall_kernel(const double* gt, const int* gt_off, int G, const double* prop,
                                                          const int* prop_off, int P, int V, const double* thr, int T, int* hits) {
    const int g = blockIdx.x * 256 + threadIdx.x;
    if (g >= G) return;
    const int v = eval_find(gt_off, V, g);
    int p0 = prop_off[v], p1 = prop_off[v + 1];
    p0 = p0 < 0 ? 0 : p0;
    p1 = p1 > P ? P : p1;
    if (p1 <= p0) return;
    const double a0 = gt[2 * (long)g], a1 = gt[2 * (long)g + 1];
    double best = 0.0;
    bool first = true;
    for (int p = p0; p < p1; ++p) {
        const double e0 = prop[2 * (long)p], e1 = prop[2 * (long)p + 1];
        const double i0 = eval_pymax(a0, e0), i1 = eval_pymin(a1, e1);
        double ov = 0.0;
        if (!(i0 >= i1)) ov = (i1 - i0) / (eval_pymax(a1, e1) - eval_pymin(a0, e0));
        if (first || ov > best) best = ov;
        first = false;
    }
    for (int t = 0; t < T; ++t)
        if (best > thr[t]) atomicAdd(&hits[(long)v * T + t], 1);
}

}  // namespace

// Ground-truth rows of one (class, video) group that are matched out of LDS; a larger group needs
// rows + 32 * ceil(rows / 64) 8-byte units of the workspace (`big_units`).
extern "C" int ssn_eval_lds_gt(void) { return EVAL_LDS_GT; }

// Device scratch of ssn_eval_ap: 16 bytes per sort entry, 8 per unit of the large groups, one cursor per class.
extern "C" size_t ssn_eval_workspace_bytes(long sort_entries, long big_units, int C) {
    if (sort_entries < 0 || big_units < 0 || C < 0) return 0;
    return 16 + 16 * (size_t)sort_entries + 8 * (size_t)big_units + 4 * (size_t)C;
}

// Sizing pass: counts [C + 1] int32 (device) <- predictions per class, and in counts[C] the rows whose class lies
// outside [0, C) or whose score is not finite (the caller refuses the evaluation when that is not zero).
extern "C" int ssn_eval_count(const double* pred_score, const int* pred_cls, int N, int C, int* counts, hipStream_t stream) {
    SSN_CHECK_ARG(counts && C >= 1 && N >= 0, "eval_count: bad arguments");
    SSN_CHECK_ARG(N == 0 || (pred_score && pred_cls), "eval_count: null pointer");
    if (hipMemsetAsync(counts, 0, sizeof(int) * ((size_t)C + 1), stream) != hipSuccess) {
        ssn_set_error("eval_count: memset failed");
        return SSN_ERR_LAUNCH;
    }
    if (N == 0) return SSN_OK;
    hipLaunchKernelGGL(eval_count_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, stream, pred_score, pred_cls, N, C,
                       counts);
    SSN_CHECK_LAUNCH("eval_count");
    return SSN_OK;
}

// Average precision of every (class, threshold).  Predictions flat in any order: pred_seg [N][2], pred_score [N] fp64,
// pred_cls / pred_vid [N] int32.  Ground truth: gt_seg [G][2] fp64 with the rows of one (class, video) group next to
// each other, groups [NG][5] int32 = (class, video, first row, rows, offset of the group's scratch in 8-byte units),
// npos [C] int32 rows per class.  thresholds [T] fp64, T <= 32.  pred_off [C + 1] int32: exclusive prefix sums of the
// counts of ssn_eval_count; sort_off [C + 1] int64: the same with every class rounded up to a power of two (0 stays 0).
// Out: order [N] int32 (flat indices class by class in descending score, equal scores lower index first), tp [T][N]
// uint8 in that order, ap [C][T] fp64 (NaN where npos is 0).  Everything but the sizes is device memory.
extern "C" int ssn_eval_ap(const double* pred_seg, const double* pred_score, const int* pred_cls, const int* pred_vid, int N,
                           const double* gt_seg, const int* groups, int NG, int G, const int* npos, const double* thresholds,
                           int T, int C, const int* pred_off, const long* sort_off, long sort_entries, long big_units,
                           int* order, unsigned char* tp, double* ap, void* workspace, size_t ws_bytes, hipStream_t stream) {
    SSN_CHECK_ARG(T >= 1 && T <= EVAL_MAX_T, "eval_ap: %d thresholds, at most %d in one call", T, EVAL_MAX_T);
    SSN_CHECK_ARG(C >= 1 && N >= 0 && NG >= 0 && G >= 0 && (long)C * T < (1L << 30) && sort_entries >= 0 && big_units >= 0 &&
                      sort_entries < (1L << 31) && (long)N * T < (1L << 40),
                  "eval_ap: bad sizes");
    SSN_CHECK_ARG(npos && thresholds && pred_off && sort_off && ap && workspace, "eval_ap: null pointer");
    SSN_CHECK_ARG(N == 0 || (pred_seg && pred_score && pred_cls && pred_vid && order && tp), "eval_ap: null pointer");
    SSN_CHECK_ARG(NG == 0 || (gt_seg && groups), "eval_ap: null pointer");
    SSN_CHECK_ARG(sort_entries >= N, "eval_ap: %ld sort entries for %d predictions", sort_entries, N);
    if (ws_bytes < ssn_eval_workspace_bytes(sort_entries, big_units, C)) {
        ssn_set_error("eval_ap: workspace of %zu bytes, %zu needed", ws_bytes, ssn_eval_workspace_bytes(sort_entries, big_units, C));
        return SSN_ERR_WORKSPACE;
    }
    u64* hi = (u64*)workspace;
    u64* lo = hi + sort_entries;
    double* big = (double*)(lo + sort_entries);
    int* cursor = (int*)(big + big_units);
    if (N > 0) {
        if (hipMemsetAsync(hi, 0xff, 16 * (size_t)sort_entries, stream) != hipSuccess ||
            hipMemsetAsync(cursor, 0, sizeof(int) * (size_t)C, stream) != hipSuccess ||
            hipMemsetAsync(tp, 0, (size_t)T * (size_t)N, stream) != hipSuccess) {
            ssn_set_error("eval_ap: memset failed");
            return SSN_ERR_LAUNCH;
        }
        hipLaunchKernelGGL(eval_fill_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, stream, pred_score, pred_cls,
                           pred_vid, N, C, sort_off, sort_entries, cursor, hi, lo);
        hipLaunchKernelGGL(eval_sort_kernel, dim3((unsigned)C), dim3(256), 0, stream, hi, lo, sort_off, sort_entries, pred_off, N,
                           order);
        if (NG > 0) {
            EvalMatchArgs a;
            a.pred_seg = pred_seg;
            a.lo = lo;
            a.gt_seg = gt_seg;
            a.groups = groups;
            a.thr = thresholds;
            a.pred_off = pred_off;
            a.sort_off = sort_off;
            a.big = big;
            a.tp = tp;
            a.N = N;
            a.G = G;
            a.T = T;
            a.C = C;
            a.sort_entries = sort_entries;
            a.big_units = big_units;
            hipLaunchKernelGGL(eval_match_kernel<true>, dim3((unsigned)NG), dim3(64), 0, stream, a);
            if (big_units > 0) hipLaunchKernelGGL(eval_match_kernel<false>, dim3((unsigned)NG), dim3(64), 0, stream, a);
        }
    }
    hipLaunchKernelGGL(eval_ap_kernel, dim3((unsigned)(C * T)), dim3(256), 0, stream, (const unsigned char*)tp, pred_off, npos, N,
                       T, ap);
    SSN_CHECK_LAUNCH("eval_ap");
    return SSN_OK;
}

// temporal_recall for a batch: gt_span [G][2] fp64 ragged by gt_off [V + 1], prop [P][2] fp64 ragged by prop_off [V + 1],
// thresholds [T] fp64 (all device) -> hits [V][T] int32: ground-truth spans of video v that some proposal overlaps with
// temporal_iou strictly above threshold t.
extern "C" int ssn_eval_recall(const double* gt_span, const int* gt_off, int G, const double* prop, const int* prop_off, int P,
                               int V, const double* thresholds, int T, int* hits, hipStream_t stream) {
    SSN_CHECK_ARG(V >= 1 && G >= 0 && P >= 0 && T >= 1 && (long)V * T < (1L << 30), "eval_recall: bad sizes");
    SSN_CHECK_ARG(gt_off && prop_off && thresholds && hits, "eval_recall: null pointer");
    SSN_CHECK_ARG((G == 0 || gt_span) && (P == 0 || prop), "eval_recall: null pointer");
    if (hipMemsetAsync(hits, 0, sizeof(int) * (size_t)V * (size_t)T, stream) != hipSuccess) {
        ssn_set_error("eval_recall: memset failed");
        return SSN_ERR_LAUNCH;
    }
    if (G == 0 || P == 0) return SSN_OK;
    hipLaunchKernelGGL(eval_recall_kernel, dim3((unsigned)((G + 255) / 256)), dim3(256), 0, stream, gt_span, gt_off, G, prop,
                       prop_off, P, V, thresholds, T, hits);
    SSN_CHECK_LAUNCH("eval_recall");
    return SSN_OK;
}
