// Detection post-processing of one video on the GPU: the per-video arithmetic of the reference's evaluation script
//   score fusion  softmax(activity)[1:] * exp(completeness)          /root/reference/eval_detection_results.py:91-128
//   top-k over all (proposal, class) pairs                           :113-128 (np.argsort(...)[-top_k:])
//   temporal NMS per class                                           /root/reference/ops/utils.py:56-82
//   location regression                                              /root/reference/eval_detection_results.py:167-178
// which the reference runs in numpy, class by class and video by video.  Box arithmetic is fp64 as in numpy (the
// proposal spans are float64 there and promote everything they touch); the fused scores are fp32 as in numpy.
#include "detect_common.h"

namespace {

// the selection of detect_common.h over all P * C fused scores of the video, one workgroup
__global__ __launch_bounds__(1024) void det_topk_threshold_kernel(const float* v, long n, long k, uint32_t* out) {
    det_topk_select(v, n, k, out);
}

struct DetArgs {
    const double* rel_prop;   // [P][2] start, end (normalised)
    const float* combined;    // [P][C]
    const float* reg;         // [P][C][2] or nullptr
    double* dets;             // [C][max_det][5]: start, end, score, loc, dur
    int* counts;              // [C]
    int P, C, max_det;
    const uint32_t* sel;      // {threshold key, flat-index cut lo, hi} from the selection kernel, or nullptr: keep all
    double nms_thresh;
    int regress;
    // storage of the candidates of one class when they do not fit in LDS (P > DET_MAXN): [C][cap] each
    uint32_t* g_key;
    int* g_idx;
    unsigned char* g_supp;
    int cap;
};

// One workgroup per class: collect the class's candidates, sort them (descending score; equal scores: higher proposal
// index first, the order `scores.argsort()[::-1]` gives with a stable sort, ops/utils.py:68), suppress greedily.
// IN_LDS: the candidate arrays live in LDS (up to DET_MAXN per class); otherwise in the caller's workspace.
template <bool IN_LDS>
__global__ __launch_bounds__(256) void det_nms_kernel(DetArgs a) {
    constexpr int LN = IN_LDS ? DET_MAXN : 1;
    __shared__ uint32_t l_key[LN];
    __shared__ int l_idx[LN];
    __shared__ double l_t1[LN], l_t2[LN];
    __shared__ unsigned char l_supp[LN];
    __shared__ int s_n, s_keep;
    const int c = blockIdx.x, tid = threadIdx.x;
    uint32_t* key = IN_LDS ? l_key : a.g_key + (long)c * a.cap;
    int* idx = IN_LDS ? l_idx : a.g_idx + (long)c * a.cap;
    unsigned char* supp = IN_LDS ? l_supp : a.g_supp + (long)c * a.cap;
    const int cap = IN_LDS ? DET_MAXN : a.cap;
    uint32_t thr = 0;
    long cut = 0;
    if (a.sel) {
        thr = a.sel[0];
        cut = (long)(((unsigned long)a.sel[2] << 32) | a.sel[1]);
    }
    if (tid == 0) {
        s_n = 0;
        s_keep = 0;
    }
    __syncthreads();
    // candidates of this class, in any order (the sort's order is total)
    for (int p = tid; p < a.P; p += 256) {
        const long flat = (long)p * a.C + c;
        const uint32_t kk = det_key(a.combined[flat]);
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
    if (n > cap) n = cap;             // cannot happen: cap >= P (host-checked)
    int n2 = 1;
    while (n2 < n) n2 <<= 1;
    for (int i = n + tid; i < n2; i += 256) {
        key[i] = 0;                   // below every real key (det_key never returns 0 for a non-NaN, NaNs map to the top)
        idx[i] = -1;                  // and behind every real entry on a key tie
    }
    __syncthreads();
    for (int k = 2; k <= n2; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = tid; i < n2; i += 256) {
                const int l = i ^ j;
                if (l > i) {
                    const bool desc = (i & k) == 0;
                    const uint32_t ki = key[i], kl = key[l];
                    const int ii = idx[i], il = idx[l];
                    const bool before = det_before(ki, ii, kl, il);   // i belongs first
                    if (desc != before) {
                        key[i] = kl;
                        key[l] = ki;
                        idx[i] = il;
                        idx[l] = ii;
                    }
                }
            }
            __syncthreads();
        }
    for (int i = tid; i < n; i += 256) {
        int p = idx[i];
        if (p < 0 || p >= a.P) p = 0;          // defensive: never index outside the proposal table
        if (IN_LDS) {
            l_t1[i] = a.rel_prop[2 * (long)p];
            l_t2[i] = a.rel_prop[2 * (long)p + 1];
        }
        idx[i] = p;
        supp[i] = 0;
    }
    __syncthreads();
    // greedy NMS in score order (ops/utils.py:71-80): box i survives if no surviving higher-scored box overlaps it by
    // more than the threshold; the intersection is NOT clamped at zero there, so neither is it here.  A barrier is only
    // needed behind a box that survives (suppressed ones write nothing).
    for (int i = 0; i < n; ++i) {
        if (supp[i]) continue;       // uniform: supp[i] was settled before the last barrier
        const int pi = idx[i];
        const double a1 = IN_LDS ? l_t1[i] : a.rel_prop[2 * (long)pi];
        const double a2 = IN_LDS ? l_t2[i] : a.rel_prop[2 * (long)pi + 1];
        for (int j = i + 1 + tid; j < n; j += 256) {
            const double b1 = IN_LDS ? l_t1[j] : a.rel_prop[2 * (long)idx[j]];
            const double b2 = IN_LDS ? l_t2[j] : a.rel_prop[2 * (long)idx[j] + 1];
            if (det_suppresses(a1, a2, b1, b2, a.nms_thresh)) supp[j] = 1;
        }
        if (tid == 0) {
            const int o = s_keep++;
            if (o < a.max_det) {
                det_write_row(a.dets + ((long)c * a.max_det + o) * 5, a1, a2, a.combined, a.reg, (long)pi * a.C + c, a.regress);
            }
        }
        __syncthreads();
    }
    if (tid == 0) a.counts[c] = s_keep < a.max_det ? s_keep : a.max_det;
}

}  // namespace

// Device scratch ssn_detections needs for a video of P proposals and C classes: the selection words, plus -- when the
// candidates of a class do not fit in LDS (P > 2048) -- key / index / flag arrays of pow2(P) entries per class.
extern "C" size_t ssn_detections_workspace_bytes(int P, int C) {
    size_t b = 16;
    if (P > DET_MAXN) b += (size_t)C * (size_t)det_pow2(P) * 12;     // u32 key + i32 idx + u8 flag (padded to 4)
    return b;
}

// act [P][C+1], comp [P][C], reg [P][C][2] (or NULL) fp32; rel_prop [P][2] fp64.  combined [P][C] fp32 (scratch + output),
// dets [C][max_det][5] fp64, counts [C] int32, workspace: ssn_detections_workspace_bytes(P, C) bytes, 16-byte aligned.
// include_bg: softmax over all C+1 activity scores (the `top_k <= 0` branch, :98) instead of over the C class scores
// (:113); top_k <= 0 keeps every pair.  Non-finite scores are ordered as numpy orders them (NaN above +inf); nothing
// in here can index outside its inputs whatever the scores are.
extern "C" int ssn_detections(const float* act, const float* comp, const float* reg, const double* rel_prop, float* combined,
                              double* dets, int* counts, void* workspace, size_t ws_bytes, int P, int C, int max_det,
                              int top_k, int include_bg, double nms_thresh, int regress, hipStream_t stream) {
    SSN_CHECK_ARG(dets && counts, "detections: null pointer");
    SSN_CHECK_ARG(P >= 0 && C >= 1 && max_det >= 1, "detections: bad sizes");
    SSN_CHECK_ARG((long)P * C < (1L << 40), "detections: too many (proposal, class) pairs");
    SSN_CHECK_ARG(P == 0 || (act && comp && rel_prop && combined && workspace), "detections: null pointer");
    if (hipMemsetAsync(counts, 0, sizeof(int) * (size_t)C, stream) != hipSuccess) {
        ssn_set_error("detections: memset failed");
        return SSN_ERR_LAUNCH;
    }
    if (P == 0) return SSN_OK;
    if (ws_bytes < ssn_detections_workspace_bytes(P, C)) {
        ssn_set_error("detections: workspace of %zu bytes, %zu needed", ws_bytes, ssn_detections_workspace_bytes(P, C));
        return SSN_ERR_WORKSPACE;
    }
    hipLaunchKernelGGL(det_scores_kernel, dim3((unsigned)((P + 3) / 4)), dim3(256), 0, stream, act, comp, combined, P, C,
                       include_bg);
    const long n = (long)P * C;
    const bool select = top_k > 0 && (long)top_k < n;
    uint32_t* sel = (uint32_t*)workspace;
    if (select)
        hipLaunchKernelGGL(det_topk_threshold_kernel, dim3(1), dim3(1024), 0, stream, (const float*)combined, n, (long)top_k,
                           sel);
    DetArgs a;
    a.rel_prop = rel_prop;
    a.combined = combined;
    a.reg = reg;
    a.dets = dets;
    a.counts = counts;
    a.P = P;
    a.C = C;
    a.max_det = max_det;
    a.sel = select ? sel : nullptr;
    a.nms_thresh = nms_thresh;
    a.regress = regress;
    a.g_key = nullptr;
    a.g_idx = nullptr;
    a.g_supp = nullptr;
    a.cap = 0;
    if (P <= DET_MAXN) {
        hipLaunchKernelGGL(det_nms_kernel<true>, dim3((unsigned)C), dim3(256), 0, stream, a);
    } else {
        const size_t cap = (size_t)det_pow2(P);
        char* w = (char*)workspace + 16;
        a.g_key = (uint32_t*)w;
        a.g_idx = (int*)(w + (size_t)C * cap * 4);
        a.g_supp = (unsigned char*)(w + (size_t)C * cap * 8);
        a.cap = (int)cap;
        hipLaunchKernelGGL(det_nms_kernel<false>, dim3((unsigned)C), dim3(256), 0, stream, a);
    }
    SSN_CHECK_LAUNCH("detections");
    return SSN_OK;
}
