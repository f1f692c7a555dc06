// Device helpers shared by the per-video (detect.hip) and the batched (detect_batch.hip) detection post-processing: both
// units run the SAME expressions on the same values, which is what makes their results bit-identical.
#pragma once
#include "ssn_common.h"

namespace {

constexpr int DET_MAXN = 2048;   // candidates of one class that are sorted and suppressed in LDS

// combined[p][c] = softmax(act[p][off : off + n_sm])[c + 1 - off] * exp(comp[p][c]),  off = 0 (include_bg 1: softmax over all
// C + 1 activity scores, then drop the background column) or 1 (include_bg 0: softmax over the C class scores only);
// include_bg 2: NO softmax, the raw class scores act[p][c + 1] (the `--cls_scores` branch without --softmax_before_filter, :135)
// One wave per row; rows are independent, so P may be one video's proposals or those of a whole batch.
__global__ __launch_bounds__(256) void det_scores_kernel(const float* act, const float* comp, float* combined, int P, int C,
                                                         int include_bg) {
    const int p = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (p >= P) return;
    const float* a = act + (long)p * (C + 1);
    if (include_bg == 2) {
        for (int c = lane; c < C; c += 64) combined[(long)p * C + c] = a[c + 1] * expf(comp[(long)p * C + c]);
        return;
    }
    const int lo = include_bg ? 0 : 1;
    float mx = -INFINITY;
    for (int c = lo + lane; c <= C; c += 64) mx = fmaxf(mx, a[c]);
    mx = wave_max(mx);
    float sum = 0.f;
    for (int c = lo + lane; c <= C; c += 64) sum += expf(a[c] - mx);
    sum = wave_sum(sum);
    for (int c = lane; c < C; c += 64)
        combined[(long)p * C + c] = (expf(a[c + 1] - mx) / sum) * expf(comp[(long)p * C + c]);
}

// Total order on fused scores, the one numpy's sorts use: ascending floats, every NaN after +inf.  The key is the
// usual monotone map of the bit pattern (negative: all bits flipped, non-negative: sign bit set) with all NaNs
// collapsed onto the largest key.  softmax * exp overflows to inf and inf * 0 to NaN on real (diverged) scores; sorting
// on raw floats is then not a total order and a bitonic network may move its padding anywhere.
__device__ __forceinline__ uint32_t det_key(float v) {
    const uint32_t b = __builtin_bit_cast(uint32_t, v);
    if ((b & 0x7fffffffu) > 0x7f800000u) return 0xffffffffu;
    return (b >> 31) ? ~b : (b | 0x80000000u);
}

// Exactly-k selection (np.argsort(v)[-k:], eval_detection_results.py:113-114) in two numbers, by the 1024 threads of one
// workgroup: out[0] = key T of the k-th largest element (radix select on det_key); elements with a larger key are all
// kept; of the elements whose key equals T, those with index >= out[1..2] (a 64-bit cut) are kept -- the `need` highest
// indices, which is what a stable ascending argsort leaves in its last k positions.  Needs 0 < k < n.
__device__ __forceinline__ void det_topk_select(const float* v, long n, long k, uint32_t* out) {
    __shared__ int hist[256];
    __shared__ uint32_t s_prefix, s_mask;
    __shared__ long s_k, s_ties, s_cut;
    __shared__ int s_cnt;
    __shared__ unsigned char flags[1024];
    if (threadIdx.x == 0) {
        s_prefix = 0;
        s_mask = 0;
        s_k = k;
        s_ties = 0;
        s_cut = 0;
    }
    __syncthreads();
    for (int shift = 24; shift >= 0; shift -= 8) {
        for (int i = threadIdx.x; i < 256; i += 1024) hist[i] = 0;
        __syncthreads();
        const uint32_t prefix = s_prefix, mask = s_mask;
        for (long i = threadIdx.x; i < n; i += 1024) {
            const uint32_t b = det_key(v[i]);
            if ((b & mask) == prefix) atomicAdd(&hist[(b >> shift) & 255u], 1);
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            long need = s_k;
            int d = 255;
            for (; d > 0; --d) {
                if ((long)hist[d] >= need) break;
                need -= hist[d];
            }
            s_k = need;
            s_ties = hist[d];
            s_prefix = prefix | ((uint32_t)d << shift);
            s_mask = mask | (255u << shift);
        }
        __syncthreads();
    }
    const uint32_t T = s_prefix;
    const long need = s_k;
    if (s_ties > need) {
        // more elements tie at T than are still wanted: walk the array from its end in chunks of 1024 until the chunk
        // that holds the need-th tie, then find it
        long hi = n, cum = 0;
        while (hi > 0) {
            const long base = hi > 1024 ? hi - 1024 : 0;
            if (threadIdx.x == 0) s_cnt = 0;
            __syncthreads();
            const long i = base + threadIdx.x;
            const int tie = i < hi && det_key(v[i]) == T;
            flags[threadIdx.x] = (unsigned char)tie;
            if (tie) atomicAdd(&s_cnt, 1);
            __syncthreads();
            const int cnt = s_cnt;
            if (cum + cnt >= need) {
                if (threadIdx.x == 0) {
                    long c = cum;
                    for (long j = hi - base - 1; j >= 0; --j)
                        if (flags[j] && ++c == need) {
                            s_cut = base + j;
                            break;
                        }
                }
                break;
            }
            cum += cnt;
            hi = base;
            __syncthreads();
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        out[0] = T;
        out[1] = (uint32_t)((unsigned long)s_cut & 0xffffffffu);
        out[2] = (uint32_t)((unsigned long)s_cut >> 32);
    }
}

// is the pair with fused-score key kk and flat index `flat` among the selected ones?  (thr = 0, cut = 0 keeps everything:
// no key is below 0 and no index below 0)
__device__ __forceinline__ bool det_selected(uint32_t kk, long flat, uint32_t thr, long cut) {
    return kk > thr || (kk == thr && flat >= cut);
}

// does entry (ki, ii) belong in front of (kl, il)?  Descending score; equal scores: higher proposal index first, the order
// `scores.argsort()[::-1]` gives with a stable sort (ops/utils.py:68).  Padding (key 0, index -1) sorts behind everything.
__device__ __forceinline__ bool det_before(uint32_t ki, int ii, uint32_t kl, int il) {
    return ki > kl || (ki == kl && ii > il);
}

// does the kept box (a1, a2) suppress (b1, b2)?  ops/utils.py:71-80: the intersection is NOT clamped at zero there, so
// neither is it here; a NaN IoU suppresses.
__device__ __forceinline__ bool det_suppresses(double a1, double a2, double b1, double b2, double nms_thresh) {
    const double da = a2 - a1;
    const double tt1 = a1 > b1 ? a1 : b1;
    const double tt2 = a2 < b2 ? a2 : b2;
    const double inter = tt2 - tt1;
    const double iou = inter / (da + (b2 - b1) - inter);
    return !(iou <= nms_thresh);
}

__device__ __forceinline__ double det_clip01(double x) { return x < 0.0 ? 0.0 : (x > 1.0 ? 1.0 : x); }   // np.clip: NaN stays

// The five values of one detection: start, end (regressed and clipped, eval_detection_results.py:167-178, or the proposal's
// own span), fused score, loc, dur.  (a1, a2): the proposal's span; pair: its index p * C + c into combined and reg.
__device__ __forceinline__ void det_write_row(double* d, double a1, double a2, const float* combined, const float* reg,
                                              long pair, int regress) {
    const float loc = reg ? reg[pair * 2] : 0.f;
    const float dur = reg ? reg[pair * 2 + 1] : 0.f;
    double s0 = a1, s1 = a2;
    if (regress) {
        const double center = (a1 + a2) / 2, duration = a2 - a1;
        const double nc = center + duration * (double)loc;
        const double nd = duration * exp((double)dur);
        s0 = det_clip01(nc - nd / 2);
        s1 = det_clip01(nc + nd / 2);
    }
    d[0] = s0;
    d[1] = s1;
    d[2] = (double)combined[pair];
    d[3] = (double)loc;
    d[4] = (double)dur;
}

inline int det_pow2(int n) {
    int n2 = 1;
    while (n2 < n) n2 <<= 1;
    return n2;
}

}  // namespace
