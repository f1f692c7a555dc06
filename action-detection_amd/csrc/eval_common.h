// Device helpers shared by the evaluation units (eval.hip: detection AP with classes as segments; proposal_eval.hip:
// AR-AN with videos as segments): the total order on fp64 scores, the search in an offset table, and the per-segment
// bitonic sort on (descending score, lower flat index).  Every unit that includes this gets its own copy of the kernel.
#pragma once
#include "ssn_common.h"

namespace {

constexpr int EVAL_SORT_LDS = 2048;    // entries of one segment sorted inside LDS; more are sorted in place in the workspace
constexpr int EVAL_MAX_T = 32;         // thresholds per call (one lane each in the matching wave)

typedef unsigned long long u64;

// total order on finite fp64 bit patterns (-0.0 counts as +0.0, as numpy compares them)
__device__ __forceinline__ u64 eval_key(double s) {
    const u64 b = __builtin_bit_cast(u64, s == 0.0 ? 0.0 : s);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}

__device__ __forceinline__ bool eval_finite(double s) {
    return (__builtin_bit_cast(u64, s) & 0x7ff0000000000000ull) != 0x7ff0000000000000ull;
}

// the largest v with off[v] <= i (off non-decreasing, off[0] = 0 <= i < off[V])
__device__ __forceinline__ int eval_find(const int* off, int V, int i) {
    int lo = 0, hi = V - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (off[mid] <= i) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// One workgroup per segment: bitonic sort of its pow2 range, ascending on (hi, lo) -- descending score, then lower flat
// index (the padding is all ones and stays behind).  Writes the segment-wise order of the flat indices.
__global__ __launch_bounds__(256) void eval_sort_kernel(u64* g_hi, u64* g_lo, const long* sort_off, long sort_entries,
                                                        const int* pred_off, int N, int* order) {
    __shared__ u64 l_hi[EVAL_SORT_LDS], l_lo[EVAL_SORT_LDS];
    const int c = blockIdx.x, tid = threadIdx.x;
    const long sb = sort_off[c], nl = sort_off[c + 1] - sb;
    if (sb < 0 || nl <= 0 || sb + nl > sort_entries || nl > (1L << 30) || (nl & (nl - 1))) return;
    const int n2 = (int)nl;
    const bool in_lds = n2 <= EVAL_SORT_LDS;
    u64* hi = in_lds ? l_hi : g_hi + sb;
    u64* lo = in_lds ? l_lo : g_lo + sb;
    if (in_lds) {
        for (int i = tid; i < n2; i += 256) {
            l_hi[i] = g_hi[sb + i];
            l_lo[i] = g_lo[sb + i];
        }
    }
    __syncthreads();
    for (int k = 2; k <= n2; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = tid; i < n2; i += 256) {
                const int l = i ^ j;
                if (l > i) {
                    const bool asc = (i & k) == 0;
                    const u64 hi_i = hi[i], hi_l = hi[l], lo_i = lo[i], lo_l = lo[l];
                    const bool before = hi_i < hi_l || (hi_i == hi_l && lo_i < lo_l);      // i belongs first
                    if (asc != before) {
                        hi[i] = hi_l;
                        hi[l] = hi_i;
                        lo[i] = lo_l;
                        lo[l] = lo_i;
                    }
                }
            }
            __syncthreads();
        }
    const int pb = pred_off[c], n = pred_off[c + 1] - pb;
    if (pb < 0 || n < 0 || n > n2 || (long)pb + n > N) return;
    for (int i = tid; i < n; i += 256) {
        const u64 e = lo[i];
        if (in_lds) g_lo[sb + i] = e;            // (the matching pass reads video and flat index from here)
        order[pb + i] = (int)(e >> 32);
    }
}

}  // namespace
