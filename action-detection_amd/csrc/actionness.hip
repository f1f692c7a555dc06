// The scoring tail of the actionness stage (stage 2 of the reference's workflow) and the merge in front of TAG:
//   test_fc on the backbone output + the (mis)grouping of its rows      /root/reference/binary_test.py:84-92
//   mean over the crop axis and the merging loop over score files       /root/reference/gen_bottom_up_proposals.py:76-91
// binary_test.py gets its frames crop-major ([crop][tick], 4 ticks per generator batch, load_binary_score.py:265,288-304)
// and views the logits as view(-1, num_crop, D), i.e. as if they were tick-major: row i of its output is ten CONSECUTIVE
// rows of the crop-major list of its batch, not the ten crops of tick i.  Here the linear kernel always writes the TRUE
// layout raw_true[tick][crop][:]; the grouping kernel then either keeps it ("tick") or re-creates the reference's rows
// from it ("reference"), and averages the crops the way numpy does.  fp32 without contraction, as in tag.hip: the crop
// mean and the merge are bit-equal to the host arithmetic of tag_proposals.merge_scores.
#include "ssn_common.h"

#pragma clang fp contract(off)

namespace {

constexpr int ACT_KC = 4;      // classes one pass over a feature row serves

struct __attribute__((aligned(4))) ActF4 {      // 16 bytes that start on any dword: rows of a [R][D] matrix with D % 4 != 0
    float x, y, z, w;
};

// One wave per feature row r = c * ticks + t (crop-major).  The D products of a (row, class) pair are summed in an order
// that depends on D alone: lane l takes the groups of four elements l, l + 64, ... (each group in element order; the
// D % 4 elements behind the last full group are one more, shorter group), then the 64 partial sums meet in a butterfly.
// Neither the number of rows of the call nor the alignment of the row enters, so a tick scores bit-identically in any
// batching.
__global__ __launch_bounds__(256) void actionness_fc_kernel(const float* feat, const float* w, const float* b, float* raw_true,
                                                            int R, int ticks, int crops, int C, int D, long tick0) {
    const int lane = threadIdx.x & 63;
    const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= R) return;      // (wave-uniform)
    const int c = (int)(row / ticks), t = (int)(row - (long)c * ticks);
    const float* x = feat + row * D;
    float* out = raw_true + ((tick0 + t) * crops + c) * C;
    const int groups = D >> 2, tail = D & 3;
    for (int k0 = 0; k0 < C; k0 += ACT_KC) {
        const int kc = C - k0 < ACT_KC ? C - k0 : ACT_KC;
        float acc[ACT_KC] = {0.f, 0.f, 0.f, 0.f};
        for (int g = lane; g < groups; g += 64) {
            const ActF4 xv = *(const ActF4*)(x + 4 * g);
#pragma unroll
            for (int j = 0; j < ACT_KC; ++j) {
                if (j < kc) {
                    const ActF4 wv = *(const ActF4*)(w + (long)(k0 + j) * D + 4 * g);
                    acc[j] += xv.x * wv.x;
                    acc[j] += xv.y * wv.y;
                    acc[j] += xv.z * wv.z;
                    acc[j] += xv.w * wv.w;
                }
            }
        }
        if (tail && lane == (groups & 63)) {
            for (int e = 4 * groups; e < D; ++e) {
                const float xe = x[e];
#pragma unroll
                for (int j = 0; j < ACT_KC; ++j)
                    if (j < kc) acc[j] += xe * w[(long)(k0 + j) * D + e];
            }
        }
#pragma unroll
        for (int j = 0; j < ACT_KC; ++j) {
            float s = acc[j];
            for (int off = 32; off >= 1; off >>= 1) s += __shfl_xor(s, off, 64);
            if (lane == 0 && j < kc) out[k0 + j] = s + (b ? b[k0 + j] : 0.f);
        }
    }
}

// raw_true [T][crops][C] -> raw [T][crops][C] and mean [T][C]; one thread per (row i, class k) walks the crop slots in
// order.  g = 0: raw = raw_true.  g > 0: the rows binary_test.py writes when its generator yields g ticks per batch: batch
// q = i / g holds b = min(g, T - g q) ticks, its crop-major list has the logits of (crop r / b, tick g q + r % b) at
// position r, and output row i takes positions (i - g q) * crops + j, j = 0 .. crops - 1.
// mean: slot 0, plus the slots 1 .. crops - 1 in order, one division by float(crops) -- numpy's mean over this axis.
__global__ __launch_bounds__(256) void actionness_group_kernel(const float* raw_true, float* raw, float* mean, int T, int crops,
                                                               int C, int g) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long)T * C) return;
    const int i = (int)(idx / C), k = (int)(idx - (long)i * C);
    int base = i, b = 1, r0 = 0;
    if (g > 0) {
        const int q = i / g;
        base = g * q;
        b = T - base < g ? T - base : g;
        r0 = (i - base) * crops;
    }
    float acc = 0.f;
    for (int j = 0; j < crops; ++j) {
        long src;
        if (g > 0) {
            const int r = r0 + j;
            src = ((long)(base + r % b) * crops + r / b) * C + k;
        } else {
            src = ((long)i * crops + j) * C + k;
        }
        const float v = raw_true[src];
        raw[((long)i * crops + j) * C + k] = v;
        acc = j == 0 ? v : acc + v;
    }
    mean[idx] = acc / (float)crops;
}

// video of output row x: the largest v with off[v] <= x (tag_find of tag.hip; the caller checks the result against the table)
__device__ __forceinline__ int act_find(const int* off, int V, int x) {
    int lo = 0, hi = V - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (off[mid] <= x) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// The merging loop for all videos: one thread per (output row, class).  Stream s of video v is the rows
// off[s * V + v] .. off[s * V + v + 1] of `rows`.  The loop keeps a merged length: a shorter stream truncates it (for every
// stream that follows as well), a longer one is read at int(x * (T_add / float(T_merged))) in fp64.  A row x of the result
// depends on the rows x of the prefixes only, so every thread replays the loop for its own row.  Every offset read from
// the tables is checked against the operand sizes, and the length the loop arrives at against out_off: a video whose tables
// disagree writes nothing.
__global__ __launch_bounds__(256) void actionness_merge_kernel(const float* rows, const int* off, const float* weights,
                                                               const int* out_off, float* out, int S, int V, int C, int total_rows,
                                                               int out_rows) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long)out_rows * C) return;
    const int xg = (int)(idx / C), k = (int)(idx - (long)xg * C);
    const int v = act_find(out_off, V, xg);
    const int o0 = out_off[v], o1 = out_off[v + 1];
    if (o0 < 0 || o1 > out_rows || xg < o0 || xg >= o1) return;
    const int x = xg - o0;
    // first pass: the tables of this video, and the length the loop ends with
    int len = 0;
    for (int s = 0; s < S; ++s) {
        const int a0 = off[(long)s * V + v], a1 = off[(long)s * V + v + 1];
        if (a0 < 0 || a1 > total_rows || a1 <= a0) return;
        const int n = a1 - a0;
        if (s == 0 || n < len) len = n;
    }
    if (len != o1 - o0) return;
    float merged = 0.f;
    int cur = 0;
    for (int s = 0; s < S; ++s) {
        const int a0 = off[(long)s * V + v], n = off[(long)s * V + v + 1] - a0;
        int src = x;
        if (s == 0) {
            cur = n;
        } else if (n < cur) {
            cur = n;
        } else if (n > cur) {
            const double tick = (double)n / (double)cur;
            src = (int)((double)x * tick);
        }
        if (src < 0 || src >= n) return;
        const float add = rows[((long)a0 + src) * C + k] * weights[s];
        merged = s == 0 ? add : merged + add;
    }
    out[idx] = merged;
}

}  // namespace

// test_fc of one backbone call, written in true layout.  feat [R][D] crop-major with R = num_crop * ticks, w [C][D], b [C] or
// NULL; raw_true [T][num_crop][C] is the video's staging tensor, the call covers its ticks tick0 .. tick0 + ticks - 1.
extern "C" int ssn_actionness_fc(const float* feat, const float* w, const float* b, float* raw_true, int ticks, int num_crop,
                                 int C, int D, int tick0, int T, hipStream_t stream) {
    SSN_CHECK_ARG(ticks >= 0 && num_crop >= 1 && C >= 1 && D >= 1 && tick0 >= 0 && T >= 0, "actionness_fc: bad sizes");
    SSN_CHECK_ARG((long)tick0 + ticks <= T, "actionness_fc: ticks %d..%d outside the video's %d", tick0, tick0 + ticks, T);
    SSN_CHECK_ARG((long)ticks * num_crop < (1L << 30) && (long)T * num_crop * C < (1L << 40), "actionness_fc: too many rows");
    if (ticks == 0) return SSN_OK;
    SSN_CHECK_ARG(feat && w && raw_true, "actionness_fc: null pointer");
    SSN_CHECK_ARG((((uintptr_t)feat | (uintptr_t)w) & 3) == 0, "actionness_fc: operands must be 4-byte aligned");
    const int R = ticks * num_crop;
    hipLaunchKernelGGL(actionness_fc_kernel, dim3((unsigned)((R + 3) / 4)), dim3(256), 0, stream, feat, w, b, raw_true, R, ticks,
                       num_crop, C, D, (long)tick0);
    SSN_CHECK_LAUNCH("actionness_fc");
    return SSN_OK;
}

// One video.  raw may be raw_true itself when ref_batch == 0 (every element is read and written by the same thread).
extern "C" int ssn_actionness_group(const float* raw_true, float* raw, float* mean, int T, int num_crop, int C, int ref_batch,
                                    hipStream_t stream) {
    SSN_CHECK_ARG(T >= 0 && num_crop >= 1 && C >= 1 && ref_batch >= 0, "actionness_group: bad sizes");
    SSN_CHECK_ARG((long)T * num_crop * C < (1L << 40) && (long)T * C < (1L << 31) && (long)ref_batch * num_crop < (1L << 30),
                  "actionness_group: too many rows");
    if (T == 0) return SSN_OK;
    SSN_CHECK_ARG(raw_true && raw && mean, "actionness_group: null pointer");
    SSN_CHECK_ARG(ref_batch == 0 || raw != raw_true, "actionness_group: the reference grouping cannot run in place");
    const long n = (long)T * C;
    hipLaunchKernelGGL(actionness_group_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, raw_true, raw, mean, T,
                       num_crop, C, ref_batch);
    SSN_CHECK_LAUNCH("actionness_group");
    return SSN_OK;
}

// rows [total_rows][C] fp32: the crop-averaged scores of S streams x V videos one after the other, stream-major; offsets
// [S * V + 1] int32, weights [S] fp32, out_offsets [V + 1] int32 (all device); out [out_rows][C].
extern "C" int ssn_actionness_merge(const float* rows, const int* offsets, const float* weights, const int* out_offsets, float* out,
                                    int S, int V, int C, int total_rows, int out_rows, hipStream_t stream) {
    SSN_CHECK_ARG(S >= 1 && V >= 1 && C >= 1 && total_rows >= 0 && out_rows >= 0, "actionness_merge: bad sizes");
    SSN_CHECK_ARG((long)S * V < (1L << 30) && total_rows < (1 << 30) && (long)out_rows * C < (1L << 31),
                  "actionness_merge: too many rows");
    if (out_rows == 0) return SSN_OK;
    SSN_CHECK_ARG(rows && offsets && weights && out_offsets && out, "actionness_merge: null pointer");
    const long n = (long)out_rows * C;
    hipLaunchKernelGGL(actionness_merge_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, rows, offsets, weights,
                       out_offsets, out, S, V, C, total_rows, out_rows);
    SSN_CHECK_LAUNCH("actionness_merge");
    return SSN_OK;
}
