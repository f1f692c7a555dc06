// Video-level classification for a whole batch of videos on the GPU: the step between the dense per-tick scores of the
// tester (ActionnessScores) and ONE score vector per video, and the classification metrics on those vectors.
//   aggregation   ops/video_funcs.py:8-82 of the reference (default / top-k / sliding window / TPP, fusion)
//   metrics       ops/metrics.py:14-60 (top-k hit rate, video mAP through sklearn, mean class accuracy)
// All videos lie one after the other: rows [N][C] fp32 and offsets [V + 1] int32; every kernel covers the whole batch,
// so the launches of a call do not depend on V.  Passes: status (non-finite input, empty video) -> crop reduction ->
// window maxima per (video, span) -> mean of the k largest per (segment, class) -> finish (mean over spans or weighted
// fusion, optional softmax, NaN rows for flagged videos).
//
// What is exact: maxima and the selection choose values; the k-th largest is found on order-preserving unsigned keys
// by a bit-by-bit threshold search (32 counting passes), and exactly min(k, n) entries are counted however many equal
// the k-th value: (sum of the values above it + (k' - count_above) * it) / k'.  Sums run rows ascending inside a wave's
// share (rows w, w + 4, ...) and then (w0 + w1) + (w2 + w3); every division is one IEEE fp32 division.
#include "ssn_common.h"

#include <math.h>

#pragma clang fp contract(off)

namespace {

constexpr int VCLS_LDS_ROWS = 128;     // rows of one segment whose keys are staged in LDS (x 64 classes); more are streamed
constexpr int VCLS_SORT_LDS = 4096;    // videos of one class sorted inside LDS for the AP; more are sorted in the workspace

typedef unsigned long long u64;

// total order on fp32 bit patterns (-0.0 counts as +0.0, as numpy compares them)
__device__ __forceinline__ uint32_t vcls_key(float x) {
    const uint32_t b = __builtin_bit_cast(uint32_t, x == 0.f ? 0.f : x);
    return (b >> 31) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float vcls_unkey(uint32_t k) {
    return __builtin_bit_cast(float, (k & 0x80000000u) ? (k ^ 0x80000000u) : ~k);
}
__device__ __forceinline__ bool vcls_finite(float x) { return (__builtin_bit_cast(uint32_t, x) & 0x7f800000u) != 0x7f800000u; }
// numpy's maximum: a NaN on either side stays
__device__ __forceinline__ float vcls_max(float m, float x) { return (x > m || x != x) ? x : m; }

// the largest g with off[g] <= i (off non-decreasing, off[0] <= i < off[G])
__device__ __forceinline__ int vcls_find(const int* off, int G, int i) {
    int lo = 0, hi = G - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (off[mid] <= i) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// the per-lane partial sums of the four waves of a workgroup in a fixed tree
__device__ __forceinline__ float vcls_combine(float v, float (*s)[64]) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    s[w][lane] = v;
    __syncthreads();
    const float r = (s[0][lane] + s[1][lane]) + (s[2][lane] + s[3][lane]);
    __syncthreads();
    return r;
}

// status[v]: bit 1 (value 1) a non-finite value among the video's rows, bit 2 (value 2) no rows at all
__global__ __launch_bounds__(256) void vcls_status_kernel(const float* x, const int* offsets, int N, int width, int* status) {
    __shared__ int s_flag;
    const int v = blockIdx.x, tid = threadIdx.x;
    int r0 = offsets[v], n = offsets[v + 1] - r0;
    if (tid == 0) s_flag = 0;
    __syncthreads();
    if (r0 < 0 || n < 0 || (long)r0 + n > N) n = 0;
    const long total = (long)n * width;
    const float* p = x + (long)r0 * width;
    bool bad = false;
    for (long i = tid; i < total; i += 256) bad = bad || !vcls_finite(p[i]);
    if (bad) atomicOr(&s_flag, 1);
    __syncthreads();
    if (tid == 0) status[v] = s_flag | (n == 0 ? 2 : 0);
}

// raw [N][crops][C] -> frm [N][C]: the crops added in order and divided once, or their maximum
__global__ __launch_bounds__(256) void vcls_crop_kernel(const float* raw, float* frm, long total, int crops, int C, int use_max) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const long r = i / C;
    const int c = (int)(i - r * C);
    const float* p = raw + r * crops * C + c;
    float a = p[0];
    if (use_max) {
        for (int j = 1; j < crops; ++j) a = vcls_max(a, p[(long)j * C]);
    } else {
        for (int j = 1; j < crops; ++j) a += p[(long)j * C];
        a = a / (float)crops;
    }
    frm[i] = a;
}

// Window i of (video v, span s) covers the ticks [i * step_s, min(i * step_s + span_s, T_v)); one output row of per-class
// maxima per window, the windows of segment g = v * S + s at the rows win_off[g] ... win_off[g + 1].
__global__ __launch_bounds__(256) void vcls_window_kernel(const float* frm, const int* offsets, const int* win_off, const int* spans,
                                                          const int* steps, int S, int G, int N, int C, long total, float* out) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const int row = (int)(idx / C), c = (int)(idx - (long)row * C);
    const int g = vcls_find(win_off, G, row);
    const int v = g / S, s = g - v * S;
    const int r0 = offsets[v], T = offsets[v + 1] - r0;
    const int span = spans[s], step = steps[s];
    const long t0 = (long)(row - win_off[g]) * step;
    long t1 = t0 + span;
    if (t1 > T) t1 = T;
    float m = __builtin_nanf("");
    if (r0 >= 0 && T >= 0 && (long)r0 + T <= N && t0 >= 0 && t0 < t1) {
        const float* p = frm + ((long)r0 + t0) * C + c;
        m = p[0];
        for (long t = 1; t < t1 - t0; ++t) m = vcls_max(m, p[t * C]);
    }
    out[idx] = m;
}

// Mean of the min(k, n) largest of the n rows of a segment, per class.  Lanes run along classes (coalesced rows), the
// four waves split the rows.  k >= n: a plain sum.
__global__ __launch_bounds__(256) void vcls_topk_kernel(const float* rows, const int* seg_off, const int* ks, int N, int C,
                                                        float* out) {
    __shared__ uint32_t l_key[VCLS_LDS_ROWS * 64];
    __shared__ int s_cnt[2][4][64];
    __shared__ float s_sum[4][64];
    const int g = blockIdx.x, lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int c = blockIdx.y * 64 + lane;
    const bool live = c < C;
    int r0 = seg_off[g], n = seg_off[g + 1] - r0;
    if (r0 < 0 || n < 0 || (long)r0 + n > N) n = 0;
    int k = ks[g];
    if (k > n || k < 1) k = n;
    float* o = out + (long)g * C + c;
    if (n == 0) {      // (uniform over the workgroup)
        if (live && w == 0) *o = __builtin_nanf("");
        return;
    }
    const float* p = rows + (long)r0 * C + c;
    if (k == n) {
        float s = 0.f;
        if (live)
            for (int r = w; r < n; r += 4) s += p[(long)r * C];
        const float tot = vcls_combine(s, s_sum);
        if (live && w == 0) *o = tot / (float)n;
        return;
    }
    const bool in_lds = n <= VCLS_LDS_ROWS;
    if (in_lds)
        for (int r = w; r < n; r += 4) l_key[r * 64 + lane] = live ? vcls_key(p[(long)r * C]) : 0u;
    __syncthreads();
    // the k-th largest key: the largest t with count(key >= t) >= k, one bit per pass from the top
    uint32_t t = 0;
    for (int bit = 31; bit >= 0; --bit) {
        const uint32_t cand = t | (1u << bit);
        int cnt = 0;
        if (in_lds) {
            for (int r = w; r < n; r += 4) cnt += l_key[r * 64 + lane] >= cand ? 1 : 0;
        } else if (live) {
            for (int r = w; r < n; r += 4) cnt += vcls_key(p[(long)r * C]) >= cand ? 1 : 0;
        }
        int(*buf)[64] = s_cnt[bit & 1];      // two buffers: one barrier per pass is enough
        buf[w][lane] = cnt;
        __syncthreads();
        if (buf[0][lane] + buf[1][lane] + buf[2][lane] + buf[3][lane] >= k) t = cand;
    }
    float s = 0.f;
    int above = 0;
    if (in_lds) {
        for (int r = w; r < n; r += 4) {
            const uint32_t key = l_key[r * 64 + lane];
            if (key > t) {
                s += vcls_unkey(key);
                ++above;
            }
        }
    } else if (live) {
        for (int r = w; r < n; r += 4) {
            const float x = p[(long)r * C];
            if (vcls_key(x) > t) {
                s += x;
                ++above;
            }
        }
    }
    __syncthreads();
    s_cnt[0][w][lane] = above;
    const float tot = vcls_combine(s, s_sum);      // (its first barrier publishes the counts as well)
    const int n_above = s_cnt[0][0][lane] + s_cnt[0][1][lane] + s_cnt[0][2][lane] + s_cnt[0][3][lane];
    if (live && w == 0) *o = (tot + (float)(k - n_above) * vcls_unkey(t)) / (float)k;
}

// tpp_aggregation_func: out[c] = (1 / T) sum_t frm[t][k_t * C + c], k_t = int(t * (stages / T)) in fp64
__global__ __launch_bounds__(256) void vcls_tpp_kernel(const float* frm, const int* offsets, int N, int C, int stages, float* out) {
    __shared__ float s_sum[4][64];
    const int v = blockIdx.x, lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int c = blockIdx.y * 64 + lane;
    const bool live = c < C;
    int r0 = offsets[v], T = offsets[v + 1] - r0;
    if (r0 < 0 || T < 0 || (long)r0 + T > N) T = 0;
    float* o = out + (long)v * C + c;
    if (T == 0) {
        if (live && w == 0) *o = __builtin_nanf("");
        return;
    }
    const double step = (double)stages / (double)T;
    const long width = (long)stages * C;
    float s = 0.f;
    if (live)
        for (int t = w; t < T; t += 4) {
            int kt = (int)((double)t * step);
            kt = kt < 0 ? 0 : (kt >= stages ? stages - 1 : kt);
            s += frm[((long)r0 + t) * width + (long)kt * C + c];
        }
    const float tot = vcls_combine(s, s_sum);
    if (live && w == 0) *o = tot / (float)T;
}

// out[v][c] = in[v][0][c] + sum_{s >= 1} (weights ? weights[s - 1] : 1) * in[v][s][c], added in order, divided by S when
// `divide`; a flagged video's row is NaN; then the optional softmax exp(x - max) / sum along C.
__global__ __launch_bounds__(256) void vcls_finish_kernel(const float* in, const float* weights, const int* status, int S, int C,
                                                          long stride_v, long stride_s, int divide, int softmax, float* out) {
    __shared__ float s_red[4];
    const int v = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const bool bad = status && status[v] != 0;
    const float* p = in + (long)v * stride_v;
    float* o = out + (long)v * C;
    float m = -INFINITY;
    for (int c = tid; c < C; c += 256) {
        float x = p[c];
        for (int s = 1; s < S; ++s) {
            float term = p[(long)s * stride_s + c];
            if (weights) term = term * weights[s - 1];
            x += term;
        }
        if (divide) x = x / (float)S;
        if (bad) x = __builtin_nanf("");
        o[c] = x;
        m = fmaxf(m, x);
    }
    if (!softmax) return;      // (uniform)
    m = wave_max(m);
    if (lane == 0) s_red[w] = m;
    __syncthreads();
    m = fmaxf(fmaxf(s_red[0], s_red[1]), fmaxf(s_red[2], s_red[3]));
    __syncthreads();
    float sum = 0.f;
    for (int c = tid; c < C; c += 256) {
        const float e = expf(o[c] - m);      // (o[c]: this thread's own store)
        o[c] = e;
        sum += e;
    }
    sum = wave_sum(sum);
    if (lane == 0) s_red[w] = sum;
    __syncthreads();
    sum = (s_red[0] + s_red[1]) + (s_red[2] + s_red[3]);
    for (int c = tid; c < C; c += 256) o[c] = o[c] / sum;
}

// ---- metrics ----
// counts: hits [K], cls_hit [C], cls_tot [C], cls_pred [C].  One workgroup per video.  The rank of class c from the top
// in the STABLE ascending order (of equal scores the higher class index ranks higher) is #{s_j > s_c} + #{j > c, s_j ==
// s_c}; the video hits at k when one of its label classes has a rank below k.  The prediction is the first argmax.
__global__ __launch_bounds__(256) void vcls_rank_kernel(const float* scores, const unsigned char* gt, const int* label,
                                                        const int* top_ks, int C, int K, int* counts) {
    __shared__ unsigned int s_best;
    const int v = blockIdx.x, tid = threadIdx.x;
    const float* s = scores + (long)v * C;
    int* hits = counts;
    int* cls_hit = counts + K;
    int* cls_tot = cls_hit + C;
    int* cls_pred = cls_tot + C;
    int lbl = label ? label[v] : -1;
    if (lbl >= C) lbl = -1;
    if (tid == 0) s_best = 0;
    __syncthreads();
    for (int c = tid; c < C; c += 256) {
        const float sc = s[c];
        int above = 0, tie_hi = 0, tie_lo = 0;
        for (int j = 0; j < C; ++j) {
            const float sj = s[j];
            above += sj > sc ? 1 : 0;
            if (sj == sc) {
                tie_hi += j > c ? 1 : 0;
                tie_lo += j < c ? 1 : 0;
            }
        }
        if (gt[(long)v * C + c]) atomicMax(&s_best, (unsigned int)(C - (above + tie_hi)));
        if (above == 0 && tie_lo == 0 && sc == sc) {
            atomicAdd(&cls_pred[c], 1);
            if (c == lbl) atomicAdd(&cls_hit[c], 1);
        }
    }
    __syncthreads();
    if (tid == 0) {
        if (lbl >= 0) atomicAdd(&cls_tot[lbl], 1);
        const int best = (int)s_best;
        if (best > 0)
            for (int k = 0; k < K; ++k)
                if (C - best < top_ks[k]) atomicAdd(&hits[k], 1);
    }
}

// inclusive sum scan over the 256 threads of the workgroup (+ the total)
__device__ __forceinline__ int vcls_scan_sum(int v, int* s_wave, int& total) {
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

// One workgroup per class: the videos sorted by descending score (bitonic, entries = ~key << 32 | positive), the low
// half then replaced by the running count of positives; AP = sum over the ENDS of runs of equal scores of
// (positives in the run / npos) * (positives so far / videos so far), fp64; NaN for a class without a positive video.
__global__ __launch_bounds__(256) void vcls_ap_kernel(const float* scores, const unsigned char* gt, int V, int C, int n2,
                                                      u64* ws, double* ap) {
    __shared__ u64 l_e[VCLS_SORT_LDS];
    __shared__ int s_i[4];
    __shared__ double s_acc[256];
    const int c = blockIdx.x, tid = threadIdx.x;
    u64* e = n2 <= VCLS_SORT_LDS ? l_e : ws + (long)c * n2;
    for (int i = tid; i < n2; i += 256)
        e[i] = i < V ? (((u64)(~vcls_key(scores[(long)i * C + c])) << 32) | (gt[(long)i * C + c] ? 1u : 0u)) : ~0ull;
    __syncthreads();
    for (int k = 2; k <= n2; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = tid; i < n2; i += 256) {
                const int l = i ^ j;
                if (l > i) {
                    const u64 a = e[i], b = e[l];
                    if (((i & k) == 0) != (a < b)) {
                        e[i] = b;
                        e[l] = a;
                    }
                }
            }
            __syncthreads();
        }
    int npos = 0;
    for (int base = 0; base < V; base += 256) {
        const int i = base + tid;
        const int f = i < V ? (int)(e[i] & 1) : 0;
        int total;
        const int incl = vcls_scan_sum(f, s_i, total);
        if (i < V) e[i] = (e[i] & 0xffffffff00000000ull) | (uint32_t)(npos + incl);
        npos += total;
    }
    __syncthreads();
    double acc = 0.0;
    for (int i = tid; i < V; i += 256) {
        const uint32_t hi = (uint32_t)(e[i] >> 32);
        if (i + 1 < V && (uint32_t)(e[i + 1] >> 32) == hi) continue;      // not the end of its run
        int j = i;
        while (j > 0 && (uint32_t)(e[j - 1] >> 32) == hi) --j;
        const int cum = (int)(uint32_t)e[i], prev = j > 0 ? (int)(uint32_t)e[j - 1] : 0;
        acc += ((double)(cum - prev) / (double)npos) * ((double)cum / (double)(i + 1));
    }
    s_acc[tid] = acc;
    __syncthreads();
    if (tid == 0) {
        double sum = 0.0;
        for (int j = 0; j < 256; ++j) sum += s_acc[j];
        ap[c] = npos > 0 ? sum : (double)__builtin_nanf("");
    }
}

// numpy's pairwise summation (what np.mean adds with): below 8 in order; up to 128 eight running sums joined as a
// tree and the tail in order; above that split at n / 2 rounded down to a multiple of 8.
__device__ double vcls_np_leaf(const double* a, int n) {
    if (n < 8) {
        double r = 0.0;
        for (int i = 0; i < n; ++i) r += a[i];
        return r;
    }
    double r[8];
    for (int j = 0; j < 8; ++j) r[j] = a[j];
    int i = 8;
    for (; i < n - (n % 8); i += 8)
        for (int j = 0; j < 8; ++j) r[j] += a[i + j];
    double res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
    for (; i < n; ++i) res += a[i];
    return res;
}
// (the recursion left + right written with an explicit stack: n <= 2^20 gives at most 14 levels)
__device__ double vcls_np_sum(const double* a, int n) {
    struct Frame {
        int off, n, state;
        double left;
    } st[24];
    int sp = 0;
    double ret = 0.0;
    st[0] = Frame{0, n, 0, 0.0};
    while (sp >= 0) {
        Frame& f = st[sp];
        if (f.n <= 128) {
            ret = vcls_np_leaf(a + f.off, f.n);
            --sp;
            continue;
        }
        int n2 = f.n / 2;
        n2 -= n2 % 8;
        if (f.state == 0) {
            f.state = 1;
            st[sp + 1] = Frame{f.off, n2, 0, 0.0};
            ++sp;
        } else if (f.state == 1) {
            f.left = ret;
            f.state = 2;
            st[sp + 1] = Frame{f.off + n2, f.n - n2, 0, 0.0};
            ++sp;
        } else {
            ret = f.left + ret;
            --sp;
        }
    }
    return ret;
}

// results: [K] top-k hit rates, [K] mean AP, [K + 1] mean class accuracy (hit / total over the classes that occur among
// labels or predictions; a class that is only predicted gives 0 / 0 = NaN, as the reference's confusion matrix does)
__global__ void vcls_metrics_final_kernel(const int* counts, const double* ap, int V, int C, int K, double* tmp, double* results) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const int* hits = counts;
    const int* cls_hit = counts + K;
    const int* cls_tot = cls_hit + C;
    const int* cls_pred = cls_tot + C;
    for (int k = 0; k < K; ++k) results[k] = (double)hits[k] / (double)V;
    results[K] = vcls_np_sum(ap, C) / (double)C;
    int m = 0;
    for (int c = 0; c < C; ++c)
        if (cls_tot[c] > 0 || cls_pred[c] > 0) tmp[m++] = (double)cls_hit[c] / (double)cls_tot[c];
    results[K + 1] = vcls_np_sum(tmp, m) / (double)m;
}

inline unsigned vcls_blocks(long total) { return (unsigned)((total + 255) / 256); }

}  // namespace

// Rows of one segment whose keys ssn_vcls_topk_mean stages in LDS; longer segments are streamed from memory in every pass.
extern "C" int ssn_vcls_lds_rows(void) { return VCLS_LDS_ROWS; }

// Device scratch of ssn_vcls_metrics: C fp64 for the class accuracies, and C * pow2(V) sort entries when V does not fit LDS.
extern "C" size_t ssn_vcls_metrics_workspace_bytes(int V, int C) {
    if (V < 1 || C < 1) return 0;
    size_t n2 = 1;
    while (n2 < (size_t)V) n2 <<= 1;
    return 8 * (size_t)C + (n2 > (size_t)VCLS_SORT_LDS ? 8 * (size_t)C * n2 : 0);
}

// status [V] int32 <- 1 where a row of the video holds a non-finite value, 2 where the video has no rows.  x [N][width].
extern "C" int ssn_vcls_status(const float* x, const int* offsets, int V, int N, int width, int* status, hipStream_t stream) {
    SSN_CHECK_ARG(V >= 1 && N >= 0 && width >= 1, "vcls_status: bad sizes");
    SSN_CHECK_ARG(offsets && status && (N == 0 || x), "vcls_status: null pointer");
    hipLaunchKernelGGL(vcls_status_kernel, dim3((unsigned)V), dim3(256), 0, stream, x, offsets, N, width, status);
    SSN_CHECK_LAUNCH("vcls_status");
    return SSN_OK;
}

// raw [N][crops][C] -> frm [N][C]; use_max 0: mean (crops added in order, one division), 1: maximum.
extern "C" int ssn_vcls_crop_reduce(const float* raw, float* frm, int N, int crops, int C, int use_max, hipStream_t stream) {
    SSN_CHECK_ARG(N >= 0 && crops >= 1 && C >= 1 && (long)N * C < (1L << 38), "vcls_crop_reduce: bad sizes");
    if (N == 0) return SSN_OK;
    SSN_CHECK_ARG(raw && frm, "vcls_crop_reduce: null pointer");
    const long total = (long)N * C;
    hipLaunchKernelGGL(vcls_crop_kernel, dim3(vcls_blocks(total)), dim3(256), 0, stream, raw, frm, total, crops, C, use_max);
    SSN_CHECK_LAUNCH("vcls_crop_reduce");
    return SSN_OK;
}

// frm [N][C] ragged by offsets [V + 1]; spans / steps [S] int32; win_off [V * S + 1] int32: exclusive prefix sums of
// ceil(T_v / step_s) (0 for an empty video), segment v * S + s.  out [W][C], W = win_off[V * S].  All device memory.
extern "C" int ssn_vcls_window_max(const float* frm, const int* offsets, const int* win_off, const int* spans, const int* steps,
                                   int V, int S, int N, int C, int W, float* out, hipStream_t stream) {
    SSN_CHECK_ARG(V >= 1 && S >= 1 && N >= 0 && C >= 1 && W >= 0 && (long)V * S < (1L << 30) && (long)W * C < (1L << 38),
                  "vcls_window_max: bad sizes");
    SSN_CHECK_ARG(offsets && win_off && spans && steps, "vcls_window_max: null pointer");
    if (W == 0) return SSN_OK;
    SSN_CHECK_ARG(frm && out, "vcls_window_max: null pointer");
    const long total = (long)W * C;
    hipLaunchKernelGGL(vcls_window_kernel, dim3(vcls_blocks(total)), dim3(256), 0, stream, frm, offsets, win_off, spans, steps, S,
                       V * S, N, C, total, out);
    SSN_CHECK_LAUNCH("vcls_window_max");
    return SSN_OK;
}

// out [G][C] <- per class the mean of the min(ks[g], n_g) largest of the rows seg_off[g] ... seg_off[g + 1] of rows [N][C]
// (NaN for a segment without rows).
extern "C" int ssn_vcls_topk_mean(const float* rows, const int* seg_off, const int* ks, int G, int N, int C, float* out,
                                  hipStream_t stream) {
    SSN_CHECK_ARG(G >= 1 && G < 65536 * 1024 && N >= 0 && C >= 1 && C <= 64 * 65535, "vcls_topk_mean: bad sizes");
    SSN_CHECK_ARG(seg_off && ks && out && (N == 0 || rows), "vcls_topk_mean: null pointer");
    hipLaunchKernelGGL(vcls_topk_kernel, dim3((unsigned)G, (unsigned)((C + 63) / 64)), dim3(256), 0, stream, rows, seg_off, ks, N,
                       C, out);
    SSN_CHECK_LAUNCH("vcls_topk_mean");
    return SSN_OK;
}

// frm [N][stages * C] ragged by offsets [V + 1] -> out [V][C]
extern "C" int ssn_vcls_tpp(const float* frm, const int* offsets, int V, int N, int C, int stages, float* out, hipStream_t stream) {
    SSN_CHECK_ARG(V >= 1 && N >= 0 && C >= 1 && C <= 64 * 65535 && stages >= 1 && (long)stages * C < (1L << 30),
                  "vcls_tpp: bad sizes");
    SSN_CHECK_ARG(offsets && out && (N == 0 || frm), "vcls_tpp: null pointer");
    hipLaunchKernelGGL(vcls_tpp_kernel, dim3((unsigned)V, (unsigned)((C + 63) / 64)), dim3(256), 0, stream, frm, offsets, N, C,
                       stages, out);
    SSN_CHECK_LAUNCH("vcls_tpp");
    return SSN_OK;
}

// out [V][C] from S terms per video: term s of video v at in + v * stride_v + s * stride_s (floats).  weights NULL: the
// terms are added in order (and divided by S when `divide`); weights [S - 1]: term 0 + sum weights[s - 1] * term s.
// status [V] or NULL: a non-zero entry makes the row NaN.  softmax: exp(x - max) / sum along C afterwards.
extern "C" int ssn_vcls_finish(const float* in, const float* weights, const int* status, int V, int S, int C, long stride_v,
                               long stride_s, int divide, int softmax, float* out, hipStream_t stream) {
    SSN_CHECK_ARG(V >= 1 && S >= 1 && C >= 1 && stride_v >= 0 && stride_s >= 0, "vcls_finish: bad sizes");
    SSN_CHECK_ARG(in && out, "vcls_finish: null pointer");
    hipLaunchKernelGGL(vcls_finish_kernel, dim3((unsigned)V), dim3(256), 0, stream, in, weights, status, S, C, stride_v, stride_s,
                       divide, softmax, out);
    SSN_CHECK_LAUNCH("vcls_finish");
    return SSN_OK;
}

// scores [V][C] fp32, gt [V][C] uint8 (1: the class is a label of the video), label [V] int32 or NULL (the single label,
// for the class accuracy), top_ks [K] int32 -> counts [K + 3 C] int32 (hits, class hits, class totals, class predictions),
// ap [C] fp64, results [K + 2] fp64 (top-k hit rates, mean AP, mean class accuracy).  All device memory.
extern "C" int ssn_vcls_metrics(const float* scores, const unsigned char* gt, const int* label, const int* top_ks, int V, int C,
                                int K, int* counts, double* ap, double* results, void* workspace, size_t ws_bytes,
                                hipStream_t stream) {
    SSN_CHECK_ARG(V >= 1 && V <= (1 << 24) && C >= 1 && C <= (1 << 20) && K >= 0 && K <= 64, "vcls_metrics: bad sizes");
    SSN_CHECK_ARG(scores && gt && counts && ap && results && workspace && (K == 0 || top_ks), "vcls_metrics: null pointer");
    if (ws_bytes < ssn_vcls_metrics_workspace_bytes(V, C)) {
        ssn_set_error("vcls_metrics: workspace of %zu bytes, %zu needed", ws_bytes, ssn_vcls_metrics_workspace_bytes(V, C));
        return SSN_ERR_WORKSPACE;
    }
    if (hipMemsetAsync(counts, 0, sizeof(int) * ((size_t)K + 3 * (size_t)C), stream) != hipSuccess) {
        ssn_set_error("vcls_metrics: memset failed");
        return SSN_ERR_LAUNCH;
    }
    int n2 = 1;
    while (n2 < V) n2 <<= 1;
    double* tmp = (double*)workspace;
    u64* sort_ws = (u64*)(tmp + C);
    hipLaunchKernelGGL(vcls_rank_kernel, dim3((unsigned)V), dim3(256), 0, stream, scores, gt, label, top_ks, C, K, counts);
    hipLaunchKernelGGL(vcls_ap_kernel, dim3((unsigned)C), dim3(256), 0, stream, scores, gt, V, C, n2, sort_ws, ap);
    hipLaunchKernelGGL(vcls_metrics_final_kernel, dim3(1), dim3(64), 0, stream, (const int*)counts, (const double*)ap, V, C, K, tmp,
                       results);
    SSN_CHECK_LAUNCH("vcls_metrics");
    return SSN_OK;
}
