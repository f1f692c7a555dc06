// Temporal actionness grouping (TAG) for a BATCH of videos on the GPU: the per-video arithmetic of the reference's
// bottom-up proposal script
//   softmax + Gaussian smoothing + thresholding        /root/reference/ops/sequence_funcs.py:11-34 (label_frame_by_threshold)
//   edge search over (threshold, tolerance) pairs      :101-136 (build_box_by_search)
//   temporal NMS, the `+1` form                        :71-97 (temporal_nms_fallback)
//   frames -> seconds and the minimum-length mask      /root/reference/gen_bottom_up_proposals.py:138-141
//   best ground-truth instance of a proposal           /root/reference/ops/detection_metrics.py:54-76 (name_proposal)
// which the reference runs in numpy, video by video in a pool of 32 processes.  Here the scores of all videos are
// concatenated ([sum T][2] fp32 + offsets[V + 1]) and every kernel covers the whole batch: launches and host
// synchronisations per call do not depend on V.  Arithmetic is the reference's: fp32 softmax, fp64 filter rounded to
// fp32, fp64 signal WITHOUT contraction (t * i rounded, then subtracted: a fused multiply-add resolves ties of
// `signal[up[y]] > s` differently from numpy), sequential fp32 box sums in index order, one IEEE fp64 division per IoU.
#include "ssn_common.h"

#pragma clang fp contract(off)

namespace {

constexpr int TAG_MAXN = 2048;        // candidates of one video sorted and suppressed in LDS; more go through the workspace
constexpr int TAG_MAX_RADIUS = 64;    // int(4 * bw + 0.5) of scipy's gaussian_filter (bw = 3: 12)

struct TagFilter {
    int radius;
    double w[TAG_MAX_RADIUS + 1];     // weight at distance d from the centre (the kernel is symmetric)
};

__device__ __forceinline__ uint32_t tag_key(uint32_t b) {       // total order on fp32 bit patterns, NaN on top (det_key of detect.hip)
    if ((b & 0x7fffffffu) > 0x7f800000u) return 0xffffffffu;
    return (b >> 31) ? ~b : (b | 0x80000000u);
}

// video of concatenated index i: the largest v with off[v] <= i (off is non-decreasing, off[0] = 0 <= i < off[V])
__device__ __forceinline__ int tag_find(const int* off, int V, int i) {
    int lo = 0, hi = V - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (off[mid] <= i) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// fp32 softmax over the two columns, foreground probability (ops/metrics.py:8-11: exp(x - max) / sum)
__global__ __launch_bounds__(256) void tag_prob_kernel(const float* scores, float* prob, int n) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float a = scores[2 * (long)i], b = scores[2 * (long)i + 1];
    const float m = fmaxf(a, b);
    const float ea = expf(a - m), eb = expf(b - m);
    prob[i] = eb / (ea + eb);
}

// scipy.ndimage.gaussian_filter(prob, bw), mode 'reflect' (d c b a | a b c d | d c b a, periodic for any T >= 1): the
// line in fp64, centre tap first, then the pairs from the outermost inwards, result rounded to fp32
__global__ __launch_bounds__(256) void tag_smooth_kernel(const float* prob, const int* off, int V, int n, TagFilter f,
                                                         float* smoothed) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int v = tag_find(off, V, i);
    int t0 = off[v], t1 = off[v + 1];
    t0 = t0 < 0 ? 0 : t0;
    t1 = t1 > n ? n : t1;
    const int T = t1 - t0, c = i - t0;
    if (T < 1 || c < 0 || c >= T) return;
    const int period = 2 * T;
    double acc = (double)prob[i] * f.w[0];
    for (int d = f.radius; d >= 1; --d) {
        int l = (c - d) % period, r = (c + d) % period;
        if (l < 0) l += period;
        l = l < T ? l : period - 1 - l;
        r = r < T ? r : period - 1 - r;
        acc += ((double)prob[t0 + l] + (double)prob[t0 + r]) * f.w[d];
    }
    smoothed[i] = (float)acc;
}

struct TagRow {
    const float* sm;     // smoothed probabilities of this video
    int t0, T;
    float th;
    __device__ __forceinline__ bool label(int i) const { return sm[i] > th; }      // NaN: background
};

__device__ __forceinline__ bool tag_row(const float* smoothed, const int* off, int n, const float* thresholds, int v, int k,
                                        TagRow& r) {
    const int t0 = off[v], t1 = off[v + 1];
    if (t0 < 0 || t1 > n || t1 <= t0) return false;
    r.sm = smoothed + t0;
    r.t0 = t0;
    r.T = t1 - t0;
    r.th = thresholds[k];
    return true;
}

// counting phase: number of foreground runs of every (video, threshold) label row (+ the label rows themselves)
__global__ __launch_bounds__(256) void tag_count_kernel(const float* smoothed, const int* off, int n, const float* thresholds,
                                                        int n_thr, unsigned char* labels, int* runs) {
    __shared__ int s_u;
    const int row = blockIdx.x, v = row / n_thr, k = row - v * n_thr, tid = threadIdx.x;
    if (tid == 0) s_u = 0;
    __syncthreads();
    TagRow r;
    if (tag_row(smoothed, off, n, thresholds, v, k, r)) {
        int u = 0;
        for (int i = tid; i < r.T; i += 256) {
            const bool l = r.label(i);
            if (labels) labels[(long)k * n + r.t0 + i] = (unsigned char)l;
            u += l && (i == 0 || !r.label(i - 1));
        }
        if (u) atomicAdd(&s_u, u);
    }
    __syncthreads();
    if (tid == 0) runs[row] = s_u;
}

// exclusive scan of one int per thread over the 256 threads of the workgroup (+ the total)
__device__ __forceinline__ int tag_block_scan(int v, int* s_wave, int& total) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    int inc = v;
    for (int d = 1; d < 64; d <<= 1) {
        const int o = __shfl(inc, lane >= d ? lane - d : lane, 64);
        if (lane >= d) inc += o;
    }
    __syncthreads();                 // (the readers of the previous scan's s_wave are done)
    if (lane == 63) s_wave[w] = inc;
    __syncthreads();
    int base = 0;
    total = 0;
    for (int j = 0; j < 4; ++j) {
        if (j < w) base += s_wave[j];
        total += s_wave[j];
    }
    return base + inc - v;
}

struct TagGroupArgs {
    const float* scores;      // [n][2]: column 1 is the raw foreground score that is summed
    const float* smoothed;    // [n]
    const int* off;           // [V + 1]
    const float* thresholds;  // [n_thr]
    const double* tol;        // [n_tol]
    const int* run_off;       // [V * n_thr + 1] prefix sums of the counting phase
    int *up, *down, *bgb;     // [total_runs] workspace: run start, run end (exclusive), background frames before the run
    int* cand_box;            // [2 * n_tol * total_runs][2]
    float* cand_score;
    int n, n_thr, n_tol;
    long total_runs;
};

// grouping: one workgroup per (video, threshold).  Ordered compaction of the rising / falling edges, then the
// 2 * n_tol * U searches of build_box_by_search, one per lane.  cs = cumsum(1 - label) is only read at edges:
// cs[up[x]] = B[x] (background frames before run x), cs[down[x]] = B[x] + 1 for down[x] < T, and cs[T - 1] = B[U - 1] when
// the last run touches the end.
__global__ __launch_bounds__(256) void tag_group_kernel(TagGroupArgs a) {
    __shared__ int s_wave[4];
    const int row = blockIdx.x, v = row / a.n_thr, k = row - v * a.n_thr, tid = threadIdx.x;
    TagRow r;
    if (!tag_row(a.smoothed, a.off, a.n, a.thresholds, v, k, r)) return;
    const int T = r.T;
    const long rbase = a.run_off[row];
    const long U_want = (long)a.run_off[row + 1] - rbase;
    // thread tid owns frames [lo, hi): their rising edges, the falling edges right behind them and their background count
    const int L = (T + 255) >> 8;
    const int lo = tid * L < T ? tid * L : T, hi = lo + L < T ? lo + L : T;
    int nu = 0, nb = 0;
    for (int i = lo; i < hi; ++i) {
        const bool l = r.label(i);
        nu += l && (i == 0 || !r.label(i - 1));
        nb += !l;
    }
    int U, B;
    int u = tag_block_scan(nu, s_wave, U);
    int b = tag_block_scan(nb, s_wave, B);
    if (U == 0 || (long)U != U_want || rbase < 0 || rbase + U > a.total_runs) return;      // (uniform) table and labels disagree: write nothing
    int* up = a.up + rbase;
    int* down = a.down + rbase;
    int* bgb = a.bgb + rbase;
    for (int i = lo; i < hi; ++i) {
        const bool l = r.label(i);
        if (l && (i == 0 || !r.label(i - 1))) {
            up[u] = i;
            bgb[u] = b;
            ++u;
        }
        // the run that ends behind frame i is the one whose rising edge is the last at or before i: index u - 1 >= 0
        if (l && (i == T - 1 || !r.label(i + 1))) down[u - 1] = i + 1;
        b += !l;
    }
    __syncthreads();
    const float* frm = a.scores + 2 * (long)r.t0 + 1;       // frm[2 * i] = scores[t0 + i][1]
    const long cbase = 2L * a.n_tol * rbase;
    const int work = 2 * a.n_tol * U;
    for (int w = tid; w < work; w += 256) {
        const int ti = w / (2 * U), rem = w - ti * 2 * U;
        const double t = a.tol[ti];
        int start, end, s0, s1;
        if (rem < U) {              // forward from up[x]  (sequence_funcs.py:118-125)
            const int x = rem;
            const double s = (double)bgb[x] - t * (double)up[x];
            int y = x + 1;
            for (; y < U; ++y)
                if ((double)bgb[y] - t * (double)up[y] > s) break;
            start = up[x];
            end = down[y - 1] + 1;           // found: down[y - 1] + 1; fall-through (y == U): down[-1] + 1
            s0 = start;
            s1 = end;
        } else {                    // backward from down[x], x descending  (:127-134)
            const int x = 2 * U - 1 - rem;
            const int dx = down[x];
            const double s = dx < T ? (double)(bgb[x] + 1) - t * (double)dx : ((double)bgb[x] - t * (double)(T - 1)) - t;
            int y = x - 1;
            for (; y >= 0; --y)
                if ((double)(bgb[y] + 1) - t * (double)down[y] < s) break;
            end = dx + 1;
            if (y >= 0) {
                start = up[y + 1];
                s0 = start;
                s1 = end;
            } else {                // the fall-through branch sums frm_scores[0 : down[x] + 2]
                start = up[0];
                s0 = 0;
                s1 = dx + 2;
            }
        }
        if (s1 > T) s1 = T;         // Python slicing clamps
        float acc = 0.f;
        for (int i = s0; i < s1; ++i) acc += frm[2 * (long)i];
        const long slot = cbase + w;
        a.cand_box[2 * slot] = start;
        a.cand_box[2 * slot + 1] = end;
        a.cand_score[slot] = acc;
    }
}

struct TagNmsArgs {
    const int* off;
    const double* durations;   // [V] seconds
    const int* run_off;
    const long* sort_off;      // [V + 1] entries of the sort workspace in front of video v (videos with N <= TAG_MAXN take none)
    const int* cand_box;
    const float* cand_score;
    int* kept_box;             // [total_cand][2], the boxes of video v from its candidate base on
    float* kept_score;
    double* seconds;           // [total_cand][2]
    unsigned char* longer;     // [total_cand] span > minimum_len
    int* kept_count;           // [V]
    uint32_t* g_bits;          // sort workspace: [sort_entries] each
    int *g_s, *g_e;
    unsigned char* g_supp;
    int n, n_thr, n_tol;
    long total_runs, sort_entries;
    double nms_thresh, minimum_len;
};

__device__ __forceinline__ int tag_pow2(int n) {
    int n2 = 1;
    while (n2 < n) n2 <<= 1;
    return n2;
}

// One workgroup per video: sort its candidates (descending score on the total order of tag_key; equal scores: smaller
// start, then smaller end, first), greedy NMS with durations and intersections counted as `+ 1` and not clamped at
// zero, IoU <= thresh survives.  IN_LDS handles the videos with at most TAG_MAXN candidates, the other instantiation
// the rest (arrays in the caller's workspace); each skips the videos of the other.
template <bool IN_LDS>
__global__ __launch_bounds__(256) void tag_nms_kernel(TagNmsArgs a) {
    constexpr int LN = IN_LDS ? TAG_MAXN : 1;
    __shared__ uint32_t l_bits[LN];
    __shared__ int l_s[LN], l_e[LN];
    __shared__ unsigned char l_supp[LN];
    __shared__ int s_keep;
    const int v = blockIdx.x, tid = threadIdx.x;
    const long rb = a.run_off[(long)v * a.n_thr], re = a.run_off[((long)v + 1) * a.n_thr];
    if (rb < 0 || re < rb || re > a.total_runs) return;
    const long nl = 2L * a.n_tol * (re - rb);
    if ((nl <= TAG_MAXN) != IN_LDS || nl == 0 || nl > (1L << 30)) return;      // (kept_count was zeroed by the host)
    const int n = (int)nl, n2 = tag_pow2(n);
    const long cbase = 2L * a.n_tol * rb;
    long so = 0;
    if (!IN_LDS) {
        so = a.sort_off[v];
        if (so < 0 || so + n2 > a.sort_entries) return;
    }
    uint32_t* bits = IN_LDS ? l_bits : a.g_bits + so;
    int* bs = IN_LDS ? l_s : a.g_s + so;
    int* be = IN_LDS ? l_e : a.g_e + so;
    unsigned char* supp = IN_LDS ? l_supp : a.g_supp + so;
    const int T = a.off[v + 1] - a.off[v];
    if (tid == 0) s_keep = 0;
    for (int i = tid; i < n2; i += 256) {
        if (i < n) {
            bits[i] = __builtin_bit_cast(uint32_t, a.cand_score[cbase + i]);
            bs[i] = a.cand_box[2 * (cbase + i)];
            be[i] = a.cand_box[2 * (cbase + i) + 1];
        } else {                     // padding: the lowest key, and behind every real entry that has it
            bits[i] = 0xff800000u;
            bs[i] = 0x7fffffff;
            be[i] = 0x7fffffff;
        }
        supp[i] = 0;
    }
    __syncthreads();
    for (int k = 2; k <= n2; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = tid; i < n2; i += 256) {
                const int l = i ^ j;
                if (l > i) {
                    const bool desc = (i & k) == 0;
                    const uint32_t bi = bits[i], bl = bits[l];
                    const uint32_t ki = tag_key(bi), kl = tag_key(bl);
                    const int si = bs[i], sl = bs[l], ei = be[i], el = be[l];
                    const bool before = ki > kl || (ki == kl && (si < sl || (si == sl && ei < el)));   // i belongs first
                    if (desc != before) {
                        bits[i] = bl;
                        bits[l] = bi;
                        bs[i] = sl;
                        bs[l] = si;
                        be[i] = el;
                        be[l] = ei;
                    }
                }
            }
            __syncthreads();
        }
    const double dT = (double)T, dur = a.durations[v];
    for (int i = 0; i < n; ++i) {
        if (supp[i]) continue;       // uniform: supp[i] was settled before the last barrier
        const int a1 = bs[i], a2 = be[i];
        const long da = (long)a2 - a1 + 1;
        for (int j = i + 1 + tid; j < n; j += 256) {
            const int b1 = bs[j], b2 = be[j];
            const long tt1 = a1 > b1 ? a1 : b1, tt2 = a2 < b2 ? a2 : b2;
            const long inter = tt2 - tt1 + 1;
            const double iou = (double)inter / (double)(da + ((long)b2 - b1 + 1) - inter);
            if (!(iou <= a.nms_thresh)) supp[j] = 1;
        }
        if (tid == 0) {
            const long o = cbase + s_keep++;           // s_keep <= n: inside this video's candidate range
            a.kept_box[2 * o] = a1;
            a.kept_box[2 * o + 1] = a2;
            a.kept_score[o] = __builtin_bit_cast(float, bits[i]);
            const double s0 = (double)a1 / dT * dur, s1 = (double)a2 / dT * dur;     // x / float(T) * duration
            a.seconds[2 * o] = s0;
            a.seconds[2 * o + 1] = s1;
            a.longer[o] = (unsigned char)(s1 - s0 > a.minimum_len);
        }
        __syncthreads();
    }
    if (tid == 0) a.kept_count[v] = s_keep;
}

// Python's two-argument max / min: the first argument unless the second compares greater / smaller (NaN: the first)
__device__ __forceinline__ double tag_pymax(double x, double y) { return y > x ? y : x; }
__device__ __forceinline__ double tag_pymin(double x, double y) { return y < x ? y : x; }

// name_proposal (detection_metrics.py:54-76), one lane per proposal: the ground-truth instance of its video with the
// largest temporal IoU (first maximum; `ov > thresh and ov > max_overlap`), that IoU and intersection / own length
__global__ __launch_bounds__(256) void tag_name_kernel(const double* gt_span, const int* gt_label, const int* gt_off, int G,
                                                       const double* prop, const int* prop_off, int V, int P, double thresh,
                                                       int* out_label, double* out_iou, double* out_self) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= P) return;
    const int v = tag_find(prop_off, V, p);
    int g0 = gt_off[v], g1 = gt_off[v + 1];
    g0 = g0 < 0 ? 0 : g0;
    g1 = g1 > G ? G : g1;
    const double e0 = prop[2 * (long)p], e1 = prop[2 * (long)p + 1];
    int label = 0;
    double best = 0.0, best_self = 0.0;
    for (int g = g0; g < g1; ++g) {
        const double a0 = gt_span[2 * (long)g], a1 = gt_span[2 * (long)g + 1];
        const double i0 = tag_pymax(a0, e0), i1 = tag_pymin(a1, e1);
        double ov = 0.0, ov_pr = 0.0;
        if (!(i0 >= i1)) {
            const double u0 = tag_pymin(a0, e0), u1 = tag_pymax(a1, e1);
            ov = (i1 - i0) / (u1 - u0);
            ov_pr = (i1 - i0) / (e1 - e0);
        }
        if (ov > thresh && ov > best) {
            label = gt_label[g] + 1;
            best = ov;
            best_self = ov_pr;
        }
    }
    out_label[p] = label;
    out_iou[p] = best;
    out_self[p] = best_self;
}

inline int tag_check_offsets(const int* h, int V, int total) {
    if (h[0] != 0 || h[V] != total) return 0;
    for (int v = 0; v < V; ++v)
        if (h[v + 1] <= h[v]) return 0;
    return 1;
}

}  // namespace

// Candidates of one video that are sorted inside LDS; a video with more needs pow2(candidates) entries of sort workspace.
extern "C" int ssn_tag_lds_candidates(void) { return TAG_MAXN; }

// Device scratch of ssn_tag_generate: three ints per foreground run (run tables) and 16 bytes per sort entry.
extern "C" size_t ssn_tag_workspace_bytes(long total_runs, long sort_entries) {
    if (total_runs < 0 || sort_entries < 0) return 0;
    return 16 + 12 * (size_t)total_runs + 16 * (size_t)sort_entries;
}

// Counting phase.  scores [total_T][2] fp32 (device), h_offsets / d_offsets [V + 1]: the same frame offsets in host and in
// device memory (the host copy is validated before anything is launched), thresholds [n_thr] fp32 (device, already
// rounded to fp32 as numpy compares them), bw: the Gaussian's sigma.  Out: prob, smoothed [total_T] fp32, labels
// [n_thr][total_T] uint8 or NULL, runs [V][n_thr] int32 foreground runs per label row.
extern "C" int ssn_tag_count(const float* scores, const int* h_offsets, const int* d_offsets, int V, int total_T,
                             const float* thresholds, int n_thr, double bw, float* prob, float* smoothed,
                             unsigned char* labels, int* runs, hipStream_t stream) {
    SSN_CHECK_ARG(scores && h_offsets && d_offsets && thresholds && prob && smoothed && runs, "tag_count: null pointer");
    SSN_CHECK_ARG(V >= 1 && total_T >= 1 && total_T < (1 << 30) && n_thr >= 1 && (long)V * n_thr < (1L << 30),
                  "tag_count: bad sizes");      // (total_T < 2^30: the reflect period 2 * T of one video fits an int)
    SSN_CHECK_ARG(tag_check_offsets(h_offsets, V, total_T),
                  "tag_count: offsets must start at 0, increase strictly and end at the frame count");
    SSN_CHECK_ARG(bw > 0.0 && 4.0 * bw + 0.5 < (double)(TAG_MAX_RADIUS + 1), "tag_count: bw out of range");
    TagFilter f;
    f.radius = (int)(4.0 * bw + 0.5);                     // scipy: truncate = 4.0
    // scipy's weights exp(-x^2 / (2 bw^2)) / sum.  Summed here in index order with libm's exp, where numpy sums pairwise with its
    // own exp: each weight agrees with scipy's to about one ulp of a double, NOT bit for bit.  That moves a smoothed probability by
    // ~1e-16, far below the fp32 rounding that follows; equality of the label rows with the reference's rests on the
    // distance of the inputs from the thresholds (tools/make_tag_golden.py asserts 1e-5), not on these bits.
    double sum = 0.0;
    for (int x = -f.radius; x <= f.radius; ++x) sum += exp(-0.5 / (bw * bw) * (double)(x * x));
    for (int d = 0; d <= TAG_MAX_RADIUS; ++d) f.w[d] = d <= f.radius ? exp(-0.5 / (bw * bw) * (double)(d * d)) / sum : 0.0;
    const unsigned blocks = (unsigned)((total_T + 255) / 256);
    hipLaunchKernelGGL(tag_prob_kernel, dim3(blocks), dim3(256), 0, stream, scores, prob, total_T);
    hipLaunchKernelGGL(tag_smooth_kernel, dim3(blocks), dim3(256), 0, stream, (const float*)prob, d_offsets, V, total_T, f,
                       smoothed);
    hipLaunchKernelGGL(tag_count_kernel, dim3((unsigned)(V * n_thr)), dim3(256), 0, stream, (const float*)smoothed, d_offsets,
                       total_T, thresholds, n_thr, labels, runs);
    SSN_CHECK_LAUNCH("tag_count");
    return SSN_OK;
}

// Generating phase.  run_off [V * n_thr + 1] int32 (device): exclusive prefix sums of `runs`; the candidates of label row r
// are the 2 * n_tol * runs[r] entries from 2 * n_tol * run_off[r] on, in the reference's order.  sort_off [V + 1] int64
// (device): entries of sort workspace in front of video v (pow2(candidates) for a video above ssn_tag_lds_candidates, else
// none).  Out, all indexed like the candidates: cand_box [C][2] int32 + cand_score [C] fp32 (every candidate before NMS),
// kept_box / kept_score (the kept_count[v] survivors of video v from its candidate base on, in NMS order), seconds [C][2]
// fp64 and longer [C] uint8 (span > minimum_len).  A label row whose run count differs from the table writes nothing.
// Unlike the counting phase this call takes no host copy of the offsets: it is meant to follow ssn_tag_count on the
// same d_offsets, and the kernels bound every index they derive from the device tables (a video whose offsets or run
// table are inconsistent yields no boxes instead of an out-of-range access).
extern "C" int ssn_tag_generate(const float* scores, const float* smoothed, const int* d_offsets, const double* durations, int V,
                                int total_T, const float* thresholds, int n_thr, const double* tolerances, int n_tol,
                                const int* run_off, const long* sort_off, long total_runs, long sort_entries, double nms_thresh,
                                double minimum_len, int* cand_box, float* cand_score, int* kept_box, float* kept_score,
                                double* seconds, unsigned char* longer, int* kept_count, void* workspace, size_t ws_bytes,
                                hipStream_t stream) {
    SSN_CHECK_ARG(scores && smoothed && d_offsets && durations && thresholds && tolerances && run_off && sort_off && kept_count,
                  "tag_generate: null pointer");
    SSN_CHECK_ARG(V >= 1 && total_T >= 1 && total_T < (1 << 30) && n_thr >= 1 && n_tol >= 1 && (long)V * n_thr < (1L << 30),
                  "tag_generate: bad sizes");
    SSN_CHECK_ARG(total_runs >= 0 && sort_entries >= 0 && 2L * n_tol * total_runs < (1L << 30) && sort_entries < (1L << 31),
                  "tag_generate: bad table sizes");
    SSN_CHECK_ARG(total_runs == 0 || (cand_box && cand_score && kept_box && kept_score && seconds && longer && workspace),
                  "tag_generate: null pointer");
    if (hipMemsetAsync(kept_count, 0, sizeof(int) * (size_t)V, stream) != hipSuccess) {
        ssn_set_error("tag_generate: memset failed");
        return SSN_ERR_LAUNCH;
    }
    if (total_runs == 0) return SSN_OK;
    if (ws_bytes < ssn_tag_workspace_bytes(total_runs, sort_entries)) {
        ssn_set_error("tag_generate: workspace of %zu bytes, %zu needed", ws_bytes,
                      ssn_tag_workspace_bytes(total_runs, sort_entries));
        return SSN_ERR_WORKSPACE;
    }
    int* wi = (int*)workspace;
    TagGroupArgs g;
    g.scores = scores;
    g.smoothed = smoothed;
    g.off = d_offsets;
    g.thresholds = thresholds;
    g.tol = tolerances;
    g.run_off = run_off;
    g.up = wi;
    g.down = wi + total_runs;
    g.bgb = wi + 2 * total_runs;
    g.cand_box = cand_box;
    g.cand_score = cand_score;
    g.n = total_T;
    g.n_thr = n_thr;
    g.n_tol = n_tol;
    g.total_runs = total_runs;
    hipLaunchKernelGGL(tag_group_kernel, dim3((unsigned)(V * n_thr)), dim3(256), 0, stream, g);
    TagNmsArgs a;
    a.off = d_offsets;
    a.durations = durations;
    a.run_off = run_off;
    a.sort_off = sort_off;
    a.cand_box = cand_box;
    a.cand_score = cand_score;
    a.kept_box = kept_box;
    a.kept_score = kept_score;
    a.seconds = seconds;
    a.longer = longer;
    a.kept_count = kept_count;
    int* ws = wi + 3 * total_runs;
    a.g_bits = (uint32_t*)ws;
    a.g_s = ws + sort_entries;
    a.g_e = ws + 2 * sort_entries;
    a.g_supp = (unsigned char*)(ws + 3 * sort_entries);
    a.n = total_T;
    a.n_thr = n_thr;
    a.n_tol = n_tol;
    a.total_runs = total_runs;
    a.sort_entries = sort_entries;
    a.nms_thresh = nms_thresh;
    a.minimum_len = minimum_len;
    hipLaunchKernelGGL(tag_nms_kernel<true>, dim3((unsigned)V), dim3(256), 0, stream, a);
    if (sort_entries > 0) hipLaunchKernelGGL(tag_nms_kernel<false>, dim3((unsigned)V), dim3(256), 0, stream, a);
    SSN_CHECK_LAUNCH("tag_generate");
    return SSN_OK;
}

// name_proposal for a batch: gt_span [G][2] fp64 + gt_label [G] int32 ragged by gt_off [V + 1], prop [P][2] fp64 ragged by
// prop_off [V + 1] (all device).  Out per proposal: label (ground-truth label + 1, or 0), best IoU, overlap over itself.
extern "C" int ssn_tag_name_proposals(const double* gt_span, const int* gt_label, const int* gt_off, int G, const double* prop,
                                      const int* prop_off, int V, int P, double thresh, int* out_label, double* out_iou,
                                      double* out_self, hipStream_t stream) {
    SSN_CHECK_ARG(V >= 1 && G >= 0 && P >= 0, "tag_name_proposals: bad sizes");
    SSN_CHECK_ARG(gt_off && prop_off, "tag_name_proposals: null pointer");
    SSN_CHECK_ARG(G == 0 || (gt_span && gt_label), "tag_name_proposals: null pointer");
    if (P == 0) return SSN_OK;
    SSN_CHECK_ARG(prop && out_label && out_iou && out_self, "tag_name_proposals: null pointer");
    hipLaunchKernelGGL(tag_name_kernel, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, stream, gt_span, gt_label, gt_off, G,
                       prop, prop_off, V, P, thresh, out_label, out_iou, out_self);
    SSN_CHECK_LAUNCH("tag_name_proposals");
    return SSN_OK;
}
