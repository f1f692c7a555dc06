// The test table of a BATCH of videos: everything the dense tester needs to know about the proposals of a list file,
// formed on the device from the frame-number columns alone
//   which proposals a record keeps        proposal_sampling.VideoRecord.__init__ (end > start, start < frame_cnt; the end
//                                         is cut at frame_cnt); a video that keeps none gets the whole-video row
//   relative spans, ticks, scaling        ProposalSampler.test_ticks (/root/reference/ssn_dataset.py:393-428)
//   STPP row ranges, activity ranges      STPPReorgainzed.host_ranges + the clamps of STPPReorgainzed.forward
//                                         (/root/reference/ops/ssn_ops.py:125-157: np.arange + int(), Python slices)
// All arithmetic is int32 or fp64, every fp64 result is ONE IEEE operation (a division, a multiplication, an addition, a
// subtraction; contraction is off), so the numbers are the host code's bit for bit.  The kept rows are compacted in input
// order with prefix sums (a block scan, a scan of the block totals): no atomics decide a position, two runs write the
// same bytes.  Launches per call do not depend on the number of videos.
#include "ssn_common.h"

#pragma clang fp contract(off)

namespace {

constexpr int TT_MAX_PARTS = 16;
constexpr int TT_BLOCK = 256;

struct TtCfg {
    int n_parts;                 // sum of all parts = rows of `ranges` per proposal
    int n_entries;               // pyramid levels over the three stages
    int stage_entries[3];        // levels of the starting / course / ending stage
    int parts[TT_MAX_PARTS];     // parts of every level, stage by stage
};

// the largest i < n with off[i] <= w (off non-decreasing, off[0] = 0 <= w < off[n]): the video of flat row w
__device__ __forceinline__ int tt_find(const int* off, int n, int w) {
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (off[mid] <= w) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// inclusive prefix sum of x over the 256 lanes of the block (every lane calls it); *total: the block's sum
__device__ __forceinline__ int tt_block_scan(int x, int* total) {
    __shared__ int sh[TT_BLOCK];
    const int t = threadIdx.x;
    sh[t] = x;
    __syncthreads();
    for (int off = 1; off < TT_BLOCK; off <<= 1) {
        const int y = t >= off ? sh[t - off] : 0;
        __syncthreads();
        sh[t] += y;
        __syncthreads();
    }
    const int incl = sh[t];
    *total = sh[TT_BLOCK - 1];
    __syncthreads();            // (the next call overwrites sh)
    return incl;
}

// kept proposals in front of flat row x (0 <= x <= P): block prefix + prefix inside the block
__device__ __forceinline__ int tt_prefix(const int* pre, const int* bp, int nblk, int P, int x) {
    return x < P ? bp[x / TT_BLOCK] + pre[x] : bp[nblk];
}

// One lane per proposal: the keep flag, its exclusive prefix inside the block, the block's total; a negative frame
// number marks the video's word of `counts` (zeroed by the caller).
__global__ __launch_bounds__(TT_BLOCK) void tt_mark_kernel(const int* frames, const int* p_off, int P, const int* frame_cnt,
                                                           int V, int* keep, int* pre, int* bp, int* counts) {
    const long j = (long)blockIdx.x * TT_BLOCK + threadIdx.x;
    int k = 0;
    if (j < P) {
        const int v = tt_find(p_off, V, (int)j);
        const int s = frames[2 * j], e = frames[2 * j + 1];
        if (s < 0 || e < 0) atomicOr(&counts[v], 1);
        k = (e > s && s < frame_cnt[v]) ? 1 : 0;
        keep[j] = k;
    }
    int total;
    const int incl = tt_block_scan(k, &total);
    if (j < P) pre[j] = incl - k;
    if (threadIdx.x == 0) bp[blockIdx.x] = total;
}

// One workgroup: bp [nblk + 1] block totals -> their exclusive prefix sums, the grand total behind them.
__global__ __launch_bounds__(TT_BLOCK) void tt_scan_kernel(int* bp, int nblk) {
    int carry = 0;
    for (int base = 0; base < nblk; base += TT_BLOCK) {
        const int i = base + (int)threadIdx.x;
        const int x = i < nblk ? bp[i] : 0;
        int total;
        const int incl = tt_block_scan(x, &total);
        if (i < nblk) bp[i] = carry + incl - x;
        carry += total;
    }
    if (threadIdx.x == 0) bp[nblk] = carry;
}

// One lane per video: rows of the video = kept proposals, 1 (the whole-video row) when none; -1 when marked.
__global__ __launch_bounds__(TT_BLOCK) void tt_count_kernel(const int* p_off, int P, int V, const int* pre, const int* bp,
                                                            int nblk, int* counts) {
    const int v = blockIdx.x * TT_BLOCK + threadIdx.x;
    if (v >= V) return;
    int b = p_off[v], e = p_off[v + 1];
    b = b < 0 ? 0 : (b > P ? P : b);
    e = e < b ? b : (e > P ? P : e);
    const int kept = tt_prefix(pre, bp, nblk, P, e) - tt_prefix(pre, bp, nblk, P, b);
    counts[v] = counts[v] ? -1 : (kept > 0 ? kept : 1);
}

// element j of np.arange(left, right + 1e-5, step): numpy writes start, start + step, then start + j * (next - start)
__device__ __forceinline__ double tt_arange_at(double first, double step, double delta, int j) {
    if (j == 0) return first;
    if (j == 1) return first + step;
    return first + (double)j * delta;
}

// Row k of the table from the proposal (s, e) of a video with fc frames and n ticks (e already cut at fc).
__device__ __forceinline__ void tt_row(int s, int e, int fc, int n, const TtCfg& cfg, long k, double* rel, int* ticks,
                                       double* scaling, int* ranges, int* act) {
    const double r0 = (double)s / (double)fc, r1 = (double)e / (double)fc;
    const double half = (r1 - r0) * 0.5;                  // starting_ratio = ending_ratio = 0.5
    const double below = r0 - half, above = r1 + half;
    const double lo = below > 0.0 ? below : 0.0;          // max(0.0, .) / min(1.0, .) of Python
    const double hi = above < 1.0 ? above : 1.0;
    const double dn = (double)n;
    int t[4];
    t[0] = (int)(lo * dn);
    t[1] = (int)(r0 * dn);
    t[2] = (int)(r1 * dn);
    t[3] = (int)(hi * dn);
    rel[2 * k] = r0;
    rel[2 * k + 1] = r1;
    for (int i = 0; i < 4; ++i) ticks[4 * k + i] = t[i];
    scaling[2 * k] = (r0 - lo) / half;
    scaling[2 * k + 1] = (hi - r1) / half;

    int a0 = t[1], a1 = t[1] + 1 > t[2] ? t[1] + 1 : t[2];
    a1 = a1 < n ? a1 : n;
    if (a0 >= n) a0 = a1 = -1;
    act[2 * k] = a0;
    act[2 * k + 1] = a1;

    int* rg = ranges + 2 * k * cfg.n_parts;
    int part = 0, ent = 0;
    for (int stage = 0; stage < 3; ++stage) {
        const int left = t[stage];
        const int right = t[stage] + 1 > t[stage + 1] ? t[stage] + 1 : t[stage + 1];
        const bool skipped = right <= 0 || left >= n;
        for (int q = 0; q < cfg.stage_entries[stage] && ent < TT_MAX_PARTS; ++q, ++ent) {
            const int np = cfg.parts[ent];
            const double first = (double)left;
            const double step = (double)(right - left) / (double)np;
            const double delta = (first + step) - first;
            for (int j = 0; j < np && part < cfg.n_parts; ++j, ++part) {
                int pl = 0, pr = 0;
                if (!skipped) {
                    const int x0 = (int)tt_arange_at(first, step, delta, j);
                    const int x1 = (int)tt_arange_at(first, step, delta, j + 1);
                    if (x1 - x0 >= 1) {                                  // a live part: the end is cut at n, a start at or behind n is (-1, -1)
                        pl = x0 >= n ? -1 : x0;
                        pr = x0 >= n ? -1 : (x1 < n ? x1 : n);
                    }
                }
                rg[2 * part] = pl;
                rg[2 * part + 1] = pr;
            }
        }
    }
    for (; part < cfg.n_parts; ++part) rg[2 * part] = rg[2 * part + 1] = 0;
}

// One lane per proposal and, behind them, one per video (its whole-video row when it keeps no proposal).  A kept proposal
// goes to row k_off[v] + (kept proposals of the video in front of it): input order.
__global__ __launch_bounds__(TT_BLOCK) void tt_fill_kernel(const int* frames, const int* p_off, int P, const int* frame_cnt,
                                                           const int* n_rows, int V, const int* keep, const int* pre,
                                                           const int* bp, int nblk, const int* k_off, int K, TtCfg cfg,
                                                           int* src, double* rel, int* ticks, double* scaling, int* ranges,
                                                           int* act) {
    const long r = (long)blockIdx.x * TT_BLOCK + threadIdx.x;
    if (r >= (long)P + V) return;
    int v, s, e, from;
    long k;
    if (r < P) {
        const int j = (int)r;
        if (!keep[j]) return;
        v = tt_find(p_off, V, j);
        int b = p_off[v];
        b = b < 0 ? 0 : (b > P ? P : b);
        k = (long)k_off[v] + (tt_prefix(pre, bp, nblk, P, j) - tt_prefix(pre, bp, nblk, P, b));
        if (k < k_off[v] || k >= k_off[v + 1]) return;                  // tables disagree: leave the row (zero-filled by the caller)
        s = frames[2 * (long)j];
        e = frames[2 * (long)j + 1];
        from = j - b;
    } else {
        v = (int)(r - P);
        int b = p_off[v], en = p_off[v + 1];
        b = b < 0 ? 0 : (b > P ? P : b);
        en = en < b ? b : (en > P ? P : en);
        if (tt_prefix(pre, bp, nblk, P, en) - tt_prefix(pre, bp, nblk, P, b) > 0) return;
        k = k_off[v];
        s = 0;
        e = frame_cnt[v] - 1;                                            // Instance(0, frame_cnt - 1, frame_cnt)
        from = -1;
    }
    if (k < 0 || k >= K) return;
    const int fc = frame_cnt[v], n = n_rows[v];
    if (fc < 2 || n < 1 || s < 0) return;                                // (the host refuses these before any launch)
    e = e < fc ? e : fc;
    src[k] = from;
    tt_row(s, e, fc, n, cfg, k, rel, ticks, scaling, ranges, act);
}

int tt_config(const int* h_stage_entries, const int* h_parts, int n_entries, TtCfg* cfg) {
    SSN_CHECK_ARG(h_stage_entries && h_parts, "test_table_fill: null pointer");
    SSN_CHECK_ARG(n_entries >= 3 && n_entries <= TT_MAX_PARTS, "test_table_fill: %d pyramid levels, 3 ... %d supported", n_entries,
                  TT_MAX_PARTS);
    int sum = 0, total = 0;
    for (int s = 0; s < 3; ++s) {
        SSN_CHECK_ARG(h_stage_entries[s] >= 1 && h_stage_entries[s] <= TT_MAX_PARTS, "test_table_fill: stage %d has %d levels", s,
                      h_stage_entries[s]);
        cfg->stage_entries[s] = h_stage_entries[s];
        sum += h_stage_entries[s];
    }
    SSN_CHECK_ARG(sum == n_entries, "test_table_fill: the stages hold %d levels, %d given", sum, n_entries);
    for (int i = 0; i < TT_MAX_PARTS; ++i) {
        cfg->parts[i] = i < n_entries ? h_parts[i] : 1;
        SSN_CHECK_ARG(cfg->parts[i] >= 1 && cfg->parts[i] <= TT_MAX_PARTS, "test_table_fill: a level of %d parts", cfg->parts[i]);
        if (i < n_entries) total += cfg->parts[i];
    }
    SSN_CHECK_ARG(total <= TT_MAX_PARTS, "test_table_fill: %d parts in total, at most %d supported", total, TT_MAX_PARTS);
    cfg->n_parts = total;
    cfg->n_entries = n_entries;
    return SSN_OK;
}

}  // namespace

// Marking phase: frames [P][2] int32 (start, end as a list file holds them), ragged by p_off [V + 1] int32, frame_cnt [V]
// int32 (all device) -> keep [P] int32 (1: the record keeps the proposal), pre [P] int32 and bp [ceil(P / 256) + 1] int32
// (prefix sums of keep: inside a block of 256 rows / over the blocks, the total last), counts [V] int32: the rows of every
// video in the table (kept proposals, 1 when none), or -1 for a video with a negative frame number.  A memset and three
// launches whatever V and P.
extern "C" int ssn_test_table_mark(const int* frames, const int* p_off, int P, const int* frame_cnt, int V, int* keep, int* pre,
                                   int* bp, int* counts, hipStream_t stream) {
    SSN_CHECK_ARG(V >= 1 && V < (1 << 30) && P >= 0 && P < (1 << 30), "test_table_mark: bad sizes");
    SSN_CHECK_ARG(p_off && frame_cnt && bp && counts, "test_table_mark: null pointer");
    SSN_CHECK_ARG(P == 0 || (frames && keep && pre), "test_table_mark: null pointer");
    const int nblk = (P + TT_BLOCK - 1) / TT_BLOCK;
    if (hipMemsetAsync(counts, 0, sizeof(int) * (size_t)V, stream) != hipSuccess) {
        ssn_set_error("test_table_mark: memset failed");
        return SSN_ERR_LAUNCH;
    }
    if (P > 0) {
        hipLaunchKernelGGL(tt_mark_kernel, dim3((unsigned)nblk), dim3(TT_BLOCK), 0, stream, frames, p_off, P, frame_cnt, V, keep,
                           pre, bp, counts);
        SSN_CHECK_LAUNCH("test_table_mark");
    }
    hipLaunchKernelGGL(tt_scan_kernel, dim3(1), dim3(TT_BLOCK), 0, stream, bp, nblk);
    SSN_CHECK_LAUNCH("test_table_mark (scan)");
    hipLaunchKernelGGL(tt_count_kernel, dim3((unsigned)((V + TT_BLOCK - 1) / TT_BLOCK)), dim3(TT_BLOCK), 0, stream, p_off, P, V,
                       pre, bp, nblk, counts);
    SSN_CHECK_LAUNCH("test_table_mark (count)");
    return SSN_OK;
}

// Filling phase: the outputs of the marking phase, n_rows [V] int32 (ticks of every video) and k_off [V + 1] int32
// (exclusive prefix sums of counts, K last; all device), the STPP configuration on the HOST (h_stage_entries [3] pyramid
// levels per stage, h_parts [n_entries] parts per level, at most 16 parts in total; validated before any launch) ->
// src [K] int32, rel [K][2] fp64, ticks [K][4] int32, scaling [K][2] fp64, ranges [K][n_parts][2] int32, act [K][2] int32.
// A row the tables do not cover is left as it was.  One launch.
extern "C" int ssn_test_table_fill(const int* frames, const int* p_off, int P, const int* frame_cnt, const int* n_rows, int V,
                                   const int* keep, const int* pre, const int* bp, const int* k_off, int K,
                                   const int* h_stage_entries, const int* h_parts, int n_entries, int* src, double* rel,
                                   int* ticks, double* scaling, int* ranges, int* act, hipStream_t stream) {
    TtCfg cfg;
    if (int rc = tt_config(h_stage_entries, h_parts, n_entries, &cfg)) return rc;
    SSN_CHECK_ARG(V >= 1 && V < (1 << 30) && P >= 0 && P < (1 << 30) && K >= V && K <= P + V, "test_table_fill: bad sizes");
    SSN_CHECK_ARG(p_off && frame_cnt && n_rows && bp && k_off && src && rel && ticks && scaling && ranges && act,
                  "test_table_fill: null pointer");
    SSN_CHECK_ARG(P == 0 || (frames && keep && pre), "test_table_fill: null pointer");
    const int nblk = (P + TT_BLOCK - 1) / TT_BLOCK;
    hipLaunchKernelGGL(tt_fill_kernel, dim3((unsigned)(((long)P + V + TT_BLOCK - 1) / TT_BLOCK)), dim3(TT_BLOCK), 0, stream, frames,
                       p_off, P, frame_cnt, n_rows, V, keep, pre, bp, nblk, k_off, K, cfg, src, rel, ticks, scaling, ranges, act);
    SSN_CHECK_LAUNCH("test_table_fill");
    return SSN_OK;
}
