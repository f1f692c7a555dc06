// The TEXT of a proposal-list file for a batch of videos, formed on the device from the arrays the proposal-list stage left
// there (proposal_list.hip, tag.hip): what the reference prints per video and per row in Python
//   the record                         the reference's ops/io.py:95-134 (dump_window_list) under the '# <index>' line of
//                                      its gen_sliding_window_proposals.py:64-67 / gen_bottom_up_proposals.py:188-191
// The text is a flat, video-major sequence of ITEMS; written video k (video v = write[k]) contributes 3 + n_gt + K of them
//   H1   "# <first_index + k>\n" and, behind it, the bytes of the path (copied from the path buffer, never staged)
//   H2   "\n<frame_cnt>\n1\n<n_gt>\n"
//   GT   "<label> <start> <end>\n"                           per ground-truth row
//   CNT  "<K>\n"  ("0\n\n" when K = 0: '\n'.join([]) + '\n' of the reference leaves a blank line)
//   PR   "<label> <iou:.4f> <own:.4f> <start> <end>\n"       per proposal row
// A size pass gives every item's byte length, exclusive prefix sums (a block scan, a scan of the block totals) give its
// position: no atomic decides a position, two runs write the same bytes.  The fill pass formats the items of a workgroup
// into LDS at block-local offsets and streams the staging buffer out with dword stores (consecutive items are consecutive
// in the output; a path cuts the block's range into segments, each copied with its unaligned head and tail as bytes).
//
// '%.4f' of a double is its correctly rounded decimal.  x = m 2^e with m < 2^53 gives x 10^4 = (m 625) 2^(e + 4) with
// m 625 < 2^63, and for |x| < 2^32 the exponent e + 4 is negative: a right shift of -(e + 4) >= 17 bits, rounded half to
// even on the bits shifted out (a shift of 64 or more leaves 0: m 625 < 2^63 is below half of 2^64).  Integer arithmetic
// only.  NaN, +-inf and |x| >= 2^32 print as a placeholder of fixed length and set bit 2 of the video's status word.
// Launches per call do not depend on the number of videos; every index derived from a device table is bounded.
#include "ssn_common.h"

#pragma clang fp contract(off)

namespace {

constexpr int PT_BLOCK = 256;
constexpr int PT_ITEM_MAX = 70;            // a proposal row: 11 + 1 + 16 + 1 + 16 + 1 + 11 + 1 + 11 + 1
constexpr int PT_STATUS_FLOAT = 4;         // bit 2 of status: a float of the video is outside the printable domain

enum { PT_NONE = 0, PT_H1, PT_H2, PT_GT, PT_CNT, PT_PR };

struct PtIn {
    const int* gt_label;      // [G] as written (label + 1)
    const int* gt_frames;     // [G][2]
    const int* gt_off;        // [V + 1]
    const int* label;         // [P]
    const double* iou;        // [P]
    const double* own;        // [P]
    const int* frames;        // [P][2]
    const int* prop_off;      // [V + 1]
    const int* frame_cnt;     // [V]
    const int* path_off;      // [W + 1] into the path buffer, by written video
    const int* write;         // [W] video of every written record
    const int* item_off;      // [W + 1] first item of every written record
    int G, P, V, W, N, first_index;
    long path_bytes;
};

struct PtItem {
    int kind;
    int v;                    // the video (status word)
    int k;                    // the written record
    int iv[3];
    unsigned long long fq[2]; // |x| 10^4, rounded
    int fneg[2], fbad[2];
    int path_src, path_len;
};

// the largest i with off[i] <= w (off non-decreasing, off[0] = 0 <= w < off[n])
__device__ __forceinline__ int pt_find(const int* off, int n, int w) {
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (off[mid] <= w) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// round-half-even(|x| 10^4) of a double given by its bits; false: NaN, inf or |x| >= 2^32
__device__ __forceinline__ bool pt_fixed4(unsigned long long bits, unsigned long long* q, int* neg) {
    const int e = (int)((bits >> 52) & 0x7FFu);
    const unsigned long long frac = bits & 0xFFFFFFFFFFFFFull;
    *neg = (int)(bits >> 63);
    *q = 0;
    if (e >= 1055) return false;                                   // 2^32 has the biased exponent 1055
    const unsigned long long m = e ? (frac | (1ull << 52)) : frac;  // x = m 2^(max(e, 1) - 1075)
    const int sh = 1071 - (e ? e : 1);                             // -(exponent + 4): 17 ... 1070
    if (sh >= 64) return true;
    const unsigned long long p = m * 625ull;                       // < 2^63
    unsigned long long r = p >> sh;
    const unsigned long long rem = p & ((1ull << sh) - 1ull), half = 1ull << (sh - 1);
    if (rem > half || (rem == half && (r & 1ull))) ++r;
    *q = r;
    return true;
}

__device__ __forceinline__ int pt_digits(unsigned long long x) {
    int n = 1;
    while (x >= 10ull) {
        x /= 10ull;
        ++n;
    }
    return n;
}
__device__ __forceinline__ unsigned int pt_mag(int x) { return x < 0 ? 0u - (unsigned int)x : (unsigned int)x; }
__device__ __forceinline__ int pt_int_len(int x) { return pt_digits(pt_mag(x)) + (x < 0 ? 1 : 0); }
__device__ __forceinline__ int pt_float_len(const PtItem& it, int i) {
    if (it.fbad[i]) return 6;
    const int d = pt_digits(it.fq[i]);
    return it.fneg[i] + (d < 5 ? 5 : d) + 1;
}

// digits of x, right-aligned in the n bytes at p (zero-filled on the left)
__device__ __forceinline__ void pt_put_digits(unsigned char* p, int n, unsigned long long x) {
    for (int i = n - 1; i >= 0; --i) {
        p[i] = (unsigned char)('0' + (int)(x % 10ull));
        x /= 10ull;
    }
}
__device__ __forceinline__ unsigned char* pt_put_int(unsigned char* p, int x) {
    if (x < 0) *p++ = '-';
    const unsigned int m = pt_mag(x);
    const int n = pt_digits(m);
    pt_put_digits(p, n, m);
    return p + n;
}
__device__ __forceinline__ unsigned char* pt_put_float(unsigned char* p, const PtItem& it, int i) {
    if (it.fbad[i]) {
        p[0] = '?', p[1] = '.', p[2] = p[3] = p[4] = p[5] = '?';
        return p + 6;
    }
    if (it.fneg[i]) *p++ = '-';
    const unsigned long long q = it.fq[i];
    int d = pt_digits(q);
    d = (d < 5 ? 5 : d) - 4;                             // digits in front of the point
    pt_put_digits(p, d, q / 10000ull);
    p[d] = '.';
    pt_put_digits(p + d + 1, 4, q % 10000ull);
    return p + d + 5;
}

// Item t of the text.  Anything the tables do not cover (a video, a row or a path range outside its array) is PT_NONE, an
// item without bytes.
__device__ __forceinline__ void pt_decode(const PtIn& in, int t, PtItem& it) {
    it.kind = PT_NONE;
    it.path_src = it.path_len = 0;
    it.fbad[0] = it.fbad[1] = 0;
    const int k = pt_find(in.item_off, in.W, t);
    const int r = t - in.item_off[k];
    const int v = in.write[k];
    it.k = k;
    it.v = v;
    if (v < 0 || v >= in.V || r < 0) return;
    const int g0 = in.gt_off[v], n_gt = in.gt_off[v + 1] - g0;
    const int p0 = in.prop_off[v], n_pr = in.prop_off[v + 1] - p0;
    if (n_gt < 0 || n_pr < 0 || g0 < 0 || p0 < 0 || (long)g0 + n_gt > in.G || (long)p0 + n_pr > in.P) return;
    if (r == 0) {
        it.kind = PT_H1;
        it.iv[0] = in.first_index + k;
        const int b = in.path_off[k], e = in.path_off[k + 1];
        if (b >= 0 && e >= b && (long)e <= in.path_bytes) it.path_src = b, it.path_len = e - b;
    } else if (r == 1) {
        it.kind = PT_H2;
        it.iv[0] = in.frame_cnt[v];
        it.iv[1] = n_gt;
    } else if (r < 2 + n_gt) {
        const long j = (long)g0 + (r - 2);
        it.kind = PT_GT;
        it.iv[0] = in.gt_label[j];
        it.iv[1] = in.gt_frames[2 * j];
        it.iv[2] = in.gt_frames[2 * j + 1];
    } else if (r == 2 + n_gt) {
        it.kind = PT_CNT;
        it.iv[0] = n_pr;
    } else if (r - 3 - n_gt < n_pr) {
        const long j = (long)p0 + (r - 3 - n_gt);
        it.kind = PT_PR;
        it.iv[0] = in.label[j];
        it.iv[1] = in.frames[2 * j];
        it.iv[2] = in.frames[2 * j + 1];
        it.fbad[0] = !pt_fixed4(__builtin_bit_cast(unsigned long long, in.iou[j]), &it.fq[0], &it.fneg[0]);
        it.fbad[1] = !pt_fixed4(__builtin_bit_cast(unsigned long long, in.own[j]), &it.fq[1], &it.fneg[1]);
    }
}

// bytes of the item that pass through the staging buffer (all but the path), at most PT_ITEM_MAX
__device__ __forceinline__ int pt_staged_len(const PtItem& it) {
    switch (it.kind) {
    case PT_H1: return 2 + pt_int_len(it.iv[0]) + 1;
    case PT_H2: return 1 + pt_int_len(it.iv[0]) + 3 + pt_int_len(it.iv[1]) + 1;
    case PT_GT: return pt_int_len(it.iv[0]) + 1 + pt_int_len(it.iv[1]) + 1 + pt_int_len(it.iv[2]) + 1;
    case PT_CNT: return pt_int_len(it.iv[0]) + (it.iv[0] == 0 ? 2 : 1);
    case PT_PR:
        return pt_int_len(it.iv[0]) + 1 + pt_float_len(it, 0) + 1 + pt_float_len(it, 1) + 1 + pt_int_len(it.iv[1]) + 1 +
               pt_int_len(it.iv[2]) + 1;
    default: return 0;
    }
}

__device__ __forceinline__ void pt_write(const PtItem& it, unsigned char* p) {
    switch (it.kind) {
    case PT_H1:
        p[0] = '#', p[1] = ' ';
        p = pt_put_int(p + 2, it.iv[0]);
        *p = '\n';
        break;
    case PT_H2:
        *p = '\n';
        p = pt_put_int(p + 1, it.iv[0]);
        p[0] = '\n', p[1] = '1', p[2] = '\n';
        p = pt_put_int(p + 3, it.iv[1]);
        *p = '\n';
        break;
    case PT_GT:
        p = pt_put_int(p, it.iv[0]);
        *p++ = ' ';
        p = pt_put_int(p, it.iv[1]);
        *p++ = ' ';
        p = pt_put_int(p, it.iv[2]);
        *p = '\n';
        break;
    case PT_CNT:
        p = pt_put_int(p, it.iv[0]);
        *p++ = '\n';
        if (it.iv[0] == 0) *p = '\n';
        break;
    case PT_PR:
        p = pt_put_int(p, it.iv[0]);
        *p++ = ' ';
        p = pt_put_float(p, it, 0);
        *p++ = ' ';
        p = pt_put_float(p, it, 1);
        *p++ = ' ';
        p = pt_put_int(p, it.iv[1]);
        *p++ = ' ';
        p = pt_put_int(p, it.iv[2]);
        *p = '\n';
        break;
    default: break;
    }
}

// inclusive prefix sum of x over the 256 lanes of the block (every lane calls it); *total: the block's sum
__device__ __forceinline__ unsigned long long pt_block_scan(unsigned long long x, unsigned long long* total) {
    __shared__ unsigned long long sh[PT_BLOCK];
    const int t = threadIdx.x;
    sh[t] = x;
    __syncthreads();
    for (int off = 1; off < PT_BLOCK; off <<= 1) {
        const unsigned long long y = t >= off ? sh[t - off] : 0ull;
        __syncthreads();
        sh[t] += y;
        __syncthreads();
    }
    const unsigned long long incl = sh[t];
    *total = sh[PT_BLOCK - 1];
    __syncthreads();            // (the next call overwrites sh)
    return incl;
}

// One lane per item: its byte length; the block's total goes to bp [blocks].  A float outside the domain marks its video.
__global__ __launch_bounds__(PT_BLOCK) void pt_size_kernel(PtIn in, int* bp, int* status) {
    const long t = (long)blockIdx.x * PT_BLOCK + threadIdx.x;
    unsigned long long len = 0;
    if (t < in.N) {
        PtItem it;
        pt_decode(in, (int)t, it);
        len = (unsigned long long)(pt_staged_len(it) + it.path_len);
        if (it.fbad[0] | it.fbad[1]) atomicOr(&status[it.v], PT_STATUS_FLOAT);
    }
    unsigned long long total;
    pt_block_scan(len, &total);
    if (threadIdx.x == 0) bp[blockIdx.x] = (int)total;
}

// One workgroup: bp [nblk + 1] block totals -> their exclusive prefix sums, the grand total behind them; -1 in its place
// when it does not fit int32 (the host refuses such a text, the prefix sums are then not used).
__global__ __launch_bounds__(PT_BLOCK) void pt_scan_kernel(int* bp, int nblk) {
    unsigned long long carry = 0;
    for (int base = 0; base < nblk; base += PT_BLOCK) {
        const int i = base + (int)threadIdx.x;
        const unsigned long long x = i < nblk ? (unsigned long long)(unsigned int)bp[i] : 0ull;
        unsigned long long total;
        const unsigned long long incl = pt_block_scan(x, &total);
        if (i < nblk) bp[i] = (int)(carry + incl - x);
        carry += total;
    }
    if (threadIdx.x == 0) bp[nblk] = carry < (1ull << 31) ? (int)carry : -1;
}

// All lanes of the block: n bytes from src to dst, dwords where dst is aligned, the unaligned head and tail as bytes.
__device__ __forceinline__ void pt_copy(unsigned char* dst, const unsigned char* src, int n) {
    const int t = threadIdx.x;
    int head = (int)((4u - (unsigned int)((uintptr_t)dst & 3u)) & 3u);
    if (head > n) head = n;
    if (t < head) dst[t] = src[t];
    const int nd = (n - head) >> 2;
    for (int i = t; i < nd; i += PT_BLOCK) {
        const unsigned char* s = src + head + 4 * i;
        const uint32_t w = (uint32_t)s[0] | ((uint32_t)s[1] << 8) | ((uint32_t)s[2] << 16) | ((uint32_t)s[3] << 24);
        *reinterpret_cast<uint32_t*>(dst + head + 4 * i) = w;
    }
    const int done = head + 4 * nd;
    if (t < n - done) dst[done + t] = src[done + t];
}

// One lane per item.  One scan carries three sums: bytes in the output (bits 0-31; a block holds fewer than 2^30 path
// bytes and 256 * 70 others), staged bytes (bits 32-47; at most 256 * 70) and H1 items (bits 48-56).  An H1 item ends a SEGMENT of the
// block's output range: segment q is the staged bytes [seg_lo[q], seg_lo[q + 1]) at seg_g[q], and -- all but the last --
// the path seg_psrc / seg_plen behind them.
__global__ __launch_bounds__(PT_BLOCK) void pt_fill_kernel(PtIn in, const unsigned char* paths, const int* bp,
                                                           unsigned char* out, long cap, int* rec_off) {
    __shared__ unsigned char stage[PT_BLOCK * PT_ITEM_MAX];
    __shared__ int seg_lo[PT_BLOCK + 2], seg_g[PT_BLOCK + 1], seg_psrc[PT_BLOCK], seg_plen[PT_BLOCK];
    const int tid = threadIdx.x;
    const long t = (long)blockIdx.x * PT_BLOCK + tid;
    PtItem it;
    it.kind = PT_NONE;
    it.path_len = 0;
    int s = 0;
    if (t < in.N) {
        pt_decode(in, (int)t, it);
        s = pt_staged_len(it);
    }
    const int is_h1 = it.kind == PT_H1 ? 1 : 0;
    const unsigned long long mine =
        (unsigned long long)(unsigned int)(s + it.path_len) | ((unsigned long long)s << 32) | ((unsigned long long)is_h1 << 48);
    unsigned long long total;
    const unsigned long long excl = pt_block_scan(mine, &total) - mine;
    const int base = bp[blockIdx.x];
    const int g = base + (int)(unsigned int)(excl & 0xFFFFFFFFull);
    const int lo = (int)((excl >> 32) & 0xFFFFull);
    const int q = (int)(excl >> 48);
    const int n_seg = (int)(total >> 48) + 1;
    if (tid == 0) {
        seg_lo[0] = 0;
        seg_g[0] = base;
        seg_lo[n_seg] = (int)((total >> 32) & 0xFFFFull);
    }
    if (is_h1) {
        seg_lo[q + 1] = lo + s;
        seg_g[q + 1] = g + s + it.path_len;
        seg_psrc[q] = it.path_src;
        seg_plen[q] = it.path_len;
        rec_off[it.k] = g;
    }
    if (t == (long)in.N - 1) rec_off[in.W] = g + s + it.path_len;
    pt_write(it, stage + lo);
    __syncthreads();
    for (int i = 0; i < n_seg; ++i) {
        const int a = seg_lo[i], n = seg_lo[i + 1] - a;
        const long at = seg_g[i];
        if (at < 0 || n < 0) continue;                   // (block-uniform: the tables are shared)
        if (n > 0 && at + n <= cap) pt_copy(out + at, stage + a, n);
        if (i + 1 < n_seg) {
            const int pn = seg_plen[i];
            if (pn > 0 && at + n + pn <= cap) pt_copy(out + at + n, paths + seg_psrc[i], pn);
        }
    }
}

int pt_args(PtIn* in, const int* gt_label, const int* gt_frames, const int* gt_off, int G, const int* label, const double* iou,
            const double* own, const int* frames, const int* prop_off, int P, const int* frame_cnt, int V, const int* path_off,
            long path_bytes, const int* write, const int* item_off, int n_written, int n_items, int first_index, const char* who) {
    SSN_CHECK_ARG(V >= 1 && V < (1 << 30) && G >= 0 && P >= 0 && G < (1 << 30) && P < (1 << 30), "%s: bad sizes", who);
    SSN_CHECK_ARG(n_written >= 1 && n_written < (1 << 28) && path_bytes >= 0 && path_bytes < (1L << 30), "%s: bad sizes", who);
    SSN_CHECK_ARG(n_items >= 3L * n_written && n_items <= (long)n_written * (3L + G + P), "%s: bad sizes", who);      // (3 + n_gt + K items a record)
    SSN_CHECK_ARG(first_index >= 0 && (long)first_index + n_written <= 2147483647L, "%s: bad first index", who);
    SSN_CHECK_ARG(gt_off && prop_off && frame_cnt && path_off && write && item_off, "%s: null pointer", who);
    SSN_CHECK_ARG((G == 0 || (gt_label && gt_frames)) && (P == 0 || (label && iou && own && frames)), "%s: null pointer", who);
    *in = PtIn{gt_label, gt_frames, gt_off, label, iou, own, frames, prop_off, frame_cnt, path_off, write, item_off,
               G, P, V, n_written, n_items, first_index, path_bytes};
    return SSN_OK;
}

}  // namespace

// Size pass of the list text (see the header of this file and include/ssn_hip.h): bp [ceil(n_items / 256) + 1] int32
// receives the exclusive prefix sums of the byte counts of every 256 items and, last, the bytes of the whole text; bit 2
// of status [V] is ORed in for every video with a float outside the printable domain (status is not zeroed here).
extern "C" int ssn_proposal_text_size(const int* gt_label, const int* gt_frames, const int* gt_off, int G, const int* label,
                                      const double* iou, const double* own, const int* frames, const int* prop_off, int P,
                                      const int* frame_cnt, int V, const int* path_off, long path_bytes, const int* write,
                                      const int* item_off, int n_written, int n_items, int first_index, int* bp, int* status,
                                      hipStream_t stream) {
    PtIn in;
    if (int rc = pt_args(&in, gt_label, gt_frames, gt_off, G, label, iou, own, frames, prop_off, P, frame_cnt, V, path_off,
                         path_bytes, write, item_off, n_written, n_items, first_index, "proposal_text_size"))
        return rc;
    SSN_CHECK_ARG(bp && status, "proposal_text_size: null pointer");
    const int nblk = (n_items + PT_BLOCK - 1) / PT_BLOCK;
    hipLaunchKernelGGL(pt_size_kernel, dim3((unsigned)nblk), dim3(PT_BLOCK), 0, stream, in, bp, status);
    SSN_CHECK_LAUNCH("proposal_text_size");
    hipLaunchKernelGGL(pt_scan_kernel, dim3(1), dim3(PT_BLOCK), 0, stream, bp, nblk);
    SSN_CHECK_LAUNCH("proposal_text_size (scan)");
    return SSN_OK;
}

// Fill pass: the same inputs, the path bytes and bp as the size pass left it -> out [out_bytes] uint8 (out_bytes at least
// the total of the size pass; nothing is written at or behind out_bytes) and rec_off [n_written + 1] int32, the first byte
// of every record and the end of the text.
extern "C" int ssn_proposal_text_fill(const int* gt_label, const int* gt_frames, const int* gt_off, int G, const int* label,
                                      const double* iou, const double* own, const int* frames, const int* prop_off, int P,
                                      const int* frame_cnt, int V, const unsigned char* paths, const int* path_off,
                                      long path_bytes, const int* write, const int* item_off, int n_written, int n_items,
                                      int first_index, const int* bp, unsigned char* out, long out_bytes, int* rec_off,
                                      hipStream_t stream) {
    PtIn in;
    if (int rc = pt_args(&in, gt_label, gt_frames, gt_off, G, label, iou, own, frames, prop_off, P, frame_cnt, V, path_off,
                         path_bytes, write, item_off, n_written, n_items, first_index, "proposal_text_fill"))
        return rc;
    SSN_CHECK_ARG(out_bytes >= 0 && out_bytes < (1L << 31), "proposal_text_fill: bad sizes");
    SSN_CHECK_ARG(bp && out && rec_off && (path_bytes == 0 || paths), "proposal_text_fill: null pointer");
    const int nblk = (n_items + PT_BLOCK - 1) / PT_BLOCK;
    hipLaunchKernelGGL(pt_fill_kernel, dim3((unsigned)nblk), dim3(PT_BLOCK), 0, stream, in, paths, bp, out, out_bytes, rec_off);
    SSN_CHECK_LAUNCH("proposal_text_fill");
    return SSN_OK;
}
