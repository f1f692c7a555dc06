// Baseline JPEG encoding of a batch of images that may differ in size: what PIL's Image.save(f, "JPEG", quality=, subsampling=,
// restart_marker_blocks=) writes, byte for byte, for the libjpeg PIL links (integer colour conversion, h2v1 / h2v2 box downsampling,
// the "islow" forward DCT, Annex K tables scaled by libjpeg's quality rule, the standard Huffman tables).  DESIGN.md section 3.11 has
// the reasoning and the worst-case sizes of the buffers.
//
//   ssn_jpeg_enc_blocks    colour conversion + edge expansion + downsampling + forward DCT + quantisation, one thread per 8 x 8 block;
//                          int16 coefficients in zigzag order, one row per block, rows in the scan's MCU order, dummy blocks included
//   ssn_jpeg_enc_count     bits the Huffman codes of every block take (DC difference against the component's previous block)
//   ssn_jpeg_enc_scan      per image: bit offset of every block inside its restart interval, byte offset of every interval
//   ssn_jpeg_enc_pack      every block ORs its codes into the (zeroed) raw scan at its bit offset; the last block of an interval pads
//                          with 1-bits.  Words a block shares with a neighbour are written with atomic OR, so the order blocks run in
//                          does not matter
//   ssn_jpeg_enc_assemble  counts the FF bytes of every image's raw scan, takes the prefix sum of the file lengths and writes the files:
//                          header, scan with 00 after every FF and RSTn between intervals, FFD9
//
// The host (jpeg_encode.py) describes the batch in desc int32 [images][ENC_DESC_INTS] and prepares the header bytes and the tables;
// it reads nothing between the launches.  No kernel trusts desc: every row is checked against the sizes of the buffers it indexes, and
// every write is bounded by its buffer.
#pragma clang fp contract(off)
#include "ssn_common.h"
#include "jpeg_dct.h"      // enc_fdct8, enc_quantise

namespace {

constexpr int ENC_DESC_INTS = 20;
constexpr int ENC_BLOCK_BITS = 1660;      // most bits a block takes: 11 + 11 (DC) + 63 x (16 + 10) (AC)
// desc row
enum { E_W = 0, E_H, E_NCOMP, E_HS, E_VS, E_MCUX, E_MCUY, E_PIX_OFF, E_BLK_OFF, E_NBLOCKS, E_RI, E_INT_OFF, E_NINT, E_RAW_OFF, E_RAW_CAP,
       E_HDR_OFF, E_HDR_LEN, E_OUT_CAP };
// status bits: the file does not fit its capacity; a coefficient the standard tables have no code for; an unusable desc row
enum { ENC_ST_CAPACITY = 1, ENC_ST_RANGE = 2, ENC_ST_DESC = 4 };

__device__ const unsigned char enc_natural_order[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                                        41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                                        30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

struct EncGeom {
    int W, H, ncomp, hs, vs, mcux, mcuy, bpm, luma, seg, nint, int_off;
    long blk_off;
    unsigned nblocks;
    bool ok;
};

// the geometry of a desc row, ok only if it is consistent and inside the block and interval tables
__device__ __forceinline__ EncGeom enc_geom(const int* d, long total_blocks, long total_intervals) {
    EncGeom g;
    g.W = d[E_W], g.H = d[E_H], g.ncomp = d[E_NCOMP], g.hs = d[E_HS], g.vs = d[E_VS], g.mcux = d[E_MCUX], g.mcuy = d[E_MCUY];
    g.blk_off = d[E_BLK_OFF];
    g.nblocks = (unsigned)d[E_NBLOCKS];
    g.int_off = d[E_INT_OFF], g.nint = d[E_NINT];
    const int ri = d[E_RI];
    g.ok = g.W >= 1 && g.H >= 1 && g.W <= 65535 && g.H <= 65535 && (g.ncomp == 1 || g.ncomp == 3) && g.hs >= 1 && g.hs <= 2 && g.vs >= 1 &&
           g.vs <= g.hs && (g.ncomp == 3 || g.hs == 1) && ri >= 1;
    g.luma = g.bpm = g.seg = 1;
    if (!g.ok) return g;
    g.luma = g.hs * g.vs;
    g.bpm = g.ncomp == 1 ? 1 : g.luma + 2;
    const long mcus = (long)g.mcux * g.mcuy, nb = mcus * g.bpm;
    g.ok = g.mcux == (g.W + 8 * g.hs - 1) / (8 * g.hs) && g.mcuy == (g.H + 8 * g.vs - 1) / (8 * g.vs) && nb * ENC_BLOCK_BITS < (1L << 31) &&
           (long)g.nblocks == nb && g.blk_off >= 0 && g.blk_off + nb <= total_blocks && ri <= mcus && g.nint == (mcus + ri - 1) / ri &&
           g.int_off >= 0 && (long)g.int_off + g.nint <= total_intervals;
    if (g.ok) g.seg = ri * g.bpm;
    return g;
}

// component, and block coordinates inside the component, of block j of MCU (mx, my)
__device__ __forceinline__ void enc_block_at(const EncGeom& g, int mx, int my, int j, int& comp, int& bx, int& by) {
    if (j < g.luma) {
        comp = 0;
        bx = mx * g.hs + (j & (g.hs - 1));
        by = my * g.vs + (j >> (g.hs - 1));
    } else {
        comp = j - g.luma + 1;
        bx = mx;
        by = my;
    }
}

__device__ __forceinline__ int enc_component(const unsigned char* p, int ncomp, int comp) {
    if (ncomp == 1) return p[0];
    const int r = p[0], gg = p[1], b = p[2];
    if (comp == 0) return (19595 * r + 38470 * gg + 7471 * b + 32768) >> 16;
    if (comp == 1) return (-11059 * r - 21709 * gg + 32768 * b + (128 << 16) + 32767) >> 16;
    return (32768 * r - 27439 * gg - 5329 * b + (128 << 16) + 32767) >> 16;
}

// sample (x, y) of a component after edge expansion and downsampling.  Columns past the image repeat its last column BEFORE the
// downsampling; rows repeat the last input row up to a multiple of the vertical factor, and past that the last DOWNSAMPLED row.
__device__ __forceinline__ int enc_sample(const unsigned char* pix, const EncGeom& g, int comp, int x, int y) {
    const int W = g.W, H = g.H, nc = g.ncomp;
    if (comp == 0 || g.hs == 1) {
        x = x < W ? x : W - 1;
        y = y < H ? y : H - 1;
        return enc_component(pix + ((long)y * W + x) * nc, nc, comp);
    }
    const int x0 = 2 * x < W ? 2 * x : W - 1, x1 = 2 * x + 1 < W ? 2 * x + 1 : W - 1;
    if (g.vs == 1) {
        y = y < H ? y : H - 1;
        const unsigned char* row = pix + (long)y * W * nc;
        return (enc_component(row + (long)x0 * nc, nc, comp) + enc_component(row + (long)x1 * nc, nc, comp) + (x & 1)) >> 1;
    }
    const int ch = (H + 1) >> 1;
    y = y < ch ? y : ch - 1;
    const int y0 = 2 * y, y1 = 2 * y + 1 < H ? 2 * y + 1 : H - 1;
    const unsigned char* r0 = pix + (long)y0 * W * nc;
    const unsigned char* r1 = pix + (long)y1 * W * nc;
    return (enc_component(r0 + (long)x0 * nc, nc, comp) + enc_component(r0 + (long)x1 * nc, nc, comp) +
            enc_component(r1 + (long)x0 * nc, nc, comp) + enc_component(r1 + (long)x1 * nc, nc, comp) + 1 + (x & 1)) >> 2;
}

// grid (ceil(max blocks of an image / 256), images): thread = one block of one image.  quant: uint16 [2][64], natural order
__global__ __launch_bounds__(256) void jpeg_enc_blocks_kernel(const unsigned char* pix, long pix_bytes, const int* desc,
                                                              const unsigned short* quant, short* coef, long total_blocks) {
    const int* d = desc + (long)blockIdx.y * ENC_DESC_INTS;
    const EncGeom g = enc_geom(d, total_blocks, 1L << 40);
    const unsigned lb = blockIdx.x * 256u + threadIdx.x;
    const long pix_off = d[E_PIX_OFF];
    if (!g.ok || lb >= g.nblocks || pix_off < 0 || pix_off + (long)g.W * g.H * g.ncomp > pix_bytes) return;
    const unsigned char* p = pix + pix_off;
    const int mcu = (int)(lb / (unsigned)g.bpm), j = (int)(lb - (unsigned)mcu * g.bpm);
    const int my = mcu / g.mcux, mx = mcu - my * g.mcux;
    int comp, bx, by;
    enc_block_at(g, mx, my, j, comp, bx, by);
    const unsigned short* qt = quant + (comp ? 64 : 0);
    uint32_t* out = reinterpret_cast<uint32_t*>(coef + (g.blk_off + lb) * 64);
    // real blocks of the component (only luma has blocks past them: an MCU holds one block of each chroma component)
    const int rbw = (g.W + 7) / 8, rbh = (g.H + 7) / 8;
    if (comp == 0 && (bx >= rbw || by >= rbh)) {
        // a dummy block: no AC, the DC of the block in front of it in the MCU -- i.e. of the last REAL block in front of it.  The DC
        // the islow transform gives is the plain sum of the 64 (sample - 128), so it is summed here instead of awaited
        int sj = j - 1, sx = bx, sy = by;
        for (; sj > 0; --sj) {
            int c0;
            enc_block_at(g, mx, my, sj, c0, sx, sy);
            if (sx < rbw && sy < rbh) break;
        }
        int c0;
        enc_block_at(g, mx, my, sj, c0, sx, sy);
        int sum = 0;
        for (int r = 0; r < 8; ++r)
            for (int c = 0; c < 8; ++c) sum += enc_sample(p, g, 0, sx * 8 + c, sy * 8 + r) - 128;
        out[0] = (uint32_t)(unsigned short)(short)enc_quantise(sum, qt[0]);
#pragma unroll
        for (int i = 1; i < 32; ++i) out[i] = 0;
        return;
    }
    int x[64];
#pragma unroll
    for (int r = 0; r < 8; ++r)
#pragma unroll
        for (int c = 0; c < 8; ++c) x[8 * r + c] = enc_sample(p, g, comp, bx * 8 + c, by * 8 + r) - 128;
#pragma unroll
    for (int r = 0; r < 8; ++r) enc_fdct8(x + 8 * r, 1, true);
#pragma unroll
    for (int c = 0; c < 8; ++c) enc_fdct8(x + c, 8, false);
#pragma unroll
    for (int i = 0; i < 32; ++i) {
        const int n0 = enc_natural_order[2 * i], n1 = enc_natural_order[2 * i + 1];
        const int v0 = enc_quantise(x[n0], qt[n0]), v1 = enc_quantise(x[n1], qt[n1]);
        out[i] = (uint32_t)(unsigned short)(short)v0 | ((uint32_t)(unsigned short)(short)v1 << 16);
    }
}

// ---- Huffman coding of one block, shared by the count and the pack stage so that the two cannot disagree.
// tables: uint32 [4][256] (DC luma, AC luma, DC chroma, AC chroma), entry = length << 16 | code, 0: the symbol has no code.
// A value the tables have no code for (an AC coefficient past 10 bits, a DC difference past 11) is coded as zero and reported.
struct EncCountSink {
    int bits;
    __device__ __forceinline__ void put(unsigned, int len) { bits += len; }
};

struct EncPackSink {
    unsigned long long acc;      // the low n bits wait to be written, first bit of the stream in the most significant
    int n, bits;
    long w, w_lo, w_hi;          // next word; the words of the image's raw region
    int* raw32;
    bool first;
    int err;
    __device__ __forceinline__ void word(unsigned v, bool shared) {
        if (w < w_lo || w >= w_hi) {
            err |= ENC_ST_CAPACITY;
        } else if (shared) {
            if (v) atomicOr(raw32 + w, (int)__builtin_bswap32(v));
        } else {
            raw32[w] = (int)__builtin_bswap32(v);
        }
        ++w;
    }
    __device__ __forceinline__ void put(unsigned v, int len) {      // len <= 27, n < 32 on entry
        acc = (acc << len) | v;
        n += len;
        bits += len;
        if (n >= 32) {
            word((unsigned)(acc >> (n - 32)), first);      // (after the first word, a full word holds bits of this block only)
            first = false;
            n -= 32;
            acc &= (1ull << n) - 1ull;
        }
    }
    __device__ __forceinline__ void finish() {
        if (n > 0) word((unsigned)(acc << (32 - n)), true);
        n = 0;
    }
};

template <class Sink>
__device__ __forceinline__ int enc_block_codes(const short* c, int pred, const uint32_t* dc, const uint32_t* ac, Sink& s) {
    int err = 0;
    int diff = (int)c[0] - pred;
    int a = diff < 0 ? -diff : diff;
    int nb = a ? 32 - __builtin_clz((unsigned)a) : 0;
    if (nb > 11) {
        err = ENC_ST_RANGE;
        nb = 0;
        diff = 0;
    }
    uint32_t e = dc[nb];
    if (e == 0) err = ENC_ST_RANGE;
    else s.put(((e & 0xFFFFu) << nb) | ((unsigned)(diff < 0 ? diff - 1 : diff) & ((1u << nb) - 1u)), (int)(e >> 16) + nb);
    int run = 0;
    const uint32_t zrl = ac[0xF0], eob = ac[0];
    for (int k = 1; k < 64; ++k) {
        const int v = c[k];
        a = v < 0 ? -v : v;
        nb = a ? 32 - __builtin_clz((unsigned)a) : 0;
        if (nb > 10) {
            err = ENC_ST_RANGE;
            nb = 0;
        }
        if (nb == 0) {
            ++run;
            continue;
        }
        while (run > 15) {
            s.put(zrl & 0xFFFFu, (int)(zrl >> 16));
            run -= 16;
        }
        e = ac[(run << 4) | nb];
        if (e == 0) err = ENC_ST_RANGE;
        else s.put(((e & 0xFFFFu) << nb) | ((unsigned)(v < 0 ? v - 1 : v) & ((1u << nb) - 1u)), (int)(e >> 16) + nb);
        run = 0;
    }
    if (run > 0) s.put(eob & 0xFFFFu, (int)(eob >> 16));
    return err;
}

// the block's place in its image: the DC prediction (0 at the start of a restart interval), its tables and interval
struct EncBlockCtx {
    int pred, k;
    bool last;              // the last block of its interval
    const uint32_t* dc;
    const uint32_t* ac;
};
__device__ __forceinline__ EncBlockCtx enc_block_ctx(const EncGeom& g, unsigned lb, const short* coef, const uint32_t* tables) {
    EncBlockCtx x;
    const int mcu = (int)(lb / (unsigned)g.bpm), j = (int)(lb - (unsigned)mcu * g.bpm);
    const int comp = j < g.luma ? 0 : j - g.luma + 1;
    x.k = (int)(lb / (unsigned)g.seg);
    const unsigned seg0 = (unsigned)x.k * g.seg;
    x.last = lb + 1 == g.nblocks || lb + 1 == seg0 + g.seg;
    // the component's previous block in scan order: the block in front (luma inside an MCU), else the same place one MCU back
    long prev;
    if (comp == 0 && j > 0) prev = (long)lb - 1;
    else if (comp == 0) prev = (long)lb - g.bpm + g.luma - 1;
    else prev = (long)lb - g.bpm;
    const bool first_mcu = lb - seg0 < (unsigned)g.bpm;
    x.pred = (first_mcu && !(comp == 0 && j > 0)) || prev < 0 ? 0 : coef[(g.blk_off + prev) * 64];
    x.dc = tables + (comp ? 512 : 0);
    x.ac = x.dc + 256;
    return x;
}

// grid (ceil(max blocks / 256), images)
__global__ __launch_bounds__(256) void jpeg_enc_count_kernel(const short* coef, long total_blocks, const int* desc, const uint32_t* tables,
                                                             int* blkbits, int* status) {
    const int* d = desc + (long)blockIdx.y * ENC_DESC_INTS;
    const EncGeom g = enc_geom(d, total_blocks, 1L << 40);
    const unsigned lb = blockIdx.x * 256u + threadIdx.x;
    if (!g.ok) {
        if (lb == 0) atomicOr(status + blockIdx.y, ENC_ST_DESC);
        return;
    }
    if (lb >= g.nblocks) return;
    const EncBlockCtx x = enc_block_ctx(g, lb, coef, tables);
    EncCountSink s{0};
    const int err = enc_block_codes(coef + (g.blk_off + lb) * 64, x.pred, x.dc, x.ac, s);
    blkbits[g.blk_off + lb] = s.bits;
    if (err) atomicOr(status + blockIdx.y, err);
}

// inclusive scan of v over the 256 threads of the block; seg: restart where f is set (f comes back as "a flag at or before me")
__device__ __forceinline__ int enc_scan256(int v, int& f, int* sv, int* sf) {
    const int t = threadIdx.x;
    sv[t] = v;
    sf[t] = f;
    __syncthreads();
    for (int off = 1; off < 256; off <<= 1) {
        int pv = 0, pf = 0;
        if (t >= off) {
            pv = sv[t - off];
            pf = sf[t - off];
        }
        __syncthreads();
        if (t >= off) {
            if (!sf[t]) sv[t] += pv;
            sf[t] |= pf;
        }
        __syncthreads();
    }
    v = sv[t];
    f = sf[t];
    __syncthreads();
    return v;
}

// one workgroup per image.  blkbits: bits of every block -> its bit offset inside its restart interval.  ivals [intervals]: the raw
// bytes of every interval (its bits rounded up to a byte) -> its byte offset inside the image's raw region.  rawlen [images].
__global__ __launch_bounds__(256) void jpeg_enc_scan_kernel(const int* desc, int* blkbits, long total_blocks, int* ivals, long total_intervals,
                                                            int* rawlen, int* status) {
    __shared__ int sv[256], sf[256], s_carry;
    const int image = blockIdx.x, t = threadIdx.x;
    const int* d = desc + (long)image * ENC_DESC_INTS;
    const EncGeom g = enc_geom(d, total_blocks, total_intervals);
    if (!g.ok) {
        if (t == 0) {
            atomicOr(status + image, ENC_ST_DESC);
            rawlen[image] = 0;
        }
        return;
    }
    int carry = 0;
    for (unsigned base = 0; base < g.nblocks; base += 256) {
        const unsigned lb = base + t;
        const bool live = lb < g.nblocks;
        const int v = live ? blkbits[g.blk_off + lb] : 0;
        const unsigned k = live ? lb / (unsigned)g.seg : 0;
        int f = live && lb == k * g.seg;
        int incl = enc_scan256(v, f, sv, sf);
        if (!f) incl += carry;
        if (live) {
            blkbits[g.blk_off + lb] = incl - v;
            if (lb + 1 == g.nblocks || lb + 1 == (k + 1) * g.seg) ivals[g.int_off + k] = (incl + 7) >> 3;
        }
        if (t == 255) s_carry = incl;
        __syncthreads();
        carry = s_carry;
    }
    __syncthreads();      // (the interval lengths other threads of this workgroup wrote are read below)
    long run = 0;
    for (int base = 0; base < g.nint; base += 256) {
        const int k = base + t;
        const int v = k < g.nint ? ivals[g.int_off + k] : 0;
        int f = 0;
        const int incl = enc_scan256(v, f, sv, sf);
        if (k < g.nint) ivals[g.int_off + k] = (int)(run + incl - v);
        if (t == 255) s_carry = incl;
        __syncthreads();
        run += s_carry;
        __syncthreads();
    }
    if (t == 0) {
        const int cap = d[E_RAW_CAP];
        if (run > cap || cap < 0) {
            atomicOr(status + image, ENC_ST_CAPACITY);
            run = 0;
        }
        rawlen[image] = (int)run;
    }
}

// the image's raw region [off, off + cap): whole words inside the raw buffer
__device__ __forceinline__ bool enc_raw_region(const int* d, long raw_bytes, long& off, long& cap) {
    off = d[E_RAW_OFF];
    cap = d[E_RAW_CAP];
    return off >= 0 && cap >= 0 && (off & 3) == 0 && (cap & 3) == 0 && off + cap <= raw_bytes;
}

// grid (ceil(max blocks / 256), images)
__global__ __launch_bounds__(256) void jpeg_enc_pack_kernel(const short* coef, long total_blocks, const int* desc, const uint32_t* tables,
                                                            const int* blkbits, const int* ivals, long total_intervals, const int* rawlen,
                                                            unsigned char* raw, long raw_bytes, int* status) {
    const int image = blockIdx.y;
    const int* d = desc + (long)image * ENC_DESC_INTS;
    const EncGeom g = enc_geom(d, total_blocks, total_intervals);
    const unsigned lb = blockIdx.x * 256u + threadIdx.x;
    long raw_off, raw_cap;
    if (!g.ok || lb >= g.nblocks || rawlen[image] <= 0) return;      // (an image that does not fit has length 0)
    if (!enc_raw_region(d, raw_bytes, raw_off, raw_cap)) {
        if (lb == 0) atomicOr(status + image, ENC_ST_DESC);
        return;
    }
    const EncBlockCtx x = enc_block_ctx(g, lb, coef, tables);
    const int bit0 = blkbits[g.blk_off + lb];
    const long p = (raw_off + ivals[g.int_off + x.k]) * 8 + bit0;
    EncPackSink s;
    s.acc = 0;
    s.n = (int)(p & 31);
    s.bits = 0;
    s.w = p >> 5;
    s.w_lo = raw_off >> 2;
    s.w_hi = (raw_off + raw_cap) >> 2;
    s.raw32 = reinterpret_cast<int*>(raw);
    s.first = true;
    s.err = 0;
    if (bit0 < 0 || ivals[g.int_off + x.k] < 0) s.w = -1;
    enc_block_codes(coef + (g.blk_off + lb) * 64, x.pred, x.dc, x.ac, s);
    if (x.last) {
        const int pad = (8 - ((bit0 + s.bits) & 7)) & 7;
        if (pad) s.put((1u << pad) - 1u, pad);
    }
    s.finish();
    if (s.err) atomicOr(status + image, s.err);
}

__device__ __forceinline__ int enc_count_ff(uint32_t w) {
    return ((w & 0xFFu) == 0xFFu) + ((w & 0xFF00u) == 0xFF00u) + ((w & 0xFF0000u) == 0xFF0000u) + ((w >> 24) == 0xFFu);
}

// one workgroup per image: the FF bytes of its raw scan
__global__ __launch_bounds__(256) void jpeg_enc_ffcount_kernel(const unsigned char* raw, long raw_bytes, const int* desc, const int* rawlen,
                                                               int* ffcount) {
    __shared__ int sv[256], sf[256];
    const int image = blockIdx.x, t = threadIdx.x;
    const int* d = desc + (long)image * ENC_DESC_INTS;
    long raw_off, raw_cap;
    int n = rawlen[image];
    if (!enc_raw_region(d, raw_bytes, raw_off, raw_cap) || n > raw_cap) n = 0;
    const uint32_t* src = reinterpret_cast<const uint32_t*>(raw + raw_off);
    int count = 0;
    for (long r = (long)t * 16; r < n; r += 4096)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const long b = r + 4 * i;
            if (b >= n) break;
            uint32_t w = src[b >> 2];
            if (n - b < 4) w &= (1u << (8 * (n - b))) - 1u;      // (bytes past the scan's end do not count)
            count += enc_count_ff(w);
        }
    int f = 0;
    const int incl = enc_scan256(count, f, sv, sf);
    if (t == 255) ffcount[image] = incl;
}

__device__ __forceinline__ bool enc_header_ok(const int* d, long header_bytes) {
    return d[E_HDR_OFF] >= 0 && d[E_HDR_LEN] >= 1 && (long)d[E_HDR_OFF] + d[E_HDR_LEN] <= header_bytes;
}

// ONE workgroup: lengths of the files and the prefix sum that places them.  A file that does not fit its capacity gets length 0.
__global__ __launch_bounds__(256) void jpeg_enc_offsets_kernel(const int* desc, int n_images, const int* rawlen, const int* ffcount,
                                                               long header_bytes, long data_bytes, long* offsets, int* lengths, int* status) {
    __shared__ int sv[256];
    __shared__ long s_carry;
    const int t = threadIdx.x;
    long run = 0;
    for (int base = 0; base < n_images; base += 256) {
        const int i = base + t;
        int len = 0;
        if (i < n_images) {
            const int* d = desc + (long)i * ENC_DESC_INTS;
            const int rl = rawlen[i], nint = d[E_NINT], cap = d[E_OUT_CAP];
            if (rl > 0 && nint >= 1 && enc_header_ok(d, header_bytes) && !(status[i] & (ENC_ST_CAPACITY | ENC_ST_DESC))) {
                const long want = (long)d[E_HDR_LEN] + rl + ffcount[i] + 2L * (nint - 1) + 2;
                if (want <= cap && want < (1L << 30)) len = (int)want;
                else atomicOr(status + i, ENC_ST_CAPACITY);
            } else if (!(status[i] & ENC_ST_CAPACITY)) {
                atomicOr(status + i, ENC_ST_DESC);
            }
        }
        // the lengths of a chunk go through shared memory; thread 0 walks them in 64 bits (files, not bytes: 256 steps a chunk)
        sv[t] = len;
        __syncthreads();
        if (t == 0) {
            long o = run;
            for (int q = 0; q < 256; ++q) {
                const long l = sv[q];
                if (base + q < n_images) {
                    if (o + l > data_bytes) {      // (cannot happen when data holds the sum of the capacities)
                        atomicOr(status + base + q, ENC_ST_CAPACITY);
                        lengths[base + q] = 0;
                        offsets[base + q] = o;
                    } else {
                        lengths[base + q] = (int)l;
                        offsets[base + q] = o;
                        o += l;
                    }
                }
            }
            s_carry = o;
        }
        __syncthreads();
        run = s_carry;
        __syncthreads();
    }
}

// one workgroup per image: header, the raw scan with 00 after every FF and RSTn in front of every interval but the first, FFD9
__global__ __launch_bounds__(256) void jpeg_enc_files_kernel(const unsigned char* raw, long raw_bytes, const int* desc, const int* ivals,
                                                             long total_intervals, const int* rawlen, const unsigned char* headers,
                                                             long header_bytes, unsigned char* data, long data_bytes, const long* offsets,
                                                             const int* lengths) {
    __shared__ int sv[256], sf[256], s_carry;
    const int image = blockIdx.x, t = threadIdx.x;
    const int* d = desc + (long)image * ENC_DESC_INTS;
    const int len = lengths[image], n = rawlen[image], nint = d[E_NINT], int_off = d[E_INT_OFF], hdr_len = d[E_HDR_LEN];
    const long off = offsets[image];
    long raw_off, raw_cap;
    if (len <= 0 || n <= 0 || off < 0 || off + len > data_bytes || !enc_header_ok(d, header_bytes) || nint < 1 || int_off < 0 ||
        (long)int_off + nint > total_intervals || !enc_raw_region(d, raw_bytes, raw_off, raw_cap) || n > raw_cap)
        return;
    unsigned char* out = data + off;
    const long body_end = (long)len - 2;      // every scan byte lands in [hdr_len, body_end)
    for (int i = t; i < hdr_len && i < len; i += 256) out[i] = headers[d[E_HDR_OFF] + i];
    const uint32_t* src = reinterpret_cast<const uint32_t*>(raw + raw_off);
    const int* iv = ivals + int_off;
    long extras = 0;      // stuffed zeros and marker bytes in front of this chunk
    for (long base = 0; base < n; base += 4096) {
        const long r0 = base + (long)t * 16;
        const long r1 = r0 + 16 < n ? r0 + 16 : n;
        uint32_t w[4] = {0, 0, 0, 0};
        int next_k = nint, extra = 0;
        if (r0 < n) {
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (r0 + 4 * i < n) w[i] = src[(r0 >> 2) + i];
            // the first interval that starts at or after r0
            int lo = 0, hi = nint;
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (iv[mid] < r0) lo = mid + 1;
                else hi = mid;
            }
            next_k = lo;
            int k = next_k;
            for (long r = r0; r < r1; ++r) {
                while (k < nint && iv[k] == r) {
                    if (k > 0) extra += 2;
                    ++k;
                }
                extra += ((w[(r - r0) >> 2] >> (8 * ((r - r0) & 3))) & 0xFFu) == 0xFFu;
            }
        }
        int f = 0;
        const int incl = enc_scan256(extra, f, sv, sf);
        if (r0 < n) {
            long pos = hdr_len + r0 + extras + (incl - extra);
            int k = next_k;
            for (long r = r0; r < r1; ++r) {
                while (k < nint && iv[k] == r) {
                    if (k > 0 && pos + 2 <= body_end) {
                        out[pos] = 0xFF;
                        out[pos + 1] = (unsigned char)(0xD0 + ((k - 1) & 7));
                        pos += 2;
                    }
                    ++k;
                }
                const unsigned b = (w[(r - r0) >> 2] >> (8 * ((r - r0) & 3))) & 0xFFu;
                if (pos < body_end) out[pos] = (unsigned char)b;
                ++pos;
                if (b == 0xFFu) {
                    if (pos < body_end) out[pos] = 0;
                    ++pos;
                }
            }
        }
        if (t == 255) s_carry = incl;
        __syncthreads();
        extras += s_carry;
        __syncthreads();
    }
    if (t == 0) {
        out[len - 2] = 0xFF;
        out[len - 1] = 0xD9;
    }
}

}  // namespace

// the sizes the host builds its tables and buffers with: ints of a desc row, the most bits one block takes
extern "C" int ssn_jpeg_enc_layout(int* desc_ints, int* block_bits) {
    if (desc_ints) *desc_ints = ENC_DESC_INTS;
    if (block_bits) *block_bits = ENC_BLOCK_BITS;
    return SSN_OK;
}

#define ENC_CHECK_COUNTS(name)                                                                                            \
    SSN_CHECK_ARG(n_images >= 1 && n_images <= 65535 && max_blocks >= 1 && total_blocks >= 1 && total_blocks < (1L << 25), \
                  name ": bad counts")

extern "C" int ssn_jpeg_enc_blocks(const unsigned char* pix, long pix_bytes, const int* desc, int n_images, int max_blocks,
                                   const unsigned short* quant, short* coef, long total_blocks, hipStream_t stream) {
    ENC_CHECK_COUNTS("jpeg_enc_blocks");
    SSN_CHECK_ARG(pix_bytes >= 1 && pix_bytes < (1L << 31), "jpeg_enc_blocks: bad buffer sizes");
    SSN_CHECK_ARG(pix && desc && quant && coef, "jpeg_enc_blocks: null pointer");
    SSN_CHECK_ARG(((uintptr_t)coef & 3) == 0, "jpeg_enc_blocks: the coefficient buffer must be 4-byte aligned");
    hipLaunchKernelGGL(jpeg_enc_blocks_kernel, dim3((unsigned)((max_blocks + 255) / 256), (unsigned)n_images), dim3(256), 0, stream, pix,
                       pix_bytes, desc, quant, coef, total_blocks);
    SSN_CHECK_LAUNCH("jpeg_enc_blocks");
    return SSN_OK;
}

// zero-fills status [n_images], then writes blkbits [total_blocks]
extern "C" int ssn_jpeg_enc_count(const short* coef, long total_blocks, const int* desc, int n_images, int max_blocks,
                                  const unsigned int* tables, int* blkbits, int* status, hipStream_t stream) {
    ENC_CHECK_COUNTS("jpeg_enc_count");
    SSN_CHECK_ARG(coef && desc && tables && blkbits && status, "jpeg_enc_count: null pointer");
    if (hipMemsetAsync(status, 0, (size_t)n_images * sizeof(int), stream) != hipSuccess) {
        ssn_set_error("jpeg_enc_count: memset failed");
        return SSN_ERR_LAUNCH;
    }
    hipLaunchKernelGGL(jpeg_enc_count_kernel, dim3((unsigned)((max_blocks + 255) / 256), (unsigned)n_images), dim3(256), 0, stream, coef,
                       total_blocks, desc, tables, blkbits, status);
    SSN_CHECK_LAUNCH("jpeg_enc_count");
    return SSN_OK;
}

extern "C" int ssn_jpeg_enc_scan(const int* desc, int n_images, int* blkbits, long total_blocks, int* ivals, long total_intervals,
                                 int* rawlen, int* status, hipStream_t stream) {
    SSN_CHECK_ARG(n_images >= 1 && n_images <= 65535 && total_blocks >= 1 && total_blocks < (1L << 25) && total_intervals >= 1 &&
                      total_intervals <= total_blocks,
                  "jpeg_enc_scan: bad counts");
    SSN_CHECK_ARG(desc && blkbits && ivals && rawlen && status, "jpeg_enc_scan: null pointer");
    hipLaunchKernelGGL(jpeg_enc_scan_kernel, dim3((unsigned)n_images), dim3(256), 0, stream, desc, blkbits, total_blocks, ivals,
                       total_intervals, rawlen, status);
    SSN_CHECK_LAUNCH("jpeg_enc_scan");
    return SSN_OK;
}

// zero-fills raw [raw_bytes], then packs
extern "C" int ssn_jpeg_enc_pack(const short* coef, long total_blocks, const int* desc, int n_images, int max_blocks,
                                 const unsigned int* tables, const int* blkbits, const int* ivals, long total_intervals, const int* rawlen,
                                 unsigned char* raw, long raw_bytes, int* status, hipStream_t stream) {
    ENC_CHECK_COUNTS("jpeg_enc_pack");
    SSN_CHECK_ARG(total_intervals >= 1 && raw_bytes >= 4 && raw_bytes < (1L << 31) && (raw_bytes & 3) == 0, "jpeg_enc_pack: bad buffer sizes");
    SSN_CHECK_ARG(coef && desc && tables && blkbits && ivals && rawlen && raw && status, "jpeg_enc_pack: null pointer");
    SSN_CHECK_ARG(((uintptr_t)raw & 3) == 0, "jpeg_enc_pack: the raw buffer must be 4-byte aligned");
    if (hipMemsetAsync(raw, 0, (size_t)raw_bytes, stream) != hipSuccess) {
        ssn_set_error("jpeg_enc_pack: memset failed");
        return SSN_ERR_LAUNCH;
    }
    hipLaunchKernelGGL(jpeg_enc_pack_kernel, dim3((unsigned)((max_blocks + 255) / 256), (unsigned)n_images), dim3(256), 0, stream, coef,
                       total_blocks, desc, tables, blkbits, ivals, total_intervals, rawlen, raw, raw_bytes, status);
    SSN_CHECK_LAUNCH("jpeg_enc_pack");
    return SSN_OK;
}

// three launches: FF count per image, lengths + offsets, the files.  ffcount [n_images] is scratch.
extern "C" int ssn_jpeg_enc_assemble(const unsigned char* raw, long raw_bytes, const int* desc, int n_images, const int* ivals,
                                     long total_intervals, const int* rawlen, const unsigned char* headers, long header_bytes, int* ffcount,
                                     unsigned char* data, long data_bytes, long* offsets, int* lengths, int* status, hipStream_t stream) {
    SSN_CHECK_ARG(n_images >= 1 && n_images <= 65535 && total_intervals >= 1, "jpeg_enc_assemble: bad counts");
    SSN_CHECK_ARG(raw_bytes >= 4 && raw_bytes < (1L << 31) && (raw_bytes & 3) == 0 && header_bytes >= 1 && data_bytes >= 1,
                  "jpeg_enc_assemble: bad buffer sizes");
    SSN_CHECK_ARG(raw && desc && ivals && rawlen && headers && ffcount && data && offsets && lengths && status,
                  "jpeg_enc_assemble: null pointer");
    SSN_CHECK_ARG(((uintptr_t)raw & 3) == 0, "jpeg_enc_assemble: the raw buffer must be 4-byte aligned");
    hipLaunchKernelGGL(jpeg_enc_ffcount_kernel, dim3((unsigned)n_images), dim3(256), 0, stream, raw, raw_bytes, desc, rawlen, ffcount);
    hipLaunchKernelGGL(jpeg_enc_offsets_kernel, dim3(1), dim3(256), 0, stream, desc, n_images, rawlen, ffcount, header_bytes, data_bytes,
                       offsets, lengths, status);
    hipLaunchKernelGGL(jpeg_enc_files_kernel, dim3((unsigned)n_images), dim3(256), 0, stream, raw, raw_bytes, desc, ivals, total_intervals,
                       rawlen, headers, header_bytes, data, data_bytes, offsets, lengths);
    SSN_CHECK_LAUNCH("jpeg_enc_assemble");
    return SSN_OK;
}
