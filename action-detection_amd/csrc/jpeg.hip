// Baseline JPEG decoding for the input pipeline: what PIL's Image.open(...).convert(mode) does in the loader workers of the
// reference (ssn_dataset.py:208-215), as three launches over a BATCH of files that may differ in size, sampling and tables.
// DESIGN.md section 3.10 has the reasoning; the arithmetic is libjpeg's (islow inverse DCT, fancy upsampling, 16-bit colour
// conversion), bit for bit.
//
//   ssn_jpeg_entropy   Huffman decode, one LANE per restart interval (or per scan of a file without restart markers)
//   ssn_jpeg_idct      dequantise + inverse DCT, one thread per 8 x 8 block, into padded component planes
//   ssn_jpeg_pixels    upsample + colour conversion + crop, one thread per output pixel
//   ssn_jpeg_index     optional, in front of the entropy stage: the restart intervals of every file, one workgroup per file
//
// The host (jpeg_decode.py) walks the markers and writes three device tables:
//   desc   int32 [images][JPEG_DESC_INTS]   geometry and the image's offsets into the coefficient, plane and output buffers
//   units  int32 [units][JPEG_UNIT_INTS]    one row per sequential unit, padded to whole workgroups of 64
//   tables uint32 [sets][4][JPEG_TABLE_WORDS]   the distinct Huffman table sets of the batch (DC0, AC0, DC1, AC1)
// Nothing a file says is trusted past the parser: every bitstream read is bounded by the unit's byte range (bytes past its end
// read as zero), every coefficient write by the image's block count AND the buffer's, every plane / pixel write by the buffer.
#include "ssn_common.h"
#include "jpeg_dct.h"      // jpeg_idct8

namespace {

constexpr int JPEG_DESC_INTS = 24;
constexpr int JPEG_UNIT_INTS = 8;
constexpr int JPEG_TABLE_WORDS = 384;      // per table: 256 words of first-level entries, 17 maxcode, 17 valoff, 64 words of symbols
constexpr int JPEG_SET_WORDS = 4 * JPEG_TABLE_WORDS;
constexpr int JPEG_LDS_SETS = 8;           // table sets one workgroup may hold (48 KiB)
constexpr int JPEG_LUT_BITS = 9;

// desc row
enum { D_W = 0, D_H, D_NCOMP, D_HS, D_VS, D_MCUX, D_MCUY, D_COEF_OFF, D_NBLOCKS, D_PLANE_OFF, D_OUT_OFF, D_Q0, D_Q1, D_Q2, D_TSEL };
// unit row: image (-1: padding), first byte, end byte, first MCU, MCU count, table set; in a workgroup's FIRST row additionally the
// first table set the workgroup stages and how many
enum { U_IMAGE = 0, U_BEGIN, U_END, U_MCU0, U_NMCU, U_SET, U_WG_SET0, U_WG_NSETS };

enum { JPEG_ST_DATA = 1, JPEG_ST_CODE = 2, JPEG_ST_BLOCK = 4, JPEG_ST_TABLE = 8 };

__device__ const unsigned char jpeg_natural_order[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                                         41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                                         30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

// Entropy stage.  64 lanes, one unit each.  A trip of the loop decodes ONE symbol -- refill, table lookup, place -- whatever image,
// component or coefficient the lane is at, so lanes that own different files run the same instructions; end of block, end of MCU
// and end of unit are selects on the lane's state, not branches around different code.
__global__ __launch_bounds__(64) void jpeg_entropy_kernel(const unsigned char* bits, long bits_bytes, const int* desc, int n_images,
                                                         const int* units, const uint32_t* tables, int n_sets, short* coef,
                                                         long total_blocks, int* status) {
    __shared__ uint32_t s_tab[JPEG_LDS_SETS * JPEG_SET_WORDS];
    const int lane = threadIdx.x;
    const int* wg_row = units + (long)blockIdx.x * 64 * JPEG_UNIT_INTS;
    int set0 = wg_row[U_WG_SET0], nsets = wg_row[U_WG_NSETS];
    if (set0 < 0 || set0 >= n_sets) nsets = 0;
    if (nsets > JPEG_LDS_SETS) nsets = JPEG_LDS_SETS;
    if (nsets > n_sets - set0) nsets = n_sets - set0;
    if (nsets < 0) nsets = 0;
    for (int i = lane; i < nsets * JPEG_SET_WORDS; i += 64) s_tab[i] = tables[(long)set0 * JPEG_SET_WORDS + i];
    __syncthreads();

    const int* u = wg_row + lane * JPEG_UNIT_INTS;
    const int image = u[U_IMAGE];
    if (image < 0 || image >= n_images) return;      // padding row
    const int* d = desc + (long)image * JPEG_DESC_INTS;
    int err = 0;
    const int set = u[U_SET] - set0;
    if (set < 0 || set >= nsets) err = JPEG_ST_TABLE;
    const uint32_t* tset = s_tab + (err ? 0 : set) * JPEG_SET_WORDS;

    long pos = u[U_BEGIN], end = u[U_END];
    if (end > bits_bytes) end = bits_bytes;
    if (pos < 0) pos = 0;
    if (pos > end) pos = end;
    const int ncomp = d[D_NCOMP], hs = d[D_HS], vs = d[D_VS], mcux = d[D_MCUX], mcuy = d[D_MCUY];
    const int tsel = d[D_TSEL];                      // bit 2 c: component c takes DC table 1, bit 2 c + 1: AC table 1
    const long coef_off = d[D_COEF_OFF];
    const unsigned nblocks = (unsigned)d[D_NBLOCKS];
    if (ncomp != 1 && ncomp != 3) err |= JPEG_ST_TABLE;
    if (hs < 1 || hs > 2 || vs < 1 || vs > 2 || mcux < 1 || mcuy < 1) err |= JPEG_ST_TABLE;
    const int luma_blocks = hs * vs;
    const int mcu_blocks = ncomp == 1 ? 1 : luma_blocks + 2;
    const unsigned luma_total = (unsigned)mcux * hs * (unsigned)mcuy * vs, chroma_total = (unsigned)mcux * mcuy;
    int mcu = u[U_MCU0];
    long mcu_end = (long)mcu + u[U_NMCU];
    if (mcu_end > (long)mcux * mcuy) mcu_end = (long)mcux * mcuy;
    if (mcu < 0) err |= JPEG_ST_TABLE;
    int my = err ? 0 : mcu / mcux, mx = err ? 0 : mcu - my * mcux;

    unsigned long long acc = 0;       // the low `nbits` bits are the stream's next bits, most significant first
    int nbits = 0, pad = 0;           // pad: zero bits appended after the unit's last byte (or in front of a marker)
    int j = 0, k = 0;                 // block of the MCU, coefficient of the block (0: the DC symbol is next)
    int pred0 = 0, pred1 = 0, pred2 = 0;
    bool active = !err && mcu < mcu_end;

    while (active) {
        // ---- refill: four bytes whenever 32 bits or fewer are left, so that a code (<= 16) and its extra bits (<= 15) are there
        if (nbits <= 32) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                unsigned b = 0;
                if (pos < end) {
                    b = bits[pos];
                    if (b == 0xFFu) {
                        const unsigned nx = pos + 1 < end ? bits[pos + 1] : 0xD9u;
                        if (nx == 0u) {
                            pos += 2;                  // FF 00: a stuffed FF
                        } else {
                            b = 0;                     // a marker inside the unit: the data ends here
                            end = pos;
                            pad += 8;
                        }
                    } else {
                        pos += 1;
                    }
                } else {
                    pad += 8;
                }
                acc = (acc << 8) | b;
                nbits += 8;
            }
        }
        // ---- lookup
        const int comp = ncomp == 1 ? 0 : (j < luma_blocks ? 0 : j - luma_blocks + 1);
        const int ac = k != 0;
        const uint32_t* tab = tset + (((tsel >> (2 * comp + ac)) & 1) * 2 + ac) * JPEG_TABLE_WORDS;
        const unsigned code16 = (unsigned)(acc >> (nbits - 16)) & 0xFFFFu;
        const unsigned e = reinterpret_cast<const unsigned short*>(tab)[code16 >> (16 - JPEG_LUT_BITS)];
        int len = (int)(e >> 8), sym = (int)(e & 0xFFu);
        if (len == 0) {                                // overflow path: codes of 10 .. 16 bits, by the canonical maxcode walk
            const int* maxcode = reinterpret_cast<const int*>(tab) + 256;
            const int* valoff = maxcode + 17;
            len = 17;
#pragma unroll
            for (int l = 16; l > JPEG_LUT_BITS; --l)
                if ((int)(code16 >> (16 - l)) <= maxcode[l]) len = l;
            if (len <= 16) {
                const int idx = valoff[len] + (int)(code16 >> (16 - len));
                sym = reinterpret_cast<const unsigned char*>(tab + 290)[idx & 255];
            }
        }
        if (len > 16) {
            err = JPEG_ST_CODE;
            break;
        }
        nbits -= len;
        // ---- place
        const int size = sym & 15, run = k == 0 ? 0 : sym >> 4;
        const int nread = k == 0 ? sym : size;         // (a DC symbol IS its size)
        if (nread > 15) {
            err = JPEG_ST_CODE;
            break;
        }
        int v = nread ? (int)((acc >> (nbits - nread)) & ((1u << nread) - 1u)) : 0;
        nbits -= nread;
        if (nread && v < (1 << (nread - 1))) v += 1 - (1 << nread);       // EXTEND
        if (nbits < pad) {                             // consumed bits the file does not have
            err = JPEG_ST_DATA;
            break;
        }
        const int hh = j & (hs - 1), vv = j >> (hs - 1);
        unsigned lb;                                   // the block's index inside its image
        if (comp == 0)
            lb = (unsigned)(my * vs + vv) * (unsigned)(mcux * hs) + (unsigned)(mx * hs + hh);
        else
            lb = luma_total + (unsigned)(comp - 1) * chroma_total + (unsigned)my * mcux + mx;
        const bool eob = k != 0 && size == 0 && run != 15;
        int kk = k + run;                              // ZRL: run 15, size 0 -> skips 16 with the increment below
        if (k == 0) {
            const int p = (comp == 0 ? pred0 : comp == 1 ? pred1 : pred2) + v;
            if (comp == 0) pred0 = p; else if (comp == 1) pred1 = p; else pred2 = p;
            v = p;
        }
        if (!eob && (k == 0 || size != 0)) {
            if (kk > 63 || lb >= nblocks || coef_off + lb >= total_blocks || coef_off < 0) {
                err = JPEG_ST_BLOCK;
                break;
            }
            coef[(coef_off + lb) * 64 + jpeg_natural_order[kk]] = (short)v;
        }
        k = eob ? 64 : kk + 1;
        if (k > 64) {                                  // a run past the end of the block
            err = JPEG_ST_BLOCK;
            break;
        }
        if (k == 64) {
            k = 0;
            if (++j == mcu_blocks) {
                j = 0;
                ++mcu;
                if (++mx == mcux) {
                    mx = 0;
                    ++my;
                }
                active = mcu < mcu_end;
            }
        }
    }
    if (err) atomicOr(status + image, err);
}

// bytes of an image's component planes (padded to whole MCUs), luma first
__device__ __forceinline__ long jpeg_plane_offset(int comp, int mcux, int mcuy, int hs, int vs) {
    const long luma = (long)mcux * hs * 8 * ((long)mcuy * vs * 8), chroma = (long)mcux * 8 * ((long)mcuy * 8);
    return comp == 0 ? 0 : luma + (comp - 1) * chroma;
}

// grid (ceil(max blocks of an image / 256), images): thread = one block of one image
__global__ __launch_bounds__(256) void jpeg_idct_kernel(const short* coef, long total_blocks, const int* desc, const unsigned short* quant,
                                                        int n_quant, unsigned char* planes, long plane_bytes) {
    const int* d = desc + (long)blockIdx.y * JPEG_DESC_INTS;
    const unsigned lb = blockIdx.x * 256u + threadIdx.x;
    const long coef_off = d[D_COEF_OFF];
    if (lb >= (unsigned)d[D_NBLOCKS] || coef_off < 0 || coef_off + lb >= total_blocks) return;
    const int ncomp = d[D_NCOMP], hs = d[D_HS], vs = d[D_VS], mcux = d[D_MCUX], mcuy = d[D_MCUY];
    if (hs < 1 || hs > 2 || vs < 1 || vs > 2 || mcux < 1 || mcuy < 1) return;
    const unsigned luma_total = (unsigned)mcux * hs * (unsigned)mcuy * vs, chroma_total = (unsigned)mcux * mcuy;
    int comp = 0;
    unsigned in_comp = lb;
    if (lb >= luma_total) {
        comp = 1 + (int)((lb - luma_total) / chroma_total);
        in_comp = (lb - luma_total) - (unsigned)(comp - 1) * chroma_total;
    }
    if (comp >= ncomp || comp > 2) return;
    const int bw = comp == 0 ? mcux * hs : mcux, bh = comp == 0 ? mcuy * vs : mcuy;
    const int by = (int)(in_comp / (unsigned)bw), bx = (int)(in_comp - (unsigned)by * bw);
    const int q = d[D_Q0 + comp];
    if (q < 0 || q >= n_quant) return;
    const unsigned short* qt = quant + q * 64;
    const short* c = coef + (coef_off + lb) * 64;
    int x[64];
#pragma unroll
    for (int i = 0; i < 64; ++i) x[i] = (int)c[i] * (int)qt[i];
#pragma unroll
    for (int col = 0; col < 8; ++col) jpeg_idct8(x + col, 8, 11);
#pragma unroll
    for (int row = 0; row < 8; ++row) jpeg_idct8(x + 8 * row, 1, 18);
    const long base = (long)d[D_PLANE_OFF] + jpeg_plane_offset(comp, mcux, mcuy, hs, vs) + ((long)by * 8 * bw + bx) * 8;
    const long pitch = (long)bw * 8;
    if (d[D_PLANE_OFF] < 0 || (d[D_PLANE_OFF] & 7) || base + 7 * pitch + 8 > plane_bytes || by >= bh) return;
#pragma unroll
    for (int row = 0; row < 8; ++row) {
        uint32_t w[2];
#pragma unroll
        for (int hcol = 0; hcol < 2; ++hcol) {
            uint32_t pk = 0;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                int v = x[8 * row + 4 * hcol + i] + 128;
                v = v < 0 ? 0 : (v > 255 ? 255 : v);
                pk |= (uint32_t)v << (8 * i);
            }
            w[hcol] = pk;
        }
        // (plane offsets are multiples of 8: every plane is a whole number of 8 x 8 blocks and the host aligns the first)
        *reinterpret_cast<uint2*>(planes + base + row * pitch) = uint2{w[0], w[1]};
    }
}

__device__ __forceinline__ int jpeg_clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// libjpeg's fancy upsampling of one chroma sample at luma position (x, y): the triangle filter from the plane's TRUE extent
// cw x ch (neighbours clamped there, which reproduces its edge formulas), plain replication when the plane has two columns or fewer
__device__ __forceinline__ int jpeg_chroma_at(const unsigned char* p, long pitch, int cw, int ch, int hs, int vs, int x, int y) {
    if (hs == 1) return p[(long)y * pitch + x];       // (4:4:4; 1 x 2 sampling is not accepted)
    const int cx = x >> 1;
    if (cw <= 2) return p[(long)(vs == 2 ? y >> 1 : y) * pitch + cx];
    const int nx = jpeg_clampi((x & 1) ? cx + 1 : cx - 1, 0, cw - 1);
    if (vs == 1) {
        const unsigned char* r = p + (long)y * pitch;
        return (3 * r[cx] + r[nx] + ((x & 1) ? 2 : 1)) >> 2;
    }
    const int cy = y >> 1;
    const int ny = jpeg_clampi((y & 1) ? cy + 1 : cy - 1, 0, ch - 1);
    const unsigned char* r0 = p + (long)cy * pitch;
    const unsigned char* r1 = p + (long)ny * pitch;
    const int here = 3 * r0[cx] + r1[cx], there = 3 * r0[nx] + r1[nx];
    return (3 * here + there + ((x & 1) ? 7 : 8)) >> 4;
}

// grid (ceil(max pixels of an image / 256), images); out_c = 3: .convert("RGB"), 1: .convert("L")
__global__ __launch_bounds__(256) void jpeg_pixels_kernel(const unsigned char* planes, long plane_bytes, const int* desc, int out_c,
                                                          unsigned char* out, long out_bytes) {
    const int* d = desc + (long)blockIdx.y * JPEG_DESC_INTS;
    const int W = d[D_W], H = d[D_H], ncomp = d[D_NCOMP], hs = d[D_HS], vs = d[D_VS], mcux = d[D_MCUX], mcuy = d[D_MCUY];
    if (W < 1 || H < 1 || hs < 1 || hs > 2 || vs < 1 || vs > hs || mcux < 1 || mcuy < 1) return;
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long)W * H) return;
    const int y = (int)(i / W), x = (int)(i - (long)y * W);
    const long lw = (long)mcux * hs * 8, lh = (long)mcuy * vs * 8, cwp = (long)mcux * 8, chp = (long)mcuy * 8;
    const long plane_off = d[D_PLANE_OFF], out_off = d[D_OUT_OFF];
    const long need = ncomp == 1 ? lw * lh : lw * lh + 2 * cwp * chp;
    if (plane_off < 0 || plane_off + need > plane_bytes || x >= lw || y >= lh) return;
    if (out_off < 0 || out_off + (long)W * H * out_c > out_bytes) return;
    const unsigned char* py = planes + plane_off;
    const int Y = py[(long)y * lw + x];
    unsigned char* o = out + out_off + i * out_c;
    if (ncomp == 1) {
        o[0] = (unsigned char)Y;
        if (out_c == 3) o[1] = o[2] = (unsigned char)Y;
        return;
    }
    const int cw = (W + hs - 1) / hs, ch = (H + vs - 1) / vs;
    const int cb = jpeg_chroma_at(py + lw * lh, cwp, cw, ch, hs, vs, x, y) - 128;
    const int cr = jpeg_chroma_at(py + lw * lh + cwp * chp, cwp, cw, ch, hs, vs, x, y) - 128;
    const int r = jpeg_clampi(Y + ((91881 * cr + 32768) >> 16), 0, 255);
    const int g = jpeg_clampi(Y + ((-22554 * cb - 46802 * cr + 32768) >> 16), 0, 255);
    const int b = jpeg_clampi(Y + ((116130 * cb + 32768) >> 16), 0, 255);
    if (out_c == 3) {
        o[0] = (unsigned char)r;
        o[1] = (unsigned char)g;
        o[2] = (unsigned char)b;
    } else {
        o[0] = (unsigned char)((19595 * r + 38470 * g + 7471 * b + 32768) >> 16);
    }
}

// ---- restart-interval index: the marker search of jpeg_decode._parse_scan on the device --------------------------------------
// The host uploads every file from the first byte of its entropy-coded data to the file's end (each file's first byte at a
// multiple of 16) and, in the spare columns of its desc row, where: its byte range in `bits`, its first unit row and the units its
// header promises.  The unit rows arrive with everything the bytes do not decide (image, MCU range, table set, workgroup pair,
// padding rows); the kernel fills U_BEGIN / U_END.  One workgroup per file walks it in order, JPEG_IX_CHUNK bytes at a time:
//   a marker is a position i with b[i] == FF and b[i + 1] neither 00 nor FF (the last byte of a file has no b[i + 1]);
//   the scan ends at the first marker that is not RST0..7 (or at the file's end), restart markers behind it are ignored;
//   the k-th restart marker at p ends unit k at p and begins unit k + 1 at p + 2; units past the last found one get (end, end).
// More restart markers than the promised units hold, or another SOS / a DNL among the segments behind the scan, set
// JPEG_ST_INDEX in the file's word of `refused`.  Nothing in the desc row is trusted: the byte range is clamped to `bits`, the row
// range to the table, and a row is written only if it names this file; whatever had to be clamped refuses the file as well.
enum { D_IX_BEGIN = 15, D_IX_END, D_IX_ROW0, D_IX_NUNITS };
enum { JPEG_ST_INDEX = 16 };
constexpr int JPEG_IX_THREADS = 256;
constexpr int JPEG_IX_WAVES = JPEG_IX_THREADS / 64;
constexpr int JPEG_IX_CHUNK = JPEG_IX_THREADS * 16;
constexpr int JPEG_IX_NONE = 0x7FFFFFFF;

typedef unsigned int jpeg_u32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ void jpeg_index_put(int* units, int n_units, int file, int row0, int nunits, int k, int col, int value) {
    if (k < 0 || k >= nunits) return;
    const long row = (long)row0 + k;
    if (row < 0 || row >= n_units) return;
    int* u = units + row * JPEG_UNIT_INTS;
    if (u[U_IMAGE] == file) u[col] = value;
}

__global__ __launch_bounds__(JPEG_IX_THREADS) void jpeg_index_kernel(const unsigned char* bits, long bits_bytes, const int* desc, int* units,
                                                                     int n_units, int* refused) {
    __shared__ int s_min[JPEG_IX_WAVES];
    __shared__ int s_cnt[JPEG_IX_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int file = blockIdx.x;
    const int* d = desc + (long)file * JPEG_DESC_INTS;
    int nunits = d[D_IX_NUNITS], row0 = d[D_IX_ROW0];
    if (nunits == 0) {                                   // a file the kernels do not take: nothing to index
        if (tid == 0) refused[file] = 0;
        return;
    }
    int flags = 0;
    long fb = d[D_IX_BEGIN], fe = d[D_IX_END];
    if (fb < 0 || fe < fb || fe > bits_bytes || (fb & 15)) {
        flags = JPEG_ST_INDEX;
        fb = fe = 0;                                     // (nothing of such a file is read)
    }
    const long room = (long)n_units - row0;              // rows from the file's first to the table's end
    if (nunits < 0 || row0 < 0 || room <= 0 || nunits > room) {
        flags = JPEG_ST_INDEX;
        nunits = (nunits < 0 || row0 < 0 || room <= 0) ? 0 : (int)room;
    }
    if (nunits > 0 && units[(long)row0 * JPEG_UNIT_INTS + U_IMAGE] != file) flags = JPEG_ST_INDEX;      // another file's rows

    int base = 0;                                        // restart markers in front of the chunk
    int end = (int)fe;                                   // the scan's end, once found
    for (long chunk = fb; chunk < fe; chunk += JPEG_IX_CHUNK) {
        const long p = chunk + (long)tid * 16;
        // ---- this lane's 16 bytes and the one behind them; bytes at or past the file's end read as 00
        unsigned w[4] = {0u, 0u, 0u, 0u};
        if (p + 16 <= fe) {
            const jpeg_u32x4 v = *reinterpret_cast<const jpeg_u32x4*>(bits + p);
            w[0] = v[0];
            w[1] = v[1];
            w[2] = v[2];
            w[3] = v[3];
        } else {
            for (int j = 0; j < 16; ++j)
                if (p + j < fe) w[j >> 2] |= (unsigned)bits[p + j] << (8 * (j & 3));
        }
        unsigned next = (unsigned)__shfl_down((int)(w[0] & 0xFFu), 1, 64);
        if (lane == 63) next = 0u;
        const bool last_ff = (w[3] >> 24) == 0xFFu;
        if (lane == 63 && last_ff && p + 16 < fe) next = bits[p + 16];      // (a wave's, and a chunk's, edge)
        unsigned rst = 0u, other = 0u;
        unsigned any_ff = 0u;                                              // (the zero-byte test on the complement)
#pragma unroll
        for (int i = 0; i < 4; ++i) any_ff |= (~w[i] - 0x01010101u) & w[i] & 0x80808080u;
        if (any_ff) {
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                const unsigned cur = (w[j >> 2] >> (8 * (j & 3))) & 0xFFu;
                const unsigned nx = j == 15 ? next : (w[(j + 1) >> 2] >> (8 * ((j + 1) & 3))) & 0xFFu;
                const bool marker = cur == 0xFFu && nx != 0u && nx != 0xFFu;
                const bool restart = (nx & 0xF8u) == 0xD0u;
                rst |= (marker && restart ? 1u : 0u) << j;
                other |= (marker && !restart ? 1u : 0u) << j;
            }
        }
        // ---- the first marker of the chunk that is not a restart marker: wave minimum, then across the waves
        int first = other ? (int)p + __builtin_ctz(other) : JPEG_IX_NONE;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const int o = __shfl_xor(first, off, 64);
            first = o < first ? o : first;
        }
        if (lane == 0) s_min[wave] = first;
        __syncthreads();
        first = s_min[0];
#pragma unroll
        for (int i = 1; i < JPEG_IX_WAVES; ++i) first = s_min[i] < first ? s_min[i] : first;
        // ---- restart markers in front of it: exclusive prefix over the lanes, then over the waves
        if (first != JPEG_IX_NONE) {
            const long keep = (long)first - p;
            rst = keep <= 0 ? 0u : (keep < 16 ? rst & ((1u << keep) - 1u) : rst);
        }
        const int mine = __builtin_popcount(rst);
        int incl = mine;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const int o = __shfl(incl, lane >= off ? lane - off : lane, 64);
            if (lane >= off) incl += o;
        }
        if (lane == 63) s_cnt[wave] = incl;
        __syncthreads();
        int k = base + incl - mine, total = 0;
#pragma unroll
        for (int i = 0; i < JPEG_IX_WAVES; ++i) {
            if (i < wave) k += s_cnt[i];
            total += s_cnt[i];
        }
        while (rst) {
            const int at = (int)p + __builtin_ctz(rst);
            rst &= rst - 1u;
            jpeg_index_put(units, n_units, file, row0, nunits, k, U_END, at);
            jpeg_index_put(units, n_units, file, row0, nunits, k + 1, U_BEGIN, at + 2);
            ++k;
        }
        base += total;
        if (first != JPEG_IX_NONE) {
            end = first;
            break;                                       // (uniform: every lane holds the same `first`)
        }
    }
    if (base > nunits - 1) flags = JPEG_ST_INDEX;        // more restart markers than the interval allows (or than no DRI allows: none)
    // ---- unit 0 begins at the file's begin, the last found unit ends at the scan's end, the promised rest is empty there
    const int found = base + 1 < nunits ? base + 1 : nunits;
    if (tid == 0) jpeg_index_put(units, n_units, file, row0, nunits, 0, U_BEGIN, (int)fb);
    if (tid == 0) jpeg_index_put(units, n_units, file, row0, nunits, base, U_END, end);
    for (int k = found + tid; k < nunits; k += JPEG_IX_THREADS) {
        jpeg_index_put(units, n_units, file, row0, nunits, k, U_BEGIN, end);
        jpeg_index_put(units, n_units, file, row0, nunits, k, U_END, end);
    }
    // ---- what follows the scan, segment by segment on one lane: anything but another scan or a DNL (normally just FF D9)
    if (tid == 0) {
        long q = end;
        while (q + 4 <= fe && bits[q] == 0xFFu && bits[q + 1] != 0xD9u) {
            const unsigned m = bits[q + 1];
            if (m == 0xDAu || m == 0xDCu) {
                flags = JPEG_ST_INDEX;
                break;
            }
            q += m == 0xFFu ? 1 : 2 + (long)(((unsigned)bits[q + 2] << 8) | bits[q + 3]);
        }
        refused[file] = flags;
    }
}

__global__ __launch_bounds__(256) void jpeg_index_status_kernel(const int* refused, int* status, int n_images) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n_images && refused[i]) status[i] |= refused[i];
}

}  // namespace

// the sizes the host builds its tables with
extern "C" int ssn_jpeg_layout(int* desc_ints, int* unit_ints, int* table_words, int* lds_sets) {
    if (desc_ints) *desc_ints = JPEG_DESC_INTS;
    if (unit_ints) *unit_ints = JPEG_UNIT_INTS;
    if (table_words) *table_words = JPEG_TABLE_WORDS;
    if (lds_sets) *lds_sets = JPEG_LDS_SETS;
    return SSN_OK;
}

// Zero-fills coef [total_blocks][64] and status [n_images], then decodes n_units (a multiple of 64) unit rows.
extern "C" int ssn_jpeg_entropy(const unsigned char* bits, long bits_bytes, const int* desc, int n_images, const int* units, int n_units,
                                const unsigned int* tables, int n_sets, short* coef, long total_blocks, int* status,
                                hipStream_t stream) {
    SSN_CHECK_ARG(n_images >= 1 && n_units >= 64 && n_units % 64 == 0 && n_sets >= 1, "jpeg_entropy: bad counts (units come in rows of 64)");
    SSN_CHECK_ARG(bits_bytes >= 0 && bits_bytes < (1L << 31) && total_blocks >= 1 && total_blocks < (1L << 25),
                  "jpeg_entropy: bad buffer sizes");
    SSN_CHECK_ARG((bits || bits_bytes == 0) && desc && units && tables && coef && status, "jpeg_entropy: null pointer");
    if (hipMemsetAsync(coef, 0, (size_t)total_blocks * 64 * sizeof(short), stream) != hipSuccess ||
        hipMemsetAsync(status, 0, (size_t)n_images * sizeof(int), stream) != hipSuccess) {
        ssn_set_error("jpeg_entropy: memset failed");
        return SSN_ERR_LAUNCH;
    }
    hipLaunchKernelGGL(jpeg_entropy_kernel, dim3((unsigned)(n_units / 64)), dim3(64), 0, stream, bits, bits_bytes, desc, n_images, units,
                       tables, n_sets, coef, total_blocks, status);
    SSN_CHECK_LAUNCH("jpeg_entropy");
    return SSN_OK;
}

// max_blocks: the largest block count of an image of the batch (sizes the grid; an image's own count bounds its threads)
extern "C" int ssn_jpeg_idct(const short* coef, long total_blocks, const int* desc, int n_images, int max_blocks,
                             const unsigned short* quant, int n_quant, unsigned char* planes, long plane_bytes, hipStream_t stream) {
    SSN_CHECK_ARG(n_images >= 1 && n_images <= 65535 && max_blocks >= 1 && n_quant >= 1, "jpeg_idct: bad counts");
    SSN_CHECK_ARG(total_blocks >= 1 && plane_bytes >= 64, "jpeg_idct: bad buffer sizes");
    SSN_CHECK_ARG(coef && desc && quant && planes, "jpeg_idct: null pointer");
    SSN_CHECK_ARG(((uintptr_t)planes & 7) == 0, "jpeg_idct: the plane buffer must be 8-byte aligned");
    hipLaunchKernelGGL(jpeg_idct_kernel, dim3((unsigned)((max_blocks + 255) / 256), (unsigned)n_images), dim3(256), 0, stream, coef,
                       total_blocks, desc, quant, n_quant, planes, plane_bytes);
    SSN_CHECK_LAUNCH("jpeg_idct");
    return SSN_OK;
}

// max_pixels: the largest H * W of the batch; out_c 3 (RGB) or 1 (L)
extern "C" int ssn_jpeg_pixels(const unsigned char* planes, long plane_bytes, const int* desc, int n_images, long max_pixels, int out_c,
                               unsigned char* out, long out_bytes, hipStream_t stream) {
    SSN_CHECK_ARG(n_images >= 1 && n_images <= 65535 && max_pixels >= 1 && max_pixels < (1L << 31), "jpeg_pixels: bad counts");
    SSN_CHECK_ARG(out_c == 1 || out_c == 3, "jpeg_pixels: out_c is 1 (L) or 3 (RGB)");
    SSN_CHECK_ARG(plane_bytes >= 64 && out_bytes >= 1, "jpeg_pixels: bad buffer sizes");
    SSN_CHECK_ARG(planes && desc && out, "jpeg_pixels: null pointer");
    hipLaunchKernelGGL(jpeg_pixels_kernel, dim3((unsigned)((max_pixels + 255) / 256), (unsigned)n_images), dim3(256), 0, stream, planes,
                       plane_bytes, desc, out_c, out, out_bytes);
    SSN_CHECK_LAUNCH("jpeg_pixels");
    return SSN_OK;
}

// The restart-interval index of a batch: fills U_BEGIN / U_END of the unit rows the desc rows name (columns 15 .. 18: first byte,
// end byte, first unit row, units) and writes refused int32 [n_images]: 16 for a file the index does not take, else 0.
extern "C" int ssn_jpeg_index(const unsigned char* bits, long bits_bytes, const int* desc, int n_images, int* units, int n_units,
                              int* refused, hipStream_t stream) {
    SSN_CHECK_ARG(n_images >= 1 && n_units >= 64 && n_units % 64 == 0, "jpeg_index: bad counts (units come in rows of 64)");
    SSN_CHECK_ARG(bits_bytes >= 0 && bits_bytes < (1L << 31), "jpeg_index: bad buffer size");
    SSN_CHECK_ARG((bits || bits_bytes == 0) && desc && units && refused, "jpeg_index: null pointer");
    SSN_CHECK_ARG(((uintptr_t)bits & 15) == 0, "jpeg_index: bits must be 16-byte aligned");
    hipLaunchKernelGGL(jpeg_index_kernel, dim3((unsigned)n_images), dim3(JPEG_IX_THREADS), 0, stream, bits, bits_bytes, desc, units, n_units,
                       refused);
    SSN_CHECK_LAUNCH("jpeg_index");
    return SSN_OK;
}

// status[i] |= refused[i]: after ssn_jpeg_entropy, which zeroes status
extern "C" int ssn_jpeg_index_status(const int* refused, int* status, int n_images, hipStream_t stream) {
    SSN_CHECK_ARG(n_images >= 1 && refused && status, "jpeg_index_status: bad arguments");
    hipLaunchKernelGGL(jpeg_index_status_kernel, dim3((unsigned)((n_images + 255) / 256)), dim3(256), 0, stream, refused, status, n_images);
    SSN_CHECK_LAUNCH("jpeg_index_status");
    return SSN_OK;
}
