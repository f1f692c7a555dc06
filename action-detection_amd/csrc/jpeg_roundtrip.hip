// What a gray image looks like after Image.save(f, "JPEG", quality=q) and Image.open(f).convert("L"), without the file: per 8 x 8
// block the level shift, the encoder's forward DCT and quantisation, the multiplication back by the table, the decoder's inverse DCT
// and its range limit.  The entropy coding between the two halves is lossless, so leaving it out changes no pixel.
// The transforms are the encoder's and the decoder's own (jpeg_dct.h).
//
// A workgroup of 256 lanes takes 32 consecutive blocks of the flat block order (image, block row, block column), 8 lanes a block.
// A lane is pixel ROW `l` of its block in the first and the last pass and COLUMN `l` in the two passes between; the block changes
// hands through a padded LDS tile:
//
//   1  load row l (8 bytes at once where the row is inside the image and aligned, else bytes with the edge pixel repeated), level
//      shift, forward row pass                                                                                         -> tile
//   2  column l of the tile: forward column pass, quantise, dequantise, inverse COLUMN pass (the decoder starts with the columns, so
//      the coefficients never leave the registers)                                                                    -> tile
//   3  row l of the tile: inverse row pass, + 128, clamp, store the pixels that are inside the image
//
// A block reads and writes its own 8 x 8 pixels only (the repeated edge pixels are its own), and every read of a block is done before
// the first barrier while every write comes after the second: dst may be src.
#include "ssn_common.h"
#include "jpeg_dct.h"

namespace {

constexpr int RT_BLOCKS = 32;      // blocks of a workgroup (256 lanes, 8 a block)
constexpr int RT_ROW = 9;          // ints of a tile row: 8 + 1, so that the 8 lanes of a block hit 8 banks by row and by column
constexpr int RT_TILE = 8 * RT_ROW;      // 72 ints a block: 4 consecutive blocks start 8 banks apart, 32 lanes cover the 32 banks

__global__ __launch_bounds__(256) void jpeg_roundtrip_gray_kernel(const unsigned char* src, unsigned char* dst, int H, int W, int bw,
                                                                  long blocks_per_image, long total_blocks, const int* quant64) {
    __shared__ int s_tile[RT_BLOCKS * RT_TILE];
    __shared__ int s_q[64];
    const int t = threadIdx.x, b = t >> 3, l = t & 7;
    if (t < 64) {
        const int q = quant64[t];
        s_q[t] = q < 1 ? 1 : (q > 255 ? 255 : q);      // (an 8-bit table; the host has checked it)
    }
    const long gb = (long)blockIdx.x * RT_BLOCKS + b;
    const bool live = gb < total_blocks;
    int* tile = s_tile + b * RT_TILE;
    long image_off = 0;
    int x0 = 0, y0 = 0;
    if (live) {
        const long n = gb / blocks_per_image;
        const int r = (int)(gb - n * blocks_per_image);      // blocks_per_image < 2^26 (65535 x 65535 pixels at most)
        const int by = r / bw, bx = r - by * bw;
        image_off = n * ((long)H * W);
        x0 = bx * 8;
        y0 = by * 8;
        // ---- 1: row l, edge pixels repeated
        const int y = y0 + l < H ? y0 + l : H - 1;
        const unsigned char* p = src + image_off + (long)y * W + x0;
        int x[8];
        if (x0 + 8 <= W && ((uintptr_t)p & 3) == 0) {
            uint32_t w0, w1;
            if (((uintptr_t)p & 7) == 0) {
                const uint2 v = *reinterpret_cast<const uint2*>(p);
                w0 = v.x;
                w1 = v.y;
            } else {
                w0 = *reinterpret_cast<const uint32_t*>(p);
                w1 = *reinterpret_cast<const uint32_t*>(p + 4);
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                x[i] = (int)((w0 >> (8 * i)) & 0xFFu) - 128;
                x[4 + i] = (int)((w1 >> (8 * i)) & 0xFFu) - 128;
            }
        } else {
            const int last = W - 1 - x0;      // >= 0: the block starts inside the image
#pragma unroll
            for (int i = 0; i < 8; ++i) x[i] = (int)p[i < last ? i : last] - 128;
        }
        enc_fdct8(x, 1, true);
#pragma unroll
        for (int i = 0; i < 8; ++i) tile[l * RT_ROW + i] = x[i];
    }
    __syncthreads();
    if (live) {
        // ---- 2: column l
        int x[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) x[i] = tile[i * RT_ROW + l];
        enc_fdct8(x, 1, false);
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int q = s_q[8 * i + l];
            x[i] = enc_quantise(x[i], q) * q;
        }
        jpeg_idct8(x, 1, 11);
#pragma unroll
        for (int i = 0; i < 8; ++i) tile[i * RT_ROW + l] = x[i];      // (the lane's own column: nobody else reads or writes it in this pass)
    }
    __syncthreads();
    if (live && y0 + l < H) {
        // ---- 3: row l
        int x[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) x[i] = tile[l * RT_ROW + i];
        jpeg_idct8(x, 1, 18);
        uint32_t w[2] = {0, 0};
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            int v = x[i] + 128;
            v = v < 0 ? 0 : (v > 255 ? 255 : v);
            x[i] = v;
            w[i >> 2] |= (uint32_t)v << (8 * (i & 3));
        }
        unsigned char* p = dst + image_off + (long)(y0 + l) * W + x0;
        if (x0 + 8 <= W && ((uintptr_t)p & 3) == 0) {
            if (((uintptr_t)p & 7) == 0) {
                *reinterpret_cast<uint2*>(p) = uint2{w[0], w[1]};
            } else {
                *reinterpret_cast<uint32_t*>(p) = w[0];
                *reinterpret_cast<uint32_t*>(p + 4) = w[1];
            }
        } else {
            const int n = W - x0 < 8 ? W - x0 : 8;
#pragma unroll
            for (int i = 0; i < 8; ++i)
                if (i < n) p[i] = (unsigned char)x[i];
        }
    }
}

}  // namespace

// src, dst uint8 [n][h][w] (dst may be src); quant64 int32 [64] on the device: the table in natural order, 1 .. 255
extern "C" int ssn_jpeg_roundtrip_gray(const unsigned char* src, unsigned char* dst, int n, int h, int w, const int* quant64,
                                       hipStream_t stream) {
    SSN_CHECK_ARG(n >= 1 && h >= 1 && w >= 1 && h <= 65535 && w <= 65535, "jpeg_roundtrip_gray: bad sizes (n >= 1, h and w 1 .. 65535)");
    SSN_CHECK_ARG(src && dst && quant64, "jpeg_roundtrip_gray: null pointer");
    SSN_CHECK_ARG(((uintptr_t)quant64 & 3) == 0, "jpeg_roundtrip_gray: the table must be 4-byte aligned");
    const int bw = (w + 7) / 8, bh = (h + 7) / 8;
    const long per_image = (long)bw * bh, total = per_image * n;
    const long groups = (total + RT_BLOCKS - 1) / RT_BLOCKS;
    SSN_CHECK_ARG(groups < (1L << 31), "jpeg_roundtrip_gray: too many blocks for one launch");
    hipLaunchKernelGGL(jpeg_roundtrip_gray_kernel, dim3((unsigned)groups), dim3(256), 0, stream, src, dst, h, w, bw, per_image, total,
                       quant64);
    SSN_CHECK_LAUNCH("jpeg_roundtrip_gray");
    return SSN_OK;
}
