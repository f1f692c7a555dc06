// Lossless JPEG transcoding, the stage between the decoder's entropy stage (csrc/jpeg.hip) and the encoder's count stage
// (csrc/jpeg_encode.hip): the quantised coefficients of a batch of files, re-laid from the order one writes to the order the other
// reads.  No coefficient changes its value, so the files written from the result decode to the pixels of the source.
//
//   source       short [block][64]: NATURAL order; blocks PLANAR per image -- luma in raster order over the padded MCU grid
//                (mcux * hs blocks a row, mcuy * vs rows), then Cb, then Cr (mcux blocks a row, mcuy rows); absolute DC
//   destination  short [block][64]: ZIGZAG order; blocks in SCAN order per image -- MCU after MCU in raster order, inside an MCU
//                hs * vs luma blocks (raster), Cb, Cr; dummy blocks included (the source holds them, decoded from the file)
//
// The host describes the batch in desc int32 [images][TR_DESC_INTS].  The kernel does not trust it: a row is used only if its geometry
// is consistent and both of its block ranges lie inside their buffers; any other row sets ENC_ST_DESC in its image's status word and
// writes nothing.
//
// The kernel moves 128 bytes per block and computes nothing: a workgroup takes 32 destination blocks, 8 lanes a block, a lane loads
// one 16-byte piece of the source row (the 8 lanes of a block read its 128 contiguous bytes), parks it in LDS, and after the barrier
// picks its 8 zigzag neighbours out of the block's LDS row and stores them as one 16-byte piece of the destination row (a wave writes
// 1 KiB of consecutive bytes).
#include "ssn_common.h"

namespace {

constexpr int TR_DESC_INTS = 8;
constexpr int TR_BLOCKS = 32;       // destination blocks of a workgroup (256 lanes, 8 a block)
constexpr int TR_ROW = 72;          // shorts of a block's LDS row: 64 + 8, so that rows stay 16-byte aligned and start 4 banks apart
enum { T_NCOMP = 0, T_HS, T_VS, T_MCUX, T_MCUY, T_SRC_OFF, T_DST_OFF, T_NBLOCKS };
enum { ENC_ST_DESC = 4 };           // the status bit of jpeg_encode.hip for an unusable desc row

typedef unsigned int tr_u32x4 __attribute__((ext_vector_type(4)));

__device__ const unsigned char tr_natural_order[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                                       41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                                       30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

// grid (ceil(max blocks of an image / 32), images)
__global__ __launch_bounds__(256) void jpeg_transcode_blocks_kernel(const short* src, long src_blocks, const int* desc, short* dst,
                                                                    long dst_blocks, int* status) {
    __shared__ __attribute__((aligned(16))) short s_blk[TR_BLOCKS * TR_ROW];
    const int image = blockIdx.y, t = threadIdx.x;
    const int* d = desc + (long)image * TR_DESC_INTS;
    const int ncomp = d[T_NCOMP], hs = d[T_HS], vs = d[T_VS], mcux = d[T_MCUX], mcuy = d[T_MCUY];
    const long src_off = d[T_SRC_OFF], dst_off = d[T_DST_OFF];
    const long nblocks = d[T_NBLOCKS];
    // (every term is the same for the whole workgroup: the returns below are taken by all of its lanes or by none)
    bool ok = (ncomp == 1 || ncomp == 3) && hs >= 1 && hs <= 2 && vs >= 1 && vs <= hs && (ncomp == 3 || hs == 1) && mcux >= 1 &&
              mcux <= 8192 && mcuy >= 1 && mcuy <= 8192;
    const int luma = ok ? hs * vs : 1, bpm = ncomp == 1 ? 1 : luma + 2;
    const long mcus = ok ? (long)mcux * mcuy : 0;
    ok = ok && nblocks == mcus * bpm && nblocks < (1L << 25) && src_off >= 0 && src_off + nblocks <= src_blocks && dst_off >= 0 &&
         dst_off + nblocks <= dst_blocks;
    if (!ok) {
        if (blockIdx.x == 0 && t == 0) atomicOr(status + image, ENC_ST_DESC);
        return;
    }
    const long first = (long)blockIdx.x * TR_BLOCKS;
    if (first >= nblocks) return;
    const int b = t >> 3, piece = t & 7;
    const long lb = first + b;              // destination block of the image, scan order
    const bool live = lb < nblocks;
    if (live) {
        const int mcu = (int)(lb / bpm), j = (int)(lb - (long)mcu * bpm);
        const int my = mcu / mcux, mx = mcu - my * mcux;
        long sb;                            // the same block in the planar order
        if (j < luma) {
            const int bx = mx * hs + (j & (hs - 1)), by = my * vs + (j >> (hs - 1));
            sb = (long)by * (mcux * hs) + bx;
        } else {
            sb = mcus * luma + (long)(j - luma) * mcus + (long)my * mcux + mx;
        }
        // sb < nblocks: by < mcuy * vs and bx < mcux * hs, resp. j - luma < 2 with ncomp == 3
        const tr_u32x4 v = *reinterpret_cast<const tr_u32x4*>(src + (src_off + sb) * 64 + piece * 8);
        *reinterpret_cast<tr_u32x4*>(s_blk + b * TR_ROW + piece * 8) = v;
    }
    __syncthreads();
    if (!live) return;
    const short* row = s_blk + b * TR_ROW;
    tr_u32x4 out;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const unsigned lo = (unsigned short)row[tr_natural_order[piece * 8 + 2 * i]];
        const unsigned hi = (unsigned short)row[tr_natural_order[piece * 8 + 2 * i + 1]];
        out[i] = lo | (hi << 16);
    }
    *reinterpret_cast<tr_u32x4*>(dst + (dst_off + lb) * 64 + piece * 8) = out;
}

}  // namespace

// ints of a desc row: ncomp, hs, vs, mcux, mcuy, first source block, first destination block, blocks
extern "C" int ssn_jpeg_transcode_layout(int* desc_ints) {
    if (desc_ints) *desc_ints = TR_DESC_INTS;
    return SSN_OK;
}

// Zero-fills status [n_images], then gathers.  max_blocks: the largest block count of an image of the batch (sizes the grid; an
// image's own count bounds its workgroups).  Blocks of dst that no row names are left as they are.
extern "C" int ssn_jpeg_transcode_blocks(const short* src, long src_blocks, const int* desc, int n_images, int max_blocks, short* dst,
                                         long dst_blocks, int* status, hipStream_t stream) {
    SSN_CHECK_ARG(n_images >= 1 && n_images <= 65535 && max_blocks >= 1 && src_blocks >= 1 && src_blocks < (1L << 25) && dst_blocks >= 1 &&
                      dst_blocks < (1L << 25),
                  "jpeg_transcode_blocks: bad counts");
    SSN_CHECK_ARG(src && desc && dst && status, "jpeg_transcode_blocks: null pointer");
    SSN_CHECK_ARG(((uintptr_t)src & 15) == 0 && ((uintptr_t)dst & 15) == 0,
                  "jpeg_transcode_blocks: the coefficient buffers must be 16-byte aligned");
    SSN_CHECK_ARG(src != dst, "jpeg_transcode_blocks: source and destination must differ");
    if (hipMemsetAsync(status, 0, (size_t)n_images * sizeof(int), stream) != hipSuccess) {
        ssn_set_error("jpeg_transcode_blocks: memset failed");
        return SSN_ERR_LAUNCH;
    }
    hipLaunchKernelGGL(jpeg_transcode_blocks_kernel, dim3((unsigned)((max_blocks + TR_BLOCKS - 1) / TR_BLOCKS), (unsigned)n_images),
                       dim3(256), 0, stream, src, src_blocks, desc, dst, dst_blocks, status);
    SSN_CHECK_LAUNCH("jpeg_transcode_blocks");
    return SSN_OK;
}
