// The integer ("islow") 8-point transforms of libjpeg, one dimension each, and the encoder's quantisation rule: the ONE copy that
// the decoder (jpeg.hip), the encoder (jpeg_encode.hip) and the gray round trip (jpeg_roundtrip.hip) share, so that the three cannot
// drift apart.  Each works in place on eight ints `stride` apart (registers, or a row / column of a tile).
#pragma once
#include "ssn_common.h"

// jfdctint.c's jpeg_fdct_islow, one dimension: CONST_BITS 13, PASS1_BITS 2.  first: the row pass (results scaled up by 4)
__device__ __forceinline__ void enc_fdct8(int* x, int stride, bool first) {
    const int tmp0 = x[0] + x[7 * stride], tmp7 = x[0] - x[7 * stride];
    const int tmp1 = x[1 * stride] + x[6 * stride], tmp6 = x[1 * stride] - x[6 * stride];
    const int tmp2 = x[2 * stride] + x[5 * stride], tmp5 = x[2 * stride] - x[5 * stride];
    const int tmp3 = x[3 * stride] + x[4 * stride], tmp4 = x[3 * stride] - x[4 * stride];
    const int tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
    const int shift = first ? 11 : 15, half = 1 << (shift - 1);
    if (first) {
        x[0] = (int)((unsigned)(tmp10 + tmp11) << 2);
        x[4 * stride] = (int)((unsigned)(tmp10 - tmp11) << 2);
    } else {
        x[0] = (tmp10 + tmp11 + 2) >> 2;
        x[4 * stride] = (tmp10 - tmp11 + 2) >> 2;
    }
    int z1 = (tmp12 + tmp13) * 4433;
    x[2 * stride] = (z1 + tmp13 * 6270 + half) >> shift;
    x[6 * stride] = (z1 - tmp12 * 15137 + half) >> shift;
    z1 = tmp4 + tmp7;
    int z2 = tmp5 + tmp6, z3 = tmp4 + tmp6, z4 = tmp5 + tmp7;
    const int z5 = (z3 + z4) * 9633;
    const int t4 = tmp4 * 2446, t5 = tmp5 * 16819, t6 = tmp6 * 25172, t7 = tmp7 * 12299;
    z1 *= -7373;
    z2 *= -20995;
    z3 = z3 * -16069 + z5;
    z4 = z4 * -3196 + z5;
    x[7 * stride] = (t4 + z1 + z3 + half) >> shift;
    x[5 * stride] = (t5 + z2 + z4 + half) >> shift;
    x[3 * stride] = (t6 + z2 + z3 + half) >> shift;
    x[1 * stride] = (t7 + z1 + z4 + half) >> shift;
}

__device__ __forceinline__ int enc_quantise(int c, int q) {
    q = q < 1 ? 1 : q;
    const int a = c < 0 ? -c : c;
    const int r = (a + 4 * q) / (8 * q);
    return c < 0 ? -r : r;
}

// jidctint.c's jpeg_idct_islow, one dimension: CONST_BITS 13, results descaled by `shift` with rounding
__device__ __forceinline__ void jpeg_idct8(int* x, int stride, int shift) {
    int z2 = x[2 * stride], z3 = x[6 * stride];
    int z1 = (z2 + z3) * 4433;
    int tmp2 = z1 - z3 * 15137;
    int tmp3 = z1 + z2 * 6270;
    z2 = x[0];
    z3 = x[4 * stride];
    int tmp0 = (int)((unsigned)(z2 + z3) << 13);
    int tmp1 = (int)((unsigned)(z2 - z3) << 13);
    const int tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
    tmp0 = x[7 * stride];
    tmp1 = x[5 * stride];
    tmp2 = x[3 * stride];
    tmp3 = x[1 * stride];
    z1 = tmp0 + tmp3;
    z2 = tmp1 + tmp2;
    z3 = tmp0 + tmp2;
    int z4 = tmp1 + tmp3;
    const int z5 = (z3 + z4) * 9633;
    tmp0 *= 2446;
    tmp1 *= 16819;
    tmp2 *= 25172;
    tmp3 *= 12299;
    z1 *= -7373;
    z2 *= -20995;
    z3 = z3 * -16069 + z5;
    z4 = z4 * -3196 + z5;
    tmp0 += z1 + z3;
    tmp1 += z2 + z4;
    tmp2 += z2 + z3;
    tmp3 += z1 + z4;
    const int half = 1 << (shift - 1);
    x[0] = (tmp10 + tmp3 + half) >> shift;
    x[7 * stride] = (tmp10 - tmp3 + half) >> shift;
    x[1 * stride] = (tmp11 + tmp2 + half) >> shift;
    x[6 * stride] = (tmp11 - tmp2 + half) >> shift;
    x[2 * stride] = (tmp12 + tmp1 + half) >> shift;
    x[5 * stride] = (tmp12 - tmp1 + half) >> shift;
    x[3 * stride] = (tmp13 + tmp0 + half) >> shift;
    x[4 * stride] = (tmp13 - tmp0 + half) >> shift;
}
