// Input side of the hot path on the GPU: crop / horizontal flip / channel roll / float conversion / normalisation of
// decoded uint8 frames, i.e. the arithmetic of the reference's transform chain after image decoding and scaling
//   GroupOverSample | (crop + GroupRandomHorizontalFlip)  ->  Stack(roll)  ->  ToTorchFormatTensor(div=False)  ->
//   GroupNormalize          (/root/reference/transforms.py:103-132, 49-64, 256-268, 271-288, 67-80;
//                            wired at ssn_test.py:101-112 and ssn_train.py:106-111)
// which the reference runs image by image in PIL / numpy on the loader workers ("this transpose takes 80% of the
// loading time", transforms.py:286).  HBM-bound: 1 byte read, 4 bytes written per output element.
#include "ssn_common.h"

namespace {

constexpr int MAX_CROPS = 16;
struct CropTable {
    int n;
    int ox[MAX_CROPS], oy[MAX_CROPS], flip[MAX_CROPS];
};

// src [n_img][Hs][Ws][C] uint8 (HWC as decoded);  dst [n_crops][n_img][C][ch][cw] fp32
//   dst[k][i][c][y][x] = (float(px) - mean[c]) / std[c],
//   px = src[i][oy_k + y][ox_k + (flip_k ? cw - 1 - x : x)][roll ? C - 1 - c : c],
//   px = 255 - px when invert_even && flip_k && i is even (flow: the x component changes sign under a flip).
__global__ __launch_bounds__(256) void frames_kernel(const uint8_t* src, float* dst, int n_img, int Hs, int Ws, int C,
                                                     int ch, int cw, CropTable t, int roll, int invert_even,
                                                     const float* mean, const float* stdv, int n_mean, int n_std) {
    const long plane = (long)ch * cw;
    const long total = (long)t.n * n_img * C * plane;
    for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long)gridDim.x * 256) {
        const int x = (int)(idx % cw);
        long r = idx / cw;
        const int y = (int)(r % ch);
        r /= ch;
        const int c = (int)(r % C);
        r /= C;
        const int i = (int)(r % n_img);
        const int k = (int)(r / n_img);
        const int sx = t.ox[k] + (t.flip[k] ? cw - 1 - x : x);
        const int sc = roll ? C - 1 - c : c;
        int px = src[(((long)i * Hs + t.oy[k] + y) * Ws + sx) * C + sc];
        if (invert_even && t.flip[k] && (i & 1) == 0) px = 255 - px;
        // GroupNormalize repeats mean / std over the stacked channels: channel (i * C + c) of the stack
        const int sch = i * C + c;
        dst[idx] = ((float)px - mean[sch % n_mean]) / stdv[sch % n_std];
    }
}

// RGBDiff input (SSN._get_diff, /root/reference/ssn_models.py:302-316, keep_rgb = False): every segment holds
// new_length + 1 stacked RGB frames; the network sees the new_length differences of consecutive frames,
//   out[g][x][c][hw] = in[g][x + 1][c][hw] - in[g][x][c][hw],   x < new_length
// i.e. out[g][j] = in[g][j + plane] - in[g][j] with plane = C * HW floats and j < new_length * plane.
__global__ __launch_bounds__(256) void frame_diff_kernel(const float* in, float* out, long per_seg_out, long per_seg_in,
                                                         long plane, long total) {
    for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long)gridDim.x * 256) {
        const long g = idx / per_seg_out, j = idx - g * per_seg_out;
        const float* src = in + g * per_seg_in + j;
        out[idx] = src[plane] - src[0];
    }
}


// ---------------------------------------------------------------------------------------------------------------------------
// Training augmentation on the GPU: GroupMultiScaleCrop (crop + PIL bilinear resize to the network input) ->
// GroupRandomHorizontalFlip -> Stack(roll) -> ToTorchFormatTensor(div=False) -> GroupNormalize
// (/root/reference/transforms.py:135-206, 49-64, 256-268, 271-288, 67-80; the chain of ssn_train.py:106-111 with
// SSN.get_augmentation(), ssn_models.py:386-395) on decoded uint8 frames, so that loader workers only decode.
//
// The resize restates Pillow's ImagingResample for 8-bit images (what `img.crop(box).resize(size, Image.BILINEAR)` runs): per
// axis, output index xx takes the source window [xmin, xmin + n) around centre (xx + 0.5) * scale with triangle weights of
// support max(scale, 1), normalised, rounded to 22-bit fixed point; the horizontal pass rounds to uint8 before the vertical
// pass reads it.  Coefficients are computed in double with contraction off -- the same IEEE operations in the same order as
// the C library -- so the result is bit-identical to PIL's, not "within an LSB".
constexpr int RS_MAXK = 7;                 // taps per axis: downscaling by up to 3x
constexpr int RS_ENT = 2 + RS_MAXK;        // ints per table entry: first source index, tap count, coefficients
constexpr int RS_PREC = 22;                // Pillow: PRECISION_BITS = 32 - 8 - 2

// one thread per (image, axis, output index): tab[img][out_w + out_h][RS_ENT]
__global__ __launch_bounds__(256) void resize_coeffs_kernel(const int* box, int n_img, int out_w, int out_h, int* tab) {
#pragma clang fp contract(off)
    const int per = out_w + out_h;
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= n_img * per) return;
    const int img = t / per, j = t - img * per;
    const bool vert = j >= out_w;
    const int xx = vert ? j - out_w : j;
    const int inSize = box[img * 4 + (vert ? 3 : 2)], outSize = vert ? out_h : out_w;
    double scale = (double)inSize / (double)outSize;
    double filterscale = scale;
    if (filterscale < 1.0) filterscale = 1.0;
    const double support = 1.0 * filterscale;          // bilinear: support 1
    const double center = 0.0 + (xx + 0.5) * scale;
    const double ss = 1.0 / filterscale;
    int xmin = (int)(center - support + 0.5);
    if (xmin < 0) xmin = 0;
    int xmax = (int)(center + support + 0.5);
    if (xmax > inSize) xmax = inSize;
    xmax -= xmin;
    if (xmax > RS_MAXK) xmax = RS_MAXK;                 // (the host refuses such boxes)
    double k[RS_MAXK];
    double ww = 0.0;
    for (int x = 0; x < RS_MAXK; ++x) {
        double w = 0.0;
        if (x < xmax) {
            double a = (x + xmin - center + 0.5) * ss;
            if (a < 0.0) a = -a;
            w = a < 1.0 ? 1.0 - a : 0.0;
        }
        k[x] = w;
        ww += w;
    }
    int* e = tab + ((long)img * per + j) * RS_ENT;
    e[0] = xmin;
    e[1] = xmax;
    for (int x = 0; x < RS_MAXK; ++x) {
        double v = k[x];
        if (ww != 0.0) v /= ww;
        e[2 + x] = v < 0 ? (int)(-0.5 + v * (double)(1 << RS_PREC)) : (int)(0.5 + v * (double)(1 << RS_PREC));
    }
}

__device__ __forceinline__ int rs_clip8(int v) {
    v >>= RS_PREC;
    return v < 0 ? 0 : (v > 255 ? 255 : v);
}

// dst [n_img][C][out_h][out_w] fp32 = normalise(roll(flip(resize(crop(src[i], box[i])))))
__global__ __launch_bounds__(256) void frames_resize_kernel(const uint8_t* src, float* dst, int n_img, int Hs, int Ws, int C,
                                                            int out_h, int out_w, const int* box, const int* flip,
                                                            const int* tab, int roll, int invert_even, const float* mean,
                                                            const float* stdv, int n_mean, int n_std) {
    const long plane = (long)out_h * out_w;
    const long total = (long)n_img * C * plane;
    const int per = out_w + out_h;
    for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long)gridDim.x * 256) {
        const int x = (int)(idx % out_w);
        long r = idx / out_w;
        const int y = (int)(r % out_h);
        r /= out_h;
        const int c = (int)(r % C);
        const int i = (int)(r / C);
        const int fl = flip[i];
        const int rx = fl ? out_w - 1 - x : x;                       // FLIP_LEFT_RIGHT is applied to the resized image
        const int sc = roll ? C - 1 - c : c;
        const int x0 = box[i * 4 + 0], y0 = box[i * 4 + 1];
        const int* eh = tab + ((long)i * per + rx) * RS_ENT;
        const int* ev = tab + ((long)i * per + out_w + y) * RS_ENT;
        const int hx = eh[0], hn = eh[1], vy = ev[0], vn = ev[1];
        int acc_v = 1 << (RS_PREC - 1);
        for (int ky = 0; ky < vn; ++ky) {
            const uint8_t* row = src + (((long)i * Hs + y0 + vy + ky) * Ws + x0 + hx) * C + sc;
            int acc_h = 1 << (RS_PREC - 1);
            for (int kx = 0; kx < hn; ++kx) acc_h += (int)row[(long)kx * C] * eh[2 + kx];
            acc_v += rs_clip8(acc_h) * ev[2 + ky];                   // (the horizontal pass is stored as uint8 by Pillow)
        }
        int px = rs_clip8(acc_v);
        if (invert_even && fl && (i & 1) == 0) px = 255 - px;
        const int sch = i * C + c;
        dst[idx] = ((float)px - mean[sch % n_mean]) / stdv[sch % n_std];
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// Test-time GroupScale on the GPU: the WHOLE frame through Pillow's 8-bit bilinear ImagingResample, uint8 -> uint8
// (transforms.py:83-96 inside GroupOverSample, :103-132, and in front of GroupCenterCrop: ssn_test.py:107-115).  The
// ten crops are cut from the scaled frame afterwards by frames_kernel, so the result has to exist as an image: the kernel above
// cannot express that, recomputes the horizontal pass for every vertical tap and stops at 7 taps.
//
// All frames of a call share one size (the frames of one video), so there is ONE coefficient table of out_w + out_h entries per
// call, built like resize_coeffs_kernel builds its per-image ones (double, contraction off, normalised, 22-bit fixed point).  One
// workgroup per (image, tile of SC_TH x SC_TW output pixels): stage 1 runs the horizontal pass for exactly the source rows the
// tile's output rows read and leaves it in LDS as uint8 (Pillow's intermediate image is 8-bit: rounded and clipped before the
// vertical pass reads it), stage 2 runs the vertical pass out of LDS.  Both stages work on dwords of 4 consecutive output bytes
// (x * C + c order, the layout of the output row), so LDS traffic is one conflict-free dword per lane and the stores are packed.
constexpr int SC_MAXK = 13;                // taps per axis.  Pillow's window is floor(c + s + .5) - floor(c - s + .5) <= floor(2 s) + 1
                                           // source pixels for support s = max(in / out, 1): 13 taps hold every s < 6.5
constexpr int SC_ENT = 2 + SC_MAXK;        // ints per table entry: first source index, tap count, coefficients
constexpr int SC_TH = 16, SC_TW = 64;      // output pixels per tile
// source rows under one tile: from floor(c_first - s + .5) to floor(c_last + s + .5) with c_last - c_first = (SC_TH - 1) s, i.e.
// fewer than (SC_TH + 1) s + 1 rows, s < 6.5  (at the documented ratio of 6 this is 6 SC_TH + 7 <= 6 SC_TH + 13)
constexpr int SC_ROWS = (13 * (SC_TH + 1)) / 2 + 1;
constexpr int SC_STRIDE = SC_TW * 3;       // bytes per LDS row: a tile row of RGB pixels
constexpr int SC_LDS_BYTES = SC_ROWS * SC_STRIDE + (SC_TW + SC_TH) * SC_ENT * (int)sizeof(int);
static_assert(SC_ROWS >= 6 * SC_TH + 13, "LDS rows: the tile height at ratio 6 with 13 taps must fit");
static_assert(SC_STRIDE % 4 == 0, "LDS rows are read and written as dwords");
static_assert(SC_LDS_BYTES <= 64 * 1024, "frames_scale: LDS footprint");
static_assert(SC_LDS_BYTES * 4 <= 160 * 1024, "frames_scale: four workgroups per CU by LDS");

// Four clipped accumulators as the bytes of one dword.  Through v_perm_b32, not `b0 | b1 << 8 | b2 << 16 | b3 << 24`: for that form hipcc
// emitted `v_ashr_pk_u8_i32 v1, a0, a1, 22` followed by `v_or3_b32 v1, v1, b2 << 16, b3 << 24`, and on the MI355X bytes 2 and 3 of every
// output row with an even tap count (the path where v1 had held an accumulator before) came out with extra bits set, as if the upper half
// of v1 had kept its old contents.  With this form neither the instruction nor the wrong bytes appear; the GPU tier of
// tests/test_frames_scale.py pins the result (the host emulator cannot show the difference).
__device__ __forceinline__ uint32_t sc_pack4(int a0, int a1, int a2, int a3) {
    const uint32_t lo = __builtin_amdgcn_perm((uint32_t)rs_clip8(a1), (uint32_t)rs_clip8(a0), 0x0c0c0400u);
    const uint32_t hi = __builtin_amdgcn_perm((uint32_t)rs_clip8(a3), (uint32_t)rs_clip8(a2), 0x0c0c0400u);
    return __builtin_amdgcn_perm(hi, lo, 0x05040100u);
}

// one thread per (axis, output index): tab[out_w + out_h][SC_ENT]
__global__ __launch_bounds__(256) void scale_coeffs_kernel(int in_w, int in_h, int out_w, int out_h, int* tab) {
#pragma clang fp contract(off)
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= out_w + out_h) return;
    const bool vert = j >= out_w;
    const int xx = vert ? j - out_w : j;
    const int inSize = vert ? in_h : in_w, outSize = vert ? out_h : out_w;
    double scale = (double)inSize / (double)outSize;
    double filterscale = scale;
    if (filterscale < 1.0) filterscale = 1.0;
    const double support = 1.0 * filterscale;          // bilinear: support 1
    const double center = 0.0 + (xx + 0.5) * scale;
    const double ss = 1.0 / filterscale;
    int xmin = (int)(center - support + 0.5);
    if (xmin < 0) xmin = 0;
    int xmax = (int)(center + support + 0.5);
    if (xmax > inSize) xmax = inSize;
    xmax -= xmin;
    if (xmax > SC_MAXK) xmax = SC_MAXK;                 // (the host refuses such sizes)
    double k[SC_MAXK];
    double ww = 0.0;
    for (int x = 0; x < SC_MAXK; ++x) {
        double w = 0.0;
        if (x < xmax) {
            double a = (x + xmin - center + 0.5) * ss;
            if (a < 0.0) a = -a;
            w = a < 1.0 ? 1.0 - a : 0.0;
        }
        k[x] = w;
        ww += w;
    }
    int* e = tab + (long)j * SC_ENT;
    e[0] = xmin;
    e[1] = xmax;
    for (int x = 0; x < SC_MAXK; ++x) {
        double v = k[x];
        if (ww != 0.0) v /= ww;
        e[2 + x] = v < 0 ? (int)(-0.5 + v * (double)(1 << RS_PREC)) : (int)(0.5 + v * (double)(1 << RS_PREC));
    }
}

// src [n_img][Hs][Ws][C] uint8 -> dst [n_img][out_h][out_w][C] uint8; grid (tiles in x, tiles in y, image)
__global__ __launch_bounds__(256) void frames_scale_kernel(const uint8_t* src, uint8_t* dst, int Hs, int Ws, int C, int out_h,
                                                           int out_w, const int* tab) {
    __shared__ int s_h[SC_TW * SC_ENT];
    __shared__ int s_v[SC_TH * SC_ENT];
    __shared__ uint32_t s_px[SC_ROWS * (SC_STRIDE / 4)];
    const int tid = threadIdx.x;
    const int img = blockIdx.z;
    const int x0 = blockIdx.x * SC_TW, y0 = blockIdx.y * SC_TH;
    const int tw = out_w - x0 < SC_TW ? out_w - x0 : SC_TW;
    const int th = out_h - y0 < SC_TH ? out_h - y0 : SC_TH;
    for (int i = tid; i < tw * SC_ENT; i += 256) s_h[i] = tab[(long)x0 * SC_ENT + i];
    for (int i = tid; i < th * SC_ENT; i += 256) s_v[i] = tab[(long)(out_w + y0) * SC_ENT + i];
    __syncthreads();
    // the source rows this tile reads: first row of its first output row .. last row of its last one (both grow with y)
    const int row0 = s_v[0];
    int nrows = s_v[(th - 1) * SC_ENT] + s_v[(th - 1) * SC_ENT + 1] - row0;
    if (nrows > SC_ROWS) nrows = SC_ROWS;               // (cannot happen below ratio 6.5; keeps LDS indices in range regardless)
    const int rowbytes = tw * C;
    const int rowdw = (rowbytes + 3) >> 2;

    // stage 1: horizontal pass of rows [row0, row0 + nrows), 4 output bytes per item
    for (int it = tid; it < nrows * rowdw; it += 256) {
        const int r = it / rowdw, d = it - r * rowdw;
        const uint8_t* srow = src + ((long)img * Hs + row0 + r) * Ws * C;
        int acc4[4] = {0, 0, 0, 0};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int b = d * 4 + j;
            if (b < rowbytes) {
                const int xl = C == 3 ? b / 3 : b;
                const int c = b - xl * C;
                const int* e = s_h + xl * SC_ENT;
                const int hn = e[1];
                const uint8_t* p = srow + (long)e[0] * C + c;
                int acc = 1 << (RS_PREC - 1);
                for (int kx = 0; kx < hn; ++kx) acc += (int)p[kx * C] * e[2 + kx];
                acc4[j] = acc;
            }
        }
        s_px[r * (SC_STRIDE / 4) + d] = sc_pack4(acc4[0], acc4[1], acc4[2], acc4[3]);
    }
    __syncthreads();

    // stage 2: vertical pass out of LDS, packed stores
    for (int it = tid; it < th * rowdw; it += 256) {
        const int y = it / rowdw, d = it - y * rowdw;
        const int* e = s_v + y * SC_ENT;
        const int vy = e[0] - row0;
        int vn = e[1];
        if (vy + vn > nrows) vn = nrows - vy;
        int a0 = 1 << (RS_PREC - 1), a1 = a0, a2 = a0, a3 = a0;
        for (int ky = 0; ky < vn; ++ky) {
            const uint32_t w = s_px[(vy + ky) * (SC_STRIDE / 4) + d];
            const int cf = e[2 + ky];
            a0 += (int)(w & 255u) * cf;
            a1 += (int)((w >> 8) & 255u) * cf;
            a2 += (int)((w >> 16) & 255u) * cf;
            a3 += (int)(w >> 24) * cf;
        }
        const uint32_t pack = sc_pack4(a0, a1, a2, a3);
        uint8_t* q = dst + (((long)img * out_h + y0 + y) * out_w + x0) * C + d * 4;
        const int valid = rowbytes - d * 4 < 4 ? rowbytes - d * 4 : 4;
        if (valid == 4 && ((uintptr_t)q & 3) == 0) {
            *reinterpret_cast<uint32_t*>(q) = pack;
        } else {
            for (int j = 0; j < valid; ++j) q[j] = (uint8_t)(pack >> (8 * j));
        }
    }
}

}  // namespace

extern "C" int ssn_frame_diff(const float* in, float* out, long n_segments, int new_length, int C, int HW,
                              hipStream_t stream) {
    SSN_CHECK_ARG(in && out && n_segments >= 0 && new_length >= 1 && C >= 1 && HW >= 1, "frame_diff: bad arguments");
    const long plane = (long)C * HW;
    const long total = n_segments * new_length * plane;
    if (total == 0) return SSN_OK;
    long blocks = (total + 256 * 8 - 1) / (256 * 8);
    if (blocks > 65535 * 4) blocks = 65535 * 4;
    hipLaunchKernelGGL(frame_diff_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, in, out, new_length * plane,
                       (new_length + 1) * plane, plane, total);
    SSN_CHECK_LAUNCH("frame_diff");
    return SSN_OK;
}

extern "C" int ssn_frames_crop_normalize(const unsigned char* src, float* dst, int n_img, int Hs, int Ws, int C,
                                         int crop_h, int crop_w, int n_crops, const int* off_x, const int* off_y,
                                         const int* flip, int roll, int invert_even, const float* mean, int n_mean,
                                         const float* stdv, int n_std, hipStream_t stream) {
    SSN_CHECK_ARG(src && dst && off_x && off_y && flip && mean && stdv, "frames: null pointer");
    SSN_CHECK_ARG(n_crops >= 1 && n_crops <= MAX_CROPS, "frames: %d crops (max %d)", n_crops, MAX_CROPS);
    SSN_CHECK_ARG(n_mean >= 1 && n_std >= 1 && C >= 1, "frames: bad channel arguments");
    CropTable t;
    t.n = n_crops;
    for (int k = 0; k < n_crops; ++k) {
        SSN_CHECK_ARG(off_x[k] >= 0 && off_y[k] >= 0 && off_x[k] + crop_w <= Ws && off_y[k] + crop_h <= Hs,
                      "frames: crop %d (%d, %d) + %dx%d leaves the %dx%d frame", k, off_x[k], off_y[k], crop_w, crop_h, Ws, Hs);
        t.ox[k] = off_x[k];
        t.oy[k] = off_y[k];
        t.flip[k] = flip[k];
    }
    const long total = (long)n_crops * n_img * C * crop_h * crop_w;
    if (total == 0) return SSN_OK;
    long blocks = (total + 256 * 8 - 1) / (256 * 8);
    if (blocks > 65535 * 4) blocks = 65535 * 4;
    hipLaunchKernelGGL(frames_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, (const uint8_t*)src, dst, n_img, Hs, Ws,
                       C, crop_h, crop_w, t, roll, invert_even, mean, stdv, n_mean, n_std);
    SSN_CHECK_LAUNCH("frames_crop_normalize");
    return SSN_OK;
}

// GroupMultiScaleCrop + GroupRandomHorizontalFlip + Stack + ToTorchFormatTensor + GroupNormalize in two launches (see above).
// src [n_img][Hs][Ws][C] uint8 (decoded frames, HWC); dst [n_img][C][out_h][out_w] fp32.  box: DEVICE int [n_img][4] =
// (x0, y0, crop_w, crop_h) of every image (the reference draws one box per group = per proposal: ssn_dataset.py:347-380), flip:
// DEVICE int [n_img].  The caller validates the boxes (they must lie inside the frame; crop / output <= 3 per axis).
// workspace: ssn_frames_resize_workspace_bytes(n_img, out_h, out_w) bytes of device memory (the coefficient tables).
extern "C" size_t ssn_frames_resize_workspace_bytes(int n_img, int out_h, int out_w) {
    return (size_t)n_img * (size_t)(out_h + out_w) * RS_ENT * sizeof(int);
}
extern "C" int ssn_frames_crop_resize_normalize(const unsigned char* src, float* dst, int n_img, int Hs, int Ws, int C,
                                                int out_h, int out_w, const int* box, const int* flip, int roll,
                                                int invert_even, const float* mean, int n_mean, const float* stdv, int n_std,
                                                void* workspace, size_t workspace_bytes, hipStream_t stream) {
    SSN_CHECK_ARG(src && dst && box && flip && mean && stdv && workspace, "frames resize: null pointer");
    SSN_CHECK_ARG(n_img >= 0 && C >= 1 && out_h >= 1 && out_w >= 1 && n_mean >= 1 && n_std >= 1, "frames resize: bad arguments");
    if (workspace_bytes < ssn_frames_resize_workspace_bytes(n_img, out_h, out_w)) {
        ssn_set_error("frames resize: workspace too small");
        return SSN_ERR_WORKSPACE;
    }
    if (n_img == 0) return SSN_OK;
    int* tab = reinterpret_cast<int*>(workspace);
    const int nt = n_img * (out_w + out_h);
    hipLaunchKernelGGL(resize_coeffs_kernel, dim3((nt + 255) / 256), dim3(256), 0, stream, box, n_img, out_w, out_h, tab);
    const long total = (long)n_img * C * out_h * out_w;
    long blocks = (total + 256 * 4 - 1) / (256 * 4);
    if (blocks > 65535 * 4) blocks = 65535 * 4;
    hipLaunchKernelGGL(frames_resize_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, (const uint8_t*)src, dst, n_img, Hs,
                       Ws, C, out_h, out_w, box, flip, tab, roll, invert_even, mean, stdv, n_mean, n_std);
    SSN_CHECK_LAUNCH("frames_crop_resize_normalize");
    return SSN_OK;
}

// GroupScale of a batch of equally sized frames: Pillow's 8-bit BILINEAR resize of the whole frame, bit for bit (see above).
// src [n_img][Hs][Ws][C] uint8 -> dst [n_img][out_h][out_w][C] uint8, C = 1 or 3.  The documented limit is an in / out ratio of 6
// on the axis with the smaller ratio (the side GroupScale sets: the other side's length is truncated to an integer, so its ratio
// comes out a little larger); either axis must stay below the 13-tap capacity, ratio 6.5.  Two launches on `stream`, nothing else.
extern "C" size_t ssn_frames_scale_workspace_bytes(int out_h, int out_w) {
    if (out_h < 0 || out_w < 0) return 0;
    return ((size_t)out_h + (size_t)out_w) * SC_ENT * sizeof(int);
}
extern "C" int ssn_frames_scale(const unsigned char* src, unsigned char* dst, int n_img, int Hs, int Ws, int C, int out_h,
                                int out_w, void* workspace, size_t workspace_bytes, hipStream_t stream) {
    SSN_CHECK_ARG(src && dst && workspace, "frames scale: null pointer");
    SSN_CHECK_ARG(C == 1 || C == 3, "frames scale: %d channels (1 or 3)", C);
    SSN_CHECK_ARG(n_img >= 0 && n_img <= 65535 && Hs >= 1 && Ws >= 1 && out_h >= 1 && out_w >= 1 && out_h <= (1 << 19) &&
                      out_w <= (1 << 19) && Hs <= (1 << 19) && Ws <= (1 << 19),
                  "frames scale: bad arguments");
    SSN_CHECK_ARG((long)Hs <= 6L * out_h || (long)Ws <= 6L * out_w, "frames scale: %dx%d -> %dx%d shrinks by more than 6", Ws, Hs,
                  out_w, out_h);
    SSN_CHECK_ARG(2L * Hs < 13L * out_h && 2L * Ws < 13L * out_w, "frames scale: %dx%d -> %dx%d needs more than %d taps", Ws, Hs,
                  out_w, out_h, SC_MAXK);
    SSN_CHECK_ARG(((uintptr_t)workspace & 3) == 0, "frames scale: workspace not aligned");
    if (workspace_bytes < ssn_frames_scale_workspace_bytes(out_h, out_w)) {
        ssn_set_error("frames scale: workspace too small");
        return SSN_ERR_WORKSPACE;
    }
    if (n_img == 0) return SSN_OK;
    int* tab = reinterpret_cast<int*>(workspace);
    hipLaunchKernelGGL(scale_coeffs_kernel, dim3((out_w + out_h + 255) / 256), dim3(256), 0, stream, Ws, Hs, out_w, out_h, tab);
    const dim3 grid((out_w + SC_TW - 1) / SC_TW, (out_h + SC_TH - 1) / SC_TH, n_img);
    hipLaunchKernelGGL(frames_scale_kernel, grid, dim3(256), 0, stream, (const uint8_t*)src, (uint8_t*)dst, Hs, Ws, C, out_h, out_w,
                       (const int*)tab);
    SSN_CHECK_LAUNCH("frames_scale");
    return SSN_OK;
}
