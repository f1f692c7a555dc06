// TV-L1 optical flow for the Flow modality (the "Extract Frames and Optical Flow Images" stage of the reference's README, which
// it hands to dense_flow / OpenCV's CUDA OpticalFlowDual_TVL1).  The algorithm is the published one (Zach, Pock, Bischof 2007;
// Sanchez, Meinhardt-Llopis, Facciolo, IPOL 2013) in the restatement DESIGN.md section 3.9 fixes: fp32, no contraction, so that a
// pixel's arithmetic does not depend on the tile it falls in, on the number of iterations a launch advances, or on the batch.
//
//   ssn_flow_gray      RGB uint8 -> gray uint8, exact integer arithmetic
//   ssn_flow_resize    bilinear (align_corners = False) with a multiplier per plane; optionally picks each pair's source buffer
//   ssn_tvl1_warp      gradient of I1 + the three bilinear samples + grad + rho_c in one pass, starts a warp
//   ssn_tvl1_iterate   THE hot path: up to TVL1_HALO iterations per launch on LDS-resident tiles
//   ssn_flow_quantize  dense_flow's CAST to uint8
//
// Control without a host read.  Every pair has a record ctl[b] = {done, launches, iterations, 0} and the six state fields
// (u1, u2, p11, p12, p21, p22) live in TWO buffers: launch number `launches` of a pair reads buffer launches & 1 and writes the
// other one (a workgroup reads the halo its neighbours own, so it cannot update in place).  The record itself is double-buffered
// by the host: every launch reads ctl_in and workgroup 0 of the pair writes ctl_out, so no workgroup reads a word another one of the
// same launch writes.  The error of a chunk's last iteration goes to part_out[b][tile]; the first launch of the next chunk sums a
// pair's partials in tile order -- every workgroup does, and arrives at the same answer -- and a pair whose sum is below the
// threshold is done: its workgroups exit at once, in this launch and in every later one of the warp.
#include "ssn_common.h"

#pragma clang fp contract(off)

namespace {

constexpr int TVL1_R = 64;          // LDS region: TVL1_R x TVL1_R cells of the six state fields (96 KiB)
constexpr int TVL1_HALO = 10;       // iterations one launch may advance: the valid part of the region shrinks by a ring per iteration
constexpr int TVL1_T = TVL1_R - 2 * TVL1_HALO;      // interior a workgroup owns and stores: 44 x 44
constexpr int TVL1_CELLS = TVL1_R * TVL1_R / 256;   // cells per thread (16): column tid & 63, rows 4 k + (tid >> 6)

__global__ __launch_bounds__(256) void flow_gray_kernel(const unsigned char* rgb, unsigned char* gray, long n) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const unsigned r = rgb[3 * i], g = rgb[3 * i + 1], b = rgb[3 * i + 2];
    gray[i] = (unsigned char)((4899u * r + 9617u * g + 1868u * b + 8192u) >> 14);
}

__device__ __forceinline__ int imin(int a, int b) { return a < b ? a : b; }
__device__ __forceinline__ int imax(int a, int b) { return a > b ? a : b; }

// which of a pair's two state buffers holds its current fields
__device__ __forceinline__ int tvl1_current(const int* ctl, int b) { return ctl ? (ctl[4 * b + 1] & 1) : 0; }

// dst[b][c] = mul(c) * bilinear(src[b][c]); source coordinate (d + 0.5) * src / dst - 0.5, indices clamped
__global__ __launch_bounds__(256) void flow_resize_kernel(const float* src0, const float* src1, const int* ctl, float* dst, int C,
                                                          long src_bstride, long dst_bstride, int Hs, int Ws, int Hd, int Wd,
                                                          float mul_x, float mul_y) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    const int b = blockIdx.y;
    if (i >= (long)C * Hd * Wd) return;
    const int c = (int)(i / ((long)Hd * Wd));
    const int rem = (int)(i - (long)c * Hd * Wd);
    const int y = rem / Wd, x = rem - y * Wd;
    const float* s = (tvl1_current(ctl, b) ? src1 : src0) + b * src_bstride + (long)c * Hs * Ws;
    const float sx = fmaxf(((float)Ws / (float)Wd) * ((float)x + 0.5f) - 0.5f, 0.f);
    const float sy = fmaxf(((float)Hs / (float)Hd) * ((float)y + 0.5f) - 0.5f, 0.f);
    const int x0 = imin((int)sx, Ws - 1), y0 = imin((int)sy, Hs - 1);
    const int x1 = imin(x0 + 1, Ws - 1), y1 = imin(y0 + 1, Hs - 1);
    const float fx = sx - (float)x0, fy = sy - (float)y0;
    const float top = (1.f - fx) * s[(long)y0 * Ws + x0] + fx * s[(long)y0 * Ws + x1];
    const float bot = (1.f - fx) * s[(long)y1 * Ws + x0] + fx * s[(long)y1 * Ws + x1];
    const float v = (1.f - fy) * top + fy * bot;
    dst[b * dst_bstride + i] = v * ((c & 1) ? mul_y : mul_x);
}

__device__ __forceinline__ float tvl1_bilinear(float a00, float a01, float a10, float a11, float fx, float fy) {
    return (1.f - fy) * ((1.f - fx) * a00 + fx * a01) + fy * ((1.f - fx) * a10 + fx * a11);
}

// One thread per pixel.  Moves the pair's state to buffer 0 when the previous warp left it in buffer 1 (each thread its own
// pixel), samples I1 and its centred gradient (formed at the four corners) at (x + u1, y + u2), and writes the per-warp
// constants cst[b] = {gx, gy, grad, rho_c}.  The thread of pixel 0 starts the pair's record afresh.
__global__ __launch_bounds__(256) void tvl1_warp_kernel(const float* I0, const float* I1, float* state0, const float* state1, float* cst,
                                                        const int* ctl_in, int* ctl_out, int H, int W) {
    const int b = blockIdx.y;
    const long hw = (long)H * W;
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= hw) return;
    float* st = state0 + (long)b * 6 * hw;
    if (tvl1_current(ctl_in, b)) {
        const float* from = state1 + (long)b * 6 * hw;
        for (int f = 0; f < 6; ++f) st[f * hw + i] = from[f * hw + i];
    }
    if (i == 0) {
        ctl_out[4 * b] = 0;
        ctl_out[4 * b + 1] = 0;
        ctl_out[4 * b + 2] = 0;
        ctl_out[4 * b + 3] = 0;
    }
    const int y = (int)(i / W), x = (int)(i - (long)y * W);
    const float u1 = st[i], u2 = st[hw + i];
    const float cx = fminf(fmaxf((float)x + u1, 0.f), (float)(W - 1));
    const float cy = fminf(fmaxf((float)y + u2, 0.f), (float)(H - 1));
    const int x0 = imin((int)cx, W - 1), y0 = imin((int)cy, H - 1);
    const int x1 = imin(x0 + 1, W - 1), y1 = imin(y0 + 1, H - 1);
    const float fx = cx - (float)x0, fy = cy - (float)y0;
    const float* im = I1 + b * hw;
    float v[4], dx[4], dy[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int xx = (k & 1) ? x1 : x0, yy = (k & 2) ? y1 : y0;
        const long row = (long)yy * W;
        v[k] = im[row + xx];
        dx[k] = 0.5f * (im[row + imin(xx + 1, W - 1)] - im[row + imax(xx - 1, 0)]);
        dy[k] = 0.5f * (im[(long)imin(yy + 1, H - 1) * W + xx] - im[(long)imax(yy - 1, 0) * W + xx]);
    }
    const float i1w = tvl1_bilinear(v[0], v[1], v[2], v[3], fx, fy);
    const float gx = tvl1_bilinear(dx[0], dx[1], dx[2], dx[3], fx, fy);
    const float gy = tvl1_bilinear(dy[0], dy[1], dy[2], dy[3], fx, fy);
    float* c = cst + (long)b * 4 * hw;
    c[i] = gx;
    c[hw + i] = gy;
    c[2 * hw + i] = gx * gx + gy * gy;
    c[3 * hw + i] = ((i1w - gx * u1) - gy * u2) - I0[b * hw + i];
}

// The iterations.  Grid (tiles_x, tiles_y, B), 256 threads.  A workgroup stages the TVL1_T^2 interior it owns plus a halo of n_iter
// cells of the six state fields into LDS (the interior always at offset TVL1_HALO: which thread owns a cell, and with it the order
// of the error sum, does not depend on n_iter), keeps each thread's own cells and their four constants in registers, advances n_iter
// iterations (two barriers each) and stores its interior.  Every cell of the region is computed in every iteration; a cell whose
// neighbour lies outside the region sees zero there, which is wrong, and the wrong values advance one ring per iteration -- after
// n_iter <= halo iterations they have not reached the interior.  Cells outside the IMAGE are never read by cells inside it: the
// divergence takes p[-1] = 0 at column / row 0 and the forward difference is zero in the last column / row.
__global__ __launch_bounds__(256) void tvl1_iterate_kernel(float* state0, float* state1, const float* cst, int H, int W, int n_iter,
                                                           float l_t, float theta, float taut, float err_thresh, const int* ctl_in,
                                                           int* ctl_out, const float* part_in, float* part_out, int* iters) {
    __shared__ float s_f[6][TVL1_R * TVL1_R];
    __shared__ float s_wave[4];
    const int tid = threadIdx.x, b = blockIdx.z;
    const int ntiles = (int)(gridDim.x * gridDim.y), tile = (int)(blockIdx.y * gridDim.x + blockIdx.x);
    int done = ctl_in[4 * b];
    const int launches = ctl_in[4 * b + 1], iters_run = ctl_in[4 * b + 2];
    if (!done && part_in) {      // the previous chunk's error: the same sum, in tile order, in every workgroup of the pair
        float e = 0.f;
        for (int t = 0; t < ntiles; ++t) e += part_in[(long)b * ntiles + t];
        done = e < err_thresh;
    }
    if (tile == 0 && tid == 0) {
        ctl_out[4 * b] = done;
        ctl_out[4 * b + 1] = launches + (done ? 0 : 1);
        ctl_out[4 * b + 2] = iters_run + (done ? 0 : n_iter);
        ctl_out[4 * b + 3] = 0;
        if (!done) iters[b] = iters_run + n_iter;
    }
    if (done) return;      // (uniform over the workgroup)

    const long hw = (long)H * W;
    const float* src = ((launches & 1) ? state1 : state0) + (long)b * 6 * hw;
    float* dst = ((launches & 1) ? state0 : state1) + (long)b * 6 * hw;
    const float* cb = cst + (long)b * 4 * hw;
    const int lo = TVL1_HALO - n_iter, hi = TVL1_HALO + TVL1_T + n_iter;      // the part of the region this launch uses
    const int c = tid & 63, r0 = tid >> 6;
    const int gx_ = (int)blockIdx.x * TVL1_T - TVL1_HALO + c;
    const bool col_ok = c >= lo && c < hi && gx_ >= 0 && gx_ < W;
    const bool has_left = c > 0 && gx_ > 0, has_right = c < TVL1_R - 1 && gx_ < W - 1;
    const bool col_own = c >= TVL1_HALO && c < TVL1_HALO + TVL1_T;

    float kgx[TVL1_CELLS], kgy[TVL1_CELLS], kgrad[TVL1_CELLS], krho[TVL1_CELLS];
    float u1[TVL1_CELLS], u2[TVL1_CELLS], p11[TVL1_CELLS], p12[TVL1_CELLS], p21[TVL1_CELLS], p22[TVL1_CELLS];
#pragma unroll
    for (int k = 0; k < TVL1_CELLS; ++k) {
        const int r = 4 * k + r0, gy_ = (int)blockIdx.y * TVL1_T - TVL1_HALO + r;
        const bool live = col_ok && r >= lo && r < hi && gy_ >= 0 && gy_ < H;
        const long g = live ? (long)gy_ * W + gx_ : 0;
        kgx[k] = live ? cb[g] : 0.f;
        kgy[k] = live ? cb[hw + g] : 0.f;
        kgrad[k] = live ? cb[2 * hw + g] : 0.f;
        krho[k] = live ? cb[3 * hw + g] : 0.f;
        u1[k] = live ? src[g] : 0.f;
        u2[k] = live ? src[hw + g] : 0.f;
        p11[k] = live ? src[2 * hw + g] : 0.f;
        p12[k] = live ? src[3 * hw + g] : 0.f;
        p21[k] = live ? src[4 * hw + g] : 0.f;
        p22[k] = live ? src[5 * hw + g] : 0.f;
        const int cell = r * TVL1_R + c;
        s_f[2][cell] = p11[k];
        s_f[3][cell] = p12[k];
        s_f[4][cell] = p21[k];
        s_f[5][cell] = p22[k];
    }
    __syncthreads();

    float err = 0.f;
    for (int it = 0; it < n_iter; ++it) {
        const bool last = it == n_iter - 1;
#pragma unroll
        for (int k = 0; k < TVL1_CELLS; ++k) {
            const int r = 4 * k + r0, gy_ = (int)blockIdx.y * TVL1_T - TVL1_HALO + r;
            const bool live = col_ok && r >= lo && r < hi && gy_ >= 0 && gy_ < H;
            const int cell = r * TVL1_R + c;
            float n1 = 0.f, n2 = 0.f;
            if (live) {
                const float gx = kgx[k], gy = kgy[k], grad = kgrad[k];
                const float rho = (krho[k] + gx * u1[k]) + gy * u2[k];
                const float thr = l_t * grad;
                float d1 = 0.f, d2 = 0.f;
                if (rho < -thr) {
                    d1 = l_t * gx;
                    d2 = l_t * gy;
                } else if (rho > thr) {
                    d1 = -l_t * gx;
                    d2 = -l_t * gy;
                } else if (grad > 1e-9f) {
                    const float fi = -rho / grad;
                    d1 = fi * gx;
                    d2 = fi * gy;
                }
                const bool has_up = r > 0 && gy_ > 0;
                const float l11 = has_left ? s_f[2][cell - 1] : 0.f, t12 = has_up ? s_f[3][cell - TVL1_R] : 0.f;
                const float l21 = has_left ? s_f[4][cell - 1] : 0.f, t22 = has_up ? s_f[5][cell - TVL1_R] : 0.f;
                const float div1 = (p11[k] - l11) + (p12[k] - t12);
                const float div2 = (p21[k] - l21) + (p22[k] - t22);
                n1 = (u1[k] + d1) + theta * div1;
                n2 = (u2[k] + d2) + theta * div2;
                if (last && part_out && col_own && r >= TVL1_HALO && r < TVL1_HALO + TVL1_T) {
                    const float e1 = n1 - u1[k], e2 = n2 - u2[k];
                    err += e1 * e1 + e2 * e2;
                }
            }
            u1[k] = n1;
            u2[k] = n2;
            s_f[0][cell] = n1;
            s_f[1][cell] = n2;
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < TVL1_CELLS; ++k) {
            const int r = 4 * k + r0, gy_ = (int)blockIdx.y * TVL1_T - TVL1_HALO + r;
            const bool live = col_ok && r >= lo && r < hi && gy_ >= 0 && gy_ < H;
            const int cell = r * TVL1_R + c;
            if (live) {
                const bool has_down = r < TVL1_R - 1 && gy_ < H - 1;
                const float u1x = has_right ? s_f[0][cell + 1] - u1[k] : 0.f;
                const float u1y = has_down ? s_f[0][cell + TVL1_R] - u1[k] : 0.f;
                const float u2x = has_right ? s_f[1][cell + 1] - u2[k] : 0.f;
                const float u2y = has_down ? s_f[1][cell + TVL1_R] - u2[k] : 0.f;
                const float q1 = 1.f + taut * sqrtf(u1x * u1x + u1y * u1y);
                const float q2 = 1.f + taut * sqrtf(u2x * u2x + u2y * u2y);
                p11[k] = (p11[k] + taut * u1x) / q1;
                p12[k] = (p12[k] + taut * u1y) / q1;
                p21[k] = (p21[k] + taut * u2x) / q2;
                p22[k] = (p22[k] + taut * u2y) / q2;
            }
            s_f[2][cell] = p11[k];
            s_f[3][cell] = p12[k];
            s_f[4][cell] = p21[k];
            s_f[5][cell] = p22[k];
        }
        __syncthreads();
    }

#pragma unroll
    for (int k = 0; k < TVL1_CELLS; ++k) {
        const int r = 4 * k + r0, gy_ = (int)blockIdx.y * TVL1_T - TVL1_HALO + r;
        if (col_own && col_ok && r >= TVL1_HALO && r < TVL1_HALO + TVL1_T && gy_ < H) {      // (gy_ >= 0: r >= halo)
            const long g = (long)gy_ * W + gx_;
            dst[g] = u1[k];
            dst[hw + g] = u2[k];
            dst[2 * hw + g] = p11[k];
            dst[3 * hw + g] = p12[k];
            dst[4 * hw + g] = p21[k];
            dst[5 * hw + g] = p22[k];
        }
    }
    if (part_out) {      // fixed order: a thread's cells by k, the lanes in a butterfly, the four waves one after the other
        const float wv = wave_sum(err);
        if ((tid & 63) == 0) s_wave[tid >> 6] = wv;
        __syncthreads();
        if (tid == 0) part_out[(long)b * ntiles + tile] = ((s_wave[0] + s_wave[1]) + s_wave[2]) + s_wave[3];
    }
}

__global__ __launch_bounds__(256) void flow_quantize_kernel(const float* flow, unsigned char* out, long n, float bound) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float v = flow[i];
    unsigned char q;
    if (v > bound) {
        q = 255;
    } else if (v < -bound) {
        q = 0;
    } else {
        const float r = rintf(255.0f * (v + bound) / (2.f * bound));      // half to even: cvRound
        q = (r >= 0.f && r <= 255.f) ? (unsigned char)(int)r : (unsigned char)0;
    }
    out[i] = q;
}

}  // namespace

// interior (th x tw) a workgroup of ssn_tvl1_iterate owns, and the halo = the most iterations one launch advances
extern "C" int ssn_tvl1_tile_shape(int* th, int* tw, int* halo) {
    if (th) *th = TVL1_T;
    if (tw) *tw = TVL1_T;
    if (halo) *halo = TVL1_HALO;
    return SSN_OK;
}

extern "C" int ssn_flow_gray(const unsigned char* rgb, unsigned char* gray, long pixels, hipStream_t stream) {
    SSN_CHECK_ARG(pixels >= 0 && pixels < (1L << 38), "flow_gray: bad size");
    if (pixels == 0) return SSN_OK;
    SSN_CHECK_ARG(rgb && gray, "flow_gray: null pointer");
    hipLaunchKernelGGL(flow_gray_kernel, dim3((unsigned)((pixels + 255) / 256)), dim3(256), 0, stream, rgb, gray, pixels);
    SSN_CHECK_LAUNCH("flow_gray");
    return SSN_OK;
}

extern "C" int ssn_flow_resize(const float* src0, const float* src1, const int* ctl, float* dst, int B, int C, long src_bstride,
                               long dst_bstride, int Hs, int Ws, int Hd, int Wd, float mul_x, float mul_y, hipStream_t stream) {
    SSN_CHECK_ARG(B >= 1 && B <= 65535 && C >= 1 && Hs >= 1 && Ws >= 1 && Hd >= 1 && Wd >= 1, "flow_resize: bad sizes");
    SSN_CHECK_ARG((long)C * Hs * Ws < (1L << 31) && (long)C * Hd * Wd < (1L << 31), "flow_resize: image too large");
    SSN_CHECK_ARG(src_bstride >= (long)C * Hs * Ws && dst_bstride >= (long)C * Hd * Wd, "flow_resize: batch stride below the planes");
    SSN_CHECK_ARG(src0 && dst, "flow_resize: null pointer");
    SSN_CHECK_ARG(!ctl || src1, "flow_resize: a control record needs both source buffers");
    const long n = (long)C * Hd * Wd;
    hipLaunchKernelGGL(flow_resize_kernel, dim3((unsigned)((n + 255) / 256), (unsigned)B), dim3(256), 0, stream, src0, src1, ctl, dst, C,
                       src_bstride, dst_bstride, Hs, Ws, Hd, Wd, mul_x, mul_y);
    SSN_CHECK_LAUNCH("flow_resize");
    return SSN_OK;
}

// I0, I1 [B][H][W]; state0 / state1 [B][6][H][W] (u1, u2, p11, p12, p21, p22); cst [B][4][H][W]; ctl_in [B][4] or NULL (the
// state is in buffer 0: first warp of a level), ctl_out [B][4].
extern "C" int ssn_tvl1_warp(const float* I0, const float* I1, float* state0, const float* state1, float* cst, const int* ctl_in,
                             int* ctl_out, int B, int H, int W, hipStream_t stream) {
    SSN_CHECK_ARG(B >= 1 && B <= 65535 && H >= 1 && W >= 1 && (long)H * W < (1L << 28), "tvl1_warp: bad sizes");
    SSN_CHECK_ARG(I0 && I1 && state0 && state1 && cst && ctl_out, "tvl1_warp: null pointer");
    SSN_CHECK_ARG(ctl_in != ctl_out, "tvl1_warp: the control record is read and written in different slots");
    const long n = (long)H * W;
    hipLaunchKernelGGL(tvl1_warp_kernel, dim3((unsigned)((n + 255) / 256), (unsigned)B), dim3(256), 0, stream, I0, I1, state0, state1, cst,
                       ctl_in, ctl_out, H, W);
    SSN_CHECK_LAUNCH("tvl1_warp");
    return SSN_OK;
}

// n_iter iterations (1 .. halo) of every pair that is not done.  part_in [B][tiles] or NULL: the error partials of the chunk that
// ended with the previous launch, tested against err_thresh; part_out [B][tiles] or NULL: this launch ends a chunk.  iters [B]:
// the warp's iteration count, kept up to date.  tiles = ceil(H / th) * ceil(W / tw).
extern "C" int ssn_tvl1_iterate(float* state0, float* state1, const float* cst, int B, int H, int W, int n_iter, float l_t, float theta,
                                float taut, float err_thresh, const int* ctl_in, int* ctl_out, const float* part_in, float* part_out,
                                int* iters, hipStream_t stream) {
    SSN_CHECK_ARG(B >= 1 && B <= 65535 && H >= 1 && W >= 1 && (long)H * W < (1L << 28), "tvl1_iterate: bad sizes");
    SSN_CHECK_ARG(n_iter >= 1 && n_iter <= TVL1_HALO, "tvl1_iterate: %d iterations per launch, the halo allows 1..%d", n_iter, TVL1_HALO);
    SSN_CHECK_ARG(state0 && state1 && cst && ctl_in && ctl_out && iters, "tvl1_iterate: null pointer");
    SSN_CHECK_ARG(state0 != state1 && ctl_in != ctl_out && (!part_in || part_in != part_out),
                  "tvl1_iterate: state, control record and partials are read and written in different buffers");
    const unsigned tx = (unsigned)((W + TVL1_T - 1) / TVL1_T), ty = (unsigned)((H + TVL1_T - 1) / TVL1_T);
    SSN_CHECK_ARG(ty <= 65535, "tvl1_iterate: image too tall");
    hipLaunchKernelGGL(tvl1_iterate_kernel, dim3(tx, ty, (unsigned)B), dim3(256), 0, stream, state0, state1, cst, H, W, n_iter, l_t, theta,
                       taut, err_thresh, ctl_in, ctl_out, part_in, part_out, iters);
    SSN_CHECK_LAUNCH("tvl1_iterate");
    return SSN_OK;
}

extern "C" int ssn_flow_quantize(const float* flow, unsigned char* out, long n, float bound, hipStream_t stream) {
    SSN_CHECK_ARG(n >= 0 && n < (1L << 38) && bound > 0.f, "flow_quantize: bad size or bound");
    if (n == 0) return SSN_OK;
    SSN_CHECK_ARG(flow && out, "flow_quantize: null pointer");
    hipLaunchKernelGGL(flow_quantize_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, flow, out, n, bound);
    SSN_CHECK_LAUNCH("flow_quantize");
    return SSN_OK;
}
