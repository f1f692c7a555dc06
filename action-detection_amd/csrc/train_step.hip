// Per-step bookkeeping of the training loops (/root/reference/ssn_train.py:216-253, binary_train.py:180-204) on the device, in a
// constant number of launches and without a host read, so that the whole step -- meters, clipping, optimizer -- can be captured
// into a hipGraph:
//   ssn_step_meters          AverageMeter.update of every loss / accuracy meter, one launch
//   ssn_sumsq_multi          clip_grad_norm's total norm and the gradient scale it implies, ceil(count / 48) + 1 launches
//   ssn_sgd_step_multi_dev   ssn_sgd_step_multi with that scale read from device memory
// No atomics anywhere: every sum has a fixed order, two calls on the same data give the same bits.
#include "ssn_common.h"

namespace {

// launches issued by the entry points of this file on the calling thread (ssn_train_step_launches)
thread_local long g_launches = 0;

// ---------------------------------------------------------------------------------------------------------------- meters
constexpr int METER_MAX_LOSSES = 4;

// One workgroup.  A thread owns rows tid, tid + 256, ...; the prediction of a row is its largest value, the lowest column among
// equals, NaN above every number and the first NaN taken (what torch.topk(1) returns on the CPU).  state: per meter
// {sum, count, last_num, last_den}, then the count of skipped calls.
__global__ __launch_bounds__(256) void step_meters_kernel(const float* logits, long row_stride, const long* target, int rows,
                                                          int cols, const float* losses, int n_losses, double loss_weight,
                                                          float pct_all, float pct_half, double* state, const int* skip) {
    const int n_meters = n_losses + 3;
    if (skip && *skip) {       // (block-uniform) a flagged step is redone: count it, change nothing else
        if (threadIdx.x == 0) state[4 * n_meters] += 1.0;
        return;
    }
    int hit_even = 0, hit_odd = 0;
    for (int r = threadIdx.x; r < rows; r += 256) {
        const float* row = logits + (long)r * row_stride;
        float best = row[0];
        int arg = 0;
        for (int c = 1; c < cols; ++c) {
            const float v = row[c];
            if (best != best) break;                       // the first NaN stays
            if (v != v || v > best) {
                best = v;
                arg = c;
            }
        }
        const long t = target[r];
        const int hit = (t >= 0 && t < cols && t == (long)arg) ? 1 : 0;
        if (r & 1) hit_odd += hit; else hit_even += hit;
    }
    __shared__ int red[4][2];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        hit_even += __shfl_xor(hit_even, off, 64);
        hit_odd += __shfl_xor(hit_odd, off, 64);
    }
    if ((threadIdx.x & 63) == 0) {
        red[threadIdx.x >> 6][0] = hit_even;
        red[threadIdx.x >> 6][1] = hit_odd;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    const int even = red[0][0] + red[1][0] + red[2][0] + red[3][0];
    const int odd = red[0][1] + red[1][1] + red[2][1] + red[3][1];
    for (int m = 0; m < n_meters; ++m) {
        double val, n;
        if (m < n_losses) {
            val = (double)losses[m];
            n = loss_weight;
        } else if (m == n_losses) {
            // accuracy(): correct_k.mul_(100.0 / batch_size) on a float tensor, then .item()
            val = (double)((float)(even + odd) * pct_all);
            n = (double)rows;
        } else {
            val = (double)((float)(m == n_losses + 1 ? even : odd) * pct_half);
            n = (double)(rows / 2);
        }
        const double num = val * n;
        double* s = state + 4 * m;
        s[0] += num;
        s[1] += n;
        s[2] = num;
        s[3] = n;
    }
}

// ------------------------------------------------------------------------------------------------------- multi-tensor norm
constexpr int MT_MAX = 48;
constexpr int MT_CHUNK = 4096;
struct SumsqTable {
    const float* x[MT_MAX];
    long n[MT_MAX];
    int blk0[MT_MAX + 1];   // first block of tensor t inside this launch (MT_CHUNK elements per block)
    int count;
};
// One fp32 partial per MT_CHUNK-element block, to the fixed slot slot0 + blockIdx.x.  A value passes 16 roundings in its thread
// (fused multiply-adds), 6 in the wave butterfly and 2 in the sum of the four waves.  Dword loads: the tensors may be views at
// any element offset of a flat buffer.
__global__ __launch_bounds__(256) void sumsq_multi_kernel(SumsqTable t, float* partial, long slot0) {
    int ti = 0;
    while (ti + 1 < t.count && (int)blockIdx.x >= t.blk0[ti + 1]) ++ti;   // block-uniform linear search
    const long base = (long)((int)blockIdx.x - t.blk0[ti]) * MT_CHUNK;
    const float* x = t.x[ti];
    long end = base + MT_CHUNK;
    if (end > t.n[ti]) end = t.n[ti];
    float s = 0.f;
    for (long i = base + threadIdx.x; i < end; i += 256) {
        const float v = x[i];
        s = fmaf(v, v, s);
    }
    s = wave_sum(s);
    __shared__ float red[4];
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) partial[slot0 + blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}
// Single workgroup: thread t adds the partials t, t + 256, ... in index order in double, a fixed tree over LDS joins the 256
// sums.  out[0] = sqrt(sum) * pre_scale, out[1] = the factor the update has to apply to the gradients
// (ssn_train.py:239-248: grad / iter_size, then clip_coef = max_norm / (total_norm + 1e-6) applied when it is below 1).
__global__ __launch_bounds__(256) void sumsq_final_kernel(const float* partial, long nb, float pre_scale, float max_norm,
                                                          float* out) {
    __shared__ double acc[256];
    double s = 0.0;
    for (long i = threadIdx.x; i < nb; i += 256) s += (double)partial[i];
    acc[threadIdx.x] = s;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) acc[threadIdx.x] += acc[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x != 0) return;
    const float norm = (float)sqrt(acc[0]) * pre_scale;
    float scale = pre_scale;
    if (max_norm > 0.f) {
        const double c = (double)max_norm / ((double)norm + 1e-6);
        if (c < 1.0) scale = (float)((double)pre_scale * c);      // (a NaN norm compares false: gradients stay unscaled)
    }
    out[0] = norm;
    out[1] = scale;
}

// ------------------------------------------------------------------------------------------ SGD, gradient scale from the device
// The table and the body of sgd_multi_kernel (elementwise.hip); only the origin of grad_scale differs.
struct SgdTable {
    float* w[MT_MAX];
    const float* g[MT_MAX];
    float* buf[MT_MAX];
    int blk0[MT_MAX + 1];
    long n[MT_MAX];
    float lr[MT_MAX], wd[MT_MAX];
    int count;
};
__global__ __launch_bounds__(256) void sgd_multi_dev_kernel(SgdTable t, float momentum, const float* grad_scale_dev,
                                                            int first_step, const int* skip) {
    if (skip && *skip) return;
    const float grad_scale = grad_scale_dev[0];
    int ti = 0;
    while (ti + 1 < t.count && (int)blockIdx.x >= t.blk0[ti + 1]) ++ti;
    const long base = (long)((int)blockIdx.x - t.blk0[ti]) * MT_CHUNK;
    float* w = t.w[ti];
    const float* g = t.g[ti];
    float* buf = t.buf[ti];
    const float lr = t.lr[ti], wd = t.wd[ti];
    long end = base + MT_CHUNK;
    if (end > t.n[ti]) end = t.n[ti];
    for (long i = base + threadIdx.x; i < end; i += 256) {
        const float gg = g[i] * grad_scale + wd * w[i];
        const float b = first_step ? gg : momentum * buf[i] + gg;
        buf[i] = b;
        w[i] = w[i] - lr * b;
    }
}

}  // namespace

extern "C" long ssn_train_step_launches(int reset) {
    const long n = g_launches;
    if (reset) g_launches = 0;
    return n;
}

extern "C" int ssn_step_meters(const float* logits, long row_stride, const long* target, int rows, int cols,
                               const float* losses, int n_losses, double loss_weight, double* state, const int* skip_flag,
                               hipStream_t stream) {
    SSN_CHECK_ARG(logits && target && state, "step_meters: null pointer");
    SSN_CHECK_ARG(n_losses >= 0 && n_losses <= METER_MAX_LOSSES && (n_losses == 0 || losses), "step_meters: bad losses");
    SSN_CHECK_ARG(rows >= 2 && rows % 2 == 0, "step_meters: rows must be even and positive (FG / BG pairs)");
    SSN_CHECK_ARG(cols >= 1 && row_stride >= cols, "step_meters: bad row shape");
    const float pct_all = (float)(100.0 / rows), pct_half = (float)(100.0 / (rows / 2));
    hipLaunchKernelGGL(step_meters_kernel, dim3(1), dim3(256), 0, stream, logits, row_stride, target, rows, cols, losses,
                       n_losses, loss_weight, pct_all, pct_half, state, skip_flag);
    ++g_launches;
    SSN_CHECK_LAUNCH("step_meters");
    return SSN_OK;
}

extern "C" long ssn_sumsq_multi_workspace_floats(int count, const long* n) {
    long blocks = 0;
    for (int i = 0; i < count; ++i) blocks += (n[i] + MT_CHUNK - 1) / MT_CHUNK;
    return blocks > 0 ? blocks : 1;
}

extern "C" int ssn_sumsq_multi(int count, const float* const* x, const long* n, float* workspace, long ws_floats,
                               float pre_scale, float max_norm, float* out, hipStream_t stream) {
    SSN_CHECK_ARG(count >= 0 && (count == 0 || (x && n)) && workspace && out, "sumsq_multi: null pointer");
    long need = 0;
    for (int i = 0; i < count; ++i) {
        SSN_CHECK_ARG(n[i] >= 0 && (n[i] == 0 || x[i]), "sumsq_multi: bad tensor %d", i);
        need += (n[i] + MT_CHUNK - 1) / MT_CHUNK;
    }
    if (need > ws_floats) {
        ssn_set_error("sumsq_multi: workspace %ld < %ld floats", ws_floats, need);
        return SSN_ERR_WORKSPACE;
    }
    long slot0 = 0;
    for (int base = 0; base < count; base += MT_MAX) {
        SumsqTable t;
        t.count = count - base < MT_MAX ? count - base : MT_MAX;
        int blocks = 0;
        for (int i = 0; i < t.count; ++i) {
            t.x[i] = x[base + i];
            t.n[i] = n[base + i];
            t.blk0[i] = blocks;
            blocks += (int)((n[base + i] + MT_CHUNK - 1) / MT_CHUNK);
        }
        t.blk0[t.count] = blocks;
        if (blocks == 0) continue;
        hipLaunchKernelGGL(sumsq_multi_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, t, workspace, slot0);
        ++g_launches;
        slot0 += blocks;
    }
    hipLaunchKernelGGL(sumsq_final_kernel, dim3(1), dim3(256), 0, stream, (const float*)workspace, slot0, pre_scale, max_norm,
                       out);
    ++g_launches;
    SSN_CHECK_LAUNCH("sumsq_multi");
    return SSN_OK;
}

extern "C" int ssn_sgd_step_multi_dev(int count, float* const* w, const float* const* grad, float* const* momentum_buf,
                                      const long* n, const float* lr, const float* weight_decay, float momentum,
                                      const float* grad_scale_dev, int first_step, const int* skip_flag, hipStream_t stream) {
    SSN_CHECK_ARG(count >= 0 && (count == 0 || (w && grad && momentum_buf && n && lr && weight_decay)) && grad_scale_dev,
                  "sgd_step_multi_dev: bad arguments");
    for (int base = 0; base < count; base += MT_MAX) {
        SgdTable t;
        t.count = count - base < MT_MAX ? count - base : MT_MAX;
        int blocks = 0;
        for (int i = 0; i < t.count; ++i) {
            t.w[i] = w[base + i];
            t.g[i] = grad[base + i];
            t.buf[i] = momentum_buf[base + i];
            t.n[i] = n[base + i];
            t.lr[i] = lr[base + i];
            t.wd[i] = weight_decay[base + i];
            t.blk0[i] = blocks;
            blocks += (int)((n[base + i] + MT_CHUNK - 1) / MT_CHUNK);
        }
        t.blk0[t.count] = blocks;
        if (blocks == 0) continue;
        hipLaunchKernelGGL(sgd_multi_dev_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, t, momentum, grad_scale_dev,
                           first_step, skip_flag);
        ++g_launches;
    }
    SSN_CHECK_LAUNCH("sgd_step_multi_dev");
    return SSN_OK;
}
