// The fused clip + Adam update on one flat fp32 buffer for gfx950: the squared gradient norm (sep_sqnorm), then clip_grad_norm_ and Adam.step in
// one elementwise pass (sep_adam_step; sep_adam_step_dev is its graph-replayable form).
//
// Reference arithmetic replaced (paths under the reference's root): egs/wsj0-mix/common/src/driver.py:152-155 (clip_grad_norm_ + Adam.step).
//
// Called by sepkernels/train.py (FusedTrainStep: the eager step and the captured one).
#include "common.hpp"

namespace {

// ---- clip + Adam on a flat fp32 buffer ----------------------------------------------------------
__global__ __launch_bounds__(256) void sqnorm_kernel(const float* __restrict__ g, double* __restrict__ out, int64_t n) {
    __shared__ double red[4];
    double acc = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * 1024 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 1024) {
        float s = 0.f;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int64_t idx = i + k * 256;
            if (idx < n) { const float v = g[idx]; s = fmaf(v, v, s); }
        }
        acc += (double)s;
    }
    const double r = block_sum_256<double>(acc, red);
    if (threadIdx.x == 0) atomicAdd(out, r);
}

__global__ __launch_bounds__(256) void adam_kernel(float* __restrict__ p, float* __restrict__ g, float* __restrict__ m,
                                                   float* __restrict__ v, const double* __restrict__ sqnorm, int64_t n,
                                                   float lr, float b1, float b2, float eps, float wd, float max_norm,
                                                   float grad_scale, float bc1, float bc2s) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    float coef = grad_scale;
    if (max_norm > 0.f) {
        const float total = grad_scale * (float)sqrt(sqnorm[0]);
        const float c = max_norm / (total + 1e-6f);
        coef *= (c < 1.f ? c : 1.f);
    }
    float gi = g[i] * coef;
    g[i] = gi;                       // clip_grad_norm_ rescales .grad in place
    const float pi = p[i];
    if (wd != 0.f) gi = fmaf(wd, pi, gi);
    const float mi = b1 * m[i] + (1.f - b1) * gi;
    const float vi = b2 * v[i] + (1.f - b2) * gi * gi;
    m[i] = mi; v[i] = vi;
    const float denom = sqrtf(vi) / bc2s + eps;
    p[i] = pi - (lr / bc1) * (mi / denom);
}

// Graph-replayable form: the step count and the learning rate live in device memory (a captured launch freezes its kernel
// arguments), the count is advanced by a one-thread kernel in front of this one.
__global__ void adam_tick_kernel(int* step) { step[0] += 1; }

__global__ __launch_bounds__(256) void adam_dev_kernel(float* __restrict__ p, float* __restrict__ g, float* __restrict__ m,
                                                       float* __restrict__ v, const double* __restrict__ sqnorm, int64_t n,
                                                       const float* __restrict__ lr_dev, const int* __restrict__ step_dev, float b1, float b2,
                                                       float eps, float wd, float max_norm, float grad_scale) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float lr = lr_dev[0];
    const float st = (float)step_dev[0];
    const float bc1 = 1.f - powf(b1, st);
    const float bc2s = sqrtf(1.f - powf(b2, st));
    float coef = grad_scale;
    if (max_norm > 0.f) {
        const float total = grad_scale * (float)sqrt(sqnorm[0]);
        const float c = max_norm / (total + 1e-6f);
        coef *= (c < 1.f ? c : 1.f);
    }
    float gi = g[i] * coef;
    g[i] = gi;
    const float pi = p[i];
    if (wd != 0.f) gi = fmaf(wd, pi, gi);
    const float mi = b1 * m[i] + (1.f - b1) * gi;
    const float vi = b2 * v[i] + (1.f - b2) * gi * gi;
    m[i] = mi; v[i] = vi;
    const float denom = sqrtf(vi) / bc2s + eps;
    p[i] = pi - (lr / bc1) * (mi / denom);
}

}  // namespace

extern "C" int sep_sqnorm(const float* g, double* sqnorm, int64_t n, sep_stream_t stream) {
    SEP_REQUIRE(g && sqnorm && n > 0, "sep_sqnorm: bad arguments");
    int64_t blocks = (n + 1023) / 1024;
    if (blocks > 256) blocks = 256;      // one fp64 atomic per workgroup on ONE address: 2048 of them serialised into ~30 us (profiles/r08a: 33 us for 20 MB)
    hipLaunchKernelGGL(sqnorm_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, g, sqnorm, n);
    SEP_CHECK_LAUNCH("sep_sqnorm");
    return 0;
}

extern "C" int sep_adam_step(float* p, float* g, float* m, float* v, const double* sqnorm, int64_t n, float lr, float beta1,
                             float beta2, float eps, float weight_decay, float max_norm, float grad_scale, int step,
                             sep_stream_t stream) {
    SEP_REQUIRE(p && g && m && v && n > 0 && step >= 1, "sep_adam_step: bad arguments");
    SEP_REQUIRE(max_norm <= 0.f || sqnorm, "sep_adam_step: clipping needs sqnorm");
    const float bc1 = 1.f - powf(beta1, (float)step);
    const float bc2s = sqrtf(1.f - powf(beta2, (float)step));
    hipLaunchKernelGGL(adam_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, p, g, m, v, sqnorm, n, lr, beta1, beta2, eps, weight_decay, max_norm, grad_scale, bc1, bc2s);
    SEP_CHECK_LAUNCH("sep_adam_step");
    return 0;
}

extern "C" int sep_adam_step_dev(float* p, float* g, float* m, float* v, const double* sqnorm, int64_t n, const float* lr_dev,
                                 int32_t* step_dev, float beta1, float beta2, float eps, float weight_decay, float max_norm,
                                 float grad_scale, sep_stream_t stream) {
    SEP_REQUIRE(p && g && m && v && n > 0 && lr_dev && step_dev, "sep_adam_step_dev: bad arguments");
    SEP_REQUIRE(max_norm <= 0.f || sqnorm, "sep_adam_step_dev: clipping needs sqnorm");
    hipLaunchKernelGGL(adam_tick_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, step_dev);
    hipLaunchKernelGGL(adam_dev_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, p, g, m, v, sqnorm, n, lr_dev, step_dev,
                       beta1, beta2, eps, weight_decay, max_norm, grad_scale);
    SEP_CHECK_LAUNCH("sep_adam_step_dev");
    return 0;
}
