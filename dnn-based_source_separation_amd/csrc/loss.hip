// SI-SDR / PIT / Sinkhorn-PIT and the fused clip+Adam update for gfx950.
//
// Reference arithmetic replaced (under /root/reference/src): criterion/sdr.py:122-139 (sisdr),
// criterion/pit.py:9-44 (pit: loop over n! permutations), criterion/pit.py:163-193 (sinkpit);
// egs/wsj0-mix/common/src/driver.py:152-155 (clip_grad_norm_ + Adam.step).
//
// The O(T) work is two kernels: one pass producing the three dot products per (est_i, tgt_j) pair in
// fp64 (wavefront shuffles + one fp64 atomic per block), and one elementwise pass applying the analytic
// gradient  d_est_i = sum_j gw_ij * (cT_ij * tgt_j + cE_ij * est_i).  Everything in between (n x n
// matrices, n! search, Sinkhorn iterations) is O(n^2) per utterance and runs in tiny kernels.
#include "common.hpp"

namespace {

constexpr int DOT_CHUNK = 256 * 16;

// grid: (nchunk, npairs, B); pair p -> (i, j) = all_pairs ? (p / n, p % n) : (p, p)
__global__ __launch_bounds__(256) void sisdr_dots_kernel(const float* __restrict__ est, const float* __restrict__ tgt,
                                                         double* __restrict__ dots, double* __restrict__ tt,
                                                         double* __restrict__ xx, int n, int T, int all_pairs) {
    __shared__ double red[4];
    const int b = blockIdx.z, p = blockIdx.y;
    const int i = all_pairs ? p / n : p, j = all_pairs ? p % n : p;
    const float* e = est + ((size_t)b * n + i) * T;
    const float* t = tgt + ((size_t)b * n + j) * T;
    const bool do_tt = all_pairs ? (i == 0) : true;
    const bool do_xx = all_pairs ? (j == 0) : true;
    const int beg = blockIdx.x * DOT_CHUNK;
    float s_et = 0.f, s_tt = 0.f, s_xx = 0.f;
    double d_et = 0.0, d_tt = 0.0, d_xx = 0.0;
#pragma unroll 4
    for (int k = 0; k < 16; ++k) {
        const int idx = beg + k * 256 + threadIdx.x;
        if (idx < T) {
            const float ev = e[idx], tv = t[idx];
            s_et = fmaf(ev, tv, s_et); s_tt = fmaf(tv, tv, s_tt); s_xx = fmaf(ev, ev, s_xx);
        }
        if ((k & 3) == 3) {   // short fp32 runs, fp64 across them
            d_et += (double)s_et; d_tt += (double)s_tt; d_xx += (double)s_xx;
            s_et = s_tt = s_xx = 0.f;
        }
    }
    const double r_et = block_sum_256<double>(d_et, red);
    const double r_tt = block_sum_256<double>(d_tt, red);
    const double r_xx = block_sum_256<double>(d_xx, red);
    if (threadIdx.x == 0) {
        atomicAdd(dots + ((size_t)b * n + i) * n + j, r_et);
        if (do_tt) atomicAdd(tt + (size_t)b * n + j, r_tt);
        if (do_xx) atomicAdd(xx + (size_t)b * n + i, r_xx);
    }
}

struct SdrTerms { double alpha, c, S, Nn; };
__device__ __forceinline__ SdrTerms sdr_terms(double a, double ttv, double xxv, double eps) {
    SdrTerms r;
    r.c = ttv + eps;
    r.alpha = a / r.c;
    r.S = r.alpha * r.alpha * ttv + eps;
    double nn = r.alpha * r.alpha * ttv - 2.0 * r.alpha * a + xxv;   // |alpha t - x|^2
    if (nn < 0.0) nn = 0.0;
    r.Nn = nn + eps;
    return r;
}

__global__ void sisdr_from_dots_kernel(const double* __restrict__ dots, const double* __restrict__ tt,
                                       const double* __restrict__ xx, float* __restrict__ out, int B, int n,
                                       int all_pairs, float eps) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= B * n * n) return;
    const int b = idx / (n * n), i = (idx / n) % n, j = idx % n;
    if (!all_pairs && i != j) { out[idx] = 0.f; return; }
    const SdrTerms r = sdr_terms(dots[idx], tt[b * n + j], xx[b * n + i], (double)eps);
    out[idx] = (float)(10.0 * log10(r.S / r.Nn));
}

// grid: (ceil(T/1024), n, B); block 256 threads x 4 elements
__global__ __launch_bounds__(256) void sisdr_bwd_kernel(const float* __restrict__ est, const float* __restrict__ tgt,
                                                        const double* __restrict__ dots, const double* __restrict__ tt,
                                                        const double* __restrict__ xx, const float* __restrict__ gw,
                                                        float* __restrict__ d_est, int n, int T, int all_pairs, float eps) {
    __shared__ float cT[64];
    __shared__ float cE;
    const int b = blockIdx.z, i = blockIdx.y;
    if (threadIdx.x < 64) cT[threadIdx.x] = 0.f;
    __syncthreads();
    if (threadIdx.x == 0) {
        const double K = 10.0 / log(10.0);
        double ce = 0.0;
        for (int j = 0; j < n; ++j) {
            if (!all_pairs && j != i) continue;
            const double g = (double)gw[((size_t)b * n + i) * n + j];
            if (g == 0.0) continue;
            const double a = dots[((size_t)b * n + i) * n + j], ttv = tt[b * n + j], xxv = xx[b * n + i];
            const SdrTerms r = sdr_terms(a, ttv, xxv, (double)eps);
            // d sisdr/dx = K [ (2 alpha tt / c) t / S - ( ((2 alpha tt - 2a)/c - 2 alpha) t + 2 x ) / N ]
            const double ct = K * (2.0 * r.alpha * ttv / (r.c * r.S) - ((2.0 * r.alpha * ttv - 2.0 * a) / r.c - 2.0 * r.alpha) / r.Nn);
            cT[j] = (float)(g * ct);
            ce += g * K * (-2.0 / r.Nn);
        }
        cE = (float)ce;
    }
    __syncthreads();
    const float* e = est + ((size_t)b * n + i) * T;
    float* o = d_est + ((size_t)b * n + i) * T;
    const float cev = cE;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int t = blockIdx.x * 1024 + k * 256 + threadIdx.x;
        if (t < T) {
            float v = cev * e[t];
            for (int j = 0; j < n; ++j) {
                const float c = cT[j];
                if (c != 0.f) v = fmaf(c, tgt[((size_t)b * n + j) * T + t], v);
            }
            o[t] = v;
        }
    }
}

// one thread per batch item; permutations in itertools order, first extremum wins (torch.min/max semantics)
__global__ void pit_search_kernel(const float* __restrict__ val, const int32_t* __restrict__ perms, int P, int n, int B,
                                  int maximize, int use_mean, float* __restrict__ best_val, int64_t* __restrict__ best_idx) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const float* v = val + (size_t)b * n * n;
    float best = 0.f;
    int bi = 0;
    for (int p = 0; p < P; ++p) {
        float s = 0.f;
        for (int k = 0; k < n; ++k) s += v[k * n + perms[p * n + k]];
        if (use_mean) s /= (float)n;
        if (p == 0 || (maximize ? (s > best) : (s < best))) { best = s; bi = p; }
    }
    best_val[b] = best;
    best_idx[b] = bi;
}

// ---- Sinkhorn: one 64-thread block per batch item, all iterates kept for the reverse sweep --------
__device__ __forceinline__ void lse_step(double* Z, double* lse, int n, int over_rows, int tid) {
    // over_rows = 1: logsumexp over the first index i for every j (torch dim=1 of (B,n,n)); else over j for every i
    for (int q = tid; q < n; q += 64) {
        double mx = -1e300;
        for (int r = 0; r < n; ++r) { const double z = over_rows ? Z[r * n + q] : Z[q * n + r]; mx = z > mx ? z : mx; }
        double s = 0.0;
        for (int r = 0; r < n; ++r) { const double z = over_rows ? Z[r * n + q] : Z[q * n + r]; s += exp(z - mx); }
        lse[q] = mx + log(s);
    }
    __syncthreads();
    for (int e = tid; e < n * n; e += 64) Z[e] -= over_rows ? lse[e % n] : lse[e / n];
    __syncthreads();
}

__global__ __launch_bounds__(64) void sinkhorn_fwd_kernel(const float* __restrict__ C, double* __restrict__ zwork,
                                                          float* __restrict__ loss, float* __restrict__ Pout, int n,
                                                          float coldness, int iters) {
    extern __shared__ __attribute__((aligned(16))) double sh[];   // Z[n*n], lse[n], red[64]
    double* Z = sh;
    double* lse = sh + n * n;
    double* red = lse + n;
    const int b = blockIdx.x, tid = threadIdx.x, nn = n * n;
    const float* Cb = C + (size_t)b * nn;
    double* zw = zwork + (size_t)b * (2 * iters + 1) * nn;
    const double beta = (double)coldness;
    for (int e = tid; e < nn; e += 64) { Z[e] = -beta * (double)Cb[e]; zw[e] = Z[e]; }
    __syncthreads();
    for (int h = 1; h <= 2 * iters; ++h) {
        lse_step(Z, lse, n, h & 1, tid);
        for (int e = tid; e < nn; e += 64) zw[(size_t)h * nn + e] = Z[e];
    }
    double acc = 0.0;
    for (int e = tid; e < nn; e += 64) {
        const double p = exp(Z[e]);
        Pout[(size_t)b * nn + e] = (float)p;
        acc += ((double)Cb[e] + Z[e] / beta) * p;
    }
    red[tid] = acc;
    __syncthreads();
    if (tid == 0) { double s = 0.0; for (int k = 0; k < 64; ++k) s += red[k]; loss[b] = (float)s; }
}

__global__ __launch_bounds__(64) void sinkhorn_bwd_kernel(const float* __restrict__ C, const double* __restrict__ zwork,
                                                          const float* __restrict__ dloss, float* __restrict__ dC, int n,
                                                          float coldness, int iters) {
    extern __shared__ __attribute__((aligned(16))) double sh[];   // dZ[n*n], red[n]
    double* dZ = sh;
    double* red = sh + n * n;
    const int b = blockIdx.x, tid = threadIdx.x, nn = n * n;
    const float* Cb = C + (size_t)b * nn;
    const double* zw = zwork + (size_t)b * (2 * iters + 1) * nn;
    const double beta = (double)coldness, g = (double)dloss[b];
    const double* Zf = zw + (size_t)(2 * iters) * nn;
    for (int e = tid; e < nn; e += 64) {
        const double p = exp(Zf[e]);
        dZ[e] = g * p * (1.0 / beta + (double)Cb[e] + Zf[e] / beta);
    }
    __syncthreads();
    for (int h = 2 * iters; h >= 1; --h) {
        const int over_rows = h & 1;
        const double* Zh = zw + (size_t)h * nn;        // Z_h = Z_{h-1} - LSE  ->  softmax(Z_{h-1}) = exp(Z_h)
        for (int q = tid; q < n; q += 64) {
            double s = 0.0;
            for (int r = 0; r < n; ++r) s += over_rows ? dZ[r * n + q] : dZ[q * n + r];
            red[q] = s;
        }
        __syncthreads();
        for (int e = tid; e < nn; e += 64) dZ[e] -= exp(Zh[e]) * (over_rows ? red[e % n] : red[e / n]);
        __syncthreads();
    }
    for (int e = tid; e < nn; e += 64) {
        const double p = exp(Zf[e]);
        dC[(size_t)b * nn + e] = (float)(g * p - beta * dZ[e]);
    }
}

// ---- row difference sums: the O(T) part of the distance criteria and plain SDR ---------------------------
// One workgroup per row (rows = every leading index of the reduced axis).  sums[row] = {sum |x-t|, sum (x-t)^2,
// sum t^2}: fp32 partials per thread over <= T/256 elements, fp64 across the workgroup.
template <bool VEC>
__global__ __launch_bounds__(256) void rowdiff_sums_kernel(const float* __restrict__ x, const float* __restrict__ t,
                                                           double* __restrict__ sums, int T) {
    __shared__ double red[4];
    const int64_t base = (int64_t)blockIdx.x * T;
    float sa = 0.f, sq = 0.f, st = 0.f;
    if (VEC) {
        const float4* x4 = reinterpret_cast<const float4*>(x + base);
        const float4* t4 = reinterpret_cast<const float4*>(t + base);
        for (int i = threadIdx.x; i < T / 4; i += 256) {
            const float4 a = x4[i], b = t4[i];
            const float d0 = a.x - b.x, d1 = a.y - b.y, d2 = a.z - b.z, d3 = a.w - b.w;
            sa += (fabsf(d0) + fabsf(d1)) + (fabsf(d2) + fabsf(d3));
            sq = fmaf(d0, d0, fmaf(d1, d1, fmaf(d2, d2, fmaf(d3, d3, sq))));
            st = fmaf(b.x, b.x, fmaf(b.y, b.y, fmaf(b.z, b.z, fmaf(b.w, b.w, st))));
        }
    } else {
        for (int i = threadIdx.x; i < T; i += 256) {
            const float b = t[base + i], d = x[base + i] - b;
            sa += fabsf(d);
            sq = fmaf(d, d, sq);
            st = fmaf(b, b, st);
        }
    }
    const double ra = block_sum_256<double>((double)sa, red);
    const double rq = block_sum_256<double>((double)sq, red);
    const double rt = block_sum_256<double>((double)st, red);
    if (threadIdx.x == 0) {
        sums[3 * (int64_t)blockIdx.x + 0] = ra;
        sums[3 * (int64_t)blockIdx.x + 1] = rq;
        sums[3 * (int64_t)blockIdx.x + 2] = rt;
    }
}

// dx[row][i] = c_abs[row] * sign(x - t) + c_sq[row] * (x - t); grid = (column chunks of 1024, rows).
template <bool VEC>
__global__ __launch_bounds__(256) void rowdiff_bwd_kernel(const float* __restrict__ x, const float* __restrict__ t,
                                                          const float* __restrict__ c_abs, const float* __restrict__ c_sq,
                                                          float* __restrict__ dx, int T) {
    const int64_t base = (int64_t)blockIdx.y * T;
    const float ca = c_abs ? c_abs[blockIdx.y] : 0.f, cs = c_sq ? c_sq[blockIdx.y] : 0.f;
    auto g = [&](float d) { return fmaf(cs, d, d > 0.f ? ca : (d < 0.f ? -ca : 0.f)); };
    if (VEC) {
        const int i = blockIdx.x * 256 + threadIdx.x;
        if (i < T / 4) {
            const float4 a = reinterpret_cast<const float4*>(x + base)[i], b = reinterpret_cast<const float4*>(t + base)[i];
            reinterpret_cast<float4*>(dx + base)[i] = make_float4(g(a.x - b.x), g(a.y - b.y), g(a.z - b.z), g(a.w - b.w));
        }
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int i = blockIdx.x * 1024 + k * 256 + threadIdx.x;
            if (i < T) dx[base + i] = g(x[base + i] - t[base + i]);
        }
    }
}

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

extern "C" int sep_sisdr_dots(const float* est, const float* tgt, double* dots, double* tt, double* xx, int B, int n, int T,
                              int all_pairs, sep_stream_t stream) {
    SEP_REQUIRE(est && tgt && dots && tt && xx && B > 0 && n > 0 && T > 0, "sep_sisdr_dots: bad arguments");
    SEP_REQUIRE(n <= 64 && B <= 65535, "sep_sisdr_dots: n <= 64 and B <= 65535 supported");
    dim3 grid(ceil_div(T, DOT_CHUNK), all_pairs ? n * n : n, B);
    hipLaunchKernelGGL(sisdr_dots_kernel, grid, dim3(256), 0, (hipStream_t)stream, est, tgt, dots, tt, xx, n, T, all_pairs);
    SEP_CHECK_LAUNCH("sep_sisdr_dots");
    return 0;
}

extern "C" int sep_sisdr_from_dots(const double* dots, const double* tt, const double* xx, float* sisdr, int B, int n,
                                   int all_pairs, float eps, sep_stream_t stream) {
    SEP_REQUIRE(dots && tt && xx && sisdr && B > 0 && n > 0, "sep_sisdr_from_dots: bad arguments");
    hipLaunchKernelGGL(sisdr_from_dots_kernel, dim3(ceil_div(B * n * n, 256)), dim3(256), 0, (hipStream_t)stream, dots, tt, xx, sisdr, B, n, all_pairs, eps);
    SEP_CHECK_LAUNCH("sep_sisdr_from_dots");
    return 0;
}

extern "C" int sep_sisdr_bwd(const float* est, const float* tgt, const double* dots, const double* tt, const double* xx,
                             const float* gw, float* d_est, int B, int n, int T, int all_pairs, float eps,
                             sep_stream_t stream) {
    SEP_REQUIRE(est && tgt && dots && tt && xx && gw && d_est, "sep_sisdr_bwd: null pointer");
    SEP_REQUIRE(n <= 64 && B <= 65535, "sep_sisdr_bwd: n <= 64 and B <= 65535 supported");
    dim3 grid(ceil_div(T, 1024), n, B);
    hipLaunchKernelGGL(sisdr_bwd_kernel, grid, dim3(256), 0, (hipStream_t)stream, est, tgt, dots, tt, xx, gw, d_est, n, T, all_pairs, eps);
    SEP_CHECK_LAUNCH("sep_sisdr_bwd");
    return 0;
}

extern "C" int sep_pit_search(const float* val, const int32_t* perms, int P, int n, int B, int maximize, int use_mean,
                              float* best_val, int64_t* best_idx, sep_stream_t stream) {
    SEP_REQUIRE(val && perms && best_val && best_idx && P > 0 && n > 0 && B > 0, "sep_pit_search: bad arguments");
    hipLaunchKernelGGL(pit_search_kernel, dim3(ceil_div(B, 64)), dim3(64), 0, (hipStream_t)stream, val, perms, P, n, B, maximize, use_mean, best_val, best_idx);
    SEP_CHECK_LAUNCH("sep_pit_search");
    return 0;
}

extern "C" int sep_sinkhorn_fwd(const float* C, double* zwork, float* loss, float* P, int B, int n, float coldness,
                                int iters, sep_stream_t stream) {
    SEP_REQUIRE(C && zwork && loss && P && B > 0 && n > 0 && n <= 32 && iters >= 0 && coldness != 0.f, "sep_sinkhorn_fwd: bad arguments (n <= 32)");
    const size_t smem = (size_t)(n * n + n + 64) * sizeof(double);
    hipLaunchKernelGGL(sinkhorn_fwd_kernel, dim3(B), dim3(64), smem, (hipStream_t)stream, C, zwork, loss, P, n, coldness, iters);
    SEP_CHECK_LAUNCH("sep_sinkhorn_fwd");
    return 0;
}

extern "C" int sep_sinkhorn_bwd(const float* C, const double* zwork, const float* dloss, float* dC, int B, int n,
                                float coldness, int iters, sep_stream_t stream) {
    SEP_REQUIRE(C && zwork && dloss && dC && B > 0 && n > 0 && n <= 32 && iters >= 0, "sep_sinkhorn_bwd: bad arguments (n <= 32)");
    const size_t smem = (size_t)(n * n + n) * sizeof(double);
    hipLaunchKernelGGL(sinkhorn_bwd_kernel, dim3(B), dim3(64), smem, (hipStream_t)stream, C, zwork, dloss, dC, n, coldness, iters);
    SEP_CHECK_LAUNCH("sep_sinkhorn_bwd");
    return 0;
}

extern "C" int sep_rowdiff_sums(const float* x, const float* t, double* sums, int64_t rows, int T, sep_stream_t stream) {
    SEP_REQUIRE(x && t && sums && rows > 0 && rows < (1ll << 31) && T > 0, "sep_rowdiff_sums: bad arguments");
    const bool vec = T % 4 == 0 && (((uintptr_t)x | (uintptr_t)t) & 15) == 0;
    if (vec) hipLaunchKernelGGL(rowdiff_sums_kernel<true>, dim3((unsigned)rows), dim3(256), 0, (hipStream_t)stream, x, t, sums, T);
    else hipLaunchKernelGGL(rowdiff_sums_kernel<false>, dim3((unsigned)rows), dim3(256), 0, (hipStream_t)stream, x, t, sums, T);
    SEP_CHECK_LAUNCH("sep_rowdiff_sums");
    return 0;
}

extern "C" int sep_rowdiff_bwd(const float* x, const float* t, const float* c_abs, const float* c_sq, float* dx, int64_t rows,
                               int T, sep_stream_t stream) {
    SEP_REQUIRE(x && t && dx && (c_abs || c_sq) && rows > 0 && rows < 65536 && T > 0, "sep_rowdiff_bwd: bad arguments");
    const bool vec = T % 4 == 0 && (((uintptr_t)x | (uintptr_t)t | (uintptr_t)dx) & 15) == 0;
    const dim3 grid((unsigned)((T + 1023) / 1024), (unsigned)rows);
    if (vec) hipLaunchKernelGGL(rowdiff_bwd_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, x, t, c_abs, c_sq, dx, T);
    else hipLaunchKernelGGL(rowdiff_bwd_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, x, t, c_abs, c_sq, dx, T);
    SEP_CHECK_LAUNCH("sep_rowdiff_bwd");
    return 0;
}

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

// ---- BSS-eval v3 ("sources"): the O(T) parts of SDR / SIR / SAR -------------------------------------------------------------------------
// Reference arithmetic replaced: src/utils/bss.py:4-30 (a wrapper of mir_eval.separation.bss_eval_sources), called per utterance by
// egs/wsj0-mix/common/src/driver.py:291-309.  The metric projects every estimate on the span of the references delayed by 0 .. flen - 1
// samples (normal equations) and compares energies.  Two O(T flen) passes are kernels here -- the lagged correlations that fill the normal
// equations and the FIR pass that turns the solved filters into the five energies of a pair; the (n flen)^2 solve between them is the
// caller's (utils/bss.py).  fp64 arithmetic on fp32 audio.  No atomics: every workgroup owns one time slab of FIXED size and writes its partial
// sums to the caller's scratch, a second launch adds the slabs in ascending order -- two runs give the same bits, and a row gives the same
// bits whatever the pitch T and the batch around it are (samples beyond a row's length enter as exact zeros, slabs beyond it as 0.0).
namespace {

constexpr int BSS_TILE = 256;           // samples staged per step = lags (outputs) per workgroup: one per thread
constexpr int BSS_XC_SLAB = 2048;       // time samples behind one partial of sep_bss_xcorr
constexpr int BSS_EN_SLAB = 1024;       // output samples behind one partial of sep_bss_energies
constexpr int BSS_MAX_T = 1 << 30;

__device__ __forceinline__ int bss_row_length(const int32_t* lengths, const int b, const int T) {
    if (!lengths) return T;
    const int v = lengths[b];
    return v < 0 ? 0 : (v > T ? T : v);
}

static inline int64_t bss_slabs(const int64_t len, const int slab) { return (len + slab - 1) / slab; }

// part[b][i][k][slab][l] = sum over the slab's t of a[b][i][t] c[b][k][t + lag_lo + l].  grid (nslab * lag tiles, n m, B).
// a_s holds the tile of a, c_s the 2 BSS_TILE - 1 samples of c that BSS_TILE lags of it touch: a_s[tt] is one address for the whole wave (a
// broadcast), c_s[tt + lane] consecutive doubles (no bank conflict).
__global__ __launch_bounds__(256) void bss_xcorr_kernel(const float* __restrict__ a, const float* __restrict__ c, double* __restrict__ part,
                                                        const int32_t* __restrict__ lengths, const int n, const int m, const int T,
                                                        const int lag_lo, const int nlag, const int nslab) {
    __shared__ double a_s[BSS_TILE];
    __shared__ double c_s[2 * BSS_TILE];
    const int tid = threadIdx.x, b = blockIdx.z, i = blockIdx.y / m, k = blockIdx.y % m;
    const int slab = blockIdx.x % nslab, l0 = (blockIdx.x / nslab) * BSS_TILE;
    const int Tb = bss_row_length(lengths, b, T);
    const float* ar = a + ((int64_t)b * n + i) * T;
    const float* cr = c + ((int64_t)b * m + k) * T;
    const int64_t shift = (int64_t)lag_lo + l0;                         // c_s[q] = c[t0 + shift + q]
    const int64_t t_end = (int64_t)(slab + 1) * BSS_XC_SLAB < Tb ? (int64_t)(slab + 1) * BSS_XC_SLAB : Tb;
    double acc = 0.0;
    for (int64_t t0 = (int64_t)slab * BSS_XC_SLAB; t0 < t_end; t0 += BSS_TILE) {
        a_s[tid] = t0 + tid < Tb ? (double)ar[t0 + tid] : 0.0;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int q = tid + h * BSS_TILE;
            const int64_t u = t0 + shift + q;
            c_s[q] = (u >= 0 && u < Tb) ? (double)cr[u] : 0.0;
        }
        __syncthreads();
#pragma unroll 8
        for (int tt = 0; tt < BSS_TILE; ++tt) acc = fma(a_s[tt], c_s[tt + tid], acc);
        __syncthreads();
    }
    if (l0 + tid < nlag) part[((((int64_t)b * n + i) * m + k) * nslab + slab) * nlag + l0 + tid] = acc;
}

// out[o][r] = part[o][0][r] + part[o][1][r] + ... in this order; total = outer * inner
__global__ __launch_bounds__(256) void bss_reduce_kernel(const double* __restrict__ part, double* __restrict__ out, const int nslab,
                                                         const int inner, const int64_t total) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= total) return;
    const int64_t o = e / inner, r = e % inner;
    double s = 0.0;
    for (int sl = 0; sl < nslab; ++sl) s += part[(o * nslab + sl) * inner + r];
    out[e] = s;
}

// The pair (estimate j, reference i) of sample b, output samples [slab BSS_EN_SLAB, (slab + 1) BSS_EN_SLAB) of the T_b + flen - 1: thread `tid`
// of a step owns t = t0 + tid and forms P_all(e_j)[t] = sum_k sum_tau fa[j][k][tau] r_k[t - tau] (passes 0 .. n - 1) and
// P_i(e_j)[t] = sum_tau fo[j][i][tau] r_i[t - tau] (pass n) from staged tiles: r_s[q] = r[t0 - tau0 - (BSS_TILE - 1) + q], so the tap tau0 + x
// of thread tid reads r_s[tid + BSS_TILE - 1 - x] -- consecutive doubles across the wave, the tap itself a broadcast.  The projected signals
// live in registers only.  grid (nslab, m n, B).
__global__ __launch_bounds__(256) void bss_energies_kernel(const float* __restrict__ ref, const float* __restrict__ est,
                                                           const double* __restrict__ filt_all, const double* __restrict__ filt_one,
                                                           double* __restrict__ part, const int32_t* __restrict__ lengths, const int n,
                                                           const int m, const int T, const int flen, const int nslab) {
    __shared__ double r_s[2 * BSS_TILE];
    __shared__ double f_s[BSS_TILE];
    __shared__ double red[4];
    const int tid = threadIdx.x, b = blockIdx.z, j = blockIdx.y / n, i = blockIdx.y % n, slab = blockIdx.x;
    const int Tb = bss_row_length(lengths, b, T);
    const int64_t Tx = Tb > 0 ? (int64_t)Tb + flen - 1 : 0;
    const int64_t t_end = (int64_t)(slab + 1) * BSS_EN_SLAB < Tx ? (int64_t)(slab + 1) * BSS_EN_SLAB : Tx;
    const float* er = est + ((int64_t)b * m + j) * T;
    double e_s = 0.0, e_i = 0.0, e_a = 0.0, e_ia = 0.0, e_si = 0.0;
    for (int64_t t0 = (int64_t)slab * BSS_EN_SLAB; t0 < t_end; t0 += BSS_TILE) {
        double pall = 0.0, sf = 0.0;
        for (int pass = 0; pass <= n; ++pass) {
            const int k = pass < n ? pass : i;
            const float* rr = ref + ((int64_t)b * n + k) * T;
            const double* f = (pass < n ? filt_all : filt_one) + (((int64_t)b * m + j) * n + k) * flen;
            double acc = 0.0;
            for (int tau0 = 0; tau0 < flen; tau0 += BSS_TILE) {
                const int nx = flen - tau0 < BSS_TILE ? flen - tau0 : BSS_TILE;
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    const int q = tid + h * BSS_TILE;
                    const int64_t u = t0 - tau0 - (BSS_TILE - 1) + q;
                    r_s[q] = (u >= 0 && u < Tb) ? (double)rr[u] : 0.0;
                }
                f_s[tid] = tid < nx ? f[tau0 + tid] : 0.0;
                __syncthreads();
#pragma unroll 4
                for (int x = 0; x < nx; ++x) acc = fma(f_s[x], r_s[tid + BSS_TILE - 1 - x], acc);
                __syncthreads();
            }
            if (pass < n) pall += acc; else sf = acc;
        }
        const int64_t t = t0 + tid;
        if (t < Tx) {
            const double e = t < Tb ? (double)er[t] : 0.0;
            const double interf = pall - sf, artif = e - pall;
            e_s = fma(sf, sf, e_s);
            e_i = fma(interf, interf, e_i);
            e_a = fma(artif, artif, e_a);
            e_ia = fma(interf + artif, interf + artif, e_ia);
            e_si = fma(sf + interf, sf + interf, e_si);
        }
    }
    const double v[5] = {e_s, e_i, e_a, e_ia, e_si};
#pragma unroll
    for (int q = 0; q < 5; ++q) {
        const double r = block_sum_256<double>(v[q], red);
        if (tid == 0) part[((((int64_t)b * m + j) * n + i) * nslab + slab) * 5 + q] = r;
    }
}

// doubles of scratch one call needs, or -1 where a grid limit is exceeded
static int64_t bss_xcorr_scratch(const int B, const int n, const int m, const int T, const int nlag) {
    const int64_t nslab = bss_slabs(T, BSS_XC_SLAB), ntile = bss_slabs(nlag, BSS_TILE);
    int64_t need = (int64_t)B * n * m;                                  // (< 2^32 once the grid limits hold)
    if ((int64_t)n * m > 65535 || B > 65535 || nslab * ntile > 0x7fffffff) return -1;
    if (((int64_t)B * n * m * nlag + 255) / 256 > 0x7fffffff) return -1;   // the grid of the reduction
    if (__builtin_mul_overflow(need, nslab * nlag, &need) || need > (int64_t)1 << 56) return -1;
    return need;
}
static int64_t bss_energies_scratch(const int B, const int n, const int m, const int T, const int flen) {
    const int64_t nslab = bss_slabs((int64_t)T + flen - 1, BSS_EN_SLAB);
    if ((int64_t)n * m > 65535 || B > 65535) return -1;
    return (int64_t)B * n * m * nslab * 5;
}
static bool bss_shape_ok(const int B, const int n, const int m, const int T) { return B >= 1 && n >= 1 && m >= 1 && T >= 1 && T <= BSS_MAX_T; }

}  // namespace

extern "C" size_t sep_bss_scratch_bytes(int B, int n, int m, int T, int flen) {
    if (!bss_shape_ok(B, n, m, T) || flen < 1 || flen > BSS_MAX_T / 2) return 0;
    const int64_t need[3] = {bss_xcorr_scratch(B, n, n, T, 2 * flen - 1), bss_xcorr_scratch(B, n, m, T, flen), bss_energies_scratch(B, n, m, T, flen)};
    int64_t most = 0;
    for (int q = 0; q < 3; ++q) {
        if (need[q] < 0) return 0;
        most = need[q] > most ? need[q] : most;
    }
    return (size_t)most * sizeof(double);
}

extern "C" int sep_bss_xcorr(const float* a, const float* c, const int32_t* lengths, double* out, double* scratch, size_t scratch_bytes, int B,
                             int n, int m, int T, int lag_lo, int nlag, sep_stream_t stream) {
    SEP_REQUIRE(a && c && out && scratch, "sep_bss_xcorr: null pointer");
    SEP_REQUIRE(bss_shape_ok(B, n, m, T) && nlag >= 1 && nlag <= BSS_MAX_T && lag_lo >= -BSS_MAX_T && lag_lo <= BSS_MAX_T,
                "sep_bss_xcorr: bad arguments (B=%d n=%d m=%d T=%d lag_lo=%d nlag=%d; all counts >= 1, T and the lags within 2^30)", B, n, m, T, lag_lo, nlag);
    const int64_t need = bss_xcorr_scratch(B, n, m, T, nlag);
    SEP_REQUIRE(need >= 0, "sep_bss_xcorr: grid limit (B <= 65535, n m <= 65535, slabs x lag tiles < 2^31, B n m nlag < 2^39, scratch < 2^59 bytes)");
    SEP_REQUIRE(scratch_bytes / sizeof(double) >= (size_t)need, "sep_bss_xcorr: scratch holds %zu bytes, %lld needed", scratch_bytes,
                (long long)need * (long long)sizeof(double));
    const int nslab = (int)bss_slabs(T, BSS_XC_SLAB), ntile = (int)bss_slabs(nlag, BSS_TILE);
    hipLaunchKernelGGL(bss_xcorr_kernel, dim3((unsigned)(nslab * ntile), (unsigned)(n * m), (unsigned)B), dim3(256), 0, (hipStream_t)stream, a, c, scratch,
                       lengths, n, m, T, lag_lo, nlag, nslab);
    SEP_CHECK_LAUNCH("sep_bss_xcorr");
    const int64_t total = (int64_t)B * n * m * nlag;
    hipLaunchKernelGGL(bss_reduce_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (const double*)scratch, out, nslab, nlag, total);
    SEP_CHECK_LAUNCH("sep_bss_xcorr (reduction)");
    return 0;
}

extern "C" int sep_bss_energies(const float* ref, const float* est, const double* filt_all, const double* filt_one, const int32_t* lengths,
                                double* out, double* scratch, size_t scratch_bytes, int B, int n, int m, int T, int flen, sep_stream_t stream) {
    SEP_REQUIRE(ref && est && filt_all && filt_one && out && scratch, "sep_bss_energies: null pointer");
    SEP_REQUIRE(bss_shape_ok(B, n, m, T) && flen >= 1 && flen <= BSS_MAX_T,
                "sep_bss_energies: bad arguments (B=%d n=%d m=%d T=%d flen=%d; all >= 1, T and flen within 2^30)", B, n, m, T, flen);
    const int64_t need = bss_energies_scratch(B, n, m, T, flen);
    SEP_REQUIRE(need >= 0, "sep_bss_energies: grid limit (B <= 65535, n m <= 65535)");
    SEP_REQUIRE(scratch_bytes / sizeof(double) >= (size_t)need, "sep_bss_energies: scratch holds %zu bytes, %lld needed", scratch_bytes,
                (long long)need * (long long)sizeof(double));
    const int nslab = (int)bss_slabs((int64_t)T + flen - 1, BSS_EN_SLAB);
    hipLaunchKernelGGL(bss_energies_kernel, dim3((unsigned)nslab, (unsigned)(m * n), (unsigned)B), dim3(256), 0, (hipStream_t)stream, ref, est, filt_all,
                       filt_one, scratch, lengths, n, m, T, flen, nslab);
    SEP_CHECK_LAUNCH("sep_bss_energies");
    const int64_t total = (int64_t)B * m * n * 5;
    hipLaunchKernelGGL(bss_reduce_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (const double*)scratch, out, nslab, 5, total);
    SEP_CHECK_LAUNCH("sep_bss_energies (reduction)");
    return 0;
}

// ---- BSS-eval v4 ("images"): the framewise decomposition pass of museval's SDR / ISR / SIR / SAR ---------------------------------------------
// Reference arithmetic replaced: museval.eval_mus_track, where the reference's music tester ends (egs/musdb18/conv-tasnet/src/adhoc_driver.py:
// 352-380).  The filters are the caller's (utils/bss.py: sep_bss_xcorr on (B, n C, T) views, one dense solve per row); this pass applies them to
// every frame's segment alone -- samples outside the frame count as zero -- and forms the seven energies and the two silence counts of a
// (frame, source).  The rules of the v3 kernels hold: no atomics, slabs of FIXED size counted from the frame's first sample, partials added in
// ascending order by bss_reduce_kernel, 64-bit offsets, the projected signals in registers only.
namespace {

constexpr int BSS_IM_SLAB = 1024;       // output samples of a frame behind one partial of sep_bss_image_energies
constexpr int BSS_IM_SUMS = 9;

__device__ __forceinline__ int bss_row_frames(const int Tb, const int window, const int hop, const int nwin) {
    if (Tb < window) return 0;
    const int64_t f = ((int64_t)Tb - window + hop) / hop;               // every frame is full: (f - 1) hop + window <= Tb
    return f < nwin ? (int)f : nwin;
}

// Frame w of source j of sample b, output samples [slab BSS_IM_SLAB, (slab + 1) BSS_IM_SLAB) of the frame's window + flen - 1: thread `tid` of a
// step owns t = t0 + tid and forms, for every channel c in turn, P_all[t] = sum_{kc} sum_tau fa[j][c][kc][tau] r_w[kc][t - tau] in ONE walk over
// the n C reference channels; the C channels of source j feed P_j[t] = sum_{c2} sum_tau fo[j][c][c2][tau] r_w[j][c2][t - tau] from the same
// staged tile.  r_s[q] = r_w[t0 - tau0 - (BSS_TILE - 1) + q] with r_w zero outside [0, window): the tap tau0 + x of thread tid reads
// r_s[tid + BSS_TILE - 1 - x] -- consecutive doubles across the wave, the taps broadcasts.  A frame beyond the row's own count writes zeros.
// grid (nslab, n nwin, B).
__global__ __launch_bounds__(256) void bss_image_energies_kernel(const float* __restrict__ ref, const float* __restrict__ est,
                                                                 const double* __restrict__ filt_all, const double* __restrict__ filt_one,
                                                                 double* __restrict__ part, const int32_t* __restrict__ lengths, const int n,
                                                                 const int C, const int T, const int flen, const int window, const int hop,
                                                                 const int nwin, const int nslab) {
    __shared__ double r_s[2 * BSS_TILE];
    __shared__ double f_s[BSS_TILE];
    __shared__ double g_s[BSS_TILE];
    __shared__ double red[4];
    const int tid = threadIdx.x, b = blockIdx.z, j = blockIdx.y / nwin, w = blockIdx.y % nwin, slab = blockIdx.x;
    double* po = part + ((((int64_t)b * n + j) * nwin + w) * nslab + slab) * BSS_IM_SUMS;
    if (w >= bss_row_frames(bss_row_length(lengths, b, T), window, hop, nwin)) {           // (the same for the whole workgroup)
        if (tid < BSS_IM_SUMS) po[tid] = 0.0;
        return;
    }
    const int nc = n * C;
    const int64_t Wx = (int64_t)window + flen - 1, origin = (int64_t)w * hop;              // origin + window <= T_b
    const int64_t t_end = (int64_t)(slab + 1) * BSS_IM_SLAB < Wx ? (int64_t)(slab + 1) * BSS_IM_SLAB : Wx;
    const float* rb = ref + (int64_t)b * nc * T + origin;
    const float* eb = est + ((int64_t)b * n + j) * C * T + origin;
    double v[BSS_IM_SUMS] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int64_t t0 = (int64_t)slab * BSS_IM_SLAB; t0 < t_end; t0 += BSS_TILE) {
        const int64_t t = t0 + tid;
        double rsum = 0.0, esum = 0.0;
        for (int c = 0; c < C; ++c) {
            double pall = 0.0, pj = 0.0;
            for (int kc = 0; kc < nc; ++kc) {
                const bool own = kc / C == j;
                const float* rr = rb + (int64_t)kc * T;
                const double* fa = filt_all + ((((int64_t)b * n + j) * C + c) * nc + kc) * flen;
                const double* fo = filt_one + ((((int64_t)b * n + j) * C + c) * C + (own ? kc - j * C : 0)) * flen;
                for (int tau0 = 0; tau0 < flen; tau0 += BSS_TILE) {
                    const int nx = flen - tau0 < BSS_TILE ? flen - tau0 : BSS_TILE;
#pragma unroll
                    for (int h = 0; h < 2; ++h) {
                        const int q = tid + h * BSS_TILE;
                        const int64_t u = t0 - tau0 - (BSS_TILE - 1) + q;
                        r_s[q] = (u >= 0 && u < window) ? (double)rr[u] : 0.0;
                    }
                    f_s[tid] = tid < nx ? fa[tau0 + tid] : 0.0;
                    if (own) g_s[tid] = tid < nx ? fo[tau0 + tid] : 0.0;
                    __syncthreads();
                    if (own) {
#pragma unroll 4
                        for (int x = 0; x < nx; ++x) {
                            const double r = r_s[tid + BSS_TILE - 1 - x];
                            pall = fma(f_s[x], r, pall);
                            pj = fma(g_s[x], r, pj);
                        }
                    } else {
#pragma unroll 4
                        for (int x = 0; x < nx; ++x) pall = fma(f_s[x], r_s[tid + BSS_TILE - 1 - x], pall);
                    }
                    __syncthreads();
                }
            }
            if (t < Wx) {
                const bool in = t < window;
                const double s = in ? (double)rb[((int64_t)j * C + c) * T + t] : 0.0, e = in ? (double)eb[(int64_t)c * T + t] : 0.0;
                const double d = e - s, sp = pj - s, it = pall - pj, ar = e - pall;
                v[0] = fma(s, s, v[0]);
                v[1] = fma(d, d, v[1]);
                v[2] = fma(sp, sp, v[2]);
                v[3] = fma(pj, pj, v[3]);
                v[4] = fma(it, it, v[4]);
                v[5] = fma(pall, pall, v[5]);
                v[6] = fma(ar, ar, v[6]);
                rsum += s;
                esum += e;
            }
        }
        if (t < window) {
            v[7] += rsum != 0.0 ? 1.0 : 0.0;
            v[8] += esum != 0.0 ? 1.0 : 0.0;
        }
    }
#pragma unroll
    for (int q = 0; q < BSS_IM_SUMS; ++q) {
        const double r = block_sum_256<double>(v[q], red);
        if (tid == 0) po[q] = r;
    }
}

// doubles of scratch the call needs, or -1 where a grid limit is exceeded
static int64_t bss_image_scratch(const int B, const int n, const int flen, const int window, const int nwin) {
    const int64_t nslab = bss_slabs((int64_t)window + flen - 1, BSS_IM_SLAB);
    if ((int64_t)n * nwin > 65535 || B > 65535) return -1;
    return (int64_t)B * n * nwin * nslab * BSS_IM_SUMS;                // < 2^16 2^16 2^21 9
}
static bool bss_image_shape_ok(const int B, const int n, const int C, const int flen, const int window, const int nwin) {
    return B >= 1 && n >= 1 && C >= 1 && (int64_t)n * C <= 65535 && flen >= 1 && flen <= BSS_MAX_T && window >= 1 && window <= BSS_MAX_T && nwin >= 1;
}

}  // namespace

extern "C" size_t sep_bss_image_scratch_bytes(int B, int n, int C, int flen, int window, int nwin) {
    if (!bss_image_shape_ok(B, n, C, flen, window, nwin)) return 0;
    const int64_t need = bss_image_scratch(B, n, flen, window, nwin);
    return need < 0 ? 0 : (size_t)need * sizeof(double);
}

extern "C" int sep_bss_image_energies(const float* ref, const float* est, const double* filt_all, const double* filt_one, const int32_t* lengths,
                                      double* out, double* scratch, size_t scratch_bytes, int B, int n, int C, int T, int flen, int window, int hop,
                                      int nwin, sep_stream_t stream) {
    SEP_REQUIRE(ref && est && filt_all && filt_one && out && scratch, "sep_bss_image_energies: null pointer");
    SEP_REQUIRE(bss_image_shape_ok(B, n, C, flen, window, nwin) && T >= 1 && T <= BSS_MAX_T && hop >= 1 && hop <= BSS_MAX_T,
                "sep_bss_image_energies: bad arguments (B=%d n=%d C=%d T=%d flen=%d window=%d hop=%d nwin=%d; all >= 1, n C <= 65535, T, flen, window "
                "and hop within 2^30)", B, n, C, T, flen, window, hop, nwin);
    const int64_t need = bss_image_scratch(B, n, flen, window, nwin);
    SEP_REQUIRE(need >= 0, "sep_bss_image_energies: grid limit (B <= 65535, n nwin <= 65535)");
    SEP_REQUIRE(scratch_bytes / sizeof(double) >= (size_t)need, "sep_bss_image_energies: scratch holds %zu bytes, %lld needed", scratch_bytes,
                (long long)need * (long long)sizeof(double));
    const int nslab = (int)bss_slabs((int64_t)window + flen - 1, BSS_IM_SLAB);
    hipLaunchKernelGGL(bss_image_energies_kernel, dim3((unsigned)nslab, (unsigned)(n * nwin), (unsigned)B), dim3(256), 0, (hipStream_t)stream, ref, est,
                       filt_all, filt_one, scratch, lengths, n, C, T, flen, window, hop, nwin, nslab);
    SEP_CHECK_LAUNCH("sep_bss_image_energies");
    const int64_t total = (int64_t)B * n * nwin * BSS_IM_SUMS;
    hipLaunchKernelGGL(bss_reduce_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (const double*)scratch, out, nslab,
                       BSS_IM_SUMS, total);
    SEP_CHECK_LAUNCH("sep_bss_image_energies (reduction)");
    return 0;
}

// ---- Mixture invariant training (MixIT) ---------------------------------------------------------------------------------------------------
// The reference has no arithmetic to replace here: src/criterion/mixit.py is a stub that raises NotImplementedError.  The criterion is the one
// of Wisdom et al. 2020: the best of the N^M ways to hand each of M estimates to one of N reference mixtures.  Every measure this library
// knows is a function of <x_n, x_n>, <x_n, y_n> and <y_n, y_n>, and for a remix y_n = sum_{m in set} s_m those are sums of entries of the Gram
// matrix of the M + N rows: one pass over the waveforms gives the value of every assignment (sep_mixit_gram, sep_mixit_search), one more
// pass the gradient of the chosen one (sep_mixit_bwd).  The contract is in include/sepkernels.h.
namespace {

constexpr int MIXIT_SLAB = SEP_MIXIT_SLAB;      // samples behind one partial of sep_mixit_gram: 8 per thread
constexpr int MIXIT_MAX_M = SEP_MIXIT_MAX_EST, MIXIT_MAX_N = SEP_MIXIT_MAX_MIX, MIXIT_MAX_R = MIXIT_MAX_M + MIXIT_MAX_N;
constexpr int MIXIT_GRAM_BLOCK = 8;             // rows per block of the blocked form (R > 12)
static_assert(MIXIT_SLAB % 256 == 0, "a slab is a whole number of 256-sample steps");

__device__ __forceinline__ const float* mixit_row(const float* est, const float* tgt, const int b, const int M, const int N, const int T, const int r) {
    return r < M ? est + ((int64_t)b * M + r) * T : tgt + ((int64_t)b * N + (r - M)) * T;
}

// part[b][slab][i][j] = sum over the slab's t of row_i[t] row_j[t], rows = the item's estimates, then its mixtures.  grid (nslab, block pairs, B).
// TRI: R <= RB, the workgroup owns the whole matrix: a thread holds the R values of a sample and forms the RB (RB + 1) / 2 products of the upper
// triangle (rows beyond R enter as zeros and are not stored).  Otherwise the workgroup owns rows [RB bi, RB bi + RB) x [RB bj, RB bj + RB),
// bi <= bj, as a full square.  Per thread the samples are added in ascending order, the wave by a butterfly, the four waves in order.
template <int RB, bool TRI>
__global__ __launch_bounds__(256) void mixit_gram_kernel(const float* __restrict__ est, const float* __restrict__ tgt, double* __restrict__ part,
                                                         const int M, const int N, const int T, const int nslab) {
    constexpr int NACC = TRI ? RB * (RB + 1) / 2 : RB * RB;
    __shared__ double red[4][NACC];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, slab = blockIdx.x, b = blockIdx.z, R = M + N;
    int bi = 0, bj = 0;
    if (!TRI) {
        const int nblk = (R + RB - 1) / RB;
        int p = blockIdx.y;
        while (p >= nblk - bi) { p -= nblk - bi; ++bi; }
        bj = bi + p;
    }
    const int ra = bi * RB, rb = bj * RB;
    const float* pa[RB];
    const float* pb[RB];
#pragma unroll
    for (int i = 0; i < RB; ++i) {
        pa[i] = ra + i < R ? mixit_row(est, tgt, b, M, N, T, ra + i) : nullptr;
        pb[i] = rb + i < R ? mixit_row(est, tgt, b, M, N, T, rb + i) : nullptr;
    }
    double acc[NACC];
#pragma unroll
    for (int q = 0; q < NACC; ++q) acc[q] = 0.0;
    const int64_t t0 = (int64_t)slab * MIXIT_SLAB;
#pragma unroll 2
    for (int k = 0; k < MIXIT_SLAB / 256; ++k) {
        const int64_t t = t0 + k * 256 + tid;
        if (t < T) {
            double va[RB], vb[RB];
#pragma unroll
            for (int i = 0; i < RB; ++i) va[i] = pa[i] ? (double)pa[i][t] : 0.0;
            if (TRI) {
                int q = 0;
#pragma unroll
                for (int i = 0; i < RB; ++i)
#pragma unroll
                    for (int j = i; j < RB; ++j, ++q) acc[q] = fma(va[i], va[j], acc[q]);
            } else {
#pragma unroll
                for (int i = 0; i < RB; ++i) vb[i] = pb[i] ? (double)pb[i][t] : 0.0;
#pragma unroll
                for (int i = 0; i < RB; ++i)
#pragma unroll
                    for (int j = 0; j < RB; ++j) acc[i * RB + j] = fma(va[i], vb[j], acc[i * RB + j]);
            }
        }
    }
#pragma unroll
    for (int q = 0; q < NACC; ++q) {
        const double v = wave_sum(acc[q]);
        if (lane == 0) red[w][q] = v;
    }
    __syncthreads();
    double* P = part + ((int64_t)b * nslab + slab) * R * R;
    for (int q = tid; q < NACC; q += 256) {
        int i, j;
        if (TRI) {
            i = 0;
            int rem = q;
            while (rem >= RB - i) { rem -= RB - i; ++i; }
            j = i + rem;
        } else {
            i = q / RB;
            j = q % RB;
        }
        const int gi = ra + i, gj = rb + j;
        if (gi >= R || gj >= R) continue;
        const int src = (!TRI && bi == bj && i > j) ? j * RB + i : q;      // a diagonal block: both triangles from the upper one
        const double s = ((red[0][src] + red[1][src]) + red[2][src]) + red[3][src];
        P[gi * R + gj] = s;
        if (TRI || bi != bj) P[gj * R + gi] = s;
    }
}

// the estimates of mixture n under `code`, as a bit mask: estimate 0 is the most significant digit of the code in base N
__device__ __forceinline__ unsigned mixit_set(int code, const int M, const int N, const int n) {
    unsigned mask = 0;
    for (int m = M - 1; m >= 0; --m) {
        if (code % N == n) mask |= 1u << m;
        code /= N;
    }
    return mask;
}

// a = sum_{m in set} G[M+n][m], yy = sum_{m, m' in set} G[m][m'] (the diagonal once, the upper triangle twice), estimates in ascending order
__device__ __forceinline__ void mixit_sums(const double* G, const int R, const int M, const int n, const unsigned mask, double& a, double& yy) {
    a = 0.0;
    yy = 0.0;
    for (int m = 0; m < M; ++m) {
        if (!((mask >> m) & 1u)) continue;
        a += G[(M + n) * R + m];
        double s = 0.0;
        for (int q = m + 1; q < M; ++q)
            if ((mask >> q) & 1u) s += G[m * R + q];
        yy += G[m * R + m] + 2.0 * s;
    }
}

// the measure of one mixture in dB and the coefficients of d measure / d y = cT x + cE y
__device__ __forceinline__ double mixit_measure(const int kind, const double a, const double ttv, const double yy, const double eps, const double tau,
                                                double* cT, double* cE) {
    const double K = 10.0 / log(10.0);
    if (kind == 0) {
        const SdrTerms r = sdr_terms(a, ttv, yy, eps);
        if (cT) {   // sisdr_bwd_kernel's expressions with xx = yy
            *cT = K * (2.0 * r.alpha * ttv / (r.c * r.S) - ((2.0 * r.alpha * ttv - 2.0 * a) / r.c - 2.0 * r.alpha) / r.Nn);
            *cE = K * (-2.0 / r.Nn);
        }
        return 10.0 * log10(r.S / r.Nn);
    }
    double nn = ttv - 2.0 * a + yy;          // |x - y|^2
    if (nn < 0.0) nn = 0.0;
    const double den = nn + (kind == 2 ? tau * ttv : 0.0) + eps;
    if (cT) {
        *cT = 2.0 * K / den;
        *cE = -2.0 * K / den;
    }
    return 10.0 * log10((ttv + eps) / den);
}

// one workgroup per item; thread `tid` scores the codes tid, tid + 256, ... in ascending order
__global__ __launch_bounds__(256) void mixit_search_kernel(const double* __restrict__ gram, const int M, const int N, const int ncodes, const int kind,
                                                           const int maximize, const int use_mean, const double eps, const double tau,
                                                           float* __restrict__ best_val, int64_t* __restrict__ best_idx, float* __restrict__ per_mix) {
    __shared__ double G[MIXIT_MAX_R * MIXIT_MAX_R];
    __shared__ double rv[256];
    __shared__ int rc[256];
    const int b = blockIdx.x, tid = threadIdx.x, R = M + N;
    for (int e = tid; e < R * R; e += 256) G[e] = gram[(int64_t)b * R * R + e];
    __syncthreads();
    double best = 0.0;
    int bc = -1;
    for (int code = tid; code < ncodes; code += 256) {
        double s = 0.0;
        for (int n = 0; n < N; ++n) {
            double a, yy;
            mixit_sums(G, R, M, n, mixit_set(code, M, N, n), a, yy);
            s += mixit_measure(kind, a, G[(M + n) * R + M + n], yy, eps, tau, nullptr, nullptr);
        }
        if (use_mean) s /= (double)N;
        if (bc < 0 || (maximize ? s > best : s < best)) { best = s; bc = code; }
    }
    rv[tid] = best;
    rc[tid] = bc;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {      // the extremum; equal values keep the lower code
        if (tid < h) {
            const double v1 = rv[tid], v2 = rv[tid + h];
            const int c1 = rc[tid], c2 = rc[tid + h];
            if (c2 >= 0 && (c1 < 0 || (maximize ? v2 > v1 : v2 < v1) || (v2 == v1 && c2 < c1))) { rv[tid] = v2; rc[tid] = c2; }
        }
        __syncthreads();
    }
    const int code = rc[0];
    if (tid < N) {
        double a, yy;
        mixit_sums(G, R, M, tid, mixit_set(code, M, N, tid), a, yy);
        per_mix[(int64_t)b * N + tid] = (float)mixit_measure(kind, a, G[(M + tid) * R + M + tid], yy, eps, tau, nullptr, nullptr);
    }
    if (tid == 0) {
        best_val[b] = (float)rv[0];
        best_idx[b] = code;
    }
}

// grid (ceil(T / 1024), B); 256 threads x 4 samples.  Thread n < N forms the set and the two coefficients of mixture n; then every thread sums the
// estimates of each set at its samples and stores the same value to every row of the set.
__global__ __launch_bounds__(256) void mixit_bwd_kernel(const float* __restrict__ est, const float* __restrict__ tgt, const double* __restrict__ gram,
                                                        const int64_t* __restrict__ best_idx, const float* __restrict__ gw, float* __restrict__ d_est,
                                                        const int M, const int N, const int T, const int kind, const double eps, const double tau) {
    __shared__ double G[MIXIT_MAX_R * MIXIT_MAX_R];
    __shared__ float cT[MIXIT_MAX_N], cE[MIXIT_MAX_N];
    __shared__ unsigned sets[MIXIT_MAX_N];
    const int b = blockIdx.y, tid = threadIdx.x, R = M + N;
    for (int e = tid; e < R * R; e += 256) G[e] = gram[(int64_t)b * R * R + e];
    __syncthreads();
    if (tid < N) {
        const int64_t idx = best_idx[b];
        const unsigned mask = mixit_set(idx < 0 || idx >= SEP_MIXIT_MAX_CODES ? 0 : (int)idx, M, N, tid);
        double a, yy, ct, ce;
        mixit_sums(G, R, M, tid, mask, a, yy);
        mixit_measure(kind, a, G[(M + tid) * R + M + tid], yy, eps, tau, &ct, &ce);
        const double g = (double)gw[b];
        sets[tid] = mask;
        cT[tid] = (float)(g * ct);
        cE[tid] = (float)(g * ce);
    }
    __syncthreads();
    const int64_t t0 = (int64_t)blockIdx.x * 1024 + tid;
    for (int n = 0; n < N; ++n) {
        const unsigned mask = sets[n];
        if (!mask) continue;                              // nothing is handed to this mixture: no row to write
        const float* x = tgt + ((int64_t)b * N + n) * T;
        float y[4] = {0.f, 0.f, 0.f, 0.f};
        for (int m = 0; m < M; ++m) {
            if (!((mask >> m) & 1u)) continue;
            const float* e = est + ((int64_t)b * M + m) * T;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int64_t t = t0 + k * 256;
                if (t < T) y[k] += e[t];
            }
        }
        const float ct = cT[n], ce = cE[n];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int64_t t = t0 + k * 256;
            y[k] = t < T ? fmaf(ct, x[t], ce * y[k]) : 0.f;
        }
        for (int m = 0; m < M; ++m) {
            if (!((mask >> m) & 1u)) continue;
            float* o = d_est + ((int64_t)b * M + m) * T;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int64_t t = t0 + k * 256;
                if (t < T) o[t] = y[k];
            }
        }
    }
}

static bool mixit_shape_ok(const int B, const int M, const int N, const int T) {
    return B >= 1 && B <= 65535 && M >= 1 && M <= MIXIT_MAX_M && N >= 1 && N <= MIXIT_MAX_N && T >= 1 && T <= BSS_MAX_T;
}
// N^M, or 0 beyond SEP_MIXIT_MAX_CODES
static int mixit_codes(const int M, const int N) {
    int64_t c = 1;
    for (int m = 0; m < M; ++m) {
        c *= N;
        if (c > SEP_MIXIT_MAX_CODES) return 0;
    }
    return (int)c;
}

}  // namespace

extern "C" size_t sep_mixit_scratch_bytes(int B, int M, int N, int T) {
    if (!mixit_shape_ok(B, M, N, T)) return 0;
    return sizeof(double) * (size_t)B * (size_t)bss_slabs(T, MIXIT_SLAB) * (size_t)((M + N) * (M + N));
}

extern "C" int sep_mixit_gram(const float* est, const float* tgt, double* gram, double* scratch, size_t scratch_bytes, int B, int M, int N, int T,
                              sep_stream_t stream) {
    SEP_REQUIRE(est && tgt && gram && scratch, "sep_mixit_gram: null pointer");
    SEP_REQUIRE(mixit_shape_ok(B, M, N, T), "sep_mixit_gram: bad arguments (B=%d M=%d N=%d T=%d; 1 <= B <= 65535, 1 <= M <= %d, 1 <= N <= %d, 1 <= T <= 2^30)", B,
                M, N, T, MIXIT_MAX_M, MIXIT_MAX_N);
    const size_t need = sep_mixit_scratch_bytes(B, M, N, T);
    SEP_REQUIRE(scratch_bytes >= need, "sep_mixit_gram: scratch holds %zu bytes, %zu needed", scratch_bytes, need);
    const int R = M + N, nslab = (int)bss_slabs(T, MIXIT_SLAB);
    const dim3 grid((unsigned)nslab, 1, (unsigned)B);
    if (R <= 4) {
        hipLaunchKernelGGL((mixit_gram_kernel<4, true>), grid, dim3(256), 0, (hipStream_t)stream, est, tgt, scratch, M, N, T, nslab);
    } else if (R <= 8) {
        hipLaunchKernelGGL((mixit_gram_kernel<8, true>), grid, dim3(256), 0, (hipStream_t)stream, est, tgt, scratch, M, N, T, nslab);
    } else if (R <= 12) {
        hipLaunchKernelGGL((mixit_gram_kernel<12, true>), grid, dim3(256), 0, (hipStream_t)stream, est, tgt, scratch, M, N, T, nslab);
    } else {
        const int nblk = ceil_div(R, MIXIT_GRAM_BLOCK);
        hipLaunchKernelGGL((mixit_gram_kernel<MIXIT_GRAM_BLOCK, false>), dim3((unsigned)nslab, (unsigned)(nblk * (nblk + 1) / 2), (unsigned)B), dim3(256), 0,
                           (hipStream_t)stream, est, tgt, scratch, M, N, T, nslab);
    }
    SEP_CHECK_LAUNCH("sep_mixit_gram");
    const int64_t total = (int64_t)B * R * R;
    hipLaunchKernelGGL(bss_reduce_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (const double*)scratch, gram, nslab, R * R, total);
    SEP_CHECK_LAUNCH("sep_mixit_gram (reduction)");
    return 0;
}

extern "C" int sep_mixit_search(const double* gram, int B, int M, int N, int kind, int maximize, int use_mean, double eps, double tau, float* best_val,
                                int64_t* best_idx, float* per_mix, sep_stream_t stream) {
    SEP_REQUIRE(gram && best_val && best_idx && per_mix, "sep_mixit_search: null pointer");
    SEP_REQUIRE(mixit_shape_ok(B, M, N, 1) && kind >= 0 && kind <= 2, "sep_mixit_search: bad arguments (B=%d M=%d N=%d kind=%d; 1 <= B <= 65535, 1 <= M <= %d, 1 <= N <= %d, kind 0 .. 2)",
                B, M, N, kind, MIXIT_MAX_M, MIXIT_MAX_N);
    const int ncodes = mixit_codes(M, N);
    SEP_REQUIRE(ncodes > 0, "sep_mixit_search: N^M = %d^%d exceeds %d assignments", N, M, SEP_MIXIT_MAX_CODES);
    hipLaunchKernelGGL(mixit_search_kernel, dim3((unsigned)B), dim3(256), 0, (hipStream_t)stream, gram, M, N, ncodes, kind, maximize, use_mean, eps, tau, best_val,
                       best_idx, per_mix);
    SEP_CHECK_LAUNCH("sep_mixit_search");
    return 0;
}

extern "C" int sep_mixit_bwd(const float* est, const float* tgt, const double* gram, const int64_t* best_idx, const float* gw, float* d_est, int B, int M,
                             int N, int T, int kind, double eps, double tau, sep_stream_t stream) {
    SEP_REQUIRE(est && tgt && gram && best_idx && gw && d_est, "sep_mixit_bwd: null pointer");
    SEP_REQUIRE(mixit_shape_ok(B, M, N, T) && kind >= 0 && kind <= 2,
                "sep_mixit_bwd: bad arguments (B=%d M=%d N=%d T=%d kind=%d; 1 <= B <= 65535, 1 <= M <= %d, 1 <= N <= %d, 1 <= T <= 2^30, kind 0 .. 2)", B, M, N, T, kind,
                MIXIT_MAX_M, MIXIT_MAX_N);
    hipLaunchKernelGGL(mixit_bwd_kernel, dim3((unsigned)ceil_div(T, 1024), (unsigned)B), dim3(256), 0, (hipStream_t)stream, est, tgt, gram, best_idx, gw, d_est, M,
                       N, T, kind, eps, tau);
    SEP_CHECK_LAUNCH("sep_mixit_bwd");
    return 0;
}

// ---- Optimal-permutation (Hungarian) training ---------------------------------------------------------------------------------------------
// The reference has no arithmetic to replace here: src/criterion/hungarian.py is a stub that raises NotImplementedError (it cites Dovrat,
// Nachmani and Wolf 2021).  PIT's table of n! permutations stops at about eight sources; the best permutation of an n x n pair matrix is a linear
// assignment problem, solved exactly in O(n^3).  sep_pair_gram makes ONE pass over the 2n waveforms into the three inner products behind every pair
// measure, sep_assign / sep_pair_assign solve the assignment with one wavefront per item, sep_pair_bwd applies the gradient of the chosen
// permutation.  The contract is in include/sepkernels.h.
namespace {

constexpr int PAIR_SLAB = SEP_PAIR_SLAB;        // samples behind one partial of sep_pair_gram: 8 per thread
constexpr int ASSIGN_MAX_N = SEP_ASSIGN_MAX_N;  // one lane per column: the wavefront width
static_assert(PAIR_SLAB % 256 == 0, "a slab is a whole number of 256-sample steps");
static_assert(ASSIGN_MAX_N == 64, "sep_assign gives every column a lane of one wavefront");

// part[b][slab][.] = the slab's share of dots (n n values, [i][j]), then of tt (n), then of xx (n).  grid (nslab, blocks of i x blocks of j, B).
// The workgroup owns estimates [RB bi, RB bi + RB) x targets [RB bj, RB bj + RB) as RB RB products in fp64 registers; the workgroups of the
// first block column also hold |est_i|^2, those of the first block row |tgt_j|^2.  Rows beyond n enter as zeros and are not stored.  Per
// thread the samples are added in ascending order, the wave by a butterfly (wave_fold, common.hpp), the four waves in order.
template <int RB>
__global__ __launch_bounds__(256) void pair_gram_kernel(const float* __restrict__ est, const float* __restrict__ tgt, double* __restrict__ part,
                                                        const int n, const int T, const int nslab) {
    constexpr int NACC = RB * RB + 2 * RB;
    __shared__ double red[4][NACC];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, slab = blockIdx.x, b = blockIdx.z;
    const int nblk = (n + RB - 1) / RB, bi = blockIdx.y / nblk, bj = blockIdx.y % nblk;
    const int ra = bi * RB, rb = bj * RB;
    const bool do_xx = bj == 0, do_tt = bi == 0;
    const float* pa[RB];
    const float* pb[RB];
#pragma unroll
    for (int i = 0; i < RB; ++i) {
        pa[i] = ra + i < n ? est + ((int64_t)b * n + ra + i) * T : nullptr;
        pb[i] = rb + i < n ? tgt + ((int64_t)b * n + rb + i) * T : nullptr;
    }
    double acc[NACC];
#pragma unroll
    for (int q = 0; q < NACC; ++q) acc[q] = 0.0;
    const int64_t t0 = (int64_t)slab * PAIR_SLAB;
#pragma unroll 2
    for (int k = 0; k < PAIR_SLAB / 256; ++k) {
        const int64_t t = t0 + k * 256 + tid;
        if (t < T) {
            double va[RB], vb[RB];
#pragma unroll
            for (int i = 0; i < RB; ++i) va[i] = pa[i] ? (double)pa[i][t] : 0.0;
#pragma unroll
            for (int i = 0; i < RB; ++i) vb[i] = pb[i] ? (double)pb[i][t] : 0.0;
#pragma unroll
            for (int i = 0; i < RB; ++i)
#pragma unroll
                for (int j = 0; j < RB; ++j) acc[i * RB + j] = fma(va[i], vb[j], acc[i * RB + j]);
            if (do_tt) {
#pragma unroll
                for (int j = 0; j < RB; ++j) acc[RB * RB + j] = fma(vb[j], vb[j], acc[RB * RB + j]);
            }
            if (do_xx) {
#pragma unroll
                for (int i = 0; i < RB; ++i) acc[RB * RB + RB + i] = fma(va[i], va[i], acc[RB * RB + RB + i]);
            }
        }
    }
    int base = 0;
    wave_fold<NACC, 32>(acc, lane, base);
    constexpr int LEFT = wave_fold_left(NACC), SHARED = wave_fold_shared(NACC);
    if ((lane & SHARED) == 0) {
#pragma unroll
        for (int q = 0; q < LEFT; ++q) red[w][base + q] = acc[q];
    }
    __syncthreads();
    double* P = part + ((int64_t)b * nslab + slab) * ((int64_t)n * n + 2 * n);
    for (int q = tid; q < NACC; q += 256) {
        const double s = ((red[0][q] + red[1][q]) + red[2][q]) + red[3][q];
        if (q < RB * RB) {
            const int gi = ra + q / RB, gj = rb + q % RB;
            if (gi < n && gj < n) P[gi * n + gj] = s;
        } else if (q < RB * RB + RB) {
            const int gj = rb + q - RB * RB;
            if (do_tt && gj < n) P[n * n + gj] = s;
        } else {
            const int gi = ra + q - RB * RB - RB;
            if (do_xx && gi < n) P[n * n + n + gi] = s;
        }
    }
}

// dots / tt / xx = the slab partials added in ascending slab order; one thread per output value
__global__ __launch_bounds__(256) void pair_reduce_kernel(const double* __restrict__ part, double* __restrict__ dots, double* __restrict__ tt,
                                                          double* __restrict__ xx, const int n, const int nslab, const int64_t total) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= total) return;
    const int inner = n * n + 2 * n;
    const int64_t b = e / inner;
    const int r = (int)(e % inner);
    double s = 0.0;
    for (int sl = 0; sl < nslab; ++sl) s += part[(b * nslab + sl) * inner + r];
    if (r < n * n) dots[b * n * n + r] = s;
    else if (r < n * n + n) tt[b * n + r - n * n] = s;
    else xx[b * n + r - n * n - n] = s;
}

// The minimum-cost perfect matching of the n x n matrix C (LDS, row pitch n) by shortest augmenting paths with potentials (Jonker-Volgenant;
// the O(n^3) Hungarian method), run by ONE wavefront: lane j owns column j (v_j, the row matched to it, minv, way, used) and row j (u_j and
// whether the row is in the alternating tree).  Every value that steers the control flow (i0, j0, j1, delta) is the same in all lanes, so
// every lane reaches every shuffle.  Returns the row matched to this lane's column (-1 for lane >= n), u and v of the lane's row / column.
// Termination and the range of every index hold for ANY bit pattern in C: the row loop runs n times; an augmentation marks one more unused
// column per step, only matched columns are ever marked and fewer than n are matched, so a free column is reached within n steps (the loop
// allows n + 1); the columns offered to the minimum are the unused ones only, one whose minv does not compare (NaN) offers +inf with its own
// index and the lowest index wins among equals, so some unused column below n is always chosen; `way` of a column names a column marked
// strictly before it (or -1, the root), so the walk back takes at most n steps.
__device__ __forceinline__ int assign_solve(const double* C, const int n, const int lane, double& u_out, double& v_out) {
    const double INF = HUGE_VAL;
    double u = 0.0, v = 0.0;
    int p = -1;                                        // the row matched to column `lane`
    for (int i = 0; i < n; ++i) {
        double minv = INF;
        int way = -1, j0 = -1, i0 = i;
        bool used = false, in_tree = false;
        for (int step = 0; step <= n; ++step) {
            if (lane == i0) in_tree = true;
            const double ui0 = __shfl(u, i0, 64);
            const bool open = lane < n && !used;
            if (open) {
                const double cur = C[i0 * n + lane] - ui0 - v;
                if (cur < minv) { minv = cur; way = j0; }
            }
            double bv = (open && minv == minv) ? minv : INF;      // (value, column) of the least minv among the unused columns
            int bc = open ? lane : ASSIGN_MAX_N;
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                const double ov = __shfl_xor(bv, o, 64);
                const int oc = __shfl_xor(bc, o, 64);
                if (ov < bv || (ov == bv && oc < bc)) { bv = ov; bc = oc; }
            }
            const int j1 = bc < n ? bc : n - 1;
            const double delta = bv;
            if (in_tree) u += delta;
            if (used) v -= delta;
            else minv -= delta;
            j0 = j1;
            if (lane == j0) used = true;
            i0 = __shfl(p, j0, 64);
            if (i0 < 0) break;                                     // a free column: the path is complete
        }
        for (int step = 0; step < n; ++step) {                     // walk back to the root, moving every row of the path one column on
            const int j1 = __shfl(way, j0, 64);
            const int moved = __shfl(p, j1 < 0 ? 0 : j1, 64);
            if (lane == j0) p = j1 < 0 ? i : moved;
            j0 = j1;
            if (j0 < 0) break;
        }
    }
    u_out = u;
    v_out = v;
    return lane < n ? p : -1;
}

// one wavefront per item
__global__ __launch_bounds__(64) void assign_kernel(const double* __restrict__ cost, const int n, const int maximize, int64_t* __restrict__ perm,
                                                    double* __restrict__ total, double* __restrict__ duals) {
    __shared__ double C[ASSIGN_MAX_N * ASSIGN_MAX_N];
    __shared__ int col_of[ASSIGN_MAX_N];
    const int b = blockIdx.x, lane = threadIdx.x;
    const double* src = cost + (int64_t)b * n * n;
    for (int e = lane; e < n * n; e += 64) C[e] = maximize ? -src[e] : src[e];
    __syncthreads();
    double u, v;
    const int row = assign_solve(C, n, lane, u, v);
    if (lane < n) {
        col_of[row] = lane;
        duals[(int64_t)b * 2 * n + lane] = u;
        duals[(int64_t)b * 2 * n + n + lane] = v;
    }
    __syncthreads();
    if (lane < n) perm[(int64_t)b * n + lane] = col_of[lane];
    if (lane == 0) {
        double s = 0.0;
        for (int i = 0; i < n; ++i) s += C[i * n + col_of[i]];
        total[b] = maximize ? -s : s;
    }
}

// one wavefront per item: the pair measures into LDS (negated for a maximum), the same solver, the chosen measures again from the inner products
__global__ __launch_bounds__(64) void pair_assign_kernel(const double* __restrict__ dots, const double* __restrict__ tt, const double* __restrict__ xx,
                                                         const int n, const int kind, const int maximize, const int use_mean, const double eps,
                                                         const double tau, float* __restrict__ best_val, int64_t* __restrict__ perm,
                                                         float* __restrict__ per_src, double* __restrict__ duals) {
    __shared__ double C[ASSIGN_MAX_N * ASSIGN_MAX_N];
    __shared__ double chosen[ASSIGN_MAX_N];
    __shared__ int col_of[ASSIGN_MAX_N];
    const int b = blockIdx.x, lane = threadIdx.x;
    const double* D = dots + (int64_t)b * n * n;
    for (int e = lane; e < n * n; e += 64) {
        const double m = mixit_measure(kind, D[e], tt[(int64_t)b * n + e % n], xx[(int64_t)b * n + e / n], eps, tau, nullptr, nullptr);
        C[e] = maximize ? -m : m;
    }
    __syncthreads();
    double u, v;
    const int row = assign_solve(C, n, lane, u, v);
    if (lane < n) {
        col_of[row] = lane;
        if (duals) {
            duals[(int64_t)b * 2 * n + lane] = u;
            duals[(int64_t)b * 2 * n + n + lane] = v;
        }
    }
    __syncthreads();
    if (lane < n) {
        const int j = col_of[lane];
        const double m = mixit_measure(kind, D[lane * n + j], tt[(int64_t)b * n + j], xx[(int64_t)b * n + lane], eps, tau, nullptr, nullptr);
        chosen[lane] = m;
        perm[(int64_t)b * n + lane] = j;
        per_src[(int64_t)b * n + lane] = (float)m;
    }
    __syncthreads();
    if (lane == 0) {
        double s = 0.0;
        for (int i = 0; i < n; ++i) s += chosen[i];
        best_val[b] = (float)(use_mean ? s / (double)n : s);
    }
}

// grid (ceil(T / 1024), n, B); 256 threads x 4 samples: estimate i against the target its permutation names
__global__ __launch_bounds__(256) void pair_bwd_kernel(const float* __restrict__ est, const float* __restrict__ tgt, const double* __restrict__ dots,
                                                       const double* __restrict__ tt, const double* __restrict__ xx, const int64_t* __restrict__ perm,
                                                       const float* __restrict__ gw, float* __restrict__ d_est, const int n, const int T, const int kind,
                                                       const double eps, const double tau) {
    __shared__ float coef[2];
    __shared__ int col;
    const int b = blockIdx.z, i = blockIdx.y, tid = threadIdx.x;
    if (tid == 0) {
        const int64_t pj = perm[(int64_t)b * n + i];
        const int j = pj < 0 || pj >= n ? 0 : (int)pj;
        double ct, ce;
        mixit_measure(kind, dots[((int64_t)b * n + i) * n + j], tt[(int64_t)b * n + j], xx[(int64_t)b * n + i], eps, tau, &ct, &ce);
        const double g = (double)gw[b];
        coef[0] = (float)(g * ct);
        coef[1] = (float)(g * ce);
        col = j;
    }
    __syncthreads();
    const float ct = coef[0], ce = coef[1];
    const float* e = est + ((int64_t)b * n + i) * T;
    const float* x = tgt + ((int64_t)b * n + col) * T;
    float* o = d_est + ((int64_t)b * n + i) * T;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int64_t t = (int64_t)blockIdx.x * 1024 + k * 256 + tid;
        if (t < T) o[t] = fmaf(ct, x[t], ce * e[t]);
    }
}

static bool pair_shape_ok(const int B, const int n, const int T) { return B >= 1 && B <= 65535 && n >= 1 && n <= ASSIGN_MAX_N && T >= 1; }

}  // namespace

extern "C" size_t sep_pair_gram_scratch_bytes(int B, int n, int T) {
    if (!pair_shape_ok(B, n, T)) return 0;
    return sizeof(double) * (size_t)B * (size_t)bss_slabs(T, PAIR_SLAB) * (size_t)(n * n + 2 * n);
}

extern "C" int sep_pair_gram(const float* est, const float* tgt, double* dots, double* tt, double* xx, double* scratch, size_t scratch_bytes, int B, int n,
                             int T, sep_stream_t stream) {
    SEP_REQUIRE(est && tgt && dots && tt && xx && scratch, "sep_pair_gram: null pointer");
    SEP_REQUIRE(pair_shape_ok(B, n, T), "sep_pair_gram: bad arguments (B=%d n=%d T=%d; 1 <= B <= 65535, 1 <= n <= %d, T >= 1)", B, n, T, ASSIGN_MAX_N);
    const size_t need = sep_pair_gram_scratch_bytes(B, n, T);
    SEP_REQUIRE(scratch_bytes >= need, "sep_pair_gram: scratch holds %zu bytes, %zu needed", scratch_bytes, need);
    const int nslab = (int)bss_slabs(T, PAIR_SLAB);
    if (n <= 4) {
        hipLaunchKernelGGL((pair_gram_kernel<4>), dim3((unsigned)nslab, 1, (unsigned)B), dim3(256), 0, (hipStream_t)stream, est, tgt, scratch, n, T, nslab);
    } else {
        const int nblk = ceil_div(n, 8);
        hipLaunchKernelGGL((pair_gram_kernel<8>), dim3((unsigned)nslab, (unsigned)(nblk * nblk), (unsigned)B), dim3(256), 0, (hipStream_t)stream, est, tgt,
                           scratch, n, T, nslab);
    }
    SEP_CHECK_LAUNCH("sep_pair_gram");
    const int64_t total = (int64_t)B * (n * n + 2 * n);
    hipLaunchKernelGGL(pair_reduce_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (const double*)scratch, dots, tt, xx, n, nslab,
                       total);
    SEP_CHECK_LAUNCH("sep_pair_gram (reduction)");
    return 0;
}

extern "C" int sep_assign(const double* cost, int B, int n, int maximize, int64_t* perm, double* total, double* duals, sep_stream_t stream) {
    SEP_REQUIRE(cost && perm && total && duals, "sep_assign: null pointer");
    SEP_REQUIRE(B >= 1 && n >= 1 && n <= ASSIGN_MAX_N, "sep_assign: bad arguments (B=%d n=%d; B >= 1, 1 <= n <= %d)", B, n, ASSIGN_MAX_N);
    hipLaunchKernelGGL(assign_kernel, dim3((unsigned)B), dim3(64), 0, (hipStream_t)stream, cost, n, maximize, perm, total, duals);
    SEP_CHECK_LAUNCH("sep_assign");
    return 0;
}

extern "C" int sep_pair_assign(const double* dots, const double* tt, const double* xx, int B, int n, int kind, int maximize, int use_mean, double eps,
                               double tau, float* best_val, int64_t* perm, float* per_src, double* duals, sep_stream_t stream) {
    SEP_REQUIRE(dots && tt && xx && best_val && perm && per_src, "sep_pair_assign: null pointer");
    SEP_REQUIRE(B >= 1 && n >= 1 && n <= ASSIGN_MAX_N && kind >= 0 && kind <= 2, "sep_pair_assign: bad arguments (B=%d n=%d kind=%d; B >= 1, 1 <= n <= %d, kind 0 .. 2)",
                B, n, kind, ASSIGN_MAX_N);
    hipLaunchKernelGGL(pair_assign_kernel, dim3((unsigned)B), dim3(64), 0, (hipStream_t)stream, dots, tt, xx, n, kind, maximize, use_mean, eps, tau, best_val, perm,
                       per_src, duals);
    SEP_CHECK_LAUNCH("sep_pair_assign");
    return 0;
}

extern "C" int sep_pair_bwd(const float* est, const float* tgt, const double* dots, const double* tt, const double* xx, const int64_t* perm, const float* gw,
                            float* d_est, int B, int n, int T, int kind, double eps, double tau, sep_stream_t stream) {
    SEP_REQUIRE(est && tgt && dots && tt && xx && perm && gw && d_est, "sep_pair_bwd: null pointer");
    SEP_REQUIRE(pair_shape_ok(B, n, T) && kind >= 0 && kind <= 2, "sep_pair_bwd: bad arguments (B=%d n=%d T=%d kind=%d; 1 <= B <= 65535, 1 <= n <= %d, T >= 1, kind 0 .. 2)",
                B, n, T, kind, ASSIGN_MAX_N);
    hipLaunchKernelGGL(pair_bwd_kernel, dim3((unsigned)(((int64_t)T + 1023) / 1024), (unsigned)n, (unsigned)B), dim3(256), 0, (hipStream_t)stream, est, tgt, dots, tt,
                       xx, perm, gw, d_est, n, T, kind, eps, tau);
    SEP_CHECK_LAUNCH("sep_pair_bwd");
    return 0;
}
