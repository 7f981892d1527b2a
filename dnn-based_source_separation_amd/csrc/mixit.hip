// Mixture invariant training (MixIT) for gfx950.
// The reference has no arithmetic to replace here: src/criterion/mixit.py is a stub that raises NotImplementedError.  The criterion is the one
// of Wisdom et al. 2020: the best of the N^M ways to hand each of M estimates to one of N reference mixtures.  Every measure this library
// knows is a function of <x_n, x_n>, <x_n, y_n> and <y_n, y_n>, and for a remix y_n = sum_{m in set} s_m those are sums of entries of the Gram
// matrix of the M + N rows: one pass over the waveforms gives the value of every assignment (sep_mixit_gram, sep_mixit_search), one more
// pass the gradient of the chosen one (sep_mixit_bwd).  The contract is in include/sepkernels.h.
//
// The measure (pair_measure) is loss_common.hpp's; the slabs of the Gram pass are added by bss.hip's second stage (sep_bss_reduce).
// Called by criterion/mixit.py.
#include "loss_common.hpp"

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
            s += pair_measure(kind, a, G[(M + n) * R + M + n], yy, eps, tau, nullptr, nullptr);
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
        per_mix[(int64_t)b * N + tid] = (float)pair_measure(kind, a, G[(M + tid) * R + M + tid], yy, eps, tau, nullptr, nullptr);
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
        pair_measure(kind, a, G[(M + tid) * R + M + tid], yy, eps, tau, &ct, &ce);
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
    return sizeof(double) * (size_t)B * (size_t)slab_count(T, MIXIT_SLAB) * (size_t)((M + N) * (M + N));
}

extern "C" int sep_mixit_gram(const float* est, const float* tgt, double* gram, double* scratch, size_t scratch_bytes, int B, int M, int N, int T,
                              sep_stream_t stream) {
    SEP_REQUIRE(est && tgt && gram && scratch, "sep_mixit_gram: null pointer");
    SEP_REQUIRE(mixit_shape_ok(B, M, N, T), "sep_mixit_gram: bad arguments (B=%d M=%d N=%d T=%d; 1 <= B <= 65535, 1 <= M <= %d, 1 <= N <= %d, 1 <= T <= 2^30)", B,
                M, N, T, MIXIT_MAX_M, MIXIT_MAX_N);
    const size_t need = sep_mixit_scratch_bytes(B, M, N, T);
    SEP_REQUIRE(scratch_bytes >= need, "sep_mixit_gram: scratch holds %zu bytes, %zu needed", scratch_bytes, need);
    const int R = M + N, nslab = (int)slab_count(T, MIXIT_SLAB);
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
    sep_bss_reduce((const double*)scratch, gram, nslab, R * R, total, (hipStream_t)stream);
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
