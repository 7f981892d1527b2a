// Optimal-permutation (Hungarian) training and the linear assignment solver for gfx950.
// The reference has no arithmetic to replace here: src/criterion/hungarian.py is a stub that raises NotImplementedError (it cites Dovrat,
// Nachmani and Wolf 2021).  PIT's table of n! permutations stops at about eight sources; the best permutation of an n x n pair matrix is a linear
// assignment problem, solved exactly in O(n^3).  sep_pair_gram makes ONE pass over the 2n waveforms into the three inner products behind every pair
// measure, sep_assign / sep_pair_assign solve the assignment with one wavefront per item, sep_pair_bwd applies the gradient of the chosen
// permutation.  The contract is in include/sepkernels.h.
//
// The measure (pair_measure) is loss_common.hpp's.  Called by criterion/hungarian.py; sep_assign also by sepkernels/longform.py, whose
// windows' permutations stitch.hip chains.
#include "loss_common.hpp"

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
        const double m = pair_measure(kind, D[e], tt[(int64_t)b * n + e % n], xx[(int64_t)b * n + e / n], eps, tau, nullptr, nullptr);
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
        const double m = pair_measure(kind, D[lane * n + j], tt[(int64_t)b * n + j], xx[(int64_t)b * n + lane], eps, tau, nullptr, nullptr);
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
        pair_measure(kind, dots[((int64_t)b * n + i) * n + j], tt[(int64_t)b * n + j], xx[(int64_t)b * n + i], eps, tau, &ct, &ce);
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
    return sizeof(double) * (size_t)B * (size_t)slab_count(T, PAIR_SLAB) * (size_t)(n * n + 2 * n);
}

extern "C" int sep_pair_gram(const float* est, const float* tgt, double* dots, double* tt, double* xx, double* scratch, size_t scratch_bytes, int B, int n,
                             int T, sep_stream_t stream) {
    SEP_REQUIRE(est && tgt && dots && tt && xx && scratch, "sep_pair_gram: null pointer");
    SEP_REQUIRE(pair_shape_ok(B, n, T), "sep_pair_gram: bad arguments (B=%d n=%d T=%d; 1 <= B <= 65535, 1 <= n <= %d, T >= 1)", B, n, T, ASSIGN_MAX_N);
    const size_t need = sep_pair_gram_scratch_bytes(B, n, T);
    SEP_REQUIRE(scratch_bytes >= need, "sep_pair_gram: scratch holds %zu bytes, %zu needed", scratch_bytes, need);
    const int nslab = (int)slab_count(T, PAIR_SLAB);
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
