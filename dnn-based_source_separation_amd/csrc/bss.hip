// BSS-eval on the device for gfx950: the O(T flen) passes of v3 ("sources": SDR / SIR / SAR of mir_eval) and of v4 ("images": museval's framewise
// SDR / ISR / SIR / SAR), and bss_reduce_kernel, the deterministic second stage they and mixit.hip's Gram pass share.  The reference arithmetic
// each half replaces is named at its section (paths under the reference's root).  The contract is in include/sepkernels.h.
//
// Called by utils/bss.py (the filters' dense solves between the passes are that module's).
#include "loss_common.hpp"

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

__device__ __forceinline__ int bss_row_length(const int32_t* lengths, const int b, const int T) {
    if (!lengths) return T;
    const int v = lengths[b];
    return v < 0 ? 0 : (v > T ? T : v);
}

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
    const int64_t nslab = slab_count(T, BSS_XC_SLAB), ntile = slab_count(nlag, BSS_TILE);
    int64_t need = (int64_t)B * n * m;                                  // (< 2^32 once the grid limits hold)
    if ((int64_t)n * m > 65535 || B > 65535 || nslab * ntile > 0x7fffffff) return -1;
    if (((int64_t)B * n * m * nlag + 255) / 256 > 0x7fffffff) return -1;   // the grid of the reduction
    if (__builtin_mul_overflow(need, nslab * nlag, &need) || need > (int64_t)1 << 56) return -1;
    return need;
}
static int64_t bss_energies_scratch(const int B, const int n, const int m, const int T, const int flen) {
    const int64_t nslab = slab_count((int64_t)T + flen - 1, BSS_EN_SLAB);
    if ((int64_t)n * m > 65535 || B > 65535) return -1;
    return (int64_t)B * n * m * nslab * 5;
}
static bool bss_shape_ok(const int B, const int n, const int m, const int T) { return B >= 1 && n >= 1 && m >= 1 && T >= 1 && T <= BSS_MAX_T; }

}  // namespace

// the launch of the second stage for sep_mixit_gram (mixit.hip; declared in loss_common.hpp)
void sep_bss_reduce(const double* part, double* out, int nslab, int inner, int64_t total, hipStream_t stream) {
    hipLaunchKernelGGL(bss_reduce_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, part, out, nslab, inner, total);
}

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
    const int nslab = (int)slab_count(T, BSS_XC_SLAB), ntile = (int)slab_count(nlag, BSS_TILE);
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
    const int nslab = (int)slab_count((int64_t)T + flen - 1, BSS_EN_SLAB);
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
    const int64_t nslab = slab_count((int64_t)window + flen - 1, BSS_IM_SLAB);
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
    const int nslab = (int)slab_count((int64_t)window + flen - 1, BSS_IM_SLAB);
    hipLaunchKernelGGL(bss_image_energies_kernel, dim3((unsigned)nslab, (unsigned)(n * nwin), (unsigned)B), dim3(256), 0, (hipStream_t)stream, ref, est,
                       filt_all, filt_one, scratch, lengths, n, C, T, flen, window, hop, nwin, nslab);
    SEP_CHECK_LAUNCH("sep_bss_image_energies");
    const int64_t total = (int64_t)B * n * nwin * BSS_IM_SUMS;
    hipLaunchKernelGGL(bss_reduce_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (const double*)scratch, out, nslab,
                       BSS_IM_SUMS, total);
    SEP_CHECK_LAUNCH("sep_bss_image_energies (reduction)");
    return 0;
}
