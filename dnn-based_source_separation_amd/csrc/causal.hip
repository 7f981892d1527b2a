// The causal TCN layer's first norm folded into its depthwise convolution (ABI 23, additive).
//
// Per layer the staged causal path (models/conv_tasnet.py::_run_staged; reference src/models/tdcn.py:107-147) ran
//     a = W1 x + b1  ->  v1 = cLN(PReLU(a))  ->  z = depthwise(pad(v1))  ->  v2 = cLN(PReLU(z))  ->  heads
// with v1 -- an H-wide tensor whose only reader is the depthwise convolution -- written and read back through HBM.  Here the norm's two
// per-frame statistics are all that is stored (sep_cln_stats: (B, ldt) each), and the depthwise kernels form v1 on load:
//     v1[b][c][t'] = gamma[c] (PReLU(a[b][c][t']; alpha) - mean[b][t']) rstd[b][t'] + beta[c]      0 <= t' < T, ZERO outside
// (the reference pads AFTER the norm: the zeros in front of the row are zeros of v1, not of a).  sep_depthwise_cln_fwd is the
// forward, sep_depthwise_cln_bwd_weight the weight / bias gradient with the same prologue on its x operand; the input gradient needs
// nothing new (sep_depthwise_bwd_input yields d v1, sep_cln_bwd takes a, mean, rstd and alpha).
//
// Also here: sep_sum_f64, the fp64-accumulating sum that turns the B * C row partials of a PReLU slope's gradient into the slope's -- the
// recorded causal step's replacement for torch's `pa.sum(dtype=float64)`.
//
// sep_cln_stats itself lives in cln.hip: it is sep_cln_fwd's own kernels without the apply pass (one source, bit-identical statistics).
//
// Also here: sep_unfold_dilated / sep_fold_dilated, the dilated unfold (im2col over the taps) of a (B, C, ldt) activation and its adjoint, for
// the causal layers with FULL k-tap convolutions (separable=False: reference src/models/tdcn.py:100-147).  With the unfolded row index
// c * P + p a layer's nn.Conv1d(H, M, P, dilation=d) weight (M, H, P) is, in place, the (M, H P) matrix of a 1x1 product over the unfolded
// rows, so the two convolutions of a layer, their input gradient and their weight gradients are the products the separable layers run.
// Streaming kernels: a lane owns four consecutive frames of a row, reads them for every tap as one or two aligned 16-byte loads (the
// tap's shift modulo four is uniform over the launch, so the pick of four out of eight is a uniform switch), masks with selects (what
// lies beyond T may be NaN) and stores 16 bytes.  One writer per output element, no atomics.
//
// One (b, c) row per workgroup, as the depthwise row kernels of depthwise.hip: the normalised row is formed ONCE into LDS (float4 loads of
// a, mean, rstd), the taps then read LDS -- float4 where every tap shift is a multiple of four frames (d % 4 == 0), one frame per lane
// (conflict-free) otherwise.  Any kernel width, any dilation >= 1, 0 <= pad <= (Kw - 1) d; three taps are unrolled.  Rows that do not
// fit the LDS take the same kernels with the prologue evaluated per tap from global memory.  Plain loads and vector stores, no atomics:
// results are bit-stable run to run.
#include "common.hpp"
#include <stdlib.h>

namespace {

constexpr size_t CD_LDS_ROW_BYTES = 64 * 1024;      // the staged row: up to 16384 frames

struct CdRow {
    const float* x;       // the row of a: (b, c)
    const float* mean;    // the sample's statistics: (b)
    const float* rstd;
    float al, ga, be;
    bool act;
    int T;
};

// v1 at frame i of the row, formed from global memory (zero outside [0, T))
__device__ __forceinline__ float cd_v1(const CdRow& r, const int i) {
    if (i < 0 || i >= r.T) return 0.f;
    const float xv = r.x[i];
    const float u = r.act ? prelu_f(xv, r.al) : xv;
    return (u - r.mean[i]) * r.rstd[i] * r.ga + r.be;
}

// the whole normalised row into LDS: frames [0, ldt), zeros from T on
__device__ __forceinline__ void cd_stage_row(const CdRow& r, float* rowbuf, const int ldt) {
    for (int t = 4 * threadIdx.x; t < ldt; t += 1024) {
        const float4 xv = ld4(r.x + t), m4 = ld4(r.mean + t), r4 = ld4(r.rstd + t);
        const float xs[4] = {xv.x, xv.y, xv.z, xv.w}, ms[4] = {m4.x, m4.y, m4.z, m4.w}, rs[4] = {r4.x, r4.y, r4.z, r4.w};
        float o[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float u = r.act ? prelu_f(xs[e], r.al) : xs[e];
            o[e] = t + e < r.T ? (u - ms[e]) * rs[e] * r.ga + r.be : 0.f;
        }
        st4(rowbuf + t, make_float4(o[0], o[1], o[2], o[3]));
    }
}

__device__ __forceinline__ CdRow cd_row(const float* x, const float* alpha, const float* gamma, const float* beta, const float* mean, const float* rstd,
                                        const int row, const int C, const int T, const int ldt) {
    const int b = row / C, c = row % C;
    CdRow r;
    r.x = x + (size_t)row * ldt;
    r.mean = mean + (size_t)b * ldt;
    r.rstd = rstd + (size_t)b * ldt;
    r.act = alpha != nullptr;
    r.al = r.act ? alpha[0] : 1.f;
    r.ga = gamma[c];
    r.be = beta[c];
    r.T = T;
    return r;
}

// y[t] = bias + sum_k w[k] v1[t + k d - pad] for t < T, zero for T <= t < ldt.     KW: 3 = unrolled taps, 0 = Kw taps in a loop
template <int KW, bool STAGED>
__global__ __launch_bounds__(256) void cd_depthwise_fwd_kernel(const float* __restrict__ x, const float* __restrict__ alpha, const float* __restrict__ gamma,
                                                               const float* __restrict__ beta, const float* __restrict__ mean, const float* __restrict__ rstd,
                                                               const float* __restrict__ w, const float* __restrict__ bias, float* __restrict__ y,
                                                               int C, int T, int ldt, int Kw_, int pad, int dil) {
    extern __shared__ __attribute__((aligned(16))) float rowbuf[];
    const int Kw = KW ? KW : Kw_;
    const int row = blockIdx.x, c = row % C;
    const CdRow r = cd_row(x, alpha, gamma, beta, mean, rstd, row, C, T, ldt);
    float* yr = y + (size_t)row * ldt;
    const float* wr = w + (size_t)c * Kw;
    const float bb = bias ? bias[c] : 0.f;
    if (STAGED) {
        cd_stage_row(r, rowbuf, ldt);
        __syncthreads();
    }
    if (STAGED && ((pad | dil) & 3) == 0) {
        // every tap shift is a multiple of four frames: a lane's four outputs read whole float4s of the staged row
        for (int t = 4 * threadIdx.x; t < ldt; t += 1024) {
            float o[4] = {bb, bb, bb, bb};
            for (int k = 0; k < Kw; ++k) {          // (Kw is a constant in the three-tap instance: unrolled)
                const int i = t + k * dil - pad;
                if (i < 0 || i >= ldt) continue;
                const float4 v = ld4(rowbuf + i);
                const float wk = wr[k];
                o[0] = fmaf(wk, v.x, o[0]); o[1] = fmaf(wk, v.y, o[1]); o[2] = fmaf(wk, v.z, o[2]); o[3] = fmaf(wk, v.w, o[3]);
            }
            st4(yr + t, make_float4(t < T ? o[0] : 0.f, t + 1 < T ? o[1] : 0.f, t + 2 < T ? o[2] : 0.f, t + 3 < T ? o[3] : 0.f));
        }
        return;
    }
    // one frame per lane: consecutive lanes read consecutive LDS words whatever the shift
    for (int t = threadIdx.x; t < ldt; t += 256) {
        float o = bb;
        for (int k = 0; k < Kw; ++k) {
            const int i = t + k * dil - pad;
            const float v = STAGED ? ((i >= 0 && i < ldt) ? rowbuf[i] : 0.f) : cd_v1(r, i);
            o = fmaf(wr[k], v, o);
        }
        yr[t] = t < T ? o : 0.f;
    }
}

// partial[row][k] = sum_{t < T} dy[t] v1[t + k d - pad] (k < Kw), partial[row][Kw] = sum_{t < T} dy[t]; fixed summation order
template <int KW, bool STAGED>
__global__ __launch_bounds__(256) void cd_depthwise_wgrad_kernel(const float* __restrict__ dy, const float* __restrict__ x, const float* __restrict__ alpha,
                                                                 const float* __restrict__ gamma, const float* __restrict__ beta, const float* __restrict__ mean,
                                                                 const float* __restrict__ rstd, float* __restrict__ partial, int C, int T, int ldt, int Kw_,
                                                                 int pad, int dil) {
    extern __shared__ __attribute__((aligned(16))) float rowbuf[];
    __shared__ float red[4][4];
    const int Kw = KW ? KW : Kw_;
    const int row = blockIdx.x;
    const CdRow r = cd_row(x, alpha, gamma, beta, mean, rstd, row, C, T, ldt);
    const float* gr = dy + (size_t)row * ldt;
    float* pr = partial + (size_t)row * (Kw + 1);
    if (STAGED) {
        cd_stage_row(r, rowbuf, ldt);
        __syncthreads();
    }
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    if (KW == 3) {
        float q0 = 0.f, q1 = 0.f, q2 = 0.f, q3 = 0.f;
        for (int t = threadIdx.x; t < T; t += 256) {
            const float g = gr[t];
            const int i0 = t - pad, i1 = i0 + dil, i2 = i1 + dil;
            q0 = fmaf(g, STAGED ? ((i0 >= 0 && i0 < ldt) ? rowbuf[i0] : 0.f) : cd_v1(r, i0), q0);
            q1 = fmaf(g, STAGED ? ((i1 >= 0 && i1 < ldt) ? rowbuf[i1] : 0.f) : cd_v1(r, i1), q1);
            q2 = fmaf(g, STAGED ? ((i2 >= 0 && i2 < ldt) ? rowbuf[i2] : 0.f) : cd_v1(r, i2), q2);
            q3 += g;
        }
        q0 = wave_sum(q0); q1 = wave_sum(q1); q2 = wave_sum(q2); q3 = wave_sum(q3);
        if (lane == 0) { red[wv][0] = q0; red[wv][1] = q1; red[wv][2] = q2; red[wv][3] = q3; }
        __syncthreads();
        if (threadIdx.x < 4) pr[threadIdx.x] = (red[0][threadIdx.x] + red[1][threadIdx.x]) + (red[2][threadIdx.x] + red[3][threadIdx.x]);
        return;
    }
    for (int k = 0; k <= Kw; ++k) {
        float acc = 0.f;
        for (int t = threadIdx.x; t < T; t += 256) {
            const float g = gr[t];
            if (k == Kw) {
                acc += g;
            } else {
                const int i = t + k * dil - pad;
                acc = fmaf(g, STAGED ? ((i >= 0 && i < ldt) ? rowbuf[i] : 0.f) : cd_v1(r, i), acc);
            }
        }
        const float tot = block_sum_256<float>(acc, &red[0][0]);
        if (threadIdx.x == 0) pr[k] = tot;
    }
}

// out[0] = sum of n floats, accumulated in fp64 in a fixed order by one workgroup
__global__ __launch_bounds__(256) void cd_sum_f64_kernel(const float* __restrict__ x, const int64_t n, float* __restrict__ out) {
    __shared__ double red[4];
    double acc = 0.0;
    for (int64_t i = threadIdx.x; i < n; i += 256) acc += (double)x[i];
    const double tot = block_sum_256<double>(acc, red);
    if (threadIdx.x == 0) out[0] = (float)tot;
}

// frames [i, i + 4) of a row of ldt floats (ldt % 4 == 0), i of any sign and alignment, as aligned 16-byte loads; r = i & 3 is uniform over
// the launch.  Quads that are not wholly inside [0, ldt) read as zero: their frames are outside [0, T) and masked by the caller anyway.
__device__ __forceinline__ float4 ud_quad(const float* __restrict__ row, const int q, const int ldt) {
    return (q >= 0 && q + 4 <= ldt) ? ld4(row + q) : make_float4(0.f, 0.f, 0.f, 0.f);
}
__device__ __forceinline__ float4 ud_window(const float* __restrict__ row, const int i, const int ldt) {
    const int r = i & 3, q = i - r;
    const float4 a = ud_quad(row, q, ldt);
    if (r == 0) return a;
    const float4 b = ud_quad(row, q + 4, ldt);
    if (r == 1) return make_float4(a.y, a.z, a.w, b.x);
    if (r == 2) return make_float4(a.z, a.w, b.x, b.y);
    return make_float4(a.w, b.x, b.y, b.z);
}
// the four frames kept where both the destination frame t + e and the source frame i + e lie in [0, T), zero elsewhere (selects: no NaN passes)
__device__ __forceinline__ float4 ud_mask(const float4 v, const int t, const int i, const int T) {
    float4 o;
    o.x = (t < T && i >= 0 && i < T) ? v.x : 0.f;
    o.y = (t + 1 < T && i + 1 >= 0 && i + 1 < T) ? v.y : 0.f;
    o.z = (t + 2 < T && i + 2 >= 0 && i + 2 < T) ? v.z : 0.f;
    o.w = (t + 3 < T && i + 3 >= 0 && i + 3 < T) ? v.w : 0.f;
    return o;
}

// cols[row P + p][t] = x[row][t + p dil - pad] where both frames are in [0, T), zero elsewhere (all of [T, ldt) included).  grid (rows, frame tiles of 1024)
__global__ __launch_bounds__(256) void ud_unfold_kernel(const float* __restrict__ x, float* __restrict__ cols, int T, int ldt, int P, int dil, int pad) {
    const int64_t row = blockIdx.x;
    const int t = 4 * (blockIdx.y * 256 + threadIdx.x);
    if (t >= ldt) return;
    const float* xr = x + (size_t)row * ldt;
    float* cr = cols + (size_t)row * P * ldt + t;
    for (int p = 0; p < P; ++p) {
        const int i = t + p * dil - pad;
        st4(cr + (size_t)p * ldt, ud_mask(ud_window(xr, i, ldt), t, i, T));
    }
}

// dx[row][u] = sum_p dcols[row P + p][u - p dil + pad] over the p whose frame is in [0, T), ascending p; zero for u >= T
__global__ __launch_bounds__(256) void ud_fold_kernel(const float* __restrict__ dcols, float* __restrict__ dx, int T, int ldt, int P, int dil, int pad) {
    const int64_t row = blockIdx.x;
    const int u = 4 * (blockIdx.y * 256 + threadIdx.x);
    if (u >= ldt) return;
    const float* cr = dcols + (size_t)row * P * ldt;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int p = 0; p < P; ++p) {
        const int i = u - p * dil + pad;
        const float4 v = ud_mask(ud_window(cr + (size_t)p * ldt, i, ldt), u, i, T);
        acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w;
    }
    st4(dx + (size_t)row * ldt + u, acc);
}

inline bool cd_args_ok(int B, int C, int T, int ldt, int Kw, int pad, int dil) {
    return B > 0 && C > 0 && T > 0 && ldt >= T && ldt % 4 == 0 && Kw >= 1 && dil >= 1 && pad >= 0 && (long)pad <= (long)(Kw - 1) * dil &&
           (long)B * C <= 0x7fffffffL;
}

}  // namespace

/* the B * C row partials of a PReLU slope's gradient (sep_cln_bwd's dalpha_part) -> the one slope: what the eager step leaves to
 * torch's `sum(dtype=float64)`; cancelling sums, hence fp64 */
extern "C" int sep_sum_f64(const float* x, int64_t n, float* out, sep_stream_t stream) {
    SEP_REQUIRE(x && out && n > 0, "sep_sum_f64: bad arguments");
    hipLaunchKernelGGL(cd_sum_f64_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, x, n, out);
    SEP_CHECK_LAUNCH("sep_sum_f64");
    return 0;
}

extern "C" int sep_depthwise_cln_fwd(const float* x, const float* alpha, const float* gamma, const float* beta, const float* mean, const float* rstd,
                                     const float* w, const float* bias, float* y, int B, int C, int T, int ldt, int Kw, int pad, int dil,
                                     sep_stream_t stream_) {
    SEP_REQUIRE(x && gamma && beta && mean && rstd && w && y && cd_args_ok(B, C, T, ldt, Kw, pad, dil),
                "sep_depthwise_cln_fwd: bad arguments (ldt a multiple of 4, 0 <= pad <= (Kw - 1) dil)");
    hipStream_t stream = (hipStream_t)stream_;
    const size_t bytes = (size_t)ldt * sizeof(float);
    const dim3 grid((unsigned)((long)B * C)), block(256);
#define SEP_CDF(KW, ST) sep_set_kernel("cd_depthwise_fwd<" #KW "," #ST ">"); hipLaunchKernelGGL((cd_depthwise_fwd_kernel<KW, ST>), grid, block, ST ? bytes : (size_t)0, stream, x, alpha, gamma, beta, mean, rstd, w, bias, y, C, T, ldt, Kw, pad, dil)
    if (bytes <= CD_LDS_ROW_BYTES) {
        if (Kw == 3) { SEP_CDF(3, true); } else { SEP_CDF(0, true); }
    } else {
        if (Kw == 3) { SEP_CDF(3, false); } else { SEP_CDF(0, false); }
    }
#undef SEP_CDF
    SEP_CHECK_LAUNCH("sep_depthwise_cln_fwd");
    return 0;
}

extern "C" int sep_depthwise_cln_bwd_weight(const float* dy, const float* x, const float* alpha, const float* gamma, const float* beta, const float* mean,
                                            const float* rstd, float* partial, int B, int C, int T, int ldt, int Kw, int pad, int dil,
                                            sep_stream_t stream_) {
    SEP_REQUIRE(dy && x && gamma && beta && mean && rstd && partial && cd_args_ok(B, C, T, ldt, Kw, pad, dil),
                "sep_depthwise_cln_bwd_weight: bad arguments (ldt a multiple of 4, 0 <= pad <= (Kw - 1) dil)");
    hipStream_t stream = (hipStream_t)stream_;
    const size_t bytes = (size_t)ldt * sizeof(float);
    const dim3 grid((unsigned)((long)B * C)), block(256);
#define SEP_CDW(KW, ST) sep_set_kernel("cd_depthwise_wgrad<" #KW "," #ST ">"); hipLaunchKernelGGL((cd_depthwise_wgrad_kernel<KW, ST>), grid, block, ST ? bytes : (size_t)0, stream, dy, x, alpha, gamma, beta, mean, rstd, partial, C, T, ldt, Kw, pad, dil)
    if (bytes <= CD_LDS_ROW_BYTES) {
        if (Kw == 3) { SEP_CDW(3, true); } else { SEP_CDW(0, true); }
    } else {
        if (Kw == 3) { SEP_CDW(3, false); } else { SEP_CDW(0, false); }
    }
#undef SEP_CDW
    SEP_CHECK_LAUNCH("sep_depthwise_cln_bwd_weight");
    return 0;
}

/* the dilated unfold of the causal layers with full k-tap convolutions and its adjoint (include/sepkernels.h) */
extern "C" int sep_unfold_dilated(const float* x, float* cols, int B, int C, int T, int ldt, int P, int dil, int pad, sep_stream_t stream) {
    SEP_REQUIRE(x && cols && x != cols && cd_args_ok(B, C, T, ldt, P, pad, dil) && (long)(P - 1) * dil <= 0x3fffffffL,
                "sep_unfold_dilated: bad arguments (ldt a multiple of 4, 0 <= pad <= (P - 1) dil)");
    SEP_REQUIRE(ldt <= 65535 * 1024, "sep_unfold_dilated: ldt = %d exceeds the grid", ldt);
    hipLaunchKernelGGL(ud_unfold_kernel, dim3((unsigned)((long)B * C), (unsigned)((ldt + 1023) / 1024)), dim3(256), 0, (hipStream_t)stream, x, cols, T, ldt, P, dil, pad);
    SEP_CHECK_LAUNCH("sep_unfold_dilated");
    return 0;
}

extern "C" int sep_fold_dilated(const float* dcols, float* dx, int B, int C, int T, int ldt, int P, int dil, int pad, sep_stream_t stream) {
    SEP_REQUIRE(dcols && dx && dcols != dx && cd_args_ok(B, C, T, ldt, P, pad, dil) && (long)(P - 1) * dil <= 0x3fffffffL,
                "sep_fold_dilated: bad arguments (ldt a multiple of 4, 0 <= pad <= (P - 1) dil)");
    SEP_REQUIRE(ldt <= 65535 * 1024, "sep_fold_dilated: ldt = %d exceeds the grid", ldt);
    hipLaunchKernelGGL(ud_fold_kernel, dim3((unsigned)((long)B * C), (unsigned)((ldt + 1023) / 1024)), dim3(256), 0, (hipStream_t)stream, dcols, dx, T, ldt, P, dil, pad);
    SEP_CHECK_LAUNCH("sep_fold_dilated");
    return 0;
}
