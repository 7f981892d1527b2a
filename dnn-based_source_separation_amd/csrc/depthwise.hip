// Generic depthwise Conv1d with the three-tap row forms of the TCN layers' own geometry, Segment1d / OverlapAdd1d of the dual-path models
// and the row repack, for gfx950 (HBM-bound streaming kernels, fp32).
//
// Reference arithmetic replaced (reference src/): modules/conv.py:13-29 (depthwise Conv1d), models/transform.py:6-65 (segment, overlap-add).
#include <stdlib.h>
#include "common.hpp"

namespace {

// =====================================================================================
// Generic depthwise Conv1d (reference src/modules/conv.py:13-29, nn.Conv1d(groups=C) with any kernel size / stride /
// padding / dilation).  Not on the Conv-TasNet hot path (its depthwise is dwconv_fwd of tcn.hip); plain streaming kernels.
//   y[r][to] = bias[c] + sum_k w[c][k] * xpad[r][to*stride + k*dil - pad]           r = b*C + c
// =====================================================================================
__global__ __launch_bounds__(256) void depthwise_fwd_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                            const float* __restrict__ bias, float* __restrict__ y, int C,
                                                            int Tin, int Tout, int Kw, int stride, int pad, int dil) {
    const int row = blockIdx.y, c = row % C;
    const int to = blockIdx.x * 256 + threadIdx.x;
    if (to >= Tout) return;
    float acc = bias ? bias[c] : 0.f;
    for (int k = 0; k < Kw; ++k) {
        const int ti = to * stride + k * dil - pad;
        if (ti >= 0 && ti < Tin) acc = fmaf(w[c * Kw + k], x[(size_t)row * Tin + ti], acc);
    }
    y[(size_t)row * Tout + to] = acc;
}

__global__ __launch_bounds__(256) void depthwise_bwd_input_kernel(const float* __restrict__ dy, const float* __restrict__ w,
                                                                  float* __restrict__ dx, int C, int Tin, int Tout, int Kw,
                                                                  int stride, int pad, int dil) {
    const int row = blockIdx.y, c = row % C;
    const int ti = blockIdx.x * 256 + threadIdx.x;
    if (ti >= Tin) return;
    float acc = 0.f;
    for (int k = 0; k < Kw; ++k) {
        const int num = ti + pad - k * dil;
        if (num >= 0 && num % stride == 0) {
            const int to = num / stride;
            if (to < Tout) acc = fmaf(w[c * Kw + k], dy[(size_t)row * Tout + to], acc);
        }
    }
    dx[(size_t)row * Tin + ti] = acc;
}

// partial[b][c][0..Kw-1] = sum_to dy * xpad(tap k) ; partial[b][c][Kw] = sum_to dy     (one block per (b, c) row)
__global__ __launch_bounds__(256) void depthwise_bwd_weight_kernel(const float* __restrict__ dy, const float* __restrict__ x,
                                                                   float* __restrict__ partial, int C, int Tin, int Tout, int Kw,
                                                                   int stride, int pad, int dil) {
    __shared__ float red[4];
    const int row = blockIdx.x;
    for (int k = 0; k <= Kw; ++k) {
        float acc = 0.f;
        for (int to = threadIdx.x; to < Tout; to += 256) {
            const float g = dy[(size_t)row * Tout + to];
            if (k == Kw) acc += g;
            else {
                const int ti = to * stride + k * dil - pad;
                if (ti >= 0 && ti < Tin) acc = fmaf(g, x[(size_t)row * Tin + ti], acc);
            }
        }
        const float tot = block_sum_256<float>(acc, red);
        if (threadIdx.x == 0) partial[(size_t)row * (Kw + 1) + k] = tot;
    }
}

// ---- the TCN layers' own depthwise geometry (stride 1, three taps, Tin = Tout = the workspace stride, `pad` zeros in front: (P - 1) d when
// causal), one (b, c) row per workgroup, a float4 of frames per thread and trip.  Tap k sits at t + k d - pad.  For shifts that are multiples
// of 4 the taps are aligned float4 loads; for the others (d = 1, 2: the first two layers of a block) the row goes through LDS once.
// The generic kernels above take one frame per thread: 130 - 144 us per call at the paper-best sizes (profiles/r05o_causal_kernel_stats.md).
template <int MODE>      // 0: forward  y = b + sum_k w_k x[t + k d - pad];  1: input gradient  dx[t] = sum_k w_k dy[t - k d + pad]
__global__ __launch_bounds__(256) void depthwise3_row_kernel(const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ bias,
                                                             float* __restrict__ y, int C, int ldt, int dil, int pad) {
    extern __shared__ __attribute__((aligned(16))) float rowbuf[];
    const int row = blockIdx.x, c = row % C;
    const float* xr = x + (size_t)row * ldt;
    float* yr = y + (size_t)row * ldt;
    const float w0 = w[c * 3 + 0], w1 = w[c * 3 + 1], w2 = w[c * 3 + 2];
    const float bb = (MODE == 0 && bias) ? bias[c] : 0.f;
    // shifts of the three taps relative to the output frame
    const int s0 = MODE == 0 ? -pad : pad, s1 = MODE == 0 ? dil - pad : pad - dil, s2 = MODE == 0 ? 2 * dil - pad : pad - 2 * dil;
    const bool aligned = ((s0 | s1 | s2) & 3) == 0;
    if (!aligned) {
        for (int t = 4 * threadIdx.x; t < ldt; t += 1024) st4(rowbuf + t, ld4(xr + t));
        __syncthreads();
    }
    const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int t = 4 * threadIdx.x; t < ldt; t += 1024) {
        float a0[4], a1[4], a2[4];
        if (aligned) {
            const float4 v0 = (t + s0 >= 0 && t + s0 < ldt) ? ld4(xr + t + s0) : zero4;
            const float4 v1 = (t + s1 >= 0 && t + s1 < ldt) ? ld4(xr + t + s1) : zero4;
            const float4 v2 = (t + s2 >= 0 && t + s2 < ldt) ? ld4(xr + t + s2) : zero4;
            a0[0] = v0.x; a0[1] = v0.y; a0[2] = v0.z; a0[3] = v0.w;
            a1[0] = v1.x; a1[1] = v1.y; a1[2] = v1.z; a1[3] = v1.w;
            a2[0] = v2.x; a2[1] = v2.y; a2[2] = v2.z; a2[3] = v2.w;
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int i0 = t + e + s0, i1 = t + e + s1, i2 = t + e + s2;
                a0[e] = (i0 >= 0 && i0 < ldt) ? rowbuf[i0] : 0.f;
                a1[e] = (i1 >= 0 && i1 < ldt) ? rowbuf[i1] : 0.f;
                a2[e] = (i2 >= 0 && i2 < ldt) ? rowbuf[i2] : 0.f;
            }
        }
        float o[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = fmaf(w2, a2[e], fmaf(w1, a1[e], fmaf(w0, a0[e], bb)));
        st4(yr + t, make_float4(o[0], o[1], o[2], o[3]));
    }
}

// partial[b][c][k] = sum_t dy[t] x[t + k d - pad] (k < 3), partial[b][c][3] = sum_t dy[t]: one row per workgroup, the x row through LDS
__global__ __launch_bounds__(256) void depthwise3_wgrad_row_kernel(const float* __restrict__ dy, const float* __restrict__ x, float* __restrict__ partial,
                                                                   int ldt, int dil, int pad) {
    extern __shared__ __attribute__((aligned(16))) float rowbuf[];
    __shared__ float red[4][4];
    const int row = blockIdx.x;
    const float* xr = x + (size_t)row * ldt;
    const float* gr = dy + (size_t)row * ldt;
    for (int t = 4 * threadIdx.x; t < ldt; t += 1024) st4(rowbuf + t, ld4(xr + t));
    __syncthreads();
    float q0 = 0.f, q1 = 0.f, q2 = 0.f, q3 = 0.f;
    for (int t = 4 * threadIdx.x; t < ldt; t += 1024) {
        const float4 g4 = ld4(gr + t);
        const float g[4] = {g4.x, g4.y, g4.z, g4.w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int i0 = t + e - pad, i1 = i0 + dil, i2 = i1 + dil;
            q0 = fmaf(g[e], (i0 >= 0 && i0 < ldt) ? rowbuf[i0] : 0.f, q0);
            q1 = fmaf(g[e], (i1 >= 0 && i1 < ldt) ? rowbuf[i1] : 0.f, q1);
            q2 = fmaf(g[e], (i2 >= 0 && i2 < ldt) ? rowbuf[i2] : 0.f, q2);
            q3 += g[e];
        }
    }
    q0 = wave_sum(q0); q1 = wave_sum(q1); q2 = wave_sum(q2); q3 = wave_sum(q3);
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    if (lane == 0) { red[wv][0] = q0; red[wv][1] = q1; red[wv][2] = q2; red[wv][3] = q3; }
    __syncthreads();
    if (threadIdx.x < 4) partial[(size_t)row * 4 + threadIdx.x] = (red[0][threadIdx.x] + red[1][threadIdx.x]) + (red[2][threadIdx.x] + red[3][threadIdx.x]);
}

// the row kernels take the TCN layers' geometry: stride 1, three taps, rows of a multiple of 4 frames that fit the LDS
static inline bool depthwise3_rows(int Tin, int Tout, int Kw, int stride) {
    static const bool off = getenv("SEPK_DEPTHWISE_ROWS") != nullptr && atoi(getenv("SEPK_DEPTHWISE_ROWS")) == 0;
    return !off && Kw == 3 && stride == 1 && Tin == Tout && Tin % 4 == 0 && (size_t)Tin * sizeof(float) <= 128 * 1024;      // one row of LDS: 128 of gfx950's 160 KB
}

// =====================================================================================
// Segment1d / OverlapAdd1d of the dual-path models (reference src/models/transform.py:6-65) as index maps, without
// the unfold/fold materialisation + permute copies of the reference:
//   segment:     out[b][c][s][k] = xpad[b][c][s*hop + k],  xpad = x (padded rows, T valid frames) shifted right by pad_left
//   overlap-add: out[b][c][t]    = sum_{(s,k): s*hop + k == t + pad_left} y[b][c][s][k]   (t < T; zero for T <= t < ldt)
// The two are adjoints, so each is the other's backward.
// =====================================================================================
__global__ __launch_bounds__(256) void segment_kernel(const float* __restrict__ x, float* __restrict__ out, int T, int ldt,
                                                      int S, int Kc, int hop, int pad_left) {
    const int row = blockIdx.y;                                  // b*C + c
    const int i = blockIdx.x * 256 + threadIdx.x;                // s*Kc + k
    if (i >= S * Kc) return;
    const int s = i / Kc, k = i % Kc;
    const int t = s * hop + k - pad_left;
    out[(size_t)row * S * Kc + i] = (t >= 0 && t < T) ? x[(size_t)row * ldt + t] : 0.f;
}

__global__ __launch_bounds__(256) void overlap_add_kernel(const float* __restrict__ y, float* __restrict__ out, int T, int ldt,
                                                          int S, int Kc, int hop, int pad_left) {
    const int row = blockIdx.y;
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= ldt) return;
    float acc = 0.f;
    if (t < T) {
        const int tp = t + pad_left;
        // chunks covering tp: s*hop <= tp < s*hop + Kc
        int s_hi = tp / hop;
        if (s_hi > S - 1) s_hi = S - 1;
        for (int s = s_hi; s >= 0 && tp - s * hop < Kc; --s) acc += y[((size_t)row * S + s) * Kc + (tp - s * hop)];
    }
    out[(size_t)row * ldt + t] = acc;
}

__global__ __launch_bounds__(256) void repack_kernel(const float* __restrict__ src, int ld_src, float* __restrict__ dst,
                                                     int ld_dst, int T) {
    const int row = blockIdx.y;
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= ld_dst) return;
    dst[(size_t)row * ld_dst + t] = (t < T) ? src[(size_t)row * ld_src + t] : 0.f;
}

}  // namespace

// ---------------------------------------------------------------------------------------
extern "C" int sep_depthwise_fwd(const float* x, const float* w, const float* bias, float* y, int B, int C, int Tin, int Tout,
                                 int Kw, int stride, int pad, int dil, sep_stream_t stream) {
    SEP_REQUIRE(x && w && y && B > 0 && C > 0 && Tin > 0 && Tout > 0 && Kw > 0 && stride > 0 && dil > 0 && pad >= 0, "sep_depthwise_fwd: bad arguments");
    if (depthwise3_rows(Tin, Tout, Kw, stride)) {
        // the LDS row is only touched when a tap's shift is not a multiple of 4 frames (the kernel's `aligned`): none is asked for otherwise,
        // which is every dilation >= 4 of the TCN -- 128 KB per workgroup at the longest row would leave one workgroup per compute unit
        const bool al = ((pad | (dil - pad) | (2 * dil - pad)) & 3) == 0;
        sep_set_kernel(al ? "depthwise3_row<0>/aligned" : "depthwise3_row<0>/lds");
        hipLaunchKernelGGL((depthwise3_row_kernel<0>), dim3((unsigned)((long)B * C)), dim3(256), al ? (size_t)0 : (size_t)Tin * sizeof(float), (hipStream_t)stream, x, w, bias, y, C, Tin, dil, pad);
        SEP_CHECK_LAUNCH("sep_depthwise_fwd");
        return 0;
    }
    SEP_REQUIRE((long)B * C <= 65535, "sep_depthwise_fwd: B*C too large");
    sep_set_kernel("depthwise_fwd");
    hipLaunchKernelGGL(depthwise_fwd_kernel, dim3(ceil_div(Tout, 256), B * C), dim3(256), 0, (hipStream_t)stream, x, w, bias, y, C, Tin, Tout, Kw, stride, pad, dil);
    SEP_CHECK_LAUNCH("sep_depthwise_fwd");
    return 0;
}

extern "C" int sep_depthwise_bwd_input(const float* dy, const float* w, float* dx, int B, int C, int Tin, int Tout, int Kw,
                                       int stride, int pad, int dil, sep_stream_t stream) {
    SEP_REQUIRE(dy && w && dx && B > 0 && C > 0 && stride > 0, "sep_depthwise_bwd_input: bad arguments");
    if (depthwise3_rows(Tin, Tout, Kw, stride)) {
        const bool al = ((pad | (pad - dil) | (pad - 2 * dil)) & 3) == 0;          // (see sep_depthwise_fwd)
        sep_set_kernel(al ? "depthwise3_row<1>/aligned" : "depthwise3_row<1>/lds");
        hipLaunchKernelGGL((depthwise3_row_kernel<1>), dim3((unsigned)((long)B * C)), dim3(256), al ? (size_t)0 : (size_t)Tin * sizeof(float), (hipStream_t)stream, dy, w, (const float*)nullptr, dx, C, Tin, dil, pad);
        SEP_CHECK_LAUNCH("sep_depthwise_bwd_input");
        return 0;
    }
    SEP_REQUIRE((long)B * C <= 65535, "sep_depthwise_bwd_input: B*C too large");
    sep_set_kernel("depthwise_bwd_input");
    hipLaunchKernelGGL(depthwise_bwd_input_kernel, dim3(ceil_div(Tin, 256), B * C), dim3(256), 0, (hipStream_t)stream, dy, w, dx, C, Tin, Tout, Kw, stride, pad, dil);
    SEP_CHECK_LAUNCH("sep_depthwise_bwd_input");
    return 0;
}

extern "C" int sep_depthwise_bwd_weight(const float* dy, const float* x, float* partial, int B, int C, int Tin, int Tout, int Kw,
                                        int stride, int pad, int dil, sep_stream_t stream) {
    SEP_REQUIRE(dy && x && partial && B > 0 && C > 0, "sep_depthwise_bwd_weight: bad arguments");
    if (depthwise3_rows(Tin, Tout, Kw, stride)) {
        sep_set_kernel("depthwise3_wgrad_row");
        hipLaunchKernelGGL(depthwise3_wgrad_row_kernel, dim3((unsigned)((long)B * C)), dim3(256), (size_t)Tin * sizeof(float), (hipStream_t)stream, dy, x, partial, Tin, dil, pad);
        SEP_CHECK_LAUNCH("sep_depthwise_bwd_weight");
        return 0;
    }
    sep_set_kernel("depthwise_bwd_weight");
    hipLaunchKernelGGL(depthwise_bwd_weight_kernel, dim3(B * C), dim3(256), 0, (hipStream_t)stream, dy, x, partial, C, Tin, Tout, Kw, stride, pad, dil);
    SEP_CHECK_LAUNCH("sep_depthwise_bwd_weight");
    return 0;
}

extern "C" int sep_segment(const float* x, float* out, int rows, int T, int ldt, int S, int chunk, int hop, int pad_left,
                           sep_stream_t stream) {
    SEP_REQUIRE(x && out && rows > 0 && T > 0 && ldt >= T && S > 0 && chunk > 0 && hop > 0, "sep_segment: bad arguments");
    int done = 0;
    while (done < rows) {
        const int nr = (rows - done) > 65535 ? 65535 : (rows - done);
        dim3 grid(ceil_div(S * chunk, 256), nr);
        hipLaunchKernelGGL(segment_kernel, grid, dim3(256), 0, (hipStream_t)stream, x + (size_t)done * ldt, out + (size_t)done * S * chunk, T, ldt, S, chunk, hop, pad_left);
        done += nr;
    }
    SEP_CHECK_LAUNCH("sep_segment");
    return 0;
}

extern "C" int sep_overlap_add(const float* y, float* out, int rows, int T, int ldt, int S, int chunk, int hop, int pad_left,
                               sep_stream_t stream) {
    SEP_REQUIRE(y && out && rows > 0 && T > 0 && ldt >= T && S > 0 && chunk > 0 && hop > 0, "sep_overlap_add: bad arguments");
    int done = 0;
    while (done < rows) {
        const int nr = (rows - done) > 65535 ? 65535 : (rows - done);
        dim3 grid(ceil_div(ldt, 256), nr);
        hipLaunchKernelGGL(overlap_add_kernel, grid, dim3(256), 0, (hipStream_t)stream, y + (size_t)done * S * chunk, out + (size_t)done * ldt, T, ldt, S, chunk, hop, pad_left);
        done += nr;
    }
    SEP_CHECK_LAUNCH("sep_overlap_add");
    return 0;
}

extern "C" int sep_repack(const float* src, int ld_src, float* dst, int ld_dst, int rows, int T, sep_stream_t stream) {
    SEP_REQUIRE(src && dst && rows > 0 && T > 0 && ld_src >= T && ld_dst >= T, "sep_repack: bad arguments");
    SEP_REQUIRE(rows <= 65535 * 64, "sep_repack: too many rows");
    // grid.y limited to 65535: fold rows
    int done = 0;
    while (done < rows) {
        const int chunk = (rows - done) > 65535 ? 65535 : (rows - done);
        dim3 grid(ceil_div(ld_dst, 256), chunk);
        hipLaunchKernelGGL(repack_kernel, grid, dim3(256), 0, (hipStream_t)stream, src + (size_t)done * ld_src, ld_src, dst + (size_t)done * ld_dst, ld_dst, T);
        done += chunk;
    }
    SEP_CHECK_LAUNCH("sep_repack");
    return 0;
}
