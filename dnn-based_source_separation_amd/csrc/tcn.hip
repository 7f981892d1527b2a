// The fused depthwise block of a Conv-TasNet TCN layer for gfx950 (HBM-bound streaming kernels): the dilated depthwise conv with the
// gLN + PReLU of its input fused on load, forward and backward, each as a direct / row form and an LDS-tiled fallback; the gradient of the
// head behind the encoder; the channel softmax of the mask; the fp16 row pre-split of the skip gradient.  All tensors (batch, channel,
// frame) fp32 with padded row stride ldt; frames [T, ldt) of every written tensor are zero.
//
// Reference arithmetic replaced (reference src/): models/tdcn.py:113-132,177-186 (PReLU -> gLN -> zero pad -> depthwise conv -> PReLU),
// models/conv_tasnet.py:353-357,375 (softmax masks).
#include <stdlib.h>
#include "common.hpp"

namespace {

// =====================================================================================
// Depthwise dilated conv, forward.  One wave = one (b, c, 1024-frame tile): the tile plus a halo of
// round_up(d,4) frames each side is loaded with float4, normalised (gLN o PReLU) and zero-masked on the
// way into wave-private LDS; outputs are computed lane-consecutive (conflict-free ds_read_b32).
// =====================================================================================
constexpr int DW_TT = 1024;

__global__ __launch_bounds__(256) void dwconv_fwd_kernel(const float* __restrict__ a, const double* __restrict__ stats1,
                                                         const float* __restrict__ gamma1, const float* __restrict__ beta1,
                                                         const float* __restrict__ alpha1, const float* __restrict__ wd,
                                                         const float* __restrict__ bd, const float* __restrict__ alpha2,
                                                         float* __restrict__ z, double* __restrict__ stats2, int B, int C,
                                                         int T, int ldt, int d, int dpad, float eps) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    __shared__ double wred[4][2];
    __shared__ int wb[4];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int ntile = (ldt + DW_TT - 1) / DW_TT;
    const long total = (long)B * C * ntile;
    const long g = (long)blockIdx.x * 4 + wv;
    const bool active = g < total;
    const int wlen = DW_TT + 2 * dpad;
    float* vs = lds + (size_t)wv * wlen;

    int b = 0, c = 0, t0 = 0;
    float s = 0.f, ss = 0.f;
    if (active) {
        const int tile = (int)(g % ntile);
        c = (int)((g / ntile) % C);
        b = (int)(g / ((long)ntile * C));
        t0 = tile * DW_TT;
        float mu, rstd;
        gln_mu_rstd(stats1 + (size_t)b * SEP_STATS_SLOTS * 2, (double)C * T, eps, mu, rstd);
        const float a1 = alpha1[0];
        const float sc = gamma1[c] * rstd, sh = beta1[c] - mu * sc;
        const float* arow = a + ((size_t)b * C + c) * ldt;
        for (int q = lane; q < wlen / 4; q += 64) {
            const int tp = t0 - dpad + 4 * q;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (tp >= 0 && tp < ldt) {
                const float4 r = ld4(arow + tp);
                v.x = (tp + 0 < T) ? prelu_f(r.x, a1) * sc + sh : 0.f;
                v.y = (tp + 1 < T) ? prelu_f(r.y, a1) * sc + sh : 0.f;
                v.z = (tp + 2 < T) ? prelu_f(r.z, a1) * sc + sh : 0.f;
                v.w = (tp + 3 < T) ? prelu_f(r.w, a1) * sc + sh : 0.f;
            }
            st4(vs + 4 * q, v);
        }
    }
    __syncthreads();
    if (active) {
        const float w0 = wd[c * 3 + 0], w1 = wd[c * 3 + 1], w2 = wd[c * 3 + 2], bb = bd[c];
        const float a2 = alpha2[0];
        float* zrow = z + ((size_t)b * C + c) * ldt;
#pragma unroll 4
        for (int i = 0; i < DW_TT / 64; ++i) {
            const int o = lane + 64 * i;
            const int t = t0 + o;
            if (t >= ldt) break;
            float zz = 0.f;
            if (t < T) {
                zz = bb + w0 * vs[dpad + o - d] + w1 * vs[dpad + o] + w2 * vs[dpad + o + d];
                const float u = prelu_f(zz, a2);
                s += u; ss += u * u;
            }
            zrow[t] = zz;
        }
    }
    const double dsum = wave_sum((double)s), dss = wave_sum((double)ss);
    if (lane == 0) { wred[wv][0] = dsum; wred[wv][1] = dss; wb[wv] = active ? b : -1; }
    __syncthreads();
    if (threadIdx.x == 0) {
        // merge waves that belong to the same sample -> at most one atomic pair per sample per block
        for (int i = 0; i < 4; ++i) {
            if (wb[i] < 0) continue;
            double x0 = wred[i][0], x1 = wred[i][1];
            for (int k = i + 1; k < 4; ++k)
                if (wb[k] == wb[i]) { x0 += wred[k][0]; x1 += wred[k][1]; wb[k] = -1; }
            double* st = stats2 + ((size_t)wb[i] * SEP_STATS_SLOTS + (blockIdx.x & (SEP_STATS_SLOTS - 1))) * 2;
            atomicAdd(st, x0);
            atomicAdd(st + 1, x1);
        }
    }
}

// =====================================================================================
// Depthwise dilated conv forward, direct form (dilation 1, 2 or a multiple of 4 -- every power of two, i.e. every
// layer of the TCN): one workgroup = one (b, c) row; a thread produces float4s of output from three float4 loads
// (t-d, t, t+d; for d < 4 the two neighbouring float4s and a register shuffle).  The neighbours are another thread's
// centre, so two of the three loads hit L1/L2; nothing goes through LDS and there is no barrier before the stores.
// (Issuing all of a thread's loads before the first use, as dwconv_bwd_row_kernel does, was measured 6 % SLOWER here.)
// DM: 0 -> d % 4 == 0, 1 -> d == 1, 2 -> d == 2.
// =====================================================================================
template <int DM, int ROWS>
__global__ __launch_bounds__(256) void dwconv_fwd_direct_kernel(const float* __restrict__ a, const double* __restrict__ stats1,
                                                                const float* __restrict__ gamma1, const float* __restrict__ beta1,
                                                                const float* __restrict__ alpha1, const float* __restrict__ wd,
                                                                const float* __restrict__ bd, const float* __restrict__ alpha2,
                                                                float* __restrict__ z, double* __restrict__ stats2, int C, int T,
                                                                int ldt, int d, float eps) {
    __shared__ double red[4];
    const int row0 = blockIdx.x * ROWS;       // b * C + c of the first of ROWS consecutive channels of one sample (C % ROWS == 0)
    const int b = row0 / C;
    float mu, rstd;
    gln_mu_rstd(stats1 + (size_t)b * SEP_STATS_SLOTS * 2, (double)C * T, eps, mu, rstd);
    const float a1 = alpha1[0], a2 = alpha2[0];
    float s = 0.f, ss = 0.f;
#pragma unroll 1
    for (int rr = 0; rr < ROWS; ++rr) {
    const int row = row0 + rr, c = row % C;
    const float sc = gamma1[c] * rstd, sh = beta1[c] - mu * sc;
    const float w0 = wd[c * 3 + 0], w1 = wd[c * 3 + 1], w2 = wd[c * 3 + 2], bb = bd[c];
    const float* arow = a + (size_t)row * ldt;
    float* zrow = z + (size_t)row * ldt;
    const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
    auto norm = [&](float x, int t) { return (t >= 0 && t < T) ? fmaf(prelu_f(x, a1), sc, sh) : 0.f; };
    for (int q = threadIdx.x; q < ldt / 4; q += 256) {
        const int t = 4 * q;
        const float4 cc = ld4(arow + t);
        float lft[4], rgt[4];
        if (DM == 0) {
            const float4 l4 = t - d >= 0 ? ld4(arow + t - d) : zero4;
            const float4 r4 = t + d < ldt ? ld4(arow + t + d) : zero4;
            lft[0] = l4.x; lft[1] = l4.y; lft[2] = l4.z; lft[3] = l4.w;
            rgt[0] = r4.x; rgt[1] = r4.y; rgt[2] = r4.z; rgt[3] = r4.w;
        } else {
            const float4 l4 = t >= 4 ? ld4(arow + t - 4) : zero4;
            const float4 r4 = t + 4 < ldt ? ld4(arow + t + 4) : zero4;
            if (DM == 1) {
                lft[0] = l4.w; lft[1] = cc.x; lft[2] = cc.y; lft[3] = cc.z;
                rgt[0] = cc.y; rgt[1] = cc.z; rgt[2] = cc.w; rgt[3] = r4.x;
            } else {
                lft[0] = l4.z; lft[1] = l4.w; lft[2] = cc.x; lft[3] = cc.y;
                rgt[0] = cc.z; rgt[1] = cc.w; rgt[2] = r4.x; rgt[3] = r4.y;
            }
        }
        const float ce[4] = {cc.x, cc.y, cc.z, cc.w};
        float o[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int te = t + e;
            float zz = 0.f;
            if (te < T) {
                zz = bb + w0 * norm(lft[e], te - d) + w1 * norm(ce[e], te) + w2 * norm(rgt[e], te + d);
                const float u = prelu_f(zz, a2);
                s += u; ss = fmaf(u, u, ss);
            }
            o[e] = zz;
        }
        st4(zrow + t, make_float4(o[0], o[1], o[2], o[3]));
    }
    }
    const double ds = block_sum_256<double>((double)s, red);
    const double dss = block_sum_256<double>((double)ss, red);
    if (threadIdx.x == 0) {
        double* st = stats2 + ((size_t)b * SEP_STATS_SLOTS + (blockIdx.x & (SEP_STATS_SLOTS - 1))) * 2;
        atomicAdd(st, ds);
        atomicAdd(st + 1, dss);
    }
}

// =====================================================================================
// Backward of [gLN2 o PReLU2 o depthwise]: dv2 -> dv1 plus the per-row partial sums every downstream
// reduction needs (gLN1 backward, depthwise weight/bias gradient, PReLU2 slope gradient).
// rowpart[b][c][tile][8] = {sum dv1, sum dv1*u1, sum dz, sum dz*v1(t-d), sum dz*v1(t), sum dz*v1(t+d), dalpha2, 0}
// =====================================================================================
__global__ __launch_bounds__(256) void dwconv_bwd_kernel(
    const float* __restrict__ dv2, const float* __restrict__ z, const float* __restrict__ a,
    const double* __restrict__ stats1, const float* __restrict__ gamma1, const float* __restrict__ beta1,
    const float* __restrict__ alpha1, const double* __restrict__ stats2, const float* __restrict__ gamma2,
    const float* __restrict__ alpha2, const float* __restrict__ bsum2, const float* __restrict__ wd,
    float* __restrict__ dv1, float* __restrict__ rowpart, double* __restrict__ bacc1, int* __restrict__ arrive1, float* __restrict__ bsum1,
    int B, int C, int T, int ldt, int d, int dpad, float eps) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int ntile = (ldt + DW_TT - 1) / DW_TT;
    const long total = (long)B * C * ntile;
    const long g = (long)blockIdx.x * 4 + wv;
    const bool active = g < total;
    const int wlen = DW_TT + 2 * dpad;
    float* dzs = lds + (size_t)wv * 2 * wlen;
    float* us = dzs + wlen;

    int b = 0, c = 0, t0 = 0, tile = 0;
    float sc1 = 0.f, sh1 = 0.f;
    float q_dal = 0.f;
    if (active) {
        tile = (int)(g % ntile);
        c = (int)((g / ntile) % C);
        b = (int)(g / ((long)ntile * C));
        t0 = tile * DW_TT;
        float mu1, r1, mu2, r2;
        gln_mu_rstd(stats1 + (size_t)b * SEP_STATS_SLOTS * 2, (double)C * T, eps, mu1, r1);
        gln_mu_rstd(stats2 + (size_t)b * SEP_STATS_SLOTS * 2, (double)C * T, eps, mu2, r2);
        const float a1 = alpha1[0], a2 = alpha2[0];
        sc1 = gamma1[c] * r1; sh1 = beta1[c] - mu1 * sc1;
        const float g2 = gamma2[c];
        const float mg = bsum2[2 * b], mgx = bsum2[2 * b + 1];
        const size_t rowoff = ((size_t)b * C + c) * ldt;
        for (int q = lane; q < wlen / 4; q += 64) {
            const int tp = t0 - dpad + 4 * q;
            float dzv[4] = {0.f, 0.f, 0.f, 0.f}, uv[4] = {0.f, 0.f, 0.f, 0.f};
            if (tp >= 0 && tp < ldt) {
                const float4 gv = ld4(dv2 + rowoff + tp);
                const float4 zv = ld4(z + rowoff + tp);
                const float4 av = ld4(a + rowoff + tp);
                const float g4[4] = {gv.x, gv.y, gv.z, gv.w};
                const float z4[4] = {zv.x, zv.y, zv.z, zv.w};
                const float a4[4] = {av.x, av.y, av.z, av.w};
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int t = tp + e;
                    if (t < T) {
                        const float u2 = prelu_f(z4[e], a2);
                        const float xh = (u2 - mu2) * r2;
                        const float du2 = r2 * (g2 * g4[e] - mg - xh * mgx);
                        dzv[e] = du2 * prelu_grad(z4[e], a2);
                        uv[e] = prelu_f(a4[e], a1);
                        if (z4[e] <= 0.f && t >= t0 && t < t0 + DW_TT) q_dal += du2 * z4[e];
                    }
                }
            }
            st4(dzs + 4 * q, make_float4(dzv[0], dzv[1], dzv[2], dzv[3]));
            st4(us + 4 * q, make_float4(uv[0], uv[1], uv[2], uv[3]));
        }
    }
    __syncthreads();
    float q0 = 0.f, q1 = 0.f, q2 = 0.f, q3 = 0.f, q4 = 0.f, q5 = 0.f;
    if (active) {
        const float w0 = wd[c * 3 + 0], w1 = wd[c * 3 + 1], w2 = wd[c * 3 + 2];
        float* orow = dv1 + ((size_t)b * C + c) * ldt;
#pragma unroll 4
        for (int i = 0; i < DW_TT / 64; ++i) {
            const int o = lane + 64 * i;
            const int t = t0 + o;
            if (t >= ldt) break;
            float dv = 0.f;
            if (t < T) {
                const int p = dpad + o;
                // dv1[t] = sum_k w[k] * dz[t - (k-1) d]
                dv = w0 * dzs[p + d] + w1 * dzs[p] + w2 * dzs[p - d];
                const float dzt = dzs[p];
                // v1 = gLN1(u1) inside [0,T), literal zero outside (padding is applied after the norm)
                const float vm = (t - d >= 0) ? us[p - d] * sc1 + sh1 : 0.f;
                const float v0 = us[p] * sc1 + sh1;
                const float vp = (t + d < T) ? us[p + d] * sc1 + sh1 : 0.f;
                q0 += dv; q1 += dv * us[p];
                q2 += dzt; q3 += dzt * vm; q4 += dzt * v0; q5 += dzt * vp;
            }
            orow[t] = dv;
        }
    }
    q0 = wave_sum(q0); q1 = wave_sum(q1); q2 = wave_sum(q2); q3 = wave_sum(q3);
    q4 = wave_sum(q4); q5 = wave_sum(q5); q_dal = wave_sum(q_dal);
    if (active && lane == 0) {
        float* rp = rowpart + (((size_t)b * C + c) * ntile + tile) * 8;
        rp[0] = q0; rp[1] = q1; rp[2] = q2; rp[3] = q3; rp[4] = q4; rp[5] = q5; rp[6] = q_dal; rp[7] = 0.f;
        if (bacc1) {        // gLN1's gamma-weighted totals; the sample's last (channel, tile) publishes the two means (gln_bwd_publish)
            const float g1 = gamma1[c];
            const int slot = (int)(g & (SEP_STATS_SLOTS - 1));
            // slots are taken by the global unit number g; a sample's units are C * ntile consecutive numbers starting at b * C * ntile
            const long first = (long)b * C * ntile, nun = (long)C * ntile;
            int in_slot = 0, used = 0;
            for (int q = 0; q < SEP_STATS_SLOTS; ++q) {
                const long f0 = first + ((q - first) & (SEP_STATS_SLOTS - 1));      // first unit of the sample landing in slot q
                const int cnt_q = f0 < first + nun ? (int)((first + nun - f0 + SEP_STATS_SLOTS - 1) / SEP_STATS_SLOTS) : 0;
                used += cnt_q > 0;
                if (q == slot) in_slot = cnt_q;
            }
            if (arrive1)
                gln_bwd_publish(bacc1 + (size_t)b * SEP_STATS_SLOTS * 2, stats1 + (size_t)b * SEP_STATS_SLOTS * 2, arrive1 + (size_t)b * SEP_ARRIVE_INTS,
                                bsum1 + 2 * b, slot, in_slot, used, (double)(g1 * q0), (double)(g1 * q1), (double)C * T, eps);
            else {      // sums only: the consumer forms the means (sep_gemm_desc.pro_bacc)
                double* ba = bacc1 + ((size_t)b * SEP_STATS_SLOTS + slot) * 2;
                atomicAdd(ba, (double)(g1 * q0)); atomicAdd(ba + 1, (double)(g1 * q1));
            }
        }
    }
}

// =====================================================================================
// Same backward, one workgroup per (b, c) ROW: dz of the whole row lives in LDS (ldt floats), so there is no halo to re-load
// or re-compute (the 1024-frame tiles of the kernel above re-do 25 % of the row at dilation 128) and every global access is
// a float4.  u1 never goes to LDS: the three correlation sums are re-indexed onto the thread's own frame,
//   sum_t dz[t] v1[t-d] = sum_s v1[s] dz[s+d],   sum_t dz[t] v1[t+d] = sum_s v1[s] dz[s-d]      (dz = 0 outside [0, T)),
// so a thread keeps the PReLU1 outputs of its NIT float4 in registers across the barrier: 16 KiB of LDS per workgroup at
// ldt = 4096 instead of 32 (8 workgroups per CU instead of 4) and half the LDS traffic.  DM: see dw_row_neighbours (d % 4 == 0: ds_read_b128
// neighbours); NIT >= ldt / 1024.  Writes the row totals into tile 0 of rowpart and zeros into the other tiles (the
// finalize kernel sums over tiles).
// =====================================================================================
// the neighbours at distance d of the four frames t .. t + 3 of an LDS row: DM 0: d % 4 == 0 (two aligned float4 reads), 1 / 2: d = 1 / 2 (the
// two neighbouring float4s and register selects, as dwconv_fwd_direct_kernel does with global loads), 3: any d (eight scalar reads)
#ifndef DWB_WAVES
#define DWB_WAVES 6      // waves per SIMD the depthwise backward row kernel is compiled for (79 registers, no spills; 8 would spill 34)
#endif
template <int DM>
__device__ __forceinline__ void dw_row_neighbours(const float* row, const float4 c, const int t, const int d, const int ldt, float (&lft)[4], float (&rgt)[4]) {
    const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
    if (DM == 0) {
        const float4 m1 = t - d >= 0 ? ld4(row + t - d) : zero4, p1 = t + d < ldt ? ld4(row + t + d) : zero4;
        lft[0] = m1.x; lft[1] = m1.y; lft[2] = m1.z; lft[3] = m1.w;
        rgt[0] = p1.x; rgt[1] = p1.y; rgt[2] = p1.z; rgt[3] = p1.w;
    } else if (DM == 1 || DM == 2) {
        const float4 l4 = t >= 4 ? ld4(row + t - 4) : zero4, r4 = t + 4 < ldt ? ld4(row + t + 4) : zero4;
        if (DM == 1) {
            lft[0] = l4.w; lft[1] = c.x; lft[2] = c.y; lft[3] = c.z;
            rgt[0] = c.y; rgt[1] = c.z; rgt[2] = c.w; rgt[3] = r4.x;
        } else {
            lft[0] = l4.z; lft[1] = l4.w; lft[2] = c.x; lft[3] = c.y;
            rgt[0] = c.z; rgt[1] = c.w; rgt[2] = r4.x; rgt[3] = r4.y;
        }
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int tm = t + e - d, tq = t + e + d;
            lft[e] = tm >= 0 ? row[tm] : 0.f;
            rgt[e] = tq < ldt ? row[tq] : 0.f;
        }
    }
}

template <int DM, int NIT, bool RECOMP>
__global__ __launch_bounds__(256, NIT <= 4 ? DWB_WAVES : 3) void dwconv_bwd_row_kernel(
    const float* __restrict__ dv2, const float* __restrict__ z, const float* __restrict__ bd, const float* __restrict__ a,
    const double* __restrict__ stats1, const float* __restrict__ gamma1, const float* __restrict__ beta1,
    const float* __restrict__ alpha1, const double* __restrict__ stats2, const float* __restrict__ gamma2,
    const float* __restrict__ alpha2, const float* __restrict__ bsum2, const float* __restrict__ wd,
    float* __restrict__ dv1, float* __restrict__ rowpart, double* __restrict__ bacc1, int* __restrict__ arrive1, float* __restrict__ bsum1,
    int C, int T, int ldt, int d, float eps) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    __shared__ float part[4][8];
    float* dzs = lds;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int row = blockIdx.x;
    const int b = row / C, c = row % C;
    float mu1, r1, mu2, r2;
    gln_mu_rstd(stats1 + (size_t)b * SEP_STATS_SLOTS * 2, (double)C * T, eps, mu1, r1);
    gln_mu_rstd(stats2 + (size_t)b * SEP_STATS_SLOTS * 2, (double)C * T, eps, mu2, r2);
    const float a1 = alpha1[0], a2 = alpha2[0];
    const float sc1 = gamma1[c] * r1, sh1 = beta1[c] - mu1 * sc1;
    const float g2 = gamma2[c];
    const float mg = bsum2[2 * b], mgx = bsum2[2 * b + 1];
    const size_t rowoff = (size_t)row * ldt;
    const int nq4 = ldt / 4;
    float q_dal = 0.f;
    float4 gv[NIT], zv[NIT], av[NIT];
    float uv[NIT][4];
    const float w0 = wd[c * 3 + 0], w1 = wd[c * 3 + 1], w2 = wd[c * 3 + 2];
    // all global reads of the row first: 3 (RECOMP: 2) * NIT float4 in flight per thread
#pragma unroll
    for (int k = 0; k < NIT; ++k) {
        const int q = threadIdx.x + 256 * k;
        if (q < nq4) {
            gv[k] = ld4(dv2 + rowoff + 4 * q);
            if (!RECOMP) zv[k] = ld4(z + rowoff + 4 * q);
            av[k] = ld4(a + rowoff + 4 * q);
        }
    }
    if (RECOMP) {
        // z is not read: the row of v1 = gLN1(PReLU1(a)) goes to a second LDS row and z = bd + the three taps is formed again exactly as
        // dwconv_fwd_direct_kernel formed it (same expression, zero outside [0, T)) -- a quarter of the kernel's HBM bytes for 8 B of LDS
        // traffic per frame
        // v1s and dzs are never live together (v1 is dead once every thread has formed its z): ONE LDS row serves both, behind one more
        // barrier -- 16 KiB per workgroup at ldt = 4096 instead of 32: six workgroups per compute unit (the register limit) instead of four
        float* v1s = lds;
#pragma unroll
        for (int k = 0; k < NIT; ++k) {
            const int q = threadIdx.x + 256 * k;
            if (q < nq4) {
                const int tp = 4 * q;
                const float a4[4] = {av[k].x, av[k].y, av[k].z, av[k].w};
                float v4[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    uv[k][e] = tp + e < T ? prelu_f(a4[e], a1) : 0.f;
                    v4[e] = tp + e < T ? fmaf(uv[k][e], sc1, sh1) : 0.f;
                }
                st4(v1s + tp, make_float4(v4[0], v4[1], v4[2], v4[3]));
            }
        }
        __syncthreads();
        const float bb = bd[c];
#pragma unroll
        for (int k = 0; k < NIT; ++k) {
            const int q = threadIdx.x + 256 * k;
            if (q < nq4) {
                const int t = 4 * q;
                float lft[4], rgt[4], o[4];
                float c4[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) c4[e] = t + e < T ? fmaf(uv[k][e], sc1, sh1) : 0.f;      // this thread's own v1 (what it wrote)
                dw_row_neighbours<DM>(v1s, make_float4(c4[0], c4[1], c4[2], c4[3]), t, d, ldt, lft, rgt);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float ce = t + e < T ? fmaf(uv[k][e], sc1, sh1) : 0.f;
                    o[e] = t + e < T ? bb + w0 * lft[e] + w1 * ce + w2 * rgt[e] : 0.f;
                }
                zv[k] = make_float4(o[0], o[1], o[2], o[3]);
            }
        }
        __syncthreads();                                  // every neighbour read of v1 is done: the row becomes dz
    }
#pragma unroll
    for (int k = 0; k < NIT; ++k) {
        const int q = threadIdx.x + 256 * k;
        if (q < nq4) {
            const int tp = 4 * q;
            const float g4[4] = {gv[k].x, gv[k].y, gv[k].z, gv[k].w};
            const float z4[4] = {zv[k].x, zv[k].y, zv[k].z, zv[k].w};
            const float a4[4] = {av[k].x, av[k].y, av[k].z, av[k].w};
            float dzv[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                dzv[e] = 0.f;
                if (!RECOMP) uv[k][e] = 0.f;
                if (tp + e < T) {
                    const float u2 = prelu_f(z4[e], a2);
                    const float xh = (u2 - mu2) * r2;
                    const float du2 = r2 * (g2 * g4[e] - mg - xh * mgx);
                    dzv[e] = du2 * prelu_grad(z4[e], a2);
                    if (!RECOMP) uv[k][e] = prelu_f(a4[e], a1);
                    if (z4[e] <= 0.f) q_dal = fmaf(du2, z4[e], q_dal);
                }
            }
            st4(dzs + tp, make_float4(dzv[0], dzv[1], dzv[2], dzv[3]));
        }
    }
    __syncthreads();
    float* orow = dv1 + rowoff;
    float q0 = 0.f, q1 = 0.f, q2 = 0.f, q3 = 0.f, q4 = 0.f, q5 = 0.f;
#pragma unroll
    for (int k = 0; k < NIT; ++k) {
        const int q = threadIdx.x + 256 * k;
        if (q < nq4) {
            const int t = 4 * q;
            const float4 dzc4 = ld4(dzs + t);
            float dzm[4], dzp[4];
            dw_row_neighbours<DM>(dzs, dzc4, t, d, ldt, dzm, dzp);
            const float dzc[4] = {dzc4.x, dzc4.y, dzc4.z, dzc4.w};
            float o[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int te = t + e;
                float dv = 0.f;
                if (te < T) {
                    // dv1[t] = sum_k w[k] * dz[t - (k-1) d];  dz is zero outside [0, T) by construction
                    dv = w0 * dzp[e] + w1 * dzc[e] + w2 * dzm[e];
                    // v1 = gLN1(u1) inside [0,T) (the zero padding is applied after the norm and is covered by dz = 0 there)
                    const float v0 = fmaf(uv[k][e], sc1, sh1);
                    q0 += dv; q1 = fmaf(dv, uv[k][e], q1);
                    q2 += dzc[e]; q3 = fmaf(dzp[e], v0, q3); q4 = fmaf(dzc[e], v0, q4); q5 = fmaf(dzm[e], v0, q5);
                }
                o[e] = dv;
            }
            st4(orow + t, make_float4(o[0], o[1], o[2], o[3]));
        }
    }
    q0 = wave_sum(q0); q1 = wave_sum(q1); q2 = wave_sum(q2); q3 = wave_sum(q3);
    q4 = wave_sum(q4); q5 = wave_sum(q5); q_dal = wave_sum(q_dal);
    if (lane == 0) {
        part[wv][0] = q0; part[wv][1] = q1; part[wv][2] = q2; part[wv][3] = q3;
        part[wv][4] = q4; part[wv][5] = q5; part[wv][6] = q_dal; part[wv][7] = 0.f;
    }
    __syncthreads();
    const int ntile = (ldt + DW_TT - 1) / DW_TT;
    float* rp = rowpart + (size_t)row * ntile * 8;
    for (int i = threadIdx.x; i < ntile * 8; i += 256)
        rp[i] = i < 8 ? (part[0][i] + part[1][i]) + (part[2][i] + part[3][i]) : 0.f;
    if (bacc1 && threadIdx.x == 0) {     // gLN1's gamma-weighted totals; the sample's last row publishes the two means (gln_bwd_publish)
        const float g1c = gamma1[c];
        // slots are taken by the global row number; a sample's rows are C consecutive numbers starting at b * C
        const int slot = row & (SEP_STATS_SLOTS - 1), first = b * C;
        int in_slot = 0, used = 0;
        for (int q = 0; q < SEP_STATS_SLOTS; ++q) {
            const int f0 = first + ((q - first) & (SEP_STATS_SLOTS - 1));
            const int cnt_q = f0 < first + C ? (first + C - f0 + SEP_STATS_SLOTS - 1) / SEP_STATS_SLOTS : 0;
            used += cnt_q > 0;
            if (q == slot) in_slot = cnt_q;
        }
        const double t0_ = (double)(g1c * ((part[0][0] + part[1][0]) + (part[2][0] + part[3][0])));
        const double t1_ = (double)(g1c * ((part[0][1] + part[1][1]) + (part[2][1] + part[3][1])));
        if (arrive1)
            gln_bwd_publish(bacc1 + (size_t)b * SEP_STATS_SLOTS * 2, stats1 + (size_t)b * SEP_STATS_SLOTS * 2, arrive1 + (size_t)b * SEP_ARRIVE_INTS, bsum1 + 2 * b,
                            slot, in_slot, used, t0_, t1_, (double)C * T, eps);
        else {          // sums only: the consumer forms the means (sep_gemm_desc.pro_bacc)
            double* ba = bacc1 + ((size_t)b * SEP_STATS_SLOTS + slot) * 2;
            atomicAdd(ba, t0_); atomicAdd(ba + 1, t1_);
        }
    }
}

// dw = r0*(gamma*dvw - mg - xhat*mgx) + dwm  [* (w>0)]   in place on dvw
__global__ __launch_bounds__(256) void head_bwd_kernel(float* __restrict__ dvw, const float* __restrict__ w,
                                                       const float* __restrict__ dwm, const double* __restrict__ stats0,
                                                       const float* __restrict__ gamma0, const float* __restrict__ bsum0,
                                                       int C, int T, int ldt, double count, float eps, int relu) {
    const int row = blockIdx.y;            // b*C + c
    const int b = row / C, c = row % C;
    const int t4 = (blockIdx.x * 256 + threadIdx.x) * 4;
    if (t4 >= ldt) return;
    float mu, rstd;
    gln_mu_rstd(stats0 + (size_t)b * SEP_STATS_SLOTS * 2, count, eps, mu, rstd);
    const float gc = gamma0[c], mg = bsum0[2 * b], mgx = bsum0[2 * b + 1];
    const size_t off = (size_t)row * ldt + t4;
    const float4 g = ld4(dvw + off), ww = ld4(w + off), dm = ld4(dwm + off);
    const float g4[4] = {g.x, g.y, g.z, g.w}, w4[4] = {ww.x, ww.y, ww.z, ww.w}, m4[4] = {dm.x, dm.y, dm.z, dm.w};
    float o[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const float xh = (w4[e] - mu) * rstd;
        float v = rstd * (gc * g4[e] - mg - xh * mgx) + m4[e];
        if (relu && !(w4[e] > 0.f)) v = 0.f;
        o[e] = (t4 + e < T) ? v : 0.f;
    }
    st4(dvw + off, make_float4(o[0], o[1], o[2], o[3]));
}

// =====================================================================================
// Softmax over the channel axis, in place (reference conv_tasnet.py:353-357, 375: nn.Softmax(dim=1) on the (B, n_src*N, T')
// output of the mask convolution -- over ALL n_src*N channels of a frame, not over the sources).
// Workgroup = 64 frames x 4 channel groups (one wave each); a wave reads 256 contiguous bytes per channel row.
//   forward : y <- exp(y - max_c y) / sum_c exp(y - max_c y)      (frames >= T: 0, the layout contract)
//   backward: g <- y * (g - sum_c g*y)                            (frames >= T: 0)
// =====================================================================================
template <bool BWD>
__global__ __launch_bounds__(256) void softmax_ch_kernel(float* __restrict__ y, float* __restrict__ g, int C, int T, int ldt) {
    __shared__ float sa[4][64], sb[4][64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int t = blockIdx.x * 64 + lane;
    const size_t base = (size_t)blockIdx.y * C * ldt + t;
    const bool valid = t < T;
    if (!BWD) {
        float mx = -INFINITY, sum = 0.f;
        for (int c = w; c < C; c += 4) {
            const float v = y[base + (size_t)c * ldt];
            const float nm = fmaxf(mx, v);
            sum = sum * expf(mx - nm) + expf(v - nm);
            mx = nm;
        }
        sa[w][lane] = mx; sb[w][lane] = sum;
        __syncthreads();
        float M = fmaxf(fmaxf(sa[0][lane], sa[1][lane]), fmaxf(sa[2][lane], sa[3][lane]));
        float S = 0.f;
#pragma unroll
        for (int q = 0; q < 4; ++q) S += sb[q][lane] * expf(sa[q][lane] - M);
        const float inv = 1.f / S;
        for (int c = w; c < C; c += 4) {
            const size_t off = base + (size_t)c * ldt;
            y[off] = valid ? expf(y[off] - M) * inv : 0.f;
        }
    } else {
        float dot = 0.f;
        for (int c = w; c < C; c += 4) dot = fmaf(g[base + (size_t)c * ldt], y[base + (size_t)c * ldt], dot);
        sa[w][lane] = dot;
        __syncthreads();
        const float tot = (sa[0][lane] + sa[1][lane]) + (sa[2][lane] + sa[3][lane]);
        for (int c = w; c < C; c += 4) {
            const size_t off = base + (size_t)c * ldt;
            g[off] = valid ? y[off] * (g[off] - tot) : 0.f;
        }
    }
}

}  // namespace

// ---------------------------------------------------------------------------------------
extern "C" int sep_dwconv_fwd(const float* a, const double* stats1, const float* gamma1, const float* beta1,
                              const float* alpha1, const float* wd, const float* bd, const float* alpha2, float* z,
                              double* stats2, int B, int C, int T, int ldt, int dilation, float eps, sep_stream_t stream) {
    SEP_REQUIRE(a && stats1 && gamma1 && beta1 && alpha1 && wd && bd && alpha2 && z && stats2, "sep_dwconv_fwd: null pointer");
    SEP_REQUIRE(B > 0 && C > 0 && T > 0 && ldt % 128 == 0 && ldt >= T, "sep_dwconv_fwd: bad sizes");
    SEP_REQUIRE(dilation >= 1 && dilation <= 4096, "sep_dwconv_fwd: dilation %d out of range [1, 4096]", dilation);
    static const bool force_lds = getenv("SEPK_DWCONV_LDS") != nullptr;
    if (!force_lds && (dilation == 1 || dilation == 2 || dilation % 4 == 0) && (long)B * C <= 0x7fffffffL) {
        // two channels per workgroup: the statistics loads, the two block reductions and the two fp64 atomics are paid once per two
        // rows (0.430 -> 0.385 ms per 8 layers; four rows: 0.42; the same in the backward row kernel: slower, 0.79 -> 0.82)
        const int rows = C % 2 == 0 ? 2 : 1;
        const dim3 grid((unsigned)((long)B * C / rows));
#define SEP_DWF(DM) do { \
            sep_set_kernel(rows == 2 ? "dwconv_fwd_direct<" #DM ",2>" : "dwconv_fwd_direct<" #DM ",1>"); \
            if (rows == 2) hipLaunchKernelGGL((dwconv_fwd_direct_kernel<DM, 2>), grid, dim3(256), 0, (hipStream_t)stream, a, stats1, gamma1, beta1, alpha1, wd, bd, alpha2, z, stats2, C, T, ldt, dilation, eps); \
            else hipLaunchKernelGGL((dwconv_fwd_direct_kernel<DM, 1>), grid, dim3(256), 0, (hipStream_t)stream, a, stats1, gamma1, beta1, alpha1, wd, bd, alpha2, z, stats2, C, T, ldt, dilation, eps); \
        } while (0)
        if (dilation == 1) SEP_DWF(1);
        else if (dilation == 2) SEP_DWF(2);
        else SEP_DWF(0);
#undef SEP_DWF
        SEP_CHECK_LAUNCH("sep_dwconv_fwd");
        return 0;
    }
    const int dpad = (dilation + 3) & ~3;
    const size_t smem = 4 * (size_t)(DW_TT + 2 * dpad) * sizeof(float);
    const long total = (long)B * C * ceil_div(ldt, DW_TT);
    sep_set_kernel("dwconv_fwd_tiles");
    hipLaunchKernelGGL(dwconv_fwd_kernel, dim3((unsigned)((total + 3) / 4)), dim3(256), smem, (hipStream_t)stream, a, stats1, gamma1, beta1, alpha1, wd, bd, alpha2, z, stats2, B, C, T, ldt, dilation, dpad, eps);
    SEP_CHECK_LAUNCH("sep_dwconv_fwd");
    return 0;
}

extern "C" int sep_dwconv_bwd(const float* dv2, const float* z, const float* a, const double* stats1, const float* gamma1,
                              const float* beta1, const float* alpha1, const double* stats2, const float* gamma2,
                              const float* alpha2, const float* bsum2, const float* wd, const float* bd, float* dv1, float* rowpart,
                              double* bacc1, int* arrive1, float* bsum1, int B, int C, int T, int ldt, int dilation, float eps, sep_stream_t stream) {
    SEP_REQUIRE(dv2 && z && a && stats1 && gamma1 && beta1 && alpha1 && stats2 && gamma2 && alpha2 && bsum2 && wd && dv1 && rowpart, "sep_dwconv_bwd: null pointer");
    SEP_REQUIRE((arrive1 == nullptr) == (bsum1 == nullptr) && (bacc1 != nullptr || arrive1 == nullptr), "sep_dwconv_bwd: arrive1 and bsum1 come together and need bacc1");
    SEP_REQUIRE(B > 0 && C > 0 && T > 0 && ldt % 128 == 0 && ldt >= T, "sep_dwconv_bwd: bad sizes");
    SEP_REQUIRE(dilation >= 1 && dilation <= 2048, "sep_dwconv_bwd: dilation %d out of range [1, 2048]", dilation);
    static const bool force_tiles = getenv("SEPK_DWCONV_LDS") != nullptr;
    static const bool no_recompute = getenv("SEPK_DWB_RECOMPUTE") != nullptr && atoi(getenv("SEPK_DWB_RECOMPUTE")) == 0;
    if (!force_tiles && ldt <= 8192 && (long)B * C <= 0x7fffffffL) {        // the row (ldt floats of LDS, ldt / 1024 float4 triples in registers)
        // with the depthwise bias at hand z is formed again from `a` instead of being read (two LDS rows): 3 streams of HBM instead of 4
        const bool recomp = bd != nullptr && !no_recompute;
        const size_t rsmem = (size_t)ldt * sizeof(float);      // (the recomputing form's v1 row and the dz row share it)
        const dim3 grid((unsigned)((long)B * C));
#define SEP_DWB(AL, NIT, RC) hipLaunchKernelGGL((dwconv_bwd_row_kernel<AL, NIT, RC>), grid, dim3(256), rsmem, (hipStream_t)stream, dv2, z, bd, a, stats1, gamma1, beta1, alpha1, stats2, gamma2, alpha2, bsum2, wd, dv1, rowpart, bacc1, arrive1, bsum1, C, T, ldt, dilation, eps)
#define SEP_DWB2(AL, NIT) do { sep_set_kernel(recomp ? "dwconv_bwd_row<" #AL "," #NIT ",true>" : "dwconv_bwd_row<" #AL "," #NIT ",false>"); \
                               if (recomp) SEP_DWB(AL, NIT, true); else SEP_DWB(AL, NIT, false); } while (0)
        const int dm = dilation % 4 == 0 ? 0 : dilation <= 2 ? dilation : 3;
        if (dm == 0) { if (ldt <= 4096) SEP_DWB2(0, 4); else SEP_DWB2(0, 8); }
        else if (dm == 1) { if (ldt <= 4096) SEP_DWB2(1, 4); else SEP_DWB2(1, 8); }
        else if (dm == 2) { if (ldt <= 4096) SEP_DWB2(2, 4); else SEP_DWB2(2, 8); }
        else { if (ldt <= 4096) SEP_DWB2(3, 4); else SEP_DWB2(3, 8); }
#undef SEP_DWB2
#undef SEP_DWB
        SEP_CHECK_LAUNCH("sep_dwconv_bwd");
        return 0;
    }
    const int dpad = (dilation + 3) & ~3;
    const size_t smem = 4 * 2 * (size_t)(DW_TT + 2 * dpad) * sizeof(float);
    const long total = (long)B * C * ceil_div(ldt, DW_TT);
    sep_set_kernel("dwconv_bwd_tiles");
    hipLaunchKernelGGL(dwconv_bwd_kernel, dim3((unsigned)((total + 3) / 4)), dim3(256), smem, (hipStream_t)stream, dv2, z, a, stats1, gamma1, beta1, alpha1, stats2, gamma2, alpha2, bsum2, wd, dv1, rowpart, bacc1, arrive1, bsum1, B, C, T, ldt, dilation, dpad, eps);
    SEP_CHECK_LAUNCH("sep_dwconv_bwd");
    return 0;
}

extern "C" int sep_head_bwd(float* dvw, const float* w, const float* dwm, const double* stats0, const float* gamma0,
                            const float* bsum0, int B, int C, int T, int ldt, double count, float eps, int relu,
                            sep_stream_t stream) {
    SEP_REQUIRE(dvw && w && dwm && stats0 && gamma0 && bsum0 && ldt % 4 == 0, "sep_head_bwd: bad arguments");
    SEP_REQUIRE((long)B * C <= 65535, "sep_head_bwd: B*C too large for grid.y");
    dim3 grid(ceil_div(ldt, 1024), B * C);
    hipLaunchKernelGGL(head_bwd_kernel, grid, dim3(256), 0, (hipStream_t)stream, dvw, w, dwm, stats0, gamma0, bsum0, C, T, ldt, count, eps, relu);
    SEP_CHECK_LAUNCH("sep_head_bwd");
    return 0;
}

extern "C" int sep_softmax_ch_fwd(float* y, int B, int C, int T, int ldt, sep_stream_t stream) {
    SEP_REQUIRE(y && B > 0 && B <= 65535 && C > 0 && T > 0 && ldt % 64 == 0 && ldt >= T, "sep_softmax_ch_fwd: bad arguments");
    hipLaunchKernelGGL((softmax_ch_kernel<false>), dim3(ldt / 64, B), dim3(256), 0, (hipStream_t)stream, y, (float*)nullptr, C, T, ldt);
    SEP_CHECK_LAUNCH("sep_softmax_ch_fwd");
    return 0;
}

extern "C" int sep_softmax_ch_bwd(const float* y, float* g, int B, int C, int T, int ldt, sep_stream_t stream) {
    SEP_REQUIRE(y && g && B > 0 && B <= 65535 && C > 0 && T > 0 && ldt % 64 == 0 && ldt >= T, "sep_softmax_ch_bwd: bad arguments");
    hipLaunchKernelGGL((softmax_ch_kernel<true>), dim3(ldt / 64, B), dim3(256), 0, (hipStream_t)stream, const_cast<float*>(y), g, C, T, ldt);
    SEP_CHECK_LAUNCH("sep_softmax_ch_bwd");
    return 0;
}


// =====================================================================================
// sep_split_rows: rows of an activation tensor split once into the {hi, lo} fp16 operand form of the fp16 weight-gradient kernel's G operand
// (wgrad_pc16.hip, G2_pre): the skip gradient dS is the second G source of all 24 heads' weight gradients of a Conv-TasNet step (reference
// src/models/tdcn.py:173,175: the skip / output pointwise convolutions), so its half of the split arithmetic is done here once per step.
// One workgroup per (sample, row); the row (ldt <= 8192 floats) stays in registers between the maximum and the split.
// =====================================================================================
namespace {
constexpr int SPLIT_MAXK = 64;      // slabs per sample (small batches: one sample is cut into up to 64 slabs so that the weight gradient still fills the chip)
typedef __fp16 split_h2_t __attribute__((ext_vector_type(2)));
template <int NIT>
__global__ __launch_bounds__(256) void split_rows_kernel(const float* __restrict__ x, unsigned* __restrict__ out, int* __restrict__ exps,
                                                         float* __restrict__ sums, int C, int T, int ldt, int k) {
    __shared__ float red[4][SPLIT_MAXK + 1];
    const int row = blockIdx.x;                       // b * C + r
    const int b = row / C, r = row % C;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int nq4 = ldt / 4, per = ldt / k;
    float4 v[NIT];
    float m = 0.f;
    float rs[SPLIT_MAXK];
#pragma unroll
    for (int q = 0; q < SPLIT_MAXK; ++q) rs[q] = 0.f;
#pragma unroll
    for (int i = 0; i < NIT; ++i) {
        const int q = threadIdx.x + 256 * i;
        v[i] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (q < nq4) {
            v[i] = ld4(x + (size_t)row * ldt + 4 * q);
            const float e4[4] = {v[i].x, v[i].y, v[i].z, v[i].w};
            float s4 = 0.f;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float val = 4 * q + e < T ? e4[e] : 0.f;
                m = fmaxf(m, fabsf(val));
                s4 += val;
            }
            const int range = (4 * q) / per;              // per is a multiple of 32: the four frames lie in one range
#pragma unroll
            for (int qq = 0; qq < SPLIT_MAXK; ++qq) rs[qq] += qq == range ? s4 : 0.f;
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
#pragma unroll
    for (int qq = 0; qq < SPLIT_MAXK; ++qq) rs[qq] = wave_sum(rs[qq]);
    if (lane == 0) {
        red[wv][SPLIT_MAXK] = m;
#pragma unroll
        for (int qq = 0; qq < SPLIT_MAXK; ++qq) red[wv][qq] = rs[qq];
    }
    __syncthreads();
    m = fmaxf(fmaxf(red[0][SPLIT_MAXK], red[1][SPLIT_MAXK]), fmaxf(red[2][SPLIT_MAXK], red[3][SPLIT_MAXK]));
    const int ex = m > 0.f ? 13 - __builtin_amdgcn_frexp_expf(m) : 0;      // m = f 2^e', f in [0.5, 1): the maximum lands in [2^12, 2^13)
    if (threadIdx.x == 0) exps[row] = ex;
    if (sums && (int)threadIdx.x < k) sums[((size_t)b * k + threadIdx.x) * C + r] = (red[0][threadIdx.x] + red[1][threadIdx.x]) + (red[2][threadIdx.x] + red[3][threadIdx.x]);
    unsigned* orow = out + (size_t)row * ldt;          // the row in 32-bit words: 32 words per 32-frame line = 16 words of hi pairs, 16 of lo pairs
#pragma unroll
    for (int i = 0; i < NIT; ++i) {
        const int q = threadIdx.x + 256 * i;
        if (q < nq4) {
            const int t = 4 * q;
            const float e4[4] = {v[i].x, v[i].y, v[i].z, v[i].w};
            float w4[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) w4[e] = t + e < T ? __builtin_ldexpf(e4[e], ex) : 0.f;
            unsigned hi[2], lo[2];
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const split_h2_t hh = __builtin_amdgcn_cvt_pkrtz(w4[2 * h], w4[2 * h + 1]);
                hi[h] = __builtin_bit_cast(unsigned, hh);
                const float l0 = w4[2 * h] - (float)hh.x, l1 = w4[2 * h + 1] - (float)hh.y;      // exact in fp32
                lo[h] = __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_pkrtz(l0, l1));
            }
            unsigned* line = orow + (t / 32) * 32;        // 128 bytes per 32 frames
            const int w0 = (t % 32) / 2;                  // word of the frame pair inside the hi half
            line[w0] = hi[0]; line[w0 + 1] = hi[1];
            line[16 + w0] = lo[0]; line[16 + w0 + 1] = lo[1];
        }
    }
}
}  // namespace

extern "C" int sep_split_rows(const float* x, void* out, int32_t* exps, float* sums, int B, int C, int T, int ldt, int k, sep_stream_t stream) {
    SEP_REQUIRE(x && out && exps && B > 0 && C > 0 && T > 0 && ldt >= T && ldt % 128 == 0 && ldt <= 8192, "sep_split_rows: bad sizes (ldt <= 8192)");
    SEP_REQUIRE(k >= 1 && k <= SPLIT_MAXK && ldt % (32 * k) == 0 && (long)B * C <= 0x7fffffffL, "sep_split_rows: k = %d must divide ldt / 32 (<= %d)", k, SPLIT_MAXK);
    const dim3 grid((unsigned)((long)B * C));
    sep_set_kernel(ldt <= 4096 ? "split_rows<4>" : "split_rows<8>");
    if (ldt <= 4096) hipLaunchKernelGGL(split_rows_kernel<4>, grid, dim3(256), 0, (hipStream_t)stream, x, reinterpret_cast<unsigned*>(out), exps, sums, C, T, ldt, k);
    else hipLaunchKernelGGL(split_rows_kernel<8>, grid, dim3(256), 0, (hipStream_t)stream, x, reinterpret_cast<unsigned*>(out), exps, sums, C, T, ldt, k);
    SEP_CHECK_LAUNCH("sep_split_rows");
    return 0;
}
