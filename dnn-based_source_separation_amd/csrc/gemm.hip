// Pointwise (1x1) convolutions of the Conv-TasNet separator as fp32 MFMA GEMMs for gfx950: the forward and input-gradient products.
//
//   Y[b][m][t] = epi( sum_k A[m][k] * pro(X[b][k][t]) + bias[m] )     (sep_pw_gemm)
//
// Replaces nn.Conv1d(kernel_size=1) of reference src/models/tdcn.py:86,173,175 and
// src/models/conv_tasnet.py:335,341 together with the elementwise ops the reference runs as separate
// ATen kernels around them (PReLU, gLN apply, residual/skip adds, sigmoid, their backward forms).
// The weight gradients of the same layers: wgrad.hip.
//
// Kernels of this file, the first two ending in gemm_epilogue<EF> (gemm_common.hpp: LDS-transposed float4 epilogue with bias, PReLU
// statistics, residual / skip accumulate, sigmoid, PReLU backward, gLN-backward row sums):
//   pw_gemm_kernel                register-staged GEMM; fallback for contractions that are not a multiple of 16
//   pw_gemm_direct_kernel<...,AR> THE fast path, LDS-DMA ring, prologue (PReLU / gLN / gLN backward) on the B fragments.
//                                 AR = 2 (SEP_ARITH_F16X3, default): fp32 products by a scaled two-part fp16 split on
//                                 v_mfma_f32_32x32x16_f16 (one scale for A, one per column of X kept per lane);
//                                 AR = 1 (SEP_ARITH_BF16X6): fp32 products by exact three-way bf16 split on
//                                 v_mfma_f32_32x32x16_bf16; both: 3-stage ring, 3 workgroups per CU, whole-chunk steps;
//                                 AR = 0 (SEP_ARITH_F32): v_mfma_f32_32x32x2_f32, 2-stage ring, 4 workgroups per CU,
//                                 half-chunk software pipeline -- design notes at the kernel
//   pw_wgrad_kernel               register-staged weight gradient; fallback (g_mul = decoder basis gradient) of sep_pw_wgrad (wgrad.hip),
//                                 here because its generated code depends on pw_gemm_kernel's presence -- note at the kernel
// sep_pw_gemm, below the kernels, offers descriptors that carry packed weights to sep_pw_gemm_packed (gemm_coop.hip) first.
#include "gemm_common.hpp"
#include <stdlib.h>
#include <string.h>
#include <stddef.h>

namespace {

constexpr int BK = 32;       // contraction rows per chunk (forward / dgrad): 64 MFMAs per wave between barriers
constexpr int LDA_S = 132;   // allocated As[k][m] row stride (floats); 16B aligned rows for the float4 (transposed-A) writes
constexpr int LDA_NT = 129;  // row stride actually used by the non-transposed path: odd -> conflict-free transposing scalar writes
constexpr int LDB_S = 128;

struct __attribute__((aligned(16))) GemmSmem {
    float As[2][BK * LDA_S];
    float Bs[2][BK * LDB_S];
    double red[8];
};

__global__ __launch_bounds__(256, 2) void pw_gemm_kernel(const sep_gemm_desc d) {
    __shared__ GemmSmem sm;
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int wr = wid >> 1, wc = wid & 1;

    const int NR = (d.M + BM - 1) / BM;
    const int ntile_t = d.ldt / BN;
    const int NC = d.B * ntile_t;
    int rt, ct;                                     // row tile, (sample, column tile): all row tiles of one column tile on the same XCD
    if (!xcd_decode(blockIdx.x, NR, NC, rt, ct)) return;
    const int b = ct / ntile_t;
    const int t0 = (ct % ntile_t) * BN;
    const int m0 = rt * BM;
    if (t0 >= d.T && d.pro_mode != SEP_PRO_GLN_BWD) {
        // whole tile lies in the pad region: outputs are zero there (never read-modify-written)
        for (int i = tid; i < BM * (BN / 4); i += 256) {
            const int r = i / (BN / 4), c4 = i % (BN / 4);
            const int row = m0 + r;
            if (row >= d.M) continue;
            float* dst;
            size_t idx;
            if (d.m_split && row >= d.m_split) {
                dst = d.Y2; idx = ((size_t)b * (d.M - d.m_split) + (row - d.m_split)) * d.ldt;
            } else {
                dst = d.Y; idx = ((size_t)b * (d.m_split ? d.m_split : d.M) + row) * d.ldt;
            }
            st4(dst + idx + t0 + 4 * c4, make_float4(0.f, 0.f, 0.f, 0.f));
        }
        if (d.epi_flags & SEP_EPI_ROWSUMS) {
            for (int i = tid; i < BM * 2; i += 256) {
                const int row = m0 + (i >> 1);
                if (row < d.M) {
                    float* rp = d.epi_rowpart + (((size_t)b * d.M + row) * (d.ldt / 64) + (t0 / 64) + (i & 1)) * 2;
                    rp[0] = 0.f; rp[1] = 0.f;
                }
            }
        }
        return;
    }

    // ---- per-block prologue constants ------------------------------------------------
    float mu = 0.f, rstd = 1.f, alpha_p = 0.f, mg = 0.f, mgx = 0.f;
    const int pro = d.pro_mode;
    if (pro == SEP_PRO_GLN || pro == SEP_PRO_GLN_PRELU || pro == SEP_PRO_GLN_BWD) gln_mu_rstd(d.pro_stats + (size_t)b * SEP_STATS_SLOTS * 2, d.count, d.eps, mu, rstd);
    if (pro == SEP_PRO_PRELU || pro == SEP_PRO_GLN_PRELU || pro == SEP_PRO_GLN_BWD) alpha_p = d.pro_alpha[0];
    if (pro == SEP_PRO_GLN_BWD) {
        if (d.pro_bacc) gln_bwd_means(d.pro_bacc + (size_t)b * SEP_STATS_SLOTS * 2, d.pro_stats + (size_t)b * SEP_STATS_SLOTS * 2, d.count, d.eps, mg, mgx);
        else { mg = d.pro_bsum[2 * b]; mgx = d.pro_bsum[2 * b + 1]; }
    }
    float dalpha_pro = 0.f;

    // ---- thread -> staging coordinates -------------------------------------------------
    const int br = tid >> 5, bc4 = tid & 31;   // B tile: rows br + 8i (i<4) ; float4 column bc4
    const int am = tid >> 3, ak4 = tid & 7;    // A tile (non-trans): rows am + 32i (i<4) ; float4 along k
    const int nk = d.K / BK;
    const int lda_s = d.trans_a ? LDA_S : LDA_NT;

    float4 ra[4], rb[4], rx[4];
    float pgam[4], pbet[4];     // gLN affine of the rows being staged, fetched together with the tile (one chunk ahead)

    auto load_global = [&](int kc) {
        const int k0 = kc * BK;
        const float* Xs = d.X;
        const float* As_ = d.A;
        int krow = k0, Ksrc = d.K;
        bool second = false;
        if (d.k_split) {
            if (k0 >= d.k_split) { Xs = d.X2; As_ = d.A2; krow = k0 - d.k_split; Ksrc = d.K - d.k_split; second = true; }
            else { Ksrc = d.k_split; }
        }
        (void)second;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const size_t off = ((size_t)b * Ksrc + krow + br + 8 * i) * d.ldt + t0 + 4 * bc4;
            rb[i] = ld4(Xs + off);
            if (pro == SEP_PRO_GLN_BWD) rx[i] = ld4(d.pro_aux + off);
            if (pro >= SEP_PRO_GLN) {
                pgam[i] = d.pro_gamma[k0 + br + 8 * i];
                pbet[i] = (pro == SEP_PRO_GLN_BWD) ? 0.f : d.pro_beta[k0 + br + 8 * i];
            }
        }
        if (d.trans_a) {
            // A is [K][M]: row k, float4 along m
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int mm = m0 + 4 * bc4;
                if (mm < d.M) ra[i] = ld4(As_ + (size_t)(krow + br + 8 * i) * d.M + mm);
                else ra[i] = make_float4(0.f, 0.f, 0.f, 0.f);
            }
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int mm = m0 + am + 32 * i;
                if (mm < d.M) ra[i] = ld4(As_ + (size_t)mm * Ksrc + krow + 4 * ak4);
                else ra[i] = make_float4(0.f, 0.f, 0.f, 0.f);
            }
        }
    };

    auto store_lds = [&](int kc, int buf) {
        const int k0 = kc * BK;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            float v[4] = {rb[i].x, rb[i].y, rb[i].z, rb[i].w};
            const int kg = k0 + br + 8 * i;   // global contraction row (parameter index of gamma/beta)
            if (pro == SEP_PRO_PRELU) {
#pragma unroll
                for (int q = 0; q < 4; ++q) v[q] = prelu_f(v[q], alpha_p);
            } else if (pro == SEP_PRO_GLN || pro == SEP_PRO_GLN_PRELU) {
                const float sc = pgam[i] * rstd;
                const float sh = pbet[i] - mu * sc;
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const float u = (pro == SEP_PRO_GLN_PRELU) ? prelu_f(v[q], alpha_p) : v[q];
                    v[q] = u * sc + sh;
                }
            } else if (pro == SEP_PRO_GLN_BWD) {
                const float a4[4] = {rx[i].x, rx[i].y, rx[i].z, rx[i].w};
                const float gk = pgam[i];
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int t = t0 + 4 * bc4 + q;
                    const float a = a4[q];
                    const float u = prelu_f(a, alpha_p);
                    const float xh = (u - mu) * rstd;
                    const float du = rstd * (gk * v[q] - mg - xh * mgx);
                    float da = du * prelu_grad(a, alpha_p);
                    if (t >= d.T) da = 0.f;
                    else if (a <= 0.f && rt == 0) dalpha_pro += du * a;
                    v[q] = da;
                }
                if (rt == 0) {
                    const size_t off = ((size_t)b * d.K + kg) * d.ldt + t0 + 4 * bc4;
                    st4(d.pro_store + off, make_float4(v[0], v[1], v[2], v[3]));
                }
            }
            st4(&sm.Bs[buf][(br + 8 * i) * LDB_S + 4 * bc4], make_float4(v[0], v[1], v[2], v[3]));
        }
        if (d.trans_a) {
#pragma unroll
            for (int i = 0; i < 4; ++i) st4(&sm.As[buf][(br + 8 * i) * LDA_S + 4 * bc4], ra[i]);
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int mm = am + 32 * i;
                sm.As[buf][(4 * ak4 + 0) * LDA_NT + mm] = ra[i].x;
                sm.As[buf][(4 * ak4 + 1) * LDA_NT + mm] = ra[i].y;
                sm.As[buf][(4 * ak4 + 2) * LDA_NT + mm] = ra[i].z;
                sm.As[buf][(4 * ak4 + 3) * LDA_NT + mm] = ra[i].w;
            }
        }
    };

    f32x16 acc[2][2];
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int ni = 0; ni < 2; ++ni)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[mi][ni][r] = 0.f;

    load_global(0);
    store_lds(0, 0);
    __syncthreads();

    const int lk = lane >> 5, l31 = lane & 31;
    for (int kc = 0; kc < nk; ++kc) {
        const int cur = kc & 1;
        if (kc + 1 < nk) load_global(kc + 1);
        mfma_chunk32(sm.As[cur], lda_s, sm.Bs[cur], LDB_S, wr * 64 + l31, wc * 64 + l31, lk, acc[0][0], acc[0][1], acc[1][0], acc[1][1]);
        if (kc + 1 < nk) store_lds(kc + 1, cur ^ 1);
        __syncthreads();
    }

    __syncthreads();                                    // K-loop LDS reads are done: the staging area becomes the transpose buffer
    #ifdef SEP_PROF
    const int prof_slot = -1;
#endif
    gemm_epilogue<-1>(d, acc, b, m0, t0, wr, wc, lk, l31, tid, &sm.As[0][0], sm.red, BN, true PROF_PASS);
    if (pro == SEP_PRO_GLN_BWD && rt == 0) {
        const double s = block_sum_256<double>((double)dalpha_pro, sm.red);
        if (tid == 0) atomicAdd(d.pro_dalpha, s);
    }
}



// ======================================================================================
// The fast GEMM: direct-to-LDS, 2-stage ring, high occupancy.
//
// Why this shape (all measured on MI355X, tools/gemm_bench.py + rocprofv3):
//  * a register-staged kernel (above, kept for odd shapes) is latency-bound: removing all its MFMAs shortened it by < 35 %;
//  * a 4-stage DMA ring with counted vmcnt, fragment double-buffering and a hand-ordered instruction stream reached
//    120 TF/s on long contractions but only 65 TF/s at K = 128, and 1 -> 2 workgroups per CU was worth +25...45 %:
//    a wave issues in order, so while it runs its DMA issue / ds_reads / prologue / epilogue the matrix pipe needs
//    OTHER waves.  Trading ring depth and register double-buffering for occupancy (2 stages = 32 KiB LDS, <= 128
//    VGPRs => FOUR workgroups per CU) beat that kernel on every shape of the model, with far simpler code;
//  * with one chunk of lead (a chunk's DMA is issued one MFMA burst x 4 co-resident waves before it is needed) the
//    waits are plain vmcnt(0), so other memory traffic in flight (epilogue stores, the gLN-backward store-back) is harmless.
//
//   A k-major ([K][M], input-gradient form): rows DMA'd verbatim, fragments by conflict-free ds_read_b32.
//   A row-major ([M][K], forward form): 16-byte granules DMA'd with an XOR swizzle on the SOURCE address (the LDS image
//   of a DMA is lane-linear), fragments by two ds_read_b128 per 32-row block; the contraction index is permuted (lane
//   half lk owns k = 8*lk .. 8*lk+7 of the chunk) identically for A and B, which a sum allows.
//   The elementwise prologue acts on the B fragments after the ds_read; its per-row affine sits in LDS.
//   PRO == GLN_BWD streams a third operand (the pre-activation a), forms d(pre-activation) on the fragments, and the
//   wr == 0 waves of row tile 0 write it back for the weight-gradient GEMM and accumulate the PReLU slope gradient.
// ======================================================================================
constexpr int OMAXK = 512;      // rows of the per-row affine table in LDS (3 stages x 3 workgroups per CU must fit 160 KiB)

template <bool AUX, int NS = 2>
struct __attribute__((aligned(16))) DirectSmem {
    float As[NS][DK * 128];
    float Bs[NS][DK * 128];
    float Cs[AUX ? 2 : 1][AUX ? DK * 128 : 4];
    float sc[OMAXK];
    float sh[AUX ? 4 : OMAXK];
    double red[8];
};

#ifndef SEP_GLN_OCC
#define SEP_GLN_OCC 4       // measured: 4 blocks/CU with ~40 B of spill (outside the hot loop) = 3 blocks/CU spill-free (182 vs 186 us on the heads GEMM)
#endif
// AR selects the arithmetic of the contraction:
//   0  v_mfma_f32_32x32x2_f32 on the fp32 fragments (157 TF/s peak).
//   1  fp32 by exact three-way bf16 splitting: every fragment value x = hi + mid + lo with each part a truncated bf16
//      (8 + 8 + 8 significand bits: the sum is EXACT), and x*y = hi*hi + hi*mid + mid*hi + mid*mid + hi*lo + lo*hi
//      (+ three terms <= 2^-24 |xy| that are dropped) on v_mfma_f32_32x32x16_bf16 with fp32 accumulation: 6 MFMAs of
//      32 cycles per 16-deep chunk and tile pair instead of 8 of 64.  Error per product <= 2^-23 relative, i.e. the
//      rounding of an fp32 multiply; measured against fp64 it is no worse than the fp32 MFMA path (tests).  The
//      lane half lk already owns k = 8*lk .. 8*lk+7 of a chunk, which is the operand layout of the bf16 instruction.
//      (split3_pair, split3_frag, mfma_split6 and mfma_bf16: gemm_common.hpp)

template <bool TRANS_A, int PRO, bool SPLIT, int EF, int AR = 0>
__global__ __launch_bounds__(256, (AR >= 1 ? 3 : PRO == SEP_PRO_GLN_BWD ? 3 : PRO >= SEP_PRO_GLN ? SEP_GLN_OCC : 4)) void pw_gemm_direct_kernel(const sep_gemm_desc d) {
    constexpr bool P_PRELU = PRO == SEP_PRO_PRELU || PRO == SEP_PRO_GLN_PRELU;
    constexpr bool P_GLN = PRO == SEP_PRO_GLN || PRO == SEP_PRO_GLN_PRELU;
    constexpr bool P_BWD = PRO == SEP_PRO_GLN_BWD;
    static_assert(AR == 0 || PRO != SEP_PRO_GLN_BWD, "the split arithmetic has no GLN_BWD form");
    constexpr int NS = AR >= 1 ? 3 : 2;          // ring depth: the split paths consume a chunk ~3x faster, so they prefetch two ahead          // ring depth: the bf16 path consumes a chunk ~3x faster, so it prefetches two ahead
    __shared__ DirectSmem<P_BWD, NS> sm;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);   // provably wave-uniform: the DMA's LDS base goes to M0 without a waterfall loop
    const int wr = wid >> 1, wc = wid & 1;
    const int lk = lane >> 5, l31 = lane & 31;

    const int NR = (d.M + BM - 1) / BM;
    const int ntile_t = d.ldt / BN;
    const int NC = d.B * ntile_t;
    const int bid = blockIdx.x;
    int rt, ct;                                     // row tile, (sample, column tile): all row tiles of one column tile share X through one XCD's L2
    if (!xcd_decode(bid, NR, NC, rt, ct)) return;
    const int b = ct / ntile_t;
    const int t0 = (ct % ntile_t) * BN;
    const int m0 = rt * BM;
    const int nk = d.K / DK;
#ifdef SEP_PROF
    const int prof_slot = bid == 8 ? 0 : bid == 1500 ? 1 : bid == 1501 ? 2 : bid == (int)gridDim.x - 9 ? 3 : -1;
#endif
    PROF_STAMP(0);
#ifdef SEP_PROF
    if (tid == 0 && bid < 8192) g_blk_start[bid] = wall_clock64();
#endif

    // per-row affine of the prologue, once per workgroup
    float alpha_p = 0.f, mu = 0.f, rstd = 1.f, mg = 0.f, mgx = 0.f;
    if (P_PRELU || P_BWD) alpha_p = d.pro_alpha[0];
    if (P_GLN || P_BWD) {
        gln_mu_rstd(d.pro_stats + (size_t)b * SEP_STATS_SLOTS * 2, d.count, d.eps, mu, rstd);
        for (int k = tid; k < d.K; k += 256) {
            if (P_BWD) sm.sc[k] = d.pro_gamma[k];
            else {
                const float scv = d.pro_gamma[k] * rstd;
                sm.sc[k] = scv;
                sm.sh[k] = d.pro_beta[k] - mu * scv;
            }
        }
    }
    if (P_BWD) {
        if (d.pro_bacc) gln_bwd_means(d.pro_bacc + (size_t)b * SEP_STATS_SLOTS * 2, d.pro_stats + (size_t)b * SEP_STATS_SLOTS * 2, d.count, d.eps, mg, mgx);
        else { mg = d.pro_bsum[2 * b]; mgx = d.pro_bsum[2 * b + 1]; }
    }
    float dalpha_pro = 0.f;
    const bool writer = P_BWD && wr == 0 && rt == 0;           // the waves that own the store-back / slope gradient

    // This wave's share of one stage: 2 DMA instructions per operand (1 KiB each).  Every source address is a
    // wave-uniform base (SGPR pair, advanced with scalar adds: chunks are issued strictly in order) plus a per-lane
    // 32-bit offset fixed for the whole tile.
    const int Ks1 = SPLIT ? d.k_split : d.K;
    const int split_chunk = SPLIT ? d.k_split / DK : -1;
    const size_t stepB = (size_t)DK * d.ldt;
    const size_t stepA = TRANS_A ? (size_t)DK * d.M : (size_t)DK;
    const float* baseB[2];
    const float* baseC[2];
    const float* baseA[2];
    unsigned offA[2];                                             // BYTE offsets, unsigned: base(SGPR pair) + zext(voffset) is the
    const unsigned offB = 4u * (unsigned)(lk * d.ldt + 4 * l31);   // saddr form of global_load_lds (one VGPR, no 64-bit VALU add)
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        const int r2 = 4 * wid + 2 * q;                           // first of the two k rows this instruction covers
        baseB[q] = d.X + ((size_t)b * Ks1 + r2) * d.ldt + t0;
        baseC[q] = P_BWD ? d.pro_aux + ((size_t)b * Ks1 + r2) * d.ldt + t0 : nullptr;
        if (TRANS_A) {
            int mm = m0 + 4 * l31;
            if (mm > d.M - 4) mm = d.M - 4;                       // rows past M are never stored; keep the read in bounds
            baseA[q] = d.A + (size_t)r2 * d.M;
            offA[q] = 4u * (unsigned)(lk * d.M + mm);
        } else {
            // [128 m][16 k] image, 64-byte rows; instruction covers 16 rows; granule p of row r holds k-chunk p ^ ((r>>2)&3)
            const int r = lane >> 2, pch = lane & 3;
            int mm = m0 + 16 * (2 * wid + q) + r;
            if (mm > d.M - 1) mm = d.M - 1;
            baseA[q] = d.A;
            offA[q] = 4u * (unsigned)(mm * Ks1 + 4 * (pch ^ ((r >> 2) & 3)));
        }
    }
    int kci = 0;                                                  // next chunk to issue
    auto issue = [&](const int stage) {
        if (SPLIT && kci == split_chunk) {                        // uniform, taken once per tile: switch to the second source
            const int Ks2 = d.K - d.k_split;
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                const int r2 = 4 * wid + 2 * q;
                baseB[q] = d.X2 + ((size_t)b * Ks2 + r2) * d.ldt + t0;
                if (TRANS_A) baseA[q] = d.A2 + (size_t)r2 * d.M;
                else {
                    const int r = lane >> 2, pch = lane & 3;
                    int mm = m0 + 16 * (2 * wid + q) + r;
                    if (mm > d.M - 1) mm = d.M - 1;
                    baseA[q] = d.A2;
                    offA[q] = 4u * (unsigned)(mm * Ks2 + 4 * (pch ^ ((r >> 2) & 3)));
                }
            }
        }
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            glds16_asm(baseB[q], offB, lds_addr(&sm.Bs[stage][(4 * wid + 2 * q) * 128]));
            if (P_BWD) glds16_asm(baseC[q], offB, lds_addr(&sm.Cs[stage][(4 * wid + 2 * q) * 128]));
            glds16_asm(baseA[q], offA[q], lds_addr(TRANS_A ? &sm.As[stage][(4 * wid + 2 * q) * 128] : &sm.As[stage][(2 * wid + q) * 256]));
            baseB[q] += stepB;
            if (P_BWD) baseC[q] += stepB;
            baseA[q] += stepA;
        }
        ++kci;
    };

    f32x16 acc[2][2];
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int ni = 0; ni < 2; ++ni)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[mi][ni][r] = 0.f;

    // Software pipeline at half-chunk granularity.  On a SIMD the co-resident waves share the matrix pipe fairly, so they
    // run in lockstep and reach their barriers / LDS reads TOGETHER: whatever a wave does between two MFMA bursts is pipe
    // idle time for all of them (measured: MFMA idle ~= SQ_WAIT_ANY + non-MFMA issue).  So each wave keeps its own MFMA
    // stream dense: the fragments of half h+1 are read from LDS while the 16 MFMAs of half h run, and the per-chunk
    // barrier sits between two bursts with the next burst's operands already in registers.  Same 32 fragment registers.
    float fa[2][2][4], fb[2][2][4];      // [half][mi|ni][kk]
    float fc[2][2][4];                   // GLN_BWD: the pre-activation fragments
    float fs[2][4], fh[2][4];            // gLN prologues: the per-row scale / shift of the half's four k
    auto read_half = [&](const int stage, const int h, const int kc) {
        const float* Ab = sm.As[stage];
        const float* Bb = sm.Bs[stage];
        if (TRANS_A) {
#pragma unroll
            for (int kk = 0; kk < 4; ++kk) {
                fa[h][0][kk] = Ab[(8 * lk + 4 * h + kk) * 128 + wr * 64 + l31];
                fa[h][1][kk] = Ab[(8 * lk + 4 * h + kk) * 128 + wr * 64 + 32 + l31];
            }
        } else {
#pragma unroll
            for (int mi = 0; mi < 2; ++mi) {
                const int m = wr * 64 + mi * 32 + l31;
                const float* p = Ab + m * 16 + 4 * ((2 * lk + h) ^ ((m >> 2) & 3));
#pragma unroll
                for (int e = 0; e < 4; ++e) fa[h][mi][e] = p[e];
            }
        }
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) {
            fb[h][0][kk] = Bb[(8 * lk + 4 * h + kk) * 128 + wc * 64 + l31];
            fb[h][1][kk] = Bb[(8 * lk + 4 * h + kk) * 128 + wc * 64 + 32 + l31];
        }
        if (P_BWD) {
            const float* Cb = sm.Cs[stage];
#pragma unroll
            for (int kk = 0; kk < 4; ++kk) {
                fc[h][0][kk] = Cb[(8 * lk + 4 * h + kk) * 128 + wc * 64 + l31];
                fc[h][1][kk] = Cb[(8 * lk + 4 * h + kk) * 128 + wc * 64 + 32 + l31];
            }
        }
        if (P_GLN || P_BWD) {
            const int kbase = kc * DK + 8 * lk + 4 * h;
#pragma unroll
            for (int kk = 0; kk < 4; ++kk) {
                fs[h][kk] = sm.sc[kbase + kk];
                if (P_GLN) fh[h][kk] = sm.sh[kbase + kk];
            }
        }
        __builtin_amdgcn_sched_barrier(0);      // the reads stay HERE: ahead of the MFMA burst that hides their latency
    };
    const bool live0 = t0 + wc * 64 + l31 < d.T, live1 = t0 + wc * 64 + 32 + l31 < d.T;
    const unsigned st_lane_off = 4u * (unsigned)(8 * lk * d.ldt + l31);      // GLN_BWD store-back: this lane's byte offset in the chunk
    auto apply_pro = [&](const int kc, const int h, const int kk) {
        if (P_BWD) {
            // d(pre-activation) = rstd*(gamma_k*dv - mg - xhat*mgx) * PReLU'(a)   on the fragments
            const float gk = fs[h][kk];
#pragma unroll
            for (int ni = 0; ni < 2; ++ni) {
                const bool live = ni ? live1 : live0;
                const float a = fc[h][ni][kk];
                const float u = prelu_f(a, alpha_p);
                const float xh = (u - mu) * rstd;
                const float du = rstd * (gk * fb[h][ni][kk] - mg - xh * mgx);
                const float da = live ? du * prelu_grad(a, alpha_p) : 0.f;
                fb[h][ni][kk] = da;
                if (writer) {
                    if (live && a <= 0.f) dalpha_pro += du * a;
                    // uniform row pointer (SGPR pair) + per-lane byte offset: the saddr form of global_store
                    float* srow = d.pro_store + ((size_t)b * d.K + kc * DK + 4 * h + kk) * d.ldt + t0 + wc * 64 + ni * 32;
                    *reinterpret_cast<float*>(reinterpret_cast<char*>(srow) + (size_t)st_lane_off) = da;
                }
            }
        } else if (PRO != SEP_PRO_NONE) {
            const float scv = P_GLN ? fs[h][kk] : 1.f;
            const float shv = P_GLN ? fh[h][kk] : 0.f;
#pragma unroll
            for (int ni = 0; ni < 2; ++ni) {
                float v = fb[h][ni][kk];
                if (P_PRELU) v = prelu_f(v, alpha_p);
                fb[h][ni][kk] = P_GLN ? v * scv + shv : v;
            }
        }
    };
    auto mfma_half = [&](const int kc, const int h) {
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) {
            apply_pro(kc, h, kk);
            acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[h][0][kk], fb[h][0][kk], acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[h][0][kk], fb[h][1][kk], acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[h][1][kk], fb[h][0][kk], acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[h][1][kk], fb[h][1][kk], acc[1][1], 0, 0, 0);
        }
    };
    // AR == 1: whole-chunk steps.  prologue + split of chunk kc (VALU), then -- behind the barrier that says chunk kc+1 has
    // landed -- the LDS reads of chunk kc+1 in three portions between the four groups of six bf16 MFMAs of chunk kc, so
    // that no more than one portion of raw fragments is live beside the 48 packed operand registers.
    auto read_a6 = [&](const int stage) {
        const float* Ab = sm.As[stage];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            if (TRANS_A) {
#pragma unroll
                for (int kk = 0; kk < 4; ++kk) {
                    fa[h][0][kk] = Ab[(8 * lk + 4 * h + kk) * 128 + wr * 64 + l31];
                    fa[h][1][kk] = Ab[(8 * lk + 4 * h + kk) * 128 + wr * 64 + 32 + l31];
                }
            } else {
#pragma unroll
                for (int mi = 0; mi < 2; ++mi) {
                    const int m = wr * 64 + mi * 32 + l31;
                    const float* p = Ab + m * 16 + 4 * ((2 * lk + h) ^ ((m >> 2) & 3));
#pragma unroll
                    for (int e = 0; e < 4; ++e) fa[h][mi][e] = p[e];
                }
            }
        }
    };
    auto read_b6 = [&](const int stage, const int ni) {
        const float* Bb = sm.Bs[stage];
        const float* Cb = sm.Cs[P_BWD ? stage : 0];
#pragma unroll
        for (int h = 0; h < 2; ++h)
#pragma unroll
            for (int kk = 0; kk < 4; ++kk) {
                fb[h][ni][kk] = Bb[(8 * lk + 4 * h + kk) * 128 + wc * 64 + ni * 32 + l31];
                if (P_BWD) fc[h][ni][kk] = Cb[(8 * lk + 4 * h + kk) * 128 + wc * 64 + ni * 32 + l31];
            }
    };
    auto step6 = [&](const int kc, const int stage, const int nstage) {
        u32x4_t pa[2][3], pb[2][3];
        if (P_GLN || P_BWD) {
#pragma unroll
            for (int h = 0; h < 2; ++h)
#pragma unroll
                for (int kk = 0; kk < 4; ++kk) {
                    fs[h][kk] = sm.sc[kc * DK + 8 * lk + 4 * h + kk];
                    if (P_GLN) fh[h][kk] = sm.sh[kc * DK + 8 * lk + 4 * h + kk];
                }
        }
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            split3_frag(fa[0][i], fa[1][i], pa[i]);
        }
#pragma unroll
        for (int h = 0; h < 2; ++h)
#pragma unroll
            for (int kk = 0; kk < 4; ++kk) apply_pro(kc, h, kk);
#pragma unroll
        for (int i = 0; i < 2; ++i) split3_frag(fb[0][i], fb[1][i], pb[i]);
        __builtin_amdgcn_sched_barrier(0);
        const bool more = kc + 1 < nk;
        if (more) {
            // chunk kc+1 has landed (mine: all but the DMAs of chunk kc+2; everyone's: barrier), and every wave is past
            // its reads of chunk kc's stage, which chunk kc+NS now overwrites
            wait_keep4_and_barrier(NS == 3 && kc + 2 < nk);
            if (kc + NS < nk) issue(stage);
            read_a6(nstage);
        }
        __builtin_amdgcn_sched_barrier(0);
        mfma_split6(pa[0], pb[0], acc[0][0]);
        mfma_split6(pa[1], pb[0], acc[1][0]);
        __builtin_amdgcn_sched_barrier(0);
        if (more) read_b6(nstage, 0);
        __builtin_amdgcn_sched_barrier(0);
        mfma_split6(pa[0], pb[1], acc[0][1]);
        mfma_split6(pa[1], pb[1], acc[1][1]);
        __builtin_amdgcn_sched_barrier(0);
        if (more) read_b6(nstage, 1);
        __builtin_amdgcn_sched_barrier(0);
    };
    int bexp[2] = {0, 0};                // per-lane scale exponent of this lane's column in column block ni
    bool bset[2] = {false, false};       // ... chosen yet?  (a column stays unset while it has only seen zeros)
    int aexp = 0;                        // A * 2^aexp < 2^13
    if (AR == 2) aexp = 13 - __builtin_amdgcn_frexp_expf(__builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, d.a_amax[0]))));
    auto step3h = [&](const int kc, const int stage, const int nstage) {
        u32x4_t pa[2][2], pb[2][2];
        if (P_GLN) {
#pragma unroll
            for (int h = 0; h < 2; ++h)
#pragma unroll
                for (int kk = 0; kk < 4; ++kk) {
                    fs[h][kk] = sm.sc[kc * DK + 8 * lk + 4 * h + kk];
                    fh[h][kk] = sm.sh[kc * DK + 8 * lk + 4 * h + kk];
                }
        }
#pragma unroll
        for (int i = 0; i < 2; ++i) {
#pragma unroll
            for (int h = 0; h < 2; ++h)
#pragma unroll
                for (int kk = 0; kk < 4; ++kk) fa[h][i][kk] = __builtin_ldexpf(fa[h][i][kk], aexp);
            split2_frag(fa[0][i], fa[1][i], pa[i]);
        }
#pragma unroll
        for (int h = 0; h < 2; ++h)
#pragma unroll
            for (int kk = 0; kk < 4; ++kk) apply_pro(kc, h, kk);
#pragma unroll
        for (int ni = 0; ni < 2; ++ni) {
            float m = 0.f;
#pragma unroll
            for (int h = 0; h < 2; ++h)
#pragma unroll
                for (int kk = 0; kk < 4; ++kk) m = fmaxf(m, fabsf(fb[h][ni][kk]));
            m = fmaxf(m, __shfl_xor(m, 32, 64));                          // the other lane half holds the column's other 8 k
            const int e = __builtin_amdgcn_frexp_expf(m);                  // m = f * 2^e, f in [0.5, 1)
            const bool grow = m > 0.f && (!bset[ni] || e + bexp[ni] > 14);      // first non-zero chunk, or the column outgrew its scale
            bset[ni] = bset[ni] || m > 0.f;
            const int nexp = grow ? 9 - e : bexp[ni];
            if (__builtin_amdgcn_ballot_w64(grow) != 0) {                  // rare after the first chunks
                const int delta = nexp - bexp[ni];
#pragma unroll
                for (int mi = 0; mi < 2; ++mi)
#pragma unroll
                    for (int r = 0; r < 16; ++r) acc[mi][ni][r] = __builtin_ldexpf(acc[mi][ni][r], delta);
            }
            bexp[ni] = nexp;
#pragma unroll
            for (int h = 0; h < 2; ++h)
#pragma unroll
                for (int kk = 0; kk < 4; ++kk) fb[h][ni][kk] = __builtin_ldexpf(fb[h][ni][kk], nexp);
            split2_frag(fb[0][ni], fb[1][ni], pb[ni]);
        }
        __builtin_amdgcn_sched_barrier(0);
        const bool more = kc + 1 < nk;
        if (more) {
            wait_keep4_and_barrier(NS == 3 && kc + 2 < nk);
            if (kc + NS < nk) issue(stage);
            read_a6(nstage);
        }
        __builtin_amdgcn_sched_barrier(0);
        mfma_split3(pa[0], pb[0], acc[0][0]);
        mfma_split3(pa[1], pb[0], acc[1][0]);
        __builtin_amdgcn_sched_barrier(0);
        if (more) read_b6(nstage, 0);
        __builtin_amdgcn_sched_barrier(0);
        mfma_split3(pa[0], pb[1], acc[0][1]);
        mfma_split3(pa[1], pb[1], acc[1][1]);
        __builtin_amdgcn_sched_barrier(0);
        if (more) read_b6(nstage, 1);
        __builtin_amdgcn_sched_barrier(0);
    };
    auto step = [&](const int kc, const int stage) {
        read_half(stage, 1, kc);
        mfma_half(kc, 0);
        __builtin_amdgcn_sched_barrier(0);
        if (kc + 1 < nk) {
            // chunk kc+1 has landed (mine: vmcnt(0); everyone's: barrier) and every wave is past its reads of this stage
            wait_all_and_barrier();
            if (kc + 2 < nk) issue(stage);
            read_half(stage ^ 1, 0, kc + 1);
        }
        mfma_half(kc, 1);
        __builtin_amdgcn_sched_barrier(0);
    };

    PROF_STAMP(1);
    issue(0);
    if (NS == 3 && nk > 1) {
        issue(1);
        wait_keep4_and_barrier(true);
        if (nk > 2) issue(2);
    } else {
        wait_all_and_barrier();
        if (nk > 1) issue(1);
    }
    PROF_STAMP(2);
    if (AR == 0) read_half(0, 0, 0);
    int kc = 0;
    if (AR == 2) {
        read_a6(0);
        read_b6(0, 0);
        read_b6(0, 1);
        for (; kc + 2 < nk; kc += 3) {
            step3h(kc, 0, 1);
            step3h(kc + 1, 1, 2);
            step3h(kc + 2, 2, 0);
        }
        if (kc < nk) step3h(kc, 0, 1);
        if (kc + 1 < nk) step3h(kc + 1, 1, 2);
        // undo the scales: 2^aexp of A, 2^bexp of this lane's column
#pragma unroll
        for (int mi = 0; mi < 2; ++mi)
#pragma unroll
            for (int ni = 0; ni < 2; ++ni)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[mi][ni][r] = __builtin_ldexpf(acc[mi][ni][r], -aexp - bexp[ni]);
    } else if (AR == 1) {
        read_a6(0);
        read_b6(0, 0);
        read_b6(0, 1);
        if (NS == 3) {
            for (; kc + 2 < nk; kc += 3) {
                step6(kc, 0, 1);
                step6(kc + 1, 1, 2);
                step6(kc + 2, 2, 0);
            }
            if (kc < nk) step6(kc, 0, 1);
            if (kc + 1 < nk) step6(kc + 1, 1, 2);
        } else {
            for (; kc + 1 < nk; kc += 2) {
                step6(kc, 0, 1);
                step6(kc + 1, 1, 0);
            }
            if (kc < nk) step6(kc, 0, 1);
        }
    } else {
        for (; kc + 1 < nk; kc += 2) {       // two steps per trip so the stage index is a literal
            step(kc, 0);
            step(kc + 1, 1);
        }
        if (kc < nk) step(kc, 0);
    }
    PROF_STAMP(3);
    __syncthreads();
    PROF_STAMP(4);
    // Launder the thread id: everything the epilogue derives from it (lane offsets, row pointers) would otherwise be
    // hoisted above the main loop as loop-invariant and held in registers through it -- at 128 VGPRs that spilled INSIDE
    // the loop (a scratch reload waits on vmcnt, i.e. on the DMA ring).
    int etid = tid, eb = b, em0 = m0, et0 = t0;
    asm volatile("" : "+v"(etid), "+s"(eb), "+s"(em0), "+s"(et0));
    const int ewid = __builtin_amdgcn_readfirstlane(etid >> 6);
    const int elane = etid & 63;
    gemm_epilogue<EF>(d, acc, eb, em0, et0, ewid >> 1, ewid & 1, elane >> 5, elane & 31, etid, &sm.As[0][0], sm.red, BN, true PROF_PASS);
    PROF_STAMP(5);
    if (P_BWD && rt == 0) {
        const double sdal = block_sum_256<double>((double)dalpha_pro, sm.red);
        if (tid == 0) atomicAdd(d.pro_dalpha, sdal);
    }
#ifdef SEP_PROF
    __builtin_amdgcn_s_waitcnt(0x0070);
#endif
    PROF_STAMP(6);
#ifdef SEP_PROF
    if (tid == 0 && bid < 8192) g_blk_end[bid] = wall_clock64();
#endif
}

// ======================================================================================
// The register-staged weight gradient: the reduction over the (sample, frame) columns of slab s, in the staging scheme of pw_gemm_kernel.
// It is kept in this file, beside that kernel, because hipcc generates other code for it in a translation unit without pw_gemm_kernel
// (seven address instructions fewer, registers renumbered; profiles/r21_gemm_files_ab.json has the timing that decided it).
// sep_pw_wgrad (wgrad.hip) reaches it through sep_pw_wgrad_staged below.
// ======================================================================================
constexpr int LDW_S = 129;  // k-major LDS row stride: odd -> conflict-free transposing writes AND fragment reads

struct __attribute__((aligned(16))) WgradSmem {
    float Gs[2][WK * LDW_S];
    float Xs[2][WK * LDW_S];
};

__global__ __launch_bounds__(256, 2) void pw_wgrad_kernel(const sep_wgrad_desc d) {
    __shared__ WgradSmem sm;
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int wr = wid >> 1, wc = wid & 1;
    const int ntm = (d.M + BM - 1) / BM, ntn = (d.N + BN - 1) / BN;
    const int ntiles = ntm * ntn;
    int tile, s;                                  // output tile, slab: all tiles of one slab on the same XCD
    if (!xcd_decode(blockIdx.x, ntiles, d.nsplit, tile, s)) return;
    const int m0 = (tile / ntn) * BM, n0 = (tile % ntn) * BN;

    const int cps_t = d.ldt / WK;                 // chunks per sample
    const long chunks_total = (long)d.B * cps_t;
    const long cper = slab_cper(chunks_total, d.nsplit, false);      // (not slab_chunks: the loops below run on c_end, and through it this kernel's generated code changes)
    const long c_begin = (long)s * cper;
    long c_end = c_begin + cper;
    if (c_end > chunks_total) c_end = chunks_total;

    const int lr = tid >> 3, lc4 = tid & 7;       // staging: rows lr + 32*i (i<4), float4 column lc4
    const bool do_bias = d.partial_bias != nullptr && (tile % ntn) == 0;
    float bias_acc = 0.f;

    const float alpha_x = (d.x_mode == SEP_PRO_PRELU || d.x_mode == SEP_PRO_GLN_PRELU) ? d.x_alpha[0] : 0.f;
    float4 rg[4], rx[4];
    float xsc[4], xsh[4];
    int stat_b = -1;            // sample whose gLN constants are cached below
    float stat_mu = 0.f, stat_rstd = 1.f;
    float xgam[4] = {0.f, 0.f, 0.f, 0.f}, xbet[4] = {0.f, 0.f, 0.f, 0.f};   // rows are fixed per thread: fetch once
    if (d.x_mode == SEP_PRO_GLN || d.x_mode == SEP_PRO_GLN_PRELU) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int n = n0 + lr + 32 * i;
            if (n < d.N) { xgam[i] = d.x_gamma[n]; xbet[i] = d.x_beta[n]; }
        }
    }

    auto chunk_valid = [&](long c) -> bool { return (int)(c % cps_t) * WK < d.T; };

    auto load_global = [&](long c) {
        const int b = (int)(c / cps_t);
        const int t0 = (int)(c % cps_t) * WK;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int m = m0 + lr + 32 * i;
            float4 g = make_float4(0.f, 0.f, 0.f, 0.f);
            if (m < d.M) {
                const float* src;
                size_t off;
                if (d.g_split && m >= d.g_split) { src = d.G2; off = ((size_t)b * (d.M - d.g_split) + (m - d.g_split)) * d.ldt; }
                else { src = d.G; off = ((size_t)b * (d.g_split ? d.g_split : d.M) + m) * d.ldt; }
                g = ld4(src + off + t0 + 4 * lc4);
                if (d.g_mul) {
                    const float4 w = ld4(d.Gaux + ((size_t)(b / d.g_div) * d.M + m) * d.ldt + t0 + 4 * lc4);
                    g.x *= w.x; g.y *= w.y; g.z *= w.z; g.w *= w.w;
                }
            }
            rg[i] = g;
            const int n = n0 + lr + 32 * i;
            float4 x = make_float4(0.f, 0.f, 0.f, 0.f);
            xsc[i] = 0.f; xsh[i] = 0.f;
            if (n < d.N) {
                const int bx = b / d.x_div;
                x = ld4(d.X + ((size_t)bx * d.N + n) * d.ldt + t0 + 4 * lc4);
                if (d.x_mode == SEP_PRO_GLN || d.x_mode == SEP_PRO_GLN_PRELU) {
                    if (bx != stat_b) { gln_mu_rstd(d.x_stats + (size_t)bx * SEP_STATS_SLOTS * 2, d.count, d.eps, stat_mu, stat_rstd); stat_b = bx; }
                    xsc[i] = xgam[i] * stat_rstd;
                    xsh[i] = xbet[i] - stat_mu * xsc[i];
                }
            }
            rx[i] = x;
        }
    };

    auto store_lds = [&](int buf) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int mm = lr + 32 * i;
            sm.Gs[buf][(4 * lc4 + 0) * LDW_S + mm] = rg[i].x;
            sm.Gs[buf][(4 * lc4 + 1) * LDW_S + mm] = rg[i].y;
            sm.Gs[buf][(4 * lc4 + 2) * LDW_S + mm] = rg[i].z;
            sm.Gs[buf][(4 * lc4 + 3) * LDW_S + mm] = rg[i].w;
            float v[4] = {rx[i].x, rx[i].y, rx[i].z, rx[i].w};
            const bool row_ok = (n0 + mm) < d.N;
            if (d.x_mode == SEP_PRO_PRELU) {
#pragma unroll
                for (int q = 0; q < 4; ++q) v[q] = prelu_f(v[q], alpha_x);
            } else if (d.x_mode == SEP_PRO_GLN || d.x_mode == SEP_PRO_GLN_PRELU) {
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const float u = (d.x_mode == SEP_PRO_GLN_PRELU) ? prelu_f(v[q], alpha_x) : v[q];
                    v[q] = row_ok ? (u * xsc[i] + xsh[i]) : 0.f;
                }
            }
            sm.Xs[buf][(4 * lc4 + 0) * LDW_S + mm] = v[0];
            sm.Xs[buf][(4 * lc4 + 1) * LDW_S + mm] = v[1];
            sm.Xs[buf][(4 * lc4 + 2) * LDW_S + mm] = v[2];
            sm.Xs[buf][(4 * lc4 + 3) * LDW_S + mm] = v[3];
        }
    };

    f32x16 acc[2][2];
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int ni = 0; ni < 2; ++ni)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[mi][ni][r] = 0.f;

    // skip chunks that lie entirely in the zero pad (G is exactly 0 there)
    long c = c_begin;
    while (c < c_end && !chunk_valid(c)) ++c;
    const int lk = lane >> 5, l31 = lane & 31;
    int cur = 0;
    if (c < c_end) {
        load_global(c);
        store_lds(0);
    }
    __syncthreads();
    while (c < c_end) {
        long cn = c + 1;
        while (cn < c_end && !chunk_valid(cn)) ++cn;
        if (cn < c_end) load_global(cn);
        mfma_chunk32(sm.Gs[cur], LDW_S, sm.Xs[cur], LDW_S, wr * 64 + l31, wc * 64 + l31, lk, acc[0][0], acc[0][1], acc[1][0], acc[1][1]);
        if (do_bias && tid < BM) {
            float sacc = 0.f;
#pragma unroll 8
            for (int k = 0; k < WK; ++k) sacc += sm.Gs[cur][k * LDW_S + tid];
            bias_acc += sacc;
        }
        if (cn < c_end) store_lds(cur ^ 1);
        __syncthreads();
        cur ^= 1;
        c = cn;
    }

    auto put_tile = [&](auto atomic_c) {                // a plain store into slab s
        constexpr bool AT = decltype(atomic_c)::value;
        float* out = d.partial + (AT ? 0 : (size_t)s * d.M * d.N);
#pragma unroll
        for (int mi = 0; mi < 2; ++mi)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = m0 + wr * 64 + mi * 32 + (r & 3) + 8 * (r >> 2) + 4 * lk;
                if (row < d.M) {
#pragma unroll
                    for (int ni = 0; ni < 2; ++ni) {
                        const int col = n0 + wc * 64 + ni * 32 + l31;
                        if (col < d.N) wg_put<AT>(out + (size_t)row * d.N + col, acc[mi][ni][r]);
                    }
                }
            }
        if (do_bias && tid < BM && (m0 + tid) < d.M) wg_put<AT>(d.partial_bias + (AT ? 0 : (size_t)s * d.M) + m0 + tid, bias_acc);
    };
    put_tile(std::false_type{});
}

}  // namespace

// Called by sep_pw_wgrad (wgrad.hip), which has checked the descriptor, sized the grid and named the kernel.
void sep_pw_wgrad_staged(const sep_wgrad_desc* d, int grid, hipStream_t stream) {
    hipLaunchKernelGGL(pw_wgrad_kernel, dim3(grid), dim3(256), 0, stream, *d);
}

#ifdef SEP_PROF
extern "C" int sep_debug_blocks(long long* start, long long* end) {
    if (hipMemcpyFromSymbol(start, HIP_SYMBOL(g_blk_start), sizeof(long long) * 8192) != hipSuccess) return -1;
    return hipMemcpyFromSymbol(end, HIP_SYMBOL(g_blk_end), sizeof(long long) * 8192) == hipSuccess ? 0 : -1;
}
extern "C" int sep_debug_prof(long long* out) {      // development builds only (tools/gemm_prof.py)
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(g_prof), sizeof(long long) * 4 * 4 * 16) == hipSuccess ? 0 : -1;
}
#endif

extern "C" int sep_pw_gemm(const sep_gemm_desc* d, sep_stream_t stream) {
    SEP_REQUIRE(d != nullptr, "sep_pw_gemm: null descriptor");
    SEP_REQUIRE(d->B > 0 && d->M > 0 && d->K > 0 && d->T > 0, "sep_pw_gemm: empty problem (B=%d M=%d K=%d T=%d)", d->B, d->M, d->K, d->T);
    SEP_REQUIRE(d->ldt % 128 == 0 && d->ldt >= d->T, "sep_pw_gemm: ldt=%d must be a multiple of 128 and >= T=%d", d->ldt, d->T);
    SEP_REQUIRE(d->K % 16 == 0, "sep_pw_gemm: K=%d must be a multiple of 16", d->K);
    SEP_REQUIRE(d->k_split % 16 == 0 && d->k_split < d->K, "sep_pw_gemm: bad k_split=%d", d->k_split);
    SEP_REQUIRE(d->m_split % BM == 0 && d->m_split < d->M, "sep_pw_gemm: bad m_split=%d (M=%d)", d->m_split, d->M);
    SEP_REQUIRE(!d->trans_a || d->M % 4 == 0, "sep_pw_gemm: transposed A needs M %% 4 == 0 (M=%d)", d->M);
    SEP_REQUIRE(d->A && d->X && d->Y, "sep_pw_gemm: null operand");
    SEP_REQUIRE(!d->k_split || (d->A2 && d->X2), "sep_pw_gemm: k_split without A2/X2");
    SEP_REQUIRE(!d->m_split || d->Y2, "sep_pw_gemm: m_split without Y2");
    SEP_REQUIRE(d->pro_mode >= 0 && d->pro_mode <= SEP_PRO_GLN_BWD, "sep_pw_gemm: bad pro_mode %d", d->pro_mode);
    SEP_REQUIRE(d->arith >= SEP_ARITH_F32 && d->arith <= SEP_ARITH_F16X3, "sep_pw_gemm: bad arith %d", d->arith);
    if (d->pro_mode == SEP_PRO_PRELU || d->pro_mode == SEP_PRO_GLN_PRELU || d->pro_mode == SEP_PRO_GLN_BWD)
        SEP_REQUIRE(d->pro_alpha, "sep_pw_gemm: prologue needs pro_alpha");
    if (d->pro_mode >= SEP_PRO_GLN)
        SEP_REQUIRE(d->pro_stats && d->pro_gamma && (d->pro_mode == SEP_PRO_GLN_BWD || d->pro_beta) && d->count > 0, "sep_pw_gemm: gLN prologue needs stats/gamma/beta/count");
    if (d->pro_mode == SEP_PRO_GLN_BWD)
        SEP_REQUIRE(d->pro_aux && (d->pro_bsum || d->pro_bacc) && d->pro_store && d->pro_dalpha && !d->k_split, "sep_pw_gemm: GLN_BWD prologue needs aux/bsum/store/dalpha");
    if (d->pro_mode == SEP_PRO_GLN_BWD)      // row tile 0 stores da while the other row tiles still read X: in place only with one row tile
        SEP_REQUIRE(d->pro_store != d->X || d->M <= BM, "sep_pw_gemm: pro_store may alias X only when M <= %d (one row tile)", BM);
    if (d->epi_flags & SEP_EPI_STATS_PRELU) SEP_REQUIRE(d->epi_stats && d->epi_alpha, "sep_pw_gemm: STATS_PRELU needs epi_stats/epi_alpha");
    if (d->epi_flags & SEP_EPI_RESIDUAL) SEP_REQUIRE(d->epi_res, "sep_pw_gemm: RESIDUAL needs epi_res");
    if (d->epi_flags & SEP_EPI_PRELU_BWD) SEP_REQUIRE(d->epi_aux && d->epi_alpha && d->epi_dalpha, "sep_pw_gemm: PRELU_BWD needs aux/alpha/dalpha");
    if (d->epi_flags & SEP_EPI_ROWSUMS) SEP_REQUIRE(d->epi_aux && d->epi_rowpart && !d->m_split, "sep_pw_gemm: ROWSUMS needs aux/rowpart");
    if (d->epi_flags & SEP_EPI_ROWSUMS_PRELU) SEP_REQUIRE(d->epi_alpha, "sep_pw_gemm: ROWSUMS_PRELU needs epi_alpha");
    if (d->arith == SEP_ARITH_F16X3 && d->A_pk != nullptr) {
        SEP_REQUIRE(d->a_rscale != nullptr, "sep_pw_gemm: A_pk without a_rscale");
        if (sep_pw_gemm_packed(d, (hipStream_t)stream)) {      // packed weights, cooperative split (gemm_coop.hip)
            SEP_CHECK_LAUNCH("sep_pw_gemm (packed)");
            return 0;
        }
    }
    const int NR = ceil_div(d->M, BM);
    const int NC = d->B * (d->ldt / BN);
    const int grid = xcd_grid(NR, NC);
    // fast path: direct-to-LDS high-occupancy kernel; the register-staged kernel remains for shapes outside its limits
    static const bool force_staged = getenv("SEPK_FORCE_STAGED") != nullptr;
    const bool direct_ok = !force_staged && d->K % DK == 0 && d->k_split % DK == 0 && d->M >= 4 && d->M % 4 == 0 &&
                           (d->pro_mode < SEP_PRO_GLN || d->K <= OMAXK);
    SEP_REQUIRE(direct_ok || (d->K % BK == 0 && d->k_split % BK == 0), "sep_pw_gemm: the register-staged fallback (K=%d) needs K %% 32 == 0", d->K);
    if (direct_ok) {
        // curated combinations exist in both arithmetics (GLN_BWD: fp32 MFMA only -- its time is the prologue, measured equal)
        const bool split3 = d->arith == SEP_ARITH_F16X3 && d->a_amax != nullptr;
        const bool split6 = d->arith == SEP_ARITH_BF16X6 || d->arith == SEP_ARITH_F16X3;
        // 1. the fused products of the Conv-TasNet step (gemm_common.hpp: one row each), epilogue flags compile-time
        const int ef = d->epi_flags, pm = d->pro_mode;
        const bool tr = d->trans_a != 0, sp = d->k_split != 0;
        bool done = false;
#define SEP_LD(T, P, S, E, MI4)                                                                                                                      \
    if (tr == T && sp == S && pm == P && ef == (E)) {                                                                                                \
        done = true;                                                                                                                                 \
        if (split3 && P != SEP_PRO_GLN_BWD) {                                                                                                        \
            sep_set_kernel("direct<" #T "," #P "," #S "," #E ",arith=2>");                                                                           \
            hipLaunchKernelGGL((pw_gemm_direct_kernel<T, P, S, E, (P != SEP_PRO_GLN_BWD ? 2 : 0)>), dim3(grid), dim3(256), 0, (hipStream_t)stream, *d); \
        } else if (split6 && P != SEP_PRO_GLN_BWD) {                                                                                                 \
            sep_set_kernel("direct<" #T "," #P "," #S "," #E ",arith=1>");                                                                           \
            hipLaunchKernelGGL((pw_gemm_direct_kernel<T, P, S, E, (P != SEP_PRO_GLN_BWD ? 1 : 0)>), dim3(grid), dim3(256), 0, (hipStream_t)stream, *d); \
        } else {                                                                                                                                     \
            sep_set_kernel("direct<" #T "," #P "," #S "," #E ",arith=0>");                                                                           \
            hipLaunchKernelGGL((pw_gemm_direct_kernel<T, P, S, E, 0>), dim3(grid), dim3(256), 0, (hipStream_t)stream, *d);                           \
        }                                                                                                                                            \
    }
        if (d->M % BM == 0) {                      // the specialised epilogues have no row predicate
            SEP_FUSED_COMBOS(SEP_LD, SEP_LD)
        }
#undef SEP_LD
        // 2. anything else: same kernels with the flags read at run time, one row per prologue (gemm_common.hpp).  A prologue without a
        // two-source form (TWO = 0; the argument checks above refuse k_split with it) names its one-source instance in both branches.
        if (!done) {
            // (NAME: the arguments as SEP_LRT spells them -- P has passed through SEP_LRT when it arrives here, expanded to its number)
#define SEP_LG(T, P, S, NAME)                                                                                                     \
    do {                                                                                                                          \
        sep_set_kernel("direct_rt<" NAME ">");                                                                                    \
        hipLaunchKernelGGL((pw_gemm_direct_kernel<T, P, S, -1, 0>), dim3(grid), dim3(256), 0, (hipStream_t)stream, *d);            \
    } while (0)
#define SEP_LRT(P, TWO)                                                                \
    if (pm == P) {                                                                     \
        if (TWO && sp) {                                                               \
            if (tr) SEP_LG(true, P, (TWO != 0), "true," #P ",true");                   \
            else SEP_LG(false, P, (TWO != 0), "false," #P ",true");                    \
        } else {                                                                       \
            if (tr) SEP_LG(true, P, false, "true," #P ",false");                       \
            else SEP_LG(false, P, false, "false," #P ",false");                        \
        }                                                                              \
    }
            SEP_GEMM_PROLOGUES(SEP_LRT)
#undef SEP_LRT
#undef SEP_LG
        }
    } else {
        sep_set_kernel("staged");
        hipLaunchKernelGGL(pw_gemm_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, *d);
    }
    SEP_CHECK_LAUNCH("sep_pw_gemm");
    return 0;
}
