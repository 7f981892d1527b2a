// Global layer norm for gfx950 (HBM-bound streaming kernels): the second stage of the fused network's gLN backward reductions (one gLN
// or up to 64 per launch), the same sums taken from the weight gradient, a stand-alone gLN on (batch, channel, frame) rows and gLN on
// token-major rows.  Channel-major tensors are fp32 with padded row stride ldt; frames [T, ldt) of every written tensor are zero.
//
// Reference arithmetic replaced (reference src/): modules/norm.py:11-35 (gLN = GroupNorm(1, C)).
#include "common.hpp"

namespace {

// =====================================================================================
// gLN backward, second stage, in two small kernels.
//  rows:   one WAVE per (b, c) row reduces that row's per-tile partials (nq in {2, 8}) and writes
//          pbeta[b][c] = R1, pgamma[b][c] = r_b (R2 - mu_b R1), nq == 8: pextra[b] = [db[C] | dw[C][3]] and
//          scratch[b][c] = rowpart[..][6] total (PReLU slope partial)
//  sample: one block per sample sums over channels: bsum[b] = {sum_c gamma_c R1, sum_c gamma_c pgamma} / count,
//          palpha[b] = sum_c scratch[b][c]
// =====================================================================================
__global__ __launch_bounds__(256) void gln_bwd_finalize_rows_kernel(const float* __restrict__ rowpart, int ntile, int nq,
                                                                    const double* __restrict__ stats, double count, float eps,
                                                                    float* __restrict__ pbeta, float* __restrict__ pgamma,
                                                                    float* __restrict__ pextra, float* __restrict__ scratch,
                                                                    int B, int C) {
    const int lane = threadIdx.x & 63;
    const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);      // b*C + c
    if (row >= (long)B * C) return;
    const int b = (int)(row / C), c = (int)(row % C);
    float mu, rstd;
    gln_mu_rstd(stats + (size_t)b * SEP_STATS_SLOTS * 2, count, eps, mu, rstd);
    const int rowlen = ntile * nq;
    const float* rp = rowpart + (size_t)row * rowlen;
    float acc = 0.f;
    for (int i = lane; i < rowlen; i += 64) acc += rp[i];            // i % nq == lane % nq (nq divides 64)
    for (int o = nq; o < 64; o <<= 1) acc += __shfl_xor(acc, o, 64);
    // every lane now holds the total of quantity q = lane % nq
    const float R1 = __shfl(acc, 0, 64), R2 = __shfl(acc, 1, 64);
    if (lane == 0) {
        pbeta[row] = R1;
        pgamma[row] = rstd * (R2 - mu * R1);
    }
    if (nq == 8) {
        // per-sample slab of 4C floats: [ db[C] | dw[C][3] ]
        if (lane == 2) pextra[(size_t)b * 4 * C + c] = acc;
        if (lane >= 3 && lane < 6) pextra[(size_t)b * 4 * C + C + (size_t)c * 3 + (lane - 3)] = acc;
        if (lane == 6) scratch[row] = acc;
    }
}

__global__ __launch_bounds__(256) void gln_bwd_finalize_sample_kernel(const float* __restrict__ pbeta, const float* __restrict__ pgamma,
                                                                      const float* __restrict__ gamma, const float* __restrict__ scratch,
                                                                      double count, float* __restrict__ bsum,
                                                                      float* __restrict__ palpha, int C) {
    __shared__ double red[4];
    const int b = blockIdx.x;
    double sg = 0.0, sgx = 0.0, sal = 0.0;
    for (int c = threadIdx.x; c < C; c += 256) {
        const float gc = gamma[c];
        sg += (double)(gc * pbeta[(size_t)b * C + c]);
        sgx += (double)(gc * pgamma[(size_t)b * C + c]);
        if (palpha) sal += (double)scratch[(size_t)b * C + c];
    }
    const double tg = block_sum_256<double>(sg, red);
    const double tgx = block_sum_256<double>(sgx, red);
    const double tal = block_sum_256<double>(sal, red);
    if (threadIdx.x == 0) {
        if (bsum) {
            bsum[2 * b] = (float)(tg / count);
            bsum[2 * b + 1] = (float)(tgx / count);
        }
        if (palpha) palpha[b] = (float)tal;
    }
}

// The same two stages for up to 64 gLNs in ONE launch each (the Conv-TasNet step queues the second stages of all its layers -- leaves of
// the backward pass -- and flushes them together: 2 launches instead of 2 per layer).
constexpr int FMAXSEG = 64;
struct FinalizeArgs {
    sep_finalize_seg seg[FMAXSEG];
    int blk_start[FMAXSEG + 1];
    int nseg;
};
// lanes that share one row of partials: rowlen / 4 (a float4 each) when that is a power of two <= 64 -- 8 for the depthwise kernel's
// 4 tiles x 8 sums, so a wave reduces EIGHT rows -- else the whole wave walks the row by scalars (the stand-alone kernel's form).  One wave
// per 128-byte row made this launch 133 us for 49 segments (100,000 workgroups of a few instructions each).
__host__ __device__ inline int fin_lanes_per_row(int rowlen, int nq) {
    const int l = rowlen / 4;
    const bool pow2 = rowlen % 4 == 0 && l >= 1 && l <= 64 && (l & (l - 1)) == 0;
    return pow2 && (nq == 2 || l >= 2) ? l : 64;
}
__global__ __launch_bounds__(256) void gln_bwd_finalize_rows_batch_kernel(const FinalizeArgs a) {
    int sgi = 0;
    while (sgi + 1 < a.nseg && (int)blockIdx.x >= a.blk_start[sgi + 1]) ++sgi;
    const sep_finalize_seg sg = a.seg[sgi];
    const int lane = threadIdx.x & 63;
    const int rowlen = sg.ntile * sg.nq;
    const int lpr = fin_lanes_per_row(rowlen, sg.nq), rpw = 64 / lpr;
    const bool packed = lpr != 64 || rowlen == 256;
    const long nrows = (long)sg.B * sg.C;
    const long row = ((long)((int)blockIdx.x - a.blk_start[sgi]) * 4 + (threadIdx.x >> 6)) * rpw + lane / lpr;      // b*C + c
    const int p = lane % lpr;
    const bool live = row < nrows;
    const float* rp = sg.rowpart + (size_t)(live ? row : 0) * rowlen;
    float q[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};      // the row's totals of quantity 0 .. nq-1, valid in the row's lane p == 0
    if (packed) {
        float4 v = live ? ld4(rp + 4 * p) : make_float4(0.f, 0.f, 0.f, 0.f);
        if (sg.nq == 8) {                                        // float4 p holds quantities 4 (p & 1) .. + 3
            for (int o = 2; o < lpr; o <<= 1) {
                v.x += __shfl_xor(v.x, o, 64); v.y += __shfl_xor(v.y, o, 64); v.z += __shfl_xor(v.z, o, 64); v.w += __shfl_xor(v.w, o, 64);
            }
            q[0] = v.x; q[1] = v.y; q[2] = v.z; q[3] = v.w;
            q[4] = __shfl_xor(v.x, 1, 64); q[5] = __shfl_xor(v.y, 1, 64); q[6] = __shfl_xor(v.z, 1, 64); q[7] = __shfl_xor(v.w, 1, 64);
        } else {                                                 // nq == 2: elements alternate between the two quantities
            float s0 = v.x + v.z, s1 = v.y + v.w;
            for (int o = 1; o < lpr; o <<= 1) { s0 += __shfl_xor(s0, o, 64); s1 += __shfl_xor(s1, o, 64); }
            q[0] = s0; q[1] = s1;
        }
    } else {
        float acc = 0.f;
        if (live)
            for (int i = lane; i < rowlen; i += 64) acc += rp[i];    // i % nq == lane % nq (nq divides 64)
        for (int o = sg.nq; o < 64; o <<= 1) acc += __shfl_xor(acc, o, 64);
#pragma unroll
        for (int k = 0; k < 8; ++k) q[k] = __shfl(acc, k, 64);
    }
    if (!live || p != 0) return;
    const int b = (int)(row / sg.C), c = (int)(row % sg.C);
    float mu, rstd;
    gln_mu_rstd(sg.stats + (size_t)b * SEP_STATS_SLOTS * 2, sg.count, sg.eps, mu, rstd);
    sg.pbeta[row] = q[0];
    sg.pgamma[row] = rstd * (q[1] - mu * q[0]);
    if (sg.nq == 8) {
        float* scratch = sg.pextra + (size_t)sg.B * sg.C * 4 + sg.B;
        sg.pextra[(size_t)b * 4 * sg.C + c] = q[2];
        sg.pextra[(size_t)b * 4 * sg.C + sg.C + (size_t)c * 3 + 0] = q[3];
        sg.pextra[(size_t)b * 4 * sg.C + sg.C + (size_t)c * 3 + 1] = q[4];
        sg.pextra[(size_t)b * 4 * sg.C + sg.C + (size_t)c * 3 + 2] = q[5];
        scratch[row] = q[6];
    }
}
__global__ __launch_bounds__(256) void gln_bwd_finalize_sample_batch_kernel(const FinalizeArgs a) {
    __shared__ double red[4];
    int sgi = 0;
    while (sgi + 1 < a.nseg && (int)blockIdx.x >= a.blk_start[sgi + 1]) ++sgi;      // (blk_start counts samples here)
    const sep_finalize_seg sg = a.seg[sgi];
    const int b = (int)blockIdx.x - a.blk_start[sgi];
    const bool slopes = sg.nq == 8;
    const float* scratch = slopes ? sg.pextra + (size_t)sg.B * sg.C * 4 + sg.B : nullptr;
    double sg1 = 0.0, sgx = 0.0, sal = 0.0;
    for (int c = threadIdx.x; c < sg.C; c += 256) {
        const float gc = sg.gamma[c];
        sg1 += (double)(gc * sg.pbeta[(size_t)b * sg.C + c]);
        sgx += (double)(gc * sg.pgamma[(size_t)b * sg.C + c]);
        if (slopes) sal += (double)scratch[(size_t)b * sg.C + c];
    }
    const double tg = block_sum_256<double>(sg1, red);
    const double tgx = block_sum_256<double>(sgx, red);
    const double tal = block_sum_256<double>(sal, red);
    if (threadIdx.x == 0) {
        if (sg.bsum) {
            sg.bsum[2 * b] = (float)(tg / sg.count);
            sg.bsum[2 * b + 1] = (float)(tgx / sg.count);
        }
        if (slopes) sg.pextra[(size_t)sg.B * sg.C * 4 + b] = (float)tal;
    }
}

// =====================================================================================
// gLN backward statistics FROM the weight gradient.  For a product y = W v (1x1 convolution) behind v = gLN(u), u = PReLU(z), the
// gradient arriving at v is dv = W^T g, and the two row sums the gLN backward needs are contractions the weight gradient has
// already done:
//     R1[n] = sum_t dv[n][t]        = sum_m W[m][n] * (sum_t g[m][t])            = sum_m W[m][n] * gs[m]
//     R2[n] = sum_t dv[n][t] u[n][t] = sum_m W[m][n] * (sum_t g[m][t] u[n][t])    = sum_m W[m][n] * raw[m][n]
// with raw = the weight gradient taken against u instead of v (sep_pw_wgrad with x_mode = PRELU) and gs the bias gradient, both PER
// SAMPLE (sample-aligned slabs).  So the input-gradient product dv = W^T g needs no row-sum epilogue and does not read z at all (one
// H-tensor less per layer and step), and no second-stage kernel runs for this gLN.  The gain / shift of the normalisation, which
// the raw gradient skipped, is applied here on the small matrices:  dW_b[m][n] = sc_bn raw_b[m][n] + sh_bn gs_b[m].
// grid (ceil(N / 32), B), 1024 threads: lane & 31 = column n, (wave, lane >> 5) = 32 row classes -- a thread's rows are m = cls + 32 i, all of
// whose loads are in flight together (the first version walked 64 rows one by one in a 256-thread workgroup: 87 us per launch for 42 MB,
// profiles/r03c_kernel_stats.md).  The sample's last workgroup publishes the two means the consumer of dv reads (gln_bwd_publish).
// =====================================================================================
constexpr int GW_ROWS = 8;        // rows per thread and pass
__global__ __launch_bounds__(1024) void gln_bwd_from_wgrad_kernel(const float* __restrict__ part, const float* __restrict__ part_bias,
                                                                  const float* __restrict__ W, const double* __restrict__ stats,
                                                                  const float* __restrict__ gamma, const float* __restrict__ beta,
                                                                  double count, float eps, float* __restrict__ dW_b,
                                                                  float* __restrict__ pbeta, float* __restrict__ pgamma,
                                                                  double* __restrict__ bacc, int* __restrict__ arrive, float* __restrict__ bsum,
                                                                  int M, int N, int sps, int accumulate, int products) {
    extern __shared__ __attribute__((aligned(16))) float lds[];      // gs[M] | red[32 classes][32 columns][2]
    float* gs = lds;
    float* red = lds + M;
    const int b = blockIdx.y;
    const int col = threadIdx.x & 31, cls = threadIdx.x >> 5;        // 32 row classes
    const int n = blockIdx.x * 32 + col;
    const bool live = n < N;
    for (int m = threadIdx.x; m < M; m += 1024) {
        float t = 0.f;
        for (int k = 0; k < sps; ++k) t += part_bias[(size_t)(b * sps + k) * M + m];
        gs[m] = t;
    }
    float mu, rstd;
    gln_mu_rstd(stats + (size_t)b * SEP_STATS_SLOTS * 2, count, eps, mu, rstd);
    const float gm = live ? gamma[n] : 0.f;
    const float sc = gm * rstd, sh = live ? beta[n] - mu * sc : 0.f;
    __syncthreads();
    float r1 = 0.f, r2 = 0.f;
    const size_t slab = (size_t)M * N;
    const int nc = live ? n : 0;
    const float* p0 = part + (size_t)b * sps * slab + nc;
    for (int m0 = cls; m0 < M; m0 += 32 * GW_ROWS) {
        float raw[GW_ROWS], w[GW_ROWS];
#pragma unroll
        for (int i = 0; i < GW_ROWS; ++i) {
            const int m = m0 + 32 * i;
            const int mc = m < M ? m : 0;                      // rows past M: a harmless in-bounds load, zero weight
            w[i] = (m < M && live) ? W[(size_t)mc * N + nc] : 0.f;
            raw[i] = p0[(size_t)mc * N];
        }
        for (int k = 1; k < sps; ++k)
#pragma unroll
            for (int i = 0; i < GW_ROWS; ++i) {
                const int m = m0 + 32 * i;
                raw[i] += p0[k * slab + (size_t)(m < M ? m : 0) * N];
            }
#pragma unroll
        for (int i = 0; i < GW_ROWS; ++i) {
            const int m = m0 + 32 * i;
            if (m < M && live) {
                const float g = gs[m];
                r1 = fmaf(w[i], g, r1);
                r2 = fmaf(w[i], raw[i], r2);
                dW_b[((size_t)b * M + m) * N + n] = fmaf(sc, raw[i], sh * g);
            }
        }
    }
    red[(cls * 32 + col) * 2] = r1;
    red[(cls * 32 + col) * 2 + 1] = r2;
    __syncthreads();
    if (threadIdx.x < 64) {                                // lanes 0-31: R1 of the block's columns, lanes 32-63: R2
        const int q = threadIdx.x >> 5;
        float R = 0.f;
#pragma unroll 8
        for (int k = 0; k < 32; ++k) R += red[(k * 32 + col) * 2 + q];
        const float R1 = __shfl(R, col, 64), R2 = __shfl(R, 32 + col, 64);
        if (live && q == 0) {
            const float pg = rstd * (R2 - mu * R1);
            if (accumulate) { pbeta[(size_t)b * N + n] += R1; pgamma[(size_t)b * N + n] += pg; }
            else { pbeta[(size_t)b * N + n] = R1; pgamma[(size_t)b * N + n] = pg; }
        }
        float a = gm * R;                                  // lanes 0-31: gamma R1 ; lanes 32-63: gamma R2
#pragma unroll
        for (int o = 16; o > 0; o >>= 1) a += __shfl_xor(a, o, 64);      // sums inside each 32-lane half
        const float a2 = __shfl(a, 32, 64);
        if (threadIdx.x == 0) {      // gridDim.x workgroups per sample and product, numbered blockIdx.x: slot blockIdx.x & 15
            const int slot = blockIdx.x & (SEP_STATS_SLOTS - 1);
            gln_bwd_publish(bacc + (size_t)b * SEP_STATS_SLOTS * 2, stats + (size_t)b * SEP_STATS_SLOTS * 2, arrive + (size_t)b * SEP_ARRIVE_INTS, bsum + 2 * b,
                            slot, arrivals_in_slot((int)gridDim.x, slot) * products, slots_in_use((int)gridDim.x), (double)a, (double)a2, count, eps);
        }
    }
}

// =====================================================================================
// Stand-alone gLN (for callers outside the fused network)
// =====================================================================================
__global__ __launch_bounds__(256) void gln_stats_kernel(const float* __restrict__ x, double* __restrict__ stats, int C,
                                                        int T, int ldt) {
    __shared__ double red[4];
    const int row = blockIdx.y;
    const int b = row / C;
    // a row is shared by at most 8 workgroups, each thread taking every gridDim.x-th group of 256 float4s: one block reduction and one pair of
    // fp64 atomics per ~8 K frames instead of per 1 K (DPRNN-TasNet's 64,250-frame rows: 8064 workgroups of one float4 per thread took 67 us)
    float s = 0.f, ss = 0.f;
    for (int t4 = (blockIdx.x * 256 + threadIdx.x) * 4; t4 < ldt; t4 += gridDim.x * 1024) {
        const float4 v = ld4(x + (size_t)row * ldt + t4);
        const float v4[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (t4 + e < T) { s += v4[e]; ss += v4[e] * v4[e]; }
    }
    const double ds = block_sum_256<double>((double)s, red);
    const double dss = block_sum_256<double>((double)ss, red);
    if (threadIdx.x == 0) { double* st = stats + ((size_t)b * SEP_STATS_SLOTS + ((blockIdx.x + blockIdx.y) & (SEP_STATS_SLOTS - 1))) * 2; atomicAdd(st, ds); atomicAdd(st + 1, dss); }
}

__global__ __launch_bounds__(256) void gln_apply_kernel(const float* __restrict__ x, const double* __restrict__ stats,
                                                        const float* __restrict__ gamma, const float* __restrict__ beta,
                                                        float* __restrict__ y, int C, int T, int ldt, double count,
                                                        float eps) {
    const int row = blockIdx.y;
    const int b = row / C, c = row % C;
    const int t4 = (blockIdx.x * 256 + threadIdx.x) * 4;
    if (t4 >= ldt) return;
    float mu, rstd;
    gln_mu_rstd(stats + (size_t)b * SEP_STATS_SLOTS * 2, count, eps, mu, rstd);
    const float sc = gamma[c] * rstd, sh = beta[c] - mu * sc;
    const float4 v = ld4(x + (size_t)row * ldt + t4);
    float4 o;
    o.x = (t4 + 0 < T) ? v.x * sc + sh : 0.f;
    o.y = (t4 + 1 < T) ? v.y * sc + sh : 0.f;
    o.z = (t4 + 2 < T) ? v.z * sc + sh : 0.f;
    o.w = (t4 + 3 < T) ? v.w * sc + sh : 0.f;
    st4(y + (size_t)row * ldt + t4, o);
}

// rowpart[b][c][tile][2] = {sum dy, sum dy*x} over a 1024-frame tile (one block per tile)
__global__ __launch_bounds__(256) void gln_bwd_rowsums_kernel(const float* __restrict__ dy, const float* __restrict__ x,
                                                              float* __restrict__ rowpart, int T, int ldt, int ntile) {
    __shared__ float red[4];
    const int row = blockIdx.y;
    const int tile = blockIdx.x;
    const int t4 = tile * 1024 + threadIdx.x * 4;
    float s1 = 0.f, s2 = 0.f;
    if (t4 < ldt) {
        const float4 g = ld4(dy + (size_t)row * ldt + t4), v = ld4(x + (size_t)row * ldt + t4);
        const float g4[4] = {g.x, g.y, g.z, g.w}, v4[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (t4 + e < T) { s1 += g4[e]; s2 += g4[e] * v4[e]; }
    }
    const float r1 = block_sum_256<float>(s1, red);
    const float r2 = block_sum_256<float>(s2, red);
    if (threadIdx.x == 0) {
        float* rp = rowpart + ((size_t)row * ntile + tile) * 2;
        rp[0] = r1; rp[1] = r2;
    }
}

__global__ __launch_bounds__(256) void gln_bwd_apply_kernel(const float* __restrict__ dy, const float* __restrict__ x,
                                                            const double* __restrict__ stats, const float* __restrict__ gamma,
                                                            const float* __restrict__ bsum, float* __restrict__ dx, int C,
                                                            int T, int ldt, double count, float eps) {
    const int row = blockIdx.y;
    const int b = row / C, c = row % C;
    const int t4 = (blockIdx.x * 256 + threadIdx.x) * 4;
    if (t4 >= ldt) return;
    float mu, rstd;
    gln_mu_rstd(stats + (size_t)b * SEP_STATS_SLOTS * 2, count, eps, mu, rstd);
    const float gc = gamma[c], mg = bsum[2 * b], mgx = bsum[2 * b + 1];
    const size_t off = (size_t)row * ldt + t4;
    const float4 g = ld4(dy + off), v = ld4(x + off);
    const float g4[4] = {g.x, g.y, g.z, g.w}, v4[4] = {v.x, v.y, v.z, v.w};
    float o[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const float xh = (v4[e] - mu) * rstd;
        o[e] = (t4 + e < T) ? rstd * (gc * g4[e] - mg - xh * mgx) : 0.f;
    }
    st4(dx + off, make_float4(o[0], o[1], o[2], o[3]));
}

// =====================================================================================
// Global layer norm on TOKEN-MAJOR rows: x (nseq, L, C) with the features contiguous -- the layout the dual-path separators keep between
// their attention / LSTM / Linear layers (DPTNet's and GALRNet's blocks: reference src/models/dptnet.py:505-560, `norm1d(x.permute(1, 2, 0))`).
// Statistics over all L*C values of a sequence (nn.GroupNorm(1, C) on (batch, C, L): mean, biased variance, eps inside the root), gain and
// shift per feature.  One workgroup per sequence, float4 per thread and trip; the second pass over the sequence's <= a few hundred KB
// comes out of L2.  With the features innermost the channel-major sep_gln_* kernels would need two transposing copies per norm
// (DPTNet: 96 of its 244 strided copies per step).  C must divide 1024 (a thread's four lanes keep their features across trips).
//   forward : y = (x - mu) rstd gamma_c + beta_c ; stats[s] = {mu, rstd}
//   backward: dx = rstd (g gamma_c - m1 - xhat m2), m1 = mean(g gamma), m2 = mean(g gamma xhat) ; part[s] = {sum_t g xhat [C] | sum_t g [C]}
// =====================================================================================
__global__ __launch_bounds__(256) void gln_tokens_fwd_kernel(const float* __restrict__ x, const float* __restrict__ gamma, const float* __restrict__ beta,
                                                             float* __restrict__ y, float* __restrict__ stats, int n, int C, float eps) {
    __shared__ double red[4];
    const float* xs = x + (size_t)blockIdx.x * n;
    float* ys = y + (size_t)blockIdx.x * n;
    double s = 0.0, ss = 0.0;
    for (int i = 4 * threadIdx.x; i < n; i += 1024) {
        const float4 v = ld4(xs + i);
        s += (double)((v.x + v.y) + (v.z + v.w));
        ss += (double)(fmaf(v.x, v.x, v.y * v.y) + fmaf(v.z, v.z, v.w * v.w));
    }
    const double ts = block_sum_256<double>(s, red), tss = block_sum_256<double>(ss, red);
    const double m = ts / n;
    double var = tss / n - m * m;
    if (var < 0.0) var = 0.0;
    const float mu = (float)m, rstd = (float)(1.0 / sqrt(var + (double)eps));
    if (threadIdx.x == 0) { stats[2 * blockIdx.x] = mu; stats[2 * blockIdx.x + 1] = rstd; }
    const int c0 = (4 * threadIdx.x) % C;
    const float4 g4 = ld4(gamma + c0), b4 = ld4(beta + c0);
    for (int i = 4 * threadIdx.x; i < n; i += 1024) {
        const float4 v = ld4(xs + i);
        st4(ys + i, make_float4(fmaf((v.x - mu) * rstd, g4.x, b4.x), fmaf((v.y - mu) * rstd, g4.y, b4.y),
                                fmaf((v.z - mu) * rstd, g4.z, b4.z), fmaf((v.w - mu) * rstd, g4.w, b4.w)));
    }
}

__global__ __launch_bounds__(256) void gln_tokens_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ x, const float* __restrict__ gamma,
                                                             const float* __restrict__ stats, float* __restrict__ dx, float* __restrict__ part,
                                                             int n, int C) {
    __shared__ double red[4];
    __shared__ float pc[256][8];
    const float* xs = x + (size_t)blockIdx.x * n;
    const float* gs = dy + (size_t)blockIdx.x * n;
    float* ds = dx + (size_t)blockIdx.x * n;
    const float mu = stats[2 * blockIdx.x], rstd = stats[2 * blockIdx.x + 1];
    const int c0 = (4 * threadIdx.x) % C;
    const float4 g4 = ld4(gamma + c0);
    const float ga[4] = {g4.x, g4.y, g4.z, g4.w};
    double s1 = 0.0, s2 = 0.0;
    float pg[4] = {0.f, 0.f, 0.f, 0.f}, pb[4] = {0.f, 0.f, 0.f, 0.f};
    for (int i = 4 * threadIdx.x; i < n; i += 1024) {
        const float4 v = ld4(xs + i), g = ld4(gs + i);
        const float xv[4] = {v.x, v.y, v.z, v.w}, gv[4] = {g.x, g.y, g.z, g.w};
        float a1 = 0.f, a2 = 0.f;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float xh = (xv[e] - mu) * rstd, gg = gv[e] * ga[e];
            a1 += gg; a2 = fmaf(gg, xh, a2);
            pg[e] = fmaf(gv[e], xh, pg[e]); pb[e] += gv[e];
        }
        s1 += (double)a1; s2 += (double)a2;
    }
    const double t1 = block_sum_256<double>(s1, red), t2 = block_sum_256<double>(s2, red);
    const float m1 = (float)(t1 / n), m2 = (float)(t2 / n);
    for (int i = 4 * threadIdx.x; i < n; i += 1024) {
        const float4 v = ld4(xs + i), g = ld4(gs + i);
        const float xv[4] = {v.x, v.y, v.z, v.w}, gv[4] = {g.x, g.y, g.z, g.w};
        float o[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float xh = (xv[e] - mu) * rstd;
            o[e] = rstd * (gv[e] * ga[e] - m1 - xh * m2);
        }
        st4(ds + i, make_float4(o[0], o[1], o[2], o[3]));
    }
    // per-feature partials: thread t holds features (4 t) % C .. + 3; the threads of a feature are C / 4 apart
#pragma unroll
    for (int e = 0; e < 4; ++e) { pc[threadIdx.x][e] = pg[e]; pc[threadIdx.x][4 + e] = pb[e]; }
    __syncthreads();
    float* ps = part + (size_t)blockIdx.x * 2 * C;
    for (int c = threadIdx.x; c < C; c += 256) {
        float tg = 0.f, tb = 0.f;
        for (int t = c / 4; t < 256; t += C / 4) { tg += pc[t][c & 3]; tb += pc[t][4 + (c & 3)]; }
        ps[c] = tg; ps[C + c] = tb;
    }
}

// ---- few, long sequences (GALRNet: one sequence per SAMPLE, ~1 MB each): one workgroup per sequence leaves the chip to nseq compute
// units (96 / 128 us forward / backward with 4 samples, profiles/r05zj_galrnet_kernel_stats.md).  Split form: grid (nsplit, nseq), slices of
// whole 1024-float trips (a thread keeps its four features), the slices' partial sums in a workspace, every workgroup adding them up in
// slice order for itself; two launches each way.
//   wsd[(s * nsplit + j) * 2 + {0, 1}]            forward: sum, sum of squares of slice j | backward: sum g gamma, sum g gamma xhat
//   wsf[((s * nsplit + j) * 2 + {0, 1}) * C + c]  backward: slice j's sum_t g xhat, sum_t g of feature c
__device__ __forceinline__ void gln_tokens_slice(const int n, const int nsplit, int& lo, int& hi) {
    const int trips = (n + 1023) / 1024, per = (trips + nsplit - 1) / nsplit;
    lo = blockIdx.x * per * 1024;
    hi = lo + per * 1024;
    if (hi > n) hi = n;
}
__global__ __launch_bounds__(256) void gln_tokens_part_fwd_kernel(const float* __restrict__ x, double* __restrict__ wsd, int n, int nsplit) {
    __shared__ double red[4];
    const float* xs = x + (size_t)blockIdx.y * n;
    int lo, hi;
    gln_tokens_slice(n, nsplit, lo, hi);
    double s = 0.0, ss = 0.0;
    for (int i = lo + 4 * threadIdx.x; i < hi; i += 1024) {
        const float4 v = ld4(xs + i);
        s += (double)((v.x + v.y) + (v.z + v.w));
        ss += (double)(fmaf(v.x, v.x, v.y * v.y) + fmaf(v.z, v.z, v.w * v.w));
    }
    const double ts = block_sum_256<double>(s, red), tss = block_sum_256<double>(ss, red);
    if (threadIdx.x == 0) {
        wsd[((size_t)blockIdx.y * nsplit + blockIdx.x) * 2] = ts;
        wsd[((size_t)blockIdx.y * nsplit + blockIdx.x) * 2 + 1] = tss;
    }
}
__global__ __launch_bounds__(256) void gln_tokens_apply_fwd_kernel(const float* __restrict__ x, const float* __restrict__ gamma, const float* __restrict__ beta,
                                                                   const double* __restrict__ wsd, float* __restrict__ y, float* __restrict__ stats, int n,
                                                                   int nsplit, int C, float eps) {
    const float* xs = x + (size_t)blockIdx.y * n;
    float* ys = y + (size_t)blockIdx.y * n;
    double ts = 0.0, tss = 0.0;
    for (int j = 0; j < nsplit; ++j) {
        ts += wsd[((size_t)blockIdx.y * nsplit + j) * 2];
        tss += wsd[((size_t)blockIdx.y * nsplit + j) * 2 + 1];
    }
    const double m = ts / n;
    double var = tss / n - m * m;
    if (var < 0.0) var = 0.0;
    const float mu = (float)m, rstd = (float)(1.0 / sqrt(var + (double)eps));
    if (blockIdx.x == 0 && threadIdx.x == 0) { stats[2 * blockIdx.y] = mu; stats[2 * blockIdx.y + 1] = rstd; }
    int lo, hi;
    gln_tokens_slice(n, nsplit, lo, hi);
    const int c0 = (4 * threadIdx.x) % C;
    const float4 g4 = ld4(gamma + c0), b4 = ld4(beta + c0);
    for (int i = lo + 4 * threadIdx.x; i < hi; i += 1024) {
        const float4 v = ld4(xs + i);
        st4(ys + i, make_float4(fmaf((v.x - mu) * rstd, g4.x, b4.x), fmaf((v.y - mu) * rstd, g4.y, b4.y),
                                fmaf((v.z - mu) * rstd, g4.z, b4.z), fmaf((v.w - mu) * rstd, g4.w, b4.w)));
    }
}
__global__ __launch_bounds__(256) void gln_tokens_part_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ x, const float* __restrict__ gamma,
                                                                  const float* __restrict__ stats, double* __restrict__ wsd, float* __restrict__ wsf, int n,
                                                                  int nsplit, int C) {
    __shared__ double red[4];
    __shared__ float pc[256][8];
    const float* xs = x + (size_t)blockIdx.y * n;
    const float* gs = dy + (size_t)blockIdx.y * n;
    const float mu = stats[2 * blockIdx.y], rstd = stats[2 * blockIdx.y + 1];
    const int c0 = (4 * threadIdx.x) % C;
    const float4 g4 = ld4(gamma + c0);
    const float ga[4] = {g4.x, g4.y, g4.z, g4.w};
    int lo, hi;
    gln_tokens_slice(n, nsplit, lo, hi);
    double s1 = 0.0, s2 = 0.0;
    float pg[4] = {0.f, 0.f, 0.f, 0.f}, pb[4] = {0.f, 0.f, 0.f, 0.f};
    for (int i = lo + 4 * threadIdx.x; i < hi; i += 1024) {
        const float4 v = ld4(xs + i), g = ld4(gs + i);
        const float xv[4] = {v.x, v.y, v.z, v.w}, gv[4] = {g.x, g.y, g.z, g.w};
        float a1 = 0.f, a2 = 0.f;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float xh = (xv[e] - mu) * rstd, gg = gv[e] * ga[e];
            a1 += gg; a2 = fmaf(gg, xh, a2);
            pg[e] = fmaf(gv[e], xh, pg[e]); pb[e] += gv[e];
        }
        s1 += (double)a1; s2 += (double)a2;
    }
    const double t1 = block_sum_256<double>(s1, red), t2 = block_sum_256<double>(s2, red);
    const size_t rec = (size_t)blockIdx.y * nsplit + blockIdx.x;
    if (threadIdx.x == 0) { wsd[rec * 2] = t1; wsd[rec * 2 + 1] = t2; }
#pragma unroll
    for (int e = 0; e < 4; ++e) { pc[threadIdx.x][e] = pg[e]; pc[threadIdx.x][4 + e] = pb[e]; }
    __syncthreads();
    float* ps = wsf + rec * 2 * C;
    for (int c = threadIdx.x; c < C; c += 256) {
        float tg = 0.f, tb = 0.f;
        for (int t = c / 4; t < 256; t += C / 4) { tg += pc[t][c & 3]; tb += pc[t][4 + (c & 3)]; }
        ps[c] = tg; ps[C + c] = tb;
    }
}
__global__ __launch_bounds__(256) void gln_tokens_apply_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ x, const float* __restrict__ gamma,
                                                                   const float* __restrict__ stats, const double* __restrict__ wsd, const float* __restrict__ wsf,
                                                                   float* __restrict__ dx, float* __restrict__ part, int n, int nsplit, int C) {
    const float* xs = x + (size_t)blockIdx.y * n;
    const float* gs = dy + (size_t)blockIdx.y * n;
    float* ds = dx + (size_t)blockIdx.y * n;
    const float mu = stats[2 * blockIdx.y], rstd = stats[2 * blockIdx.y + 1];
    double t1 = 0.0, t2 = 0.0;
    for (int j = 0; j < nsplit; ++j) {
        t1 += wsd[((size_t)blockIdx.y * nsplit + j) * 2];
        t2 += wsd[((size_t)blockIdx.y * nsplit + j) * 2 + 1];
    }
    const float m1 = (float)(t1 / n), m2 = (float)(t2 / n);
    if (blockIdx.x == 0) {                                                       // the per-feature sums of the sequence, slices in order
        float* ps = part + (size_t)blockIdx.y * 2 * C;
        for (int c = threadIdx.x; c < 2 * C; c += 256) {
            float t = 0.f;
            for (int j = 0; j < nsplit; ++j) t += wsf[((size_t)blockIdx.y * nsplit + j) * 2 * C + c];
            ps[c] = t;
        }
    }
    int lo, hi;
    gln_tokens_slice(n, nsplit, lo, hi);
    const int c0 = (4 * threadIdx.x) % C;
    const float4 g4 = ld4(gamma + c0);
    const float ga[4] = {g4.x, g4.y, g4.z, g4.w};
    for (int i = lo + 4 * threadIdx.x; i < hi; i += 1024) {
        const float4 v = ld4(xs + i), g = ld4(gs + i);
        const float xv[4] = {v.x, v.y, v.z, v.w}, gv[4] = {g.x, g.y, g.z, g.w};
        float o[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float xh = (xv[e] - mu) * rstd;
            o[e] = rstd * (gv[e] * ga[e] - m1 - xh * m2);
        }
        st4(ds + i, make_float4(o[0], o[1], o[2], o[3]));
    }
}
// slices per sequence: none while the sequences alone fill the chip; otherwise ~512 workgroups, at least 16 trips each
static int gln_tokens_nsplit(int nseq, long n) {
    if (nseq >= 128) return 1;
    const long trips = (n + 1023) / 1024;
    long ns = (512 + nseq - 1) / nseq;
    if (ns > trips / 16) ns = trips / 16;
    if (ns > 64) ns = 64;
    return ns < 2 ? 1 : (int)ns;
}

}  // namespace

// ---------------------------------------------------------------------------------------
extern "C" int sep_gln_bwd_finalize(const float* rowpart, int ntile, int nq, const double* stats, const float* gamma,
                                    double count, float eps, float* bsum, float* pbeta, float* pgamma, float* pextra,
                                    int B, int C, sep_stream_t stream) {
    SEP_REQUIRE(rowpart && stats && gamma && pbeta && pgamma, "sep_gln_bwd_finalize: null pointer");
    SEP_REQUIRE(nq == 2 || nq == 8, "sep_gln_bwd_finalize: nq must be 2 or 8 (got %d)", nq);
    SEP_REQUIRE(nq == 2 || pextra, "sep_gln_bwd_finalize: nq == 8 needs pextra");
    // pextra layout for nq == 8: B slabs of 4C floats [db[C] | dw[C][3]], then palpha[B], then B*C floats of scratch
    float* palpha = (nq == 8) ? pextra + (size_t)B * C * 4 : nullptr;
    float* scratch = (nq == 8) ? palpha + B : nullptr;
    const long rows = (long)B * C;
    hipLaunchKernelGGL(gln_bwd_finalize_rows_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, (hipStream_t)stream, rowpart, ntile, nq, stats, count, eps, pbeta, pgamma, pextra, scratch, B, C);
    if (bsum || palpha)      // the per-sample stage: the means (stand-alone gLN backward) and / or the PReLU slope partials
        hipLaunchKernelGGL(gln_bwd_finalize_sample_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, pbeta, pgamma, gamma, scratch, count, bsum, palpha, C);
    SEP_CHECK_LAUNCH("sep_gln_bwd_finalize");
    return 0;
}

extern "C" int sep_gln_bwd_finalize_batch(const sep_finalize_seg* segs, int nseg, sep_stream_t stream) {
    SEP_REQUIRE(segs && nseg >= 1 && nseg <= FMAXSEG, "sep_gln_bwd_finalize_batch: 1..64 segments per launch (got %d)", nseg);
    FinalizeArgs rows, samples;
    int rb = 0, sb = 0;
    bool any_sample = false;
    for (int i = 0; i < nseg; ++i) {
        const sep_finalize_seg& g = segs[i];
        SEP_REQUIRE(g.rowpart && g.stats && g.gamma && g.pbeta && g.pgamma && (g.nq == 2 || (g.nq == 8 && g.pextra)) && g.B > 0 && g.C > 0 && g.ntile > 0,
                    "sep_gln_bwd_finalize_batch: bad segment %d", i);
        rows.seg[i] = g; samples.seg[i] = g;
        rows.blk_start[i] = rb; samples.blk_start[i] = sb;
        const int rows_per_block = 4 * (64 / fin_lanes_per_row(g.ntile * g.nq, g.nq));
        rb += (int)(((long)g.B * g.C + rows_per_block - 1) / rows_per_block);
        sb += (g.bsum || g.nq == 8) ? g.B : 0;           // segments that need no per-sample stage take no blocks of it
        any_sample |= (g.bsum || g.nq == 8);
    }
    rows.blk_start[nseg] = rb; samples.blk_start[nseg] = sb;
    rows.nseg = samples.nseg = nseg;
    hipLaunchKernelGGL(gln_bwd_finalize_rows_batch_kernel, dim3(rb), dim3(256), 0, (hipStream_t)stream, rows);
    if (any_sample) hipLaunchKernelGGL(gln_bwd_finalize_sample_batch_kernel, dim3(sb), dim3(256), 0, (hipStream_t)stream, samples);
    SEP_CHECK_LAUNCH("sep_gln_bwd_finalize_batch");
    return 0;
}

extern "C" int sep_gln_bwd_from_wgrad(const float* part, const float* part_bias, const float* W, const double* stats, const float* gamma,
                                      const float* beta, double count, float eps, float* dW_b, float* pbeta, float* pgamma, double* bacc,
                                      int* arrive, float* bsum, int B, int M, int N, int slabs_per_sample, int accumulate, int products,
                                      sep_stream_t stream) {
    SEP_REQUIRE(part && part_bias && W && stats && gamma && beta && dW_b && pbeta && pgamma && bacc && arrive && bsum, "sep_gln_bwd_from_wgrad: null pointer");
    SEP_REQUIRE(B > 0 && B <= 65535 && M > 0 && M <= 8192 && N > 0 && slabs_per_sample > 0 && products >= 1, "sep_gln_bwd_from_wgrad: bad sizes");
    const size_t smem = ((size_t)M + 32 * 32 * 2) * sizeof(float);
    hipLaunchKernelGGL(gln_bwd_from_wgrad_kernel, dim3(ceil_div(N, 32), B), dim3(1024), smem, (hipStream_t)stream, part, part_bias, W, stats, gamma,
                       beta, count, eps, dW_b, pbeta, pgamma, bacc, arrive, bsum, M, N, slabs_per_sample, accumulate, products);
    SEP_CHECK_LAUNCH("sep_gln_bwd_from_wgrad");
    return 0;
}

extern "C" int sep_gln_stats(const float* x, double* stats, int B, int C, int T, int ldt, sep_stream_t stream) {
    SEP_REQUIRE(x && stats && ldt % 4 == 0 && (long)B * C <= 65535, "sep_gln_stats: bad arguments");
    const int tiles = ceil_div(ldt, 1024);
    dim3 grid(tiles < 8 ? tiles : 8, B * C);
    hipLaunchKernelGGL(gln_stats_kernel, grid, dim3(256), 0, (hipStream_t)stream, x, stats, C, T, ldt);
    SEP_CHECK_LAUNCH("sep_gln_stats");
    return 0;
}

extern "C" int sep_gln_apply(const float* x, const double* stats, const float* gamma, const float* beta, float* y, int B,
                             int C, int T, int ldt, double count, float eps, sep_stream_t stream) {
    SEP_REQUIRE(x && stats && gamma && beta && y && ldt % 4 == 0 && (long)B * C <= 65535, "sep_gln_apply: bad arguments");
    dim3 grid(ceil_div(ldt, 1024), B * C);
    hipLaunchKernelGGL(gln_apply_kernel, grid, dim3(256), 0, (hipStream_t)stream, x, stats, gamma, beta, y, C, T, ldt, count, eps);
    SEP_CHECK_LAUNCH("sep_gln_apply");
    return 0;
}

extern "C" int sep_gln_bwd_rowsums(const float* dy, const float* x, float* rowpart, int B, int C, int T, int ldt,
                                   sep_stream_t stream) {
    SEP_REQUIRE(dy && x && rowpart && ldt % 4 == 0 && (long)B * C <= 65535, "sep_gln_bwd_rowsums: bad arguments");
    const int ntile = ceil_div(ldt, 1024);
    dim3 grid(ntile, B * C);
    hipLaunchKernelGGL(gln_bwd_rowsums_kernel, grid, dim3(256), 0, (hipStream_t)stream, dy, x, rowpart, T, ldt, ntile);
    SEP_CHECK_LAUNCH("sep_gln_bwd_rowsums");
    return 0;
}

extern "C" int sep_gln_bwd_apply(const float* dy, const float* x, const double* stats, const float* gamma, const float* bsum,
                                 float* dx, int B, int C, int T, int ldt, double count, float eps, sep_stream_t stream) {
    SEP_REQUIRE(dy && x && stats && gamma && bsum && dx && ldt % 4 == 0 && (long)B * C <= 65535, "sep_gln_bwd_apply: bad arguments");
    dim3 grid(ceil_div(ldt, 1024), B * C);
    hipLaunchKernelGGL(gln_bwd_apply_kernel, grid, dim3(256), 0, (hipStream_t)stream, dy, x, stats, gamma, bsum, dx, C, T, ldt, count, eps);
    SEP_CHECK_LAUNCH("sep_gln_bwd_apply");
    return 0;
}

extern "C" size_t sep_gln_tokens_ws_bytes(int nseq, int L, int C) {
    if (nseq <= 0 || L <= 0 || C <= 0) return 0;
    const int ns = gln_tokens_nsplit(nseq, (long)L * C);
    return ns == 1 ? 0 : (size_t)nseq * ns * 2 * (sizeof(double) + (size_t)C * sizeof(float));
}

extern "C" int sep_gln_tokens_fwd(const float* x, const float* gamma, const float* beta, float* y, float* stats, void* ws, int nseq, int L, int C,
                                  float eps, sep_stream_t stream) {
    SEP_REQUIRE(x && gamma && beta && y && stats && nseq > 0 && L > 0 && C >= 4 && 1024 % C == 0, "sep_gln_tokens_fwd: bad arguments (C must divide 1024, C >= 4)");
    SEP_REQUIRE((long)L * C <= 0x7fffffffL && nseq <= 65535, "sep_gln_tokens_fwd: sequence too long / too many sequences");
    const int ns = gln_tokens_nsplit(nseq, (long)L * C);
    if (ns > 1) {
        SEP_REQUIRE(ws != nullptr, "sep_gln_tokens_fwd: this shape needs the workspace of sep_gln_tokens_ws_bytes");
        sep_set_kernel("gln_tokens_fwd/sliced");
        hipLaunchKernelGGL(gln_tokens_part_fwd_kernel, dim3(ns, nseq), dim3(256), 0, (hipStream_t)stream, x, (double*)ws, L * C, ns);
        hipLaunchKernelGGL(gln_tokens_apply_fwd_kernel, dim3(ns, nseq), dim3(256), 0, (hipStream_t)stream, x, gamma, beta, (const double*)ws, y, stats, L * C, ns, C, eps);
    } else {
        sep_set_kernel("gln_tokens_fwd");
        hipLaunchKernelGGL(gln_tokens_fwd_kernel, dim3((unsigned)nseq), dim3(256), 0, (hipStream_t)stream, x, gamma, beta, y, stats, L * C, C, eps);
    }
    SEP_CHECK_LAUNCH("sep_gln_tokens_fwd");
    return 0;
}

extern "C" int sep_gln_tokens_bwd(const float* dy, const float* x, const float* gamma, const float* stats, float* dx, float* part, void* ws, int nseq,
                                  int L, int C, sep_stream_t stream) {
    SEP_REQUIRE(dy && x && gamma && stats && dx && part && nseq > 0 && L > 0 && C >= 4 && 1024 % C == 0, "sep_gln_tokens_bwd: bad arguments (C must divide 1024, C >= 4)");
    SEP_REQUIRE((long)L * C <= 0x7fffffffL && nseq <= 65535, "sep_gln_tokens_bwd: sequence too long / too many sequences");
    const int ns = gln_tokens_nsplit(nseq, (long)L * C);
    if (ns > 1) {
        SEP_REQUIRE(ws != nullptr, "sep_gln_tokens_bwd: this shape needs the workspace of sep_gln_tokens_ws_bytes");
        double* wsd = (double*)ws;
        float* wsf = (float*)(wsd + (size_t)nseq * ns * 2);
        sep_set_kernel("gln_tokens_bwd/sliced");
        hipLaunchKernelGGL(gln_tokens_part_bwd_kernel, dim3(ns, nseq), dim3(256), 0, (hipStream_t)stream, dy, x, gamma, stats, wsd, wsf, L * C, ns, C);
        hipLaunchKernelGGL(gln_tokens_apply_bwd_kernel, dim3(ns, nseq), dim3(256), 0, (hipStream_t)stream, dy, x, gamma, stats, (const double*)wsd, (const float*)wsf, dx, part, L * C, ns, C);
    } else {
        sep_set_kernel("gln_tokens_bwd");
        hipLaunchKernelGGL(gln_tokens_bwd_kernel, dim3((unsigned)nseq), dim3(256), 0, (hipStream_t)stream, dy, x, gamma, stats, dx, part, L * C, C);
    }
    SEP_CHECK_LAUNCH("sep_gln_tokens_bwd");
    return 0;
}
