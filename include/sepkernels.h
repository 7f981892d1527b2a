/*
 * sepkernels.h -- C ABI of libsepkernels.so: the MI355X (gfx950) kernels behind the
 * Conv-TasNet separation path of tky823/DNN-based_source_separation.
 *
 * The reference is pure PyTorch and has NO FFI for this path; each entry
 * point below therefore names the reference *Python* interface whose arithmetic it replaces
 * (file:line under /root/reference/src).  INTEGRATION.md shows the ctypes binding a
 * maintainer of the reference adds to route those interfaces here.
 *
 * Conventions
 *   - plain pointers and sizes only; no torch types; every pointer is a DEVICE pointer
 *     unless the name ends in _host.
 *   - activations are fp32, layout (batch, channel, frame) as in the reference, frame
 *     contiguous, with a padded row stride `ldt` (floats, multiple of 128).  Frames
 *     [T, ldt) of every tensor a kernel WRITES are set to 0.
 *   - gLN statistics are carried as double[B][SEP_STATS_SLOTS][2]: SEP_STATS_SLOTS independent
 *     {sum, sum of squares} accumulators over the valid (C, T) region of a sample (producer blocks
 *     spread their fp64 atomics over the slots; consumers add the slots up).  The caller zeroes them.
 *   - the caller owns every buffer (inputs, outputs, saved activations, workspaces).
 *     The library keeps no global mutable state, is re-entrant, never synchronises the
 *     device and launches only on the stream it is given (the caller selects the device).
 *   - return 0 on success, <0 on error; sep_last_error() gives the thread-local message.
 */
#ifndef SEPKERNELS_H
#define SEPKERNELS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* sep_stream_t; /* hipStream_t */

#define SEP_ABI_VERSION 23
#define SEP_STATS_SLOTS 16
#define SEP_ARRIVE_INTS 17 /* arrival counters per sample: one per slot + one for the slots (csrc/common.hpp, gln_bwd_publish) */

int sep_version(void);
const char* sep_last_error(void);
/* Which kernel instance the calling thread's last sep_pw_gemm / sep_pw_wgrad / sep_pw_wgrad_batch launch, or its last launch through one
 * of the streaming dispatchers listed below, went to: a string literal naming the family and the template arguments as the dispatcher
 * spells them, "" before the first such launch.  The GEMM families:
 *   pc<WR,WC,prologue,two-source,epilogue>         producer / consumer kernel, packed weights (csrc/gemm_pc.hip)
 *   coop<MI,prologue,two-source,epilogue,ns=N>     cooperative kernel, packed weights (csrc/gemm_coop.hip)
 *   direct<trans_a,prologue,two-source,epilogue,arith=A>   per-wave kernel, flags compile-time (csrc/gemm.hip)
 *   direct_rt<trans_a,prologue,two-source>         the same kernel with the epilogue flags read at run time
 *   staged                                         register-staged fallback
 *   wgrad_pc16<..> / wgrad_pc16_pre<..> / wgrad_pc16_batch<..> / wgrad_pc<..> / wgrad_split<..> / wgrad_direct<..> / wgrad
 * e.g. "pc<4,1,SEP_PRO_GLN_PRELU,false,SEP_EPI_RESIDUAL>".  The streaming dispatchers (csrc/filterbank.hip, tcn.hip, gln.hip, depthwise.hip, cln.hip, causal.hip) name the kernel
 * function and its template arguments as spelled at the launch; a run-time value that selects behaviour without a template argument
 * follows a "/":
 *   sep_encoder_fwd                   encoder_l16s8 | encoder<16> | encoder<0>
 *   sep_dwconv_fwd                    dwconv_fwd_direct<DM,ROWS> | dwconv_fwd_tiles
 *   sep_dwconv_bwd                    dwconv_bwd_row<AL,NIT,recompute> | dwconv_bwd_tiles
 *   sep_decoder_fwd                   decoder_fwd16<2|4> | decoder_fwd<16|0>
 *   sep_decoder_bwd                   decoder_bwd<16,2|16,4|0,0>/nz1|nz8        (nz: slices of the basis rows, the grid's z)
 *   sep_depthwise_fwd / _bwd_input    depthwise3_row<0|1>/aligned|lds | depthwise_fwd | depthwise_bwd_input
 *   sep_depthwise_bwd_weight          depthwise3_wgrad_row | depthwise_bwd_weight
 *   sep_split_rows                    split_rows<4|8>
 *   sep_gln_tokens_fwd / _bwd         gln_tokens_fwd[/sliced] | gln_tokens_bwd[/sliced]
 *   sep_cln_fwd / _stats / _bwd       cln_chain_fwd<RR,true|false> | cln_chain_bwd<RR,8> | cln_three_fwd | cln_three_stats | cln_three_bwd
 *   sep_depthwise_cln_fwd / _bwd_weight   cd_depthwise_fwd<KW,staged> | cd_depthwise_wgrad<KW,staged>
 * Every other entry point leaves the name as it was.  Thread-local like sep_last_error; one pointer store per launch, no device
 * work; takes no stream, so it is not a sequence op.  For tests and tools that must know which instance a shape reaches
 * (tests/gemm_matrix.py, tests/stream_matrix.py); additive to ABI 23. */
const char* sep_last_kernel(void);

/* ---- prologue modes applied to the X operand while it is staged into LDS ---------- */
#define SEP_PRO_NONE 0
#define SEP_PRO_PRELU 1     /* x -> PReLU(x; alpha)                         conv_tasnet.py:373 */
#define SEP_PRO_GLN 2       /* x -> gLN(x)                                  modules/norm.py:27 */
#define SEP_PRO_GLN_PRELU 3 /* x -> gLN(PReLU(x; alpha))                    tdcn.py:113-116,182-186 */
#define SEP_PRO_GLN_BWD 4   /* X = d(gLN out); uses pro_aux = pre-activation a:
                               da = rstd*(gamma*X - mg - xhat*mgx) * PReLU'(a); da is also stored to pro_store
                               and sum(du * a * [a<=0]) is accumulated into pro_dalpha.  pro_store may be X itself (in place)
                               only when M <= 128: with several 128-row tiles the others still read the untouched X */

/* ---- epilogue flags ----------------------------------------------------------------- */
#define SEP_EPI_STATS_PRELU 1 /* accumulate sum/sumsq of PReLU(y; epi_alpha) into epi_stats (y itself is stored) */
#define SEP_EPI_RESIDUAL 2    /* y += epi_res                                tdcn.py:144-145 */
#define SEP_EPI_SIGMOID 4     /* y = 1/(1+exp(-y))                           conv_tasnet.py:375 */
#define SEP_EPI_PRELU_BWD 8   /* y = y * PReLU'(epi_aux); epi_dalpha += sum(y_in * epi_aux * [epi_aux<=0]) */
#define SEP_EPI_ROWSUMS 16    /* epi_rowpart[b][m][t/64][0..1] = sum_t y, sum_t y*u, u = epi_aux (or PReLU(epi_aux)) */
#define SEP_EPI_ROWSUMS_PRELU 32

/* ---- arithmetic of the contraction (fp32 operands and fp32 accumulation in both) ------------------------------
 * F32:    v_mfma_f32_32x32x2_f32 on the operands as they are.
 * BF16X6: every operand value is split EXACTLY into three truncated-bf16 parts (8+8+8 significand bits) and
 *         x*y = hi*hi + hi*mid + mid*hi + mid*mid + hi*lo + lo*hi on v_mfma_f32_32x32x16_bf16 (the three dropped part
 *         products are <= 2^-24 |xy| each); results agree with fp64 as closely as the F32 path's do (tests), at
 *         6 x 32 instead of 8 x 64 matrix-pipe cycles per 16-deep chunk.  Inputs are assumed finite.
 * F16X3:  sep_pw_gemm only (sep_pw_wgrad treats it as BF16X6).  Two-part fp16 split x*2^s = hi + lo (11 + 11 bits),
 *         x*y = hi*hi + hi*lo + lo*hi on v_mfma_f32_32x32x16_f16 (3 x 32 cycles), operands brought into fp16's exponent
 *         range by exact power-of-two scales: one for A from the caller's bound a_amax >= max|A| (device scalar), one per
 *         column of X chosen and adjusted inside the kernel.  The error is relative to |A||X| per output (like fp32
 *         accumulation's), not elementwise: values ~2^-25 below their column's maximum lose low bits.  Without a_amax
 *         the call runs as BF16X6.
 *         PACKED WEIGHTS (A_pk != NULL, the form the Conv-TasNet step uses): A has been split ONCE per pass by
 *         sep_pack_weights into {hi, lo} fp16 pairs with one power-of-two scale PER ROW of A (a_rscale[m] undoes it in the
 *         epilogue); the kernel then DMAs MFMA-ready A operands, and the X tile is put through the prologue and split once
 *         per workgroup (cooperatively, shared through LDS) instead of once per wave.  Needs M % 128 == 0. */
#define SEP_ARITH_F32 0
#define SEP_ARITH_BF16X6 1
#define SEP_ARITH_F16X3 2

/* Pointwise (1x1) convolution as a GEMM on MFMA (fp32 in / fp32 accumulate):
 *     Y[b][m][t] = epilogue( sum_k A[m][k] * prologue(X[b][k][t]) + bias[m] )
 * Replaces nn.Conv1d(kernel_size=1) at tdcn.py:86,173,175 and conv_tasnet.py:335,341 in the
 * forward direction, and the same layers' input-gradient (A transposed) in backward.
 * M and K must be multiples of 16 (K) / any (M); ldt multiple of 128. */
typedef struct sep_gemm_desc {
    int32_t B, M, K, T, ldt;
    int32_t trans_a;    /* 0: A is [M][K] row-major ; 1: A is [K][M] row-major (input-gradient form) */
    int32_t k_split;    /* 0, or multiple of 16: contraction rows k >= k_split are read from (A2, X2) at row k-k_split */
    int32_t m_split;    /* 0, or multiple of 128: output rows m >= m_split are written to Y2 (row m-m_split) */
    int32_t pro_mode;   /* SEP_PRO_* */
    int32_t epi_flags;  /* SEP_EPI_* bitmask; RESIDUAL applies to Y rows only */
    int32_t accumulate; /* 1: Y2 (or Y when m_split==0) += result instead of = */
    int32_t arith;      /* SEP_ARITH_* */
    float eps;
    double count; /* number of valid elements per sample (C*T) of the gLN used by the prologue */
    const float* A;
    const float* A2;
    const float* X;
    const float* X2;
    float* Y;
    float* Y2;
    const float* bias; /* [M] or NULL */
    const float* pro_alpha;
    const double* pro_stats;
    const float* pro_gamma;
    const float* pro_beta;
    const float* pro_aux;
    const float* pro_bsum; /* GLN_BWD: [B][2] = mean(gamma g), mean(gamma g xhat) of the gLN being back-propagated (bsum1 of sep_dwconv_bwd,
                              bsum of sep_gln_bwd_from_wgrad / sep_gln_bwd_finalize) */
    const double* pro_bacc; /* GLN_BWD, instead of pro_bsum: [B][SEP_STATS_SLOTS][2], the raw sums {sum_c gamma_c sum_t g, sum_c gamma_c sum_t g*u} a
                               producer only added up (sep_dwconv_bwd's bacc1 without arrive1 / bsum1); the kernel forms the two means itself */
    float* pro_store;
    double* pro_dalpha;
    const float* epi_alpha;
    double* epi_stats;
    const float* epi_res;
    const float* epi_aux;
    double* epi_dalpha;
    float* epi_rowpart;
    const float* a_amax; /* SEP_ARITH_F16X3: device scalar >= max|A| (and |A2|); any upper bound, e.g. over all parameters */
    const void* A_pk;       /* SEP_ARITH_F16X3: A ([M][K], already in the orientation of the product: the transpose and the
                               [A|A2] concatenation of a k_split call are done by the packer) as written by sep_pack_weights,
                               or NULL.  A / A2 / trans_a must still describe the fp32 weights: shapes the packed kernel does
                               not cover run on them. */
    const float* a_rscale;  /* [M] = 2^-e_m, the inverse row scales belonging to A_pk */
} sep_gemm_desc;

int sep_pw_gemm(const sep_gemm_desc* d, sep_stream_t stream);

/* Weight packer of the SEP_ARITH_F16X3 path: for every segment, A[m][k] = trans ? W[k*ldw + m] : W[m*ldw + k] (M x K,
 * K % 8 == 0), e_m = 13 - exponent(max_k |A[m][k]|), and each group of 8 consecutive k becomes 32 bytes
 *     dst[(m*K/8 + g)*32 ..] = { fp16 hi[8] , fp16 lo[8] },  A*2^e_m = hi + lo (hi toward zero, 11 + 11 significand bits)
 * i.e. 4 bytes per weight like the fp32 matrix; rscale[m] = 2^-e_m.  One launch for up to 256 segments (all 1x1-conv
 * weights of a Conv-TasNet in both orientations).  Replaces nothing in the reference: it is the once-per-pass half of the
 * operand split of the nn.Conv1d(kernel_size=1) products (tdcn.py:86,173,175; conv_tasnet.py:335,341). */
typedef struct sep_pack_seg {
    const float* W;
    void* dst;      /* M*K*4 bytes, 32-byte aligned */
    float* rscale;  /* [M] */
    int32_t M, K, trans, ldw;
} sep_pack_seg;
int sep_pack_weights(const sep_pack_seg* segs_host, int nseg, sep_stream_t stream);

/* Weight gradient of a pointwise convolution (reduction over batch and frames) on MFMA:
 *     partial[s][m][n] = sum over the (b,t) columns of slab s of  Gp[b][m][t] * Xp[b][n][t]
 *     partial_bias[s][m] = sum of Gp[b][m][t]
 * followed by sep_reduce_slabs.  Replaces autograd's conv weight/bias gradient for the same
 * nn.Conv1d layers, and (with unfolded frames as X) for Encoder.conv1d (filterbank.py:212)
 * and Decoder.conv_transpose1d (filterbank.py:243). */
typedef struct sep_wgrad_desc {
    int32_t B, M, N, T, ldt;
    int32_t g_split; /* 0, or multiple of 128: rows m >= g_split of G are read from G2 */
    int32_t g_mul;   /* 1: Gp = G * Gaux[b / g_div] (latent = mask * w) */
    int32_t g_div;
    int32_t x_mode; /* SEP_PRO_NONE / PRELU / GLN / GLN_PRELU */
    int32_t x_div;  /* X (and its gLN stats) are indexed with b / x_div */
    int32_t nsplit; /* number of partial slabs, <= B*ldt/32; slab s covers the chunk range [s*ceil(C/nsplit), (s+1)*ceil(C/nsplit)) of the C = B*ldt/q
                      * frame chunks (q = 16 or 32, the kernel's choice).  SAMPLE-ALIGNED slabs: with nsplit = B*k and k a divisor of ldt/32,
                      * slab s holds frames of sample s/k only, in every kernel */
    int32_t arith;  /* SEP_ARITH_* */
    float eps;
    double count;
    const float* G;
    const float* G2;
    const float* Gaux;
    const float* X;
    const float* x_alpha;
    const double* x_stats;
    const float* x_gamma;
    const float* x_beta;
    float* partial;      /* [nsplit][M][N] */
    float* partial_bias; /* [nsplit][M] or NULL */
    /* ABI 23: the second G source PRE-SPLIT by sep_split_rows (NULL: not used).  With M = 256, g_split = 128 and slabs that lie inside one sample the fp16
     * weight-gradient kernel takes rows m >= g_split as ready {hi, lo} operands (no split arithmetic for them in any layer that reads the same tensor:
     * the skip gradient dS of the Conv-TasNet step is the second source of all 24 heads' weight gradients); G2 must still be given (other kernels,
     * other shapes fall back to it). */
    const void* G2_pre;    /* [B][M - g_split][ldt / 32] lines of 128 bytes: 32 hi then 32 lo fp16 of x * 2^e */
    const int32_t* g2_exps; /* [B][M - g_split]: e */
    const float* g2_sums;  /* [nsplit][M - g_split]: sum over the slab's frames (the bias partials of those rows), or NULL with partial_bias == NULL */
} sep_wgrad_desc;

int sep_pw_wgrad(const sep_wgrad_desc* d, sep_stream_t stream);
/* n <= 8 weight gradients that agree in EVERYTHING but G, G2, X, partial, partial_bias (e.g. the conv1 weight gradients of consecutive TCN layers,
 * which nothing in the backward pass waits for), as ONE launch where the fp16 producer / consumer kernel takes the shape: the grid stays one
 * workgroup per compute unit, so the caller gives every product 1/n of the slabs it would give a single call (nsplit of the descriptors) and
 * gets n times longer contractions per workgroup and 1/n of the slab traffic.  Other shapes / arithmetics: n calls of sep_pw_wgrad.
 * Same results as n separate calls with the same nsplit.  (ABI 23; reference: the same convolutions' weight gradients, tdcn.py:86.) */
int sep_pw_wgrad_batch(const sep_wgrad_desc* descs_host, int n, sep_stream_t stream);
/* Rows of an activation tensor split ONCE for every weight gradient that takes them as (second) G operand: for row r of sample b
 *   e = 13 - exponent(max_t |x[b][r][t]|)   (the row's maximum lands in [2^12, 2^13); an all-zero row: e = 0)
 *   out line (b, r, p) = { hi[32] | lo[32] } fp16 of x[b][r][32 p .. 32 p + 31] * 2^e,  hi = fp16 toward zero, lo = fp16(x 2^e - hi)
 *   sums[(b * k + q) * C + r] = sum of x[b][r][t] over the q-th of k equal frame ranges of the row (k slabs per sample: the bias partials)
 * out has the shape and row pitch of x (B, C, ldt floats).  ldt % (32 k) == 0.  (ABI 23; no reference counterpart: it is half of the operand split
 * of the heads' weight gradient, reference src/models/tdcn.py:173,175, hoisted out of the 24 layers.) */
int sep_split_rows(const float* x, void* out, int32_t* exps, float* sums, int B, int C, int T, int ldt, int k, sep_stream_t stream);

/* dst[i] (+)= scale * sum_s src[s*stride + i] for up to 64 independent segments in one launch
 * (deterministic second stage of every split reduction). */
typedef struct sep_reduce_seg {
    const float* src;
    float* dst;
    int32_t n, nslab;
    int64_t stride;
    int32_t accumulate;
    float scale;
} sep_reduce_seg;
int sep_reduce_slabs(const sep_reduce_seg* segs_host, int nseg, sep_stream_t stream);

/* dst(double scalar partials) -> float parameter gradient: dst[i] (+)= (float)src[i] */
int sep_f64_to_f32(const double* src, float* dst, int n, int accumulate, sep_stream_t stream);

/* Encoder.forward (filterbank.py:222-230) with ConvTasNet's input padding (conv_tasnet.py:145-149):
 *   w[b][n][f] = sum_{c,k} E[n][c][k] * xpad[b][c][S*f+k] (+ReLU), xpad = x shifted right by pad_left, zero elsewhere.
 * Also accumulates the gLN statistics of w (separator.norm1d, conv_tasnet.py:370). */
int sep_encoder_fwd(const float* x, const float* E, float* w, double* stats, int B, int Cin, int Tin, int N, int L,
                    int S, int F, int ldt, int pad_left, int relu, sep_stream_t stream);

/* frames[b][c*L+k][f] = xpad[b][c][S*f+k]  (the im2col operand of the encoder/decoder weight gradients) */
int sep_unfold(const float* x, float* frames, int Bp, int C, int Tin, int L, int S, int F, int ldt, int pad_left,
               sep_stream_t stream);

/* Depthwise dilated conv of ResidualBlock1d/DepthwiseSeparableConv1d (tdcn.py:113-132,177-186), forward:
 *   v = gLN(PReLU(a; alpha1)) ; v = 0 outside [0,T) ; z[c][t] = bd[c] + sum_k wd[c][k] * v[c][t+(k-1)*d]
 * and accumulation of the statistics of PReLU(z; alpha2) for the following gLN.  P = 3 only. */
int sep_dwconv_fwd(const float* a, const double* stats1, const float* gamma1, const float* beta1, const float* alpha1,
                   const float* wd, const float* bd, const float* alpha2, float* z, double* stats2, int B, int C, int T,
                   int ldt, int dilation, float eps, sep_stream_t stream);

/* Backward of [gLN2 o PReLU2 o depthwise] given dv2 = d(gLN2 output):
 *   du2 = r2*(gamma2*dv2 - mg2 - xhat2*mgx2) ; dz = du2*PReLU'(z) ; dv1 = depthwise^T(dz)
 * bsum2 [B][2] = {mg2, mgx2} = mean(gamma2 dv2), mean(gamma2 dv2 xhat2), written by the producer of dv2's sums (sep_gln_bwd_from_wgrad).
 * For gLN1 this kernel is the producer: bacc1 [B][SEP_STATS_SLOTS][2] (fp64, zeroed by the caller) receives its workgroups'
 * {sum_c gamma1_c sum_t dv1, sum_c gamma1_c sum_t dv1*u1}, arrive1 [B][SEP_ARRIVE_INTS] (int, zeroed) counts them, and the sample's LAST workgroup stores
 * bsum1 [B][2] = {mean(gamma1 dv1), mean(gamma1 dv1 xhat1)} for the consumer's prologue (sep_gemm_desc.pro_bsum) -- no second-stage launch
 * between the two (round 2: sep_gln_bwd_finalize, 98 launches per step on the critical path).  arrive1 = bsum1 = NULL: the sums only (the
 * consumer forms the means from them: sep_gemm_desc.pro_bacc -- what the Conv-TasNet step uses, this kernel has thousands of short
 * workgroups and the arrival protocol's two waited-for round trips cost it 10 us per launch); all three NULL: none of it.
 * Writes dv1 and, per (b, c, 1024-frame tile), 8 partial row sums into rowpart[b][c][ntile][8]:
 *   {sum dv1, sum dv1*u1, sum dz, sum dz*v1[t-d], sum dz*v1[t], sum dz*v1[t+d], sum du2*z*[z<=0], 0}
 * (u1 = PReLU(a), v1 = gLN1(u1) inside [0,T) and 0 outside; ntile = ceil(ldt/1024)).
 * bd (the depthwise bias, may be NULL): with it the kernel forms z = bd + depthwise(v1) again from `a`, which it reads anyway, instead of
 * reading z -- three streams of HBM instead of four (rows of up to 8192 frames; longer rows and bd = NULL read z). */
int sep_dwconv_bwd(const float* dv2, const float* z, const float* a, const double* stats1, const float* gamma1,
                   const float* beta1, const float* alpha1, const double* stats2, const float* gamma2,
                   const float* alpha2, const float* bsum2, const float* wd, const float* bd, float* dv1, float* rowpart,
                   double* bacc1, int* arrive1, float* bsum1, int B, int C, int T, int ldt, int dilation, float eps, sep_stream_t stream);

/* Second stage of every gLN backward (Appendix A of SURVEY.md).  rowpart is [B][C][ntile][nq], nq in {2, 8}:
 *   R1 = sum_tiles rowpart[..][0], R2 = sum_tiles rowpart[..][1]
 *   pbeta[b][c] = R1 ; pgamma[b][c] = r_b*(R2 - mu_b*R1)
 *   bsum[b] = { sum_c gamma_c*R1 / count , sum_c gamma_c*pgamma[b][c] / count }     (bsum may be NULL: inside the TCN layers of the fused
 *             Conv-TasNet path the producers publish these means themselves -- sep_dwconv_bwd's bsum1, sep_gln_bwd_from_wgrad's bsum -- and
 *             this kernel only forms the parameter gradients, off the critical path)
 *   nq == 8 additionally (pextra holds B*C*4 + B + B*C floats; the last B*C are scratch):
 *     pextra[b*4C + c]           = sum_tiles rowpart[..][2]      (depthwise bias gradient, per sample)
 *     pextra[b*4C + C + 3c + k]  = sum_tiles rowpart[..][3+k]    (depthwise weight gradient [C][3], per sample)
 *     pextra[B*4C + b]           = sum_{c,tiles} rowpart[..][6]  (PReLU slope gradient, per sample) */
int sep_gln_bwd_finalize(const float* rowpart, int ntile, int nq, const double* stats, const float* gamma, double count,
                         float eps, float* bsum, float* pbeta, float* pgamma, float* pextra, int B, int C,
                         sep_stream_t stream);

/* sep_gln_bwd_finalize for up to 64 gLNs in one launch per stage (same outputs; bsum may be NULL per segment). */
typedef struct sep_finalize_seg {
    const float* rowpart;
    const double* stats;
    const float* gamma;
    float* bsum;
    float* pbeta;
    float* pgamma;
    float* pextra;
    double count;
    float eps;
    int32_t ntile, nq, B, C;
} sep_finalize_seg;
int sep_gln_bwd_finalize_batch(const sep_finalize_seg* segs_host, int nseg, sep_stream_t stream);

/* gLN backward statistics FROM the weight gradient (round 3).  For y = W v with v = gLN(u), u = PReLU(z): the gradient at v is
 * dv = W^T g, and the row sums its gLN backward needs are contractions the weight gradient has already done,
 *     R1[n] = sum_t dv[n][t] = sum_m W[m][n] gs[m],        R2[n] = sum_t dv[n][t] u[n][t] = sum_m W[m][n] raw[m][n],
 * raw = sum_t g[m][t] u[n][t] (sep_pw_wgrad with x_mode = SEP_PRO_PRELU: the gain and shift of the norm left out), gs = sum_t g (its
 * bias slabs), both per sample -- the slabs must be SAMPLE-ALIGNED: nsplit = B * slabs_per_sample with slabs_per_sample dividing ldt / 32,
 * so that slab s holds frames of sample s / slabs_per_sample only.  Then the input-gradient product W^T g needs no ROWSUMS epilogue
 * and does not read z (reference tdcn.py:173-175 backward + modules/norm.py:18,27 backward).  Outputs:
 *     dW_b[b][m][n] = sc_bn raw_b[m][n] + sh_bn gs_b[m]      (the true per-sample weight gradient; sum over b with sep_reduce_slabs)
 *     pbeta[b][n] (+)= R1,  pgamma[b][n] (+)= rstd_b (R2 - mu_b R1)      (accumulate = 1 adds: a second product feeding the same gLN)
 *     bacc[b][slot] += { sum_n gamma_n R1, sum_n gamma_n R2 }   (fp64, zeroed by the caller; `products` calls feed one gLN -- e.g. the
 *                          output and the skip product when their weights are not adjacent -- each adding its share)
 *     bsum[b] = { mean(gamma dv), mean(gamma dv xhat) }         stored by the LAST workgroup of the last call (arrive [B][SEP_ARRIVE_INTS], int,
 *                          zeroed by the caller, counts the arrivals): what the consumer of dv reads (sep_dwconv_bwd's bsum2)
 * W is [M][N] row-major (rows of adjacent matrices may be handed over as one, e.g. [Wo; Ws]). */
int sep_gln_bwd_from_wgrad(const float* part, const float* part_bias, const float* W, const double* stats, const float* gamma,
                           const float* beta, double count, float eps, float* dW_b, float* pbeta, float* pgamma, double* bacc,
                           int* arrive, float* bsum, int B, int M, int N, int slabs_per_sample, int accumulate, int products,
                           sep_stream_t stream);

/* Backward tail of the separator head: dw = r0*(gamma0*dvw - mg - xhat*mgx) + dwm, times [w>0] if the encoder has ReLU
 * (bsum0 [B][2] = {mg, mgx} from sep_gln_bwd_finalize).
 * In place on dvw. (conv_tasnet.py:370 gLN backward + conv_tasnet.py:159-160 product rule + filterbank.py:227) */
int sep_head_bwd(float* dvw, const float* w, const float* dwm, const double* stats0, const float* gamma0,
                 const float* bsum0, int B, int C, int T, int ldt, double count, float eps, int relu,
                 sep_stream_t stream);

/* mask * w, Decoder.forward = basis synthesis + overlap-add, and the crop (conv_tasnet.py:159-169, filterbank.py:245-247):
 *   est[b][s][c][tau] = sum_{n,f,k: S*f+k = tau+pad_left} w[b][n][f] * m[b][s][n][f] * D[n][c][k]
 * latent (may be NULL) receives w*m as (B, n_src, N, ldt). */
int sep_decoder_fwd(const float* w, const float* m, const float* D, float* est, float* latent, int B, int n_src, int N,
                    int Cout, int L, int S, int F, int ldt, int Tout, int pad_left, sep_stream_t stream);

/* Backward of the same: given d_est, writes dpre as (B, n_src*N, ldt) and dwm[b][n][f] = sum_s dlatent*m.
 * raw_mask = 0: dpre = d(mask pre-activation) of a sigmoid mask; 1: dpre = d(mask) (softmax mask: sep_softmax_ch_bwd next). */
int sep_decoder_bwd(const float* d_est, const float* w, const float* m, const float* D, float* dpre, float* dwm, int B,
                    int n_src, int N, int Cout, int L, int S, int F, int ldt, int Tout, int pad_left, int raw_mask,
                    sep_stream_t stream);

/* mask_nonlinear = 'softmax' (conv_tasnet.py:353-357, 375): nn.Softmax(dim=1) over the n_src*N channels of a frame, in place
 * on y (B, C, ldt); backward in place on g given the forward output y: g <- y * (g - sum_c g*y).  Frames >= T are zeroed. */
int sep_softmax_ch_fwd(float* y, int B, int C, int T, int ldt, sep_stream_t stream);
int sep_softmax_ch_bwd(const float* y, float* g, int B, int C, int T, int ldt, sep_stream_t stream);

/* Cumulative layer norm (causal cLN), CumulativeLayerNorm1d of reference src/modules/norm.py:42-101 and its autograd backward:
 *   y = (x - m_t) / (sqrt(v_t) + eps) * gamma_c + beta_c with the mean / biased variance of all channels and frames <= t.
 * x, y, dy, dx: (B, C, ldt) fp32, frames contiguous, ldt % 4 == 0, frames >= T written as zeros; mean, rstd: (B, ldt) fp32 (ABI 20: rows of
 * ldt, entries >= T untouched), written by the forward and read by the backward; ws: scratch of sep_cln_ws_bytes(B, C, T, ldt) bytes, 16-byte
 * aligned (ABI 21: for C <= 512 one pass each way -- a workgroup holds all channels of a 32-frame tile and takes the prefix / suffix of the
 * earlier / later tiles from a look-back chain whose records live in ws, with the per-tile partial sums of the parameter gradients behind
 * them; for wider rows the column sums of three launches: (B, 2, ldt) fp64);
 * dgamma_part, dbeta_part: (B, C) per-sample sums, to be added over the samples (sep_reduce_slabs).
 * alpha (ABI 20; may be NULL): the single slope of a PReLU in FRONT of the norm (tdcn.py:113-116, 182-186: nonlinear1d then norm1d): the
 * kernels normalise u = PReLU(x; alpha), dx is the gradient at x, and dalpha_part (B, C) receives sum_t du * x * [x <= 0] per row. */
size_t sep_cln_ws_bytes(int B, int C, int T, int ldt);
int sep_cln_fwd(const float* x, const float* gamma, const float* beta, float* y, float* mean, float* rstd, double* ws, int B, int C,
                int T, int ldt, float eps, const float* alpha, sep_stream_t stream);
int sep_cln_bwd(const float* dy, const float* x, const float* gamma, const float* mean, const float* rstd, float* dx,
                float* dgamma_part, float* dbeta_part, double* ws, int B, int C, int T, int ldt, float eps, const float* alpha,
                float* dalpha_part, sep_stream_t stream);

/* gLN on TOKEN-MAJOR rows (ABI 20): x, y, dy, dx (nseq, L, C) with the C features contiguous -- the layout between the attention / LSTM /
 * Linear layers of the dual-path separators (dptnet.py:505-560 `norm1d(x.permute(1, 2, 0))`): statistics over the L*C values of a sequence
 * (biased variance, eps inside the root, as nn.GroupNorm(1, C)), gain / shift per feature.  C must divide 1024, C >= 4, (L*C) % 4 == 0.
 * stats (nseq, 2) = {mean, rstd}, written forward, read backward; part (nseq, 2, C) = {sum_t dy*xhat | sum_t dy} per sequence: summed over
 * the sequences they are d(gamma), d(beta).  ws (ABI 21): scratch of sep_gln_tokens_ws_bytes(nseq, L, C) bytes, 8-byte aligned; 0 bytes (ws may
 * be NULL) while the sequences alone fill the chip -- few long sequences (GALRNet normalises one per sample) are cut into slices whose
 * partial sums meet there. */
size_t sep_gln_tokens_ws_bytes(int nseq, int L, int C);
int sep_gln_tokens_fwd(const float* x, const float* gamma, const float* beta, float* y, float* stats, void* ws, int nseq, int L, int C, float eps,
                       sep_stream_t stream);
int sep_gln_tokens_bwd(const float* dy, const float* x, const float* gamma, const float* stats, float* dx, float* part, void* ws, int nseq, int L,
                       int C, sep_stream_t stream);

/* Scaled dot-product attention of the dual-path separators' transformer blocks (ABI 21): O = dropout(softmax(scale Q K^T)) V per (sequence,
 * head) -- the core of nn.MultiheadAttention as the reference calls it (models/dptnet.py:505-527, models/galr.py:160-226, the
 * nn.TransformerEncoderLayer of models/sepformer.py:395-520) and its autograd backward, fp32 on the matrix pipe.
 * qkv, dqkv: (N, L, 3, H, D) -- the packed input projection's output as it is; o, dout: (N, L, H, D); lse, delta: (N, H, L) (lse written
 * forward, read backward; delta is scratch of the backward).  L <= 320, D in {8, 16, 32}.  p_drop: dropout rate on the probabilities
 * (0: none); the mask is a function of (seed, n, h, query, key), so forward and backward must be given the same seed. */
int sep_attn_fwd(const float* qkv, float* o, float* lse, int N, int L, int H, int D, float scale, float p_drop, unsigned long long seed,
                 sep_stream_t stream);
int sep_attn_bwd(const float* qkv, const float* o, const float* dout, const float* lse, float* delta, float* dqkv, int N, int L, int H, int D,
                 float scale, float p_drop, unsigned long long seed, sep_stream_t stream);

/* Layer norm over the features of token-major rows with the residual sum in front of it (ABI 22): nn.LayerNorm(C) as the post-norm
 * nn.TransformerEncoderLayer of SepFormer applies it (reference models/sepformer.py:395-520: `norm1(x + dropout1(self_attention(x)))`,
 * `norm2(x + dropout2(feed_forward(x)))`) and GALRNet's channel norm (models/galr.py:172-190 LayerNormAlongChannel), one pass each way.
 *   forward : s = x + drop(res) ; y = (s - mu) rstd gamma + beta with mu / biased variance of the row's C values, eps inside the root
 *   backward: ds = the gradient at s (it is the gradient at x AND at drop(res)) ; dres = the gradient at res
 * x, res, s, y, dy, ds, dres: (rows, C) fp32, features contiguous, C a multiple of 4 and <= 1024.  res NULL: y = LN(x), s must be NULL and the
 * backward is given x as s; s NULL with a branch: the sum is not kept (inference).  stat (rows, 2) = {mu, rstd}, written forward, read backward.  p_drop: rate of the inverted dropout on
 * res (0: none; then dres must be NULL -- ds serves both); the mask is a function of (seed, element index), the hash of sep_attn_*, so the
 * backward must be given the forward's seed.  part: (sep_rownorm_parts(rows, C), 2, C) = {sum dy * xhat | sum dy} over each workgroup's rows:
 * summed over the slabs they are d(gamma), d(beta). */
int sep_rownorm_parts(long rows, int C);
int sep_rownorm_fwd(const float* x, const float* res, const float* gamma, const float* beta, float* s, float* y, float* stat, long rows, int C,
                    float eps, float p_drop, unsigned long long seed, sep_stream_t stream);
int sep_rownorm_bwd(const float* dy, const float* s, const float* gamma, const float* stat, float* ds, float* dres, float* part, long rows, int C,
                    float p_drop, unsigned long long seed, sep_stream_t stream);

/* ReLU + inverted dropout between the two Linear layers of the transformer layers' feed-forward sub-block (ABI 22; torch/nn/modules/
 * transformer.py _ff_block as models/sepformer.py:395-520 instantiates it): a = keep ? max(h, 0) / (1 - p) : 0 with the mask of sep_rownorm_*
 * (hash of (seed, element index)); backward dh = a != 0 ? dy / (1 - p) : 0 -- from the forward's OUTPUT, no mask, no seed.  n a multiple of 4. */
int sep_relu_drop_fwd(const float* h, float* a, long n, float p_drop, unsigned long long seed, sep_stream_t stream);
int sep_relu_drop_bwd(const float* dy, const float* a, float* dh, long n, float p_drop, sep_stream_t stream);

/* Stand-alone gLN (modules/norm.py:11-35) for callers outside the fused network. */
int sep_gln_stats(const float* x, double* stats, int B, int C, int T, int ldt, sep_stream_t stream);
int sep_gln_apply(const float* x, const double* stats, const float* gamma, const float* beta, float* y, int B, int C,
                  int T, int ldt, double count, float eps, sep_stream_t stream);
/* rowpart[b][c][ntile][2] = {sum_t dy, sum_t dy*x} per 1024-frame tile */
int sep_gln_bwd_rowsums(const float* dy, const float* x, float* rowpart, int B, int C, int T, int ldt,
                        sep_stream_t stream);
int sep_gln_bwd_apply(const float* dy, const float* x, const double* stats, const float* gamma, const float* bsum,
                      float* dx, int B, int C, int T, int ldt, double count, float eps, sep_stream_t stream);

/* Segment1d / OverlapAdd1d (models/transform.py:6-65) for rows = B*C padded rows of x (T valid frames, stride ldt):
 *   segment:     out[row][s][k] = xpad[row][s*hop + k]   (xpad = x shifted right by pad_left, zero elsewhere)
 *   overlap_add: out[row][t]    = sum_{s*hop + k == t + pad_left} y[row][s][k] for t < T, 0 for T <= t < ldt
 * adjoint pair: each one is the other's backward. */
int sep_segment(const float* x, float* out, int rows, int T, int ldt, int S, int chunk, int hop, int pad_left,
                sep_stream_t stream);
int sep_overlap_add(const float* y, float* out, int rows, int T, int ldt, int S, int chunk, int hop, int pad_left,
                    sep_stream_t stream);

/* Generic depthwise Conv1d of modules.conv.DepthwiseSeparableConv1d (src/modules/conv.py:13-29; nn.Conv1d(groups=C) with
 * kernel size Kw, stride, zero padding, dilation) on contiguous (B, C, T) tensors:
 *   y[b][c][to] = bias[c] + sum_k w[c][k] * xpad[b][c][to*stride + k*dil - pad]
 * bwd_weight writes partial[b][c][0..Kw-1] = dL/dw contributions and partial[b][c][Kw] = dL/dbias contribution of row (b,c). */
int sep_depthwise_fwd(const float* x, const float* w, const float* bias, float* y, int B, int C, int Tin, int Tout, int Kw,
                      int stride, int pad, int dil, sep_stream_t stream);
int sep_depthwise_bwd_input(const float* dy, const float* w, float* dx, int B, int C, int Tin, int Tout, int Kw, int stride,
                            int pad, int dil, sep_stream_t stream);
int sep_depthwise_bwd_weight(const float* dy, const float* x, float* partial, int B, int C, int Tin, int Tout, int Kw,
                             int stride, int pad, int dil, sep_stream_t stream);

/* (B, C, T) <-> (B, C, ldt) repack with zero fill of the pad frames */
int sep_repack(const float* src, int ld_src, float* dst, int ld_dst, int rows, int T, sep_stream_t stream);

/* SI-SDR (criterion/sdr.py:122-139): per batch item and per (i, j) pair the three dot products
 *   dots[b][i][j] = <est_i, tgt_j>, tt[b][j] = |tgt_j|^2, xx[b][i] = |est_i|^2      (double)
 * all_pairs = 0 computes only i == j. */
int sep_sisdr_dots(const float* est, const float* tgt, double* dots, double* tt, double* xx, int B, int n, int T,
                   int all_pairs, sep_stream_t stream);
/* sisdr[b][i][j] (float) from the dot products, reference formula with eps. */
int sep_sisdr_from_dots(const double* dots, const double* tt, const double* xx, float* sisdr, int B, int n,
                        int all_pairs, float eps, sep_stream_t stream);
/* d_est[b][i][:] = sum_j gw[b][i][j] * d sisdr_ij / d est_i ; gw = dL/d sisdr (float, [B][n][n]; diagonal only if !all_pairs) */
int sep_sisdr_bwd(const float* est, const float* tgt, const double* dots, const double* tt, const double* xx,
                  const float* gw, float* d_est, int B, int n, int T, int all_pairs, float eps, sep_stream_t stream);

/* PIT search (criterion/pit.py:9-44) on the pair matrix: score[b][p] = reduce_s val[b][s][perm_p(s)] with
 * reduce = mean (or sum); picks min (maximize=0) or max; ties resolve to the first permutation in
 * itertools.permutations order like torch.min/max.  perms is [P][n] int32.  best_idx int64 [B], best_val float [B]. */
int sep_pit_search(const float* val, const int32_t* perms, int P, int n, int B, int maximize, int use_mean,
                   float* best_val, int64_t* best_idx, sep_stream_t stream);

/* Sinkhorn PIT (criterion/pit.py:163-193) on the cost matrix C[b][n][n] (float):
 * forward keeps every iterate in zwork (double [B][2*iters+1][n][n]) for the reverse sweep. */
int sep_sinkhorn_fwd(const float* C, double* zwork, float* loss, float* P, int B, int n, float coldness, int iters,
                     sep_stream_t stream);
int sep_sinkhorn_bwd(const float* C, const double* zwork, const float* dloss, float* dC, int B, int n, float coldness,
                     int iters, sep_stream_t stream);

/* The O(T) part of the waveform-distance criteria (reference src/criterion/distance.py:7-285: L1Loss, L2Loss,
 * SquaredError, MeanAbsoluteError, MeanSquaredError) and of plain SDR (src/criterion/sdr.py:6-22), over the last axis:
 *   sums[row] = { sum |x-t|, sum (x-t)^2, sum t^2 }   (double [rows][3]; x, t float [rows][T])
 *   dx[row][i] = c_abs[row] * sign(x-t) + c_sq[row] * (x-t)     (either coefficient vector may be NULL = 0)
 * the per-row value and coefficients are a few scalars per row formed by the caller exactly as the reference formula
 * states (mean / sqrt / log10 / eps placement).  rows < 65536 for the backward. */
int sep_rowdiff_sums(const float* x, const float* t, double* sums, int64_t rows, int T, sep_stream_t stream);
int sep_rowdiff_bwd(const float* x, const float* t, const float* c_abs, const float* c_sq, float* dx, int64_t rows, int T,
                    sep_stream_t stream);

/* clip_grad_norm_ + Adam of the train step (egs/wsj0-mix/common/src/driver.py:152-155), fused on a flat buffer:
 *   sqnorm[0] += sum g^2  (double, caller zeroes) ; then
 *   g *= min(1, max_norm/(sqrt(sqnorm)+1e-6)) (if max_norm > 0) ; Adam(lr, b1, b2, eps, weight_decay), step t. */
int sep_sqnorm(const float* g, double* sqnorm, int64_t n, sep_stream_t stream);
int sep_adam_step(float* p, float* g, float* m, float* v, const double* sqnorm, int64_t n, float lr, float beta1,
                  float beta2, float eps, float weight_decay, float max_norm, float grad_scale, int step,
                  sep_stream_t stream);

/* The same step with its two per-step scalars in DEVICE memory, so that a captured launch (hipGraph of the whole train step)
 * replays correctly: step_dev[0] is incremented first (a one-thread kernel), then used for the bias corrections; lr_dev[0] is
 * read at run time (learning-rate halving of driver.py:101-111 is a host write into that word between replays). */
int sep_adam_step_dev(float* p, float* g, float* m, float* v, const double* sqnorm, int64_t n, const float* lr_dev,
                      int32_t* step_dev, float beta1, float beta2, float eps, float weight_decay, float max_norm,
                      float grad_scale, sep_stream_t stream);

/* Time recurrence of ONE direction of nn.LSTM (reference src/models/dprnn.py:9-148 -> choose_rnn('lstm'), i.e.
 * IntraChunkRNN / InterChunkRNN of DPRNN-TasNet).  The input projection is done by the caller (a plain GEMM):
 *   xg[seq][t][4H] = x[seq][t][:] W_ih^T + b_ih + b_hh,   gate order i, f, g, o as in torch.
 * forward : a_t = xg_t + W_hh h_{t-1};  c_t = sigmoid(a_f) c_{t-1} + sigmoid(a_i) tanh(a_g);  h_t = sigmoid(a_o) tanh(c_t),
 *           h_0 = c_0 = 0, t ascending (reverse = 0) or descending (reverse = 1).  gates (post-activation i,f,g,o) and
 *           cstate are saved for the backward sweep; both may be NULL for inference.
 * backward: dh_out[seq][t][H] = gradient at h_t  ->  dxg[seq][t][4H] = gradient at the pre-activations a_t (= at xg_t).
 *           The caller forms dW_ih = dxg^T x, dW_hh = dxg^T h_{t-1}, db = sum dxg, dx = dxg W_ih (plain GEMMs).
 * H in {16, 32, 64, 128}; w_hh is [4H][H] row-major.
 * reverse = 2 runs BOTH directions in one launch (a sweep occupies only nseq/16 compute units): every buffer then holds
 * two slabs back to back, slab 0 = forward in time, slab 1 = backward in time (xg [2][nseq][L][4H], w_hh [2][4H][H], ...).
 * Two sweep kernels exist: sixteen sequences per workgroup (v_mfma_f32_16x16x4_f32) and four (v_mfma_f32_4x4x1_16b_f32); the
 * library picks four while those workgroups fit one round on the chip.  OR-ing SEP_LSTM_FORCE16 / SEP_LSTM_FORCE4 into
 * `reverse` forces one of them for the call (tests). */
#define SEP_LSTM_FORCE16 0x100
#define SEP_LSTM_FORCE4 0x200
/* with reverse = 2: h_out (sep_lstm_fwd) and dh_out (sep_lstm_bwd) are ONE (nseq, L, 2H) buffer, forward direction in columns [0, H),
 * reversed in [H, 2H) -- the layout nn.LSTM(bidirectional=True) returns -- instead of two (nseq, L, H) slabs: no torch.cat / torch.stack
 * around the sweeps.  gates, cstate, xg and dxg keep one slab per direction. */
#define SEP_LSTM_INTERLEAVED 0x400
int sep_lstm_fwd(const float* xg, const float* w_hh, float* h_out, float* gates, float* cstate, int nseq, int L, int H,
                 int reverse, sep_stream_t stream);
int sep_lstm_bwd(const float* dh_out, const float* gates, const float* cstate, const float* w_hh, float* dxg, int nseq,
                 int L, int H, int reverse, sep_stream_t stream);

/* Token-major dense layers of the dual-path separators (fp32 on the matrix pipe): the LSTMs' input projections and the nn.Linear behind
 * them at reference src/models/dprnn.py:65-148, with their gradients -- torch.addmm / `@` on [tokens][features] activations (features
 * contiguous) and torch's [N out][K in] weights.  K and N: multiples of 64 (sep_linear_fwd: K of 32; sep_linear_bwd_input: N of 32).
 *   sep_linear_fwd         y[t][n] = sum_k x[t][k] w[n][k] + bias[n] + bias2[n]          (bias, bias2 may be NULL)
 *   sep_linear_bwd_input   dx[t][k] = sum_n dy[t][n] w[n][k]                             (accumulate != 0: added to dx)
 *   sep_linear_bwd_weight  partial[s][n][k] = sum over the tokens of slab s of dy[t][n] x[t + shift][k],  s < nslab (the caller adds the
 *                          slabs: sep_reduce_slabs), partial_bias[s][n] = sum of dy[t][n] over the same tokens (may be NULL).
 *                          shift in {-1, 0, +1} and L: with shift != 0 the tokens are sequences of L steps (ntok % L == 0) and x[t + shift]
 *                          is the previous / next step's row of the SAME sequence, zero at its first / last step: the h_{t-1} operand of
 *                          the recurrent weights' gradient (dW_hh = sum_t dgates_t h_{t-1}^T) taken from h itself.  ldx: row stride of x in
 *                          floats (>= K, multiple of 4; x 16-byte aligned): one direction's half of an interleaved bi-LSTM output. */
int sep_linear_fwd(const float* x, const float* w, const float* bias, const float* bias2, float* y, long ntok, int K, int N,
                   sep_stream_t stream);
int sep_linear_bwd_input(const float* dy, const float* w, float* dx, long ntok, int K, int N, int accumulate, sep_stream_t stream);
int sep_linear_bwd_weight(const float* dy, const float* x, long ldx, float* partial, float* partial_bias, long ntok, int K, int N, int L,
                          int shift, int nslab, sep_stream_t stream);

/* The layout change in front of and behind those layers (reference src/models/dprnn.py:73-76,123-126, the permute / reshape pairs around
 * the intra- and inter-chunk recurrences), each the other's inverse and backward:
 *   sep_chunk_to_tokens   y[b][s][k][f] = x[b][f][s][k]   (inter = 0: sequences over k for every (b, s): y is (B*S, K, F))
 *                         y[b][k][s][f] = x[b][f][s][k]   (inter = 1: sequences over s for every (b, k): y is (B*K, S, F))
 *   sep_tokens_to_chunk   the reverse, x (B, F, S, K) contiguous. */
int sep_chunk_to_tokens(const float* x, float* y, int B, int F, int S, int K, int inter, sep_stream_t stream);
int sep_tokens_to_chunk(const float* y, float* x, int B, int F, int S, int K, int inter, sep_stream_t stream);

/* ---- recorded launch sequences (ABI 23) ------------------------------------------------------------------------------------
 * One C-ABI call per pass instead of one Python call per kernel.  The host runs a step ONCE through the ordinary entry points while it
 * records every call as a sep_seq_op -- the entry point's id (sep_seq_lookup) and its arguments in order, WITHOUT the trailing stream:
 * pointers (device buffers, and HOST descriptors / segment arrays the caller keeps alive and unchanged) in .p, integers in .i, float /
 * double parameters in .f.  sep_run_sequence then calls the same entry points again, in order, on `stream`; it stops at the first op that
 * fails and returns that op's code (sep_last_error names the op).  The buffers named by the ops must stay allocated at the recorded
 * addresses; values that change between runs live in device memory (sep_adam_step_dev's step count and learning rate, the input batch).
 * Replaces the per-launch Python of the train step of reference egs/wsj0-mix/common/src/driver.py:141-157 (model(mixture) ->
 * pit_criterion -> backward -> clip_grad_norm_ -> optimizer.step()); there is no FFI there to cite: the reference issues the same work as
 * ~900 ATen launches from the interpreter. */
#define SEP_SEQ_MAX_ARGS 26
typedef union sep_seq_arg {
    int64_t i;
    double f;
    const void* p;
} sep_seq_arg;
typedef struct sep_seq_op {
    int32_t fn;    /* sep_seq_lookup(name) */
    int32_t nargs; /* must equal sep_seq_nargs(fn) */
    sep_seq_arg args[SEP_SEQ_MAX_ARGS];
} sep_seq_op;
int sep_seq_count(void);              /* number of recordable entry points: ids are 0 .. count-1 */
int sep_seq_lookup(const char* name); /* id of the entry point `name`, -1 if it cannot be recorded (queries without a stream) */
const char* sep_seq_name(int fn);
int sep_seq_nargs(int fn); /* parameters of the entry point minus the stream */
int sep_run_sequence(const sep_seq_op* ops_host, int n, sep_stream_t stream);

/* What a fully recorded step needs where the eager step used torch kernels:
 *   sep_memset      hipMemsetAsync on the stream (statistics slots, fp64 accumulators, arrival counters: `torch.zeros` in the eager step)
 *   sep_absmax      out[0] = max |x[i]|: the A-operand bound a_amax of SEP_ARITH_F16X3 over the flat parameter buffer
 *   sep_pit_finish  tail of PIT (criterion/pit.py:33-44) behind sep_pit_search, and its backward: loss[0] = sign * mean_b best_val[b];
 *                   gw[b][i][j] = sign * scale if j == perms[best_idx[b]][i] else 0 (the dL/d sisdr matrix sep_sisdr_bwd takes: scale =
 *                   1 / (B n) for a mean over sources and batch); pattern[b][i] = perms[best_idx[b]][i] (int64).  loss, gw, pattern may be NULL. */
int sep_memset(void* dst, int value, size_t bytes, sep_stream_t stream);
int sep_absmax(const float* x, int64_t n, float* out, sep_stream_t stream);
int sep_pit_finish(const float* best_val, const int64_t* best_idx, const int32_t* perms, int P, int n, int B, float sign, float scale,
                   float* loss, float* gw, int64_t* pattern, sep_stream_t stream);
/*   sep_axpby       out[i] = a x[i] + b y[i] (y may be NULL; out may alias x or y): the sign flips between criterion kernels the eager step leaves to
 *                   torch -- SinkPIT's cost matrix C = -SI-SDR and dL / d SI-SDR = -dL / dC (criterion/pit.py:143-146).  With best_idx = perms = NULL
 *                   sep_pit_finish only forms loss[0] = sign * mean_b best_val[b] (the batch mean of SinkPIT's per-item losses, pit.py:155-156). */
int sep_axpby(const float* x, float a, const float* y, float b, float* out, int64_t n, sep_stream_t stream);

/* ---- online (chunk-by-chunk) separation of a causal Conv-TasNet (ABI 23, additive) ------------------------------------------------
 * Symbols added to ABI 23 without changing any existing one.  sepkernels/online.py (OnlineSeparator) runs a chunk of n encoder frames of
 * every stream (n S samples each) as one pass over STREAM-MAJOR columns: column j = stream * n + frame of a (C, ldt) matrix, ldt a multiple
 * of 128 >= num_streams * n, columns beyond zero.  Per-stream state, all in device memory (a recorded chunk step replays correctly):
 *   carry  (num_streams, L - S)           the last L - S input samples (starts as zeros: the pre-roll)
 *   frames (num_streams) int64            encoder frames seen so far
 *   sums   (num_streams, sums_stride)     fp64 {sum x, sum x^2} of every cLN, 2 per norm
 *   ring   (num_streams, ring_stride)     per TCN layer the last (P - 1) d frames of its depthwise input, (C, (P - 1) d) in time order
 *   tail   (num_streams, n_src, L - S)    overlap-add samples not yet final
 * The reference formulas: filterbank.py:205-251 (encoder / decoder), modules/norm.py:58-101 (cLN), tdcn.py:125-132 (causal taps).
 *   sep_online_encoder_fwd    w[nb][s n + f] = [ReLU] sum_k E[nb][k] ext_s[f S + k], ext_s = [carry_s | chunk_s]; carry_next_s = the last L - S
 *                             samples of ext_s.  chunk (num_streams, n S).  carry / carry_next may be NULL when L == S.
 *   sep_online_cln_fwd        y = (u - m_t) r_t gamma + beta with u = x or PReLU(x; alpha) (alpha may be NULL), m_t / r_t of norm.py:58-101 over
 *                             everything the stream has seen: count C (t + 1), t = frames[s] + f.  sums (fp64) are read and updated.
 *   sep_online_depthwise_fwd  y[c][s n + f] = bias[c] + sum_k w[c][k] ext[f + k d], ext = [ring (P - 1) d | x]; the ring takes the last (P - 1) d
 *                             frames of ext.  Any P >= 2, (P - 1) d <= 16384.  bias may be NULL.
 *   sep_online_decoder_fwd    out[s][src][i] (i < n S) and tail_next[s][src][i - n S] = tail[s][src][i] (i < L - S) + sum over the frames f of the
 *                             chunk with f S <= i < f S + L of sum_nb w[nb][s n + f] mask[src N + nb][s n + f] D[nb][i - f S].
 *   sep_online_advance        frames += n; carry <- carry_next; tail <- tail_next (carry_len, tail_len: floats per stream).  The last launch of a chunk.
 *   sep_online_reset          for every stream s with mask[s] != 0: frames[s] = 0 and its slices of carry, sums, rings, tail (lengths per stream) = 0.
 * SLOTS.  The state buffers may hold more streams than a pass runs.  Each sep_online_*_sel is its sibling plus `const int32_t* slots`, device
 * memory of num_streams entries, and num_streams is then the number of COLUMN BLOCKS of the pass: block j (columns [j n, (j + 1) n), row j of
 * chunk and of out) reads and updates the state of stream slots[j] -- the encoder its rows of carry / carry_next, the cLN its row of sums and
 * frames[slots[j]], the depthwise kernel its row of ring, the decoder its rows of tail / tail_next; sep_online_advance_sel adds n to
 * frames[slots[j]] and copies carry_next -> carry and tail_next -> tail for those rows only.  Rows of streams that slots does not name are
 * neither read nor written, those of carry_next / tail_next included.  Entries must be distinct and inside the state buffers: the library
 * cannot look at device memory, duplicates or entries out of range are undefined (sepkernels/online.py checks before it uploads).  The list
 * is read when the kernels run, so a recorded pass replays for whatever selection of num_streams streams the buffer holds by then.  Both
 * forms are instances of the same kernels (the indirection is a template argument); the plain entry points compute what they did before the
 * _sel ones existed, bit for bit.
 * RAGGED.  Each sep_online_*_rag is its _sel sibling plus `const int32_t* offs`, device memory of num_streams + 1 entries next to the slot list:
 * column block j is [offs[j], offs[j + 1]) with offs[0] = 0, so stream slots[j] brings n_j = offs[j + 1] - offs[j] >= 1 frames of its own, the
 * columns are compact, and ldt is a multiple of 128 >= offs[num_streams].  `n` becomes n_cap: the widest block allowed and the row pitch of
 * chunk (num_streams, n_cap S) and out (num_streams, n_src, n_cap S) in hops.  The encoder reads the first n_j S samples of row j and nothing
 * beyond (the rest may hold anything, NaN included), finds a column's block by a search in offs, and its carry_next is the last L - S samples
 * of [carry | n_j S samples]; the cLN runs one workgroup per block over n_j frames with t = frames[slots[j]] + f; the depthwise kernel runs
 * workgroup (channel, block), and n_j < (P - 1) d and n_j > (P - 1) d may meet in one launch; the decoder writes samples [0, n_j S) of row j,
 * ZERO in [n_j S, n_cap S), and takes tail_next from position n_j S on; sep_online_advance_rag adds n_j to frames[slots[j]] and copies carry /
 * tail back for the named rows only.  Every kernel that writes a matrix writes its columns [offs[num_streams], ldt) as zero.  Ownership is that
 * of the _sel form: no atomics, rows of unnamed streams are neither read nor written (second buffers included).  slots is required (all
 * streams: the identity list).  offs is read when the kernels run, so a recorded pass replays for other lengths with an ldt that still holds
 * them.  The library cannot look at device memory: an offs that is not increasing, a block wider than n_cap or offs[num_streams] > ldt is
 * undefined (sepkernels/online.py checks before it uploads).  The plain and _sel entry points stay the instances they were (the ragged path is
 * a further template argument), bit for bit. */
int sep_online_encoder_fwd(const float* chunk, const float* E, const float* carry, float* carry_next, float* w, int num_streams, int N, int L, int S,
                           int n, int ldt, int relu, sep_stream_t stream);
int sep_online_cln_fwd(const float* x, const float* alpha, const float* gamma, const float* beta, float* y, double* sums, int sums_stride,
                       const int64_t* frames, int num_streams, int C, int n, int ldt, float eps, sep_stream_t stream);
int sep_online_depthwise_fwd(const float* x, const float* w, const float* bias, float* ring, int64_t ring_stride, float* y, int num_streams, int C,
                             int n, int ldt, int P, int dilation, sep_stream_t stream);
int sep_online_decoder_fwd(const float* w, const float* mask, const float* D, const float* tail, float* tail_next, float* out, int num_streams,
                           int n_src, int N, int L, int S, int n, int ldt, sep_stream_t stream);
int sep_online_advance(int64_t* frames, float* carry, const float* carry_next, int carry_len, float* tail, const float* tail_next, int tail_len,
                       int num_streams, int n, sep_stream_t stream);
int sep_online_reset(const uint8_t* mask, int num_streams, int64_t* frames, float* carry, int carry_len, double* sums, int sums_len, float* rings,
                     int64_t rings_len, float* tail, int tail_len, sep_stream_t stream);
int sep_online_encoder_fwd_sel(const float* chunk, const float* E, const float* carry, float* carry_next, float* w, int num_streams, int N, int L,
                               int S, int n, int ldt, int relu, const int32_t* slots, sep_stream_t stream);
int sep_online_cln_fwd_sel(const float* x, const float* alpha, const float* gamma, const float* beta, float* y, double* sums, int sums_stride,
                           const int64_t* frames, int num_streams, int C, int n, int ldt, float eps, const int32_t* slots, sep_stream_t stream);
int sep_online_depthwise_fwd_sel(const float* x, const float* w, const float* bias, float* ring, int64_t ring_stride, float* y, int num_streams,
                                 int C, int n, int ldt, int P, int dilation, const int32_t* slots, sep_stream_t stream);
int sep_online_decoder_fwd_sel(const float* w, const float* mask, const float* D, const float* tail, float* tail_next, float* out, int num_streams,
                               int n_src, int N, int L, int S, int n, int ldt, const int32_t* slots, sep_stream_t stream);
int sep_online_advance_sel(int64_t* frames, float* carry, const float* carry_next, int carry_len, float* tail, const float* tail_next, int tail_len,
                           int num_streams, int n, const int32_t* slots, sep_stream_t stream);
int sep_online_encoder_fwd_rag(const float* chunk, const float* E, const float* carry, float* carry_next, float* w, int num_streams, int N, int L,
                               int S, int n_cap, int ldt, int relu, const int32_t* slots, const int32_t* offs, sep_stream_t stream);
int sep_online_cln_fwd_rag(const float* x, const float* alpha, const float* gamma, const float* beta, float* y, double* sums, int sums_stride,
                           const int64_t* frames, int num_streams, int C, int n_cap, int ldt, float eps, const int32_t* slots, const int32_t* offs,
                           sep_stream_t stream);
int sep_online_depthwise_fwd_rag(const float* x, const float* w, const float* bias, float* ring, int64_t ring_stride, float* y, int num_streams,
                                 int C, int n_cap, int ldt, int P, int dilation, const int32_t* slots, const int32_t* offs, sep_stream_t stream);
int sep_online_decoder_fwd_rag(const float* w, const float* mask, const float* D, const float* tail, float* tail_next, float* out, int num_streams,
                               int n_src, int N, int L, int S, int n_cap, int ldt, const int32_t* slots, const int32_t* offs, sep_stream_t stream);
int sep_online_advance_rag(int64_t* frames, float* carry, const float* carry_next, int carry_len, float* tail, const float* tail_next, int tail_len,
                           int num_streams, int n_cap, const int32_t* slots, const int32_t* offs, sep_stream_t stream);

/* ---- the causal TCN layer's first norm folded into its depthwise convolution (ABI 23, additive; csrc/causal.hip) ------------------------
 * The first cLN of a causal layer (tdcn.py:107-147) feeds only the depthwise convolution, so its output v1 need not exist in memory:
 *   sep_cln_stats                 sep_cln_fwd without the apply pass and without y: mean, rstd (B, ldt), bit for bit what sep_cln_fwd writes
 *                                 (same ws, same alpha convention).
 *   sep_depthwise_cln_fwd         y[b][c][t] = bias[c] + sum_k w[c][k] v1[b][c][t + k dil - pad] for t < T, zero for T <= t < ldt, with
 *                                 v1[b][c][t'] = gamma[c] (PReLU(x[b][c][t']; alpha) - mean[b][t']) rstd[b][t'] + beta[c] for 0 <= t' < T and ZERO
 *                                 outside (the reference pads after the norm).  x, y (B, C, ldt), ldt % 4 == 0; w (C, Kw); any Kw >= 1,
 *                                 dil >= 1, 0 <= pad <= (Kw - 1) dil.  alpha and bias may be NULL.
 *   sep_depthwise_cln_bwd_weight  partial[b][c][k] = sum_{t < T} dy[b][c][t] v1[b][c][t + k dil - pad] (k < Kw), partial[b][c][Kw] = sum_{t < T} dy:
 *                                 sep_depthwise_bwd_weight with its x operand re-formed by the same prologue; to be added over b.
 * The gradient at x needs nothing new: sep_depthwise_bwd_input yields d v1, sep_cln_bwd takes x, mean, rstd and alpha.
 *   sep_sum_f64                   out[0] = sum_i x[i] over n floats, accumulated in fp64 in a fixed order: the (B, C) row partials of a PReLU
 *                                 slope's gradient (sep_cln_bwd's dalpha_part) -> the one slope, inside a recorded step. */
int sep_sum_f64(const float* x, int64_t n, float* out, sep_stream_t stream);
int sep_cln_stats(const float* x, float* mean, float* rstd, double* ws, int B, int C, int T, int ldt, float eps, const float* alpha,
                  sep_stream_t stream);
int sep_depthwise_cln_fwd(const float* x, const float* alpha, const float* gamma, const float* beta, const float* mean, const float* rstd,
                          const float* w, const float* bias, float* y, int B, int C, int T, int ldt, int Kw, int pad, int dil, sep_stream_t stream);
int sep_depthwise_cln_bwd_weight(const float* dy, const float* x, const float* alpha, const float* gamma, const float* beta, const float* mean,
                                 const float* rstd, float* partial, int B, int C, int T, int ldt, int Kw, int pad, int dil, sep_stream_t stream);

/* ---- the causal TCN layer with full k-tap convolutions (separable=False) on the 1x1 products (ABI 23, additive) ------------------------------
 * A layer of ConvTasNet(causal=True, separable=False) (reference tdcn.py:100-147) is conv1 -> PReLU + cLN -> left padding (P - 1) d -> two
 * nn.Conv1d(H, M, P, dilation=d), output_conv1d and skip_conv1d.  With the activation UNFOLDED over the taps into rows c P + p, a weight
 * (M, H, P) is -- in place -- the row-major (M, H P) matrix of a 1x1 product, so both convolutions, their input gradient ([Wo; Ws]^T product,
 * then the adjoint fold) and their weight gradients (sep_pw_wgrad, already in the parameters' layout) are the separable layers' products.
 *   sep_unfold_dilated      cols[b][c P + p][t] = x[b][c][t + p dil - pad] where t < T and 0 <= t + p dil - pad < T, ZERO elsewhere, every
 *                           column of [T, ldt) included.  x (B, C, ldt), cols (B, C P, ldt), ldt % 4 == 0; any P >= 1, dil >= 1,
 *                           0 <= pad <= (P - 1) dil (the causal layers: pad = (P - 1) dil).  Columns [T, ldt) of x may hold anything (NaN
 *                           included) and do not reach the output.  Copies only: the result is exact.
 *   sep_fold_dilated        the adjoint: dx[b][c][u] = sum_p dcols[b][c P + p][u - p dil + pad] over the p whose column u - p dil + pad lies in
 *                           [0, T), added in ascending p; ZERO for T <= u < ldt.  A gather: one writer per element, no atomics, bit-stable.
 *                           Columns [T, ldt) of dcols may hold anything.
 *   sep_online_unfold_fwd   (+ _sel, _rag) sep_online_depthwise_fwd without its taps: cols[c P + p][column of (stream, f)] = ext[f + p d],
 *                           ext = [ring (P - 1) d | x]; the ring then takes the last (P - 1) d frames of ext.  cols (C P, ldt).  The ring layout,
 *                           ring_stride, the slot list, offs and every ownership rule are sep_online_depthwise_fwd's; columns beyond the last
 *                           block are written as zero in all C P rows.  Any P >= 1, (P - 1) d <= 16384; ring may be NULL when P == 1. */
int sep_unfold_dilated(const float* x, float* cols, int B, int C, int T, int ldt, int P, int dil, int pad, sep_stream_t stream);
int sep_fold_dilated(const float* dcols, float* dx, int B, int C, int T, int ldt, int P, int dil, int pad, sep_stream_t stream);
int sep_online_unfold_fwd(const float* x, float* ring, int64_t ring_stride, float* cols, int num_streams, int C, int n, int ldt, int P, int dilation,
                          sep_stream_t stream);
int sep_online_unfold_fwd_sel(const float* x, float* ring, int64_t ring_stride, float* cols, int num_streams, int C, int n, int ldt, int P,
                              int dilation, const int32_t* slots, sep_stream_t stream);
int sep_online_unfold_fwd_rag(const float* x, float* ring, int64_t ring_stride, float* cols, int num_streams, int C, int n_cap, int ldt, int P,
                              int dilation, const int32_t* slots, const int32_t* offs, sep_stream_t stream);

/* ---- export / import of the online separator's per-stream state (ABI 23, additive; csrc/online.hip) ------------------------------------------
 * The five state buffers above (frames, carry, sums, rings, tail; carry_len, sums_len, rings_len, tail_len are the element counts PER STREAM, the
 * vocabulary of sep_online_reset) hold everything a stream carries from chunk to chunk.  These entry points move the complete state of the
 * streams a slot list names into a caller's blob and back, so a stream can leave the buffers it started in: migrate to other buffers (another
 * number of slots, another process, another GPU via the host), persist, or be rewound to an earlier export -- for some slots while the others
 * keep running.  carry_next / tail_next are not part of the state: sep_online_advance is the last launch of every chunk, between two chunks
 * they are scratch, and neither entry point takes or touches them.
 * ROW FORMAT, VERSION 1.  One stream is one row of sep_online_state_row_bytes(carry_len, sums_len, rings_len, tail_len) bytes, little endian,
 * the sections in this order and at these byte offsets:
 *        0                      int64   frames
 *        8                      double  sums[sums_len]
 *        8 + 8 sums_len         zero bytes up to the next multiple of 16 =: R
 *        R                      float   rings[rings_len]
 *        R + 4 rings_len        float   carry[carry_len]
 *        .. + 4 carry_len       float   tail[tail_len]
 *        .. + 4 tail_len        zero bytes up to the next multiple of 16 = row_bytes
 * so rings, the large section, starts on a 16-byte boundary of a 16-byte aligned row (H % 16 == 0 makes rings_len a multiple of 16 floats, and
 * carry and tail then start on one too when their lengths are multiples of 4).  A format that lays a row out differently gets another version
 * number; the number is kept by the caller next to the blob (sepkernels/online.py: OnlineState.version), not inside the rows.
 *   sep_online_state_row_bytes   the size of one row, a multiple of 16 (0 for a negative length).  Not a launch: no stream, no sequence-table entry.
 *   sep_online_state_export      row j of blob, at byte j * row_pitch, receives the state of stream slots[j]; the padding bytes inside a row are
 *                                written as zero; bytes [row_bytes, row_pitch) of a row are left untouched.  Nothing of a stream that slots does not
 *                                name is read.  The state buffers are not changed.
 *   sep_online_state_import      the exact inverse: the state of stream slots[j] receives row j.  No entry of a stream that slots does not name is
 *                                written.  The buffers may belong to another separator than the exporting one (another number of streams, other
 *                                slots) as long as the four lengths are the same; whether the MODEL is the same the library cannot know.
 * slots is device memory of num_streams (<= 65535) distinct entries inside the state buffers, read when the kernel runs (a recorded call replays
 * for whatever the buffer holds by then); duplicates or entries out of range are undefined, as for the _sel entry points.  blob is device memory,
 * 16-byte aligned, row_pitch >= row_bytes and row_pitch % 16 == 0; it must not overlap the state buffers.  A length may be zero (L == S: no carry,
 * no tail; a model without history: no rings) and its pointer then NULL.  Each call is ONE launch, grid (G, num_streams) with G workgroups
 * sharing a row; the sections are copied as integer words -- never through floating-point arithmetic, so every bit pattern (NaN payloads,
 * denormals) arrives unchanged -- in the widest of 16-, 8- and 4-byte accesses that the alignment of both sides of a section allows (carry_len
 * need not be a multiple of 4).  No atomics; all offsets are 64-bit (1024 streams x 3.13 MB exceeds 2^32 bytes).  Ownership: a caller that binds
 * the C ABI directly owns blob and the state buffers; the library keeps no copy and no pointer. */
size_t sep_online_state_row_bytes(int carry_len, int sums_len, int64_t rings_len, int tail_len);
int sep_online_state_export(const int32_t* slots, int num_streams, const int64_t* frames, const float* carry, int carry_len, const double* sums,
                            int sums_len, const float* rings, int64_t rings_len, const float* tail, int tail_len, void* blob, int64_t row_pitch,
                            sep_stream_t stream);
int sep_online_state_import(const int32_t* slots, int num_streams, int64_t* frames, float* carry, int carry_len, double* sums, int sums_len,
                            float* rings, int64_t rings_len, float* tail, int tail_len, const void* blob, int64_t row_pitch, sep_stream_t stream);

/* ---- BSS-eval v3 ("sources"): SDR, SIR and SAR of the test recipes (ABI 23, additive; csrc/bss.hip) --------------------------------------------
 * The metric of Vincent et al. 2006 as the reference's testers call it (src/utils/bss.py -> mir_eval.separation.bss_eval_sources,
 * egs/wsj0-mix/common/src/driver.py:291-309).  For references r_0 .. r_{n-1} and estimates e_0 .. e_{m-1} of T_b samples, all extended by flen - 1
 * zeros: P_i(e_j) is the least-squares projection of e_j on { r_i delayed by tau, tau = 0 .. flen - 1 }, P_all(e_j) the projection on the delayed
 * versions of every reference; s_filt = P_i(e_j), e_interf = P_all(e_j) - P_i(e_j), e_artif = e_j - P_all(e_j);
 * SDR = 10 log10(|s_filt|^2 / |e_interf + e_artif|^2), SIR = 10 log10(|s_filt|^2 / |e_interf|^2), SAR = 10 log10(|s_filt + e_interf|^2 / |e_artif|^2).
 * The projections solve normal equations whose entries are lagged correlations; that solve ((n flen)^2, a few thousand at most) is the CALLER's
 * (utils/bss.py: torch.linalg in fp64).  The two O(T flen) passes around it are these entry points, fp64 arithmetic on fp32 audio:
 *   sep_bss_xcorr          out[b][i][k][l] = sum_t a[b][i][t] c[b][k][t + lag_lo + l], l < nlag, over the t with both indices in [0, T_b); product and
 *                          sum in fp64.  a (B, n, T), c (B, m, T) fp32 rows of pitch T, out (B, n, m, nlag) fp64.  A lag without overlap
 *                          (|lag| >= T_b) is exactly 0.  One evaluation of the metric calls it twice: references x references with
 *                          lag_lo = -(flen - 1), nlag = 2 flen - 1 (the block-Toeplitz matrix G), and references x estimates with lag_lo = 0,
 *                          nlag = flen (the right-hand sides D).
 *   sep_bss_energies       ref (B, n, T), est (B, m, T); filt_all (B, m, n, flen): [b][j][k] is the filter on r_k in P_all(e_j); filt_one
 *                          (B, m, n, flen): [b][j][i] is the filter of P_i(e_j); both fp64.  out (B, m, n, 5) fp64: for the pair (e_j, r_i) the
 *                          sums over t in [0, T_b + flen - 1) of s_filt^2, e_interf^2, e_artif^2, (e_interf + e_artif)^2, (s_filt + e_interf)^2,
 *                          in this order.  The projected signals are never stored.
 *   sep_bss_scratch_bytes  the scratch that all three calls of one evaluation (the two sep_bss_xcorr above and sep_bss_energies) can share; 0 for
 *                          arguments they would refuse.  A single sep_bss_xcorr needs 8 B n m ceil(T / 2048) nlag bytes, sep_bss_energies
 *                          40 B n m ceil((T + flen - 1) / 1024).  Not a launch: no stream, no sequence-table entry.
 * lengths: device memory of B int32, T_b = lengths[b] clamped to [0, T], read when the kernels run; NULL means T_b = T for every row.  Samples at
 * and beyond T_b are never read.  No atomics: a workgroup owns one time slab of fixed size (2048 / 1024 samples, counted from sample 0) and
 * writes its partial sums to scratch, a second launch of the same call adds the slabs in ascending order.  So two runs give the same bits, and
 * a row gives the same bits whatever the pitch T and the rows around it are.  scratch is device memory of scratch_bytes bytes, 8-byte aligned,
 * checked against the need before anything is launched; its contents are scratch before and after.  All offsets are 64-bit.  B <= 65535,
 * n m <= 65535, T, flen and the lags within 2^30. */
size_t sep_bss_scratch_bytes(int B, int n, int m, int T, int flen);
int sep_bss_xcorr(const float* a, const float* c, const int32_t* lengths, double* out, double* scratch, size_t scratch_bytes, int B, int n, int m,
                  int T, int lag_lo, int nlag, sep_stream_t stream);
int sep_bss_energies(const float* ref, const float* est, const double* filt_all, const double* filt_one, const int32_t* lengths, double* out,
                     double* scratch, size_t scratch_bytes, int B, int n, int m, int T, int flen, sep_stream_t stream);

/* ---- BSS-eval v4 ("images"): museval's framewise SDR, ISR, SIR and SAR of music separation (ABI 23, additive; csrc/bss.hip) -------------------
 * The figure music separation is published with, as museval 0.4's metrics.bss_eval computes it for eval_mus_track (window = hop = 1 s,
 * filters_len = 512, framewise_filters = False, compute_permutation = False, images version; the reference's music tester ends there,
 * egs/musdb18/conv-tasnet/src/adhoc_driver.py:352-380).  Restated from that code; agreement with the museval PACKAGE itself is untested, it is on
 * none of the project's machines.  One recording has references r[i][c] and estimates e[j][c], i, j < n sources, c < C channels, T_b samples;
 * filter length F = flen, window W, hop H.
 *   Filters, once on the whole recording, every signal extended by F - 1 zeros: h_all[j][c][k][c2] (F taps each) minimises
 *   |e[j][c] - sum_{k,c2} h_all[j][c][k][c2] * r[k][c2]|^2 over all n C reference channels, h_one[j][c][c2] the same over the C channels of
 *   reference j alone.  Their normal equations are those of v3 above with n C rows in place of n: G is (n C F)^2 block Toeplitz from the lagged
 *   correlations at lags -(F-1) .. F-1, D the correlations of the reference channels with the estimate channels at lags 0 .. F-1, h_one uses
 *   the diagonal (C F)^2 block of source j.  sep_bss_xcorr computes both sets on (B, n C, T) views; the solves are the CALLER's (utils/bss.py).
 *   Frames: row b has nwin_b = max(0, floor((T_b - W + H) / H)) frames, frame w covers samples [w H, w H + W): every frame is full, a trailing
 *   partial window is dropped.  The decomposition is applied to the frame's segment ALONE: r_w, e_w are its W samples, samples outside the frame
 *   count as zero even where the row has audio there, each segment is extended by F - 1 zeros.  For source j, per channel c:
 *     s_true = r_w[j][c],  P_j = sum_{c2} h_one[j][c][c2] * r_w[j][c2],  P_all = sum_{k,c2} h_all[j][c][k][c2] * r_w[k][c2]   (* = convolution)
 *     e_spat = P_j - s_true,  e_interf = P_all - P_j,  e_artif = e_w[j][c] - P_all;
 *   energies are summed over the C channels and the W + F - 1 samples:
 *     SDR = |s_true|^2 / |e_w - s_true|^2, ISR = |s_true|^2 / |e_spat|^2, SIR = |P_j|^2 / |e_interf|^2, SAR = |P_all|^2 / |e_artif|^2,
 *   each 10 log10 of its quotient, +inf for a zero denominator.  A frame is NaN for EVERY source if some reference source, or some estimate, has
 *   a channel sum sum_c x_w[i][c][t] of zero at every sample of the frame (museval's _any_source_silent; a stereo source with L = -R throughout a
 *   frame counts as silent).  A track's score is the NaN-ignoring median over its frames, a corpus' the median over tracks.
 *   sep_bss_image_energies  ref, est (B, n, C, T) fp32 rows of pitch T; filt_all (B, n, C, n C, flen): [b][j][c][k C + c2] = h_all[j][c][k][c2];
 *                           filt_one (B, n, C, C, flen): [b][j][c][c2] = h_one[j][c][c2]; both fp64.  out (B, n, nwin, 9) fp64, per source j and
 *                           frame w: |s_true|^2, |e_w - s_true|^2, |e_spat|^2, |P_j|^2, |e_interf|^2, |P_all|^2, |e_artif|^2, the count of frame
 *                           samples whose reference channel sum is non-zero, the same count for the estimate (both sums formed in fp64).  The
 *                           ratios, the silence rule and the medians are the caller's.  Frames at or beyond nwin_b are written as zeros.
 *   sep_bss_image_scratch_bytes  72 B n nwin ceil((window + flen - 1) / 1024) bytes, 0 for arguments the call would refuse.  Not a launch: no
 *                           stream, no sequence-table entry.  (The two sep_bss_xcorr calls before it need sep_bss_scratch_bytes(B, n C, n C, T, flen).)
 * lengths, scratch, determinism: as the v3 calls -- T_b = lengths[b] clamped to [0, T], NULL means T; samples at and beyond T_b are never read; no
 * atomics, a workgroup owns one slab of 1024 output samples counted from the FRAME's first sample, a second launch adds the slabs in ascending
 * order: two runs give the same bits, and a row gives the same bits whatever the pitch T and the rows around it are.  The projected signals exist in
 * registers only.  All offsets are 64-bit.  B <= 65535, n nwin <= 65535, n C <= 65535, T, flen, window and hop within 2^30. */
size_t sep_bss_image_scratch_bytes(int B, int n, int C, int flen, int window, int nwin);
int sep_bss_image_energies(const float* ref, const float* est, const double* filt_all, const double* filt_one, const int32_t* lengths, double* out,
                           double* scratch, size_t scratch_bytes, int B, int n, int C, int T, int flen, int window, int hop, int nwin,
                           sep_stream_t stream);

/* ---- Mixture invariant training (MixIT, Wisdom et al. 2020; ABI 23, additive; csrc/mixit.hip, criterion/mixit.py) ---------------------------------
 * M estimates est (B, M, T) of the sum of N reference mixtures tgt (B, N, T), fp32 rows of pitch T.  An assignment hands every estimate to exactly
 * one mixture; its code is sum_m n(m) N^(M-1-m) (itertools.product(range(N), repeat=M) order, estimate 0 most significant).  The remix of
 * mixture n is y_n = sum of the estimates with n(m) = n (zero for an empty set), and the measure of (y_n, x_n) is a function of three inner
 * products, each a sum of entries of ONE Gram matrix of the R = M + N rows (estimates first):
 *     tt = G[M+n][M+n],   a = sum_{m in set n} G[M+n][m],   yy = sum_{m, m' in set n} G[m][m'].
 *   kind 0 (SI-SDR)           alpha = a / (tt + eps);  10 log10((alpha^2 tt + eps) / (max(alpha^2 tt - 2 alpha a + yy, 0) + eps))
 *   kind 1 (SDR)              10 log10((tt + eps) / (max(tt - 2 a + yy, 0) + eps))
 *   kind 2 (thresholded SNR)  10 log10((tt + eps) / (max(tt - 2 a + yy, 0) + tau tt + eps))
 * 1 <= M <= 16, 1 <= N <= 8, N^M <= 65536, B <= 65535, T <= 2^30.
 *   sep_mixit_gram           gram (B, R, R) fp64: G[i][j] = sum_t row_i[t] row_j[t], product and sum in fp64 (the product of two fp32 values is
 *                            exact there).  Both triangles are written, bit for bit symmetric; no entry keeps what it held.  ONE pass over the
 *                            rows for R <= 12 (a workgroup owns SEP_MIXIT_SLAB samples of all R rows of an item, a thread holds the R values of a
 *                            sample and forms the R (R + 1) / 2 products); beyond that 8 x 8 blocks of the matrix per workgroup.  No atomics: the
 *                            slab partials go to scratch and a second launch of the same call adds them in ascending order, so two runs give the
 *                            same bits and an item gives the same bits in any batch.
 *   sep_mixit_scratch_bytes  8 B ceil(T / SEP_MIXIT_SLAB) R^2, or 0 for arguments sep_mixit_gram would refuse.  Not a launch.
 *   sep_mixit_search         one workgroup per item strides over the N^M codes, evaluates the measure of every mixture in fp64 from gram, reduces
 *                            over the mixtures by mean (use_mean) or sum and keeps the maximum (maximize) or minimum; the lowest code wins a tie
 *                            (torch.max / torch.min).  best_val (B) fp32, best_idx (B) int64: the code, per_mix (B, N) fp32: the measure of every
 *                            mixture at that code.
 *   sep_mixit_bwd            d_est[b][m][t] = gw[b] (cT_n x_n[t] + cE_n y_n[t]) with n = n(m) under the code best_idx[b], where
 *                            cT_n x_n + cE_n y_n = d measure_n / d y_n.  gw (B) fp32 is the gradient that arrives at EVERY per-mixture measure of
 *                            item b: the caller folds the 1 / N of a mean over the mixtures (and any sign) into it.  One read of the R rows, one
 *                            write of the M rows; every element of d_est is written.  A best_idx outside [0, 65536) is read as code 0. */
#define SEP_MIXIT_SLAB 2048
#define SEP_MIXIT_MAX_EST 16
#define SEP_MIXIT_MAX_MIX 8
#define SEP_MIXIT_MAX_CODES 65536
size_t sep_mixit_scratch_bytes(int B, int M, int N, int T);
int sep_mixit_gram(const float* est, const float* tgt, double* gram, double* scratch, size_t scratch_bytes, int B, int M, int N, int T,
                   sep_stream_t stream);
int sep_mixit_search(const double* gram, int B, int M, int N, int kind, int maximize, int use_mean, double eps, double tau, float* best_val,
                     int64_t* best_idx, float* per_mix, sep_stream_t stream);
int sep_mixit_bwd(const float* est, const float* tgt, const double* gram, const int64_t* best_idx, const float* gw, float* d_est, int B, int M,
                  int N, int T, int kind, double eps, double tau, sep_stream_t stream);

/* ---- Optimal-permutation (Hungarian) training (Dovrat, Nachmani, Wolf 2021; ABI 23, additive; csrc/assign.hip, criterion/hungarian.py) --------------
 * n estimates est (B, n, T) of n targets tgt (B, n, T), fp32 rows of pitch T.  The loss is the best of the n! ways to pair them, found as a linear
 * assignment problem on the n x n matrix of pair measures in O(n^3), not by a table of permutations.  1 <= n <= SEP_ASSIGN_MAX_N = 64 (a column
 * per lane of one wavefront), B <= 65535 for the calls that walk the waveforms, T >= 1.  Anything else is refused with a message before any launch.
 *   sep_pair_gram            dots (B, n, n): dots[b][i][j] = <est_i, tgt_j>, tt (B, n): |tgt_j|^2, xx (B, n): |est_i|^2, all fp64, product and sum
 *                            in fp64 (the product of two fp32 values is exact there): the layout sep_sisdr_dots fills with all_pairs = 1, so
 *                            sep_sisdr_from_dots and sep_sisdr_bwd take them.  The outputs are WRITTEN, not accumulated: no zeroing.  ONE pass: a
 *                            workgroup owns SEP_PAIR_SLAB samples of an 8 x 8 block of (estimate, target) pairs in fp64 registers (4 x 4 for
 *                            n <= 4), so a sample is read ceil(n / 8) times per side -- sep_sisdr_dots reads it n times.  No atomics: per thread in
 *                            ascending time, a wave butterfly, the four waves in order, the slab partials to scratch, a second launch of the same
 *                            call adds them in ascending slab order.  Two runs give the same bits; an item gives the same bits in any batch.
 *   sep_pair_gram_scratch_bytes  8 B ceil(T / SEP_PAIR_SLAB) (n^2 + 2 n), or 0 for arguments sep_pair_gram would refuse.  Not a launch.
 *   sep_assign               cost (B, n, n) fp64 -> perm (B, n) int64: row i is matched to column perm[i]; total (B) fp64: sum_i cost[i][perm[i]]
 *                            added in ascending i; duals (B, 2 n) fp64: row potentials u, then column potentials v.  The exact minimum-cost
 *                            perfect matching, or the maximum-cost one if `maximize`: the costs are then negated on entry (total is the sum of the
 *                            costs as given) and duals are those of the negated, i.e. minimisation, problem: u_i + v_j <= c_ij for every pair
 *                            and sum u + sum v = sum_i c[i][perm[i]] in exact arithmetic -- a certificate of optimality.  Shortest augmenting
 *                            paths with potentials (Jonker-Volgenant, the O(n^3) Hungarian method), one wavefront per item, the matrix in 32 KB
 *                            of LDS, lane j owns column j; the next column is the unused one of least reduced cost by a wave reduction on
 *                            (value, column) pairs, the lowest column among equals.  TIES: any optimal assignment is a correct answer; the call
 *                            returns the same one every time for the same bits, the one this search order reaches -- NOT "the first in
 *                            itertools.permutations order" of sep_pit_search.  NON-FINITE costs: every loop has a trip count fixed by n (n rows,
 *                            at most n + 1 columns per augmentation, at most n steps back along the path) and a column whose value does not
 *                            compare is offered as +inf, the lowest unused column taken if nothing compares: NaN and +-Inf give SOME valid
 *                            permutation and whatever total the arithmetic gives; the call never spins and never indexes out of range.
 *   sep_pair_assign          the same solver on the matrix of pair measures m[i][j] formed in fp64 from (dots[i][j], tt[j], xx[i]) -- in dB, not
 *                            negated; `maximize` picks the sense, the caller maps a negated loss onto it:
 *                              kind 0 (SI-SDR)           alpha = a / (tt + eps);  10 log10((alpha^2 tt + eps) / (max(alpha^2 tt - 2 alpha a + xx, 0) + eps))
 *                              kind 1 (SDR)              10 log10((tt + eps) / (max(tt - 2 a + xx, 0) + eps))
 *                              kind 2 (thresholded SNR)  10 log10((tt + eps) / (max(tt - 2 a + xx, 0) + tau tt + eps))
 *                            best_val (B) fp32: the sum, or the mean if use_mean, of m[i][perm[i]] added in ascending i in fp64; perm (B, n) int64;
 *                            per_src (B, n) fp32: m[i][perm[i]]; duals (B, 2 n) as above, of the matrix the solver saw (-m for a maximum), or null.
 *   sep_pair_bwd             d_est[b][i][t] = gw[b] (cT tgt[b][perm[i]][t] + cE est[b][i][t]) with cT x + cE y = d m / d y of the pair (i, perm[i]).
 *                            gw (B) fp32 is the gradient arriving at EVERY per-source measure of item b (fold the 1 / n of a mean and the sign of
 *                            a loss into it).  Reads two rows and writes one per estimate; every element of d_est is written.  A perm entry
 *                            outside [0, n) is read as 0. */
#define SEP_PAIR_SLAB 2048
#define SEP_ASSIGN_MAX_N 64
size_t sep_pair_gram_scratch_bytes(int B, int n, int T);
int sep_pair_gram(const float* est, const float* tgt, double* dots, double* tt, double* xx, double* scratch, size_t scratch_bytes, int B, int n, int T,
                  sep_stream_t stream);
int sep_assign(const double* cost, int B, int n, int maximize, int64_t* perm, double* total, double* duals, sep_stream_t stream);
int sep_pair_assign(const double* dots, const double* tt, const double* xx, int B, int n, int kind, int maximize, int use_mean, double eps, double tau,
                    float* best_val, int64_t* perm, float* per_src, double* duals, sep_stream_t stream);
int sep_pair_bwd(const float* est, const float* tgt, const double* dots, const double* tt, const double* xx, const int64_t* perm, const float* gw,
                 float* d_est, int B, int n, int T, int kind, double eps, double tau, sep_stream_t stream);

/* ---- Stitching the windows of a long recording (continuous speech separation; ABI 23, additive; csrc/stitch.hip, sepkernels/longform.py) ----------
 * A recording is separated window by window: est (B, W, n, win) fp32, contiguous, holds the n outputs of W windows of `win` samples at stride
 * `hop` (window w covers samples [w hop, w hop + win) of the recording).  Neighbours share O = win - hop samples.  The outputs of a window come in
 * an order of their own; the calls below find the order of every window relative to the first and join the windows into n tracks.
 * 1 <= n <= SEP_ASSIGN_MAX_N, B >= 1, W >= 1, win / 2 <= hop < win (a sample lies in at most two windows), win <= 2^30.  Anything else is refused
 * with a message before any launch.  All offsets are 64-bit.
 *   sep_stitch_cost    cost (B, W - 1, n, n) fp64: cost[b][w][i][j] = sum_{t < O} (est[b][w][i][hop + t] - est[b][w + 1][j][t])^2, difference, square
 *                      and sum in fp64: the layout sep_assign takes as B (W - 1) matrices (maximize = 0).  WRITTEN, not accumulated.  One
 *                      workgroup per (boundary, 8 x 8 tile of pairs; 4 x 4 for n <= 4) walks the whole overlap with the tile in fp64 registers:
 *                      no scratch, no second launch, no atomics -- per thread in ascending time, a wave butterfly, the four waves in order, so
 *                      two runs give the same bits and identical rows cost exactly 0.  16-byte loads when win and hop are multiples of 4 and est
 *                      is 16-byte aligned, sample by sample otherwise.  B (W - 1) < 2^31.  W = 1 launches nothing (cost may be null).
 *   sep_stitch_chain   perm_local (B, W - 1, n) int64 as sep_assign writes it for those matrices (row i of window w is matched to row
 *                      perm_local[b][w][i] of window w + 1) -> perm_abs (B, W, n) int64, the row of every window that continues track s:
 *                      perm_abs[b][0][s] = s, perm_abs[b][w + 1][s] = perm_local[b][w][perm_abs[b][w][s]].  Sequential in w: one wavefront per
 *                      recording, lane s, perm_local staged through LDS 64 windows at a time.  An entry of perm_local outside [0, n) is read as
 *                      0 (sep_pair_bwd's convention): nothing is indexed out of range, every entry of perm_abs lies in [0, n).  W = 1 writes
 *                      the identity (perm_local may be null).
 *   sep_stitch_ola     out (B, n, T) fp32, 1 <= T <= (W - 1) hop + win, B <= 65535.  For sample t: w = min(t / hop, W - 1), k = t - w hop,
 *                      c = est[b][w][perm_abs[b][w][s]][k].  If w >= 1 and k < O the sample lies in the overlap with the window before and
 *                      out[b][s][t] = a + g (c - a) with a = est[b][w - 1][perm_abs[b][w - 1][s]][hop + k], g = (k + 0.5f) / O, all in fp32: a
 *                      linear cross-fade whose weights add to one, so no normaliser.  Otherwise out[b][s][t] = c, a copy bit for bit.  Every
 *                      element is written, each once, by the thread that owns it: no atomics.  An entry of perm_abs outside [0, n) is read as 0.
 *                      16-byte loads and stores when win, hop and T are multiples of 4 and est, out are 16-byte aligned. */
int sep_stitch_cost(const float* est, double* cost, int B, int W, int n, int win, int hop, sep_stream_t stream);
int sep_stitch_chain(const int64_t* perm_local, int64_t* perm_abs, int B, int W, int n, sep_stream_t stream);
int sep_stitch_ola(const float* est, const int64_t* perm_abs, float* out, int B, int W, int n, int win, int hop, int T, sep_stream_t stream);

/* ---- Sample-rate conversion: whole signals and online streams (ABI 23, additive; csrc/resample.hip, sepkernels/resample.py) ----------------------
 * The definition is torchaudio.functional.resample, restated here in full because that package is on none of our machines.  With
 * g = gcd(orig_freq, new_freq), o = orig_freq / g, u = new_freq / g, lpw = lowpass_filter_width (6) and rolloff (0.99):
 *     base  = min(o, u) rolloff,   width = ceil(lpw o / base),   K = 2 width + o
 *     t[p][k] = clamp(((k - width) / o - p / u) base, -lpw, lpw)                          p in [0, u), k in [0, K)
 *     h[p][k] = sinc(pi t) w(t) base / o,   sinc(0) = 1,   w(t) = cos(pi t / (2 lpw))^2                       ("sinc_interp_hann")
 *                                           or             w(t) = i0(beta sqrt(1 - (t / lpw)^2)) / i0(beta)   ("sinc_interp_kaiser", beta 14.769656459379492)
 *     y[i u + p] = sum_k h[p][k] x[i o + k - width],   x = 0 outside [0, T),   T_out = ceil(u T / o)
 * everything formed in fp64 and then cast.  The table is the CALLER's (sepkernels/resample.py builds it on the host), and it is handed over
 * COMPACT: of every phase the Kc taps from first[p] on, table[j u + p] = (float)h[p][first[p] + j], j < Kc (tap-major: consecutive phases are
 * consecutive words), 0 <= first[p] <= K - Kc, so that every tap left out is negligible (the module drops leading and trailing taps below
 * 2^-60 of the phase's largest; Kc is the longest run that leaves, 67 of K = 509 at 44.1 k -> 8 k).  table and first (u int32) are device memory;
 * the library cannot look at them: an entry of first outside [0, K - Kc] is read as the nearest end of that range, nothing is indexed out of range.
 *   sep_resample_fwd         x: R rows of T fp32 samples at pitch x_pitch >= T; y: R rows of T_out at pitch y_pitch >= T_out (pitches in elements).
 *                            y[r][i u + p] = sum_{j < Kc} table[j u + p] x[r][i o + first[p] + j - width], added by fmaf in ascending j from +0
 *                            in fp32 -- the same sequence for every output of a phase wherever it lies in the row.  Nothing outside [0, T) of a
 *                            row is read (the zeros are a predicate), elements [T_out, y_pitch) are not written, every element below T_out is
 *                            written once by the thread that owns it: no atomics, two runs give the same bits.  A workgroup stages the input
 *                            span of a tile of frames in LDS beside the table.  Instances (sep_last_kernel): "resample_frames<U>" for
 *                            u = U <= 3 (a thread per frame, the tap of a step wave-uniform) and "resample_phases" for any u (a thread per
 *                            output, lanes on consecutive phases).  All offsets are 64-bit.
 *   sep_resample_stream_fwd  A rows of an online call.  chunk (A, m o), y (A, m u), history (num_streams, H) with D = ceil(width / o) o and
 *                            H = width + D.  Row j belongs to stream slots[j] (device memory of A distinct entries in [0, num_streams), the
 *                            convention of sep_online_*_sel: read when the kernel runs, not checked; NULL means row j is stream j and
 *                            A = num_streams); rows of history that slots does not name are neither read nor written.  With
 *                            cat = [history of the slot | row j of chunk]: y[j][i u + p] = sum_{j' < Kc} table[j' u + p] cat[i o + first[p] + j'],
 *                            the arithmetic of sep_resample_fwd, tap for tap -- so a stream that starts from a zero history computes
 *                            sep_resample_fwd of [D zeros | its samples] bit for bit however it is cut into chunks, frame by frame as the samples
 *                            arrive (delay: D input samples), and m = D / o frames of zero samples flush the rest.  The history then becomes the
 *                            last H samples of cat, also when the chunk is shorter than H.  RACE-FREE BY OWNERSHIP, no second buffer: one
 *                            workgroup per (row, tile of frames); the history row is read and written by the workgroup of the row's tile 0
 *                            alone, which reads its input span and the H samples of the new history before a barrier and writes after it; a
 *                            geometry in which a later tile would reach back into the history is refused.  Instances "resample_stream_frames<U>",
 *                            "resample_stream_phases".
 * Refused with a message before any launch: a null pointer, T_out != ceil(u T / o), a pitch shorter than its row, Kc > K, K > 8192 (the staged
 * span), u > 1024, Kc u > 6144 (the table's LDS), H > SEP_RESAMPLE_MAX_HISTORY, more than 2^31 - 1 tiles.  The module then takes its composed route. */
#define SEP_RESAMPLE_MAX_HISTORY 2048
int sep_resample_fwd(const float* x, int64_t x_pitch, const float* table, const int32_t* first, float* y, int64_t y_pitch, int R, int64_t T,
                     int64_t T_out, int o, int u, int width, int Kc, sep_stream_t stream);
int sep_resample_stream_fwd(const float* chunk, const float* table, const int32_t* first, float* history, float* y, const int32_t* slots, int A,
                            int num_streams, int m, int o, int u, int width, int Kc, sep_stream_t stream);

/* ---- Dynamic mixing from a device-resident corpus (ABI 23, additive; csrc/mixing.hip, sepkernels/mixing.py) --------------------------------------
 * A training batch of fresh mixtures per step -- new speakers, utterances, crops and gains every time -- drawn and rendered on the device from a
 * corpus that lives there (the whole wsj0 si_tr_s set is about 1.7 GB as int16).  The reference mixes on the fly only for music
 * (egs/musdb18/<model>/local/train.py with src/utils/augmentation.py) and in its tutorials (egs/tutorials/common/src/dataset.py:44).
 * The corpus (the CALLER's; sepkernels/mixing.py::DeviceCorpus builds it):
 *     samples    ONE flat tensor of all utterances, int16 (SEP_MIX_INT16, a sample is pcm 2^-15) or fp32 (SEP_MIX_F32); at least SEP_MIX_GUARD zero
 *                elements in front of the first utterance and behind the last, so that whole aligned 16-byte words may be loaded
 *     offsets    int64, U + 1 entries: utterance u is samples[offsets[u] : offsets[u + 1]], 1 <= its length < 2^31; offsets[0] is the guard length
 *     spk_first  int32, S + 1 entries: utterances are sorted by speaker, speaker s owns utterances [spk_first[s], spk_first[s + 1]), at least one
 *     level      fp32, U entries: ref_rms / rms_u (plain RMS over the whole utterance in fp64 on the host, NOT the ITU active level of wsj0-mix's Matlab
 *                scripts; 0 for a silent utterance, 1 everywhere without normalisation)
 * THE DRAW.  Counter-based, no generator state, all in wrapping uint64:
 *     mix64(z):  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9;  z = (z ^ (z >> 27)) * 0x94D049BB133111EB;  return z ^ (z >> 31)
 *     word(seed, item, k) = mix64(mix64(seed + 0x9E3779B97F4A7C15 * (item + 1)) + k)
 *     below(w, m) = ((w >> 32) * m) >> 32                                   1 <= m < 2^31
 *     item = step * item_stride + item_first + b                            (item_stride = the global batch, item_first = rank * B)
 * For item b and source i < n, with `chosen` the ascending list of the speakers already taken:
 *     speaker     r = below(word(.., i), S - i); for c in chosen, ascending: if r >= c then r += 1; s_i = r, and r is inserted into chosen -- the sources
 *                 of a mixture have distinct speakers, drawn uniformly without replacement; every loop is bounded by n
 *     utterance   u = spk_first[s] + below(word(.., n + i), spk_first[s + 1] - spk_first[s])
 *     position    len = offsets[u + 1] - offsets[u], w = word(.., 2 n + i): if len >= T then start = below(w, len - T + 1), lead = 0; else start = 0,
 *                 lead = below(w, T - len + 1) -- a short utterance is placed at a random offset inside the segment, zeros around it
 *     gain index  g = below(word(.., 3 n + i), G);   gain[b][i] = level[u] * gain_table[g], ONE fp32 multiply
 *     noise row   (with a noise index, the WHAM recipes' third signal; no speaker structure) u = below(word(.., 4 n), U_noise), the position from draw
 *                 4 n + 1, the gain index from draw 4 n + 2 into noise_gain_table of G_noise entries, gain = noise_level[u] * noise_gain_table[g]
 * gain_table[j] = (float)10^((lo + (hi - lo) j / (G - 1)) / 20) is built by the host in fp64: nothing transcendental is evaluated on the device, so the
 * draw is bit-exact against a restatement in Python integers.  Known answers:
 *     word(1234, 0, 0) = 0x2851ddd6c202938b   word(1234, 0, 1) = 0xf344a9a461c929aa   word(1234, 1, 0) = 0xc4c7e6b923620b24
 *     word(1234, 1, 1) = 0x22531db8ef59e66f   word(0, 0, 0) = 0x48218226ff3cd4bf      word(2^63, 2^40 + 3, 31) = 0x568966ec49cd65d1
 *   sep_mix_draw    writes plan int64 (B, R, 4) = {utterance, start, lead, gain index} and gain fp32 (B, R); R = n without a noise index (noise_offsets
 *                   NULL, U_noise 0), n + 1 with one.  `seed` is read as unsigned.  The step lives in device memory: counter[0] is the step of this call
 *                   and the kernel leaves counter[0] + 1, so a recorded call replays into the NEXT batch (as sep_adam_step_dev does with its step
 *                   count).  One workgroup whose threads loop over the items; every thread reads the counter, then a barrier, then one thread stores
 *                   the increment: no atomics.  The index is device memory the library cannot look at: a speaker's count below 1 is read as 1, an
 *                   utterance outside [0, U) as the nearest end, a length outside [1, 2^31) likewise.
 *   sep_mix_render  writes sources (B, n, T), mixture (B, 1, T) and, if `noise` is not NULL (then the plan has n + 1 rows and noise_samples,
 *                   noise_offsets come with it), the noise row (B, 1, T) from a plan:
 *                       src[b][i][t] = gain[b][i] * ((float)pcm[offsets[u] + start + t - lead] * scale)   where lead <= t and t - lead < len - start,
 *                                      +0.0f elsewhere;   scale = 2^-15 for int16 (that product is exact), 1 for fp32: one rounding per sample
 *                       mixture[b][0][t] = ((src_0 + src_1) + src_2) + ... in ascending i in fp32, the noise row added last
 *                   Every element is written once by the thread that owns it: no atomics, two runs give the same bits.  The plan is device memory the
 *                   library cannot look at: u is clamped into [0, U), start into [0, len - 1], and the predicate keeps every read inside the utterance
 *                   whatever lead holds, so no plan can index outside the storage.  Instances (sep_last_kernel): "mix_render_vec<int16,8>" and
 *                   "mix_render_vec<float,4>" when T % 4 == 0 and the outputs are 16-byte aligned (a thread owns 8 or 4 consecutive samples of every
 *                   row, 16-byte stores; for int16 aligned 16-byte loads selected by the row's misalignment, which is uniform per (item, source) -- the
 *                   guard zeros are there for this), "mix_render_scalar<int16>" and "mix_render_scalar<float>" for everything else.  All offsets are 64-bit.
 * Refused with a message before any launch: a null pointer, n outside [1, SEP_MIX_MAX_SOURCES], n > S, S > U, B outside [1, 65535], T < 1, G < 1, an
 * unknown sample kind, a noise index without its levels and table (draw), a noise row without its samples and index or the other way round (render). */
#define SEP_MIX_MAX_SOURCES 8
#define SEP_MIX_GUARD 16
#define SEP_MIX_INT16 0
#define SEP_MIX_F32 1
int sep_mix_draw(const int64_t* offsets, const int32_t* spk_first, int U, int S, const int64_t* noise_offsets, int U_noise, const float* level,
                 const float* gain_table, int G, const float* noise_level, const float* noise_gain_table, int G_noise, int64_t* counter, int64_t seed,
                 int64_t item_stride, int64_t item_first, int B, int n, int T, int64_t* plan, float* gain, sep_stream_t stream);
int sep_mix_render(const void* samples, int kind, const int64_t* offsets, int U, const void* noise_samples, const int64_t* noise_offsets, int U_noise,
                   const int64_t* plan, const float* gain, int B, int n, int T, float* sources, float* mixture, float* noise, sep_stream_t stream);

/* ---- Speed perturbation in dynamic mixing (ABI 23, additive; csrc/mixing.hip, sepkernels/mixing.py) ----------------------------------------------
 * Every source of a drawn mixture is resampled by a few percent before it is cropped, scaled and summed, so that tempo and pitch move together
 * (sox `speed`).  sep_mix_draw and sep_mix_render are unchanged; the two entry points below are their twins.
 * SPEEDS.  A list of J distinct integer percentages P_j, 1 <= J <= SEP_MIX_MAX_SPEEDS, SEP_MIX_SPEED_MIN <= P_j <= SEP_MIX_SPEED_MAX.  For a speed P:
 * g = gcd(P, 100), o = P / g, u = 100 / g, and the filter is the resampler's (above: orig_freq = P, new_freq = 100, lowpass_filter_width 6, rolloff
 * 0.99, sinc_interp_hann) in its compact form: fp32 table[k][p] (Kc rows of u, tap-major), first[p], Kc, width.  Over the whole range width <= 13,
 * Kc <= 25 <= SEP_MIX_SPEED_MAX_TAPS and Kc u <= 2500 (25 taps of 100 phases at P = 199; Kc u <= 1300 for P < 100).  P = 100 is the identity:
 * o = u = 1, no filter, exactly the copy formula of sep_mix_render.
 * CONVENTION.  The perturbed utterance is the utterance resampled from rate P to rate 100: len' = ceil(u len / o) samples, a tone of frequency f comes
 * out at f P / 100 -- P > 100 is shorter and higher.  (A 1 kHz tone at 8 kHz: 949.2 Hz at P = 95, 1050.8 Hz at P = 105, RMS ratios 0.99998 and 1.0005.)
 * The level is NOT renormalised after the perturbation: gain = level[u] * gain_table[g] as in sep_mix_draw.
 * A PERTURBED SAMPLE.  x is the raw sample (the int16 integer, or the fp32 value), zero outside [0, len) of its OWN utterance, never a neighbour's
 * sample.  With m = i u + p:
 *     acc  = sum over k < Kc, ascending, from +0.0, in fp64, of (double)table[k][p] * (double)x[i o + first[p] + k - width]
 *     v[m] = (float)acc
 * Every product is exact in fp64 (24 x 16 or 24 x 24 bits), so a fused and an unfused multiply-add give the same bits: device, numpy and the host
 * simulation agree bit for bit.
 * A ROW.  src[b][i][t] = gain * (v[start + t - lead] * scale) where lead <= t and t - lead < len' - start, +0.0f elsewhere; scale as in sep_mix_render.
 * The mixture is summed in ascending order, the noise row added last.
 * THE DRAW.  Speaker, utterance and gain index as in sep_mix_draw.  The speed index of source i is j = below(word(.., 4 n + 3 + i), J) -- draws
 * 0 .. 4 n + 2 are taken, so nothing existing moves -- and the position is drawn from len' in place of len (formed in int64, clamped into [1, 2^31)),
 * with draw 2 n + i as before.  The noise row is never perturbed.  Known answers:
 *     word(1234, 0, 11) = 0x718ad7f33aef0177 (below 3: 1)   word(1234, 0, 12) = 0x0de521a7eba82090 (0)   word(1234, 1, 11) = 0x5f314ef19e801a70 (1)
 *     word(0, 0, 7) = 0x915f11bbbfb2963d (1)                word(2^63, 2^40 + 3, 42) = 0xd90fbd8340eb6aa8 (2)
 * DESCRIPTORS.  desc is int32 (J, SEP_MIX_SPEED_DESC) in device memory: {o, u, width, Kc, offset of table[0][0] in filter_table (floats), offset of
 * first[0] in filter_first (entries), P, 0}; an identity speed is {1, 1, 0, 1, 0, 0, 100, 0}.  filter_table (table_numel floats) and filter_first
 * (first_numel int32) hold the speeds' tables and `first` one behind the other.
 *   sep_mix_draw_speed    sep_mix_draw plus desc, J and the output speed int32 (B, R): j per source, -1 for the noise row.  The plan stays (B, R, 4), the
 *                         counter protocol is sep_mix_draw's.  With one identity speed the plan and the gains are sep_mix_draw's.
 *   sep_mix_render_speed  sep_mix_render plus speed, desc, J and the filter buffers with their sizes.  One workgroup owns a tile of 2048 (int16) or 1024
 *                         (fp32) output samples of one item and loops over its rows; for a perturbed row it stages the row's filter and the input span of
 *                         the tile in LDS (aligned 16-byte loads, a word only where it holds a sample of the utterance), sums the taps in fp64, and
 *                         accumulates the mixture in registers across rows.  Copy rows (j = -1, o == u) take sep_mix_render's formula in the same kernel.
 *                         Every element is written once, no atomics, two runs give the same bits.  Instances: "mix_render_speed<int16>" and
 *                         "mix_render_speed<float>" (T % 4 == 0, outputs 16-byte aligned: 16-byte stores), "mix_render_speed_scalar<int16>" and
 *                         "mix_render_speed_scalar<float>" otherwise.
 * The plan, speed and desc are device memory the library cannot look at.  Whatever they hold: the utterance is clamped into [0, U), j into [-1, J)
 * (below -1 reads as -1), start into [0, len' - 1], o into [1, SEP_MIX_SPEED_MAX], u into [1, 100], width into [0, SEP_MIX_SPEED_MAX_TAPS], Kc into
 * [1, SEP_MIX_SPEED_MAX_TAPS], every index into filter_table and filter_first into [0, table_numel) and [0, first_numel), every first[p] and every LDS index
 * into the allocation; corpus reads stay inside the utterance and writes inside the outputs.
 * Refused with a message before any launch: what the plain calls refuse, a null pointer, J outside [1, SEP_MIX_MAX_SPEEDS], table_numel outside
 * [1, SEP_MIX_MAX_SPEEDS * SEP_MIX_SPEED_MAX_TAPS * 100], first_numel outside [1, SEP_MIX_MAX_SPEEDS * 100], samples not aligned to their own size.
 * Not offered: perturbing the noise row, non-integer percentages, renormalising the level after the perturbation. */
#define SEP_MIX_MAX_SPEEDS 16
#define SEP_MIX_SPEED_MIN 50
#define SEP_MIX_SPEED_MAX 200
#define SEP_MIX_SPEED_MAX_TAPS 32
#define SEP_MIX_SPEED_DESC 8
int sep_mix_draw_speed(const int64_t* offsets, const int32_t* spk_first, int U, int S, const int64_t* noise_offsets, int U_noise, const float* level,
                       const float* gain_table, int G, const float* noise_level, const float* noise_gain_table, int G_noise, int64_t* counter, int64_t seed,
                       int64_t item_stride, int64_t item_first, int B, int n, int T, const int32_t* desc, int J, int64_t* plan, float* gain, int32_t* speed,
                       sep_stream_t stream);
int sep_mix_render_speed(const void* samples, int kind, const int64_t* offsets, int U, const void* noise_samples, const int64_t* noise_offsets, int U_noise,
                         const int64_t* plan, const float* gain, const int32_t* speed, const int32_t* desc, int J, const float* filter_table, int64_t table_numel,
                         const int32_t* filter_first, int64_t first_numel, int B, int n, int T, float* sources, float* mixture, float* noise, sep_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
