// The learned filterbank of the Conv-TasNet path for gfx950 (HBM-bound streaming kernels): the encoder with the gLN statistics of its
// output, the unfold behind the encoder's weight gradient, the decoder with mask and overlap-add, and the decoder's backward.  All
// tensors (batch, channel, frame) fp32 with padded row stride ldt; frames [T, ldt) of every written tensor are zero.
//
// Reference arithmetic replaced (reference src/): models/filterbank.py:205-251 (Encoder/Decoder), models/conv_tasnet.py:145-169
// (pad, mask*w, crop).
#include "common.hpp"

namespace {

// =====================================================================================
// Encoder: w[b][n][f] = sum_{c,k} E[n][c][k] * xpad[b][c][S f + k]   (+ReLU), + gLN statistics of w
// One block = 128 frames x all N basis rows.  Thread = (frame, n parity); the basis row is wave-uniform
// (scalar loads), the frame's samples sit in registers (LC = Cin*L <= 16) or LDS (generic).
// =====================================================================================
constexpr int ENC_FT = 128;

template <int LC_REG>
__global__ __launch_bounds__(256) void encoder_fwd_kernel(const float* __restrict__ x, const float* __restrict__ E,
                                                          float* __restrict__ w, double* __restrict__ stats, int B,
                                                          int Cin, int Tin, int N, int L, int S, int F, int ldt,
                                                          int pad_left, int relu) {
    extern __shared__ __attribute__((aligned(16))) float xs[];   // [Cin][span]
    __shared__ double red[4];
    const int tid = threadIdx.x;
    const int b = blockIdx.y;
    const int f0 = blockIdx.x * ENC_FT;
    const int span = ENC_FT * S + L - S;
    for (int i = tid; i < Cin * span; i += 256) {
        const int c = i / span, o = i % span;
        const int tau = S * f0 + o - pad_left;
        xs[i] = (tau >= 0 && tau < Tin) ? x[((size_t)b * Cin + c) * Tin + tau] : 0.f;
    }
    __syncthreads();
    const int fl = tid & (ENC_FT - 1);
    const int f = f0 + fl;
    const int nh = __builtin_amdgcn_readfirstlane(tid >> 7);   // wave-uniform
    const bool fvalid = f < F;
    const int LC = Cin * L;
    float xr[LC_REG > 0 ? LC_REG : 1];
    if (LC_REG > 0) {
#pragma unroll
        for (int q = 0; q < LC_REG; ++q) {
            const int c = q / L, k = q % L;
            xr[q] = xs[c * span + S * fl + k];
        }
    }
    float s = 0.f, ss = 0.f;
    for (int n = nh; n < N; n += 2) {
        const float* En = E + (size_t)n * LC;
        float acc = 0.f;
        if (LC_REG > 0) {
#pragma unroll
            for (int q = 0; q < LC_REG; ++q) acc = fmaf(En[q], xr[q], acc);
        } else {
            for (int c = 0; c < Cin; ++c)
                for (int k = 0; k < L; ++k) acc = fmaf(En[c * L + k], xs[c * span + S * fl + k], acc);
        }
        if (relu) acc = fmaxf(acc, 0.f);
        if (!fvalid) acc = 0.f;
        s += acc; ss += acc * acc;
        if (f < ldt) w[((size_t)b * N + n) * ldt + f] = acc;
    }
    const double ds = block_sum_256<double>((double)s, red);
    const double dss = block_sum_256<double>((double)ss, red);
    if (tid == 0) { double* st = stats + ((size_t)b * SEP_STATS_SLOTS + (blockIdx.x & (SEP_STATS_SLOTS - 1))) * 2; atomicAdd(st, ds); atomicAdd(st + 1, dss); }
}

// Mono 16-tap / stride-8 encoder (the paper-best front end): a lane owns FOUR consecutive frames (40 input samples in registers),
// so every store of w is a float4 -- 1 KiB per wave instruction instead of 256 B (the dword-per-lane form is store-issue bound:
// 81 us for 131 MB).  One workgroup = 256 frames of one sample; its four waves take the basis rows n = wave (mod 4).
__global__ __launch_bounds__(256) void encoder_fwd_l16s8_kernel(const float* __restrict__ x, const float* __restrict__ E, float* __restrict__ w,
                                                                double* __restrict__ stats, int Tin, int N, int F, int ldt, int pad_left, int relu) {
    __shared__ double red[4];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int b = blockIdx.y;
    const int f = blockIdx.x * 256 + 4 * lane;            // first of this lane's four frames
    float xr[40];
#pragma unroll
    for (int i = 0; i < 40; ++i) {
        const int tau = 8 * f + i - pad_left;
        xr[i] = (tau >= 0 && tau < Tin) ? x[(size_t)b * Tin + tau] : 0.f;
    }
    float s = 0.f, ss = 0.f;
    if (f < ldt) {
        for (int n = wv; n < N; n += 4) {
            const float* En = E + (size_t)n * 16;         // wave-uniform: scalar loads
            float o[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                float acc = 0.f;
#pragma unroll
                for (int k = 0; k < 16; ++k) acc = fmaf(En[k], xr[8 * j + k], acc);
                if (relu) acc = fmaxf(acc, 0.f);
                if (f + j >= F) acc = 0.f;
                s += acc; ss = fmaf(acc, acc, ss);
                o[j] = acc;
            }
            st4(w + ((size_t)b * N + n) * ldt + f, make_float4(o[0], o[1], o[2], o[3]));
        }
    }
    const double ds = block_sum_256<double>((double)s, red);
    const double dss = block_sum_256<double>((double)ss, red);
    if (threadIdx.x == 0) { double* st = stats + ((size_t)b * SEP_STATS_SLOTS + (blockIdx.x & (SEP_STATS_SLOTS - 1))) * 2; atomicAdd(st, ds); atomicAdd(st + 1, dss); }
}

// frames[bp][c*L+k][f] = xpad[bp][c][S f + k] (f < F), 0 for F <= f < ldt
__global__ __launch_bounds__(256) void unfold_kernel(const float* __restrict__ x, float* __restrict__ frames, int C,
                                                     int Tin, int L, int S, int F, int ldt, int pad_left) {
    const int f = blockIdx.x * 256 + threadIdx.x;
    const int row = blockIdx.y;           // c*L + k
    const int bp = blockIdx.z;
    if (f >= ldt) return;
    const int c = row / L, k = row % L;
    const int tau = S * f + k - pad_left;
    float v = 0.f;
    if (f < F && tau >= 0 && tau < Tin) v = x[((size_t)bp * C + c) * Tin + tau];
    frames[((size_t)bp * C * L + row) * ldt + f] = v;
}

// =====================================================================================
// Decoder forward: mask*w, basis synthesis, overlap-add, crop.  Thread = frame; loop over basis rows n
// with the decoder row D[n][:] wave-uniform.  LC = Cout*L; frames exchanged through LDS for the OLA.
// Block covers FB = 256-(R-1) output frames, computing R-1 halo frames redundantly (R = L/S).
// =====================================================================================
template <int LC_REG>
__global__ __launch_bounds__(256) void decoder_fwd_kernel(const float* __restrict__ w, const float* __restrict__ m,
                                                          const float* __restrict__ D, float* __restrict__ est,
                                                          float* __restrict__ latent, int n_src, int N, int Cout, int L,
                                                          int S, int F, int ldt, int Tout, int pad_left) {
    extern __shared__ __attribute__((aligned(16))) float ys[];     // [256][LC+1]
    const int LC = Cout * L;
    const int R = L / S;
    // LC_REG > 0: a workgroup owns 64-(R-1) frames and its four waves split the basis rows (2080 workgroups at paper-best;
    // the 256-frame mapping gave 544 = two per CU, each thread a serial loop of 512 dependent load pairs: 1.6 TB/s)
    const int FW = LC_REG > 0 ? 64 : 256;
    const int FB = FW - (R - 1);
    const int bs = blockIdx.y;            // b*n_src + s
    const int b = bs / n_src;
    const int f0 = blockIdx.x * FB;
    const int i = LC_REG > 0 ? (int)(threadIdx.x & 63) : (int)threadIdx.x;
    const int wv = threadIdx.x >> 6;
    const int f = f0 - (R - 1) + i;
    const bool fvalid = f >= 0 && f < F;
    const bool owner = i >= R - 1 && f < ldt;       // this block owns latent[f]
    const float* wrow = w + (size_t)b * N * ldt;
    const float* mrow = m + (size_t)bs * N * ldt;
    float* lrow = latent ? latent + (size_t)bs * N * ldt : nullptr;
    const int fc = fvalid ? f : 0;

    if (LC_REG > 0) {
        float acc[LC_REG > 0 ? LC_REG : 1];
#pragma unroll
        for (int q = 0; q < LC_REG; ++q) acc[q] = 0.f;
        const int nper = (N + 3) / 4;
        const int n_lo = wv * nper, n_hi = n_lo + nper < N ? n_lo + nper : N;
        for (int n = n_lo; n < n_hi; ++n) {
            float wh = wrow[(size_t)n * ldt + fc] * mrow[(size_t)n * ldt + fc];
            if (!fvalid) wh = 0.f;
            if (lrow && owner) lrow[(size_t)n * ldt + f] = wh;
            const float* Dn = D + (size_t)n * LC;
#pragma unroll
            for (int q = 0; q < LC_REG; ++q) acc[q] = fmaf(wh, Dn[q], acc[q]);
        }
#pragma unroll
        for (int q = 0; q < LC_REG; ++q) ys[(wv * 64 + i) * (LC + 1) + q] = acc[q];
    } else {
        for (int q0 = 0; q0 < LC; q0 += 16) {
            float acc[16];
#pragma unroll
            for (int q = 0; q < 16; ++q) acc[q] = 0.f;
            for (int n = 0; n < N; ++n) {
                float wh = wrow[(size_t)n * ldt + fc] * mrow[(size_t)n * ldt + fc];
                if (!fvalid) wh = 0.f;
                if (q0 == 0 && lrow && owner) lrow[(size_t)n * ldt + f] = wh;
                const float* Dn = D + (size_t)n * LC + q0;
#pragma unroll
                for (int q = 0; q < 16; ++q)
                    if (q0 + q < LC) acc[q] = fmaf(wh, Dn[q], acc[q]);
            }
#pragma unroll
            for (int q = 0; q < 16; ++q)
                if (q0 + q < LC) ys[i * (LC + 1) + q0 + q] = acc[q];
        }
    }
    __syncthreads();
    // overlap-add: padded sample tp = S*fo + k0 gets frames fo - r at tap k0 + r*S
    const int nsamp = FB * S;
    for (int j = threadIdx.x; j < nsamp * Cout; j += 256) {
        const int c = j / nsamp, o = j % nsamp;
        const int fo = o / S, k0 = o % S;            // frame offset inside the block's owned range
        const int tau = S * (f0 + fo) + k0 - pad_left;
        if (tau < 0 || tau >= Tout) continue;
        float v = 0.f;
        for (int r = 0; r < R; ++r) {
            const int cell = (fo + (R - 1) - r) * (LC + 1) + c * L + k0 + r * S;
            if (LC_REG > 0) v += (ys[cell] + ys[64 * (LC + 1) + cell]) + (ys[128 * (LC + 1) + cell] + ys[192 * (LC + 1) + cell]);
            else v += ys[cell];
        }
        est[((size_t)bs * Cout + c) * Tout + tau] = v;
    }
}

// Decoder + mask backward.  Thread = frame, every source handled by the same thread so that dwm = sum_s dlatent*m needs
// no atomics.  raw_mask = 0: dpre = d(sigmoid pre-activation); 1: dpre = d(mask) (softmax masks: sep_softmax_ch_bwd follows).
template <int LC_REG, int NS_REG>
__global__ __launch_bounds__(256) void decoder_bwd_kernel(const float* __restrict__ d_est, const float* __restrict__ w,
                                                          const float* __restrict__ m, const float* __restrict__ D,
                                                          float* __restrict__ dpre, float* __restrict__ dwm, int n_src,
                                                          int N, int Cout, int L, int S, int F, int ldt, int Tout,
                                                          int pad_left, int raw_mask) {
    const int LC = Cout * L;
    const int b = blockIdx.y;
    const int f = blockIdx.x * 256 + threadIdx.x;
    if (f >= ldt) return;
    const bool fvalid = f < F;
    const float* wrow = w + (size_t)b * N * ldt;
    float* dwrow = dwm + (size_t)b * N * ldt;
    // basis rows are independent here: blockIdx.z splits them so that the grid fills the chip (16 x B blocks do not)
    const int nper = (N + (int)gridDim.z - 1) / (int)gridDim.z;
    const int n_lo = (int)blockIdx.z * nper;
    const int n_hi = n_lo + nper < N ? n_lo + nper : N;

    auto dsample = [&](int s, int q) -> float {
        const int c = q / L, k = q % L;
        const int tau = S * f + k - pad_left;
        return (fvalid && tau >= 0 && tau < Tout) ? d_est[(((size_t)b * n_src + s) * Cout + c) * Tout + tau] : 0.f;
    };

    if (LC_REG > 0 && NS_REG > 0) {
        float ds[(NS_REG > 0 ? NS_REG : 1)][(LC_REG > 0 ? LC_REG : 1)];
#pragma unroll
        for (int s = 0; s < NS_REG; ++s)
#pragma unroll
            for (int q = 0; q < LC_REG; ++q) ds[s][q] = (s < n_src) ? dsample(s, q) : 0.f;
        for (int n = n_lo; n < n_hi; ++n) {
            const float wv = wrow[(size_t)n * ldt + f];
            const float* Dn = D + (size_t)n * LC;
            float dacc = 0.f;
#pragma unroll
            for (int s = 0; s < NS_REG; ++s) {
                if (s < n_src) {
                    const size_t off = ((size_t)(b * n_src + s) * N + n) * ldt + f;
                    const float mv = m[off];
                    float dl = 0.f;
#pragma unroll
                    for (int q = 0; q < LC_REG; ++q) dl = fmaf(ds[s][q], Dn[q], dl);
                    dpre[off] = fvalid ? (raw_mask ? dl * wv : dl * wv * mv * (1.f - mv)) : 0.f;
                    dacc += dl * mv;
                }
            }
            dwrow[(size_t)n * ldt + f] = fvalid ? dacc : 0.f;
        }
    } else {
        for (int n = n_lo; n < n_hi; ++n) {
            const float wv = wrow[(size_t)n * ldt + f];
            const float* Dn = D + (size_t)n * LC;
            float dacc = 0.f;
            for (int s = 0; s < n_src; ++s) {
                const size_t off = ((size_t)(b * n_src + s) * N + n) * ldt + f;
                const float mv = m[off];
                float dl = 0.f;
                for (int q = 0; q < LC; ++q) dl = fmaf(dsample(s, q), Dn[q], dl);
                dpre[off] = fvalid ? (raw_mask ? dl * wv : dl * wv * mv * (1.f - mv)) : 0.f;
                dacc += dl * mv;
            }
            dwrow[(size_t)n * ldt + f] = fvalid ? dacc : 0.f;
        }
    }
}

// =====================================================================================
// Decoder forward for the mono 16-tap / stride-8 basis (Cout*L = 16, R = 2): one workgroup = 64 frames, a 256-byte ALIGNED
// run of every row, of one sample for ALL its sources, so w is read once and every mask once, two full cache lines per
// wave load (the 63-frame tiles of the general kernel start on odd frames: three lines per 256 bytes, and every source
// re-read w: 797 MB fetched for 402).  No halo frame: the eight samples a tile shares with its neighbour are added with
// atomicAdd onto a zeroed `est` by both of them (two addends: the sum does not depend on the order), the rest are stores.
// Four waves split the basis rows; lane = frame; the decoder row D[n][:] is wave-uniform (scalar loads).
// =====================================================================================
template <int NSRC>
__global__ __launch_bounds__(256) void decoder_fwd16_kernel(const float* __restrict__ w, const float* __restrict__ m, const float* __restrict__ D,
                                                            float* __restrict__ est, float* __restrict__ latent, int n_src, int N, int F,
                                                            int ldt, int Tout, int pad_left) {
    constexpr int RU = 4;                             // rows per trip: RU * (1 + n_src) independent loads in flight per lane (8 rows: 197 us instead of 134)
    __shared__ float ys[4][NSRC][64][17];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int b = blockIdx.y, f0 = blockIdx.x * 64, f = f0 + lane;
    const bool fvalid = f < F;
    const float* wrow = w + (size_t)b * N * ldt + f;
    const float* mrow = m + (size_t)b * n_src * N * ldt + f;
    float* lrow = latent ? latent + (size_t)b * n_src * N * ldt + f : nullptr;
    float acc[NSRC][16];
#pragma unroll
    for (int s = 0; s < NSRC; ++s)
#pragma unroll
        for (int q = 0; q < 16; ++q) acc[s][q] = 0.f;
    const int nper = (N + 3) / 4;
    const int n_lo = wv * nper, n_hi = n_lo + nper < N ? n_lo + nper : N;
    for (int n = n_lo; n < n_hi; n += RU) {
        float wv4[RU], mv4[NSRC][RU];
#pragma unroll
        for (int r = 0; r < RU; ++r) {
            const bool ok = n + r < n_hi;
            wv4[r] = ok ? wrow[(size_t)(n + r) * ldt] : 0.f;
#pragma unroll
            for (int s = 0; s < NSRC; ++s) mv4[s][r] = ok && s < n_src ? mrow[((size_t)s * N + n + r) * ldt] : 0.f;
        }
#pragma unroll
        for (int r = 0; r < RU; ++r) {
            if (n + r >= n_hi) break;
            const float* Dn = D + (size_t)(n + r) * 16;
#pragma unroll
            for (int s = 0; s < NSRC; ++s) {
                if (s >= n_src) break;
                const float wh = fvalid ? wv4[r] * mv4[s][r] : 0.f;
                if (lrow) lrow[((size_t)s * N + n + r) * ldt] = wh;
#pragma unroll
                for (int q = 0; q < 16; ++q) acc[s][q] = fmaf(wh, Dn[q], acc[s][q]);
            }
        }
    }
#pragma unroll
    for (int s = 0; s < NSRC; ++s)
#pragma unroll
        for (int q = 0; q < 16; ++q) ys[wv][s][lane][q] = acc[s][q];
    __syncthreads();
    // overlap-add: padded sample 8*f + k of this tile, o = 8*(f - f0) + k in [0, 520): frame o/8 at tap k (o < 512) and frame o/8 - 1 at tap k + 8 (o >= 8)
    for (int j = threadIdx.x; j < 520 * n_src; j += 256) {
        const int s = j / 520, o = j % 520;
        const int tau = 8 * f0 + o - pad_left;
        if (tau < 0 || tau >= Tout) continue;
        const int fo = o >> 3, k = o & 7;
        float v = 0.f;
        if (fo < 64) v += (ys[0][s][fo][k] + ys[1][s][fo][k]) + (ys[2][s][fo][k] + ys[3][s][fo][k]);
        if (fo >= 1) v += (ys[0][s][fo - 1][k + 8] + ys[1][s][fo - 1][k + 8]) + (ys[2][s][fo - 1][k + 8] + ys[3][s][fo - 1][k + 8]);
        float* dst = est + ((size_t)b * n_src + s) * Tout + tau;
        if (o < 8 || o >= 512) atomicAdd(dst, v);          // shared with the neighbouring tile
        else *dst = v;
    }
}

}  // namespace

// ---------------------------------------------------------------------------------------
extern "C" int sep_encoder_fwd(const float* x, const float* E, float* w, double* stats, int B, int Cin, int Tin, int N,
                               int L, int S, int F, int ldt, int pad_left, int relu, sep_stream_t stream) {
    SEP_REQUIRE(x && E && w && stats, "sep_encoder_fwd: null pointer");
    SEP_REQUIRE(B > 0 && Cin > 0 && N > 0 && L > 0 && S > 0 && F > 0 && F <= ldt && ldt % 128 == 0, "sep_encoder_fwd: bad sizes (F=%d ldt=%d)", F, ldt);
    const int span = ENC_FT * S + L - S;
    const size_t smem = (size_t)Cin * span * sizeof(float);
    SEP_REQUIRE(smem <= 150 * 1024, "sep_encoder_fwd: Cin*(128*S+L-S) floats exceed LDS (Cin=%d L=%d S=%d)", Cin, L, S);
    if (Cin == 1 && L == 16 && S == 8 && B <= 65535) {
        sep_set_kernel("encoder_l16s8");
        hipLaunchKernelGGL(encoder_fwd_l16s8_kernel, dim3(ceil_div(ldt, 256), B), dim3(256), 0, (hipStream_t)stream, x, E, w, stats, Tin, N, F, ldt, pad_left, relu);
        SEP_CHECK_LAUNCH("sep_encoder_fwd");
        return 0;
    }
    dim3 grid(ldt / ENC_FT, B);
    if (Cin * L == 16) {
        sep_set_kernel("encoder<16>");
        hipLaunchKernelGGL(encoder_fwd_kernel<16>, grid, dim3(256), smem, (hipStream_t)stream, x, E, w, stats, B, Cin, Tin, N, L, S, F, ldt, pad_left, relu);
    } else {
        sep_set_kernel("encoder<0>");
        hipLaunchKernelGGL(encoder_fwd_kernel<0>, grid, dim3(256), smem, (hipStream_t)stream, x, E, w, stats, B, Cin, Tin, N, L, S, F, ldt, pad_left, relu);
    }
    SEP_CHECK_LAUNCH("sep_encoder_fwd");
    return 0;
}

extern "C" int sep_unfold(const float* x, float* frames, int Bp, int C, int Tin, int L, int S, int F, int ldt,
                          int pad_left, sep_stream_t stream) {
    SEP_REQUIRE(x && frames && Bp > 0 && C > 0 && L > 0 && S > 0 && F > 0 && F <= ldt, "sep_unfold: bad arguments");
    SEP_REQUIRE(Bp <= 65535 && C * L <= 65535, "sep_unfold: grid too large");
    dim3 grid(ceil_div(ldt, 256), C * L, Bp);
    hipLaunchKernelGGL(unfold_kernel, grid, dim3(256), 0, (hipStream_t)stream, x, frames, C, Tin, L, S, F, ldt, pad_left);
    SEP_CHECK_LAUNCH("sep_unfold");
    return 0;
}

extern "C" int sep_decoder_fwd(const float* w, const float* m, const float* D, float* est, float* latent, int B, int n_src,
                               int N, int Cout, int L, int S, int F, int ldt, int Tout, int pad_left, sep_stream_t stream) {
    SEP_REQUIRE(w && m && D && est, "sep_decoder_fwd: null pointer");
    SEP_REQUIRE(L % S == 0 && L / S <= 64, "sep_decoder_fwd: kernel_size %d must be a multiple of stride %d", L, S);
    const int LC = Cout * L;
    SEP_REQUIRE(LC <= 144, "sep_decoder_fwd: Cout*L=%d too large for the LDS frame buffer", LC);
    SEP_REQUIRE((long)B * n_src <= 65535, "sep_decoder_fwd: B*n_src too large");
    if (LC == 16 && L == 16 && S == 8 && n_src <= 4 && ldt % 64 == 0 && B <= 65535) {
        // est is completed by stores and by two-addend atomic adds at the tile seams: it starts from zero
        SEP_REQUIRE(hipMemsetAsync(est, 0, (size_t)B * n_src * Tout * sizeof(float), (hipStream_t)stream) == hipSuccess, "sep_decoder_fwd: memset failed");
        const dim3 g16(ldt / 64, B);
        sep_set_kernel(n_src <= 2 ? "decoder_fwd16<2>" : "decoder_fwd16<4>");
        if (n_src <= 2) hipLaunchKernelGGL(decoder_fwd16_kernel<2>, g16, dim3(256), 0, (hipStream_t)stream, w, m, D, est, latent, n_src, N, F, ldt, Tout, pad_left);
        else hipLaunchKernelGGL(decoder_fwd16_kernel<4>, g16, dim3(256), 0, (hipStream_t)stream, w, m, D, est, latent, n_src, N, F, ldt, Tout, pad_left);
        SEP_CHECK_LAUNCH("sep_decoder_fwd");
        return 0;
    }
    const int R = L / S, FB = (LC == 16 ? 64 : 256) - (R - 1);
    SEP_REQUIRE(FB > 0, "sep_decoder_fwd: kernel_size / stride too large");
    dim3 grid(ceil_div(ldt + R - 1, FB), B * n_src);
    const size_t smem = (size_t)256 * (LC + 1) * sizeof(float);
    sep_set_kernel(LC == 16 ? "decoder_fwd<16>" : "decoder_fwd<0>");
    if (LC == 16)
        hipLaunchKernelGGL(decoder_fwd_kernel<16>, grid, dim3(256), smem, (hipStream_t)stream, w, m, D, est, latent, n_src, N, Cout, L, S, F, ldt, Tout, pad_left);
    else
        hipLaunchKernelGGL(decoder_fwd_kernel<0>, grid, dim3(256), smem, (hipStream_t)stream, w, m, D, est, latent, n_src, N, Cout, L, S, F, ldt, Tout, pad_left);
    SEP_CHECK_LAUNCH("sep_decoder_fwd");
    return 0;
}

extern "C" int sep_decoder_bwd(const float* d_est, const float* w, const float* m, const float* D, float* dpre, float* dwm,
                               int B, int n_src, int N, int Cout, int L, int S, int F, int ldt, int Tout, int pad_left,
                               int raw_mask, sep_stream_t stream) {
    SEP_REQUIRE(d_est && w && m && D && dpre && dwm, "sep_decoder_bwd: null pointer");
    SEP_REQUIRE(B <= 65535, "sep_decoder_bwd: B too large");
    const int nz = N >= 64 ? 8 : 1;                               // 2048 workgroups at paper-best instead of 256
    dim3 grid(ceil_div(ldt, 256), B, nz);
    const int LC = Cout * L;
#define SEP_DEB(NAME) sep_set_kernel(nz == 8 ? NAME "/nz8" : NAME "/nz1")
    if (LC == 16 && n_src <= 2) SEP_DEB("decoder_bwd<16,2>");
    else if (LC == 16 && n_src <= 4) SEP_DEB("decoder_bwd<16,4>");
    else SEP_DEB("decoder_bwd<0,0>");
#undef SEP_DEB
    if (LC == 16 && n_src <= 2)
        hipLaunchKernelGGL((decoder_bwd_kernel<16, 2>), grid, dim3(256), 0, (hipStream_t)stream, d_est, w, m, D, dpre, dwm, n_src, N, Cout, L, S, F, ldt, Tout, pad_left, raw_mask);
    else if (LC == 16 && n_src <= 4)
        hipLaunchKernelGGL((decoder_bwd_kernel<16, 4>), grid, dim3(256), 0, (hipStream_t)stream, d_est, w, m, D, dpre, dwm, n_src, N, Cout, L, S, F, ldt, Tout, pad_left, raw_mask);
    else
        hipLaunchKernelGGL((decoder_bwd_kernel<0, 0>), grid, dim3(256), 0, (hipStream_t)stream, d_est, w, m, D, dpre, dwm, n_src, N, Cout, L, S, F, ldt, Tout, pad_left, raw_mask);
    SEP_CHECK_LAUNCH("sep_decoder_bwd");
    return 0;
}
