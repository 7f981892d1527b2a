// Sample-rate conversion (ABI 23, additive; sepkernels/resample.py): whole signals (sep_resample_fwd) and online streams (sep_resample_stream_fwd).
//
// The definition is torchaudio.functional.resample, restated in include/sepkernels.h: with o = orig / gcd, u = new / gcd a polyphase FIR of u
// phases and K = 2 width + o taps whose frame i reads the input from sample i o - width on.  As a convolution that is `u` output channels of K
// taps at stride o; most of those taps are zero (the window ends where |t| reaches lowpass_filter_width: at 44.1 k -> 8 k 67 of 509 survive in
// any phase).  The host hands over the COMPACT table: per phase the Kc taps from first[p] on, tap-major (table[j u + p]), and the kernels do
// Kc multiply-adds per output on an input span staged once in LDS.  The reference calls torchaudio for this (egs/musdb18/common/src/dataset.py:623).
//
// One kernel template; its two arguments choose among:
//   frames<U>   u = U in {1, 2, 3} (the speech conversions 16 k -> 8 k, 8 k -> 16 k, 48 k -> 8 k): a thread owns a frame and its U outputs, lanes
//               on consecutive frames, so the tap of a step is the same LDS word for the whole wave (a broadcast) and U is a compile-time
//               trip count.
//   phases      any u (147, 80, 160): a thread owns output q = tid + 256 n of the tile, lanes on consecutive phases of (mostly) one frame, so the
//               table is read with consecutive lanes on consecutive words (tap-major) and the input words of a step are a handful.
//   STREAM      the input of a row is [history of its slot | its chunk] instead of a signal between two runs of zeros; see the contract.
// Every output is sum_{j < Kc} table[j u + p] x[...] by fmaf in ascending j from +0 in fp32 -- one function for all four, so where a sample
// lies in a row, a tile or a chunk cannot change a bit.  An output is written once by the thread that owns it; no atomics; offsets are 64-bit.
#include "common.hpp"

namespace {

constexpr int RS_SPAN = 8192;       // input samples staged per tile: 32 KB of LDS
constexpr int RS_TAB_F = 2048;      // table words in LDS, frames<U> (8 KB) ...
constexpr int RS_TAB_P = 6144;      // ... and phases (24 KB: 160 phases x 34 taps of 44.1 k -> 16 k are 5440)
constexpr int RS_PHASES = 1024;     // first[] in LDS (4 KB)
constexpr int RS_OUT = 2048;        // outputs of a tile at most (frames<U>: frames), eight steps of the workgroup
constexpr int RS_HMAX = SEP_RESAMPLE_MAX_HISTORY;      // a history row goes through eight registers per thread of tile 0
static_assert(RS_HMAX == 8 * 256, "the new history is held as eight values per thread");

// One output: the Kc taps of phase p (stride u in the tap-major table) on the staged samples from xp on.  The only arithmetic of the file.
__device__ __forceinline__ float rs_dot(const float* ts, const int u, const int p, const float* xp, const int Kc) {
    float acc = 0.f;
    for (int j = 0; j < Kc; ++j) acc = fmaf(ts[j * u + p], xp[j], acc);
    return acc;
}

// grid: row * ntile + tile, 256 threads.  Tile `tile` owns the frames [tile FT, tile FT + nf) of its row: outputs [tile FT u, ...) below T_out.
// xs[e] holds the sample that frame i0, tap 0 of the FULL table would read, plus e: offline x[i0 o - width + e] or zero outside [0, T);
// streaming cat[i0 o + e] of cat = [history (H) | chunk (T)].  (nf - 1) o + K <= RS_SPAN by the host's choice of FT.
// STREAM: the history row of a slot is read and written by the workgroup of tile 0 of its row alone (the host refuses a geometry in which a
// later tile would reach into it); that workgroup reads its span AND the H samples that become the new history, the last H of cat, before
// the barrier and writes them after it.
template <int U, bool STREAM>
__global__ __launch_bounds__(256) void resample_kernel(const float* __restrict__ x, const int64_t x_pitch, const float* __restrict__ table,
                                                       const int32_t* __restrict__ first, float* __restrict__ y, const int64_t y_pitch,
                                                       float* __restrict__ history, const int32_t* __restrict__ slots, const int64_t T,
                                                       const int64_t T_out, const int64_t frames, const int o, const int u_rt, const int width,
                                                       const int Kc, const int FT, const int ntile, const int H) {
    constexpr int TAB = U ? RS_TAB_F : RS_TAB_P;
    __shared__ float xs[RS_SPAN];
    __shared__ float ts[TAB];
    __shared__ int fs[U ? 4 : RS_PHASES];
    const int u = U ? U : u_rt;
    const int tid = threadIdx.x, K = 2 * width + o;
    const int64_t row = blockIdx.x / ntile;
    const int tile = (int)(blockIdx.x % ntile);
    const int64_t i0 = (int64_t)tile * FT;
    const int nf = frames - i0 < FT ? (int)(frames - i0) : FT;
    const int span = (nf - 1) * o + K;
    const int64_t s0 = i0 * o;
    const float* xr = x + row * x_pitch;
    float* yr = y + row * y_pitch;
    for (int e = tid; e < Kc * u; e += 256) ts[e] = table[e];
    for (int p = tid; p < u; p += 256) {                   // whatever first[] holds, phase p stays inside its K taps
        const int f = first[p];
        fs[p] = f < 0 ? 0 : f > K - Kc ? K - Kc : f;
    }
    if constexpr (STREAM) {
        const int64_t slot = slots ? (int64_t)slots[row] : row;
        float* hist = history + slot * H;
        for (int e = tid; e < span; e += 256) {
            const int64_t s = s0 + e;
            xs[e] = s < H ? hist[s] : s - H < T ? xr[s - H] : 0.f;
        }
        float hv[8];
        if (tile == 0) {
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                const int64_t s = T + tid + 256 * q;           // cat[T + e] -> history[e], e < H
                hv[q] = tid + 256 * q < H ? (s < H ? hist[s] : xr[s - H]) : 0.f;
            }
        }
        __syncthreads();
        if (tile == 0) {
#pragma unroll
            for (int q = 0; q < 8; ++q)
                if (tid + 256 * q < H) hist[tid + 256 * q] = hv[q];
        }
    } else {
        for (int e = tid; e < span; e += 256) {
            const int64_t t = s0 + e - width;
            xs[e] = t >= 0 && t < T ? xr[t] : 0.f;
        }
        __syncthreads();
    }
    if constexpr (U > 0) {
        for (int f = tid; f < nf; f += 256) {
            const int64_t t0 = (i0 + f) * U;
#pragma unroll
            for (int p = 0; p < U; ++p)
                if (t0 + p < T_out) yr[t0 + p] = rs_dot(ts, U, p, xs + f * o + fs[p], Kc);
        }
    } else {
        const int64_t t0 = i0 * u;
        for (int q = tid; q < nf * u; q += 256) {
            const int f = q / u, p = q - f * u;
            if (t0 + q < T_out) yr[t0 + q] = rs_dot(ts, u, p, xs + f * o + fs[p], Kc);
        }
    }
}

struct rs_plan { int U, FT, ntile, H; int64_t frames; };

// what both calls ask of the filter's geometry, and the tiling: -> null, or the words of the refusal
static const char* rs_make_plan(const int64_t frames, const int64_t R, const int o, const int u, const int width, const int Kc, rs_plan& pl) {
    if (o < 1 || u < 1 || width < 1 || Kc < 1 || o > (1 << 20) || u > (1 << 20) || width > (1 << 20)) return "o, u, width, Kc must be positive (o, u, width <= 2^20)";
    const int K = 2 * width + o;
    if (Kc > K) return "Kc exceeds the K = 2 width + o taps of a phase";
    if (K > RS_SPAN) return "a frame's K = 2 width + o samples exceed the staged span";
    if (u > RS_PHASES) return "more phases than the kernels take";
    pl.U = u <= 3 && (int64_t)Kc * u <= RS_TAB_F ? u : 0;
    if ((int64_t)Kc * u > RS_TAB_P) return "the compact table exceeds the kernels' LDS";
    const int by_span = (RS_SPAN - K) / o + 1, by_out = pl.U ? RS_OUT : (RS_OUT / u > 1 ? RS_OUT / u : 1);
    pl.FT = by_span < by_out ? by_span : by_out;
    pl.frames = frames;
    const int64_t ntile = (frames + pl.FT - 1) / pl.FT;
    if (ntile * R > 0x7fffffff) return "more than 2^31 - 1 tiles";
    pl.ntile = (int)ntile;
    pl.H = width + (width + o - 1) / o * o;
    return nullptr;
}

template <bool STREAM>
static void rs_launch(const rs_plan& pl, const float* x, int64_t x_pitch, const float* table, const int32_t* first, float* y, int64_t y_pitch, float* history,
                      const int32_t* slots, int64_t R, int64_t T, int64_t T_out, int o, int u, int width, int Kc, hipStream_t stream) {
    const dim3 grid((unsigned)(R * pl.ntile));
#define SEP_RS(UU, NAME)                                                                                                                              \
    sep_set_kernel(STREAM ? "resample_stream_" NAME : "resample_" NAME);                                                                             \
    hipLaunchKernelGGL((resample_kernel<UU, STREAM>), grid, dim3(256), 0, stream, x, x_pitch, table, first, y, y_pitch, history, slots, T, T_out, \
                       pl.frames, o, u, width, Kc, pl.FT, pl.ntile, pl.H)
    if (pl.U == 1) { SEP_RS(1, "frames<1>"); }
    else if (pl.U == 2) { SEP_RS(2, "frames<2>"); }
    else if (pl.U == 3) { SEP_RS(3, "frames<3>"); }
    else { SEP_RS(0, "phases"); }
#undef SEP_RS
}

}  // namespace

extern "C" int sep_resample_fwd(const float* x, int64_t x_pitch, const float* table, const int32_t* first, float* y, int64_t y_pitch, int R, int64_t T,
                                int64_t T_out, int o, int u, int width, int Kc, sep_stream_t stream) {
    SEP_REQUIRE(x && table && first && y, "sep_resample_fwd: null pointer");
    SEP_REQUIRE(R >= 1 && T >= 1 && T <= ((int64_t)1 << 40) && x_pitch >= T, "sep_resample_fwd: bad arguments (R=%d T=%lld x_pitch=%lld; R >= 1, 1 <= T <= 2^40, x_pitch >= T)",
                R, (long long)T, (long long)x_pitch);
    rs_plan pl;
    const bool rates = o >= 1 && u >= 1 && o <= (1 << 20) && u <= (1 << 20);
    const int64_t want = rates ? (T * u + o - 1) / o : 0;                      // u T < 2^60
    const char* why = rs_make_plan(rates ? (want + u - 1) / u : 1, R, o, u, width, Kc, pl);
    SEP_REQUIRE(!why, "sep_resample_fwd: refused (R=%d T=%lld o=%d u=%d width=%d Kc=%d): %s", R, (long long)T, o, u, width, Kc, why ? why : "");
    SEP_REQUIRE(T_out == want && y_pitch >= T_out, "sep_resample_fwd: bad arguments (T_out=%lld y_pitch=%lld; T_out = ceil(u T / o) = %lld, y_pitch >= T_out)",
                (long long)T_out, (long long)y_pitch, (long long)want);
    rs_launch<false>(pl, x, x_pitch, table, first, y, y_pitch, nullptr, nullptr, R, T, T_out, o, u, width, Kc, (hipStream_t)stream);
    SEP_CHECK_LAUNCH("sep_resample_fwd");
    return 0;
}

extern "C" int sep_resample_stream_fwd(const float* chunk, const float* table, const int32_t* first, float* history, float* y, const int32_t* slots, int A,
                                       int num_streams, int m, int o, int u, int width, int Kc, sep_stream_t stream) {
    SEP_REQUIRE(chunk && table && first && history && y, "sep_resample_stream_fwd: null pointer");
    SEP_REQUIRE(A >= 1 && num_streams >= A && m >= 1 && m <= (1 << 30) && (slots || A == num_streams),
                "sep_resample_stream_fwd: bad arguments (A=%d num_streams=%d m=%d; 1 <= A <= num_streams, A = num_streams without slots, 1 <= m <= 2^30)", A,
                num_streams, m);
    rs_plan pl;
    const char* why = rs_make_plan(m, A, o, u, width, Kc, pl);
    SEP_REQUIRE(!why, "sep_resample_stream_fwd: refused (A=%d m=%d o=%d u=%d width=%d Kc=%d): %s", A, m, o, u, width, Kc, why ? why : "");
    SEP_REQUIRE(pl.H <= RS_HMAX, "sep_resample_stream_fwd: refused (o=%d width=%d): the history of %d samples per stream exceeds %d", o, width, pl.H, RS_HMAX);
    SEP_REQUIRE(pl.ntile == 1 || (int64_t)pl.FT * o >= pl.H, "sep_resample_stream_fwd: refused (o=%d u=%d width=%d): a tile of %d frames is shorter than the history of %d samples",
                o, u, width, pl.FT, pl.H);
    const int64_t T = (int64_t)m * o, T_out = (int64_t)m * u;
    rs_launch<true>(pl, chunk, T, table, first, y, T_out, history, slots, A, T, T_out, o, u, width, Kc, (hipStream_t)stream);
    SEP_CHECK_LAUNCH("sep_resample_stream_fwd");
    return 0;
}
