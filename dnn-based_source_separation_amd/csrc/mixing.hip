// Dynamic mixing from a device-resident corpus (ABI 23, additive; sepkernels/mixing.py): sep_mix_draw writes the plan of a training batch,
// sep_mix_render gathers, scales and sums it into sources (B, n, T), mixture (B, 1, T) and, with a noise corpus, a noise row (B, 1, T).
//
// The corpus is ONE flat tensor of int16 or fp32 samples with an index beside it (include/sepkernels.h: offsets, spk_first, level); the draw is
// counter-based -- a function of (seed, item, draw number) in wrapping uint64, no generator state -- and takes its gains from a table the host
// built in fp64, so nothing transcendental is evaluated here and a Python-integer restatement of the rule gives the same plan bit for bit.
// The step lives in device memory: a recorded sep_mix_draw replays into the NEXT batch, as sep_adam_step_dev does with its step count.
//
// Render: every output element is written once by the thread that owns it, no atomics; two runs give the same bits.  The plan is device memory
// the library cannot look at: the utterance is clamped into [0, U), the start into [0, len - 1], and a sample is read only where
// lead <= t and t - lead < len - start, so no plan can index outside the storage.  Instances (sep_last_kernel):
//   mix_render_vec<int16,8>    T % 4 == 0, outputs 16-byte aligned: a thread owns 8 consecutive samples of all rows; per row it loads the (at most) two
//                              ALIGNED 16-byte words that hold them and selects by the row's misalignment, which is the same for every thread of an
//                              (item, source) because a thread's first sample is a multiple of 8 -- no 2-byte loads.  A word is loaded only when it
//                              holds a sample of the utterance, so it lies within 7 elements of it: inside the corpus's guard zeros.
//   mix_render_vec<float,4>    the same with 4 samples per thread (4-byte loads under the predicate)
//   mix_render_scalar<int16|float>   a thread per sample: any T, any alignment
// About 8 MB move per paper-size batch: the kernels are bound by launch and fill, no tile size is tuned and no fraction of a roof is claimed.
//
// Speed perturbation (sep_mix_draw_speed, sep_mix_render_speed; the definition stands in include/sepkernels.h): every source also draws one of J
// integer percentages and is resampled from rate P to rate 100 WHILE it is gathered -- the draw places it by its perturbed length, the render
// stages the row's polyphase filter and the input span of a tile in LDS and sums the taps in fp64 (every product exact: the same bits as numpy).
//   mix_render_speed<int16|float>          T % 4 == 0, outputs 16-byte aligned: a workgroup owns a tile of 256 x 8 (4) outputs of one item, 16-byte stores
//   mix_render_speed_scalar<int16|float>   the same with scalar stores: any T, any alignment
#include "common.hpp"

// gain * (sample * scale) is rounded once and the mixture adds the ROUNDED sources: no product may be fused into the sum
#pragma clang fp contract(off)

namespace {

// ---- the draw (the rule of include/sepkernels.h, line for line) -----------------------------------------------------------------------
__device__ __forceinline__ uint64_t mx_mix64(uint64_t z) {
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
__device__ __forceinline__ uint64_t mx_below(const uint64_t w, const uint64_t m) { return ((w >> 32) * m) >> 32; }      // 1 <= m < 2^31

// utterance u of an index the library cannot look at: u clamped into [0, U), its length into [1, 2^31)
__device__ __forceinline__ int64_t mx_length(const int64_t* __restrict__ offsets, const int U, int64_t& u) {
    u = u < 0 ? 0 : u >= U ? U - 1 : u;
    const int64_t len = offsets[u + 1] - offsets[u];
    return len < 1 ? 1 : len > 0x7fffffff ? 0x7fffffff : len;
}

// position and gain of one row from draws `wpos`, `wgain`: a long utterance is cropped at a random start, a short one placed at a random lead
__device__ __forceinline__ void mx_place(const int64_t u, const int64_t len, const int T, const uint64_t wpos, const uint64_t wgain, const float* __restrict__ level,
                                         const float* __restrict__ table, const int G, int64_t* __restrict__ row, float* __restrict__ gain) {
    const int64_t start = len >= T ? (int64_t)mx_below(wpos, (uint64_t)(len - T + 1)) : 0;
    const int64_t lead = len >= T ? 0 : (int64_t)mx_below(wpos, (uint64_t)(T - len + 1));
    const int64_t g = (int64_t)mx_below(wgain, (uint64_t)G);
    row[0] = u;
    row[1] = start;
    row[2] = lead;
    row[3] = g;
    *gain = level[u] * table[g];
}

// speed descriptors (include/sepkernels.h): SEP_MIX_SPEED_DESC int32 per speed {o, u, width, Kc, table offset, first offset, P, 0}; device memory the
// library cannot look at, so every field is clamped into the published limits where it is read
struct mx_speed {
    int o, u, width, Kc, toff, foff;
};
__device__ __forceinline__ int mx_clampi(const int v, const int lo, const int hi) { return v < lo ? lo : v > hi ? hi : v; }
__device__ __forceinline__ mx_speed mx_read_speed(const int32_t* __restrict__ desc, const int j) {
    const int32_t* d = desc + (int64_t)SEP_MIX_SPEED_DESC * j;
    return mx_speed{mx_clampi(d[0], 1, SEP_MIX_SPEED_MAX), mx_clampi(d[1], 1, 100), mx_clampi(d[2], 0, SEP_MIX_SPEED_MAX_TAPS), mx_clampi(d[3], 1, SEP_MIX_SPEED_MAX_TAPS), d[4], d[5]};
}
// len' = ceil(u len / o) formed in int64 and clamped into [1, 2^31); len itself is read as clamped into [0, 2^31)
__device__ __forceinline__ int64_t mx_speed_length(const mx_speed& s, int64_t len) {
    len = len < 0 ? 0 : len > 0x7fffffff ? 0x7fffffff : len;
    const int64_t lp = ((int64_t)s.u * len + s.o - 1) / s.o;
    return lp < 1 ? 1 : lp > 0x7fffffff ? 0x7fffffff : lp;
}

// ONE workgroup; its threads loop over the items.  Every thread reads the step, then the barrier, then one thread stores the increment.
// SPEED (sep_mix_draw_speed): source i also draws a speed index j = below(word(.., 4 n + 3 + i), J) and is placed by its perturbed length.
template <bool SPEED>
__global__ __launch_bounds__(256) void mix_draw_kernel(const int64_t* __restrict__ offsets, const int32_t* __restrict__ spk_first, const int U, const int S,
                                                       const int64_t* __restrict__ noise_offsets, const int U_noise, const float* __restrict__ level,
                                                       const float* __restrict__ gain_table, const int G, const float* __restrict__ noise_level,
                                                       const float* __restrict__ noise_gain_table, const int G_noise, int64_t* counter, const uint64_t seed,
                                                       const uint64_t item_stride, const uint64_t item_first, const int B, const int n, const int T,
                                                       int64_t* __restrict__ plan, float* __restrict__ gain, const int32_t* __restrict__ desc, const int J,
                                                       int32_t* __restrict__ speed) {
    const uint64_t step = (uint64_t)counter[0];
    __syncthreads();
    if (threadIdx.x == 0) counter[0] = (int64_t)(step + 1);
    const int R = n + (noise_offsets ? 1 : 0);
    for (int b = threadIdx.x; b < B; b += 256) {
        const uint64_t item = step * item_stride + item_first + (uint64_t)b;
        const uint64_t key = mx_mix64(seed + 0x9E3779B97F4A7C15ull * (item + 1));
        int chosen[SEP_MIX_MAX_SOURCES];                       // the speakers taken so far, ascending (static indices only: registers)
#pragma unroll
        for (int c = 0; c < SEP_MIX_MAX_SOURCES; ++c) chosen[c] = 0x7fffffff;
#pragma unroll
        for (int i = 0; i < SEP_MIX_MAX_SOURCES; ++i) {
            if (i < n) {
                int r = (int)mx_below(mx_mix64(key + (uint64_t)i), (uint64_t)(S - i));
                int pos = 0;
#pragma unroll
                for (int c = 0; c < i; ++c)
                    if (r >= chosen[c]) { ++r; pos = c + 1; }
#pragma unroll
                for (int c = i; c > 0; --c)
                    if (c > pos) chosen[c] = chosen[c - 1];
#pragma unroll
                for (int c = 0; c <= i; ++c)
                    if (c == pos) chosen[c] = r;
                const int s = r < 0 ? 0 : r >= S ? S - 1 : r;
                const int f0 = spk_first[s], cnt = spk_first[s + 1] - f0;
                int64_t u = (int64_t)f0 + (int64_t)mx_below(mx_mix64(key + (uint64_t)(n + i)), (uint64_t)(cnt < 1 ? 1 : cnt));
                int64_t len = mx_length(offsets, U, u);
                const int64_t e = (int64_t)b * R + i;
                if constexpr (SPEED) {
                    const int j = (int)mx_below(mx_mix64(key + (uint64_t)(4 * n + 3 + i)), (uint64_t)J);
                    len = mx_speed_length(mx_read_speed(desc, j), len);
                    speed[e] = j;
                }
                mx_place(u, len, T, mx_mix64(key + (uint64_t)(2 * n + i)), mx_mix64(key + (uint64_t)(3 * n + i)), level, gain_table, G, plan + 4 * e, gain + e);
            }
        }
        if (noise_offsets) {
            int64_t u = (int64_t)mx_below(mx_mix64(key + (uint64_t)(4 * n)), (uint64_t)U_noise);
            const int64_t len = mx_length(noise_offsets, U_noise, u);
            const int64_t e = (int64_t)b * R + n;
            if constexpr (SPEED) speed[e] = -1;                  // the noise row is never perturbed
            mx_place(u, len, T, mx_mix64(key + (uint64_t)(4 * n + 1)), mx_mix64(key + (uint64_t)(4 * n + 2)), noise_level, noise_gain_table, G_noise, plan + 4 * e,
                     gain + e);
        }
    }
}

// ---- the render ------------------------------------------------------------------------------------------------------------------------
template <typename P> struct mx_kind;
template <> struct mx_kind<int16_t> { static constexpr float scale = 0x1p-15f; };       // (float)pcm * 2^-15 is exact
template <> struct mx_kind<float> { static constexpr float scale = 1.f; };

// one row of a plan as the kernels use it: sample t of the row is pcm[first + (t - lead)] where lead <= t and t - lead < avail
struct mx_row {
    int64_t first, avail, lead;
    float g;
};
__device__ __forceinline__ mx_row mx_read_row(const int64_t* __restrict__ row, const float g, const int64_t* __restrict__ offsets, const int U) {
    int64_t u = row[0];
    u = u < 0 ? 0 : u >= U ? U - 1 : u;
    const int64_t o0 = offsets[u], len = offsets[u + 1] - o0;
    int64_t start = row[1];
    start = start > len - 1 ? len - 1 : start;
    start = start < 0 ? 0 : start;
    return mx_row{o0 + start, len > start ? len - start : 0, row[2], g};
}
// whatever lead holds (the differences are formed in wrapping uint64: a hostile lead overflows nothing)
__device__ __forceinline__ bool mx_inside(const mx_row& r, const int64_t t) { return r.lead <= t && (uint64_t)t - (uint64_t)r.lead < (uint64_t)r.avail; }
template <typename P>
__device__ __forceinline__ float mx_sample(const mx_row& r, const P v) { return r.g * ((float)v * mx_kind<P>::scale); }

// the V samples of row r from t0 on (t0 a multiple of V); +0 where the predicate fails
template <typename P, int V>
__device__ __forceinline__ void mx_gather(const P* __restrict__ pcm, const mx_row& r, const int64_t t0, float (&out)[V]) {
    unsigned inside = 0;
#pragma unroll
    for (int j = 0; j < V; ++j) inside |= mx_inside(r, t0 + j) ? 1u << j : 0u;
#pragma unroll
    for (int j = 0; j < V; ++j) out[j] = 0.f;
    if (!inside) return;
    const uint64_t e0 = (uint64_t)r.first + ((uint64_t)t0 - (uint64_t)r.lead);          // element of sample t0 (meaningful where `inside`)
    if constexpr (sizeof(P) == 2) {
        static_assert(V == 8, "eight int16 samples are one 16-byte word");
        const uintptr_t a = (uintptr_t)pcm + 2 * (uintptr_t)e0;
        const unsigned m = (unsigned)(a & 15) >> 1;                                     // the row's misalignment in elements: uniform per (item, source)
        const uint4* w = reinterpret_cast<const uint4*>(a & ~(uintptr_t)15);
        uint4 lo = make_uint4(0, 0, 0, 0), hi = lo;
        if (inside & (0xffu >> m)) lo = w[0];                                           // samples j < 8 - m lie in the first word ...
        if (m && (inside >> (8 - m))) hi = w[1];                                        // ... the others in the second: a word is loaded only for a sample of the utterance
        const unsigned d[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
        const unsigned q = m >> 1, odd = m & 1;
        unsigned s[5];
#pragma unroll
        for (int k = 0; k < 5; ++k) s[k] = q == 0 ? d[k] : q == 1 ? d[k + 1] : q == 2 ? d[k + 2] : d[(k + 3) & 7];      // (k = 4, q = 3 is only read when odd: d[7])
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const unsigned word = odd ? (s[k] >> 16) | (s[k + 1] << 16) : s[k];
            const int16_t v0 = (int16_t)(word & 0xffffu), v1 = (int16_t)(word >> 16);
            if (inside & (1u << (2 * k))) out[2 * k] = mx_sample<int16_t>(r, v0);
            if (inside & (2u << (2 * k))) out[2 * k + 1] = mx_sample<int16_t>(r, v1);
        }
    } else {
#pragma unroll
        for (int j = 0; j < V; ++j)
            if (inside & (1u << j)) out[j] = mx_sample<P>(r, pcm[e0 + j]);
    }
}

// grid (chunks of 256 threads over ceil(T / V), B).  A thread owns samples [t0, t0 + V) of every row of item b: the n sources, the mixture
// ((s0 + s1) + s2) + ... in ascending order, the noise row added last.
template <typename P, int V>
__global__ __launch_bounds__(256) void mix_render_vec_kernel(const P* __restrict__ pcm, const int64_t* __restrict__ offsets, const int U, const P* __restrict__ noise_pcm,
                                                             const int64_t* __restrict__ noise_offsets, const int U_noise, const int64_t* __restrict__ plan,
                                                             const float* __restrict__ gain, const int n, const int T, float* __restrict__ sources,
                                                             float* __restrict__ mixture, float* __restrict__ noise) {
    const int64_t t0 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * V;
    if (t0 >= T) return;
    const int64_t b = blockIdx.y;
    const int R = n + (noise ? 1 : 0);
    float acc[V], val[V];
#pragma unroll
    for (int j = 0; j < V; ++j) acc[j] = 0.f;
    for (int i = 0; i < R; ++i) {
        const int64_t e = b * R + i;
        const bool is_noise = i == n;
        const mx_row r = is_noise ? mx_read_row(plan + 4 * e, gain[e], noise_offsets, U_noise) : mx_read_row(plan + 4 * e, gain[e], offsets, U);
        mx_gather<P, V>(is_noise ? noise_pcm : pcm, r, t0, val);
#pragma unroll
        for (int j = 0; j < V; ++j) acc[j] = i == 0 ? val[j] : acc[j] + val[j];
        float* dst = (is_noise ? noise + b * T : sources + (b * n + i) * T) + t0;
#pragma unroll
        for (int j = 0; j < V; j += 4)
            if (t0 + j < T) st4(dst + j, make_float4(val[j], val[j + 1], val[j + 2], val[j + 3]));          // T % 4 == 0: a quad is inside or outside
    }
#pragma unroll
    for (int j = 0; j < V; j += 4)
        if (t0 + j < T) st4(mixture + b * T + t0 + j, make_float4(acc[j], acc[j + 1], acc[j + 2], acc[j + 3]));
}

// grid (ceil(T / 256), B): a thread per sample
template <typename P>
__global__ __launch_bounds__(256) void mix_render_scalar_kernel(const P* __restrict__ pcm, const int64_t* __restrict__ offsets, const int U, const P* __restrict__ noise_pcm,
                                                                const int64_t* __restrict__ noise_offsets, const int U_noise, const int64_t* __restrict__ plan,
                                                                const float* __restrict__ gain, const int n, const int T, float* __restrict__ sources,
                                                                float* __restrict__ mixture, float* __restrict__ noise) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= T) return;
    const int64_t b = blockIdx.y;
    const int R = n + (noise ? 1 : 0);
    float acc = 0.f;
    for (int i = 0; i < R; ++i) {
        const int64_t e = b * R + i;
        const bool is_noise = i == n;
        const mx_row r = is_noise ? mx_read_row(plan + 4 * e, gain[e], noise_offsets, U_noise) : mx_read_row(plan + 4 * e, gain[e], offsets, U);
        const P* src = is_noise ? noise_pcm : pcm;
        float v = 0.f;
        if (mx_inside(r, t)) v = mx_sample<P>(r, src[(uint64_t)r.first + ((uint64_t)t - (uint64_t)r.lead)]);
        acc = i == 0 ? v : acc + v;
        (is_noise ? noise + b * T : sources + (b * n + i) * T)[t] = v;
    }
    mixture[b * T + t] = acc;
}

template <typename P, int V>
static void mx_launch(const void* samples, const int64_t* offsets, int U, const void* noise_samples, const int64_t* noise_offsets, int U_noise, const int64_t* plan,
                      const float* gain, int B, int n, int T, float* sources, float* mixture, float* noise, hipStream_t stream) {
    const P* pcm = static_cast<const P*>(samples);
    const P* npcm = static_cast<const P*>(noise_samples);
    if constexpr (V > 0) {
        const unsigned gx = (unsigned)((((int64_t)T + V - 1) / V + 255) / 256);
        hipLaunchKernelGGL((mix_render_vec_kernel<P, V>), dim3(gx, (unsigned)B), dim3(256), 0, stream, pcm, offsets, U, npcm, noise_offsets, U_noise, plan, gain, n, T,
                           sources, mixture, noise);
    } else {
        const unsigned gx = (unsigned)(((int64_t)T + 255) / 256);
        hipLaunchKernelGGL((mix_render_scalar_kernel<P>), dim3(gx, (unsigned)B), dim3(256), 0, stream, pcm, offsets, U, npcm, noise_offsets, U_noise, plan, gain, n, T,
                           sources, mixture, noise);
    }
}

// ---- the render with speed perturbation ---------------------------------------------------------------------------------------------------
// LDS of one workgroup: the input span of a tile, one speed's filter, its `first`, and the tile's outputs of one row (39.8 KB in all).
// The span of a tile of TILE outputs is at most ((TILE - 1) / u + 2) o + 2 width samples: 4404 over the speeds 50 .. 200 at TILE = 2048 (P = 199).
constexpr int MXS_SPAN = 4608, MXS_PHASES = 100, MXS_TAB = SEP_MIX_SPEED_MAX_TAPS * MXS_PHASES;

// element jj of an aligned 16-byte word of the corpus as the raw sample: the int16 integer or the fp32 value
template <typename P>
__device__ __forceinline__ float mxs_elem(const unsigned (&d)[4], const int jj) {
    if constexpr (sizeof(P) == 2) return (float)(int16_t)((jj & 1) ? d[jj >> 1] >> 16 : d[jj >> 1] & 0xffffu);
    else return __uint_as_float(d[jj]);
}

// grid (ceil(T / (256 V)), B).  A workgroup owns a tile of 256 V output samples of item b and loops over its rows; a thread owns samples
// [t0, t0 + V) of every row and keeps the mixture of them in registers.  A copy row (the noise row, a speed with o == u) is sep_mix_render's
// formula through mx_gather.  For a perturbed row the workgroup stages the row's filter and the input span of the tile in LDS (aligned 16-byte
// loads, a word only where it holds a sample of the utterance), then thread `tid` forms outputs tid + 256 jj -- neighbouring lanes take neighbouring
// phases and (nearly) neighbouring samples: the table reads fall on distinct banks except where the phase wraps (two-way), the sample reads
// step by o / u <= 2 (two-way at most) -- with the taps summed in fp64, and hands them through LDS to the threads that own them.
template <typename P, int V, bool VEC>
__global__ __launch_bounds__(256) void mix_render_speed_kernel(const P* __restrict__ pcm, const int64_t* __restrict__ offsets, const int U, const P* __restrict__ noise_pcm,
                                                               const int64_t* __restrict__ noise_offsets, const int U_noise, const int64_t* __restrict__ plan,
                                                               const float* __restrict__ gain, const int32_t* __restrict__ speed, const int32_t* __restrict__ desc, const int J,
                                                               const float* __restrict__ ftab, const int64_t ntab, const int32_t* __restrict__ ffirst, const int64_t nfirst,
                                                               const int n, const int T, float* __restrict__ sources, float* __restrict__ mixture, float* __restrict__ noise) {
    constexpr int TILE = 256 * V, E = 16 / (int)sizeof(P);
    __shared__ float s_x[MXS_SPAN];
    __shared__ float s_h[MXS_TAB];
    __shared__ int s_first[MXS_PHASES];
    __shared__ __attribute__((aligned(16))) float s_out[TILE];
    const int tid = threadIdx.x;
    const int64_t tile0 = (int64_t)blockIdx.x * TILE, t0 = tile0 + (int64_t)tid * V;
    const int64_t tile_end = tile0 + TILE < T ? tile0 + TILE : T;
    const int64_t b = blockIdx.y;
    const int R = n + (noise ? 1 : 0);
    float acc[V], val[V];
#pragma unroll
    for (int j = 0; j < V; ++j) acc[j] = 0.f;
    for (int i = 0; i < R; ++i) {
        const int64_t e = b * R + i;
        const bool is_noise = i == n;
        int j = is_noise ? -1 : speed[e];
        j = j < -1 ? -1 : j >= J ? J - 1 : j;
        mx_speed sp{1, 1, 0, 1, 0, 0};
        if (j >= 0) sp = mx_read_speed(desc, j);
#pragma unroll
        for (int q = 0; q < V; ++q) val[q] = 0.f;
        if (j < 0 || sp.o == sp.u) {                                                    // (uniform over the workgroup, as everything down to the barriers)
            const mx_row r = is_noise ? mx_read_row(plan + 4 * e, gain[e], noise_offsets, U_noise) : mx_read_row(plan + 4 * e, gain[e], offsets, U);
            if (t0 < T) mx_gather<P, V>(is_noise ? noise_pcm : pcm, r, t0, val);
        } else {
            int64_t uu = plan[4 * e];
            uu = uu < 0 ? 0 : uu >= U ? U - 1 : uu;
            const int64_t o0 = offsets[uu];
            int64_t len = offsets[uu + 1] - o0;
            len = len < 0 ? 0 : len > 0x7fffffff ? 0x7fffffff : len;
            const int64_t lenp = mx_speed_length(sp, len);
            int64_t start = plan[4 * e + 1];
            start = start > lenp - 1 ? lenp - 1 : start;
            start = start < 0 ? 0 : start;
            const int64_t lead = plan[4 * e + 2];
            const uint64_t avail = (uint64_t)(lenp - start);
            const float g = gain[e];
            // the offsets d = t - lead of the tile's samples that lie in the row: [d_lo, d_hi)
            const uint64_t d_lo = lead > tile0 ? 0 : (uint64_t)tile0 - (uint64_t)lead;
            if (lead < tile_end && d_lo < avail) {
                const uint64_t d_end = (uint64_t)tile_end - (uint64_t)lead, d_hi = d_end < avail ? d_end : avail;
                const int o = sp.o, u = sp.u, Kc = sp.Kc;
                const int64_t i_lo = (start + (int64_t)d_lo) / u, i_hi = (start + (int64_t)d_hi - 1) / u;
                const int64_t xb = i_lo * o - sp.width;                                     // the utterance's sample behind s_x[0]
                const int64_t span = (i_hi - i_lo) * o + o + 2 * sp.width;
                const int S = (int)(span > MXS_SPAN ? MXS_SPAN : span);
                // the filter: table[k][p] at s_h[k u + p], first[p]; every global index clamped into the buffers
                for (int q = tid; q < Kc * u; q += 256) {
                    int64_t gi = (int64_t)sp.toff + q;
                    gi = gi < 0 ? 0 : gi > ntab - 1 ? ntab - 1 : gi;
                    s_h[q] = ftab[gi];
                }
                for (int q = tid; q < u; q += 256) {
                    int64_t gi = (int64_t)sp.foff + q;
                    gi = gi < 0 ? 0 : gi > nfirst - 1 ? nfirst - 1 : gi;
                    s_first[q] = mx_clampi(ffirst[gi], 0, MXS_SPAN - 1);
                }
                // the span: s_x[s] = x[xb + s], zero outside [0, len) of this utterance
                const uintptr_t a = (uintptr_t)pcm + sizeof(P) * (uintptr_t)(o0 + xb);
                const int mis = (int)((a & 15) / sizeof(P));
                const uint4* words = reinterpret_cast<const uint4*>(a & ~(uintptr_t)15);
                const int nwords = (S + mis + E - 1) / E;
                for (int w = tid; w < nwords; w += 256) {
                    const int s0 = w * E - mis;
                    const int64_t r0 = xb + s0;
                    uint4 word = make_uint4(0, 0, 0, 0);
                    if (r0 + E > 0 && r0 < len) word = words[w];                            // a word is loaded only where it holds a sample of the utterance
                    const unsigned d[4] = {word.x, word.y, word.z, word.w};
#pragma unroll
                    for (int jj = 0; jj < E; ++jj) {
                        const int s = s0 + jj;
                        const int64_t r = r0 + jj;
                        if (s >= 0 && s < S) s_x[s] = r >= 0 && r < len ? mxs_elem<P>(d, jj) : 0.f;
                    }
                }
                __syncthreads();
#pragma unroll
                for (int jj = 0; jj < V; ++jj) {
                    const int tl = tid + 256 * jj;
                    const int64_t t = tile0 + tl;
                    float v = 0.f;
                    if (t < T && lead <= t && (uint64_t)t - (uint64_t)lead < avail) {
                        const unsigned m = (unsigned)(start + (int64_t)((uint64_t)t - (uint64_t)lead));         // < len' < 2^31
                        const unsigned mi = m / (unsigned)u, p = m - mi * (unsigned)u;
                        const int base = (int)((int64_t)mi - i_lo) * o + s_first[p];
                        double sum = 0.0;
                        for (int k = 0; k < Kc; ++k) {
                            const int idx = base + k < S ? base + k : S - 1;                                    // (only hostile descriptors reach beyond the staged span)
                            sum = __builtin_fma((double)s_h[k * u + (int)p], (double)s_x[idx], sum);            // the product is exact: fused or not, the same bits
                        }
                        v = g * ((float)sum * mx_kind<P>::scale);
                    }
                    s_out[tl] = v;
                }
                __syncthreads();
#pragma unroll
                for (int q = 0; q < V; ++q) val[q] = s_out[tid * V + q];
            }
        }
#pragma unroll
        for (int q = 0; q < V; ++q) acc[q] = i == 0 ? val[q] : acc[q] + val[q];
        float* dst = (is_noise ? noise + b * T : sources + (b * n + i) * T) + t0;
        if constexpr (VEC) {
#pragma unroll
            for (int q = 0; q < V; q += 4)
                if (t0 + q < T) st4(dst + q, make_float4(val[q], val[q + 1], val[q + 2], val[q + 3]));      // T % 4 == 0: a quad is inside or outside
        } else {
#pragma unroll
            for (int q = 0; q < V; ++q)
                if (t0 + q < T) dst[q] = val[q];
        }
    }
    if constexpr (VEC) {
#pragma unroll
        for (int q = 0; q < V; q += 4)
            if (t0 + q < T) st4(mixture + b * T + t0 + q, make_float4(acc[q], acc[q + 1], acc[q + 2], acc[q + 3]));
    } else {
#pragma unroll
        for (int q = 0; q < V; ++q)
            if (t0 + q < T) mixture[b * T + t0 + q] = acc[q];
    }
}

template <typename P, int V, bool VEC>
static void mxs_launch(const void* samples, const int64_t* offsets, int U, const void* noise_samples, const int64_t* noise_offsets, int U_noise, const int64_t* plan,
                       const float* gain, const int32_t* speed, const int32_t* desc, int J, const float* ftab, int64_t ntab, const int32_t* ffirst, int64_t nfirst, int B, int n,
                       int T, float* sources, float* mixture, float* noise, hipStream_t stream) {
    const unsigned gx = (unsigned)(((int64_t)T + 256 * V - 1) / (256 * V));
    hipLaunchKernelGGL((mix_render_speed_kernel<P, V, VEC>), dim3(gx, (unsigned)B), dim3(256), 0, stream, static_cast<const P*>(samples), offsets, U,
                       static_cast<const P*>(noise_samples), noise_offsets, U_noise, plan, gain, speed, desc, J, ftab, ntab, ffirst, nfirst, n, T, sources, mixture, noise);
}

}  // namespace

extern "C" int sep_mix_draw(const int64_t* offsets, const int32_t* spk_first, int U, int S, const int64_t* noise_offsets, int U_noise, const float* level,
                            const float* gain_table, int G, const float* noise_level, const float* noise_gain_table, int G_noise, int64_t* counter, int64_t seed,
                            int64_t item_stride, int64_t item_first, int B, int n, int T, int64_t* plan, float* gain, sep_stream_t stream) {
    SEP_REQUIRE(offsets && spk_first && level && gain_table && counter && plan && gain, "sep_mix_draw: null pointer");
    SEP_REQUIRE(U >= 1 && S >= 1 && S <= U && G >= 1, "sep_mix_draw: bad arguments (U=%d S=%d G=%d; 1 <= S <= U, G >= 1)", U, S, G);
    SEP_REQUIRE(n >= 1 && n <= SEP_MIX_MAX_SOURCES && n <= S, "sep_mix_draw: bad arguments (n=%d S=%d; 1 <= n <= %d sources of distinct speakers, n <= S)", n, S,
                SEP_MIX_MAX_SOURCES);
    SEP_REQUIRE(B >= 1 && B <= 65535 && T >= 1, "sep_mix_draw: bad arguments (B=%d T=%d; 1 <= B <= 65535, 1 <= T < 2^31)", B, T);
    SEP_REQUIRE(!noise_offsets || (U_noise >= 1 && noise_level && noise_gain_table && G_noise >= 1),
                "sep_mix_draw: bad arguments (U_noise=%d G_noise=%d; a noise index needs U_noise >= 1, its levels and a gain table of G_noise >= 1)", U_noise, G_noise);
    hipLaunchKernelGGL(mix_draw_kernel<false>, dim3(1), dim3(256), 0, (hipStream_t)stream, offsets, spk_first, U, S, noise_offsets, U_noise, level, gain_table, G,
                       noise_level, noise_gain_table, G_noise, counter, (uint64_t)seed, (uint64_t)item_stride, (uint64_t)item_first, B, n, T, plan, gain,
                       (const int32_t*)nullptr, 0, (int32_t*)nullptr);
    SEP_CHECK_LAUNCH("sep_mix_draw");
    return 0;
}

extern "C" int sep_mix_render(const void* samples, int kind, const int64_t* offsets, int U, const void* noise_samples, const int64_t* noise_offsets, int U_noise,
                              const int64_t* plan, const float* gain, int B, int n, int T, float* sources, float* mixture, float* noise, sep_stream_t stream) {
    SEP_REQUIRE(samples && offsets && plan && gain && sources && mixture, "sep_mix_render: null pointer");
    SEP_REQUIRE(kind == SEP_MIX_INT16 || kind == SEP_MIX_F32, "sep_mix_render: bad arguments (kind=%d; SEP_MIX_INT16 or SEP_MIX_F32)", kind);
    SEP_REQUIRE(U >= 1 && n >= 1 && n <= SEP_MIX_MAX_SOURCES, "sep_mix_render: bad arguments (U=%d n=%d; U >= 1, 1 <= n <= %d)", U, n, SEP_MIX_MAX_SOURCES);
    SEP_REQUIRE(B >= 1 && B <= 65535 && T >= 1, "sep_mix_render: bad arguments (B=%d T=%d; 1 <= B <= 65535, 1 <= T < 2^31)", B, T);
    const bool any = noise || noise_samples || noise_offsets;
    SEP_REQUIRE(!any || (noise && noise_samples && noise_offsets && U_noise >= 1),
                "sep_mix_render: bad arguments (U_noise=%d; the noise row, the noise samples and the noise index come together or not at all)", U_noise);
    const bool vec = T % 4 == 0 && ((uintptr_t)sources | (uintptr_t)mixture | (uintptr_t)noise) % 16 == 0;
    hipStream_t s = (hipStream_t)stream;
#define SEP_MX(PP, VV, NAME)                                                                                                                       \
    sep_set_kernel(NAME);                                                                                                                          \
    mx_launch<PP, VV>(samples, offsets, U, noise_samples, noise_offsets, U_noise, plan, gain, B, n, T, sources, mixture, noise, s)
    if (kind == SEP_MIX_INT16) {
        if (vec) { SEP_MX(int16_t, 8, "mix_render_vec<int16,8>"); }
        else { SEP_MX(int16_t, 0, "mix_render_scalar<int16>"); }
    } else {
        if (vec) { SEP_MX(float, 4, "mix_render_vec<float,4>"); }
        else { SEP_MX(float, 0, "mix_render_scalar<float>"); }
    }
#undef SEP_MX
    SEP_CHECK_LAUNCH("sep_mix_render");
    return 0;
}

extern "C" int sep_mix_draw_speed(const int64_t* offsets, const int32_t* spk_first, int U, int S, const int64_t* noise_offsets, int U_noise, const float* level,
                                  const float* gain_table, int G, const float* noise_level, const float* noise_gain_table, int G_noise, int64_t* counter, int64_t seed,
                                  int64_t item_stride, int64_t item_first, int B, int n, int T, const int32_t* desc, int J, int64_t* plan, float* gain, int32_t* speed,
                                  sep_stream_t stream) {
    SEP_REQUIRE(offsets && spk_first && level && gain_table && counter && plan && gain && desc && speed, "sep_mix_draw_speed: null pointer");
    SEP_REQUIRE(U >= 1 && S >= 1 && S <= U && G >= 1, "sep_mix_draw_speed: bad arguments (U=%d S=%d G=%d; 1 <= S <= U, G >= 1)", U, S, G);
    SEP_REQUIRE(n >= 1 && n <= SEP_MIX_MAX_SOURCES && n <= S, "sep_mix_draw_speed: bad arguments (n=%d S=%d; 1 <= n <= %d sources of distinct speakers, n <= S)", n, S,
                SEP_MIX_MAX_SOURCES);
    SEP_REQUIRE(B >= 1 && B <= 65535 && T >= 1, "sep_mix_draw_speed: bad arguments (B=%d T=%d; 1 <= B <= 65535, 1 <= T < 2^31)", B, T);
    SEP_REQUIRE(J >= 1 && J <= SEP_MIX_MAX_SPEEDS, "sep_mix_draw_speed: bad arguments (J=%d; 1 <= J <= %d speeds)", J, SEP_MIX_MAX_SPEEDS);
    SEP_REQUIRE(!noise_offsets || (U_noise >= 1 && noise_level && noise_gain_table && G_noise >= 1),
                "sep_mix_draw_speed: bad arguments (U_noise=%d G_noise=%d; a noise index needs U_noise >= 1, its levels and a gain table of G_noise >= 1)", U_noise, G_noise);
    hipLaunchKernelGGL(mix_draw_kernel<true>, dim3(1), dim3(256), 0, (hipStream_t)stream, offsets, spk_first, U, S, noise_offsets, U_noise, level, gain_table, G,
                       noise_level, noise_gain_table, G_noise, counter, (uint64_t)seed, (uint64_t)item_stride, (uint64_t)item_first, B, n, T, plan, gain, desc, J, speed);
    SEP_CHECK_LAUNCH("sep_mix_draw_speed");
    return 0;
}

extern "C" int sep_mix_render_speed(const void* samples, int kind, const int64_t* offsets, int U, const void* noise_samples, const int64_t* noise_offsets, int U_noise,
                                    const int64_t* plan, const float* gain, const int32_t* speed, const int32_t* desc, int J, const float* filter_table,
                                    int64_t table_numel, const int32_t* filter_first, int64_t first_numel, int B, int n, int T, float* sources, float* mixture,
                                    float* noise, sep_stream_t stream) {
    SEP_REQUIRE(samples && offsets && plan && gain && sources && mixture && speed && desc && filter_table && filter_first, "sep_mix_render_speed: null pointer");
    SEP_REQUIRE(kind == SEP_MIX_INT16 || kind == SEP_MIX_F32, "sep_mix_render_speed: bad arguments (kind=%d; SEP_MIX_INT16 or SEP_MIX_F32)", kind);
    SEP_REQUIRE(U >= 1 && n >= 1 && n <= SEP_MIX_MAX_SOURCES, "sep_mix_render_speed: bad arguments (U=%d n=%d; U >= 1, 1 <= n <= %d)", U, n, SEP_MIX_MAX_SOURCES);
    SEP_REQUIRE(B >= 1 && B <= 65535 && T >= 1, "sep_mix_render_speed: bad arguments (B=%d T=%d; 1 <= B <= 65535, 1 <= T < 2^31)", B, T);
    SEP_REQUIRE(J >= 1 && J <= SEP_MIX_MAX_SPEEDS, "sep_mix_render_speed: bad arguments (J=%d; 1 <= J <= %d speeds)", J, SEP_MIX_MAX_SPEEDS);
    SEP_REQUIRE(table_numel >= 1 && table_numel <= (int64_t)SEP_MIX_MAX_SPEEDS * SEP_MIX_SPEED_MAX_TAPS * 100 && first_numel >= 1 && first_numel <= SEP_MIX_MAX_SPEEDS * 100,
                "sep_mix_render_speed: bad arguments (table_numel=%lld first_numel=%lld; 1 .. %d taps and 1 .. %d phases in all)", (long long)table_numel,
                (long long)first_numel, SEP_MIX_MAX_SPEEDS * SEP_MIX_SPEED_MAX_TAPS * 100, SEP_MIX_MAX_SPEEDS * 100);
    const bool any = noise || noise_samples || noise_offsets;
    SEP_REQUIRE(!any || (noise && noise_samples && noise_offsets && U_noise >= 1),
                "sep_mix_render_speed: bad arguments (U_noise=%d; the noise row, the noise samples and the noise index come together or not at all)", U_noise);
    const unsigned esize = kind == SEP_MIX_INT16 ? 2 : 4;
    SEP_REQUIRE((uintptr_t)samples % esize == 0 && (uintptr_t)noise_samples % esize == 0, "sep_mix_render_speed: bad arguments (the samples are not aligned to their own size)");
    const bool vec = T % 4 == 0 && ((uintptr_t)sources | (uintptr_t)mixture | (uintptr_t)noise) % 16 == 0;
    hipStream_t s = (hipStream_t)stream;
#define SEP_MXS(PP, VV, VEC, NAME)                                                                                                                            \
    sep_set_kernel(NAME);                                                                                                                                     \
    mxs_launch<PP, VV, VEC>(samples, offsets, U, noise_samples, noise_offsets, U_noise, plan, gain, speed, desc, J, filter_table, table_numel, filter_first, \
                            first_numel, B, n, T, sources, mixture, noise, s)
    if (kind == SEP_MIX_INT16) {
        if (vec) { SEP_MXS(int16_t, 8, true, "mix_render_speed<int16>"); }
        else { SEP_MXS(int16_t, 8, false, "mix_render_speed_scalar<int16>"); }
    } else {
        if (vec) { SEP_MXS(float, 4, true, "mix_render_speed<float>"); }
        else { SEP_MXS(float, 4, false, "mix_render_speed_scalar<float>"); }
    }
#undef SEP_MXS
    SEP_CHECK_LAUNCH("sep_mix_render_speed");
    return 0;
}
