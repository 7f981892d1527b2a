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

// ONE workgroup; its threads loop over the items.  Every thread reads the step, then the barrier, then one thread stores the increment.
__global__ __launch_bounds__(256) void mix_draw_kernel(const int64_t* __restrict__ offsets, const int32_t* __restrict__ spk_first, const int U, const int S,
                                                       const int64_t* __restrict__ noise_offsets, const int U_noise, const float* __restrict__ level,
                                                       const float* __restrict__ gain_table, const int G, const float* __restrict__ noise_level,
                                                       const float* __restrict__ noise_gain_table, const int G_noise, int64_t* counter, const uint64_t seed,
                                                       const uint64_t item_stride, const uint64_t item_first, const int B, const int n, const int T,
                                                       int64_t* __restrict__ plan, float* __restrict__ gain) {
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
                const int64_t len = mx_length(offsets, U, u);
                const int64_t e = (int64_t)b * R + i;
                mx_place(u, len, T, mx_mix64(key + (uint64_t)(2 * n + i)), mx_mix64(key + (uint64_t)(3 * n + i)), level, gain_table, G, plan + 4 * e, gain + e);
            }
        }
        if (noise_offsets) {
            int64_t u = (int64_t)mx_below(mx_mix64(key + (uint64_t)(4 * n)), (uint64_t)U_noise);
            const int64_t len = mx_length(noise_offsets, U_noise, u);
            const int64_t e = (int64_t)b * R + n;
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
    hipLaunchKernelGGL(mix_draw_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, offsets, spk_first, U, S, noise_offsets, U_noise, level, gain_table, G, noise_level,
                       noise_gain_table, G_noise, counter, (uint64_t)seed, (uint64_t)item_stride, (uint64_t)item_first, B, n, T, plan, gain);
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
