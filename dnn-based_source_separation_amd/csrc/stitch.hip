// Stitching the windows of a long recording (continuous speech separation; ABI 23, additive; sepkernels/longform.py).
//
// A non-causal separator is trained on segments of a few seconds and cannot take a meeting in one forward (memory grows with T, gLN statistics
// over minutes, chunk counts outside the trained range).  The recording is cut into W overlapping windows of the trained length `win` at stride
// `hop` (sep_segment), every window is separated on its own, and the n outputs of a window come in an order of their own.  The three kernels here
// undo that order and join the windows: sep_stitch_cost measures every (output of window w, output of window w + 1) pair on the O = win - hop
// samples the two windows share, sep_assign (csrc/assign.hip) matches them, sep_stitch_chain composes the per-boundary matchings into one
// permutation per window relative to the first, sep_stitch_ola cross-fades the aligned windows into n tracks.  win / 2 <= hop < win: a sample
// lies in at most two windows, so the output is a function of at most two inputs and is written once, without a normaliser.  The contract is in
// include/sepkernels.h.  The reference has nothing of the kind.
#include "common.hpp"

namespace {

constexpr int STITCH_MAX_N = SEP_ASSIGN_MAX_N;      // the matching is sep_assign's; a track per lane of one wavefront in the chain
constexpr int CHAIN_BLOCK = 64;                     // windows of perm_local staged in LDS at a time: 64 x 64 ints, 16 KB
static_assert(STITCH_MAX_N == SEP_WAVE, "sep_stitch_chain gives every track a lane of one wavefront");

// cost[b][w][i][j] = sum_{t < O} (est[b][w][i][hop + t] - est[b][w + 1][j][t])^2.  grid (B (W - 1) boundaries, tiles of i x tiles of j): ONE
// workgroup walks the whole overlap of its boundary with an RB x RB tile of pairs in fp64 registers, as pair_gram_kernel holds its products: a
// sample is read ceil(n / RB) times per side, there is no scratch buffer and no second launch.  Per thread the samples are added in ascending
// order, the wave by the butterfly wave_fold (common.hpp), the four waves in order: no atomics, the same bits every time.  A recording has W - 1 boundaries: a
// ten-minute one at 2 s hops launches 299 x ceil(n / 8)^2 workgroups that each walk 16000 samples -- latency-bound by design, and left so: the
// stage stands beside W forwards of the model, which dominate it by orders of magnitude; a slab split over the overlap would
// buy back microseconds at the price of a scratch buffer and a reduction launch.
// VEC: win and hop are multiples of 4 and est is 16-byte aligned, so every row of either side starts on a 16-byte boundary and O is a multiple of
// 4: a thread takes four consecutive samples per step with one 16-byte load per row.  Otherwise one sample per step.
template <int RB, bool VEC>
__global__ __launch_bounds__(256) void stitch_cost_kernel(const float* __restrict__ est, double* __restrict__ cost, const int W, const int n, const int win,
                                                          const int hop) {
    constexpr int NACC = RB * RB;
    __shared__ double red[4][NACC];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int64_t bd = blockIdx.x;                         // b (W - 1) + w
    const int64_t b = bd / (W - 1), w = bd % (W - 1);
    const int nblk = (n + RB - 1) / RB, ra = (blockIdx.y / nblk) * RB, rb = (blockIdx.y % nblk) * RB;
    const int O = win - hop;
    const float* A = est + ((b * W + w) * n) * (int64_t)win + hop;        // row i of window w, from the first shared sample
    const float* C = est + ((b * W + w + 1) * n) * (int64_t)win;          // row j of window w + 1
    const float* pa[RB];
    const float* pc[RB];
#pragma unroll
    for (int i = 0; i < RB; ++i) {                         // rows beyond n enter as zeros and are not stored
        pa[i] = ra + i < n ? A + (int64_t)(ra + i) * win : nullptr;
        pc[i] = rb + i < n ? C + (int64_t)(rb + i) * win : nullptr;
    }
    double acc[NACC];
#pragma unroll
    for (int q = 0; q < NACC; ++q) acc[q] = 0.0;
    if constexpr (VEC) {
        const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int t = 4 * tid; t < O; t += 4 * 256) {       // O % 4 == 0: t + 3 < O
            float4 va[RB], vc[RB];
#pragma unroll
            for (int i = 0; i < RB; ++i) va[i] = pa[i] ? *reinterpret_cast<const float4*>(pa[i] + t) : zero;
#pragma unroll
            for (int i = 0; i < RB; ++i) vc[i] = pc[i] ? *reinterpret_cast<const float4*>(pc[i] + t) : zero;
#pragma unroll
            for (int i = 0; i < RB; ++i)
#pragma unroll
                for (int j = 0; j < RB; ++j) {             // ascending time within the quad
                    double d = (double)va[i].x - (double)vc[j].x;
                    acc[i * RB + j] = fma(d, d, acc[i * RB + j]);
                    d = (double)va[i].y - (double)vc[j].y;
                    acc[i * RB + j] = fma(d, d, acc[i * RB + j]);
                    d = (double)va[i].z - (double)vc[j].z;
                    acc[i * RB + j] = fma(d, d, acc[i * RB + j]);
                    d = (double)va[i].w - (double)vc[j].w;
                    acc[i * RB + j] = fma(d, d, acc[i * RB + j]);
                }
        }
    } else {
        for (int t = tid; t < O; t += 256) {
            double va[RB], vc[RB];
#pragma unroll
            for (int i = 0; i < RB; ++i) va[i] = pa[i] ? (double)pa[i][t] : 0.0;
#pragma unroll
            for (int i = 0; i < RB; ++i) vc[i] = pc[i] ? (double)pc[i][t] : 0.0;
#pragma unroll
            for (int i = 0; i < RB; ++i)
#pragma unroll
                for (int j = 0; j < RB; ++j) {
                    const double d = va[i] - vc[j];
                    acc[i * RB + j] = fma(d, d, acc[i * RB + j]);
                }
        }
    }
    int base = 0;
    wave_fold<NACC, 32>(acc, lane, base);
    constexpr int SHARED = NACC >= 64 ? 0 : 64 / NACC - 1;   // lanes that differ only in these bits hold the same total: one of them stores it
    if ((lane & SHARED) == 0) red[wv][base] = acc[0];
    __syncthreads();
    if (tid < NACC) {
        const int gi = ra + tid / RB, gj = rb + tid % RB;
        if (gi < n && gj < n) cost[(bd * n + gi) * n + gj] = ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid];
    }
}

// perm_abs[b][0][s] = s; perm_abs[b][w + 1][s] = perm_local[b][w][perm_abs[b][w][s]].  One wavefront per recording, lane s; the chain is
// sequential in w, so perm_local goes through LDS CHAIN_BLOCK windows at a time (one coalesced read per block, entries outside [0, n) stored
// as 0) and a step of the chain is an LDS read, not a global-memory round trip.
__global__ __launch_bounds__(64) void stitch_chain_kernel(const int64_t* __restrict__ perm_local, int64_t* __restrict__ perm_abs, const int W, const int n) {
    __shared__ int stage[CHAIN_BLOCK * STITCH_MAX_N];
    const int lane = threadIdx.x;
    const int64_t b = blockIdx.x;
    const int64_t* pl = perm_local + b * (int64_t)(W - 1) * n;
    int64_t* pa = perm_abs + b * (int64_t)W * n;
    int cur = lane < n ? lane : 0;
    if (lane < n) pa[lane] = cur;
    for (int w0 = 0; w0 < W - 1; w0 += CHAIN_BLOCK) {
        const int cnt = W - 1 - w0 < CHAIN_BLOCK ? W - 1 - w0 : CHAIN_BLOCK;
        for (int e = lane; e < cnt * n; e += 64) {
            const int64_t v = pl[(int64_t)w0 * n + e];
            stage[e] = v < 0 || v >= n ? 0 : (int)v;
        }
        __syncthreads();
        for (int k = 0; k < cnt; ++k) {
            cur = stage[k * n + cur];
            if (lane < n) pa[(int64_t)(w0 + k + 1) * n + lane] = cur;
        }
        __syncthreads();
    }
}

// the window and the row of that window behind track s at sample position (w, k): an entry of perm_abs outside [0, n) is read as 0
__device__ __forceinline__ const float* stitch_row(const float* __restrict__ est, const int64_t* __restrict__ perm_abs, const int64_t b, const int W, const int n,
                                                   const int win, const int w, const int s) {
    const int64_t p = perm_abs[(b * W + w) * n + s];
    const int r = p < 0 || p >= n ? 0 : (int)p;
    return est + ((b * W + w) * n + r) * (int64_t)win;
}

// out[b][s][t]: w = min(t / hop, W - 1), k = t - w hop; inside the overlap with the window before (w >= 1, k < O) the cross-fade
// a + g (c - a), g = (k + 0.5) / O, in fp32, of a = est[b][w - 1][perm_abs[b][w - 1][s]][hop + k] and c = est[b][w][perm_abs[b][w][s]][k];
// elsewhere a copy of c.  grid (ceil(T / 1024), n, B), a thread four samples: output-stationary, every element written once.
// VEC: win, hop and T are multiples of 4 and est, out are 16-byte aligned: the four samples are consecutive, lie in one window and on one side
// of the overlap's end, and move as 16-byte loads and one 16-byte store.  Otherwise sample by sample, a wave on consecutive addresses.
template <bool VEC>
__global__ __launch_bounds__(256) void stitch_ola_kernel(const float* __restrict__ est, const int64_t* __restrict__ perm_abs, float* __restrict__ out, const int W,
                                                         const int n, const int win, const int hop, const int T) {
    const int s = blockIdx.y, tid = threadIdx.x;
    const int64_t b = blockIdx.z;
    const int O = win - hop;
    const float fo = (float)O;
    float* o = out + (b * n + s) * (int64_t)T;
    if constexpr (VEC) {
        const int64_t t = (int64_t)blockIdx.x * 1024 + 4 * tid;
        if (t >= T) return;                                 // T % 4 == 0: t + 3 < T
        const int w = t / hop < W - 1 ? (int)(t / hop) : W - 1, k = (int)(t - (int64_t)w * hop);
        const float4 c = *reinterpret_cast<const float4*>(stitch_row(est, perm_abs, b, W, n, win, w, s) + k);
        if (w >= 1 && k < O) {
            const float4 a = *reinterpret_cast<const float4*>(stitch_row(est, perm_abs, b, W, n, win, w - 1, s) + hop + k);
            float4 r;
            r.x = a.x + ((float)k + 0.5f) / fo * (c.x - a.x);
            r.y = a.y + ((float)(k + 1) + 0.5f) / fo * (c.y - a.y);
            r.z = a.z + ((float)(k + 2) + 0.5f) / fo * (c.z - a.z);
            r.w = a.w + ((float)(k + 3) + 0.5f) / fo * (c.w - a.w);
            *reinterpret_cast<float4*>(o + t) = r;
        } else {
            *reinterpret_cast<float4*>(o + t) = c;
        }
    } else {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int64_t t = (int64_t)blockIdx.x * 1024 + q * 256 + tid;
            if (t >= T) return;
            const int w = t / hop < W - 1 ? (int)(t / hop) : W - 1, k = (int)(t - (int64_t)w * hop);
            const float c = stitch_row(est, perm_abs, b, W, n, win, w, s)[k];
            if (w >= 1 && k < O) {
                const float a = stitch_row(est, perm_abs, b, W, n, win, w - 1, s)[hop + k];
                o[t] = a + ((float)k + 0.5f) / fo * (c - a);
            } else {
                o[t] = c;
            }
        }
    }
}

// what the calls ask of the shape and of the window geometry; every offset into est is 64-bit
static bool stitch_shape_ok(const int B, const int W, const int n) { return B >= 1 && W >= 1 && n >= 1 && n <= STITCH_MAX_N; }
static bool stitch_windows_ok(const int W, const int win, const int hop) {
    return win >= 2 && win <= (1 << 30) && hop < win && 2 * (int64_t)hop >= win;
}
static bool stitch_aligned(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

extern "C" int sep_stitch_cost(const float* est, double* cost, int B, int W, int n, int win, int hop, sep_stream_t stream) {
    SEP_REQUIRE(est && (cost || W == 1), "sep_stitch_cost: null pointer");
    SEP_REQUIRE(stitch_shape_ok(B, W, n) && stitch_windows_ok(W, win, hop) && (int64_t)B * (W - 1) <= 0x7fffffff,
                "sep_stitch_cost: bad arguments (B=%d W=%d n=%d win=%d hop=%d; B, W >= 1, 1 <= n <= %d, win / 2 <= hop < win, B (W - 1) < 2^31)", B, W, n, win, hop,
                STITCH_MAX_N);
    if (W == 1) return 0;                                   // no boundary: nothing to launch
    const bool vec = win % 4 == 0 && hop % 4 == 0 && stitch_aligned(est);
    const unsigned nbd = (unsigned)((int64_t)B * (W - 1));
    if (n <= 4) {
        if (vec) hipLaunchKernelGGL((stitch_cost_kernel<4, true>), dim3(nbd, 1), dim3(256), 0, (hipStream_t)stream, est, cost, W, n, win, hop);
        else hipLaunchKernelGGL((stitch_cost_kernel<4, false>), dim3(nbd, 1), dim3(256), 0, (hipStream_t)stream, est, cost, W, n, win, hop);
    } else {
        const int nblk = ceil_div(n, 8);
        if (vec) hipLaunchKernelGGL((stitch_cost_kernel<8, true>), dim3(nbd, (unsigned)(nblk * nblk)), dim3(256), 0, (hipStream_t)stream, est, cost, W, n, win, hop);
        else hipLaunchKernelGGL((stitch_cost_kernel<8, false>), dim3(nbd, (unsigned)(nblk * nblk)), dim3(256), 0, (hipStream_t)stream, est, cost, W, n, win, hop);
    }
    SEP_CHECK_LAUNCH("sep_stitch_cost");
    return 0;
}

extern "C" int sep_stitch_chain(const int64_t* perm_local, int64_t* perm_abs, int B, int W, int n, sep_stream_t stream) {
    SEP_REQUIRE(perm_abs && (perm_local || W == 1), "sep_stitch_chain: null pointer");
    SEP_REQUIRE(stitch_shape_ok(B, W, n), "sep_stitch_chain: bad arguments (B=%d W=%d n=%d; B, W >= 1, 1 <= n <= %d)", B, W, n, STITCH_MAX_N);
    hipLaunchKernelGGL(stitch_chain_kernel, dim3((unsigned)B), dim3(64), 0, (hipStream_t)stream, perm_local, perm_abs, W, n);
    SEP_CHECK_LAUNCH("sep_stitch_chain");
    return 0;
}

extern "C" int sep_stitch_ola(const float* est, const int64_t* perm_abs, float* out, int B, int W, int n, int win, int hop, int T, sep_stream_t stream) {
    SEP_REQUIRE(est && perm_abs && out, "sep_stitch_ola: null pointer");
    SEP_REQUIRE(stitch_shape_ok(B, W, n) && B <= 65535 && stitch_windows_ok(W, win, hop) && T >= 1 && (int64_t)(W - 1) * hop + win >= T,
                "sep_stitch_ola: bad arguments (B=%d W=%d n=%d win=%d hop=%d T=%d; 1 <= B <= 65535, W >= 1, 1 <= n <= %d, win / 2 <= hop < win, "
                "1 <= T <= (W - 1) hop + win)", B, W, n, win, hop, T, STITCH_MAX_N);
    const dim3 grid((unsigned)(((int64_t)T + 1023) / 1024), (unsigned)n, (unsigned)B);
    if (win % 4 == 0 && hop % 4 == 0 && T % 4 == 0 && stitch_aligned(est) && stitch_aligned(out))
        hipLaunchKernelGGL((stitch_ola_kernel<true>), grid, dim3(256), 0, (hipStream_t)stream, est, perm_abs, out, W, n, win, hop, T);
    else
        hipLaunchKernelGGL((stitch_ola_kernel<false>), grid, dim3(256), 0, (hipStream_t)stream, est, perm_abs, out, W, n, win, hop, T);
    SEP_CHECK_LAUNCH("sep_stitch_ola");
    return 0;
}
