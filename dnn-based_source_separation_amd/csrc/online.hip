// Online (chunk-by-chunk) separation of a CAUSAL Conv-TasNet: the kernels that carry state from one chunk of a stream to the next.
//
// A causal model (reference src/models/conv_tasnet.py:62, causal=True) uses cumulative layer norm and left padding only, so mask frame f
// depends on encoder frames <= f (modules/norm.py:58-101, models/tdcn.py:125-132) and output sample tau of the overlap-add is final once
// every frame with f S <= tau has been seen.  sepkernels/online.py runs a chunk of n frames of every stream as ONE pass over stream-major
// columns -- column j = stream * n + frame of a (C, ldt) matrix, so that each 1x1 product of a layer is one sep_pw_gemm over all streams --
// and these kernels are the pieces of that pass that look back in time:
//   sep_online_encoder_fwd    analysis convolution of [carry | chunk] (filterbank.py:205-235), new carry -> carry_next
//   sep_online_cln_fwd        [PReLU ->] cLN with the fp64 running sums {sum x, sum x^2} of every stream carried in device memory
//   sep_online_depthwise_fwd  causal dilated depthwise taps over [history | chunk], the history of (P - 1) d frames kept in time order
//   sep_online_unfold_fwd     the same history, no taps: the dilated unfold of [history | chunk] for a layer with full k-tap convolutions
//   sep_online_decoder_fwd    mask * w, synthesis and overlap-add into [tail | n S]: n S final samples, new tail -> tail_next
//   sep_online_advance        frame counters += n, carry <- carry_next, tail <- tail_next (the last launch of a chunk)
//   sep_online_reset          zero the state of the streams a device mask selects
//   sep_online_state_export   the whole state of the streams a slot list names -> one packed row each of a caller's blob (format in sepkernels.h)
//   sep_online_state_import   the inverse: rows of a blob -> the state of the named streams (any other separator of the same model structure)
// Every entry point of a chunk has a sibling sep_online_*_sel that takes `const int32_t* slots` (device memory, num_streams distinct entries):
// the pass then has num_streams column blocks and block j works on the state rows of stream slots[j], so a separator with many slots runs
// a chunk of the few that have audio.  Both forms are the same kernel templates; without a slot list block j works on stream j.
// RAGGED.  A third form sep_online_*_rag takes the slot list plus `const int32_t* offs` (device memory, num_streams + 1 increasing entries,
// offs[0] = 0): column block j is [offs[j], offs[j + 1]), so every stream of a pass brings its own number of frames n_j >= 1, and `n` is n_cap,
// the row pitch of chunk / out in hops.  The lengths are read when the kernels run, so a recorded pass replays for other lengths.
// Everything that changes from chunk to chunk (frame counters, running sums, histories, carries, tails) lives in device memory, so a
// recorded chunk step (sep_run_sequence) replays correctly.  No atomics: every result is formed in a fixed order, replays are bitwise.
// State that is read and written by the same launch is owned by ONE workgroup that reads before a barrier and writes after it (cLN sums,
// depthwise histories); the encoder carry and the decoder tail are read by many workgroups and therefore written to a second buffer that
// sep_online_advance copies back.  With a slot list the owner of a stream's state is the workgroup of the column block that names it
// (entries are distinct), and state rows of streams the list does not name are neither read nor written, the second buffers included.
#include "common.hpp"

namespace {

// The stream whose state column block j works on.  SEL is a template argument of every kernel below, so the instance behind the plain
// entry points (SEL = false, slots unused) is the code it was before the slot list existed.
template <bool SEL>
__device__ __forceinline__ int slot_of(const int32_t* __restrict__ slots, const int j) {
    if constexpr (SEL) return slots[j];
    else return j;
}

// The column block that holds column col < offs[blocks]: the largest j with offs[j] <= col (offs increasing, offs[0] = 0).
__device__ __forceinline__ int block_of(const int32_t* __restrict__ offs, const int blocks, const int col) {
    int lo = 0, hi = blocks;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (offs[mid] <= col) lo = mid;
        else hi = mid;
    }
    return lo;
}

// w[nb][s n + f] = [ReLU] sum_k E[nb][k] ext_s[f S + k], ext_s = [carry_s (L - S) | chunk_s (n S)];  columns [num_streams n, ldt) = 0.
// carry_next_s = ext_s[n S .. n S + L - S).  RAG: column block s is [offs[s], offs[s + 1]) with n_s frames, found by a search in offs; row s of chunk
// has the pitch n S and only its first n_s S samples are read.
template <bool SEL, bool RAG>
__global__ __launch_bounds__(256) void online_encoder_kernel(const float* __restrict__ chunk, const float* __restrict__ E, const float* __restrict__ carry,
                                                             float* __restrict__ carry_next, float* __restrict__ w, int num_streams, int L, int S, int n,
                                                             int ldt, int relu, const int32_t* __restrict__ slots, const int32_t* __restrict__ offs) {
    const int nb = blockIdx.y;
    const int col = blockIdx.x * 256 + threadIdx.x;
    const int keep = L - S;
    const int64_t span = (int64_t)n * S;
    int cols;
    if constexpr (RAG) cols = offs[num_streams];
    else cols = num_streams * n;
    if (col < ldt) {
        float acc = 0.f;
        if (col < cols) {
            int s, f;
            if constexpr (RAG) {
                s = block_of(offs, num_streams, col);
                f = col - offs[s];
            } else {
                s = col / n;
                f = col - s * n;
            }
            const float* cs = carry + (size_t)slot_of<SEL>(slots, s) * keep;
            const float* xs = chunk + (size_t)s * span;
            const float* e = E + (size_t)nb * L;
            for (int k = 0; k < L; ++k) {
                const int i = f * S + k;
                const float v = i < keep ? cs[i] : xs[i - keep];
                acc = fmaf(e[k], v, acc);
            }
            if (relu) acc = fmaxf(acc, 0.f);
        }
        w[(size_t)nb * ldt + col] = acc;
    }
    if (nb == 0 && keep > 0) {
        for (int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x; g < (int64_t)num_streams * keep; g += (int64_t)gridDim.x * 256) {
            const int s = (int)(g / keep), i = (int)(g - (int64_t)s * keep);
            int64_t e = span + i;                                         // index into ext_s
            if constexpr (RAG) e = (int64_t)(offs[s + 1] - offs[s]) * S + i;
            const size_t st = (size_t)slot_of<SEL>(slots, s) * keep;
            carry_next[st + i] = e < keep ? carry[st + e] : chunk[(size_t)s * span + (e - keep)];
        }
    }
}

constexpr int OC_TW = 32;         // frames per tile of the cLN pass
constexpr int OC_CG = 8;          // channel groups: 8 x 32 = 256 threads

// One workgroup per stream: tiles of 32 frames, column sums over the channels (fp32 per channel group -> fp64), an inclusive fp64 scan
// over the tile on top of the running sums of everything the stream has seen, then the apply pass over the tile.  count = C (t + 1) with t
// the absolute frame index (frames[s] + f).  The running sums are read by wave 0 at the start and written by lane 0 after the last barrier.
// RAG: the stream's columns are [offs[s], offs[s + 1]), so n differs from workgroup to workgroup (it is uniform inside one: the barriers meet).
template <bool SEL, bool RAG>
__global__ __launch_bounds__(256) void online_cln_kernel(const float* __restrict__ x, const float* __restrict__ alpha, const float* __restrict__ gamma,
                                                         const float* __restrict__ beta, float* __restrict__ y, double* __restrict__ sums, int sums_stride,
                                                         const int64_t* __restrict__ frames, int C, int n, int ldt, float eps,
                                                         const int32_t* __restrict__ slots, const int32_t* __restrict__ offs) {
    __shared__ float red[2][OC_CG][OC_TW];
    __shared__ float mr[2][OC_TW];
    const int s = blockIdx.x, tid = threadIdx.x;
    const int fl = tid & (OC_TW - 1), cg = tid / OC_TW;
    const bool act = alpha != nullptr;
    const float al = act ? alpha[0] : 1.f;
    size_t col0 = (size_t)s * n;
    if constexpr (RAG) {
        col0 = (size_t)offs[s];
        n = offs[s + 1] - offs[s];
    }
    const int st = slot_of<SEL>(slots, s);
    double* sm = sums + (size_t)st * sums_stride;
    double ca = 0.0, cq = 0.0, t0 = 0.0;
    if (tid < 64) {
        ca = sm[0];
        cq = sm[1];
        t0 = (double)frames[st];
    }
    for (int f0 = 0; f0 < n; f0 += OC_TW) {
        const int f = f0 + fl;
        float s1 = 0.f, s2 = 0.f;
        if (f < n) {
            for (int c = cg; c < C; c += OC_CG) {
                float u = x[(size_t)c * ldt + col0 + f];
                if (act) u = prelu_f(u, al);
                s1 += u;
                s2 = fmaf(u, u, s2);
            }
        }
        red[0][cg][fl] = s1;
        red[1][cg][fl] = s2;
        __syncthreads();
        if (tid < 64) {
            double a = 0.0, q = 0.0;
            if (tid < OC_TW) {
#pragma unroll
                for (int g = 0; g < OC_CG; ++g) { a += (double)red[0][g][tid]; q += (double)red[1][g][tid]; }
            }
#pragma unroll
            for (int off = 1; off < OC_TW; off <<= 1) {                 // inclusive prefix over the tile's frames (lanes 32 .. 63 carry zeros)
                const double ua = __shfl_up(a, off, 64), uq = __shfl_up(q, off, 64);
                if (tid >= off) { a += ua; q += uq; }
            }
            const double ta = __shfl(a, OC_TW - 1, 64), tq = __shfl(q, OC_TW - 1, 64);
            if (tid < OC_TW) {
                float mf = 0.f, rf = 0.f;
                if (f0 + tid < n) {
                    const double cnt = (double)C * (t0 + (double)(f0 + tid) + 1.0);
                    const double m = (ca + a) / cnt;
                    double var = (cq + q) / cnt - m * m;
                    if (var < 0.0) var = 0.0;
                    mf = (float)m;
                    rf = (float)(1.0 / (sqrt(var) + (double)eps));
                }
                mr[0][tid] = mf;
                mr[1][tid] = rf;
            }
            ca += ta;
            cq += tq;
        }
        __syncthreads();
        const int nf = n - f0 < OC_TW ? n - f0 : OC_TW;
        for (int e = tid; e < C * OC_TW; e += 256) {
            const int c = e / OC_TW, j = e - c * OC_TW;
            if (j >= nf) continue;
            const size_t idx = (size_t)c * ldt + col0 + f0 + j;
            float u = x[idx];
            if (act) u = prelu_f(u, al);
            y[idx] = (u - mr[0][j]) * mr[1][j] * gamma[c] + beta[c];
        }
        __syncthreads();                                                  // red / mr are rewritten by the next tile
    }
    if (s == (int)gridDim.x - 1) {                                        // the pad columns [num_streams n, ldt) of every row
        int cols = (int)gridDim.x * n;
        if constexpr (RAG) cols = offs[gridDim.x];
        const int pad = ldt - cols;
        for (int64_t e = tid; e < (int64_t)C * pad; e += 256) {
            const int c = (int)(e / pad), j = (int)(e - (int64_t)c * pad);
            y[(size_t)c * ldt + cols + j] = 0.f;
        }
    }
    if (tid == 0) {
        sm[0] = ca;
        sm[1] = cq;
    }
}

// One workgroup per (channel, stream) row: the history is copied to LDS before the barrier, outputs and the new history are formed after
// it from the LDS copy and the (unmodified) input, so a chunk shorter than the history (n < (P - 1) d) cannot race with itself.
// y[f] = bias + sum_k w[k] ext[f + k d], ext = [history ((P - 1) d) | x (n)];  new history = ext[n .. n + (P - 1) d).
// RAG: the row's columns are [offs[s], offs[s + 1]); n_s below and above (P - 1) d may meet in one launch.
template <bool SEL, bool RAG>
__global__ __launch_bounds__(256) void online_depthwise_kernel(const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ bias,
                                                               float* __restrict__ ring, int64_t ring_stride, float* __restrict__ y, int n, int ldt, int P, int d,
                                                               const int32_t* __restrict__ slots, const int32_t* __restrict__ offs) {
    extern __shared__ float hist[];
    const int c = blockIdx.x, s = blockIdx.y, tid = threadIdx.x;
    const int D = (P - 1) * d;
    float* rg = ring + (size_t)slot_of<SEL>(slots, s) * ring_stride + (size_t)c * D;
    size_t col0 = (size_t)s * n;
    if constexpr (RAG) {
        col0 = (size_t)offs[s];
        n = offs[s + 1] - offs[s];
    }
    const float* xr = x + (size_t)c * ldt + col0;
    float* yr = y + (size_t)c * ldt + col0;
    for (int i = tid; i < D; i += 256) hist[i] = rg[i];
    __syncthreads();
    const float b = bias ? bias[c] : 0.f;
    const float* wc = w + (size_t)c * P;
    for (int f = tid; f < n; f += 256) {
        float acc = b;
        for (int k = 0; k < P; ++k) {
            const int e = f + k * d;
            acc = fmaf(wc[k], e < D ? hist[e] : xr[e - D], acc);
        }
        yr[f] = acc;
    }
    for (int i = tid; i < D; i += 256) {
        const int e = n + i;
        rg[i] = e < D ? hist[e] : xr[e - D];
    }
    if (s == (int)gridDim.y - 1) {
        int cols = (int)gridDim.y * n;
        if constexpr (RAG) cols = offs[gridDim.y];
        for (int t = cols + tid; t < ldt; t += 256) y[(size_t)c * ldt + t] = 0.f;
    }
}

// The depthwise kernel without its taps, for a layer whose convolutions are full (separable=False): cols[c P + p][f] = ext[f + p d], the
// dilated unfold of ext = [history | x] over the row index c P + p that makes the layer's (M, C, P) weights the matrix of a 1x1 product.
// Same ownership: workgroup (channel, block) copies the history to LDS before the barrier, writes its P rows of cols and the new history
// after it.  History layout, ring_stride, slot list and offs are the depthwise kernel's.
template <bool SEL, bool RAG>
__global__ __launch_bounds__(256) void online_unfold_kernel(const float* __restrict__ x, float* __restrict__ ring, int64_t ring_stride, float* __restrict__ cols,
                                                            int n, int ldt, int P, int d, const int32_t* __restrict__ slots, const int32_t* __restrict__ offs) {
    extern __shared__ float hist[];
    const int c = blockIdx.x, s = blockIdx.y, tid = threadIdx.x;
    const int D = (P - 1) * d;
    float* rg = ring + (size_t)slot_of<SEL>(slots, s) * ring_stride + (size_t)c * D;
    size_t col0 = (size_t)s * n;
    if constexpr (RAG) {
        col0 = (size_t)offs[s];
        n = offs[s + 1] - offs[s];
    }
    const float* xr = x + (size_t)c * ldt + col0;
    float* cr = cols + (size_t)c * P * ldt + col0;
    for (int i = tid; i < D; i += 256) hist[i] = rg[i];
    __syncthreads();
    for (int g = tid; g < P * n; g += 256) {
        const int p = g / n, f = g - p * n;
        const int e = f + p * d;
        cr[(size_t)p * ldt + f] = e < D ? hist[e] : xr[e - D];
    }
    for (int i = tid; i < D; i += 256) {
        const int e = n + i;
        rg[i] = e < D ? hist[e] : xr[e - D];
    }
    if (s == (int)gridDim.y - 1) {
        int used = (int)gridDim.y * n;
        if constexpr (RAG) used = offs[gridDim.y];
        const int pad = ldt - used;
        for (int g = tid; g < P * pad; g += 256) {
            const int p = g / pad, j = g - p * pad;
            cols[((size_t)c * P + p) * ldt + used + j] = 0.f;
        }
    }
}

// Thread per output sample i of [0, n S + L - S) of (stream, source): the old tail plus the overlap-add of the frames that cover i
// (f S <= i < f S + L), latent = w * mask.  i < n S goes to out, the rest to tail_next.  RAG: the grid covers n_cap S + L - S samples, the stream has
// n_s frames at columns offs[s] ..; its row of out has the pitch n_cap S and is written as zero from n_s S on.
template <bool SEL, bool RAG>
__global__ __launch_bounds__(256) void online_decoder_kernel(const float* __restrict__ w, const float* __restrict__ mask, const float* __restrict__ Dm,
                                                             const float* __restrict__ tail, float* __restrict__ tail_next, float* __restrict__ out,
                                                             int n_src, int N, int L, int S, int n, int ldt, const int32_t* __restrict__ slots,
                                                             const int32_t* __restrict__ offs) {
    const int src = blockIdx.y, s = blockIdx.z;
    const int keep = L - S;
    const int pitch = n * S;                                              // samples per row of out
    size_t col0 = (size_t)s * n;
    if constexpr (RAG) {
        col0 = (size_t)offs[s];
        n = offs[s + 1] - offs[s];
    }
    const int span = n * S;
    const int i = blockIdx.x * 256 + threadIdx.x;
    const size_t row = (size_t)s * n_src + src;
    if constexpr (RAG) {                                                  // a thread with span <= i < span + keep stores this zero AND goes on to the
        if (i >= span && i < pitch) out[row * pitch + i] = 0.f;           // tail below: two different destinations, so the return stays behind the store
    }
    if (i >= span + keep) return;
    const size_t trow = (size_t)slot_of<SEL>(slots, s) * n_src + src;           // the stream's row of tail / tail_next
    float acc = i < keep ? tail[trow * keep + i] : 0.f;
    const int f_hi = (i / S) < n - 1 ? (i / S) : n - 1;
    const int f_lo = i - L + 1 > 0 ? (i - L + S) / S : 0;
    for (int f = f_lo; f <= f_hi; ++f) {
        const int k = i - f * S;
        const size_t col = col0 + f;
        for (int nb = 0; nb < N; ++nb) {
            const float lat = w[(size_t)nb * ldt + col] * mask[((size_t)src * N + nb) * ldt + col];
            acc = fmaf(lat, Dm[(size_t)nb * L + k], acc);
        }
    }
    if (i < span) out[row * pitch + i] = acc;
    else tail_next[trow * keep + (i - span)] = acc;
}

template <bool SEL, bool RAG>
__global__ __launch_bounds__(256) void online_advance_kernel(int64_t* __restrict__ frames, float* __restrict__ carry, const float* __restrict__ carry_next,
                                                             int64_t carry_total, float* __restrict__ tail, const float* __restrict__ tail_next,
                                                             int64_t tail_total, int num_streams, int n, int carry_len, int tail_len,
                                                             const int32_t* __restrict__ slots, const int32_t* __restrict__ offs) {
    if constexpr (SEL) {                                                  // element g of column block g / len -> the same element of its stream's row
        for (int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x; g < carry_total || g < tail_total || g < num_streams; g += (int64_t)gridDim.x * 256) {
            if (g < num_streams) {
                if constexpr (RAG) frames[slots[g]] += offs[g + 1] - offs[g];
                else frames[slots[g]] += n;
            }
            if (g < carry_total) {
                const int64_t j = g / carry_len, e = (int64_t)slots[j] * carry_len + (g - j * carry_len);
                carry[e] = carry_next[e];
            }
            if (g < tail_total) {
                const int64_t j = g / tail_len, e = (int64_t)slots[j] * tail_len + (g - j * tail_len);
                tail[e] = tail_next[e];
            }
        }
        return;
    }
    for (int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x; g < carry_total || g < tail_total || g < num_streams; g += (int64_t)gridDim.x * 256) {
        if (g < num_streams) frames[g] += n;
        if (g < carry_total) carry[g] = carry_next[g];
        if (g < tail_total) tail[g] = tail_next[g];
    }
}

// grid (G, num_streams): the workgroups of a selected stream zero its slice of every state buffer
__global__ __launch_bounds__(256) void online_reset_kernel(const uint8_t* __restrict__ mask, int64_t* __restrict__ frames, float* __restrict__ carry,
                                                           int carry_len, double* __restrict__ sums, int sums_len, float* __restrict__ rings,
                                                           int64_t rings_len, float* __restrict__ tail, int tail_len) {
    const int s = blockIdx.y;
    if (!mask[s]) return;
    const int64_t g0 = (int64_t)blockIdx.x * 256 + threadIdx.x, step = (int64_t)gridDim.x * 256;
    if (g0 == 0) frames[s] = 0;
    for (int64_t g = g0; g < carry_len; g += step) carry[(size_t)s * carry_len + g] = 0.f;
    for (int64_t g = g0; g < sums_len; g += step) sums[(size_t)s * sums_len + g] = 0.0;
    for (int64_t g = g0; g < rings_len; g += step) rings[(size_t)s * rings_len + g] = 0.f;
    for (int64_t g = g0; g < tail_len; g += step) tail[(size_t)s * tail_len + g] = 0.f;
}

// ---- export / import of per-stream state (row format, version 1: include/sepkernels.h) ----
// Byte offsets of the sections of one packed row.  frames and sums are 8-byte words; rings starts on a 16-byte boundary, carry and tail follow
// it without gaps (4-byte words); the row ends on a 16-byte boundary.
struct state_layout {
    int64_t rings, carry, tail, end, row_bytes;
};
__host__ __device__ inline state_layout state_layout_of(int carry_len, int sums_len, int64_t rings_len, int tail_len) {
    state_layout o;
    o.rings = (8 + 8 * (int64_t)sums_len + 15) / 16 * 16;
    o.carry = o.rings + 4 * rings_len;
    o.tail = o.carry + 4 * (int64_t)carry_len;
    o.end = o.tail + 4 * (int64_t)tail_len;
    o.row_bytes = (o.end + 15) / 16 * 16;
    return o;
}

// len 4-byte words src -> dst as INTEGER words (every bit pattern arrives unchanged), thread g0 of `step`.  The access width follows the real
// alignment of BOTH sides: 16 bytes where both are 16-byte aligned (rings with H % 16 == 0, every section at paper size), else 8, else 4; the
// words behind the last whole vector go one by one.  The choice is uniform over a workgroup (it depends on the row only).
__device__ __forceinline__ void state_copy_words(uint32_t* __restrict__ dst, const uint32_t* __restrict__ src, const int64_t len, const int64_t g0,
                                                 const int64_t step) {
    const uintptr_t both = (uintptr_t)dst | (uintptr_t)src;
    int64_t done = 0;
    if ((both & 15) == 0) {
        const int64_t nv = len >> 2;
        for (int64_t g = g0; g < nv; g += step) reinterpret_cast<uint4*>(dst)[g] = reinterpret_cast<const uint4*>(src)[g];
        done = nv << 2;
    } else if ((both & 7) == 0) {
        const int64_t nv = len >> 1;
        for (int64_t g = g0; g < nv; g += step) reinterpret_cast<uint2*>(dst)[g] = reinterpret_cast<const uint2*>(src)[g];
        done = nv << 1;
    }
    for (int64_t g = done + g0; g < len; g += step) dst[g] = src[g];
}

// grid (G, num_streams): the G workgroups of row j share the sections of stream slots[j], each thread its stride of every section.
// IMPORT = false: state -> row j of blob, padding bytes written as zero, nothing beyond row_bytes;  IMPORT = true: row j -> state.
// Every word has one writer and no word is read and written in the same launch (blob and state do not overlap), so no barrier is needed.
template <bool IMPORT>
__global__ __launch_bounds__(256) void online_state_kernel(const int32_t* __restrict__ slots, int64_t* frames, float* carry, int carry_len, double* sums,
                                                           int sums_len, float* rings, int64_t rings_len, float* tail, int tail_len,
                                                           unsigned char* blob, int64_t row_pitch) {
    const int64_t st = slots[blockIdx.y];
    unsigned char* row = blob + (int64_t)blockIdx.y * row_pitch;
    const state_layout lay = state_layout_of(carry_len, sums_len, rings_len, tail_len);
    const int64_t g0 = (int64_t)blockIdx.x * 256 + threadIdx.x, step = (int64_t)gridDim.x * 256;
    uint64_t* head = reinterpret_cast<uint64_t*>(row);                   // [frames | sums_len doubles | zero up to the 16-byte boundary]
    uint64_t* fr = reinterpret_cast<uint64_t*>(frames) + st;
    uint64_t* sm = reinterpret_cast<uint64_t*>(sums) + st * sums_len;
    uint32_t* rg = reinterpret_cast<uint32_t*>(rings) + st * rings_len;
    uint32_t* cr = reinterpret_cast<uint32_t*>(carry) + st * carry_len;
    uint32_t* tl = reinterpret_cast<uint32_t*>(tail) + st * tail_len;
    uint32_t* brg = reinterpret_cast<uint32_t*>(row + lay.rings);
    uint32_t* bcr = reinterpret_cast<uint32_t*>(row + lay.carry);
    uint32_t* btl = reinterpret_cast<uint32_t*>(row + lay.tail);
    if constexpr (IMPORT) {
        if (g0 == 0) fr[0] = head[0];
        for (int64_t g = g0; g < sums_len; g += step) sm[g] = head[1 + g];
        state_copy_words(rg, brg, rings_len, g0, step);
        state_copy_words(cr, bcr, carry_len, g0, step);
        state_copy_words(tl, btl, tail_len, g0, step);
    } else {
        if (g0 == 0) {
            head[0] = fr[0];
            for (int64_t b = 8 + 8 * (int64_t)sums_len; b < lay.rings; b += 8) head[b >> 3] = 0;
            for (int64_t b = lay.end; b < lay.row_bytes; b += 4) *reinterpret_cast<uint32_t*>(row + b) = 0u;
        }
        for (int64_t g = g0; g < sums_len; g += step) head[1 + g] = sm[g];
        state_copy_words(brg, rg, rings_len, g0, step);
        state_copy_words(bcr, cr, carry_len, g0, step);
        state_copy_words(btl, tl, tail_len, g0, step);
    }
}

inline int ceil_div_i(int64_t a, int64_t b) { return (int)((a + b - 1) / b); }

}  // namespace

// The launchers behind the three forms of an entry point: `who` names the caller in its errors, slots == nullptr is the plain form, offs != nullptr
// (with slots) the ragged one, whose n is n_cap.
static int online_encoder(const char* who, const float* chunk, const float* E, const float* carry, float* carry_next, float* w, int num_streams, int N,
                          int L, int S, int n, int ldt, int relu, const int32_t* slots, const int32_t* offs, sep_stream_t stream) {
    SEP_REQUIRE(chunk && E && w && num_streams > 0 && N > 0 && S > 0 && L >= S && L % S == 0 && n > 0, "%s: bad arguments", who);
    SEP_REQUIRE((carry && carry_next) || L == S, "%s: carry buffers missing", who);
    SEP_REQUIRE((int64_t)num_streams * (offs ? 1 : n) <= ldt && ldt % 128 == 0 && N <= 65535, "%s: bad sizes (streams=%d n=%d ldt=%d N=%d)", who,
                num_streams, n, ldt, N);
    const auto kern = offs ? online_encoder_kernel<true, true> : slots ? online_encoder_kernel<true, false> : online_encoder_kernel<false, false>;
    hipLaunchKernelGGL(kern, dim3(ceil_div_i(ldt, 256), N), dim3(256), 0, (hipStream_t)stream, chunk, E, carry, carry_next, w,
                       num_streams, L, S, n, ldt, relu, slots, offs);
    SEP_CHECK_LAUNCH(who);
    return 0;
}

static int online_cln(const char* who, const float* x, const float* alpha, const float* gamma, const float* beta, float* y, double* sums, int sums_stride,
                      const int64_t* frames, int num_streams, int C, int n, int ldt, float eps, const int32_t* slots, const int32_t* offs,
                      sep_stream_t stream) {
    SEP_REQUIRE(x && gamma && beta && y && sums && frames && num_streams > 0 && C > 0 && n > 0 && sums_stride >= 2, "%s: bad arguments", who);
    SEP_REQUIRE(x != y, "%s: y may not alias x", who);
    SEP_REQUIRE((int64_t)num_streams * (offs ? 1 : n) <= ldt && ldt % 128 == 0, "%s: bad sizes (streams=%d n=%d ldt=%d)", who, num_streams, n, ldt);
    const auto kern = offs ? online_cln_kernel<true, true> : slots ? online_cln_kernel<true, false> : online_cln_kernel<false, false>;
    hipLaunchKernelGGL(kern, dim3(num_streams), dim3(256), 0, (hipStream_t)stream, x, alpha, gamma, beta, y, sums, sums_stride, frames,
                       C, n, ldt, eps, slots, offs);
    SEP_CHECK_LAUNCH(who);
    return 0;
}

static int online_depthwise(const char* who, const float* x, const float* w, const float* bias, float* ring, int64_t ring_stride, float* y,
                            int num_streams, int C, int n, int ldt, int P, int dilation, const int32_t* slots, const int32_t* offs,
                            sep_stream_t stream) {
    SEP_REQUIRE(x && w && ring && y && x != y && num_streams > 0 && num_streams <= 65535 && C > 0 && n > 0 && P >= 2 && dilation > 0,
                "%s: bad arguments", who);
    const int64_t D = (int64_t)(P - 1) * dilation;
    SEP_REQUIRE(D <= 16384, "%s: history of %lld frames exceeds LDS", who, (long long)D);
    SEP_REQUIRE(ring_stride >= (int64_t)C * D, "%s: ring_stride %lld < C (P - 1) d", who, (long long)ring_stride);
    SEP_REQUIRE((int64_t)num_streams * (offs ? 1 : n) <= ldt && ldt % 128 == 0, "%s: bad sizes (streams=%d n=%d ldt=%d)", who, num_streams, n, ldt);
    const auto kern = offs ? online_depthwise_kernel<true, true> : slots ? online_depthwise_kernel<true, false> : online_depthwise_kernel<false, false>;
    hipLaunchKernelGGL(kern, dim3(C, num_streams), dim3(256), (size_t)D * sizeof(float), (hipStream_t)stream, x, w, bias, ring,
                       ring_stride, y, n, ldt, P, dilation, slots, offs);
    SEP_CHECK_LAUNCH(who);
    return 0;
}

static int online_unfold(const char* who, const float* x, float* ring, int64_t ring_stride, float* cols, int num_streams, int C, int n, int ldt, int P,
                         int dilation, const int32_t* slots, const int32_t* offs, sep_stream_t stream) {
    SEP_REQUIRE(x && cols && x != cols && num_streams > 0 && num_streams <= 65535 && C > 0 && n > 0 && P >= 1 && dilation > 0, "%s: bad arguments", who);
    const int64_t D = (int64_t)(P - 1) * dilation;
    SEP_REQUIRE(D <= 16384, "%s: history of %lld frames exceeds LDS", who, (long long)D);
    SEP_REQUIRE(ring || D == 0, "%s: ring missing", who);
    SEP_REQUIRE(ring_stride >= (int64_t)C * D, "%s: ring_stride %lld < C (P - 1) d", who, (long long)ring_stride);
    SEP_REQUIRE((int64_t)num_streams * (offs ? 1 : n) <= ldt && ldt % 128 == 0 && (int64_t)P * ldt <= 0x7fffffff, "%s: bad sizes (streams=%d n=%d ldt=%d P=%d)",
                who, num_streams, n, ldt, P);
    const auto kern = offs ? online_unfold_kernel<true, true> : slots ? online_unfold_kernel<true, false> : online_unfold_kernel<false, false>;
    hipLaunchKernelGGL(kern, dim3(C, num_streams), dim3(256), (size_t)D * sizeof(float), (hipStream_t)stream, x, ring, ring_stride, cols, n, ldt, P,
                       dilation, slots, offs);
    SEP_CHECK_LAUNCH(who);
    return 0;
}

static int online_decoder(const char* who, const float* w, const float* mask, const float* D, const float* tail, float* tail_next, float* out,
                          int num_streams, int n_src, int N, int L, int S, int n, int ldt, const int32_t* slots, const int32_t* offs,
                          sep_stream_t stream) {
    SEP_REQUIRE(w && mask && D && out && num_streams > 0 && num_streams <= 65535 && n_src > 0 && n_src <= 65535 && N > 0 && S > 0 && L >= S &&
                L % S == 0 && n > 0, "%s: bad arguments", who);
    SEP_REQUIRE((tail && tail_next) || L == S, "%s: tail buffers missing", who);
    SEP_REQUIRE((int64_t)num_streams * (offs ? 1 : n) <= ldt && ldt % 128 == 0, "%s: bad sizes (streams=%d n=%d ldt=%d)", who, num_streams, n, ldt);
    const auto kern = offs ? online_decoder_kernel<true, true> : slots ? online_decoder_kernel<true, false> : online_decoder_kernel<false, false>;
    hipLaunchKernelGGL(kern, dim3(ceil_div_i((int64_t)n * S + L - S, 256), n_src, num_streams), dim3(256), 0, (hipStream_t)stream, w, mask,
                       D, tail, tail_next, out, n_src, N, L, S, n, ldt, slots, offs);
    SEP_CHECK_LAUNCH(who);
    return 0;
}

static int online_advance(const char* who, int64_t* frames, float* carry, const float* carry_next, int carry_len, float* tail, const float* tail_next,
                          int tail_len, int num_streams, int n, const int32_t* slots, const int32_t* offs, sep_stream_t stream) {
    SEP_REQUIRE(frames && num_streams > 0 && n > 0 && carry_len >= 0 && tail_len >= 0, "%s: bad arguments", who);
    SEP_REQUIRE((carry && carry_next) || carry_len == 0, "%s: carry buffers missing", who);
    SEP_REQUIRE((tail && tail_next) || tail_len == 0, "%s: tail buffers missing", who);
    const int64_t ct = (int64_t)num_streams * carry_len, tt = (int64_t)num_streams * tail_len;
    int64_t most = ct > tt ? ct : tt;
    most = most > num_streams ? most : num_streams;
    const int grid = ceil_div_i(most, 256) > 1024 ? 1024 : ceil_div_i(most, 256);
    const auto kern = offs ? online_advance_kernel<true, true> : slots ? online_advance_kernel<true, false> : online_advance_kernel<false, false>;
    hipLaunchKernelGGL(kern, dim3(grid), dim3(256), 0, (hipStream_t)stream, frames, carry, carry_next, ct, tail, tail_next, tt,
                       num_streams, n, carry_len, tail_len, slots, offs);
    SEP_CHECK_LAUNCH(who);
    return 0;
}

extern "C" int sep_online_encoder_fwd(const float* chunk, const float* E, const float* carry, float* carry_next, float* w, int num_streams, int N,
                                      int L, int S, int n, int ldt, int relu, sep_stream_t stream) {
    return online_encoder("sep_online_encoder_fwd", chunk, E, carry, carry_next, w, num_streams, N, L, S, n, ldt, relu, nullptr, nullptr, stream);
}

extern "C" int sep_online_encoder_fwd_sel(const float* chunk, const float* E, const float* carry, float* carry_next, float* w, int num_streams, int N,
                                          int L, int S, int n, int ldt, int relu, const int32_t* slots, sep_stream_t stream) {
    SEP_REQUIRE(slots, "sep_online_encoder_fwd_sel: slots missing");
    return online_encoder("sep_online_encoder_fwd_sel", chunk, E, carry, carry_next, w, num_streams, N, L, S, n, ldt, relu, slots, nullptr, stream);
}

extern "C" int sep_online_cln_fwd(const float* x, const float* alpha, const float* gamma, const float* beta, float* y, double* sums, int sums_stride,
                                  const int64_t* frames, int num_streams, int C, int n, int ldt, float eps, sep_stream_t stream) {
    return online_cln("sep_online_cln_fwd", x, alpha, gamma, beta, y, sums, sums_stride, frames, num_streams, C, n, ldt, eps, nullptr, nullptr, stream);
}

extern "C" int sep_online_cln_fwd_sel(const float* x, const float* alpha, const float* gamma, const float* beta, float* y, double* sums,
                                      int sums_stride, const int64_t* frames, int num_streams, int C, int n, int ldt, float eps, const int32_t* slots,
                                      sep_stream_t stream) {
    SEP_REQUIRE(slots, "sep_online_cln_fwd_sel: slots missing");
    return online_cln("sep_online_cln_fwd_sel", x, alpha, gamma, beta, y, sums, sums_stride, frames, num_streams, C, n, ldt, eps, slots, nullptr, stream);
}

extern "C" int sep_online_depthwise_fwd(const float* x, const float* w, const float* bias, float* ring, int64_t ring_stride, float* y, int num_streams,
                                        int C, int n, int ldt, int P, int dilation, sep_stream_t stream) {
    return online_depthwise("sep_online_depthwise_fwd", x, w, bias, ring, ring_stride, y, num_streams, C, n, ldt, P, dilation, nullptr, nullptr, stream);
}

extern "C" int sep_online_depthwise_fwd_sel(const float* x, const float* w, const float* bias, float* ring, int64_t ring_stride, float* y,
                                            int num_streams, int C, int n, int ldt, int P, int dilation, const int32_t* slots, sep_stream_t stream) {
    SEP_REQUIRE(slots, "sep_online_depthwise_fwd_sel: slots missing");
    return online_depthwise("sep_online_depthwise_fwd_sel", x, w, bias, ring, ring_stride, y, num_streams, C, n, ldt, P, dilation, slots, nullptr, stream);
}

extern "C" int sep_online_decoder_fwd(const float* w, const float* mask, const float* D, const float* tail, float* tail_next, float* out, int num_streams,
                                      int n_src, int N, int L, int S, int n, int ldt, sep_stream_t stream) {
    return online_decoder("sep_online_decoder_fwd", w, mask, D, tail, tail_next, out, num_streams, n_src, N, L, S, n, ldt, nullptr, nullptr, stream);
}

extern "C" int sep_online_decoder_fwd_sel(const float* w, const float* mask, const float* D, const float* tail, float* tail_next, float* out,
                                          int num_streams, int n_src, int N, int L, int S, int n, int ldt, const int32_t* slots, sep_stream_t stream) {
    SEP_REQUIRE(slots, "sep_online_decoder_fwd_sel: slots missing");
    return online_decoder("sep_online_decoder_fwd_sel", w, mask, D, tail, tail_next, out, num_streams, n_src, N, L, S, n, ldt, slots, nullptr, stream);
}

extern "C" int sep_online_advance(int64_t* frames, float* carry, const float* carry_next, int carry_len, float* tail, const float* tail_next,
                                  int tail_len, int num_streams, int n, sep_stream_t stream) {
    return online_advance("sep_online_advance", frames, carry, carry_next, carry_len, tail, tail_next, tail_len, num_streams, n, nullptr, nullptr, stream);
}

extern "C" int sep_online_advance_sel(int64_t* frames, float* carry, const float* carry_next, int carry_len, float* tail, const float* tail_next,
                                      int tail_len, int num_streams, int n, const int32_t* slots, sep_stream_t stream) {
    SEP_REQUIRE(slots, "sep_online_advance_sel: slots missing");
    return online_advance("sep_online_advance_sel", frames, carry, carry_next, carry_len, tail, tail_next, tail_len, num_streams, n, slots, nullptr, stream);
}

extern "C" int sep_online_encoder_fwd_rag(const float* chunk, const float* E, const float* carry, float* carry_next, float* w, int num_streams, int N,
                                          int L, int S, int n_cap, int ldt, int relu, const int32_t* slots, const int32_t* offs, sep_stream_t stream) {
    SEP_REQUIRE(slots && offs, "sep_online_encoder_fwd_rag: slots / offs missing");
    return online_encoder("sep_online_encoder_fwd_rag", chunk, E, carry, carry_next, w, num_streams, N, L, S, n_cap, ldt, relu, slots, offs, stream);
}

extern "C" int sep_online_cln_fwd_rag(const float* x, const float* alpha, const float* gamma, const float* beta, float* y, double* sums,
                                      int sums_stride, const int64_t* frames, int num_streams, int C, int n_cap, int ldt, float eps,
                                      const int32_t* slots, const int32_t* offs, sep_stream_t stream) {
    SEP_REQUIRE(slots && offs, "sep_online_cln_fwd_rag: slots / offs missing");
    return online_cln("sep_online_cln_fwd_rag", x, alpha, gamma, beta, y, sums, sums_stride, frames, num_streams, C, n_cap, ldt, eps, slots, offs, stream);
}

extern "C" int sep_online_depthwise_fwd_rag(const float* x, const float* w, const float* bias, float* ring, int64_t ring_stride, float* y,
                                            int num_streams, int C, int n_cap, int ldt, int P, int dilation, const int32_t* slots,
                                            const int32_t* offs, sep_stream_t stream) {
    SEP_REQUIRE(slots && offs, "sep_online_depthwise_fwd_rag: slots / offs missing");
    return online_depthwise("sep_online_depthwise_fwd_rag", x, w, bias, ring, ring_stride, y, num_streams, C, n_cap, ldt, P, dilation, slots, offs,
                            stream);
}

extern "C" int sep_online_decoder_fwd_rag(const float* w, const float* mask, const float* D, const float* tail, float* tail_next, float* out,
                                          int num_streams, int n_src, int N, int L, int S, int n_cap, int ldt, const int32_t* slots,
                                          const int32_t* offs, sep_stream_t stream) {
    SEP_REQUIRE(slots && offs, "sep_online_decoder_fwd_rag: slots / offs missing");
    return online_decoder("sep_online_decoder_fwd_rag", w, mask, D, tail, tail_next, out, num_streams, n_src, N, L, S, n_cap, ldt, slots, offs, stream);
}

extern "C" int sep_online_advance_rag(int64_t* frames, float* carry, const float* carry_next, int carry_len, float* tail, const float* tail_next,
                                      int tail_len, int num_streams, int n_cap, const int32_t* slots, const int32_t* offs, sep_stream_t stream) {
    SEP_REQUIRE(slots && offs, "sep_online_advance_rag: slots / offs missing");
    return online_advance("sep_online_advance_rag", frames, carry, carry_next, carry_len, tail, tail_next, tail_len, num_streams, n_cap, slots, offs,
                          stream);
}

extern "C" int sep_online_unfold_fwd(const float* x, float* ring, int64_t ring_stride, float* cols, int num_streams, int C, int n, int ldt, int P,
                                     int dilation, sep_stream_t stream) {
    return online_unfold("sep_online_unfold_fwd", x, ring, ring_stride, cols, num_streams, C, n, ldt, P, dilation, nullptr, nullptr, stream);
}

extern "C" int sep_online_unfold_fwd_sel(const float* x, float* ring, int64_t ring_stride, float* cols, int num_streams, int C, int n, int ldt, int P,
                                         int dilation, const int32_t* slots, sep_stream_t stream) {
    SEP_REQUIRE(slots, "sep_online_unfold_fwd_sel: slots missing");
    return online_unfold("sep_online_unfold_fwd_sel", x, ring, ring_stride, cols, num_streams, C, n, ldt, P, dilation, slots, nullptr, stream);
}

extern "C" int sep_online_unfold_fwd_rag(const float* x, float* ring, int64_t ring_stride, float* cols, int num_streams, int C, int n_cap, int ldt, int P,
                                         int dilation, const int32_t* slots, const int32_t* offs, sep_stream_t stream) {
    SEP_REQUIRE(slots && offs, "sep_online_unfold_fwd_rag: slots / offs missing");
    return online_unfold("sep_online_unfold_fwd_rag", x, ring, ring_stride, cols, num_streams, C, n_cap, ldt, P, dilation, slots, offs, stream);
}

extern "C" int sep_online_reset(const uint8_t* mask, int num_streams, int64_t* frames, float* carry, int carry_len, double* sums, int sums_len,
                                float* rings, int64_t rings_len, float* tail, int tail_len, sep_stream_t stream) {
    SEP_REQUIRE(mask && frames && num_streams > 0 && num_streams <= 65535 && carry_len >= 0 && sums_len >= 0 && rings_len >= 0 && tail_len >= 0,
                "sep_online_reset: bad arguments");
    SEP_REQUIRE((carry || carry_len == 0) && (sums || sums_len == 0) && (rings || rings_len == 0) && (tail || tail_len == 0),
                "sep_online_reset: state buffer missing");
    int64_t most = rings_len;
    if (carry_len > most) most = carry_len;
    if (sums_len > most) most = sums_len;
    if (tail_len > most) most = tail_len;
    const int g = ceil_div_i(most < 1 ? 1 : most, 256);
    hipLaunchKernelGGL(online_reset_kernel, dim3(g > 256 ? 256 : g, num_streams), dim3(256), 0, (hipStream_t)stream, mask, frames, carry, carry_len,
                       sums, sums_len, rings, rings_len, tail, tail_len);
    SEP_CHECK_LAUNCH("sep_online_reset");
    return 0;
}

extern "C" size_t sep_online_state_row_bytes(int carry_len, int sums_len, int64_t rings_len, int tail_len) {
    if (carry_len < 0 || sums_len < 0 || rings_len < 0 || tail_len < 0) return 0;
    return (size_t)state_layout_of(carry_len, sums_len, rings_len, tail_len).row_bytes;
}

// both directions: the checks, then ONE launch of grid (G, num_streams), G workgroups per row with >= 4 16-byte vectors per thread where the row is long
static int online_state(const char* who, bool import, const int32_t* slots, int num_streams, int64_t* frames, float* carry, int carry_len, double* sums,
                        int sums_len, float* rings, int64_t rings_len, float* tail, int tail_len, unsigned char* blob, int64_t row_pitch,
                        sep_stream_t stream) {
    SEP_REQUIRE(slots && frames && blob && num_streams > 0 && num_streams <= 65535 && carry_len >= 0 && sums_len >= 0 && rings_len >= 0 && tail_len >= 0,
                "%s: bad arguments", who);
    SEP_REQUIRE((carry || carry_len == 0) && (sums || sums_len == 0) && (rings || rings_len == 0) && (tail || tail_len == 0), "%s: state buffer missing",
                who);
    const int64_t row_bytes = state_layout_of(carry_len, sums_len, rings_len, tail_len).row_bytes;
    SEP_REQUIRE(row_pitch >= row_bytes, "%s: row_pitch %lld < the %lld bytes of a row", who, (long long)row_pitch, (long long)row_bytes);
    SEP_REQUIRE(row_pitch % 16 == 0, "%s: row_pitch %lld is not a multiple of 16", who, (long long)row_pitch);
    SEP_REQUIRE((uintptr_t)blob % 16 == 0, "%s: blob is not 16-byte aligned", who);
    const int g = ceil_div_i(row_bytes / 16, 256 * 4);
    const auto kern = import ? online_state_kernel<true> : online_state_kernel<false>;
    hipLaunchKernelGGL(kern, dim3(g > 256 ? 256 : g, num_streams), dim3(256), 0, (hipStream_t)stream, slots, frames, carry, carry_len, sums, sums_len,
                       rings, rings_len, tail, tail_len, blob, row_pitch);
    SEP_CHECK_LAUNCH(who);
    return 0;
}

extern "C" int sep_online_state_export(const int32_t* slots, int num_streams, const int64_t* frames, const float* carry, int carry_len,
                                       const double* sums, int sums_len, const float* rings, int64_t rings_len, const float* tail, int tail_len,
                                       void* blob, int64_t row_pitch, sep_stream_t stream) {
    return online_state("sep_online_state_export", false, slots, num_streams, const_cast<int64_t*>(frames), const_cast<float*>(carry), carry_len,
                        const_cast<double*>(sums), sums_len, const_cast<float*>(rings), rings_len, const_cast<float*>(tail), tail_len,
                        static_cast<unsigned char*>(blob), row_pitch, stream);
}

extern "C" int sep_online_state_import(const int32_t* slots, int num_streams, int64_t* frames, float* carry, int carry_len, double* sums, int sums_len,
                                       float* rings, int64_t rings_len, float* tail, int tail_len, const void* blob, int64_t row_pitch,
                                       sep_stream_t stream) {
    return online_state("sep_online_state_import", true, slots, num_streams, frames, carry, carry_len, sums, sums_len, rings, rings_len, tail, tail_len,
                        static_cast<unsigned char*>(const_cast<void*>(blob)), row_pitch, stream);
}
