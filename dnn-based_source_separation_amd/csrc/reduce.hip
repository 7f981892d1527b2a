// The deterministic second stages of the split reductions for gfx950: every kernel that sums over (sample, frame) columns writes one partial
// per slab or per workgroup, and these add the partials in a fixed order, bit-stable run to run.
//
//   dst[i] (+)= scale * sum_s src[s * stride + i]     (sep_reduce_slabs: the slabs of the weight gradients of wgrad.hip, wgrad_pc.hip and
//                                                      wgrad_pc16.hip, of the dense layers of linear.hip, of the gLN paths, the recorded step)
//   dst[i] (+)= (float)src[i]                         (sep_f64_to_f32: scalar gradients accumulated in double, e.g. PReLU slopes)
//
// No counterpart in the reference, where each of these gradients is one ATen reduction whose summation order is the library's.
//
// Kernels of this file:
//   reduce_slabs_kernel           up to 64 segments per launch, two forms per segment (notes at the kernel)
//   f64_to_f32_kernel             one thread per value
#include "common.hpp"

namespace {

constexpr int RMAXSEG = 64;
struct ReduceArgs {
    sep_reduce_seg seg[RMAXSEG];
    int blk_start[RMAXSEG + 1];
    unsigned char phased[RMAXSEG];      // 1: 64 outputs per workgroup, four slab phases per output
    int nseg;
};

// Two forms per segment, both with a fixed summation order (bit-stable run to run).  Launches that stream (the Conv-TasNet step's batched weight
// gradients: dozens of segments of 64 - 128 slabs of 64 K ... 128 K values, 0.5 GB per launch) keep one thread per output and four chains.  Short ones -- the
// dual-path models' dense layers: 170 slabs of 12 K values took 20 us, latency, 54 launches per DPTNet step -- get 64 outputs per
// workgroup and four threads per output: thread (i, g) adds the slabs k = g, g + 4, ... in four chains of its own (sixteen loads in flight
// per output), the four phases meet in LDS.
__global__ __launch_bounds__(256) void reduce_slabs_kernel(const ReduceArgs a) {
    __shared__ float ph[4][64];
    int sgi = 0;
    while (sgi + 1 < a.nseg && (int)blockIdx.x >= a.blk_start[sgi + 1]) ++sgi;
    const sep_reduce_seg sg = a.seg[sgi];
    if (!a.phased[sgi]) {
        const int i = ((int)blockIdx.x - a.blk_start[sgi]) * 256 + threadIdx.x;
        if (i >= sg.n) return;
        float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
        int k = 0;
        for (; k + 3 < sg.nslab; k += 4) {
            s0 += sg.src[(size_t)(k + 0) * sg.stride + i];
            s1 += sg.src[(size_t)(k + 1) * sg.stride + i];
            s2 += sg.src[(size_t)(k + 2) * sg.stride + i];
            s3 += sg.src[(size_t)(k + 3) * sg.stride + i];
        }
        for (; k < sg.nslab; ++k) s0 += sg.src[(size_t)k * sg.stride + i];
        float v = ((s0 + s1) + (s2 + s3)) * sg.scale;
        if (sg.accumulate) v += sg.dst[i];
        sg.dst[i] = v;
        return;
    }
    const int g = threadIdx.x >> 6, li = threadIdx.x & 63;
    const int i = ((int)blockIdx.x - a.blk_start[sgi]) * 64 + li;
    float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
    if (i < sg.n) {
        int k = g;
        for (; k + 12 < sg.nslab; k += 16) {
            s0 += sg.src[(size_t)(k + 0) * sg.stride + i];
            s1 += sg.src[(size_t)(k + 4) * sg.stride + i];
            s2 += sg.src[(size_t)(k + 8) * sg.stride + i];
            s3 += sg.src[(size_t)(k + 12) * sg.stride + i];
        }
        for (; k < sg.nslab; k += 4) s0 += sg.src[(size_t)k * sg.stride + i];
    }
    ph[g][li] = (s0 + s1) + (s2 + s3);
    __syncthreads();
    if (g == 0 && i < sg.n) {
        float v = ((ph[0][li] + ph[1][li]) + (ph[2][li] + ph[3][li])) * sg.scale;
        if (sg.accumulate) v += sg.dst[i];
        sg.dst[i] = v;
    }
}

__global__ void f64_to_f32_kernel(const double* src, float* dst, int n, int accumulate) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) dst[i] = (accumulate ? dst[i] : 0.f) + (float)src[i];
}

}  // namespace

extern "C" int sep_reduce_slabs(const sep_reduce_seg* segs, int nseg, sep_stream_t stream) {
    SEP_REQUIRE(segs && nseg >= 1 && nseg <= RMAXSEG, "sep_reduce_slabs: 1..64 segments per launch (got %d)", nseg);
    ReduceArgs a;
    int blocks = 0;
    double launch_bytes = 0.0;                       // a launch that moves more than this streams: one thread per output is the faster form there
    for (int i = 0; i < nseg; ++i) launch_bytes += 4.0 * (double)segs[i].n * (double)segs[i].nslab;
    const bool streams = launch_bytes > 64e6;
    for (int i = 0; i < nseg; ++i) {
        SEP_REQUIRE(segs[i].src && segs[i].dst && segs[i].n > 0 && segs[i].nslab > 0, "sep_reduce_slabs: bad segment %d", i);
        a.seg[i] = segs[i];
        a.blk_start[i] = blocks;
        a.phased[i] = !streams && segs[i].nslab >= 16;
        blocks += ceil_div(segs[i].n, a.phased[i] ? 64 : 256);
    }
    a.blk_start[nseg] = blocks;
    a.nseg = nseg;
    hipLaunchKernelGGL(reduce_slabs_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, a);
    SEP_CHECK_LAUNCH("sep_reduce_slabs");
    return 0;
}

extern "C" int sep_f64_to_f32(const double* src, float* dst, int n, int accumulate, sep_stream_t stream) {
    SEP_REQUIRE(src && dst && n > 0, "sep_f64_to_f32: bad arguments");
    hipLaunchKernelGGL(f64_to_f32_kernel, dim3(ceil_div(n, 256)), dim3(256), 0, (hipStream_t)stream, src, dst, n, accumulate);
    SEP_CHECK_LAUNCH("sep_f64_to_f32");
    return 0;
}
