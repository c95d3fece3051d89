// The pixel map, the launch grid and the colour store that the one-thread-per-pixel post-process
// kernels share (lrt_temporal, lrt_temporal_gbuffer, lrt_temporal_upsample, lrt_upsample,
// lrt_gbuffer, lrt_gbuffer_chain; lrt_rectify takes the store only). Nothing here multiplies and adds, so the header
// needs no contraction pragma. Every kernel that uses it compiles to the instructions it had with
// these lines in its own text (tools/isa_same.sh).
#pragma once
#include <hip/hip_runtime.h>

namespace lrt {

// A wave covers 8 x 8 pixels and a workgroup of four waves 32 x 8: a streamed access of a wave is
// eight whole 128 B lines, and its gathers stay within about nine rows of the previous state
// whatever the direction of the motion. Timed against waves of 64 x 1 pixels in blocks of 64 x 4
// (the denoiser's shape), alternating in one process: 3 % faster on the orbit, 6 % under a static
// camera. Thread t is lane t % 64 of wave t / 64, at pixel (t % 8, t / 8 % 8) of its wave.
// The kernel tests x < w && y < h itself: returned through references from one function, the map
// changed lrt_temporal.hip's instructions.
constexpr int kPixBlockW = 32, kPixBlockH = 8;
__device__ __forceinline__ int block_x() {
    const int t = threadIdx.x;
    return blockIdx.x * kPixBlockW + (t >> 6) * 8 + (t & 7);
}
__device__ __forceinline__ int block_y() {
    const int t = threadIdx.x;
    return blockIdx.y * kPixBlockH + ((t >> 3) & 7);
}
// The grid of kPixBlockW * kPixBlockH threads that covers w x h pixels.
inline dim3 pixel_grid(int w, int h) {
    return dim3((unsigned)((w + kPixBlockW - 1) / kPixBlockW), (unsigned)((h + kPixBlockH - 1) / kPixBlockH));
}

// The colour of pixel i, 12 B: the alpha stays.
__device__ __forceinline__ void write_rgb(float4* dst, size_t i, const float3 v) {
    float* const o = reinterpret_cast<float*>(dst + i);
    o[0] = v.x;
    o[1] = v.y;
    o[2] = v.z;
}

}  // namespace lrt
