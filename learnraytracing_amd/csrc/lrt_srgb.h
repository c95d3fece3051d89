// The present step's quantiser (main.cpp:109-115), shared by lrt_frame.hip (lrt_present_bgra8)
// and lrt_tonemap.hip (lrt_tonemap_*): LinearToSRGB of one channel to 0..255 with the glibc-exact
// powf. Bit-pinned: contraction stays off inside it whatever the including unit allows around it.
#pragma once
#include "lrt_trace.h"

namespace lrt {

LRT_DEV uint32_t linear_to_srgb(float x) {   // main.cpp:109-115
#pragma clang fp contract(off)
    x = (x < 0.0f) ? 0.0f : x;                                   // std::max(x, 0.0f)
    x = 1.055f * libm::powf(x, 0.416666667f) - 0.055f;
    x = (x < 0.0f) ? 0.0f : x;                                   // std::max(..., 0.0f)
    uint32_t u = (uint32_t)(x * 255.9f);
    return u < 255u ? u : 255u;                                  // std::min(u, 255u)
}

// b | g << 8 | r << 16 (main.cpp:135-141)
LRT_DEV uint32_t pack_bgra8(float r, float g, float b) {
    return linear_to_srgb(b) | (linear_to_srgb(g) << 8) | (linear_to_srgb(r) << 16);
}

}  // namespace lrt
