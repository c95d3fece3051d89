// The lattice tile of the two a-trous filters (denoise_kernel, lrt_denoise.hip; svgf_pass_kernel,
// lrt_svgf.hip): its geometry, its staging and the parts of a tap that both take alike. Each
// kernel keeps its arguments, the centre loads it issues ahead of the staging, its colour scale,
// its accumulators and its epilogue.
#pragma once
#include "lrt_internal.h"

// The library is built with -ffp-contract=off (the render units are bit-pinned); the filters are
// not, and their results depend on the a * b + c below being contracted like their own.
#pragma clang fp contract(fast)

namespace lrt {

// The tiled form. A workgroup filters kTileW columns x kTileRows rows that lie s apart (one
// residue class of the rows mod s), so that every tap of its pixels falls on the workgroup's own
// lattice: the LDS tile holds the kTileRows + 4 lattice rows y0 + (r - 2) s and the
// kTileW + 4 s contiguous columns x0 - 2 s .. x0 + kTileW + 2 s - 1 of the pass's input colour
// and the per-tap guides, alphas dropped: 12 floats per pixel as six float2 planes (a wave's tap
// read is 64 consecutive float2 of one plane: ds_read_b64, no bank conflict). Every global access
// is a contiguous run of float4 along a row. At s = 16 the tile is 8 x 128 pixels = 48 KiB;
// 2.1 (s = 1) to 4 (s = 16) pixels are staged per pixel filtered, against 25 read by the direct
// form.
constexpr int kTileW = 64, kTileRows = 4, kTileLds = kTileRows + 4;
constexpr int kPlanes = 6;
constexpr int kTileStage = 4;   // tile pixels staged per thread (tile_slot)
static_assert(kTileLds == 2 * kTileRows, "two lattice rows per thread row");
// a unit's static_assert on its own MAX_ITER: two columns per thread cover the widest tile
constexpr bool tile_covers(int max_iter) { return 4 * (1 << (max_iter - 1)) <= kTileW; }
inline int tile_width(int s) { return kTileW + 4 * s; }
inline size_t tile_bytes(int s) { return sizeof(float2) * kPlanes * kTileLds * (size_t)tile_width(s); }
// The grid of kTileW x kTileRows blocks. blockIdx.y = group * s + phase: the rows y0 + r s,
// r = 0 .. kTileRows - 1 (tile_y0).
inline dim3 tile_grid(int w, int h, int s) {
    const int groups = (h + kTileRows * s - 1) / (kTileRows * s);
    return dim3((unsigned)((w + kTileW - 1) / kTileW), (unsigned)(groups * s));
}

// The taps are branch-free: pixels outside the image and absent guides are staged as zeros and
// an out-of-image tap gets a zero spline weight; the guides are staged divided by their sigma
// (times sqrt(log2 e), so that a tap's weight is one v_exp_f32 of its summed squares).
// world_pos is staged relative to an anchor, the position at the workgroup's first pixel, as
// fma(x, k, -(anchor k)): one rounding, of a value of the size of the tile's extent instead of
// the scene's distance from the origin (x k alone: at 1000 units, sigma_pos 0.5, an ulp of the
// staged value is 4e-4 of a sigma and the weights were off by 5e-5 of the result). The taps take
// differences of staged values, in which the constant cancels, its own rounding included; a
// non-finite component of the anchor counts as 0. No instruction more per staged pixel.
LRT_DEV float finite_or_0(const float v) { return fabsf(v) < INFINITY ? v : 0.0f; }   // (a NaN fails the compare)

// -(anchor k) of the workgroup whose first pixel is (x0, y0), inside the image: a uniform load.
LRT_DEV float3 tile_anchor(const float4* pos, const int w, const int x0, const int y0, const float kx) {
    const float4 an = pos[(size_t)y0 * w + x0];
    return make_float3(finite_or_0(-an.x * kx), finite_or_0(-an.y * kx), finite_or_0(-an.z * kx));
}

// The workgroup's first row (its first column: blockIdx.x * kTileW).
__device__ __forceinline__ int tile_y0(const int s) { return (blockIdx.y / s) * (kTileRows * s) + blockIdx.y % s; }

// Staging. A thread takes kTileStage tile pixels: slot u is lattice row ty + (u >> 1) kTileRows,
// tile column tx + (u & 1) kTileW (past the tile's width below s = 16: such a slot stores nothing).
// Straight-line: every load of every slot is issued, from an address clamped into the image and
// into the tile (the lanes past its width all read its last column), before the first LDS store
// waits for one; what lay outside the image becomes zero afterwards.
LRT_DEV int tile_slot_row(const int u, const int ty) { return ty + (u >> 1) * kTileRows; }
LRT_DEV int tile_slot_col(const int u, const int tx) { return tx + (u & 1) * kTileW; }
// Where slot u is staged from: its global index, clamped, and ok: its pixel is inside the image.
// w, h: the kernel's arguments themselves, by reference: by value they are read ahead of the &&
// chain instead of inside it, the chain is flattened differently and denoise_kernel's registers
// change with it (69 -> 72 VGPRs). svgf_pass_kernel writes these four lines out instead: through
// any form of this function it took 104 VGPRs for 102 and ran 4 % slower.
LRT_DEV size_t tile_slot(const int u, const int tx, const int ty, const int x0, const int y0, const int s,
                         const int tw, const int& w, const int& h, bool& ok) {
    const int lr = tile_slot_row(u, ty), cx = min(tile_slot_col(u, tx), tw - 1);
    const int gy = y0 + (lr - 2) * s, gx = x0 - 2 * s + cx;
    ok = gy >= 0 && gy < h && gx >= 0 && gx < w;
    return (size_t)min(max(gy, 0), h - 1) * w + min(max(gx, 0), w - 1);
}

// A slot's six LDS stores at t = tile + row * tw + col, planes `plane` float2s apart: colour,
// normal / sigma, anchored world_pos / sigma, and the three channels that differ between the
// filters (albedo / sigma, or the variance) as ee * ke where oe. ok: tile_slot's; on, ox: ok and
// the guide is given; ax: tile_anchor's. (The place and the raw ee are the caller's: computed in
// here, or ee passed in scaled and masked, the same stores come out in another order.)
LRT_DEV void tile_store(float2* t, const int plane, const bool ok, const bool on, const bool ox, const bool oe,
                        const float4& cc, const float4& nn, const float4& xx, const float4& ee, const float kn,
                        const float kx, const float3& ax, const float ke) {
    t[0 * plane] = make_float2(ok ? cc.x : 0.0f, ok ? cc.y : 0.0f);
    t[1 * plane] = make_float2(ok ? cc.z : 0.0f, on ? nn.x * kn : 0.0f);
    t[2 * plane] = make_float2(on ? nn.y * kn : 0.0f, on ? nn.z * kn : 0.0f);
    t[3 * plane] = make_float2(ox ? fmaf(xx.x, kx, ax.x) : 0.0f, ox ? fmaf(xx.y, kx, ax.y) : 0.0f);
    t[4 * plane] = make_float2(ox ? fmaf(xx.z, kx, ax.z) : 0.0f, oe ? ee.x * ke : 0.0f);
    t[5 * plane] = make_float2(oe ? ee.y * ke : 0.0f, oe ? ee.z * ke : 0.0f);
}

// The B3-spline weight of tap i of 5 at coordinate g of an axis of n pixels: zero outside the
// image. (n by reference as in tile_slot, and both axes' g computed before either weight: other
// forms change the kernels' code.)
LRT_DEV float tile_spline(const int i, const int g, const int& n) {
    const float hw[5] = {0.0625f, 0.25f, 0.375f, 0.25f, 0.0625f};
    return g >= 0 && g < n ? hw[i] : 0.0f;
}

// e plus the squared normal and world_pos distance of the staged pixels p and q (planes 1.y to
// 4.x), accumulated in this order.
LRT_DEV float tile_guide_dist(float e, const float2 p1, const float2 p2, const float2 p3, const float2 p4,
                              const float2 q1, const float2 q2, const float2 q3, const float2 q4) {
    float d;
    d = p1.y - q1.y, e += d * d;
    d = p2.x - q2.x, e += d * d;
    d = p2.y - q2.y, e += d * d;
    d = p3.x - q3.x, e += d * d;
    d = p3.y - q3.y, e += d * d;
    d = p4.x - q4.x, e += d * d;
    return e;
}

}  // namespace lrt
