// Firefly restore (lrt_firefly_restore_*, include/lrt.h): the excess that lrt_firefly_* took out of
// each clamped pixel, spread over that pixel's neighbours of the same id with a tent of radius R,
// every source normalised by the weights it actually reaches, and added to a frame. A workgroup
// stages the ids of its pixels plus a halo of 2R, then the normalised excess n = e / W of its pixels
// plus a halo of R as three 4-byte LDS planes; each thread then gathers its (2R + 1)^2 taps in the
// defined order. One launch, no scratch, no atomics. No id is used as an index. No contraction:
// `out` is pinned bit for bit to tests/firefly_restore_ref.py.
#include "lrt_internal.h"

#pragma clang fp contract(off)

namespace lrt {

struct FireflyRestoreArgs {
    const float4* color;
    const float4* excess;
    const int* id;       // or null: every in-image tap matches
    float4* out;         // may be color itself: a thread reads its own quad only
    int w, h;
};

// firefly_kernel's workgroup (lrt_firefly.hip): 32 x 8 pixels, a pixel per thread, a wave two rows
// of 32. Every LDS plane is 4 bytes wide, so each half of a wave reads one tile row at 32
// consecutive words: conflict-free whatever the row pitch is.
constexpr int kFrW = 32, kFrH = 8, kFrThreads = kFrW * kFrH;
constexpr float kFrCap = 0x1p100f;

template <int R>
__global__ __launch_bounds__(kFrThreads) void firefly_restore_kernel(FireflyRestoreArgs a) {
    constexpr int D = 2 * R + 1;
    constexpr int IW = kFrW + 4 * R, IH = kFrH + 4 * R;   // ids: the tile and a halo of 2R
    constexpr int NW = kFrW + 2 * R, NH = kFrH + 2 * R;   // n: the tile and a halo of R
    constexpr int NS = (NW * NH + kFrThreads - 1) / kFrThreads;   // n slots per thread
    __shared__ int tile_id[IH * IW];
    __shared__ float tile_nx[NH * NW], tile_ny[NH * NW], tile_nz[NH * NW];
    const int t = threadIdx.x, lx = t & (kFrW - 1), ly = t / kFrW;
    const int bx = blockIdx.x * kFrW, by = blockIdx.y * kFrH;
    const int x = bx + lx, y = by + ly;
    const bool live = x < a.w && y < a.h;
    // the thread's own quad and the excess of its n slots, issued ahead of the id staging and the
    // barrier; addresses clamped into the image (what an outside slot holds is never counted: below)
    const size_t ip = (size_t)min(y, a.h - 1) * a.w + min(x, a.w - 1);
    const float4 c4 = a.color[ip];
    float4 ex[NS];
#pragma unroll
    for (int k = 0; k < NS; ++k) {
        const int i = min(t + k * kFrThreads, NH * NW - 1);
        const int gx = min(max(bx + i % NW - R, 0), a.w - 1), gy = min(max(by + i / NW - R, 0), a.h - 1);
        ex[k] = a.excess[(size_t)gy * a.w + gx];
    }
    for (int i = t; i < IH * IW; i += kFrThreads) {
        const int gx = min(max(bx + i % IW - 2 * R, 0), a.w - 1), gy = min(max(by + i / IW - 2 * R, 0), a.h - 1);
        tile_id[i] = a.id ? a.id[(size_t)gy * a.w + gx] : 0;
    }
    __syncthreads();
    // Phase 1, steps 1 and 2: n of every slot. A slot outside the image holds zeros and is never
    // counted. A slot whose e is all zero skips the count: its n would be a zero of either sign,
    // and adding a zero to acc (never -0: it starts at +0) changes no bit of it.
#pragma unroll
    for (int k = 0; k < NS; ++k) {
        const int i = t + k * kFrThreads;
        if (i < NH * NW) {
            const int tx = i % NW, ty = i / NW;
            const int gx = bx + tx - R, gy = by + ty - R;
            const bool inside = (unsigned)gx < (unsigned)a.w && (unsigned)gy < (unsigned)a.h;
            const float4 e4 = ex[k];
            // a select: NaN and +-Inf fail the comparison
            const bool ok = inside && __builtin_fabsf(e4.x) <= kFrCap && __builtin_fabsf(e4.y) <= kFrCap &&
                            __builtin_fabsf(e4.z) <= kFrCap;
            float nx = ok ? e4.x : 0.0f, ny = ok ? e4.y : 0.0f, nz = ok ? e4.z : 0.0f;
            if (nx != 0.0f || ny != 0.0f || nz != 0.0f) {
                const int centre = (ty + R) * IW + tx + R;
                const int id = tile_id[centre];
                int W = 0;   // an integer: exact in any order
#pragma unroll
                for (int dy = -R; dy <= R; ++dy) {
                    const int iny = (unsigned)(gy + dy) < (unsigned)a.h;
#pragma unroll
                    for (int dx = -R; dx <= R; ++dx) {
                        const int same = iny & (int)((unsigned)(gx + dx) < (unsigned)a.w) &
                                         (int)(tile_id[centre + dy * IW + dx] == id);
                        W += same * ((R + 1 - (dy < 0 ? -dy : dy)) * (R + 1 - (dx < 0 ? -dx : dx)));
                    }
                }
                const float Wf = (float)W;   // >= (R + 1)^2: the centre counts
                nx = nx / Wf;
                ny = ny / Wf;
                nz = nz / Wf;
            }
            tile_nx[i] = nx;
            tile_ny[i] = ny;
            tile_nz[i] = nz;
        }
    }
    __syncthreads();
    // Phase 2, step 3. The window's columns and rows that lie in the image are lane masks, taken once
    // per thread (0 / 1 words combined with &, as in firefly_kernel). A thread outside the image runs
    // on clamped values and stores nothing.
    int inx[D];
#pragma unroll
    for (int j = 0; j < D; ++j) inx[j] = (unsigned)(x + j - R) < (unsigned)a.w;
    const int id = tile_id[(ly + 2 * R) * IW + lx + 2 * R];
    float ax = 0.0f, ay = 0.0f, az = 0.0f;
#pragma unroll
    for (int dy = 0; dy < D; ++dy) {
        const int iny = (unsigned)(y + dy - R) < (unsigned)a.h;
        const int irow = (ly + R + dy) * IW + lx + R, nrow = (ly + dy) * NW + lx;
#pragma unroll
        for (int dx = 0; dx < D; ++dx) {
            const int same = iny & inx[dx] & (int)(tile_id[irow + dx] == id);
            const float wt = (float)((R + 1 - (dy < R ? R - dy : dy - R)) * (R + 1 - (dx < R ? R - dx : dx - R)));
            // A tap that does not count adds +0 instead of being skipped: acc is finite and never -0,
            // so the sum keeps its bits. Every product is finite (the cap of step 1).
            const float px = wt * tile_nx[nrow + dx], py = wt * tile_ny[nrow + dx], pz = wt * tile_nz[nrow + dx];
            ax = ax + (same ? px : 0.0f);
            ay = ay + (same ? py : 0.0f);
            az = az + (same ? pz : 0.0f);
        }
    }
    // Step 4
    const float inf = __builtin_inff();
    float4 o = c4;
    if (ax != 0.0f && __builtin_fabsf(c4.x) < inf) o.x = c4.x + ax;
    if (ay != 0.0f && __builtin_fabsf(c4.y) < inf) o.y = c4.y + ay;
    if (az != 0.0f && __builtin_fabsf(c4.z) < inf) o.z = c4.z + az;
    if (live) a.out[ip] = o;
}

// Everything that needs neither the library's state nor the device.
static int validate_firefly_restore(const lrt_firefly_restore_desc* d, const float* color, const float* excess,
                                    const int32_t* id, const float* out) {
    if (!d) return fail(LRT_E_INVALID, "desc is NULL");
    if (!color) return fail(LRT_E_INVALID, "color is NULL");
    if (!excess) return fail(LRT_E_INVALID, "excess is NULL");
    if (!out) return fail(LRT_E_INVALID, "out is NULL");
    if (int rc = validate_frame_size(d->width, d->height)) return rc;
    if (d->radius < 1 || d->radius > LRT_FIREFLY_RESTORE_MAX_RADIUS) return fail(LRT_E_INVALID, "radius must be in 1..4");
    if (d->flags != 0) return fail(LRT_E_INVALID, "flags and reserved must be 0");
    for (int32_t r : d->reserved)
        if (r != 0) return fail(LRT_E_INVALID, "flags and reserved must be 0");
    // out may be color itself (a thread reads its own quad only); neighbours of excess and id are read
    const size_t px = (size_t)d->width * d->height, quad = 16 * px, word = 4 * px;
    const Span outs[1] = {{out, quad}}, ins[3] = {{excess, quad}, {id, word}, {out == color ? nullptr : color, quad}};
    if (spans_alias(outs, 1, ins, 3))
        return fail(LRT_E_INVALID, "aliasing: out overlaps an input (only out == color, in place, is allowed)");
    return LRT_OK;
}

// The pass on stream s (device pointers, validated).
static int firefly_restore_device(const lrt_firefly_restore_desc* d, const float* color, const float* excess,
                                  const int32_t* id, float* out, hipStream_t s) {
    FireflyRestoreArgs a;
    memset(&a, 0, sizeof(a));
    a.color = quads(color);
    a.excess = quads(excess);
    a.id = id;
    a.out = quads(out);
    a.w = d->width;
    a.h = d->height;
    const dim3 grid((unsigned)((a.w + kFrW - 1) / kFrW), (unsigned)((a.h + kFrH - 1) / kFrH));
    switch (d->radius) {
        case 1: firefly_restore_kernel<1><<<grid, kFrThreads, 0, s>>>(a); break;
        case 2: firefly_restore_kernel<2><<<grid, kFrThreads, 0, s>>>(a); break;
        case 3: firefly_restore_kernel<3><<<grid, kFrThreads, 0, s>>>(a); break;
        default: firefly_restore_kernel<4><<<grid, kFrThreads, 0, s>>>(a); break;
    }
    LRT_HIP(hipGetLastError());
    return LRT_OK;
}

}  // namespace lrt

using namespace lrt;

extern "C" {

int lrt_firefly_restore_default(int width, int height, lrt_firefly_restore_desc* out) {
    if (int rc = frame_default_begin(out, sizeof(*out), width, height)) return rc;
    out->width = width;
    out->height = height;
    out->radius = 2;
    return LRT_OK;
}

int lrt_firefly_restore_device(const lrt_firefly_restore_desc* desc, const float* d_color, const float* d_excess,
                               const int32_t* d_id, float* d_out, void* stream) {
    RoctxRange rr_("lrt_firefly_restore_device");
    if (int rc = validate_firefly_restore(desc, d_color, d_excess, d_id, d_out)) return rc;
    std::lock_guard<std::mutex> lk(g_mu);
    if (int rc = require_initialized()) return rc;
    DeviceScope ds_(0);   // context 0's device (device 0 of lrt_initialize_devices)
    return firefly_restore_device(desc, d_color, d_excess, d_id, d_out, (hipStream_t)stream);
}

int lrt_firefly_restore_host(const lrt_firefly_restore_desc* desc, const float* color, const float* excess,
                             const int32_t* id, float* out) {
    RoctxRange rr_("lrt_firefly_restore_host");
    if (int rc = validate_firefly_restore(desc, color, excess, id, out)) return rc;
    std::lock_guard<std::mutex> lk(g_mu);
    if (int rc = require_initialized()) return rc;
    DeviceScope ds_(0);
    hipStream_t s = ctx().stream;
    const size_t px = (size_t)desc->width * desc->height, quad = 16 * px, word = 4 * px;
    const bool in_place = out == color;
    HostMirrors m;
    const int excess_ = m.in(excess, quad), id_ = m.in(id, word);
    // in place: one mirror, copied in and back
    const int color_ = in_place ? m.inout(out, quad) : m.in(color, quad);
    const int out_ = in_place ? color_ : m.out(out, quad);
    if (int rc = m.alloc("hipMalloc(firefly restore staging)")) return rc;
    if (int rc = m.upload(s)) return rc;
    if (int rc = firefly_restore_device(desc, m.dev<float>(color_), m.dev<float>(excess_), m.dev<int32_t>(id_),
                                        m.dev<float>(out_), s))
        return rc;
    return m.download(s);
}

}  // extern "C"
