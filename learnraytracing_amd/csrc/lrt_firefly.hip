// Firefly suppression (lrt_firefly_*, include/lrt.h): a rank-order clamp of each pixel's luminance
// against its neighbours of the same id, ahead of the temporal stages. A workgroup stages the
// luminance and the id of its pixels plus a halo of `radius` into two 4-byte LDS planes -- a
// luminance that cannot count (not finite) is already -inf there -- and each thread then runs its
// window through a branch-free insertion chain that keeps the `rank` largest values in registers.
// One launch, no scratch; the only atomics are the two info words, one each per workgroup, behind a
// ballot count per wave and a sum over the waves, and only when info is given. No id is used as an
// index. No contraction: every output is pinned bit for bit to tests/firefly_ref.py.
#include "lrt_internal.h"

#pragma clang fp contract(off)

namespace lrt {

struct FireflyArgs {
    const float4* in;
    const int* id;       // or null: every in-image tap matches
    float4* out;
    float4* excess;      // or null
    int* cls;            // or null
    unsigned* info;      // or null: two words, zeroed on the stream ahead of the launch
    int w, h, min_taps;
    float gain, floor;
};

// A workgroup covers 32 x 8 pixels, a pixel per thread; a wave covers two rows of 32. A 4-byte LDS
// access is served in two halves of 32 lanes over 32 banks: each half is one row of the tile at 32
// consecutive words, so reads and the staging writes are conflict-free whatever the row pitch is.
constexpr int kFfW = 32, kFfH = 8, kFfWaves = kFfW * kFfH / 64;

// lrt_sample_budget.hip's expression
__device__ __forceinline__ float firefly_luma(const float4 c) { return (0.2126f * c.x + 0.7152f * c.y) + 0.0722f * c.z; }

template <int R, int K>
__global__ __launch_bounds__(kFfW* kFfH) void firefly_kernel(FireflyArgs a) {
    constexpr int TW = kFfW + 2 * R, TH = kFfH + 2 * R, D = 2 * R + 1;
    __shared__ float tile_y[TH * TW];
    __shared__ int tile_id[TH * TW];
    __shared__ unsigned part[2][kFfWaves];
    const float ninf = -__builtin_inff();
    const int t = threadIdx.x, lx = t & (kFfW - 1), ly = t / kFfW;
    const int bx = blockIdx.x * kFfW, by = blockIdx.y * kFfH;
    const int x = bx + lx, y = by + ly;
    const bool live = x < a.w && y < a.h;
    // the thread's own quad, issued ahead of the staging loads and the barrier
    const size_t ip = (size_t)min(y, a.h - 1) * a.w + min(x, a.w - 1);
    const float4 c4 = a.in[ip];
    // the tile: addresses clamped into the image (what an outside slot holds is never counted: below)
    for (int i = t; i < TH * TW; i += kFfW * kFfH) {
        const int tx = i % TW, ty = i / TW;
        const int gx = min(max(bx + tx - R, 0), a.w - 1), gy = min(max(by + ty - R, 0), a.h - 1);
        const size_t iq = (size_t)gy * a.w + gx;
        const float yq = firefly_luma(a.in[iq]);
        tile_y[i] = __builtin_fabsf(yq) < __builtin_inff() ? yq : ninf;
        tile_id[i] = a.id ? a.id[iq] : 0;
    }
    __syncthreads();
    // Step 1. Every int32 is a legal id, so the window's columns and rows that lie in the image are
    // lane masks, taken once per thread (0 / 1 words combined with &, as in rectify_kernel). A thread
    // outside the image runs on clamped values and stores nothing.
    int inx[D];
#pragma unroll
    for (int j = 0; j < D; ++j) inx[j] = (unsigned)(x + j - R) < (unsigned)a.w;
    const int id = tile_id[(ly + R) * TW + lx + R];
    int m = 0;
    float top[K];   // the K largest so far, descending (registers: every index is a constant)
#pragma unroll
    for (int k = 0; k < K; ++k) top[k] = ninf;
#pragma unroll
    for (int dy = 0; dy < D; ++dy) {
        const int iny = (unsigned)(y + dy - R) < (unsigned)a.h;
        const int row = (ly + dy) * TW + lx;
#pragma unroll
        for (int dx = 0; dx < D; ++dx) {
            if (dy == R && dx == R) continue;   // the centre is excluded
            const float yq = tile_y[row + dx];
            const int same = iny & inx[dx] & (int)(tile_id[row + dx] == id);
            // a select: a tap that does not count is -inf whatever it holds
            float v = same ? yq : ninf;
            m += (int)(v != ninf);
#pragma unroll
            for (int k = 0; k < K; ++k) {
                const float hi = fmaxf(top[k], v);
                if (k + 1 < K) v = fminf(top[k], v);
                top[k] = hi;
            }
        }
    }
    // Steps 2 to 4
    const float T = a.gain * fmaxf(top[K - 1], 0.0f) + a.floor;
    const float yc = firefly_luma(c4);
    const bool supported = m >= a.min_taps, finite = __builtin_fabsf(yc) < __builtin_inff();
    const int cls = !supported ? 2 : !finite ? 3 : yc > T ? 1 : 0;
    const float s = T / yc;
    float4 o = c4, e = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (cls == 1) {
        o = make_float4(s * c4.x, s * c4.y, s * c4.z, c4.w);
        e = make_float4(c4.x - o.x, c4.y - o.y, c4.z - o.z, 0.0f);
    } else if (cls == 3) {
        o = make_float4(T, T, T, c4.w);
    }
    if (live) {
        a.out[ip] = o;
        if (a.excess) a.excess[ip] = e;
        if (a.cls) a.cls[ip] = cls;
    }
    if (a.info) {   // (the same in every thread)
        const unsigned n1 = (unsigned)__popcll(__ballot(live && cls == 1));
        const unsigned n3 = (unsigned)__popcll(__ballot(live && cls == 3));
        if ((t & 63) == 0) {
            part[0][t >> 6] = n1;
            part[1][t >> 6] = n3;
        }
        __syncthreads();
        if (t < 2) {
            unsigned n = 0;
            for (int wv = 0; wv < kFfWaves; ++wv) n += part[t][wv];
            if (n) atomicAdd(a.info + t, n);
        }
    }
}

// Everything that needs neither the library's state nor the device.
static int validate_firefly(const lrt_firefly_desc* d, const float* in, const int32_t* id, const float* out,
                            const float* excess, const int32_t* cls, const uint32_t* info) {
    if (!d) return fail(LRT_E_INVALID, "desc is NULL");
    if (!in) return fail(LRT_E_INVALID, "in is NULL");
    if (!out) return fail(LRT_E_INVALID, "out is NULL");
    if (int rc = validate_frame_size(d->width, d->height)) return rc;
    if (d->radius < 1 || d->radius > LRT_FIREFLY_MAX_RADIUS) return fail(LRT_E_INVALID, "radius must be in 1..2");
    if (d->rank < 1 || d->rank > 4) return fail(LRT_E_INVALID, "rank must be in 1..4");
    const int side = 2 * d->radius + 1;
    if (d->min_taps < d->rank || d->min_taps > side * side - 1)
        return fail(LRT_E_INVALID, "min_taps must be in rank..(2 radius + 1)^2 - 1");
    if (d->flags != 0) return fail(LRT_E_INVALID, "flags and reserved must be 0");
    for (int32_t r : d->reserved)
        if (r != 0) return fail(LRT_E_INVALID, "flags and reserved must be 0");
    for (float v : {d->gain, d->floor})
        if (!std::isfinite(v) || !(v > 0.0f)) return fail(LRT_E_INVALID, "gain and floor must be finite and > 0");
    // neighbours are read: not in place either
    const size_t px = (size_t)d->width * d->height, quad = 16 * px, word = 4 * px;
    const Span outs[4] = {{out, quad}, {excess, quad}, {cls, word}, {info, 8}}, ins[2] = {{in, quad}, {id, word}};
    if (const int k = spans_alias(outs, 4, ins, 2))
        return fail(LRT_E_INVALID, k == 1 ? "aliasing: an output buffer overlaps an input (in place is not allowed)"
                                          : "aliasing: two output buffers overlap");
    return LRT_OK;
}

template <int R>
static void launch_firefly(const FireflyArgs& a, int rank, dim3 grid, hipStream_t s) {
    switch (rank) {
        case 1: firefly_kernel<R, 1><<<grid, kFfW * kFfH, 0, s>>>(a); break;
        case 2: firefly_kernel<R, 2><<<grid, kFfW * kFfH, 0, s>>>(a); break;
        case 3: firefly_kernel<R, 3><<<grid, kFfW * kFfH, 0, s>>>(a); break;
        default: firefly_kernel<R, 4><<<grid, kFfW * kFfH, 0, s>>>(a); break;
    }
}

// The pass on stream s (device pointers, validated).
static int firefly_device(const lrt_firefly_desc* d, const float* in, const int32_t* id, float* out, float* excess,
                          int32_t* cls, uint32_t* info, hipStream_t s) {
    FireflyArgs a;
    memset(&a, 0, sizeof(a));
    a.in = quads(in);
    a.id = id;
    a.out = quads(out);
    a.excess = quads(excess);
    a.cls = cls;
    a.info = info;
    a.w = d->width;
    a.h = d->height;
    a.min_taps = d->min_taps;
    a.gain = d->gain;
    a.floor = d->floor;
    if (info) LRT_HIP(hipMemsetAsync(info, 0, 2 * sizeof(uint32_t), s));
    const dim3 grid((unsigned)((a.w + kFfW - 1) / kFfW), (unsigned)((a.h + kFfH - 1) / kFfH));
    if (d->radius == 1) launch_firefly<1>(a, d->rank, grid, s);
    else launch_firefly<2>(a, d->rank, grid, s);
    LRT_HIP(hipGetLastError());
    return LRT_OK;
}

}  // namespace lrt

using namespace lrt;

extern "C" {

int lrt_firefly_default(int width, int height, lrt_firefly_desc* out) {
    if (int rc = frame_default_begin(out, sizeof(*out), width, height)) return rc;
    out->width = width;
    out->height = height;
    out->radius = 1;
    out->rank = 2;
    out->min_taps = 3;
    out->gain = 2.0f;
    out->floor = 0.01f;
    return LRT_OK;
}

int lrt_firefly_device(const lrt_firefly_desc* desc, const float* d_in, const int32_t* d_id, float* d_out,
                       float* d_excess, int32_t* d_class, uint32_t* d_info, void* stream) {
    RoctxRange rr_("lrt_firefly_device");
    if (int rc = validate_firefly(desc, d_in, d_id, d_out, d_excess, d_class, d_info)) return rc;
    std::lock_guard<std::mutex> lk(g_mu);
    if (int rc = require_initialized()) return rc;
    DeviceScope ds_(0);   // context 0's device (device 0 of lrt_initialize_devices)
    return firefly_device(desc, d_in, d_id, d_out, d_excess, d_class, d_info, (hipStream_t)stream);
}

int lrt_firefly_host(const lrt_firefly_desc* desc, const float* in, const int32_t* id, float* out, float* excess_out,
                     int32_t* class_out, uint32_t* info) {
    RoctxRange rr_("lrt_firefly_host");
    if (int rc = validate_firefly(desc, in, id, out, excess_out, class_out, info)) return rc;
    std::lock_guard<std::mutex> lk(g_mu);
    if (int rc = require_initialized()) return rc;
    DeviceScope ds_(0);
    hipStream_t s = ctx().stream;
    const size_t px = (size_t)desc->width * desc->height, quad = 16 * px, word = 4 * px;
    HostMirrors m;
    const int in_ = m.in(in, quad), id_ = m.in(id, word);
    const int out_ = m.out(out, quad), excess_ = m.out(excess_out, quad), class_ = m.out(class_out, word);
    const int info_ = m.out(info, 2 * sizeof(uint32_t));
    if (int rc = m.alloc("hipMalloc(firefly staging)")) return rc;
    if (int rc = m.upload(s)) return rc;
    if (int rc = firefly_device(desc, m.dev<float>(in_), m.dev<int32_t>(id_), m.dev<float>(out_), m.dev<float>(excess_),
                                m.dev<int32_t>(class_), m.dev<uint32_t>(info_), s))
        return rc;
    return m.download(s);
}

}  // extern "C"
