// History rectification (lrt_temporal_rectify_*, include/lrt.h): the state's colour is held to the
// local range of a reference frame. Per pixel a windowed, id-aware mean and standard deviation of
// the reference, the clamp of the history into mean +- gamma sigma, and a history length shortened
// by how far the clamp had to move it. A workgroup stages its pixels' reference (rgb, the id's bits
// in the fourth word) plus a halo of `radius` into an LDS tile; each thread then reads its window
// with 16-byte LDS reads. One launch, one barrier, no atomics, no scratch. No id is used as an
// index. Not bit-pinned: contraction is allowed, as in lrt_temporal_gbuffer.hip.
#include "lrt_internal.h"

#pragma clang fp contract(fast)

#include "lrt_temporal_blend.h"   // step 7, under this unit's contraction

namespace lrt {

struct RectifyArgs {
    const float4* ref;   // the reference frame
    const int* id;       // the current G-buffer's ids
    const float4* sc;    // the state's color and moment2
    const float4* sm;
    float4* oc;          // the rectified state's (may be sc and sm: each pixel is read and written by its own thread)
    float4* om;
    float4* ostd;        // or null
    int* ocls;           // or null
    int w, h, min_taps;
    float k, gamma, range_floor, reset_history, short_std, min_history;
};

// A workgroup covers 32 x 8 pixels, a pixel per thread; a wave covers two rows of 32. With that map
// the sixteen lanes that a 16-byte LDS read serves in one cycle ({0-3, 12-15, 20-27} and so on,
// DESIGN 7.10) lie in one row at columns that differ mod 16: their quads cover the 64 banks once
// whatever the row pitch is, so the tile needs no padding.
constexpr int kRectW = 32, kRectH = 8;
// A tile slot as one native vector: a float4's members are loaded one by one and come back together
// as a 12-byte and a 4-byte read; a vector load stays one 16-byte read.
typedef float RectQuad __attribute__((ext_vector_type(4)));

template <int R>
__global__ __launch_bounds__(kRectW* kRectH) void rectify_kernel(RectifyArgs a) {
    constexpr int TW = kRectW + 2 * R, TH = kRectH + 2 * R, D = 2 * R + 1;
    __shared__ RectQuad tile[TH * TW];
    const int t = threadIdx.x, lx = t & (kRectW - 1), ly = t / kRectW;
    const int bx = blockIdx.x * kRectW, by = blockIdx.y * kRectH;
    const int x = bx + lx, y = by + ly;
    const bool live = x < a.w && y < a.h;
    // the thread's own state, issued ahead of the staging loads and the barrier
    const size_t ip = (size_t)min(y, a.h - 1) * a.w + min(x, a.w - 1);
    const float4 c4 = a.sc[ip], m4 = a.sm[ip];
    // the tile: addresses clamped into the image (what an outside slot holds is never counted: below)
    for (int i = t; i < TH * TW; i += kRectW * kRectH) {
        const int tx = i % TW, ty = i / TW;
        const int gx = min(max(bx + tx - R, 0), a.w - 1), gy = min(max(by + ty - R, 0), a.h - 1);
        const size_t iq = (size_t)gy * a.w + gx;
        const float4 r = a.ref[iq];
        tile[i] = RectQuad{a.k * r.x, a.k * r.y, a.k * r.z, __int_as_float(a.id[iq])};
    }
    __syncthreads();
    if (!live) return;
    // Step 1. Every int32 is a legal id, so no value of the fourth word can mean "outside": the
    // window's columns and rows that lie in the image are lane masks, taken once per thread.
    // (0 / 1 words combined with &: as bools under && every tap became a branch that waited for its
    // own read before the next was issued)
    int inx[D];
#pragma unroll
    for (int j = 0; j < D; ++j) inx[j] = (unsigned)(x + j - R) < (unsigned)a.w;
    const RectQuad K = tile[(ly + R) * TW + lx + R];
    const int id = __float_as_int(K.w);
    int m = 0;
    float3 s1 = make_float3(0.0f, 0.0f, 0.0f), s2 = s1;
    // a row of the window per trip (its 2 R + 1 reads in flight together): unrolled over the rows
    // too, the compiler hoists all (2 R + 1)^2 reads and radius 3 takes 208 VGPRs
#pragma unroll 1
    for (int dy = 0; dy < D; ++dy) {
        const int iny = (unsigned)(y + dy - R) < (unsigned)a.h;
        const RectQuad* const row = tile + (ly + dy) * TW + lx;
#pragma unroll
        for (int dx = 0; dx < D; ++dx) {
            const RectQuad q = row[dx];
            const int cnt = iny & inx[dx] & (int)(__float_as_int(q.w) == id);
            const bool counts = cnt != 0;
            // a select, not a product: a tap that does not count adds 0 whatever it holds
            const float ex = counts ? q.x - K.x : 0.0f, ey = counts ? q.y - K.y : 0.0f, ez = counts ? q.z - K.z : 0.0f;
            m += cnt;
            s1 = make_float3(s1.x + ex, s1.y + ey, s1.z + ez);
            s2 = make_float3(ex * ex + s2.x, ey * ey + s2.y, ez * ez + s2.z);
        }
    }
    const float fm = (float)m;
    const float3 av = make_float3(s1.x / fm, s1.y / fm, s1.z / fm);
    const float3 mu = make_float3(K.x + av.x, K.y + av.y, K.z + av.z);
    const float3 gs = make_float3(a.gamma * sqrtf(fmaxf(s2.x / fm - av.x * av.x, 0.0f)),
                                  a.gamma * sqrtf(fmaxf(s2.y / fm - av.y * av.y, 0.0f)),
                                  a.gamma * sqrtf(fmaxf(s2.z / fm - av.z * av.z, 0.0f)));
    // Steps 2 to 4. A channel that did not move, and every channel of an unsupported pixel, keeps its bits.
    const bool supported = m >= a.min_taps;
    float3 col = make_float3(c4.x, c4.y, c4.z), m2 = make_float3(m4.x, m4.y, m4.z);
    float n = m4.w;
    int cls = 2;
    if (supported) {
        const float cc[3] = {c4.x, c4.y, c4.z}, mm[3] = {m4.x, m4.y, m4.z};
        const float mus[3] = {mu.x, mu.y, mu.z}, gss[3] = {gs.x, gs.y, gs.z};
        float oc[3], om[3], tmax = 0.0f;
        bool any = false;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            const float c = cc[ch], cl = fminf(fmaxf(c, mus[ch] - gss[ch]), mus[ch] + gss[ch]);
            const bool moved = cl != c;
            const float d = fabsf(cl - c);
            tmax = fmaxf(tmax, d / (d + gss[ch] + a.range_floor));
            oc[ch] = moved ? cl : c;
            om[ch] = moved ? cl * cl + fmaxf(mm[ch] - c * c, 0.0f) : mm[ch];
            any = any || moved;
        }
        const float e = tmax * tmax;
        col = make_float3(oc[0], oc[1], oc[2]);
        m2 = make_float3(om[0], om[1], om[2]);
        n = any ? n + e * (fminf(n, a.reset_history) - n) : n;
        cls = any ? 1 : 0;
    }
    const size_t io = (size_t)y * a.w + x;
    write_rgb(a.oc, io, col);
    a.om[io] = make_float4(m2.x, m2.y, m2.z, n);
    write_std(a.ostd, io, col, m2, n, a.short_std, a.min_history);
    if (a.ocls) a.ocls[io] = cls;
}

// Everything that needs neither the library's state nor the device.
static int validate_rectify(const lrt_rectify_desc* d, const float* ref, const int32_t* id,
                            const lrt_temporal_state* state, const lrt_temporal_state* out, const float* std,
                            const int32_t* cls) {
    if (!d) return fail(LRT_E_INVALID, "desc is NULL");
    if (!ref) return fail(LRT_E_INVALID, "ref is NULL");
    if (!id) return fail(LRT_E_INVALID, "id is NULL");
    if (!state || !state->color || !state->moment2) return fail(LRT_E_INVALID, "state needs color and moment2");
    if (!out || !out->color || !out->moment2) return fail(LRT_E_INVALID, "out needs color and moment2");
    if (int rc = validate_frame_size(d->width, d->height)) return rc;
    if (d->flags != 0 || d->reserved != 0) return fail(LRT_E_INVALID, "flags and reserved must be 0");
    if (d->radius < 1 || d->radius > LRT_RECTIFY_MAX_RADIUS) return fail(LRT_E_INVALID, "radius must be in 1..3");
    const int side = 2 * d->radius + 1;
    if (d->min_taps < 1 || d->min_taps > side * side) return fail(LRT_E_INVALID, "min_taps must be in 1..(2 radius + 1)^2");
    if (int rc = validate_min_history(d->min_history)) return rc;
    for (float v : {d->ref_scale, d->gamma, d->range_floor, d->reset_history, d->short_std})
        if (!std::isfinite(v)) return fail(LRT_E_INVALID, "parameters must be finite");
    if (!(d->ref_scale > 0.0f) || !(d->range_floor > 0.0f) || !(d->short_std > 0.0f))
        return fail(LRT_E_INVALID, "ref_scale, range_floor and short_std must be > 0");
    if (!(d->gamma >= 0.0f) || !(d->reset_history >= 0.0f)) return fail(LRT_E_INVALID, "gamma and reset_history must be >= 0");
    // out's color and moment2 may be the state's own, exactly (in place); otherwise no output may
    // overlap an input or another output
    const size_t px = (size_t)d->width * d->height, quad = 16 * px, word = 4 * px;
    const Span outs[4] = {{out->color, quad}, {out->moment2, quad}, {std, quad}, {cls, word}};
    const Span ins[4] = {{ref, quad}, {id, word}, {state->color, quad}, {state->moment2, quad}};
    for (int i = 0; i < 4; ++i) {
        for (int k = 0; k < 4; ++k)
            if (ranges_overlap(outs[i].p, outs[i].bytes, ins[k].p, ins[k].bytes) &&
                !(i < 2 && k == i + 2 && outs[i].p == ins[k].p))
                return fail(LRT_E_INVALID, "aliasing: an output buffer overlaps an input (only out's color and moment2 "
                                           "may be the state's own, exactly)");
        for (int j = i + 1; j < 4; ++j)
            if (ranges_overlap(outs[i].p, outs[i].bytes, outs[j].p, outs[j].bytes))
                return fail(LRT_E_INVALID, "aliasing: two output buffers overlap");
    }
    return LRT_OK;
}

// The step on stream s (device pointers, validated).
static int rectify_device(const lrt_rectify_desc* d, const float* ref, const int32_t* id, const lrt_temporal_state* state,
                          const lrt_temporal_state* out, float* std, int32_t* cls, hipStream_t s) {
    RectifyArgs a;
    memset(&a, 0, sizeof(a));
    a.ref = quads(ref);
    a.id = id;
    a.sc = quads(state->color);
    a.sm = quads(state->moment2);
    a.oc = quads(out->color);
    a.om = quads(out->moment2);
    a.ostd = quads(std);
    a.ocls = cls;
    a.w = d->width;
    a.h = d->height;
    a.min_taps = d->min_taps;
    a.k = d->ref_scale;
    a.gamma = d->gamma;
    a.range_floor = d->range_floor;
    a.reset_history = d->reset_history;
    a.short_std = d->short_std;
    a.min_history = (float)d->min_history;
    const dim3 grid((unsigned)((a.w + kRectW - 1) / kRectW), (unsigned)((a.h + kRectH - 1) / kRectH));
    switch (d->radius) {
        case 1: rectify_kernel<1><<<grid, kRectW * kRectH, 0, s>>>(a); break;
        case 2: rectify_kernel<2><<<grid, kRectW * kRectH, 0, s>>>(a); break;
        default: rectify_kernel<3><<<grid, kRectW * kRectH, 0, s>>>(a); break;
    }
    LRT_HIP(hipGetLastError());
    return LRT_OK;
}

}  // namespace lrt

using namespace lrt;

extern "C" {

int lrt_temporal_rectify_default(int width, int height, lrt_rectify_desc* out) {
    if (int rc = frame_default_begin(out, sizeof(*out), width, height)) return rc;
    out->width = width;
    out->height = height;
    out->radius = 2;
    out->min_taps = 5;
    out->min_history = 4;
    out->ref_scale = 1.0f;
    out->gamma = 1.0f;
    out->range_floor = 1e-4f;
    out->reset_history = 1.0f;
    out->short_std = 1e3f;
    return LRT_OK;
}

int lrt_temporal_rectify_device(const lrt_rectify_desc* desc, const float* d_ref, const int32_t* d_id,
                                const lrt_temporal_state* d_state, const lrt_temporal_state* d_out,
                                float* d_color_std, int32_t* d_class, void* stream) {
    RoctxRange rr_("lrt_temporal_rectify_device");
    if (int rc = validate_rectify(desc, d_ref, d_id, d_state, d_out, d_color_std, d_class)) return rc;
    std::lock_guard<std::mutex> lk(g_mu);
    if (int rc = require_initialized()) return rc;
    DeviceScope ds_(0);   // context 0's device (device 0 of lrt_initialize_devices)
    return rectify_device(desc, d_ref, d_id, d_state, d_out, d_color_std, d_class, (hipStream_t)stream);
}

int lrt_temporal_rectify_host(const lrt_rectify_desc* desc, const float* ref, const int32_t* id,
                              const lrt_temporal_state* state, const lrt_temporal_state* out,
                              float* color_std, int32_t* class_out) {
    RoctxRange rr_("lrt_temporal_rectify_host");
    if (int rc = validate_rectify(desc, ref, id, state, out, color_std, class_out)) return rc;
    std::lock_guard<std::mutex> lk(g_mu);
    if (int rc = require_initialized()) return rc;
    DeviceScope ds_(0);
    hipStream_t s = ctx().stream;
    // Every buffer goes through a device mirror of its own: a call in place on the host has two
    // mirrors of each state frame and runs out of place on the device (the same bits). The two
    // outputs whose alpha stays (out->color, color_std) are copied in first.
    const size_t px = (size_t)desc->width * desc->height, quad = 16 * px, word = 4 * px;
    HostMirrors m;
    const int ref_ = m.in(ref, quad), id_ = m.in(id, word);
    const int scolor_ = m.in(state->color, quad), smoment_ = m.in(state->moment2, quad);
    const int ocolor_ = m.inout(out->color, quad), omoment_ = m.out(out->moment2, quad), std_ = m.inout(color_std, quad);
    const int class_ = m.out(class_out, word);
    if (int rc = m.alloc("hipMalloc(rectify staging)")) return rc;
    if (int rc = m.upload(s)) return rc;
    auto f = [&m](int i) { return m.dev<float>(i); };
    const lrt_temporal_state dstate = {f(scolor_), f(smoment_), nullptr, nullptr, nullptr};
    const lrt_temporal_state dnext = {f(ocolor_), f(omoment_), nullptr, nullptr, nullptr};
    if (int rc = rectify_device(desc, f(ref_), m.dev<int32_t>(id_), &dstate, &dnext, f(std_), m.dev<int32_t>(class_), s))
        return rc;
    return m.download(s);
}

}  // extern "C"
