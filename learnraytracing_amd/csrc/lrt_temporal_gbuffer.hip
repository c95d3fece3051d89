// Temporal accumulation driven by the G-buffer (lrt_temporal_accumulate_gbuffer_*, include/lrt.h):
// the step of lrt_temporal.hip without cameras, scenes or a sphere loop. One thread per pixel reads
// its motion vector and its sphere's id from the planes lrt_gbuffer_* wrote, gathers the four
// bilinear taps of the previous state whose id is the pixel's (and, for a hit, whose normal agrees),
// blends the history in and keeps the second moment. One launch per step, no atomics, no LDS, no
// barrier. No id is used as an index. Not bit-pinned: contraction is allowed, as in lrt_temporal.hip.
#include "lrt_internal.h"

#pragma clang fp contract(fast)

#include "lrt_temporal_blend.h"   // steps 6 and 7, under this unit's contraction

namespace lrt {

struct TemporalGbufferArgs {
    const float4* color;   // the current frame
    const float4* nrm;     // its G-buffer: normal, motion, id
    const float4* motion;
    const int* id;
    const float4* pc;      // the previous state's color and moment2 (kHist launches)
    const float4* pm;
    const float4* pn;      // the previous G-buffer's normal and id
    const int* pid;
    float4* oc;            // the next state's color and moment2
    float4* om;
    float4* ostd;          // or null
    int w, h;
    float k, alpha_min, normal_min, short_std, min_history;
};

// One pixel of the step. kHist: there is a previous state (else every pixel is reset).
template <bool kHist>
__global__ __launch_bounds__(kPixBlockW* kPixBlockH) void temporal_gbuffer_kernel(TemporalGbufferArgs a) {
    const int x = block_x(), y = block_y();
    if (x >= a.w || y >= a.h) return;
    const size_t ip = (size_t)y * a.w + x;
    const float4 c4 = a.color[ip];
    const float3 C = make_float3(a.k * c4.x, a.k * c4.y, a.k * c4.z);
    float3 col = C, m2 = make_float3(C.x * C.x, C.y * C.y, C.z * C.z);
    float n = 1.0f;
    if (kHist) {
        const float4 n4 = a.nrm[ip], mv = a.motion[ip];
        const int id = a.id[ip];
        // a zero motion gives fx = x with no rounding: the G-buffer's static-camera guarantee carries through
        float fx = (float)x + mv.x, fy = (float)y + mv.y;
        const bool ok = mv.w != 0.0f && fabsf(fx) < 1e6f && fabsf(fy) < 1e6f;   // (a NaN fails both compares)
        if (!ok) fx = fy = 0.0f;
        const float flx = floorf(fx), fly = floorf(fy);
        const int x0 = (int)flx, y0 = (int)fly;
        const float tx = fx - flx, ty = fy - fly;
        // the sixteen gathers issued back to back, from addresses clamped into the image
        float4 qc[4], qm[4], qn[4];
        int qi[4];
        bool in[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int gx = x0 + (i & 1), gy = y0 + (i >> 1);
            in[i] = ok && gx >= 0 && gx < a.w && gy >= 0 && gy < a.h;
            const size_t iq = (size_t)min(max(gy, 0), a.h - 1) * a.w + min(max(gx, 0), a.w - 1);
            qi[i] = a.pid[iq];
            qn[i] = a.pn[iq];
            qc[i] = a.pc[iq];
            qm[i] = a.pm[iq];
        }
        float sw = 0.0f, sn = 0.0f;
        float3 sc = make_float3(0.0f, 0.0f, 0.0f), sm = sc;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const float b = ((i & 1) ? tx : 1.0f - tx) * ((i >> 1) ? ty : 1.0f - ty);
            const float nd = qn[i].x * n4.x + qn[i].y * n4.y + qn[i].z * n4.z;
            const bool same = qi[i] == id && (id < 0 || nd >= a.normal_min);
            const float bw = in[i] && same ? b : 0.0f;
            sw += bw;
            sn += bw * qm[i].w;
            sc = make_float3(bw * qc[i].x + sc.x, bw * qc[i].y + sc.y, bw * qc[i].z + sc.z);
            sm = make_float3(bw * qm[i].x + sm.x, bw * qm[i].y + sm.y, bw * qm[i].z + sm.z);
        }
        if (sw > 1e-3f) temporal_blend(sw, sn, sc, sm, C, a.alpha_min, col, m2, n);
    }
    write_rgb(a.oc, ip, col);
    a.om[ip] = make_float4(m2.x, m2.y, m2.z, n);
    write_std(a.ostd, ip, col, m2, n, a.short_std, a.min_history);
}

// Everything that needs neither the library's state nor the device.
static int validate_temporal_gbuffer(const lrt_temporal_gbuffer_desc* d, const float* color, const lrt_gbuffer* cur,
                                     const lrt_gbuffer* prev_g, const lrt_temporal_state* prev,
                                     const lrt_temporal_state* next, const float* std) {
    if (!d) return fail(LRT_E_INVALID, "desc is NULL");
    if (!color) return fail(LRT_E_INVALID, "color is NULL");
    if (!cur || !cur->normal || !cur->motion || !cur->id) return fail(LRT_E_INVALID, "cur needs normal, motion and id");
    if (!next || !next->color || !next->moment2) return fail(LRT_E_INVALID, "next needs color and moment2");
    if (int rc = validate_history_pair(prev, prev_g)) return rc;
    if (int rc = validate_frame_size(d->width, d->height)) return rc;
    if (d->flags != 0 || d->reserved != 0 || d->reserved2 != 0) return fail(LRT_E_INVALID, "flags and reserved must be 0");
    if (int rc = validate_min_history(d->min_history)) return rc;
    for (float v : {d->cur_scale, d->alpha_min, d->normal_min, d->short_std})
        if (!std::isfinite(v)) return fail(LRT_E_INVALID, "parameters must be finite");
    if (!(d->cur_scale > 0.0f) || !(d->short_std > 0.0f)) return fail(LRT_E_INVALID, "cur_scale and short_std must be > 0");
    if (int rc = validate_alpha_min(d->alpha_min)) return rc;
    if (int rc = validate_normal_min(d->normal_min)) return rc;
    // no output may overlap an input, a previous buffer or another output
    const size_t px = (size_t)d->width * d->height, quad = 16 * px, word = 4 * px;
    const Span outs[3] = {{next->color, quad}, {next->moment2, quad}, {std, quad}};
    const Span ins[8] = {{color, quad}, {cur->normal, quad}, {cur->motion, quad}, {cur->id, word},
                         {prev ? prev->color : nullptr, quad}, {prev ? prev->moment2 : nullptr, quad},
                         {prev_g ? prev_g->normal : nullptr, quad}, {prev_g ? prev_g->id : nullptr, word}};
    if (const int al = spans_alias(outs, 3, ins, 8))
        return fail(LRT_E_INVALID, al == 1 ? "aliasing: an output buffer overlaps an input or a prev buffer"
                                           : "aliasing: two output buffers overlap");
    return validate_gbuffer_kept(ins[1], ins[3], ins[6], ins[7]);
}

// The step on stream s (device pointers, validated).
static int temporal_gbuffer_device(const lrt_temporal_gbuffer_desc* d, const float* color, const lrt_gbuffer* cur,
                                   const lrt_gbuffer* prev_g, const lrt_temporal_state* prev,
                                   const lrt_temporal_state* next, float* std, hipStream_t s) {
    TemporalGbufferArgs a;
    memset(&a, 0, sizeof(a));
    a.color = quads(color);
    a.nrm = quads(cur->normal);
    a.motion = quads(cur->motion);
    a.id = cur->id;
    if (prev) a.pc = quads(prev->color), a.pm = quads(prev->moment2), a.pn = quads(prev_g->normal), a.pid = prev_g->id;
    a.oc = quads(next->color);
    a.om = quads(next->moment2);
    a.ostd = quads(std);
    a.w = d->width;
    a.h = d->height;
    a.k = d->cur_scale;
    a.alpha_min = d->alpha_min;
    a.normal_min = d->normal_min;
    a.short_std = d->short_std;
    a.min_history = (float)d->min_history;
    const dim3 grid = pixel_grid(a.w, a.h);
    if (prev)
        temporal_gbuffer_kernel<true><<<grid, kPixBlockW * kPixBlockH, 0, s>>>(a);
    else
        temporal_gbuffer_kernel<false><<<grid, kPixBlockW * kPixBlockH, 0, s>>>(a);
    LRT_HIP(hipGetLastError());
    return LRT_OK;
}

}  // namespace lrt

using namespace lrt;

extern "C" {

int lrt_temporal_gbuffer_default(int width, int height, lrt_temporal_gbuffer_desc* out) {
    if (int rc = frame_default_begin(out, sizeof(*out), width, height)) return rc;
    out->width = width;
    out->height = height;
    out->min_history = 4;
    out->cur_scale = 1.0f;
    out->alpha_min = 0.05f;
    out->normal_min = 0.9f;
    out->short_std = 1e3f;
    return LRT_OK;
}

int lrt_temporal_accumulate_gbuffer_device(const lrt_temporal_gbuffer_desc* desc, const float* d_color,
                                           const lrt_gbuffer* d_cur, const lrt_gbuffer* d_prev_g,
                                           const lrt_temporal_state* d_prev, const lrt_temporal_state* d_next,
                                           float* d_color_std, void* stream) {
    RoctxRange rr_("lrt_temporal_accumulate_gbuffer_device");
    if (int rc = validate_temporal_gbuffer(desc, d_color, d_cur, d_prev_g, d_prev, d_next, d_color_std)) return rc;
    std::lock_guard<std::mutex> lk(g_mu);
    if (int rc = require_initialized()) return rc;
    DeviceScope ds_(0);   // context 0's device (device 0 of lrt_initialize_devices)
    return temporal_gbuffer_device(desc, d_color, d_cur, d_prev_g, d_prev, d_next, d_color_std, (hipStream_t)stream);
}

int lrt_temporal_accumulate_gbuffer_host(const lrt_temporal_gbuffer_desc* desc, const float* color,
                                         const lrt_gbuffer* cur, const lrt_gbuffer* prev_g,
                                         const lrt_temporal_state* prev, const lrt_temporal_state* next,
                                         float* color_std) {
    RoctxRange rr_("lrt_temporal_accumulate_gbuffer_host");
    if (int rc = validate_temporal_gbuffer(desc, color, cur, prev_g, prev, next, color_std)) return rc;
    std::lock_guard<std::mutex> lk(g_mu);
    if (int rc = require_initialized()) return rc;
    DeviceScope ds_(0);
    hipStream_t s = ctx().stream;
    // Every buffer that is given goes through a device mirror of its own. The two outputs whose alpha
    // stays (next->color, color_std) are copied in first.
    const size_t px = (size_t)desc->width * desc->height, quad = 16 * px, word = 4 * px;
    HostMirrors m;
    const int color_ = m.in(color, quad), normal_ = m.in(cur->normal, quad), motion_ = m.in(cur->motion, quad);
    const int id_ = m.in(cur->id, word);
    const int pcolor_ = m.in(prev ? prev->color : nullptr, quad), pmoment_ = m.in(prev ? prev->moment2 : nullptr, quad);
    const int pnormal_ = m.in(prev_g ? prev_g->normal : nullptr, quad), pid_ = m.in(prev_g ? prev_g->id : nullptr, word);
    const int ncolor_ = m.inout(next->color, quad), nmoment_ = m.out(next->moment2, quad), std_ = m.inout(color_std, quad);
    if (int rc = m.alloc("hipMalloc(temporal staging)")) return rc;
    if (int rc = m.upload(s)) return rc;
    auto f = [&m](int i) { return m.dev<float>(i); };
    lrt_gbuffer dcur, dprev_g;
    memset(&dcur, 0, sizeof(dcur));
    memset(&dprev_g, 0, sizeof(dprev_g));
    dcur.normal = f(normal_);
    dcur.motion = f(motion_);
    dcur.id = m.dev<int32_t>(id_);
    dprev_g.normal = f(pnormal_);
    dprev_g.id = m.dev<int32_t>(pid_);
    const lrt_temporal_state dprev = {f(pcolor_), f(pmoment_), nullptr, nullptr, nullptr};
    const lrt_temporal_state dnext = {f(ncolor_), f(nmoment_), nullptr, nullptr, nullptr};
    if (int rc = temporal_gbuffer_device(desc, f(color_), &dcur, prev ? &dprev_g : nullptr, prev ? &dprev : nullptr, &dnext,
                                         f(std_), s))
        return rc;
    return m.download(s);
}

}  // extern "C"
