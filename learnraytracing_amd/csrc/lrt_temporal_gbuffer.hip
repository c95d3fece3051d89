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

// lrt_temporal.hip's shape: a wave covers 8 x 8 pixels, a workgroup of four waves 32 x 8.
constexpr int kBlockW = 32, kBlockH = 8;

// One pixel of the step. kHist: there is a previous state (else every pixel is reset).
template <bool kHist>
__global__ __launch_bounds__(kBlockW* kBlockH) void temporal_gbuffer_kernel(TemporalGbufferArgs a) {
    const int t = threadIdx.x;   // wave t / 64, its lane's pixel (t % 8, t / 8 % 8)
    const int x = blockIdx.x * kBlockW + (t >> 6) * 8 + (t & 7), y = blockIdx.y * kBlockH + ((t >> 3) & 7);
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
    float* const oc = reinterpret_cast<float*>(a.oc + ip);   // 12 B: the alpha stays
    oc[0] = col.x;
    oc[1] = col.y;
    oc[2] = col.z;
    a.om[ip] = make_float4(m2.x, m2.y, m2.z, n);
    if (a.ostd) {
        const float3 sd = temporal_std(col, m2, n, a.short_std, a.min_history);
        float* const os = reinterpret_cast<float*>(a.ostd + ip);
        os[0] = sd.x;
        os[1] = sd.y;
        os[2] = sd.z;
    }
}

// Everything that needs neither the library's state nor the device.
static int validate_temporal_gbuffer(const lrt_temporal_gbuffer_desc* d, const float* color, const lrt_gbuffer* cur,
                                     const lrt_gbuffer* prev_g, const lrt_temporal_state* prev,
                                     const lrt_temporal_state* next, const float* std) {
    if (!d) return fail(LRT_E_INVALID, "desc is NULL");
    if (!color) return fail(LRT_E_INVALID, "color is NULL");
    if (!cur || !cur->normal || !cur->motion || !cur->id) return fail(LRT_E_INVALID, "cur needs normal, motion and id");
    if (!next || !next->color || !next->moment2) return fail(LRT_E_INVALID, "next needs color and moment2");
    if (!prev != !prev_g) return fail(LRT_E_INVALID, "prev and prev_g must both be given, or neither");
    if (prev && (!prev->color || !prev->moment2)) return fail(LRT_E_INVALID, "prev needs color and moment2");
    if (prev_g && (!prev_g->normal || !prev_g->id)) return fail(LRT_E_INVALID, "prev_g needs normal and id");
    if (int rc = validate_frame_size(d->width, d->height)) return rc;
    if (d->flags != 0 || d->reserved != 0 || d->reserved2 != 0) return fail(LRT_E_INVALID, "flags and reserved must be 0");
    if (d->min_history < 1) return fail(LRT_E_INVALID, "min_history must be >= 1");
    for (float v : {d->cur_scale, d->alpha_min, d->normal_min, d->short_std})
        if (!std::isfinite(v)) return fail(LRT_E_INVALID, "parameters must be finite");
    if (!(d->cur_scale > 0.0f) || !(d->short_std > 0.0f)) return fail(LRT_E_INVALID, "cur_scale and short_std must be > 0");
    if (!(d->alpha_min > 0.0f && d->alpha_min <= 1.0f)) return fail(LRT_E_INVALID, "alpha_min must be in (0, 1]");
    if (!(d->normal_min >= -1.0f && d->normal_min <= 1.0f)) return fail(LRT_E_INVALID, "normal_min must be in [-1, 1]");
    // no output may overlap an input, a previous buffer or another output
    const size_t px = (size_t)d->width * d->height, quad = 16 * px, word = 4 * px;
    const Span outs[3] = {{next->color, quad}, {next->moment2, quad}, {std, quad}};
    const Span ins[8] = {{color, quad}, {cur->normal, quad}, {cur->motion, quad}, {cur->id, word},
                         {prev ? prev->color : nullptr, quad}, {prev ? prev->moment2 : nullptr, quad},
                         {prev_g ? prev_g->normal : nullptr, quad}, {prev_g ? prev_g->id : nullptr, word}};
    if (const int al = spans_alias(outs, 3, ins, 8))
        return fail(LRT_E_INVALID, al == 1 ? "aliasing: an output buffer overlaps an input or a prev buffer"
                                           : "aliasing: two output buffers overlap");
    // a G-buffer overwritten in place is no history
    if (prev_g)
        for (const Span& c : {ins[1], ins[3]})
            for (const Span& p : {ins[6], ins[7]})
                if (ranges_overlap(c.p, c.bytes, p.p, p.bytes))
                    return fail(LRT_E_INVALID, "aliasing: cur's normal or id overlaps prev_g's");
    return LRT_OK;
}

// The step on stream s (device pointers, validated).
static int temporal_gbuffer_device(const lrt_temporal_gbuffer_desc* d, const float* color, const lrt_gbuffer* cur,
                                   const lrt_gbuffer* prev_g, const lrt_temporal_state* prev,
                                   const lrt_temporal_state* next, float* std, hipStream_t s) {
    TemporalGbufferArgs a;
    memset(&a, 0, sizeof(a));
    auto q = [](const float* p) { return reinterpret_cast<const float4*>(p); };
    a.color = q(color);
    a.nrm = q(cur->normal);
    a.motion = q(cur->motion);
    a.id = cur->id;
    if (prev) a.pc = q(prev->color), a.pm = q(prev->moment2), a.pn = q(prev_g->normal), a.pid = prev_g->id;
    a.oc = reinterpret_cast<float4*>(next->color);
    a.om = reinterpret_cast<float4*>(next->moment2);
    a.ostd = reinterpret_cast<float4*>(std);
    a.w = d->width;
    a.h = d->height;
    a.k = d->cur_scale;
    a.alpha_min = d->alpha_min;
    a.normal_min = d->normal_min;
    a.short_std = d->short_std;
    a.min_history = (float)d->min_history;
    const dim3 grid((unsigned)((a.w + kBlockW - 1) / kBlockW), (unsigned)((a.h + kBlockH - 1) / kBlockH));
    if (prev)
        temporal_gbuffer_kernel<true><<<grid, kBlockW * kBlockH, 0, s>>>(a);
    else
        temporal_gbuffer_kernel<false><<<grid, kBlockW * kBlockH, 0, s>>>(a);
    LRT_HIP(hipGetLastError());
    return LRT_OK;
}

}  // namespace lrt

using namespace lrt;

extern "C" {

int lrt_temporal_gbuffer_default(int width, int height, lrt_temporal_gbuffer_desc* out) {
    if (!out) return fail(LRT_E_INVALID, "out is NULL");
    if (width < 1 || height < 1) return fail(LRT_E_INVALID, "invalid image size");
    memset(out, 0, sizeof(*out));
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
    // Every buffer goes through a device mirror of its own, all in one allocation that lives for the
    // call: nine RGBA frames (3 inputs, 3 of the history, 3 outputs), then the two id planes, so that
    // every mirror stays 16 B aligned. The two outputs whose alpha stays are copied in first.
    const size_t px = (size_t)desc->width * desc->height, quad = 16 * px, word = 4 * px;
    const float* const hin[6] = {color, cur->normal, cur->motion, prev ? prev->color : nullptr,
                                 prev ? prev->moment2 : nullptr, prev_g ? prev_g->normal : nullptr};
    const int32_t* const hid[2] = {cur->id, prev_g ? prev_g->id : nullptr};
    float* const hout[3] = {next->color, next->moment2, color_std};
    DeviceStaging<char> m;
    if (hipMalloc(&m.p, 9 * quad + 2 * word) != hipSuccess) return fail(LRT_E_NOMEM, "hipMalloc(temporal staging)");
    float* din[6];
    float* dout[3];
    int32_t* did[2];
    for (int i = 0; i < 6; ++i) {
        din[i] = hin[i] ? reinterpret_cast<float*>(m.p + i * quad) : nullptr;
        if (hin[i]) LRT_HIP(hipMemcpyAsync(din[i], hin[i], quad, hipMemcpyHostToDevice, s));
    }
    for (int i = 0; i < 2; ++i) {
        did[i] = hid[i] ? reinterpret_cast<int32_t*>(m.p + 9 * quad + i * word) : nullptr;
        if (hid[i]) LRT_HIP(hipMemcpyAsync(did[i], hid[i], word, hipMemcpyHostToDevice, s));
    }
    for (int i = 0; i < 3; ++i) {
        dout[i] = hout[i] ? reinterpret_cast<float*>(m.p + (6 + i) * quad) : nullptr;
        if (hout[i] && i != 1) LRT_HIP(hipMemcpyAsync(dout[i], hout[i], quad, hipMemcpyHostToDevice, s));
    }
    lrt_gbuffer dcur, dprev_g;
    memset(&dcur, 0, sizeof(dcur));
    memset(&dprev_g, 0, sizeof(dprev_g));
    dcur.normal = din[1];
    dcur.motion = din[2];
    dcur.id = did[0];
    dprev_g.normal = din[5];
    dprev_g.id = did[1];
    const lrt_temporal_state dprev = {din[3], din[4], nullptr, nullptr, nullptr};
    const lrt_temporal_state dnext = {dout[0], dout[1], nullptr, nullptr, nullptr};
    if (int rc = temporal_gbuffer_device(desc, din[0], &dcur, prev ? &dprev_g : nullptr, prev ? &dprev : nullptr, &dnext,
                                         dout[2], s))
        return rc;
    for (int i = 0; i < 3; ++i)
        if (hout[i]) LRT_HIP(hipMemcpyAsync(hout[i], dout[i], quad, hipMemcpyDeviceToHost, s));
    LRT_HIP(hipStreamSynchronize(s));
    return LRT_OK;
}

}  // extern "C"
