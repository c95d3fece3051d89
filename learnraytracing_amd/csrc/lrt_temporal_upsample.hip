// Temporal upsampling (lrt_temporal_upsample_*, include/lrt.h): a history at the output resolution
// fed by low frames whose camera is shifted by a sub-pixel jitter each step. One thread per output
// pixel does what temporal_gbuffer_kernel and upsample_kernel each do half of: it finds its four low
// taps with integer arithmetic (the jitter included), blends those of its own sphere into a current
// estimate I with a confidence beta (how near the nearest such sample lies), gathers the four
// history taps its motion vector points at, and blends the two by beta. One launch per step, no
// atomics, no LDS, no barrier. No id is used as an index. Not bit-pinned: contraction is allowed,
// as in its two parents.
#include "lrt_internal.h"

#pragma clang fp contract(fast)

#include "lrt_temporal_blend.h"   // step 7, under this unit's contraction

namespace lrt {

struct TemporalUpsampleArgs {
    const float4* color;   // the low frame
    const float4* ln;      // its G-buffer (under the jittered camera): normal, id
    const int* lid;
    const float4* nrm;     // the output frame's G-buffer (unjittered): normal, motion, id
    const float4* motion;
    const int* id;
    const float4* pc;      // the previous state's color and moment2 (kHist launches)
    const float4* pm;
    const float4* pn;      // the previous G-buffer's normal and id
    const int* pid;
    float4* oc;            // the next state's color and moment2
    float4* om;
    float4* ostd;          // or null
    int* cls;              // or null
    int w, h, lw, lh, jx, jy;
    float k;               // cur_scale
    float kn;              // -log2(e) / sigma_normal^2
    float ks;              // -log2(e) / (2 sigma_sample^2)
    float rx, ry;          // width / low_width, height / low_height
    float weight_min, alpha_min, normal_min, short_std, min_history;
};

constexpr int kMaxSize = 32768;   // (2x + 1) low_width + width stays below 2^31

// Step 1 along one axis: the first tap and the weight of the second, for output coordinate x of n
// from a low axis of nl whose samples are shifted by j / (2 n) of a low pixel, |j| <= n.
// a = (2x + 1) nl - n - j lies in (-2n, 2^31 - 2n): a + 2n is positive and fits 32 unsigned bits, so
// the true floor of a / 2n is an unsigned quotient less one.
__device__ __forceinline__ void jittered_taps(int x, int n, int nl, int j, int& x0, float& t) {
    const unsigned n2 = 2u * (unsigned)n;
    const unsigned a = (unsigned)((2 * x + 1) * nl - n - j) + n2;
    const unsigned q = a / n2;
    x0 = (int)q - 1;
    t = (float)(a - q * n2) / (float)n2;
}

// s + w c where on, s itself where not: a tap that is skipped, refused or of weight 0 adds nothing,
// whatever its colour holds (0 x Inf would be NaN).
__device__ __forceinline__ float3 add_tap(const float3 s, bool on, float w, const float4 c) {
    const float wz = on ? w : 0.0f, cx = on ? c.x : 0.0f, cy = on ? c.y : 0.0f, cz = on ? c.z : 0.0f;
    return make_float3(wz * cx + s.x, wz * cy + s.y, wz * cz + s.z);
}

// One pixel of the step. kHist: there is a previous state (else classes 2 and 3 only).
template <bool kHist>
__global__ __launch_bounds__(kPixBlockW* kPixBlockH) void temporal_upsample_kernel(TemporalUpsampleArgs a) {
    const int x = block_x(), y = block_y();
    if (x >= a.w || y >= a.h) return;
    const size_t ip = (size_t)y * a.w + x;
    int lx0, ly0;
    float ltx, lty;
    jittered_taps(x, a.w, a.lw, a.jx, lx0, ltx);
    jittered_taps(y, a.h, a.lh, a.jy, ly0, lty);
    // the pixel's own three planes, the twelve low-tap loads and the sixteen history gathers issued
    // back to back, from addresses clamped into their frames
    const int id = a.id[ip];
    const float4 n4 = a.nrm[ip];
    float4 mv = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (kHist) mv = a.motion[ip];
    float4 lc[4], ln[4];
    int li[4];
    bool lin[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int gx = lx0 + (i & 1), gy = ly0 + (i >> 1);
        lin[i] = gx >= 0 && gx < a.lw && gy >= 0 && gy < a.lh;
        const size_t iq = (size_t)min(max(gy, 0), a.lh - 1) * a.lw + min(max(gx, 0), a.lw - 1);
        li[i] = a.lid[iq];
        ln[i] = a.ln[iq];
        lc[i] = a.color[iq];
    }
    float4 qc[4], qm[4], qn[4];
    int qi[4];
    bool in[4];
    float tx = 0.0f, ty = 0.0f;
    if (kHist) {
        // a zero motion gives fx = x with no rounding: the G-buffer's static-camera guarantee carries through
        float fx = (float)x + mv.x, fy = (float)y + mv.y;
        const bool ok = mv.w != 0.0f && fabsf(fx) < 1e6f && fabsf(fy) < 1e6f;   // (a NaN fails both compares)
        if (!ok) fx = fy = 0.0f;
        const float flx = floorf(fx), fly = floorf(fy);
        const int x0 = (int)flx, y0 = (int)fly;
        tx = fx - flx;
        ty = fy - fly;
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
    }
    // step 2: the current estimate over the taps of the pixel's id (s0, sw, sk), and the plain
    // bilinear mixture of class 3 (s3, sb) beside it
    float sw = 0.0f, sk = 0.0f, sb = 0.0f;
    float3 s0 = make_float3(0.0f, 0.0f, 0.0f), s3 = s0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const float ux = (i & 1) ? ltx : 1.0f - ltx, uy = (i >> 1) ? lty : 1.0f - lty;
        const float b = ux * uy;
        // from p's centre to the tap's sample, in output pixels
        const float dx = ((float)(i & 1) - ltx) * a.rx, dy = ((float)(i >> 1) - lty) * a.ry;
        const bool inb = lin[i] && b > 0.0f;
        sb += inb ? b : 0.0f;
        s3 = add_tap(s3, inb, b, lc[i]);
        float g = 1.0f;
        if (id >= 0) {
            const float ex = ln[i].x - n4.x, ey = ln[i].y - n4.y, ez = ln[i].z - n4.z;
            g = __builtin_amdgcn_exp2f((ex * ex + ey * ey + ez * ez) * a.kn);
        }
        const float wq = b * g;
        const bool on = inb && li[i] == id && wq > 0.0f;
        const float kq = __builtin_amdgcn_exp2f((dx * dx + dy * dy) * a.ks);
        sw += on ? wq : 0.0f;
        sk += on ? wq * kq : 0.0f;
        s0 = add_tap(s0, on, wq, lc[i]);
    }
    const bool speaks = sw >= a.weight_min;
    // step 3: the history, as in temporal_gbuffer_kernel
    float hw = 0.0f, hn = 0.0f;
    float3 hc = make_float3(0.0f, 0.0f, 0.0f), hm = hc;
    if (kHist) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const float b = ((i & 1) ? tx : 1.0f - tx) * ((i >> 1) ? ty : 1.0f - ty);
            const float nd = qn[i].x * n4.x + qn[i].y * n4.y + qn[i].z * n4.z;
            const bool same = qi[i] == id && (id < 0 || nd >= a.normal_min);
            const float bw = in[i] && same ? b : 0.0f;
            hw += bw;
            hn += bw * qm[i].w;
            hc = make_float3(bw * qc[i].x + hc.x, bw * qc[i].y + hc.y, bw * qc[i].z + hc.z);
            hm = make_float3(bw * qm[i].x + hm.x, bw * qm[i].y + hm.y, bw * qm[i].z + hm.z);
        }
    }
    const bool counts = kHist && hw > 1e-3f;
    // step 4
    int cls;
    float3 col, m2;
    float n;
    if (speaks) {
        const float rs = 1.0f / sw, ki = a.k * rs, beta = sk * rs;
        const float3 I = make_float3(ki * s0.x, ki * s0.y, ki * s0.z);
        cls = 2;
        col = I;
        m2 = make_float3(I.x * I.x, I.y * I.y, I.z * I.z);
        n = beta;
        if (counts) {
            const float r = 1.0f / hw;
            cls = 0;
            n = hn * r + beta;
            // (beta = n = 0, an underflowed k over a history of count 0: fmaxf drops the 0 / 0, al = 0)
            const float al = fmaxf(beta / n, a.alpha_min * beta), be = (1.0f - al) * r;
            col = make_float3(be * hc.x + al * I.x, be * hc.y + al * I.y, be * hc.z + al * I.z);
            m2 = make_float3(be * hm.x + al * m2.x, be * hm.y + al * m2.y, be * hm.z + al * m2.z);
        }
    } else if (counts) {
        const float r = 1.0f / hw;
        cls = 1;
        col = make_float3(r * hc.x, r * hc.y, r * hc.z);
        m2 = make_float3(r * hm.x, r * hm.y, r * hm.z);
        n = hn * r;
    } else {
        const float ki = a.k / sb;   // on either axis a tap is inside with a weight > 0 (r >= 1 where X0 = -1): sb > 0
        cls = 3;
        col = make_float3(ki * s3.x, ki * s3.y, ki * s3.z);
        m2 = make_float3(col.x * col.x, col.y * col.y, col.z * col.z);
        n = 0.0f;
    }
    write_rgb(a.oc, ip, col);
    a.om[ip] = make_float4(m2.x, m2.y, m2.z, n);
    write_std(a.ostd, ip, col, m2, n, a.short_std, a.min_history);
    if (a.cls) a.cls[ip] = cls;
}

static int validate_sizes_and_jitter(int width, int height, int low_width, int low_height, int jitter_x, int jitter_y) {
    if (int rc = validate_frame_size(width, height)) return rc;
    if (low_width < 1 || low_height < 1) return fail(LRT_E_INVALID, "invalid image size");
    if (width > kMaxSize || height > kMaxSize) return fail(LRT_E_INVALID, "width and height must be <= 32768");
    if (low_width > width || low_height > height)
        return fail(LRT_E_INVALID, "the low frame must not exceed the output frame");
    if (jitter_x < -width || jitter_x > width || jitter_y < -height || jitter_y > height)
        return fail(LRT_E_INVALID, "the jitter must not exceed half a low pixel (|jitter_x| <= width, |jitter_y| <= height)");
    return LRT_OK;
}

// Everything that needs neither the library's state nor the device.
static int validate_temporal_upsample(const lrt_temporal_upsample_desc* d, const float* color_low, const lrt_gbuffer* low,
                                      const lrt_gbuffer* cur, const lrt_gbuffer* prev_g, const lrt_temporal_state* prev,
                                      const lrt_temporal_state* next, const float* std, const int32_t* cls) {
    if (!d) return fail(LRT_E_INVALID, "desc is NULL");
    if (!color_low) return fail(LRT_E_INVALID, "color_low is NULL");
    if (!low || !low->id || !low->normal) return fail(LRT_E_INVALID, "low needs id and normal");
    if (!cur || !cur->normal || !cur->motion || !cur->id) return fail(LRT_E_INVALID, "cur needs normal, motion and id");
    if (!next || !next->color || !next->moment2) return fail(LRT_E_INVALID, "next needs color and moment2");
    if (int rc = validate_history_pair(prev, prev_g)) return rc;
    if (int rc = validate_sizes_and_jitter(d->width, d->height, d->low_width, d->low_height, d->jitter_x, d->jitter_y))
        return rc;
    if (d->flags != 0 || d->reserved != 0) return fail(LRT_E_INVALID, "flags and reserved must be 0");
    if (int rc = validate_min_history(d->min_history)) return rc;
    for (float v : {d->cur_scale, d->alpha_min, d->normal_min, d->short_std, d->sigma_normal, d->sigma_sample,
                    d->weight_min})
        if (!std::isfinite(v)) return fail(LRT_E_INVALID, "parameters must be finite");
    for (float v : {d->cur_scale, d->short_std, d->sigma_normal, d->sigma_sample, d->weight_min})
        if (!(v > 0.0f))
            return fail(LRT_E_INVALID, "cur_scale, short_std, sigma_normal, sigma_sample and weight_min must be > 0");
    if (int rc = validate_alpha_min(d->alpha_min)) return rc;
    if (int rc = validate_normal_min(d->normal_min)) return rc;
    // no output may overlap an input, a previous buffer or another output
    const size_t px = (size_t)d->width * d->height, lpx = (size_t)d->low_width * d->low_height;
    const size_t quad = 16 * px, word = 4 * px;
    const Span outs[4] = {{next->color, quad}, {next->moment2, quad}, {std, quad}, {cls, word}};
    const Span ins[10] = {{cur->normal, quad}, {cur->id, word}, {cur->motion, quad},
                          {prev_g ? prev_g->normal : nullptr, quad}, {prev_g ? prev_g->id : nullptr, word},
                          {prev ? prev->color : nullptr, quad}, {prev ? prev->moment2 : nullptr, quad},
                          {color_low, 16 * lpx}, {low->normal, 16 * lpx}, {low->id, 4 * lpx}};
    if (const int al = spans_alias(outs, 4, ins, 10))
        return fail(LRT_E_INVALID, al == 1 ? "aliasing: an output buffer overlaps an input or a prev buffer"
                                           : "aliasing: two output buffers overlap");
    return validate_gbuffer_kept(ins[0], ins[1], ins[3], ins[4]);
}

// The step on stream s (device pointers, validated).
static int temporal_upsample_device(const lrt_temporal_upsample_desc* d, const float* color_low, const lrt_gbuffer* low,
                                    const lrt_gbuffer* cur, const lrt_gbuffer* prev_g, const lrt_temporal_state* prev,
                                    const lrt_temporal_state* next, float* std, int32_t* cls, hipStream_t s) {
    TemporalUpsampleArgs a;
    memset(&a, 0, sizeof(a));
    a.color = quads(color_low);
    a.ln = quads(low->normal);
    a.lid = low->id;
    a.nrm = quads(cur->normal);
    a.motion = quads(cur->motion);
    a.id = cur->id;
    if (prev) a.pc = quads(prev->color), a.pm = quads(prev->moment2), a.pn = quads(prev_g->normal), a.pid = prev_g->id;
    a.oc = quads(next->color);
    a.om = quads(next->moment2);
    a.ostd = quads(std);
    a.cls = cls;
    a.w = d->width;
    a.h = d->height;
    a.lw = d->low_width;
    a.lh = d->low_height;
    a.jx = d->jitter_x;
    a.jy = d->jitter_y;
    a.k = d->cur_scale;
    a.kn = -1.44269504f / (d->sigma_normal * d->sigma_normal);
    a.ks = -1.44269504f / (2.0f * d->sigma_sample * d->sigma_sample);
    a.rx = (float)d->width / (float)d->low_width;
    a.ry = (float)d->height / (float)d->low_height;
    a.weight_min = d->weight_min;
    a.alpha_min = d->alpha_min;
    a.normal_min = d->normal_min;
    a.short_std = d->short_std;
    a.min_history = (float)d->min_history;
    const dim3 grid = pixel_grid(a.w, a.h);
    if (prev)
        temporal_upsample_kernel<true><<<grid, kPixBlockW * kPixBlockH, 0, s>>>(a);
    else
        temporal_upsample_kernel<false><<<grid, kPixBlockW * kPixBlockH, 0, s>>>(a);
    LRT_HIP(hipGetLastError());
    return LRT_OK;
}

}  // namespace lrt

using namespace lrt;

extern "C" {

int lrt_temporal_upsample_default(int width, int height, int low_width, int low_height, lrt_temporal_upsample_desc* out) {
    if (int rc = frame_default_begin(out, sizeof(*out), std::min(width, low_width), std::min(height, low_height)))
        return rc;
    out->width = width;
    out->height = height;
    out->low_width = low_width;
    out->low_height = low_height;
    out->min_history = 4;
    out->cur_scale = 1.0f;
    out->alpha_min = 0.05f;
    out->normal_min = 0.9f;
    out->short_std = 1e3f;
    out->sigma_normal = 0.3f;
    out->sigma_sample = 0.5f;
    out->weight_min = 1e-3f;
    return LRT_OK;
}

int lrt_camera_jitter(const lrt_camera* camera, int width, int height, int low_width, int low_height, int jitter_x,
                      int jitter_y, lrt_camera* out) {
#pragma clang fp contract(off)   // each product rounded, as the header states the shift
    if (!camera || !out) return fail(LRT_E_INVALID, "camera or out is NULL");
    if (int rc = validate_sizes_and_jitter(width, height, low_width, low_height, jitter_x, jitter_y)) return rc;
    const float sx = ((float)jitter_x / (float)(2 * width)) / (float)low_width;
    const float sy = ((float)jitter_y / (float)(2 * height)) / (float)low_height;
    lrt_camera c = *camera;
    c.lowerLeftCorner.x = (c.lowerLeftCorner.x + sx * c.horizontalVec.x) + sy * c.verticalVec.x;
    c.lowerLeftCorner.y = (c.lowerLeftCorner.y + sx * c.horizontalVec.y) + sy * c.verticalVec.y;
    c.lowerLeftCorner.z = (c.lowerLeftCorner.z + sx * c.horizontalVec.z) + sy * c.verticalVec.z;
    *out = c;
    return LRT_OK;
}

int lrt_temporal_upsample_device(const lrt_temporal_upsample_desc* desc, const float* d_color_low,
                                 const lrt_gbuffer* d_low, const lrt_gbuffer* d_cur, const lrt_gbuffer* d_prev_g,
                                 const lrt_temporal_state* d_prev, const lrt_temporal_state* d_next,
                                 float* d_color_std, int32_t* d_class, void* stream) {
    RoctxRange rr_("lrt_temporal_upsample_device");
    if (int rc = validate_temporal_upsample(desc, d_color_low, d_low, d_cur, d_prev_g, d_prev, d_next, d_color_std, d_class))
        return rc;
    std::lock_guard<std::mutex> lk(g_mu);
    if (int rc = require_initialized()) return rc;
    DeviceScope ds_(0);   // context 0's device (device 0 of lrt_initialize_devices)
    return temporal_upsample_device(desc, d_color_low, d_low, d_cur, d_prev_g, d_prev, d_next, d_color_std, d_class,
                                    (hipStream_t)stream);
}

int lrt_temporal_upsample_host(const lrt_temporal_upsample_desc* desc, const float* color_low, const lrt_gbuffer* low,
                               const lrt_gbuffer* cur, const lrt_gbuffer* prev_g, const lrt_temporal_state* prev,
                               const lrt_temporal_state* next, float* color_std, int32_t* class_out) {
    RoctxRange rr_("lrt_temporal_upsample_host");
    if (int rc = validate_temporal_upsample(desc, color_low, low, cur, prev_g, prev, next, color_std, class_out)) return rc;
    std::lock_guard<std::mutex> lk(g_mu);
    if (int rc = require_initialized()) return rc;
    DeviceScope ds_(0);
    hipStream_t s = ctx().stream;
    // Every buffer that is given goes through a device mirror of its own. The two outputs whose alpha
    // stays (next->color, color_std) are copied in first.
    const size_t px = (size_t)desc->width * desc->height, lpx = (size_t)desc->low_width * desc->low_height;
    const size_t quad = 16 * px, word = 4 * px, lquad = 16 * lpx, lword = 4 * lpx;
    HostMirrors m;
    const int color_ = m.in(color_low, lquad), lnormal_ = m.in(low->normal, lquad), lid_ = m.in(low->id, lword);
    const int normal_ = m.in(cur->normal, quad), motion_ = m.in(cur->motion, quad), id_ = m.in(cur->id, word);
    const int pcolor_ = m.in(prev ? prev->color : nullptr, quad), pmoment_ = m.in(prev ? prev->moment2 : nullptr, quad);
    const int pnormal_ = m.in(prev_g ? prev_g->normal : nullptr, quad), pid_ = m.in(prev_g ? prev_g->id : nullptr, word);
    const int ncolor_ = m.inout(next->color, quad), nmoment_ = m.out(next->moment2, quad), std_ = m.inout(color_std, quad);
    const int class_ = m.out(class_out, word);
    if (int rc = m.alloc("hipMalloc(temporal upsample staging)")) return rc;
    if (int rc = m.upload(s)) return rc;
    auto f = [&m](int i) { return m.dev<float>(i); };
    lrt_gbuffer dlow, dcur, dprev_g;
    memset(&dlow, 0, sizeof(dlow));
    memset(&dcur, 0, sizeof(dcur));
    memset(&dprev_g, 0, sizeof(dprev_g));
    dlow.normal = f(lnormal_);
    dlow.id = m.dev<int32_t>(lid_);
    dcur.normal = f(normal_);
    dcur.motion = f(motion_);
    dcur.id = m.dev<int32_t>(id_);
    dprev_g.normal = f(pnormal_);
    dprev_g.id = m.dev<int32_t>(pid_);
    const lrt_temporal_state dprev = {f(pcolor_), f(pmoment_), nullptr, nullptr, nullptr};
    const lrt_temporal_state dnext = {f(ncolor_), f(nmoment_), nullptr, nullptr, nullptr};
    if (int rc = temporal_upsample_device(desc, f(color_), &dlow, &dcur, prev ? &dprev_g : nullptr, prev ? &dprev : nullptr,
                                          &dnext, f(std_), m.dev<int32_t>(class_), s))
        return rc;
    return m.download(s);
}

}  // extern "C"
