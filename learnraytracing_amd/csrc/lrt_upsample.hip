// G-buffer-guided upsampling of a low-resolution frame (lrt_upsample_*, include/lrt.h): one thread
// per output pixel finds its four bilinear taps in the low frame with integer arithmetic, keeps
// those that show the pixel's own sphere (weighted by how well the normals agree), looks one ring
// further out where none does, and falls back to the plain bilinear mixture last. With albedo
// planes the low colours are demodulated per tap and the result is modulated by the pixel's own
// albedo. One launch, no atomics, no LDS, no barrier. No id is used as an index. Not bit-pinned:
// contraction is allowed, as in the temporal units.
#include "lrt_internal.h"
#include "lrt_pixel.h"

#pragma clang fp contract(fast)

namespace lrt {

struct UpsampleArgs {
    const float4* color;   // the low frame
    const float4* ln;      // its G-buffer: normal (null under LRT_UP_BILINEAR), albedo (or null), id
    const float4* la;
    const int* lid;
    const float4* hn;      // the output frame's G-buffer, likewise
    const float4* ha;
    const int* hid;
    float4* out;
    int* cls;              // or null
    int w, h, lw, lh;
    float kn;              // -log2(e) / sigma_normal^2
    float floor_a, weight_min;
};

constexpr int kMaxSize = 32768;   // (2x + 1) low_width stays below 2^31

// Step 1 along one axis: the first tap and the weight of the second, for output coordinate x of n
// from a low axis of nl. a = (2x + 1) nl - n lies in (-n, 2^31): the quotient is taken unsigned.
__device__ __forceinline__ void axis_taps(int x, int n, int nl, int& x0, float& t) {
    const int a = (2 * x + 1) * nl - n;
    const unsigned n2 = 2u * (unsigned)n;
    unsigned r;
    if (a < 0) {
        x0 = -1;
        r = (unsigned)(a + (int)n2);
    } else {
        const unsigned q = (unsigned)a / n2;
        x0 = (int)q;
        r = (unsigned)a - q * n2;
    }
    t = (float)r / (float)n2;
}

// c(Q) of step 5: the tap's colour, over its albedo where the tap is a hit.
template <bool kAlbedo>
__device__ __forceinline__ float3 tap_colour(const float4 c, const float4 al, int id, float floor_a) {
    if (!kAlbedo || id < 0) return make_float3(c.x, c.y, c.z);
    return make_float3(c.x / fmaxf(al.x, floor_a), c.y / fmaxf(al.y, floor_a), c.z / fmaxf(al.z, floor_a));
}

// s + w c, and s itself where w is not > 0: a tap that is skipped, refused or of weight 0 adds
// nothing, whatever its colour holds (0 x Inf would be NaN).
__device__ __forceinline__ float3 add_weighted(const float3 s, float w, const float3 c) {
    const bool on = w > 0.0f;   // selects on the operands: no branch between the taps
    const float wz = on ? w : 0.0f, cx = on ? c.x : 0.0f, cy = on ? c.y : 0.0f, cz = on ? c.z : 0.0f;
    return make_float3(wz * cx + s.x, wz * cy + s.y, wz * cz + s.z);
}

// g of step 2 for a hit: exp(-|nq - np|^2 / sigma_normal^2).
__device__ __forceinline__ float normal_weight(const float4 nq, const float4 np, float kn) {
    const float dx = nq.x - np.x, dy = nq.y - np.y, dz = nq.z - np.z;
    return __builtin_amdgcn_exp2f((dx * dx + dy * dy + dz * dz) * kn);
}

// One pixel. kBilinear: LRT_UP_BILINEAR (every pixel is class 2, no normal is read); kAlbedo: both
// albedo planes are given.
template <bool kBilinear, bool kAlbedo>
__global__ __launch_bounds__(kPixBlockW* kPixBlockH) void upsample_kernel(UpsampleArgs a) {
    const int x = block_x(), y = block_y();
    if (x >= a.w || y >= a.h) return;
    const size_t ip = (size_t)y * a.w + x;
    int x0, y0;
    float tx, ty;
    axis_taps(x, a.w, a.lw, x0, tx);
    axis_taps(y, a.h, a.lh, y0, ty);
    // the pixel's own planes and the four taps' loads issued back to back, from addresses clamped
    // into the low frame
    const int id = a.hid[ip];
    float4 n4 = make_float4(0.0f, 0.0f, 0.0f, 0.0f), ah = n4;
    if (!kBilinear) n4 = a.hn[ip];
    if (kAlbedo) ah = a.ha[ip];
    float4 qc[4], qn[4], qa[4];
    int qi[4];
    bool in[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        qn[i] = qa[i] = n4;   // (planes that are not read)
        qi[i] = -1;
        const int gx = x0 + (i & 1), gy = y0 + (i >> 1);
        in[i] = gx >= 0 && gx < a.lw && gy >= 0 && gy < a.lh;
        const size_t iq = (size_t)min(max(gy, 0), a.lh - 1) * a.lw + min(max(gx, 0), a.lw - 1);
        qc[i] = a.color[iq];
        if (!kBilinear || kAlbedo) qi[i] = a.lid[iq];
        if (!kBilinear) qn[i] = a.ln[iq];
        if (kAlbedo) qa[i] = a.la[iq];
    }
    // class 0 (the taps of the pixel's id) and class 2 (all inside taps) side by side
    float sw = 0.0f, sb = 0.0f;
    float3 s0 = make_float3(0.0f, 0.0f, 0.0f), s2 = s0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const float b = ((i & 1) ? tx : 1.0f - tx) * ((i >> 1) ? ty : 1.0f - ty);
        const float3 c = tap_colour<kAlbedo>(qc[i], qa[i], qi[i], a.floor_a);
        const float bi = in[i] ? b : 0.0f;
        sb += bi;
        s2 = add_weighted(s2, bi, c);
        if (!kBilinear) {
            const float g = id >= 0 ? normal_weight(qn[i], n4, a.kn) : 1.0f;
            const float wq = in[i] && qi[i] == id ? b * g : 0.0f;
            sw += wq;
            s0 = add_weighted(s0, wq, c);
        }
    }
    int cls = 2;
    float3 I;
    if (!kBilinear && sw >= a.weight_min) {
        cls = 0;
        I = make_float3(s0.x / sw, s0.y / sw, s0.z / sw);
    } else {
        if (!kBilinear) {
            // class 1, the cold branch: the sixteen taps one ring further out, under the tent k
            float s = 0.0f;
            float3 s1 = make_float3(0.0f, 0.0f, 0.0f);
            for (int j = 0; j < 4; ++j) {
                const int gy = y0 - 1 + j;
                const float ky = fmaxf(0.0f, 1.0f - fabsf((float)(j - 1) - ty) / 2.0f);
                const size_t row = (size_t)min(max(gy, 0), a.lh - 1) * a.lw;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int gx = x0 - 1 + i;
                    const float kx = fmaxf(0.0f, 1.0f - fabsf((float)(i - 1) - tx) / 2.0f);
                    const size_t iq = row + min(max(gx, 0), a.lw - 1);
                    const bool same = gx >= 0 && gx < a.lw && gy >= 0 && gy < a.lh && a.lid[iq] == id;
                    if (same) {
                        const float g = id >= 0 ? normal_weight(a.ln[iq], n4, a.kn) : 1.0f;
                        const float wq = kx * ky * g;
                        const float3 c = tap_colour<kAlbedo>(a.color[iq], kAlbedo ? a.la[iq] : n4, id, a.floor_a);
                        s += wq;
                        s1 = add_weighted(s1, wq, c);
                    }
                }
            }
            if (s >= a.weight_min) {
                cls = 1;
                I = make_float3(s1.x / s, s1.y / s, s1.z / s);
            }
        }
        if (cls == 2) I = make_float3(s2.x / sb, s2.y / sb, s2.z / sb);   // a tap is inside: sb >= 1/4
    }
    if (kAlbedo && id >= 0)
        I = make_float3(I.x * fmaxf(ah.x, a.floor_a), I.y * fmaxf(ah.y, a.floor_a), I.z * fmaxf(ah.z, a.floor_a));
    write_rgb(a.out, ip, I);
    if (a.cls) a.cls[ip] = cls;
}

// Everything that needs neither the library's state nor the device.
static int validate_upsample(const lrt_upsample_desc* d, const float* color_low, const lrt_gbuffer* low,
                             const lrt_gbuffer* high, const float* out, const int32_t* cls) {
    if (!d) return fail(LRT_E_INVALID, "desc is NULL");
    if (!color_low) return fail(LRT_E_INVALID, "color_low is NULL");
    if (!out) return fail(LRT_E_INVALID, "out is NULL");
    if (!low || !high || !low->id || !high->id) return fail(LRT_E_INVALID, "low and high need id");
    if (int rc = validate_frame_size(d->width, d->height)) return rc;
    if (d->low_width < 1 || d->low_height < 1) return fail(LRT_E_INVALID, "invalid image size");
    if (d->width > kMaxSize || d->height > kMaxSize)
        return fail(LRT_E_INVALID, "width and height must be <= 32768");
    if (d->low_width > d->width || d->low_height > d->height)
        return fail(LRT_E_INVALID, "the low frame must not exceed the output frame");
    if ((d->flags & ~LRT_UP_BILINEAR) != 0 || d->reserved != 0 || d->reserved2 != 0)
        return fail(LRT_E_INVALID, "unknown flag, or reserved not 0");
    for (float v : {d->sigma_normal, d->albedo_floor, d->weight_min})
        if (!std::isfinite(v) || !(v > 0.0f))
            return fail(LRT_E_INVALID, "sigma_normal, albedo_floor and weight_min must be finite and > 0");
    if (!(d->flags & LRT_UP_BILINEAR) && (!low->normal || !high->normal))
        return fail(LRT_E_INVALID, "low and high need normal");
    if (!low->albedo != !high->albedo) return fail(LRT_E_INVALID, "albedo must be given in both G-buffers, or in neither");
    // no output may overlap an input or the other output
    const size_t px = (size_t)d->width * d->height, lpx = (size_t)d->low_width * d->low_height;
    const Span outs[2] = {{out, 16 * px}, {cls, 4 * px}};
    const Span ins[7] = {{color_low, 16 * lpx}, {low->normal, 16 * lpx}, {low->albedo, 16 * lpx}, {low->id, 4 * lpx},
                         {high->normal, 16 * px}, {high->albedo, 16 * px}, {high->id, 4 * px}};
    if (const int al = spans_alias(outs, 2, ins, 7))
        return fail(LRT_E_INVALID, al == 1 ? "aliasing: an output buffer overlaps an input"
                                           : "aliasing: two output buffers overlap");
    return LRT_OK;
}

// The pass on stream s (device pointers, validated).
static int upsample_device(const lrt_upsample_desc* d, const float* color_low, const lrt_gbuffer* low,
                           const lrt_gbuffer* high, float* out, int32_t* cls, hipStream_t s) {
    UpsampleArgs a;
    memset(&a, 0, sizeof(a));
    const bool bilinear = (d->flags & LRT_UP_BILINEAR) != 0, albedo = low->albedo != nullptr;
    a.color = quads(color_low);
    a.ln = bilinear ? nullptr : quads(low->normal);
    a.la = quads(low->albedo);
    a.lid = low->id;
    a.hn = bilinear ? nullptr : quads(high->normal);
    a.ha = quads(high->albedo);
    a.hid = high->id;
    a.out = quads(out);
    a.cls = cls;
    a.w = d->width;
    a.h = d->height;
    a.lw = d->low_width;
    a.lh = d->low_height;
    a.kn = -1.44269504f / (d->sigma_normal * d->sigma_normal);
    a.floor_a = d->albedo_floor;
    a.weight_min = d->weight_min;
    const dim3 grid = pixel_grid(a.w, a.h);
    const int block = kPixBlockW * kPixBlockH;
    if (bilinear && albedo)
        upsample_kernel<true, true><<<grid, block, 0, s>>>(a);
    else if (bilinear)
        upsample_kernel<true, false><<<grid, block, 0, s>>>(a);
    else if (albedo)
        upsample_kernel<false, true><<<grid, block, 0, s>>>(a);
    else
        upsample_kernel<false, false><<<grid, block, 0, s>>>(a);
    LRT_HIP(hipGetLastError());
    return LRT_OK;
}

}  // namespace lrt

using namespace lrt;

extern "C" {

int lrt_upsample_default(int width, int height, int low_width, int low_height, lrt_upsample_desc* out) {
    if (int rc = frame_default_begin(out, sizeof(*out), std::min(width, low_width), std::min(height, low_height)))
        return rc;
    out->width = width;
    out->height = height;
    out->low_width = low_width;
    out->low_height = low_height;
    out->sigma_normal = 0.3f;
    out->albedo_floor = 0.01f;
    out->weight_min = 1e-3f;
    return LRT_OK;
}

int lrt_upsample_device(const lrt_upsample_desc* desc, const float* d_color_low, const lrt_gbuffer* d_low,
                        const lrt_gbuffer* d_high, float* d_out, int32_t* d_class, void* stream) {
    RoctxRange rr_("lrt_upsample_device");
    if (int rc = validate_upsample(desc, d_color_low, d_low, d_high, d_out, d_class)) return rc;
    std::lock_guard<std::mutex> lk(g_mu);
    if (int rc = require_initialized()) return rc;
    DeviceScope ds_(0);   // context 0's device (device 0 of lrt_initialize_devices)
    return upsample_device(desc, d_color_low, d_low, d_high, d_out, d_class, (hipStream_t)stream);
}

int lrt_upsample_host(const lrt_upsample_desc* desc, const float* color_low, const lrt_gbuffer* low,
                      const lrt_gbuffer* high, float* out, int32_t* class_out) {
    RoctxRange rr_("lrt_upsample_host");
    if (int rc = validate_upsample(desc, color_low, low, high, out, class_out)) return rc;
    std::lock_guard<std::mutex> lk(g_mu);
    if (int rc = require_initialized()) return rc;
    DeviceScope ds_(0);
    hipStream_t s = ctx().stream;
    // Every plane that is given and read goes through a device mirror of its own (LRT_UP_BILINEAR reads
    // no normal). out, whose alpha stays, is copied in first.
    const bool bilinear = (desc->flags & LRT_UP_BILINEAR) != 0;
    const size_t px = (size_t)desc->width * desc->height, lpx = (size_t)desc->low_width * desc->low_height;
    const size_t quad = 16 * px, lquad = 16 * lpx, word = 4 * px, lword = 4 * lpx;
    HostMirrors m;
    const int color_ = m.in(color_low, lquad), lnormal_ = m.in(bilinear ? nullptr : low->normal, lquad);
    const int lalbedo_ = m.in(low->albedo, lquad), lid_ = m.in(low->id, lword);
    const int hnormal_ = m.in(bilinear ? nullptr : high->normal, quad), halbedo_ = m.in(high->albedo, quad);
    const int hid_ = m.in(high->id, word);
    const int out_ = m.inout(out, quad), class_ = m.out(class_out, word);
    if (int rc = m.alloc("hipMalloc(upsample staging)")) return rc;
    if (int rc = m.upload(s)) return rc;
    lrt_gbuffer dl, dh;
    memset(&dl, 0, sizeof(dl));
    memset(&dh, 0, sizeof(dh));
    dl.normal = m.dev<float>(lnormal_);
    dl.albedo = m.dev<float>(lalbedo_);
    dl.id = m.dev<int32_t>(lid_);
    dh.normal = m.dev<float>(hnormal_);
    dh.albedo = m.dev<float>(halbedo_);
    dh.id = m.dev<int32_t>(hid_);
    if (int rc = upsample_device(desc, m.dev<float>(color_), &dl, &dh, m.dev<float>(out_), m.dev<int32_t>(class_), s))
        return rc;
    return m.download(s);
}

}  // extern "C"
