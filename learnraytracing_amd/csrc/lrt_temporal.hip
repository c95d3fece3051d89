// Temporal reprojection and accumulation (lrt_temporal_*, include/lrt.h): the first stage of
// SVGF, ahead of the denoiser. One thread per pixel finds its pixel-centre surface point in the
// previous camera, gathers the four bilinear taps of the previous state that are consistent with
// it (normal, world position, hit / miss), blends the history in and keeps a second moment. One
// launch per step, no atomics, no LDS (the reprojection offset is arbitrary per pixel: a fixed
// halo does not fit). Not bit-pinned (the reference has no such stage): contraction is allowed
// here, unlike in the render units.
//
// The moving form (lrt_temporal_accumulate_moving_*) is the same pixel function with kMove set: a
// hit pixel first finds its sphere among the scene's (a wave-uniform loop over the packed current
// spheres, read through uniform loads: no LDS, no barrier), is carried back with it, and may write
// a motion vector. The spheres come in the kernel's arguments (up to kInlineSpheres) or from the
// stream's scratch. The static instances compile without any of it.
#include "lrt_internal.h"

#pragma clang fp contract(fast)

#include "lrt_temporal_blend.h"   // step 7, under this unit's contraction

namespace lrt {

struct TemporalArgs {
    const float4* color;   // the current frame
    const float4* nrm;
    const float4* pos;
    const float4* alb;     // or null
    const float4* pc;      // the previous state (kHist launches)
    const float4* pm;
    const float4* pn;
    const float4* px;
    float4* oc;            // the next state
    float4* om;
    float4* on;
    float4* ox;
    float4* oa;            // or null (also when alb is)
    float4* ostd;          // or null
    int w, h;
    float3 O, LO, H, V;            // the camera: origin, lowerLeftCorner - origin, the two spans
    float3 pO, pa, pLO, pH, pV;    // the previous camera
    float fd, rhh, rvv;            // -(L' - O').a', 1 / H'.H', 1 / V'.V'
    float k, alpha_min, normal_min, pos_tol2, short_std, min_history;
    int same_cam;                  // the two cameras are the same bits
};

// What the moving form adds. The two arrays are packed by the host (pack_motion): sph[i] = (c_i,
// r_i), or radius -1 where sphere i is no candidate (r_i <= 0 or r'_i <= 0); psph[i] = (c'_i,
// r'_i / r_i), or ratio -1 where the sphere's eight floats are the same bits in both scenes.
struct MotionArgs {
    const float4* sph;
    const float4* psph;
    float4* motion;   // or null
    int count;
};
// (up to kInlineSpheres spheres travel in the kernel's arguments instead: InlineSpheres, lrt_internal.h)
constexpr int kMoveOff = 0, kMoveScratch = 1, kMoveInline = 2;   // temporal_pixel's kMove

LRT_DEV float3 rgb(const float4 v) { return make_float3(v.x, v.y, v.z); }
LRT_DEV float dot3(const float3 a, const float3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
LRT_DEV float3 sub3(const float3 a, const float3 b) { return make_float3(a.x - b.x, a.y - b.y, a.z - b.z); }
LRT_DEV float3 mad3(const float s, const float3 a, const float3 b) {   // s a + b
    return make_float3(s * a.x + b.x, s * a.y + b.y, s * a.z + b.z);
}

// (the pixel map, 8 x 8 pixels per wave, and why: lrt_pixel.h)
constexpr int kMatchBatch = 4;   // spheres per trip of the moving form's match loop

// One pixel of the step. kHist: there is a previous state (else every pixel is reset). kMove: the
// moving form (m is read only then), its spheres at m.sph / m.psph (kMoveScratch) or in the
// kernel's own arguments at isph (kMoveInline).
template <bool kHist, int kMove>
__device__ __forceinline__ void temporal_pixel(const TemporalArgs& a, const MotionArgs& m,
                                               const float4* isph = nullptr) {
    const float4* const sph = kMove == kMoveInline ? isph : m.sph;
    const float4* const psph = kMove == kMoveInline ? isph + m.count : m.psph;
    const int x = block_x(), y = block_y();
    if (x >= a.w || y >= a.h) return;
    const size_t ip = (size_t)y * a.w + x;
    const float k = a.k;
    const float4 c4 = a.color[ip], n4 = a.nrm[ip], x4 = a.pos[ip];
    float4 a4 = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (a.oa) a4 = a.alb[ip];
    const float3 C = make_float3(k * c4.x, k * c4.y, k * c4.z);
    const float3 N = make_float3(k * n4.x, k * n4.y, k * n4.z);
    const float3 X = make_float3(k * x4.x, k * x4.y, k * x4.z);
    float3 col = C, m2 = make_float3(C.x * C.x, C.y * C.y, C.z * C.z);
    float n = 1.0f;
    float4 mv = make_float4(0.0f, 0.0f, -1.0f, 0.0f);   // kMove: the motion vector
    if (kHist) {
        const float nn = dot3(N, N);
        const bool hit = nn >= 0.25f;
        const float u = ((float)x + 0.5f) / (float)a.w, v = ((float)y + 0.5f) / (float)a.h;
        const float3 D = mad3(v, a.V, mad3(u, a.H, a.LO));
        // the pixel centre's surface point
        float3 Xc = X;
        bool centred = false;
        if (hit) {
            const float dn = dot3(D, N);
            if (fabsf(dn) > 1e-3f * sqrtf(dot3(D, D))) {
                const float lam = dot3(sub3(X, a.O), N) / dn;
                if (lam > 0.0f) {
                    Xc = mad3(lam, D, a.O);
                    centred = true;
                }
            }
        }
        // kMove: the sphere whose point of outward normal N / |N| lies nearest X (the index is
        // wave-uniform: scalar loads; a wave of misses skips the loop), then the centre's point
        // carried back with it, Xp. Xp = Xc bit for bit unless that sphere moved.
        float3 Xp = Xc;
        bool moved = false;
        if (kMove && hit) {
            const float rn = 1.0f / sqrtf(nn);
            const float3 nh = make_float3(rn * N.x, rn * N.y, rn * N.z);
            float best = INFINITY;
            int id = -1;
            for (int i0 = 0; i0 < m.count; i0 += kMatchBatch) {
                float4 s[kMatchBatch];   // a batch of loads in flight per trip, the last one clamped
#pragma unroll
                for (int j = 0; j < kMatchBatch; ++j) s[j] = sph[min(i0 + j, m.count - 1)];
#pragma unroll
                for (int j = 0; j < kMatchBatch; ++j) {
                    const float3 e = sub3(X, mad3(s[j].w, nh, rgb(s[j])));
                    const float sc = dot3(e, e);
                    if (i0 + j < m.count && s[j].w > 0.0f && sc < best) {
                        best = sc;
                        id = i0 + j;
                    }
                }
            }
            const float3 XO0 = sub3(X, a.O);
            if (id >= 0 && best <= a.pos_tol2 * dot3(XO0, XO0)) {
                mv.z = (float)id;
                const float4 p = psph[id];
                if (p.w >= 0.0f) {
                    moved = true;
                    Xp = mad3(p.w, sub3(Xc, rgb(sph[id])), rgb(p));
                }
            }
        }
        // into the previous camera. Under the same camera a pixel-centre point (and a miss) lands
        // on its own pixel centre exactly: taken as such, because the ~1e-5 px that the f32
        // projection is off by would bleed the neighbours in at every step of a static accumulation.
        float fx, fy;
        bool ok;
        if (a.same_cam && (centred || !hit) && !moved) {
            fx = (float)x;
            fy = (float)y;
            ok = true;
        } else {
            const float3 d = hit ? sub3(Xp, a.pO) : D;
            const float da = dot3(d, a.pa);
            const float3 q = sub3(mad3(-a.fd / da, d, make_float3(0.0f, 0.0f, 0.0f)), a.pLO);
            fx = dot3(q, a.pH) * a.rhh * (float)a.w - 0.5f;
            fy = dot3(q, a.pV) * a.rvv * (float)a.h - 0.5f;
            ok = da < 0.0f && fabsf(fx) < 1e6f && fabsf(fy) < 1e6f;   // (a NaN fails both compares)
        }
        if (!ok) fx = fy = 0.0f;
        if (kMove && ok) mv.x = fx - (float)x, mv.y = fy - (float)y, mv.w = 1.0f;
        const float flx = floorf(fx), fly = floorf(fy);
        const int x0 = (int)flx, y0 = (int)fly;
        const float tx = fx - flx, ty = fy - fly;
        // the sixteen gathers issued back to back, from addresses clamped into the image
        float4 qc[4], qm[4], qn[4], qx[4];
        bool in[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int gx = x0 + (i & 1), gy = y0 + (i >> 1);
            in[i] = ok && gx >= 0 && gx < a.w && gy >= 0 && gy < a.h;
            const size_t iq = (size_t)min(max(gy, 0), a.h - 1) * a.w + min(max(gx, 0), a.w - 1);
            qn[i] = a.pn[iq];
            qx[i] = a.px[iq];
            qc[i] = a.pc[iq];
            qm[i] = a.pm[iq];
        }
        const float3 XO = sub3(Xc, a.O);
        const float lim = a.pos_tol2 * dot3(XO, XO);
        float sw = 0.0f, sn = 0.0f;
        float3 sc = make_float3(0.0f, 0.0f, 0.0f), sm = sc;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const float b = ((i & 1) ? tx : 1.0f - tx) * ((i >> 1) ? ty : 1.0f - ty);
            const float3 Np = rgb(qn[i]);
            const bool hitp = dot3(Np, Np) >= 0.25f;
            const float3 dX = sub3(rgb(qx[i]), Xp);
            const bool same = hit ? hitp && dot3(Np, N) >= a.normal_min && dot3(dX, dX) <= lim : !hitp;
            const float bw = in[i] && same ? b : 0.0f;
            sw += bw;
            sn += bw * qm[i].w;
            sc = mad3(bw, rgb(qc[i]), sc);
            sm = mad3(bw, rgb(qm[i]), sm);
        }
        if (sw > 1e-3f) {   // (temporal_blend's lines, kept here: through the call these kernels' moves reorder)
            const float r = 1.0f / sw;
            n = sn * r + 1.0f;
            const float al = fmaxf(1.0f / n, a.alpha_min), be = (1.0f - al) * r;
            col = make_float3(be * sc.x + al * C.x, be * sc.y + al * C.y, be * sc.z + al * C.z);
            m2 = make_float3(be * sm.x + al * m2.x, be * sm.y + al * m2.y, be * sm.z + al * m2.z);
        }
    }
    write_rgb(a.oc, ip, col);
    a.om[ip] = make_float4(m2.x, m2.y, m2.z, n);
    a.on[ip] = make_float4(N.x, N.y, N.z, 0.0f);
    a.ox[ip] = make_float4(X.x, X.y, X.z, 0.0f);
    if (a.oa) a.oa[ip] = make_float4(k * a4.x, k * a4.y, k * a4.z, 0.0f);
    write_std(a.ostd, ip, col, m2, n, a.short_std, a.min_history);
    if (kMove && m.motion) m.motion[ip] = mv;
}

template <bool kHist>
__global__ __launch_bounds__(kPixBlockW* kPixBlockH) void temporal_kernel(TemporalArgs a) {
    temporal_pixel<kHist, kMoveOff>(a, MotionArgs{});
}

// The moving form: the same block of 8 x 8-pixel waves.
template <bool kHist>
__global__ __launch_bounds__(kPixBlockW* kPixBlockH) void temporal_moving_kernel(TemporalArgs a, MotionArgs m) {
    temporal_pixel<kHist, kMoveScratch>(a, m);
}

// ... with the spheres in the arguments (count <= kInlineSpheres).
__global__ __launch_bounds__(kPixBlockW* kPixBlockH) void temporal_moving_inline_kernel(TemporalArgs a, MotionArgs m,
                                                                                  InlineSpheres sc) {
    temporal_pixel<true, kMoveInline>(a, m, sc.v);
}

static float3 f3(const lrt_float3& v) { return make_float3(v.x, v.y, v.z); }
static float hdot(const float3 a, const float3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
static float3 hsub(const float3 a, const float3 b) { return make_float3(a.x - b.x, a.y - b.y, a.z - b.z); }

// A step's buffers as the aliasing checks see them: the 9 inputs (the previous state's among them),
// then the 6 outputs.
struct TemporalSpans {
    Span v[15];
    TemporalSpans(const lrt_temporal_desc* d, const float* color, const lrt_features* cur, const lrt_temporal_state* prev,
                  const lrt_temporal_state* next, const float* std) {
        const lrt_temporal_state none = {};
        const lrt_temporal_state& p = prev ? *prev : none;
        const float* const all[15] = {color, cur->normal, cur->world_pos, cur->albedo, p.color, p.moment2, p.normal,
                                      p.world_pos, p.albedo, next->color, next->moment2, next->normal, next->world_pos,
                                      next->albedo, std};
        for (int i = 0; i < 15; ++i) v[i] = {all[i], (size_t)d->width * d->height * 4 * sizeof(float)};
    }
};

static int validate_temporal(const lrt_temporal_desc* d, const float* color, const lrt_features* cur,
                             const lrt_temporal_state* prev, const lrt_temporal_state* next, const float* std) {
    if (!d) return fail(LRT_E_INVALID, "desc is NULL");
    if (!color) return fail(LRT_E_INVALID, "color is NULL");
    if (!cur || !cur->normal || !cur->world_pos) return fail(LRT_E_INVALID, "cur needs normal and world_pos");
    if (!next || !next->color || !next->moment2 || !next->normal || !next->world_pos)
        return fail(LRT_E_INVALID, "next needs color, moment2, normal and world_pos");
    if (prev && (!prev->color || !prev->moment2 || !prev->normal || !prev->world_pos))
        return fail(LRT_E_INVALID, "prev needs color, moment2, normal and world_pos");
    if (int rc = validate_frame_size(d->width, d->height)) return rc;
    if (d->flags != 0 || d->reserved != 0) return fail(LRT_E_INVALID, "flags and reserved must be 0");
    if (int rc = validate_min_history(d->min_history)) return rc;
    for (float v : {d->cur_scale, d->alpha_min, d->normal_min, d->pos_tol, d->short_std})
        if (!std::isfinite(v)) return fail(LRT_E_INVALID, "parameters must be finite");
    if (!(d->cur_scale > 0.0f) || !(d->pos_tol > 0.0f) || !(d->short_std > 0.0f))
        return fail(LRT_E_INVALID, "cur_scale, pos_tol and short_std must be > 0");
    if (int rc = validate_alpha_min(d->alpha_min)) return rc;
    if (int rc = validate_normal_min(d->normal_min)) return rc;
    if (int rc = validate_prev_camera(d->prev_camera)) return rc;
    // no output may overlap an input, a prev buffer or another output
    TemporalSpans sp(d, color, cur, prev, next, std);
    if (const int al = spans_alias(sp.v + 9, 6, sp.v, 9))
        return fail(LRT_E_INVALID, al == 1 ? "aliasing: an output buffer overlaps an input or a prev buffer"
                                           : "aliasing: two output buffers overlap");
    return LRT_OK;
}

// What lrt_temporal_accumulate_moving_* checks on top of validate_temporal (which has passed).
static int validate_motion(const lrt_temporal_desc* d, const lrt_scene_motion* sm, const float* color,
                           const lrt_features* cur, const lrt_temporal_state* prev, const lrt_temporal_state* next,
                           const float* std, const float* motion) {
    if (int rc = validate_scene_motion(sm)) return rc;
    TemporalSpans sp(d, color, cur, prev, next, std);
    const Span mo = {motion, sp.v[0].bytes};
    if (spans_alias(&mo, 1, sp.v, 15)) return fail(LRT_E_INVALID, "aliasing: motion overlaps another buffer");
    return LRT_OK;
}

// The two sphere arrays as the kernels read them (MotionArgs; lrt_internal.h), 2 x count float4 into dst.
void pack_motion(const lrt_scene_motion* sm, float4* dst) {
    const int n = sm->count;
    for (int i = 0; i < n; ++i) {
        const lrt_sphere &c = sm->spheres[i], &p = sm->prev_spheres[i];
        const bool cand = c.radius > 0.0f && p.radius > 0.0f;
        const bool differs = memcmp(&c, &p, sizeof(c)) != 0;
        dst[i] = make_float4(c.center.x, c.center.y, c.center.z, cand ? c.radius : -1.0f);
        dst[n + i] = make_float4(p.center.x, p.center.y, p.center.z, cand && differs ? p.radius / c.radius : -1.0f);
    }
}

// A page-locked slot whose last upload has completed (Context::motion_slots): a free one, a new
// one, or, with kMotionSlots uploads all still in flight, the oldest after waiting for it.
static int motion_slot(Context& c, Context::MotionSlot** out) {
    for (auto& m : c.motion_slots) {
        bool done = false;
        LRT_HIP(event_done(m.ev, &done));
        if (done) {
            *out = &m;
            return LRT_OK;
        }
    }
    if ((int)c.motion_slots.size() < Context::kMotionSlots) {
        Context::MotionSlot m;
        if (hipHostMalloc(&m.h, Context::kMotionSlotBytes, hipHostMallocDefault) != hipSuccess)
            return fail(LRT_E_NOMEM, "hipHostMalloc(sphere upload)");
        const hipError_t e = hipEventCreateWithFlags(&m.ev, hipEventDisableTiming);
        if (e != hipSuccess) {
            (void)hipHostFree(m.h);
            return hip_fail(e, "hipEventCreateWithFlags");
        }
        c.motion_slots.push_back(m);
        *out = &c.motion_slots.back();
        return LRT_OK;
    }
    Context::MotionSlot& m = c.motion_slots[c.motion_next++ % Context::kMotionSlots];
    LRT_HIP(hipEventSynchronize(m.ev));
    *out = &m;
    return LRT_OK;
}

// The packed spheres into stream s's scratch, in stream order: the host arrays are read here, into
// a page-locked slot, and the copy out of it is asynchronous. *d_sph gets the device copy.
int upload_motion(const lrt_scene_motion* sm, hipStream_t s, const char* what, const float4** d_sph) {
    Context::MotionSlot* slot = nullptr;
    if (int rc = motion_slot(ctx(), &slot)) return rc;
    const size_t bytes = 2 * (size_t)sm->count * sizeof(float4);
    void* d = nullptr;
    if (int rc = scratch_or_fail(s, bytes, what, &d)) return rc;
    pack_motion(sm, static_cast<float4*>(slot->h));
    LRT_HIP(hipMemcpyAsync(d, slot->h, bytes, hipMemcpyHostToDevice, s));
    LRT_HIP(hipEventRecord(slot->ev, s));
    *d_sph = static_cast<const float4*>(d);
    return LRT_OK;
}

// The step on stream s (device pointers, validated). sm: the moving form (its spheres are read
// here: packed into the kernel's arguments, or uploaded), with motion or without.
static int temporal_device(const lrt_temporal_desc* d, const float* color, const lrt_features* cur,
                           const lrt_temporal_state* prev, const lrt_temporal_state* next, float* std,
                           hipStream_t s, const lrt_scene_motion* sm = nullptr, float* motion = nullptr) {
    MotionArgs ma;
    memset(&ma, 0, sizeof(ma));
    ma.motion = quads(motion);
    const bool inl = sm && prev && sm->count <= kInlineSpheres;   // the spheres in the kernel's arguments
    const bool upl = sm && prev && !inl;                         // ... or uploaded to the stream's scratch
    if (upl) {
        if (int rc = upload_motion(sm, s, "temporal scratch", &ma.sph)) return rc;
        ma.psph = ma.sph + sm->count;
        ma.count = sm->count;
    }
    TemporalArgs a;
    memset(&a, 0, sizeof(a));
    a.color = quads(color);
    a.nrm = quads(cur->normal);
    a.pos = quads(cur->world_pos);
    a.alb = quads(cur->albedo);
    if (prev) {
        a.pc = quads(prev->color), a.pm = quads(prev->moment2);
        a.pn = quads(prev->normal), a.px = quads(prev->world_pos);
    }
    a.oc = quads(next->color);
    a.om = quads(next->moment2);
    a.on = quads(next->normal);
    a.ox = quads(next->world_pos);
    a.oa = cur->albedo ? quads(next->albedo) : nullptr;
    a.ostd = quads(std);
    a.w = d->width;
    a.h = d->height;
    const lrt_camera &c = d->camera, &p = d->prev_camera;
    a.O = f3(c.origin);
    a.LO = hsub(f3(c.lowerLeftCorner), a.O);
    a.H = f3(c.horizontalVec);
    a.V = f3(c.verticalVec);
    a.pO = f3(p.origin);
    a.pa = f3(p.a);
    a.pLO = hsub(f3(p.lowerLeftCorner), a.pO);
    a.pH = f3(p.horizontalVec);
    a.pV = f3(p.verticalVec);
    a.fd = prev_camera_fd(p);
    a.rhh = 1.0f / hdot(a.pH, a.pH);
    a.rvv = 1.0f / hdot(a.pV, a.pV);
    a.k = d->cur_scale;
    a.alpha_min = d->alpha_min;
    a.normal_min = d->normal_min;
    a.pos_tol2 = d->pos_tol * d->pos_tol;
    a.short_std = d->short_std;
    a.min_history = (float)d->min_history;
    auto same = [](const lrt_float3& u, const lrt_float3& v) { return !memcmp(&u, &v, sizeof(u)); };
    a.same_cam = same(c.origin, p.origin) && same(c.a, p.a) && same(c.lowerLeftCorner, p.lowerLeftCorner) &&
                 same(c.horizontalVec, p.horizontalVec) && same(c.verticalVec, p.verticalVec);
    const dim3 grid = pixel_grid(a.w, a.h);
    if (inl) {
        InlineSpheres sc;
        memset(&sc, 0, sizeof(sc));
        pack_motion(sm, sc.v);
        ma.count = sm->count;
        temporal_moving_inline_kernel<<<grid, kPixBlockW * kPixBlockH, 0, s>>>(a, ma, sc);
    } else if (upl)
        temporal_moving_kernel<true><<<grid, kPixBlockW * kPixBlockH, 0, s>>>(a, ma);
    else if (sm)   // nothing to reproject into: motion is (0, 0, -1, 0)
        temporal_moving_kernel<false><<<grid, kPixBlockW * kPixBlockH, 0, s>>>(a, ma);
    else if (prev)
        temporal_kernel<true><<<grid, kPixBlockW * kPixBlockH, 0, s>>>(a);
    else
        temporal_kernel<false><<<grid, kPixBlockW * kPixBlockH, 0, s>>>(a);
    LRT_HIP(hipGetLastError());
    if (upl) LRT_HIP(stream_scratch_used(s));
    return LRT_OK;
}

}  // namespace lrt

using namespace lrt;

extern "C" {

int lrt_temporal_default(int width, int height, const lrt_camera* camera, const lrt_camera* prev_camera,
                         lrt_temporal_desc* out) {
    if (out && !camera) return fail(LRT_E_INVALID, "camera is NULL");
    if (int rc = frame_default_begin(out, sizeof(*out), width, height)) return rc;
    out->width = width;
    out->height = height;
    out->min_history = 4;
    out->camera = *camera;
    out->prev_camera = prev_camera ? *prev_camera : *camera;
    out->cur_scale = 1.0f;
    out->alpha_min = 0.05f;
    out->normal_min = 0.9f;
    out->pos_tol = 0.05f;
    out->short_std = 1e3f;
    return LRT_OK;
}

int lrt_temporal_accumulate_device(const lrt_temporal_desc* desc, const float* d_color, const lrt_features* d_cur,
                                   const lrt_temporal_state* d_prev, const lrt_temporal_state* d_next,
                                   float* d_color_std, void* stream) {
    RoctxRange rr_("lrt_temporal_accumulate_device");
    if (int rc = validate_temporal(desc, d_color, d_cur, d_prev, d_next, d_color_std)) return rc;
    std::lock_guard<std::mutex> lk(g_mu);
    if (int rc = require_initialized()) return rc;
    DeviceScope ds_(0);   // context 0's device (device 0 of lrt_initialize_devices)
    return temporal_device(desc, d_color, d_cur, d_prev, d_next, d_color_std, (hipStream_t)stream);
}

// The host forms (validated): sm and motion as temporal_device takes them.
static int temporal_host(const lrt_temporal_desc* desc, const float* color, const lrt_features* cur,
                         const lrt_temporal_state* prev, const lrt_temporal_state* next, float* color_std,
                         const lrt_scene_motion* sm, float* motion) {
    std::lock_guard<std::mutex> lk(g_mu);
    if (int rc = require_initialized()) return rc;
    DeviceScope ds_(0);
    const size_t quad = (size_t)desc->width * desc->height * 4 * sizeof(float);
    hipStream_t s = ctx().stream;
    // Every buffer that is given goes through a device mirror of its own. The two outputs whose alpha
    // stays (next->color, color_std) are copied in first.
    const lrt_temporal_state none = {};
    const lrt_temporal_state& p = prev ? *prev : none;
    HostMirrors m;
    const int color_ = m.in(color, quad), normal_ = m.in(cur->normal, quad), pos_ = m.in(cur->world_pos, quad);
    const int albedo_ = m.in(cur->albedo, quad);
    const int pcolor_ = m.in(p.color, quad), pmoment_ = m.in(p.moment2, quad), pnormal_ = m.in(p.normal, quad);
    const int ppos_ = m.in(p.world_pos, quad);
    const int ncolor_ = m.inout(next->color, quad), nmoment_ = m.out(next->moment2, quad);
    const int nnormal_ = m.out(next->normal, quad), npos_ = m.out(next->world_pos, quad);
    const int nalbedo_ = m.out(cur->albedo ? next->albedo : nullptr, quad);
    const int std_ = m.inout(color_std, quad), motion_ = m.out(motion, quad);
    if (int rc = m.alloc("hipMalloc(temporal staging)")) return rc;
    if (int rc = m.upload(s)) return rc;
    auto f = [&m](int i) { return m.dev<float>(i); };
    lrt_features dcur;
    memset(&dcur, 0, sizeof(dcur));
    dcur.normal = f(normal_);
    dcur.world_pos = f(pos_);
    dcur.albedo = f(albedo_);
    const lrt_temporal_state dprev = {f(pcolor_), f(pmoment_), f(pnormal_), f(ppos_), nullptr};
    const lrt_temporal_state dnext = {f(ncolor_), f(nmoment_), f(nnormal_), f(npos_), f(nalbedo_)};
    if (int rc = temporal_device(desc, f(color_), &dcur, prev ? &dprev : nullptr, &dnext, f(std_), s, sm, f(motion_)))
        return rc;
    return m.download(s);
}

int lrt_temporal_accumulate_host(const lrt_temporal_desc* desc, const float* color, const lrt_features* cur,
                                 const lrt_temporal_state* prev, const lrt_temporal_state* next,
                                 float* color_std) {
    RoctxRange rr_("lrt_temporal_accumulate_host");
    if (int rc = validate_temporal(desc, color, cur, prev, next, color_std)) return rc;
    return temporal_host(desc, color, cur, prev, next, color_std, nullptr, nullptr);
}

int lrt_temporal_accumulate_moving_device(const lrt_temporal_desc* desc, const lrt_scene_motion* scene,
                                          const float* d_color, const lrt_features* d_cur,
                                          const lrt_temporal_state* d_prev, const lrt_temporal_state* d_next,
                                          float* d_color_std, float* d_motion, void* stream) {
    RoctxRange rr_("lrt_temporal_accumulate_moving_device");
    if (int rc = validate_temporal(desc, d_color, d_cur, d_prev, d_next, d_color_std)) return rc;
    if (int rc = validate_motion(desc, scene, d_color, d_cur, d_prev, d_next, d_color_std, d_motion)) return rc;
    std::lock_guard<std::mutex> lk(g_mu);
    if (int rc = require_initialized()) return rc;
    DeviceScope ds_(0);
    return temporal_device(desc, d_color, d_cur, d_prev, d_next, d_color_std, (hipStream_t)stream, scene, d_motion);
}

int lrt_temporal_accumulate_moving_host(const lrt_temporal_desc* desc, const lrt_scene_motion* scene,
                                        const float* color, const lrt_features* cur, const lrt_temporal_state* prev,
                                        const lrt_temporal_state* next, float* color_std, float* motion) {
    RoctxRange rr_("lrt_temporal_accumulate_moving_host");
    if (int rc = validate_temporal(desc, color, cur, prev, next, color_std)) return rc;
    if (int rc = validate_motion(desc, scene, color, cur, prev, next, color_std, motion)) return rc;
    return temporal_host(desc, color, cur, prev, next, color_std, scene, motion);
}

}  // extern "C"
