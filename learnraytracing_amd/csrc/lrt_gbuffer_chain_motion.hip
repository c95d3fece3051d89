// The chain motion pass (lrt_gbuffer_chain_motion_*, include/lrt.h): for every pixel whose chain
// (lrt_gbuffer_chain_*) followed at least one surface, the position q in the PREVIOUS frame whose
// chain under the previous camera and scene ends at the same surface point, found by a fixed
// number of Gauss-Newton steps on forward differences and checked by one more evaluation. It writes
// motion = q - p in lrt_gbuffer_*'s layout where the search converged, and the first-hit motion it
// was given, bit for bit, everywhere else.
//
// gbuffer_chain_kernel's shape: one thread per pixel, lrt_pixel.h's 8 x 8 pixels per wave, no LDS,
// no atomics, whole float4 loads and stores, a scan and a grid instance. A wave none of whose lanes
// followed anything (a ballot) copies its quads and leaves. Every chain evaluation keeps the chain
// pass's discipline: ONE closest-hit site per walk iteration that every lane of the wave reaches
// together; a lane that has finished, or that is not searching, walks its last ray with the wave
// and discards the result, so the scan's loop stays wave-uniform and its sphere reads scalar. The
// evaluations under the previous camera run through one call site in one loop (three per iteration,
// then step 5's), so the walk's text is instantiated twice per kernel, not eleven times.
//
// The walk below is this unit's OWN text of lrt_gbuffer_chain.hip's (steps 2 and 3 of
// lrt_gbuffer_chain_*): that kernel has the walk inline between its own loads and stores, and a
// shared header would have to leave its instructions as they are. No contraction.
#include "lrt_internal.h"
#include "lrt_pixel.h"
#include "lrt_trace.h"

namespace lrt {

constexpr int kCmSpheres = kBvhMinSpheres;   // the scan instance's previous scene travels in the arguments

struct CmCamera {
    F3 O, L, H, V;   // origin, lowerLeftCorner, the two spans
};

struct ChainMotionArgs {
    const float4* first;   // lrt_gbuffer_*'s motion plane
    float4* motion;        // the two planes, either may be null
    int* status;
    int w, h;
    float rw, rh;           // 1 / w, 1 / h (host IEEE divisions)
    float rough_max;
    int max_bounces;
    int iterations;
    float probe, inv_probe; // probe_px and 1 / probe_px (host IEEE division)
    float step_max, converged;
    CmCamera cam, pcam;
    const float4* sph;      // the scene: float4(centre, r^2), three rows per material
    const float4* mats;
    int count;
    int moving;             // an lrt_scene_motion was given (the scan instance only)
    GridView gv;            // count > kBvhMinSpheres
};
// The scan instance's previous scene: float4(c', r'^2) as pack_scene packs the current one, and per
// sphere r' / r (one host division) where its eight floats differ between the two scenes, -1 where
// they are the same bits, -2 where r <= 0 or r' <= 0 (it did not exist in one of the frames).
struct CmPrevScene {
    float4 sph[kCmSpheres];
    float ratio[kCmSpheres];
};

struct CmMat {
    int type;
    float ri;
    bool delta;
};
__device__ __forceinline__ CmMat cm_material(const float4* __restrict__ mats, int id, float rough_max) {
    CmMat m;
    const float4 a = mats[3 * id];
    m.type = libm::f2u_i(a.w);
    m.ri = 1.0f;
    m.delta = false;
    if (m.type == LRT_METAL) {
        m.delta = mats[3 * id + 1].w <= rough_max;
    } else if (m.type == LRT_DIELECTRIC) {
        m.ri = mats[3 * id + 2].w;
        m.delta = true;
    }
    return m;
}

// chain(C, S, fx, fy) of include/lrt.h: where the walk from the continuous position (fx, fy) ends.
struct ChainEnd {
    int key;       // the path key (step 3 of lrt_gbuffer_chain_*)
    int id;        // the terminal sphere, -1: the sky
    int bounces;   // the surfaces followed
    bool open;     // max_bounces surfaces were followed and the hit is still delta: unresolved
    F3 F;          // the terminal point on a hit, the last ray's unit direction on the sky
};
// on: the lane wants the result. Every lane of the wave calls this together with a finite (fx, fy).
template <bool kGrid>
__device__ __forceinline__ ChainEnd chain_end(const CmCamera& c, float fx, float fy, bool on, const ChainMotionArgs& a,
                                              const float4* sph) {
    const float s = (fx + 0.5f) * a.rw, t = (fy + 0.5f) * a.rh;
    const F3 D = ((c.L + s * c.H) + t * c.V) - c.O;
    Ray r = make_ray(c.O, D);
    float t0;
    int id = kGrid ? ClosestHitGrid(r.orig, r.dir, a.gv, t0) : ClosestHit(r.orig, r.dir, sph, a.count, t0);
    F3 P = f3(0.0f, 0.0f, 0.0f), n = P;
    CmMat m;
    m.type = LRT_LAMBERT;
    m.ri = 1.0f;
    m.delta = false;
    if (id >= 0) {
        const float4 sp = sph[id];
        P = point_at(r, t0);
        n = normalize(P - f3(sp.x, sp.y, sp.z));
        m = cm_material(a.mats, id, a.rough_max);
    }
    uint32_t hkey = (uint32_t)id;
    int bounces = 0;
    bool active = on && m.delta;
    for (int k = 0; k < a.max_bounces; ++k) {
        if (__ballot(active) == 0) break;
        if (active) {
            const F3 d = r.dir;
            F3 nd;
            if (m.type == LRT_METAL) {
                nd = reflect(d, n);
            } else {
                const bool leaving = dot(d, n) > 0.0f;
                const F3 outwardN = leaving ? -n : n;
                const float nint = leaving ? m.ri : rcp_rn(m.ri);
                if (!refract(d, outwardN, nint, nd)) nd = reflect(d, n);
            }
            r = make_ray(P, nd);
        }
        // the one closest-hit site of the iteration: every lane of the wave is here
        float tk;
        const int nid = kGrid ? ClosestHitGrid(r.orig, r.dir, a.gv, tk) : ClosestHit(r.orig, r.dir, sph, a.count, tk);
        if (active) {
            ++bounces;
            uint32_t hk = hkey * 0x9E3779B1u + (uint32_t)(nid + 1);
            hkey = hk ^ (hk >> 15);
            id = nid;
            if (nid >= 0) {
                const float4 sp = sph[nid];
                P = point_at(r, tk);
                n = normalize(P - f3(sp.x, sp.y, sp.z));
                m = cm_material(a.mats, nid, a.rough_max);
                active = m.delta;
            } else {
                active = false;
            }
        }
    }
    ChainEnd e;
    e.key = bounces > 0 ? (int)(0x40000000u | (hkey & 0x3FFFFFFFu)) : id;
    e.id = id;
    e.bounces = bounces;
    e.open = active;
    e.F = id >= 0 ? P : r.dir;
    return e;
}

// The Gauss-Newton step of the 3 x 2 system (Jx, Jy)(dx, dy) = r by its normal equations.
__device__ __forceinline__ void cm_step(const F3& Jx, const F3& Jy, const F3& r, float& dx, float& dy) {
    const float aa = dot(Jx, Jx), bb = dot(Jx, Jy), cc = dot(Jy, Jy);
    const float e = dot(Jx, r), f = dot(Jy, r);
    const float det = aa * cc - bb * bb;
    dx = (cc * e - bb * f) / det;
    dy = (aa * f - bb * e) / det;
}

template <bool kGrid>
__device__ __forceinline__ void chain_motion_pixel(const ChainMotionArgs& a, const float4* psph, const float* pratio) {
    const int x = block_x(), y = block_y();
    // (a lane outside the frame walks its own, harmless rays with the wave, loads and stores nothing)
    const bool inside = x < a.w && y < a.h;
    const size_t ip = (size_t)y * a.w + x;
    const float xf = (float)x, yf = (float)y;
    // step 1: the chain of the current frame
    const ChainEnd cur = chain_end<kGrid>(a.cam, xf, yf, inside, a, a.sph);
    int status = LRT_CM_NOT_FOLLOWED;
    if (cur.bounces > 0) status = cur.open ? LRT_CM_UNRESOLVED : -1;   // -1: searching
    float4 fm = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (inside) fm = a.first[ip];
    if (__ballot(status < 0) == 0) {   // nothing to search in this wave
        if (inside) {
            if (a.motion) a.motion[ip] = fm;
            if (a.status) a.status[ip] = status;
        }
        return;
    }
    // step 2: the target, carried back with its sphere
    F3 Yp = cur.F;
    if (!kGrid && a.moving && status < 0 && cur.id >= 0) {
        const float ratio = pratio[cur.id];
        if (ratio == -2.0f) {
            status = LRT_CM_NO_SEED;
        } else if (ratio >= 0.0f) {
            const float4 sc = a.sph[cur.id], sp = psph[cur.id];
            Yp = f3(sp.x, sp.y, sp.z) + ratio * (cur.F - f3(sc.x, sc.y, sc.z));
        }
    }
    // step 3: the seed, if the temporal stages would take it (their step 1; a NaN fails both compares)
    float qx = xf, qy = yf;
    if (status < 0) {
        const float sx = xf + fm.x, sy = yf + fm.y;
        if (fm.w != 0.0f && fabsf(sx) < 1e6f && fabsf(sy) < 1e6f) {
            qx = sx;
            qy = sy;
        } else {
            status = LRT_CM_NO_SEED;
        }
    }
    bool search = status < 0;
    // steps 4 and 5: evaluation e of 3 iterations + 1 is F0 (e % 3 == 0), Fx or Fy; the last is step 5's
    F3 F0 = Yp, Fx = Yp, Jx = f3(0.0f, 0.0f, 0.0f), Jy = Jx;
    const int total = 3 * a.iterations + 1;
    for (int e = 0; e < total; ++e) {
        if (__ballot(search) == 0) break;
        const int ph = e % 3;
        const float px = ph == 1 ? qx + a.probe : qx, py = ph == 2 ? qy + a.probe : qy;
        const ChainEnd c = chain_end<kGrid>(a.pcam, px, py, search, a, psph);
        if (!search) continue;
        if (c.key != cur.key) {
            status = LRT_CM_KEY_LOST;
            search = false;
        } else if (ph == 1) {
            Fx = c.F;
        } else if (ph == 0 && e + 1 < total) {
            F0 = c.F;
        } else {
            float dx, dy;
            if (ph == 0) {   // step 5: the remaining step with the last Jacobian
                cm_step(Jx, Jy, Yp - c.F, dx, dy);
                const float rem = sqrt_rn(dx * dx + dy * dy);
                const bool ok = rem <= a.converged && fabsf(qx) < 1e6f && fabsf(qy) < 1e6f;   // (a NaN fails)
                status = ok ? LRT_CM_CONVERGED : LRT_CM_NOT_CONVERGED;
                search = false;
            } else {
                Jx = (Fx - F0) * a.inv_probe;
                Jy = (c.F - F0) * a.inv_probe;
                cm_step(Jx, Jy, Yp - F0, dx, dy);
                if (!(__builtin_isfinite(dx) && __builtin_isfinite(dy))) {
                    status = LRT_CM_NOT_CONVERGED;
                    search = false;
                } else {
                    const float len = sqrt_rn(dx * dx + dy * dy);
                    if (len > a.step_max) {
                        const float k = a.step_max / len;
                        dx = dx * k;
                        dy = dy * k;
                    }
                    qx = qx + dx;
                    qy = qy + dy;
                    if (!(fabsf(qx) < 1e6f && fabsf(qy) < 1e6f)) {   // step 5 would refuse it: no ray is cast there
                        status = LRT_CM_NOT_CONVERGED;
                        search = false;
                        qx = xf;
                        qy = yf;
                    }
                }
            }
        }
    }
    if (!inside) return;
    if (a.motion) a.motion[ip] = status == LRT_CM_CONVERGED ? make_float4(qx - xf, qy - yf, fm.z, 1.0f) : fm;
    if (a.status) a.status[ip] = status;
}

// The grid instance: no scene motion, the previous scene is the current one.
__global__ __launch_bounds__(kPixBlockW* kPixBlockH) void chain_motion_grid_kernel(ChainMotionArgs a) {
    chain_motion_pixel<true>(a, a.sph, nullptr);
}
// The scan instance: the previous scene in the arguments (the current one's bits where none is given).
__global__ __launch_bounds__(kPixBlockW* kPixBlockH) void chain_motion_scan_kernel(ChainMotionArgs a, CmPrevScene ps) {
    chain_motion_pixel<false>(a, ps.sph, ps.ratio);
}

static F3 hf3(const lrt_float3& v) { return f3(v.x, v.y, v.z); }
static CmCamera cm_camera(const lrt_camera& c) {
    return {hf3(c.origin), hf3(c.lowerLeftCorner), hf3(c.horizontalVec), hf3(c.verticalVec)};
}

// Everything that needs neither the library's state nor the device.
static int validate_chain_motion(const lrt_gbuffer_chain_motion_desc* d, const lrt_scene_motion* sm, const float* first,
                                 const lrt_gbuffer_chain_motion* o) {
    if (!d) return fail(LRT_E_INVALID, "desc is NULL");
    if (!o) return fail(LRT_E_INVALID, "out is NULL");
    if (!o->motion && !o->status) return fail(LRT_E_INVALID, "out needs at least one plane");
    if (int rc = validate_frame_size(d->width, d->height)) return rc;
    if (d->flags != 0 || d->reserved != 0 || d->reserved2 != 0 || d->reserved3 != 0)
        return fail(LRT_E_INVALID, "flags and reserved must be 0");
    if (d->max_bounces < 0 || d->max_bounces > LRT_CHAIN_MAX_BOUNCES)
        return fail(LRT_E_INVALID, "max_bounces must be 0..LRT_CHAIN_MAX_BOUNCES");
    if (!std::isfinite(d->roughness_max) || !(d->roughness_max >= 0.0f))
        return fail(LRT_E_INVALID, "roughness_max must be finite and >= 0");
    if (d->iterations < 1 || d->iterations > LRT_CM_MAX_ITERATIONS)
        return fail(LRT_E_INVALID, "iterations must be 1..LRT_CM_MAX_ITERATIONS");
    for (float v : {d->probe_px, d->step_max_px, d->converged_px})
        if (!std::isfinite(v) || !(v > 0.0f))
            return fail(LRT_E_INVALID, "probe_px, step_max_px and converged_px must be finite and > 0");
    if (int rc = validate_prev_camera(d->prev_camera)) return rc;
    if (!first) return fail(LRT_E_INVALID, "first_motion is NULL");
    const size_t px = (size_t)d->width * d->height;
    const Span outs[2] = {{o->motion, 16 * px}, {o->status, 4 * px}};
    const Span in = {first, 16 * px};
    if (const int al = spans_alias(outs, 2, &in, 1))
        return fail(LRT_E_INVALID, al == 1 ? "aliasing: an output overlaps first_motion" : "aliasing: the two outputs overlap");
    if (sm) {
        if (int rc = validate_scene_motion(sm)) return rc;
        if (sm->count > kCmSpheres) return fail(LRT_E_INVALID, "scene: more than 16 spheres");
    }
    return LRT_OK;
}

// The pass on stream s (device pointers, validated; context 0 is current).
static int chain_motion_device(const lrt_gbuffer_chain_motion_desc* d, const lrt_scene_motion* sm, const float* first,
                               const lrt_gbuffer_chain_motion* o, hipStream_t s) {
    Context& c = ctx();
    if (c.count < 1) return fail(LRT_E_STATE, "no scene");
    const bool grid = c.count > kBvhMinSpheres;   // (a scene given has the current scene's count: never here)
    if (grid)
        if (int rc = ensure_grid(c)) return rc;
    if (grid && !c.grid_built) return fail(LRT_E_STATE, "the grid is not built");
    ChainMotionArgs a;
    memset(&a, 0, sizeof(a));
    a.first = quads(first);
    a.motion = quads(o->motion);
    a.status = o->status;
    a.w = d->width;
    a.h = d->height;
    a.rw = 1.0f / (float)d->width;
    a.rh = 1.0f / (float)d->height;
    a.rough_max = d->roughness_max;
    a.max_bounces = d->max_bounces;
    a.iterations = d->iterations;
    a.probe = d->probe_px;
    a.inv_probe = 1.0f / d->probe_px;
    a.step_max = d->step_max_px;
    a.converged = d->converged_px;
    a.cam = cm_camera(d->camera);
    a.pcam = cm_camera(d->prev_camera);
    a.sph = c.d_sph;
    a.mats = c.d_mats;
    a.count = c.count;
    a.moving = sm != nullptr;
    const dim3 g = pixel_grid(a.w, a.h);
    const int b = kPixBlockW * kPixBlockH;
    if (grid) {
        a.gv = c.gv;
        chain_motion_grid_kernel<<<g, b, 0, s>>>(a);
    } else {
        CmPrevScene ps;
        memset(&ps, 0, sizeof(ps));
        for (int i = 0; i < c.count; ++i) {
            const lrt_sphere& cs = c.spheres[i];
            const lrt_sphere& p = sm ? sm->prev_spheres[i] : cs;
            ps.sph[i] = make_float4(p.center.x, p.center.y, p.center.z, p.radius * p.radius);
            const bool cand = cs.radius > 0.0f && p.radius > 0.0f;
            ps.ratio[i] = !cand ? -2.0f : memcmp(&cs, &p, sizeof(cs)) != 0 ? p.radius / cs.radius : -1.0f;
        }
        chain_motion_scan_kernel<<<g, b, 0, s>>>(a, ps);
    }
    LRT_HIP(hipGetLastError());
    return LRT_OK;
}

}  // namespace lrt

using namespace lrt;

extern "C" {

int lrt_gbuffer_chain_motion_default(int width, int height, const lrt_camera* camera, const lrt_camera* prev_camera,
                                     lrt_gbuffer_chain_motion_desc* out) {
    if (out && !camera) return fail(LRT_E_INVALID, "camera is NULL");
    if (int rc = frame_default_begin(out, sizeof(*out), width, height)) return rc;
    out->width = width;
    out->height = height;
    out->camera = *camera;
    out->prev_camera = prev_camera ? *prev_camera : *camera;
    out->max_bounces = 4;
    out->roughness_max = 0.25f;
    out->iterations = 3;
    out->probe_px = 0.25f;
    out->step_max_px = 16.0f;
    out->converged_px = 0.0625f;
    return LRT_OK;
}

int lrt_gbuffer_chain_motion_device(const lrt_gbuffer_chain_motion_desc* desc, const lrt_scene_motion* scene,
                                    const float* d_first_motion, const lrt_gbuffer_chain_motion* d_out, void* stream) {
    RoctxRange rr_("lrt_gbuffer_chain_motion_device");
    if (int rc = validate_chain_motion(desc, scene, d_first_motion, d_out)) return rc;
    std::lock_guard<std::mutex> lk(g_mu);
    if (int rc = validate_current_scene(scene)) return rc;
    if (int rc = require_initialized()) return rc;
    DeviceScope ds_(0);   // context 0's device (device 0 of lrt_initialize_devices)
    return chain_motion_device(desc, scene, d_first_motion, d_out, (hipStream_t)stream);
}

int lrt_gbuffer_chain_motion_host(const lrt_gbuffer_chain_motion_desc* desc, const lrt_scene_motion* scene,
                                  const float* first_motion, const lrt_gbuffer_chain_motion* out) {
    RoctxRange rr_("lrt_gbuffer_chain_motion_host");
    if (int rc = validate_chain_motion(desc, scene, first_motion, out)) return rc;
    std::lock_guard<std::mutex> lk(g_mu);
    if (int rc = validate_current_scene(scene)) return rc;
    if (int rc = require_initialized()) return rc;
    DeviceScope ds_(0);
    hipStream_t s = ctx().stream;
    const size_t px = (size_t)desc->width * desc->height;
    HostMirrors m;
    const int in = m.in(first_motion, 16 * px);
    const int mo = m.out(out->motion, 16 * px), st = m.out(out->status, 4 * px);
    if (int rc = m.alloc("hipMalloc(gbuffer chain motion staging)")) return rc;
    if (int rc = m.upload(s)) return rc;
    const lrt_gbuffer_chain_motion d_out = {m.dev<float>(mo), m.dev<int32_t>(st)};
    if (int rc = chain_motion_device(desc, scene, m.dev<float>(in), &d_out, s)) return rc;
    return m.download(s);
}

}  // extern "C"
