// The G-buffer pass (lrt_gbuffer_*, include/lrt.h): one primary ray per pixel through the pixel
// centre, no lens, no RNG, against the scene the library holds. One thread per pixel finds the
// closest hit with the render kernels' own functions (the linear scan up to kBvhMinSpheres
// spheres, the uniform grid above: HitWorld's bits), derives the point, the normal and the albedo,
// and, if asked, carries the point back with its sphere and projects it into the previous camera
// (steps 3a and 4 of lrt_temporal_*). One launch, no atomics, no LDS: the scan's sphere reads are
// wave-uniform (scalar loads). The pass is store-bound, up to 72 B per pixel: whole float4s, and
// only the planes asked for (uniform branches on the plane pointers). No contraction, like the
// render units: id and depth are pinned bit for bit to lrt_accel_eval.
#include "lrt_internal.h"
#include "lrt_pixel.h"
#include "lrt_primary.h"

namespace lrt {

struct GbufferArgs {
    float4* normal;   // the six planes, any may be null
    float4* pos;
    float4* alb;
    float4* motion;
    int* id;
    float* depth;
    int w, h;
    float rw, rh;                  // 1 / w, 1 / h (host IEEE divisions)
    float scale;                   // guide_scale
    F3 O, L, H, V;                 // the camera: origin, lowerLeftCorner, the two spans
    F3 pO, pa, pLO, pH, pV;        // the previous camera (motion): origin, axis, L' - O', spans
    float fd, rhh, rvv;            // -(L' - O').a', 1 / H'.H', 1 / V'.V'
    int same_cam;                  // the two cameras are the same bits
    const float4* sph;             // the scene: float4(centre, r^2), three rows per material
    const float4* mats;
    int count;
    GridView gv;                   // count > kBvhMinSpheres
    const float4* msph;            // the packed two-scene arrays (pack_motion) in the stream's
    const float4* mpsph;           // scratch (kSceneScratch), or null
};

constexpr int kSceneOff = 0, kSceneScratch = 1, kSceneInline = 2;   // gbuffer_pixel's kScene

// lrt_pixel.h's map, 8 x 8 pixels per wave: coherent primary rays keep the grid walk's cells and the
// scan's exits together, and a float4 store of the wave is eight whole 128 B lines. Timed against
// waves of 32 x 2 pixels in the same workgroup at 1280 x 720 over random_scene(1000, 1), all six
// planes, alternating in one process: 0.0242 ms against 0.0250 ms, twice each.
//
// One pixel. kGrid: the uniform grid (else the scan). kScene: an lrt_scene_motion was given, its
// packed arrays at a.msph / a.mpsph or in the kernel's own arguments at isph.
template <bool kGrid, int kScene>
__device__ __forceinline__ void gbuffer_pixel(const GbufferArgs& a, const float4* isph = nullptr) {
    const int x = block_x(), y = block_y();
    if (x >= a.w || y >= a.h) return;
    const size_t ip = (size_t)y * a.w + x;
    // steps 1 and 2, shared with lrt_gbuffer_chain.hip (its segment 0)
    const PrimaryHit ph = primary_hit<kGrid>(x, y, a.rw, a.rh, a.O, a.L, a.H, a.V, a.sph, a.count, a.gv);
    const F3 D = ph.D;
    const Ray r = ph.r;
    const float tHit = ph.t;
    const int id = ph.id;
    const bool hit = id >= 0;
    F3 P = f3(0.0f, 0.0f, 0.0f), n = P, alb = P, c = P;
    if (hit) {
        const float4 sp = a.sph[id];
        c = f3(sp.x, sp.y, sp.z);
        P = point_at(r, tHit);
        n = normalize(P - c);
        if (a.alb) {
            const float4 m = a.mats[3 * id];
            alb = f3(m.x, m.y, m.z);
        }
    }
    if (a.normal) a.normal[ip] = make_float4(a.scale * n.x, a.scale * n.y, a.scale * n.z, 0.0f);
    if (a.pos) a.pos[ip] = make_float4(a.scale * P.x, a.scale * P.y, a.scale * P.z, 0.0f);
    if (a.alb) a.alb[ip] = make_float4(a.scale * alb.x, a.scale * alb.y, a.scale * alb.z, 0.0f);
    if (a.id) a.id[ip] = id;
    if (a.depth) a.depth[ip] = hit ? tHit : __builtin_inff();
    if (!a.motion) return;
    // the point carried back with its sphere (3a): Xp = P bit for bit unless that sphere moved;
    // gone: it was not there in the previous frame
    F3 Xp = P;
    bool moved = false, gone = false;
    if (kScene != kSceneOff && hit) {
        const float4* const sph = kScene == kSceneInline ? isph : a.msph;
        const float4* const psph = kScene == kSceneInline ? isph + a.count : a.mpsph;
        const float4 q = psph[id];
        gone = sph[id].w < 0.0f;
        if (q.w >= 0.0f) {
            moved = true;
            Xp = f3(q.x, q.y, q.z) + q.w * (P - c);
        }
    }
    // into the previous camera (4). Under the same camera an unmoved point (and a miss) lands on
    // its own pixel centre exactly, and is taken as such (lrt_temporal.hip)
    float fx, fy;
    bool ok;
    if (a.same_cam && !moved) {
        fx = (float)x;
        fy = (float)y;
        ok = true;
    } else {
        const F3 d = hit ? Xp - a.pO : D;
        const float da = dot(d, a.pa);
        const F3 q = (-a.fd / da) * d - a.pLO;
        fx = dot(q, a.pH) * a.rhh * (float)a.w - 0.5f;
        fy = dot(q, a.pV) * a.rvv * (float)a.h - 0.5f;
        ok = da < 0.0f && fabsf(fx) < 1e6f && fabsf(fy) < 1e6f;   // (a NaN fails both compares)
    }
    ok = ok && !gone;
    a.motion[ip] = ok ? make_float4(fx - (float)x, fy - (float)y, (float)id, 1.0f)
                      : make_float4(0.0f, 0.0f, (float)id, 0.0f);
}

template <bool kGrid, bool kScene>
__global__ __launch_bounds__(kPixBlockW* kPixBlockH) void gbuffer_kernel(GbufferArgs a) {
    gbuffer_pixel<kGrid, kScene ? kSceneScratch : kSceneOff>(a);
}
// ... with the two scenes' spheres in the arguments (count <= kInlineSpheres).
template <bool kGrid>
__global__ __launch_bounds__(kPixBlockW* kPixBlockH) void gbuffer_inline_kernel(GbufferArgs a, InlineSpheres sc) {
    gbuffer_pixel<kGrid, kSceneInline>(a, sc.v);
}

static F3 hf3(const lrt_float3& v) { return f3(v.x, v.y, v.z); }

struct Plane {
    const void* p;
    size_t bytes;
};
static void planes_of(const lrt_gbuffer_desc* d, const lrt_gbuffer* o, Plane out[6]) {
    const size_t px = (size_t)d->width * d->height;
    out[0] = {o->normal, 16 * px};
    out[1] = {o->world_pos, 16 * px};
    out[2] = {o->albedo, 16 * px};
    out[3] = {o->motion, 16 * px};
    out[4] = {o->id, 4 * px};
    out[5] = {o->depth, 4 * px};
}

// Everything that needs neither the library's state nor the device.
static int validate_gbuffer(const lrt_gbuffer_desc* d, const lrt_scene_motion* sm, const lrt_gbuffer* o) {
    if (!d) return fail(LRT_E_INVALID, "desc is NULL");
    if (!o) return fail(LRT_E_INVALID, "out is NULL");
    if (!o->normal && !o->world_pos && !o->albedo && !o->motion && !o->id && !o->depth)
        return fail(LRT_E_INVALID, "out needs at least one plane");
    if (int rc = validate_frame_size(d->width, d->height)) return rc;
    if (d->flags != 0 || d->reserved != 0 || d->reserved2 != 0) return fail(LRT_E_INVALID, "flags and reserved must be 0");
    if (!std::isfinite(d->guide_scale) || !(d->guide_scale > 0.0f))
        return fail(LRT_E_INVALID, "guide_scale must be finite and > 0");
    Plane pl[6];
    planes_of(d, o, pl);
    for (int i = 0; i < 6; ++i)
        for (int j = i + 1; j < 6; ++j)
            if (ranges_overlap(pl[i].p, pl[i].bytes, pl[j].p, pl[j].bytes))
                return fail(LRT_E_INVALID, "aliasing: two output planes overlap");
    if (o->motion)
        if (int rc = validate_prev_camera(d->prev_camera)) return rc;
    if (sm)
        if (int rc = validate_scene_motion(sm)) return rc;
    return LRT_OK;
}

// The pass on stream s (device pointers, validated; context 0 is current).
static int gbuffer_device(const lrt_gbuffer_desc* d, const lrt_scene_motion* sm, const lrt_gbuffer* o, hipStream_t s) {
    Context& c = ctx();
    if (c.count < 1) return fail(LRT_E_STATE, "no scene");
    const bool grid = c.count > kBvhMinSpheres;
    if (grid)
        if (int rc = ensure_grid(c)) return rc;
    if (grid && !c.grid_built) return fail(LRT_E_STATE, "the grid is not built");
    GbufferArgs a;
    memset(&a, 0, sizeof(a));
    a.normal = quads(o->normal);
    a.pos = quads(o->world_pos);
    a.alb = quads(o->albedo);
    a.motion = quads(o->motion);
    a.id = o->id;
    a.depth = o->depth;
    a.w = d->width;
    a.h = d->height;
    a.rw = 1.0f / (float)d->width;
    a.rh = 1.0f / (float)d->height;
    a.scale = d->guide_scale;
    const lrt_camera &cam = d->camera, &p = d->prev_camera;
    a.O = hf3(cam.origin);
    a.L = hf3(cam.lowerLeftCorner);
    a.H = hf3(cam.horizontalVec);
    a.V = hf3(cam.verticalVec);
    a.sph = c.d_sph;
    a.mats = c.d_mats;
    a.count = c.count;
    if (grid) a.gv = c.gv;
    const bool scene = sm && o->motion;   // (without motion the two scenes are not read)
    const bool inl = scene && sm->count <= kInlineSpheres;
    const bool upl = scene && !inl;
    if (o->motion) {
        a.pO = hf3(p.origin);
        a.pa = hf3(p.a);
        a.pLO = hf3(p.lowerLeftCorner) - a.pO;
        a.pH = hf3(p.horizontalVec);
        a.pV = hf3(p.verticalVec);
        a.fd = prev_camera_fd(p);
        a.rhh = 1.0f / dot(a.pH, a.pH);
        a.rvv = 1.0f / dot(a.pV, a.pV);
        auto same = [](const lrt_float3& u, const lrt_float3& v) { return !memcmp(&u, &v, sizeof(u)); };
        a.same_cam = same(cam.origin, p.origin) && same(cam.a, p.a) && same(cam.lowerLeftCorner, p.lowerLeftCorner) &&
                     same(cam.horizontalVec, p.horizontalVec) && same(cam.verticalVec, p.verticalVec);
    }
    if (upl) {
        if (int rc = upload_motion(sm, s, "gbuffer scratch", &a.msph)) return rc;
        a.mpsph = a.msph + sm->count;
    }
    const dim3 g = pixel_grid(a.w, a.h);
    const int b = kPixBlockW * kPixBlockH;
    if (inl) {
        InlineSpheres sc;
        memset(&sc, 0, sizeof(sc));
        pack_motion(sm, sc.v);
        if (grid) gbuffer_inline_kernel<true><<<g, b, 0, s>>>(a, sc);
        else gbuffer_inline_kernel<false><<<g, b, 0, s>>>(a, sc);
    } else if (grid) {
        if (upl) gbuffer_kernel<true, true><<<g, b, 0, s>>>(a);
        else gbuffer_kernel<true, false><<<g, b, 0, s>>>(a);
    } else {   // (a scan scene's two arrays always fit the arguments)
        gbuffer_kernel<false, false><<<g, b, 0, s>>>(a);
    }
    LRT_HIP(hipGetLastError());
    if (upl) LRT_HIP(stream_scratch_used(s));
    return LRT_OK;
}

}  // namespace lrt

using namespace lrt;

extern "C" {

int lrt_gbuffer_default(int width, int height, const lrt_camera* camera, const lrt_camera* prev_camera,
                        lrt_gbuffer_desc* out) {
    if (out && !camera) return fail(LRT_E_INVALID, "camera is NULL");
    if (int rc = frame_default_begin(out, sizeof(*out), width, height)) return rc;
    out->width = width;
    out->height = height;
    out->camera = *camera;
    out->prev_camera = prev_camera ? *prev_camera : *camera;
    out->guide_scale = 1.0f;
    return LRT_OK;
}

int lrt_gbuffer_device(const lrt_gbuffer_desc* desc, const lrt_scene_motion* scene, const lrt_gbuffer* d_out,
                       void* stream) {
    RoctxRange rr_("lrt_gbuffer_device");
    if (int rc = validate_gbuffer(desc, scene, d_out)) return rc;
    std::lock_guard<std::mutex> lk(g_mu);
    if (int rc = validate_current_scene(scene)) return rc;
    if (int rc = require_initialized()) return rc;
    DeviceScope ds_(0);   // context 0's device (device 0 of lrt_initialize_devices)
    return gbuffer_device(desc, scene, d_out, (hipStream_t)stream);
}

int lrt_gbuffer_host(const lrt_gbuffer_desc* desc, const lrt_scene_motion* scene, const lrt_gbuffer* out) {
    RoctxRange rr_("lrt_gbuffer_host");
    if (int rc = validate_gbuffer(desc, scene, out)) return rc;
    std::lock_guard<std::mutex> lk(g_mu);
    if (int rc = validate_current_scene(scene)) return rc;
    if (int rc = require_initialized()) return rc;
    DeviceScope ds_(0);
    hipStream_t s = ctx().stream;
    // every plane asked for gets a device mirror; none is copied in (whole planes are written)
    Plane pl[6];
    planes_of(desc, out, pl);
    HostMirrors m;
    int at[6];
    for (int i = 0; i < 6; ++i) at[i] = m.out(const_cast<void*>(pl[i].p), pl[i].bytes);
    if (int rc = m.alloc("hipMalloc(gbuffer staging)")) return rc;
    const lrt_gbuffer d_out = {m.dev<float>(at[0]), m.dev<float>(at[1]), m.dev<float>(at[2]),
                               m.dev<float>(at[3]), m.dev<int32_t>(at[4]), m.dev<float>(at[5])};
    if (int rc = gbuffer_device(desc, scene, &d_out, s)) return rc;
    return m.download(s);
}

}  // extern "C"
