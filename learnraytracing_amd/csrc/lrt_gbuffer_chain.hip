// The chain pass (lrt_gbuffer_chain_*, include/lrt.h): the pixel-centre primary ray of lrt_gbuffer_*,
// followed through perfect and near-perfect mirrors (reflect) and through glass (refract, or reflect
// where the refraction does not exist) to the first surface that scatters diffusely. It writes that
// surface's guides and id, the throughput-tinted albedo, the path's length, the surfaces followed and
// a path key: an opaque equality key that the temporal, upsample and rectify stages take as `id`.
//
// One thread per pixel, lrt_pixel.h's 8 x 8 pixels per wave, no LDS, no atomics, whole float4 stores
// of the planes asked for. Chains differ in length inside a wave, so the walk is written with ONE
// closest-hit site per iteration that every lane of the wave reaches together: a lane whose chain
// has ended keeps its last ray and discards the result, the wave leaves the loop when no lane is
// active (a ballot), and the per-material branches only compute the next direction. The scan's loop
// is then wave-uniform and its sphere reads stay scalar loads, as in gbuffer_kernel. No contraction,
// like the render units: segment 0 is lrt_primary.h's, the bits of lrt_gbuffer_*.
#include "lrt_internal.h"
#include "lrt_pixel.h"
#include "lrt_primary.h"

namespace lrt {

struct ChainArgs {
    float4* normal;   // the seven planes, any may be null
    float4* pos;
    float4* alb;
    int* key;
    int* id;
    int* bounces;
    float* depth;
    int w, h;
    float rw, rh;           // 1 / w, 1 / h (host IEEE divisions)
    float scale;            // guide_scale
    float rough_max;        // a Metal of roughness <= rough_max is followed
    int max_bounces;
    F3 O, L, H, V;          // the camera: origin, lowerLeftCorner, the two spans
    const float4* sph;      // the scene: float4(centre, r^2), three rows per material
    const float4* mats;
    int count;
    GridView gv;            // count > kBvhMinSpheres
};

// What the walk needs of sphere id's material: the type first (a Dielectric's roughness slot holds
// schlick_r0), then the roughness of a Metal or the index of a Dielectric. The albedo row is read
// anyway: a followed Metal tints the throughput with it, the terminal surface is written with it.
struct ChainMat {
    F3 albedo;
    int type;
    float ri;
    bool delta;
};
__device__ __forceinline__ ChainMat chain_material(const float4* __restrict__ mats, int id, float rough_max) {
    ChainMat m;
    const float4 a = mats[3 * id];
    m.albedo = f3(a.x, a.y, a.z);
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

// The key's step for one further hit or miss (include/lrt.h: exact uint32 arithmetic).
__device__ __forceinline__ uint32_t chain_key_step(uint32_t h, int id) {
    h = h * 0x9E3779B1u + (uint32_t)(id + 1);
    return h ^ (h >> 15);
}

template <bool kGrid>
__global__ __launch_bounds__(kPixBlockW* kPixBlockH) void gbuffer_chain_kernel(ChainArgs a) {
    const int x = block_x(), y = block_y();
    // (a lane outside the frame walks its own, harmless ray with the wave and stores nothing: the
    // closest-hit sites below are reached by whole waves)
    const bool inside = x < a.w && y < a.h;
    // segment 0: lrt_gbuffer_*'s steps 1 and 2
    const PrimaryHit ph = primary_hit<kGrid>(x, y, a.rw, a.rh, a.O, a.L, a.H, a.V, a.sph, a.count, a.gv);
    Ray r = ph.r;
    int id = ph.id;
    float depth = ph.t;
    F3 P = f3(0.0f, 0.0f, 0.0f), n = P;
    F3 T = f3(1.0f, 1.0f, 1.0f);   // the throughput: the followed Metals' albedos
    ChainMat m;
    m.albedo = P;
    m.type = LRT_LAMBERT;
    m.ri = 1.0f;
    m.delta = false;
    if (id >= 0) {
        const float4 sp = a.sph[id];
        P = point_at(r, ph.t);
        n = normalize(P - f3(sp.x, sp.y, sp.z));
        m = chain_material(a.mats, id, a.rough_max);
    }
    uint32_t hkey = (uint32_t)id;
    int bounces = 0;
    bool active = inside && m.delta;   // the current hit is delta: its surface is followed next
    for (int k = 0; k < a.max_bounces; ++k) {
        if (__ballot(active) == 0) break;
        if (active) {
            const F3 d = r.dir;
            F3 nd;
            if (m.type == LRT_METAL) {
                nd = reflect(d, n);
                T = T * m.albedo;
            } else {   // Dielectric: Scatter's geometry (parallel.cpp:149-190) without its random choice
                const bool leaving = dot(d, n) > 0.0f;
                const F3 outwardN = leaving ? -n : n;
                const float nint = leaving ? m.ri : rcp_rn(m.ri);
                if (!refract(d, outwardN, nint, nd)) nd = reflect(d, n);   // total internal reflection
            }
            r = make_ray(P, nd);
        }
        // the one closest-hit site of the iteration: every lane of the wave is here
        float t;
        const int nid = kGrid ? ClosestHitGrid(r.orig, r.dir, a.gv, t) : ClosestHit(r.orig, r.dir, a.sph, a.count, t);
        if (active) {
            ++bounces;
            hkey = chain_key_step(hkey, nid);
            id = nid;
            depth = depth + t;
            if (nid >= 0) {
                const float4 sp = a.sph[nid];
                P = point_at(r, t);
                n = normalize(P - f3(sp.x, sp.y, sp.z));
                m = chain_material(a.mats, nid, a.rough_max);
                active = m.delta;
            } else {
                active = false;
            }
        }
    }
    if (!inside) return;
    // (active here: max_bounces surfaces were followed and the hit is still delta: unresolved)
    const size_t ip = (size_t)y * a.w + x;
    const bool hit = id >= 0;
    F3 alb = f3(0.0f, 0.0f, 0.0f);
    if (hit) alb = T * m.albedo;
    else if (bounces > 0) alb = T;   // the sky seen through the chain: the tint alone
    if (!hit) P = n = f3(0.0f, 0.0f, 0.0f);
    if (a.normal) a.normal[ip] = make_float4(a.scale * n.x, a.scale * n.y, a.scale * n.z, 0.0f);
    if (a.pos) a.pos[ip] = make_float4(a.scale * P.x, a.scale * P.y, a.scale * P.z, 0.0f);
    if (a.alb) a.alb[ip] = make_float4(a.scale * alb.x, a.scale * alb.y, a.scale * alb.z, 0.0f);
    if (a.key) a.key[ip] = bounces > 0 ? (int)(0x40000000u | (hkey & 0x3FFFFFFFu)) : id;
    if (a.id) a.id[ip] = id;
    if (a.bounces) a.bounces[ip] = bounces | (active ? LRT_CHAIN_UNRESOLVED : 0);
    if (a.depth) a.depth[ip] = hit ? depth : __builtin_inff();
}

static F3 hf3(const lrt_float3& v) { return f3(v.x, v.y, v.z); }

constexpr int kChainPlanes = 7;
static void planes_of(const lrt_gbuffer_chain_desc* d, const lrt_gbuffer_chain* o, Span out[kChainPlanes]) {
    const size_t px = (size_t)d->width * d->height;
    out[0] = {o->normal, 16 * px};
    out[1] = {o->world_pos, 16 * px};
    out[2] = {o->albedo, 16 * px};
    out[3] = {o->key, 4 * px};
    out[4] = {o->id, 4 * px};
    out[5] = {o->bounces, 4 * px};
    out[6] = {o->depth, 4 * px};
}

// Everything that needs neither the library's state nor the device.
static int validate_chain(const lrt_gbuffer_chain_desc* d, const lrt_gbuffer_chain* o) {
    if (!d) return fail(LRT_E_INVALID, "desc is NULL");
    if (!o) return fail(LRT_E_INVALID, "out is NULL");
    if (!o->normal && !o->world_pos && !o->albedo && !o->key && !o->id && !o->bounces && !o->depth)
        return fail(LRT_E_INVALID, "out needs at least one plane");
    if (int rc = validate_frame_size(d->width, d->height)) return rc;
    if (d->flags != 0 || d->reserved != 0 || d->reserved2 != 0) return fail(LRT_E_INVALID, "flags and reserved must be 0");
    if (d->max_bounces < 0 || d->max_bounces > LRT_CHAIN_MAX_BOUNCES)
        return fail(LRT_E_INVALID, "max_bounces must be 0..LRT_CHAIN_MAX_BOUNCES");
    if (!std::isfinite(d->roughness_max) || !(d->roughness_max >= 0.0f))
        return fail(LRT_E_INVALID, "roughness_max must be finite and >= 0");
    if (!std::isfinite(d->guide_scale) || !(d->guide_scale > 0.0f))
        return fail(LRT_E_INVALID, "guide_scale must be finite and > 0");
    Span pl[kChainPlanes];
    planes_of(d, o, pl);
    if (spans_alias(pl, kChainPlanes, nullptr, 0)) return fail(LRT_E_INVALID, "aliasing: two output planes overlap");
    return LRT_OK;
}

// The pass on stream s (device pointers, validated; context 0 is current).
static int chain_device(const lrt_gbuffer_chain_desc* d, const lrt_gbuffer_chain* o, hipStream_t s) {
    Context& c = ctx();
    if (c.count < 1) return fail(LRT_E_STATE, "no scene");
    const bool grid = c.count > kBvhMinSpheres;
    if (grid)
        if (int rc = ensure_grid(c)) return rc;
    if (grid && !c.grid_built) return fail(LRT_E_STATE, "the grid is not built");
    ChainArgs a;
    memset(&a, 0, sizeof(a));
    a.normal = quads(o->normal);
    a.pos = quads(o->world_pos);
    a.alb = quads(o->albedo);
    a.key = o->key;
    a.id = o->id;
    a.bounces = o->bounces;
    a.depth = o->depth;
    a.w = d->width;
    a.h = d->height;
    a.rw = 1.0f / (float)d->width;
    a.rh = 1.0f / (float)d->height;
    a.scale = d->guide_scale;
    a.rough_max = d->roughness_max;
    a.max_bounces = d->max_bounces;
    a.O = hf3(d->camera.origin);
    a.L = hf3(d->camera.lowerLeftCorner);
    a.H = hf3(d->camera.horizontalVec);
    a.V = hf3(d->camera.verticalVec);
    a.sph = c.d_sph;
    a.mats = c.d_mats;
    a.count = c.count;
    if (grid) a.gv = c.gv;
    const dim3 g = pixel_grid(a.w, a.h);
    const int b = kPixBlockW * kPixBlockH;
    if (grid) gbuffer_chain_kernel<true><<<g, b, 0, s>>>(a);
    else gbuffer_chain_kernel<false><<<g, b, 0, s>>>(a);
    LRT_HIP(hipGetLastError());
    return LRT_OK;
}

}  // namespace lrt

using namespace lrt;

extern "C" {

int lrt_gbuffer_chain_default(int width, int height, const lrt_camera* camera, lrt_gbuffer_chain_desc* out) {
    if (out && !camera) return fail(LRT_E_INVALID, "camera is NULL");
    if (int rc = frame_default_begin(out, sizeof(*out), width, height)) return rc;
    out->width = width;
    out->height = height;
    out->camera = *camera;
    out->max_bounces = 4;
    out->roughness_max = 0.25f;
    out->guide_scale = 1.0f;
    return LRT_OK;
}

int lrt_gbuffer_chain_device(const lrt_gbuffer_chain_desc* desc, const lrt_gbuffer_chain* d_out, void* stream) {
    RoctxRange rr_("lrt_gbuffer_chain_device");
    if (int rc = validate_chain(desc, d_out)) return rc;
    std::lock_guard<std::mutex> lk(g_mu);
    if (int rc = require_initialized()) return rc;
    DeviceScope ds_(0);   // context 0's device (device 0 of lrt_initialize_devices)
    return chain_device(desc, d_out, (hipStream_t)stream);
}

int lrt_gbuffer_chain_host(const lrt_gbuffer_chain_desc* desc, const lrt_gbuffer_chain* out) {
    RoctxRange rr_("lrt_gbuffer_chain_host");
    if (int rc = validate_chain(desc, out)) return rc;
    std::lock_guard<std::mutex> lk(g_mu);
    if (int rc = require_initialized()) return rc;
    DeviceScope ds_(0);
    hipStream_t s = ctx().stream;
    // every plane asked for gets a device mirror; none is copied in (whole planes are written)
    Span pl[kChainPlanes];
    planes_of(desc, out, pl);
    HostMirrors m;
    int at[kChainPlanes];
    for (int i = 0; i < kChainPlanes; ++i) at[i] = m.out(const_cast<void*>(pl[i].p), pl[i].bytes);
    if (int rc = m.alloc("hipMalloc(gbuffer chain staging)")) return rc;
    const lrt_gbuffer_chain d_out = {m.dev<float>(at[0]), m.dev<float>(at[1]), m.dev<float>(at[2]),
                                     m.dev<int32_t>(at[3]), m.dev<int32_t>(at[4]), m.dev<int32_t>(at[5]),
                                     m.dev<float>(at[6])};
    if (int rc = chain_device(desc, &d_out, s)) return rc;
    return m.download(s);
}

}  // extern "C"
