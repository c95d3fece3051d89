// The pixel-centre primary ray and its closest hit: steps 1 and 2 of lrt_gbuffer_* (include/lrt.h),
// which are segment 0 of lrt_gbuffer_chain_* word for word. Both units take them from here, so the
// two passes agree bit for bit wherever the chain follows nothing. lrt_gbuffer.hip compiles to the
// instructions it had with these lines in its own text (tools/isa_same.sh). Included
// after lrt_internal.h by units built without contraction.
#pragma once
#include "lrt_trace.h"

namespace lrt {

struct PrimaryHit {
    F3 D;      // the ray's direction before the normalize (a miss's motion target)
    Ray r;     // Ray(O, D)
    int id;    // the sphere, -1 on a miss
    float t;   // along r.dir; kMaxT on a miss
};

// Pixel (x, y) of a w x h frame, rw = 1 / w and rh = 1 / h (host IEEE divisions), the camera's
// origin, lowerLeftCorner and two spans. kGrid: the uniform grid gv (else the scan over sph).
template <bool kGrid>
__device__ __forceinline__ PrimaryHit primary_hit(int x, int y, float rw, float rh, const F3& O, const F3& L,
                                                  const F3& H, const F3& V, const float4* sph, int count,
                                                  const GridView& gv) {
    PrimaryHit p;
    const float s = ((float)x + 0.5f) * rw, t = ((float)y + 0.5f) * rh;
    p.D = ((L + s * H) + t * V) - O;
    p.r = make_ray(O, p.D);
    p.id = kGrid ? ClosestHitGrid(p.r.orig, p.r.dir, gv, p.t) : ClosestHit(p.r.orig, p.r.dir, sph, count, p.t);
    return p;
}

}  // namespace lrt
