// Steps 6 and 7 of lrt_temporal_* (include/lrt.h). Step 7 and its store (temporal_std, write_std)
// serve every kernel that writes color_std: lrt_temporal.hip (the static and the moving step),
// lrt_temporal_gbuffer.hip, lrt_temporal_upsample.hip and lrt_rectify.hip. Step 6 (temporal_blend)
// serves lrt_temporal_gbuffer.hip alone: lrt_temporal.hip keeps it in its own text, which leaves its
// kernels' instructions what they were before this header existed, and
// lrt_temporal_upsample.hip blends by its own rule. The including unit sets its own contraction.
#pragma once
#include "lrt_internal.h"
#include "lrt_pixel.h"

namespace lrt {

// Step 6 where the history counts (the caller has tested sw > 1e-3): sw = sum b over the counting taps,
// sn = sum b n', sc = sum b c', sm = sum b m2'. col, m2 and n come in as the reset values (C, C^2, 1).
LRT_DEV void temporal_blend(const float sw, const float sn, const float3 sc, const float3 sm, const float3 C,
                            const float alpha_min, float3& col, float3& m2, float& n) {
    const float r = 1.0f / sw;
    n = sn * r + 1.0f;
    const float al = fmaxf(1.0f / n, alpha_min), be = (1.0f - al) * r;
    col = make_float3(be * sc.x + al * C.x, be * sc.y + al * C.y, be * sc.z + al * C.z);
    m2 = make_float3(be * sm.x + al * m2.x, be * sm.y + al * m2.y, be * sm.z + al * m2.z);
}

// Step 7: the standard deviation per channel, or short_std below min_history.
LRT_DEV float3 temporal_std(const float3 col, const float3 m2, const float n, const float short_std,
                            const float min_history) {
    float3 sd = make_float3(short_std, short_std, short_std);
    if (!(n < min_history))
        sd = make_float3(sqrtf(fmaxf(m2.x - col.x * col.x, 0.0f)), sqrtf(fmaxf(m2.y - col.y * col.y, 0.0f)),
                         sqrtf(fmaxf(m2.z - col.z * col.z, 0.0f)));
    return sd;
}
// ... stored for pixel i where the caller asked for it (12 B: the alpha stays).
LRT_DEV void write_std(float4* ostd, size_t i, const float3 col, const float3 m2, const float n, const float short_std,
                       const float min_history) {
    if (ostd) write_rgb(ostd, i, temporal_std(col, m2, n, short_std, min_history));
}

}  // namespace lrt
