// The feature-guided denoiser (lrt_denoise_*, include/lrt.h): an edge-avoiding a-trous wavelet
// filter (Dammertz et al. 2010) over a rendered frame, guided by the first-hit normal, world
// position and albedo of lrt_features and, for the colour term, by the pixel's running colour
// standard deviation (as in SVGF). One launch per pass; pass k uses the 5x5 B3-spline taps at
// dilation s = 2^k. Not bit-pinned (the reference has no such filter): contraction and the
// hardware exp are allowed here, unlike in the render units.
#include "lrt_atrous.h"

#pragma clang fp contract(fast)

namespace lrt {

struct DenoiseArgs {
    const float4* in;    // c_k
    float4* out;         // c_{k+1}
    const float4* std;   // the guides (any may be null: its term is dropped)
    const float4* nrm;
    const float4* pos;
    const float4* alb;
    int w, h, s;         // the frame, this pass's dilation
    float sc2;           // (sigma_color * 2^-k)^2
    float kn, kx, ka;    // sqrt(log2 e) / sigma of normal, world_pos, albedo
    int rgb_only;        // the last pass: 12 B stores, the destination's alpha stays
};

// A pass over the lattice tile of lrt_atrous.h, which explains the tile, the branch-free taps and
// the anchor-relative world_pos. kStd: color_std is given (else there is no colour term).
template <bool kStd>
__global__ __launch_bounds__(kTileW* kTileRows) void denoise_kernel(DenoiseArgs a) {
    extern __shared__ float2 tile[];
    const int s = a.s, tw = kTileW + 4 * s;
    const int plane = kTileLds * tw;   // float2s per plane
    const int tx = threadIdx.x, ty = threadIdx.y;
    const int x0 = blockIdx.x * kTileW, y0 = tile_y0(s);
    if (y0 >= a.h) return;   // the whole workgroup: the last group's unused phases
    const float kn = a.kn, kx = a.kx, ka = a.ka;
    const float3 an = tile_anchor(a.pos, a.w, x0, y0, kx);   // uniform over the workgroup
    // the centre's std first: its latency passes behind the staging
    const int px = x0 + tx, py = y0 + ty * s;
    const bool live = px < a.w && py < a.h;
    float4 sd = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (kStd && live) sd = a.std[(size_t)py * a.w + px];
    // stage, straight-line: all of a thread's loads, then its LDS stores (tile_slot)
    static_assert(tile_covers(LRT_DENOISE_MAX_ITER), "two columns per thread cover the tile");
    float4 c[kTileStage], n[kTileStage], x[kTileStage], al[kTileStage];
    bool ok[kTileStage];
#pragma unroll
    for (int u = 0; u < kTileStage; ++u) {
        const size_t ig = tile_slot(u, tx, ty, x0, y0, s, tw, a.w, a.h, ok[u]);
        c[u] = a.in[ig];
        n[u] = a.nrm[ig];
        x[u] = a.pos[ig];
        al[u] = a.alb[ig];
    }
#pragma unroll
    for (int u = 0; u < kTileStage; ++u) {
        const int lr = tile_slot_row(u, ty), cx = tile_slot_col(u, tx);
        if (cx >= tw) continue;
        const bool on = ok[u] && a.nrm != a.in, ox = ok[u] && a.pos != a.in, oa = ok[u] && a.alb != a.in;
        tile_store(tile + lr * tw + cx, plane, ok[u], on, ox, oa, c[u], n[u], x[u], al[u], kn, kx, an, ka);
    }
    float inv_c = 0.0f;
    if (kStd && live) {
        inv_c = 1.44269504f / (a.sc2 * (sd.x * sd.x + sd.y * sd.y + sd.z * sd.z) + 1e-6f);
    }
    __syncthreads();
    if (!live) return;

    float hx[5], hy[5];
#pragma unroll
    for (int i = 0; i < 5; ++i) {
        const int gx = px + (i - 2) * s, gy = py + (i - 2) * s;
        hx[i] = tile_spline(i, gx, a.w);
        hy[i] = tile_spline(i, gy, a.h);
    }
    const float2* ctr = tile + (ty + 2) * tw + tx + 2 * s;
    const float2 p0 = ctr[0 * plane], p1 = ctr[1 * plane], p2 = ctr[2 * plane];
    const float2 p3 = ctr[3 * plane], p4 = ctr[4 * plane], p5 = ctr[5 * plane];
    float sr = 0.0f, sg = 0.0f, sb = 0.0f, sw = 0.0f;
#pragma unroll
    for (int j = 0; j < 5; ++j) {
        const float2* row = tile + (ty + j) * tw + tx;
        float rr = 0.0f, rg = 0.0f, rb = 0.0f, rw = 0.0f;
#pragma unroll
        for (int i = 0; i < 5; ++i) {
            const float2* q = row + i * s;
            const float2 q0 = q[0 * plane], q1 = q[1 * plane], q2 = q[2 * plane];
            const float2 q3 = q[3 * plane], q4 = q[4 * plane], q5 = q[5 * plane];
            float e = 0.0f;
            if (kStd) {
                const float dx = p0.x - q0.x, dy = p0.y - q0.y, dz = p1.x - q1.x;
                e = (dx * dx + dy * dy + dz * dz) * inv_c;
            }
            e = tile_guide_dist(e, p1, p2, p3, p4, q1, q2, q3, q4);
            float d;
            d = p4.y - q4.y, e += d * d;
            d = p5.x - q5.x, e += d * d;
            d = p5.y - q5.y, e += d * d;
            const float wq = hx[i] * __builtin_amdgcn_exp2f(-e);
            rr += wq * q0.x;
            rg += wq * q0.y;
            rb += wq * q1.x;
            rw += wq;
        }
        sr += hy[j] * rr;
        sg += hy[j] * rg;
        sb += hy[j] * rb;
        sw += hy[j] * rw;
    }
    const float r = 1.0f / sw;   // the centre tap has E = 0: sw >= 9/64
    float4* o = a.out + (size_t)py * a.w + px;
    if (a.rgb_only) {
        float* of = reinterpret_cast<float*>(o);
        of[0] = sr * r;
        of[1] = sg * r;
        of[2] = sb * r;
    } else {
        *o = make_float4(sr * r, sg * r, sb * r, 0.0f);
    }
}

static hipError_t launch_pass(DenoiseArgs a, hipStream_t s) {
    const dim3 grid = tile_grid(a.w, a.h, a.s), block(kTileW, kTileRows);
    // an absent guide reads the colour instead (a valid address) and is staged as zeros
    if (!a.nrm) a.nrm = a.in;
    if (!a.pos) a.pos = a.in;
    if (!a.alb) a.alb = a.in;
    if (a.std)
        denoise_kernel<true><<<grid, block, tile_bytes(a.s), s>>>(a);
    else
        denoise_kernel<false><<<grid, block, tile_bytes(a.s), s>>>(a);
    return hipGetLastError();
}

static int validate_denoise(const lrt_denoise_desc* d, const float* color, const lrt_features* g, const float* out) {
    if (!d) return fail(LRT_E_INVALID, "desc is NULL");
    if (!color || !out) return fail(LRT_E_INVALID, "color or out is NULL");
    if (int rc = validate_frame_size(d->width, d->height)) return rc;
    if (d->iterations < 1 || d->iterations > LRT_DENOISE_MAX_ITER)
        return fail(LRT_E_INVALID, "iterations must be in 1..LRT_DENOISE_MAX_ITER");
    if (d->flags != 0) return fail(LRT_E_INVALID, "flags must be 0");
    for (float sg : {d->sigma_color, d->sigma_normal, d->sigma_pos, d->sigma_albedo})
        if (!std::isfinite(sg) || !(sg > 0.0f)) return fail(LRT_E_INVALID, "sigmas must be finite and > 0");
    if (g)
        for (const float* p : {g->normal, g->world_pos, g->albedo, g->color_std})
            if (p && p == out) return fail(LRT_E_INVALID, "out may not be a guide buffer");
    return LRT_OK;
}

// The passes on stream s (device pointers, validated): color -> scratch -> ... -> out. The
// intermediate frames are stream s's scratch; a single in-place pass filters a copy.
static int denoise_device(const lrt_denoise_desc* d, const float* color, const lrt_features* g, float* out,
                          hipStream_t s) {
    const size_t npix = (size_t)d->width * d->height;
    const int K = d->iterations;
    const int ntmp = K == 1 ? (out == color ? 1 : 0) : K == 2 ? 1 : 2;
    float4* tmp[2] = {nullptr, nullptr};
    if (ntmp) {
        void* p = nullptr;
        if (int rc = scratch_or_fail(s, ntmp * npix * sizeof(float4), "denoise scratch", &p)) return rc;
        tmp[0] = static_cast<float4*>(p);
        tmp[1] = ntmp == 2 ? tmp[0] + npix : nullptr;
    }
    DenoiseArgs a;
    memset(&a, 0, sizeof(a));
    a.std = g ? quads(g->color_std) : nullptr;
    a.nrm = g ? quads(g->normal) : nullptr;
    a.pos = g ? quads(g->world_pos) : nullptr;
    a.alb = g ? quads(g->albedo) : nullptr;
    a.w = d->width;
    a.h = d->height;
    const float rl2e = sqrtf(1.44269504f);
    a.kn = rl2e / d->sigma_normal;
    a.kx = rl2e / d->sigma_pos;
    a.ka = rl2e / d->sigma_albedo;
    const float4* src = quads(color);
    if (K == 1 && out == color) {
        LRT_HIP(hipMemcpyAsync(tmp[0], color, npix * sizeof(float4), hipMemcpyDeviceToDevice, s));
        src = tmp[0];
    }
    for (int k = 0; k < K; ++k) {
        const bool last = k == K - 1;
        const float sc = d->sigma_color / (float)(1 << k);
        a.in = src;
        a.out = last ? quads(out) : tmp[k & 1];
        a.s = 1 << k;
        a.sc2 = sc * sc;
        a.rgb_only = last;
        LRT_HIP(launch_pass(a, s));
        src = a.out;
    }
    if (ntmp) LRT_HIP(stream_scratch_used(s));
    return LRT_OK;
}

// A device mirror of at least `bytes` in feature slot k (the staging lrt_render_host_ex uses).
static int ensure_feat(int k, size_t bytes) {
    Context& c = ctx();
    if (c.feat_bytes[k] >= bytes) return LRT_OK;
    if (c.d_feat[k]) (void)hipFree(c.d_feat[k]);
    c.d_feat[k] = nullptr;
    c.feat_bytes[k] = 0;
    if (hipMalloc(&c.d_feat[k], bytes) != hipSuccess) return fail(LRT_E_NOMEM, "hipMalloc(features)");
    c.feat_bytes[k] = bytes;
    return LRT_OK;
}

}  // namespace lrt

using namespace lrt;

extern "C" {

int lrt_denoise_default(int width, int height, lrt_denoise_desc* out) {
    if (int rc = frame_default_begin(out, sizeof(*out), width, height)) return rc;
    out->width = width;
    out->height = height;
    out->iterations = LRT_DENOISE_MAX_ITER;
    out->sigma_color = 2.0f;
    out->sigma_normal = 0.3f;
    out->sigma_pos = 0.5f;
    out->sigma_albedo = 0.2f;
    return LRT_OK;
}

int lrt_denoise_device(const lrt_denoise_desc* desc, const float* d_color, const lrt_features* d_guides,
                       float* d_out, void* stream) {
    RoctxRange rr_("lrt_denoise_device");
    if (int rc = validate_denoise(desc, d_color, d_guides, d_out)) return rc;
    std::lock_guard<std::mutex> lk(g_mu);
    if (int rc = require_initialized()) return rc;
    DeviceScope ds_(0);   // context 0's device (device 0 of lrt_initialize_devices)
    return denoise_device(desc, d_color, d_guides, d_out, (hipStream_t)stream);
}

int lrt_denoise_host(const lrt_denoise_desc* desc, const float* color, const lrt_features* guides, float* out) {
    RoctxRange rr_("lrt_denoise_host");
    if (int rc = validate_denoise(desc, color, guides, out)) return rc;
    std::lock_guard<std::mutex> lk(g_mu);
    if (int rc = require_initialized()) return rc;
    DeviceScope ds_(0);
    const size_t bytes = (size_t)desc->width * desc->height * 4 * sizeof(float);
    hipStream_t s = ctx().stream;
    // colour, the four guides and (out of place, for its alpha) the destination go through
    // device mirrors: the frame buffer, feature slots 0-3 and slot 4
    if (int rc = ensure_frame(bytes)) return rc;
    LRT_HIP(hipMemcpyAsync(ctx().d_frame, color, bytes, hipMemcpyHostToDevice, s));
    lrt_features dg;
    memset(&dg, 0, sizeof(dg));
    const float* const hp[4] = {guides ? guides->normal : nullptr, guides ? guides->world_pos : nullptr,
                                guides ? guides->albedo : nullptr, guides ? guides->color_std : nullptr};
    float** const dp[4] = {&dg.normal, &dg.world_pos, &dg.albedo, &dg.color_std};
    for (int k = 0; k < 4; ++k) {
        if (!hp[k]) continue;
        if (int rc = ensure_feat(k, bytes)) return rc;
        *dp[k] = ctx().d_feat[k];
        LRT_HIP(hipMemcpyAsync(ctx().d_feat[k], hp[k], bytes, hipMemcpyHostToDevice, s));
    }
    float* d_out = ctx().d_frame;
    if (out != color) {
        if (int rc = ensure_feat(4, bytes)) return rc;
        d_out = ctx().d_feat[4];
        LRT_HIP(hipMemcpyAsync(d_out, out, bytes, hipMemcpyHostToDevice, s));
    }
    if (int rc = denoise_device(desc, ctx().d_frame, guides ? &dg : nullptr, d_out, s)) return rc;
    LRT_HIP(hipMemcpyAsync(out, d_out, bytes, hipMemcpyDeviceToHost, s));
    LRT_HIP(hipStreamSynchronize(s));
    return LRT_OK;
}

}  // extern "C"
