// The variance-guided filter over the temporal state (lrt_svgf_*, include/lrt.h): stages 2 and 3
// of SVGF (Schied et al. 2017). A stage-0 launch estimates each pixel's variance (from its temporal
// moments, or from its 7x7 neighbourhood where the history is short) and divides the albedo out;
// then one launch per a-trous pass, pass k at dilation s = 2^k, filters colour and variance
// together, the colour weight scaled by the 3x3 pre-filtered variance of the pass's own input.
// Not bit-pinned (the reference has no such filter): contraction and the hardware exp are allowed
// here, unlike in the render units.
#include "lrt_atrous.h"

#pragma clang fp contract(fast)

namespace lrt {

struct SvgfArgs {
    const float4* cin;    // stage 0: the state's colour; a pass: c_k
    const float4* vin;    // stage 0: the state's moment2 (n in its alpha); a pass: var_k
    float4* cout;         // c_0 / c_{k+1} (the last pass: out)
    float4* vout;         // var_0 / var_{k+1} (the last pass: variance_out, or null)
    const float4* nrm;    // the guides; an absent one points at cin (a valid address) with its has_ flag 0
    const float4* pos;
    const float4* alb;
    int has_n, has_x, has_a;
    int last;             // the last pass: times D, 12 B stores (the destinations' alphas stay), vout may be null
    int w, h, s;          // the frame, this pass's dilation
    float sc2;            // sigma_color^2
    float kn, kx;         // sqrt(log2 e) / sigma of normal, world_pos
    float floor_a;        // albedo_floor
    float min_history;
};

// The demodulation divisor of a pixel from its raw normal and albedo quads.
LRT_DEV float3 divisor(const SvgfArgs& a, const float4 n4, const float4 a4) {
    const bool hit = !a.has_n || n4.x * n4.x + n4.y * n4.y + n4.z * n4.z >= 0.25f;
    if (!a.has_a || !hit) return make_float3(1.0f, 1.0f, 1.0f);
    return make_float3(fmaxf(a4.x, a.floor_a), fmaxf(a4.y, a.floor_a), fmaxf(a4.z, a.floor_a));
}

// ---- stage 0. A workgroup takes k0W x k0H pixels, a wave two rows of 32 (its streamed accesses
// are whole 512 B runs). The 7x7 spatial estimate runs only where n < min_history; a workgroup
// that holds such a pixel (a workgroup-wide vote on the centres' n) stages its tile plus a halo
// of 3 in LDS first -- colour, moment, normal and position, alphas dropped: 12 floats per pixel
// as six float2 planes, the guides divided by their sigma and world_pos relative to the
// workgroup's first pixel (tile_anchor, as the pass kernel stages them) -- so that a first frame,
// where every pixel takes that branch, reads 2.1 pixels per pixel from memory and its 49 taps
// from LDS. A workgroup with history everywhere stages nothing.
constexpr int k0W = 32, k0H = 8, k0R = 3;
constexpr int k0TW = k0W + 2 * k0R, k0TH = k0H + 2 * k0R, k0Tile = k0TW * k0TH;
constexpr int k0Stage = (k0Tile + k0W * k0H - 1) / (k0W * k0H);

__global__ __launch_bounds__(k0W* k0H) void svgf_stage0_kernel(SvgfArgs a) {
    __shared__ float2 tile[6 * k0Tile];
    const int t = threadIdx.x;
    const int tx = t % k0W, ty = t / k0W;
    const int x0 = blockIdx.x * k0W, y0 = blockIdx.y * k0H;
    const int px = x0 + tx, py = y0 + ty;
    const bool live = px < a.w && py < a.h;
    const size_t ip = (size_t)min(py, a.h - 1) * a.w + min(px, a.w - 1);
    const float4 c4 = a.cin[ip], m4 = a.vin[ip], n4 = a.nrm[ip], a4 = a.alb[ip];
    const bool spatial = live && !(m4.w >= a.min_history);
    float3 v = make_float3(fmaxf(m4.x - c4.x * c4.x, 0.0f), fmaxf(m4.y - c4.y * c4.y, 0.0f),
                           fmaxf(m4.z - c4.z * c4.z, 0.0f));
    if (__syncthreads_or(spatial)) {   // uniform over the workgroup
        const float kn = a.kn, kx = a.kx;
        const float3 an = tile_anchor(a.pos, a.w, x0, y0, kx);
        // straight-line staging: every load is issued, from an address clamped into the image (and
        // into the tile), before the first LDS store waits for one
        float4 c[k0Stage], m[k0Stage], n[k0Stage], x[k0Stage];
#pragma unroll
        for (int u = 0; u < k0Stage; ++u) {
            const int id = min(t + u * (k0W * k0H), k0Tile - 1);
            const int gy = min(max(y0 - k0R + id / k0TW, 0), a.h - 1), gx = min(max(x0 - k0R + id % k0TW, 0), a.w - 1);
            const size_t ig = (size_t)gy * a.w + gx;
            c[u] = a.cin[ig];
            m[u] = a.vin[ig];
            n[u] = a.nrm[ig];
            x[u] = a.pos[ig];
        }
#pragma unroll
        for (int u = 0; u < k0Stage; ++u) {
            const int id = t + u * (k0W * k0H);
            if (id >= k0Tile) continue;
            const bool on = a.has_n, ox = a.has_x;
            float2* q = tile + id;
            q[0 * k0Tile] = make_float2(c[u].x, c[u].y);
            q[1 * k0Tile] = make_float2(c[u].z, m[u].x);
            q[2 * k0Tile] = make_float2(m[u].y, m[u].z);
            q[3 * k0Tile] = make_float2(on ? n[u].x * kn : 0.0f, on ? n[u].y * kn : 0.0f);
            q[4 * k0Tile] = make_float2(on ? n[u].z * kn : 0.0f, ox ? fmaf(x[u].x, kx, an.x) : 0.0f);
            q[5 * k0Tile] = make_float2(ox ? fmaf(x[u].y, kx, an.y) : 0.0f, ox ? fmaf(x[u].z, kx, an.z) : 0.0f);
        }
        __syncthreads();
        if (spatial) {
            // an out-of-image tap was staged from a clamped address and gets a zero weight
            float inx[7];
#pragma unroll
            for (int i = 0; i < 7; ++i) inx[i] = px + i - k0R >= 0 && px + i - k0R < a.w ? 1.0f : 0.0f;
            const float2* ctr = tile + (ty + k0R) * k0TW + tx + k0R;
            const float2 p3 = ctr[3 * k0Tile], p4 = ctr[4 * k0Tile], p5 = ctr[5 * k0Tile];
            float sg = 0.0f;
            float3 s1 = make_float3(0.0f, 0.0f, 0.0f), s2 = s1;
            for (int j = 0; j < 7; ++j) {
                const float2* row = tile + (ty + j) * k0TW + tx;
                const float iny = py + j - k0R >= 0 && py + j - k0R < a.h ? 1.0f : 0.0f;
#pragma unroll
                for (int i = 0; i < 7; ++i) {
                    const float2* q = row + i;
                    const float2 q0 = q[0 * k0Tile], q1 = q[1 * k0Tile], q2 = q[2 * k0Tile];
                    const float2 q3 = q[3 * k0Tile], q4 = q[4 * k0Tile], q5 = q[5 * k0Tile];
                    float d, e = 0.0f;
                    d = p3.x - q3.x, e += d * d;
                    d = p3.y - q3.y, e += d * d;
                    d = p4.x - q4.x, e += d * d;
                    d = p4.y - q4.y, e += d * d;
                    d = p5.x - q5.x, e += d * d;
                    d = p5.y - q5.y, e += d * d;
                    const float g = inx[i] * iny * __builtin_amdgcn_exp2f(-e);
                    sg += g;
                    s1.x += g * q0.x, s1.y += g * q0.y, s1.z += g * q1.x;
                    s2.x += g * q1.y, s2.y += g * q2.x, s2.z += g * q2.y;
                }
            }
            const float r = 1.0f / sg;   // the centre tap has g = 1
            const float boost = a.min_history / fmaxf(m4.w, 1.0f);
            const float3 m1 = make_float3(s1.x * r, s1.y * r, s1.z * r);
            v = make_float3(fmaxf(s2.x * r - m1.x * m1.x, 0.0f) * boost, fmaxf(s2.y * r - m1.y * m1.y, 0.0f) * boost,
                            fmaxf(s2.z * r - m1.z * m1.z, 0.0f) * boost);
        }
    }
    if (!live) return;
    const float3 D = divisor(a, n4, a4);
    a.cout[ip] = make_float4(c4.x / D.x, c4.y / D.y, c4.z / D.z, 0.0f);
    a.vout[ip] = make_float4(v.x / (D.x * D.x), v.y / (D.y * D.y), v.z / (D.z * D.z), 0.0f);
}

// ---- a pass: the lattice tile of lrt_atrous.h (which explains the tile, the branch-free taps and
// the anchor-relative world_pos), as denoise_kernel; where the denoiser stages albedo, the variance.
// The 3x3 variance pre-filter is undilated, off the lattice for s > 1: its nine taps are loaded
// for the centre alone straight from global memory, issued ahead of the staging so that their
// latency passes behind it (rows one apart: a wave's nine loads cover three 1 KiB runs, which its
// neighbours in x and the next pass's phases share in L2).
// The last pass (a.last, a launch argument as denoise_kernel's rgb_only is) multiplies the albedo
// back in from the centre's raw normal and albedo and stores 12 B. As a template parameter it
// made the compiler issue all 150 LDS reads ahead of the first tap (256 VGPRs, one wave per SIMD,
// against 102 and four).
__global__ __launch_bounds__(kTileW* kTileRows) void svgf_pass_kernel(SvgfArgs a) {
    extern __shared__ float2 tile[];
    const int s = a.s, tw = kTileW + 4 * s;
    const int plane = kTileLds * tw;   // float2s per plane
    const int tx = threadIdx.x, ty = threadIdx.y;
    const int x0 = blockIdx.x * kTileW, y0 = tile_y0(s);
    if (y0 >= a.h) return;   // the whole workgroup: the last group's unused phases
    const float kn = a.kn, kx = a.kx;
    const float3 an = tile_anchor(a.pos, a.w, x0, y0, kx);   // uniform over the workgroup
    const int px = x0 + tx, py = y0 + ty * s;
    const bool live = px < a.w && py < a.h;
    const int cpx = min(px, a.w - 1), cpy = min(py, a.h - 1);
    // the centre's 3x3 variance taps first
    float4 pv[9];
    float pb[9];
    const float b3[3] = {0.25f, 0.5f, 0.25f};
#pragma unroll
    for (int j = 0; j < 3; ++j)
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const int gx = cpx + i - 1, gy = cpy + j - 1;
            pb[j * 3 + i] = gx >= 0 && gx < a.w && gy >= 0 && gy < a.h ? b3[i] * b3[j] : 0.0f;
            pv[j * 3 + i] = a.vin[(size_t)min(max(gy, 0), a.h - 1) * a.w + min(max(gx, 0), a.w - 1)];
        }
    // stage, straight-line: all of a thread's loads, then its LDS stores (tile_slot's arithmetic,
    // written out: lrt_atrous.h says why)
    static_assert(tile_covers(LRT_SVGF_MAX_ITER), "two columns per thread cover the tile");
    float4 c[kTileStage], vr[kTileStage], n[kTileStage], x[kTileStage];
    bool ok[kTileStage];
#pragma unroll
    for (int u = 0; u < kTileStage; ++u) {
        const int lr = tile_slot_row(u, ty), cx = min(tile_slot_col(u, tx), tw - 1);
        const int gy = y0 + (lr - 2) * s, gx = x0 - 2 * s + cx;
        ok[u] = gy >= 0 && gy < a.h && gx >= 0 && gx < a.w;
        const size_t ig = (size_t)min(max(gy, 0), a.h - 1) * a.w + min(max(gx, 0), a.w - 1);
        c[u] = a.cin[ig];
        vr[u] = a.vin[ig];
        n[u] = a.nrm[ig];
        x[u] = a.pos[ig];
    }
#pragma unroll
    for (int u = 0; u < kTileStage; ++u) {
        const int lr = tile_slot_row(u, ty), cx = tile_slot_col(u, tx);
        if (cx >= tw) continue;
        const bool on = ok[u] && a.has_n, ox = ok[u] && a.has_x;
        tile_store(tile + lr * tw + cx, plane, ok[u], on, ox, ok[u], c[u], n[u], x[u], vr[u], kn, kx, an, 1.0f);
    }
    float vt = 0.0f, bs = 0.0f;
#pragma unroll
    for (int i = 0; i < 9; ++i) {
        vt += pb[i] * (pv[i].x + pv[i].y + pv[i].z);
        bs += pb[i];
    }
    const float inv_c = 1.44269504f / (a.sc2 * (vt / bs) + 1e-6f);   // the centre is inside: bs >= 1/4
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
    const float2 p3 = ctr[3 * plane], p4 = ctr[4 * plane];
    float sr = 0.0f, sg = 0.0f, sb = 0.0f, sw = 0.0f, vr_ = 0.0f, vg_ = 0.0f, vb_ = 0.0f;
#pragma unroll
    for (int j = 0; j < 5; ++j) {
        const float2* row = tile + (ty + j) * tw + tx;
        float rr = 0.0f, rg = 0.0f, rb = 0.0f, rw = 0.0f, ur = 0.0f, ug = 0.0f, ub = 0.0f;
#pragma unroll
        for (int i = 0; i < 5; ++i) {
            const float2* q = row + i * s;
            const float2 q0 = q[0 * plane], q1 = q[1 * plane], q2 = q[2 * plane];
            const float2 q3 = q[3 * plane], q4 = q[4 * plane], q5 = q[5 * plane];
            const float dx = p0.x - q0.x, dy = p0.y - q0.y, dz = p1.x - q1.x;
            const float e = tile_guide_dist((dx * dx + dy * dy + dz * dz) * inv_c, p1, p2, p3, p4, q1, q2, q3, q4);
            const float wq = hx[i] * __builtin_amdgcn_exp2f(-e);
            const float w2 = wq * wq;
            rr += wq * q0.x;
            rg += wq * q0.y;
            rb += wq * q1.x;
            rw += wq;
            ur += w2 * q4.y;
            ug += w2 * q5.x;
            ub += w2 * q5.y;
        }
        const float h2 = hy[j] * hy[j];
        sr += hy[j] * rr;
        sg += hy[j] * rg;
        sb += hy[j] * rb;
        sw += hy[j] * rw;
        vr_ += h2 * ur;
        vg_ += h2 * ug;
        vb_ += h2 * ub;
    }
    const float r = 1.0f / sw, r2 = r * r;   // the centre tap has E = 0: sw >= 9/64
    const size_t ip = (size_t)py * a.w + px;
    if (a.last) {
        const float3 D = divisor(a, a.nrm[ip], a.alb[ip]);
        float* const oc = reinterpret_cast<float*>(a.cout + ip);
        oc[0] = sr * r * D.x;
        oc[1] = sg * r * D.y;
        oc[2] = sb * r * D.z;
        if (a.vout) {
            float* const ov = reinterpret_cast<float*>(a.vout + ip);
            ov[0] = vr_ * r2 * (D.x * D.x);
            ov[1] = vg_ * r2 * (D.y * D.y);
            ov[2] = vb_ * r2 * (D.z * D.z);
        }
    } else {
        a.cout[ip] = make_float4(sr * r, sg * r, sb * r, 0.0f);
        a.vout[ip] = make_float4(vr_ * r2, vg_ * r2, vb_ * r2, 0.0f);
    }
}

static hipError_t launch_stage0(const SvgfArgs& a, hipStream_t s) {
    const dim3 grid((unsigned)((a.w + k0W - 1) / k0W), (unsigned)((a.h + k0H - 1) / k0H));
    svgf_stage0_kernel<<<grid, k0W * k0H, 0, s>>>(a);
    return hipGetLastError();
}

static hipError_t launch_pass(const SvgfArgs& a, hipStream_t s) {
    svgf_pass_kernel<<<tile_grid(a.w, a.h, a.s), dim3(kTileW, kTileRows), tile_bytes(a.s), s>>>(a);
    return hipGetLastError();
}

static int validate_svgf(const lrt_svgf_desc* d, const float* color, const float* moment2, const lrt_features* g,
                         const float* out, const float* var) {
    if (!d) return fail(LRT_E_INVALID, "desc is NULL");
    if (!color || !moment2 || !out) return fail(LRT_E_INVALID, "color, moment2 or out is NULL");
    if (int rc = validate_frame_size(d->width, d->height)) return rc;
    if (d->iterations < 1 || d->iterations > LRT_SVGF_MAX_ITER)
        return fail(LRT_E_INVALID, "iterations must be in 1..LRT_SVGF_MAX_ITER");
    if (d->flags != 0 || d->reserved != 0) return fail(LRT_E_INVALID, "flags and reserved must be 0");
    if (int rc = validate_min_history(d->min_history)) return rc;
    for (float v : {d->sigma_color, d->sigma_normal, d->sigma_pos, d->albedo_floor})
        if (!std::isfinite(v) || !(v > 0.0f))
            return fail(LRT_E_INVALID, "sigmas and albedo_floor must be finite and > 0");
    // out may be color itself; otherwise no output may overlap an input or the other output
    const size_t bytes = (size_t)d->width * d->height * 4 * sizeof(float);
    const float* const ins[5] = {color, moment2, g ? g->normal : nullptr, g ? g->world_pos : nullptr,
                                 g ? g->albedo : nullptr};
    for (int j = 0; j < 5; ++j) {
        if (ranges_overlap(out, bytes, ins[j], bytes) && !(j == 0 && out == color))
            return fail(LRT_E_INVALID, "aliasing: out overlaps an input (it may only be color itself)");
        if (ranges_overlap(var, bytes, ins[j], bytes))
            return fail(LRT_E_INVALID, "aliasing: variance_out overlaps an input");
    }
    if (ranges_overlap(out, bytes, var, bytes)) return fail(LRT_E_INVALID, "aliasing: out and variance_out overlap");
    return LRT_OK;
}

// The filter on stream s (device pointers, validated): stage 0 writes (c_0, var_0) into stream
// s's scratch, the passes ping-pong between two such pairs and the last one writes the outputs.
// Nothing reads color after stage 0, so out == color needs no copy.
static int svgf_device(const lrt_svgf_desc* d, const float* color, const float* moment2, const lrt_features* g,
                       float* out, float* var, hipStream_t s) {
    const size_t npix = (size_t)d->width * d->height;
    const int K = d->iterations;
    const int ntmp = K == 1 ? 2 : 4;
    void* p = nullptr;
    if (int rc = scratch_or_fail(s, ntmp * npix * sizeof(float4), "svgf scratch", &p)) return rc;
    float4* const base = static_cast<float4*>(p);
    float4* const tc[2] = {base, ntmp == 4 ? base + 2 * npix : nullptr};
    float4* const tv[2] = {base + npix, ntmp == 4 ? base + 3 * npix : nullptr};
    SvgfArgs a;
    memset(&a, 0, sizeof(a));
    a.cin = quads(color);
    a.vin = quads(moment2);
    a.cout = tc[0];
    a.vout = tv[0];
    a.nrm = g && g->normal ? quads(g->normal) : nullptr;
    a.pos = g && g->world_pos ? quads(g->world_pos) : nullptr;
    a.alb = g && g->albedo ? quads(g->albedo) : nullptr;
    a.has_n = a.nrm != nullptr;
    a.has_x = a.pos != nullptr;
    a.has_a = a.alb != nullptr;
    // an absent guide reads the colour instead (a valid address); its has_ flag drops what was read
    if (!a.nrm) a.nrm = a.cin;
    if (!a.pos) a.pos = a.cin;
    if (!a.alb) a.alb = a.cin;
    a.w = d->width;
    a.h = d->height;
    a.s = 1;
    a.sc2 = d->sigma_color * d->sigma_color;
    const float rl2e = sqrtf(1.44269504f);
    a.kn = rl2e / d->sigma_normal;
    a.kx = rl2e / d->sigma_pos;
    a.floor_a = d->albedo_floor;
    a.min_history = (float)d->min_history;
    LRT_HIP(launch_stage0(a, s));
    for (int k = 0; k < K; ++k) {
        const bool last = k == K - 1;
        a.cin = tc[k & 1];
        a.vin = tv[k & 1];
        a.cout = last ? quads(out) : tc[(k + 1) & 1];
        a.vout = last ? quads(var) : tv[(k + 1) & 1];
        if (!a.has_n) a.nrm = a.cin;
        if (!a.has_x) a.pos = a.cin;
        if (!a.has_a) a.alb = a.cin;
        a.s = 1 << k;
        a.last = last;
        LRT_HIP(launch_pass(a, s));
    }
    LRT_HIP(stream_scratch_used(s));
    return LRT_OK;
}

}  // namespace lrt

using namespace lrt;

extern "C" {

int lrt_svgf_default(int width, int height, lrt_svgf_desc* out) {
    if (int rc = frame_default_begin(out, sizeof(*out), width, height)) return rc;
    out->width = width;
    out->height = height;
    out->iterations = LRT_SVGF_MAX_ITER;
    out->min_history = 4;
    out->sigma_color = 4.0f;
    out->sigma_normal = 0.3f;
    out->sigma_pos = 0.5f;
    out->albedo_floor = 0.01f;
    return LRT_OK;
}

int lrt_svgf_filter_device(const lrt_svgf_desc* desc, const float* d_color, const float* d_moment2,
                           const lrt_features* d_guides, float* d_out, float* d_variance_out, void* stream) {
    RoctxRange rr_("lrt_svgf_filter_device");
    if (int rc = validate_svgf(desc, d_color, d_moment2, d_guides, d_out, d_variance_out)) return rc;
    std::lock_guard<std::mutex> lk(g_mu);
    if (int rc = require_initialized()) return rc;
    DeviceScope ds_(0);   // context 0's device (device 0 of lrt_initialize_devices)
    return svgf_device(desc, d_color, d_moment2, d_guides, d_out, d_variance_out, (hipStream_t)stream);
}

int lrt_svgf_filter_host(const lrt_svgf_desc* desc, const float* color, const float* moment2,
                         const lrt_features* guides, float* out, float* variance_out) {
    RoctxRange rr_("lrt_svgf_filter_host");
    if (int rc = validate_svgf(desc, color, moment2, guides, out, variance_out)) return rc;
    std::lock_guard<std::mutex> lk(g_mu);
    if (int rc = require_initialized()) return rc;
    DeviceScope ds_(0);
    const size_t quad = (size_t)desc->width * desc->height * 4 * sizeof(float);
    hipStream_t s = ctx().stream;
    // Every buffer that is given goes through a device mirror of its own. The two outputs are copied
    // in first (their alphas stay); in place, out's mirror is color's.
    const bool in_place = out == color;
    HostMirrors m;
    const int color_ = m.add(color, in_place ? out : nullptr, quad), moment_ = m.in(moment2, quad);
    const int normal_ = m.in(guides ? guides->normal : nullptr, quad);
    const int pos_ = m.in(guides ? guides->world_pos : nullptr, quad);
    const int albedo_ = m.in(guides ? guides->albedo : nullptr, quad);
    const int out_ = in_place ? color_ : m.inout(out, quad), var_ = m.inout(variance_out, quad);
    if (int rc = m.alloc("hipMalloc(svgf staging)")) return rc;
    if (int rc = m.upload(s)) return rc;
    auto f = [&m](int i) { return m.dev<float>(i); };
    lrt_features dg;
    memset(&dg, 0, sizeof(dg));
    dg.normal = f(normal_);
    dg.world_pos = f(pos_);
    dg.albedo = f(albedo_);
    if (int rc = svgf_device(desc, f(color_), f(moment_), &dg, f(out_), f(var_), s)) return rc;
    return m.download(s);
}

}  // extern "C"
