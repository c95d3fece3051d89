// Auto-exposure metering and tone mapping (lrt_tonemap_*, include/lrt.h): three launches (behind
// a 1 KiB fill that zeroes the histogram) whose boundaries do the ordering. The meter kernel
// counts the frame's luminances into a 256-bin log2 histogram (integer counts only:
// deterministic), the exposure kernel (one workgroup) turns the histogram into the new exposure
// state, the map kernel reads the exposure from that state in device memory, applies the tone
// curve and quantises as present_kernel does. Not bit-pinned but for that quantiser
// (lrt_srgb.h): contraction is allowed inside the curve alone.
#include "lrt_internal.h"
#include "lrt_srgb.h"

#include <cfloat>

namespace lrt {

constexpr int kBins = LRT_TONEMAP_BINS, kWords = LRT_TONEMAP_HIST_WORDS;
constexpr int kUnder = kBins, kOver = kBins + 1;
constexpr int kMeterBlock = 256, kMeterWaves = kMeterBlock / 64;
constexpr int kMeterUnroll = 4;                          // float4 loads in flight per thread
constexpr int kMeterChunk = kMeterBlock * kMeterUnroll;  // pixels per workgroup step
static_assert(kBins == 256 && kWords == kBins + 2, "one exposure thread per bin");

// The bin of a luminance, from its bits: positive floats order as their bits do, so one unsigned
// range check takes [2^-16, 2^16) (bits 0x37800000 .. 0x477fffff, eight values of bits >> 20 per
// octave), a second takes [2^16, +Inf]; what is left (zero, negatives: the sign bit; NaNs: above
// +Inf's bits; below 2^-16) is `under`.
LRT_DEV int luminance_bin(const float4 c) {
    const float y = 0.2126f * c.x + 0.7152f * c.y + 0.0722f * c.z;
    const uint32_t b = __builtin_bit_cast(uint32_t, y);
    if (b - 0x37800000u < 0x10000000u) return (int)(b >> 20) - 888;
    return b - 0x47800000u <= 0x7f800000u - 0x47800000u ? kOver : kUnder;
}

// One count per live lane into this wave's LDS histogram. Rendered frames put most of a wave into
// one or two bins (the sky, a large diffuse sphere) and same-address LDS adds serialise, so up to
// kPeel times the wave takes the bin of its first remaining lane, counts the lanes that share it
// (one ballot) and adds that count from one lane; whoever is left adds 1. (Against a plain
// atomicAdd per lane: DESIGN 7.4.)
constexpr int kPeel = 2;
__device__ __forceinline__ void count(uint32_t* hw, const int bin, bool live) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int r = 0; r < kPeel; ++r) {
        const unsigned long long todo = __ballot(live);
        if (!todo) return;   // uniform
        const int first = __ffsll((long long)todo) - 1;
        const int lead = __builtin_amdgcn_readlane(bin, first);
        const bool same = live && bin == lead;
        const unsigned long long mask = __ballot(same);
        if (lane == first) atomicAdd(hw + lead, (uint32_t)__popcll(mask));
        live = live && !same;
    }
    if (live) atomicAdd(hw + bin, 1u);
}

// ---- kernel 1. gridDim.x workgroups stride over chunks of kMeterChunk whole pixels; a thread has
// kMeterUnroll float4 loads in flight. Counts go to per-wave LDS histograms, summed over the
// waves and flushed once per workgroup: integer atomics (any order gives the same sums) of the
// non-zero counts into the zeroed histogram. (Against per-workgroup slabs summed by kernel 2:
// DESIGN 7.4.)
__global__ __launch_bounds__(kMeterBlock) void meter_kernel(const float4* __restrict__ color, const int npix,
                                                            uint32_t* __restrict__ dst) {
    __shared__ uint32_t hist[kMeterWaves][kWords];
    const int t = threadIdx.x;
    for (int i = t; i < kMeterWaves * kWords; i += kMeterBlock) (&hist[0][0])[i] = 0u;
    __syncthreads();
    uint32_t* const hw = hist[t >> 6];
    const int nchunks = (npix + kMeterChunk - 1) / kMeterChunk;
    for (int ch = blockIdx.x; ch < nchunks; ch += gridDim.x) {
        const int i0 = ch * kMeterChunk + t;   // < npix + kMeterChunk <= INT_MAX / 4 + 1024
        float4 c[kMeterUnroll];
#pragma unroll
        for (int u = 0; u < kMeterUnroll; ++u) c[u] = color[min(i0 + u * kMeterBlock, npix - 1)];
#pragma unroll
        for (int u = 0; u < kMeterUnroll; ++u) count(hw, luminance_bin(c[u]), i0 + u * kMeterBlock < npix);
    }
    __syncthreads();
    for (int b = t; b < kWords; b += kMeterBlock) {
        uint32_t n = 0;
#pragma unroll
        for (int w = 0; w < kMeterWaves; ++w) n += hist[w][b];
        if (n) atomicAdd(dst + b, n);
    }
}

struct ExposureArgs {
    const uint32_t* hist;    // the kWords counts
    lrt_exposure_state* state;
    double npix;
    double log2_key;
    float p_low, p_high, ev_bias, ev_min, ev_max, adapt;
};

// log2(1 + (k + 0.5) / 8), k = 0 .. 7: the middle of an eighth of an octave
__device__ const double kSubBin[8] = {0.0874628412503394, 0.2479275134435855, 0.3923174227787603, 0.5235619560570128,
                                      0.6438561897747247, 0.7548875021634686, 0.8579809951275721, 0.9541963103868752};

// ---- kernel 2: one workgroup, thread b owns bin b. An LDS prefix sum of the counts,
// the window's share m_b of the bin, then sum m_b l_b and sum m_b by a tree whose order is fixed,
// in f64 (the counts are exact there), and the state update by thread 0.
__global__ __launch_bounds__(kBins) void exposure_kernel(const ExposureArgs a) {
    __shared__ uint32_t scan[kBins];
    __shared__ double s1[kBins], s0[kBins];
    const int b = threadIdx.x;
    const uint32_t h = a.hist[b];
    scan[b] = h;
    __syncthreads();
    for (int off = 1; off < kBins; off <<= 1) {   // inclusive (Hillis-Steele)
        const uint32_t v = b >= off ? scan[b - off] : 0u;
        __syncthreads();
        scan[b] += v;
        __syncthreads();
    }
    const double N = (double)scan[kBins - 1];
    const double cb = (double)(scan[b] - h), ce = (double)scan[b];
    const double lo = (double)a.p_low * N, hi = (double)a.p_high * N;
    const double m = fmax(0.0, fmin(ce, hi) - fmax(cb, lo));
    const double l = (double)((b >> 3) - 16) + kSubBin[b & 7];
    s1[b] = m * l;
    s0[b] = m;
    __syncthreads();
    for (int off = kBins / 2; off > 0; off >>= 1) {
        if (b < off) {
            s1[b] += s1[b + off];
            s0[b] += s0[b + off];
        }
        __syncthreads();
    }
    if (b != 0) return;
    const lrt_exposure_state prev = *a.state;
    const bool has = prev.frames >= 1.0f;
    lrt_exposure_state next;
    if (N > 0.0) {
        const double mean = s1[0] / s0[0];   // s0 = (p_high - p_low) N > 0
        const double target = fmin(fmax(a.log2_key - mean + (double)a.ev_bias, (double)a.ev_min), (double)a.ev_max);
        const double p = (double)prev.log2_exposure;
        next.log2_exposure = (float)(has ? p + (double)a.adapt * (target - p) : target);
        next.log2_luminance = (float)mean;
        next.counted = (float)(N / a.npix);
    } else {
        next.log2_exposure = has ? prev.log2_exposure : fminf(fmaxf(a.ev_bias, a.ev_min), a.ev_max);
        next.log2_luminance = prev.log2_luminance;
        next.counted = 0.0f;
    }
    next.frames = prev.frames + 1.0f;
    *a.state = next;
}

struct MapArgs {
    const float4* color;
    float4* out;                       // or null; may be color
    uint32_t* bgra;                    // or null
    const lrt_exposure_state* state;   // auto_exposure: the state kernel 2 wrote; else null
    float ev;                          // ... else the log2 exposure
    float white2;                      // white^2, within [FLT_MIN, FLT_MAX]
    int op, npix;
};

// The curve of one channel: the one function both outputs take t from.
__device__ __forceinline__ float tone(const float x, const float e, const int op, const float white2) {
#pragma clang fp contract(fast)
    float c = x * e;
    c = c > 0.0f ? fminf(c, LRT_TM_MAX) : 0.0f;   // a NaN fails the compare
    if (op == LRT_TM_LINEAR) return c;
    if (op == LRT_TM_REINHARD) return c * (1.0f + c / white2) / (1.0f + c);
    const float t = c * (2.51f * c + 0.03f) / (c * (2.43f * c + 0.59f) + 0.14f);
    return fminf(fmaxf(t, 0.0f), 1.0f);
}

// ---- kernel 3: a pixel per thread, one 16 B load, up to one 12 B store (out's alpha stays) and
// one 4 B store. The exposure is a uniform load from the state.
__global__ __launch_bounds__(256) void map_kernel(const MapArgs a) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.npix) return;
    const float e = exp2f(a.state ? a.state->log2_exposure : a.ev);
    const float4 c = a.color[i];
    const float r = tone(c.x, e, a.op, a.white2), g = tone(c.y, e, a.op, a.white2), b = tone(c.z, e, a.op, a.white2);
    if (a.out) {
        float* const o = reinterpret_cast<float*>(a.out + i);
        o[0] = r;
        o[1] = g;
        o[2] = b;
    }
    if (a.bgra) a.bgra[i] = pack_bgra8(r, g, b);
}

static int validate_tonemap(const lrt_tonemap_desc* d, const float* color, const lrt_exposure_state* state,
                            const uint32_t* hist, const float* out, const uint32_t* bgra) {
    if (!d) return fail(LRT_E_INVALID, "desc is NULL");
    if (!color) return fail(LRT_E_INVALID, "color is NULL");
    if (int rc = validate_frame_size(d->width, d->height)) return rc;
    if (d->op != LRT_TM_LINEAR && d->op != LRT_TM_REINHARD && d->op != LRT_TM_ACES)
        return fail(LRT_E_INVALID, "op must be one of LRT_TM_*");
    if (d->auto_exposure != 0 && d->auto_exposure != 1) return fail(LRT_E_INVALID, "auto_exposure must be 0 or 1");
    if (d->flags != 0 || d->reserved != 0) return fail(LRT_E_INVALID, "flags and reserved must be 0");
    for (float v : {d->key, d->p_low, d->p_high, d->ev_bias, d->ev_min, d->ev_max, d->adapt, d->white})
        if (!std::isfinite(v)) return fail(LRT_E_INVALID, "every parameter must be finite");
    if (!(d->key > 0.0f) || !(d->white > 0.0f)) return fail(LRT_E_INVALID, "key and white must be > 0");
    if (!(d->p_low >= 0.0f && d->p_low < d->p_high && d->p_high <= 1.0f))
        return fail(LRT_E_INVALID, "the window must satisfy 0 <= p_low < p_high <= 1");
    if (!(d->ev_min <= d->ev_max)) return fail(LRT_E_INVALID, "ev_min must be <= ev_max");
    if (!(d->adapt > 0.0f && d->adapt <= 1.0f)) return fail(LRT_E_INVALID, "adapt must be in (0, 1]");
    if (d->auto_exposure && !state) return fail(LRT_E_INVALID, "auto_exposure needs the exposure state");
    if (!d->auto_exposure && !out && !bgra) return fail(LRT_E_INVALID, "nothing to do: no output and no metering");
    // bgra, histogram and state may overlap nothing; out may be color itself and otherwise not overlap it
    const size_t npix = (size_t)d->width * d->height;
    const size_t nc = npix * 16, nb = npix * 4, nh = kWords * sizeof(uint32_t), ns = sizeof(lrt_exposure_state);
    if (ranges_overlap(bgra, nb, color, nc) || ranges_overlap(bgra, nb, out, nc) ||
        ranges_overlap(bgra, nb, hist, nh) || ranges_overlap(bgra, nb, state, ns))
        return fail(LRT_E_INVALID, "aliasing: bgra overlaps another buffer");
    if (ranges_overlap(hist, nh, color, nc) || ranges_overlap(hist, nh, out, nc) || ranges_overlap(hist, nh, state, ns))
        return fail(LRT_E_INVALID, "aliasing: histogram overlaps another buffer");
    if (ranges_overlap(state, ns, color, nc) || ranges_overlap(state, ns, out, nc))
        return fail(LRT_E_INVALID, "aliasing: state overlaps another buffer");
    if (ranges_overlap(out, nc, color, nc) && out != color)
        return fail(LRT_E_INVALID, "aliasing: out overlaps color (it may only be color itself)");
    return LRT_OK;
}

// The call on stream s (device pointers, validated).
static int tonemap_device(const lrt_tonemap_desc* d, const float* color, lrt_exposure_state* state, uint32_t* hist,
                          float* out, uint32_t* bgra, hipStream_t s) {
    const int npix = d->width * d->height;
    if (d->auto_exposure) {
        // a bounded grid: one workgroup per CU, fewer on a small frame (two per CU were slower)
        const int groups = std::max(1, std::min((npix + kMeterChunk - 1) / kMeterChunk, ctx().num_cus));
        uint32_t* total = hist;
        if (!total) {
            void* p = nullptr;
            if (int rc = scratch_or_fail(s, kWords * sizeof(uint32_t), "tonemap scratch", &p)) return rc;
            total = static_cast<uint32_t*>(p);
        }
        LRT_HIP(hipMemsetAsync(total, 0, kWords * sizeof(uint32_t), s));
        meter_kernel<<<groups, kMeterBlock, 0, s>>>(quads(color), npix, total);
        LRT_HIP(hipGetLastError());
        ExposureArgs x;
        memset(&x, 0, sizeof(x));
        x.hist = total;
        x.state = state;
        x.npix = (double)npix;
        x.log2_key = log2((double)d->key);
        x.p_low = d->p_low;
        x.p_high = d->p_high;
        x.ev_bias = d->ev_bias;
        x.ev_min = d->ev_min;
        x.ev_max = d->ev_max;
        x.adapt = d->adapt;
        exposure_kernel<<<1, kBins, 0, s>>>(x);
        LRT_HIP(hipGetLastError());
        if (!hist) LRT_HIP(stream_scratch_used(s));
    }
    if (out || bgra) {
        MapArgs m;
        memset(&m, 0, sizeof(m));
        m.color = quads(color);
        m.out = quads(out);
        m.bgra = bgra;
        m.state = d->auto_exposure ? state : nullptr;
        m.ev = d->ev_bias;
        m.white2 = std::min(std::max(d->white * d->white, FLT_MIN), FLT_MAX);
        m.op = d->op;
        m.npix = npix;
        map_kernel<<<(npix + 255) / 256, 256, 0, s>>>(m);
        LRT_HIP(hipGetLastError());
    }
    return LRT_OK;
}

}  // namespace lrt

using namespace lrt;

extern "C" {

int lrt_tonemap_default(int width, int height, lrt_tonemap_desc* out) {
    if (int rc = frame_default_begin(out, sizeof(*out), width, height)) return rc;
    out->width = width;
    out->height = height;
    out->op = LRT_TM_ACES;
    out->auto_exposure = 1;
    out->key = 0.18f;
    out->p_low = 0.1f;
    out->p_high = 0.9f;
    out->ev_bias = 0.0f;
    out->ev_min = -8.0f;
    out->ev_max = 8.0f;
    out->adapt = 1.0f;
    out->white = 4.0f;
    return LRT_OK;
}

int lrt_tonemap_device(const lrt_tonemap_desc* desc, const float* d_color, lrt_exposure_state* d_state,
                       uint32_t* d_histogram, float* d_out, uint32_t* d_bgra, void* stream) {
    RoctxRange rr_("lrt_tonemap_device");
    if (int rc = validate_tonemap(desc, d_color, d_state, d_histogram, d_out, d_bgra)) return rc;
    std::lock_guard<std::mutex> lk(g_mu);
    if (int rc = require_initialized()) return rc;
    DeviceScope ds_(0);   // context 0's device (device 0 of lrt_initialize_devices)
    return tonemap_device(desc, d_color, d_state, d_histogram, d_out, d_bgra, (hipStream_t)stream);
}

int lrt_tonemap_host(const lrt_tonemap_desc* desc, const float* color, lrt_exposure_state* state,
                     uint32_t* histogram, float* out, uint32_t* bgra) {
    RoctxRange rr_("lrt_tonemap_host");
    if (int rc = validate_tonemap(desc, color, state, histogram, out, bgra)) return rc;
    std::lock_guard<std::mutex> lk(g_mu);
    if (int rc = require_initialized()) return rc;
    DeviceScope ds_(0);
    const size_t npix = (size_t)desc->width * desc->height;
    const bool meter = desc->auto_exposure != 0, in_place = out == color;
    hipStream_t s = ctx().stream;
    // Device mirrors: color, out (copied in first: its alpha stays; in place it is color's mirror),
    // bgra, and the histogram and the state, which are mirrored only when the call meters.
    HostMirrors m;
    const int color_ = m.add(color, in_place ? out : nullptr, npix * 16);
    const int out_ = in_place ? color_ : m.inout(out, npix * 16), bgra_ = m.out(bgra, npix * 4);
    const int hist_ = m.out(meter ? histogram : nullptr, kWords * sizeof(uint32_t));
    const int state_ = m.inout(meter ? state : nullptr, sizeof(lrt_exposure_state));
    if (int rc = m.alloc("hipMalloc(tonemap staging)")) return rc;
    if (int rc = m.upload(s)) return rc;
    if (int rc = tonemap_device(desc, m.dev<float>(color_), m.dev<lrt_exposure_state>(state_), m.dev<uint32_t>(hist_),
                                m.dev<float>(out_), m.dev<uint32_t>(bgra_), s))
        return rc;
    return m.download(s);
}

}  // extern "C"
