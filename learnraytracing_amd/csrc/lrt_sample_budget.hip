// The per-pixel sample budget (lrt_sample_budget_*, include/lrt.h): a noise plane in, an integer
// sample count per pixel out, under a total budget. One weight kernel (the f32 part: q_p, and the
// first pass's sums), then one apply kernel per pass; a pass reads E, Q and m from device memory and
// accumulates the next pass's sums while it writes the counts, so the passes need no host round
// trip. The sums are integer atomics, a block's partial sums reduced first: exact in any order.
// No contraction, like the render units: the counts are pinned to tests/sample_budget_ref.py.
#include "lrt_internal.h"

namespace lrt {

constexpr int kSbBlock = 1024, kSbWaves = kSbBlock / 64;
constexpr int kSbMaxPasses = 4;
// One pass's sums, two words: sum count (bits 0-31: it never exceeds the budget, below 2^31) with
// m = |U| above it (bits 32-63), and Q (over U). Set j holds what pass j + 1 reads; set `passes` ends
// up with the final sum count. Same-address atomics serialise (~12 ns each), so a call keeps them
// few: one block of 1024 threads per CU at most, two atomics per block.
constexpr int kSbSet = 2;

struct BudgetArgs {
    const float4* var;
    const float4* color;   // or null
    uint32_t* q;           // npix weights (scratch)
    int32_t* counts;
    unsigned long long* sums;   // (kSbMaxPasses + 1) sets, zeroed before the weight kernel
    int npix;
    int std_in;            // LRT_SB_STD
    int min_count, max_count;
    long long budget;
    float luma_floor, weight_max;
};

// A block's partial sums into set `dst`: one 64-bit atomic per word and block.
__device__ __forceinline__ void block_sums(unsigned long long* dst, unsigned long long s, unsigned long long q,
                                           unsigned long long m) {
    __shared__ unsigned long long part[2][kSbWaves];
    s = wave_sum(s + (m << 32));
    q = wave_sum(q);
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        part[0][wave] = s;
        part[1][wave] = q;
    }
    __syncthreads();
    if (threadIdx.x < 2) {
        unsigned long long t = 0;
        for (int w = 0; w < kSbWaves; ++w) t += part[threadIdx.x][w];
        if (t) atomicAdd(dst + threadIdx.x, t);
    }
}

__device__ __forceinline__ float luma(const float4 c) { return (0.2126f * c.x + 0.7152f * c.y) + 0.0722f * c.z; }

// Steps 1 and 2: q_p, count_p = min_count, and set 0.
__global__ __launch_bounds__(kSbBlock) void budget_weight_kernel(const BudgetArgs a) {
    unsigned long long s = 0, qs = 0, m = 0;
    const int stride = gridDim.x * kSbBlock;   // npix + stride <= INT_MAX / 4 + 2^22
    for (int i = blockIdx.x * kSbBlock + threadIdx.x; i < a.npix; i += stride) {
        float4 v = a.var[i];
        if (a.std_in) {
            v.x = v.x * v.x;
            v.y = v.y * v.y;
            v.z = v.z * v.z;
        }
        float w = __builtin_sqrtf(luma(v));
        if (a.color) w = w / (fmaxf(luma(a.color[i]), 0.0f) + a.luma_floor);
        uint32_t q = 0;
        if (w > 0.0f && w < __builtin_inff()) q = (uint32_t)(fminf(w, a.weight_max) * 65536.0f);
        a.q[i] = q;
        a.counts[i] = a.min_count;
        s += (unsigned long long)a.min_count;
        if (a.min_count < a.max_count) {
            qs += q;
            m += 1;
        }
    }
    block_sums(a.sums, s, qs, m);
}

// Pass j + 1 (set j in, set j + 1 out).
__global__ __launch_bounds__(kSbBlock) void budget_apply_kernel(const BudgetArgs a, const int j) {
    const unsigned long long* in = a.sums + kSbSet * j;
    const long long E = a.budget - (long long)(in[0] & 0xffffffffull);
    const unsigned long long Q = in[1], M = in[0] >> 32;
    const bool act = E > 0 && M > 0;
    const unsigned long long even = act && Q == 0 ? (unsigned long long)E / M : 0ull;
    unsigned long long s = 0, qs = 0, m = 0;
    const int stride = gridDim.x * kSbBlock;
    for (int i = blockIdx.x * kSbBlock + threadIdx.x; i < a.npix; i += stride) {
        int c = a.counts[i];
        const uint32_t q = a.q[i];
        if (act && c < a.max_count) {
            const unsigned long long add = Q == 0 ? even : (unsigned long long)E * q / Q;
            const unsigned long long n = (unsigned long long)c + add;
            c = n < (unsigned long long)a.max_count ? (int)n : a.max_count;
            a.counts[i] = c;
        }
        s += (unsigned long long)c;
        if (c < a.max_count) {
            qs += q;
            m += 1;
        }
    }
    block_sums(a.sums + kSbSet * (j + 1), s, qs, m);
}

__global__ void budget_info_kernel(const unsigned long long* sums, int passes, unsigned long long* info) {
    info[0] = sums[kSbSet * passes] & 0xffffffffull;
    info[1] = sums[1];
}

static int validate_budget(const lrt_sample_budget_desc* d, const float* variance, const float* color,
                           const int32_t* counts, const unsigned long long* info) {
    if (!d) return fail(LRT_E_INVALID, "desc is NULL");
    if (!variance) return fail(LRT_E_INVALID, "variance is NULL");
    if (!counts) return fail(LRT_E_INVALID, "counts is NULL");
    if (int rc = validate_frame_size(d->width, d->height)) return rc;
    if ((d->flags & ~LRT_SB_STD) != 0 || d->reserved != 0 || d->reserved2 != 0)
        return fail(LRT_E_INVALID, "unknown flag, or a reserved word != 0");
    if (d->min_count < 0 || d->min_count > d->max_count || d->max_count > LRT_COUNT_MAX)
        return fail(LRT_E_INVALID, "counts must satisfy 0 <= min_count <= max_count <= LRT_COUNT_MAX");
    if (d->passes < 1 || d->passes > kSbMaxPasses) return fail(LRT_E_INVALID, "passes must be 1..4");
    const long long npix = (long long)d->width * d->height;
    if (d->budget < (long long)d->min_count * npix || d->budget > 0x7fffffffLL)
        return fail(LRT_E_INVALID, "budget must be in min_count * width * height .. 2^31 - 1");
    if (!std::isfinite(d->luma_floor) || !(d->luma_floor > 0.0f))
        return fail(LRT_E_INVALID, "luma_floor must be finite and > 0");
    if (!std::isfinite(d->weight_max) || !(d->weight_max > 0.0f) || d->weight_max > 16384.0f)
        return fail(LRT_E_INVALID, "weight_max must be finite, > 0 and <= 16384");
    const size_t px = (size_t)npix;
    const Span outs[2] = {{counts, 4 * px}, {info, 16}}, ins[2] = {{variance, 16 * px}, {color, 16 * px}};
    if (const int k = spans_alias(outs, 2, ins, 2))
        return fail(LRT_E_INVALID, k == 1 ? "aliasing: counts or info overlaps an input"
                                          : "aliasing: counts and info overlap");
    return LRT_OK;
}

// The call on stream s (device pointers, validated; context 0 is current).
static int budget_device(const lrt_sample_budget_desc* d, const float* variance, const float* color, int32_t* counts,
                         unsigned long long* info, hipStream_t s) {
    const int npix = d->width * d->height;
    const size_t sums_bytes = sizeof(unsigned long long) * kSbSet * (kSbMaxPasses + 1);
    void* p = nullptr;
    if (int rc = scratch_or_fail(s, sums_bytes + sizeof(uint32_t) * (size_t)npix, "sample budget scratch", &p)) return rc;
    BudgetArgs a;
    memset(&a, 0, sizeof(a));
    a.var = quads(variance);
    a.color = quads(color);
    a.sums = static_cast<unsigned long long*>(p);
    a.q = reinterpret_cast<uint32_t*>(static_cast<char*>(p) + sums_bytes);
    a.counts = counts;
    a.npix = npix;
    a.std_in = (d->flags & LRT_SB_STD) ? 1 : 0;
    a.min_count = d->min_count;
    a.max_count = d->max_count;
    a.budget = d->budget;
    a.luma_floor = d->luma_floor;
    a.weight_max = d->weight_max;
    // a bounded grid: one block per CU at most, striding over the frame
    const int groups = std::max(1, std::min((npix + kSbBlock - 1) / kSbBlock, ctx().num_cus));
    LRT_HIP(hipMemsetAsync(a.sums, 0, sums_bytes, s));
    budget_weight_kernel<<<groups, kSbBlock, 0, s>>>(a);
    LRT_HIP(hipGetLastError());
    for (int j = 0; j < d->passes; ++j) {
        budget_apply_kernel<<<groups, kSbBlock, 0, s>>>(a, j);
        LRT_HIP(hipGetLastError());
    }
    if (info) {
        budget_info_kernel<<<1, 1, 0, s>>>(a.sums, d->passes, info);
        LRT_HIP(hipGetLastError());
    }
    LRT_HIP(stream_scratch_used(s));
    return LRT_OK;
}

}  // namespace lrt

using namespace lrt;

extern "C" {

int lrt_sample_budget_default(int width, int height, int min_count, int max_count, long long budget,
                              lrt_sample_budget_desc* out) {
    if (int rc = frame_default_begin(out, sizeof(*out), width, height)) return rc;
    out->width = width;
    out->height = height;
    out->min_count = min_count;
    out->max_count = max_count;
    out->passes = 2;
    out->budget = budget;
    out->luma_floor = 0.01f;
    out->weight_max = 256.0f;
    return LRT_OK;
}

int lrt_sample_budget_device(const lrt_sample_budget_desc* desc, const float* d_variance, const float* d_color,
                             int32_t* d_counts, unsigned long long* d_info, void* stream) {
    RoctxRange rr_("lrt_sample_budget_device");
    if (int rc = validate_budget(desc, d_variance, d_color, d_counts, d_info)) return rc;
    std::lock_guard<std::mutex> lk(g_mu);
    if (int rc = require_initialized()) return rc;
    DeviceScope ds_(0);   // context 0's device (device 0 of lrt_initialize_devices)
    return budget_device(desc, d_variance, d_color, d_counts, d_info, (hipStream_t)stream);
}

int lrt_sample_budget_host(const lrt_sample_budget_desc* desc, const float* variance, const float* color,
                           int32_t* counts, unsigned long long* info) {
    RoctxRange rr_("lrt_sample_budget_host");
    if (int rc = validate_budget(desc, variance, color, counts, info)) return rc;
    std::lock_guard<std::mutex> lk(g_mu);
    if (int rc = require_initialized()) return rc;
    DeviceScope ds_(0);
    hipStream_t s = ctx().stream;
    const size_t npix = (size_t)desc->width * desc->height;
    HostMirrors m;
    const int var_ = m.in(variance, npix * 16), color_ = m.in(color, npix * 16);
    const int counts_ = m.out(counts, npix * 4), info_ = m.out(info, 16);
    if (int rc = m.alloc("hipMalloc(sample budget staging)")) return rc;
    if (int rc = m.upload(s)) return rc;
    if (int rc = budget_device(desc, m.dev<float>(var_), m.dev<float>(color_), m.dev<int32_t>(counts_),
                               m.dev<unsigned long long>(info_), s))
        return rc;
    return m.download(s);
}

}  // extern "C"
