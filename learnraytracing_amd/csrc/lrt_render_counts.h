// The sample-list trace kernel of lrt_render_counts_* (counts_trace_kernel) and its launch;
// instantiated per depth class by lrt_render_counts_d8.hip and lrt_render_counts_d64.hip. The scan
// before it, the merge behind it and the entry points are lrt_render_counts.hip's.
//
// The call's samples are one compacted list: pixel p (local row-major) owns the slots
// o_p .. o_p + c_p - 1 of the exclusive scan of the clamped counts. Lane s of the list reads its
// pixel from the per-sample index the scan stage wrote, builds the ray as trace_kernel does
// (PixelSeed, the two rng_offset draws, GetRay), traces it and stores the colour in slot s;
// merge_counts_kernel then lerps a pixel's slots in frame order, as merge_samples_kernel does for
// v0's sample mode. 64 consecutive samples are neighbouring pixels of a row, so first rays stay
// coherent and every lane has work whatever the count map looks like. The number of samples is
// device data: persistent single-wave blocks take 64-sample chunks from kV0Queues counters, as
// trace_kernel takes its tiles (one counter serialises at ~12 ns per fetch: 57,600 chunks of a
// 1280x720 frame at 4 spp were 0.69 ms of a 0.79 ms launch), until the list ends. The LDS layout,
// the scene staging, the tables, the overflow stack and the launch bounds are trace_kernel's (lrt_v0.h).
#pragma once
#include "lrt_internal.h"

namespace lrt {

// What the stages of one call share, all in the stream's scratch but counts.
struct CountsArgs {
    const int32_t* counts;        // the caller's plane
    const int* offs;              // npix + 1 exclusive offsets, saturated at kCountsSat
    const int* pix;               // nslots: the pixel of each sample of the list
    unsigned long long* head;     // [0] the scan's total (unsaturated), [1] the merge's info word (traced in
                                  // bits 0-31, skipped above), [kCtrStride * (1 + q)] chunk queue q's counter
    float4* slots;                // nslots: one colour per sample
    long long nslots;             // min(capacity, pixels * frames)
    int npix;
    long long capacity;
};
// Offsets above the largest capacity (2^27) are stored as this: a pixel there is never rendered.
constexpr int kCountsSat = 1 << 28;
constexpr long long kCountsCapacityMax = 1ll << 27;
constexpr size_t kCountsHeadBytes = sizeof(unsigned long long) * kCtrStride * (1 + kV0Queues);

__device__ __forceinline__ int clamped_count(const int32_t c, const int frames) { return min(max(c, 0), frames); }

template <int MAXD, bool kLds, int kAcc, int kNS = 0>
__global__ __launch_bounds__(kBlock, kWavesPerEU) void counts_trace_kernel(const KernelArgs a, const CountsArgs ca) {
    static_assert(kBlock == 64, "a block is one wave: a chunk is 64 samples");
    static_assert(kNS == 0 || (kLds && !kAcc), "a fixed sphere count is for the LDS linear scan");
    // LDS: [recursion stack kTraceLdsLevels x kBlock][powf tables][renormalize table][spheres][materials][lights]
    extern __shared__ float4 smem[];
    const int tid = threadIdx.x;
    double* s_pow = reinterpret_cast<double*>(smem + kTraceLdsLevels * kBlock);
    {
        const libm::PowTables g = libm::pow_tables();
        for (int i = tid; i < 16; i += kBlock) {
            s_pow[i] = g.invc[i];
            s_pow[16 + i] = g.logc[i];
        }
        for (int i = tid; i < 32; i += kBlock) reinterpret_cast<uint64_t*>(s_pow + 32)[i] = g.exp2[i];
    }
    constexpr int kLutBytes = kAcc ? 0 : kRenormBytes;
    float* s_lut = kAcc ? nullptr : reinterpret_cast<float*>(s_pow + 64);
    if (!kAcc) renorm_lut_fill(s_lut, tid, kBlock);
    float4* s_sph = smem + kTraceLdsLevels * kBlock + (kPowTableBytes + kLutBytes) / 16;
    float4* s_mat = s_sph + a.count;
    int* s_lights = reinterpret_cast<int*>(s_mat + 3 * a.count);
    if (kLds) {
        for (int i = tid; i < a.count; i += kBlock) s_sph[i] = a.sph[i];
        for (int i = tid; i < 3 * a.count; i += kBlock) s_mat[i] = a.mats[i];
        for (int i = tid; i < a.nlights; i += kBlock) s_lights[i] = a.lights[i];
    }
    __syncthreads();
    SceneView sc;
    sc.pow.invc = s_pow;
    sc.pow.logc = s_pow + 16;
    sc.pow.exp2 = reinterpret_cast<const uint64_t*>(s_pow + 32);
    sc.rnlut = s_lut;
    sc.sph = kLds ? s_sph : a.sph;
    sc.mats = kLds ? s_mat : a.mats;
    sc.lights = kLds ? s_lights : a.lights;
    sc.count = a.count;
    sc.nlights = a.nlights;
    sc.bv = a.bv;
    sc.gv = a.gv;
    sc.bstk = reinterpret_cast<unsigned short*>(reinterpret_cast<char*>(smem) + a.bvh_stack_offset) + tid;
    sc.bstride = kBlock;
    const size_t gtid = (size_t)blockIdx.x * kBlock + tid;
    const size_t gthreads = (size_t)gridDim.x * kBlock;
    const float invWidth = 1.0f / (float)a.width;     // parallel.cpp:260
    const float invHeight = 1.0f / (float)a.height;   // parallel.cpp:261
    // the list's length: what the scan counted, cut at the capacity (samples past it are never traced)
    const unsigned long long counted = ca.head[0];
    const long long total = counted < (unsigned long long)ca.capacity ? (long long)counted : ca.capacity;
    const long long nchunks = (total + 63) / 64;
    // block b serves queue b % kV0Queues, which owns chunks q, q + kV0Queues, ... (trace_kernel's scheme)
    const int q = blockIdx.x % kV0Queues;
    const long long bq = ((long long)gridDim.x - q + kV0Queues - 1) / kV0Queues;   // blocks serving queue q
    const long long nq = (nchunks - q + kV0Queues - 1) / kV0Queues;                 // chunks owned by queue q
    unsigned long long* ctr = ca.head + kCtrStride * (1 + q);
    int rays = 0;
    for (long long i = blockIdx.x / kV0Queues; i < nq;) {
        const long long s = (q + kV0Queues * i) * 64 + tid;
        // the next chunk is reserved before this one's trace, which hides the atomic's round trip
        unsigned long long fetched = 0;
        if (tid == 0) fetched = atomicAdd(ctr, 1ull);
        if (s < total) {
            const int p = ca.pix[s], o = ca.offs[p];
            const int c = clamped_count(ca.counts[p], a.frames);
            if ((long long)o + c <= ca.capacity) {   // (a pixel that does not fit is skipped whole)
                const int lx = p % a.xc, ly = p / a.xc;
                const int x = a.x0 + lx, y = GlobalRow(a, ly);
                const int f = a.frame0 + (int)(s - o);
                uint32_t rng = PixelSeed((uint32_t)x, (uint32_t)y, (uint32_t)f);
                float u = rng_offset(RandomK24(rng), (float)x) * invWidth;    // :272
                float v = rng_offset(RandomK24(rng), (float)y) * invHeight;   // :273
                Ray r = GetRay(a.cam, u, v, rng, sc.rnlut);
                const F3 col = Trace<MAXD, kAcc, false, kTraceLdsLevels, kNS>(r, a.maxDepth, rays, rng, sc, smem + tid, kBlock,
                                                                             a.ovf + gtid, gthreads, a.ndl, nullptr);
                ca.slots[s] = make_float4(col.x, col.y, col.z, 0.0f);
            }
        }
        const unsigned long long n = __shfl(fetched, 0, 64) + (unsigned long long)bq;
        i = n < (unsigned long long)nq ? (long long)n : nq;
    }
    // one ray-count atomic per block (a block is one wave)
    const unsigned long long t = wave_sum((unsigned long long)rays);
    if (tid == 0 && t) atomicAdd(a.rays, t);
}

// The trace stage on stream s: `a` filled for the window (kernel_args_window), a.gv.on set where the
// scene goes through the grid. The overflow stack (max_depth above the LDS levels) is per resident
// thread, allocated and freed in stream order around the launch, as launch_depth does.
template <int MAXD>
int launch_counts_trace(KernelArgs a, const CountsArgs& ca, bool lds, hipStream_t s) {
    const int acc = a.gv.on ? kAccGrid : kAccScan;
    // (a scanned scene has at most kBvhMinSpheres spheres: it is always staged in LDS)
    if (acc == kAccScan && !lds) return fail(LRT_E_STATE, "a scanned scene must fit LDS");
    const size_t stack = sizeof(float4) * kTraceLdsLevels * kBlock + kPowTableBytes + (acc ? 0 : kRenormBytes);
    const size_t scene = lds ? sizeof(float4) * (4 * (size_t)a.count + (size_t)(a.nlights + 3) / 4 + 1) : 0;
    a.bvh_stack_offset = (int)(stack + scene);
    const size_t ldsb = stack + scene;
    const bool fixed = lds && acc == kAccScan && a.count == kFixedSpheres;
    const void* kern = acc == kAccGrid ? (lds ? (const void*)counts_trace_kernel<MAXD, true, kAccGrid>
                                              : (const void*)counts_trace_kernel<MAXD, false, kAccGrid>)
                       : fixed ? (const void*)counts_trace_kernel<MAXD, true, kAccScan, kFixedSpheres>
                               : (const void*)counts_trace_kernel<MAXD, true, kAccScan>;
    int per_cu = 0;
    const hipError_t e = occupancy(&per_cu, kern, kBlock, ldsb);
    if (e != hipSuccess) return hip_fail(e, "hipOccupancyMaxActiveBlocksPerMultiprocessor");
    if (per_cu < 1) return fail(LRT_E_INVALID, "counts_trace_kernel does not fit on a CU");
    int cus = ctx().num_cus;
    for (const auto& m : ctx().masked_streams)   // a CU-masked render stream: a grid for its CUs
        if (m.first == s) cus = m.second;
    // persistent blocks, a block at least for every queue (also on a CU-masked stream left with fewer
    // slots), but no more than the list can ever have chunks: a queue without a block then owns none
    const long long most = (ca.nslots + 63) / 64;
    const long long blocks = std::max(1ll, std::min(std::max((long long)per_cu * cus, (long long)kV0Queues), most));
    const dim3 grid((unsigned)blocks);
    a.ovf = nullptr;
    if (a.maxDepth > kTraceLdsLevels) {
        const size_t gthreads = (size_t)grid.x * kBlock;
        const hipError_t me =
            hipMallocAsync((void**)&a.ovf, sizeof(float4) * gthreads * (size_t)(a.maxDepth - kTraceLdsLevels), s);
        if (me != hipSuccess) return hip_fail(me, "hipMallocAsync(trace stack overflow)");
    }
    kernel_timing(s, 0);
    if (acc == kAccGrid) {
        if (lds) counts_trace_kernel<MAXD, true, kAccGrid><<<grid, kBlock, ldsb, s>>>(a, ca);
        else counts_trace_kernel<MAXD, false, kAccGrid><<<grid, kBlock, ldsb, s>>>(a, ca);
    } else if (fixed) {
        counts_trace_kernel<MAXD, true, kAccScan, kFixedSpheres><<<grid, kBlock, ldsb, s>>>(a, ca);
    } else {
        counts_trace_kernel<MAXD, true, kAccScan><<<grid, kBlock, ldsb, s>>>(a, ca);
    }
    kernel_timing(s, 1);
    const hipError_t le = hipGetLastError();
    if (le != hipSuccess) return hip_fail(le, "counts_trace_kernel launch");
    snprintf(g_last_launch, sizeof(g_last_launch),
             "kernel=counts_trace_kernel maxd=%d lds=%d bvh=0 acc=%s ns=%d grid=%u per_cu=%d", MAXD, lds ? 1 : 0,
             acc_name(acc), fixed ? kFixedSpheres : 0, grid.x, per_cu);
    if (a.ovf) {
        const hipError_t fe = hipFreeAsync(a.ovf, s);
        if (fe != hipSuccess) return hip_fail(fe, "hipFreeAsync(trace stack overflow)");
    }
    return LRT_OK;
}

}  // namespace lrt
