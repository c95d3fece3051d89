// The render under a per-pixel count plane (lrt_render_counts_*, include/lrt.h): validation, the
// exclusive scan of the clamped counts (reduce, scan the block sums, scan again: three launches, no
// host read-back; the last one also writes the pixel of every sample of the list), the merge of a
// pixel's sample slots and the entry points. The trace stage between scan and merge is
// lrt_render_counts.h's, instantiated by the depth-class units.
#include "lrt_render_counts.h"

namespace lrt {

constexpr int kScanBlock = 256, kScanItems = 4, kScanTile = kScanBlock * kScanItems;   // counts per block
constexpr int kScanWaves = kScanBlock / 64;

struct ScanArgs {
    const int32_t* counts;
    int* offs;                      // npix + 1
    int* pix;                       // nslots: CountsArgs::pix
    long long nslots;
    unsigned long long* bsum;       // a tile's total, then (in place) the total of the tiles before it
    unsigned long long* head;       // CountsArgs::head
    int npix, ntiles, frames;
};

// The exclusive prefix of v over the block (and the block's total), 64-bit: a tile of 1024 counts of
// up to 2^31 - 1 does not fit 32 bits.
__device__ __forceinline__ unsigned long long block_exclusive(unsigned long long v, unsigned long long* total) {
    __shared__ unsigned long long wsum[kScanWaves];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned long long inc = v;
    for (int off = 1; off < 64; off <<= 1) {
        const unsigned long long up = __shfl_up(inc, off, 64);
        if (lane >= off) inc += up;
    }
    if (lane == 63) wsum[wave] = inc;
    __syncthreads();
    unsigned long long before = 0, all = 0;
    for (int w = 0; w < kScanWaves; ++w) {
        if (w < wave) before += wsum[w];
        all += wsum[w];
    }
    __syncthreads();   // (wsum is written again by the next call)
    *total = all;
    return before + inc - v;
}

// This thread's kScanItems consecutive clamped counts of tile blockIdx.x, and their sum.
__device__ __forceinline__ unsigned long long tile_counts(const ScanArgs& a, int c[kScanItems]) {
    const long long i0 = (long long)blockIdx.x * kScanTile + (long long)threadIdx.x * kScanItems;
    unsigned long long sum = 0;
#pragma unroll
    for (int k = 0; k < kScanItems; ++k) {
        c[k] = i0 + k < a.npix ? clamped_count(a.counts[i0 + k], a.frames) : 0;
        sum += (unsigned long long)c[k];
    }
    return sum;
}

// ---- scan 1: a tile's total.
__global__ __launch_bounds__(kScanBlock) void counts_reduce_kernel(const ScanArgs a) {
    int c[kScanItems];
    unsigned long long total;
    (void)block_exclusive(tile_counts(a, c), &total);
    if (threadIdx.x == 0) a.bsum[blockIdx.x] = total;
}

// ---- scan 2: one block turns the tile totals into the totals before each tile, in place: a thread
// sums a run of consecutive tiles, the runs are scanned across the block, the thread walks its run
// again. It also arms the call's head: the grand total, the info word and the chunk queues' counters.
__global__ __launch_bounds__(kScanBlock) void counts_spine_kernel(const ScanArgs a) {
    const int run = (a.ntiles + kScanBlock - 1) / kScanBlock;
    const int b0 = min(threadIdx.x * run, a.ntiles), b1 = min(b0 + run, a.ntiles);
    unsigned long long sum = 0;
    for (int b = b0; b < b1; ++b) sum += a.bsum[b];
    unsigned long long total;
    unsigned long long at = block_exclusive(sum, &total);
    for (int b = b0; b < b1; ++b) {
        const unsigned long long v = a.bsum[b];
        a.bsum[b] = at;
        at += v;
    }
    if (threadIdx.x == 0) {
        a.head[0] = total;
        a.head[1] = 0;
        a.offs[a.npix] = (int)min(total, (unsigned long long)kCountsSat);
    }
    if (threadIdx.x < kV0Queues) a.head[kCtrStride * (1 + threadIdx.x)] = 0;
}

// ---- scan 3: the offsets of a tile's pixels, saturated, and the pixel of each of their samples
// (below nslots: a sample past the capacity is never traced). A thread writes its pixel's run itself
// up to 64 samples; a longer run is written by the pixel's whole wave, 64 samples a step.
__global__ __launch_bounds__(kScanBlock) void counts_offsets_kernel(const ScanArgs a) {
    int c[kScanItems];
    unsigned long long total;
    unsigned long long at = a.bsum[blockIdx.x] + block_exclusive(tile_counts(a, c), &total);
    const long long i0 = (long long)blockIdx.x * kScanTile + (long long)threadIdx.x * kScanItems;
    const int lane = threadIdx.x & 63;
    const unsigned long long nslots = (unsigned long long)a.nslots;
#pragma unroll
    for (int k = 0; k < kScanItems; ++k) {   // (c[k] is 0 past the window's last pixel)
        const int p = (int)(i0 + k);
        if (i0 + k < a.npix) a.offs[p] = (int)min(at, (unsigned long long)kCountsSat);
        const bool wide = c[k] > 64;
        if (!wide)
            for (int j = 0; j < c[k] && at + j < nslots; ++j) a.pix[at + j] = p;
        unsigned long long todo = __ballot(wide);
        while (todo) {   // uniform
            const int src = __ffsll((long long)todo) - 1;
            todo &= todo - 1;
            const unsigned long long o = __shfl(at, src, 64);
            const int n = __shfl(c[k], src, 64), pp = __shfl(p, src, 64);
            for (int j = lane; j < n && o + j < nslots; j += 64) a.pix[o + j] = pp;
        }
        at += (unsigned long long)c[k];
    }
}

// ---- merge: a thread per pixel, a bounded grid striding over the window. A rendered pixel's slots
// lerped in frame order from the buffer's value (merge_samples_kernel's chain), then the LRT_RC_MEAN
// factor; rgb only. The call's two info words are summed per block and added, packed into one word
// (traced <= 2^27 in bits 0-31, skipped above), with one atomic per block: same-address atomics
// serialise, hence the bounded grid.
__global__ __launch_bounds__(kScanBlock) void merge_counts_kernel(const CountsArgs ca, float4* __restrict__ out,
                                                                  const float* lerp, int frame0, int frames, int mean,
                                                                  int want_info) {
    unsigned long long word = 0;
    const int stride = gridDim.x * kScanBlock;   // npix + stride <= INT_MAX / 4 + 2^21
    for (int i = blockIdx.x * kScanBlock + threadIdx.x; i < ca.npix; i += stride) {
        const int c = clamped_count(ca.counts[i], frames);
        const int o = ca.offs[i];
        if (c > 0 && (long long)o + c <= ca.capacity) {
            const float4 prev = out[i];
            F3 acc = f3(prev.x, prev.y, prev.z);
            for (int k = 0; k < c; ++k) {
                const float4 s = ca.slots[(size_t)o + k];
                const int f = frame0 + k;
                const float lerpFac = f < kLerpTable ? lerp[f] : (float)f / (float)(f + 1);
                acc = acc * lerpFac + f3(s.x, s.y, s.z) * (1.0f - lerpFac);
            }
            if (mean) {
                const float scale = (float)(frame0 + c) / (float)c;
                acc = f3(acc.x * scale, acc.y * scale, acc.z * scale);
            }
            float* d = reinterpret_cast<float*>(out + i);   // alpha untouched
            d[0] = acc.x;
            d[1] = acc.y;
            d[2] = acc.z;
            word += (unsigned long long)c;
        } else if (c > 0) {
            word += 1ull << 32;
        }
    }
    if (!want_info) return;   // uniform
    __shared__ unsigned long long part[kScanWaves];
    word = wave_sum(word);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = word;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long t = 0;
        for (int w = 0; w < kScanWaves; ++w) t += part[w];
        if (t) atomicAdd(ca.head + 1, t);
    }
}

__global__ void counts_info_kernel(const unsigned long long* head, unsigned long long* info) {
    info[0] = head[1] & 0xffffffffull;
    info[1] = head[1] >> 32;
}

// Everything that needs neither the library's state nor the device.
static int validate_counts(const lrt_render_desc* d, const lrt_render_counts* rc, const float* buf, const void* rays) {
    if (int e = validate(d)) return e;
    if (!buf || !rays) return fail(LRT_E_INVALID, "device buffer / ray counter is NULL");
    if (d->flags != LRT_F_NONE) return fail(LRT_E_INVALID, "a counted render takes no LRT_F_* flag");
    if ((long long)d->x_count * d->row_count > INT_MAX / 4) return fail(LRT_E_INVALID, "window too large");
    if (!rc) return fail(LRT_E_INVALID, "rc is NULL");
    if (!rc->counts) return fail(LRT_E_INVALID, "counts is NULL");
    if (rc->capacity < 1 || rc->capacity > kCountsCapacityMax) return fail(LRT_E_INVALID, "capacity must be 1 .. 2^27");
    if ((rc->flags & ~LRT_RC_MEAN) != 0 || rc->reserved != 0)
        return fail(LRT_E_INVALID, "unknown flag, or reserved != 0");
    const size_t px = (size_t)d->x_count * d->row_count;
    const Span outs[2] = {{buf, 16 * px}, {rc->info, 16}}, ins[1] = {{rc->counts, 4 * px}};
    if (spans_alias(outs, 2, ins, 1) || ranges_overlap(rays, 8, rc->counts, 4 * px) ||
        ranges_overlap(rays, 8, rc->info, 16))
        return fail(LRT_E_INVALID, "aliasing: counts or info overlaps the backbuffer, the ray counter or each other");
    return LRT_OK;
}

// The call on stream s (device pointers, validated; context 0 is current).
static int counts_device(const lrt_render_desc* d, const lrt_render_counts* rc, float* d_buf, unsigned long long* d_rays,
                         hipStream_t s) {
    Context& c = ctx();
    const long long npix = (long long)d->x_count * d->row_count;
    if (npix == 0 || d->frames == 0) {   // no pixel can have a sample
        if (rc->info) LRT_HIP(hipMemsetAsync(rc->info, 0, 16, s));
        return LRT_OK;
    }
    if (c.count < 1) return fail(LRT_E_STATE, "no scene");
    const bool grid = c.count > kBvhMinSpheres;   // as lrt_gbuffer_chain_* decides
    if (grid)
        if (int e = ensure_grid(c)) return e;
    if (grid && !c.grid_built) return fail(LRT_E_STATE, "the grid is not built");
    KernelArgs a;
    memset(&a, 0, sizeof(a));
    kernel_args_window(d, d_buf, d_rays, a);
    a.bv = c.bvh;
    a.bv.on = 0;
    a.gv = c.gv;
    a.gv.on = grid ? 1 : 0;
    a.lerp = c.d_lerp;
    const bool lds = sizeof(float4) * (kTraceLdsLevels * kBlock + 4 * (size_t)a.count + a.nlights / 4 + 1) <= 64 * 1024;
    // the scratch: [head][tile sums][offsets][sample pixels][slots], each part on a 256-B boundary
    const int ntiles = (int)((npix + kScanTile - 1) / kScanTile);
    const long long nslots = std::min<long long>(rc->capacity, npix * (long long)d->frames);
    auto up = [](size_t b) { return (b + 255) / 256 * 256; };
    const size_t head_b = up(kCountsHeadBytes), bsum_b = up(sizeof(unsigned long long) * (size_t)ntiles),
                 offs_b = up(sizeof(int) * (size_t)(npix + 1)), pix_b = up(sizeof(int) * (size_t)nslots),
                 slots_b = sizeof(float4) * (size_t)nslots;
    void* p = nullptr;
    if (int e = scratch_or_fail(s, head_b + bsum_b + offs_b + pix_b + slots_b, "render counts scratch", &p)) return e;
    char* base = static_cast<char*>(p);
    ScanArgs sa;
    memset(&sa, 0, sizeof(sa));
    sa.counts = rc->counts;
    sa.head = reinterpret_cast<unsigned long long*>(base);
    sa.bsum = reinterpret_cast<unsigned long long*>(base + head_b);
    sa.offs = reinterpret_cast<int*>(base + head_b + bsum_b);
    sa.pix = reinterpret_cast<int*>(base + head_b + bsum_b + offs_b);
    sa.nslots = nslots;
    sa.npix = (int)npix;
    sa.ntiles = ntiles;
    sa.frames = d->frames;
    counts_reduce_kernel<<<ntiles, kScanBlock, 0, s>>>(sa);
    LRT_HIP(hipGetLastError());
    counts_spine_kernel<<<1, kScanBlock, 0, s>>>(sa);
    LRT_HIP(hipGetLastError());
    counts_offsets_kernel<<<ntiles, kScanBlock, 0, s>>>(sa);
    LRT_HIP(hipGetLastError());
    CountsArgs ca;
    memset(&ca, 0, sizeof(ca));
    ca.counts = rc->counts;
    ca.offs = sa.offs;
    ca.head = sa.head;
    ca.pix = sa.pix;
    ca.slots = reinterpret_cast<float4*>(base + head_b + bsum_b + offs_b + pix_b);
    ca.nslots = nslots;
    ca.npix = (int)npix;
    ca.capacity = rc->capacity;
    if (int e = d->max_depth <= 8 ? launch_counts_d8(a, ca, lds, s) : launch_counts_d64(a, ca, lds, s)) return e;
    const long long mblocks = std::min((npix + kScanBlock - 1) / kScanBlock, 4ll * c.num_cus);
    merge_counts_kernel<<<(unsigned)mblocks, kScanBlock, 0, s>>>(ca, a.out, a.lerp, d->frame0, d->frames,
                                                                (rc->flags & LRT_RC_MEAN) ? 1 : 0, rc->info ? 1 : 0);
    LRT_HIP(hipGetLastError());
    if (rc->info) {
        counts_info_kernel<<<1, 1, 0, s>>>(ca.head, rc->info);
        LRT_HIP(hipGetLastError());
    }
    LRT_HIP(stream_scratch_used(s));
    return LRT_OK;
}

}  // namespace lrt

using namespace lrt;

extern "C" {

int lrt_render_counts_device(const lrt_render_desc* desc, const lrt_render_counts* d_rc, float* d_backbuffer,
                             unsigned long long* d_rays, void* stream) {
    RoctxRange rr_("lrt_render_counts_device");
    if (int rc = validate_counts(desc, d_rc, d_backbuffer, d_rays)) return rc;
    std::lock_guard<std::mutex> lk(g_mu);
    if (int rc = require_initialized()) return rc;
    DeviceScope ds_(0);   // context 0's device (device 0 of lrt_initialize_devices)
    return counts_device(desc, d_rc, d_backbuffer, d_rays, (hipStream_t)stream);
}

int lrt_render_counts_host(const lrt_render_desc* desc, const lrt_render_counts* rc, float* backbuffer,
                           long long* out_rays) {
    RoctxRange rr_("lrt_render_counts_host");
    unsigned long long rays = 0;
    if (int e = validate_counts(desc, rc, backbuffer, &rays)) return e;
    std::lock_guard<std::mutex> lk(g_mu);
    if (int e = require_initialized()) return e;
    DeviceScope ds_(0);
    hipStream_t s = ctx().stream;
    const size_t npix = (size_t)desc->x_count * desc->row_count;
    // Device mirrors: the backbuffer (copied in first: prev values, alphas and the pixels not rendered
    // stay), the counts, the info words and the ray counter, which starts at the zero uploaded here.
    HostMirrors m;
    const int buf_ = m.inout(npix ? backbuffer : nullptr, npix * 16);
    const int counts_ = m.in(npix ? rc->counts : nullptr, npix * 4);
    const int info_ = m.out(rc->info, 16), rays_ = m.inout(&rays, sizeof(rays));
    if (int e = m.alloc("hipMalloc(render counts staging)")) return e;
    if (int e = m.upload(s)) return e;
    lrt_render_counts d_rc = *rc;
    d_rc.counts = m.dev<int32_t>(counts_);
    d_rc.info = m.dev<unsigned long long>(info_);
    if (npix == 0) d_rc.counts = rc->counts;   // (not read: the call returns before any launch)
    if (int e = counts_device(desc, &d_rc, npix ? m.dev<float>(buf_) : backbuffer, m.dev<unsigned long long>(rays_), s))
        return e;
    if (int e = m.download(s)) return e;
    if (out_rays) *out_rays = (long long)rays;
    return LRT_OK;
}

}  // extern "C"
