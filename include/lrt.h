/* lrt.h — C-ABI of the MI355X path tracer (liblrt_hip.so).
 *
 * Drop-in boundary for the reference's src/cpu renderer API
 * (Sefaice/LearnRayTracing src/cpu/parallel.h:6-8):
 *
 *     void InitializeTest();                                         -> lrt_initialize
 *     void ShutdownTest();                                           -> lrt_shutdown
 *     void DrawTest(float time, int frameCount, int screenWidth,
 *                   int screenHeight, float* backbuffer, int& outRayCount);
 *                                                                    -> lrt_draw_test
 *
 * plus the extended entry points the multi-GPU / benchmark callers need
 * (runtime scene and camera, device-resident progressive buffer, S samples per
 * call, D bounces, row-block-cyclic sharding, 64-bit ray counts).
 *
 * Plain types and pointers only. Every function returns LRT_OK (0) or a negative
 * LRT_E_* code; lrt_last_error() describes the last failure of the calling thread.
 * Not re-entrant per process (like the reference's global scheduler, parallel.cpp:229).
 */
#ifndef LRT_H
#define LRT_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LRT_OK 0
#define LRT_E_INVALID (-1) /* bad argument (sizes, pointers, scene contents)        */
#define LRT_E_HIP (-2)     /* a HIP runtime call failed                              */
#define LRT_E_STATE (-3)   /* lrt_initialize() not called / already shut down        */
#define LRT_E_NOMEM (-4)   /* device allocation failed                               */

/* Material::Type, parallel.cpp:31 */
#define LRT_LAMBERT 0
#define LRT_METAL 1
#define LRT_DIELECTRIC 2

/* Reference kMaxDepth (parallel.cpp:12): lrt_draw_test allows this many scatter events. */
#define LRT_REFERENCE_MAX_DEPTH 20
/* Largest scene the device path accepts (spheres + materials are staged per workgroup). */
#define LRT_MAX_SPHERES 4096

/* float3, maths.h:10-61 (12 bytes, no padding) */
typedef struct lrt_float3 { float x, y, z; } lrt_float3;

/* Sphere, maths.h:156-163 (16 bytes) */
typedef struct lrt_sphere { lrt_float3 center; float radius; } lrt_sphere;

/* Material, parallel.cpp:29-37 (36 bytes: type @0, albedo @4, emissive @16,
 * roughness @28, ri @32). type is the enum's int value. */
typedef struct lrt_material {
    int32_t type;
    lrt_float3 albedo;
    lrt_float3 emissive;
    float roughness;
    float ri;
} lrt_material;

/* Camera, maths.h:176-225 (88 bytes: the member order of the reference). */
typedef struct lrt_camera {
    lrt_float3 origin;
    lrt_float3 a, u, r;
    lrt_float3 lowerLeftCorner;
    lrt_float3 horizontalVec;
    lrt_float3 verticalVec;
    float lensRadius;
} lrt_camera;

/* One render call (the extended form of DrawTest, parallel.cpp:297-323).
 *
 * The image is width x height; pixel (x, y) has row 0 at the bottom (v grows with y,
 * maths.h:198,214). The call renders the column window [x0, x0 + x_count) of
 * row_count LOCAL rows; local row ly maps to the global row
 *     y = y0 + (ly / row_block) * row_block * row_period + row_phase * row_block + ly % row_block
 * (row_period = 1, row_phase = 0 gives the contiguous rows y0 .. y0 + row_count - 1;
 *  row_period = G, row_phase = g gives GPU g's share of a row-block-cyclic split).
 * For each pixel it runs samples frame0 .. frame0 + frames - 1 in order; sample f
 * uses the per-pixel XorShift32 stream seeded with
 *     ((uint32)(x * 1973 + y * 9277 + f * 26699)) | 1
 * and is blended into the buffer with the reference's progressive lerp
 * (parallel.cpp:262,280-286): rgb = prev * (f / (f + 1)) + col * (1 - f / (f + 1)).
 * max_depth is the number of scatter events a path may take (the reference's
 * kMaxDepth = 20; "8 bounces" = 8). */
typedef struct lrt_render_desc {
    lrt_camera camera;
    int32_t width, height;
    int32_t x0, x_count;
    int32_t y0, row_count;
    int32_t row_block, row_period, row_phase;
    int32_t frame0, frames;
    int32_t max_depth;
    int32_t flags; /* LRT_F_* */
} lrt_render_desc;

#define LRT_F_NONE 0
#define LRT_F_SCENE_GLOBAL 1 /* read the scene from global memory instead of LDS staging */
#define LRT_F_SIMPLE 2       /* v0 kernel (the default): the reference's per-pixel loop,
                                a pixel's frames spread over adjacent lanes, persistent
                                single-wave blocks fed from tile queues               */
#define LRT_F_NO_BVH 32      /* scan every sphere (the reference's HitWorld loop) even
                                when the scene has a BVH (> 16 spheres)                */
#define LRT_F_NO_DOUBLE_LIGHT 64 /* opt-in GL-path rule (fragmentShader.fs.glsl:430,456-457,
                                "doMaterialE"): a scatter event reached through a Lambert
                                bounce does not add its emissive again (that light was
                                sampled explicitly); the terminating hit always adds it.
                                Off by default: the CPU reference double counts
                                (parallel.cpp:214). v0 kernel only.                   */
#define LRT_F_WAVEFRONT 256  /* v4: wavefront (breadth-first) path tracing: path state in
                                HBM, closest-hit and per-material shading kernels over
                                compacted queues, frame planes merged in order. No
                                lrt_features.                                          */

#define LRT_F_POOL 512       /* v5 kernel: the v0 loop with sample-pool regeneration: a lane
                                whose path ends takes the wave's next pixel-sample at once;
                                colours are lerped in frame order per pixel when the pool
                                is done. No lrt_features (lrt_gbuffer_* gives guides). */
#define LRT_F_BVH 1024       /* closest hits through the 4-wide BVH even where the library
                                would pick the uniform grid (scenes above 16 spheres) */
#define LRT_F_GRID 2048      /* closest hits through the uniform grid (lrt_grid.h) even where
                                the library would pick the BVH; same bits either way */
/* With none of SIMPLE / WAVEFRONT / POOL set the library picks v0 or v5 per call. Any bit not
 * defined above (4, 8, 16 and 128 belonged to kernels removed in rounds 2-3) is rejected with
 * LRT_E_INVALID. */

/* ---- the reference API (parallel.h:6-8) ---------------------------------- */

/* InitializeTest (parallel.cpp:231-235): binds the calling thread's current HIP device,
 * creates the stream, uploads the reference's default 9-sphere scene (parallel.cpp:15-51). */
int lrt_initialize(void);

/* ShutdownTest (parallel.cpp:237-240): frees every device resource. */
int lrt_shutdown(void);

/* DrawTest (parallel.cpp:297-323): one progressive frame of the current scene with
 * DrawTest's camera (parallel.cpp:299-307) and kMaxDepth 20 into a caller-owned host
 * buffer of screenWidth*screenHeight*4 floats (RGBA stride, alpha untouched), blocking.
 * `time` is accepted and unused, as in the reference. */
int lrt_draw_test(float time, int frameCount, int screenWidth, int screenHeight,
                  float* backbuffer, int* outRayCount);

/* ---- multi-GPU (one process) ---------------------------------------------- */

/* InitializeTest over several devices (BASELINE config 5: the frame row-tiled across the
 * node's GPUs). Instead of lrt_initialize: n device ids (n = 0 and device_ids = NULL: every
 * visible device). Afterwards lrt_draw_test and lrt_render_host(_ex without features) split
 * the caller's rows over all of them in blocks of 8 rows dealt round-robin (row-block-cyclic;
 * LRT_ROW_BLOCK overrides); each device copies its rows' previous values from the caller's
 * buffer (page-locked for the call), renders them, and by default copies them straight back
 * over its own PCIe link. With LRT_DEV_GATHER the shards' RGB is gathered into the first
 * device instead -- ncclCommInitAll + a grouped ncclGather (RCCL, over xGMI) when the ids are
 * distinct, device-to-device copies when an id repeats (RCCL refuses two ranks on one GPU) or
 * with LRT_DEV_PEER_COPY -- which assembles the frame and copies it to the caller. The result
 * is bit-identical to one device either way. The other calls (lrt_render_device, streams,
 * scene) act on the first device; lrt_set_scene updates every device. lrt_shutdown releases
 * all. */
#define LRT_DEV_PEER_COPY 1 /* gather, with device-to-device copies instead of RCCL */
#define LRT_DEV_GATHER 2    /* gather the shards into the first device (RCCL when the ids are distinct) */
int lrt_initialize_devices(int n, const int* device_ids, int flags);
/* Bytes one multi-device host render of an x_count x rows window moves between the devices
 * and the caller: *direct = the RGBA rows each device copies back over its own link (the
 * default exchange); *gather_xgmi = the packed RGB (12 B per pixel) the other devices' shards
 * send to the first one (LRT_DEV_GATHER). No device is touched. */
int lrt_exchange_bytes(int x_count, int rows, int row_block, int devices, long long* direct, long long* gather_xgmi);
/* Devices in use (0 before lrt_initialize / lrt_initialize_devices). */
int lrt_device_count(void);

/* ---- extended API -------------------------------------------------------- */

const char* lrt_last_error(void);
/* Library version string ("lrt-mi355x <semver> gfx950"). */
const char* lrt_version(void);
/* The kernel instance the last render call on any thread launched, as "key=value" words
 * (e.g. "kernel=trace_kernel maxd=8 lds=1 bvh=1 split=16 samp=0 feat=0 ns=0 grid=4096
 * tasks=..."): lets tests and benchmarks name the exact instance they exercised. */
const char* lrt_last_launch(void);

/* Camera constructor (maths.h:183-202). */
int lrt_camera_make(lrt_float3 lookFrom, lrt_float3 lookAt, lrt_float3 vup, float vfov,
                    float aspect, float aperture, float focusDist, lrt_camera* out);
/* DrawTest's camera for a width x height image (parallel.cpp:299-307). */
int lrt_camera_default(int width, int height, lrt_camera* out);

/* Replace the scene (the reference's s_Spheres / s_SphereMats, parallel.cpp:15-51).
 * 1 <= count <= LRT_MAX_SPHERES; material types must be 0..2. Emissive spheres are
 * those with any emissive channel > 0 (parallel.cpp:96). */
int lrt_set_scene(const lrt_sphere* spheres, const lrt_material* materials, int count);
/* The scene the devices hold (what lrt_set_scene last uploaded, or the default scene):
 * *count spheres; copies them when capacity >= *count. */
int lrt_get_scene(lrt_sphere* spheres, lrt_material* materials, int capacity, int* count);

/* Copy the reference's default scene (9 spheres) into caller arrays of >= 9 entries. */
int lrt_default_scene(lrt_sphere* spheres, lrt_material* materials, int capacity, int* count);

/* Render into a DEVICE buffer of row_count * x_count RGBA float quads (row-major,
 * local rows), adding the counted rays into *d_rays (device uint64, caller-zeroed).
 * Asynchronous on `stream` (a hipStream_t, used as given: NULL is the default stream), and
 * ordered only against that stream: a buffer or counter filled on another stream must be
 * ordered before the call by the caller (an event, or a stream wait). */
int lrt_render_device(const lrt_render_desc* desc, float* d_backbuffer,
                      unsigned long long* d_rays, void* stream);

/* lrt_render_device plus the multi-GPU frame exchange fused into the render: every finished
 * pixel is also stored, as RGBA, into d_frame -- the whole width x height frame, row-major --
 * at its global row (the row map above). d_frame may be another device's memory opened with
 * lrt_ipc_open (one process per GPU) or peer-accessible memory: each rank's render writes its
 * rows straight into rank 0's frame over xGMI, with no pack, gather or assembly launch; the
 * frame is complete once every rank's render has completed (e.g. after a barrier). */
int lrt_render_device_to_frame(const lrt_render_desc* desc, float* d_backbuffer,
                               unsigned long long* d_rays, float* d_frame, void* stream);

/* Device memory shareable across processes (hipIpc*) for that exchange: lrt_ipc_alloc makes a
 * zeroed buffer of `bytes` on the first device and its handle (LRT_IPC_HANDLE_BYTES bytes, to
 * send to the other processes); lrt_ipc_open maps a handle from another process (peer access
 * enabled lazily); lrt_ipc_close unmaps it; lrt_ipc_free frees an lrt_ipc_alloc buffer. */
#define LRT_IPC_HANDLE_BYTES 64
int lrt_ipc_alloc(size_t bytes, void** d_ptr, void* handle);
int lrt_ipc_free(void* d_ptr);
int lrt_ipc_open(const void* handle, void** d_ptr);
int lrt_ipc_close(void* d_ptr);

/* Same on a HOST buffer: H2D of prev, render, D2H, blocking. *out_rays = counted rays. */
int lrt_render_host(const lrt_render_desc* desc, float* backbuffer, long long* out_rays);

/* Opt-in first-hit features of the reference's GL path (fragmentShader.fs.glsl:444-451,
 * 494-568): per pixel, running means (the backbuffer's lerp, parallel.cpp:282) of the
 * first hit's normal, world position and material albedo (zero on a camera-ray miss),
 * and running standard deviations (AdaptiveStdvar, :494-497, pow(x,2) taken as x*x) of
 * the linear colour, the normal and the world position. Each non-NULL buffer has the
 * backbuffer's shape (row_count * x_count RGBA float quads, alpha untouched) and is
 * read and updated in place; features update for frames f <= max_frame (the GL path
 * uses 4), every frame if max_frame < 0. The backbuffer is bit-identical to a render
 * without features. v0 kernel only; a feature render keeps each pixel on one lane. */
typedef struct lrt_features {
    float* normal;
    float* world_pos;
    float* albedo;
    float* color_std;
    float* normal_std;
    float* world_pos_std;
    int32_t max_frame;
    int32_t reserved;   /* 0 */
} lrt_features;

/* lrt_render_device / lrt_render_host with features (device resp. host buffers;
 * features == NULL is the plain call). */
int lrt_render_device_ex(const lrt_render_desc* desc, float* d_backbuffer,
                         unsigned long long* d_rays, const lrt_features* d_features, void* stream);
int lrt_render_host_ex(const lrt_render_desc* desc, float* backbuffer, long long* out_rays,
                       const lrt_features* features);

/* A render stream for lrt_render_device(_ex) that leaves the last `reserved_cus` CUs of the
 * device free (hipExtStreamCreateWithCUMask), so that work on other streams -- the RCCL
 * gather of the previous frame -- can run beside the persistent render kernel instead of
 * waiting for its workgroups to retire; renders on it size their grid to the remaining
 * CUs. Destroy with lrt_stream_destroy (lrt_shutdown destroys any left). */
int lrt_stream_create(int reserved_cus, void** stream);
int lrt_stream_destroy(void* stream);

/* Page-locked host memory for a backbuffer (hipHostMalloc; contents undefined, like the
 * `new float[]` of main.cpp:40 it replaces). lrt_draw_test / lrt_render_host(_ex without
 * features) detect such a buffer -- or any other page-locked one -- and render it in place
 * over PCIe instead of staging it through device memory either side of the kernel
 * (LRT_HOST_ZEROCOPY=0 turns that off). Free with lrt_host_free. */
int lrt_host_alloc(size_t bytes, void** out);
int lrt_host_free(void* p);
/* A PAGEABLE host backbuffer (the reference's `new float[]`, main.cpp:40) is page-locked by
 * lrt_draw_test / lrt_render_host for the duration of that one call (hipHostRegister when it
 * starts, hipHostUnregister before it returns) and takes the page-locked paths. The library
 * keeps nothing of the caller's buffer between calls: the caller may free it, or reuse or
 * remap its address, at any time between calls -- DrawTest's own contract (parallel.h:8).
 * LRT_HOST_REGISTER=0 stages pageable buffers instead. */

/* Number of local rows GPU `phase` owns in a row-block-cyclic split of `height` rows
 * into blocks of row_block rows dealt over `period` GPUs. */
int lrt_shard_rows(int height, int row_block, int period, int phase);

/* Frame assembly after a gather: src holds `period` shard buffers of max_rows rows each
 * (max_rows = lrt_shard_rows(height, row_block, period, 0)), shard g at
 * src + g * max_rows * width * 4; dst receives the full width x height RGBA image.
 * Device pointers, asynchronous on stream. */
int lrt_unshard_rows(const float* d_src, float* d_dst, int width, int height, int row_block,
                     int period, void* stream);

/* The RGB-only form of the exchange (12 of 16 bytes per pixel cross the interconnect; the
 * render never writes alpha): lrt_pack_rgb copies npix RGBA quads to packed RGB triples;
 * lrt_unshard_rows_rgb assembles `period` packed shards of max_rows rows each (shard g at
 * d_src_rgb + g * max_rows * width * 3) into the RGBA frame, leaving its alpha untouched.
 * Device pointers, asynchronous on stream. */
int lrt_pack_rgb(const float* d_rgba, float* d_rgb, long long npix, void* stream);
int lrt_unshard_rows_rgb(const float* d_src_rgb, float* d_dst, int width, int height, int row_block,
                         int period, void* stream);

/* Present step (main.cpp:109-141 LinearToSRGB + BGRA8 pack, GDI blit removed):
 * d_rgba (width*height*4 floats) -> d_bgra (width*height uint32, b | g<<8 | r<<16). */
int lrt_present_bgra8(const float* d_rgba, uint32_t* d_bgra, int width, int height, void* stream);

/* ---- denoiser ---------------------------------------------------------------- */

/* Feature-guided denoiser for a rendered frame: an edge-avoiding a-trous wavelet filter
 * (Dammertz et al. 2010) over the guides lrt_render_device_ex / lrt_render_host_ex produce,
 * its colour weight scaled by the centre pixel's colour standard deviation (as in SVGF).
 * `iterations` passes k = 0 .. iterations - 1 with the 5x5 B3-spline taps
 * q = p + 2^k * (i, j), i, j in -2..2, h = [1/16, 1/4, 3/8, 1/4, 1/16]; taps outside the
 * image are skipped:
 *     c_{k+1}(p) = sum_q w(p,q) c_k(q) / sum_q w(p,q)                     (rgb only)
 *     w(p,q) = h[i] h[j] exp(-E(p,q))
 *     E = |c_k(p) - c_k(q)|^2 / ((sigma_color 2^-k)^2 |std(p)|^2 + 1e-6)   if color_std is given
 *       + |n(p) - n(q)|^2 / sigma_normal^2                                 if normal is given
 *       + |x(p) - x(q)|^2 / sigma_pos^2                                    if world_pos is given
 *       + |a(p) - a(q)|^2 / sigma_albedo^2                                 if albedo is given
 * (|.|^2: the squared rgb distance; the guides are the input buffers, unchanged over the
 * passes). f32 throughout, deterministic run to run; tolerance-checked against its NumPy
 * restatement (tests/denoise_ref.py), not bit-pinned: the reference has no such filter.
 *
 * Whole frames only: every buffer is height rows of width RGBA float quads. A
 * row-block-cyclic shard (row_period > 1) lacks its rows' neighbours and cannot be filtered
 * on its own -- assemble the frame first. No temporal reuse of its own (lrt_temporal_* below is
 * the stage for that). This filter does not demodulate albedo and reads color_std as it is, the
 * same value at every pass; lrt_svgf_* (further below) is the filter that divides albedo out and
 * filters and propagates the variance, from the temporal state directly. */
#define LRT_DENOISE_MAX_ITER 5
typedef struct lrt_denoise_desc {
    int32_t width, height;      /* a whole frame: height rows of width RGBA float quads */
    int32_t iterations;         /* 1..LRT_DENOISE_MAX_ITER */
    int32_t flags;              /* 0 */
    float sigma_color, sigma_normal, sigma_pos, sigma_albedo;   /* finite, > 0 */
} lrt_denoise_desc;

/* The defaults for a width x height frame: 5 iterations, sigma_color 2, sigma_normal 0.3,
 * sigma_pos 0.5, sigma_albedo 0.2. */
int lrt_denoise_default(int width, int height, lrt_denoise_desc* out);

/* Filter d_color into d_out (device buffers). Of d_guides, normal, world_pos, albedo and
 * color_std are read (a NULL member drops its term; without color_std there is no colour
 * term); the other members and max_frame are ignored; d_guides == NULL means no guides.
 * d_out may be d_color (in place) but not one of the guide buffers (LRT_E_INVALID); only its
 * rgb is written, its alpha stays. No input is written when d_out != d_color. Asynchronous on
 * `stream` and ordered only against it, like lrt_render_device; the intermediate passes live
 * in that stream's scratch of the library. Acts on the first device. */
int lrt_denoise_device(const lrt_denoise_desc* desc, const float* d_color, const lrt_features* d_guides,
                       float* d_out, void* stream);

/* Same on HOST buffers: staged through device memory, blocking; the output equals
 * lrt_denoise_device's bit for bit. */
int lrt_denoise_host(const lrt_denoise_desc* desc, const float* color, const lrt_features* guides, float* out);

/* ---- temporal reprojection and accumulation ------------------------------------ */

/* The first stage of SVGF, ahead of the denoiser: find each pixel's surface point in the previous
 * frame, blend that frame's history in, and keep a second moment, so that render (1-4 spp, moving
 * camera) -> temporal accumulate -> denoise -> present stays on the device and the denoiser gets a
 * variance guide that a single frame cannot give. All buffers are whole frames: `height` rows of
 * `width` RGBA float quads, row 0 at the bottom. f32 throughout.
 *
 * Per pixel p = (x, y), with the current colour and guides each times cur_scale = k:
 *     C = k color.rgb, N = k normal.rgb, X = k world_pos.rgb, A = k albedo.rgb
 * the current camera O, L, H, V (origin, lowerLeftCorner, horizontalVec, verticalVec) and the
 * previous camera O', a', L', H', V':
 *  1. hit = |N|^2 >= 0.25 (a camera miss has zero features; a pixel whose samples mix hit and
 *     miss counts as a miss below one half).
 *  2. Pixel-centre direction D = L + ((x + 1/2) / w) H + ((y + 1/2) / h) V - O.
 *  3. The surface point of the pixel CENTRE, not of the jittered sample (reprojecting the jittered
 *     X lands up to half a pixel off and blurs the history even under a static camera): if hit,
 *     |D.N| > 1e-3 |D| and lambda = ((X - O).N) / (D.N) > 0 then Xc = O + lambda D, else Xc = X.
 *     The target is d = Xc - O' for a hit, d = D (the point at infinity that way) for a miss.
 *  4. Into the previous camera: da = d.a' (in front iff da < 0), fd = -(L' - O').a',
 *     q = (-fd / da) d - (L' - O'), fx = (q.H') / (H'.H') w - 1/2, fy = (q.V') / (V'.V') h - 1/2.
 *     No history if the point is not in front, if anything is non-finite, or if |fx| or |fy| is
 *     >= 1e6. The lens offset is ignored.
 *  5. Four bilinear taps Q = (floor(fx) + i, floor(fy) + j), i, j in 0..1, weights b_ij. A tap
 *     counts iff it lies inside the image and is consistent: with hit'(Q) = |N'(Q)|^2 >= 0.25, a
 *     hit pixel needs hit'(Q), N'(Q).N >= normal_min and
 *     |X'(Q) - Xc|^2 <= pos_tol^2 |Xc - O|^2; a miss pixel needs !hit'(Q).
 *  6. sw = sum of b over the counting taps. With sw > 1e-3: history n = sum b n'(Q) / sw + 1,
 *     alpha = max(1 / n, alpha_min), color = (1 - alpha) sum b c'(Q) / sw + alpha C,
 *     moment2 = (1 - alpha) sum b m2'(Q) / sw + alpha C^2 per channel. Otherwise, and whenever
 *     there is no previous state: color = C, moment2 = C^2, n = 1.
 *  7. std = sqrt(max(moment2 - color^2, 0)) per channel; where n < min_history,
 *     std = (short_std, short_std, short_std) instead: a large value switches the denoiser's colour
 *     term off where the variance is not yet known (a disoccluded pixel would otherwise have
 *     std = 0, which the denoiser reads as "keep").
 * Outputs (the next state): color rgb (alpha untouched); moment2 rgb with n in its alpha;
 * normal = N, world_pos = X (the scaled inputs, alpha written as 0: the next step's history
 * guides and ready-made denoiser guides); albedo = A when both the input and the output are
 * given; color_std rgb (alpha untouched) if requested, in the layout lrt_denoise_device reads.
 *
 * cur_scale exists because lrt_render_desc.frame0 couples the seed to the lerp weight: a render
 * of samples frame0 .. frame0 + frames - 1 into ZEROED buffers with max_frame < 0 leaves
 * sum / (frame0 + frames); k = (frame0 + frames) / frames turns that into the plain mean of the
 * fresh samples. That is how a caller gets new seeds every time step without touching the render
 * kernels (a static camera re-rendering frame0 = 0 would accumulate identical frames).
 *
 * Limits: whole frames only. Static scene: the camera moves, the spheres do not (for spheres that
 * move between two frames there is lrt_temporal_accumulate_moving_* below, and
 * lrt_temporal_accumulate_gbuffer_* further down takes ids and motion vectors instead). First-hit
 * reprojection only: reflections and refractions lag. Like the denoiser it is not bit-pinned (the
 * reference has no such stage) but tolerance-checked against its NumPy restatement
 * (tests/temporal_ref.py); it is deterministic run to run. */
typedef struct lrt_temporal_desc {
    int32_t width, height;      /* a whole frame */
    int32_t flags;              /* 0 */
    int32_t min_history;        /* >= 1 */
    lrt_camera camera, prev_camera;
    float cur_scale;            /* finite, > 0 */
    float alpha_min;            /* in (0, 1] */
    float normal_min;           /* in [-1, 1] */
    float pos_tol, short_std;   /* finite, > 0 */
    int32_t reserved;           /* 0 */
} lrt_temporal_desc;

/* One accumulation state: five frames (albedo may be NULL). */
typedef struct lrt_temporal_state {
    float* color;
    float* moment2;   /* rgb: the running second moment; alpha: the history length n */
    float* normal;
    float* world_pos;
    float* albedo;
} lrt_temporal_state;

/* The defaults for a width x height frame and a camera pair: alpha_min 0.05, normal_min 0.9,
 * pos_tol 0.05, min_history 4, short_std 1e3, cur_scale 1. prev_camera == NULL: the camera. */
int lrt_temporal_default(int width, int height, const lrt_camera* camera, const lrt_camera* prev_camera,
                         lrt_temporal_desc* out);

/* One step on device buffers. d_color: the current frame's colour. d_cur: its normal and
 * world_pos (required) and albedo (optional); the other members are ignored. d_prev: the previous
 * state, or NULL for no history (everything is reset); if given, its color, moment2, normal and
 * world_pos are required. d_next: the state written; the same four are required, albedo is
 * optional. d_color_std may be NULL.
 *
 * No aliasing: the kernel gathers from d_prev at arbitrary pixels, so the step cannot run in place
 * and the caller ping-pongs two states. No d_next buffer and no d_color_std may overlap a d_prev
 * buffer, an input, or each other (LRT_E_INVALID).
 *
 * LRT_E_INVALID, before any device use: NULL required pointers; sizes < 1 or
 * width * height > INT_MAX / 4; flags or reserved != 0; min_history < 1; non-finite parameters;
 * cur_scale, pos_tol or short_std <= 0; alpha_min outside (0, 1]; normal_min outside [-1, 1]; a
 * prev_camera whose H'.H', V'.V' or fd is not finite and > 0. Asynchronous on `stream` and ordered
 * only against it, like lrt_render_device. Acts on the first device. */
int lrt_temporal_accumulate_device(const lrt_temporal_desc* desc, const float* d_color, const lrt_features* d_cur,
                                   const lrt_temporal_state* d_prev, const lrt_temporal_state* d_next,
                                   float* d_color_std, void* stream);

/* Same on HOST buffers: staged through device memory, blocking; every output equals
 * lrt_temporal_accumulate_device's bit for bit (the alphas of next->color and color_std are the
 * host buffers' own). */
int lrt_temporal_accumulate_host(const lrt_temporal_desc* desc, const float* color, const lrt_features* cur,
                                 const lrt_temporal_state* prev, const lrt_temporal_state* next,
                                 float* color_std);

/* The step under moving spheres. lrt_set_scene lets a caller move a sphere between two frames; the
 * step above then reprojects every pixel as if its surface point had stood still, and either
 * rejects the history of the moved sphere (a move of more than pos_tol x its distance: n stays 1
 * for as long as it moves) or blends in another point of it. This form is given the two scenes.
 * The scene is spheres only and a sphere moves rigidly (a translation and a uniform scale), so a
 * pixel's own guides identify its sphere; the render kernels are not involved.
 *
 * With the spheres (c_i, r_i) of the scene the current frame was rendered with and (c'_i, r'_i)
 * of the scene of the frame behind the previous state, steps 1-7 are those above, except:
 *  2a. Match (hit pixels only). n^ = N / |N|; for each sphere i,
 *      s_i = |X - (c_i + r_i n^)|^2: the squared distance from the pixel's mean hit point to the
 *      point of sphere i whose outward normal is n^ (two spheres in contact have opposite normals
 *      there, so the score separates them). Sphere i is a candidate iff r_i > 0 and r'_i > 0.
 *      i* is the candidate of the smallest s_i, the lowest index on a tie. The pixel is matched iff
 *      s_i* <= pos_tol^2 |X - O|^2 (the scale of the position test). A miss pixel is never matched;
 *      a hit pixel without a match (its samples straddle two spheres, or its guides are not of
 *      this scene) behaves exactly as in the static step.
 *  3a. Carry back. If the pixel is matched and sphere i*'s eight floats differ in any bit between
 *      the two arrays: Xc' = c'_i* + (r'_i* / r_i*) (Xc - c_i*). Otherwise Xc' = Xc, with no
 *      arithmetic applied. The target of step 4 is d = Xc' - O' for a hit.
 *  5a. The position test is |X'(Q) - Xc'|^2 <= pos_tol^2 |Xc - O|^2. The normal test is unchanged:
 *      a translation with a uniform scale keeps normals.
 * Under bit-identical cameras a pixel takes its own centre (as above) only if its Xc' = Xc; a
 * moved sphere always goes through the projection.
 * motion (optional, a whole frame of RGBA float quads, all four channels written):
 *      x = fx - x, y = fy - y   the previous position minus the current one, in pixels
 *      z = i* as a float, or -1 for an unmatched or a miss pixel
 *      w = 1 if step 4 found a projectable point, else 0 (then x = y = 0)
 * It says nothing about whether the taps counted: n says that. Without a previous state there is
 * nothing to reproject into: motion is (0, 0, -1, 0) everywhere.
 *
 * Limits: first-hit motion only. The shadow, the reflection and the refraction of a moving sphere
 * lag, as reflections already do. A moving emissive sphere changes the lighting everywhere, and the
 * history follows at alpha_min. Spheres do not rotate visibly (materials are uniform). Whole frames
 * only. */
typedef struct lrt_scene_motion {
    const lrt_sphere* spheres;       /* HOST: the scene the current frame was rendered with   */
    const lrt_sphere* prev_spheres;  /* HOST: the scene of the frame behind the previous state */
    int32_t count;                   /* 1..LRT_MAX_SPHERES, the same spheres in the same order */
    int32_t reserved;                /* 0 */
} lrt_scene_motion;

/* lrt_temporal_accumulate_device under moving spheres. Both sphere arrays are read from host
 * memory before the call returns (as lrt_set_scene reads its arrays). Up to 64 spheres travel in
 * the kernel's own arguments; more are uploaded on `stream` into that stream's scratch, with no
 * host round trip and no synchronisation (with sixteen uploads all still in flight, the call waits
 * for the oldest). Either way back-to-back calls with different scenes each use their own.
 * d_motion may be NULL.
 *
 * LRT_E_INVALID, before any device use: everything lrt_temporal_accumulate_device rejects; a NULL
 * `scene` or a NULL array in it; count outside 1..LRT_MAX_SPHERES; reserved != 0; a non-finite
 * float in either array; d_motion overlapping any other buffer (by address range). A sphere of
 * radius <= 0 in either array is no error: it is never matched. */
int lrt_temporal_accumulate_moving_device(const lrt_temporal_desc* desc, const lrt_scene_motion* scene,
                                          const float* d_color, const lrt_features* d_cur,
                                          const lrt_temporal_state* d_prev, const lrt_temporal_state* d_next,
                                          float* d_color_std, float* d_motion, void* stream);

/* Same on HOST buffers: staged through device memory, blocking; every output equals
 * lrt_temporal_accumulate_moving_device's bit for bit. */
int lrt_temporal_accumulate_moving_host(const lrt_temporal_desc* desc, const lrt_scene_motion* scene,
                                        const float* color, const lrt_features* cur, const lrt_temporal_state* prev,
                                        const lrt_temporal_state* next, float* color_std, float* motion);

/* ---- variance-guided filter over the temporal state ------------------------------ */

/* Stages 2 and 3 of SVGF (Schied et al. 2017) on the state lrt_temporal_accumulate_* leaves:
 * estimate each pixel's variance (from its temporal moments, or from its neighbourhood where
 * the history is short), divide the albedo out, and run `iterations` a-trous passes whose
 * colour weight follows the variance, which is itself pre-filtered and propagated from pass to
 * pass. All buffers are whole frames: `height` rows of `width` RGBA float quads. f32 throughout.
 *
 * Stage 0, per pixel p, with C = color.rgb, M = moment2.rgb, n = moment2.a:
 *     hit = |N|^2 >= 0.25 if normal is given, else true
 *     D   = max(A, albedo_floor) per channel if albedo is given and hit, else 1
 *     v   = max(M - C^2, 0)                                        if n >= min_history
 *         = max(m2 - m1^2, 0) * (min_history / max(n, 1))           otherwise, with
 *           m1 = sum_q g C(q) / sum_q g, m2 = sum_q g M(q) / sum_q g over the 7x7 window
 *           q = p + (i, j), i, j in -3..3 (taps outside the image are skipped),
 *           g(p,q) = exp(-(|n(p) - n(q)|^2 / sigma_normal^2 + |x(p) - x(q)|^2 / sigma_pos^2))
 *           (a term is dropped if its guide is absent)
 *     c_0 = C / D, var_0 = v / D^2
 * Passes k = 0 .. iterations - 1, with the 5x5 B3-spline taps q = p + 2^k (i, j), i, j in -2..2,
 * h = [1/16, 1/4, 3/8, 1/4, 1/16], as in lrt_denoise_*; taps outside the image are skipped:
 *     vt(p) = sum_{|i|,|j| <= 1} b_i b_j var_k(p + (i, j)) / sum b_i b_j,  b = [1/4, 1/2, 1/4]
 *             (undilated at every pass; only the taps inside the image count)
 *     E(p,q) = |c_k(p) - c_k(q)|^2 / (sigma_color^2 (vt.r + vt.g + vt.b) + 1e-6)
 *            + |n(p) - n(q)|^2 / sigma_normal^2 + |x(p) - x(q)|^2 / sigma_pos^2
 *     w = h[i] h[j] exp(-E)
 *     c_{k+1}(p) = sum_q w c_k(q) / sum_q w,  var_{k+1}(p) = sum_q w^2 var_k(q) / (sum_q w)^2
 * There is no albedo term (albedo is divided out instead) and sigma_color is the same at every
 * pass (the variance shrinks by itself). End: out.rgb = c_K D, variance_out.rgb = var_K D^2.
 * The only decisions are n < min_history and hit, both on input values. Deterministic run to
 * run; tolerance-checked against its NumPy restatement (tests/svgf_ref.py), not bit-pinned. */
#define LRT_SVGF_MAX_ITER 5
typedef struct lrt_svgf_desc {
    int32_t width, height;     /* a whole frame */
    int32_t iterations;        /* 1..LRT_SVGF_MAX_ITER */
    int32_t flags;             /* 0 */
    int32_t min_history;       /* >= 1 */
    int32_t reserved;          /* 0 */
    float sigma_color, sigma_normal, sigma_pos;   /* finite, > 0 */
    float albedo_floor;        /* finite, > 0 */
} lrt_svgf_desc;

/* The defaults for a width x height frame: 5 iterations, min_history 4, sigma_color 4,
 * sigma_normal 0.3, sigma_pos 0.5, albedo_floor 0.01. */
int lrt_svgf_default(int width, int height, lrt_svgf_desc* out);

/* Filter the state's d_color / d_moment2 (the color and moment2 members of an
 * lrt_temporal_state; moment2's alpha is n) into d_out (device buffers). Of d_guides, normal,
 * world_pos and albedo are read; each may be NULL, and d_guides may be NULL; the other members
 * are ignored. d_variance_out may be NULL. Only the rgb of d_out and d_variance_out is written,
 * their alphas stay. d_out may be d_color (in place); otherwise neither output may overlap an
 * input or the other output (address ranges; LRT_E_INVALID).
 *
 * LRT_E_INVALID, before any device use: NULL desc, color, moment2 or out; sizes < 1 or
 * width * height > INT_MAX / 4; iterations outside 1..LRT_SVGF_MAX_ITER; flags or reserved != 0;
 * min_history < 1; a sigma or albedo_floor that is not finite and > 0; aliasing. Then
 * LRT_E_STATE without lrt_initialize(). Asynchronous on `stream` and ordered only against it;
 * the intermediate frames live in that stream's scratch of the library. Acts on the first
 * device. */
int lrt_svgf_filter_device(const lrt_svgf_desc* desc, const float* d_color, const float* d_moment2,
                           const lrt_features* d_guides, float* d_out, float* d_variance_out, void* stream);

/* Same on HOST buffers: staged through device memory, blocking; the outputs equal
 * lrt_svgf_filter_device's bit for bit. */
int lrt_svgf_filter_host(const lrt_svgf_desc* desc, const float* color, const float* moment2,
                         const lrt_features* guides, float* out, float* variance_out);

/* ---- auto-exposure metering and tone mapping ------------------------------------- */

/* The stage between the filters and the screen: meter the frame's exposure from the frame
 * itself, adapt it over time, apply a tone curve, and quantise as lrt_present_bgra8 does. The
 * frame is `height` rows of `width` RGBA float quads; alphas are never read.
 *
 * Metering (auto_exposure = 1). Per pixel, in f32, Y = 0.2126 R + 0.7152 G + 0.0722 B of the
 * rgb as read. Its bin comes from the bits of Y, with no logarithm:
 *     2^-16 <= Y < 2^16:        bin (bits(Y) >> 20) - 888: eight bins per octave, 256 bins
 *     Y >= 2^16, +Inf included: `over`
 *     everything else (zero, negative, NaN, below 2^-16): `under`
 * The histogram is LRT_TONEMAP_HIST_WORDS counts h: the 256 bins, then `under`, then `over`
 * (they sum to width * height). Bin b stands for the log2 luminance
 *     l_b = (b >> 3) - 16 + log2(1 + ((b & 7) + 0.5) / 8)
 * With N = the sum of the 256 bins and c_b their exclusive prefix sum, the percentile window
 * takes m_b = max(0, min(c_b + h_b, p_high N) - max(c_b, p_low N)) from bin b (a firefly is a
 * few pixels at the top of the histogram: p_high < 1 leaves them out, whatever their value), and
 *     mean   = sum_b m_b l_b / sum_b m_b
 *     target = clamp(log2(key) - mean + ev_bias, ev_min, ev_max)
 * The state (read and written by the call; zero-filled = no history), with N > 0:
 *     log2_exposure  = prev.frames >= 1 ? prev.log2_exposure + adapt (target - prev.log2_exposure)
 *                                       : target           (adaptation is linear in log space)
 *     log2_luminance = mean, counted = N / (width height), frames = prev.frames + 1
 * and with N = 0: log2_exposure stays if prev.frames >= 1, else it is clamp(ev_bias, ev_min,
 * ev_max); log2_luminance stays; counted = 0; frames = prev.frames + 1.
 *
 * Mapping. e = exp2(log2_exposure) of the state just written; with auto_exposure = 0 it is
 * exp2(ev_bias), unclamped, and the state and the histogram are neither read nor written. Per
 * channel c = x e, then c = c > 0 ? min(c, LRT_TM_MAX) : 0 (a NaN becomes 0), then
 *     LRT_TM_LINEAR:   t = c
 *     LRT_TM_REINHARD: t = c (1 + c / white^2) / (1 + c)          (white maps to 1)
 *     LRT_TM_ACES:     t = clamp(c (2.51 c + 0.03) / (c (2.43 c + 0.59) + 0.14), 0, 1)
 *                      (Narkowicz's fit of the ACES filmic curve)
 * out.rgb = t (linear; its alpha stays); bgra = lrt_present_bgra8's quantiser applied to t.
 *
 * The metering is exact integer counting (deterministic); the state and the mapped frame are
 * tolerance-checked against the NumPy restatement (tests/tonemap_ref.py), the quantiser of bgra
 * is lrt_present_bgra8's bit for bit. */
#define LRT_TONEMAP_BINS 256
#define LRT_TONEMAP_HIST_WORDS 258          /* 256 bins, then `under`, then `over` */
#define LRT_TM_LINEAR 0
#define LRT_TM_REINHARD 1
#define LRT_TM_ACES 2
#define LRT_TM_MAX 65504.0f

typedef struct lrt_tonemap_desc {
    int32_t width, height;       /* a whole frame of RGBA float quads */
    int32_t op;                  /* LRT_TM_* */
    int32_t auto_exposure;       /* 0: log2 exposure = ev_bias; 1: metered */
    int32_t flags, reserved;     /* 0 */
    float key;                   /* > 0 */
    float p_low, p_high;         /* 0 <= p_low < p_high <= 1 */
    float ev_bias;               /* finite */
    float ev_min, ev_max;        /* finite, ev_min <= ev_max */
    float adapt;                 /* in (0, 1] */
    float white;                 /* > 0 (Reinhard's white point) */
} lrt_tonemap_desc;

typedef struct lrt_exposure_state { float log2_exposure, log2_luminance, counted, frames; } lrt_exposure_state;

/* The defaults for a width x height frame: ACES, auto_exposure 1, key 0.18, p_low 0.1,
 * p_high 0.9, ev_bias 0, ev_min -8, ev_max 8, adapt 1, white 4. They are choices (the usual
 * middle grey, a window that drops a tenth of the pixels at each end, no smoothing), not values
 * tuned on this renderer's frames. */
int lrt_tonemap_default(int width, int height, lrt_tonemap_desc* out);

/* Meter and map d_color (device buffers). d_state: the exposure state, required with
 * auto_exposure = 1. d_histogram: if given, receives the LRT_TONEMAP_HIST_WORDS counts (with
 * auto_exposure = 1). d_out: if given, receives t in its rgb (12 B per pixel; its alpha stays);
 * it may be d_color (in place). d_bgra: if given, receives the quantised pixels, width * height
 * words. Both may be NULL with auto_exposure = 1: a meter-only call. With auto_exposure = 0,
 * d_state and d_histogram may be NULL and are left untouched if given.
 *
 * LRT_E_INVALID, before any device use: NULL desc or color; sizes < 1 or width * height >
 * INT_MAX / 4; an unknown op; auto_exposure outside 0..1; flags or reserved != 0; a parameter
 * outside the range in the struct's comments, or not finite; auto_exposure = 1 without d_state;
 * no output and no metering; d_bgra, d_histogram or d_state overlapping any other buffer (address
 * ranges); d_out overlapping d_color other than being equal to it. Then LRT_E_STATE without
 * lrt_initialize(). Asynchronous on `stream` and ordered only against it, with no host round
 * trip (the exposure goes from the metering to the mapping through device memory); the
 * intermediates live in that stream's scratch of the library. Acts on the first device. */
int lrt_tonemap_device(const lrt_tonemap_desc* desc, const float* d_color, lrt_exposure_state* d_state,
                       uint32_t* d_histogram, float* d_out, uint32_t* d_bgra, void* stream);

/* Same on HOST buffers: staged through device memory, blocking; every output equals
 * lrt_tonemap_device's bit for bit. */
int lrt_tonemap_host(const lrt_tonemap_desc* desc, const float* color, lrt_exposure_state* state,
                     uint32_t* histogram, float* out, uint32_t* bgra);

/* ---- G-buffer: pixel-centre first-hit guides, ids, depth and motion --------------- */

/* The guides of the post-process chain from a pass of their own, as every real-time SVGF pipeline
 * takes them: one primary ray per pixel through the pixel CENTRE, with no lens and no RNG, against
 * the scene the library holds. lrt_features (the v0 kernel's side output) are means over jittered
 * lens samples; these are the values of one exact point per pixel, they come with the sphere's id
 * and the depth, and any render kernel (LRT_F_POOL, LRT_F_WAVEFRONT) can supply the colour. f32
 * throughout, no contraction. Whole frames: `height` rows of `width` pixels, row 0 at the bottom.
 *
 * Per pixel (x, y), with the camera O, L, H, V (origin, lowerLeftCorner, horizontalVec,
 * verticalVec; lensRadius, u and r are not read):
 *  1. s = ((float)x + 0.5f) * (1.0f / (float)width), t likewise with height (the reciprocals are
 *     taken once, on the host); D = ((L + s H) + t V) - O, in that order: GetRay's expression
 *     (maths.h:205-215) with a zero lens offset. The ray is Ray(O, D): one normalize.
 *  2. The closest hit over (kMinT, kMaxT) = (0.001, 1e7), HitWorld's bits: (id, t).
 *  3. Hit: P = O + dir t, n = normalize(P - c_id), albedo = the material's. Miss: the three guides
 *     are 0, id = -1, depth = +Inf.
 *  4. Motion (if requested): steps 3a and 4 of lrt_temporal_* on the exact point. The target is
 *     d = Xc' - O' for a hit, d = D for a miss; Xc' = P, unless `scene` is given and sphere id's
 *     eight floats differ in a bit between scene->spheres and scene->prev_spheres: then
 *     Xc' = c' + (r' / r) (P - c). Into the previous camera as step 4 does: da = d.a',
 *     fd = -(L' - O').a', q = (-fd / da) d - (L' - O'), fx = (q.H') (1 / H'.H') w - 1/2,
 *     fy = (q.V') (1 / V'.V') h - 1/2; projectable iff da < 0 and |fx|, |fy| < 1e6 (a NaN fails).
 *     A hit sphere with r' <= 0 (or r <= 0) did not exist in the previous frame: not projectable.
 *     Under bit-identical cameras (origin, a, lowerLeftCorner, horizontalVec, verticalVec) a miss
 *     and a hit on a sphere that did not move take their own centre, fx = x, fy = y, with no
 *     arithmetic: the temporal step's own rule.
 * Outputs (each optional): normal, world_pos, albedo = guide_scale * (n, P, albedo) in rgb, alpha
 * written 0; id; depth = t; motion = (fx - x, fy - y, (float)id, 1) if projectable, else
 * (0, 0, (float)id, 0): the layout of lrt_temporal_accumulate_moving_*'s motion.
 *
 * guide_scale exists because lrt_temporal_desc.cur_scale = k multiplies colour and guides alike: a
 * caller who renders fresh seeds (frame0 > 0) into zeroed buffers needs
 * k = (frame0 + frames) / frames for the colour, passes guide_scale = 1 / k here, and the temporal
 * step then sees these guides at scale 1, within rounding. id and depth are never scaled.
 *
 * id and depth are pinned bit for bit to the library's closest hit (lrt_accel_eval, lrt_diag.h);
 * the guides and the motion are tolerance-checked against the NumPy restatement
 * (tests/gbuffer_ref.py). Limits: whole frames, the first device, spheres only, first hits only
 * (no lens, no jitter: an edge pixel is one surface or the other, never a mixture;
 * lrt_gbuffer_chain_* further down follows the path through mirrors and glass). */
typedef struct lrt_gbuffer_desc {
    int32_t width, height;          /* a whole frame */
    int32_t flags, reserved;        /* 0 */
    lrt_camera camera, prev_camera; /* prev_camera is read only when motion is requested */
    float guide_scale;              /* finite, > 0; default 1 */
    int32_t reserved2;              /* 0 */
} lrt_gbuffer_desc;

typedef struct lrt_gbuffer {        /* every member optional, at least one non-NULL */
    float* normal;     /* RGBA quads: rgb = guide_scale * n, alpha written 0 */
    float* world_pos;  /* RGBA quads: rgb = guide_scale * P, alpha written 0 */
    float* albedo;     /* RGBA quads: rgb = guide_scale * material albedo, alpha written 0 */
    float* motion;     /* RGBA quads, all four written (layout of lrt_temporal's motion) */
    int32_t* id;       /* width*height: sphere index, -1 on a miss */
    float* depth;      /* width*height: t along the unit ray; +Inf on a miss */
} lrt_gbuffer;

/* The defaults for a width x height frame and a camera pair: guide_scale 1. prev_camera == NULL:
 * the camera. */
int lrt_gbuffer_default(int width, int height, const lrt_camera* camera,
                        const lrt_camera* prev_camera, lrt_gbuffer_desc* out);

/* The pass into device buffers. `scene` may be NULL (nothing moved); if given, scene->spheres must
 * be the scene the library holds (what lrt_get_scene returns, bit for bit) and both arrays are read
 * from host memory before the call returns: up to 64 spheres travel in the kernel's own arguments,
 * more are uploaded on `stream` into that stream's scratch, as in
 * lrt_temporal_accumulate_moving_device. Only the planes given are written, and nothing else is
 * paid for. Scenes of up to 16 spheres are scanned, larger ones go through the uniform grid (built
 * on first use, as a render would).
 *
 * LRT_E_INVALID, before any device use: NULL desc or d_out, or all six planes NULL; sizes < 1 or
 * width * height > INT_MAX / 4; flags, reserved or reserved2 != 0; guide_scale not finite or <= 0;
 * any two planes overlapping (address ranges); with motion, a prev_camera that lrt_temporal_*
 * rejects; with `scene`, a NULL array, count outside 1..LRT_MAX_SPHERES, reserved != 0, a
 * non-finite float, a count other than the current scene's, or spheres that are not the current
 * scene's bit for bit (an uninitialised library holds no scene: any `scene` is refused). Then
 * LRT_E_STATE without lrt_initialize(). Asynchronous on `stream` and ordered only against it; it
 * sees the scene as an lrt_render_device call made at the same moment would. Acts on the first
 * device. */
int lrt_gbuffer_device(const lrt_gbuffer_desc* desc, const lrt_scene_motion* scene,
                       const lrt_gbuffer* d_out, void* stream);

/* Same into HOST buffers: staged through device memory, blocking; every output equals
 * lrt_gbuffer_device's bit for bit. */
int lrt_gbuffer_host(const lrt_gbuffer_desc* desc, const lrt_scene_motion* scene, const lrt_gbuffer* out);

/* ---- temporal accumulation driven by the G-buffer's ids and motion vectors -------- */

/* lrt_temporal_accumulate_* as every real-time SVGF pipeline has it: the step takes the motion
 * vectors and the ids that lrt_gbuffer_* wrote, and needs no cameras, no scenes and no loop over
 * the spheres (its cost does not depend on their count). The state it keeps is color and moment2
 * only: the previous frame's normal and id are read from the previous G-buffer's own planes.
 *
 * Per pixel (x, y), with C = cur_scale color.rgb, N = normal.rgb as read, i = id and
 * (mx, my, ., mw) = motion of the current G-buffer, N', i' of the previous one:
 *  1. fx = x + mx, fy = y + my; ok = mw != 0 and |fx|, |fy| < 1e6 (a NaN fails). A zero motion
 *     gives fx = x with no rounding: what lrt_gbuffer_* guarantees under a static camera carries
 *     through, and a static accumulation never bleeds its neighbours in.
 *  2. The four bilinear taps Q of step 5 of lrt_temporal_*. A tap counts iff it lies inside the
 *     image and i'(Q) = i; for a hit (i >= 0) it also needs N'(Q).N >= normal_min. A miss matches
 *     a miss (-1 = -1). No id is ever used as an index.
 *  3. Steps 6 and 7 of lrt_temporal_*, unchanged.
 * Outputs: next->color rgb (alpha untouched), next->moment2 (rgb and n), color_std rgb (alpha
 * untouched) if requested. Nothing else is written.
 *
 * cur_scale multiplies the COLOUR only: the planes must be those of an lrt_gbuffer_* call with
 * guide_scale 1 (unit normals).
 *
 * Limits: first-hit motion only (shadows, reflections and refractions lag). The test is id plus
 * normal: a point that was behind its own sphere's silhouette in the previous frame is rejected
 * by the normal test only. Spheres only, whole frames only, the first device. Guides must be at
 * scale 1. Tolerance-checked against its NumPy restatement (tests/temporal_gbuffer_ref.py);
 * deterministic run to run. */
typedef struct lrt_temporal_gbuffer_desc {
    int32_t width, height;      /* a whole frame */
    int32_t flags;              /* 0 */
    int32_t min_history;        /* >= 1 */
    float cur_scale;            /* finite, > 0: multiplies the COLOUR only */
    float alpha_min;            /* in (0, 1] */
    float normal_min;           /* in [-1, 1] */
    float short_std;            /* finite, > 0 */
    int32_t reserved, reserved2;/* 0 */
} lrt_temporal_gbuffer_desc;

/* The defaults for a width x height frame, lrt_temporal_default's: alpha_min 0.05, normal_min 0.9,
 * min_history 4, short_std 1e3, cur_scale 1. */
int lrt_temporal_gbuffer_default(int width, int height, lrt_temporal_gbuffer_desc* out);

/* One step on device buffers. d_color: the current frame's colour. d_cur: the current G-buffer;
 * normal, motion and id are required, the other members are ignored. d_prev_g: the previous
 * frame's G-buffer; normal and id are required. d_prev / d_next: the previous state and the one
 * written; of either only color and moment2 are required, read or written, and the other three
 * members are never touched. d_prev and d_prev_g are both NULL (no history: every pixel is reset)
 * or both given. d_color_std may be NULL.
 *
 * LRT_E_INVALID, before any device use: NULL required pointers; exactly one of d_prev and
 * d_prev_g; sizes < 1 or width * height > INT_MAX / 4; flags, reserved or reserved2 != 0;
 * min_history < 1; non-finite parameters; cur_scale or short_std <= 0; alpha_min outside (0, 1];
 * normal_min outside [-1, 1]; d_next->color, d_next->moment2 or d_color_std overlapping an input,
 * a previous buffer or each other (by address range: the id planes are width * height * 4 bytes,
 * the others 16 bytes per pixel); d_cur->normal or d_cur->id overlapping d_prev_g's (a G-buffer
 * overwritten in place is no history: ping-pong two). Then LRT_E_STATE without lrt_initialize().
 * Asynchronous on `stream` and ordered only against it, with no host round trip. Acts on the
 * first device. */
int lrt_temporal_accumulate_gbuffer_device(const lrt_temporal_gbuffer_desc* desc, const float* d_color,
                                           const lrt_gbuffer* d_cur, const lrt_gbuffer* d_prev_g,
                                           const lrt_temporal_state* d_prev, const lrt_temporal_state* d_next,
                                           float* d_color_std, void* stream);

/* Same on HOST buffers: staged through device memory, blocking; every output equals
 * lrt_temporal_accumulate_gbuffer_device's bit for bit (the alphas of next->color and color_std
 * are the host buffers' own). */
int lrt_temporal_accumulate_gbuffer_host(const lrt_temporal_gbuffer_desc* desc, const float* color,
                                         const lrt_gbuffer* cur, const lrt_gbuffer* prev_g,
                                         const lrt_temporal_state* prev, const lrt_temporal_state* next,
                                         float* color_std);

/* ---- G-buffer-guided upsampling of a low-resolution frame ------------------------- */

/* Trace and filter at a fraction of the resolution, then reconstruct the full frame with the
 * full-resolution G-buffer as guide: the G-buffer of lrt_gbuffer_* does not depend on who renders
 * the colour or at what size, and gives exact pixel-centre ids and normals per pixel. f32, not
 * bit-pinned (contraction allowed).
 *
 * Inputs. color_low: low_height rows of low_width RGBA quads (svgf_filter's output, say). low: the
 * G-buffer of the low frame, high: the G-buffer of the output frame (width x height); of either,
 * id and normal are required and albedo is optional, in both or in neither; the other members are
 * ignored. Both come from the same camera at guide_scale 1 (unit normals).
 * 1 <= low_width <= width <= 32768 and likewise the heights; the ratio need not be an integer and
 * need not be the same on both axes.
 *
 * Per output pixel p = (x, y):
 *  1. The taps. The position of p's centre in the low frame is found with integers, so that no
 *     decision about which taps are used depends on rounding: a = (2x + 1) low_width - width (no
 *     overflow of 32 bits under the size limit), X0 = floor(a / (2 width)), r = a - X0 2 width,
 *     tx = (float)r / (float)(2 width), one IEEE division; Y0 and ty likewise. The four taps are
 *     Q = (X0 + i, Y0 + j), i, j in {0, 1}, with the bilinear weight
 *     b = (i ? tx : 1 - tx)(j ? ty : 1 - ty). A tap outside the low frame is skipped.
 *  2. Class 0. A tap counts iff it is inside the frame and id_low(Q) = id_high(p); a miss matches
 *     a miss (-1 = -1), and no id is ever used as an index. Its weight is w = b g, with
 *     g = exp(-|N_low(Q) - N_high(p)|^2 / sigma_normal^2) for a hit and g = 1 for a miss.
 *     sw = sum w. If sw >= weight_min: I = sum w c(Q) / sw.
 *  3. Class 1, when sw < weight_min: a surface the four taps do not show is sought one ring
 *     further out. Taps Q = (X0 - 1 + i, Y0 - 1 + j), i, j in 0..3,
 *     w = k(i - 1 - tx) k(j - 1 - ty) g with k(d) = max(0, 1 - |d| / 2); the id rule and g as in
 *     step 2. If that sum >= weight_min: I = sum w c(Q) / sum w.
 *  4. Class 2, otherwise: plain bilinear, I = sum b c(Q) / sum b over the inside taps of step 1,
 *     whatever their ids. At least one tap is inside, with b >= 1/4.
 *  5. Albedo. With albedo planes, c(Q) = color_low(Q).rgb / max(A_low(Q), albedo_floor) per
 *     channel where id_low(Q) >= 0, else color_low(Q).rgb; out = I max(A_high(p), albedo_floor)
 *     where id_high(p) >= 0, else out = I. This is lrt_svgf's D: a silhouette pixel that falls to
 *     class 2 still gets its own surface's albedo. Without albedo planes c = color_low.rgb and
 *     out = I.
 *  6. out.rgb is written, its alpha is left untouched. class_out (optional): width * height
 *     int32 holding 0, 1 or 2. Flag LRT_UP_BILINEAR makes every pixel class 2: the baseline a
 *     caller has without this stage. With it set the normals are not read and may be NULL.
 * A tap that is skipped, does not count, or has weight 0 adds nothing to a sum, whatever its colour
 * holds: a non-finite colour reaches only the pixels that give its tap a weight > 0.
 *
 * Limits: spheres only, first-hit guides only (reflections and refractions are upsampled with the
 * mirror's own guides), whole frames, the first device. The normals are not anti-aliased at the
 * output resolution: an edge pixel is one surface or the other. Tolerance-checked against its
 * NumPy restatement (tests/upsample_ref.py); deterministic run to run. */
#define LRT_UP_BILINEAR 1

typedef struct lrt_upsample_desc {
    int32_t width, height, low_width, low_height;
    int32_t flags, reserved;                        /* LRT_UP_BILINEAR | 0 ; 0 */
    float sigma_normal, albedo_floor, weight_min;   /* finite, > 0 */
    int32_t reserved2;                              /* 0 */
} lrt_upsample_desc;

/* The defaults for a width x height frame from a low_width x low_height one: sigma_normal 0.3 and
 * albedo_floor 0.01 (lrt_svgf's), weight_min 1e-3 (the temporal step's threshold on its sum of
 * weights), flags 0. Choices taken from the neighbouring stages, not values tuned here. */
int lrt_upsample_default(int width, int height, int low_width, int low_height, lrt_upsample_desc* out);

/* The pass on device buffers. d_class may be NULL.
 *
 * LRT_E_INVALID, before any device use: NULL desc, d_color_low, d_low, d_high or d_out; a NULL id,
 * or (without LRT_UP_BILINEAR) a NULL normal, in either G-buffer; sizes < 1, width or height >
 * 32768, low_width > width, low_height > height, or width * height > INT_MAX / 4; an unknown flag
 * bit; reserved or reserved2 != 0; sigma_normal, albedo_floor or weight_min not finite or <= 0;
 * albedo in exactly one G-buffer; d_out or d_class overlapping an input or each other (by address
 * range: the id planes and d_class are 4 bytes per pixel, the others 16, each sized by its own
 * frame's dimensions). Then LRT_E_STATE without lrt_initialize(). Asynchronous on `stream` and
 * ordered only against it, with no host round trip. Acts on the first device. */
int lrt_upsample_device(const lrt_upsample_desc* desc, const float* d_color_low, const lrt_gbuffer* d_low,
                        const lrt_gbuffer* d_high, float* d_out, int32_t* d_class, void* stream);

/* Same on HOST buffers: staged through device memory, blocking; every output equals
 * lrt_upsample_device's bit for bit (the alpha of out is the host buffer's own). */
int lrt_upsample_host(const lrt_upsample_desc* desc, const float* color_low, const lrt_gbuffer* low,
                      const lrt_gbuffer* high, float* out, int32_t* class_out);

/* ---- temporal upsampling: a full-resolution history from jittered low frames ------- */

/* lrt_upsample_* cannot bring back what the low frame never sampled: a sphere smaller than a low
 * pixel is simply not in it. This stage closes the gap the way TAAU and FSR 2 do: the low camera is
 * shifted by a different sub-pixel offset each frame (lrt_camera_jitter), and the shifted frames are
 * accumulated into a history kept at the OUTPUT resolution. Per output pixel it does what
 * lrt_temporal_accumulate_gbuffer_* and lrt_upsample_* each do half of. f32, not bit-pinned
 * (contraction allowed).
 *
 * The intended chain: render at the low size under the jittered camera; lrt_gbuffer_* at the low
 * size (id, normal) under the same jittered camera; lrt_gbuffer_* at the output size (id, normal,
 * motion) under the UNJITTERED camera, so that a static camera still gives zero motion and the
 * history is never resampled; this step; lrt_svgf_* at the output size on the state it leaves.
 *
 * The jitter (jitter_x, jitter_y) is the low camera's shift in units of 1 / (2 width) resp.
 * 1 / (2 height) of a LOW pixel: low pixel X of a frame under lrt_camera_jitter's camera has its
 * centre at the continuous low coordinate X + 1/2 + jitter_x / (2 width).
 *
 * Per output pixel p = (x, y):
 *  1. Low taps, in integers. a = (2x + 1) low_width - width - jitter_x, X0 = floor(a / (2 width))
 *     (a true floor: a >= -2 width + 1, so X0 >= -1), r = a - X0 2 width,
 *     tx = (float)r / (float)(2 width); Y0 and ty likewise. Everything fits 32 bits under the size
 *     limit (the largest product is 65535 x 32768). The four taps are Q = (X0 + i, Y0 + j) with the
 *     bilinear weight b of lrt_upsample step 1. Which taps are used never depends on rounding.
 *  2. Current estimate. A tap counts iff it is inside the low frame, b > 0 and
 *     id_low(Q) = id_cur(p); a miss matches a miss (-1 = -1), and no id is ever used as an index.
 *     w = b g, with g = exp(-|N_low(Q) - N_cur(p)|^2 / sigma_normal^2) for a hit and g = 1 for a
 *     miss. sw = sum w. The current frame SPEAKS for p iff sw >= weight_min; then
 *     I = cur_scale sum w color_low(Q).rgb / sw, and its confidence is beta = sum w k(Q) / sw with
 *     k(Q) = exp(-(dx^2 + dy^2) / (2 sigma_sample^2)), dx = (i - tx) width / low_width,
 *     dy = (j - ty) height / low_height: the distance from p's centre to the tap's sample in OUTPUT
 *     pixels. beta = 1 where a low sample sits on p's centre and falls off as the nearest sample of
 *     p's surface recedes. A tap that is skipped, does not count or has weight 0 is kept out of
 *     every sum by a select, not by a product with 0: a non-finite colour reaches only the pixels
 *     that count its tap.
 *  3. History. Steps 1 and 2 of lrt_temporal_accumulate_gbuffer_*, word for word, on the
 *     full-size planes: d_cur supplies motion, id and normal, d_prev_g normal and id, d_prev color
 *     and moment2. The history COUNTS iff its sum of weights exceeds 1e-3; then h = sum b c' / sum b,
 *     m = sum b m2' / sum b per channel and n_h = sum b n' / sum b. As in that step, a tap that is
 *     outside or refused gets the weight 0 and stays in the sums as a product: the select of step 2
 *     is step 2's alone, and a non-finite value in d_prev reaches every pixel that gathers it.
 *  4. Blend; the class is what class_out receives.
 *     class 0, history and current: n = n_h + beta, alpha = max(beta / n, alpha_min beta),
 *       color = (1 - alpha) h + alpha I, moment2 = (1 - alpha) m + alpha I^2. With beta = 1 this
 *       is step 6 of lrt_temporal_* exactly. The maximum is fmaxf, which ignores a NaN: where beta
 *       underflows to 0 over n_h = 0 (a sigma_sample far below the spacing of the samples, a history
 *       of class-3 pixels), beta / n is 0 / 0, alpha is 0 and the history stays.
 *     class 1, history only: color = h, moment2 = m, n = n_h. The pixel waits for a phase of the
 *       jitter that samples its surface.
 *     class 2, current only: color = I, moment2 = I^2, n = beta.
 *     class 3, neither: color = cur_scale x the plain bilinear mean over the inside taps of step 1
 *       with b > 0, whatever their ids (class 2 of lrt_upsample); moment2 its square, n = 0.
 *  5. Step 7 of lrt_temporal_*, unchanged: color_std, or short_std where n < min_history (n may
 *     now be fractional).
 * Outputs: next->color rgb (alpha untouched), next->moment2 (rgb and n), color_std rgb (alpha
 * untouched) if given, class_out (int32, width * height) if given. Nothing else is written.
 *
 * Limits: first-hit motion only. Under a moving camera the history is resampled bilinearly every
 * step and softens, as in any TAA. moment2 takes the square of an INTERPOLATED current colour where
 * no sample sits on the pixel, so the variance there is underestimated; lrt_svgf's spatial estimate
 * covers short histories. No albedo demodulation: the id test already keeps the taps on the pixel's
 * own sphere, and one sphere has one albedo. Spheres only, whole frames, the first device; all
 * planes at guide_scale 1. Tolerance-checked against its NumPy restatement
 * (tests/temporal_upsample_ref.py); deterministic run to run. */
typedef struct lrt_temporal_upsample_desc {
    int32_t width, height, low_width, low_height;   /* the limits of lrt_upsample_desc */
    int32_t jitter_x, jitter_y;   /* the low camera's shift, in units of 1/(2 width) resp. 1/(2 height) of a LOW
                                     pixel; |jitter_x| <= width, |jitter_y| <= height (half a low pixel) */
    int32_t flags;                /* 0 */
    int32_t min_history;          /* >= 1 */
    float cur_scale;              /* finite, > 0: multiplies the COLOUR only */
    float alpha_min;              /* in (0, 1] */
    float normal_min;             /* in [-1, 1] */
    float short_std;              /* finite, > 0 */
    float sigma_normal, sigma_sample, weight_min;   /* finite, > 0 */
    int32_t reserved;             /* 0 */
} lrt_temporal_upsample_desc;

/* The defaults: alpha_min 0.05, normal_min 0.9, min_history 4, short_std 1e3 and cur_scale 1
 * (lrt_temporal_gbuffer_default's); sigma_normal 0.3 and weight_min 1e-3 (lrt_upsample_default's);
 * sigma_sample 0.5 output pixels; jitter 0. Choices taken from the neighbouring stages, not values
 * tuned here. */
int lrt_temporal_upsample_default(int width, int height, int low_width, int low_height, lrt_temporal_upsample_desc* out);

/* *out = *camera with lowerLeftCorner += (dx / low_width) horizontalVec + (dy / low_height)
 * verticalVec, dx = jitter_x / (2 width) and dy = jitter_y / (2 height) in f32; every other member
 * is unchanged. Touches no device and needs no lrt_initialize. LRT_E_INVALID on NULLs, sizes < 1 or
 * > 32768, low > output, |jitter_x| > width or |jitter_y| > height. */
int lrt_camera_jitter(const lrt_camera* camera, int width, int height, int low_width, int low_height,
                      int jitter_x, int jitter_y, lrt_camera* out);

/* One step on device buffers. d_color_low: the low frame's colour. d_low: its G-buffer under the
 * JITTERED camera; id and normal are required. d_cur: the output frame's G-buffer under the
 * unjittered camera; id, normal and motion are required. d_prev_g (normal, id), d_prev and d_next
 * (color, moment2) as in lrt_temporal_accumulate_gbuffer_device: d_prev and d_prev_g are both NULL
 * (no history: classes 2 and 3 only) or both given. d_color_std and d_class may be NULL.
 *
 * LRT_E_INVALID, before any device use: whatever lrt_temporal_accumulate_gbuffer_device and
 * lrt_upsample_device refuse about the arguments they share (NULL required pointers; sizes < 1,
 * width or height > 32768, low_width > width, low_height > height, width * height > INT_MAX / 4;
 * flags or reserved != 0; min_history < 1; non-finite parameters; cur_scale, short_std,
 * sigma_normal, sigma_sample or weight_min <= 0; alpha_min outside (0, 1]; normal_min outside
 * [-1, 1]; exactly one of d_prev and d_prev_g); |jitter_x| > width or |jitter_y| > height;
 * d_next->color, d_next->moment2, d_color_std or d_class overlapping an input, a previous buffer
 * or each other (by address range: id planes and d_class are 4 bytes per pixel, the others 16,
 * each sized by its own frame); d_cur->normal or d_cur->id overlapping d_prev_g's. Then LRT_E_STATE
 * without lrt_initialize(). Asynchronous on `stream` and ordered only against it, with no host
 * round trip. Acts on the first device. */
int lrt_temporal_upsample_device(const lrt_temporal_upsample_desc* desc, const float* d_color_low,
                                 const lrt_gbuffer* d_low, const lrt_gbuffer* d_cur, const lrt_gbuffer* d_prev_g,
                                 const lrt_temporal_state* d_prev, const lrt_temporal_state* d_next,
                                 float* d_color_std, int32_t* d_class, void* stream);

/* Same on HOST buffers: staged through device memory, blocking; every output equals
 * lrt_temporal_upsample_device's bit for bit (the alphas of next->color and color_std are the host
 * buffers' own). */
int lrt_temporal_upsample_host(const lrt_temporal_upsample_desc* desc, const float* color_low,
                               const lrt_gbuffer* low, const lrt_gbuffer* cur, const lrt_gbuffer* prev_g,
                               const lrt_temporal_state* prev, const lrt_temporal_state* next,
                               float* color_std, int32_t* class_out);

/* ---- history rectification: the state held to the frame's local range -------------- */

/* The temporal stages above accept a history tap whenever its id (and normal) agree. Where a shadow
 * crosses a floor, a light is dimmed or a mirror shows something that moved, ids and normals stay,
 * and the stale colour decays at alpha_min per frame. This stage is the correction that TAA variance
 * clipping, ReLAX history clamping and FSR 2 share: the local mean and standard deviation of a
 * reference frame, the history clamped into that range, and the history length shortened where the
 * clamp had to move it, so that it re-converges at 1/n instead of alpha_min. It reads and writes the
 * (color, moment2) state that lrt_temporal_accumulate_gbuffer_* and lrt_temporal_upsample_* leave.
 * f32, not bit-pinned (contraction allowed).
 *
 * Buffers. ref: a whole frame of RGBA quads at the state's resolution: the current frame's colour
 * (the intended use, with ref_scale = the step's cur_scale), a faster history, or an upsampled low
 * frame. id: the current G-buffer's id plane. Of state and out only color and moment2 are required
 * and touched.
 *
 * Per pixel p, with i = id(p), r(q) = ref_scale ref(q).rgb, K = r(p), c and M the state's color and
 * moment2 rgb and n moment2's alpha:
 *  1. Window. q = p + (dx, dy), |dx|, |dy| <= radius. A tap counts iff it lies inside the image and
 *     id(q) = i; the centre always counts, a miss matches a miss (-1 = -1), and no id is ever used
 *     as an index. m is the count. Per channel the sums are taken about the pixel's own reference
 *     value, so that nothing cancels against K: S1 = sum (r(q) - K), S2 = sum (r(q) - K)^2 over the
 *     counting taps. A tap that does not count is kept out by a select, not by a product with 0: a
 *     non-finite reference value reaches only the pixels that count its tap. a = S1 / m, mu = K + a,
 *     sigma = sqrt(max(S2 / m - a^2, 0)).
 *  2. Support. The pixel is supported iff m >= min_taps. An unsupported pixel passes c, M and n
 *     through bit for bit; its class is 2.
 *  3. Box. lo = mu - gamma sigma, hi = mu + gamma sigma; per channel c' = fminf(fmaxf(c, lo), hi).
 *  4. History. Per channel moved = (c' != c), d = |c' - c|, t = d / (d + gamma sigma + range_floor);
 *     e = (the largest t of the three)^2; n' = n + e (min(n, reset_history) - n). On a moved channel
 *     M' = c'^2 + max(M - c^2, 0): the variance is kept and the mean shifted; M' = M on a channel
 *     that did not move. The class is 1 if any channel moved, else 0; a class-0 pixel comes out bit
 *     for bit as it went in (e = 0 exactly). The square in e makes a rounding-sized overshoot cost
 *     nothing and a large one the whole history.
 *  5. Step 7 of lrt_temporal_*, unchanged, on c', M' and n': color_std, or short_std where
 *     n' < min_history.
 * Outputs: out->color rgb (alpha untouched), out->moment2 (rgb and n'), color_std rgb (alpha
 * untouched) if given, class_out (int32, width * height) if given. Nothing else is written.
 *
 * A non-finite value in the state is that pixel's own affair: what it gives there is unspecified,
 * and it never reaches another pixel, because the state is read at p only.
 *
 * Limits: the box comes from a noisy reference: it is wide where the frame is noisy and catches
 * large changes first. A surface with fewer than min_taps pixels of its id in the window is not
 * rectified. The clamp is per RGB channel, with no YCoCg transform. Whole frames only, the first
 * device, spheres only (the ids are lrt_gbuffer_*'s). Not measured: other references (a fast
 * history), the effect on lrt_svgf's variance estimate, a moving camera. Tolerance-checked against
 * its NumPy restatement (tests/rectify_ref.py); deterministic run to run. */
#define LRT_RECTIFY_MAX_RADIUS 3
typedef struct lrt_rectify_desc {      /* 48 bytes */
    int32_t width, height;             /* a whole frame */
    int32_t radius;                    /* 1..LRT_RECTIFY_MAX_RADIUS: the window is (2 radius + 1)^2 */
    int32_t min_taps;                  /* 1..(2 radius + 1)^2 */
    int32_t min_history;               /* >= 1: color_std's, step 7 of lrt_temporal_* */
    int32_t flags;                     /* 0 */
    float ref_scale;                   /* finite, > 0: multiplies the reference only (cur_scale's role) */
    float gamma;                       /* finite, >= 0: the box is mean +- gamma sigma */
    float range_floor;                 /* finite, > 0 */
    float reset_history;               /* finite, >= 0 */
    float short_std;                   /* finite, > 0 */
    int32_t reserved;                  /* 0 */
} lrt_rectify_desc;

/* The defaults: radius 2, min_taps 5, gamma 1, range_floor 1e-4, reset_history 1, ref_scale 1;
 * min_history 4 and short_std 1e3 (lrt_temporal_gbuffer_default's). Choices in the range the
 * techniques named above use, not values tuned here. */
int lrt_temporal_rectify_default(int width, int height, lrt_rectify_desc* out);

/* One call on device buffers. d_color_std and d_class may be NULL.
 *
 * Aliasing: d_out->color may equal d_state->color and d_out->moment2 may equal d_state->moment2,
 * exactly (in place), each independently. Otherwise no output may overlap an input or another
 * output, by address range (the id and class planes are width * height * 4 bytes, the others 16
 * bytes per pixel); d_ref and d_id may never overlap an output.
 *
 * LRT_E_INVALID, before any device use: NULL required pointers; sizes < 1 or width * height >
 * INT_MAX / 4; radius outside 1..LRT_RECTIFY_MAX_RADIUS; min_taps outside 1..(2 radius + 1)^2;
 * min_history < 1; flags or reserved != 0; non-finite parameters; ref_scale, range_floor or
 * short_std <= 0; gamma or reset_history < 0; aliasing other than the above. Then LRT_E_STATE
 * without lrt_initialize(). Asynchronous on `stream` and ordered only against it, with no host
 * round trip and no scratch. Acts on the first device. */
int lrt_temporal_rectify_device(const lrt_rectify_desc* desc, const float* d_ref, const int32_t* d_id,
                                const lrt_temporal_state* d_state, const lrt_temporal_state* d_out,
                                float* d_color_std, int32_t* d_class, void* stream);

/* Same on HOST buffers: staged through device memory, blocking; every output equals
 * lrt_temporal_rectify_device's bit for bit (the alphas of out->color and color_std are the host
 * buffers' own). */
int lrt_temporal_rectify_host(const lrt_rectify_desc* desc, const float* ref, const int32_t* id,
                              const lrt_temporal_state* state, const lrt_temporal_state* out,
                              float* color_std, int32_t* class_out);

/* ---- G-buffer chain: guides and path keys through mirrors and glass ---------------- */

/* lrt_gbuffer_* describes the FIRST hit. On a mirror or a glass ball that is the ball, not what is
 * seen in it: the filters find no edge inside a reflection, and the temporal stages keep a history
 * whose reflected content changed. This pass follows the deterministic (delta) part of the path from
 * the pixel-centre primary hit to the first surface that scatters diffusely and describes THAT
 * surface, and it names the whole path with a key. Every consumer treats `id` as an opaque equality
 * key (no id is ever used as an index), so `key` goes to lrt_temporal_accumulate_gbuffer_*,
 * lrt_temporal_upsample_*, lrt_temporal_rectify_* and lrt_upsample_* in place of id, and normal,
 * world_pos and albedo go to lrt_svgf_* and lrt_denoise_* as guides; none of those stages changes.
 * There is no motion plane: motion, and the first-hit normal the temporal step compares, come from
 * lrt_gbuffer_*. f32 throughout, no contraction, whole frames, row 0 at the bottom, the first
 * device, against the scene the library holds.
 *
 * Per pixel:
 *  1. Segment 0 is steps 1 and 2 of lrt_gbuffer_*, word for word (one shared header): the ray
 *     Ray(O, D) through the pixel centre and its closest hit over (kMinT, kMaxT): (id_0, t_0),
 *     P_0 = O + dir t_0, n_0 = normalize(P_0 - c).
 *  2. The walk. After k followed surfaces the hit is (id_k, P_k, n_k), reached along the unit
 *     direction d_k. The hit is DELTA iff its material is LRT_METAL with roughness <= roughness_max,
 *     or LRT_DIELECTRIC (the type is tested first). The walk ends on a miss, on a hit that is not
 *     delta, or once k = max_bounces; in the last case a delta hit leaves the pixel UNRESOLVED.
 *       Metal:      d' = reflect(d_k, n_k) = d_k + 2 (-(d_k.n_k) n_k); throughput T *= albedo.
 *       Dielectric: Scatter's geometry (parallel.cpp:149-190) without its random choice:
 *                   dn = d_k.n_k; dn > 0: outwardN = -n_k, nint = ri; else outwardN = n_k,
 *                   nint = 1 / ri (one IEEE division). d' = the refracted direction
 *                   nint (d_k - outwardN dt) - outwardN sqrt(discr), dt = d_k.outwardN,
 *                   discr = 1 - nint nint (1 - dt dt), if discr > 0; otherwise reflect(d_k, n_k)
 *                   (total internal reflection). T is unchanged (the attenuation is 1).
 *     The next ray is Ray(P_k, d') (one normalize), its closest hit over the same (kMinT, kMaxT)
 *     gives (id_{k+1}, t_{k+1}), and the path length grows by t_{k+1}.
 *  3. The key. -1 on a primary miss; id_0 where no surface was followed. Otherwise, in uint32
 *     arithmetic (exact, wrapping): h = (uint32)id_0; for each further hit or miss j >= 1 (a miss
 *     has id_j = -1): h = h * 0x9E3779B1 + (uint32)(id_j + 1), then h ^= h >> 15;
 *     key = 0x40000000 | (h & 0x3FFFFFFF). A chain key is therefore never a plain id or -1. Two
 *     different paths may share a key (30 bits); a consumer then keeps a history it could have
 *     dropped, which is what it did on every such pixel before.
 *  4. Outputs, each optional, at least one given:
 *       normal, world_pos: guide_scale * (n, P) of the terminal hit, alpha written 0; 0 where the
 *                  walk ended on the sky, as lrt_gbuffer_* writes a miss.
 *       albedo:    guide_scale * (T * the terminal material's albedo); where the walk ended on the
 *                  sky after at least one followed surface, guide_scale * T (the tint alone); 0 on a
 *                  primary miss, as lrt_gbuffer_*. Alpha written 0.
 *       key:       step 3.
 *       id:        the terminal sphere, -1: the sky.
 *       bounces:   the surfaces followed, plus LRT_CHAIN_UNRESOLVED on an unresolved pixel.
 *       depth:     t_0 + t_1 + ... summed in that order; +Inf where the terminal is the sky.
 *
 * Two identities hold bit for bit: with max_bounces = 0 every shared plane equals lrt_gbuffer_*'s on
 * any scene (key = id = its id; bounces = 0, or LRT_CHAIN_UNRESOLVED on a delta first hit); and for
 * any max_bounces the same holds at every pixel whose first hit is not delta.
 *
 * key, id and bounces are compared exactly, the float planes by tolerance, against the NumPy
 * restatement (tests/gbuffer_chain_ref.py). Limits: the chain is the deterministic branch only
 * (glass shows its refraction, never its Fresnel reflection; a rough metal below roughness_max is
 * followed as if polished). This pass writes no motion plane: the motion vector of what a followed
 * pixel shows is lrt_gbuffer_chain_motion_*'s, further down; with lrt_gbuffer_*'s first-hit motion
 * alone a reflection is reprojected as the ball's surface. A terminal on the sky has zero normal and
 * position. Spheres only, whole frames, the first device. */
#define LRT_CHAIN_MAX_BOUNCES 16
#define LRT_CHAIN_UNRESOLVED 0x100
typedef struct lrt_gbuffer_chain_desc {
    int32_t width, height;          /* a whole frame */
    int32_t flags, reserved;        /* 0 */
    lrt_camera camera;
    int32_t max_bounces;            /* 0..LRT_CHAIN_MAX_BOUNCES; default 4 */
    float roughness_max;            /* finite, >= 0; default 0.25 */
    float guide_scale;              /* finite, > 0; default 1 (lrt_gbuffer_desc.guide_scale's role) */
    int32_t reserved2;              /* 0 */
} lrt_gbuffer_chain_desc;

typedef struct lrt_gbuffer_chain {  /* every member optional, at least one non-NULL */
    float* normal;      /* RGBA quads: rgb = guide_scale * terminal n, alpha written 0 */
    float* world_pos;   /* RGBA quads: rgb = guide_scale * terminal P, alpha written 0 */
    float* albedo;      /* RGBA quads: rgb = guide_scale * T * terminal albedo, alpha written 0 */
    int32_t* key;       /* width*height: the path key */
    int32_t* id;        /* width*height: the terminal sphere, -1: the sky */
    int32_t* bounces;   /* width*height: surfaces followed (+ LRT_CHAIN_UNRESOLVED) */
    float* depth;       /* width*height: the path's length; +Inf where it ends on the sky */
} lrt_gbuffer_chain;

/* The defaults for a width x height frame and a camera: max_bounces 4, roughness_max 0.25,
 * guide_scale 1. Choices, not tuned values: on the default scene 0.25 follows spheres 3, 4 and 5
 * and stops at sphere 6 (roughness 0.6). */
int lrt_gbuffer_chain_default(int width, int height, const lrt_camera* camera, lrt_gbuffer_chain_desc* out);

/* The pass into device buffers. Only the planes given are written. Scenes of up to 16 spheres are
 * scanned, larger ones go through the uniform grid (built on first use, as a render would).
 *
 * LRT_E_INVALID, before any device use: NULL desc or d_out, or all seven planes NULL; sizes < 1 or
 * width * height > INT_MAX / 4; flags, reserved or reserved2 != 0; max_bounces outside
 * 0..LRT_CHAIN_MAX_BOUNCES; roughness_max not finite or < 0; guide_scale not finite or <= 0; any two
 * planes overlapping by address range (16 bytes per pixel for the quads, 4 for key, id, bounces and
 * depth). Then LRT_E_STATE without lrt_initialize(). Asynchronous on `stream` and ordered only
 * against it, with no host round trip and no scratch; it sees the scene as an lrt_render_device
 * call made at the same moment would. Acts on the first device. */
int lrt_gbuffer_chain_device(const lrt_gbuffer_chain_desc* desc, const lrt_gbuffer_chain* d_out, void* stream);

/* Same into HOST buffers: staged through device memory, blocking; every output equals
 * lrt_gbuffer_chain_device's bit for bit. */
int lrt_gbuffer_chain_host(const lrt_gbuffer_chain_desc* desc, const lrt_gbuffer_chain* out);

/* ---- G-buffer chain motion: motion vectors inside mirrors and glass --------------- */

/* lrt_gbuffer_*'s motion is the motion of the FIRST hit: on a mirror or a glass ball, of the ball's
 * surface, not of what is seen in it. For every pixel whose chain (lrt_gbuffer_chain_*) followed at
 * least one surface this pass finds the position q in the PREVIOUS frame whose chain, under the
 * previous camera and scene, ends at the same surface point, and writes motion = q - p in
 * lrt_gbuffer_*'s layout. Everywhere else, and wherever the search fails, it copies the first-hit
 * motion it was given, bit for bit. The plane goes where `motion` goes
 * (lrt_temporal_accumulate_gbuffer_*, lrt_temporal_upsample_*, lrt_temporal_rectify_*), with the
 * chain's key as id; no stage changes. Every surface is a sphere and glass refracts, so there is no
 * closed form: the definition is a search with a fixed number of steps, and it checks its own
 * answer. f32 throughout, no contraction, whole frames, row 0 at the bottom, the first device.
 *
 * chain(C, S, fx, fy) is the chain at a continuous pixel position under camera C and spheres S:
 * s = (fx + 0.5f) * (1.0f / (float)width), t = (fy + 0.5f) * (1.0f / (float)height) (the host's
 * reciprocals), D = ((L + s H) + t V) - O, the ray Ray(O, D), its closest hit, then the walk of
 * lrt_gbuffer_chain_* step 2 and the key of step 3, unchanged (materials: the current ones). At
 * integer fx, fy it is lrt_gbuffer_chain_*'s pixel. It yields the key, the terminal id, the bounces
 * and the terminal vector F: the terminal point P on a hit, the last ray's unit direction where the
 * walk ends on the sky.
 *
 * Per pixel (x, y):
 *  1. (K, j, b, Y) = chain(camera, the current spheres, x, y). Nothing followed (a primary miss
 *     included): LRT_CM_NOT_FOLLOWED. Unresolved after at least one surface: LRT_CM_UNRESOLVED.
 *  2. The target Y'. If j >= 0, `scene` is given and sphere j's eight floats differ in a bit between
 *     scene->spheres and scene->prev_spheres: Y' = c' + (r' / r) (Y - c), lrt_gbuffer_*'s carry-back.
 *     Otherwise Y' = Y. With `scene` given, r' <= 0 or r <= 0 of sphere j: LRT_CM_NO_SEED.
 *  3. The seed q = (x + mx, y + my) of first_motion's quad (mx, my, ., mw). mw == 0, or a q that
 *     fails |q.x|, |q.y| < 1e6 (a NaN fails): LRT_CM_NO_SEED. This is the test of step 1 of
 *     lrt_temporal_accumulate_gbuffer_*: a vector that stage would not take is not searched from.
 *  4. `iterations` times: F0 = chain(prev_camera, the previous spheres, q), Fx at q + (probe_px, 0),
 *     Fy at q + (0, probe_px). Any of the three keys other than K: LRT_CM_KEY_LOST.
 *     Jx = (Fx - F0) (1 / probe_px), Jy = (Fy - F0) (1 / probe_px) (one host division), r = Y' - F0;
 *     a = Jx.Jx, bb = Jx.Jy, c = Jy.Jy, e = Jx.r, f = Jy.r, det = a c - bb bb;
 *     dx = (c e - bb f) / det, dy = (a f - bb e) / det. A dx or dy that is not finite:
 *     LRT_CM_NOT_CONVERGED. len = sqrt(dx dx + dy dy); if len > step_max_px both are multiplied by
 *     step_max_px / len. q += (dx, dy); a q that fails |q.x|, |q.y| < 1e6: LRT_CM_NOT_CONVERGED
 *     (no ray is cast from there; the defaults move q by at most 48 pixels).
 *  5. F0 = chain(prev_camera, the previous spheres, q); a key other than K: LRT_CM_KEY_LOST.
 *     (dx, dy) as above with the LAST iteration's Jx and Jy and the new r; rem = sqrt(dx dx + dy dy).
 *     LRT_CM_CONVERGED iff rem <= converged_px and |q.x|, |q.y| < 1e6 (a NaN fails); otherwise
 *     LRT_CM_NOT_CONVERGED.
 *  6. Outputs, each optional, at least one given:
 *       motion: where LRT_CM_CONVERGED, (q.x - x, q.y - y, first_motion's third word, 1); everywhere
 *               else first_motion's quad, its four words unchanged.
 *       status: the LRT_CM_* constant.
 * The iteration count is fixed and there is no early exit. A static frame has r = 0 and a step of
 * exactly 0: under bit-identical cameras and an unmoved scene, motion equals first_motion at every
 * pixel, bit for bit. A pixel costs 1 + 3 iterations + 1 walks: 11 at the defaults.
 *
 * `scene` follows lrt_gbuffer_device's rules and must have at most 16 spheres (the scanned scenes:
 * the previous spheres travel in the kernel's arguments). With `scene` NULL the previous scene is
 * the current one, at any count; above 16 spheres the walks go through the uniform grid.
 *
 * status is compared exactly and motion by tolerance against the NumPy restatement
 * (tests/gbuffer_chain_motion_ref.py). Limits: the search needs the previous frame to have shown
 * the same path key: content newly reflected falls back to the first-hit motion, and the key test
 * of the temporal stages then drops it, as before. A silhouette pixel whose probe crosses a key
 * boundary falls back too. Glass shows its refraction only (the chain's limit). Scene motion up to
 * 16 spheres; the previous materials are the current ones. Spheres only, whole frames, the first
 * device. */
#define LRT_CM_NOT_FOLLOWED 0   /* the chain followed nothing: first_motion is the pixel's motion */
#define LRT_CM_CONVERGED 1      /* motion was written */
#define LRT_CM_UNRESOLVED 2     /* the chain is LRT_CHAIN_UNRESOLVED */
#define LRT_CM_NO_SEED 3        /* first_motion is not projectable, or the terminal sphere did not exist */
#define LRT_CM_KEY_LOST 4       /* an evaluation in the previous frame had another path key */
#define LRT_CM_NOT_CONVERGED 5  /* a step was not finite, or the remaining step exceeds converged_px */
#define LRT_CM_MAX_ITERATIONS 8
typedef struct lrt_gbuffer_chain_motion_desc {
    int32_t width, height;          /* a whole frame */
    int32_t flags, reserved;        /* 0 */
    lrt_camera camera, prev_camera;
    int32_t max_bounces;            /* 0..LRT_CHAIN_MAX_BOUNCES; default 4 (the chain desc's) */
    float roughness_max;            /* finite, >= 0; default 0.25 (the chain desc's) */
    int32_t iterations;             /* 1..LRT_CM_MAX_ITERATIONS; default 3 */
    float probe_px;                 /* finite, > 0; default 0.25 */
    float step_max_px;              /* finite, > 0; default 16 */
    float converged_px;             /* finite, > 0; default 0.0625 */
    int32_t reserved2, reserved3;   /* 0 */
} lrt_gbuffer_chain_motion_desc;

typedef struct lrt_gbuffer_chain_motion {  /* both optional, at least one non-NULL */
    float* motion;      /* RGBA quads, all four written (lrt_gbuffer.motion's layout) */
    int32_t* status;    /* width*height: LRT_CM_* */
} lrt_gbuffer_chain_motion;

/* The defaults for a width x height frame and a camera pair: the chain's max_bounces 4 and
 * roughness_max 0.25, iterations 3, probe_px 0.25, step_max_px 16, converged_px 0.0625.
 * prev_camera == NULL: the camera. */
int lrt_gbuffer_chain_motion_default(int width, int height, const lrt_camera* camera, const lrt_camera* prev_camera,
                                     lrt_gbuffer_chain_motion_desc* out);

/* The pass into device buffers. d_first_motion: the motion plane of an lrt_gbuffer_* call for the
 * same camera pair and scene pair (width*height RGBA quads), required. `scene` may be NULL; if given
 * it is read from host memory before the call returns. Only the planes given are written.
 *
 * LRT_E_INVALID, before any device use: NULL desc or d_out, or both planes NULL; sizes < 1 or
 * width * height > INT_MAX / 4; flags or a reserved word != 0; max_bounces outside
 * 0..LRT_CHAIN_MAX_BOUNCES; roughness_max not finite or < 0; iterations outside
 * 1..LRT_CM_MAX_ITERATIONS; probe_px, step_max_px or converged_px not finite or <= 0; a prev_camera
 * that lrt_temporal_* rejects; d_first_motion NULL; an output overlapping d_first_motion or the other
 * output by address range; with `scene`, what lrt_gbuffer_device refuses, or a count above 16. Then
 * LRT_E_STATE without lrt_initialize(). Asynchronous on `stream` and ordered only against it, with
 * no host round trip and no scratch. Acts on the first device. */
int lrt_gbuffer_chain_motion_device(const lrt_gbuffer_chain_motion_desc* desc, const lrt_scene_motion* scene,
                                    const float* d_first_motion, const lrt_gbuffer_chain_motion* d_out, void* stream);

/* Same with HOST buffers: staged through device memory, blocking; every output equals
 * lrt_gbuffer_chain_motion_device's bit for bit. */
int lrt_gbuffer_chain_motion_host(const lrt_gbuffer_chain_motion_desc* desc, const lrt_scene_motion* scene,
                                  const float* first_motion, const lrt_gbuffer_chain_motion* out);

/* ---- adaptive sampling, part a: the per-pixel sample budget -------------------------------------
 * lrt_sample_budget_* turns a per-pixel noise estimate -- the variance_out of lrt_svgf_filter_*, or
 * the color_std of the temporal stages with LRT_SB_STD -- into an integer sample count per pixel
 * under a total budget, for lrt_render_counts_* below. f32 with no contraction, then exact integers:
 * the counts are pinned exactly to the NumPy restatement (tests/sample_budget_ref.py).
 *
 *  1. Weight. V is the plane's rgb (with LRT_SB_STD each channel squared);
 *     vY = (0.2126f Vr + 0.7152f Vg) + 0.0722f Vb, Y the same expression of the colour's rgb.
 *     With a colour plane w = sqrtf(vY) / (fmaxf(Y, 0) + luma_floor) (a relative error), without
 *     w = sqrtf(vY); sqrtf and the division correctly rounded. A w that is not finite or not > 0
 *     gives q = 0; otherwise q = (uint32)(fminf(w, weight_max) * 65536.0f), truncated. Alphas are
 *     never read.
 *  2. count_p = min_count everywhere.
 *  3. `passes` times: U = {p : count_p < max_count}, E = budget - sum count (int64),
 *     Q = sum over U of q_p (uint64), m = |U|. E <= 0 or m = 0: the pass changes nothing. Q = 0:
 *     add_p = E / m for p in U. Otherwise add_p = (uint64)E * q_p / Q (the product is below 2^62).
 *     count_p = min(max_count, count_p + add_p). sum count <= budget holds after every pass; what a
 *     clamp at max_count frees in one pass is handed out again in the next.
 *  4. d_counts receives width * height int32; d_info[0] = sum count, d_info[1] = pass 1's Q.
 *
 * The sums are integer atomics (exact, independent of order); each pass reads E, Q and m from device
 * memory, so there is no host round trip. Limits: a Neyman-style allocation from a NOISY variance
 * estimate -- a pixel whose few samples happened to agree is starved until min_count samples show
 * otherwise, so min_count >= 1 and a filtered variance are the intended inputs. Whole frames, the
 * first device. */
#define LRT_COUNT_MAX 4096
#define LRT_SB_STD 1                 /* the input plane holds a standard deviation (color_std), not a variance */
typedef struct lrt_sample_budget_desc {
    int32_t width, height;           /* a whole frame */
    int32_t flags, reserved;         /* LRT_SB_STD | 0 ; 0 */
    int32_t min_count, max_count;    /* 0 <= min_count <= max_count <= LRT_COUNT_MAX */
    int32_t passes;                  /* 1..4; default 2 */
    int32_t reserved2;               /* 0 */
    int64_t budget;                  /* min_count * width * height <= budget <= 2^31 - 1 */
    float luma_floor;                /* finite, > 0; default 0.01 */
    float weight_max;                /* finite, > 0, <= 16384; default 256 */
} lrt_sample_budget_desc;

/* The defaults for a width x height frame: flags 0, passes 2, luma_floor 0.01, weight_max 256, and
 * the counts and the budget as given (checked by the call, not here). */
int lrt_sample_budget_default(int width, int height, int min_count, int max_count, long long budget,
                              lrt_sample_budget_desc* out);

/* The counts into device buffers. d_variance: width*height RGBA quads; d_color: the same shape, or
 * NULL; d_counts: width*height int32; d_info: 2 words, or NULL.
 *
 * LRT_E_INVALID, before any device use: NULL desc, d_variance or d_counts; sizes < 1 or
 * width * height > INT_MAX / 4; an unknown flag or a reserved word != 0; min_count, max_count,
 * passes, budget, luma_floor or weight_max outside the ranges above (a non-finite float included);
 * d_counts or d_info overlapping an input or each other by address range. Then LRT_E_STATE without
 * lrt_initialize(); LRT_E_NOMEM if the scratch cannot be had. Asynchronous on `stream` and ordered
 * only against it; the intermediates live in the stream's scratch. Acts on the first device. */
int lrt_sample_budget_device(const lrt_sample_budget_desc* desc, const float* d_variance, const float* d_color,
                             int32_t* d_counts, unsigned long long* d_info, void* stream);

/* Same with HOST buffers: staged through device memory, blocking; counts and info equal
 * lrt_sample_budget_device's exactly. */
int lrt_sample_budget_host(const lrt_sample_budget_desc* desc, const float* variance, const float* color,
                           int32_t* counts, unsigned long long* info);

/* ---- adaptive sampling, part b: a render that honours a per-pixel count plane --------------------
 * lrt_render_counts_* renders the window of an ordinary lrt_render_desc (window, row map, frame0,
 * max_depth and camera honoured; flags must be LRT_F_NONE) with a sample count of its own per pixel.
 *
 *   c_p = min(max(counts[p], 0), desc->frames): frames is the per-pixel cap. Pixels are enumerated
 *   in local row-major order, o_p = sum of c_q over q < p. Pixel p is RENDERED iff c_p > 0 and
 *   o_p + c_p <= capacity; a pixel with c_p > 0 that does not fit is SKIPPED (the pixels behind it
 *   keep their offsets). A rendered pixel runs samples frame0 .. frame0 + c_p - 1 with the usual
 *   seeds, lerped in frame order from the buffer's previous value. Every other pixel keeps all four
 *   floats; alpha is never written. info[0] = the samples traced, info[1] = the skipped pixels;
 *   *d_rays grows by the rays of the samples traced.
 *   LRT_RC_MEAN: after the chain a rendered pixel's rgb is multiplied by
 *   (float)(frame0 + c_p) / (float)c_p (one IEEE division, three multiplications): rendered into a
 *   zeroed buffer with frame0 > 0 this is the plain mean of the pixel's fresh samples, the per-pixel
 *   form of cur_scale; the temporal stages then run with cur_scale = 1.
 *
 * Two identities hold bit for bit. A: a rendered pixel equals the same pixel of lrt_render_device
 * with frames = c_p, everything else equal (whichever kernel that call picks). B: with
 * counts == frames everywhere and enough capacity, buffer and ray count equal lrt_render_device's.
 *
 * Three stages on the stream: an exclusive scan of the clamped counts, a trace kernel over the
 * compacted sample list (64 consecutive samples are neighbouring pixels of a row; one colour slot of
 * 16 B per sample), and a merge with one thread per pixel. Scenes of up to 16 spheres are scanned,
 * larger ones go through the uniform grid, as lrt_gbuffer_chain_* decides; every accelerator gives
 * the same bits. Limits: the first device; no lrt_features (guides come from lrt_gbuffer_*); no
 * row-shard exchange into a frame; the scratch holds min(capacity, pixels * frames) slots. */
#define LRT_RC_MEAN 1
typedef struct lrt_render_counts {
    const int32_t* counts;           /* row_count * x_count, the backbuffer's local shape */
    int64_t capacity;                /* 1 .. 2^27: the most samples the call may trace (sizes its scratch) */
    int32_t flags, reserved;         /* LRT_RC_MEAN | 0 ; 0 */
    unsigned long long* info;        /* optional, 2 words written: samples traced, pixels skipped */
} lrt_render_counts;

/* The render into device buffers (d_rc itself is host memory; its counts and info are device
 * pointers).
 *
 * LRT_E_INVALID, before any device use: what lrt_render_device rejects (a NULL buffer or ray
 * counter included); a window of more than INT_MAX / 4 pixels; NULL d_rc or counts; capacity outside
 * 1 .. 2^27; an unknown flag or reserved != 0; desc->flags != 0; counts or info overlapping the
 * backbuffer or each other by address range. Then LRT_E_STATE without lrt_initialize(); LRT_E_NOMEM
 * if the scratch cannot be had. Asynchronous on `stream` and ordered only against it, with no host
 * read-back. Acts on the first device. */
int lrt_render_counts_device(const lrt_render_desc* desc, const lrt_render_counts* d_rc, float* d_backbuffer,
                             unsigned long long* d_rays, void* stream);

/* Same with HOST buffers (rc->counts, rc->info and backbuffer in host memory): staged through
 * device memory, blocking; *out_rays receives the rays of this call. Bit for bit the device form. */
int lrt_render_counts_host(const lrt_render_desc* desc, const lrt_render_counts* rc, float* backbuffer,
                           long long* out_rays);

/* ---- firefly suppression: a rank-order clamp ahead of the temporal stages ------------- */

/* A renderer that samples the light explicitly leaves isolated pixels tens of times brighter than
 * their surroundings. Blended into a history such a spike stays for 1 / alpha_min frames, and
 * lrt_temporal_rectify_* cannot remove it, because the frame is its reference. This stage is the
 * one that ReLAX / ReBLUR anti-firefly, the RCRS filter and SVGF's pre-pass share: each pixel's
 * luminance is clamped against the `rank`-th largest luminance among its neighbours of the same id.
 * It runs on the current frame's colour, before lrt_temporal_accumulate_gbuffer_*. Comparisons plus
 * a handful of rounded f32 operations, no contraction: every output is pinned bit for bit to the
 * NumPy restatement (tests/firefly_ref.py).
 *
 * Buffers. in: a whole frame of RGBA f32 quads. id: the int32 plane of lrt_gbuffer_* or the chain's
 * key, or NULL: every in-image tap then matches.
 *
 * Y(c) = (0.2126f c.x + 0.7152f c.y) + 0.0722f c.z, lrt_sample_budget_*'s expression. Per pixel p,
 * with c = in(p).rgb:
 *  1. Window. q = p + (dx, dy), |dx|, |dy| <= radius, the centre excluded. A tap counts iff it lies
 *     inside the image, id(q) = id(p) and Y(q) is finite; a miss matches a miss, and no id is ever
 *     used as an index. A tap that does not count is kept out by a select: a non-finite neighbour
 *     never reaches p. m is the count of counting taps.
 *  2. Support. A pixel with m < min_taps passes through bit for bit, whatever it contains (a
 *     non-finite value included); its class is 2.
 *  3. Threshold. Yk is the rank-th largest Y(q) over the counting taps as a multiset (rank 1: the
 *     maximum; only the value is used, so ties need no rule). T = gain * fmaxf(Yk, 0) + floor: one
 *     multiplication and one addition, two roundings. floor > 0 makes T positive and the sign of a
 *     zero Yk irrelevant.
 *  4. Clamp. Y(c) finite and Y(c) > T, strictly: s = T / Y(c) (IEEE division), c' = s c per
 *     channel, class 1. Y(c) not finite (a non-finite channel, or a sum that overflows):
 *     c' = (T, T, T), class 3. Otherwise c' = c bit for bit, class 0.
 *  5. Outputs. out(p) = c' with in(p)'s alpha bits. excess_out(p), if given, is (c - c', 0) for
 *     class 1 and four zeros otherwise: a caller that wants the energy back can blur it and add it.
 *     class_out, if given, is an int32 per pixel. info, if given, is two uint32: the pixels of class
 *     1 and the pixels of class 3; the call zeroes it on the stream and the integers are exact.
 *     Nothing else is written.
 *
 * Limits: the clamp loses energy; energy is not conserved unless the caller re-adds excess_out. A
 * legitimately bright feature smaller than `rank` pixels of its own id (a light seen as one pixel)
 * is dimmed. The threshold comes from one noisy frame. A non-finite pixel without support passes
 * through. Whole frames only, the first device. */
#define LRT_FIREFLY_MAX_RADIUS 2
typedef struct lrt_firefly_desc {      /* 48 bytes */
    int32_t width, height;             /* a whole frame */
    int32_t radius;                    /* 1..LRT_FIREFLY_MAX_RADIUS: the window is (2 radius + 1)^2 - 1 taps */
    int32_t rank;                      /* 1..4 */
    int32_t min_taps;                  /* rank..(2 radius + 1)^2 - 1: the rank-th tap exists on a supported pixel */
    int32_t flags;                     /* 0 */
    float gain;                        /* finite, > 0 */
    float floor;                       /* finite, > 0, in the buffer's own units */
    int32_t reserved[4];               /* 0 */
} lrt_firefly_desc;

/* The defaults: radius 1, rank 2, min_taps 3, gain 2, floor 0.01. Choices in the range the
 * techniques named above use, not values tuned here: rank 2 lets a pair of adjacent spikes be
 * caught; at gain 1 a centre that is merely the largest of nine i.i.d. values would already be
 * clamped. */
int lrt_firefly_default(int width, int height, lrt_firefly_desc* out);

/* One call on device buffers. d_id, d_excess, d_class and d_info may be NULL.
 *
 * Aliasing: no output may overlap an input or another output, by address range (the id and class
 * planes are width * height * 4 bytes, info 8 bytes, the others 16 bytes per pixel). In place is
 * not allowed, since neighbours are read.
 *
 * LRT_E_INVALID, before any device use: NULL desc, d_in or d_out; sizes < 1 or width * height >
 * INT_MAX / 4; radius outside 1..LRT_FIREFLY_MAX_RADIUS; rank outside 1..4; min_taps outside
 * rank..(2 radius + 1)^2 - 1; flags or reserved != 0; gain or floor not finite or <= 0; any overlap
 * named above. Then LRT_E_STATE without lrt_initialize(). Asynchronous on `stream` and ordered only
 * against it, with no host round trip and no scratch. Acts on the first device. */
int lrt_firefly_device(const lrt_firefly_desc* desc, const float* d_in, const int32_t* d_id, float* d_out,
                       float* d_excess, int32_t* d_class, uint32_t* d_info, void* stream);

/* Same on HOST buffers: staged through device memory, blocking; every output equals
 * lrt_firefly_device's bit for bit. */
int lrt_firefly_host(const lrt_firefly_desc* desc, const float* in, const int32_t* id, float* out,
                     float* excess_out, int32_t* class_out, uint32_t* info);

/* ---- firefly restore: the clamp's excess spread back over its surface ------------------ */

/* lrt_firefly_* removes energy (7 to 8 % of a 4 spp frame's luminance) that no accumulation
 * returns. This stage spreads the excess of every clamped pixel over that pixel's neighbours of the
 * same id with a tent kernel, each source normalised so that what it gives away sums to what it
 * had, and adds the result to a frame. Small-integer weights, one division, one multiplication and
 * one addition per tap in a fixed order, no contraction: `out` is pinned bit for bit to the NumPy
 * restatement (tests/firefly_restore_ref.py).
 *
 * Buffers. color: a whole frame of RGBA f32 quads, the clamped `out` of lrt_firefly_* or any later
 * frame of the same size. excess: RGBA f32, the excess_out of lrt_firefly_*; any plane is legal
 * input. id: int32 or NULL: every tap in the image then matches; a miss matches a miss, and no id
 * is ever used as an index. out: RGBA f32.
 *
 * With R = radius, t(d) = R + 1 - |d| and w(dx, dy) = t(dx) t(dy): small integers, exact in f32.
 *  1. Source. e(p) = excess(p).xyz if all three channels satisfy |e| <= 0x1p100f, otherwise
 *     (0, 0, 0): NaN and +-Inf fail the test. A select. The cap keeps every partial sum finite, so
 *     no NaN is ever made by arithmetic.
 *  2. Normaliser. W(p) = the sum of w(dx, dy) over dx, dy in -R..R, the centre included, over the
 *     taps q = p + (dx, dy) that lie in the image with id(q) = id(p): an integer in
 *     (R + 1)^2..(R + 1)^4, exact in f32 in any order. n(p) = e(p) / (float)W(p), one IEEE division
 *     per channel.
 *  3. Gather. Per destination q, acc = (+0, +0, +0); for dy = -R..R ascending and inside it
 *     dx = -R..R ascending, p = q + (dx, dy): if p lies in the image and id(p) = id(q),
 *     acc = acc + (float)w(dx, dy) * n(p) per channel, one rounded multiplication and then one
 *     rounded addition. A tap that does not count is skipped.
 *  4. Write. Per channel out.c = color.c + acc.c if acc.c != 0 and color.c is finite; otherwise
 *     out.c keeps color.c's bits. out.w keeps color.w's bits. A pixel that no excess reaches comes
 *     out bit for bit, -0, NaN payloads and alpha included.
 *
 * The id test and the weights are symmetric, so in real arithmetic the sum of out over the frame is
 * the sum of color plus the sum of e: a source alone on its id gets its own excess back
 * (W = (R + 1)^2, one tap).
 *
 * Limits: energy returns to the surface, not to the pixel it left, so the frame is blurred by what
 * was clamped; a source whose excess is not finite or above 0x1p100f gives nothing; rounding makes
 * the conservation first-order exact only ((2R + 1)^2 + 3 roundings of 2^-24 per pixel). Whole
 * frames only, the first device. */
#define LRT_FIREFLY_RESTORE_MAX_RADIUS 4
typedef struct lrt_firefly_restore_desc {   /* 32 bytes */
    int32_t width, height;             /* a whole frame */
    int32_t radius;                    /* 1..LRT_FIREFLY_RESTORE_MAX_RADIUS: the tent spans (2 radius + 1)^2 taps */
    int32_t flags;                     /* 0 */
    int32_t reserved[4];               /* 0 */
} lrt_firefly_restore_desc;

/* The default: radius 2. */
int lrt_firefly_restore_default(int width, int height, lrt_firefly_restore_desc* out);

/* One call on device buffers. d_id may be NULL.
 *
 * Aliasing: d_out may be d_color itself (the same pointer: in place; a thread reads only its own
 * color quad). Any other overlap between d_out and an input, by address range (the id plane is
 * width * height * 4 bytes, the others 16 bytes per pixel), is refused.
 *
 * LRT_E_INVALID, before any device use: NULL desc, d_color, d_excess or d_out; sizes < 1 or
 * width * height > INT_MAX / 4; radius outside 1..LRT_FIREFLY_RESTORE_MAX_RADIUS; flags or reserved
 * != 0; any overlap named above. Then LRT_E_STATE without lrt_initialize(). Asynchronous on
 * `stream` and ordered only against it, with no host round trip, no scratch and no atomics. Acts on
 * the first device. */
int lrt_firefly_restore_device(const lrt_firefly_restore_desc* desc, const float* d_color, const float* d_excess,
                               const int32_t* d_id, float* d_out, void* stream);

/* Same on HOST buffers: staged through device memory, blocking; out equals
 * lrt_firefly_restore_device's bit for bit. out may be color itself. */
int lrt_firefly_restore_host(const lrt_firefly_restore_desc* desc, const float* color, const float* excess,
                             const int32_t* id, float* out);

#ifdef __cplusplus
}
#endif
#endif /* LRT_H */
