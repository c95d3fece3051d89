"""ctypes binding of liblrt_hip.so (the C-ABI declared in include/lrt.h).

The library is the product: HIP kernels for gfx950 plus the C-ABI shim. There is no
CPU fallback anywhere in this package -- if the library is missing or fails to load,
`lib()` raises LrtError.
"""
from __future__ import annotations

import ctypes
import os
import threading

_HERE = os.path.dirname(os.path.abspath(__file__))
# LRT_LIB overrides the library path (development A/B builds only)
LIB_PATH = os.environ.get("LRT_LIB") or os.path.join(_HERE, "liblrt_hip.so")
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "lrt.h")
DIAG_HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "lrt_diag.h")   # diagnostics

LRT_OK = 0
LRT_E_INVALID = -1
LRT_E_HIP = -2
LRT_E_STATE = -3
LRT_E_NOMEM = -4

LAMBERT, METAL, DIELECTRIC = 0, 1, 2          # parallel.cpp:31
REFERENCE_MAX_DEPTH = 20                      # parallel.cpp:12
MAX_SPHERES = 4096
F_SCENE_GLOBAL = 1
F_SIMPLE = 2
F_NO_BVH = 32
F_NO_DOUBLE_LIGHT = 64
F_WAVEFRONT = 256
F_POOL = 512
F_BVH = 1024
F_GRID = 2048
REMOVED_FLAG_BITS = (4, 8, 16, 128)   # v1, v2s, v2, v3 (rounds 2-3): rejected with LRT_E_INVALID
DEV_PEER_COPY = 1   # lrt_initialize_devices: gather by device-to-device copies, not RCCL
DEV_GATHER = 2      # lrt_initialize_devices: gather the shards into the first device (RCCL)
IPC_HANDLE_BYTES = 64


class LrtError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"lrt error {code}: {msg}")
        self.code = code


class Float3(ctypes.Structure):               # maths.h:10-61
    _fields_ = [("x", ctypes.c_float), ("y", ctypes.c_float), ("z", ctypes.c_float)]

    def tolist(self):
        return [self.x, self.y, self.z]


class Sphere(ctypes.Structure):               # maths.h:156-163
    _fields_ = [("center", Float3), ("radius", ctypes.c_float)]


class Material(ctypes.Structure):             # parallel.cpp:29-37
    _fields_ = [("type", ctypes.c_int32), ("albedo", Float3), ("emissive", Float3),
                ("roughness", ctypes.c_float), ("ri", ctypes.c_float)]


class Camera(ctypes.Structure):               # maths.h:176-225
    _fields_ = [("origin", Float3), ("a", Float3), ("u", Float3), ("r", Float3),
                ("lowerLeftCorner", Float3), ("horizontalVec", Float3),
                ("verticalVec", Float3), ("lensRadius", ctypes.c_float)]

    def to22(self):
        out = []
        for name in ("origin", "a", "u", "r", "lowerLeftCorner", "horizontalVec", "verticalVec"):
            out += getattr(self, name).tolist()
        return out + [self.lensRadius]


class RenderDesc(ctypes.Structure):           # lrt_render_desc
    _fields_ = [("camera", Camera),
                ("width", ctypes.c_int32), ("height", ctypes.c_int32),
                ("x0", ctypes.c_int32), ("x_count", ctypes.c_int32),
                ("y0", ctypes.c_int32), ("row_count", ctypes.c_int32),
                ("row_block", ctypes.c_int32), ("row_period", ctypes.c_int32),
                ("row_phase", ctypes.c_int32),
                ("frame0", ctypes.c_int32), ("frames", ctypes.c_int32),
                ("max_depth", ctypes.c_int32), ("flags", ctypes.c_int32)]


class Features(ctypes.Structure):             # lrt_features (fragmentShader.fs.glsl:444-451, 494-568)
    _fields_ = [("normal", ctypes.c_void_p), ("world_pos", ctypes.c_void_p), ("albedo", ctypes.c_void_p),
                ("color_std", ctypes.c_void_p), ("normal_std", ctypes.c_void_p),
                ("world_pos_std", ctypes.c_void_p), ("max_frame", ctypes.c_int32), ("reserved", ctypes.c_int32)]


FEATURE_NAMES = ("normal", "world_pos", "albedo", "color_std", "normal_std", "world_pos_std")
GUIDE_NAMES = ("normal", "world_pos", "albedo", "color_std")   # what lrt_denoise_* reads of lrt_features
DENOISE_MAX_ITER = 5


class DenoiseDesc(ctypes.Structure):          # lrt_denoise_desc
    _fields_ = [("width", ctypes.c_int32), ("height", ctypes.c_int32),
                ("iterations", ctypes.c_int32), ("flags", ctypes.c_int32),
                ("sigma_color", ctypes.c_float), ("sigma_normal", ctypes.c_float),
                ("sigma_pos", ctypes.c_float), ("sigma_albedo", ctypes.c_float)]


class TemporalDesc(ctypes.Structure):         # lrt_temporal_desc
    _fields_ = [("width", ctypes.c_int32), ("height", ctypes.c_int32),
                ("flags", ctypes.c_int32), ("min_history", ctypes.c_int32),
                ("camera", Camera), ("prev_camera", Camera),
                ("cur_scale", ctypes.c_float), ("alpha_min", ctypes.c_float), ("normal_min", ctypes.c_float),
                ("pos_tol", ctypes.c_float), ("short_std", ctypes.c_float), ("reserved", ctypes.c_int32)]


class TemporalState(ctypes.Structure):        # lrt_temporal_state
    _fields_ = [("color", ctypes.c_void_p), ("moment2", ctypes.c_void_p), ("normal", ctypes.c_void_p),
                ("world_pos", ctypes.c_void_p), ("albedo", ctypes.c_void_p)]


class SceneMotion(ctypes.Structure):          # lrt_scene_motion
    _fields_ = [("spheres", ctypes.POINTER(Sphere)), ("prev_spheres", ctypes.POINTER(Sphere)),
                ("count", ctypes.c_int32), ("reserved", ctypes.c_int32)]


TEMPORAL_STATE_NAMES = ("color", "moment2", "normal", "world_pos", "albedo")
TEMPORAL_CUR_NAMES = ("normal", "world_pos", "albedo")   # what lrt_temporal_* reads of lrt_features
TEMPORAL_PARAMS = ("cur_scale", "alpha_min", "normal_min", "pos_tol", "short_std", "min_history")

SVGF_MAX_ITER = 5
SVGF_GUIDE_NAMES = ("normal", "world_pos", "albedo")   # what lrt_svgf_* reads of lrt_features
SVGF_PARAMS = ("iterations", "min_history", "sigma_color", "sigma_normal", "sigma_pos", "albedo_floor")


class SvgfDesc(ctypes.Structure):             # lrt_svgf_desc
    _fields_ = [("width", ctypes.c_int32), ("height", ctypes.c_int32),
                ("iterations", ctypes.c_int32), ("flags", ctypes.c_int32),
                ("min_history", ctypes.c_int32), ("reserved", ctypes.c_int32),
                ("sigma_color", ctypes.c_float), ("sigma_normal", ctypes.c_float),
                ("sigma_pos", ctypes.c_float), ("albedo_floor", ctypes.c_float)]


TONEMAP_BINS = 256
TONEMAP_HIST_WORDS = 258                      # 256 bins, then `under`, then `over`
TM_LINEAR, TM_REINHARD, TM_ACES = 0, 1, 2
TM_MAX = 65504.0
TONEMAP_PARAMS = ("op", "auto_exposure", "key", "p_low", "p_high", "ev_bias", "ev_min", "ev_max", "adapt", "white")
TONEMAP_OPS = {"linear": TM_LINEAR, "reinhard": TM_REINHARD, "aces": TM_ACES}


class TonemapDesc(ctypes.Structure):          # lrt_tonemap_desc
    _fields_ = [("width", ctypes.c_int32), ("height", ctypes.c_int32),
                ("op", ctypes.c_int32), ("auto_exposure", ctypes.c_int32),
                ("flags", ctypes.c_int32), ("reserved", ctypes.c_int32),
                ("key", ctypes.c_float), ("p_low", ctypes.c_float), ("p_high", ctypes.c_float),
                ("ev_bias", ctypes.c_float), ("ev_min", ctypes.c_float), ("ev_max", ctypes.c_float),
                ("adapt", ctypes.c_float), ("white", ctypes.c_float)]


class ExposureState(ctypes.Structure):        # lrt_exposure_state
    _fields_ = [("log2_exposure", ctypes.c_float), ("log2_luminance", ctypes.c_float),
                ("counted", ctypes.c_float), ("frames", ctypes.c_float)]


class GbufferDesc(ctypes.Structure):         # lrt_gbuffer_desc
    _fields_ = [("width", ctypes.c_int32), ("height", ctypes.c_int32),
                ("flags", ctypes.c_int32), ("reserved", ctypes.c_int32),
                ("camera", Camera), ("prev_camera", Camera),
                ("guide_scale", ctypes.c_float), ("reserved2", ctypes.c_int32)]


class Gbuffer(ctypes.Structure):              # lrt_gbuffer
    _fields_ = [("normal", ctypes.c_void_p), ("world_pos", ctypes.c_void_p), ("albedo", ctypes.c_void_p),
                ("motion", ctypes.c_void_p), ("id", ctypes.c_void_p), ("depth", ctypes.c_void_p)]


GBUFFER_GUIDE_NAMES = ("normal", "world_pos", "albedo")   # always returned
GBUFFER_EXTRA_NAMES = ("id", "depth", "motion")           # on request
GBUFFER_NAMES = GBUFFER_GUIDE_NAMES + GBUFFER_EXTRA_NAMES

CHAIN_MAX_BOUNCES = 16      # LRT_CHAIN_MAX_BOUNCES
CHAIN_UNRESOLVED = 0x100    # LRT_CHAIN_UNRESOLVED, in the bounces plane


class GbufferChainDesc(ctypes.Structure):    # lrt_gbuffer_chain_desc
    _fields_ = [("width", ctypes.c_int32), ("height", ctypes.c_int32),
                ("flags", ctypes.c_int32), ("reserved", ctypes.c_int32),
                ("camera", Camera),
                ("max_bounces", ctypes.c_int32), ("roughness_max", ctypes.c_float),
                ("guide_scale", ctypes.c_float), ("reserved2", ctypes.c_int32)]


class GbufferChain(ctypes.Structure):         # lrt_gbuffer_chain
    _fields_ = [("normal", ctypes.c_void_p), ("world_pos", ctypes.c_void_p), ("albedo", ctypes.c_void_p),
                ("key", ctypes.c_void_p), ("id", ctypes.c_void_p), ("bounces", ctypes.c_void_p),
                ("depth", ctypes.c_void_p)]


GBUFFER_CHAIN_GUIDE_NAMES = ("normal", "world_pos", "albedo")   # RGBA quads
GBUFFER_CHAIN_INT_NAMES = ("key", "id", "bounces")              # int32 [height, width]
GBUFFER_CHAIN_NAMES = GBUFFER_CHAIN_GUIDE_NAMES + GBUFFER_CHAIN_INT_NAMES + ("depth",)

# LRT_CM_*: the status plane of lrt_gbuffer_chain_motion_*
CM_NOT_FOLLOWED, CM_CONVERGED, CM_UNRESOLVED, CM_NO_SEED, CM_KEY_LOST, CM_NOT_CONVERGED = range(6)
CM_MAX_ITERATIONS = 8       # LRT_CM_MAX_ITERATIONS


class GbufferChainMotionDesc(ctypes.Structure):   # lrt_gbuffer_chain_motion_desc
    _fields_ = [("width", ctypes.c_int32), ("height", ctypes.c_int32),
                ("flags", ctypes.c_int32), ("reserved", ctypes.c_int32),
                ("camera", Camera), ("prev_camera", Camera),
                ("max_bounces", ctypes.c_int32), ("roughness_max", ctypes.c_float),
                ("iterations", ctypes.c_int32), ("probe_px", ctypes.c_float),
                ("step_max_px", ctypes.c_float), ("converged_px", ctypes.c_float),
                ("reserved2", ctypes.c_int32), ("reserved3", ctypes.c_int32)]


class GbufferChainMotion(ctypes.Structure):       # lrt_gbuffer_chain_motion
    _fields_ = [("motion", ctypes.c_void_p), ("status", ctypes.c_void_p)]


GBUFFER_CHAIN_MOTION_NAMES = ("motion", "status")
GBUFFER_CHAIN_MOTION_PARAMS = ("max_bounces", "roughness_max", "iterations", "probe_px", "step_max_px", "converged_px")


class TemporalGbufferDesc(ctypes.Structure):  # lrt_temporal_gbuffer_desc
    _fields_ = [("width", ctypes.c_int32), ("height", ctypes.c_int32),
                ("flags", ctypes.c_int32), ("min_history", ctypes.c_int32),
                ("cur_scale", ctypes.c_float), ("alpha_min", ctypes.c_float), ("normal_min", ctypes.c_float),
                ("short_std", ctypes.c_float), ("reserved", ctypes.c_int32), ("reserved2", ctypes.c_int32)]


TEMPORAL_GBUFFER_PARAMS = ("cur_scale", "alpha_min", "normal_min", "short_std", "min_history")
TEMPORAL_GBUFFER_CUR_NAMES = ("normal", "motion", "id")    # what lrt_temporal_accumulate_gbuffer_* reads of d_cur
TEMPORAL_GBUFFER_PREV_NAMES = ("normal", "id")             # ... of d_prev_g
TEMPORAL_GBUFFER_STATE_NAMES = ("color", "moment2")        # ... and reads or writes of a state
TEMPORAL_GBUFFER_PLANES = ("normal", "world_pos", "albedo", "motion", "id")   # TemporalAccumulator.gbuffer_planes()


UP_BILINEAR = 1       # lrt_upsample_desc.flags: every pixel plain bilinear
UP_MAX_SIZE = 32768


class UpsampleDesc(ctypes.Structure):         # lrt_upsample_desc
    _fields_ = [("width", ctypes.c_int32), ("height", ctypes.c_int32),
                ("low_width", ctypes.c_int32), ("low_height", ctypes.c_int32),
                ("flags", ctypes.c_int32), ("reserved", ctypes.c_int32),
                ("sigma_normal", ctypes.c_float), ("albedo_floor", ctypes.c_float), ("weight_min", ctypes.c_float),
                ("reserved2", ctypes.c_int32)]


UPSAMPLE_PARAMS = ("sigma_normal", "albedo_floor", "weight_min", "flags")
UPSAMPLE_NAMES = ("id", "normal", "albedo")   # what lrt_upsample_* reads of either G-buffer (albedo: both or neither)


class TemporalUpsampleDesc(ctypes.Structure):  # lrt_temporal_upsample_desc
    _fields_ = [("width", ctypes.c_int32), ("height", ctypes.c_int32),
                ("low_width", ctypes.c_int32), ("low_height", ctypes.c_int32),
                ("jitter_x", ctypes.c_int32), ("jitter_y", ctypes.c_int32),
                ("flags", ctypes.c_int32), ("min_history", ctypes.c_int32),
                ("cur_scale", ctypes.c_float), ("alpha_min", ctypes.c_float), ("normal_min", ctypes.c_float),
                ("short_std", ctypes.c_float), ("sigma_normal", ctypes.c_float), ("sigma_sample", ctypes.c_float),
                ("weight_min", ctypes.c_float), ("reserved", ctypes.c_int32)]


TEMPORAL_UPSAMPLE_PARAMS = ("cur_scale", "alpha_min", "normal_min", "short_std", "min_history", "sigma_normal",
                            "sigma_sample", "weight_min", "jitter_x", "jitter_y")
TEMPORAL_UPSAMPLE_LOW_NAMES = ("id", "normal")             # what lrt_temporal_upsample_* reads of d_low


RECTIFY_MAX_RADIUS = 3


class RectifyDesc(ctypes.Structure):          # lrt_rectify_desc
    _fields_ = [("width", ctypes.c_int32), ("height", ctypes.c_int32),
                ("radius", ctypes.c_int32), ("min_taps", ctypes.c_int32),
                ("min_history", ctypes.c_int32), ("flags", ctypes.c_int32),
                ("ref_scale", ctypes.c_float), ("gamma", ctypes.c_float), ("range_floor", ctypes.c_float),
                ("reset_history", ctypes.c_float), ("short_std", ctypes.c_float), ("reserved", ctypes.c_int32)]


RECTIFY_PARAMS = ("radius", "min_taps", "min_history", "ref_scale", "gamma", "range_floor", "reset_history",
                  "short_std")
RECTIFY_INT_PARAMS = ("radius", "min_taps", "min_history")


COUNT_MAX = 4096      # LRT_COUNT_MAX
SB_STD = 1            # lrt_sample_budget_desc.flags: the input plane is a standard deviation
RC_MEAN = 1           # lrt_render_counts.flags: the per-pixel mean factor
RC_CAPACITY_MAX = 1 << 27


class SampleBudgetDesc(ctypes.Structure):     # lrt_sample_budget_desc
    _fields_ = [("width", ctypes.c_int32), ("height", ctypes.c_int32),
                ("flags", ctypes.c_int32), ("reserved", ctypes.c_int32),
                ("min_count", ctypes.c_int32), ("max_count", ctypes.c_int32),
                ("passes", ctypes.c_int32), ("reserved2", ctypes.c_int32),
                ("budget", ctypes.c_int64),
                ("luma_floor", ctypes.c_float), ("weight_max", ctypes.c_float)]


SAMPLE_BUDGET_PARAMS = ("flags", "passes", "luma_floor", "weight_max")


class RenderCounts(ctypes.Structure):         # lrt_render_counts
    _fields_ = [("counts", ctypes.c_void_p), ("capacity", ctypes.c_int64),
                ("flags", ctypes.c_int32), ("reserved", ctypes.c_int32),
                ("info", ctypes.c_void_p)]


FIREFLY_MAX_RADIUS = 2        # LRT_FIREFLY_MAX_RADIUS
FIREFLY_MAX_RANK = 4


class FireflyDesc(ctypes.Structure):          # lrt_firefly_desc
    _fields_ = [("width", ctypes.c_int32), ("height", ctypes.c_int32),
                ("radius", ctypes.c_int32), ("rank", ctypes.c_int32),
                ("min_taps", ctypes.c_int32), ("flags", ctypes.c_int32),
                ("gain", ctypes.c_float), ("floor", ctypes.c_float),
                ("reserved", ctypes.c_int32 * 4)]


FIREFLY_PARAMS = ("radius", "rank", "min_taps", "gain", "floor")
FIREFLY_INT_PARAMS = ("radius", "rank", "min_taps")

FIREFLY_RESTORE_MAX_RADIUS = 4        # LRT_FIREFLY_RESTORE_MAX_RADIUS


class FireflyRestoreDesc(ctypes.Structure):   # lrt_firefly_restore_desc
    _fields_ = [("width", ctypes.c_int32), ("height", ctypes.c_int32),
                ("radius", ctypes.c_int32), ("flags", ctypes.c_int32),
                ("reserved", ctypes.c_int32 * 4)]


FIREFLY_RESTORE_PARAMS = ("radius",)


_c = ctypes
_vp = ctypes.c_void_p
_i = ctypes.c_int
# name -> (restype, argtypes); must cover every function include/lrt.h declares (required)
SIGNATURES = {
    "lrt_initialize": (_i, []),
    "lrt_shutdown": (_i, []),
    "lrt_draw_test": (_i, [_c.c_float, _i, _i, _i, _vp, _c.POINTER(_i)]),
    "lrt_last_error": (_c.c_char_p, []),
    "lrt_version": (_c.c_char_p, []),
    "lrt_initialize_devices": (_i, [_i, _vp, _i]),
    "lrt_device_count": (_i, []),
    "lrt_last_launch": (_c.c_char_p, []),
    "lrt_camera_make": (_i, [Float3, Float3, Float3, _c.c_float, _c.c_float, _c.c_float,
                             _c.c_float, _c.POINTER(Camera)]),
    "lrt_camera_default": (_i, [_i, _i, _c.POINTER(Camera)]),
    "lrt_set_scene": (_i, [_c.POINTER(Sphere), _c.POINTER(Material), _i]),
    "lrt_default_scene": (_i, [_c.POINTER(Sphere), _c.POINTER(Material), _i, _c.POINTER(_i)]),
    "lrt_get_scene": (_i, [_c.POINTER(Sphere), _c.POINTER(Material), _i, _c.POINTER(_i)]),
    "lrt_render_device": (_i, [_c.POINTER(RenderDesc), _vp, _vp, _vp]),
    "lrt_render_device_to_frame": (_i, [_c.POINTER(RenderDesc), _vp, _vp, _vp, _vp]),
    "lrt_ipc_alloc": (_i, [_c.c_size_t, _c.POINTER(_vp), _vp]),
    "lrt_ipc_free": (_i, [_vp]),
    "lrt_ipc_open": (_i, [_vp, _c.POINTER(_vp)]),
    "lrt_ipc_close": (_i, [_vp]),
    "lrt_render_host": (_i, [_c.POINTER(RenderDesc), _vp, _c.POINTER(_c.c_longlong)]),
    "lrt_render_device_ex": (_i, [_c.POINTER(RenderDesc), _vp, _vp, _c.POINTER(Features), _vp]),
    "lrt_render_host_ex": (_i, [_c.POINTER(RenderDesc), _vp, _c.POINTER(_c.c_longlong), _c.POINTER(Features)]),
    "lrt_stream_create": (_i, [_i, _c.POINTER(_vp)]),
    "lrt_stream_destroy": (_i, [_vp]),
    "lrt_host_alloc": (_i, [_c.c_size_t, _c.POINTER(_vp)]),
    "lrt_host_free": (_i, [_vp]),
    "lrt_exchange_bytes": (_i, [_i, _i, _i, _i, _c.POINTER(_c.c_longlong), _c.POINTER(_c.c_longlong)]),
    "lrt_shard_rows": (_i, [_i, _i, _i, _i]),
    "lrt_unshard_rows": (_i, [_vp, _vp, _i, _i, _i, _i, _vp]),
    "lrt_pack_rgb": (_i, [_vp, _vp, _c.c_longlong, _vp]),
    "lrt_unshard_rows_rgb": (_i, [_vp, _vp, _i, _i, _i, _i, _vp]),
    "lrt_present_bgra8": (_i, [_vp, _vp, _i, _i, _vp]),
    "lrt_denoise_default": (_i, [_i, _i, _c.POINTER(DenoiseDesc)]),
    "lrt_denoise_device": (_i, [_c.POINTER(DenoiseDesc), _vp, _c.POINTER(Features), _vp, _vp]),
    "lrt_denoise_host": (_i, [_c.POINTER(DenoiseDesc), _vp, _c.POINTER(Features), _vp]),
    "lrt_temporal_default": (_i, [_i, _i, _c.POINTER(Camera), _c.POINTER(Camera), _c.POINTER(TemporalDesc)]),
    "lrt_temporal_accumulate_device": (_i, [_c.POINTER(TemporalDesc), _vp, _c.POINTER(Features),
                                            _c.POINTER(TemporalState), _c.POINTER(TemporalState), _vp, _vp]),
    "lrt_temporal_accumulate_host": (_i, [_c.POINTER(TemporalDesc), _vp, _c.POINTER(Features),
                                          _c.POINTER(TemporalState), _c.POINTER(TemporalState), _vp]),
    "lrt_temporal_accumulate_moving_device": (_i, [_c.POINTER(TemporalDesc), _c.POINTER(SceneMotion), _vp,
                                                   _c.POINTER(Features), _c.POINTER(TemporalState),
                                                   _c.POINTER(TemporalState), _vp, _vp, _vp]),
    "lrt_temporal_accumulate_moving_host": (_i, [_c.POINTER(TemporalDesc), _c.POINTER(SceneMotion), _vp,
                                                 _c.POINTER(Features), _c.POINTER(TemporalState),
                                                 _c.POINTER(TemporalState), _vp, _vp]),
    "lrt_svgf_default": (_i, [_i, _i, _c.POINTER(SvgfDesc)]),
    "lrt_svgf_filter_device": (_i, [_c.POINTER(SvgfDesc), _vp, _vp, _c.POINTER(Features), _vp, _vp, _vp]),
    "lrt_svgf_filter_host": (_i, [_c.POINTER(SvgfDesc), _vp, _vp, _c.POINTER(Features), _vp, _vp]),
    "lrt_tonemap_default": (_i, [_i, _i, _c.POINTER(TonemapDesc)]),
    "lrt_tonemap_device": (_i, [_c.POINTER(TonemapDesc), _vp, _vp, _vp, _vp, _vp, _vp]),
    "lrt_tonemap_host": (_i, [_c.POINTER(TonemapDesc), _vp, _vp, _vp, _vp, _vp]),
    "lrt_gbuffer_default": (_i, [_i, _i, _c.POINTER(Camera), _c.POINTER(Camera), _c.POINTER(GbufferDesc)]),
    "lrt_gbuffer_device": (_i, [_c.POINTER(GbufferDesc), _c.POINTER(SceneMotion), _c.POINTER(Gbuffer), _vp]),
    "lrt_gbuffer_host": (_i, [_c.POINTER(GbufferDesc), _c.POINTER(SceneMotion), _c.POINTER(Gbuffer)]),
    "lrt_temporal_gbuffer_default": (_i, [_i, _i, _c.POINTER(TemporalGbufferDesc)]),
    "lrt_temporal_accumulate_gbuffer_device": (_i, [_c.POINTER(TemporalGbufferDesc), _vp, _c.POINTER(Gbuffer),
                                                    _c.POINTER(Gbuffer), _c.POINTER(TemporalState),
                                                    _c.POINTER(TemporalState), _vp, _vp]),
    "lrt_temporal_accumulate_gbuffer_host": (_i, [_c.POINTER(TemporalGbufferDesc), _vp, _c.POINTER(Gbuffer),
                                                  _c.POINTER(Gbuffer), _c.POINTER(TemporalState),
                                                  _c.POINTER(TemporalState), _vp]),
    "lrt_upsample_default": (_i, [_i, _i, _i, _i, _c.POINTER(UpsampleDesc)]),
    "lrt_upsample_device": (_i, [_c.POINTER(UpsampleDesc), _vp, _c.POINTER(Gbuffer), _c.POINTER(Gbuffer), _vp, _vp,
                                 _vp]),
    "lrt_upsample_host": (_i, [_c.POINTER(UpsampleDesc), _vp, _c.POINTER(Gbuffer), _c.POINTER(Gbuffer), _vp, _vp]),
    "lrt_temporal_upsample_default": (_i, [_i, _i, _i, _i, _c.POINTER(TemporalUpsampleDesc)]),
    "lrt_camera_jitter": (_i, [_c.POINTER(Camera), _i, _i, _i, _i, _i, _i, _c.POINTER(Camera)]),
    "lrt_temporal_upsample_device": (_i, [_c.POINTER(TemporalUpsampleDesc), _vp, _c.POINTER(Gbuffer),
                                          _c.POINTER(Gbuffer), _c.POINTER(Gbuffer), _c.POINTER(TemporalState),
                                          _c.POINTER(TemporalState), _vp, _vp, _vp]),
    "lrt_temporal_upsample_host": (_i, [_c.POINTER(TemporalUpsampleDesc), _vp, _c.POINTER(Gbuffer),
                                        _c.POINTER(Gbuffer), _c.POINTER(Gbuffer), _c.POINTER(TemporalState),
                                        _c.POINTER(TemporalState), _vp, _vp]),
    "lrt_temporal_rectify_default": (_i, [_i, _i, _c.POINTER(RectifyDesc)]),
    "lrt_temporal_rectify_device": (_i, [_c.POINTER(RectifyDesc), _vp, _vp, _c.POINTER(TemporalState),
                                         _c.POINTER(TemporalState), _vp, _vp, _vp]),
    "lrt_temporal_rectify_host": (_i, [_c.POINTER(RectifyDesc), _vp, _vp, _c.POINTER(TemporalState),
                                       _c.POINTER(TemporalState), _vp, _vp]),
    "lrt_gbuffer_chain_default": (_i, [_i, _i, _c.POINTER(Camera), _c.POINTER(GbufferChainDesc)]),
    "lrt_gbuffer_chain_device": (_i, [_c.POINTER(GbufferChainDesc), _c.POINTER(GbufferChain), _vp]),
    "lrt_gbuffer_chain_host": (_i, [_c.POINTER(GbufferChainDesc), _c.POINTER(GbufferChain)]),
    "lrt_gbuffer_chain_motion_default": (_i, [_i, _i, _c.POINTER(Camera), _c.POINTER(Camera),
                                              _c.POINTER(GbufferChainMotionDesc)]),
    "lrt_gbuffer_chain_motion_device": (_i, [_c.POINTER(GbufferChainMotionDesc), _c.POINTER(SceneMotion), _vp,
                                             _c.POINTER(GbufferChainMotion), _vp]),
    "lrt_gbuffer_chain_motion_host": (_i, [_c.POINTER(GbufferChainMotionDesc), _c.POINTER(SceneMotion), _vp,
                                           _c.POINTER(GbufferChainMotion)]),
    "lrt_sample_budget_default": (_i, [_i, _i, _i, _i, _c.c_longlong, _c.POINTER(SampleBudgetDesc)]),
    "lrt_sample_budget_device": (_i, [_c.POINTER(SampleBudgetDesc), _vp, _vp, _vp, _vp, _vp]),
    "lrt_sample_budget_host": (_i, [_c.POINTER(SampleBudgetDesc), _vp, _vp, _vp, _vp]),
    "lrt_render_counts_device": (_i, [_c.POINTER(RenderDesc), _c.POINTER(RenderCounts), _vp, _vp, _vp]),
    "lrt_render_counts_host": (_i, [_c.POINTER(RenderDesc), _c.POINTER(RenderCounts), _vp,
                                    _c.POINTER(_c.c_longlong)]),
    "lrt_firefly_default": (_i, [_i, _i, _c.POINTER(FireflyDesc)]),
    "lrt_firefly_device": (_i, [_c.POINTER(FireflyDesc), _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "lrt_firefly_host": (_i, [_c.POINTER(FireflyDesc), _vp, _vp, _vp, _vp, _vp, _vp]),
    "lrt_firefly_restore_default": (_i, [_i, _i, _c.POINTER(FireflyRestoreDesc)]),
    "lrt_firefly_restore_device": (_i, [_c.POINTER(FireflyRestoreDesc), _vp, _vp, _vp, _vp, _vp]),
    "lrt_firefly_restore_host": (_i, [_c.POINTER(FireflyRestoreDesc), _vp, _vp, _vp, _vp]),
}
# include/lrt_diag.h: diagnostics and test hooks, bound when the library exports them (the
# product path needs none of them; a build without them still loads)
DIAG_SIGNATURES = {
    "lrt_libm_eval_host": (_i, [_i, _vp, _vp, _c.c_longlong]),
    "lrt_libm_eval_device": (_i, [_i, _vp, _vp, _c.c_longlong]),
    "lrt_exact_div_sweep": (_i, [_i, _c.c_ulonglong, _c.c_ulonglong, _i, _vp]),
    "lrt_rng_form_sweep": (_i, [_i, _vp]),
    "lrt_sphere_roots_eval": (_i, [_vp, _vp, _vp, _vp, _i, _vp, _vp]),
    "lrt_pool_force_pix": (_i, [_i]),
    "lrt_bvh_stats": (_i, [_c.POINTER(Sphere), _i, _vp, _i, _vp]),
    "lrt_grid_stats": (_i, [_c.POINTER(Sphere), _i, _vp, _i, _vp]),
    "lrt_accel_eval": (_i, [_c.POINTER(Sphere), _i, _vp, _i, _i, _i, _vp, _vp]),
    "lrt_kernel_timing": (_i, [_i]),
    "lrt_kernel_times": (_i, [_vp, _i, _vp]),
    "lrt_scatter_eval": (_i, [_c.POINTER(Sphere), _c.POINTER(Material), _i, _vp, _vp, _vp, _vp, _i, _vp, _vp, _vp,
                              _vp, _i]),
}

_lock = threading.Lock()
_lib = None


def lib() -> ctypes.CDLL:
    """Load liblrt_hip.so once; raise LrtError if it is not built."""
    global _lib
    with _lock:
        if _lib is None:
            if not os.path.exists(LIB_PATH):
                raise LrtError(LRT_E_STATE, f"{LIB_PATH} is missing: run __graft_entry__.build() "
                                            "(make -C learnraytracing_amd/csrc)")
            # One HIP runtime per process: torch ships its own libamdhip64 (DT_NEEDED
            # "libamdhip64.so", SONAME libamdhip64.so.7). Importing torch first makes this
            # library's DT_NEEDED libamdhip64.so.7 resolve to that same, already loaded copy;
            # loading /opt/rocm's copy first would leave torch with a second runtime that
            # finds no GPU.
            try:
                import torch  # noqa: F401
            except ImportError:  # pragma: no cover - torch is part of the image
                pass
            try:
                handle = ctypes.CDLL(LIB_PATH)
            except OSError as e:   # pragma: no cover - depends on the box
                raise LrtError(LRT_E_STATE, f"cannot load {LIB_PATH}: {e}") from e
            for name, (res, args) in list(SIGNATURES.items()) + list(DIAG_SIGNATURES.items()):
                fn = getattr(handle, name, None)
                if fn is None and (name in DIAG_SIGNATURES or os.environ.get("LRT_LIB")):
                    continue   # an A/B build of an older revision: entry points it predates stay unbound
                if fn is None:
                    raise LrtError(LRT_E_STATE, f"{LIB_PATH} does not export {name}")
                fn.restype = res
                fn.argtypes = args
            _lib = handle
        return _lib


def last_launch() -> dict:
    """The kernel instance of the last render call (lrt_last_launch) as a dict."""
    words = lib().lrt_last_launch().decode().split()
    return dict(w.split("=", 1) for w in words if "=" in w)


def check(rc: int) -> int:
    """Raise LrtError for a negative LRT_E_* return code."""
    if rc < 0:
        msg = lib().lrt_last_error().decode(errors="replace")
        raise LrtError(rc, msg)
    return rc


def f3(x, y, z) -> Float3:
    return Float3(float(x), float(y), float(z))
