"""Host-side mirror of the reference renderer API (src/cpu/parallel.h:6-8) over the
C-ABI, plus the device-resident render used by the benchmark and the multi-GPU path.

Reference API (same names, same argument meaning):
    InitializeTest()                                  parallel.cpp:231-235
    ShutdownTest()                                    parallel.cpp:237-240
    DrawTest(time, frameCount, screenWidth, screenHeight, backbuffer) -> rayCount
                                                      parallel.cpp:297-323
`backbuffer` is a float32 array of screenWidth*screenHeight*4 (RGBA stride, row 0 at
the bottom); DrawTest adds one progressive sample per pixel exactly as the reference's
TraceRowJob does (kMaxDepth 20), but every pixel-sample owns its XorShift32 stream
(seed (x*1973 + y*9277 + frameCount*26699) | 1) instead of the reference's shared,
racy global one (maths.cpp:5), so the output is deterministic.

Error behaviour: the reference returns void and has no argument checks (bad sizes are
undefined behaviour). Here every failure raises LrtError with the library's message.
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass
from typing import Optional, Sequence

import numpy as np

from . import _buffers as B
from . import _lib as L


# ---- the reference API ---------------------------------------------------------------
def InitializeTest() -> None:
    L.check(L.lib().lrt_initialize())


def ShutdownTest() -> None:
    L.check(L.lib().lrt_shutdown())


def InitializeDevices(device_ids: Optional[Sequence[int]] = None, peer_copy: bool = False,
                      gather: bool = False) -> None:
    """InitializeTest over several GPUs of this process (lrt_initialize_devices): DrawTest and
    render_host then split the rows over all of them; each device copies its rows back to the
    caller's buffer itself, or with gather=True they are gathered into the first device by RCCL
    (device-to-device copies when an id repeats, or with peer_copy). None: every visible GPU."""
    flags = (L.DEV_PEER_COPY if peer_copy else 0) | (L.DEV_GATHER if gather else 0)
    if device_ids is None:
        L.check(L.lib().lrt_initialize_devices(0, None, flags))
        return
    ids = (ctypes.c_int * len(device_ids))(*[int(i) for i in device_ids])
    L.check(L.lib().lrt_initialize_devices(len(device_ids), ctypes.cast(ids, ctypes.c_void_p), flags))


def device_count() -> int:
    return int(L.lib().lrt_device_count())


def DrawTest(time: float, frameCount: int, screenWidth: int, screenHeight: int,
             backbuffer: np.ndarray) -> int:
    """The reference's DrawTest (parallel.h:8): one progressive frame into the caller's
    float RGBA backbuffer (any host memory; a pageable array is page-locked for the call
    only). Returns the rays counted (outRayCount)."""
    B.HostBuffers().check(backbuffer, "backbuffer", screenWidth * screenHeight * 4)
    rays = ctypes.c_int(0)
    L.check(L.lib().lrt_draw_test(float(time), int(frameCount), int(screenWidth), int(screenHeight),
                                  backbuffer.ctypes.data_as(ctypes.c_void_p), ctypes.byref(rays)))
    return rays.value


# ---- extended API -----------------------------------------------------------------------
def default_camera(width: int, height: int) -> L.Camera:
    cam = L.Camera()
    L.check(L.lib().lrt_camera_default(int(width), int(height), ctypes.byref(cam)))
    return cam


def make_camera(look_from, look_at, vup, vfov, aspect, aperture, focus_dist) -> L.Camera:
    cam = L.Camera()
    L.check(L.lib().lrt_camera_make(L.f3(*look_from), L.f3(*look_at), L.f3(*vup), float(vfov),
                                    float(aspect), float(aperture), float(focus_dist), ctypes.byref(cam)))
    return cam


def set_scene(spheres: Sequence[L.Sphere], materials: Sequence[L.Material]) -> None:
    n = len(spheres)
    if n != len(materials):
        raise L.LrtError(L.LRT_E_INVALID, "spheres and materials differ in length")
    sa = (L.Sphere * max(n, 1))(*spheres)
    ma = (L.Material * max(n, 1))(*materials)
    L.check(L.lib().lrt_set_scene(sa, ma, n))


def get_scene():
    """(spheres, materials) the devices hold now (lrt_get_scene)."""
    n = ctypes.c_int(0)
    rc = L.lib().lrt_get_scene(None, None, 0, ctypes.byref(n))
    if rc != 0 and n.value == 0:
        L.check(rc)
    sa = (L.Sphere * max(n.value, 1))()
    ma = (L.Material * max(n.value, 1))()
    L.check(L.lib().lrt_get_scene(sa, ma, n.value, ctypes.byref(n)))
    return list(sa)[: n.value], list(ma)[: n.value]


def shard_rows(height: int, row_block: int, period: int, phase: int) -> int:
    return L.check(L.lib().lrt_shard_rows(int(height), int(row_block), int(period), int(phase)))


@dataclass
class Job:
    """One render call (lrt_render_desc). Rows are local; see include/lrt.h."""
    width: int
    height: int
    frame0: int = 0
    frames: int = 1
    max_depth: int = 8
    x0: int = 0
    x_count: Optional[int] = None
    y0: int = 0
    row_count: Optional[int] = None
    row_block: Optional[int] = None
    row_period: int = 1
    row_phase: int = 0
    camera: Optional[L.Camera] = None
    flags: int = 0

    def desc(self) -> L.RenderDesc:
        d = L.RenderDesc()
        d.camera = self.camera if self.camera is not None else default_camera(self.width, self.height)
        d.width, d.height = self.width, self.height
        d.x0 = self.x0
        d.x_count = self.width - self.x0 if self.x_count is None else self.x_count
        d.y0 = self.y0
        rb = self.row_block if self.row_block is not None else max(1, self.height)
        d.row_block, d.row_period, d.row_phase = rb, self.row_period, self.row_phase
        if self.row_count is None:
            if self.row_period == 1:
                d.row_count = self.height - self.y0
            else:
                d.row_count = shard_rows(self.height - self.y0, rb, self.row_period, self.row_phase)
        else:
            d.row_count = self.row_count
        d.frame0, d.frames, d.max_depth, d.flags = self.frame0, self.frames, self.max_depth, self.flags
        return d


def pinned_backbuffer(n_floats: int) -> np.ndarray:
    """A zeroed float32 host array in page-locked memory (a torch pin_memory tensor viewed
    by numpy; the array keeps the tensor alive). DrawTest / render_host detect such buffers:
    the colours are rendered while the previous values come in by DMA, and the lerp writes
    the result straight into the buffer over PCIe (LRT_HOST_PIPELINE=0: the kernel reads and
    writes the buffer in place; LRT_HOST_ZEROCOPY=0: staged like pageable memory)."""
    import torch
    return torch.zeros(int(n_floats), dtype=torch.float32, pin_memory=True).numpy()


def render_host(job: Job, backbuffer: np.ndarray) -> int:
    """Render `job` into a host float32 buffer (row_count*x_count*4). Returns rays."""
    d = job.desc()
    B.HostBuffers().check(backbuffer, "backbuffer", d.row_count * d.x_count * 4)
    rays = ctypes.c_longlong(0)
    L.check(L.lib().lrt_render_host(ctypes.byref(d), backbuffer.ctypes.data_as(ctypes.c_void_p),
                                    ctypes.byref(rays)))
    return rays.value


def render_host_features(job: Job, backbuffer: np.ndarray, features: dict, max_frame: int = 4) -> int:
    """render_host plus the GL path's first-hit features (lrt_render_host_ex): `features`
    maps names of lrt_features ("normal", "world_pos", "albedo", "color_std", "normal_std",
    "world_pos_std") to host float32 buffers shaped like the backbuffer, updated in place
    for frames <= max_frame (< 0: all). Returns rays."""
    d = job.desc()
    n = d.row_count * d.x_count * 4
    B.HostBuffers().check(backbuffer, "backbuffer", n)
    f = _features(B.HostBuffers(), features, n, L.FEATURE_NAMES, "feature")
    f.max_frame = int(max_frame)
    rays = ctypes.c_longlong(0)
    L.check(L.lib().lrt_render_host_ex(ctypes.byref(d), backbuffer.ctypes.data_as(ctypes.c_void_p),
                                       ctypes.byref(rays), ctypes.byref(f)))
    return rays.value


def render_device(job: Job, buf_ptr: int, rays_ptr: int, stream_ptr: int = 0) -> None:
    """Asynchronous render into device memory (raw pointers, e.g. torch's data_ptr())."""
    d = job.desc()
    L.check(L.lib().lrt_render_device(ctypes.byref(d), ctypes.c_void_p(buf_ptr), ctypes.c_void_p(rays_ptr),
                                      ctypes.c_void_p(stream_ptr)))


def render_tensor(job: Job, buf, rays, stream=None) -> None:
    """torch front end of render_device: buf is a cuda float32 tensor with
    row_count*x_count*4 elements, rays a cuda int64 tensor with >= 1 element
    (incremented by the counted rays), stream a torch.cuda.Stream (default: current)."""
    import torch

    d = job.desc()
    need = d.row_count * d.x_count * 4
    if not (buf.is_cuda and buf.dtype == torch.float32 and buf.is_contiguous() and buf.numel() >= need):
        raise L.LrtError(L.LRT_E_INVALID, f"buf must be a contiguous cuda float32 tensor of >= {need} elements")
    if not (rays.is_cuda and rays.dtype == torch.int64 and rays.numel() >= 1):
        raise L.LrtError(L.LRT_E_INVALID, "rays must be a cuda int64 tensor")
    s = stream if stream is not None else torch.cuda.current_stream(buf.device)
    L.check(L.lib().lrt_render_device(ctypes.byref(d), ctypes.c_void_p(buf.data_ptr()),
                                      ctypes.c_void_p(rays.data_ptr()), ctypes.c_void_p(s.cuda_stream)))


def render_tensor_to_frame(job: Job, buf, rays, frame_ptr: int, stream=None) -> None:
    """render_tensor plus the fused frame exchange (lrt_render_device_to_frame): each finished
    pixel is also stored into the width x height RGBA frame at frame_ptr (a device pointer,
    e.g. rank 0's frame opened over IPC) at its global row."""
    import torch

    d = job.desc()
    need = d.row_count * d.x_count * 4
    if not (buf.is_cuda and buf.dtype == torch.float32 and buf.is_contiguous() and buf.numel() >= need):
        raise L.LrtError(L.LRT_E_INVALID, f"buf must be a contiguous cuda float32 tensor of >= {need} elements")
    if not (rays.is_cuda and rays.dtype == torch.int64 and rays.numel() >= 1):
        raise L.LrtError(L.LRT_E_INVALID, "rays must be a cuda int64 tensor")
    s = stream if stream is not None else torch.cuda.current_stream(buf.device)
    L.check(L.lib().lrt_render_device_to_frame(ctypes.byref(d), ctypes.c_void_p(buf.data_ptr()),
                                               ctypes.c_void_p(rays.data_ptr()), ctypes.c_void_p(int(frame_ptr)),
                                               ctypes.c_void_p(s.cuda_stream)))


class RenderStream:
    """A CU-masked render stream (lrt_stream_create) leaving `reserved_cus` CUs free for
    concurrent work such as RCCL collectives; `.torch` is the torch.cuda.ExternalStream."""

    def __init__(self, reserved_cus: int):
        import torch

        h = ctypes.c_void_p()
        L.check(L.lib().lrt_stream_create(int(reserved_cus), ctypes.byref(h)))
        self.handle = h.value
        self.torch = torch.cuda.ExternalStream(self.handle)

    def close(self) -> None:
        if self.handle:
            L.check(L.lib().lrt_stream_destroy(ctypes.c_void_p(self.handle)))
            self.handle = None


def unshard_tensor(gathered, out, width: int, height: int, row_block: int, period: int, stream=None) -> None:
    """Frame assembly (lrt_unshard_rows) on cuda tensors."""
    import torch

    s = stream if stream is not None else torch.cuda.current_stream(out.device)
    L.check(L.lib().lrt_unshard_rows(ctypes.c_void_p(gathered.data_ptr()), ctypes.c_void_p(out.data_ptr()),
                                     int(width), int(height), int(row_block), int(period),
                                     ctypes.c_void_p(s.cuda_stream)))


def pack_rgb_tensor(rgba, rgb, stream=None) -> None:
    """RGBA quads -> packed RGB triples (lrt_pack_rgb) on cuda tensors: the shard a rank
    sends in the frame exchange."""
    import torch

    if rgba.numel() // 4 != rgb.numel() // 3:
        raise ValueError("pack_rgb: rgba and rgb must hold the same pixels")
    s = stream if stream is not None else torch.cuda.current_stream(rgba.device)
    L.check(L.lib().lrt_pack_rgb(ctypes.c_void_p(rgba.data_ptr()), ctypes.c_void_p(rgb.data_ptr()),
                                 int(rgba.numel() // 4), ctypes.c_void_p(s.cuda_stream)))


def unshard_rgb_tensor(gathered_rgb, out, width: int, height: int, row_block: int, period: int, stream=None) -> None:
    """Frame assembly from packed RGB shards (lrt_unshard_rows_rgb); out's alpha untouched."""
    import torch

    s = stream if stream is not None else torch.cuda.current_stream(out.device)
    L.check(L.lib().lrt_unshard_rows_rgb(ctypes.c_void_p(gathered_rgb.data_ptr()), ctypes.c_void_p(out.data_ptr()),
                                         int(width), int(height), int(row_block), int(period),
                                         ctypes.c_void_p(s.cuda_stream)))


def present_tensor(rgba, bgra, width: int, height: int, stream=None) -> None:
    """LinearToSRGB + BGRA8 pack (main.cpp:109-141) on cuda tensors."""
    import torch

    s = stream if stream is not None else torch.cuda.current_stream(rgba.device)
    L.check(L.lib().lrt_present_bgra8(ctypes.c_void_p(rgba.data_ptr()), ctypes.c_void_p(bgra.data_ptr()),
                                      int(width), int(height), ctypes.c_void_p(s.cuda_stream)))


def render_tensor_features(job: Job, buf, rays, features: dict, max_frame: int = 4, stream=None) -> None:
    """torch front end of lrt_render_device_ex: render_tensor plus the first-hit features.
    `features` maps names of lrt_features to cuda float32 tensors shaped like buf, updated in
    place for frames <= max_frame (< 0: all), so that render -> denoise -> present stays on
    the device."""
    import torch

    d = job.desc()
    need = d.row_count * d.x_count * 4
    if not (buf.is_cuda and buf.dtype == torch.float32 and buf.is_contiguous() and buf.numel() >= need):
        raise L.LrtError(L.LRT_E_INVALID, f"buf must be a contiguous cuda float32 tensor of >= {need} elements")
    if not (rays.is_cuda and rays.dtype == torch.int64 and rays.numel() >= 1):
        raise L.LrtError(L.LRT_E_INVALID, "rays must be a cuda int64 tensor")
    s = stream if stream is not None else torch.cuda.current_stream(buf.device)
    f = _features(B.TensorBuffers(buf.device, s), features, need, L.FEATURE_NAMES, "feature")
    f.max_frame = int(max_frame)
    L.check(L.lib().lrt_render_device_ex(ctypes.byref(d), ctypes.c_void_p(buf.data_ptr()),
                                         ctypes.c_void_p(rays.data_ptr()), ctypes.byref(f),
                                         ctypes.c_void_p(s.cuda_stream)))


# ---- what the post-process front ends share ------------------------------------------------
# Each unit below has one body taking a back end of _buffers.py (`bufs`: NumPy arrays -> lrt_*_host,
# cuda tensors -> lrt_*_device on a stream); its *_host and *_tensor size the frame, fill the desc and
# construct the back end.
def _override(d, params: dict, allowed, int_names, what: str):
    """The desc `d` with the caller's `params` set over its defaults."""
    for name, v in params.items():
        if name not in allowed:
            raise L.LrtError(L.LRT_E_INVALID, f"unknown {what} parameter {name!r}")
        setattr(d, name, int(v) if name in int_names else float(v))
    return d


def _kinds(width: int, height: int, words=("id",), scalars=("depth",)) -> dict:
    """B.planes of a width x height frame, plus the names of the planes that are not RGBA quads: an
    int32 word per pixel for those in `words`, a float for those in `scalars`."""
    k = B.planes(width, height)
    for name in words:
        k[name] = k["word"]
    for name in scalars:
        k[name] = k["scalar"]
    return k


def _members(bufs, given, struct, kinds: dict, *, known, stored, noun: str, need=(), what: str = ""):
    """A dict of buffers as the ctypes `struct` of their addresses. `given` (called `what` in messages)
    must hold the names in `need` and may hold any in `known`, so that a whole G-buffer or a returned
    state passes as it is; only the members in `stored` are checked, as their plane of _kinds(), and
    stored."""
    quad = kinds["quad"]
    for name in need:
        if not isinstance(given, dict) or name not in given:
            raise L.LrtError(L.LRT_E_INVALID, f"{what} lacks {name!r}: it must hold " + " and ".join(need))
    st = struct()
    for name, buf in given.items():
        if name not in known:
            raise L.LrtError(L.LRT_E_INVALID, f"unknown {noun} {name!r}")
        if name in stored:
            bufs.check_plane(buf, f"{what} {name}" if what else name, kinds.get(name, quad))
            setattr(st, name, bufs.address(buf))
    return st


def _features(bufs, given: dict, n: int, known, noun: str, stored=None) -> L.Features:
    """lrt_features over float32 buffers of >= n elements, keyed by its member names."""
    every = {"quad": (n, ("float32",), None)}        # (no other kind of plane among the features)
    return _members(bufs, given, L.Features, every, known=known, stored=known if stored is None else stored, noun=noun)


def _color_std(bufs, out: dict, quad):
    """The address of a state's optional color_std, or None."""
    if "color_std" not in out:
        return None
    bufs.check_plane(out["color_std"], "out color_std", quad)
    return bufs.ptr(out["color_std"])


def _moved(spheres, prev_spheres):
    """The lrt_scene_motion argument of the units that take a previous scene: None without one."""
    if prev_spheres is not None:
        return ctypes.byref(_scene_motion(spheres if spheres is not None else get_scene()[0], prev_spheres))
    if spheres is not None:
        raise L.LrtError(L.LRT_E_INVALID, "spheres needs prev_spheres")
    return None


# ---- denoiser ---------------------------------------------------------------------------
def denoise_desc(width: int, height: int, **params) -> L.DenoiseDesc:
    """lrt_denoise_default for a width x height frame, with any of iterations, sigma_color,
    sigma_normal, sigma_pos, sigma_albedo overridden."""
    d = L.DenoiseDesc()
    L.check(L.lib().lrt_denoise_default(int(width), int(height), ctypes.byref(d)))
    return _override(d, params, ("iterations", "sigma_color", "sigma_normal", "sigma_pos", "sigma_albedo"),
                     ("iterations",), "denoise")


def _frame_size(color, params: dict):
    """(width, height) of a [height, width, 4] frame, or the width= / height= given for a flat one."""
    w, h = params.pop("width", None), params.pop("height", None)
    if w is None or h is None:
        if len(color.shape) != 3 or color.shape[2] != 4:
            raise L.LrtError(L.LRT_E_INVALID, "color must be [height, width, 4], or pass width= and height=")
        h, w = int(color.shape[0]), int(color.shape[1])
    return int(w), int(h)


def _denoise(bufs, d, color, guides, out):
    n = d.width * d.height * 4
    bufs.check(color, "color", n)
    if out is None:
        out = bufs.copy(color)
    bufs.check(out, "out", n)
    f = _features(bufs, guides or {}, n, L.GUIDE_NAMES, "guide")
    L.check(bufs.entry("denoise")(ctypes.byref(d), bufs.ptr(color), ctypes.byref(f) if guides else None,
                                  bufs.ptr(out), *bufs.tail))
    return out


def denoise_host(color: np.ndarray, guides: Optional[dict], out: Optional[np.ndarray] = None, **params):
    """Filter a rendered frame with the feature-guided a-trous denoiser (lrt_denoise_host).
    color: float32 [height, width, 4] (or flat with width=, height=); guides: {name: buffer}
    with the lrt_features names "normal", "world_pos", "albedo", "color_std" (a missing one
    drops its term; None or {}: no guides), as render_host_features fills them. out: the
    destination (may be color; only its rgb is written), default a copy of color. params:
    iterations, sigma_color, sigma_normal, sigma_pos, sigma_albedo. Returns out."""
    params = dict(params)
    w, h = _frame_size(color, params)
    return _denoise(B.HostBuffers(), denoise_desc(w, h, **params), color, guides, out)


def denoise_tensor(color, guides: Optional[dict], out=None, stream=None, **params):
    """denoise_host on cuda float32 tensors (lrt_denoise_device): asynchronous on `stream` (a
    torch.cuda.Stream, default: current) and ordered only against it. Returns out."""
    params = dict(params)
    w, h = _frame_size(color, params)
    d = denoise_desc(w, h, **params)
    return _denoise(B.tensor_buffers(color, "color", w * h * 4, stream), d, color, guides, out)


# ---- temporal reprojection and accumulation ------------------------------------------------
def temporal_desc(width: int, height: int, camera: L.Camera, prev_camera: Optional[L.Camera] = None,
                  **params) -> L.TemporalDesc:
    """lrt_temporal_default for a width x height frame seen from `camera`, the previous frame from
    `prev_camera` (None: the same camera), with any of cur_scale, alpha_min, normal_min, pos_tol,
    short_std, min_history overridden."""
    if not isinstance(camera, L.Camera) or not (prev_camera is None or isinstance(prev_camera, L.Camera)):
        raise L.LrtError(L.LRT_E_INVALID, "camera and prev_camera must be Camera structs")
    d = L.TemporalDesc()
    L.check(L.lib().lrt_temporal_default(int(width), int(height), ctypes.byref(camera),
                                         ctypes.byref(prev_camera) if prev_camera is not None else None,
                                         ctypes.byref(d)))
    return _override(d, params, L.TEMPORAL_PARAMS, ("min_history",), "temporal")


def _temporal(bufs, unit, head, color, cur, prev, out, motion=()):
    """The step's marshalling. head: (desc,) or (desc, scene motion), by reference; motion: the moving
    form's (motion,). Returns the new state."""
    k = _kinds(head[0].width, head[0].height)
    quad = k["quad"]
    for buf in motion:                       # (ahead of color, as the moving form always checked it)
        if buf is not None:
            bufs.check_plane(buf, "motion", quad)
    bufs.check_plane(color, "color", quad)
    f = _members(bufs, cur, L.Features, k, what="cur", need=("normal", "world_pos"), known=L.TEMPORAL_CUR_NAMES,
                 stored=L.TEMPORAL_CUR_NAMES, noun="feature")
    # (a returned state may be passed back as it is: its color_std is not read)
    known = L.TEMPORAL_STATE_NAMES + ("color_std",)
    ps = None
    if prev is not None:
        ps = _members(bufs, prev, L.TemporalState, k, what="prev", need=L.TEMPORAL_STATE_NAMES[:4], known=known,
                      stored=L.TEMPORAL_STATE_NAMES, noun="state buffer")
    if out is None:
        out = {name: bufs.new(quad) for name in L.TEMPORAL_STATE_NAMES[:4] + ("color_std",)}
        if "albedo" in cur:
            out["albedo"] = bufs.new(quad)
    ns = _members(bufs, out, L.TemporalState, k, what="out", need=L.TEMPORAL_STATE_NAMES[:4], known=known,
                  stored=L.TEMPORAL_STATE_NAMES, noun="state buffer")
    L.check(bufs.entry(unit)(*(ctypes.byref(a) for a in head), bufs.ptr(color), ctypes.byref(f),
                             ctypes.byref(ps) if ps is not None else None, ctypes.byref(ns),
                             _color_std(bufs, out, quad), *(bufs.ptr(m) for m in motion), *bufs.tail))
    return out


def temporal_accumulate_host(color: np.ndarray, cur: dict, prev: Optional[dict], camera: L.Camera,
                             prev_camera: Optional[L.Camera] = None, out: Optional[dict] = None, **params) -> dict:
    """One temporal accumulation step on host buffers (lrt_temporal_accumulate_host). color: the
    current frame, float32 [height, width, 4] (or flat with width=, height=); cur: its features
    {"normal", "world_pos"[, "albedo"]} as render_host_features fills them; prev: the state a
    previous call returned, or None for no history; camera / prev_camera: this frame's and the
    previous frame's camera. out: the destination buffers {"color", "moment2", "normal",
    "world_pos"[, "albedo"][, "color_std"]} (none may be an input or a prev buffer; the alphas of
    color and color_std stay), default new zeroed ones. params: cur_scale, alpha_min, normal_min,
    pos_tol, short_std, min_history. Returns the new state (out), color_std included."""
    params = dict(params)
    w, h = _frame_size(color, params)
    d = temporal_desc(w, h, camera, prev_camera, **params)
    return _temporal(B.HostBuffers(), "temporal_accumulate", (d,), color, cur, prev, out)


def temporal_accumulate_tensor(color, cur: dict, prev: Optional[dict], camera: L.Camera,
                               prev_camera: Optional[L.Camera] = None, out: Optional[dict] = None, stream=None,
                               **params) -> dict:
    """temporal_accumulate_host on cuda float32 tensors (lrt_temporal_accumulate_device):
    asynchronous on `stream` (a torch.cuda.Stream, default: current) and ordered only against it.
    Returns the new state."""
    params = dict(params)
    w, h = _frame_size(color, params)
    d = temporal_desc(w, h, camera, prev_camera, **params)
    bufs = B.tensor_buffers(color, "color", w * h * 4, stream)
    return _temporal(bufs, "temporal_accumulate", (d,), color, cur, prev, out)


def _sphere_array(spheres, what):
    """A scene as a ctypes Sphere array: a sequence of Sphere structs, or floats [count, 4]
    (centre, radius)."""
    if isinstance(spheres, ctypes.Array) and spheres._type_ is L.Sphere:
        return spheres
    if len(spheres) < 1:
        raise L.LrtError(L.LRT_E_INVALID, f"{what} is empty")
    if isinstance(spheres, np.ndarray) or (len(spheres) and not isinstance(spheres[0], L.Sphere)):
        a = np.ascontiguousarray(spheres, np.float32)
        if a.ndim != 2 or a.shape[1] != 4:
            raise L.LrtError(L.LRT_E_INVALID, f"{what} must be Sphere structs or floats [count, 4]")
        return (L.Sphere * max(len(a), 1)).from_buffer_copy(a.tobytes() if len(a) else bytes(16))
    return (L.Sphere * max(len(spheres), 1))(*spheres)


def _scene_motion(spheres, prev_spheres) -> L.SceneMotion:
    """lrt_scene_motion of two scenes of the same spheres in the same order (it keeps them alive)."""
    n = len(spheres)
    if prev_spheres is None or len(prev_spheres) != n:
        raise L.LrtError(L.LRT_E_INVALID, "spheres and prev_spheres differ in length")
    sm = L.SceneMotion()
    sm._arrays = (_sphere_array(spheres, "spheres"), _sphere_array(prev_spheres, "prev_spheres"))
    sm.spheres = ctypes.cast(sm._arrays[0], ctypes.POINTER(L.Sphere))
    sm.prev_spheres = ctypes.cast(sm._arrays[1], ctypes.POINTER(L.Sphere))
    sm.count = n
    return sm


def temporal_accumulate_moving_host(color: np.ndarray, cur: dict, prev: Optional[dict], camera: L.Camera,
                                    prev_camera: Optional[L.Camera], spheres, prev_spheres,
                                    out: Optional[dict] = None, motion: Optional[np.ndarray] = None,
                                    **params) -> dict:
    """temporal_accumulate_host under moving spheres (lrt_temporal_accumulate_moving_host).
    spheres: the scene the current frame was rendered with, prev_spheres: the scene of the frame
    behind `prev` -- Sphere structs or floats [count, 4], the same spheres in the same order.
    motion: a float32 [height, width, 4] buffer for the motion vectors (x, y: previous minus current
    position in pixels; z: the matched sphere or -1; w: 1 if projectable), or None for none."""
    params = dict(params)
    w, h = _frame_size(color, params)
    d = temporal_desc(w, h, camera, prev_camera, **params)
    sm = _scene_motion(spheres, prev_spheres)
    return _temporal(B.HostBuffers(), "temporal_accumulate_moving", (d, sm), color, cur, prev, out, (motion,))


def temporal_accumulate_moving_tensor(color, cur: dict, prev: Optional[dict], camera: L.Camera,
                                      prev_camera: Optional[L.Camera], spheres, prev_spheres,
                                      out: Optional[dict] = None, motion=None, stream=None, **params) -> dict:
    """temporal_accumulate_moving_host on cuda float32 tensors (lrt_temporal_accumulate_moving_device):
    asynchronous on `stream` and ordered only against it; the sphere arrays are read before it
    returns. motion: a cuda tensor [height, width, 4], or None."""
    params = dict(params)
    w, h = _frame_size(color, params)
    d = temporal_desc(w, h, camera, prev_camera, **params)
    sm = _scene_motion(spheres, prev_spheres)
    bufs = B.tensor_buffers(color, "color", w * h * 4, stream)
    return _temporal(bufs, "temporal_accumulate_moving", (d, sm), color, cur, prev, out, (motion,))


def temporal_gbuffer_desc(width: int, height: int, **params) -> L.TemporalGbufferDesc:
    """lrt_temporal_gbuffer_default for a width x height frame, with any of cur_scale, alpha_min,
    normal_min, short_std, min_history overridden."""
    d = L.TemporalGbufferDesc()
    L.check(L.lib().lrt_temporal_gbuffer_default(int(width), int(height), ctypes.byref(d)))
    return _override(d, params, L.TEMPORAL_GBUFFER_PARAMS, ("min_history",), "temporal")


def _gbuffer_planes(bufs, given, what, need, kinds, stored=None) -> L.Gbuffer:
    """lrt_gbuffer of the planes a unit reads of a G-buffer (a whole one may be passed: the rest is not
    read): those in `stored`, by default the `need`ed ones."""
    return _members(bufs, given, L.Gbuffer, kinds, what=what, need=need, known=L.GBUFFER_NAMES,
                    stored=need if stored is None else stored, noun="G-buffer plane")


def _gbuffer_state(bufs, given, what, known, kinds) -> L.TemporalState:
    """lrt_temporal_state of the color and moment2 of a state of the G-buffer-driven units."""
    return _members(bufs, given, L.TemporalState, kinds, what=what, need=L.TEMPORAL_GBUFFER_STATE_NAMES,
                    known=known + ("color_std",), stored=L.TEMPORAL_GBUFFER_STATE_NAMES, noun="state buffer")


def _new_gbuffer_state(bufs, quad) -> dict:
    return {name: bufs.new(quad) for name in L.TEMPORAL_GBUFFER_STATE_NAMES + ("color_std",)}


def _byref(st):
    return ctypes.byref(st) if st is not None else None


def _temporal_gbuffer(bufs, d, color, cur, prev_g, prev, out):
    k = _kinds(d.width, d.height)
    quad = k["quad"]
    bufs.check_plane(color, "color", quad)
    gc = _gbuffer_planes(bufs, cur, "cur", L.TEMPORAL_GBUFFER_CUR_NAMES, k)
    gp = _gbuffer_planes(bufs, prev_g, "prev_g", L.TEMPORAL_GBUFFER_PREV_NAMES, k) if prev_g is not None else None
    # (a returned state, or an accumulator's, may be passed back as it is: only color and moment2 are read)
    ps = _gbuffer_state(bufs, prev, "prev", L.TEMPORAL_STATE_NAMES, k) if prev is not None else None
    if out is None:
        out = _new_gbuffer_state(bufs, quad)
    ns = _gbuffer_state(bufs, out, "out", L.TEMPORAL_GBUFFER_STATE_NAMES, k)
    L.check(bufs.entry("temporal_accumulate_gbuffer")(ctypes.byref(d), bufs.ptr(color), ctypes.byref(gc), _byref(gp),
                                                      _byref(ps), ctypes.byref(ns), _color_std(bufs, out, quad),
                                                      *bufs.tail))
    return out


def temporal_accumulate_gbuffer_host(color: np.ndarray, cur: dict, prev_g: Optional[dict], prev: Optional[dict],
                                     out: Optional[dict] = None, **params) -> dict:
    """One temporal accumulation step driven by the G-buffer, on host buffers
    (lrt_temporal_accumulate_gbuffer_host). color: the current frame, float32 [height, width, 4] (or
    flat with width=, height=); cur: its G-buffer {"normal", "motion", "id"[, ...]} as
    gbuffer_host(id=True, motion=True) returns it at guide_scale 1 (id int32, the rest float32; the
    other planes are not read); prev_g: the previous frame's G-buffer {"normal", "id"[, ...]} and
    prev: the state {"color", "moment2"[, ...]} a previous call returned -- both, or None and None for
    no history. out: the destination buffers {"color", "moment2"[, "color_std"]} (none may be an
    input or a previous buffer; the alphas of color and color_std stay), default new zeroed ones.
    params: cur_scale (the colour's only), alpha_min, normal_min, short_std, min_history. Returns the
    new state (out)."""
    params = dict(params)
    w, h = _frame_size(color, params)
    d = temporal_gbuffer_desc(w, h, **params)
    return _temporal_gbuffer(B.HostBuffers(), d, color, cur, prev_g, prev, out)


def temporal_accumulate_gbuffer_tensor(color, cur: dict, prev_g: Optional[dict], prev: Optional[dict],
                                       out: Optional[dict] = None, stream=None, **params) -> dict:
    """temporal_accumulate_gbuffer_host on cuda tensors (lrt_temporal_accumulate_gbuffer_device):
    asynchronous on `stream` (a torch.cuda.Stream, default: current) and ordered only against it.
    "id" is an int32 tensor, the others float32. Returns the new state."""
    params = dict(params)
    w, h = _frame_size(color, params)
    d = temporal_gbuffer_desc(w, h, **params)
    bufs = B.tensor_buffers(color, "color", w * h * 4, stream)
    return _temporal_gbuffer(bufs, d, color, cur, prev_g, prev, out)


# ---- history rectification -----------------------------------------------------------------
def temporal_rectify_desc(width: int, height: int, **params) -> L.RectifyDesc:
    """lrt_temporal_rectify_default for a width x height frame, with any of radius, min_taps,
    min_history, ref_scale, gamma, range_floor, reset_history, short_std overridden."""
    d = L.RectifyDesc()
    L.check(L.lib().lrt_temporal_rectify_default(int(width), int(height), ctypes.byref(d)))
    return _override(d, params, L.RECTIFY_PARAMS, L.RECTIFY_INT_PARAMS, "rectify")


def _temporal_rectify(bufs, d, ref, ids, state, out, class_out):
    k = _kinds(d.width, d.height)
    quad, word = k["quad"], k["word"]
    bufs.check_plane(ref, "ref", quad)
    bufs.check_plane(ids, "id", word)
    # (a returned state, or an accumulator's, may be passed as it is: only color and moment2 are read)
    ss = _gbuffer_state(bufs, state, "state", L.TEMPORAL_STATE_NAMES, k)
    if out is None:
        out = _new_gbuffer_state(bufs, quad)
    # out=state is in place: the state's other members are left alone (its color_std, if any, is refreshed)
    ns = _gbuffer_state(bufs, out, "out", L.TEMPORAL_STATE_NAMES if out is state else L.TEMPORAL_GBUFFER_STATE_NAMES,
                        k)
    std = _color_std(bufs, out, quad)
    if class_out is not None:
        bufs.check_plane(class_out, "class_out", word)
    L.check(bufs.entry("temporal_rectify")(ctypes.byref(d), bufs.ptr(ref), bufs.ptr(ids), ctypes.byref(ss),
                                           ctypes.byref(ns), std, bufs.ptr(class_out), *bufs.tail))
    return out


def temporal_rectify_host(ref: np.ndarray, id: np.ndarray, state: dict, out: Optional[dict] = None,
                          class_out: Optional[np.ndarray] = None, **params) -> dict:
    """Hold a temporal state to the local range of a reference frame, on host buffers
    (lrt_temporal_rectify_host). ref: float32 [height, width, 4] (or flat with width=, height=), the
    current frame's colour with ref_scale = the step's cur_scale, or any frame at the state's size;
    id: the current G-buffer's int32 [height, width] id plane; state: {"color", "moment2"[, ...]} as a
    temporal step returned it. out: the destination buffers {"color", "moment2"[, "color_std"]}; out=state
    rectifies in place; otherwise none may be an input (the alphas of color and color_std stay);
    default new zeroed ones. class_out: int32 [height, width], receives 0 (inside the box), 1
    (clamped) or 2 (fewer than min_taps pixels of its id in the window: passed through). params:
    radius, min_taps, min_history, ref_scale, gamma, range_floor, reset_history, short_std. Returns
    the rectified state (out)."""
    params = dict(params)
    w, h = _frame_size(ref, params)
    d = temporal_rectify_desc(w, h, **params)
    return _temporal_rectify(B.HostBuffers(), d, ref, id, state, out, class_out)


def temporal_rectify_tensor(ref, id, state: dict, out: Optional[dict] = None, class_out=None, stream=None,
                            **params) -> dict:
    """temporal_rectify_host on cuda tensors (lrt_temporal_rectify_device): asynchronous on `stream`
    (a torch.cuda.Stream, default: current) and ordered only against it. id and class_out are int32
    tensors, the others float32. Returns the rectified state."""
    params = dict(params)
    w, h = _frame_size(ref, params)
    d = temporal_rectify_desc(w, h, **params)
    bufs = B.tensor_buffers(ref, "ref", w * h * 4, stream)
    return _temporal_rectify(bufs, d, ref, id, state, out, class_out)


class TemporalAccumulator:
    """The two ping-pong states of a width x height frame on `device`, the previous camera and, for
    a scene whose spheres move, the previous step's spheres: step() blends a freshly rendered frame
    into the history and returns what the denoiser takes. step_gbuffer() is the same step driven by a
    G-buffer's ids and motion vectors; switching between the two forms, like reset(), drops the
    history."""

    def __init__(self, width: int, height: int, device="cuda:0"):
        import torch

        self.width, self.height = int(width), int(height)
        if self.width < 1 or self.height < 1:
            raise L.LrtError(L.LRT_E_INVALID, "invalid image size")
        self.device = torch.device(device)
        names = L.TEMPORAL_STATE_NAMES + ("color_std",)
        self._states = [{n: torch.zeros((self.height, self.width, 4), device=self.device) for n in names}
                        for _ in range(2)]
        self._cur = 0            # the state the last step wrote
        self._camera = None      # its camera (None: no history for step())
        self._spheres = None     # its scene, if it was given one
        self._prev_g = None      # the last step_gbuffer's normal and id tensors (None: no history for step_gbuffer())
        self._planes = [None, None]   # gbuffer_planes()'s two sets, allocated on first use
        self._firefly = None          # step_gbuffer(firefly=...)'s filtered frame, allocated on first use
        self._excess = None           # step_gbuffer(firefly_restore=...)'s excess frame, allocated on first use

    def reset(self) -> None:
        """Drop the history: the next step or step_gbuffer starts over (a new scene, a camera cut)."""
        self._camera = None
        self._spheres = None
        self._prev_g = None

    def step(self, color, features: dict, camera: L.Camera, cur_scale: float = 1.0, stream=None, spheres=None,
             motion=None, **params):
        """One accumulation step (temporal_accumulate_tensor) of the frame `color` with its
        features {"normal", "world_pos"[, "albedo"]} seen from `camera`. Returns (color, guides):
        the accumulated frame and the dict denoise_tensor takes ("normal", "world_pos", "albedo"
        if given, "color_std"); both are the accumulator's own tensors, valid until the step after
        the next. spheres: the scene the frame was rendered with (Sphere structs or floats
        [count, 4]) where spheres move between steps: the step is then
        temporal_accumulate_moving_tensor against the previous step's scene (on the first step, after
        reset() and after a step without spheres the scene is its own predecessor), and `motion`, a
        cuda tensor [height, width, 4], receives the motion vectors. After a step_gbuffer() the
        history is dropped: the two forms keep different states."""
        self._prev_g = None
        cur = {k: v for k, v in features.items() if k in L.TEMPORAL_CUR_NAMES}
        unknown = [k for k in features if k not in L.FEATURE_NAMES]
        if unknown:
            raise L.LrtError(L.LRT_E_INVALID, f"unknown feature {unknown[0]!r}")
        nxt = self._states[1 - self._cur]
        out = {k: v for k, v in nxt.items() if k != "albedo" or "albedo" in cur}
        prev = None
        if self._camera is not None:
            prev = {k: v for k, v in self._states[self._cur].items() if k != "color_std"}
        if spheres is None:
            if motion is not None:
                raise L.LrtError(L.LRT_E_INVALID, "motion needs spheres")
            temporal_accumulate_tensor(color, cur, prev, camera, self._camera, out=out, stream=stream,
                                       width=self.width, height=self.height, cur_scale=cur_scale, **params)
            self._spheres = None
        else:
            scene = _sphere_array(spheres, "spheres")
            before = self._spheres if self._spheres is not None and len(self._spheres) == len(scene) else scene
            temporal_accumulate_moving_tensor(color, cur, prev, camera, self._camera, scene, before, out=out,
                                              motion=motion, stream=stream, width=self.width, height=self.height,
                                              cur_scale=cur_scale, **params)
            self._spheres = (L.Sphere * len(scene)).from_buffer_copy(scene)
        self._cur = 1 - self._cur
        self._camera = L.Camera.from_buffer_copy(camera)
        return nxt["color"], {k: nxt[k] for k in L.GUIDE_NAMES if k in out}

    def step_gbuffer(self, color, gbuffer: dict, cur_scale: float = 1.0, stream=None, rectify: Optional[dict] = None,
                     firefly: Optional[dict] = None, firefly_restore: Optional[dict] = None, **params):
        """One accumulation step driven by the G-buffer (temporal_accumulate_gbuffer_tensor) of the
        frame `color` with its planes {"normal", "motion", "id"[, ...]} as gbuffer_tensor(id=True,
        motion=True) fills them at guide_scale 1: no camera and no scene. Returns (color,
        {"color_std": ...}), the accumulator's own tensors, valid until the step after the next; the
        G-buffer's own normal, world_pos and albedo are the guides of denoise_tensor and
        svgf_filter_tensor. The accumulator remembers the `normal` and `id` tensors by reference,
        without copying: they are the next step's history, so they must stay as they are until it has
        run, and handing the same tensors in again raises LRT_E_INVALID (ping-pong two sets:
        gbuffer_planes()). Of `state` only color and moment2 are written. After a step() the history is
        dropped: the two forms keep different states. params: alpha_min, normal_min, short_std,
        min_history. rectify: None, or a dict of temporal_rectify_tensor's parameters (possibly empty):
        the step is then followed on the same stream by temporal_rectify_tensor in place on the state
        just written, with `color` as the reference, gbuffer's id, ref_scale = cur_scale and the
        step's own min_history and short_std (unless the dict sets them); color_std is refreshed.
        firefly: None, or a dict of firefly_tensor's parameters (possibly empty): `color` is then first
        filtered by firefly_tensor with gbuffer's id, on the same stream, into a scratch frame the
        accumulator owns, and the step (and its rectify, as the reference) takes that frame instead;
        `color` itself is left as it is. firefly_restore: None, or a dict of firefly_restore_tensor's
        parameters (possibly empty); it needs firefly: the firefly call then also writes its excess
        into a second scratch frame, and firefly_restore_tensor runs in place on the clamped frame with
        gbuffer's id, on the same stream, ahead of the accumulation."""
        if not isinstance(gbuffer, dict) or any(n not in gbuffer for n in L.TEMPORAL_GBUFFER_CUR_NAMES):
            raise L.LrtError(L.LRT_E_INVALID, "gbuffer must hold normal, motion and id")
        if firefly is not None:
            if not isinstance(firefly, dict):
                raise L.LrtError(L.LRT_E_INVALID, "firefly must be None or a dict of firefly_tensor's parameters")
            firefly_desc(self.width, self.height, **firefly)         # an unknown name raises before the step runs
        if firefly_restore is not None:
            if not isinstance(firefly_restore, dict):
                raise L.LrtError(L.LRT_E_INVALID,
                                 "firefly_restore must be None or a dict of firefly_restore_tensor's parameters")
            if firefly is None:
                raise L.LrtError(L.LRT_E_INVALID, "firefly_restore needs firefly: the clamp supplies the excess")
            firefly_restore_desc(self.width, self.height, **firefly_restore)
        rp = None
        if rectify is not None:
            if not isinstance(rectify, dict):
                raise L.LrtError(L.LRT_E_INVALID, "rectify must be None or a dict of temporal_rectify_tensor's parameters")
            rp = {k: params[k] for k in ("min_history", "short_std") if k in params}
            rp.update(ref_scale=cur_scale)
            rp.update(rectify)
            temporal_rectify_desc(self.width, self.height, **rp)     # an unknown name raises before the step runs
        if self._prev_g is not None and any(gbuffer[n] is self._prev_g[n] for n in L.TEMPORAL_GBUFFER_PREV_NAMES):
            raise L.LrtError(L.LRT_E_INVALID, "gbuffer's normal and id are the previous step's tensors: they are its "
                                              "history (fill another set: gbuffer_planes())")
        nxt = self._states[1 - self._cur]
        out = {k: nxt[k] for k in L.TEMPORAL_GBUFFER_STATE_NAMES + ("color_std",)}
        prev = self._states[self._cur] if self._prev_g is not None else None
        if firefly is not None:
            if self._firefly is None:
                import torch
                # (every quad is written by the pass: uninitialised, so that no fill runs on another stream)
                self._firefly = torch.empty((self.height, self.width, 4), device=self.device)
            if firefly_restore is not None and self._excess is None:
                import torch
                self._excess = torch.empty((self.height, self.width, 4), device=self.device)
            color = firefly_tensor(color, gbuffer["id"], out=self._firefly, stream=stream, width=self.width,
                                   height=self.height, excess_out=self._excess if firefly_restore is not None else None,
                                   **firefly)["out"]
            if firefly_restore is not None:
                firefly_restore_tensor(color, self._excess, gbuffer["id"], out=color, stream=stream, width=self.width,
                                       height=self.height, **firefly_restore)
        temporal_accumulate_gbuffer_tensor(color, gbuffer, self._prev_g, prev, out=out, stream=stream,
                                           width=self.width, height=self.height, cur_scale=cur_scale, **params)
        if rp is not None:
            temporal_rectify_tensor(color, gbuffer["id"], out, out=out, stream=stream, width=self.width,
                                    height=self.height, **rp)
        self._prev_g = {n: gbuffer[n] for n in L.TEMPORAL_GBUFFER_PREV_NAMES}
        self._cur = 1 - self._cur
        self._camera = None
        self._spheres = None
        return nxt["color"], {"color_std": nxt["color_std"]}

    def gbuffer_planes(self) -> dict:
        """The set of G-buffer planes to fill next, {"normal", "world_pos", "albedo", "motion", "id"}
        (id int32 [height, width], the others float32 [height, width, 4]): one of two sets the
        accumulator allocates on first use (uninitialised until filled), the one the last
        step_gbuffer() does not hold as its history. Meant as gbuffer_tensor(..., out=acc.gbuffer_planes()),
        whose result goes to step_gbuffer(): the caller ping-pongs without owning buffers."""
        import torch

        held = self._prev_g["normal"] if self._prev_g is not None else None
        k = 1 if self._planes[0] is not None and held is self._planes[0]["normal"] else 0
        if self._planes[k] is None:
            self._planes[k] = {n: torch.empty((self.height, self.width) if n == "id" else (self.height, self.width, 4),
                                              dtype=torch.int32 if n == "id" else torch.float32, device=self.device)
                               for n in L.TEMPORAL_GBUFFER_PLANES}
        return dict(self._planes[k])

    @property
    def state(self) -> dict:
        """The state the last step wrote, {"color", "moment2", "normal", "world_pos", "albedo"}: the
        accumulator's own tensors, valid until the step after the next; read-only (a new dict each
        time). svgf_filter_tensor(acc.state["color"], acc.state["moment2"], guides) chains on the
        step's stream. step_gbuffer() writes color and moment2 only."""
        return {k: self._states[self._cur][k] for k in L.TEMPORAL_STATE_NAMES}


# ---- variance-guided filter over the temporal state ----------------------------------------
def svgf_desc(width: int, height: int, **params) -> L.SvgfDesc:
    """lrt_svgf_default for a width x height frame, with any of iterations, min_history,
    sigma_color, sigma_normal, sigma_pos, albedo_floor overridden."""
    d = L.SvgfDesc()
    L.check(L.lib().lrt_svgf_default(int(width), int(height), ctypes.byref(d)))
    return _override(d, params, L.SVGF_PARAMS, ("iterations", "min_history"), "svgf")


def _svgf_filter(bufs, d, color, moment2, guides, out, variance_out):
    n = d.width * d.height * 4
    bufs.check(color, "color", n)
    bufs.check(moment2, "moment2", n)
    if out is None:
        out = bufs.copy(color)
    bufs.check(out, "out", n)
    if variance_out is not None:
        bufs.check(variance_out, "variance_out", n)
    # (step()'s guides may be passed as they are: color_std is not read)
    f = _features(bufs, guides or {}, n, L.FEATURE_NAMES, "guide", stored=L.SVGF_GUIDE_NAMES)
    L.check(bufs.entry("svgf_filter")(ctypes.byref(d), bufs.ptr(color), bufs.ptr(moment2),
                                      ctypes.byref(f) if guides else None, bufs.ptr(out), bufs.ptr(variance_out),
                                      *bufs.tail))
    return out


def svgf_filter_host(color: np.ndarray, moment2: np.ndarray, guides: Optional[dict],
                     out: Optional[np.ndarray] = None, variance_out: Optional[np.ndarray] = None, **params):
    """Filter a temporal state with the variance-guided a-trous filter (lrt_svgf_filter_host).
    color, moment2: the state's members, float32 [height, width, 4] (or flat with width=,
    height=), the history length in moment2's alpha; guides: {name: buffer} with "normal",
    "world_pos", "albedo" (a missing one drops its term; None or {}: no guides; the other
    lrt_features names are accepted and not read, so that step()'s guides pass as they are). out: the
    destination (may be color; only its rgb is written), default a copy of color. variance_out:
    if given, receives the filtered variance (rgb only). params: iterations, min_history,
    sigma_color, sigma_normal, sigma_pos, albedo_floor. Returns out."""
    params = dict(params)
    w, h = _frame_size(color, params)
    return _svgf_filter(B.HostBuffers(), svgf_desc(w, h, **params), color, moment2, guides, out, variance_out)


def svgf_filter_tensor(color, moment2, guides: Optional[dict], out=None, variance_out=None, stream=None, **params):
    """svgf_filter_host on cuda float32 tensors (lrt_svgf_filter_device): asynchronous on `stream`
    (a torch.cuda.Stream, default: current) and ordered only against it. Returns out."""
    params = dict(params)
    w, h = _frame_size(color, params)
    d = svgf_desc(w, h, **params)
    bufs = B.tensor_buffers(color, "color", w * h * 4, stream)
    return _svgf_filter(bufs, d, color, moment2, guides, out, variance_out)


# ---- auto-exposure metering and tone mapping -------------------------------------------------
def tonemap_desc(width: int, height: int, **params) -> L.TonemapDesc:
    """lrt_tonemap_default for a width x height frame, with any of op (an LRT_TM_* value or
    "linear" / "reinhard" / "aces"), auto_exposure, key, p_low, p_high, ev_bias, ev_min, ev_max,
    adapt, white overridden."""
    d = L.TonemapDesc()
    L.check(L.lib().lrt_tonemap_default(int(width), int(height), ctypes.byref(d)))
    op = params.get("op")
    if isinstance(op, str):
        if op not in L.TONEMAP_OPS:
            raise L.LrtError(L.LRT_E_INVALID, f"unknown tone operator {op!r}")
        params = dict(params, op=L.TONEMAP_OPS[op])
    return _override(d, params, L.TONEMAP_PARAMS, ("op", "auto_exposure"), "tonemap")


def _tonemap(bufs, d, color, state, out, bgra, histogram):
    n = d.width * d.height * 4
    words = (bufs.uword, "int32", "uint32")       # either passes; the message names the back end's own
    bufs.check(color, "color", n)
    if state is None and d.auto_exposure:
        state = bufs.zeros(4)
    for what, buf, count, dtypes in (("state", state, 4, ("float32",)), ("out", out, n, ("float32",)),
                                     ("bgra", bgra, d.width * d.height, words),
                                     ("histogram", histogram, L.TONEMAP_HIST_WORDS, words)):
        if buf is not None:
            bufs.check(buf, what, count, dtypes)
    L.check(bufs.entry("tonemap")(ctypes.byref(d), bufs.ptr(color), bufs.ptr(state), bufs.ptr(histogram), bufs.ptr(out),
                                  bufs.ptr(bgra), *bufs.tail))
    return state


def tonemap_host(color: np.ndarray, state: Optional[np.ndarray] = None, out: Optional[np.ndarray] = None,
                 bgra: Optional[np.ndarray] = None, histogram: Optional[np.ndarray] = None, **params):
    """Meter and tone-map a frame on host buffers (lrt_tonemap_host). color: float32 [height, width,
    4] (or flat with width=, height=). state: the exposure state, float32[4] (log2_exposure,
    log2_luminance, counted, frames), read and updated in place; None: a new zeroed one (no
    history). out: if given, receives the mapped linear rgb (its alpha stays; it may be color).
    bgra: if given, uint32 of >= width * height, receives the quantised pixels. histogram: if
    given, uint32 of >= 258, receives the counts. params: op, auto_exposure, key, p_low, p_high,
    ev_bias, ev_min, ev_max, adapt, white. Returns the state (None with auto_exposure=0 and no state
    given; it is left untouched then)."""
    params = dict(params)
    w, h = _frame_size(color, params)
    return _tonemap(B.HostBuffers(), tonemap_desc(w, h, **params), color, state, out, bgra, histogram)


def tonemap_tensor(color, state=None, out=None, bgra=None, histogram=None, stream=None, **params):
    """tonemap_host on cuda tensors (lrt_tonemap_device): asynchronous on `stream` (a
    torch.cuda.Stream, default: current) and ordered only against it; the exposure never visits
    the host. color, out: float32; state: float32 of >= 4; bgra, histogram: int32 (or uint32).
    Returns the state tensor."""
    params = dict(params)
    w, h = _frame_size(color, params)
    d = tonemap_desc(w, h, **params)
    bufs = B.tensor_buffers(color, "color", w * h * 4, stream)
    return _tonemap(bufs, d, color, state, out, bgra, histogram)


class ToneMapper:
    """The exposure state (16 B) and a histogram of a width x height frame on `device`: step() meters
    a frame, adapts the exposure and maps the frame, all on the stream."""

    def __init__(self, width: int, height: int, device="cuda:0"):
        import torch

        self.width, self.height = int(width), int(height)
        if self.width < 1 or self.height < 1:
            raise L.LrtError(L.LRT_E_INVALID, "invalid image size")
        self.device = torch.device(device)
        self._state = torch.zeros(4, device=self.device)
        self.histogram = torch.zeros(L.TONEMAP_HIST_WORDS, dtype=torch.int32, device=self.device)

    def reset(self, stream=None) -> None:
        """Drop the exposure history (a new scene, a cut): the next step takes its target at once."""
        import torch

        with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream(self.device)):
            self._state.zero_()

    def step(self, color, bgra=None, out=None, stream=None, **params):
        """One tonemap_tensor call of `color` against the mapper's state and histogram. Returns
        (bgra, out) as given."""
        tonemap_tensor(color, self._state, out=out, bgra=bgra, histogram=self.histogram, stream=stream,
                       width=self.width, height=self.height, **params)
        return bgra, out

    @property
    def state(self) -> dict:
        """The four floats of the exposure state after the work enqueued so far (synchronises)."""
        import torch

        torch.cuda.synchronize(self.device)   # whichever streams the steps went to
        v = self._state.cpu().tolist()
        return dict(zip(("log2_exposure", "log2_luminance", "counted", "frames"), v))


# ---- G-buffer: pixel-centre first-hit guides, ids, depth and motion -------------------------
def gbuffer_desc(width: int, height: int, camera: L.Camera, prev_camera: Optional[L.Camera] = None,
                 guide_scale: float = 1.0) -> L.GbufferDesc:
    """lrt_gbuffer_default for a width x height frame seen from `camera`, the previous frame from
    `prev_camera` (None: the same camera), with guide_scale set."""
    if not isinstance(camera, L.Camera) or not (prev_camera is None or isinstance(prev_camera, L.Camera)):
        raise L.LrtError(L.LRT_E_INVALID, "camera and prev_camera must be Camera structs")
    d = L.GbufferDesc()
    L.check(L.lib().lrt_gbuffer_default(int(width), int(height), ctypes.byref(camera),
                                        ctypes.byref(prev_camera) if prev_camera is not None else None,
                                        ctypes.byref(d)))
    d.guide_scale = float(guide_scale)
    return d


def _out_tensor_buffers(out, kinds, device, stream):
    """The TensorBuffers of a unit that keys on its output planes: on the device of out's first plane,
    or on `device` where it allocates them."""
    if not out:
        return B.TensorBuffers(device, stream)
    name, first = next(iter(out.items()))
    count, dtypes, _ = kinds.get(name, kinds["quad"])
    return B.tensor_buffers(first, name, count, stream, dtypes[0])


def _new_planes(bufs, names, kinds) -> dict:
    return {name: bufs.new(kinds.get(name, kinds["quad"])) for name in names}


def _gbuffer(bufs, d, out, want, spheres, prev_spheres):
    """out: the caller's planes {name: buffer} (only those are written), or None for new ones."""
    k = _kinds(d.width, d.height)
    if out is None:
        out = _new_planes(bufs, L.GBUFFER_GUIDE_NAMES + tuple(n for n in L.GBUFFER_EXTRA_NAMES if want[n]), k)
    g = _gbuffer_planes(bufs, out, "", (), k, stored=L.GBUFFER_NAMES)
    L.check(bufs.entry("gbuffer")(ctypes.byref(d), _moved(spheres, prev_spheres), ctypes.byref(g), *bufs.tail))
    return out


def gbuffer_host(width: int, height: int, camera: L.Camera, prev_camera: Optional[L.Camera] = None,
                 id: bool = False, depth: bool = False, motion: bool = False, spheres=None, prev_spheres=None,
                 guide_scale: float = 1.0, out: Optional[dict] = None) -> dict:
    """The G-buffer of the current scene seen from `camera` through the pixel centres
    (lrt_gbuffer_host): {"normal", "world_pos", "albedo"} as float32 [height, width, 4] (what
    TemporalAccumulator.step, denoise_* and svgf_* take as features or guides), each times
    guide_scale, plus "id" (int32 [height, width], -1 on a miss), "depth" (float32 [height, width],
    +Inf on a miss) and "motion" (float32 [height, width, 4]: previous minus current position in
    pixels, the sphere, 1 if projectable) when asked for. prev_camera: the previous frame's camera
    (motion only). prev_spheres: the previous frame's scene where spheres moved (Sphere structs or
    floats [count, 4]); spheres: the current one (default: what the library holds; it must be that).
    out: the caller's planes instead, any subset of the six names; only those are written."""
    w, h = int(width), int(height)
    d = gbuffer_desc(w, h, camera, prev_camera, guide_scale)
    return _gbuffer(B.HostBuffers(), d, out, dict(id=id, depth=depth, motion=motion), spheres, prev_spheres)


def gbuffer_tensor(width: int, height: int, camera: L.Camera, prev_camera: Optional[L.Camera] = None,
                   id: bool = False, depth: bool = False, motion: bool = False, spheres=None, prev_spheres=None,
                   guide_scale: float = 1.0, out: Optional[dict] = None, stream=None, device="cuda:0") -> dict:
    """gbuffer_host into cuda tensors (lrt_gbuffer_device): asynchronous on `stream` (a
    torch.cuda.Stream, default: current) and ordered only against it; the sphere arrays are read
    before it returns. "id" is an int32 tensor, the others float32."""
    w, h = int(width), int(height)
    d = gbuffer_desc(w, h, camera, prev_camera, guide_scale)
    bufs = _out_tensor_buffers(out, _kinds(w, h), device, stream)
    return _gbuffer(bufs, d, out, dict(id=id, depth=depth, motion=motion), spheres, prev_spheres)


# ---- G-buffer chain: guides and path keys through mirrors and glass -------------------------
def gbuffer_chain_desc(width: int, height: int, camera: L.Camera, max_bounces: int = 4, roughness_max: float = 0.25,
                       guide_scale: float = 1.0) -> L.GbufferChainDesc:
    """lrt_gbuffer_chain_default for a width x height frame seen from `camera`, with max_bounces
    (0..CHAIN_MAX_BOUNCES), roughness_max and guide_scale set."""
    if not isinstance(camera, L.Camera):
        raise L.LrtError(L.LRT_E_INVALID, "camera must be a Camera struct")
    d = L.GbufferChainDesc()
    L.check(L.lib().lrt_gbuffer_chain_default(int(width), int(height), ctypes.byref(camera), ctypes.byref(d)))
    d.max_bounces = int(max_bounces)
    d.roughness_max = float(roughness_max)
    d.guide_scale = float(guide_scale)
    return d


def _chain_kinds(width: int, height: int):
    return _kinds(width, height, words=L.GBUFFER_CHAIN_INT_NAMES)


def _gbuffer_chain(bufs, d, out, which):
    """which: name=False leaves a plane out of the new ones."""
    for name in which:
        if name not in L.GBUFFER_CHAIN_NAMES:
            raise L.LrtError(L.LRT_E_INVALID, f"unknown chain plane {name!r}")
    k = _chain_kinds(d.width, d.height)
    if out is None:
        out = _new_planes(bufs, [name for name in L.GBUFFER_CHAIN_NAMES if which.get(name, True)], k)
    g = _members(bufs, out, L.GbufferChain, k, known=L.GBUFFER_CHAIN_NAMES, stored=L.GBUFFER_CHAIN_NAMES,
                 noun="chain plane")
    L.check(bufs.entry("gbuffer_chain")(ctypes.byref(d), ctypes.byref(g), *bufs.tail))
    return out


def gbuffer_chain_host(width: int, height: int, camera: L.Camera, max_bounces: int = 4, roughness_max: float = 0.25,
                       guide_scale: float = 1.0, out: Optional[dict] = None, **which) -> dict:
    """The G-buffer of the current scene followed through mirrors and glass (lrt_gbuffer_chain_host):
    from the pixel-centre first hit along reflect / refract through every Metal of roughness <=
    roughness_max and every Dielectric, up to max_bounces surfaces, to the first surface that
    scatters diffusely. Returns {"normal", "world_pos", "albedo"} as float32 [height, width, 4]
    (that surface's, each times guide_scale, the albedo tinted by the mirrors on the way), "key"
    (int32 [height, width]: the path key, the first hit's id where nothing was followed), "id" (the
    terminal sphere, -1: the sky), "bounces" (the surfaces followed, plus CHAIN_UNRESOLVED where the
    walk stopped on a delta surface) and "depth" (float32 [height, width]: the path's length, +Inf
    on the sky). which: name=False leaves a plane out. out: the caller's planes instead, any subset
    of the seven names; only those are written.

    The composition with the stages that exist (none of them changes; motion and the first-hit
    normal come from gbuffer_*):
      TemporalAccumulator.step_gbuffer(color, {"normal": g["normal"], "motion": g["motion"],
                                               "id": chain["key"]})   # ping-pong two key tensors, as the planes
      temporal_rectify_tensor(..., id=chain["key"])
      svgf_filter_tensor / denoise_tensor with chain["normal"], chain["world_pos"], chain["albedo"] as guides
      upsample_tensor with "key" as "id" in both G-buffers."""
    w, h = int(width), int(height)
    d = gbuffer_chain_desc(w, h, camera, max_bounces, roughness_max, guide_scale)
    return _gbuffer_chain(B.HostBuffers(), d, out, which)


def gbuffer_chain_tensor(width: int, height: int, camera: L.Camera, max_bounces: int = 4, roughness_max: float = 0.25,
                         guide_scale: float = 1.0, out: Optional[dict] = None, stream=None, device="cuda:0",
                         **which) -> dict:
    """gbuffer_chain_host into cuda tensors (lrt_gbuffer_chain_device): asynchronous on `stream` (a
    torch.cuda.Stream, default: current) and ordered only against it. "key", "id" and "bounces" are
    int32 tensors, the others float32. The composition is gbuffer_chain_host's."""
    w, h = int(width), int(height)
    d = gbuffer_chain_desc(w, h, camera, max_bounces, roughness_max, guide_scale)
    return _gbuffer_chain(_out_tensor_buffers(out, _chain_kinds(w, h), device, stream), d, out, which)


# ---- G-buffer chain motion: motion vectors inside mirrors and glass -------------------------
def gbuffer_chain_motion_desc(width: int, height: int, camera: L.Camera, prev_camera: Optional[L.Camera] = None,
                              **params) -> L.GbufferChainMotionDesc:
    """lrt_gbuffer_chain_motion_default for a width x height frame seen from `camera`, the previous
    frame from `prev_camera` (None: the same camera), with any of max_bounces, roughness_max,
    iterations, probe_px, step_max_px, converged_px overridden."""
    if not isinstance(camera, L.Camera) or not (prev_camera is None or isinstance(prev_camera, L.Camera)):
        raise L.LrtError(L.LRT_E_INVALID, "camera and prev_camera must be Camera structs")
    d = L.GbufferChainMotionDesc()
    L.check(L.lib().lrt_gbuffer_chain_motion_default(int(width), int(height), ctypes.byref(camera),
                                                     ctypes.byref(prev_camera) if prev_camera is not None else None,
                                                     ctypes.byref(d)))
    return _override(d, params, L.GBUFFER_CHAIN_MOTION_PARAMS, ("max_bounces", "iterations"), "chain motion")


def _gbuffer_chain_motion(bufs, d, first_motion, out, want, spheres, prev_spheres):
    k = _kinds(d.width, d.height, words=("status",))
    if out is None:
        out = _new_planes(bufs, [name for name in L.GBUFFER_CHAIN_MOTION_NAMES if want[name]], k)
    g = _members(bufs, out, L.GbufferChainMotion, k, known=L.GBUFFER_CHAIN_MOTION_NAMES,
                 stored=L.GBUFFER_CHAIN_MOTION_NAMES, noun="chain motion plane")
    bufs.check_plane(first_motion, "first_motion", k["quad"])
    L.check(bufs.entry("gbuffer_chain_motion")(ctypes.byref(d), _moved(spheres, prev_spheres), bufs.ptr(first_motion),
                                               ctypes.byref(g), *bufs.tail))
    return out


def gbuffer_chain_motion_host(width: int, height: int, camera: L.Camera, prev_camera: Optional[L.Camera],
                              first_motion: np.ndarray, spheres=None, prev_spheres=None, motion: bool = True,
                              status: bool = True, out: Optional[dict] = None, **params) -> dict:
    """Motion vectors of what mirrors and glass SHOW (lrt_gbuffer_chain_motion_host). first_motion is
    gbuffer_*'s "motion" for the same camera pair and scene pair (float32 [height, width, 4]); for every
    pixel whose chain followed a surface the pass searches the previous frame for the position whose
    chain ends at the same surface point. Returns {"motion": float32 [height, width, 4], gbuffer_*'s
    layout: the found vector where the search converged, first_motion's quad bit for bit everywhere
    else; "status": int32 [height, width], CM_*}. prev_spheres: the previous frame's scene where
    spheres moved (at most 16 spheres), spheres: the current one (default: what the library holds).
    motion / status = False leaves a plane out. out: the caller's planes instead; only those are
    written. params: max_bounces and roughness_max (the chain's), iterations, probe_px, step_max_px,
    converged_px.

    The composition (no stage changes): with g = gbuffer_*(motion=True), chain = gbuffer_chain_* and
    cm = this pass,
      TemporalAccumulator.step_gbuffer(color, {"normal": g["normal"], "motion": cm["motion"],
                                               "id": chain["key"]})
    and likewise "motion" of temporal_upsample_* and temporal_rectify_*."""
    w, h = int(width), int(height)
    d = gbuffer_chain_motion_desc(w, h, camera, prev_camera, **params)
    return _gbuffer_chain_motion(B.HostBuffers(), d, first_motion, out, dict(motion=motion, status=status), spheres,
                                 prev_spheres)


def gbuffer_chain_motion_tensor(width: int, height: int, camera: L.Camera, prev_camera: Optional[L.Camera],
                                first_motion, spheres=None, prev_spheres=None, motion: bool = True,
                                status: bool = True, out: Optional[dict] = None, stream=None, **params) -> dict:
    """gbuffer_chain_motion_host on cuda tensors (lrt_gbuffer_chain_motion_device): asynchronous on
    `stream` (a torch.cuda.Stream, default: current) and ordered only against it; the sphere arrays are
    read before it returns. "status" is an int32 tensor, "motion" float32, on first_motion's device."""
    w, h = int(width), int(height)
    d = gbuffer_chain_motion_desc(w, h, camera, prev_camera, **params)
    bufs = B.tensor_buffers(first_motion, "first_motion", w * h * 4, stream)
    return _gbuffer_chain_motion(bufs, d, first_motion, out, dict(motion=motion, status=status), spheres, prev_spheres)


# ---- G-buffer-guided upsampling of a low-resolution frame -----------------------------------
def upsample_desc(width: int, height: int, low_width: int, low_height: int, **params) -> L.UpsampleDesc:
    """lrt_upsample_default for a width x height frame from a low_width x low_height one, with any of
    sigma_normal, albedo_floor, weight_min, flags (UP_BILINEAR) overridden."""
    d = L.UpsampleDesc()
    L.check(L.lib().lrt_upsample_default(int(width), int(height), int(low_width), int(low_height), ctypes.byref(d)))
    return _override(d, params, L.UPSAMPLE_PARAMS, ("flags",), "upsample")


def _upsample_sizes(color_low, low, high):
    """(width, height, low_width, low_height) from color_low [low_height, low_width, 4] and high's id
    [height, width]."""
    if len(getattr(color_low, "shape", ())) != 3 or color_low.shape[2] != 4:
        raise L.LrtError(L.LRT_E_INVALID, "color_low must be [low_height, low_width, 4]")
    for d, what in ((low, "low"), (high, "high")):
        if not isinstance(d, dict) or "id" not in d:
            raise L.LrtError(L.LRT_E_INVALID, f"{what} must hold id")
    if len(getattr(high["id"], "shape", ())) != 2:
        raise L.LrtError(L.LRT_E_INVALID, "high id must be [height, width]")
    return int(high["id"].shape[1]), int(high["id"].shape[0]), int(color_low.shape[1]), int(color_low.shape[0])


def _upsample(bufs, d, color_low, low, high, out, class_out):
    k, kl = _kinds(d.width, d.height), _kinds(d.low_width, d.low_height)
    need = ("id",) if d.flags & L.UP_BILINEAR else ("id", "normal")
    bufs.check_plane(color_low, "color_low", kl["quad"])
    gl = _gbuffer_planes(bufs, low, "low", need, kl, stored=L.UPSAMPLE_NAMES)
    gh = _gbuffer_planes(bufs, high, "high", need, k, stored=L.UPSAMPLE_NAMES)
    if out is None:
        out = bufs.new(k["quad"])
    bufs.check_plane(out, "out", k["quad"])
    if class_out is not None:
        bufs.check_plane(class_out, "class_out", k["word"])
    L.check(bufs.entry("upsample")(ctypes.byref(d), bufs.ptr(color_low), ctypes.byref(gl), ctypes.byref(gh),
                                   bufs.ptr(out), bufs.ptr(class_out), *bufs.tail))
    return out


def upsample_host(color_low: np.ndarray, low: dict, high: dict, out: Optional[np.ndarray] = None,
                  class_out: Optional[np.ndarray] = None, **params) -> np.ndarray:
    """Upsample a low-resolution frame with the output frame's G-buffer as guide, on host buffers
    (lrt_upsample_host). color_low: float32 [low_height, low_width, 4] (svgf_filter_host's output,
    say); low and high: the G-buffers of the low and of the output frame as gbuffer_host(id=True)
    returns them for the same camera at guide_scale 1, {"id", "normal"[, "albedo"][, ...]} (id int32
    [height, width], the rest float32; albedo in both or in neither -- drop it from both for a plain
    colour; the other planes are not read). The sizes are the arrays'. out: the destination, float32
    of >= width * height * 4 elements (only its rgb is written), default a zeroed [height, width, 4];
    class_out: int32 of >= width * height elements receiving each pixel's class (0: its own surface
    among the four taps, 1: one ring further out, 2: plain bilinear). params: sigma_normal,
    albedo_floor, weight_min, flags (UP_BILINEAR: every pixel class 2, no normals needed). Returns out."""
    w, h, lw, lh = _upsample_sizes(color_low, low, high)
    d = upsample_desc(w, h, lw, lh, **params)
    return _upsample(B.HostBuffers(), d, color_low, low, high, out, class_out)


def upsample_tensor(color_low, low: dict, high: dict, out=None, class_out=None, stream=None, **params):
    """upsample_host on cuda tensors (lrt_upsample_device): asynchronous on `stream` (a
    torch.cuda.Stream, default: current) and ordered only against it. "id" and class_out are int32
    tensors, the others float32. Returns out."""
    w, h, lw, lh = _upsample_sizes(color_low, low, high)
    d = upsample_desc(w, h, lw, lh, **params)
    bufs = B.tensor_buffers(color_low, "color_low", lw * lh * 4, stream)
    return _upsample(bufs, d, color_low, low, high, out, class_out)


# ---- temporal upsampling: a full-resolution history from jittered low frames -----------------
def temporal_upsample_desc(width: int, height: int, low_width: int, low_height: int, **params) -> L.TemporalUpsampleDesc:
    """lrt_temporal_upsample_default for a width x height frame from a low_width x low_height one,
    with any of cur_scale, alpha_min, normal_min, short_std, min_history, sigma_normal, sigma_sample,
    weight_min, jitter_x, jitter_y overridden."""
    d = L.TemporalUpsampleDesc()
    L.check(L.lib().lrt_temporal_upsample_default(int(width), int(height), int(low_width), int(low_height),
                                                  ctypes.byref(d)))
    return _override(d, params, L.TEMPORAL_UPSAMPLE_PARAMS, ("min_history", "jitter_x", "jitter_y"), "temporal upsample")


def jitter_camera(camera: L.Camera, width: int, height: int, low_width: int, low_height: int, jitter_x: int,
                  jitter_y: int) -> L.Camera:
    """The low frame's camera under the jitter (lrt_camera_jitter): `camera` with its lower left
    corner shifted so that low pixel X has its centre at X + 1/2 + jitter_x / (2 width) (rows
    likewise). Render the low frame and its G-buffer with it, and the output frame's G-buffer with
    `camera` itself."""
    if not isinstance(camera, L.Camera):
        raise L.LrtError(L.LRT_E_INVALID, "camera must be a Camera struct")
    out = L.Camera()
    L.check(L.lib().lrt_camera_jitter(ctypes.byref(camera), int(width), int(height), int(low_width), int(low_height),
                                      int(jitter_x), int(jitter_y), ctypes.byref(out)))
    return out


def jitter_phases(width: int, low_width: int, height: int, low_height: int):
    """The jitters [(jitter_x, jitter_y), ...] that put a low sample on every output pixel centre, for
    a whole-number ratio on either axis (R x R of them at ratio R; (-+low_width, -+low_height) at ratio
    2): phase p of an axis is low (2p + 1 - R). Each step moves along both axes, so that a short run of
    steps already covers either. Raises LRT_E_INVALID for another ratio."""
    w, lw, h, lh = int(width), int(low_width), int(height), int(low_height)
    if lw < 1 or lh < 1 or w % lw or h % lh or w < lw or h < lh:
        raise L.LrtError(L.LRT_E_INVALID, "jitter_phases needs whole-number ratios width / low_width and height / low_height")
    rx, ry = w // lw, h // lh
    return [(lw * (2 * (k % rx) + 1 - rx), lh * (2 * ((k // rx + k % rx) % ry) + 1 - ry)) for k in range(rx * ry)]


def _temporal_upsample_sizes(color_low, cur):
    """(width, height, low_width, low_height) from color_low [low_height, low_width, 4] and cur's id
    [height, width]."""
    if len(getattr(color_low, "shape", ())) != 3 or color_low.shape[2] != 4:
        raise L.LrtError(L.LRT_E_INVALID, "color_low must be [low_height, low_width, 4]")
    if not isinstance(cur, dict) or "id" not in cur or len(getattr(cur["id"], "shape", ())) != 2:
        raise L.LrtError(L.LRT_E_INVALID, "cur must hold id as [height, width]")
    return int(cur["id"].shape[1]), int(cur["id"].shape[0]), int(color_low.shape[1]), int(color_low.shape[0])


def _temporal_upsample(bufs, d, color_low, low, cur, prev_g, prev, out, class_out):
    k, kl = _kinds(d.width, d.height), _kinds(d.low_width, d.low_height)
    quad = k["quad"]
    bufs.check_plane(color_low, "color_low", kl["quad"])
    gl = _gbuffer_planes(bufs, low, "low", L.TEMPORAL_UPSAMPLE_LOW_NAMES, kl)
    gc = _gbuffer_planes(bufs, cur, "cur", L.TEMPORAL_GBUFFER_CUR_NAMES, k)
    gp = _gbuffer_planes(bufs, prev_g, "prev_g", L.TEMPORAL_GBUFFER_PREV_NAMES, k) if prev_g is not None else None
    ps = _gbuffer_state(bufs, prev, "prev", L.TEMPORAL_STATE_NAMES, k) if prev is not None else None
    if out is None:
        out = _new_gbuffer_state(bufs, quad)
    ns = _gbuffer_state(bufs, out, "out", L.TEMPORAL_GBUFFER_STATE_NAMES, k)
    std = _color_std(bufs, out, quad)
    if class_out is not None:
        bufs.check_plane(class_out, "class_out", k["word"])
    L.check(bufs.entry("temporal_upsample")(ctypes.byref(d), bufs.ptr(color_low), ctypes.byref(gl), ctypes.byref(gc),
                                            _byref(gp), _byref(ps), ctypes.byref(ns), std, bufs.ptr(class_out),
                                            *bufs.tail))
    return out


def temporal_upsample_host(color_low: np.ndarray, low: dict, cur: dict, prev_g: Optional[dict], prev: Optional[dict],
                           out: Optional[dict] = None, class_out: Optional[np.ndarray] = None, jitter=(0, 0),
                           **params) -> dict:
    """One temporal upsampling step on host buffers (lrt_temporal_upsample_host). color_low: the low
    frame rendered under jitter_camera(camera, ..., *jitter), float32 [low_height, low_width, 4]; low:
    its G-buffer {"id", "normal"[, ...]} under the same jittered camera; cur: the output frame's
    G-buffer {"normal", "motion", "id"[, ...]} under `camera` itself, as gbuffer_host(id=True,
    motion=True) returns it at guide_scale 1; prev_g {"normal", "id"[, ...]} and prev {"color",
    "moment2"[, ...]}: the previous step's output-size G-buffer and the state it returned -- both, or
    None and None for no history. The sizes are the arrays'. out: the destination buffers {"color",
    "moment2"[, "color_std"]} at the output size (the alphas of color and color_std stay), default new
    zeroed ones; class_out: int32 of >= width * height elements receiving each pixel's class (0: history
    and current, 1: history only, 2: current only, 3: neither). params: cur_scale (the colour's only),
    alpha_min, normal_min, short_std, min_history, sigma_normal, sigma_sample, weight_min. Returns the
    new state (out)."""
    w, h, lw, lh = _temporal_upsample_sizes(color_low, cur)
    d = temporal_upsample_desc(w, h, lw, lh, jitter_x=jitter[0], jitter_y=jitter[1], **params)
    return _temporal_upsample(B.HostBuffers(), d, color_low, low, cur, prev_g, prev, out, class_out)


def temporal_upsample_tensor(color_low, low: dict, cur: dict, prev_g: Optional[dict], prev: Optional[dict],
                             out: Optional[dict] = None, class_out=None, jitter=(0, 0), stream=None, **params) -> dict:
    """temporal_upsample_host on cuda tensors (lrt_temporal_upsample_device): asynchronous on `stream`
    (a torch.cuda.Stream, default: current) and ordered only against it. "id" and class_out are int32
    tensors, the others float32. Returns the new state."""
    w, h, lw, lh = _temporal_upsample_sizes(color_low, cur)
    d = temporal_upsample_desc(w, h, lw, lh, jitter_x=jitter[0], jitter_y=jitter[1], **params)
    bufs = B.tensor_buffers(color_low, "color_low", lw * lh * 4, stream)
    return _temporal_upsample(bufs, d, color_low, low, cur, prev_g, prev, out, class_out)


class TemporalUpsampler:
    """The two ping-pong states of a width x height history on `device`, fed by low_width x low_height
    frames whose camera is shifted by a different jitter each step (jitter_phases, jitter_camera):
    step() blends one low frame in and returns what svgf_filter_tensor takes at the output size.
    There is no rectify= here: the low frame is not at the state's size. The state can be handed to
    temporal_rectify_tensor(ref, gbuffer["id"], state, out=state) with a full-size reference the caller
    makes (upsample_tensor of the low frame, say)."""

    def __init__(self, width: int, height: int, low_width: int, low_height: int, device="cuda:0"):
        import torch

        self.width, self.height = int(width), int(height)
        self.low_width, self.low_height = int(low_width), int(low_height)
        if not (1 <= self.low_width <= self.width and 1 <= self.low_height <= self.height):
            raise L.LrtError(L.LRT_E_INVALID, "invalid image size")
        self.device = torch.device(device)
        names = L.TEMPORAL_GBUFFER_STATE_NAMES + ("color_std",)
        self._states = [{n: torch.zeros((self.height, self.width, 4), device=self.device) for n in names}
                        for _ in range(2)]
        self._cur = 0            # the state the last step wrote
        self._prev_g = None      # the last step's normal and id tensors (None: no history)
        self._planes = [None, None]   # gbuffer_planes()'s two sets, allocated on first use

    def reset(self) -> None:
        """Drop the history: the next step starts over (a new scene, a camera cut)."""
        self._prev_g = None

    def step(self, color_low, low_gbuffer: dict, gbuffer: dict, jitter=(0, 0), cur_scale: float = 1.0, class_out=None,
             stream=None, **params):
        """One step (temporal_upsample_tensor) of the low frame `color_low` rendered under
        jitter_camera(camera, ..., *jitter), with its planes low_gbuffer {"id", "normal"[, ...]} under
        the same jittered camera and the output frame's planes gbuffer {"normal", "motion", "id"[, ...]}
        under `camera` itself. Returns (color, {"color_std": ...}), the upsampler's own tensors, valid
        until the step after the next; the G-buffer's own normal, world_pos and albedo are the guides
        of svgf_filter_tensor. The upsampler remembers gbuffer's `normal` and `id` tensors by reference,
        without copying: they are the next step's history, and handing the same tensors in again raises
        LRT_E_INVALID (ping-pong two sets: gbuffer_planes()). params: alpha_min, normal_min, short_std,
        min_history, sigma_normal, sigma_sample, weight_min."""
        if not isinstance(gbuffer, dict) or any(n not in gbuffer for n in L.TEMPORAL_GBUFFER_CUR_NAMES):
            raise L.LrtError(L.LRT_E_INVALID, "gbuffer must hold normal, motion and id")
        if self._prev_g is not None and any(gbuffer[n] is self._prev_g[n] for n in L.TEMPORAL_GBUFFER_PREV_NAMES):
            raise L.LrtError(L.LRT_E_INVALID, "gbuffer's normal and id are the previous step's tensors: they are its "
                                              "history (fill another set: gbuffer_planes())")
        if tuple(getattr(color_low, "shape", ())) != (self.low_height, self.low_width, 4) or \
                tuple(getattr(gbuffer["id"], "shape", ())) != (self.height, self.width):
            raise L.LrtError(L.LRT_E_INVALID, "color_low must be [low_height, low_width, 4] and gbuffer id [height, width]")
        nxt = self._states[1 - self._cur]
        prev = self._states[self._cur] if self._prev_g is not None else None
        temporal_upsample_tensor(color_low, low_gbuffer, gbuffer, self._prev_g, prev, out=dict(nxt), class_out=class_out,
                                 jitter=jitter, stream=stream, cur_scale=cur_scale, **params)
        self._prev_g = {n: gbuffer[n] for n in L.TEMPORAL_GBUFFER_PREV_NAMES}
        self._cur = 1 - self._cur
        return nxt["color"], {"color_std": nxt["color_std"]}

    def gbuffer_planes(self) -> dict:
        """The set of output-size G-buffer planes to fill next, {"normal", "world_pos", "albedo",
        "motion", "id"}: one of two sets the upsampler allocates on first use (uninitialised until
        filled), the one the last step() does not hold as its history
        (TemporalAccumulator.gbuffer_planes)."""
        import torch

        held = self._prev_g["normal"] if self._prev_g is not None else None
        k = 1 if self._planes[0] is not None and held is self._planes[0]["normal"] else 0
        if self._planes[k] is None:
            self._planes[k] = {n: torch.empty((self.height, self.width) if n == "id" else (self.height, self.width, 4),
                                              dtype=torch.int32 if n == "id" else torch.float32, device=self.device)
                               for n in L.TEMPORAL_GBUFFER_PLANES}
        return dict(self._planes[k])

    @property
    def state(self) -> dict:
        """The state the last step wrote, {"color", "moment2"}: the upsampler's own tensors, valid until
        the step after the next; read-only (a new dict each time)."""
        return {k: self._states[self._cur][k] for k in L.TEMPORAL_GBUFFER_STATE_NAMES}


# ---- adaptive sampling: the per-pixel sample budget and the render that honours it ------------
def sample_budget_desc(width: int, height: int, min_count: int, max_count: int, budget: int,
                       **params) -> L.SampleBudgetDesc:
    """lrt_sample_budget_default for a width x height frame, with any of flags (L.SB_STD), passes,
    luma_floor, weight_max overridden."""
    d = L.SampleBudgetDesc()
    L.check(L.lib().lrt_sample_budget_default(int(width), int(height), int(min_count), int(max_count), int(budget),
                                              ctypes.byref(d)))
    return _override(d, params, L.SAMPLE_BUDGET_PARAMS, ("flags", "passes"), "sample budget")


def _sample_budget(bufs, d, variance, color, counts, info, info_dtype: str):
    """info: two 64-bit words (the host's own uint64 pair, the caller's int64 tensor), or None."""
    k = B.planes(d.width, d.height)
    bufs.check_plane(variance, "variance", k["quad"])
    if color is not None:
        bufs.check_plane(color, "color", k["quad"])
    if counts is None:
        counts = bufs.new(k["word"])
    bufs.check_plane(counts, "counts", k["word"])
    if info is not None:
        bufs.check(info, "info", 2, (info_dtype,))
    L.check(bufs.entry("sample_budget")(ctypes.byref(d), bufs.ptr(variance), bufs.ptr(color), bufs.ptr(counts),
                                        bufs.ptr(info), *bufs.tail))
    return counts


def sample_budget_host(variance: np.ndarray, min_count: int, max_count: int, budget: int,
                       color: Optional[np.ndarray] = None, counts: Optional[np.ndarray] = None, **params):
    """Per-pixel sample counts from a noise plane (lrt_sample_budget_host). variance: float32
    [height, width, 4] (or flat with width=, height=), the variance_out of svgf_filter_*, or a
    color_std with flags=L.SB_STD; color: the same shape, or None (absolute instead of relative
    error); counts: int32 of >= width * height, default a new [height, width] array. params: flags,
    passes, luma_floor, weight_max. Returns (counts, info) with info = (sum of the counts, the first
    pass's weight sum)."""
    params = dict(params)
    w, h = _frame_size(variance, params)
    d = sample_budget_desc(w, h, min_count, max_count, budget, **params)
    info = np.zeros(2, np.uint64)
    counts = _sample_budget(B.HostBuffers(), d, variance, color, counts, info, "uint64")
    return counts, (int(info[0]), int(info[1]))


def sample_budget_tensor(variance, min_count: int, max_count: int, budget: int, color=None, counts=None, info=None,
                         stream=None, **params):
    """sample_budget_host on cuda tensors (lrt_sample_budget_device): asynchronous on `stream` (a
    torch.cuda.Stream, default: current) and ordered only against it; nothing visits the host.
    variance, color: float32; counts: int32 of >= width * height (default a new [height, width]
    tensor); info: int64 of >= 2, or None. Returns counts."""
    params = dict(params)
    w, h = _frame_size(variance, params)
    d = sample_budget_desc(w, h, min_count, max_count, budget, **params)
    bufs = B.tensor_buffers(variance, "variance", w * h * 4, stream)
    return _sample_budget(bufs, d, variance, color, counts, info, "int64")


def _render_counts(d: L.RenderDesc, counts_ptr, capacity, mean: bool, info_ptr, total_cap: int) -> L.RenderCounts:
    rc = L.RenderCounts()
    rc.counts = counts_ptr
    # default: room for every sample the plane can ask for (frames per pixel), within the ABI's range
    rc.capacity = int(capacity) if capacity is not None else max(1, min(total_cap, L.RC_CAPACITY_MAX))
    rc.flags = L.RC_MEAN if mean else 0
    rc.info = info_ptr
    return rc


def render_counts_host(job: Job, backbuffer: np.ndarray, counts: np.ndarray, capacity: Optional[int] = None,
                       mean: bool = False):
    """Render `job` with a sample count of its own per pixel (lrt_render_counts_host): counts is an
    int32 array of row_count * x_count (the backbuffer's local shape), clamped to 0 .. job.frames;
    capacity: the most samples the call may trace (default: pixels * frames, 2^27 at most) -- a pixel
    whose samples do not fit is skipped; mean: LRT_RC_MEAN. Pixels with no samples keep their
    values. Returns (rays, info) with info = (samples traced, pixels skipped)."""
    d = job.desc()
    npix = d.row_count * d.x_count
    B.HostBuffers().check(backbuffer, "backbuffer", npix * 4)
    B.HostBuffers().check(counts, "counts", npix, ("int32",), exact=True)
    info = np.zeros(2, np.uint64)
    rc = _render_counts(d, counts.ctypes.data, capacity, mean, info.ctypes.data, npix * d.frames)
    rays = ctypes.c_longlong(0)
    L.check(L.lib().lrt_render_counts_host(ctypes.byref(d), ctypes.byref(rc),
                                           backbuffer.ctypes.data_as(ctypes.c_void_p), ctypes.byref(rays)))
    return rays.value, (int(info[0]), int(info[1]))


def render_counts_tensor(job: Job, buf, rays, counts, capacity: Optional[int], mean: bool = False, info=None,
                         stream=None) -> None:
    """torch front end of lrt_render_counts_device: buf and rays as render_tensor takes them, counts
    a cuda int32 tensor of row_count * x_count elements, capacity as render_counts_host (it sizes the
    call's scratch; None: pixels * frames), info a cuda int64 tensor of >= 2 elements or None.
    Asynchronous on `stream` (default: current)."""
    import torch

    d = job.desc()
    npix = d.row_count * d.x_count
    bufs = B.tensor_buffers(buf, "buf", npix * 4, stream)
    bufs.check(buf, "buf", npix * 4)
    if not (getattr(rays, "is_cuda", False) and rays.dtype == torch.int64 and rays.numel() >= 1):
        raise L.LrtError(L.LRT_E_INVALID, "rays must be a cuda int64 tensor")
    bufs.check(counts, "counts", npix, ("int32",), exact=True)
    if info is not None:
        bufs.check(info, "info", 2, ("int64",))
    rc = _render_counts(d, counts.data_ptr(), capacity, mean, info.data_ptr() if info is not None else None,
                        npix * d.frames)
    L.check(L.lib().lrt_render_counts_device(ctypes.byref(d), ctypes.byref(rc), bufs.ptr(buf),
                                             ctypes.c_void_p(rays.data_ptr()), *bufs.tail))


# ---- firefly suppression ---------------------------------------------------------------------
def firefly_desc(width: int, height: int, **params) -> L.FireflyDesc:
    """lrt_firefly_default for a width x height frame, with any of radius, rank, min_taps, gain,
    floor overridden."""
    d = L.FireflyDesc()
    L.check(L.lib().lrt_firefly_default(int(width), int(height), ctypes.byref(d)))
    return _override(d, params, L.FIREFLY_PARAMS, L.FIREFLY_INT_PARAMS, "firefly")


def _firefly(bufs, d, color, ids, out, excess_out, class_out, info) -> dict:
    """An optional output given as True is allocated. Returns {"out"[, "excess"][, "class"][, "info"]}."""
    k = B.planes(d.width, d.height)
    k["info"] = (2, (bufs.uword,), (2,))   # the two counts: uint32 on the host, an int32 tensor
    bufs.check_plane(color, "color", k["quad"])
    if ids is not None:
        bufs.check_plane(ids, "id", k["word"])
    res = {"out": bufs.new(k["quad"]) if out is None else out}
    for name, buf, kind in (("excess", excess_out, "quad"), ("class", class_out, "word"), ("info", info, "info")):
        if buf is not None and buf is not False:
            res[name] = bufs.new(k[kind]) if buf is True else buf
    for name, kind in (("out", "quad"), ("excess", "quad"), ("class", "word"), ("info", "info")):
        if name in res:
            bufs.check_plane(res[name], name if name == "out" or name == "info" else f"{name}_out", k[kind])
    L.check(bufs.entry("firefly")(ctypes.byref(d), bufs.ptr(color), bufs.ptr(ids), bufs.ptr(res["out"]),
                                  bufs.ptr(res.get("excess")), bufs.ptr(res.get("class")), bufs.ptr(res.get("info")),
                                  *bufs.tail))
    return res


def firefly_host(color: np.ndarray, id: Optional[np.ndarray] = None, out: Optional[np.ndarray] = None,
                 excess_out=None, class_out=None, info=None, **params) -> dict:
    """Rank-order firefly suppression of a frame, on host buffers (lrt_firefly_host). color: float32
    [height, width, 4] (or flat with width=, height=), the current frame before the temporal step;
    id: the G-buffer's int32 [height, width] id plane (or the chain's key), or None: every tap in
    the image matches. out: float32 quads, default a new array (never color itself: neighbours are
    read). excess_out (float32 quads: what the clamp took, for a caller that re-adds it), class_out
    (int32 per pixel: 0 kept, 1 clamped, 2 fewer than min_taps counting taps: passed through, 3 not
    finite: grey at the threshold) and info (uint32 of >= 2: the pixels of class 1 and of class 3)
    are written when given; True allocates one. params: radius, rank, min_taps, gain, floor.
    Returns {"out"[, "excess"][, "class"][, "info"]}."""
    params = dict(params)
    w, h = _frame_size(color, params)
    d = firefly_desc(w, h, **params)
    return _firefly(B.HostBuffers(), d, color, id, out, excess_out, class_out, info)


def firefly_tensor(color, id=None, out=None, excess_out=None, class_out=None, info=None, stream=None, **params) -> dict:
    """firefly_host on cuda tensors (lrt_firefly_device): asynchronous on `stream` (a
    torch.cuda.Stream, default: current) and ordered only against it; nothing visits the host. id
    and class_out are int32 tensors, info an int32 tensor of >= 2 elements (the two counts), the
    others float32. Returns {"out"[, "excess"][, "class"][, "info"]}."""
    params = dict(params)
    w, h = _frame_size(color, params)
    d = firefly_desc(w, h, **params)
    bufs = B.tensor_buffers(color, "color", w * h * 4, stream)
    return _firefly(bufs, d, color, id, out, excess_out, class_out, info)


# ---- firefly restore ---------------------------------------------------------------------------
def firefly_restore_desc(width: int, height: int, **params) -> L.FireflyRestoreDesc:
    """lrt_firefly_restore_default for a width x height frame, with radius overridden if given."""
    d = L.FireflyRestoreDesc()
    L.check(L.lib().lrt_firefly_restore_default(int(width), int(height), ctypes.byref(d)))
    return _override(d, params, L.FIREFLY_RESTORE_PARAMS, L.FIREFLY_RESTORE_PARAMS, "firefly restore")


def _firefly_restore(bufs, d, color, excess, ids, out) -> dict:
    k = B.planes(d.width, d.height)
    bufs.check_plane(color, "color", k["quad"])
    bufs.check_plane(excess, "excess", k["quad"])
    if ids is not None:
        bufs.check_plane(ids, "id", k["word"])
    if out is None:
        out = bufs.new(k["quad"])
    bufs.check_plane(out, "out", k["quad"])
    L.check(bufs.entry("firefly_restore")(ctypes.byref(d), bufs.ptr(color), bufs.ptr(excess), bufs.ptr(ids),
                                          bufs.ptr(out), *bufs.tail))
    return {"out": out}


def firefly_restore_host(color: np.ndarray, excess: np.ndarray, id: Optional[np.ndarray] = None,
                         out: Optional[np.ndarray] = None, **params) -> dict:
    """The firefly clamp's excess spread back over its surface and added to a frame, on host buffers
    (lrt_firefly_restore_host). color: float32 [height, width, 4] (or flat with width=, height=), the
    `out` of firefly_host or a later frame of the same size; excess: float32 quads, firefly_host's
    excess_out; id: the int32 [height, width] plane the clamp ran with, or None: every tap in the
    image matches. out: float32 quads, default a new array; out=color means in place. params: radius.
    Returns {"out"}."""
    params = dict(params)
    w, h = _frame_size(color, params)
    return _firefly_restore(B.HostBuffers(), firefly_restore_desc(w, h, **params), color, excess, id, out)


def firefly_restore_tensor(color, excess, id=None, out=None, stream=None, **params) -> dict:
    """firefly_restore_host on cuda tensors (lrt_firefly_restore_device): asynchronous on `stream` (a
    torch.cuda.Stream, default: current) and ordered only against it; nothing visits the host. id is
    an int32 tensor, the others float32; out=color means in place. Returns {"out"}."""
    params = dict(params)
    w, h = _frame_size(color, params)
    d = firefly_restore_desc(w, h, **params)
    return _firefly_restore(B.tensor_buffers(color, "color", w * h * 4, stream), d, color, excess, id, out)
