"""The G-buffer pass, host side (no GPU): its NumPy restatement (tests/gbuffer_ref.py) tied to the
library's own closest hit (lrt_accel_eval, the host build of the device walk) bit for bit, the
restatement's f32 - f64 gap held to the values tests/test_gpu_gbuffer.py derives its tolerances
from, a motion case with a known answer, the designed cases' branches, and the C-ABI's validation
(lrt_gbuffer_*), which fires before any device use."""
import ctypes
import os

import numpy as np
import pytest

import gbuffer_ref as G
import temporal_ref as R
from learnraytracing_amd import LrtError, _lib as L
from learnraytracing_amd import (default_camera, default_scene, gbuffer_desc, gbuffer_host, make_camera,
                                 random_scene)

# the restatement's own f32 - f64 gaps off the fragile mask (`python tests/gbuffer_ref.py`), as
# tests/test_gpu_gbuffer.py records them
F32_F64_GAP = 2e-4                          # measured: 1.89e-04 (the default scene at SHAPES; counts up to 17: 1.09e-04)
F32_F64_GAP_COUNT = {1000: 3.1e-3, 4096: 4e-2}   # measured: 3.04e-03, 3.90e-02 (HitSphere's cancellation on r = 0.05)
F32_F64_GAP_DESIGNED = 1.1e-5               # measured: 1.01e-05
MAX_FRAGILE = 0.02


def _gpu_present():
    import torch
    return torch.cuda.device_count() > 0


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _accel(spheres, rays, accel):
    sa = (L.Sphere * len(spheres))(*spheres)
    ids, ts = np.zeros(len(rays), np.int32), np.zeros(len(rays), np.float32)
    L.check(L.lib().lrt_accel_eval(sa, len(spheres), rays.ctypes.data, len(rays), accel, 0, ids.ctypes.data,
                                   ts.ctypes.data))
    return ids, ts


CASES = G.gap_cases(default_scene, random_scene, make_camera)


@pytest.mark.parametrize("label,kw", CASES, ids=[c[0] for c in CASES])
def test_restatement_is_the_librarys_closest_hit(label, kw):
    """The f32 restatement's id and t against lrt_accel_eval's host walk of the grid on the same
    rays (O, D): ids bit for bit, t bit for bit on hits."""
    w, h, cam, spheres = kw["w"], kw["h"], kw["camera"], kw["spheres"]
    got, _ = G.gbuffer(w, h, cam, spheres, kw["albedo"], motion=False, dtype=np.float32)
    ids, ts = _accel(spheres, G.accel_rays(w, h, cam), 2)
    ids, ts = ids.reshape(h, w), ts.reshape(h, w)
    assert got["depth"].dtype == np.float32
    assert np.array_equal(got["id"], ids)
    hit = ids >= 0
    assert np.array_equal(_bits(got["depth"][hit]), _bits(ts[hit]))
    assert np.isposinf(got["depth"][~hit]).all()
    if w * h > 100 and len(spheres) > 1:
        assert hit.any() and len(np.unique(ids)) >= 3


def test_f32_f64_gap_within_its_record():
    """The gap the GPU test's tolerances are 16 x of, per family; the fragile share and the f32 / f64
    id differences the issue quotes (at most 0.1 %; none off the mask)."""
    for label, kw in CASES:
        gap, report = G.f32_f64_gap([(label, kw)])
        share, differ, differ_ok = report[label]
        bound = F32_F64_GAP_COUNT.get(len(kw["spheres"]), F32_F64_GAP)
        print(f"{label}: gap {gap:.3g} (recorded {bound:.3g}), fragile {100 * share:.2f} %, ids differ {differ}")
        assert gap <= bound, label
        assert share <= 0.001 and differ_ok == 0, label
        if kw["w"] * kw["h"] <= 15:
            assert share == 0
    for name in G.DESIGNED_CASES:
        gap, report = G.f32_f64_gap([(name, G.designed_case(name, make_camera))])
        assert gap <= F32_F64_GAP_DESIGNED and report[name][0] <= MAX_FRAGILE and report[name][2] == 0, name


def test_analytic_motion():
    """Camera along -z, sphere B translated parallel to the image plane: the displacement of a point
    at depth z is -dx h / (2 tan(vfov / 2) z) pixels along x and none along y; A and the sky, which
    did not move, take their own centre exactly."""
    kw = G.designed_case("analytic", make_camera)
    # f64: the camera's own floats are f32 (tanf, kPI = 3.1415926f): a few 2^-24 of two pixels
    for T, tol in ((np.float64, 1e-6), (np.float32, 16 * F32_F64_GAP_DESIGNED)):
        out, fragile = G.gbuffer(dtype=T, **kw)
        assert not fragile.any()
        mv, on_b = out["motion"], out["id"] == 1
        assert on_b.sum() > 50 and (out["id"] == 0).sum() > 50 and (out["id"] == -1).sum() > 50
        depth = 3.0 - np.float64(out["world_pos"][..., 2])
        assert R.rel_gap(mv[..., 0][on_b], G.analytic_displacement(kw["h"], depth)[on_b]) <= tol
        assert np.abs(mv[..., 1][on_b]).max() <= tol
        assert (mv[..., 3] == 1).all() and np.array_equal(mv[..., 2], out["id"])
        assert (mv[..., :2][~on_b] == 0).all()


def test_designed_cases_hold_their_branches():
    w, h = G.DESIGNED_SIZE
    out = {name: G.gbuffer(dtype=np.float64, **G.designed_case(name, make_camera))[0] for name in G.DESIGNED_CASES}
    ids = out["static"]["id"]
    assert all((ids == i).sum() > 50 for i in (-1, 0, 1))
    for name in ("static", "static_scene"):             # hits and misses alike: their own centre
        assert (out[name]["motion"][..., :2] == 0).all() and (out[name]["motion"][..., 3] == 1).all()
    assert np.array_equal(out["static"]["motion"], out["static_scene"]["motion"])
    m = out["moved"]["motion"]
    assert (m[..., 3] == 1).all() and (np.abs(m[..., :2]) > 0.5).any(-1)[ids >= 0].mean() > 0.9
    assert (np.abs(m[..., :2][ids < 0]) < 3).all()       # the sky moves with the camera only
    for name in ("behind", "gone"):
        m = out[name]["motion"]
        assert (m[ids == 1] == np.float64([0, 0, 1, 0])).all(), name
        assert (m[..., 3][ids != 1] == 1).all(), name
    for name in G.DESIGNED_CASES:                        # the planes do not depend on the previous frame
        for plane in G.GUIDES + ("id", "depth"):
            assert np.array_equal(out[name][plane], out["static"][plane])
    k = G.gbuffer(dtype=np.float64, guide_scale=0.25, **G.designed_case("moved", make_camera))[0]
    for plane in G.GUIDES:
        assert np.array_equal(k[plane], 0.25 * out["moved"][plane])
    for plane in ("id", "depth", "motion"):
        assert np.array_equal(k[plane], out["moved"][plane])


# ---- the C-ABI
def test_struct_layouts():
    assert ctypes.sizeof(L.GbufferDesc) == 16 + 2 * 88 + 8 == 200
    assert L.GbufferDesc.camera.offset == 16 and L.GbufferDesc.guide_scale.offset == 192
    assert ctypes.sizeof(L.Gbuffer) == 6 * ctypes.sizeof(ctypes.c_void_p)
    d = gbuffer_desc(16, 9, default_camera(16, 9))
    assert (d.width, d.height, d.flags, d.reserved, d.reserved2, d.guide_scale) == (16, 9, 0, 0, 0, 1.0)
    assert bytes(d.camera) == bytes(d.prev_camera) == bytes(default_camera(16, 9))
    assert gbuffer_desc(16, 9, default_camera(16, 9), guide_scale=0.5).guide_scale == 0.5
    with pytest.raises(LrtError):
        gbuffer_desc(0, 9, default_camera(16, 9))
    with pytest.raises(LrtError):
        gbuffer_desc(16, 9, None)


def test_validation_before_device_use():
    """Every invalid argument is LRT_E_INVALID before any device use, host and device entry points
    alike; a valid call without lrt_initialize() is LRT_E_STATE."""
    lib = L.lib()
    w, h = 16, 9
    cam = default_camera(w, h)
    rgba = [np.zeros((h, w, 4), np.float32) for _ in range(4)]
    idp, depth = np.zeros((h, w), np.int32), np.zeros((h, w), np.float32)
    ptr = lambda a: a.ctypes.data   # noqa: E731
    d = L.GbufferDesc()
    assert lib.lrt_gbuffer_default(w, h, ctypes.byref(cam), None, ctypes.byref(d)) == 0
    assert lib.lrt_gbuffer_default(w, h, None, None, ctypes.byref(d)) == L.LRT_E_INVALID
    assert lib.lrt_gbuffer_default(w, h, ctypes.byref(cam), None, None) == L.LRT_E_INVALID
    assert lib.lrt_gbuffer_default(0, h, ctypes.byref(cam), None, ctypes.byref(d)) == L.LRT_E_INVALID

    def planes(**kw):
        g = L.Gbuffer()
        g.normal, g.world_pos, g.albedo, g.motion = (ptr(b) for b in rgba)
        g.id, g.depth = ptr(idp), ptr(depth)
        for k, v in kw.items():
            setattr(g, k, v)
        return g

    def desc(**kw):
        dd = L.GbufferDesc.from_buffer_copy(d)
        for k, v in kw.items():
            setattr(dd, k, v)
        return dd

    sph = (L.Sphere * 3)(L.Sphere(L.f3(0, 0, 0), 1.0), L.Sphere(L.f3(2, 0, 0), 0.5), L.Sphere(L.f3(0, 3, 0), 0.25))
    psph = (L.Sphere * 3)(*sph)

    def scene(**kw):
        sm = L.SceneMotion()
        sm.spheres, sm.prev_spheres, sm.count = sph, psph, 3
        for k, v in kw.items():
            setattr(sm, k, v)
        return sm

    def calls(dd, sm, g):
        ref = lambda x: ctypes.byref(x) if x is not None else None   # noqa: E731
        return (lib.lrt_gbuffer_host(ref(dd), ref(sm), ref(g)), lib.lrt_gbuffer_device(ref(dd), ref(sm), ref(g), None))

    inv = (L.LRT_E_INVALID, L.LRT_E_INVALID)
    assert calls(None, None, planes()) == inv
    assert calls(d, None, None) == inv
    assert calls(d, None, L.Gbuffer()) == inv                                   # all six planes NULL
    for kw in (dict(width=0), dict(height=0), dict(width=-3), dict(width=1 << 15, height=1 << 15),
               dict(flags=1), dict(reserved=1), dict(reserved2=1), dict(guide_scale=0.0), dict(guide_scale=-1.0),
               dict(guide_scale=float("nan")), dict(guide_scale=float("inf"))):
        assert calls(desc(**kw), None, planes()) == inv, kw
    assert "guide_scale" in lib.lrt_last_error().decode()
    # any two planes overlapping, by address range (the id and depth planes are a quarter as long)
    names = [f[0] for f in L.Gbuffer._fields_]
    for i, a in enumerate(names):
        for b in names[i + 1:]:
            assert calls(d, None, planes(**{b: getattr(planes(), a)})) == inv, (a, b)
    assert calls(d, None, planes(world_pos=ptr(rgba[0]) + 16)) == inv           # a partial overlap
    assert calls(d, None, planes(depth=ptr(rgba[2]) + 16 * w * h - 4)) == inv   # the last word of albedo
    assert calls(d, None, planes(id=ptr(idp), depth=ptr(idp) + 4 * w * h - 4)) == inv
    assert "alias" in lib.lrt_last_error().decode()
    # with motion: a prev_camera that lrt_temporal_* rejects (without motion it is not read)
    bad = desc()
    bad.prev_camera.horizontalVec = L.f3(0, 0, 0)
    assert calls(bad, None, planes()) == inv
    bad = desc()
    bad.prev_camera.lowerLeftCorner = bad.prev_camera.origin                    # no focus distance
    assert calls(bad, None, planes()) == inv
    bad = desc()
    bad.prev_camera.verticalVec = L.f3(float("nan"), 0, 0)
    assert calls(bad, None, planes()) == inv
    # with a scene
    null = ctypes.POINTER(L.Sphere)()
    assert calls(d, scene(spheres=null), planes()) == inv
    assert calls(d, scene(prev_spheres=null), planes()) == inv
    assert calls(d, scene(reserved=1), planes()) == inv
    for count in (0, -1, L.MAX_SPHERES + 1):
        assert calls(d, scene(count=count), planes()) == inv, count
    for arr in (sph, psph):
        for v in (float("nan"), float("inf")):
            keep = arr[1].radius
            arr[1].radius = v
            assert calls(d, scene(), planes()) == inv
            assert "finite" in lib.lrt_last_error().decode()
            arr[1].radius = keep
            keep = arr[2].center.y
            arr[2].center.y = v
            assert calls(d, scene(), planes()) == inv
            arr[2].center.y = keep
    # a count other than the current scene's (3 is neither the default scene's 9 nor, without
    # lrt_initialize(), no scene's 0), and spheres that are not the current scene's
    assert calls(d, scene(), planes()) == inv
    assert "current scene" in lib.lrt_last_error().decode()
    nine = (L.Sphere * 9)(*default_scene()[0])
    nine[4].center.x += 0.25
    assert calls(d, scene(spheres=nine, prev_spheres=nine, count=9), planes()) == inv
    assert "current scene" in lib.lrt_last_error().decode()
    if os.environ.get("HIP_VISIBLE_DEVICES") == "" or not _gpu_present():
        st = (L.LRT_E_STATE, L.LRT_E_STATE)
        assert calls(d, None, planes()) == st
        for name in names:                                                       # every member is optional
            assert calls(d, None, planes(**{name: None})) == st, name
            only = L.Gbuffer()
            setattr(only, name, getattr(planes(), name))
            assert calls(d, None, only) == st, name
        bad = desc()
        bad.prev_camera.horizontalVec = L.f3(0, 0, 0)
        assert calls(bad, None, planes(motion=None)) == st                       # read only with motion
        assert calls(desc(width=4, height=2), None, planes()) == st


def test_front_end_argument_checks():
    w, h = 16, 9
    cam = default_camera(w, h)
    for bad in (dict(out={"normals": np.zeros((h, w, 4), np.float32)}),          # an unknown plane
                dict(out={"normal": np.zeros((h, w, 4), np.float64)}),
                dict(out={"id": np.zeros((h, w), np.float32)}),
                dict(out={"depth": np.zeros((h, w - 1), np.float32)}),
                dict(out={"normal": np.zeros((h, w, 4), np.float32)[:, ::2]}),
                dict(spheres=np.zeros((3, 4), np.float32))):                     # spheres without prev_spheres
        with pytest.raises(LrtError) as e:
            gbuffer_host(w, h, cam, **bad)
        assert e.value.code == L.LRT_E_INVALID, bad
    with pytest.raises(LrtError) as e:
        gbuffer_host(w, h, cam, out={})
    assert e.value.code == L.LRT_E_INVALID
