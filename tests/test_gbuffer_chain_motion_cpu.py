"""The chain motion pass, host side (no GPU): the NumPy restatement (tests/gbuffer_chain_motion_ref.py)
in f32 against f64, an independent f64 check of the answers, the identities, the designed case "flat"
with the temporal step it is for, and the C-ABI's validation (lrt_gbuffer_chain_motion_*), which fires
before any device use."""
import ctypes
import functools
import os

import numpy as np
import pytest

import gbuffer_chain_motion_ref as M
import gbuffer_chain_ref as C
import gbuffer_ref as G
import temporal_gbuffer_ref as TG
from learnraytracing_amd import LrtError, _lib as L
from learnraytracing_amd import (default_camera, default_scene, gbuffer_chain_motion_desc, gbuffer_chain_motion_host,
                                 make_camera)

# the restatement's own f32 - f64 motion gaps in pixels off the fragile mask, per size
# (`python tests/gbuffer_chain_motion_ref.py`); tests/test_gpu_gbuffer_chain_motion.py takes 16 x these
F32_F64_GAP = {(19, 13): 1.7e-5,     # measured: 1.61e-05 (orbit and both), 1.09e-05 (moved)
               (67, 45): 8.0e-5,     # measured: 6.92e-05, 7.81e-05, 7.38e-05
               (160, 90): 3.3e-4}    # measured: 1.86e-04, 3.17e-04, 2.61e-04
F32_F64_GAP_FLAT = 1.3e-5            # measured: 1.20e-05
MAX_FRAGILE = 0.05                   # of the followed pixels: a cap (measured: at most 1.36 %)
CONVERGED_PX = M.DEFAULTS["converged_px"]

CASES = dict(M.shape_cases(default_scene, make_camera))


def _gpu_present():
    import torch
    return torch.cuda.device_count() > 0


@functools.lru_cache(maxsize=None)
def _pair(label):
    return M.pair(M.flat_case(make_camera) if label == "flat" else CASES[label])


def _case(label):
    return M.flat_case(make_camera) if label == "flat" else CASES[label]


@pytest.mark.parametrize("label", list(CASES))
def test_f32_against_f64(label):
    """Status is equal off the mask, the mask covers at most 5 % of the followed pixels, and the motion
    gap stays within its record."""
    kw = CASES[label]
    a, b, fragile = _pair(label)
    fol = M.followed(a) | M.followed(b)
    share = (fragile & fol).sum() / max(1, fol.sum())
    gap = M.motion_gap(a, b, ~fragile)
    differ = (a["status"] != b["status"])
    print(f"{label}: gap {gap:.3g} px, fragile {100 * share:.2f} % of {fol.sum()} followed, status differs at "
          f"{differ.sum()} px ({(differ & ~fragile).sum()} off the mask), {np.bincount(a['status'].ravel(), minlength=6).tolist()}")
    assert not (differ & ~fragile).any()
    assert share <= MAX_FRAGILE
    assert gap <= F32_F64_GAP[(kw["w"], kw["h"])]
    assert np.array_equal(M.followed(a), M.followed(b))
    if kw["w"] >= 67:                                       # the search has something to do
        assert (a["status"] == M.CONVERGED).sum() >= 0.8 * fol.sum()
    # outside CONVERGED the plane is the copy, inside z is kept and w is 1, in both runs
    for out in (a, b):
        conv = out["status"] == M.CONVERGED
        assert np.array_equal(out["motion"][~conv].astype(np.float32).view(np.uint32), kw["first_motion"][~conv].view(np.uint32))
        assert np.array_equal(out["motion"][conv][:, 2], kw["first_motion"][conv][:, 2]) and (out["motion"][conv][:, 3] == 1).all()


@pytest.mark.parametrize("label", list(CASES) + ["flat"])
def test_independent_check_of_the_answer(label):
    """At every CONVERGED pixel of the f32 run, the f64 chain at (x + mx, y + my) under the previous
    camera and scene has the pixel's key, and a fresh f64 Gauss-Newton step there (its own Jacobian,
    probe 0.125 px, solved by least squares) is at most 2 converged_px long: the remaining step the
    search accepted is an estimate with the last iteration's Jacobian, hence the factor."""
    kw = _case(label)
    a, _, _ = _pair(label)
    conv = a["status"] == M.CONVERGED
    k0, K, length = M.independent_step(kw, a["motion"])
    assert np.array_equal(k0[conv], K[conv])
    assert not np.isnan(length[conv]).any()
    worst = float(length[conv].max()) if conv.any() else 0.0
    print(f"{label}: {conv.sum()} converged, largest fresh step {worst:.3g} px, largest accepted {float(a['rem'][conv].max() if conv.any() else 0):.3g}")
    assert worst <= 2 * CONVERGED_PX


def test_first_hit_motion_fails_the_check_on_flat():
    """The vector every stage used before fails the same check at every converged pixel of the
    near-flat mirror: a fresh step from where it points is 1.29 to 1.40 px long here (median 1.39;
    the issue's prototype quotes about 2 px), twenty times the 2 converged_px the answers stay within."""
    kw = M.flat_case(make_camera)
    a, _, _ = _pair("flat")
    conv = a["status"] == M.CONVERGED
    _, _, length = M.independent_step(kw, kw["first_motion"])
    ok = conv & ~np.isnan(length)
    print(f"flat: first-hit motion, fresh step median {np.median(length[ok]):.3g} px, min {length[ok].min():.3g}, max {length[ok].max():.3g}")
    assert ok.sum() >= 0.9 * conv.sum()
    assert (length[ok] > 2 * CONVERGED_PX).all()
    assert 1.0 <= np.median(length[ok]) <= 2.5


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_identities(dtype):
    w, h = 67, 45
    s, m = default_scene()
    cam, pcam = G.camera_pair(make_camera, w, h)
    # static camera and scene: motion is first_motion in all bits at all pixels
    for prev_s in (None, G.sphere_array(s)):
        kw = M.make_case(w, h, cam, cam, s, m, prev_s)
        out, _ = M.chain_motion(dtype=dtype, **kw)
        assert np.array_equal(out["motion"].astype(np.float32).view(np.uint32), kw["first_motion"].view(np.uint32))
        assert (np.abs(out["motion"][..., :2]) == 0).all()
        # (a silhouette pixel whose probe leaves the key is KEY_LOST in a static frame too)
        assert set(np.unique(out["status"])) <= {M.NOT_FOLLOWED, M.CONVERGED, M.KEY_LOST}
        assert (out["status"] == M.CONVERGED).sum() >= 0.8 * M.followed(out).sum()
        assert (out["rem"] == 0).all()
    # max_bounces 0: nothing is followed, the plane is the copy
    kw = M.make_case(w, h, cam, pcam, s, m, G.moved_scene(s), max_bounces=0)
    out, _ = M.chain_motion(dtype=dtype, **kw)
    assert np.isin(out["status"], (M.NOT_FOLLOWED, M.UNRESOLVED)).all()
    assert np.array_equal(out["motion"].astype(np.float32).view(np.uint32), kw["first_motion"].view(np.uint32))
    # non-followed pixels are the copy under any camera pair
    kw = M.make_case(w, h, cam, make_camera((1.0, 2.5, 2.0), (0.1, 0.0, 0.0), (0.0, 1.0, 0.0), 50.0, w / h, 0.0, 3.0), s, m)
    out, _ = M.chain_motion(dtype=dtype, **kw)
    not_followed = out["status"] == M.NOT_FOLLOWED
    assert not_followed.sum() > 2000 and (~not_followed).sum() > 300
    assert np.array_equal(out["motion"][not_followed].astype(np.float32).view(np.uint32), kw["first_motion"][not_followed].view(np.uint32))


def test_flat_reproduces_the_prototype():
    """777 followed and 736 converged, as the issue's prototype; |motion - first-hit motion| is 1.35 px
    in the mean here (1.28 to 1.42; the prototype quotes about 1.0 px at 37 x 21, and 2.1 px for the
    same miss elsewhere), and test_independent_check_of_the_answer holds these answers to 0.125 px."""
    kw = M.flat_case(make_camera)
    a, b, fragile = _pair("flat")
    assert M.motion_gap(a, b, ~fragile) <= F32_F64_GAP_FLAT
    assert not ((a["status"] != b["status"]) & ~fragile).any()
    conv = a["status"] == M.CONVERGED
    fol = M.followed(a)
    moved = np.linalg.norm((a["motion"] - kw["first_motion"])[..., :2], axis=-1)[conv]
    print(f"flat: {fol.sum()} followed, {conv.sum()} converged, |motion - first| mean {moved.mean():.3g} px, max {moved.max():.3g}")
    assert abs(int(fol.sum()) - 777) <= 8 and abs(int(conv.sum()) - 736) <= 15
    assert 0.5 <= moved.mean() <= 2.1


def test_flat_temporal_step_improves_tenfold():
    a, _, _ = _pair("flat")
    kw = M.flat_case(make_camera)

    def step(color, cur, prev_g, prev):
        info = {}
        out, _ = TG.step(color, cur, prev_g, prev, np.float32, info=info)
        return (out["color"], info["keep"]) if prev is not None else (TG.as_state(out), None)

    errs, keeps = M.flat_temporal_ratio(make_camera, step, (kw["first_motion"], a["motion"]))
    on = (a["status"] == M.CONVERGED) & keeps[0] & keeps[1]
    ratio = errs[1][on].mean() / errs[0][on].mean()
    print(f"flat: {on.sum()} px, mean error first-hit {errs[0][on].mean():.3g}, new {errs[1][on].mean():.3g}, ratio {ratio:.3g}")
    assert on.sum() >= 600
    assert ratio <= 0.1


def test_flat_moved_branches():
    """NO_SEED and the carry-back: the left sphere did not exist in the previous frame, the right one
    moved and changed its radius, and first_motion carries w = 0, a NaN and 2e6 px at 18 pixels."""
    kw = M.flat_moved_case(make_camera)
    a, b, fragile = M.pair(kw)
    assert not ((a["status"] != b["status"]) & ~fragile).any() and fragile.mean() <= 0.01
    assert M.motion_gap(a, b, ~fragile) <= F32_F64_GAP_FLAT
    poked = np.zeros(a["status"].shape, bool)
    for where in (M.FLAT_POKED_W0, M.FLAT_POKED_NAN, M.FLAT_POKED_FAR):
        poked[where] = True
    w, h = kw["w"], kw["h"]
    ys, xs = np.mgrid[0:h, 0:w]
    _, j, _, _, _ = M.chain_at(w, h, kw["camera"], kw["spheres"], C.material_arrays(kw["materials"]),
                               xs.astype(np.float32), ys.astype(np.float32), 4, 0.25, np.float32)
    assert poked.sum() == 18 and (j == 1).sum() >= 20 and (j == 2).sum() >= 20
    assert np.array_equal(a["status"] == M.NO_SEED, (j == 1) | poked)
    conv = a["status"] == M.CONVERGED
    assert (j[conv] == 2).sum() >= 10                       # found through the carried-back point
    assert np.array_equal(a["motion"][~conv].astype(np.float32).view(np.uint32), kw["first_motion"][~conv].view(np.uint32))
    k0, K, length = M.independent_step(kw, a["motion"])
    assert np.array_equal(k0[conv], K[conv]) and np.nanmax(length[conv]) <= 2 * CONVERGED_PX
    assert not np.isnan(length[conv]).any()


# ---- the C-ABI
def test_struct_layouts():
    assert ctypes.sizeof(L.GbufferChainMotionDesc) == 16 + 2 * 88 + 32 == 224
    assert L.GbufferChainMotionDesc.prev_camera.offset == 104 and L.GbufferChainMotionDesc.max_bounces.offset == 192
    assert ctypes.sizeof(L.GbufferChainMotion) == 2 * ctypes.sizeof(ctypes.c_void_p)
    assert (L.CM_NOT_FOLLOWED, L.CM_CONVERGED, L.CM_UNRESOLVED, L.CM_NO_SEED, L.CM_KEY_LOST, L.CM_NOT_CONVERGED) == \
        (M.NOT_FOLLOWED, M.CONVERGED, M.UNRESOLVED, M.NO_SEED, M.KEY_LOST, M.NOT_CONVERGED)
    src = open(L.HEADER_PATH).read()
    for name, v in zip(("NOT_FOLLOWED", "CONVERGED", "UNRESOLVED", "NO_SEED", "KEY_LOST", "NOT_CONVERGED"), range(6)):
        assert f"#define LRT_CM_{name} {v} " in src
    cam, pcam = G.camera_pair(make_camera, 16, 9)
    d = gbuffer_chain_motion_desc(16, 9, cam, pcam)
    assert (d.width, d.height, d.flags, d.reserved, d.reserved2, d.reserved3) == (16, 9, 0, 0, 0, 0)
    assert (d.max_bounces, d.roughness_max, d.iterations, d.probe_px, d.step_max_px, d.converged_px) == \
        tuple(M.DEFAULTS[k] for k in L.GBUFFER_CHAIN_MOTION_PARAMS)
    assert bytes(d.camera) == bytes(cam) and bytes(d.prev_camera) == bytes(pcam)
    assert bytes(gbuffer_chain_motion_desc(16, 9, cam).prev_camera) == bytes(cam)
    d = gbuffer_chain_motion_desc(16, 9, cam, pcam, iterations=5, probe_px=0.5, max_bounces=2)
    assert (d.iterations, d.probe_px, d.max_bounces) == (5, 0.5, 2)
    with pytest.raises(LrtError):
        gbuffer_chain_motion_desc(16, 9, cam, pcam, probe=0.5)
    with pytest.raises(LrtError):
        gbuffer_chain_motion_desc(0, 9, cam)


def test_validation_before_device_use():
    """Every invalid argument is LRT_E_INVALID before any device use, host and device entry points
    alike; a valid call without lrt_initialize() is LRT_E_STATE."""
    lib = L.lib()
    w, h = 16, 9
    cam, pcam = G.camera_pair(make_camera, w, h)
    first = np.zeros((h, w, 4), np.float32)
    motion = np.zeros((h, w, 4), np.float32)
    status = np.zeros((h, w), np.int32)
    ptr = lambda a: a.ctypes.data   # noqa: E731
    d = L.GbufferChainMotionDesc()
    dflt = lib.lrt_gbuffer_chain_motion_default
    assert dflt(w, h, ctypes.byref(cam), ctypes.byref(pcam), ctypes.byref(d)) == 0
    assert dflt(w, h, None, ctypes.byref(pcam), ctypes.byref(d)) == L.LRT_E_INVALID
    assert dflt(w, h, ctypes.byref(cam), ctypes.byref(pcam), None) == L.LRT_E_INVALID
    assert dflt(w, 0, ctypes.byref(cam), ctypes.byref(pcam), ctypes.byref(d)) == L.LRT_E_INVALID
    assert dflt(w, h, ctypes.byref(cam), ctypes.byref(pcam), ctypes.byref(d)) == 0

    def planes(**kw):
        g = L.GbufferChainMotion()
        g.motion, g.status = ptr(motion), ptr(status)
        for k, v in kw.items():
            setattr(g, k, v)
        return g

    def desc(**kw):
        dd = L.GbufferChainMotionDesc.from_buffer_copy(d)
        for k, v in kw.items():
            setattr(dd, k, v)
        return dd

    def calls(dd, g, fm=ptr(first), sm=None):
        ref = lambda x: ctypes.byref(x) if x is not None else None   # noqa: E731
        return (lib.lrt_gbuffer_chain_motion_host(ref(dd), ref(sm), fm, ref(g)),
                lib.lrt_gbuffer_chain_motion_device(ref(dd), ref(sm), fm, ref(g), None))

    inv = (L.LRT_E_INVALID, L.LRT_E_INVALID)
    assert calls(None, planes()) == inv
    assert calls(d, None) == inv
    assert calls(d, L.GbufferChainMotion()) == inv                               # both planes NULL
    for kw in (dict(width=0), dict(height=0), dict(width=-3), dict(width=1 << 15, height=1 << 15),
               dict(flags=1), dict(reserved=1), dict(reserved2=1), dict(reserved3=1)):
        assert calls(desc(**kw), planes()) == inv, kw
    for kw in (dict(max_bounces=-1), dict(max_bounces=L.CHAIN_MAX_BOUNCES + 1)):
        assert calls(desc(**kw), planes()) == inv, kw
    assert "max_bounces" in lib.lrt_last_error().decode()
    for v in (-0.5, float("nan"), float("inf")):
        assert calls(desc(roughness_max=v), planes()) == inv, v
    assert "roughness_max" in lib.lrt_last_error().decode()
    for v in (0, -1, L.CM_MAX_ITERATIONS + 1):
        assert calls(desc(iterations=v), planes()) == inv, v
    assert "iterations" in lib.lrt_last_error().decode()
    for name in ("probe_px", "step_max_px", "converged_px"):
        for v in (0.0, -1.0, float("nan"), float("inf")):
            assert calls(desc(**{name: v}), planes()) == inv, (name, v)
        assert name in lib.lrt_last_error().decode()
    # a prev_camera that lrt_temporal_* rejects: no horizontal span
    bad = L.Camera.from_buffer_copy(pcam)
    bad.horizontalVec = L.f3(0.0, 0.0, 0.0)
    assert calls(desc(prev_camera=bad), planes()) == inv
    assert "prev_camera" in lib.lrt_last_error().decode()
    assert calls(d, planes(), fm=None) == inv                                    # first_motion is required
    assert "first_motion" in lib.lrt_last_error().decode()
    # any output overlapping first_motion or the other output, by address range
    assert calls(d, planes(motion=ptr(first))) == inv
    assert calls(d, planes(motion=ptr(first) + 16 * w * h - 16)) == inv          # its last quad
    assert calls(d, planes(status=ptr(first) + 16)) == inv
    assert "first_motion" in lib.lrt_last_error().decode()
    assert calls(d, planes(status=ptr(first) + 16 * w * h - 4)) == inv           # its last word
    assert calls(d, planes(status=ptr(motion))) == inv
    assert calls(d, planes(status=ptr(motion) + 16 * w * h - 4)) == inv
    assert "alias" in lib.lrt_last_error().decode()
    # scene: lrt_gbuffer_device's checks, and at most 16 spheres
    def scene(cur, prev, **kw):
        sm = L.SceneMotion()
        sm._keep = (np.ascontiguousarray(cur, np.float32), np.ascontiguousarray(prev, np.float32))
        sm.spheres = ctypes.cast(sm._keep[0].ctypes.data, ctypes.POINTER(L.Sphere))
        sm.prev_spheres = ctypes.cast(sm._keep[1].ctypes.data, ctypes.POINTER(L.Sphere))
        sm.count = len(cur)
        for k, v in kw.items():
            setattr(sm, k, v)
        return sm

    s9 = G.sphere_array(default_scene()[0])
    s17 = np.concatenate([s9, s9[:8] + np.float32([10, 0, 0, 0])])
    assert calls(d, planes(), sm=scene(s17, s17)) == inv                         # 17 spheres
    assert "16" in lib.lrt_last_error().decode()
    assert calls(d, planes(), sm=scene(s9, s9, count=0)) == inv
    assert calls(d, planes(), sm=scene(s9, s9, reserved=1)) == inv
    assert calls(d, planes(), sm=scene(s9, s9, prev_spheres=None)) == inv
    nan = s9.copy()
    nan[3, 1] = np.nan
    assert calls(d, planes(), sm=scene(s9, nan)) == inv
    if os.environ.get("HIP_VISIBLE_DEVICES") == "" or not _gpu_present():
        # (an uninitialised library holds no scene: any `scene` is refused)
        assert calls(d, planes(), sm=scene(s9, G.moved_scene(s9))) == inv
        st = (L.LRT_E_STATE, L.LRT_E_STATE)
        assert calls(d, planes()) == st
        assert calls(d, planes(motion=None)) == st and calls(d, planes(status=None)) == st
        for kw in (dict(max_bounces=0), dict(iterations=1), dict(iterations=L.CM_MAX_ITERATIONS), dict(width=4, height=2),
                   dict(probe_px=1e-3), dict(step_max_px=1e4)):
            assert calls(desc(**kw), planes()) == st, kw
        # adjacent is not overlapping
        both = np.zeros((2, h, w, 4), np.float32)
        assert calls(d, planes(motion=ptr(both) + 16 * w * h), fm=ptr(both)) == st
        assert calls(d, planes(motion=ptr(both) + 16 * w * h - 4), fm=ptr(both)) == inv


def test_front_end_argument_checks():
    w, h = 16, 9
    cam = default_camera(w, h)
    first = np.zeros((h, w, 4), np.float32)
    for bad in (dict(out={"motions": np.zeros((h, w, 4), np.float32)}),          # an unknown plane
                dict(out={"motion": np.zeros((h, w, 4), np.float64)}),
                dict(out={"status": np.zeros((h, w), np.float32)}),
                dict(out={"status": np.zeros((h, w - 1), np.int32)}),
                dict(out={"motion": np.zeros((h, w, 4), np.float32)[:, ::2]}),
                dict(out={}), dict(motion=False, status=False),
                dict(first_motion=np.zeros((h, w, 3), np.float32)), dict(first_motion=np.zeros((h, w, 4), np.float64)),
                dict(spheres=G.sphere_array(default_scene()[0])),                 # spheres needs prev_spheres
                dict(iterations=9), dict(probe_px=0.0), dict(max_bounces=17), dict(no_such_parameter=1)):
        args = dict(first_motion=first)
        args.update(bad)
        with pytest.raises(LrtError) as e:
            gbuffer_chain_motion_host(w, h, cam, None, **args)
        assert e.value.code == L.LRT_E_INVALID, bad
