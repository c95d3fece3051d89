"""Temporal accumulation under moving spheres, host side (no GPU): the C-ABI's validation
(lrt_temporal_accumulate_moving_*), the Python front end's argument checks, and the rule itself --
its NumPy restatement (tests/temporal_motion_ref.py): equal to the static restatement where nothing
moves, every branch of the designed sphere cases populated, an analytic displacement, and what it is
for (a translated Lambert sphere keeps its history, in f64 on the oracle's frames)."""
import ctypes
import os

import numpy as np
import pytest

import oracle
import temporal_motion_ref as M
import temporal_ref as R
from learnraytracing_amd import LrtError, _lib as L
from learnraytracing_amd import default_camera, make_camera, temporal_accumulate_moving_host

CUR = ("normal", "world_pos", "albedo")
MAX_FRAGILE = 0.02            # tests/test_gpu_temporal.py's
# the restatement's own f32 - f64 gaps (`python tests/temporal_motion_ref.py`), as
# tests/test_gpu_temporal_motion.py records them
F32_F64_GAP, F32_F64_GAP_STD = 7e-5, 3.3e-5                        # measured: 6.71e-05, 3.17e-05
F32_F64_GAP_DESIGNED, F32_F64_GAP_STD_DESIGNED = 2.3e-5, 2.3e-5    # measured: 2.2e-05, 2.16e-05
F32_F64_GAP_COUNT = 5.5e-6                                         # measured: 5.23e-06 (color_std: 0, every pixel is reset)
S0, M0 = oracle.default_scene_arrays()


def _gpu_present():
    import torch
    return torch.cuda.device_count() > 0


def _n(mask):
    return int(np.count_nonzero(mask))


def _render(w, h, camera, frame0, spheres=None, depth=8):
    """One fresh 1 spp frame and its features through the oracle: sample frame0 into zeroed buffers."""
    feats = {n: np.zeros((h, w, 4), np.float32) for n in CUR}
    sp = S0 if spheres is None else np.float32(spheres).ravel()
    buf, _ = oracle.orc_render_ex(w, h, frames=1, depth=depth, frame0=frame0, cam22=R.cam22(camera),
                                  features=feats, max_frame=-1, spheres=sp, mats=M0)
    return buf, feats


# ---- the C-ABI
def test_moving_validation_before_device_use():
    """Everything the static call rejects, and the scene's own cases, are LRT_E_INVALID before any
    device use, host and device entry points alike; a valid call without lrt_initialize() is
    LRT_E_STATE, radii <= 0 included."""
    lib = L.lib()
    w, h = 16, 9
    cam = default_camera(w, h)
    bufs = [np.zeros((h, w, 4), np.float32) for _ in range(17)]
    ptr = lambda a: a.ctypes.data   # noqa: E731
    d = L.TemporalDesc()
    assert lib.lrt_temporal_default(w, h, ctypes.byref(cam), ctypes.byref(cam), ctypes.byref(d)) == 0
    f = L.Features()
    f.normal, f.world_pos, f.albedo = ptr(bufs[1]), ptr(bufs[2]), ptr(bufs[3])

    def state(first):
        s = L.TemporalState()
        for i, k in enumerate(L.TEMPORAL_STATE_NAMES):
            setattr(s, k, ptr(bufs[first + i]))
        return s

    prev, nxt, std, motion = state(4), state(9), ptr(bufs[14]), ptr(bufs[15])
    sph = (L.Sphere * 3)(L.Sphere(L.f3(0, 0, 0), 1.0), L.Sphere(L.f3(2, 0, 0), 0.5), L.Sphere(L.f3(0, 3, 0), 0.25))
    psph = (L.Sphere * 3)(*sph)

    def scene(**kw):
        sm = L.SceneMotion()
        sm.spheres, sm.prev_spheres, sm.count = sph, psph, 3
        for k, v in kw.items():
            setattr(sm, k, v)
        return sm

    def calls(dd, sm, c=ptr(bufs[0]), ff=f, p=prev, n=nxt, s=std, m=motion):
        ref = lambda x: ctypes.byref(x) if x is not None else None   # noqa: E731
        return (lib.lrt_temporal_accumulate_moving_host(ref(dd), ref(sm), c, ref(ff), ref(p), ref(n), s, m),
                lib.lrt_temporal_accumulate_moving_device(ref(dd), ref(sm), c, ref(ff), ref(p), ref(n), s, m, None))

    inv = (L.LRT_E_INVALID, L.LRT_E_INVALID)
    # what the static call rejects
    assert calls(None, scene()) == inv
    assert calls(d, scene(), c=None) == inv
    assert calls(d, scene(), ff=None) == inv
    assert calls(d, scene(), n=None) == inv
    bad = L.TemporalDesc.from_buffer_copy(d)
    bad.pos_tol = 0.0
    assert calls(bad, scene()) == inv
    bad = L.TemporalDesc.from_buffer_copy(d)
    bad.width = 0
    assert calls(bad, scene()) == inv
    assert calls(d, scene(), s=ptr(bufs[4])) == inv                       # color_std on a prev buffer
    # the scene
    assert calls(d, None) == inv
    null = ctypes.POINTER(L.Sphere)()
    assert calls(d, scene(spheres=null)) == inv
    assert calls(d, scene(prev_spheres=null)) == inv
    for count in (0, -1, L.MAX_SPHERES + 1):
        assert calls(d, scene(count=count)) == inv, count
    assert calls(d, scene(reserved=1)) == inv
    for arr in (sph, psph):
        for member in ("x", "y", "z", "radius"):
            for v in (float("nan"), float("inf"), -float("inf")):
                keep = arr[2].radius if member == "radius" else getattr(arr[2].center, member)
                if member == "radius":
                    arr[2].radius = v
                else:
                    setattr(arr[2].center, member, v)
                assert calls(d, scene()) == inv, (member, v)
                if member == "radius":
                    arr[2].radius = keep
                else:
                    setattr(arr[2].center, member, keep)
    # motion may overlap no other buffer
    for b in bufs[:15]:
        assert calls(d, scene(), m=ptr(b)) == inv
    assert calls(d, scene(), m=ptr(bufs[9]) + 16) == inv                  # a partial overlap
    assert "alias" in lib.lrt_last_error().decode()
    if os.environ.get("HIP_VISIBLE_DEVICES") == "" or not _gpu_present():
        st = (L.LRT_E_STATE, L.LRT_E_STATE)
        assert calls(d, scene()) == st
        assert calls(d, scene(), m=None) == st                            # motion is optional
        assert calls(d, scene(), p=None) == st
        assert calls(d, scene(count=1)) == st
        sph[1].radius, psph[2].radius = 0.0, -1.0                         # never matched, but no error
        assert calls(d, scene()) == st
        big = (L.Sphere * L.MAX_SPHERES)(*[L.Sphere(L.f3(i, 0, 0), 0.1) for i in range(L.MAX_SPHERES)])
        assert calls(d, scene(spheres=big, prev_spheres=big, count=L.MAX_SPHERES)) == st


def test_scene_motion_struct_and_front_end():
    assert ctypes.sizeof(L.SceneMotion) == 2 * ctypes.sizeof(ctypes.c_void_p) + 8 == 24
    assert L.SceneMotion.count.offset == 16 and L.SceneMotion.reserved.offset == 20
    cam = default_camera(16, 9)
    z = lambda: np.zeros((9, 16, 4), np.float32)   # noqa: E731
    color, cur = z(), {"normal": z(), "world_pos": z()}
    two = np.float32([[0, 0, 0, 1], [2, 0, 0, 1]])
    for spheres, prev_spheres in ((two, two[:1]), (two, None), (np.zeros((2, 3), np.float32), np.zeros((2, 3), np.float32)),
                                  ([], [])):
        with pytest.raises(LrtError):
            temporal_accumulate_moving_host(color, cur, None, cam, None, spheres, prev_spheres)
    with pytest.raises(LrtError):
        temporal_accumulate_moving_host(color, cur, None, cam, None, two, two, motion=np.zeros((9, 16, 3), np.float32))
    with pytest.raises(LrtError):
        temporal_accumulate_moving_host(color, cur, None, cam, None, two, two, alpha=0.5)
    with pytest.raises(LrtError) as e:       # the library's own check
        temporal_accumulate_moving_host(color, cur, None, cam, None, two, two, motion=color)
    assert e.value.code == L.LRT_E_INVALID
    with pytest.raises(LrtError) as e:
        temporal_accumulate_moving_host(color, cur, None, cam, None, np.float32([[0, 0, np.nan, 1]]),
                                        np.float32([[0, 0, 0, 1]]))
    assert e.value.code == L.LRT_E_INVALID
    structs = [L.Sphere(L.f3(0, 0, 0), 1.0), L.Sphere(L.f3(2, 0, 0), 1.0)]
    assert np.array_equal(M.sphere_array(structs), two)


# ---- nothing moves: the static restatement, exactly
@pytest.mark.parametrize("case", R.DESIGNED_CASES)
def test_unmatched_planes_equal_the_static_restatement(case):
    """temporal_ref's designed plane cases under a scene far from every plane: no pixel is matched,
    so the outputs are the static restatement's bit for bit in both dtypes, whether the spheres
    moved or not."""
    far = np.float32([[50, 60, 70, 1], [-40, 80, 10, 2], [0, 0, 90, 0.5]])
    came_from = far + np.float32([1, 2, 3, 0.5])
    for run in R.designed_runs(case):
        color, cur, prev, cam, pcam = R.designed_inputs(run, make_camera)
        for T in (np.float32, np.float64):
            want, wf = R.step(color, cur, prev, cam, pcam, T, **run["params"])
            for before in (far, came_from):
                info = {}
                got, gf = M.step(color, cur, prev, cam, pcam, far, before, T, info=info, **run["params"])
                assert not info["matched"].any() and (got["motion"][..., 2] == -1).all()
                for name in R.OUTPUTS:
                    assert np.array_equal(got[name], want[name]), (run["label"], name)
                assert np.array_equal(gf, wf)


@pytest.fixture(scope="module")
def orbit_pair():
    """67x45: two oracle frames of the default scene 0.08 rad apart on the orbit."""
    w, h = 67, 45
    (_, f0, cam0, _), (color, cur, cam1, k) = R.orbit_frames(_render, make_camera, w, h, 2, 0.08)
    return color, cur, R.random_prev(f0, 3), cam1, cam0, k


def test_unmoved_spheres_equal_the_static_restatement(orbit_pair):
    """The rendered default scene given as its own predecessor: nearly every hit pixel is matched
    (measured: all of them) and nothing changes."""
    color, cur, prev, cam1, cam0, k = orbit_pair
    sph = M.sphere_array(S0)
    for T in (np.float32, np.float64):
        want, wf = R.step(color, cur, prev, cam1, cam0, T, cur_scale=k)
        info = {}
        got, gf = M.step(color, cur, prev, cam1, cam0, sph, sph.copy(), T, info=info, cur_scale=k)
        hit = info["hit"]
        print(f"{T.__name__}: matched {_n(info['matched'])} of {_n(hit)} hit pixels")
        assert _n(hit) > 1000 and _n(info["matched"]) >= 0.98 * _n(hit) and not info["moved"].any()
        for name in R.OUTPUTS:
            assert np.array_equal(got[name], want[name]), name
        # the extra fragile pixels are match decisions only
        assert not (wf & ~gf).any()
        assert np.array_equal(got["motion"][..., 2] >= 0, info["matched"])
        assert np.array_equal(got["motion"][..., 3] == 1, info["ok"])


def test_matched_ids_are_the_oracles_first_hits(orbit_pair):
    """Which sphere a pixel shows is known independently: the one whose surface holds X."""
    color, cur, prev, cam1, cam0, k = orbit_pair
    sph = M.sphere_array(S0)
    info = {}
    M.step(color, cur, prev, cam1, cam0, sph, sph, np.float64, info=info, cur_scale=k)
    X = np.float64(cur["world_pos"][..., :3]) * k
    surf = np.abs(np.linalg.norm(X[..., None, :] - sph[:, :3], axis=-1) - sph[:, 3])
    own = surf.argmin(-1)
    m = info["matched"]
    assert (info["id"][m] == own[m]).all() and len(np.unique(own[m])) >= 7


# ---- the designed sphere cases
# {run label: [(branch, pixels of it in the f64 info, at least)]}
DESIGNED_BRANCHES = {
    "translate 37x21": [("matched and moved", lambda i: i["moved"], 50),
                        ("matched, not moved", lambda i: i["matched"] & ~i["moved"], 50),
                        ("miss", lambda i: ~i["hit"], 500),
                        ("moved, history kept", lambda i: i["moved"] & i["keep"], 50)],
    "translate 33x9": [("matched and moved", lambda i: i["moved"], 8), ("moved, history kept", lambda i: i["moved"] & i["keep"], 8),
                       ("column 32 written", lambda i: i["ok"][:, 32], 9)],
    "contact": [("two spheres in contact at the pixel", lambda i: i["touching"], 40),
                ("in contact and matched", lambda i: i["touching"] & i["matched"], 40),
                ("in contact, moved", lambda i: i["touching"] & i["moved"], 8),
                ("in contact, not moved", lambda i: i["touching"] & i["matched"] & ~i["moved"], 8)],
    "radius": [("matched and moved", lambda i: i["moved"], 120), ("moved, history kept", lambda i: i["moved"] & i["keep"], 100)],
    "carried_out": [("moved, projectable, no tap inside", lambda i: i["moved"] & i["ok"] & (i["taps_inside"] == 0), 60),
                    ("moved and reset", lambda i: i["moved"] & ~i["keep"], 60)],
    "carried_behind": [("moved, not projectable", lambda i: i["moved"] & ~i["ok"], 60),
                       ("moved and reset", lambda i: i["moved"] & ~i["keep"], 60)],
    "same_camera": [("moved under identical cameras, kept", lambda i: i["moved"] & i["keep"], 50),
                    ("not moved, kept", lambda i: i["matched"] & ~i["moved"] & i["keep"], 50)],
    "unmatched": [("unmatched hit", lambda i: i["hit"] & ~i["matched"], 150), ("matched", lambda i: i["matched"], 30)],
    "analytic": [("matched and moved", lambda i: i["moved"], 60), ("moved, history kept", lambda i: i["moved"] & i["keep"], 60)],
}


def test_designed_cases_cover_their_branches():
    worst, worst_std = 0.0, 0.0
    labels = []
    for case in M.DESIGNED_CASES:
        for run in M.designed_runs(case):
            labels.append(run["label"])
            args = M.designed_inputs(run, make_camera)
            info = {}
            out, fragile = M.step(*args, np.float64, info=info, **run["params"])
            plain, fragile2 = M.step(*args, np.float64, **run["params"])
            for name in M.MOTION_OUTPUTS:
                assert np.array_equal(out[name], plain[name]), name
            assert np.array_equal(fragile, fragile2)
            assert fragile.mean() <= MAX_FRAGILE, run["label"]
            for what, mask, least in DESIGNED_BRANCHES[run["label"]]:
                print(f"{run['label']}: {what}: {_n(mask(info))} (>= {least:g})")
                assert _n(mask(info)) >= least, (run["label"], what)
            assert not (info["matched"] & ~info["hit"]).any()             # a miss is never matched
            assert np.array_equal(out["motion"][..., 2], np.where(info["matched"], info["id"], -1))
            assert (out["motion"][..., :2][~info["ok"]] == 0).all()
            f32, ff = M.step(*args, np.float32, **run["params"])
            ok = ~(fragile | ff)
            assert np.array_equal(f32["motion"][..., 2][ok], out["motion"][..., 2][ok])
            for name in M.MOTION_OUTPUTS:
                g = R.rel_gap(f32[name], out[name], ok)
                if name == "color_std":
                    worst_std = max(worst_std, g)
                else:
                    worst = max(worst, g)
            if case == "unmatched":
                # spheres 0 (no radius in either scene), 1 (none before) and 2 (none now) are never matched;
                # the unmatched pixels behave as in the static step
                assert set(np.unique(info["id"])) == {-1, 3}
                static, _ = R.step(*args[:5], np.float64, **run["params"])
                un = ~info["matched"]
                for name in R.OUTPUTS:
                    assert np.array_equal(out[name][un], static[name][un]), name
            if case == "same_camera":
                # the static rule, blind to the move, keeps next to nothing of the moved sphere
                i2 = {}
                R.step(*args[:5], np.float64, info=i2, **run["params"])
                assert _n(i2["keep"] & info["moved"]) <= 0.1 * _n(info["moved"])
    assert sorted(labels) == sorted(DESIGNED_BRANCHES)
    print(f"f32 - f64 over the designed sphere cases: {worst:.3g} (color_std: {worst_std:.3g})")
    assert worst <= F32_F64_GAP_DESIGNED and worst_std <= F32_F64_GAP_STD_DESIGNED


@pytest.mark.parametrize("T", [np.float32, np.float64])
def test_analytic_displacement_and_kept_history(T):
    """A sphere translated along x under one pinhole camera, no jitter: every one of its pixels keeps
    its history (the previous state shows the same sphere where it was), and motion is the known
    displacement -ANALYTIC_DX h / (2 tan(vfov / 2) depth) along x and 0 along y, within the house
    tolerance of the designed cases."""
    run = M.designed_runs("analytic")[0]
    args = M.designed_inputs(run, make_camera)
    info = {}
    out, fragile = M.step(*args, T, info=info, **run["params"])
    mv = info["moved"]
    assert _n(mv) >= 60 and not fragile.any()
    assert info["keep"][mv].all() and (out["n"][mv] > 1).all()
    depth = 3.0 - np.float64(args[1]["world_pos"][..., 2])
    want = M.analytic_displacement(run["h"], depth)
    tol = 16 * F32_F64_GAP_DESIGNED
    assert R.rel_gap(out["motion"][..., 0][mv], want[mv]) <= tol
    assert np.abs(out["motion"][..., 1][mv]).max() <= tol
    assert np.abs(want[mv]).min() > 1.0                                   # more than a pixel
    assert (out["motion"][..., 2][mv] == 1).all() and (out["motion"][..., 3][mv] == 1).all()
    # the sphere that stands still and the sky take their own pixel
    still = ~mv
    assert np.abs(out["motion"][..., :2][still]).max() <= tol


def test_count_cases():
    """Every pixel a random sphere out of `count`: the match finds it at every count; the history is
    reset (a pixel's neighbours show other spheres), so it is motion.xy that checks the previous entry."""
    worst = 0.0
    for count in M.COUNTS:
        *args, pick = M.count_inputs(count, make_camera)
        info = {}
        out, fragile = M.step(*args, np.float64, info=info, pos_tol=M.COUNT_POS_TOL)
        assert fragile.mean() <= MAX_FRAGILE
        assert info["matched"].all() and np.array_equal(info["id"], pick)
        assert len(np.unique(pick)) == min(count, len(np.unique(pick))) and info["ok"].mean() > 0.9
        if count >= 9:
            assert _n(info["moved"]) > 100 and _n(~info["moved"]) > 20
        f32, ff = M.step(*args, np.float32, pos_tol=M.COUNT_POS_TOL)
        ok = ~(fragile | ff)
        assert np.array_equal(f32["motion"][..., 2][ok], out["motion"][..., 2][ok])
        worst = max([worst] + [R.rel_gap(f32[name], out[name], ok) for name in M.MOTION_OUTPUTS if name in out])
    print(f"f32 - f64 over the count cases: {worst:.3g}")
    assert worst <= F32_F64_GAP_COUNT


def test_rendered_cases_gap_and_fragile_share():
    """The GPU test's rendered cases through the oracle: the restatement's own f32 run is within the
    recorded gap of its f64 run, few pixels are fragile (none at the two smallest sizes), and the
    moved spheres are there."""
    gap, gap_std, shares = M.f32_f64_gap(_render, make_camera, S0)
    print(f"f32 - f64 over the rendered cases: {gap:.3g} (color_std: {gap_std:.3g})")
    assert gap <= F32_F64_GAP and gap_std <= F32_F64_GAP_STD
    for (w, h, dt), s in shares.items():
        assert s <= MAX_FRAGILE and (w * h > 15 or s == 0), (w, h, dt)
    args = M.rendered_case(_render, make_camera, S0, 67, 45, 0.02)
    info = {}
    M.step(*args, np.float64, info=info, cur_scale=M.CUR_SCALE)
    ids = info["id"][info["moved"]]
    for i in (M.LAMBERT_ID, M.METAL_ID, M.RESIZED_ID):
        assert _n(ids == i) >= 20, i
    assert _n(info["moved"] & info["keep"]) >= 0.8 * _n(info["moved"])


# ---- what it is for
def test_quality_moving_sphere():
    """160x90, depth 8, 16 steps of 1 spp under a static camera while Lambert sphere MOVING_ID comes
    down MOVING_STEP per step, against 1024 spp of the final scene, in f64. The static rule resets
    that sphere's pixels at every step (asserted); the moving rule keeps their history. Measured:
    see QUALITY_RATIO in tests/temporal_motion_ref.py."""
    q = M.QUALITY
    frames = M.moving_frames(_render, make_camera, S0)
    cam = frames[-1][2]
    # the step is above pos_tol x the sphere's distance from the camera
    dist = np.linalg.norm(np.float64(R.cam22(cam)[:3]) - M.sphere_array(S0)[M.MOVING_ID, :3])
    assert np.linalg.norm(M.MOVING_STEP) > R.DEFAULTS["pos_tol"] * dist
    # the static restatement, step by step: the moved sphere's pixels are reset every time
    state_s, state_m, prev_sph, on = None, None, frames[0][4], None
    for t, (color, feats, cam, k, sph) in enumerate(frames):
        info = {}
        out_s, _ = R.step(color, feats, state_s, cam, cam, np.float64, cur_scale=k)
        out_m, _ = M.step(color, feats, state_m, cam, cam, sph, prev_sph, np.float64, info=info, cur_scale=k)
        if t:
            on = info["matched"] & (info["id"] == M.MOVING_ID)
            assert (out_s["n"][on] == 1).all(), t
        state_s, state_m, prev_sph = R.as_state(out_s, np.float64), R.as_state(out_m, np.float64), sph
    gt, _ = oracle.orc_render(q["w"], q["h"], frames=q["gt_spp"], depth=q["depth"], cam22=R.cam22(cam))
    color, _, _, k, _ = frames[-1]
    single = np.float64(color[..., :3]) * k
    assert _n(on) >= 150
    r1, rs, rm = M.rel_mse(single, gt, on), M.rel_mse(out_s["color"], gt, on), M.rel_mse(out_m["color"], gt, on)
    ws, wm = M.rel_mse(out_s["color"], gt), M.rel_mse(out_m["color"], gt)
    print(f"sphere {M.MOVING_ID} ({_n(on)} px): relMSE single {r1:.4g}, static {rs:.4g}, moving {rm:.4g} "
          f"({rm / r1:.4f}x of the single frame); whole frame: static {ws:.4g}, moving {wm:.4g}; "
          f"mean n on the sphere: {out_m['n'][on].mean():.2f}")
    assert rm < rs
    assert wm <= ws
    assert rm / r1 <= M.QUALITY_RATIO * 1.02          # the recorded ratio is this measurement
    assert M.QUALITY_BAR == pytest.approx(1.25 * M.QUALITY_RATIO)
    assert rm <= M.QUALITY_BAR * r1


def test_temporal_bench_moving_leg_leaves_the_line_alone():
    import importlib.util
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("temporal_bench", os.path.join(root, "tools", "temporal_bench.py"))
    B = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(B)
    assert B.step_bytes() == 216 and B.step_bytes(albedo=False, color_std=False) == 172
    assert B.MOVING_FIELDS == ("moving_step_ms", "moving_step_motion_ms", "moving_step_1000_ms")
    with pytest.raises(SystemExit):
        B.main(["--moving", "--reps", "5"])
