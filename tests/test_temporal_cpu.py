"""Temporal accumulation's host-side contract (no GPU): argument validation and defaults of the
C-ABI (lrt_temporal_*), the Python front end's argument checks, and the specified algorithm itself
-- its NumPy restatement (tests/temporal_ref.py) in f64 on the oracle's 1 spp frames: properties
(static camera = plain accumulation, no history, misses, alphas) and what it is for (an orbit's
accumulated frame against the oracle's 1024 spp frame at the final camera)."""
import ctypes
import os

import numpy as np
import pytest

import denoise_ref as DR
import oracle
import temporal_ref as R
from learnraytracing_amd import LrtError, _lib as L
from learnraytracing_amd import default_camera, make_camera, temporal_accumulate_host, temporal_desc

W, H = 160, 90
CUR = ("normal", "world_pos", "albedo")


def _gpu_present():
    import torch
    return torch.cuda.device_count() > 0


def _render(w, h, camera, frame0, depth=8):
    """One fresh 1 spp frame and its features through the oracle: sample frame0 into zeroed buffers."""
    feats = {n: np.zeros((h, w, 4), np.float32) for n in CUR}
    buf, _ = oracle.orc_render_ex(w, h, frames=1, depth=depth, frame0=frame0, cam22=R.cam22(camera),
                                  features=feats, max_frame=-1)
    return buf, feats


# ---- the C-ABI
def test_temporal_validation_before_device_use():
    """Every invalid argument is LRT_E_INVALID, a valid call without lrt_initialize() LRT_E_STATE:
    no GPU needed for either, host and device entry points alike."""
    lib = L.lib()
    w, h = 16, 9
    cam = default_camera(w, h)
    bufs = [np.zeros((h, w, 4), np.float32) for _ in range(16)]
    color, nrm, pos, alb = bufs[0:4]
    ptr = lambda a: a.ctypes.data   # noqa: E731

    def desc(**kw):
        d = L.TemporalDesc()
        assert lib.lrt_temporal_default(w, h, ctypes.byref(cam), ctypes.byref(cam), ctypes.byref(d)) == 0
        for k, v in kw.items():
            setattr(d, k, v)
        return d

    def features(**kw):
        f = L.Features()
        for k, v in dict(dict(normal=ptr(nrm), world_pos=ptr(pos), albedo=ptr(alb)), **kw).items():
            setattr(f, k, v)
        return f

    def state(first, **kw):
        s = L.TemporalState()
        for i, k in enumerate(L.TEMPORAL_STATE_NAMES):
            setattr(s, k, ptr(bufs[first + i]))
        for k, v in kw.items():
            setattr(s, k, v)
        return s

    std = bufs[14]

    def calls(d, c, f, p, n, s):
        ref = lambda x: ctypes.byref(x) if x is not None else None   # noqa: E731
        return (lib.lrt_temporal_accumulate_host(ref(d), c, ref(f), ref(p), ref(n), s),
                lib.lrt_temporal_accumulate_device(ref(d), c, ref(f), ref(p), ref(n), s, None))

    inv = (L.LRT_E_INVALID, L.LRT_E_INVALID)
    good = (desc(), ptr(color), features(), state(4), state(9), ptr(std))
    # NULL required pointers
    assert calls(None, *good[1:]) == inv
    assert calls(good[0], None, *good[2:]) == inv
    assert calls(good[0], good[1], None, *good[3:]) == inv
    assert calls(*good[:4], None, good[5]) == inv
    for name in ("normal", "world_pos"):
        assert calls(good[0], good[1], features(**{name: None}), *good[3:]) == inv, name
    for name in L.TEMPORAL_STATE_NAMES[:4]:
        assert calls(*good[:3], state(4, **{name: None}), *good[4:]) == inv, ("prev", name)
        assert calls(*good[:4], state(9, **{name: None}), good[5]) == inv, ("next", name)
    # the descriptor
    for bad in (dict(width=0), dict(height=0), dict(width=-3), dict(width=46341, height=46341), dict(flags=1),
                dict(reserved=1), dict(min_history=0), dict(min_history=-2)):
        assert calls(desc(**bad), *good[1:]) == inv, bad
    for name in ("cur_scale", "alpha_min", "normal_min", "pos_tol", "short_std"):
        for v in (float("inf"), float("nan"), -float("inf")):
            assert calls(desc(**{name: v}), *good[1:]) == inv, (name, v)
    for name in ("cur_scale", "pos_tol", "short_std", "alpha_min"):
        for v in (0.0, -1.0):
            assert calls(desc(**{name: v}), *good[1:]) == inv, (name, v)
    assert calls(desc(alpha_min=1.0001), *good[1:]) == inv
    for v in (-1.0001, 1.0001):
        assert calls(desc(normal_min=v), *good[1:]) == inv, v
    # a previous camera that cannot be projected into
    for member, value in (("horizontalVec", L.f3(0, 0, 0)), ("verticalVec", L.f3(0, 0, 0)),
                          ("horizontalVec", L.f3(float("nan"), 0, 0)), ("verticalVec", L.f3(float("inf"), 0, 0)),
                          ("lowerLeftCorner", cam.origin), ("a", L.f3(-cam.a.x, -cam.a.y, -cam.a.z))):
        d = desc()
        setattr(d.prev_camera, member, value)
        assert calls(d, *good[1:]) == inv, member
    # aliasing: no output may be an input, a prev buffer or another output
    ins = [ptr(color), ptr(nrm), ptr(pos), ptr(alb)] + [ptr(b) for b in bufs[4:9]]
    for name in L.TEMPORAL_STATE_NAMES:
        for p in ins + [ptr(std)]:
            assert calls(*good[:4], state(9, **{name: p}), good[5]) == inv, name
    for p in ins:
        assert calls(*good[:5], p) == inv
    assert calls(*good[:4], state(9, color=ptr(bufs[10])), good[5]) == inv            # two outputs, one buffer
    assert calls(*good[:4], state(9, color=ptr(bufs[10]) + 16), good[5]) == inv       # a partial overlap
    assert "alias" in lib.lrt_last_error().decode()
    if os.environ.get("HIP_VISIBLE_DEVICES") == "" or not _gpu_present():
        st = (L.LRT_E_STATE, L.LRT_E_STATE)
        assert calls(*good) == st
        assert calls(*good[:3], None, *good[4:]) == st                                  # no history
        assert calls(*good[:5], None) == st                                             # no color_std
        assert calls(good[0], good[1], features(albedo=None), good[3], state(9, albedo=None), good[5]) == st
        assert calls(desc(alpha_min=1.0, normal_min=-1.0), *good[1:]) == st             # the closed ends


def test_temporal_default_desc_and_struct_sizes():
    lib = L.lib()
    assert ctypes.sizeof(L.TemporalDesc) == 16 + 2 * 88 + 24 == 216
    assert ctypes.sizeof(L.TemporalState) == 5 * ctypes.sizeof(ctypes.c_void_p) == 40
    assert L.TemporalDesc.camera.offset == 16 and L.TemporalDesc.cur_scale.offset == 192
    cam, prev = default_camera(1280, 720), make_camera(*R.orbit_args(0.3, 1280, 720))
    d = L.TemporalDesc()
    assert lib.lrt_temporal_default(1280, 720, ctypes.byref(cam), ctypes.byref(prev), ctypes.byref(d)) == 0
    assert (d.width, d.height, d.flags, d.min_history, d.reserved) == (1280, 720, 0, 4, 0)
    assert d.camera.to22() == cam.to22() and d.prev_camera.to22() == prev.to22()
    for name, v in R.DEFAULTS.items():
        assert getattr(d, name) == (v if name == "min_history" else np.float32(v)), name
    assert R.DEFAULTS == dict(cur_scale=1.0, alpha_min=0.05, normal_min=0.9, pos_tol=0.05, short_std=1e3,
                              min_history=4)
    assert lib.lrt_temporal_default(1280, 720, ctypes.byref(cam), None, ctypes.byref(d)) == 0
    assert d.prev_camera.to22() == cam.to22()
    assert lib.lrt_temporal_default(1280, 720, ctypes.byref(cam), None, None) == L.LRT_E_INVALID
    assert lib.lrt_temporal_default(1280, 720, None, None, ctypes.byref(d)) == L.LRT_E_INVALID
    assert lib.lrt_temporal_default(0, 720, ctypes.byref(cam), None, ctypes.byref(d)) == L.LRT_E_INVALID
    assert L.lib().lrt_version().decode() == "lrt-mi355x 0.4.0 gfx950"
    import learnraytracing_amd
    assert learnraytracing_amd.__version__ == "0.4.0"


def test_python_front_end_rejects_bad_arguments():
    cam = default_camera(16, 9)
    z = lambda: np.zeros((9, 16, 4), np.float32)   # noqa: E731
    color, cur = z(), {"normal": z(), "world_pos": z()}
    assert temporal_desc(16, 9, cam, min_history=2, pos_tol=0.1).min_history == 2
    with pytest.raises(LrtError):
        temporal_desc(16, 9, cam, sigma=1.0)
    with pytest.raises(LrtError):
        temporal_desc(16, 9, cam.to22())
    with pytest.raises(LrtError):
        temporal_accumulate_host(color, cur, None, cam, alpha=0.5)
    with pytest.raises(LrtError):
        temporal_accumulate_host(color, dict(cur, depth=z()), None, cam)
    with pytest.raises(LrtError):
        temporal_accumulate_host(color, {"normal": z()}, None, cam)
    with pytest.raises(LrtError):
        temporal_accumulate_host(color.ravel(), cur, None, cam)
    with pytest.raises(LrtError):
        temporal_accumulate_host(color, dict(cur, normal=np.zeros((9, 16, 3), np.float32)), None, cam)
    with pytest.raises(LrtError):
        temporal_accumulate_host(color, cur, {"color": z(), "moment2": z(), "normal": z()}, cam)
    with pytest.raises(LrtError):
        temporal_accumulate_host(color, cur, {"color": z(), "moment2": z(), "normal": z(), "world_pos": z(),
                                              "depth": z()}, cam)
    with pytest.raises(LrtError):
        temporal_accumulate_host(color, cur, None, cam, out={"color": z(), "moment2": z(), "normal": z()})
    with pytest.raises(LrtError):
        temporal_accumulate_host(color, cur, None, cam, out={"color": z().astype(np.float64), "moment2": z(),
                                                             "normal": z(), "world_pos": z()})
    with pytest.raises(LrtError) as e:   # the library's own check: an output that is an input
        temporal_accumulate_host(color, cur, None, cam, out={"color": color, "moment2": z(), "normal": z(),
                                                             "world_pos": z()})
    assert e.value.code == L.LRT_E_INVALID


# ---- the restatement, in f64
def test_restatement_tap_weights_and_alpha_rule():
    """An all-miss frame under a turned camera: every tap is consistent, so the weights of a pixel
    whose four taps are inside sum to 1, a border pixel's are renormalised, and a pixel that lands
    outside is reset; n = n' + 1 and alpha = max(1 / n, alpha_min) exactly as specified."""
    w, h = 24, 14
    z = lambda: np.zeros((h, w, 4), np.float32)   # noqa: E731
    rng = np.random.default_rng(5)
    color = z()
    color[..., :3] = rng.uniform(0.1, 2.0, (h, w, 3))
    cur = {"normal": z(), "world_pos": z()}
    cam1 = make_camera(*R.orbit_args(0.0, w, h))
    args0 = list(R.orbit_args(0.0, w, h))
    args0[1] = (0.35, 0.2, 0.0)               # the previous camera looked a little to the side and up
    cam0 = make_camera(*args0)
    for n_prev, alpha in ((1.0, 0.5), (2.0, 1 / 3), (15.0, 1 / 16), (40.0, 0.05)):
        prev = {"color": z(), "moment2": z(), "normal": z(), "world_pos": z()}
        prev["color"][..., :3] = 3.0
        prev["moment2"][..., :3] = 11.0
        prev["moment2"][..., 3] = n_prev
        out, _ = R.step(color, cur, prev, cam1, cam0, np.float64)
        kept = out["n"] > 1.5
        assert 0.5 < kept.mean() < 1.0
        C = np.float64(color[..., :3])
        assert np.abs(out["n"][kept] - (n_prev + 1)).max() <= 1e-12
        assert np.abs(out["color"][kept] - ((1 - alpha) * 3.0 + alpha * C[kept])).max() <= 1e-12
        assert np.abs(out["moment2"][kept] - ((1 - alpha) * 11.0 + alpha * C[kept] ** 2)).max() <= 1e-12
        assert np.array_equal(out["color"][~kept], C[~kept]) and (out["n"][~kept] == 1).all()
        assert (out["color_std"][~kept] == 1e3).all()
        want_short = n_prev + 1 < 4
        assert (out["color_std"][kept] == 1e3).all() == want_short


@pytest.fixture(scope="module")
def static_frames():
    """16 fresh 1 spp frames of one camera (the orbit's last)."""
    cam = make_camera(*R.orbit_args(0.0, W, H))
    return [(*_render(W, H, cam, t), cam, float(t + 1)) for t in range(16)]


def test_static_camera_is_plain_accumulation(static_frames):
    """Under a static camera, with alpha = 1 / n all the way (alpha_min 1/64), a pixel that kept its
    history at every step holds the mean of its 16 fresh samples: the oracle's 16 spp frame
    (measured: 89.8 % of the pixels, gap 1.1e-6)."""
    out = R.accumulate(static_frames, np.float64, alpha_min=1 / 64)
    want, _ = oracle.orc_render(W, H, frames=16, depth=8, cam22=R.cam22(static_frames[0][2]))
    full = np.abs(out["n"] - 16) < 1e-3   # (the f32 camera's axes are orthogonal to ~1e-8 only: n is 16 - 1e-6 at some)
    gap = R.rel_gap(out["color"], want[..., :3], full)
    print(f"static camera: {100 * full.mean():.1f} % of the pixels kept their history, gap {gap:.3g}")
    assert full.mean() >= 0.85
    assert gap <= 1e-5
    assert (out["color_std"][full] < 1e3).all()


def test_no_history(static_frames):
    color, cur, cam, _ = static_frames[3]
    C = np.float64(color[..., :3]) * 4
    away = list(R.orbit_args(0.0, W, H))
    away[1] = tuple(2 * np.array(away[0]))     # from the same place, looking the other way
    behind = make_camera(*away)
    prev = R.random_prev(cur, 7)
    for p, pc in ((None, cam), (prev, behind)):
        out, _ = R.step(color, cur, p, cam, pc, np.float64, cur_scale=4.0)
        assert np.array_equal(out["color"], C) and np.array_equal(out["moment2"], C * C)
        assert (out["n"] == 1).all() and (out["color_std"] == 1e3).all()
        assert np.array_equal(out["normal"], np.float64(cur["normal"][..., :3]) * 4)
        assert np.array_equal(out["albedo"], np.float64(cur["albedo"][..., :3]) * 4)
    out, _ = R.step(color, cur, None, cam, cam, np.float64, min_history=1, cur_scale=4.0)
    assert (out["color_std"] == 0).all()       # n = 1 is enough history then: the variance of one sample


def test_miss_pixels_reproject_only_onto_misses():
    frames = R.orbit_frames(_render, make_camera, W, H, 2, 0.08)
    (_, f0, cam0, _), (color, cur, cam1, k) = frames
    prev = R.random_prev(f0, 3)
    hit_prev = (prev["normal"][..., :3] ** 2).sum(-1) >= 0.25
    prev["color"][..., :3] = np.where(hit_prev[..., None], 7.0, 1.0)
    prev["moment2"][..., 3] = 3.0
    out, _ = R.step(color, cur, prev, cam1, cam0, np.float64, cur_scale=k)
    miss = (out["normal"] ** 2).sum(-1) < 0.25
    kept = out["n"] > 1.5
    assert (miss & kept).sum() > 100 and (~miss & kept).sum() > 1000 and 0.02 < hit_prev.mean() < 0.98
    C = np.float64(color[..., :3]) * k
    assert np.abs(out["color"][miss & kept] - (0.75 * 1.0 + 0.25 * C[miss & kept])).max() <= 1e-12
    assert np.abs(out["color"][~miss & kept] - (0.75 * 7.0 + 0.25 * C[~miss & kept])).max() <= 1e-12


def test_alpha_channels():
    """The history length travels in moment2's alpha and nowhere else: the other alphas are ignored."""
    frames = R.orbit_frames(_render, make_camera, 67, 45, 2, 0.02)
    (_, f0, cam0, _), (color, cur, cam1, k) = frames
    prev = R.random_prev(f0, 11)
    out, _ = R.step(color, cur, prev, cam1, cam0, np.float64, cur_scale=k)
    junk = lambda a: np.concatenate([a[..., :3], np.full_like(a[..., :1], 123.0)], -1)   # noqa: E731
    prev2 = {n: (v if n == "moment2" else junk(v)) for n, v in prev.items()}
    out2, _ = R.step(junk(color), {n: junk(v) for n, v in cur.items()}, prev2, cam1, cam0, np.float64, cur_scale=k)
    for name in R.OUTPUTS:
        assert np.array_equal(out[name], out2[name]), name
    prev3 = dict(prev, moment2=prev["moment2"].copy())
    prev3["moment2"][..., 3] = 100.0
    out3, _ = R.step(color, cur, prev3, cam1, cam0, np.float64, cur_scale=k)
    kept = out["n"] > 1.5
    assert kept.mean() > 0.8 and np.abs(out3["n"][kept] - 101).max() < 1e-9
    st = R.as_state(out)
    assert np.array_equal(st["moment2"][..., 3], np.float32(out["n"])) and (st["color"][..., 3] == 0).all()


# ---- the designed scenes
MAX_FRAGILE = 0.02            # tests/test_gpu_temporal.py's
F32_F64_GAP_DESIGNED, F32_F64_GAP_STD_DESIGNED = 2.5e-5, 4.8e-5   # tests/test_gpu_temporal.py's


def _n(mask):
    return int(np.count_nonzero(mask))


# what each case is there for: {run label: [(branch, pixels of it in the f64 info, at least)]}
DESIGNED_BRANCHES = {
    "shift 37x21": [("kept", lambda i: i["keep"], 0.98 * 37 * 21), ("four taps inside", lambda i: i["taps_inside"] == 4, 8)],
    "shift 33x9": [("kept", lambda i: i["keep"], 0.95 * 33 * 9), ("kept with four taps inside", lambda i: i["keep"] & (i["taps_inside"] == 4), 8)],
    "same 37x21": [("kept", lambda i: i["keep"], 37 * 21)],
    "same 33x9": [("kept", lambda i: i["keep"], 33 * 9), ("column 32 kept", lambda i: i["keep"][:, 32], 9)],
    "behind": [("not projectable", lambda i: ~i["ok"], 37 * 21), ("reset", lambda i: ~i["keep"], 37 * 21)],
    "sideways": [("projectable, no tap inside", lambda i: i["ok"] & (i["taps_inside"] == 0), 37 * 21),
                 ("reset", lambda i: ~i["keep"], 37 * 21)],
    "half_off side": [("kept", lambda i: i["keep"], 0.7 * 37 * 21), ("reset", lambda i: ~i["keep"], 0.2 * 37 * 21),
                      ("two taps inside", lambda i: i["taps_inside"] == 2, 8),
                      ("no tap inside", lambda i: i["taps_inside"] == 0, 8)],
    "half_off corner": [("one tap inside", lambda i: i["taps_inside"] == 1, 8),
                        ("one tap inside, kept", lambda i: (i["taps_inside"] == 1) & i["keep"], 8),
                        ("two taps inside", lambda i: i["taps_inside"] == 2, 8)],
    "horizon same camera": [("miss", lambda i: ~i["hit"], 8), ("grazing", lambda i: i["grazing"], 8),
                            ("hit, not centred (the same-camera shortcut declined)", lambda i: i["hit"] & ~i["centred"], 8),
                            ("miss kept (onto misses)", lambda i: ~i["hit"] & i["keep"], 8),
                            ("miss onto hit rejected", lambda i: ~i["hit"] & (i["rej_hitmiss"] > 0), 8)],
    "horizon shift": [("miss", lambda i: ~i["hit"], 8), ("lambda <= 0", lambda i: i["lam_le0"], 8),
                      ("miss kept (onto misses)", lambda i: ~i["hit"] & i["keep"], 8),
                      ("hit onto miss rejected", lambda i: i["hit"] & (i["rej_hitmiss"] > 0), 8)],
    "corner": [("rejected by normal alone", lambda i: i["rej_normal"] > 0, 4),
               ("rejected by position alone", lambda i: i["rej_pos"] > 0, 4),
               ("rejected by hit / miss", lambda i: i["rej_hitmiss"] > 0, 4),
               ("taps inside, all rejected", lambda i: (i["taps_inside"] > 0) & ~i["keep"], 8)],
    "moments": [("variance clamped", lambda i: i["var_clamped"], 8), ("variance not clamped", lambda i: i["keep"] & ~i["var_clamped"], 8),
                ("alpha clamped", lambda i: i["alpha_clamped"], 8), ("alpha not clamped", lambda i: i["keep"] & ~i["alpha_clamped"], 8),
                ("short history", lambda i: i["short_history"], 8), ("long history", lambda i: ~i["short_history"], 8)],
}


def test_designed_cases_cover_their_branches():
    """The designed scenes reach what they are designed for, in the f64 restatement alone: every
    listed branch holds its pixels, few pixels are fragile, the restatement's own f32 run is within
    the recorded gap, and over all cases every mask of `info` is populated on both sides."""
    seen = {name: [0, 0] for name in R.INFO_MASKS + R.INFO_COUNTS}
    labels = []
    taps = set()
    worst, worst_std = 0.0, 0.0
    for case in R.DESIGNED_CASES:
        for run in R.designed_runs(case):
            labels.append(run["label"])
            color, cur, prev, cam, pcam = R.designed_inputs(run, make_camera)
            assert (pcam is cam) == (run["prev_cam"] is None)
            info = {}
            out, fragile = R.step(color, cur, prev, cam, pcam, np.float64, info=info, **run["params"])
            plain, fragile2 = R.step(color, cur, prev, cam, pcam, np.float64, **run["params"])
            for name in R.OUTPUTS:                       # info= changes nothing
                assert np.array_equal(out[name], plain[name]), name
            assert np.array_equal(fragile, fragile2)
            assert set(info) == set(R.INFO_MASKS + R.INFO_COUNTS)
            assert fragile.mean() <= MAX_FRAGILE, run["label"]
            for what, mask, least in DESIGNED_BRANCHES[run["label"]]:
                print(f"{run['label']}: {what}: {_n(mask(info))} (>= {least:g})")
                assert _n(mask(info)) >= least, (run["label"], what)
            for name in seen:
                seen[name][0] += _n(info[name])
                seen[name][1] += _n(info[name] == 0)
            taps |= set(np.unique(info["taps_inside"]).tolist())
            # the masks say what the outputs say
            assert np.array_equal(info["keep"], out["n"] > 1)
            assert (out["n"][~info["keep"]] == 1).all()
            assert np.array_equal(info["short_history"], (out["color_std"] == 1e3).all(-1))
            assert (out["color_std"][info["var_clamped"] & ~info["short_history"]] == 0).any(-1).all()
            f32, ff = R.step(color, cur, prev, cam, pcam, np.float32, **run["params"])
            for name in R.OUTPUTS:
                g = R.rel_gap(f32[name], out[name], ~(fragile | ff))
                if name == "color_std":
                    worst_std = max(worst_std, g)
                else:
                    worst = max(worst, g)
    assert sorted(labels) == sorted(DESIGNED_BRANCHES)
    for name, (on, off) in seen.items():
        assert on > 0 and off > 0, name
    assert taps == {0, 1, 2, 4}                           # (three cannot be: the previous image is a rectangle)
    print(f"f32 - f64 over the designed cases: {worst:.3g} (color_std: {worst_std:.3g})")
    assert worst <= F32_F64_GAP_DESIGNED and worst_std <= F32_F64_GAP_STD_DESIGNED


def test_plane_frame_and_make_prev():
    w, h = R.DESIGNED_SIZE
    run = R.designed_runs("corner")[0]
    color, cur, prev, cam, pcam = R.designed_inputs(run, make_camera)
    c2, f2, hit = R.plane_frame(w, h, cam, run["planes"], [0, w, h, 0])
    assert np.array_equal(c2, color) and all(np.array_equal(f2[k], cur[k]) for k in cur)
    assert 0.2 < hit.mean() < 0.9 and color.dtype == np.float32 and (color[..., :3] >= 0.05).all()
    n2 = (cur["normal"][..., :3] ** 2).sum(-1)
    assert np.allclose(n2[hit], 1, atol=1e-6) and (n2[~hit] == 0).all() and (cur["world_pos"][~hit] == 0).all()
    pos, O = np.float64(cur["world_pos"][..., :3]), np.float64(R.cam22(cam)[:3])
    on_plane = [np.abs((pos - np.float64(pl["p"])) @ np.float64(pl["n"])) < 1e-5 for pl in run["planes"]]
    assert np.logical_or.reduce(on_plane)[hit].all() and all(8 <= _n(m & hit) for m in on_plane)
    assert (((O - pos) * cur["normal"][..., :3]).sum(-1)[hit] > 0).all()         # turned towards the camera
    # the hit point lies within JITTER px of the pixel centre as the camera sees it
    c = np.float64(R.cam22(cam))
    L, H, V = c[12:15], c[15:18], c[18:21]
    d = pos - O
    q = d * ((L - O) @ c[3:6] / (d @ c[3:6]))[..., None] - (L - O)
    ys, xs = np.mgrid[0:h, 0:w]
    fx, fy = q @ H / (H @ H) * w - 0.5 - xs, q @ V / (V @ V) * h - 0.5 - ys
    assert np.abs(fx[hit]).max() <= R.JITTER + 1e-4 and np.abs(fy[hit]).max() <= R.JITTER + 1e-4
    assert np.abs(fx[hit]).max() > 0.2
    # make_prev: random_prev but for n and, on a tenth of the pixels, the moment
    base = R.random_prev(cur, 5)
    st = R.make_prev(cur, 5, n_range=(1.0, 40.0), under_moment=True)
    assert all(np.array_equal(st[k], base[k]) for k in ("color", "normal", "world_pos"))
    n = st["moment2"][..., 3]
    assert n.min() >= 1 and n.max() <= 40 and n.max() > 30
    under = (st["moment2"][..., :3] < st["color"][..., :3] ** 2).all(-1)
    assert 0.05 < under.mean() < 0.15
    assert np.array_equal(st["moment2"][..., :3][~under], base["moment2"][..., :3][~under])
    assert np.array_equal(st["moment2"][..., :3][under], np.float32(0.5) * st["color"][..., :3][under] ** 2)
    assert np.array_equal(R.make_prev(cur, 5)["moment2"][..., :3], base["moment2"][..., :3])


# ---- what it is for
@pytest.fixture(scope="module")
def ground_truth():
    q = R.QUALITY
    cam = make_camera(*R.orbit_args(0.0, q["w"], q["h"]))
    gt, _ = oracle.orc_render(q["w"], q["h"], frames=q["gt_spp"], depth=q["depth"], cam22=R.cam22(cam))
    return gt


@pytest.mark.parametrize("dtheta", [0.02, 0.0, 0.08])
def test_quality_of_accumulated_orbit(ground_truth, dtheta):
    """160x90, depth 8, 16 steps of 1 spp along the orbit, against 1024 spp at the final camera
    (measured, f64: relMSE 0.04x / 0.10x / 0.10x of the last single frame's for steps of 0.02 / 0 /
    0.08 rad, MSE 0.32-0.35x, accumulated then filtered 0.26-0.40x of the filtered single frame)."""
    q = R.QUALITY
    frames = R.orbit_frames(_render, make_camera, q["w"], q["h"], q["steps"], dtheta)
    out = R.accumulate(frames, np.float64)
    color, feats, _, k = frames[-1]
    single = np.float64(color[..., :3]) * k
    guides1 = {n: np.float64(feats[n][..., :3]) * k for n in CUR}
    r0, r1 = DR.rel_mse(single, ground_truth), DR.rel_mse(out["color"], ground_truth)
    m0, m1 = DR.mse(single, ground_truth), DR.mse(out["color"], ground_truth)
    cand = DR.atrous(out["color"], {n: out[n] for n in L.GUIDE_NAMES}, np.float64)
    base = DR.atrous(single, dict(guides1, color_std=np.full_like(single, R.DEFAULTS["short_std"])), np.float64)
    d0, d1 = DR.rel_mse(base, ground_truth), DR.rel_mse(cand, ground_truth)
    print(f"step {dtheta}: relMSE {r0:.4g} -> {r1:.4g} ({r1 / r0:.3f}x), MSE {m0:.4g} -> {m1:.4g} "
          f"({m1 / m0:.3f}x), filtered relMSE {d0:.4g} -> {d1:.4g} ({d1 / d0:.3f}x)")
    assert r1 <= R.BAR_REL * r0
    assert m1 <= R.BAR_MSE * m0
    assert d1 <= R.BAR_DENOISED * d0


def test_temporal_bench_byte_count():
    """tools/temporal_bench.py's compulsory bytes per pixel: 3-4 current and 4 history quads read,
    colour and color_std written as 12 B, the other outputs as 16 B."""
    import importlib.util
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("temporal_bench", os.path.join(root, "tools", "temporal_bench.py"))
    B = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(B)
    assert B.step_bytes() == 4 * 16 + 4 * 16 + 12 + 4 * 16 + 12 == 216
    assert B.step_bytes(albedo=False, color_std=False) == 3 * 16 + 4 * 16 + 12 + 3 * 16 == 172
    assert B.orbit_args(0.3, 160, 90) == R.orbit_args(0.3, 160, 90)
    with pytest.raises(SystemExit):
        B.main(["--reps", "5"])
