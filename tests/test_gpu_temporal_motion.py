"""Temporal accumulation under moving spheres on the GPU (lrt_temporal_accumulate_moving_device /
_host, temporal_moving_kernel of learnraytracing_amd/csrc/lrt_temporal.hip) against its NumPy
restatement (tests/temporal_motion_ref.py): rendered pairs of the default scene with moved spheres,
the designed sphere cases, sphere counts around the match loop's batch, the static entry point where
nothing moves, the buffer contract and the upload's stream order, the TemporalAccumulator front end,
and what it is for: a translated sphere that keeps its history.

The house rule of tests/test_gpu_temporal.py: |got - f64| <= TOL * max(1, |f64|) at every pixel none
of whose decisions lies within 1e-4 of its threshold (the restatement's `fragile` mask), TOL = 16 x
the largest gap between the restatement's own f32 and f64 runs on the same cases
(`python tests/temporal_motion_ref.py` measures it on the CPU; tests/test_temporal_motion_cpu.py
holds the restatement to it). The matched sphere in motion.z is exact on those pixels."""
import numpy as np
import pytest

import temporal_motion_ref as M
import temporal_ref as R

pytestmark = pytest.mark.gpu

F32_F64_GAP = 7e-5                 # measured: 6.71e-05 (f32_f64_gap()), all outputs but color_std, motion included
F32_F64_GAP_STD = 3.3e-5           # measured: 3.17e-05, color_std
TOL, TOL_STD = 16 * F32_F64_GAP, 16 * F32_F64_GAP_STD
F32_F64_GAP_DESIGNED = 2.3e-5      # measured: 2.2e-05 (designed_gap())
F32_F64_GAP_STD_DESIGNED = 2.3e-5  # measured: 2.16e-05
TOL_DESIGNED, TOL_STD_DESIGNED = 16 * F32_F64_GAP_DESIGNED, 16 * F32_F64_GAP_STD_DESIGNED
F32_F64_GAP_COUNT = 5.5e-6         # measured: 5.23e-06 (count_gap(); color_std: 0, every pixel is reset)
TOL_COUNT = 16 * F32_F64_GAP_COUNT
MAX_FRAGILE = 0.02
CUR = ("normal", "world_pos", "albedo")


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _outputs(state, motion=None):
    out = {k: v[..., :3] for k, v in state.items()}
    out["n"] = state["moment2"][..., 3]
    if motion is not None:
        out["motion"] = motion
    return out


@pytest.fixture
def scene_render(gpu):
    """render(w, h, camera, frame0, spheres): one fresh 1 spp frame and its features of the default
    materials on `spheres`; the default scene is back afterwards."""
    _, mats = gpu.default_scene()

    def render(w, h, camera, frame0, spheres):
        gpu.set_scene([gpu._lib.Sphere(gpu._lib.f3(*s[:3]), float(s[3])) for s in M.sphere_array(spheres)], mats)
        buf = np.zeros((h, w, 4), np.float32)
        feats = {n: np.zeros((h, w, 4), np.float32) for n in CUR}
        gpu.render_host_features(gpu.Job(width=w, height=h, frame0=frame0, frames=1, max_depth=8, camera=camera),
                                 buf, feats, -1)
        return buf, feats
    try:
        yield render
    finally:
        gpu.set_scene(*gpu.default_scene())


def _moving(gpu, args, **params):
    """The host entry point on step()'s arguments: the restatement's outputs, motion included."""
    color, cur, prev, cam, pcam, sph, psph = args
    motion = np.full((*color.shape[:2], 4), 7.0, np.float32)
    state = gpu.temporal_accumulate_moving_host(color, cur, prev, cam, pcam, sph, psph, motion=motion, **params)
    return _outputs(state, motion)


def _check(got, want, fragile, tol, tol_std, label):
    """The house rule over every output; returns the largest gap as a share of its bound."""
    worst = 0.0
    ok = ~fragile
    assert np.array_equal(got["motion"][..., 2][ok], np.float32(want["motion"][..., 2][ok])), f"{label}: matched ids"
    assert np.array_equal(got["motion"][..., 3][ok], np.float32(want["motion"][..., 3][ok])), f"{label}: projectable"
    for name in M.MOTION_OUTPUTS:
        if name not in want:
            continue
        t = tol_std if name == "color_std" else tol
        assert np.isfinite(got[name]).all(), name
        gap = R.rel_gap(got[name], want[name], ok)
        worst = max(worst, gap / t)
        assert gap <= t, f"{label} {name}: {gap:.3g} > {t:.3g}"
    return worst


@pytest.mark.parametrize("w,h", M.SHAPES, ids=[f"{w}x{h}" for w, h in M.SHAPES])
def test_step_vs_restatement(gpu, scene_render, w, h):
    """Rendered pairs of the default scene: a Lambert and a metal sphere translated, a third resized,
    the camera one orbit step on."""
    spheres, _ = gpu.default_scene()
    worst = 0.0
    for dt in M.DTHETAS:
        args = M.rendered_case(scene_render, gpu.make_camera, spheres, w, h, dt)
        got = _moving(gpu, args, cur_scale=M.CUR_SCALE)
        info = {}
        want, fragile = M.step(*args, np.float64, info=info, cur_scale=M.CUR_SCALE)
        print(f"{w}x{h} step {dt}: fragile {100 * fragile.mean():.2f} %, matched {int(info['matched'].sum())}, "
              f"moved {int(info['moved'].sum())}, of those kept {int((info['moved'] & info['keep']).sum())}")
        assert fragile.mean() <= MAX_FRAGILE
        if w * h <= 15:
            assert not fragile.any()
        worst = max(worst, _check(got, want, fragile, TOL, TOL_STD, f"{w}x{h} step {dt}"))
    print(f"{w}x{h}: largest gap {worst:.3g} of its bound")


@pytest.mark.parametrize("case", M.DESIGNED_CASES)
def test_step_designed_cases(gpu, case):
    """The designed sphere cases (tests/test_temporal_motion_cpu.py counts their branches): every
    output against the f64 restatement, and n = 1 exactly wherever the f64 decision is to reset."""
    worst = 0.0
    for run in M.designed_runs(case):
        args = M.designed_inputs(run, gpu.make_camera)
        got = _moving(gpu, args, **run["params"])
        info = {}
        want, fragile = M.step(*args, np.float64, info=info, **run["params"])
        assert fragile.mean() <= MAX_FRAGILE
        reset = ~info["keep"] & ~fragile
        assert (got["n"][reset] == 1).all()
        worst = max(worst, _check(got, want, fragile, TOL_DESIGNED, TOL_STD_DESIGNED, run["label"]))
        if case == "analytic":
            mv = info["moved"]
            depth = 3.0 - np.float64(args[1]["world_pos"][..., 2])
            assert R.rel_gap(got["motion"][..., 0][mv], M.analytic_displacement(run["h"], depth)[mv]) <= TOL_DESIGNED
            assert (got["n"][mv] > 1).all()
        if case == "same_camera":       # an unmoved pixel and the sky take their own centre exactly
            still = ~info["moved"] & info["centred"] | ~info["hit"]
            assert (got["motion"][..., :2][still] == 0).all() and (got["motion"][..., :2][info["moved"]] != 0).any()
    print(f"{case}: largest gap {worst:.3g} of its bound")


@pytest.mark.parametrize("count", M.COUNTS)
def test_sphere_counts(gpu, count):
    """19x13 synthetic frames, each pixel a random sphere out of `count` (the match loop takes four
    per trip and stages nothing; 4096 is LRT_MAX_SPHERES): the ids, and the outputs, against the
    restatement."""
    *args, pick = M.count_inputs(count, gpu.make_camera)
    got = _moving(gpu, args, pos_tol=M.COUNT_POS_TOL)
    want, fragile = M.step(*args, np.float64, pos_tol=M.COUNT_POS_TOL)
    assert fragile.mean() <= MAX_FRAGILE
    assert np.array_equal(got["motion"][..., 2][~fragile], np.float32(pick[~fragile]))
    worst = _check(got, want, fragile, TOL_COUNT, TOL_COUNT, f"count {count}")
    print(f"count {count}: largest gap {worst:.3g} of its bound")


@pytest.fixture(scope="module")
def one_step(gpu):
    """67x45: the inputs of one rendered step with moved spheres (the scene is set and restored here:
    a module fixture cannot use scene_render)."""
    w, h = 67, 45
    spheres, mats = gpu.default_scene()

    def render(w, h, camera, frame0, sph):
        gpu.set_scene([gpu._lib.Sphere(gpu._lib.f3(*s[:3]), float(s[3])) for s in M.sphere_array(sph)], mats)
        buf = np.zeros((h, w, 4), np.float32)
        feats = {n: np.zeros((h, w, 4), np.float32) for n in CUR}
        gpu.render_host_features(gpu.Job(width=w, height=h, frame0=frame0, frames=1, max_depth=8, camera=camera),
                                 buf, feats, -1)
        return buf, feats
    try:
        args = M.rendered_case(render, gpu.make_camera, spheres, w, h, 0.02)
    finally:
        gpu.set_scene(spheres, mats)
    return dict(w=w, h=h, args=args)


def test_no_motion_is_the_static_step(gpu, one_step):
    """prev_spheres equal to spheres: every output within TOL of lrt_temporal_accumulate_host's on the
    same inputs (two instances of one pixel function, which the compiler may contract differently),
    n equal wherever neither restatement's pixel is fragile; under identical cameras too, where
    both take the pixel's own centre."""
    color, cur, prev, cam, pcam, sph, _ = one_step["args"]
    got = _outputs(gpu.temporal_accumulate_moving_host(color, cur, prev, cam, pcam, sph, sph.copy(), cur_scale=M.CUR_SCALE))
    static = _outputs(gpu.temporal_accumulate_host(color, cur, prev, cam, pcam, cur_scale=M.CUR_SCALE))
    _, f1 = M.step(color, cur, prev, cam, pcam, sph, sph, np.float64, cur_scale=M.CUR_SCALE)
    _, f2 = R.step(color, cur, prev, cam, pcam, np.float64, cur_scale=M.CUR_SCALE)
    for name in R.OUTPUTS:
        gap = R.rel_gap(got[name], static[name])
        assert gap <= (TOL_STD if name == "color_std" else TOL), name
    ok = ~(f1 | f2)
    assert np.array_equal(got["n"][ok], static["n"][ok])
    self_prev = R.random_prev({k: cur[k] * np.float32(M.CUR_SCALE) for k in ("normal", "world_pos")}, 9)
    hmot = np.zeros((*color.shape[:2], 4), np.float32)
    got = _outputs(gpu.temporal_accumulate_moving_host(color, cur, self_prev, cam, None, sph, sph, motion=hmot,
                                                       cur_scale=M.CUR_SCALE))
    static = _outputs(gpu.temporal_accumulate_host(color, cur, self_prev, cam, None, cur_scale=M.CUR_SCALE))
    for name in R.OUTPUTS:
        assert R.rel_gap(got[name], static[name]) <= (TOL_STD if name == "color_std" else TOL), name
    assert (got["n"] > 1).mean() > 0.9
    assert ((hmot[..., :2] == 0).all(-1)).mean() > 0.9       # their own centre, exactly


def test_contract(gpu, one_step):
    import torch
    from learnraytracing_amd import LrtError
    L = gpu._lib
    s = one_step
    w, h = s["w"], s["h"]
    color, cur, prev, cam, pcam, sph, psph = s["args"]
    kw = dict(cur_scale=M.CUR_SCALE)
    keep = [a.copy() for a in (color, *cur.values(), *prev.values(), sph, psph)]
    names = R.STATE_NAMES + ("color_std",)
    hout = {n: np.full((h, w, 4), 7.0, np.float32) for n in names}
    hmot = np.full((h, w, 4), np.nan, np.float32)
    assert gpu.temporal_accumulate_moving_host(color, cur, prev, cam, pcam, sph, psph, out=hout, motion=hmot, **kw) is hout
    for a, b in zip((color, *cur.values(), *prev.values(), sph, psph), keep):     # inputs untouched
        assert np.array_equal(_bits(a), _bits(b))
    assert np.isfinite(hmot).all()                                                 # all four channels written
    assert set(np.unique(hmot[..., 3])) <= {0.0, 1.0} and (hmot[..., 2] >= -1).all()
    assert (hout["color"][..., 3] == 7.0).all() and (hout["color_std"][..., 3] == 7.0).all()
    # motion is optional and changes nothing else; two runs give the same bits
    again = gpu.temporal_accumulate_moving_host(color, cur, prev, cam, pcam, sph, psph, **kw)
    for n in names:
        assert np.array_equal(_bits(again[n][..., :3]), _bits(hout[n][..., :3])), n
    hmot2 = np.zeros_like(hmot)
    gpu.temporal_accumulate_moving_host(color, cur, prev, cam, pcam, sph, psph, motion=hmot2, **kw)
    assert np.array_equal(_bits(hmot2), _bits(hmot))
    # without a previous state: everything reset, motion (0, 0, -1, 0)
    first = gpu.temporal_accumulate_moving_host(color, cur, None, cam, pcam, sph, psph, motion=hmot2, **kw)
    assert (first["moment2"][..., 3] == 1).all() and (hmot2 == np.float32([0, 0, -1, 0])).all()
    # the device form: the same bits, asynchronous on its stream
    dev = torch.device("cuda:0")
    up = lambda d: {k: torch.from_numpy(v).to(dev) for k, v in d.items()}   # noqa: E731
    tcolor, tcur, tprev = torch.from_numpy(color).to(dev), up(cur), up(prev)
    tout = {n: torch.full((h, w, 4), 7.0, device=dev) for n in names}
    tmot = torch.full((h, w, 4), 7.0, device=dev)
    assert gpu.temporal_accumulate_moving_tensor(tcolor, tcur, tprev, cam, pcam, sph, psph, out=tout, motion=tmot,
                                                 **kw) is tout
    torch.cuda.synchronize()
    for n in names:
        assert np.array_equal(_bits(tout[n].cpu().numpy()), _bits(hout[n])), n
    assert np.array_equal(_bits(tmot.cpu().numpy()), _bits(hmot))
    # back-to-back calls on one stream with different scenes each use their own spheres: the
    # second upload may not overtake the first kernel, nor the caller's arrays be read late
    st = torch.cuda.Stream(dev)
    other = psph.copy()
    other[M.LAMBERT_ID, :3] += np.float32([0.3, 0.0, 0.1])
    want_other = np.zeros_like(hmot)
    hother = gpu.temporal_accumulate_moving_host(color, cur, prev, cam, pcam, sph, other, motion=want_other, **kw)
    assert not np.array_equal(want_other, hmot)
    assert not np.array_equal(hother["color"][..., :3], hout["color"][..., :3])
    with torch.cuda.stream(st):
        outs = [{n: torch.zeros((h, w, 4), device=dev) for n in names} for _ in range(6)]
        mots = [torch.zeros((h, w, 4), device=dev) for _ in range(6)]
        st.synchronize()
        for i in range(6):
            scratch = (psph if i % 2 == 0 else other).copy()
            gpu.temporal_accumulate_moving_tensor(tcolor, tcur, tprev, cam, pcam, sph, scratch, out=outs[i],
                                                  motion=mots[i], stream=st, **kw)
            scratch[:] = 99.0            # the call has read it
    st.synchronize()
    for i in range(6):
        assert np.array_equal(_bits(mots[i].cpu().numpy()), _bits(hmot if i % 2 == 0 else want_other)), i
        assert np.array_equal(_bits(outs[i]["color"].cpu().numpy()[..., :3]),
                              _bits((hout if i % 2 == 0 else hother)["color"][..., :3])), i
    # LRT_E_INVALID: the scene's cases through the front end, and motion on every other buffer
    bad_nan = sph.copy()
    bad_nan[3, 1] = np.inf
    for a, b in ((bad_nan, psph), (sph, bad_nan)):
        with pytest.raises(LrtError) as e:
            gpu.temporal_accumulate_moving_tensor(tcolor, tcur, tprev, cam, pcam, a, b, out=tout, **kw)
        assert e.value.code == L.LRT_E_INVALID
    for t in [tcolor, *tcur.values(), *tprev.values(), *tout.values()]:
        with pytest.raises(LrtError) as e:
            gpu.temporal_accumulate_moving_tensor(tcolor, tcur, tprev, cam, pcam, sph, psph, out=tout, motion=t, **kw)
        assert e.value.code == L.LRT_E_INVALID
    with pytest.raises(LrtError):      # what the static call rejects
        gpu.temporal_accumulate_moving_tensor(tcolor, tcur, tprev, cam, pcam, sph, psph, out=dict(tout, color=tcolor), **kw)
    import ctypes
    d = gpu.temporal_desc(w, h, cam, pcam, **kw)
    sm = gpu.renderer._scene_motion(sph, psph)
    f = L.Features()
    f.normal, f.world_pos = tcur["normal"].data_ptr(), tcur["world_pos"].data_ptr()
    ns = L.TemporalState()
    for n in R.STATE_NAMES[:4]:
        setattr(ns, n, tout[n].data_ptr())

    def raw(scene):
        return L.lib().lrt_temporal_accumulate_moving_device(ctypes.byref(d), ctypes.byref(scene) if scene else None,
                                                             tcolor.data_ptr(), ctypes.byref(f), None, ctypes.byref(ns),
                                                             None, None, None)
    assert raw(None) == L.LRT_E_INVALID
    null = ctypes.POINTER(L.Sphere)()
    for member, value in (("count", 0), ("count", L.MAX_SPHERES + 1), ("reserved", 2), ("spheres", null),
                          ("prev_spheres", null)):
        bad = gpu.renderer._scene_motion(sph, psph)
        setattr(bad, member, value)
        assert raw(bad) == L.LRT_E_INVALID, member
    assert raw(sm) == 0
    torch.cuda.synchronize()
    for n in names:                    # the refused calls wrote nothing (the last, valid one had no history)
        if n in ("albedo", "color_std"):
            assert np.array_equal(_bits(tout[n].cpu().numpy()), _bits(hout[n])), n


def test_uploaded_scenes_keep_stream_order(gpu):
    """More than INLINE_SPHERES spheres go through an upload into the stream's scratch: back-to-back
    calls on one stream with different scenes (and sizes, 257 and 65, so that the scratch is reused
    at another length) each use their own spheres, and equal the blocking host form bit for bit."""
    import torch
    dev = torch.device("cuda:0")
    cases = []
    for count in (257, M.INLINE_SPHERES + 1, 257):
        color, cur, prev, cam, pcam, sph, psph, _ = M.count_inputs(count, gpu.make_camera, seed=len(cases))
        assert count > M.INLINE_SPHERES
        hmot = np.zeros((*color.shape[:2], 4), np.float32)
        gpu.temporal_accumulate_moving_host(color, cur, prev, cam, pcam, sph, psph, motion=hmot, pos_tol=M.COUNT_POS_TOL)
        up = lambda d: {k: torch.from_numpy(v).to(dev) for k, v in d.items()}   # noqa: E731
        cases.append((torch.from_numpy(color).to(dev), up(cur), up(prev), cam, pcam, sph, psph, hmot))
    assert not np.array_equal(cases[0][7], cases[2][7])
    st = torch.cuda.Stream(dev)
    h, w = cases[0][7].shape[:2]
    with torch.cuda.stream(st):
        mots = [torch.zeros((h, w, 4), device=dev) for _ in range(9)]
    st.synchronize()
    for i in range(9):
        tcolor, tcur, tprev, cam, pcam, sph, psph, _ = cases[i % 3]
        gpu.temporal_accumulate_moving_tensor(tcolor, tcur, tprev, cam, pcam, sph, psph, motion=mots[i], stream=st,
                                              pos_tol=M.COUNT_POS_TOL)
    st.synchronize()
    for i in range(9):
        assert np.array_equal(_bits(mots[i].cpu().numpy()), _bits(cases[i % 3][7])), i


def test_accumulator_with_spheres(gpu, one_step):
    """TemporalAccumulator.step(spheres=): the first step takes the scene as its own predecessor, the
    next one remembers it; without spheres it is the static call."""
    import torch
    color, cur, prev, cam, pcam, sph, psph = one_step["args"]
    w, h = one_step["w"], one_step["h"]
    dev = torch.device("cuda:0")
    tcur = {k: torch.from_numpy(v).to(dev) for k, v in cur.items()}
    tcolor = torch.from_numpy(color).to(dev)
    acc = gpu.TemporalAccumulator(w, h, dev)
    mot = torch.full((h, w, 4), 7.0, device=dev)
    acc.step(tcolor, tcur, pcam, cur_scale=M.CUR_SCALE, spheres=psph, motion=mot)
    torch.cuda.synchronize()
    assert (mot.cpu().numpy() == np.float32([0, 0, -1, 0])).all()
    first = {k: v.cpu().numpy() for k, v in acc.state.items()}
    tcol, guides = acc.step(tcolor, tcur, cam, cur_scale=M.CUR_SCALE, spheres=sph, motion=mot)
    torch.cuda.synchronize()
    hmot = np.zeros((h, w, 4), np.float32)
    want = gpu.temporal_accumulate_moving_host(color, cur, {k: first[k] for k in R.STATE_NAMES}, cam, pcam, sph, psph,
                                               motion=hmot, cur_scale=M.CUR_SCALE)
    assert np.array_equal(_bits(tcol.cpu().numpy()[..., :3]), _bits(want["color"][..., :3]))
    assert np.array_equal(_bits(mot.cpu().numpy()), _bits(hmot))
    assert set(guides) == set(gpu._lib.GUIDE_NAMES)
    moved_ids = set(np.unique(hmot[..., 2][(np.abs(hmot[..., :2]) > 0.5).any(-1)]).tolist())
    assert {float(M.LAMBERT_ID), float(M.METAL_ID)} <= moved_ids
    acc.reset()                        # after a reset the scene serves as its own predecessor again
    acc.step(tcolor, tcur, pcam, cur_scale=M.CUR_SCALE, spheres=psph)
    acc.step(tcolor, tcur, cam, cur_scale=M.CUR_SCALE, spheres=sph, motion=mot)
    torch.cuda.synchronize()
    assert np.array_equal(_bits(mot.cpu().numpy()), _bits(hmot))
    with pytest.raises(gpu.LrtError):
        acc.step(tcolor, tcur, cam, motion=mot)


def test_quality_moving_sphere_on_gpu(gpu, scene_render):
    """tests/test_temporal_motion_cpu.py::test_quality_moving_sphere the whole way through the
    library: 16 steps of 1 spp while Lambert sphere MOVING_ID comes down, against 1024 spp of the
    final scene. Over the final frame's pixels matched to that sphere: relMSE of the moving
    accumulation < the static one's and <= QUALITY_BAR (0.175 = 1.25 x the f64 restatement's 0.14 on
    the oracle's frames) x the single frame's; over the whole frame it does not exceed the static
    run's."""
    q = M.QUALITY
    spheres, _ = gpu.default_scene()
    frames = M.moving_frames(scene_render, gpu.make_camera, spheres)
    cam = frames[-1][2]
    gpu.set_scene(*gpu.default_scene())
    gt = np.zeros((q["h"], q["w"], 4), np.float32)
    gpu.render_host(gpu.Job(width=q["w"], height=q["h"], frames=q["gt_spp"], max_depth=q["depth"], camera=cam), gt)
    st_s, st_m, prev_sph = None, None, frames[0][4]
    motion = np.zeros((q["h"], q["w"], 4), np.float32)
    for color, feats, cam, k, sph in frames:
        st_s = gpu.temporal_accumulate_host(color, feats, st_s, cam, cam, cur_scale=k)
        st_m = gpu.temporal_accumulate_moving_host(color, feats, st_m, cam, cam, sph, prev_sph, motion=motion, cur_scale=k)
        prev_sph = sph
    on = motion[..., 2] == M.MOVING_ID
    color, _, _, k, _ = frames[-1]
    single = color * np.float32(k)
    r1, rs, rm = M.rel_mse(single, gt, on), M.rel_mse(st_s["color"], gt, on), M.rel_mse(st_m["color"], gt, on)
    ws, wm = M.rel_mse(st_s["color"], gt), M.rel_mse(st_m["color"], gt)
    print(f"sphere {M.MOVING_ID} ({int(on.sum())} px): relMSE single {r1:.4g}, static {rs:.4g}, moving {rm:.4g} "
          f"({rm / r1:.4f}x; bar {M.QUALITY_BAR:.4f}); whole frame: static {ws:.4g}, moving {wm:.4g}")
    assert on.sum() >= 150
    assert (st_s["moment2"][..., 3][on] == 1).all()      # the static step has reset them
    assert rm < rs
    assert rm <= M.QUALITY_BAR * r1
    assert wm <= ws
