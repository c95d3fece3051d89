"""Temporal upsampling on the GPU (lrt_temporal_upsample_device / _host, temporal_upsample_kernel of
learnraytracing_amd/csrc/lrt_temporal_upsample.hip) against its NumPy restatement
(tests/temporal_upsample_ref.py): the library's own G-buffer planes (the low one under jitter_camera)
and pool-kernel colours at the low size, two steps per case (no history, then a history step against
a moved camera and moved spheres) under four jitters, sphere counts on either side of the grid, the
designed cases, the buffer contract, the TemporalUpsampler front end, and what it is for: a frame
rebuilt exactly from its jittered samples, and spheres smaller than a low pixel that a later phase hits.

The house rule of tests/test_gpu_temporal.py: |got - f64| <= TOL * max(1, |f64|) at every pixel none
of whose decisions lies within its margin of its threshold (the restatement's `fragile` mask), and
the class plane equal there; TOL = 16 x the largest gap between the restatement's own f32 and f64
runs on the same cases (`python tests/temporal_upsample_ref.py` measures it on the CPU;
tests/test_temporal_upsample_cpu.py holds the restatement to it and to the fragile share)."""
import numpy as np
import pytest

import gbuffer_ref as G
import temporal_gbuffer_ref as TG
import temporal_ref as R
import temporal_upsample_ref as TU

pytestmark = pytest.mark.gpu

F32_F64_GAP = 1.1e-6                # measured: 1.03e-06 (rendered_gap()), color, moment2 and n
F32_F64_GAP_STD = 0.0               # measured: 0, color_std (n <= 2 after two steps: short_std itself, exactly)
TOL, TOL_STD = 16 * F32_F64_GAP, 16 * F32_F64_GAP_STD
F32_F64_GAP_DESIGNED = 2.7e-7       # measured: 2.51e-07 (designed_gap())
F32_F64_GAP_STD_DESIGNED = 1.5e-6   # measured: 1.44e-06
TOL_DESIGNED, TOL_STD_DESIGNED = 16 * F32_F64_GAP_DESIGNED, 16 * F32_F64_GAP_STD_DESIGNED
SENTINEL = 7.0
GUARD = 64
POOL = 512   # LRT_F_POOL
OUT = ("color", "moment2", "color_std")
UPSAMPLE_CLASS0_1000 = 564          # lrt_upsample's class-0 pixels of random_scene(1000, 1) at 38 x 26 from 19 x 13


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _spheres(L, arr):
    return [L.Sphere(L.f3(*s[:3]), float(s[3])) for s in G.sphere_array(arr)]


def _outputs(state):
    return dict(color=state["color"][..., :3], moment2=state["moment2"][..., :3], n=state["moment2"][..., 3],
                color_std=state["color_std"][..., :3])


@pytest.fixture
def scene(gpu):
    """set(spheres, materials); the default scene is back afterwards."""
    try:
        yield gpu.set_scene
    finally:
        gpu.set_scene(*gpu.default_scene())


def _library(gpu, scene):
    """(planes, colour) as temporal_upsample_ref.rendered_case takes them: the library's own G-buffer
    (gbuffer_host) and the pool kernel's colours."""
    L = gpu._lib

    def planes(w, h, camera, spheres, mats, prev_camera, prev_spheres):
        scene(_spheres(L, spheres), mats)
        if prev_camera is None:
            return gpu.gbuffer_host(w, h, camera, id=True)
        return gpu.gbuffer_host(w, h, camera, prev_camera, id=True, motion=True, prev_spheres=prev_spheres)

    def colour(w, h, camera, spheres, mats, frame0):
        scene(_spheres(L, spheres), mats)
        buf = np.zeros((h, w, 4), np.float32)
        gpu.render_host(gpu.Job(width=w, height=h, frame0=frame0, frames=1, max_depth=8, camera=camera, flags=POOL), buf)
        return buf

    return planes, colour


def _case(gpu, scene, count, w, h, lw, lh, jit_a, jit_b):
    planes, colour = _library(gpu, scene)
    return TU.rendered_case(count, w, h, lw, lh, jit_a, jit_b, TU.scene_of(gpu.default_scene, gpu.random_scene),
                            gpu.make_camera, gpu.jitter_camera, planes, colour)


def _run(gpu, s, prev_g, prev, **params):
    """One step through the host entry point: (state, class plane)."""
    h, w = s["cur"]["id"].shape
    cls = np.full((h, w), -9, np.int32)
    st = gpu.temporal_upsample_host(s["color_low"], s["low"], s["cur"], prev_g, prev, class_out=cls, jitter=s["jitter"],
                                    **params)
    return st, cls


def _check(got, cls, want, fragile, tol, tol_std, label):
    """The house rule over every output and the class plane; returns the largest gap as a share of its bound."""
    state, wcls, _ = want
    worst, ok = 0.0, ~fragile
    gaps = {}
    for name in TU.OUTPUTS:
        t = tol_std if name == "color_std" else tol
        assert np.isfinite(got[name]).all(), name
        gaps[name] = R.rel_gap(got[name], state[name], ok)
        print(f"{label} {name}: gap {gaps[name]:.3g} (bound {t:.3g})")
        worst = max(worst, gaps[name] / t if t else float(gaps[name] > 0))
    assert np.array_equal(cls[ok], wcls[ok]), f"{label}: classes"
    for name in TU.OUTPUTS:
        t = tol_std if name == "color_std" else tol
        assert gaps[name] <= t, f"{label} {name}: {gaps[name]:.3g} > {t:.3g}"
    return worst


CASES = [(f"{label.replace(' ', '')}-{name}", count, w, h, lw, lh, k)
         for label, count, w, h, lw, lh in TU.RENDERED_CASES for k, name in enumerate(TU.JITTER_NAMES)]


@pytest.mark.parametrize("label,count,w,h,lw,lh,k", CASES, ids=[c[0] for c in CASES])
def test_step_vs_restatement(gpu, scene, label, count, w, h, lw, lh, k):
    """Two steps per case and jitter: the previous frame (one orbit step back, the moved scene) under the
    jitter before this one in the list, with no history; then the current frame under this jitter, its
    history the state the library returned. The restatement reads the same arrays the library was given."""
    jits = TU.case_jitters(w, h, lw, lh)
    a, b = _case(gpu, scene, count, w, h, lw, lh, jits[k - 1], jits[k])
    first, cls_a = _run(gpu, a, None, None, **TU.RENDERED_PARAMS)
    prev_g = {n: a["cur"][n] for n in ("normal", "id")}
    second, cls_b = _run(gpu, b, prev_g, first, **TU.RENDERED_PARAMS)
    want_a, want_b = TU.two_steps(a, b, np.float64, first=first)
    worst = 0.0
    for step, got, cls, want in (("a", first, cls_a, want_a), ("b", second, cls_b, want_b)):
        fragile = want[2]
        print(f"{label} step {step}: fragile {100 * fragile.mean():.2f} %, class 0 / 1 / 2 / 3: "
              + " / ".join(map(str, TU.class_counts(want[1]))))
        assert fragile.mean() <= TU.MAX_FRAGILE
        worst = max(worst, _check(_outputs(got), cls, want, fragile, TOL, TOL_STD, f"{label} {step}"))
    assert ((cls_a == 2) | (cls_a == 3)).all()                         # no history: classes 2 and 3 only
    assert (first["moment2"][..., 3][cls_a == 3] == 0).all()
    print(f"{label}: largest gap {worst:.3g} of its bound")


@pytest.mark.parametrize("case", TU.DESIGNED_CASES)
def test_step_designed_cases(gpu, case):
    """The designed cases (tests/test_temporal_upsample_cpu.py holds their classes): every output and the
    class plane against the f64 restatement; n = 0 exactly in class 3; beta = 1 exactly on an aligned pixel."""
    color, low, cur, prev_g, prev, jitter, params, expect = TU.designed_inputs(case)
    s = dict(color_low=color, low=low, cur=cur, jitter=jitter)
    got, cls = _run(gpu, s, prev_g, prev, **params)
    info = {}
    want = TU.step(color, low, cur, prev_g, prev, jitter, np.float64, info=info, **params)
    assert want[2].mean() <= TU.MAX_FRAGILE
    worst = _check(_outputs(got), cls, want, want[2], TOL_DESIGNED, TOL_STD_DESIGNED, case)
    mask, value = expect["cls"]
    value = np.asarray(value)
    assert np.array_equal(cls[mask], np.broadcast_to(value[mask] if value.shape == mask.shape else value, cls[mask].shape))
    n = got["moment2"][..., 3]
    assert (n[cls == 3] == 0).all()
    if "beta_is_1" in expect:                                           # n = n_h + 1 there, n_h the history's own n'
        on = expect["beta_is_1"][0]
        assert np.array_equal(n[on], prev["moment2"][..., 3][on] + np.float32(1))
    print(f"{case}: largest gap {worst:.3g} of its bound")


def test_a_tap_of_b_zero_adds_nothing(gpu):
    """A NaN / Inf colour changes nothing, bit for bit, at the pixels that give its tap no weight > 0
    (a tap of b = 0 among them), and reaches the others."""
    color, zeroed, low, cur, prev_g, prev, jitter, untouched, b0 = TU.nan_inputs()
    assert b0.any()
    a, ca = _run(gpu, dict(color_low=color, low=low, cur=cur, jitter=jitter), prev_g, prev)
    b, cb = _run(gpu, dict(color_low=zeroed, low=low, cur=cur, jitter=jitter), prev_g, prev)
    assert np.array_equal(ca, cb)
    for name in OUT:
        assert np.isfinite(a[name][untouched]).all(), name
        assert np.array_equal(_bits(a[name][untouched]), _bits(b[name][untouched])), name
    assert not np.isfinite(a["color"][~untouched][..., :3]).all(axis=-1).any()


def test_underflowed_beta_over_an_empty_history(gpu):
    """beta = n_h = 0 (every k underflows under sigma_sample 0.03, the history's count is 0): alpha is
    max(0 / 0, 0) = 0 in the kernel as in the f32 restatement: finite everywhere, the history kept and
    n = 0 there, the class plane and the rest as the f32 restatement has them."""
    color, low, cur, prev_g, prev, jitter, params, mask = TU.beta_zero_inputs()
    got, cls = _run(gpu, dict(color_low=color, low=low, cur=cur, jitter=jitter), prev_g, prev, **params)
    want, wcls, fragile = TU.step(color, low, cur, prev_g, prev, jitter, np.float32, **params)
    assert np.array_equal(fragile, mask) and np.array_equal(cls, wcls)
    got = _outputs(got)
    for name in TU.OUTPUTS:
        tol = TOL_STD_DESIGNED if name == "color_std" else TOL_DESIGNED
        assert np.isfinite(got[name]).all(), name
        gap = R.rel_gap(got[name], want[name])
        print(f"{name}: gap to the f32 restatement {gap:.3g} (bound {tol:.3g})")
        assert gap <= tol, name
    assert (got["n"][mask] == 0).all()
    assert R.rel_gap(got["color"][mask], prev["color"][..., :3][mask]) <= TOL_DESIGNED


@pytest.mark.parametrize("w,h,lw,lh", TU.CONVERGE_SIZES)
def test_jittered_samples_rebuild_the_frame(gpu, w, h, lw, lh):
    """tests/test_temporal_upsample_cpu.py's derivable check on the device: the first step all class 2,
    the later ones all class 0, the first three far from the target and the fourth on it, within 16 x
    what the restatement's own f32 run leaves."""
    def fn(color, low, cur, prev_g, prev, jitter):
        s = dict(color_low=np.float32(color), low=low, cur=cur, jitter=jitter)
        return _run(gpu, s, prev_g, prev, sigma_sample=TU.CONVERGE_SIGMA)

    ref32 = TU.converge_ref(w, h, lw, lh, np.float32)
    bound = 16 * ref32[3][1]
    assert 0 < bound < 1e-6
    steps = TU.converge(w, h, lw, lh, fn)
    print(f"{w}x{h} from {lw}x{lh}: |color - T| per step " + ", ".join(f"{e:.3g}" for _, e in steps)
          + f" (the f32 restatement: {ref32[3][1]:.3g}, bound {bound:.3g})")
    assert (steps[0][0] == 2).all()
    for cls, _ in steps[1:]:
        assert (cls == 0).all()
    assert all(e > 0.1 for _, e in steps[:3])
    assert steps[3][1] <= bound


@pytest.fixture(scope="module")
def one_step(gpu):
    """{(w, h): (a, b, the state of a)}: 67 x 45 from 33 x 22 under (7, -3) and 1 x 1 from 1 x 1, rendered
    once (the scene is set and restored here: a module fixture cannot use `scene`)."""
    out = {}
    try:
        for w, h, lw, lh, jit in ((67, 45, 33, 22, (7, -3)), (1, 1, 1, 1, (1, -1))):
            a, b = _case(gpu, gpu.set_scene, 9, w, h, lw, lh, (0, 0), jit)
            out[(w, h)] = (a, b, _run(gpu, a, None, None, **TU.RENDERED_PARAMS)[0])
    finally:
        gpu.set_scene(*gpu.default_scene())
    return out


def test_ratio_one_is_the_gbuffer_step(gpu, scene):
    """19 x 13 from 19 x 13 with jitter 0, the frame's own planes as the low ones: the outputs agree with
    temporal_accumulate_gbuffer_host's within TOL, class 0 where n > 1 there and 2 where it resets."""
    w, h = 19, 13
    planes, colour = _library(gpu, scene)
    color, cur, prev_g, prev = TG.rendered_case(w, h, 9, TG.scene_of(gpu.default_scene, gpu.random_scene), gpu.make_camera,
                                                planes, colour)
    want = _outputs(gpu.temporal_accumulate_gbuffer_host(color, cur, prev_g, prev, cur_scale=TG.CUR_SCALE))
    s = dict(color_low=color, low={k: cur[k] for k in ("id", "normal")}, cur=cur, jitter=(0, 0))
    got, cls = _run(gpu, s, prev_g, prev, cur_scale=TG.CUR_SCALE)
    got = _outputs(got)
    for name in TU.OUTPUTS:
        gap = R.rel_gap(got[name], want[name])
        print(f"{name}: gap {gap:.3g} (bound {TOL:.3g})")
        assert gap <= TOL, name
    assert np.array_equal(cls, np.where(want["n"] > 1, 0, 2))


@pytest.mark.parametrize("w,h", [(67, 45), (1, 1)], ids=["67x45", "1x1"])
def test_contract(gpu, one_step, w, h):
    """Host and tensor (device) forms give the same bits; the alphas of next->color and color_std stay;
    64 sentinel words behind every output stay; every input is unchanged; color_std and class_out are
    optional and change nothing else; a refused call writes nothing."""
    import torch
    L = gpu._lib
    dev = torch.device("cuda:0")
    a, b, prev = one_step[(w, h)]
    prev = {k: prev[k] for k in ("color", "moment2")}
    prev_g = {k: a["cur"][k] for k in ("normal", "id")}
    kw = dict(jitter=b["jitter"], **TU.RENDERED_PARAMS)
    inputs = (b["color_low"], *b["low"].values(), *b["cur"].values(), *prev_g.values(), *prev.values())
    keep = [x.copy() for x in inputs]
    hout = {n: np.full((h, w, 4), SENTINEL, np.float32) for n in OUT}
    hcls = np.full((h, w), -9, np.int32)
    assert gpu.temporal_upsample_host(b["color_low"], b["low"], b["cur"], prev_g, prev, out=hout, class_out=hcls, **kw) is hout
    for x, y in zip(inputs, keep):
        assert np.array_equal(_bits(x), _bits(y))
    assert (hout["color"][..., 3] == SENTINEL).all() and (hout["color_std"][..., 3] == SENTINEL).all()
    assert np.isfinite(hout["moment2"]).all() and ((hcls >= 0) & (hcls <= 3)).all()
    # color_std and class_out are optional and change nothing else
    plain = gpu.temporal_upsample_host(b["color_low"], b["low"], b["cur"], prev_g, prev,
                                       out={n: np.zeros((h, w, 4), np.float32) for n in OUT[:2]}, **kw)
    assert set(plain) == set(OUT[:2])
    assert np.array_equal(_bits(plain["moment2"]), _bits(hout["moment2"]))
    assert np.array_equal(_bits(plain["color"][..., :3]), _bits(hout["color"][..., :3]))
    # the tensor form: every output with a guard behind it, on a stream of its own
    up = lambda d: {k: torch.from_numpy(v).to(dev) for k, v in d.items()}   # noqa: E731
    tcolor, tlow, tcur, tprev_g, tprev = torch.from_numpy(b["color_low"]).to(dev), up(b["low"]), up(b["cur"]), up(prev_g), \
        up(prev)
    n4 = w * h * 4
    tout = {n: torch.full((n4 + GUARD,), SENTINEL, device=dev) for n in OUT}
    tcls = torch.full((w * h + GUARD,), -9, dtype=torch.int32, device=dev)
    st = torch.cuda.Stream(dev)
    st.wait_stream(torch.cuda.current_stream(dev))
    assert gpu.temporal_upsample_tensor(tcolor, tlow, tcur, tprev_g, tprev, out=tout, class_out=tcls, stream=st, **kw) is tout
    st.synchronize()
    for n in OUT:
        t = tout[n].cpu().numpy()
        assert np.array_equal(_bits(t[:n4]), _bits(hout[n]).ravel()), n      # (the sentinel alphas included)
        assert (t[n4:] == SENTINEL).all(), f"{n}: guard"
    c = tcls.cpu().numpy()
    assert np.array_equal(c[:w * h], hcls.ravel()) and (c[w * h:] == -9).all()
    for t, x in zip((tcolor, *tlow.values(), *tcur.values(), *tprev_g.values(), *tprev.values()), keep):
        assert np.array_equal(_bits(t.cpu().numpy()), _bits(x))
    # a refused call writes nothing: an output on an input, exactly one of prev and prev_g, a jitter too far
    snap = {n: tout[n].clone() for n in OUT}
    for bad in (dict(out=dict(tout, color=tcur["normal"])), dict(prev=None), dict(prev_g=None),
                dict(prev_g=dict(tprev_g, id=tcur["id"])), dict(jitter=(w + 1, 0)), dict(class_out=tcur["id"])):
        args = dict(prev_g=tprev_g, prev=tprev, out=tout, class_out=tcls, **kw)
        args.update(bad)
        with pytest.raises(gpu.LrtError) as e:
            gpu.temporal_upsample_tensor(tcolor, tlow, tcur, args.pop("prev_g"), args.pop("prev"), **args)
        assert e.value.code == L.LRT_E_INVALID
    torch.cuda.synchronize()
    for n in OUT:
        assert torch.equal(tout[n], snap[n]), n
    assert np.array_equal(tcls.cpu().numpy(), c)


def test_state_after_shutdown(gpu, one_step):
    """Without lrt_initialize(): LRT_E_STATE (tests/test_gpu_gbuffer.py shuts down and comes back the
    same way)."""
    L = gpu._lib
    a, _, _ = one_step[(1, 1)]
    gpu.ShutdownTest()
    try:
        with pytest.raises(gpu.LrtError) as e:
            _run(gpu, a, None, None)
        assert e.value.code == L.LRT_E_STATE
    finally:
        gpu.InitializeTest()
    assert _run(gpu, a, None, None)[1][0, 0] in (2, 3)


def test_upsampler_front_end(gpu):
    """38 x 26 from 19 x 13: six steps of jitter_phases through TemporalUpsampler equal the chained
    temporal_upsample_tensor calls bit for bit; gbuffer_planes() hands out its two sets in turn; the
    previous step's planes handed in again are refused; reset() drops the history. Then the chain at
    66 x 44 from 33 x 22: svgf_filter_tensor on the upsampler's state is finite everywhere."""
    import torch
    L = gpu._lib
    dev = torch.device("cuda:0")
    for (w, h, lw, lh), steps in (((38, 26, 19, 13), 6), ((66, 44, 33, 22), 2)):
        cam = gpu.default_camera(w, h)
        up = gpu.TemporalUpsampler(w, h, lw, lh, dev)
        phases = gpu.jitter_phases(w, lw, h, lh)
        gen = torch.Generator(device=dev).manual_seed(w)
        prev_g = prev = None
        for t in range(steps):
            jit = phases[t % len(phases)]
            color = torch.rand((lh, lw, 4), device=dev, generator=gen) + 0.05
            low = gpu.gbuffer_tensor(lw, lh, gpu.jitter_camera(cam, w, h, lw, lh, *jit), id=True)
            planes = up.gbuffer_planes()
            assert set(planes) == set(L.TEMPORAL_GBUFFER_PLANES)
            assert prev_g is None or planes["normal"] is not prev_g["normal"]
            assert gpu.gbuffer_tensor(w, h, cam, out=planes) is planes
            cls = torch.zeros((h, w), dtype=torch.int32, device=dev)
            col, guides = up.step(color, low, planes, jitter=jit, cur_scale=2.0, class_out=cls)
            assert set(guides) == {"color_std"} and col is up.state["color"] and set(up.state) == {"color", "moment2"}
            want = gpu.temporal_upsample_tensor(color, low, planes, prev_g, prev, jitter=jit, cur_scale=2.0)
            torch.cuda.synchronize()
            for k, got in (("color", col), ("moment2", up.state["moment2"]), ("color_std", guides["color_std"])):
                assert np.array_equal(_bits(got.cpu().numpy()[..., :3]), _bits(want[k].cpu().numpy()[..., :3])), (t, k)
            assert torch.equal(up.state["moment2"][..., 3], want["moment2"][..., 3])
            assert bool(((cls == 2) | (cls == 3)).all()) == (t == 0)
            with pytest.raises(gpu.LrtError) as e:                        # the planes it now holds as history
                up.step(color, low, dict(planes), jitter=jit)
            assert e.value.code == L.LRT_E_INVALID
            prev_g, prev = {k: planes[k] for k in ("normal", "id")}, {k: v.clone() for k, v in want.items()}
        st = up.state
        out = gpu.svgf_filter_tensor(st["color"], st["moment2"], {k: planes[k] for k in ("normal", "world_pos", "albedo")})
        torch.cuda.synchronize()
        assert out.shape == (h, w, 4) and torch.isfinite(out).all()
        up.reset()
        cls = torch.zeros((h, w), dtype=torch.int32, device=dev)
        up.step(color, low, planes, jitter=jit, class_out=cls)          # after reset() nothing is held: the same planes pass
        torch.cuda.synchronize()
        assert bool(((cls == 2) | (cls == 3)).all())
    with pytest.raises(gpu.LrtError):
        gpu.TemporalUpsampler(8, 8, 9, 8, dev)


def test_small_spheres_are_found_by_a_later_phase(gpu, scene):
    """What it is for. random_scene(1000, 1) at 38 x 26 from 19 x 13 under a static camera, eight steps
    cycling jitter_phases, color_low = palette[id_low + 1]: every pixel whose class was 0 or 2 in at
    least one step holds palette[id_cur + 1] within TOL, and there are more of them than lrt_upsample
    has class-0 pixels for the same frame (a sphere its low samples miss stays missed there)."""
    w, h, lw, lh = 38, 26, 19, 13
    spheres, mats = gpu.random_scene(1000, 1)
    scene(spheres, mats)
    cam = gpu.default_camera(w, h)
    palette = np.zeros((1001, 4), np.float32)
    palette[:, :3] = np.random.default_rng(11).uniform(0.05, 1.0, (1001, 3))
    phases = gpu.jitter_phases(w, lw, h, lh)
    spoke = np.zeros((h, w), bool)
    prev_g = prev = None
    for t in range(8):
        jit = phases[t % len(phases)]
        low = gpu.gbuffer_host(lw, lh, gpu.jitter_camera(cam, w, h, lw, lh, *jit), id=True)
        cur = gpu.gbuffer_host(w, h, cam, id=True, motion=True)
        assert (cur["motion"][..., :2] == 0).all()                      # a static camera: the history is never resampled
        s = dict(color_low=np.ascontiguousarray(palette[low["id"] + 1]), low=low, cur=cur, jitter=jit)
        prev, cls = _run(gpu, s, prev_g, prev)
        prev_g = {k: cur[k] for k in ("normal", "id")}
        spoke |= (cls == 0) | (cls == 2)
    want = palette[cur["id"] + 1][..., :3]
    gap = R.rel_gap(prev["color"][..., :3][spoke], want[spoke])
    low0 = gpu.gbuffer_host(lw, lh, cam, id=True)
    ucls = np.zeros((h, w), np.int32)
    gpu.upsample_host(np.ascontiguousarray(palette[low0["id"] + 1]), {k: low0[k] for k in ("id", "normal")},
                      {k: cur[k] for k in ("id", "normal")}, class_out=ucls)
    spatial = int((ucls == 0).sum())
    print(f"pixels whose own surface spoke in at least one of 8 steps: {int(spoke.sum())} of {w * h}; lrt_upsample's "
          f"class 0 for the same frame: {spatial} (DESIGN 7.8: {UPSAMPLE_CLASS0_1000}); gap {gap:.3g} (bound {TOL:.3g})")
    assert gap <= TOL
    assert spoke.sum() > spatial
