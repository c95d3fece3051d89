"""Temporal accumulation driven by the G-buffer on the GPU (lrt_temporal_accumulate_gbuffer_device /
_host, temporal_gbuffer_kernel of learnraytracing_amd/csrc/lrt_temporal_gbuffer.hip) against its
NumPy restatement (tests/temporal_gbuffer_ref.py): the library's own G-buffer planes and pool-kernel
colours of the default scene one orbit step on with moved spheres, sphere counts on either side of
the grid, the designed cases, the buffer contract, the TemporalAccumulator front end, and what it is
for: a static accumulation that is exact and a translated sphere that keeps its history.

The house rule of tests/test_gpu_temporal.py: |got - f64| <= TOL * max(1, |f64|) at every pixel none
of whose decisions lies within 1e-4 of its threshold (the restatement's `fragile` mask), TOL = 16 x
the largest gap between the restatement's own f32 and f64 runs on the same cases
(`python tests/temporal_gbuffer_ref.py` measures it on the CPU; tests/test_temporal_gbuffer_cpu.py
holds the restatement to it and to the fragile share). n is exact where fx and fy are whole numbers."""
import ctypes

import numpy as np
import pytest

import gbuffer_ref as G
import temporal_gbuffer_ref as T
import temporal_motion_ref as M
import temporal_ref as R

pytestmark = pytest.mark.gpu

F32_F64_GAP = 2.6e-7                # measured: 2.52e-07 (rendered_gap()), color, moment2 and n
F32_F64_GAP_STD = 8e-7              # measured: 7.87e-07, color_std
TOL, TOL_STD = 16 * F32_F64_GAP, 16 * F32_F64_GAP_STD
F32_F64_GAP_DESIGNED = 1.8e-7       # measured: 1.69e-07 (designed_gap())
F32_F64_GAP_STD_DESIGNED = 9e-7     # measured: 8.62e-07
TOL_DESIGNED, TOL_STD_DESIGNED = 16 * F32_F64_GAP_DESIGNED, 16 * F32_F64_GAP_STD_DESIGNED
SENTINEL = 7.0
GUARD = 64
POOL = 512   # LRT_F_POOL
OUT = ("color", "moment2", "color_std")


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
    """(planes, colour) as temporal_gbuffer_ref.rendered_case takes them: the library's own G-buffer
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


def _check(got, want, fragile, tol, tol_std, label):
    """The house rule over every output; returns the largest gap as a share of its bound."""
    worst, ok = 0.0, ~fragile
    for name in T.OUTPUTS:
        t = tol_std if name == "color_std" else tol
        assert np.isfinite(got[name]).all(), name
        gap = R.rel_gap(got[name], want[name], ok)
        print(f"{label} {name}: gap {gap:.3g} (bound {t:.3g})")
        worst = max(worst, gap / t)
    for name in T.OUTPUTS:
        t = tol_std if name == "color_std" else tol
        gap = R.rel_gap(got[name], want[name], ok)
        assert gap <= t, f"{label} {name}: {gap:.3g} > {t:.3g}"
    return worst


def _whole_motion(cur, prev):
    """The pixels whose fx and fy are whole numbers (one tap of weight 1: n = n' + 1 exactly)."""
    mv = cur["motion"]
    return (mv[..., 3] != 0) & (mv[..., 0] == np.floor(mv[..., 0])) & (mv[..., 1] == np.floor(mv[..., 1])) \
        if prev is not None else np.zeros(mv.shape[:2], bool)


@pytest.mark.parametrize("label,w,h,count", T.case_list(), ids=[c[0].replace(" ", "") for c in T.case_list()])
def test_step_vs_restatement(gpu, scene, label, w, h, count):
    """The default scene one orbit step on with spheres 2 and 3 moved and sphere 8 resized, at sizes
    that cross the 32-wide block, the 8-high wave and partial blocks; 1, 16, 17 and 1000 spheres at
    19 x 13. The restatement reads the same arrays the library was given."""
    planes, colour = _library(gpu, scene)
    args = T.rendered_case(w, h, count, T.scene_of(gpu.default_scene, gpu.random_scene), gpu.make_camera, planes, colour)
    color, cur, prev_g, prev = args
    got = _outputs(gpu.temporal_accumulate_gbuffer_host(color, cur, prev_g, prev, cur_scale=T.CUR_SCALE))
    info = {}
    want, fragile = T.step(*args, np.float64, info=info, cur_scale=T.CUR_SCALE)
    print(f"{label}: fragile {100 * fragile.mean():.2f} %, kept {int(info['keep'].sum())} of {w * h}, taps refused by id "
          f"{int(info['rej_id'].sum())}, by normal {int(info['rej_normal'].sum())}")
    assert fragile.mean() <= T.MAX_FRAGILE
    if w * h <= 15:
        assert not fragile.any()
    worst = _check(got, want, fragile, TOL, TOL_STD, label)
    whole = _whole_motion(cur, prev) & ~fragile
    assert np.array_equal(got["n"][whole], np.float32(want["n"][whole]))
    reset = ~info["keep"] & ~fragile
    assert (got["n"][reset] == 1).all()
    print(f"{label}: largest gap {worst:.3g} of its bound")


@pytest.mark.parametrize("case", T.DESIGNED_CASES)
def test_step_designed_cases(gpu, case):
    """The designed cases (tests/test_temporal_gbuffer_cpu.py holds their branches): every output
    against the f64 restatement, n = 1 exactly wherever the decision is to reset, n = n' + 1 exactly
    under one tap of weight 1."""
    color, cur, prev_g, prev, params, expect = T.designed_inputs(case)
    got = _outputs(gpu.temporal_accumulate_gbuffer_host(color, cur, prev_g, prev, **params))
    info = {}
    want, fragile = T.step(color, cur, prev_g, prev, np.float64, info=info, **params)
    assert fragile.mean() <= T.MAX_FRAGILE
    worst = _check(got, want, fragile, TOL_DESIGNED, TOL_STD_DESIGNED, case)
    if prev is not None:
        assert (got["n"][~info["keep"]] == 1).all()
    for name, (mask, value) in expect.items():
        if name == "n_is_1":
            assert (got["n"][mask] == 1).all()
            assert np.array_equal(_bits(got["color"][mask]), _bits(color[..., :3][mask]))
        elif name == "n_prev":
            assert np.array_equal(got["n"][mask], np.float32(value) + np.float32(1))
        elif name == "keep":
            value = np.asarray(value)
            assert np.array_equal(got["n"][mask] > 1, np.broadcast_to(value[mask] if value.shape == mask.shape else value,
                                                                      got["n"][mask].shape))
    print(f"{case}: largest gap {worst:.3g} of its bound")


@pytest.fixture(scope="module")
def one_step(gpu):
    """{(w, h): the inputs of one rendered step}: 67 x 45 and 1 x 1, rendered once (the scene is set
    and restored here: a module fixture cannot use `scene`)."""
    out = {}
    try:
        planes, colour = _library(gpu, gpu.set_scene)
        for w, h in ((67, 45), (1, 1)):
            out[(w, h)] = T.rendered_case(w, h, 9, T.scene_of(gpu.default_scene, gpu.random_scene), gpu.make_camera,
                                          planes, colour)
    finally:
        gpu.set_scene(*gpu.default_scene())
    return out


@pytest.mark.parametrize("w,h", [(67, 45), (1, 1)], ids=["67x45", "1x1"])
def test_contract(gpu, one_step, w, h):
    """Host, device and tensor forms give the same bits; of d_next only color's rgb and moment2 are
    written (normal, world_pos, albedo and the alphas of color and color_std stay); 64 sentinel words
    behind every output stay; every input is unchanged; without history everything is reset."""
    import torch
    L = gpu._lib
    dev = torch.device("cuda:0")
    color, cur, prev_g, prev = one_step[(w, h)]
    kw = dict(cur_scale=T.CUR_SCALE)
    inputs = (color, *cur.values(), *prev_g.values(), *prev.values())
    keep = [a.copy() for a in inputs]
    hout = {n: np.full((h, w, 4), SENTINEL, np.float32) for n in OUT}
    assert gpu.temporal_accumulate_gbuffer_host(color, cur, prev_g, prev, out=hout, **kw) is hout
    for a, b in zip(inputs, keep):
        assert np.array_equal(_bits(a), _bits(b))
    assert (hout["color"][..., 3] == SENTINEL).all() and (hout["color_std"][..., 3] == SENTINEL).all()
    assert np.isfinite(hout["moment2"]).all() and (hout["moment2"][..., 3] >= 1).all()
    # color_std is optional and changes nothing else; a fresh call gives the same bits
    again = gpu.temporal_accumulate_gbuffer_host(color, cur, prev_g, prev, **kw)
    nostd = gpu.temporal_accumulate_gbuffer_host(color, cur, prev_g, prev, out={n: np.zeros((h, w, 4), np.float32)
                                                                                   for n in OUT[:2]}, **kw)
    for n in OUT:
        assert np.array_equal(_bits(again[n][..., :3]), _bits(hout[n][..., :3])), n
    assert set(nostd) == set(OUT[:2])
    assert np.array_equal(_bits(nostd["moment2"]), _bits(hout["moment2"]))
    assert np.array_equal(_bits(nostd["color"][..., :3]), _bits(hout["color"][..., :3]))
    # without a previous state everything is reset
    first = gpu.temporal_accumulate_gbuffer_host(color, cur, None, None, **kw)
    C = np.float32(T.CUR_SCALE) * color[..., :3]
    assert (first["moment2"][..., 3] == 1).all() and np.array_equal(_bits(first["color"][..., :3]), _bits(C))
    assert (first["color_std"][..., :3] == np.float32(1e3)).all()
    # the tensor form: every output with a guard behind it, on a stream of its own
    up = lambda d: {k: torch.from_numpy(v).to(dev) for k, v in d.items()}   # noqa: E731
    tcolor, tcur, tprev_g, tprev = torch.from_numpy(color).to(dev), up(cur), up(prev_g), up(prev)
    n4 = w * h * 4
    tout = {n: torch.full((n4 + GUARD,), SENTINEL, device=dev) for n in OUT}
    st = torch.cuda.Stream(dev)
    st.wait_stream(torch.cuda.current_stream(dev))
    assert gpu.temporal_accumulate_gbuffer_tensor(tcolor, tcur, tprev_g, tprev, out=tout, stream=st, width=w, height=h,
                                                  **kw) is tout
    st.synchronize()
    for n in OUT:
        t = tout[n].cpu().numpy()
        assert np.array_equal(_bits(t[:n4]), _bits(hout[n]).ravel()), n      # (the sentinel alphas included)
        assert (t[n4:] == SENTINEL).all(), f"{n}: guard"
    # the device entry point itself: the other members of d_next are never touched
    other = {n: torch.full((n4 + GUARD,), SENTINEL, device=dev) for n in ("normal", "world_pos", "albedo")}
    raw = {n: torch.full((n4 + GUARD,), SENTINEL, device=dev) for n in OUT}
    d = gpu.temporal_gbuffer_desc(w, h, **kw)
    gc, gp, ps, ns = L.Gbuffer(), L.Gbuffer(), L.TemporalState(), L.TemporalState()
    for k in L.TEMPORAL_GBUFFER_CUR_NAMES:
        setattr(gc, k, tcur[k].data_ptr())
    for k in L.TEMPORAL_GBUFFER_PREV_NAMES:
        setattr(gp, k, tprev_g[k].data_ptr())
    ps.color, ps.moment2 = tprev["color"].data_ptr(), tprev["moment2"].data_ptr()
    ns.color, ns.moment2 = raw["color"].data_ptr(), raw["moment2"].data_ptr()
    ns.normal, ns.world_pos, ns.albedo = (other[k].data_ptr() for k in ("normal", "world_pos", "albedo"))
    torch.cuda.synchronize()
    assert L.lib().lrt_temporal_accumulate_gbuffer_device(ctypes.byref(d), tcolor.data_ptr(), ctypes.byref(gc),
                                                          ctypes.byref(gp), ctypes.byref(ps), ctypes.byref(ns),
                                                          raw["color_std"].data_ptr(), None) == 0
    torch.cuda.synchronize()
    for n in OUT:
        assert np.array_equal(_bits(raw[n].cpu().numpy()), _bits(tout[n].cpu().numpy())), n
    for n, t in other.items():
        assert (t.cpu().numpy() == SENTINEL).all(), n
    for t, a in zip((tcolor, *tcur.values(), *tprev_g.values(), *tprev.values()), keep):   # the inputs on the device
        assert np.array_equal(_bits(t.cpu().numpy()), _bits(a))
    # a refused call writes nothing: an output on an input, exactly one of prev and prev_g
    for bad in (dict(out=dict(tout, color=tcolor)), dict(prev=None), dict(prev_g=None),
                dict(prev_g=dict(tprev_g, id=tcur["id"]))):
        a = dict(cur=tcur, prev_g=tprev_g, prev=tprev, out=tout, width=w, height=h)
        a.update(bad)
        with pytest.raises(gpu.LrtError) as e:
            gpu.temporal_accumulate_gbuffer_tensor(tcolor, a.pop("cur"), a.pop("prev_g"), a.pop("prev"), **a, **kw)
        assert e.value.code == L.LRT_E_INVALID
    torch.cuda.synchronize()
    for n in OUT:
        assert np.array_equal(_bits(tout[n].cpu().numpy()), _bits(raw[n].cpu().numpy())), n


def test_state_after_shutdown(gpu, one_step):
    """Without lrt_initialize(): LRT_E_STATE (tests/test_gpu_gbuffer.py shuts down and comes back the
    same way)."""
    L = gpu._lib
    color, cur, prev_g, prev = one_step[(1, 1)]
    gpu.ShutdownTest()
    try:
        with pytest.raises(gpu.LrtError) as e:
            gpu.temporal_accumulate_gbuffer_host(color, cur, prev_g, prev)
        assert e.value.code == L.LRT_E_STATE
    finally:
        gpu.InitializeTest()
    assert gpu.temporal_accumulate_gbuffer_host(color, cur, prev_g, prev)["moment2"][0, 0, 3] >= 1


def test_accumulator_front_end(gpu):
    """19 x 13: gbuffer_planes() hands out its two sets in turn, step_gbuffer() equals the plain
    tensor call, refuses the tensors it holds as history, and drops the history on reset() and when
    step() comes in between."""
    import torch
    L = gpu._lib
    w, h = 19, 13
    dev = torch.device("cuda:0")
    cam = gpu.default_camera(w, h)
    acc = gpu.TemporalAccumulator(w, h, dev)
    color = torch.rand((h, w, 4), device=dev) + 0.05

    def fill():
        planes = acc.gbuffer_planes()
        assert set(planes) == set(L.TEMPORAL_GBUFFER_PLANES) and planes["id"].dtype == torch.int32
        assert gpu.gbuffer_tensor(w, h, cam, out=planes) is planes
        return planes

    p0 = fill()
    assert acc.gbuffer_planes()["normal"] is p0["normal"]           # not held yet: the same set again
    col, guides = acc.step_gbuffer(color, p0, cur_scale=2.0)
    assert set(guides) == {"color_std"} and col is acc.state["color"]
    torch.cuda.synchronize()
    assert (acc.state["moment2"][..., 3] == 1).all()
    first = {k: acc.state[k].clone() for k in ("color", "moment2")}
    with pytest.raises(gpu.LrtError) as e:
        acc.step_gbuffer(color, p0)
    assert e.value.code == L.LRT_E_INVALID
    with pytest.raises(gpu.LrtError) as e:                            # another dict of the same tensors
        acc.step_gbuffer(color, dict(p0))
    assert e.value.code == L.LRT_E_INVALID
    p1 = fill()
    assert p1["normal"] is not p0["normal"] and p1["id"] is not p0["id"]
    col, guides = acc.step_gbuffer(color, p1, cur_scale=2.0, min_history=2)
    want = gpu.temporal_accumulate_gbuffer_tensor(color, p1, p0, first, cur_scale=2.0, min_history=2)
    torch.cuda.synchronize()
    assert (acc.state["moment2"][..., 3] == 2).all()                  # a static camera: exactly
    for k, t in (("color", col), ("moment2", acc.state["moment2"]), ("color_std", guides["color_std"])):
        assert np.array_equal(_bits(t.cpu().numpy()[..., :3]), _bits(want[k].cpu().numpy()[..., :3])), k
    assert acc.gbuffer_planes()["normal"] is p0["normal"]             # the set that is not the history
    acc.reset()
    acc.step_gbuffer(color, fill())
    torch.cuda.synchronize()
    assert (acc.state["moment2"][..., 3] == 1).all()
    p = fill()
    acc.step_gbuffer(color, p)
    acc.step(color, {k: p[k] for k in ("normal", "world_pos", "albedo")}, cam)     # the other form: its own history
    torch.cuda.synchronize()
    assert (acc.state["moment2"][..., 3] == 1).all()
    acc.step_gbuffer(color, fill())
    torch.cuda.synchronize()
    assert (acc.state["moment2"][..., 3] == 1).all()
    with pytest.raises(gpu.LrtError):
        acc.step_gbuffer(color, {"normal": p["normal"], "id": p["id"]})


def test_pool_colour_accumulates_through_the_gbuffer(gpu, scene):
    """What it is for. 67 x 45, a static camera, fresh seeds: step t renders sample frame0 = t with
    the pool kernel, cur_scale = t + 1, and goes through step_gbuffer with planes from
    gbuffer_planes(): after 8 steps n == 8 exactly at every pixel (a zero motion makes it exact).
    Then sphere MOVING_ID comes down a step at a time: its interior pixels keep n > 1 at every
    step, and a TemporalAccumulator fed step(spheres=, motion=) on the same frames keeps n > 1
    wherever this one does. Last, svgf_filter_tensor runs on the new state with the G-buffer's planes
    as guides."""
    import torch
    L = gpu._lib
    w, h, steps, moving = 67, 45, 8, 4
    dev = torch.device("cuda:0")
    cam = gpu.default_camera(w, h)
    spheres, mats = gpu.default_scene()
    base = G.sphere_array(spheres)
    acc, old = gpu.TemporalAccumulator(w, h, dev), gpu.TemporalAccumulator(w, h, dev)
    rays = torch.zeros(1, dtype=torch.int64, device=dev)
    motion = torch.zeros((h, w, 4), device=dev)

    def frame(t, sph, before):
        scene(_spheres(L, sph), mats)
        buf = torch.zeros((h, w, 4), device=dev)
        gpu.render_tensor(gpu.Job(width=w, height=h, frame0=t, frames=1, max_depth=8, camera=cam, flags=POOL), buf, rays)
        assert L.last_launch()["kernel"] == "pool_kernel"
        k = float(t + 1)
        planes = gpu.gbuffer_tensor(w, h, cam, prev_spheres=before, out=acc.gbuffer_planes())
        acc.step_gbuffer(buf, planes, cur_scale=k)
        guides = gpu.gbuffer_tensor(w, h, cam, guide_scale=1.0 / k)
        old.step(buf, guides, cam, cur_scale=k, spheres=sph, motion=motion)
        return planes

    first = base.copy()
    first[M.MOVING_ID, :3] -= np.float32(M.MOVING_STEP) * np.float32(moving)
    for t in range(steps):
        frame(t, first, None)
    torch.cuda.synchronize()
    n = acc.state["moment2"][..., 3].cpu().numpy()
    assert (n == steps).all(), f"n == {steps} on {100 * (n == steps).mean():.2f} % of the pixels"
    before = first
    for i in range(1, moving + 1):
        sph = base.copy()
        sph[M.MOVING_ID, :3] -= np.float32(M.MOVING_STEP) * np.float32(moving - i)
        planes = frame(steps - 1 + i, sph, before)
        before = sph
        torch.cuda.synchronize()
        on = planes["id"].cpu().numpy() == M.MOVING_ID
        inner = on.copy()                       # the pixels whose eight neighbours show the sphere too
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                inner &= np.roll(np.roll(on, dy, 0), dx, 1)
        inner[[0, -1], :] = inner[:, [0, -1]] = False
        n = acc.state["moment2"][..., 3].cpu().numpy()
        n_old = old.state["moment2"][..., 3].cpu().numpy()
        mv = planes["motion"].cpu().numpy()
        print(f"moving step {i}: sphere {M.MOVING_ID} on {int(on.sum())} px, interior {int(inner.sum())}, least n there "
              f"{n[inner].min() if inner.any() else 0:.3g} (step(spheres=): {n_old[inner].min() if inner.any() else 0:.3g})")
        assert inner.sum() >= 10
        assert (np.abs(mv[..., 1][inner]) > 1).all() and (mv[..., 3][inner] == 1).all()
        assert (n[inner] > 1).all()
        assert (n_old[inner & (n > 1)] > 1).all()
    st = acc.state
    guides = {k: planes[k] for k in ("normal", "world_pos", "albedo")}
    out = gpu.svgf_filter_tensor(st["color"], st["moment2"], guides)
    torch.cuda.synchronize()
    assert out.shape == (h, w, 4) and torch.isfinite(out).all()
    assert not torch.equal(out[..., :3], st["color"][..., :3])
