"""History rectification on the GPU (lrt_temporal_rectify_device / _host, rectify_kernel of
learnraytracing_amd/csrc/lrt_rectify.hip) against its NumPy restatement (tests/rectify_ref.py): the
library's own ids and pool-kernel colours at sizes that cross the 32 x 8 tile and its halo, sphere
counts on either side of the grid, each at radius 1, 2 and 3; the designed cases with their exact
expectations; the buffer contract; the TemporalAccumulator front end; and what it is for: a
noise-free change taken in one step, and a dimmed light followed faster than the plain history.

The house rule of tests/test_gpu_temporal_gbuffer.py: |got - f64| <= TOL * max(1, |f64|) at every
pixel none of whose decisions lies within 1e-4 of its threshold (the restatement's `fragile` mask),
TOL = 16 x the largest gap between the restatement's own f32 and f64 runs on the same cases
(`python tests/rectify_ref.py` measures it on the CPU; tests/test_rectify_cpu.py holds the
restatement to it and to the fragile share). The class planes are equal off the mask."""
import ctypes

import numpy as np
import pytest

import gbuffer_ref as G
import rectify_ref as Q
import temporal_gbuffer_ref as TG
import temporal_ref as R

pytestmark = pytest.mark.gpu

F32_F64_GAP = 4.2e-6                # measured: 4.13e-06 (rendered_gap()), color, moment2 and n
F32_F64_GAP_STD = 2.5e-5            # measured: 2.48e-05, color_std
TOL, TOL_STD = 16 * F32_F64_GAP, 16 * F32_F64_GAP_STD
F32_F64_GAP_DESIGNED = 2.2e-6       # measured: 2.15e-06 (designed_gap())
F32_F64_GAP_STD_DESIGNED = 5.5e-7   # measured: 5.37e-07
TOL_DESIGNED, TOL_STD_DESIGNED = 16 * F32_F64_GAP_DESIGNED, 16 * F32_F64_GAP_STD_DESIGNED
SENTINEL = 7.0
GUARD = 64
POOL = 512   # LRT_F_POOL
OUT = ("color", "moment2", "color_std")


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _spheres(L, arr):
    return [L.Sphere(L.f3(*s[:3]), float(s[3])) for s in G.sphere_array(arr)]


def _library(gpu):
    """(planes, colour) as rectify_ref.rendered_inputs takes them: the library's own G-buffer
    (gbuffer_host) and the pool kernel's colours. They set the scene: the caller restores it."""
    L = gpu._lib

    def planes(w, h, camera, spheres, mats, prev_camera, prev_spheres):
        gpu.set_scene(_spheres(L, spheres), mats)
        return gpu.gbuffer_host(w, h, camera, id=True)

    def colour(w, h, camera, spheres, mats, frame0, frames=1):
        gpu.set_scene(_spheres(L, spheres), mats)
        buf = np.zeros((h, w, 4), np.float32)
        gpu.render_host(gpu.Job(width=w, height=h, frame0=frame0, frames=frames, max_depth=8, camera=camera, flags=POOL),
                        buf)
        return buf

    return planes, colour


@pytest.fixture(scope="module")
def rendered(gpu):
    """{(w, h, count): (ref, ids, state)} of every rendered case, rendered once and left unchanged
    (the scene is set and restored here: a module fixture cannot use a function-scoped one)."""
    out = {}
    try:
        planes, colour = _library(gpu)
        for _, w, h, count in TG.case_list():
            out[(w, h, count)] = Q.rendered_inputs(w, h, count, TG.scene_of(gpu.default_scene, gpu.random_scene),
                                                   gpu.make_camera, planes, colour)
    finally:
        gpu.set_scene(*gpu.default_scene())
    return out


def _check(got, want, fragile, tol, tol_std, label):
    """The house rule over every output; returns the largest gap as a share of its bound."""
    worst, ok = 0.0, ~fragile
    gaps = {}
    for name in Q.OUTPUTS:
        t = tol_std if name == "color_std" else tol
        assert np.isfinite(got[name]).all(), name
        gaps[name] = R.rel_gap(got[name], want[name], ok)
        print(f"{label} {name}: gap {gaps[name]:.3g} (bound {t:.3g})")
        worst = max(worst, gaps[name] / t)
    for name in Q.OUTPUTS:
        t = tol_std if name == "color_std" else tol
        assert gaps[name] <= t, f"{label} {name}: {gaps[name]:.3g} > {t:.3g}"
    return worst


def _passthrough(got, state, mask):
    """color, moment2 and n came out as they went in, bit for bit, on mask."""
    return (np.array_equal(_bits(got["color"][mask]), _bits(state["color"][..., :3][mask]))
            and np.array_equal(_bits(got["moment2"][mask]), _bits(state["moment2"][..., :3][mask]))
            and np.array_equal(_bits(got["n"][mask]), _bits(state["moment2"][..., 3][mask])))


@pytest.mark.parametrize("label,w,h,count,rad", Q.case_list(), ids=[c[0].replace(" ", "") for c in Q.case_list()])
def test_call_vs_restatement(gpu, rendered, label, w, h, count, rad):
    """One fresh 1 spp frame as the reference of a random state, at sizes that cross the 32-wide and
    8-high tile, partial tiles and images smaller than the window; 1, 16, 17 and 1000 spheres at
    19 x 13. The restatement reads the same arrays the library was given."""
    ref, ids, state = rendered[(w, h, count)]
    cls = np.full((h, w), -1, np.int32)
    got = Q.outputs_of(gpu.temporal_rectify_host(ref, ids, state, class_out=cls, ref_scale=Q.CUR_SCALE, radius=rad))
    info = {}
    want, fragile = Q.step(ref, ids, state, np.float64, info=info, ref_scale=Q.CUR_SCALE, radius=rad)
    share = np.bincount(info["class"].ravel(), minlength=3) / (w * h)
    print(f"{label}: fragile {100 * fragile.mean():.2f} %, classes 0/1/2 {share}")
    assert fragile.mean() <= Q.MAX_FRAGILE
    if w * h <= 15:
        assert not fragile.any()
    worst = _check(got, want, fragile, TOL, TOL_STD, label)
    ok = ~fragile
    assert np.array_equal(cls[ok], info["class"][ok])
    assert _passthrough(got, state, ok & (info["class"] != 1))
    print(f"{label}: largest gap {worst:.3g} of its bound")


@pytest.mark.parametrize("case", Q.DESIGNED_CASES)
def test_designed_cases(gpu, case):
    """The designed cases (tests/test_rectify_cpu.py holds their branches on the restatement): every
    output against the f64 restatement, and the exact expectations on the library's own output --
    the class plane, the colours that sigma = 0 fixes bit for bit, the bit-for-bit passthrough of
    classes 0 and 2."""
    ref, ids, state, params, expect = Q.designed_inputs(case)
    h, w = ids.shape
    cls = np.full((h, w), -1, np.int32)
    got = Q.outputs_of(gpu.temporal_rectify_host(ref, ids, state, class_out=cls, **params))
    info = {}
    want, fragile = Q.step(ref, ids, state, np.float64, info=info, **params)
    assert not fragile.any()
    worst = _check(got, want, fragile, TOL_DESIGNED, TOL_STD_DESIGNED, case)
    assert np.array_equal(cls, info["class"])
    assert _passthrough(got, state, cls != 1)
    for name, (mask, *value) in expect.items():
        v = np.asarray(value[0]) if value else None
        if v is not None and v.shape[:2] == mask.shape:
            v = v[mask]
        if name == "class":
            assert np.array_equal(cls[mask], np.broadcast_to(v, cls[mask].shape))
        elif name == "color_is":
            assert np.array_equal(_bits(got["color"][mask]), _bits(np.broadcast_to(np.float32(v), got["color"][mask].shape)))
        elif name == "passthrough":
            assert _passthrough(got, state, mask)
        elif name == "n_near":
            assert (np.abs(got["n"][mask] - v) <= value[1]).all()
        elif name == "n_is":
            assert (got["n"][mask] == np.float32(v)).all()
        elif name == "short":
            std = got["color_std"][mask]
            assert np.array_equal((std == np.float32(1e3)).all(-1), np.broadcast_to(v, std.shape[:1]))
    print(f"{case}: largest gap {worst:.3g} of its bound")


@pytest.mark.parametrize("own_id", (False, True), ids=["another_id", "own_id"])
def test_nan_in_the_reference(gpu, own_id):
    """A NaN at a tap of another id gives the bits of the run with it zeroed; a NaN at a tap of the
    pixel's own id changes no pixel further than `radius` away."""
    ref, zeroed, ids, state = Q.nan_ref_inputs(own_id)
    ys, xs = np.mgrid[0:ids.shape[0], 0:ids.shape[1]]
    for rad in Q.RADII:
        a = gpu.temporal_rectify_host(ref, ids, state, radius=rad)
        b = gpu.temporal_rectify_host(zeroed, ids, state, radius=rad)
        far = np.maximum(np.abs(ys - Q.NAN_AT[0]), np.abs(xs - Q.NAN_AT[1])) > rad
        mask = far if own_id else np.ones_like(far)
        for name in OUT:
            assert np.array_equal(_bits(a[name][mask]), _bits(b[name][mask])), (name, rad)


@pytest.mark.parametrize("w,h", [(67, 45), (1, 1)], ids=["67x45", "1x1"])
def test_contract(gpu, rendered, w, h):
    """Host, device and tensor forms give the same bits; in place equals out of place; the alphas of
    color and color_std stay; 64 sentinel words behind every output stay; every input is unchanged
    when the call is not in place; color_std and class_out are optional and change nothing else."""
    import torch
    L = gpu._lib
    dev = torch.device("cuda:0")
    ref, ids, state = rendered[(w, h, 9)]
    kw = dict(ref_scale=Q.CUR_SCALE, radius=3 if w > 1 else 2)
    inputs = (ref, ids, state["color"], state["moment2"])
    keep = [a.copy() for a in inputs]
    hout = {n: np.full((h, w, 4), SENTINEL, np.float32) for n in OUT}
    hcls = np.full((h, w), -1, np.int32)
    assert gpu.temporal_rectify_host(ref, ids, state, out=hout, class_out=hcls, **kw) is hout
    for a, b in zip(inputs, keep):
        assert np.array_equal(_bits(a), _bits(b))
    assert (hout["color"][..., 3] == SENTINEL).all() and (hout["color_std"][..., 3] == SENTINEL).all()
    assert np.isfinite(hout["moment2"]).all() and ((hcls >= 0) & (hcls <= 2)).all()
    # color_std and class_out are optional and change nothing else
    nostd = gpu.temporal_rectify_host(ref, ids, state, out={n: np.zeros((h, w, 4), np.float32) for n in OUT[:2]}, **kw)
    assert set(nostd) == set(OUT[:2])
    assert np.array_equal(_bits(nostd["moment2"]), _bits(hout["moment2"]))
    assert np.array_equal(_bits(nostd["color"][..., :3]), _bits(hout["color"][..., :3]))
    # in place on the host: the same bits, the state's own alpha
    hin = {n: state[n].copy() for n in OUT[:2]}
    hin["color"][..., 3] = SENTINEL
    hin["color_std"] = np.full((h, w, 4), SENTINEL, np.float32)
    assert gpu.temporal_rectify_host(ref, ids, hin, out=hin, **kw) is hin
    for n in OUT:
        assert np.array_equal(_bits(hin[n][..., :3]), _bits(hout[n][..., :3])), n
    assert np.array_equal(_bits(hin["moment2"]), _bits(hout["moment2"]))
    assert (hin["color"][..., 3] == SENTINEL).all()
    # the tensor form: every output with a guard behind it, on a stream of its own
    tref, tids = torch.from_numpy(ref).to(dev), torch.from_numpy(ids).to(dev)
    tstate = {k: torch.from_numpy(v).to(dev) for k, v in state.items()}
    n4 = w * h * 4
    tout = {n: torch.full((n4 + GUARD,), SENTINEL, device=dev) for n in OUT}
    tcls = torch.full((w * h + GUARD,), -1, dtype=torch.int32, device=dev)
    st = torch.cuda.Stream(dev)
    st.wait_stream(torch.cuda.current_stream(dev))
    assert gpu.temporal_rectify_tensor(tref, tids, tstate, out=tout, class_out=tcls, stream=st, width=w, height=h,
                                       **kw) is tout
    st.synchronize()
    for n in OUT:
        t = tout[n].cpu().numpy()
        assert np.array_equal(_bits(t[:n4]), _bits(hout[n]).ravel()), n      # (the sentinel alphas included)
        assert (t[n4:] == SENTINEL).all(), f"{n}: guard"
    c = tcls.cpu().numpy()
    assert np.array_equal(c[:w * h], hcls.ravel()) and (c[w * h:] == -1).all()
    for t, a in zip((tref, tids, tstate["color"], tstate["moment2"]), keep):   # the inputs on the device
        assert np.array_equal(_bits(t.cpu().numpy()), _bits(a))
    # the device entry point itself, in place on a copy of the state, without color_std and class
    raw = {k: torch.cat([tstate[k].clone().ravel(), torch.full((GUARD,), SENTINEL, device=dev)]) for k in OUT[:2]}
    d = gpu.temporal_rectify_desc(w, h, **kw)
    ss = L.TemporalState()
    ss.color, ss.moment2 = raw["color"].data_ptr(), raw["moment2"].data_ptr()
    torch.cuda.synchronize()
    assert L.lib().lrt_temporal_rectify_device(ctypes.byref(d), tref.data_ptr(), tids.data_ptr(), ctypes.byref(ss),
                                               ctypes.byref(ss), None, None, None) == 0
    torch.cuda.synchronize()
    got = {k: raw[k].cpu().numpy() for k in raw}
    assert np.array_equal(_bits(got["moment2"][:n4]), _bits(hout["moment2"]).ravel())
    assert np.array_equal(_bits(got["color"][:n4].reshape(h, w, 4)[..., :3]), _bits(hout["color"][..., :3]))
    assert np.array_equal(_bits(got["color"][:n4].reshape(h, w, 4)[..., 3]), _bits(state["color"][..., 3]))
    assert (got["color"][n4:] == SENTINEL).all() and (got["moment2"][n4:] == SENTINEL).all()
    # in place on one buffer only, each independently
    for mine in OUT[:2]:
        other = OUT[1] if mine == OUT[0] else OUT[0]
        work = {mine: tstate[mine].clone(), other: tstate[other]}
        res = gpu.temporal_rectify_tensor(tref, tids, work, out={mine: work[mine], other: torch.zeros((h, w, 4), device=dev)},
                                          **kw)
        torch.cuda.synchronize()
        for n in OUT[:2]:
            assert np.array_equal(_bits(res[n].cpu().numpy()[..., :3]), _bits(hout[n][..., :3])), (mine, n)
        assert np.array_equal(_bits(tstate[other].cpu().numpy()), _bits(state[other]))
    # a refused call writes nothing
    for bad in (dict(out=dict(tout, color=tref)), dict(class_out=tids), dict(out=dict(tout, color=tstate["moment2"]))):
        a = dict(out=tout, class_out=tcls, width=w, height=h)
        a.update(bad)
        with pytest.raises(gpu.LrtError) as e:
            gpu.temporal_rectify_tensor(tref, tids, tstate, **a, **kw)
        assert e.value.code == L.LRT_E_INVALID
    torch.cuda.synchronize()
    for n in OUT:
        assert np.array_equal(_bits(tout[n].cpu().numpy()[:n4]), _bits(hout[n]).ravel()), n


def test_state_after_shutdown(gpu, rendered):
    """Without lrt_initialize(): LRT_E_STATE (tests/test_gpu_gbuffer.py shuts down and comes back the
    same way)."""
    L = gpu._lib
    ref, ids, state = rendered[(1, 1, 9)]
    gpu.ShutdownTest()
    try:
        with pytest.raises(gpu.LrtError) as e:
            gpu.temporal_rectify_host(ref, ids, state)
        assert e.value.code == L.LRT_E_STATE
    finally:
        gpu.InitializeTest()
    assert gpu.temporal_rectify_host(ref, ids, state)["moment2"][0, 0, 3] == state["moment2"][0, 0, 3]   # m = 1: class 2


def test_accumulator_front_end(gpu):
    """19 x 13, six steps: step_gbuffer(rectify={}) equals temporal_accumulate_gbuffer_tensor followed
    by temporal_rectify_tensor in place, bit for bit; rectify=None equals the plain tensor call; the
    rectify dict's parameters arrive; svgf_filter_tensor runs on the rectified state."""
    import torch
    L = gpu._lib
    w, h, steps = 19, 13, 6
    dev = torch.device("cuda:0")
    cam = gpu.default_camera(w, h)
    accs = {k: gpu.TemporalAccumulator(w, h, dev) for k in ("rect", "plain", "r1")}
    gen = torch.Generator(device=dev).manual_seed(5)
    chained = plain = chained1 = prev_g = None
    some_clamped = False
    for t in range(steps):
        k = float(t + 1)
        color = (torch.rand((h, w, 4), device=dev, generator=gen) + 0.05) / k
        planes = {}
        for name, acc in accs.items():
            planes[name] = gpu.gbuffer_tensor(w, h, cam, out=acc.gbuffer_planes())
        g = planes["rect"]
        col, guides = accs["rect"].step_gbuffer(color, g, cur_scale=k, rectify={}, min_history=2)
        accs["plain"].step_gbuffer(color, planes["plain"], cur_scale=k, rectify=None, min_history=2)
        accs["r1"].step_gbuffer(color, planes["r1"], cur_scale=k, rectify=dict(radius=1, gamma=0.5), min_history=2)
        pg = None if prev_g is None else {n: prev_g[n] for n in L.TEMPORAL_GBUFFER_PREV_NAMES}
        plain = gpu.temporal_accumulate_gbuffer_tensor(color, g, pg, plain, cur_scale=k, min_history=2)
        nxt = gpu.temporal_accumulate_gbuffer_tensor(color, g, pg, chained, cur_scale=k, min_history=2)
        cls = torch.full((h, w), -1, dtype=torch.int32, device=dev)
        chained = gpu.temporal_rectify_tensor(color, g["id"], nxt, out=nxt, class_out=cls, ref_scale=k, min_history=2)
        nxt1 = gpu.temporal_accumulate_gbuffer_tensor(color, g, pg, chained1, cur_scale=k, min_history=2)
        chained1 = gpu.temporal_rectify_tensor(color, g["id"], nxt1, out=nxt1, ref_scale=k, min_history=2, radius=1, gamma=0.5)
        prev_g = {n: g[n].clone() for n in L.TEMPORAL_GBUFFER_PREV_NAMES}
        torch.cuda.synchronize()
        some_clamped |= bool((cls == 1).any())
        for name, want in (("rect", chained), ("plain", plain), ("r1", chained1)):
            st = accs[name]._states[accs[name]._cur]
            for n in OUT:
                assert np.array_equal(_bits(st[n].cpu().numpy()[..., :3]), _bits(want[n].cpu().numpy()[..., :3])), (t, name, n)
            assert np.array_equal(_bits(st["moment2"].cpu().numpy()), _bits(want["moment2"].cpu().numpy())), (t, name)
        assert col is accs["rect"].state["color"] and guides["color_std"] is accs["rect"]._states[accs["rect"]._cur]["color_std"]
    assert some_clamped
    assert not torch.equal(accs["rect"].state["color"], accs["plain"].state["color"])
    assert not torch.equal(accs["rect"].state["color"], accs["r1"].state["color"])
    before = {n: accs["rect"].state[n].clone() for n in OUT[:2]}
    with pytest.raises(gpu.LrtError):                       # refused before the step runs
        accs["rect"].step_gbuffer(color, gpu.gbuffer_tensor(w, h, cam, out=accs["rect"].gbuffer_planes()),
                                  rectify=dict(alpha_min=0.5))
    st = accs["rect"].state
    torch.cuda.synchronize()
    assert all(torch.equal(st[n], before[n]) for n in before)
    out = gpu.svgf_filter_tensor(st["color"], st["moment2"], {n: g[n] for n in ("normal", "world_pos", "albedo")})
    torch.cuda.synchronize()
    assert out.shape == (h, w, 4) and torch.isfinite(out).all()


def test_noise_free_change_is_taken_in_one_step(gpu):
    """What it is for, derivable (tests/test_rectify_cpu.py holds the same sequence on the
    restatement): 40 frames of A, then frames of B, one id, zero motion. The plain history is still
    0.95 (B - A) away after one frame of B; rectified on the frame itself it is B, the bits of B
    since sigma = 0, and its n starts over at 1, 2, 3, ..."""
    cur, prev_g = Q.sequence_planes()
    plain = rect = None
    B = np.float32(Q.SEQ_B)
    for k in range(Q.SEQ_BEFORE + Q.SEQ_AFTER):
        frame = Q.sequence_frame(Q.SEQ_A if k < Q.SEQ_BEFORE else Q.SEQ_B)
        pg = prev_g if plain is not None else None
        plain = gpu.temporal_accumulate_gbuffer_host(frame, cur, pg, plain)
        rect = gpu.temporal_accumulate_gbuffer_host(frame, cur, pg, rect)
        rect = gpu.temporal_rectify_host(frame, cur["id"], rect, out=rect)
        j = k - Q.SEQ_BEFORE + 1
        if j >= 1:
            assert np.array_equal(_bits(rect["color"][..., :3]), _bits(np.full_like(rect["color"][..., :3], B))), j
            assert (np.abs(rect["moment2"][..., 3] - j) <= Q.N_TOL).all(), j
            err = np.abs(plain["color"][..., :3] - B).max() / abs(Q.SEQ_B - Q.SEQ_A)
            assert err == pytest.approx(0.95 ** j, abs=1e-5)      # (f32: 40 blends of 2^-24 each)


def test_dimmed_light_is_followed_faster(gpu):
    """What it is for, rendered. 67 x 45, the default scene, a static camera, the pool kernel at 1 spp
    with fresh seeds per step. Twelve steps; then the light's (sphere 8's) emissive x 0.25: ids and
    normals are unchanged, so the plain step keeps all its history. Both chains run four more steps.
    Truth is a 256 spp render of the dimmed scene: the rectified chain's mean |color - truth| is
    below the plain chain's at the first and at the fourth step after the change. (On the CPU, with
    the restatement and the oracle's colours: plain 0.476, 0.443, 0.414, 0.389, rectified 0.063,
    0.040, 0.035, 0.035 at the four steps)"""
    L = gpu._lib
    D = Q.DIM
    w, h = D["w"], D["h"]
    spheres, mats = gpu.default_scene()
    dim = [L.Material.from_buffer_copy(m) for m in mats]
    e = dim[D["light"]].emissive
    assert max(e.x, e.y, e.z) > 1
    dim[D["light"]].emissive = L.f3(e.x * D["factor"], e.y * D["factor"], e.z * D["factor"])
    cam, _ = G.camera_pair(gpu.make_camera, w, h)
    planes_of, colour = _library(gpu)
    sph = G.sphere_array(spheres)
    try:
        cur = gpu.gbuffer_host(w, h, cam, cam, id=True, motion=True)
        prev_g = {n: cur[n].copy() for n in ("normal", "id")}
        gpu.set_scene(spheres, dim)
        after = gpu.gbuffer_host(w, h, cam, cam, id=True, motion=True)
        assert np.array_equal(after["id"], cur["id"]) and np.array_equal(_bits(after["normal"]), _bits(cur["normal"]))

        def render(t, dimmed):
            return colour(w, h, cam, sph, dim if dimmed else mats, t)

        def accumulate(frame, state, k):
            return gpu.temporal_accumulate_gbuffer_host(frame, cur, prev_g if state is not None else None, state, cur_scale=k)

        def rectify(frame, state, k):
            return gpu.temporal_rectify_host(frame, cur["id"], state, out=state, ref_scale=k)

        chain = Q.dimmed_chain(render, cur["id"], accumulate, rectify)
        truth = colour(w, h, cam, sph, dim, 0, D["truth_spp"])[..., :3]
        truth_before = colour(w, h, cam, sph, mats, 0, D["truth_spp"])[..., :3]
    finally:
        gpu.set_scene(*gpu.default_scene())
    p, r = (np.abs(c - truth_before).mean() for c in chain[D["steps"] - 1])
    print(f"step {D['steps'] - 1}, nothing changed yet: plain {p:.4f}, rectified {r:.4f}")
    errs = []
    for i in range(D["after"]):
        p, r = (np.abs(c - truth).mean() for c in chain[D["steps"] + i])
        print(f"step {i + 1} after the change: plain {p:.4f}, rectified {r:.4f}")
        errs.append((p, r))
    assert errs[0][1] < errs[0][0]
    assert errs[3][1] < errs[3][0]
