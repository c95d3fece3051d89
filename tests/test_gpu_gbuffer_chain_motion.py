"""The chain motion pass on the GPU (lrt_gbuffer_chain_motion_device / _host, the two kernels of
learnraytracing_amd/csrc/lrt_gbuffer_chain_motion.hip).

Pinned: status equals the f32 restatement of tests/gbuffer_chain_motion_ref.py at every pixel and the
f64 one off its `fragile` mask; motion.zw, and every quad outside LRT_CM_CONVERGED, are first_motion's
bits.

The house rule of tests/test_gpu_gbuffer.py for motion.xy, in pixels: |got - f64| <= TOL at every
converged pixel off the mask, TOL = 16 x the largest gap between the restatement's own f32 and f64 runs
on the same cases (`python tests/gbuffer_chain_motion_ref.py` measures it on the CPU;
tests/test_gbuffer_chain_motion_cpu.py holds the restatement to it)."""
import numpy as np
import pytest

import gbuffer_chain_motion_ref as M
import gbuffer_chain_ref as C
import gbuffer_ref as G
import temporal_gbuffer_ref as TG
import temporal_ref as R

pytestmark = pytest.mark.gpu

F32_F64_GAP = {(1, 1): 0.0, (19, 13): 1.7e-5, (67, 45): 8.0e-5}   # px; measured: 0 (nothing followed), 1.61e-05, 7.81e-05
F32_F64_GAP_FLAT = 1.3e-5                        # measured: 1.20e-05
F32_F64_GAP_GRID17 = 8.0e-5                      # measured: 6.92e-05 (the default scene's pixels at 67 x 45, through the grid)
F32_F64_GAP_TEMPORAL = 2.6e-7                    # tests/test_gpu_temporal_gbuffer.py's, color, moment2 and n
MAX_FRAGILE = 0.05                               # of the followed pixels
SENTINEL = 7.0


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.fixture
def scene(gpu):
    """set(spheres, materials); the default scene is back afterwards."""
    try:
        yield gpu.set_scene
    finally:
        gpu.set_scene(*gpu.default_scene())


def _run(gpu, kw, **extra):
    """The library on a restatement case (it holds kw's scene), fed the restatement's own first_motion."""
    params = {k: kw[k] for k in M.DEFAULTS if k in kw}
    return gpu.gbuffer_chain_motion_host(kw["w"], kw["h"], kw["camera"], kw["prev_camera"], kw["first_motion"],
                                         prev_spheres=kw["prev_spheres"], **params, **extra)


def _check_case(gpu, kw, gap, label):
    got = _run(gpu, kw)
    f32, want, fragile = M.pair(kw)
    first = kw["first_motion"]
    differ = got["status"] != f32["status"]
    hist = np.bincount(got["status"].ravel(), minlength=6).tolist()
    print(f"{label}: status {dict(zip(M.STATUS_NAMES, hist))}, differs from the f32 restatement at {int(differ.sum())} px")
    assert not differ.any(), f"{label}: status against the f32 restatement"
    fol = M.followed(f32)
    share = (fragile & fol).sum() / max(1, fol.sum())
    assert share <= MAX_FRAGILE
    ok = ~fragile
    assert np.array_equal(got["status"][ok], want["status"][ok]), f"{label}: f64 status off the mask"
    conv = got["status"] == M.CONVERGED
    assert np.array_equal(_bits(got["motion"])[~conv], _bits(first)[~conv]), f"{label}: copied quads"
    assert np.array_equal(_bits(got["motion"][..., 2]), _bits(first[..., 2])), f"{label}: motion.z"
    assert (got["motion"][..., 3][conv] == 1).all()
    on = conv & ok & (want["status"] == M.CONVERGED)
    tol = 16 * gap
    err = float(np.abs(got["motion"][..., :2].astype(np.float64) - want["motion"][..., :2])[on].max()) if on.any() else 0.0
    err32 = float(np.abs(got["motion"][..., :2] - f32["motion"][..., :2])[conv].max()) if conv.any() else 0.0
    print(f"{label}: fragile {100 * share:.2f} % of {int(fol.sum())} followed, motion gap to f64 {err:.3g} px "
          f"(bound {tol:.3g}), to the f32 restatement {err32:.3g} px")
    assert err <= tol, f"{label}: {err:.3g} > {tol:.3g}"
    return got


@pytest.mark.parametrize("how", M.MOTIONS)
@pytest.mark.parametrize("w,h", [(1, 1), (19, 13), (67, 45)], ids=["1x1", "19x13", "67x45"])
def test_default_scene(gpu, w, h, how):
    """The default scene (the scan instance): one orbit step, moved spheres, both."""
    kw = M.motion_case(w, h, how, gpu.default_scene, gpu.make_camera)
    got = _check_case(gpu, kw, F32_F64_GAP[(w, h)], f"{w}x{h} {how}")
    if (w, h) == (67, 45):
        conv = got["status"] == M.CONVERGED
        assert conv.sum() >= 400 and (got["status"] == M.KEY_LOST).sum() >= 20
        assert np.abs((got["motion"] - kw["first_motion"])[..., :2][conv]).max() > 0.05   # the search moved something


@pytest.mark.parametrize("count", M.COUNTS)
def test_grid_counts(gpu, scene, count):
    """17 spheres and random_scene(1000, 1) at 19 x 13 through the uniform grid, the orbit alone."""
    cases = dict(M.count_cases(gpu.default_scene, gpu.random_scene, gpu.make_camera))
    kw = cases[f"count {count}"]
    spheres, mats = G.count_scene(count, gpu.default_scene, gpu.random_scene)
    assert len(spheres) == count > G.GRID_ABOVE
    scene(spheres, mats)
    _check_case(gpu, kw, F32_F64_GAP[(19, 13)], f"count {count}")


def test_grid_with_mirrors(gpu, scene):
    """The grid instance with something to find (at 19 x 13 the two scenes above show next to no followed
    pixel that keeps its key): the default scene plus eight spheres out of sight, 17 in all, at 67 x 45."""
    L = gpu._lib
    w, h = 67, 45
    spheres, mats = gpu.default_scene()
    spheres = list(spheres) + [L.Sphere(L.f3(40.0 + 2 * i, 0.0, -60.0), 0.5) for i in range(8)]
    mats = list(mats) + [L.Material(L.LAMBERT, L.f3(0.5, 0.5, 0.5), L.f3(0, 0, 0), 0.0, 0.0) for _ in range(8)]
    scene(spheres, mats)
    cam, pcam = G.camera_pair(gpu.make_camera, w, h)
    kw = M.make_case(w, h, cam, pcam, spheres, mats)
    got = _check_case(gpu, kw, F32_F64_GAP_GRID17, "default + 8, the grid")
    assert (got["status"] == M.CONVERGED).sum() >= 400


def test_static_identity(gpu):
    """Bit-identical cameras and an unmoved scene: motion is first_motion in all bits at all pixels, fed
    the library's own first-hit motion, with and without a scene."""
    w, h = 67, 45
    cam = G.camera_pair(gpu.make_camera, w, h)[0]
    spheres = G.sphere_array(gpu.default_scene()[0])
    for prev_s in (None, spheres):
        g = gpu.gbuffer_host(w, h, cam, cam, motion=True, prev_spheres=prev_s)
        got = gpu.gbuffer_chain_motion_host(w, h, cam, cam, g["motion"], prev_spheres=prev_s)
        assert np.array_equal(_bits(got["motion"]), _bits(g["motion"]))
        assert (got["status"] == M.CONVERGED).sum() >= 400
        assert np.isin(got["status"], (M.NOT_FOLLOWED, M.CONVERGED, M.KEY_LOST)).all()
    zero = gpu.gbuffer_chain_motion_host(w, h, cam, G.camera_pair(gpu.make_camera, w, h)[1], g["motion"], max_bounces=0)
    assert np.isin(zero["status"], (M.NOT_FOLLOWED, M.UNRESOLVED)).all()
    assert np.array_equal(_bits(zero["motion"]), _bits(g["motion"]))


def test_flat_and_the_temporal_step(gpu, scene):
    """The designed case "flat" through the library, then what the plane is for: two steps of
    temporal_accumulate_gbuffer_host with the chain's keys as ids, once with lrt_gbuffer_*'s motion and
    once with this pass's. The mean error against the current colour drops at least tenfold, and the
    step's outputs follow temporal_gbuffer_ref fed the same planes."""
    kw = M.flat_case(gpu.make_camera)
    w, h = kw["w"], kw["h"]
    scene(*C.library_scene(gpu._lib, kw))
    got = _check_case(gpu, kw, F32_F64_GAP_FLAT, "flat")
    conv = got["status"] == M.CONVERGED
    assert abs(int(M.followed(got).sum()) - 777) <= 8 and abs(int(conv.sum()) - 736) <= 15
    cam, pcam = M.flat_cameras(gpu.make_camera)
    first = gpu.gbuffer_host(w, h, cam, pcam, motion=True)["motion"]
    cm = gpu.gbuffer_chain_motion_host(w, h, cam, pcam, first)
    assert np.array_equal(cm["status"] == M.CONVERGED, conv)
    worst = [0.0]

    def step(color, cur, prev_g, prev):
        s = gpu.temporal_accumulate_gbuffer_host(color, cur, prev_g, prev)
        want, fragile = TG.step(color, cur, prev_g, prev)
        for name in ("color", "moment2"):
            worst[0] = max(worst[0], R.rel_gap(s[name][..., :3], want[name], ~fragile))
        worst[0] = max(worst[0], R.rel_gap(s["moment2"][..., 3], want["n"], ~fragile))
        if prev is None:
            return {"color": s["color"], "moment2": s["moment2"]}, None
        return s["color"], s["moment2"][..., 3] != 1

    errs, keeps = M.flat_temporal_ratio(gpu.make_camera, step, (first, cm["motion"]))
    on = conv & keeps[0] & keeps[1]
    ratio = errs[1][on].mean() / errs[0][on].mean()
    print(f"flat: {int(on.sum())} px, mean error first-hit {errs[0][on].mean():.3g}, new {errs[1][on].mean():.3g}, "
          f"ratio {ratio:.3g}; temporal step against its restatement {worst[0]:.3g}")
    assert on.sum() >= 600
    assert ratio <= 0.1
    assert worst[0] <= 16 * F32_F64_GAP_TEMPORAL


def test_flat_moved_branches(gpu, scene):
    """LRT_CM_NO_SEED (a sphere that did not exist, w = 0, a NaN and 2e6 px in first_motion) and the
    carry-back of a moved and resized terminal sphere, through the scene in the kernel's arguments."""
    kw = M.flat_moved_case(gpu.make_camera)
    scene(*C.library_scene(gpu._lib, kw))
    got = _check_case(gpu, kw, F32_F64_GAP_FLAT, "flat, moved")
    assert (got["status"] == M.NO_SEED).sum() == 50 and (got["status"] == M.CONVERGED).sum() >= 650


def test_plumbing(gpu):
    """Host and tensor forms give the same bits; a second run equals the first; with out= only the
    planes given are written, and 64 sentinel words behind each stay intact."""
    import torch
    L = gpu._lib
    w, h = 67, 45
    dev = torch.device("cuda:0")
    kw = M.motion_case(w, h, "both", gpu.default_scene, gpu.make_camera)
    args = (w, h, kw["camera"], kw["prev_camera"])
    host = _run(gpu, kw)
    assert host["motion"].shape == (h, w, 4) and host["status"].shape == (h, w) and host["status"].dtype == np.int32
    again = _run(gpu, kw)
    first_t = torch.from_numpy(kw["first_motion"]).to(dev)
    tens = gpu.gbuffer_chain_motion_tensor(*args, first_t, prev_spheres=kw["prev_spheres"])
    torch.cuda.synchronize()
    for k in L.GBUFFER_CHAIN_MOTION_NAMES:
        assert np.array_equal(_bits(again[k]), _bits(host[k])), k
        assert np.array_equal(_bits(tens[k].cpu().numpy()), _bits(host[k])), k
    assert np.array_equal(_bits(first_t.cpu().numpy()), _bits(kw["first_motion"]))     # the input is only read
    assert set(_run(gpu, kw, status=False)) == {"motion"} and set(_run(gpu, kw, motion=False)) == {"status"}
    guard = 64
    sizes = {"motion": 4 * w * h, "status": w * h}

    def fresh(k, extra):
        if k == "status":
            return torch.full((sizes[k] + extra,), 0x7F7F7F7F, dtype=torch.int32, device=dev)
        return torch.full((sizes[k] + extra,), SENTINEL, device=dev)

    st = torch.cuda.Stream(dev)
    st.wait_stream(torch.cuda.current_stream(dev))
    for only in (L.GBUFFER_CHAIN_MOTION_NAMES, ("motion",), ("status",)):
        part = {k: fresh(k, guard) for k in L.GBUFFER_CHAIN_MOTION_NAMES}
        out = {k: part[k] for k in only}
        assert gpu.gbuffer_chain_motion_tensor(*args, first_t, prev_spheres=kw["prev_spheres"], out=out, stream=st) is out
        st.synchronize()
        for k, n in sizes.items():
            t = part[k].cpu().numpy()
            sentinel = fresh(k, guard).cpu().numpy()
            assert np.array_equal(_bits(t[:n]), _bits(host[k]).ravel() if k in only else _bits(sentinel[:n])), (only, k)
            assert np.array_equal(_bits(t[n:]), _bits(sentinel[n:])), f"{only} {k}: guard"
    # the search parameters reach the kernel: one iteration and a tight converged_px end as the restatement's do
    one = _run(gpu, kw, iterations=1, converged_px=1e-3)
    assert (one["status"] == M.CONVERGED).sum() < (host["status"] == M.CONVERGED).sum()
    f32, _ = M.chain_motion(dtype=np.float32, **dict(kw, iterations=1, converged_px=1e-3))
    assert np.array_equal(one["status"], f32["status"])


def test_composition_with_step_gbuffer(gpu):
    """The documented composition, no stage changed: gbuffer_tensor's motion through
    gbuffer_chain_motion_tensor into TemporalAccumulator.step_gbuffer with the chain's key as id, two
    orbit frames on one stream. The state equals temporal_accumulate_gbuffer_host's fed the same planes,
    bit for bit, and the followed pixels that converged keep their history."""
    import torch
    w, h = 67, 45
    dev = torch.device("cuda:0")
    cam, pcam = G.camera_pair(gpu.make_camera, w, h)
    rng = np.random.default_rng(11)
    colours = [TG.quad(rng.uniform(0.05, 2.0, (h, w, 3))) for _ in range(2)]
    acc = gpu.TemporalAccumulator(w, h, dev)
    frames = []
    for colour, (c, p) in zip(colours, ((pcam, pcam), (cam, pcam))):
        g = gpu.gbuffer_tensor(w, h, c, p, out=acc.gbuffer_planes())
        chain = gpu.gbuffer_chain_tensor(w, h, c, out={"key": torch.zeros((h, w), dtype=torch.int32, device=dev)})
        cm = gpu.gbuffer_chain_motion_tensor(w, h, c, p, g["motion"])
        planes = {"normal": g["normal"], "motion": cm["motion"], "id": chain["key"]}
        acc.step_gbuffer(torch.from_numpy(colour).to(dev), planes)
        torch.cuda.synchronize()
        frames.append(({k: v.cpu().numpy() for k, v in planes.items()}, cm["status"].cpu().numpy()))
    (p0, _), (p1, status) = frames
    s0 = gpu.temporal_accumulate_gbuffer_host(colours[0], p0, None, None)
    s1 = gpu.temporal_accumulate_gbuffer_host(colours[1], p1, {"normal": p0["normal"], "id": p0["id"]}, s0)
    for name in ("color", "moment2"):
        got = acc.state[name].cpu().numpy()
        keep = [0, 1, 2] if name == "color" else [0, 1, 2, 3]            # (the colour's alpha is not the step's)
        assert np.array_equal(_bits(got[..., keep]), _bits(s1[name][..., keep])), name
    conv = status == M.CONVERGED
    n = s1["moment2"][..., 3]
    print(f"composition: {int(conv.sum())} converged, of those {int((n[conv] == 2).sum())} kept their history")
    # (a converged q lies inside its key's region, but near a silhouette its four taps need not)
    assert conv.sum() >= 400 and (n[conv] > 1).mean() >= 0.8


def test_state_after_shutdown(gpu):
    """Without lrt_initialize(): LRT_E_STATE."""
    L = gpu._lib
    cam, pcam = G.camera_pair(gpu.make_camera, 16, 9)
    first = np.zeros((9, 16, 4), np.float32)
    first[..., 3] = 1
    gpu.ShutdownTest()
    try:
        with pytest.raises(gpu.LrtError) as e:
            gpu.gbuffer_chain_motion_host(16, 9, cam, pcam, first)
        assert e.value.code == L.LRT_E_STATE
    finally:
        gpu.InitializeTest()
    assert (gpu.gbuffer_chain_motion_host(16, 9, cam, pcam, first)["status"] != M.NOT_FOLLOWED).any()
