"""The G-buffer pass on the GPU (lrt_gbuffer_device / _host, gbuffer_kernel of
learnraytracing_amd/csrc/lrt_gbuffer.hip).

Pinned: id and depth equal the library's own closest hit (lrt_accel_eval's host walk, mode 0, of the
grid, and of the BVH where there are two spheres) on the NumPy rays of tests/gbuffer_ref.py bit for
bit at every pixel, and albedo is the material's bit for bit.

The house rule of tests/test_gpu_temporal.py for normal, world_pos and motion:
|got - f64| <= TOL * max(1, |f64|) at every pixel none of whose decisions lies within 1e-4 of its
threshold (the restatement's `fragile` mask), TOL = 16 x the largest gap between the restatement's
own f32 and f64 runs on the same cases (`python tests/gbuffer_ref.py` measures it on the CPU;
tests/test_gbuffer_cpu.py holds the restatement to it). motion.z and motion.w are exact there."""
import ctypes

import numpy as np
import pytest

import gbuffer_ref as G
import temporal_motion_ref as M
import temporal_ref as R

pytestmark = pytest.mark.gpu

F32_F64_GAP = 2e-4                               # measured: 1.89e-04 (the default scene at SHAPES; counts up to 17: 1.09e-04)
F32_F64_GAP_COUNT = {1000: 3.1e-3, 4096: 4e-2}   # measured: 3.04e-03, 3.90e-02 (HitSphere's cancellation on r = 0.05)
F32_F64_GAP_DESIGNED = 1.1e-5                    # measured: 1.01e-05
MAX_FRAGILE = 0.02
SENTINEL = 7.0
POOL = 512   # LRT_F_POOL


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _accel(L, spheres, rays, accel):
    sa = (L.Sphere * len(spheres))(*spheres)
    ids, ts = np.zeros(len(rays), np.int32), np.zeros(len(rays), np.float32)
    L.check(L.lib().lrt_accel_eval(sa, len(spheres), rays.ctypes.data, len(rays), accel, 0, ids.ctypes.data,
                                   ts.ctypes.data))
    return ids, ts


def _spheres(L, arr):
    return [L.Sphere(L.f3(*s[:3]), float(s[3])) for s in G.sphere_array(arr)]


@pytest.fixture
def scene(gpu):
    """set(spheres, materials); the default scene is back afterwards."""
    try:
        yield gpu.set_scene
    finally:
        gpu.set_scene(*gpu.default_scene())


def _check_case(gpu, kw, gap, label):
    """One restatement case (the library holds kw's scene): the pin and the house rule."""
    L = gpu._lib
    w, h, cam, spheres = kw["w"], kw["h"], kw["camera"], kw["spheres"]
    got = gpu.gbuffer_host(w, h, cam, kw["prev_camera"], id=True, depth=True, motion=True,
                           prev_spheres=kw["prev_spheres"])
    assert set(got) == set(L.GBUFFER_NAMES)
    rays = G.accel_rays(w, h, cam)
    for accel in (2, 1) if len(spheres) >= 2 else (2,):
        ids, ts = _accel(L, spheres, rays, accel)
        ids, ts = ids.reshape(h, w), ts.reshape(h, w)
        assert np.array_equal(got["id"], ids), f"{label}: id, accel {accel}"
        hit = ids >= 0
        assert np.array_equal(_bits(got["depth"][hit]), _bits(ts[hit])), f"{label}: depth, accel {accel}"
        assert np.isposinf(got["depth"][~hit]).all()
    want_alb = np.where(hit[..., None], kw["albedo"][np.maximum(ids, 0)], np.float32(0))
    assert np.array_equal(_bits(got["albedo"][..., :3]), _bits(want_alb)), f"{label}: albedo"
    quarter = gpu.gbuffer_host(w, h, cam, guide_scale=0.25, out={"albedo": np.full((h, w, 4), SENTINEL, np.float32)})
    assert np.array_equal(_bits(quarter["albedo"][..., :3]), _bits(np.float32(0.25) * want_alb))
    for name in G.GUIDES:
        assert (got[name][..., 3] == 0).all() and np.isfinite(got[name]).all(), name
    # the f32 restatement is the kernel's arithmetic operation for operation (IEEE operations in the
    # same order, no contraction; the library's short sqrt and reciprocal are correctly rounded): the
    # point and the normal are its bits, which a tolerance 16 x a gap of 4e-2 would not show
    f32, _ = G.gbuffer(dtype=np.float32, **kw)
    for name in ("normal", "world_pos"):
        assert np.array_equal(_bits(got[name][..., :3]), _bits(f32[name])), f"{label}: {name} against the f32 restatement"
    want, fragile = G.gbuffer(dtype=np.float64, **kw)
    share = fragile.mean()
    assert share <= MAX_FRAGILE
    if w * h <= 15:
        assert not fragile.any()
    ok = ~fragile
    assert np.array_equal(got["id"][ok], want["id"][ok]), f"{label}: f64 ids off the mask"
    assert np.array_equal(got["motion"][..., 2:][ok], np.float32(want["motion"][..., 2:][ok])), f"{label}: motion z, w"
    gaps = G.rel_gaps(got, want, ok)
    tol = 16 * gap
    print(f"{label}: fragile {100 * share:.2f} %, gaps " + ", ".join(f"{k} {v:.3g}" for k, v in gaps.items()) +
          f" (bound {tol:.3g})")
    for name, g in gaps.items():
        assert g <= tol, f"{label} {name}: {g:.3g} > {tol:.3g}"
    return got


@pytest.mark.parametrize("w,h", G.SHAPES, ids=[f"{w}x{h}" for w, h in G.SHAPES])
def test_default_scene_shapes(gpu, w, h):
    """The default scene from the default camera, one orbit step and moved spheres behind it."""
    spheres, mats = gpu.default_scene()
    cam, pcam = G.camera_pair(gpu.make_camera, w, h)
    kw = dict(w=w, h=h, camera=cam, spheres=spheres, albedo=G.albedo_array(mats), prev_camera=pcam,
              prev_spheres=G.moved_scene(spheres))
    got = _check_case(gpu, kw, F32_F64_GAP, f"{w}x{h}")
    if w * h > 1000:
        moved = np.isin(got["id"], (2, 4, 6))
        assert moved.sum() >= 10 and (np.abs(got["motion"][..., :2][moved]) > 0.25).any()


@pytest.mark.parametrize("count", G.COUNTS)
def test_sphere_counts(gpu, scene, count):
    """19 x 13: 1 sphere, the scan up to 16, the grid from 17 on, 1000 and LRT_MAX_SPHERES (the two
    scenes' spheres in the kernel's arguments up to 64, uploaded above)."""
    w, h = G.COUNT_SIZE
    spheres, mats = G.count_scene(count, gpu.default_scene, gpu.random_scene)
    assert len(spheres) == count
    scene(spheres, mats)
    cam, pcam = G.camera_pair(gpu.make_camera, w, h)
    kw = dict(w=w, h=h, camera=cam, spheres=spheres, albedo=G.albedo_array(mats), prev_camera=pcam,
              prev_spheres=G.moved_scene(spheres))
    got = _check_case(gpu, kw, F32_F64_GAP_COUNT.get(count, F32_F64_GAP), f"count {count}")
    assert (got["id"] >= 0).any() and got["id"].max() < count


@pytest.mark.parametrize("name", G.DESIGNED_CASES)
def test_designed_motion(gpu, scene, name):
    """Two spheres and the sky in front of a pinhole camera: nothing moved (no scene, and a scene
    whose two arrays agree), a translated and a resized sphere, a sphere that came from behind the
    previous camera, one that was not there, and a translation with a known answer."""
    L = gpu._lib
    kw = G.designed_case(name, gpu.make_camera)
    w, h = kw["w"], kw["h"]
    scene(_spheres(L, kw["spheres"]), [L.Material(L.LAMBERT, L.f3(*a), L.f3(0, 0, 0), 0.0, 0.0) for a in kw["albedo"]])
    got = gpu.gbuffer_host(w, h, kw["camera"], kw["prev_camera"], id=True, depth=True, motion=True,
                           prev_spheres=kw["prev_spheres"])
    want, fragile = G.gbuffer(dtype=np.float64, **kw)
    assert fragile.mean() <= MAX_FRAGILE
    ok = ~fragile
    ids, mv = got["id"], got["motion"]
    assert np.array_equal(ids[ok], want["id"][ok]) and all((ids == i).sum() > 50 for i in (-1, 0, 1))
    assert np.array_equal(mv[..., 2:][ok], np.float32(want["motion"][..., 2:][ok]))
    for plane, g in G.rel_gaps(got, want, ok).items():
        assert g <= 16 * F32_F64_GAP_DESIGNED, f"{name} {plane}: {g:.3g}"
    if name in ("static", "static_scene"):      # hits and misses alike take their own centre, exactly
        assert (mv[..., :2] == 0).all() and (mv[..., 3] == 1).all()
    if name == "static_scene":                  # scene = NULL against a scene in which nothing moved: the same bits
        none = gpu.gbuffer_host(w, h, kw["camera"], kw["prev_camera"], id=True, depth=True, motion=True)
        for plane in L.GBUFFER_NAMES:
            assert np.array_equal(_bits(none[plane]), _bits(got[plane])), plane
    if name == "moved":
        assert (mv[..., 3] == 1).all() and (np.abs(mv[..., :2]) > 0.5).any(-1)[ids >= 0].mean() > 0.9
    if name in ("behind", "gone"):              # not projectable: w = 0 with x = y = 0, the id stays
        assert (mv[ids == 1] == np.float32([0, 0, 1, 0])).all() and (mv[..., 3][ids != 1] == 1).all()
    if name == "analytic":
        on_b = ids == 1
        depth = 3.0 - np.float64(got["world_pos"][..., 2])
        assert R.rel_gap(mv[..., 0][on_b], G.analytic_displacement(h, depth)[on_b]) <= 16 * F32_F64_GAP_DESIGNED
        assert np.abs(mv[..., 1][on_b]).max() <= 16 * F32_F64_GAP_DESIGNED
        assert (mv[..., :2][~on_b] == 0).all() and (mv[..., 3] == 1).all()


def _guarded(torch, name, n, guard, dev):
    """A flat plane of n elements and `guard` more, all the sentinel."""
    if name == "id":
        return torch.full((n + guard,), 0x7F7F7F7F, dtype=torch.int32, device=dev)
    return torch.full((n + guard,), SENTINEL, device=dev)


@pytest.mark.parametrize("w,h", [(67, 45), (1, 1)], ids=["67x45", "1x1"])
def test_contract(gpu, w, h):
    """Host, device and tensor forms give the same bits; a plane that is not asked for stays
    untouched; nothing is written past a plane's end; the RGBA alphas are 0; guide_scale multiplies
    the guides and nothing else; the scene's cases of LRT_E_INVALID."""
    import torch
    L = gpu._lib
    dev = torch.device("cuda:0")
    spheres, _ = gpu.default_scene()
    cam, pcam = G.camera_pair(gpu.make_camera, w, h)
    prev = G.moved_scene(spheres)
    kw = dict(id=True, depth=True, motion=True, prev_spheres=prev)
    host = gpu.gbuffer_host(w, h, cam, pcam, **kw)
    assert [host[k].shape for k in L.GBUFFER_NAMES] == [(h, w, 4)] * 3 + [(h, w), (h, w), (h, w, 4)]
    assert host["id"].dtype == np.int32
    for name in G.GUIDES:
        assert (host[name][..., 3] == 0).all()
    # the tensor form, every plane with a guard behind it
    guard = 64
    sizes = {k: w * h * (1 if k in ("id", "depth") else 4) for k in L.GBUFFER_NAMES}
    tout = {k: _guarded(torch, k, n, guard, dev) for k, n in sizes.items()}
    st = torch.cuda.Stream(dev)
    st.wait_stream(torch.cuda.current_stream(dev))
    assert gpu.gbuffer_tensor(w, h, cam, pcam, prev_spheres=prev, out=tout, stream=st) is tout
    st.synchronize()
    for k, n in sizes.items():
        t = tout[k].cpu().numpy()
        assert np.array_equal(_bits(t[:n]), _bits(host[k]).ravel()), k
        assert np.array_equal(_bits(t[n:]), _bits(_guarded(torch, k, 0, guard, "cpu").numpy())), f"{k}: guard"
    # the device entry point itself, into fresh tensors
    fresh = gpu.gbuffer_tensor(w, h, cam, pcam, **kw)
    d = gpu.gbuffer_desc(w, h, cam, pcam)
    raw = {k: _guarded(torch, k, n, 0, dev) for k, n in sizes.items()}
    g = L.Gbuffer()
    for k, t in raw.items():
        setattr(g, k, t.data_ptr())
    sm = gpu.renderer._scene_motion(spheres, prev)
    torch.cuda.synchronize()
    assert L.lib().lrt_gbuffer_device(ctypes.byref(d), ctypes.byref(sm), ctypes.byref(g), None) == 0
    torch.cuda.synchronize()
    for k in L.GBUFFER_NAMES:
        assert np.array_equal(_bits(fresh[k].cpu().numpy()), _bits(host[k])), k
        assert np.array_equal(_bits(raw[k].cpu().numpy()), _bits(host[k]).ravel()), k
    # only what is asked for is written, and asking for less changes nothing
    for only in (("normal",), ("id",), ("depth", "motion"), ("world_pos", "albedo")):
        part = {k: _guarded(torch, k, n, 0, dev) for k, n in sizes.items()}
        gpu.gbuffer_tensor(w, h, cam, pcam, prev_spheres=prev, out={k: part[k] for k in only})
        torch.cuda.synchronize()
        for k, n in sizes.items():
            want = _bits(host[k]).ravel() if k in only else _bits(_guarded(torch, k, n, 0, "cpu").numpy())
            assert np.array_equal(_bits(part[k].cpu().numpy()), want), (only, k)
    guides = gpu.gbuffer_host(w, h, cam)
    assert set(guides) == set(G.GUIDES)
    # guide_scale: the guides (an exact factor here), not id, depth or motion
    half = gpu.gbuffer_host(w, h, cam, pcam, guide_scale=0.5, **kw)
    for k in G.GUIDES:
        assert np.array_equal(_bits(half[k]), _bits(np.float32(0.5) * host[k])), k
    for k in L.GBUFFER_EXTRA_NAMES:
        assert np.array_equal(_bits(half[k]), _bits(host[k])), k
    third = gpu.gbuffer_host(w, h, cam, guide_scale=1 / 3)
    for k in G.GUIDES:
        assert np.array_equal(_bits(third[k]), _bits(np.float32(1 / 3) * host[k])), k
    # the scene must be the library's: another count, another sphere
    for bad in (G.sphere_array(spheres)[:8], G.moved_scene(spheres)):
        with pytest.raises(gpu.LrtError) as e:
            gpu.gbuffer_host(w, h, cam, pcam, motion=True, spheres=bad, prev_spheres=bad)
        assert e.value.code == L.LRT_E_INVALID and "current scene" in str(e.value)
    same = gpu.gbuffer_host(w, h, cam, pcam, spheres=spheres, **kw)
    for k in L.GBUFFER_NAMES:
        assert np.array_equal(_bits(same[k]), _bits(host[k])), k


def test_state_after_shutdown(gpu):
    """Without lrt_initialize(): LRT_E_STATE (tests/test_gpu_multidev.py shuts down and comes back
    the same way)."""
    L = gpu._lib
    cam = gpu.default_camera(16, 9)
    gpu.ShutdownTest()
    try:
        with pytest.raises(gpu.LrtError) as e:
            gpu.gbuffer_host(16, 9, cam)
        assert e.value.code == L.LRT_E_STATE
    finally:
        gpu.InitializeTest()
    assert (gpu.gbuffer_host(16, 9, cam, id=True)["id"] >= 0).any()


def test_pool_colour_with_gbuffer_guides_accumulates(gpu, scene):
    """What it is for. 67 x 45, a static camera, fresh seeds: step t renders sample frame0 = t with
    the pool kernel (which has no feature output) into zeroed buffers, cur_scale = t + 1, and takes
    its guides from gbuffer_tensor(guide_scale = 1 / cur_scale) through TemporalAccumulator: after 8
    steps the history is 8 long on at least 99 % of the pixels. Then sphere MOVING_ID comes down a
    step at a time (step(spheres=, motion=)): its interior pixels keep their history, n > 1."""
    import torch
    L = gpu._lib
    w, h, steps = 67, 45, 8
    dev = torch.device("cuda:0")
    cam = gpu.default_camera(w, h)
    spheres, mats = gpu.default_scene()
    moving = 4
    base = G.sphere_array(spheres)
    acc = gpu.TemporalAccumulator(w, h, dev)
    rays = torch.zeros(1, dtype=torch.int64, device=dev)
    motion = torch.zeros((h, w, 4), device=dev)

    def frame(t, sph, **kw):
        scene(_spheres(L, sph), mats)
        buf = torch.zeros((h, w, 4), device=dev)
        gpu.render_tensor(gpu.Job(width=w, height=h, frame0=t, frames=1, max_depth=8, camera=cam, flags=POOL), buf, rays)
        assert L.last_launch()["kernel"] == "pool_kernel"
        k = float(t + 1)
        guides = gpu.gbuffer_tensor(w, h, cam, guide_scale=1.0 / k)
        acc.step(buf, guides, cam, cur_scale=k, **kw)
        return guides

    first = base.copy()
    first[M.MOVING_ID, :3] -= np.float32(M.MOVING_STEP) * np.float32(moving)
    for t in range(steps):
        frame(t, first, spheres=first)
    torch.cuda.synchronize()
    n = acc.state["moment2"][..., 3].cpu().numpy()
    full = n >= steps - 0.01                    # (n is a bilinear mean of histories plus one: 8 within rounding)
    print(f"history after {steps} static steps: n = {steps} on {100 * full.mean():.2f} % of the pixels "
          f"(exactly on {100 * (n == steps).mean():.2f} %)")
    assert full.mean() >= 0.99
    for i in range(1, moving + 1):
        sph = base.copy()
        sph[M.MOVING_ID, :3] -= np.float32(M.MOVING_STEP) * np.float32(moving - i)
        frame(steps - 1 + i, sph, spheres=sph, motion=motion)
        ids = gpu.gbuffer_tensor(w, h, cam, out={"id": torch.zeros((h, w), dtype=torch.int32, device=dev)})["id"]
        torch.cuda.synchronize()
        on = ids.cpu().numpy() == M.MOVING_ID
        inner = on.copy()                       # the pixels whose eight neighbours show the sphere too
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                inner &= np.roll(np.roll(on, dy, 0), dx, 1)
        inner[[0, -1], :] = inner[:, [0, -1]] = False
        n = acc.state["moment2"][..., 3].cpu().numpy()
        mv = motion.cpu().numpy()
        print(f"moving step {i}: sphere {M.MOVING_ID} on {int(on.sum())} px, interior {int(inner.sum())}, "
              f"least n there {n[inner].min() if inner.any() else 0:.3g}, matched {int((mv[..., 2][inner] == M.MOVING_ID).sum())}")
        assert inner.sum() >= 10
        assert (n[inner] > 1).all()
        assert (mv[..., 2][inner] == M.MOVING_ID).all() and (np.abs(mv[..., 1][inner]) > 1).all()
