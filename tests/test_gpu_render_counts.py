"""The render under a per-pixel count plane on the GPU (lrt_render_counts_device / _host,
learnraytracing_amd/csrc/lrt_render_counts*.{h,hip}). Its two identities hold bit for bit:
  A. a rendered pixel equals the same pixel of lrt_render_host with frames = its clamped count,
     everything else equal (whichever kernel that call picks);
  B. with counts == frames everywhere and enough capacity, buffer and ray count equal the plain
     render's.
The yardstick is the library's own plain render, once per count class, from the same previous buffer
(random rgb, a sentinel alpha per pixel). Pixels without samples, and pixels whose samples do not fit
the capacity, keep all four floats; alpha is never written."""
import numpy as np
import pytest

import gbuffer_ref as G

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.fixture
def scene(gpu):
    """set(spheres, materials); the default scene is back afterwards."""
    try:
        yield gpu.set_scene
    finally:
        gpu.set_scene(*gpu.default_scene())


def _prev(rows, xc, seed=0):
    rng = np.random.default_rng(seed)
    p = rng.uniform(0.0, 2.0, (rows, xc, 4)).astype(np.float32)
    p[..., 3] = 1000.0 + np.arange(rows * xc, dtype=np.float32).reshape(rows, xc)   # sentinel alphas
    return p


def _plan(counts, frames, capacity):
    """(clamped counts, rendered mask, skipped mask) by the definition, in Python integers."""
    c = np.clip(counts.astype(np.int64), 0, frames)
    o = np.concatenate([[0], np.cumsum(c.ravel())[:-1]]).reshape(c.shape)
    cap = int(c.sum()) if capacity is None else capacity
    fits = o + c <= cap
    return c, (c > 0) & fits, (c > 0) & ~fits


def _expected(gpu, kw, frames, prev, counts, capacity=None):
    """The buffer identity A defines: per count class one plain host render from `prev`."""
    c, rendered, skipped = _plan(counts, frames, capacity)
    want = prev.copy()
    for k in np.unique(c[rendered]):
        ref = prev.copy()
        gpu.render_host(gpu.Job(frames=int(k), **kw), ref)
        sel = rendered & (c == k)
        want[sel] = ref[sel]
    return want, c, rendered, skipped


def _check(gpu, kw, frames, counts, capacity=None, seed=0, label=""):
    d = gpu.Job(frames=frames, **kw).desc()
    prev = _prev(d.row_count, d.x_count, seed)
    assert counts.shape == (d.row_count, d.x_count)
    want, c, rendered, skipped = _expected(gpu, kw, frames, prev, counts, capacity)
    got = prev.copy()
    rays, info = gpu.render_counts_host(gpu.Job(frames=frames, **kw), got, counts,
                                        capacity=capacity if capacity is not None else max(1, int(c.sum())))
    diff = _bits(got) != _bits(want)
    assert not diff.any(), f"{label}: {int(diff.any(axis=-1).sum())} pixels differ, first {np.argwhere(diff)[0]}"
    assert info == (int(c[rendered].sum()), int(skipped.sum())), f"{label}: info {info}"
    if rendered.any():
        assert rays >= int(c[rendered].sum()), f"{label}: every sample casts a ray"
        assert (_bits(got[rendered][:, :3]) != _bits(prev[rendered][:, :3])).any()
    else:
        assert rays == 0
    return got, rays, info


@pytest.mark.parametrize("max_depth", [8, 20, 0])
@pytest.mark.parametrize("frame0", [0, 7])
def test_random_counts_19x13(gpu, frame0, max_depth):
    """Counts in 0..5, a total that is no multiple of 64; depth 20 uses the overflow stack."""
    w, h = 19, 13
    counts = np.random.default_rng(frame0 + max_depth).integers(0, 6, (h, w)).astype(np.int32)
    assert counts.sum() % 64 != 0 and (counts == 0).any() and (counts == 5).any()
    _check(gpu, dict(width=w, height=h, frame0=frame0, max_depth=max_depth), 5, counts,
           label=f"frame0 {frame0} depth {max_depth}")


def _maps(w, h):
    bands = np.ascontiguousarray(np.repeat(np.array([[0, 1, 4, 2, 0, 3, 1]], np.int32), h, 0)[:, np.arange(w) * 7 // w])
    yy, xx = np.mgrid[0:h, 0:w]
    checker = np.where((xx + yy) % 2 == 0, 0, 3).astype(np.int32)
    ends = np.full((h, w), 2, np.int32)
    ends[0, 0] = ends[-1, -1] = 0
    spike = np.ones((h, w), np.int32)
    spike[h // 2, w // 2] = 130           # one pixel over three waves of the sample list
    clamp = np.random.default_rng(5).integers(-4, 12, (h, w)).astype(np.int32)
    clamp[3, 3], clamp[4, 4] = -2 ** 31, 2 ** 31 - 1
    return {"bands": (bands, 4), "checker": (checker, 3), "zero": (np.zeros((h, w), np.int32), 4),
            "ends": (ends, 2), "spike": (spike, 130), "clamp": (clamp, 3)}


@pytest.mark.parametrize("name", ["bands", "checker", "zero", "ends", "spike", "clamp"])
def test_maps_67x45(gpu, name):
    w, h = 67, 45
    counts, frames = _maps(w, h)[name]
    got, rays, info = _check(gpu, dict(width=w, height=h, frame0=2), frames, counts, label=name)
    if name == "zero":
        assert rays == 0 and info == (0, 0)
    if name == "clamp":
        assert info[0] == int(np.clip(counts, 0, 3).sum())


def test_column_window_with_a_row_map(gpu):
    w, h = 67, 45
    kw = dict(width=w, height=h, x0=3, x_count=11, row_block=2, row_period=2, row_phase=1, frame0=1)
    d = gpu.Job(frames=4, **kw).desc()
    assert (d.x_count, d.row_count) == (11, 22)
    counts = np.random.default_rng(9).integers(0, 5, (d.row_count, d.x_count)).astype(np.int32)
    _check(gpu, kw, 4, counts, label="window")


@pytest.mark.parametrize("count", [17, 1000])
def test_larger_scenes_go_through_the_grid(gpu, scene, count):
    w, h = 19, 13
    spheres, mats = G.count_scene(count, gpu.default_scene, gpu.random_scene)
    assert len(spheres) == count
    scene(spheres, mats)
    cam = G.camera_pair(gpu.make_camera, w, h)[0]
    counts = np.random.default_rng(count).integers(0, 5, (h, w)).astype(np.int32)
    for depth in (8, 12):
        _check(gpu, dict(width=w, height=h, camera=cam, max_depth=depth), 4, counts, label=f"{count} spheres depth {depth}")
    assert "acc=grid" in gpu.lib().lrt_last_launch().decode()


@pytest.mark.parametrize("w,h,frames,depth", [(19, 13, 3, 8), (67, 45, 4, 8), (67, 45, 8, 20)])
def test_identity_b_uniform_counts(gpu, w, h, frames, depth):
    """counts == frames: the buffer and the ray count of the plain render."""
    kw = dict(width=w, height=h, frame0=3, max_depth=depth)
    prev = _prev(h, w, 4)
    want = prev.copy()
    want_rays = gpu.render_host(gpu.Job(frames=frames, **kw), want)
    got = prev.copy()
    rays, info = gpu.render_counts_host(gpu.Job(frames=frames, **kw), got, np.full((h, w), frames, np.int32))
    assert np.array_equal(_bits(got), _bits(want))
    assert rays == want_rays and info == (w * h * frames, 0)


def test_two_bands_ray_count(gpu):
    """A two-band map: the rays are the sum of two windowed lrt_render_device calls."""
    import torch
    w, h, split = 67, 45, 30
    dev = torch.device("cuda:0")
    counts = np.full((h, w), 5, np.int32)
    counts[:, :split] = 2
    want_rays = torch.zeros(1, dtype=torch.int64, device=dev)
    want = np.zeros((h, w, 4), np.float32)
    for x0, xc, frames in ((0, split, 2), (split, w - split, 5)):
        buf = torch.zeros((h, xc, 4), device=dev)
        gpu.render_tensor(gpu.Job(width=w, height=h, x0=x0, x_count=xc, frames=frames), buf, want_rays)
        want[:, x0:x0 + xc] = buf.cpu().numpy()
    got = np.zeros((h, w, 4), np.float32)
    rays, info = gpu.render_counts_host(gpu.Job(width=w, height=h, frames=5), got, counts)
    assert rays == int(want_rays.item()) and info == (int(counts.sum()), 0)
    assert np.array_equal(_bits(got), _bits(want))


def test_capacity(gpu):
    w, h = 19, 13
    kw = dict(width=w, height=h, frame0=1)
    counts = np.random.default_rng(3).integers(0, 4, (h, w)).astype(np.int32)
    counts[-1, -3:] = [2, 0, 0]                       # the last non-zero pixel is not the last pixel
    total = int(counts.sum())
    _, _, info = _check(gpu, kw, 3, counts, capacity=total, label="capacity == total")
    assert info == (total, 0)
    got, _, info = _check(gpu, kw, 3, counts, capacity=total - 1, label="capacity == total - 1")
    assert info == (total - 2, 1) and np.array_equal(_bits(got[-1, -3]), _bits(_prev(h, w)[-1, -3]))
    got, _, info = _check(gpu, kw, 3, counts, capacity=1, label="capacity 1")
    assert info[0] <= 1 and info[1] == int((counts > 0).sum()) - info[0]
    # a pixel that does not fit is skipped, the pixels behind it keep their offsets: they do not move up
    c = np.zeros((h, w), np.int32)
    c[0, 0], c[0, 1], c[0, 2] = 2, 3, 1
    got, _, info = _check(gpu, kw, 3, c, capacity=4, label="a skipped pixel in the middle")
    assert info == (2, 2)
    _check(gpu, kw, 3, counts, capacity=2 ** 27, label="the largest capacity")


def test_mean_factor(gpu):
    """LRT_RC_MEAN on a zeroed buffer with frame0 = 5: NumPy's f32 out * (f32(frame0 + c) / f32(c))."""
    w, h, frame0 = 19, 13, 5
    kw = dict(width=w, height=h, frame0=frame0)
    counts = np.random.default_rng(8).integers(0, 7, (h, w)).astype(np.int32)
    prev = np.zeros((h, w, 4), np.float32)
    prev[..., 3] = 9.0
    plain, c, rendered, _ = _expected(gpu, kw, 6, prev, counts)
    f = np.float32
    scale = np.where(rendered, (frame0 + c).astype(np.float32) / np.maximum(c, 1).astype(np.float32), f(1))
    want = plain.copy()
    want[..., :3] = plain[..., :3] * scale[..., None].astype(np.float32)
    got = prev.copy()
    gpu.render_counts_host(gpu.Job(frames=6, **kw), got, counts, mean=True)
    assert np.array_equal(_bits(got), _bits(want))
    # ... which is the plain mean of the fresh samples, up to rounding
    one = [np.zeros((h, w, 4), np.float32) for _ in range(2)]
    for k in range(2):
        gpu.render_host(gpu.Job(width=w, height=h, frame0=frame0 + k, frames=1), one[k])
    two = rendered & (c == 2)
    fresh = (one[0][two][:, :3] * f(frame0 + 1) + one[1][two][:, :3] * f(frame0 + 2)) / f(2)
    assert two.any() and np.allclose(got[two][:, :3], fresh, rtol=1e-5, atol=1e-6)


def test_device_form_on_a_stream_and_determinism(gpu):
    import torch
    w, h = 67, 45
    dev = torch.device("cuda:0")
    counts = np.random.default_rng(12).integers(0, 6, (h, w)).astype(np.int32)
    job = gpu.Job(width=w, height=h, frame0=4, frames=5, max_depth=20)
    prev = _prev(h, w, 2)
    want = prev.copy()
    want_rays, want_info = gpu.render_counts_host(job, want, counts)
    again = prev.copy()
    assert gpu.render_counts_host(job, again, counts) == (want_rays, want_info)
    assert np.array_equal(_bits(again), _bits(want))
    st = torch.cuda.Stream(dev)
    with torch.cuda.stream(st):
        buf = torch.from_numpy(prev).to(dev, non_blocking=False)
        tcounts = torch.from_numpy(counts).to(dev)
        rays = torch.zeros(1, dtype=torch.int64, device=dev)
        info = torch.full((2,), -1, dtype=torch.int64, device=dev)
    gpu.render_counts_tensor(job, buf, rays, tcounts, None, info=info, stream=st)
    st.synchronize()
    assert np.array_equal(_bits(buf.cpu().numpy()), _bits(want))
    assert int(rays.item()) == want_rays and tuple(info.cpu().tolist()) == want_info
    assert "counts_trace_kernel" in gpu.lib().lrt_last_launch().decode()
    with pytest.raises(gpu.LrtError):
        gpu.render_counts_tensor(job, buf, rays, tcounts.to(torch.int64), None)
    with pytest.raises(gpu.LrtError):
        gpu.render_counts_tensor(job, buf, rays, tcounts[:-1], None)


def test_budget_render_accumulate_composition(gpu):
    """sample_budget_tensor -> render_counts_tensor(mean=True) -> step_gbuffer(cur_scale=1) on one
    stream: it runs, and the colour is finite wherever a sample was taken."""
    import torch
    w, h = 67, 45
    dev = torch.device("cuda:0")
    cam = gpu.default_camera(w, h)
    acc = gpu.TemporalAccumulator(w, h, dev)
    rays = torch.zeros(1, dtype=torch.int64, device=dev)
    pilot = torch.zeros((h, w, 4), device=dev)
    gpu.render_tensor(gpu.Job(width=w, height=h, frames=2, camera=cam), pilot, rays)
    planes = gpu.gbuffer_tensor(w, h, cam, out=acc.gbuffer_planes())
    _, guides = acc.step_gbuffer(pilot, planes)
    counts = gpu.sample_budget_tensor(guides["color_std"], 0, 16, 3 * w * h, color=acc.state["color"],
                                      flags=gpu._lib.SB_STD)
    info = torch.zeros(2, dtype=torch.int64, device=dev)
    buf = torch.zeros((h, w, 4), device=dev)
    gpu.render_counts_tensor(gpu.Job(width=w, height=h, frame0=2, frames=16, camera=cam), buf, rays, counts,
                             3 * w * h, mean=True, info=info)
    planes = gpu.gbuffer_tensor(w, h, cam, out=acc.gbuffer_planes())
    col, _ = acc.step_gbuffer(buf, planes, cur_scale=1.0)
    torch.cuda.synchronize()
    c = counts.cpu().numpy()
    assert c.sum() <= 3 * w * h and tuple(info.cpu().tolist()) == (int(c.sum()), 0)
    assert np.isfinite(col.cpu().numpy()[c > 0][:, :3]).all()
    assert (buf.cpu().numpy()[c == 0] == 0).all()
