"""The *_host entry points' device mirrors (HostMirrors, learnraytracing_amd/csrc/lrt_internal.h) in
the argument combinations that the per-unit contract tests do not reach: buffers that are absent,
given but not read, updated in place, or a lone 4-byte plane. Each host call must give the bits of
the tensor form on the same inputs, keep the alphas the kernels leave, and write nothing past a
buffer's end. Inputs are seeded noise (the forms run the same kernel: any input serves), at 67 x 45
(no multiple of a tile, word planes of 12,060 B) and 1 x 1.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SIZES = [(67, 45), (1, 1)]
IDS = [f"{w}x{h}" for w, h in SIZES]
STATE = ("color", "moment2", "normal", "world_pos")
GUARD = 4   # sentinel words behind a word plane


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _same(t, a):
    return np.array_equal(_bits(t.cpu().numpy()), _bits(a))


def _quads(rng, w, h, lo=-1.0, hi=1.0):
    return rng.uniform(lo, hi, (h, w, 4)).astype(np.float32)


def _up(x):
    import torch
    if isinstance(x, dict):
        return {k: _up(v) for k, v in x.items()}
    return torch.from_numpy(x.copy()).to("cuda:0")


def _state(rng, w, h):
    s = {n: _quads(rng, w, h) for n in STATE}
    s["moment2"][..., 3] = rng.integers(1, 9, (h, w))   # the history length
    return s


@pytest.mark.parametrize("w,h", SIZES, ids=IDS)
def test_temporal_static_minimal(gpu, w, h):
    """No prev, no albedo, no color_std: four outputs, of which color keeps its alpha."""
    import torch
    rng = np.random.default_rng(100 * w + h)
    cam = gpu.default_camera(w, h)
    color, cur = _quads(rng, w, h, 0, 2), {n: _quads(rng, w, h) for n in ("normal", "world_pos")}
    out = {n: np.full((h, w, 4), 7.0, np.float32) for n in STATE}
    gpu.temporal_accumulate_host(color, cur, None, cam, cam, out=out)
    tout = {n: torch.full((h, w, 4), 7.0, device="cuda:0") for n in STATE}
    gpu.temporal_accumulate_tensor(_up(color), _up(cur), None, cam, cam, out=tout)
    torch.cuda.synchronize()
    assert (out["color"][..., 3] == 7.0).all() and (out["moment2"][..., 3] == 1.0).all()
    for n in STATE:
        assert _same(tout[n], out[n]), n


@pytest.mark.parametrize("with_motion", [True, False], ids=["motion", "no-motion"])
@pytest.mark.parametrize("w,h", SIZES, ids=IDS)
def test_temporal_moving(gpu, w, h, with_motion):
    import torch
    rng = np.random.default_rng(200 * w + h)
    cam = gpu.default_camera(w, h)
    sph = np.array([[s.center.x, s.center.y, s.center.z, s.radius] for s in gpu.get_scene()[0]], np.float32)
    psph = sph.copy()
    psph[1, 0] += 0.25
    color, prev = _quads(rng, w, h, 0, 2), _state(rng, w, h)
    cur = {n: _quads(rng, w, h) for n in ("normal", "world_pos", "albedo")}
    names = STATE + ("albedo", "color_std")
    out = {n: np.full((h, w, 4), 7.0, np.float32) for n in names}
    motion = np.full((h, w, 4), 77.0, np.float32) if with_motion else None
    gpu.temporal_accumulate_moving_host(color, cur, prev, cam, cam, sph, psph, out=out, motion=motion)
    tout = {n: torch.full((h, w, 4), 7.0, device="cuda:0") for n in names}
    tmotion = torch.full((h, w, 4), 77.0, device="cuda:0") if with_motion else None
    gpu.temporal_accumulate_moving_tensor(_up(color), _up(cur), _up(prev), cam, cam, sph, psph, out=tout, motion=tmotion)
    torch.cuda.synchronize()
    assert (out["color"][..., 3] == 7.0).all() and (out["color_std"][..., 3] == 7.0).all()
    for n in names:
        assert _same(tout[n], out[n]), n
    if with_motion:
        assert _same(tmotion, motion) and (motion[..., 3] <= 1.0).all()   # all four words are written


@pytest.mark.parametrize("albedo", [True, False], ids=["albedo", "no-albedo"])
@pytest.mark.parametrize("w,h", SIZES, ids=IDS)
def test_upsample_bilinear(gpu, w, h, albedo):
    """LRT_UP_BILINEAR: the normals are given and not read; with and without the albedo planes."""
    import torch
    rng = np.random.default_rng(300 * w + h)
    lw, lh = (w + 1) // 2, (h + 1) // 2

    def planes(pw, ph):
        g = {"id": rng.integers(-1, 9, (ph, pw)).astype(np.int32), "normal": _quads(rng, pw, ph)}
        if albedo:
            g["albedo"] = _quads(rng, pw, ph, 0.05, 1.0)
        return g

    color, low, high = _quads(rng, lw, lh, 0, 2), planes(lw, lh), planes(w, h)
    out = np.full((h, w, 4), 7.0, np.float32)
    cls = np.full(w * h + GUARD, 7, np.int32)
    gpu.upsample_host(color, low, high, out=out, class_out=cls, flags=gpu._lib.UP_BILINEAR)
    tout = torch.full((h, w, 4), 7.0, device="cuda:0")
    tcls = torch.full((w * h + GUARD,), 7, dtype=torch.int32, device="cuda:0")
    gpu.upsample_tensor(_up(color), _up(low), _up(high), out=tout, class_out=tcls, flags=gpu._lib.UP_BILINEAR)
    torch.cuda.synchronize()
    assert (out[..., 3] == 7.0).all() and (cls[:w * h] == 2).all() and (cls[w * h:] == 7).all()
    assert _same(tout, out) and _same(tcls, cls)
    plain = gpu.upsample_host(color, low, high, flags=gpu._lib.UP_BILINEAR)   # no class plane
    assert np.array_equal(_bits(plain[..., :3]), _bits(out[..., :3]))


@pytest.mark.parametrize("w,h", SIZES, ids=IDS)
def test_svgf_in_place_without_variance(gpu, w, h):
    import torch
    rng = np.random.default_rng(400 * w + h)
    color, moment2 = _quads(rng, w, h, 0, 2), _quads(rng, w, h, 4, 6)
    moment2[..., 3] = rng.integers(1, 9, (h, w))
    guides = {"normal": _quads(rng, w, h), "world_pos": _quads(rng, w, h), "albedo": _quads(rng, w, h, 0.05, 1.0)}
    color[..., 3] = 7.0
    tcolor, tm2, tg = _up(color), _up(moment2), _up(guides)
    assert gpu.svgf_filter_tensor(tcolor, tm2, tg, out=tcolor, iterations=2) is tcolor
    torch.cuda.synchronize()
    keep = color.copy()
    assert gpu.svgf_filter_host(color, moment2, guides, out=color, iterations=2) is color
    assert (color[..., 3] == 7.0).all() and not np.array_equal(color[..., :3], keep[..., :3])
    assert _same(tcolor, color)
    # out of place without variance_out: the same rgb, and color is left as it was
    out = gpu.svgf_filter_host(keep, moment2, guides, iterations=2)
    assert np.array_equal(_bits(out), _bits(color))


@pytest.mark.parametrize("w,h", SIZES, ids=IDS)
def test_tonemap_without_metering(gpu, w, h):
    """auto_exposure = 0: neither the state nor the histogram is mirrored. out == color, and bgra alone."""
    import torch
    rng = np.random.default_rng(500 * w + h)
    color = _quads(rng, w, h, 0, 4)
    color[..., 3] = 7.0
    kw = dict(auto_exposure=0, ev_bias=0.5)
    tcolor = _up(color)
    gpu.tonemap_tensor(tcolor, out=tcolor, **kw)
    tbgra = torch.full((w * h + GUARD,), 7, dtype=torch.int32, device="cuda:0")
    gpu.tonemap_tensor(_up(color), bgra=tbgra, **kw)
    torch.cuda.synchronize()
    mapped, keep = color.copy(), color.copy()
    assert gpu.tonemap_host(mapped, out=mapped, **kw) is None
    assert (mapped[..., 3] == 7.0).all() and not np.array_equal(mapped[..., :3], keep[..., :3])
    assert _same(tcolor, mapped)
    bgra = np.full(w * h + GUARD, 7, np.uint32)
    gpu.tonemap_host(color, bgra=bgra, **kw)
    assert np.array_equal(_bits(color), _bits(keep)) and (bgra[w * h:] == 7).all()
    assert _same(tbgra, bgra)


@pytest.mark.parametrize("w,h", SIZES, ids=IDS)
def test_gbuffer_id_alone(gpu, w, h):
    """A single 4-byte plane: the mirror's rounded size is not the plane's."""
    import torch
    cam = gpu.default_camera(w, h)
    ids = np.full(w * h + GUARD, 7, np.int32)
    gpu.gbuffer_host(w, h, cam, out={"id": ids})
    tids = torch.full((w * h + GUARD,), 7, dtype=torch.int32, device="cuda:0")
    gpu.gbuffer_tensor(w, h, cam, out={"id": tids})
    torch.cuda.synchronize()
    assert (ids[w * h:] == 7).all() and ((ids[:w * h] >= -1) & (ids[:w * h] < 9)).all()
    assert _same(tids, ids)
