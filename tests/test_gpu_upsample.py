"""G-buffer-guided upsampling on the GPU (lrt_upsample_device / _host, upsample_kernel of
learnraytracing_amd/csrc/lrt_upsample.hip) against its NumPy restatement (tests/upsample_ref.py): the
library's own G-buffer planes at both sizes and pool-kernel colours at the low size, sizes that cross
the 32-wide block and the 8-high wave, ratios 1, 2, 3 by 1 and a non-integer one, sphere counts on
either side of the grid, the designed cases, the buffer contract, what it is for (full-resolution
silhouettes from a quarter of the pixels) and a run through the chain.

The house rule of tests/test_gpu_temporal.py: |got - f64| <= TOL * max(1, |f64|) at every pixel off
the restatement's `fragile` mask (a class-0 or class-1 sum within 1 +- 1e-3 of weight_min), TOL = 16 x
the largest gap between the restatement's own f32 and f64 runs on the same cases
(`python tests/upsample_ref.py` measures it on the CPU; tests/test_upsample_cpu.py holds the
restatement to it and to the fragile share). The class plane equals the restatement's off the mask."""
import ctypes

import numpy as np
import pytest

import gbuffer_ref as G
import temporal_ref as R
import upsample_ref as U

pytestmark = pytest.mark.gpu

F32_F64_GAP = 9.5e-7                # measured: 9.04e-07 (rendered_gap()), with albedo, without, the flag form
TOL = 16 * F32_F64_GAP
F32_F64_GAP_DESIGNED = 1.9e-7       # measured: 1.80e-07 (designed_gap())
TOL_DESIGNED = 16 * F32_F64_GAP_DESIGNED
SENTINEL = 7.0
GUARD = 64
POOL = 512   # LRT_F_POOL
CASES = {c[0]: c for c in U.RENDERED_CASES}


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _spheres(L, arr):
    return [L.Sphere(L.f3(*s[:3]), float(s[3])) for s in G.sphere_array(arr)]


def _library(gpu, set_scene):
    """(planes, colour) as upsample_ref.rendered_case takes them: the library's own G-buffer
    (gbuffer_host) and the pool kernel's colours."""
    L = gpu._lib

    def planes(w, h, camera, spheres, mats):
        set_scene(_spheres(L, spheres), mats)
        g = gpu.gbuffer_host(w, h, camera, id=True)
        return {k: g[k] for k in ("normal", "albedo", "id")}

    def colour(w, h, camera, spheres, mats, frame0):
        set_scene(_spheres(L, spheres), mats)
        buf = np.zeros((h, w, 4), np.float32)
        gpu.render_host(gpu.Job(width=w, height=h, frame0=frame0, frames=1, max_depth=8, camera=camera, flags=POOL), buf)
        return buf

    return planes, colour


@pytest.fixture(scope="module")
def rendered(gpu):
    """{label: (color_low, low, high)} over upsample_ref.RENDERED_CASES, rendered once and left
    unchanged (the scene is set and restored here: a module fixture cannot use a function fixture)."""
    out = {}
    try:
        planes, colour = _library(gpu, gpu.set_scene)
        for label, count, w, h, lw, lh, _ in U.RENDERED_CASES:
            out[label] = U.rendered_case(count, w, h, lw, lh, U.scene_of(gpu.default_scene, gpu.random_scene),
                                         gpu.default_camera, planes, colour)
    finally:
        gpu.set_scene(*gpu.default_scene())
    return out


def _variants(low, high):
    """(name, low, high, flags): with albedo, without, the flag form (no normals given)."""
    return (("albedo", low, high, 0), ("plain", U.without_albedo(low), U.without_albedo(high), 0),
            ("flag", {k: v for k, v in low.items() if k != "normal"}, {k: v for k, v in high.items() if k != "normal"},
             U.UP_BILINEAR))


def _check(gpu, color, low, high, flags, tol, label):
    """One call against the f64 restatement under the house rule; returns the class plane."""
    h, w = high["id"].shape
    cls = np.full((h, w), -9, np.int32)
    got = gpu.upsample_host(color, low, high, class_out=cls, flags=flags)
    want, wcls, fragile = U.upsample(color, low, high, np.float64, flags)
    ok = ~fragile
    assert np.isfinite(got).all() and fragile.mean() <= U.MAX_FRAGILE
    gap = R.rel_gap(got[..., :3], want, ok)
    print(f"{label}: gap {gap:.3g} (bound {tol:.3g}), fragile {int(fragile.sum())}, classes {U.class_counts(cls)}")
    assert np.array_equal(cls[ok], wcls[ok]), label
    assert gap <= tol, f"{label}: {gap:.3g} > {tol:.3g}"
    assert (got[..., 3] == 0).all()                       # the zeroed default out: its alpha stays
    return cls, fragile


@pytest.mark.parametrize("label", list(CASES), ids=[c.replace(" ", "") for c in CASES])
def test_upsample_vs_restatement(gpu, rendered, label):
    color, low, high = rendered[label]
    _, _, w, h, lw, lh, counts = CASES[label]
    for name, lo, hi, flags in _variants(low, high):
        cls, fragile = _check(gpu, color, lo, hi, flags, TOL, f"{label} {name}")
        if flags:
            assert (cls == 2).all()
        elif counts is not None and not fragile.any():
            assert U.class_counts(cls) == counts, label
    if (w, h) == (lw, lh):          # the identity: bit for bit without albedo, every pixel class 0
        cls = np.zeros((h, w), np.int32) - 1
        got = gpu.upsample_host(color, U.without_albedo(low), U.without_albedo(high), class_out=cls)
        assert np.array_equal(_bits(got[..., :3]), _bits(color[..., :3])) and (cls == 0).all()


def test_every_class_occurs(gpu, rendered):
    seen = np.zeros(3, np.int64)
    for label, (color, low, high) in rendered.items():
        cls = np.zeros(high["id"].shape, np.int32)
        gpu.upsample_host(color, low, high, class_out=cls)
        seen += np.bincount(cls.ravel(), minlength=3)[:3]
    print(f"classes over the rendered cases: {seen.tolist()}")
    assert (seen > 0).all()


@pytest.mark.parametrize("case", U.DESIGNED_CASES)
def test_designed_cases(gpu, case):
    """The designed cases (tests/test_upsample_cpu.py holds their branches), with and without albedo
    and under the flag."""
    color, low, high, expect = U.designed_inputs(case)
    for name, lo, hi, flags in _variants(low, high):
        cls, fragile = _check(gpu, color, lo, hi, flags, TOL_DESIGNED, f"{case} {name}")
        assert not fragile.any()
        if not flags and "cls" in expect:
            mask, value = expect["cls"]
            value = np.asarray(value)
            assert np.array_equal(cls[mask], np.broadcast_to(value[mask] if value.shape == mask.shape else value,
                                                             cls[mask].shape))


@pytest.mark.parametrize("label", ["67x45 from 33x22", "1x1 from 1x1"], ids=["67x45", "1x1"])
def test_contract(gpu, rendered, label):
    """Host, device and tensor forms give the same bits; of out only the rgb is written; class_out is
    optional and changes nothing; 64 sentinel words behind each output stay; every input is
    unchanged; a refused call writes nothing."""
    import torch
    L = gpu._lib
    dev = torch.device("cuda:0")
    color, low, high = rendered[label]
    h, w = high["id"].shape
    inputs = (color, *low.values(), *high.values())
    keep = [a.copy() for a in inputs]
    hout, hcls = np.full((h, w, 4), SENTINEL, np.float32), np.full((h, w), 9, np.int32)
    assert gpu.upsample_host(color, low, high, out=hout, class_out=hcls) is hout
    for a, b in zip(inputs, keep):
        assert np.array_equal(_bits(a), _bits(b))
    assert (hout[..., 3] == SENTINEL).all() and np.isfinite(hout).all() and ((hcls >= 0) & (hcls <= 2)).all()
    nocls = gpu.upsample_host(color, low, high)                      # class_out is optional; a fresh call, the same bits
    assert np.array_equal(_bits(nocls[..., :3]), _bits(hout[..., :3]))
    # the tensor form: both outputs with a guard behind them, on a stream of its own
    up = lambda d: {k: torch.from_numpy(v).to(dev) for k, v in d.items()}   # noqa: E731
    tcolor, tlow, thigh = torch.from_numpy(color).to(dev), up(low), up(high)
    n = w * h
    tout = torch.full((4 * n + GUARD,), SENTINEL, device=dev)
    tcls = torch.full((n + GUARD,), 9, dtype=torch.int32, device=dev)
    st = torch.cuda.Stream(dev)
    st.wait_stream(torch.cuda.current_stream(dev))
    assert gpu.upsample_tensor(tcolor, tlow, thigh, out=tout, class_out=tcls, stream=st) is tout
    st.synchronize()
    t, c = tout.cpu().numpy(), tcls.cpu().numpy()
    assert np.array_equal(_bits(t[:4 * n]), _bits(hout).ravel())     # (the sentinel alphas included)
    assert (t[4 * n:] == SENTINEL).all() and np.array_equal(c[:n], hcls.ravel()) and (c[n:] == 9).all()
    # the device entry point itself, without a class plane
    raw = torch.full((4 * n + GUARD,), SENTINEL, device=dev)
    d = gpu.upsample_desc(w, h, color.shape[1], color.shape[0])
    gl, gh = L.Gbuffer(), L.Gbuffer()
    for k in L.UPSAMPLE_NAMES:
        setattr(gl, k, tlow[k].data_ptr())
        setattr(gh, k, thigh[k].data_ptr())
    torch.cuda.synchronize()
    assert L.lib().lrt_upsample_device(ctypes.byref(d), tcolor.data_ptr(), ctypes.byref(gl), ctypes.byref(gh),
                                       raw.data_ptr(), None, None) == 0
    torch.cuda.synchronize()
    assert np.array_equal(_bits(raw.cpu().numpy()), _bits(t))
    for tt, a in zip((tcolor, *tlow.values(), *thigh.values()), keep):   # the inputs on the device
        assert np.array_equal(_bits(tt.cpu().numpy()), _bits(a))
    # a refused call writes nothing: an output on an input, albedo on one side, an unknown flag
    for bad in (dict(out=thigh["normal"]), dict(low=U.without_albedo(tlow)), dict(flags=2), dict(weight_min=0.0),
                dict(class_out=thigh["id"])):
        a = dict(low=tlow, high=thigh, out=tout, class_out=tcls)
        a.update(bad)
        with pytest.raises(gpu.LrtError) as e:
            gpu.upsample_tensor(tcolor, a.pop("low"), a.pop("high"), **a)
        assert e.value.code == L.LRT_E_INVALID
    torch.cuda.synchronize()
    assert np.array_equal(_bits(tout.cpu().numpy()), _bits(t)) and np.array_equal(tcls.cpu().numpy(), c)
    for tt, a in zip((tcolor, *tlow.values(), *thigh.values()), keep):
        assert np.array_equal(_bits(tt.cpu().numpy()), _bits(a))


def test_state_after_shutdown(gpu, rendered):
    """Without lrt_initialize(): LRT_E_STATE (tests/test_gpu_gbuffer.py shuts down and comes back the
    same way)."""
    L = gpu._lib
    color, low, high = rendered["1x1 from 1x1"]
    gpu.ShutdownTest()
    try:
        with pytest.raises(gpu.LrtError) as e:
            gpu.upsample_host(color, low, high)
        assert e.value.code == L.LRT_E_STATE
    finally:
        gpu.InitializeTest()
    assert np.isfinite(gpu.upsample_host(color, low, high)).all()


def test_silhouettes_at_full_resolution(gpu, rendered):
    """What it is for, derivable: at 66 x 44 from 33 x 22 on the default scene colour the low frame by
    id, color_low = palette[id_low + 1], no albedo planes. Every pixel is class 0, so the guided form
    returns palette[id_high + 1] at EVERY pixel within TOL; the flag form differs from that at the
    pixels that have a tap of another id (748, counted on the CPU): at more than 500 of them, and at
    none of the pixels whose four taps all carry the pixel's own id."""
    _, low, high = rendered["66x44 from 33x22"]
    low, high = U.without_albedo(low), U.without_albedo(high)
    palette = np.random.default_rng(1).uniform(0.1, 1.0, (10, 3)).astype(np.float32)
    color = U.quad(palette[low["id"] + 1])
    want = palette[high["id"] + 1]
    cls = np.zeros(high["id"].shape, np.int32) - 1
    guided = gpu.upsample_host(color, low, high, class_out=cls)[..., :3]
    assert (cls == 0).all()
    gap = R.rel_gap(guided, want)
    print(f"guided against the palette: {gap:.3g} (bound {TOL:.3g})")
    assert gap <= TOL
    flag = gpu.upsample_host(color, low, high, flags=U.UP_BILINEAR)[..., :3]
    other = U.other_sphere_taps(low["id"], high["id"])
    differs = (np.abs(np.float64(flag) - want) > TOL * np.maximum(1, np.abs(want))).any(-1)
    print(f"pixels with a tap of another sphere: {int(other.sum())}; the flag form differs at {int(differs.sum())}")
    assert differs.sum() > 500 and not differs[~other].any()


def test_through_the_chain(gpu):
    """svgf_filter_tensor's output at 33 x 22 (pool render, G-buffer, step_gbuffer, filter) goes into
    upsample_tensor with gbuffer_tensor planes at both sizes: finite everywhere, and the host form's
    bits."""
    import torch
    dev = torch.device("cuda:0")
    (w, h), (lw, lh) = (66, 44), (33, 22)
    cam = gpu.default_camera(w, h)
    buf = torch.zeros((lh, lw, 4), device=dev)
    rays = torch.zeros(1, dtype=torch.int64, device=dev)
    gpu.render_tensor(gpu.Job(width=lw, height=lh, frames=4, max_depth=8, camera=cam, flags=POOL), buf, rays)
    acc = gpu.TemporalAccumulator(lw, lh, dev)
    low = gpu.gbuffer_tensor(lw, lh, cam, out=acc.gbuffer_planes())
    acc.step_gbuffer(buf, low)
    st = acc.state
    filtered = gpu.svgf_filter_tensor(st["color"], st["moment2"], {k: low[k] for k in ("normal", "world_pos", "albedo")})
    high = gpu.gbuffer_tensor(w, h, cam, id=True)
    cls = torch.zeros((h, w), dtype=torch.int32, device=dev)
    out = gpu.upsample_tensor(filtered, low, high, class_out=cls)
    torch.cuda.synchronize()
    assert out.shape == (h, w, 4) and torch.isfinite(out).all() and (cls == 0).all()
    host = gpu.upsample_host(filtered.cpu().numpy(), {k: low[k].cpu().numpy() for k in ("id", "normal", "albedo")},
                             {k: high[k].cpu().numpy() for k in ("id", "normal", "albedo")})
    assert np.array_equal(_bits(out.cpu().numpy()), _bits(host))


def test_refused_taps_may_hold_anything(gpu):
    """The `ring` case with NaN and Inf as the colours of the other sphere's low pixels
    (upsample_ref.nonfinite_inputs): a tap that does not count adds nothing, so the guided form is
    finite everywhere, within TOL_DESIGNED of the restatement, and the bits of the run with those
    colours zeroed, with albedo and without."""
    color, zeroed, low, high = U.nonfinite_inputs()
    for name, lo, hi in (("albedo", low, high), ("plain", U.without_albedo(low), U.without_albedo(high))):
        cls, wcls = np.zeros(high["id"].shape, np.int32) - 1, np.zeros(high["id"].shape, np.int32) - 1
        got = gpu.upsample_host(color, lo, hi, class_out=cls)
        same = gpu.upsample_host(zeroed, lo, hi, class_out=wcls)
        want, rcls, fragile = U.upsample(color, lo, hi, np.float64)
        assert np.isfinite(got).all() and not fragile.any()
        assert np.array_equal(_bits(got), _bits(same)) and np.array_equal(cls, wcls) and np.array_equal(cls, rcls)
        gap = R.rel_gap(got[..., :3], want)
        print(f"non-finite refused taps, {name}: gap {gap:.3g} (bound {TOL_DESIGNED:.3g}), classes {U.class_counts(cls)}")
        assert gap <= TOL_DESIGNED
