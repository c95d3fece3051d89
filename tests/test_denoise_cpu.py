"""The denoiser's host-side contract (no GPU): argument validation and defaults of the C-ABI
(lrt_denoise_*), and the specified filter itself -- its NumPy restatement (tests/denoise_ref.py)
on the oracle's 4 spp render with features against the oracle's 1024 spp render, plus sanity
checks of the restatement the GPU tests compare the kernel with."""
import ctypes
import os

import numpy as np
import pytest

import denoise_ref as R
import oracle
from learnraytracing_amd import _lib as L


def _gpu_present():
    import torch
    return torch.cuda.device_count() > 0


def test_denoise_validation_before_device_use():
    """Every invalid argument is LRT_E_INVALID, a valid call without lrt_initialize() LRT_E_STATE:
    no GPU needed for either, host and device entry points alike."""
    lib = L.lib()
    w, h = 16, 9
    color = np.zeros((h, w, 4), np.float32)
    out = np.zeros((h, w, 4), np.float32)
    guide = np.zeros((h, w, 4), np.float32)
    ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)   # noqa: E731

    def desc(**kw):
        d = L.DenoiseDesc()
        assert lib.lrt_denoise_default(w, h, ctypes.byref(d)) == 0
        for k, v in kw.items():
            setattr(d, k, v)
        return d

    def calls(d, c, g, o):
        dp = ctypes.byref(d) if d is not None else None
        gp = ctypes.byref(g) if g is not None else None
        return (lib.lrt_denoise_host(dp, c, gp, o), lib.lrt_denoise_device(dp, c, gp, o, None))

    inv = (L.LRT_E_INVALID, L.LRT_E_INVALID)
    assert calls(None, ptr(color), None, ptr(out)) == inv
    assert calls(desc(), None, None, ptr(out)) == inv
    assert calls(desc(), ptr(color), None, None) == inv
    for bad in (dict(width=0), dict(height=0), dict(width=-3), dict(iterations=0),
                dict(iterations=L.DENOISE_MAX_ITER + 1), dict(iterations=-1), dict(flags=1)):
        assert calls(desc(**bad), ptr(color), None, ptr(out)) == inv, bad
    for name in ("sigma_color", "sigma_normal", "sigma_pos", "sigma_albedo"):
        for v in (0.0, -1.0, float("inf"), float("nan")):
            assert calls(desc(**{name: v}), ptr(color), None, ptr(out)) == inv, (name, v)
    for name in L.GUIDE_NAMES:   # out may not be a guide buffer
        g = L.Features()
        setattr(g, name, guide.ctypes.data)
        assert calls(desc(), ptr(color), g, ptr(guide)) == inv, name
    assert "guide" in lib.lrt_last_error().decode()
    if os.environ.get("HIP_VISIBLE_DEVICES") == "" or not _gpu_present():
        g = L.Features()
        g.normal = guide.ctypes.data
        assert calls(desc(), ptr(color), g, ptr(out)) == (L.LRT_E_STATE, L.LRT_E_STATE)
        assert calls(desc(), ptr(color), None, ptr(color)) == (L.LRT_E_STATE, L.LRT_E_STATE)   # in place is valid


def test_denoise_default_desc():
    lib = L.lib()
    assert ctypes.sizeof(L.DenoiseDesc) == 32
    d = L.DenoiseDesc()
    assert lib.lrt_denoise_default(1280, 720, ctypes.byref(d)) == 0
    assert (d.width, d.height, d.iterations, d.flags) == (1280, 720, 5, 0)
    assert L.DENOISE_MAX_ITER == 5 == R.DEFAULTS["iterations"]
    for name in ("sigma_color", "sigma_normal", "sigma_pos", "sigma_albedo"):
        assert getattr(d, name) == np.float32(R.DEFAULTS[name]), name
    assert (R.DEFAULTS["sigma_color"], R.DEFAULTS["sigma_normal"], R.DEFAULTS["sigma_pos"],
            R.DEFAULTS["sigma_albedo"]) == (2.0, 0.3, 0.5, 0.2)
    assert lib.lrt_denoise_default(1280, 720, None) == L.LRT_E_INVALID
    assert lib.lrt_denoise_default(0, 720, ctypes.byref(d)) == L.LRT_E_INVALID


def test_python_front_end_rejects_bad_arguments():
    from learnraytracing_amd import LrtError, denoise_host
    color = np.zeros((9, 16, 4), np.float32)
    with pytest.raises(LrtError):
        denoise_host(color, {"depth": color.copy()})
    with pytest.raises(LrtError):
        denoise_host(color, None, sigma=1.0)
    with pytest.raises(LrtError):
        denoise_host(color.ravel(), None)
    with pytest.raises(LrtError):
        denoise_host(color, {"normal": np.zeros((9, 16, 3), np.float32)})


def test_front_end_message_names_the_offending_argument():
    """The checks the front ends share name the argument that failed, whichever unit it reached."""
    from learnraytracing_amd import LrtError, denoise_host, svgf_filter_host
    color = np.zeros((9, 16, 4), np.float32)
    with pytest.raises(LrtError) as e:
        denoise_host(color, None, out=np.zeros((9, 16, 4), np.float64))
    assert e.value.code == L.LRT_E_INVALID and "out must be" in str(e.value) and "float32" in str(e.value)
    with pytest.raises(LrtError) as e:
        denoise_host(color, {"albedo": color[:8]})
    assert e.value.code == L.LRT_E_INVALID and "albedo must be" in str(e.value) and ">= 576" in str(e.value)
    with pytest.raises(LrtError) as e:
        svgf_filter_host(color, color.copy(), None, variance_out=color[:, :, :3])
    assert e.value.code == L.LRT_E_INVALID and "variance_out must be" in str(e.value)


def test_every_tensor_front_end_rejects_a_host_array():
    """A NumPy array where a post-process *_tensor front end keys on a cuda tensor is LRT_E_INVALID, before
    any use of the device: not an AttributeError, and never a pointer handed to the library."""
    import learnraytracing_amd as lrt
    w, h = 16, 9
    q, low = np.zeros((h, w, 4), np.float32), np.zeros((5, 8, 4), np.float32)
    ids, low_ids = np.zeros((h, w), np.int32), np.zeros((5, 8), np.int32)
    cam = lrt.default_camera(w, h)
    g = {"normal": q, "motion": q, "id": ids}
    gl = {"normal": low, "id": low_ids}
    job = lrt.Job(width=w, height=h)
    calls = {
        "denoise": lambda: lrt.denoise_tensor(q, None),
        "temporal_accumulate": lambda: lrt.temporal_accumulate_tensor(q, {"normal": q, "world_pos": q}, None, cam),
        "temporal_accumulate_moving": lambda: lrt.temporal_accumulate_moving_tensor(
            q, {"normal": q, "world_pos": q}, None, cam, None, [[0, 0, 0, 1]], [[0, 0, 0, 1]]),
        "temporal_accumulate_gbuffer": lambda: lrt.temporal_accumulate_gbuffer_tensor(q, g, None, None),
        "temporal_rectify": lambda: lrt.temporal_rectify_tensor(q, ids, {"color": q, "moment2": q}),
        "svgf_filter": lambda: lrt.svgf_filter_tensor(q, q, None),
        "tonemap": lambda: lrt.tonemap_tensor(q),
        "gbuffer": lambda: lrt.gbuffer_tensor(w, h, cam, out={"normal": q}),
        "gbuffer_chain": lambda: lrt.gbuffer_chain_tensor(w, h, cam, out={"key": ids}),
        "gbuffer_chain_motion": lambda: lrt.gbuffer_chain_motion_tensor(w, h, cam, None, q),
        "upsample": lambda: lrt.upsample_tensor(low, gl, g),
        "temporal_upsample": lambda: lrt.temporal_upsample_tensor(low, gl, g, None, None),
        "sample_budget": lambda: lrt.sample_budget_tensor(q, 1, 8, 600),
        "render_counts": lambda: lrt.render_counts_tensor(job, q, np.zeros(1, np.int64), ids, None),
        "firefly": lambda: lrt.firefly_tensor(q, ids),
        "firefly_restore": lambda: lrt.firefly_restore_tensor(q, q, ids),
    }
    assert sorted(n + "_tensor" for n in calls) == sorted(
        n for n in dir(lrt) if n.endswith("_tensor") and n != "render_tensor")
    for name, call in calls.items():
        with pytest.raises(lrt.LrtError) as e:
            call()
        assert e.value.code == L.LRT_E_INVALID and "cuda" in str(e.value), name


def test_filter_quality_on_reference_render():
    """The specified filter earns its place: on the oracle's 160x90, 4 spp, depth 8 render with
    features, the f64 restatement with the defaults brings the MSE against the 1024 spp render to
    <= 0.5x and the relative MSE to <= 0.1x of the noisy frame's (measured: 0.35x, 0.040x)."""
    w, h = 160, 90
    feats = {n: np.zeros((h, w, 4), np.float32) for n in oracle.FEATURE_NAMES}
    noisy, _ = oracle.orc_render_ex(w, h, frames=4, depth=8, features=feats, max_frame=4)
    gt, _ = oracle.orc_render(w, h, frames=1024, depth=8)
    guides = {n: feats[n] for n in L.GUIDE_NAMES}
    got = R.atrous(noisy, guides, np.float64)
    m0, m1 = R.mse(noisy, gt), R.mse(got, gt)
    r0, r1 = R.rel_mse(noisy, gt), R.rel_mse(got, gt)
    print(f"MSE {m0:.4g} -> {m1:.4g} ({m1 / m0:.3f}x), relMSE {r0:.4g} -> {r1:.4g} ({r1 / r0:.4f}x)")
    assert m1 <= 0.5 * m0
    assert r1 <= 0.1 * r0


def test_restatement_constant_image_stays_constant():
    color, guides = R.synthetic_inputs(37, 21)
    color[..., :3] = np.float32([0.25, 1.5, 3.0])
    for names in R.GUIDE_SETS.values():
        got = R.atrous(color, {k: guides[k] for k in names}, np.float64)
        assert np.abs(got - np.float64(color[..., :3])).max() <= 1e-12, names


def test_restatement_orthogonal_half_planes_do_not_mix():
    """Two half-planes with orthogonal normals, sigma_normal 0.1: |dn|^2 / sigma^2 = 200, the
    cross weights are exp(-200) ~ 1e-87 -- zero against the same-side weights in f64 too -- so
    each side's output is a mean of its own side only."""
    w, h = 48, 20
    color = np.zeros((h, w, 4), np.float32)
    color[:, : w // 2, :3] = 1.0
    color[:, w // 2:, :3] = 3.0
    normal = np.zeros((h, w, 4), np.float32)
    normal[:, : w // 2, 1] = 1.0
    normal[:, w // 2:, 0] = 1.0
    for dtype in (np.float32, np.float64):
        got = R.atrous(color, {"normal": normal}, dtype, sigma_normal=0.1)
        assert np.array_equal(got, color[..., :3].astype(dtype))
    mixed = R.atrous(color, None, np.float64)   # and without the guide they do mix
    assert 1.0 < mixed[h // 2, w // 2 - 1, 0] < 3.0


def test_restatement_null_guides_drop_their_terms():
    color, guides = R.synthetic_inputs(40, 24)
    none = R.atrous(color, None, np.float64, iterations=3)
    assert np.array_equal(none, R.atrous(color, {}, np.float64, iterations=3))
    assert np.array_equal(none, R.atrous(color, {"normal": None, "color_std": None}, np.float64, iterations=3))
    # an unguided pass is the plain B3-spline blur, renormalised at the border
    one = R.atrous(color, None, np.float64, iterations=1)
    c = np.float64(color[..., :3])
    y, x = 12, 20
    k = np.outer(R.H5, R.H5)
    assert np.allclose(one[y, x], (k[..., None] * c[y - 2:y + 3, x - 2:x + 3]).sum((0, 1)), rtol=1e-13)
    k00 = k[2:, 2:]
    assert np.allclose(one[0, 0], (k00[..., None] * c[:3, :3]).sum((0, 1)) / k00.sum(), rtol=1e-13)
    # each guide changes the result, and a term scales with its sigma only
    for name in L.GUIDE_NAMES:
        assert not np.array_equal(none, R.atrous(color, {name: guides[name]}, np.float64, iterations=3)), name
    a = R.atrous(color, {"normal": guides["normal"]}, np.float64, sigma_pos=0.01, sigma_albedo=7.0, sigma_color=9.0)
    assert np.array_equal(a, R.atrous(color, {"normal": guides["normal"]}, np.float64))


SYNTHETIC_67x45_SHA256 = dict(          # the first 16 hex digits, from before synthetic_inputs took variant=
    color="2bb1ff2d8af43b53", albedo="62fa4bcf6e119588", color_std="d09e2577683e6718",
    normal="b8566b37d1ca083c", world_pos="b7e0acce522f24a7")
F32_F64_GAP_EDGE = 9.9e-7               # tests/test_gpu_denoise.py's


def test_synthetic_inputs_default_is_unchanged():
    import hashlib
    color, guides = R.synthetic_inputs(67, 45)
    for name, a in dict(guides, color=color).items():
        assert a.dtype == np.float32 and a.shape == (45, 67, 4)
        assert hashlib.sha256(a.tobytes()).hexdigest()[:16] == SYNTHETIC_67x45_SHA256[name], name
    again, _ = R.synthetic_inputs(67, 45, variant=None)
    assert np.array_equal(again, color)
    with pytest.raises(ValueError):
        R.synthetic_inputs(67, 45, variant="nope")


def test_edge_table_is_what_the_gpu_test_quotes():
    sweeps = R.edge_sweeps()
    table = R.edge_table()
    assert 50 <= len(table) <= 150 and len(table) == sum(len(c) for c in sweeps.values())
    assert {(c["w"], c["h"]) for c in table} == set(R.EDGE_SHAPES) | {R.EDGE_BASE, R.EDGE_WIDE}
    w, h = R.EDGE_WIDE           # more workgroups than 256 CUs x 8 hold, the second row group's far behind the first's
    assert sweeps["wide"][0]["params"]["iterations"] == 5 and h > 32 and (w // 64) * 8 >= 2048
    for w, h in R.EDGE_SHAPES:
        assert [c["params"]["iterations"] for c in sweeps[f"shape_{w}x{h}"]] == [3, 4, 5]
    assert sorted(c["guides"] for c in sweeps["guides"]) == sorted(
        [(g,) for g in L.GUIDE_NAMES] + [tuple(n for n in R.GUIDE_SETS["all"] if n != g) for g in L.GUIDE_NAMES])
    assert len(set(R.EDGE_SIGMAS_ALL.values())) == 4 and set(R.EDGE_SIGMAS_ALL) == set(R.SIGMAS)
    assert [c["variant"] for c in sweeps["variants"]] == list(R.VARIANTS)
    assert len(R.default_table()) == len(R.SHAPES) * len(R.ITERATIONS) * len(R.GUIDE_SETS)


@pytest.mark.parametrize("variant", R.VARIANTS)
def test_variant_inputs_and_their_restatement(variant):
    """Each variant is what it says, touches nothing else, and the f32 restatement of it is finite
    and within the recorded gap of the f64 one."""
    w, h = R.EDGE_BASE
    base_c, base_g = R.synthetic_inputs(w, h)
    color, guides = R.synthetic_inputs(w, h, variant=variant)
    changed = {"std_extremes": "color_std", "fireflies": "color", "far_origin": "world_pos"}.get(variant)
    for name, a in dict(guides, color=color).items():
        b = dict(base_g, color=base_c)[name]
        if name != changed:
            assert np.array_equal(a[..., :3], b[..., :3]), name
        if variant != "dirty_alpha" or name == "color":
            assert np.array_equal(a[..., 3], b[..., 3]), name
    if variant == "std_extremes":
        std = guides["color_std"][..., :3]
        zero, big = (std == 0).all(-1), (std == np.float32(1e3)).all(-1)
        assert 0.25 < zero.mean() < 0.42 and 0.25 < big.mean() < 0.42 and not (zero & big).any()
        assert np.array_equal(std[~(zero | big)], base_g["color_std"][..., :3][~(zero | big)])
    elif variant == "fireflies":
        hot = (color[..., :3] > 4).all(-1)
        assert hot.sum() == 6 and (color[..., :3] == 65504.0).all(-1).sum() == 1
        assert ((color[..., :3] == 1e4).all(-1)).sum() == 5
    elif variant == "dirty_alpha":
        for name, g in guides.items():
            al = g[..., 3]
            assert np.isnan(al).sum() > 100 and np.isposinf(al).sum() > 100 and (al == np.float32(1e30)).sum() > 100, name
        assert np.isfinite(color).all()
    else:
        shift = guides["world_pos"][..., :3] - base_g["world_pos"][..., :3]
        assert np.abs(shift - np.float32(R.FAR_ORIGIN)).max() <= 1e-4          # (the f32 sum rounds at 6e-5)
    a32 = R.atrous(color, guides, np.float32)
    a64 = R.atrous(color, guides, np.float64)
    assert a32.dtype == np.float32 and np.isfinite(a32).all() and np.isfinite(a64).all()
    assert R.rel_gap(a32, a64) <= F32_F64_GAP_EDGE
    if variant == "dirty_alpha":
        assert np.array_equal(a64, R.atrous(base_c, base_g, np.float64))


def test_denoise_bench_byte_count():
    """tools/denoise_bench.py's bytes per pass, from the tile geometry: a frame of exactly one tile
    stages itself once; a large frame stages ~2.1x (s = 1) to ~4x (s = 16) its pixels; never less
    than the compulsory 64 B per pixel."""
    import importlib.util
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("denoise_bench", os.path.join(root, "tools", "denoise_bench.py"))
    B = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(B)
    assert B.pass_bytes(64, 4, 1, False) == 64 * 4 * (64 + 16 + 16)
    assert B.pass_bytes(64, 4, 1, True) == 64 * 4 * (64 + 16 + 12)
    w, h = 1280, 720
    for s, lo, hi in ((1, 2.0, 2.2), (16, 3.5, 4.0)):
        staged = (B.pass_bytes(w, h, s, False) - w * h * 32) / 64 / (w * h)
        assert lo <= staged <= hi, (s, staged)
        assert B.pass_bytes(w, h, s, True) >= B.MIN_BYTES_PER_PIXEL * w * h
    with pytest.raises(SystemExit):
        B.main(["--reps", "5"])
