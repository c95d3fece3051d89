"""The variance-guided filter's host-side contract (no GPU): argument validation and defaults of
the C-ABI (lrt_svgf_*), the Python front end's argument checks, and the specified filter itself --
its NumPy restatement (tests/svgf_ref.py) in f64: properties that follow from the formulas, and what
it is for (the accumulated orbit of tests/test_temporal_cpu.py, filtered, against the oracle's
1024 spp frame, beside the existing temporal -> lrt_denoise path)."""
import ctypes
import importlib.util
import os

import numpy as np
import pytest

import denoise_ref as DR
import oracle
import svgf_ref as R
import temporal_ref as TR
from learnraytracing_amd import LrtError, _lib as L
from learnraytracing_amd import make_camera, svgf_desc, svgf_filter_host, svgf_filter_tensor

CUR = ("normal", "world_pos", "albedo")


def _gpu_present():
    import torch
    return torch.cuda.device_count() > 0


# ---- the C-ABI
def test_svgf_validation_before_device_use():
    """Every invalid argument is LRT_E_INVALID, a valid call without lrt_initialize() LRT_E_STATE:
    no GPU needed for either, host and device entry points alike."""
    lib = L.lib()
    w, h = 16, 9
    bufs = [np.zeros((h, w, 4), np.float32) for _ in range(7)]
    color, m2, nrm, pos, alb, out, var = (b.ctypes.data for b in bufs)

    def desc(**kw):
        d = L.SvgfDesc()
        assert lib.lrt_svgf_default(w, h, ctypes.byref(d)) == 0
        for k, v in kw.items():
            setattr(d, k, v)
        return d

    def features(**kw):
        f = L.Features()
        for k, v in dict(dict(normal=nrm, world_pos=pos, albedo=alb), **kw).items():
            setattr(f, k, v)
        return f

    def calls(d, c, m, g, o, v):
        ref = lambda x: ctypes.byref(x) if x is not None else None   # noqa: E731
        return (lib.lrt_svgf_filter_host(ref(d), c, m, ref(g), o, v),
                lib.lrt_svgf_filter_device(ref(d), c, m, ref(g), o, v, None))

    inv = (L.LRT_E_INVALID, L.LRT_E_INVALID)
    good = (desc(), color, m2, features(), out, var)
    assert calls(None, *good[1:]) == inv
    assert calls(good[0], None, *good[2:]) == inv
    assert calls(*good[:2], None, *good[3:]) == inv
    assert calls(*good[:4], None, var) == inv
    for bad in (dict(width=0), dict(height=0), dict(width=-3), dict(width=46341, height=46341), dict(iterations=0),
                dict(iterations=L.SVGF_MAX_ITER + 1), dict(iterations=-1), dict(flags=1), dict(reserved=1),
                dict(min_history=0), dict(min_history=-2)):
        assert calls(desc(**bad), *good[1:]) == inv, bad
    for name in ("sigma_color", "sigma_normal", "sigma_pos", "albedo_floor"):
        for v in (0.0, -1.0, float("inf"), -float("inf"), float("nan")):
            assert calls(desc(**{name: v}), *good[1:]) == inv, (name, v)
    # aliasing: out may be color itself and nothing else; variance_out nothing at all
    for p in (m2, nrm, pos, alb, color + 16, color - 16, m2 + 16):
        assert calls(*good[:4], p, var) == inv, "out"
    assert "alias" in lib.lrt_last_error().decode()
    for p in (color, m2, nrm, pos, alb, out, out + 16, color + 16):
        assert calls(*good[:5], p) == inv, "variance_out"
    assert calls(*good[:4], color, color) == inv                      # in place, and variance_out on it too
    if os.environ.get("HIP_VISIBLE_DEVICES") == "" or not _gpu_present():
        st = (L.LRT_E_STATE, L.LRT_E_STATE)
        assert calls(*good) == st
        assert calls(*good[:4], color, var) == st                      # in place is valid
        assert calls(*good[:5], None) == st                            # no variance_out
        assert calls(*good[:3], None, out, var) == st                  # no guides
        for name in CUR:
            assert calls(*good[:3], features(**{name: None}), out, var) == st, name
        assert calls(desc(iterations=1, min_history=100), *good[1:]) == st
        # a guide member the filter does not read may be anything, out included
        assert calls(*good[:3], features(color_std=out, normal_std=var), out, var) == st


def test_svgf_default_desc():
    lib = L.lib()
    assert ctypes.sizeof(L.SvgfDesc) == 40
    assert L.SvgfDesc.min_history.offset == 16 and L.SvgfDesc.sigma_color.offset == 24
    d = L.SvgfDesc()
    assert lib.lrt_svgf_default(1280, 720, ctypes.byref(d)) == 0
    assert (d.width, d.height, d.iterations, d.flags, d.min_history, d.reserved) == (1280, 720, 5, 0, 4, 0)
    assert L.SVGF_MAX_ITER == 5 == R.DEFAULTS["iterations"]
    for name in ("sigma_color", "sigma_normal", "sigma_pos", "albedo_floor"):
        assert getattr(d, name) == np.float32(R.DEFAULTS[name]), name
    assert {k: R.DEFAULTS[k] for k in ("min_history", "sigma_normal", "sigma_pos", "albedo_floor")} == \
        dict(min_history=4, sigma_normal=0.3, sigma_pos=0.5, albedo_floor=0.01)
    assert R.DEFAULTS["sigma_color"] in (1.0, 2.0, 4.0, 8.0)
    assert set(L.SVGF_PARAMS) == set(R.DEFAULTS)
    assert lib.lrt_svgf_default(1280, 720, None) == L.LRT_E_INVALID
    assert lib.lrt_svgf_default(0, 720, ctypes.byref(d)) == L.LRT_E_INVALID
    assert lib.lrt_svgf_default(1280, -1, ctypes.byref(d)) == L.LRT_E_INVALID


def test_python_front_end_rejects_bad_arguments():
    z = lambda: np.zeros((9, 16, 4), np.float32)   # noqa: E731
    color, m2 = z(), z()
    assert svgf_desc(16, 9, min_history=2, sigma_color=1.5, iterations=3).min_history == 2
    with pytest.raises(LrtError):
        svgf_desc(16, 9, sigma_albedo=1.0)
    with pytest.raises(LrtError):
        svgf_filter_host(color, m2, {"depth": z()})
    with pytest.raises(LrtError):
        svgf_filter_host(color, m2, None, sigma=1.0)
    with pytest.raises(LrtError):
        svgf_filter_host(color.ravel(), m2, None)
    with pytest.raises(LrtError):
        svgf_filter_host(color, m2[:4], None)
    with pytest.raises(LrtError):
        svgf_filter_host(color, m2.astype(np.float64), None)
    with pytest.raises(LrtError):
        svgf_filter_host(color, m2, {"normal": np.zeros((9, 16, 3), np.float32)})
    with pytest.raises(LrtError):
        svgf_filter_host(color, m2, None, variance_out=np.zeros((9, 16, 4), np.float64))
    with pytest.raises(LrtError) as e:   # the library's own check: an output that is an input
        svgf_filter_host(color, m2, None, out=m2)
    assert e.value.code == L.LRT_E_INVALID
    with pytest.raises(LrtError):        # host arrays are not tensors
        svgf_filter_tensor(color, m2, None)
    from learnraytracing_amd import TemporalAccumulator
    assert isinstance(TemporalAccumulator.state, property) and TemporalAccumulator.state.fset is None


# ---- the restatement, in f64
def _state(w, h, C, var, n):
    """color and moment2 = C^2 + var with history n, as f64 [h, w, 4] buffers."""
    color, m2 = np.zeros((h, w, 4)), np.zeros((h, w, 4))
    color[..., :3] = C
    m2[..., :3] = color[..., :3] ** 2 + var
    m2[..., 3] = n
    return color, m2


def test_restatement_constant_colour_and_variance():
    """(a) Constant colour, constant variance v, unguided, one pass: every weight is h[i] h[j], so an
    interior pixel keeps its colour and its variance becomes v (sum h^2)^2 = v (70/256)^2."""
    v = 0.37
    color, m2 = _state(21, 17, [0.25, 1.5, 3.0], v, 40.0)
    c, var = R.svgf(color, m2, None, np.float64, iterations=1)
    assert np.abs(c - color[..., :3]).max() <= 1e-12
    assert np.abs(var[2:-2, 2:-2] - v * (70 / 256) ** 2).max() <= 1e-12
    assert (var[0, 0] > v * (70 / 256) ** 2).all()        # fewer taps at the border: less averaging


def test_restatement_min_history_only_matters_below_it():
    """(b) With n >= min_history everywhere the result does not depend on min_history."""
    color, m2, g = R.synthetic_inputs(37, 21, variant="n40")
    a = R.svgf(color, m2, g, np.float64, min_history=4)
    b = R.svgf(color, m2, g, np.float64, min_history=1)
    c = R.svgf(color, m2, g, np.float64, min_history=40)
    d = R.svgf(color, m2, g, np.float64, min_history=41)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert np.array_equal(a[0], c[0]) and np.array_equal(a[1], c[1])
    assert not np.array_equal(a[1], d[1])                  # n < min_history: the spatial estimate


def test_restatement_spatial_estimate_of_a_constant():
    """(c) n = 1 everywhere, C = M = const: m1 = m2 = const, v = max(const - const^2, 0) min_history
    (iterations=0: stage 0 alone)."""
    for const, mh in ((0.5, 4), (0.25, 7), (2.0, 4)):
        color, m2 = _state(13, 9, const, 0.0, 1.0)
        m2[..., :3] = const
        c, var = R.svgf(color, m2, None, np.float64, iterations=0, min_history=mh)
        assert np.array_equal(c, color[..., :3])
        assert np.abs(var - max(const - const * const, 0.0) * mh).max() <= 1e-12, (const, mh)
    color, m2 = _state(13, 9, 0.5, 0.0, 2.0)               # n = 2: the boost is min_history / n
    m2[..., :3] = 0.5
    assert np.abs(R.svgf(color, m2, None, np.float64, iterations=0)[1] - 0.25 * 4 / 2).max() <= 1e-12


def test_restatement_unit_albedo_is_no_albedo():
    """(d) albedo = 1: D = 1, the same arrays as without albedo."""
    color, m2, g = R.synthetic_inputs(37, 21)
    g["albedo"][..., :3] = 1.0
    a = R.svgf(color, m2, g, np.float64)
    b = R.svgf(color, m2, {k: g[k] for k in ("normal", "world_pos")}, np.float64)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_restatement_demodulation_keeps_texture():
    """(e) The 7 x 5 block palette of denoise_ref as albedo times a smooth irradiance with noise: with
    albedo divided out the result is closer to albedo x clean irradiance than without; and under a
    constant irradiance nothing bleeds across a palette edge (c_0 is constant: the result is the
    texture itself), while the same frame without the albedo guide is blurred across the edges."""
    w, h = 56, 40
    _, g = DR.synthetic_inputs(w, h)
    A = np.float64(g["albedo"][..., :3])
    y, x = np.mgrid[0:h, 0:w]
    clean = (1.0 + 0.5 * np.sin(x / 9.0) * np.cos(y / 7.0))[..., None] * np.ones(3)
    rng = np.random.default_rng(3)
    sd = 0.3
    color, m2 = _state(w, h, A * (clean + rng.normal(0, sd, (h, w, 3))), (A * sd) ** 2, 40.0)
    with_a, _ = R.svgf(color, m2, {"albedo": g["albedo"]}, np.float64)
    without, _ = R.svgf(color, m2, None, np.float64)
    e1, e0 = DR.mse(with_a, A * clean), DR.mse(without, A * clean)
    print(f"MSE against albedo x clean irradiance: demodulated {e1:.4g}, not demodulated {e0:.4g}")
    assert e1 < 0.5 * e0
    flat, m2f = _state(w, h, A * 1.25, (A * sd) ** 2, 40.0)
    kept, _ = R.svgf(flat, m2f, {"albedo": g["albedo"]}, np.float64)
    bled, _ = R.svgf(flat, m2f, None, np.float64)
    assert np.abs(kept - A * 1.25).max() <= 1e-12
    assert np.abs(bled - A * 1.25).max() > 1e-2


def test_restatement_absent_guide_is_none():
    """(f) A guide passed as None is a guide left out; a name the filter does not read changes nothing."""
    color, m2, g = R.synthetic_inputs(19, 13)
    for names in R.GUIDE_SETS.values():
        a = R.svgf(color, m2, {k: g[k] for k in names}, np.float64)
        b = R.svgf(color, m2, {k: (g[k] if k in names else None) for k in g}, np.float64)
        c = R.svgf(color, m2, dict({k: g[k] for k in names}, color_std=color), np.float64)
        for u in (b, c):
            assert np.array_equal(a[0], u[0]) and np.array_equal(a[1], u[1]), names
    assert not np.array_equal(R.svgf(color, m2, g, np.float64)[0], R.svgf(color, m2, None, np.float64)[0])


def _by_hand(color, m2, K, mh, sc):
    """The unguided filter written out pixel by pixel, tap by tap, straight from include/lrt.h."""
    h, w = color.shape[:2]
    inside = lambda x, y: 0 <= x < w and 0 <= y < h   # noqa: E731
    c, var = np.zeros((h, w, 3)), np.zeros((h, w, 3))
    for y in range(h):
        for x in range(w):
            C, M, n = color[y, x, :3], m2[y, x, :3], m2[y, x, 3]
            if n >= mh:
                v = np.maximum(M - C * C, 0)
            else:
                taps = [(x + i, y + j) for j in range(-3, 4) for i in range(-3, 4) if inside(x + i, y + j)]
                m1 = sum(color[q, p, :3] for p, q in taps) / len(taps)
                mm = sum(m2[q, p, :3] for p, q in taps) / len(taps)
                v = np.maximum(mm - m1 * m1, 0) * (mh / max(n, 1))
            c[y, x], var[y, x] = C, v
    b, hh = (0.25, 0.5, 0.25), (1 / 16, 1 / 4, 3 / 8, 1 / 4, 1 / 16)
    for k in range(K):
        s = 2 ** k
        cn, vn = np.zeros_like(c), np.zeros_like(var)
        for y in range(h):
            for x in range(w):
                num = den = 0.0
                for j in range(-1, 2):
                    for i in range(-1, 2):
                        if inside(x + i, y + j):
                            num += b[i + 1] * b[j + 1] * var[y + j, x + i].sum()
                            den += b[i + 1] * b[j + 1]
                vt = num / den
                sw, swc, sw2v = 0.0, np.zeros(3), np.zeros(3)
                for j in range(-2, 3):
                    for i in range(-2, 3):
                        if inside(x + i * s, y + j * s):
                            q = (y + j * s, x + i * s)
                            e = ((c[y, x] - c[q]) ** 2).sum() / (sc * sc * vt + 1e-6)
                            wq = hh[i + 2] * hh[j + 2] * np.exp(-e)
                            sw += wq
                            swc += wq * c[q]
                            sw2v += wq * wq * var[q]
                cn[y, x], vn[y, x] = swc / sw, sw2v / (sw * sw)
        c, var = cn, vn
    return c, var


def test_restatement_taps_outside_the_image_are_skipped():
    """(g) A 1 x 1 frame has the centre tap alone: colour and variance pass through every pass; a 3 x 2
    frame against the filter written out tap by tap."""
    for n, want in ((40.0, 0.3), (1.0, 0.3 * 4), (2.5, 0.3 * 4 / 2.5)):
        color, m2 = _state(1, 1, [0.5, 1.0, 2.0], 0.3, n)
        for K in (1, 5):
            c, var = R.svgf(color, m2, None, np.float64, iterations=K)
            assert np.abs(c - color[..., :3]).max() <= 1e-15 and np.abs(var - want).max() <= 1e-12, (n, K)
    rng = np.random.default_rng(11)
    color, m2 = _state(3, 2, rng.uniform(0.1, 2.0, (2, 3, 3)), rng.uniform(0.05, 1.0, (2, 3, 3)), 40.0)
    m2[0, 1, 3], m2[1, 2, 3] = 1.0, 3.0                    # two short histories
    for K in (1, 2, 3):
        got = R.svgf(color, m2, None, np.float64, iterations=K, sigma_color=2.0)
        want = _by_hand(color, m2, K, 4, 2.0)
        assert np.abs(got[0] - want[0]).max() <= 1e-12 and np.abs(got[1] - want[1]).max() <= 1e-12, K


def test_synthetic_inputs_are_what_the_gpu_tests_need():
    """No pixel's |N|^2 lies within HIT_MARGIN of 0.25 in any case of either table, the variance is
    bounded below, every n of N_VALUES and a tenth of misses are there."""
    for c in R.default_table() + R.edge_table():
        if (c["w"], c["h"]) == R.EDGE_WIDE:
            continue                                       # unguided
        color, m2, g = R.case_inputs(c)
        assert R.hit_margin(g) >= R.HIT_MARGIN, R.case_label(c)
    color, m2, g = R.synthetic_inputs(160, 90)
    assert set(np.unique(m2[..., 3])) == set(R.N_VALUES.tolist())
    miss = (g["normal"][..., :3] == 0).all(-1)
    assert 0.08 <= miss.mean() <= 0.13 and (g["albedo"][..., :3][miss] == 0).all()
    var = np.float64(m2[..., :3]) - np.float64(color[..., :3]) ** 2
    assert var.min() >= 0.05 ** 2 * 0.99 and var.max() <= 1.01
    assert (R.synthetic_inputs(67, 45, variant="n1")[1][..., 3] == 1).all()
    assert (R.synthetic_inputs(67, 45, variant="n40")[1][..., 3] == 40).all()
    c0, m0, g0 = R.synthetic_inputs(67, 45, variant="var0")
    zero = (m0[..., :3] == c0[..., :3] ** 2).all(-1)
    assert 0.25 <= zero.mean() <= 0.42
    a0 = R.synthetic_inputs(67, 45, variant="albedo0")[2]
    hit = (a0["normal"][..., :3] != 0).any(-1)
    assert 0.2 <= ((a0["albedo"][..., :3] == 0).all(-1) & hit).mean() <= 0.4
    assert not np.isfinite(R.synthetic_inputs(67, 45, variant="dirty_alpha")[0][..., 3]).all()
    assert R.synthetic_inputs(67, 45, variant="fireflies")[0][..., :3].max() == 65504.0


# ---- what it is for
def _render(w, h, camera, frame0, depth=8):
    feats = {n: np.zeros((h, w, 4), np.float32) for n in CUR}
    buf, _ = oracle.orc_render_ex(w, h, frames=1, depth=depth, frame0=frame0, cam22=TR.cam22(camera),
                                  features=feats, max_frame=-1)
    return buf, feats


SIGMA_GRID = (1.0, 2.0, 4.0, 8.0)


def test_quality_of_filtered_orbit_and_sigma_grid():
    """tests/test_temporal_cpu.py's setup (160x90, depth 8, 16 steps of 1 spp along the orbit, 1024
    spp at the final camera): for steps of 0.02, 0 and 0.08 rad the new filter on the final state
    meets the bar the existing path has to meet, d_new <= BAR_DENOISED x d0 (d0: the filtered last
    single frame); the figures are printed beside the existing path's (denoise_ref.atrous with the
    temporal color_std) over the sigma_color grid, and the default sigma_color is the grid's best by
    the mean of the three relative MSEs (the grid: DESIGN 7.3)."""
    q = TR.QUALITY
    cam = make_camera(*TR.orbit_args(0.0, q["w"], q["h"]))
    gt, _ = oracle.orc_render(q["w"], q["h"], frames=q["gt_spp"], depth=q["depth"], cam22=TR.cam22(cam))
    grid = {sc: [] for sc in SIGMA_GRID}
    for dtheta in (0.02, 0.0, 0.08):
        frames = TR.orbit_frames(_render, make_camera, q["w"], q["h"], q["steps"], dtheta)
        out = TR.accumulate(frames, np.float64)
        color, feats, _, k = frames[-1]
        single = np.float64(color[..., :3]) * k
        guides1 = {n: np.float64(feats[n][..., :3]) * k for n in CUR}
        base = DR.atrous(single, dict(guides1, color_std=np.full_like(single, TR.DEFAULTS["short_std"])), np.float64)
        old = DR.atrous(out["color"], {n: out[n] for n in L.GUIDE_NAMES}, np.float64)
        d0, d_old = DR.rel_mse(base, gt), DR.rel_mse(old, gt)
        st = TR.as_state(out, np.float64)
        for sc in SIGMA_GRID:
            new, _ = R.svgf(st["color"], st["moment2"], {n: st[n] for n in CUR}, np.float64, sigma_color=sc)
            grid[sc].append(DR.rel_mse(new, gt))
        d_new = grid[R.DEFAULTS["sigma_color"]][-1]
        print(f"step {dtheta}: filtered relMSE d0 {d0:.4g}; existing path {d_old:.4g} ({d_old / d0:.3f}x); "
              f"lrt_svgf {d_new:.4g} ({d_new / d0:.3f}x); grid " +
              ", ".join(f"sigma_color {sc:g}: {grid[sc][-1]:.4g}" for sc in SIGMA_GRID))
        assert d_new <= TR.BAR_DENOISED * d0, dtheta
    means = {sc: float(np.mean(v)) for sc, v in grid.items()}
    print("mean relMSE over the three: " + ", ".join(f"sigma_color {sc:g}: {m:.4g}" for sc, m in means.items()))
    assert min(means, key=means.get) == R.DEFAULTS["sigma_color"]


# ---- tools/svgf_bench.py
def test_svgf_bench_bytes_and_arguments():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("svgf_bench", os.path.join(root, "tools", "svgf_bench.py"))
    B = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(B)
    # stage 0: colour, moment2, normal, albedo read, (c_0, var_0) written; a pass: c, var, normal, world_pos
    # read, (c, var) written; the last pass: albedo read again, 12 B + 12 B written
    assert B.filter_bytes(1) == (4 * 16 + 32) + (4 * 16 + 16 + 24) == 200
    assert B.filter_bytes(5) == (4 * 16 + 32) + 4 * (4 * 16 + 32) + (4 * 16 + 16 + 24) == 584
    assert B.filter_bytes(5, first_frame=True) == 584 + 16          # stage 0 reads world_pos too
    assert B.filter_bytes(5, variance_out=False) == 584 - 12
    assert B.orbit_args(0.3, 160, 90) == TR.orbit_args(0.3, 160, 90)
    with pytest.raises(SystemExit) as e:
        B.main(["--help"])
    assert e.value.code == 0
    with pytest.raises(SystemExit) as e:
        B.main(["--reps", "5"])
    assert e.value.code != 0
    with pytest.raises(SystemExit):
        B.main(["--iterations", "6"])
