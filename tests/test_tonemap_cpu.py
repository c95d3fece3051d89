"""Auto-exposure metering and tone mapping without a GPU: the specified algorithm in its NumPy
restatement (tests/tonemap_ref.py) -- the bin rule at its edges, the fragile-pixel caps of every table
input, the properties that follow from the formulas -- and the C-ABI's host-side contract
(lrt_tonemap_*: defaults, struct layouts, validation before any device use) with the Python front
end's argument checks."""
import ctypes
import importlib.util
import os
import re

import numpy as np
import pytest

import tonemap_ref as R
from learnraytracing_amd import LrtError, _lib as L
from learnraytracing_amd import ToneMapper, tonemap_desc, tonemap_host, tonemap_tensor


def _gpu_present():
    import torch
    return torch.cuda.device_count() > 0


# ---- the bin rule
def test_bin_edges():
    """2^-16, its predecessor, the predecessor of 2^16, 2^16, 1, 1.125, 0, -1, NaN, +Inf."""
    f = np.float32
    y = np.array([f(2.0 ** -16), np.nextafter(f(2.0 ** -16), f(0)), np.nextafter(f(2.0 ** 16), f(0)), f(2.0 ** 16),
                  f(1), f(1.125), f(0), f(-1), f(np.nan), f(np.inf)], np.float32)
    want = [0, R.UNDER, 255, R.OVER, 128, 129, R.UNDER, R.UNDER, R.UNDER, R.OVER]
    assert R.bins_from_bits(y).tolist() == want
    assert R.bins_from_definition(y).tolist() == want
    assert R.bins_from_bits(np.array([-0.0, 1e-40, -np.inf, 3e38], np.float32)).tolist() == \
        [R.UNDER, R.UNDER, R.UNDER, R.OVER]
    # eight bins per octave, whose lower edges are 2^e (1 + k / 8)
    e, k = np.meshgrid(np.arange(-16, 16), np.arange(8), indexing="ij")
    edges = (np.exp2(e) * (1 + k / 8)).ravel()
    assert R.bins_from_bits(edges.astype(np.float32)).tolist() == list(range(256))
    assert R.bins_from_bits(np.nextafter(edges.astype(np.float32), np.float32(0))).tolist() == \
        [R.UNDER] + list(range(255))
    # the bin's value is the log2 of its middle
    b = np.arange(256)
    mid = np.exp2((b >> 3) - 16.0) * (1 + ((b & 7) + 0.5) / 8)
    assert np.abs(R.bin_values(np.float64) - np.log2(mid)).max() <= 1e-14
    assert (R.bins_from_definition(mid) == b).all()


@pytest.mark.parametrize("case", R.histogram_table(), ids=lambda c: f"{c[0]}x{c[1]}-{c[2]}")
def test_bits_agree_with_definition_and_fragile_caps(case):
    """The bin from the bits of the f32 luminance is the bin of the f64 luminance by definition at
    every non-fragile pixel, for three evaluation orders of the dot product; the table's inputs
    hold no fragile pixel below 20,000 pixels and at most 1e-4 of them above."""
    w, h, kind, seed = case
    color = R.frame(w, h, kind, seed)
    mask, below, above = R.fragile(color)
    n = int(mask.sum())
    if w * h < R.SMALL_PIXELS:
        assert n == 0
    else:
        assert n <= R.LARGE_FRACTION * w * h
        print(f"{w}x{h} {kind}: {n} fragile pixels of {w * h}")
    want = R.bins_from_definition(R.luminance(color, np.float64))
    c = color[..., :3]
    wr, wg, wb = (np.float32(v) for v in (0.2126, 0.7152, 0.0722))
    with np.errstate(all="ignore"):
        orders = (R.luminance(color, np.float32), wr * c[..., 0] + (wg * c[..., 1] + wb * c[..., 2]),
                  (wr * c[..., 0] + wb * c[..., 2]) + wg * c[..., 1])
    for y in orders:
        got = R.bins_from_bits(y)
        assert (got[~mask] == want[~mask]).all()
        assert ((got[mask] == below[mask]) | (got[mask] == above[mask])).all()
    hist = R.histogram(color, np.float32)
    lower, slack = R.histogram_bounds(color)
    assert hist.sum() == w * h and ((lower <= hist) & (hist <= lower + slack)).all()
    assert slack.sum() == 2 * n
    if kind == "constant":
        assert (hist > 0).sum() == 1 and hist[121] == w * h


def test_fragile_finds_the_edges():
    """A luminance on an edge, 4 ulp beside it and 6 ulp beside it; the ends of the range."""
    def grey(y):   # a pixel whose f64 luminance is y up to the weights' sum, 1 + 2.2e-8
        return np.full((1, 1, 4), y, np.float64)
    ulp = 2.0 ** -23
    for y, want in ((1.125, True), (1.125 * (1 + 3 * ulp), True), (1.125 * (1 + 6 * ulp), False), (1.18, False),
                    (2.0 ** -16, True), (2.0 ** 16 * (1 - ulp), True), (2.0 ** -17, False), (2.0 ** 16.5, False),
                    (0.0, False), (np.nan, False), (np.inf, False)):
        s = np.float64(np.float32(0.2126)) + np.float64(np.float32(0.7152)) + np.float64(np.float32(0.0722))
        m, lo, hi = R.fragile(grey(y / s))
        assert bool(m[0, 0]) == want, y
    m, lo, hi = R.fragile(grey(2.0 ** -16))
    assert (lo[0, 0], hi[0, 0]) == (R.UNDER, 0)
    m, lo, hi = R.fragile(grey(2.0 ** 16))
    assert (lo[0, 0], hi[0, 0]) == (255, R.OVER)


# ---- properties of the algorithm (f64)
def _mid_frame(seed=0):
    return R.frame(96, 64, seed=seed, lo=-10.0, hi=10.0)   # no mass within 3 octaves of the range's ends


def test_scaling_by_eight_shifts_everything_by_three_octaves():
    color = _mid_frame()
    big = color.copy()
    big[..., :3] *= np.float32(8)                           # exact in f32
    h0, h1 = R.histogram(color, np.float32), R.histogram(big, np.float32)
    assert h0[:24].sum() == 0 and h0[256 - 48:].sum() == 0
    assert np.array_equal(h1[24:256], h0[:232]) and h1[:24].sum() == 0 and np.array_equal(h1[256:], h0[256:])
    n = color.shape[0] * color.shape[1]
    for window in R.WINDOWS:
        p = dict(p_low=window[0], p_high=window[1], ev_min=-30.0, ev_max=30.0)   # (no clamp in the way)
        s0, s1 = (R.exposure(hh, R.NO_HISTORY, n, np.float64, **p) for hh in (h0, h1))
        assert abs((s1[0] - s0[0]) + 3) <= 1e-12 and abs((s1[1] - s0[1]) - 3) <= 1e-12
        assert s0[2] == s1[2] == 1 and s0[3] == s1[3] == 1
        le = np.float32(np.round(s0[0] * 8) / 8)          # (le - 3 is exact in f32)
        for op in R.OPS:
            a = R.tonemap(color, le, np.float64, op)
            b = R.tonemap(big, le - np.float32(3), np.float64, op)
            assert R.rel_gap(a, b) <= 1e-12


def test_percentile_window_resists_fireflies():
    """0.5 % of the pixels at 1e4: the exposure under the window (0.1, 0.9) moves strictly less than
    under (0, 1)."""
    color = _mid_frame(seed=1)
    color[..., :3] = np.clip(color[..., :3], 2.0 ** -6, 2.0)   # a frame of ordinary range
    fire = color.copy()
    n = color.shape[0] * color.shape[1]
    idx = np.random.default_rng(5).permutation(n)[: n // 200]
    fire.reshape(-1, 4)[idx, :3] = 1e4
    shift = {}
    for window in ((0.1, 0.9), (0.0, 1.0)):
        p = dict(p_low=window[0], p_high=window[1])
        a = R.exposure(R.histogram(color, np.float32), R.NO_HISTORY, n, np.float64, **p)[0]
        b = R.exposure(R.histogram(fire, np.float32), R.NO_HISTORY, n, np.float64, **p)[0]
        shift[window] = abs(b - a)
    print(f"log2 exposure shift under 0.5 % fireflies: window (0.1, 0.9) {shift[(0.1, 0.9)]:.4g}, "
          f"window (0, 1) {shift[(0.0, 1.0)]:.4g}")
    assert shift[(0.1, 0.9)] < shift[(0.0, 1.0)]
    assert shift[(0.0, 1.0)] > 0.05


def test_window_by_hand():
    """Three occupied bins, windows cut through them: the mean against the sums written out."""
    hist = np.zeros(R.WORDS, np.int64)
    hist[[100, 128, 200]] = (10, 70, 20)
    hist[R.UNDER], hist[R.OVER] = 5, 7                      # not counted
    l = R.bin_values(np.float64)
    for (lo, hi), m in (((0.0, 1.0), (10, 70, 20)), ((0.5, 1.0), (0, 30, 20)), ((0.05, 0.5), (5, 40, 0)),
                        ((0.0, 0.0625), (6.25, 0, 0)), ((0.85, 0.9), (0, 0, 5))):
        lo32, hi32 = np.float64(np.float32(lo)), np.float64(np.float32(hi))
        got = np.maximum(0, np.minimum(np.array([10, 80, 100.0]), hi32 * 100) - np.maximum(np.array([0, 10, 80.0]), lo32 * 100))
        assert np.abs(got - m).max() <= 1e-5                # (the f32 window ends, promoted)
        m = got
        want = (m * l[[100, 128, 200]]).sum() / m.sum()
        st = R.exposure(hist, R.NO_HISTORY, 112, np.float64, p_low=lo, p_high=hi, ev_min=-30.0, ev_max=30.0)
        assert abs(st[1] - want) <= 1e-12 and st[2] == 100 / 112 and st[3] == 1
        assert abs(st[0] - (np.log2(np.float64(np.float32(0.18))) - want)) <= 1e-12


def test_state_update_rules():
    hist = R.histogram(_mid_frame(), np.float32)
    n = 96 * 64
    first = R.exposure(hist, R.NO_HISTORY, n, np.float64, adapt=0.25)
    target = first[0]                                       # no history: the target at once
    prev = (1.5, -2.0, 1.0, 3.0)
    nxt = R.exposure(hist, prev, n, np.float64, adapt=0.25)
    assert abs(nxt[0] - (1.5 + 0.25 * (target - 1.5))) <= 1e-12 and nxt[3] == 4 and nxt[1] == first[1]
    assert R.exposure(hist, prev, n, np.float64, adapt=1.0)[0] == pytest.approx(target, abs=1e-12)
    assert R.exposure(hist, R.NO_HISTORY, n, np.float64, ev_min=3.0)[0] == max(target, 3.0) == 3.0
    assert R.exposure(hist, R.NO_HISTORY, n, np.float64, ev_max=-6.0)[0] == -6.0
    for kind in R.EMPTY_KINDS:                              # N = 0
        eh = R.histogram(R.empty_frame(9, 7, kind), np.float32)
        assert eh[:256].sum() == 0 and eh[R.UNDER] == 63
        assert R.exposure(eh, prev, 63, np.float64).tolist() == [1.5, -2.0, 0.0, 4.0]
        assert R.exposure(eh, R.NO_HISTORY, 63, np.float64, ev_bias=2.5).tolist() == [2.5, 0.0, 0.0, 1.0]
        assert R.exposure(eh, R.NO_HISTORY, 63, np.float64, ev_bias=9.5).tolist() == [8.0, 0.0, 0.0, 1.0]
        assert R.exposure(eh, (0.5, 0.25, 1.0, 0.0), 63, np.float64, ev_bias=-1).tolist() == [-1.0, 0.25, 0.0, 1.0]


def test_curves():
    c = np.zeros((1, 4001, 4))
    c[0, :, :3] = np.concatenate([[0.0], np.exp2(np.linspace(-20, 16, 4000))])[:, None]
    t = R.tonemap(c, 0.0, np.float64, R.ACES)[0, :, 0]
    assert t.min() >= 0 and t.max() <= 1 and (np.diff(t) >= 0).all() and t[-1] == 1.0 and t[1] > 0
    for white in (1.0, 4.0, 0.5, 11.0):
        w = np.full((1, 1, 4), white)
        assert abs(R.tonemap(w, 0.0, np.float64, R.REINHARD, white=white)[0, 0, 0] - 1.0) <= 1e-15
    r = R.tonemap(c, 0.0, np.float64, R.REINHARD)[0, :, 0]
    assert (np.diff(r) >= 0).all() and r[0] == 0
    x = np.zeros((1, 6, 4), np.float32)
    x[0, :, 0] = [0.0, 1e-30, 0.5, 1.0, 60.0, 65504.0]
    for dtype in (np.float32, np.float64):                  # LINEAR is the identity on [0, 65504]
        assert np.array_equal(R.tonemap(x, 0.0, dtype, R.LINEAR)[0, :, 0], x[0, :, 0].astype(dtype))
    bad = np.zeros((1, 5, 4), np.float32)
    bad[0, :, 0] = [np.nan, -1.0, -np.inf, np.inf, 1e30]
    for op in R.OPS:
        t = R.tonemap(bad, 0.0, np.float64, op)[0, :, 0]
        assert t[:3].tolist() == [0, 0, 0] and np.isfinite(t).all() and t[3] == t[4] > 0


# ---- the C-ABI
def _header():
    return re.sub(r"/\*.*?\*/", "", open(L.HEADER_PATH).read(), flags=re.S)


def test_tonemap_default_desc_and_layouts():
    lib = L.lib()
    d = L.TonemapDesc()
    assert lib.lrt_tonemap_default(1280, 720, ctypes.byref(d)) == 0
    assert (d.width, d.height, d.op, d.auto_exposure, d.flags, d.reserved) == (1280, 720, L.TM_ACES, 1, 0, 0)
    for name in ("key", "p_low", "p_high", "ev_bias", "ev_min", "ev_max", "adapt", "white"):
        assert getattr(d, name) == np.float32(R.DEFAULTS[name]), name
    assert {k: R.DEFAULTS[k] for k in L.TONEMAP_PARAMS} == dict(
        op=2, auto_exposure=1, key=0.18, p_low=0.1, p_high=0.9, ev_bias=0, ev_min=-8, ev_max=8, adapt=1, white=4)
    assert set(L.TONEMAP_PARAMS) == set(R.DEFAULTS)
    assert lib.lrt_tonemap_default(1280, 720, None) == L.LRT_E_INVALID
    assert lib.lrt_tonemap_default(0, 720, ctypes.byref(d)) == L.LRT_E_INVALID
    assert lib.lrt_tonemap_default(1280, -1, ctypes.byref(d)) == L.LRT_E_INVALID
    # the structs as the header declares them: 6 int32 then 8 floats; 4 floats
    src = _header()
    body = re.search(r"typedef struct lrt_tonemap_desc \{(.*?)\} lrt_tonemap_desc;", src, flags=re.S).group(1)
    fields = [(t, n.strip()) for t, names in re.findall(r"(int32_t|float)\s+([^;]+);", body) for n in names.split(",")]
    assert fields == [({"c_int": "int32_t", "c_float": "float"}[t.__name__], n) for n, t in L.TonemapDesc._fields_]
    assert ctypes.sizeof(L.TonemapDesc) == 4 * len(fields) == 56
    body = re.search(r"typedef struct lrt_exposure_state \{(.*?)\} lrt_exposure_state;", src, flags=re.S).group(1)
    names = [n.strip() for n in re.search(r"float\s+([^;]+);", body).group(1).split(",")]
    assert names == [n for n, _ in L.ExposureState._fields_] and ctypes.sizeof(L.ExposureState) == 16
    consts = dict(re.findall(r"#define (LRT_T\w+) (\S+)", src))
    assert (int(consts["LRT_TONEMAP_BINS"]), int(consts["LRT_TONEMAP_HIST_WORDS"])) == (L.TONEMAP_BINS, L.TONEMAP_HIST_WORDS)
    assert [int(consts[k]) for k in ("LRT_TM_LINEAR", "LRT_TM_REINHARD", "LRT_TM_ACES")] == list(R.OPS) == \
        [L.TM_LINEAR, L.TM_REINHARD, L.TM_ACES]
    assert float(consts["LRT_TM_MAX"].rstrip("f")) == L.TM_MAX == R.TM_MAX
    assert (R.BINS, R.WORDS) == (L.TONEMAP_BINS, L.TONEMAP_HIST_WORDS)


def test_tonemap_validation_before_device_use():
    """Every invalid argument is LRT_E_INVALID, a valid call without lrt_initialize() LRT_E_STATE: no
    GPU needed for either, host and device entry points alike."""
    lib = L.lib()
    w, h = 16, 9
    color_a, out_a = (np.zeros((h, w, 4), np.float32) for _ in range(2))
    bgra_a, hist_a, state_a = np.zeros(w * h, np.uint32), np.zeros(L.TONEMAP_HIST_WORDS + 6, np.uint32), np.zeros(8, np.float32)
    color, out, bgra, hist, state = (a.ctypes.data for a in (color_a, out_a, bgra_a, hist_a, state_a))

    def desc(**kw):
        d = L.TonemapDesc()
        assert lib.lrt_tonemap_default(w, h, ctypes.byref(d)) == 0
        for k, v in kw.items():
            setattr(d, k, v)
        return d

    def calls(d, c, s, hg, o, b):
        ref = ctypes.byref(d) if d is not None else None
        return (lib.lrt_tonemap_host(ref, c, s, hg, o, b), lib.lrt_tonemap_device(ref, c, s, hg, o, b, None))

    inv = (L.LRT_E_INVALID, L.LRT_E_INVALID)
    good = (desc(), color, state, hist, out, bgra)
    assert calls(None, *good[1:]) == inv
    assert calls(good[0], None, *good[2:]) == inv
    for bad in (dict(width=0), dict(height=0), dict(width=-3), dict(width=46341, height=46341), dict(op=3), dict(op=-1),
                dict(auto_exposure=2), dict(auto_exposure=-1), dict(flags=1), dict(reserved=1),
                dict(key=0.0), dict(key=-1.0), dict(white=0.0), dict(white=-2.0),
                dict(p_low=-0.1), dict(p_high=1.5), dict(p_low=0.5, p_high=0.5), dict(p_low=0.9, p_high=0.1),
                dict(ev_min=1.0, ev_max=0.5), dict(adapt=0.0), dict(adapt=-0.5), dict(adapt=1.5)):
        assert calls(desc(**bad), *good[1:]) == inv, bad
    for name in ("key", "p_low", "p_high", "ev_bias", "ev_min", "ev_max", "adapt", "white"):
        for v in (float("inf"), -float("inf"), float("nan")):
            assert calls(desc(**{name: v}), *good[1:]) == inv, (name, v)
            assert calls(desc(auto_exposure=0, **{name: v}), *good[1:]) == inv, (name, v)
    assert calls(good[0], color, None, hist, out, bgra) == inv                      # metering needs the state
    assert "state" in lib.lrt_last_error().decode()
    assert calls(desc(auto_exposure=0), color, state, hist, None, None) == inv       # nothing to do
    assert calls(desc(auto_exposure=0), color, None, None, None, None) == inv
    # aliasing, by address range: bgra, histogram and state overlap nothing
    for p in (color, color + 16, out, out + w * h * 16 - 4, hist, hist + 1028, state, state + 12):
        assert calls(*good[:5], p) == inv, "bgra"
    assert "alias" in lib.lrt_last_error().decode()
    for p in (color, color + w * h * 16 - 4, out, bgra, bgra + w * h * 4 - 4, state, state - 1028):
        assert calls(*good[:3], p, out, bgra) == inv, "histogram"
    for p in (color, color + w * h * 16 - 4, out + 32, bgra, hist, hist + 1028, hist - 12):
        assert calls(*good[:2], p, hist, out, bgra) == inv, "state"
    for p in (color + 16, color - 16, color + w * h * 16 - 4):
        assert calls(*good[:4], p, bgra) == inv, "out"
    assert calls(desc(auto_exposure=0), color, state, hist, out, out) == inv         # given buffers are checked
    assert calls(desc(auto_exposure=0), color, color, None, out, bgra) == inv        # ... metering or not
    if os.environ.get("HIP_VISIBLE_DEVICES") == "" or not _gpu_present():
        st = (L.LRT_E_STATE, L.LRT_E_STATE)
        assert calls(*good) == st
        assert calls(*good[:4], color, bgra) == st                                   # in place
        assert calls(*good[:3], None, None, None) == st                              # meter only
        assert calls(*good[:4], None, bgra) == st and calls(*good[:4], out, None) == st
        assert calls(good[0], color, hist + 1032, hist, out, bgra) == st              # adjacent is not overlapping
        assert calls(desc(auto_exposure=0), color, None, None, out, None) == st
        assert calls(desc(auto_exposure=0, ev_bias=-200.0, op=L.TM_LINEAR), color, None, None, None, bgra) == st
        for op in R.OPS:
            assert calls(desc(op=op, p_low=0.0, p_high=1.0, ev_min=2.0, ev_max=2.0, adapt=1.0), *good[1:]) == st


def test_python_front_end_rejects_bad_arguments():
    z = lambda: np.zeros((9, 16, 4), np.float32)   # noqa: E731
    color = z()
    d = tonemap_desc(16, 9, op="reinhard", white=2.0, auto_exposure=0, ev_bias=1)
    assert (d.op, d.white, d.auto_exposure, d.ev_bias) == (L.TM_REINHARD, 2.0, 0, 1.0)
    assert tonemap_desc(16, 9, op=L.TM_LINEAR).op == 0
    with pytest.raises(LrtError):
        tonemap_desc(16, 9, gamma=2.2)
    with pytest.raises(LrtError):
        tonemap_desc(16, 9, op="filmic")
    with pytest.raises(LrtError):
        tonemap_host(color.ravel())
    with pytest.raises(LrtError):
        tonemap_host(color.astype(np.float64))
    with pytest.raises(LrtError):
        tonemap_host(color, state=np.zeros(3, np.float32))
    with pytest.raises(LrtError):
        tonemap_host(color, state=np.zeros(4, np.float64))
    with pytest.raises(LrtError):
        tonemap_host(color, out=z()[:4])
    with pytest.raises(LrtError):
        tonemap_host(color, bgra=np.zeros(16 * 9, np.float32))
    with pytest.raises(LrtError):
        tonemap_host(color, bgra=np.zeros(16 * 9 - 1, np.uint32))
    with pytest.raises(LrtError):
        tonemap_host(color, histogram=np.zeros(257, np.uint32))
    with pytest.raises(LrtError) as e:   # the library's own check: nothing to do
        tonemap_host(color, auto_exposure=0)
    assert e.value.code == L.LRT_E_INVALID
    with pytest.raises(LrtError) as e:
        tonemap_host(color, out=z(), key=-1.0)
    assert e.value.code == L.LRT_E_INVALID
    with pytest.raises(LrtError):        # host arrays are not tensors
        tonemap_tensor(color)
    assert isinstance(ToneMapper.state, property) and ToneMapper.state.fset is None


# ---- tools/tonemap_bench.py
def test_tonemap_bench_bytes_and_arguments():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("tonemap_bench", os.path.join(root, "tools", "tonemap_bench.py"))
    B = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(B)
    # the meter reads the frame, the map reads it again and writes 4 B (and 12 B of out)
    assert B.call_bytes() == 16 + 16 + 4 == 36
    assert B.call_bytes(meter=False) == 20 and B.call_bytes(bgra=False) == 16 and B.call_bytes(out=True) == 48
    with pytest.raises(SystemExit) as e:
        B.main(["--help"])
    assert e.value.code == 0
    with pytest.raises(SystemExit) as e:
        B.main(["--reps", "5"])
    assert e.value.code != 0
