"""Firefly suppression without a GPU: the NumPy restatement (tests/firefly_ref.py) on its designed
cases against hand-written expectations and on the properties that follow from the definition, and
the C-ABI's host-side contract (lrt_firefly_*: defaults, struct layout, validation before any device
use) with the Python front ends' argument checks and the bench tool's byte arithmetic."""
import ctypes
import os
import re

import numpy as np
import pytest

import firefly_ref as R
from learnraytracing_amd import LrtError, _lib as L
from learnraytracing_amd import TemporalAccumulator, firefly_desc, firefly_host, firefly_tensor

F = np.float32


def _gpu_present():
    import torch
    return torch.cuda.device_count() > 0


# ---- the restatement's designed cases
@pytest.mark.parametrize("case", R.DESIGNED_CASES)
def test_designed_cases(case):
    color, ids, params, expect = R.designed_inputs(case)
    keep = color.copy()
    res = R.step(color, ids, **params)
    assert np.array_equal(R.bits(color), R.bits(keep))
    R.check_designed(case, color, res, expect)


def test_a_rank1_spike_is_exactly_s_times_c():
    color, ids, params, _ = R.designed_inputs("spike_rank1")
    res = R.step(color, ids, **params)
    yk = (F(0.2126) * F(0.5) + F(0.7152) * F(0.25)) + F(0.0722) * F(0.125)
    T = F(2.0) * yk + F(0.01)
    s = T / ((F(0.2126) * F(1e4) + F(0.7152) * F(5e3)) + F(0.0722) * F(2e3))
    assert res["T"][2, 3] == T and res["m"][2, 3] == 8
    assert res["out"][2, 3, :3].tolist() == [s * F(1e4), s * F(5e3), s * F(2e3)]
    assert res["excess"][2, 3].tolist() == [F(1e4) - s * F(1e4), F(5e3) - s * F(5e3), F(2e3) - s * F(2e3), 0.0]
    assert abs(float(R.luma(res["out"][2, 3])) / float(T) - 1) < 1e-6        # the luminance lands on T


def test_pair_passes_at_rank_1_and_is_caught_at_rank_2():
    color, ids, _, _ = R.designed_inputs("pair_rank1")
    assert R.step(color, ids, rank=1)["info"].tolist() == [0, 0]
    assert R.step(color, ids, rank=2)["info"].tolist() == [2, 0]
    # a 2 x 2 cluster passes ranks 1 to 3 and is caught at rank 4
    color[1:3, 3:5, :3] = R.HOT
    assert [int(R.step(color, ids, rank=k, min_taps=4)["info"][0]) for k in (1, 2, 3, 4)] == [0, 0, 0, 4]


def test_threshold_is_floor_for_a_zero_or_negative_rank_value():
    for case in ("yk_negative_zero", "yk_negative"):
        color, ids, params, _ = R.designed_inputs(case)
        res = R.step(color, ids, **params)
        assert res["T"][2, 3] == F(0.01) and res["class"][2, 3] == 1


def test_properties_on_generated_fields():
    """Whatever the field holds: classes 0 and 2 keep every bit, alpha is kept everywhere, no
    non-finite value appears at a pixel that was finite, a clamped pixel's luminance does not grow,
    info counts the classes, and a pixel without support is class 2 whatever it contains."""
    for label, w, h, seed, with_id, params in R.case_list():
        color, ids = R.field(w, h, seed)
        res = R.step(color, ids if with_id else None, **params)
        cls, out = res["class"], res["out"]
        assert set(np.unique(cls)) <= {0, 1, 2, 3}, label
        keep = (cls == 0) | (cls == 2)
        assert np.array_equal(R.bits(out[keep]), R.bits(color[keep])), label
        assert np.array_equal(R.bits(out[..., 3]), R.bits(color[..., 3])), label
        p = dict(R.DEFAULTS, **params)
        assert np.array_equal(cls == 2, res["m"] < p["min_taps"]), label
        fin_in = np.isfinite(color[..., :3]).all(-1)
        c1 = cls == 1
        assert fin_in[c1].all() and np.isfinite(out[c1][:, :3]).all(), label
        assert (R.luma(out[c1]) <= R.luma(color[c1])).all(), label
        assert res["info"].tolist() == [int(c1.sum()), int((cls == 3).sum())], label
        assert not R.bits(res["excess"][~c1]).any(), label
    # the generator delivers what it promises (19 x 13, seed 6)
    color, ids = R.field(19, 13, 6)
    y = R.luma(color)
    assert np.isnan(color).any() and np.isposinf(color).any() and np.isneginf(color).any()
    assert (color[..., :3] < 0).any() and (R.bits(color[..., :3]) == 0x80000000).any() and (color[..., :3] == 0).any()
    assert ((np.abs(color[..., :3]) < np.finfo(np.float32).tiny) & (color[..., :3] != 0)).any()
    assert (color[..., :3] == R.FLT_MAX).any() and len(np.unique(ids)) >= 5 and (ids == -1).any()
    res = R.step(color, ids)
    assert sorted(np.unique(res["class"])) == [0, 1, 2, 3] and (y[res["class"] == 1] >= 100).any()


def test_a_non_finite_neighbour_never_reaches_a_pixel():
    """The bits of every other pixel are those of the run with the bad pixel replaced by a value that
    does not count either way (another id)."""
    color, ids = R.field(19, 13, 3)
    color = np.nan_to_num(color, nan=0.5, posinf=1.0, neginf=0.25)
    color[..., :3] = np.minimum(color[..., :3], 100.0)
    bad = color.copy()
    bad[6, 9, :3] = [np.nan, np.inf, -np.inf]
    other = ids.copy()
    other[6, 9] = 12345
    for r in (1, 2):
        a = R.step(bad, ids, radius=r, min_taps=2)
        b = R.step(color, other, radius=r, min_taps=2)
        mask = np.ones(ids.shape, bool)
        mask[6, 9] = False
        for name in ("out", "excess", "class"):
            assert np.array_equal(R.bits(a[name][mask]), R.bits(b[name][mask])), (r, name)


# ---- the C-ABI's host side
def test_struct_layout_and_defaults():
    src = open(L.HEADER_PATH).read()
    body = re.search(r"typedef struct lrt_firefly_desc \{(.*?)\} lrt_firefly_desc;", src, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [re.sub(r"\[\d+\]", "", n.strip()) for decl in re.findall(r"(?:int32_t|float)\s+([^;]+);", body)
             for n in decl.split(",")]
    assert names == [n for n, _ in L.FireflyDesc._fields_]
    D = L.FireflyDesc
    assert ctypes.sizeof(D) == 48 and "48 bytes" in re.search(r"typedef struct lrt_firefly_desc \{[^\n]*", src).group(0)
    assert [getattr(D, n).offset for n, _ in D._fields_] == [0, 4, 8, 12, 16, 20, 24, 28, 32]
    assert int(re.search(r"#define LRT_FIREFLY_MAX_RADIUS (\d+)", src).group(1)) == L.FIREFLY_MAX_RADIUS == R.MAX_RADIUS == 2
    d = firefly_desc(640, 360)
    assert (d.width, d.height, d.radius, d.rank, d.min_taps, d.flags, list(d.reserved)) == (640, 360, 1, 2, 3, 0, [0] * 4)
    assert (d.gain, d.floor) == (2.0, F(0.01))
    assert {k: getattr(d, k) for k in ("radius", "rank", "min_taps", "gain")} == {k: R.DEFAULTS[k] for k in
                                                                                 ("radius", "rank", "min_taps", "gain")}
    assert F(R.DEFAULTS["floor"]) == d.floor
    lib = L.lib()
    assert lib.lrt_firefly_default(4, 4, None) == L.LRT_E_INVALID
    assert lib.lrt_firefly_default(0, 4, ctypes.byref(d)) == L.LRT_E_INVALID
    assert lib.lrt_firefly_default(4, -1, ctypes.byref(d)) == L.LRT_E_INVALID


def test_validation_before_device_use():
    """Every invalid argument is LRT_E_INVALID, a valid call without lrt_initialize() LRT_E_STATE: no
    GPU needed for either, host and device entry points alike."""
    lib = L.lib()
    w, h = 16, 9
    quad, word = w * h * 16, w * h * 4
    in_a, out_a, exc_a = (np.zeros((h, w, 4), np.float32) for _ in range(3))
    id_a, cls_a, info_a = np.zeros((h, w), np.int32), np.zeros(w * h + 8, np.int32), np.zeros(4, np.uint32)
    cin, out, exc, ids, cls, info = (a.ctypes.data for a in (in_a, out_a, exc_a, id_a, cls_a, info_a))

    def desc(**kw):
        d = L.FireflyDesc()
        assert lib.lrt_firefly_default(w, h, ctypes.byref(d)) == 0
        for k, v in kw.items():
            if k == "reserved":
                d.reserved[v] = 1
            else:
                setattr(d, k, v)
        return d

    def calls(d, *a):
        ref = ctypes.byref(d) if d is not None else None
        return (lib.lrt_firefly_host(ref, *a), lib.lrt_firefly_device(ref, *a, None))

    inv, st = (L.LRT_E_INVALID,) * 2, (L.LRT_E_STATE,) * 2
    good = (cin, ids, out, exc, cls, info)
    assert calls(None, *good) == inv
    assert calls(desc(), None, ids, out, exc, cls, info) == inv
    assert calls(desc(), cin, ids, None, exc, cls, info) == inv
    for bad in (dict(width=0), dict(height=0), dict(width=-3), dict(width=46341, height=46341),
                dict(radius=0), dict(radius=3), dict(radius=-1), dict(rank=0), dict(rank=5), dict(rank=-2),
                dict(min_taps=1), dict(min_taps=0), dict(min_taps=9), dict(radius=2, min_taps=25),
                dict(rank=4, min_taps=3), dict(flags=1), dict(flags=-1),
                dict(reserved=0), dict(reserved=1), dict(reserved=2), dict(reserved=3),
                dict(gain=0.0), dict(gain=-1.0), dict(floor=0.0), dict(floor=-0.01)):
        assert calls(desc(**bad), *good) == inv, bad
    for name in ("gain", "floor"):
        for v in (float("inf"), -float("inf"), float("nan")):
            assert calls(desc(**{name: v}), *good) == inv, (name, v)
    # aliasing, by address range: in place, partial overlaps, every output against every input and output
    d = desc()
    for p in (cin, cin + 16, cin + quad - 4, ids, ids + word - 4, ids - quad + 4):
        assert calls(d, cin, ids, p, exc, cls, info) == inv, "out"
    assert "alias" in lib.lrt_last_error().decode()
    for p in (cin, cin + quad - 4, ids, out, out + 32, out - quad + 4):
        assert calls(d, cin, ids, out, p, cls, info) == inv, "excess"
    for p in (cin, cin + quad - 4, ids, ids + 4, out, out + quad - 4, exc + 8):
        assert calls(d, cin, ids, out, exc, p, info) == inv, "class"
    for p in (cin, cin + quad - 4, ids + word - 4, out, out + quad - 4, exc, cls, cls + word - 4, cls - 4):
        assert calls(d, cin, ids, out, exc, cls, p) == inv, "info"
    assert calls(d, cin, None, cin, None, None, None) == inv                   # in place, nothing optional
    if os.environ.get("HIP_VISIBLE_DEVICES") == "" or not _gpu_present():
        assert calls(d, *good) == st
        assert calls(d, cin, None, out, None, None, None) == st
        assert calls(d, cin, ids, out, exc, cls, cls + word) == st             # adjacent is not overlapping
        for ok in (dict(radius=2), dict(radius=2, min_taps=24), dict(min_taps=8), dict(rank=1, min_taps=1),
                   dict(rank=4, min_taps=4), dict(gain=1e-30, floor=1e30)):
            assert calls(desc(**ok), *good) == st, ok


def test_python_front_ends_reject_bad_arguments():
    v = np.zeros((9, 16, 4), np.float32)
    ids = np.zeros((9, 16), np.int32)
    d = firefly_desc(16, 9, radius=2, rank=3, min_taps=7, gain=1.5, floor=0.25)
    assert (d.radius, d.rank, d.min_taps, d.gain, d.floor) == (2, 3, 7, 1.5, 0.25)
    with pytest.raises(LrtError) as e:
        firefly_desc(16, 9, gamma=1.0)
    assert e.value.code == L.LRT_E_INVALID
    for bad in (dict(color=v.ravel()), dict(color=v.astype(np.float64)), dict(color=v[:, ::2]),
                dict(id=ids.astype(np.int64)), dict(id=ids[:4]), dict(out=v[:4]), dict(out=v.astype(np.float64)),
                dict(excess_out=ids), dict(class_out=v), dict(class_out=np.zeros(16 * 9 - 1, np.int32)),
                dict(info=np.zeros(1, np.uint32)), dict(info=np.zeros(2, np.int64)), dict(sigma=1.0)):
        a = dict(color=v, id=ids)
        a.update(bad)
        with pytest.raises(LrtError) as e:
            firefly_host(**a)
        assert e.value.code == L.LRT_E_INVALID, bad
    for bad in (dict(out=v), dict(radius=3), dict(rank=3, min_taps=2), dict(floor=0.0)):   # the library's own checks
        with pytest.raises(LrtError) as e:
            firefly_host(v, ids, **bad)
        assert e.value.code == L.LRT_E_INVALID, bad
    with pytest.raises(LrtError) as e:        # host arrays are not tensors
        firefly_tensor(v, ids)
    assert e.value.code == L.LRT_E_INVALID
    import inspect
    sig = inspect.signature(TemporalAccumulator.step_gbuffer)
    assert sig.parameters["firefly"].default is None


# ---- tools/firefly_bench.py
def test_firefly_bench_bytes_and_arguments():
    import importlib.util
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("firefly_bench", os.path.join(root, "tools", "firefly_bench.py"))
    B = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(B)
    # the quad and the id read, the quad written; the excess quad and the class word on top
    assert B.firefly_bytes() == 16 + 4 + 16 == 36
    assert B.firefly_bytes(ids=False) == 32
    assert B.firefly_bytes(excess=True, cls=True) == 36 + 16 + 4
    with pytest.raises(SystemExit) as e:
        B.main(["--help"])
    assert e.value.code == 0
    with pytest.raises(SystemExit) as e:
        B.main(["--reps", "5"])
    assert e.value.code != 0
