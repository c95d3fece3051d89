"""Firefly restore without a GPU: the NumPy restatement (tests/firefly_restore_ref.py) on its designed
cases against hand-written expectations and on the conservation identity over tame fields, and the
C-ABI's host-side contract (lrt_firefly_restore_*: defaults, struct layout, validation before any
device use) with the Python front ends' argument checks and the bench tool's byte arithmetic."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

import firefly_restore_ref as R
from learnraytracing_amd import LrtError, _lib as L
from learnraytracing_amd import (TemporalAccumulator, firefly_restore_desc, firefly_restore_host,
                                 firefly_restore_tensor)

F = np.float32


def _gpu_present():
    import torch
    return torch.cuda.device_count() > 0


# ---- the restatement
@pytest.mark.parametrize("case", R.DESIGNED_CASES)
def test_designed_cases(case):
    color, excess, ids, params, acc = R.designed_inputs(case)
    keep = color.copy(), excess.copy()
    res = R.step(color, excess, ids, **params)
    assert np.array_equal(R.bits(color), R.bits(keep[0])) and np.array_equal(R.bits(excess), R.bits(keep[1]))
    R.check_designed(case, color, res["out"], acc)


def test_designed_cases_by_hand():
    """The numbers the designed cases stand on, written out."""
    color, excess, ids, params, _ = R.designed_inputs("interior_spike")
    res = R.step(color, excess, ids, **params)
    assert res["W"][3, 4] == 16
    assert res["acc"][2:5, 3:6, 0].tolist() == [[1, 2, 1], [2, 4, 2], [1, 2, 1]]
    assert res["acc"][2:5, 3:6, 1].tolist() == [[2, 4, 2], [4, 8, 4], [2, 4, 2]]
    assert res["acc"][..., 0].sum() == 16 and res["acc"][..., 1].sum() == 32 and res["acc"][..., 2].sum() == 8
    assert res["out"][3, 4, :3].tolist() == [4.5, 8.25, 2.125]
    color, excess, ids, params, _ = R.designed_inputs("corner_spike")
    res = R.step(color, excess, ids, **params)
    assert res["W"][0, 0] == 9 and res["acc"][:2, :2, 0].tolist() == [[4, 2], [2, 1]]
    assert res["acc"][..., 2].sum() == 27 and not res["acc"][2:].any() and not res["acc"][:, 2:].any()
    color, excess, ids, params, _ = R.designed_inputs("alone_on_its_id")
    res = R.step(color, excess, ids, **params)
    assert res["W"][3, 4] == 9 and res["acc"][3, 4].tolist() == [9, 18, 4.5]
    res["acc"][3, 4] = 0
    assert not res["acc"].any()
    color, excess, ids, params, _ = R.designed_inputs("id_border")
    res = R.step(color, excess, ids, **params)
    assert res["W"][3, 3] == 12 and not res["acc"][:, 4:].any() and res["acc"][..., 0].sum() == 12
    color, excess, ids, params, _ = R.designed_inputs("dead_sources")
    res = R.step(color, excess, ids, **params)
    assert not res["e"][1].any() and not res["e"][5, 4].any() and res["e"][5, 1].tolist() == [2.0 ** 100, 16, 32]
    assert not res["acc"][:4].any() and not res["acc"][:, 3:].any() and np.isfinite(res["out"][4:, :3]).all()
    color, excess, ids, params, _ = R.designed_inputs("non_finite_destination")
    out = R.step(color, excess, ids, **params)["out"]
    assert R.bits(out[2, 4, 1]) == 0x7FC12345 and np.isneginf(out[2, 4, 0]) and out[2, 4, 2] == F(0.125) + F(1)
    assert np.isnan(out[3, 5, 0]) and out[3, 5, 1] == F(0.25) + F(4) and np.isposinf(out[3, 5, 2])
    color, excess, ids, params, _ = R.designed_inputs("zero_excess")
    out = R.step(color, excess, ids, **params)["out"]
    assert np.array_equal(R.bits(out), R.bits(color)) and (R.bits(out[1:4, 2:6, :3]) == 0x80000000).all()


def test_the_radius_bounds_the_normaliser():
    for r in range(1, R.MAX_RADIUS + 1):
        z = np.zeros((11, 13, 4), np.float32)
        W = R.step(z, z, None, radius=r)["W"]
        assert W.max() == W[5, 6] == (r + 1) ** 4 and W.min() == W[0, 0] == sum(range(1, r + 2)) ** 2
        ids = np.arange(11 * 13, dtype=np.int32).reshape(11, 13)
        assert (R.step(z, z, ids, radius=r)["W"] == (r + 1) ** 2).all()


@pytest.mark.parametrize("w,h", R.TAME_SIZES, ids=[f"{w}x{h}" for w, h in R.TAME_SIZES])
def test_conservation_on_tame_fields(w, h):
    """sum out = sum color + sum excess over rgb, to the first-order bound of the roundings; every
    field clamps at least two pixels, so the identity is not vacuous; and the restored sum lies
    nearer the input's than the clamped one does."""
    worst = 0.0
    for with_id in (True, False):
        frame, color, excess, ids, clamped = R.tame(w, h, w + h, with_id)
        assert clamped >= 2 and excess[..., :3].sum() > 0
        for r in range(1, R.MAX_RADIUS + 1):
            out = R.step(color, excess, ids, radius=r)["out"]
            err, bound = R.conservation(color, excess, out, r)
            print(f"{w}x{h} r{r} id={with_id}: clamped {clamped}, |error| {err:.4g}, bound {bound:.4g}")
            assert err <= bound, (r, with_id, err, bound)
            worst = max(worst, err / bound)
            s = lambda a: float(a[..., :3].astype(np.float64).sum())   # noqa: E731
            assert abs(s(out) - s(frame)) < abs(s(color) - s(frame))
            assert np.array_equal(R.bits(out[..., 3]), R.bits(color[..., 3]))
    print(f"{w}x{h}: worst error / bound {worst:.3f}")


def test_generated_fields_hold_what_they_promise():
    color, excess, ids = R.wild(19, 13, 3)
    e = excess[..., :3]
    assert np.isnan(e).any() and np.isposinf(e).any() and np.isneginf(e).any() and (e < 0).any()
    assert (e == R.CAP).any() and (e == F(2.0 ** 101)).any() and (R.bits(e) == 0x80000000).any()
    assert ((np.abs(e) < np.finfo(np.float32).tiny) & (e != 0)).any()
    res = R.step(color, excess, ids, radius=2)
    assert (res["e"] == R.CAP).any() and not (np.abs(res["e"]) > R.CAP).any() and np.isfinite(res["acc"]).all()
    labels = [c[0] for c in R.case_list()]
    assert len(labels) == len(set(labels)) == 7 * 4 * 2


# ---- the C-ABI's host side
def test_struct_layout_and_defaults():
    src = open(L.HEADER_PATH).read()
    body = re.search(r"typedef struct lrt_firefly_restore_desc \{(.*?)\} lrt_firefly_restore_desc;", src, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [re.sub(r"\[\d+\]", "", n.strip()) for decl in re.findall(r"(?:int32_t|float)\s+([^;]+);", body)
             for n in decl.split(",")]
    D = L.FireflyRestoreDesc
    assert names == [n for n, _ in D._fields_]
    assert ctypes.sizeof(D) == 32
    assert "32 bytes" in re.search(r"typedef struct lrt_firefly_restore_desc \{[^\n]*", src).group(0)
    assert [getattr(D, n).offset for n, _ in D._fields_] == [0, 4, 8, 12, 16]
    assert int(re.search(r"#define LRT_FIREFLY_RESTORE_MAX_RADIUS (\d+)", src).group(1)) \
        == L.FIREFLY_RESTORE_MAX_RADIUS == R.MAX_RADIUS == 4
    d = firefly_restore_desc(640, 360)
    assert (d.width, d.height, d.radius, d.flags, list(d.reserved)) == (640, 360, R.DEFAULTS["radius"], 0, [0] * 4)
    assert d.radius == 2
    lib = L.lib()
    assert lib.lrt_firefly_restore_default(4, 4, None) == L.LRT_E_INVALID
    assert lib.lrt_firefly_restore_default(0, 4, ctypes.byref(d)) == L.LRT_E_INVALID
    assert lib.lrt_firefly_restore_default(4, -1, ctypes.byref(d)) == L.LRT_E_INVALID


def test_validation_before_device_use():
    """Every invalid argument is LRT_E_INVALID, a valid call without lrt_initialize() LRT_E_STATE: no
    GPU needed for either, host and device entry points alike."""
    lib = L.lib()
    w, h = 16, 9
    quad, word = w * h * 16, w * h * 4
    col_a, exc_a, out_a = (np.zeros((h, w, 4), np.float32) for _ in range(3))
    id_a = np.zeros((h, w), np.int32)
    col, exc, out, ids = (a.ctypes.data for a in (col_a, exc_a, out_a, id_a))

    def desc(**kw):
        d = L.FireflyRestoreDesc()
        assert lib.lrt_firefly_restore_default(w, h, ctypes.byref(d)) == 0
        for k, v in kw.items():
            if k == "reserved":
                d.reserved[v] = 1
            else:
                setattr(d, k, v)
        return d

    def calls(d, *a):
        ref = ctypes.byref(d) if d is not None else None
        return (lib.lrt_firefly_restore_host(ref, *a), lib.lrt_firefly_restore_device(ref, *a, None))

    inv, st = (L.LRT_E_INVALID,) * 2, (L.LRT_E_STATE,) * 2
    good = (col, exc, ids, out)
    assert calls(None, *good) == inv
    assert calls(desc(), None, exc, ids, out) == inv
    assert calls(desc(), col, None, ids, out) == inv
    assert calls(desc(), col, exc, ids, None) == inv
    for bad in (dict(width=0), dict(height=0), dict(width=-3), dict(width=46341, height=46341),
                dict(radius=0), dict(radius=5), dict(radius=-1), dict(flags=1), dict(flags=-1),
                dict(reserved=0), dict(reserved=1), dict(reserved=2), dict(reserved=3)):
        assert calls(desc(**bad), *good) == inv, bad
    # aliasing, by address range: out against every input; only out == color is in place
    d = desc()
    for p in (col + 16, col - 16, col + quad - 4, col - quad + 4, exc, exc + 16, exc + quad - 4, exc - quad + 4,
              ids, ids + 4, ids + word - 4, ids - quad + 4):
        assert calls(d, col, exc, ids, p) == inv, p
    assert "alias" in lib.lrt_last_error().decode()
    assert calls(d, col, col, ids, col) == inv                     # in place, but excess is the same frame too
    assert calls(d, col, exc, None, exc) == inv
    if os.environ.get("HIP_VISIBLE_DEVICES") == "" or not _gpu_present():
        assert calls(d, *good) == st
        assert calls(d, col, exc, None, out) == st
        assert calls(d, col, exc, ids, col) == st                  # out is color: in place is accepted
        assert calls(d, col, exc, None, col) == st
        assert calls(d, col, col + quad, None, col + 2 * quad) == st   # adjacent is not overlapping
        for r in (1, 2, 3, 4):
            assert calls(desc(radius=r), *good) == st, r


def test_python_front_ends_reject_bad_arguments():
    v, x = np.zeros((9, 16, 4), np.float32), np.zeros((9, 16, 4), np.float32)
    ids = np.zeros((9, 16), np.int32)
    assert firefly_restore_desc(16, 9, radius=4).radius == 4
    with pytest.raises(LrtError) as e:
        firefly_restore_desc(16, 9, rank=2)
    assert e.value.code == L.LRT_E_INVALID
    for bad in (dict(color=v.ravel()), dict(color=v.astype(np.float64)), dict(color=v[:, ::2]),
                dict(excess=x.astype(np.float64)), dict(excess=x[:4]), dict(excess=ids), dict(excess=None),
                dict(id=ids.astype(np.int64)), dict(id=ids[:4]), dict(out=v[:4]), dict(out=v.astype(np.float64)),
                dict(sigma=1.0)):
        a = dict(color=v, excess=x, id=ids)
        a.update(bad)
        with pytest.raises(LrtError) as e:
            firefly_restore_host(**a)
        assert e.value.code == L.LRT_E_INVALID, bad
    for bad in (dict(out=x), dict(radius=0), dict(radius=5)):      # the library's own checks
        with pytest.raises(LrtError) as e:
            firefly_restore_host(v, x, ids, **bad)
        assert e.value.code == L.LRT_E_INVALID, bad
    with pytest.raises(LrtError) as e:        # host arrays are not tensors
        firefly_restore_tensor(v, x, ids)
    assert e.value.code == L.LRT_E_INVALID
    if os.environ.get("HIP_VISIBLE_DEVICES") == "" or not _gpu_present():
        for out in (None, v):                 # a good call, in place too, gets as far as the library's state
            with pytest.raises(LrtError) as e:
                firefly_restore_host(v, x, ids, out=out)
            assert e.value.code == L.LRT_E_STATE
    sig = inspect.signature(TemporalAccumulator.step_gbuffer)
    assert sig.parameters["firefly_restore"].default is None


# ---- tools/firefly_restore_bench.py
def test_firefly_restore_bench_bytes_and_arguments():
    import importlib.util
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("firefly_restore_bench",
                                                  os.path.join(root, "tools", "firefly_restore_bench.py"))
    B = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(B)
    # the colour and excess quads and the id read, the quad written
    assert B.restore_bytes() == 16 + 16 + 4 + 16 == 52
    assert B.restore_bytes(ids=False) == 48
    with pytest.raises(SystemExit) as e:
        B.main(["--help"])
    assert e.value.code == 0
    with pytest.raises(SystemExit) as e:
        B.main(["--reps", "5"])
    assert e.value.code != 0
