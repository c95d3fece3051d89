"""The per-pixel sample budget without a GPU: the NumPy restatement (tests/sample_budget_ref.py) on
its designed cases and the properties that follow from the definition, and the C-ABI's host-side
contract (lrt_sample_budget_*: defaults, struct layout, validation before any device use) with the
Python front end's argument checks."""
import ctypes
import os
import re

import numpy as np
import pytest

import sample_budget_ref as R
from learnraytracing_amd import LrtError, _lib as L
from learnraytracing_amd import sample_budget_desc, sample_budget_host, sample_budget_tensor


def _gpu_present():
    import torch
    return torch.cuda.device_count() > 0


def _var(h, w, value=0.0):
    v = np.zeros((h, w, 4), np.float32)
    v[..., :3] = value
    return v


# ---- the restatement's designed cases
def test_zero_variance_spreads_evenly():
    counts, info = R.budget(_var(5, 7), 1, 8, 35 + 100)
    assert (counts == 1 + 100 // 35).all() and info == (35 * 3, 0)
    counts, _ = R.budget(_var(5, 7), 0, 8, 34)      # E / m = 0: nothing to hand out in whole samples
    assert (counts == 0).all()


def test_hot_pixel_clamps_and_the_next_pass_hands_on():
    v = _var(4, 4, 1e-6)
    v[2, 1, :3] = 1e4
    one, info1 = R.budget(v, 1, 16, 16 + 64, passes=1)
    two, info2 = R.budget(v, 1, 16, 16 + 64, passes=2)
    assert one[2, 1] == 16 and two[2, 1] == 16
    others = np.ones((4, 4), bool)
    others[2, 1] = False
    assert (one[others] == 1).all() and info1[0] == 15 + 16       # the surplus is lost with one pass
    assert (two[others] == 1 + (80 - 31) // 15).all() and info2[0] == 16 + 15 * 4
    assert info1[1] == info2[1] == int(R.weights(v).sum())


def test_budget_of_the_minimum_adds_nothing_and_equal_bounds():
    v = R.random_field(9, 6, 3)
    counts, info = R.budget(v, 2, 9, 2 * 54)
    assert (counts == 2).all() and info[0] == 108
    counts, info = R.budget(v, 5, 5, 5 * 54 + 1000, passes=4)
    assert (counts == 5).all() and info == (270, 0)                # U is empty: Q = 0


def test_bad_variance_has_no_weight_and_weight_max_saturates():
    v = _var(1, 8)
    v[0, :, 0] = [np.nan, np.inf, -np.inf, -1.0, 0.0, 4.0, 1e12, 1e-30]
    q = R.weights(v)
    f = np.float32
    w5 = np.sqrt(f(0.2126) * f(4.0))
    assert q[0, :5].tolist() == [0, 0, 0, 0, 0]
    assert q[0, 5] == int(w5 * f(65536.0)) and q[0, 6] == 256 * 65536 and q[0, 7] == 0
    assert R.weights(v, weight_max=16384.0)[0, 6] == 16384 * 65536 == 1 << 30
    c = np.ones((1, 8, 4), np.float32)
    c[0, 5, :3] = [np.nan, 0.0, 0.0]     # fmaxf(NaN, 0) = 0: the floor alone divides
    c[0, 6, :3] = np.inf                 # w = 0
    qc = R.weights(v, c)
    assert qc[0, 5] == int(w5 / f(0.01) * f(65536.0)) and qc[0, 6] == 0
    # LRT_SB_STD squares first: a negative deviation is a variance
    s = _var(1, 2)
    s[0, :, 1] = [-2.0, 2.0]
    qs = R.weights(s, flags=R.SB_STD)
    assert qs[0, 0] == qs[0, 1] == int(np.sqrt(f(0.7152) * f(4.0)) * f(65536.0))
    assert (R.weights(s)[0] == [0, int(np.sqrt(f(0.7152) * f(2.0)) * f(65536.0))]).all()


def test_sum_never_exceeds_the_budget_on_random_fields():
    rng = np.random.default_rng(11)
    for k in range(100):
        w, h = int(rng.integers(1, 12)), int(rng.integers(1, 9))
        lo = int(rng.integers(0, 3))
        hi = lo + int(rng.integers(0, 20))
        total = lo * w * h + int(rng.integers(0, 4 * w * h + 1))
        passes = int(rng.integers(1, 5))
        v, c = R.random_field(w, h, k), (R.random_color(w, h, k) if k % 2 else None)
        counts, info = R.budget(v, lo, hi, total, color=c, passes=passes, flags=R.SB_STD if k % 3 == 0 else 0)
        assert counts.shape == (h, w) and counts.min() >= lo and counts.max() <= hi
        assert info[0] == int(counts.sum()) <= total


def test_counts_are_monotone_in_the_weight_within_a_pass():
    for seed in range(10):
        v = R.random_field(16, 8, seed)
        q = R.weights(v).ravel()
        counts, _ = R.budget(v, 1, 4096, 128 * 20, passes=1)
        order = np.argsort(q, kind="stable")
        assert (np.diff(counts.ravel()[order]) >= 0).all()


# ---- the C-ABI's host side
def test_struct_layout_and_defaults():
    src = open(L.HEADER_PATH).read()
    body = re.search(r"typedef struct lrt_sample_budget_desc \{(.*?)\} lrt_sample_budget_desc;", src, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [n.strip() for decl in re.findall(r"(?:int32_t|int64_t|float)\s+([^;]+);", body) for n in decl.split(",")]
    assert names == [n for n, _ in L.SampleBudgetDesc._fields_]
    assert ctypes.sizeof(L.SampleBudgetDesc) == 48 and L.SampleBudgetDesc.budget.offset == 32
    assert L.SampleBudgetDesc.luma_floor.offset == 40 and L.SampleBudgetDesc.weight_max.offset == 44
    consts = dict(re.findall(r"#define (LRT_(?:COUNT_MAX|SB_STD)) (\S+)", src))
    assert (int(consts["LRT_COUNT_MAX"]), int(consts["LRT_SB_STD"])) == (L.COUNT_MAX, L.SB_STD) == (R.COUNT_MAX, R.SB_STD)
    d = sample_budget_desc(640, 360, 1, 32, 4 * 640 * 360)
    assert (d.width, d.height, d.flags, d.reserved, d.min_count, d.max_count, d.passes, d.reserved2, d.budget) == \
        (640, 360, 0, 0, 1, 32, 2, 0, 921600)
    assert (d.luma_floor, d.weight_max) == (np.float32(0.01), 256.0)
    assert (d.passes, d.flags) == (R.DEFAULTS["passes"], R.DEFAULTS["flags"])
    lib = L.lib()
    assert lib.lrt_sample_budget_default(4, 4, 1, 2, 16, None) == L.LRT_E_INVALID
    assert lib.lrt_sample_budget_default(0, 4, 1, 2, 16, ctypes.byref(d)) == L.LRT_E_INVALID


def test_validation_before_device_use():
    """Every invalid argument is LRT_E_INVALID, a valid call without lrt_initialize() LRT_E_STATE: no
    GPU needed for either, host and device entry points alike."""
    lib = L.lib()
    w, h = 16, 9
    var_a, col_a = (np.zeros((h, w, 4), np.float32) for _ in range(2))
    cnt_a, info_a = np.zeros(w * h + 8, np.int32), np.zeros(4, np.uint64)
    var, col, cnt, info = (a.ctypes.data for a in (var_a, col_a, cnt_a, info_a))

    def desc(**kw):
        d = L.SampleBudgetDesc()
        assert lib.lrt_sample_budget_default(w, h, 1, 8, 4 * w * h, ctypes.byref(d)) == 0
        for k, v in kw.items():
            setattr(d, k, v)
        return d

    def calls(d, v, c, n, i):
        ref = ctypes.byref(d) if d is not None else None
        return (lib.lrt_sample_budget_host(ref, v, c, n, i), lib.lrt_sample_budget_device(ref, v, c, n, i, None))

    inv = (L.LRT_E_INVALID, L.LRT_E_INVALID)
    good = (desc(), var, col, cnt, info)
    assert calls(None, *good[1:]) == inv
    assert calls(good[0], None, col, cnt, info) == inv
    assert calls(good[0], var, col, None, info) == inv
    for bad in (dict(width=0), dict(height=0), dict(width=-3), dict(width=46341, height=46341, budget=2 ** 31 - 1),
                dict(flags=2), dict(flags=-1), dict(reserved=1), dict(reserved2=1),
                dict(min_count=-1), dict(min_count=9), dict(max_count=L.COUNT_MAX + 1),
                dict(min_count=0, max_count=-1), dict(passes=0), dict(passes=5),
                dict(budget=w * h - 1), dict(budget=2 ** 31), dict(budget=-1), dict(min_count=8, budget=7 * w * h),
                dict(luma_floor=0.0), dict(luma_floor=-1.0), dict(weight_max=0.0), dict(weight_max=-2.0),
                dict(weight_max=16385.0)):
        assert calls(desc(**bad), *good[1:]) == inv, bad
    for name in ("luma_floor", "weight_max"):
        for v in (float("inf"), -float("inf"), float("nan")):
            assert calls(desc(**{name: v}), *good[1:]) == inv, (name, v)
    # aliasing, by address range
    for p in (var, var + w * h * 16 - 4, col, col + 4, info - w * h * 4 + 4):
        assert calls(good[0], var, col, p, info) == inv, "counts"
    assert "alias" in lib.lrt_last_error().decode()
    for p in (var, var + w * h * 16 - 8, col + 8, cnt, cnt + w * h * 4 - 8):
        assert calls(good[0], var, col, cnt, p) == inv, "info"
    assert calls(good[0], var, var, var, None) == inv
    if os.environ.get("HIP_VISIBLE_DEVICES") == "" or not _gpu_present():
        st = (L.LRT_E_STATE, L.LRT_E_STATE)
        assert calls(*good) == st
        assert calls(good[0], var, None, cnt, None) == st
        assert calls(good[0], var, var, cnt, info) == st                       # two inputs may be one buffer
        assert calls(good[0], var, col, cnt, cnt + w * h * 4) == st            # adjacent is not overlapping
        for ok in (dict(flags=L.SB_STD), dict(passes=1), dict(passes=4), dict(min_count=0, max_count=0, budget=0),
                   dict(min_count=8, max_count=8, budget=8 * w * h), dict(max_count=L.COUNT_MAX, budget=2 ** 31 - 1),
                   dict(weight_max=16384.0), dict(luma_floor=1e-30)):
            assert calls(desc(**ok), *good[1:]) == st, ok


def test_python_front_end_rejects_bad_arguments():
    v = np.zeros((9, 16, 4), np.float32)
    d = sample_budget_desc(16, 9, 1, 8, 600, flags=L.SB_STD, passes=3, luma_floor=0.5, weight_max=8)
    assert (d.flags, d.passes, d.luma_floor, d.weight_max) == (1, 3, 0.5, 8.0)
    with pytest.raises(LrtError):
        sample_budget_desc(16, 9, 1, 8, 600, sigma=1.0)
    with pytest.raises(LrtError):
        sample_budget_host(v.ravel(), 1, 8, 600)
    with pytest.raises(LrtError):
        sample_budget_host(v.astype(np.float64), 1, 8, 600)
    with pytest.raises(LrtError):
        sample_budget_host(v, 1, 8, 600, color=v[:4])
    with pytest.raises(LrtError):
        sample_budget_host(v, 1, 8, 600, counts=np.zeros((9, 16), np.int64))
    with pytest.raises(LrtError):
        sample_budget_host(v, 1, 8, 600, counts=np.zeros(16 * 9 - 1, np.int32))
    with pytest.raises(LrtError) as e:   # the library's own check
        sample_budget_host(v, 4, 8, 100)
    assert e.value.code == L.LRT_E_INVALID and "budget" in str(e.value)
    with pytest.raises(LrtError):        # host arrays are not tensors
        sample_budget_tensor(v, 1, 8, 600)


# ---- tools/adaptive_bench.py
def test_adaptive_bench_bytes_and_arguments():
    import importlib.util
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("adaptive_bench", os.path.join(root, "tools", "adaptive_bench.py"))
    B = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(B)
    # the weight kernel reads variance and colour and writes q and the count; a pass reads both, writes the count
    assert B.budget_bytes() == 16 + 16 + 8 + 2 * 12 == 64
    assert B.budget_bytes(color=False, passes=1) == 36
    with pytest.raises(SystemExit) as e:
        B.main(["--help"])
    assert e.value.code == 0
    with pytest.raises(SystemExit) as e:
        B.main(["--reps", "5"])
    assert e.value.code != 0
