"""The short exact divisions of the Lambert light sample (lrt_trace.h) against the plain IEEE
divisions, through the diagnostics entry lrt_exact_div_sweep (include/lrt_diag.h): the sweep
calls div_pi / div_pi_fast and member_quot / div_by_rcp, the functions the kernels call, so a
change to either sequence or to its range test is what gets checked, not a restatement.

  div_pi(x) = x / kPI as q = x*c, r = fma(-q, kPI, x), fma(r, c, q) with c = RN(1 / kPI):
      every one of the 2^32 bit patterns. The bare sequence must match on its stated range
      ({+0} and [2^-104, FLT_MAX]); the complete function (range test, fallback) everywhere.
  member_quot(v, l) = v / l per component with one reciprocal, normalize_member's quotients:
      every float l of [0.5, 2] against 32 dividend patterns (the range's edges 2^-96 and 2^96,
      values around 1 and l, both signs, +-0, denormal and tiny dividends, random ones), 2^30
      random pairs inside the range, and divisors of every kind (zero, denormal, negative,
      huge, inf, NaN) for the fallback.

The host build runs the same fma sequences (r = RN(1 / l) is the host's division there; the
device's v_rcp_f32 plus two Newton steps gives the same bits, swept in tests/test_gpu_exact_div.py).
"""
import ctypes

import numpy as np

from learnraytracing_amd import _lib as L

N_DIVISORS = (1 << 24) + 1   # the floats of [0.5, 2]
PATTERNS = 32


def sweep(what, first, count, on_device=0):
    out = np.zeros(4, np.uint64)
    L.check(L.lib().lrt_exact_div_sweep(what, first, count, on_device, out.ctypes.data_as(ctypes.c_void_p)))
    full, bare, inside, lowest = (int(v) for v in out)
    return full, bare, inside, lowest


def check(what, first, count, inside_want, on_device=0):
    full, bare, inside, lowest = sweep(what, first, count, on_device)
    print(f"sweep {what}: {count} cases, {inside} inside the range, {full} / {bare} mismatches")
    assert (full, bare) == (0, 0), f"sweep {what}: first failing case {lowest:#x}"
    assert lowest == 2 ** 64 - 1
    assert inside == inside_want, (inside, inside_want)


# the floats of {+0} and [2^-104, FLT_MAX]
DIV_PI_INSIDE = 1 + (0x7f7fffff - 0x0b800000 + 1)
# of the 32 dividend patterns 27 lie inside [2^-96, 2^96] (5 are zeros, denormal or tiny)
MEMBER_INSIDE = N_DIVISORS * 27


def test_div_pi_every_float():
    check(0, 0, 1 << 32, DIV_PI_INSIDE)


def test_member_quot_every_divisor():
    check(1, 0, N_DIVISORS * PATTERNS, MEMBER_INSIDE)


def test_member_quot_random_pairs():
    check(2, 0, 1 << 30, 1 << 30)


def test_member_quot_fallback_divisors():
    """Divisors of any bit pattern: about 1 in 128 falls into [0.5, 2], the rest divide."""
    full, bare, inside, lowest = sweep(3, 0, 1 << 24)
    assert (full, bare) == (0, 0), f"first failing case {lowest:#x}"
    assert 0 < inside < (1 << 24) // 64


def test_sweep_arguments():
    out = np.zeros(4, np.uint64)
    p = out.ctypes.data_as(ctypes.c_void_p)
    lib = L.lib()
    assert lib.lrt_exact_div_sweep(0, 0, 0, 0, p) == 0 and int(out[3]) == 2 ** 64 - 1
    assert lib.lrt_exact_div_sweep(4, 0, 1, 0, p) != 0
    assert lib.lrt_exact_div_sweep(0, 1 << 32, 1, 0, p) != 0
    assert lib.lrt_exact_div_sweep(1, 0, N_DIVISORS * PATTERNS + 1, 0, p) != 0
    assert lib.lrt_exact_div_sweep(0, 0, 1, 0, None) != 0

