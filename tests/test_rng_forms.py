"""The one-rounding forms of the RNG's floats (lrt_trace.h) against the reference's expressions,
through the diagnostics entry lrt_rng_form_sweep (include/lrt_diag.h). The sweep calls rng_signed,
rng_angle, rng_offset and rng_one_minus, the functions the kernels call, for every draw integer
k = XorShift32 & 0xFFFFFF in [0, 2^24), beside the source form on R = (float)k * 2^-24:

  2 R - 1, R * 2 - 1          fma(kf, 2^-23, -1)      maths.cpp:24-49 (the rejection candidates, z)
  R * 2 * kPI, 2 * kPI * R    kf * (kPI * 2^-23)      maths.cpp:31, parallel.cpp:113
  1 - R                       fma(kf, -2^-24, 1)      parallel.cpp:111
  (float)x + R                fma(kf, 2^-24, x)       parallel.cpp:272-273, x in CAM_X

Every product of kf with a power of two is exact, so each source chain rounds once and the short
form takes the same rounding: 0 mismatches. This is the host build (hardware fma where
the CPU has it); tests/test_gpu_rng_forms.py sweeps the device's instructions.
"""
import ctypes

import numpy as np

from learnraytracing_amd import _lib as L

FORMS = ("2R-1", "R*2*kPI", "2*kPI*R", "1-R")
CAM_X = (0, 1, 2, 3, 1279, 4095, 7679)
DRAWS = 1 << 24


def sweep(on_device=0):
    out = np.full(len(FORMS) + len(CAM_X) + 1, 77, np.uint64)
    L.check(L.lib().lrt_rng_form_sweep(on_device, out.ctypes.data_as(ctypes.c_void_p)))
    names = FORMS + tuple(f"{x}+R" for x in CAM_X)
    return dict(zip(names, (int(v) for v in out[:-1]))), int(out[-1])


def check(on_device=0):
    bad, draws = sweep(on_device)
    print(f"rng forms ({'device' if on_device else 'host'}): {draws} draws, mismatches {bad}")
    assert draws == DRAWS
    assert len(bad) == len(FORMS) + len(CAM_X)
    assert all(v == 0 for v in bad.values()), bad


def test_host_sweep():
    check(0)


def test_constants_are_what_the_argument_needs():
    """kPI * 2^-23 is kPI's significand at another exponent (exact), and the smallest non-zero
    angle is a normal float."""
    kpi = np.float32(3.1415926)
    c = np.float32(kpi * np.float32(2.0 ** -23))
    assert float(c) == float(kpi) * 2.0 ** -23
    assert float(c) > 2.0 ** -126 and 3.6e-7 < float(c) < 3.8e-7


def test_sweep_rejects_null():
    assert L.lib().lrt_rng_form_sweep(0, None) != 0
