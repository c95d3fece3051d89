"""The one-rounding forms of the RNG's floats on gfx950: v_fma_f32 and v_mul_f32 as the kernels
issue them against the device's own evaluation of the reference's expressions, every draw integer
in [0, 2^24) and every camera column of tests/test_rng_forms.py, in one launch
(lrt_rng_form_sweep, include/lrt_diag.h). 0 mismatches.
"""
import pytest

from test_rng_forms import check

pytestmark = pytest.mark.gpu


def test_device_sweep(gpu):
    check(1)
