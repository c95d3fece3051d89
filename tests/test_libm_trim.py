"""The range-check-trimmed sqrt / reciprocal forms (lrt_trace.h) against the checked ones, bit
for bit, on the domains they are used on (lrt_libm_eval kinds 8-10, include/lrt_diag.h):

  kind 8   rsqrt_len(d): normalize's 1 / sqrt(d) with ONE range check for both steps, against
           kind 9, rcp_rn(sqrt_rn(d)), the two checked sequences it replaces. The single check
           sends d < 2^-96, infinity and NaN to the checked pair, so the two must agree
           everywhere; the test walks both ends of the fast range exhaustively -- every float of
           [2^-96, 2^-90], and of [2^126, FLT_MAX] (float32 ends below 2^128: the top two
           binades stand for the range's upper end) -- and the values just outside it.
  kind 10  sqrt_fast(x): the fast root without its check, against kind 4 (sqrt_rn) on
           SphereRoots' proven operand range x >= 2^-94 (every float of [2^-96, 2^-90]), and on
           the operand set of the 1 - y sites, {0} and [2^-24, 1] sampled at 2^22 points.

The host build evaluates the plain IEEE operations for all of them (the definition the device
sequences are held to); the GPU-marked case runs the device sequences themselves.
"""
import ctypes

import numpy as np
import pytest

from learnraytracing_amd import _lib as L


def _bits(lo, hi):
    """Every float32 from lo to hi (both positive), as an array."""
    a, b = (int(np.float32(v).view(np.uint32)) for v in (lo, hi))
    return np.arange(a, b + 1, dtype=np.uint32).view(np.float32)


def _domains():
    low = _bits(2.0 ** -96, 2.0 ** -90)
    top = _bits(2.0 ** 126, np.finfo(np.float32).max)
    outside = np.array([0.0, -0.0, 1e-45, 2.0 ** -97, np.nextafter(np.float32(2.0 ** -96), np.float32(0)),
                        -1.0, np.inf, -np.inf, np.nan], np.float32)
    unit = np.concatenate([[0.0], np.linspace(2.0 ** -24, 1.0, 1 << 22)]).astype(np.float32)
    return {"normalize": np.concatenate([low, top, outside, unit]), "roots": np.concatenate([low, unit])}


DOM = _domains()


def host(kind, x):
    x = np.ascontiguousarray(x, np.float32)
    out = np.empty_like(x)
    L.check(L.lib().lrt_libm_eval_host(kind, x.ctypes.data_as(ctypes.c_void_p),
                                       out.ctypes.data_as(ctypes.c_void_p), x.size))
    return out


def _same(got, want, x, what):
    same = (got.view(np.uint32) == want.view(np.uint32)) | (np.isnan(got) & np.isnan(want))
    assert same.all(), f"{what}: {int((~same).sum())} mismatches, first x = {x[~same][:4]!r}"


def test_host_forms_agree():
    x = DOM["normalize"]
    _same(host(8, x), host(9, x), x, "rsqrt_len vs rcp_rn(sqrt_rn)")
    with np.errstate(all="ignore"):
        _same(host(9, x), np.float32(1.0) / np.sqrt(x), x, "rcp_rn(sqrt_rn) vs IEEE 1 / sqrt")
    x = DOM["roots"]
    _same(host(10, x), host(4, x), x, "sqrt_fast vs sqrt_rn")
    _same(host(10, x), np.sqrt(x), x, "sqrt_fast vs IEEE sqrt")
    z = host(10, np.zeros(1, np.float32))
    assert z.view(np.uint32)[0] == 0, "sqrt of +0 is +0"


def test_new_kinds_bounds():
    x = np.ones(1, np.float32)
    p = x.ctypes.data_as(ctypes.c_void_p)
    assert L.lib().lrt_libm_eval_host(10, p, p, 1) == 0
    assert L.lib().lrt_libm_eval_host(11, p, p, 1) != 0


@pytest.mark.gpu
def test_device_forms_agree(gpu):
    """The device sequences: the merged check and the unchecked root give the checked forms'
    bits, which are the host's IEEE results."""
    import torch

    def dev(kind, d_in):
        o = torch.empty_like(d_in)
        L.check(L.lib().lrt_libm_eval_device(kind, d_in.data_ptr(), o.data_ptr(), d_in.numel()))
        return o.cpu().numpy()

    x = DOM["normalize"]
    d = torch.from_numpy(x).cuda()
    want = dev(9, d)
    _same(dev(8, d), want, x, "device rsqrt_len vs rcp_rn(sqrt_rn)")
    _same(want, host(9, x), x, "device rcp_rn(sqrt_rn) vs host")
    x = DOM["roots"]
    d = torch.from_numpy(x).cuda()
    want = dev(4, d)
    got = dev(10, d)
    _same(got, want, x, "device sqrt_fast vs sqrt_rn")
    _same(want, host(4, x), x, "device sqrt_rn vs host")
    assert got.view(np.uint32)[x.view(np.uint32) == 0][0] == 0, "sqrt_fast(+0) is +0"
