"""lrt_render_counts_* without a GPU: the struct's layout, validation before any device use (host and
device entry points alike) and the Python front end's argument checks."""
import ctypes
import os
import re

import numpy as np
import pytest

from learnraytracing_amd import Job, LrtError, _lib as L
from learnraytracing_amd import render_counts_host, render_counts_tensor


def _gpu_present():
    import torch
    return torch.cuda.device_count() > 0


def test_struct_layout():
    src = open(L.HEADER_PATH).read()
    body = re.search(r"typedef struct lrt_render_counts \{(.*?)\} lrt_render_counts;", src, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [n.strip().lstrip("*") for decl in re.findall(r"(?:const int32_t\*|int64_t|int32_t|unsigned long long\*)\s+([^;]+);", body)
             for n in decl.split(",")]
    assert names == [n for n, _ in L.RenderCounts._fields_]
    assert ctypes.sizeof(L.RenderCounts) == 32
    assert [getattr(L.RenderCounts, n).offset for n in names] == [0, 8, 16, 20, 24]
    consts = dict(re.findall(r"#define (LRT_RC_MEAN) (\S+)", src))
    assert int(consts["LRT_RC_MEAN"]) == L.RC_MEAN == 1 and L.RC_CAPACITY_MAX == 2 ** 27


def test_validation_before_device_use():
    lib = L.lib()
    w, h = 16, 9
    buf_a = np.zeros((h, w, 4), np.float32)
    cnt_a, info_a, rays_a = np.ones(w * h + 8, np.int32), np.zeros(4, np.uint64), np.zeros(2, np.uint64)
    buf, cnt, info, rays = (a.ctypes.data for a in (buf_a, cnt_a, info_a, rays_a))

    def rcs(counts=cnt, capacity=w * h * 4, flags=0, reserved=0, info_=info):
        rc = L.RenderCounts()
        rc.counts, rc.capacity, rc.flags, rc.reserved, rc.info = counts, capacity, flags, reserved, info_
        return rc

    def calls(job, rc, b=buf, r=rays):
        d = job.desc() if job is not None else None
        dref = ctypes.byref(d) if d is not None else None
        rref = ctypes.byref(rc) if rc is not None else None
        out = ctypes.c_longlong(0)
        return (lib.lrt_render_counts_host(dref, rref, b, ctypes.byref(out)),
                lib.lrt_render_counts_device(dref, rref, b, r, None))

    inv = (L.LRT_E_INVALID, L.LRT_E_INVALID)
    job = Job(width=w, height=h, frames=4)
    assert calls(None, rcs()) == inv
    assert calls(job, None) == inv
    assert calls(job, rcs(), b=None) == inv
    assert lib.lrt_render_counts_device(ctypes.byref(job.desc()), ctypes.byref(rcs()), buf, None, None) == L.LRT_E_INVALID
    # what lrt_render_device rejects
    for bad in (dict(max_depth=65), dict(max_depth=-1), dict(x0=10, x_count=10), dict(frames=-1), dict(y0=5, row_count=7),
                dict(row_block=8, row_period=2, row_phase=2, row_count=1), dict(frame0=2 ** 31 - 2, frames=4)):
        kw = dict(width=w, height=h, frames=4)
        kw.update(bad)
        assert calls(Job(**kw), rcs()) == inv, bad
    # a counted render takes no flag
    for flag in (L.F_SIMPLE, L.F_POOL, L.F_WAVEFRONT, L.F_GRID, L.F_NO_DOUBLE_LIGHT, L.F_SCENE_GLOBAL, 4):
        assert calls(Job(width=w, height=h, frames=4, flags=flag), rcs()) == inv, flag
    assert "flag" in lib.lrt_last_error().decode()
    assert calls(job, rcs(counts=None)) == inv
    for cap in (0, -1, 2 ** 27 + 1, 2 ** 40):
        assert calls(job, rcs(capacity=cap)) == inv, cap
    assert "capacity" in lib.lrt_last_error().decode()
    for kw in (dict(flags=2), dict(flags=-1), dict(reserved=1)):
        assert calls(job, rcs(**kw)) == inv, kw
    # aliasing, by address range
    for p in (buf, buf + w * h * 16 - 4, buf - w * h * 4 + 4):
        assert calls(job, rcs(counts=p)) == inv, "counts"
    assert "alias" in lib.lrt_last_error().decode()
    for p in (buf, buf + w * h * 16 - 8, cnt, cnt + w * h * 4 - 8):
        assert calls(job, rcs(info_=p)) == inv, "info"
    assert lib.lrt_render_counts_device(ctypes.byref(job.desc()), ctypes.byref(rcs()), buf, info + 8, None) == L.LRT_E_INVALID
    assert lib.lrt_render_counts_device(ctypes.byref(job.desc()), ctypes.byref(rcs()), buf, cnt + 4, None) == L.LRT_E_INVALID
    if os.environ.get("HIP_VISIBLE_DEVICES") == "" or not _gpu_present():
        st = (L.LRT_E_STATE, L.LRT_E_STATE)
        assert calls(job, rcs()) == st
        assert calls(job, rcs(info_=None, flags=L.RC_MEAN, capacity=1)) == st
        assert calls(job, rcs(capacity=2 ** 27)) == st
        assert calls(job, rcs(info_=cnt + w * h * 4)) == st                        # adjacent is not overlapping
        assert calls(Job(width=w, height=h, frames=0), rcs()) == st
        assert calls(Job(width=w, height=h, x0=3, x_count=11, row_block=2, row_period=2, row_phase=1, frames=2,
                         max_depth=20), rcs()) == st


def test_python_front_end_rejects_bad_arguments():
    w, h = 16, 9
    job = Job(width=w, height=h, frames=4)
    buf = np.zeros((h, w, 4), np.float32)
    ok = np.ones((h, w), np.int32)
    for counts in (np.ones((h, w), np.int64), np.ones((h, w), np.float32), np.ones((h, w - 1), np.int32),
                   np.ones((h + 1, w), np.int32), np.ones((w, h), np.int32).T, [1] * (w * h)):
        with pytest.raises(LrtError):
            render_counts_host(job, buf, counts)
    with pytest.raises(LrtError):
        render_counts_host(job, buf[:4], ok)
    with pytest.raises(LrtError):
        render_counts_host(job, buf.astype(np.float64), ok)
    with pytest.raises(LrtError) as e:   # the library's own checks
        render_counts_host(job, buf, ok, capacity=0)
    assert e.value.code == L.LRT_E_INVALID and "capacity" in str(e.value)
    with pytest.raises(LrtError) as e:
        render_counts_host(Job(width=w, height=h, frames=4, flags=L.F_SIMPLE), buf, ok)
    assert e.value.code == L.LRT_E_INVALID
    # a window's counts have the window's shape
    win = Job(width=w, height=h, x0=3, x_count=5, frames=2)
    with pytest.raises(LrtError):
        render_counts_host(win, np.zeros((h, 5, 4), np.float32), ok)
    with pytest.raises(LrtError):        # host arrays are not tensors
        render_counts_tensor(job, buf, np.zeros(1, np.int64), ok, None)
