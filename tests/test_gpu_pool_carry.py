"""The pool kernel's bounce loop with its carried path state written once per iteration (lrt_pool.h).

The loop's carried values -- the ray, the deferred light, carry, pend, prevLambert, depth, the
slim instance's packed ids, state -- are read by the hit pass and the material code and written at
the bottom of the iteration, from temporaries the material code leaves; the pending event's stack
entry keeps the id it was given; the refill stage is a loop of its own. None of it may change a
bit or a counted ray of the C restatement (oracle.orc_render / orc_render_ex).

Every case renders one 67 x 45 window of the 1280 x 720 default view (no multiple of the 8x8 or
the 16x8 tile: partial right column and top row, lanes outside the window) and compares RGB and
the ray count bit for bit; lrt_last_launch() names the instance that ran. The 128-px tiles, which
the policy gives only to an overlapping launch with a tile per resident wave, are asked for through
lrt_pool_force_pix (include/lrt_diag.h). References: parallel.cpp:200-227 (Trace), :78-196
(Scatter, :147 Metal's absorption), :214 (the fold), :262,280-286 (the lerp chain).
"""
import copy
import functools

import numpy as np
import pytest

import oracle
from learnraytracing_amd import _lib as L
from learnraytracing_amd.scene import scene_arrays
from test_gpu_pool_trim import _bitwise

pytestmark = pytest.mark.gpu

POOL, NDL = 512, 64   # LRT_F_POOL, LRT_F_NO_DOUBLE_LIGHT
W, H = 1280, 720
WIN = dict(x0=420, x_count=67, y0=260, row_count=45)   # spheres, ground and sky: 3.6 rays per sample at depth 8


def _default():
    import learnraytracing_amd as lrt
    sph, mat = lrt.default_scene()
    return [copy.copy(x) for x in sph], [copy.copy(x) for x in mat]


def _all_of(kind, roughness, ri):
    """The default scene's spheres, every material of one type; albedo and emissive as they are
    (the light stays a light)."""
    sph, mat = _default()
    for i, m in enumerate(mat):
        mat[i] = L.Material(kind, m.albedo, m.emissive, roughness, ri)
    return sph, mat


def _ten_spheres_two_lights():
    sph, mat = _default()
    k = next(i for i, x in enumerate(mat) if (x.emissive.x, x.emissive.y, x.emissive.z) == (0, 0, 0) and i > 0)
    mat[k].emissive = L.f3(4.0, 6.0, 8.0)
    sph.append(L.Sphere(L.f3(-1.2, 0.6, 0.5), 0.3))
    mat.append(L.Material(L.LAMBERT, L.f3(0.3, 0.7, 0.4), L.f3(0, 0, 0), 0.0, 0.0))
    return sph, mat


BUILD = {"metals": lambda: _all_of(L.METAL, 1.0, 0.0), "dielectrics": lambda: _all_of(L.DIELECTRIC, 0.0, 1.5),
         "ten_two_lights": _ten_spheres_two_lights}


@pytest.fixture
def scene(gpu, request):
    """A scene of BUILD (None: the default) for one test, then the default scene again."""
    name = getattr(request, "param", None)
    if name is None:
        yield None
        return
    gpu.set_scene(*BUILD[name]())
    try:
        yield name
    finally:
        gpu.set_scene(*gpu.default_scene())


@pytest.fixture
def pix128():
    L.check(L.lib().lrt_pool_force_pix(128))
    try:
        yield
    finally:
        L.check(L.lib().lrt_pool_force_pix(0))


@functools.lru_cache(maxsize=None)
def _want(frames, depth, scene=None, flags=0):
    """The restatement's window, computed once per case and shared."""
    s = m = None
    if scene is not None:
        s, m = (np.array(v, np.float32) for v in scene_arrays(*BUILD[scene]()))
    buf, rays = oracle.orc_render_ex(W, H, frames, depth, 0, WIN["x0"], WIN["x_count"], WIN["y0"], WIN["row_count"],
                                     spheres=s, mats=m, flags=flags, threads=16)
    buf.setflags(write=False)
    return buf, rays


def _check(gpu, frames, depth, scene=None, flags=0):
    job = gpu.Job(flags=POOL | flags, width=W, height=H, frames=frames, max_depth=depth, **WIN)
    buf = np.zeros((WIN["row_count"], WIN["x_count"], 4), np.float32)
    rays = gpu.render_host(job, buf)
    info = L.last_launch()
    want, wrays = _want(frames, depth, scene, flags)
    samples = frames * WIN["x_count"] * WIN["row_count"]   # one camera ray each, bounces on top
    print(f"{scene or 'default'} frames {frames} depth {depth} flags {flags}: {rays} rays (oracle {wrays}), "
          f"{wrays / samples:.2f} per sample; {info}")
    assert wrays > samples, wrays   # no window of sky
    _bitwise(buf, want, f"{scene or 'default'} frames {frames} depth {depth} flags {flags} pix {info['pix']}")
    assert rays == wrays
    assert info["kernel"] == "pool_kernel", info
    return info


def _is_trimmed(info):
    return info["maxd"] == "8" and info["ns"] == "9" and info["nl"] == "1" and info["chk"] == "0" and info["wpb"] == "1"


def test_trimmed_instance_64px_vs_oracle(gpu):
    info = _check(gpu, 4, 8)
    assert _is_trimmed(info) and info["pix"] == "64" and info["per_cu"] == "20", info


def test_trimmed_instance_128px_vs_oracle(gpu, pix128):
    """6 x 5 tiles of 16 x 8 px, the benchmark's overlapped launches' tile."""
    info = _check(gpu, 4, 8)
    assert _is_trimmed(info) and info["pix"] == "128" and info["tasks"] == "30" and info["per_cu"] == "20", info


@pytest.mark.parametrize("frames", [1, 5])
def test_one_and_five_frames_vs_oracle(gpu, frames):
    """One frame: a pool (64 samples of a tile's edge) smaller than a wave's lanes want; five: the
    lerp's tail after its four-at-a-time chain."""
    assert _is_trimmed(_check(gpu, frames, 8))


def test_depth_one_vs_oracle(gpu):
    """The depth < maxDepth cut at the first level (depth 8, above, cuts at the last)."""
    assert _is_trimmed(_check(gpu, 4, 1))


def test_no_double_light_vs_oracle(gpu):
    """prevLambert: a Lambert hit after a Lambert scatter drops its emission."""
    assert _is_trimmed(_check(gpu, 4, 8, flags=NDL))


@pytest.mark.parametrize("scene", ["metals"], indirect=True)
def test_nine_rough_metals_vs_oracle(gpu, scene):
    """Roughness 1: about half the scatters point below the surface and are absorbed."""
    info = _check(gpu, 4, 8, scene)
    assert info["maxd"] == "8" and info["ns"] == "9", info


@pytest.mark.parametrize("scene", ["dielectrics"], indirect=True)
def test_nine_dielectrics_vs_oracle(gpu, scene):
    info = _check(gpu, 4, 8, scene)
    assert info["maxd"] == "8" and info["ns"] == "9", info


@pytest.mark.parametrize("depth,maxd", [(8, "8"), (9, "64")])
@pytest.mark.parametrize("scene", ["ten_two_lights"], indirect=True)
def test_general_instances_vs_oracle(gpu, scene, depth, maxd):
    """Ten spheres, two lights: the general scan instance (float4 stack levels, run-time counts);
    at depth 9 the depth-64 unit with one level in the global overflow stack."""
    info = _check(gpu, 4, depth, scene)
    assert info["maxd"] == maxd and info["ns"] == "0" and info["chk"] == "1" and info["nl"] == "0", info
