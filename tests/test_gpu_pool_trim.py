"""The pool kernel's trimmed fixed-scene instance and what selects it (lrt_pool.h, lrt_pool_launch.h).

A 9-sphere scene with one light whose radii all satisfy r*r >= 2^-70 runs pool_kernel with a
compile-time light count of 1 and closest-hit roots that skip their range check
(lrt_last_launch(): ns=9 nl=1 chk=0). Every instance's path start reads the window, the row
map and the camera in one batch and takes y = y0 + ly without a division when the row map is
the identity. Every other scene keeps the general instances (chk=1, nl=0). All of it must leave the bits and the ray counts of the C
restatement (oracle.orc_render) unchanged. References: parallel.cpp:54-73 (HitWorld),
:78-136 (Lambert's light loop), :214 (the fold), :262,280-286 (the lerp chain).
"""
import copy
import functools

import numpy as np
import pytest

import oracle
from learnraytracing_amd import _lib as L
from learnraytracing_amd.scene import scene_arrays

pytestmark = pytest.mark.gpu

V0, POOL = 2, 512   # LRT_F_SIMPLE (trace_kernel), LRT_F_POOL (pool_kernel)
W, H = 1280, 720
# 200 columns are no multiple of the 16-wide tiles, and the second window is no multiple of
# the 8x8 tiles either: edge tiles and lanes outside the window run
WIN = dict(x0=100, x_count=200, y0=40, row_count=72)
WIN_ODD = dict(x0=101, x_count=203, y0=41, row_count=75)


def _bitwise(got, want, what):
    g = got[..., :3]
    if not np.array_equal(g.view(np.uint32), np.ascontiguousarray(want[..., :3]).view(np.uint32)):
        d = np.abs(g.astype(np.float64) - want[..., :3].astype(np.float64))
        raise AssertionError(f"{what}: {int((g != want[..., :3]).any(axis=-1).sum())} pixels differ, "
                             f"max |diff| {d.max():.3g}")


def _render(gpu, flags, **kw):
    job = gpu.Job(flags=flags, width=W, height=H, **kw)
    d = job.desc()
    buf = np.zeros((d.row_count, d.x_count, 4), np.float32)
    rays = gpu.render_host(job, buf)
    return buf, rays, L.last_launch()


@functools.lru_cache(maxsize=None)
def _want(frames, depth, x0, xc, y0, yc, scene=None):
    """The restatement's window, computed once per case and shared."""
    s = m = None
    if scene is not None:
        s, m = (np.array(v, np.float32) for v in SCENES[scene]())
    buf, rays = oracle.orc_render(W, H, frames, depth, 0, x0, xc, y0, yc, spheres=s, mats=m, threads=16)
    buf.setflags(write=False)
    return buf, rays


def _default():
    import learnraytracing_amd as lrt
    sph, mat = lrt.default_scene()
    return [copy.copy(x) for x in sph], [copy.copy(x) for x in mat]


def _tiny_radius():
    """The reference scene with one radius of 1e-12: r*r = 1e-24 < 2^-70, outside the proof."""
    sph, mat = _default()
    sph[3].radius = 1e-12
    return sph, mat


def _ten_spheres():
    sph, mat = _default()
    sph.append(L.Sphere(L.f3(-1.2, 0.6, 0.5), 0.3))   # inside the window's view
    mat.append(L.Material(L.LAMBERT, L.f3(0.3, 0.7, 0.4), L.f3(0, 0, 0), 0.0, 0.0))
    return sph, mat


def _two_lights():
    sph, mat = _default()
    k = next(i for i, x in enumerate(mat) if (x.emissive.x, x.emissive.y, x.emissive.z) == (0, 0, 0) and i > 0)
    mat[k].emissive = L.f3(4.0, 6.0, 8.0)
    return sph, mat


SCENES = {"tiny_radius": lambda: scene_arrays(*_tiny_radius()), "ten_spheres": lambda: scene_arrays(*_ten_spheres()),
          "two_lights": lambda: scene_arrays(*_two_lights())}
BUILD = {"tiny_radius": _tiny_radius, "ten_spheres": _ten_spheres, "two_lights": _two_lights}


@pytest.fixture
def scene(gpu, request):
    """A scene of BUILD for one test, then the default scene again (conftest's scene guard)."""
    gpu.set_scene(*BUILD[request.param]())
    try:
        yield request.param
    finally:
        gpu.set_scene(*gpu.default_scene())


def _check(gpu, flags, frames, depth, win, scene=None, **shard):
    buf, rays, info = _render(gpu, flags, frames=frames, max_depth=depth, **win, **shard)
    want, wrays = _want(frames, depth, win["x0"], win["x_count"], win["y0"], win["row_count"], scene)
    samples = frames * win["x_count"] * win["row_count"]   # one camera ray each, bounces on top
    assert wrays == samples if depth == 0 else wrays > 2 * samples, wrays
    _bitwise(buf, want, f"frames {frames} depth {depth} {scene or 'default'} flags {flags}")
    assert rays == wrays
    return info


@pytest.mark.parametrize("win", [WIN, WIN_ODD], ids=["window", "odd-window"])
@pytest.mark.parametrize("frames,depth", [(4, 8), (5, 8), (4, 3), (4, 0)])
def test_trimmed_instance_vs_oracle(gpu, frames, depth, win):
    """The default scene runs the trimmed instance, on the identity row map."""
    info = _check(gpu, POOL, frames, depth, win)
    assert info["kernel"] == "pool_kernel" and info["ns"] == "9" and info["nl"] == "1" and info["chk"] == "0", info


def test_row_block_cyclic_shard_vs_oracle(gpu):
    """row_period 2: the refill's and the frame store's division path. Local rows 8b.. of the
    shard are global rows y0 + 16b + 8 .. of the frame."""
    rb, rp, ph = 8, 2, 1
    buf, rays, info = _render(gpu, POOL, frames=4, max_depth=8, row_block=rb, row_period=rp, row_phase=ph, **WIN)
    assert info["kernel"] == "pool_kernel" and info["nl"] == "1" and info["chk"] == "0", info
    total = 0
    for band in range(WIN["row_count"] // rb):
        gy = WIN["y0"] + band * rb * rp + ph * rb
        want, wr = _want(4, 8, WIN["x0"], WIN["x_count"], gy, rb)
        _bitwise(buf[band * rb:(band + 1) * rb], want, f"shard band {band}")
        total += wr
    assert rays == total and total > 0


@pytest.mark.parametrize("scene", ["tiny_radius"], indirect=True)
def test_radius_outside_the_proof_keeps_checked_roots(gpu, scene):
    """r*r = 1e-24 is below 2^-70: the launch keeps the range-checked instance."""
    info = _check(gpu, POOL, 4, 8, WIN, scene)
    assert info["kernel"] == "pool_kernel" and info["ns"] == "9" and info["chk"] == "1", info


@pytest.mark.parametrize("scene", ["ten_spheres", "two_lights"], indirect=True)
def test_other_scenes_keep_general_instances(gpu, scene):
    """Ten spheres: no fixed-scene instance; two lights: the run-time light loop."""
    info = _check(gpu, POOL, 4, 8, WIN, scene)
    assert info["kernel"] == "pool_kernel" and info["nl"] != "1" and info["chk"] == "1", info
    assert info["ns"] == ("0" if scene == "ten_spheres" else "9"), info


@pytest.mark.parametrize("frames,depth", [(4, 8), (5, 8), (4, 3), (4, 0)])
def test_v0_same_window_vs_oracle(gpu, frames, depth):
    """The same window through trace_kernel (the shared normalize and argument layout)."""
    info = _check(gpu, V0, frames, depth, WIN)
    assert info["kernel"] == "trace_kernel", info
