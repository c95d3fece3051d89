"""The kernels' Scatter with the materials' shared work issued once per bounce (lrt_trace.h ScatterDir:
dot(r_in.dir, rec.normal), reflect and the scatter's first three draws ahead of the material switch)
and the scan's root selection with one root chosen first (SphereRoots).

None of it may change a bit or a counted ray of the C restatement (oracle.orc_render_ex). Every case
renders a small window of the 1280 x 720 view -- 37 x 21 (no multiple of the 8x8 or the 16x8 tile:
ragged right column and top row, lanes outside the window) or 32 x 16 -- and compares RGB and the ray
count bit for bit; lrt_last_launch() names the instance that ran. Scenes of one material each send
every lane of a wave through the same branch, the default scene mixes the three. References:
parallel.cpp:78-196 (Scatter), maths.cpp:7-49 (the draws), maths.cpp:61-90 (the roots).
"""
import copy
import functools

import numpy as np
import pytest

import oracle
from learnraytracing_amd import _lib as L
from learnraytracing_amd.scene import scene_arrays
from test_gpu_pool_trim import _bitwise
from test_scatter import check_scene, scenes

pytestmark = pytest.mark.gpu

V0, WF, POOL = 2, 256, 512   # LRT_F_SIMPLE (trace_kernel), LRT_F_WAVEFRONT, LRT_F_POOL
W, H = 1280, 720
WINS = {"37x21": dict(x0=440, x_count=37, y0=270, row_count=21),   # spheres, ground and sky
        "32x16": dict(x0=448, x_count=32, y0=272, row_count=16)}


def _default():
    import learnraytracing_amd as lrt
    sph, mat = lrt.default_scene()
    return [copy.copy(x) for x in sph], [copy.copy(x) for x in mat]


def _metals():
    sph, mat = _default()
    return sph, [L.Material(L.METAL, m.albedo, m.emissive, 1.0, 0.0) for m in mat]


def _dielectrics():
    sph, mat = _default()
    return sph, [L.Material(L.DIELECTRIC, m.albedo, m.emissive, 0.0, (1.5, 2.4, 0.5)[i % 3]) for i, m in enumerate(mat)]


def _lamberts():
    """Nine Lamberts; the default scene's light stays the only light (and is a Lambert itself)."""
    sph, mat = _default()
    return sph, [L.Material(L.LAMBERT, m.albedo, m.emissive, 0.0, 0.0) for m in mat]


def _ten_spheres_two_lights():
    sph, mat = _default()
    k = next(i for i, x in enumerate(mat) if (x.emissive.x, x.emissive.y, x.emissive.z) == (0, 0, 0) and i > 0)
    mat[k].emissive = L.f3(4.0, 6.0, 8.0)
    sph.append(L.Sphere(L.f3(-1.2, 0.6, 0.5), 0.3))
    mat.append(L.Material(L.LAMBERT, L.f3(0.3, 0.7, 0.4), L.f3(0, 0, 0), 0.0, 0.0))
    return sph, mat


BUILD = {"metals": _metals, "dielectrics": _dielectrics, "lamberts": _lamberts,
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
def _want(win, frames, depth, scene=None):
    """The restatement's window, computed once per case and shared."""
    s = m = None
    if scene is not None:
        s, m = (np.array(v, np.float32) for v in scene_arrays(*BUILD[scene]()))
    w = WINS[win]
    buf, rays = oracle.orc_render_ex(W, H, frames, depth, 0, w["x0"], w["x_count"], w["y0"], w["row_count"],
                                     spheres=s, mats=m, flags=0, threads=16)
    buf.setflags(write=False)
    return buf, rays


def _check(gpu, win, frames, depth, scene=None, flags=POOL):
    w = WINS[win]
    job = gpu.Job(flags=flags, width=W, height=H, frames=frames, max_depth=depth, **w)
    buf = np.zeros((w["row_count"], w["x_count"], 4), np.float32)
    rays = gpu.render_host(job, buf)
    info = L.last_launch()
    want, wrays = _want(win, frames, depth, scene)
    samples = frames * w["x_count"] * w["row_count"]
    print(f"{scene or 'default'} {win} frames {frames} depth {depth} flags {flags}: {rays} rays (oracle {wrays}), "
          f"{wrays / samples:.2f} per sample; {info}")
    assert wrays > samples, wrays   # no window of sky
    _bitwise(buf, want, f"{scene or 'default'} {win} frames {frames} depth {depth} flags {flags}")
    assert rays == wrays
    return info


def _is_trimmed(info):
    return (info["kernel"] == "pool_kernel" and info["maxd"] == "8" and info["ns"] == "9" and info["nl"] == "1"
            and info["chk"] == "0" and info["wpb"] == "1")


@pytest.mark.parametrize("depth", [8, 1])
@pytest.mark.parametrize("frames", [1, 4, 5])
@pytest.mark.parametrize("win", ["37x21", "32x16"])
def test_default_scene_trimmed_64px_vs_oracle(gpu, win, frames, depth):
    info = _check(gpu, win, frames, depth)
    assert _is_trimmed(info) and info["pix"] == "64", info


@pytest.mark.parametrize("win", ["37x21", "32x16"])
def test_default_scene_trimmed_128px_vs_oracle(gpu, pix128, win):
    info = _check(gpu, win, 4, 8)
    assert _is_trimmed(info) and info["pix"] == "128", info


@pytest.mark.parametrize("win,frames,depth", [("37x21", 4, 8), ("32x16", 5, 1), ("32x16", 1, 8)])
@pytest.mark.parametrize("scene", ["metals", "dielectrics", "lamberts"], indirect=True)
def test_one_material_scenes_vs_oracle(gpu, scene, win, frames, depth):
    """Nine metals of roughness 1 (rejected candidates, absorption), nine dielectrics of ri 0.5 / 1.5 /
    2.4 (both sides, total reflection), nine Lamberts of which one is the light (no third draw there):
    nine spheres and one light, so the trimmed instance."""
    assert _is_trimmed(_check(gpu, win, frames, depth, scene))


@pytest.mark.parametrize("win,frames,depth,maxd", [("37x21", 4, 8, "8"), ("32x16", 5, 1, "8"), ("32x16", 4, 9, "64")])
@pytest.mark.parametrize("scene", ["ten_two_lights"], indirect=True)
def test_general_instances_vs_oracle(gpu, scene, win, frames, depth, maxd):
    """Ten spheres, two lights: the general scan instances (run-time counts, checked roots), whose
    light loop draws after an undeferred sample."""
    info = _check(gpu, win, frames, depth, scene)
    assert info["kernel"] == "pool_kernel" and info["maxd"] == maxd, info
    assert info["ns"] == "0" and info["chk"] == "1" and info["nl"] == "0", info


def test_depth_50_vs_oracle(gpu):
    """The depth-64 unit."""
    info = _check(gpu, "32x16", 4, 50)
    assert info["kernel"] == "pool_kernel" and info["maxd"] == "64", info


@pytest.mark.parametrize("flags,kernel", [(V0, "trace_kernel"), (WF, "wf_extend")], ids=["v0", "wavefront"])
def test_other_kernels_same_window_vs_oracle(gpu, flags, kernel):
    """trace_kernel and the wavefront kernels share ScatterDir and the scan."""
    info = _check(gpu, "37x21", 4, 8, flags=flags)
    assert info["kernel"] == kernel, info


@pytest.mark.parametrize("mode", [1, 2], ids=["per_lane", "packet"])
@pytest.mark.parametrize("sc", [t for t in scenes() if t[0] in ("default", "fuzz7", "scene1000")], ids=lambda t: t[0])
def test_scatter_device_matches_reference(gpu, sc, mode):
    """lrt_scatter_eval's device legs: one thread per case, 64 unrelated cases a wave, so that the
    three branches run one after the other behind the shared head."""
    check_scene(*sc, on_device=mode, n_cases=400)
