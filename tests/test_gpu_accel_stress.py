"""The device's BVH and grid walks on the rays that stress a DDA, against the reference's HitWorld.

test_grid_host.py and test_bvh_host.py run the host build of the device traversal on axis-aligned
rays, rays in cell planes and through lattice corners, grazing rays over the flat field, rays
leaving sphere surfaces, NaN / inf / zero-radius / coincident spheres, tiny scenes, a colinear
chain and the adversarial scenes. The device build differs from the host build in exactly the
places those rays probe (contraction, the short sqrt / rcp sequences), so the same families --
built by the same functions -- run here through lrt_accel_eval's device modes: the BVH per lane
(1, 1) and as a packet (1, 2), and the grid (2, 1). (id, t) must equal the reference's own
HitSphere looped over the sphere array (oracle.ref_hit_spheres; HitWorld's loop,
parallel.cpp:54-73, maths.cpp:51-94) bit for bit. 4096 rays a case: whole waves for the packet.
"""
import functools

import numpy as np
import pytest

import oracle
from learnraytracing_amd.scene import random_scene
from test_bvh_host import adversarial_scene, chain_rays, colinear_chain, random_rays, stats
from test_exact_far import _need_ref, accel, assert_same, sphere_array
from test_grid_host import (FIELD_BOX, SMALL_BOX, SMALL_SCENES, axis_plane_and_corner_rays, big_spheres_scene,
                            degenerate_scene, far_origin_rays, grazing_and_surface_rays, gstats, small_scene)

pytestmark = pytest.mark.gpu

N = 4096   # rays per case: a multiple of 64
PATHS = [(1, 1, "bvh-lane"), (1, 2, "bvh-packet"), (2, 1, "grid")]   # lrt_accel_eval's (accel, mode)


def _adversarial(seed):
    g = np.random.default_rng(300 + seed)
    sph = adversarial_scene(g, int(g.integers(20, 600)))
    return sph, random_rays(g, N, -25, 25)


def _lattice():
    sph, _ = random_scene(1000, 1)
    return sph, axis_plane_and_corner_rays(np.random.default_rng(21), sph, per_axis=256, lattice=N - 6 * 256)


def _grazing():
    sph, _ = random_scene(1000, 1)
    return sph, grazing_and_surface_rays(np.random.default_rng(22), sph, ground=N // 2, surface=N // 2)


def _degenerate():
    return degenerate_scene(), random_rays(np.random.default_rng(24), N, *FIELD_BOX)


def _big_only():
    g = np.random.default_rng(25)
    return big_spheres_scene(g), random_rays(g, N, -10, 10)


def _chain():
    n = 4096
    return colinear_chain(n), chain_rays(np.random.default_rng(26), n, across=N - 128, along=128)


def _far():
    sph, _ = random_scene(300, 2)
    return sph, far_origin_rays(np.random.default_rng(23), N)


FAMILIES = {
    "adversarial0": lambda: _adversarial(0),
    "adversarial1": lambda: _adversarial(1),
    "axis_plane_corner": _lattice,
    "grazing_surface": _grazing,
    "non_finite_degenerate": _degenerate,
    "big_spheres_only": _big_only,
    "colinear_chain": _chain,
    "far_origins": _far,
}
FAMILIES.update({f"small{n}": lambda n=n: (small_scene(n), random_rays(np.random.default_rng(50 + n), N, *SMALL_BOX))
                 for n in SMALL_SCENES})


@functools.lru_cache(maxsize=None)
def _case(family):
    """(spheres, rays, the reference's (ids, ts)): built once and shared by the device paths."""
    sph, rays = FAMILIES[family]()
    assert len(rays) == N and N % 64 == 0
    want = oracle.ref_hit_spheres(rays, sphere_array(sph))
    for a in (rays, *want):
        a.setflags(write=False)
    return sph, rays, want


# (the BVH needs two spheres: the one-sphere scene runs the grid alone)
CASES = [pytest.param(f, acc, mode, id=f"{f}-{name}") for f in sorted(FAMILIES) for acc, mode, name in PATHS
         if not (f == "small1" and acc == 1)]


@pytest.mark.parametrize("family,acc,mode", CASES)
def test_stress_rays_device_vs_reference(gpu, family, acc, mode):
    _need_ref()
    sph, rays, want = _case(family)
    hits = float((want[0] >= 0).mean())
    print(f"{family}: {len(sph)} spheres, hit fraction {hits:.3f}")
    assert hits > 0.2, hits   # the rays do hit (the reference's scan: 0.27 for the chain, 0.42 and more elsewhere)
    if family == "far_origins":   # the host walk of these very rays finishes with the scan
        assert gstats(sph, rays)[4] > 0.5
    if acc == 1:   # no traversal of these rays writes past the traversal stack (test_bvh_host.stats)
        stats(sph, rays)
    assert_same(accel(sph, rays, acc, mode), want, f"{family} device {acc}/{mode}")
