"""NumPy restatement of the G-buffer pass (include/lrt.h, lrt_gbuffer_*) in the kernel's own order of
operations, the cases its tests share, and the scenes they use. A helper module, not a conftest:
imported by tests/test_gbuffer_cpu.py and tests/test_gpu_gbuffer.py.

Per pixel (x, y), in `dtype` (np.float32: the kernel's arithmetic operation for operation;
np.float64: the reference the GPU test compares against):
  1. s = (x + 1/2) (1 / w), t = (y + 1/2) (1 / h); D = ((L + s H) + t V) - O; dir = D (1 / sqrt(D.D))
  2. the closest hit over (0.001, 1e7): HitSphere's arithmetic per sphere in index order
     (maths.cpp:51-94): rs = c - O, p = rs.dir, ifHit = rs.rs - p p - r r; with ifHit < 0 the roots
     p -+ sqrt(-ifHit), the first one inside (tMin, closest) wins
  3. P = O + dir t, n = normalize(P - c), the material's albedo; zero on a miss, id -1, depth +Inf
  4. motion: Xc' = c' + (r' / r) (P - c) if the sphere's eight floats differ between the scenes, else
     P; d = Xc' - O' (a miss: D); da = d.a', q = (-fd / da) d - (L' - O'),
     fx = (q.H') (1 / H'.H') w - 1/2, fy likewise; projectable iff da < 0, |fx|, |fy| < 1e6 and the
     sphere existed (r > 0 and r' > 0); bit-identical cameras and an unmoved point: fx = x, fy = y.
`fragile` marks the pixels one of whose decisions lies near its threshold: some sphere's
|ifHit| <= FRAGILE_REL r^2 (a grazing ray: hit or miss, and which sphere, may flip), and for the
motion |da| <= FRAGILE_REL |d| or |fx|, |fy| within FRAGILE_REL of 1e6.

`python tests/gbuffer_ref.py` prints the largest gap between the f32 and the f64 run over the GPU
test's cases (F32_F64_GAP of tests/test_gpu_gbuffer.py), the fragile share and the pixels whose
f32 and f64 ids differ, per case.
"""
import numpy as np

import temporal_ref as R

FRAGILE_REL = 1e-4
K_MIN_T, K_MAX_T = np.float32(0.001), np.float32(1.0e7)   # parallel.cpp:9-10
GUIDES = ("normal", "world_pos", "albedo")
SHAPES = ((1, 1), (5, 3), (19, 13), (67, 45), (257, 9), (160, 90))   # w x h; 67 x 45: partial tiles on both axes
DTHETA = 0.02
COUNTS = (1, 9, 16, 17, 1000, 4096)     # 17: the first count on the grid; 4096: LRT_MAX_SPHERES
COUNT_SIZE = (19, 13)
GRID_ABOVE = 16                         # kBvhMinSpheres


def sphere_array(spheres):
    """[count, 4] float32 (centre, radius) of ctypes Spheres, a flat list or an array."""
    if len(spheres) and hasattr(spheres[0], "center"):
        return np.array([[s.center.x, s.center.y, s.center.z, s.radius] for s in spheres], np.float32)
    return np.asarray(spheres, np.float32).reshape(-1, 4).copy()


def albedo_array(materials):
    """[count, 3] float32 of ctypes Materials, or of the oracle's 9 floats per material."""
    if len(materials) and hasattr(materials[0], "albedo"):
        return np.array([m.albedo.tolist() for m in materials], np.float32)
    return np.asarray(materials, np.float32).reshape(-1, 9)[:, 1:4].copy()


def _dot(a, b):
    return a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1] + a[..., 2] * b[..., 2]


def _normalize(v, T):
    return v * (T(1) / np.sqrt(_dot(v, v)))[..., None]


def primary_rays(w, h, camera, dtype=np.float32):
    """(O, D, dir): the pixel-centre rays of step 1, D [h, w, 3] before and dir after the normalize."""
    T = dtype
    c = R._cam(camera, T)
    ys, xs = np.mgrid[0:h, 0:w]
    s = ((xs.astype(T) + T(0.5)) * (T(1) / T(w)))[..., None]
    t = ((ys.astype(T) + T(0.5)) * (T(1) / T(h)))[..., None]
    D = ((c["L"] + s * c["H"]) + t * c["V"]) - c["O"]
    with np.errstate(all="ignore"):
        return c["O"], D, _normalize(D, T)


def accel_rays(w, h, camera):
    """lrt_accel_eval's input, [w h, 6] float32 (O, D): the f32 rays, which it normalises itself."""
    O, D, _ = primary_rays(w, h, camera, np.float32)
    return np.ascontiguousarray(np.concatenate([np.broadcast_to(O, D.shape), D], -1).reshape(-1, 6), np.float32)


def closest_hit(O, d, spheres, dtype):
    """(id [h, w] int32, t [h, w], grazing [h, w]) of step 2; t = kMaxT on a miss."""
    T = dtype
    s32 = sphere_array(spheres)
    cs, r2 = s32[:, :3].astype(T), (s32[:, 3].astype(T) * s32[:, 3].astype(T))
    closest = np.full(d.shape[:-1], T(K_MAX_T), T)
    ids = np.full(d.shape[:-1], -1, np.int32)
    grazing = np.zeros(d.shape[:-1], bool)
    tmin = T(K_MIN_T)
    with np.errstate(all="ignore"):
        for i in range(len(s32)):
            rs = cs[i] - O
            p = _dot(rs, d)
            if_hit = _dot(rs, rs) - p * p - r2[i]
            grazing |= np.abs(if_hit) <= T(FRAGILE_REL) * r2[i]
            half = np.sqrt(-if_hit)
            t1, t2 = p - half, p + half
            inside = if_hit < 0
            ok1 = inside & (t1 > tmin) & (t1 < closest)
            ok2 = inside & (t2 > tmin) & (t2 < closest)
            ids = np.where(ok1 | ok2, np.int32(i), ids)
            closest = np.where(ok1, t1, np.where(ok2, t2, closest))
    return ids, closest, grazing


def same_camera(camera, prev_camera):
    a, b = R.cam22(camera).view(np.uint32), R.cam22(prev_camera).view(np.uint32)
    keep = np.r_[0:6, 12:21]           # origin, a, lowerLeftCorner, horizontalVec, verticalVec
    return bool(np.array_equal(a[keep], b[keep]))


def gbuffer(w, h, camera, spheres, albedo, prev_camera=None, prev_spheres=None, guide_scale=1.0, motion=True,
            dtype=np.float64):
    """The six planes {"normal", "world_pos", "albedo" [h, w, 3], "id" [h, w] int32, "depth" [h, w],
    "motion" [h, w, 4]} in `dtype`, and the fragile mask. prev_camera None: the camera; prev_spheres
    None: no scene is given (nothing moved)."""
    T = dtype
    s32 = sphere_array(spheres)
    O, D, d = primary_rays(w, h, camera, T)
    ids, t, fragile = closest_hit(O, d, s32, T)
    hit = ids >= 0
    im = np.maximum(ids, 0)
    cs = s32[:, :3].astype(T)
    k = T(guide_scale)
    with np.errstate(all="ignore"):
        P = np.where(hit[..., None], O + d * t[..., None], T(0))
        n = np.where(hit[..., None], _normalize(P - cs[im], T), T(0))
    alb = np.where(hit[..., None], np.asarray(albedo, np.float32).astype(T)[im], T(0))
    out = dict(normal=k * n, world_pos=k * P, albedo=k * alb, id=ids,
               depth=np.where(hit, t, T(np.inf)))
    if not motion:
        return out, fragile
    pcm = R._cam(prev_camera if prev_camera is not None else camera, T)
    same = prev_camera is None or same_camera(camera, prev_camera)
    moved = np.zeros((h, w), bool)
    gone = np.zeros((h, w), bool)
    Xp = P
    if prev_spheres is not None:
        p32 = sphere_array(prev_spheres)
        assert p32.shape == s32.shape
        cand = (s32[:, 3] > 0) & (p32[:, 3] > 0)
        differs = (s32.view(np.uint32) != p32.view(np.uint32)).any(-1)
        moved = hit & (cand & differs)[im]
        gone = hit & ~cand[im]
        with np.errstate(all="ignore"):
            ratio = (p32[:, 3].astype(T) / s32[:, 3].astype(T))[im][..., None]
            Xp = np.where(moved[..., None], p32[:, :3].astype(T)[im] + ratio * (P - cs[im]), P)
    ys, xs = np.mgrid[0:h, 0:w]
    pO, pa = pcm["O"], pcm["a"]
    pLO = pcm["L"] - pO
    fd = -_dot(pLO, pa)
    with np.errstate(all="ignore"):
        tgt = np.where(hit[..., None], Xp - pO, D)
        da = _dot(tgt, pa)
        q = (-fd / da)[..., None] * tgt - pLO
        fx = _dot(q, pcm["H"]) * (T(1) / _dot(pcm["H"], pcm["H"])) * T(w) - T(0.5)
        fy = _dot(q, pcm["V"]) * (T(1) / _dot(pcm["V"], pcm["V"])) * T(h) - T(0.5)
        ok = (da < 0) & (np.abs(fx) < T(1e6)) & (np.abs(fy) < T(1e6))
        near = (np.abs(da) <= T(FRAGILE_REL) * np.sqrt(_dot(tgt, tgt))) | R._near(np.abs(fx), T(1e6)) | \
            R._near(np.abs(fy), T(1e6))
    centre = same & ~moved
    fragile = fragile | (~centre & ~gone & near)
    fx, fy, ok = np.where(centre, xs.astype(T), fx), np.where(centre, ys.astype(T), fy), (ok | centre) & ~gone
    mv = np.zeros((h, w, 4), T)
    mv[..., 0] = np.where(ok, fx - xs.astype(T), T(0))
    mv[..., 1] = np.where(ok, fy - ys.astype(T), T(0))
    mv[..., 2] = ids
    mv[..., 3] = ok
    out["motion"] = mv
    return out, fragile


# ---- the scenes and cameras the tests share
def count_scene(count, default_scene, random_scene):
    """(spheres, materials) of `count` spheres: the default scene's middle sphere, the default scene,
    or random_scene(count, 1)."""
    if count == 1:
        s, m = default_scene()
        return s[1:2], m[1:2]
    return default_scene() if count == 9 else random_scene(count, 1)


def camera_pair(make_camera, w, h, dtheta=DTHETA):
    """(camera, prev_camera): the default camera (parallel.cpp:299-307) and the one an orbit step of
    dtheta before it."""
    def at(theta):
        return make_camera((3.0 * np.sin(theta), 2.0, 3.0 * np.cos(theta)), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), 60.0,
                           w / h, 0.1, 3.0)
    return at(0.0), at(-dtheta)


def moved_scene(spheres):
    """The previous scene of the restatement cases: of the default scene (temporal_motion_ref's
    pair: a Lambert and a metal sphere elsewhere, a third of another radius), or of a larger scene
    (spheres 3 and 5 elsewhere, sphere 7 of another radius)."""
    prev = sphere_array(spheres)
    if len(prev) == 9:
        prev[2, :3] -= np.float32((0.12, 0.04, -0.08))
        prev[4, :3] -= np.float32((-0.1, 0.06, 0.05))
        prev[6, 3] = 0.42
    elif len(prev) > 7:
        prev[3, :3] += np.float32((0.05, 0.0, 0.03))
        prev[5, :3] -= np.float32((0.04, 0.0, 0.02))
        prev[7, 3] *= np.float32(1.25)
    else:
        prev[0, :3] += np.float32((0.1, -0.05, 0.02))
    return prev


def rel_gaps(a, b, ok):
    """The largest |a - b| / max(1, |b|) over the pixels of ok, per tolerance-checked plane."""
    return {name: R.rel_gap(a[name][..., :3] if name != "motion" else a[name][..., :2],
                            b[name][..., :3] if name != "motion" else b[name][..., :2], ok)
            for name in GUIDES + ("motion",) if name in b}


def f32_f64_gap(cases):
    """The largest f32 - f64 gap over [(label, gbuffer's arguments)], off the fragile mask, and per
    case (fragile share, pixels whose ids differ, of those not fragile)."""
    worst, report = 0.0, {}
    for label, kw in cases:
        a, fa = gbuffer(dtype=np.float32, **kw)
        b, fb = gbuffer(dtype=np.float64, **kw)
        ok = ~(fa | fb)
        differ = a["id"] != b["id"]
        report[label] = (float(fb.mean()), int(differ.sum()), int((differ & ok).sum()))
        ok &= ~differ
        assert np.array_equal(a["motion"][..., 2:][ok], b["motion"][..., 2:][ok]), label
        worst = max(worst, *rel_gaps(a, b, ok).values())
    return worst, report


def gap_cases(default_scene, random_scene, make_camera):
    """The GPU test's restatement cases: the default scene at SHAPES and COUNTS at COUNT_SIZE, one
    orbit step, spheres moved (moved_scene)."""
    cases = []
    for w, h in SHAPES:
        s, m = default_scene()
        cam, pcam = camera_pair(make_camera, w, h)
        cases.append((f"{w}x{h}", dict(w=w, h=h, camera=cam, spheres=s, albedo=albedo_array(m), prev_camera=pcam,
                                       prev_spheres=moved_scene(s))))
    for count in COUNTS:
        w, h = COUNT_SIZE
        s, m = count_scene(count, default_scene, random_scene)
        cam, pcam = camera_pair(make_camera, w, h)
        cases.append((f"count {count}", dict(w=w, h=h, camera=cam, spheres=s, albedo=albedo_array(m),
                                             prev_camera=pcam, prev_spheres=moved_scene(s))))
    return cases


# ---- the designed motion cases: two spheres in front of a pinhole camera on the z axis, sky around them
DESIGNED_SIZE = (37, 21)
DESIGNED_ALBEDO = np.float32([[0.8, 0.3, 0.2], [0.2, 0.4, 0.9]])
ANALYTIC_DX = 0.3
_A, _B = [-0.9, 0.0, 0.0, 0.7], [0.9, 0.0, 0.0, 0.7]
_EYE, _SHIFTED, _ORIGIN = (0.0, 0.0, 3.0), (0.1, 0.05, 3.0), (0.0, 0.0, 0.0)
DESIGNED_CASES = {   # name: (prev spheres or None, prev look_from or None: the same camera, passed as the same bits)
    "static": (None, None),                                                # no scene given
    "static_scene": ([_A, _B], None),                                      # a scene given, nothing moved
    "moved": ([[-0.8, 0.1, 0.0, 0.55], [0.6, -0.25, 0.2, 0.7]], _SHIFTED),  # A resized and moved, B translated
    "behind": ([_A, [0.9, 0.0, 6.0, 0.7]], _SHIFTED),                      # B came from behind the previous camera
    "gone": ([_A, [0.9, 0.0, 0.0, 0.0]], _SHIFTED),                        # B was not there: r' = 0
    "analytic": ([_A, [0.9 - ANALYTIC_DX, 0.0, 0.0, 0.7]], None),          # B translated along x under one camera
}


def designed_case(name, make_camera):
    """gbuffer()'s arguments of one designed case (spheres: the current scene, A and B)."""
    w, h = DESIGNED_SIZE
    prev, look_from = DESIGNED_CASES[name]
    cam = make_camera(*R._cam_args(_EYE, _ORIGIN, w, h))
    pcam = None if look_from is None else make_camera(*R._cam_args(look_from, _ORIGIN, w, h))
    return dict(w=w, h=h, camera=cam, spheres=np.float32([_A, _B]), albedo=DESIGNED_ALBEDO, prev_camera=pcam,
                prev_spheres=None if prev is None else np.float32(prev))


def analytic_displacement(h, depth):
    """The pixel displacement along x (previous minus current) of a point `depth` in front of the
    `analytic` case's camera when its sphere came from ANALYTIC_DX to the left
    (temporal_motion_ref.analytic_displacement)."""
    return -ANALYTIC_DX * h / (2.0 * np.tan(np.radians(R.VFOV / 2)) * depth)


if __name__ == "__main__":
    import os
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [root]
    from learnraytracing_amd import default_scene, make_camera, random_scene

    cases = gap_cases(default_scene, random_scene, make_camera)
    designed = [(name, designed_case(name, make_camera)) for name in DESIGNED_CASES]
    for title, group in (("the default scene at SHAPES", cases[:len(SHAPES)]),
                         ("counts up to 17", [c for c in cases[len(SHAPES):] if len(c[1]["spheres"]) <= 17]),
                         ("count 1000", [c for c in cases if len(c[1]["spheres"]) == 1000]),
                         ("count 4096", [c for c in cases if len(c[1]["spheres"]) == 4096]),
                         ("the designed cases", designed)):
        gap, report = f32_f64_gap(group)
        print(f"largest f32 - f64 gap off the fragile mask over {title}: {gap:.3g}")
        for label, (share, differ, differ_ok) in report.items():
            print(f"  {label}: fragile {100 * share:.2f} %, ids differ at {differ} px ({differ_ok} of them not fragile)")
