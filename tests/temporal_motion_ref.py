"""NumPy restatement of temporal accumulation under moving spheres (include/lrt.h,
lrt_temporal_accumulate_moving_*), the cases its tests share and the scene pairs they render. A
helper module, not a conftest: imported by tests/test_temporal_motion_cpu.py and
tests/test_gpu_temporal_motion.py.

The rule is tests/temporal_ref.py's steps 1-7 with, for `count` spheres (c_i, r_i) of the current
scene and (c'_i, r'_i) of the scene behind the previous state:
  2a. hit pixels only: n^ = N / |N|, s_i = |X - (c_i + r_i n^)|^2 over the candidates (r_i > 0 and
      r'_i > 0); i* = the smallest s_i (lowest index on a tie); matched iff
      s_i* <= pos_tol^2 |X - O|^2
  3a. matched, and sphere i*'s eight floats differ in a bit: Xc' = c'_i* + (r'_i* / r_i*) (Xc - c_i*);
      else Xc' = Xc (no arithmetic). d = Xc' - O' for a hit
  5a. the position test is |X'(Q) - Xc'|^2 <= pos_tol^2 |Xc - O|^2
  motion = (fx - x, fy - y, i* or -1, 1) where step 4 found a projectable point, else (0, 0, id, 0)

`python tests/temporal_motion_ref.py` prints the largest gap between the f32 and the f64 run over
the GPU test's rendered cases (F32_F64_GAP* of tests/test_gpu_temporal_motion.py), over the designed
sphere cases (F32_F64_GAP*_DESIGNED) and over the count cases (F32_F64_GAP_COUNT), with the share of
fragile pixels per case. QUALITY_RATIO is measured by
tests/test_temporal_motion_cpu.py::test_quality_moving_sphere.
"""
import numpy as np

import temporal_ref as R

DEFAULTS, FRAGILE_REL, OUTPUTS = R.DEFAULTS, R.FRAGILE_REL, R.OUTPUTS
MOTION_OUTPUTS = OUTPUTS + ("motion",)
INFO_MASKS = R.INFO_MASKS + ("matched", "moved", "touching")
INFO_COUNTS = R.INFO_COUNTS
CHUNK = 256   # spheres scored at a time (memory only)


def sphere_array(spheres):
    """[count, 4] float32 (centre, radius) of a list of ctypes Spheres, a flat list or an array."""
    if len(spheres) and hasattr(spheres[0], "center"):
        return np.array([[s.center.x, s.center.y, s.center.z, s.radius] for s in spheres], np.float32)
    return np.asarray(spheres, np.float32).reshape(-1, 4).copy()


def step(color, cur, prev, camera, prev_camera, spheres, prev_spheres, dtype=np.float64, info=None, **params):
    """One step of the moving form; arguments and returns as temporal_ref.step, plus spheres and
    prev_spheres ([count, 4] float32: centre, radius). The state holds "motion" [h, w, 4] besides
    OUTPUTS. fragile additionally marks the hit pixels whose match test lies within FRAGILE_REL of
    its threshold and those whose best and second-best scores lie within FRAGILE_REL of each other.
    info also gets matched, moved (matched to a sphere whose eight floats differ), touching (a hit
    whose X lies within the match threshold of two candidates' surfaces), id (int, -1 unmatched),
    best, second and thr (the two smallest scores and the threshold)."""
    p = dict(DEFAULTS, **params)
    T = dtype
    k = T(p["cur_scale"])
    C = k * np.asarray(color)[..., :3].astype(T)
    N = k * np.asarray(cur["normal"])[..., :3].astype(T)
    X = k * np.asarray(cur["world_pos"])[..., :3].astype(T)
    h, w = C.shape[:2]
    out = {"normal": N, "world_pos": X}
    if cur.get("albedo") is not None:
        out["albedo"] = k * np.asarray(cur["albedo"])[..., :3].astype(T)
    s32, p32 = sphere_array(spheres), sphere_array(prev_spheres)
    assert s32.shape == p32.shape and len(s32) >= 1
    fragile = np.zeros((h, w), bool)
    col, m2, n = C.copy(), C * C, np.ones((h, w), T)
    motion = np.zeros((h, w, 4), T)
    motion[..., 2] = -1
    if info is not None:
        info.update({name: np.zeros((h, w), bool) for name in INFO_MASKS})
        info.update({name: np.zeros((h, w), np.int64) for name in INFO_COUNTS})
        info["id"] = np.full((h, w), -1, np.int64)
    if prev is not None:
        cam, pcm = R._cam(camera, T), R._cam(prev_camera, T)
        O, pO, pa = cam["O"], pcm["O"], pcm["a"]
        pLO = pcm["L"] - pO
        nn = (N * N).sum(-1)
        hit = nn >= T(0.25)
        fragile |= R._near(nn, T(0.25))
        ys, xs = np.mgrid[0:h, 0:w]
        u = ((xs.astype(T) + T(0.5)) / T(w))[..., None]
        v = ((ys.astype(T) + T(0.5)) / T(h))[..., None]
        D = cam["L"] + u * cam["H"] + v * cam["V"] - O
        # 2a. the match
        sc_, sr_ = s32[:, :3].astype(T), s32[:, 3].astype(T)
        pc_, pr_ = p32[:, :3].astype(T), p32[:, 3].astype(T)
        cand = (s32[:, 3] > 0) & (p32[:, 3] > 0)
        differs = (s32.view(np.uint32) != p32.view(np.uint32)).any(-1)
        best, second = np.full((h, w), np.inf, T), np.full((h, w), np.inf, T)
        bid = np.full((h, w), -1, np.int64)
        near_surfaces = np.zeros((h, w), np.int64)
        XO0 = X - O
        thr = T(p["pos_tol"]) * T(p["pos_tol"]) * (XO0 * XO0).sum(-1)
        with np.errstate(all="ignore"):
            nhat = N / np.sqrt(nn)[..., None]
            for i0 in range(0, len(s32), CHUNK):
                sl = slice(i0, i0 + CHUNK)
                P = sc_[sl] + sr_[sl, None] * nhat[..., None, :]              # [h, w, chunk, 3]
                S = ((X[..., None, :] - P) ** 2).sum(-1)
                S = np.where(cand[sl], S, np.inf).astype(T)
                surf = (np.sqrt(((X[..., None, :] - sc_[sl]) ** 2).sum(-1)) - sr_[sl]) ** 2
                near_surfaces += (cand[sl] & (surf <= thr[..., None])).sum(-1)
                j = S.argmin(-1)                                              # the first of equal scores
                s1 = np.take_along_axis(S, j[..., None], -1)[..., 0]
                S2 = S.copy()
                np.put_along_axis(S2, j[..., None], np.inf, -1)
                s2 = S2.min(-1)
                upd = s1 < best                                               # an earlier chunk wins a tie
                second = np.where(upd, np.minimum(best, s2), np.minimum(second, s1))
                bid = np.where(upd, j + i0, bid)
                best = np.where(upd, s1, best)
        has = hit & (bid >= 0) & np.isfinite(best)
        matched = has & (best <= thr)
        fragile |= has & R._near(best, thr)
        fragile |= matched & np.isfinite(second) & R._near(second, best)
        ids = np.where(matched, bid, -1)
        moved = matched & differs[np.maximum(ids, 0)]
        with np.errstate(all="ignore"):
            dn = (D * N).sum(-1)
            dlen = T(1e-3) * np.sqrt((D * D).sum(-1))
            lam = ((X - O) * N).sum(-1) / dn
            centred = hit & (np.abs(dn) > dlen) & (lam > 0)
            fragile |= hit & R._near(np.abs(dn), dlen)
            Xc = np.where(centred[..., None], O + lam[..., None] * D, X)
            # 3a. carried back with its sphere
            im = np.maximum(ids, 0)
            ratio = (pr_[im] / sr_[im])[..., None]
            Xp_ = np.where(moved[..., None], pc_[im] + ratio * (Xc - sc_[im]), Xc)
            d = np.where(hit[..., None], Xp_ - pO, D)
            da = (d * pa).sum(-1)
            fd = -(pLO * pa).sum()
            q = (-fd / da)[..., None] * d - pLO
            fx = (q * pcm["H"]).sum(-1) / (pcm["H"] * pcm["H"]).sum() * T(w) - T(0.5)
            fy = (q * pcm["V"]).sum(-1) / (pcm["V"] * pcm["V"]).sum() * T(h) - T(0.5)
            ok = (da < 0) & np.isfinite(fx) & np.isfinite(fy) & (np.abs(fx) < 1e6) & (np.abs(fy) < 1e6)
        fx, fy = np.where(ok, fx, 0), np.where(ok, fy, 0)
        motion[..., 0] = np.where(ok, fx - xs.astype(T), 0)
        motion[..., 1] = np.where(ok, fy - ys.astype(T), 0)
        motion[..., 2] = ids
        motion[..., 3] = ok
        flx, fly = np.floor(fx), np.floor(fy)
        tx, ty = (fx - flx).astype(T), (fy - fly).astype(T)
        x0, y0 = flx.astype(np.int64), fly.astype(np.int64)
        pc = np.asarray(prev["color"])[..., :3].astype(T)
        pm = np.asarray(prev["moment2"]).astype(T)
        pn = np.asarray(prev["normal"])[..., :3].astype(T)
        px = np.asarray(prev["world_pos"])[..., :3].astype(T)
        XO = Xc - O
        lim = T(p["pos_tol"]) * T(p["pos_tol"]) * (XO * XO).sum(-1)
        sw, sn = np.zeros((h, w), T), np.zeros((h, w), T)
        sc, sm = np.zeros((h, w, 3), T), np.zeros((h, w, 3), T)
        for j in (0, 1):
            for i in (0, 1):
                gx, gy = x0 + i, y0 + j
                inside = ok & (gx >= 0) & (gx < w) & (gy >= 0) & (gy < h)
                cx, cy = np.clip(gx, 0, w - 1), np.clip(gy, 0, h - 1)
                b = (tx if i else T(1) - tx) * (ty if j else T(1) - ty)
                Np, Xp = pn[cy, cx], px[cy, cx]
                npn = (Np * Np).sum(-1)
                hitp = npn >= T(0.25)
                ndot = (Np * N).sum(-1)
                dist = ((Xp - Xp_) ** 2).sum(-1)                 # 5a
                same = np.where(hit, hitp & (ndot >= T(p["normal_min"])) & (dist <= lim), ~hitp)
                fragile |= inside & (R._near(npn, T(0.25)) |
                                     (hit & hitp & (R._near(ndot, T(p["normal_min"])) | R._near(dist, lim))))
                bw = np.where(inside & same, b, T(0))
                if info is not None:
                    nok, xok = ndot >= T(p["normal_min"]), dist <= lim
                    info["taps_inside"] += inside
                    info["rej_normal"] += inside & hit & hitp & ~nok & xok
                    info["rej_pos"] += inside & hit & hitp & nok & ~xok
                    info["rej_hitmiss"] += inside & (hit != hitp)
                sw += bw
                sn += bw * pm[cy, cx, 3]
                sc += bw[..., None] * pc[cy, cx]
                sm += bw[..., None] * pm[cy, cx, :3]
        fragile |= R._near(sw, T(1e-3))
        keep = sw > T(1e-3)
        with np.errstate(all="ignore"):
            nh = sn / sw + T(1)
            al = np.maximum(T(1) / nh, T(p["alpha_min"]))[..., None]
            swc = sw[..., None]
            col = np.where(keep[..., None], (T(1) - al) * (sc / swc) + al * C, C)
            m2 = np.where(keep[..., None], (T(1) - al) * (sm / swc) + al * (C * C), C * C)
            n = np.where(keep, nh, T(1))
        if info is not None:
            grazing = hit & ~(np.abs(dn) > dlen)
            info.update(hit=hit, centred=centred, grazing=grazing, lam_le0=hit & ~grazing & ~(lam > 0), ok=ok,
                        keep=keep, alpha_clamped=keep & (T(p["alpha_min"]) > T(1) / nh), matched=matched,
                        moved=moved, touching=hit & (near_surfaces >= 2), id=ids, best=best, second=second,
                        thr=thr)
    fragile |= R._near(n, T(p["min_history"]))
    std = np.sqrt(np.maximum(m2 - col * col, T(0)))
    std = np.where((n < T(p["min_history"]))[..., None], T(p["short_std"]), std)
    if info is not None:
        info.update(short_history=n < T(p["min_history"]), var_clamped=(m2 - col * col < 0).any(-1))
    out.update(color=col, moment2=m2, n=n, color_std=std, motion=motion)
    return out, fragile


def accumulate(frames, moving=True, dtype=np.float64, **params):
    """The restatement chained over [(color, features, camera, cur_scale, spheres)] in `dtype`: the
    moving form, or with moving=False the static one (temporal_ref.step). Returns the last outputs
    and the share of the last frame's pixels whose history was reset at every step after the first."""
    state, prev_cam, prev_sph, out = None, None, None, None
    for color, feats, cam, k, sph in frames:
        pcam = prev_cam if prev_cam is not None else cam
        if moving:
            out, _ = step(color, feats, state, cam, pcam, sph, prev_sph if prev_sph is not None else sph, dtype,
                          cur_scale=k, **params)
        else:
            out, _ = R.step(color, feats, state, cam, pcam, dtype, cur_scale=k, **params)
        state, prev_cam, prev_sph = R.as_state(out, dtype), cam, sph
    return out


# ---- rendered pairs of the default scene: tests/test_gpu_temporal_motion.py::test_step_vs_restatement
SHAPES = ((1, 1), (5, 3), (19, 13), (67, 45))
DTHETAS = R.DTHETAS
FRAME0, CUR_SCALE = R.FRAME0, R.CUR_SCALE
# the default scene's spheres (oracle.default_scene_arrays): 0 ground, 1-2 Lambert, 3-6 metal,
# 7 dielectric, 8 the light
LAMBERT_ID, METAL_ID, RESIZED_ID = 2, 4, 6
LAMBERT_STEP, METAL_STEP, RESIZED_FROM = (0.12, 0.04, -0.08), (-0.1, 0.06, 0.05), 0.42


def scene_pair(spheres):
    """(prev, cur) [count, 4] arrays of the default scene: `cur` is the scene itself, `prev` has one
    Lambert and one metal sphere elsewhere and a third with another radius."""
    cur = sphere_array(spheres)
    prev = cur.copy()
    prev[LAMBERT_ID, :3] -= np.float32(LAMBERT_STEP)
    prev[METAL_ID, :3] -= np.float32(METAL_STEP)
    prev[RESIZED_ID, 3] = RESIZED_FROM
    return prev, cur


def rendered_case(render, make_camera, spheres, w, h, dt):
    """The inputs of one rendered case: (color, cur, prev, cam1, cam0, cur spheres, prev spheres).
    render(w, h, camera, frame0, spheres) returns (color, features) of one 1 spp frame of that scene."""
    sp0, sp1 = scene_pair(spheres)
    cam0, cam1 = (make_camera(*R.orbit_args(t, w, h)) for t in (-dt, 0.0))
    _, g0 = render(w, h, cam0, FRAME0, sp0)
    color, cur = render(w, h, cam1, FRAME0, sp1)
    prev = R.random_prev({k: g0[k] * np.float32(CUR_SCALE) for k in ("normal", "world_pos")}, 1000 * w + h)
    return color, cur, prev, cam1, cam0, sp1, sp0


def _gaps(a, fa, b, fb, worst):
    ok = ~(fa | fb)
    for name in MOTION_OUTPUTS:
        if name not in b:
            continue
        g = R.rel_gap(a[name], b[name], ok)
        key = "std" if name == "color_std" else "all"
        worst[key] = max(worst[key], g)
    assert np.array_equal(a["motion"][..., 2][ok], b["motion"][..., 2][ok])


def f32_f64_gap(render, make_camera, spheres):
    """The largest f32 - f64 gap of the restatement over the rendered cases, on non-fragile pixels:
    (all outputs but color_std, color_std, {case: fragile share})."""
    worst, shares = {"all": 0.0, "std": 0.0}, {}
    for w, h in SHAPES:
        for dt in DTHETAS:
            args = rendered_case(render, make_camera, spheres, w, h, dt)
            a, fa = step(*args, np.float32, cur_scale=CUR_SCALE)
            b, fb = step(*args, np.float64, cur_scale=CUR_SCALE)
            shares[(w, h, dt)] = float(fb.mean())
            _gaps(a, fa, b, fb, worst)
    return worst["all"], worst["std"], shares


# ---- the designed sphere scenes of test_step_designed_cases: frames built analytically (one jittered
# pinhole ray per pixel against the frame's spheres), cameras and scene pairs placed so that each
# branch of the moving step holds pixels; tests/test_temporal_motion_cpu.py counts them.
DESIGNED_SIZE = R.DESIGNED_SIZE
DESIGNED_POS_TOL = R.DESIGNED_POS_TOL
DESIGNED_CASES = ("translate", "contact", "radius", "carried_out", "carried_behind", "same_camera", "unmatched",
                  "analytic")


def sphere_frame(w, h, camera, spheres, seed, jitter=R.JITTER):
    """(color, features, id) of spheres ([count, 4]; radius <= 0: not there) seen from a 22-float
    camera through its origin: one ray per pixel through (x + 1/2 + jx, y + 1/2 + jy), jx, jy uniform
    in +-jitter px, the nearest hit wins. X = c + r n^ with the unit normal n^ (float32 buffers
    [h, w, 4], 0 on a miss); color random in [0.05, 2]; id [h, w], -1 on a miss."""
    rng = np.random.default_rng(seed)
    c = R.cam22(camera).astype(np.float64)
    O, L, H, V = c[0:3], c[12:15], c[15:18], c[18:21]
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float64)
    u = (xs + 0.5 + rng.uniform(-jitter, jitter, (h, w))) / w
    v = (ys + 0.5 + rng.uniform(-jitter, jitter, (h, w))) / h
    D = L + u[..., None] * H + v[..., None] * V - O
    D /= np.linalg.norm(D, axis=-1, keepdims=True)
    best = np.full((h, w), np.inf)
    ids = np.full((h, w), -1, np.int64)
    X, N = np.zeros((h, w, 3)), np.zeros((h, w, 3))
    for i, s in enumerate(np.float64(sphere_array(spheres))):
        cc, r = s[:3], s[3]
        if not r > 0:
            continue
        oc = O - cc
        bq = D @ oc
        disc = bq * bq - (oc @ oc - r * r)
        with np.errstate(invalid="ignore"):
            t = -bq - np.sqrt(disc)
        good = (disc > 0) & (t > 1e-3) & (t < best)
        nh = (O + t[..., None] * D - cc) / r
        nh /= np.linalg.norm(nh, axis=-1, keepdims=True)
        best = np.where(good, t, best)
        ids[good] = i
        N[good] = nh[good]
        X[good] = (cc + r * nh)[good]
    color = np.zeros((h, w, 4), np.float32)
    color[..., :3] = rng.uniform(0.05, 2.0, (h, w, 3))
    feats = {}
    for name, a in (("normal", N), ("world_pos", X), ("albedo", np.where(ids[..., None] >= 0, 0.5, 0.0) * np.ones(3))):
        feats[name] = np.zeros((h, w, 4), np.float32)
        feats[name][..., :3] = a
    return color, feats, ids


def designed_runs(case):
    """The runs of one designed case: dicts of label, w, h, spheres / prev_spheres (what the call is
    given), frame_spheres / prev_frame_spheres (what the frames show; None: the same), cam / prev_cam
    (look_from, look_at; prev_cam None: the same camera, passed as the same bits), jitter, params."""
    def run(label, spheres, prev_spheres, cam, prev_cam, frame_spheres=None, prev_frame_spheres=None,
            jitter=R.JITTER, w=DESIGNED_SIZE[0], h=DESIGNED_SIZE[1], **params):
        return dict(label=f"{case} {label}".strip(), w=w, h=h, spheres=np.float32(spheres),
                    prev_spheres=np.float32(prev_spheres), cam=cam, prev_cam=prev_cam,
                    frame_spheres=np.float32(spheres if frame_spheres is None else frame_spheres),
                    prev_frame_spheres=np.float32(prev_spheres if prev_frame_spheres is None else prev_frame_spheres),
                    jitter=jitter, params=dict(dict(pos_tol=DESIGNED_POS_TOL), **params))
    eye, origin = (0.0, 0.0, 3.0), (0.0, 0.0, 0.0)
    shifted = ((0.1, 0.05, 3.0), origin)
    A, B = [-0.9, 0.0, 0.0, 0.7], [0.9, 0.0, 0.0, 0.7]
    if case == "translate":     # A stands, B moved; sky around them; 33 x 9: larger pixels, a 32-wide block and one column
        Bp = [0.6, -0.25, 0.2, 0.7]
        return [run("37x21", [A, B], [A, Bp], (eye, origin), shifted),
                run("33x9", [A, B], [A, Bp], (eye, origin), shifted, w=33, h=9, pos_tol=0.4)]
    if case == "contact":       # two spheres that touch at the origin, seen from above the contact; one moved
        A1, B1 = [-0.7, 0.0, 0.0, 0.7], [0.7, 0.0, 0.0, 0.7]
        return [run("", [A1, B1], [A1, [0.7, 0.3, 0.0, 0.7]], ((0.0, 0.6, 1.2), origin), ((0.02, 0.6, 1.2), origin),
                    pos_tol=0.3)]
    if case == "radius":        # B grew about its centre, A grew and moved
        return [run("", [A, B], [[-0.8, 0.1, 0.0, 0.55], [0.9, 0.0, 0.0, 0.5]], (eye, origin), shifted)]
    if case == "carried_out":   # B came from far outside the previous image
        return [run("", [A, B], [A, [40.0, 0.0, 0.0, 0.7]], (eye, origin), shifted)]
    if case == "carried_behind":   # B came from behind the previous camera
        return [run("", [A, B], [A, [0.9, 0.0, 6.0, 0.7]], (eye, origin), shifted)]
    if case == "same_camera":   # identical cameras: A's pixels take their own centre, B's go through the projection
        return [run("", [A, B], [A, [0.6, -0.25, 0.2, 0.7]], (eye, origin), None)]
    if case == "unmatched":
        # the frames show a third sphere that the arrays lack (guides not of this scene), A has no
        # radius in the previous array and B none in the current one: no pixel may be matched to
        # either; the zero-radius twin at index 0 of the sphere the frames show at index 3 neither
        Z = [0.0, 0.9, 0.5, 0.0]
        Cs = [0.0, 0.9, 0.5, 0.45]
        E = [0.0, -0.9, 0.5, 0.45]
        shown = [Z, A, B, Cs, E]
        return [run("", [Z, A, [0.9, 0.0, 0.0, -0.7], Cs, [5.0, 5.0, -9.0, 0.1]],
                    [Z, [-0.9, 0.0, 0.0, 0.0], B, [0.1, 0.8, 0.5, 0.45], [5.0, 5.0, -9.0, 0.1]],
                    (eye, origin), shifted, frame_spheres=shown,
                    prev_frame_spheres=[Z, A, B, [0.1, 0.8, 0.5, 0.45], E])]
    if case == "analytic":      # no jitter, identical pinhole cameras, B translated along x: the displacement is known
        return [run("", [A, B], [A, [0.9 - ANALYTIC_DX, 0.0, 0.0, 0.7]], (eye, origin), None, jitter=0.0)]
    raise ValueError(f"unknown designed case {case!r}")


ANALYTIC_DX = 0.3


def analytic_displacement(h, depth):
    """The pixel displacement (previous minus current, along x) of a point `depth` in front of the
    pinhole camera of the `analytic` case when its sphere came from ANALYTIC_DX to the left."""
    return -ANALYTIC_DX * h / (2.0 * np.tan(np.radians(R.VFOV / 2)) * depth)


def designed_inputs(run, make_camera, seed=0):
    """(color, cur, prev, camera, prev_camera, spheres, prev_spheres) of one designed run; the feature
    buffers hold their values / cur_scale."""
    w, h = run["w"], run["h"]
    cam = make_camera(*R._cam_args(*run["cam"], w, h))
    pcam = cam if run["prev_cam"] is None else make_camera(*R._cam_args(*run["prev_cam"], w, h))
    color, cur, _ = sphere_frame(w, h, cam, run["frame_spheres"], [seed, w, h, 0], run["jitter"])
    _, g0, _ = sphere_frame(w, h, pcam, run["prev_frame_spheres"], [seed, w, h, 1], run["jitter"])
    prev = R.make_prev({k: g0[k] for k in ("normal", "world_pos")}, 1000 * w + h + seed)
    k = np.float32(run["params"].get("cur_scale", 1.0))
    return color / k, {n: v / k for n, v in cur.items()}, prev, cam, pcam, run["spheres"], run["prev_spheres"]


def designed_gap(make_camera):
    """f32_f64_gap over the designed sphere cases."""
    worst, shares = {"all": 0.0, "std": 0.0}, {}
    for case in DESIGNED_CASES:
        for run in designed_runs(case):
            args = designed_inputs(run, make_camera)
            a, fa = step(*args, np.float32, **run["params"])
            b, fb = step(*args, np.float64, **run["params"])
            shares[run["label"]] = float(fb.mean())
            _gaps(a, fa, b, fb, worst)
    return worst["all"], worst["std"], shares


# ---- sphere counts (test_sphere_counts): 19 x 13 synthetic frames, every pixel a random sphere of `count`
COUNT_SIZE = (19, 13)
# the kernel stages nothing in LDS; its loop takes four spheres per trip (3, 4, 5), and up to
# INLINE_SPHERES travel in the kernel's arguments, more through an upload (63, 64, 65)
INLINE_SPHERES = 64
COUNTS = (1, 3, 4, 5, 9, 63, 64, 65, 257, 4096)


def count_inputs(count, make_camera, seed=0):
    """(color, cur, prev, camera, prev_camera, spheres, prev_spheres): `count` small spheres on a
    jittered lattice in front of the camera, three in four moved; each pixel shows a random sphere at
    a random normal that faces the camera (no visibility: X = c + r n^), the previous state the same
    sphere where it was, so that history is kept."""
    w, h = COUNT_SIZE
    rng = np.random.default_rng([seed, count])
    side = int(np.ceil(count ** (1 / 3)))
    g = np.stack(np.meshgrid(*[np.arange(side)] * 3, indexing="ij"), -1).reshape(-1, 3)[:count]
    cur = np.zeros((count, 4), np.float32)
    cur[:, :3] = (g - (side - 1) / 2) * (2.0 / side) + rng.uniform(-0.1, 0.1, (count, 3)) / side
    cur[:, 3] = rng.uniform(0.2, 0.3, count) / side
    prv = cur.copy()
    mv = rng.uniform(size=count) < 0.75
    prv[mv, :3] += np.float32(rng.uniform(-0.3, 0.3, (int(mv.sum()), 3)) / side)
    prv[mv, 3] *= np.float32(rng.uniform(0.8, 1.25, int(mv.sum())))
    cam = make_camera(*R._cam_args((0.0, 0.0, 4.0), (0.0, 0.0, 0.0), w, h))
    pcam = make_camera(*R._cam_args((0.05, 0.02, 4.0), (0.0, 0.0, 0.0), w, h))
    pick = rng.integers(0, count, (h, w))
    nh = rng.normal(size=(h, w, 3))
    nh[..., 2] = np.abs(nh[..., 2]) + 0.5
    nh /= np.linalg.norm(nh, axis=-1, keepdims=True)
    color = np.zeros((h, w, 4), np.float32)
    color[..., :3] = rng.uniform(0.05, 2.0, (h, w, 3))
    feats, g0 = {}, {}
    for name, a, b in (("normal", nh, nh), ("world_pos", cur[pick, :3] + cur[pick, 3:] * nh,
                                            prv[pick, :3] + prv[pick, 3:] * nh)):
        feats[name], g0[name] = np.zeros((h, w, 4), np.float32), np.zeros((h, w, 4), np.float32)
        feats[name][..., :3], g0[name][..., :3] = a, b
    prev = R.make_prev(g0, 77 + count)
    return color, feats, prev, cam, pcam, cur, prv, pick


def count_gap(make_camera):
    worst, shares = {"all": 0.0, "std": 0.0}, {}
    for count in COUNTS:
        *args, _ = count_inputs(count, make_camera)
        a, fa = step(*args, np.float32, pos_tol=COUNT_POS_TOL)
        b, fb = step(*args, np.float64, pos_tol=COUNT_POS_TOL)
        shares[count] = float(fb.mean())
        _gaps(a, fa, b, fb, worst)
    return worst["all"], worst["std"], shares


COUNT_POS_TOL = 0.004   # 0.016 at distance 4: a fifth of the smallest radius (0.2 / 16), so the match is the pixel's own sphere


# ---- what it is for: a Lambert sphere of the default scene translated at every step
QUALITY = R.QUALITY
MOVING_ID = 2                       # (0, 0, -1), r 0.5, Lambert
MOVING_STEP = (0.0, -0.3, 0.0)      # per step: it comes down onto the ground, clear of the other spheres;
#                                     its centre ends 4.47 from the camera: pos_tol x that = 0.22


def moving_scenes(spheres, steps):
    """`steps` scenes in which sphere MOVING_ID comes along MOVING_STEP and ends at its default place."""
    out = []
    for t in range(steps):
        s = sphere_array(spheres)
        s[MOVING_ID, :3] -= np.float32(MOVING_STEP) * np.float32(steps - 1 - t)
        out.append(s)
    return out


def moving_frames(render, make_camera, spheres):
    """[(color, features, camera, cur_scale, spheres)] of the quality run: a static camera (the
    orbit's angle 0), step t one fresh sample per pixel of scene t."""
    q = QUALITY
    cam = make_camera(*R.orbit_args(0.0, q["w"], q["h"]))
    return [(*render(q["w"], q["h"], cam, t, s), cam, float(t + 1), s)
            for t, s in enumerate(moving_scenes(spheres, q["steps"]))]


def rel_mse(img, ref, mask=None):
    """denoise_ref.rel_mse's quantity over the pixels of mask."""
    a, b = np.float64(np.asarray(img)[..., :3]), np.float64(np.asarray(ref)[..., :3])
    e = (a - b) ** 2 / (b * b + 1e-2)
    return float((e if mask is None else e[mask]).mean())


# measured in f64 on the oracle's frames (tests/test_temporal_motion_cpu.py::test_quality_moving_sphere
# prints it): relMSE over the moved sphere's pixels, moving accumulation / single 1 spp frame
QUALITY_RATIO = 0.14   # measured: 0.1394 (relMSE 3.758 -> 0.524 over the sphere's 160 pixels; static rule: 3.758)
QUALITY_BAR = 1.25 * QUALITY_RATIO   # the margin covers the f32 kernel and flipped fragile decisions


if __name__ == "__main__":
    import os
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [root, os.path.join(root, "oracle")]
    import oracle
    from learnraytracing_amd import make_camera

    S0, M0 = oracle.default_scene_arrays()

    def _render(w, h, camera, frame0, spheres):
        feats = {n: np.zeros((h, w, 4), np.float32) for n in ("normal", "world_pos", "albedo")}
        buf, _ = oracle.orc_render_ex(w, h, frames=1, depth=8, frame0=frame0, cam22=R.cam22(camera), features=feats,
                                      max_frame=-1, spheres=np.float32(spheres).ravel(), mats=M0)
        return buf, feats

    for title, (gap, gap_std, shares) in (("rendered", f32_f64_gap(_render, make_camera, S0)),
                                          ("designed", designed_gap(make_camera)),
                                          ("count", count_gap(make_camera))):
        print(f"largest f32 - f64 gap over the {title} cases: {gap:.3g} (color_std: {gap_std:.3g})")
        for label, s in shares.items():
            print(f"  {label}: fragile {100 * s:.2f} %")
