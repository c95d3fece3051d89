"""NumPy restatement of the chain motion pass (include/lrt.h, lrt_gbuffer_chain_motion_*) in the
kernel's own order of operations, the cases its tests share, and the designed scene. A helper module,
not a conftest: imported by tests/test_gbuffer_chain_motion_cpu.py and
tests/test_gpu_gbuffer_chain_motion.py. Built on gbuffer_chain_ref (the walk, the key) and gbuffer_ref
(the closest hit, the first-hit motion).

chain_at(C, S, fx, fy) is gbuffer_chain_ref.chain's walk from a continuous pixel position:
s = (fx + 1/2) (1 / w), t = (fy + 1/2) (1 / h), D = ((L + s H) + t V) - O. It yields the key, the
terminal id, the bounces and the terminal vector F (the terminal point on a hit, the last ray's unit
direction on the sky).

Per pixel (x, y), in `dtype` (np.float32: the kernel's arithmetic operation for operation;
np.float64: the reference):
  1. (K, j, b, Y) = chain_at(camera, spheres, x, y); nothing followed: NOT_FOLLOWED; unresolved:
     UNRESOLVED
  2. Y' = c' + (r' / r) (Y - c) if j >= 0, a previous scene is given and sphere j's eight floats
     differ, else Y; r <= 0 or r' <= 0: NO_SEED
  3. q = (x + mx, y + my) of first_motion; its w == 0, or not |q.x|, |q.y| < 1e6: NO_SEED
  4. `iterations` times: F0, Fx, Fy = chain_at(prev camera, prev spheres, q [+ (probe, 0), + (0, probe)]);
     a key other than K: KEY_LOST; Jx = (Fx - F0) (1 / probe), Jy likewise, r = Y' - F0;
     a = Jx.Jx, bb = Jx.Jy, c = Jy.Jy, e = Jx.r, f = Jy.r, det = a c - bb bb,
     dx = (c e - bb f) / det, dy = (a f - bb e) / det; not finite: NOT_CONVERGED;
     len = sqrt(dx dx + dy dy) > step_max: both times step_max / len; q += (dx, dy); not
     |q.x|, |q.y| < 1e6: NOT_CONVERGED
  5. F0 = chain_at(..., q), key other than K: KEY_LOST; (dx, dy) with the last Jx, Jy and the new r;
     rem = sqrt(dx dx + dy dy); CONVERGED iff rem <= converged and |q.x|, |q.y| < 1e6
  6. motion = (q.x - x, q.y - y, first_motion.z, 1) where CONVERGED, else first_motion's quad.
`fragile` (of one run) marks a pixel if any chain evaluated for it while it was still searching is
fragile in gbuffer_chain_ref's sense, or |rem - converged| <= converged / 4. pair() runs f32 and f64
and adds the pixels one of whose evaluated keys differs between the two.

`python tests/gbuffer_chain_motion_ref.py` prints, per case, the f32 - f64 motion gap in pixels off
the mask, the fragile share of the followed pixels and the status histogram.
"""
import numpy as np

import gbuffer_chain_ref as C
import gbuffer_ref as G
import temporal_gbuffer_ref as TG
import temporal_ref as R

NOT_FOLLOWED, CONVERGED, UNRESOLVED, NO_SEED, KEY_LOST, NOT_CONVERGED = range(6)   # LRT_CM_*
STATUS_NAMES = ("not_followed", "converged", "unresolved", "no_seed", "key_lost", "not_converged")
DEFAULTS = dict(max_bounces=4, roughness_max=0.25, iterations=3, probe_px=0.25, step_max_px=16.0, converged_px=0.0625)
SIZES = ((19, 13), (67, 45), (160, 90))          # the CPU test's; the GPU test takes the first two and 1 x 1
MOTIONS = ("orbit", "moved", "both")
DTHETA = G.DTHETA
COUNTS = C.COUNTS
COUNT_SIZE = C.COUNT_SIZE


def chain_at(w, h, camera, s32, mats, fx, fy, max_bounces, roughness_max, T):
    """gbuffer_chain_ref.chain's walk from the positions (fx, fy) [h, w] of a w x h frame: (key int32,
    id int32, bounces int32 (with C.UNRESOLVED), F [h, w, 3], fragile)."""
    typ, alb32, rough, ri32 = mats
    cs, ri = s32[:, :3].astype(T), ri32.astype(T)
    rmax = np.float32(roughness_max)
    c = R._cam(camera, T)
    s = ((fx + T(0.5)) * (T(1) / T(w)))[..., None]
    t = ((fy + T(0.5)) * (T(1) / T(h)))[..., None]
    with np.errstate(all="ignore"):
        D = ((c["L"] + s * c["H"]) + t * c["V"]) - c["O"]
        d = G._normalize(D, T)
    org = np.broadcast_to(c["O"], d.shape).copy()
    ids, t, fragile = G.closest_hit(org, d, s32, T)
    fragile = fragile | C._near_min_t(org, d, s32, T)
    hit = ids >= 0
    with np.errstate(all="ignore"):
        P = np.where(hit[..., None], org + d * t[..., None], T(0))
        n = np.where(hit[..., None], G._normalize(P - cs[np.maximum(ids, 0)], T), T(0))
    hkey = ids.astype(np.uint32)
    bounces = np.zeros(ids.shape, np.int32)

    def delta_of(ids, hit):
        m = np.maximum(ids, 0)
        return hit & (((typ[m] == C.METAL) & (rough[m] <= rmax)) | (typ[m] == C.DIELECTRIC))

    active = delta_of(ids, hit)
    for _ in range(int(max_bounces)):
        if not active.any():
            break
        im = np.maximum(ids, 0)
        with np.errstate(all="ignore"):
            dn = G._dot(d, n)
            refl = d + T(2) * (-dn[..., None] * n)
            metal = typ[im] == C.METAL
            leaving = dn > 0
            N = np.where(leaving[..., None], -n, n)
            nint = np.where(leaving, ri[im], T(1) / ri[im])
            dt = G._dot(d, N)
            discr = T(1) - nint * nint * (T(1) - dt * dt)
            refr = nint[..., None] * (d - N * dt[..., None]) - N * np.sqrt(discr)[..., None]
            nd = np.where((metal | ~(discr > 0))[..., None], refl, refr)
            fragile |= active & ~metal & ((np.abs(discr) <= C.FRAGILE_REL) | (np.abs(dn) <= C.FRAGILE_REL))
            org = np.where(active[..., None], P, org)
            d = np.where(active[..., None], G._normalize(nd, T), d)
        nid, t, grazing = G.closest_hit(org, d, s32, T)
        fragile |= active & (grazing | C._near_min_t(org, d, s32, T))
        with np.errstate(all="ignore"):
            step = hkey * np.uint32(0x9E3779B1) + (nid + 1).astype(np.uint32)
            step ^= step >> np.uint32(15)
            hkey = np.where(active, step, hkey)
            bounces = bounces + active
            ids = np.where(active, nid, ids)
            nhit = nid >= 0
            Pn = org + d * t[..., None]
            nn = G._normalize(Pn - cs[np.maximum(nid, 0)], T)
            P = np.where(active[..., None], np.where(nhit[..., None], Pn, T(0)), P)
            n = np.where(active[..., None], np.where(nhit[..., None], nn, T(0)), n)
        active = active & delta_of(nid, nhit)
    key = np.where(bounces > 0, np.uint32(0x40000000) | (hkey & np.uint32(0x3FFFFFFF)), hkey).astype(np.uint32)
    F = np.where((ids >= 0)[..., None], P, d)
    return (key.view(np.int32), ids.astype(np.int32), (bounces + np.where(active, C.UNRESOLVED, 0)).astype(np.int32), F,
            fragile)


def _gn(Jx, Jy, r, T):
    """The Gauss-Newton step of the 3 x 2 system (Jx, Jy) (dx, dy) = r, by its normal equations."""
    a, bb, c = G._dot(Jx, Jx), G._dot(Jx, Jy), G._dot(Jy, Jy)
    e, f = G._dot(Jx, r), G._dot(Jy, r)
    det = a * c - bb * bb
    return (c * e - bb * f) / det, (a * f - bb * e) / det


def chain_motion(w, h, camera, prev_camera, spheres, materials, first_motion, prev_spheres=None, dtype=np.float64,
                 **params):
    """{"motion" [h, w, 4] in `dtype`, "status" [h, w] int32, "rem" [h, w], "keys" [1 + 3 iterations + 1, h, w]
    int32, "searched" likewise bool} and the run's fragile mask. first_motion: lrt_gbuffer's plane
    (float32; an input, the same in both dtypes). prev_spheres None: no scene is given."""
    p = dict(DEFAULTS, **params)
    T = dtype
    s32 = G.sphere_array(spheres)
    p32 = s32 if prev_spheres is None else G.sphere_array(prev_spheres)
    mats = C.material_arrays(materials)
    fm = np.asarray(first_motion, np.float32)[..., :4]
    ys, xs = np.mgrid[0:h, 0:w]
    xs, ys = xs.astype(T), ys.astype(T)
    walk = (int(p["max_bounces"]), p["roughness_max"], T)
    probe = T(np.float32(p["probe_px"]))
    inv_probe = T(1) / probe
    step_max, conv = T(np.float32(p["step_max_px"])), T(np.float32(p["converged_px"]))

    K, j, b, Y, fragile = chain_at(w, h, camera, s32, mats, xs, ys, *walk)
    status = np.full((h, w), -1, np.int32)
    status[(b & 0xFF) == 0] = NOT_FOLLOWED
    status[(status < 0) & (b >= C.UNRESOLVED)] = UNRESOLVED
    keys, searched = [K], [np.ones((h, w), bool)]
    jm = np.maximum(j, 0)
    Yp = Y
    if prev_spheres is not None:
        cand = (s32[:, 3] > 0) & (p32[:, 3] > 0)
        differs = (s32.view(np.uint32) != p32.view(np.uint32)).any(-1)
        moved = (j >= 0) & (cand & differs)[jm]
        with np.errstate(all="ignore"):
            ratio = (p32[:, 3].astype(T) / s32[:, 3].astype(T))[jm][..., None]
            Yp = np.where(moved[..., None], p32[:, :3].astype(T)[jm] + ratio * (Y - s32[:, :3].astype(T)[jm]), Y)
        status[(status < 0) & (j >= 0) & ~cand[jm]] = NO_SEED
    with np.errstate(all="ignore"):
        sx, sy = xs + fm[..., 0].astype(T), ys + fm[..., 1].astype(T)
        seed = (fm[..., 3] != 0) & (np.abs(sx) < T(1e6)) & (np.abs(sy) < T(1e6))
    status[(status < 0) & ~seed] = NO_SEED
    search = status < 0
    fragile = fragile & search
    qx, qy = np.where(search, sx, xs), np.where(search, sy, ys)
    Jx = Jy = np.zeros((h, w, 3), T)

    def evaluate(fx, fy):
        nonlocal fragile
        k, _, _, F, fr = chain_at(w, h, prev_camera, p32, mats, fx, fy, *walk)
        fragile |= search & fr
        keys.append(k)
        searched.append(search.copy())
        return k, F

    for _ in range(int(p["iterations"])):
        k0, F0 = evaluate(qx, qy)
        k1, F1 = evaluate(qx + probe, qy)
        k2, F2 = evaluate(qx, qy + probe)
        lost = search & ((k0 != K) | (k1 != K) | (k2 != K))
        status[lost] = KEY_LOST
        search = search & ~lost
        with np.errstate(all="ignore"):
            Jx, Jy = (F1 - F0) * inv_probe, (F2 - F0) * inv_probe
            dx, dy = _gn(Jx, Jy, Yp - F0, T)
            bad = search & ~(np.isfinite(dx) & np.isfinite(dy))
            status[bad] = NOT_CONVERGED
            search = search & ~bad
            ln = np.sqrt(dx * dx + dy * dy)
            k = np.where(ln > step_max, step_max / ln, T(1))
            dx, dy = np.where(ln > step_max, dx * k, dx), np.where(ln > step_max, dy * k, dy)
            qx, qy = np.where(search, qx + dx, qx), np.where(search, qy + dy, qy)
            far = search & ~((np.abs(qx) < T(1e6)) & (np.abs(qy) < T(1e6)))
            status[far] = NOT_CONVERGED
            search = search & ~far
            qx, qy = np.where(far, xs, qx), np.where(far, ys, qy)
    k0, F0 = evaluate(qx, qy)
    lost = search & (k0 != K)
    status[lost] = KEY_LOST
    search = search & ~lost
    with np.errstate(all="ignore"):
        dx, dy = _gn(Jx, Jy, Yp - F0, T)
        rem = np.sqrt(dx * dx + dy * dy)
        good = search & (rem <= conv) & (np.abs(qx) < T(1e6)) & (np.abs(qy) < T(1e6))
        fragile |= search & (np.abs(rem - conv) <= conv / T(4))
    status[search] = NOT_CONVERGED
    status[good] = CONVERGED
    mv = fm.astype(T)
    mv[..., 0] = np.where(good, qx - xs, mv[..., 0])
    mv[..., 1] = np.where(good, qy - ys, mv[..., 1])
    mv[..., 3] = np.where(good, T(1), mv[..., 3])
    return dict(motion=mv, status=status, rem=np.where(search, rem, T(0)), keys=np.stack(keys),
                searched=np.stack(searched)), fragile


def pair(kw):
    """The f32 and the f64 run of one case and the `fragile` mask of the two together."""
    a, fa = chain_motion(dtype=np.float32, **kw)
    b, fb = chain_motion(dtype=np.float64, **kw)
    differ = ((a["keys"] != b["keys"]) & a["searched"] & b["searched"]).any(0)
    return a, b, fa | fb | differ


def followed(out):
    return out["status"] != NOT_FOLLOWED


def motion_gap(a, b, ok):
    """The largest |a - b| over motion.xy in pixels on the pixels of ok where both converged."""
    ok = ok & (a["status"] == CONVERGED) & (b["status"] == CONVERGED)
    if not ok.any():
        return 0.0
    return float(np.abs(a["motion"][..., :2].astype(np.float64) - b["motion"][..., :2])[ok].max())


def first_hit_motion(w, h, camera, prev_camera, spheres, materials, prev_spheres=None):
    """lrt_gbuffer's motion plane in its own arithmetic (gbuffer_ref's f32 run), float32 [h, w, 4]."""
    g, _ = G.gbuffer(w, h, camera, spheres, np.zeros((len(G.sphere_array(spheres)), 3), np.float32), prev_camera,
                     prev_spheres, dtype=np.float32)
    return np.ascontiguousarray(g["motion"], np.float32)


def make_case(w, h, camera, prev_camera, spheres, materials, prev_spheres=None, **params):
    """chain_motion's arguments with the first-hit motion worked out."""
    s = G.sphere_array(spheres)
    return dict(w=w, h=h, camera=camera, prev_camera=prev_camera, spheres=s, materials=materials, prev_spheres=prev_spheres,
                first_motion=first_hit_motion(w, h, camera, prev_camera, s, materials, prev_spheres), **params)


# ---- the restatement cases
def motion_case(w, h, how, default_scene, make_camera):
    """The default scene at w x h: "orbit" (one step of DTHETA), "moved" (the same camera,
    gbuffer_ref.moved_scene) or "both"."""
    s, m = default_scene()
    cam, pcam = G.camera_pair(make_camera, w, h, DTHETA)
    return make_case(w, h, cam, cam if how == "moved" else pcam, s, m, None if how == "orbit" else G.moved_scene(s))


def shape_cases(default_scene, make_camera, sizes=SIZES):
    return [(f"{w}x{h} {how}", motion_case(w, h, how, default_scene, make_camera)) for w, h in sizes for how in MOTIONS]


def count_cases(default_scene, random_scene, make_camera):
    """COUNTS at COUNT_SIZE, the orbit alone, no scene given: the grid instance."""
    w, h = COUNT_SIZE
    cases = []
    for count in COUNTS:
        s, m = G.count_scene(count, default_scene, random_scene)
        cam, pcam = G.camera_pair(make_camera, w, h, DTHETA)
        cases.append((f"count {count}", make_case(w, h, cam, pcam, s, m)))
    return cases


# ---- the designed case "flat": a mirror of radius 50 fills the lower part of the frame and shows two
# Lambert spheres that stand behind the camera; the camera steps sideways
FLAT_SPHERES = [[0, 0, -52, 50], [-1.5, 0, 5, 1.5], [1.5, 0, 5, 1.5]]
FLAT_MATERIALS = [(C.METAL, (0.9, 0.8, 0.7), 0.0, 0.0), (C.LAMBERT, (0.8, 0.3, 0.2), 0.0, 0.0),
                  (C.LAMBERT, (0.2, 0.4, 0.9), 0.0, 0.0)]
FLAT_SIZE = (37, 21)
FLAT_VFOV = 40.0
FLAT_DX = 0.3


def flat_cameras(make_camera):
    w, h = FLAT_SIZE
    def at(x):
        return make_camera((x, 0.0, 3.0), (x, 0.0, 0.0), R.VUP, FLAT_VFOV, w / h, 0.0, 3.0)
    return at(0.0), at(-FLAT_DX)


def flat_case(make_camera):
    cam, pcam = flat_cameras(make_camera)
    return make_case(*FLAT_SIZE, cam, pcam, np.float32(FLAT_SPHERES), list(FLAT_MATERIALS))


FLAT_POKED_W0, FLAT_POKED_NAN, FLAT_POKED_FAR = (slice(2, 5), slice(3, 6)), (slice(8, 10), slice(20, 24)), (12, 30)


def flat_moved_case(make_camera):
    """"flat" with a previous scene and a first_motion that was tampered with, for the branches the
    rendered cases do not reach: the left Lambert sphere did not exist in the previous frame (r' = 0:
    NO_SEED wherever the mirror shows it), the right one came from elsewhere with another radius (its
    pixels are searched for the carried-back point), and first_motion has w = 0 in one block, a NaN
    in another and 2e6 px at one pixel (NO_SEED)."""
    cam, pcam = flat_cameras(make_camera)
    prev = np.float32(FLAT_SPHERES)
    prev[1, 3] = 0.0
    prev[2] += np.float32((0.1, 0.05, 0.0, 0.2))
    kw = make_case(*FLAT_SIZE, cam, pcam, np.float32(FLAT_SPHERES), list(FLAT_MATERIALS), prev)
    kw["first_motion"][FLAT_POKED_W0][..., 3] = 0
    kw["first_motion"][FLAT_POKED_NAN][..., 0] = np.nan
    kw["first_motion"][FLAT_POKED_FAR][1] = 2e6
    return kw


def terminal_colour(w, h, camera, spheres, materials, dtype=np.float64, **params):
    """0.5 + 0.25 lx + 0.15 ly + 0.1 lz of the terminal vector at the pixel centres (sphere-local on a
    hit: the point minus its sphere's centre), as an RGBA quad of three equal channels, and the
    chain's key."""
    p = dict(DEFAULTS, **params)
    T = dtype
    s32 = G.sphere_array(spheres)
    ys, xs = np.mgrid[0:h, 0:w]
    key, j, _, F, _ = chain_at(w, h, camera, s32, C.material_arrays(materials), xs.astype(T), ys.astype(T),
                               int(p["max_bounces"]), p["roughness_max"], T)
    local = np.where((j >= 0)[..., None], F - s32[:, :3].astype(T)[np.maximum(j, 0)], F)
    v = T(0.5) + T(0.25) * local[..., 0] + T(0.15) * local[..., 1] + T(0.1) * local[..., 2]
    out = np.zeros((h, w, 4), np.float32)
    out[..., :3] = v[..., None]
    return out, key


def flat_temporal_ratio(make_camera, step, motions):
    """What the plane is for. Colours that are a smooth function of the terminal point, at the pixel
    centres of the previous and of the current frame; two steps of the temporal rule with the chain's
    keys as ids; the mean |out - current colour| over the converged pixels that kept a history in
    both runs, with the new motion over with the first-hit motion. step(color, cur, prev_g, prev) ->
    (color [h, w, >= 3], keep [h, w]); motions = (first-hit, new)."""
    kw = flat_case(make_camera)
    w, h = kw["w"], kw["h"]
    cam, pcam = flat_cameras(make_camera)
    col_prev, key_prev = terminal_colour(w, h, pcam, kw["spheres"], kw["materials"], np.float32)
    col_cur, key_cur = terminal_colour(w, h, cam, kw["spheres"], kw["materials"], np.float32)
    g_prev = TG.ref_planes(w, h, pcam, kw["spheres"], motion=False)
    g_cur = TG.ref_planes(w, h, cam, kw["spheres"], motion=False)
    errs, keeps = [], []
    for mv in motions:
        first = {"normal": g_prev["normal"], "motion": TG.quad(np.zeros((h, w, 4))), "id": key_prev}
        s0, _ = step(col_prev, first, None, None)
        out, keep = step(col_cur, {"normal": g_cur["normal"], "motion": np.ascontiguousarray(mv, np.float32), "id": key_cur},
                         {"normal": g_prev["normal"], "id": key_prev}, s0)
        errs.append(np.abs(np.asarray(out)[..., :3].astype(np.float64) - col_cur[..., :3]).mean(-1))
        keeps.append(keep)
    return errs, keeps


def independent_step(kw, motion, probe=0.125):
    """The f64 check of an answer that shares nothing with the search but chain_at: at (x + mx, y + my)
    under the previous camera and scene, the key, and the length of a fresh Gauss-Newton step with
    differences of `probe` px, solved by least squares. Returns (the key there [h, w], the current
    frame's key [h, w], step length [h, w]; NaN where the probes leave the key on both sides)."""
    T = np.float64
    p = dict(DEFAULTS, **{k: v for k, v in kw.items() if k in DEFAULTS})
    w, h = kw["w"], kw["h"]
    s32 = G.sphere_array(kw["spheres"])
    p32 = s32 if kw.get("prev_spheres") is None else G.sphere_array(kw["prev_spheres"])
    mats = C.material_arrays(kw["materials"])
    walk = (int(p["max_bounces"]), p["roughness_max"], T)
    ys, xs = np.mgrid[0:h, 0:w]
    K, j, _, Y, _ = chain_at(w, h, kw["camera"], s32, mats, xs.astype(T), ys.astype(T), *walk)
    jm = np.maximum(j, 0)
    if kw.get("prev_spheres") is not None:
        differs = (s32.view(np.uint32) != p32.view(np.uint32)).any(-1)
        with np.errstate(all="ignore"):
            back = p32[jm, :3].astype(T) + (p32[jm, 3].astype(T) / s32[jm, 3].astype(T))[..., None] * (Y - s32[jm, :3].astype(T))
        Y = np.where(((j >= 0) & differs[jm])[..., None], back, Y)
    qx, qy = xs + np.asarray(motion)[..., 0].astype(T), ys + np.asarray(motion)[..., 1].astype(T)
    k0, _, _, F0, _ = chain_at(w, h, kw["prev_camera"], p32, mats, qx, qy, *walk)

    def column(ox, oy):
        """dF / d(one axis): the forward difference at `probe`; where that probe leaves the key (a
        silhouette, or a hole in a many-bounce key region) the backward one, then both at half and at
        a quarter of the probe."""
        col, have = np.zeros((h, w, 3), T), np.zeros((h, w), bool)
        for step in (probe, -probe, probe / 2, -probe / 2, probe / 4, -probe / 4):
            k, _, _, F, _ = chain_at(w, h, kw["prev_camera"], p32, mats, qx + ox * step, qy + oy * step, *walk)
            take = ~have & (k == K)
            col = np.where(take[..., None], (F - F0) / step, col)
            have |= take
        return col, have

    (Jx, okx), (Jy, oky) = column(1, 0), column(0, 1)
    length = np.full((h, w), np.nan)
    for y, x in zip(*np.nonzero((k0 == K) & okx & oky)):
        J = np.stack([Jx[y, x], Jy[y, x]], 1)
        length[y, x] = np.linalg.norm(np.linalg.lstsq(J, Y[y, x] - F0[y, x], rcond=None)[0])
    return k0, K, length


def report(cases):
    """Per case: (motion gap in px off the mask, fragile share of the followed pixels, status
    disagreements off the mask, status histogram of the f32 run)."""
    out = {}
    for label, kw in cases:
        a, b, fragile = pair(kw)
        fol = followed(a) | followed(b)
        share = float((fragile & fol).sum() / max(1, fol.sum()))
        out[label] = (motion_gap(a, b, ~fragile), share, int(((a["status"] != b["status"]) & ~fragile).sum()),
                      np.bincount(a["status"].ravel(), minlength=6).tolist())
    return out


if __name__ == "__main__":
    import os
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [root]
    from learnraytracing_amd import default_scene, make_camera, random_scene

    groups = [("the default scene", shape_cases(default_scene, make_camera, SIZES + ((1, 1),))),
              ("the grid counts", count_cases(default_scene, random_scene, make_camera)),
              ("flat", [("flat", flat_case(make_camera))])]
    for title, group in groups:
        print(title)
        for label, (gap, share, differ, hist) in report(group).items():
            print(f"  {label}: f32 - f64 motion gap {gap:.3g} px, fragile {100 * share:.2f} % of the followed, "
                  f"status differs off the mask at {differ} px, {dict(zip(STATUS_NAMES, hist))}")
