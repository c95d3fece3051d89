"""NumPy restatement of temporal reprojection and accumulation (include/lrt.h, lrt_temporal_*), the
cases the temporal tests share, and the orbit they render. A helper module, not a conftest: imported
by tests/test_temporal_cpu.py and tests/test_gpu_temporal.py.

Per pixel p = (x, y), with C, N, X, A = cur_scale x (color, normal, world_pos, albedo).rgb, the
camera O, L, H, V and the previous camera O', a', L', H', V':
  1. hit = |N|^2 >= 0.25
  2. D = L + ((x + 1/2) / w) H + ((y + 1/2) / h) V - O
  3. if hit, |D.N| > 1e-3 |D| and lambda = ((X - O).N) / (D.N) > 0: Xc = O + lambda D, else Xc = X;
     d = Xc - O' for a hit, D for a miss
  4. da = d.a', fd = -(L' - O').a', q = (-fd / da) d - (L' - O'),
     fx = (q.H') / (H'.H') w - 1/2, fy = (q.V') / (V'.V') h - 1/2; no history unless da < 0,
     everything is finite and |fx|, |fy| < 1e6
  5. taps Q = (floor(fx) + i, floor(fy) + j), bilinear weights b_ij; a tap counts iff it is inside
     the image and consistent: hit pixel: hit'(Q), N'(Q).N >= normal_min and
     |X'(Q) - Xc|^2 <= pos_tol^2 |Xc - O|^2; miss pixel: !hit'(Q)
  6. sw = sum b; if sw > 1e-3: n = sum b n' / sw + 1, alpha = max(1 / n, alpha_min),
     color = (1 - alpha) sum b c' / sw + alpha C, moment2 likewise with C^2; else (and without a
     previous state) color = C, moment2 = C^2, n = 1
  7. std = sqrt(max(moment2 - color^2, 0)), or short_std where n < min_history

`python tests/temporal_ref.py` prints the largest gap between the f32 and the f64 run over the GPU
test's cases (the constants F32_F64_GAP and F32_F64_GAP_STD of tests/test_gpu_temporal.py) and the
share of fragile pixels per case.
"""
import numpy as np

DEFAULTS = dict(cur_scale=1.0, alpha_min=0.05, normal_min=0.9, pos_tol=0.05, short_std=1e3, min_history=4)
STATE_NAMES = ("color", "moment2", "normal", "world_pos", "albedo")
OUTPUTS = ("color", "moment2", "n", "normal", "world_pos", "albedo", "color_std")
FRAGILE_REL = 1e-4


def cam22(camera):
    """A camera as its 22 floats (origin, a, u, r, lowerLeftCorner, horizontalVec, verticalVec,
    lensRadius): a ctypes Camera or any sequence of 22."""
    return np.asarray(camera.to22() if hasattr(camera, "to22") else camera, np.float32)


def _cam(camera, T):
    c = cam22(camera).astype(T)
    return dict(O=c[0:3], a=c[3:6], L=c[12:15], H=c[15:18], V=c[18:21])


def _near(v, thr):
    """Is the decision v <> thr within FRAGILE_REL (relative) of its threshold?"""
    return np.abs(v - thr) <= FRAGILE_REL * np.maximum(np.abs(thr), np.abs(v))


def step(color, cur, prev, camera, prev_camera, dtype=np.float64, **params):
    """One step. color [h, w, >= 3]; cur {"normal", "world_pos"[, "albedo"]}; prev: a state
    {"color", "moment2" (n in its alpha), "normal", "world_pos"} of [h, w, 4] buffers, or None.
    Arithmetic in `dtype`. Returns (state, fragile): state maps OUTPUTS to [h, w, 3] arrays ("n":
    [h, w]; "albedo" only if cur has it) in `dtype`; fragile [h, w] marks the pixels one of whose
    decisions lies within FRAGILE_REL of its threshold."""
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
    fragile = np.zeros((h, w), bool)
    col, m2, n = C.copy(), C * C, np.ones((h, w), T)
    if prev is not None:
        cam, pcm = _cam(camera, T), _cam(prev_camera, T)
        O, pO, pa = cam["O"], pcm["O"], pcm["a"]
        pLO = pcm["L"] - pO
        nn = (N * N).sum(-1)
        hit = nn >= T(0.25)
        fragile |= _near(nn, T(0.25))
        ys, xs = np.mgrid[0:h, 0:w]
        u = ((xs.astype(T) + T(0.5)) / T(w))[..., None]
        v = ((ys.astype(T) + T(0.5)) / T(h))[..., None]
        D = cam["L"] + u * cam["H"] + v * cam["V"] - O
        with np.errstate(all="ignore"):
            dn = (D * N).sum(-1)
            dlen = T(1e-3) * np.sqrt((D * D).sum(-1))
            lam = ((X - O) * N).sum(-1) / dn
            centred = hit & (np.abs(dn) > dlen) & (lam > 0)
            fragile |= hit & _near(np.abs(dn), dlen)
            Xc = np.where(centred[..., None], O + lam[..., None] * D, X)
            d = np.where(hit[..., None], Xc - pO, D)
            da = (d * pa).sum(-1)
            fd = -(pLO * pa).sum()
            q = (-fd / da)[..., None] * d - pLO
            fx = (q * pcm["H"]).sum(-1) / (pcm["H"] * pcm["H"]).sum() * T(w) - T(0.5)
            fy = (q * pcm["V"]).sum(-1) / (pcm["V"] * pcm["V"]).sum() * T(h) - T(0.5)
            ok = (da < 0) & np.isfinite(fx) & np.isfinite(fy) & (np.abs(fx) < 1e6) & (np.abs(fy) < 1e6)
        fx, fy = np.where(ok, fx, 0), np.where(ok, fy, 0)
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
                dist = ((Xp - Xc) ** 2).sum(-1)
                same = np.where(hit, hitp & (ndot >= T(p["normal_min"])) & (dist <= lim), ~hitp)
                fragile |= inside & (_near(npn, T(0.25)) |
                                     (hit & hitp & (_near(ndot, T(p["normal_min"])) | _near(dist, lim))))
                bw = np.where(inside & same, b, T(0))
                sw += bw
                sn += bw * pm[cy, cx, 3]
                sc += bw[..., None] * pc[cy, cx]
                sm += bw[..., None] * pm[cy, cx, :3]
        fragile |= _near(sw, T(1e-3))
        keep = sw > T(1e-3)
        with np.errstate(all="ignore"):
            nh = sn / sw + T(1)
            al = np.maximum(T(1) / nh, T(p["alpha_min"]))[..., None]
            swc = sw[..., None]
            col = np.where(keep[..., None], (T(1) - al) * (sc / swc) + al * C, C)
            m2 = np.where(keep[..., None], (T(1) - al) * (sm / swc) + al * (C * C), C * C)
            n = np.where(keep, nh, T(1))
    fragile |= _near(n, T(p["min_history"]))
    std = np.sqrt(np.maximum(m2 - col * col, T(0)))
    std = np.where((n < T(p["min_history"]))[..., None], T(p["short_std"]), std)
    out.update(color=col, moment2=m2, n=n, color_std=std)
    return out, fragile


def as_state(out, dtype=np.float32):
    """A step's outputs as the [h, w, 4] buffers the next step takes (float32: the library's)."""
    h, w = out["n"].shape
    st = {}
    for name in STATE_NAMES:
        if name in out:
            st[name] = np.zeros((h, w, 4), dtype)
            st[name][..., :3] = out[name]
    st["moment2"][..., 3] = out["n"]
    return st


def rel_gap(a, ref, mask=None):
    """max |a - ref| / max(1, |ref|) over the pixels of mask -- the quantity the GPU test bounds."""
    ref = np.asarray(ref, np.float64)
    g = np.abs(np.asarray(a, np.float64) - ref) / np.maximum(1.0, np.abs(ref))
    if mask is not None:
        g = g[mask]
    return float(g.max()) if g.size else 0.0


# ---- the orbit the tests render
LOOK_AT, VUP, VFOV, APERTURE = (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), 60.0, 0.1


def orbit_args(theta, w, h):
    """lrt_camera_make's arguments for the orbit lookFrom = (3 sin t, 2, 3 cos t) around the
    origin: aperture 0.1, focus distance |lookFrom|."""
    look_from = (3.0 * np.sin(theta), 2.0, 3.0 * np.cos(theta))
    return look_from, LOOK_AT, VUP, VFOV, w / h, APERTURE, float(np.linalg.norm(look_from))


def orbit_thetas(steps, dtheta):
    """`steps` angles dtheta apart that end at 0."""
    return [(-(steps - 1) + t) * dtheta for t in range(steps)]


def orbit_frames(render, make_camera, w, h, steps, dtheta):
    """The time steps of an orbit that ends at angle 0: [(color, features, camera, cur_scale)], step t
    one fresh sample per pixel (frame0 = t into zeroed buffers, so cur_scale = t + 1).
    render(w, h, camera, frame0) returns (color, features)."""
    out = []
    for t, theta in enumerate(orbit_thetas(steps, dtheta)):
        cam = make_camera(*orbit_args(theta, w, h))
        color, feats = render(w, h, cam, t)
        out.append((color, feats, cam, float(t + 1)))
    return out


def accumulate(frames, dtype=np.float64, **params):
    """The restatement chained over orbit_frames' steps in `dtype`. Returns the last step's outputs."""
    state, prev_cam, out = None, None, None
    for color, feats, cam, k in frames:
        out, _ = step(color, feats, state, cam, prev_cam if prev_cam is not None else cam, dtype,
                      cur_scale=k, **params)
        state, prev_cam = as_state(out, dtype), cam
    return out


# the quality bars (tests/test_temporal_cpu.py::test_quality_*, tests/test_gpu_temporal.py::test_quality_on_gpu)
QUALITY = dict(w=160, h=90, depth=8, steps=16, gt_spp=1024)
BAR_REL, BAR_MSE, BAR_DENOISED = 0.25, 0.5, 0.6


# ---- the cases of tests/test_gpu_temporal.py::test_step_vs_restatement
SHAPES = ((1, 1), (5, 3), (19, 13), (67, 45), (257, 9), (160, 90))   # w x h
DTHETAS = (0.02, 0.08)
FRAME0, CUR_SCALE = 3, 4.0


def random_prev(guides, seed):
    """A previous state over a frame's guides: seeded random positive colour and second moment, n
    drawn from 1..20 (reals: a whole n' = min_history - 1 under a single counting tap would put n
    exactly on the min_history threshold)."""
    h, w = guides["normal"].shape[:2]
    rng = np.random.default_rng(seed)
    st = {"normal": guides["normal"].copy(), "world_pos": guides["world_pos"].copy()}
    st["color"] = np.zeros((h, w, 4), np.float32)
    st["color"][..., :3] = rng.uniform(0.05, 2.0, (h, w, 3))
    st["moment2"] = np.zeros((h, w, 4), np.float32)
    st["moment2"][..., :3] = st["color"][..., :3] ** 2 + rng.uniform(0.0, 1.0, (h, w, 3))
    st["moment2"][..., 3] = rng.uniform(1.0, 20.0, (h, w))
    return st


def f32_f64_gap(render, make_camera):
    """The largest f32 - f64 gap of the restatement over the GPU test's cases, on non-fragile pixels:
    (all outputs but color_std, color_std, {case: fragile share}). render(w, h, camera, frame0)
    returns (color, features) of one 1 spp frame; make_camera(*orbit_args(...)) a camera."""
    worst, worst_std, shares = 0.0, 0.0, {}
    for w, h in SHAPES:
        for dt in DTHETAS:
            cam0, cam1 = (make_camera(*orbit_args(t, w, h)) for t in (-dt, 0.0))
            _, g0 = render(w, h, cam0, FRAME0)
            color, cur = render(w, h, cam1, FRAME0)
            prev = random_prev({k: g0[k] * np.float32(CUR_SCALE) for k in ("normal", "world_pos")}, 1000 * w + h)
            a, fa = step(color, cur, prev, cam1, cam0, np.float32, cur_scale=CUR_SCALE)
            b, fb = step(color, cur, prev, cam1, cam0, np.float64, cur_scale=CUR_SCALE)
            ok = ~(fa | fb)
            shares[(w, h, dt)] = float(fb.mean())
            for name in OUTPUTS:
                g = rel_gap(a[name], b[name], ok)
                if name == "color_std":
                    worst_std = max(worst_std, g)
                else:
                    worst = max(worst, g)
    return worst, worst_std, shares


if __name__ == "__main__":
    import os
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [root, os.path.join(root, "oracle")]
    import oracle
    from learnraytracing_amd import make_camera

    def _render(w, h, camera, frame0):
        feats = {n: np.zeros((h, w, 4), np.float32) for n in ("normal", "world_pos", "albedo")}
        buf, _ = oracle.orc_render_ex(w, h, frames=1, depth=8, frame0=frame0, cam22=cam22(camera), features=feats,
                                      max_frame=-1)
        return buf, feats

    gap, gap_std, shares = f32_f64_gap(_render, make_camera)
    print(f"largest f32 - f64 gap over the GPU test's cases: {gap:.3g} (color_std: {gap_std:.3g})")
    for (w, h, dt), s in shares.items():
        print(f"  {w}x{h} step {dt}: fragile {100 * s:.2f} %")
