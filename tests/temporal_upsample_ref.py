"""NumPy restatement of temporal upsampling (include/lrt.h, lrt_temporal_upsample_*), the cases its
tests share and the scenes they use. A helper module, not a conftest: imported by
tests/test_temporal_upsample_cpu.py and tests/test_gpu_temporal_upsample.py. Built from
tests/upsample_ref.py (the integer taps, the normal weight, the select that keeps a tap out of a sum)
and tests/temporal_gbuffer_ref.py (the history gather and its fragile marks).

Per output pixel p = (x, y) of a width x height history from a low_width x low_height frame whose
camera was shifted by (jitter_x, jitter_y):
  1. a = (2x + 1) low_width - width - jitter_x, X0 = floor(a / (2 width)), r = a - X0 2 width,
     tx = r / (2 width); Y0, ty likewise; taps Q = (X0 + i, Y0 + j), b = (i ? tx : 1 - tx)(j ? ty : 1 - ty)
  2. a tap counts iff inside, b > 0 and id_low(Q) = id_cur(p); w = b g, g = exp(-|N_low(Q) - N_cur(p)|^2
     / sigma_normal^2) for a hit, 1 for a miss; sw = sum w; the frame speaks iff sw >= weight_min:
     I = cur_scale sum w c(Q) / sw, beta = sum w k(Q) / sw, k = exp(-(dx^2 + dy^2) / (2 sigma_sample^2)),
     dx = (i - tx) width / low_width, dy = (j - ty) height / low_height
  3. the history of temporal_gbuffer_ref.step (steps 1 and 2): it counts iff sum b > 1e-3; h, m, n_h
  4. class 0 (both): n = n_h + beta, alpha = max(beta / n, alpha_min beta), color = (1 - alpha) h + alpha I,
     moment2 likewise with I^2; class 1 (history only): h, m, n_h; class 2 (current only): I, I^2, beta;
     class 3 (neither): cur_scale x the bilinear mean over the inside taps with b > 0, its square, n = 0
  5. std = sqrt(max(moment2 - color^2, 0)), or short_std where n < min_history
`fragile` marks the pixels with a decision within its neighbours' margins of its threshold: sw within
1 +- upsample_ref.FRAGILE_REL of weight_min, what temporal_gbuffer_ref.step marks for the history sum,
the normal test and the motion bounds, n against min_history (temporal_ref._near), and a class-0 count
n below N_TINY (beta underflowed over n_h = 0: alpha = max(0 / 0, 0) is 0 under the maximum that ignores
a NaN, the kernel's fmaxf and np.fmax here, where a wider format finds beta / n = 1).

`python tests/temporal_upsample_ref.py` prints the largest gap between the f32 and the f64 run over
the GPU test's cases (F32_F64_GAP* of tests/test_gpu_temporal_upsample.py) with the fragile share and
the class counts per case; the planes come from tests/gbuffer_ref.py's f32 run and the colours from
the oracle there, from the library on the GPU.
"""
import numpy as np

import gbuffer_ref as G
import temporal_gbuffer_ref as TG
import temporal_ref as R
import upsample_ref as U

DEFAULTS = dict(TG.DEFAULTS, sigma_normal=0.3, sigma_sample=0.5, weight_min=1e-3)
OUTPUTS = TG.OUTPUTS
MAX_FRAGILE = U.MAX_FRAGILE
MAX_SIZE = U.MAX_SIZE
N_TINY = 1e-30       # a class-0 count below this is an underflowed beta over n_h = 0: alpha is 0 / 0 in f32
FRAME0, CUR_SCALE = TG.FRAME0, TG.CUR_SCALE


def taps(n_out, n_low, jitter, dtype):
    """(X0 [n_out] int64, t [n_out]) of step 1 along one axis."""
    assert abs(jitter) <= n_out
    x = np.arange(n_out, dtype=np.int64)
    a = (2 * x + 1) * n_low - n_out - int(jitter)
    x0 = a // (2 * n_out)                     # floor, for a negative a too
    r = a - x0 * 2 * n_out
    return x0, (r.astype(dtype) / dtype(2 * n_out)).astype(dtype)


def jitter_camera(camera, w, h, lw, lh, jx, jy):
    """lrt_camera_jitter in NumPy f32: the camera's 22 floats with lowerLeftCorner shifted."""
    c = R.cam22(camera).copy()
    f = np.float32
    sx, sy = (f(jx) / f(2 * w)) / f(lw), (f(jy) / f(2 * h)) / f(lh)
    c[12:15] = (c[12:15] + sx * c[15:18]) + sy * c[18:21]
    return c


def jitter_phases(w, lw, h, lh):
    """renderer.jitter_phases restated: phase p of an axis of ratio R is low (2p + 1 - R)."""
    rx, ry = w // lw, h // lh
    assert rx * lw == w and ry * lh == h
    return [(lw * (2 * (k % rx) + 1 - rx), lh * (2 * ((k // rx + k % rx) % ry) + 1 - ry)) for k in range(rx * ry)]


def step(color_low, low, cur, prev_g, prev, jitter=(0, 0), dtype=np.float64, info=None, **params):
    """One step. color_low [lh, lw, >= 3]; low {"id" [lh, lw], "normal" [lh, lw, >= 3]}; cur {"normal",
    "motion" [h, w, 4], "id" [h, w]}; prev_g {"normal", "id"} and prev {"color", "moment2"}, or None
    and None. Arithmetic in `dtype`. Returns (state, cls [h, w] int32, fragile [h, w]); state maps
    OUTPUTS to [h, w, 3] arrays ("n": [h, w]). info: a dict to fill with beta, sw, speaks, counts (the
    history was taken), n_h, inside (the inside taps with b > 0, 1..4), matched (those of the pixel's
    id) and short_history."""
    p = dict(DEFAULTS, **params)
    T = dtype
    assert (prev is None) == (prev_g is None)
    idl, idc = np.asarray(low["id"]).astype(np.int64), np.asarray(cur["id"]).astype(np.int64)
    lh, lw = idl.shape
    h, w = idc.shape
    assert 1 <= lw <= w <= MAX_SIZE and 1 <= lh <= h <= MAX_SIZE
    c = np.asarray(color_low)[..., :3].astype(T)
    nl, nc = np.asarray(low["normal"])[..., :3].astype(T), np.asarray(cur["normal"])[..., :3].astype(T)
    x0, tx = taps(w, lw, jitter[0], T)
    y0, ty = taps(h, lh, jitter[1], T)
    X0, Y0 = np.broadcast_to(x0[None, :], (h, w)), np.broadcast_to(y0[:, None], (h, w))
    TX, TY = np.broadcast_to(tx[None, :], (h, w)), np.broadcast_to(ty[:, None], (h, w))
    hit = idc >= 0
    inv_s2 = T(1) / (T(p["sigma_normal"]) * T(p["sigma_normal"]))
    inv_2ss = T(1) / (T(2) * T(p["sigma_sample"]) * T(p["sigma_sample"]))
    rx, ry = T(w) / T(lw), T(h) / T(lh)

    def sel(on, v):                # a tap that is off adds nothing, whatever its colour holds
        return np.where(on[..., None], v, T(0))

    zero, zero3 = np.zeros((h, w), T), np.zeros((h, w, 3), T)
    sw, sk, sb, s0, s3 = zero.copy(), zero.copy(), zero.copy(), zero3.copy(), zero3.copy()
    ninside, matched = np.zeros((h, w), np.int64), np.zeros((h, w), np.int64)
    with np.errstate(all="ignore"):
        for j in (0, 1):
            for i in (0, 1):
                gx, gy = X0 + i, Y0 + j
                inside = (gx >= 0) & (gx < lw) & (gy >= 0) & (gy < lh)
                cx, cy = np.clip(gx, 0, lw - 1), np.clip(gy, 0, lh - 1)
                b = ((TX if i else T(1) - TX) * (TY if j else T(1) - TY)).astype(T)
                inb = inside & (b > 0)
                sb += np.where(inb, b, T(0))
                s3 += sel(inb, b[..., None] * c[cy, cx])
                d = nl[cy, cx] - nc
                g = np.where(hit, np.exp(-(d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2]) * inv_s2),
                             T(1)).astype(T)
                wq = b * g
                on = inb & (idl[cy, cx] == idc) & (wq > 0)
                dx, dy = (T(i) - TX) * rx, (T(j) - TY) * ry
                kq = np.exp(-(dx * dx + dy * dy) * inv_2ss).astype(T)
                sw += np.where(on, wq, T(0))
                sk += np.where(on, wq * kq, T(0))
                s0 += sel(on, wq[..., None] * c[cy, cx])
                ninside += inb
                matched += on
        wmin = T(p["weight_min"])
        speaks = sw >= wmin
        fragile = np.abs(sw - wmin) <= T(U.FRAGILE_REL) * wmin
        k = T(p["cur_scale"])
        I = k * (s0 / sw[..., None])
        beta = sk / sw
        flat = k * (s3 / sb[..., None])
        counts = np.zeros((h, w), bool)
        hc, hm, n_h = zero3, zero3, zero
        if prev is not None:
            # the history: temporal_gbuffer_ref.step's gather restated, its fragile marks taken from it
            # (min_history out of reach there: its n is not this step's)
            tinfo = {}
            _, fh = TG.step(np.zeros((h, w, 3), T), cur, prev_g, prev, T, info=tinfo, normal_min=p["normal_min"],
                            min_history=1e30)
            fragile |= fh
            mv = np.asarray(cur["motion"]).astype(T)
            ys, xs = np.mgrid[0:h, 0:w]
            fx, fy = xs.astype(T) + mv[..., 0], ys.astype(T) + mv[..., 1]
            ok = (mv[..., 3] != 0) & (np.abs(fx) < T(1e6)) & (np.abs(fy) < T(1e6))
            fx, fy = np.where(ok, fx, T(0)), np.where(ok, fy, T(0))
            flx, fly = np.floor(fx), np.floor(fy)
            htx, hty = (fx - flx).astype(T), (fy - fly).astype(T)
            hx0, hy0 = flx.astype(np.int64), fly.astype(np.int64)
            pc = np.asarray(prev["color"])[..., :3].astype(T)
            pm = np.asarray(prev["moment2"]).astype(T)
            pn = np.asarray(prev_g["normal"])[..., :3].astype(T)
            pid = np.asarray(prev_g["id"]).astype(np.int64)
            hw, sn, sc, sm = zero.copy(), zero.copy(), zero3.copy(), zero3.copy()
            for j in (0, 1):
                for i in (0, 1):
                    gx, gy = hx0 + i, hy0 + j
                    inside = ok & (gx >= 0) & (gx < w) & (gy >= 0) & (gy < h)
                    cx, cy = np.clip(gx, 0, w - 1), np.clip(gy, 0, h - 1)
                    b = (htx if i else T(1) - htx) * (hty if j else T(1) - hty)
                    same = (pid[cy, cx] == idc) & (~hit | ((pn[cy, cx] * nc).sum(-1) >= T(p["normal_min"])))
                    bw = np.where(inside & same, b, T(0))
                    hw += bw
                    sn += bw * pm[cy, cx, 3]
                    sc += bw[..., None] * pc[cy, cx]
                    sm += bw[..., None] * pm[cy, cx, :3]
            counts = hw > T(1e-3)
            assert np.array_equal(counts, tinfo["keep"])
            hc, hm, n_h = sc / hw[..., None], sm / hw[..., None], sn / hw
        cls = np.where(speaks, np.where(counts, 0, 2), np.where(counts, 1, 3)).astype(np.int32)
        n0 = n_h + beta
        # beta = n_h = 0 (k underflowed under a small sigma_sample, over a history of count 0): beta / n is
        # 0 / 0, and the maximum that ignores a NaN (fmaxf in the kernel) leaves alpha = 0. With more
        # exponent range beta / n is 1 there, so the formats disagree: fragile.
        al = np.fmax(beta / n0, T(p["alpha_min"]) * beta)[..., None]
        fragile |= (cls == 0) & (n0 < T(N_TINY))
        pick = lambda a0, a1, a2, a3: np.where((cls == 0)[..., None], a0, np.where((cls == 1)[..., None], a1,   # noqa: E731
                                               np.where((cls == 2)[..., None], a2, a3)))
        col = pick((T(1) - al) * hc + al * I, hc, I, flat)
        m2 = pick((T(1) - al) * hm + al * (I * I), hm, I * I, flat * flat)
        n = pick(n0[..., None], n_h[..., None], beta[..., None], zero[..., None])[..., 0]
        fragile |= R._near(n, T(p["min_history"]))
        short = n < T(p["min_history"])
        std = np.where(short[..., None], T(p["short_std"]), np.sqrt(np.maximum(m2 - col * col, T(0))))
    if info is not None:
        info.update(beta=beta, sw=sw, speaks=speaks, counts=counts, n_h=n_h, inside=ninside, matched=matched,
                    short_history=short)
    return dict(color=col.astype(T), moment2=m2.astype(T), n=n.astype(T), color_std=std.astype(T)), cls, fragile


def class_counts(cls):
    return tuple(int((cls == k).sum()) for k in range(4))


as_state, quad = TG.as_state, TG.quad


# ---- the rendered cases of tests/test_gpu_temporal_upsample.py::test_step_vs_restatement:
# (label, sphere count, w, h, lw, lh)
RENDERED_CASES = (
    ("1x1 from 1x1", 9, 1, 1, 1, 1),
    ("2x2 from 1x1", 9, 2, 2, 1, 1),
    ("5x3 from 3x2", 9, 5, 3, 3, 2),
    ("66x44 from 33x22", 9, 66, 44, 33, 22),
    ("67x45 from 33x22", 9, 67, 45, 33, 22),      # a non-integer ratio, partial blocks
    ("257x9 from 129x5", 9, 257, 9, 129, 5),
    ("96x8 from 32x8", 9, 96, 8, 32, 8),          # ratio 3 by 1
    ("19x13 from 19x13", 9, 19, 13, 19, 13),      # ratio 1
    ("1 sphere", 1, 38, 26, 19, 13),
    ("16 spheres", 16, 38, 26, 19, 13),
    ("17 spheres", 17, 38, 26, 19, 13),
    ("1000 spheres", 1000, 38, 26, 19, 13),
)
JITTER_NAMES = ("zero", "aligned", "extreme", "odd")
RENDERED_PARAMS = dict(cur_scale=CUR_SCALE)


def case_jitters(w, h, lw, lh):
    """The four jitters of a case, as JITTER_NAMES: (0, 0); an aligned phase (the first of x and the
    last of y at the whole part of the ratio: a low sample on a pixel centre where the ratio is whole);
    (+width, -height), the limits; (7, -3), cut to the limits where the frame is smaller."""
    return ((0, 0), (-lw * (w // lw - 1), lh * (h // lh - 1)), (w, -h), (min(7, w), max(-3, -h)))


def rendered_case(count, w, h, lw, lh, jit_a, jit_b, scene_of, make_camera, jitter_cam, planes, colour):
    """(a, b) of one rendered case, each {"color_low", "low", "cur", "jitter"}: step a is the previous
    frame (the camera one orbit step back, the moved scene) under jitter jit_a, with no history and
    zero motion; step b the current frame under jit_b, whose motion points back at a.
    scene_of(count) -> (spheres, materials); jitter_cam(camera, w, h, lw, lh, jx, jy) -> the low camera;
    planes and colour as temporal_gbuffer_ref.rendered_case takes them."""
    spheres, mats = scene_of(count)
    cur_s, prev_s = G.sphere_array(spheres), TG.moved_scene(spheres)
    cam, pcam = G.camera_pair(make_camera, w, h, TG.DTHETA)

    def one(camera, scene, jit, prev_camera, prev_scene):
        jc = jitter_cam(camera, w, h, lw, lh, *jit)
        low = planes(lw, lh, jc, scene, mats, None, None)
        return dict(color_low=colour(lw, lh, jc, scene, mats, FRAME0), low={k: low[k] for k in ("id", "normal")},
                    cur=planes(w, h, camera, scene, mats, prev_camera, prev_scene), jitter=tuple(jit))

    return one(pcam, prev_s, jit_a, pcam, None), one(cam, cur_s, jit_b, pcam, prev_s)


def two_steps(a, b, dtype, first=None):
    """The two steps of a rendered case in `dtype`: ((state, cls, fragile) of a, the same of b). The
    history of b is `first` (the state the library returned for a) or a's own outputs as float32.
    After two steps n <= 2 < min_history: every color_std here is short_std itself (the designed cases
    hold the other branch; a lower min_history would put n = 1 and n = 2, which aligned samples give
    exactly, on its threshold)."""
    ra = step(a["color_low"], a["low"], a["cur"], None, None, a["jitter"], dtype, **RENDERED_PARAMS)
    prev = first if first is not None else as_state(ra[0])
    prev_g = {k: a["cur"][k] for k in ("normal", "id")}
    rb = step(b["color_low"], b["low"], b["cur"], prev_g, prev, b["jitter"], dtype, **RENDERED_PARAMS)
    return ra, rb


def gaps(ra, rb, worst):
    """The f32 - f64 (or got - f64) gaps of one step folded into worst = {"all", "std"}; the classes
    must agree off both fragile masks."""
    ok = ~(ra[2] | rb[2])
    assert np.array_equal(ra[1][ok], rb[1][ok])
    for name in OUTPUTS:
        key = "std" if name == "color_std" else "all"
        worst[key] = max(worst[key], R.rel_gap(ra[0][name], rb[0][name], ok))


def rendered_gap(scene_of, make_camera, jitter_cam, planes, colour):
    """(all outputs but color_std, color_std, {label: (largest fragile share, class counts of step b
    under the last jitter)}) of the f32 - f64 gap over RENDERED_CASES under every jitter."""
    worst, report = {"all": 0.0, "std": 0.0}, {}
    for label, count, w, h, lw, lh in RENDERED_CASES:
        jits = case_jitters(w, h, lw, lh)
        share = 0.0
        for k, jit in enumerate(jits):
            a, b = rendered_case(count, w, h, lw, lh, jits[k - 1], jit, scene_of, make_camera, jitter_cam, planes, colour)
            r32, r64 = two_steps(a, b, np.float32), two_steps(a, b, np.float64)
            for s32, s64 in zip(r32, r64):
                gaps(s32, s64, worst)
                share = max(share, float(s64[2].mean()))
        report[label] = (share, class_counts(r64[1][1]))
    return worst["all"], worst["std"], report


# ---- the designed cases: 12 x 8 from 6 x 4 planes written by hand so that each branch holds pixels
DESIGNED_SIZE, DESIGNED_LOW = (12, 8), (6, 4)
DESIGNED_CASES = ("all_classes", "aligned", "other_id_near", "normal_refused", "mw_zero", "borders", "min_history",
                  "no_prev")
UP, SIDE = TG.UP, TG.SIDE


def designed_inputs(case, seed=0):
    """(color_low, low, cur, prev_g, prev, jitter, params, expect) of one designed case. expect maps a
    name to (mask [h, w], value): "cls", "inside", "matched", "short_history" as the restatement's class
    plane and info must show them on those pixels; "beta_is_1": beta = 1 exactly there; "beta_below":
    beta < value there. By default every pixel of all frames shows sphere 0 with the normal UP, does
    not move, and the jitter is 0: every pixel is class 0."""
    (w, h), (lw, lh) = DESIGNED_SIZE, DESIGNED_LOW
    rng = np.random.default_rng([seed, 40 + DESIGNED_CASES.index(case)])
    color = np.zeros((lh, lw, 4), np.float32)
    color[..., :3] = rng.uniform(0.05, 2.0, (lh, lw, 3))
    color[..., 3] = 1
    low = {"normal": quad(np.broadcast_to(np.float32(UP), (lh, lw, 3))), "id": np.zeros((lh, lw), np.int32)}
    cur = {"normal": quad(np.broadcast_to(np.float32(UP), (h, w, 3))), "motion": np.zeros((h, w, 4), np.float32),
           "id": np.zeros((h, w), np.int32)}
    cur["motion"][..., 3] = 1
    prev_g = {"normal": cur["normal"].copy(), "id": cur["id"].copy()}
    prev = TG.random_state(w, h, 177 + DESIGNED_CASES.index(case))
    jitter, params = (0, 0), {}
    ys, xs = np.mgrid[0:h, 0:w]
    every = np.ones((h, w), bool)
    if case == "all_classes":
        a, b, c3 = (ys < 4) & (xs >= 8), (ys >= 5) & (xs < 4), (ys >= 5) & (xs >= 8)
        cur["id"][a] = prev_g["id"][a] = 7          # a sphere the low frame does not show, the history does
        prev_g["id"][b] = 5                         # the history shows another sphere
        cur["id"][c3] = 8                           # a sphere neither shows
        cls = np.zeros((h, w), np.int32)
        cls[a], cls[b], cls[c3] = 1, 2, 3
        expect = {"cls": (every, cls)}
    elif case == "aligned":        # the first phase: the pixels of even x and y sit on a low sample
        jitter = (-lw, -lh)
        on = (xs % 2 == 0) & (ys % 2 == 0)
        expect = {"cls": (every, 0), "beta_is_1": (on, True), "beta_below": (~on, 0.2), "matched": (on, 1)}
    elif case == "other_id_near":  # output (5, 3): its nearest low sample (2, 1) is another sphere, the far three its own
        low["id"][1, 2] = 1
        mask = (xs == 5) & (ys == 3)
        expect = {"cls": (mask, 0), "matched": (mask, 3), "beta_below": (mask, 0.02)}
    elif case == "normal_refused":  # a history of the pixel's id whose normals disagree on the right: the frame alone
        right = xs >= w // 2
        prev_g["normal"][right, :3] = SIDE
        expect = {"cls": (every, np.where(right, 2, 0))}
    elif case == "mw_zero":        # not projectable: no history, whatever x and y hold
        cur["motion"][..., 3] = 0
        cur["motion"][::2, :, 0] = 3e7
        expect = {"cls": (every, 2)}
    elif case == "borders":        # the limits of the jitter: half a low pixel right and up
        jitter = (w, -h)
        # a_x = 12 x - 18 over 24: X0 = -1 in columns 0 and 1; a_y = 8 y + 4 over 16: Y0 + 1 = 4 in rows 6 and 7
        inside = np.full((h, w), 4)
        inside[:, [0, 1]] = inside[[h - 2, h - 1], :] = 2
        inside[h - 2:, :2] = 1
        expect = {"cls": (every, 0), "inside": (every, inside), "matched": (every, inside)}
    elif case == "min_history":    # beta ~ 0.21 under jitter 0: n = n' + beta on either side of 4, both fractional
        prev["moment2"][..., 3] = np.where(xs < w // 2, 3.7, 3.9)
        inner = (xs >= 1) & (xs <= w - 2) & (ys >= 1) & (ys <= h - 2)
        expect = {"cls": (every, 0), "short_history": (inner, (xs < w // 2)[inner])}
    elif case == "no_prev":        # no history: classes 2 and 3 only
        prev_g = prev = None
        cur["id"][2:5, 3:6] = 7
        expect = {"cls": (every, np.where(cur["id"] == 7, 3, 2))}
    else:
        raise ValueError(f"unknown designed case {case!r}")
    return color, low, cur, prev_g, prev, jitter, params, expect


def nan_inputs():
    """(color_low, the same with the marked colour zeroed, low, cur, prev_g, prev, jitter, untouched,
    b0): the `aligned` case with NaN and Inf as the colour of low (3, 2). untouched [h, w]: the pixels
    that give that tap no weight > 0; b0: those of them that have it as a tap of b = 0 (column 4, where
    tx = 0 and X0 + 1 = 3)."""
    color, low, cur, prev_g, prev, jitter, _, _ = designed_inputs("aligned")
    zeroed = color.copy()
    zeroed[2, 3, :3] = 0
    color = color.copy()
    color[2, 3, :3] = np.float32([np.nan, np.inf, -np.inf])
    (w, h), (lw, lh) = DESIGNED_SIZE, DESIGNED_LOW
    x0, tx = taps(w, lw, jitter[0], np.float64)
    y0, ty = taps(h, lh, jitter[1], np.float64)
    touched = np.zeros((h, w), bool)
    b0 = np.zeros((h, w), bool)
    for j in (0, 1):
        for i in (0, 1):
            at = ((x0 + i)[None, :] == 3) & ((y0 + j)[:, None] == 2)
            b = (tx if i else 1 - tx)[None, :] * (ty if j else 1 - ty)[:, None]
            touched |= at & (b > 0)
            b0 |= at & (b == 0)
    return color, zeroed, low, cur, prev_g, prev, jitter, ~touched, b0 & ~touched


def beta_zero_inputs():
    """(color_low, low, cur, prev_g, prev, jitter, params, mask): the default designed frame under
    sigma_sample 0.03, where every k underflows to 0 in f32 (exp(-278) at the nearest sample), over a
    history whose count is 0 on the left half (mask): beta = n = 0 there."""
    color, low, cur, prev_g, prev, jitter, params, _ = designed_inputs("min_history")
    left = np.mgrid[0:DESIGNED_SIZE[1], 0:DESIGNED_SIZE[0]][1] < DESIGNED_SIZE[0] // 2
    prev["moment2"][..., 3] = np.where(left, 0.0, 2.5)
    return color, low, cur, prev_g, prev, jitter, dict(params, sigma_sample=0.03), left


def designed_gap():
    """(all outputs but color_std, color_std, {case: (fragile share, class counts)}) of the f32 - f64
    gap over the designed cases."""
    worst, report = {"all": 0.0, "std": 0.0}, {}
    for case in DESIGNED_CASES:
        color, low, cur, prev_g, prev, jitter, params, _ = designed_inputs(case)
        r32 = step(color, low, cur, prev_g, prev, jitter, np.float32, **params)
        r64 = step(color, low, cur, prev_g, prev, jitter, np.float64, **params)
        gaps(r32, r64, worst)
        report[case] = (float(r64[2].mean()), class_counts(r64[1]))
    return worst["all"], worst["std"], report


# ---- what it is for: a static frame of misses rebuilt exactly from its jittered low samples
CONVERGE_SIZES = ((16, 12, 8, 6), (18, 10, 9, 5))
CONVERGE_SIGMA = 0.15


def converge_target(w, h, seed=5):
    return np.random.default_rng(seed).uniform(0.0, 1.0, (h, w, 3))


def converge(w, h, lw, lh, step_fn, steps=4):
    """Cycle jitter_phases over a frame of misses whose low colours are the target T at the pixels the
    phase's samples sit on. step_fn(color_low [lh, lw, 4] f64, low, cur, prev_g, prev, jitter) ->
    (state as as_state gives it, cls). Returns [(cls, max |color - T|)] per step."""
    target = converge_target(w, h)
    rx, ry = w // lw, h // lh
    low = {"normal": np.zeros((lh, lw, 4), np.float32), "id": np.full((lh, lw), -1, np.int32)}
    out, prev, prev_g = [], None, None
    for t, (jx, jy) in zip(range(steps), jitter_phases(w, lw, h, lh) * steps):
        px, py = (jx // lw + rx - 1) // 2, (jy // lh + ry - 1) // 2
        color = np.zeros((lh, lw, 4))
        color[..., :3] = target[py::ry, px::rx]
        cur = {"normal": np.zeros((h, w, 4), np.float32), "motion": np.zeros((h, w, 4), np.float32),
               "id": np.full((h, w), -1, np.int32)}        # fresh planes every step: the previous ones are the history
        cur["motion"][..., 3] = 1
        state, cls = step_fn(color, low, cur, prev_g, prev, (jx, jy))
        out.append((cls, float(np.abs(np.asarray(state["color"], np.float64)[..., :3] - target).max())))
        prev, prev_g = state, {k: cur[k] for k in ("normal", "id")}
    return out


def converge_ref(w, h, lw, lh, dtype, steps=4):
    def fn(color, low, cur, prev_g, prev, jitter):
        st, cls, _ = step(color, low, cur, prev_g, prev, jitter, dtype, sigma_sample=CONVERGE_SIGMA)
        return as_state(st, dtype), cls
    return converge(w, h, lw, lh, fn, steps)


# ---- the CPU stand-ins of the library's planes and colours (the oracle renders the colours)
cpu_planes, cpu_colour, scene_of = TG.cpu_planes, TG.cpu_colour, TG.scene_of


if __name__ == "__main__":
    import os
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [root, os.path.join(root, "oracle")]
    from learnraytracing_amd import default_scene, make_camera, random_scene

    for title, (gap, gap_std, report) in (
            ("rendered", rendered_gap(scene_of(default_scene, random_scene), make_camera, jitter_camera, cpu_planes,
                                      cpu_colour)),
            ("designed", designed_gap())):
        print(f"largest f32 - f64 gap over the {title} cases: {gap:.3g} (color_std: {gap_std:.3g})")
        for label, (share, counts) in report.items():
            print(f"  {label}: fragile {100 * share:.2f} %, class 0 / 1 / 2 / 3: " + " / ".join(map(str, counts)))
    for w, h, lw, lh in CONVERGE_SIZES:
        for T in (np.float64, np.float32):
            print(f"{w}x{h} from {lw}x{lh} in {np.dtype(T).name}: |color - T| per step "
                  + ", ".join(f"{e:.3g}" for _, e in converge_ref(w, h, lw, lh, T)))
