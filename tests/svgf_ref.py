"""NumPy restatement of the variance-guided a-trous filter over the temporal state (include/lrt.h,
lrt_svgf_*), the inputs and case tables its tests share. A helper module, not a conftest: imported
by tests/test_svgf_cpu.py and tests/test_gpu_svgf.py.

Stage 0, per pixel p (C = color.rgb, M = moment2.rgb, n = moment2.a):
    hit = |N|^2 >= 0.25 if normal is given, else true
    D   = max(A, albedo_floor) if albedo is given and hit, else 1
    v   = max(M - C^2, 0)                                   if n >= min_history
        = max(m2 - m1^2, 0) * (min_history / max(n, 1))      otherwise: m1, m2 the g-weighted means of
          C and M over the 7x7 window (inside the image), g = exp(-(|dn|^2 / sigma_normal^2 + |dx|^2 / sigma_pos^2))
    c_0 = C / D, var_0 = v / D^2
Passes k = 0 .. K - 1, taps q = p + 2^k (i, j), i, j in -2..2 (inside the image), h = [1/16, 1/4, 3/8, 1/4, 1/16]:
    vt(p) = the 3x3 [1/4, 1/2, 1/4]^2 mean of var_k around p (undilated, normalised over the taps inside)
    E = |c_k(p) - c_k(q)|^2 / (sigma_color^2 (vt.r + vt.g + vt.b) + 1e-6) + |dn|^2 / sigma_normal^2 + |dx|^2 / sigma_pos^2
    w = h[i] h[j] exp(-E);  c_{k+1} = sum w c_k(q) / sum w;  var_{k+1} = sum w^2 var_k(q) / (sum w)^2
End: out = c_K D, variance_out = var_K D^2.

`python tests/svgf_ref.py` prints the largest gap between the f32 and the f64 run over each of the GPU
tests' two case tables, colour and variance separately (the constants of tests/test_gpu_svgf.py).
"""
import numpy as np

import denoise_ref as DR

DEFAULTS = dict(iterations=5, min_history=4, sigma_color=4.0, sigma_normal=0.3, sigma_pos=0.5, albedo_floor=0.01)
H5 = DR.H5
B3 = (1 / 4, 1 / 2, 1 / 4)
GUIDE_NAMES = ("normal", "world_pos", "albedo")


def _shifted(h, w, dy, dx):
    """(ys, xs, yq, xq): the pixels p whose tap p + (dx, dy) is inside the image, and those taps; None if none."""
    ys = slice(max(0, -dy), h - max(0, dy))
    xs = slice(max(0, -dx), w - max(0, dx))
    if ys.start >= ys.stop or xs.start >= xs.stop:
        return None
    return ys, xs, slice(ys.start + dy, ys.stop + dy), slice(xs.start + dx, xs.stop + dx)


def _geometry(guides, p, T, sl):
    """|dn|^2 / sigma_normal^2 + |dx|^2 / sigma_pos^2 of the taps of `sl` (a term is dropped if its guide is absent)."""
    ys, xs, yq, xq = sl
    e = np.zeros((ys.stop - ys.start, xs.stop - xs.start), T)
    for name, sig in (("normal", "sigma_normal"), ("world_pos", "sigma_pos")):
        if name in guides:
            g = guides[name]
            e += ((g[ys, xs] - g[yq, xq]) ** 2).sum(-1) / (T(p[sig]) * T(p[sig]))
    return e


def svgf(color, moment2, guides=None, dtype=np.float64, **params):
    """The filter on color[h, w, >=3], moment2[h, w, 4] (n in its alpha) with guides {name: [h, w, >=3]}
    ("normal", "world_pos", "albedo"; a missing or None guide drops its term; other names are not
    read). Arithmetic in `dtype`. Returns (colour, variance), rgb [h, w, 3] each, in `dtype`."""
    p = dict(DEFAULTS, **params)
    T = dtype
    guides = {k: np.asarray(v)[..., :3].astype(T) for k, v in (guides or {}).items()
              if v is not None and k in GUIDE_NAMES}
    C = np.asarray(color)[..., :3].astype(T)
    M = np.asarray(moment2)[..., :3].astype(T)
    n = np.asarray(moment2)[..., 3].astype(T)
    h, w = C.shape[:2]
    mh = T(p["min_history"])
    # stage 0
    hit = (guides["normal"] ** 2).sum(-1) >= T(0.25) if "normal" in guides else np.ones((h, w), bool)
    D = np.ones_like(C)
    if "albedo" in guides:
        D = np.where(hit[..., None], np.maximum(guides["albedo"], T(p["albedo_floor"])), T(1))
    v = np.maximum(M - C * C, T(0))
    short = ~(n >= mh)
    if short.any():
        sg = np.zeros((h, w), T)
        s1, s2 = np.zeros_like(C), np.zeros_like(C)
        for j in range(-3, 4):
            for i in range(-3, 4):
                sl = _shifted(h, w, j, i)
                if sl is None:
                    continue
                ys, xs, yq, xq = sl
                g = np.exp(-_geometry(guides, p, T, sl))
                sg[ys, xs] += g
                s1[ys, xs] += g[..., None] * C[yq, xq]
                s2[ys, xs] += g[..., None] * M[yq, xq]
        m1, m2 = s1 / sg[..., None], s2 / sg[..., None]
        vs = np.maximum(m2 - m1 * m1, T(0)) * (mh / np.maximum(n, T(1)))[..., None]
        v = np.where(short[..., None], vs, v)
    c, var = C / D, v / (D * D)
    # the passes
    sc2 = T(p["sigma_color"]) * T(p["sigma_color"])
    for k in range(int(p["iterations"])):
        s = 1 << k
        vsum = var.sum(-1)
        num, bsum = np.zeros((h, w), T), np.zeros((h, w), T)
        for j in range(-1, 2):
            for i in range(-1, 2):
                sl = _shifted(h, w, j, i)
                if sl is None:
                    continue
                ys, xs, yq, xq = sl
                b = T(B3[i + 1]) * T(B3[j + 1])
                num[ys, xs] += b * vsum[yq, xq]
                bsum[ys, xs] += b
        inv_c = T(1) / (sc2 * (num / bsum) + T(1e-6))
        cn, vn = np.zeros_like(c), np.zeros_like(var)
        den = np.zeros((h, w), T)
        for j in range(-2, 3):
            for i in range(-2, 3):
                sl = _shifted(h, w, j * s, i * s)
                if sl is None:
                    continue
                ys, xs, yq, xq = sl
                e = ((c[ys, xs] - c[yq, xq]) ** 2).sum(-1) * inv_c[ys, xs] + _geometry(guides, p, T, sl)
                wq = T(H5[i + 2]) * T(H5[j + 2]) * np.exp(-e)
                cn[ys, xs] += wq[..., None] * c[yq, xq]
                vn[ys, xs] += (wq * wq)[..., None] * var[yq, xq]
                den[ys, xs] += wq
        c = cn / den[..., None]
        var = vn / (den * den)[..., None]
    return c * D, var * (D * D)


# ---- the synthetic inputs of tests/test_gpu_svgf.py
SHAPES = DR.SHAPES
ITERATIONS = DR.ITERATIONS
GUIDE_SETS = {"all": GUIDE_NAMES, "none": (), "normal": ("normal",), "no_albedo": ("normal", "world_pos")}
N_VALUES = np.float32([1, 2, 3, 5, 17.5, 40])
VARIANTS = ("n1", "n40", "var0", "fireflies", "dirty_alpha", "far_origin", "albedo0")
HIT_MARGIN = 1e-4   # no pixel's |N|^2 lies within this (relative) of 0.25: asserted by hit_margin()


def synthetic_inputs(w, h, seed=0, variant=None):
    """(color, moment2, guides): float32 [h, w, 4] buffers, from denoise_ref.synthetic_inputs(w, h, seed):
    its colour, normal, world_pos and albedo; moment2 rgb = C^2 + std^2 with its std in [0.05, 1]; n
    (moment2's alpha) drawn from N_VALUES in 6 x 4 blocks; a contiguous region of about a tenth of the
    pixels (the upper right corner) a miss: normal 0, albedo 0.
    variant (one of VARIANTS) changes that frame afterwards, from a generator of its own:
      n1 / n40     n = 1 / n = 40 everywhere
      var0         moment2 rgb = C^2 exactly (computed in f32) on a third of the pixels
      fireflies    up to five pixels at 1e4 and one at 65504 (moment2 = C^2 + std^2 of the new colour)
      dirty_alpha  NaN, +Inf and 1e30 in the alpha of every guide buffer and of color
      far_origin   world_pos rgb shifted by denoise_ref.FAR_ORIGIN, in f32
      albedo0      albedo exactly 0 on a third of the hit pixels (the floor)"""
    if variant is not None and variant not in VARIANTS:
        raise ValueError(f"unknown variant {variant!r}")
    color, g = DR.synthetic_inputs(w, h, seed)
    std = g.pop("color_std")
    rng = np.random.default_rng([7, w, h, seed])
    y, x = np.mgrid[0:h, 0:w]
    miss = (x >= w - max(w // 3, 1)) & (y >= h - max(h // 3, 1)) if w * h > 1 else np.zeros((h, w), bool)
    g["normal"][miss] = 0.0
    g["albedo"][miss] = 0.0
    blocks = rng.integers(0, len(N_VALUES), ((h + 3) // 4, (w + 5) // 6))
    n = N_VALUES[blocks[y // 4, x // 6]]
    vr = np.random.default_rng([8, VARIANTS.index(variant) if variant else 99, w, h, seed])
    if variant == "n1":
        n = np.full((h, w), 1.0, np.float32)
    elif variant == "n40":
        n = np.full((h, w), 40.0, np.float32)
    elif variant == "fireflies":
        at = vr.choice(w * h, min(6, w * h), replace=False)
        rgb = color.reshape(-1, 4)[:, :3]
        rgb[at] = 1e4
        rgb[at[-1]] = 65504.0
    elif variant == "dirty_alpha":
        junk = np.float32([np.nan, np.inf, 1e30])
        for buf in list(g.values()) + [color]:
            buf[..., 3] = junk[vr.integers(0, 3, (h, w))]
    elif variant == "far_origin":
        g["world_pos"][..., :3] += np.float32(DR.FAR_ORIGIN)
    elif variant == "albedo0":
        g["albedo"][..., :3][(vr.integers(0, 3, (h, w)) == 0) & ~miss] = 0.0
    moment2 = np.empty((h, w, 4), np.float32)
    moment2[..., :3] = color[..., :3] ** 2 + std[..., :3] ** 2
    if variant == "var0":
        third = vr.integers(0, 3, (h, w)) == 0
        moment2[..., :3][third] = color[..., :3][third] ** 2
    moment2[..., 3] = n
    return color, moment2, {k: np.ascontiguousarray(v, np.float32) for k, v in g.items()}


def hit_margin(guides):
    """The smallest relative distance of a pixel's |N|^2 (in f64, of the f32 inputs) from 0.25."""
    if "normal" not in guides:
        return np.inf
    n2 = (np.float64(guides["normal"][..., :3]) ** 2).sum(-1)
    return float(np.abs(n2 / 0.25 - 1.0).min())


def rel_gap(a, ref):
    return DR.rel_gap(a, ref)


def case(w, h, iterations=5, guides=None, variant=None, variance=True, **params):
    """One filter call of a case table: synthetic_inputs(w, h, variant=variant), the guides named
    (default: all three), whether variance_out is asked for, svgf's parameters."""
    return dict(w=w, h=h, variant=variant, guides=tuple(GUIDE_NAMES if guides is None else guides),
                variance=variance, params=dict(params, iterations=iterations))


def case_label(c):
    extra = "".join(f" {k}={v:g}" for k, v in c["params"].items() if k != "iterations")
    return (f"{c['w']}x{c['h']} iterations={c['params']['iterations']} guides={'+'.join(c['guides']) or 'none'}"
            f"{extra}{' ' + c['variant'] if c['variant'] else ''}{'' if c['variance'] else ' no variance_out'}")


def case_inputs(c):
    """(color, moment2, the case's guides) of one case."""
    color, moment2, guides = synthetic_inputs(c["w"], c["h"], variant=c["variant"])
    return color, moment2, {k: guides[k] for k in c["guides"]}


def default_table():
    """The cases of test_svgf_vs_restatement: SHAPES x ITERATIONS x GUIDE_SETS, variance_out on; off
    (the same filter, one output less) for the first and the last iteration count with all guides."""
    t = [case(w, h, it, names) for w, h in SHAPES for it in ITERATIONS for names in GUIDE_SETS.values()]
    return t + [case(w, h, it, variance=False) for w, h in SHAPES for it in (ITERATIONS[0], ITERATIONS[-1])]


# ---- the edge table of tests/test_gpu_svgf.py::test_svgf_edges_vs_restatement: a base case (67x45,
# 5 iterations, all guides, the defaults) and sweeps of one axis each from it.
EDGE_BASE = (67, 45)
EDGE_SHAPES = ((1, 130), (63, 5), (64, 4), (65, 8), (129, 65), (70, 129), (64, 64))
EDGE_SHAPE_ITERATIONS = (3, 4, 5)
EDGE_WIDE = (16384, 40)       # more workgroups than are resident at once (denoise_ref.EDGE_WIDE), at K = 4
EDGE_MIN_HISTORY = (1, 4, 100)
SIGMAS = ("sigma_color", "sigma_normal", "sigma_pos")
EDGE_SIGMA_FACTORS = (0.5, 3.0)
EDGE_FLOORS = (1e-3, 0.5)
EDGE_VARIANTS = ("var0", "fireflies", "dirty_alpha", "far_origin", "albedo0", "n1", "n40")


def edge_sweeps():
    """{sweep: [case]}: the edge table, one entry per id of test_svgf_edges_vs_restatement."""
    sweeps = {f"shape_{w}x{h}": [case(w, h, it) for it in EDGE_SHAPE_ITERATIONS] for w, h in EDGE_SHAPES}
    sweeps["min_history"] = [case(*EDGE_BASE, min_history=m) for m in EDGE_MIN_HISTORY]
    sweeps["sigmas"] = [case(*EDGE_BASE, **{name: DEFAULTS[name] * f}) for name in SIGMAS for f in EDGE_SIGMA_FACTORS]
    sweeps["albedo_floor"] = [case(*EDGE_BASE, albedo_floor=f) for f in EDGE_FLOORS]
    sweeps["variants"] = [case(*EDGE_BASE, variant=v) for v in EDGE_VARIANTS]
    sweeps["wide"] = [case(*EDGE_WIDE, 4, guides=())]
    return sweeps


def edge_table():
    return [c for cases in edge_sweeps().values() for c in cases]


def f32_f64_gap(table):
    """The largest gap between the restatement's f32 and f64 runs over a case table: (colour, variance)."""
    worst = [0.0, 0.0]
    for c in table:
        color, moment2, g = case_inputs(c)
        a = svgf(color, moment2, g, np.float32, **c["params"])
        b = svgf(color, moment2, g, np.float64, **c["params"])
        worst = [max(worst[i], rel_gap(a[i], b[i])) for i in range(2)]
    return tuple(worst)


if __name__ == "__main__":
    gc, gv = f32_f64_gap(default_table())
    print(f"largest f32 - f64 gap over the main table ({len(default_table())} filter calls): "
          f"colour {gc:.3g}, variance {gv:.3g}")
    for name, cases in edge_sweeps().items():
        gc, gv = f32_f64_gap(cases)
        print(f"  edge {name}: colour {gc:.3g}, variance {gv:.3g}")
    gc, gv = f32_f64_gap(edge_table())
    print(f"largest f32 - f64 gap over the edge table ({len(edge_table())} filter calls): "
          f"colour {gc:.3g}, variance {gv:.3g}")
