"""NumPy restatement of the feature-guided a-trous denoiser (include/lrt.h, lrt_denoise_*), the
inputs and cases the denoiser tests share, and the image metrics they use. A helper module, not
a conftest: imported by tests/test_denoise_cpu.py and tests/test_gpu_denoise.py.

    c_{k+1}(p) = sum_q w(p,q) c_k(q) / sum_q w(p,q),  q = p + 2^k (i, j),  i, j in -2..2 (inside the image)
    w(p,q) = h[i] h[j] exp(-E(p,q)),  h = [1/16, 1/4, 3/8, 1/4, 1/16]
    E = |c_k(p) - c_k(q)|^2 / ((sigma_color 2^-k)^2 |std(p)|^2 + 1e-6)   if color_std is given
      + |n(p) - n(q)|^2 / sigma_normal^2 + |x(p) - x(q)|^2 / sigma_pos^2 + |a(p) - a(q)|^2 / sigma_albedo^2
        (each only if its guide is given)

`python tests/denoise_ref.py` prints the largest gap between the f32 and the f64 run over each of the
GPU tests' two case tables (the constants F32_F64_GAP and F32_F64_GAP_EDGE of
tests/test_gpu_denoise.py).
"""
import numpy as np

DEFAULTS = dict(iterations=5, sigma_color=2.0, sigma_normal=0.3, sigma_pos=0.5, sigma_albedo=0.2)
H5 = (1 / 16, 1 / 4, 3 / 8, 1 / 4, 1 / 16)
GUIDE_SIGMA = (("normal", "sigma_normal"), ("world_pos", "sigma_pos"), ("albedo", "sigma_albedo"))


def atrous(color, guides=None, dtype=np.float64, **params):
    """The filter on color[h, w, >=3] with guides {name: [h, w, >=3]} (lrt_features names; a missing
    or None guide drops its term). Arithmetic in `dtype`. Returns rgb [h, w, 3] in `dtype`."""
    p = dict(DEFAULTS, **params)
    T = dtype
    guides = {k: np.asarray(v)[..., :3].astype(T) for k, v in (guides or {}).items() if v is not None}
    c = np.asarray(color)[..., :3].astype(T)
    h, w = c.shape[:2]
    std2 = (guides["color_std"] ** 2).sum(-1) if "color_std" in guides else None
    for k in range(int(p["iterations"])):
        s = 1 << k
        num = np.zeros_like(c)
        den = np.zeros((h, w), T)
        inv_c = None
        if std2 is not None:
            sc = T(p["sigma_color"]) / T(s)
            inv_c = T(1) / (sc * sc * std2 + T(1e-6))
        for j in range(-2, 3):
            for i in range(-2, 3):
                dy, dx = j * s, i * s
                ys = slice(max(0, -dy), h - max(0, dy))      # the pixels p whose tap p + (dx, dy) is inside
                xs = slice(max(0, -dx), w - max(0, dx))
                if ys.start >= ys.stop or xs.start >= xs.stop:
                    continue
                yq = slice(ys.start + dy, ys.stop + dy)
                xq = slice(xs.start + dx, xs.stop + dx)
                e = np.zeros((ys.stop - ys.start, xs.stop - xs.start), T)
                if inv_c is not None:
                    e += ((c[ys, xs] - c[yq, xq]) ** 2).sum(-1) * inv_c[ys, xs]
                for name, sig in GUIDE_SIGMA:
                    if name in guides:
                        g = guides[name]
                        e += ((g[ys, xs] - g[yq, xq]) ** 2).sum(-1) / (T(p[sig]) * T(p[sig]))
                wq = T(H5[i + 2]) * T(H5[j + 2]) * np.exp(-e)
                num[ys, xs] += wq[..., None] * c[yq, xq]
                den[ys, xs] += wq
        c = num / den[..., None]
    return c


def mse(a, gt):
    return float(((np.asarray(a, np.float64)[..., :3] - np.asarray(gt, np.float64)[..., :3]) ** 2).mean())


def rel_mse(a, gt):
    a, gt = np.asarray(a, np.float64)[..., :3], np.asarray(gt, np.float64)[..., :3]
    return float(((a - gt) ** 2 / (gt ** 2 + 0.01)).mean())


# ---- the synthetic cases of tests/test_gpu_denoise.py::test_denoise_vs_restatement
SHAPES = ((1, 1), (5, 3), (19, 13), (67, 45), (257, 9), (160, 90))   # w x h
ITERATIONS = (1, 2, 5)
GUIDE_SETS = {
    "all": ("normal", "world_pos", "albedo", "color_std"),
    "none": (),
    "normal": ("normal",),
    "no_std": ("normal", "world_pos", "albedo"),
}
PALETTE = np.array([[0.8, 0.8, 0.8], [0.8, 0.4, 0.4], [0.4, 0.8, 0.4], [0.7, 0.7, 0.9]], np.float32)


VARIANTS = ("std_extremes", "fireflies", "dirty_alpha", "far_origin")
FAR_ORIGIN = (1000.0, 0.0, 1000.0)


def synthetic_inputs(w, h, seed=0, variant=None):
    """(color, guides): float32 [h, w, 4] buffers. colour: a smooth field plus noise in [0, 4];
    std in [0.05, 1]; normals: three plane regions plus jitter; position: a ramp plus jitter;
    albedo: a four-colour palette in blocks. The jitters are of the size of the default sigmas,
    so that a fair share of the weights is neither 0 nor 1.
    variant (one of VARIANTS) changes the default frame afterwards, from a generator of its own:
      std_extremes  color_std rgb exactly 0 on a third of the pixels, exactly 1e3 (the temporal
                    stage's short_std) on another third
      fireflies     up to five pixels at 1e4 and one at 65504
      dirty_alpha   NaN, +Inf and 1e30 in the alpha of every guide buffer
      far_origin    world_pos rgb shifted by FAR_ORIGIN, in f32"""
    if variant is not None:
        if variant not in VARIANTS:
            raise ValueError(f"unknown variant {variant!r}")
        color, guides = synthetic_inputs(w, h, seed)
        rng = np.random.default_rng([VARIANTS.index(variant), w, h, seed])
        if variant == "std_extremes":
            third = rng.integers(0, 3, (h, w))
            guides["color_std"][..., :3][third == 0] = 0.0
            guides["color_std"][..., :3][third == 1] = 1e3
        elif variant == "fireflies":
            at = rng.choice(w * h, min(6, w * h), replace=False)
            rgb = color.reshape(-1, 4)[:, :3]
            rgb[at] = 1e4
            rgb[at[-1]] = 65504.0
        elif variant == "dirty_alpha":
            junk = np.float32([np.nan, np.inf, 1e30])
            for g in guides.values():
                g[..., 3] = junk[rng.integers(0, 3, (h, w))]
        else:
            guides["world_pos"][..., :3] += np.float32(FAR_ORIGIN)
        return color, guides
    rng = np.random.default_rng(1000 * w + h + seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float32)
    u, v = x / max(w - 1, 1), y / max(h - 1, 1)
    smooth = 2.0 + 1.5 * np.sin(6.0 * u + 2.0 * v)[..., None] * np.array([1.0, 0.7, 0.4], np.float32)
    color = np.empty((h, w, 4), np.float32)
    color[..., :3] = np.clip(smooth + rng.normal(0, 0.5, (h, w, 3)), 0, 4)
    color[..., 3] = rng.random((h, w))
    std = np.empty((h, w, 4), np.float32)
    std[..., :3] = rng.uniform(0.05, 1.0, (h, w, 3))
    std[..., 3] = 0
    planes = np.array([[0, 1, 0], [1, 0, 0], [0, 0, 1]], np.float32)
    region = (u * 3).astype(np.int64).clip(0, 2)
    region[v > 0.7] = 0
    n = planes[region] + rng.normal(0, 0.08, (h, w, 3))
    n /= np.linalg.norm(n, axis=-1, keepdims=True)
    normal = np.zeros((h, w, 4), np.float32)
    normal[..., :3] = n
    pos = np.zeros((h, w, 4), np.float32)
    pos[..., 0] = 4 * u - 2
    pos[..., 1] = 2 * v
    pos[..., 2] = -1 - u - v
    pos[..., :3] += rng.normal(0, 0.1, (h, w, 3))
    albedo = np.zeros((h, w, 4), np.float32)
    albedo[..., :3] = PALETTE[((x // 7 + y // 5) % 4).astype(np.int64)]
    guides = {"normal": normal, "world_pos": pos, "albedo": albedo, "color_std": std}
    return color, {k: np.ascontiguousarray(g, np.float32) for k, g in guides.items()}


def rel_gap(a, ref):
    """max |a - ref| / max(1, |ref|) -- the quantity the GPU test bounds."""
    ref = np.asarray(ref, np.float64)
    return float((np.abs(np.asarray(a, np.float64) - ref) / np.maximum(1.0, np.abs(ref))).max())


def case(w, h, iterations=5, guides=None, variant=None, **params):
    """One filter call of a case table: synthetic_inputs(w, h, variant=variant), the guides named
    (default: all four), atrous' parameters."""
    return dict(w=w, h=h, variant=variant, guides=tuple(GUIDE_SETS["all"] if guides is None else guides),
                params=dict(params, iterations=iterations))


def case_label(c):
    extra = "".join(f" {k}={v:g}" for k, v in c["params"].items() if k != "iterations")
    return (f"{c['w']}x{c['h']} iterations={c['params']['iterations']} guides={'+'.join(c['guides']) or 'none'}"
            f"{extra}{' ' + c['variant'] if c['variant'] else ''}")


def case_inputs(c):
    """(color, the case's guides) of one case."""
    color, guides = synthetic_inputs(c["w"], c["h"], variant=c["variant"])
    return color, {k: guides[k] for k in c["guides"]}


def default_table():
    """The cases of test_denoise_vs_restatement: SHAPES x ITERATIONS x GUIDE_SETS."""
    return [case(w, h, it, names) for w, h in SHAPES for it in ITERATIONS for names in GUIDE_SETS.values()]


# ---- the edge cases of tests/test_gpu_denoise.py::test_denoise_edges_vs_restatement: a base case
# (67x45, 5 iterations, all guides, the default sigmas) and sweeps of one axis each from it, not
# their product. At s = 16 a row group is 64 rows and a tile 64 columns: the shapes sit on and
# beside those edges (one group exactly, a second group with one live phase, three groups, tall and
# narrow) and run at the iteration counts that end on s = 4, 8 and 16, the three ping-pong parities.
EDGE_BASE = (67, 45)
EDGE_SHAPES = ((1, 130), (3, 70), (63, 5), (64, 4), (65, 8), (128, 3), (129, 65), (70, 129), (64, 64))
EDGE_SHAPE_ITERATIONS = (3, 4, 5)
# One frame of more workgroups than the device holds at once (256 x 16 of them at s = 8; about a
# thousand are resident), the second row group's 2048 launches after the first's rows: a pass that
# read the buffer it writes would pass every small frame, whose workgroups all stage before any
# stores, and shows here. Unguided, so that the restatement of its 655 K pixels takes seconds.
EDGE_WIDE = (16384, 40)
EDGE_ITERATIONS = (1, 2, 3, 4, 5)
EDGE_ITERATION_SHAPES = (EDGE_BASE, (129, 65))
_ALL = GUIDE_SETS["all"]
EDGE_GUIDE_SETS = {**{g: (g,) for g in _ALL}, **{"no_" + g: tuple(n for n in _ALL if n != g) for g in _ALL}}
SIGMAS = ("sigma_color", "sigma_normal", "sigma_pos", "sigma_albedo")
EDGE_SIGMA_FACTORS = (0.5, 3.0)
EDGE_SIGMAS_ALL = dict(sigma_color=0.7, sigma_normal=2.5, sigma_pos=0.4, sigma_albedo=1.6)   # factors, all differ


def edge_sweeps():
    """{sweep: [case]}: the edge table, one entry per id of test_denoise_edges_vs_restatement."""
    sweeps = {f"shape_{w}x{h}": [case(w, h, it) for it in EDGE_SHAPE_ITERATIONS] for w, h in EDGE_SHAPES}
    sweeps["iterations"] = [case(w, h, it) for w, h in EDGE_ITERATION_SHAPES for it in EDGE_ITERATIONS]
    sweeps["guides"] = [case(*EDGE_BASE, guides=names) for names in EDGE_GUIDE_SETS.values()]
    sweeps["sigmas"] = [case(*EDGE_BASE, **{name: DEFAULTS[name] * f}) for name in SIGMAS for f in EDGE_SIGMA_FACTORS]
    sweeps["sigmas"].append(case(*EDGE_BASE, **{name: DEFAULTS[name] * f for name, f in EDGE_SIGMAS_ALL.items()}))
    sweeps["variants"] = [case(*EDGE_BASE, variant=v) for v in VARIANTS]
    sweeps["wide"] = [case(*EDGE_WIDE, guides=())]
    return sweeps


def edge_table():
    return [c for cases in edge_sweeps().values() for c in cases]


def f32_f64_gap(table=None):
    """The largest gap between the restatement's f32 and f64 runs over a case table (default: the
    one of test_denoise_vs_restatement)."""
    worst = 0.0
    for c in default_table() if table is None else table:
        color, g = case_inputs(c)
        worst = max(worst, rel_gap(atrous(color, g, np.float32, **c["params"]),
                                   atrous(color, g, np.float64, **c["params"])))
    return worst


if __name__ == "__main__":
    print(f"largest f32 - f64 gap over the GPU test's cases: {f32_f64_gap():.3g}")
    print(f"largest f32 - f64 gap over the edge table ({len(edge_table())} filter calls): "
          f"{f32_f64_gap(edge_table()):.3g}")
    for name, cases in edge_sweeps().items():
        print(f"  {name}: {f32_f64_gap(cases):.3g}")
