"""NumPy restatement of lrt_sample_budget_* (include/lrt.h): the weight in f32, one operation at a
time in the order the header gives, then the passes in Python / NumPy integers. The library's counts
and info are pinned to it exactly."""
import numpy as np

COUNT_MAX = 4096
SB_STD = 1
DEFAULTS = dict(passes=2, luma_floor=0.01, weight_max=256.0, flags=0)


def luma(rgb):
    """(0.2126f r + 0.7152f g) + 0.0722f b, every product and sum rounded to f32."""
    f = np.float32
    c = np.asarray(rgb, np.float32)
    with np.errstate(all="ignore"):
        return (f(0.2126) * c[..., 0] + f(0.7152) * c[..., 1]) + f(0.0722) * c[..., 2]


def weights(variance, color=None, flags=0, luma_floor=0.01, weight_max=256.0):
    """q per pixel (uint64 array holding uint32 values), step 1."""
    f = np.float32
    v = np.asarray(variance, np.float32)[..., :3]
    with np.errstate(all="ignore"):
        if flags & SB_STD:
            v = v * v
        w = np.sqrt(luma(v))                       # correctly rounded in f32
        if color is not None:
            y = luma(np.asarray(color, np.float32)[..., :3])
            w = w / (np.fmax(y, f(0)) + f(luma_floor))   # fmaxf: a NaN luminance counts as 0
        ok = np.isfinite(w) & (w > 0)
        scaled = np.minimum(np.where(ok, w, f(0)), f(weight_max)) * f(65536.0)
    assert scaled.dtype == np.float32
    return np.where(ok, scaled.astype(np.uint64), np.uint64(0)).astype(np.uint64)


def allocate(q, min_count, max_count, budget, passes=2):
    """(counts int32 in q's shape, info): steps 2 to 4 on the weights q."""
    qi = [int(x) for x in np.asarray(q).ravel()]
    counts = [int(min_count)] * len(qi)
    q1 = None
    for _ in range(int(passes)):
        U = [p for p, c in enumerate(counts) if c < max_count]
        E = int(budget) - sum(counts)
        Q = sum(qi[p] for p in U)
        if q1 is None:
            q1 = Q
        if E <= 0 or not U:
            continue
        for p in U:
            add = E // len(U) if Q == 0 else (E * qi[p]) // Q
            counts[p] = min(int(max_count), counts[p] + add)
    total = sum(counts)
    assert total <= int(budget)
    return np.array(counts, np.int32).reshape(np.asarray(q).shape), (total, q1)


def budget(variance, min_count, max_count, total, color=None, passes=2, luma_floor=0.01, weight_max=256.0, flags=0):
    """The whole call: (counts [height, width] int32, (sum of the counts, pass 1's Q))."""
    q = weights(variance, color, flags, luma_floor, weight_max)
    return allocate(q, min_count, max_count, total, passes)


def random_field(w, h, seed, nasty=True):
    """A variance-like RGBA field: log-uniform magnitudes over twelve decades, alphas of garbage, and
    (nasty) NaN, +-Inf, negatives, zeros and denormals sprinkled in."""
    rng = np.random.default_rng(seed)
    v = np.exp(rng.uniform(np.log(1e-9), np.log(1e3), (h, w, 4))).astype(np.float32)
    v[..., 3] = rng.choice(np.array([np.nan, -1.0, 1e30, 0.0], np.float32), (h, w))
    if nasty:
        pick = rng.random((h, w, 3))
        for lo, hi, val in ((0.00, 0.02, np.nan), (0.02, 0.04, np.inf), (0.04, 0.06, -np.inf), (0.06, 0.08, -0.5),
                            (0.08, 0.12, 0.0), (0.12, 0.13, 1e-41), (0.13, 0.14, 3e38)):
            v[..., :3][(pick >= lo) & (pick < hi)] = val
    return v


def random_color(w, h, seed, nasty=True):
    rng = np.random.default_rng(seed + 1000)
    c = rng.uniform(0.0, 2.0, (h, w, 4)).astype(np.float32)
    if nasty:
        pick = rng.random((h, w))
        c[pick < 0.02, 1] = np.nan
        c[(pick >= 0.02) & (pick < 0.04)] = -3.0
        c[(pick >= 0.04) & (pick < 0.06), 0] = np.inf
        c[(pick >= 0.06) & (pick < 0.10), :3] = 0.0
    return c
