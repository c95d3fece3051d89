"""NumPy restatement of lrt_tonemap_* (include/lrt.h): the luminance histogram from the bits of Y
(f32) or from the bins' definition (f64), the percentile-window exposure with its state update, the
tone curves and the present quantiser; the fragile-pixel accounting the histogram checks use; the
input frames and case tables the CPU and GPU tests share.

    python tests/tonemap_ref.py

prints the restatement's own f32 - f64 gaps per table (the tolerances of tests/test_gpu_tonemap.py
are 16 x these)."""
import itertools

import numpy as np

BINS, WORDS, UNDER, OVER = 256, 258, 256, 257
LINEAR, REINHARD, ACES = 0, 1, 2
OPS = (LINEAR, REINHARD, ACES)
TM_MAX = 65504.0
DEFAULTS = dict(op=ACES, auto_exposure=1, key=0.18, p_low=0.1, p_high=0.9, ev_bias=0.0, ev_min=-8.0, ev_max=8.0,
                adapt=1.0, white=4.0)
NO_HISTORY = (0.0, 0.0, 0.0, 0.0)
FRAGILE_ULPS = 4
_W = (np.float32(0.2126), np.float32(0.7152), np.float32(0.0722))   # the f32 constants of the kernel


def _params(params):
    unknown = set(params) - set(DEFAULTS)
    assert not unknown, unknown
    p = dict(DEFAULTS, **params)
    return {k: (int(v) if k in ("op", "auto_exposure") else np.float32(v)) for k, v in p.items()}


def luminance(color, dtype):
    """Y = 0.2126 R + 0.7152 G + 0.0722 B of the rgb as read, left to right, in dtype."""
    c = np.asarray(color)[..., :3].astype(dtype)
    with np.errstate(all="ignore"):
        return (dtype(_W[0]) * c[..., 0] + dtype(_W[1]) * c[..., 1]) + dtype(_W[2]) * c[..., 2]


def bins_from_bits(y32):
    """The bin of each f32 luminance from its bits (what the kernel does)."""
    y32 = np.ascontiguousarray(y32, np.float32)
    bits = y32.view(np.uint32).astype(np.int64)
    out = np.full(y32.shape, UNDER, np.int64)
    inside = (bits >= 0x37800000) & (bits < 0x47800000)
    out[inside] = (bits[inside] >> 20) - 888
    out[(bits >= 0x47800000) & (bits <= 0x7F800000)] = OVER
    return out


def bins_from_definition(y):
    """The bin of each luminance from the definition: [2^-16, 2^16) in octaves of eight equal parts;
    at and above 2^16 (+Inf included) `over`; everything else `under`."""
    y = np.asarray(y, np.float64)
    out = np.full(y.shape, UNDER, np.int64)
    with np.errstate(invalid="ignore"):
        inside = (y >= 2.0 ** -16) & (y < 2.0 ** 16)
        out[y >= 2.0 ** 16] = OVER
    mant, exp = np.frexp(np.where(inside, y, 1.0))          # y = mant 2^exp, mant in [0.5, 1)
    b = 8 * (exp - 1 + 16) + np.floor((2.0 * mant - 1.0) * 8.0).astype(np.int64)
    out[inside] = b[inside]
    return out


def histogram(color, dtype):
    """The WORDS counts (256 bins, under, over) of a frame: f32 from the bits of the f32 luminance,
    f64 from the definition on the f64 luminance."""
    y = luminance(color, dtype)
    b = bins_from_bits(y) if dtype == np.float32 else bins_from_definition(y)
    return np.bincount(b.ravel(), minlength=WORDS).astype(np.int64)


def fragile(color):
    """(mask, below, above): the pixels whose f64 luminance lies within FRAGILE_ULPS f32 ulps of a bin
    edge inside [2^-16, 2^16] (both ends included), and the words on either side of that edge."""
    y = luminance(color, np.float64)
    with np.errstate(invalid="ignore"):
        cand = np.isfinite(y) & (y >= 2.0 ** -17) & (y < 2.0 ** 17)
    mant, exp = np.frexp(np.where(cand, y, 1.0))
    q = (2.0 * mant - 1.0) * 8.0                            # position within the octave, in bins
    k = np.rint(q)
    edge = 8 * (exp - 1 + 16) + k.astype(np.int64)          # the edge between bins edge - 1 and edge
    # an f32 ulp at y is 2^(e - 23) and a bin is 2^(e - 3) wide: 4 ulp = 4 * 2^-20 bins
    near = np.abs(q - k) <= FRAGILE_ULPS * 2.0 ** -20
    mask = cand & near & (edge >= 0) & (edge <= BINS)
    below = np.where(edge == 0, UNDER, edge - 1)
    above = np.where(edge == BINS, OVER, edge)
    return mask, below, above


def histogram_bounds(color):
    """(lower, slack): the f64 histogram of the non-fragile pixels, and per word the number of fragile
    pixels beside it: lower[b] <= got[b] <= lower[b] + slack[b] for any correct f32 evaluation."""
    y = luminance(color, np.float64)
    mask, below, above = fragile(color)
    b = bins_from_definition(y)
    lower = np.bincount(b[~mask].ravel(), minlength=WORDS).astype(np.int64)
    slack = (np.bincount(below[mask].ravel(), minlength=WORDS) +
             np.bincount(above[mask].ravel(), minlength=WORDS)).astype(np.int64)
    return lower, slack


def bin_values(dtype):
    b = np.arange(BINS)
    return ((b >> 3) - 16).astype(dtype) + np.log2(dtype(1) + ((b & 7).astype(dtype) + dtype(0.5)) / dtype(8))


def exposure(hist, prev, npix, dtype, **params):
    """The state (log2_exposure, log2_luminance, counted, frames) after metering a frame with the
    counts `hist` over the state `prev`, every step in dtype."""
    p = _params(params)
    f = lambda name: dtype(p[name])   # noqa: E731 - the descriptor's f32 values, promoted
    prev = [dtype(np.float32(v)) for v in prev]
    h = np.asarray(hist[:BINS]).astype(dtype)
    N = dtype(np.asarray(hist[:BINS]).sum())
    has = prev[3] >= 1
    frames = dtype(np.float32(prev[3]) + np.float32(1))
    if N == 0:
        le = prev[0] if has else min(max(f("ev_bias"), f("ev_min")), f("ev_max"))
        return np.array([le, prev[1], 0.0, frames], dtype)
    c = np.cumsum(h, dtype=dtype) - h
    lo, hi = f("p_low") * N, f("p_high") * N
    m = np.maximum(dtype(0), np.minimum(c + h, hi) - np.maximum(c, lo))
    mean = (m * bin_values(dtype)).sum(dtype=dtype) / m.sum(dtype=dtype)
    target = min(max(np.log2(f("key")) - mean + f("ev_bias"), f("ev_min")), f("ev_max"))
    le = prev[0] + f("adapt") * (target - prev[0]) if has else target
    return np.array([le, mean, N / dtype(npix), frames], dtype)


def tonemap(color, log2_exposure, dtype, op=ACES, white=4.0):
    """t of every channel, [..., 3] in dtype, for the given log2 exposure (an f32 value)."""
    x = np.asarray(color)[..., :3].astype(dtype)
    e = np.exp2(dtype(np.float32(log2_exposure)))
    with np.errstate(all="ignore"):
        c = x * e
        c = np.where(c > 0, np.minimum(c, dtype(TM_MAX)), dtype(0))
        if op == LINEAR:
            return c
        if op == REINHARD:
            w2 = dtype(np.float32(white)) * dtype(np.float32(white))
            return c * (dtype(1) + c / w2) / (dtype(1) + c)
        t = c * (dtype(2.51) * c + dtype(0.03)) / (c * (dtype(2.43) * c + dtype(0.59)) + dtype(0.14))
        return np.clip(t, dtype(0), dtype(1))


def srgb8(t):
    """The present quantiser on f32 rgb [..., 3]: LinearToSRGB through the oracle's glibc-exact powf,
    * 255.9, b | g << 8 | r << 16."""
    import oracle

    def q(x):
        x = np.ascontiguousarray(np.where(x < 0, np.float32(0), x), np.float32)
        pw = oracle.orc_libm(3, x.ravel()).reshape(x.shape)
        y = (np.float32(1.055) * pw - np.float32(0.055)).astype(np.float32)
        y = np.where(y < 0, np.float32(0), y).astype(np.float32)
        u = (y * np.float32(255.9)).astype(np.float32)
        return np.minimum(u.astype(np.uint64), 255).astype(np.uint32)

    t = np.asarray(t, np.float32)
    return q(t[..., 2]) | (q(t[..., 1]) << 8) | (q(t[..., 0]) << 16)


def rel_gap(got, want):
    want = np.asarray(want, np.float64)
    return float(np.max(np.abs(np.asarray(got, np.float64) - want) / np.maximum(1.0, np.abs(want))))


# ---- inputs
SHAPES = ((1, 1), (5, 3), (63, 1), (64, 4), (65, 4), (257, 3), (67, 45), (129, 65), (4099, 1))
MAP_SHAPES = ((5, 3), (67, 45), (129, 65))
LARGE = (4096, 512)
KINDS = ("loguniform", "constant", "specials")
CONSTANT = (0.4, 0.6, 0.9)          # Y = 0.579: bin 121, a quarter of a bin from its edges
SPECIALS = (0.0, -0.0, -1.0, -1e30, 1e-40, -1e-42, np.nan, np.inf, -np.inf, 1e30, 65504.0)
SMALL_PIXELS, LARGE_FRACTION = 20000, 1e-4


def frame(w, h, kind="loguniform", seed=0, dirty_alpha=False, lo=-20.0, hi=20.0):
    """An f32 [h, w, 4] frame. loguniform: a magnitude 2^U(lo, hi) per pixel times a tint in [0.25, 1]
    per channel; constant: CONSTANT everywhere (every pixel in one bin); specials: loguniform with
    SPECIALS sprinkled over single channels. Alphas are 1, or NaN / Inf / garbage if dirty_alpha."""
    rng = np.random.default_rng([seed, w, h])
    if kind == "constant":
        rgb = np.broadcast_to(np.float32(CONSTANT), (h, w, 3)).copy()
    else:
        mag = np.exp2(rng.uniform(lo, hi, (h, w, 1)))
        rgb = (mag * rng.uniform(0.25, 1.0, (h, w, 3))).astype(np.float32)
        if kind == "specials":
            n = max(w * h // 3, min(w * h, len(SPECIALS)))
            where = rng.permutation(w * h)[:n]
            flat = rgb.reshape(-1, 3)
            with np.errstate(over="ignore"):
                flat[where, rng.integers(0, 3, n)] = np.float32(SPECIALS)[np.arange(n) % len(SPECIALS)]
        else:
            assert kind == "loguniform", kind
    out = np.ones((h, w, 4), np.float32)
    out[..., :3] = rgb
    if dirty_alpha:
        out[..., 3] = np.float32((np.nan, np.inf, -np.inf, -7.0, 3e38))[np.arange(w * h) % 5].reshape(h, w)
    return out


def histogram_table():
    """(w, h, kind, seed) of every frame the histogram tests meter."""
    return [(w, h, k, 0) for (w, h), k in itertools.product(SHAPES, KINDS)] + \
           [LARGE + ("loguniform", 0), LARGE + ("constant", 0)]


WINDOWS = ((0.0, 1.0), (0.1, 0.9), (0.5, 0.95), (0.49, 0.51), (0.0, 1e-3))
PREVS = (NO_HISTORY, (1.5, -2.0, 1.0, 3.0))


def state_table():
    """The parameter sets of the state tests (each is run without and with a previous state)."""
    t = [dict(p_low=a, p_high=b) for a, b in WINDOWS]
    t += [dict(key=0.18 * 0.5), dict(key=0.18 * 4)]
    t += [dict(ev_min=3.0, ev_max=8.0), dict(ev_min=-8.0, ev_max=-6.0)]      # the target clamps on either side
    t += [dict(adapt=0.25), dict(adapt=0.25, p_low=0.5, p_high=0.95, ev_bias=-1.5)]
    return t


STATE_FRAMES = ((67, 45, "loguniform", 0), (129, 65, "specials", 0), (5, 3, "loguniform", 0), (64, 4, "constant", 0))
EMPTY_KINDS = ("black", "nan")


def empty_frame(w, h, kind):
    """A frame no pixel of which is counted (N = 0)."""
    out = np.zeros((h, w, 4), np.float32)
    if kind == "nan":
        out[..., :3] = np.nan
    return out


def map_table():
    """(w, h, kind, op, ev_bias): the three operators x MAP_SHAPES x ev_bias, plus the specials frame."""
    t = [(w, h, "loguniform", op, ev) for (w, h), op, ev in itertools.product(MAP_SHAPES, OPS, (-3.0, 0.0, 2.0))]
    return t + [(67, 45, "specials", op, 0.0) for op in OPS]


MAP_RANGE = dict(lo=-12.0, hi=12.0)   # the map frames: dark to far above the curves' shoulders


def map_frame(w, h, kind):
    return frame(w, h, kind, seed=1, **MAP_RANGE)


def main():
    gap = 0.0
    n = 0
    for (w, h, kind, seed), params, prev in itertools.product(STATE_FRAMES, state_table(), PREVS):
        hist = histogram(frame(w, h, kind, seed), np.float32)
        a = exposure(hist, prev, w * h, np.float32, **params)
        b = exposure(hist, prev, w * h, np.float64, **params)
        gap = max(gap, rel_gap(a, b))
        n += 1
    print(f"largest f32 - f64 gap over the state table ({n} exposure updates): {gap:.3g}")
    gap, n = 0.0, 0
    for w, h, kind, op, ev in map_table():
        color = map_frame(w, h, kind)
        hist = histogram(color, np.float32)
        le = np.float32(exposure(hist, NO_HISTORY, w * h, np.float64, ev_bias=ev)[0])
        gap = max(gap, rel_gap(tonemap(color, le, np.float32, op), tonemap(color, le, np.float64, op)))
        n += 1
    print(f"largest f32 - f64 gap over the map table ({n} frames): {gap:.3g}")
    frag = {t: int(fragile(frame(*t))[0].sum()) for t in histogram_table()}
    print("fragile pixels: " + ", ".join(f"{w}x{h} {k}: {v}" for (w, h, k, s), v in frag.items() if v or w * h > SMALL_PIXELS))


if __name__ == "__main__":
    main()
