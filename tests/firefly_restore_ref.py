"""NumPy restatement of lrt_firefly_restore_* (include/lrt.h, "firefly restore"): plain f32, every
operation rounded once, whole-frame shifted planes tap by tap in the defined order. The library's
output is held to it bit for bit (tests/test_gpu_firefly_restore.py);
tests/test_firefly_restore_cpu.py holds the restatement itself to hand-written expectations on the
designed cases below and to the conservation identity on tame fields."""
import numpy as np

import firefly_ref as FR

F = np.float32
DEFAULTS = dict(radius=2)
MAX_RADIUS = 4
CAP = F(2.0 ** 100)
bits = FR.bits


def tent(r, d):
    return r + 1 - abs(d)


def step(color, excess, ids=None, **params):
    """One call on color, excess [h, w, 4] f32 and ids [h, w] int32 (or None). Returns {"out": [h, w, 4],
    "acc": [h, w, 3], "W": int64 [h, w], "e": the live sources' excess [h, w, 3]}."""
    p = dict(DEFAULTS, **params)
    r = int(p["radius"])
    color = np.ascontiguousarray(color, np.float32)
    excess = np.ascontiguousarray(excess, np.float32)
    h, w = color.shape[:2]
    idp = np.zeros((h, w), np.int32) if ids is None else np.asarray(ids, np.int32).reshape(h, w)
    # 1. source: a select; NaN fails the comparison
    with np.errstate(invalid="ignore"):
        live = (np.abs(excess[..., :3]) <= CAP).all(-1)
    e = np.where(live[..., None], excess[..., :3], F(0)).astype(np.float32)
    pad2 = lambda a, v: np.pad(a, r, constant_values=v)   # noqa: E731
    idpp, inside = pad2(idp, 0), pad2(np.ones((h, w), bool), False)
    window = [(dy, dx) for dy in range(-r, r + 1) for dx in range(-r, r + 1)]
    counts = {}
    for dy, dx in window:
        sl = (slice(r + dy, r + dy + h), slice(r + dx, r + dx + w))
        counts[(dy, dx)] = inside[sl] & (idpp[sl] == idp)
    # 2. normaliser
    W = np.zeros((h, w), np.int64)
    for dy, dx in window:
        W += counts[(dy, dx)] * (tent(r, dy) * tent(r, dx))
    n = (e / W.astype(np.float32)[..., None]).astype(np.float32)
    npad = np.pad(n, ((r, r), (r, r), (0, 0)))
    # 3. gather, dy then dx ascending
    acc = np.zeros((h, w, 3), np.float32)
    for dy, dx in window:
        term = (F(tent(r, dy) * tent(r, dx)) * npad[r + dy:r + dy + h, r + dx:r + dx + w]).astype(np.float32)
        acc = np.where(counts[(dy, dx)][..., None], (acc + term).astype(np.float32), acc)
    # 4. write
    out = color.copy()
    with np.errstate(all="ignore"):
        total = (color[..., :3] + acc).astype(np.float32)
    change = (acc != 0) & np.isfinite(color[..., :3])
    out[..., :3][change] = total[change]
    return {"out": out, "acc": acc, "W": W, "e": e}


# ---- generated fields: bits only
def wild(w, h, seed):
    """(color, excess, ids): firefly_ref.field through firefly_ref.step at its defaults, then NaN, +-Inf,
    0x1p100f, 0x1p101f, denormals, -0, negative and ordinary values replanted into the excess plane."""
    color0, ids = FR.field(w, h, seed)
    res = FR.step(color0, ids)
    color, excess = res["out"], res["excess"].copy()
    rng = np.random.default_rng(7000 + seed)
    k = max(1, w * h // 40)
    at = lambda: (rng.integers(0, h, k), rng.integers(0, w, k))   # noqa: E731
    for _ in range(3):
        y, x = at()
        excess[y, x, :3] = np.exp(rng.normal(2.0, 2.0, (k, 3))).astype(np.float32)
    y, x = at()
    excess[y, x, :3] = -excess[y, x, :3] - F(1.5)
    y, x = at()
    excess[y, x, :3] = [1e-40, 3e-42, 1e-45]
    y, x = at()
    excess[y, x, :3] = -0.0
    y, x = at()
    excess[y, x, :3] = CAP
    y, x = at()
    excess[y, x, rng.integers(0, 3, k)] = -CAP
    y, x = at()
    excess[y, x, rng.integers(0, 3, k)] = F(2.0 ** 101)
    y, x = at()
    excess[y, x, rng.integers(0, 3, k)] = np.nan
    y, x = at()
    excess[y, x, rng.integers(0, 3, k)] = np.inf
    y, x = at()
    excess[y, x, rng.integers(0, 3, k)] = -np.inf
    y, x = at()
    excess[y, x, 3] = np.nan                                   # the fourth word is never read
    return color, excess, ids


def case_list():
    """(label, w, h, seed, with_id, radius): firefly_ref.SIZES at every radius, with and without ids."""
    return [(f"{w}x{h} r{r} {'id' if with_id else 'noid'}", w, h, 10 * k + r, with_id, r)
            for k, (w, h) in enumerate(FR.SIZES) for r in range(1, MAX_RADIUS + 1) for with_id in (True, False)]


# ---- tame fields: conservation
TAME_SIZES = [(5, 5), (33, 9), (65, 17), (64, 36)]


def tame(w, h, seed, with_id):
    """(input, clamped, excess, ids or None, pixels clamped): exp(N(-1, 1)) noise with w h / 40 (at least two) spikes
    of (1e4, 8e3, 6e3) and a 3 x 2 grid of ids, through firefly_ref.step at its defaults."""
    rng = np.random.default_rng(9000 + seed)
    c = np.exp(rng.normal(-1.0, 1.0, (h, w, 4))).astype(np.float32)
    k = max(2, w * h // 40)
    c[rng.integers(0, h, k), rng.integers(0, w, k), :3] = [1e4, 8e3, 6e3]
    ys, xs = np.mgrid[0:h, 0:w]
    ids = ((xs * 3 // w) + 3 * (ys * 2 // h)).astype(np.int32) if with_id else None
    res = FR.step(c, ids)
    return c, res["out"], res["excess"], ids, int(res["info"][0])


def conservation(color, excess, out, radius, mask=None):
    """(|sum out - (sum color + sum excess)|, bound) over rgb in f64: the bound is first-order, one
    rounding of 2^-24 per division, product, accumulation and final add: (2R + 1)^2 + 3 of them."""
    sel = (lambda a: a[..., :3].astype(np.float64)) if mask is None else (lambda a: a[mask][:, :3].astype(np.float64))
    c, e, o = sel(color), sel(excess), sel(out)
    d = (2 * radius + 1) ** 2
    return abs(o.sum() - (c.sum() + e.sum())), (d + 3) * 2.0 ** -24 * (np.abs(c).sum() + np.abs(e).sum())


# ---- designed cases: hand-written expectations, exact in f32
DESIGNED_CASES = ("interior_spike", "corner_spike", "alone_on_its_id", "id_border", "dead_sources",
                  "non_finite_destination", "zero_excess")
GREY = (0.5, 0.25, 0.125)


def designed_inputs(case):
    """(color, excess, ids, params, acc): acc = {(y, x): the three sums that must reach the pixel}; every
    channel not named (or named with 0) must come out with the bits it went in with, and every alpha."""
    h, w = 7, 9
    rng = np.random.default_rng(11)
    c = np.empty((h, w, 4), np.float32)
    c[..., :3] = GREY
    c[..., 3] = rng.normal(size=(h, w))
    x = np.zeros((h, w, 4), np.float32)
    ids, params, acc = None, dict(radius=1), {}
    block = lambda cy, cx, rows, n: {(cy + dy, cx + dx): [F(wt) * F(v) for v in n]   # noqa: E731
                                     for dy, row in rows.items() for dx, wt in row.items()}
    full = {-1: {-1: 1, 0: 2, 1: 1}, 0: {-1: 2, 0: 4, 1: 2}, 1: {-1: 1, 0: 2, 1: 1}}
    if case == "interior_spike":
        x[3, 4, :3] = [16, 32, 8]                       # W = 16, n = (1, 2, 0.5)
        acc = block(3, 4, full, (1, 2, 0.5))
    elif case == "corner_spike":
        x[0, 0, :3] = [9, 18, 27]                       # W = 4 + 2 + 2 + 1 = 9, n = (1, 2, 3)
        acc = block(0, 0, {0: {0: 4, 1: 2}, 1: {0: 2, 1: 1}}, (1, 2, 3))
    elif case == "alone_on_its_id":
        params = dict(radius=2)
        ids = np.zeros((h, w), np.int32)
        ids[3, 4] = 5
        x[3, 4, :3] = [9, 18, 4.5]                      # W = 9, one tap of weight 9: its own excess back
        acc = {(3, 4): [F(9), F(18), F(4.5)]}
    elif case == "id_border":
        ids = np.zeros((h, w), np.int32)
        ids[:, 4:] = -1
        x[3, 3, :3] = [12, 24, 6]                       # dx = -1, 0 only: W = (1 + 2)(1 + 2 + 1) = 12
        acc = block(3, 3, {dy: {dx: full[dy][dx] for dx in (-1, 0)} for dy in (-1, 0, 1)}, (1, 2, 0.5))
    elif case == "dead_sources":
        x[1, 1, :3] = [np.nan, 16, 16]
        x[1, 4, :3] = [16, np.inf, 16]
        x[1, 7, :3] = [16, 16, 2.0 ** 101]
        x[5, 4, :3] = [-np.inf, 0, 0]
        x[5, 1, :3] = [2.0 ** 100, 16, 32]              # live: n = (2^96, 1, 2)
        acc = block(5, 1, full, (2.0 ** 96, 1, 2))
    elif case == "non_finite_destination":
        x[3, 4, :3] = [16, 32, 8]
        c[3, 5, :3] = [np.nan, 0.25, np.inf]
        c[2, 4, :3] = [-np.inf, 0.25, 0.125]
        c[2, 4, 1:2].view(np.uint32)[...] = 0x7FC12345  # a NaN with a payload
        acc = block(3, 4, full, (1, 2, 0.5))
    elif case == "zero_excess":
        params = dict(radius=2)
        c[1:4, 2:6, :3] = -0.0
        x[2, 3, :3] = -0.0
        x[..., 3] = 7.0                                 # never read
    else:
        raise KeyError(case)
    return c, x, ids, params, acc


def check_designed(case, color, out, acc):
    """The hand-written expectations on one output frame."""
    want = color.copy()
    for (y, x), v in acc.items():
        for ch in range(3):
            if v[ch] != 0 and np.isfinite(color[y, x, ch]):
                want[y, x, ch] = F(color[y, x, ch]) + F(v[ch])
    bad = bits(out) != bits(want)
    assert not bad.any(), (case, np.argwhere(bad)[:4].tolist())
