"""NumPy restatement of lrt_firefly_* (include/lrt.h, "firefly suppression"): plain f32, every
operation rounded once, and sort-based -- np.sort of the counting taps, descending, then element
rank - 1 -- so that it shares nothing with the kernel's insertion chain. The library's outputs are
held to it bit for bit (tests/test_gpu_firefly.py); tests/test_firefly_cpu.py holds the restatement
itself to hand-written expectations on the designed cases below."""
import numpy as np

F = np.float32
DEFAULTS = dict(radius=1, rank=2, min_taps=3, gain=2.0, floor=0.01)
MAX_RADIUS, MAX_RANK = 2, 4
SPIKE = 1e4
FLT_MAX = np.finfo(np.float32).max


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def luma(c):
    """Y of [..., >= 3] f32, lrt_sample_budget's expression."""
    c = np.asarray(c, np.float32)
    with np.errstate(all="ignore"):
        return (F(0.2126) * c[..., 0] + F(0.7152) * c[..., 1]) + F(0.0722) * c[..., 2]


def step(color, ids=None, **params):
    """One call on color [h, w, 4] f32 and ids [h, w] int32 (or None). Returns {"out": [h, w, 4],
    "excess": [h, w, 4], "class": int32 [h, w], "info": uint32 [2], "m": taps counted, "T": threshold}."""
    p = dict(DEFAULTS, **params)
    r, rank, min_taps = int(p["radius"]), int(p["rank"]), int(p["min_taps"])
    gain, floor = F(p["gain"]), F(p["floor"])
    color = np.ascontiguousarray(color, np.float32)
    h, w = color.shape[:2]
    Y = luma(color)
    fin = np.isfinite(Y)
    idp = np.zeros((h, w), np.int32) if ids is None else np.asarray(ids, np.int32).reshape(h, w)
    pad = lambda a, v: np.pad(a, r, constant_values=v)   # noqa: E731
    Yp, finp, idpp, inside = pad(Y, F(0)), pad(fin, False), pad(idp, 0), pad(np.ones((h, w), bool), False)
    taps, m = [], np.zeros((h, w), np.int64)
    for dy in range(-r, r + 1):
        for dx in range(-r, r + 1):
            if dy == 0 and dx == 0:
                continue
            sl = (slice(r + dy, r + dy + h), slice(r + dx, r + dx + w))
            counts = inside[sl] & (idpp[sl] == idp) & finp[sl]
            taps.append(np.where(counts, Yp[sl], F(-np.inf)).astype(np.float32))
            m += counts
    srt = np.sort(np.stack(taps, -1), axis=-1)[..., ::-1]
    Yk = srt[..., rank - 1]
    with np.errstate(all="ignore"):
        T = (gain * np.maximum(Yk, F(0)) + floor).astype(np.float32)
        s = (T / Y).astype(np.float32)
        cls = np.where(m < min_taps, 2, np.where(~fin, 3, np.where(Y > T, 1, 0))).astype(np.int32)
        out = color.copy()
        excess = np.zeros_like(color)
        c1, c3 = cls == 1, cls == 3
        out[c1, :3] = s[c1, None] * color[c1, :3]
        out[c3, :3] = T[c3, None]
        excess[c1, :3] = color[c1, :3] - out[c1, :3]
    info = np.array([c1.sum(), c3.sum()], np.uint32)
    return {"out": out, "excess": excess, "class": cls, "info": info, "m": m, "T": T}


# ---- generated fields
def field(w, h, seed):
    """(color [h, w, 4] f32, ids [h, w] int32) at a fixed seed: positive noise with NaN, +-Inf,
    negatives, +-0, denormals, FLT_MAX pixels (the luminance's sum is at the edge of overflow),
    opposite infinities in one pixel, plateaus of equal luminance, single 1e4 spikes, adjacent pairs,
    a 2 x 2 cluster, spikes on id borders and in the image's corners; ids in a few regions, among them
    the miss (-1) and the extreme int32 values."""
    rng = np.random.default_rng(1000 + seed)
    c = np.exp(rng.normal(-1.0, 1.0, (h, w, 4))).astype(np.float32)
    ys, xs = np.mgrid[0:h, 0:w]
    names = np.array([0, -1, 7, 2 ** 31 - 1, -2 ** 31, 3], np.int64)
    ids = names[(xs * 3 // w) + 3 * (ys * 2 // h)].astype(np.int32)
    if w >= 5 and h >= 5:
        ids[h // 2 - 1:h // 2 + 1, w // 2 - 1:w // 2 + 2] = 42          # a small surface of its own
    k = max(1, w * h // 40)
    at = lambda: (rng.integers(0, h, k), rng.integers(0, w, k))   # noqa: E731
    spike = np.array([SPIKE, 0.8 * SPIKE, 0.6 * SPIKE], np.float32)

    def put(y, x, v):
        if 0 <= y < h and 0 <= x < w:
            c[y, x, :3] = v

    y0, x0 = int(rng.integers(0, h)), int(rng.integers(0, w))
    for dy in range(3):
        for dx in range(3):
            put(y0 + dy, x0 + dx, [0.25, 0.5, 0.125])                    # a plateau
    y0, x0 = int(rng.integers(0, h)), int(rng.integers(0, w))
    for dy in range(2):
        for dx in range(4):
            put(y0 + dy, x0 + dx, 0.0)                                  # a plateau of zeros
    c[at() + (rng.integers(0, 3, k),)] = np.nan
    c[at() + (rng.integers(0, 3, k),)] = np.inf
    c[at() + (rng.integers(0, 3, k),)] = -np.inf
    y, x = at()
    c[y, x, :3] = -c[y, x, :3]
    y, x = at()
    c[y, x, :3] = 0.0
    y, x = at()
    c[y, x, :3] = -0.0
    y, x = at()
    c[y, x, :3] = [1e-40, 3e-42, 1e-45]
    y, x = at()
    c[y, x, :3] = FLT_MAX
    y, x = at()
    c[y, x, :3] = [np.inf, -np.inf, 1.0]
    for y, x in zip(*at()):
        put(y, x, spike)                                                # singles
    y, x = int(rng.integers(0, h)), int(rng.integers(0, w))
    put(y, x, spike), put(y, x + 1, spike * F(1.5))                     # an adjacent pair
    y, x = int(rng.integers(0, h)), int(rng.integers(0, w))
    for dy in range(2):
        for dx in range(2):
            put(y + dy, x + dx, spike * F(1 + dy + 2 * dx))             # a 2 x 2 cluster
    put(0, 0, spike), put(h - 1, w - 1, spike), put(0, w - 1, spike * F(3))   # corners
    for xb in (w // 3, 2 * w // 3):                                     # on id borders, either side
        put(int(rng.integers(0, h)), xb, spike)
        put(int(rng.integers(0, h)), xb - 1, spike)
    put(h // 2, int(rng.integers(0, w)), spike), put(h // 2 - 1, int(rng.integers(0, w)), spike)
    y, x = at()
    c[y, x, 3] = np.nan                                                 # alphas are bits
    return c, ids


SIZES = [(1, 1), (3, 2), (5, 5), (31, 7), (33, 9), (65, 17), (19, 13)]


def case_list():
    """(label, w, h, seed, with_id, params): every size at radius 1 and 2; at 19 x 13 each radius with
    rank 1..4, with and without ids; and support thresholds up to the whole window."""
    cases = []
    for k, (w, h) in enumerate(SIZES):
        for r in (1, 2):
            cases.append((f"{w}x{h} r{r}", w, h, k, True, dict(radius=r)))
    for r in (1, 2):
        for rank in (1, 2, 3, 4):
            for with_id in (True, False):
                cases.append((f"19x13 r{r} rank{rank} {'id' if with_id else 'noid'}", 19, 13, 10 * r + rank, with_id,
                              dict(radius=r, rank=rank, min_taps=max(rank, 3))))
    cases.append(("33x9 r1 full window", 33, 9, 31, True, dict(radius=1, min_taps=8, gain=1.0, floor=1e-3)))
    cases.append(("33x9 r2 full window", 33, 9, 32, False, dict(radius=2, rank=4, min_taps=24, gain=0.5, floor=5.0)))
    cases.append(("65x17 r2 rank3", 65, 17, 33, True, dict(radius=2, rank=3, min_taps=12, gain=4.0)))
    return cases


# ---- designed cases: hand-written expectations
DESIGNED_CASES = ("spike_rank1", "pair_rank1", "pair_rank2", "corner_unsupported", "nan_centre", "nan_neighbour",
                  "id_border", "id_border_without_ids", "yk_negative_zero", "yk_negative")
GREY = (0.5, 0.25, 0.125)
HOT = (1e4, 5e3, 2e3)


def _y(c):
    """Y of one rgb triple, scalar f32 arithmetic written out."""
    r, g, b = (F(v) for v in c)
    return F(F(F(0.2126) * r) + F(F(0.7152) * g)) + F(F(0.0722) * b)


def _threshold(yk, gain=2.0, floor=0.01):
    return F(F(F(gain) * max(F(yk), F(0))) + F(floor))


def _clamped(c, T):
    s = F(T / _y(c))
    return np.array([F(s * F(v)) for v in c], np.float32)


def designed_inputs(case):
    """(color, ids, params, expect): expect = {"class": int plane, "rgb": {(y, x): f32[3]}}; every pixel
    not in "rgb" must come out with the bits it went in with, and every alpha too."""
    h, w = 5, 7
    rng = np.random.default_rng(5)
    c = np.empty((h, w, 4), np.float32)
    c[..., :3] = GREY
    c[..., 3] = rng.normal(size=(h, w))
    ids, params = np.zeros((h, w), np.int32), {}
    cls = np.zeros((h, w), np.int32)
    rgb = {}
    Tg = _threshold(_y(GREY))
    if case == "spike_rank1":
        params = dict(rank=1)
        c[2, 3, :3] = HOT
        cls[2, 3] = 1
        rgb[(2, 3)] = _clamped(HOT, Tg)
    elif case in ("pair_rank1", "pair_rank2"):
        params = dict(rank=1 if case == "pair_rank1" else 2)
        c[2, 3, :3] = c[2, 4, :3] = HOT
        if case == "pair_rank2":
            cls[2, 3] = cls[2, 4] = 1
            rgb[(2, 3)] = rgb[(2, 4)] = _clamped(HOT, Tg)
    elif case == "corner_unsupported":
        params = dict(min_taps=4)                       # a corner has three neighbours
        c[0, 0, :3] = [np.nan, 1.0, np.inf]
        c[h - 1, w - 1, :3] = HOT
        c[0, w - 1, :3] = [-3.0, 0.0, 1e30]
        cls[0, 0] = cls[h - 1, w - 1] = cls[0, w - 1] = cls[h - 1, 0] = 2
        # (the edge pixels beside the NaN corner count four finite neighbours: supported)
    elif case == "nan_centre":
        c[2, 3, 1] = np.nan
        cls[2, 3] = 3
        rgb[(2, 3)] = np.array([Tg, Tg, Tg], np.float32)
    elif case == "nan_neighbour":
        params = dict(rank=1)
        c[2, 3, :3] = HOT
        c[2, 4, 0] = np.nan
        c[1, 3, :3] = np.inf
        cls[2, 3], cls[2, 4], cls[1, 3] = 1, 3, 3
        rgb[(2, 3)] = _clamped(HOT, Tg)                 # as if the two were not there
        # their own thresholds: the spike is the largest of their finite neighbours
        Th = _threshold(_y(HOT))
        rgb[(2, 4)] = rgb[(1, 3)] = np.array([Th, Th, Th], np.float32)
    elif case in ("id_border", "id_border_without_ids"):
        dim, bright, mid = (0.1, 0.1, 0.1), (50.0, 50.0, 50.0), (1.0, 1.0, 1.0)
        c[:, :3, :3], c[:, 3:, :3] = dim, bright
        ids[:, 3:] = 1
        c[2, 2, :3] = mid                                # on the dim side of the border
        if case == "id_border":
            cls[2, 2] = 1                                # its own surface alone sets the threshold
            rgb[(2, 2)] = _clamped(mid, _threshold(_y(dim)))
        else:
            ids = None                                   # three bright neighbours: the second largest is bright
    elif case in ("yk_negative_zero", "yk_negative"):
        params = dict(rank=1)
        c[..., :3] = -0.0 if case == "yk_negative_zero" else -1.0
        c[2, 3, :3] = GREY
        cls[2, 3] = 1
        floor = F(0.01)
        assert _threshold(-0.0) == floor and _threshold(_y((-1.0, -1.0, -1.0))) == floor
        rgb[(2, 3)] = _clamped(GREY, floor)
    else:
        raise KeyError(case)
    return c, ids, params, {"class": cls, "rgb": rgb}


def check_designed(case, color, res, expect):
    """The hand-written expectations on one set of outputs ({"out", "excess", "class", "info"})."""
    cls, out, exc = res["class"], res["out"], res["excess"]
    assert np.array_equal(cls, expect["class"]), (case, cls)
    changed = np.zeros(cls.shape, bool)
    for (y, x), v in expect["rgb"].items():
        changed[y, x] = True
        assert np.array_equal(bits(out[y, x, :3]), bits(v)), (case, y, x, out[y, x], v)
        want = color[y, x, :3] - v if cls[y, x] == 1 else np.zeros(3, np.float32)
        assert np.array_equal(bits(exc[y, x, :3]), bits(want.astype(np.float32))), (case, y, x, "excess")
    assert np.array_equal(changed, (cls == 1) | (cls == 3)), case
    assert np.array_equal(bits(out[~changed]), bits(color[~changed])), (case, "classes 0 and 2 keep their bits")
    assert np.array_equal(bits(out[..., 3]), bits(color[..., 3])), (case, "alpha")
    assert not bits(exc[~changed]).any() and not bits(exc[..., 3]).any(), (case, "excess is zero elsewhere")
    assert res["info"].tolist() == [int((cls == 1).sum()), int((cls == 3).sum())], case


# ---- what it is for: planted spikes
PLANT = dict(w=64, h=36, spp=64,
             at=[(3, 5), (3, 6), (10, 40), (17, 22), (20, 50), (25, 9), (30, 33), (8, 27), (33, 60), (14, 3)])


def plant(frame):
    """The frame with 1e4 spikes at a fixed scatter of pixels, (3, 5) and (3, 6) an adjacent pair."""
    out = frame.copy()
    for y, x in PLANT["at"]:
        out[y, x, :3] = SPIKE
    return out
