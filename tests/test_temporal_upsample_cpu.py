"""Temporal upsampling, host side (no GPU): the C-ABI's validation (lrt_temporal_upsample_*,
lrt_camera_jitter), the Python front end's argument checks, and the rule itself -- its NumPy
restatement (tests/temporal_upsample_ref.py): the integer taps under a jitter, every class of the
designed cases, the identity with temporal_gbuffer_ref.step at ratio 1, what it is for (a frame rebuilt
exactly from its jittered low samples), and the restatement's own f32 - f64 gap and fragile share on
the GPU test's cases."""
import ctypes
import os
from fractions import Fraction

import numpy as np
import pytest

import gbuffer_ref as G
import temporal_gbuffer_ref as TG
import temporal_upsample_ref as TU
import upsample_ref as U
from learnraytracing_amd import LrtError, _lib as L
from learnraytracing_amd import (default_camera, default_scene, jitter_camera, jitter_phases, make_camera, random_scene,
                                 temporal_gbuffer_desc, temporal_upsample_desc, temporal_upsample_host, upsample_desc)

# the restatement's own f32 - f64 gaps (`python tests/temporal_upsample_ref.py`), as
# tests/test_gpu_temporal_upsample.py records them
F32_F64_GAP = 1.1e-6                # measured: 1.03e-06 (rendered_gap()), color, moment2 and n
F32_F64_GAP_STD = 0.0               # measured: 0, color_std (n <= 2 after two steps: short_std itself)
F32_F64_GAP_DESIGNED = 2.7e-7       # measured: 2.51e-07 (designed_gap())
F32_F64_GAP_STD_DESIGNED = 1.5e-6   # measured: 1.44e-06
SCENE_OF = TU.scene_of(default_scene, random_scene)


def _gpu_present():
    import torch
    return torch.cuda.device_count() > 0


def _no_device():
    return os.environ.get("HIP_VISIBLE_DEVICES") == "" or not _gpu_present()


# ---- the C-ABI
def test_struct_and_defaults():
    assert ctypes.sizeof(L.TemporalUpsampleDesc) == 64
    assert [getattr(L.TemporalUpsampleDesc, f).offset for f in ("width", "low_width", "jitter_x", "flags", "min_history",
                                                                "cur_scale", "short_std", "sigma_normal", "weight_min",
                                                                "reserved")] == [0, 8, 16, 24, 28, 32, 44, 48, 56, 60]
    d = temporal_upsample_desc(16, 9, 8, 5)
    t, u = temporal_gbuffer_desc(16, 9), upsample_desc(16, 9, 8, 5)
    for name in ("alpha_min", "normal_min", "min_history", "short_std", "cur_scale"):
        assert getattr(d, name) == getattr(t, name), name                  # lrt_temporal_gbuffer_default's
    assert (d.sigma_normal, d.weight_min) == (u.sigma_normal, u.weight_min)   # lrt_upsample_default's
    assert d.sigma_sample == 0.5
    assert (d.width, d.height, d.low_width, d.low_height, d.jitter_x, d.jitter_y, d.flags, d.reserved) == \
        (16, 9, 8, 5, 0, 0, 0, 0)
    for name, v in TU.DEFAULTS.items():
        assert getattr(d, name) == np.float32(v), name
    assert temporal_upsample_desc(16, 9, 8, 5, jitter_x=-3, sigma_sample=0.25).jitter_x == -3
    lib = L.lib()
    assert lib.lrt_temporal_upsample_default(16, 9, 8, 5, None) == L.LRT_E_INVALID
    for bad in ((0, 9, 8, 5), (16, 0, 8, 5), (16, 9, 0, 5), (16, 9, 8, -1)):
        assert lib.lrt_temporal_upsample_default(*bad, ctypes.byref(d)) == L.LRT_E_INVALID
    with pytest.raises(LrtError):
        temporal_upsample_desc(16, 9, 8, 5, sigma_pos=0.1)
    src = open(L.HEADER_PATH).read()
    assert "not values\n * tuned here" in src or "not values tuned here" in src.replace("\n * ", " ")


def test_camera_jitter():
    """lrt_camera_jitter against its f32 restatement, bit for bit; only lowerLeftCorner moves; the low
    pixel centres land where the header says; refusals; no device is needed."""
    lib = L.lib()
    w, h, lw, lh = 67, 45, 33, 22
    cam = default_camera(w, h)
    base = np.float32(cam.to22())
    for jx, jy in ((0, 0), (7, -3), (w, -h), (-w, h), (1, 1), (-33, 22)):
        got = np.float32(jitter_camera(cam, w, h, lw, lh, jx, jy).to22())
        want = TU.jitter_camera(cam, w, h, lw, lh, jx, jy)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (jx, jy)
        moved = np.zeros(22, bool)
        moved[12:15] = True
        assert np.array_equal(got[~moved].view(np.uint32), base[~moved].view(np.uint32))
        assert (jx, jy) != (0, 0) or np.array_equal(got.view(np.uint32), base.view(np.uint32))
        # low pixel X's centre ray is the unjittered camera's ray through X + 1/2 + jx / (2 w)
        c = {k: v.astype(np.float64) for k, v in TU.R._cam(cam, np.float32).items()}
        _, D, _ = G.primary_rays(lw, lh, got, np.float64)
        ys, xs = np.mgrid[0:lh, 0:lw]
        s = (xs + 0.5 + jx / (2 * w)) / lw
        t = (ys + 0.5 + jy / (2 * h)) / lh
        want_d = c["L"] + s[..., None] * c["H"] + t[..., None] * c["V"] - c["O"]
        assert np.abs(D - want_d).max() <= 1e-6
    out = L.Camera()
    call = lambda *a: lib.lrt_camera_jitter(*a)   # noqa: E731
    ok = (ctypes.byref(cam), w, h, lw, lh, 1, 1, ctypes.byref(out))
    assert call(*ok) == 0
    assert call(None, *ok[1:]) == L.LRT_E_INVALID
    assert call(*ok[:7], None) == L.LRT_E_INVALID
    for k, v in ((1, 0), (2, -1), (3, 0), (4, 0), (3, w + 1), (4, h + 1), (1, 32769), (5, w + 1), (5, -w - 1), (6, h + 1),
                 (6, -h - 1)):
        bad = list(ok)
        bad[k] = v
        assert call(*bad) == L.LRT_E_INVALID, (k, v)
    assert "jitter" in lib.lrt_last_error().decode()
    with pytest.raises(LrtError):
        jitter_camera(cam.to22(), w, h, lw, lh, 0, 0)


def test_validation_before_device_use():
    """Every LRT_E_INVALID case, host and device entry points alike, with no device use; a valid
    call without lrt_initialize() is LRT_E_STATE."""
    lib = L.lib()
    w, h, lw, lh = 16, 9, 8, 5
    ptr = lambda a: a.ctypes.data   # noqa: E731
    lq = [np.zeros((lh, lw, 4), np.float32) for _ in range(2)]            # color_low, low normal
    hq = [np.zeros((h, w, 4), np.float32) for _ in range(8)]              # cur normal, motion; prev_g normal; prev 2; out 3
    ids = [np.zeros(5 * w * h + 16, np.int32) for _ in range(3)]          # low, cur, prev_g (room for a frame behind each)
    cls = np.zeros(w * h, np.int32)
    d = temporal_upsample_desc(w, h, lw, lh)

    def gb(normal, motion, idp):
        g = L.Gbuffer()
        g.normal, g.motion, g.id = normal, motion, idp
        return g

    def st(color, moment2):
        s = L.TemporalState()
        s.color, s.moment2 = color, moment2
        return s

    color = ptr(lq[0])
    low, cur, prev_g = gb(ptr(lq[1]), None, ptr(ids[0])), gb(ptr(hq[0]), ptr(hq[1]), ptr(ids[1])), \
        gb(ptr(hq[2]), None, ptr(ids[2]))
    prev, nxt = st(ptr(hq[3]), ptr(hq[4])), st(ptr(hq[5]), ptr(hq[6]))
    std, klass = ptr(hq[7]), ptr(cls)

    def calls(dd=d, c=color, lo=low, cu=cur, pg=prev_g, pv=prev, nx=nxt, sd=std, k=klass):
        ref = lambda x: ctypes.byref(x) if x is not None else None   # noqa: E731
        return (lib.lrt_temporal_upsample_host(ref(dd), c, ref(lo), ref(cu), ref(pg), ref(pv), ref(nx), sd, k),
                lib.lrt_temporal_upsample_device(ref(dd), c, ref(lo), ref(cu), ref(pg), ref(pv), ref(nx), sd, k, None))

    inv = (L.LRT_E_INVALID, L.LRT_E_INVALID)
    # required pointers, exactly one of prev and prev_g
    for kw in (dict(dd=None), dict(c=None), dict(lo=None), dict(cu=None), dict(nx=None), dict(pg=None), dict(pv=None)):
        assert calls(**kw) == inv, kw
    for which, g, members in (("lo", low, ("normal", "id")), ("cu", cur, ("normal", "motion", "id")),
                              ("pg", prev_g, ("normal", "id"))):
        for member in members:
            bad = gb(g.normal, g.motion, g.id)
            setattr(bad, member, None)
            assert calls(**{which: bad}) == inv, (which, member)
    for which, s in (("pv", prev), ("nx", nxt)):
        assert calls(**{which: st(None, s.moment2)}) == inv
        assert calls(**{which: st(s.color, None)}) == inv
    # the sizes, the jitter and the parameters
    nan, inf = np.nan, np.inf
    for member, values in (("width", (0, -1, lw - 1, 32769)), ("height", (0, lh - 1, 32769)), ("low_width", (0, -2, w + 1)),
                           ("low_height", (0, h + 1)), ("jitter_x", (w + 1, -w - 1, 1 << 30)),
                           ("jitter_y", (h + 1, -h - 1, -(1 << 30))), ("flags", (1, -1)), ("reserved", (1,)),
                           ("min_history", (0, -1)), ("cur_scale", (0.0, -1.0, nan, inf)),
                           ("alpha_min", (0.0, -0.1, 1.5, nan, inf)), ("normal_min", (-1.5, 1.5, nan, inf)),
                           ("short_std", (0.0, -1.0, nan, inf)), ("sigma_normal", (0.0, -1.0, nan, inf)),
                           ("sigma_sample", (0.0, -0.5, nan, inf)), ("weight_min", (0.0, -1e-3, nan, -inf, inf))):
        for v in values:
            bad = L.TemporalUpsampleDesc.from_buffer_copy(d)
            setattr(bad, member, v)
            assert calls(dd=bad) == inv, (member, v)
    bad = L.TemporalUpsampleDesc.from_buffer_copy(d)
    bad.width, bad.low_width = 32769, 32769
    assert calls(dd=bad) == inv
    bad = L.TemporalUpsampleDesc.from_buffer_copy(d)
    bad.width, bad.height = 1 << 15, 1 << 15                          # width * height > INT_MAX / 4
    assert calls(dd=bad) == inv
    # each output on each input and each previous buffer, and the outputs on each other
    ins = [color, low.normal, low.id, cur.normal, cur.motion, cur.id, prev_g.normal, prev_g.id, prev.color, prev.moment2]
    outs = dict(color=nxt.color, moment2=nxt.moment2, sd=std, k=klass)

    def with_out(name, p):
        if name in ("color", "moment2"):
            return calls(nx=st(p if name == "color" else nxt.color, p if name == "moment2" else nxt.moment2))
        return calls(**{name: p})

    for name in outs:
        for a in ins:
            assert with_out(name, a) == inv, name
        assert "alias" in lib.lrt_last_error().decode()
        for other, p in outs.items():
            if other != name:
                assert with_out(name, p) == inv, (name, other)
    assert with_out("k", std + 16 * w * h - 4) == inv                 # the class plane on color_std's last word
    assert with_out("color", cur.normal + 16) == inv                  # a partial overlap
    # the planes are sized by their own frames
    behind = ptr(ids[0]) + lw * lh * 4
    assert with_out("sd", behind - 4) == inv
    assert with_out("k", ptr(ids[1]) + w * h * 4 - 4) == inv
    # cur's normal or id on prev_g's
    assert calls(pg=gb(cur.normal, None, prev_g.id)) == inv
    assert calls(pg=gb(prev_g.normal, None, cur.id)) == inv
    assert "prev_g" in lib.lrt_last_error().decode()
    if _no_device():
        state = (L.LRT_E_STATE, L.LRT_E_STATE)
        assert calls() == state
        assert calls(sd=None, k=None) == state                           # both optional
        assert calls(pg=None, pv=None) == state                          # no history
        assert with_out("sd", behind) == state                           # right behind the low id plane
        assert with_out("k", ptr(ids[1]) + w * h * 4) == state
        lim = L.TemporalUpsampleDesc.from_buffer_copy(d)
        lim.jitter_x, lim.jitter_y = w, -h
        assert calls(dd=lim) == state


def test_front_end_argument_checks():
    w, h, lw, lh = 16, 9, 8, 5
    z = lambda hh, ww: np.zeros((hh, ww, 4), np.float32)   # noqa: E731
    zi = lambda hh, ww: np.zeros((hh, ww), np.int32)       # noqa: E731
    color = z(lh, lw)
    low = {"id": zi(lh, lw), "normal": z(lh, lw)}
    cur = {"id": zi(h, w), "normal": z(h, w), "motion": z(h, w)}
    prev_g, prev = {"id": zi(h, w), "normal": z(h, w)}, {"color": z(h, w), "moment2": z(h, w)}

    def bad(**kw):
        a = dict(color_low=color, low=low, cur=cur, prev_g=prev_g, prev=prev)
        a.update(kw)
        with pytest.raises(LrtError) as e:
            temporal_upsample_host(a.pop("color_low"), a.pop("low"), a.pop("cur"), a.pop("prev_g"), a.pop("prev"), **a)
        assert e.value.code == L.LRT_E_INVALID
        return str(e.value)

    assert "color_low must be" in bad(color_low=color.ravel())
    assert "hold" in bad(low={"normal": z(lh, lw)})
    assert "hold" in bad(cur={"id": zi(h, w), "normal": z(h, w)})
    assert "[height, width]" in bad(cur=dict(cur, id=zi(h, w).ravel()))
    assert "int32" in bad(low=dict(low, id=np.zeros((lh, lw), np.float32)))
    assert "unknown G-buffer plane" in bad(low=dict(low, colour=z(lh, lw)))
    assert "unknown temporal upsample parameter" in bad(sigma_pos=0.1)
    assert ">=" in bad(low=dict(low, normal=z(lh - 1, lw)))
    assert "lacks" in bad(prev={"color": z(h, w)})
    assert "int32" in bad(class_out=np.zeros((h, w), np.float32))
    assert "both" in bad(prev=None)                                       # through the library
    assert "jitter" in bad(jitter=(w + 1, 0))
    assert "alias" in bad(out={"color": cur["normal"], "moment2": z(h, w)})
    if _no_device():
        whole = dict(cur, world_pos=z(h, w), albedo=z(h, w), depth=np.zeros((h, w), np.float32))
        for kw in (dict(), dict(class_out=zi(h, w)), dict(jitter=(w, -h)), dict(prev_g=None, prev=None)):
            with pytest.raises(LrtError) as e:
                temporal_upsample_host(color, low, whole, kw.pop("prev_g", prev_g), kw.pop("prev", prev), **kw)
            assert e.value.code == L.LRT_E_STATE


# ---- step 1
@pytest.mark.parametrize("n,nl", [(7, 7), (12, 6), (96, 32), (67, 33), (5, 3), (2, 1), (1, 1), (32768, 32768), (32768, 1)])
def test_taps(n, nl):
    """The integer taps against exact rationals: the low coordinate of x's centre, less the jitter's
    shift, less the half pixel of tap X0, is X0 + t with 0 <= t < 1 -- a true floor for negative a too.
    Jitter 0 is upsample_ref's; at the extremes X0 = -1 at x = 0."""
    x0, t = TU.taps(n, nl, 0, np.float64)
    u0, ut = U.taps(n, nl, np.float64)
    assert np.array_equal(x0, u0) and np.array_equal(t, ut)
    pick = np.unique(np.clip([0, 1, 2, n // 2, n - 2, n - 1], 0, n - 1))
    for j in (0, n, -n, min(7, n), -min(3, n), 1, -1):
        x0, t = TU.taps(n, nl, j, np.float64)
        assert x0.min() >= -1 and x0.max() <= nl - 1 and (t >= 0).all() and (t < 1).all()
        for x in pick:
            pos = Fraction(2 * int(x) + 1, 2) * Fraction(nl, n) - Fraction(j, 2 * n) - Fraction(1, 2)   # in tap units
            fl = pos.numerator // pos.denominator
            assert int(x0[x]) == fl and Fraction(float(t[x])).limit_denominator(2 * n) == pos - fl, (j, x)
        a = (2 * np.arange(n, dtype=np.int64) + 1) * nl - n - j
        assert a.min() >= -2 * n + 1 and a.max() + 2 * n < 2 ** 32 and a.max() < 2 ** 31
    assert TU.taps(n, nl, n, np.float64)[0][0] == -1                  # a = nl - 2 n < 0 at x = 0
    if nl == n:
        x0, t = TU.taps(n, nl, n, np.float64)                          # ratio 1, half a pixel: between x - 1 and x
        assert np.array_equal(x0, np.arange(n) - 1) and (t == 0.5).all()
    if n > 1:
        assert TU.taps(n, nl, 1, np.float32)[1][0] > 0                 # r > 0: the true floor of a negative a
    with pytest.raises(AssertionError):
        TU.taps(n, nl, n + 1, np.float64)


@pytest.mark.parametrize("w,lw,h,lh", [(12, 6, 8, 4), (96, 32, 8, 8), (19, 19, 13, 13), (16, 4, 12, 3)])
def test_jitter_phases(w, lw, h, lh):
    """Over the phases every output pixel is sat on exactly once (tx = ty = 0: one tap of b = 1), each
    jitter is within the limits, and the order alternates the axes: the first R steps at ratio R already
    hold every phase of x and every phase of y."""
    ph = jitter_phases(w, lw, h, lh)
    assert ph == TU.jitter_phases(w, lw, h, lh) and len(ph) == (w // lw) * (h // lh) == len(set(ph))
    hits = np.zeros((h, w), int)
    for jx, jy in ph:
        assert abs(jx) <= w and abs(jy) <= h
        _, tx = TU.taps(w, lw, jx, np.float64)
        _, ty = TU.taps(h, lh, jy, np.float64)
        hits += (tx == 0)[None, :] & (ty == 0)[:, None]
    assert (hits == 1).all()
    rx, ry = w // lw, h // lh
    first = ph[:max(rx, ry)]                                           # a short run already covers either axis
    assert len({jx for jx, _ in first}) == rx and len({jy for _, jy in first}) == min(ry, len(first))
    if (w, h) == (2 * lw, 2 * lh):
        assert sorted(ph) == sorted((sx * lw, sy * lh) for sx in (-1, 1) for sy in (-1, 1)) and ph[0] == (-lw, -lh)
    with pytest.raises(LrtError):
        jitter_phases(67, 33, 44, 22)


# ---- the rule on the designed cases
def _expectations(case, cls, info, expect):
    for name, (mask, value) in expect.items():
        value = np.asarray(value)
        v = value[mask] if value.shape == mask.shape else value
        if name == "cls":
            assert np.array_equal(cls[mask], np.broadcast_to(v, cls[mask].shape)), case
        elif name == "beta_is_1":
            assert (info["beta"][mask] == 1).all(), case
        elif name == "beta_below":
            assert (info["beta"][mask] < value).all() and (info["beta"][mask] > 0).all(), case
        else:
            assert np.array_equal(info[name][mask], np.broadcast_to(v, info[name][mask].shape)), (case, name)


def test_designed_cases_hold_every_class():
    seen = np.zeros(4, int)
    for case in TU.DESIGNED_CASES:
        color, low, cur, prev_g, prev, jitter, params, expect = TU.designed_inputs(case)
        for T in (np.float64, np.float32):
            info = {}
            out, cls, fragile = TU.step(color, low, cur, prev_g, prev, jitter, T, info=info, **params)
            assert not fragile.any(), case
            _expectations(case, cls, info, expect)
            for name in TU.OUTPUTS:
                assert np.isfinite(out[name]).all(), (case, name)
        seen += TU.class_counts(cls)
        # what each class writes
        C = np.float64(color[..., :3])
        k2, k3, k1 = cls == 2, cls == 3, cls == 1
        assert np.array_equal(out["n"][k2], info["beta"][k2]) and (out["n"][k3] == 0).all()
        assert np.allclose(out["moment2"][k2 | k3], out["color"][k2 | k3] ** 2, rtol=1e-12)
        if k1.any():                                              # zero motion: the history's own pixel
            assert np.allclose(out["color"][k1], prev["color"][..., :3][k1], rtol=1e-12)
            assert np.array_equal(out["n"][k1], np.float64(prev["moment2"][..., 3][k1]))
        if k3.any():                                              # plain bilinear: within the low frame's range
            assert (out["color"][k3] <= C.max()).all() and (out["color"][k3] >= C.min()).all()
    assert (seen >= 9).all(), seen
    # all four classes in one frame
    cls = TU.step(*TU.designed_inputs("all_classes")[:6])[1]
    assert TU.class_counts(cls) == (56, 16, 12, 12)
    # n fractional on either side of min_history
    color, low, cur, prev_g, prev, jitter, params, _ = TU.designed_inputs("min_history")
    out, _, _ = TU.step(color, low, cur, prev_g, prev, jitter, **params)
    n = out["n"][1:-1, 1:-1]
    assert ((n != np.floor(n)) & (np.abs(n - 4) < 0.2)).all() and (n < 4).any() and (n > 4).any()
    assert np.array_equal(out["color_std"][1:-1, 1:-1, 0] == 1e3, n < 4)


def test_aligned_pixel_is_the_temporal_step():
    """beta = 1 on an aligned pixel: there the outputs are temporal_gbuffer_ref.step's on the colour of
    the one low sample."""
    color, low, cur, prev_g, prev, jitter, params, expect = TU.designed_inputs("aligned")
    out, _, _ = TU.step(color, low, cur, prev_g, prev, jitter, **params)
    on = expect["beta_is_1"][0]
    full = np.zeros((*on.shape, 4), np.float32)
    full[::2, ::2] = color                                      # the sample under every aligned pixel
    want, _ = TG.step(full, cur, prev_g, prev, **params)
    for name in TU.OUTPUTS:
        assert np.abs(out[name][on] - want[name][on]).max() <= 1e-12, name


def test_a_tap_of_b_zero_adds_nothing():
    """A NaN / Inf colour at a tap with b = 0 (and at taps of other pixels) changes nothing, bit for
    bit, at the pixels that give it no weight > 0; it reaches the others."""
    color, zeroed, low, cur, prev_g, prev, jitter, untouched, b0 = TU.nan_inputs()
    assert b0.sum() >= 4 and (~untouched).sum() >= 4
    for T in (np.float64, np.float32):
        a, ca, _ = TU.step(color, low, cur, prev_g, prev, jitter, T)
        b, cb, _ = TU.step(zeroed, low, cur, prev_g, prev, jitter, T)
        assert np.array_equal(ca, cb)
        for name in TU.OUTPUTS:
            assert np.isfinite(a[name][untouched]).all(), name
            assert a[name][untouched].tobytes() == b[name][untouched].tobytes(), name
        assert not np.isfinite(a["color"][~untouched]).all(axis=-1).any()


def test_underflowed_beta_over_an_empty_history():
    """beta = n_h = 0: alpha = max(0 / 0, 0) is 0 under the maximum that ignores a NaN, so the f32 run
    keeps the history and stays finite; f64 has beta / n = 1 and takes the frame. The pixels are
    fragile in both runs, and nowhere else."""
    color, low, cur, prev_g, prev, jitter, params, mask = TU.beta_zero_inputs()
    info = {}
    a, cls, fa = TU.step(color, low, cur, prev_g, prev, jitter, np.float32, info=info, **params)
    b, _, fb = TU.step(color, low, cur, prev_g, prev, jitter, np.float64, **params)
    assert (cls == 0).all() and (info["beta"] == 0).all() and info["speaks"].all()
    assert np.array_equal(fa, mask) and np.array_equal(fb, mask)
    for name in TU.OUTPUTS:
        assert np.isfinite(a[name]).all() and np.isfinite(b[name]).all(), name
    assert np.abs(a["color"][mask] - prev["color"][..., :3][mask]).max() <= 1e-6 and (a["n"][mask] == 0).all()
    assert np.abs(b["color"] - a["color"])[mask].max() > 0.1                 # the formats disagree there
    assert np.abs(b["color"] - a["color"])[~mask].max() <= 1e-6


# ---- the identity
def _identity_cases():
    for case in TG.DESIGNED_CASES:
        color, cur, prev_g, prev, params, _ = TG.designed_inputs(case)
        yield case, color, cur, prev_g, prev, params
    for w, h, count in ((19, 13, 9), (19, 13, 1000)):
        color, cur, prev_g, prev = TG.rendered_case(w, h, count, SCENE_OF, make_camera, TG.cpu_planes, TG.cpu_colour)
        yield f"{w}x{h} count {count}", color, cur, prev_g, prev, dict(cur_scale=TG.CUR_SCALE)


def test_ratio_one_without_jitter_is_the_temporal_step():
    """At ratio 1 with jitter 0, the pixel's own planes as the low ones: every output equals
    temporal_gbuffer_ref.step's to 1e-12 in f64; class 0 where that step keeps its history, 2 where it
    resets."""
    for case, color, cur, prev_g, prev, params in _identity_cases():
        low = {"id": cur["id"], "normal": cur["normal"]}
        info = {}
        want, _ = TG.step(color, cur, prev_g, prev, np.float64, info=info, **params)
        got, cls, _ = TU.step(color, low, cur, prev_g, prev, (0, 0), np.float64, **params)
        for name in TU.OUTPUTS:
            scale = np.maximum(1.0, np.abs(want[name]))
            assert (np.abs(got[name] - want[name]) <= 1e-12 * scale).all(), (case, name)
        keep = info["keep"] if prev is not None else np.zeros(cls.shape, bool)
        assert np.array_equal(cls, np.where(keep, 0, 2)), case


# ---- what it is for
@pytest.mark.parametrize("w,h,lw,lh", TU.CONVERGE_SIZES)
def test_jittered_samples_rebuild_the_frame(w, h, lw, lh):
    """A static frame of misses, sigma_sample 0.15, four steps cycling jitter_phases, the low colours the
    target T at the pixels each phase's samples sit on: the first step is all class 2, the later ones
    all class 0, and after the fourth |color - T| <= 1e-6 everywhere (each pixel has been sat on once
    with beta = 1 and is moved by beta ~ 2e-10 otherwise). upsample_ref with one such low frame stays
    above 0.1."""
    steps = TU.converge_ref(w, h, lw, lh, np.float64)
    print(f"{w}x{h} from {lw}x{lh}: |color - T| per step " + ", ".join(f"{e:.3g}" for _, e in steps))
    assert (steps[0][0] == 2).all()
    for cls, _ in steps[1:]:
        assert (cls == 0).all()
    assert all(e > 0.1 for _, e in steps[:3])
    assert steps[3][1] <= 1e-6
    target = TU.converge_target(w, h)
    miss = lambda hh, ww: {"id": np.full((hh, ww), -1, np.int32), "normal": np.zeros((hh, ww, 4), np.float32)}   # noqa: E731
    up, _, _ = U.upsample(target[0::h // lh, 0::w // lw], miss(lh, lw), miss(h, w))
    print(f"upsample_ref from the first phase's samples: {np.abs(up - target).max():.3g}")
    assert np.abs(up - target).max() > 0.1


# ---- the restatement's own gap and fragile share on the GPU test's cases
def test_f32_f64_gap_and_fragile_share():
    gap, gap_std, report = TU.rendered_gap(SCENE_OF, make_camera, TU.jitter_camera, TU.cpu_planes, TU.cpu_colour)
    print(f"rendered: {gap:.3g}, color_std {gap_std:.3g}")
    for label, (share, counts) in report.items():
        print(f"  {label}: fragile {100 * share:.2f} %, classes {counts}")
        assert share <= TU.MAX_FRAGILE, label
    assert gap <= F32_F64_GAP and gap_std <= F32_F64_GAP_STD
    assert gap >= F32_F64_GAP / 4                                           # the record is not stale
    gap, gap_std, report = TU.designed_gap()
    print(f"designed: {gap:.3g}, color_std {gap_std:.3g}")
    assert all(share <= TU.MAX_FRAGILE for share, _ in report.values())
    assert gap <= F32_F64_GAP_DESIGNED and gap_std <= F32_F64_GAP_STD_DESIGNED
    assert gap >= F32_F64_GAP_DESIGNED / 4 and gap_std >= F32_F64_GAP_STD_DESIGNED / 4
    counts = np.sum([c for _, c in report.values()], axis=0)
    assert (counts > 0).all()
