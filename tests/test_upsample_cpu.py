"""G-buffer-guided upsampling, host side (no GPU): the C-ABI's validation (lrt_upsample_*), the
Python front end's argument checks, and the rule itself -- its NumPy restatement
(tests/upsample_ref.py) against itself, every branch of the designed cases populated, the class
counts of the rendered cases, and the restatement's own f32 - f64 gap and fragile share on the GPU
test's cases."""
import ctypes
import os

import numpy as np
import pytest

import upsample_ref as U
from learnraytracing_amd import LrtError, _lib as L
from learnraytracing_amd import default_camera, default_scene, random_scene, upsample_desc, upsample_host

# the restatement's own f32 - f64 gaps (`python tests/upsample_ref.py`), as tests/test_gpu_upsample.py
# records them
F32_F64_GAP = 9.5e-7            # measured: 9.04e-07 (rendered_gap())
F32_F64_GAP_DESIGNED = 1.9e-7   # measured: 1.80e-07 (designed_gap())
SCENE_OF = U.scene_of(default_scene, random_scene)


def _gpu_present():
    import torch
    return torch.cuda.device_count() > 0


def _no_device():
    return os.environ.get("HIP_VISIBLE_DEVICES") == "" or not _gpu_present()


# ---- the C-ABI
def test_struct_and_defaults():
    assert ctypes.sizeof(L.UpsampleDesc) == 40
    assert [getattr(L.UpsampleDesc, f).offset for f in ("width", "low_width", "flags", "sigma_normal", "weight_min",
                                                        "reserved2")] == [0, 8, 16, 24, 32, 36]
    d = upsample_desc(16, 9, 8, 5)
    s = L.SvgfDesc()
    assert L.lib().lrt_svgf_default(16, 9, ctypes.byref(s)) == 0
    assert (d.sigma_normal, d.albedo_floor) == (s.sigma_normal, s.albedo_floor)       # lrt_svgf's
    assert (d.width, d.height, d.low_width, d.low_height, d.flags, d.reserved, d.reserved2) == (16, 9, 8, 5, 0, 0, 0)
    assert (d.sigma_normal, d.albedo_floor, d.weight_min) == (np.float32(0.3), np.float32(0.01), np.float32(1e-3))
    assert upsample_desc(16, 9, 8, 5, flags=L.UP_BILINEAR, weight_min=0.5).flags == 1
    lib = L.lib()
    assert lib.lrt_upsample_default(16, 9, 8, 5, None) == L.LRT_E_INVALID
    for bad in ((0, 9, 8, 5), (16, 0, 8, 5), (16, 9, 0, 5), (16, 9, 8, -1)):
        assert lib.lrt_upsample_default(*bad, ctypes.byref(d)) == L.LRT_E_INVALID
    with pytest.raises(LrtError):
        upsample_desc(16, 9, 8, 5, sigma_pos=0.1)
    assert L.UP_BILINEAR == U.UP_BILINEAR and L.UP_MAX_SIZE == U.MAX_SIZE
    src = open(L.HEADER_PATH).read()
    assert "#define LRT_UP_BILINEAR 1" in src


def test_validation_before_device_use():
    """Every LRT_E_INVALID case, host and device entry points alike, with no device use; a valid
    call without lrt_initialize() is LRT_E_STATE."""
    lib = L.lib()
    w, h, lw, lh = 16, 9, 8, 5
    ptr = lambda a: a.ctypes.data   # noqa: E731
    lq = [np.zeros((lh, lw, 4), np.float32) for _ in range(3)]            # color_low, low normal, low albedo
    hq = [np.zeros((h, w, 4), np.float32) for _ in range(3)]              # high normal, high albedo, out
    lid = np.zeros(lw * lh + 4 * w * h + 16, np.int32)                    # (an id plane and room for a frame behind it)
    hid = np.zeros(5 * w * h + 16, np.int32)
    cls = np.zeros(w * h, np.int32)
    d = upsample_desc(w, h, lw, lh)

    def gb(normal, albedo, idp):
        g = L.Gbuffer()
        g.normal, g.albedo, g.id = normal, albedo, idp
        return g

    color, out, klass = ptr(lq[0]), ptr(hq[2]), ptr(cls)
    low, high = gb(ptr(lq[1]), ptr(lq[2]), ptr(lid)), gb(ptr(hq[0]), ptr(hq[1]), ptr(hid))

    def calls(dd=d, c=color, lo=low, hi=high, o=out, k=klass):
        ref = lambda x: ctypes.byref(x) if x is not None else None   # noqa: E731
        return (lib.lrt_upsample_host(ref(dd), c, ref(lo), ref(hi), o, k),
                lib.lrt_upsample_device(ref(dd), c, ref(lo), ref(hi), o, k, None))

    inv = (L.LRT_E_INVALID, L.LRT_E_INVALID)
    # required pointers
    assert calls(dd=None) == inv
    assert calls(c=None) == inv
    assert calls(lo=None) == inv
    assert calls(hi=None) == inv
    assert calls(o=None) == inv
    for member in ("normal", "id"):
        for which, g in (("lo", low), ("hi", high)):
            bad = gb(g.normal, g.albedo, g.id)
            setattr(bad, member, None)
            assert calls(**{which: bad}) == inv, (which, member)
    # albedo on one side only
    assert calls(lo=gb(low.normal, None, low.id)) == inv
    assert calls(hi=gb(high.normal, None, high.id)) == inv
    assert "albedo" in lib.lrt_last_error().decode()
    # the sizes
    for member, values in (("width", (0, -1, lw - 1, 32769)), ("height", (0, lh - 1, 32769)), ("low_width", (0, -2, w + 1)),
                           ("low_height", (0, h + 1)), ("flags", (2, 3, -1)), ("reserved", (1,)), ("reserved2", (1,)),
                           ("sigma_normal", (0.0, -1.0, np.nan, np.inf)), ("albedo_floor", (0.0, -0.01, np.nan, np.inf)),
                           ("weight_min", (0.0, -1e-3, np.nan, -np.inf, np.inf))):
        for v in values:
            bad = L.UpsampleDesc.from_buffer_copy(d)
            setattr(bad, member, v)
            assert calls(dd=bad) == inv, (member, v)
    bad = L.UpsampleDesc.from_buffer_copy(d)
    bad.width, bad.low_width = 32769, 32769                          # past the limit whatever the low frame
    assert calls(dd=bad) == inv
    bad = L.UpsampleDesc.from_buffer_copy(d)
    bad.width, bad.height = 1 << 15, 1 << 15                          # width * height > INT_MAX / 4
    assert calls(dd=bad) == inv
    # each output on each input, and the outputs on each other
    ins = [color, low.normal, low.albedo, low.id, high.normal, high.albedo, high.id]
    for a in ins:
        assert calls(o=a) == inv
        assert calls(k=a) == inv
    assert "alias" in lib.lrt_last_error().decode()
    assert calls(k=out) == inv
    assert calls(k=out + 16 * w * h - 4) == inv                       # the class plane on out's last word
    assert calls(o=klass) == inv
    assert calls(o=high.normal + 16) == inv                           # a partial overlap
    # the planes are sized by their own frames: the low id plane is low_width * low_height * 4 bytes
    behind = ptr(lid) + lw * lh * 4
    assert calls(o=behind - 4) == inv
    assert calls(k=ptr(hid) + w * h * 4 - 4) == inv
    if _no_device():
        state = (L.LRT_E_STATE, L.LRT_E_STATE)
        assert calls() == state
        assert calls(k=None) == state                                    # class_out is optional
        assert calls(lo=gb(low.normal, None, low.id), hi=gb(high.normal, None, high.id)) == state    # no albedo
        assert calls(o=behind) == state                                  # right behind the low id plane
        assert calls(k=ptr(hid) + w * h * 4) == state
        flag = L.UpsampleDesc.from_buffer_copy(d)
        flag.flags = L.UP_BILINEAR                                       # the normals may then be NULL
        assert calls(dd=flag, lo=gb(None, low.albedo, low.id), hi=gb(None, high.albedo, high.id)) == state
        same = L.UpsampleDesc.from_buffer_copy(d)
        same.low_width, same.low_height = w, h
        big = [np.zeros((h, w, 4), np.float32) for _ in range(3)]
        assert calls(dd=same, c=ptr(big[0]), lo=gb(ptr(big[1]), ptr(big[2]), ptr(hid) + 4 * w * h)) == state


def test_front_end_argument_checks():
    w, h, lw, lh = 16, 9, 8, 5
    z = lambda hh, ww: np.zeros((hh, ww, 4), np.float32)   # noqa: E731
    zi = lambda hh, ww: np.zeros((hh, ww), np.int32)       # noqa: E731
    color = z(lh, lw)
    low, high = {"id": zi(lh, lw), "normal": z(lh, lw), "albedo": z(lh, lw)}, {"id": zi(h, w), "normal": z(h, w),
                                                                               "albedo": z(h, w)}

    def bad(**kw):
        a = dict(color_low=color, low=low, high=high)
        a.update(kw)
        with pytest.raises(LrtError) as e:
            upsample_host(a.pop("color_low"), a.pop("low"), a.pop("high"), **a)
        assert e.value.code == L.LRT_E_INVALID
        return str(e.value)

    assert "color_low must be" in bad(color_low=color.ravel())
    assert "hold" in bad(low={"normal": z(lh, lw)})
    assert "hold" in bad(high={"id": zi(h, w)})
    assert "[height, width]" in bad(high=dict(high, id=zi(h, w).ravel()))
    assert "int32" in bad(low=dict(low, id=np.zeros((lh, lw), np.float32)))
    assert "float32" in bad(high=dict(high, normal=np.zeros((h, w, 4), np.float64)))
    assert "unknown G-buffer plane" in bad(low=dict(low, colour=z(lh, lw)))
    assert "unknown upsample parameter" in bad(sigma_pos=0.1)
    assert ">=" in bad(low=dict(low, normal=z(lh - 1, lw)))
    assert ">=" in bad(out=z(h - 1, w))
    assert "int32" in bad(class_out=np.zeros((h, w), np.float32))
    assert "albedo" in bad(low={k: v for k, v in low.items() if k != "albedo"})       # through the library
    assert "alias" in bad(out=high["normal"])
    assert "exceed" in bad(color_low=z(h + 1, w), low={"id": zi(h + 1, w), "normal": z(h + 1, w), "albedo": z(h + 1, w)})
    if _no_device():
        whole = dict(low, world_pos=z(lh, lw), depth=np.zeros((lh, lw), np.float32), motion=z(lh, lw))
        for kw in (dict(), dict(class_out=zi(h, w)), dict(flags=L.UP_BILINEAR)):
            with pytest.raises(LrtError) as e:
                upsample_host(color, whole, high, **kw)
            assert e.value.code == L.LRT_E_STATE
        with pytest.raises(LrtError) as e:                         # under the flag the normals are not needed
            upsample_host(color, {"id": low["id"]}, {"id": high["id"]}, flags=L.UP_BILINEAR)
        assert e.value.code == L.LRT_E_STATE


# ---- the rule
def test_taps_are_exact_integers():
    """Step 1 at ratio 2, 3, 1 and a non-integer ratio: X0 and tx are the centre's position exactly."""
    x0, tx = U.taps(12, 6, np.float64)
    assert x0.tolist() == [-1, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5]
    assert tx.tolist() == [0.75, 0.25] * 6
    x0, tx = U.taps(9, 3, np.float32)
    assert x0.tolist() == [-1, 0, 0, 0, 1, 1, 1, 2, 2] and np.allclose(tx, [2 / 3, 0, 1 / 3] * 3, atol=1e-7)
    assert tx[1] == 0 and tx.dtype == np.float32
    x0, tx = U.taps(7, 7, np.float64)
    assert x0.tolist() == list(range(7)) and (tx == 0).all()
    x0, tx = U.taps(67, 33, np.float64)
    centre = (np.arange(67) + 0.5) * 33 / 67 - 0.5
    assert np.array_equal(x0, np.floor(centre)) and np.allclose(tx, centre - np.floor(centre), atol=1e-12)
    x0, _ = U.taps(32768, 32768, np.float64)                     # the largest a: below 2^31
    assert (2 * 32767 + 1) * 32768 - 32768 < 2 ** 31 and x0[-1] == 32767


def test_identity_is_bit_exact_without_albedo():
    rng = np.random.default_rng(3)
    h, w = 13, 19
    color = rng.uniform(0.0, 50.0, (h, w, 4)).astype(np.float32)
    g = {"id": rng.integers(-1, 4, (h, w)).astype(np.int32), "normal": U.quad(rng.normal(size=(h, w, 3)))}
    g["normal"][g["id"] < 0] = 0
    for dt in (np.float32, np.float64):
        out, cls, fragile = U.upsample(color, g, g, dt)
        assert np.array_equal(out, color[..., :3].astype(dt)) and (cls == 0).all() and not fragile.any()


def test_flag_form_keeps_a_constant():
    (w, h), (lw, lh) = (12, 8), (6, 4)
    color = np.full((lh, lw, 4), 0.37, np.float32)
    low, high = {"id": np.zeros((lh, lw), np.int32)}, {"id": np.zeros((h, w), np.int32)}
    out, cls, fragile = U.upsample(color, low, high, np.float64, U.UP_BILINEAR)
    assert (cls == 2).all() and not fragile.any()
    assert np.abs(out - np.float64(np.float32(0.37))).max() <= 1e-12


@pytest.mark.parametrize("case", U.DESIGNED_CASES)
def test_designed_cases_hold_their_branches(case):
    color, low, high, expect = U.designed_inputs(case)
    assert expect
    for albedo in (True, False):
        lo, hi = (low, high) if albedo else (U.without_albedo(low), U.without_albedo(high))
        info = {}
        out, cls, fragile = U.upsample(color, lo, hi, np.float64, info=info)
        assert not fragile.any() and np.isfinite(out).all()
        for name, (mask, value) in expect.items():
            assert mask.any(), name
            value = np.asarray(value)
            value = value[mask] if value.shape == mask.shape else value
            got = cls if name == "cls" else info[name]
            assert np.array_equal(got[mask], np.broadcast_to(value, got[mask].shape)), (name, albedo)
    out, cls, _ = U.upsample(color, low, high, np.float64)
    plain, _, _ = U.upsample(color, U.without_albedo(low), U.without_albedo(high), np.float64)
    if case == "all_match":        # g is the same at every tap: the guided form is the bilinear one of the inside taps
        flag, _, _ = U.upsample(color, U.without_albedo(low), U.without_albedo(high), np.float64, U.UP_BILINEAR)
        assert np.abs(plain - flag).max() <= 1e-12
    if case == "ring":             # nothing of the 2 x 2's other sphere reaches its pixels
        mask = expect["cls"][0]
        ring = np.float64(color[..., :3])[low["id"] == 0]
        assert (plain[mask] >= ring.min(0) - 1e-12).all() and (plain[mask] <= ring.max(0) + 1e-12).all()
    if case == "opposite":         # g = exp(-4 / 0.09) = 5e-20: nothing within the ring either
        info = {}
        U.upsample(color, low, high, np.float64, info=info)
        right = expect["cls"][1] == 2
        assert (info["sw0"][right] < 1e-18).all() and (info["sw1"][right] < 1e-18).all() and (info["sw1"][right] > 0).all()
    if case == "albedo_floor":     # the floor divides and multiplies: finite, and the low rows' colours come back over 0.01
        assert np.isfinite(out).all()
        assert out[0, 0] == pytest.approx(np.float64(color[0, 0, :3]) / 0.01 * 0.01, rel=1e-12)
        # 0.001, 0 and 0.004 all stand at the floor: over it and times it, the plain result
        assert out[:5] == pytest.approx(plain[:5], rel=1e-9)
    if case == "firefly":          # 1e4 in one tap spreads to the pixels that read it and no further
        hot = plain.max(-1) > 100
        assert 4 <= hot.sum() <= 16 and np.isfinite(plain).all()
    if case == "miss_among_hits":  # class 2 of a miss: the demodulated mixture, not multiplied back
        y, x = np.argwhere(high["id"] == -1)[0]
        assert np.isfinite(out[y, x]).all() and not np.allclose(out[y, x], plain[y, x])


def test_every_designed_class_occurs():
    seen = set()
    for case in U.DESIGNED_CASES:
        color, low, high, _ = U.designed_inputs(case)
        seen |= set(np.unique(U.upsample(color, low, high, np.float64)[1]).tolist())
    assert seen == {0, 1, 2}


def test_restatement_gap_fragile_share_and_class_counts_on_the_gpu_cases():
    """The restatement's own f32 - f64 gap stays within the recorded constants (the GPU test's TOL is
    16 x them), no case of the GPU test has more than MAX_FRAGILE fragile pixels, and the rendered
    cases hold the class counts recorded in upsample_ref.RENDERED_CASES."""
    gap, report = U.rendered_gap(SCENE_OF, default_camera, U.cpu_planes, U.cpu_colour)
    print(f"rendered: {gap:.3g}; " + ", ".join(f"{k}: fragile {100 * s:.2f} % classes {c}" for k, (s, c) in report.items()))
    assert gap <= F32_F64_GAP
    assert set(report) == {case[0] for case in U.RENDERED_CASES}
    for label, _, w, h, _, _, counts in U.RENDERED_CASES:
        share, got = report[label]
        assert share <= U.MAX_FRAGILE, label
        assert sum(got) == w * h
        if counts is not None:
            assert got == counts, label
    gap, report = U.designed_gap()
    print(f"designed: {gap:.3g}")
    assert gap <= F32_F64_GAP_DESIGNED
    for label, (share, _) in report.items():
        assert share <= U.MAX_FRAGILE, label


def test_bilinear_taps_of_another_sphere():
    """What the stage is for, counted: at 66 x 44 from 33 x 22 on the default scene 748 of 2904 pixels
    have a bilinear tap of another sphere (1773 of 14400 at 160 x 90 from 80 x 45), and the guided form
    takes none of them: every pixel is class 0."""
    s, m = default_scene()
    for (w, h, lw, lh), want in (((66, 44, 33, 22), 748), ((160, 90, 80, 45), 1773)):
        cam = default_camera(w, h)
        low, high = U.cpu_planes(lw, lh, cam, s, m), U.cpu_planes(w, h, cam, s, m)
        assert int(U.other_sphere_taps(low["id"], high["id"]).sum()) == want
    palette = np.random.default_rng(1).uniform(0.1, 1.0, (10, 3)).astype(np.float32)
    cam = default_camera(66, 44)
    low, high = U.cpu_planes(33, 22, cam, s, m), U.cpu_planes(66, 44, cam, s, m)
    color = U.quad(palette[low["id"] + 1])
    out, cls, _ = U.upsample(color, U.without_albedo(low), U.without_albedo(high), np.float64)
    assert (cls == 0).all() and np.abs(out - palette[high["id"] + 1]).max() <= 1e-6


def test_refused_taps_may_hold_anything():
    """The `ring` case with NaN and Inf as the colours of the other sphere's low pixels: no pixel of
    sphere 0 counts such a tap, so the guided form is finite everywhere and equal, bit for bit, to the
    run with those colours zeroed; the flag form, which counts every inside tap, is not finite."""
    color, zeroed, low, high = U.nonfinite_inputs()
    for lo, hi in ((low, high), (U.without_albedo(low), U.without_albedo(high))):
        for dt in (np.float32, np.float64):
            out, cls, _ = U.upsample(color, lo, hi, dt)
            want, wcls, _ = U.upsample(zeroed, lo, hi, dt)
            assert np.isfinite(out).all() and np.array_equal(out, want) and np.array_equal(cls, wcls)
            assert set(np.unique(cls)) == {0, 1}
    assert not np.isfinite(U.upsample(color, low, high, np.float64, U.UP_BILINEAR)[0]).all()
