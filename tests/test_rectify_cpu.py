"""History rectification, host side (no GPU): the C-ABI's struct, defaults and validation
(lrt_temporal_rectify_*), the Python front end's argument checks, and the rule itself -- its NumPy
restatement (tests/rectify_ref.py): every branch of the designed cases held by exact expectations,
the restatement's own f32 - f64 gap and fragile share on the GPU test's cases, and what the stage is
for on a noise-free sequence whose errors can be derived by hand."""
import ctypes
import os

import numpy as np
import pytest

import rectify_ref as Q
import temporal_gbuffer_ref as TG
from learnraytracing_amd import LrtError, _lib as L
from learnraytracing_amd import (default_scene, make_camera, random_scene, temporal_gbuffer_desc, temporal_rectify_desc,
                                 temporal_rectify_host)

# the restatement's own f32 - f64 gaps (`python tests/rectify_ref.py`), as tests/test_gpu_rectify.py records them
F32_F64_GAP, F32_F64_GAP_STD = 4.2e-6, 2.5e-5                     # measured: 4.13e-06, 2.48e-05
F32_F64_GAP_DESIGNED, F32_F64_GAP_STD_DESIGNED = 2.2e-6, 5.5e-7   # measured: 2.15e-06, 5.37e-07
SCENE_OF = TG.scene_of(default_scene, random_scene)


def _gpu_present():
    import torch
    return torch.cuda.device_count() > 0


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ---- the C-ABI
def test_struct_and_defaults():
    assert ctypes.sizeof(L.RectifyDesc) == 48
    names = [f for f, _ in L.RectifyDesc._fields_]
    assert names == ["width", "height", "radius", "min_taps", "min_history", "flags", "ref_scale", "gamma", "range_floor",
                     "reset_history", "short_std", "reserved"]
    assert [getattr(L.RectifyDesc, f).offset for f in names] == list(range(0, 48, 4))
    d = temporal_rectify_desc(16, 9)
    assert (d.width, d.height, d.flags, d.reserved) == (16, 9, 0, 0)
    assert (d.radius, d.min_taps, d.gamma, d.range_floor, d.reset_history, d.ref_scale) == \
        (2, 5, 1.0, np.float32(1e-4), 1.0, 1.0)
    g = temporal_gbuffer_desc(16, 9)
    assert (d.min_history, d.short_std) == (g.min_history, g.short_std) == (4, 1e3)
    assert L.RECTIFY_MAX_RADIUS == 3 and set(L.RECTIFY_PARAMS) == set(names) - {"width", "height", "flags", "reserved"}
    d = temporal_rectify_desc(16, 9, radius=3, min_taps=49, gamma=0.5)
    assert (d.radius, d.min_taps, d.gamma) == (3, 49, 0.5)
    lib = L.lib()
    assert lib.lrt_temporal_rectify_default(16, 9, None) == L.LRT_E_INVALID
    assert lib.lrt_temporal_rectify_default(0, 9, ctypes.byref(d)) == L.LRT_E_INVALID
    with pytest.raises(LrtError):
        temporal_rectify_desc(16, 9, alpha_min=0.1)            # the stage blends nothing


def test_validation_before_device_use():
    """Every LRT_E_INVALID case, host and device entry points alike, with no device use; the two
    allowed equalities get as far as LRT_E_STATE without lrt_initialize()."""
    lib = L.lib()
    w, h = 16, 9
    quads = [np.zeros((h, w, 4), np.float32) for _ in range(7)]
    words = [np.zeros(5 * w * h + 16, np.int32) for _ in range(2)]   # (a word plane and room for a frame behind it)
    ptr = lambda a: a.ctypes.data   # noqa: E731
    d = temporal_rectify_desc(w, h)

    def st(color, moment2):
        s = L.TemporalState()
        s.color, s.moment2 = color, moment2
        return s

    ref, ids, cls = ptr(quads[0]), ptr(words[0]), ptr(words[1])
    state, out, std = st(ptr(quads[1]), ptr(quads[2])), st(ptr(quads[3]), ptr(quads[4])), ptr(quads[5])

    def calls(dd=d, r=ref, i=ids, s=state, o=out, sd=std, c=cls):
        byref = lambda x: ctypes.byref(x) if x is not None else None   # noqa: E731
        return (lib.lrt_temporal_rectify_host(byref(dd), r, i, byref(s), byref(o), sd, c),
                lib.lrt_temporal_rectify_device(byref(dd), r, i, byref(s), byref(o), sd, c, None))

    inv = (L.LRT_E_INVALID, L.LRT_E_INVALID)
    # required pointers
    for kw in (dict(dd=None), dict(r=None), dict(i=None), dict(s=None), dict(o=None)):
        assert calls(**kw) == inv, kw
    for member in ("color", "moment2"):
        for which, base in (("s", state), ("o", out)):
            bad = st(base.color, base.moment2)
            setattr(bad, member, None)
            assert calls(**{which: bad}) == inv, (which, member)
    # the parameter ranges
    for member, values in (("width", (0, -1)), ("height", (0,)), ("flags", (1,)), ("reserved", (1,)),
                           ("radius", (0, 4, -1)), ("min_taps", (0, 26, -2)), ("min_history", (0, -3)),
                           ("ref_scale", (0.0, -1.0, np.nan, np.inf)), ("gamma", (-0.5, np.nan, np.inf)),
                           ("range_floor", (0.0, -1e-4, np.nan, np.inf)), ("reset_history", (-1.0, np.nan, np.inf)),
                           ("short_std", (0.0, -1.0, np.inf, np.nan))):
        for v in values:
            bad = L.RectifyDesc.from_buffer_copy(d)
            setattr(bad, member, v)
            assert calls(dd=bad) == inv, (member, v)
    for rad, taps in ((1, 10), (3, 50)):                              # min_taps follows the radius
        bad = L.RectifyDesc.from_buffer_copy(d)
        bad.radius, bad.min_taps = rad, taps
        assert calls(dd=bad) == inv, (rad, taps)
    bad = L.RectifyDesc.from_buffer_copy(d)
    bad.width, bad.height = 1 << 15, 1 << 15                          # width * height > INT_MAX / 4
    assert calls(dd=bad) == inv
    # each of the four outputs on each input ...
    ins = [ref, ids, state.color, state.moment2]
    for a in ins:
        if a != state.color:
            assert calls(o=st(a, out.moment2)) == inv
        if a != state.moment2:
            assert calls(o=st(out.color, a)) == inv
        assert calls(sd=a) == inv
        assert calls(c=a) == inv
    assert "alias" in lib.lrt_last_error().decode()
    # ... partially where the whole is allowed ...
    assert calls(o=st(state.color + 16, out.moment2)) == inv
    assert calls(o=st(out.color, state.moment2 + 16)) == inv
    assert calls(o=st(state.moment2, state.color)) == inv             # crossed over
    # ... and on each other
    assert calls(o=st(out.color, out.color)) == inv
    for a in (out.color, out.moment2):
        assert calls(sd=a) == inv
        assert calls(c=a) == inv
    assert calls(c=std) == inv
    assert calls(sd=out.moment2 + 16) == inv
    assert calls(o=st(state.color, state.color)) == inv               # in place, and moment2 on top of it
    # the id and class planes are width * height * 4 bytes: an output may start right behind one, not inside it
    behind = ptr(words[0]) + w * h * 4
    assert calls(sd=behind - 4) == inv
    assert calls(c=behind - 4) == inv
    assert calls(sd=cls + w * h * 4 - 4) == inv
    if os.environ.get("HIP_VISIBLE_DEVICES") == "" or not _gpu_present():
        ok = (L.LRT_E_STATE, L.LRT_E_STATE)
        assert calls() == ok
        assert calls(sd=None) == ok and calls(c=None) == ok and calls(sd=None, c=None) == ok
        assert calls(o=st(state.color, out.moment2)) == ok            # in place, each independently
        assert calls(o=st(out.color, state.moment2)) == ok
        assert calls(o=state) == ok
        assert calls(sd=behind) == ok and calls(c=behind) == ok       # right behind the id plane: no overlap
        for rad, taps in ((1, 9), (2, 25), (3, 49)):
            good = L.RectifyDesc.from_buffer_copy(d)
            good.radius, good.min_taps, good.gamma, good.reset_history = rad, taps, 0.0, 0.0
            assert calls(dd=good) == ok, rad


def test_front_end_argument_checks():
    w, h = 16, 9
    z = lambda: np.zeros((h, w, 4), np.float32)   # noqa: E731
    ref, ids, state = z(), np.zeros((h, w), np.int32), {"color": z(), "moment2": z()}

    def bad(**kw):
        a = dict(ref=ref, id=ids, state=state)
        a.update(kw)
        with pytest.raises(LrtError) as e:
            temporal_rectify_host(a.pop("ref"), a.pop("id"), a.pop("state"), **a)
        assert e.value.code == L.LRT_E_INVALID
        return str(e.value)

    assert "int32" in bad(id=np.zeros((h, w), np.float32))
    assert "float32" in bad(ref=np.zeros((h, w, 4), np.float64))
    assert "lacks" in bad(state={"color": z()})
    assert "lacks" in bad(out={"color": z()})
    assert "unknown state buffer" in bad(out={"color": z(), "moment2": z(), "normal": z()})
    assert "unknown rectify parameter" in bad(alpha_min=0.1)
    assert "int32" in bad(class_out=np.zeros((h, w), np.float32))
    assert ">=" in bad(id=np.zeros((h - 1, w), np.int32))
    assert "radius" in bad(radius=4)                     # through the library
    assert "alias" in bad(out={"color": ref, "moment2": z()})
    assert "alias" in bad(out={"color": state["moment2"], "moment2": z()})
    if os.environ.get("HIP_VISIBLE_DEVICES") == "" or not _gpu_present():
        whole = dict(state, normal=z(), world_pos=z(), albedo=z(), color_std=z())
        for kw in (dict(), dict(out=whole), dict(out=dict(state)), dict(class_out=np.zeros((h, w), np.int32))):
            with pytest.raises(LrtError) as e:
                temporal_rectify_host(ref, ids, whole, **kw)
            assert e.value.code == L.LRT_E_STATE, kw


def test_step_gbuffer_takes_rectify():
    import inspect
    from learnraytracing_amd import TemporalAccumulator, TemporalUpsampler
    assert inspect.signature(TemporalAccumulator.step_gbuffer).parameters["rectify"].default is None
    assert "temporal_rectify_tensor" in TemporalUpsampler.__doc__


def test_rectify_bench_bytes():
    """tools/rectify_bench.py counts the bytes the header's buffers give: 16 + 4 + 16 + 16 read, 12 + 16
    written, 12 more for color_std."""
    import importlib.util
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "rectify_bench.py")
    spec = importlib.util.spec_from_file_location("rectify_bench_for_test", path)
    rb = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(rb)
    assert rb.rectify_bytes() == 92 and rb.rectify_bytes(color_std=False) == 80
    assert rb.RADII == Q.RADII and rb.RUNS == 3


# ---- the rule
@pytest.mark.parametrize("case", Q.DESIGNED_CASES)
def test_designed_cases_hold_their_branches(case):
    ref, ids, state, params, expect = Q.designed_inputs(case)
    info = {}
    out, fragile = Q.step(ref, ids, state, np.float64, info=info, **params)
    assert not fragile.any()
    assert expect
    assert np.array_equal(info["m"], Q.count_m(ids, params.get("radius", 2)))
    assert np.array_equal(info["supported"], info["m"] >= params.get("min_taps", 5))
    assert np.array_equal(info["class"] == 1, info["moved"].any(-1)) and np.array_equal(info["class"] == 2, ~info["supported"])
    assert (info["e"][info["class"] != 1] == 0).all()
    c, M, n = (np.float64(state["color"][..., :3]), np.float64(state["moment2"][..., :3]), np.float64(state["moment2"][..., 3]))
    same = info["class"] != 1                              # classes 0 and 2 come out as they went in
    assert np.array_equal(out["color"][same], c[same]) and np.array_equal(out["moment2"][same], M[same])
    assert np.array_equal(out["n"][same], n[same])
    for name, (mask, *value) in expect.items():
        assert mask.any(), name
        v = np.asarray(value[0]) if value else None
        if v is not None and v.shape[:2] == mask.shape:
            v = v[mask]
        if name in ("m", "class"):
            assert np.array_equal(info[name][mask], np.broadcast_to(v, info[name][mask].shape)), name
        elif name == "color_is":
            assert np.array_equal(out["color"][mask], np.float64(v))
            assert (info["sigma"][mask] == 0).all() and np.array_equal(info["mu"][mask], np.float64(v))
        elif name == "color_is_mu":
            assert np.array_equal(out["color"][mask], info["mu"][mask])
        elif name == "passthrough":
            assert np.array_equal(out["color"][mask], c[mask]) and np.array_equal(out["moment2"][mask], M[mask])
            assert np.array_equal(out["n"][mask], n[mask])
        elif name == "n_near":
            assert (np.abs(out["n"][mask] - v) <= value[1]).all()
        elif name == "n_is":
            assert (out["n"][mask] == v).all()
        elif name == "short":
            std = out["color_std"][mask]
            assert np.array_equal((std == 1e3).all(-1), np.broadcast_to(v, std.shape[:1]))
            assert np.array_equal((std < 1e3).all(-1), ~np.broadcast_to(v, std.shape[:1]))
        else:
            raise AssertionError(name)
    for name in Q.OUTPUTS:
        assert np.isfinite(out[name]).all(), name
    if case == "step":             # the variance is kept, the mean shifted
        assert np.allclose(out["moment2"] - out["color"] ** 2, 0.125, rtol=0, atol=1e-12)
    if case.startswith("borders"):
        rad = params["radius"]
        w, h = Q.DESIGNED_SIZE
        for y, x in ((0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1)):
            assert info["m"][y, x] == (rad + 1) ** 2
        assert info["m"][0, w // 2] == info["m"][h - 1, w // 2] == (rad + 1) * (2 * rad + 1)
        assert info["m"][h // 2, 0] == info["m"][h // 2, w - 1] == (rad + 1) * (2 * rad + 1)
    if case == "miss":
        w, h = Q.DESIGNED_SIZE
        assert info["m"][h // 2, w // 2 - 1] == 3 * 5 and info["m"][h // 2, w // 2] == 3 * 5


def test_noise_free_reference():
    """With the fresh frame as the reference the rectified history is the new value in one step; with
    a noise-free history as the reference (sigma = 0) it equals that history exactly."""
    w, h = Q.DESIGNED_SIZE
    state = TG.random_state(w, h, 3)
    ids = np.zeros((h, w), np.int32)
    fast = np.zeros((h, w, 4), np.float32)
    fast[..., :3] = (0.75, 1.5, 0.125)
    out, fragile = Q.step(fast, ids, state, np.float64)
    assert not fragile.any() and np.array_equal(out["color"], np.float64(fast[..., :3]))


@pytest.mark.parametrize("own_id", (False, True), ids=["another_id", "own_id"])
def test_nan_in_the_reference(own_id):
    """A NaN at a tap of another id gives the bits of the run with it zeroed; a NaN at a tap of the
    pixel's own id changes no pixel further than `radius` away."""
    ref, zeroed, ids, state = Q.nan_ref_inputs(own_id)
    for dtype in (np.float32, np.float64):
        for rad in Q.RADII:
            a, _ = Q.step(ref, ids, state, dtype, radius=rad)
            b, _ = Q.step(zeroed, ids, state, dtype, radius=rad)
            ys, xs = np.mgrid[0:ids.shape[0], 0:ids.shape[1]]
            far = np.maximum(np.abs(ys - Q.NAN_AT[0]), np.abs(xs - Q.NAN_AT[1])) > rad
            mask = far if own_id else np.ones_like(far)
            assert far.any() and (own_id or ids[Q.NAN_AT] != ids[Q.NAN_AT[0], Q.NAN_AT[1] + 1])
            for name in Q.OUTPUTS:
                assert np.array_equal(a[name][mask], b[name][mask], equal_nan=False), (name, rad)
            if own_id:                                                # (the zero does change its neighbours)
                assert not np.array_equal(a["color"][~far], b["color"][~far])


def test_restatement_gap_and_fragile_share_on_the_gpu_cases():
    """The restatement's own f32 - f64 gap stays within the recorded constants (the GPU test's TOL
    is 16 x them), and no case of the GPU test has more than MAX_FRAGILE fragile pixels."""
    gap, gap_std, shares = Q.rendered_gap(SCENE_OF, make_camera, TG.cpu_planes, TG.cpu_colour)
    print(f"rendered: {gap:.3g} (color_std {gap_std:.3g}); fragile " + ", ".join(f"{k} {100 * v:.2f} %" for k, v in shares.items()))
    assert gap <= F32_F64_GAP and gap_std <= F32_F64_GAP_STD
    assert set(shares) == {label for label, *_ in Q.case_list()} and len(shares) == 30
    for label, s in shares.items():
        assert s <= Q.MAX_FRAGILE, label
    gap, gap_std, shares = Q.designed_gap()
    print(f"designed: {gap:.3g} (color_std {gap_std:.3g})")
    assert gap <= F32_F64_GAP_DESIGNED and gap_std <= F32_F64_GAP_STD_DESIGNED
    for label, s in shares.items():
        assert s <= Q.MAX_FRAGILE, label


def test_rendered_cases_reach_the_classes():
    """The rendered cases are not all one branch: at 67 x 45 classes 0 and 1 hold pixels at every
    radius, class 2 at radius 1 and 2."""
    args = Q.rendered_inputs(67, 45, 9, SCENE_OF, make_camera, TG.cpu_planes, TG.cpu_colour)
    for rad in Q.RADII:
        info = {}
        Q.step(*args, np.float64, info=info, ref_scale=Q.CUR_SCALE, radius=rad)
        share = np.bincount(info["class"].ravel(), minlength=3) / info["class"].size
        print(f"radius {rad}: classes {share}")
        assert (share[:2] > 0.02).all()                       # (60 pixels of either class)
        assert share[2] > 0 or rad == 3                       # (49 taps always hold 5 of a 67 x 45 view's ids)


# ---- what it is for, derivable
def test_purpose_on_a_noise_free_sequence():
    """40 frames of A, then frames of B, one id, zero motion. Without rectification the history
    follows at alpha_min = 0.05: after k frames of B the error is |A - B| 0.95^k. With rectification
    on the frame itself the error is 0 from the first frame of B on, and the history starts over:
    n = 1, 2, 3, ..."""
    gapAB = abs(Q.SEQ_A - Q.SEQ_B)
    plain = Q.derivable_sequence(False)
    for k, share in ((1, 0.95), (3, 0.857375), (4, 0.81450625)):
        assert plain[k - 1][0] / gapAB == pytest.approx(0.95 ** k, abs=1e-12)
        assert 0.95 ** k == pytest.approx(share, abs=1e-12)
        assert plain[k - 1][1] == Q.SEQ_BEFORE + k
    rect = Q.derivable_sequence(True)
    for k, (err, n) in enumerate(rect, 1):
        assert err <= 1e-12, k
        assert abs(n - k) <= Q.N_TOL, (k, n)
