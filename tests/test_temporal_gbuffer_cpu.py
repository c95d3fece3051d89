"""Temporal accumulation driven by the G-buffer, host side (no GPU): the C-ABI's validation
(lrt_temporal_accumulate_gbuffer_*), the Python front end's argument checks, and the rule itself --
its NumPy restatement (tests/temporal_gbuffer_ref.py): equal to the static restatement
(tests/temporal_ref.py) under identical cameras and an unmoved scene, every branch of the designed
cases populated, the restatement's own f32 - f64 gap and fragile share on the GPU test's cases."""
import ctypes
import os

import numpy as np
import pytest

import gbuffer_ref as G
import temporal_gbuffer_ref as T
import temporal_ref as R
from learnraytracing_amd import LrtError, _lib as L
from learnraytracing_amd import (default_scene, make_camera, random_scene, temporal_accumulate_gbuffer_host,
                                 temporal_gbuffer_desc)

# the restatement's own f32 - f64 gaps (`python tests/temporal_gbuffer_ref.py`), as
# tests/test_gpu_temporal_gbuffer.py records them
F32_F64_GAP, F32_F64_GAP_STD = 2.6e-7, 8e-7                       # measured: 2.52e-07, 7.87e-07
F32_F64_GAP_DESIGNED, F32_F64_GAP_STD_DESIGNED = 1.8e-7, 9e-7     # measured: 1.69e-07, 8.62e-07
SCENE_OF = T.scene_of(default_scene, random_scene)


def _gpu_present():
    import torch
    return torch.cuda.device_count() > 0


# ---- the C-ABI
def test_struct_and_defaults():
    assert ctypes.sizeof(L.TemporalGbufferDesc) == 40
    assert [getattr(L.TemporalGbufferDesc, f).offset for f in ("width", "min_history", "cur_scale", "short_std",
                                                               "reserved2")] == [0, 12, 16, 28, 36]
    d = temporal_gbuffer_desc(16, 9)
    t = L.TemporalDesc()
    cam = make_camera(*R.orbit_args(0.0, 16, 9))
    assert L.lib().lrt_temporal_default(16, 9, ctypes.byref(cam), None, ctypes.byref(t)) == 0
    for name in L.TEMPORAL_GBUFFER_PARAMS:                     # lrt_temporal_default's, where the parameter exists
        assert getattr(d, name) == getattr(t, name), name
    assert (d.width, d.height, d.flags, d.reserved, d.reserved2) == (16, 9, 0, 0, 0)
    assert (d.alpha_min, d.normal_min, d.min_history, d.short_std, d.cur_scale) == \
        (np.float32(0.05), np.float32(0.9), 4, 1e3, 1.0)
    assert temporal_gbuffer_desc(16, 9, min_history=2, normal_min=0.5).min_history == 2
    lib = L.lib()
    assert lib.lrt_temporal_gbuffer_default(16, 9, None) == L.LRT_E_INVALID
    assert lib.lrt_temporal_gbuffer_default(0, 9, ctypes.byref(d)) == L.LRT_E_INVALID
    with pytest.raises(LrtError):
        temporal_gbuffer_desc(16, 9, pos_tol=0.1)              # the step has no position test


def test_validation_before_device_use():
    """Every LRT_E_INVALID case, host and device entry points alike, with no device use; a valid
    call without lrt_initialize() is LRT_E_STATE."""
    lib = L.lib()
    w, h = 16, 9
    quads = [np.zeros((h, w, 4), np.float32) for _ in range(10)]
    words = [np.zeros(5 * w * h + 16, np.int32) for _ in range(2)]   # (an id plane and room for a frame behind it)
    ptr = lambda a: a.ctypes.data   # noqa: E731
    d = temporal_gbuffer_desc(w, h)

    def gb(normal, motion, idp):
        g = L.Gbuffer()
        g.normal, g.motion, g.id = normal, motion, idp
        return g

    def st(color, moment2):
        s = L.TemporalState()
        s.color, s.moment2 = color, moment2
        return s

    color = ptr(quads[0])
    cur, prev_g = gb(ptr(quads[1]), ptr(quads[2]), ptr(words[0])), gb(ptr(quads[3]), None, ptr(words[1]))
    prev, nxt, std = st(ptr(quads[4]), ptr(quads[5])), st(ptr(quads[6]), ptr(quads[7])), ptr(quads[8])

    def calls(dd=d, c=color, g=cur, pg=prev_g, p=prev, n=nxt, s=std):
        ref = lambda x: ctypes.byref(x) if x is not None else None   # noqa: E731
        return (lib.lrt_temporal_accumulate_gbuffer_host(ref(dd), c, ref(g), ref(pg), ref(p), ref(n), s),
                lib.lrt_temporal_accumulate_gbuffer_device(ref(dd), c, ref(g), ref(pg), ref(p), ref(n), s, None))

    inv = (L.LRT_E_INVALID, L.LRT_E_INVALID)
    # required pointers
    assert calls(dd=None) == inv
    assert calls(c=None) == inv
    assert calls(g=None) == inv
    assert calls(n=None) == inv
    for member in ("normal", "motion", "id"):
        bad = gb(cur.normal, cur.motion, cur.id)
        setattr(bad, member, None)
        assert calls(g=bad) == inv, member
    for member in ("normal", "id"):
        bad = gb(prev_g.normal, None, prev_g.id)
        setattr(bad, member, None)
        assert calls(pg=bad) == inv, member
    for member in ("color", "moment2"):
        for which in ("p", "n"):
            bad = st(*((prev if which == "p" else nxt).color, (prev if which == "p" else nxt).moment2))
            setattr(bad, member, None)
            assert calls(**{which: bad}) == inv, (which, member)
    # exactly one of prev and prev_g
    assert calls(p=None) == inv
    assert calls(pg=None) == inv
    assert "both" in lib.lrt_last_error().decode()
    # the parameter ranges
    for member, values in (("width", (0, -1)), ("height", (0,)), ("flags", (1,)), ("reserved", (1,)), ("reserved2", (1,)),
                           ("min_history", (0, -3)), ("cur_scale", (0.0, -1.0, np.nan, np.inf)),
                           ("alpha_min", (0.0, 1.5, np.nan)), ("normal_min", (-1.5, 1.5, np.nan)),
                           ("short_std", (0.0, -1.0, np.inf, np.nan))):
        for v in values:
            bad = L.TemporalGbufferDesc.from_buffer_copy(d)
            setattr(bad, member, v)
            assert calls(dd=bad) == inv, (member, v)
    bad = L.TemporalGbufferDesc.from_buffer_copy(d)
    bad.width, bad.height = 1 << 15, 1 << 15                      # width * height > INT_MAX / 4
    assert calls(dd=bad) == inv
    # no output on an input, a previous buffer or another output
    ins = [color, cur.normal, cur.motion, cur.id, prev_g.normal, prev_g.id, prev.color, prev.moment2]
    for a in ins:
        assert calls(n=st(a, nxt.moment2)) == inv
        assert calls(n=st(nxt.color, a)) == inv
        assert calls(s=a) == inv
    assert calls(n=st(nxt.color, nxt.color)) == inv
    assert calls(s=nxt.color) == inv
    assert calls(s=nxt.moment2) == inv
    assert calls(s=nxt.moment2 + 16) == inv                           # a partial overlap
    assert "alias" in lib.lrt_last_error().decode()
    # an id plane is width * height * 4 bytes: an output may start right behind it, not inside it
    behind = ptr(words[0]) + w * h * 4
    assert calls(s=behind - 4) == inv
    # a G-buffer overwritten in place is no history
    assert calls(pg=gb(cur.normal, None, prev_g.id)) == inv
    assert calls(pg=gb(prev_g.normal, None, cur.id)) == inv
    assert calls(pg=gb(prev_g.normal, None, cur.id + 4 * w)) == inv      # a partial overlap of the id planes
    assert calls(pg=gb(cur.normal + 16, None, prev_g.id)) == inv
    if os.environ.get("HIP_VISIBLE_DEVICES") == "" or not _gpu_present():
        state = (L.LRT_E_STATE, L.LRT_E_STATE)
        assert calls() == state
        assert calls(s=None) == state                                    # color_std is optional
        assert calls(p=None, pg=None) == state                           # no history
        assert calls(s=behind) == state                                  # right behind the id plane: no overlap
        assert calls(g=gb(cur.normal, cur.motion, cur.id), pg=gb(prev_g.normal, prev.color, prev_g.id)) == state


def test_front_end_argument_checks():
    w, h = 16, 9
    z = lambda: np.zeros((h, w, 4), np.float32)   # noqa: E731
    zi = lambda: np.zeros((h, w), np.int32)       # noqa: E731
    color, cur = z(), {"normal": z(), "motion": z(), "id": zi()}
    prev_g, prev = {"normal": z(), "id": zi()}, {"color": z(), "moment2": z()}

    def bad(**kw):
        a = dict(color=color, cur=cur, prev_g=prev_g, prev=prev)
        a.update(kw)
        with pytest.raises(LrtError) as e:
            temporal_accumulate_gbuffer_host(a.pop("color"), a.pop("cur"), a.pop("prev_g"), a.pop("prev"), **a)
        assert e.value.code == L.LRT_E_INVALID
        return str(e.value)

    assert "hold" in bad(cur={"normal": z(), "motion": z()})
    assert "int32" in bad(cur=dict(cur, id=np.zeros((h, w), np.float32)))
    assert "float32" in bad(cur=dict(cur, normal=np.zeros((h, w, 4), np.float64)))
    assert "unknown G-buffer plane" in bad(cur=dict(cur, colour=z()))
    assert "hold" in bad(prev_g={"normal": z()})
    assert "lacks" in bad(prev={"color": z()})
    assert "lacks" in bad(out={"color": z()})
    assert "unknown state buffer" in bad(out={"color": z(), "moment2": z(), "normal": z()})
    assert "unknown temporal parameter" in bad(pos_tol=0.1)
    assert ">=" in bad(cur=dict(cur, id=np.zeros((h - 1, w), np.int32)))
    assert "both" in bad(prev=None)                     # through the library
    assert "both" in bad(prev_g=None)
    assert "alias" in bad(out={"color": color, "moment2": z()})
    assert "alias" in bad(prev_g=dict(prev_g, id=cur["id"]))
    # a whole G-buffer and a whole state pass as they are: the rest is not read
    whole = dict(cur, world_pos=z(), albedo=z(), depth=np.zeros((h, w), np.float32))
    state = dict(prev, normal=z(), world_pos=z(), albedo=z(), color_std=z())
    if os.environ.get("HIP_VISIBLE_DEVICES") == "" or not _gpu_present():
        with pytest.raises(LrtError) as e:
            temporal_accumulate_gbuffer_host(color, whole, dict(prev_g, motion=z()), state)
        assert e.value.code == L.LRT_E_STATE


def test_accumulator_methods_exist():
    from learnraytracing_amd import TemporalAccumulator
    assert callable(TemporalAccumulator.step_gbuffer) and callable(TemporalAccumulator.gbuffer_planes)
    assert L.TEMPORAL_GBUFFER_PLANES == ("normal", "world_pos", "albedo", "motion", "id")


# ---- the rule
# Under identical cameras the static restatement projects each pixel-centre point back in f64 and
# lands on its own centre within the f32 rounding of the guide it read: a point X at distance t from
# the camera O (|O| = 3.6, t >= 1.5 in this view, so |X| / t <= (|O| + t) / t <= 3.4) is off by
# |X| 2^-24, which is |X| 2^-24 x 45 / (2 tan 30 deg x t) <= 3.4 x 6e-8 x 39 = 8e-6 px in the previous
# image. That weight bleeds the neighbours in: times their difference, n up to 19 apart, 1.5e-4.
STATIC_TOL = 1.5e-4   # (measured: 6.6e-07, printed below)


def test_equals_the_static_step_where_nothing_moves():
    """67 x 45, the default scene, identical cameras, no scene motion: color, moment2, n and std
    equal temporal_ref.step's on the same colours and guides in f64 at every pixel neither
    restatement marks fragile -- exactly in the decisions (kept, short history), within the bleed
    of the static projection's rounding in the values."""
    w, h = 67, 45
    spheres, mats = default_scene()
    cam, _ = G.camera_pair(make_camera, w, h)
    planes = T.ref_planes(w, h, cam, spheres, None, None)
    assert (planes["motion"][..., :2] == 0).all() and (planes["motion"][..., 3] == 1).all()
    color = T.cpu_colour(w, h, cam, G.sphere_array(spheres), mats, 0)
    prev = T.random_state(w, h, 5)
    guides = {k: planes[k] for k in ("normal", "world_pos")}
    i1, i2 = {}, {}
    got, f1 = T.step(color, planes, {k: planes[k] for k in ("normal", "id")}, prev, np.float64, info=i1)
    want, f2 = R.step(color, guides, dict(prev, **guides), cam, cam, np.float64, info=i2)
    ok = ~(f1 | f2)
    assert ok.mean() >= 1 - T.MAX_FRAGILE
    assert i1["keep"].all() and np.array_equal(i1["keep"][ok], i2["keep"][ok])
    assert np.array_equal(i1["short_history"][ok], i2["short_history"][ok])
    worst = {name: R.rel_gap(got[name], want[name], ok) for name in T.OUTPUTS}
    print("gbuffer step against the static step, nothing moved: " + ", ".join(f"{k} {v:.3g}" for k, v in worst.items()))
    for name, g in worst.items():
        assert g <= STATIC_TOL, f"{name}: {g:.3g}"
    # and with no bleed at all the two are the same numbers: a previous state that is constant
    flat = {"color": np.ones((h, w, 4), np.float32), "moment2": np.full((h, w, 4), 2, np.float32)}
    flat["moment2"][..., 3] = 7
    got, f1 = T.step(color, planes, {k: planes[k] for k in ("normal", "id")}, flat, np.float64)
    want, f2 = R.step(color, guides, dict(flat, **guides), cam, cam, np.float64)
    ok = ~(f1 | f2)
    for name in T.OUTPUTS:
        assert R.rel_gap(got[name], want[name], ok) <= 1e-12, name
    assert (got["n"] == 8).all()


@pytest.mark.parametrize("case", T.DESIGNED_CASES)
def test_designed_cases_hold_their_branches(case):
    color, cur, prev_g, prev, params, expect = T.designed_inputs(case)
    info = {}
    out, fragile = T.step(color, cur, prev_g, prev, np.float64, info=info, **params)
    assert not fragile.any()
    assert expect
    for name, (mask, value) in expect.items():
        assert mask.any(), name
        value = np.asarray(value)
        value = value[mask] if value.shape == mask.shape else value
        if name == "n_is_1":
            assert (out["n"][mask] == 1).all()
            C = np.float64(color[..., :3])
            assert np.array_equal(out["color"][mask], C[mask]) and np.array_equal(out["moment2"][mask], (C * C)[mask])
            assert (out["color_std"][mask] == 1e3).all()
        elif name == "n_prev":
            assert np.array_equal(out["n"][mask], np.float64(value) + 1)
        else:
            assert np.array_equal(info[name][mask], np.broadcast_to(value, info[name][mask].shape)), name
    for name in T.OUTPUTS:
        assert np.isfinite(out[name]).all(), name
    if case == "other_id":         # four taps of 1/4: sw = 3/4, 1/2 and nothing
        n3 = out["n"][2, 1]
        pn = np.float64(prev["moment2"][..., 3])
        assert n3 == pytest.approx((pn[2, 1] + pn[2, 2] + pn[3, 1]) / 3 + 1, rel=1e-12)
    if case == "min_history":
        assert (out["color_std"][:, :T.DESIGNED_SIZE[0] // 2] == 1e3).all()
        assert (out["color_std"][:, T.DESIGNED_SIZE[0] // 2:] < 1e3).all()


def test_restatement_gap_and_fragile_share_on_the_gpu_cases():
    """The restatement's own f32 - f64 gap stays within the recorded constants (the GPU test's TOL
    is 16 x them), and no case of the GPU test has more than MAX_FRAGILE fragile pixels."""
    gap, gap_std, shares = T.rendered_gap(SCENE_OF, make_camera, T.cpu_planes, T.cpu_colour)
    print(f"rendered: {gap:.3g} (color_std {gap_std:.3g}); fragile " + ", ".join(f"{k} {100 * v:.2f} %" for k, v in shares.items()))
    assert gap <= F32_F64_GAP and gap_std <= F32_F64_GAP_STD
    assert set(shares) == {label for label, *_ in T.case_list()}
    for label, s in shares.items():
        assert s <= T.MAX_FRAGILE, label
    gap, gap_std, shares = T.designed_gap()
    assert gap <= F32_F64_GAP_DESIGNED and gap_std <= F32_F64_GAP_STD_DESIGNED
    for label, s in shares.items():
        assert s <= T.MAX_FRAGILE, label


def test_rendered_cases_reach_the_branches():
    """The rendered cases are not all one branch: at 67 x 45 the moved spheres' pixels move by more
    than a quarter of a pixel, some taps are refused by id and some by normal, and most pixels keep
    their history."""
    args = T.rendered_case(67, 45, 9, SCENE_OF, make_camera, T.cpu_planes, T.cpu_colour)
    info = {}
    out, _ = T.step(*args, np.float64, info=info, cur_scale=T.CUR_SCALE)
    ids, mv = args[1]["id"], args[1]["motion"]
    for i, _ in T.MOVED:
        on = ids == i
        assert on.sum() >= 10 and (np.abs(mv[..., :2][on]) > 0.25).any(), i
    assert (ids == T.RESIZED).sum() >= 4
    assert info["rej_id"].sum() > 50 and info["keep"].mean() > 0.9 and (~info["keep"]).sum() > 0
    assert (out["n"] > 1).mean() > 0.9


def test_temporal_bench_constants_unchanged():
    """tools/temporal_bench.py: what its line always held is what it holds with --gbuffer present."""
    import importlib.util
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "temporal_bench.py")
    spec = importlib.util.spec_from_file_location("temporal_bench_for_gbuffer", path)
    tb = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tb)
    assert tb.MOVING_FIELDS == ("moving_step_ms", "moving_step_motion_ms", "moving_step_1000_ms")
    assert tb.step_bytes() == 216 and tb.step_bytes(albedo=False) == 184 and tb.step_bytes(color_std=False) == 204
    assert tb.GBUFFER_FIELDS == ("gbuffer_step_ms", "gbuffer_step_1000_ms", "gbuffer_pass_ms")
    assert tb.gbuffer_step_bytes() == 144
    assert "--gbuffer" in tb.__doc__
