"""The chain pass, host side (no GPU): the C-ABI's validation (lrt_gbuffer_chain_*), which fires before
any device use, the NumPy restatement's (tests/gbuffer_chain_ref.py) f32 - f64 gaps held to the
values tests/test_gpu_gbuffer_chain.py derives its tolerances from, the designed cases' branches, the
two identities against gbuffer_ref, and the key formula on id sequences written out by hand."""
import ctypes
import os

import numpy as np
import pytest

import gbuffer_chain_ref as C
import gbuffer_ref as G
import temporal_gbuffer_ref as TG
from learnraytracing_amd import LrtError, _lib as L
from learnraytracing_amd import (default_camera, default_scene, gbuffer_chain_desc, gbuffer_chain_host, make_camera,
                                 random_scene)

# the restatement's own f32 - f64 gaps off the fragile mask (`python tests/gbuffer_chain_ref.py`), as
# tests/test_gpu_gbuffer_chain.py records them
F32_F64_GAP = 4.5e-3                             # measured: 4.41e-03 (world_pos at 67 x 45, a reflection that meets the ground far away)
F32_F64_GAP_COUNT = {17: 1.1e-4, 1000: 3.1e-3}   # measured: 1.09e-04, 3.04e-03 (HitSphere's cancellation on r = 0.05)
F32_F64_GAP_DESIGNED = 3.1e-5                    # measured: 3.07e-05 (sixteen total reflections inside the glass sphere)
MAX_FRAGILE = 0.02


def _gpu_present():
    import torch
    return torch.cuda.device_count() > 0


SHAPE_CASES = C.shape_cases(default_scene, make_camera)
COUNT_CASES = C.count_cases(default_scene, random_scene, make_camera)


def test_f32_f64_gap_within_its_record():
    """The gaps the GPU test's tolerances are 16 x of; the fragile share (at most 0.1 % on the
    rendered cases, none where w h <= 15) and no key, id or bounce count that differs between the f32
    and the f64 run, on or off the mask."""
    for label, kw in SHAPE_CASES + COUNT_CASES:
        gap, report = C.f32_f64_gap([(label, kw)])
        share, differ, differ_ok, hist = report[label]
        bound = F32_F64_GAP_COUNT.get(len(kw["spheres"]), F32_F64_GAP)
        print(f"{label}: gap {gap:.3g} (recorded {bound:.3g}), fragile {100 * share:.2f} %, differ {differ}, followed {hist}")
        assert gap <= bound, label
        assert share <= 0.001 and differ == 0 and differ_ok == 0, label
        if kw["w"] * kw["h"] <= 15:
            assert share == 0
    for name in C.DESIGNED:
        gap, report = C.f32_f64_gap([(name, C.designed_case(name, make_camera))])
        assert gap <= F32_F64_GAP_DESIGNED and report[name][0] <= MAX_FRAGILE and report[name][1] == 0, name


def test_default_scene_walks_chains():
    """What the GPU test relies on: chains of two and more followed surfaces at 67 x 45, up to four at
    160 x 90; the default roughness_max follows spheres 3, 4, 5 (and the glass, 7), not sphere 6."""
    by_label = dict(SHAPE_CASES)
    out, _ = C.chain(dtype=np.float32, **by_label["67x45"])
    assert ((out["bounces"] & 0xFF) >= 2).sum() >= 100
    out, _ = C.chain(dtype=np.float32, **by_label["160x90"])
    assert np.bincount(out["bounces"].ravel()).tolist() == [11930, 1636, 770, 62, 2]
    first, _ = G.gbuffer(160, 90, by_label["160x90"]["camera"], by_label["160x90"]["spheres"],
                         G.albedo_array(by_label["160x90"]["materials"]), motion=False, dtype=np.float32)
    followed = out["bounces"] > 0
    assert set(np.unique(first["id"][followed])) == {3, 4, 5, 7}
    assert (first["id"] == 6).sum() > 50 and not followed[first["id"] == 6].any()
    chained = out["key"] >= 0x40000000
    assert np.array_equal(chained, followed) and np.array_equal(out["key"][~followed], first["id"][~followed])


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_identities_in_the_restatement(dtype):
    """max_bounces = 0 is gbuffer_ref's G-buffer everywhere, and any max_bounces is at the pixels
    whose first hit is not delta: the same arrays, since the restatement shares its first segment."""
    for label, kw in (SHAPE_CASES[2], SHAPE_CASES[3], COUNT_CASES[1]):
        first, _ = G.gbuffer(kw["w"], kw["h"], kw["camera"], kw["spheres"], G.albedo_array(kw["materials"]),
                             motion=False, dtype=dtype)
        zero, _ = C.chain(dtype=dtype, **dict(kw, max_bounces=0))
        full, _ = C.chain(dtype=dtype, **kw)
        assert (zero["bounces"] & 0xFF == 0).all()
        assert np.array_equal(zero["bounces"] != 0, full["bounces"] != 0), label   # the delta first hits
        for out, where in ((zero, np.ones_like(first["id"], bool)), (full, full["bounces"] == 0)):
            assert np.array_equal(out["key"][where], first["id"][where]) and np.array_equal(out["id"][where], first["id"][where])
            for plane in G.GUIDES + ("depth",):
                assert np.array_equal(out[plane][where], first[plane][where]), (label, plane)


def test_designed_cases_hold_their_branches():
    out = {name: C.chain(dtype=np.float64, **C.designed_case(name, make_camera)) for name in C.DESIGNED}
    tol = 16 * F32_F64_GAP_DESIGNED
    tint, red = np.float64(np.float32(C._TINT)), np.float64(np.float32(C._RED))
    # head-on mirror: one reflection, back past the camera onto the sphere behind it
    m, fragile = out["mirror"]
    assert not fragile.any() and m["bounces"][0, 0] == 1 and m["id"][0, 0] == 1 and m["key"][0, 0] == C.path_key([0, 1])
    assert np.abs(m["world_pos"][0, 0] - (0, 0, 5)).max() <= tol and abs(m["depth"][0, 0] - (2.5 + 4.5)) <= tol
    assert np.abs(m["normal"][0, 0] - (0, 0, -1)).max() <= tol
    assert np.abs(m["albedo"][0, 0] - tint * red).max() <= tol
    # head-on glass: in and out along the axis, T = 1
    g, fragile = out["glass"]
    assert not fragile.any() and g["bounces"][0, 0] == 2 and g["id"][0, 0] == 1 and g["key"][0, 0] == C.path_key([0, 0, 1])
    assert np.abs(g["world_pos"][0, 0] - (0, 0, -2)).max() <= tol and abs(g["depth"][0, 0] - (2.5 + 1 + 1.5)) <= tol
    assert np.array_equal(g["albedo"][0, 0], red)
    # inside the glass sphere: refracted out after one surface, or totally reflected for ever
    for name, maxb in (("inside6", 6), ("inside16", 16)):
        o, fragile = out[name]
        assert fragile.mean() <= MAX_FRAGILE
        unresolved = o["bounces"] == (maxb | C.UNRESOLVED)
        assert (o["bounces"] == 1).sum() == 101 and unresolved.sum() == 146 and unresolved.sum() + 101 == o["id"].size
        assert (o["id"][unresolved] == 0).all() and (o["id"][~unresolved] != 0).all()
        assert (o["key"][unresolved] == C.path_key([0] * (maxb + 1))).all()
    assert not out["inside6"][1].any()
    assert np.array_equal(out["inside6"][0]["bounces"] > 0xFF, out["inside16"][0]["bounces"] > 0xFF)
    assert np.array_equal(out["inside6"][0]["id"], out["inside16"][0]["id"])
    # two facing mirrors: the axis alone never escapes
    f, fragile = out["facing"]
    assert not fragile.any() and f["bounces"].shape == (3, 5)
    unresolved = f["bounces"] > 0xFF
    assert unresolved.sum() == 1 and unresolved[1, 2] and f["bounces"][1, 2] == (16 | C.UNRESOLVED)
    assert f["key"][1, 2] == C.path_key([0, 1] * 8 + [0])
    assert (f["id"][~unresolved] == -1).all() and (f["world_pos"][~unresolved] == 0).all()
    assert np.isposinf(f["depth"][~unresolved]).all()
    n = f["bounces"][~unresolved]                      # the sky through n mirrors: the tint to the nth
    assert np.abs(f["albedo"][~unresolved] - tint[None, :] ** n[:, None]).max() <= tol
    # roughness_max is a threshold with <=
    le, gt = out["rough_le"][0], out["rough_gt"][0]
    assert le["bounces"][0, 0] == 1 and le["id"][0, 0] == 1 and gt["bounces"][0, 0] == 0 and gt["id"][0, 0] == 0
    assert gt["key"][0, 0] == 0 and np.array_equal(gt["albedo"][0, 0], tint)
    # guide_scale: the three guides and nothing else
    kw = C.designed_case("inside6", make_camera)
    k, _ = C.chain(dtype=np.float64, guide_scale=0.25, **kw)
    for plane in C.NAMES:
        want = out["inside6"][0][plane]
        assert np.array_equal(k[plane], 0.25 * want if plane in C.GUIDES else want), plane


def test_key_formula_by_hand():
    """h = h 0x9E3779B1 + (id + 1), h ^= h >> 15 in uint32, per id after the first; the constants below
    were worked out with a desk calculator's integers, not with path_key."""
    assert C.path_key([-1]) == -1 and C.path_key([5]) == 5 and C.path_key([0]) == 0
    # [0, 1]: h = 0 * M + 2 = 2, 2 >> 15 = 0
    assert C.path_key([0, 1]) == 0x40000002
    # [0, -1]: h = 0 + 0 = 0: a mirror (sphere 0) that shows the sky
    assert C.path_key([0, -1]) == 0x40000000
    # [3, -1]: h = 3 M mod 2^32 = 0xDAA66D13; h >> 15 = 0x1B54C; h = 0xDAA7D85F; & 0x3FFFFFFF = 0x1AA7D85F
    assert C.path_key([3, -1]) == 0x5AA7D85F
    # [3, 0]: h = 0xDAA66D14; h >> 15 = 0x1B54C; h = 0xDAA7D858
    assert C.path_key([3, 0]) == 0x5AA7D858
    # [1, 2, 3]: h = M + 3 = 0x9E3779B4, ^ 0x13C6E = 0x9E3645DA; then h M + 4 (mod 2^32), ^ h >> 15
    h = (0x9E3645DA * 0x9E3779B1 + 4) % (1 << 32)
    assert C.path_key([1, 2, 3]) == 0x40000000 | ((h ^ (h >> 15)) & 0x3FFFFFFF)
    # order matters, every key has bit 30 and not bit 31, and none is a plain id
    keys = [C.path_key(s) for s in ([0, 1], [1, 0], [0, 1, 0], [0, 0, 1], [4095, 4095], [4095, -1], [7, 7, 7, 7, 7])]
    assert len(set(keys)) == len(keys) and all(0x40000000 <= k < 0x80000000 for k in keys)
    # the restatement's uint32 arrays give the same keys as the Python integers
    for name, seq in (("mirror", [0, 1]), ("glass", [0, 0, 1])):
        for T in (np.float32, np.float64):
            out, _ = C.chain(dtype=T, **C.designed_case(name, make_camera))
            assert out["key"].dtype == np.int32 and out["key"][0, 0] == C.path_key(seq)


def test_key_in_the_restated_temporal_step():
    """The head-on mirror at 37 x 21, the sphere behind the camera moved aside between two frames:
    the first-hit ids do not change, the keys change inside the mirror, and temporal_gbuffer_ref
    drops the history exactly there."""
    w, h = C.TEMPORAL_SIZE
    kw = C.designed_case("mirror", make_camera, size=(w, h))
    moved = dict(kw, spheres=np.float32(C.TEMPORAL_MOVED))
    a, _ = C.chain(dtype=np.float32, **kw)
    b, _ = C.chain(dtype=np.float32, **moved)
    first = TG.ref_planes(w, h, kw["camera"], kw["spheres"])
    assert np.array_equal(first["id"], TG.ref_planes(w, h, kw["camera"], moved["spheres"])["id"])
    changed = a["key"] != b["key"]
    # (a convex mirror of r 0.5 shows the sphere small: the changed set is a pixel or a few)
    assert changed.any() and (first["id"][changed] == 0).all() and (first["id"] == 0).sum() > changed.sum()
    rng = np.random.default_rng(5)
    colours = [TG.quad(rng.uniform(0.05, 2.0, (h, w, 3))) for _ in range(2)]
    for ids0, ids1, want in ((first["id"], first["id"], np.full((h, w), 2.0)), (a["key"], b["key"], np.where(changed, 1.0, 2.0))):
        s0, _ = TG.step(colours[0], dict(first, id=ids0), None, None)
        s1, _ = TG.step(colours[1], dict(first, id=ids1), {"normal": first["normal"], "id": ids0}, TG.as_state(s0))
        assert np.array_equal(s1["n"], want)


# ---- the C-ABI
def test_struct_layouts():
    assert ctypes.sizeof(L.GbufferChainDesc) == 16 + 88 + 16 == 120
    assert L.GbufferChainDesc.camera.offset == 16 and L.GbufferChainDesc.max_bounces.offset == 104
    assert ctypes.sizeof(L.GbufferChain) == 7 * ctypes.sizeof(ctypes.c_void_p)
    assert [f[0] for f in L.GbufferChain._fields_] == ["normal", "world_pos", "albedo", "key", "id", "bounces", "depth"]
    assert set(L.GBUFFER_CHAIN_NAMES) == set(C.NAMES) and L.CHAIN_UNRESOLVED == C.UNRESOLVED
    d = gbuffer_chain_desc(16, 9, default_camera(16, 9))
    assert (d.width, d.height, d.flags, d.reserved, d.reserved2) == (16, 9, 0, 0, 0)
    assert (d.max_bounces, d.roughness_max, d.guide_scale) == (4, 0.25, 1.0)
    assert bytes(d.camera) == bytes(default_camera(16, 9))
    d = gbuffer_chain_desc(16, 9, default_camera(16, 9), max_bounces=7, roughness_max=0.5, guide_scale=0.5)
    assert (d.max_bounces, d.roughness_max, d.guide_scale) == (7, 0.5, 0.5)
    with pytest.raises(LrtError):
        gbuffer_chain_desc(0, 9, default_camera(16, 9))
    with pytest.raises(LrtError):
        gbuffer_chain_desc(16, 9, None)


def test_validation_before_device_use():
    """Every invalid argument is LRT_E_INVALID before any device use, host and device entry points
    alike; a valid call without lrt_initialize() is LRT_E_STATE."""
    lib = L.lib()
    w, h = 16, 9
    cam = default_camera(w, h)
    rgba = [np.zeros((h, w, 4), np.float32) for _ in range(3)]
    ints = [np.zeros((h, w), np.int32) for _ in range(3)]
    depth = np.zeros((h, w), np.float32)
    ptr = lambda a: a.ctypes.data   # noqa: E731
    d = L.GbufferChainDesc()
    assert lib.lrt_gbuffer_chain_default(w, h, ctypes.byref(cam), ctypes.byref(d)) == 0
    assert lib.lrt_gbuffer_chain_default(w, h, None, ctypes.byref(d)) == L.LRT_E_INVALID
    assert lib.lrt_gbuffer_chain_default(w, h, ctypes.byref(cam), None) == L.LRT_E_INVALID
    assert lib.lrt_gbuffer_chain_default(0, h, ctypes.byref(cam), ctypes.byref(d)) == L.LRT_E_INVALID

    def planes(**kw):
        g = L.GbufferChain()
        g.normal, g.world_pos, g.albedo = (ptr(b) for b in rgba)
        g.key, g.id, g.bounces = (ptr(b) for b in ints)
        g.depth = ptr(depth)
        for k, v in kw.items():
            setattr(g, k, v)
        return g

    def desc(**kw):
        dd = L.GbufferChainDesc.from_buffer_copy(d)
        for k, v in kw.items():
            setattr(dd, k, v)
        return dd

    def calls(dd, g):
        ref = lambda x: ctypes.byref(x) if x is not None else None   # noqa: E731
        return (lib.lrt_gbuffer_chain_host(ref(dd), ref(g)), lib.lrt_gbuffer_chain_device(ref(dd), ref(g), None))

    inv = (L.LRT_E_INVALID, L.LRT_E_INVALID)
    assert calls(None, planes()) == inv
    assert calls(d, None) == inv
    assert calls(d, L.GbufferChain()) == inv                                     # all seven planes NULL
    for kw in (dict(width=0), dict(height=0), dict(width=-3), dict(width=1 << 15, height=1 << 15),
               dict(flags=1), dict(reserved=1), dict(reserved2=1)):
        assert calls(desc(**kw), planes()) == inv, kw
    for kw in (dict(max_bounces=-1), dict(max_bounces=L.CHAIN_MAX_BOUNCES + 1)):
        assert calls(desc(**kw), planes()) == inv, kw
    assert "max_bounces" in lib.lrt_last_error().decode()
    for v in (-0.5, float("nan"), float("inf")):
        assert calls(desc(roughness_max=v), planes()) == inv, v
    assert "roughness_max" in lib.lrt_last_error().decode()
    for v in (0.0, -1.0, float("nan"), float("inf")):
        assert calls(desc(guide_scale=v), planes()) == inv, v
    assert "guide_scale" in lib.lrt_last_error().decode()
    # any two planes overlapping, by address range (the int and depth planes are a quarter as long)
    names = [f[0] for f in L.GbufferChain._fields_]
    for i, a in enumerate(names):
        for b in names[i + 1:]:
            assert calls(d, planes(**{b: getattr(planes(), a)})) == inv, (a, b)
    assert calls(d, planes(world_pos=ptr(rgba[0]) + 16)) == inv                  # a partial overlap
    assert calls(d, planes(depth=ptr(rgba[2]) + 16 * w * h - 4)) == inv          # the last word of albedo
    assert calls(d, planes(bounces=ptr(ints[0]) + 4 * w * h - 4)) == inv         # the last word of key
    assert "alias" in lib.lrt_last_error().decode()
    if os.environ.get("HIP_VISIBLE_DEVICES") == "" or not _gpu_present():
        st = (L.LRT_E_STATE, L.LRT_E_STATE)
        assert calls(d, planes()) == st
        for name in names:                                                       # every member is optional
            assert calls(d, planes(**{name: None})) == st, name
            only = L.GbufferChain()
            setattr(only, name, getattr(planes(), name))
            assert calls(d, only) == st, name
        for kw in (dict(max_bounces=0), dict(max_bounces=L.CHAIN_MAX_BOUNCES), dict(roughness_max=0.0),
                   dict(width=4, height=2)):
            assert calls(desc(**kw), planes()) == st, kw
        # adjacent is not overlapping: key and bounces as the two halves of one array (the word after a
        # separate array may belong to any other plane's array)
        pair = np.zeros((2, h, w), np.int32)
        assert calls(d, planes(key=ptr(pair), bounces=ptr(pair) + 4 * w * h)) == st
        assert calls(d, planes(key=ptr(pair), bounces=ptr(pair) + 4 * w * h - 4)) == inv


def test_front_end_argument_checks():
    w, h = 16, 9
    cam = default_camera(w, h)
    for bad in (dict(out={"keys": np.zeros((h, w), np.int32)}),                  # an unknown plane
                dict(motion=True),                                               # there is no motion plane
                dict(out={"normal": np.zeros((h, w, 4), np.float64)}),
                dict(out={"key": np.zeros((h, w), np.float32)}),
                dict(out={"bounces": np.zeros((h, w), np.int64)}),
                dict(out={"depth": np.zeros((h, w - 1), np.float32)}),
                dict(out={"normal": np.zeros((h, w, 4), np.float32)[:, ::2]}),
                dict(out={}),
                dict(max_bounces=17), dict(roughness_max=-1.0), dict(guide_scale=0.0)):
        with pytest.raises(LrtError) as e:
            gbuffer_chain_host(w, h, cam, **bad)
        assert e.value.code == L.LRT_E_INVALID, bad
