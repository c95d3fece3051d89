"""Firefly restore on the GPU (lrt_firefly_restore_device / _host, firefly_restore_kernel of
learnraytracing_amd/csrc/lrt_firefly_restore.hip) against its NumPy restatement
(tests/firefly_restore_ref.py). EVERY comparison of an output is an equality of bits: generated
fields with NaN, Inf, the cap and the value above it, denormals, -0 and negatives in the excess at
sizes that cross the 32 x 8 tile, its R and 2R halos and images smaller than the window, at every
radius, with and without ids; the designed cases with their hand-written expectations; the host
entry, the device entry and in place; the library's own frames through firefly_host, where the
conservation identity is checked too; and the TemporalAccumulator front end."""
import ctypes

import numpy as np
import pytest

import firefly_ref as FR
import firefly_restore_ref as R

pytestmark = pytest.mark.gpu

SENTINEL = 7.0
GUARD = 64
POOL = 512   # LRT_F_POOL
bits = R.bits


def _same(got, want, label):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (label, got.shape, want.shape)
    bad = bits(got) != bits(want)
    assert not bad.any(), f"{label}: {int(bad.sum())} words differ, first at {np.argwhere(bad)[0]}"


@pytest.mark.parametrize("label,w,h,seed,with_id,radius", R.case_list(), ids=[c[0].replace(" ", "_") for c in R.case_list()])
def test_generated_fields_equal_the_restatement(gpu, label, w, h, seed, with_id, radius):
    color, excess, ids = R.wild(w, h, seed)
    ids = ids if with_id else None
    keep = color.copy(), excess.copy()
    got = gpu.firefly_restore_host(color, excess, ids, radius=radius)["out"]
    assert np.array_equal(bits(color), bits(keep[0])) and np.array_equal(bits(excess), bits(keep[1]))
    want = R.step(color, excess, ids, radius=radius)
    print(f"{label}: {int(want['e'].any(-1).sum())} live sources, {int((want['acc'] != 0).any(-1).sum())} pixels reached")
    _same(got, want["out"], label)


@pytest.mark.parametrize("case", R.DESIGNED_CASES)
def test_designed_cases(gpu, case):
    color, excess, ids, params, acc = R.designed_inputs(case)
    got = gpu.firefly_restore_host(color, excess, ids, **params)["out"]
    R.check_designed(case, color, got, acc)
    _same(got, R.step(color, excess, ids, **params)["out"], case)


@pytest.mark.parametrize("radius", (1, 2, 3, 4))
def test_host_device_and_in_place(gpu, radius):
    """33 x 9, with and without ids: the host entry, the device entry and both in place agree bit for
    bit with each other and the restatement; the guard band behind out stays; the inputs are
    unchanged when the call is not in place, and excess and id when it is."""
    import torch
    L = gpu._lib
    w, h = 33, 9
    n4 = w * h * 4
    color, excess, ids = R.wild(w, h, 60 + radius)
    color[..., 3] = SENTINEL
    dev = torch.device("cuda:0")
    tcolor, texcess, tids = (torch.from_numpy(a).to(dev) for a in (color, excess, ids))
    st = torch.cuda.Stream(dev)
    st.wait_stream(torch.cuda.current_stream(dev))
    for with_id in (True, False):
        i, ti = (ids, tids) if with_id else (None, None)
        want = R.step(color, excess, i, radius=radius)["out"]
        label = f"r{radius} id={with_id}"
        _same(gpu.firefly_restore_host(color, excess, i, radius=radius)["out"], want, "host " + label)
        hcol = color.copy()
        res = gpu.firefly_restore_host(hcol, excess, i, out=hcol, radius=radius)
        assert res["out"] is hcol
        _same(hcol, want, "host in place " + label)
        # the device entry into a guarded buffer, on a stream of its own
        out = torch.full((n4 + GUARD,), SENTINEL, device=dev)
        res = gpu.firefly_restore_tensor(tcolor, texcess, ti, out=out, stream=st, width=w, height=h, radius=radius)
        assert res["out"] is out
        st.synchronize()
        o = out.cpu().numpy()
        _same(o[:n4].reshape(h, w, 4), want, "device " + label)
        assert (o[n4:] == SENTINEL).all() and (o[3:n4:4] == SENTINEL).all()
        # in place, guarded
        work = torch.full((n4 + GUARD,), SENTINEL, device=dev)
        work[:n4] = tcolor.ravel()
        torch.cuda.synchronize()
        gpu.firefly_restore_tensor(work, texcess, ti, out=work, stream=st, width=w, height=h, radius=radius)
        st.synchronize()
        o = work.cpu().numpy()
        _same(o[:n4].reshape(h, w, 4), want, "device in place " + label)
        assert (o[n4:] == SENTINEL).all()
        # a new out when none is given
        res = gpu.firefly_restore_tensor(tcolor, texcess, ti, stream=st, radius=radius)
        st.synchronize()
        _same(res["out"].cpu().numpy(), want, "device, out allocated " + label)
    for t, a in ((tcolor, color), (texcess, excess), (tids, ids)):
        assert np.array_equal(bits(t.cpu().numpy()), bits(a))
    # the device entry point itself: NULL id, the NULL stream
    out = torch.full((n4 + GUARD,), SENTINEL, device=dev)
    d = gpu.firefly_restore_desc(w, h, radius=radius)
    torch.cuda.synchronize()
    assert L.lib().lrt_firefly_restore_device(ctypes.byref(d), tcolor.data_ptr(), texcess.data_ptr(), None,
                                              out.data_ptr(), None) == 0
    torch.cuda.synchronize()
    o = out.cpu().numpy()
    _same(o[:n4].reshape(h, w, 4), R.step(color, excess, None, radius=radius)["out"], "NULL id, NULL stream")
    assert (o[n4:] == SENTINEL).all()
    # a refused call writes nothing
    before = out.clone()
    for bad in (dict(out=texcess), dict(excess=out, out=out), dict(radius=5), dict(radius=0)):
        a = dict(color=tcolor, excess=texcess, id=tids, out=out, width=w, height=h, radius=radius)
        a.update(bad)
        with pytest.raises(gpu.LrtError) as e:
            gpu.firefly_restore_tensor(**a)
        assert e.value.code == L.LRT_E_INVALID, bad
    torch.cuda.synchronize()
    assert torch.equal(out, before) and np.array_equal(bits(texcess.cpu().numpy()), bits(excess))


def test_state_after_shutdown(gpu):
    L = gpu._lib
    color, excess, ids = R.wild(3, 2, 1)
    gpu.ShutdownTest()
    try:
        with pytest.raises(gpu.LrtError) as e:
            gpu.firefly_restore_host(color, excess, ids)
        assert e.value.code == L.LRT_E_STATE
    finally:
        gpu.InitializeTest()
    _same(gpu.firefly_restore_host(color, excess, ids)["out"], R.step(color, excess, ids)["out"], "after re-initialising")


@pytest.fixture(scope="module")
def rendered(gpu):
    """{(w, h, count): (colour, ids)}: the library's own 1 spp pool-kernel frame at depth 8 and
    gbuffer_host's ids, rendered once (the scene is set and restored here)."""
    out = {}
    try:
        for count in (9, 1000):
            gpu.set_scene(*(gpu.default_scene() if count == 9 else gpu.random_scene(1000, 1)))
            for w, h in ((19, 13), (65, 17)):
                cam = gpu.default_camera(w, h)
                buf = np.zeros((h, w, 4), np.float32)
                gpu.render_host(gpu.Job(width=w, height=h, frames=1, max_depth=8, camera=cam, flags=POOL), buf)
                out[(w, h, count)] = (buf, gpu.gbuffer_host(w, h, cam, id=True)["id"])
    finally:
        gpu.set_scene(*gpu.default_scene())
    return out


@pytest.mark.parametrize("w,h,count", [(19, 13, 9), (65, 17, 9), (19, 13, 1000), (65, 17, 1000)])
def test_rendered_input(gpu, rendered, w, h, count):
    """The library's own frames and ids through firefly_host(excess_out=True): bits against the
    restatement, the conservation bound on the finite pixels, and the restored sum strictly nearer
    the input's than the clamped one whenever a pixel was clamped."""
    frame, ids = rendered[(w, h, count)]
    assert np.isfinite(frame).all() and len(np.unique(ids)) >= 3
    ff = gpu.firefly_host(frame, ids, excess_out=True, info=True)
    _same(ff["excess"], FR.step(frame, ids)["excess"], "the clamp's excess")
    clamped = int(ff["info"][0])
    color, excess = ff["out"], ff["excess"]
    s = lambda a: float(a[..., :3].astype(np.float64).sum())   # noqa: E731
    for r in (1, 2, 3, 4):
        got = gpu.firefly_restore_host(color, excess, ids, radius=r)["out"]
        _same(got, R.step(color, excess, ids, radius=r)["out"], f"{w}x{h} {count} r{r}")
        fin = np.isfinite(frame[..., :3]).all(-1) & np.isfinite(got[..., :3]).all(-1)
        err, bound = R.conservation(color, excess, got, r, mask=fin)
        print(f"{w}x{h} {count} spheres r{r}: clamped {clamped}, finite {int(fin.sum())} of {w * h}, "
              f"|error| {err:.4g}, bound {bound:.4g}, sums in {s(frame):.6g} clamped {s(color):.6g} restored {s(got):.6g}")
        assert err <= bound
        if clamped >= 1:
            assert abs(s(got) - s(frame)) < abs(s(color) - s(frame))


def test_accumulator_front_end(gpu):
    """19 x 13, five steps: step_gbuffer(firefly={}, firefly_restore={"radius": 2}) leaves the state
    bit for bit what firefly_tensor, then firefly_restore_tensor, then the plain step_gbuffer give;
    firefly_restore=None is the step with firefly alone; the caller's colour is left as it is;
    firefly_restore without firefly, or with an unknown name, raises before the step runs."""
    import torch
    L = gpu._lib
    w, h, steps = 19, 13, 5
    dev = torch.device("cuda:0")
    cam = gpu.default_camera(w, h)
    names = ("fr", "manual", "fr_r4", "manual_r4", "ff_none", "ff")
    accs = {k: gpu.TemporalAccumulator(w, h, dev) for k in names}
    gen = torch.Generator(device=dev).manual_seed(9)
    clamped = 0
    for t in range(steps):
        color = torch.rand((h, w, 4), device=dev, generator=gen) + 0.05
        color[(3 + t) % h, (5 + 2 * t) % w, :3] = FR.SPIKE
        color[6, 7 + t, :3] = FR.SPIKE
        color[6, 8 + t, :3] = FR.SPIKE                                       # an adjacent pair
        keep = color.clone()
        planes = {k: gpu.gbuffer_tensor(w, h, cam, out=a.gbuffer_planes()) for k, a in accs.items()}
        accs["fr"].step_gbuffer(color, planes["fr"], firefly={}, firefly_restore={"radius": 2}, min_history=2)
        accs["fr_r4"].step_gbuffer(color, planes["fr_r4"], firefly=dict(radius=2), firefly_restore=dict(radius=4),
                                   rectify={}, min_history=2)
        accs["ff_none"].step_gbuffer(color, planes["ff_none"], firefly={}, firefly_restore=None, min_history=2)
        accs["ff"].step_gbuffer(color, planes["ff"], firefly={}, min_history=2)
        info = torch.zeros(2, dtype=torch.int32, device=dev)
        f = gpu.firefly_tensor(color, planes["manual"]["id"], excess_out=True, info=info)
        g = gpu.firefly_restore_tensor(f["out"], f["excess"], planes["manual"]["id"], out=f["out"], radius=2)
        accs["manual"].step_gbuffer(g["out"], planes["manual"], min_history=2)
        f4 = gpu.firefly_tensor(color, planes["manual_r4"]["id"], excess_out=True, radius=2)
        g4 = gpu.firefly_restore_tensor(f4["out"], f4["excess"], planes["manual_r4"]["id"], radius=4)
        accs["manual_r4"].step_gbuffer(g4["out"], planes["manual_r4"], rectify={}, min_history=2)
        torch.cuda.synchronize()
        clamped += int(info[0])
        assert torch.equal(color.view(torch.int32), keep.view(torch.int32))
        for a, b in (("fr", "manual"), ("fr_r4", "manual_r4"), ("ff_none", "ff")):
            for n in ("color", "moment2", "color_std"):
                x, y = (accs[k]._states[accs[k]._cur][n].cpu().numpy() for k in (a, b))
                assert np.array_equal(bits(x), bits(y)), (t, a, b, n)
    assert clamped > 0
    assert not torch.equal(accs["fr"].state["color"], accs["ff"].state["color"])
    assert not torch.equal(accs["fr"].state["color"], accs["fr_r4"].state["color"])
    before = {n: accs["fr"].state[n].clone() for n in ("color", "moment2")}
    for bad in (dict(firefly_restore={}), dict(firefly_restore={"radius": 2}), dict(firefly={}, firefly_restore=3),
                dict(firefly={}, firefly_restore=dict(rank=2))):
        with pytest.raises(gpu.LrtError) as e:                  # refused before the step runs
            accs["fr"].step_gbuffer(color, gpu.gbuffer_tensor(w, h, cam, out=accs["fr"].gbuffer_planes()), **bad)
        assert e.value.code == L.LRT_E_INVALID, bad
    torch.cuda.synchronize()
    assert all(torch.equal(accs["fr"].state[n], before[n]) for n in before)
