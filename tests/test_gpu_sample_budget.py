"""The per-pixel sample budget on the GPU (lrt_sample_budget_device / _host,
learnraytracing_amd/csrc/lrt_sample_budget.hip): counts and info EQUAL the NumPy restatement
(tests/sample_budget_ref.py) -- f32 with no contraction, then exact integers -- on random fields
with NaN, Inf, negatives, zeros and denormals, the designed cases, and the variance_out of a
rendered frame; the device form equals the host form and two runs are identical."""
import numpy as np
import pytest

import sample_budget_ref as R

pytestmark = pytest.mark.gpu

SIZES = [(19, 13), (67, 45)]      # one partial block; several blocks with a partial last one


def _check(gpu, v, lo, hi, total, color=None, label="", **params):
    counts, info = gpu.sample_budget_host(v, lo, hi, total, color=color, **params)
    want, winfo = R.budget(v, lo, hi, total, color=color, **params)
    assert counts.dtype == np.int32 and counts.shape == want.shape
    bad = int((counts != want).sum())
    assert bad == 0, f"{label}: {bad} counts differ, first at {np.argwhere(counts != want)[0]}"
    assert info == winfo, f"{label}: info {info} != {winfo}"
    return counts, info


@pytest.mark.parametrize("w,h", SIZES, ids=["19x13", "67x45"])
@pytest.mark.parametrize("passes", [1, 2, 4])
def test_random_fields_equal_the_restatement(gpu, w, h, passes):
    L = gpu._lib
    npix = w * h
    for k, (lo, hi, spp) in enumerate([(1, 8, 3), (0, 32, 4), (2, L.COUNT_MAX, 40)]):
        v, c = R.random_field(w, h, 10 * k + passes), R.random_color(w, h, 10 * k + passes)
        for color in (None, c):
            for flags in (0, L.SB_STD):
                counts, info = _check(gpu, v, lo, hi, spp * npix, color=color, passes=passes, flags=flags,
                                      label=f"{w}x{h} case {k} passes {passes} color {color is not None} flags {flags}")
                assert counts.min() >= lo and counts.max() <= hi and info[0] <= spp * npix
                assert len(np.unique(counts)) >= 3
    # other parameters
    v, c = R.random_field(w, h, 77), R.random_color(w, h, 77, nasty=False)
    _check(gpu, v, 1, 64, 6 * npix, color=c, passes=passes, luma_floor=0.5, weight_max=16384.0, label="params")
    _check(gpu, v, 1, 64, 6 * npix, passes=passes, weight_max=0.125, label="small weight_max")


@pytest.mark.parametrize("w,h", SIZES, ids=["19x13", "67x45"])
def test_designed_cases_equal_the_restatement(gpu, w, h):
    npix = w * h
    zero = np.zeros((h, w, 4), np.float32)
    counts, info = _check(gpu, zero, 1, 8, npix + 2 * npix + 5, label="zero variance")
    assert (counts == 3).all() and info == (3 * npix, 0)
    hot = np.full((h, w, 4), 1e-6, np.float32)
    hot[h // 2, w // 3, :3] = 1e4
    one, i1 = _check(gpu, hot, 1, 16, 3 * npix, passes=1, label="hot pixel, one pass")
    two, i2 = _check(gpu, hot, 1, 16, 3 * npix, passes=2, label="hot pixel, two passes")
    assert one[h // 2, w // 3] == 16 == two[h // 2, w // 3]
    assert i1[0] == npix + 15 and i2[0] > i1[0] and two.min() >= 2      # pass 2 hands the surplus on
    v = R.random_field(w, h, 5)
    counts, info = _check(gpu, v, 2, 9, 2 * npix, passes=4, label="budget of the minimum")
    assert (counts == 2).all()
    counts, info = _check(gpu, v, 5, 5, 5 * npix + 999, passes=3, label="min_count == max_count")
    assert (counts == 5).all() and info == (5 * npix, 0)
    counts, info = _check(gpu, v, 0, 0, 0, label="nothing to give")
    assert (counts == 0).all()
    bad = np.zeros((h, w, 4), np.float32)
    bad[..., 0] = np.resize(np.array([np.nan, np.inf, -np.inf, -1.0, 0.0], np.float32), (h, w))
    counts, info = _check(gpu, bad, 1, 8, 4 * npix, label="NaN, Inf, negative: q = 0 everywhere")
    assert info[1] == 0 and (counts == 4).all()
    sat = np.full((h, w, 4), 1e12, np.float32)
    sat[0, 0, :3] = 1e20
    counts, info = _check(gpu, sat, 1, 4096, 5 * npix, passes=1, label="weight_max saturates")
    assert info[1] == npix * 256 * 65536 and (counts == 5).all()
    # the largest sums the ABI admits: q = 2^30 everywhere, E near 2^31
    _check(gpu, sat, 0, 4096, 2 ** 31 - 1, passes=2, weight_max=16384.0, label="largest product")


def test_svgf_variance_of_a_rendered_frame(gpu):
    """67 x 45: four 1 spp steps through the accumulator, the filtered variance, the budget from it
    (relative to the filtered colour): the tensor form on a stream of its own equals the host form and
    the restatement, and the counts follow the noise."""
    import torch
    w, h = 67, 45
    dev = torch.device("cuda:0")
    cam = gpu.default_camera(w, h)
    acc = gpu.TemporalAccumulator(w, h, dev)
    rays = torch.zeros(1, dtype=torch.int64, device=dev)
    for t in range(4):
        buf = torch.zeros((h, w, 4), device=dev)
        gpu.render_tensor(gpu.Job(width=w, height=h, frame0=t, frames=1, camera=cam), buf, rays)
        planes = gpu.gbuffer_tensor(w, h, cam, out=acc.gbuffer_planes())
        acc.step_gbuffer(buf, planes, cur_scale=float(t + 1))
    var = torch.zeros((h, w, 4), device=dev)
    guides = {k: planes[k] for k in ("normal", "world_pos", "albedo")}
    out = gpu.svgf_filter_tensor(acc.state["color"], acc.state["moment2"], guides, variance_out=var)
    st = torch.cuda.Stream(dev)
    st.wait_stream(torch.cuda.current_stream(dev))
    info = torch.zeros(2, dtype=torch.int64, device=dev)
    counts = gpu.sample_budget_tensor(var, 1, 32, 4 * w * h, color=out, info=info, stream=st)
    again = gpu.sample_budget_tensor(var, 1, 32, 4 * w * h, color=out, stream=st)
    st.synchronize()
    hv, hc = var.cpu().numpy(), out.cpu().numpy()
    assert np.isfinite(hv[..., :3]).all() and (hv[..., :3] > 0).any()
    want, winfo = R.budget(hv, 1, 32, 4 * w * h, color=hc)
    got = counts.cpu().numpy()
    assert got.shape == (h, w) and np.array_equal(got, want) and tuple(info.cpu().tolist()) == winfo
    assert np.array_equal(again.cpu().numpy(), got)                      # two runs are identical
    hcounts, hinfo = gpu.sample_budget_host(hv, 1, 32, 4 * w * h, color=hc)
    assert np.array_equal(hcounts, got) and hinfo == winfo               # device form == host form
    assert got.min() >= 1 and got.max() > got.min() and winfo[0] <= 4 * w * h       # the counts follow the noise


def test_front_end_defaults_and_flat_buffers(gpu):
    import torch
    w, h = 19, 13
    v = R.random_field(w, h, 3)
    want, winfo = R.budget(v, 1, 8, 3 * w * h)
    counts = np.full(w * h + 5, -7, np.int32)
    got, info = gpu.sample_budget_host(v.ravel(), 1, 8, 3 * w * h, counts=counts, width=w, height=h)
    assert got is counts and np.array_equal(counts[:w * h].reshape(h, w), want) and (counts[w * h:] == -7).all()
    tv = torch.from_numpy(v).cuda()
    tc = gpu.sample_budget_tensor(tv, 1, 8, 3 * w * h)
    assert tc.dtype == torch.int32 and tuple(tc.shape) == (h, w) and np.array_equal(tc.cpu().numpy(), want)
    with pytest.raises(gpu.LrtError):
        gpu.sample_budget_tensor(tv, 1, 8, 3 * w * h, counts=torch.zeros((h, w), dtype=torch.int64, device="cuda"))
    with pytest.raises(gpu.LrtError):
        gpu.sample_budget_tensor(tv, 1, 8, 3 * w * h, info=torch.zeros(1, dtype=torch.int64, device="cuda"))
