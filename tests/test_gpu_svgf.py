"""The variance-guided filter on the GPU (lrt_svgf_filter_device / lrt_svgf_filter_host,
learnraytracing_amd/csrc/lrt_svgf.hip) against its NumPy restatement (tests/svgf_ref.py), its buffer
contract (in place, alphas, inputs untouched, aliasing), determinism, stream scratch and stream
ordering behind TemporalAccumulator, and what it is for.

The filter is tolerance-checked, not bit-pinned (the reference has no such filter; the kernels may
contract and use the hardware exp). Bound: |got - f64| <= TOL * max(1, |f64|) at every pixel, for
colour and variance separately, TOL = 16 x the largest gap between the restatement's own f32 and
f64 runs over these same cases (`python tests/svgf_ref.py` measures it on the CPU; the variance
estimate M - C^2 cancels, so the gaps are larger than the denoiser's). No exclusions: the filter's
two decisions (n < min_history, |N|^2 >= 0.25) compare inputs, and no input lies near either
threshold (tests/test_svgf_cpu.py asserts it).
Measured on the GPU: at most 8.7e-7 (colour) and 4.2e-6 (variance) over the main table, 0.06 and
0.08 of its bounds; 3.4e-6 and 1.1e-5 over the edge table (albedo0 and fireflies), 0.06 and 0.05 of
its bounds."""
import numpy as np
import pytest

import denoise_ref as DR
import svgf_ref as R
import temporal_ref as TR

pytestmark = pytest.mark.gpu

# python tests/svgf_ref.py:
#   largest f32 - f64 gap over the main table (84 filter calls): colour 9.8e-07, variance 3.4e-06
#   largest f32 - f64 gap over the edge table (40 filter calls): colour 3.35e-06, variance 1.28e-05
F32_F64_GAP = (9.8e-7, 3.4e-6)            # colour, variance
F32_F64_GAP_EDGE = (3.35e-6, 1.28e-5)
TOL = tuple(16 * g for g in F32_F64_GAP)
TOL_EDGE = tuple(16 * g for g in F32_F64_GAP_EDGE)
CUR = ("normal", "world_pos", "albedo")
SENTINEL = 7.0


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _run_case(gpu, c):
    """One case through lrt_svgf_filter_host: (colour gap, variance gap or None), alphas checked."""
    color, m2, g = R.case_inputs(c)
    out = np.full_like(color, SENTINEL)
    var = np.full_like(color, SENTINEL) if c["variance"] else None
    assert gpu.svgf_filter_host(color, m2, g if g else None, out=out, variance_out=var, **c["params"]) is out
    want_c, want_v = R.svgf(color, m2, g, np.float64, **c["params"])
    assert (out[..., 3] == SENTINEL).all()
    assert np.isfinite(out[..., :3]).all(), R.case_label(c)
    gaps = [R.rel_gap(out[..., :3], want_c), None]
    if var is not None:
        assert (var[..., 3] == SENTINEL).all() and np.isfinite(var[..., :3]).all() and (var[..., :3] >= 0).all()
        gaps[1] = R.rel_gap(var[..., :3], want_v)
    return gaps, out, var


def _check(label, gaps, tol):
    print(f"{label}: colour gap {gaps[0]:.3g} ({gaps[0] / tol[0]:.3f} of the bound)" +
          (f", variance gap {gaps[1]:.3g} ({gaps[1] / tol[1]:.3f})" if gaps[1] is not None else ""))
    assert gaps[0] <= tol[0], f"{label}: colour {gaps[0]:.3g} > {tol[0]:.3g}"
    assert gaps[1] is None or gaps[1] <= tol[1], f"{label}: variance {gaps[1]:.3g} > {tol[1]:.3g}"


@pytest.mark.parametrize("w,h", R.SHAPES, ids=[f"{w}x{h}" for w, h in R.SHAPES])
def test_svgf_vs_restatement(gpu, w, h):
    """The main table: K in {1, 2, 5} x {all guides, none, normal only, no albedo} with variance_out,
    and without it at K = 1 and 5 (the colour is the same bits with and without)."""
    worst = [0.0, 0.0]
    with_var = {}
    for c in R.default_table():
        if (c["w"], c["h"]) != (w, h):
            continue
        gaps, out, var = _run_case(gpu, c)
        _check(R.case_label(c), gaps, TOL)
        worst = [max(worst[0], gaps[0]), max(worst[1], gaps[1] or 0.0)]
        key = (c["guides"], c["params"]["iterations"])
        if c["variance"]:
            with_var[key] = out
        else:
            assert np.array_equal(_bits(out), _bits(with_var[key])), R.case_label(c)
    print(f"{w}x{h}: largest gap colour {worst[0]:.3g} (bound {TOL[0]:.3g}), variance {worst[1]:.3g} (bound {TOL[1]:.3g})")


EDGE_SWEEPS = R.edge_sweeps()


@pytest.mark.parametrize("sweep", list(EDGE_SWEEPS))
def test_svgf_edges_vs_restatement(gpu, sweep):
    """The edge table: the shapes on and beside the 64-row group and the 64-column tile at the three
    ping-pong parities, min_history, other sigmas and floors, the input variants (zero variance,
    fireflies, non-finite alphas, a far origin, zero albedo, n = 1 and n = 40 everywhere) and one
    frame of more workgroups than the device holds at once. Every pixel, no exclusions."""
    worst = [0.0, 0.0]
    for c in EDGE_SWEEPS[sweep]:
        gaps, out, var = _run_case(gpu, c)
        _check(R.case_label(c), gaps, TOL_EDGE)
        worst = [max(worst[0], gaps[0]), max(worst[1], gaps[1] or 0.0)]
        if c["variant"] == "dirty_alpha":       # no alpha but moment2's is ever read
            color, m2, g = R.case_inputs(c)
            clean, cm2, cg = R.case_inputs(dict(c, variant=None))
            assert np.array_equal(_bits(clean[..., :3]), _bits(color[..., :3])) and np.array_equal(_bits(cm2), _bits(m2))
            again = gpu.svgf_filter_host(clean, cm2, cg, out=np.full_like(clean, SENTINEL), **c["params"])
            assert np.array_equal(_bits(again), _bits(out))
    print(f"{sweep}: largest gap colour {worst[0]:.3g} (bound {TOL_EDGE[0]:.3g}), "
          f"variance {worst[1]:.3g} (bound {TOL_EDGE[1]:.3g})")


@pytest.mark.parametrize("it", [1, 2, 5])
def test_svgf_buffer_contract(gpu, it):
    """In place = out of place bit for bit, the outputs' alphas survive, the inputs are untouched,
    host = device, two calls agree, and each aliasing case raises."""
    import torch
    from learnraytracing_amd import LrtError
    w, h = 67, 45
    color, m2, guides = R.synthetic_inputs(w, h)
    dev = torch.device("cuda:0")
    up = lambda a: torch.from_numpy(a).to(dev)   # noqa: E731
    tc, tm = up(color), up(m2)
    tg = {k: up(v) for k, v in guides.items()}
    out, var = (torch.full((h, w, 4), SENTINEL, device=dev) for _ in range(2))
    assert gpu.svgf_filter_tensor(tc, tm, tg, out=out, variance_out=var, iterations=it) is out
    out2, var2 = (torch.full((h, w, 4), SENTINEL, device=dev) for _ in range(2))
    gpu.svgf_filter_tensor(tc, tm, tg, out=out2, variance_out=var2, iterations=it)
    inplace, var3 = tc.clone(), torch.full((h, w, 4), SENTINEL, device=dev)
    assert gpu.svgf_filter_tensor(inplace, tm, tg, out=inplace, variance_out=var3, iterations=it) is inplace
    default_out = gpu.svgf_filter_tensor(tc, tm, tg, iterations=it)      # out defaults to a copy of color
    torch.cuda.synchronize()
    o, v, ip = out.cpu().numpy(), var.cpu().numpy(), inplace.cpu().numpy()
    assert np.array_equal(_bits(out2.cpu().numpy()), _bits(o)) and np.array_equal(_bits(var2.cpu().numpy()), _bits(v))
    assert np.array_equal(_bits(ip[..., :3]), _bits(o[..., :3]))        # in place = out of place, bit for bit
    assert np.array_equal(_bits(var3.cpu().numpy()), _bits(v))
    assert (o[..., 3] == SENTINEL).all() and (v[..., 3] == SENTINEL).all()
    assert np.array_equal(_bits(ip[..., 3]), _bits(color[..., 3]))
    d = default_out.cpu().numpy()
    assert np.array_equal(_bits(d[..., :3]), _bits(o[..., :3])) and np.array_equal(_bits(d[..., 3]), _bits(color[..., 3]))
    assert np.array_equal(_bits(tc.cpu().numpy()), _bits(color)) and np.array_equal(_bits(tm.cpu().numpy()), _bits(m2))
    for k in guides:
        assert np.array_equal(_bits(tg[k].cpu().numpy()), _bits(guides[k])), k
    # the host entry point: the same bits, the same contract
    hout, hvar = np.full((h, w, 4), SENTINEL, np.float32), np.full((h, w, 4), SENTINEL, np.float32)
    c0, m0, g0 = color.copy(), m2.copy(), {k: x.copy() for k, x in guides.items()}
    assert gpu.svgf_filter_host(color, m2, guides, out=hout, variance_out=hvar, iterations=it) is hout
    assert np.array_equal(_bits(hout), _bits(o)) and np.array_equal(_bits(hvar), _bits(v))
    assert np.array_equal(_bits(color), _bits(c0)) and np.array_equal(_bits(m2), _bits(m0))
    assert all(np.array_equal(_bits(guides[k]), _bits(g0[k])) for k in g0)
    hin = color.copy()
    gpu.svgf_filter_host(hin, m2, guides, out=hin, iterations=it)
    assert np.array_equal(_bits(hin), _bits(ip))
    # aliasing
    before = out.clone()
    for bad in (dict(out=tm), dict(out=tg["normal"]), dict(out=tg["world_pos"]), dict(out=tg["albedo"]),
                dict(out=out, variance_out=out), dict(out=out, variance_out=tc), dict(out=out, variance_out=tm),
                dict(out=out, variance_out=tg["albedo"]), dict(out=tc, variance_out=tc)):
        with pytest.raises(LrtError) as e:
            gpu.svgf_filter_tensor(tc, tm, tg, iterations=it, **bad)
        assert e.value.code == gpu._lib.LRT_E_INVALID
    flat = torch.zeros(2 * w * h * 4, device=dev)                       # a partial overlap of the two outputs
    with pytest.raises(LrtError):
        gpu.svgf_filter_tensor(tc, tm, tg, iterations=it, width=w, height=h, out=flat, variance_out=flat[8:])
    torch.cuda.synchronize()
    assert np.array_equal(_bits(out.cpu().numpy()), _bits(before.cpu().numpy()))   # a refused call wrote nothing


def test_svgf_scratch_grows_across_two_streams(gpu):
    """Two non-default streams with scratch of their own: on A 19x13, then 129x65 (its scratch has to
    grow), then 19x13 again, with other inputs enqueued on B between them, K = 1 (two scratch frames)
    and in-place calls among them; one synchronisation per stream at the end. Every result is
    lrt_svgf_filter_host's of the same inputs, bit for bit."""
    import torch
    dev = torch.device("cuda:0")
    A, B = torch.cuda.Stream(dev), torch.cuda.Stream(dev)
    plan = [(A, 19, 13, 0, 5, False), (B, 67, 45, 1, 5, False), (A, 129, 65, 0, 5, True), (B, 19, 13, 2, 1, True),
            (A, 19, 13, 3, 2, False), (B, 129, 65, 5, 4, False)]
    up = lambda a: torch.from_numpy(a).to(dev)   # noqa: E731
    staged = []
    for s, w, h, seed, it, inplace in plan:
        color, m2, guides = R.synthetic_inputs(w, h, seed=seed)
        tc = up(color)
        out = tc if inplace else torch.full((h, w, 4), SENTINEL, device=dev)
        staged.append((color, m2, guides, tc, up(m2), {k: up(v) for k, v in guides.items()}, out,
                       torch.full((h, w, 4), SENTINEL, device=dev)))
    torch.cuda.synchronize()                      # the uploads (default stream) are done before A and B start
    for (s, w, h, seed, it, inplace), (_, _, _, tc, tm, tg, out, var) in zip(plan, staged):
        assert gpu.svgf_filter_tensor(tc, tm, tg, out=out, variance_out=var, stream=s, iterations=it) is out
    A.synchronize()
    B.synchronize()
    for (s, w, h, seed, it, inplace), (color, m2, guides, _, _, _, out, var) in zip(plan, staged):
        hvar = np.full((h, w, 4), SENTINEL, np.float32)
        want = gpu.svgf_filter_host(color, m2, guides, variance_out=hvar, iterations=it)
        got = out.cpu().numpy()
        assert np.array_equal(_bits(got[..., :3]), _bits(want[..., :3])), (w, h, seed, it, inplace)
        assert np.array_equal(got[..., 3], color[..., 3]) if inplace else (got[..., 3] == SENTINEL).all()
        assert np.array_equal(_bits(var.cpu().numpy()), _bits(hvar)), (w, h, seed, it, inplace)


def _job(gpu, w, h, cam, frame0, frames=1):
    return gpu.Job(width=w, height=h, frame0=frame0, frames=frames, max_depth=TR.QUALITY["depth"], camera=cam)


def _render(gpu):
    def render(w, h, camera, frame0):
        buf = np.zeros((h, w, 4), np.float32)
        feats = {n: np.zeros((h, w, 4), np.float32) for n in CUR}
        gpu.render_host_features(_job(gpu, w, h, camera, frame0), buf, feats, -1)
        return buf, feats
    return render


def test_svgf_chains_behind_the_accumulator_on_one_stream(gpu):
    """render (features) -> TemporalAccumulator.step x 3 along the orbit -> svgf_filter_tensor on
    acc.state, on one non-default stream with nothing between them but the stream's order: the
    same chain through the host entry points, bit for bit."""
    import torch
    w, h = 160, 90
    cams = [gpu.make_camera(*TR.orbit_args(t, w, h)) for t in (-0.04, -0.02, 0.0)]
    render = _render(gpu)
    state = None
    for t, cam in enumerate(cams):
        color, cur = render(w, h, cam, t)
        state = gpu.temporal_accumulate_host(color, cur, state, cam, cams[max(t - 1, 0)], cur_scale=t + 1)
    hvar = np.zeros((h, w, 4), np.float32)
    want = gpu.svgf_filter_host(state["color"], state["moment2"], {n: state[n] for n in CUR}, variance_out=hvar)
    dev = torch.device("cuda:0")
    st = torch.cuda.Stream(dev)
    with torch.cuda.stream(st):
        acc = gpu.TemporalAccumulator(w, h, dev)
        rays = torch.zeros(1, dtype=torch.int64, device=dev)
        tvar = torch.zeros((h, w, 4), device=dev)
        for t, cam in enumerate(cams):
            tbuf = torch.zeros((h, w, 4), device=dev)
            tfe = {n: torch.zeros((h, w, 4), device=dev) for n in CUR}
            gpu.render_tensor_features(_job(gpu, w, h, cam, t), tbuf, rays, tfe, -1, stream=st)
            tcol, guides = acc.step(tbuf, tfe, cam, cur_scale=t + 1, stream=st)
        assert set(acc.state) == set(gpu._lib.TEMPORAL_STATE_NAMES) and acc.state["color"] is tcol
        tout = gpu.svgf_filter_tensor(acc.state["color"], acc.state["moment2"], guides, variance_out=tvar, stream=st)
        got = tout.to("cpu", non_blocking=False).numpy()
        gvar = tvar.to("cpu", non_blocking=False).numpy()
    st.synchronize()
    for n in gpu._lib.TEMPORAL_STATE_NAMES:
        assert np.array_equal(_bits(acc.state[n].cpu().numpy()[..., :3]), _bits(state[n][..., :3])), n
    assert np.array_equal(_bits(acc.state["moment2"].cpu().numpy()), _bits(state["moment2"]))
    assert np.array_equal(_bits(got[..., :3]), _bits(want[..., :3]))
    assert np.array_equal(_bits(gvar[..., :3]), _bits(hvar[..., :3]))
    short = state["moment2"][..., 3] < 4
    assert 0 < short.mean() <= 1                                          # the spatial estimate ran


@pytest.fixture(scope="module")
def ground_truth(gpu):
    q = TR.QUALITY
    cam = gpu.make_camera(*TR.orbit_args(0.0, q["w"], q["h"]))
    gt = np.zeros((q["h"], q["w"], 4), np.float32)
    gpu.render_host(gpu.Job(width=q["w"], height=q["h"], frames=q["gt_spp"], max_depth=q["depth"], camera=cam), gt)
    return gt


@pytest.mark.parametrize("dtheta", [0.02, 0.0, 0.08])
def test_svgf_quality_on_gpu(gpu, ground_truth, dtheta):
    """tests/test_svgf_cpu.py's bar, the whole way through the library: 16 steps of 1 spp with
    features through the v0 kernel, lrt_temporal_accumulate_host, lrt_svgf_filter_host, against 1024
    spp through render_host; the existing temporal -> lrt_denoise_host path beside it."""
    q = TR.QUALITY
    frames = TR.orbit_frames(_render(gpu), gpu.make_camera, q["w"], q["h"], q["steps"], dtheta)
    state, prev_cam = None, None
    for color, feats, cam, k in frames:
        state = gpu.temporal_accumulate_host(color, feats, state, cam, prev_cam, cur_scale=k)
        prev_cam = cam
    color, feats, _, k = frames[-1]
    single = color * np.float32(k)
    guides1 = {n: feats[n] * np.float32(k) for n in CUR}
    gt = ground_truth
    base = gpu.denoise_host(single, dict(guides1, color_std=np.full_like(single, TR.DEFAULTS["short_std"])))
    old = gpu.denoise_host(state["color"], {n: state[n] for n in gpu._lib.GUIDE_NAMES})
    new = gpu.svgf_filter_host(state["color"], state["moment2"], {n: state[n] for n in CUR})
    d0, d_old, d_new = DR.rel_mse(base, gt), DR.rel_mse(old, gt), DR.rel_mse(new, gt)
    print(f"step {dtheta}: filtered relMSE d0 {d0:.4g}; existing path {d_old:.4g} ({d_old / d0:.3f}x); "
          f"lrt_svgf {d_new:.4g} ({d_new / d0:.3f}x)")
    assert d_new <= TR.BAR_DENOISED * d0
