"""The denoiser on the GPU (lrt_denoise_device / lrt_denoise_host, learnraytracing_amd/csrc/
lrt_denoise.hip) against its NumPy restatement (tests/denoise_ref.py), its buffer contract
(in place, alpha, inputs untouched), determinism and stream ordering, the torch front end of
lrt_render_device_ex that feeds it, and what it is for: a 4 spp frame closer to the converged one.

The filter is tolerance-checked, not bit-pinned (the reference has no such filter; the kernel may
contract and uses the hardware exp). Bound: |got - f64| <= TOL * max(1, |f64|) at every pixel, TOL
= 16 x the largest gap between the restatement's own f32 and f64 runs over these same cases
(`python tests/denoise_ref.py` measures it on the CPU); the 16x allows for another exp and
another summation order. The edge table (tests/denoise_ref.py, edge_sweeps()) is judged by the same
rule with the gap measured over its own cases. Measured on the GPU: at most 7.6e-7 over the edge table
(0.05 of its bound); far_origin 6.0e-7 (4.98e-5, 3.1 x the bound, before world_pos was staged
relative to a per-workgroup anchor)."""
import numpy as np
import pytest

import denoise_ref as R

pytestmark = pytest.mark.gpu

F32_F64_GAP = 9.5e-7          # measured: 9.5e-07 (tests/denoise_ref.py, f32_f64_gap())
TOL = 16 * F32_F64_GAP
F32_F64_GAP_EDGE = 9.9e-7     # measured: 9.86e-07 (tests/denoise_ref.py, f32_f64_gap(edge_table()))
TOL_EDGE = 16 * F32_F64_GAP_EDGE


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize("w,h", R.SHAPES, ids=[f"{w}x{h}" for w, h in R.SHAPES])
def test_denoise_vs_restatement(gpu, w, h):
    color, guides = R.synthetic_inputs(w, h)
    worst = 0.0
    for it in R.ITERATIONS:
        for label, names in R.GUIDE_SETS.items():
            g = {k: guides[k] for k in names}
            got = gpu.denoise_host(color, g if g else None, iterations=it)
            want = R.atrous(color, g, np.float64, iterations=it)
            assert np.array_equal(got[..., 3], color[..., 3])          # alpha: out's own (a copy of color's)
            gap = R.rel_gap(got[..., :3], want)                         # every pixel
            worst = max(worst, gap)
            assert np.isfinite(got).all() and gap <= TOL, f"{w}x{h} iterations={it} guides={label}: {gap:.3g} > {TOL:.3g}"
    print(f"{w}x{h}: largest gap {worst:.3g} (bound {TOL:.3g})")


EDGE_SWEEPS = R.edge_sweeps()


@pytest.mark.parametrize("sweep", list(EDGE_SWEEPS))
def test_denoise_edges_vs_restatement(gpu, sweep):
    """The edge table: the shapes on and beside the 64-row group and the 64-column tile at the three
    ping-pong parities, every iteration count, single and leave-one-out guide sets, other sigmas
    and the input variants (far_origin among them, by the same bound), and one frame of more
    workgroups than the device holds at once. Every pixel, no exclusions."""
    worst = 0.0
    for c in EDGE_SWEEPS[sweep]:
        color, g = R.case_inputs(c)
        got = gpu.denoise_host(color, g, **c["params"])
        want = R.atrous(color, g, np.float64, **c["params"])
        assert np.array_equal(_bits(got[..., 3]), _bits(color[..., 3]))
        gap = R.rel_gap(got[..., :3], want)
        worst = max(worst, gap)
        print(f"{R.case_label(c)}: gap {gap:.3g} ({gap / TOL_EDGE:.3f} of the bound)")
        assert np.isfinite(got).all() and gap <= TOL_EDGE, f"{R.case_label(c)}: {gap:.3g} > {TOL_EDGE:.3g}"
        if c["variant"] == "dirty_alpha":       # a guide's alpha is never read
            clean, cg = R.case_inputs(dict(c, variant=None))
            assert np.array_equal(_bits(clean), _bits(color))
            assert np.array_equal(_bits(gpu.denoise_host(clean, cg, **c["params"])), _bits(got))
    print(f"{sweep}: largest gap {worst:.3g} (bound {TOL_EDGE:.3g})")


def test_denoise_scratch_grows_across_two_streams(gpu):
    """Two non-default streams with scratch of their own: on A 19x13, then 129x65 (its scratch has
    to grow), then 19x13 again, all at K = 5, with other inputs enqueued on B between them and a
    K = 1 in-place call (the copy path) on each; one synchronisation per stream at the end. Every
    result is lrt_denoise_host's of the same inputs, bit for bit."""
    import torch
    dev = torch.device("cuda:0")
    A, B = torch.cuda.Stream(dev), torch.cuda.Stream(dev)
    plan = [(A, 19, 13, 0, 5, False), (B, 67, 45, 1, 5, False), (A, 129, 65, 0, 5, False), (B, 19, 13, 2, 3, False),
            (B, 65, 8, 1, 1, True), (A, 19, 13, 3, 5, False), (A, 129, 65, 4, 1, True), (B, 129, 65, 5, 4, False)]
    up = lambda a: torch.from_numpy(a).to(dev)   # noqa: E731
    staged = []
    for s, w, h, seed, it, inplace in plan:
        color, guides = R.synthetic_inputs(w, h, seed=seed)
        tc = up(color)
        out = tc if inplace else torch.full((h, w, 4), 7.0, device=dev)    # 7: the alpha sentinel
        staged.append((color, guides, tc, {k: up(v) for k, v in guides.items()}, out))
    torch.cuda.synchronize()                      # the uploads (default stream) are done before A and B start
    for (s, w, h, seed, it, inplace), (_, _, tc, tg, out) in zip(plan, staged):
        assert gpu.denoise_tensor(tc, tg, out=out, stream=s, iterations=it) is out
    A.synchronize()
    B.synchronize()
    for (s, w, h, seed, it, inplace), (color, guides, _, _, out) in zip(plan, staged):
        want = gpu.denoise_host(color, guides, iterations=it)
        got = out.cpu().numpy()
        assert np.array_equal(_bits(got[..., :3]), _bits(want[..., :3])), (w, h, seed, it, inplace)
        assert np.array_equal(got[..., 3], color[..., 3]) if inplace else (got[..., 3] == 7.0).all()


@pytest.mark.parametrize("it", [1, 2, 5])
def test_denoise_in_place_alpha_inputs(gpu, it):
    import torch
    w, h = 67, 45
    color, guides = R.synthetic_inputs(w, h)
    dev = torch.device("cuda:0")
    tc = torch.from_numpy(color).to(dev)
    tg = {k: torch.from_numpy(v).to(dev) for k, v in guides.items()}
    out = torch.full((h, w, 4), 7.0, device=dev)                        # the alpha sentinel (and rgb to overwrite)
    gpu.denoise_tensor(tc, tg, out=out, iterations=it)
    inplace = tc.clone()
    assert gpu.denoise_tensor(inplace, tg, out=inplace, iterations=it) is inplace
    torch.cuda.synchronize()
    o, ip = out.cpu().numpy(), inplace.cpu().numpy()
    assert np.array_equal(_bits(ip[..., :3]), _bits(o[..., :3]))        # in place = out of place, bit for bit
    assert (o[..., 3] == 7.0).all()                                     # out's alpha survives
    assert np.array_equal(_bits(ip[..., 3]), _bits(color[..., 3]))
    assert np.array_equal(_bits(tc.cpu().numpy()), _bits(color))        # inputs untouched
    for k in guides:
        assert np.array_equal(_bits(tg[k].cpu().numpy()), _bits(guides[k])), k
    # the host entry point: the same bits, the same contract
    hout = np.full((h, w, 4), 7.0, np.float32)
    c0, g0 = color.copy(), {k: v.copy() for k, v in guides.items()}
    assert gpu.denoise_host(color, guides, out=hout, iterations=it) is hout
    assert np.array_equal(_bits(hout), _bits(o))
    assert np.array_equal(_bits(color), _bits(c0)) and all(np.array_equal(_bits(guides[k]), _bits(g0[k])) for k in g0)
    hin = color.copy()
    gpu.denoise_host(hin, guides, out=hin, iterations=it)
    assert np.array_equal(_bits(hin), _bits(ip))
    from learnraytracing_amd import LrtError
    with pytest.raises(LrtError):                                        # out may not be a guide
        gpu.denoise_tensor(tc, tg, out=tg["albedo"], iterations=it)


def _job(gpu, w, h, frames):
    return gpu.Job(width=w, height=h, frames=frames, max_depth=8)


def test_denoise_deterministic_and_stream_ordered(gpu):
    import torch
    w, h = 160, 90
    color, guides = R.synthetic_inputs(w, h)
    a = gpu.denoise_host(color, guides)
    b = gpu.denoise_host(color, guides)
    assert np.array_equal(_bits(a), _bits(b))
    # render -> denoise on one non-default stream, nothing between them but the stream's order
    buf = np.zeros((h, w, 4), np.float32)
    feats = {n: np.zeros((h, w, 4), np.float32) for n in gpu._lib.FEATURE_NAMES}
    rays = gpu.render_host_features(_job(gpu, w, h, 4), buf, feats, 4)
    want = gpu.denoise_host(buf, {n: feats[n] for n in gpu._lib.GUIDE_NAMES})
    dev = torch.device("cuda:0")
    s = torch.cuda.Stream(dev)
    with torch.cuda.stream(s):
        tbuf = torch.zeros((h, w, 4), device=dev)
        tfe = {n: torch.zeros((h, w, 4), device=dev) for n in gpu._lib.FEATURE_NAMES}
        trays = torch.zeros(1, dtype=torch.int64, device=dev)
        gpu.render_tensor_features(_job(gpu, w, h, 4), tbuf, trays, tfe, 4, stream=s)
        tout = gpu.denoise_tensor(tbuf, {n: tfe[n] for n in gpu._lib.GUIDE_NAMES}, stream=s)
        got = tout.to("cpu", non_blocking=False).numpy()
    s.synchronize()
    assert int(trays.item()) == rays
    assert np.array_equal(_bits(tbuf.cpu().numpy()), _bits(buf))
    assert np.array_equal(_bits(got), _bits(want))


def test_render_tensor_features_matches_host(gpu):
    import torch
    w, h, frames = 128, 72, 3
    names = gpu._lib.FEATURE_NAMES
    buf = np.zeros((h, w, 4), np.float32)
    feats = {n: np.zeros((h, w, 4), np.float32) for n in names}
    rays = gpu.render_host_features(_job(gpu, w, h, frames), buf, feats, 4)
    dev = torch.device("cuda:0")
    tbuf = torch.zeros((h, w, 4), device=dev)
    tfe = {n: torch.zeros((h, w, 4), device=dev) for n in names}
    trays = torch.zeros(1, dtype=torch.int64, device=dev)
    gpu.render_tensor_features(_job(gpu, w, h, frames), tbuf, trays, tfe, 4)
    torch.cuda.synchronize()
    assert gpu._lib.last_launch().get("feat") == "1"
    assert int(trays.item()) == rays and rays > 0
    assert np.array_equal(_bits(tbuf.cpu().numpy()), _bits(buf))
    for n in names:
        assert np.array_equal(_bits(tfe[n].cpu().numpy()), _bits(feats[n])), n
        assert feats[n][..., :3].any(), n
    from learnraytracing_amd import LrtError
    with pytest.raises(LrtError):
        gpu.render_tensor_features(_job(gpu, w, h, frames), tbuf, trays, {"depth": tbuf})


def test_denoise_improves_render(gpu):
    """tests/test_denoise_cpu.py's quality bars, the whole way on the GPU: 4 spp with features
    through the v0 kernel, filtered by lrt_denoise_host, against 1024 spp through render_host."""
    w, h = 160, 90
    noisy = np.zeros((h, w, 4), np.float32)
    feats = {n: np.zeros((h, w, 4), np.float32) for n in gpu._lib.FEATURE_NAMES}
    gpu.render_host_features(_job(gpu, w, h, 4), noisy, feats, 4)
    assert gpu._lib.last_launch().get("feat") == "1"
    gt = np.zeros((h, w, 4), np.float32)
    gpu.render_host(_job(gpu, w, h, 1024), gt)
    got = gpu.denoise_host(noisy, {n: feats[n] for n in gpu._lib.GUIDE_NAMES})
    m0, m1 = R.mse(noisy, gt), R.mse(got, gt)
    r0, r1 = R.rel_mse(noisy, gt), R.rel_mse(got, gt)
    print(f"MSE {m0:.4g} -> {m1:.4g} ({m1 / m0:.3f}x), relMSE {r0:.4g} -> {r1:.4g} ({r1 / r0:.4f}x)")
    assert m1 <= 0.5 * m0
    assert r1 <= 0.1 * r0
