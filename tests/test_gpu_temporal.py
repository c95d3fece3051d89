"""Temporal reprojection and accumulation on the GPU (lrt_temporal_accumulate_device / _host,
learnraytracing_amd/csrc/lrt_temporal.hip) against its NumPy restatement (tests/temporal_ref.py),
its buffer contract (alphas, inputs untouched, no aliasing, optional buffers), determinism and
stream ordering, the TemporalAccumulator front end, and what it is for: an orbit's accumulated
frame closer to the converged one than a single frame.

The step is tolerance-checked, not bit-pinned (the reference has no such stage; the kernel may
contract). Bound: |got - f64| <= TOL * max(1, |f64|) at every pixel none of whose decisions lies
within 1e-4 of its threshold (the restatement's `fragile` mask; a flipped decision is another
result, not an error), TOL = 16 x the largest gap between the restatement's own f32 and f64 runs on
these same cases (`python tests/temporal_ref.py` measures it on the CPU). The gap is that large
because a reprojected position carries ~1e-5 px of f32 rounding, which the bilinear weights turn
into that share of the difference between neighbouring history values (random, of order 1, here).
Measured on the GPU: at most 0.061 of the bound (160x90), 8e-8 of it at 1x1. The designed plane
scenes (test_step_designed_cases) follow the same rule with the gap measured over themselves, a
tenth of the orbit's; measured on the GPU: at most 0.062 of that bound (`moments`)."""
import numpy as np
import pytest

import denoise_ref as DR
import temporal_ref as R

pytestmark = pytest.mark.gpu

F32_F64_GAP = 2.5e-4          # measured: 2.43e-04 (tests/temporal_ref.py, f32_f64_gap()), all outputs but color_std
F32_F64_GAP_STD = 1.6e-4      # measured: 1.53e-04, color_std (a square root of a cancelling difference)
TOL, TOL_STD = 16 * F32_F64_GAP, 16 * F32_F64_GAP_STD
MAX_FRAGILE = 0.02
# the designed plane scenes (tests/temporal_ref.py, designed_gap()): no rendered geometry, few fragile
# pixels, so the same rule gives a bound an order of magnitude tighter than the orbit's
F32_F64_GAP_DESIGNED = 2.5e-5       # measured: 2.47e-05, all outputs but color_std
F32_F64_GAP_STD_DESIGNED = 4.8e-5   # measured: 4.71e-05, color_std (`moments`: roots next to the variance clamp)
TOL_DESIGNED, TOL_STD_DESIGNED = 16 * F32_F64_GAP_DESIGNED, 16 * F32_F64_GAP_STD_DESIGNED
CUR = ("normal", "world_pos", "albedo")


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _job(gpu, w, h, camera, frame0, frames=1):
    return gpu.Job(width=w, height=h, frame0=frame0, frames=frames, max_depth=8, camera=camera)


def _render(gpu):
    def render(w, h, camera, frame0):
        """One fresh 1 spp frame and its features: sample frame0 into zeroed buffers."""
        buf = np.zeros((h, w, 4), np.float32)
        feats = {n: np.zeros((h, w, 4), np.float32) for n in CUR}
        gpu.render_host_features(_job(gpu, w, h, camera, frame0), buf, feats, -1)
        return buf, feats
    return render


def _outputs(state):
    """A library state as the restatement's outputs (rgb; n out of moment2's alpha)."""
    out = {k: v[..., :3] for k, v in state.items()}
    out["n"] = state["moment2"][..., 3]
    return out


def _tol(name):
    return TOL_STD if name == "color_std" else TOL


@pytest.mark.parametrize("w,h", R.SHAPES, ids=[f"{w}x{h}" for w, h in R.SHAPES])
def test_step_vs_restatement(gpu, w, h):
    render = _render(gpu)
    worst = 0.0
    for dt in R.DTHETAS:
        cam0, cam1 = (gpu.make_camera(*R.orbit_args(t, w, h)) for t in (-dt, 0.0))
        _, g0 = render(w, h, cam0, R.FRAME0)
        color, cur = render(w, h, cam1, R.FRAME0)
        prev = R.random_prev({k: g0[k] * np.float32(R.CUR_SCALE) for k in ("normal", "world_pos")}, 1000 * w + h)
        got = _outputs(gpu.temporal_accumulate_host(color, cur, prev, cam1, cam0, cur_scale=R.CUR_SCALE))
        want, fragile = R.step(color, cur, prev, cam1, cam0, np.float64, cur_scale=R.CUR_SCALE)
        share = float(fragile.mean())
        print(f"{w}x{h} step {dt}: fragile {100 * share:.2f} %, history kept at "
              f"{100 * float((want['n'] > 1.5).mean()):.0f} %")
        assert share <= MAX_FRAGILE
        if w * h <= 15:
            assert not fragile.any()            # these are asserted pixel by pixel, with no exclusions
        for name in R.OUTPUTS:
            assert np.isfinite(got[name]).all(), name
            gap = R.rel_gap(got[name], want[name], ~fragile)
            worst = max(worst, gap / _tol(name))
            assert gap <= _tol(name), f"{w}x{h} step {dt} {name}: {gap:.3g} > {_tol(name):.3g}"
    print(f"{w}x{h}: largest gap {worst:.3g} of its bound")


@pytest.mark.parametrize("case", R.DESIGNED_CASES)
def test_step_designed_cases(gpu, case):
    """Plane scenes and camera pairs built so that each branch of the step holds pixels (counted on
    the CPU by tests/test_temporal_cpu.py::test_designed_cases_cover_their_branches): every output
    against the f64 restatement on the non-fragile pixels, and n = 1 exactly wherever the f64
    decision is to reset."""
    worst = 0.0
    for run in R.designed_runs(case):
        color, cur, prev, cam, pcam = R.designed_inputs(run, gpu.make_camera)
        got = _outputs(gpu.temporal_accumulate_host(color, cur, prev, cam, pcam, **run["params"]))
        info = {}
        want, fragile = R.step(color, cur, prev, cam, pcam, np.float64, info=info, **run["params"])
        assert fragile.mean() <= MAX_FRAGILE
        reset = ~info["keep"] & ~fragile
        print(f"{run['label']}: fragile {100 * fragile.mean():.2f} %, history kept at {100 * info['keep'].mean():.0f} %")
        assert (got["n"][reset] == 1).all()
        if case in ("behind", "sideways"):
            k = np.float32(run["params"]["cur_scale"])
            assert reset.all() and np.array_equal(_bits(got["color"]), _bits(k * color[..., :3]))
            assert (got["color_std"] == np.float32(R.DEFAULTS["short_std"])).all()
        if case == "same":
            assert info["keep"].all() and (got["n"] > 1).all()
        for name in R.OUTPUTS:
            tol = TOL_STD_DESIGNED if name == "color_std" else TOL_DESIGNED
            assert np.isfinite(got[name]).all(), name
            gap = R.rel_gap(got[name], want[name], ~fragile)
            worst = max(worst, gap / tol)
            print(f"  {name}: gap {gap:.3g} ({gap / tol:.3f} of its bound)")
            assert gap <= tol, f"{run['label']} {name}: {gap:.3g} > {tol:.3g}"
    print(f"{case}: largest gap {worst:.3g} of its bound")


@pytest.fixture(scope="module")
def one_step(gpu):
    """67x45: the inputs of one step with history, and its result through the host entry point."""
    w, h = 67, 45
    render = _render(gpu)
    cam0, cam1 = (gpu.make_camera(*R.orbit_args(t, w, h)) for t in (-0.02, 0.0))
    _, g0 = render(w, h, cam0, R.FRAME0)
    color, cur = render(w, h, cam1, R.FRAME0)
    prev = R.random_prev({k: g0[k] * np.float32(R.CUR_SCALE) for k in ("normal", "world_pos")}, 42)
    out = {n: np.full((h, w, 4), 7.0, np.float32) for n in R.STATE_NAMES + ("color_std",)}   # the alpha sentinel
    keep = [a.copy() for a in (color, *cur.values(), *prev.values())]
    assert gpu.temporal_accumulate_host(color, cur, prev, cam1, cam0, out=out, cur_scale=R.CUR_SCALE) is out
    for a, b in zip((color, *cur.values(), *prev.values()), keep):       # inputs and prev untouched
        assert np.array_equal(_bits(a), _bits(b))
    return dict(w=w, h=h, cams=(cam0, cam1), color=color, cur=cur, prev=prev, out=out)


def test_buffer_contract(gpu, one_step):
    import torch
    from learnraytracing_amd import LrtError
    s = one_step
    w, h, (cam0, cam1), hout = s["w"], s["h"], s["cams"], s["out"]
    assert (hout["color"][..., 3] == 7.0).all() and (hout["color_std"][..., 3] == 7.0).all()   # these alphas stay
    assert not (hout["moment2"][..., 3] == 7.0).all() and (hout["moment2"][..., 3] >= 1.0).all()   # n
    dev = torch.device("cuda:0")
    up = lambda d: {k: torch.from_numpy(v).to(dev) for k, v in d.items()}   # noqa: E731
    tcolor, tcur, tprev = torch.from_numpy(s["color"]).to(dev), up(s["cur"]), up(s["prev"])
    tout = {n: torch.full((h, w, 4), 7.0, device=dev) for n in hout}
    kw = dict(cur_scale=R.CUR_SCALE)
    assert gpu.temporal_accumulate_tensor(tcolor, tcur, tprev, cam1, cam0, out=tout, **kw) is tout
    torch.cuda.synchronize()
    for n in hout:                                                    # host and tensor entry points: the same bits
        assert np.array_equal(_bits(tout[n].cpu().numpy()), _bits(hout[n])), n
    assert np.array_equal(_bits(tcolor.cpu().numpy()), _bits(s["color"]))            # inputs and prev untouched
    for k in tcur:
        assert np.array_equal(_bits(tcur[k].cpu().numpy()), _bits(s["cur"][k])), k
    for k in tprev:
        assert np.array_equal(_bits(tprev[k].cpu().numpy()), _bits(s["prev"][k])), k
    # albedo and color_std are optional, and leave the rest as it was
    small = {n: torch.full((h, w, 4), 7.0, device=dev) for n in R.STATE_NAMES[:4]}
    gpu.temporal_accumulate_tensor(tcolor, {k: tcur[k] for k in ("normal", "world_pos")}, tprev, cam1, cam0,
                                   out=small, **kw)
    torch.cuda.synchronize()
    for n in small:
        assert np.array_equal(_bits(small[n].cpu().numpy()), _bits(hout[n])), n
    fresh = gpu.temporal_accumulate_tensor(tcolor, tcur, tprev, cam1, cam0, **kw)     # buffers of its own
    torch.cuda.synchronize()
    assert set(fresh) == set(hout)
    for n in hout:
        assert np.array_equal(_bits(fresh[n][..., :3].cpu().numpy()), _bits(hout[n][..., :3])), n
    # every aliasing case raises: an output that is an input, a prev buffer or another output
    ins = [tcolor, *tcur.values(), *tprev.values()]
    for n in tout:
        for t in ins + [tout["moment2" if n != "moment2" else "normal"]]:
            with pytest.raises(LrtError):
                gpu.temporal_accumulate_tensor(tcolor, tcur, tprev, cam1, cam0, out=dict(tout, **{n: t}), **kw)
    torch.cuda.synchronize()
    for n in hout:                                                    # and a refused call wrote nothing
        assert np.array_equal(_bits(tout[n].cpu().numpy()), _bits(hout[n])), n


def test_deterministic_and_stream_ordered(gpu, one_step):
    import torch
    s = one_step
    cam0, cam1 = s["cams"]
    again = gpu.temporal_accumulate_host(s["color"], s["cur"], s["prev"], cam1, cam0, cur_scale=R.CUR_SCALE)
    for n in again:
        assert np.array_equal(_bits(again[n][..., :3]), _bits(s["out"][n][..., :3])), n
    # render -> accumulate, twice, -> denoise on one non-default stream, nothing between them but the
    # stream's order, against the host-staged chain
    w, h = 160, 90
    cams = [gpu.make_camera(*R.orbit_args(t, w, h)) for t in (-0.02, 0.0)]
    render = _render(gpu)
    state = None
    for t, cam in enumerate(cams):
        color, cur = render(w, h, cam, t)
        state = gpu.temporal_accumulate_host(color, cur, state, cam, cams[max(t - 1, 0)], cur_scale=t + 1)
    want = gpu.denoise_host(state["color"], {n: state[n] for n in gpu._lib.GUIDE_NAMES})
    dev = torch.device("cuda:0")
    st = torch.cuda.Stream(dev)
    with torch.cuda.stream(st):
        acc = gpu.TemporalAccumulator(w, h, dev)
        rays = torch.zeros(1, dtype=torch.int64, device=dev)
        for t, cam in enumerate(cams):
            tbuf = torch.zeros((h, w, 4), device=dev)
            tfe = {n: torch.zeros((h, w, 4), device=dev) for n in CUR}
            gpu.render_tensor_features(_job(gpu, w, h, cam, t), tbuf, rays, tfe, -1, stream=st)
            tcol, guides = acc.step(tbuf, tfe, cam, cur_scale=t + 1, stream=st)
        tout = gpu.denoise_tensor(tcol, guides, stream=st)
        got = tout.to("cpu", non_blocking=False).numpy()
    st.synchronize()
    assert set(guides) == set(gpu._lib.GUIDE_NAMES)
    for n in guides:
        assert np.array_equal(_bits(guides[n].cpu().numpy()[..., :3]), _bits(state[n][..., :3])), n
    assert np.array_equal(_bits(got[..., :3]), _bits(want[..., :3]))


def test_accumulator_static_camera(gpu):
    """TemporalAccumulator over 16 fresh 1 spp frames of one camera, alpha = 1 / n all the way:
    the plain 16 spp render where the history was kept at every step, and the restatement chained
    in f64, in which a decision flipped at one step stays flipped (measured: full history at 89.8 %
    of the pixels, gap to the plain render 4.2e-7, 98.94 % of the pixels within TOL of the chain)."""
    import torch
    w, h, steps = 160, 90, 16
    dev = torch.device("cuda:0")
    cam = gpu.make_camera(*R.orbit_args(0.0, w, h))
    acc = gpu.TemporalAccumulator(w, h, dev)
    rays = torch.zeros(1, dtype=torch.int64, device=dev)
    frames = []
    for t in range(steps):
        tbuf = torch.zeros((h, w, 4), device=dev)
        tfe = {n: torch.zeros((h, w, 4), device=dev) for n in CUR}
        gpu.render_tensor_features(_job(gpu, w, h, cam, t), tbuf, rays, tfe, -1)
        tcol, guides = acc.step(tbuf, tfe, cam, cur_scale=t + 1, alpha_min=1 / 64)
        frames.append((tbuf.cpu().numpy(), {n: v.cpu().numpy() for n, v in tfe.items()}, cam, float(t + 1)))
    torch.cuda.synchronize()
    got = _outputs({n: v.cpu().numpy() for n, v in acc._states[acc._cur].items()})
    plain = np.zeros((h, w, 4), np.float32)
    gpu.render_host(_job(gpu, w, h, cam, 0, frames=steps), plain)
    full = got["n"] == steps
    gap = R.rel_gap(got["color"], plain[..., :3], full)
    want = R.accumulate(frames, np.float64, alpha_min=1 / 64)
    good = np.ones((h, w), bool)
    for name in R.OUTPUTS:
        ref = np.float64(want[name])
        err = np.abs(got[name] - ref) / np.maximum(1.0, np.abs(ref))
        good &= (err if err.ndim == 2 else err.max(-1)) <= _tol(name)
    print(f"static camera: full history at {100 * full.mean():.1f} % of the pixels, gap to the plain render "
          f"{gap:.3g}; within TOL of the chained f64 restatement: {100 * good.mean():.2f} %")
    assert full.mean() >= 0.85
    assert gap <= 1e-5
    assert good.mean() >= 0.98
    acc.reset()                                   # and after a reset the next step starts over
    tcol, guides = acc.step(tbuf, tfe, cam, cur_scale=steps)
    torch.cuda.synchronize()
    assert np.array_equal(_bits(tcol.cpu().numpy()[..., :3]), _bits(frames[-1][0][..., :3] * np.float32(steps)))
    assert (guides["color_std"][..., :3] == 1e3).all()


@pytest.fixture(scope="module")
def ground_truth(gpu):
    q = R.QUALITY
    cam = gpu.make_camera(*R.orbit_args(0.0, q["w"], q["h"]))
    gt = np.zeros((q["h"], q["w"], 4), np.float32)
    gpu.render_host(gpu.Job(width=q["w"], height=q["h"], frames=q["gt_spp"], max_depth=q["depth"], camera=cam), gt)
    return gt


@pytest.mark.parametrize("dtheta", [0.02, 0.0, 0.08])
def test_quality_on_gpu(gpu, ground_truth, dtheta):
    """tests/test_temporal_cpu.py's three bars, the whole way through the library: 16 steps of 1 spp
    with features through the v0 kernel, lrt_temporal_accumulate_host, lrt_denoise_host, against
    1024 spp through render_host."""
    q = R.QUALITY
    frames = R.orbit_frames(_render(gpu), gpu.make_camera, q["w"], q["h"], q["steps"], dtheta)
    state, prev_cam = None, None
    for color, feats, cam, k in frames:
        state = gpu.temporal_accumulate_host(color, feats, state, cam, prev_cam, cur_scale=k)
        prev_cam = cam
    color, feats, _, k = frames[-1]
    single = color * np.float32(k)
    guides1 = {n: feats[n] * np.float32(k) for n in CUR}
    gt = ground_truth
    r0, r1 = DR.rel_mse(single, gt), DR.rel_mse(state["color"], gt)
    m0, m1 = DR.mse(single, gt), DR.mse(state["color"], gt)
    cand = gpu.denoise_host(state["color"], {n: state[n] for n in gpu._lib.GUIDE_NAMES})
    base = gpu.denoise_host(single, dict(guides1, color_std=np.full_like(single, R.DEFAULTS["short_std"])))
    d0, d1 = DR.rel_mse(base, gt), DR.rel_mse(cand, gt)
    print(f"step {dtheta}: relMSE {r0:.4g} -> {r1:.4g} ({r1 / r0:.3f}x), MSE {m0:.4g} -> {m1:.4g} "
          f"({m1 / m0:.3f}x), filtered relMSE {d0:.4g} -> {d1:.4g} ({d1 / d0:.3f}x)")
    assert r1 <= R.BAR_REL * r0
    assert m1 <= R.BAR_MSE * m0
    assert d1 <= R.BAR_DENOISED * d0
