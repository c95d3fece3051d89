#!/usr/bin/env python3
"""Time firefly suppression (lrt_firefly_device) on the headline frame, 1280x720, beside a fill of
its bytes and history rectification at radius 2 in the same process. Prints one JSON line. Reported,
nothing is gated on.

Method (tools/temporal_bench.py's `timed`): warm-up calls, then untimed calls until 25 ms of load
have passed, then >= 20 timed repetitions (default 40), each between two device events on the stream;
the median. The passes are timed alternately, twice each in one process (a, b, c, a, b, c), and both
medians of each are reported: their distance is the run-to-run spread a ratio has to exceed. The
input is one 1 spp pool-kernel frame of the default scene with its G-buffer's ids.
  firefly_ms[form]   one call; forms: r1, r2 (the default form: id, no optional output), r1_noid,
                     r2_noid, r1_all, r2_all (excess_out, class_out and info written), r1_excess_class
                     (the two planes, no info), r1_info (info alone: its zeroing on the stream, the
                     second barrier and the two atomics per workgroup)
  fill_ms            a plain device fill of firefly_bytes() per pixel (36 B: the default form)
  rectify_r2_ms      temporal_rectify_tensor at radius 2 in place on a state (tools/rectify_bench.py's form)
  classes            pixels per class of the default call (0 kept, 1 clamped, 2 unsupported, 3 not finite)
The quality leg (--quality), for the default scene and random_scene(1000, 1):
  class_share, luma_ratio   per class the share of pixels, and mean Y(out) / mean Y(in): the energy lost,
                            on a 4 spp frame
  raw_rel_mse, filtered_rel_mse   mean((out - ref)^2 / (ref^2 + 0.01)) over rgb against 1024 spp, of
                            that 4 spp frame and of the filtered one
  chain_rel_mse, chain_firefly_rel_mse   16 orbit steps of 1 spp -> step_gbuffer -> svgf_filter_tensor,
                            the last filtered frame against 1024 spp from the last camera, without and
                            with step_gbuffer(firefly={})
  adaptive                  DESIGN 7.14's experiment: a four-frame pilot's variance_out -> sample
                            budget -> counted render at 4 samples per pixel from frame0 = 4, against
                            uniform 4 spp, the pilot's frames unfiltered and filtered

  python tools/firefly_bench.py [--width W --height H --reps N --quality]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from temporal_bench import orbit_args, timed  # noqa: E402

POOL = 512          # LRT_F_POOL
GUIDES = ("normal", "world_pos", "albedo")
SPP, MIN_COUNT, MAX_COUNT, PILOT, STEPS, DTHETA = 4, 1, 32, 4, 16, 0.02


def firefly_bytes(ids=True, excess=False, cls=False):
    """Bytes per pixel one call must move: the quad read (16 B; its neighbours come from the tile), the
    id read (4 B), the quad written (16 B), plus excess_out (16 B) and class_out (4 B) where given."""
    return 16 + (4 if ids else 0) + 16 + (16 if excess else 0) + (4 if cls else 0)


def rel_mse(a, ref):
    return float(((a[..., :3] - ref[..., :3]) ** 2 / (ref[..., :3] ** 2 + 0.01)).mean())


def luma(t):
    return 0.2126 * t[..., 0] + 0.7152 * t[..., 1] + 0.0722 * t[..., 2]


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--height", type=int, default=720)
    ap.add_argument("--depth", type=int, default=8)
    ap.add_argument("--reps", type=int, default=40, help="timed repetitions (>= 20)")
    ap.add_argument("--quality", action="store_true", help="also report the quality leg")
    args = ap.parse_args(argv)
    if args.reps < 20:
        ap.error("--reps must be >= 20")

    import torch

    if not torch.cuda.is_available():
        sys.exit("firefly_bench: needs a GPU (there is no CPU path)")
    import learnraytracing_amd as lrt
    from learnraytracing_amd import _lib as L

    w, h, depth = args.width, args.height, args.depth
    npix = w * h
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    lrt.InitializeTest()
    try:
        s = torch.cuda.Stream(dev)
        cam = lrt.default_camera(w, h)

        def frame(camera, frame0, frames, flags=POOL):
            """The mean of `frames` fresh samples per pixel (a zeroed buffer, the lerp's factor undone)."""
            with torch.cuda.stream(s):
                buf = torch.zeros((h, w, 4), device=dev)
            lrt.render_tensor(lrt.Job(width=w, height=h, frame0=frame0, frames=frames, max_depth=depth, camera=camera,
                                      flags=flags), buf, rays, stream=s)
            if frame0:
                with torch.cuda.stream(s):
                    buf.mul_((frame0 + frames) / frames)
            return buf

        with torch.cuda.stream(s):
            rays = torch.zeros(1, dtype=torch.int64, device=dev)
            out, exc = torch.zeros((h, w, 4), device=dev), torch.zeros((h, w, 4), device=dev)
            cls = torch.zeros((h, w), dtype=torch.int32, device=dev)
            info = torch.zeros(2, dtype=torch.int32, device=dev)
            fill = torch.zeros(npix * firefly_bytes(), dtype=torch.uint8, device=dev)
            acc = lrt.TemporalAccumulator(w, h, dev)
        line = {"tool": "firefly_bench", "width": w, "height": h, "depth": depth, "reps": args.reps,
                "firefly_bytes": firefly_bytes(), "firefly_ms": {}, "firefly_ms_runs": {}}
        # a state of four accumulated frames (rectify's), and a fresh 1 spp frame with its ids
        for t in range(4):
            col = frame(cam, t, 1)
            planes = lrt.gbuffer_tensor(w, h, cam, out=acc.gbuffer_planes(), stream=s)
            acc.step_gbuffer(col, planes, stream=s)
        with torch.cuda.stream(s):
            state = {k: acc._states[acc._cur][k].clone() for k in ("color", "moment2", "color_std")}
            ids = planes["id"].clone()
        col = frame(cam, 4, 1)
        s.synchronize()

        def do_fill():
            with torch.cuda.stream(s):
                fill.fill_(1)

        passes = {"fill_ms": do_fill,
                  "rectify_r2_ms": lambda: lrt.temporal_rectify_tensor(col, ids, state, out=state, stream=s, radius=2)}
        for r in (1, 2):
            mt = dict(radius=r)
            passes[f"r{r}"] = lambda mt=mt: lrt.firefly_tensor(col, ids, out=out, stream=s, **mt)
            passes[f"r{r}_noid"] = lambda mt=mt: lrt.firefly_tensor(col, None, out=out, stream=s, **mt)
            passes[f"r{r}_all"] = lambda mt=mt: lrt.firefly_tensor(col, ids, out=out, excess_out=exc, class_out=cls,
                                                                   info=info, stream=s, **mt)
        # where r1_all's time goes: the two planes without the counts, and the counts alone
        passes["r1_excess_class"] = lambda: lrt.firefly_tensor(col, ids, out=out, excess_out=exc, class_out=cls, stream=s)
        passes["r1_info"] = lambda: lrt.firefly_tensor(col, ids, out=out, info=info, stream=s)
        runs = {name: [] for name in passes}
        for _ in range(2):                      # alternating, twice each
            for name, fn in passes.items():
                runs[name].append(round(timed(torch, s, fn, args.reps)["median"], 4))
        for name, v in runs.items():
            if name.endswith("_ms"):
                line[name], line[name + "_runs"] = min(v), v
            else:
                line["firefly_ms"][name], line["firefly_ms_runs"][name] = min(v), v
        line["firefly_over_fill"] = {k: round(v / line["fill_ms"], 3) for k, v in line["firefly_ms"].items()}
        line["firefly_over_rectify_r2"] = {k: round(v / line["rectify_r2_ms"], 3) for k, v in line["firefly_ms"].items()}
        line["firefly_gbytes_per_s"] = round(npix * firefly_bytes() / (line["firefly_ms"]["r1"] * 1e-3) / 1e9, 1)
        lrt.firefly_tensor(col, ids, out=out, class_out=cls, info=info, stream=s)
        s.synchronize()
        line["classes"] = torch.bincount(cls.ravel(), minlength=4)[:4].tolist()
        line["info"] = info.tolist()

        if args.quality:
            line["quality"] = {}
            scenes = {"default": lrt.default_scene(), "random1000": lrt.random_scene(1000, 1)}
            try:
                for label, (sph, mats) in scenes.items():
                    lrt.set_scene(sph, mats)
                    q = {"spheres": len(sph), "gt_spp": 1024}
                    ref = frame(cam, 0, 1024, flags=0)
                    raw = frame(cam, 0, SPP)
                    g = lrt.gbuffer_tensor(w, h, cam, id=True, stream=s)
                    res = lrt.firefly_tensor(raw, g["id"], class_out=True, stream=s)
                    s.synchronize()
                    share = torch.bincount(res["class"].ravel(), minlength=4)[:4].double() / npix
                    q["class_share"] = [round(float(v), 6) for v in share]
                    q["luma_ratio"] = round(float(luma(res["out"]).double().mean() / luma(raw).double().mean()), 5)
                    q["raw_rel_mse"], q["filtered_rel_mse"] = round(rel_mse(raw, ref), 5), round(rel_mse(res["out"], ref), 5)
                    # the orbit chain
                    for name, ff in (("chain_rel_mse", None), ("chain_firefly_rel_mse", {})):
                        a = lrt.TemporalAccumulator(w, h, dev)
                        for t in range(STEPS):
                            c = lrt.make_camera(*orbit_args((t - STEPS + 1) * DTHETA, w, h))
                            pc = lrt.make_camera(*orbit_args((t - STEPS) * DTHETA, w, h))
                            buf = frame(c, t, 1)
                            p = lrt.gbuffer_tensor(w, h, c, pc, out=a.gbuffer_planes(), stream=s)
                            a.step_gbuffer(buf, p, stream=s, firefly=ff)
                        st = a.state
                        flt = lrt.svgf_filter_tensor(st["color"], st["moment2"], {k: p[k] for k in GUIDES}, stream=s)
                        if name == "chain_rel_mse":
                            ref_last = frame(c, 0, 1024, flags=0)
                        s.synchronize()
                        q[name] = round(rel_mse(flt, ref_last), 5)
                    # DESIGN 7.14's experiment, the pilot's frames unfiltered and filtered
                    ad = {}
                    with torch.cuda.stream(s):
                        four = torch.full((h, w), SPP, dtype=torch.int32, device=dev)
                        uni = torch.zeros((h, w, 4), device=dev)
                    job = lrt.Job(width=w, height=h, frame0=PILOT, frames=SPP, max_depth=depth, camera=cam)
                    lrt.render_counts_tensor(job, uni, rays, four, SPP * npix, mean=True, stream=s)
                    s.synchronize()
                    ad["uniform_rel_mse"] = round(rel_mse(uni, ref), 5)
                    for name, ff in (("adaptive_rel_mse", None), ("adaptive_firefly_rel_mse", {})):
                        a = lrt.TemporalAccumulator(w, h, dev)
                        for t in range(PILOT):
                            buf = frame(cam, t, 1, flags=0)
                            p = lrt.gbuffer_tensor(w, h, cam, out=a.gbuffer_planes(), stream=s)
                            a.step_gbuffer(buf, p, stream=s, firefly=ff)
                        with torch.cuda.stream(s):
                            var, ada = torch.zeros((h, w, 4), device=dev), torch.zeros((h, w, 4), device=dev)
                            sinfo = torch.zeros(2, dtype=torch.int64, device=dev)
                        flt = lrt.svgf_filter_tensor(a.state["color"], a.state["moment2"], {k: p[k] for k in GUIDES},
                                                     variance_out=var, stream=s)
                        counts = lrt.sample_budget_tensor(var, MIN_COUNT, MAX_COUNT, SPP * npix, color=flt, stream=s)
                        job = lrt.Job(width=w, height=h, frame0=PILOT, frames=MAX_COUNT, max_depth=depth, camera=cam)
                        lrt.render_counts_tensor(job, ada, rays, counts, SPP * npix, mean=True, info=sinfo, stream=s)
                        s.synchronize()
                        ad[name] = round(rel_mse(ada, ref), 5)
                        ad[name.replace("rel_mse", "samples")] = int(sinfo[0].item())
                    q["adaptive"] = ad
                    line["quality"][label] = q
            finally:
                lrt.set_scene(*lrt.default_scene())
        line["version"] = L.lib().lrt_version().decode()
        print(json.dumps(line), flush=True)
    finally:
        lrt.ShutdownTest()
    return 0


if __name__ == "__main__":
    sys.exit(main())
