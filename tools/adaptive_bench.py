#!/usr/bin/env python3
"""Time adaptive sampling (lrt_sample_budget_device, lrt_render_counts_device) on the headline
frame, 1280x720 from the default camera at depth 8, for the default scene and random_scene(1000, 1).
Prints one JSON line. Reported, nothing is gated on.

Method (tools/temporal_bench.py's `timed`): warm-up calls, then untimed calls until 25 ms of load
have passed, then >= 20 timed repetitions, each between two device events on the stream; median and
spread. The passes are timed alternately, twice each in one process (a, b, c, a, b, c), and the two
medians of each are reported: their distance is the run-to-run spread a ratio has to exceed. Per scene:
  counted_uniform_ms   lrt_render_counts_device with counts == 4 everywhere (frames 4, capacity 4 per pixel)
  render_ms            lrt_render_device, frames 4, its own kernel choice: the yardstick at the same samples
  render_simple_ms     the same with LRT_F_SIMPLE (v0)
  counted_adaptive_ms  the counted render under a budget map: four 1 spp temporal steps through
                       svgf_filter_tensor give variance_out, lrt_sample_budget_device turns it into counts
                       (min_count 1, max_count 32, budget 4 per pixel); frames 32, the same capacity
  adaptive_samples     that map's total, and its histogram in powers of two
  counted_zero_ms      the counted render with counts == 0: the scan, an empty trace launch, the merge's reads
  trace_kernel_ms      the trace kernel alone inside counted_uniform (lrt_kernel_timing's events)
  scan_merge_ms        counted_uniform_ms - trace_kernel_ms: the scan, the merge and the gaps between launches
  budget_ms            lrt_sample_budget_device (variance and colour in, counts and info out, 2 passes)
  budget_fill_ms       a plain device fill of its bytes (budget_bytes per pixel)
The quality leg (--quality): 1280x720 too; relative MSE, mean((out - ref)^2 / (ref^2 + 0.01)) over rgb,
against a 1024 spp render at EQUAL total samples: uniform 4 spp (sample frames 4..7 of every pixel)
against the counted render with LRT_RC_MEAN from frame0 = 4 under the pilot's budget map (the four
pilot frames 0..3 feed the variance only and are in neither picture); raw pictures, no filter behind.

  python tools/adaptive_bench.py [--width W --height H --reps N --quality]
"""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from temporal_bench import timed  # noqa: E402

SIMPLE = 2           # LRT_F_SIMPLE
SPP, MIN_COUNT, MAX_COUNT, PILOT = 4, 1, 32, 4
GUIDES = ("normal", "world_pos", "albedo")


def budget_bytes(color=True, passes=2):
    """Bytes per pixel lrt_sample_budget_device moves: the weight kernel reads the variance (16) and the
    colour (16) and writes q (4) and the count (4); a pass reads both (8) and writes the count (4)."""
    return 16 + (16 if color else 0) + 8 + 12 * passes


def pilot_variance(torch, lrt, w, h, depth, cam, dev, stream):
    """(variance_out, filtered colour) after PILOT 1 spp steps through the accumulator and the filter."""
    acc = lrt.TemporalAccumulator(w, h, dev)
    rays = torch.zeros(1, dtype=torch.int64, device=dev)
    with torch.cuda.stream(stream):
        var = torch.zeros((h, w, 4), device=dev)
    for t in range(PILOT):
        with torch.cuda.stream(stream):
            buf = torch.zeros((h, w, 4), device=dev)
        lrt.render_tensor(lrt.Job(width=w, height=h, frame0=t, frames=1, max_depth=depth, camera=cam), buf, rays, stream=stream)
        g = lrt.gbuffer_tensor(w, h, cam, out=acc.gbuffer_planes(), stream=stream)
        acc.step_gbuffer(buf, g, cur_scale=float(t + 1), stream=stream)
    out = lrt.svgf_filter_tensor(acc.state["color"], acc.state["moment2"], {n: g[n] for n in GUIDES}, variance_out=var,
                                 stream=stream)
    stream.synchronize()
    return var, out


def rel_mse(a, ref):
    return float(((a[..., :3] - ref[..., :3]) ** 2 / (ref[..., :3] ** 2 + 0.01)).mean())


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
        sys.exit("adaptive_bench: needs a GPU (there is no CPU path)")
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
        with torch.cuda.stream(s):
            buf = torch.zeros((h, w, 4), device=dev)
            rays = torch.zeros(1, dtype=torch.int64, device=dev)
            info = torch.zeros(2, dtype=torch.int64, device=dev)
            four = torch.full((h, w), SPP, dtype=torch.int32, device=dev)
            zero = torch.zeros((h, w), dtype=torch.int32, device=dev)
            counts = torch.zeros((h, w), dtype=torch.int32, device=dev)
            fill = torch.zeros(budget_bytes() * npix, dtype=torch.uint8, device=dev)
        line = {"tool": "adaptive_bench", "width": w, "height": h, "depth": depth, "reps": args.reps, "spp": SPP,
                "min_count": MIN_COUNT, "max_count": MAX_COUNT, "budget_bytes": budget_bytes(), "scenes": {}}
        job4 = lrt.Job(width=w, height=h, frames=SPP, max_depth=depth, camera=cam)
        job4s = lrt.Job(width=w, height=h, frames=SPP, max_depth=depth, camera=cam, flags=SIMPLE)
        job32 = lrt.Job(width=w, height=h, frames=MAX_COUNT, max_depth=depth, camera=cam)

        def do_fill():
            with torch.cuda.stream(s):
                fill.fill_(1)

        scenes = {"default": lrt.default_scene(), "random1000": lrt.random_scene(1000, 1)}
        try:
            for label, (sph, mats) in scenes.items():
                lrt.set_scene(sph, mats)
                var, col = pilot_variance(torch, lrt, w, h, depth, cam, dev, s)
                lrt.sample_budget_tensor(var, MIN_COUNT, MAX_COUNT, SPP * npix, color=col, counts=counts, info=info, stream=s)
                s.synchronize()
                hc = counts.cpu()
                out = {"spheres": len(sph), "adaptive_samples": int(hc.sum()),
                       "adaptive_histogram": {str(1 << k): int(((hc >= (1 << k)) & (hc < (2 << k))).sum()) for k in range(6)}}
                passes = {
                    "counted_uniform_ms": lambda: lrt.render_counts_tensor(job4, buf, rays, four, SPP * npix, stream=s),
                    "render_ms": lambda: lrt.render_tensor(job4, buf, rays, stream=s),
                    "render_simple_ms": lambda: lrt.render_tensor(job4s, buf, rays, stream=s),
                    "counted_adaptive_ms": lambda: lrt.render_counts_tensor(job32, buf, rays, counts, SPP * npix, stream=s),
                    "counted_zero_ms": lambda: lrt.render_counts_tensor(job4, buf, rays, zero, SPP * npix, stream=s),
                    "budget_ms": lambda: lrt.sample_budget_tensor(var, MIN_COUNT, MAX_COUNT, SPP * npix, color=col,
                                                                  counts=counts, info=info, stream=s),
                    "budget_fill_ms": do_fill,
                }
                runs = {name: [] for name in passes}
                for _ in range(2):                      # alternating, twice each
                    for name, fn in passes.items():
                        runs[name].append(timed(torch, s, fn, args.reps))
                for name, (a, b) in runs.items():
                    out[name] = round(min(a["median"], b["median"]), 4)
                    out[name + "_runs"] = [round(a["median"], 4), round(b["median"], 4)]
                    out[name + "_spread"] = {k: round(min(a[k], b[k]) if k == "min" else max(a[k], b[k]), 4)
                                             for k in ("min", "max")}
                out["render_kernel"] = None
                passes["render_ms"]()
                s.synchronize()
                out["render_kernel"] = L.last_launch().get("kernel")
                # the trace kernel alone, by the library's own events around it
                L.check(L.lib().lrt_kernel_timing(1))
                for _ in range(args.reps):
                    passes["counted_uniform_ms"]()
                s.synchronize()
                kt = (ctypes.c_float * args.reps)()
                nk = ctypes.c_int(0)
                L.check(L.lib().lrt_kernel_times(kt, args.reps, ctypes.byref(nk)))
                L.check(L.lib().lrt_kernel_timing(0))
                ks = sorted(kt[:nk.value])
                out["trace_kernel_ms"] = round(ks[len(ks) // 2], 4) if ks else None
                if ks:
                    out["scan_merge_ms"] = round(out["counted_uniform_ms"] - out["trace_kernel_ms"], 4)
                out["counted_over_render"] = round(out["counted_uniform_ms"] / out["render_ms"], 3)
                out["counted_over_simple"] = round(out["counted_uniform_ms"] / out["render_simple_ms"], 3)
                out["adaptive_over_uniform"] = round(out["counted_adaptive_ms"] / out["counted_uniform_ms"], 3)
                out["budget_over_fill"] = round(out["budget_ms"] / out["budget_fill_ms"], 3)
                if args.quality:
                    with torch.cuda.stream(s):
                        ref = torch.zeros((h, w, 4), device=dev)
                        uni = torch.zeros((h, w, 4), device=dev)
                        ada = torch.zeros((h, w, 4), device=dev)
                    lrt.render_tensor(lrt.Job(width=w, height=h, frames=1024, max_depth=depth, camera=cam), ref, rays, stream=s)
                    lrt.render_counts_tensor(lrt.Job(width=w, height=h, frame0=PILOT, frames=SPP, max_depth=depth, camera=cam),
                                             uni, rays, four, SPP * npix, mean=True, stream=s)
                    lrt.render_counts_tensor(lrt.Job(width=w, height=h, frame0=PILOT, frames=MAX_COUNT, max_depth=depth,
                                                     camera=cam), ada, rays, counts, SPP * npix, mean=True, info=info, stream=s)
                    s.synchronize()
                    out["quality"] = {"gt_spp": 1024, "uniform_samples": SPP * npix, "adaptive_samples": int(info[0].item()),
                                      "uniform_rel_mse": round(rel_mse(uni, ref), 5),
                                      "adaptive_rel_mse": round(rel_mse(ada, ref), 5)}
                line["scenes"][label] = out
        finally:
            lrt.set_scene(*lrt.default_scene())
        print(json.dumps(line))
    finally:
        lrt.ShutdownTest()


if __name__ == "__main__":
    main()
