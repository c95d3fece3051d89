#!/usr/bin/env python3
"""Time the variance-guided filter (lrt_svgf_filter_device) on the headline frame: 1280x720, the
default scene at depth 8, the state two 1 spp frames from cameras of the orbit lookFrom =
(3 sin t, 2, 3 cos t) one step (0.02 rad) apart leave behind, default parameters, K = 5,
variance_out on. Prints one JSON line.

Two states are filtered: the accumulated one ("history": min_history is lowered to 2 for it, so
that the 7x7 spatial estimate runs only where the reprojection found nothing, as it does after a
few frames at the default) and a first frame (n = 1 everywhere: the spatial estimate runs at every
pixel). For scale the existing lrt_denoise_device 5-pass filters the same accumulated frame in the
same process, and a device-to-device copy moves the filter's compulsory bytes.

Method (as bench.py and tools/temporal_bench.py): warm-up calls of every candidate, untimed calls
until 25 ms of load have passed (the shader clock settles under load), then --reps rounds; a round
times one call of each candidate in turn, each between two device events on the stream, so that the
candidates alternate and share whatever else the machine is doing. Medians and spreads per candidate.
Bytes: what a call must move at least -- every buffer a launch reads or writes, once per launch.

  python tools/svgf_bench.py [--width W --height H --reps N --dtheta RAD --iterations K]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HOLD_SECONDS = 0.025
CUR = ("normal", "world_pos", "albedo")


def filter_bytes(iterations=5, albedo=True, variance_out=True, first_frame=False):
    """Bytes per pixel one lrt_svgf_filter_device call must move with normal and world_pos given:
    stage 0 reads colour, moment2 and normal (and albedo; and world_pos where the spatial estimate
    runs: first_frame), 16 B each, and writes (c_0, var_0), 32 B; a pass reads c, var, normal and
    world_pos and writes (c, var), 32 B; the last pass reads albedo again and writes 12 B of out
    (and 12 B of variance_out) instead."""
    stage0 = 16 * (3 + albedo + first_frame) + 32
    passes = iterations * 4 * 16 + (iterations - 1) * 32
    return stage0 + passes + 16 * albedo + 12 + 12 * variance_out


def denoise_bytes(iterations=5):
    """The same count for lrt_denoise_device with all four guides: a pass reads colour, normal,
    world_pos, albedo and color_std and writes 16 B (the last: 12 B)."""
    return iterations * 5 * 16 + (iterations - 1) * 16 + 12


def orbit_args(theta, w, h):
    look_from = (3.0 * np.sin(theta), 2.0, 3.0 * np.cos(theta))
    return look_from, (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), 60.0, w / h, 0.1, float(np.linalg.norm(look_from))


def timed_alternating(torch, stream, fns, reps):
    """{name: median / min / max / p10 / p90 ms} of each fn over reps rounds, one call of each per round."""
    for fn in fns.values():
        for _ in range(3):
            fn()
    stream.synchronize()
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < HOLD_SECONDS:
        for fn in fns.values():
            fn()
        stream.synchronize()
    ev = {k: [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
          for k in fns}
    for r in range(reps):
        for k, fn in fns.items():
            a, b = ev[k][r]
            a.record(stream)
            fn()
            b.record(stream)
    stream.synchronize()
    out = {}
    for k in fns:
        ms = sorted(a.elapsed_time(b) for a, b in ev[k])
        out[k] = {"median": statistics.median(ms), "min": ms[0], "max": ms[-1],
                  "p10": ms[len(ms) // 10], "p90": ms[(len(ms) * 9) // 10]}
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--height", type=int, default=720)
    ap.add_argument("--depth", type=int, default=8)
    ap.add_argument("--dtheta", type=float, default=0.02, help="the orbit step between the two cameras (rad)")
    ap.add_argument("--iterations", type=int, default=5, help="passes K of both filters (1..5)")
    ap.add_argument("--reps", type=int, default=40, help="timed rounds (>= 20)")
    args = ap.parse_args(argv)
    if args.reps < 20:
        ap.error("--reps must be >= 20")
    if not 1 <= args.iterations <= 5:
        ap.error("--iterations must be in 1..5")

    import torch

    if not torch.cuda.is_available():
        sys.exit("svgf_bench: needs a GPU (there is no CPU path)")
    import learnraytracing_amd as lrt
    from learnraytracing_amd import _lib as L

    w, h, K = args.width, args.height, args.iterations
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    lrt.InitializeTest()
    try:
        s = torch.cuda.Stream(dev)
        frame = lambda: torch.zeros((h, w, 4), device=dev)   # noqa: E731
        with torch.cuda.stream(s):
            rays = torch.zeros(1, dtype=torch.int64, device=dev)
            acc = lrt.TemporalAccumulator(w, h, dev)
            for t, theta in enumerate((-args.dtheta, 0.0)):
                cam = lrt.make_camera(*orbit_args(theta, w, h))
                buf, feats = frame(), {n: frame() for n in CUR}
                lrt.render_tensor_features(lrt.Job(width=w, height=h, frame0=t, frames=1, max_depth=args.depth,
                                                   camera=cam), buf, rays, feats, -1, stream=s)
                col, guides = acc.step(buf, feats, cam, cur_scale=t + 1, stream=s, min_history=2)
            st = acc.state
            g3 = {n: st[n] for n in CUR}
            first_m2 = st["moment2"].clone()
            first_m2[..., :3] = st["color"][..., :3] ** 2
            first_m2[..., 3] = 1.0
            out, var, den = frame(), frame(), frame()
            moved = filter_bytes(K) * w * h
            src = torch.zeros(moved // 8, dtype=torch.float32, device=dev)   # a copy of moved / 2 bytes reads and
            dst = torch.zeros_like(src)                                       # writes `moved` bytes

        def copy():
            with torch.cuda.stream(s):
                dst.copy_(src, non_blocking=True)

        fns = {
            "svgf": lambda: lrt.svgf_filter_tensor(st["color"], st["moment2"], g3, out=out, variance_out=var, stream=s,
                                                   iterations=K, min_history=2),
            "denoise": lambda: lrt.denoise_tensor(col, guides, out=den, stream=s, iterations=K),
            "svgf_first": lambda: lrt.svgf_filter_tensor(st["color"], first_m2, g3, out=out, variance_out=var,
                                                         stream=s, iterations=K),
            "copy": copy,
        }
        t = timed_alternating(torch, s, fns, args.reps)
        s.synchronize()
        short = float((st["moment2"][..., 3] < 2).float().mean().item())
        rnd = lambda d: {k: round(v, 4) for k, v in d.items()}   # noqa: E731
        med = {k: v["median"] for k, v in t.items()}
        line = {
            "tool": "svgf_bench", "width": w, "height": h, "depth": args.depth, "dtheta": args.dtheta,
            "iterations": K, "reps": args.reps,
            "svgf_ms": round(med["svgf"], 4), "svgf_ms_spread": rnd(t["svgf"]),
            "svgf_first_frame_ms": round(med["svgf_first"], 4), "svgf_first_frame_ms_spread": rnd(t["svgf_first"]),
            "denoise_ms": round(med["denoise"], 4), "denoise_ms_spread": rnd(t["denoise"]),
            "copy_ms": round(med["copy"], 4), "copy_ms_spread": rnd(t["copy"]),
            "bytes_per_pixel": filter_bytes(K), "denoise_bytes_per_pixel": denoise_bytes(K),
            "gbytes_per_s": round(moved / (med["svgf"] * 1e-3) / 1e9, 1),
            "denoise_gbytes_per_s": round(denoise_bytes(K) * w * h / (med["denoise"] * 1e-3) / 1e9, 1),
            "copy_gbytes_per_s": round(moved / (med["copy"] * 1e-3) / 1e9, 1),
            "svgf_over_copy": round(med["svgf"] / med["copy"], 3),
            "svgf_over_denoise": round(med["svgf"] / med["denoise"], 3),
            "short_history": round(short, 4),
            "version": L.lib().lrt_version().decode(),
        }
        print(json.dumps(line), flush=True)
    finally:
        lrt.ShutdownTest()
    return 0


if __name__ == "__main__":
    sys.exit(main())
