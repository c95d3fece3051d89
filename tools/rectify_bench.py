#!/usr/bin/env python3
"""Time history rectification (lrt_temporal_rectify_device) on the headline frame, 1280x720, at radius
1, 2 and 3 beside a fill of its bytes, and the full-resolution G-buffer chain with and without it.
Prints one JSON line.

Method (as tools/temporal_bench.py): warm-up calls, then untimed calls until 25 ms of load have
passed, then >= 20 timed repetitions, each between two device events on the stream; the median, three
runs of each. Default scene.
  rectify_ms[r]      one call in place on a state (color_std written, no class plane), the reference one
                     1 spp pool frame; three medians
  fill_ms            a plain device fill of rectify_bytes() in the same run; three medians
  rectify_over_fill  the middle rectify median over the middle fill median, per radius
  classes[r]         pixels per class of that call out of place (0: inside the box, 1: clamped, 2: unsupported)
  chain_ms           pool render at 1 spp, depth 8 -> G-buffer -> step_gbuffer -> svgf_filter_tensor
  chain_rectify_ms   the same with step_gbuffer(rectify={})
Nothing is gated on.

  python tools/rectify_bench.py [--width W --height H --reps N]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from temporal_bench import timed  # noqa: E402

POOL = 512          # LRT_F_POOL
GUIDES = ("normal", "world_pos", "albedo")
RADII = (1, 2, 3)
RUNS = 3


def rectify_bytes(color_std=True):
    """Bytes per pixel one call must move: the reference (16 B), the id (4 B) and the state's color and
    moment2 (16 B each) read; color's rgb (12 B) and moment2 (16 B) written, plus color_std's rgb (12 B)."""
    return 16 + 4 + 16 + 16 + 12 + 16 + (12 if color_std else 0)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--height", type=int, default=720)
    ap.add_argument("--depth", type=int, default=8)
    ap.add_argument("--reps", type=int, default=40, help="timed repetitions (>= 20)")
    args = ap.parse_args(argv)
    if args.reps < 20:
        ap.error("--reps must be >= 20")

    import torch

    if not torch.cuda.is_available():
        sys.exit("rectify_bench: needs a GPU (there is no CPU path)")
    import learnraytracing_amd as lrt
    from learnraytracing_amd import _lib as L

    w, h = args.width, args.height
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    lrt.InitializeTest()
    try:
        s = torch.cuda.Stream(dev)
        cam = lrt.default_camera(w, h)
        nbytes = w * h * rectify_bytes()
        with torch.cuda.stream(s):
            buf, flt = torch.zeros((h, w, 4), device=dev), torch.zeros((h, w, 4), device=dev)
            rays = torch.zeros(1, dtype=torch.int64, device=dev)
            fill = torch.zeros(nbytes, dtype=torch.uint8, device=dev)
            cls = torch.zeros((h, w), dtype=torch.int32, device=dev)
            acc, acc_r = lrt.TemporalAccumulator(w, h, dev), lrt.TemporalAccumulator(w, h, dev)
        line = {"tool": "rectify_bench", "width": w, "height": h, "depth": args.depth, "reps": args.reps,
                "runs": RUNS, "rectify_bytes": nbytes, "rectify_ms": {}, "rectify_over_fill": {}, "classes": {}}

        def medians(fn):
            return [round(timed(torch, s, fn, args.reps)["median"], 4) for _ in range(RUNS)]

        def filler():
            with torch.cuda.stream(s):
                fill.fill_(1)

        def chain(a, rectify):
            lrt.render_tensor(lrt.Job(width=w, height=h, frames=1, max_depth=args.depth, camera=cam, flags=POOL), buf, rays,
                              stream=s)
            planes = lrt.gbuffer_tensor(w, h, cam, out=a.gbuffer_planes(), stream=s)
            a.step_gbuffer(buf, planes, stream=s, rectify=rectify)
            st = a.state
            lrt.svgf_filter_tensor(st["color"], st["moment2"], {k: planes[k] for k in GUIDES}, out=flt, stream=s)
            return planes

        # a state of four accumulated frames and a fresh frame as the reference
        for _ in range(4):
            planes = chain(acc, None)
        with torch.cuda.stream(s):
            state = {k: acc._states[acc._cur][k].clone() for k in ("color", "moment2", "color_std")}
            ref, ids = buf.clone(), planes["id"].clone()
            work = {k: v.clone() for k, v in state.items()}
            scratch = {k: torch.zeros((h, w, 4), device=dev) for k in state}
        s.synchronize()
        line["fill_ms"] = medians(filler)
        mid = lambda v: sorted(v)[len(v) // 2]   # noqa: E731
        for r in RADII:
            lrt.temporal_rectify_tensor(ref, ids, state, out=scratch, class_out=cls, stream=s, radius=r)
            s.synchronize()
            line["classes"][str(r)] = torch.bincount(cls.ravel(), minlength=3)[:3].tolist()
            line["rectify_ms"][str(r)] = medians(lambda: lrt.temporal_rectify_tensor(ref, ids, work, out=work, stream=s,
                                                                                     radius=r))
            line["rectify_over_fill"][str(r)] = round(mid(line["rectify_ms"][str(r)]) / mid(line["fill_ms"]), 3)
        line["rectify_gbytes_per_s"] = {k: round(nbytes / (mid(v) * 1e-3) / 1e9, 1) for k, v in line["rectify_ms"].items()}
        line["chain_ms"] = medians(lambda: chain(acc, None))
        line["chain_rectify_ms"] = medians(lambda: chain(acc_r, {}))
        s.synchronize()
        line["version"] = L.lib().lrt_version().decode()
        print(json.dumps(line), flush=True)
    finally:
        lrt.ShutdownTest()
    return 0


if __name__ == "__main__":
    sys.exit(main())
