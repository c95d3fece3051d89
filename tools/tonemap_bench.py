#!/usr/bin/env python3
"""Time auto-exposure metering and tone mapping (lrt_tonemap_device) on the headline frame:
1280x720, the default scene at depth 8, the accumulated colour two 1 spp frames from cameras of
the orbit lookFrom = (3 sin t, 2, 3 cos t) one step (0.02 rad) apart leave behind. Prints one JSON
line.

Candidates, each on that frame ("render") and on a constant frame ("constant": every pixel in one
bin, the contention case for a plain LDS add; the meter aggregates equal bins within a wave first):
  full     the whole call: auto_exposure 1, ACES, bgra only (meter, exposure, map)
  meter    the meter-only call (no output)
  map      the map alone (auto_exposure 0, ACES, bgra only)
  present  lrt_present_bgra8 of the same frame
  copy     a device-to-device copy that moves the full call's compulsory 36 B per pixel

Method (as tools/svgf_bench.py): warm-up calls of every candidate, untimed calls until 25 ms of load
have passed, then --reps rounds; a round times one call of each candidate in turn, each between two
device events on the stream. Medians and spreads per candidate.

  python tools/tonemap_bench.py [--width W --height H --reps N --dtheta RAD --images DIR]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

CUR = ("normal", "world_pos", "albedo")
CONSTANT = (0.4, 0.6, 0.9)


def call_bytes(meter=True, bgra=True, out=False):
    """Bytes per pixel one lrt_tonemap_device call must move: the meter reads the frame (16 B); the
    map, if there is an output, reads it again and writes 4 B of bgra and 12 B of out."""
    return 16 * meter + (16 if (bgra or out) else 0) + 4 * bgra + 12 * out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--height", type=int, default=720)
    ap.add_argument("--depth", type=int, default=8)
    ap.add_argument("--dtheta", type=float, default=0.02, help="the orbit step between the two cameras (rad)")
    ap.add_argument("--reps", type=int, default=40, help="timed rounds (>= 20)")
    ap.add_argument("--images", metavar="DIR", help="write the clamped and the tone-mapped frame there as PPM")
    args = ap.parse_args(argv)
    if args.reps < 20:
        ap.error("--reps must be >= 20")

    import torch

    if not torch.cuda.is_available():
        sys.exit("tonemap_bench: needs a GPU (there is no CPU path)")
    import learnraytracing_amd as lrt
    from learnraytracing_amd import _lib as L
    from learnraytracing_amd.renderer import present_tensor
    from svgf_bench import orbit_args, timed_alternating

    w, h = args.width, args.height
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
                col, _ = acc.step(buf, feats, cam, cur_scale=t + 1, stream=s)
            const = frame()
            const[..., :3] = torch.tensor(CONSTANT, device=dev)
            frames = {"render": col, "constant": const}
            state = torch.zeros(4, device=dev)
            bgra = torch.zeros(w * h, dtype=torch.int32, device=dev)
            moved = call_bytes() * w * h
            src = torch.zeros(moved // 8, dtype=torch.float32, device=dev)   # a copy of moved / 2 bytes reads and
            dst = torch.zeros_like(src)                                       # writes `moved` bytes

        def copy():
            with torch.cuda.stream(s):
                dst.copy_(src, non_blocking=True)

        fns = {}
        for name, f in frames.items():
            fns[f"full_{name}"] = lambda f=f: lrt.tonemap_tensor(f, state, bgra=bgra, stream=s)
            fns[f"meter_{name}"] = lambda f=f: lrt.tonemap_tensor(f, state, stream=s)
            fns[f"map_{name}"] = lambda f=f: lrt.tonemap_tensor(f, bgra=bgra, stream=s, auto_exposure=0)
            fns[f"present_{name}"] = lambda f=f: present_tensor(f, bgra, w, h, stream=s)
        fns["copy"] = copy
        t = timed_alternating(torch, s, fns, args.reps)
        s.synchronize()
        med = {k: v["median"] for k, v in t.items()}
        line = {"tool": "tonemap_bench", "width": w, "height": h, "depth": args.depth, "dtheta": args.dtheta,
                "reps": args.reps}
        for k, v in t.items():
            line[f"{k}_ms"] = round(med[k], 4)
            line[f"{k}_ms_spread"] = {q: round(x, 4) for q, x in v.items()}
        line.update({
            "bytes_per_pixel": call_bytes(), "meter_bytes_per_pixel": call_bytes(bgra=False),
            "map_bytes_per_pixel": call_bytes(meter=False),
            "gbytes_per_s": round(moved / (med["full_render"] * 1e-3) / 1e9, 1),
            "copy_gbytes_per_s": round(moved / (med["copy"] * 1e-3) / 1e9, 1),
            "full_over_present": round(med["full_render"] / med["present_render"], 3),
            "full_over_copy": round(med["full_render"] / med["copy"], 3),
            "meter_constant_over_render": round(med["meter_constant"] / med["meter_render"], 3),
            "version": L.lib().lrt_version().decode(),
        })
        with torch.cuda.stream(s):
            lrt.tonemap_tensor(col, state, bgra=bgra, stream=s)
        s.synchronize()
        line["log2_exposure"] = round(float(state[0].item()), 4)
        if args.images:
            from learnraytracing_amd import image
            os.makedirs(args.images, exist_ok=True)
            mapped = bgra.cpu().numpy().view(np.uint32).copy()
            with torch.cuda.stream(s):
                present_tensor(col, bgra, w, h, stream=s)
            s.synchronize()
            clamped = bgra.cpu().numpy().view(np.uint32)
            for name, words in (("clamped", clamped), ("tonemapped", mapped)):
                image.save_ppm_bgra(os.path.join(args.images, f"{name}.ppm"), words, w, h)
            line["images"] = args.images
        print(json.dumps(line), flush=True)
    finally:
        lrt.ShutdownTest()
    return 0


if __name__ == "__main__":
    sys.exit(main())
