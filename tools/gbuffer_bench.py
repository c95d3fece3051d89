#!/usr/bin/env python3
"""Time the G-buffer pass (lrt_gbuffer_device) on the headline frame, 1280x720 from the default
camera, for the default scene and random_scene(1000, 1). Prints one JSON line.

Method (as tools/temporal_bench.py): warm-up calls, then untimed calls until 25 ms of load have
passed, then >= 20 timed repetitions, each between two device events on the stream; median and
spread. Per scene:
  gbuffer_guides_ms   normal, world_pos and albedo (48 B per pixel)
  gbuffer_all_ms      all six planes, no scene given (72 B per pixel)
  gbuffer_moved_ms    all six planes with a scene in which one sphere moved and an orbit step of
                      the camera
  fill_guides_ms, fill_all_ms   a plain device fill of the same number of bytes in the same run:
                      the store floor
  render_features_ms  the 4 spp, depth 8 render with its feature side output (render_tensor_features)
  render_pool_ms      the same job with LRT_F_POOL, which has no feature output
  pool_plus_gbuffer_ms = render_pool_ms + gbuffer_guides_ms, and `cheaper`: which of the two ways
                      to a frame with guides took less
Nothing is gated on.

  python tools/gbuffer_bench.py [--width W --height H --reps N]
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
MOVING_STEP = 0.1
GUIDES = ("normal", "world_pos", "albedo")


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--height", type=int, default=720)
    ap.add_argument("--depth", type=int, default=8)
    ap.add_argument("--spp", type=int, default=4)
    ap.add_argument("--reps", type=int, default=40, help="timed repetitions (>= 20)")
    args = ap.parse_args(argv)
    if args.reps < 20:
        ap.error("--reps must be >= 20")

    import torch

    if not torch.cuda.is_available():
        sys.exit("gbuffer_bench: needs a GPU (there is no CPU path)")
    import learnraytracing_amd as lrt
    from learnraytracing_amd import _lib as L

    w, h = args.width, args.height
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    lrt.InitializeTest()
    rnd = lambda d: {k: round(v, 4) for k, v in d.items()}   # noqa: E731
    try:
        s = torch.cuda.Stream(dev)
        cam = lrt.default_camera(w, h)
        pcam = lrt.make_camera(*orbit_args(-0.02, w, h)[:6], 3.0)
        with torch.cuda.stream(s):
            planes = {n: torch.zeros((h, w) if n in ("id", "depth") else (h, w, 4),
                                     dtype=torch.int32 if n == "id" else torch.float32, device=dev)
                      for n in L.GBUFFER_NAMES}
            buf = torch.zeros((h, w, 4), device=dev)
            feats = {n: torch.zeros((h, w, 4), device=dev) for n in GUIDES}
            rays = torch.zeros(1, dtype=torch.int64, device=dev)
            fill = torch.zeros(72 * w * h, dtype=torch.uint8, device=dev)
        guides = {n: planes[n] for n in GUIDES}
        line = {"tool": "gbuffer_bench", "width": w, "height": h, "depth": args.depth, "spp": args.spp,
                "reps": args.reps, "scenes": {}}

        def put(out, name, t):
            out[name] = round(t["median"], 4)
            out[name + "_spread"] = rnd(t)

        def filler(nbytes):
            def fn():
                with torch.cuda.stream(s):
                    fill[:nbytes].fill_(1)
            return fn

        t_fill = {48: timed(torch, s, filler(48 * w * h), args.reps), 72: timed(torch, s, filler(72 * w * h), args.reps)}
        scenes = {"default": lrt.default_scene(), "random1000": lrt.random_scene(1000, 1)}
        try:
            for label, (sph, mats) in scenes.items():
                lrt.set_scene(sph, mats)
                before = list(sph)
                moved = 2 if len(sph) == 9 else 500
                c = before[moved].center
                before[moved] = L.Sphere(L.f3(c.x - MOVING_STEP, c.y, c.z), before[moved].radius)
                sph, before = (L.Sphere * len(sph))(*sph), (L.Sphere * len(sph))(*before)   # marshalled once
                out = {"spheres": len(sph)}
                put(out, "gbuffer_guides_ms", timed(torch, s, lambda: lrt.gbuffer_tensor(w, h, cam, out=guides, stream=s),
                                                    args.reps))
                put(out, "gbuffer_all_ms", timed(torch, s, lambda: lrt.gbuffer_tensor(w, h, cam, pcam, out=planes, stream=s),
                                                 args.reps))
                put(out, "gbuffer_moved_ms", timed(torch, s, lambda: lrt.gbuffer_tensor(
                    w, h, cam, pcam, spheres=sph, prev_spheres=before, out=planes, stream=s), args.reps))
                put(out, "fill_guides_ms", t_fill[48])
                put(out, "fill_all_ms", t_fill[72])
                out["guides_over_fill"] = round(out["gbuffer_guides_ms"] / out["fill_guides_ms"], 3)
                out["all_over_fill"] = round(out["gbuffer_all_ms"] / out["fill_all_ms"], 3)
                out["all_gbytes_per_s"] = round(72 * w * h / (out["gbuffer_all_ms"] * 1e-3) / 1e9, 1)
                job = lrt.Job(width=w, height=h, frames=args.spp, max_depth=args.depth, camera=cam)
                pool = lrt.Job(width=w, height=h, frames=args.spp, max_depth=args.depth, camera=cam, flags=POOL)
                put(out, "render_features_ms", timed(torch, s, lambda: lrt.render_tensor_features(
                    job, buf, rays, feats, -1, stream=s), args.reps))
                out["render_features_kernel"] = L.last_launch().get("kernel")
                put(out, "render_pool_ms", timed(torch, s, lambda: lrt.render_tensor(pool, buf, rays, stream=s), args.reps))
                out["render_pool_kernel"] = L.last_launch().get("kernel")
                out["pool_plus_gbuffer_ms"] = round(out["render_pool_ms"] + out["gbuffer_guides_ms"], 4)
                out["cheaper"] = ("pool_plus_gbuffer" if out["pool_plus_gbuffer_ms"] < out["render_features_ms"]
                                  else "render_features")
                line["scenes"][label] = out
        finally:
            lrt.set_scene(*scenes["default"])
        s.synchronize()
        line["version"] = L.lib().lrt_version().decode()
        print(json.dumps(line), flush=True)
    finally:
        lrt.ShutdownTest()
    return 0


if __name__ == "__main__":
    sys.exit(main())
