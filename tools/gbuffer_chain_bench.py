#!/usr/bin/env python3
"""Time the chain pass (lrt_gbuffer_chain_device) on the headline frame, 1280x720 from the default
camera, for the default scene and random_scene(1000, 1), beside the G-buffer pass it extends.
Prints one JSON line.

Method (tools/temporal_bench.py's `timed`): warm-up calls, then untimed calls until 25 ms of load
have passed, then >= 20 timed repetitions, each between two device events on the stream; median and
spread. The passes are timed alternately, twice each in one process (a, b, a, b), and the two medians
of each are reported: their distance is the run-to-run spread a ratio has to exceed. Per scene:
  chain_ms         all seven planes (64 B per pixel), the defaults: max_bounces 4, roughness_max 0.25
  chain_d0_ms      the same with max_bounces 0: segment 0 alone
  gbuffer_all_ms   lrt_gbuffer_device, all six planes (72 B per pixel): the yardstick, the parent's code
  fill_ms          a plain device fill of 64 B per pixel: the store floor
  d0_over_gbuffer_bytes   chain_d0_ms / (gbuffer_all_ms * 64 / 72): 1 if both are bound by their stores
  chain_over_d0, chain_over_fill, chain_over_gbuffer   the ratios
  bounces          the histogram of the surfaces followed, and the unresolved pixels
The quality leg (--quality, reported, nothing is gated on): the default scene at 160x90 under a static
camera, 16 frames of 1 spp from the pool kernel through TemporalAccumulator.step_gbuffer and
svgf_filter_tensor, against a 1024 spp render; rel_mse = mean((out - ref)^2 / (ref^2 + 0.01)) over
the rgb of the pixels with bounces > 0 (and over all pixels), under
  first_hit        lrt_gbuffer's id and guides
  key              the chain's key as id, lrt_gbuffer's guides
  key_and_guides   the chain's key as id, the chain's normal, world_pos and albedo as guides

Measured on an MI355X, both medians of each pass:
  default scene     chain 0.0186 / 0.0186, d0 0.0142 / 0.0141, gbuffer_all 0.0150 / 0.0149, fill 0.0121 / 0.0121 ms;
                    d0 over byte-scaled gbuffer_all 1.065, chain over d0 1.32;
                    surfaces followed 763338 / 104899 / 49531 / 3718 / 114, 3 unresolved
  random_scene(1000, 1)   chain 0.0730 / 0.0737, d0 0.0235 / 0.0234, gbuffer_all 0.0237 / 0.0238 ms;
                    d0 over byte-scaled gbuffer_all 1.111, chain over d0 3.12;
                    surfaces followed 846684 / 33760 / 39097 / 1032 / 1027, 144 unresolved
  quality, rel_mse over the 2470 followed pixels (all pixels): first_hit 0.0722 (0.0697), key 0.0722
                    (0.0697: a static scene keeps every key), key_and_guides 0.0496 (0.0686)

  python tools/gbuffer_chain_bench.py [--width W --height H --reps N --quality]
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
QUALITY = dict(w=160, h=90, depth=8, steps=16, gt_spp=1024)


def quality(torch, lrt, dev):
    """The three settings' relative MSE after QUALITY["steps"] frames."""
    w, h, depth, steps = QUALITY["w"], QUALITY["h"], QUALITY["depth"], QUALITY["steps"]
    cam = lrt.default_camera(w, h)
    rays = torch.zeros(1, dtype=torch.int64, device=dev)
    ref = torch.zeros((h, w, 4), device=dev)
    lrt.render_tensor(lrt.Job(width=w, height=h, frames=QUALITY["gt_spp"], max_depth=depth, camera=cam, flags=POOL), ref, rays)
    chain = lrt.gbuffer_chain_tensor(w, h, cam)
    torch.cuda.synchronize()
    mirror = chain["bounces"] > 0
    out = {"width": w, "height": h, "steps": steps, "gt_spp": QUALITY["gt_spp"], "pixels_followed": int(mirror.sum())}
    for label, use_key, use_guides in (("first_hit", False, False), ("key", True, False), ("key_and_guides", True, True)):
        acc = lrt.TemporalAccumulator(w, h, dev)
        for t in range(steps):
            buf = torch.zeros((h, w, 4), device=dev)
            lrt.render_tensor(lrt.Job(width=w, height=h, frame0=t, frames=1, max_depth=depth, camera=cam, flags=POOL), buf, rays)
            g = lrt.gbuffer_tensor(w, h, cam, out=acc.gbuffer_planes())          # (ping-pongs two sets)
            c = lrt.gbuffer_chain_tensor(w, h, cam)                              # (new tensors: the keys ping-pong too)
            planes = {"normal": g["normal"], "motion": g["motion"], "id": c["key"] if use_key else g["id"]}
            acc.step_gbuffer(buf, planes, cur_scale=float(t + 1))
            guides = {n: (c if use_guides else g)[n] for n in GUIDES}
            done = lrt.svgf_filter_tensor(acc.state["color"], acc.state["moment2"], guides)
        torch.cuda.synchronize()
        err = ((done[..., :3] - ref[..., :3]) ** 2 / (ref[..., :3] ** 2 + 0.01)).mean(-1)
        out[label] = {"rel_mse_followed": round(float(err[mirror].mean()), 5), "rel_mse_all": round(float(err.mean()), 5)}
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--height", type=int, default=720)
    ap.add_argument("--reps", type=int, default=40, help="timed repetitions (>= 20)")
    ap.add_argument("--quality", action="store_true", help="also report the quality leg")
    args = ap.parse_args(argv)
    if args.reps < 20:
        ap.error("--reps must be >= 20")

    import torch

    if not torch.cuda.is_available():
        sys.exit("gbuffer_chain_bench: needs a GPU (there is no CPU path)")
    import learnraytracing_amd as lrt
    from learnraytracing_amd import _lib as L

    w, h = args.width, args.height
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    lrt.InitializeTest()
    try:
        s = torch.cuda.Stream(dev)
        cam = lrt.default_camera(w, h)
        with torch.cuda.stream(s):
            def plane(n):
                ints = n in L.GBUFFER_CHAIN_INT_NAMES or n == "id"
                return torch.zeros((h, w) if ints or n == "depth" else (h, w, 4),
                                   dtype=torch.int32 if ints else torch.float32, device=dev)
            cplanes = {n: plane(n) for n in L.GBUFFER_CHAIN_NAMES}
            gplanes = {n: plane(n) for n in L.GBUFFER_NAMES}
            fill = torch.zeros(64 * w * h, dtype=torch.uint8, device=dev)
        line = {"tool": "gbuffer_chain_bench", "width": w, "height": h, "reps": args.reps, "scenes": {}}

        def do_fill():
            with torch.cuda.stream(s):
                fill.fill_(1)

        passes = {
            "chain_ms": lambda: lrt.gbuffer_chain_tensor(w, h, cam, out=cplanes, stream=s),
            "chain_d0_ms": lambda: lrt.gbuffer_chain_tensor(w, h, cam, max_bounces=0, out=cplanes, stream=s),
            "gbuffer_all_ms": lambda: lrt.gbuffer_tensor(w, h, cam, cam, out=gplanes, stream=s),
            "fill_ms": do_fill,
        }
        scenes = {"default": lrt.default_scene(), "random1000": lrt.random_scene(1000, 1)}
        try:
            for label, (sph, mats) in scenes.items():
                lrt.set_scene(sph, mats)
                out = {"spheres": len(sph)}
                runs = {name: [] for name in passes}
                for _ in range(2):                      # alternating: a, b, c, d, a, b, c, d
                    for name, fn in passes.items():
                        runs[name].append(timed(torch, s, fn, args.reps))
                for name, (a, b) in runs.items():
                    out[name] = round(min(a["median"], b["median"]), 4)
                    out[name + "_runs"] = [round(a["median"], 4), round(b["median"], 4)]
                    out[name + "_spread"] = {k: round(min(a[k], b[k]) if k == "min" else max(a[k], b[k]), 4)
                                             for k in ("min", "max")}
                out["d0_over_gbuffer_bytes"] = round(out["chain_d0_ms"] / (out["gbuffer_all_ms"] * 64 / 72), 3)
                out["chain_over_d0"] = round(out["chain_ms"] / out["chain_d0_ms"], 3)
                out["chain_over_fill"] = round(out["chain_ms"] / out["fill_ms"], 3)
                out["chain_over_gbuffer"] = round(out["chain_ms"] / out["gbuffer_all_ms"], 3)
                out["chain_gbytes_per_s"] = round(64 * w * h / (out["chain_ms"] * 1e-3) / 1e9, 1)
                lrt.gbuffer_chain_tensor(w, h, cam, out=cplanes, stream=s)
                s.synchronize()
                b = cplanes["bounces"]
                out["bounces"] = torch.bincount((b & 0xFF).flatten()).tolist()
                out["unresolved"] = int((b >= L.CHAIN_UNRESOLVED).sum())
                line["scenes"][label] = out
        finally:
            lrt.set_scene(*scenes["default"])
        s.synchronize()
        if args.quality:
            line["quality"] = quality(torch, lrt, dev)
        line["version"] = L.lib().lrt_version().decode()
        print(json.dumps(line), flush=True)
    finally:
        lrt.ShutdownTest()
    return 0


if __name__ == "__main__":
    sys.exit(main())
