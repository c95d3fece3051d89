#!/usr/bin/env python3
"""Time the chain motion pass (lrt_gbuffer_chain_motion_device) on the headline frame, 1280x720, one
orbit step of 0.02 rad, for the default scene and random_scene(1000, 1), beside the chain pass and the
G-buffer pass. Prints one JSON line.

Method (tools/temporal_bench.py's `timed`): warm-up calls, then untimed calls until 25 ms of load
have passed, then >= 20 timed repetitions (40 by default), each between two device events on the
stream; median and spread. The passes are timed alternately, twice each in one process (a, b, a, b),
and the two medians of each are reported: their distance is the run-to-run spread a ratio has to
exceed. Per scene:
  chain_motion_ms  both planes, the defaults (3 iterations: 11 walks per followed pixel)
  chain_ms         lrt_gbuffer_chain_device, all seven planes, from the current camera
  gbuffer_all_ms   lrt_gbuffer_device, all six planes, for the camera pair
  fill_ms          a plain device copy of 16 B per pixel into 16 of its 20 B, plus a 4 B fill: the
                   pass's bytes (32 B per pixel read and written, plus 4)
  status           the histogram of LRT_CM_*
  ns_per_followed_walk   chain_motion_ms over (followed pixels x 11 walks)
  motion_over_chain, motion_over_gbuffer   the ratios
The quality leg (--quality, reported, nothing is gated on): the default scene at 160x90, 16 orbit steps
of 1 spp from the pool kernel through TemporalAccumulator.step_gbuffer and svgf_filter_tensor with the
chain's key as id and the chain's guides, once with lrt_gbuffer's first-hit motion and once with this
pass's plane, against a 1024 spp render of the last frame;
rel_mse = mean((out - ref)^2 / (ref^2 + 0.01)) over the rgb of the followed pixels (and of all pixels).

  python tools/gbuffer_chain_motion_bench.py [--width W --height H --reps N --quality]
"""
import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from temporal_bench import timed  # noqa: E402

POOL = 512          # LRT_F_POOL
DTHETA = 0.02
GUIDES = ("normal", "world_pos", "albedo")
QUALITY = dict(w=160, h=90, depth=8, steps=16, gt_spp=1024)
STATUS = ("not_followed", "converged", "unresolved", "no_seed", "key_lost", "not_converged")


def orbit(lrt, w, h, theta):
    return lrt.make_camera((3.0 * math.sin(theta), 2.0, 3.0 * math.cos(theta)), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), 60.0,
                           w / h, 0.1, 3.0)


def quality(torch, lrt, dev):
    """The two motions' relative MSE after QUALITY["steps"] orbit steps."""
    w, h, depth, steps = QUALITY["w"], QUALITY["h"], QUALITY["depth"], QUALITY["steps"]
    cams = [orbit(lrt, w, h, DTHETA * t) for t in range(steps)]
    rays = torch.zeros(1, dtype=torch.int64, device=dev)
    ref = torch.zeros((h, w, 4), device=dev)
    lrt.render_tensor(lrt.Job(width=w, height=h, frames=QUALITY["gt_spp"], max_depth=depth, camera=cams[-1], flags=POOL),
                      ref, rays)
    followed = lrt.gbuffer_chain_tensor(w, h, cams[-1])["bounces"] > 0
    torch.cuda.synchronize()
    out = {"width": w, "height": h, "steps": steps, "dtheta": DTHETA, "gt_spp": QUALITY["gt_spp"],
           "pixels_followed": int(followed.sum())}
    for label, use_new in (("first_hit_motion", False), ("chain_motion", True)):
        acc = lrt.TemporalAccumulator(w, h, dev)
        for t, cam in enumerate(cams):
            prev = cams[max(t - 1, 0)]
            buf = torch.zeros((h, w, 4), device=dev)
            lrt.render_tensor(lrt.Job(width=w, height=h, frame0=t, frames=1, max_depth=depth, camera=cam, flags=POOL), buf, rays)
            g = lrt.gbuffer_tensor(w, h, cam, prev, out=acc.gbuffer_planes())      # (ping-pongs two sets)
            c = lrt.gbuffer_chain_tensor(w, h, cam)                                # (new tensors: the keys ping-pong too)
            motion = lrt.gbuffer_chain_motion_tensor(w, h, cam, prev, g["motion"], status=False)["motion"] if use_new \
                else g["motion"]
            acc.step_gbuffer(buf, {"normal": g["normal"], "motion": motion, "id": c["key"]}, cur_scale=float(t + 1))
            done = lrt.svgf_filter_tensor(acc.state["color"], acc.state["moment2"], {n: c[n] for n in GUIDES})
        torch.cuda.synchronize()
        err = ((done[..., :3] - ref[..., :3]) ** 2 / (ref[..., :3] ** 2 + 0.01)).mean(-1)
        out[label] = {"rel_mse_followed": round(float(err[followed].mean()), 5), "rel_mse_all": round(float(err.mean()), 5),
                      "mean_history_followed": round(float(acc.state["moment2"][..., 3][followed].mean()), 2)}
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
        sys.exit("gbuffer_chain_motion_bench: needs a GPU (there is no CPU path)")
    import learnraytracing_amd as lrt
    from learnraytracing_amd import _lib as L

    w, h = args.width, args.height
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    lrt.InitializeTest()
    try:
        s = torch.cuda.Stream(dev)
        cam, pcam = orbit(lrt, w, h, 0.0), orbit(lrt, w, h, -DTHETA)
        with torch.cuda.stream(s):
            def plane(n):
                ints = n in L.GBUFFER_CHAIN_INT_NAMES or n in ("id", "status")
                return torch.zeros((h, w) if ints or n == "depth" else (h, w, 4),
                                   dtype=torch.int32 if ints else torch.float32, device=dev)
            cplanes = {n: plane(n) for n in L.GBUFFER_CHAIN_NAMES}
            gplanes = {n: plane(n) for n in L.GBUFFER_NAMES}
            mplanes = {n: plane(n) for n in L.GBUFFER_CHAIN_MOTION_NAMES}
            copy_dst, fill = torch.zeros((h, w, 4), device=dev), torch.zeros((h, w), dtype=torch.int32, device=dev)
        line = {"tool": "gbuffer_chain_motion_bench", "width": w, "height": h, "reps": args.reps, "dtheta": DTHETA,
                "scenes": {}}

        def do_fill():
            with torch.cuda.stream(s):
                copy_dst.copy_(gplanes["motion"])
                fill.fill_(1)

        passes = {
            "chain_motion_ms": lambda: lrt.gbuffer_chain_motion_tensor(w, h, cam, pcam, gplanes["motion"], out=mplanes,
                                                                       stream=s),
            "chain_ms": lambda: lrt.gbuffer_chain_tensor(w, h, cam, out=cplanes, stream=s),
            "gbuffer_all_ms": lambda: lrt.gbuffer_tensor(w, h, cam, pcam, out=gplanes, stream=s),
            "fill_ms": do_fill,
        }
        scenes = {"default": lrt.default_scene(), "random1000": lrt.random_scene(1000, 1)}
        try:
            for label, (sph, mats) in scenes.items():
                lrt.set_scene(sph, mats)
                lrt.gbuffer_tensor(w, h, cam, pcam, out=gplanes, stream=s)      # the first-hit motion the pass reads
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
                lrt.gbuffer_chain_motion_tensor(w, h, cam, pcam, gplanes["motion"], out=mplanes, stream=s)
                s.synchronize()
                hist = torch.bincount(mplanes["status"].flatten(), minlength=len(STATUS)).tolist()
                out["status"] = dict(zip(STATUS, hist))
                followed = w * h - hist[0]
                moved = (mplanes["motion"] - gplanes["motion"])[..., :2].norm(dim=-1)[mplanes["status"] == 1]
                out["followed_share"] = round(followed / (w * h), 4)
                out["converged_of_followed"] = round(hist[1] / max(1, followed), 4)
                out["motion_minus_first_px"] = {"median": round(float(moved.median()), 3), "max": round(float(moved.max()), 3)} \
                    if moved.numel() else None
                out["ns_per_followed_walk"] = round(out["chain_motion_ms"] * 1e6 / max(1, followed * 11), 4)
                out["motion_over_chain"] = round(out["chain_motion_ms"] / out["chain_ms"], 3)
                out["motion_over_gbuffer"] = round(out["chain_motion_ms"] / out["gbuffer_all_ms"], 3)
                out["motion_over_fill"] = round(out["chain_motion_ms"] / out["fill_ms"], 3)
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
