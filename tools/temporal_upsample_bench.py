#!/usr/bin/env python3
"""Time temporal upsampling (lrt_temporal_upsample_device) on the headline frame, 1280x720 from
640x360, for the default scene and random_scene(1000, 1), beside a fill of its bytes, its chain beside
tools/upsample_bench.py's two, and what the jitter buys. Prints one JSON line.

Method (as tools/temporal_bench.py): warm-up calls, then untimed calls until 25 ms of load have
passed, then >= 20 timed repetitions, each between two device events on the stream; median and
spread. Per scene:
  temporal_upsample_ms   one history step (color_std written, no class plane) under the phase (-low_width, -low_height)
  fill_ms                a plain device fill of temporal_upsample_bytes() in the same run
  classes                pixels per class of that step (0: history and current, 1: history only, 2: current only, 3: neither)
  chain_temporal_ms  pool render at 640x360, 4 spp, depth 8, under the jittered camera -> low G-buffer (id, normal)
                     under the same camera -> 1280x720 G-buffer under the unjittered one -> the step ->
                     svgf_filter_tensor at 1280x720
  chain_half_ms      upsample_bench's: the chain at 640x360, then the 1280x720 G-buffer and lrt_upsample
  chain_full_ms      upsample_bench's: the chain at 1280x720, 1 spp
  relmse             mean over the pixels of |x - ref|^2 / (|ref|^2 + 0.01) against a 1024 spp render at
                     1280x720 made once here, after 8 steps of fresh seeds under a static camera cycling
                     jitter_phases, filtered by svgf_filter_tensor: `sigma_0.5`, `sigma_0.25` (sigma_sample);
                     `*_state` the same before the filter. Reported, not targets.
Nothing is gated on.

  python tools/temporal_upsample_bench.py [--width W --height H --reps N]
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
UP_NAMES = ("id", "normal", "albedo")
GUIDES = ("normal", "world_pos", "albedo")
QUALITY_STEPS = 8
REF_SPP = 1024
LOW_SPP = 4         # as many primary samples as the full-resolution chain's 1 spp
SIGMAS = (0.5, 0.25)


def temporal_upsample_bytes(w, h, lw, lh):
    """Bytes one history step must move: per output pixel id (4 B), normal and motion (16 B each), the
    previous color, moment2 and normal (16 B each) and id (4 B) read, color, moment2 and color_std
    (16 B each) written; per low pixel colour and normal (16 B each) and id (4 B) read once."""
    return w * h * (4 + 2 * 16 + 3 * 16 + 4 + 3 * 16) + lw * lh * (2 * 16 + 4)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--height", type=int, default=720)
    ap.add_argument("--depth", type=int, default=8)
    ap.add_argument("--reps", type=int, default=40, help="timed repetitions (>= 20)")
    args = ap.parse_args(argv)
    if args.reps < 20:
        ap.error("--reps must be >= 20")
    if args.width % 2 or args.height % 2:
        ap.error("--width and --height must be even (the low frame is half of each)")

    import torch

    if not torch.cuda.is_available():
        sys.exit("temporal_upsample_bench: needs a GPU (there is no CPU path)")
    import learnraytracing_amd as lrt
    from learnraytracing_amd import _lib as L

    w, h = args.width, args.height
    lw, lh = w // 2, h // 2
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    lrt.InitializeTest()
    rnd = lambda d: {k: round(v, 4) for k, v in d.items()}   # noqa: E731
    try:
        s = torch.cuda.Stream(dev)
        cam = lrt.default_camera(w, h)
        phases = lrt.jitter_phases(w, lw, h, lh)
        jcams = [lrt.jitter_camera(cam, w, h, lw, lh, *p) for p in phases]
        nbytes = temporal_upsample_bytes(w, h, lw, lh)
        with torch.cuda.stream(s):
            high = lrt.gbuffer_tensor(w, h, cam, id=True, stream=s)
            high = {k: high[k] for k in UP_NAMES}
            lowg = {"id": torch.zeros((lh, lw), dtype=torch.int32, device=dev), "normal": torch.zeros((lh, lw, 4), device=dev)}
            out = torch.zeros((h, w, 4), device=dev)
            cls = torch.zeros((h, w), dtype=torch.int32, device=dev)
            buf_low, buf_full = torch.zeros((lh, lw, 4), device=dev), torch.zeros((h, w, 4), device=dev)
            flt_low, flt_full = torch.zeros((lh, lw, 4), device=dev), torch.zeros((h, w, 4), device=dev)
            rays = torch.zeros(1, dtype=torch.int64, device=dev)
            fill = torch.zeros(nbytes, dtype=torch.uint8, device=dev)
        line = {"tool": "temporal_upsample_bench", "width": w, "height": h, "low_width": lw, "low_height": lh,
                "depth": args.depth, "reps": args.reps, "temporal_upsample_bytes": nbytes, "scenes": {}}

        def put(o, name, t):
            o[name] = round(t["median"], 4)
            o[name + "_spread"] = rnd(t)

        def filler():
            with torch.cuda.stream(s):
                fill.fill_(1)

        def chain(acc, buf, flt, ww, hh, spp):
            """upsample_bench's chain: one frame at ww x hh into flt."""
            lrt.render_tensor(lrt.Job(width=ww, height=hh, frames=spp, max_depth=args.depth, camera=cam, flags=POOL), buf, rays,
                              stream=s)
            planes = lrt.gbuffer_tensor(ww, hh, cam, out=acc.gbuffer_planes(), stream=s)
            acc.step_gbuffer(buf, planes, stream=s)
            st = acc.state
            lrt.svgf_filter_tensor(st["color"], st["moment2"], {k: planes[k] for k in GUIDES}, out=flt, stream=s)
            return planes

        def half(acc):
            low = chain(acc, buf_low, flt_low, lw, lh, LOW_SPP)
            lrt.gbuffer_tensor(w, h, cam, out=high, stream=s)
            return lrt.upsample_tensor(flt_low, {k: low[k] for k in UP_NAMES}, high, out=out, stream=s)

        def temporal(up, t=0, fresh=False, class_out=None, **kw):
            """One frame of the new chain into flt_full; fresh: sample t's seeds into a zeroed buffer."""
            p = t % len(phases)
            if fresh:
                buf_low.zero_()
            job = lrt.Job(width=lw, height=lh, frame0=t * LOW_SPP if fresh else 0, frames=LOW_SPP, max_depth=args.depth,
                          camera=jcams[p], flags=POOL)
            lrt.render_tensor(job, buf_low, rays, stream=s)
            lrt.gbuffer_tensor(lw, lh, jcams[p], out=lowg, stream=s)
            planes = lrt.gbuffer_tensor(w, h, cam, out=up.gbuffer_planes(), stream=s)
            up.step(buf_low, lowg, planes, jitter=phases[p], cur_scale=float(t + 1) if fresh else 1.0, class_out=class_out,
                    stream=s, **kw)
            st = up.state
            lrt.svgf_filter_tensor(st["color"], st["moment2"], {k: planes[k] for k in GUIDES}, out=flt_full, stream=s)
            return planes

        def relmse(x, ref):
            x, ref = x[..., :3].double(), ref[..., :3].double()
            return float((((x - ref) ** 2).sum(-1) / ((ref ** 2).sum(-1) + 0.01)).mean())

        scenes = {"default": lrt.default_scene(), "random1000": lrt.random_scene(1000, 1)}
        try:
            for label, (sph, mats) in scenes.items():
                lrt.set_scene(sph, mats)
                o = {"spheres": len(sph)}
                with torch.cuda.stream(s):
                    up = lrt.TemporalUpsampler(w, h, lw, lh, dev)
                    acc_l, acc_f = lrt.TemporalAccumulator(lw, lh, dev), lrt.TemporalAccumulator(w, h, dev)
                    first = temporal(up)
                    prev_g = {k: first[k] for k in ("normal", "id")}
                    prev = {k: v.clone() for k, v in up.state.items()}
                    second = temporal(up, 1, class_out=cls)
                    nxt = {k: torch.zeros((h, w, 4), device=dev) for k in ("color", "moment2", "color_std")}
                s.synchronize()
                o["classes"] = torch.bincount(cls.ravel(), minlength=4)[:4].tolist()
                # the step alone: the second frame's planes against the first's, as the chain just ran it
                put(o, "temporal_upsample_ms", timed(torch, s, lambda: lrt.temporal_upsample_tensor(
                    buf_low, lowg, second, prev_g, prev, out=nxt, jitter=phases[1], stream=s), args.reps))
                put(o, "fill_ms", timed(torch, s, filler, args.reps))
                o["temporal_upsample_over_fill"] = round(o["temporal_upsample_ms"] / o["fill_ms"], 3)
                o["temporal_upsample_gbytes_per_s"] = round(nbytes / (o["temporal_upsample_ms"] * 1e-3) / 1e9, 1)
                put(o, "chain_temporal_ms", timed(torch, s, lambda: temporal(up), args.reps))
                put(o, "chain_half_ms", timed(torch, s, lambda: half(acc_l), args.reps))
                put(o, "chain_full_ms", timed(torch, s, lambda: chain(acc_f, buf_full, flt_full, w, h, 1), args.reps))
                o["temporal_over_full"] = round(o["chain_temporal_ms"] / o["chain_full_ms"], 3)
                # quality: the reference once, then QUALITY_STEPS steps of fresh seeds per sigma_sample
                with torch.cuda.stream(s):
                    ref = torch.zeros((h, w, 4), device=dev)
                    lrt.render_tensor(lrt.Job(width=w, height=h, frames=REF_SPP, max_depth=args.depth, camera=cam,
                                              flags=POOL), ref, rays, stream=s)
                    o["relmse"] = {}
                    for sigma in SIGMAS:
                        up.reset()
                        for t in range(QUALITY_STEPS):
                            temporal(up, t, True, sigma_sample=sigma)
                        s.synchronize()
                        o["relmse"][f"sigma_{sigma}"] = round(relmse(flt_full, ref), 6)
                        o["relmse"][f"sigma_{sigma}_state"] = round(relmse(up.state["color"], ref), 6)
                line["scenes"][label] = o
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
