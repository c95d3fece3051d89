#!/usr/bin/env python3
"""Time G-buffer-guided upsampling (lrt_upsample_device) on the headline frame, 1280x720 from
640x360, for the default scene and random_scene(1000, 1), and the post-process chain at half
resolution plus the upsample against the chain at full resolution. Prints one JSON line.

Method (as tools/temporal_bench.py): warm-up calls, then untimed calls until 25 ms of load have
passed, then >= 20 timed repetitions, each between two device events on the stream; median and
spread. Per scene:
  upsample_ms, upsample_plain_ms   the guided form with albedo planes and without
  bilinear_ms                      the LRT_UP_BILINEAR form (with albedo planes)
  fill_ms, fill_plain_ms           a plain device fill of upsample_bytes() in the same run
  classes                          pixels per class (0: own surface among the four taps, 1: the ring, 2: bilinear)
  chain_half_ms    pool render at 640x360, 4 spp, depth 8 -> G-buffer -> step_gbuffer -> svgf_filter_tensor,
                   then the 1280x720 G-buffer (id, normal, albedo) and the upsample
  chain_full_ms    pool render at 1280x720, 1 spp (as many primary samples) -> G-buffer -> step_gbuffer ->
                   svgf_filter_tensor
  relmse           mean over the pixels of |x - ref|^2 / (|ref|^2 + 0.01) against a 1024 spp render at
                   1280x720 made once here, after 8 steps of fresh seeds under a static camera: `full` (the
                   full-resolution chain), `half_guided`, `half_bilinear`, `half_guided_plain` (no albedo
                   planes). Reported, not targets.
Nothing is gated on. --images DIR writes the four frames of the default scene as PPM.

  python tools/upsample_bench.py [--width W --height H --reps N --images DIR]
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
FRAMES = ("full", "half_guided", "half_bilinear", "half_guided_plain")


def upsample_bytes(w, h, lw, lh, albedo=True):
    """Bytes one call must move: per output pixel id (4 B), normal (and albedo, 16 B each) read and out
    written (16 B); per low pixel colour, normal (and albedo, 16 B each) and id (4 B) read once."""
    return w * h * (4 + 16 + 16 * albedo + 16) + lw * lh * (16 + 4 + 16 + 16 * albedo)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--height", type=int, default=720)
    ap.add_argument("--depth", type=int, default=8)
    ap.add_argument("--reps", type=int, default=40, help="timed repetitions (>= 20)")
    ap.add_argument("--images", metavar="DIR", help="write the four quality frames of the default scene as PPM")
    ap.add_argument("--full-only", action="store_true",
                    help="time chain_full_ms only (runs on a library that predates lrt_upsample_*, through LRT_LIB)")
    args = ap.parse_args(argv)
    if args.reps < 20:
        ap.error("--reps must be >= 20")
    if args.width % 2 or args.height % 2:
        ap.error("--width and --height must be even (the low frame is half of each)")

    import torch

    if not torch.cuda.is_available():
        sys.exit("upsample_bench: needs a GPU (there is no CPU path)")
    import learnraytracing_amd as lrt
    from learnraytracing_amd import _lib as L
    from learnraytracing_amd import image

    w, h = args.width, args.height
    lw, lh = w // 2, h // 2
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    lrt.InitializeTest()
    rnd = lambda d: {k: round(v, 4) for k, v in d.items()}   # noqa: E731
    try:
        s = torch.cuda.Stream(dev)
        cam = lrt.default_camera(w, h)
        with torch.cuda.stream(s):
            high = lrt.gbuffer_tensor(w, h, cam, id=True, stream=s)
            high = {k: high[k] for k in UP_NAMES}
            out = torch.zeros((h, w, 4), device=dev)
            cls = torch.zeros((h, w), dtype=torch.int32, device=dev)
            buf_low, buf_full = torch.zeros((lh, lw, 4), device=dev), torch.zeros((h, w, 4), device=dev)
            flt_low, flt_full = torch.zeros((lh, lw, 4), device=dev), torch.zeros((h, w, 4), device=dev)
            rays = torch.zeros(1, dtype=torch.int64, device=dev)
            fill = torch.zeros(upsample_bytes(w, h, lw, lh), dtype=torch.uint8, device=dev)
        line = {"tool": "upsample_bench", "width": w, "height": h, "low_width": lw, "low_height": lh, "depth": args.depth,
                "reps": args.reps, "upsample_bytes": upsample_bytes(w, h, lw, lh),
                "upsample_plain_bytes": upsample_bytes(w, h, lw, lh, False), "scenes": {}}

        def put(o, name, t):
            o[name] = round(t["median"], 4)
            o[name + "_spread"] = rnd(t)

        def filler(nbytes):
            def fn():
                with torch.cuda.stream(s):
                    fill[:nbytes].fill_(1)
            return fn

        def plain(g):
            return {k: v for k, v in g.items() if k != "albedo"}

        def chain(acc, buf, flt, ww, hh, spp, t=0, fresh=False):
            """One frame of the chain at ww x hh into flt; fresh: sample t's seeds into a zeroed buffer."""
            if fresh:
                buf.zero_()
            job = lrt.Job(width=ww, height=hh, frame0=t * spp if fresh else 0, frames=spp, max_depth=args.depth,
                          camera=cam, flags=POOL)
            lrt.render_tensor(job, buf, rays, stream=s)
            planes = lrt.gbuffer_tensor(ww, hh, cam, out=acc.gbuffer_planes(), stream=s)
            acc.step_gbuffer(buf, planes, cur_scale=float(t + 1) if fresh else 1.0, stream=s)
            st = acc.state
            lrt.svgf_filter_tensor(st["color"], st["moment2"], {k: planes[k] for k in GUIDES}, out=flt, stream=s)
            return planes

        def half(acc, t=0, fresh=False, **kw):
            low = chain(acc, buf_low, flt_low, lw, lh, 4, t, fresh)
            lrt.gbuffer_tensor(w, h, cam, out=high, stream=s)
            lo, hi = ({k: low[k] for k in UP_NAMES}, high)
            if kw.pop("plain", False):
                lo, hi = plain(lo), plain(hi)
            return lrt.upsample_tensor(flt_low, lo, hi, out=out, stream=s, **kw)

        def relmse(x, ref):
            x, ref = x[..., :3].double(), ref[..., :3].double()
            return float((((x - ref) ** 2).sum(-1) / ((ref ** 2).sum(-1) + 0.01)).mean())

        scenes = {"default": lrt.default_scene(), "random1000": lrt.random_scene(1000, 1)}
        try:
            for label, (sph, mats) in scenes.items():
                lrt.set_scene(sph, mats)
                o = {"spheres": len(sph)}
                if args.full_only:
                    with torch.cuda.stream(s):
                        acc_f = lrt.TemporalAccumulator(w, h, dev)
                    put(o, "chain_full_ms", timed(torch, s, lambda: chain(acc_f, buf_full, flt_full, w, h, 1), args.reps))
                    line["scenes"][label] = o
                    continue
                with torch.cuda.stream(s):
                    acc_l, acc_f = lrt.TemporalAccumulator(lw, lh, dev), lrt.TemporalAccumulator(w, h, dev)
                    low = chain(acc_l, buf_low, flt_low, lw, lh, 4)
                    low = {k: low[k] for k in UP_NAMES}
                    lrt.gbuffer_tensor(w, h, cam, out=high, stream=s)
                    lrt.upsample_tensor(flt_low, low, high, out=out, class_out=cls, stream=s)
                s.synchronize()
                o["classes"] = torch.bincount(cls.ravel(), minlength=3)[:3].tolist()
                put(o, "upsample_ms", timed(torch, s, lambda: lrt.upsample_tensor(flt_low, low, high, out=out, stream=s),
                                            args.reps))
                put(o, "upsample_plain_ms", timed(torch, s, lambda: lrt.upsample_tensor(
                    flt_low, plain(low), plain(high), out=out, stream=s), args.reps))
                put(o, "bilinear_ms", timed(torch, s, lambda: lrt.upsample_tensor(
                    flt_low, low, high, out=out, stream=s, flags=L.UP_BILINEAR), args.reps))
                put(o, "fill_ms", timed(torch, s, filler(upsample_bytes(w, h, lw, lh)), args.reps))
                put(o, "fill_plain_ms", timed(torch, s, filler(upsample_bytes(w, h, lw, lh, False)), args.reps))
                o["upsample_over_fill"] = round(o["upsample_ms"] / o["fill_ms"], 3)
                o["upsample_plain_over_fill"] = round(o["upsample_plain_ms"] / o["fill_plain_ms"], 3)
                o["upsample_gbytes_per_s"] = round(upsample_bytes(w, h, lw, lh) / (o["upsample_ms"] * 1e-3) / 1e9, 1)
                put(o, "chain_half_ms", timed(torch, s, lambda: half(acc_l), args.reps))
                put(o, "chain_full_ms", timed(torch, s, lambda: chain(acc_f, buf_full, flt_full, w, h, 1), args.reps))
                o["half_over_full"] = round(o["chain_half_ms"] / o["chain_full_ms"], 3)
                # quality: the reference once, then QUALITY_STEPS steps of fresh seeds per frame
                with torch.cuda.stream(s):
                    ref = torch.zeros((h, w, 4), device=dev)
                    lrt.render_tensor(lrt.Job(width=w, height=h, frames=REF_SPP, max_depth=args.depth, camera=cam,
                                              flags=POOL), ref, rays, stream=s)
                    frames = {}
                    acc = lrt.TemporalAccumulator(w, h, dev)
                    for t in range(QUALITY_STEPS):
                        chain(acc, buf_full, flt_full, w, h, 1, t, True)
                    frames["full"] = flt_full.clone()
                    for name, kw in (("half_guided", {}), ("half_bilinear", dict(flags=L.UP_BILINEAR)),
                                     ("half_guided_plain", dict(plain=True))):
                        acc = lrt.TemporalAccumulator(lw, lh, dev)
                        for t in range(QUALITY_STEPS):
                            half(acc, t, True, **kw)
                        frames[name] = out.clone()
                s.synchronize()
                o["relmse"] = {name: round(relmse(frames[name], ref), 6) for name in FRAMES}
                if args.images and label == "default":
                    os.makedirs(args.images, exist_ok=True)
                    with torch.cuda.stream(s):
                        bgra = torch.zeros(w * h, dtype=torch.int32, device=dev)
                        for name in FRAMES:
                            lrt.renderer.present_tensor(frames[name], bgra, w, h, stream=s)
                            s.synchronize()
                            image.save_ppm_bgra(os.path.join(args.images, f"{name}.ppm"),
                                                bgra.cpu().numpy().view("uint32"), w, h)
                    line["images"] = args.images
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
