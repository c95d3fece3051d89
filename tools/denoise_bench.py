#!/usr/bin/env python3
"""Time the denoiser (lrt_denoise_device) on the headline frame: 1280x720, the default scene's
4 spp / depth 8 render with features, default parameters (5 iterations). Prints one JSON line.

Method (as bench.py): warm-up calls, then untimed calls until 25 ms of load have passed (the shader
clock settles under load), then >= 20 timed repetitions, each between two device events on the
stream. The total is the 5-iteration call; iteration k's time is the difference of the medians of
the (k+1)- and k-iteration calls (the C-ABI has no single-pass call; the last pass of every call
stores 12 B per pixel instead of 16). render_4spp_ms times the render that produces the frame and
its features, for scale. Bytes: what the passes request from the memory system, from the tile
geometry, against the 64 B per pixel a pass must read at least (colour and three guides).

  python tools/denoise_bench.py [--width W --height H --reps N] [--images DIR]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HOLD_SECONDS = 0.025
TILE_W, TILE_ROWS = 64, 4       # lrt_atrous.h: kTileW, kTileRows
MIN_BYTES_PER_PIXEL = 64        # colour + normal + world_pos + albedo, 16 B each, read once


def pass_bytes(w, h, s, last):
    """Bytes one pass at dilation s requests: every workgroup stages (TILE_ROWS + 4) lattice rows x
    (TILE_W + 4 s) columns of four 16 B buffers (clipped to the image), reads one 16 B std per pixel
    and stores 16 B (12 B in the last pass) per pixel."""
    staged = 0
    for x0 in range(0, w, TILE_W):
        cols = min(w, x0 + TILE_W + 2 * s) - max(0, x0 - 2 * s)
        for g0 in range(0, h, TILE_ROWS * s):
            for ph in range(s):
                y0 = g0 + ph
                if y0 >= h:
                    break
                rows = sum(1 for r in range(-2, TILE_ROWS + 2) if 0 <= y0 + r * s < h)
                staged += rows * cols
    return staged * 64 + w * h * (16 + (12 if last else 16))


def timed(torch, stream, fn, reps):
    """Median / min / max ms of fn() over reps repetitions, after warm-up and the 25 ms hold."""
    for _ in range(3):
        fn()
    stream.synchronize()
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < HOLD_SECONDS:
        for _ in range(4):
            fn()
        stream.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for a, b in ev:
        a.record(stream)
        fn()
        b.record(stream)
    stream.synchronize()
    ms = sorted(a.elapsed_time(b) for a, b in ev)
    return {"median": statistics.median(ms), "min": ms[0], "max": ms[-1],
            "p10": ms[len(ms) // 10], "p90": ms[(len(ms) * 9) // 10]}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--height", type=int, default=720)
    ap.add_argument("--spp", type=int, default=4)
    ap.add_argument("--depth", type=int, default=8)
    ap.add_argument("--reps", type=int, default=40, help="timed repetitions (>= 20)")
    ap.add_argument("--images", metavar="DIR", help="write before/after PFM and PPM there")
    args = ap.parse_args(argv)
    if args.reps < 20:
        ap.error("--reps must be >= 20")

    import torch

    if not torch.cuda.is_available():
        sys.exit("denoise_bench: needs a GPU (there is no CPU path)")
    import learnraytracing_amd as lrt
    from learnraytracing_amd import _lib as L
    from learnraytracing_amd import image

    w, h = args.width, args.height
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    lrt.InitializeTest()
    try:
        s = torch.cuda.Stream(dev)
        job = lrt.Job(width=w, height=h, frames=args.spp, max_depth=args.depth)
        with torch.cuda.stream(s):
            buf = torch.zeros((h, w, 4), device=dev)
            feats = {n: torch.zeros((h, w, 4), device=dev) for n in L.FEATURE_NAMES}
            rays = torch.zeros(1, dtype=torch.int64, device=dev)
            out = torch.zeros((h, w, 4), device=dev)
            lrt.render_tensor_features(job, buf, rays, feats, 4, stream=s)
        s.synchronize()
        guides = {n: feats[n] for n in L.GUIDE_NAMES}
        desc = lrt.denoise_desc(w, h)
        iters = desc.iterations

        def plain_render():   # the frame alone, as the headline benchmark renders it (no features)
            lrt.render_tensor(job, buf2, rays, stream=s)

        with torch.cuda.stream(s):
            buf2 = torch.zeros((h, w, 4), device=dev)
        render = timed(torch, s, plain_render, args.reps)
        calls = {}
        for k in range(1, iters + 1):
            calls[k] = timed(torch, s, lambda k=k: lrt.denoise_tensor(buf, guides, out=out, stream=s, iterations=k),
                             args.reps)
        per_iter = [calls[1]["median"]] + [calls[k]["median"] - calls[k - 1]["median"] for k in range(2, iters + 1)]
        moved = [pass_bytes(w, h, 1 << k, k == iters - 1) for k in range(iters)]
        total = calls[iters]
        line = {
            "tool": "denoise_bench", "width": w, "height": h, "spp": args.spp, "depth": args.depth,
            "iterations": iters, "reps": args.reps,
            "denoise_ms": round(total["median"], 4),
            "denoise_ms_spread": {k: round(v, 4) for k, v in total.items()},
            "iteration_ms": [round(v, 4) for v in per_iter],
            "calls_ms": {str(k): {m: round(v, 4) for m, v in c.items()} for k, c in calls.items()},
            "render_4spp_ms": round(render["median"], 4),
            "render_ms_spread": {k: round(v, 4) for k, v in render.items()},
            "bytes_per_pixel_per_iteration": [round(b / (w * h), 1) for b in moved],
            "min_bytes_per_pixel": MIN_BYTES_PER_PIXEL,
            "gbytes_per_s": round(sum(moved) / (total["median"] * 1e-3) / 1e9, 1),
            "version": L.lib().lrt_version().decode(),
        }
        if args.images:
            os.makedirs(args.images, exist_ok=True)
            with torch.cuda.stream(s):
                lrt.denoise_tensor(buf, guides, out=out, stream=s)
                bgra = torch.zeros(w * h, dtype=torch.int32, device=dev)
                for name, t in (("noisy", buf), ("denoised", out)):
                    lrt.renderer.present_tensor(t, bgra, w, h, stream=s)
                    s.synchronize()
                    image.save_pfm(os.path.join(args.images, f"{name}.pfm"), t.cpu().numpy())
                    image.save_ppm_bgra(os.path.join(args.images, f"{name}.ppm"),
                                        bgra.cpu().numpy().view("uint32"), w, h)
            line["images"] = args.images
        print(json.dumps(line), flush=True)
    finally:
        lrt.ShutdownTest()
    return 0


if __name__ == "__main__":
    sys.exit(main())
