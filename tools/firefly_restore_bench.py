#!/usr/bin/env python3
"""Time firefly restore (lrt_firefly_restore_device) on the headline frame, 1280x720, beside a fill
of its bytes and the firefly pass that supplies its excess, in the same process. Prints one JSON
line. Reported, nothing is gated on.

Method (tools/temporal_bench.py's `timed`): warm-up calls, then untimed calls until 25 ms of load
have passed, then >= 20 timed repetitions (default 40), each between two device events on the stream;
the median. The passes are timed alternately, twice each in one process, and both medians of each
are reported: their distance is the run-to-run spread a ratio has to exceed. The input is one 4 spp
pool-kernel frame of the default scene through firefly_tensor(excess_out=True) with its G-buffer's ids.
  restore_ms[form]   one call; forms: r1..r4 (id, a separate out), rN_noid, rN_inplace (out = color),
                     rN_noid_inplace
  fill_ms            a plain device fill of restore_bytes() per pixel (52 B: id and a separate out)
  firefly_excess_ms  firefly_tensor at its defaults with excess_out
  sources            pixels of the frame whose excess is not zero
The quality leg (--quality), for the default scene and random_scene(1000, 1), against 1024 spp:
  luma_ratio, rel_mse           mean Y(out) / mean Y(in) and mean((out - ref)^2 / (ref^2 + 0.01)) over
                                rgb of the 4 spp frame: "raw", "clamped", and "restored" at each radius
  chain                         16 orbit steps of 1 spp -> step_gbuffer -> svgf_filter_tensor, the last
                                filtered frame against 1024 spp from the last camera: the same two
                                numbers (the ratio against the chain without either option) with
                                firefly only and with firefly + firefly_restore at radius 2

  python tools/firefly_restore_bench.py [--width W --height H --reps N --quality]
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
GUIDES = ("normal", "world_pos", "albedo")
SPP, STEPS, DTHETA = 4, 16, 0.02
RADII = (1, 2, 3, 4)


def restore_bytes(ids=True):
    """Bytes per pixel one call must move: the colour quad and the excess quad read (16 B each; the
    neighbours' excess comes from the tile), the id read (4 B), the quad written (16 B, to another
    frame or over the colour: the same bytes in place)."""
    return 16 + 16 + (4 if ids else 0) + 16


def rel_mse(a, ref):
    return float(((a[..., :3] - ref[..., :3]) ** 2 / (ref[..., :3] ** 2 + 0.01)).mean())


def luma(t):
    return 0.2126 * t[..., 0] + 0.7152 * t[..., 1] + 0.0722 * t[..., 2]


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
        sys.exit("firefly_restore_bench: needs a GPU (there is no CPU path)")
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

        def frame(camera, frame0, frames, flags=POOL):
            """The mean of `frames` fresh samples per pixel (a zeroed buffer, the lerp's factor undone)."""
            with torch.cuda.stream(s):
                buf = torch.zeros((h, w, 4), device=dev)
            lrt.render_tensor(lrt.Job(width=w, height=h, frame0=frame0, frames=frames, max_depth=depth, camera=camera,
                                      flags=flags), buf, rays, stream=s)
            if frame0:
                with torch.cuda.stream(s):
                    buf.mul_((frame0 + frames) / frames)
            return buf

        with torch.cuda.stream(s):
            rays = torch.zeros(1, dtype=torch.int64, device=dev)
            out, clamped, exc = (torch.zeros((h, w, 4), device=dev) for _ in range(3))
            fill = torch.zeros(npix * restore_bytes(), dtype=torch.uint8, device=dev)
        line = {"tool": "firefly_restore_bench", "width": w, "height": h, "depth": depth, "reps": args.reps,
                "spp": SPP, "restore_bytes": restore_bytes(), "restore_ms": {}, "restore_ms_runs": {}}
        col = frame(cam, 0, SPP)
        ids = lrt.gbuffer_tensor(w, h, cam, id=True, stream=s)["id"]
        lrt.firefly_tensor(col, ids, out=clamped, excess_out=exc, stream=s)
        with torch.cuda.stream(s):
            work = clamped.clone()              # what the in-place forms overwrite
        s.synchronize()
        line["sources"] = int((exc[..., :3] != 0).any(-1).sum())

        def do_fill():
            with torch.cuda.stream(s):
                fill.fill_(1)

        passes = {"fill_ms": do_fill,
                  "firefly_excess_ms": lambda: lrt.firefly_tensor(col, ids, out=clamped, excess_out=exc, stream=s)}
        for r in RADII:
            for tag, i in (("", ids), ("_noid", None)):
                passes[f"r{r}{tag}"] = lambda r=r, i=i: lrt.firefly_restore_tensor(clamped, exc, i, out=out, stream=s,
                                                                                  radius=r)
                passes[f"r{r}{tag}_inplace"] = lambda r=r, i=i: lrt.firefly_restore_tensor(work, exc, i, out=work,
                                                                                          stream=s, radius=r)
        runs = {name: [] for name in passes}
        for _ in range(2):                      # alternating, twice each
            for name, fn in passes.items():
                runs[name].append(round(timed(torch, s, fn, args.reps)["median"], 4))
        for name, v in runs.items():
            if name.endswith("_ms"):
                line[name], line[name + "_runs"] = min(v), v
            else:
                line["restore_ms"][name], line["restore_ms_runs"][name] = min(v), v
        line["restore_over_fill"] = {k: round(v / line["fill_ms"], 3) for k, v in line["restore_ms"].items()}
        line["restore_over_firefly_excess"] = {k: round(v / line["firefly_excess_ms"], 3)
                                               for k, v in line["restore_ms"].items()}
        line["restore_gbytes_per_s"] = round(npix * restore_bytes() / (line["restore_ms"]["r2"] * 1e-3) / 1e9, 1)

        if args.quality:
            line["quality"] = {}
            scenes = {"default": lrt.default_scene(), "random1000": lrt.random_scene(1000, 1)}
            try:
                for label, (sph, mats) in scenes.items():
                    lrt.set_scene(sph, mats)
                    q = {"spheres": len(sph), "gt_spp": 1024, "luma_ratio": {}, "rel_mse": {}}
                    ref = frame(cam, 0, 1024, flags=0)
                    raw = frame(cam, 0, SPP)
                    g = lrt.gbuffer_tensor(w, h, cam, id=True, stream=s)
                    res = lrt.firefly_tensor(raw, g["id"], excess_out=True, stream=s)
                    frames = {"raw": raw, "clamped": res["out"]}
                    for r in RADII:
                        frames[f"restored_r{r}"] = lrt.firefly_restore_tensor(res["out"], res["excess"], g["id"], stream=s,
                                                                              radius=r)["out"]
                    s.synchronize()
                    y_in = luma(raw).double().mean()
                    for name, f in frames.items():
                        q["luma_ratio"][name] = round(float(luma(f).double().mean() / y_in), 5)
                        q["rel_mse"][name] = round(rel_mse(f, ref), 5)
                    # the orbit chain
                    chain = {}
                    for name, opts in (("plain", {}), ("firefly", dict(firefly={})),
                                       ("firefly_restore_r2", dict(firefly={}, firefly_restore=dict(radius=2)))):
                        a = lrt.TemporalAccumulator(w, h, dev)
                        for t in range(STEPS):
                            c = lrt.make_camera(*orbit_args((t - STEPS + 1) * DTHETA, w, h))
                            pc = lrt.make_camera(*orbit_args((t - STEPS) * DTHETA, w, h))
                            buf = frame(c, t, 1)
                            p = lrt.gbuffer_tensor(w, h, c, pc, out=a.gbuffer_planes(), stream=s)
                            a.step_gbuffer(buf, p, stream=s, **opts)
                        st = a.state
                        flt = lrt.svgf_filter_tensor(st["color"], st["moment2"], {k: p[k] for k in GUIDES}, stream=s)
                        if name == "plain":
                            ref_last = frame(c, 0, 1024, flags=0)
                        s.synchronize()
                        if name == "plain":
                            y_plain = luma(flt).double().mean()
                        chain[name] = {"luma_ratio": round(float(luma(flt).double().mean() / y_plain), 5),
                                       "rel_mse": round(rel_mse(flt, ref_last), 5)}
                    q["chain"] = chain
                    line["quality"][label] = q
            finally:
                lrt.set_scene(*lrt.default_scene())
        line["version"] = L.lib().lrt_version().decode()
        print(json.dumps(line), flush=True)
    finally:
        lrt.ShutdownTest()
    return 0


if __name__ == "__main__":
    sys.exit(main())
