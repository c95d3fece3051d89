#!/usr/bin/env python3
"""Time one temporal accumulation step (lrt_temporal_accumulate_device) on the headline frame:
1280x720, the default scene at depth 8, 1 spp per time step, two cameras of the orbit
lookFrom = (3 sin t, 2, 3 cos t) one step (0.02 rad) apart, default parameters, albedo and color_std
on. Prints one JSON line.

Method (as bench.py and tools/denoise_bench.py): warm-up calls, then untimed calls until 25 ms of
load have passed (the shader clock settles under load), then >= 20 timed repetitions, each between
two device events on the stream. The timed step blends the second camera's frame into the state the
first camera's frame left. Bytes: what the step must move at least -- every input, history and
output buffer once -- against which the same session's device-to-device copy moving that many bytes
(reads plus writes) is the yardstick; render_4spp_ms (the plain 4 spp render of the frame) and
denoise_ms (the 5-pass denoise of the accumulated frame) are there for scale.

  python tools/temporal_bench.py [--width W --height H --reps N --dtheta RAD] [--moving] [--gbuffer] [--images DIR]

--moving adds the step under moving spheres (lrt_temporal_accumulate_moving_device) on the same
camera pair: moving_step_ms (the default scene, one sphere translated between the two frames, no
motion output), moving_step_motion_ms (with it), moving_step_1000_ms (random_scene(1000, 1), no
motion output) and moving_over_static = moving_step_ms / step_ms. Without the flag the line is the
one it always was.

--gbuffer adds the step driven by the G-buffer's ids and motion vectors
(lrt_temporal_accumulate_gbuffer_device) on the same camera pair, its colours from the pool kernel:
gbuffer_step_ms (the default scene, one sphere translated between the two frames),
gbuffer_step_1000_ms (the same on random_scene(1000, 1)), gbuffer_pass_ms (the G-buffer call that
feeds it: normal, world_pos, albedo, motion and id) and gbuffer_step_bytes; the line's step_ms, and
the moving figures where --moving is given too, are the same session's.
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
# --moving: the step under moving spheres, one sphere translated by MOVING_STEP between the two
# frames -- the default scene without and with motion vectors, and random_scene(1000, 1) without
MOVING_FIELDS = ("moving_step_ms", "moving_step_motion_ms", "moving_step_1000_ms")
MOVING_STEP = 0.1
# --gbuffer: the step driven by the G-buffer, and the pass that feeds it
GBUFFER_FIELDS = ("gbuffer_step_ms", "gbuffer_step_1000_ms", "gbuffer_pass_ms")
POOL = 512   # LRT_F_POOL


def step_bytes(albedo=True, color_std=True):
    """Bytes per pixel one step must move: the current colour, normal, world_pos (and albedo) read,
    16 B each; the history's colour, moment2, normal and world_pos read, 16 B each (a bilinear
    gather touches every history pixel about once); colour (12 B: its alpha stays), moment2, normal,
    world_pos (and albedo, 16 B each, and color_std, 12 B) written."""
    return 16 * (3 + albedo) + 16 * 4 + 12 + 16 * (3 + albedo) + 12 * color_std


def gbuffer_step_bytes(color_std=True):
    """Bytes per pixel the G-buffer step must move: the current colour, normal and motion (16 B each)
    and id (4 B) read; the history's colour, moment2 and normal (16 B each) and id (4 B) read (a
    bilinear gather touches every history pixel about once); colour (12 B: its alpha stays), moment2
    (16 B) and color_std (12 B) written."""
    return (16 * 3 + 4) + (16 * 3 + 4) + 12 + 16 + 12 * color_std


def orbit_args(theta, w, h):
    look_from = (3.0 * np.sin(theta), 2.0, 3.0 * np.cos(theta))
    return look_from, (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), 60.0, w / h, 0.1, float(np.linalg.norm(look_from))


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
    ap.add_argument("--depth", type=int, default=8)
    ap.add_argument("--dtheta", type=float, default=0.02, help="the orbit step between the two cameras (rad)")
    ap.add_argument("--reps", type=int, default=40, help="timed repetitions (>= 20)")
    ap.add_argument("--moving", action="store_true",
                    help="also time lrt_temporal_accumulate_moving_device (the MOVING_FIELDS of the line)")
    ap.add_argument("--gbuffer", action="store_true",
                    help="also time lrt_temporal_accumulate_gbuffer_device and its G-buffer pass (the GBUFFER_FIELDS)")
    ap.add_argument("--images", metavar="DIR",
                    help="write the 1 spp, accumulated and accumulated-then-denoised frames of 16 orbit steps there")
    args = ap.parse_args(argv)
    if args.reps < 20:
        ap.error("--reps must be >= 20")

    import torch

    if not torch.cuda.is_available():
        sys.exit("temporal_bench: needs a GPU (there is no CPU path)")
    import learnraytracing_amd as lrt
    from learnraytracing_amd import _lib as L
    from learnraytracing_amd import image

    w, h = args.width, args.height
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    lrt.InitializeTest()
    try:
        s = torch.cuda.Stream(dev)
        frame = lambda: torch.zeros((h, w, 4), device=dev)   # noqa: E731

        def render(cam, t):
            """Time step t's fresh 1 spp frame and features (sample t into zeroed buffers) on s."""
            with torch.cuda.stream(s):
                buf, feats = frame(), {n: frame() for n in CUR}
                lrt.render_tensor_features(lrt.Job(width=w, height=h, frame0=t, frames=1, max_depth=args.depth,
                                                   camera=cam), buf, rays, feats, -1, stream=s)
            return buf, feats

        with torch.cuda.stream(s):
            rays = torch.zeros(1, dtype=torch.int64, device=dev)
        cam0, cam1 = (lrt.make_camera(*orbit_args(t, w, h)) for t in (-args.dtheta, 0.0))
        buf0, feats0 = render(cam0, 0)
        buf1, feats1 = render(cam1, 1)
        first = lrt.temporal_accumulate_tensor(buf0, feats0, None, cam0, stream=s, cur_scale=1.0)
        prev = {n: first[n] for n in L.TEMPORAL_STATE_NAMES}
        with torch.cuda.stream(s):
            nxt = {n: frame() for n in L.TEMPORAL_STATE_NAMES + ("color_std",)}
            den, buf4 = frame(), frame()
        s.synchronize()

        def step():
            lrt.temporal_accumulate_tensor(buf1, feats1, prev, cam1, cam0, out=nxt, stream=s, cur_scale=2.0)

        per_pixel = step_bytes()
        moved = per_pixel * w * h
        with torch.cuda.stream(s):   # a copy of moved / 2 bytes reads and writes `moved` bytes
            src = torch.zeros(moved // 8, dtype=torch.float32, device=dev)
            dst = torch.zeros_like(src)

        def copy():
            with torch.cuda.stream(s):
                dst.copy_(src, non_blocking=True)

        job4 = lrt.Job(width=w, height=h, frames=4, max_depth=args.depth, camera=cam1)
        t_step = timed(torch, s, step, args.reps)
        t_copy = timed(torch, s, copy, args.reps)
        t_render = timed(torch, s, lambda: lrt.render_tensor(job4, buf4, rays, stream=s), args.reps)
        guides = {n: nxt[n] for n in L.GUIDE_NAMES}
        t_den = timed(torch, s, lambda: lrt.denoise_tensor(nxt["color"], guides, out=den, stream=s), args.reps)
        s.synchronize()
        kept = float((nxt["moment2"][..., 3] > 1.5).float().mean().item())
        rnd = lambda d: {k: round(v, 4) for k, v in d.items()}   # noqa: E731
        line = {
            "tool": "temporal_bench", "width": w, "height": h, "depth": args.depth, "dtheta": args.dtheta,
            "reps": args.reps,
            "step_ms": round(t_step["median"], 4), "step_ms_spread": rnd(t_step),
            "bytes_per_pixel": per_pixel,
            "gbytes_per_s": round(moved / (t_step["median"] * 1e-3) / 1e9, 1),
            "copy_ms": round(t_copy["median"], 4), "copy_ms_spread": rnd(t_copy),
            "copy_gbytes_per_s": round(moved / (t_copy["median"] * 1e-3) / 1e9, 1),
            "step_over_copy": round(t_step["median"] / t_copy["median"], 3),
            "history_kept": round(kept, 4),
            "render_4spp_ms": round(t_render["median"], 4), "render_ms_spread": rnd(t_render),
            "denoise_ms": round(t_den["median"], 4), "denoise_ms_spread": rnd(t_den),
            "version": L.lib().lrt_version().decode(),
        }
        if args.moving:
            motion = frame()

            def moving_leg(spheres, mats, moved, with_motion):
                """Median ms of the moving step on the scene `spheres` whose sphere `moved` came
                MOVING_STEP along x: the previous state is the previous scene's frame from cam0."""
                before = list(spheres)
                c = before[moved].center
                before[moved] = L.Sphere(L.f3(c.x - MOVING_STEP, c.y, c.z), before[moved].radius)
                lrt.set_scene(before, mats)
                b0, f0 = render(cam0, 0)
                lrt.set_scene(spheres, mats)
                b1, f1 = render(cam1, 1)
                st = lrt.temporal_accumulate_tensor(b0, f0, None, cam0, stream=s, cur_scale=1.0)
                pv = {n: st[n] for n in L.TEMPORAL_STATE_NAMES}
                s.synchronize()
                return timed(torch, s, lambda: lrt.temporal_accumulate_moving_tensor(
                    b1, f1, pv, cam1, cam0, spheres, before, out=nxt, motion=motion if with_motion else None,
                    stream=s, cur_scale=2.0), args.reps)

            sph9, mat9 = lrt.default_scene()
            sph1000, mat1000 = lrt.random_scene(1000, 1)
            try:
                t_mov = moving_leg(sph9, mat9, 2, False)
                t_mot = moving_leg(sph9, mat9, 2, True)
                t_1000 = moving_leg(sph1000, mat1000, 500, False)
            finally:
                lrt.set_scene(sph9, mat9)
            s.synchronize()
            for name, t in zip(MOVING_FIELDS, (t_mov, t_mot, t_1000)):
                line[name] = round(t["median"], 4)
                line[name + "_spread"] = rnd(t)
            line["moving_over_static"] = round(t_mov["median"] / t_step["median"], 3)
        if args.gbuffer:
            planes = ("normal", "world_pos", "albedo", "motion", "id")

            def gbuffer_leg(spheres, mats, moved):
                """Median ms of the G-buffer step, of the five-plane pass that feeds it and of a
                guides-only pass (what feeds the moving step), on the scene `spheres` whose sphere
                `moved` came MOVING_STEP along x: the previous state is the previous scene's
                pool-kernel frame from cam0."""
                before = list(spheres)
                c = before[moved].center
                before[moved] = L.Sphere(L.f3(c.x - MOVING_STEP, c.y, c.z), before[moved].radius)

                def pool(cam, t):
                    with torch.cuda.stream(s):
                        buf = frame()
                    lrt.render_tensor(lrt.Job(width=w, height=h, frame0=t, frames=1, max_depth=args.depth, camera=cam,
                                              flags=POOL), buf, rays, stream=s)
                    return buf

                lrt.set_scene(before, mats)
                b0 = pool(cam0, 0)
                g0 = lrt.gbuffer_tensor(w, h, cam0, id=True, motion=True, stream=s)
                lrt.set_scene(spheres, mats)
                b1 = pool(cam1, 1)
                g1 = lrt.gbuffer_tensor(w, h, cam1, cam0, id=True, motion=True, prev_spheres=before, stream=s)
                st = lrt.temporal_accumulate_gbuffer_tensor(b0, g0, None, None, stream=s, cur_scale=1.0)
                out = {n: nxt[n] for n in ("color", "moment2", "color_std")}
                s.synchronize()
                t_st = timed(torch, s, lambda: lrt.temporal_accumulate_gbuffer_tensor(
                    b1, g1, g0, st, out=out, stream=s, cur_scale=2.0), args.reps)
                gout = {n: g1[n] for n in planes}
                sph_a, before_a = (L.Sphere * len(before))(*spheres), (L.Sphere * len(before))(*before)   # marshalled once
                t_gb = timed(torch, s, lambda: lrt.gbuffer_tensor(w, h, cam1, cam0, spheres=sph_a, prev_spheres=before_a,
                                                                  out=gout, stream=s), args.reps)
                guides = {n: g1[n] for n in ("normal", "world_pos", "albedo")}   # what the moving step takes
                t_gd = timed(torch, s, lambda: lrt.gbuffer_tensor(w, h, cam1, out=guides, stream=s), args.reps)
                s.synchronize()
                return t_st, t_gb, t_gd, float((nxt["moment2"][..., 3] > 1.5).float().mean().item())

            sph9, mat9 = lrt.default_scene()
            sph1000, mat1000 = lrt.random_scene(1000, 1)
            try:
                t_g9, t_pass9, t_guides9, kept9 = gbuffer_leg(sph9, mat9, 2)
                t_g1000, t_pass1000, t_guides1000, _ = gbuffer_leg(sph1000, mat1000, 500)
            finally:
                lrt.set_scene(sph9, mat9)
            s.synchronize()
            for name, t in zip(GBUFFER_FIELDS, (t_g9, t_g1000, t_pass9)):
                line[name] = round(t["median"], 4)
                line[name + "_spread"] = rnd(t)
            line["gbuffer_pass_1000_ms"] = round(t_pass1000["median"], 4)
            line["gbuffer_guides_ms"] = round(t_guides9["median"], 4)        # the three guides alone, for scale
            line["gbuffer_guides_1000_ms"] = round(t_guides1000["median"], 4)
            line["gbuffer_step_bytes"] = gbuffer_step_bytes()
            line["gbuffer_history_kept"] = round(kept9, 4)
            line["gbuffer_over_static"] = round(t_g9["median"] / t_step["median"], 3)
        if args.images:
            os.makedirs(args.images, exist_ok=True)
            steps = 16
            with torch.cuda.stream(s):
                acc = lrt.TemporalAccumulator(w, h, dev)
                for t in range(steps):
                    cam = lrt.make_camera(*orbit_args((t - steps + 1) * args.dtheta, w, h))
                    buf, feats = render(cam, t)
                    col, g = acc.step(buf, feats, cam, cur_scale=t + 1, stream=s)
                lrt.denoise_tensor(col, g, out=den, stream=s)
                bgra = torch.zeros(w * h, dtype=torch.int32, device=dev)
                for name, t in (("frame_1spp", buf * float(steps)), ("accumulated", col),
                                ("accumulated_denoised", den)):
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
