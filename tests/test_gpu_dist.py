"""The N>1 path on the GPU box with two ranks sharing GPU 0 over gloo (RCCL refuses two
ranks on one device, so the RCCL gather itself runs only in the driver's multi-GPU
bench): each rank renders its row-block-cyclic shard with the HIP kernels, the shards go
to rank 0 through learnraytracing_amd.dist.gather_to_root, rank 0 assembles them with the
unshard kernel, and the frame equals a one-rank render bit for bit. Also runs bench.py's
multi-rank path end to end."""
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, w, h, rb, frames, depth, outdir, backend="gloo"):
    sys.path.insert(0, ROOT)
    import torch
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.cuda.set_device(0)
    if backend == "nccl":   # RCCL: one rank per GPU, so one rank on this 1-GPU box
        dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda", 0))
    else:
        dist.init_process_group(backend, rank=rank, world_size=world)
    import learnraytracing_amd as lrt
    from learnraytracing_amd.dist import gather_to_root, max_shard_rows
    from learnraytracing_amd.renderer import pack_rgb_tensor, unshard_rgb_tensor, unshard_tensor
    lrt.InitializeTest()
    try:
        max_rows = max_shard_rows(h, rb, world)
        local = torch.zeros((max_rows, w, 4), dtype=torch.float32, device="cuda")
        rays = torch.zeros(1, dtype=torch.int64, device="cuda")
        job = lrt.Job(width=w, height=h, frames=frames, max_depth=depth, row_block=rb, row_period=world,
                      row_phase=rank)
        lrt.render_tensor(job, local, rays)
        packed = torch.empty((max_rows, w, 3), dtype=torch.float32, device="cuda")
        pack_rgb_tensor(local, packed)
        torch.cuda.synchronize()
        gathered, _ = gather_to_root(local, max_rows, world, rank)       # RGBA exchange
        gathered3, _ = gather_to_root(packed, max_rows, world, rank)     # RGB exchange (bench.py's)
        tot = rays.clone() if backend == "nccl" else rays.cpu()   # RCCL reduces device tensors
        dist.all_reduce(tot)
        tot = tot.cpu()
        if rank == 0:
            frame = torch.zeros((h, w, 4), dtype=torch.float32, device="cuda")
            unshard_tensor(gathered, frame, w, h, rb, world)
            frame3 = torch.full((h, w, 4), 0.5, dtype=torch.float32, device="cuda")
            unshard_rgb_tensor(gathered3, frame3, w, h, rb, world)
            torch.cuda.synchronize()
            np.save(os.path.join(outdir, "frame.npy"), frame.cpu().numpy())
            np.save(os.path.join(outdir, "frame3.npy"), frame3.cpu().numpy())
            np.save(os.path.join(outdir, "rays.npy"), tot.numpy())
    finally:
        lrt.ShutdownTest()
        dist.destroy_process_group()


@pytest.mark.parametrize("world,rb,frames", [(2, 8, 4), (2, 5, 32)])
def test_two_rank_gpu_shards_assemble_bitwise(gpu, tmp_path, world, rb, frames):
    import torch.multiprocessing as mp
    w, h, depth = 256, 144, 8
    mp.start_processes(_worker, args=(world, _free_port(), w, h, rb, frames, depth, str(tmp_path)),
                       nprocs=world, start_method="spawn", join=True)
    frame = np.load(tmp_path / "frame.npy")
    frame3 = np.load(tmp_path / "frame3.npy")
    want = np.zeros((h, w, 4), np.float32)
    want_rays = gpu.render_host(gpu.Job(width=w, height=h, frames=frames, max_depth=depth), want)
    assert np.array_equal(frame[..., :3].view(np.uint32), want[..., :3].view(np.uint32))
    assert np.array_equal(frame3[..., :3].view(np.uint32), want[..., :3].view(np.uint32))
    assert np.all(frame3[..., 3] == 0.5)   # the RGB exchange leaves the frame's alpha alone
    assert int(np.load(tmp_path / "rays.npy")[0]) == want_rays


def _remote_worker(rank, world, port, w, h, rb, frames, depth, outdir):
    """The fused exchange: rank 0's frame is mapped into every rank over IPC and each rank's
    render stores its finished pixels into it (lrt_render_device_to_frame)."""
    sys.path.insert(0, ROOT)
    import torch
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    import learnraytracing_amd as lrt
    from learnraytracing_amd.dist import SharedFrames, max_shard_rows
    from learnraytracing_amd.renderer import render_tensor_to_frame
    lrt.InitializeTest()
    shared = None
    try:
        shared = SharedFrames(w, h, 1, rank)
        local = torch.zeros((max_shard_rows(h, rb, world), w, 4), dtype=torch.float32, device="cuda")
        rays = torch.zeros(1, dtype=torch.int64, device="cuda")
        job = lrt.Job(width=w, height=h, frames=frames, max_depth=depth, row_block=rb, row_period=world,
                      row_phase=rank)
        render_tensor_to_frame(job, local, rays, shared.ptrs[0])
        torch.cuda.synchronize()
        dist.barrier()   # every rank's render has completed: the frame is assembled
        tot = rays.cpu()
        dist.all_reduce(tot)
        if rank == 0:
            np.save(os.path.join(outdir, "frame.npy"), shared.tensor(0).cpu().numpy())
            np.save(os.path.join(outdir, "rays.npy"), tot.numpy())
        if rank != 0:
            shared.close()
        dist.barrier()
    finally:
        if shared is not None and rank == 0:
            shared.close()
        lrt.ShutdownTest()
        dist.destroy_process_group()


@pytest.mark.parametrize("world,rb,frames", [(2, 8, 4), (3, 5, 32)])
def test_remote_store_exchange_assembles_bitwise(gpu, tmp_path, world, rb, frames):
    """Ranks sharing GPU 0 (gloo for the control plane) write their rows straight into rank 0's
    IPC-mapped frame from the render kernel: the frame equals a one-rank render bit for bit."""
    import torch.multiprocessing as mp
    w, h, depth = 256, 144, 8
    mp.start_processes(_remote_worker, args=(world, _free_port(), w, h, rb, frames, depth, str(tmp_path)),
                       nprocs=world, start_method="spawn", join=True)
    frame = np.load(tmp_path / "frame.npy")
    want = np.zeros((h, w, 4), np.float32)
    want_rays = gpu.render_host(gpu.Job(width=w, height=h, frames=frames, max_depth=depth), want)
    assert np.array_equal(frame[..., :3].view(np.uint32), want[..., :3].view(np.uint32))
    assert int(np.load(tmp_path / "rays.npy")[0]) == want_rays


def test_one_rank_rccl_gather_assembles_bitwise(gpu, tmp_path):
    """The RCCL path itself: a one-rank "nccl" (RCCL) process group, where gather_to_root
    still issues dist.gather (RCCL moves the device shard into rank 0's gathered buffer),
    then the unshard kernels assemble the frame: bit-identical to a plain render."""
    import torch.multiprocessing as mp
    w, h, rb, frames, depth = 256, 144, 8, 4, 8
    mp.start_processes(_worker, args=(1, _free_port(), w, h, rb, frames, depth, str(tmp_path), "nccl"),
                       nprocs=1, start_method="spawn", join=True)
    frame = np.load(tmp_path / "frame.npy")
    frame3 = np.load(tmp_path / "frame3.npy")
    want = np.zeros((h, w, 4), np.float32)
    want_rays = gpu.render_host(gpu.Job(width=w, height=h, frames=frames, max_depth=depth), want)
    assert np.array_equal(frame[..., :3].view(np.uint32), want[..., :3].view(np.uint32))
    assert np.array_equal(frame3[..., :3].view(np.uint32), want[..., :3].view(np.uint32))
    assert int(np.load(tmp_path / "rays.npy")[0]) == want_rays


@pytest.mark.parametrize("scaling,exchange", [("strong", "remote"), ("weak", "remote"), ("strong", "rccl")])
def test_bench_two_ranks_gloo(gpu, scaling, exchange):
    """bench.py --gpus 2 over gloo on one GPU: one JSON line from rank 0 with the
    aggregate of both ranks. Strong scaling (the default) renders config 2's own frame
    (4 spp over the two row shards: exactly the 1-GPU ray count); weak renders 8 spp."""
    env = dict(os.environ, LRT_DIST_BACKEND="gloo")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
           "--master-addr", "127.0.0.1", "--master-port", str(_free_port()), os.path.join(ROOT, "bench.py"),
           "--gpus", "2", "--steps", "3", "--warmup", "1", "--full", "--scaling", scaling, "--exchange", exchange]
    out = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=110)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["scaling"] == scaling and d["cpu_baseline"] is None
    if scaling == "strong":
        assert d["config"]["spp_total"] == 4
        assert d["config"]["rays_per_step"] == 11669343   # config 2's frame, any sharding
    else:
        assert d["config"]["spp_total"] == 8
        assert 2.0e7 < d["config"]["rays_per_step"] < 2.6e7   # ~2 x config 2's 11.67 M rays
    assert d["value"] > 0
    # both exchanges timed in the same line (north_star's RCCL gather beside the IPC stores),
    # their assembled frames identical bit for bit
    ex = d["exchange"]
    assert ex["primary"] == exchange and ex["frames_identical"] is True, ex
    assert set(ex["legs"]) == {"remote", "rccl"} and all(v["value"] > 0 for v in ex["legs"].values()), ex


def test_bench_two_ranks_ipc_refused(gpu):
    """The driver's N > 1 line when IPC mapping is refused on a rank (LRT_BENCH_FORCE_IPC_FAIL):
    the run falls back to the RCCL exchange and the line still carries its timed leg, with the
    remote leg marked refused -- never a line without exchange legs."""
    env = dict(os.environ, LRT_DIST_BACKEND="gloo", LRT_BENCH_FORCE_IPC_FAIL="1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
           "--master-addr", "127.0.0.1", "--master-port", str(_free_port()), os.path.join(ROOT, "bench.py"),
           "--gpus", "2", "--steps", "3", "--warmup", "1", "--full"]
    out = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=110)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [json.loads(l) for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout
    d = lines[0]
    assert d["value"] > 0 and d["config"]["rays_per_step"] == 11669343
    ex = d["exchange"]
    assert ex["primary"] == "rccl" and ex["legs"]["rccl"]["value"] > 0, ex
    assert "refused" in ex["legs"]["remote"] and ex["legs"]["remote"]["refused"], ex
    assert "RCCL gather" in d["config"]["parallelism"]


@pytest.mark.parametrize("kernel,scene", [("pool", "default"), ("wavefront", "default"), ("pool", "scene1000"),
                                          ("v0", "scene1000"), ("pool-bvh", "scene1000")])
def test_fused_frame_store_every_kernel(gpu, kernel, scene):
    """The fused exchange's frame stores (lrt_render_device_to_frame) in every kernel that has
    them -- pool_kernel's round lerp, the wavefront merge (merge_samples, pix0 / GlobalRow), v0
    -- on row-block-cyclic shards of a window with x0, y0 != 0, on the reference scene and on
    the 1000-sphere scene (grid and BVH): the frame the shards assemble in place equals
    render_host's window bit for bit (advisor r3: the pool and wavefront stores were never
    compared with a plain render)."""
    import torch

    from learnraytracing_amd.scene import random_scene
    flags = {"pool": 512, "wavefront": 256, "v0": 2, "pool-bvh": 512 | 1024}[kernel]
    W, H = (640, 360) if scene == "default" else (3840, 2160)
    x0, xc, y0, yc, rb, period = 37, 256, 21, 133, 8, 3
    frames, depth = (4, 8) if scene == "default" else (8, 8)
    if scene == "scene1000":
        gpu.set_scene(*random_scene(1000, 1))
    try:
        want = np.zeros((yc, xc, 4), np.float32)
        gpu.render_host(gpu.Job(width=W, height=H, frames=frames, max_depth=depth, x0=x0, x_count=xc, y0=y0,
                                row_count=yc, flags=flags), want)
        frame = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda")
        rays = torch.zeros(1, dtype=torch.int64, device="cuda")
        for ph in range(period):
            rows = sum(1 for ly in range(yc) if (ly // rb) % period == ph)
            job = gpu.Job(width=W, height=H, frames=frames, max_depth=depth, x0=x0, x_count=xc, y0=y0,
                          row_count=rows, row_block=rb, row_period=period, row_phase=ph, flags=flags)
            buf = torch.zeros((rows, xc, 4), dtype=torch.float32, device="cuda")
            gpu.render_tensor_to_frame(job, buf, rays, frame.data_ptr())
        torch.cuda.synchronize()
        got = frame[y0:y0 + yc, x0:x0 + xc].cpu().numpy()
    finally:
        if scene == "scene1000":
            gpu.set_scene(*gpu.default_scene())
    assert np.array_equal(got[..., :3].view(np.uint32), want[..., :3].view(np.uint32)), kernel


def test_bench_gpus_2_self_launches(gpu):
    """`python bench.py --gpus 2` with no launcher around it (the shape of the driver's
    command) starts its two ranks itself and reports both: n_gpus 2 and config 2's own ray
    count (round-5 verdict, Next 1). Both ranks share GPU 0 (gloo control plane)."""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    env["LRT_DIST_BACKEND"] = "gloo"
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "3", "--warmup", "1",
           "--full", "--no-cpu-baseline"]
    out = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=110)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [json.loads(l) for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout
    d = lines[0]
    assert d["n_gpus"] == 2 and d["value"] > 0 and d["config"]["rays_per_step"] == 11669343, d
    assert d["exchange"]["frames_identical"] is True, d["exchange"]


def test_bench_gpus_4_self_launches_remote_and_rccl(gpu):
    """Four ranks on GPU 0 (more than the two the other tests use): `bench.py --gpus 4`, no
    launcher, config 2 -- the row-block-cyclic shards of 4, both exchanges timed, rank 0's two
    assembled frames identical, and config 2's own ray count across the four shards."""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    env["LRT_DIST_BACKEND"] = "gloo"
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "4", "--steps", "3", "--warmup", "1",
           "--full", "--no-cpu-baseline"]
    out = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=170)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [json.loads(l) for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout
    d = lines[0]
    assert d["n_gpus"] == 4 and d["config"]["rays_per_step"] == 11669343, d
    ex = d["exchange"]
    assert ex["frames_identical"] is True and set(ex["legs"]) == {"remote", "rccl"}, ex


def test_fused_frame_store_with_overlapped_128px_tiles(gpu):
    """Two row shards of a 1920x1080 window rendered at once on two streams, each storing into
    one shared frame (lrt_render_device_to_frame): the second launch overlaps the first, so it
    takes 128-px pool tiles (lrt_last_launch pix=128). The assembled frame equals one plain
    render bit for bit."""
    import torch

    from learnraytracing_amd import _lib as L
    W, H, frames, depth, rb, period = 1920, 1080, 16, 8, 8, 2
    want = np.zeros((H, W, 4), np.float32)
    gpu.render_host(gpu.Job(width=W, height=H, frames=frames, max_depth=depth), want)
    frame = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda")
    rays = torch.zeros(1, dtype=torch.int64, device="cuda")
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    cur = torch.cuda.current_stream()
    pix = []
    bufs = []
    for ph in range(period):
        rows = gpu.shard_rows(H, rb, period, ph)
        bufs.append(torch.zeros((rows, W, 4), dtype=torch.float32, device="cuda"))
    for s in streams:
        s.wait_stream(cur)
    for rep in range(3):   # (the first launches record the tile orders)
        for ph in range(period):
            job = gpu.Job(width=W, height=H, frames=frames, max_depth=depth, row_count=bufs[ph].shape[0],
                          row_block=rb, row_period=period, row_phase=ph)
            bufs[ph].zero_()
            streams[ph].wait_stream(cur)
            gpu.render_tensor_to_frame(job, bufs[ph], rays, frame.data_ptr(), streams[ph])
            pix.append(L.last_launch()["pix"])
        torch.cuda.synchronize()
        got = frame.cpu().numpy()
        assert np.array_equal(got[..., :3].view(np.uint32), want[..., :3].view(np.uint32)), (rep, pix)
    assert "128" in pix, pix
