"""Every pool tile size, the round loop, the half tiles and v0's eight frame lanes, vs the oracle.

pool_pixels (lrt_render.hip) picks the pixels per tile from the frame count: 64 up to 64 frames,
32 up to 128, 16 up to 256, 4 up to 1024 and 1 above (kPoolSamples = 4096 samples a round).
launch_pool<MAXD, kPix> compiles its own tile geometry (PoolTile, kLgPix, kLgTX), lerp stage and
slot sizing per size; a tile of one pixel takes a second round above 4096 frames; the split tail
(pool_kernel's kSplit) serves left and right halves of 4x8, 4x4, 2x4 and 1x2 pixels; the probe
(probe_kernel) places its 16 rays by TX and TY. Each case here renders a small window of the
1280x720 default view -- 6 x 5 tiles with a partial top row and right column, whose last
column's right halves lie wholly outside the window -- and compares RGB and the ray count bit
for bit with the C restatement (oracle.orc_render) of the same window; lrt_last_launch() names
the instance that ran, and alpha must come back as given. Cases that start from a seeded buffer
at frame0 = 3 make the lerp chain read the previous value (at frame0 = 0 its factor is 0).
References: parallel.cpp:262,280-286 (the lerp chain), :214 (the fold), :54-73 (HitWorld).
"""
import functools

import numpy as np
import pytest

import oracle
from learnraytracing_amd import _lib as L
from learnraytracing_amd.scene import random_scene, scene_arrays
from test_gpu_pool_trim import BUILD, SCENES, _bitwise

pytestmark = pytest.mark.gpu

GLOBAL, V0, WAVEFRONT, POOL, BVH, GRID = 1, 2, 256, 512, 1024, 2048   # LRT_F_*
W, H = 1280, 720
# rich regions of the view: 3.56 and 4.26 rays per sample (43x27 window, 8 spp, depth 8)
ORIGINS = ((420, 260), (300, 330))
TILE = {64: (8, 8), 32: (8, 4), 16: (4, 4), 4: (2, 2), 1: (1, 1)}   # PoolTile<kPix>
kPoolSamples, kV0Queues, kLerpTable = 4096, 16, 1 << 16
SCENE1000 = dict(size=(3840, 2160), x0=1880, x_count=24, y0=1000, row_count=8)   # config 4's window origin


def pool_pix(frames):
    """pool_pixels for a launch alone (tile cap 64)."""
    return 64 if frames <= 64 else 32 if frames <= 128 else 16 if frames <= 256 else 4 if frames <= 1024 else 1


def window(pix, origin=0):
    """6 x 5 tiles of `pix` pixels: five whole columns and a partial one that ends before its
    tiles' right halves begin, four whole rows and a partial one."""
    tx, ty = TILE[pix]
    x0, y0 = ORIGINS[origin]
    return dict(x0=x0, x_count=5 * tx + max(1, tx // 2 - 1), y0=y0, row_count=4 * ty + max(1, ty - 1))


ORDER_WINDOWS = {32: (67, 35), 16: (35, 35), 4: (17, 17), 1: (9, 9)}   # 9 x 9 tiles, the last ones partial


def seed_buffer(rows, xc):
    """A non-zero, non-uniform RGBA start: what the lerp chain's first step reads."""
    return np.random.default_rng(1000 * rows + xc).uniform(0.05, 2.0, (rows, xc, 4)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _scene1000():
    sph, mat = random_scene(1000, 1)
    return (sph, mat), tuple(np.array(v, np.float32) for v in scene_arrays(sph, mat))


def _render(gpu, flags, init=None, size=(W, H), **kw):
    job = gpu.Job(flags=flags, width=size[0], height=size[1], **kw)
    d = job.desc()
    buf = np.zeros((d.row_count, d.x_count, 4), np.float32) if init is None else init.copy()
    rays = gpu.render_host(job, buf)
    return buf, rays, L.last_launch()


@functools.lru_cache(maxsize=None)
def _want(frames, depth, x0, xc, y0, yc, scene=None, frame0=0, seeded=False, size=(W, H)):
    """The restatement's window, computed once per case and shared."""
    s = m = None
    if scene == "scene1000":
        s, m = _scene1000()[1]
    elif scene is not None:
        s, m = (np.array(v, np.float32) for v in SCENES[scene]())
    buf, rays = oracle.orc_render(size[0], size[1], frames, depth, frame0, x0, xc, y0, yc, spheres=s, mats=m,
                                  buf=seed_buffer(yc, xc) if seeded else None, threads=16)
    buf.setflags(write=False)
    return buf, rays


@pytest.fixture
def scene(gpu, request):
    """A scene of BUILD (or random_scene(1000, 1), or None: the default) for one test, then the
    default scene again (conftest's scene guard)."""
    name = getattr(request, "param", None)
    if name is None:
        yield None
        return
    gpu.set_scene(*(_scene1000()[0] if name == "scene1000" else BUILD[name]()))
    try:
        yield name
    finally:
        gpu.set_scene(*gpu.default_scene())


def _check(gpu, flags, frames, depth, win, scene=None, frame0=0, seeded=False, what=""):
    win = dict(win)
    size = win.pop("size", (W, H))
    init = seed_buffer(win["row_count"], win["x_count"]) if seeded else None
    buf, rays, info = _render(gpu, flags, init, size, frames=frames, frame0=frame0, max_depth=depth, **win)
    want, wrays = _want(frames, depth, win["x0"], win["x_count"], win["y0"], win["row_count"], scene, frame0, seeded, size)
    samples = frames * win["x_count"] * win["row_count"]   # one camera ray each, bounces on top
    print(f"{what} frames {frames} frame0 {frame0} depth {depth} {scene or 'default'} flags {flags}: "
          f"{wrays / samples:.2f} rays per sample; {info}")
    assert wrays == samples if depth == 0 else wrays > 2 * samples, wrays   # no window of sky
    _bitwise(buf, want, f"{what} frames {frames} frame0 {frame0} depth {depth} {scene or 'default'} flags {flags}")
    assert rays == wrays
    alpha = init[..., 3] if seeded else np.zeros(buf.shape[:2], np.float32)
    assert np.array_equal(buf[..., 3].view(np.uint32), alpha.view(np.uint32)), "alpha must come back as given"
    return info


def split_from(tasks, pix, halves, trimmed=False):
    """launch_pool's split tail for a launch alone: the last 8/16 (the trimmed instance) or 5/16
    of the tiles as halves where the instance serves halves (pool_kernel's kSplit: depth <= 8,
    linear scan, one-wave blocks, tiles two or more pixels wide), no tail elsewhere."""
    return tasks - tasks * (8 if trimmed else 5) // 16 if halves and pix >= 4 else tasks


def _assert_pool(info, frames, tasks=30, maxd="8", acc="scan", order="0"):
    pix = pool_pix(frames)
    assert info["kernel"] == "pool_kernel" and info["pix"] == str(pix) and info["maxd"] == maxd, info
    assert info["acc"] == acc and info["tasks"] == str(tasks), info
    assert order is None or info["order"] == order, info
    return pix


# ---- a. tile-size bands, both sides of every boundary --------------------------------------
@pytest.mark.parametrize("start", ["zero", "seeded"])
@pytest.mark.parametrize("frames", [64, 65, 128, 129, 256, 257, 1024, 1025])
def test_tile_size_bands_vs_oracle(gpu, frames, start):
    """The trimmed instance (the benchmark's family) at every tile size: 30 tiles are fewer than
    2 * kV0Queues, so the launch has no tile order, reserves late and serves its split tail at
    once. The seeded start (frame0 = 3, the second origin) makes the first lerp read the buffer."""
    seeded = start == "seeded"
    pix = pool_pix(frames)
    info = _check(gpu, POOL, frames, 8, window(pix, 1 if seeded else 0), frame0=3 if seeded else 0, seeded=seeded,
                  what="bands")
    assert _assert_pool(info, frames) == pix
    assert info["ns"] == "9" and info["nl"] == "1" and info["chk"] == "0" and info["wpb"] == "1", info
    if pix >= 4:
        assert int(info["split_from"]) < int(info["tasks"]), info
    assert int(info["split_from"]) == split_from(30, pix, True, True) == (15 if pix >= 4 else 30), info


# ---- b. rounds --------------------------------------------------------------------------------
@pytest.mark.parametrize("frame0,frames", [(0, 4096), (0, 4097), (5, 8203), (65530, 4100)],
                         ids=["one-full-round", "second-round-of-one-frame", "two-rounds-and-eleven", "past-the-lerp-table"])
def test_rounds_vs_oracle(gpu, frame0, frames):
    """One-pixel tiles above 4096 frames take a second round: the lerp re-reads what the round
    before wrote, the slots are overwritten behind a fence pair, and the late reservation waits
    for the last round. 8203 frames leave the 4-at-a-time chain a remainder of 3; from frame
    65530 the second round lies wholly past the host-divided lerp table."""
    info = _check(gpu, POOL, frames, 8, window(1), frame0=frame0, seeded=frame0 > 0, what="rounds")
    pix = _assert_pool(info, frames)
    rounds = -(-frames * pix // kPoolSamples)
    assert pix == 1 and rounds == (1 if frames == 4096 else 3 if frames == 8203 else 2), (info, rounds)
    if frame0 == 65530:
        assert frame0 < kLerpTable < frame0 + kPoolSamples < frame0 + frames
    assert info["ns"] == "9" and info["nl"] == "1" and info["chk"] == "0", info
    assert int(info["split_from"]) == int(info["tasks"]) == 30, info   # a one-pixel tile has no halves


# ---- c. the other instance families at the tile sizes no other test launches --------------------
FAMILIES = {
    # name: (scene, flags, depth, expected last_launch fields, serves halves)
    "depth20": (None, POOL, 20, dict(maxd="64", acc="scan", ns="9", chk="1", nl="0", lds="1", wpb="1"), False),
    "ten_spheres": ("ten_spheres", POOL, 8, dict(maxd="8", acc="scan", ns="0", chk="1", nl="0", lds="1", wpb="1"), True),
    # (nine spheres keep the fixed-count scan, ns=9; the second light takes the run-time light loop)
    "two_lights": ("two_lights", POOL, 8, dict(maxd="8", acc="scan", ns="9", chk="1", nl="0", lds="1", wpb="1"), True),
    "scene_global": (None, POOL | GLOBAL, 8, dict(maxd="8", acc="scan", ns="0", chk="1", nl="0", lds="0", wpb="1"), True),
    "grid": (None, POOL | GRID, 8, dict(maxd="8", acc="grid", ns="0", chk="1", nl="0", lds="1", wpb="1"), False),
    "scene1000_pick": ("scene1000", POOL, 8, dict(maxd="8", acc="grid", lds="0", wpb="16"), False),
    "scene1000_bvh": ("scene1000", POOL | BVH, 8, dict(maxd="8", acc="bvh", lds="0", wpb="1"), False),
}


@pytest.mark.parametrize("frames", [128, 1024, 1100])
@pytest.mark.parametrize("family,scene", [(k, v[0]) for k, v in FAMILIES.items()], indirect=["scene"],
                         ids=list(FAMILIES))
def test_other_families_at_small_tiles_vs_oracle(gpu, family, scene, frames):
    """Depth 20, the general scan instances, the global-memory scene, the grid (one-wave and
    16-wave blocks) and the BVH at 32-, 4- and 1-pixel tiles. The 1000-sphere window has fewer
    32-pixel tiles (6) than a grid block has waves."""
    _, flags, depth, fields, halves = FAMILIES[family]
    pix = pool_pix(frames)
    win = SCENE1000 if scene == "scene1000" else window(pix, {32: 0, 4: 1, 1: 0}[pix])
    tx, ty = TILE[pix]
    tasks = -(-win["x_count"] // tx) * -(-win["row_count"] // ty)
    info = _check(gpu, flags, frames, depth, win, scene, what=family)
    _assert_pool(info, frames, tasks, fields["maxd"], fields["acc"], "0" if tasks < 2 * kV0Queues else None)
    assert {k: info[k] for k in fields} == fields, info
    if tasks >= 2 * kV0Queues:   # a recording launch times whole tiles
        assert info["order"] in ("3", "4") and int(info["split_from"]) == tasks, info
    else:
        assert int(info["split_from"]) == split_from(tasks, pix, halves), info
        assert tasks != 30 or int(info["split_from"]) == (21 if halves and pix >= 4 else 30), info


# ---- d. order and probe at every tile shape --------------------------------------------------
@pytest.mark.parametrize("frames", [65, 129, 257, 1025], ids=["pix32", "pix16", "pix4", "pix1"])
def test_tile_order_and_probe_at_small_tiles_vs_oracle(gpu, frames):
    """9 x 9 tiles, rendered four times: the first launch records in the probe's (or a borrowed)
    order -- probe_kernel's 16 rays fall on 4 or 1 pixels of a 2x2 or 1x1 tile --, the last takes
    the measured order and, where the tile has halves, serves them through the permutation.
    Every launch equals the restatement."""
    pix = pool_pix(frames)
    xc, rows = ORDER_WINDOWS[pix]
    assert (-(-xc // TILE[pix][0]), -(-rows // TILE[pix][1])) == (9, 9)
    win = dict(x0=ORIGINS[1][0], x_count=xc, y0=ORIGINS[1][1], row_count=rows)
    infos = [_check(gpu, POOL, frames, 8, win, what=f"order launch {k}") for k in range(4)]
    for info in infos:
        _assert_pool(info, frames, 81, order=None)
        assert info["ns"] == "9" and info["nl"] == "1" and info["chk"] == "0", info
    orders = [info["order"] for info in infos]
    assert orders[0] in ("3", "4") and orders[-1] == "2", orders   # recorded, then reordered
    assert int(infos[0]["split_from"]) == 81, infos[0]             # a recording launch times whole tiles
    assert int(infos[-1]["split_from"]) == split_from(81, pix, True, True), infos[-1]
    if pix >= 4:
        assert int(infos[-1]["split_from"]) < int(infos[-1]["tasks"]), infos[-1]


# ---- e. the fused exchange at a small tile ----------------------------------------------------
def test_fused_exchange_at_half_tiles_vs_oracle(gpu):
    """lrt_render_device_to_frame with 8x4 tiles on a row-block-cyclic shard: the tile height
    divides the row block of 8, and the store's my / rb path runs on whole and half tiles. The
    shard buffer and the frame's rows equal the restatement's global rows; every other pixel of
    the frame is untouched."""
    import torch

    frames, frame0, rb, rp, ph = 65, 3, 8, 2, 1
    win = window(32, 1)
    x0, xc, y0, rows = win["x0"], win["x_count"], win["y0"], win["row_count"]
    init = seed_buffer(rows, xc)
    buf = torch.from_numpy(init).cuda()
    frame = torch.full((H, W, 4), -3.0, dtype=torch.float32, device="cuda")
    rays = torch.zeros(1, dtype=torch.int64, device="cuda")
    job = gpu.Job(flags=POOL, width=W, height=H, frames=frames, frame0=frame0, max_depth=8, row_block=rb,
                  row_period=rp, row_phase=ph, **win)
    gpu.render_tensor_to_frame(job, buf, rays, frame.data_ptr())
    info = L.last_launch()
    torch.cuda.synchronize()
    assert _assert_pool(info, frames) == 32 and info["chk"] == "0" and info["nl"] == "1", info
    assert int(info["split_from"]) == split_from(30, 32, True, True), info
    got, got_frame = buf.cpu().numpy(), frame.cpu().numpy()
    want_frame = np.full((H, W, 4), -3.0, np.float32)
    total = 0
    for lo in range(0, rows, rb):   # local rows lo.. are global rows gy..
        n, gy = min(rb, rows - lo), y0 + (lo // rb) * rb * rp + ph * rb
        want, wr = oracle.orc_render(W, H, frames, 8, frame0, x0, xc, gy, n, buf=init[lo:lo + n].copy(), threads=16)
        assert wr > 2 * frames * xc * n, wr
        _bitwise(got[lo:lo + n], want, f"shard rows {lo}..")
        want_frame[gy:gy + n, x0:x0 + xc] = want
        total += wr
    assert int(rays.item()) == total
    assert np.array_equal(got[..., 3].view(np.uint32), init[..., 3].view(np.uint32))
    assert np.array_equal(got_frame.view(np.uint32), want_frame.view(np.uint32)), \
        f"{int((got_frame != want_frame).any(axis=-1).sum())} frame pixels differ"


# ---- f. v0 and wavefront on the same inputs ----------------------------------------------------
def _v0_lanes(frames):
    """launch_split's frame lanes per pixel and launch_depth's sample mode for these windows (an
    LDS linear-scan scene, few tiles): several rounds per task run as one task per round."""
    split = 1
    while split * 2 <= frames and split * 2 <= 16:
        split *= 2
    return str(split), "1" if split >= 4 and -(-frames // split) >= 2 else "0"


@pytest.mark.parametrize("frames,split", [(7, "4"), (8, "8"), (12, "8"), (15, "8"), (16, "16")])
def test_v0_eight_frame_lanes_vs_oracle(gpu, frames, split):
    """8..15 frames take eight frame lanes per pixel (launch_split), an instance no other frame
    count in the suite selects; 7 and 16 are its neighbours."""
    info = _check(gpu, V0, frames, 8, window(32), what="v0 lanes")
    assert info["kernel"] == "trace_kernel" and info["split"] == split, info
    assert (info["split"], info["samp"]) == _v0_lanes(frames), info


@pytest.mark.parametrize("frames", [65, 1025, 4097])
def test_v0_same_windows_vs_oracle(gpu, frames):
    """The bands' and the rounds' windows through trace_kernel: 16 lanes, many lerp rounds."""
    info = _check(gpu, V0, frames, 8, window(pool_pix(frames)), what="v0")
    assert info["kernel"] == "trace_kernel" and (info["split"], info["samp"]) == _v0_lanes(frames) == ("16", "1"), info


@pytest.mark.parametrize("frames", [65, 1025])
def test_wavefront_same_windows_vs_oracle(gpu, frames):
    info = _check(gpu, WAVEFRONT, frames, 8, window(pool_pix(frames)), what="wavefront")
    assert info["kernel"] == "wf_extend", info


def test_policy_sends_small_windows_to_v0(gpu):
    """Without flags a window of 30 tiles is v0's: the pool needs a tile per resident wave."""
    info = _check(gpu, 0, 65, 8, window(32), what="policy")
    assert info["kernel"] == "trace_kernel" and info["split"] == "16", info
