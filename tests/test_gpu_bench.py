"""bench.py as every change's benchmark run starts it: a plain one-GPU run (no --full) times
only the headline figure, and --dump-outputs writes the frame and ray count of its last timed
step -- the same bits as a plain render of that frame, and the same from run to run."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu


def test_plain_bench_run_is_lean_and_dumps_its_last_frame(gpu, tmp_path):
    w, h, spp, depth = 1280, 720, 1, 8   # config 2's frame at 1 spp
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
           "--spp", str(spp), "--dump-outputs", str(tmp_path / "out")]
    out = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=110)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [json.loads(l) for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout
    d = lines[0]
    assert d["steps"] == 3 and d["n_gpus"] == 1 and d["full"] is False
    assert d["value"] > 0 and d["ms_per_step"] > 0 and d["unit"] == "Mray/s" and d["dtype"] == "f32"
    assert d["higher_is_better"] is True and d["metric"].startswith("Mray/s")
    # value is rays per step over ms_per_step (both rounded in the line)
    assert d["value"] == pytest.approx(d["config"]["rays_per_step"] / d["ms_per_step"] / 1e3, rel=1e-3)
    # none of --full's legs ran
    for k in ("cpu_baseline", "cpu_baseline_1core", "cpu_reference_drawtest", "drawtest", "drawtest_multi",
              "end_to_end", "ms_per_launch_alone", "ms_per_call_alone", "exchange"):
        assert d[k] is None, k
    assert "cpu baseline" not in out.stderr
    assert 2 <= d["clock_hold_steps"] <= 126
    assert d["dumped_outputs"] == {"frame_rgb": [h, w, 3], "rays_per_step": [1]}
    frame = np.load(tmp_path / "out" / "frame_rgb.npy")
    rays = np.load(tmp_path / "out" / "rays_per_step.npy")
    assert frame.dtype == np.float32 and rays.dtype == np.float64
    want = np.zeros((h, w, 4), np.float32)
    want_rays = gpu.render_host(gpu.Job(width=w, height=h, frames=spp, max_depth=depth), want)
    assert np.array_equal(frame.view(np.uint32), want[..., :3].view(np.uint32))
    assert rays.tolist() == [float(want_rays)] and d["config"]["rays_per_step"] == want_rays
