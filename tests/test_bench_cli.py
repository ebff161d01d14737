"""`python bench.py --gpus N` as the driver types it: without a launcher around it the script starts its own N rank
processes (bench.self_launch), relays rank 0's single JSON line and exits with the ranks' verdict."""
import json
import os
import subprocess
import sys

import pytest

from tests.conftest import ROOT

BENCH = os.path.join(ROOT, "bench.py")


def _run(args, env_extra, timeout):
    env = dict(os.environ, **env_extra)
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)                                   # exactly the bare command: no launcher's environment
    p = subprocess.run([sys.executable, BENCH] + args, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       timeout=timeout, text=True)
    lines = [ln for ln in p.stdout.splitlines() if ln.strip()]
    return p.returncode, lines, p.stderr


def test_self_launch_reports_failing_ranks_and_leaves_nothing_behind():
    """No GPU in this container: every rank fails when it selects its device.  The launcher must come back non-zero,
    print no line, and not hang on the ranks that are still alive."""
    import torch

    if torch.cuda.is_available():
        pytest.skip("needs a box without a GPU (the GPU flavour of this test is below)")
    rc, lines, err = _run(["--gpus", "2", "--steps", "2", "--warmup", "1", "--no-cpu-baseline"],
                          {"LOM_BENCH_LAUNCH_TIMEOUT_S": "200"}, timeout=400)
    assert rc != 0
    assert lines == []
    assert "failed; ending the others" in err or "still running" in err


def test_event_sampling_of_short_and_long_blocks():
    """bench.event_period: a step that carries HIP events takes ~40 % longer, so a short block (the driver's 20 steps) carries
    them on its first step only and a long one on every 32nd."""
    sys.path.insert(0, ROOT)
    import bench

    assert bench.event_period(20) == 20 and bench.event_period(5) == 5 and bench.event_period(1) == 1
    assert bench.event_period(95) == 95 and bench.event_period(96) == 32 and bench.event_period(200) == 32
    assert bench.event_period(0) == 1


def test_dump_outputs_writes_the_pose_as_f32_arrays(tmp_path):
    """--dump-outputs DIR: the pose the last timed step returned, one float32 .npy per array (no GPU needed for the
    writer); the option and --full are accepted by the command line before anything touches a GPU."""
    sys.path.insert(0, ROOT)
    import numpy as np

    import bench
    from lidar_odometry_demo_amd import Pose3D

    bench.dump_outputs(str(tmp_path / "out"), Pose3D((1.5, -2.0, 0.25), (0.5, 0.5, -0.5, 0.5)))
    t = np.load(tmp_path / "out" / "pose_translation.npy")
    q = np.load(tmp_path / "out" / "pose_rotation_wxyz.npy")
    assert t.dtype == np.float32 and q.dtype == np.float32
    assert t.tolist() == [1.5, -2.0, 0.25] and q.tolist() == [0.5, 0.5, -0.5, 0.5]
    p = subprocess.run([sys.executable, BENCH, "--help"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                       timeout=60)
    assert p.returncode == 0 and "--full" in p.stdout and "--dump-outputs" in p.stdout, p.stderr


@pytest.mark.gpu
def test_plain_line_dumps_the_same_outputs_every_run_and_full_adds_the_side_figures(tmp_path):
    """A plain run is the timed steps only: --steps sets them, the line carries ms_per_step and none of the --full
    figures; two runs with the same arguments dump bit-equal poses, the ones the line reports.  --full (without the CPU
    baseline and the extras, to stay short) adds the roofline, the kernels and the spread."""
    outs = []
    for k in range(2):
        d = tmp_path / f"dump{k}"
        rc, lines, err = _run(["--gpus", "1", "--steps", "7", "--warmup", "2", "--dump-outputs", str(d)], {}, timeout=600)
        assert rc == 0, err[-3000:]
        assert len(lines) == 1, lines
        line = json.loads(lines[0])
        assert line["steps"] == 7 and line["ms_per_step"] > 0 and line["value"] > 0
        assert line["metric"] == "icp_correspondences_per_sec" and line["higher_is_better"] is True
        assert abs(line["frames_per_s"] * line["ms_per_step"] - 1e3) < 1e-6 * 1e3
        for key in ("roofline", "roofline_kernels", "ms_per_step_blocks", "cpu_baseline", "extra_configs",
                    "concurrent_contexts"):
            assert key not in line, key
        import numpy as np

        t, q = np.load(d / "pose_translation.npy"), np.load(d / "pose_rotation_wxyz.npy")
        assert t.dtype == np.float32 and q.dtype == np.float32 and t.shape == (3,) and q.shape == (4,)
        assert t.tolist() == line["pose"]["t"] and q.tolist() == line["pose"]["q_wxyz"]
        outs.append((t.tobytes(), q.tobytes()))
    assert outs[0] == outs[1]
    rc, lines, err = _run(["--gpus", "1", "--steps", "5", "--warmup", "1", "--full", "--no-cpu-baseline", "--no-extras"],
                          {}, timeout=600)
    assert rc == 0, err[-3000:]
    line = json.loads(lines[-1])
    assert line["steps"] == 5 and line["roofline"]["avg_launch_us"] > 0 and len(line["roofline_kernels"]) == 3
    assert len(line["ms_per_step_blocks"]["blocks"]) == 6 and line["config"]["pcie_inclusive_ms_per_step"] > 0


@pytest.mark.gpu
def test_plain_command_with_two_ranks_prints_one_line():
    """`python bench.py --gpus 2 --steps 5 --full`, nothing else: two fresh rank processes (here both on the one GPU of
    the box, LOM_BENCH_ONE_DEVICE=1: a rehearsal of the flow, the number means nothing), one JSON line, both ranks seen
    through the exchange object the transport itself uses, the other transport timed beside it (--full)."""
    rc, lines, err = _run(["--gpus", "2", "--steps", "5", "--warmup", "2", "--full"], {"LOM_BENCH_ONE_DEVICE": "1"},
                          timeout=900)
    assert rc == 0, err[-3000:]
    assert len(lines) == 1, lines
    line = json.loads(lines[0])
    assert line["n_gpus"] == 2 and line["steps"] == 5 and line["metric"] == "icp_correspondences_per_sec"
    cfg = line["config"]
    assert cfg["ranks_seen"]["ranks"] == [0, 1], cfg["ranks_seen"]
    assert cfg["exchange"] in ("p2p", "host")
    assert cfg["exchange_selftest"]["result"] in ("passed", "failed")
    assert line["value"] > 0 and line["ms_per_step"] > 0
    others = cfg["other_exchange"]
    assert isinstance(others, list) and others, others
    assert any(o.get("exchange") == "host" and o.get("value", 0) > 0 for o in others) or cfg["exchange"] == "host", others
    assert any(o.get("exchange") == "rccl" for o in others)                 # skipped here, with the reason given


@pytest.mark.gpu
def test_one_rank_line_is_the_same_with_and_without_the_launcher_path():
    """--gpus 1 never self-launches; its value must not depend on the N > 1 plumbing being present: two short runs
    agree within 10 % (the second with LOM_BENCH_FORCE_DIST=1, the multi-rank code path with one rank)."""
    a = _run(["--gpus", "1", "--steps", "20", "--warmup", "3", "--no-cpu-baseline", "--no-extras"], {}, timeout=600)
    b = _run(["--gpus", "1", "--steps", "20", "--warmup", "3", "--no-cpu-baseline", "--no-extras"],
             {"LOM_BENCH_FORCE_DIST": "1", "LOM_BENCH_NO_COMPARE": "1"}, timeout=600)
    assert a[0] == 0 and b[0] == 0, (a[2][-2000:], b[2][-2000:])
    la, lb = json.loads(a[1][-1]), json.loads(b[1][-1])
    assert la["n_gpus"] == lb["n_gpus"] == 1
    assert abs(la["value"] - lb["value"]) / la["value"] < 0.10, (la["value"], lb["value"])
