"""bench.py as the driver runs it (GPU): one JSON line on stdout and nothing else, the contract's keys, the self-check of the
timed output, and the multi-rank form -- `python -m torch.distributed.run ... bench.py --gpus 2` -- rehearsed with two gloo
ranks sharing the one GPU a lease has (RCCL refuses two ranks on one device; the rank logic, the barriers, the max over ranks,
the histogram exchange and the sequence leg are the same code)."""
import json
import os
import socket
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = ["--steps", "3", "--warmup", "1", "--repeats", "3", "--batch", "4", "--width", "320", "--height", "96", "--disparities", "64", "--no-pcie"]


def one_json_line(stdout):
    lines = [l for l in stdout.decode().splitlines() if l.strip()]
    assert len(lines) == 1, f"stdout must hold exactly one line, got {len(lines)}:\n" + "\n".join(l[:200] for l in lines[:8])
    return json.loads(lines[0])


def test_single_gpu_line_is_verified_and_complete():
    pr = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--full"] + SMALL, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=540)
    assert pr.returncode == 0, pr.stderr.decode(errors="replace")[-3000:]
    d = one_json_line(pr.stdout)
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data",
              "config", "roofline", "cpu_baseline", "spread", "repeats", "prewarm_steps", "verified", "placement_tuning"):
        assert k in d, k
    assert d["verified"] is True and d["verification"]["mismatches"] == []
    assert d["n_gpus"] == 1 and d["steps"] == 3 and d["repeats"] == 3 and d["value"] > 0
    assert d["spread"]["min"] <= d["value"] <= d["spread"]["max"]
    assert abs(d["value"] - 4 * 3 / (d["ms_per_step"] * 3e-3)) / d["value"] < 1e-3      # value = pairs of the median block / its time
    r = d["roofline"]
    assert r["bound"] == "hbm" and r["peak"] == 8000.0 and abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-3
    assert "frac_of_copy_ceiling" not in r and "copy_ceiling_GBps" not in r   # renamed in round 4: the copy is a reference rate, not a ceiling
    assert r["ratio_to_copy_rate"] is None or 0 < r["ratio_to_copy_rate"] <= 1.3
    assert d["cpu_baseline"]["kind"] == "port" and d["cpu_baseline"]["cores"] >= 1
    assert d["config"]["distinct_frames_per_batch"] == 4
    assert d["bgr_input"]["disparity_equals_gray_run"] is True and d["value_bgr_input"] > 0   # the 8UC3 input disparity.cu:66-67 is handed
    assert d["value_without_stage_events"] > 0   # informational block after the timed ones, the engine's stage events off
    pt = d["placement_tuning"]
    # (the kept set is re-timed after every candidate: its last timing may lie a per cent above the first one)
    assert 0 < pt["launch_pair_ms_kept"] <= 1.05 * pt["launch_pair_ms_first"] and pt["launch_pair_ms_kept"] <= pt["launch_pair_ms_slowest_seen"]
    assert 1 <= pt["candidates_timed"] <= pt["units"] * pt["tries_allowed"] and pt["tries_allowed"] <= 8   # the default search is short
    assert pt["mode"] in ("fast", "mixed", "uniform") and pt["stopped_on"] in ("fast set found", "uniform", "tries", "time", "memory")
    # the line says which mode the run ended in (unit 0's verdict; the line's times are means over the units: compare loosely)
    assert pt["mode"] != "fast" or pt["launch_pair_ms_kept"] < 0.97 * pt["launch_pair_ms_slowest_seen"]
    assert pt["value_untuned"] > 0 and pt["seconds"] < 12


def test_plain_run_times_its_steps_and_dumps_the_same_outputs(tmp_path):
    """Without --full: one timed block of exactly --steps steps and none of the --full legs; --dump-outputs writes what the last timed
    step handed its caller, the same in two fresh processes, and its disparity is the oracle's."""
    import numpy as np
    import oracle_lib as O
    from cartslam import synth
    dumps = []
    for i in range(2):
        out = tmp_path / str(i)
        pr = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "3", "--warmup", "1", "--batch", "4", "--width", "320", "--height", "96",
                             "--disparities", "64", "--dump-outputs", str(out)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
        assert pr.returncode == 0, pr.stderr.decode(errors="replace")[-3000:]
        d = one_json_line(pr.stdout)
        assert d["steps"] == 3 and d["repeats"] == 1 and d["value"] > 0 and d["unit"] == "stereo-pairs/sec" and d["dtype"] == "u8"
        assert abs(d["value"] - 4 * 3 / (d["ms_per_step"] * 3e-3)) / d["value"] < 1e-3
        for k in ("cpu_baseline", "verification", "bgr_input", "pcie_inclusive", "value_without_stage_events"):
            assert k not in d, k
        assert d["verified"] is None and "value_untuned" not in d["placement_tuning"] and d["roofline"]["copy_rate_GBps"] is None
        dumps.append({f.name: np.load(f) for f in out.iterdir()})
    assert set(dumps[0]) == {n + ".npy" for n in ("disparity", "planes", "params", "ids", "components", "n_components")}
    for name, a in dumps[0].items():
        assert a.dtype in (np.float32, np.float64) and np.array_equal(a, dumps[1][name]), name
    disp = dumps[0]["disparity.npy"]
    assert disp.shape == (4, 96, 320)
    for k in (0, 3):
        l, r, _ = synth.make_pair(320, 96, 64, 4, frame=k)
        assert (disp[k] == O.disparity_module(l, r, 64, 8, 4, radius=2, iterations=1)).all(), f"frame {k}"


def test_two_ranks_through_the_drivers_launch_form():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1", "--master-port", str(port),
           os.path.join(ROOT, "bench.py"), "--gpus", "2", "--backend", "gloo", "--allow-shared-gpu", "--sequence", "--full"] + SMALL
    pr = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=540)
    assert pr.returncode == 0, pr.stderr.decode(errors="replace")[-3000:]
    d = one_json_line(pr.stdout)
    assert d["n_gpus"] == 2 and d["config"]["global_pairs_per_step"] == 8 and d["config"]["world_size"] == 2
    assert d["scaling"] == "weak" and d["verified"] is True and "cpu_baseline" not in d   # rank 0's outputs are checked, the CPU baseline is an N = 1 figure
    assert d["sequence_mode"]["frames"] == 8 and d["sequence_mode"]["pairs_per_s"] > 0


def test_four_ranks_and_a_64_frame_sequence():
    """The driver's SCALE command shape, as far as one leased GPU allows: a GPU box admits at most 6 of a user's processes on its card
    (gpurun's process guard), this pytest process is one of them, so FOUR real-engine ranks is the largest rehearsal that is safe
    -- each with its own engine, placement search, per-step histogram all-gather and BASELINE configs[4]'s 64-frame sequence dealt
    16 per rank, scattered and gathered through the backend, pipelined.  One verified JSON line, exit 0.  (Eight ranks run on CPU
    over gloo in tests/test_distributed.py: the schedule over 8 x 8 frames and the sequence pipeliner with 64 / 63 / 65 / 7 frames.)
    No scaling number comes out of ranks that share a GPU, and none is asserted."""
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "4", "--master-addr", "127.0.0.1", "--master-port", str(port),
           os.path.join(ROOT, "bench.py"), "--gpus", "4", "--backend", "gloo", "--allow-shared-gpu", "--sequence", "--full",
           "--steps", "3", "--warmup", "1", "--repeats", "3", "--batch", "16", "--width", "256", "--height", "96", "--disparities", "64", "--no-pcie"]
    pr = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=540)
    assert pr.returncode == 0, pr.stderr.decode(errors="replace")[-3000:]
    d = one_json_line(pr.stdout)
    assert d["n_gpus"] == 4 and d["config"]["global_pairs_per_step"] == 64 and d["config"]["world_size"] == 4
    assert d["scaling"] == "weak" and d["verified"] is True
    assert d["sequence_mode"]["frames"] == 64 and d["sequence_mode"]["pairs_per_s"] > 0


def test_self_launch_starts_its_own_ranks():
    """`python bench.py --gpus 2` without RANK in the environment: bench.py starts the two ranks itself (launch_ranks) and relays
    rank 0's line and the exit code."""
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT")}
    env["HSA_ENABLE_IPC_MODE_LEGACY"] = "0"
    pr = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--backend", "gloo", "--allow-shared-gpu", "--no-cpu-baseline"] + SMALL,
                        env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=540)
    assert pr.returncode == 0, pr.stderr.decode(errors="replace")[-3000:]
    d = one_json_line(pr.stdout)
    assert d["n_gpus"] == 2 and d["value"] > 0


def test_self_launch_refuses_more_gpus_than_the_box_has():
    import torch
    n = torch.cuda.device_count() + 1
    pr = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", str(n)] + SMALL, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert pr.returncode == 2 and b"GPUs" in pr.stderr and pr.stdout.strip() == b""
