"""Every N > 1 code path of bench.py with REAL kernels on a one-GPU box: two ranks share GPU 0
(`--same-device`), the per-step exchange goes through the host-staged gloo transport (RCCL refuses two ranks per device), the
library's pipeline joins the launch stream at the end of every step, the gather of step k overlaps the kernels of step k + 1
(two output sets), config 4 runs strong + weak on an UNEVEN global batch (1023), the guarded C-ABI group leg must come back --
with a result or with the error RCCL raises for two ranks on one device -- without hanging, and frames of the OTHER rank's
shard, read from the gathered blocks, equal the oracle.  The line is marked same_device and is never a scaling figure."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def _env():
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env["OMP_NUM_THREADS"] = "1"
    env["ORBFE_BENCH_GROUP_TIMEOUT"] = "120"
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    return env


@pytest.mark.gpu
def test_two_ranks_on_one_device_run_every_multi_gpu_path():
    cmd = [sys.executable, BENCH, "--gpus", "2", "--same-device", "--full", "--steps", "3", "--warmup", "1", "--frames", "128", "--launches", "4",
           "--seeds", "128", "--config4-batch", "1023"]
    r = subprocess.run(cmd, env=_env(), capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    j = json.loads(lines[0])
    assert j["n_gpus"] == 2 and j["same_device"] is True and "SAME-DEVICE TEST MODE" in j["config"]["workload"]
    assert j["exact_checked"] is True                       # rank 0's own frames of the timed region, incl. cross-sub-batch matches
    assert j["gathered_exact_checked"] is True              # rank 1's frames as they arrived through the overlapped gather
    assert {c["rank"] for c in j["gathered_exact_checked_frames"]} == {1}
    assert "joins the launch stream" in j["config"]["streams"]
    c4 = j["config4"]
    assert c4["global_batch"] == 1023 and c4["n_gpus"] == 2
    assert c4["strong"]["frames_per_gpu"] == 512 and c4["strong"]["gathered_frames"] == 2 * 512   # 512 + 511, padded to 2 x 512
    assert c4["weak"]["gathered_frames"] == 2 * 1023
    assert c4["gathered_exact_checked"] is True
    cg = c4["cabi_group"]
    # the library's own communicator: two ranks on one device is what RCCL refuses -- the leg reports that, the line survives
    assert ("frames_per_s" in cg) or ("error" in cg and cg["error"]), cg
    assert j["config4_cabi_group_status"]
    assert j["value"] > 0 and j["scaling"] == "weak"
    # the exchange step in numbers (what the first 8-GPU run needs to be explainable): time, bytes, bus bandwidth, what of it
    # the kernels hid, and the same steps without it
    ex = j["exchange"]
    for k in ("gather_ms", "gather_bytes_per_rank", "gather_bus_GBps", "gather_hidden_frac", "ms_per_step_no_gather", "value_no_gather"):
        assert ex[k] is not None and j[k] == ex[k], k
    cap, gcap = ex["gather_slots_full"], ex["gather_slots_per_frame"]
    B = 128 * 4
    assert gcap % 64 == 0 and 1004 <= gcap <= cap and ex["gather_truncated_frames"] == 0     # the valid prefix travels
    assert ex["gather_bytes_per_rank"] == B * 4 + B * gcap * (28 + 32)
    assert ex["gather_ms"] > 0 and 0.0 <= ex["gather_hidden_frac"] <= 1.0 and ex["ms_per_step_no_gather"] > 0


@pytest.mark.gpu
def test_two_ranks_on_one_device_without_the_gather_and_with_the_full_blocks():
    base = [sys.executable, BENCH, "--gpus", "2", "--same-device", "--steps", "2", "--warmup", "1", "--frames", "64", "--launches", "2",
            "--seeds", "64", "--no-extras"]
    for extra in (["--no-gather"], ["--gather-full", "--rccl-channels", "4"]):
        r = subprocess.run(base + extra, env=_env(), capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
        j = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][0])
        assert j["n_gpus"] == 2 and j["value"] > 0
        if extra[0] == "--no-gather":
            assert "disabled" in j["exchange"]["gather"] and "gather_ms" not in j
        else:
            ex = j["exchange"]
            assert ex["gather_slots_per_frame"] == ex["gather_slots_full"] and ex["rccl_max_nchannels"] == "4" and ex["gather_ms"] > 0
