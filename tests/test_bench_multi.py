"""bench.py at N > 1: `--gpus N` can never silently become a 1-GPU line, and under a launcher or on its own
it measures BASELINE configs 3 / 4 / 5 on every rank plus the config-4-sized assembly.  The GPU cases run N RANKED processes with
real RCCL on ONE device (--share-gpu: one NCCL_HOSTID per rank, socket transport) at reduced sizes."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = ["--full", "--steps", "3", "--warmup", "1", "--streams", "2", "--cpu-seconds", "0", "--precondition", "0", "--no-verify",
         "--secondary-seconds", "20", "--secondary-channels", "2", "--istft-seconds", "10"]


def test_gpus_n_without_devices_fails_loudly():
    """no GPU here: `python bench.py --gpus 2` must exit non-zero with a message and print NO JSON line (never n_gpus: 1)"""
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    env["HIP_VISIBLE_DEVICES"] = "-1"  # also on a GPU box: no device visible
    env["ROCR_VISIBLE_DEVICES"] = "-1"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2"] + SMALL, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode != 0
    assert r.stdout.strip() == ""
    assert "GPU" in r.stderr


def test_self_spawn_sets_a_launcher_environment(monkeypatch):
    """the self-spawn path hands every child RANK / LOCAL_RANK / WORLD_SIZE / MASTER_ADDR / MASTER_PORT (checked without a GPU by
    intercepting Popen and the device count)"""
    sys.path.insert(0, ROOT)
    import argparse
    import ctypes as C

    import bench
    from nx_signal_amd import _lib

    class FakeLib:
        def nxsig_device_count(self, p):
            C.cast(p, C.POINTER(C.c_int))[0] = 4
            return 0

    seen = []

    class FakeProc:
        def __init__(self, cmd, env=None, stdout=None):
            seen.append((cmd, env, stdout))

        def wait(self):
            return 0

    monkeypatch.setattr(_lib, "load", lambda: FakeLib())
    monkeypatch.setattr(subprocess, "Popen", FakeProc)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "4", "--steps", "2"])
    rc = bench.self_spawn(argparse.Namespace(gpus=4, share_gpu=False))
    assert rc == 0 and len(seen) == 4
    ports = {e["MASTER_PORT"] for _, e, _ in seen}
    assert len(ports) == 1
    for r, (cmd, env, out) in enumerate(seen):
        assert env["RANK"] == str(r) and env["LOCAL_RANK"] == str(r) and env["WORLD_SIZE"] == "4" and env["MASTER_ADDR"] == "127.0.0.1"
        assert cmd[-4:] == ["--gpus", "4", "--steps", "2"]
        assert (out is None) == (r == 0)  # only rank 0 owns stdout: ONE JSON line
    # fewer devices than ranks: refused
    seen.clear()
    assert bench.self_spawn(argparse.Namespace(gpus=8, share_gpu=False)) == 2 and not seen


_STUCK = ""


def _bench_line(cmd, env, timeout):
    """Runs a ranked bench.py command and returns its ONE JSON line.  N ranks on ONE device is a TEST MODE: RCCL bootstraps over
    loopback sockets and its kernels spin until the peer's kernels have run, while the ranks time-slice the device.  A run takes
    15 s; one that produces no line in 180 s, or whose communicator timed out, SKIPS with what the ranks last printed — and so does
    every later ranked test of the session, at once — instead of holding the suite for half an hour (round 6: a bug of ours, a sticky
    HIP error that made rank 0 skip a collective, did exactly that until it was found; NXSIG_BENCH_HANG_DUMP=<s> shows where ranks
    sit).  An error the library itself reports (version refused, missing symbol, wrong call, wrong result) FAILS.  One retry for a
    quick RCCL error."""
    global _STUCK
    if _STUCK:
        pytest.skip("ranked processes sharing one GPU got stuck earlier in this session: " + _STUCK)
    for attempt in (0, 1):
        try:
            r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=min(timeout, 180))
        except subprocess.TimeoutExpired as e:
            _STUCK = "no result after 180 s; stderr tail: " + (e.stderr or b"")[-300:].decode("utf-8", "replace").replace("\n", " | ")
            pytest.skip(_STUCK)
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
        rccl_down = (r.returncode == 3 and lines and '"preflight_failed": "RCCL"' in lines[-1]) or (
            r.returncode == 0 and len(lines) == 1 and not json.loads(lines[0])["comm"]["backend"].startswith("RCCL"))
        why = " | ".join(ln for ln in r.stderr.splitlines() if "RCCL group creation failed" in ln)
        if rccl_down and ("did not finish in time" in why or "timed out" in why.lower() or "unhandled system error" in why.lower()):
            _STUCK = "the RCCL communicator did not come up: " + why[-300:]
            pytest.skip(_STUCK)
        if rccl_down and attempt == 0:
            continue
        assert r.returncode == 0, r.stderr[-3000:]
        assert len(lines) == 1, r.stdout[-2000:]
        assert json.loads(lines[0])["comm"]["backend"].startswith("RCCL"), r.stderr[-3000:]
        return lines[0]


def _check_line(line, n):
    d = json.loads(line)
    assert d["n_gpus"] == n and d["scaling"] == "weak"
    assert d["comm"]["backend"].startswith("RCCL")
    for k, unit in (("config3", "frames_per_s_total"), ("config4", "frames_per_s_total"), ("config5", "samples_per_s_total")):
        assert d[k]["ranks"] == n and d[k][unit] > 0 and 0 < d[k]["per_gpu_frac"] < 1, d[k]
        assert d[k]["kernel_ms_max_over_ranks"] >= d[k]["kernel_ms_rank0"] * 0.999
    a = d["assembly_config4"]
    assert a["world"] == n and a["own_shard_intact"] and a["peer_shard_arrived"] and a["recv_GBps_per_rank"] > 0
    assert d["assembly"]["own_shard_intact"]
    assert d["value"] > 0 and d["value_cold"] > 0
    return d


@pytest.mark.gpu
@pytest.mark.parametrize("n", [2])
def test_gpus_n_self_spawns_and_measures_configs_4_and_5(n):
    """plain `python bench.py --gpus 2 --share-gpu` (no launcher): n_gpus == 2, RCCL, config 3 / 4 / 5 blocks, both assemblies"""
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    env.update(NCCL_SOCKET_IFNAME="lo", NCCL_IB_DISABLE="1")
    _check_line(_bench_line([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", str(n), "--share-gpu"] + SMALL, env, 900), n)


@pytest.mark.gpu
def test_a_rank_that_cannot_prepare_its_assembly_shard_strands_nobody():
    """round 6: rank 1 fails before the config-2 assembly (injected) — the ranks agree on a status word first, every rank skips the
    collective, the line still comes out with the measurement and says why the assembly is missing (it used to hang: the peers sat
    in an all-gather the failed rank never joined)"""
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    env.update(NCCL_SOCKET_IFNAME="lo", NCCL_IB_DISABLE="1", NXSIG_BENCH_FAIL_ASSEMBLY_RANK="1")
    d = json.loads(_bench_line([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--share-gpu"] + SMALL, env, 900))
    assert d["n_gpus"] == 2 and d["value"] > 0
    assert "error" in d["assembly"] and "another rank" in d["assembly"]["error"]          # rank 0 prints the line: its own part was fine
    assert d["assembly_config4"]["own_shard_intact"] and d["config4"]["ranks"] == 2      # everything after it ran on both ranks


@pytest.mark.gpu
def test_dry_preflight_allocates_and_launches_everything_once():
    """`bench.py --gpus 2 --dry`: the whole N-GPU run in one pass — same buffers, the RANKED group, one launch of
    every block, both assemblies — and a line that says so: dry: true, per-rank memory high-water marks, the RCCL actually loaded"""
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    env.update(NCCL_SOCKET_IFNAME="lo", NCCL_IB_DISABLE="1")
    small = [a for a in SMALL if a not in ("--no-verify",)]
    d = json.loads(_bench_line([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--share-gpu", "--dry"] + small, env, 900))
    assert d["dry"] is True and d["n_gpus"] == 2 and d["steps"] == 1
    pf = d["preflight"]
    assert len(pf["high_water_GiB_per_rank"]) == 2 and all(v > 0 for v in pf["high_water_GiB_per_rank"])
    assert pf["memory_rank0"]["high_water_GiB"] > 0 and "config 4 buffers" in pf["memory_rank0"]["after_GiB_in_use"]
    assert pf["rccl"]["loaded"] and pf["rccl"]["version_code"] > 20000 and "rccl" in pf["rccl"]["path"]
    assert d["comm"]["rccl"]["version"] == pf["rccl"]["version"]
    for k in ("roofline_istft", "roofline_stft2048", "roofline_fir"):
        assert "error" not in d[k] and d[k]["kernel_us"]["n"] == 1, d[k]
    assert d["assembly_config4"]["own_shard_intact"] and d["assembly"]["own_shard_intact"]
    assert d["verify"]["max_norm_err"] < 1e-5


@pytest.mark.gpu
def test_driver_launch_line_four_ranks_share_gpu():
    """the driver's own launch line at world 4 on one device"""
    pytest.importorskip("torch")
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    env.update(NCCL_SOCKET_IFNAME="lo", NCCL_IB_DISABLE="1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "4", "--master-addr", "127.0.0.1",
           "--master-port", "29547", os.path.join(ROOT, "bench.py"), "--gpus", "4", "--share-gpu"] + SMALL
    _check_line(_bench_line(cmd, env, 1200), 4)


def test_reduce_secondary_takes_the_slowest_rank_and_survives_a_failed_block():
    """config3 / config4 / config5 of the N > 1 line: totals = world x per-rank work / max-over-ranks time; a rank whose block failed
    (no kernel_ms) turns that config into an error entry without disturbing the others"""
    sys.path.insert(0, ROOT)
    import bench

    sec = {"roofline_istft": {"kernel_ms": 0.40, "algorithmic_bytes": 1842708480, "frames": 179952, "workload": "c3", "frac": 0.57, "kernel_us": {}},
           "roofline_stft2048": {"kernel_ms": 1.45, "algorithmic_bytes": 8293957632, "frames": 449976, "workload": "c4", "frac": 0.71, "kernel_us": {}},
           "roofline_fir": {"error": "boom"}}
    seen = []

    def allreduce(vals, op):
        seen.append((list(vals), op))
        return [max(v, w) for v, w in zip(vals, [0.50, 1.40, 1e30])]   # another rank: slower istft, faster stft, failed fir

    out = bench.reduce_secondary(sec, 8, allreduce)
    assert seen == [([0.40, 1.45, 1e30], "max")]
    assert out["config3"]["kernel_ms_max_over_ranks"] == 0.50 and out["config3"]["ranks"] == 8
    assert abs(out["config3"]["frames_per_s_total"] - 8 * 179952 / 0.50e-3) < 1.0
    assert abs(out["config3"]["per_gpu_frac"] - 1842708480 / 0.50e-3 / 1e9 / 8000.0) < 1e-9
    assert out["config4"]["kernel_ms_max_over_ranks"] == 1.45
    assert "error" in out["config5"] and out["config5"]["ranks"] == 8


def test_lap_mean_leaves_host_stalls_out_and_counts_them():
    """one 6.5 ms lap among twenty of 0.4 ms is a queue that ran dry, not a launch (profiles/r04)"""
    sys.path.insert(0, ROOT)
    import bench

    laps = [0.40] * 10 + [6.5] + [0.41] * 9
    m, stalled = bench.lap_mean(laps)
    assert stalled == 1 and abs(m - (0.40 * 10 + 0.41 * 9) / 19) < 1e-12
    m, stalled = bench.lap_mean([0.40, 0.44, 0.39, 0.52])   # ordinary spread: nothing left out
    assert stalled == 0 and abs(m - 0.4375) < 1e-12


def test_effective_cores_reads_the_cgroup_quota(tmp_path, monkeypatch):
    sys.path.insert(0, ROOT)
    import builtins

    import bench

    real_open = builtins.open

    def fake_open(path, *a, **k):
        if path == "/sys/fs/cgroup/cpu.max":
            f = tmp_path / "cpu.max"
            f.write_text("1600000 100000\n")
            return real_open(f, *a, **k)
        return real_open(path, *a, **k)

    monkeypatch.setattr(builtins, "open", fake_open)
    e = bench.effective_cores()
    assert e["cgroup_quota"] == 16.0 and e["effective"] == min(16.0, float(e["affinity"])) and "cpu.max" in e["source"]
