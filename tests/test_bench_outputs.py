"""bench.py's plain run and --dump-outputs: a plain run times the headline alone, --steps sets the timed steps, and the dumped sample of
the spectrum is the timed path's result (against the oracle) and the same from run to run with the same arguments."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")
SMALL = ["--gpus", "1", "--steps", "3", "--warmup", "1", "--streams", "2", "--precondition", "0"]


def _env():
    return {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}


def test_steps_below_one_are_refused():
    r = subprocess.run([sys.executable, BENCH, "--steps", "0"], env=_env(), capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and r.stdout.strip() == "" and "--steps" in r.stderr


@pytest.mark.parametrize("B", [2, 100])
def test_dump_outputs_samples_fixed_rows_within_the_size_limit(tmp_path, B):
    """no GPU: a fake download fills each row with its (stream, frame) row index, so the file says which rows were taken"""
    sys.path.insert(0, ROOT)
    import bench
    from nx_signal_amd import _lib

    base = 4096

    class FakeLib:
        def nxsig_download(self, handle, dst, src, n):
            assert n == bench.N_FFT * 8 and 0 <= src.value - base < B * bench.M * bench.N_FFT * 8
            np.ctypeslib.as_array(C.cast(dst, C.POINTER(C.c_float)), (n // 4,))[:] = (src.value - base) // n
            return 0

    class FakeBuf:
        ptr = base

    class FakeCtx:
        handle = None

    dumps = []
    for run in ("a", "b"):
        info = bench.dump_outputs(str(tmp_path / run), FakeCtx(), FakeLib(), _lib, C, FakeBuf(), B)
        z = np.load(tmp_path / run / "stft.npy")
        assert z.dtype == np.float32 and z.nbytes <= 64 * 2**20 and list(z.shape) == info["files"]["stft.npy"]
        assert z.shape[0] == B and z.shape[2:] == (bench.N_FFT, 2) and z.shape[1] == (64 if B <= 64 else 4096 // B)
        rows = z[:, :, 0, 0].astype(np.int64)
        assert np.all(z == z[:, :, :1, :1])
        for b in range(B):
            m = rows[b] - b * bench.M
            assert m[0] == 0 and m[-1] == bench.M - 1 and np.all(np.diff(m) > 0)
        dumps.append(z)
    assert np.array_equal(dumps[0], dumps[1])


def _line(args):
    r = subprocess.run([sys.executable, BENCH] + args, env=_env(), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_times_the_headline_and_dumps_what_it_computed(tmp_path):
    sys.path.insert(0, ROOT)
    import bench
    from oracle import nx_oracle as O

    d = _line(SMALL + ["--dump-outputs", str(tmp_path / "a")])
    assert d["steps"] == 3 and d["warmup"] == 1 and d["ms_per_step"] > 0 and d["value"] > 0 and d["full"] is False
    assert d["unit"] == "frames/s" and d["higher_is_better"] is True and d["dtype"] == "f32"
    for k in ("single_stream", "host_path", "verify", "yardsticks"):
        assert d[k] is None, k
    assert "roofline_istft" not in d and "cpu_baseline" not in d
    z = np.load(tmp_path / "a" / "stft.npy")
    assert z.dtype == np.float32 and z.shape == (2, 64, bench.N_FFT, 2)
    zc = z[..., 0] + 1j * z[..., 1]
    w = O.hann(bench.N_FFT)
    for b in range(2):
        x = bench.synth(1234 + b)
        for i, m in ((0, 0), (63, bench.M - 1)):   # every stream's first and last frame
            zo, _, _ = O.stft(x[m * bench.HOP: m * bench.HOP + bench.N_FFT], w, overlap_length=bench.N_FFT - bench.HOP,
                              fft_length=bench.N_FFT, sampling_rate=bench.SR)
            assert np.max(np.abs(zc[b, i] - zo[0])) / np.max(np.abs(zo)) < 1e-5, (b, m)
    _line(SMALL + ["--dump-outputs", str(tmp_path / "b")])
    assert np.array_equal(z, np.load(tmp_path / "b" / "stft.npy"))


@pytest.mark.gpu
def test_plain_run_takes_more_steps_than_one_lap_series_holds():
    """--steps K beyond the 4096 events of a timer_lap series: all K steps are timed, the per-step distribution covers the last 4095"""
    d = _line(["--gpus", "1", "--steps", "5000", "--warmup", "2", "--streams", "1", "--precondition", "0"])
    assert d["steps"] == 5000 and d["ms_per_step"] > 0 and d["value"] > 0
    r = d["roofline"]
    assert r["kernel_us"]["n"] == 4095 and 0 < r["kernel_ms"] <= d["ms_per_step"] * 1.01
