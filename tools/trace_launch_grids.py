"""Do the geometry switches reach the launchers, and does tests/launch_geometry.py restate their arithmetic?

Two steps, the first on a GPU under a kernel trace, the second anywhere:

    rocprofv3 --kernel-trace -d OUT -o probe --output-format csv -- python tools/trace_launch_grids.py run > OUT/plan.log
    python tools/trace_launch_grids.py report OUT/plan.log OUT/probe_kernel_trace.csv > profiles/launch_geometry/kernel_trace_grids.txt

`run` makes one call per (case, geometry) of a sample of the catalogue — every chunked launcher form, the three FIR stream kernels,
the inverse launcher forms, the many-rows shapes of NXSIG_ISTFT_RUNS_PER_CU — and prints what forward_launch / fir_launch /
inverse_launch predict for it (PLAN lines).  `report` puts the grid of the streaming kernel of each call, in dispatch order, beside
the prediction and exits non-zero when a workgroup count differs.  The record is a spot check made when the arithmetic was restated;
it is not part of the test suite (the suite has no profiler), so run it again when a launcher's geometry code changes."""
import csv
import os
import re
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path[:0] = [os.path.join(ROOT, "tests"), ROOT]

FORWARD_KEYS = ("pair-hop256", "rab960", "rab3840", "r20", "blue443", "8k", "c64-rab512", "rows1024", "rows4096", "mel-pair", "mag-real2x",
                "mel-rab960", "quad2", "real2x")
FIR_KEYS = ("fir33-same", "fir257-same", "fir257-full", "fir513-full")
INVERSE_KEYS = ("packed", "wave-deep-hop256", "half-hop128", "mask-real", "dbl", "4k", "r20", "rab960-hop240", "rabq1152", "quad-256")
STREAM = re.compile(r"k_(stft_rab_c64|stft_rab|stft_r20|stft_blue_wave|stft_wave_8k|fft_rows_wave_4k|fft_rows_wave|stft_mel_wave|stft_mag_wave|"
                    r"stft_wave|fir_wave32|fir_r2k|fir_wave|istft_packed|istft_wave_quad|istft_wave_half_deep|istft_wave_half|istft_wave_mask|"
                    r"istft_wave_dbl|istft_wave_4k|istft_wave|istft_rab_q|istft_rab|istft_r20)\b")


def run():
    import numpy as np

    import launch_geometry as G
    import test_gpu_launch_geometry as T

    import nx_signal_amd as S

    def ctx_of(knobs):
        c = S.Context(0)
        c.clear_tuning()
        for k, v in knobs.items():
            c.set_tuning(k, v)
        return c

    def plan(key, name, family, launches, workgroups, threads):
        print("PLAN", key, name, family, launches, workgroups, threads)

    for key in FORWARD_KEYS:
        case = G.FORWARD[key]
        x = T.forward_input(case, False)
        geos = G.forward_geometries(case)
        for name in ["base", "upw1", "upw3", f"upw{G.UPW_MAX}"] + [g for g in ("small-w0", "chunk5", "chunk18-w0") if g in geos]:
            knobs = {**dict(case.base), **({} if name == "base" else geos[name])}
            c = ctx_of(knobs)
            T.run_forward(c, case, x)
            c.sync()
            la = G.forward_launch(case, knobs)
            edge = case.kind == "quad"                # the ragged last unit of a quad row: an edge launch behind the stream launch
            plan(key, name, la.name, 2 if edge else 1, la.workgroups, la.W * 64)
    for key in FIR_KEYS:
        case = G.FIR[key]
        h = T.fir_taps(case)
        x = np.random.default_rng(1).standard_normal((case.rows, case.L)).astype(np.float32)
        for name in ("base", "upw3", f"upw{G.UPW_MAX}"):
            knobs = {} if name == "base" else G.fir_geometries(case)[name]
            c = ctx_of(knobs)
            S.filters.fir(x, h, mode=case.mode, ctx=c)
            c.sync()
            la, _ = G.fir_launch(case, knobs)
            plan(key, name, la.name, 2, la.workgroups, la.W * 64)      # stream launch + edge launch
    for key in INVERSE_KEYS:
        case = G.INVERSE[key]
        shapes = [(G.ROWS, n, {} if n == "base" else G.inverse_geometries(case, G.INVERSE_M)[n]) for n in ("base", "run1", "run5", "run17")]
        if key in G.MANY_ROWS_KEYS:
            shapes += [(G.many_rows(case), n, k) for n, k in G.MANY_ROWS_GEOMETRIES.items()]
        for rows, name, geo in shapes:
            z, extra = T.inverse_input(case, G.INVERSE_M, False, rows)
            knobs = {**dict(case.base), **geo}
            c = ctx_of(knobs)
            T.run_inverse(c, case, z, extra)
            c.sync()
            r = G.inverse_launch(case, G.INVERSE_M, knobs, rows=rows)
            plan(key, f"rows{rows}-{name}", case.lead, 1, r.runs_per_row * rows, f"runs-of-{r.run_len}")


def report(plan_log, trace_csv):
    with open(trace_csv) as f:
        rows = sorted(csv.DictReader(f), key=lambda r: int(r["Dispatch_Id"]))
    traced = []
    for r in rows:
        m = STREAM.search(r["Kernel_Name"])
        if m:
            traced.append((m.group(0), int(r["Grid_Size_X"]) // int(r["Workgroup_Size_X"]), int(r["Workgroup_Size_X"])))
    it = iter(traced)
    bad = 0
    print("# Grids of the streaming launches under the geometry switches: predicted by tests/launch_geometry.py, and traced on the GPU")
    print("# (tools/trace_launch_grids.py; a spot check of the restated arithmetic, regenerate it when a launcher's geometry code changes).")
    print("# Forward / FIR: workgroups x threads.  Inverses: the prediction is the number of runs over all rows and their length in units;")
    print("# the kernel takes one run per wave, so it must show ceil(runs / waves per workgroup) workgroups.")
    print(f"# {'case':<17} {'geometry':<14} {'family':<16} {'predicted':<24} traced")
    with open(plan_log) as f:
        for line in f:
            if not line.startswith("PLAN "):
                continue
            _, key, name, family, launches, count, what = line.split()
            kernel, wgs, threads = next(it)
            for _ in range(int(launches) - 1):
                next(it)
            if what.startswith("runs-of-"):
                ok = wgs == -(-int(count) // (threads // 64))
                pred = f"{count} {what.replace('-', ' ')}"
            else:
                ok = (wgs, threads) == (int(count), int(what))
                pred = f"{count} x {what}"
            bad += not ok
            print(f"{key:<19} {name:<14} {family:<16} {pred:<24} {kernel} {wgs} x {threads}{'' if ok else '   <-- DIFFERS'}")
    return 1 if bad else 0


if __name__ == "__main__":
    if sys.argv[1:2] == ["run"]:
        run()
    elif sys.argv[1:2] == ["report"] and len(sys.argv) == 4:
        sys.exit(report(sys.argv[2], sys.argv[3]))
    else:
        sys.exit(__doc__)
