"""Device time of the per-series statistics entry (anofox_hip_stats_device) on device-resident time-major blocks:

    python tools/time_stats.py [n_series] [steps] [check_series] [--out profiles/stats_m5.txt] [--no-trace] [--no-cpu] [--no-big]
                               [--ab LIB_NO_STABILITY LIB_NO_SORT]

Cases: the synthetic M5 block (30,490 x 1,913, synth.SEED_M5) as raw counts and as the positive variant, the raw counts with a
block of daily dates (sorted, so the date sort is skipped) and with the dates of every series reversed (sorted by the network);
1,048,576 x 1,024 Poisson(1) counts drawn on the device (--no-big leaves it out); 2,048 series of 5,000 rows, which take the
general path (workspace in global memory).  Per case: the median over `steps` runs of the wall time of the entry (it returns after
its stream has finished), series/s and the algorithmic bytes per second (8 T N for the values, twice that with dates).  The first
`check_series` series of every case are compared with the restatement tests/stats_ref.py: the largest deviation
|a - b| / max(1, |b|) per figure, and whether every exact figure is equal.  Unless --no-cpu is given, the restatement itself is
timed on the first 3,000 series of the M5 counts on 15 processes.  Unless --no-trace is given, the timing loop is repeated in a
fresh child process under `rocprofv3 --kernel-trace --stats` and the per-dispatch time of the kernels is read from the trace; the
registers, scratch and LDS of the kernels come from tools/resource_usage.py.  --ab times the first case again with two experiment
builds of the library (csrc/stats.hip, ANOFOX_STATS_SKIP=1 and =2), each in a child process, to split the kernel's time into
stability, the sorting network and the rest."""
import ctypes as C
import glob
import json
import os
import shutil
import sqlite3
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

T_M5 = 1913
DAY = 86400 * 10**6
CPU_SERIES, CPU_PROCS = 3000, 15


def _ref_chunk(block):
    import stats_ref
    return [stats_ref.compute(y) for y in block]


def cpu_restatement_seconds(Y):
    from concurrent.futures import ProcessPoolExecutor
    chunks = [Y[i::CPU_PROCS] for i in range(CPU_PROCS)]
    with ProcessPoolExecutor(CPU_PROCS) as ex:
        list(ex.map(_ref_chunk, [c[:2] for c in chunks]))          # start the workers
        t0 = time.perf_counter()
        list(ex.map(_ref_chunk, chunks))
        return time.perf_counter() - t0


def run_cases(n, steps, n_check, big, only_first=False):
    import torch

    import stats_ref as R
    from anofox_forecast_amd import lib, synth
    from anofox_forecast_amd.device import pack_time_major
    L = lib.load()
    Y = synth.gen_series(synth.SEED_M5, 0, n, T_M5, 7, positive=False)
    ld = (n + 63) // 64 * 64
    y = torch.from_numpy(pack_time_major(Y, ld)).cuda()
    days = torch.arange(T_M5, dtype=torch.int64, device="cuda")[:, None] * DAY + torch.zeros((1, ld), dtype=torch.int64, device="cuda")
    cases = [("m5_counts", y, None, n, T_M5)]
    if not only_first:
        cases += [("m5_positive", y + 1.0, None, n, T_M5), ("m5_counts_dates_sorted", y, days.contiguous(), n, T_M5),
                  ("m5_counts_dates_reversed", y, torch.flip(days, dims=[0]).contiguous(), n, T_M5)]
        if big:
            nb = 1 << 20
            cases.append(("poisson_1M_x_1024", None, None, nb, 1024))
        gen = torch.Generator(device="cuda").manual_seed(20261006)
        cases.append(("long_2048_x_5000", 10.0 + 3.0 * torch.randn((5000, 2048), generator=gen, dtype=torch.float64, device="cuda"), None, 2048, 5000))
    recs = []
    for name, blk, dts, ns, rows in cases:
        if blk is None:
            gen = torch.Generator(device="cuda").manual_seed(20261007)
            blk = torch.poisson(torch.ones((rows, ns), dtype=torch.float32, device="cuda"), generator=gen).double()
        cld = blk.shape[1]
        ln = torch.full((cld,), rows, dtype=torch.int32, device="cuda")
        ln[ns:] = 0
        oi = torch.empty((14, cld), dtype=torch.int64, device="cuda")
        of = torch.empty((22, cld), dtype=torch.float64, device="cuda")
        err = lib.AnofoxError()

        def run():
            if not L.anofox_hip_stats_device(blk.data_ptr(), None, dts.data_ptr() if dts is not None else None, cld, ln.data_ptr(), ns, rows,
                                             DAY, 0, oi.data_ptr(), of.data_ptr(), None, C.byref(err)):
                raise RuntimeError(err.message.decode())
        torch.cuda.synchronize()
        run()                            # warm-up
        wall = []
        for _ in range(steps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run()
            wall.append((time.perf_counter() - t0) * 1e3)
        worst, exact = {f: 0.0 for f in R.TOL_FP}, True
        if n_check:
            hy = blk[:, :n_check].cpu().numpy()
            hd = dts[:, :n_check].cpu().numpy() if dts is not None else None
            hi, hf = oi[:, :n_check].cpu().numpy(), of[:, :n_check].cpu().numpy()
            for i in range(n_check):
                ref = R.compute(hy[:, i], None, None if hd is None else hd[:, i], DAY, "FIXED")
                for k, f in enumerate(R.INT_FIELDS):
                    exact &= int(hi[k, i]) == int(ref[f])
                if hd is not None:
                    exact &= int(hi[12, i]) == ref["expected_length"] and int(hi[13, i]) == ref["n_gaps"]
                for k, f in enumerate(R.FP_FIELDS):
                    if f in R.EXACT_FP:
                        exact &= R.same(float(hf[k, i]), ref[f])
                    else:
                        worst[f] = max(worst[f], R.deviation(float(hf[k, i]), ref[f]))
        ms = float(np.median(wall))
        nbytes = 8.0 * rows * ns * (2 if dts is not None else 1)
        recs.append({"case": name, "n_series": ns, "t": rows, "dates": dts is not None, "steps": steps, "ms_median": round(ms, 3),
                     "ms_min": round(float(np.min(wall)), 3), "series_per_s": round(ns / ms * 1e3), "algorithmic_TB_per_s": round(nbytes / ms / 1e9, 4),
                     "checked_series": n_check, "exact_figures_equal": bool(exact), "max_deviation": {f: worst[f] for f in worst if worst[f] > 0}})
        del oi, of, blk
    return recs, Y


def kernel_trace(n, steps, big):
    """[(kernel, calls, mean ms)] per case, in case order, from a rocprofv3 --kernel-trace --stats run of the same loop."""
    exe = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    out = tempfile.mkdtemp(prefix="stats_trace_")
    cmd = [exe, "--kernel-trace", "--stats", "-d", out, "--", sys.executable, os.path.abspath(__file__), str(n), str(steps), "0", "--no-trace",
           "--no-cpu"] + ([] if big else ["--no-big"])
    subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=900)
    rows = []
    for db in glob.glob(os.path.join(out, "**", "*.db"), recursive=True):
        con = sqlite3.connect(db)
        tabs = [r[0] for r in con.execute("select name from sqlite_master where type in ('table','view')")]
        kd = [t for t in tabs if t.startswith("rocpd_kernel_dispatch")][0]
        ks = [t for t in tabs if t.startswith("rocpd_info_kernel_symbol")][0]
        rows += [(nme, b - a) for nme, a, b in con.execute(f"select s.kernel_name, d.start, d.end from {kd} d join {ks} s on d.kernel_id = s.id "
                                                           "order by d.start") if "stats_" in nme and "kernel" in nme]
    shutil.rmtree(out, ignore_errors=True)
    short = [d for nme, d in rows if "stats_long_kernel" not in nme]
    long_ = [d for nme, d in rows if "stats_long_kernel" in nme]
    per = steps + 1
    return [short[k:k + per] for k in range(0, len(short), per)], long_


def resources():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "resource_usage.py"), "stats"], capture_output=True, text=True)
    return [" ".join(line.split()) for line in r.stdout.splitlines() if "stats_" in line]


def ab_ms(libpath, n, steps):
    env = dict(os.environ, ANOFOX_HIP_LIB=os.path.abspath(libpath))
    r = subprocess.run([sys.executable, os.path.abspath(__file__), str(n), str(steps), "0", "--no-trace", "--no-cpu", "--first"], env=env,
                       capture_output=True, text=True, timeout=600)
    for line in r.stdout.splitlines():
        if line.startswith("{"):
            return json.loads(line)["ms_median"]
    return None


def main():
    argv = sys.argv[1:]
    out_path, ab = None, None
    if "--out" in argv:
        i = argv.index("--out")
        out_path = argv[i + 1]
        del argv[i:i + 2]
    if "--ab" in argv:
        i = argv.index("--ab")
        ab = argv[i + 1:i + 3]
        del argv[i:i + 3]
    args = [a for a in argv if not a.startswith("--")]
    n = int(args[0]) if len(args) > 0 else 30490
    steps = int(args[1]) if len(args) > 1 else 5
    n_check = int(args[2]) if len(args) > 2 else 8
    big = "--no-big" not in argv
    trace = None if "--no-trace" in argv else kernel_trace(n, steps, big)      # first: the child runs while this process is idle
    ab_times = [ab_ms(p, n, steps) for p in ab] if ab else None
    recs, Y = run_cases(n, steps, n_check, big, only_first="--first" in argv)
    lines = [f"Per-series statistics entry (anofox_hip_stats_device) on one MI355X, device-resident time-major blocks",
             f"(tools/time_stats.py {n} {steps} {n_check}).  Wall time of the entry, which returns after its stream has finished; TB/s is the",
             "algorithmic traffic: 8 T N bytes for the values, twice that with a date block (croston_kernel: 0.80 TB/s for one sweep of the",
             "M5 block, profiles/intermittent_m5.txt).", ""]
    for r in recs:
        lines.append(f"{r['case']:26s} {r['n_series']:>9,d} x {r['t']:5d}  {r['ms_median']:10.3f} ms/step (min {r['ms_min']:10.3f})  "
                     f"{r['series_per_s']:>11,d} series/s  {r['algorithmic_TB_per_s']:7.4f} TB/s")
    lines.append("")
    if n_check:
        lines.append(f"Against the restatement (tests/stats_ref.py), first {n_check} series of every case: largest |a - b| / max(1, |b|) per figure")
        lines.append("(figures with deviation 0 are left out); the counts, date figures, min, max, range, median, q1, q3, iqr must be equal.")
        for r in recs:
            dev = " ".join(f"{f}={v:.2e}" for f, v in r["max_deviation"].items()) or "all 0"
            lines.append(f"{r['case']:26s} exact figures equal: {r['exact_figures_equal']}; {dev}")
        lines.append("")
    if "--no-cpu" not in argv:
        sec = cpu_restatement_seconds(Y[:CPU_SERIES])
        m5 = recs[0]
        full = sec * m5["n_series"] / min(CPU_SERIES, len(Y))
        lines += [f"The restatement tests/stats_ref.py on {CPU_PROCS} CPU processes: {sec:.2f} s for the first {min(CPU_SERIES, len(Y)):,d} series of the M5 counts,",
                  f"i.e. {full:.1f} s for the block at that rate against {m5['ms_median'] / 1e3:.4f} s on the GPU ({full / (m5['ms_median'] / 1e3):,.0f} x).  The reference's own",
                  "one-thread loop is Rust and is not built here; numpy / Python is slower than it, so this ratio is not a speed-up over the reference.", ""]
        recs[0]["cpu_restatement_s_for_block"] = round(full, 2)
    if trace and trace[0]:
        lines.append("rocprofv3 --kernel-trace --stats (a separate run of the same loop, warm-up included), mean time per dispatch:")
        for r, durs in zip(recs, trace[0]):
            lines.append(f"{r['case']:26s} stats_kernel       {len(durs)} dispatches, {sum(durs) / len(durs) / 1e6:10.3f} ms per dispatch")
            r["trace_ms_per_dispatch"] = round(sum(durs) / len(durs) / 1e6, 3)
        if trace[1]:
            lines.append(f"{recs[-1]['case']:26s} stats_long_kernel  {len(trace[1])} dispatches, {sum(trace[1]) / len(trace[1]) / 1e6:10.3f} ms per dispatch")
        lines.append("")
    elif "--no-trace" not in argv:
        lines += ["rocprofv3 --kernel-trace --stats: the trace held no stats kernel dispatches.", ""]
    if ab_times and all(t is not None for t in ab_times):
        full = recs[0]["ms_median"]
        lines += [f"Split of the {recs[0]['case']} step by experiment builds (ANOFOX_STATS_SKIP): {full:.3f} ms in full, {ab_times[0]:.3f} ms without",
                  f"stability ({full - ab_times[0]:.3f} ms), {ab_times[1]:.3f} ms without the sorting network ({full - ab_times[1]:.3f} ms); the rest is the load, the two",
                  "sweeps and the selections.", ""]
    res = resources()
    if res:
        lines.append("Resources (tools/resource_usage.py stats, gfx950):")
        lines += res
    text = "\n".join(lines) + "\n"
    print(text, flush=True)
    if out_path:
        open(out_path, "w").write(text)
    for r in recs:
        print(json.dumps(r))


if __name__ == "__main__":
    main()
