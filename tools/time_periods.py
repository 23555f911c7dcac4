"""Device time of the period-detection entry on the synthetic M5 block (device-resident, 30,490 x 1,913 raw counts), the three
methods with their default parameters (1,000 frequencies, 50 candidates, zero_pad_factor 4):

    python tools/time_periods.py [n_series] [steps] [check_series] [--out profiles/periods_m5.txt] [--no-trace]

Per method: the median over `steps` runs of the wall time of anofox_hip_periods_device (it returns after its stream has
finished), series/s and sin/cos pairs per second (pairs counted from the source's loops: 2 n per frequency, 2 n per candidate,
n per DFT bin); the first `check_series` series are compared with the numpy restatement tests/periods_ref.py under their own
contract (periods_ref.contract: the selected index equal, every figure within its tolerance) and the worst deviation is reported
as a fraction of its tolerance; the same series are timed through the restatement on the CPU, and the block's time on the
machine's processes is extrapolated from them.  Unless --no-trace is given, the timing loop is then repeated in a fresh child
process under `rocprofv3 --kernel-trace --stats` and each kernel's time per dispatch is read from the trace; registers, scratch
and LDS come from tools/resource_usage.py.  --out writes the report to a file as well.  One JSON line per method goes to stdout."""
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

T = 1913
METHODS = ("lomb_scargle", "aic", "sazed")
KERNEL = {"lomb_scargle": "periods_ls_kernel", "aic": "periods_aic_kernel", "sazed": "periods_sazed_kernel"}
CPU_PROCESSES = 16


def trig_pairs(method, n):
    """sin/cos pairs of one series of n rows with default parameters, from the source's loops."""
    if method == "lomb_scargle":
        return 1000 * 2 * n
    if method == "aic":
        return 50 * 2 * n
    L = 1
    while L < 4 * n:
        L *= 2
    return (L // 2 - 1) * n


def run_cases(n, steps, n_check):
    import torch

    import periods_ref as R
    from anofox_forecast_amd import lib, synth
    from anofox_forecast_amd.device import pack_time_major
    Y = synth.gen_series(synth.SEED_M5, 0, n, T, 7, positive=False)
    L = lib.load()
    ld = (n + 63) // 64 * 64
    y = torch.from_numpy(pack_time_major(Y, ld)).cuda()
    ln = torch.full((ld,), T, dtype=torch.int32, device="cuda")
    ln[n:] = 0
    recs = []
    for m in METHODS:
        fig = torch.empty((lib.PERIODS_N_FP, ld), dtype=torch.float64, device="cuda")
        idx = torch.empty(ld, dtype=torch.int32, device="cuda")
        st = torch.empty(ld, dtype=torch.int32, device="cuda")
        err = lib.AnofoxError()

        def run():
            if not L.anofox_hip_periods_device(y.data_ptr(), ld, ln.data_ptr(), n, T, lib.PERIOD_METHODS[m], 0.0, 0.0, 0, fig.data_ptr(),
                                               idx.data_ptr(), st.data_ptr(), None, C.byref(err)):
                raise RuntimeError(err.message.decode())
        torch.cuda.synchronize()
        run()                            # warm-up
        wall = []
        for _ in range(steps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run()
            wall.append((time.perf_counter() - t0) * 1e3)
        hf, hi = fig[:, :n_check].cpu().numpy(), idx[:n_check].cpu().numpy()
        worst, index_equal, cpu_s, unsafe = 0.0, True, [], 0
        for i in range(n_check):
            t0 = time.perf_counter()
            R.run(m, Y[i])
            cpu_s.append(time.perf_counter() - t0)
            c = R.contract(m, Y[i])
            if not c["ok"]:
                unsafe += 1              # a near tie: the contract makes no statement about this series
                continue
            index_equal &= int(hi[i]) == c["ref"]["index"]
            for f, tol in R.figure_tolerances(m, c["ref"], c["tol"], T).items():
                want, got = float(c["ref"][f]), float(hf[lib.PERIOD_FIGURES[m].index(f), i])
                if np.isfinite(want) and tol > 0.0:
                    worst = max(worst, abs(got - want) / tol)
        ms = float(np.median(wall))
        print(f"{m}: {ms:.1f} ms per step", file=sys.stderr, flush=True)
        pairs = trig_pairs(m, T) * n
        cpu = float(np.median(cpu_s)) if cpu_s else float("nan")
        recs.append({"case": "periods", "method": m, "n_series": n, "t": T, "steps": steps, "ms_median": round(ms, 3),
                     "ms_min": round(float(np.min(wall)), 3), "series_per_s": round(n / ms * 1e3), "trig_pairs": pairs,
                     "trig_pairs_per_s": pairs / ms * 1e3, "failed_series": int((st[:n] != 0).sum().item()), "checked_series": n_check,
                     "near_ties_not_checked": unsafe, "index_equal": index_equal, "worst_deviation_over_tolerance": worst,
                     "cpu_restatement_s_per_series": cpu, "cpu_block_s_extrapolated": cpu * n / CPU_PROCESSES})
        del fig, idx, st
    return recs


def kernel_trace(n, steps):
    """{method: (dispatches, total ms)} from a rocprofv3 --kernel-trace --stats run of the same loop in a fresh process."""
    exe = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    out = tempfile.mkdtemp(prefix="periods_trace_")
    cmd = [exe, "--kernel-trace", "--stats", "-d", out, "--", sys.executable, os.path.abspath(__file__), str(n), str(steps), "0", "--no-trace"]
    subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=900)
    durs = {m: [] for m in METHODS}
    for db in glob.glob(os.path.join(out, "**", "*.db"), recursive=True):
        con = sqlite3.connect(db)
        tabs = [r[0] for r in con.execute("select name from sqlite_master where type in ('table','view')")]
        kd = [t for t in tabs if t.startswith("rocpd_kernel_dispatch")][0]
        ks = [t for t in tabs if t.startswith("rocpd_info_kernel_symbol")][0]
        for name, a, b in con.execute(f"select s.kernel_name, d.start, d.end from {kd} d join {ks} s on d.kernel_id = s.id order by d.start"):
            for m in METHODS:
                if KERNEL[m] in name:
                    durs[m].append(b - a)
    shutil.rmtree(out, ignore_errors=True)
    return {m: (len(d), sum(d) / 1e6) for m, d in durs.items() if d}


def resources():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "resource_usage.py"), "periods"], capture_output=True, text=True)
    return [" ".join(line.split()) for line in r.stdout.splitlines() if "periods_" in line]


def main():
    argv = sys.argv[1:]
    out_path = None
    if "--out" in argv:
        i = argv.index("--out")
        out_path = argv[i + 1]
        del argv[i:i + 2]
    args = [a for a in argv if not a.startswith("--")]
    n = int(args[0]) if len(args) > 0 else 30490
    steps = int(args[1]) if len(args) > 1 else 3
    n_check = int(args[2]) if len(args) > 2 else 4
    trace = {} if "--no-trace" in sys.argv else kernel_trace(n, steps)       # first: the child runs while this process is idle
    recs = run_cases(n, steps, n_check)
    lines = [f"Period detection entry on one MI355X: {n:,d} x {T:,d} raw M5-shape counts (synth.SEED_M5), device-resident time-major block,",
             f"default parameters: 1,000 frequencies, 50 candidates, zero_pad_factor 4 (tools/time_periods.py {n} {steps} {n_check}).  Wall",
             "time of anofox_hip_periods_device, which returns after its stream has finished.", ""]
    for r in recs:
        lines.append(f"{r['method']:13s} {r['ms_median']:10.3f} ms/step (min {r['ms_min']:10.3f})  {r['series_per_s']:>9,d} series/s  "
                     f"{r['trig_pairs']:.3e} sin/cos pairs, {r['trig_pairs_per_s']:.3e} pairs/s  {r['failed_series']} failed series")
    lines.append("")
    if recs and recs[0]["checked_series"]:
        lines.append(f"Against the numpy restatement (tests/periods_ref.py), first {recs[0]['checked_series']} series, each under its own contract "
                     "(index equal, figures within tolerance):")
        for r in recs:
            lines.append(f"{r['method']:13s} index equal: {r['index_equal']}; worst deviation {r['worst_deviation_over_tolerance']:.3e} of its tolerance; "
                         f"{r['near_ties_not_checked']} near ties outside the contract")
        lines.append("")
        lines.append(f"The restatement on this machine's CPU (median of the same series, one process), and the block over {CPU_PROCESSES} processes, extrapolated:")
        for r in recs:
            lines.append(f"{r['method']:13s} {r['cpu_restatement_s_per_series']:8.3f} s per series, {r['cpu_block_s_extrapolated']:10.1f} s for the block")
        lines.append("")
    if trace:
        lines.append("rocprofv3 --kernel-trace --stats (a separate run of the same loop, warm-up included):")
        for m, (calls, total) in trace.items():
            lines.append(f"{KERNEL[m]:22s} {calls} dispatches, total {total:10.3f} ms, {total / calls:10.3f} ms per dispatch")
            for r in recs:
                if r["method"] == m:
                    r["trace_ms_per_dispatch"] = round(total / calls, 3)
        lines.append("")
    elif "--no-trace" not in sys.argv:
        lines += ["rocprofv3 --kernel-trace --stats: the trace held no dispatches of the period kernels.", ""]
    res = resources()
    if res:
        lines.append("Resources (tools/resource_usage.py periods, gfx950):")
        lines += res
    text = "\n".join(lines) + "\n"
    print(text, flush=True)
    if out_path:
        open(out_path, "w").write(text)
    for r in recs:
        print(json.dumps(r))


if __name__ == "__main__":
    main()
