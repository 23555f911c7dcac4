"""Device time of the changepoint (BOCPD) entry on the synthetic M5 block (device-resident, 30,490 x 1,913 raw counts, hazard_lambda
250) and on the same block cut to 400 rows, where the growing phase (fewer than 500 live run lengths) dominates:

    python tools/time_changepoints.py [n_series] [steps] [check_series] [--out profiles/changepoints_m5.txt] [--no-trace]

Per case: the median over `steps` runs of the wall time of anofox_hip_changepoints_device (it returns after its stream has
finished) and series/s; the first `check_series` series are compared with the numpy restatement tests/changepoint_ref.py and the
largest |difference| / max(1, |reference|) is reported (the contract is 1e-12).  Unless --no-trace is given,
the timing loop is then repeated in a fresh child process under `rocprofv3 --kernel-trace --stats` and the kernel's own total is
read from the trace; the registers, scratch and LDS of the kernel come from tools/resource_usage.py.  --out writes the report to
a file as well.  One JSON line per case goes to stdout after the table."""
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

ROWS = (1913, 400)
LAMBDA = 250.0


def run_cases(n, steps, n_check):
    import torch

    import changepoint_ref
    from anofox_forecast_amd import lib, synth
    from anofox_forecast_amd.device import pack_time_major
    T = ROWS[0]
    Y = synth.gen_series(synth.SEED_M5, 0, n, T, 7, positive=False)
    L = lib.load()
    ld = (n + 63) // 64 * 64
    y = torch.from_numpy(pack_time_major(Y, ld)).cuda()
    recs = []
    for rows in ROWS:
        ln = torch.full((ld,), rows, dtype=torch.int32, device="cuda")
        ln[n:] = 0
        prob = torch.empty((rows, ld), dtype=torch.float64, device="cuda")
        flag = torch.empty((rows, ld), dtype=torch.uint8, device="cuda")
        cnt = torch.empty(ld, dtype=torch.int32, device="cuda")
        err = lib.AnofoxError()

        def run():
            if not L.anofox_hip_changepoints_device(y.data_ptr(), ld, ln.data_ptr(), n, rows, LAMBDA, prob.data_ptr(), flag.data_ptr(),
                                                    cnt.data_ptr(), None, C.byref(err)):
                raise RuntimeError(err.message.decode())
        torch.cuda.synchronize()
        run()                            # warm-up
        wall = []
        for _ in range(steps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run()
            wall.append((time.perf_counter() - t0) * 1e3)
        worst, flags_equal = 0.0, True
        if n_check:
            pn, fn = prob[:, :n_check].cpu().numpy(), flag[:, :n_check].cpu().numpy()
            for i in range(n_check):
                f, p, _ = changepoint_ref.bocpd(Y[i, :rows], LAMBDA)
                worst = max(worst, changepoint_ref.rel(pn[:, i], p))
                flags_equal &= bool(np.array_equal(fn[:, i].astype(bool), f))
        ms = float(np.median(wall))
        recs.append({"case": "changepoints", "hazard_lambda": LAMBDA, "n_series": n, "t": rows, "steps": steps, "ms_median": round(ms, 3),
                     "ms_min": round(float(np.min(wall)), 3), "series_per_s": round(n / ms * 1e3), "flagged_points": int(cnt[:n].sum().item()),
                     "checked_series": n_check, "max_rel_diff_vs_restatement": worst, "flags_equal": flags_equal})
        del prob, flag, cnt
    return recs


def kernel_trace_totals(n, steps):
    """{rows: (calls, total ms)} of bocpd_kernel from a rocprofv3 --kernel-trace --stats run of the same loop in a fresh process."""
    exe = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    out = tempfile.mkdtemp(prefix="cp_trace_")
    cmd = [exe, "--kernel-trace", "--stats", "-d", out, "--", sys.executable, os.path.abspath(__file__), str(n), str(steps), "0", "--no-trace"]
    subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=900)
    durs = []
    for db in glob.glob(os.path.join(out, "**", "*.db"), recursive=True):
        con = sqlite3.connect(db)
        tabs = [r[0] for r in con.execute("select name from sqlite_master where type in ('table','view')")]
        kd = [t for t in tabs if t.startswith("rocpd_kernel_dispatch")][0]
        ks = [t for t in tabs if t.startswith("rocpd_info_kernel_symbol")][0]
        durs += [b - a for nme, a, b in con.execute(f"select s.kernel_name, d.start, d.end from {kd} d join {ks} s on d.kernel_id = s.id "
                                                    "order by d.start") if "bocpd_kernel" in nme]
    if not durs:
        import csv
        for f in glob.glob(os.path.join(out, "**", "*kernel_trace.csv"), recursive=True):
            for r in csv.DictReader(open(f)):
                if "bocpd_kernel" in r.get("Kernel_Name", ""):
                    durs.append(int(r["End_Timestamp"]) - int(r["Start_Timestamp"]))
    shutil.rmtree(out, ignore_errors=True)
    per = steps + 1                                       # warm-up + steps dispatches per case, cases in ROWS order
    if len(durs) != per * len(ROWS):
        return {}
    return {rows: (per, sum(durs[k * per:(k + 1) * per]) / 1e6) for k, rows in enumerate(ROWS)}


def resources():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "resource_usage.py"), "changepoint"], capture_output=True, text=True)
    return [" ".join(line.split()) for line in r.stdout.splitlines() if "bocpd_kernel" in line]


def main():
    argv = sys.argv[1:]
    out_path = None
    if "--out" in argv:
        i = argv.index("--out")
        out_path = argv[i + 1]
        del argv[i:i + 2]
    args = [a for a in argv if not a.startswith("--")]
    n = int(args[0]) if len(args) > 0 else 30490
    steps = int(args[1]) if len(args) > 1 else 5
    n_check = int(args[2]) if len(args) > 2 else 8
    trace = {} if "--no-trace" in sys.argv else kernel_trace_totals(n, steps)       # first: the child runs while this process is idle
    recs = run_cases(n, steps, n_check)
    lines = [f"Changepoint detection (BOCPD) entry on one MI355X: {n:,d} x 1,913 raw M5-shape counts (synth.SEED_M5), device-resident",
             f"time-major block, hazard_lambda {LAMBDA:g} (tools/time_changepoints.py {n} {steps} {n_check}).  Wall time of",
             "anofox_hip_changepoints_device, which returns after its stream has finished; the 400-row case is the same block cut to",
             "its first 400 rows (fewer than 500 live run lengths throughout).", ""]
    for r in recs:
        lines.append(f"rows {r['t']:5d}  {r['ms_median']:10.3f} ms/step (min {r['ms_min']:10.3f})  {r['series_per_s']:>10,d} series/s  "
                     f"{r['flagged_points']:,d} flagged points")
    lines.append("")
    if recs and recs[0]["checked_series"]:
        lines.append(f"Against the numpy restatement (tests/changepoint_ref.py), first {recs[0]['checked_series']} series: max |difference| / max(1, |ref|) = "
                     + ", ".join(f"{r['max_rel_diff_vs_restatement']:.3e} ({r['t']} rows)" for r in recs)
                     + f"; flags equal: {all(r['flags_equal'] for r in recs)}.  Contract: 1e-12.")
        lines.append("")
    if trace:
        lines.append("rocprofv3 --kernel-trace --stats, bocpd_kernel (a separate run of the same loop, warm-up included):")
        for rows, (calls, total) in trace.items():
            lines.append(f"rows {rows:5d}  {calls} dispatches, total {total:10.3f} ms, {total / calls:10.3f} ms per dispatch")
            for r in recs:
                if r["t"] == rows:
                    r["trace_ms_per_dispatch"] = round(total / calls, 3)
        lines.append("")
    elif "--no-trace" not in sys.argv:
        lines += ["rocprofv3 --kernel-trace --stats: the trace held no bocpd_kernel dispatches that could be matched to the cases.", ""]
    res = resources()
    if res:
        lines.append("Resources (tools/resource_usage.py changepoint, gfx950):")
        lines += res
    text = "\n".join(lines) + "\n"
    print(text, flush=True)
    if out_path:
        open(out_path, "w").write(text)
    for r in recs:
        print(json.dumps(r))


if __name__ == "__main__":
    main()
