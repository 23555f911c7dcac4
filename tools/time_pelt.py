"""Device time of the PELT entry (csrc/pelt.hip) on the synthetic M5 block (device-resident, 30,490 x 1,913 raw counts, min_size 2,
default penalty 2 ln n) and on the same block cut to its first 400 rows:

    python tools/time_pelt.py [n_series] [steps] [check_series] [--rows 1913,400] [--literal K] [--ubench tools/ubench/op_rates]
                              [--out profiles/pelt_m5.txt] [--no-trace]

Per case: the median over `steps` runs of anofox_hip_pelt_device between two events on its stream (and the wall time of the call,
which returns after the stream has finished), series/s and pair-steps/s -- a pair-step is one subtract-multiply-add of the second
pass, n^3 / 6 of them per series of n rows.  The first `check_series` series of the 400-row case are compared with the restatement
tests/pelt_ref.py: changepoints and the bits of the cost must be EQUAL.  --literal K times the literal Python restatement on the first K
series cut to 400 rows (64: the slice itself; another K is scaled to 64 and called an extrapolation).  --ubench runs the micro-benchmark binary (built beforehand from
tools/ubench/op_rates.hip) and relates the pair-step rate to the fp64 issue rate of a dependent subtract-multiply-add.  Unless
--no-trace is given, the timing loop is repeated in a fresh child process under `rocprofv3 --kernel-trace --stats` and the kernel's
own total is read from the trace.  An experiment build with another PELT_TSTAR (t* per sweep) is timed by pointing ANOFOX_HIP_LIB
at it.  The registers, scratch and LDS come from tools/resource_usage.py.  One JSON line per case goes to stdout after the table."""
import ctypes as C
import glob
import json
import os
import re
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

MIN_SIZE, PENALTY = 2, 0.0


def pair_steps(rows):
    return rows ** 3 / 6.0


def run_cases(n, steps, n_check, rows_list):
    import torch

    import pelt_ref
    from anofox_forecast_amd import lib, synth
    from anofox_forecast_amd.device import pack_time_major
    T = max(rows_list)
    Y = synth.gen_series(synth.SEED_M5, 0, n, T, 7, positive=False)
    L = lib.load()
    ld = (n + 63) // 64 * 64
    y = torch.from_numpy(pack_time_major(Y, ld)).cuda()
    st = torch.cuda.current_stream()
    recs = []
    for rows in rows_list:
        ln = torch.full((ld,), rows, dtype=torch.int32, device="cuda")
        ln[n:] = 0
        flag = torch.empty((rows, ld), dtype=torch.uint8, device="cuda")
        cnt = torch.empty(ld, dtype=torch.int32, device="cuda")
        cost = torch.empty(ld, dtype=torch.float64, device="cuda")
        err = lib.AnofoxError()

        def run():
            if not L.anofox_hip_pelt_device(y.data_ptr(), ld, ln.data_ptr(), n, rows, MIN_SIZE, PENALTY, flag.data_ptr(), cnt.data_ptr(),
                                            cost.data_ptr(), C.c_void_p(st.cuda_stream), C.byref(err)):
                raise RuntimeError(err.message.decode())
        torch.cuda.synchronize()
        run()                            # warm-up
        wall, dev = [], []
        for _ in range(steps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            e0.record(st)
            run()
            e1.record(st)
            e1.synchronize()
            wall.append((time.perf_counter() - t0) * 1e3)
            dev.append(e0.elapsed_time(e1))
        equal = None
        if n_check and rows <= 400:
            fl, cn, co = flag[:, :n_check].cpu().numpy(), cnt[:n_check].cpu().numpy(), cost[:n_check].cpu().numpy()
            equal = True
            for i in range(n_check):
                cps, c = pelt_ref.fast(Y[i, :rows], MIN_SIZE, PENALTY)
                equal &= [int(k) for k in np.flatnonzero(fl[:, i])] == cps and int(cn[i]) == len(cps) and pelt_ref.bits(co[i]) == pelt_ref.bits(c)
        ms = float(np.median(dev))
        recs.append({"case": "pelt", "min_size": MIN_SIZE, "n_series": n, "t": rows, "steps": steps, "device_ms_median": round(ms, 3),
                     "device_ms_min": round(float(np.min(dev)), 3), "wall_ms_median": round(float(np.median(wall)), 3),
                     "series_per_s": round(n / ms * 1e3, 1), "pair_steps_per_s": n * pair_steps(rows) / ms * 1e3,
                     "changepoints": int(cnt[:n].sum().item()), "checked_series": n_check if equal is not None else 0, "equal_to_restatement": equal})
        del flag, cnt, cost
    return recs, Y


def kernel_trace_totals(n, steps, rows_list):
    """{rows: (calls, total ms)} of pelt_kernel from a rocprofv3 --kernel-trace --stats run of the same loop in a fresh process."""
    exe = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    out = tempfile.mkdtemp(prefix="pelt_trace_")
    cmd = [exe, "--kernel-trace", "--stats", "-d", out, "--", sys.executable, os.path.abspath(__file__), str(n), str(steps), "0", "--no-trace",
           "--rows", ",".join(str(r) for r in rows_list)]
    subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=900)
    durs = []
    for db in glob.glob(os.path.join(out, "**", "*.db"), recursive=True):
        con = sqlite3.connect(db)
        tabs = [r[0] for r in con.execute("select name from sqlite_master where type in ('table','view')")]
        kd = [t for t in tabs if t.startswith("rocpd_kernel_dispatch")][0]
        ks = [t for t in tabs if t.startswith("rocpd_info_kernel_symbol")][0]
        durs += [b - a for nme, a, b in con.execute(f"select s.kernel_name, d.start, d.end from {kd} d join {ks} s on d.kernel_id = s.id "
                                                    "order by d.start") if "pelt_kernel" in nme]
    shutil.rmtree(out, ignore_errors=True)
    per = steps + 1                                       # warm-up + steps dispatches per case, cases in rows_list order
    if len(durs) != per * len(rows_list):
        return {}
    return {rows: (per, sum(durs[k * per:(k + 1) * per]) / 1e6) for k, rows in enumerate(rows_list)}


def resources():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "resource_usage.py"), "pelt"], capture_output=True, text=True)
    return [" ".join(line.split()) for line in r.stdout.splitlines() if "pelt" in line]


def ubench_rate(path):
    """pair-steps/s the chip issues when every lane runs dependent subtract-multiply-add groups (tools/ubench/op_rates)."""
    import torch
    txt = subprocess.run([path], capture_output=True, text=True, timeout=300).stdout
    m = re.search(r"sub \+ mul \+ add\s+[\d.]+ ms\s+([\d.]+) ns per group", txt)
    if not m:
        return None, txt
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    return cus * 4 * 64 / (float(m.group(1)) * 1e-9), txt


def opt(argv, name, default=None):
    if name in argv:
        i = argv.index(name)
        v = argv[i + 1]
        del argv[i:i + 2]
        return v
    return default


def main():
    argv = sys.argv[1:]
    out_path = opt(argv, "--out")
    rows_list = [int(r) for r in opt(argv, "--rows", "1913,400").split(",")]
    n_literal = int(opt(argv, "--literal", "0"))
    ubench = opt(argv, "--ubench")
    args = [a for a in argv if not a.startswith("--")]
    n = int(args[0]) if len(args) > 0 else 30490
    steps = int(args[1]) if len(args) > 1 else 3
    n_check = int(args[2]) if len(args) > 2 else 8
    trace = {} if "--no-trace" in sys.argv else kernel_trace_totals(n, steps, rows_list)
    recs, Y = run_cases(n, steps, n_check, rows_list)
    lib_name = os.environ.get("ANOFOX_HIP_LIB", "the built library")
    lines = [f"PELT entry (L2 cost, min_size {MIN_SIZE}, default penalty 2 ln n) on one MI355X: {n:,d} x {max(rows_list):,d} raw M5-shape counts",
             f"(synth.SEED_M5), device-resident time-major block (tools/time_pelt.py {n} {steps} {n_check}; {lib_name}).  Device time of",
             "anofox_hip_pelt_device between two events on its stream; a pair-step is one subtract-multiply-add of a segment's second pass,",
             "n^3 / 6 per series.", ""]
    for r in recs:
        lines.append(f"rows {r['t']:5d}  {r['device_ms_median']:12.3f} ms/step (min {r['device_ms_min']:12.3f}, wall {r['wall_ms_median']:12.3f})  "
                     f"{r['series_per_s']:>12,.1f} series/s  {r['pair_steps_per_s']:.3e} pair-steps/s  {r['changepoints']:,d} changepoints")
    lines.append("")
    for r in recs:
        if r["checked_series"]:
            lines += [f"Against the restatement (tests/pelt_ref.py), first {r['checked_series']} series at {r['t']} rows: changepoints, counts and the bits "
                      f"of the cost equal: {r['equal_to_restatement']}.", ""]
    if trace:
        lines.append("rocprofv3 --kernel-trace --stats, pelt_kernel (a separate run of the same loop, warm-up included):")
        for rows, (calls, total) in trace.items():
            lines.append(f"rows {rows:5d}  {calls} dispatches, total {total:12.3f} ms, {total / calls:12.3f} ms per dispatch")
        lines.append("")
    if ubench:
        rate, txt = ubench_rate(ubench)
        if rate:
            lines.append(f"fp64 issue rate of a dependent subtract-multiply-add ({ubench}, 4 chains per wave, 2 waves per SIMD): {rate:.3e} groups/s on the chip")
            lines.append("(built by the command in the file's header, hipcc --offload-arch=gfx950 -O3 -o op_rates op_rates.hip; the group carries its own")
            lines.append("`fp contract(off)`, so it is v_add + v_mul + v_add, the three instructions the kernel pays per pair-step, never an fma);")
            lines += [f"rows {r['t']:5d}  the kernel runs at {r['pair_steps_per_s'] / rate * 100:.1f} % of it" for r in recs]
            lines.append("")
    if n_literal:
        t0 = time.perf_counter()
        import pelt_ref
        for i in range(n_literal):
            pelt_ref.literal(Y[i, :400], MIN_SIZE, PENALTY)
        per = (time.perf_counter() - t0) / n_literal
        whole = f"{per * 64:.0f} s for the 64-series slice, all of it timed" if n_literal == 64 else \
            f"{per * 64:.0f} s for a 64-series slice by extrapolation from the {n_literal} timed"
        lines += [f"The literal Python restatement on one CPU thread, series of 400 rows: {per:.2f} s per series, {whole}.", ""]
    res = resources()
    if res:
        lines.append("Resources (tools/resource_usage.py pelt, gfx950; pelt_kernel adds (min(t_rows, 2048) + 1) x 26 bytes of dynamic LDS):")
        lines += res
    text = "\n".join(lines) + "\n"
    print(text, flush=True)
    if out_path:
        open(out_path, "w").write(text)
    for r in recs:
        print(json.dumps(r))


if __name__ == "__main__":
    main()
