"""Device time of anofox_hip_seasonality_device on a device-resident block, beside detect_period_kernel (the forecast batch's private
autocorrelation kernel, reached through the auto-detect adoption of the same block) and the numpy restatement on the CPU:
    python tools/time_seasonality.py [n_series] [steps] [--out FILE] [--check N] [--ab LIB ...]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/time_seasonality.py [n_series] [steps] --kernels
    python tools/time_seasonality.py [n_series] [steps] --report DIR [--out FILE]
    python tools/time_seasonality.py --trace-only DIR [n_series]

The block is the synthetic M5 shape, n_series x 1,913 daily counts, time-major, all rows valid; a second case masks 5 % of the rows as
NULL.  Without --kernels a step is one call, which returns after its stream has finished (launch and wait included): one warm-up call,
then `steps` calls, median and minimum.  --kernels only runs the two kernels `steps` times each in one process, for a kernel
trace; --report reads that trace's kernel statistics and adds the two kernel times, their ratio and the algorithmic multiply-adds per second to the wall-clock lines
(--trace-only prints that section alone and needs no GPU).  --ab times the all-valid case with experiment builds of the library
(csrc/seasonality.hip, ANOFOX_SEAS_LAGS = lags per lane), each in a child process."""
import csv
import ctypes as C
import glob
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

T_M5 = 1913


def timed(fn, steps):
    import torch
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(steps):
        t0 = time.perf_counter()
        fn()
        ms.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ms)), float(np.min(ms))


def lag_macs(n):
    """Multiply-adds of the lag sums of one series of n values: sum over lag = 1 .. n / 2 of n - lag."""
    m = n // 2
    return m * n - m * (m + 1) // 2


def numpy_block(Y, max_lag=None):
    """Primary period and its ACF value of every column of the time-major block Y [T x n] (all rows valid): sequential sums by cumsum."""
    T, n = Y.shape
    mean = np.cumsum(Y, axis=0)[-1] / float(T)
    D = Y - mean
    var = np.cumsum(D * D, axis=0)[-1]
    m = T // 2 if max_lag is None else max_lag
    acf = np.empty((m, n))
    with np.errstate(all="ignore"):
        for lag in range(1, m + 1):
            acf[lag - 1] = np.cumsum(D[:T - lag] * D[lag:], axis=0)[-1] / var
    mid = acf[1:-1]
    peak = (mid > acf[:-2]) & (mid > acf[2:]) & (mid > 0.1) & ~(np.abs(var) < 2.220446049250313e-16)
    score = np.where(peak, mid, -np.inf)
    best = score.argmax(axis=0)                           # the first of equal maxima: ascending lag
    has = peak.any(axis=0)
    return np.where(has, best + 2, 0), np.where(has, score[best, np.arange(n)], 0.0)


def kernel_stats(trace_dir):
    """{kernel name: (calls, average ns, minimum ns)} from a rocprofv3 output directory: every *kernel_stats.csv below it, or, where the
    profiler wrote its database instead, the `kernels` view of every *_results.db."""
    out = {}
    for path in glob.glob(os.path.join(trace_dir, "**", "*kernel_stats.csv"), recursive=True):
        with open(path, newline="") as fh:
            for row in csv.DictReader(fh):
                out[row["Name"]] = (int(row["Calls"]), float(row["AverageNs"]), float(row.get("MinNs") or row["AverageNs"]))
    if not out:
        import sqlite3
        for path in glob.glob(os.path.join(trace_dir, "**", "*_results.db"), recursive=True):
            with sqlite3.connect(path) as db:
                for name, calls, avg, lo in db.execute("select name, count(*), avg(end - start), min(end - start) from kernels group by name"):
                    out[name] = (int(calls), float(avg), float(lo))
    return out


def trace_lines(trace_dir, n):
    """The kernel-trace section of the report."""
    macs = lag_macs(T_M5) * n
    ks = kernel_stats(trace_dir)
    new = [v for k, v in ks.items() if "seasonality_kernel" in k]
    old = [v for k, v in ks.items() if "detect_period_kernel" in k]
    if not (new and old):
        return ["", f"Kernel trace: no kernel statistics for both kernels below {trace_dir}"]
    t_new, t_old = new[0][1] / 1e6, old[0][1] / 1e6
    return ["", f"Kernel trace (rocprofv3 --kernel-trace --stats, one process, {new[0][0]} and {old[0][0]} calls, the first of each cold; average "
            f"(minimum) ms per call):",
            f"    seasonality_kernel   : {t_new:8.3f} ({new[0][2] / 1e6:8.3f})   {macs / (t_new * 1e-3) / 1e12:5.2f} T multiply-adds/s of the lag sums",
            f"    detect_period_kernel : {t_old:8.3f} ({old[0][2] / 1e6:8.3f})   {macs / (t_old * 1e-3) / 1e12:5.2f} T multiply-adds/s",
            f"    ratio new / old      : {t_new / t_old:8.3f}   (target: at most 1.10)"]


def main():
    if "--trace-only" in sys.argv:                        # no GPU: only the kernel-trace section of an earlier --kernels run
        n = int(sys.argv[sys.argv.index("--trace-only") + 2]) if len(sys.argv) > sys.argv.index("--trace-only") + 2 else 30490
        print("\n".join(trace_lines(sys.argv[sys.argv.index("--trace-only") + 1], n)))
        return
    import torch

    import seasonality_cases as SC
    from anofox_forecast_amd import lib, synth
    from anofox_forecast_amd.device import DeviceBatch, pack_time_major
    argv = sys.argv[1:]
    opt = lambda name: argv[argv.index(name) + 1] if name in argv else None
    out_path, report = opt("--out"), opt("--report")
    n_check = int(opt("--check") or 64)
    ab = []
    if "--ab" in argv:
        ab = [a for a in argv[argv.index("--ab") + 1:] if not a.startswith("--")]
    pos, skip = [], False
    for a in argv:
        if skip:
            skip = False
        elif a in ("--out", "--check", "--report"):
            skip = True
        elif a == "--ab":
            break
        elif not a.startswith("--"):
            pos.append(a)
    n = int(pos[0]) if pos else 30490
    steps = int(pos[1]) if len(pos) > 1 else 10
    L = lib.load()
    dev = "cuda:0"
    Y = synth.gen_series(synth.SEED_M5, 0, n, T_M5, 7, positive=False)
    ld = (n + 63) // 64 * 64
    y = torch.from_numpy(pack_time_major(Y, ld)).to(dev)
    lens = torch.full((ld,), T_M5, dtype=torch.int32, device=dev)
    oi = torch.zeros((8, ld), dtype=torch.int32, device=dev)
    of = torch.zeros((12, ld), dtype=torch.float64, device=dev)
    err = lib.AnofoxError()

    def seasonality(valid=None):
        if not L.anofox_hip_seasonality_device(y.data_ptr(), None if valid is None else valid.data_ptr(), ld, lens.data_ptr(), n, T_M5, 0,
                                               oi.data_ptr(), of.data_ptr(), None, C.byref(err)):
            raise RuntimeError(err.message.decode())

    opts = lib.make_options("Naive", 14)                  # seasonal_period 0: the adoption runs detect_period_kernel
    batch = DeviceBatch(n, T_M5, opts, dev)

    def adopt():
        batch.set_block(y, lens)
        return batch.periods()

    if "--kernels" in argv:
        for _ in range(steps + 1):
            seasonality()
        for _ in range(steps + 1):
            adopt()
        torch.cuda.synchronize()
        batch.close()
        return
    med, lo = timed(seasonality, steps)
    if "--first" in argv:                                 # a child of --ab: the one number
        print(f"SEASONALITY_MS {med:.4f} {lo:.4f}")
        return
    macs = lag_macs(T_M5) * n
    lines = [f"anofox_hip_seasonality_device on one {torch.cuda.get_device_name(0)}, device-resident, {n:,d} series x {T_M5:,d} rows (synthetic M5 "
             f"counts), {steps} steps, median (min) ms per step (launch and wait included):",
             f"    seasonality, all rows valid        : {med:8.3f} ({lo:8.3f})   {macs / (med * 1e-3) / 1e12:5.2f} T multiply-adds/s of the lag sums, "
             f"{n / med * 1e3:,.0f} series/s"]
    got_i, got_f = oi.cpu().numpy()[:, :n].copy(), of.cpu().numpy()[:, :n].copy()
    gen = torch.Generator(device=dev).manual_seed(20261019)
    valid = (torch.rand((T_M5, ld), generator=gen, device=dev) >= 0.05).to(torch.uint8).contiguous()
    med_v, lo_v = timed(lambda: seasonality(valid), steps)
    lines.append(f"    seasonality, 5 % of the rows NULL  : {med_v:8.3f} ({lo_v:8.3f})")
    got_vi, got_vf = oi.cpu().numpy()[:, :n].copy(), of.cpu().numpy()[:, :n].copy()
    med_a, lo_a = timed(adopt, steps)
    adopted = adopt()[:n]
    batch.close()
    agree = bool(np.array_equal(np.where(got_i[6] == 0, 1, got_i[6]), adopted))
    lines.append(f"    auto-detect adoption of the same block (set_block + periods: detect_period_kernel, the copy of the periods, the batch's own "
                 f"bookkeeping): {med_a:8.3f} ({lo_a:8.3f}); its periods equal primary_period (0 -> 1): {agree}")

    # the restatements
    n_check = min(n_check, n)
    hv = valid.cpu().numpy()

    def col_ok(gi, gf, i, w):
        k = len(w["detected_periods"])
        return ([int(x) for x in gi[:5, i]] == w["detected_periods"] + [0] * (5 - k) and int(gi[5, i]) == k and int(gi[7, i]) == w["status"]
                and all(SC.same_bits(a, b) for a, b in zip(gf[:5, i], w["strengths"] + [0.0] * (5 - k)))
                and SC.same_bits(gf[10, i], w["seasonal_strength"]) and SC.same_bits(gf[11, i], w["trend_strength"]))
    t0 = time.perf_counter()
    equal = all(col_ok(got_i, got_f, i, SC.expected([float(v) for v in Y[i]])) for i in range(n_check))
    t_ref = time.perf_counter() - t0
    equal_v = all(col_ok(got_vi, got_vf, i, SC.expected([float(v) if ok else None for v, ok in zip(Y[i], hv[:, i])])) for i in range(n_check))
    lines.append(f"    tests/seasonality_ref.py (its cumsum form) on {n_check} series, one process: {t_ref * 1e3:9.1f} ms, i.e. "
                 f"{t_ref / max(n_check, 1) * n:8.1f} s for the block; equal to the device bit for bit: {equal} (all valid), {equal_v} (5 % NULL)")
    n_np = min(n, 512)
    Yt = np.ascontiguousarray(Y[:n_np].T)
    t0 = time.perf_counter()
    per, val = numpy_block(Yt)
    t_np = time.perf_counter() - t0
    same = bool(np.array_equal(per, got_i[6, :n_np]) and np.array_equal(val.view(np.uint64), got_f[5, :n_np].view(np.uint64)))
    lines.append(f"    numpy restatement (np.cumsum along time, whole blocks of columns) of {n_np} series, one process: {t_np * 1e3:9.1f} ms, i.e. "
                 f"{t_np / n_np * n:8.1f} s for the block; primary period and its ACF value equal to the device bit for bit: {same}")

    if report:
        lines += trace_lines(report, n)
    if ab:
        lines.append(f"Experiment builds (ANOFOX_SEAS_LAGS, lags per lane), all rows valid, each in a process of its own; this build: {med:.3f} ms")
        for p in ab:
            env = dict(os.environ, ANOFOX_HIP_LIB=os.path.abspath(p))
            r = subprocess.run([sys.executable, os.path.abspath(__file__), str(n), str(steps), "--first"], env=env, capture_output=True, text=True,
                               timeout=300)
            m = [l for l in r.stdout.splitlines() if l.startswith("SEASONALITY_MS")]
            lines.append(f"    {os.path.basename(p):28s}: " + (f"{float(m[0].split()[1]):8.3f} ms" if m else "failed"))
    ru = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "resource_usage.py"), "seasonality"], capture_output=True, text=True).stdout
    lines += ["", "Resources (tools/resource_usage.py seasonality, gfx950; seasonality_kernel<true> adds (1.5 t_rows + 258) x 8 bytes of dynamic "
              f"LDS per workgroup: {(T_M5 + 256 + T_M5 // 2 + 2) * 8:,d} bytes here, 5 waves):", ru.rstrip()]
    text = "\n".join(lines) + "\n"
    print(text)
    if out_path:
        open(out_path, "w").write(text)


if __name__ == "__main__":
    main()
