"""Device time of the data-preparation entry (anofox_hip_prepare_device) on a device-resident raw block:

    python tools/time_dataprep.py [n_series] [steps] [check_series] [--out profiles/dataprep_m5.txt] [--no-trace] [--no-cpu]

The block is the synthetic M5 shape (30,490 x 1,913 intermittent counts, synth.SEED_M5: leading zero runs as the generator makes
them) with a seeded 5 % of the rows of every series removed (the remaining rows move up: gaps in the dates) and a further 5 %
masked (NULLs).  Cases: every fill mode alone, the edge trim alone, the gaps stage alone, and the chains gaps + edge trim + const 0
and gaps + edge trim + interpolate.  Per case: a count call sizes the output block, then the median over `steps` runs of the wall
time of the full call (it returns after its stream has finished) and the algorithmic bytes per second -- the cells of the blocks
the call reads (values 8 B, validity 1 B, dates 8 B when the stage needs them) plus the cells it writes, each counted once.  The
first `check_series` series of every case are compared with the restatement tests/dataprep_ref.py (bits).

In the same call, the route this replaces: anofox_hip_batch_pack_host of the same raw series with their masks (host
interpolation, pack and H2D; no gaps and no trim, which the host route would need SQL or Python for), and unless --no-cpu the
restatement's chain gaps + edge trim + interpolate on 15 processes.  Unless --no-trace, the timing loop runs again in a fresh
child process under `rocprofv3 --kernel-trace --stats` and the time per dispatch of the kernel is read from the trace; the
registers, scratch and LDS come from tools/resource_usage.py."""
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
CPU_SERIES, CPU_PROCS = 600, 15
CHAIN = dict(gaps=True, frequency_micros=DAY, trim="edge")
CASES = ([("fill_" + f, dict(fill=f, fill_value=0.0)) for f in ("none", "const", "forward", "backward", "mean", "interpolate")]
         + [("trim_edge", dict(trim="edge")), ("gaps", dict(gaps=True, frequency_micros=DAY)),
            ("gaps_edge_const0", dict(CHAIN, fill="const", fill_value=0.0)), ("gaps_edge_interpolate", dict(CHAIN, fill="interpolate"))])


def raw_block(n):
    """(y, valid, dates time-major [T, ld], lengths [ld], ld) on the host: 5 % of the rows removed, a further 5 % masked."""
    from anofox_forecast_amd import synth
    Y = synth.gen_series(synth.SEED_M5, 0, n, T_M5, 7, positive=False)
    rng = np.random.Generator(np.random.Philox(key=[20261018, 1]))
    keep = rng.random((n, T_M5)) >= 0.05
    keep[:, 0] = keep[:, -1] = True
    ok = rng.random((n, T_M5)) >= 0.05
    ld = (n + 63) // 64 * 64
    pos = np.cumsum(keep, axis=1) - 1
    col = np.broadcast_to(np.arange(n)[:, None], (n, T_M5))
    day = np.broadcast_to(np.arange(T_M5, dtype=np.int64)[None, :] * DAY, (n, T_M5))
    y = np.zeros((T_M5, ld))
    v = np.ones((T_M5, ld), dtype=np.uint8)
    d = np.zeros((T_M5, ld), dtype=np.int64)
    y[pos[keep], col[keep]] = Y[keep]
    v[pos[keep], col[keep]] = ok[keep]
    d[pos[keep], col[keep]] = day[keep]
    ln = np.zeros(ld, dtype=np.int32)
    ln[:n] = keep.sum(axis=1)
    return y, v, d, ln, ld


def _ref_chunk(chunk):
    import dataprep_ref as R
    return [len(R.prepare(d, c, gaps=True, frequency_micros=DAY, trim="edge", fill="interpolate")["values"]) for d, c in chunk]


def host_series(y, v, d, ln, k):
    return [([int(x) for x in d[:ln[s], s]], [float(a) if o else None for a, o in zip(y[:ln[s], s], v[:ln[s], s])]) for s in range(k)]


def cpu_restatement_seconds(series):
    from concurrent.futures import ProcessPoolExecutor
    chunks = [series[i::CPU_PROCS] for i in range(CPU_PROCS)]
    with ProcessPoolExecutor(CPU_PROCS) as ex:
        list(ex.map(_ref_chunk, [c[:1] for c in chunks]))          # start the workers
        t0 = time.perf_counter()
        list(ex.map(_ref_chunk, chunks))
        return time.perf_counter() - t0


def pack_host_ms(L, lib, y, v, ln, n, reps=3):
    """anofox_hip_batch_pack_host of the raw series with their masks: host interpolation, pack, H2D."""
    from anofox_forecast_amd import api
    vals = [np.ascontiguousarray(y[:ln[s], s]) for s in range(n)]
    masks = [api.validity_mask(v[:ln[s], s] != 0) for s in range(n)]
    opts = lib.make_options("Naive", 7)
    hb, err = C.c_void_p(), lib.AnofoxError()
    if not L.anofox_hip_batch_create(n, T_M5, C.byref(opts), C.byref(hb), C.byref(err)):
        raise RuntimeError(err.message.decode())
    vptr = (C.c_void_p * n)(*[a.ctypes.data for a in vals])
    mptr = (C.c_void_p * n)(*[m.ctypes.data for m in masks])
    lens = (C.c_size_t * n)(*[len(a) for a in vals])
    out = []
    for _ in range(reps + 1):
        t0 = time.perf_counter()
        if not L.anofox_hip_batch_pack_host(hb, vptr, mptr, lens, C.byref(err)):
            raise RuntimeError(err.message.decode())
        out.append((time.perf_counter() - t0) * 1e3)
    L.anofox_hip_batch_destroy(hb)
    return float(np.median(out[1:]))


def run_cases(n, steps, n_check):
    import torch

    import dataprep_ref as R
    from anofox_forecast_amd import lib
    L = lib.load()
    hy, hv, hd, hln, ld = raw_block(n)
    y, v, d, ln = (torch.from_numpy(a).cuda() for a in (hy, hv, hd, hln))
    len_out = torch.zeros(ld, dtype=torch.int32, device="cuda")
    fig = torch.zeros((8, ld), dtype=torch.int64, device="cuda")
    mm = torch.zeros((2, ld), dtype=torch.float64, device="cuda")
    err = lib.AnofoxError()
    rows_in = int(hln[:n].sum())
    check = host_series(hy, hv, hd, hln, n_check)
    recs = []
    for name, kw in CASES:
        o = lib.make_prep_options(**kw)
        dated = bool(kw.get("gaps"))

        def call(t_out, yo, vo, do):
            p = lambda t: t.data_ptr() if t is not None else None
            if not L.anofox_hip_prepare_device(y.data_ptr(), v.data_ptr(), d.data_ptr() if dated else None, ld, ln.data_ptr(), n, T_M5, C.byref(o),
                                               C.sizeof(o), t_out, p(yo), p(vo), p(do), len_out.data_ptr(), fig.data_ptr(), mm.data_ptr(), None,
                                               C.byref(err)):
                raise RuntimeError(err.message.decode())
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        call(0, None, None, None)
        count_ms = (time.perf_counter() - t0) * 1e3
        t_out = max(1, int(len_out[:n].max().item()))
        yo = torch.zeros((t_out, ld), dtype=torch.float64, device="cuda")
        vo = torch.zeros((t_out, ld), dtype=torch.uint8, device="cuda")
        do = torch.zeros((t_out, ld), dtype=torch.int64, device="cuda") if dated else None
        call(t_out, yo, vo, do)                                    # warm-up
        wall = []
        for _ in range(steps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            call(t_out, yo, vo, do)
            wall.append((time.perf_counter() - t0) * 1e3)
        rows_out = int(len_out[:n].sum().item())
        equal = True
        if n_check:
            gy, gv, gl = yo[:, :n_check].cpu().numpy(), vo[:, :n_check].cpu().numpy(), len_out[:n_check].cpu().numpy()
            gd = do[:, :n_check].cpu().numpy() if dated else None
            gf, gm = fig[:, :n_check].cpu().numpy(), mm[:, :n_check].cpu().numpy()
            for s, (dd, cc) in enumerate(check):
                ref = R.prepare(dd if dated else None, cc, ftype="FIXED", **{k: w for k, w in kw.items()})
                k = int(gl[s])
                got = [float(a) if ok else None for a, ok in zip(gy[:k, s], gv[:k, s])]
                equal &= R.same_values(got, ref["values"]) and list(gf[:, s]) == ref["figures"]
                equal &= all(R.bits(a) == R.bits(b) or (a != a and b != b) for a, b in zip(gm[:, s], (ref["min"], ref["max"])))
                if dated:
                    equal &= list(gd[:k, s]) == ref["dates"]
        ms = float(np.median(wall))
        per_in, per_out = 9 + (8 if dated else 0), 9 + (8 if dated else 0)
        nbytes = float(per_in * rows_in + per_out * rows_out)
        recs.append({"case": name, "n_series": n, "rows_in": rows_in, "rows_out": rows_out, "t_out": t_out, "steps": steps,
                     "ms_median": round(ms, 3), "ms_min": round(float(np.min(wall)), 3), "count_call_ms": round(count_ms, 3),
                     "algorithmic_TB_per_s": round(nbytes / ms / 1e9, 4), "checked_series": n_check, "equal_bits": bool(equal)})
        del yo, vo, do
    return recs, (L, lib, hy, hv, hd, hln)


def kernel_trace(n, steps):
    """Durations (ns) of the dataprep_kernel dispatches of a rocprofv3 --kernel-trace --stats run of the same loop, in order."""
    exe = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    out = tempfile.mkdtemp(prefix="dataprep_trace_")
    cmd = [exe, "--kernel-trace", "--stats", "-d", out, "--", sys.executable, os.path.abspath(__file__), str(n), str(steps), "0", "--no-trace",
           "--no-cpu", "--no-host"]
    subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=600)
    durs = []
    for db in glob.glob(os.path.join(out, "**", "*.db"), recursive=True):
        con = sqlite3.connect(db)
        tabs = [r[0] for r in con.execute("select name from sqlite_master where type in ('table','view')")]
        kd = [t for t in tabs if t.startswith("rocpd_kernel_dispatch")][0]
        ks = [t for t in tabs if t.startswith("rocpd_info_kernel_symbol")][0]
        durs += [b - a for nme, a, b in con.execute(f"select s.kernel_name, d.start, d.end from {kd} d join {ks} s on d.kernel_id = s.id "
                                                    "order by d.start") if "dataprep_kernel" in nme]
    shutil.rmtree(out, ignore_errors=True)
    per = steps + 2                                                # count call, warm-up, steps
    return [durs[k:k + per] for k in range(0, len(durs), per)]


def resources():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "resource_usage.py"), "dataprep"], capture_output=True, text=True)
    return [" ".join(line.split()) for line in r.stdout.splitlines() if "dataprep_" in line]


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
    trace = None if "--no-trace" in argv else kernel_trace(n, steps)          # first: the child runs while this process is idle
    recs, (L, lib, hy, hv, hd, hln) = run_cases(n, steps, n_check)
    lines = ["Data-preparation entry (anofox_hip_prepare_device) on one MI355X, device-resident raw block of the synthetic M5 shape",
             f"(tools/time_dataprep.py {n} {steps} {n_check}): 5 % of the rows removed, a further 5 % masked, the generator's leading zeros.",
             "Wall time of the full call, which returns after its stream has finished; TB/s is the algorithmic traffic, the cells read",
             "plus the cells written, each once (croston_kernel: 0.80 TB/s for one sweep of that block, profiles/intermittent_m5.txt).", ""]
    for r in recs:
        lines.append(f"{r['case']:22s} rows {r['rows_in']:>11,d} -> {r['rows_out']:>11,d}  {r['ms_median']:9.3f} ms/step (min {r['ms_min']:9.3f}, "
                     f"count call {r['count_call_ms']:8.3f})  {r['algorithmic_TB_per_s']:7.4f} TB/s  bits equal on {r['checked_series']}: {r['equal_bits']}")
    lines.append("")
    if trace:
        lines.append("rocprofv3 --kernel-trace --stats (a separate run of the same loop), dataprep_kernel per dispatch: count call / mean of the full calls")
        for r, durs in zip(recs, trace):
            if len(durs) >= 2:
                full = durs[1:]
                lines.append(f"{r['case']:22s} {durs[0] / 1e6:9.3f} ms / {sum(full) / len(full) / 1e6:9.3f} ms  ({len(durs)} dispatches)")
                r["trace_ms_per_full_dispatch"] = round(sum(full) / len(full) / 1e6, 3)
        lines.append("")
    elif "--no-trace" not in argv:
        lines += ["rocprofv3 --kernel-trace --stats: the trace held no dataprep_kernel dispatches.", ""]
    chain = recs[-1]
    if "--no-host" not in argv:
        ph = pack_host_ms(L, lib, hy, hv, hln, n)
        lines += [f"The route this replaces, same raw series: anofox_hip_batch_pack_host with the masks (host interpolation, pack, H2D) {ph:.1f} ms",
                  f"against {recs[5]['ms_median']:.3f} ms for fill_interpolate on the resident block ({ph / recs[5]['ms_median']:.1f} x) and {chain['ms_median']:.3f} ms for the whole chain",
                  "gaps + edge trim + interpolate, which the host route does not do at all.", ""]
        chain["pack_host_ms"] = round(ph, 1)
    if "--no-cpu" not in argv:
        k = min(CPU_SERIES, n)
        sec = cpu_restatement_seconds(host_series(hy, hv, hd, hln, k))
        full = sec * n / k
        lines += [f"The restatement tests/dataprep_ref.py (chain gaps + edge trim + interpolate) on {CPU_PROCS} CPU processes: {sec:.2f} s for the first {k:,d}",
                  f"series, i.e. {full:.1f} s for the block at that rate against {chain['ms_median'] / 1e3:.4f} s on the GPU.  It is Python and slower than the",
                  "reference's Rust and SQL; the ratio is not a speed-up over the reference.", ""]
        chain["cpu_restatement_s_for_block"] = round(full, 2)
    res = resources()
    if res:
        lines.append("Resources (tools/resource_usage.py dataprep, gfx950):")
        lines += res
    text = "\n".join(lines) + "\n"
    print(text, flush=True)
    if out_path:
        open(out_path, "w").write(text)
    for r in recs:
        print(json.dumps(r))


if __name__ == "__main__":
    main()
