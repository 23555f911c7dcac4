"""Device time of anofox_hip_quality_device on a device-resident block, with stats_kernel on the same block in the same run and the
restatements on the CPU beside it:
    python tools/time_quality.py [n_series] [steps] [--out FILE] [--check N] [--ab LIB_NO_SORT LIB_NO_CHAINS LIB_NEITHER]

The block is the synthetic M5 shape, n_series x 1,913 daily counts, time-major, all rows valid: the 2,048-word LDS tile, 4 waves per
workgroup.  A second case masks 3 % of the rows as NULL (the validity block is read as well, the compacted series are shorter).

A step is one call, which returns after its stream has finished: launch and wait included.  One warm-up call, then `steps` calls;
median and minimum.  anofox_hip_stats_device is timed the same way on the same tensors: stats_kernel loads the same rows, runs the
same sorting network once and sweeps the buffer more often, but its sums are butterflies over lanes, where quality_kernel walks two
passes of dependent fp64 additions in arrival order.

CPU lines: tests/quality_ref.py (pure Python, the yardstick of the tests) on --check series, scaled to the block; and a numpy
restatement of the whole block -- np.sort plus np.cumsum along the time axis, which accumulates in row order and so gives the
sequential sums -- whose five scores are compared with the device's bit for bit.

--ab times the first case again with three experiment builds of the library (csrc/quality.hip, ANOFOX_QUALITY_SKIP = 1, 2, 3: without
the sorting network, without the in-order chains, without both), each in a child process, to split the kernel's time."""
import ctypes as C
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

T_M5 = 1913
EPS = 2.220446049250313e-16


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


def numpy_scores(Y):
    """The five scores of every column of the time-major block Y [T x n], all rows valid and no NaN; sequential sums by cumsum."""
    T, n = Y.shape
    kf = float(T)
    mean = np.cumsum(Y, axis=0)[-1] / kf
    D = Y - mean
    denom = np.cumsum(D * D, axis=0)[-1]
    num = np.cumsum(D[1:] * D[:-1], axis=0)[-1]
    variance = denom / kf
    sd = np.sqrt(variance)
    with np.errstate(divide="ignore", invalid="ignore"):
        acf1 = np.where(np.abs(denom) < EPS, 0.0, num / denom)
    behavioral = np.where(np.abs(variance) < EPS, 0.0, np.where(np.abs(acf1) > 0.95, 1.0 - 0.2, 1.0))
    S = np.sort(Y, axis=0)
    q1, q3 = S[int(kf * 0.25)], S[int(kf * 0.75)]
    iqr = q3 - q1
    outliers = ((Y < q1 - 1.5 * iqr) | (Y > q3 + 1.5 * iqr)).sum(axis=0)
    extreme = (np.abs(D) > 4.0 * sd).sum(axis=0)
    magnitude = np.clip(1.0 - (outliers / kf) * 2.0 - (extreme / kf) * 3.0, 0.0, 1.0)
    structural = np.full(n, min(max((kf / kf) * 0.7 + min(kf / 30.0, 1.0) * 0.3, 0.0), 1.0))
    temporal = np.ones(n)
    return np.stack([structural, temporal, magnitude, behavioral, (structural + temporal + magnitude + behavioral) / 4.0])


def main():
    import torch

    import quality_ref as R
    from anofox_forecast_amd import lib, synth
    from anofox_forecast_amd.device import pack_time_major
    argv = sys.argv[1:]
    out_path = argv[argv.index("--out") + 1] if "--out" in argv else None
    n_check = int(argv[argv.index("--check") + 1]) if "--check" in argv else 64
    ab = argv[argv.index("--ab") + 1:argv.index("--ab") + 4] if "--ab" in argv else None
    first = "--first" in argv
    pos = []
    skip = 0
    for a in argv:
        if skip:
            skip -= 1
        elif a in ("--out", "--check"):
            skip = 1
        elif a == "--ab":
            skip = 3
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
    fp = torch.zeros((5, ld), dtype=torch.float64, device=dev)
    it = torch.zeros((4, ld), dtype=torch.int64, device=dev)
    err = lib.AnofoxError()

    def quality(valid=None):
        if not L.anofox_hip_quality_device(y.data_ptr(), None if valid is None else valid.data_ptr(), ld, lens.data_ptr(), n, T_M5, fp.data_ptr(),
                                           it.data_ptr(), None, C.byref(err)):
            raise RuntimeError(err.message.decode())

    med, lo = timed(quality, steps)
    if first:                                    # a child of --ab: the one number
        print(f"QUALITY_MS {med:.4f} {lo:.4f}")
        return
    lines = [f"anofox_hip_quality_device on one {torch.cuda.get_device_name(0)}, device-resident, {n:,d} series x {T_M5:,d} rows (synthetic M5 counts), "
             f"tile 2048 words = 16 KiB per wave, 4 waves per workgroup, {steps} steps, median (min) ms per step:",
             f"    quality, all rows valid            : {med:8.3f} ({lo:8.3f})   {8.0 * T_M5 * n / (med * 1e-3) / 1e12:5.2f} TB/s of values read, "
             f"{n / med * 1e3:,.0f} series/s"]
    got = fp.cpu().numpy()[:, :n].copy()
    got_int = it.cpu().numpy()[:, :n].copy()

    gen = torch.Generator(device=dev).manual_seed(20261018)
    valid = (torch.rand((T_M5, ld), generator=gen, device=dev) >= 0.03).to(torch.uint8).contiguous()
    med_v, lo_v = timed(lambda: quality(valid), steps)
    lines.append(f"    quality, 3 % of the rows NULL      : {med_v:8.3f} ({lo_v:8.3f})")
    got_v, got_v_int = fp.cpu().numpy()[:, :n].copy(), it.cpu().numpy()[:, :n].copy()

    oi = torch.zeros((14, ld), dtype=torch.int64, device=dev)
    of = torch.zeros((22, ld), dtype=torch.float64, device=dev)

    def stats():
        if not L.anofox_hip_stats_device(y.data_ptr(), None, None, ld, lens.data_ptr(), n, T_M5, 0, 0, oi.data_ptr(), of.data_ptr(), None, C.byref(err)):
            raise RuntimeError(err.message.decode())

    med_s, lo_s = timed(stats, steps)
    lines.append(f"    stats (anofox_hip_stats_device) on the same block, the same run: {med_s:8.3f} ({lo_s:8.3f})   quality / stats = {med / med_s:.2f}")

    # the restatements
    n_check = min(n_check, n)
    hv = valid.cpu().numpy()
    t0 = time.perf_counter()
    equal = True
    for i in range(n_check):
        want, status = R.data_quality([float(v) for v in Y[i]])
        equal &= status == 0 and all(R.same_bits(got[k, i], want[f]) for k, f in enumerate(R.FP_FIELDS))
        equal &= (int(got_int[1, i]), int(got_int[2, i]), int(got_int[3, i])) == (want["n_missing"], int(want["is_constant"]), 0)
    t_py = time.perf_counter() - t0
    equal_v = True
    for i in range(n_check):
        want, status = R.data_quality([float(v) if ok else None for v, ok in zip(Y[i], hv[:, i])])
        equal_v &= status == 0 and all(R.same_bits(got_v[k, i], want[f]) for k, f in enumerate(R.FP_FIELDS))
        equal_v &= int(got_v_int[1, i]) == want["n_missing"]
    lines.append(f"    tests/quality_ref.py (pure Python) on {n_check} series, one process: {t_py * 1e3:9.1f} ms, i.e. {t_py / max(n_check, 1) * n:8.1f} s "
                 f"for the block; equal to the device bit for bit: {bool(equal)} (all valid), {bool(equal_v)} (3 % NULL)")
    Yt = np.ascontiguousarray(Y.T)
    t0 = time.perf_counter()
    ref = np.concatenate([numpy_scores(Yt[:, c:c + 4096]) for c in range(0, n, 4096)], axis=1)     # (column blocks bound the temporaries)
    t_np = (time.perf_counter() - t0) * 1e3
    same = bool(np.array_equal(ref.view(np.uint64), got.view(np.uint64)))
    lines.append(f"    numpy restatement (np.sort + np.cumsum along time) of the whole block, one process: {t_np:9.1f} ms; "
                 f"equal to the device bit for bit: {same}" + ("" if same else f" ({int((ref.view(np.uint64) != got.view(np.uint64)).any(axis=0).sum())} series differ)"))

    if ab:
        names = ("without the sorting network", "without the in-order chains", "without both")
        times = []
        for p in ab:
            env = dict(os.environ, ANOFOX_HIP_LIB=os.path.abspath(p))
            r = subprocess.run([sys.executable, os.path.abspath(__file__), str(n), str(steps), "--first"], env=env, capture_output=True, text=True,
                               timeout=300)
            m = [l for l in r.stdout.splitlines() if l.startswith("QUALITY_MS")]
            times.append(float(m[0].split()[1]) if m else None)
        lines.append(f"Split of the all-valid step by experiment builds (ANOFOX_QUALITY_SKIP = 1, 2, 3), each in a process of its own: {med:.3f} ms in full;")
        for nm, t in zip(names, times):
            lines.append(f"    {nm:28s}: " + ("failed" if t is None else f"{t:8.3f} ms ({med - t:+.3f} ms against the full kernel)"))
    ru = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "resource_usage.py"), "quality", "stats"], capture_output=True, text=True).stdout
    lines += ["", "Resources (tools/resource_usage.py quality stats, gfx950; quality_kernel adds waves x tile x 8 bytes of dynamic LDS per workgroup, "
              "at most 64 KiB):", ru.rstrip()]
    text = "\n".join(lines) + "\n"
    print(text)
    if out_path:
        open(out_path, "w").write(text)


if __name__ == "__main__":
    main()
