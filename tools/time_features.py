"""Device time of anofox_hip_features_device on a device-resident block, per call and per kernel, with stats_kernel and
croston_kernel on the same block in the same run as yardsticks, the restatement on the CPU beside it, and the worst deviation of the
device from the restatement in units of the measured noise:
    python tools/time_features.py [n_series] [steps] [--out FILE] [--check N]

The block is the synthetic M5 shape, n_series x 1,913 daily counts, time-major, all rows valid (the 2,048-word LDS tile, one wave per
series), and its first 400 rows (the 512-word tile).  A step is one call, which returns after its stream has finished: launch and
wait included.  One warm-up call, then `steps` calls; median and minimum.  "Per kernel" is a call of
anofox_hip_features_families_device with one family bit set: that kernel alone on the same tensors (plus the 22 KiB Benford table
copy every call makes).  No profiler trace is involved, so the per-kernel times include one launch and one stream wait each.

CPU line: tests/features_ref.py through tests/features_cases.py (numpy counts above 64 rows) on --check series of the 400-row slice,
scaled to the block.  The same series give the deviations: every feature under the equality contract is compared for equality, every
feature under a tolerance as |device - restatement| / noise, where 16 is the tolerance."""
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
T_SHORT = 400


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


def main():
    import torch

    import features_cases as FC
    import features_ref as R
    from anofox_forecast_amd import lib, synth
    from anofox_forecast_amd.device import DeviceBatch, pack_time_major
    argv = sys.argv[1:]
    out_path = argv[argv.index("--out") + 1] if "--out" in argv else None
    n_check = int(argv[argv.index("--check") + 1]) if "--check" in argv else 4
    pos, skip = [], 0
    for a in argv:
        if skip:
            skip -= 1
        elif a in ("--out", "--check"):
            skip = 1
        elif not a.startswith("--"):
            pos.append(a)
    n = int(pos[0]) if pos else 30490
    steps = int(pos[1]) if len(pos) > 1 else 3
    L = lib.load()
    dev = "cuda:0"
    Y = synth.gen_series(synth.SEED_M5, 0, n, T_M5, 7, positive=False)
    ld = (n + 63) // 64 * 64
    y = torch.from_numpy(pack_time_major(Y, ld)).to(dev)
    fp = torch.zeros((lib.N_FEATURES, ld), dtype=torch.float64, device=dev)
    it = torch.zeros((3, ld), dtype=torch.int64, device=dev)
    err = lib.AnofoxError()
    lines = [f"anofox_hip_features_device on one {torch.cuda.get_device_name(0)}, device-resident, {n:,d} series (synthetic M5 counts), one wave per "
             f"series, {steps} steps, median (min) ms per step; a kernel's line is a call with that family alone:"]
    names = lib.feature_names()
    got = {}
    for rows in (T_M5, T_SHORT):
        lens = torch.full((ld,), rows, dtype=torch.int32, device=dev)

        def features(mask=31):
            if not L.anofox_hip_features_families_device(y.data_ptr(), None, ld, lens.data_ptr(), n, rows, mask, fp.data_ptr(), it.data_ptr(), None,
                                                         C.byref(err)):
                raise RuntimeError(err.message.decode())

        med, lo = timed(features, steps)
        lines.append(f"  {rows:,d} rows, tile {max(64, 1 << (rows - 1).bit_length()):,d} words:")
        lines.append(f"    all five kernels                   : {med:10.3f} ({lo:10.3f})   {n / med * 1e3:,.0f} series/s")
        got[rows] = (fp.cpu().numpy()[:, :n].copy(), it.cpu().numpy()[:, :n].copy())
        parts = []
        for k, fam in enumerate(lib.FEATURES_FAMILIES):
            m, l = timed(lambda: features(1 << k), steps)
            parts.append((fam, m))
            lines.append(f"    features_{fam + '_kernel':<26s}: {m:10.3f} ({l:10.3f})")
        top = max(parts, key=lambda p: p[1])
        lines.append(f"    the kernels alone add up to {sum(p[1] for p in parts):.3f} ms; the largest is {top[0]} ({top[1] / sum(p[1] for p in parts):.0%})")

        oi = torch.zeros((14, ld), dtype=torch.int64, device=dev)
        of = torch.zeros((22, ld), dtype=torch.float64, device=dev)

        def stats():
            if not L.anofox_hip_stats_device(y.data_ptr(), None, None, ld, lens.data_ptr(), n, rows, 0, 0, oi.data_ptr(), of.data_ptr(), None, C.byref(err)):
                raise RuntimeError(err.message.decode())

        med_s, lo_s = timed(stats, steps)
        lines.append(f"    stats_kernel (anofox_hip_stats_device), the same block, the same run : {med_s:10.3f} ({lo_s:10.3f})   features / stats = {med / med_s:.1f}")
        b = DeviceBatch(n, rows, lib.make_options("CrostonClassic", 28, auto_detect=False), dev)
        ln = lens.clone()
        ln[n:] = 0
        b.set_block(y[:rows].contiguous(), ln)
        b.run()
        torch.cuda.synchronize()
        cro = []
        for _ in range(steps):
            b.run()
            torch.cuda.synchronize()
            cro.append(b.stats()["total_device_ms"])
        b.close()
        lines.append(f"    croston_kernel (CrostonClassic, h = 28), the same block, device ms      : {float(np.median(cro)):10.3f} ({float(np.min(cro)):10.3f})")

    # the restatement on the 400-row slice: time, equality, deviations in units of the noise
    n_check = min(n_check, n)
    fpS, itS = got[T_SHORT]
    t0 = time.perf_counter()
    exp = [FC.expected([float(v) for v in Y[i][:T_SHORT]]) for i in range(n_check)]
    t_py = time.perf_counter() - t0
    unequal, worst = [], {}
    for i, e in enumerate(exp):
        for k, name in enumerate(names):
            g = float(fpS[k, i])
            if name not in e["features"]:
                if g == g:
                    unequal.append((i, name))
                continue
            w = e["features"][name]
            if e["tol"][name] == 0.0:
                if not R.same(g, w):
                    unequal.append((i, name))
            elif not R.same(g, w):
                grp = "ln" if name in R.LOG_FEATURES else "sin / cos"
                ratio = abs(g - w) / e["noise"][name]
                if ratio > worst.get(grp, (0.0, "-"))[0]:
                    worst[grp] = (ratio, name)
    lines.append(f"tests/features_ref.py (numpy counts and DFT) on {n_check} series x {T_SHORT} rows, noise measurements included, one process: {t_py * 1e3:9.1f} ms, "
                 f"i.e. {t_py / max(n_check, 1) * n:8.1f} s for the block")
    lines.append(f"    features under the equality contract that differ from the restatement on these series: {len(unequal)} {unequal[:5]}")
    for grp in ("ln", "sin / cos"):
        w = worst.get(grp, (0.0, "-"))
        lines.append(f"    worst |device - restatement| / measured noise, figures through {grp:9s}: {w[0]:6.2f} (tolerance 16; at {w[1]})")
    noise = {k: max(e["noise"].get(k, 0.0) for e in exp) for k in R.LOG_FEATURES + ("fft_coefficient_1_real", "spectral_centroid", "spectral_variance")}
    lines.append("    largest measured noise on these series: " + ", ".join(f"{k} {v:.2e}" for k, v in noise.items()))
    # the cases of the test suite (every family at every length up to 257, the four long cases): the same ratios
    from anofox_forecast_amd import device
    cases = [FC.series(f, m) for f, m in FC.short_cases() + FC.long_cases()]
    tc = max(len(s) for s in cases)
    ldc = (len(cases) + 63) // 64 * 64
    yc, vc = np.zeros((tc, ldc)), np.ones((tc, ldc), dtype=np.uint8)
    for i, s in enumerate(cases):
        yc[:len(s), i], vc[:len(s), i] = FC.split(s)
    lc = torch.tensor([len(s) for s in cases] + [0] * (ldc - len(cases)), dtype=torch.int32, device=dev)
    rc = device.features_block(torch.from_numpy(yc).to(dev), lc, torch.from_numpy(vc).to(dev), n_series=len(cases))
    fc = rc["features"].cpu().numpy()
    worst_c, n_tol, n_same, bad_c = {}, 0, 0, 0
    for i, s in enumerate(cases):
        e = FC.expected(s)
        for k, name in enumerate(names):
            if name not in e["features"] or e["status"] != 0:
                continue
            g, w = float(fc[k, i]), e["features"][name]
            if e["tol"][name] == 0.0:
                bad_c += not R.same(g, w)
                continue
            n_tol += 1
            if R.same(g, w):
                n_same += 1
            elif g == g and w == w:
                grp = "ln" if name in R.LOG_FEATURES else "sin / cos"
                ratio = abs(g - w) / e["noise"][name]
                if ratio > worst_c.get(grp, (0.0, "-", 0))[0]:
                    worst_c[grp] = (ratio, name, len(s))
    lines.append(f"The {len(cases)} series of tests/features_cases.py (ten families, lengths 1 .. 2,049) in one block: {bad_c} figures under the equality contract "
                 f"differ; of {n_tol:,d} figures under a tolerance {n_same:,d} equal the restatement bit for bit;")
    for grp in ("ln", "sin / cos"):
        w = worst_c.get(grp, (0.0, "-", 0))
        lines.append(f"    worst |device - restatement| / measured noise, figures through {grp:9s}: {w[0]:6.2f} (tolerance 16; {w[1]}, {w[2]} rows)")
    ru = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "resource_usage.py"), "features", "stats"], capture_output=True, text=True).stdout
    lines += ["", "Resources (tools/resource_usage.py features stats, gfx950; a features_*_kernel adds tile x 8 bytes of dynamic LDS per workgroup, the "
              "dft kernel twice that, at most 32 KiB):", ru.rstrip()]
    text = "\n".join(lines) + "\n"
    print(text)
    if out_path:
        open(out_path, "w").write(text)


if __name__ == "__main__":
    main()
