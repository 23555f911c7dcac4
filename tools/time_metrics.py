"""Device time of the accuracy metric entry (anofox_hip_metrics_device) on two device-resident shapes, with a numpy restatement
of the same figures on the same blocks beside it:  python tools/time_metrics.py [n_series] [steps] [--out FILE]

(a) the n_series x 1,913 time-major M5-shape block, `actual` and `forecast`, the seven two-input figures in ONE call (and the six
    without R^2, whose second sweep re-reads `actual`): ms per step and algorithmic TB/s -- 2 x 8TN bytes, plus 8TN when R^2
    re-reads; bytes the algorithm reads, not measured HBM traffic -- beside the 0.80 TB/s of croston_kernel for one sweep of the
    same block, the project's yardstick for a one-lane-per-series sweep.
(b) the series-major results of an n_series x 5 folds x 28 steps backtest: actual, yhat, a baseline, lower, upper and three quantile
    forecasts, all twelve figures, once through the LDS tiles and once with direct strided reads (ANOFOX_HIP_TUNE
    metrics_staging=0): what the staging buys.

A step is one call, which returns after its stream has finished: launch and wait included.  The numpy lines are one process on
the host (np.add.reduce along the time axis adds row by row, so its sums associate as the kernel's do)."""
import ctypes as C
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from anofox_forecast_amd import lib  # noqa: E402

FIG = lib.METRIC_FIGURES
TWO = ("mae", "mse", "rmse", "mape", "smape", "r2", "bias")
EPS = np.finfo(np.float64).eps


def mask(figs):
    return sum(1 << FIG.index(f) for f in figs)


def numpy_two_input(a, f, axis):
    """The seven two-input figures, vectorised over the groups (rows along `axis`)."""
    n = a.shape[axis]
    e = a - f
    out = {"mae": np.add.reduce(np.abs(e), axis=axis) / n, "mse": np.add.reduce(e * e, axis=axis) / n, "bias": np.add.reduce(f - a, axis=axis) / n}
    out["rmse"] = np.sqrt(out["mse"])
    keep = np.abs(a) > EPS
    with np.errstate(all="ignore"):
        cnt = np.add.reduce(keep, axis=axis)
        out["mape"] = np.add.reduce(np.where(keep, np.abs(e / a), 0.0), axis=axis) / cnt * 100.0
        den = np.abs(a) + np.abs(f)
        keep = den > EPS
        cnt = np.add.reduce(keep, axis=axis)
        out["smape"] = np.add.reduce(np.where(keep, 2.0 * np.abs(e) / den, 0.0), axis=axis) / cnt * 100.0
        mean = np.add.reduce(a, axis=axis) / n
        d = a - np.expand_dims(mean, axis)
        tot = np.add.reduce(d * d, axis=axis)
        out["r2"] = np.where(np.abs(tot) < EPS, np.nan, 1.0 - np.add.reduce(e * e, axis=axis) / tot)
    return out


def call(L, ptrs, quant, stride_q, levels, strides, lens, n, T, figs, quantile, fig, ld, status):
    err = lib.AnofoxError()
    lv = None if levels is None else levels.ctypes.data
    ok = L.anofox_hip_metrics_device(*ptrs, quant, stride_q, lv, 0 if levels is None else len(levels), strides[0], strides[1], lens.data_ptr(), n, T,
                                     mask(figs), quantile, False, fig.data_ptr(), ld, status.data_ptr(), None, C.byref(err))
    assert ok, err.message


def timed(fn, steps):
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(steps):
        t0 = time.perf_counter()
        fn()
        ms.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ms)), float(np.min(ms))


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    n = int(args[0]) if args else 30490
    steps = int(args[1]) if len(args) > 1 else 10
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
    L = lib.load()
    dev = "cuda:0"
    rng = np.random.default_rng(7)
    lines = [f"Accuracy metric entry (anofox_hip_metrics_device) on one {torch.cuda.get_device_name(0)}, device-resident, {steps} steps, median (min):"]

    # (a) time-major M5-shape block
    T, ld = 1913, (n + 63) // 64 * 64
    a = np.zeros((T, ld)); f = np.zeros((T, ld))
    a[:, :n] = np.round(rng.poisson(1.5, (T, n)).astype(np.float64), 1)
    f[:, :n] = np.round(a[:, :n] + rng.normal(0, 1, (T, n)), 1)
    ta, tf = torch.from_numpy(a).to(dev), torch.from_numpy(f).to(dev)
    lens = torch.full((n,), T, dtype=torch.int32, device=dev)
    fig = torch.zeros((len(FIG), ld), dtype=torch.float64, device=dev)
    status = torch.zeros((n,), dtype=torch.int32, device=dev)
    ptrs = (ta.data_ptr(), tf.data_ptr(), None, None, None)
    for figs, sweeps in ((TWO, 3), (tuple(x for x in TWO if x != "r2"), 2)):
        med, lo = timed(lambda: call(L, ptrs, None, 0, None, (1, ld), lens, n, T, figs, 0.5, fig, ld, status), steps)
        tb = sweeps * 8.0 * T * n / (med * 1e-3) / 1e12
        lines.append(f"(a) {n:,d} x {T:,d} time-major, {len(figs)} figures{' (R^2 re-reads actual)' if sweeps == 3 else ' (no R^2)':24s}: "
                     f"{med:8.3f} ms/step ({lo:8.3f})  {tb:5.2f} TB/s algorithmic ({sweeps} x 8TN bytes; croston_kernel: 0.80 TB/s for one sweep)")
    call(L, ptrs, None, 0, None, (1, ld), lens, n, T, TWO, 0.5, fig, ld, status)
    got = fig.cpu().numpy()
    t0 = time.perf_counter()
    ref = numpy_two_input(a[:, :n], f[:, :n], 0)
    t_np = time.perf_counter() - t0
    same = {k: bool(np.array_equal(got[FIG.index(k), :n], ref[k], equal_nan=True)) for k in TWO}
    lines.append(f"    numpy restatement of the seven figures on the same block, one process: {t_np * 1e3:9.1f} ms; equal to the device figures: {same}")
    waves = (n + 63) // 64
    lines.append(f"    {waves} one-wave workgroups for 1,024 SIMDs: the step is bound by the length of one wave's instruction stream over its "
                 f"{T:,d} rows (as config 2, DESIGN.md section 8.3), not by bandwidth; the sums stay sequential by contract.")
    del ta, tf, a, f

    # (b) series-major results of a backtest
    g, h = n * 5, 28
    ldg = (g + 63) // 64 * 64
    act = np.round(rng.poisson(1.5, (g, h)).astype(np.float64), 1)
    blocks = [act, np.round(act + rng.normal(0, 1, (g, h)), 1), np.round(act + rng.normal(0, 1.5, (g, h)), 1)]
    blocks += [blocks[1] - 1.5, blocks[1] + 1.5]
    quant = np.stack([blocks[1] + z for z in (-1.3, 0.0, 1.3)])
    levels = np.array([0.1, 0.5, 0.9])
    tb_ = [torch.from_numpy(np.ascontiguousarray(b)).to(dev) for b in blocks]
    tq = torch.from_numpy(quant).to(dev)
    lens = torch.full((g,), h, dtype=torch.int32, device=dev)
    fig = torch.zeros((len(FIG), ldg), dtype=torch.float64, device=dev)
    status = torch.zeros((g,), dtype=torch.int32, device=dev)
    ptrs = tuple(t.data_ptr() for t in tb_)
    run = lambda: call(L, ptrs, tq.data_ptr(), g * h, levels, (h, 1), lens, g, h, FIG, 0.9, fig, ldg, status)
    res = {}
    for name, knob in (("LDS staging", None), ("direct strided reads", "metrics_staging=0")):
        if knob:
            os.environ["ANOFOX_HIP_TUNE"] = knob
        med, lo = timed(run, steps)
        res[name] = fig.cpu().numpy().copy()
        os.environ.pop("ANOFOX_HIP_TUNE", None)
        nbytes = (8 + 1) * 8.0 * g * h                              # eight blocks, and actual once more for R^2
        lines.append(f"(b) {g:,d} groups x {h} rows series-major, all 12 figures, 8 blocks, {name:21s}: {med:8.3f} ms/step ({lo:8.3f})  "
                     f"{nbytes / (med * 1e-3) / 1e12:5.2f} TB/s algorithmic")
    lines.append(f"    both paths give the same bits: {bool(np.array_equal(res['LDS staging'].view(np.uint64), res['direct strided reads'].view(np.uint64)))}")
    t0 = time.perf_counter()
    numpy_two_input(blocks[0], blocks[1], 1)
    lines.append(f"    numpy restatement of the seven two-input figures alone on these blocks, one process: {(time.perf_counter() - t0) * 1e3:9.1f} ms")
    ru = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "resource_usage.py"), "metrics"], capture_output=True, text=True).stdout
    lines += ["", "Resources (tools/resource_usage.py metrics, gfx950; the staged kernels add 64 x (TR + 1) x 8 bytes of dynamic LDS per block):", ru.rstrip()]
    text = "\n".join(lines) + "\n"
    print(text)
    if out_path:
        open(out_path, "w").write(text)


if __name__ == "__main__":
    main()
