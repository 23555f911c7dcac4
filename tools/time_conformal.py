"""Device time of the three conformal kernels (anofox_hip_conformal_learn_device / _apply_device / _evaluate_device) on
device-resident blocks, with a numpy restatement on the same block beside them:
    python tools/time_conformal.py [n_groups] [steps] [--out FILE]

Two calibration shapes, three levels (alpha 0.2, 0.1, 0.05), h = 28 forecasts per group:
(a) n_groups x 140 residuals -- a 5-fold x 28-step backtest: the 256-key LDS tile, 16 waves per workgroup;
(b) n_groups x 1,913 residuals -- the M5 length: the 2,048-key tile, 4 waves per workgroup.
Both time-major; (a) also series-major.  Learn is timed for the symmetric and the asymmetric method, with and without the sorted
output; apply for the symmetric and the adaptive method; evaluate on the bounds apply wrote.

A step is one call, which returns after its stream has finished: launch and wait included.  One warm-up call, then `steps`
calls; median and minimum.  The numpy line is np.sort of |r| along the time axis plus the two-point interpolation, one process
on the host.  The figure to put beside (b) is stats_kernel on the same 1,913-row block (tools/time_stats.py, profiles/stats_m5.txt):
it sorts the same rows and does more besides."""
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

ALPHAS = np.array([0.2, 0.1, 0.05])


def timed(fn, steps):
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(steps):
        t0 = time.perf_counter()
        fn()
        ms.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ms)), float(np.min(ms))


def numpy_scores(r, alphas):
    """Symmetric scores of every column of the time-major block r [T x n]."""
    s = np.sort(np.abs(r), axis=0)
    n = s.shape[0]
    out = []
    for a in alphas:
        q = min(max(np.ceil((n + 1.0) * (1.0 - a)) / n, 0.0), 1.0)
        if q <= 0.0:
            out.append(s[0])
        elif q >= 1.0:
            out.append(s[-1])
        else:
            idx = q * (n - 1)
            lo = int(np.floor(idx))
            up = min(lo + 1, n - 1)
            frac = idx - lo
            out.append(s[lo] * (1.0 - frac) + s[up] * frac)
    return np.stack(out)


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    n = int(args[0]) if args else 30490
    steps = int(args[1]) if len(args) > 1 else 10
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
    L = lib.load()
    dev = "cuda:0"
    rng = np.random.default_rng(11)
    ld = (n + 63) // 64 * 64
    h, K = 28, len(ALPHAS)
    lines = [f"Conformal kernels on one {torch.cuda.get_device_name(0)}, device-resident, {n:,d} groups, {K} levels, h = {h}, {steps} steps, "
             f"median (min) ms per step:"]
    err = lib.AnofoxError()
    sl = torch.zeros((K, ld), dtype=torch.float64, device=dev)
    su = torch.zeros((K, ld), dtype=torch.float64, device=dev)
    kept = torch.zeros((n,), dtype=torch.int32, device=dev)
    status = torch.zeros((n,), dtype=torch.int32, device=dev)

    def learn(res, strides, lens, T, method, srt):
        ok = L.anofox_hip_conformal_learn_device(res.data_ptr(), None, None, None, strides[0], strides[1], lens.data_ptr(), n, T, ALPHAS.ctypes.data,
                                                 K, method, sl.data_ptr(), su.data_ptr(), ld, None if srt is None else srt.data_ptr(),
                                                 kept.data_ptr(), status.data_ptr(), None, C.byref(err))
        assert ok, err.message

    for tag, T in (("(a)", 140), ("(b)", 1913)):
        r = np.zeros((T, ld))
        r[:, :n] = np.round(rng.normal(0.0, 2.0, (T, n)), 1)
        tr = torch.from_numpy(r).to(dev)
        lens = torch.full((n,), T, dtype=torch.int32, device=dev)
        srt = torch.zeros_like(tr)
        tile = 64
        while tile < 2048 and tile < T:
            tile *= 2
        waves = min(16, 65536 // (tile * 8))
        lines.append(f"{tag} {n:,d} x {T:,d} residuals, tile {tile} keys = {tile * 8 // 1024} KiB per wave, {waves} waves per workgroup")
        for name, method, s in (("symmetric", 0, None), ("symmetric + sorted output", 0, srt), ("asymmetric", 1, None), ("asymmetric + sorted output", 1, srt)):
            med, lo = timed(lambda: learn(tr, (1, ld), lens, T, method, s), steps)
            lines.append(f"    learn, time-major, {name:27s}: {med:8.3f} ({lo:8.3f})   {8.0 * T * n / (med * 1e-3) / 1e12:5.2f} TB/s of residuals read")
        learn(tr, (1, ld), lens, T, 0, None)
        got = sl.cpu().numpy()[:, :n]
        t0 = time.perf_counter()
        ref = numpy_scores(r[:, :n], ALPHAS)
        t_np = (time.perf_counter() - t0) * 1e3
        lines.append(f"    numpy restatement (np.sort of |r| + interpolation) on the same block, one process: {t_np:9.1f} ms; "
                     f"equal to the device scores: {bool(np.array_equal(got, ref))}")
        if T == 140:
            rs = torch.from_numpy(np.ascontiguousarray(r[:, :n].T)).to(dev)
            for name, method in (("symmetric", 0), ("asymmetric", 1)):
                med, lo = timed(lambda: learn(rs, (T, 1), lens, T, method, None), steps)
                lines.append(f"    learn, series-major, {name:25s}: {med:8.3f} ({lo:8.3f})")
            learn(rs, (T, 1), lens, T, 0, None)
            lines.append(f"    series-major and time-major scores equal: {bool(np.array_equal(sl.cpu().numpy()[:, :n], got))}")
            del rs
        del tr, srt

    # apply and evaluate around an [n x h] series-major point block (the layout of the forecast results); scores from shape (b)
    f = np.round(rng.normal(20.0, 5.0, (n, h)), 1)
    tf = torch.from_numpy(f).to(dev)
    td = torch.from_numpy(rng.uniform(0.5, 2.0, (n, h))).to(dev)
    ta = torch.from_numpy(np.round(f + rng.normal(0.0, 2.0, (n, h)), 1)).to(dev)
    lo_b = torch.zeros((K, n, h), dtype=torch.float64, device=dev)
    up_b = torch.zeros((K, n, h), dtype=torch.float64, device=dev)
    hl = torch.full((n,), h, dtype=torch.int32, device=dev)
    fig = torch.zeros((5, ld), dtype=torch.float64, device=dev)

    def apply(method):
        ok = L.anofox_hip_conformal_apply_device(tf.data_ptr(), td.data_ptr(), h, 1, hl.data_ptr(), n, h, sl.data_ptr(), su.data_ptr(), ld, K, method,
                                                 lo_b.data_ptr(), up_b.data_ptr(), n * h, status.data_ptr(), None, C.byref(err))
        assert ok, err.message

    def evaluate():
        ok = L.anofox_hip_conformal_evaluate_device(ta.data_ptr(), lo_b[1].data_ptr(), up_b[1].data_ptr(), h, 1, hl.data_ptr(), n, h, 0.1,
                                                    fig.data_ptr(), ld, status.data_ptr(), None, C.byref(err))
        assert ok, err.message

    lines.append(f"apply and evaluate, {n:,d} x {h} series-major point block, {K} levels")
    for name, method in (("symmetric", 0), ("adaptive", 2)):
        med, lo = timed(lambda: apply(method), steps)
        lines.append(f"    apply, {name:10s}: {med:8.3f} ({lo:8.3f})   {(1 + 2 * K) * 8.0 * n * h / (med * 1e-3) / 1e12:5.2f} TB/s read + written")
    apply(0)
    med, lo = timed(evaluate, steps)
    lines.append(f"    evaluate         : {med:8.3f} ({lo:8.3f})")
    t0 = time.perf_counter()
    s1 = sl.cpu().numpy()[1, :n, None]
    lo_np, up_np = f - s1, f + s1
    a_np = ta.cpu().numpy()
    cov = ((a_np >= lo_np) & (a_np <= up_np)).sum(axis=1) / h
    t_np = (time.perf_counter() - t0) * 1e3
    lines.append(f"    numpy restatement of one level's bounds and coverage, one process: {t_np:9.1f} ms; equal: "
                 f"{bool(np.array_equal(lo_b[1].cpu().numpy(), lo_np) and np.array_equal(fig[0, :n].cpu().numpy(), cov))}")
    ru = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "resource_usage.py"), "conformal"], capture_output=True, text=True).stdout
    lines += ["", "Resources (tools/resource_usage.py conformal, gfx950; conformal_kernel adds waves x tile x 8 bytes of dynamic LDS per workgroup, "
              "at most 64 KiB):", ru.rstrip()]
    text = "\n".join(lines) + "\n"
    print(text)
    if out_path:
        open(out_path, "w").write(text)


if __name__ == "__main__":
    main()
