"""Time the ARIMA model-path chain on the M5 shape (30,490 series, m = 7, h = 28, 1,000 paths; the 6.8 GB block of
profiles/paths_m5.txt): the simulation kernel for ARIMA(1,1,1) alone and for a real AutoARIMA mix, Gaussian and joint bootstrap (and
the bootstrap of a series' own rows), beside paths_kernel and ets_paths_kernel (ANN) writing the same output block in the same run;
the innovations pass and the fit-state copy separately.

    python tools/time_arima_paths.py [--series 30490] [--length 1941] [--paths 1000] [--horizon 28] [--reps 5] > profiles/arima_paths_m5.txt

Every figure is the median of --reps runs after one warm-up, taken with device events around the enqueued work (three kernels per
simulation call: statuses, paths, n_broken).  The resource figures come from the compiler's remarks:
python tools/resource_usage.py arima_paths."""
from __future__ import annotations

import argparse
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--series", type=int, default=30490)
    ap.add_argument("--length", type=int, default=1941)
    ap.add_argument("--paths", type=int, default=1000)
    ap.add_argument("--horizon", type=int, default=28)
    ap.add_argument("--period", type=int, default=7)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    import torch
    from anofox_forecast_amd import device, lib, synth
    dev = torch.device("cuda:0")
    n, T, P, h, m = a.series, a.length, a.paths, a.horizon, a.period
    ld = (n + 63) // 64 * 64
    gb = P * h * ld * 8 / 1e9

    def timed(fn):
        fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1))
        return statistics.median(ms), min(ms)

    def line(what, t, bytes_gb=None):
        rate = f"  {bytes_gb / (t[0] * 1e-3) / 1e3:6.2f} TB/s of the {bytes_gb:.2f} GB block" if bytes_gb else ""
        print(f"{what:<58s} median {t[0]:9.3f} ms   min {t[1]:9.3f} ms{rate}", flush=True)

    print(f"# ARIMA model paths on the M5 shape: {n} series (ld {ld}), T = {T}, m = {m}, h = {h}, {P} paths, block {gb:.2f} GB, {a.reps} runs")
    print(f"# device: {torch.cuda.get_device_name(0)}")
    out = torch.zeros((P * h, ld), dtype=torch.float64, device=dev)
    rng = np.random.default_rng(7)
    lengths = torch.full((ld,), T, dtype=torch.int32, device=dev)
    pool = torch.from_numpy(rng.standard_normal((T, ld)) * 0.02).to(dev)
    plen = torch.full((ld,), T, dtype=torch.int32, device=dev)

    # the yardsticks on the same output block: paths_kernel and ets_paths_kernel (ANN)
    point = torch.from_numpy(rng.uniform(80.0, 120.0, (h, ld))).to(dev)
    for joint in (False, True):
        line(f"paths_kernel (yardstick) joint={int(joint)}",
             timed(lambda: device.paths_block(point, pool, pool_lengths=plen, n_paths=P, joint=joint, seed=1, n_series=n, out=out)), gb)
    info, states = np.full((8, ld), np.nan), np.full((2 + m, ld), np.nan)
    info[0, :n], states[0, :n], info[7, :n] = rng.uniform(0.05, 0.4, n), rng.uniform(80.0, 120.0, n), T
    spec = torch.zeros(ld, dtype=torch.int32, device=dev)
    info, states = torch.from_numpy(info).to(dev), torch.from_numpy(states).to(dev)
    for mode, joint in (("gaussian", False), ("bootstrap", True)):
        line(f"ets_paths ANN (yardstick) {mode}{' joint' if joint else ''}",
             timed(lambda: device.ets_paths_block(spec=spec, info=info, states=states, lengths=lengths, m=m, horizon=h, n_paths=P, innovations=mode,
                                                  pool=pool if joint else None, pool_lengths=plen if joint else None, joint=joint, seed=1,
                                                  n_series=n, out=out)), gb)

    Y = synth.gen_series(synth.SEED_M5, 0, n, T, m, positive=True)
    y = torch.from_numpy(device.pack_time_major(Y)).to(dev)

    def simulate(orders, coef, inn, what):
        for mode, joint in (("gaussian", False), ("bootstrap", False), ("bootstrap", True)):
            rows = int(inn["resid_lengths"][inn["resid_lengths"] > 0].min().item()) if joint else 0
            t = timed(lambda: device.arima_paths_block(orders=orders, coef=coef, y=y, lengths=lengths, resid=inn["resid"],
                                                       resid_lengths=inn["resid_lengths"], sigma=inn["sigma"], m=m, horizon=h, n_paths=P,
                                                       innovations=mode, joint=joint, pool_rows=rows, seed=1, n_series=n, out=out))
            line(f"arima_paths {what} {mode}{' joint' if joint else ''}", t, gb)

    # ARIMA(1,1,1) alone: hand-set fits on the same series
    orders, coef = np.zeros((8, ld), dtype=np.int32), np.zeros((16, ld))
    orders[0, :n], orders[1, :n], orders[2, :n], orders[7, :n] = 1, 1, 1, T - 1
    coef[0, :n], coef[5, :n] = rng.uniform(0.2, 0.7, n), rng.uniform(0.1, 0.6, n)
    orders, coef = torch.from_numpy(orders).to(dev), torch.from_numpy(coef).to(dev)
    # (the innovations entry is timed on preallocated outputs: the kernel alone, without the allocation and NaN fill of the mirror)
    inn = device.arima_innovations_block(orders, coef, y, lengths, m, n_series=n)
    line("arima_innovations_block ARIMA(1,1,1)", timed(lambda: device.arima_innovations_block(orders, coef, y, lengths, m, n_series=n, out=inn)),
         2 * T * ld * 8 / 1e9)
    simulate(orders, coef, inn, "ARIMA(1,1,1)")

    # a real AutoARIMA mix: fit the synthetic M5 batch, keep the fit on the device
    b = device.DeviceBatch(n, T, lib.make_options("AutoARIMA", h, seasonal_period=m), dev)
    b.set_block(y, lengths)
    b.run()
    torch.cuda.synchronize()
    line("arima_fit_device (orders, coef)", timed(lambda: b.arima_fit_device()))
    d = b.arima_fit_device()
    inn = device.arima_innovations_block(d["orders"], d["coef"], y, lengths, m, n_series=n)
    line("arima_innovations_block AutoARIMA mix",
         timed(lambda: device.arima_innovations_block(d["orders"], d["coef"], y, lengths, m, n_series=n, out=inn)), 2 * T * ld * 8 / 1e9)
    o = d["orders"][:, :n].cpu().numpy()
    names, counts = np.unique(["(%d,%d,%d)(%d,%d,%d)" % tuple(o[:6, s]) for s in range(n)], return_counts=True)
    top = np.argsort(-counts)[:12]
    print("# AutoARIMA mix (orders: series): " + ", ".join(f"{names[k]}: {counts[k]}" for k in top) + f"; {len(names)} order sets in all")
    simulate(d["orders"], d["coef"], inn, "AutoARIMA mix")
    g = device.arima_paths_block(b, n_paths=P, innovations="bootstrap", seed=1, out=out)
    torch.cuda.synchronize()
    print(f"# AutoARIMA mix, bootstrap of its own residuals: {int((g['status'] != 0).sum())} series without paths, "
          f"{int(g['n_broken'].sum())} broken paths of {n * P}")


if __name__ == "__main__":
    main()
