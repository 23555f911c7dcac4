"""Time the model-path chain on the M5 shape (30,490 series, m = 7, h = 28, 1,000 paths; the 6.8 GB block of profiles/paths_m5.txt):
the fit state left on the device (DeviceBatch.inspect_device), the innovations kernel, the simulation kernel for ANN, AAdA and MMdM as
uniform batches and for a real AutoETS mix, in both innovation modes, and paths_kernel on the same output block as the yardstick.

    python tools/time_ets_paths.py [--series 30490] [--length 1941] [--paths 1000] [--horizon 28] [--reps 5] > profiles/ets_paths_m5.txt

Every figure is the median of --reps runs after one warm-up, taken with device events around the enqueued work (three kernels per
simulation call: statuses, paths, n_broken).  The resource figures come from the compiler's remarks: tools/resource_usage.py."""
from __future__ import annotations

import argparse
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

TRENDS = ("N", "A", "Ad", "M", "Md")


def spec_id(notation):
    return "AM".index(notation[0]) * 15 + TRENDS.index(notation[1:-1]) * 3 + "NAM".index(notation[-1])


def uniform_records(n, ld, m, notation, T, rng):
    """Plausible fit state of one spec for n series: info [8, ld], states [2 + m, ld]."""
    e, t, s = notation[0], notation[1:-1], notation[-1]
    info, states = np.full((8, ld), np.nan), np.full((2 + m, ld), np.nan)
    alpha = rng.uniform(0.05, 0.4, n)
    info[0, :n], states[0, :n] = alpha, rng.uniform(80.0, 120.0, n)
    if t != "N":
        info[1, :n] = rng.uniform(0.0, 0.5, n) * alpha
        states[1, :n] = rng.uniform(-0.05, 0.05, n) if t in ("A", "Ad") else rng.uniform(0.999, 1.001, n)
    if s != "N":
        info[2, :n] = rng.uniform(0.0, 0.5, n) * (1.0 - alpha)
        states[2:, :n] = rng.uniform(-6.0, 6.0, (m, n)) if s == "A" else rng.uniform(0.9, 1.1, (m, n))
    if t in ("Ad", "Md"):
        info[3, :n] = rng.uniform(0.85, 0.98, n)
    sigma = rng.uniform(0.5, 1.5, n) if e == "A" else rng.uniform(0.01, 0.03, n)
    info[7, :n] = sigma * sigma * T
    return info, states


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

    print(f"# model paths on the M5 shape: {n} series (ld {ld}), T = {T}, m = {m}, h = {h}, {P} paths, block {gb:.2f} GB, {a.reps} runs")
    print(f"# device: {torch.cuda.get_device_name(0)}")
    out = torch.zeros((P * h, ld), dtype=torch.float64, device=dev)
    rng = np.random.default_rng(7)
    lengths = torch.full((ld,), T, dtype=torch.int32, device=dev)
    pool = torch.from_numpy(rng.standard_normal((T, ld)) * 0.02).to(dev)
    plen = torch.full((ld,), T, dtype=torch.int32, device=dev)

    # the yardstick: paths_kernel on the same output block (store-bound, profiles/paths_m5.txt)
    point = torch.from_numpy(rng.uniform(80.0, 120.0, (h, ld))).to(dev)
    for joint in (False, True):
        line(f"paths_kernel (yardstick) joint={int(joint)}",
             timed(lambda: device.paths_block(point, pool, pool_lengths=plen, n_paths=P, joint=joint, seed=1, n_series=n, out=out)), gb)

    def simulate(spec, info, states, what):
        for mode, joint in (("gaussian", False), ("bootstrap", False), ("bootstrap", True)):
            t = timed(lambda: device.ets_paths_block(spec=spec, info=info, states=states, lengths=lengths, m=m, horizon=h, n_paths=P,
                                                     innovations=mode, pool=pool if mode == "bootstrap" else None,
                                                     pool_lengths=plen if mode == "bootstrap" else None, joint=joint, seed=1, n_series=n, out=out))
            line(f"ets_paths {what} {mode}{' joint' if joint else ''}", t, gb)

    for notation in ("ANN", "AAdA", "MMdM"):
        info, states = uniform_records(n, ld, m, notation, T, rng)
        spec = torch.full((ld,), spec_id(notation), dtype=torch.int32, device=dev)
        simulate(spec, torch.from_numpy(info).to(dev), torch.from_numpy(states).to(dev), notation)

    # a real AutoETS mix: fit the synthetic M5 batch, keep the fit state on the device
    Y = synth.gen_series(synth.SEED_M5, 0, n, T, m, positive=True)
    y = torch.from_numpy(device.pack_time_major(Y)).to(dev)
    opts = lib.make_options("AutoETS", h, seasonal_period=m)
    b = device.DeviceBatch(n, T, opts, dev)
    b.set_block(y, lengths)
    b.run()
    torch.cuda.synchronize()
    line("inspect_device (info, states)", timed(lambda: b.inspect_device(fitted=False)))
    line("inspect_device (info, states, fitted)", timed(lambda: b.inspect_device(fitted=True)))
    d = b.inspect_device()
    line("ets_innovations_block", timed(lambda: device.ets_innovations_block(y, d["fitted"], lengths, d["spec"], n_series=n)), 3 * T * ld * 8 / 1e9)
    inn = device.ets_innovations_block(y, d["fitted"], lengths, d["spec"], n_series=n)
    pool, plen = inn["pool"], inn["pool_lengths"]
    counts = np.bincount(d["spec"].cpu().numpy().clip(min=0), minlength=30)
    print("# AutoETS mix (spec id: series): " + ", ".join(f"{k}: {c}" for k, c in enumerate(counts) if c))
    simulate(d["spec"], d["info"], d["states"], "AutoETS mix")
    g = device.ets_paths_block(b, n_paths=P, innovations="bootstrap", seed=1, out=out)
    torch.cuda.synchronize()
    print(f"# AutoETS mix, bootstrap of its own innovations: {int((g['status'] != 0).sum())} series without paths, "
          f"{int(g['n_broken'].sum())} broken paths of {n * P}")


if __name__ == "__main__":
    main()
