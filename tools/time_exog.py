"""Device time of the ARIMAX path on the synthetic M5 block (device-resident, 30,490 x 1,913, h = 28) for K = 1, 3 and 8
regressors: python tools/time_exog.py [n_series] [steps] [check_series] [K ...]

Per K: one warm-up run, then `steps` runs timed with the batch's HIP events (total_device_ms: the whole run on its stream -- output
seeding, the mean / sd sweeps of the intervals, exog_arimax_kernel, interval_kernel); the median, series/s, and for orientation the
algorithmic bytes of the ARIMAX kernel, 3 sweeps x (K + 1) x 8 T N, over that time, beside the same ratio of croston_kernel
(profiles/intermittent_m5.txt: one sweep of the same block in 0.58 ms).  The first `check_series` series are compared with the
numpy checker tests/exog_ref.py bit for bit.  One JSON line per K goes to stdout after the table."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import exog_ref  # noqa: E402
from anofox_forecast_amd import lib, synth  # noqa: E402
from anofox_forecast_amd.device import DeviceBatch, pack_time_major  # noqa: E402

CROSTON_MS = 0.58          # profiles/intermittent_m5.txt: croston_kernel, one sweep of the 30,490 x 1,913 block


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 30490
    steps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    n_check = int(sys.argv[3]) if len(sys.argv) > 3 else 16
    ks = [int(a) for a in sys.argv[4:]] or [1, 3, 8]
    T, h = 1913, 28
    ld = (n + 63) // 64 * 64
    croston_gbs = 8.0 * T * 30490 / (CROSTON_MS * 1e-3) / 1e9
    lines = []
    for K in ks:
        XF = synth.gen_regressors(synth.SEED_EXOG, 0, n, T, h, K)
        Y = synth.gen_exog_target(synth.SEED_EXOG, 0, n, XF[:, :, :T])
        y = torch.from_numpy(pack_time_major(Y, ld)).cuda()
        ln = torch.full((ld,), T, dtype=torch.int32, device="cuda")
        ln[n:] = 0
        x = torch.zeros((K, T, ld), dtype=torch.float64, device="cuda")
        f = torch.zeros((K, h, ld), dtype=torch.float64, device="cuda")
        for j in range(K):
            x[j, :, :n] = torch.from_numpy(np.ascontiguousarray(XF[:, j, :T].T)).cuda()
            f[j, :, :n] = torch.from_numpy(np.ascontiguousarray(XF[:, j, T:].T)).cuda()
        b = DeviceBatch(n, T, lib.make_options("ARIMA", h, confidence_level=0.95, auto_detect=False), "cuda:0")
        b.set_block(y, ln)
        b.set_exog(x, f)
        b.run()                              # warm-up
        torch.cuda.synchronize()
        dev = []
        for _ in range(steps):
            b.run()
            torch.cuda.synchronize()
            dev.append(b.stats()["total_device_ms"])
        got = b.results()["yhat"].cpu().numpy().reshape(n, -1)[:n_check].copy()
        b.close()
        ref = exog_ref.fit_batch(list(Y[:n_check]), [list(XF[s, :, :T]) for s in range(n_check)], [list(XF[s, :, T:]) for s in range(n_check)])
        ok = bool(np.array_equal(got, ref["point"]))
        ms = float(np.median(dev))
        alg = 3.0 * (K + 1) * 8.0 * T * n
        rec = {"case": "ARIMAX", "k": K, "n_series": n, "t": T, "h": h, "steps": steps, "device_ms_median": round(ms, 3),
               "device_ms_min": round(float(np.min(dev)), 3), "series_per_s": round(n / ms * 1e3), "algorithmic_gb": round(alg / 1e9, 3),
               "algorithmic_gb_per_s": round(alg / (ms * 1e-3) / 1e9, 1), "croston_gb_per_s": round(croston_gbs, 1),
               "checked_series": n_check, "bit_equal_to_checker": ok}
        lines.append(rec)
        print(f"ARIMAX K={K}  device {ms:9.3f} ms/step (min {rec['device_ms_min']:9.3f})  {rec['series_per_s']:>12,d} series/s  "
              f"{rec['algorithmic_gb']:7.3f} GB algorithmic = {rec['algorithmic_gb_per_s']:8.1f} GB/s (croston_kernel: {croston_gbs:.1f} GB/s)  "
              f"first {n_check} equal to the checker: {ok}", flush=True)
        del x, f, y, b
        torch.cuda.empty_cache()
    for rec in lines:
        print(json.dumps(rec))


if __name__ == "__main__":
    main()
