"""Device time of the dynamic Theta models (DynamicTheta, DynamicOptimizedTheta) on the synthetic M5 block (device-resident),
non-seasonal on the raw counts and at m = 7 on the counts shifted by +1 (strictly positive: the season test and the multiplicative
indices run): python tools/time_theta.py [n_series] [steps] [check_series]

Per (model, period): the median over `steps` runs of the batch's device time (anofox_hip_batch_stats total_device_ms), wall ms
per run and series/s; the first `check_series` series are compared with the numpy checker tests/theta_ref.py (a numpy
Nelder-Mead over the whole block would take hours).  One JSON line per case goes to stdout after the table."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import theta_ref  # noqa: E402
from anofox_forecast_amd import lib, synth  # noqa: E402
from anofox_forecast_amd.device import DeviceBatch, pack_time_major  # noqa: E402


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 30490
    steps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    n_check = int(sys.argv[3]) if len(sys.argv) > 3 else 64
    T, h = 1913, 28
    Y0 = synth.gen_series(synth.SEED_M5, 0, n, T, 7, positive=False)
    lines = []
    for period, shift in ((0, 0.0), (7, 1.0)):
        Y = Y0 + shift
        for model in theta_ref.MODELS:
            b = DeviceBatch(n, T, lib.make_options(model, h, seasonal_period=period, auto_detect=False), "cuda:0")
            y = torch.from_numpy(pack_time_major(Y, b.ld)).cuda()
            ln = torch.full((b.ld,), T, dtype=torch.int32, device="cuda")
            ln[n:] = 0
            b.set_block(y, ln)
            b.run()                      # warm-up
            torch.cuda.synchronize()
            dev, wall = [], []
            for _ in range(steps):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                b.run()
                torch.cuda.synchronize()
                wall.append((time.perf_counter() - t0) * 1e3)
                dev.append(b.stats()["total_device_ms"])
            got = b.results()["yhat"].cpu().numpy().reshape(n, -1)[:n_check].copy()
            b.close()
            ref = theta_ref.forecast(list(Y[:n_check]), model, h, period=period)[0]
            d_ms = float(np.median(dev))
            rec = {"model": model, "period": period, "n_series": n, "t": T, "h": h, "steps": steps,
                   "device_ms_median": round(d_ms, 3), "device_ms_min": round(float(np.min(dev)), 3),
                   "wall_ms_median": round(float(np.median(wall)), 3), "series_per_s": round(n / d_ms * 1e3),
                   "checked_series": n_check, "bit_equal_to_checker": bool(np.array_equal(got, ref))}
            lines.append(rec)
            print(f"{model:22s} m={period:<2d} device {d_ms:9.3f} ms/step (min {rec['device_ms_min']:9.3f})  wall "
                  f"{rec['wall_ms_median']:9.3f} ms  {rec['series_per_s']:>12,d} series/s  first {n_check} equal to the checker: "
                  f"{rec['bit_equal_to_checker']}", flush=True)
    for rec in lines:
        print(json.dumps(rec))


if __name__ == "__main__":
    main()
