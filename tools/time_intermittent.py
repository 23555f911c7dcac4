"""Device time of the intermittent-demand models (CrostonClassic, CrostonSBA, TSB, ADIDA, IMAPA) on the synthetic M5 block
(raw counts, device-resident), with the numpy checker's time on the same block beside it (the CPU reference of the tests, NOT
a product path): python tools/time_intermittent.py [n_series] [steps] [checker_workers]

Per model: the median over `steps` runs of the batch's device time (anofox_hip_batch_stats total_device_ms: first to last kernel
of the run, IMAPA's one host wait included), wall ms per run, series/s, and the checker's wall time on `checker_workers` processes.
One JSON line per model goes to stdout after the table."""
import json
import multiprocessing as mp
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from anofox_forecast_amd import lib, synth  # noqa: E402
from anofox_forecast_amd.device import DeviceBatch, pack_time_major  # noqa: E402

MODELS = ("CrostonClassic", "CrostonSBA", "TSB", "ADIDA", "IMAPA")


def _checker(args):
    Y, model = args
    import intermittent_ref
    return intermittent_ref.point_forecasts(list(Y), model)


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 30490
    steps = int(sys.argv[2]) if len(sys.argv) > 2 else 10
    workers = int(sys.argv[3]) if len(sys.argv) > 3 else 15
    T, h = 1913, 28
    Y = synth.gen_series(synth.SEED_M5, 0, n, T, 7, positive=False)
    chunks = [Y[a:a + 1024] for a in range(0, n, 1024)]
    lines = []
    with mp.get_context("spawn").Pool(workers) as pool:
        for model in MODELS:
            b = DeviceBatch(n, T, lib.make_options(model, h, auto_detect=False), "cuda:0")
            y = torch.from_numpy(pack_time_major(Y, b.ld)).cuda()
            ln = torch.full((b.ld,), T, dtype=torch.int32, device="cuda")
            ln[n:] = 0
            b.set_block(y, ln)
            b.run()                      # warm-up (IMAPA allocates its level buffer here)
            torch.cuda.synchronize()
            dev, wall = [], []
            for _ in range(steps):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                b.run()
                torch.cuda.synchronize()
                wall.append((time.perf_counter() - t0) * 1e3)
                dev.append(b.stats()["total_device_ms"])
            got = b.results()["yhat"][:, 0].cpu().numpy().copy()
            b.close()
            t0 = time.perf_counter()
            ref = np.concatenate(pool.map(_checker, [(c, model) for c in chunks]))
            t_ref = time.perf_counter() - t0
            d_ms = float(np.median(dev))
            rec = {"model": model, "n_series": n, "t": T, "h": h, "steps": steps, "device_ms_median": round(d_ms, 4),
                   "device_ms_min": round(float(np.min(dev)), 4), "wall_ms_median": round(float(np.median(wall)), 4),
                   "series_per_s": round(n / d_ms * 1e3), "checker_s": round(t_ref, 2), "checker_workers": workers,
                   "bit_equal_to_checker": bool(np.array_equal(got, ref))}
            lines.append(rec)
            print(f"{model:15s} device {d_ms:8.3f} ms/step (min {rec['device_ms_min']:8.3f})  wall {rec['wall_ms_median']:8.3f} ms  "
                  f"{rec['series_per_s']:>12,d} series/s   [numpy checker, CPU, {workers} procs: {t_ref:7.2f} s]  "
                  f"equal: {rec['bit_equal_to_checker']}", flush=True)
    for rec in lines:
        print(json.dumps(rec))


if __name__ == "__main__":
    main()
