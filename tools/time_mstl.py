"""Device time of the MSTL decomposition entry and of SeasonalWindowAverage on the synthetic M5 block (device-resident, 30,490 x
1,913 raw counts, h = 28): python tools/time_mstl.py [n_series] [steps] [check_series]

Per case: the median over `steps` runs (wall time of the decomposition entry, which returns after its stream has finished; the
batch's device time for SeasonalWindowAverage), and series/s; the first `check_series` series are compared with the numpy checker
tests/mstl_ref.py.  MSTL forecasts stay an error, so the decomposition is timed for [7] and [7, 365].  One JSON
line per case goes to stdout after the table."""
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import mstl_ref  # noqa: E402
from anofox_forecast_amd import lib, synth  # noqa: E402
from anofox_forecast_amd.device import DeviceBatch, pack_time_major  # noqa: E402


def _same(a, b):
    return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 30490
    steps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    n_check = int(sys.argv[3]) if len(sys.argv) > 3 else 16
    T, h = 1913, 28
    Y = synth.gen_series(synth.SEED_M5, 0, n, T, 7, positive=False)
    L = lib.load()
    lines = []
    ld = (n + 63) // 64 * 64
    y = torch.from_numpy(pack_time_major(Y, ld)).cuda()
    ln = torch.full((ld,), T, dtype=torch.int32, device="cuda")
    ln[n:] = 0
    for periods in ([7], [7, 365]):
        K = len(periods)
        tr = torch.empty((T, ld), dtype=torch.float64, device="cuda")
        rm = torch.empty_like(tr)
        se = torch.empty((K, T, ld), dtype=torch.float64, device="cuda")
        info = torch.empty(ld, dtype=torch.int32, device="cuda")
        per = (C.c_int * K)(*periods)
        err = lib.AnofoxError()

        def run():
            if not L.anofox_hip_mstl_decompose_device(y.data_ptr(), ld, ln.data_ptr(), n, T, per, K, 0, tr.data_ptr(), se.data_ptr(),
                                                      rm.data_ptr(), info.data_ptr(), None, C.byref(err)):
                raise RuntimeError(err.message.decode())
        torch.cuda.synchronize()
        run()                            # warm-up
        wall = []
        for _ in range(steps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run()
            wall.append((time.perf_counter() - t0) * 1e3)
        trn, rmn, sen = tr.cpu().numpy(), rm.cpu().numpy(), se.cpu().numpy()
        ok = True
        for i in range(n_check):
            d = mstl_ref.mstl_decompose(Y[i], periods)
            ok &= _same(trn[:, i], d["trend"]) and _same(rmn[:, i], d["remainder"])
            ok &= all(_same(sen[k, :, i], d["seasonal"][k]) for k in range(K))
        ms = float(np.median(wall))
        rec = {"case": "decomposition", "periods": periods, "n_series": n, "t": T, "steps": steps, "ms_median": round(ms, 3),
               "ms_min": round(float(np.min(wall)), 3), "series_per_s": round(n / ms * 1e3), "checked_series": n_check,
               "bit_equal_to_checker": bool(ok)}
        lines.append(rec)
        print(f"decomposition {str(periods):10s} {ms:9.3f} ms/step (min {rec['ms_min']:9.3f})  {rec['series_per_s']:>12,d} series/s  "
              f"first {n_check} equal to the checker: {ok}", flush=True)
        del tr, rm, se
    b = DeviceBatch(n, T, lib.make_options("SeasonalWindowAverage", h, seasonal_period=7, auto_detect=False), "cuda:0")
    b.set_block(y, ln)
    b.run()
    torch.cuda.synchronize()
    dev = []
    for _ in range(steps):
        b.run()
        torch.cuda.synchronize()
        dev.append(b.stats()["total_device_ms"])
    got = b.results()["yhat"].cpu().numpy().reshape(n, -1)[:n_check].copy()
    b.close()
    ok = all(_same(got[i], mstl_ref.swa_forecast(Y[i], 7, h)) for i in range(n_check))
    ms = float(np.median(dev))
    rec = {"case": "SeasonalWindowAverage", "period": 7, "n_series": n, "t": T, "h": h, "steps": steps, "device_ms_median": round(ms, 3),
           "device_ms_min": round(float(np.min(dev)), 3), "series_per_s": round(n / ms * 1e3), "checked_series": n_check,
           "bit_equal_to_checker": bool(ok)}
    lines.append(rec)
    print(f"SeasonalWindowAverage m=7  device {ms:9.3f} ms/step (min {rec['device_ms_min']:9.3f})  {rec['series_per_s']:>12,d} "
          f"series/s  first {n_check} equal to the checker: {ok}", flush=True)
    for rec in lines:
        print(json.dumps(rec))


if __name__ == "__main__":
    main()
