"""Device time of the backtest on a resident block (device.backtest_block: expand -> one batch run -> collect -> fold scores):
    python tools/time_backtest.py [n_series] [steps] [--folds F] [--models Naive,SES,AutoETS] [--out FILE]

The block is the synthetic M5 shape, n_series x 1,913 daily counts, time-major; horizon 28, F = 5 folds, expanding window (the fold
table of api.backtest_fold_bounds).  Per model:
  * expand, collect (without scores), the fold scores (collect with scores minus collect without) and the whole call, each a call
    that returns after its stream has finished: one warm-up, then `steps` calls, median (min) ms;
  * the ONE expanded batch (n_series * F columns) against F runs of a DeviceBatch on the source block itself -- no copy: fold f's
    batch takes the row slice [train_start_f, train_end_f] of the block (a pointer offset) and the lengths of that fold -- device ms
    of the runs (anofox_hip_batch_stats), the F runs one after the other.
The expand kernel's algorithmic bytes per second (values written + window values read) stand beside croston_kernel's on the source
block in the same run (8 bytes x rows x series over its device time)."""
import ctypes as C
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

T_M5, H = 1913, 28


def timed(fn, steps):
    import torch
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(steps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ms)), float(np.min(ms))


def main():
    import torch

    from anofox_forecast_amd import api, lib, synth
    from anofox_forecast_amd.device import DeviceBatch, backtest_block, pack_time_major
    argv = sys.argv[1:]
    opt = lambda k, d: argv[argv.index(k) + 1] if k in argv else d
    out_path = opt("--out", None)
    n_folds = int(opt("--folds", "5"))
    models = opt("--models", "Naive,SES,AutoETS").split(",")
    pos, skip = [], False
    for a in argv:
        if skip:
            skip = False
        elif a in ("--out", "--folds", "--models"):
            skip = True
        else:
            pos.append(a)
    n = int(pos[0]) if pos else 30490
    steps = int(pos[1]) if len(pos) > 1 else 5
    L = lib.load()
    dev = torch.device("cuda:0")
    Y = synth.gen_series(synth.SEED_M5, 0, n, T_M5, 7, positive=False)
    ld = (n + 63) // 64 * 64
    y = torch.from_numpy(pack_time_major(Y, ld)).to(dev)
    lens = torch.zeros(ld, dtype=torch.int32, device=dev)
    lens[:n] = T_M5
    folds = api.backtest_fold_bounds(T_M5, H, n_folds)
    F = len(folds)
    tab = lib.make_folds(folds)
    t_train, n_pairs, ld_pairs = lib.backtest_sizes(tab, F, n)
    err = lib.AnofoxError()
    lines = [f"device.backtest_block on one {torch.cuda.get_device_name(0)}, device-resident, {n:,d} series x {T_M5:,d} rows (synthetic M5 counts), "
             f"horizon {H}, {F} folds, expanding window: {n_pairs:,d} pairs, expanded block {t_train:,d} x {ld_pairs:,d} = "
             f"{t_train * ld_pairs * 8 / 1e9:.2f} GB; {steps} steps, median (min) ms",
             f"(python tools/time_backtest.py {n} {steps} --folds {n_folds} --models {','.join(models)})"]

    # expand alone, and croston_kernel on the source block in the same run
    train = torch.empty((t_train, ld_pairs), dtype=torch.float64, device=dev)
    len_pairs = torch.empty(ld_pairs, dtype=torch.int32, device=dev)
    n_test = torch.empty(ld_pairs, dtype=torch.int32, device=dev)

    def expand():
        if not L.anofox_hip_backtest_expand_device(y.data_ptr(), ld, lens.data_ptr(), n, T_M5, tab, F, t_train, train.data_ptr(), ld_pairs,
                                                   len_pairs.data_ptr(), n_test.data_ptr(), None, C.byref(err)):
            raise RuntimeError(err.message.decode())

    e_med, e_min = timed(expand, steps)
    written = t_train * ld_pairs * 8
    read = sum(f[2] - f[1] + 1 for f in folds) * n * 8
    lines.append(f"    expand                             : {e_med:9.3f} ({e_min:9.3f})   {(written + read) / (e_med * 1e-3) / 1e12:5.2f} TB/s algorithmic "
                 f"({written / 1e9:.2f} GB written + {read / 1e9:.2f} GB of window values read)")
    cb = DeviceBatch(n, T_M5, lib.make_options("CrostonClassic", H, auto_detect=False), dev)
    cb.set_block(y, lens)
    cb.run()
    torch.cuda.synchronize()
    c_ms = []
    for _ in range(steps):
        cb.run()
        torch.cuda.synchronize()
        c_ms.append(cb.stats()["total_device_ms"])
    cb.close()
    c_med = float(np.median(c_ms))
    lines.append(f"    CrostonClassic run on the source block, the same run: {c_med:9.3f} ms device   {8.0 * T_M5 * n / (c_med * 1e-3) / 1e12:5.2f} TB/s of values read")
    del train

    for model in models:
        opts = lib.make_options(model, H, confidence_level=0.0, auto_detect=False)
        keep = {}

        def whole():
            keep["r"] = backtest_block(y, lens, opts, folds, n_series=n, metric="rmse")

        m_steps = steps if model != "AutoETS" else max(2, steps // 2)
        w_med, w_min = timed(whole, m_steps)
        r = keep["r"]
        b = r["batch"]
        run_ms = []
        for _ in range(m_steps):
            b.run()
            torch.cuda.synchronize()
            run_ms.append(b.stats()["total_device_ms"])
        actual = torch.empty((n_pairs, H), dtype=torch.float64, device=dev)
        error, abs_error = torch.empty_like(actual), torch.empty_like(actual)
        n_rows = torch.zeros(n_pairs, dtype=torch.int32, device=dev)
        scores = torch.zeros(F, dtype=torch.float64, device=dev)

        def collect(with_scores):
            if not L.anofox_hip_backtest_collect_device(y.data_ptr(), ld, n, T_M5, tab, F, r["n_test"].data_ptr(), r["status"].data_ptr(),
                                                        r["yhat"].data_ptr(), r["lower"].data_ptr(), r["upper"].data_ptr(), H, b"rmse",
                                                        actual.data_ptr(), error.data_ptr(), abs_error.data_ptr(), None, n_rows.data_ptr(),
                                                        scores.data_ptr() if with_scores else None, None, C.byref(err)):
                raise RuntimeError(err.message.decode())

        c0_med, c0_min = timed(lambda: collect(False), steps)
        c1_med, c1_min = timed(lambda: collect(True), steps)
        ok_pairs = int((r["status"] == 0).sum().item())
        rows = int(r["n_rows"].sum().item())
        lines.append(f"{model}: {ok_pairs:,d} of {n_pairs:,d} pairs forecast, {rows:,d} test rows, fold rmse {[round(float(v), 4) for v in r['scores'].cpu().numpy()]}")
        lines.append(f"    whole call                         : {w_med:9.3f} ({w_min:9.3f})")
        lines.append(f"    collect (no scores)                : {c0_med:9.3f} ({c0_min:9.3f})")
        lines.append(f"    fold scores ({F} waves, in row order) : {c1_med - c0_med:9.3f}   (collect with scores {c1_med:9.3f} ({c1_min:9.3f}))")
        one = float(np.median(run_ms))
        lines.append(f"    ONE expanded batch, device ms      : {one:9.3f}   (+ expand {e_med:.3f} = {one + e_med:.3f})")
        del keep["r"], r
        b.close()
        per_fold = []
        for (_, tr0, tr1, _, _) in folds:
            fb = DeviceBatch(n, tr1 - tr0 + 1, opts, dev)
            fl = torch.zeros(ld, dtype=torch.int32, device=dev)
            fl[:n] = tr1 - tr0 + 1
            fb.set_block(y[tr0:tr1 + 1], fl)
            fb.run()
            torch.cuda.synchronize()
            ms = []
            for _ in range(m_steps):
                fb.run()
                torch.cuda.synchronize()
                ms.append(fb.stats()["total_device_ms"])
            per_fold.append(float(np.median(ms)))
            fb.close()
        lines.append(f"    {F} runs on row slices of the source : {sum(per_fold):9.3f}   ({', '.join(f'{v:.3f}' for v in per_fold)});  "
                     f"expanded / separate = {(one + e_med) / sum(per_fold):.2f}")
        print("\n".join(lines[-6:]), flush=True)
    text = "\n".join(lines) + "\n"
    print(text)
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
