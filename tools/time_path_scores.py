"""Device time of the path scores (device.path_scores_block, device.path_energy_block) beside the quantile kernel they share a sort with:
    python tools/time_path_scores.py [n_series] [steps] [--paths P] [--out FILE]

The block is that of tools/time_paths.py: joint cumulative paths around a [n_series x 28] point block, pools of 1,913 centred synthetic
M5 counts, P = 1,000 paths, the nine levels of M5's uncertainty track; the actuals are the points plus one draw of the pool.  Every
figure is the time between two stream events around calls that only enqueue: one warm-up, then `steps` calls, median (min) ms.
  * path_quantiles_kernel and the scores entry on the same block in the same run, leaves and M5's twelve groupings (42,840 columns):
    every output, without the quantile output, without levels, the per-column block alone;
  * the energy pass over the leaves (the actuals series-major as a backtest has them, and time-major) and over the whole aggregate,
    with its algorithmic rate (the block read once) beside backtest_expand_kernel's store rate in the same run;
  * the torch route for the same figures: sort + the sorted-form CRPS and the ranks, vector_norm over the columns for the energy score.
    It has another order of addition, so its time is comparable and its bits are not."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

T_M5, H, PERIOD = 1913, 28, 7
LEVELS = (0.005, 0.025, 0.165, 0.25, 0.5, 0.75, 0.835, 0.975, 0.995)


def main():
    import torch

    from anofox_forecast_amd import api, device, synth
    argv = sys.argv[1:]
    opt = lambda k, d: argv[argv.index(k) + 1] if k in argv else d
    out_path = opt("--out", None)
    P = int(opt("--paths", "1000"))
    pos, skip = [], False
    for a in argv:
        if skip:
            skip = False
        elif a in ("--out", "--paths"):
            skip = True
        else:
            pos.append(a)
    n = int(pos[0]) if pos else 30490
    steps = int(pos[1]) if len(pos) > 1 else 5
    dev = torch.device("cuda:0")
    Y = synth.gen_series(synth.SEED_M5, 0, n, T_M5, PERIOD, positive=False)
    ld = (n + 63) // 64 * 64
    y = torch.from_numpy(device.pack_time_major(Y, ld)).to(dev)
    lens = torch.zeros(ld, dtype=torch.int32, device=dev)
    lens[:n] = T_M5
    pool = (y - y.mean(0, keepdim=True)).contiguous()
    point = y[-1, :n].view(n, 1).expand(n, H).contiguous()
    actual = (point + pool[100:100 + H, :n].t()).contiguous()          # [n x 28] series-major
    rows = P * H

    def timed(fn, k=steps):
        fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(k):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1))
        return float(np.median(ms)), float(np.min(ms))

    fmt = lambda t: f"{t[0]:9.3f} ({t[1]:9.3f})"
    lines = [f"device.path_scores_block / path_energy_block on one {torch.cuda.get_device_name(0)}, device-resident, {n:,d} leaves, horizon {H}, "
             f"{P:,d} paths, {len(LEVELS)} levels; {steps} steps, median (min) ms between stream events",
             f"(python tools/time_path_scores.py {n} {steps} --paths {P})"]

    def say(text):
        lines.append(text)
        print(text, flush=True)

    block = device.paths_block(point, pool, n_paths=P, mode="cumulative", joint=True, seed=1, series_major=True, n_series=n)["paths"]
    folds = api.backtest_fold_bounds(T_M5, H, 5)
    t = timed(lambda: device.backtest_expand_block(y, lens, folds, n_series=n))
    ex = device.backtest_expand_block(y, lens, folds, n_series=n)
    say(f"  backtest_expand_kernel, the same run ({ex['t_train']:,d} x {ex['ld_pairs']:,d})            : {fmt(t)}   "
        f"{ex['t_train'] * ex['ld_pairs'] * 8 / (t[0] * 1e-3) / 1e12:5.2f} TB/s of stores")
    del ex

    def score_block(name, paths, act, cols, sm):
        k = max(2, steps // 2)
        tq = timed(lambda: device.path_quantiles_block(paths, LEVELS, horizon=H, n_paths=P, n_cols=cols), k)
        say(f"  {name}: path_quantiles_kernel, {cols:,d} columns                       : {fmt(tq)}")
        for label, lv, want in (("every output", LEVELS, device.PATH_SCORES_WANT), ("without the quantile output", LEVELS, ("crps", "ranks", "column")),
                                ("the per-column block alone", LEVELS, ("column",)), ("no levels: crps, ranks, crps_mean", (), ("crps", "ranks", "column"))):
            t = timed(lambda: device.path_scores_block(paths, act, lv, horizon=H, n_paths=P, n_cols=cols, actual_series_major=sm, want=want), k)
            say(f"  {name}: scores entry, {label:36s}: {fmt(t)}   {t[0] / tq[0]:5.2f} x the quantile kernel")
        t = timed(lambda: device.path_energy_block(paths, act, horizon=H, n_paths=P, col_begin=0, col_end=cols, actual_series_major=sm), k)
        say(f"  {name}: energy score of all {cols:,d} columns                         : {fmt(t)}   "
            f"{rows * cols * 8 / (t[0] * 1e-3) / 1e12:5.2f} TB/s of the block read once")

    score_block("leaves", block, actual, n, True)
    leaf_tm = torch.zeros((H, ld), dtype=torch.float64, device=dev)
    leaf_tm[:, :n] = actual.t()
    t = timed(lambda: device.path_energy_block(block, leaf_tm, horizon=H, n_paths=P, col_begin=0, col_end=n), max(2, steps // 2))
    say(f"  leaves: energy score of all {n:,d} columns, the actuals time-major          : {fmt(t)}   "
        f"{rows * n * 8 / (t[0] * 1e-3) / 1e12:5.2f} TB/s of the block read once")

    # ---- M5's twelve groupings ----
    s = np.arange(n)
    per_store = -(-n // 10)
    store = s // per_store
    state = store * 3 // 10
    item = s % per_store
    dept = item * 7 // per_store
    cat = np.array([0, 0, 1, 1, 2, 2, 2])[dept]
    out, base = [], 0
    for key in [np.zeros(n, dtype=np.int64), state, store, cat, dept, state * 3 + cat, state * 7 + dept, store * 3 + cat, store * 7 + dept, item,
                item * 3 + state, s]:
        _, inv = np.unique(key, return_inverse=True)
        out.append(base + inv)
        base += int(inv.max()) + 1
    plan = device.hierarchy_plan_device(torch.from_numpy(np.array(out, dtype=np.int32)).to(dev))
    n_out = plan["n_out"]
    full = torch.full((ld,), rows, dtype=torch.int32, device=dev)
    agg = device.aggregate_block(block, full, plan, n_series=n, t_out=rows)["y"]
    act_tm = torch.zeros((H, ld), dtype=torch.float64, device=dev)
    act_tm[:, :n] = actual.t()
    act_agg = device.aggregate_block(act_tm, torch.full((ld,), H, dtype=torch.int32, device=dev), plan, n_series=n, t_out=H)["y"]
    ranges = {"the 3,049 items": (int(out[9].min()), int(out[9].max()) + 1), "the 10 stores": (int(out[2].min()), int(out[2].max()) + 1)}
    score_block("twelve groupings", agg, act_agg, n_out, False)
    for name, (cb, ce) in ranges.items():
        t = timed(lambda: device.path_energy_block(agg, act_agg, horizon=H, n_paths=P, col_begin=cb, col_end=ce), max(2, steps // 2))
        say(f"  twelve groupings: energy score of {name} [{cb:,d}, {ce:,d})               : {fmt(t)}")
    del agg

    # ---- the torch route ----
    cube = block.view(P, H, ld)[:, :, :n]
    yk = actual.t().unsqueeze(0)                                        # [1, H, n]
    w = (2.0 * torch.arange(P, dtype=torch.float64, device=dev) - P + 1).view(P, 1, 1)
    lv = torch.tensor(LEVELS, dtype=torch.float64, device=dev)

    def torch_scores():
        srt = torch.sort(cube, dim=0).values
        d = srt - yk
        crps = d.abs().mean(0) - (w * d).sum(0) / (P * P)
        below, equal = (cube < yk).sum(0), (cube == yk).sum(0)
        idx = lv * (P - 1)
        lo = idx.floor().long()
        up = torch.clamp(lo + 1, max=P - 1)
        frac = (idx - lo).view(-1, 1, 1)
        q = srt[lo] * (1.0 - frac) + srt[up] * frac
        e = yk - q
        pin = torch.where(e >= 0, lv.view(-1, 1, 1) * e, (lv.view(-1, 1, 1) - 1.0) * e).mean(1)
        return crps, below, equal, q, pin

    def torch_energy():
        d1 = torch.linalg.vector_norm(cube - yk, dim=2)
        d2 = torch.linalg.vector_norm(cube[:-1] - cube[1:], dim=2)
        return d1.mean(0) - d2.sum(0) / (2.0 * (P - 1))

    t = timed(torch_scores, 2)
    say(f"  torch sort + sorted-form CRPS, ranks, quantiles, pinball, the leaves                     : {fmt(t)}")
    t = timed(torch_energy, 2)
    say(f"  torch vector_norm over the columns, the leaves                                           : {fmt(t)}   "
        f"{rows * n * 8 / (t[0] * 1e-3) / 1e12:5.2f} TB/s of the block read once")
    text = "\n".join(lines) + "\n"
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
