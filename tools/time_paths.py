"""Device time of the bootstrap sample paths and their quantiles (device.paths_block, device.path_quantiles_block, api.paths_batch):
    python tools/time_paths.py [n_series] [steps] [--paths P] [--out FILE]

The block is the synthetic M5 shape, n_series x 1,913 daily counts, time-major; the pool of a series is its 1,913 centred values, the
point block a [n_series x 28] series-major block as a batch's results are; horizon 28, P = 1,000 paths, the nine levels of M5's
uncertainty track.  Every figure is the time between two stream events around calls that only enqueue: one warm-up, then `steps`
calls, median (min) ms.
  * generate: cumulative paths, independent and joint, with the store rate of paths_kernel beside backtest_expand_kernel's in the same run;
  * aggregate: the path block added up the M5 prefix plan and M5's twelve groupings (device.aggregate_block);
  * quantiles of the leaf block and of the aggregated blocks, with the time per key;
  * the whole batch call on host buffers (api.paths_batch), leaves only and with the twelve groupings: pack, upload, the chain, download;
  * the torch route for the same work: torch.randint + gather + cumsum, index_add_ per level, torch.sort + two-point interpolation.
    It has other random numbers and another order of addition, so its time is comparable and its bits are not."""
import os
import sys
import time

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
    pool = (y - y.mean(0, keepdim=True)).contiguous()                  # [1,913 x ld] time-major: the centred values as residuals
    point = y[-1, :n].view(n, 1).expand(n, H).contiguous()             # [n x 28] series-major, as a batch's yhat
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
    lines = [f"device.paths_block / path_quantiles_block on one {torch.cuda.get_device_name(0)}, device-resident, {n:,d} series, pools of {T_M5:,d} "
             f"rows (synthetic M5 counts, centred), horizon {H}, {P:,d} paths, {len(LEVELS)} levels; {steps} steps, median (min) ms between stream events",
             f"(python tools/time_paths.py {n} {steps} --paths {P})"]

    # ---- generate ----
    block = torch.zeros((rows, ld), dtype=torch.float64, device=dev)
    stored = rows * n * 8
    for joint in (False, True):
        t = timed(lambda: device.paths_block(point, pool, n_paths=P, mode="cumulative", joint=joint, seed=1, series_major=True, n_series=n, out=block))
        lines.append(f"  generate, cumulative, {'joint      ' if joint else 'independent'} [{rows:,d} x {ld:,d}] : {fmt(t)}   {stored / (t[0] * 1e-3) / 1e12:5.2f} TB/s of stores")
        print(lines[-1], flush=True)
    t = timed(lambda: device.paths_block(point, pool, n_paths=P, mode="independent", joint=False, seed=1, series_major=True, n_series=n, out=block))
    lines.append(f"  generate, independent mode, independent draws            : {fmt(t)}   {stored / (t[0] * 1e-3) / 1e12:5.2f} TB/s of stores")
    folds = api.backtest_fold_bounds(T_M5, H, 5)
    t = timed(lambda: device.backtest_expand_block(y, lens, folds, n_series=n))
    ex = device.backtest_expand_block(y, lens, folds, n_series=n)
    lines.append(f"  backtest_expand_kernel, the same run ({ex['t_train']:,d} x {ex['ld_pairs']:,d})     : {fmt(t)}   "
                 f"{ex['t_train'] * ex['ld_pairs'] * 8 / (t[0] * 1e-3) / 1e12:5.2f} TB/s of stores")
    del ex
    print(lines[-1], flush=True)
    device.paths_block(point, pool, n_paths=P, mode="cumulative", joint=True, seed=1, series_major=True, n_series=n, out=block)

    # ---- aggregate ----
    s = np.arange(n)
    per_store = -(-n // 10)
    store = s // per_store
    state = store * 3 // 10
    item = s % per_store
    dept = item * 7 // per_store
    cat = np.array([0, 0, 1, 1, 2, 2, 2])[dept]

    def number(levels):
        out, base = [], 0
        for key in levels:
            _, inv = np.unique(key, return_inverse=True)
            out.append(base + inv)
            base += int(inv.max()) + 1
        return np.array(out, dtype=np.int32)

    zero = np.zeros(n, dtype=np.int64)
    plans = {"M5 prefix plan (total, state, store, leaf)": number([zero, state, store, s]),
             "M5's twelve groupings": number([zero, state, store, cat, dept, state * 3 + cat, state * 7 + dept, store * 3 + cat, store * 7 + dept,
                                              item, item * 3 + state, s])}
    full = torch.full((ld,), rows, dtype=torch.int32, device=dev)

    def per_key(t, cols):
        return f"{t[0] * 1e6 / (cols * H * P):7.3f} ns per key"

    t = timed(lambda: device.path_quantiles_block(block, LEVELS, horizon=H, n_paths=P, n_cols=n))
    lines.append(f"  quantiles of the leaves ({n:,d} columns x {H} steps x {P:,d} keys)    : {fmt(t)}   {per_key(t, n)}")
    print(lines[-1], flush=True)
    twelve = None
    for name, column_of in plans.items():
        plan = device.hierarchy_plan_device(torch.from_numpy(column_of).to(dev))
        n_out = plan["n_out"]
        ld_out = (n_out + 63) // 64 * 64
        out = {"y": torch.zeros((rows, ld_out), dtype=torch.float64, device=dev), "present": torch.zeros((rows, ld_out), dtype=torch.uint8, device=dev)}
        t = timed(lambda: device.aggregate_block(block, full, plan, n_series=n, t_out=rows, out=out), max(2, steps // 2))
        lines.append(f"  aggregate, {name}: {n_out:,d} columns : {fmt(t)}")
        print(lines[-1], flush=True)
        t = timed(lambda: device.path_quantiles_block(out["y"], LEVELS, horizon=H, n_paths=P, n_cols=n_out), max(2, steps // 2))
        lines.append(f"  quantiles of its {n_out:,d} columns                                   : {fmt(t)}   {per_key(t, n_out)}")
        print(lines[-1], flush=True)
        twelve = column_of
        del out
    lines.append("  (conformal learn, profiles/conformal_m5.txt: 2.07 ms for 30,490 groups of 1,913 keys in tiles of 2,048 = 0.033 ns per padded key)")

    # ---- the whole batch call on host buffers ----
    pts_h, pools_h = point.cpu().numpy(), [np.ascontiguousarray(c) for c in pool[:, :n].t().cpu().numpy()]
    for label, co in (("leaves only", None), ("the twelve groupings", twelve)):
        ms = []
        for _ in range(2):
            t0 = time.perf_counter()
            res, err = api.paths_batch(pts_h, pools_h, LEVELS, n_paths=P, mode="cumulative", joint=True, seed=1, column_of=co)
            ms.append((time.perf_counter() - t0) * 1e3)
            assert err["ok"], err
        lines.append(f"  api.paths_batch on host buffers, {label:20s}: {min(ms):9.1f} ms wall (second of two calls; pack, upload, chain, download)")
        print(lines[-1], flush=True)
    del pools_h

    # ---- the torch route ----
    pool_n = pool[:, :n].contiguous()

    def torch_generate(joint):
        if joint:
            j = torch.randint(0, T_M5, (P, H, 1), device=dev).expand(P, H, n)
        else:
            j = torch.randint(0, T_M5, (P, H, n), device=dev)
        e = torch.gather(pool_n.unsqueeze(0).expand(P, T_M5, n), 1, j)
        return torch.cumsum(e, 1) + point.t().unsqueeze(0)

    for joint in (False, True):
        t = timed(lambda: torch_generate(joint), max(2, steps // 2))
        lines.append(f"  torch randint + gather + cumsum, {'joint      ' if joint else 'independent'}                 : {fmt(t)}")
        print(lines[-1], flush=True)
    tp = torch_generate(True)                                           # [P, H, n]

    def torch_aggregate(column_of):
        n_out = int(column_of.max()) + 1
        agg = torch.zeros((P, H, n_out), dtype=torch.float64, device=dev)
        for g in range(column_of.shape[0]):
            agg.index_add_(2, torch.from_numpy(column_of[g]).to(dev).long(), tp)
        return agg

    t = timed(lambda: torch_aggregate(twelve), 2)
    lines.append(f"  torch index_add_ per level, the twelve groupings                      : {fmt(t)}")
    print(lines[-1], flush=True)
    lv = torch.tensor(LEVELS, dtype=torch.float64, device=dev)

    def torch_quantiles(x):
        srt = torch.sort(x, dim=0).values
        idx = lv * (P - 1)
        lo = idx.floor().long()
        up = torch.clamp(lo + 1, max=P - 1)
        frac = (idx - lo).view(-1, 1, 1)
        return srt[lo] * (1.0 - frac) + srt[up] * frac

    t = timed(lambda: torch_quantiles(tp), max(2, steps // 2))
    lines.append(f"  torch sort + two-point interpolation, the leaves                      : {fmt(t)}   {per_key(t, n)}")
    text = "\n".join(lines) + "\n"
    print(text)
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
