"""Device time of the choice of a method per series (device.select_block and the entries beneath it):
    python tools/time_select.py [n_series] [steps] [--folds F] [--models Naive,SeasonalNaive,SES,CrostonSBA,AutoETS] [--out FILE]

The block is the synthetic M5 shape, n_series x 1,913 daily counts, time-major; horizon 28, period 7, F = 5 expanding folds.  Every
figure is the time between two stream events around calls that return after their stream has finished: one warm-up, then `steps`
calls, median (min) ms.
  * the breakdown: the shared expand, each method's backtest run + collect on it, the scoring per series, winner + partition, the
    gathers, the sub-batch runs, the scatters, the pick of the backtest blocks, and the whole select_block call;
  * the routes, alternating within every step of the same run: select_block; (a) the route without these entries -- M x
    backtest_block, each with its own expand, then torch.argmin / index_select / index_copy_ as the glue, then the same sub-batches;
    (b) every method refitted on the whole block and the winners' rows indexed;
  * the glue kernels against torch's equivalent ops on the same resident tensors;
  * algorithmic bytes per second of gather and scatter beside backtest_expand_kernel's and croston_kernel's in the same run."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

T_M5, H, PERIOD = 1913, 28, 7
SEASONAL = ("SeasonalNaive", "HoltWinters", "SeasonalES", "AutoETS")


def main():
    import torch

    from anofox_forecast_amd import api, device, lib, synth
    argv = sys.argv[1:]
    opt = lambda k, d: argv[argv.index(k) + 1] if k in argv else d
    out_path = opt("--out", None)
    n_folds = int(opt("--folds", "5"))
    models = opt("--models", "Naive,SeasonalNaive,SES,CrostonSBA,AutoETS").split(",")
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
    dev = torch.device("cuda:0")
    M = len(models)
    Y = synth.gen_series(synth.SEED_M5, 0, n, T_M5, PERIOD, positive=False)
    ld = (n + 63) // 64 * 64
    y = torch.from_numpy(device.pack_time_major(Y, ld)).to(dev)
    lens = torch.zeros(ld, dtype=torch.int32, device=dev)
    lens[:n] = T_M5
    folds = api.backtest_fold_bounds(T_M5, H, n_folds)
    F = len(folds)
    methods = [lib.make_options(m, H, seasonal_period=PERIOD if m in SEASONAL else 0, auto_detect=False) for m in models]

    def events(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1), out

    def timed(fn, k=steps):
        events(fn)
        ms = [events(fn)[0] for _ in range(k)]
        return float(np.median(ms)), float(np.min(ms))

    fmt = lambda t: f"{t[0]:9.3f} ({t[1]:9.3f})"
    lines = [f"device.select_block on one {torch.cuda.get_device_name(0)}, device-resident, {n:,d} series x {T_M5:,d} rows (synthetic M5 counts), "
             f"horizon {H}, period {PERIOD}, {F} expanding folds, methods {', '.join(models)}; {steps} steps, median (min) ms between stream events",
             f"(python tools/time_select.py {n} {steps} --folds {n_folds} --models {','.join(models)})"]

    # ---- the breakdown ----
    t_expand = timed(lambda: device.backtest_expand_block(y, lens, folds, n_series=n))
    expanded = device.backtest_expand_block(y, lens, folds, n_series=n)
    t_train, n_pairs, ld_pairs = expanded["t_train"], expanded["n_pairs"], expanded["ld_pairs"]
    written = t_train * ld_pairs * 8
    read = sum(f[2] - f[1] + 1 for f in folds) * n * 8
    lines.append(f"  shared expand ({t_train:,d} x {ld_pairs:,d})            : {fmt(t_expand)}   {(written + read) / (t_expand[0] * 1e-3) / 1e12:5.2f} TB/s algorithmic")
    backtests, scores = [], torch.full((M, ld), float("nan"), dtype=torch.float64, device=dev)
    score_status = torch.ones((M, n), dtype=torch.int32, device=dev)
    for m, o in enumerate(methods):
        k = steps if models[m] != "AutoETS" else max(2, steps // 2)
        t_bt = timed(lambda: device.backtest_block(y, lens, o, folds, n_series=n, expanded=expanded), k)
        bt = device.backtest_block(y, lens, o, folds, n_series=n, expanded=expanded)
        a, f = bt["actual"].view(n, F * H), bt["yhat"].view(n, F * H)
        t_sc = timed(lambda: device.score_block(a, f, "rmse"))
        sc, ss = device.score_block(a, f, "rmse")
        scores[m, :n] = sc[:n]
        score_status[m] = ss
        backtests.append(bt)
        lines.append(f"  {models[m]:14s} backtest run + collect : {fmt(t_bt)}   score per series {fmt(t_sc)}")
        print(lines[-1], flush=True)
    t_win = timed(lambda: device.select_winner_block(scores, score_status, 0, n_series=n))
    chosen = device.select_winner_block(scores, score_status, 0, n_series=n)
    winner, members = chosen["winner"], chosen["members"]
    offsets = chosen["offsets"].cpu().numpy()

    def torch_winner():
        masked = torch.where((score_status == 0) & ~torch.isnan(scores[:, :n]), scores[:, :n], torch.full_like(scores[:, :n], float("inf")))
        w = torch.argmin(masked, dim=0)                              # (torch does not promise the lowest index among equal scores)
        order = torch.sort(w, stable=True).indices
        offs = torch.cumsum(torch.bincount(w, minlength=M), 0)
        return w, order, offs

    t_twin = timed(torch_winner)
    lines.append(f"  winner + partition                        : {fmt(t_win)}   torch where / argmin / stable sort / bincount / cumsum {fmt(t_twin)}")
    wins = [int(offsets[m + 1] - offsets[m]) for m in range(M)]
    lines.append(f"  wins per method: {dict(zip(models, wins))}")

    def gathers():
        return [device.select_gather_block(y, lens, members, int(offsets[m]), wins[m], n_series=n) for m in range(M) if wins[m]]

    def torch_gathers():
        out = []
        for m in range(M):
            if wins[m]:
                blk = torch.zeros((T_M5, (wins[m] + 63) // 64 * 64), dtype=torch.float64, device=dev)
                blk[:, :wins[m]] = torch.index_select(y, 1, members[int(offsets[m]):int(offsets[m + 1])].long())
                out.append(blk)
        return out

    t_g, t_tg = timed(gathers), timed(torch_gathers)
    moved = 2 * 8 * T_M5 * sum(wins)
    lines.append(f"  gather, all methods                       : {fmt(t_g)}   {moved / (t_g[0] * 1e-3) / 1e12:5.2f} TB/s algorithmic (read + written)   "
                 f"torch zeros / index_select / copy {fmt(t_tg)}")
    blocks = gathers()
    subs, k = [], 0
    for m in range(M):
        if wins[m]:
            b = device.DeviceBatch(wins[m], T_M5, methods[m], dev)
            b.set_block(blocks[k]["y"], blocks[k]["lengths"])
            subs.append((m, b))
            k += 1
    t_runs = timed(lambda: [b.run() for _, b in subs], max(2, steps // 2))
    lines.append(f"  sub-batch runs, winners only              : {fmt(t_runs)}")
    final = {k2: torch.empty((n, H), dtype=torch.float64, device=dev) for k2 in ("yhat", "lower", "upper")}
    final.update({"model_code": torch.zeros(n, dtype=torch.int32, device=dev), "status": torch.zeros(n, dtype=torch.int32, device=dev)})

    def scatters():
        for m, b in subs:
            device.select_scatter_block(b.results(), members, int(offsets[m]), wins[m], final)

    def torch_scatters():
        for m, b in subs:
            r = b.results()
            idx = members[int(offsets[m]):int(offsets[m + 1])].long()
            for k2 in ("yhat", "lower", "upper", "model_code", "status"):
                final[k2].index_copy_(0, idx, r[k2][:wins[m]])

    t_s, t_ts = timed(scatters), timed(torch_scatters)
    moved = sum(wins) * (2 * 3 * 8 * H + 2 * 2 * 4)
    lines.append(f"  scatter, all methods                      : {fmt(t_s)}   {moved / (t_s[0] * 1e-3) / 1e12:5.3f} TB/s algorithmic   torch index_copy_ {fmt(t_ts)}")
    bstat = torch.stack([bt["status"] for bt in backtests]).contiguous()
    byh = [bt["yhat"] for bt in backtests]
    t_pick = timed(lambda: device.combine_block(byh, "pick", status=bstat, winner=winner, group_div=F))
    stacked = torch.stack(byh)

    def torch_pick():
        idx = winner.long().repeat_interleave(F).view(1, n_pairs, 1).expand(1, n_pairs, H)
        return torch.gather(stacked, 0, idx)[0]

    t_tpick = timed(torch_pick)
    lines.append(f"  pick of the backtest blocks [{n_pairs:,d} x {H}]  : {fmt(t_pick)}   torch gather on the stacked blocks (stack not timed) {fmt(t_tpick)}")
    for name in ("mean", "median", "inverse_score"):
        t_c = timed(lambda: device.combine_block(byh, name, status=bstat, weights=scores, group_div=F))
        lines.append(f"  combine {name:13s} of the backtest blocks : {fmt(t_c)}")
    cb = device.DeviceBatch(n, T_M5, lib.make_options("CrostonClassic", H, auto_detect=False), dev)
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
    lines.append(f"  CrostonClassic run on the source block, the same run: {c_med:9.3f} ms device   {8.0 * T_M5 * n / (c_med * 1e-3) / 1e12:5.2f} TB/s of values read")
    for _, b in subs:
        b.close()
    del subs, blocks, backtests, byh, stacked, expanded
    print("\n".join(lines), flush=True)

    # ---- the routes, alternating in the same run ----
    def route_select():
        return device.select_block(y, lens, methods, folds, metric="rmse", mode="pick", fallback=0, n_series=n)

    def glue_and_subs(bts):
        sc = torch.stack([device.score_block(bt["actual"].view(n, F * H), bt["yhat"].view(n, F * H), "rmse")[0][:n] for bt in bts])
        w = torch.argmin(torch.where(torch.isnan(sc), torch.full_like(sc, float("inf")), sc), dim=0)
        out = torch.empty((n, H), dtype=torch.float64, device=dev)
        for m in range(M):
            idx = torch.nonzero(w == m).view(-1)
            k3 = int(idx.numel())
            if not k3:
                continue
            ldm = (k3 + 63) // 64 * 64
            blk = torch.zeros((T_M5, ldm), dtype=torch.float64, device=dev)
            blk[:, :k3] = torch.index_select(y, 1, idx)
            ln = torch.zeros(ldm, dtype=torch.int32, device=dev)
            ln[:k3] = lens[idx]
            b = device.DeviceBatch(k3, T_M5, methods[m], dev)
            b.set_block(blk, ln)
            b.run()
            out.index_copy_(0, idx, b.results()["yhat"])
            torch.cuda.synchronize()
            b.close()
        return out

    def route_a():
        return glue_and_subs([device.backtest_block(y, lens, o, folds, n_series=n) for o in methods])

    def route_b():
        bts = [device.backtest_block(y, lens, o, folds, n_series=n) for o in methods]
        sc = torch.stack([device.score_block(bt["actual"].view(n, F * H), bt["yhat"].view(n, F * H), "rmse")[0][:n] for bt in bts])
        w = torch.argmin(torch.where(torch.isnan(sc), torch.full_like(sc, float("inf")), sc), dim=0)
        full = []
        for o in methods:
            b = device.DeviceBatch(n, T_M5, o, dev)
            b.set_block(y, lens)
            b.run()
            full.append(b.results()["yhat"].clone())
            torch.cuda.synchronize()
            b.close()
        return torch.gather(torch.stack(full), 0, w.view(1, n, 1).expand(1, n, H))[0]

    for fn in (route_select, route_a, route_b):
        events(fn)
    ms = {"select": [], "a": [], "b": []}
    for _ in range(max(2, steps // 2)):
        ms["select"].append(events(route_select)[0])
        ms["a"].append(events(route_a)[0])
        ms["b"].append(events(route_b)[0])
    med = {k: (float(np.median(v)), float(np.min(v))) for k, v in ms.items()}
    lines.append(f"  whole call select_block (pick)                                            : {fmt(med['select'])}")
    lines.append(f"  route (a): {M} x backtest_block with its own expand, torch glue, sub-batches : {fmt(med['a'])}   select_block / (a) = {med['select'][0] / med['a'][0]:.2f}")
    lines.append(f"  route (b): (a)'s backtests, every method refitted on the whole block, indexed : {fmt(med['b'])}   select_block / (b) = {med['select'][0] / med['b'][0]:.2f}")
    text = "\n".join(lines) + "\n"
    print(text)
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
