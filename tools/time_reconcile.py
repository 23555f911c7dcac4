"""Device time of the reconciliation of hierarchy forecasts (device.reconcile_block: anofox_hip_reconcile_factor_device and
anofox_hip_reconcile_apply_device):
    python tools/time_reconcile.py [n_series] [steps] [--out FILE]

The keys are the synthetic M5 structure of tools/time_hierarchy.py (n_series leaves = items x 10 stores), the block is one forecast
block [n_out x 28], series-major as DeviceBatch results lie.  Three plans: the prefix plan (total, state, store: 14 aggregates at
n = 30,490), M5's nine coarse levels (154) and all twelve (12,350).  Per plan and method: the factor alone (it waits for the device:
wall time around the call) and the apply alone (between two stream events), one warm-up, then `steps` calls, median (min); the
deviation of every aggregate of the result from the chain over its bottoms is checked to be zero bits.  On the largest plan both
tiles of the trailing update (the developer knob reconcile_trailing of ANOFOX_HIP_TUNE: 0 plain FMA, 1 v_mfma_f64_16x16x4_f64).
The yardsticks: the numpy route the entries replace (block to the host, M from a sparse product, np.linalg.cholesky and two
triangular solves, the bottoms and their sums, back up) and, where this torch build has them, torch.linalg.cholesky +
torch.cholesky_solve of the same M on the same device."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

H = 28


def main():
    import torch

    from anofox_forecast_amd.device import reconcile_block, reconcile_plan_device
    argv = sys.argv[1:]
    out_path = argv[argv.index("--out") + 1] if "--out" in argv else None
    pos = [a for i, a in enumerate(argv) if a != "--out" and (i == 0 or argv[i - 1] != "--out")]
    n = int(pos[0]) if pos else 30490
    steps = int(pos[1]) if len(pos) > 1 else 5
    dev = torch.device("cuda:0")
    s = np.arange(n)
    per_store = -(-n // 10)
    store = s // per_store
    state = store * 3 // 10
    item = s % per_store
    dept = item * 7 // per_store
    cat = np.array([0, 0, 1, 1, 2, 2, 2])[dept]

    def number(levels):
        rows, base = [], 0
        for key in levels:
            _, inv = np.unique(key, return_inverse=True)
            rows.append(base + inv)
            base += int(inv.max()) + 1
        return np.array(rows, dtype=np.int32)

    zero = np.zeros(n, dtype=np.int64)
    coarse = [zero, state, store, cat, dept, state * 3 + cat, state * 7 + dept, store * 3 + cat, store * 7 + dept]
    plans = {"prefix plan (total, state, store)": number([zero, state, store, s]),
             "nine coarse levels": number(coarse + [s]),
             "all twelve levels": number(coarse + [item, item * 3 + state, s])}
    lines = [f"device.reconcile_block on one {torch.cuda.get_device_name(0)}: {n:,d} leaves (synthetic M5 keys), one forecast block of h = {H} "
             f"rows, series-major, fp64; {steps} steps, median (min) ms", f"(python tools/time_reconcile.py {n} {steps})"]

    def timed(fn, wall=False):
        fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(steps):
            if wall:
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                ms.append((time.perf_counter() - t0) * 1e3)
            else:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                torch.cuda.synchronize()
                ms.append(e0.elapsed_time(e1))
        return float(np.median(ms)), float(np.min(ms))

    rng = np.random.default_rng(7)
    for name, column_of in plans.items():
        plan = reconcile_plan_device(column_of, device=dev)
        n_out, na = plan["n_out"], plan["n_agg"]
        bottom, aggs = plan["bottom_col"].cpu().numpy(), plan["agg_cols"].cpu().numpy()
        offs, memb = plan["col_offsets"].cpu().numpy(), plan["members"].cpu().numpy()
        base = rng.uniform(0.5, 20.0, size=(n_out, H))
        A_rows = np.repeat(np.arange(na), np.diff(offs)[aggs])
        A_cols = np.concatenate([memb[offs[c]:offs[c + 1]] for c in aggs])
        for i, c in enumerate(aggs):
            base[c] = base[bottom[memb[offs[c]:offs[c + 1]]]].sum(axis=0) * rng.uniform(0.9, 1.1, size=H)
        yb = torch.from_numpy(base).to(dev)
        out = torch.empty_like(yb)
        var_w = torch.from_numpy(10.0 ** rng.uniform(0.0, 3.0, size=n_out)).to(dev)
        lines.append(f"{name}: {n_out:,d} columns, {na:,d} aggregates, {plan['n_leaf']:,d} member entries; factor {na * na * 8 / 2**20:,.1f} MiB")
        for method in ("bottom_up", "ols", "wls_struct", "wls_var"):
            w = var_w if method == "wls_var" else None
            r = reconcile_block(yb, plan, method, weights=w, out=out)
            torch.cuda.synchronize()
            y = r["y"].cpu().numpy()
            incoherent = 0
            for c in (aggs if na <= 200 else aggs[:: max(1, na // 200)]):
                acc = np.zeros(H)
                for b in bottom[memb[offs[c]:offs[c + 1]]]:
                    acc = acc + y[b]
                incoherent += int((acc != y[c]).sum())
            change = float(np.max(np.abs(y - base)))
            if method == "bottom_up":
                a_med, a_min = timed(lambda: reconcile_block(yb, plan, method, out=out))
                lines.append(f"    {method:10s}: apply {a_med:9.3f} ({a_min:9.3f}) ms   no factor   cells off the chain: {incoherent}")
                continue
            f_med, f_min = timed(lambda: reconcile_block(yb, plan, method, weights=w, out=out), wall=True)
            a_med, a_min = timed(lambda: reconcile_block(yb, plan, method, weights=w, factor=r["factor"], out=out))
            lines.append(f"    {method:10s}: factor + apply {f_med:9.3f} ({f_min:9.3f}) ms wall   apply alone {a_med:9.3f} ({a_min:9.3f}) ms   "
                         f"largest change {change:.3g}   cells off the chain: {incoherent}")
            print(lines[-1], flush=True)
        if na > 1000:
            for variant, label in (("0", "plain FMA tile, 4 x 4 per thread"), ("1", "v_mfma_f64_16x16x4_f64")):
                os.environ["ANOFOX_HIP_TUNE"] = f"reconcile_trailing={variant}"
                med, mn = timed(lambda: reconcile_block(yb, plan, "ols", out=out), wall=True)
                lines.append(f"    trailing update, {label}: factor + apply {med:9.3f} ({mn:9.3f}) ms wall")
                print(lines[-1], flush=True)
            os.environ.pop("ANOFOX_HIP_TUNE", None)
        # the numpy route: download, M, Cholesky, two solves, bottoms, sums, upload (ols)
        t0 = time.perf_counter()
        host = yb.cpu().numpy()
        starts = np.concatenate([[0], np.cumsum(np.diff(offs)[aggs])[:-1]])
        M = np.eye(na)
        leaf_offs, leaf_aggs = plan["leaf_offsets"].cpu().numpy(), plan["leaf_aggs"].cpu().numpy()
        for leaf in range(n):                                    # M = I + A A^T from the leaves' short aggregate lists
            held = leaf_aggs[leaf_offs[leaf]:leaf_offs[leaf + 1]]
            M[np.ix_(held, held)] += 1.0
        resid = host[aggs] - np.add.reduceat(host[bottom[A_cols]], starts, axis=0)
        Lh = np.linalg.cholesky(M)
        lam = np.linalg.solve(Lh.T, np.linalg.solve(Lh, resid))
        spread = np.zeros((n, H))
        np.add.at(spread, A_cols, lam[A_rows])
        host[bottom] = host[bottom] + spread
        host[aggs] = np.add.reduceat(host[bottom[A_cols]], starts, axis=0)
        up = torch.from_numpy(host).to(dev)
        torch.cuda.synchronize()
        lines.append(f"    numpy route (download, M = I + A A^T, np.linalg.cholesky, two solves, upload; one run, ols): {(time.perf_counter() - t0) * 1e3:9.1f} ms")
        print(lines[-1], flush=True)
        Mt = rt = None
        try:
            Mt = torch.from_numpy(M).to(dev)
            rt = torch.from_numpy(resid).to(dev)
            t_med, t_min = timed(lambda: torch.cholesky_solve(rt, torch.linalg.cholesky(Mt)), wall=True)
            lines.append(f"    torch.linalg.cholesky + torch.cholesky_solve of the same M on the device (M already assembled and resident): "
                         f"{t_med:9.3f} ({t_min:9.3f}) ms wall")
        except Exception as exc:  # noqa: BLE001 -- a torch build without the solver backend says so here
            lines.append(f"    torch.linalg.cholesky on the device: not available in this build ({type(exc).__name__}: {str(exc)[:120]})")
        print(lines[-1], flush=True)
        del up, Mt, rt, M
    text = "\n".join(lines) + "\n"
    print(text)
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
