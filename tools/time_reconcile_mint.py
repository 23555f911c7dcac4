"""Device time of MinT-shrink (device.reconcile_mint_block: anofox_hip_reconcile_mint_factor_device and
anofox_hip_reconcile_mint_apply_device):
    python tools/time_reconcile_mint.py [n_series] [steps] [--out FILE] [--plans K] [--n-res A,B]

The keys and the three plans are those of tools/time_reconcile.py (14 / 154 / 12,350 aggregates at n = 30,490), the forecast block
is [n_out x 28], the residual block [n_out x n_res], both series-major as DeviceBatch results and backtest_block's errors lie;
n_res 140 (5 folds x 28) and 1,913.  One warm-up, then `steps` calls, median (min).  Per plan and n_res:
  * the factor call with the intensity estimated and with the intensity passed in (wall time around the call: it waits for the
    device); their difference is the Gram product and the intensity;
  * the apply alone (between two stream events);
  * wls_var of reconcile_block on the same plan with the variances as weights: what the full covariance costs over the diagonal one;
  * torch doing the same low-rank algebra on the resident blocks: mm for G and for E^T E, linalg.cholesky + cholesky_solve of the
    same M, and the two thin products.
The time per kernel (variances, Gram, E, assembly, E^T E, factor, apply) comes from a run of its own under a kernel trace:
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/time_reconcile_mint.py 30490 1 --plans 3 --n-res 1913
Every aggregate of the result is checked to equal the chain over its bottoms, and both tiles of the E^T E update (the developer knob
reconcile_mint_ete of ANOFOX_HIP_TUNE: 0 plain FMA, 1 v_mfma_f64_16x16x4_f64) are timed on the largest plan."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

H = 28


def main():
    import torch

    from anofox_forecast_amd.device import reconcile_block, reconcile_mint_block, reconcile_plan_device
    argv = sys.argv[1:]
    opt = {}
    pos = []
    i = 0
    while i < len(argv):
        if argv[i] in ("--out", "--plans", "--n-res"):
            opt[argv[i]] = argv[i + 1]
            i += 2
        else:
            pos.append(argv[i])
            i += 1
    n = int(pos[0]) if pos else 30490
    steps = int(pos[1]) if len(pos) > 1 else 5
    n_res_list = [int(v) for v in opt.get("--n-res", "140,1913").split(",")]
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
    only = opt.get("--plans")
    if only:
        plans = {k: v for j, (k, v) in enumerate(plans.items()) if str(j + 1) in only.split(",")}
    lines = [f"device.reconcile_mint_block on one {torch.cuda.get_device_name(0)}: {n:,d} leaves (synthetic M5 keys), one forecast block of "
             f"h = {H} rows and one residual block, series-major, fp64; {steps} steps, median (min) ms",
             f"(python tools/time_reconcile_mint.py {n} {steps})"]

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

    def say(text):
        lines.append(text)
        print(text, flush=True)

    rng = np.random.default_rng(7)
    for name, column_of in plans.items():
        plan = reconcile_plan_device(column_of, device=dev)
        n_out, na = plan["n_out"], plan["n_agg"]
        bottom, aggs = plan["bottom_col"].cpu().numpy(), plan["agg_cols"].cpu().numpy()
        offs, memb = plan["col_offsets"].cpu().numpy(), plan["members"].cpu().numpy()
        width = np.diff(offs)
        base = rng.uniform(0.5, 20.0, size=(n_out, H))
        for c in aggs:
            base[c] = base[bottom[memb[offs[c]:offs[c + 1]]]].sum(axis=0) * rng.uniform(0.9, 1.1, size=H)
        yb = torch.from_numpy(base).to(dev)
        out = torch.empty_like(yb)
        say(f"{name}: {n_out:,d} columns, {na:,d} aggregates, {plan['n_leaf']:,d} member entries; factor {na * na * 8 / 2**20:,.1f} MiB")
        for n_res in n_res_list:
            # every column: a common factor plus noise, scaled with the root of its member count within 1.5 decades
            scale = np.minimum(np.sqrt(np.maximum(width, 1)), 30.0) * 10.0 ** rng.uniform(0.0, 0.5, size=n_out)
            res = torch.from_numpy(((0.6 * rng.standard_normal((1, n_res)) + rng.standard_normal((n_out, n_res))) * scale[:, None])).to(dev)
            r = reconcile_mint_block(yb, res, plan, out=out)
            torch.cuda.synchronize()
            lam, bundle = r["shrinkage"], r["factor"]
            y = r["y"].cpu().numpy()
            incoherent = 0
            for c in (aggs if na <= 200 else aggs[:: max(1, na // 200)]):
                acc = np.zeros(H)
                for b in bottom[memb[offs[c]:offs[c + 1]]]:
                    acc = acc + y[b]
                incoherent += int((acc != y[c]).sum())
            say(f"  n_res {n_res:,d}: residual block {n_out * n_res * 8 / 2**20:,.1f} MiB, E {n_res * na * 8 / 2**20:,.1f} MiB; shrinkage {lam:.6f}; "
                f"largest change {float(np.max(np.abs(y - base))):.3g}; cells off the chain: {incoherent}")
            e_med, e_min = timed(lambda: reconcile_mint_block(yb, res, plan, out=out), wall=True)
            g_med, g_min = timed(lambda: reconcile_mint_block(yb, res, plan, shrinkage=lam, out=out), wall=True)
            a_med, a_min = timed(lambda: reconcile_mint_block(yb, res, plan, factor=bundle, out=out))
            say(f"    mint_shrink, intensity estimated: factor + apply {e_med:9.3f} ({e_min:9.3f}) ms wall")
            say(f"    mint_shrink, intensity passed in: factor + apply {g_med:9.3f} ({g_min:9.3f}) ms wall   (Gram + intensity: the difference, "
                f"{e_med - g_med:9.3f} ms)")
            say(f"    mint_shrink, apply alone:                        {a_med:9.3f} ({a_min:9.3f}) ms")
            w = torch.where(r["variances"] > 0, r["variances"], torch.ones_like(r["variances"])).contiguous()
            rw = reconcile_block(yb, plan, "wls_var", weights=w, out=out)
            w_med, w_min = timed(lambda: reconcile_block(yb, plan, "wls_var", weights=w, out=out), wall=True)
            wa_med, wa_min = timed(lambda: reconcile_block(yb, plan, "wls_var", weights=w, factor=rw["factor"], out=out))
            say(f"    wls_var (the variances as weights):  factor + apply {w_med:9.3f} ({w_min:9.3f}) ms wall   apply alone {wa_med:9.3f} ({wa_min:9.3f}) ms")
            if na > 1000:
                for variant, label in (("0", "plain FMA tile, 4 x 4 per thread"), ("1", "v_mfma_f64_16x16x4_f64")):
                    os.environ["ANOFOX_HIP_TUNE"] = f"reconcile_mint_ete={variant}"
                    med, mn = timed(lambda: reconcile_mint_block(yb, res, plan, shrinkage=lam, out=out), wall=True)
                    say(f"    E^T E update, {label}: factor + apply {med:9.3f} ({mn:9.3f}) ms wall")
                os.environ.pop("ANOFOX_HIP_TUNE", None)
            # torch on the resident blocks: the same low-rank algebra
            try:
                part = torch.cat([plan["bottom_col"], plan["agg_cols"]]).long()
                v = r["variances"]
                xs = (res[part] / torch.sqrt(v[part])[:, None]).contiguous()              # [n_p, n_res] (the gather and the scaling are not timed)
                t_g, t_gm = timed(lambda: torch.mm(xs.t(), xs).square().sum())
                E = bundle["e"][:, :na].contiguous()
                t_e, t_em = timed(lambda: torch.mm(E.t(), E))
                say(f"    torch: mm for G (+ the sum of squares) {t_g:9.3f} ({t_gm:9.3f}) ms   mm for E^T E {t_e:9.3f} ({t_em:9.3f}) ms")
                rows_a = torch.from_numpy(np.repeat(np.arange(na), width[aggs])).to(dev)
                cols_a = torch.from_numpy(np.concatenate([memb[offs[c]:offs[c + 1]] for c in aggs]).astype(np.int64)).to(dev)
                A = torch.zeros((na, n), dtype=torch.float64, device=dev)             # dense: 3 GB for the largest plan (its assembly is not timed)
                A.index_put_((rows_a, cols_a), torch.ones(len(cols_a), dtype=torch.float64, device=dev), accumulate=True)
                vb, va = v[plan["bottom_col"].long()], v[plan["agg_cols"].long()]
                M = lam * (torch.mm(A * vb, A.t()) + torch.diag(va)) + ((1.0 - lam) / n_res) * torch.mm(E.t(), E)
                rt = (yb[plan["agg_cols"].long()] - torch.mm(A, yb[plan["bottom_col"].long()])).contiguous()
                xb = res[plan["bottom_col"].long()].contiguous()
                t_c, t_cm = timed(lambda: torch.cholesky_solve(rt, torch.linalg.cholesky(M)), wall=True)
                mu = torch.cholesky_solve(rt, torch.linalg.cholesky(M))
                t_t, t_tm = timed(lambda: torch.mm(xb, torch.mm(E, mu)))
                say(f"    torch: linalg.cholesky + cholesky_solve of the same M (assembled and resident) {t_c:9.3f} ({t_cm:9.3f}) ms wall   "
                    f"the two thin products {t_t:9.3f} ({t_tm:9.3f}) ms")
                del xs, E, A, M, rt, xb, mu
            except Exception as exc:  # noqa: BLE001 -- a torch build without a backend says so here
                say(f"    torch on the resident blocks: not available in this build ({type(exc).__name__}: {str(exc)[:160]})")
            del res, r, bundle, rw
            torch.cuda.empty_cache()
    text = "\n".join(lines) + "\n"
    if opt.get("--out"):
        os.makedirs(os.path.dirname(os.path.abspath(opt["--out"])), exist_ok=True)
        with open(opt["--out"], "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
