"""Device time of the SSA and STL period entries on the synthetic M5 block (device-resident, 30,490 x 1,913 raw counts):

    python tools/time_period_search.py [n_series] [steps] [--out profiles/period_search_m5.txt] [--seconds 40]

SSA: window_size 28 with 2 and with 10 components on the whole block, the one-wavefront route against the 256-lane route at that
window, the default window (637) on as many columns as `--seconds` allows (found from a first run on 256 columns; the report
states the columns and scales to the block openly).  The split between the covariance and the iterations is taken by timing the
same launch on an all-zero block of the same shape: its covariance performs the same operations and its iterations stop at the
first norm.  STL: the defaults on the whole block, against the route it replaces (one anofox_hip_mstl_decompose_device call per
candidate period plus the strengths in torch).  Slices are compared with the numpy restatement tests/period_search_ref.py (==) and
timed through it; torch's batched linalg.eigh of the same covariance matrices is timed for orientation (another algorithm, other
numbers).  Each time is the median over `steps` runs of the wall time of the device entry (it returns after its stream has
finished).  --out writes the report to a file as well."""
import ctypes as C
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

T = 1913
LINES = []


def say(text=""):
    print(text, flush=True)
    LINES.append(text)


def median_time(fn, steps):
    fn()
    times = []
    for _ in range(steps):
        t0 = time.perf_counter()
        fn()
        times.append(time.perf_counter() - t0)
    return float(np.median(times))


def main():
    import torch

    import period_search_ref as R
    from anofox_forecast_amd import device, lib, synth
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    n = int(args[0]) if args else 30490
    steps = int(args[1]) if len(args) > 1 else 3
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
    seconds = float(sys.argv[sys.argv.index("--seconds") + 1]) if "--seconds" in sys.argv else 40.0
    Y = synth.gen_series(synth.SEED_M5, 0, n, T, 7, positive=False)
    L = lib.load()
    ld = (n + 63) // 64 * 64
    y = torch.from_numpy(device.pack_time_major(Y, ld)).cuda()
    zeros = torch.zeros_like(y)
    ln = torch.full((ld,), T, dtype=torch.int32, device="cuda")
    ln[n:] = 0
    name = torch.cuda.get_device_name(0)
    say(f"SSA and STL period detection, synthetic M5 block {n} x {T} (device-resident), {name}; median of {steps} runs")
    say()

    def ssa(block, window, comps, route="auto", cols=n):
        return device.ssa_period_block(block, ln, window, comps, route=route, n_series=cols)

    # ---- SSA, window 28
    l, k = 28, T - 28 + 1
    cov_macs = l * (l + 1) // 2 * k
    for comps in (2, 10):
        t_all = median_time(lambda: ssa(y, 28, comps), steps)
        t_cov = median_time(lambda: ssa(zeros, 28, comps), steps)
        say(f"ssa window 28, {comps:2d} components: {t_all * 1e3:9.1f} ms  {n / t_all:10.0f} series/s   covariance (all-zero block) {t_cov * 1e3:8.1f} ms"
            f" = {n * cov_macs / t_cov:.3e} multiply-adds/s, iterations {1e3 * (t_all - t_cov):8.1f} ms")
    t_wave = median_time(lambda: ssa(y, 28, 2, "auto"), steps)
    t_group = median_time(lambda: ssa(y, 28, 2, "group"), steps)
    a, b = ssa(y, 28, 2, "auto"), ssa(y, 28, 2, "group")
    same = all(torch.equal(a[f][:, :n].nan_to_num(-7.0), b[f][:, :n].nan_to_num(-7.0)) for f in ("figures", "eigenvalues", "detected_periods"))
    say(f"ssa window 28, 2 components, one wavefront per series {t_wave * 1e3:.1f} ms against 256 lanes per series {t_group * 1e3:.1f} ms; the same bits: {same}")

    # ---- SSA, default window
    l = R.ssa_window(T)
    k = T - l + 1
    cov_macs = l * (l + 1) // 2 * k
    t0 = time.perf_counter()
    ssa(y, 0, 0, cols=256)
    t256 = time.perf_counter() - t0
    cols = int(min(n, max(256, 256 * seconds / t256)))
    t0 = time.perf_counter()
    r = ssa(y, 0, 0, cols=cols)
    t_all = time.perf_counter() - t0
    t0 = time.perf_counter()
    ssa(zeros, 0, 0, cols=cols)
    t_cov = time.perf_counter() - t0
    okc = int((r["status"][:cols] == 0).sum())
    say()
    say(f"ssa default window ({l}), 10 components, {cols} of {n} columns, one run (first run on 256 columns: {t256:.2f} s): {t_all:.2f} s, {cols / t_all:.1f} series/s,"
        f" {okc} done; scaled to the block by columns: {t_all * n / cols:.0f} s")
    say(f"  covariance (all-zero block, same columns): {t_cov:.2f} s = {cols * cov_macs / t_cov:.3e} multiply-adds/s; iterations: {t_all - t_cov:.2f} s")
    v0 = Y[0].astype(np.float64)
    t0 = time.perf_counter()
    ref = R.ssa_period(v0)
    t_ref = time.perf_counter() - t0
    matvecs = sum(ref["iterations"]) + ref["n_eigenvalues"]
    got = [float(x) for x in r["eigenvalues"][:ref["n_eigenvalues"], 0].cpu()]
    say(f"  series 0: numpy restatement {t_ref:.2f} s on one CPU thread, {matvecs} matvecs over {ref['n_eigenvalues']} components; eigenvalues equal (==): {got == ref['eigenvalues']},"
        f" period {float(r['period'][0])} == {ref['period']}: {float(r['period'][0]) == ref['period'] or ref['period'] != ref['period']}")
    say(f"  if every series needs about as many matvecs: {cols * matvecs * l * l / (t_all - t_cov):.3e} multiply-adds/s and {cols * matvecs * l * l * 8 / (t_all - t_cov) / 1e12:.2f} TB/s"
        f" of matrix reads in the iterations (the matrix of {l * l * 8 / 1e6:.2f} MB is read once per matvec from the workspace)")

    # ---- SSA against the restatement and torch.linalg.eigh
    chk = 8
    t0 = time.perf_counter()
    refs = [R.ssa_period(Y[i].astype(np.float64), 28, 10) for i in range(chk)]
    t_ref = (time.perf_counter() - t0) / chk
    r = ssa(y, 28, 10)
    eq = all([float(x) for x in r["eigenvalues"][:w["n_eigenvalues"], i].cpu()] == w["eigenvalues"] and float(r["variance_explained"][i]) == w["variance_explained"]
             for i, w in enumerate(refs))
    say()
    say(f"ssa window 28, 10 components: numpy restatement {t_ref * 1e3:.1f} ms per series on one CPU thread ({t_ref * n:.0f} s for the block); first {chk} series equal (==): {eq}")
    sub = min(n, 4096)
    X = y[:, :sub].t().contiguous().unfold(1, T - 28 + 1, 1)            # [sub, 28, k]
    torch.cuda.synchronize()

    def eigh():
        cmat = X @ X.transpose(1, 2) / float(T - 28 + 1)
        torch.linalg.eigh(cmat)
        torch.cuda.synchronize()
    t_eigh = median_time(eigh, steps)
    say(f"for orientation only (another algorithm, other numbers): torch covariance + batched linalg.eigh of {sub} 28 x 28 matrices {t_eigh * 1e3:.1f} ms"
        f" ({t_eigh * n / sub * 1e3:.0f} ms scaled to the block)")

    # ---- STL
    say()
    t_stl = median_time(lambda: device.stl_period_block(y, ln, n_series=n), steps)
    s = device.stl_period_block(y, ln, n_series=n)
    cands = R.stl_candidates(T)
    say(f"stl defaults ({len(cands)} candidates {cands[0]} .. {cands[-1]}): {t_stl * 1e3:.1f} ms  {n / t_stl:.0f} series/s; rows of {T} observations live in the workspace")
    trend = torch.empty_like(y); seas = torch.empty_like(y); rem = torch.empty_like(y)
    info = torch.zeros(ld, dtype=torch.int32, device="cuda")
    err = lib.AnofoxError()

    def replaced():
        best = torch.zeros(ld, dtype=torch.float64, device="cuda")
        period = torch.full((ld,), float(cands[0]), dtype=torch.float64, device="cuda")
        for p in cands:
            pp = (C.c_int * 1)(p)
            assert L.anofox_hip_mstl_decompose_device(y.data_ptr(), ld, ln.data_ptr(), n, T, pp, 1, 1, trend.data_ptr(), seas.data_ptr(), rem.data_ptr(),
                                                      info.data_ptr(), None, C.byref(err)), err.message
            var_r = rem.var(dim=0, unbiased=False)
            var_d = (seas + rem).var(dim=0, unbiased=False)
            strength = torch.where(var_d > R.EPS, (1.0 - var_r / var_d).clamp(min=0.0), torch.zeros_like(var_d))
            better = strength > best
            best = torch.where(better, strength, best)
            period = torch.where(better, torch.full_like(period, float(p)), period)
        torch.cuda.synchronize()
        return period, best
    t_old = median_time(replaced, 1)
    period, best = replaced()
    const = s["index"][:n] < 0
    agree = int(((period[:n] == s["period"][:n]) | const).sum())
    say(f"the route it replaces, {len(cands)} anofox_hip_mstl_decompose_device calls + strengths in torch: {t_old * 1e3:.1f} ms ({t_old / t_stl:.1f} x);"
        f" the same winner on {agree} of {n} series (torch's variance sums in another order; {int(const.sum())} constant series)")
    t0 = time.perf_counter()
    ref = R.stl_period(Y[0].astype(np.float64))
    t_ref = time.perf_counter() - t0
    got = [float(x) for x in s["candidate_strengths"][:len(ref["candidates"]), 0].cpu()]
    say(f"stl series 0: restatement {t_ref:.1f} s on one CPU thread ({t_ref * n / 3600:.1f} h for the block); candidate strengths equal (==): {got == ref['candidate_strengths']},"
        f" index {int(s['index'][0])} == {ref['index']}")

    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        open(out_path, "w").write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
