"""Device time of the matrix-profile period entry on the synthetic M5 block (device-resident, 30,490 x 1,913 raw counts):

    python tools/time_matrix_profile.py [n_series] [steps] [--out profiles/matrix_profile_m5.txt] [--columns 2048]

The defaults (m = 191, exclusion 47, P = 1,723: 1.4e6 pairs of 191 steps per series) on the first `--columns` columns, then on the
whole block when the first run says that takes under `--seconds` (default 60), and on the block's first 400 rows (m = 40).  The
report states the pair-steps per second of the largest run.  Slices are compared with the numpy restatement
tests/matrix_profile_ref.py (==) and timed through it.  Each time is the median over `steps` runs of the wall time of the device
entry (it returns after its stream has finished).  An experiment build (make EXTRA=-DMATRIX_PROFILE_RECOMPUTE_Z BUILD=... OUT=...)
is timed by pointing ANOFOX_HIP_LIB at it.  --out writes the report to a file as well."""
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
    times = []
    for _ in range(steps):
        t0 = time.perf_counter()
        fn()
        times.append(time.perf_counter() - t0)
    return float(np.median(times))


def option(name, default):
    return type(default)(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def pair_steps(n, sub=None, n_best=None):
    import matrix_profile_ref as R
    m = R.subsequence(n, sub)
    P, excl = n - m + 1, R.exclusion(m, n_best)
    pairs = (P - excl) * (P - excl + 1) // 2 if P > excl else 0
    return m, P, excl, pairs * m


def main():
    import torch

    import matrix_profile_ref as R
    from anofox_forecast_amd import device, lib, synth
    args = [a for a in sys.argv[1:] if not a.startswith("--") and a.isdigit()]
    n = int(args[0]) if args else 30490
    steps = int(args[1]) if len(args) > 1 else 3
    out_path = option("--out", "")
    columns = min(option("--columns", 2048), n)
    seconds = option("--seconds", 60.0)
    Y = synth.gen_series(synth.SEED_M5, 0, n, T, 7, positive=False)
    ld = (n + 63) // 64 * 64
    y = torch.from_numpy(device.pack_time_major(Y, ld)).cuda()
    ln = torch.full((ld,), T, dtype=torch.int32, device="cuda")
    ln[n:] = 0
    say(f"Matrix-profile period detection, synthetic M5 block {n} x {T} (device-resident), {torch.cuda.get_device_name(0)}; median of {steps} runs")
    say(f"library: {os.path.relpath(lib.LIB_PATH, ROOT)}")
    say()

    def run(block, lengths, cols, profile=False):
        return device.matrix_profile_block(block, lengths, 0, 0, profile=profile, n_series=cols)

    m, P, excl, work = pair_steps(T)
    run(y, ln, min(64, n))                                         # the first launch loads the code object
    t_cols = median_time(lambda: run(y, ln, columns), 1)
    say(f"defaults (m {m}, exclusion {excl}, P {P}: {work:.3e} pair-steps per series), first {columns} columns: {t_cols * 1e3:9.1f} ms"
        f"  {columns * work / t_cols:.3e} pair-steps/s")
    cols = columns
    if columns < n and t_cols * n / columns <= seconds:
        cols = n
        t_all = median_time(lambda: run(y, ln, n), steps)
        say(f"defaults, all {n} columns: {t_all * 1e3:9.1f} ms  {n / t_all:9.0f} series/s  {n * work / t_all:.3e} pair-steps/s")
        t_prof = median_time(lambda: run(y, ln, n, True), steps)
        say(f"the same with the profile and its index written ([{P} x {ld}] fp64 + int32): {t_prof * 1e3:9.1f} ms")
    elif columns < n:
        say(f"the whole block was not run: scaled by columns it takes {t_cols * n / columns:.0f} s, above --seconds {seconds:.0f}")
    y400 = y[:400].contiguous()
    ln400 = torch.clamp(ln, max=400)
    m4, P4, excl4, work4 = pair_steps(400)
    t_400 = median_time(lambda: run(y400, ln400, n), steps)
    say(f"first 400 rows (m {m4}, exclusion {excl4}, P {P4}: {work4:.3e} pair-steps per series), all {n} columns: {t_400 * 1e3:9.1f} ms"
        f"  {n / t_400:9.0f} series/s  {n * work4 / t_400:.3e} pair-steps/s")
    say()
    out = run(y, ln, min(8, n), True)
    fig, prof, idx = out["figures"].cpu().numpy(), out["profile"].cpu().numpy(), out["profile_index"].cpu().numpy()
    t0 = time.perf_counter()
    refs = [R.matrix_profile(Y[s]) for s in range(min(2, n))]
    t_ref = (time.perf_counter() - t0) / len(refs)
    same = all(all(fig[k, s] == r[f] or (fig[k, s] != fig[k, s] and r[f] != r[f]) for k, f in enumerate(R.FIGURES))
               and prof[:P, s].tolist() == r["mp"] and idx[:P, s].tolist() == r["mpi"] for s, r in enumerate(refs))
    say(f"numpy restatement: {t_ref:.2f} s per series on one CPU thread ({t_ref * n / 3600.0:.1f} h for the block);"
        f" figures, profile and index of the first {len(refs)} series equal (==): {same}")
    tied = int((out["figures"][5][:min(8, n)] > 1).sum())
    say(f"series with tied lags among the first {min(8, n)}: {tied}")
    if out_path:
        with open(out_path, "w") as f:
            f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
