"""Device time of the scaled, weighted scores (device.scale_block, device.weighted_scores_block, api.wrmsse_batch) at the M5 shape:
    python tools/time_scaled_scores.py [n_series] [steps] [--libs 1=PATH,4=PATH,8=PATH] [--out FILE]

The block is 1,913 rows of synthetic M5 counts with leading zeros, the leaves (30,490 columns) and their aggregate under M5's twelve
groupings (42,840 columns).  Every device figure is the time between two stream events around calls that only enqueue: one warm-up,
then `steps` calls, median (min) ms; the algorithmic rate beside it is the block read once (8 bytes x rows x columns) over that time.
  * scale_kernel at 1 / 4 / 8 / 16 rows in flight: the library of this build, and one experiment build per entry of --libs
    (make -C anofox-forecast_amd/csrc BUILD=... OUT=PATH EXTRA=-DANOFOX_SCALE_ROWS=R), each timed in a child process of its own that
    loads that library (ANOFOX_HIP_LIB), on the same block; the bits of every build are compared with this build's;
  * the same kernel with and without trimming, with a weight source of its own, and at lag 7 (the second stream of loads);
  * croston_kernel (a CrostonClassic run) on the leaves in the same run, the yardstick of a one-lane-per-column sweep;
  * the weighted step over the twelve column ranges, one loss row (RMSSE) and nine (the pinball rows);
  * the whole api.wrmsse_batch from host buffers (wall clock: pack, upload, four aggregations, mse, scale, weighted step, readback);
  * the route it replaces: download of the aggregate block and numpy for the same three numbers per column (wall clock)."""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

T_M5, H, PERIOD = 1913, 28, 7


def m5_block(n):
    from anofox_forecast_amd import synth
    Y = synth.gen_series(synth.SEED_M5, 0, n, T_M5, PERIOD, positive=False)
    Y = np.maximum(np.round(Y), 0.0)
    rng = np.random.default_rng(5)
    start = (rng.random(n) * rng.random(n) * (T_M5 - 100)).astype(np.int64)       # leading zeros: an item is listed some time into the span
    Y[np.arange(T_M5)[None, :] < start[:, None]] = 0.0
    return Y


def m5_groupings(n):
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
    return np.array(out, dtype=np.int32)


def timed(torch, fn, k):
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


def scale_times(n, steps):
    """The scale kernel of the loaded library on the leaves and on the aggregate -> {"leaves": (median, min), "aggregate": ..., "digest"}."""
    import torch

    from anofox_forecast_amd import device
    dev = torch.device("cuda:0")
    ld = (n + 63) // 64 * 64
    y = torch.from_numpy(device.pack_time_major(m5_block(n), ld)).to(dev)
    lens = torch.zeros(ld, dtype=torch.int32, device=dev)
    lens[:n] = T_M5
    plan = device.hierarchy_plan_device(torch.from_numpy(m5_groupings(n)).to(dev))
    agg = device.aggregate_block(y, lens, plan, n_series=n, t_out=T_M5)
    out = {}
    for name, block, ln, cols in (("leaves", y, lens, n), ("aggregate", agg["y"], agg["lengths"], plan["n_out"])):
        out[name] = timed(torch, lambda: device.scale_block(block, ln, lag=1, trim_leading_zeros=True, tail_rows=28, n_cols=cols), steps)
        r = device.scale_block(block, ln, lag=1, trim_leading_zeros=True, tail_rows=28, n_cols=cols)
        out[name + "_digest"] = int(r["scale"][:, :cols].contiguous().view(torch.int64).sum().item()) ^ int(r["first"].sum().item())
    return out


def main():
    argv = sys.argv[1:]
    opt = lambda k, d: argv[argv.index(k) + 1] if k in argv else d
    out_path, libs, child = opt("--out", None), opt("--libs", ""), opt("--child", None)
    pos, skip = [], False
    for a in argv:
        if skip:
            skip = False
        elif a in ("--out", "--libs", "--child"):
            skip = True
        else:
            pos.append(a)
    n = int(pos[0]) if pos else 30490
    steps = int(pos[1]) if len(pos) > 1 else 10
    if child is not None:                                              # an experiment build, in a process of its own
        print("CHILD " + json.dumps(scale_times(n, steps)), flush=True)
        return
    builds = {}
    for item in [v for v in libs.split(",") if v]:                    # the children first, one at a time, before this process opens the device
        rows, path = item.split("=", 1)
        env = dict(os.environ, ANOFOX_HIP_LIB=os.path.abspath(path))
        r = subprocess.run([sys.executable, os.path.abspath(__file__), str(n), str(steps), "--child", rows], env=env, capture_output=True, text=True,
                           timeout=600)
        line = [l for l in r.stdout.splitlines() if l.startswith("CHILD ")]
        if r.returncode != 0 or not line:
            raise RuntimeError(f"the build with {rows} rows in flight failed: {r.stderr[-2000:]}")
        builds[int(rows)] = json.loads(line[0][6:])
        print(f"(the build with {rows} rows in flight is timed)", flush=True)

    import torch

    from anofox_forecast_amd import api, device, lib
    dev = torch.device("cuda:0")
    fmt = lambda t: f"{t[0]:9.3f} ({t[1]:9.3f})"
    rate = lambda cols, ms: f"{8.0 * T_M5 * cols / (ms * 1e-3) / 1e12:5.2f} TB/s"
    lines = [f"device.scale_block / weighted_scores_block / api.wrmsse_batch on one {torch.cuda.get_device_name(0)}, {n:,d} leaves x {T_M5:,d} rows "
             f"(synthetic M5 counts with leading zeros), M5's twelve groupings; {steps} steps, median (min) ms between stream events",
             f"(python tools/time_scaled_scores.py {n} {steps}" + (f" --libs {libs}" if libs else "") + ")"]

    def say(text):
        lines.append(text)
        print(text, flush=True)

    here = scale_times(n, steps)
    Y = m5_block(n)
    ld = (n + 63) // 64 * 64
    y = torch.from_numpy(device.pack_time_major(Y, ld)).to(dev)
    lens = torch.zeros(ld, dtype=torch.int32, device=dev)
    lens[:n] = T_M5
    column_of = m5_groupings(n)
    plan = device.hierarchy_plan_device(torch.from_numpy(column_of).to(dev))
    n_out = plan["n_out"]
    agg = device.aggregate_block(y, lens, plan, n_series=n, t_out=T_M5)
    ay, al = agg["y"], agg["lengths"]

    say("scale_kernel, lag 1, trimmed, tail 28, by rows in flight (this build last):")
    for rows in sorted(builds):
        b = builds[rows]
        same = all(b[k + "_digest"] == here[k + "_digest"] for k in ("leaves", "aggregate"))
        say(f"  {rows:2d} rows in flight: leaves {fmt(b['leaves'])}  {rate(n, b['leaves'][0])}   aggregate of {n_out:,d} columns {fmt(b['aggregate'])}  "
            f"{rate(n_out, b['aggregate'][0])}   bits {'equal to' if same else 'DIFFER from'} this build's")
    say(f"  this build      : leaves {fmt(here['leaves'])}  {rate(n, here['leaves'][0])}   aggregate of {n_out:,d} columns {fmt(here['aggregate'])}  "
        f"{rate(n_out, here['aggregate'][0])}")

    k = steps
    t = timed(torch, lambda: device.scale_block(y, lens, lag=1, trim_leading_zeros=False, tail_rows=28, n_cols=n), k)
    say(f"  leaves, without trimming                       : {fmt(t)}  {rate(n, t[0])}")
    w = (y * 2.5).contiguous()
    t = timed(torch, lambda: device.scale_block(y, lens, w_src=w, lag=1, trim_leading_zeros=True, tail_rows=28, n_cols=n), k)
    say(f"  leaves, trimmed, a weight source of its own    : {fmt(t)}  {rate(n, t[0])}")
    del w
    t = timed(torch, lambda: device.scale_block(y, lens, lag=7, trim_leading_zeros=True, tail_rows=28, n_cols=n), k)
    say(f"  leaves, trimmed, lag 7 (a second stream)       : {fmt(t)}  {rate(n, t[0])} of the block read once")

    cb = device.DeviceBatch(n, T_M5, lib.make_options("CrostonClassic", H, auto_detect=False), dev)
    cb.set_block(y, lens)
    cb.run()
    torch.cuda.synchronize()
    c_ms = []
    for _ in range(k):
        cb.run()
        torch.cuda.synchronize()
        c_ms.append(cb.stats()["total_device_ms"])
    cb.close()
    c_med = float(np.median(c_ms))
    say(f"  croston_kernel (a CrostonClassic run), the leaves, the same run: {c_med:9.3f} ({float(np.min(c_ms)):9.3f})  {rate(n, c_med)}")

    # the weighted step on the aggregate
    sc = device.scale_block(ay, al, lag=1, trim_leading_zeros=True, tail_rows=28, n_cols=n_out)
    ranges = np.array([[int(g.min()), int(g.max()) + 1] for g in column_of], dtype=np.int32)
    rg = torch.from_numpy(ranges).to(dev)
    ld_out = int(sc["scale"].shape[1])
    loss = torch.rand((9, ld_out), dtype=torch.float64, device=dev) + 0.1
    t = timed(torch, lambda: device.weighted_scores_block(loss[0], sc["scale"][0], sc["scale"][3], rg, transform="root", col_status=sc["status"], n_cols=n_out), k)
    say(f"weighted step, twelve ranges over {n_out:,d} columns, one loss row (RMSSE)     : {fmt(t)}")
    t = timed(torch, lambda: device.weighted_scores_block(loss, sc["scale"][1], sc["scale"][3], rg, transform="ratio", col_status=sc["status"], n_cols=n_out), k)
    say(f"weighted step, twelve ranges over {n_out:,d} columns, nine loss rows (pinball) : {fmt(t)}")

    # the whole chain from host buffers, and the route it replaces
    rng = np.random.default_rng(9)
    act = rng.poisson(1.2, size=(n, H)).astype(np.float64)
    fc = act + rng.normal(0.0, 0.8, size=(n, H))
    prices = [np.full(T_M5, float(p)) for p in np.round(rng.random(n) * 9.0 + 1.0, 2)]
    train = [Y[s] for s in range(n)]
    walls = []
    for _ in range(3):
        t0 = time.perf_counter()
        res, err = api.wrmsse_batch(train, fc, act, column_of=column_of, prices=prices, lag=1, trim_leading_zeros=True, tail_rows=28)
        walls.append((time.perf_counter() - t0) * 1e3)
        assert err["ok"], err
    say(f"api.wrmsse_batch, host buffers to the WRMSSE ({res['wrmsse']:.6f}), wall clock ms (first call, then): " + ", ".join(f"{v:9.1f}" for v in walls))

    def numpy_route():
        a = ay.cpu().numpy()[:, :n_out]
        t0 = np.where((a != 0.0).any(axis=0), (a != 0.0).argmax(axis=0), T_M5)
        d = np.diff(a, axis=0)
        keep = np.arange(1, T_M5)[:, None] > t0[None, :]
        terms = np.maximum(T_M5 - t0 - 1, 1)
        return (d * d * keep).sum(axis=0) / terms, (np.abs(d) * keep).sum(axis=0) / terms, a[-28:].sum(axis=0)
    walls = []
    for _ in range(2):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        numpy_route()
        walls.append((time.perf_counter() - t0) * 1e3)
    say(f"the route it replaces: download of the {T_M5:,d} x {n_out:,d} aggregate and numpy for msd, mad and tail, wall clock ms: "
        + ", ".join(f"{v:9.1f}" for v in walls) + "   (another order of addition: comparable time, not comparable bits)")
    text = "\n".join(lines) + "\n"
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
