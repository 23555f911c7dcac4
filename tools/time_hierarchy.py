"""Device time of the hierarchy aggregation on a resident block (device.aggregate_block / anofox_hip_hierarchy_device):
    python tools/time_hierarchy.py [n_series] [steps] [--out FILE]

The block is the synthetic M5 shape, n_series x 1,913 daily counts, time-major, key-sorted.  Three plans:
  * the M5 prefix plan: total, 3 states, 10 stores (series s -> store s // (n / 10)), leaves -- 30,504 output columns at n = 30,490;
  * M5's twelve groupings (total, state, store, category, department, state x category, state x department, store x category,
    store x department, item, item x state, item x store = leaf);
  * leaf only.
Per plan: ms per call of the lane route, the tile route and the automatic choice, each the device time between two events on the
stream (sizing kernel + route kernels; one warm-up, then `steps` calls, median (min)), the algorithmic bytes per second
((nnz + n_out) * T * 8 over the time) beside CrostonClassic's device time on the same block in the same run, and the numpy route it
replaces (block to the host, np.add.reduceat per level, the aggregated series back up).
Then the threshold of the automatic choice (AnofoxHipHierarchyOptions::tile_min_members) swept on the prefix plan, and both routes
on plans of equal-width columns of 2 .. 4,096 consecutive members: the widths at which the tile route wins are what
HIER_TILE_MIN_MEMBERS (csrc/kernels.hpp) rests on."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

T_M5, H = 1913, 28


def main():
    import torch

    from anofox_forecast_amd import lib, synth
    from anofox_forecast_amd.device import DeviceBatch, aggregate_block, hierarchy_plan_device, pack_time_major
    argv = sys.argv[1:]
    out_path = argv[argv.index("--out") + 1] if "--out" in argv else None
    pos = [a for i, a in enumerate(argv) if a != "--out" and (i == 0 or argv[i - 1] != "--out")]
    n = int(pos[0]) if pos else 30490
    steps = int(pos[1]) if len(pos) > 1 else 5
    dev = torch.device("cuda:0")
    Y = synth.gen_series(synth.SEED_M5, 0, n, T_M5, 7, positive=False)
    ld = (n + 63) // 64 * 64
    y = torch.from_numpy(pack_time_major(Y, ld)).to(dev)
    lens = torch.zeros(ld, dtype=torch.int32, device=dev)
    lens[:n] = T_M5

    s = np.arange(n)
    per_store = -(-n // 10)
    store = s // per_store
    state = store * 3 // 10
    item = s % per_store
    dept = item * 7 // per_store
    cat = np.array([0, 0, 1, 1, 2, 2, 2])[dept]

    def number(levels):
        """column_of of a list of per-series keys: the columns of a level follow those of the level before, in key order"""
        rows, base = [], 0
        for key in levels:
            _, inv = np.unique(key, return_inverse=True)
            rows.append(base + inv)
            base += int(inv.max()) + 1
        return np.array(rows, dtype=np.int32)

    zero = np.zeros(n, dtype=np.int64)
    plans = {
        "M5 prefix plan (total, state, store, leaf)": number([zero, state, store, s]),
        "M5's twelve groupings": number([zero, state, store, cat, dept, state * 3 + cat, state * 7 + dept, store * 3 + cat, store * 7 + dept,
                                         item, item * 3 + state, s]),
        "leaf only": number([s]),
    }
    lines = [f"device.aggregate_block on one {torch.cuda.get_device_name(0)}, device-resident, {n:,d} series x {T_M5:,d} rows (synthetic M5 "
             f"counts, key-sorted, all first = 0, no masks); {steps} steps, median (min) ms between two stream events",
             f"(python tools/time_hierarchy.py {n} {steps})"]

    def timed(fn):
        fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(steps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1))
        return float(np.median(ms)), float(np.min(ms))

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
    lines.append(f"CrostonClassic run on the same block, the same run: {c_med:9.3f} ms device   {8.0 * T_M5 * n / (c_med * 1e-3) / 1e12:5.2f} TB/s of values read")

    def run_plan(plan, route, tile_min=0, out=None):
        return aggregate_block(y, lens, plan, n_series=n, t_out=T_M5, route=route, tile_min_members=tile_min, out=out)

    prefix_plan = None
    for name, column_of in plans.items():
        plan = hierarchy_plan_device(torch.from_numpy(column_of).to(dev))
        prefix_plan = prefix_plan or plan
        n_out, nnz = plan["n_out"], plan["nnz"]
        ld_out = (n_out + 63) // 64 * 64
        out = {"y": torch.zeros((T_M5, ld_out), dtype=torch.float64, device=dev), "present": torch.zeros((T_M5, ld_out), dtype=torch.uint8, device=dev)}
        alg = (nnz + n_out) * T_M5 * 8
        widths = np.diff(plan["col_offsets"].cpu().numpy())
        lines.append(f"{name}: {n_out:,d} output columns, nnz {nnz:,d}, widest column {int(widths.max()):,d} members, "
                     f"{int((widths >= 64).sum())} columns of 64 members or more; algorithmic bytes {alg / 1e9:.2f} GB")
        ref = None
        for route in ("lane", "tile", "auto"):
            med, mn = timed(lambda: run_plan(plan, route, out=out))
            bits = out["y"].clone()
            same = "" if ref is None else ("   same bits as the lane route" if bool((bits.view(torch.int64) == ref.view(torch.int64)).all()) else "   BITS DIFFER")
            ref = bits if ref is None else ref
            lines.append(f"    route {route:4s}: {med:9.3f} ({mn:9.3f}) ms   {alg / (med * 1e-3) / 1e12:5.2f} TB/s algorithmic{same}")
        # the numpy route: the block comes down, every level is summed with reduceat over the key-sorted columns, the sums go back up
        t0 = time.perf_counter()
        host = y[:, :n].cpu().numpy()
        sums = []
        for level in column_of:
            if np.all(np.diff(level) >= 0):
                starts = np.flatnonzero(np.diff(level, prepend=level[0] - 1))
                sums.append(np.add.reduceat(host, starts, axis=1))
            else:
                order = np.argsort(level, kind="stable")
                starts = np.flatnonzero(np.diff(level[order], prepend=level[order][0] - 1))
                sums.append(np.add.reduceat(host[:, order], starts, axis=1))
        up = torch.from_numpy(np.ascontiguousarray(np.concatenate(sums, axis=1))).to(dev)
        torch.cuda.synchronize()
        lines.append(f"    numpy route (download, np.add.reduceat per level, upload; one run, sums NOT in the operator's order): "
                     f"{(time.perf_counter() - t0) * 1e3:9.1f} ms")
        del up, host, sums, out
        print("\n".join(lines[-6:]), flush=True)

    lines.append("threshold of the automatic choice on the M5 prefix plan (columns with at least this many members take the tile route):")
    n_out = prefix_plan["n_out"]
    out = {"y": torch.zeros((T_M5, (n_out + 63) // 64 * 64), dtype=torch.float64, device=dev),
           "present": torch.zeros((T_M5, (n_out + 63) // 64 * 64), dtype=torch.uint8, device=dev)}
    for tile_min in (2, 64, 1024, 4096, 16384, 10**9):
        med, mn = timed(lambda: run_plan(prefix_plan, "auto", tile_min, out))
        lines.append(f"    tile_min_members {tile_min:>10,d}: {med:9.3f} ({mn:9.3f}) ms")
    del out
    lines.append("equal-width columns of w consecutive members (n_series // w columns), lane route against tile route:")
    crossover = None
    for w in (2, 4, 8, 16, 32, 64, 128, 256, 512, 1024, 2048, 4096):
        plan = hierarchy_plan_device(torch.from_numpy((s // w).astype(np.int32).reshape(1, -1)).to(dev))
        ld_out = (plan["n_out"] + 63) // 64 * 64
        out = {"y": torch.zeros((T_M5, ld_out), dtype=torch.float64, device=dev), "present": torch.zeros((T_M5, ld_out), dtype=torch.uint8, device=dev)}
        lane, _ = timed(lambda: run_plan(plan, "lane", out=out))
        tile, _ = timed(lambda: run_plan(plan, "tile", out=out))
        if crossover is None and tile < lane:
            crossover = w
        lines.append(f"    w = {w:5,d} ({plan['n_out']:6,d} columns): lane {lane:9.3f} ms   tile {tile:9.3f} ms   tile / lane = {tile / lane:5.2f}")
        del out
    lines.append(f"the tile route is the faster one from w = {crossover} on" if crossover else "the tile route never won")
    text = "\n".join(lines) + "\n"
    print(text)
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
