"""GPU: the data-preparation chain (dataprep.hip) against the restatement tests/dataprep_ref.py, `==` on bits for values, validity,
dates, figures, min and max.  Every case goes through the device entry (prepare_block) and the batch entry (prepare_batch);
the single entries exist per stage (anofox_ts_fill_gaps, anofox_ts_fill_nulls_*: no trimmer has one) and the mirrors per macro
(no macro interpolates), so a case runs through each of them where its stage has one, and all routes give the same bits.  The
device entry gets sentinel-filled output blocks: the ld padding and the rows past len_out must come back untouched."""
import numpy as np
import pytest

import dataprep_cases as DC
import dataprep_ref as R

pytestmark = pytest.mark.gpu

DAY = DC.US_PER_DAY
SENT_Y, SENT_V, SENT_D = -777.0, 7, -777
FILLS = ("none", "const", "forward", "backward", "mean", "interpolate")
TRIMS = ("leading", "trailing", "edge")
# every (n_series, t_rows) of the issue's two lists, paired so that each value appears
SHAPES = ((1, 1), (63, 2), (64, 3), (65, 16), (130, 17), (64, 33), (130, 70))


@pytest.fixture(scope="module")
def env(hiplib):
    import torch
    from anofox_forecast_amd import api, device
    assert torch.cuda.is_available()
    return api, device, hiplib, torch


def d64(s):
    return int(np.datetime64(s, "D").astype(np.int64)) * DAY


def make_block(series, torch):
    """series: [(dates or None, cells)] -> time-major tensors y, valid, dates (None without dates), lengths, and ld."""
    n = len(series)
    ld = (n + 63) // 64 * 64
    T = max(1, max(len(c) for _, c in series))
    y = np.zeros((T, ld))
    v = np.ones((T, ld), dtype=np.uint8)
    dated = any(d is not None for d, _ in series)
    d = np.zeros((T, ld), dtype=np.int64)
    ln = np.zeros(ld, dtype=np.int32)
    for s, (dt, cells) in enumerate(series):
        k = len(cells)
        ln[s] = k
        y[:k, s] = [0.0 if c is None else c for c in cells]
        v[:k, s] = [c is not None for c in cells]
        if dated:
            d[:k, s] = dt
    dev = "cuda:0"
    return (torch.from_numpy(y).to(dev), torch.from_numpy(v).to(dev), torch.from_numpy(d).to(dev) if dated else None,
            torch.from_numpy(ln).to(dev), ld)


def device_route(env, series, t_out=None, **opts):
    """prepare_block with sentinel-filled outputs, twice (the same bits), the sentinels checked; results as api.prepare_batch."""
    api, device, lib, torch = env
    n = len(series)
    y, v, d, ln, ld = make_block(series, torch)
    if t_out is None:
        cnt = device.prepare_block(y, ln, v, d, n_series=n, count_only=True, **opts)
        t_out = max(1, int(cnt["lengths"][:n].max().item()))
    runs = []
    for _ in range(2):
        out = {"y": torch.full((t_out, ld), SENT_Y, dtype=torch.float64, device="cuda:0"),
               "valid": torch.full((t_out, ld), SENT_V, dtype=torch.uint8, device="cuda:0"),
               "dates": torch.full((t_out, ld), SENT_D, dtype=torch.int64, device="cuda:0"),
               "lengths": torch.full((ld,), SENT_D, dtype=torch.int32, device="cuda:0")}
        r = device.prepare_block(y, ln, v, d, n_series=n, t_out=t_out, out=out, **opts)
        runs.append({k: out[k].cpu().numpy() for k in out} | {"figures": r["figures"].cpu().numpy(), "minmax": r["minmax"].cpu().numpy()})
    a, b = runs
    for k in a:
        assert np.array_equal(a[k].view(np.uint64) if a[k].dtype == np.float64 else a[k],
                              b[k].view(np.uint64) if b[k].dtype == np.float64 else b[k]), ("two runs differ", k)
    lo = a["lengths"]
    assert np.all(lo[n:] == SENT_D) and np.all(a["y"][:, n:] == SENT_Y) and np.all(a["valid"][:, n:] == SENT_V) and np.all(a["dates"][:, n:] == SENT_D)
    assert np.all(a["figures"][:, n:] == 0) and np.all(a["minmax"][:, n:] == 0.0)          # prepare_block zero-fills what it allocates
    res = []
    for s in range(n):
        k = int(lo[s])
        assert np.all(a["y"][k:, s] == SENT_Y) and np.all(a["valid"][k:, s] == SENT_V) and np.all(a["dates"][k:, s] == SENT_D), ("rows past len_out", s)
        if d is None:
            assert np.all(a["dates"][:, s] == SENT_D)
        assert set(np.unique(a["valid"][:k, s])) <= {0, 1}
        res.append({"values": a["y"][:k, s].copy(), "valid": a["valid"][:k, s].astype(bool), "dates": a["dates"][:k, s].copy() if d is not None else None,
                    "figures": dict(zip(DC.FIGURES, (int(x) for x in a["figures"][:, s]))), "min": float(a["minmax"][0, s]),
                    "max": float(a["minmax"][1, s])})
    return res, t_out


def ref_route(series, t_out=None, sort=False, **opts):
    opts = dict(opts)
    opts["ftype"] = opts.pop("frequency_type", "FIXED")
    return [DC.as_batch_result(R.prepare(d, c, sort=sort, t_out=t_out, **opts)) for d, c in series]


def batch_route(env, series, **opts):
    api = env[0]
    dated = any(d is not None for d, _ in series)
    vals = [np.array([0.0 if c is None else c for c in cells]) for _, cells in series]
    oks = [np.array([c is not None for c in cells], dtype=bool) for _, cells in series]
    return api.prepare_batch(vals, oks, [np.array(d, dtype=np.int64) for d, _ in series] if dated else None, **opts)


def assert_same(got, want, what):
    assert len(got) == len(want)
    for s, (g, w) in enumerate(zip(got, want)):
        assert DC.same_result(g, w), (what, s, g, w)


def seeded_series(n_series, t_rows, seed, dated=True):
    """Ragged series (0, 1 and t_rows rows in the first wave), a different NULL pattern in every lane, zeros at the edges, -0.0 and
    NaN among the values, dates on a daily grid with missing days."""
    rng = np.random.default_rng(seed)
    ln = DC.ragged_lengths(n_series, t_rows, rng)
    out = []
    for s in range(n_series):
        k = int(ln[s])
        vals = rng.choice([0.0, -0.0, 1.5, -2.25, float("nan"), 3.0, 7.125], size=k, p=[0.3, 0.05, 0.2, 0.1, 0.05, 0.15, 0.15])
        vals[:min(k, s % 5)] = 0.0                                  # leading zeros: another count in every lane
        vals[k - min(k, (s // 5) % 4):] = 0.0
        ok = DC.null_pattern(DC.NULL_PATTERNS[s % len(DC.NULL_PATTERNS)], k)
        dates = (np.cumsum(rng.choice([1, 1, 1, 2, 3], size=k)) + s) * DAY if dated else None
        out.append(([int(x) for x in dates] if dated else None, DC.to_cells(vals, ok)))
    return out


OPTION_SETS = ([dict(fill=f, fill_value=-1.5) for f in FILLS] + [dict(trim=t) for t in TRIMS]
               + [dict(gaps=True, frequency_micros=DAY), dict(gaps=True, frequency_micros=DAY, trim="edge", fill="const", fill_value=0.0),
                  dict(gaps=True, frequency_micros=DAY, trim="edge", fill="interpolate"), dict(trim="leading", fill="forward"),
                  dict(trim="trailing", fill="backward"), dict(gaps=True, frequency_micros=2 * DAY, trim="edge", fill="mean")])


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_shapes_device_and_batch(env, shape):
    series = seeded_series(shape[0], shape[1], 1000 + shape[0] * 100 + shape[1])
    for opts in OPTION_SETS:
        want = ref_route(series, **opts)
        got, t_out = device_route(env, series, **opts)
        assert_same(got, want, ("device", opts))
        assert t_out == max(1, max(len(w["values"]) for w in want))
        assert_same(batch_route(env, series, **opts), want, ("batch", opts))        # the dates ascend: the batch entry's sort moves nothing


def test_null_patterns_per_fill_mode(env):
    """Every pattern of the list at 70 rows (interior runs of 1, 2, 15, 16 and 17 rows cross the loader's block edge), adjacent lanes
    holding different patterns, without dates."""
    rng = np.random.default_rng(77)
    series = []
    for rep in range(5):
        for p in DC.NULL_PATTERNS:
            k = (70, 69, 40, 33, 18)[rep]
            series.append((None, DC.to_cells(rng.normal(5.0, 2.0, k), DC.null_pattern(p, k))))
    for f in FILLS:
        want = ref_route(series, fill=f, fill_value=2.5)
        assert_same(device_route(env, series, fill=f, fill_value=2.5)[0], want, ("device", f))
        assert_same(batch_route(env, series, fill=f, fill_value=2.5), want, ("batch", f))
    assert sum(w["figures"]["n_null_output"] for w in ref_route(series, fill="interpolate")) == 0


def test_single_entries_and_mirrors(env):
    """The reference's single entries on a strided subset (each is a batch of one) and the mirrors on all groups: the batch
    entry's bits."""
    api = env[0]
    series = seeded_series(65, 33, 4242)
    pick = list(range(0, 65, 5))
    for f in FILLS[1:]:
        want = ref_route(series, fill=f, fill_value=-1.5)
        for s in pick:
            cells = series[s][1]
            vals, ok = api.fill_nulls([0.0 if c is None else c for c in cells], [c is not None for c in cells], f, -1.5)
            assert np.array_equal(ok, want[s]["valid"]) and np.array_equal(vals.view(np.uint64), want[s]["values"].view(np.uint64)), (f, s)
    want = ref_route(series, gaps=True, frequency_micros=DAY)
    for s in pick:
        d, cells = series[s]
        gd, gv, gok = api.fill_gaps(d, [0.0 if c is None else c for c in cells], [c is not None for c in cells], DAY, "FIXED")
        assert np.array_equal(gd, want[s]["dates"]) and np.array_equal(gok, want[s]["valid"]), s
        assert np.array_equal(gv.view(np.uint64), want[s]["values"].view(np.uint64)), s
    # mirrors: BIGINT dates (the raw count is the frequency), one group per series, rows in date order
    grp = np.concatenate([np.full(len(c), s) for s, (_, c) in enumerate(series)]).astype(object)
    date = np.concatenate([np.array(d, dtype=np.int64) for d, _ in series])
    value = np.array([c for _, cells in series for c in cells], dtype=object)
    out = api.ts_fill_gaps_by(grp, date, value, str(DAY))
    flat = [x for w in want for x in DC.to_cells(w["values"], w["valid"])]
    assert R.same_values(out["value"], flat) and np.array_equal(out["date"], np.concatenate([w["dates"] for w in want]))
    for f in ("const", "forward", "backward", "mean"):
        fn = getattr(api, f"ts_fill_nulls_{f}_by")
        out = fn(grp, date, value, -1.5) if f == "const" else fn(grp, date, value)
        want = ref_route(series, fill=f, fill_value=-1.5)
        flat = [x for w in want for x in DC.to_cells(w["values"], w["valid"])]
        if f == "mean":                                            # AVG over no row is NULL where the core gives NaN
            flat = [None if (x is not None and x != x and not any(c is not None for c in series[int(g)][1])) else x
                    for x, g in zip(flat, out["id"])]
        assert R.same_values(out["filled_value"], flat), f
    for t in TRIMS:
        out = getattr(api, f"ts_drop_{t}_zeros_by")(grp, date, value)
        want = ref_route(series, trim=t)
        assert R.same_values(list(out["value"]), [x for w in want for x in DC.to_cells(w["values"], w["valid"])]), t
        assert np.array_equal(out["date"], np.concatenate([w["dates"] for w in want]))
    fig = ref_route(series)
    keep = api.ts_drop_zeros_by(grp, value)
    assert sorted(set(keep["id"])) == [s for s, w in enumerate(fig) if w["figures"]["n_nonzero_output"] > 0]
    keep = api.ts_drop_short_by(grp, 10)
    assert sorted(set(keep["id"])) == [s for s, w in enumerate(fig) if w["figures"]["n_input"] >= 10]
    keep = api.ts_drop_gappy_by(grp, value, 0.25)
    assert sorted(set(keep["id"])) == [s for s, w in enumerate(fig) if w["figures"]["n_input"] and w["figures"]["n_null_input"] / w["figures"]["n_input"] <= 0.25]
    keep = api.ts_drop_constant_by(grp, value)
    const = lambda w: w["figures"]["n_input"] > w["figures"]["n_null_input"] and (w["min"] == w["max"] or (w["min"] != w["min"] and w["max"] != w["max"]))
    assert sorted(set(keep["id"])) == [s for s, w in enumerate(fig) if w["figures"]["n_input"] and not const(w)]


def test_golden_statements_on_the_gpu(env):
    api = env[0]
    kats = DC.load_kats()
    for st in kats["statements"]:
        if "error" in st["expect"]:
            with pytest.raises(api.InvalidInputException):
                DC.run_statement(api, st, kats["tables"])
        else:
            DC.check_statement(DC.run_statement(api, st, kats["tables"]), st, kats["tables"])


GAP_CASES = {
    "no_gap": ("FIXED", 10, [0, 10, 20, 30]),
    "one_missing_step": ("FIXED", 10, [0, 10, 30]),
    "truncation": ("FIXED", 10, [0, 29, 58]),
    "closer_than_f": ("FIXED", 10, [0, 3, 5, 25]),
    "duplicates": ("FIXED", 10, [0, 0, 20, 20]),
    "jan31_mar31": ("MONTHLY", 0, [d64("2023-01-31"), d64("2023-03-31"), d64("2023-08-15") + 3600 * 10 ** 6]),
    "quarter_boundary": ("QUARTERLY", 0, [d64("2022-12-31"), d64("2023-07-01"), d64("2024-01-01")]),
    "year_boundary": ("YEARLY", 0, [d64("2021-12-31"), d64("2024-01-01"), d64("2024-12-31"), d64("2027-06-01")]),
    "pre_1970_negative_remainder": ("MONTHLY", 0, [d64("1969-03-15") - 1, d64("1970-04-01"), d64("1970-07-01")]),
    "pre_1970": ("MONTHLY", 0, [d64("1968-11-30"), d64("1969-03-01"), d64("1969-03-31")]),
}


@pytest.mark.parametrize("name", list(GAP_CASES), ids=list(GAP_CASES))
def test_gap_cases(env, name):
    api = env[0]
    ftype, f, dates = GAP_CASES[name]
    cells = [float(i + 1) if i != 1 else None for i in range(len(dates))]
    # the case beside series of other lengths, so that its lane is not alone in the wave
    series = [(dates[:k], cells[:k]) for k in (len(dates), 0, 1, 2)] + [(dates, cells)] * 3
    opts = dict(gaps=True, frequency_micros=f, frequency_type=ftype)
    want = ref_route(series, **opts)
    assert_same(device_route(env, series, **opts)[0], want, "device")
    assert_same(batch_route(env, series, **opts), want, "batch")
    gd, gv, gok = api.fill_gaps(dates, [0.0 if c is None else c for c in cells], [c is not None for c in cells], f, ftype)
    assert np.array_equal(gd, want[0]["dates"]) and np.array_equal(gok, want[0]["valid"])
    assert np.array_equal(gv.view(np.uint64), want[0]["values"].view(np.uint64))
    for fill in ("interpolate", "forward"):
        o = dict(opts, fill=fill, trim="edge")
        assert_same(device_route(env, series, **o)[0], ref_route(series, **o), ("device", fill))


def test_descending_rows_device_entry_does_not_sort(env):
    dates, cells = [50, 30, 31, 0, 40], [1.0, 2.0, None, 4.0, 5.0]
    series = [(dates, cells), (sorted(dates), cells)]
    opts = dict(gaps=True, frequency_micros=10)
    got, _ = device_route(env, series, **opts)
    assert_same(got, ref_route(series, **opts), "device")
    assert list(got[0]["dates"]) == [50, 30, 31, 0, 10, 20, 30, 40]        # only 0 -> 40 ascends by more than one step
    assert_same(batch_route(env, series, **opts), ref_route(series, sort=True, **opts), "batch sorts")


def test_overflow_beside_exact_fit_and_count_mode(env):
    api, device, lib, torch = env
    mk = lambda n_missing: ([0, 10 * (n_missing + 1), 10 * (n_missing + 2)], [1.0, None, 3.0])
    series = [mk(5), mk(6), mk(0), mk(5), ([], []), mk(40)]          # needs 8, 9, 3, 8, 0, 43 rows
    opts = dict(gaps=True, frequency_micros=10, fill="interpolate")
    y, v, d, ln, ld = make_block(series, torch)
    cnt = device.prepare_block(y, ln, v, d, n_series=len(series), count_only=True, **opts)
    assert cnt["y"] is None and list(cnt["lengths"][:6].cpu().numpy()) == [8, 9, 3, 8, 0, 43]
    fig = cnt["figures"].cpu().numpy()
    assert list(fig[0, :6] + fig[2, :6] - fig[3, :6] - fig[4, :6]) == [8, 9, 3, 8, 0, 43] and np.all(fig[7, :6] == 0)
    want_cnt = ref_route(series, **opts)
    for s in range(6):
        assert fig[:, s].tolist() == list(want_cnt[s]["figures"].values())
    got, _ = device_route(env, series, t_out=8, **opts)               # series 0 and 3 fit exactly, 1 and 5 do not
    want = ref_route(series, t_out=8, **opts)
    assert_same(got, want, "t_out = 8")
    assert [g["figures"]["status"] for g in got] == [0, 1, 0, 0, 0, 1] and len(got[1]["values"]) == 0 and len(got[0]["values"]) == 8
    assert got[1]["figures"]["n_input"] + got[1]["figures"]["n_inserted"] == 9
    full, t_out = device_route(env, series, **opts)                   # a full run sized from the count
    assert t_out == 43
    assert_same(full, want_cnt, "sized from the count")


def test_trim_cases(env):
    nan = float("nan")
    lanes = [(None, [0.0] * k + [1.0 + k, 0.0, 2.0] + [0.0] * (63 - k)) for k in range(64)]     # another shift in every lane of a wave
    special = [(None, [0.0, 0.0, 0.0]), (None, [1.0, 2.0, 3.0]), (None, [-0.0, 5.0, -0.0]), (None, [0.0, nan, 0.0]), (None, [None, 0.0, 4.0, 0.0, None]),
               (None, [None, None]), (None, [-0.0]), (None, [nan]), (None, []), (None, [0.0, None, 0.0])]
    series = lanes + special
    for t in TRIMS:
        for fill in ("none", "const", "interpolate"):
            opts = dict(trim=t, fill=fill, fill_value=0.0)
            want = ref_route(series, **opts)
            assert_same(device_route(env, series, **opts)[0], want, ("device", opts))
            assert_same(batch_route(env, series, **opts), want, ("batch", opts))
    edge = ref_route(series, trim="edge")
    assert [len(w["values"]) for w in edge[64:]] == [0, 3, 1, 1, 1, 0, 0, 1, 0, 0]
    assert [w["figures"]["n_trim_front"] for w in edge[:64]] == list(range(64))


def _raw_m5_like(n, seed):
    """Ragged daily series with removed days, leading zeros and NULLs, long enough after the chain for AutoETS at m = 7."""
    rng = np.random.default_rng(seed)
    out = []
    for s in range(n):
        k = int(rng.integers(60, 100))
        lead = int(rng.integers(0, 12))
        vals = np.round(np.abs(rng.normal(6.0, 3.0, k)) + 2.0 * np.sin(np.arange(k) * 2 * np.pi / 7), 3)
        vals[:lead] = 0.0
        keep = rng.random(k) > 0.05
        keep[[0, lead, k - 1]] = True
        ok = rng.random(k) > 0.05
        ok[[lead, k - 1]] = True
        dates = (np.arange(k) + 19000 + s) * DAY
        out.append(([int(x) for x in dates[keep]], DC.to_cells(vals[keep], ok[keep])))
    return out


def test_end_to_end_forecasts(env):
    """prepare_block -> DeviceBatch.set_block -> run equals the restatement's series through api.forecast_batch: forecasts,
    intervals and model names."""
    api, device, lib, torch = env
    n, h = 130, 7
    series = _raw_m5_like(n, 31)
    opts = dict(gaps=True, frequency_micros=DAY, trim="edge", fill="interpolate")
    y, v, d, ln, ld = make_block(series, torch)
    prep = device.prepare_block(y, ln, v, d, n_series=n, **opts)
    want = ref_route(series, **opts)
    clean = [w["values"] for w in want]
    assert all(w["valid"].all() for w in want) and prep["t_out"] == max(len(c) for c in clean)
    assert list(prep["lengths"][:n].cpu().numpy()) == [len(c) for c in clean]
    for model, kw in (("Naive", {}), ("SES", {}), ("AutoETS", {"seasonal_period": 7})):
        fo = lib.make_options(model, h, **kw)
        host, berr = api.forecast_batch(clean, fo)
        assert berr["ok"]
        b = device.DeviceBatch(n, prep["t_out"], fo, "cuda:0")
        try:
            assert b.ld == ld
            b.set_block(prep["y"], prep["lengths"])
            b.run()
            torch.cuda.synchronize()
            r = b.results()
            out = {k: r[k].cpu().numpy() for k in ("yhat", "lower", "upper", "status", "model_code")}
            names = [b.model_name(int(out["model_code"][s]), s) for s in range(n)]
        finally:
            b.close()
        for s in range(n):
            assert host[s]["ok"] and out["status"][s] == 0, (model, s, host[s].get("message"))
            assert np.array_equal(out["yhat"][s], host[s]["point"]), (model, s)
            assert np.array_equal(out["lower"][s], host[s]["lower"]) and np.array_equal(out["upper"][s], host[s]["upper"]), (model, s)
            assert names[s] == host[s]["model_name"], (model, s)


def test_interpolate_only_equals_pack_host(env):
    """The raw block with interpolate alone holds the bits of anofox_hip_batch_pack_host's host interpolation: a Naive batch with
    fitted values hands them back (fitted[t] = y[t - 1], the forecast is the last value)."""
    api, device, lib, torch = env
    rng = np.random.default_rng(99)
    series = []
    for s in range(130):
        k = int(rng.integers(3, 34))                               # the forecast entry wants three observations
        ok = DC.null_pattern(DC.NULL_PATTERNS[s % len(DC.NULL_PATTERNS)], k)
        if ok.any():
            series.append((None, DC.to_cells(rng.normal(20.0, 5.0, k), ok)))
    got, _ = device_route(env, series, fill="interpolate")
    vals = [np.array([0.0 if c is None else c for c in cells]) for _, cells in series]
    oks = [np.array([c is not None for c in cells], dtype=bool) for _, cells in series]
    host, berr = api.forecast_batch(vals, lib.make_options("Naive", 1, include_fitted=True), oks)
    assert berr["ok"]
    checked = 0
    for s, g in enumerate(got):
        if not host[s]["ok"]:
            continue
        packed = np.concatenate([host[s]["fitted"][1:], host[s]["point"][:1]])
        assert np.array_equal(packed.view(np.uint64), g["values"].view(np.uint64)), s
        assert host[s]["fitted"][0] == g["values"][0] or (host[s]["fitted"][0] != host[s]["fitted"][0] and g["values"][0] != g["values"][0])
        checked += 1
    assert checked == len(series) > 100
