"""GPU: ts_aggregate_hierarchy on the device -- anofox_hip_hierarchy_device (lane route, tile route, automatic), anofox_hip_hierarchy_batch,
device.aggregate_block and the api mirrors -- against the pure-Python restatement tests/hierarchy_ref.py.  The contract (DESIGN.md
section 3) is equality of bits with the operator's chain ((0.0 + v_a) + v_b) + ... in row order: every comparison is == on the bit
patterns; only the payload of a NaN is exempt (the sign of a zero is not).  The cases (tests/hierarchy_cases.py) are chosen so that an
order-agnostic sum cannot pass."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import hierarchy_cases as HC
import hierarchy_ref as R

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
Y_SENTINEL, P_SENTINEL, LEN_SENTINEL, FIRST_SENTINEL = -777.25, 0xAB, -5, -99
ROUTES = ("lane", "tile", "auto")


@pytest.fixture(scope="module")
def env(hiplib):
    import torch
    assert torch.cuda.is_available()
    L = hiplib.load()
    from anofox_forecast_amd import api, device
    return {"torch": torch, "L": L, "lib": hiplib, "api": api, "device": device, "dev": torch.device("cuda:0")}


def _device_entry(env, case, route, t_out, pad=37, pad_out=7, tile_min=0, members=None, offsets=None):
    """anofox_hip_hierarchy_device on a padded source block into sentinel-filled padded outputs; returns host copies."""
    torch, L, lib, dev = env["torch"], env["L"], env["lib"], env["dev"]
    y, valid, present, lengths, first = HC.pack(case, pad=pad)
    n_out = case["n_out"]
    ld_out = (n_out + 63) // 64 * 64 + pad_out
    up = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    ty, tv, tp, tl, tf = up(y), up(valid), up(present), up(lengths), up(first)
    to, tm = up(case["offsets"] if offsets is None else offsets), up(case["members"] if members is None else members)
    yo = torch.full((max(t_out, 1), ld_out), Y_SENTINEL, dtype=torch.float64, device=dev)
    po = torch.full((max(t_out, 1), ld_out), P_SENTINEL, dtype=torch.uint8, device=dev)
    lo = torch.full((ld_out,), LEN_SENTINEL, dtype=torch.int32, device=dev)
    fo = torch.full((ld_out,), FIRST_SENTINEL, dtype=torch.int64, device=dev)
    opts = lib.make_hierarchy_options(route, tile_min)
    err = lib.AnofoxError()
    ptr = lambda t: None if t is None else t.data_ptr()
    torch.cuda.synchronize()
    ok = L.anofox_hip_hierarchy_device(ty.data_ptr(), ptr(tv), ptr(tp), y.shape[1], tl.data_ptr(), tf.data_ptr(), case["n_series"], y.shape[0],
                                       to.data_ptr(), tm.data_ptr(), n_out, int(tm.numel()), C.byref(opts), C.sizeof(opts), t_out,
                                       yo.data_ptr() if t_out else None, po.data_ptr() if t_out else None, ld_out, lo.data_ptr(),
                                       fo.data_ptr(), None, C.byref(err))
    assert ok, err.message
    torch.cuda.synchronize()
    return yo.cpu().numpy(), po.cpu().numpy(), lo.cpu().numpy(), fo.cpu().numpy()


def _check_block(name, got, t_out, ld_out):
    """Bits of the whole padded output: cells, zeros past the lengths, untouched padding columns."""
    y, p, lens, first = got
    n_out = HC.all_cases()[name]["n_out"]
    ey, ep, el, ef = HC.expected_block(name, t_out, ld_out, Y_SENTINEL, P_SENTINEL)
    assert lens[:n_out].tolist() == el.tolist() and (lens[n_out:] == LEN_SENTINEL).all()
    assert first[:n_out].tolist() == ef.tolist() and (first[n_out:] == FIRST_SENTINEL).all()
    assert (p == ep).all()
    same = R.same_bits(y, ey)
    assert same.all(), f"{name}: {int((~same).sum())} cells differ, first at {np.argwhere(~same)[0].tolist()}"


@pytest.mark.parametrize("name", HC.CASE_NAMES)
def test_device_entry_every_route_bit_for_bit(env, name):
    case = HC.all_cases()[name]
    t_out = max(k[1] for k in HC.expected(name)) + 3            # rows past the longest column: zeros
    ld_out = (case["n_out"] + 63) // 64 * 64 + 7
    first_run = {}
    for route in ROUTES:
        got = _device_entry(env, case, route, t_out)
        _check_block(name, got, t_out, ld_out)
        first_run[route] = got[0]
    for route in ROUTES:                                        # a second run gives identical bits
        again = _device_entry(env, case, route, t_out)[0]
        assert (again.view(np.uint64) == first_run[route].view(np.uint64)).all()


def test_automatic_route_at_every_threshold(env):
    # the switch between the two routes at 1, 2, 63, 64, 65, 129 and above every width: the same bits wherever it lies
    name = "widths_T65_ragged"
    case = HC.all_cases()[name]
    t_out = max(k[1] for k in HC.expected(name))
    for tile_min in (1, 2, 63, 64, 65, 129, 201):
        _check_block(name, _device_entry(env, case, "auto", t_out, tile_min=tile_min), t_out, (case["n_out"] + 63) // 64 * 64 + 7)


def test_sizing_call_writes_lengths_and_first_only(env):
    for name in ("widths_T130_ragged", "masks"):
        case = HC.all_cases()[name]
        y, p, lens, first = _device_entry(env, case, "auto", 0)
        _ey, _ep, el, ef = HC.expected_block(name, 1, y.shape[1])
        assert (y == Y_SENTINEL).all() and (p == P_SENTINEL).all()
        assert lens[:case["n_out"]].tolist() == el.tolist() and first[:case["n_out"]].tolist() == ef.tolist()
        assert (lens[case["n_out"]:] == LEN_SENTINEL).all() and (first[case["n_out"]:] == FIRST_SENTINEL).all()


def test_masks_zero_signs_and_empty_columns(env):
    case = HC.all_cases()["masks"]
    cols = HC.expected("masks")
    t_out = max(k[1] for k in cols)
    y, p, lens, first = _device_entry(env, case, "auto", t_out)
    h0, h1 = case["hole_rows"]
    for c, (f, n, _v, _pr) in enumerate(cols):                   # the hole inside every live column's span
        if n:
            assert f < h0 and f + n > h1
            assert (p[h0 - f:h1 - f, c] == 0).all() and (y[h0 - f:h1 - f, c].view(np.uint64) == 0).all()
    nz = case["negzero_column"]
    even = y[:lens[nz]:2, nz]                                    # the single member holds -0.0 in its even rows: +0.0 comes out
    assert lens[nz] > 0 and (p[:lens[nz]:2, nz] == 1).any() and (even.view(np.uint64) == 0).all()
    for c in (case["absent_column"], case["empty_column"]):
        assert lens[c] == 0 and first[c] == 0 and (p[:, c] == 0).all() and (y[:, c].view(np.uint64) == 0).all()
    # a NULL value: the row exists and adds 0.0 (the source block holds NaN in every NULL slot)
    assert not np.isnan(y[:, :case["n_out"]]).any()


def test_a_plan_the_device_cannot_follow_is_marked_not_cut(env):
    # a member outside [0, n_series) and offsets that leave the plan: length -1, an empty column, the other columns as before
    name = "widths_T2_equal"
    case = HC.all_cases()[name]
    members = case["members"].copy()
    offsets = case["offsets"].copy()
    bad = next(c for c in range(case["n_out"]) if offsets[c + 1] - offsets[c] == 65)
    members[offsets[bad] + 64] = case["n_series"] + 1000
    for route in ROUTES:
        y, p, lens, first = _device_entry(env, case, route, 2, members=members)
        ey, ep, el, ef = HC.expected_block(name, 2, y.shape[1], Y_SENTINEL, P_SENTINEL)
        el[bad], ef[bad], ey[:, bad], ep[:, bad] = -1, 0, 0.0, 0
        assert lens[:case["n_out"]].tolist() == el.tolist() and first[:case["n_out"]].tolist() == ef.tolist()
        assert (p == ep).all() and R.same_bits(y, ey).all()


def _batch(env, case, route):
    res, err = env["api"].hierarchy_batch(case["series"], case["column_of"], first=case["first"], valids=case["valids"],
                                          presents=case["presents"], route=route)
    assert err["ok"], err
    return res


@pytest.mark.parametrize("name", ["widths_T65_ragged", "widths_T257_equal", "masks", "nonfinite", "prefix"])
def test_batch_entry_bit_for_bit(env, name):
    case = HC.all_cases()[name]
    for route in ROUTES:
        res = _batch(env, case, route)
        assert res["n_out"] == case["n_out"] and res["t_out"] == max(max(k[1] for k in HC.expected(name)), 1)
        ey, ep, el, ef = HC.expected_block(name, res["t_out"], res["y"].shape[1])
        assert res["lengths"].tolist() == el.tolist() and res["first"].tolist() == ef.tolist()
        assert (res["present"] == ep).all() and R.same_bits(res["y"], ey).all()
        assert (_batch(env, case, route)["y"].view(np.uint64) == res["y"].view(np.uint64)).all()


@pytest.mark.parametrize("name", ["widths_T64_ragged", "masks", "prefix"])
def test_aggregate_block_bit_for_bit(env, name):
    torch, device, dev = env["torch"], env["device"], env["dev"]
    case = HC.all_cases()[name]
    y, valid, present, lengths, first = HC.pack(case, pad=64 - case["n_series"] % 64 + 5)
    up = lambda a: None if a is None else torch.from_numpy(a).to(dev)
    co = up(case["column_of"])
    plan = device.hierarchy_plan_device(co)
    assert plan["n_out"] == case["n_out"] and plan["col_offsets"].cpu().tolist() == case["offsets"].tolist()
    assert plan["members"].cpu().tolist() == case["members"].tolist()
    for route, arg in (("auto", co), ("lane", plan), ("tile", co)):
        r = device.aggregate_block(up(y), up(lengths), arg, first=up(first), valid=up(valid), present=up(present), n_series=case["n_series"],
                                   route=route)
        t_out, ld_out = r["t_out"], r["y"].shape[1]
        assert ld_out == (case["n_out"] + 63) // 64 * 64 and r["n_out"] == case["n_out"]
        ey, ep, el, ef = HC.expected_block(name, t_out, ld_out)
        assert r["lengths"].cpu().numpy()[:case["n_out"]].tolist() == el.tolist()
        assert r["first"].cpu().numpy()[:case["n_out"]].tolist() == ef.tolist()
        assert (r["present"].cpu().numpy() == ep).all() and R.same_bits(r["y"].cpu().numpy(), ey).all()


def test_aggregate_block_refuses_a_marked_column(env):
    torch, device, dev = env["torch"], env["device"], env["dev"]
    y = torch.zeros((4, 64), dtype=torch.float64, device=dev)
    lengths = torch.full((64,), 4, dtype=torch.int32, device=dev)
    first = torch.zeros(64, dtype=torch.int64, device=dev)
    first[1] = 2**30                                             # column 0 would span 2^30 + 4 rows
    co = torch.zeros((1, 64), dtype=torch.int32, device=dev)
    with pytest.raises(ValueError, match="2\\^30"):
        device.aggregate_block(y, lengths, co, first=first)


def test_chain_into_the_batch_layer(env):
    """aggregate_block on a key-sorted block -> DeviceBatch.set_block as it is; Naive and SES forecasts of every level equal those of
    the host route fed the restatement's series."""
    torch, device, api, lib, dev = env["torch"], env["device"], env["api"], env["lib"], env["dev"]
    case = HC.all_cases()["prefix"]
    y, _v, _p, lengths, first = HC.pack(case, pad=64 - case["n_series"], sentinel=0.0)
    r = device.aggregate_block(torch.from_numpy(y).to(dev), torch.from_numpy(lengths).to(dev), torch.from_numpy(case["column_of"]).to(dev),
                               n_series=case["n_series"])
    n_out, t_out, h = r["n_out"], r["t_out"], 3
    assert (n_out, t_out) == (53, 60) and bool((r["present"][:, :n_out] == 1).all())        # no hole: a block the batch layer takes
    want = [np.array(k[2]) for k in HC.expected("prefix")]
    for model in ("Naive", "SES"):
        opts = lib.make_options(model, h)
        b = device.DeviceBatch(n_out, t_out, opts, dev)
        b.set_block(r["y"], r["lengths"])
        b.run()
        torch.cuda.synchronize()
        res = b.results()
        got, status = res["yhat"].cpu().numpy(), res["status"].cpu().numpy()
        b.close()
        host, berr = api.forecast_batch(want, lib.make_options(model, h))
        assert berr["ok"] and (status == 0).all()
        for c in range(n_out):
            assert host[c]["ok"] and R.same_bits(got[c], host[c]["point"]).all(), (model, c)


def test_golden_statements_replay_through_the_mirrors(env):
    api = env["api"]
    with open(os.path.join(HERE, "golden", "hierarchy_sql.json")) as fh:
        golden = json.load(fh)
    routes = []

    def aggregate(date, value, ids, params, date_name, value_name):
        info = {}
        out = api.ts_aggregate_hierarchy(date, value, ids, params, date_name, value_name, info=info)
        routes.append(info["route"])
        return out
    fns = {"ts_aggregate_hierarchy": aggregate, "ts_combine_keys": api.ts_combine_keys, "ts_split_keys": api.ts_split_keys,
           "ts_validate_separator": api.ts_validate_separator}
    assert HC.run_pins(fns, golden) == []
    assert routes and set(routes) == {"gpu"}                     # every table of the two files is sorted: none fell back


@pytest.mark.parametrize("order", ["ids_date", "date_ids"])
def test_mirror_on_a_table_with_gaps_nulls_and_colliding_ids(env, order):
    """The operator-level restatement against the mirror's GPU route: leaves that miss dates (holes), NULL values, NULL ids, an id equal
    to the keyword (two levels share a cell: the row is added twice) and ids that hold the separator."""
    api = env["api"]
    rng = np.random.default_rng(21)
    leaves = [("EU", "S1", "a"), ("EU", "S1", "b"), ("EU", "S2", "AGGREGATED"), ("EU", "AGGREGATED", "AGGREGATED"), ("US", None, "c"),
              ("US", "S3|x", "d"), ("US|S3", "x", "d"), ("ZZ", "S9", "e")]
    rows = []
    for k, leaf in enumerate(leaves):
        for day in range(1, 15):
            if rng.random() < 0.25 and not (k == 0 and day in (1, 14)):
                continue
            v = None if rng.random() < 0.15 else float(HC.PALETTE[rng.integers(0, len(HC.PALETTE))])
            rows.append((leaf, day, v))
    rows.append((leaves[-1], None, 5.0))                          # a NULL date: dropped
    key = (lambda r: (r[1] is None, r[1] or 0, tuple(str(x) for x in r[0]))) if order == "date_ids" else \
          (lambda r: (tuple(str(x) for x in r[0]), r[1] is None, r[1] or 0))
    rows.sort(key=key)
    date = np.array(["NaT" if d is None else f"2024-03-{d:02d}" for _l, d, _v in rows], dtype="datetime64[D]")
    value = [v for *_, v in rows]
    ids = [[l[i] for l, *_ in rows] for i in range(3)]
    info = {}
    got = api.ts_aggregate_hierarchy(date, value, ids, {"separator": "|"}, "day", "qty", info=info)
    assert info["route"] == "gpu"
    us = [None if np.isnat(d) else int(d.astype(np.int64)) for d in date]
    want = R.aggregate(us, value, ids)
    assert list(got["unique_id"]) == [r[0] for r in want]
    assert [int(d.astype(np.int64)) for d in got["day"]] == [r[1] for r in want]
    assert R.same_bits(got["qty"], [r[2] for r in want]).all()
    again = api.ts_aggregate_hierarchy(date, value, ids, {"separator": "|"}, "day", "qty")
    assert (again["qty"].view(np.uint64) == got["qty"].view(np.uint64)).all()
