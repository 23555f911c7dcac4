"""GPU: PELT changepoint detection (csrc/pelt.hip) through every layer above the kernel -- the single C entry, the host-buffer
batch entry, the device-resident entry, device.pelt_block, api.pelt_batch and the scalar mirror -- against tests/pelt_ref.py.

The contract is equality: the changepoints, their number and the BITS of the cost.  tests/test_pelt_cpu.py
shows that the inputs (tests/pelt_cases.py) tell another tie rule and another summation order apart."""
import ctypes as C

import numpy as np
import pytest

import pelt_cases as K
import pelt_ref as R

pytestmark = pytest.mark.gpu

_REF = {}


def ref(name, v, ms, pen):
    """(changepoints, bits of the cost) of the restatement, computed once per (case, setting)."""
    key = (name, int(ms), R.bits(pen))
    if key not in _REF:
        cps, cost = (R.fast if len(v) <= 400 else R.literal)(v, ms, pen)
        _REF[key] = (cps, R.bits(cost))
    return _REF[key]


@pytest.fixture(scope="module")
def env(hiplib):
    import torch
    assert torch.cuda.is_available()
    from anofox_forecast_amd import api, device
    return api, device, hiplib, torch


def _single(lib, y, ms, pen):
    """anofox_ts_detect_changepoints: (changepoints, bits of the cost)."""
    L = lib.load()
    y = np.ascontiguousarray(y, dtype=np.float64)
    res = lib.ChangepointResult()
    C.memset(C.byref(res), 0, C.sizeof(res))
    err = lib.AnofoxError()
    dummy = np.zeros(1)
    assert L.anofox_ts_detect_changepoints(y.ctypes.data if len(y) else dummy.ctypes.data, len(y), int(ms), float(pen), C.byref(res),
                                           C.byref(err)), err.message
    k = res.n_changepoints
    assert bool(res.changepoints) == (k > 0)                        # NULL when there are none
    cps = [int(res.changepoints[i]) for i in range(k)]
    cost = R.bits(res.cost)
    L.anofox_free_changepoint_result(C.byref(res))
    assert not res.changepoints and res.n_changepoints == 0
    return cps, cost


def _batch(lib, series, ms, pen, masks=None):
    """anofox_hip_pelt_batch: per series (changepoints from the flags, count, bits of the cost)."""
    L = lib.load()
    n = len(series)
    ys = [np.ascontiguousarray(y, dtype=np.float64) for y in series]
    lens = np.array([len(y) for y in ys], dtype=np.uint64)
    dummy = np.zeros(1)
    vals = (C.c_void_p * n)(*[y.ctypes.data if len(y) else dummy.ctypes.data for y in ys])
    mptr = (C.c_void_p * n)(*[m.ctypes.data if m is not None and len(m) else None for m in masks]) if masks is not None else None
    total = int(lens.sum())
    flags = np.full(max(total, 1), 9, dtype=np.uint8)
    cnt = np.full(n, -99, dtype=np.int32)
    cost = np.full(n, -7.0)
    errs = (lib.AnofoxError * n)()
    berr = lib.AnofoxError()
    assert L.anofox_hip_pelt_batch(vals, mptr, lens.ctypes.data, n, int(ms), float(pen), flags.ctypes.data, cnt.ctypes.data, cost.ctypes.data,
                                   errs, C.byref(berr)), berr.message
    out, off = [], 0
    for i in range(n):
        m = int(lens[i])
        fl = flags[off:off + m]
        assert set(np.unique(fl)) <= {0, 1} and errs[i].code == lib.SUCCESS
        out.append(([int(k) for k in np.flatnonzero(fl)], int(cnt[i]), R.bits(cost[i])))
        off += m
    return out


def _device(lib, torch, series, ms, pen, pad_cols=0):
    """anofox_hip_pelt_device on a block prefilled with sentinels: (flags [T x ld], counts [ld], cost [ld]) as numpy."""
    n = len(series)
    ld = (n + 63) // 64 * 64 + pad_cols
    T = max(1, max(len(y) for y in series))
    yb = np.zeros((T, ld))
    for s, y in enumerate(series):
        yb[:len(y), s] = y
    dev = torch.device("cuda:0")
    y = torch.from_numpy(yb).to(dev)
    lens = torch.tensor([len(s) for s in series] + [0] * (ld - n), dtype=torch.int32, device=dev)
    flags = torch.full((T, ld), 9, dtype=torch.uint8, device=dev)
    counts = torch.full((ld,), -99, dtype=torch.int32, device=dev)
    cost = torch.full((ld,), -7.0, dtype=torch.float64, device=dev)
    err = lib.AnofoxError()
    torch.cuda.synchronize()
    assert lib.load().anofox_hip_pelt_device(y.data_ptr(), ld, lens.data_ptr(), n, T, int(ms), float(pen), flags.data_ptr(), counts.data_ptr(),
                                             cost.data_ptr(), None, C.byref(err)), err.message
    return flags.cpu().numpy(), counts.cpu().numpy(), cost.cpu().numpy()


def _check_block(cases, ms, pen, flags, counts, cost):
    n = len(cases)
    for s, (name, v, _, _) in enumerate(cases):
        cps, cbits = ref(name, v, ms, pen)
        m = len(v)
        assert [int(k) for k in np.flatnonzero(flags[:m, s] == 1)] == cps, (name, ms, pen)
        assert np.all((flags[:m, s] == 0) | (flags[:m, s] == 1)) and np.all(flags[m:, s] == 9), name      # rows beyond the length: untouched
        assert int(counts[s]) == len(cps) and R.bits(cost[s]) == cbits, (name, ms, pen, float(cost[s]))
    assert np.all(flags[:, n:] == 9) and np.all(counts[n:] == -99) and np.all(cost[n:] == -7.0)             # columns beyond n_series


MIXED = [(2, 0.0), (1, 1.0)]


@pytest.mark.parametrize("ms,pen", MIXED)
def test_mixed_ragged_batch_through_the_device_entry(env, ms, pen):
    """Every series of families (a)-(d) in ONE launch under one setting: ragged lengths 0-300, more than 130 workgroups, ties,
    noise, edges and non-finite values side by side; twice, with the same bits."""
    api, device, lib, torch = env
    cases = K.small_families()
    assert len(cases) > 130
    series = [v for _, v, _, _ in cases]
    first = _device(lib, torch, series, ms, pen)
    _check_block(cases, ms, pen, *first)
    again = _device(lib, torch, series, ms, pen)
    for a, b in zip(first, again):
        assert a.tobytes() == b.tobytes()


def _by_setting(cases):
    groups = {}
    for case in cases:
        groups.setdefault((int(case[2]), R.bits(case[3])), []).append(case)
    return list(groups.values())


def test_every_case_under_its_own_setting_through_the_batch_entry(env):
    """Families (a)-(d), each case with its own min_size and penalty: one anofox_hip_pelt_batch call per setting."""
    api, device, lib, torch = env
    for group in _by_setting(K.small_families()):
        ms, pen = group[0][2], group[0][3]
        got = _batch(lib, [v for _, v, _, _ in group], ms, pen)
        for (name, v, _, _), (cps, cnt, cbits) in zip(group, got):
            want = ref(name, v, ms, pen)
            assert (cps, cbits) == want and cnt == len(cps), (name, cps, want)


def test_single_entry_and_mirror(env):
    """anofox_ts_detect_changepoints and api._ts_detect_changepoints_pelt on families (a) and (d) and a slice of (b) and (c)."""
    api, device, lib, torch = env
    cases = K.family_a() + K.family_d() + K.family_b()[::7] + K.family_c()[::23]
    for name, v, ms, pen in cases:
        want = ref(name, v, ms, pen)
        assert _single(lib, v, ms, pen) == want, name
        r = api._ts_detect_changepoints_pelt(list(v), ms, pen)
        if len(v) < 2:
            assert r is None
        else:
            assert (r["changepoints"], R.bits(r["cost"])) == want and r["n_changepoints"] == len(want[0]), name
    for name, v, ms, cps, cost in K.RUST_UNIT:
        assert _single(lib, v, ms, 0.0) == (cps, R.bits(cost))
    # the defaults of the scalar without parameters: min_size 2, penalty 0.0
    v = K.RUST_UNIT[3][1]
    assert api._ts_detect_changepoints_pelt(v) == {"changepoints": [4], "n_changepoints": 1, "cost": 4.1588830833596715}
    assert api._ts_detect_changepoints_pelt(None) is None and api._ts_detect_changepoints_pelt([None, 3.0]) is None


def test_null_values_are_dropped_by_the_batch_entry_and_the_mirror(env):
    """A NULL is dropped before the series is packed: the batch entry with a validity mask, api.pelt_batch and the mirror give what
    the series without its NULLs gives, flags by position in the packed series."""
    api, device, lib, torch = env
    rng = np.random.default_rng(5)
    cases = K.family_b()[3::9] + K.family_c()[5::31]
    series, valids, packed = [], [], []
    for i, (name, v, _, _) in enumerate(cases):
        valid = rng.random(len(v)) > 0.2
        if i == 0:
            valid[:] = True
        if i == 1:
            valid[:] = False
        series.append(np.where(valid, v, 12345.0))
        valids.append(valid)
        packed.append(v[valid])
    valids[2] = None                                               # no mask: all valid
    packed[2] = series[2] = cases[2][1]
    ms, pen = 2, 0.0
    got = _batch(lib, series, ms, pen, masks=[api.validity_mask(m) if m is not None else None for m in valids])
    res = api.pelt_batch(series, ms, pen, valids=valids)
    for i, p in enumerate(packed):
        want = ref("dropped_%d" % i, p, ms, pen)
        cps, cnt, cbits = got[i]
        assert (cps, cbits) == want and cnt == len(cps), i
        assert (res[i]["changepoints"], R.bits(res[i]["cost"])) == want and res[i]["n_changepoints"] == len(want[0])
        assert len(res[i]["flags"]) == len(p)
        vals = [None if (valids[i] is not None and not valids[i][t]) else float(series[i][t]) for t in range(len(series[i]))]
        r = api._ts_detect_changepoints_pelt(vals, ms, pen)
        assert (r is None) if len(p) < 2 else ((r["changepoints"], R.bits(r["cost"])) == want)
    # api.pelt_batch without masks is the batch entry
    plain = api.pelt_batch([c[1] for c in cases], 1, 1.0)
    for (name, v, _, _), r in zip(cases, plain):
        assert (r["changepoints"], R.bits(r["cost"])) == ref(name, v, 1, 1.0)


def test_pelt_block_at_a_block_edge(env):
    """device.pelt_block on a block whose ld is not n_series: device tensors out, columns beyond n_series keep their fill."""
    api, device, lib, torch = env
    cases = (K.family_a() + K.family_b() + K.family_d())[:70]
    n, ld = len(cases), 128
    T = max(len(v) for _, v, _, _ in cases) + 3
    yb = np.zeros((T, ld))
    for s, (_, v, _, _) in enumerate(cases):
        yb[:len(v), s] = v
    dev = torch.device("cuda:0")
    lens = torch.tensor([len(v) for _, v, _, _ in cases] + [T] * (ld - n), dtype=torch.int32, device=dev)
    flags, counts, cost = device.pelt_block(torch.from_numpy(yb).to(dev), lens, 3, 0.0, n_series=n)
    assert flags.is_cuda and counts.is_cuda and cost.is_cuda and flags.dtype == torch.uint8 and tuple(flags.shape) == (T, ld)
    flags, counts, cost = flags.cpu().numpy(), counts.cpu().numpy(), cost.cpu().numpy()
    for s, (name, v, _, _) in enumerate(cases):
        cps, cbits = ref(name, v, 3, 0.0)
        assert [int(k) for k in np.flatnonzero(flags[:, s])] == cps and int(counts[s]) == len(cps) and R.bits(cost[s]) == cbits, name
    assert not flags[:, n:].any() and np.all(counts[n:] == -1) and np.all(np.isnan(cost[n:]))
    # the sentinel form of the same edge: ld = 64 k + 5
    sub = cases[:9]
    _check_block(sub, 3, 0.0, *_device(lib, torch, [v for _, v, _, _ in sub], 3, 0.0, pad_cols=5))


def test_series_above_the_lds_tile(env):
    """Family (e): 2,049 rows take the global workspace; beside it a short series of the same block takes the LDS kernel.  Run twice."""
    api, device, lib, torch = env
    (name, v, ms, pen), = K.family_e()
    want = ref(name, v, ms, pen)
    assert _single(lib, v, ms, pen) == want
    short = ("e_short", v[:2 * ms + 5], ms, pen)
    first = _device(lib, torch, [v, short[1]], ms, pen)
    _check_block([(name, v, ms, pen), short], ms, pen, *first)
    for a, b in zip(first, _device(lib, torch, [v, short[1]], ms, pen)):        # the workspace route twice: the same bits
        assert a.tobytes() == b.tobytes()


def test_lengths_above_t_rows_are_cut(env):
    api, device, lib, torch = env
    name, v, ms, pen = K.family_b()[40]
    T = len(v) - 7
    dev = torch.device("cuda:0")
    yb = np.zeros((T, 64))
    yb[:, 0] = v[:T]
    lens = torch.tensor([len(v)] + [0] * 63, dtype=torch.int32, device=dev)
    flags, counts, cost = device.pelt_block(torch.from_numpy(yb).to(dev), lens, ms, pen, n_series=1)
    cps, cbits = ref(name + "_cut", v[:T], ms, pen)
    assert [int(k) for k in np.flatnonzero(flags[:, 0].cpu().numpy())] == cps and R.bits(cost[0].item()) == cbits
