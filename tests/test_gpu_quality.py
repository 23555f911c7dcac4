"""GPU: the data quality entries (anofox_ts_data_quality, anofox_hip_quality_batch, anofox_hip_quality_device), device.quality_block
and the SQL mirrors of api.py against the restatement tests/quality_ref.py.  The contract is equality of
bits through every entry and on every run; a status-2 series (a NaN among its values) is compared by its status, its counts and the
NaN-ness of its five scores."""
import ctypes as C
import math
import random

import numpy as np
import pytest

import quality_cases as QC
import quality_ref as R

pytestmark = pytest.mark.gpu

SENTINEL = -777.0
ISENT = -555
PAD = 12345.0


@pytest.fixture(scope="module")
def api(hiplib):
    import torch
    assert torch.cuda.is_available()
    hiplib.load()
    from anofox_forecast_amd import api as A
    return A


@pytest.fixture(scope="module")
def expected():
    """The restatement's answers, computed once per series (keyed by the series' identity) and left unchanged."""
    memo = {}

    def get(series):
        key = id(series)
        if key not in memo:
            memo[key] = (series, R.data_quality(series))
        return memo[key][1]
    return get


def _device(lib, batch, extra_cols=37, t_extra=0):
    """anofox_hip_quality_device on torch tensors; the outputs start as a sentinel.  Returns (scores [5 x ld], figures [4 x ld])."""
    import torch
    L = lib.load()
    dev = "cuda:0"
    n = len(batch)
    T = max(1, max(len(s) for s in batch)) + t_extra
    ld = (n + extra_cols + 63) // 64 * 64
    y = np.full((T, ld), PAD)
    v = np.ones((T, ld), dtype=np.uint8)
    any_null = False
    for i, s in enumerate(batch):
        vals, ok = QC.split(s)
        y[:len(s), i] = vals
        v[:len(s), i] = ok
        any_null = any_null or not all(ok)
    lens = torch.from_numpy(np.array([len(s) for s in batch], dtype=np.int32)).to(dev)
    yd = torch.from_numpy(y).to(dev)
    vd = torch.from_numpy(v).to(dev) if any_null else None
    fp = torch.full((5, ld), SENTINEL, dtype=torch.float64, device=dev)
    it = torch.full((4, ld), ISENT, dtype=torch.int64, device=dev)
    err = lib.AnofoxError()
    torch.cuda.synchronize()
    ok = L.anofox_hip_quality_device(yd.data_ptr(), None if vd is None else vd.data_ptr(), ld, lens.data_ptr(), n, T, fp.data_ptr(),
                                     it.data_ptr(), None, C.byref(err))
    assert ok, err.message
    return fp.cpu().numpy(), it.cpu().numpy()


def _check_device(got, batch, expected, where=""):
    fp, it = got
    n = len(batch)
    bad = []
    for i, s in enumerate(batch):
        want, status = expected(s)
        if (it[0, i], it[1, i], it[2, i], it[3, i]) != (0, want["n_missing"], int(want["is_constant"]), status):
            bad.append((where, i, len(s), "figures", [int(x) for x in it[:, i]], want, status))
            continue
        for k, f in enumerate(R.FP_FIELDS):
            if not QC.same_bits(fp[k, i], want[f]):
                bad.append((where, i, len(s), f, float(fp[k, i]), want[f]))
    assert not bad, bad[:6]
    assert (fp[:, n:] == SENTINEL).all() and (it[:, n:] == ISENT).all()        # ld > n_series: the other columns are untouched


def _batch_entry(api, batch):
    return api.quality_batch([np.array(QC.split(s)[0], dtype=np.float64) for s in batch], [QC.split(s)[1] for s in batch])


def _check_dicts(got, batch, expected, where=""):
    bad = []
    for i, (g, s) in enumerate(zip(got, batch)):
        want, status = expected(s)
        if g["status"] != status or any(g[f] != want[f] for f in ("n_gaps", "n_missing", "is_constant")) or any(
                not QC.same_bits(g[f], want[f]) for f in R.FP_FIELDS):
            bad.append((where, i, len(s), g, want, status))
    assert not bad, bad[:4]


# --------------------------------------------------------------------------------------------
# lengths, widths, families
# --------------------------------------------------------------------------------------------
LENGTH_BATCHES = {False: QC.length_batch(False), True: QC.length_batch(True)}
FAMILY_BATCH = QC.family_batch()
WIDTH_BATCHES = {w: QC.width_batch(w) for w in QC.WIDTHS}


@pytest.mark.parametrize("nulls", [False, True], ids=["dense", "nulls"])
def test_lengths(hiplib, api, expected, nulls):
    """Every length of QC.LENGTHS in one block of 5,000 rows (the tile is 2,048: the last two take the workspace kernel), and the
    short ones again in a block of their own, whose tile is sized down to 128."""
    batch = LENGTH_BATCHES[nulls]
    _check_device(_device(hiplib, batch), batch, expected, "long block")
    short = [s for s in batch if len(s) <= 128]
    _check_device(_device(hiplib, short), short, expected, "tile 128")
    tiny = [s for s in batch if len(s) <= 8]
    _check_device(_device(hiplib, tiny), tiny, expected, "tile 64")
    _check_dicts(_batch_entry(api, batch), batch, expected, "batch entry")


@pytest.mark.parametrize("width", QC.WIDTHS)
def test_widths(hiplib, expected, width):
    """1, 63, 64, 65, 257 series of at most 140 rows: a tile of at most 256 words, 16 waves per workgroup, so the widths cross whole
    and partial workgroups; in a longer block (t_extra) the same series run with a tile of 1,024 (8 waves) and 2,048 (4 waves)."""
    batch = WIDTH_BATCHES[width]
    first = _device(hiplib, batch)
    _check_device(first, batch, expected, width)
    for t_extra in (600, 1900):
        again = _device(hiplib, batch, t_extra=t_extra)
        assert again[0].tobytes() == first[0].tobytes() and again[1].tobytes() == first[1].tobytes(), t_extra


def test_families(hiplib, api, expected):
    batch = [s for _, s in FAMILY_BATCH]
    names = [n for n, _ in FAMILY_BATCH]
    got = _device(hiplib, batch)
    _check_device(got, batch, expected)
    fp, it = got
    # the families are what they are named for
    status = dict(zip(names, it[3]))
    assert all(status[n] == 2 for n in names if n.startswith("nan/") and not n.endswith("/nulls"))
    assert sum(1 for n in names if status[n] == 2 and not n.startswith("nan/")) == 0
    assert status["nan/64"] == 2 and status["masked_nan"] == 0 and all(math.isnan(x) for x in fp[:, names.index("nan/64")])
    col = lambda n: {f: fp[k, names.index(n)] for k, f in enumerate(R.FP_FIELDS)}
    assert col("ar99/333")["behavioral_score"] == 0.8 and col("ar50/333")["behavioral_score"] == 1.0
    assert col("constant/100")["behavioral_score"] == 0.0 and it[2, names.index("constant/100")] == 1
    assert it[2, names.index("near_constant/100")] == 1 and it[2, names.index("two_values")] == 0
    assert col("all_null")["overall_score"] == 0.375 and it[2, names.index("all_null")] == 1 and it[1, names.index("all_null")] == 40
    assert col("one_value")["behavioral_score"] == 0.5 and it[1, names.index("one_value")] == 50
    assert col("spikes/333")["magnitude_score"] < 1.0
    assert all(fp[k, names.index("empty")] == 0.0 for k in range(5)) and it[2, names.index("empty")] == 0
    _check_dicts(_batch_entry(api, batch), batch, expected, "batch entry")


def test_same_bits_on_two_runs(hiplib):
    batch = LENGTH_BATCHES[True] + [s for _, s in FAMILY_BATCH]
    a, b = _device(hiplib, batch), _device(hiplib, batch)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


def test_length_above_t_rows_is_cut(hiplib, expected):
    import torch
    L = hiplib.load()
    rng = random.Random(3)
    s = QC.family(rng, "positive", 50)
    y = torch.from_numpy(np.array(s).reshape(50, 1).repeat(64, axis=1)).to("cuda:0")
    lens = torch.tensor([50, 80, 20] + [0] * 61, dtype=torch.int32, device="cuda:0")
    fp = torch.full((5, 64), SENTINEL, dtype=torch.float64, device="cuda:0")
    it = torch.full((4, 64), ISENT, dtype=torch.int64, device="cuda:0")
    err = hiplib.AnofoxError()
    assert L.anofox_hip_quality_device(y.data_ptr(), None, 64, lens.data_ptr(), 3, 50, fp.data_ptr(), it.data_ptr(), None, C.byref(err)), err.message
    fp = fp.cpu().numpy()
    assert fp[:, 0].tobytes() == fp[:, 1].tobytes()
    for i, part in ((0, s), (2, s[:20])):
        want, _ = R.data_quality(part)
        assert all(QC.same_bits(fp[k, i], want[f]) for k, f in enumerate(R.FP_FIELDS))


# --------------------------------------------------------------------------------------------
# every entry gives the same bits; errors
# --------------------------------------------------------------------------------------------
def test_every_entry_gives_the_same_bits(hiplib, api, expected):
    L = hiplib.load()
    batch = [s for s in LENGTH_BATCHES[True] if len(s) <= 2049] + [s for n, s in FAMILY_BATCH if n.endswith("/100") or "/" not in n]
    fp, it = _device(hiplib, batch)
    dicts = _batch_entry(api, batch)
    err = hiplib.AnofoxError()
    for i, s in enumerate(batch):
        vals, ok = QC.split(s)
        va = np.array(vals if vals else [0.0], dtype=np.float64)
        mask = api.validity_mask(ok) if ok else None
        r = hiplib.DataQualityResult()
        done = L.anofox_ts_data_quality(va.ctypes.data, None if mask is None else mask.ctypes.data, len(s), C.byref(r), C.byref(err))
        if it[3, i] == 2:
            assert not done and err.code == hiplib.COMPUTATION_ERROR and err.message.decode() == R.NAN_TEXT
            assert dicts[i]["status"] == 2
            continue
        assert done, err.message
        for k, f in enumerate(R.FP_FIELDS):
            assert QC.bits(getattr(r, f)) == QC.bits(fp[k, i]) == QC.bits(dicts[i][f]), (i, f)
        assert (r.n_gaps, r.n_missing, int(r.is_constant)) == (it[0, i], it[1, i], it[2, i]) == (
            dicts[i]["n_gaps"], dicts[i]["n_missing"], int(dicts[i]["is_constant"]))


def test_null_pointers_and_empty(hiplib):
    L = hiplib.load()
    err = hiplib.AnofoxError()
    r = hiplib.DataQualityResult()
    one = np.array([1.0, 2.0])
    assert not L.anofox_ts_data_quality(None, None, 2, C.byref(r), C.byref(err))
    assert err.code == hiplib.NULL_POINTER and err.message.decode() == "Null pointer argument"
    assert not L.anofox_ts_data_quality(one.ctypes.data, None, 2, None, C.byref(err)) and err.code == hiplib.NULL_POINTER
    assert not L.anofox_ts_data_quality(None, None, 0, C.byref(r), None)                      # no error struct: still refused
    assert L.anofox_ts_data_quality(one.ctypes.data, None, 0, C.byref(r), C.byref(err)) and err.code == 0
    assert [getattr(r, f) for f in R.FP_FIELDS] == [0.0] * 5 and (r.n_gaps, r.n_missing, r.is_constant) == (0, 0, False)
    # batch entry
    assert L.anofox_hip_quality_batch(None, None, None, 0, None, None, C.byref(err)) and err.code == 0
    lens = np.array([2], dtype=np.uint64)
    vals = (C.c_void_p * 1)(one.ctypes.data)
    res = (hiplib.DataQualityResult * 1)()
    assert not L.anofox_hip_quality_batch(None, None, lens.ctypes.data, 1, res, None, C.byref(err)) and err.code == hiplib.NULL_POINTER
    assert not L.anofox_hip_quality_batch(vals, None, None, 1, res, None, C.byref(err)) and err.code == hiplib.NULL_POINTER
    assert not L.anofox_hip_quality_batch(vals, None, lens.ctypes.data, 1, None, None, C.byref(err)) and err.code == hiplib.NULL_POINTER
    assert not L.anofox_hip_quality_batch((C.c_void_p * 1)(None), None, lens.ctypes.data, 1, res, None, C.byref(err)) and err.code == hiplib.NULL_POINTER
    assert L.anofox_hip_quality_batch(vals, None, lens.ctypes.data, 1, res, None, C.byref(err)), err.message    # no status array: allowed
    assert res[0].behavioral_score == 0.5 and res[0].is_constant is False
    # device entry
    import torch
    y = torch.zeros((4, 64), dtype=torch.float64, device="cuda:0")
    ln = torch.zeros(64, dtype=torch.int32, device="cuda:0")
    fp = torch.full((5, 64), SENTINEL, dtype=torch.float64, device="cuda:0")
    it = torch.full((4, 64), ISENT, dtype=torch.int64, device="cuda:0")
    args = [y.data_ptr(), None, 64, ln.data_ptr(), 1, 4, fp.data_ptr(), it.data_ptr(), None, C.byref(err)]
    for k in (0, 3, 6, 7):
        broken = list(args)
        broken[k] = None
        assert not L.anofox_hip_quality_device(*broken) and err.code == hiplib.NULL_POINTER, k
    broken = list(args)
    broken[4] = 65                                                                            # n_series > ld
    assert not L.anofox_hip_quality_device(*broken) and err.code == hiplib.INVALID_INPUT
    broken[4] = 0                                                                             # n_series == 0: nothing is written
    assert L.anofox_hip_quality_device(*broken) and err.code == 0
    assert (fp.cpu().numpy() == SENTINEL).all() and (it.cpu().numpy() == ISENT).all()


# --------------------------------------------------------------------------------------------
# the Python scalar and the table mirrors
# --------------------------------------------------------------------------------------------
KATS = QC.load_kats()
DAY0 = np.datetime64("2023-01-01", "D")


def _dates(days):
    return np.array([np.datetime64("NaT", "D") if d is None else DAY0 + d for d in days], dtype="datetime64[D]")


class ApiImpl:
    """The golden statements through the mirrors of api.py (day numbers become DATE values)."""

    def __init__(self, api):
        self.api = api

    def scalar(self, values):
        return self.api._ts_data_quality(values)

    def table(self, fn, group, date, value, **kw):
        return getattr(self.api, fn)(group, _dates(date), np.array(value, dtype=object), **kw)

    def summary(self, group, date, value, **kw):
        return self.api.ts_data_quality_summary(group, _dates(date), np.array(value, dtype=object), **kw)

    def agg(self, fn, ts, value):
        return getattr(self.api, fn)(_dates(ts), np.array(value, dtype=object))


@pytest.mark.parametrize("st", KATS["scalars"], ids=lambda st: f'{st["field"]}@{st["src"].split("/")[-1]}')
def test_golden_scalars(api, st):
    ok, value = QC.golden_scalar(ApiImpl(api), st)
    assert ok, (st["src"], value)


def test_golden_pairs_and_tables(api):
    impl = ApiImpl(api)
    for st in KATS["pairs"]:
        ok, value = QC.golden_pair(impl, st)
        assert ok, (st["src"], value)
    for st in KATS["table_statements"]:
        ok, value = QC.golden_table(impl, KATS, st)
        assert ok, (st["src"], value)


def _same(got, want, where):
    if isinstance(want, dict):
        assert isinstance(got, dict) and set(got) == set(want), where
        for k in want:
            _same(got[k], want[k], where + (k,))
    elif isinstance(want, (list, tuple)):
        assert len(got) == len(want), where
        for i, (a, b) in enumerate(zip(got, want)):
            _same(a, b, where + (i,))
    elif isinstance(want, float):
        assert got is not None and QC.same_bits(got, want), (where, got, want)
    else:
        assert got == want and type(got) is type(want), (where, got, want)


def test_mirrors_equal_the_restatement_on_random_grouped_rows(api):
    rng = random.Random(31)
    n_rows = 1500
    group = [f"g{rng.randrange(23)}" for _ in range(n_rows)]
    date = [None if rng.random() < 0.02 else rng.randrange(400) for _ in range(n_rows)]          # duplicates and NULL dates
    value = [None if rng.random() < 0.05 else round(rng.lognormvariate(2.0, 1.0), 2) for _ in range(n_rows)]
    for i in range(n_rows):
        if group[i] == "g3":
            value[i] = 7.0 if value[i] is not None else None                                    # a constant group
        if group[i] == "g4" and value[i] is not None and rng.random() < 0.05:
            value[i] = math.nan                                                                  # a group whose STRUCT is NULL
        if group[i] == "g5":
            value[i] = None                                                                      # an all-NULL group
    vcol, dcol = np.array(value, dtype=object), _dates(date)
    want = R.table(group, date, value)
    assert want["overall_score"][want["unique_id"].index("g4")] is None
    for fn in (api.ts_data_quality, api.ts_data_quality_by, api.anofox_fcst_ts_data_quality, api.anofox_fcst_ts_data_quality_by):
        _same(fn(group, dcol, vcol, 5, "1d"), want, (fn.__name__,))
    _same(api.ts_data_quality(group, dcol, vcol), want, ("defaults",))
    for fn in (api.ts_data_quality_summary, api.anofox_fcst_ts_data_quality_summary):
        _same(fn(group, dcol, vcol, 5), R.summary(group, date, value), (fn.__name__,))
    _same(api.ts_data_quality_summary([], _dates([]), np.array([], dtype=object)), R.summary([], [], []), ("no rows",))
    for g in ("g0", "g3", "g4", "g5"):
        rows = [i for i in range(n_rows) if group[i] == g]
        ts, vs = [date[i] for i in rows], [value[i] for i in rows]
        if g == "g4":                                                                            # std::sort of pairs with a NaN: no order to restate
            assert api.ts_data_quality_agg(_dates(ts), np.array(vs, dtype=object)) is None
            continue
        _same(api.ts_data_quality_agg(_dates(ts), np.array(vs, dtype=object)), R.agg(ts, vs), ("agg", g))
    assert api.anofox_fcst_ts_data_quality_agg is api.ts_data_quality_agg
    # the scalar: NULL list, empty list, NULL elements, a NaN
    assert api._ts_data_quality(None) is None and api._ts_data_quality([]) is None and api._ts_data_quality([1.0, math.nan]) is None
    for s in ([None], [1.0, None, 2.5], [3.0] * 40 + [None] * 3 + [9.0]):
        _same(api._ts_data_quality(s), R.scalar(s), ("scalar", len(s)))


# --------------------------------------------------------------------------------------------
# prepare -> quality -> filter -> forecast without leaving the device
# --------------------------------------------------------------------------------------------
def test_prepare_quality_forecast_chain(api, hiplib):
    import torch
    from anofox_forecast_amd import device
    rng = random.Random(77)
    n, T, ld, h = 70, 90, 128, 5
    raw = []
    for i in range(n):
        m = rng.randrange(20, T + 1)
        lead = rng.randrange(0, 6)
        body = QC.family(rng, ("poisson", "positive", "constant", "ar99", "spikes")[i % 5], m - lead)
        body[0] = body[0] if body[0] != 0.0 else 1.0                                             # the first row after the zeros is non-zero
        s = [0.0] * lead + body
        raw.append([None if (rng.random() < 0.05 and j > lead) else v for j, v in enumerate(s)])
    y = np.full((T, ld), PAD)
    v = np.ones((T, ld), dtype=np.uint8)
    for i, s in enumerate(raw):
        vals, ok = QC.split(s)
        y[:len(s), i] = vals
        v[:len(s), i] = ok
    dev = "cuda:0"
    lens = torch.tensor([len(s) for s in raw] + [0] * (ld - n), dtype=torch.int32, device=dev)
    prep = device.prepare_block(torch.from_numpy(y).to(dev), lens, torch.from_numpy(v).to(dev), n_series=n, trim="leading")
    q = device.quality_block(prep["y"], prep["lengths"], prep["valid"], n_series=n)
    scores, figures = q["scores"].cpu().numpy(), q["figures"].cpu().numpy()
    # the host route on the same raw series: drop the leading zeros by hand, then the batch entry
    trimmed = []
    for s in raw:
        k = 0
        while k < len(s) and s[k] is not None and s[k] == 0.0:
            k += 1
        trimmed.append(s[k:])
    assert [len(s) for s in trimmed] == prep["lengths"][:n].cpu().tolist()
    host = _batch_entry(api, trimmed)
    for i in range(n):
        want, status = R.data_quality(trimmed[i])
        assert status == 0 and figures[3, i] == 0 and figures[1, i] == host[i]["n_missing"] == want["n_missing"]
        assert figures[2, i] == int(host[i]["is_constant"]) == int(want["is_constant"])
        for k, f in enumerate(R.FP_FIELDS):
            assert QC.bits(scores[k, i]) == QC.bits(host[i][f]) == QC.bits(want[f]), (i, f)
    assert np.isnan(scores[:, n:]).all() and (figures[:, n:] == -1).all()
    # filter on the device: complete series that are not constant go on to a Naive forecast
    keep = ((q["figures"][3, :n] == 0) & (q["figures"][2, :n] == 0) & (q["figures"][1, :n] == 0) & (q["scores"][4, :n] >= 0.5)).nonzero().flatten()
    m = int(keep.numel())
    assert 0 < m < n
    t_out = int(prep["t_out"])
    b = device.DeviceBatch(m, t_out, hiplib.make_options("Naive", h))
    yk = torch.zeros((t_out, b.ld), dtype=torch.float64, device=b.device)
    yk[:, :m] = prep["y"][:, keep]
    lk = torch.zeros(b.ld, dtype=torch.int32, device=b.device)
    lk[:m] = prep["lengths"][keep]
    b.set_block(yk.contiguous(), lk)
    b.run()
    torch.cuda.synchronize()
    r = b.results()
    assert (r["status"].cpu().numpy()[:m] == 0).all()
    yhat = r["yhat"].cpu().numpy()
    for j, i in enumerate(keep.cpu().tolist()):
        assert (yhat[j, :h] == trimmed[i][-1]).all(), (i, yhat[j, :h], trimmed[i][-1])
    b.close()
