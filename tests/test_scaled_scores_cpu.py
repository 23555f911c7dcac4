"""The scaled, weighted scores without a GPU: the restatement (tests/scaled_scores_ref.py) against hand-worked examples and exact
rational arithmetic, the tolerance of its sums, the host-only paths of the three C entries, and the mirror's host route."""
import ctypes as C
import math
import os
import re
import subprocess
import tempfile
from fractions import Fraction

import numpy as np
import pytest

import scaled_scores_cases as K
import scaled_scores_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "anofox_fcst_hip.h")
NEW_SYMBOLS = ("anofox_hip_scale_device", "anofox_hip_weighted_scores_device", "anofox_hip_wrmsse_batch")
U = 2.0 ** -53


def gamma(n):
    """The bound of recursive summation of n same-signed terms with one rounded product each (Higham, Accuracy and Stability of
    Numerical Algorithms, section 4.2): every term passes through at most n - 1 inexact additions -- an addition of an exact 0.0, such
    as an empty class of the wave sum, is exact -- and one product; two more roundings are allowed for."""
    return (n + 2) * U / (1.0 - (n + 2) * U)


# --------------------------------------------------------------------------------------------
# (a) the hand examples
# --------------------------------------------------------------------------------------------
def test_hand_example_of_the_scale():
    """y = [0, 0, 2, 4, 1, 3], lag 1, trimmed, tail_rows 2: t0 = 2; the differences from row 3 on are 2, -3, 2, so sq = 17, ab = 7 over
    n_terms = 3; the tail is 1 + 3."""
    r = R.scale_column([0.0, 0.0, 2.0, 4.0, 1.0, 3.0], 6, lag=1, trim=True, tail_rows=2)
    assert r == {"msd": 17.0 / 3.0, "mad": 7.0 / 3.0, "n_terms": 3.0, "tail": 4.0, "first": 2, "status": R.OK}
    # untrimmed: the two zero rows count -- differences 0, 2, 2, -3, 2
    r = R.scale_column([0.0, 0.0, 2.0, 4.0, 1.0, 3.0], 6, lag=1, trim=False, tail_rows=2)
    assert (r["msd"], r["mad"], r["n_terms"], r["first"]) == (21.0 / 5.0, 9.0 / 5.0, 5.0, 0)
    # lag 2 from t0 = 2: rows 4, 5: 1 - 2, 3 - 4
    r = R.scale_column([0.0, 0.0, 2.0, 4.0, 1.0, 3.0], 6, lag=2, trim=True, tail_rows=10)
    assert (r["msd"], r["mad"], r["n_terms"], r["tail"]) == (1.0, 1.0, 2.0, 10.0)
    # rows past the length are not read
    r = R.scale_column([0.0, 0.0, 2.0, 4.0, 1.0, 3.0, math.nan, 7.0], 6, lag=1, trim=True, tail_rows=2)
    assert (r["msd"], r["tail"], r["status"]) == (17.0 / 3.0, 4.0, R.OK)


def test_statuses_of_the_scale():
    nan, inf = math.nan, math.inf
    assert R.scale_column([], 0)["status"] == R.SHORT and R.scale_column([], 0)["tail"] == 0.0
    assert R.scale_column([5.0], 1)["status"] == R.SHORT and R.scale_column([5.0], 1)["n_terms"] == 0.0
    r = R.scale_column([0.0, -0.0, 0.0], 3)                                # all zero: t0 = n
    assert (r["first"], r["status"], r["n_terms"], r["tail"]) == (3, R.SHORT, -1.0, 0.0) and math.isnan(r["msd"])
    r = R.scale_column([0.0, 0.0, 4.0], 3)                                 # a single non-zero last row
    assert (r["first"], r["status"], r["n_terms"], r["tail"]) == (2, R.SHORT, 0.0, 4.0)
    r = R.scale_column([0.0, -0.0, 2.5, 2.5, 2.5], 5, tail_rows=2)          # constant after t0
    assert (r["first"], r["status"], r["msd"], r["mad"], r["tail"]) == (2, R.CONSTANT, 0.0, 0.0, 5.0)
    r = R.scale_column([1.0, nan, 2.0], 3)
    assert r["status"] == R.NAN and all(math.isnan(r[k]) for k in ("msd", "mad", "n_terms", "tail"))
    assert R.scale_column([nan], 1)["status"] == R.NAN                      # one row and a NaN: 2 takes precedence over 1
    r = R.scale_column([1.0, inf, 2.0, 3.0], 4)                            # +inf is a value: inf - 1 = inf, 2 - inf = -inf
    assert r["status"] == R.OK and r["msd"] == inf and r["mad"] == inf and r["tail"] == inf
    r = R.scale_column([1.0, 2.0, 4.0], 3, tail_rows=1, w=[nan, 5.0, 6.0])  # a NaN of w_src outside the tail
    assert (r["status"], r["tail"]) == (R.OK, 6.0)
    r = R.scale_column([1.0, 2.0, 4.0], 3, tail_rows=3, w=[nan, 5.0, 6.0])  # ... inside it
    assert r["status"] == R.NAN
    r = R.scale_column([1.0, 2.0, 4.0], 3, lag=3)                           # a lag that is at least the length
    assert (r["status"], r["n_terms"], r["tail"]) == (R.SHORT, 0.0, 7.0)


def _toy_wrmsse():
    """Two leaves and their total, columns (total, A, B), horizon 2, tail_rows 2, lag 1, trimmed.
        A      = [0, 2, 4, 1, 3]: t0 = 1, differences 2, -3, 2      -> msd 17/3,  tail 1 + 3 = 4
        B      = [1, 1, 3, 3, 5]: t0 = 0, differences 0, 2, 0, 2    -> msd 8/4 = 2, tail 3 + 5 = 8
        total  = [1, 3, 7, 4, 8]: differences 2, 4, -3, 4           -> msd 45/4,  tail 12
      forecasts A (2, 2) against (3, 1): mse 1; B (4, 4) against (4, 6): mse 2; total (6, 6) against (7, 7): mse 1.
      RMSSE: A sqrt(3/17), B sqrt(2/2) = 1, total sqrt(4/45).
      level 0 (the total alone): sqrt(4/45); level 1 (the leaves): (4 sqrt(3/17) + 8) / 12; WRMSSE: their mean."""
    A, B = [0.0, 2.0, 4.0, 1.0, 3.0], [1.0, 1.0, 3.0, 3.0, 5.0]
    train = np.array([[a + b, a, b] for a, b in zip(A, B)])
    fc = np.array([[6.0, 2.0, 4.0], [6.0, 2.0, 4.0]])
    act = np.array([[7.0, 3.0, 4.0], [7.0, 1.0, 6.0]])
    r = R.wrmsse(train, [5, 5, 5], None, fc, act, [(0, 1), (1, 3)], lag=1, trim=True, tail_rows=2)
    assert r["scale"][0].tolist() == [45.0 / 4.0, 17.0 / 3.0, 2.0] and r["scale"][3].tolist() == [12.0, 4.0, 8.0]
    assert r["first"].tolist() == [0, 1, 0] and r["status"].tolist() == [0, 0, 0] and r["mse"].tolist() == [1.0, 1.0, 2.0]
    assert r["rmsse"].tolist() == [math.sqrt(1.0 / (45.0 / 4.0)), math.sqrt(1.0 / (17.0 / 3.0)), 1.0]
    want = [math.sqrt(4.0 / 45.0), (4.0 * math.sqrt(3.0 / 17.0) + 8.0) / 12.0]
    assert np.allclose(r["score"], want, rtol=4 * 2.0 ** -52, atol=0.0) and r["left"].tolist() == [0, 0]
    assert math.isclose(r["wrmsse"], (want[0] + want[1]) / 2.0, rel_tol=4 * 2.0 ** -52)
    return train, fc, act, r


def test_two_level_toy_wrmsse():
    _toy_wrmsse()


def test_wave_sum_is_the_stated_order():
    rng = np.random.default_rng(1)
    for n in (0, 1, 63, 64, 65, 130, 497):
        t = rng.random(n) * 10.0 ** rng.integers(-8, 9, size=n).astype(np.float64)
        a = [0.0] * 64
        for i in range(n):
            a[i % 64] += float(t[i])
        w = a[0]
        for l in range(1, 64):
            w += a[l]
        assert R.wave_sum(t) == w
    assert R.wave_sum([]) == 0.0 and math.copysign(1.0, R.wave_sum([])) == 1.0


# --------------------------------------------------------------------------------------------
# (b) integer data: every sum is exact, whatever its order
# --------------------------------------------------------------------------------------------
def test_integer_data_sums_are_exact():
    rng = np.random.default_rng(2)
    for n, lag, trim, tail_rows in ((200, 1, True, 28), (200, 7, True, 28), (57, 1, False, 100), (3, 1, True, 1)):
        y = (rng.poisson(3.0, size=n) * (rng.random(n) < 0.7)).astype(np.float64) * float(rng.integers(1, 1000))
        y[:int(rng.integers(0, n // 2 + 1))] = 0.0
        t0, n_terms, sq, ab = R.scale_sums(y.tolist(), n, lag, trim)
        e0 = next((t for t in range(n) if y[t] != 0.0), n) if trim else 0
        esq = sum((Fraction(y[t]) - Fraction(y[t - lag])) ** 2 for t in range(e0 + lag, n))
        eab = sum(abs(Fraction(y[t]) - Fraction(y[t - lag])) for t in range(e0 + lag, n))
        assert esq < 2 ** 53 and (t0, n_terms) == (e0, n - e0 - lag)
        assert Fraction(sq) == esq and Fraction(ab) == eab
        assert Fraction(R.tail_sum(y.tolist(), n, tail_rows)) == sum(Fraction(v) for v in y[max(0, n - tail_rows):])
    # the wave sums of a range: integer weights and scaled losses
    for n in (1, 64, 65, 497):
        w = rng.integers(0, 1000, size=n).astype(np.float64)
        s = rng.integers(0, 1000, size=n).astype(np.float64)
        r = R.weighted_scores(s, np.ones(n), w, [(0, n)], R.RATIO)
        N, D = sum(Fraction(a) * Fraction(b) for a, b in zip(w, s)), sum(Fraction(a) for a in w)
        assert Fraction(float(r["weight_sum"][0, 0])) == D
        assert r["score"][0, 0] == float(N) / float(D) if D else math.isnan(r["score"][0, 0])


# --------------------------------------------------------------------------------------------
# (c) non-integer data: the sums within the derived bound of the exact value
# --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [2, 17, 200])
def test_serial_sums_within_the_bound(n):
    rng = np.random.default_rng(30 + n)
    for lag in (1, 7):
        if lag >= n:
            continue
        y = rng.normal(0.0, 1.0, size=n) * 10.0 ** rng.integers(-3, 4, size=n).astype(np.float64)
        t0, n_terms, sq, ab = R.scale_sums(y.tolist(), n, lag, False)
        d = [float(y[t]) - float(y[t - lag]) for t in range(lag, n)]
        esq, eab = sum(Fraction(v) * Fraction(v) for v in d), sum(abs(Fraction(v)) for v in d)
        g = gamma(n_terms)
        assert abs(Fraction(sq) - esq) <= Fraction(g) * esq and abs(Fraction(ab) - eab) <= Fraction(g) * eab
        w = np.abs(y)
        et = sum(Fraction(v) for v in w[max(0, n - 28):])
        assert abs(Fraction(R.tail_sum(w.tolist(), n, 28)) - et) <= Fraction(gamma(min(n, 28))) * et


@pytest.mark.parametrize("n", [5, 64, 65, 130, 497])
def test_wave_sums_within_the_bound(n):
    rng = np.random.default_rng(40 + n)
    w = rng.random(n) * 10.0 ** rng.integers(-2, 5, size=n).astype(np.float64)
    loss = rng.random(n) * 10.0 ** rng.integers(-3, 3, size=n).astype(np.float64)
    scale = rng.random(n) + 0.5
    for transform in (R.RATIO, R.ROOT):
        r = R.weighted_scores(loss, scale, w, [(0, n)], transform)
        s = r["scaled"][0]
        assert not np.isnan(s).any() and r["left"][0, 0] == 0
        N, D = sum(Fraction(a) * Fraction(b) for a, b in zip(w, s)), sum(Fraction(a) for a in w)
        g = Fraction(gamma(n))
        assert abs(Fraction(float(r["weight_sum"][0, 0])) - D) <= g * D
        got = Fraction(float(r["score"][0, 0]))
        # numerator and denominator within gamma each, the quotient one more rounding
        lo, hi = N * (1 - g) / (D * (1 + g)) * (1 - Fraction(U)), N * (1 + g) / (D * (1 - g)) * (1 + Fraction(U))
        assert lo <= got <= hi


def test_left_out_columns_and_invalid_ranges():
    loss, scale, weight, status = K.make_weighted_case(130, 9, 1)
    ranges = K.ranges_of(130)
    for transform in (R.RATIO, R.ROOT):
        r = R.weighted_scores(loss, scale, weight, ranges, transform, status, 130)
        assert r["left"][4].tolist() == [4] * 9 and np.isnan(r["score"][4]).all() and (r["weight_sum"][4] == 0.0).all()
        assert (r["left"][5:] == -1).all() and np.isnan(r["score"][5:]).all()
        for c in (11, 12, 13, 14, 15, 16, 23, 24, 25, 100, 101, 102, 103):
            assert np.isnan(r["scaled"][:, c]).all(), c
        assert not np.isnan(r["scaled"][:, 17]).any() and not np.isnan(r["scaled"][:, 18]).any()      # zero weights stay in
        assert np.isnan(r["scaled"][0, 19]) and not np.isnan(r["scaled"][1, 19])                     # per loss row
        assert np.isnan(r["scaled"][0, 21])
        assert np.isnan(r["scaled"][8, 20]) == (transform == R.ROOT)                                 # a negative loss has no root
        ok = ~np.isnan(r["score"][:4])
        assert ok.all()
        for k in range(9):                                                                          # the 1/4 over the valid ranges
            t = 0.0
            for g in range(4):
                t = t + float(r["score"][g, k])
            assert r["total"][k] == t / 4.0
    none = R.weighted_scores(loss, scale, weight, [(5, 5)], R.RATIO, status, 130)
    assert np.isnan(none["total"]).all() and math.isnan(none["total_mean"])


# --------------------------------------------------------------------------------------------
# (d) the ABI and the host-only paths of the three entries
# --------------------------------------------------------------------------------------------
def test_symbols_are_declared_and_exported(hiplib):
    L = hiplib.load()
    text = open(HEADER).read()
    for name in NEW_SYMBOLS:
        assert name in hiplib.EXPORTED_SYMBOLS and hasattr(L, name), name
        assert re.search(r"\bbool\s+" + name + r"\s*\(", text), name
    assert "Block 11" in text and "scaled_scores_ref.py" in text
    assert (hiplib.SCALE_OK, hiplib.SCALE_SHORT, hiplib.SCALE_NAN, hiplib.SCALE_CONSTANT) == (R.OK, R.SHORT, R.NAN, R.CONSTANT) == (0, 1, 2, 3)
    assert hiplib.SCALED_TRANSFORMS == {"ratio": R.RATIO, "root": R.ROOT} and hiplib.SCALED_MAX_LOSS == R.MAX_LOSS == 16
    for name, value in (("ANOFOX_SCALE_OK", 0), ("ANOFOX_SCALE_SHORT", 1), ("ANOFOX_SCALE_NAN", 2), ("ANOFOX_SCALE_CONSTANT", 3),
                        ("ANOFOX_SCALED_RATIO", 0), ("ANOFOX_SCALED_ROOT", 1)):
        assert re.search(name + r"\s*=\s*%d" % value, text), name


def _no_device(hiplib):
    return hiplib.load().anofox_hip_device_count() <= 0


_P = np.zeros(256)                                           # never dereferenced: every call below is refused first
_BIG = (1 << 30) + 1


def _scale(hiplib, L, err, **k):
    p = _P.ctypes.data
    return L.anofox_hip_scale_device(k.get("y", p), k.get("ld", 64), k.get("lengths", p), k.get("n", 10), k.get("t_rows", 5), None, k.get("lag", 1), True,
                                     k.get("tail_rows", 28), k.get("out", p), k.get("ld_out", 64), k.get("first", p), k.get("status", p), None,
                                     C.byref(err))


def _weighted(hiplib, L, err, **k):
    p = _P.ctypes.data
    return L.anofox_hip_weighted_scores_device(k.get("loss", p), k.get("ld", 64), k.get("n", 10), k.get("n_loss", 1), k.get("scale", p),
                                               k.get("weight", p), None, k.get("ranges", p), k.get("n_ranges", 1), k.get("transform", 0), None,
                                               k.get("score", p), p, p, k.get("total", p), None, C.byref(err))


def _wrmsse(hiplib, L, err, **k):
    n, h = k.get("n", 2), k.get("h", 2)
    series = [np.arange(1.0, 6.0)] * n
    ptrs = (C.c_void_p * max(n, 1))(*[a.ctypes.data for a in series])
    lens = (C.c_size_t * max(n, 1))(*k.get("lengths", [5] * n))
    fc, act = np.zeros((max(n, 1), 4)), np.zeros((max(n, 1), 4))
    co = k.get("column_of")
    co = None if co is None else np.ascontiguousarray(co, dtype=np.int32)
    n_out, ld = C.c_size_t(), C.c_size_t()
    st = np.zeros(256, dtype=np.int32)
    ok = L.anofox_hip_wrmsse_batch(ptrs if k.get("values", True) else None, lens, None, n, fc.ctypes.data if k.get("forecast", True) else None,
                                   act.ctypes.data, h, None if co is None else co.ctypes.data, 0 if co is None else co.shape[0], k.get("lag", 1),
                                   True, k.get("tail_rows", 28), k.get("ld", 64), None, None, None if k.get("sizing", False) else st.ctypes.data,
                                   None, None, None, None, C.byref(n_out), C.byref(ld), C.byref(err))
    return ok, n_out.value, ld.value


SCALE_ERRORS = (
    ({"lag": 0}, "lag is 0, the smallest lag is 1"),
    ({"tail_rows": 0}, "tail_rows is 0, the weight mass needs at least 1 row"),
    ({"lag": _BIG}, "lag 1073741825 exceeds the limit of 2^30 rows"),
    ({"tail_rows": _BIG}, "tail_rows 1073741825 exceeds the limit of 2^30 rows"),
)


def test_device_entries_refuse_bad_arguments_without_a_device(hiplib):
    L = hiplib.load()
    err = hiplib.AnofoxError()
    for kw, text in SCALE_ERRORS + (({"t_rows": _BIG}, "t_rows 1073741825 exceeds the limit of 2^30 rows"), ({"ld": 9}, "ld is smaller than n_cols"),
                                    ({"ld_out": 9}, "ld_out is smaller than n_cols"),
                                    ({"n": 1 << 31, "ld": 1 << 32, "ld_out": 1 << 32}, "n_cols exceeds the limit of 2^31 - 1")):
        assert not _scale(hiplib, L, err, **kw)
        assert err.code == hiplib.INVALID_INPUT and text in err.message.decode(), (kw, err.message)
    for kw, text in (({"n_loss": 0}, "n_loss is 0, a call needs at least 1 loss row"),
                     ({"n_loss": 17}, "n_loss 17 exceeds the limit of 16 loss rows per call"),
                     ({"transform": 2}, "transform 2 is unknown: 0 (loss / scale) or 1 (sqrt(loss / scale))"),
                     ({"transform": -1}, "transform -1 is unknown"),
                     ({"ld": 9}, "ld is smaller than n_cols"),
                     ({"n_ranges": 0}, "n_ranges is 0, a call needs at least 1 range"),
                     ({"n_ranges": 1 << 31}, "n_ranges exceeds the limit of 2^31 - 1"),
                     ({"n": 1 << 31, "ld": 1 << 32}, "n_cols exceeds the limit of 2^31 - 1")):
        assert not _weighted(hiplib, L, err, **kw)
        assert err.code == hiplib.INVALID_INPUT and text in err.message.decode(), (kw, err.message)
    for call, kw in ((_scale, {"y": None}), (_scale, {"lengths": None}), (_scale, {"out": None}), (_scale, {"first": None}), (_scale, {"status": None}),
                     (_weighted, {"loss": None}), (_weighted, {"scale": None}), (_weighted, {"weight": None}), (_weighted, {"ranges": None}),
                     (_weighted, {"score": None}), (_weighted, {"total": None})):
        assert not call(hiplib, L, err, **kw)
        assert err.code == hiplib.NULL_POINTER and err.message == b"Null pointer argument", kw
    if _no_device(hiplib):                                   # with valid arguments: the loud failure, never a CPU answer
        for call in (_scale, _weighted):
            assert not call(hiplib, L, err)
            assert err.code == hiplib.INTERNAL_ERROR and b"no CPU fallback" in err.message


def test_batch_entry_refuses_bad_requests_and_sizes_without_a_device(hiplib):
    L = hiplib.load()
    err = hiplib.AnofoxError()
    for kw, text in SCALE_ERRORS + (({"h": 0}, "horizon must be at least 1"), ({"h": _BIG}, "horizon 1073741825 exceeds the limit of 2^30 rows"),
                                    ({"lengths": [5, _BIG]}, "series 1 is longer than the limit of 2^30 rows"),
                                    ({"column_of": [[0, -2]]}, "a column_of entry is below -1"),
                                    ({"ld": 128}, "ld is not what the sizing call returns")):
        ok, _, _ = _wrmsse(hiplib, L, err, **kw)
        assert not ok and err.code == hiplib.INVALID_INPUT and text in err.message.decode(), (kw, err.message)
    for kw in ({"values": False}, {"forecast": False}):
        ok, _, _ = _wrmsse(hiplib, L, err, **kw)
        assert not ok and err.code == hiplib.NULL_POINTER, kw
    assert _wrmsse(hiplib, L, err, n=2, sizing=True) == (True, 2, 64)
    assert _wrmsse(hiplib, L, err, n=0, sizing=True) == (True, 0, 64)
    assert _wrmsse(hiplib, L, err, n=2, sizing=True, column_of=[[0, 0], [1, 2]]) == (True, 3, 64)
    assert _wrmsse(hiplib, L, err, n=70, sizing=True, column_of=K.make_hierarchy(70, 0)) == (True, 1 + 6 + 70, 128)
    if _no_device(hiplib):
        ok, _, _ = _wrmsse(hiplib, L, err)
        assert not ok and err.code == hiplib.INTERNAL_ERROR and b"no CPU fallback" in err.message


def test_python_entry_refuses_the_limits(hiplib):
    from anofox_forecast_amd import api
    train, fc, act = [np.arange(1.0, 9.0)] * 2, np.zeros((2, 3)), np.zeros((2, 3))
    for kw, text in (({"lag": 0}, "lag is 0"), ({"tail_rows": 0}, "tail_rows is 0"), ({"column_of": [[0, -3]]}, "below -1")):
        res, err = api.wrmsse_batch(train, fc, act, **kw)
        assert not err["ok"] and err["code"] == hiplib.INVALID_INPUT and text in err["message"], (kw, err)
    if _no_device(hiplib):
        res, err = api.wrmsse_batch(train, fc, act)
        assert not err["ok"] and err["code"] == hiplib.INTERNAL_ERROR and "no CPU fallback" in err["message"]
        assert np.isnan(res["rmsse"]).all() and res["ranges"].shape == (1, 2) and math.isnan(res["wrmsse"])


# --------------------------------------------------------------------------------------------
# (e) the mirror's host route
# --------------------------------------------------------------------------------------------
def _toy_tables(shuffled):
    A, B = [0.0, 2.0, 4.0, 1.0, 3.0], [1.0, 1.0, 3.0, 3.0, 5.0]
    rows = []
    for t in range(5):
        pair = [("A", A[t]), ("B", B[t])]
        if shuffled and t % 2:
            pair.reverse()                                   # no single series order reproduces this row order: the host route
        rows += [(np.datetime64("2024-01-01") + t, v, k) for k, v in pair]
    date = np.array([r[0] for r in rows], dtype="datetime64[D]")
    table = {"unique_id": np.array(["A", "A", "B", "B"], dtype=object),
             "date": np.array(["2024-01-06", "2024-01-07"] * 2, dtype="datetime64[D]"),
             "forecast": np.array([2.0, 2.0, 4.0, 4.0]), "actual": np.array([3.0, 1.0, 4.0, 6.0])}
    return date, np.array([r[1] for r in rows]), [np.array([r[2] for r in rows], dtype=object)], table


def test_mirror_host_route_gives_the_toy(hiplib):
    from anofox_forecast_amd import api
    _train, _fc, _act, want = _toy_wrmsse()
    date, value, ids, table = _toy_tables(shuffled=True)
    info = {}
    out = api.ts_wrmsse_by(date, value, ids, table, {"tail_rows": 2}, info=info)
    assert info["route"] == "host"
    assert out["level"].tolist() == [0, 1, -1] and out["n_series"].tolist() == [1, 2, 3] and out["left_out"].tolist() == [0, 0, 0]
    assert R.same_bits(out["score"], [want["score"][0], want["score"][1], want["wrmsse"]]).all()
    assert info["unique_id"].tolist() == ["AGGREGATED", "A", "B"] and R.same_bits(info["rmsse"], want["rmsse"]).all()
    # a leaf whose forecasts are missing leaves its level with the other leaf, and drops every step of the total
    table["forecast"][:2] = np.nan
    out = api.ts_wrmsse_by(date, value, ids, table, {"tail_rows": 2})
    assert out["left_out"].tolist() == [1, 1, 2] and math.isnan(out["score"][0]) and out["score"][1] == 1.0 and out["score"][2] == 1.0
    with pytest.raises(api.InvalidInputException, match="not a leaf"):
        api.ts_wrmsse_by(date, value, ids, dict(table, unique_id=np.array(["A", "A", "B", "C"], dtype=object)))


def test_mirror_host_restatement_equals_the_definition(hiplib):
    from anofox_forecast_amd import api
    rng = np.random.default_rng(5)
    n, T, h = 70, 40, 5
    train = rng.normal(0.0, 1.0, size=(T, n)) * 10.0 ** rng.integers(-2, 3, size=n).astype(np.float64)
    train[:7, ::3] = 0.0
    train[:, 4] = 1.5
    train[9, 6] = np.nan
    w = np.abs(train) * (rng.random(n) + 0.5)
    fc, act = rng.normal(size=(h, n)), rng.normal(size=(h, n))
    act[2, 8], fc[:, 9] = np.nan, np.nan
    ranges = [(0, 1), (1, 66), (66, 70), (3, 3)]
    for lag, trim, tail_rows, wb in ((1, True, 28, None), (7, False, 3, w)):
        want = R.wrmsse(train, [T] * n, wb, fc, act, ranges, lag, trim, tail_rows)
        cols = lambda b: [b[:, c].tolist() for c in range(n)]
        rmsse, score, left, total = api._wrmsse_host(cols(train), cols(train if wb is None else wb), cols(fc), cols(act), ranges, lag, trim, tail_rows)
        assert R.same_bits(rmsse, want["rmsse"]).all() and R.same_bits(score, want["score"]).all()
        assert list(left) == want["left"].tolist() and R.same_bits([total], [want["wrmsse"]]).all()


def test_host_scaled_scores_plan_under_sanitizers():
    """csrc/host_scaled_scores_plan.hpp -- the argument checks of the three entries and the column ranges of the WRMSSE chain --
    compiled on its own (no HIP) as a stand-alone program and run under ASan + UBSan (tests/c_abi/scaled_scores_san.cpp)."""
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "scaled_scores_san")
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                               os.path.join(ROOT, "tests", "c_abi", "scaled_scores_san.cpp"), "-o", exe])
        r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and r.stdout.startswith("scaled_scores_san: ok"), (r.stdout, r.stderr[-3000:])


def test_the_restatement_is_independent():
    pkg = os.path.join(ROOT, "anofox-forecast_amd")
    for base, _dirs, files in os.walk(pkg):
        for f in files:
            if f.endswith(".py"):
                assert "scaled_scores_ref" not in open(os.path.join(base, f), errors="replace").read(), f
    for f in ("scaled_scores_ref.py", "scaled_scores_cases.py"):
        text = open(os.path.join(ROOT, "tests", f)).read()
        assert "anofox_forecast_amd" not in text and "oracle" not in text, f
        assert not re.search(r"^\s*(import|from)\s+(path_scores_ref|paths_ref|metrics_ref|hierarchy_ref)", text, re.M), f
