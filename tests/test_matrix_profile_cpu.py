"""CPU: the restatement of the reference's matrix_profile_period (tests/matrix_profile_ref.py): its two forms equal with ==, the
source's visiting order against the first minimum over ascending partners, the conditions the GPU case list must meet (cases where
comparing before the square root changes an index, cases with tied lags), hand-checked shapes; the struct layout and symbols against
the header; the argument errors that need no device; the operator mirrors with the GPU batch call replaced by the restatement; the
host header under ASan + UBSan as a stand-alone program; and the boundary that must not move: the method dispatch by name still
raises for 'matrix_profile'."""
import ctypes as C
import math
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import matrix_profile_cases as PC
import matrix_profile_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = [c for c in PC.CASES if c[7] == "plain" and c[2] <= 200]


def same(a, b):
    """== on every figure, NaN equal to NaN."""
    if isinstance(a, dict):
        return set(a) == set(b) and all(same(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    if isinstance(a, float) and a != a:
        return b != b
    return a == b


# --------------------------------------------------------------------------------------------
# the restatement
# --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", SMALL, ids=lambda c: c[0])
def test_two_forms_agree_and_the_order_is_free(case):
    v = PC.series(case)
    plain = R.matrix_profile_plain(v, case[5], case[6])
    assert same(plain, R.matrix_profile(v, case[5], case[6]))
    assert same(plain, R.matrix_profile(v, case[5], case[6], rows=7))              # another blocking of the pairs, the same bits
    mp, mpi = R.first_minimum_profile(v, case[5], case[6])
    assert same(mp, plain["mp"]) and mpi == plain["mpi"]
    assert plain["period"] == min(plain["tied_lags"]) if plain["tied_lags"] else math.isnan(plain["period"])
    assert len(plain["tied_lags"]) == plain["n_tied"]


def test_rule_and_errors():
    assert (R.subsequence(32), R.subsequence(1913), R.subsequence(100, 1), R.subsequence(100, 26), R.subsequence(2300, 10 ** 6)) == (4, 191, 4, 25, 575)
    assert (R.exclusion(4), R.exclusion(191), R.exclusion(191, 5)) == (1, 47, 5)
    assert (R.profile_len(31), R.profile_len(32), R.profile_len(1913)) == (0, 29, 1723)
    assert R.in_lds(2341) and not R.in_lds(2342) and R.in_lds(2203, 4) and not R.in_lds(2204, 4)
    for f in (R.matrix_profile_plain, R.matrix_profile):
        with pytest.raises(R.InsufficientData) as e:
            f(np.arange(31.0))
        assert str(e.value) == "Insufficient data: need at least 32 observations, got 31"
    assert all(R.profile_len(n, s) >= 25 for n in range(32, 400) for s in (None, 1, 9, 10 ** 9))       # the source's second check cannot be reached


def test_known_shapes():
    # a constant series: every std is EPSILON, every z and every distance 0.0, so every entry keeps its first admissible partner
    r = R.matrix_profile_plain(PC.family("constant", 90))
    m, excl, P = 9, 2, 82
    assert (r["subsequence_length"], r["exclusion"], len(r["mp"])) == (m, excl, P) and set(r["mp"]) == {0.0}
    assert r["mpi"] == [x + excl if x < excl else 0 for x in range(P)]
    assert math.isnan(r["period"]) and r["n_motifs"] == 0 and r["confidence"] == 0.0            # the threshold is 0.0: nothing is below it
    # exactly periodic: the nearest neighbour is at distance 0.0, one period away where that is outside the zone
    r = R.matrix_profile_plain(PC.family("periodic", 100, 7, 1))
    assert set(r["mp"]) == {0.0} and r["exclusion"] == 2 and r["mpi"][:10] == [7, 8, 9, 10, 11, 12, 13, 0, 1, 2]
    # no pair at all; ten finite values
    r = R.matrix_profile_plain(PC.series(PC.by_id("no_pair")), None, 1000)
    assert set(r["mp"]) == {math.inf} and set(r["mpi"]) == {0} and math.isnan(r["period"]) and (r["confidence"], r["n_motifs"]) == (0.0, 0)
    r = R.matrix_profile_plain(PC.series(PC.by_id("few_finite")), 4, 32)
    assert sum(math.isfinite(x) for x in r["mp"]) == 10 and len(r["mp"]) == 37
    # a NaN never updates: the subsequences that hold it keep +inf and index 0
    c = PC.by_id("nan")
    r = R.matrix_profile_plain(PC.series(c))
    bad = [i for i in range(len(r["mp"])) if i <= c[2] // 3 < i + r["subsequence_length"]]
    assert all(r["mp"][i] == math.inf and r["mpi"][i] == 0 for i in bad) and all(math.isfinite(r["mp"][i]) for i in range(len(r["mp"])) if i not in bad)
    assert not any(i in bad for i in r["mpi"][bad[-1] + 1:])
    # a seasonal series finds a multiple of its period
    r = R.matrix_profile(PC.family("seasonal", 150, 12, 4))
    assert r["period"] % 12 == 0 and r["confidence"] > 0.3


def test_conditions_on_the_gpu_case_list():
    """The GPU tests can tell a wrong reduction or a wrong tie rule only on inputs where it shows."""
    differs = [name for name in PC.SQUARED_DIFFERS
               if R.matrix_profile_plain(PC.series(PC.by_id(name)), *PC.by_id(name)[5:7], squared_compare=True)["mpi"]
               != R.matrix_profile_plain(PC.series(PC.by_id(name)), *PC.by_id(name)[5:7])["mpi"]]
    assert len(differs) >= 3 and differs == list(PC.SQUARED_DIFFERS)
    tied = [name for name in PC.TIED if R.matrix_profile_plain(PC.series(PC.by_id(name)), *PC.by_id(name)[5:7])["n_tied"] > 1]
    assert len(tied) >= 3 and tied == list(PC.TIED)
    ids = [c[0] for c in PC.CASES]
    assert len(set(ids)) == len(ids)
    lens = {c[0]: R.profile_len(c[2], c[5]) for c in PC.CASES}
    assert [lens[k] for k in ("p63", "p64", "p65", "p127", "p128", "p129")] == [63, 64, 65, 127, 128, 129]
    assert [R.subsequence(PC.by_id(k)[2], PC.by_id(k)[5]) for k in ("m15", "m16", "m17", "m33", "quarter", "m2048")] == [15, 16, 17, 33, 575, 2048]
    assert R.in_lds(2203, 4) and not R.in_lds(2204, 4) and lens["quarter"] == 1726 and lens["n32"] == 29


# --------------------------------------------------------------------------------------------
# the Python layer against a restatement-backed stand-in
# --------------------------------------------------------------------------------------------
def _arg(v):
    return None if v is None or v == 0 else int(v) & 0xFFFFFFFFFFFFFFFF        # static_cast<size_t> of the BIGINT, as api._size_t


def ref_matrix_profile_batch(series, subsequence_length=None, n_best=None, profile=True):
    """api.matrix_profile_batch by the restatement: the same dicts."""
    out = []
    for s in series:
        try:
            r = R.matrix_profile(s, _arg(subsequence_length), _arg(n_best))
            d = {"ok": True, "code": 0, "message": "", "method": "matrix_profile", **{f: r[f] for f in R.FIGURES}}
        except R.InsufficientData as e:
            d = {"ok": False, "code": 3, "message": str(e), "method": "matrix_profile", "period": math.nan, "confidence": math.nan,
                 "n_motifs": 0, "subsequence_length": 0, "best_count": 0, "n_tied": 0}
        out.append(d)
    return out


@pytest.fixture()
def api(monkeypatch):
    from anofox_forecast_amd import api as A
    monkeypatch.setattr(A, "matrix_profile_batch", ref_matrix_profile_batch)
    return A


def test_scalar_mirror_null_rules(api):
    v = PC.family("seasonal", 64, 8, 3)
    r = R.matrix_profile(v)
    got = api.ts_matrix_profile_period(list(v))
    assert same(got, {"period": r["period"], "confidence": r["confidence"], "n_motifs": r["n_motifs"], "subsequence_length": 6,
                      "method": "matrix_profile"})
    assert list(got) == ["period", "confidence", "n_motifs", "subsequence_length", "method"]
    assert api.ts_matrix_profile_period(None) is None and api.ts_matrix_profile_period([1.0] * 31) is None
    assert api.ts_matrix_profile_period([1.0, None] * 31) is None                   # 31 non-NULL values
    with_nulls = [None if i % 7 == 3 else float(x) for i, x in enumerate(np.resize(v, 80))]
    dense = [x for x in with_nulls if x is not None]
    assert same(api.ts_matrix_profile_period(with_nulls, 5, 3), api.ts_matrix_profile_period(dense, 5, 3))
    assert same(api.ts_matrix_profile_period(list(v), 0, 0), api.ts_matrix_profile_period(list(v)))
    # n_best is the exclusion zone (the wrapper's quirk); a negative BIGINT wraps to a huge size_t: m = n / 4, no pair at all
    assert same(api.ts_matrix_profile_period(list(v), None, 9)["n_motifs"], R.matrix_profile(v, None, 9)["n_motifs"])
    r = api.ts_matrix_profile_period(list(v), -1, -1)
    assert r["subsequence_length"] == 16 and math.isnan(r["period"]) and r["n_motifs"] == 0


def test_by_mirror_packs_one_batch(api, monkeypatch):
    calls = []

    def counting(series, *a, **k):
        calls.append((len(series), a))
        return ref_matrix_profile_batch(series, *a, **k)
    monkeypatch.setattr(api, "matrix_profile_batch", counting)
    n = 48
    d = np.concatenate([np.arange(n)[::-1], np.arange(n), np.arange(20)]).astype("datetime64[D]")       # group a arrives in reverse date order
    va, vb = PC.family("seasonal", n, 6, 1), PC.family("counts", n, 7, 3)
    g = ["a"] * n + ["b"] * n + ["c"] * 20
    out = api.ts_matrix_profile_period_by(g, d, np.concatenate([va[::-1], vb, np.ones(20)]), 6, 2, group_name="key")
    assert calls == [(2, (6, 2))]                                  # group c has 20 rows: a NULL row, never sent
    assert out["key"] == ["a", "b", "c"] and list(out) == ["key", "period", "confidence", "n_motifs", "subsequence_length", "method"]
    ra, rb = R.matrix_profile(va, 6, 2), R.matrix_profile(vb, 6, 2)
    assert same(out["period"][:2], [ra["period"], rb["period"]]) and out["confidence"][:2] == [ra["confidence"], rb["confidence"]]
    assert out["n_motifs"][:2] == [ra["n_motifs"], rb["n_motifs"]] and out["subsequence_length"][:2] == [6, 6]
    assert out["period"][2] is None and out["method"] == ["matrix_profile", "matrix_profile", None]


# --------------------------------------------------------------------------------------------
# the C ABI's layout, the argument errors that need no device, the host header under sanitizers
# --------------------------------------------------------------------------------------------
NEW_SYMBOLS = ("anofox_ts_matrix_profile_period", "anofox_hip_matrix_profile_batch", "anofox_hip_matrix_profile_device")


def test_struct_layout_and_symbols(hiplib):
    L = hiplib.load()
    header = open(os.path.join(ROOT, "include", "anofox_fcst_hip.h")).read()
    T = hiplib.MatrixProfilePeriodResultFFI
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (T.__name__, T.__name__), header, re.S).group(1)
    ctype = {"double": C.c_double, "size_t": C.c_size_t}
    fields = []
    for line in body.split("\n"):
        m = re.match(r"\s*(double|size_t|char)\s*(\w+)(\[32\])?;", line)
        if m:
            fields.append((m.group(2), C.c_char * 32 if m.group(1) == "char" else ctype[m.group(1)]))
    assert [(n, t) for n, t in T._fields_] == fields
    assert [n for n, _ in fields] == ["period", "confidence", "n_motifs", "subsequence_length", "method"]
    assert C.sizeof(T) == 64 and T.method.offset == 32 and T.n_motifs.offset == 16
    for s in NEW_SYMBOLS:
        assert s in hiplib.EXPORTED_SYMBOLS and hasattr(L, s) and re.search(r"\b%s\(" % s, header)
    assert hiplib.MATRIX_PROFILE_FIGURES == R.FIGURES
    assert (hiplib.matrix_profile_rows(31), hiplib.matrix_profile_rows(32), hiplib.matrix_profile_rows(1913), hiplib.matrix_profile_rows(100, 4)) == (0, 29, 1723, 97)
    assert all(hiplib.matrix_profile_rows(n, s) == R.profile_len(n, s) for n in range(0, 300) for s in (None, 0, 4, 50))


def test_argument_errors_come_before_the_device(hiplib):
    from anofox_forecast_amd import api as A
    L = hiplib.load()
    err = hiplib.AnofoxError()
    v = np.arange(40.0)
    res = hiplib.MatrixProfilePeriodResultFFI()
    assert not L.anofox_ts_matrix_profile_period(None, 40, 0, 0, C.byref(res), C.byref(err)) and err.code == hiplib.NULL_POINTER
    assert err.message == b"Null pointer argument"
    assert not L.anofox_ts_matrix_profile_period(v.ctypes.data, 40, 0, 0, None, C.byref(err)) and err.message == b"Null pointer argument"
    big = np.zeros(65537)
    assert not L.anofox_ts_matrix_profile_period(big.ctypes.data, 65537, 0, 0, C.byref(res), C.byref(err)) and err.code == hiplib.INVALID_INPUT
    assert b"a series of 65537 rows exceeds the limit of 65536 rows per series" in err.message
    with pytest.raises(A.InvalidInputException, match="exceeds the limit of 65536 rows per series"):
        A.matrix_profile_batch([np.zeros(40), big])
    args = [None if t is C.c_void_p else 0 for t in L.anofox_hip_matrix_profile_device.argtypes[:-1]] + [C.byref(err)]
    assert not L.anofox_hip_matrix_profile_device(*args) and err.code == hiplib.NULL_POINTER
    one = C.c_double(0.0)
    ptr = C.addressof(one)                                             # never dereferenced: the row limit is checked first
    assert not L.anofox_hip_matrix_profile_device(ptr, 64, ptr, 1, 65537, 0, 0, ptr, None, None, ptr, None, C.byref(err))
    assert err.code == hiplib.INVALID_INPUT and b"t_rows 65537 exceeds the limit of 65536 rows per series" in err.message
    lens = np.array([40], dtype=np.uint64)
    assert not L.anofox_hip_matrix_profile_batch(None, lens.ctypes.data, 1, 0, 0, ptr, None, None, None, C.byref(err)) and err.code == hiplib.NULL_POINTER
    assert A.matrix_profile_batch([]) == []


def test_host_matrix_profile_under_sanitizers():
    """csrc/host_matrix_profile.hpp -- the m / exclusion rule, where the arrays live, the workspace, the tile walk, every argument
    check and error text -- compiled on its own (no HIP) and run under ASan + UBSan (tests/c_abi/matrix_profile_san.cpp), as a
    stand-alone program."""
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "matrix_profile_san")
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                               os.path.join(ROOT, "tests", "c_abi", "matrix_profile_san.cpp"), "-o", exe])
        r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and r.stdout.startswith("matrix_profile_san: ok"), (r.stdout, r.stderr[-3000:])


# --------------------------------------------------------------------------------------------
# the boundary: the dispatch by method name keeps its error
# --------------------------------------------------------------------------------------------
def test_method_dispatch_still_raises():
    from anofox_forecast_amd import api as A
    v = list(PC.family("seasonal", 48, 6))
    for a in ("matrix_profile", "matrixprofile", "mp"):
        for call in (lambda: A.period_method(a), lambda: A._ts_detect_periods(v, a), lambda: A.periods_batch([v], a),
                     lambda: A.ts_detect_periods_by(["g"] * 48, np.arange(48).astype("datetime64[D]"), v, {"method": a})):
            with pytest.raises(A.InvalidInputException, match="'matrix_profile' is not implemented by the HIP backend"):
                call()
    src = open(os.path.join(ROOT, "anofox-forecast_amd", "csrc", "host_api.hip")).read()
    assert '{"matrix_profile", "matrix_profile", -1}' in src and '{"mp", "matrix_profile", -1}' in src
