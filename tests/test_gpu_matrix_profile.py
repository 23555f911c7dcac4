"""GPU: the matrix-profile period entries (anofox_ts_matrix_profile_period, anofox_hip_matrix_profile_batch / _device),
device.matrix_profile_block, api.matrix_profile_batch and the operator mirrors against the restatement tests/matrix_profile_ref.py.
The contract is equality of bits: every figure, every profile value, every profile index and every status is
compared with ==, NaN exactly where the restatement has NaN, through every entry and twice in a row.  `period` is the minimum of
the restatement's set of tied lags (the rule of this package; the source returns any of the set).

Boundaries of the kernel, with a shape on each side (tests/matrix_profile_cases.py): tiles of 64 x 64 pairs (P = 63 .. 65 and
127 .. 129), chunks of 16 steps of k (m = 15 .. 17, 33), the series and its profile in LDS up to 2,203 rows at m = 4 (2,204 goes to
the workspace), m = n / 4, the subsequence limit of 2,048 (2,049 fails alone), exclusions that leave no pair or ten profile values."""
import ctypes as C
import math

import numpy as np
import pytest

import matrix_profile_cases as PC
import matrix_profile_ref as R

pytestmark = pytest.mark.gpu

COMPUTATION_ERROR = 3
_CACHE = {}


@pytest.fixture(scope="module")
def api(hiplib):
    import torch
    assert torch.cuda.is_available()
    hiplib.load()
    from anofox_forecast_amd import api as A
    return A


def eq(a, b):
    """== with NaN equal to NaN, over floats, ints and sequences."""
    if isinstance(a, (list, tuple, np.ndarray)):
        return len(a) == len(b) and all(eq(x, y) for x, y in zip(a, b))
    if a != a:
        return b != b
    return a == b


def ref(key, series, sub, n_best, form="plain"):
    """The restatement of one series, computed once per module."""
    k = (key, sub, n_best)
    if k not in _CACHE:
        n = len(series)
        if n < R.MIN_ROWS:
            _CACHE[k] = {"ok": False, "message": f"Insufficient data: need at least 32 observations, got {n}"}
        elif R.subsequence(n, sub) > R.MAX_M:
            _CACHE[k] = {"ok": False, "message": "exceeds the limit of 2048"}
        else:
            r = (R.matrix_profile if form == "numpy" else R.matrix_profile_plain)(series, sub, n_best)
            assert r["period"] == min(r["tied_lags"]) if r["tied_lags"] else math.isnan(r["period"])
            _CACHE[k] = {"ok": True, "message": "", **r}
    return _CACHE[k]


def check(got, want, where):
    assert got["ok"] == want["ok"], (where, got, want)
    if not want["ok"]:
        assert math.isnan(got["period"]) and math.isnan(got["confidence"]), where
        if "message" in got:
            assert got["code"] == COMPUTATION_ERROR and want["message"] in got["message"], (where, got["message"])
        if "profile" in got:
            assert len(got["profile"]) == 0 and len(got["profile_index"]) == 0, where
        return
    for f in R.FIGURES:
        assert eq(float(got[f]), float(want[f])), (where, f, got[f], want[f])
    if "profile" in got:
        assert eq(list(got["profile"]), want["mp"]), (where, "mp")
        assert [int(x) for x in got["profile_index"]] == want["mpi"], (where, "mpi")


def block(series, t_extra=5, extra_cols=3):
    import torch
    n = len(series)
    ld = (n + extra_cols + 63) // 64 * 64
    T = max(len(s) for s in series) + t_extra
    y = np.zeros((T, ld))
    ln = np.zeros(ld, dtype=np.int32)
    for i, s in enumerate(series):
        ln[i] = len(s)
        y[:len(s), i] = s
    return torch.from_numpy(y).to("cuda:0"), torch.from_numpy(ln).to("cuda:0"), n, ld, T


def block_dicts(fig, prof, idx, st, series, sub, rows):
    """The device outputs as the batch entry's dicts; everything beyond a series' own profile must be NaN / -1."""
    assert prof.shape[0] == rows and idx.shape[0] == rows
    res = []
    for i, s in enumerate(series):
        ok = st[i] == 0
        p = R.profile_len(len(s), sub) if ok else 0
        assert np.isnan(prof[p:, i]).all() and (idx[p:, i] == -1).all(), i
        res.append({"ok": bool(ok), **{f: fig[k, i] for k, f in enumerate(R.FIGURES)}, "profile": prof[:p, i], "profile_index": idx[:p, i]})
    assert np.isnan(fig[:, len(series):]).all() and (st[len(series):] == -1).all()
    return res


def through_every_entry(api, hiplib, series, wants, sub, n_best, tag):
    """The batch entry, the single entry, the raw device entry and device.matrix_profile_block, each twice in a row."""
    import torch
    from anofox_forecast_amd import device as D
    L = hiplib.load()
    for rep in range(2):
        got = api.matrix_profile_batch(series, sub, n_best)
        for i, (g, w) in enumerate(zip(got, wants)):
            check(g, w, (tag, "batch", rep, i))
        for i, (s, w) in enumerate(zip(series, wants)):
            res, err = hiplib.MatrixProfilePeriodResultFFI(), hiplib.AnofoxError()
            v = np.ascontiguousarray(s, dtype=np.float64)
            ok = L.anofox_ts_matrix_profile_period(v.ctypes.data, len(v), sub or 0, n_best or 0, C.byref(res), C.byref(err))
            assert bool(ok) == w["ok"], (tag, "single", i, err.message)
            if ok:
                assert eq(res.period, w["period"]) and res.confidence == w["confidence"] and res.n_motifs == w["n_motifs"]
                assert res.subsequence_length == w["subsequence_length"] and res.method == b"matrix_profile"
            else:
                assert err.code == COMPUTATION_ERROR and w["message"] in err.message.decode()
        y, ln, n, ld, T = block(series)
        rows = hiplib.matrix_profile_rows(T, sub)
        fig = torch.full((6, ld), float("nan"), dtype=torch.float64, device="cuda:0")
        prof = torch.full((max(rows, 1), ld), float("nan"), dtype=torch.float64, device="cuda:0")
        idx = torch.full((max(rows, 1), ld), -1, dtype=torch.int32, device="cuda:0")
        st = torch.full((ld,), -1, dtype=torch.int32, device="cuda:0")
        err = hiplib.AnofoxError()
        assert L.anofox_hip_matrix_profile_device(y.data_ptr(), ld, ln.data_ptr(), n, T, sub or 0, n_best or 0, fig.data_ptr(), prof.data_ptr(),
                                                  idx.data_ptr(), st.data_ptr(), None, C.byref(err)), err.message
        got = block_dicts(fig.cpu().numpy(), prof.cpu().numpy()[:rows], idx.cpu().numpy()[:rows], st.cpu().numpy(), series, sub, rows)
        for i, (g, w) in enumerate(zip(got, wants)):
            check(g, w, (tag, "device", rep, i))
        out = D.matrix_profile_block(y, ln, sub or 0, n_best or 0, n_series=n)
        got = block_dicts(out["figures"].cpu().numpy(), out["profile"].cpu().numpy(), out["profile_index"].cpu().numpy(),
                          out["status"].cpu().numpy(), series, sub, rows)
        for i, (g, w) in enumerate(zip(got, wants)):
            check(g, w, (tag, "block", rep, i))
        assert out["period"].data_ptr() == out["figures"][0].data_ptr() and out["n_tied"].data_ptr() == out["figures"][5].data_ptr()


GROUPS = sorted({(c[5], c[6]) for c in PC.CASES}, key=str)


@pytest.mark.parametrize("sub,n_best", GROUPS, ids=lambda x: str(x))
def test_cases_through_every_entry(api, hiplib, sub, n_best):
    cases = [c for c in PC.CASES if (c[5], c[6]) == (sub, n_best)]
    series = [PC.series(c) for c in cases]
    wants = [ref(c[0], s, sub, n_best, c[7]) for c, s in zip(cases, series)]
    assert all(w["ok"] for w in wants)
    through_every_entry(api, hiplib, series, wants, sub, n_best, [c[0] for c in cases])


def test_too_short(api, hiplib):
    v = PC.family("seasonal", 31, 7, 1)
    r = api.matrix_profile_batch([v])[0]
    assert not r["ok"] and r["code"] == COMPUTATION_ERROR and r["message"] == "Insufficient data: need at least 32 observations, got 31"
    assert api.ts_matrix_profile_period(list(v)) is None


def test_mixed_batch_fails_alone(api, hiplib):
    """A too-short, a NaN, a constant and ordinary series in one call; the restatement of each is that of the series alone."""
    series = [PC.family("seasonal", 31, 7, 1), PC.family("nan", 110, 9, 3), PC.family("constant", 90), PC.family("seasonal", 150, 12, 4),
              PC.family("counts", 20, 7, 0), PC.family("intermittent", 120, 7, 5), np.zeros(0), PC.family("counts", 61, 7, 1)]
    wants = [ref(("mixed", i), s, None, None) for i, s in enumerate(series)]
    assert [w["ok"] for w in wants] == [False, True, True, True, False, True, False, True]
    through_every_entry(api, hiplib, series, wants, None, None, "mixed")


def test_subsequence_limit_fails_alone(api, hiplib):
    """A forced m = 2,049 needs 8,196 rows to take effect: that series fails alone and names the limit, its neighbours (m = n / 4) run."""
    series = [PC.family("seasonal", 100, 11, 20), PC.family("seasonal", 8196, 365, 50), PC.family("counts", 160, 11, 23)]
    wants = [ref(("limit", i), s, 2049, None) for i, s in enumerate(series)]
    assert [w["ok"] for w in wants] == [True, False, True]
    through_every_entry(api, hiplib, series, wants, 2049, None, "limit")
    r = api.matrix_profile_batch(series, 2049)[1]
    assert "subsequence length of 2049 rows of a series of 8196 observations exceeds the limit of 2048" in r["message"]


def test_mirrors_on_a_grouped_table(api):
    n = 61
    va, vb = PC.family("counts", n, 7, 1), PC.family("seasonal", n, 9, 2)
    d = np.concatenate([np.arange(n)[::-1], np.arange(n), np.arange(20)]).astype("datetime64[D]")        # group a arrives in reverse date order
    g = ["a"] * n + ["b"] * n + ["c"] * 20
    out = api.ts_matrix_profile_period_by(g, d, np.concatenate([va[::-1], vb, np.ones(20)]), 5, 2, group_name="key")
    assert list(out) == ["key", "period", "confidence", "n_motifs", "subsequence_length", "method"] and out["key"] == ["a", "b", "c"]
    for k, v in enumerate((va, vb)):
        w = ref(("by", k), v, 5, 2)
        assert eq(out["period"][k], w["period"]) and out["confidence"][k] == w["confidence"] and out["n_motifs"][k] == w["n_motifs"]
        assert out["subsequence_length"][k] == 5 and out["method"][k] == "matrix_profile"
        assert eq(api.ts_matrix_profile_period(list(v), 5, 2)["period"], w["period"])
    assert all(out[f][2] is None for f in ("period", "confidence", "n_motifs", "subsequence_length", "method"))
