"""CPU: the long-double restatement of the closed-form classic models (tests/classic_ref.py) against the reference's pins and
against the oracle -- what validates the checker of tests/test_gpu_classic.py without a GPU -- and the constants of the classic
launches that the GPU tests' shapes are chosen by, read from the sources."""
import json
import os
import re

import numpy as np

import classic_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = json.load(open(os.path.join(ROOT, "tests", "golden", "reference_kats.json")))
CSRC = os.path.join(ROOT, "anofox-forecast_amd", "csrc")


def test_restatement_meets_the_reference_pins():
    """The KAT series of reference_kats.json: every closed-form model and the two fixed-constant smoothers, as the SQL tests pin them."""
    seen = set()
    for c in GOLD["cases"]:
        model = {"NAIVE": "Naive"}.get(c["model"], c["model"])
        if model not in R.MODELS:
            continue
        o = c["options"]
        assert not o["auto_detect"]
        code, p = R.point(model, c["values"], c["horizon"], period=max(o["seasonal_period"], 1), window=0)
        assert code == 0
        if c["check"] == "round6_first":
            assert round(float(p[0]), 6) == c["expected"], (model, float(p[0]))
        elif c["check"] == "abs_all":
            assert np.all(np.abs(p.astype(np.float64) - np.array(c["expected"])) <= c["tol"]), model
        elif c["check"] == "bits_all":                 # pinned to the bit in fp64: the long-double sums round to within an ulp or two of it
            assert R.rel(p, c["expected"]) <= 4 * np.finfo(np.float64).eps, model
        seen.add(model)
    assert seen == set(R.MODELS)


def _oracle_cases(oracle):
    for model, kw, series in R.closed_form_cases():
        for h in R.CASE_HORIZONS:
            oo = oracle.make_options(model, h, auto_detect=False, **kw)
            yield model, kw, h, series, [oracle.forecast(y, oo) for y in series]


def test_oracle_meets_the_restatement(oracle):
    """Error codes exactly; forecasts and interval bounds within classic_ref.ORACLE_VS_LONGDOUBLE, the figure the GPU test's tolerance is four times of:
    it is MEASURED here (the worst case over the shared cases) and pinned from both sides, so that it can neither drift nor be
    loosened without this test saying so."""
    worst, where = 0.0, None
    for model, kw, h, series, refs in _oracle_cases(oracle):
        for y, ref in zip(series, refs):
            code, p = R.point(model, y, h, period=max(kw.get("seasonal_period", 0), 1), window=kw.get("window", 0))
            assert (0 if ref["ok"] else ref["code"]) == code, (model, kw, len(y), ref)
            if code:
                continue
            lo, hi = R.intervals(ref["point"], y, 0.90)          # (the interval arithmetic alone: around the oracle's own forecasts)
            d = max(R.rel(ref["point"], p), R.rel(ref["lower"], lo), R.rel(ref["upper"], hi))
            if d > worst:
                worst, where = d, (model, kw, h, len(y))
    print(f"oracle against the long-double restatement: worst {worst:.3e} at {where}")
    assert worst <= R.ORACLE_VS_LONGDOUBLE, (worst, where)
    assert worst >= R.ORACLE_VS_LONGDOUBLE / 2, (worst, "the pinned figure is stale: measure again")


def test_intervals_and_fitted_values_meet_the_restatement(oracle):
    """forecast.rs:2558-2591 (z ladder, population sd, sqrt(step)) and :2593-2643 (fitted values) restated against the oracle's.
    Bounds from the number format: a sequential fp64 sum of n terms is within (n - 1) eps of the exact one, so mean, variance and
    the width z sd sqrt(step) (a square root halves the error) are within n eps = 1.8e-14 for n <= 80, on values below the scale of
    the bounds they are added to; the SES recursion at 0.3 rounds three times per step and damps earlier errors by 0.7, so a fitted
    value is within 3 eps / (1 - 0.7) = 10 eps of max |y| (< 50 here): 1.1e-13 on the scale max(1, |value|) of a residual near zero."""
    eps = float(np.finfo(np.float64).eps)
    tol_iv, tol_fit = 80 * eps, 10 * eps * 50
    rng = np.random.default_rng(5)
    series = [rng.normal(20.0, 6.0, int(L)) for L in rng.integers(3, 80, 24)]
    ladder = {0.5: 1.0, 0.79: 1.0, 0.8: 1.28, 0.9: 1.645, 0.949: 1.645, 0.95: 1.96, 0.99: 2.576, 0.999: 2.576}
    for conf, z in ladder.items():
        assert R.z_value(conf) == z
        oo = oracle.make_options("Naive", 7, auto_detect=False, confidence_level=conf)
        for y in series:
            ref = oracle.forecast(y, oo)
            lo, hi = R.intervals(ref["point"], y, conf)
            assert R.rel(ref["lower"], lo) <= tol_iv and R.rel(ref["upper"], hi) <= tol_iv, (conf, len(y))
    for model, kw in (("Naive", {}), ("SeasonalNaive", {"seasonal_period": 5}), ("SeasonalNaive", {"seasonal_period": 200}), ("SES", {}),
                      ("SMA", {}), ("ARIMA", {}), ("SeasonalES", {"seasonal_period": 2})):
        oo = oracle.make_options(model, 3, auto_detect=False, include_fitted=True, include_residuals=True, **kw)
        for y in series:
            ref = oracle.forecast(y, oo)
            if not ref["ok"]:
                continue
            f = R.fitted(model, y, kw.get("seasonal_period", 1))
            assert R.rel(ref["fitted"], f) <= tol_fit and R.rel(ref["residuals"], R._ld(y) - f) <= tol_fit, (model, len(y))
            assert R.rel(ref["mse"], np.sum((R._ld(y) - f) ** 2) / len(y)) <= tol_fit


def _const(text, pattern):
    m = re.search(pattern, text)
    assert m, pattern
    return m


def test_launch_constants_the_gpu_shapes_are_chosen_by():
    """tests/test_gpu_classic.py picks its batch sizes and periods from these constants; a change of any of them must move the
    shapes with it.  The LDS opt-in of the one-launch kernel: SeasonalES asks for 8 * nm_lds_doubles<1>() + 8 * NM_K * m * 64 bytes
    with nm_lds_doubles<1>() = ((1 + 1) * 1 + (1 + 1)) * 64 = 256 doubles, i.e. 2,048 + 2,048 m bytes: 49,152 bytes (48 KB, no opt-in)
    at m = 23, 51,200 (opt-in) at m = 24."""
    host = open(os.path.join(CSRC, "host_api.hip")).read()
    kern = open(os.path.join(CSRC, "kernels.hip")).read()
    nm = open(os.path.join(CSRC, "nm.hpp")).read()
    dev = open(os.path.join(CSRC, "ets_device.hpp")).read()
    assert int(_const(host, r"constexpr int TINY_BATCH_PROBLEMS = (\d+);").group(1)) == 1024
    assert int(_const(kern, r"constexpr int CLASSIC_LDS_PERIOD = (\d+);").group(1)) == 48
    assert _const(host, r"kind == CK_SEASONAL_ES\) && m > 48\)")               # the host's own copy of that limit (ring scratch or not)
    assert int(_const(dev, r"constexpr int ETS_LDS_PERIOD = (\d+);").group(1)) == 64
    assert int(_const(nm, r"constexpr int NM_K = (\d+);").group(1)) == 4 and int(_const(nm, r"constexpr int NM_BLOCK = (\d+);").group(1)) == 64
    assert _const(nm, r"nm_lds_doubles\(\) \{ return \(\(D \+ 1\) \* D \+ \(D \+ 1\)\) \* NM_BLOCK; \}")
    lds = lambda m: 8 * ((1 + 1) * 1 + (1 + 1)) * 64 + 8 * 4 * m * 64
    assert lds(23) == 48 * 1024 and lds(24) > 48 * 1024
    body = host[host.index("void run_classic("):]
    body = body[:body.index("\n}\n")]
    assert [int(x) for x in _const(body, r"static const int BUDGET\[\] = \{([^}]*)\};").group(1).split(",")] == [24, 24, 24, 24, 48, 48, 96, 192, 1024]
    assert _const(body, r"f\.spec_below = (\d+); f\.spec2_below = (\d+);").groups() == ("8192", "1024")
    assert _const(body, r"seq0 = n >= (\d+)u \* (\d+)u;").groups() == ("4", "65536")
    assert _const(body, r"std::max<size_t>\(\(n \+ 15\) / 16, std::min<size_t>\(n, 1024\)\)")      # the HBM ring area of a uniform batch


def test_product_never_imports_the_checker():
    pkg = os.path.join(ROOT, "anofox-forecast_amd")
    for dp, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".hpp", ".cpp", ".h")):
                for line in open(os.path.join(dp, f), errors="replace").read().splitlines():
                    code = line.split("//")[0].split("#")[0]
                    assert "classic_ref" not in code, (os.path.join(dp, f), line)
