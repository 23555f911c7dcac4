"""CPU: the intermittent-demand checker (tests/intermittent_ref.py) against the reference's pins, its edge cases and properties."""
import json
import os

import numpy as np

import intermittent_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KATS = json.load(open(os.path.join(ROOT, "tests", "golden", "intermittent_kats.json")))
Y30 = np.array(KATS["distinctness_series"]["y"])
Y12 = np.array(KATS["short_series"]["y"])


def test_checker_meets_the_pins():
    pins = KATS["pins"]["point_1"]
    for m in ("CrostonClassic", "CrostonSBA", "TSB", "ADIDA"):
        assert round(float(R.point_forecasts([Y30], m)[0]), 6) == pins[m], m
    # IMAPA: levels 1, 3 and 4 have their optimum on the bound 0.1 and match; level 2 has an interior optimum (alpha ~ 0.16905)
    # where the reference's optimiser evidently stops elsewhere: 1.226437 against the pin 1.226488 (-4.2e-5 relative)
    imapa = float(R.point_forecasts([Y30], "IMAPA")[0])
    assert round(imapa, 6) == 1.226437
    assert abs(imapa / pins["IMAPA"] - 1.0) < 5e-5
    assert R.aggregation_level([Y30])[0] == 4          # 8 demands, last at index 27: 28 / 8 = 3.5 -> 4 (half up)


def test_edge_cases():
    for m in ("CrostonClassic", "TSB", "ADIDA", "IMAPA"):
        assert R.point_forecasts([np.zeros(17)], m)[0] == 0.0, m
    assert R.point_forecasts([np.array([0.0, 5.0, 0.0])], "CrostonClassic")[0] == 2.5
    assert R.point_forecasts([np.array([0.0, 5.0, 0.0])], "CrostonSBA")[0] == 0.95 * 2.5
    # a single demand at the last row: K = n, one level-K sum, SESopt of one value is that value
    y = np.zeros(40); y[-1] = 8.0
    assert R.aggregation_level([y])[0] == 40
    assert R.point_forecasts([y], "ADIDA")[0] == 8.0 / 40.0


def test_properties():
    y = np.arange(1.0, 31.0)
    assert R.aggregation_level([y])[0] == 1
    # without zeros Croston's intervals are all 1: the forecast is SES(0.1) of the series; ADIDA / IMAPA (K = 1) coincide
    l = y[0]
    for v in y[1:]:
        l = l + 0.1 * (v - l)
    assert R.point_forecasts([y], "CrostonClassic")[0] == l
    assert R.point_forecasts([y], "ADIDA")[0] == R.point_forecasts([y], "IMAPA")[0]
    # vectorised over ragged series: every series as if alone
    rng = np.random.default_rng(3)
    series = [np.where(rng.random(n) < 0.3, rng.integers(1, 9, n), 0).astype(float) for n in rng.integers(3, 90, 40)]
    for m in R.MODELS:
        together = R.point_forecasts(series, m)
        alone = np.array([R.point_forecasts([s], m)[0] for s in series])
        assert np.array_equal(together, alone), m
    # the models are distinct on the pin series
    vals = {m: float(R.point_forecasts([Y30], m)[0]) for m in R.MODELS}
    assert len(set(vals.values())) == len(vals)
    assert all(float(R.point_forecasts([Y12], m)[0]) > 0 for m in R.MODELS)


def test_product_never_imports_the_checker():
    pkg = os.path.join(ROOT, "anofox-forecast_amd")
    for dp, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".hpp", ".cpp", ".h")):
                txt = open(os.path.join(dp, f), errors="replace").read()
                # (a comment may name the checker for provenance; no code line may use it)
                for line in txt.splitlines():
                    code = line.split("//")[0].split("#")[0]
                    assert "intermittent_ref" not in code, (os.path.join(dp, f), line)
