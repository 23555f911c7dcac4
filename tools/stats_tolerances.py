#!/usr/bin/env python3
"""Measure the tolerance table of the statistics contract on the CPU and write it to
tests/golden/stats_tolerances.json.

    python tools/stats_tolerances.py

Per parity input family and per floating figure that is a sum: noise = the largest deviation, over the family's series, between
the restatement tests/stats_ref.py in the source's order of additions and the same restatement with every sum taken by math.fsum
and by a fixed pairwise tree; measured = max(1e-12, 16 x noise).  The file holds 2 x measured (the 1e-12 floor stays): libm's
last bit differs between machines, and tests/test_stats_cpu.py accepts a committed value between 1 and 4 times its own fresh
measurement."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import stats_cases as SC  # noqa: E402
import stats_ref as R  # noqa: E402


def main():
    fresh = R.noise_table(SC.families())
    table = {fam: {f: (1e-12 if v == 1e-12 else 2.0 * v) for f, v in row.items()} for fam, row in fresh.items()}
    with open(SC.TOLERANCES, "w") as f:
        json.dump({"rule": "2 x max(1e-12, 16 x noise); noise = max deviation |a - b| / max(1, |b|) between the source order and the "
                           "fsum / pairwise-tree orders of tests/stats_ref.py over the family (tools/stats_tolerances.py)",
                   "series_per_family": SC.N_FAMILY, "tolerances": table}, f, indent=1)
    for fam, row in table.items():
        print(fam, " ".join(f"{f}={v:.2e}" for f, v in row.items() if v > 1e-12))


if __name__ == "__main__":
    main()
