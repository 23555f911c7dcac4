"""The inputs of the PELT tests, shared by tests/test_pelt_cpu.py and tests/test_gpu_pelt.py.  A case is (name, values, min_size,
penalty); the families:

(a) the unit-test series of changepoint.rs with their answers as the restatement gives them (asserted on the CPU);
(b) noise on steps far from zero, normal * 1e3 + step * 3e3 + 1e6: the sums round at every step, so another order of additions or
    a cost from prefix sums changes the bits of the cost; lengths 20-69 and around the wave, workgroup and 256-lane edges;
(c) ties: values from {0, 2, 4} with small penalties make many candidates EQUAL, so another tie rule changes the changepoints;
(d) edges of the size rules, the penalty rule and non-finite values;
(e) one series just above the LDS tile, with a min_size that leaves candidates for the last 250 t* only (the literal restatement
    stays affordable, the workspace route still walks full-length segments).
"""
import numpy as np

BOUNDARY_LENGTHS = [63, 64, 65, 127, 128, 129, 255, 256, 257, 300]
TILE = 2048                      # csrc/kernels.hpp PELT_RESIDENT

RUST_UNIT = [                    # (name, values, min_size, changepoints, cost)
    ("step", [0.0] * 50 + [10.0] * 50, 5, [50], 9.210340371976184),
    ("two_steps", [0.0] * 33 + [10.0] * 34 + [0.0] * 33, 5, [33, 67], 18.420680743952367),
    ("constant", [5.0] * 100, 5, [], 0.0),
    ("short", [1.0, 1.0, 1.0, 1.0, 10.0, 10.0, 10.0, 10.0], 2, [4], 4.1588830833596715),
]


def family_a():
    return [("a_" + name, np.array(v), ms, 0.0) for name, v, ms, _, _ in RUST_UNIT]


def noise_series(rng, n):
    k = int(rng.integers(1, 4))
    cuts = np.sort(rng.integers(1, n, size=k))
    level = np.zeros(n)
    for c in cuts:
        level[c:] += float(rng.integers(-2, 3))
    return rng.standard_normal(n) * 1e3 + level * 3e3 + 1e6


def family_b():
    rng = np.random.default_rng(20250211)
    out = []
    for i, n in enumerate(list(range(20, 70)) + BOUNDARY_LENGTHS):
        out.append((("b_%d" if i < 50 else "b_edge_%d") % n, noise_series(rng, n), 1 + i % 5, 0.0))
    return out


def tie_series(rng, n):
    return rng.integers(0, 3, size=n).astype(np.float64) * 2.0


def family_c():
    rng = np.random.default_rng(20250212)
    out = []
    for n in range(6, 13):
        for ms in (1, 2):
            for pen in (0.5, 1.0, 2.0, 4.0):
                for rep in range(3):
                    out.append(("c_%d_%d_%g_%d" % (n, ms, pen, rep), tie_series(rng, n), ms, pen))
    for i, n in enumerate(BOUNDARY_LENGTHS):
        out.append(("c_edge_%d" % n, tie_series(rng, n), 1 + i % 2, (0.5, 1.0, 2.0, 4.0)[i % 4]))
    return out


def family_d():
    rng = np.random.default_rng(20250213)
    out = []
    for ms in (1, 3, 7):
        for n in (2 * ms - 1, 2 * ms, 2 * ms + 1):
            out.append(("d_n%d_ms%d" % (n, ms), noise_series(rng, max(n, 2))[:n], ms, 0.0))
    base = noise_series(rng, 40)
    for ms in (0, -3, 2 ** 31 - 1):
        out.append(("d_ms%d" % ms, base, ms, 0.0))
    for pen in (float("nan"), -1.0, 1e300):
        out.append(("d_pen%r" % pen, base, 2, pen))
    for n in (0, 1, 2):
        out.append(("d_len%d" % n, base[:n], 1, 0.0))
    for name, x in (("nan", float("nan")), ("inf", float("inf")), ("negzero", -0.0)):
        for at in (0, 17, 39):
            v = base.copy() if name != "negzero" else np.zeros(40)
            v[at] = x
            out.append(("d_%s_at%d" % (name, at), v, 2, 0.0))
    out.append(("d_negzero_all", np.full(12, -0.0), 1, 1.0))
    out.append(("d_constant", np.full(77, 3.25), 2, 0.0))
    out.append(("d_two_inf", np.concatenate([base[:20], [np.inf, -np.inf], base[20:]]), 3, 0.0))
    return out


def family_e():
    rng = np.random.default_rng(20250214)
    return [("e_2049", noise_series(rng, TILE + 1), 900, 0.0)]


def small_families():
    return family_a() + family_b() + family_c() + family_d()


def random_ties(count, seed=7):
    """(values, min_size, penalty) of lengths 6-12 for the tie-rule statistic."""
    rng = np.random.default_rng(seed)
    return [(tie_series(rng, int(rng.integers(6, 13))), int(rng.integers(1, 3)), (0.5, 1.0, 2.0, 4.0)[int(rng.integers(0, 4))])
            for _ in range(count)]
