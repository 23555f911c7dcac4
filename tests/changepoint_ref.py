"""numpy restatement of the reference's Bayesian online changepoint detection, the CPU truth of tests/test_gpu_changepoints.py.

`bocpd` is detect_changepoints_bocpd (crates/anofox-fcst-core/src/changepoint.rs:198-356) with the loop over run lengths written as
array operations: every element goes through the same IEEE-754 binary64 operations in the same order as the Rust loop, and the two
sums of a step are accumulated sequentially, as the Rust loops do.  The GPU kernel differs from it in the power function (det_math
instead of libm) and in the association order of those two sums, and in nothing else.

`ffi_bocpd` adds the FFI wrapper (crates/anofox-fcst-ffi/src/lib.rs:3056-3130); `by_rows` restates the row logic of the table
function _ts_detect_changepoints_by_native (src/table_functions/ts_changepoints.cpp:547-747) on top of it.
"""
import numpy as np

MAX_KEEP = 500
REL_TOL = 1e-12


class InsufficientData(Exception):
    pass


def _seq_sum(v):
    acc = 0.0
    for e in v.tolist():
        acc += e
    return acc


def bocpd(values, hazard_lambda, include_probabilities=True, power=None):
    """(is_changepoint [n] bool, changepoint_probability [n], changepoints list).  `power`: the x^y used (default numpy's)."""
    values = np.asarray(values, dtype=np.float64)
    n = len(values)
    if n < 3:
        raise InsufficientData(f"Insufficient data: need at least 3 observations, got {n}")
    power = np.power if power is None else power
    hazard = 1.0 / (1.0 if not hazard_lambda > 1.0 else hazard_lambda)      # f64::max(hazard_lambda, 1.0); NaN gives 1.0
    mu0, kappa0, alpha0, beta0 = 0.0, 0.01, 0.01, 0.01
    run_length_prob = np.array([1.0])
    is_changepoint = np.zeros(n, dtype=bool)
    changepoint_prob = np.zeros(n)
    changepoints = []
    sum_x, sum_x2, run_counts = np.array([0.0]), np.array([0.0]), np.array([0.0])
    cp_threshold = 0.5
    with np.errstate(all="ignore"):
        for t in range(n):
            x = values[t]
            max_run = len(run_length_prob)
            pos = run_counts > 0
            kappa_n = kappa0 + run_counts
            alpha_n = alpha0 + run_counts / 2.0
            mu_n = np.where(pos, (kappa0 * mu0 + sum_x) / kappa_n, mu0)
            ss = np.where(pos, sum_x2 - sum_x * sum_x / np.fmax(run_counts, 1.0), 0.0)
            d = mu0 - mu_n
            beta_n = beta0 + 0.5 * np.fmax(ss, 0.0) + kappa0 * run_counts * (d * d) / (2.0 * kappa_n)
            scale = np.sqrt((beta_n * (kappa_n + 1.0)) / (alpha_n * kappa_n))
            z = (x - mu_n) / np.fmax(scale, 1e-10)
            nu = 2.0 * alpha_n
            pred_prob = power(1.0 + z * z / nu, -(nu + 1.0) / 2.0)

            new_run_length_prob = np.zeros(max_run + 1)
            new_run_length_prob[1:] = run_length_prob * pred_prob * (1.0 - hazard)
            new_run_length_prob[0] = _seq_sum(run_length_prob * pred_prob * hazard)
            total = _seq_sum(new_run_length_prob)
            if total > 1e-300:
                new_run_length_prob = new_run_length_prob / total
            cp_detected = new_run_length_prob[1]
            changepoint_prob[t] = cp_detected
            is_changepoint[t] = bool(cp_detected > cp_threshold) and t > 0
            if is_changepoint[t]:
                changepoints.append(t)

            sum_x = np.concatenate(([0.0], sum_x + x))
            sum_x2 = np.concatenate(([0.0], sum_x2 + x * x))
            run_counts = np.concatenate(([0.0], run_counts + 1.0))
            run_length_prob = new_run_length_prob
            if len(run_length_prob) > MAX_KEEP:
                run_length_prob = run_length_prob[:MAX_KEEP]
                sum_x, sum_x2, run_counts = sum_x[:MAX_KEEP], sum_x2[:MAX_KEEP], run_counts[:MAX_KEEP]
    if not include_probabilities:
        changepoint_prob = np.zeros(n)
    return is_changepoint, changepoint_prob, changepoints


def pow_exp_log(b, e):
    """x^y as exp(y log x): the second libm route of the tolerance argument."""
    return np.exp(e * np.log(b))


def ffi_bocpd(values, hazard_lambda, include_probabilities=True):
    """anofox_ts_detect_changepoints_bocpd: hazard_lambda <= 0 (or NaN) means 250; None where the call fails."""
    lam = hazard_lambda if hazard_lambda > 0.0 else 250.0
    try:
        return bocpd(values, lam, include_probabilities)
    except InsufficientData:
        return None


def scalar_bocpd(values, hazard_lambda=250.0, include_probabilities=False):
    """The SQL scalar _ts_detect_changepoints_bocpd (ts_changepoints.cpp:233-360) as a dict of lists, or None (SQL NULL)."""
    if values is None:
        return None
    vals = [float(v) for v in values if v is not None]
    if len(vals) < 2:
        return None
    r = ffi_bocpd(vals, 250.0 if hazard_lambda is None else hazard_lambda, bool(include_probabilities))
    if r is None:
        return None
    return {"is_changepoint": [bool(f) for f in r[0]], "changepoint_probability": [float(p) for p in r[1]],
            "changepoint_indices": [int(i) for i in r[2]]}


def by_rows(group, date_us, value, hazard_lambda):
    """Rows of _ts_detect_changepoints_by_native: `date_us` microseconds or None, `value` float or None.  A list of
    (group, date_us or None, is_changepoint, probability or None)."""
    order, groups, null_rows = [], {}, []
    for g, d, v in zip(group, date_us, value):
        if d is None:
            null_rows.append(g)
            continue
        if g not in groups:
            groups[g] = []
            order.append(g)
        groups[g].append((d, 0.0 if v is None else float(v)))
    rows = []
    for g in order:
        pairs = groups[g]
        if len(pairs) < 2:
            rows += [(g, d, False, None) for d, _ in pairs]
            continue
        pairs = sorted(pairs)
        r = ffi_bocpd([v for _, v in pairs], hazard_lambda, True)
        if r is None:
            rows += [(g, d, False, None) for d, _ in pairs]
            continue
        rows += [(g, d, bool(f), float(p)) for (d, _), f, p in zip(pairs, r[0], r[1])]
    rows += [(g, None, False, None) for g in null_rows]
    return rows


def rel(a, b):
    """The deviation measure of tests/test_gpu_intermittent.py: |a - b| / max(1, |b|), NaN against NaN and equal infinities are 0."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    same = (np.isnan(a) & np.isnan(b)) | (a == b)
    with np.errstate(all="ignore"):
        d = np.abs(a - b) / np.maximum(1.0, np.abs(b))
    d = np.where(same, 0.0, d)
    return float(np.max(np.where(np.isnan(d), np.inf, d))) if d.size else 0.0


# --------------------------------------------------------------------------------------------
# the parity batch of the GPU test (also checked on the CPU: no probability within 1e-9 of 0.5)
# --------------------------------------------------------------------------------------------
PARITY_LAMBDAS = (250.0, 10.0, 1.0, 0.5, -1.0)
PARITY_SEED = 20240611
EDGE_LENGTHS = (0, 1, 2, 3, 499, 500, 501, 502)


def parity_batch():
    """(series, valids): a few hundred ragged series of lengths 0..700 -- M5-like counts, real-valued series, constants,
    all-zero series, single spikes, NULL masks -- with every edge length present."""
    rng = np.random.default_rng(PARITY_SEED)
    series, valids = [], []

    def add(y, valid=None):
        y = np.asarray(y, dtype=np.float64)
        series.append(y)
        valids.append(None if valid is None else np.asarray(valid, dtype=bool))

    for n in EDGE_LENGTHS:
        add(rng.poisson(1.5, n).astype(np.float64))
        add(100.0 + 5.0 * rng.standard_normal(n))
    for n in (700, 640, 511, 513, 64, 65, 63, 128, 129):
        add(rng.poisson(0.8, n).astype(np.float64))
    add(np.full(300, 5.0))
    add(np.full(620, -3.25))
    add(np.zeros(200))
    add(np.zeros(560))
    for n, at, h in ((120, 60, 1e3), (600, 550, 1e6), (520, 10, -4e4), (90, 89, 250.0)):
        y = rng.standard_normal(n)
        y[at] += h
        add(y)
    y = np.concatenate((np.full(40, 100.0), np.full(40, 10.0), np.full(40, 50.0)))
    add(y)
    add(y + 0.01 * rng.standard_normal(len(y)))
    while len(series) < 240:
        n = int(rng.integers(3, 701)) if rng.random() < 0.8 else int(rng.integers(0, 40))
        kind = rng.integers(0, 4)
        if kind == 0:
            y = rng.poisson(rng.uniform(0.2, 6.0), n).astype(np.float64)
            y[rng.random(n) < 0.3] = 0.0
        elif kind == 1:
            y = rng.uniform(-1.0, 1.0) * np.arange(n) / 50.0 + rng.uniform(0.1, 30.0) * rng.standard_normal(n) + rng.uniform(-500, 500)
        elif kind == 2:
            lv = rng.uniform(-50, 50, 4)
            y = lv[np.minimum(np.arange(n) * 4 // max(n, 1), 3)] + rng.uniform(0.01, 2.0) * rng.standard_normal(n)
        else:
            y = np.exp(rng.uniform(-8, 8)) * rng.standard_normal(n)
        valid = None
        if rng.random() < 0.25 and n:
            valid = rng.random(n) >= 0.1
        add(y, valid)
    return series, valids


def masked(y, valid):
    """The series as the GPU entries see it: a NULL counts as 0.0."""
    return y if valid is None else np.where(valid, y, 0.0)


def effective_lambda(hazard_lambda):
    """The lambda the recursion runs with: the wrapper's `<= 0 means 250`, then the core's max(lambda, 1)."""
    lam = hazard_lambda if hazard_lambda > 0.0 else 250.0
    return lam if lam > 1.0 else 1.0


def _parity_job(args):
    y, lam = args
    r = ffi_bocpd(y, lam, True)
    return None if r is None else (r[0], r[1])


def parity_reference(series, valids, lambdas=PARITY_LAMBDAS, workers=None):
    """{lambda: [None (the call fails) or (is_changepoint, probability) per series]} from the restatement, on a pool of worker
    processes (fresh interpreters: they never touch the GPU).  Lambdas that run the same recursion (1 and 0.5; 250 and -1) are
    computed once."""
    import multiprocessing as mp
    import os
    clean = [masked(y, v) for y, v in zip(series, valids)]
    eff = sorted({effective_lambda(lam) for lam in lambdas})
    jobs = [(y, lam) for lam in eff for y in clean]
    workers = workers or max(1, min(15, (os.cpu_count() or 2) - 1))
    with mp.get_context("spawn").Pool(workers) as pool:
        res = pool.map(_parity_job, jobs, chunksize=4)
    by_eff = {lam: res[k * len(clean):(k + 1) * len(clean)] for k, lam in enumerate(eff)}
    return {lam: by_eff[effective_lambda(lam)] for lam in lambdas}
