"""A pure-Python restatement of the reference's conformal.rs: Python floats (IEEE fp64, one rounding per operation, no fused
multiply-add), `sorted`, `math.ceil` / `math.floor`, and sequential sums from 0.0 in row order.  It shares nothing with the
library: it is the checker of tests/test_conformal_cpu.py and tests/test_gpu_conformal.py, whose contract is equality of bits.

Errors are returned the way the FFI reports them, as the text of the source's ForecastError: every function returns
(value, None) or (None, message).

A residual vector with a NaN is outside the contract: the source sorts with partial_cmp(..).unwrap_or(Equal), which leaves the
order of such a vector to its sort's internals.  `has_nan` tells; the functions here do not special-case it."""
import math

METHODS = ("symmetric", "asymmetric", "adaptive")
STRATEGIES = ("split", "crossval", "jackknife+")

EMPTY = "Insufficient data: need at least 1 observations, got 0"
ALPHA_V1 = "Invalid input: Alpha must be between 0 and 1 (exclusive)"
NO_ALPHA = "Invalid input: At least one alpha value is required"
NO_FORECAST = "Invalid input: At least one forecast is required"
DIFFICULTY = "Invalid input: Difficulty scores must be positive"
NEED_DIFFICULTY = "Invalid input: Difficulty scores required for adaptive method"
JACKKNIFE_ASYM = "Invalid input: JackknifePlus strategy does not support asymmetric method"


def has_nan(values):
    return any(v != v for v in values)


def alpha_ok(alpha):
    """(0.0..1.0).contains(&alpha): 0 is in, 1 and a NaN are not."""
    return 0.0 <= alpha < 1.0


def show(x):
    """Rust's `{}` of an f64 for the values the messages print (no exponent, integers without a fraction)."""
    if x != x:
        return "NaN"
    if x in (math.inf, -math.inf):
        return "inf" if x > 0 else "-inf"
    if x == int(x) and abs(x) < 1e16:
        return str(int(x)) if (x != 0 or math.copysign(1.0, x) > 0) else "-0"
    return repr(x)


def seq_sum(values):
    total = 0.0
    for v in values:
        total += v
    return total


def compute_quantile(s, q):
    """conformal.rs:429-449 on a sorted list."""
    if not s:
        return math.nan
    if q <= 0.0:
        return s[0]
    if q >= 1.0:
        return s[-1]
    n = len(s)
    index = q * float(n - 1)
    lo = int(math.floor(index))
    up = min(lo + 1, n - 1)
    frac = index - float(lo)
    return s[lo] * (1.0 - frac) + s[up] * frac


def quantile_level(n, alpha):
    """ceil((n + 1)(1 - alpha)) / n clamped to [0, 1] (conformal.rs:137-141)."""
    nf = float(n)
    q = float(math.ceil((nf + 1.0) * (1.0 - alpha))) / nf
    return min(max(q, 0.0), 1.0)


def score(sorted_values, alpha):
    return compute_quantile(sorted_values, quantile_level(len(sorted_values), alpha))


def sorted_abs(residuals):
    return sorted(abs(r) for r in residuals)


# ---------------------------------------------------------------------------------------------------------------------------
# v1
# ---------------------------------------------------------------------------------------------------------------------------
def conformal_quantile(residuals, alpha):
    if not residuals:
        return None, EMPTY
    if not alpha_ok(alpha):
        return None, ALPHA_V1
    return score(sorted_abs(residuals), alpha), None


def conformal_intervals(forecasts, s):
    return [f - s for f in forecasts], [f + s for f in forecasts]


def conformal_predict(residuals, forecasts, alpha):
    s, e = conformal_quantile(residuals, alpha)
    if e:
        return None, e
    lower, upper = conformal_intervals(forecasts, s)
    return {"point": list(forecasts), "lower": lower, "upper": upper, "coverage": 1.0 - alpha, "conformity_score": s,
            "method": "split_conformal"}, None


def conformal_predict_multi(residuals, forecasts, alphas):
    if not alphas:
        return None, NO_ALPHA
    out = []
    for a in alphas:
        r, e = conformal_predict(residuals, forecasts, a)
        if e:
            return None, e
        out.append({k: r[k] for k in ("coverage", "lower", "upper", "conformity_score")})
    return {"point": list(forecasts), "intervals": out}, None


def normalized(difficulty):
    mean = seq_sum(difficulty) / float(len(difficulty))
    return [d / mean for d in difficulty]


def conformal_predict_adaptive(residuals, forecasts, difficulty, alpha):
    if len(forecasts) != len(difficulty):
        return None, f"Invalid input: Forecasts and difficulty must have the same length: {len(forecasts)} vs {len(difficulty)}"
    if any(d <= 0.0 for d in difficulty):
        return None, DIFFICULTY
    s, e = conformal_quantile(residuals, alpha)
    if e:
        return None, e
    nd = normalized(difficulty)
    return {"point": list(forecasts), "lower": [f - s * d for f, d in zip(forecasts, nd)], "upper": [f + s * d for f, d in zip(forecasts, nd)],
            "coverage": 1.0 - alpha, "conformity_score": s, "method": "adaptive_conformal"}, None


def asymmetric_margins(residuals, alpha):
    """(lower_margin, upper_margin) of conformal.rs:380-410 / 796-836."""
    half = alpha / 2.0
    pos = sorted(r for r in residuals if r > 0.0)
    neg = sorted(abs(r) for r in residuals if r < 0.0)
    up = score(pos, half) if pos else 0.0
    lo = score(neg, half) if neg else 0.0
    return lo, up


def conformal_predict_asymmetric(residuals, forecasts, alpha):
    if not residuals:
        return None, EMPTY
    if not alpha_ok(alpha):
        return None, ALPHA_V1
    lo, up = asymmetric_margins(residuals, alpha)
    return {"point": list(forecasts), "lower": [f - lo for f in forecasts], "upper": [f + up for f in forecasts], "coverage": 1.0 - alpha,
            "conformity_score": (up + lo) / 2.0, "method": "asymmetric_conformal"}, None


def mean_interval_width(lower, upper):
    widths = [u - l for l, u in zip(lower, upper)]
    if not widths:
        return math.nan
    return seq_sum(widths) / float(len(widths))


# ---------------------------------------------------------------------------------------------------------------------------
# v2: learn / apply / conformalize
# ---------------------------------------------------------------------------------------------------------------------------
def conformal_learn(residuals, alphas, method="symmetric", strategy="split", difficulty=None):
    if not residuals:
        return None, EMPTY
    if not alphas:
        return None, NO_ALPHA
    for a in alphas:
        if not alpha_ok(a):
            return None, f"Invalid input: Alpha must be in (0, 1), got {show(a)}"
    if method == "adaptive":
        if difficulty is None:
            return None, NEED_DIFFICULTY
        if len(difficulty) != len(residuals):
            return None, f"Invalid input: Difficulty length ({len(difficulty)}) must match residuals length ({len(residuals)})"
        if any(d <= 0.0 for d in difficulty):
            return None, DIFFICULTY
    if strategy == "jackknife+" and method == "asymmetric":
        return None, JACKKNIFE_ASYM
    s_abs = sorted_abs(residuals)
    lower, upper = [], []
    if strategy == "jackknife+" or method in ("symmetric", "adaptive"):
        for a in alphas:
            v = score(s_abs, a)
            lower.append(v)
            upper.append(v)
    else:
        for a in alphas:
            lo, up = asymmetric_margins(residuals, a)
            lower.append(lo)
            upper.append(up)
    state = list(s_abs) if strategy == "jackknife+" else lower + upper
    return {"method": method, "strategy": strategy, "alphas": list(alphas), "state_vector": state, "scores_lower": lower,
            "scores_upper": upper, "n_residuals": len(residuals)}, None


def conformal_apply(forecasts, profile, difficulty=None):
    if not forecasts:
        return None, NO_FORECAST
    adaptive = profile["method"] == "adaptive"
    if adaptive:
        if difficulty is None:
            return None, NEED_DIFFICULTY
        if len(difficulty) != len(forecasts):
            return None, f"Invalid input: Difficulty length ({len(difficulty)}) must match forecasts length ({len(forecasts)})"
        if any(d <= 0.0 for d in difficulty):
            return None, DIFFICULTY
    nd = normalized(difficulty) if adaptive else None
    lower, upper = [], []
    for k, a in enumerate(profile["alphas"]):
        if profile["strategy"] == "jackknife+":
            sl = su = score(profile["state_vector"], a)
        else:
            sl, su = profile["scores_lower"][k], profile["scores_upper"][k]
        if adaptive:
            lower.append([f - sl * d for f, d in zip(forecasts, nd)])
            upper.append([f + su * d for f, d in zip(forecasts, nd)])
        else:
            lower.append([f - sl for f in forecasts])
            upper.append([f + su for f in forecasts])
    return {"point": list(forecasts), "lower": lower, "upper": upper, "coverage": [1.0 - a for a in profile["alphas"]],
            "method": profile["method"]}, None


def conformalize(residuals, forecasts, alphas, method="symmetric", strategy="split", difficulty_cal=None, difficulty_pred=None):
    p, e = conformal_learn(residuals, alphas, method, strategy, difficulty_cal)
    if e:
        return None, e
    return conformal_apply(forecasts, p, difficulty_pred)


# ---------------------------------------------------------------------------------------------------------------------------
# evaluation
# ---------------------------------------------------------------------------------------------------------------------------
def _lengths(actuals, lower, upper):
    if len(actuals) != len(lower) or len(actuals) != len(upper):
        return f"Invalid input: Length mismatch: actuals={len(actuals)}, lower={len(lower)}, upper={len(upper)}"
    return None


def conformal_coverage(actuals, lower, upper):
    if not actuals:
        return None, EMPTY
    e = _lengths(actuals, lower, upper)
    if e:
        return None, e
    covered = sum(1 for a, l, u in zip(actuals, lower, upper) if a >= l and a <= u)
    return float(covered) / float(len(actuals)), None


def winkler_score(actuals, lower, upper, alpha):
    if not actuals:
        return None, EMPTY
    e = _lengths(actuals, lower, upper)
    if e:
        return None, e
    if not alpha_ok(alpha):
        return None, f"Invalid input: Alpha must be in (0, 1), got {show(alpha)}"
    penalty = 2.0 / alpha if alpha != 0.0 else math.copysign(math.inf, alpha)
    total = 0.0
    for a, l, u in zip(actuals, lower, upper):
        s = u - l
        if a < l:
            s += penalty * (l - a)
        elif a > u:
            s += penalty * (a - u)
        total += s
    return total / float(len(actuals)), None


def conformal_evaluate(actuals, lower, upper, alpha):
    c, e = conformal_coverage(actuals, lower, upper)
    if e:
        return None, e
    w, e = winkler_score(actuals, lower, upper, alpha)
    if e:
        return None, e
    return {"coverage": c, "violation_rate": 1.0 - c, "mean_width": mean_interval_width(lower, upper), "winkler_score": w,
            "n_observations": len(actuals)}, None
