"""Yardsticks for the reconciliation of hierarchy forecasts, pure Python and numpy; nothing here imports the package under test.

A plan is (col_offsets, members) as hierarchy_ref.plan returns it.  The bottom column of series s is the one column whose member
list is exactly [s]; every other column with members is an aggregate; an empty column takes no part.  With S the summing matrix of
the participating columns (row c: how often each series occurs among the members of c) and W = diag(w) the methods are

  (a) project_exact      y~ = S (S^T W^-1 S)^-1 S^T W^-1 yhat   in exact rational arithmetic (doubles are rationals)
  (b) project_longdouble the same in np.longdouble, with a hand-written Cholesky
  (c) constraint_fp64    b~ = yhat_b + W_b A^T (W_a + A W_b A^T)^-1 (yhat_a - A yhat_b),  y~_a = A b~   plainly in fp64 numpy:
                         the form the kernels use, evaluated without their fixed orders -- the noise of the problem

(Hyndman et al. 2011 for w = 1; Wickramasuriya et al. 2019 for a diagonal W.)  All three take and return blocks [n_out][n_rows]
(series-major); a column that takes no part is returned unchanged.
"""
from __future__ import annotations

from fractions import Fraction

import numpy as np

METHODS = ("bottom_up", "ols", "wls_struct", "wls_var")


def parts(col_offsets, members, n_series):
    """The Python transpose of a plan: bottom_col [n_series], agg_cols ascending, leaf lists (for each series the aggregate INDICES
    that hold it, ascending, once per occurrence), the struct weights, and A [n_agg][n_series] as integer counts.  ValueError names
    what a plan lacks."""
    n_out = len(col_offsets) - 1
    cols = [list(members[col_offsets[c]:col_offsets[c + 1]]) for c in range(n_out)]
    for c, ms in enumerate(cols):
        for s in ms:
            if not 0 <= s < n_series:
                raise ValueError(f"a member of column {c} is outside [0, {n_series})")
    bottom = [-1] * n_series
    for c, ms in enumerate(cols):
        if len(ms) == 1:
            if bottom[ms[0]] >= 0:
                raise ValueError(f"series {ms[0]} has two bottom columns")
            bottom[ms[0]] = c
    for s in range(n_series):
        if bottom[s] < 0:
            raise ValueError(f"series {s} has no bottom column")
    aggs = [c for c, ms in enumerate(cols) if len(ms) > 1]
    leaf = [[] for _ in range(n_series)]
    A = np.zeros((len(aggs), n_series), dtype=np.int64)
    for i, c in enumerate(aggs):
        for s in cols[c]:
            leaf[s].append(i)
            A[i, s] += 1
    return {"n_out": n_out, "n_series": n_series, "cols": cols, "bottom_col": bottom, "agg_cols": aggs, "leaf": leaf,
            "struct_weights": [float(len(ms)) for ms in cols], "A": A}


def method_weights(p, method, weights=None):
    """One weight per column [n_out] for a method (bottom_up: None)."""
    if method == "bottom_up":
        return None
    if method == "ols":
        return np.ones(p["n_out"])
    if method == "wls_struct":
        return np.array(p["struct_weights"])
    return np.asarray(weights, dtype=np.float64)


def chain(values):
    """((0.0 + v0) + v1) + ... in fp64."""
    acc = 0.0
    for v in values:
        acc = acc + float(v)
    return acc


def bottom_up(p, yhat):
    """The bottoms keep their bits, every aggregate is the chain over its members in plan order, an empty column is copied."""
    y = np.array(yhat, dtype=np.float64, copy=True)
    for c in p["agg_cols"]:
        for t in range(y.shape[1]):
            y[c, t] = chain(yhat[p["bottom_col"][s], t] for s in p["cols"][c])
    return y


def coherent_to_the_bit(p, y):
    """Every aggregate of y equals the chain over y's own bottoms: the boolean per (aggregate, row), NaN equal to NaN."""
    ok = np.ones((len(p["agg_cols"]), y.shape[1]), dtype=bool)
    for i, c in enumerate(p["agg_cols"]):
        for t in range(y.shape[1]):
            want = chain(y[p["bottom_col"][s], t] for s in p["cols"][c])
            got = y[c, t]
            ok[i, t] = (np.isnan(want) and np.isnan(got)) or np.float64(want).tobytes() == np.float64(got).tobytes()
    return ok


def _participants(p):
    return list(p["bottom_col"]) + list(p["agg_cols"])


def _summing(p, dtype):
    n = p["n_series"]
    S = np.zeros((n + len(p["agg_cols"]), n), dtype=dtype)
    for s in range(n):
        S[s, s] = 1
    S[n:, :] = p["A"]
    return S


def project_exact(p, w, yhat):
    """(a): Gaussian elimination on S^T W^-1 S b = S^T W^-1 yhat over the rationals; returns fp64 (each entry rounded once)."""
    n = p["n_series"]
    part = _participants(p)
    S = [[Fraction(int(v)) for v in row] for row in _summing(p, np.int64)]
    wi = [1 / Fraction(float(w[c])) for c in part]
    N = [[sum(S[k][i] * wi[k] * S[k][j] for k in range(len(part))) for j in range(n)] for i in range(n)]
    out = np.array(yhat, dtype=np.float64, copy=True)
    rows = out.shape[1]
    rhs = [[sum(S[k][i] * wi[k] * Fraction(float(yhat[part[k], t])) for k in range(len(part))) for t in range(rows)] for i in range(n)]
    for k in range(n):                                          # N is symmetric positive definite: no pivoting needed
        piv = N[k][k]
        for i in range(k + 1, n):
            f = N[i][k] / piv
            if f == 0:
                continue
            for j in range(k, n):
                N[i][j] -= f * N[k][j]
            for t in range(rows):
                rhs[i][t] -= f * rhs[k][t]
    b = [[Fraction(0)] * rows for _ in range(n)]
    for k in reversed(range(n)):
        for t in range(rows):
            b[k][t] = (rhs[k][t] - sum(N[k][j] * b[j][t] for j in range(k + 1, n))) / N[k][k]
    for k, c in enumerate(part):
        for t in range(rows):
            out[c, t] = float(sum(S[k][j] * b[j][t] for j in range(n) if S[k][j] != 0))
    return out


def cholesky_longdouble(M):
    """Lower Cholesky factor in np.longdouble, row by row (Cholesky-Banachiewicz)."""
    n = M.shape[0]
    L = np.zeros((n, n), dtype=np.longdouble)
    for i in range(n):
        for j in range(i):
            L[i, j] = (M[i, j] - np.dot(L[i, :j], L[j, :j])) / L[j, j]
        d = M[i, i] - np.dot(L[i, :i], L[i, :i])
        if not d > 0:
            raise ValueError(f"pivot {i} is not positive")
        L[i, i] = np.sqrt(d)
    return L


def solve_cholesky_longdouble(L, B):
    n = L.shape[0]
    Z = np.array(B, dtype=np.longdouble, copy=True)
    for i in range(n):
        Z[i] = (Z[i] - L[i, :i] @ Z[:i]) / L[i, i]
    for i in reversed(range(n)):
        Z[i] = (Z[i] - L[i + 1:, i] @ Z[i + 1:]) / L[i, i]
    return Z


def project_longdouble(p, w, yhat):
    """(b): the projection form in np.longdouble."""
    part = _participants(p)
    S = _summing(p, np.longdouble)
    wi = 1 / np.asarray(w, dtype=np.longdouble)[part]
    Y = np.asarray(yhat, dtype=np.float64)[part].astype(np.longdouble)
    N = S.T @ (wi[:, None] * S)
    b = solve_cholesky_longdouble(cholesky_longdouble(N), S.T @ (wi[:, None] * Y))
    out = np.array(yhat, dtype=np.float64, copy=True)
    out[part] = (S @ b).astype(np.float64)
    return out


def system_matrix(p, w, dtype=np.float64):
    """M = diag(w_a) + A diag(w_b) A^T."""
    w = np.asarray(w, dtype=dtype)
    A = p["A"].astype(dtype)
    return np.diag(w[p["agg_cols"]]) + (A * w[p["bottom_col"]][None, :]) @ A.T


def system_matrix_exact(p, w):
    """M over the rationals, as nested lists."""
    na, n = len(p["agg_cols"]), p["n_series"]
    wb = [Fraction(float(w[c])) for c in p["bottom_col"]]
    A = p["A"]
    M = [[sum(int(A[i, s]) * wb[s] * int(A[j, s]) for s in range(n) if A[i, s] and A[j, s]) for j in range(na)] for i in range(na)]
    for i, c in enumerate(p["agg_cols"]):
        M[i][i] += Fraction(float(w[c]))
    return M


def constraint_fp64(p, w, yhat):
    """(c): the constraint form plainly in fp64 numpy."""
    out = np.array(yhat, dtype=np.float64, copy=True)
    if not p["agg_cols"]:
        return out
    A = p["A"].astype(np.float64)
    w = np.asarray(w, dtype=np.float64)
    yb, ya = out[p["bottom_col"]], out[p["agg_cols"]]
    lam = np.linalg.solve(system_matrix(p, w), ya - A @ yb)
    b = yb + w[p["bottom_col"]][:, None] * (A.T @ lam)
    out[p["bottom_col"]] = b
    out[p["agg_cols"]] = A @ b
    return out


def allowance(p, w, yhat, exact_limit=40):
    """The tolerance of a case and its yardstick: 16 x the larger of (c)'s own deviation from the yardstick and eps * max|yhat| over
    the participating columns; the yardstick is (a) up to `exact_limit` output columns, (b) above."""
    part = _participants(p)
    yard = project_exact(p, w, yhat) if p["n_out"] <= exact_limit else project_longdouble(p, w, yhat)
    noise = float(np.max(np.abs(constraint_fp64(p, w, yhat)[part] - yard[part]))) if part else 0.0
    scale = float(np.max(np.abs(np.asarray(yhat)[part]))) if part else 0.0
    return yard, 16.0 * max(noise, np.finfo(np.float64).eps * scale)
