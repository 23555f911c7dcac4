"""Yardsticks for MinT with the shrinkage covariance (Wickramasuriya et al. 2019; Schaefer and Strimmer 2005), pure Python and
numpy; nothing here imports the package under test.  Plans and their parts are those of reconcile_ref.

A residual block is [n_out][n_res] (series-major); X is its participating columns (every bottom in series order, then every
aggregate) as [n_res x n_p].  With v the uncentred column variances and W = lambda diag(v) + (1 - lambda) X^T X / n_res:

  variance_chain         v_c = ((((0.0 + x_0^2) + x_1^2) + ...) / n_res) in fp64, serially: the contract of the variances (bits)
  shrinkage_dense        lambda by the dense pairwise formula of hts' shrink.estim in np.longdouble: the yardstick for lambda
  shrinkage_gram         the same sums through the n_res x n_res Gram matrix, plainly in fp64 numpy: the noise of the problem
  dense_w                W [n_p x n_p] in np.longdouble
  project_longdouble     y~ = S (S^T W^-1 S)^-1 S^T W^-1 yhat with reconcile_ref.cholesky_longdouble: the yardstick for y
  constraint_fp64        the low-rank constraint form the kernels use, plainly in fp64 numpy: the noise
  system_matrix          M = lambda (diag(v_a) + A diag(v_b) A^T) + ((1 - lambda) / n_res) E^T E in a given dtype
"""
from __future__ import annotations

import numpy as np

import reconcile_ref as R


def participants(p):
    return list(p["bottom_col"]) + list(p["agg_cols"])


def variance_chain(p, res):
    """[n_out]: the serial chain for every participating column, 0.0 for an empty one."""
    res = np.asarray(res, dtype=np.float64)
    v = np.zeros(p["n_out"])
    n_res = res.shape[1]
    for c in participants(p):
        acc = 0.0
        for x in res[c].tolist():
            acc = acc + x * x
        v[c] = acc / float(n_res)
    return v


def _x(p, res, dtype):
    return np.asarray(res, dtype=np.float64)[participants(p)].T.astype(dtype)


def shrinkage_dense(p, res):
    """shrink.estim of the hts package with the diagonal target, every pair of columns, in np.longdouble."""
    X = _x(p, res, np.longdouble)
    T, N = X.shape
    covm = X.T @ X / T
    xs = X / np.sqrt(np.diag(covm))
    corm = xs.T @ xs / T
    v = (1 / np.longdouble(T * (T - 1))) * ((xs ** 2).T @ (xs ** 2) - (xs.T @ xs) ** 2 / T)
    np.fill_diagonal(v, 0)
    d = (corm - np.eye(N, dtype=np.longdouble)) ** 2
    np.fill_diagonal(d, 0)
    return np.longdouble(min(max(v.sum() / d.sum(), 0), 1)), np.longdouble(v.sum() / d.sum())


def shrinkage_gram(p, res):
    """The same sums collapsed into the n_res x n_res Gram matrix of the scaled residuals, in plain fp64."""
    X = _x(p, res, np.float64)
    T, N = X.shape
    v = (X ** 2).sum(0) / T
    xs = X / np.sqrt(v)
    G = xs @ xs.T
    fro, q, f4 = (G ** 2).sum(), (np.diag(G) ** 2).sum(), (xs ** 4).sum()
    sum_v = ((q - f4) - (fro - N * T * T) / T) / (T * (T - 1))
    sum_d = fro / T ** 2 - N
    if not (np.isfinite(sum_d) and sum_d > 0):
        return 1.0
    return float(min(max(sum_v / sum_d, 0.0), 1.0))


def dense_w(p, res, lam):
    X = _x(p, res, np.longdouble)
    covm = X.T @ X / X.shape[0]
    lam = np.longdouble(lam)
    return lam * np.diag(np.diag(covm)) + (1 - lam) * covm


def project_longdouble(p, W, yhat):
    """The projection form with a full W, in np.longdouble; a column that takes no part is returned unchanged."""
    part = participants(p)
    S = R._summing(p, np.longdouble)
    Y = np.asarray(yhat, dtype=np.float64)[part].astype(np.longdouble)
    Lw = R.cholesky_longdouble(np.asarray(W, dtype=np.longdouble))
    WiS = R.solve_cholesky_longdouble(Lw, S)
    WiY = R.solve_cholesky_longdouble(Lw, Y)
    b = R.solve_cholesky_longdouble(R.cholesky_longdouble(S.T @ WiS), S.T @ WiY)
    out = np.array(yhat, dtype=np.float64, copy=True)
    out[part] = (S @ b).astype(np.float64)
    return out


def incoherence(p, res, dtype=np.float64):
    """E [n_res x n_agg] = X_a - X_b A^T."""
    res = np.asarray(res, dtype=np.float64).astype(dtype)
    return (res[p["agg_cols"]] - p["A"].astype(dtype) @ res[p["bottom_col"]]).T


def system_matrix(p, res, lam, v, dtype=np.float64):
    E = incoherence(p, res, dtype)
    lam = dtype(lam)
    return lam * R.system_matrix(p, np.asarray(v, dtype=dtype), dtype) + ((1 - lam) / dtype(E.shape[0])) * (E.T @ E)


def constraint_fp64(p, res, lam, yhat):
    """The low-rank constraint form plainly in fp64 numpy."""
    out = np.array(yhat, dtype=np.float64, copy=True)
    if not p["agg_cols"]:
        return out
    res = np.asarray(res, dtype=np.float64)
    T = res.shape[1]
    A = p["A"].astype(np.float64)
    Xb = res[p["bottom_col"]].T
    v = (res ** 2).sum(1) / T
    E = incoherence(p, res)
    M = system_matrix(p, res, lam, v)
    yb, ya = out[p["bottom_col"]], out[p["agg_cols"]]
    mu = np.linalg.solve(M, ya - A @ yb)
    g = E @ mu
    b = yb + lam * v[p["bottom_col"]][:, None] * (A.T @ mu) - ((1 - lam) / T) * (Xb.T @ g)
    out[p["bottom_col"]] = b
    out[p["agg_cols"]] = A @ b
    return out
