"""Device-resident batches: the series block lives in HBM as a torch tensor (plumbing only:
allocation, streams, torch.distributed); all arithmetic is in libanofox_fcst_hip.so.

Layout: time-major fp64 block Y[t, s] of shape [t_max, ld], ld = n_series rounded up to 64, so
the 64 lanes of a wave read one 512-byte row segment per time step.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import lib as _lib


def pack_time_major(series_major: np.ndarray, ld: int | None = None) -> np.ndarray:
    """[n, T] series-major host array -> [T, ld] time-major (zero padded)."""
    n, T = series_major.shape
    ld = ld or (n + 63) // 64 * 64
    out = np.zeros((T, ld), dtype=np.float64)
    out[:, :n] = series_major.T
    return out


def prepare_block(y: torch.Tensor, lengths: torch.Tensor, valid: torch.Tensor | None = None, dates: torch.Tensor | None = None, *,
                  n_series: int | None = None, gaps: bool = False, frequency_micros: int = 0, frequency_type: str = "FIXED",
                  trim: str = "none", fill: str = "none", fill_value: float = 0.0, t_out: int | None = None,
                  count_only: bool = False, out: dict | None = None, stream: torch.cuda.Stream | None = None) -> dict:
    """anofox_hip_prepare_device on torch tensors: raw block in, clean block out, no host round trip.

    y [t_rows, ld] fp64, valid [t_rows, ld] uint8 or bool (0 = NULL; None: all valid), dates [t_rows, ld] int64 microseconds (needed
    for gaps=True), lengths int32 [>= n_series] -- all on one HIP device, contiguous.  The stages run in the fixed order gaps, trim
    ("none" / "leading" / "trailing" / "edge"), fill ("none" / "const" / "forward" / "backward" / "mean" / "interpolate").  Without
    t_out a count call sizes the output block first (one device-to-host read of the largest length).  `out` may bring the output
    tensors "y", "valid", "dates" ([t_out, ld]) and "lengths" (int32 [ld]); else they are allocated, zero-filled.

    Returns {"y", "valid", "dates" (None without input dates), "lengths", "figures" (int64 [8, ld], rows lib.PREP_FIGURES),
    "minmax" (fp64 [2, ld]), "t_out"}; with count_only the blocks are None.  DeviceBatch(n_series, t_out, opts).set_block(r["y"],
    r["lengths"]) takes the result as it is (after a fill that leaves no NULL)."""
    L = _lib.load()
    assert y.dtype == torch.float64 and y.is_cuda and y.is_contiguous() and y.dim() == 2
    t_rows, ld = int(y.shape[0]), int(y.shape[1])
    n = ld if n_series is None else int(n_series)
    assert lengths.dtype == torch.int32 and lengths.is_cuda and lengths.is_contiguous() and lengths.numel() >= n
    dev = y.device
    if valid is not None:
        if valid.dtype == torch.bool:
            valid = valid.to(torch.uint8)
        assert valid.dtype == torch.uint8 and valid.is_cuda and valid.is_contiguous() and tuple(valid.shape) == (t_rows, ld)
    if dates is not None:
        assert dates.dtype == torch.int64 and dates.is_cuda and dates.is_contiguous() and tuple(dates.shape) == (t_rows, ld)
    if L.anofox_hip_set_device(dev.index or 0) != 0:
        raise RuntimeError(f"hipSetDevice({dev.index or 0}) failed")
    opts = _lib.make_prep_options(gaps, frequency_micros, frequency_type, trim, fill, fill_value)
    out = dict(out or {})
    len_out = out.get("lengths")
    if len_out is None:
        len_out = torch.zeros(ld, dtype=torch.int32, device=dev)
    figures = torch.zeros((8, ld), dtype=torch.int64, device=dev)
    minmax = torch.zeros((2, ld), dtype=torch.float64, device=dev)
    st = stream if stream is not None else torch.cuda.current_stream(dev)
    ptr = lambda t: t.data_ptr() if t is not None else None

    def call(rows, yo, vo, do):
        err = _lib.AnofoxError()
        ok = L.anofox_hip_prepare_device(y.data_ptr(), ptr(valid), ptr(dates), ld, lengths.data_ptr(), n, t_rows, C.byref(opts),
                                         C.sizeof(opts), rows, ptr(yo), ptr(vo), ptr(do), len_out.data_ptr(), figures.data_ptr(),
                                         minmax.data_ptr(), C.c_void_p(st.cuda_stream), C.byref(err))
        if not ok:
            raise RuntimeError(f"anofox_hip_prepare_device failed: [{err.code}] {err.message.decode()}")

    yo, vo, do = out.get("y"), out.get("valid"), out.get("dates")
    if t_out is None and yo is not None:
        t_out = int(yo.shape[0])
    if t_out is None or count_only:
        call(0, None, None, None)
        if count_only:
            return {"y": None, "valid": None, "dates": None, "lengths": len_out, "figures": figures, "minmax": minmax, "t_out": None}
        t_out = max(1, int(len_out[:n].max().item())) if n else 1
    t_out = int(t_out)
    if yo is None:
        yo = torch.zeros((t_out, ld), dtype=torch.float64, device=dev)
    if vo is None:
        vo = torch.zeros((t_out, ld), dtype=torch.uint8, device=dev)
    if do is None and dates is not None:
        do = torch.zeros((t_out, ld), dtype=torch.int64, device=dev)
    for t, dt in ((yo, torch.float64), (vo, torch.uint8), (do, torch.int64)):
        assert t is None or (t.dtype == dt and t.is_cuda and t.is_contiguous() and tuple(t.shape) == (t_out, ld))
    call(t_out, yo, vo, do)
    return {"y": yo, "valid": vo, "dates": do if dates is not None else None, "lengths": len_out, "figures": figures, "minmax": minmax,
            "t_out": t_out}


def quality_block(y: torch.Tensor, lengths: torch.Tensor, valid: torch.Tensor | None = None, *, n_series: int | None = None,
                  stream: torch.cuda.Stream | None = None) -> dict:
    """anofox_hip_quality_device on torch tensors: the eight ts_data_quality figures of every series of a block, no host copy.

    y [t_rows, ld] fp64, valid [t_rows, ld] uint8 or bool (0 = NULL; None: all valid), lengths int32 [>= n_series], on one HIP device,
    contiguous -- what prepare_block returns: r = prepare_block(...); q = quality_block(r["y"], r["lengths"], r["valid"]); then filter
    on q["scores"] / q["status"] and hand the kept columns to DeviceBatch.set_block.

    Returns {"scores": fp64 [5, ld], rows lib.QUALITY_FP_FIELDS; "figures": int64 [4, ld], rows lib.QUALITY_INT_FIELDS (n_gaps,
    n_missing, is_constant as 0 / 1, status: lib.QUALITY_OK, or lib.QUALITY_NAN with five NaN scores)}.  Columns s >= n_series hold
    NaN and -1."""
    L = _lib.load()
    assert y.dtype == torch.float64 and y.is_cuda and y.is_contiguous() and y.dim() == 2
    t_rows, ld = int(y.shape[0]), int(y.shape[1])
    n = ld if n_series is None else int(n_series)
    assert lengths.dtype == torch.int32 and lengths.is_cuda and lengths.is_contiguous() and lengths.numel() >= n
    dev = y.device
    if valid is not None:
        if valid.dtype == torch.bool:
            valid = valid.to(torch.uint8)
        assert valid.dtype == torch.uint8 and valid.is_cuda and valid.is_contiguous() and tuple(valid.shape) == (t_rows, ld)
    if L.anofox_hip_set_device(dev.index or 0) != 0:
        raise RuntimeError(f"hipSetDevice({dev.index or 0}) failed")
    scores = torch.full((5, ld), float("nan"), dtype=torch.float64, device=dev)
    figures = torch.full((4, ld), -1, dtype=torch.int64, device=dev)
    st = stream if stream is not None else torch.cuda.current_stream(dev)
    err = _lib.AnofoxError()
    ok = L.anofox_hip_quality_device(y.data_ptr(), valid.data_ptr() if valid is not None else None, ld, lengths.data_ptr(), n, t_rows,
                                     scores.data_ptr(), figures.data_ptr(), C.c_void_p(st.cuda_stream), C.byref(err))
    if not ok:
        raise RuntimeError(f"anofox_hip_quality_device failed: [{err.code}] {err.message.decode()}")
    return {"scores": scores, "figures": figures}


def features_block(y: torch.Tensor, lengths: torch.Tensor, valid: torch.Tensor | None = None, *, n_series: int | None = None,
                   families=None, out: dict | None = None, stream: torch.cuda.Stream | None = None) -> dict:
    """anofox_hip_features_device on torch tensors: the 117 features of every series of a block, no host copy.

    y [t_rows, ld] fp64 (t_rows <= lib.FEATURES_MAX_ROWS), valid [t_rows, ld] uint8 or bool (0 = NULL; None: all valid), lengths int32
    [>= n_series], on one HIP device, contiguous -- what prepare_block returns.  `families`: None for all five kernels, or names out of
    lib.FEATURES_FAMILIES (only their rows are written; "chains" writes present and status).  `out` may bring "features" and "figures".

    Returns {"features": fp64 [117, ld], rows in the order of lib.feature_names(), NaN where the source inserts nothing; "figures":
    int64 [3, ld]: the two presence words (bit i % 64 of word i // 64 for feature i) and the status (lib.FEATURES_OK, FEATURES_EMPTY,
    FEATURES_NAN)}.  Columns s >= n_series hold NaN and -1 (in tensors the call allocates)."""
    L = _lib.load()
    assert y.dtype == torch.float64 and y.is_cuda and y.is_contiguous() and y.dim() == 2
    t_rows, ld = int(y.shape[0]), int(y.shape[1])
    n = ld if n_series is None else int(n_series)
    assert lengths.dtype == torch.int32 and lengths.is_cuda and lengths.is_contiguous() and lengths.numel() >= n
    dev = y.device
    if valid is not None:
        if valid.dtype == torch.bool:
            valid = valid.to(torch.uint8)
        assert valid.dtype == torch.uint8 and valid.is_cuda and valid.is_contiguous() and tuple(valid.shape) == (t_rows, ld)
    if L.anofox_hip_set_device(dev.index or 0) != 0:
        raise RuntimeError(f"hipSetDevice({dev.index or 0}) failed")
    out = dict(out or {})
    feats, figures = out.get("features"), out.get("figures")
    if feats is None:
        feats = torch.full((_lib.N_FEATURES, ld), float("nan"), dtype=torch.float64, device=dev)
    if figures is None:
        figures = torch.full((3, ld), -1, dtype=torch.int64, device=dev)
    assert feats.dtype == torch.float64 and feats.is_cuda and feats.is_contiguous() and tuple(feats.shape) == (_lib.N_FEATURES, ld)
    assert figures.dtype == torch.int64 and figures.is_cuda and figures.is_contiguous() and tuple(figures.shape) == (3, ld)
    mask = sum(1 << _lib.FEATURES_FAMILIES.index(f) for f in set(families)) if families is not None else (1 << len(_lib.FEATURES_FAMILIES)) - 1
    st = stream if stream is not None else torch.cuda.current_stream(dev)
    err = _lib.AnofoxError()
    ok = L.anofox_hip_features_families_device(y.data_ptr(), valid.data_ptr() if valid is not None else None, ld, lengths.data_ptr(), n,
                                               t_rows, mask, feats.data_ptr(), figures.data_ptr(), C.c_void_p(st.cuda_stream), C.byref(err))
    if not ok:
        raise RuntimeError(f"anofox_hip_features_device failed: [{err.code}] {err.message.decode()}")
    return {"features": feats, "figures": figures}


def pelt_block(y: torch.Tensor, lengths: torch.Tensor, min_size: int = 2, penalty: float = 0.0, *, n_series: int | None = None,
               stream: torch.cuda.Stream | None = None):
    """anofox_hip_pelt_device on torch tensors: the PELT changepoints (L2 cost) of every series of a block, nothing read back.

    y [t_rows, ld] fp64, lengths int32 [>= n_series], on one HIP device, contiguous.  One min_size and one penalty for the block; a
    penalty that is not > 0 means 2 ln n of each series.

    Returns device tensors (flags, counts, cost): flags uint8 [t_rows, ld], 1 at a changepoint and 0 elsewhere (rows beyond a
    series' length and columns s >= n_series hold 0 too: the block is allocated zeroed), counts int32 [ld] (-1 in columns
    s >= n_series) and cost fp64 [ld] (NaN there)."""
    L = _lib.load()
    assert y.dtype == torch.float64 and y.is_cuda and y.is_contiguous() and y.dim() == 2
    t_rows, ld = int(y.shape[0]), int(y.shape[1])
    n = ld if n_series is None else int(n_series)
    assert lengths.dtype == torch.int32 and lengths.is_cuda and lengths.is_contiguous() and lengths.numel() >= n
    dev = y.device
    if L.anofox_hip_set_device(dev.index or 0) != 0:
        raise RuntimeError(f"hipSetDevice({dev.index or 0}) failed")
    flags = torch.zeros((t_rows, ld), dtype=torch.uint8, device=dev)
    counts = torch.full((ld,), -1, dtype=torch.int32, device=dev)
    cost = torch.full((ld,), float("nan"), dtype=torch.float64, device=dev)
    st = stream if stream is not None else torch.cuda.current_stream(dev)
    err = _lib.AnofoxError()
    ok = L.anofox_hip_pelt_device(y.data_ptr(), ld, lengths.data_ptr(), n, t_rows, int(min_size), float(penalty), flags.data_ptr(),
                                  counts.data_ptr(), cost.data_ptr(), C.c_void_p(st.cuda_stream), C.byref(err))
    if not ok:
        raise RuntimeError(f"anofox_hip_pelt_device failed: [{err.code}] {err.message.decode()}")
    return flags, counts, cost


def seasonality_block(y: torch.Tensor, lengths: torch.Tensor, valid: torch.Tensor | None = None, max_period: int = 0, *,
                      n_series: int | None = None, stream: torch.cuda.Stream | None = None) -> dict:
    """anofox_hip_seasonality_device on torch tensors: the ts_analyze_seasonality figures of every series of a block, no host copy.

    y [t_rows, ld] fp64, valid [t_rows, ld] uint8 or bool (0 = NULL, dropped; None: all valid), lengths int32 [>= n_series], on one HIP
    device, contiguous -- what prepare_block returns.  max_period <= 0: half of each series' length.

    Returns device tensors: {"periods": int32 [5, ld] (strongest first, 0 beyond n_periods), "n_periods", "primary_period", "status"
    (int32 [ld] views; lib.SEASONALITY_OK, or lib.SEASONALITY_SHORT for fewer than 4 values), "strengths", "acf" (fp64 [5, ld]),
    "seasonal_strength", "trend_strength" (fp64 [ld] views), "is_seasonal" (bool [ld]: seasonal_strength > 0.1), and the two blocks
    "figures" (int32 [8, ld], rows lib.SEASONALITY_INT_FIELDS) and "values" (fp64 [12, ld], rows lib.SEASONALITY_FP_FIELDS)}.
    Columns s >= n_series hold -1 and NaN."""
    L = _lib.load()
    assert y.dtype == torch.float64 and y.is_cuda and y.is_contiguous() and y.dim() == 2
    t_rows, ld = int(y.shape[0]), int(y.shape[1])
    n = ld if n_series is None else int(n_series)
    assert lengths.dtype == torch.int32 and lengths.is_cuda and lengths.is_contiguous() and lengths.numel() >= n
    dev = y.device
    if valid is not None:
        if valid.dtype == torch.bool:
            valid = valid.to(torch.uint8)
        assert valid.dtype == torch.uint8 and valid.is_cuda and valid.is_contiguous() and tuple(valid.shape) == (t_rows, ld)
    if L.anofox_hip_set_device(dev.index or 0) != 0:
        raise RuntimeError(f"hipSetDevice({dev.index or 0}) failed")
    figures = torch.full((8, ld), -1, dtype=torch.int32, device=dev)
    values = torch.full((12, ld), float("nan"), dtype=torch.float64, device=dev)
    st = stream if stream is not None else torch.cuda.current_stream(dev)
    err = _lib.AnofoxError()
    ok = L.anofox_hip_seasonality_device(y.data_ptr(), valid.data_ptr() if valid is not None else None, ld, lengths.data_ptr(), n, t_rows,
                                         int(max_period), figures.data_ptr(), values.data_ptr(), C.c_void_p(st.cuda_stream), C.byref(err))
    if not ok:
        raise RuntimeError(f"anofox_hip_seasonality_device failed: [{err.code}] {err.message.decode()}")
    return {"periods": figures[:5], "n_periods": figures[5], "primary_period": figures[6], "status": figures[7],
            "strengths": values[:5], "acf": values[5:10], "seasonal_strength": values[10], "trend_strength": values[11],
            "is_seasonal": values[10] > 0.1, "figures": figures, "values": values}


def _period_search_block(y, lengths, n_series):
    assert y.dtype == torch.float64 and y.is_cuda and y.is_contiguous() and y.dim() == 2
    t_rows, ld = int(y.shape[0]), int(y.shape[1])
    n = ld if n_series is None else int(n_series)
    assert lengths.dtype == torch.int32 and lengths.is_cuda and lengths.is_contiguous() and lengths.numel() >= n
    return t_rows, ld, n


def ssa_period_block(y: torch.Tensor, lengths: torch.Tensor, window_size: int = 0, n_components: int = 0, *, route: str = "auto",
                     n_series: int | None = None, stream: torch.cuda.Stream | None = None) -> dict:
    """anofox_hip_ssa_period_device on torch tensors: the reference's ssa_period for every series of a block, nothing read back.

    y [t_rows, ld] fp64 (t_rows <= 65,536), lengths int32 [>= n_series], on one HIP device, contiguous.  window_size / n_components
    0: n / 3 of each series and 10.  route 'auto' | 'group' (lib.SSA_ROUTES) chooses the lanes per series, never the bits.

    Returns device tensors: {"period", "variance_explained", "n_eigenvalues" (fp64 [ld] views of "figures" [3, ld]), "eigenvalues"
    fp64 [C, ld] with C = lib.ssa_components(n_components), "detected_periods" fp64 [4, ld] (both NaN beyond what exists), "status"
    int32 [ld]: lib.PSEARCH_OK, _TOO_SHORT (fewer than 16 rows) or _OVER_LIMIT (window above 2,048)}.  Columns s >= n_series and
    failed series hold NaN; status is -1 in columns s >= n_series."""
    L = _lib.load()
    t_rows, ld, n = _period_search_block(y, lengths, n_series)
    dev = y.device
    if L.anofox_hip_set_device(dev.index or 0) != 0:
        raise RuntimeError(f"hipSetDevice({dev.index or 0}) failed")
    comps = _lib.ssa_components(n_components)
    figures = torch.full((3, ld), float("nan"), dtype=torch.float64, device=dev)
    eig = torch.full((comps, ld), float("nan"), dtype=torch.float64, device=dev)
    det = torch.full((_lib.SSA_N_DETECTED, ld), float("nan"), dtype=torch.float64, device=dev)
    status = torch.full((ld,), -1, dtype=torch.int32, device=dev)
    st = stream if stream is not None else torch.cuda.current_stream(dev)
    err = _lib.AnofoxError()
    ok = L.anofox_hip_ssa_period_device(y.data_ptr(), ld, lengths.data_ptr(), n, t_rows, int(window_size or 0), int(n_components or 0),
                                        _lib.SSA_ROUTES[route], figures.data_ptr(), eig.data_ptr(), det.data_ptr(), status.data_ptr(),
                                        C.c_void_p(st.cuda_stream), C.byref(err))
    if not ok:
        raise RuntimeError(f"anofox_hip_ssa_period_device failed: [{err.code}] {err.message.decode()}")
    return {"period": figures[0], "variance_explained": figures[1], "n_eigenvalues": figures[2], "figures": figures, "eigenvalues": eig,
            "detected_periods": det, "status": status}


def stl_period_block(y: torch.Tensor, lengths: torch.Tensor, min_period: int = 0, max_period: int = 0, n_candidates: int = 0, *,
                     n_series: int | None = None, stream: torch.cuda.Stream | None = None) -> dict:
    """anofox_hip_stl_period_device on torch tensors: the reference's stl_period for every series of a block, nothing read back.

    y [t_rows, ld] fp64 (t_rows <= 65,536), lengths int32 [>= n_series], on one HIP device, contiguous.  0 means the source's default:
    min_period 4, max_period n / 3 of each series, 20 candidates.

    Returns device tensors: {"period", "seasonal_strength", "trend_strength" (fp64 [ld] views of "figures" [3, ld]), "index" int32 [ld]
    (the winning candidate's place in its list; -1 for a constant series), "candidates" int32 [K, ld] (-1 beyond a series' list) and
    "candidate_strengths" fp64 [K, ld] (NaN beyond it) with K = lib.stl_candidate_count(n_candidates), "status" int32 [ld]:
    lib.PSEARCH_OK, _TOO_SHORT, _STL_RANGE or _STL_NO_CANDIDATE}.  Columns s >= n_series and failed series keep NaN / -1."""
    L = _lib.load()
    t_rows, ld, n = _period_search_block(y, lengths, n_series)
    dev = y.device
    if L.anofox_hip_set_device(dev.index or 0) != 0:
        raise RuntimeError(f"hipSetDevice({dev.index or 0}) failed")
    k = _lib.stl_candidate_count(n_candidates)
    figures = torch.full((3, ld), float("nan"), dtype=torch.float64, device=dev)
    index = torch.full((ld,), -1, dtype=torch.int32, device=dev)
    cands = torch.full((k, ld), -1, dtype=torch.int32, device=dev)
    strengths = torch.full((k, ld), float("nan"), dtype=torch.float64, device=dev)
    status = torch.full((ld,), -1, dtype=torch.int32, device=dev)
    st = stream if stream is not None else torch.cuda.current_stream(dev)
    err = _lib.AnofoxError()
    ok = L.anofox_hip_stl_period_device(y.data_ptr(), ld, lengths.data_ptr(), n, t_rows, int(min_period or 0), int(max_period or 0),
                                        int(n_candidates or 0), figures.data_ptr(), index.data_ptr(), cands.data_ptr(), strengths.data_ptr(),
                                        status.data_ptr(), C.c_void_p(st.cuda_stream), C.byref(err))
    if not ok:
        raise RuntimeError(f"anofox_hip_stl_period_device failed: [{err.code}] {err.message.decode()}")
    return {"period": figures[0], "seasonal_strength": figures[1], "trend_strength": figures[2], "figures": figures, "index": index,
            "candidates": cands, "candidate_strengths": strengths, "status": status}


def matrix_profile_block(y: torch.Tensor, lengths: torch.Tensor, subsequence_length: int = 0, n_best: int = 0, *, profile: bool = True,
                         n_series: int | None = None, stream: torch.cuda.Stream | None = None) -> dict:
    """anofox_hip_matrix_profile_device on torch tensors: the reference's matrix_profile_period for every series of a block, and the
    profile itself, nothing read back.

    y [t_rows, ld] fp64 (t_rows <= 65,536), lengths int32 [>= n_series], on one HIP device, contiguous.  subsequence_length 0: n / 10
    of each series (at least 4, at most n / 4); n_best is the exclusion zone, 0: m / 4 (at least 1).

    Returns device tensors: {"period", "confidence", "n_motifs", "subsequence_length", "best_count", "n_tied" (fp64 [ld] views of
    "figures" [6, ld]; among lags of equal best count the smallest is the period), "status" int32 [ld]: lib.MPROF_OK, _TOO_SHORT
    (fewer than 32 rows) or _OVER_LIMIT (subsequence length above 2,048), and with profile=True "profile" fp64 and "profile_index"
    int32 [lib.matrix_profile_rows(t_rows, subsequence_length), ld]: every subsequence's distance to its nearest neighbour outside
    the exclusion zone and that neighbour's index, NaN / -1 beyond a series' own profile}.  Columns s >= n_series and failed series
    hold NaN / -1; status is -1 in columns s >= n_series."""
    L = _lib.load()
    t_rows, ld, n = _period_search_block(y, lengths, n_series)
    dev = y.device
    if L.anofox_hip_set_device(dev.index or 0) != 0:
        raise RuntimeError(f"hipSetDevice({dev.index or 0}) failed")
    rows = _lib.matrix_profile_rows(t_rows, int(subsequence_length or 0))
    figures = torch.full((len(_lib.MATRIX_PROFILE_FIGURES), ld), float("nan"), dtype=torch.float64, device=dev)
    status = torch.full((ld,), -1, dtype=torch.int32, device=dev)
    prof = torch.full((rows, ld), float("nan"), dtype=torch.float64, device=dev) if profile else None
    index = torch.full((rows, ld), -1, dtype=torch.int32, device=dev) if profile else None
    st = stream if stream is not None else torch.cuda.current_stream(dev)
    err = _lib.AnofoxError()
    ok = L.anofox_hip_matrix_profile_device(y.data_ptr(), ld, lengths.data_ptr(), n, t_rows, int(subsequence_length or 0), int(n_best or 0),
                                            figures.data_ptr(), prof.data_ptr() if profile and rows else None,
                                            index.data_ptr() if profile and rows else None, status.data_ptr(), C.c_void_p(st.cuda_stream),
                                            C.byref(err))
    if not ok:
        raise RuntimeError(f"anofox_hip_matrix_profile_device failed: [{err.code}] {err.message.decode()}")
    out = {name: figures[k] for k, name in enumerate(_lib.MATRIX_PROFILE_FIGURES)}
    out.update({"figures": figures, "status": status})
    if profile:
        out.update({"profile": prof, "profile_index": index})
    return out


def conformal_block(forecast: torch.Tensor, alphas, *, residual: torch.Tensor | None = None, actual: torch.Tensor | None = None,
                    calibration_forecast: torch.Tensor | None = None, valid: torch.Tensor | None = None,
                    lengths: torch.Tensor | None = None, n_groups: int | None = None, method: str = "symmetric",
                    difficulty: torch.Tensor | None = None, series_major: bool = False, calibration_series_major: bool | None = None,
                    want_sorted: bool = False, stream: torch.cuda.Stream | None = None) -> dict:
    """anofox_hip_conformal_learn_device then anofox_hip_conformal_apply_device on torch tensors: calibration residuals in, lower and
    upper blocks out, no host copy.

    The calibration set is `residual`, or `actual` and `calibration_forecast` (the residual is formed on the device as actual -
    forecast); valid (uint8 or bool, 0 = dropped) has the same shape.  A time-major block is [t_rows, ld] with group s in column s; a
    series-major one (calibration_series_major, default: as series_major) is [n_groups, t_rows].  lengths (int32, on the device) gives
    the rows of every group; None: all rows.  `forecast` is the point block the intervals go around: time-major [h, ld], or with
    series_major=True the [n_series, h] layout of DeviceBatch.results()["yhat"]; difficulty (adaptive method) has its shape.

    Returns {"lower", "upper": [n_alphas, *forecast.shape], "scores_lower", "scores_upper": fp64 [n_alphas, ld], "n_kept", "status",
    "apply_status": int32 [n_groups], "sorted": a block shaped like the calibration set (rows 0 .. n_kept - 1 of a group hold its
    ascending |residual|) or None}.  status per group: lib.CONFORMAL_OK / _EMPTY / _NAN, apply_status: _OK / _DIFFICULTY."""
    L = _lib.load()
    cal = residual if residual is not None else actual
    assert cal is not None and (residual is not None or calibration_forecast is not None)
    cal_sm = series_major if calibration_series_major is None else calibration_series_major
    blocks = [t for t in (residual, actual, calibration_forecast) if t is not None]
    for t in blocks + [forecast] + ([difficulty] if difficulty is not None else []):
        assert t.dtype == torch.float64 and t.is_cuda and t.is_contiguous() and t.dim() == 2
    assert all(tuple(t.shape) == tuple(cal.shape) for t in blocks)
    dev = forecast.device
    if valid is not None:
        if valid.dtype == torch.bool:
            valid = valid.to(torch.uint8)
        assert valid.dtype == torch.uint8 and valid.is_cuda and valid.is_contiguous() and tuple(valid.shape) == tuple(cal.shape)
    if cal_sm:
        n_cal, t_rows = int(cal.shape[0]), int(cal.shape[1])
        cs, ct = t_rows, 1
    else:
        t_rows, n_cal = int(cal.shape[0]), int(cal.shape[1])
        cs, ct = 1, n_cal
    if series_major:
        n_f, h = int(forecast.shape[0]), int(forecast.shape[1])
        fs, ft = h, 1
    else:
        h, n_f = int(forecast.shape[0]), int(forecast.shape[1])
        fs, ft = 1, n_f
    n = min(n_cal, n_f) if n_groups is None else int(n_groups)
    assert 0 < n <= n_cal and n <= n_f
    if difficulty is not None:
        assert tuple(difficulty.shape) == tuple(forecast.shape)
    if lengths is None:
        lengths = torch.full((n,), t_rows, dtype=torch.int32, device=dev)
    assert lengths.dtype == torch.int32 and lengths.is_cuda and lengths.is_contiguous() and lengths.numel() >= n
    if L.anofox_hip_set_device(dev.index or 0) != 0:
        raise RuntimeError(f"hipSetDevice({dev.index or 0}) failed")
    al = np.ascontiguousarray(alphas, dtype=np.float64).reshape(-1)
    k = len(al)
    ld = (n + 63) // 64 * 64
    code = _lib.CONFORMAL_METHODS[str(method).lower()]
    sl = torch.full((max(k, 1), ld), float("nan"), dtype=torch.float64, device=dev)
    su = torch.full((max(k, 1), ld), float("nan"), dtype=torch.float64, device=dev)
    kept = torch.zeros(n, dtype=torch.int32, device=dev)
    status = torch.zeros(n, dtype=torch.int32, device=dev)
    apply_status = torch.zeros(n, dtype=torch.int32, device=dev)
    srt = torch.zeros_like(cal) if want_sorted else None
    lower = torch.full((max(k, 1),) + tuple(forecast.shape), float("nan"), dtype=torch.float64, device=dev)
    upper = torch.full((max(k, 1),) + tuple(forecast.shape), float("nan"), dtype=torch.float64, device=dev)
    st = stream if stream is not None else torch.cuda.current_stream(dev)
    ptr = lambda t: t.data_ptr() if t is not None else None
    err = _lib.AnofoxError()
    ok = L.anofox_hip_conformal_learn_device(ptr(residual), ptr(actual), ptr(calibration_forecast), ptr(valid), cs, ct, lengths.data_ptr(), n,
                                             t_rows, al.ctypes.data, k, code, sl.data_ptr(), su.data_ptr(), ld, ptr(srt), kept.data_ptr(),
                                             status.data_ptr(), C.c_void_p(st.cuda_stream), C.byref(err))
    if not ok:
        raise RuntimeError(f"anofox_hip_conformal_learn_device failed: [{err.code}] {err.message.decode()}")
    ok = L.anofox_hip_conformal_apply_device(forecast.data_ptr(), ptr(difficulty), fs, ft, None, n, h, sl.data_ptr(), su.data_ptr(), ld, k, code,
                                             lower.data_ptr(), upper.data_ptr(), forecast.numel(), apply_status.data_ptr(),
                                             C.c_void_p(st.cuda_stream), C.byref(err))
    if not ok:
        raise RuntimeError(f"anofox_hip_conformal_apply_device failed: [{err.code}] {err.message.decode()}")
    return {"lower": lower, "upper": upper, "scores_lower": sl, "scores_upper": su, "n_kept": kept, "status": status,
            "apply_status": apply_status, "sorted": srt}


def backtest_expand_block(y: torch.Tensor, lengths: torch.Tensor, folds, *, n_series: int | None = None,
                          stream: torch.cuda.Stream | None = None) -> dict:
    """anofox_hip_backtest_expand_device on torch tensors: the training windows of every (series, fold) pair as one block, made once
    and shared by every method that is backtested on it (backtest_block(..., expanded=...), select_block).

    Returns {"train": fp64 [t_train, ld_pairs], "len_pairs", "n_test": int32 [ld_pairs], "t_train", "n_pairs", "ld_pairs", "n_folds"}."""
    L = _lib.load()
    assert y.dtype == torch.float64 and y.is_cuda and y.is_contiguous() and y.dim() == 2
    t_rows, ld = int(y.shape[0]), int(y.shape[1])
    n = ld if n_series is None else int(n_series)
    assert lengths.dtype == torch.int32 and lengths.is_cuda and lengths.is_contiguous() and lengths.numel() >= n
    dev = y.device
    if L.anofox_hip_set_device(dev.index or 0) != 0:
        raise RuntimeError(f"hipSetDevice({dev.index or 0}) failed")
    F = len(folds)
    tab = _lib.make_folds(folds)
    t_train, n_pairs, ld_pairs = _lib.backtest_sizes(tab, F, n)
    try:
        train = torch.empty((t_train, ld_pairs), dtype=torch.float64, device=dev)
    except torch.cuda.OutOfMemoryError as e:
        raise RuntimeError(f"the expanded backtest block of {t_train} x {ld_pairs} values needs {t_train * ld_pairs * 8} bytes of device "
                           "memory") from e
    len_pairs = torch.empty(ld_pairs, dtype=torch.int32, device=dev)
    n_test = torch.empty(ld_pairs, dtype=torch.int32, device=dev)
    st = stream if stream is not None else torch.cuda.current_stream(dev)
    err = _lib.AnofoxError()
    ok = L.anofox_hip_backtest_expand_device(y.data_ptr(), ld, lengths.data_ptr(), n, t_rows, tab, F, t_train, train.data_ptr(), ld_pairs,
                                             len_pairs.data_ptr(), n_test.data_ptr(), C.c_void_p(st.cuda_stream), C.byref(err))
    if not ok:
        raise RuntimeError(f"anofox_hip_backtest_expand_device failed: [{err.code}] {err.message.decode()}")
    return {"train": train, "len_pairs": len_pairs, "n_test": n_test, "t_train": t_train, "n_pairs": n_pairs, "ld_pairs": ld_pairs,
            "n_folds": F}


def backtest_block(y: torch.Tensor, lengths: torch.Tensor, opts: _lib.ForecastOptions, folds, *, n_series: int | None = None,
                   metric: str = "rmse", stream: torch.cuda.Stream | None = None, expanded: dict | None = None) -> dict:
    """The walk-forward backtest of a resident block, no host copy: anofox_hip_backtest_expand_device -> DeviceBatch(n_pairs, t_train,
    opts).set_block -> run -> anofox_hip_backtest_collect_device.

    y [t_rows, ld] fp64 time-major without NULLs, lengths int32 [>= n_series], on one HIP device, contiguous; folds is the table of
    api.backtest_fold_bounds / lib.backtest_folds ([(fold_id, train_start, train_end, test_start, test_end)], positions inclusive, the
    same for every series).  Any ForecastOptions block is allowed.  Pair p = s * F + f is series s in fold index f, so every
    [n_pairs, h] result viewed as [n_series, F * h] is the series-major block of one group per series that conformal_block(...,
    series_major=True) and anofox_hip_metrics_device(stride_s = F * h, stride_t = 1) take as it lies.

    Returns {"yhat", "lower", "upper" (views of the batch's results), "actual", "error", "abs_error": fp64 [n_pairs, h], NaN in the
    last three where the row does not exist; "valid": uint8 [n_pairs, h]; "n_rows", "status", "model_code": int32 [n_pairs];
    "scores": fp64 [F], the fold metric (backtest_metrics.backtest_metric's bits); "len_pairs", "n_test": int32 [ld_pairs]; "train":
    the expanded block [t_train, ld_pairs]; "batch": the DeviceBatch (model names: batch.model_name(code, p)); "n_pairs",
    "n_folds", "t_train"}.  `expanded`: what backtest_expand_block returned for the same block and folds -- the expanded block is
    then shared (several methods on one block: select_block) instead of made again."""
    L = _lib.load()
    assert y.dtype == torch.float64 and y.is_cuda and y.is_contiguous() and y.dim() == 2
    t_rows, ld = int(y.shape[0]), int(y.shape[1])
    n = ld if n_series is None else int(n_series)
    assert lengths.dtype == torch.int32 and lengths.is_cuda and lengths.is_contiguous() and lengths.numel() >= n
    dev = y.device
    if L.anofox_hip_set_device(dev.index or 0) != 0:
        raise RuntimeError(f"hipSetDevice({dev.index or 0}) failed")
    F = len(folds)
    tab = _lib.make_folds(folds)
    h = int(opts.horizon)
    st = stream if stream is not None else torch.cuda.current_stream(dev)
    err = _lib.AnofoxError()
    if expanded is None:
        expanded = backtest_expand_block(y, lengths, folds, n_series=n, stream=st)
    train, len_pairs, n_test = expanded["train"], expanded["len_pairs"], expanded["n_test"]
    t_train, n_pairs = int(expanded["t_train"]), int(expanded["n_pairs"])
    assert int(expanded["n_folds"]) == F and n_pairs == n * F, "the expanded block belongs to another block or fold table"
    batch = DeviceBatch(n_pairs, t_train, opts, dev)
    batch.set_block(train, len_pairs)
    batch.run(st)
    res = batch.results()
    actual = torch.empty((n_pairs, h), dtype=torch.float64, device=dev)
    error = torch.empty_like(actual)
    abs_error = torch.empty_like(actual)
    valid = torch.empty((n_pairs, h), dtype=torch.uint8, device=dev)
    n_rows = torch.zeros(n_pairs, dtype=torch.int32, device=dev)
    scores = torch.full((F,), float("nan"), dtype=torch.float64, device=dev)
    ok = L.anofox_hip_backtest_collect_device(y.data_ptr(), ld, n, t_rows, tab, F, n_test.data_ptr(), res["status"].data_ptr(),
                                              res["yhat"].data_ptr(), res["lower"].data_ptr(), res["upper"].data_ptr(), h,
                                              str(metric).encode(), actual.data_ptr(), error.data_ptr(), abs_error.data_ptr(),
                                              valid.data_ptr(), n_rows.data_ptr(), scores.data_ptr(), C.c_void_p(st.cuda_stream),
                                              C.byref(err))
    if not ok:
        raise RuntimeError(f"anofox_hip_backtest_collect_device failed: [{err.code}] {err.message.decode()}")
    return {"yhat": res["yhat"], "lower": res["lower"], "upper": res["upper"], "actual": actual, "error": error, "abs_error": abs_error,
            "valid": valid, "n_rows": n_rows, "status": res["status"], "model_code": res["model_code"], "scores": scores,
            "len_pairs": len_pairs, "n_test": n_test, "train": train, "batch": batch, "n_pairs": n_pairs, "n_folds": F,
            "t_train": t_train}


def hierarchy_plan_device(column_of: torch.Tensor) -> dict:
    """The CSR plan of anofox_hip_hierarchy_plan made on the device with torch: column_of int32 / int64 [n_groupings, n_series]
    (-1: none) -> {"col_offsets": int32 [n_out + 1], "members": int32 [nnz], "n_out", "nnz"}.  The entries are laid out by (series,
    grouping) and sorted by column with a STABLE sort, so that is their order within a column.  One device-to-host read (n_out)."""
    assert column_of.is_cuda and column_of.dim() == 2
    G, n = int(column_of.shape[0]), int(column_of.shape[1])
    dev = column_of.device
    flat = column_of.t().contiguous().reshape(-1).to(torch.int64)                     # entry e = s * G + g
    assert G * n == 0 or int(flat.min().item()) >= -1, "a column_of entry is below -1"
    keep = flat >= 0
    cols = flat[keep]
    series = torch.div(torch.arange(G * n, device=dev), max(G, 1), rounding_mode="floor")[keep]
    nnz = int(cols.numel())
    n_out = int(cols.max().item()) + 1 if nnz else 0
    assert n_out <= 2**31 - 1 and nnz <= 2**31 - 1, "n_out and nnz are limited to 2^31 - 1"
    order = torch.sort(cols, stable=True).indices
    offsets = torch.zeros(n_out + 1, dtype=torch.int64, device=dev)
    if nnz:
        offsets[1:] = torch.cumsum(torch.bincount(cols, minlength=n_out), 0)
    return {"col_offsets": offsets.to(torch.int32), "members": series[order].to(torch.int32).contiguous(), "n_out": n_out, "nnz": nnz}


def aggregate_block(y: torch.Tensor, lengths: torch.Tensor, column_of, *, first: torch.Tensor | None = None,
                    valid: torch.Tensor | None = None, present: torch.Tensor | None = None, n_series: int | None = None,
                    t_out: int | None = None, route: str | int = "auto", tile_min_members: int = 0, out: dict | None = None,
                    stream: torch.cuda.Stream | None = None) -> dict:
    """anofox_hip_hierarchy_device on torch tensors: ts_aggregate_hierarchy's sums of a resident block, no host round trip.

    y [t_rows, ld] fp64 time-major, left-aligned with lengths int32 [>= n_series]; first int64 [>= n_series]: the position of each
    series' row 0 on a common date grid (None: all 0); valid / present [t_rows, ld] uint8 or bool (valid 0 = NULL: counts as 0.0, the
    row exists; present 0 = no row there) -- all on one HIP device, contiguous.  column_of: an int tensor [n_groupings, n_series] with
    the output column of every series under every grouping (-1: none; the plan is then made on the device, hierarchy_plan_device), or
    a ready-made plan {"col_offsets", "members", "n_out"} of device tensors.  Output column c is the sum of its members in ascending
    series order, every cell one serial chain from +0.0: the bits of the operator on a table that arrives in series order per date.
    route "auto" / "lane" / "tile" (lib.HIERARCHY_ROUTES) gives the same bits.

    Without t_out a sizing call runs first (one device-to-host read of the lengths); it raises when a column is marked -1 (a member
    outside the block, a span above 2^30 rows).  `out` may bring "y", "present" ([t_out, ld_out]), "lengths" (int32 [ld_out]) and
    "first" (int64 [ld_out]); else they are allocated zero-filled with ld_out = n_out rounded up to 64.

    Returns {"y", "present", "lengths", "first", "t_out", "n_out"}.  DeviceBatch(n_out, t_out, opts).set_block(r["y"], r["lengths"])
    takes the result as it is when no column has a hole (r["present"] is 1 in every row below the column's length)."""
    L = _lib.load()
    assert y.dtype == torch.float64 and y.is_cuda and y.is_contiguous() and y.dim() == 2
    t_rows, ld = int(y.shape[0]), int(y.shape[1])
    n = ld if n_series is None else int(n_series)
    dev = y.device
    assert lengths.dtype == torch.int32 and lengths.is_cuda and lengths.is_contiguous() and lengths.numel() >= n
    if first is not None:
        assert first.dtype == torch.int64 and first.is_cuda and first.is_contiguous() and first.numel() >= n
    masks = []
    for m in (valid, present):
        if m is not None:
            if m.dtype == torch.bool:
                m = m.to(torch.uint8)
            assert m.dtype == torch.uint8 and m.is_cuda and m.is_contiguous() and tuple(m.shape) == (t_rows, ld)
        masks.append(m)
    valid, present = masks
    if L.anofox_hip_set_device(dev.index or 0) != 0:
        raise RuntimeError(f"hipSetDevice({dev.index or 0}) failed")
    if isinstance(column_of, dict):
        plan = column_of
    else:
        assert int(column_of.shape[-1]) == n, "column_of has one entry per series and grouping"
        plan = hierarchy_plan_device(column_of.reshape(-1, n))
    offsets, members, n_out = plan["col_offsets"], plan["members"], int(plan["n_out"])
    nnz = int(plan.get("nnz", members.numel()))
    assert offsets.dtype == torch.int32 and offsets.is_cuda and offsets.is_contiguous() and offsets.numel() >= n_out + 1
    assert members.dtype == torch.int32 and members.is_cuda and members.is_contiguous() and members.numel() >= nnz
    opts = _lib.make_hierarchy_options(route, tile_min_members)
    out = dict(out or {})
    yo, po, len_out, first_out = out.get("y"), out.get("present"), out.get("lengths"), out.get("first")
    ld_out = int(yo.shape[1]) if yo is not None else max((n_out + 63) // 64 * 64, 64)
    if len_out is None:
        len_out = torch.zeros(ld_out, dtype=torch.int32, device=dev)
    if first_out is None:
        first_out = torch.zeros(ld_out, dtype=torch.int64, device=dev)
    assert len_out.dtype == torch.int32 and len_out.is_cuda and len_out.numel() >= n_out
    assert first_out.dtype == torch.int64 and first_out.is_cuda and first_out.numel() >= n_out
    st = stream if stream is not None else torch.cuda.current_stream(dev)
    ptr = lambda t: t.data_ptr() if t is not None else None

    def call(rows, y_o, p_o):
        err = _lib.AnofoxError()
        ok = L.anofox_hip_hierarchy_device(y.data_ptr(), ptr(valid), ptr(present), ld, lengths.data_ptr(), ptr(first), n, t_rows,
                                           offsets.data_ptr(), members.data_ptr(), n_out, nnz, C.byref(opts), C.sizeof(opts), rows,
                                           ptr(y_o), ptr(p_o), ld_out, len_out.data_ptr(), first_out.data_ptr(),
                                           C.c_void_p(st.cuda_stream), C.byref(err))
        if not ok:
            raise RuntimeError(f"anofox_hip_hierarchy_device failed: [{err.code}] {err.message.decode()}")

    if t_out is None and yo is not None:
        t_out = int(yo.shape[0])
    if t_out is None:
        call(0, None, None)
        st.synchronize()
        sized = len_out[:n_out]
        if n_out and int(sized.min().item()) < 0:
            raise ValueError("aggregate_block: a column has a member outside the block, a first position above 2^61 or a span above "
                             "the limit of 2^30 rows (lengths -1)")
        t_out = max(1, int(sized.max().item())) if n_out else 1
    t_out = int(t_out)
    if yo is None:
        yo = torch.zeros((t_out, ld_out), dtype=torch.float64, device=dev)
    if po is None:
        po = torch.zeros((t_out, ld_out), dtype=torch.uint8, device=dev)
    for t, dt in ((yo, torch.float64), (po, torch.uint8)):
        assert t.dtype == dt and t.is_cuda and t.is_contiguous() and tuple(t.shape) == (t_out, ld_out) and ld_out >= n_out
    call(t_out, yo, po)
    return {"y": yo, "present": po, "lengths": len_out, "first": first_out, "t_out": t_out, "n_out": n_out}


def _paths_failed(entry: str, err) -> Exception:
    text = f"{entry} failed: [{err.code}] {err.message.decode()}"
    return ValueError(text) if err.code in (_lib.INVALID_INPUT, _lib.NULL_POINTER) else RuntimeError(text)


def _paths_rows(n_paths: int, horizon: int) -> None:
    # (the library checks the same before it touches the device; here the check comes before the output block is allocated)
    if not 1 <= n_paths <= _lib.PATHS_MAX_PATHS:
        raise ValueError(f"n_paths {n_paths} is outside [1, {_lib.PATHS_MAX_PATHS}], the limit of paths per call")
    if horizon < 1:
        raise ValueError("horizon must be at least 1")


def paths_block(point: torch.Tensor, pool: torch.Tensor, *, pool_lengths: torch.Tensor | None = None, n_paths: int = 1000,
                mode: str | int = "cumulative", joint: bool = False, seed: int = 0, series_major: bool = False,
                pool_series_major: bool = False, n_series: int | None = None, route: str | int = "auto",
                out: torch.Tensor | None = None, stream: torch.cuda.Stream | None = None) -> dict:
    """anofox_hip_paths_device on torch tensors: residual-bootstrap sample paths around a block of point forecasts, no host copy.

    point: time-major [h, ld], or with series_major=True the [n_series, h] layout of DeviceBatch.results()["yhat"].  pool: the
    residuals the paths draw from, time-major [pool_rows, ld], or with pool_series_major=True [n_series, pool_rows] -- the "error"
    block of backtest_block viewed as [n_series, n_folds * h] is taken as it lies.  pool_lengths int32 [>= n_series] on the device:
    the rows of every pool (None: all pool_rows).  mode "cumulative" (the errors add up along a path, so the band grows with the
    horizon) or "independent"; joint=True draws ONE pool row per (path, step) for all series -- the same date, which keeps the
    dependence between the series in their sums -- and needs every pool to have pool_rows rows.  The draws are Philox4x32-10 on the
    counter (path, series, step): the same seed gives the same bits whatever the launch shape.

    Returns {"paths": fp64 [n_paths * h, ld_out] time-major, row p * h + k of column s (`out`, or a new zero-filled block with
    ld_out = n_series rounded up to 64), "status": int32 [n_series] (lib.PATHS_OK / _EMPTY / _NAN / _RAGGED; the paths of a series
    whose status is not 0 are NaN), "n_series", "horizon", "n_paths"}.  The block is what aggregate_block takes with lengths
    n_paths * h; path_quantiles_block reads the quantiles off it or off its aggregate."""
    L = _lib.load()
    for t in (point, pool):
        assert t.dtype == torch.float64 and t.is_cuda and t.is_contiguous() and t.dim() == 2
    if series_major:
        n_f, h = int(point.shape[0]), int(point.shape[1])
        fs, ft = h, 1
    else:
        h, n_f = int(point.shape[0]), int(point.shape[1])
        fs, ft = 1, n_f
    if pool_series_major:
        n_p, pool_rows = int(pool.shape[0]), int(pool.shape[1])
        es, et = pool_rows, 1
    else:
        pool_rows, n_p = int(pool.shape[0]), int(pool.shape[1])
        es, et = 1, n_p
    n = min(n_f, n_p) if n_series is None else int(n_series)
    assert 0 < n <= n_f and n <= n_p
    n_paths = int(n_paths)
    _paths_rows(n_paths, h)
    dev = point.device
    if pool_lengths is not None:
        assert pool_lengths.dtype == torch.int32 and pool_lengths.is_cuda and pool_lengths.is_contiguous() and pool_lengths.numel() >= n
    opts = _lib.make_paths_options(mode, joint, seed, route)
    if L.anofox_hip_set_device(dev.index or 0) != 0:
        raise RuntimeError(f"hipSetDevice({dev.index or 0}) failed")
    if out is None:
        ld_out = (n + 63) // 64 * 64
        try:
            out = torch.zeros((n_paths * h, ld_out), dtype=torch.float64, device=dev)
        except torch.cuda.OutOfMemoryError as e:
            raise RuntimeError(f"the path block of {n_paths * h} x {ld_out} values needs {n_paths * h * ld_out * 8} bytes of device "
                               "memory") from e
    assert out.dtype == torch.float64 and out.is_cuda and out.is_contiguous() and out.dim() == 2 and int(out.shape[0]) == n_paths * h
    ld_out = int(out.shape[1])
    status = torch.zeros(n, dtype=torch.int32, device=dev)
    st = stream if stream is not None else torch.cuda.current_stream(dev)
    err = _lib.AnofoxError()
    ok = L.anofox_hip_paths_device(point.data_ptr(), fs, ft, pool.data_ptr(), es, et, pool_lengths.data_ptr() if pool_lengths is not None else None,
                                   pool_rows, n, h, n_paths, C.byref(opts), C.sizeof(opts), out.data_ptr(), ld_out, status.data_ptr(),
                                   C.c_void_p(st.cuda_stream), C.byref(err))
    if not ok:
        raise _paths_failed("anofox_hip_paths_device", err)
    return {"paths": out, "status": status, "n_series": n, "horizon": h, "n_paths": n_paths}


def path_quantiles_block(paths: torch.Tensor, levels, *, horizon: int, n_paths: int, n_cols: int | None = None,
                         stream: torch.cuda.Stream | None = None) -> dict:
    """anofox_hip_path_quantiles_device on torch tensors: the quantiles of a block of sample paths, no host copy.

    paths [n_paths * horizon, ld] fp64 time-major as paths_block or aggregate_block wrote it; levels: up to 16 values in [0, 1].
    The n_paths values of a (column, step) are sorted by the total order of the bits (-0.0 below +0.0) and level q is
    s[lo] * (1 - frac) + s[up] * frac at index q * (n_paths - 1).

    Returns {"quantiles": fp64 [n_levels, n_cols, horizon] -- the shape of conformal_block's "lower" / "upper" for a series-major
    forecast --, "status": int32 [n_cols]: 0, or lib.PATHS_NAN when a path of the column holds a NaN; every quantile of it is NaN}.

    The chain for the band of an aggregate -- the quantile of a sum is not the sum of the quantiles, so the paths are added up, not
    the bands:
        g = paths_block(yhat, errors, n_paths=1000, joint=True, series_major=True, pool_series_major=True)
        rows = torch.full((g["n_series"],), 1000 * h, dtype=torch.int32, device=yhat.device)
        a = aggregate_block(g["paths"], rows, column_of, n_series=g["n_series"], t_out=1000 * h)
        q = path_quantiles_block(a["y"], [0.05, 0.5, 0.95], horizon=h, n_paths=1000, n_cols=a["n_out"])"""
    L = _lib.load()
    assert paths.dtype == torch.float64 and paths.is_cuda and paths.is_contiguous() and paths.dim() == 2
    horizon, n_paths = int(horizon), int(n_paths)
    _paths_rows(n_paths, horizon)
    ld = int(paths.shape[1])
    n = ld if n_cols is None else int(n_cols)
    assert int(paths.shape[0]) >= n_paths * horizon and 0 < n <= ld
    al = np.ascontiguousarray(levels, dtype=np.float64).reshape(-1)
    k = len(al)
    dev = paths.device
    if L.anofox_hip_set_device(dev.index or 0) != 0:
        raise RuntimeError(f"hipSetDevice({dev.index or 0}) failed")
    q = torch.full((max(min(k, _lib.PATHS_MAX_LEVELS), 1), n, horizon), float("nan"), dtype=torch.float64, device=dev)
    status = torch.zeros(n, dtype=torch.int32, device=dev)
    st = stream if stream is not None else torch.cuda.current_stream(dev)
    err = _lib.AnofoxError()
    ok = L.anofox_hip_path_quantiles_device(paths.data_ptr(), ld, n, horizon, n_paths, al.ctypes.data, k, q.data_ptr(), status.data_ptr(),
                                            C.c_void_p(st.cuda_stream), C.byref(err))
    if not ok:
        raise _paths_failed("anofox_hip_path_quantiles_device", err)
    return {"quantiles": q, "status": status}


def ets_innovations_block(y: torch.Tensor, fitted: torch.Tensor, lengths: torch.Tensor, spec: torch.Tensor, *, n_series: int | None = None,
                          stream: torch.cuda.Stream | None = None) -> dict:
    """anofox_hip_ets_innovations_device on torch tensors: the in-sample innovations of a fitted block in the model's own terms.

    y and fitted fp64 [T, ld] time-major (the series block of a DeviceBatch and the "fitted" block of its inspect_device), lengths and
    spec int32 [>= n_series] on the device (spec: error * 15 + trend * 3 + season).  An additive error gives y - fitted, a
    multiplicative one (y - fitted) / fitted.

    Returns {"pool": fp64 [T, ld] time-major, NaN where nothing is written (past a series' length, the padding columns),
    "pool_lengths": int32 [n_series], 0 for a spec that is none of the project's}: what ets_paths_block takes as its pool."""
    L = _lib.load()
    for t in (y, fitted):
        assert t.dtype == torch.float64 and t.is_cuda and t.is_contiguous() and t.dim() == 2
    assert tuple(y.shape) == tuple(fitted.shape), (tuple(y.shape), tuple(fitted.shape))
    T, ld = int(y.shape[0]), int(y.shape[1])
    n = ld if n_series is None else int(n_series)
    for t in (lengths, spec):
        assert t.dtype == torch.int32 and t.is_cuda and t.is_contiguous() and t.numel() >= n
    dev = y.device
    if L.anofox_hip_set_device(dev.index or 0) != 0:
        raise RuntimeError(f"hipSetDevice({dev.index or 0}) failed")
    pool = torch.full((T, ld), float("nan"), dtype=torch.float64, device=dev)
    pool_lengths = torch.zeros(n, dtype=torch.int32, device=dev)
    st = stream if stream is not None else torch.cuda.current_stream(dev)
    err = _lib.AnofoxError()
    ok = L.anofox_hip_ets_innovations_device(y.data_ptr(), fitted.data_ptr(), ld, lengths.data_ptr(), spec.data_ptr(), n, T, pool.data_ptr(),
                                             pool_lengths.data_ptr(), C.c_void_p(st.cuda_stream), C.byref(err))
    if not ok:
        raise _paths_failed("anofox_hip_ets_innovations_device", err)
    return {"pool": pool, "pool_lengths": pool_lengths}


def ets_paths_block(batch=None, *, spec: torch.Tensor | None = None, info: torch.Tensor | None = None, states: torch.Tensor | None = None,
                    lengths: torch.Tensor | None = None, m: int | None = None, horizon: int | None = None, n_paths: int = 1000,
                    innovations: str | int = "gaussian", pool: torch.Tensor | None = None, pool_lengths: torch.Tensor | None = None,
                    pool_series_major: bool = False, joint: bool = False, seed: int = 0, n_series: int | None = None,
                    out: torch.Tensor | None = None, stream: torch.cuda.Stream | None = None) -> dict:
    """anofox_hip_ets_paths_device on torch tensors: sample paths simulated from fitted ETS models, no host copy.

    Either a DeviceBatch that has been run (AutoETS or ETS(spec), one seasonal period): its inspect_device gives spec, info, states,
    lengths, m and the horizon, and with innovations="bootstrap" and no `pool` the batch's own in-sample innovations
    (ets_innovations_block) are the pool.  Or the tensors themselves: spec int32 [>= n], info fp64 [8, ld] (rows alpha, beta, gamma,
    phi, -, -, -, sse), states fp64 [2 + max(m, 1), ld] (level, growth, seasonal state of phase j in row 2 + j), lengths int32 [>= n],
    m and horizon.  innovations "gaussian" (sigma = sqrt(sse / n) per series) or "bootstrap" (pool fp64 [pool_rows, ld] time-major,
    or [n, pool_rows] with pool_series_major=True; pool_lengths as for paths_block; joint=True: one pool row per path and step for
    all series).  The draws are Philox4x32-10 on the counter (path, series, step): the same seed gives the same bits whatever the
    launch shape.

    Returns {"paths": fp64 [n_paths * h, ld_out] in the layout of paths_block, "status": int32 [n] (lib.PATHS_* and
    lib.ETS_PATHS_NO_MODEL; the paths of a series whose status is not 0 are NaN), "n_broken": int32 [n], the paths of a series that
    hold a NaN (a damped multiplicative trend whose growth left the positive numbers), "n_series", "horizon", "n_paths"}.
    path_quantiles_block, path_scores_block and aggregate_block take the block as it lies."""
    L = _lib.load()
    if batch is not None:
        insp = batch.inspect_device(fitted=(innovations in ("bootstrap", 1) and pool is None))
        spec, info, states, lengths, m = insp["spec"], insp["info"], insp["states"], batch._len, insp["m"]
        horizon = batch.h if horizon is None else horizon
        n_series = batch.n if n_series is None else n_series
        if insp["fitted"] is not None:
            inn = ets_innovations_block(batch._y, insp["fitted"], lengths, spec, n_series=n_series, stream=stream)
            pool, pool_lengths, pool_series_major = inn["pool"], inn["pool_lengths"], False
    assert spec is not None and info is not None and states is not None and lengths is not None and m is not None and horizon is not None
    m, h, n_paths = int(m), int(horizon), int(n_paths)
    for t in (info, states):
        assert t.dtype == torch.float64 and t.is_cuda and t.is_contiguous() and t.dim() == 2
    ld = int(info.shape[1])
    assert int(info.shape[0]) >= 8 and int(states.shape[1]) == ld and int(states.shape[0]) >= 2 + max(m, 1)
    n = ld if n_series is None else int(n_series)
    assert 0 < n <= ld
    for t in (spec, lengths):
        assert t.dtype == torch.int32 and t.is_cuda and t.is_contiguous() and t.numel() >= n
    _paths_rows(n_paths, h)
    dev = info.device
    pool_rows, es, et = 0, 0, 0
    if pool is not None:
        assert pool.dtype == torch.float64 and pool.is_cuda and pool.is_contiguous() and pool.dim() == 2
        if pool_series_major:
            assert int(pool.shape[0]) >= n
            pool_rows, es, et = int(pool.shape[1]), int(pool.shape[1]), 1
        else:
            assert int(pool.shape[1]) >= n
            pool_rows, es, et = int(pool.shape[0]), 1, int(pool.shape[1])
    if pool_lengths is not None:
        assert pool_lengths.dtype == torch.int32 and pool_lengths.is_cuda and pool_lengths.is_contiguous() and pool_lengths.numel() >= n
    opts = _lib.make_ets_paths_options(innovations, joint, seed)
    if L.anofox_hip_set_device(dev.index or 0) != 0:
        raise RuntimeError(f"hipSetDevice({dev.index or 0}) failed")
    if out is None:
        ld_out = (n + 63) // 64 * 64
        try:
            out = torch.zeros((n_paths * h, ld_out), dtype=torch.float64, device=dev)
        except torch.cuda.OutOfMemoryError as e:
            raise RuntimeError(f"the path block of {n_paths * h} x {ld_out} values needs {n_paths * h * ld_out * 8} bytes of device "
                               "memory") from e
    assert out.dtype == torch.float64 and out.is_cuda and out.is_contiguous() and out.dim() == 2 and int(out.shape[0]) == n_paths * h
    ld_out = int(out.shape[1])
    status = torch.zeros(n, dtype=torch.int32, device=dev)
    n_broken = torch.zeros(n, dtype=torch.int32, device=dev)
    st = stream if stream is not None else torch.cuda.current_stream(dev)
    err = _lib.AnofoxError()
    ok = L.anofox_hip_ets_paths_device(spec.data_ptr(), info.data_ptr(), states.data_ptr(), ld, m, lengths.data_ptr(),
                                       pool.data_ptr() if pool is not None else None, es, et,
                                       pool_lengths.data_ptr() if pool_lengths is not None else None, pool_rows, n, h, n_paths,
                                       C.byref(opts), C.sizeof(opts), out.data_ptr(), ld_out, status.data_ptr(), n_broken.data_ptr(),
                                       C.c_void_p(st.cuda_stream), C.byref(err))
    if not ok:
        raise _paths_failed("anofox_hip_ets_paths_device", err)
    return {"paths": out, "status": status, "n_broken": n_broken, "n_series": n, "horizon": h, "n_paths": n_paths}


def arima_innovations_block(orders: torch.Tensor, coef: torch.Tensor, y: torch.Tensor, lengths: torch.Tensor, m: int, *,
                            n_series: int | None = None, out: dict | None = None, stream: torch.cuda.Stream | None = None) -> dict:
    """anofox_hip_arima_innovations_device on torch tensors: the in-sample innovations of fitted ARIMA models (the CSS recursion).

    orders int32 [8, ld] and coef fp64 [16, ld] as DeviceBatch.arima_fit_device gives them, y fp64 [T, ld] time-major (the series block
    of a DeviceBatch), lengths int32 [>= n_series] on the device, m the seasonal period.

    Returns {"resid": fp64 [T, ld] compacted (row j of a column is the residual of differenced index p + m P + j; NaN where nothing
    is written), "resid_lengths": int32 [n_series] (nu = n_diff - p - m P; 0 where the series has no model), "sigma": fp64 [n_series]
    (sqrt(css / nu); NaN where the series has no model)}: what arima_paths_block takes.  `out`: such a dict from an earlier call of
    the same shape, written again in place (nothing is allocated or filled: rows past a series' nu keep what they held)."""
    L = _lib.load()
    for t in (coef, y):
        assert t.dtype == torch.float64 and t.is_cuda and t.is_contiguous() and t.dim() == 2
    assert orders.dtype == torch.int32 and orders.is_cuda and orders.is_contiguous() and orders.dim() == 2
    T, ld = int(y.shape[0]), int(y.shape[1])
    assert tuple(orders.shape) == (8, ld) and tuple(coef.shape) == (16, ld), (tuple(orders.shape), tuple(coef.shape), ld)
    n = ld if n_series is None else int(n_series)
    assert lengths.dtype == torch.int32 and lengths.is_cuda and lengths.is_contiguous() and lengths.numel() >= n
    dev = y.device
    if L.anofox_hip_set_device(dev.index or 0) != 0:
        raise RuntimeError(f"hipSetDevice({dev.index or 0}) failed")
    if out is not None:
        resid, resid_lengths, sigma = out["resid"], out["resid_lengths"], out["sigma"]
        assert resid.dtype == torch.float64 and resid.is_cuda and resid.is_contiguous() and tuple(resid.shape) == (T, ld)
        assert resid_lengths.dtype == torch.int32 and resid_lengths.is_cuda and resid_lengths.is_contiguous() and resid_lengths.numel() >= n
        assert sigma.dtype == torch.float64 and sigma.is_cuda and sigma.is_contiguous() and sigma.numel() >= n
    else:
        resid = torch.full((T, ld), float("nan"), dtype=torch.float64, device=dev)
        resid_lengths = torch.zeros(n, dtype=torch.int32, device=dev)
        sigma = torch.full((n,), float("nan"), dtype=torch.float64, device=dev)
    st = stream if stream is not None else torch.cuda.current_stream(dev)
    err = _lib.AnofoxError()
    ok = L.anofox_hip_arima_innovations_device(orders.data_ptr(), coef.data_ptr(), ld, y.data_ptr(), lengths.data_ptr(), int(m), n, T,
                                               resid.data_ptr(), resid_lengths.data_ptr(), sigma.data_ptr(), C.c_void_p(st.cuda_stream),
                                               C.byref(err))
    if not ok:
        raise _paths_failed("anofox_hip_arima_innovations_device", err)
    return {"resid": resid, "resid_lengths": resid_lengths, "sigma": sigma}


def arima_paths_block(batch=None, *, orders: torch.Tensor | None = None, coef: torch.Tensor | None = None, y: torch.Tensor | None = None,
                      lengths: torch.Tensor | None = None, resid: torch.Tensor | None = None, resid_lengths: torch.Tensor | None = None,
                      sigma: torch.Tensor | None = None, m: int | None = None, horizon: int | None = None, n_paths: int = 1000,
                      innovations: str | int = "gaussian", joint: bool = False, pool_rows: int | None = None, seed: int = 0,
                      n_series: int | None = None, out: torch.Tensor | None = None, stream: torch.cuda.Stream | None = None) -> dict:
    """anofox_hip_arima_paths_device on torch tensors: sample paths simulated from fitted ARIMA models, no host copy.

    Either a DeviceBatch that has been run (AutoARIMA, one seasonal period): its arima_fit_device gives orders, coef and m, the batch
    its series, lengths and horizon, arima_innovations_block the residuals and sigma.  Or the tensors themselves (see
    arima_innovations_block).  innovations "gaussian" (e = sigma z) or "bootstrap" (the series' own residuals; joint=True: draw
    j < pool_rows takes residual row nu - pool_rows + j of every series; pool_rows None: the smallest nu among the series that have
    a model).  The draws are Philox4x32-10 on the counter (path, series, step): the same seed gives the same bits whatever the
    launch shape.

    Returns {"paths": fp64 [n_paths * h, ld_out] in the layout of paths_block, "status": int32 [n] (lib.PATHS_* and
    lib.ARIMA_PATHS_NO_MODEL; the paths of a series whose status is not 0 are NaN), "n_broken": int32 [n], the paths of a series
    that hold a NaN, "n_series", "horizon", "n_paths", "pool_rows"}.  path_quantiles_block, path_scores_block and aggregate_block
    take the block as it lies."""
    L = _lib.load()
    if batch is not None:
        fit = batch.arima_fit_device()
        orders, coef, m, y, lengths = fit["orders"], fit["coef"], fit["m"], batch._y, batch._len
        horizon = batch.h if horizon is None else horizon
        n_series = batch.n if n_series is None else n_series
        inn = arima_innovations_block(orders, coef, y, lengths, m, n_series=n_series, stream=stream)
        resid, resid_lengths, sigma = inn["resid"], inn["resid_lengths"], inn["sigma"]
    assert orders is not None and coef is not None and y is not None and lengths is not None and m is not None and horizon is not None
    assert resid is not None and resid_lengths is not None and sigma is not None
    m, h, n_paths = int(m), int(horizon), int(n_paths)
    for t in (coef, y, resid):
        assert t.dtype == torch.float64 and t.is_cuda and t.is_contiguous() and t.dim() == 2
    assert orders.dtype == torch.int32 and orders.is_cuda and orders.is_contiguous()
    T, ld = int(y.shape[0]), int(y.shape[1])
    assert tuple(orders.shape) == (8, ld) and tuple(coef.shape) == (16, ld) and tuple(resid.shape) == (T, ld)
    n = ld if n_series is None else int(n_series)
    assert 0 < n <= ld
    for t in (lengths, resid_lengths):
        assert t.dtype == torch.int32 and t.is_cuda and t.is_contiguous() and t.numel() >= n
    assert sigma.dtype == torch.float64 and sigma.is_cuda and sigma.is_contiguous() and sigma.numel() >= n
    _paths_rows(n_paths, h)
    dev = y.device
    opts = _lib.make_arima_paths_options(innovations, joint, seed)
    if opts.joint and pool_rows is None:
        nu = resid_lengths[:n]
        fitted = nu[nu > 0]
        pool_rows = int(fitted.min().item()) if fitted.numel() else 0
    pool_rows = int(pool_rows) if (opts.joint and pool_rows is not None) else 0
    if L.anofox_hip_set_device(dev.index or 0) != 0:
        raise RuntimeError(f"hipSetDevice({dev.index or 0}) failed")
    if out is None:
        ld_out = (n + 63) // 64 * 64
        try:
            out = torch.zeros((n_paths * h, ld_out), dtype=torch.float64, device=dev)
        except torch.cuda.OutOfMemoryError as e:
            raise RuntimeError(f"the path block of {n_paths * h} x {ld_out} values needs {n_paths * h * ld_out * 8} bytes of device "
                               "memory") from e
    assert out.dtype == torch.float64 and out.is_cuda and out.is_contiguous() and out.dim() == 2 and int(out.shape[0]) == n_paths * h
    ld_out = int(out.shape[1])
    status = torch.zeros(n, dtype=torch.int32, device=dev)
    n_broken = torch.zeros(n, dtype=torch.int32, device=dev)
    st = stream if stream is not None else torch.cuda.current_stream(dev)
    err = _lib.AnofoxError()
    ok = L.anofox_hip_arima_paths_device(orders.data_ptr(), coef.data_ptr(), ld, y.data_ptr(), lengths.data_ptr(), T, resid.data_ptr(),
                                         resid_lengths.data_ptr(), sigma.data_ptr(), m, pool_rows, n, h, n_paths, C.byref(opts),
                                         C.sizeof(opts), out.data_ptr(), ld_out, status.data_ptr(), n_broken.data_ptr(),
                                         C.c_void_p(st.cuda_stream), C.byref(err))
    if not ok:
        raise _paths_failed("anofox_hip_arima_paths_device", err)
    return {"paths": out, "status": status, "n_broken": n_broken, "n_series": n, "horizon": h, "n_paths": n_paths, "pool_rows": pool_rows}


PATH_SCORES_WANT = ("crps", "ranks", "quantiles", "column")


def _path_scores_actual(actual: torch.Tensor, horizon: int, n: int, series_major: bool):
    """-> (stride_c, stride_k) of the actual block: time-major [>= h, ld_a >= n], or series-major [>= n, h]."""
    assert actual.dtype == torch.float64 and actual.is_cuda and actual.is_contiguous() and actual.dim() == 2
    if series_major:
        assert int(actual.shape[0]) >= n and int(actual.shape[1]) == horizon
        return horizon, 1
    assert int(actual.shape[0]) >= horizon and int(actual.shape[1]) >= n
    return 1, int(actual.shape[1])


def path_scores_block(paths: torch.Tensor, actual: torch.Tensor, levels=(), *, horizon: int, n_paths: int, n_cols: int | None = None,
                      actual_series_major: bool = False, want=PATH_SCORES_WANT, stream: torch.cuda.Stream | None = None) -> dict:
    """anofox_hip_path_scores_device on torch tensors: the CRPS, the ranks and the pinball losses of a block of sample paths against
    the actuals, no host copy.

    paths [n_paths * horizon, ld] fp64 time-major as paths_block or aggregate_block wrote it.  actual: time-major [horizon, >= n_cols]
    (the "y" of aggregate_block on the actuals), or with actual_series_major=True [>= n_cols, horizon] -- a backtest's "actual" block
    as it lies; a NaN there drops the step.  levels: none or up to 16 values in [0, 1].  One sort per (column, step) serves every
    output; `want` names the outputs to compute: "crps" (per step), "ranks", "quantiles", "column".

    Returns {"crps": fp64 [n_cols, horizon]; "below", "equal": int32 [n_cols, horizon], the paths below the actual and equal to it
    (-1 where there is no actual); "quantiles": fp64 [n_levels, n_cols, horizon], the bits of path_quantiles_block; "crps_mean",
    "n_steps": fp64 [n_cols]; "pinball": fp64 [n_levels, n_cols] (views of "column" fp64 [2 + n_levels, ld_out]); "status": int32
    [n_cols]: lib.PATH_SCORES_OK, _NO_ACTUAL (every mean NaN) or _NAN (a NaN among the column's paths: every figure NaN)}; an output
    that was not wanted is None."""
    L = _lib.load()
    assert paths.dtype == torch.float64 and paths.is_cuda and paths.is_contiguous() and paths.dim() == 2
    horizon, n_paths = int(horizon), int(n_paths)
    _paths_rows(n_paths, horizon)
    ld = int(paths.shape[1])
    n = ld if n_cols is None else int(n_cols)
    assert int(paths.shape[0]) >= n_paths * horizon and 0 < n <= ld
    unknown = [w for w in want if w not in PATH_SCORES_WANT]
    if unknown:
        raise ValueError(f"path_scores_block: unknown outputs {unknown}; the outputs are {list(PATH_SCORES_WANT)}")
    sc, sk = _path_scores_actual(actual, horizon, n, actual_series_major)
    al = np.ascontiguousarray(levels, dtype=np.float64).reshape(-1)
    k = len(al)
    kk = min(k, _lib.PATHS_MAX_LEVELS)
    dev = paths.device
    if L.anofox_hip_set_device(dev.index or 0) != 0:
        raise RuntimeError(f"hipSetDevice({dev.index or 0}) failed")
    ld_out = (n + 63) // 64 * 64
    nan = float("nan")
    crps = torch.full((n, horizon), nan, dtype=torch.float64, device=dev) if "crps" in want else None
    below = torch.full((n, horizon), -1, dtype=torch.int32, device=dev) if "ranks" in want else None
    equal = torch.full((n, horizon), -1, dtype=torch.int32, device=dev) if "ranks" in want else None
    q = torch.full((kk, n, horizon), nan, dtype=torch.float64, device=dev) if "quantiles" in want and kk else None
    column = torch.full((2 + kk, ld_out), nan, dtype=torch.float64, device=dev) if "column" in want else None
    status = torch.zeros(n, dtype=torch.int32, device=dev)
    ptr = lambda t: t.data_ptr() if t is not None else None
    st = stream if stream is not None else torch.cuda.current_stream(dev)
    err = _lib.AnofoxError()
    ok = L.anofox_hip_path_scores_device(paths.data_ptr(), ld, n, horizon, n_paths, actual.data_ptr(), sc, sk, al.ctypes.data if k else None, k,
                                         ptr(crps), ptr(below), ptr(equal), ptr(q), ptr(column), ld_out, status.data_ptr(),
                                         C.c_void_p(st.cuda_stream), C.byref(err))
    if not ok:
        raise _paths_failed("anofox_hip_path_scores_device", err)
    out = {"crps": crps, "below": below, "equal": equal, "quantiles": q, "column": column, "status": status,
           "crps_mean": None, "n_steps": None, "pinball": None}
    if column is not None:
        out.update({"crps_mean": column[0, :n], "n_steps": column[1, :n], "pinball": column[2:, :n]})
    return out


def path_energy_block(paths: torch.Tensor, actual: torch.Tensor, *, horizon: int, n_paths: int, col_begin: int = 0, col_end: int | None = None,
                      actual_series_major: bool = False, stream: torch.cuda.Stream | None = None) -> dict:
    """anofox_hip_path_energy_device on torch tensors: the energy score of the columns [col_begin, col_end) of a block of sample
    paths -- a level of a hierarchy, the leaves alone or the whole plan -- in the estimator that takes consecutive paths as the
    independent copy: es[k] = mean_p |x_p - y| - sum_p |x_p - x_{p+1}| / (2 (P - 1)), Euclidean norms over the columns of the range.
    paths and actual as for path_scores_block; a NaN in the range propagates into es[k].

    Returns {"es": fp64 [horizon]; "summary": fp64 [2], es_mean (over the non-NaN steps) and es_steps; "workspace": fp64
    [2, n_paths, horizon], the distances D1 and D2 the sums run over}."""
    L = _lib.load()
    assert paths.dtype == torch.float64 and paths.is_cuda and paths.is_contiguous() and paths.dim() == 2
    horizon, n_paths = int(horizon), int(n_paths)
    _paths_rows(n_paths, horizon)
    ld = int(paths.shape[1])
    cb, ce = int(col_begin), ld if col_end is None else int(col_end)
    assert int(paths.shape[0]) >= n_paths * horizon
    err = _lib.AnofoxError()
    sc, sk = 1, 1
    if 0 <= cb < ce <= ld:                                    # (any other range is refused by the library, with its text)
        sc, sk = _path_scores_actual(actual, horizon, ce, actual_series_major)
    dev = paths.device
    if L.anofox_hip_set_device(dev.index or 0) != 0:
        raise RuntimeError(f"hipSetDevice({dev.index or 0}) failed")
    words = C.c_size_t()
    if not L.anofox_hip_path_scores_sizes(horizon, n_paths, C.byref(words), C.byref(err)):
        raise _paths_failed("anofox_hip_path_scores_sizes", err)
    assert int(words.value) == 2 * n_paths * horizon
    work = torch.zeros((2, n_paths, horizon), dtype=torch.float64, device=dev)
    es = torch.full((horizon,), float("nan"), dtype=torch.float64, device=dev)
    summary = torch.full((2,), float("nan"), dtype=torch.float64, device=dev)
    st = stream if stream is not None else torch.cuda.current_stream(dev)
    ok = L.anofox_hip_path_energy_device(paths.data_ptr(), ld, cb, ce, horizon, n_paths, actual.data_ptr(), sc, sk, work.data_ptr(), es.data_ptr(),
                                         summary.data_ptr(), C.c_void_p(st.cuda_stream), C.byref(err))
    if not ok:
        raise _paths_failed("anofox_hip_path_energy_device", err)
    return {"es": es, "summary": summary, "workspace": work}


def scale_block(y: torch.Tensor, lengths: torch.Tensor, *, w_src: torch.Tensor | None = None, lag: int = 1, trim_leading_zeros: bool = True,
                tail_rows: int = 28, n_cols: int | None = None, stream: torch.cuda.Stream | None = None) -> dict:
    """anofox_hip_scale_device on torch tensors: the in-sample scale and the weight mass of every column of a resident block, no
    host copy.

    y [t_rows, ld] fp64 time-major, left-aligned with lengths int32 [>= n_cols] -- the "y" and "lengths" of aggregate_block as they
    lie.  Per column: t0 = its first non-zero row (0 without trim_leading_zeros), msd and mad = the mean squared and the mean absolute
    difference y[t] - y[t - lag] over the rows t0 + lag .. n - 1 (what RMSSE, and MASE and the scaled pinball loss, divide by), and
    tail = the sum of the last tail_rows rows of w_src (a block laid out as y; None: y itself -- for M5 the aggregated units x price).

    Returns {"scale": fp64 [4, ld_out] in the rows lib.SCALE_ROWS; "msd", "mad", "n_terms", "tail": fp64 [n_cols], its views;
    "first": int32 [n_cols], t0; "status": int32 [n_cols]: lib.SCALE_OK, _SHORT (no difference: the scales NaN), _NAN (a NaN in the
    column or its tail: every figure NaN), _CONSTANT (msd == 0: the scales 0.0)}."""
    L = _lib.load()
    assert y.dtype == torch.float64 and y.is_cuda and y.is_contiguous() and y.dim() == 2
    t_rows, ld = int(y.shape[0]), int(y.shape[1])
    n = ld if n_cols is None else int(n_cols)
    assert 0 < n <= ld
    assert lengths.dtype == torch.int32 and lengths.is_cuda and lengths.is_contiguous() and lengths.numel() >= n
    if w_src is not None:
        assert w_src.dtype == torch.float64 and w_src.is_cuda and w_src.is_contiguous() and tuple(w_src.shape) == tuple(y.shape)
    dev = y.device
    if L.anofox_hip_set_device(dev.index or 0) != 0:
        raise RuntimeError(f"hipSetDevice({dev.index or 0}) failed")
    ld_out = (n + 63) // 64 * 64
    scale = torch.full((4, ld_out), float("nan"), dtype=torch.float64, device=dev)
    first = torch.zeros(n, dtype=torch.int32, device=dev)
    status = torch.zeros(n, dtype=torch.int32, device=dev)
    st = stream if stream is not None else torch.cuda.current_stream(dev)
    err = _lib.AnofoxError()
    ok = L.anofox_hip_scale_device(y.data_ptr(), ld, lengths.data_ptr(), n, t_rows, w_src.data_ptr() if w_src is not None else None, int(lag),
                                   bool(trim_leading_zeros), int(tail_rows), scale.data_ptr(), ld_out, first.data_ptr(), status.data_ptr(),
                                   C.c_void_p(st.cuda_stream), C.byref(err))
    if not ok:
        raise _paths_failed("anofox_hip_scale_device", err)
    return {"scale": scale, "msd": scale[0, :n], "mad": scale[1, :n], "n_terms": scale[2, :n], "tail": scale[3, :n], "first": first,
            "status": status}


def weighted_scores_block(loss: torch.Tensor, scale: torch.Tensor, weight: torch.Tensor, ranges, *, transform: str | int,
                          col_status: torch.Tensor | None = None, n_cols: int | None = None, want_scaled: bool = True,
                          stream: torch.cuda.Stream | None = None) -> dict:
    """anofox_hip_weighted_scores_device on torch tensors: the scaled losses and their weighted mean over column ranges, no host copy.

    loss fp64 [n_loss, ld] (or [ld]: one row) -- rows of metrics figures or of path_scores_block's "column" as they lie (a view of
    whole rows is taken as it is); scale and weight fp64 [>= n_cols] -- one row of scale_block's "scale" each, usually "msd" or "mad"
    and "tail"; col_status int32 [>= n_cols] or None; ranges: an int array or tensor [n_ranges, 2] of [begin, end).  transform "ratio"
    (loss / scale: SPL, MASE) or "root" (its square root: RMSSE).  A column is left out when its status is not 0, its scale is not
    finite or not positive, its weight is NaN or negative, or its scaled loss is not finite.

    Returns {"scaled": fp64 [n_loss, ld] (NaN where left out or in no range; None without want_scaled); "score", "weight_sum": fp64
    [n_ranges, n_loss]; "left": int32 [n_ranges, n_loss] (-1: a range that is empty, reversed or beyond n_cols; its score is NaN);
    "total": fp64 [n_loss], the mean of the ranges' scores per loss row; "total_mean": fp64 [1], the mean of those (the WSPL of nine
    pinball rows, the WRMSSE of one mse row)}."""
    L = _lib.load()
    code = _lib.SCALED_TRANSFORMS.get(transform, transform) if isinstance(transform, str) else int(transform)
    if isinstance(code, str):
        raise ValueError(f"weighted_scores_block: unknown transform {transform!r}; the transforms are {list(_lib.SCALED_TRANSFORMS)}")
    if loss.dim() == 1:
        loss = loss.view(1, -1)
    assert loss.dtype == torch.float64 and loss.is_cuda and loss.is_contiguous() and loss.dim() == 2
    n_loss, ld = int(loss.shape[0]), int(loss.shape[1])
    n = ld if n_cols is None else int(n_cols)
    assert 0 < n <= ld
    for t in (scale, weight):
        assert t.dtype == torch.float64 and t.is_cuda and t.is_contiguous() and t.dim() == 1 and t.numel() >= n
    if col_status is not None:
        assert col_status.dtype == torch.int32 and col_status.is_cuda and col_status.is_contiguous() and col_status.numel() >= n
    dev = loss.device
    rg = torch.as_tensor(np.ascontiguousarray(ranges, dtype=np.int32) if not torch.is_tensor(ranges) else ranges).to(device=dev, dtype=torch.int32)
    rg = rg.reshape(-1, 2).contiguous()
    R = int(rg.shape[0])
    if L.anofox_hip_set_device(dev.index or 0) != 0:
        raise RuntimeError(f"hipSetDevice({dev.index or 0}) failed")
    nan = float("nan")
    rows = max(min(n_loss, _lib.SCALED_MAX_LOSS), 1)
    scaled = torch.full((rows, ld), nan, dtype=torch.float64, device=dev) if want_scaled and n_loss <= _lib.SCALED_MAX_LOSS else None
    score = torch.full((max(R, 1), rows), nan, dtype=torch.float64, device=dev)
    wsum = torch.full((max(R, 1), rows), nan, dtype=torch.float64, device=dev)
    left = torch.full((max(R, 1), rows), -1, dtype=torch.int32, device=dev)
    total = torch.full((rows + 1,), nan, dtype=torch.float64, device=dev)
    st = stream if stream is not None else torch.cuda.current_stream(dev)
    err = _lib.AnofoxError()
    ok = L.anofox_hip_weighted_scores_device(loss.data_ptr(), ld, n, n_loss, scale.data_ptr(), weight.data_ptr(),
                                             col_status.data_ptr() if col_status is not None else None, rg.data_ptr(), R, code,
                                             scaled.data_ptr() if scaled is not None else None, score.data_ptr(), wsum.data_ptr(), left.data_ptr(),
                                             total.data_ptr(), C.c_void_p(st.cuda_stream), C.byref(err))
    if not ok:
        raise _paths_failed("anofox_hip_weighted_scores_device", err)
    return {"scaled": scaled, "score": score, "weight_sum": wsum, "left": left, "total": total[:n_loss], "total_mean": total[n_loss:],
            "ranges": rg}


_RECONCILE_PLAN_KEYS = ("col_offsets", "members", "bottom_col", "agg_cols", "leaf_offsets", "leaf_aggs")


def reconcile_plan_device(column_of, n_series: int | None = None, device=None) -> dict:
    """The reconciliation plan on the device.  column_of: an int array or tensor [n_groupings, n_series] as for aggregate_block, or an
    aggregation plan {"col_offsets", "members"} (host arrays or tensors) together with n_series.  The planning itself is
    anofox_hip_hierarchy_plan / anofox_hip_reconcile_plan on the host (a plan is made once and kept); the six int32 arrays and
    "struct_weights" (fp64 [n_out]) are uploaded.  A plan the planner refuses raises ValueError with its message."""
    import numpy as np
    host = lambda a: a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    if isinstance(column_of, dict):
        assert n_series is not None, "an aggregation plan needs n_series"
        n_out = int(column_of.get("n_out", len(column_of["col_offsets"]) - 1))
        offs = host(column_of["col_offsets"])[:n_out + 1]
        memb = host(column_of["members"])[:int(offs[n_out]) if n_out else 0]
        if device is None and isinstance(column_of["col_offsets"], torch.Tensor) and column_of["col_offsets"].is_cuda:
            device = column_of["col_offsets"].device
    else:
        if device is None and isinstance(column_of, torch.Tensor) and column_of.is_cuda:
            device = column_of.device
        co = host(column_of)
        co = co.reshape(-1, co.shape[-1] if n_series is None else int(n_series))
        n_series = co.shape[1]
        _n_out, offs, memb = _lib.hierarchy_plan(co)
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    p = _lib.reconcile_plan(offs, memb, int(n_series))
    plan = {k: p[k] for k in ("n_out", "nnz", "n_series", "n_agg", "n_leaf")}
    for k in _RECONCILE_PLAN_KEYS:
        plan[k] = torch.from_numpy(np.ascontiguousarray(p[k], dtype=np.int32)).to(dev)
    plan["struct_weights"] = torch.from_numpy(np.ascontiguousarray(p["struct_weights"])).to(dev)
    return plan


def reconcile_block(forecast: torch.Tensor, column_of, method: str | int = "ols", weights: torch.Tensor | None = None,
                    series_major: bool = True, factor: torch.Tensor | None = None, out: torch.Tensor | None = None,
                    stream: torch.cuda.Stream | None = None, *, n_series: int | None = None) -> dict:
    """anofox_hip_reconcile_factor_device + anofox_hip_reconcile_apply_device on torch tensors: the forecasts of the columns of an
    aggregation plan made coherent where they lie (DESIGN.md section 3 "Reconciliation").

    forecast fp64, contiguous, on one HIP device: series_major [>= n_out, h] -- the `yhat` of DeviceBatch results as it lies -- or
    time-major [n_rows, ld >= n_out].  column_of: an int array / tensor [n_groupings, n_series], or a plan of reconcile_plan_device
    (the "plan" this function returns: make it once).  method in lib.RECONCILE_METHODS; weights fp64 [>= n_out] for "wls_var".
    factor: the "factor" an earlier call with the same plan, method and weights returned -- one factor serves every block.  out: a
    tensor of forecast's shape (not forecast itself); only columns < n_out are written.

    Returns {"y", "row_status" int32 [n_rows] (0 done, 2 a base forecast that is not finite: that row's columns are NaN), "factor"
    (None for "bottom_up" or a plan without aggregates), "plan"}.  The factor call waits for the device; the apply only enqueues."""
    L = _lib.load()
    code = _lib.reconcile_method(method)
    assert forecast.dtype == torch.float64 and forecast.is_cuda and forecast.is_contiguous() and forecast.dim() == 2
    dev = forecast.device
    if L.anofox_hip_set_device(dev.index or 0) != 0:
        raise RuntimeError(f"hipSetDevice({dev.index or 0}) failed")
    plan = column_of if isinstance(column_of, dict) and "bottom_col" in column_of else reconcile_plan_device(column_of, n_series, dev)
    n_out, n_agg = int(plan["n_out"]), int(plan["n_agg"])
    for k in _RECONCILE_PLAN_KEYS:
        assert plan[k].dtype == torch.int32 and plan[k].is_cuda and plan[k].is_contiguous(), k
    if series_major:
        n_rows, stride_s, stride_t = int(forecast.shape[1]), int(forecast.shape[1]), 1
        assert int(forecast.shape[0]) >= n_out, "a series-major block has one row per output column"
    else:
        n_rows, stride_s, stride_t = int(forecast.shape[0]), 1, int(forecast.shape[1])
        assert int(forecast.shape[1]) >= n_out, "a time-major block has one column per output column"
    if out is None:
        out = forecast.clone()                                  # (columns from n_out on and the padding keep the input's values)
    assert out.dtype == torch.float64 and out.is_cuda and out.is_contiguous() and tuple(out.shape) == tuple(forecast.shape)
    assert out.data_ptr() != forecast.data_ptr(), "the input may not alias the output"
    w = None
    if code == _lib.RECONCILE_METHODS["wls_struct"]:
        w = plan["struct_weights"]
    elif code == _lib.RECONCILE_METHODS["wls_var"]:
        assert weights is not None, "wls_var takes one weight per output column"
        w = weights
    if w is not None:
        assert w.dtype == torch.float64 and w.is_cuda and w.is_contiguous() and w.numel() >= n_out
    st = stream if stream is not None else torch.cuda.current_stream(dev)
    ptr = lambda t: t.data_ptr() if t is not None else None
    plan_args = (plan["col_offsets"].data_ptr(), plan["members"].data_ptr(), n_out, int(plan["nnz"]), int(plan["n_series"]),
                 plan["bottom_col"].data_ptr(), plan["agg_cols"].data_ptr(), n_agg, plan["leaf_offsets"].data_ptr(),
                 plan["leaf_aggs"].data_ptr(), int(plan["n_leaf"]))
    solve = code != 0 and n_agg > 0
    err = _lib.AnofoxError()
    ld_a = 0
    if solve:
        if factor is None:
            factor = torch.zeros((n_agg, n_agg), dtype=torch.float64, device=dev)
            st.wait_stream(torch.cuda.current_stream(dev))
            if not L.anofox_hip_reconcile_factor_device(*plan_args, code, ptr(w), factor.data_ptr(), n_agg, C.c_void_p(st.cuda_stream), C.byref(err)):
                exc = ValueError if err.code == 2 else RuntimeError
                raise exc(f"anofox_hip_reconcile_factor_device failed: [{err.code}] {err.message.decode()}")
        assert factor.dtype == torch.float64 and factor.is_cuda and factor.is_contiguous() and factor.dim() == 2
        assert int(factor.shape[0]) >= n_agg and int(factor.shape[1]) >= n_agg
        ld_a = int(factor.shape[1])
    else:
        factor = None
    work = torch.empty((n_rows, n_agg), dtype=torch.float64, device=dev) if solve else None
    row_status = torch.zeros(max(n_rows, 1), dtype=torch.int32, device=dev)
    ok = L.anofox_hip_reconcile_apply_device(forecast.data_ptr(), stride_s, stride_t, n_rows, *plan_args, code, ptr(w), ptr(factor), ld_a,
                                             ptr(work), out.data_ptr(), row_status.data_ptr(), C.c_void_p(st.cuda_stream), C.byref(err))
    if not ok:
        raise RuntimeError(f"anofox_hip_reconcile_apply_device failed: [{err.code}] {err.message.decode()}")
    if work is not None:
        work.record_stream(st)
    return {"y": out, "row_status": row_status[:n_rows], "factor": factor, "plan": plan}


def reconcile_mint_block(forecast: torch.Tensor, residuals: torch.Tensor, column_of, shrinkage: float | None = None,
                         series_major: bool = True, residuals_series_major: bool = True, factor: dict | None = None,
                         out: torch.Tensor | None = None, stream: torch.cuda.Stream | None = None, *, n_series: int | None = None) -> dict:
    """anofox_hip_reconcile_mint_factor_device + anofox_hip_reconcile_mint_apply_device on torch tensors: MinT with the shrinkage
    covariance (DESIGN.md section 3 "MinT-shrink"), the forecasts made coherent where they lie.

    forecast as for reconcile_block.  residuals fp64, contiguous, on the same device: residuals_series_major [>= n_out, n_res] -- the
    `error` block of backtest_block over the aggregated block as it lies -- or time-major [n_res, ld >= n_out].  column_of: an int
    array / tensor or a plan of reconcile_plan_device.  shrinkage: None estimates the intensity (Schaefer and Strimmer), a value in
    [0, 1] is taken as it is.  factor: the "factor" bundle an earlier call with the same plan and residuals returned; it holds the
    intensity, so `shrinkage` is not read then.  out: a tensor of forecast's shape (not forecast itself).

    Returns {"y", "row_status", "shrinkage" (float), "variances" fp64 [n_out], "factor" (the bundle: variances, e, factor, shrinkage),
    "plan"}.  The factor call waits for the device; the apply only enqueues.  A size or an intensity the entries refuse raises
    ValueError, a residual that is not finite or a column without variance RuntimeError, each with the entry's message."""
    L = _lib.load()
    assert forecast.dtype == torch.float64 and forecast.is_cuda and forecast.is_contiguous() and forecast.dim() == 2
    assert residuals.dtype == torch.float64 and residuals.is_cuda and residuals.is_contiguous() and residuals.dim() == 2
    dev = forecast.device
    assert residuals.device == dev
    if L.anofox_hip_set_device(dev.index or 0) != 0:
        raise RuntimeError(f"hipSetDevice({dev.index or 0}) failed")
    plan = column_of if isinstance(column_of, dict) and "bottom_col" in column_of else reconcile_plan_device(column_of, n_series, dev)
    n_out, n_agg = int(plan["n_out"]), int(plan["n_agg"])
    for k in _RECONCILE_PLAN_KEYS:
        assert plan[k].dtype == torch.int32 and plan[k].is_cuda and plan[k].is_contiguous(), k
    if series_major:
        n_rows, stride_s, stride_t = int(forecast.shape[1]), int(forecast.shape[1]), 1
        assert int(forecast.shape[0]) >= n_out, "a series-major block has one row per output column"
    else:
        n_rows, stride_s, stride_t = int(forecast.shape[0]), 1, int(forecast.shape[1])
        assert int(forecast.shape[1]) >= n_out, "a time-major block has one column per output column"
    if residuals_series_major:
        n_res, res_s, res_t = int(residuals.shape[1]), int(residuals.shape[1]), 1
        assert int(residuals.shape[0]) >= n_out, "a series-major residual block has one row per output column"
    else:
        n_res, res_s, res_t = int(residuals.shape[0]), 1, int(residuals.shape[1])
        assert int(residuals.shape[1]) >= n_out, "a time-major residual block has one column per output column"
    if out is None:
        out = forecast.clone()
    assert out.dtype == torch.float64 and out.is_cuda and out.is_contiguous() and tuple(out.shape) == tuple(forecast.shape)
    assert out.data_ptr() != forecast.data_ptr(), "the input may not alias the output"
    st = stream if stream is not None else torch.cuda.current_stream(dev)
    plan_args = (plan["col_offsets"].data_ptr(), plan["members"].data_ptr(), n_out, int(plan["nnz"]), int(plan["n_series"]),
                 plan["bottom_col"].data_ptr(), plan["agg_cols"].data_ptr(), n_agg, plan["leaf_offsets"].data_ptr(),
                 plan["leaf_aggs"].data_ptr(), int(plan["n_leaf"]))
    res_args = (residuals.data_ptr(), res_s, res_t, n_res)
    err = _lib.AnofoxError()
    sizes = _lib.reconcile_mint_sizes(n_res, n_agg, n_rows)
    if factor is None:
        estimate = shrinkage is None
        variances = torch.zeros(max(n_out, 1), dtype=torch.float64, device=dev)
        e = torch.zeros((n_res, max(n_agg, 1)), dtype=torch.float64, device=dev)
        fac = torch.zeros((max(n_agg, 1), max(n_agg, 1)), dtype=torch.float64, device=dev)
        gram = torch.empty(sizes["gram"], dtype=torch.float64, device=dev) if estimate else None
        lam = C.c_double(float("nan"))
        st.wait_stream(torch.cuda.current_stream(dev))
        ok = L.anofox_hip_reconcile_mint_factor_device(*res_args, *plan_args, float("nan") if estimate else float(shrinkage), variances.data_ptr(),
                                                       e.data_ptr(), int(e.shape[1]), fac.data_ptr(), int(fac.shape[1]),
                                                       gram.data_ptr() if gram is not None else None, C.byref(lam), C.c_void_p(st.cuda_stream),
                                                       C.byref(err))
        if not ok:
            exc = ValueError if err.code == 2 else RuntimeError
            raise exc(f"anofox_hip_reconcile_mint_factor_device failed: [{err.code}] {err.message.decode()}")
        factor = {"variances": variances, "e": e, "factor": fac, "shrinkage": float(lam.value)}
    for k in ("variances", "e", "factor"):
        t = factor[k]
        assert t.dtype == torch.float64 and t.is_cuda and t.is_contiguous(), k
    assert factor["variances"].numel() >= n_out and int(factor["e"].shape[0]) >= n_res
    assert int(factor["e"].shape[1]) >= n_agg and int(factor["factor"].shape[0]) >= n_agg and int(factor["factor"].shape[1]) >= n_agg
    work = torch.empty(max(sizes["work"], 1), dtype=torch.float64, device=dev)
    row_status = torch.zeros(max(n_rows, 1), dtype=torch.int32, device=dev)
    ok = L.anofox_hip_reconcile_mint_apply_device(forecast.data_ptr(), stride_s, stride_t, n_rows, *res_args, *plan_args,
                                                  factor["variances"].data_ptr(), factor["e"].data_ptr(), int(factor["e"].shape[1]),
                                                  float(factor["shrinkage"]), factor["factor"].data_ptr(), int(factor["factor"].shape[1]),
                                                  work.data_ptr(), out.data_ptr(), row_status.data_ptr(), C.c_void_p(st.cuda_stream), C.byref(err))
    if not ok:
        exc = ValueError if err.code == 2 else RuntimeError
        raise exc(f"anofox_hip_reconcile_mint_apply_device failed: [{err.code}] {err.message.decode()}")
    work.record_stream(st)
    return {"y": out, "row_status": row_status[:n_rows], "shrinkage": float(factor["shrinkage"]), "variances": factor["variances"][:n_out],
            "factor": factor, "plan": plan}


def _check_methods(methods) -> int:
    """The method table of the selection entries: 1 .. lib.SELECT_MAX_METHODS option blocks that share one horizon >= 1."""
    M = len(methods)
    if M < 1:
        raise ValueError("Invalid input: n_methods is 0, a selection needs at least 1 method")
    if M > _lib.SELECT_MAX_METHODS:
        raise ValueError(f"Invalid input: n_methods {M} exceeds the limit of {_lib.SELECT_MAX_METHODS} methods")
    h = int(methods[0].horizon)
    if h < 1:
        raise ValueError(f"Invalid input: horizon must be at least 1, method 0 has {h}")
    for m, o in enumerate(methods):
        if int(o.horizon) != h:
            raise ValueError(f"Invalid input: all methods share one horizon, method {m} has {int(o.horizon)} and method 0 has {h}")
    return h


def combine_block(blocks, mode: str | int, *, status: torch.Tensor | None = None, winner: torch.Tensor | None = None,
                  weights: torch.Tensor | None = None, group_div: int = 1, stream: torch.cuda.Stream | None = None) -> dict:
    """anofox_hip_select_combine_device on torch tensors: M <= 16 blocks [R, h] (fp64, contiguous, one device) combined cell by cell.

    mode "pick" (needs winner int32 [groups]), "mean", "median", "inverse_score" (needs weights fp64 [M, ld_w >= groups]: the SCORES).
    status int32 [M, R] (None: all 0); a member is live in a cell when its status is 0 and its value there is not NaN.  Row r belongs to
    group r // group_div.  Returns {"y": fp64 [R, h] (NaN where no member is live), "row_status": int32 [R], 1 where the whole row is
    NaN}."""
    L = _lib.load()
    M = len(blocks)
    if M < 1 or M > _lib.SELECT_MAX_METHODS:
        raise ValueError(f"Invalid input: n_methods {M} is outside [1, {_lib.SELECT_MAX_METHODS}] (the limit of {_lib.SELECT_MAX_METHODS} methods)")
    code = _lib.select_mode(mode)
    b0 = blocks[0]
    for b in blocks:
        assert b.dtype == torch.float64 and b.is_cuda and b.is_contiguous() and b.dim() == 2 and tuple(b.shape) == tuple(b0.shape)
    R, h = int(b0.shape[0]), int(b0.shape[1])
    dev = b0.device
    if L.anofox_hip_set_device(dev.index or 0) != 0:
        raise RuntimeError(f"hipSetDevice({dev.index or 0}) failed")
    if status is None:
        status = torch.zeros((M, R), dtype=torch.int32, device=dev)
    assert status.dtype == torch.int32 and status.is_cuda and status.is_contiguous() and tuple(status.shape) == (M, R)
    groups = (R + int(group_div) - 1) // max(int(group_div), 1)
    ld_w = 0
    if winner is not None:
        assert winner.dtype == torch.int32 and winner.is_cuda and winner.is_contiguous() and winner.numel() >= groups
    if weights is not None:
        assert weights.dtype == torch.float64 and weights.is_cuda and weights.is_contiguous() and weights.dim() == 2 and int(weights.shape[0]) == M
        ld_w = int(weights.shape[1])
    out = torch.empty((R, h), dtype=torch.float64, device=dev)
    row_status = torch.zeros(max(R, 1), dtype=torch.int32, device=dev)
    tab = (C.c_void_p * M)(*[b.data_ptr() for b in blocks])
    st = stream if stream is not None else torch.cuda.current_stream(dev)
    ptr = lambda t: t.data_ptr() if t is not None else None
    err = _lib.AnofoxError()
    ok = L.anofox_hip_select_combine_device(tab, M, R, h, status.data_ptr(), code, ptr(winner), ptr(weights), ld_w, int(group_div),
                                            out.data_ptr(), row_status.data_ptr(), C.c_void_p(st.cuda_stream), C.byref(err))
    if not ok:
        exc = ValueError if err.code == _lib.INVALID_INPUT else RuntimeError
        raise exc(f"anofox_hip_select_combine_device failed: [{err.code}] {err.message.decode()}")
    return {"y": out, "row_status": row_status[:R]}


def select_winner_block(scores: torch.Tensor, score_status: torch.Tensor, fallback: int = -1, *, n_series: int | None = None,
                        stream: torch.cuda.Stream | None = None) -> dict:
    """anofox_hip_select_winner_device on torch tensors: scores fp64 [M, ld], score_status int32 [M, n_series] -> {"winner" int32 [n],
    "best_score" fp64 [n], "from_fallback" uint8 [n], "offsets" int32 [M + 1] and "members" int32 [n] (device tensors; only the first
    offsets[M] members are written)}.  Nothing is read back."""
    L = _lib.load()
    assert scores.dtype == torch.float64 and scores.is_cuda and scores.is_contiguous() and scores.dim() == 2
    M, ld = int(scores.shape[0]), int(scores.shape[1])
    n = ld if n_series is None else int(n_series)
    assert score_status.dtype == torch.int32 and score_status.is_cuda and score_status.is_contiguous() and tuple(score_status.shape) == (M, n)
    dev = scores.device
    if L.anofox_hip_set_device(dev.index or 0) != 0:
        raise RuntimeError(f"hipSetDevice({dev.index or 0}) failed")
    winner = torch.empty(n, dtype=torch.int32, device=dev)
    best = torch.empty(n, dtype=torch.float64, device=dev)
    ff = torch.empty(n, dtype=torch.uint8, device=dev)
    offsets = torch.zeros(M + 1, dtype=torch.int32, device=dev)
    members = torch.full((max(n, 1),), -1, dtype=torch.int32, device=dev)
    st = stream if stream is not None else torch.cuda.current_stream(dev)
    err = _lib.AnofoxError()
    ok = L.anofox_hip_select_winner_device(scores.data_ptr(), ld, score_status.data_ptr(), M, n, int(fallback), winner.data_ptr(),
                                           best.data_ptr(), ff.data_ptr(), offsets.data_ptr(), members.data_ptr(),
                                           C.c_void_p(st.cuda_stream), C.byref(err))
    if not ok:
        exc = ValueError if err.code == _lib.INVALID_INPUT else RuntimeError
        raise exc(f"anofox_hip_select_winner_device failed: [{err.code}] {err.message.decode()}")
    return {"winner": winner, "best_score": best, "from_fallback": ff, "offsets": offsets, "members": members[:n]}


def select_gather_block(y: torch.Tensor, lengths: torch.Tensor, members: torch.Tensor, off: int, n_m: int, *, n_series: int | None = None,
                        ld_m: int | None = None, out: dict | None = None, stream: torch.cuda.Stream | None = None) -> dict:
    """anofox_hip_select_gather_device on torch tensors: the columns members[off .. off + n_m) of a time-major block as a dense block
    {"y": fp64 [t_rows, ld_m], "lengths": int32 [ld_m]} (ld_m: n_m rounded up to 64), which DeviceBatch(n_m, t_rows, opts).set_block
    takes as it is.  `out` may bring the two tensors."""
    L = _lib.load()
    assert y.dtype == torch.float64 and y.is_cuda and y.is_contiguous() and y.dim() == 2
    t_rows, ld = int(y.shape[0]), int(y.shape[1])
    n = ld if n_series is None else int(n_series)
    assert lengths.dtype == torch.int32 and lengths.is_cuda and lengths.is_contiguous() and lengths.numel() >= n
    assert members.dtype == torch.int32 and members.is_cuda and members.is_contiguous() and members.numel() >= int(off) + int(n_m)
    dev = y.device
    if L.anofox_hip_set_device(dev.index or 0) != 0:
        raise RuntimeError(f"hipSetDevice({dev.index or 0}) failed")
    out = dict(out or {})
    ym, lm = out.get("y"), out.get("lengths")
    if ld_m is None:
        ld_m = int(ym.shape[1]) if ym is not None else max((int(n_m) + 63) // 64 * 64, 64)
    if ym is None:
        ym = torch.empty((t_rows, ld_m), dtype=torch.float64, device=dev)
    if lm is None:
        lm = torch.empty(ld_m, dtype=torch.int32, device=dev)
    assert ym.dtype == torch.float64 and ym.is_cuda and ym.is_contiguous() and tuple(ym.shape) == (t_rows, ld_m)
    assert lm.dtype == torch.int32 and lm.is_cuda and lm.is_contiguous() and lm.numel() >= ld_m
    st = stream if stream is not None else torch.cuda.current_stream(dev)
    err = _lib.AnofoxError()
    ok = L.anofox_hip_select_gather_device(y.data_ptr(), ld, lengths.data_ptr(), n, t_rows, members.data_ptr(), int(off), int(n_m),
                                           ym.data_ptr(), ld_m, lm.data_ptr(), C.c_void_p(st.cuda_stream), C.byref(err))
    if not ok:
        exc = ValueError if err.code == _lib.INVALID_INPUT else RuntimeError
        raise exc(f"anofox_hip_select_gather_device failed: [{err.code}] {err.message.decode()}")
    return {"y": ym, "lengths": lm}


def select_scatter_block(sub: dict | None, members: torch.Tensor, off: int, n_m: int, out: dict, *, winner: torch.Tensor | None = None,
                         stream: torch.cuda.Stream | None = None) -> dict:
    """anofox_hip_select_scatter_device on torch tensors: `sub` is a sub-batch's DeviceBatch.results() (None with n_m = 0), `out` holds
    "yhat", "lower", "upper" [n_series, h] and "model_code", "status" int32 [n_series] (each may be missing); with `winner` the rows of
    series whose winner is -1 become NaN / code 0 / lib.INSUFFICIENT_DATA.  Returns `out`."""
    L = _lib.load()
    some = next(t for t in (out.get("yhat"), out.get("lower"), out.get("upper")) if t is not None)
    n, h = int(some.shape[0]), int(some.shape[1])
    dev = some.device
    if L.anofox_hip_set_device(dev.index or 0) != 0:
        raise RuntimeError(f"hipSetDevice({dev.index or 0}) failed")
    for k in ("yhat", "lower", "upper"):
        t = out.get(k)
        assert t is None or (t.dtype == torch.float64 and t.is_cuda and t.is_contiguous() and tuple(t.shape) == (n, h))
    for k in ("model_code", "status"):
        t = out.get(k)
        assert t is None or (t.dtype == torch.int32 and t.is_cuda and t.is_contiguous() and t.numel() >= n)
    sub = sub or {}
    if n_m:
        for k in ("yhat", "lower", "upper"):
            assert out.get(k) is None or (sub[k].is_contiguous() and int(sub[k].shape[0]) >= n_m and int(sub[k].shape[1]) == h)
    st = stream if stream is not None else torch.cuda.current_stream(dev)
    ptr = lambda t: t.data_ptr() if t is not None else None
    err = _lib.AnofoxError()
    ok = L.anofox_hip_select_scatter_device(ptr(sub.get("yhat")), ptr(sub.get("lower")), ptr(sub.get("upper")), ptr(sub.get("model_code")),
                                            ptr(sub.get("status")), ptr(members), int(off), int(n_m), h, ptr(winner), n, ptr(out.get("yhat")),
                                            ptr(out.get("lower")), ptr(out.get("upper")), ptr(out.get("model_code")), ptr(out.get("status")),
                                            C.c_void_p(st.cuda_stream), C.byref(err))
    if not ok:
        exc = ValueError if err.code == _lib.INVALID_INPUT else RuntimeError
        raise exc(f"anofox_hip_select_scatter_device failed: [{err.code}] {err.message.decode()}")
    return out


def score_block(actual: torch.Tensor, forecast: torch.Tensor, metric: str, *, n_groups: int | None = None,
                stream: torch.cuda.Stream | None = None):
    """One figure of anofox_hip_metrics_device per row group of two series-major blocks [n_groups, t_rows] (drop_nan: a row in which
    either block holds a NaN does not count) -> (score fp64 [ld], status int32 [n_groups]: 0, or 1 with a NaN score where no row is
    left).  With the [n_pairs, h] blocks of backtest_block viewed as [n_series, F * h] this is a method's score per series."""
    L = _lib.load()
    if metric not in _lib.SELECT_CRITERIA:
        raise ValueError(f"Invalid input: unknown criterion '{metric}' (one of {', '.join(_lib.SELECT_CRITERIA)})")
    fig = _lib.SELECT_CRITERIA.index(metric)
    assert actual.dtype == torch.float64 and actual.is_cuda and actual.is_contiguous() and actual.dim() == 2
    assert forecast.dtype == torch.float64 and forecast.is_cuda and forecast.is_contiguous() and tuple(forecast.shape) == tuple(actual.shape)
    n, t_rows = int(actual.shape[0]), int(actual.shape[1])
    n = n if n_groups is None else int(n_groups)
    dev = actual.device
    ld = max((n + 63) // 64 * 64, 64)
    figures = torch.full((12, ld), float("nan"), dtype=torch.float64, device=dev)
    status = torch.ones(max(n, 1), dtype=torch.int32, device=dev)
    lengths = torch.full((max(n, 1),), t_rows, dtype=torch.int32, device=dev)
    st = stream if stream is not None else torch.cuda.current_stream(dev)
    err = _lib.AnofoxError()
    ok = L.anofox_hip_metrics_device(actual.data_ptr(), forecast.data_ptr(), None, None, None, None, 0, None, 0, t_rows, 1, lengths.data_ptr(),
                                     n, t_rows, 1 << fig, 0.5, True, figures.data_ptr(), ld, status.data_ptr(), C.c_void_p(st.cuda_stream),
                                     C.byref(err))
    if not ok:
        raise RuntimeError(f"anofox_hip_metrics_device failed: [{err.code}] {err.message.decode()}")
    return figures[fig], status[:n]


def select_block(y: torch.Tensor, lengths: torch.Tensor, methods, folds, *, metric: str = "rmse", mode: str = "pick", fallback: int = -1,
                 n_series: int | None = None, stream: torch.cuda.Stream | None = None) -> dict:
    """Choose the forecast method per series from backtest scores, on a resident block, without a host copy: expand once -> one
    backtest batch per method on the shared expanded block -> score per series (anofox_hip_metrics_device over each series' F * h
    backtest cells, drop_nan) -> anofox_hip_select_winner_device -> mode "pick": gather the winners' columns, one sub-batch per method
    that won something, scatter back; modes "mean" / "median" / "inverse_score": every method on the whole block, combined per cell.

    y [t_rows, ld] fp64 time-major without NULLs, lengths int32 [>= n_series], one HIP device, contiguous; methods: a list of 1 .. 16
    ForecastOptions of one horizon; folds as for backtest_block; metric one of lib.SELECT_CRITERIA; fallback in [-1, len(methods)): the
    method of a series without an admissible score (-1: none, its rows are NaN with status lib.INSUFFICIENT_DATA).  An ensemble mode
    needs ld == n_series rounded up to 64 (the block is run as it lies).

    Returns {"winner" int32 [n], "best_score" fp64 [n], "from_fallback" uint8 [n], "scores" fp64 [M, ld_n], "score_status" int32 [M, n],
    "offsets" numpy int32 [M + 1] (the one device-to-host read), "members" int32 [n]; the final "yhat", "lower", "upper" fp64 [n, h],
    "model_code", "status" int32 [n] (an ensemble has no intervals -- lower / upper are NaN, conformal_block on selected_backtest gives
    them -- model code 0 and status 0 / lib.INSUFFICIENT_DATA); "selected_backtest": {"yhat", "actual" fp64 [n_pairs, h], "valid" uint8
    [n_pairs, h], "n_rows" int32 [n_pairs]}, the picked or combined backtest forecasts in the layout conformal_block(...,
    series_major=True) takes viewed as [n, F * h]; "backtests": the per-method backtest_block dicts; "sub_batches": in pick mode
    [(method, off, n_m, DeviceBatch)] (model names: batch.model_name(code, j) for members[off + j]), else the M whole-block batches;
    "n_folds", "horizon"}."""
    L = _lib.load()
    h = _check_methods(methods)
    M = len(methods)
    if metric not in _lib.SELECT_CRITERIA:
        raise ValueError(f"Invalid input: unknown criterion '{metric}' (one of {', '.join(_lib.SELECT_CRITERIA)})")
    code = _lib.select_mode(mode)
    if not -1 <= int(fallback) < M:
        raise ValueError(f"Invalid input: fallback {int(fallback)} is outside [-1, {M})")
    assert y.dtype == torch.float64 and y.is_cuda and y.is_contiguous() and y.dim() == 2
    t_rows, ld = int(y.shape[0]), int(y.shape[1])
    n = ld if n_series is None else int(n_series)
    assert lengths.dtype == torch.int32 and lengths.is_cuda and lengths.is_contiguous() and lengths.numel() >= n
    dev = y.device
    if L.anofox_hip_set_device(dev.index or 0) != 0:
        raise RuntimeError(f"hipSetDevice({dev.index or 0}) failed")
    st = stream if stream is not None else torch.cuda.current_stream(dev)
    F = len(folds)
    nan = float("nan")
    # the backtest of every method on ONE expanded block, scored per series
    expanded = backtest_expand_block(y, lengths, folds, n_series=n, stream=st)
    n_pairs = int(expanded["n_pairs"])
    ld_n = max((n + 63) // 64 * 64, 64)
    scores = torch.full((M, ld_n), nan, dtype=torch.float64, device=dev)
    score_status = torch.ones((M, n), dtype=torch.int32, device=dev)
    backtests = []
    for m, o in enumerate(methods):
        bt = backtest_block(y, lengths, o, folds, n_series=n, metric=metric, stream=st, expanded=expanded)
        backtests.append(bt)
        if n_pairs and n:
            sc, ss = score_block(bt["actual"].view(n, F * h), bt["yhat"].view(n, F * h), metric, stream=st)
            scores[m, :n] = sc[:n]
            score_status[m] = ss
    chosen = select_winner_block(scores, score_status, fallback, n_series=n, stream=st)
    winner, members = chosen["winner"], chosen["members"]
    offsets = chosen["offsets"].cpu().numpy()
    final = {"yhat": torch.empty((n, h), dtype=torch.float64, device=dev), "lower": torch.empty((n, h), dtype=torch.float64, device=dev),
             "upper": torch.empty((n, h), dtype=torch.float64, device=dev), "model_code": torch.zeros(n, dtype=torch.int32, device=dev),
             "status": torch.zeros(n, dtype=torch.int32, device=dev)}
    subs = []
    if code == 0:
        for m, o in enumerate(methods):
            off, n_m = int(offsets[m]), int(offsets[m + 1] - offsets[m])
            if n_m == 0:
                continue
            g = select_gather_block(y, lengths, members, off, n_m, n_series=n, stream=st)
            batch = DeviceBatch(n_m, t_rows, o, dev)
            batch.set_block(g["y"], g["lengths"])
            batch.run(st)
            select_scatter_block(batch.results(), members, off, n_m, final, stream=st)
            subs.append((m, off, n_m, batch))
        select_scatter_block(None, members, 0, 0, final, winner=winner, stream=st)
    else:
        if ld != ld_n:
            raise ValueError(f"an ensemble mode runs the block as it lies: ld must be {ld_n} (n_series rounded up to 64), got {ld}")
        fulls, fstat = [], torch.zeros((M, n), dtype=torch.int32, device=dev)
        for m, o in enumerate(methods):
            batch = DeviceBatch(n, t_rows, o, dev)
            batch.set_block(y, lengths)
            batch.run(st)
            r = batch.results()
            fulls.append(r["yhat"])
            fstat[m] = r["status"]
            subs.append((m, 0, n, batch))
        c = combine_block(fulls, code, status=fstat, winner=winner, weights=scores, group_div=1, stream=st)
        final["yhat"] = c["y"]
        final["lower"].fill_(nan)
        final["upper"].fill_(nan)
        final["status"] = torch.where(c["row_status"] == 0, 0, _lib.INSUFFICIENT_DATA).to(torch.int32)
    # the picked or combined backtest forecasts, in the pair order of the methods' own
    if n_pairs:
        bstat = torch.stack([bt["status"] for bt in backtests]).contiguous()
        sel_yhat = combine_block([bt["yhat"] for bt in backtests], code, status=bstat, winner=winner, weights=scores, group_div=F,
                                 stream=st)["y"]
        if code == 0:
            sel_actual = combine_block([bt["actual"] for bt in backtests], 0, status=bstat, winner=winner, group_div=F, stream=st)["y"]
        else:                                                   # the test rows of every live pair, whatever became of its forecasts
            sel_actual = torch.empty_like(sel_yhat)
            work = torch.empty((2,) + tuple(sel_yhat.shape), dtype=torch.float64, device=dev)
            rows = torch.zeros(n_pairs, dtype=torch.int32, device=dev)
            zero = torch.zeros(n_pairs, dtype=torch.int32, device=dev)
            err = _lib.AnofoxError()
            ok = L.anofox_hip_backtest_collect_device(y.data_ptr(), ld, n, t_rows, _lib.make_folds(folds), F, expanded["n_test"].data_ptr(),
                                                      zero.data_ptr(), sel_yhat.data_ptr(), None, None, h, str(metric).encode(),
                                                      sel_actual.data_ptr(), work[0].data_ptr(), work[1].data_ptr(), None, rows.data_ptr(),
                                                      None, C.c_void_p(st.cuda_stream), C.byref(err))
            if not ok:
                raise RuntimeError(f"anofox_hip_backtest_collect_device failed: [{err.code}] {err.message.decode()}")
    else:
        sel_yhat = torch.empty((0, h), dtype=torch.float64, device=dev)
        sel_actual = torch.empty((0, h), dtype=torch.float64, device=dev)
    valid = (~torch.isnan(sel_yhat) & ~torch.isnan(sel_actual)).to(torch.uint8)
    selected = {"yhat": sel_yhat, "actual": sel_actual, "valid": valid, "n_rows": valid.sum(1).to(torch.int32)}
    return {"winner": winner, "best_score": chosen["best_score"], "from_fallback": chosen["from_fallback"], "scores": scores,
            "score_status": score_status, "offsets": offsets, "members": members, **final, "selected_backtest": selected,
            "backtests": backtests, "sub_batches": subs, "n_folds": F, "horizon": h}


def _ets_notation_parts(notation: str) -> tuple:
    """"AAdN" -> (0, 2, 0): the error, trend and season indices of spec id = error * 15 + trend * 3 + season."""
    return "AM".index(notation[0]), ("N", "A", "Ad", "M", "Md").index(notation[1:-1]), "NAM".index(notation[-1])


class DeviceBatch:
    """anofox_hip_batch_* over torch-owned HBM."""

    def __init__(self, n_series: int, t_max: int, opts: _lib.ForecastOptions, device: torch.device | str = "cuda:0"):
        self.L = _lib.load()
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("DeviceBatch needs a HIP device (no CPU fallback)")
        idx = self.device.index or 0
        if self.L.anofox_hip_set_device(idx) != 0:
            raise RuntimeError(f"hipSetDevice({idx}) failed")
        torch.cuda.set_device(idx)
        self.n, self.t_max, self.opts = int(n_series), int(t_max), opts
        self.h = int(opts.horizon)
        handle = C.c_void_p()
        err = _lib.AnofoxError()
        if not self.L.anofox_hip_batch_create(self.n, self.t_max, C.byref(opts), C.byref(handle), C.byref(err)):
            raise RuntimeError(f"anofox_hip_batch_create failed: [{err.code}] {err.message.decode()}")
        self.handle = handle
        self.ld = int(self.L.anofox_hip_batch_ld(handle))
        self._y = self._len = None
        self._side = None            # launch stream of runs asked for on torch's null stream (run)

    def set_block(self, y_time_major: torch.Tensor, lengths: torch.Tensor):
        assert y_time_major.dtype == torch.float64 and y_time_major.is_cuda and y_time_major.is_contiguous()
        assert tuple(y_time_major.shape) == (self.t_max, self.ld), (tuple(y_time_major.shape), (self.t_max, self.ld))
        assert lengths.dtype == torch.int32 and lengths.is_cuda and lengths.numel() >= self.n
        self._y, self._len = y_time_major, lengths
        err = _lib.AnofoxError()
        if not self.L.anofox_hip_batch_set_device_block(self.handle, y_time_major.data_ptr(), self.ld, lengths.data_ptr(), C.byref(err)):
            raise RuntimeError(f"set_device_block failed: [{err.code}] {err.message.decode()}")

    def set_fixed_params(self, alpha: float, beta: float = 0.0, gamma: float = 0.0, phi: float = 1.0):
        """ETS(spec) with given smoothing parameters: one streamed pass per series, no optimiser (BASELINE config 2)."""
        err = _lib.AnofoxError()
        if not self.L.anofox_hip_batch_set_fixed_params(self.handle, float(alpha), float(beta), float(gamma), float(phi), C.byref(err)):
            raise RuntimeError(f"set_fixed_params failed: [{err.code}] {err.message.decode()}")

    def set_arima_method(self, method: int):
        """AutoARIMA estimation method of this batch: lib.ARIMA_CSS (default) or lib.ARIMA_CSS_ML (exact-likelihood refit)."""
        err = _lib.AnofoxError()
        if not self.L.anofox_hip_batch_set_arima_method(self.handle, int(method), C.byref(err)):
            raise RuntimeError(f"set_arima_method failed: [{err.code}] {err.message.decode()}")

    def set_exog(self, x: torch.Tensor | None, future: torch.Tensor | None = None):
        """Adopt the regressor blocks (no copy; kept alive by this object): x [k, t_max, ld] and future [k, horizon, ld], fp64 on the
        batch's device, regressor j of series s at x[j, t, s] / future[j, i, s].  ARIMA and AutoARIMA batches then run ARIMAX; every
        other model ignores the blocks.  set_exog(None) clears them."""
        err = _lib.AnofoxError()
        if x is None:
            ok = self.L.anofox_hip_batch_set_exog_device(self.handle, None, None, 0, C.byref(err))
            self._x = self._f = None
        else:
            k = int(x.shape[0])
            assert x.dtype == torch.float64 and x.is_cuda and x.is_contiguous() and tuple(x.shape) == (k, self.t_max, self.ld), tuple(x.shape)
            assert future is not None and future.dtype == torch.float64 and future.is_cuda and future.is_contiguous()
            assert tuple(future.shape) == (k, self.h, self.ld), tuple(future.shape)
            ok = self.L.anofox_hip_batch_set_exog_device(self.handle, x.data_ptr(), future.data_ptr(), k, C.byref(err))
            if ok:
                self._x, self._f = x, future
        if not ok:
            raise RuntimeError(f"set_exog_device failed: [{err.code}] {err.message.decode()}")

    def exog_coefficients(self) -> dict:
        """Intercept [n], beta [n, k] (0.0 where a regressor was left out) and used [n, k] of the last ARIMAX run (waits for it)."""
        k = int(self._x.shape[0]) if getattr(self, "_x", None) is not None else 0
        b0 = np.zeros(self.n)
        beta = np.zeros((self.n, k))
        used = np.zeros(self.n, dtype=np.uint32)
        err = _lib.AnofoxError()
        if not self.L.anofox_hip_batch_exog_coefficients(self.handle, b0.ctypes.data, beta.ctypes.data, used.ctypes.data, C.byref(err)):
            raise RuntimeError(f"exog_coefficients failed: [{err.code}] {err.message.decode()}")
        return {"intercept": b0, "beta": beta, "used": ((used[:, None] >> np.arange(k, dtype=np.uint32)[None, :]) & 1).astype(bool)}

    def periods(self) -> np.ndarray:
        """The seasonal period every series runs with (auto-detected on the device when the options ask for it)."""
        out = np.zeros(self.n, dtype=np.int32)
        if not self.L.anofox_hip_batch_periods(self.handle, out.ctypes.data):
            raise RuntimeError("anofox_hip_batch_periods: no block set")
        return out

    def run(self, stream: torch.cuda.Stream | None = None):
        """One fit + forecast of the block, asynchronous and ORDERED on `stream` (torch's current stream by default): what was
        enqueued there before is visible to the run, what is enqueued there afterwards -- torch ops on results(), a collective -- sees
        the run's results.  The null stream cannot carry the run itself (the C entry reads a null handle as "the batch's own stream", a
        non-blocking one the null stream does not wait for: until the last day of round 6 a consumer on torch's default stream, the
        multi-rank gather of bench.py among them, could read the result arrays while the closing kernels were still writing them),
        so a run asked for on the null stream goes to a side stream of this batch, fenced against it on both ends."""
        cur = stream if stream is not None else torch.cuda.current_stream(self.device)
        st = cur
        if cur.cuda_stream == 0:
            if self._side is None:
                self._side = torch.cuda.Stream(device=self.device)
            self._side.wait_stream(cur)
            st = self._side
        err = _lib.AnofoxError()
        ok = self.L.anofox_hip_batch_run(self.handle, C.c_void_p(st.cuda_stream), C.byref(err))
        if st is not cur:
            cur.wait_stream(st)
        if not ok:
            raise RuntimeError(f"anofox_hip_batch_run failed: [{err.code}] {err.message.decode()}")

    def stats(self) -> dict:
        s = _lib.AnofoxHipStats()
        if not self.L.anofox_hip_batch_stats(self.handle, C.byref(s)):
            raise RuntimeError("anofox_hip_batch_stats failed")
        return {f: getattr(s, f) for f, _ in s._fields_}

    SPEC_CLASSES = ("additive", "general", "damped_mul_trend")

    def lane_stats(self) -> dict:
        """Lane-level efficiency of the round kernels of the last run (include/anofox_fcst_hip.h AnofoxHipLaneStats): per spec class and
        per spec, live lane-passes / (64 x wave passes)."""
        s = _lib.AnofoxHipLaneStats()
        if not self.L.anofox_hip_batch_lane_stats(self.handle, C.byref(s), C.sizeof(s)):
            raise RuntimeError("anofox_hip_batch_lane_stats failed")
        eff = lambda live, waves: round(live / (64.0 * waves), 4) if waves else None
        E, T, S = "AM", ("N", "A", "Ad", "M", "Md"), "NAM"
        out = {"by_class": {}, "by_spec": {}}
        tw = tl = 0
        for c, name in enumerate(self.SPEC_CLASSES):
            w, l = int(s.wave_passes[c]), int(s.live_lane_passes[c])
            tw += w; tl += l
            out["by_class"][name] = {"wave_passes": w, "live_lane_passes": l, "lane_efficiency": eff(l, w)}
        out["wave_passes"], out["live_lane_passes"], out["lane_efficiency"] = tw, tl, eff(tl, tw)
        for k in range(int(s.n_slots)):
            sid = int(s.slot_spec_id[k])
            name = E[sid // 15] + T[(sid % 15) // 3] + S[sid % 3]
            out["by_spec"][name] = {"wave_passes": int(s.slot_wave_passes[k]), "lane_efficiency": eff(int(s.slot_live_lane_passes[k]), int(s.slot_wave_passes[k]))}
        return out

    def results(self) -> dict:
        """Zero-copy torch views of the device result arrays."""
        ptrs = [C.c_void_p() for _ in range(5)]
        self.L.anofox_hip_batch_device_results(self.handle, *[C.byref(p) for p in ptrs])

        def view(ptr, shape, dtype, itemsize):
            n = int(np.prod(shape))
            if n == 0:
                return torch.empty(shape, dtype=dtype, device=self.device)
            iface = {"shape": tuple(shape), "typestr": {8: "<f8", 4: "<i4"}[itemsize], "data": (ptr.value, False), "version": 2}
            holder = type("H", (), {"__cuda_array_interface__": iface})()
            return torch.as_tensor(holder, device=self.device)

        return {
            "yhat": view(ptrs[0], (self.n, self.h), torch.float64, 8),
            "lower": view(ptrs[1], (self.n, self.h), torch.float64, 8),
            "upper": view(ptrs[2], (self.n, self.h), torch.float64, 8),
            "model_code": view(ptrs[3], (self.n,), torch.int32, 4),
            "status": view(ptrs[4], (self.n,), torch.int32, 4),
        }

    def inspect_device(self, fitted: bool = True) -> dict:
        """anofox_hip_batch_inspect_device: the fit state of an AutoETS or ETS(spec) batch that has been run, left on the device.

        Returns {"info": fp64 [8, ld] (rows alpha, beta, gamma, phi, aic, aicc, bic, sse), "states": fp64 [2 + max(m, 1), ld] (level,
        growth, seasonal state of phase j in row 2 + j), "fitted": fp64 [max(t_max, 1), ld] time-major or None, "spec": int32 [n] --
        error * 15 + trend * 3 + season of the model every series was fitted with, -1 where none was --, "m": the batch's period}:
        what ets_innovations_block and ets_paths_block take.  NaN wherever a series or a spec has no value.  Waits for the passes."""
        per = self.periods()
        m = max(int(per[0]), 1) if self.n else 1
        info = torch.empty((8, self.ld), dtype=torch.float64, device=self.device)
        states = torch.empty((2 + m, self.ld), dtype=torch.float64, device=self.device)
        fit = torch.empty((max(self.t_max, 1), self.ld), dtype=torch.float64, device=self.device) if fitted else None
        torch.cuda.current_stream(self.device).synchronize()       # (the blocks exist before the batch's own stream writes them)
        err = _lib.AnofoxError()
        if not self.L.anofox_hip_batch_inspect_device(self.handle, info.data_ptr(), states.data_ptr(), fit.data_ptr() if fitted else None,
                                                      C.byref(err)):
            raise _paths_failed("anofox_hip_batch_inspect_device", err)
        res = self.results()
        if (self.opts.model or b"").decode() == "AutoETS":
            spec = res["model_code"] - 100
        else:
            e, t, s = _ets_notation_parts(self.opts.ets_model.decode())
            if s != 0 and int(per[0]) <= 1:
                s = 0                                                # no usable period: the spec ran as its non-seasonal sibling
            spec = torch.full((self.n,), e * 15 + t * 3 + s, dtype=torch.int32, device=self.device)
        spec = torch.where(res["status"] == 0, spec, torch.full_like(spec, -1)).to(torch.int32).contiguous()
        return {"info": info, "states": states, "fitted": fit, "spec": spec, "m": m}

    def arima_fit_device(self) -> dict:
        """anofox_hip_batch_arima_fit_device: the fit of an AutoARIMA batch that has been run, left on the device.

        Returns {"orders": int32 [8, ld] (rows lib.ARIMA_FIT_ORDER_ROWS), "coef": fp64 [16, ld] (rows phi 1..5, theta 1..5, Phi 1..2,
        Theta 1..2, constant, aicc), "m": the batch's period}: what arima_innovations_block and arima_paths_block take.  A series
        nothing was fitted to has zero orders and NaN coefficients.  Waits for the pass."""
        per = self.periods()
        m = max(int(per[0]), 1) if self.n else 1
        orders = torch.zeros((8, self.ld), dtype=torch.int32, device=self.device)
        coef = torch.full((16, self.ld), float("nan"), dtype=torch.float64, device=self.device)
        torch.cuda.current_stream(self.device).synchronize()       # (the blocks exist before the batch's own stream writes them)
        err = _lib.AnofoxError()
        if not self.L.anofox_hip_batch_arima_fit_device(self.handle, orders.data_ptr(), coef.data_ptr(), C.byref(err)):
            raise _paths_failed("anofox_hip_batch_arima_fit_device", err)
        return {"orders": orders, "coef": coef, "m": m}

    def model_name(self, code: int, series: int | None = None) -> str:
        """Name of a model code; with `series`, the name anofox_hip_batch_fetch gives that series (an AutoARIMA code carries the
        period the series was fitted with -- detected periods included)."""
        buf = (C.c_char * 64)()
        if series is None:
            self.L.anofox_hip_model_name(C.byref(self.opts), int(code), buf)
        else:
            self.L.anofox_hip_batch_model_name(self.handle, int(series), int(code), buf)
        return buf.value.decode()

    def close(self):
        if getattr(self, "handle", None):
            self.L.anofox_hip_batch_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
