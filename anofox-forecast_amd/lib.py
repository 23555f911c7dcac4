"""ctypes binding of libanofox_fcst_hip.so (the C-ABI of include/anofox_fcst_hip.h).

The product path is the HIP library and nothing else: importing this module without the built
library, or calling it without a GPU, fails loudly.  The structs mirror the reference's
cbindgen header (src/include/anofox_fcst_ffi.h:72-84, 269-272, 1036-1145).
"""
from __future__ import annotations

import ctypes as C
import os

# The batch path runs the candidate ETS specs on concurrent HIP streams; ROCm maps streams onto 4
# hardware queues by default, which serialises them.  Must be set before the HIP runtime initialises.
os.environ.setdefault("GPU_MAX_HW_QUEUES", "16")   # measured best of 4/8/16/24/32 on MI355X

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("ANOFOX_HIP_LIB", os.path.join(_HERE, "libanofox_fcst_hip.so"))   # override: A/B builds only

SUCCESS, NULL_POINTER, INVALID_INPUT, COMPUTATION_ERROR, ALLOCATION_ERROR, INVALID_MODEL = 0, 1, 2, 3, 4, 5
INSUFFICIENT_DATA, INVALID_DATE_FORMAT, INVALID_FREQUENCY, PANIC_CAUGHT, INTERNAL_ERROR = 6, 7, 8, 9, 10


class AnofoxError(C.Structure):
    _fields_ = [("code", C.c_int), ("message", C.c_char * 256)]


class ForecastOptions(C.Structure):
    _fields_ = [
        ("model", C.c_char * 32),
        ("ets_model", C.c_char * 8),
        ("horizon", C.c_int),
        ("confidence_level", C.c_double),
        ("seasonal_period", C.c_int),
        ("auto_detect_seasonality", C.c_bool),
        ("include_fitted", C.c_bool),
        ("include_residuals", C.c_bool),
        ("window", C.c_int),
        ("seasonal_periods_str", C.c_char * 64),
        ("model_pool", C.c_char * 32),
        ("laplace_variant", C.c_char * 16),
        ("laplace_seasonal_batch_init", C.c_bool),
    ]


class ForecastResult(C.Structure):
    _fields_ = [
        ("point_forecasts", C.POINTER(C.c_double)),
        ("lower_bounds", C.POINTER(C.c_double)),
        ("upper_bounds", C.POINTER(C.c_double)),
        ("fitted_values", C.POINTER(C.c_double)),
        ("residuals", C.POINTER(C.c_double)),
        ("n_forecasts", C.c_size_t),
        ("n_fitted", C.c_size_t),
        ("model_name", C.c_char * 64),
        ("aic", C.c_double),
        ("bic", C.c_double),
        ("mse", C.c_double),
    ]


class AnofoxHipStats(C.Structure):
    _fields_ = [
        ("n_series", C.c_uint64),
        ("t_max", C.c_uint64),
        ("n_problems", C.c_uint64),
        ("total_passes", C.c_uint64),
        ("max_passes", C.c_uint64),
        ("total_evals", C.c_uint64),
        ("algorithmic_bytes", C.c_uint64),
        ("fit_kernel_ms", C.c_double),
        ("total_device_ms", C.c_double),
        ("fit_kernel_launches", C.c_uint32),
        ("y_storage", C.c_uint32),
        ("total_iters", C.c_uint64),
        ("min_pass_bytes", C.c_uint64),
    ]


class AnofoxHipLaneStats(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint64),
        ("wave_passes", C.c_uint64 * 3),
        ("live_lane_passes", C.c_uint64 * 3),
        ("n_slots", C.c_uint32),
        ("reserved", C.c_uint32),
        ("slot_spec_id", C.c_int32 * 30),
        ("slot_wave_passes", C.c_uint64 * 30),
        ("slot_live_lane_passes", C.c_uint64 * 30),
    ]


assert C.sizeof(ForecastOptions) == 184 and C.sizeof(ForecastResult) == 144 and C.sizeof(AnofoxError) == 260

class MstlResult(C.Structure):
    _fields_ = [
        ("trend", C.POINTER(C.c_double)),
        ("seasonal_components", C.POINTER(C.POINTER(C.c_double))),
        ("remainder", C.POINTER(C.c_double)),
        ("n_observations", C.c_size_t),
        ("n_seasonal", C.c_size_t),
        ("seasonal_periods", C.POINTER(C.c_int)),
        ("decomposition_applied", C.c_bool),
    ]


class BocpdResult(C.Structure):
    _fields_ = [
        ("is_changepoint", C.POINTER(C.c_bool)),
        ("changepoint_probability", C.POINTER(C.c_double)),
        ("n_points", C.c_size_t),
        ("changepoint_indices", C.POINTER(C.c_size_t)),
        ("n_changepoints", C.c_size_t),
    ]


class ChangepointResult(C.Structure):
    _fields_ = [
        ("changepoints", C.POINTER(C.c_size_t)),
        ("n_changepoints", C.c_size_t),
        ("cost", C.c_double),
    ]


class TsStatsResult(C.Structure):
    """include/anofox_fcst_hip.h TsStatsResult: 36 figures and has_date_metrics (296 bytes)."""
    _fields_ = ([(n, C.c_size_t) for n in ("length", "n_nulls", "n_nan", "n_zeros", "n_positive", "n_negative", "n_unique_values")]
                + [("is_constant", C.c_bool)]
                + [(n, C.c_size_t) for n in ("n_zeros_start", "n_zeros_end", "plateau_size", "plateau_size_nonzero")]
                + [(n, C.c_double) for n in ("mean", "median", "std_dev", "variance", "min", "max", "range", "sum", "skewness",
                                             "kurtosis", "tail_index", "bimodality_coef", "trimmed_mean", "coef_variation", "q1", "q3",
                                             "iqr", "autocorr_lag1", "trend_strength", "seasonality_strength", "entropy", "stability")]
                + [("expected_length", C.c_size_t), ("n_gaps", C.c_size_t), ("has_date_metrics", C.c_bool)])


class DataQualityResult(C.Structure):
    """include/anofox_fcst_hip.h DataQualityResult: five scores, n_gaps, n_missing, is_constant (64 bytes)."""
    _fields_ = ([(n, C.c_double) for n in ("structural_score", "temporal_score", "magnitude_score", "behavioral_score", "overall_score")]
                + [("n_gaps", C.c_size_t), ("n_missing", C.c_size_t), ("is_constant", C.c_bool)])


assert C.sizeof(DataQualityResult) == 64
QUALITY_FP_FIELDS = tuple(n for n, _ in DataQualityResult._fields_[:5])    # rows of out_fp of anofox_hip_quality_device
QUALITY_INT_FIELDS = ("n_gaps", "n_missing", "is_constant", "status")      # rows of its out_int
QUALITY_FIELDS = tuple(n for n, _ in DataQualityResult._fields_)
QUALITY_OK, QUALITY_NAN = 0, 2


class FeaturesResult(C.Structure):
    """include/anofox_fcst_hip.h FeaturesResult (the reference's layout, 24 bytes): both arrays and the names are malloc'ed by the entry."""
    _fields_ = [("features", C.POINTER(C.c_double)), ("feature_names", C.POINTER(C.c_char_p)), ("n_features", C.c_size_t)]


assert C.sizeof(FeaturesResult) == 24
N_FEATURES = 117                         # ANOFOX_HIP_N_FEATURES
FEATURES_MAX_ROWS = 1 << 16              # ANOFOX_HIP_FEATURES_MAX_ROWS
FEATURES_OK, FEATURES_EMPTY, FEATURES_NAN = 0, 1, 2
FEATURES_FAMILIES = ("chains", "sort", "scan", "match", "dft")      # bit i of `families` of anofox_hip_features_families_device


class SeasonalityResult(C.Structure):
    """include/anofox_fcst_hip.h SeasonalityResult (the reference's layout, 40 bytes): detected_periods is malloc'ed by the entry."""
    _fields_ = [("detected_periods", C.POINTER(C.c_int)), ("n_periods", C.c_size_t), ("primary_period", C.c_int),
                ("seasonal_strength", C.c_double), ("trend_strength", C.c_double)]


class AnofoxHipSeasonality(C.Structure):
    """include/anofox_fcst_hip.h AnofoxHipSeasonality: one record of anofox_hip_seasonality_batch (128 bytes, no pointer)."""
    _fields_ = [("periods", C.c_int32 * 5), ("n_periods", C.c_int32), ("primary_period", C.c_int32), ("reserved", C.c_int32),
                ("strengths", C.c_double * 5), ("acf", C.c_double * 5), ("seasonal_strength", C.c_double), ("trend_strength", C.c_double)]


assert C.sizeof(SeasonalityResult) == 40 and C.sizeof(AnofoxHipSeasonality) == 128
# rows of out_int / out_fp of anofox_hip_seasonality_device
SEASONALITY_INT_FIELDS = ("period_0", "period_1", "period_2", "period_3", "period_4", "n_periods", "primary_period", "status")
SEASONALITY_FP_FIELDS = ("strength_0", "strength_1", "strength_2", "strength_3", "strength_4", "acf_0", "acf_1", "acf_2", "acf_3", "acf_4",
                         "seasonal_strength", "trend_strength")
SEASONALITY_OK, SEASONALITY_SHORT = 0, 1
SEASONALITY_LDS_ROWS = 5120     # csrc/kernels.hpp: a block above it is worked on in global memory


class LombScargleResultFFI(C.Structure):
    _fields_ = [(n, C.c_double) for n in ("period", "frequency", "power", "false_alarm_prob")] + [("method", C.c_char * 32)]


class AicPeriodResultFFI(C.Structure):
    _fields_ = [(n, C.c_double) for n in ("period", "aic", "bic", "rss", "r_squared")] + [("method", C.c_char * 32)]


class SazedPeriodResultFFI(C.Structure):
    _fields_ = [(n, C.c_double) for n in ("period", "power", "snr")] + [("method", C.c_char * 32)]


class FlatMultiPeriodResult(C.Structure):
    _fields_ = [
        ("period_values", C.POINTER(C.c_double)),
        ("confidence_values", C.POINTER(C.c_double)),
        ("strength_values", C.POINTER(C.c_double)),
        ("amplitude_values", C.POINTER(C.c_double)),
        ("phase_values", C.POINTER(C.c_double)),
        ("iteration_values", C.POINTER(C.c_size_t)),
        ("matches_expected_values", C.POINTER(C.c_bool)),
        ("matched_expected_values", C.POINTER(C.c_double)),
        ("match_deviation_values", C.POINTER(C.c_double)),
        ("n_periods", C.c_size_t),
        ("primary_period", C.c_double),
        ("method", C.c_char * 32),
    ]


assert (C.sizeof(LombScargleResultFFI), C.sizeof(AicPeriodResultFFI), C.sizeof(SazedPeriodResultFFI), C.sizeof(FlatMultiPeriodResult)) \
    == (64, 72, 56, 120)
# include/anofox_fcst_hip.h: the `method` of anofox_hip_periods_batch / _device and the figures each one returns, in row order
PERIOD_METHODS = {"lomb_scargle": 0, "aic": 1, "sazed": 2}
PERIOD_FIGURES = {"lomb_scargle": ("period", "frequency", "power", "false_alarm_prob"),
                  "aic": ("period", "aic", "bic", "rss", "r_squared"),
                  "sazed": ("period", "power", "snr")}
PERIODS_N_FP = 5


class SsaPeriodResultFFI(C.Structure):
    _fields_ = [("period", C.c_double), ("variance_explained", C.c_double), ("n_eigenvalues", C.c_size_t), ("method", C.c_char * 32)]


class StlPeriodResultFFI(C.Structure):
    _fields_ = [(n, C.c_double) for n in ("period", "seasonal_strength", "trend_strength")] + [("method", C.c_char * 32)]


assert (C.sizeof(SsaPeriodResultFFI), C.sizeof(StlPeriodResultFFI)) == (56, 56)
# include/anofox_fcst_hip.h: the figure rows of anofox_hip_ssa_period_* / anofox_hip_stl_period_*, their status codes and limits
SSA_FIGURES = ("period", "variance_explained", "n_eigenvalues")
STL_FIGURES = ("period", "seasonal_strength", "trend_strength")
PSEARCH_OK, PSEARCH_TOO_SHORT, PSEARCH_OVER_LIMIT, PSEARCH_STL_RANGE, PSEARCH_STL_NO_CANDIDATE = 0, 1, 2, 3, 4
SSA_N_DETECTED, SSA_MAX_WINDOW, SSA_MAX_COMPONENTS, STL_MAX_CANDIDATES, PSEARCH_MAX_ROWS = 4, 2048, 32, 64, 65536
SSA_ROUTES = {"auto": 0, "group": 1}


def ssa_components(n_components=None) -> int:
    """Rows of the eigenvalue output: n_components, or the source's 10 for None / 0."""
    return int(n_components) if n_components else 10


def stl_candidate_count(n_candidates=None) -> int:
    """Rows of the candidate outputs: max(n_candidates or 20, 5), as the source resolves it."""
    return max(int(n_candidates) if n_candidates else 20, 5)


class MatrixProfilePeriodResultFFI(C.Structure):
    _fields_ = [("period", C.c_double), ("confidence", C.c_double), ("n_motifs", C.c_size_t), ("subsequence_length", C.c_size_t),
                ("method", C.c_char * 32)]


assert C.sizeof(MatrixProfilePeriodResultFFI) == 64
# include/anofox_fcst_hip.h: the figure rows of anofox_hip_matrix_profile_*, their status codes and limits
MATRIX_PROFILE_FIGURES = ("period", "confidence", "n_motifs", "subsequence_length", "best_count", "n_tied")
MPROF_OK, MPROF_TOO_SHORT, MPROF_OVER_LIMIT = 0, 1, 2
MPROF_MIN_ROWS, MPROF_MAX_M, MPROF_MAX_ROWS = 32, 2048, 65536


def matrix_profile_subsequence(n, subsequence_length=None) -> int:
    """The effective subsequence length of a series of n rows: min(max(subsequence_length or n / 10, 4), n / 4)."""
    return min(max(int(subsequence_length) if subsequence_length else n // 10, 4), n // 4)


def matrix_profile_rows(t_rows, subsequence_length=None) -> int:
    """Rows of the profile outputs: the profile length n - m + 1 of a series of t_rows rows (0 below 32 rows); no shorter series
    has a longer profile."""
    return 0 if t_rows < MPROF_MIN_ROWS else t_rows - matrix_profile_subsequence(t_rows, subsequence_length) + 1


# include/anofox_fcst_hip.h: bit k of the figure mask of anofox_hip_metrics_batch / _device and row k of their output
METRIC_FIGURES = ("mae", "mse", "rmse", "mape", "smape", "r2", "bias", "rmae", "mase", "quantile_loss", "mqloss", "coverage")
METRICS_MAX_LEVELS = 16


# include/anofox_fcst_hip.h: the conformal entries (anofox_hip_conformal_learn_device / _apply_device / _evaluate_device / _batch)
CONFORMAL_METHODS = {"symmetric": 0, "asymmetric": 1, "adaptive": 2}
CONFORMAL_STRATEGIES = {"split": 0, "crossval": 1, "jackknife+": 2}
CONFORMAL_MAX_LEVELS = 16
CONFORMAL_OK, CONFORMAL_EMPTY, CONFORMAL_NAN, CONFORMAL_DIFFICULTY = 0, 1, 2, 3
CONFORMAL_EVAL_FIGURES = ("coverage", "violation_rate", "mean_width", "winkler_score", "n_observations")


class AnofoxHipConformal(C.Structure):
    """include/anofox_fcst_hip.h AnofoxHipConformal: one group's answer of anofox_hip_conformal_batch (64 bytes)."""
    _fields_ = [("scores_lower", C.POINTER(C.c_double)), ("scores_upper", C.POINTER(C.c_double)), ("sorted", C.POINTER(C.c_double)),
                ("n_residuals", C.c_size_t), ("lower", C.POINTER(C.c_double)), ("upper", C.POINTER(C.c_double)),
                ("n_forecasts", C.c_size_t), ("n_levels", C.c_size_t)]


assert C.sizeof(AnofoxHipConformal) == 64


class ConformalResultFFI(C.Structure):
    """anofox_fcst_ffi.h ConformalResultFFI (types.rs:1427-1444): 80 bytes."""
    _fields_ = [("point", C.POINTER(C.c_double)), ("lower", C.POINTER(C.c_double)), ("upper", C.POINTER(C.c_double)),
                ("n_forecasts", C.c_size_t), ("coverage", C.c_double), ("conformity_score", C.c_double), ("method", C.c_char * 32)]


class ConformalMultiResultFFI(C.Structure):
    """types.rs:1478-1493: lower / upper are [n_levels x n_forecasts], level-major (56 bytes)."""
    _fields_ = [("point", C.POINTER(C.c_double)), ("n_forecasts", C.c_size_t), ("coverage_levels", C.POINTER(C.c_double)),
                ("conformity_scores", C.POINTER(C.c_double)), ("n_levels", C.c_size_t), ("lower", C.POINTER(C.c_double)),
                ("upper", C.POINTER(C.c_double))]


class CalibrationProfileFFI(C.Structure):
    """types.rs:1585-1606: method and strategy are the C enums ConformalMethodFFI / ConformalStrategyFFI (64 bytes)."""
    _fields_ = [("method", C.c_int), ("strategy", C.c_int), ("alphas", C.POINTER(C.c_double)), ("state_vector", C.POINTER(C.c_double)),
                ("state_vector_len", C.c_size_t), ("scores_lower", C.POINTER(C.c_double)), ("scores_upper", C.POINTER(C.c_double)),
                ("n_levels", C.c_size_t), ("n_residuals", C.c_size_t)]


class PredictionIntervalsFFI(C.Structure):
    """types.rs:1628-1643 (56 bytes)."""
    _fields_ = [("point", C.POINTER(C.c_double)), ("n_forecasts", C.c_size_t), ("coverage", C.POINTER(C.c_double)), ("n_levels", C.c_size_t),
                ("lower", C.POINTER(C.c_double)), ("upper", C.POINTER(C.c_double)), ("method", C.c_int)]


class ConformalEvaluationFFI(C.Structure):
    """types.rs:1661-1672 (40 bytes)."""
    _fields_ = [("coverage", C.c_double), ("violation_rate", C.c_double), ("mean_width", C.c_double), ("winkler_score", C.c_double),
                ("n_observations", C.c_size_t)]


assert (C.sizeof(ConformalResultFFI), C.sizeof(ConformalMultiResultFFI), C.sizeof(CalibrationProfileFFI), C.sizeof(PredictionIntervalsFFI),
        C.sizeof(ConformalEvaluationFFI)) == (80, 56, 64, 56, 40)


class FilledValuesResult(C.Structure):
    _fields_ = [("values", C.POINTER(C.c_double)), ("validity", C.POINTER(C.c_uint64)), ("length", C.c_size_t)]


class GapFillResult(C.Structure):
    _fields_ = [("dates", C.POINTER(C.c_int64)), ("values", C.POINTER(C.c_double)), ("validity", C.POINTER(C.c_uint64)),
                ("length", C.c_size_t)]


class AnofoxHipPrepOptions(C.Structure):
    """include/anofox_fcst_hip.h AnofoxHipPrepOptions: the stages of anofox_hip_prepare_device / _batch (32 bytes)."""
    _fields_ = [("gaps", C.c_int32), ("frequency_type", C.c_int32), ("frequency_micros", C.c_int64), ("trim", C.c_int32),
                ("fill", C.c_int32), ("fill_value", C.c_double)]


class AnofoxHipPrepared(C.Structure):
    _fields_ = [("dates", C.POINTER(C.c_int64)), ("values", C.POINTER(C.c_double)), ("validity", C.POINTER(C.c_uint64)),
                ("length", C.c_size_t), ("figures", C.c_int64 * 8), ("min", C.c_double), ("max", C.c_double)]


assert (C.sizeof(FilledValuesResult), C.sizeof(GapFillResult), C.sizeof(AnofoxHipPrepOptions), C.sizeof(AnofoxHipPrepared)) == (24, 32, 32, 112)
PREP_TRIMS = {"none": 0, "leading": 1, "trailing": 2, "edge": 3}
PREP_FILLS = {"none": 0, "const": 1, "forward": 2, "backward": 3, "mean": 4, "interpolate": 5}
# rows of out_int of anofox_hip_prepare_device, in order; out_fp holds min, max
PREP_FIGURES = ("n_input", "n_null_input", "n_inserted", "n_trim_front", "n_trim_back", "n_null_output", "n_nonzero_output", "status")
PREP_OK, PREP_NO_ROOM, PREP_OVER_LIMIT = 0, 1, 2


FREQUENCY_TYPES = {"FIXED": 0, "MONTHLY": 1, "QUARTERLY": 2, "YEARLY": 3}      # include/anofox_fcst_hip.h FrequencyType
STATS_INT_FIELDS = tuple(n for n, _ in TsStatsResult._fields_[:12])
STATS_FP_FIELDS = tuple(n for n, _ in TsStatsResult._fields_[12:34])


class ExogenousRegressor(C.Structure):
    _fields_ = [("values", C.POINTER(C.c_double)), ("n_values", C.c_size_t),
                ("future_values", C.POINTER(C.c_double)), ("n_future", C.c_size_t)]


class ExogenousData(C.Structure):
    _fields_ = [("regressors", C.POINTER(ExogenousRegressor)), ("n_regressors", C.c_size_t)]


class ForecastOptionsExog(C.Structure):
    _fields_ = [
        ("model", C.c_char * 32),
        ("ets_model", C.c_char * 8),
        ("horizon", C.c_int),
        ("confidence_level", C.c_double),
        ("seasonal_period", C.c_int),
        ("auto_detect_seasonality", C.c_bool),
        ("include_fitted", C.c_bool),
        ("include_residuals", C.c_bool),
        ("exog", C.POINTER(ExogenousData)),
        ("window", C.c_int),
        ("seasonal_periods_str", C.c_char * 64),
        ("model_pool", C.c_char * 32),
        ("laplace_variant", C.c_char * 16),
        ("laplace_seasonal_batch_init", C.c_bool),
    ]


class AnofoxHipFold(C.Structure):
    """include/anofox_fcst_hip.h AnofoxHipFold: one fold of the backtest, inclusive row positions (40 bytes)."""
    _fields_ = [(n, C.c_int64) for n in ("fold_id", "train_start", "train_end", "test_start", "test_end")]


assert C.sizeof(AnofoxHipFold) == 40
BACKTEST_WINDOWS = {"expanding": 0, "fixed": 1, "sliding": 2}      # window_type of anofox_hip_backtest_folds


class AnofoxHipHierarchyOptions(C.Structure):
    """include/anofox_fcst_hip.h AnofoxHipHierarchyOptions: route and the member count of the automatic choice (16 bytes)."""
    _fields_ = [("route", C.c_int32), ("tile_min_members", C.c_int32), ("reserved", C.c_int32 * 2)]


assert C.sizeof(AnofoxHipHierarchyOptions) == 16
HIERARCHY_ROUTES = {"auto": 0, "lane": 1, "tile": 2}      # include/anofox_fcst_hip.h ANOFOX_HIERARCHY_ROUTE_*
RECONCILE_METHODS = {"bottom_up": 0, "ols": 1, "wls_struct": 2, "wls_var": 3}      # include/anofox_fcst_hip.h ANOFOX_RECONCILE_*
RECONCILE_MAX_AGG = 16384                                 # ANOFOX_HIP_RECONCILE_MAX_AGG
RECONCILE_MAX_RESIDUAL_ROWS = 8192                        # ANOFOX_HIP_RECONCILE_MAX_RESIDUAL_ROWS (the MinT-shrink entries)


assert C.sizeof(ExogenousRegressor) == 32 and C.sizeof(ExogenousData) == 16 and C.sizeof(ForecastOptionsExog) == 192
MODEL_CODE_ARIMAX = 50             # include/anofox_fcst_hip.h: model_code of a series the ARIMAX path forecast


# every symbol include/anofox_fcst_hip.h declares
class AnofoxHipInspection(C.Structure):
    _fields_ = [("model_code", C.c_int32), ("status", C.c_int32), ("seasonal_period", C.c_int32), ("reserved", C.c_int32),
                ("alpha", C.c_double), ("beta", C.c_double), ("gamma", C.c_double), ("phi", C.c_double),
                ("aic", C.c_double), ("aicc", C.c_double), ("bic", C.c_double), ("sse", C.c_double),
                ("level", C.c_double), ("trend", C.c_double)]


class AnofoxHipArimaFit(C.Structure):
    """include/anofox_fcst_hip.h AnofoxHipArimaFit: the selected AutoARIMA fit of one series (184 bytes)."""
    _fields_ = [(k, C.c_int32) for k in ("status", "model_code", "seasonal_period", "p", "d", "q", "P", "D", "Q", "has_constant",
                                         "n_diff", "models_tried", "evals", "reserved")] + \
               [("phi", C.c_double * 5), ("theta", C.c_double * 5), ("Phi", C.c_double * 2), ("Theta", C.c_double * 2),
                ("constant", C.c_double), ("aicc", C.c_double)]


assert C.sizeof(AnofoxHipArimaFit) == 184


EXPORTED_SYMBOLS = [
    "anofox_ts_forecast", "anofox_free_forecast_result", "anofox_fcst_version", "anofox_ts_forecast_batch",
    "anofox_hip_device_count", "anofox_hip_set_device", "anofox_hip_batch_create", "anofox_hip_batch_destroy",
    "anofox_hip_batch_ld", "anofox_hip_batch_pack_host", "anofox_hip_batch_set_device_block", "anofox_hip_batch_run",
    "anofox_hip_batch_stats", "anofox_hip_batch_device_results", "anofox_hip_batch_fetch", "anofox_hip_model_name", "anofox_hip_batch_model_name",
    "anofox_hip_ingest_create", "anofox_hip_ingest_destroy", "anofox_hip_ingest_append", "anofox_hip_ingest_finish",
    "anofox_hip_ingest_group_keys", "anofox_hip_ingest_last_dates", "anofox_hip_ingest_lengths", "anofox_hip_ingest_values",
    "anofox_hip_ingest_validity", "anofox_hip_batch_pack_ingest", "anofox_hip_batch_inspect", "anofox_hip_batch_arima_fit",
    "anofox_hip_batch_n_series", "anofox_hip_batch_periods", "anofox_hip_batch_set_fixed_params",
    "anofox_hip_set_devices", "anofox_hip_get_devices", "anofox_hip_set_min_series_per_device", "anofox_hip_shard_range",
    "anofox_hip_set_default_arima_method", "anofox_hip_batch_set_arima_method", "anofox_hip_release_caches",
    "anofox_hip_batch_run_many", "anofox_hip_batch_lane_stats", "anofox_hip_selftest_recip", "anofox_hip_selftest_math",
    "anofox_ts_mstl_decomposition", "anofox_free_mstl_result", "anofox_hip_mstl_decompose_batch", "anofox_hip_mstl_decompose_device",
    "anofox_ts_forecast_exog", "anofox_ts_forecast_exog_batch", "anofox_hip_batch_set_exog_device", "anofox_hip_batch_exog_coefficients",
    "anofox_ts_detect_changepoints_bocpd", "anofox_free_bocpd_result", "anofox_hip_changepoints_batch", "anofox_hip_changepoints_device",
    "anofox_ts_detect_changepoints", "anofox_free_changepoint_result", "anofox_hip_pelt_batch", "anofox_hip_pelt_device",
    "anofox_ts_stats", "anofox_ts_stats_with_dates", "anofox_ts_stats_with_dates_and_type", "anofox_free_ts_stats_result",
    "anofox_hip_stats_batch", "anofox_hip_stats_device",
    "anofox_ts_data_quality", "anofox_hip_quality_batch", "anofox_hip_quality_device",
    "anofox_ts_features", "anofox_free_features_result", "anofox_ts_features_list", "anofox_ts_validate_feature_params",
    "anofox_free_warnings", "anofox_hip_features_batch", "anofox_hip_features_device", "anofox_hip_features_families_device",
    "anofox_ts_detect_seasonality", "anofox_ts_analyze_seasonality", "anofox_free_seasonality_result", "anofox_free_int_array",
    "anofox_hip_seasonality_batch", "anofox_hip_seasonality_device",
    "anofox_ts_lomb_scargle", "anofox_ts_aic_period", "anofox_ts_sazed_period", "anofox_ts_detect_periods_flat",
    "anofox_free_flat_multi_period_result", "anofox_hip_periods_batch", "anofox_hip_periods_device",
    "anofox_ts_ssa_period", "anofox_ts_stl_period", "anofox_hip_ssa_period_batch", "anofox_hip_stl_period_batch",
    "anofox_hip_ssa_period_device", "anofox_hip_stl_period_device",
    "anofox_ts_matrix_profile_period", "anofox_hip_matrix_profile_batch", "anofox_hip_matrix_profile_device",
    "anofox_ts_mae", "anofox_ts_mse", "anofox_ts_rmse", "anofox_ts_mape", "anofox_ts_smape", "anofox_ts_r2", "anofox_ts_bias",
    "anofox_ts_rmae", "anofox_ts_mase", "anofox_ts_quantile_loss", "anofox_ts_mqloss", "anofox_ts_coverage",
    "anofox_hip_metrics_batch", "anofox_hip_metrics_device",
    "anofox_ts_fill_nulls_const", "anofox_ts_fill_nulls_mean", "anofox_ts_fill_nulls_interpolate", "anofox_ts_fill_nulls_forward",
    "anofox_ts_fill_nulls_backward", "anofox_ts_fill_gaps", "anofox_free_gap_fill_result", "anofox_free_filled_values_result",
    "anofox_free_double_array", "anofox_hip_prepare_device", "anofox_hip_prepare_batch", "anofox_hip_free_prepared",
    "anofox_hip_conformal_learn_device", "anofox_hip_conformal_apply_device", "anofox_hip_conformal_evaluate_device",
    "anofox_hip_conformal_batch", "anofox_hip_free_conformal",
    "anofox_ts_conformal_quantile", "anofox_ts_conformal_intervals", "anofox_ts_conformal_predict", "anofox_ts_conformal_predict_multi",
    "anofox_ts_conformal_predict_adaptive", "anofox_ts_conformal_predict_asymmetric", "anofox_ts_mean_interval_width",
    "anofox_ts_conformal_learn", "anofox_ts_conformal_apply", "anofox_ts_conformal_coverage", "anofox_ts_conformal_evaluate",
    "anofox_free_conformal_result", "anofox_free_conformal_multi_result", "anofox_free_calibration_profile", "anofox_free_prediction_intervals",
    "anofox_hip_backtest_folds", "anofox_hip_backtest_sizes", "anofox_hip_backtest_expand_device", "anofox_hip_backtest_collect_device",
    "anofox_hip_backtest_batch",
    "anofox_hip_hierarchy_plan", "anofox_hip_hierarchy_device", "anofox_hip_hierarchy_batch",
    "anofox_hip_reconcile_plan", "anofox_hip_reconcile_factor_device", "anofox_hip_reconcile_apply_device", "anofox_hip_reconcile_batch",
    "anofox_hip_reconcile_mint_sizes", "anofox_hip_reconcile_mint_factor_device", "anofox_hip_reconcile_mint_apply_device",
    "anofox_hip_reconcile_mint_batch",
    "anofox_hip_select_winner_device", "anofox_hip_select_gather_device", "anofox_hip_select_scatter_device",
    "anofox_hip_select_combine_device", "anofox_hip_select_batch",
    "anofox_hip_paths_device", "anofox_hip_path_quantiles_device", "anofox_hip_paths_batch",
    "anofox_hip_path_scores_device", "anofox_hip_path_scores_sizes", "anofox_hip_path_energy_device", "anofox_hip_path_scores_batch",
    "anofox_hip_scale_device", "anofox_hip_weighted_scores_device", "anofox_hip_wrmsse_batch",
    "anofox_hip_batch_inspect_device", "anofox_hip_ets_innovations_device", "anofox_hip_ets_paths_device", "anofox_hip_batch_ets_paths",
    "anofox_hip_batch_arima_fit_device", "anofox_hip_arima_innovations_device", "anofox_hip_arima_paths_device", "anofox_hip_batch_arima_paths",
]

# include/anofox_fcst_hip.h block 9: bootstrap sample paths and their quantiles
PATHS_MODES = {"cumulative": 0, "independent": 1}      # ANOFOX_PATHS_*
PATHS_ROUTES = {"auto": 0, "lane": 1}                  # ANOFOX_PATHS_ROUTE_*
PATHS_MAX_PATHS = 2048                                 # ANOFOX_HIP_PATHS_MAX_PATHS
PATHS_MAX_LEVELS = 16                                  # ANOFOX_HIP_PATHS_MAX_LEVELS
PATHS_MAX_POOL_ROWS = 1 << 20                          # ANOFOX_HIP_PATHS_MAX_POOL_ROWS
PATHS_OK, PATHS_EMPTY, PATHS_NAN, PATHS_RAGGED = 0, 1, 2, 3
# block 10: scores of sample paths (ANOFOX_PATH_SCORES_*): done; no step with an actual; a NaN among the column's paths
PATH_SCORES_OK, PATH_SCORES_NO_ACTUAL, PATH_SCORES_NAN = 0, 1, 2
# block 11: scaled, weighted scores (ANOFOX_SCALE_*): done; no lag difference; a NaN in the column or in its tail; constant after t0
SCALE_OK, SCALE_SHORT, SCALE_NAN, SCALE_CONSTANT = 0, 1, 2, 3
SCALED_TRANSFORMS = {"ratio": 0, "root": 1}            # ANOFOX_SCALED_RATIO (loss / scale), ANOFOX_SCALED_ROOT (its square root)
SCALED_MAX_LOSS = 16                                   # ANOFOX_HIP_SCALED_MAX_LOSS
SCALE_ROWS = ("msd", "mad", "n_terms", "tail")         # the rows of out_scale
# block 12: sample paths simulated from the fitted ETS models
ETS_PATHS_INNOVATIONS = {"gaussian": 0, "bootstrap": 1}   # ANOFOX_ETS_PATHS_*
ETS_PATHS_NO_MODEL = 4                                 # ANOFOX_ETS_PATHS_NO_MODEL, beside PATHS_OK / _EMPTY / _NAN / _RAGGED
ETS_PATHS_MAX_PERIOD = 2048                            # ANOFOX_HIP_ETS_PATHS_MAX_PERIOD
ETS_PATHS_MAX_RING = 128                               # ANOFOX_HIP_ETS_PATHS_MAX_RING: R = min(m, horizon)


class AnofoxHipPathsOptions(C.Structure):
    """include/anofox_fcst_hip.h AnofoxHipPathsOptions: mode, joint, route and the seed (24 bytes)."""
    _fields_ = [("mode", C.c_int32), ("joint", C.c_int32), ("route", C.c_int32), ("reserved", C.c_int32), ("seed", C.c_uint64)]


assert C.sizeof(AnofoxHipPathsOptions) == 24


class AnofoxHipEtsPathsOptions(C.Structure):
    """include/anofox_fcst_hip.h AnofoxHipEtsPathsOptions: innovations, joint and the seed (24 bytes)."""
    _fields_ = [("innovations", C.c_int32), ("joint", C.c_int32), ("reserved", C.c_int32 * 2), ("seed", C.c_uint64)]


assert C.sizeof(AnofoxHipEtsPathsOptions) == 24

# include/anofox_fcst_hip.h block 13: sample paths simulated from the fitted AutoARIMA models
ARIMA_PATHS_INNOVATIONS = {"gaussian": 0, "bootstrap": 1}  # ANOFOX_ARIMA_PATHS_*
ARIMA_PATHS_NO_MODEL = 4                                # ANOFOX_ARIMA_PATHS_NO_MODEL, beside PATHS_OK / _EMPTY / _NAN / _RAGGED
ARIMA_PATHS_MAX_PERIOD = 2048                           # ANOFOX_HIP_ARIMA_PATHS_MAX_PERIOD
ARIMA_PATHS_MAX_LDS_ROWS = 128                          # ANOFOX_HIP_ARIMA_PATHS_MAX_LDS_ROWS: 2 min(h, 2 m + 5) + (m < h ? m : 0)
ARIMA_FIT_ORDER_ROWS = ("p", "d", "q", "P", "D", "Q", "has_constant", "n_diff")      # rows of the orders block


class AnofoxHipArimaPathsOptions(C.Structure):
    """include/anofox_fcst_hip.h AnofoxHipArimaPathsOptions: innovations, joint and the seed (24 bytes)."""
    _fields_ = [("innovations", C.c_int32), ("joint", C.c_int32), ("reserved", C.c_int32 * 2), ("seed", C.c_uint64)]


assert C.sizeof(AnofoxHipArimaPathsOptions) == 24

# include/anofox_fcst_hip.h block 8: the choice of a method per series
SELECT_MAX_METHODS = 16
SELECT_MODES = {"pick": 0, "mean": 1, "median": 2, "inverse_score": 3}
SELECT_CRITERIA = ("mae", "mse", "rmse", "mape", "smape")      # their rows of anofox_hip_metrics_device's figures are 0 .. 4

ARIMA_CSS, ARIMA_CSS_ML = 0, 1     # include/anofox_fcst_hip.h: ANOFOX_ARIMA_CSS / ANOFOX_ARIMA_CSS_ML

_lib = None


MATH_FNS = {"log": 0, "exp": 1, "scalbn": 2, "pow_step": 3, "pow_near1": 4, "pow_pos": 5, "sincos": 6}      # AnofoxHipMathFn
NM_BLOCK = 64                                          # csrc/nm.hpp: the fit kernels' workgroup; anofox_hip_selftest_math takes it or 256


def load():
    """Load the HIP library; raises if it has not been built (no fallback)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(f"{LIB_PATH} is missing: build it with `make -C anofox-forecast_amd/csrc` "
                           "(or __graft_entry__.build()); the backend has no CPU fallback")
    try:
        # PyTorch-ROCm bundles its own HIP runtime; load it first so that this library binds to the
        # same one (two HIP runtimes in one process do not share devices, streams or allocations).
        import torch  # noqa: F401
    except ImportError:
        pass
    L = C.CDLL(LIB_PATH)
    P = C.POINTER
    L.anofox_ts_forecast.restype = C.c_bool
    L.anofox_ts_forecast.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, P(ForecastOptions), P(ForecastResult), P(AnofoxError)]
    L.anofox_free_forecast_result.argtypes = [P(ForecastResult)]
    L.anofox_fcst_version.restype = C.c_char_p
    L.anofox_ts_forecast_batch.restype = C.c_bool
    L.anofox_ts_forecast_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, P(ForecastOptions), C.c_void_p,
                                          C.c_void_p, C.c_void_p, P(AnofoxError)]
    L.anofox_hip_device_count.restype = C.c_int
    L.anofox_hip_set_device.restype = C.c_int
    L.anofox_hip_set_device.argtypes = [C.c_int]
    L.anofox_hip_batch_create.restype = C.c_bool
    L.anofox_hip_batch_create.argtypes = [C.c_size_t, C.c_size_t, P(ForecastOptions), P(C.c_void_p), P(AnofoxError)]
    L.anofox_hip_batch_destroy.argtypes = [C.c_void_p]
    L.anofox_hip_batch_ld.restype = C.c_size_t
    L.anofox_hip_batch_ld.argtypes = [C.c_void_p]
    L.anofox_hip_batch_n_series.restype = C.c_size_t
    L.anofox_hip_batch_n_series.argtypes = [C.c_void_p]
    L.anofox_hip_batch_periods.restype = C.c_bool
    L.anofox_hip_batch_periods.argtypes = [C.c_void_p, C.c_void_p]
    L.anofox_hip_batch_set_fixed_params.restype = C.c_bool
    L.anofox_hip_batch_set_fixed_params.argtypes = [C.c_void_p, C.c_double, C.c_double, C.c_double, C.c_double, P(AnofoxError)]
    L.anofox_hip_batch_pack_host.restype = C.c_bool
    L.anofox_hip_batch_pack_host.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, P(AnofoxError)]
    L.anofox_hip_batch_set_device_block.restype = C.c_bool
    L.anofox_hip_batch_set_device_block.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, P(AnofoxError)]
    L.anofox_hip_batch_run.restype = C.c_bool
    L.anofox_hip_batch_run.argtypes = [C.c_void_p, C.c_void_p, P(AnofoxError)]
    L.anofox_hip_batch_stats.restype = C.c_bool
    L.anofox_hip_batch_stats.argtypes = [C.c_void_p, P(AnofoxHipStats)]
    L.anofox_hip_selftest_recip.restype = C.c_bool
    L.anofox_hip_selftest_recip.argtypes = [C.c_uint64, C.c_uint64, P(C.c_uint64), P(C.c_double)]
    L.anofox_hip_selftest_math.restype = C.c_bool
    L.anofox_hip_selftest_math.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_uint64, C.c_int, C.c_void_p, C.c_void_p, P(AnofoxError)]
    L.anofox_hip_batch_lane_stats.restype = C.c_bool
    L.anofox_hip_batch_lane_stats.argtypes = [C.c_void_p, P(AnofoxHipLaneStats), C.c_size_t]
    L.anofox_hip_batch_device_results.restype = C.c_bool
    L.anofox_hip_batch_device_results.argtypes = [C.c_void_p] + [P(C.c_void_p)] * 5
    L.anofox_hip_batch_fetch.restype = C.c_bool
    L.anofox_hip_batch_fetch.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    L.anofox_hip_model_name.argtypes = [P(ForecastOptions), C.c_int32, C.c_char * 64]
    L.anofox_hip_batch_model_name.argtypes = [C.c_void_p, C.c_size_t, C.c_int32, C.c_char * 64]
    L.anofox_hip_batch_model_name.restype = None
    L.anofox_hip_batch_inspect.restype = C.c_bool
    L.anofox_hip_batch_inspect.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, P(AnofoxError)]
    L.anofox_hip_batch_arima_fit.restype = C.c_bool
    L.anofox_hip_batch_arima_fit.argtypes = [C.c_void_p, C.c_void_p, P(AnofoxError)]
    L.anofox_hip_set_devices.restype = C.c_bool
    L.anofox_hip_set_devices.argtypes = [C.c_void_p, C.c_size_t]
    L.anofox_hip_get_devices.restype = C.c_size_t
    L.anofox_hip_get_devices.argtypes = [C.c_void_p, C.c_size_t]
    L.anofox_hip_set_min_series_per_device.argtypes = [C.c_size_t]
    L.anofox_hip_shard_range.argtypes = [C.c_size_t, C.c_size_t, C.c_size_t, P(C.c_size_t), P(C.c_size_t)]
    L.anofox_hip_set_default_arima_method.restype = C.c_bool
    L.anofox_hip_set_default_arima_method.argtypes = [C.c_int]
    L.anofox_hip_batch_set_arima_method.restype = C.c_bool
    L.anofox_hip_batch_set_arima_method.argtypes = [C.c_void_p, C.c_int, P(AnofoxError)]
    L.anofox_hip_release_caches.argtypes = []
    L.anofox_hip_batch_run_many.restype = C.c_bool
    L.anofox_hip_batch_run_many.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p]
    L.anofox_ts_mstl_decomposition.restype = C.c_bool
    L.anofox_ts_mstl_decomposition.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_int, P(MstlResult), P(AnofoxError)]
    L.anofox_free_mstl_result.argtypes = [P(MstlResult)]
    L.anofox_hip_mstl_decompose_batch.restype = C.c_bool
    L.anofox_hip_mstl_decompose_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_int,
                                                  C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, P(AnofoxError)]
    L.anofox_hip_mstl_decompose_device.restype = C.c_bool
    L.anofox_hip_mstl_decompose_device.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p, C.c_size_t,
                                                   C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, P(AnofoxError)]
    L.anofox_ts_forecast_exog.restype = C.c_bool
    L.anofox_ts_forecast_exog.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, P(ForecastOptionsExog), P(ForecastResult), P(AnofoxError)]
    L.anofox_ts_forecast_exog_batch.restype = C.c_bool
    L.anofox_ts_forecast_exog_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, P(ForecastOptions), C.c_size_t, C.c_void_p,
                                                C.c_void_p, C.c_void_p, C.c_void_p, P(AnofoxError), C.c_void_p, C.c_void_p]
    L.anofox_hip_batch_set_exog_device.restype = C.c_bool
    L.anofox_hip_batch_set_exog_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, P(AnofoxError)]
    L.anofox_hip_batch_exog_coefficients.restype = C.c_bool
    L.anofox_hip_batch_exog_coefficients.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, P(AnofoxError)]
    L.anofox_ts_detect_changepoints_bocpd.restype = C.c_bool
    L.anofox_ts_detect_changepoints_bocpd.argtypes = [C.c_void_p, C.c_size_t, C.c_double, C.c_bool, P(BocpdResult), P(AnofoxError)]
    L.anofox_free_bocpd_result.argtypes = [P(BocpdResult)]
    L.anofox_hip_changepoints_batch.restype = C.c_bool
    L.anofox_hip_changepoints_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_double, C.c_void_p, C.c_void_p,
                                                C.c_void_p, C.c_void_p, P(AnofoxError)]
    L.anofox_hip_changepoints_device.restype = C.c_bool
    L.anofox_hip_changepoints_device.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_size_t, C.c_double, C.c_void_p,
                                                 C.c_void_p, C.c_void_p, C.c_void_p, P(AnofoxError)]
    L.anofox_ts_detect_changepoints.restype = C.c_bool
    L.anofox_ts_detect_changepoints.argtypes = [C.c_void_p, C.c_size_t, C.c_int, C.c_double, P(ChangepointResult), P(AnofoxError)]
    L.anofox_free_changepoint_result.argtypes = [P(ChangepointResult)]
    L.anofox_hip_pelt_batch.restype = C.c_bool
    L.anofox_hip_pelt_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_double, C.c_void_p, C.c_void_p,
                                        C.c_void_p, C.c_void_p, P(AnofoxError)]
    L.anofox_hip_pelt_device.restype = C.c_bool
    L.anofox_hip_pelt_device.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_size_t, C.c_int, C.c_double, C.c_void_p,
                                         C.c_void_p, C.c_void_p, C.c_void_p, P(AnofoxError)]
    L.anofox_ts_stats.restype = C.c_bool
    L.anofox_ts_stats.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, P(TsStatsResult), P(AnofoxError)]
    L.anofox_ts_stats_with_dates.restype = C.c_bool
    L.anofox_ts_stats_with_dates.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int64, P(TsStatsResult), P(AnofoxError)]
    L.anofox_ts_stats_with_dates_and_type.restype = C.c_bool
    L.anofox_ts_stats_with_dates_and_type.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int64, C.c_int, P(TsStatsResult),
                                                      P(AnofoxError)]
    L.anofox_free_ts_stats_result.argtypes = [P(TsStatsResult)]
    L.anofox_hip_stats_batch.restype = C.c_bool
    L.anofox_hip_stats_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int64, C.c_int, C.c_void_p,
                                         P(AnofoxError)]
    L.anofox_hip_stats_device.restype = C.c_bool
    L.anofox_hip_stats_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_size_t, C.c_int64,
                                          C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, P(AnofoxError)]
    L.anofox_ts_data_quality.restype = C.c_bool
    L.anofox_ts_data_quality.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, P(DataQualityResult), P(AnofoxError)]
    L.anofox_hip_quality_batch.restype = C.c_bool
    L.anofox_hip_quality_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, P(AnofoxError)]
    L.anofox_ts_features.restype = C.c_bool
    L.anofox_ts_features.argtypes = [C.c_void_p, C.c_size_t, P(FeaturesResult), P(AnofoxError)]
    L.anofox_free_features_result.restype = None
    L.anofox_free_features_result.argtypes = [P(FeaturesResult)]
    L.anofox_ts_features_list.restype = C.c_bool
    L.anofox_ts_features_list.argtypes = [P(C.c_void_p), P(C.c_size_t)]
    L.anofox_ts_validate_feature_params.restype = C.c_bool
    L.anofox_ts_validate_feature_params.argtypes = [C.c_void_p, C.c_size_t, P(C.c_void_p), P(C.c_size_t)]
    L.anofox_free_warnings.restype = None
    L.anofox_free_warnings.argtypes = [C.c_void_p, C.c_size_t]
    L.anofox_hip_features_batch.restype = C.c_bool
    L.anofox_hip_features_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, P(AnofoxError)]
    L.anofox_hip_features_device.restype = C.c_bool
    L.anofox_hip_features_device.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p, C.c_void_p,
                                             C.c_void_p, P(AnofoxError)]
    L.anofox_hip_features_families_device.restype = C.c_bool
    L.anofox_hip_features_families_device.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_size_t, C.c_uint,
                                                      C.c_void_p, C.c_void_p, C.c_void_p, P(AnofoxError)]
    L.anofox_hip_quality_device.restype = C.c_bool
    L.anofox_hip_quality_device.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p, C.c_void_p,
                                            C.c_void_p, P(AnofoxError)]
    L.anofox_ts_detect_seasonality.restype = C.c_bool
    L.anofox_ts_detect_seasonality.argtypes = [C.c_void_p, C.c_size_t, C.c_int, P(P(C.c_int)), P(C.c_size_t), P(AnofoxError)]
    L.anofox_ts_analyze_seasonality.restype = C.c_bool
    L.anofox_ts_analyze_seasonality.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_int, P(SeasonalityResult), P(AnofoxError)]
    L.anofox_free_seasonality_result.restype = None
    L.anofox_free_seasonality_result.argtypes = [P(SeasonalityResult)]
    L.anofox_free_int_array.restype = None
    L.anofox_free_int_array.argtypes = [P(C.c_int)]
    L.anofox_hip_seasonality_batch.restype = C.c_bool
    L.anofox_hip_seasonality_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p, C.c_void_p, P(AnofoxError)]
    L.anofox_hip_seasonality_device.restype = C.c_bool
    L.anofox_hip_seasonality_device.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_size_t, C.c_int, C.c_void_p,
                                                C.c_void_p, C.c_void_p, P(AnofoxError)]
    L.anofox_ts_lomb_scargle.restype = C.c_bool
    L.anofox_ts_lomb_scargle.argtypes = [C.c_void_p, C.c_size_t, C.c_double, C.c_double, C.c_size_t, P(LombScargleResultFFI), P(AnofoxError)]
    L.anofox_ts_aic_period.restype = C.c_bool
    L.anofox_ts_aic_period.argtypes = [C.c_void_p, C.c_size_t, C.c_double, C.c_double, C.c_size_t, P(AicPeriodResultFFI), P(AnofoxError)]
    L.anofox_ts_sazed_period.restype = C.c_bool
    L.anofox_ts_sazed_period.argtypes = [C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t, C.c_size_t, P(SazedPeriodResultFFI), P(AnofoxError)]
    L.anofox_ts_detect_periods_flat.restype = C.c_bool
    L.anofox_ts_detect_periods_flat.argtypes = [C.c_void_p, C.c_size_t, C.c_char_p, C.c_size_t, C.c_double, C.c_void_p, C.c_size_t, C.c_double,
                                                P(FlatMultiPeriodResult), P(AnofoxError)]
    L.anofox_free_flat_multi_period_result.argtypes = [P(FlatMultiPeriodResult)]
    L.anofox_hip_periods_batch.restype = C.c_bool
    L.anofox_hip_periods_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_double, C.c_double, C.c_size_t, C.c_void_p,
                                           C.c_void_p, C.c_void_p, P(AnofoxError)]
    L.anofox_hip_periods_device.restype = C.c_bool
    L.anofox_hip_periods_device.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_size_t, C.c_int, C.c_double, C.c_double,
                                            C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, P(AnofoxError)]
    L.anofox_ts_ssa_period.restype = C.c_bool
    L.anofox_ts_ssa_period.argtypes = [C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t, P(SsaPeriodResultFFI), P(AnofoxError)]
    L.anofox_ts_stl_period.restype = C.c_bool
    L.anofox_ts_stl_period.argtypes = [C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t, C.c_size_t, P(StlPeriodResultFFI), P(AnofoxError)]
    L.anofox_hip_ssa_period_batch.restype = C.c_bool
    L.anofox_hip_ssa_period_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p,
                                              C.c_void_p, P(AnofoxError)]
    L.anofox_hip_stl_period_batch.restype = C.c_bool
    L.anofox_hip_stl_period_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t, C.c_size_t, C.c_void_p, C.c_void_p,
                                              C.c_void_p, C.c_void_p, C.c_void_p, P(AnofoxError)]
    L.anofox_hip_ssa_period_device.restype = C.c_bool
    L.anofox_hip_ssa_period_device.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t, C.c_size_t, C.c_int,
                                               C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, P(AnofoxError)]
    L.anofox_hip_stl_period_device.restype = C.c_bool
    L.anofox_hip_stl_period_device.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t, C.c_size_t, C.c_size_t,
                                               C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, P(AnofoxError)]
    L.anofox_ts_matrix_profile_period.restype = C.c_bool
    L.anofox_ts_matrix_profile_period.argtypes = [C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t, P(MatrixProfilePeriodResultFFI), P(AnofoxError)]
    L.anofox_hip_matrix_profile_batch.restype = C.c_bool
    L.anofox_hip_matrix_profile_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p,
                                                  C.c_void_p, P(AnofoxError)]
    L.anofox_hip_matrix_profile_device.restype = C.c_bool
    L.anofox_hip_matrix_profile_device.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t, C.c_size_t, C.c_void_p,
                                                   C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, P(AnofoxError)]
    for name in ("mae", "mse", "rmse", "mape", "smape", "r2", "bias"):
        f = getattr(L, "anofox_ts_" + name)
        f.restype = C.c_bool
        f.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, P(C.c_double), P(AnofoxError)]
    for name in ("rmae", "mase"):
        f = getattr(L, "anofox_ts_" + name)
        f.restype = C.c_bool
        f.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, P(C.c_double), P(AnofoxError)]
    L.anofox_ts_quantile_loss.restype = C.c_bool
    L.anofox_ts_quantile_loss.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_double, P(C.c_double), P(AnofoxError)]
    L.anofox_ts_mqloss.restype = C.c_bool
    L.anofox_ts_mqloss.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, P(C.c_double), P(AnofoxError)]
    L.anofox_ts_coverage.restype = C.c_bool
    L.anofox_ts_coverage.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, P(C.c_double), P(AnofoxError)]
    L.anofox_hip_metrics_batch.restype = C.c_bool
    L.anofox_hip_metrics_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t,
                                           C.c_void_p, C.c_size_t, C.c_uint32, C.c_double, C.c_bool, C.c_void_p, C.c_void_p, P(AnofoxError)]
    L.anofox_hip_metrics_device.restype = C.c_bool
    L.anofox_hip_metrics_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p,
                                            C.c_size_t, C.c_size_t, C.c_size_t, C.c_void_p, C.c_size_t, C.c_size_t, C.c_uint32, C.c_double,
                                            C.c_bool, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, P(AnofoxError)]
    L.anofox_ts_fill_nulls_const.restype = C.c_bool
    L.anofox_ts_fill_nulls_const.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_double, P(P(C.c_double)), P(AnofoxError)]
    for name in ("mean", "interpolate"):
        f = getattr(L, "anofox_ts_fill_nulls_" + name)
        f.restype = C.c_bool
        f.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, P(P(C.c_double)), P(AnofoxError)]
    for name in ("forward", "backward"):
        f = getattr(L, "anofox_ts_fill_nulls_" + name)
        f.restype = C.c_bool
        f.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, P(FilledValuesResult), P(AnofoxError)]
    L.anofox_ts_fill_gaps.restype = C.c_bool
    L.anofox_ts_fill_gaps.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int64, C.c_int, P(GapFillResult), P(AnofoxError)]
    L.anofox_free_gap_fill_result.argtypes = [P(GapFillResult)]
    L.anofox_free_filled_values_result.argtypes = [P(FilledValuesResult)]
    L.anofox_free_double_array.argtypes = [C.c_void_p]
    L.anofox_hip_prepare_device.restype = C.c_bool
    L.anofox_hip_prepare_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_size_t,
                                            P(AnofoxHipPrepOptions), C.c_size_t, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                            C.c_void_p, C.c_void_p, C.c_void_p, P(AnofoxError)]
    L.anofox_hip_prepare_batch.restype = C.c_bool
    L.anofox_hip_prepare_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, P(AnofoxHipPrepOptions), C.c_size_t,
                                           P(AnofoxHipPrepared), P(AnofoxError)]
    L.anofox_hip_free_prepared.argtypes = [P(AnofoxHipPrepared), C.c_size_t]
    L.anofox_hip_conformal_learn_device.restype = C.c_bool
    L.anofox_hip_conformal_learn_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p, C.c_size_t,
                                                    C.c_size_t, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p,
                                                    C.c_void_p, C.c_void_p, C.c_void_p, P(AnofoxError)]
    L.anofox_hip_conformal_apply_device.restype = C.c_bool
    L.anofox_hip_conformal_apply_device.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p,
                                                    C.c_void_p, C.c_size_t, C.c_size_t, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p,
                                                    C.c_void_p, P(AnofoxError)]
    L.anofox_hip_conformal_evaluate_device.restype = C.c_bool
    L.anofox_hip_conformal_evaluate_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p, C.c_size_t,
                                                       C.c_size_t, C.c_double, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, P(AnofoxError)]
    L.anofox_hip_conformal_batch.restype = C.c_bool
    L.anofox_hip_conformal_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p,
                                             C.c_size_t, C.c_int, C.c_int, C.c_bool, P(AnofoxHipConformal), C.c_void_p, P(AnofoxError)]
    L.anofox_hip_free_conformal.argtypes = [P(AnofoxHipConformal), C.c_size_t]
    L.anofox_ts_conformal_quantile.restype = C.c_bool
    L.anofox_ts_conformal_quantile.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_double, P(C.c_double), P(AnofoxError)]
    L.anofox_ts_conformal_intervals.restype = C.c_bool
    L.anofox_ts_conformal_intervals.argtypes = [C.c_void_p, C.c_size_t, C.c_double, P(P(C.c_double)), P(P(C.c_double)), P(AnofoxError)]
    for name in ("predict", "predict_asymmetric"):
        f = getattr(L, "anofox_ts_conformal_" + name)
        f.restype = C.c_bool
        f.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_double, P(ConformalResultFFI), P(AnofoxError)]
    L.anofox_ts_conformal_predict_multi.restype = C.c_bool
    L.anofox_ts_conformal_predict_multi.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t,
                                                    P(ConformalMultiResultFFI), P(AnofoxError)]
    L.anofox_ts_conformal_predict_adaptive.restype = C.c_bool
    L.anofox_ts_conformal_predict_adaptive.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_size_t, C.c_double,
                                                       P(ConformalResultFFI), P(AnofoxError)]
    L.anofox_ts_mean_interval_width.restype = C.c_bool
    L.anofox_ts_mean_interval_width.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, P(C.c_double), P(AnofoxError)]
    L.anofox_ts_conformal_learn.restype = C.c_bool
    L.anofox_ts_conformal_learn.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.c_void_p,
                                            P(CalibrationProfileFFI), P(AnofoxError)]
    L.anofox_ts_conformal_apply.restype = C.c_bool
    L.anofox_ts_conformal_apply.argtypes = [C.c_void_p, C.c_size_t, P(CalibrationProfileFFI), C.c_void_p, P(PredictionIntervalsFFI), P(AnofoxError)]
    L.anofox_ts_conformal_coverage.restype = C.c_bool
    L.anofox_ts_conformal_coverage.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, P(C.c_double), P(AnofoxError)]
    L.anofox_ts_conformal_evaluate.restype = C.c_bool
    L.anofox_ts_conformal_evaluate.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_double, P(ConformalEvaluationFFI), P(AnofoxError)]
    L.anofox_free_conformal_result.argtypes = [P(ConformalResultFFI)]
    L.anofox_free_conformal_multi_result.argtypes = [P(ConformalMultiResultFFI)]
    L.anofox_free_calibration_profile.argtypes = [P(CalibrationProfileFFI)]
    L.anofox_free_prediction_intervals.argtypes = [P(PredictionIntervalsFFI)]
    # block 5: the walk-forward backtest
    L.anofox_hip_backtest_folds.restype = C.c_size_t
    L.anofox_hip_backtest_folds.argtypes = [C.c_int64, C.c_int64, C.c_int64, C.c_int, C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.c_int64,
                                            C.c_bool, C.c_void_p, C.c_size_t]
    L.anofox_hip_backtest_sizes.restype = C.c_bool
    L.anofox_hip_backtest_sizes.argtypes = [C.c_void_p, C.c_size_t, C.c_size_t, P(C.c_size_t), P(C.c_size_t), P(C.c_size_t), P(AnofoxError)]
    L.anofox_hip_backtest_expand_device.restype = C.c_bool
    L.anofox_hip_backtest_expand_device.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p, C.c_size_t,
                                                    C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, P(AnofoxError)]
    L.anofox_hip_backtest_collect_device.restype = C.c_bool
    L.anofox_hip_backtest_collect_device.argtypes = [C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p,
                                                     C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_char_p, C.c_void_p,
                                                     C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, P(AnofoxError)]
    L.anofox_hip_backtest_batch.restype = C.c_bool
    L.anofox_hip_backtest_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, P(ForecastOptions), C.c_void_p, C.c_size_t, C.c_char_p,
                                            C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                            P(AnofoxError)]
    # block 6: aggregation up a key hierarchy
    L.anofox_hip_hierarchy_plan.restype = C.c_bool
    L.anofox_hip_hierarchy_plan.argtypes = [C.c_void_p, C.c_size_t, C.c_size_t, P(C.c_size_t), P(C.c_size_t), C.c_void_p, C.c_void_p,
                                            P(AnofoxError)]
    L.anofox_hip_hierarchy_device.restype = C.c_bool
    L.anofox_hip_hierarchy_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t,
                                              C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, P(AnofoxHipHierarchyOptions), C.c_size_t,
                                              C.c_size_t, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p,
                                              P(AnofoxError)]
    L.anofox_hip_hierarchy_batch.restype = C.c_bool
    L.anofox_hip_hierarchy_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t,
                                             P(AnofoxHipHierarchyOptions), C.c_size_t, C.c_size_t, C.c_size_t, C.c_void_p, C.c_void_p,
                                             C.c_void_p, C.c_void_p, P(C.c_size_t), P(C.c_size_t), P(C.c_size_t), P(AnofoxError)]
    # block 7: reconciliation
    L.anofox_hip_reconcile_plan.restype = C.c_bool
    L.anofox_hip_reconcile_plan.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, P(C.c_size_t), P(C.c_size_t), C.c_void_p, C.c_void_p,
                                            C.c_void_p, C.c_void_p, C.c_void_p, P(AnofoxError)]
    plan_args = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_size_t]
    L.anofox_hip_reconcile_factor_device.restype = C.c_bool
    L.anofox_hip_reconcile_factor_device.argtypes = plan_args + [C.c_int32, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, P(AnofoxError)]
    L.anofox_hip_reconcile_apply_device.restype = C.c_bool
    L.anofox_hip_reconcile_apply_device.argtypes = [C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t] + plan_args + \
        [C.c_int32, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, P(AnofoxError)]
    L.anofox_hip_reconcile_batch.restype = C.c_bool
    L.anofox_hip_reconcile_batch.argtypes = [C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p, C.c_size_t, C.c_int32, C.c_void_p, C.c_void_p,
                                             C.c_void_p, P(AnofoxError)]
    L.anofox_hip_reconcile_mint_sizes.restype = C.c_bool
    L.anofox_hip_reconcile_mint_sizes.argtypes = [C.c_size_t, C.c_size_t, C.c_size_t, P(C.c_size_t), P(C.c_size_t), P(C.c_size_t), P(C.c_size_t),
                                                  P(AnofoxError)]
    res_args = [C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t]            # the residual block: pointer, stride_s, stride_t, n_res
    L.anofox_hip_reconcile_mint_factor_device.restype = C.c_bool
    L.anofox_hip_reconcile_mint_factor_device.argtypes = res_args + plan_args + \
        [C.c_double, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, P(C.c_double), C.c_void_p, P(AnofoxError)]
    L.anofox_hip_reconcile_mint_apply_device.restype = C.c_bool
    L.anofox_hip_reconcile_mint_apply_device.argtypes = [C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t] + res_args + plan_args + \
        [C.c_void_p, C.c_void_p, C.c_size_t, C.c_double, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, P(AnofoxError)]
    L.anofox_hip_reconcile_mint_batch.restype = C.c_bool
    L.anofox_hip_reconcile_mint_batch.argtypes = [C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, P(C.c_double),
                                                  C.c_void_p, C.c_void_p, C.c_void_p, P(AnofoxError)]
    # block 8: the choice of a method per series
    L.anofox_hip_select_winner_device.restype = C.c_bool
    L.anofox_hip_select_winner_device.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_size_t, C.c_int32, C.c_void_p, C.c_void_p,
                                                  C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, P(AnofoxError)]
    L.anofox_hip_select_gather_device.restype = C.c_bool
    L.anofox_hip_select_gather_device.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p, C.c_size_t, C.c_size_t,
                                                  C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, P(AnofoxError)]
    L.anofox_hip_select_scatter_device.restype = C.c_bool
    L.anofox_hip_select_scatter_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t,
                                                   C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                   C.c_void_p, P(AnofoxError)]
    L.anofox_hip_select_combine_device.restype = C.c_bool
    L.anofox_hip_select_combine_device.argtypes = [C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p,
                                                   C.c_size_t, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, P(AnofoxError)]
    L.anofox_hip_select_batch.restype = C.c_bool
    L.anofox_hip_select_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_char_p, C.c_char_p,
                                          C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                          C.c_void_p, C.c_void_p, C.c_void_p, P(AnofoxError)]
    # block 9: bootstrap sample paths and their quantiles
    L.anofox_hip_paths_device.restype = C.c_bool
    L.anofox_hip_paths_device.argtypes = [C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p, C.c_size_t,
                                          C.c_size_t, C.c_size_t, C.c_size_t, P(AnofoxHipPathsOptions), C.c_size_t, C.c_void_p, C.c_size_t,
                                          C.c_void_p, C.c_void_p, P(AnofoxError)]
    L.anofox_hip_path_quantiles_device.restype = C.c_bool
    L.anofox_hip_path_quantiles_device.argtypes = [C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t, C.c_size_t, C.c_void_p, C.c_size_t,
                                                   C.c_void_p, C.c_void_p, C.c_void_p, P(AnofoxError)]
    L.anofox_hip_paths_batch.restype = C.c_bool
    L.anofox_hip_paths_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t, P(AnofoxHipPathsOptions),
                                         C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p, C.c_void_p,
                                         C.c_void_p, C.c_void_p, P(C.c_size_t), P(C.c_size_t), P(AnofoxError)]
    # block 10: scores of sample paths
    L.anofox_hip_path_scores_device.restype = C.c_bool
    L.anofox_hip_path_scores_device.argtypes = [C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t, C.c_size_t, C.c_void_p, C.c_size_t, C.c_size_t,
                                                C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t,
                                                C.c_void_p, C.c_void_p, P(AnofoxError)]
    L.anofox_hip_path_scores_sizes.restype = C.c_bool
    L.anofox_hip_path_scores_sizes.argtypes = [C.c_size_t, C.c_size_t, P(C.c_size_t), P(AnofoxError)]
    L.anofox_hip_path_energy_device.restype = C.c_bool
    L.anofox_hip_path_energy_device.argtypes = [C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t, C.c_size_t, C.c_size_t, C.c_void_p, C.c_size_t,
                                                C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, P(AnofoxError)]
    L.anofox_hip_path_scores_batch.restype = C.c_bool
    L.anofox_hip_path_scores_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t, P(AnofoxHipPathsOptions),
                                               C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p,
                                               C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                               P(C.c_size_t), P(C.c_size_t), P(AnofoxError)]
    # block 11: scaled, weighted scores of a hierarchy
    L.anofox_hip_scale_device.restype = C.c_bool
    L.anofox_hip_scale_device.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p, C.c_size_t, C.c_bool,
                                          C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, P(AnofoxError)]
    L.anofox_hip_weighted_scores_device.restype = C.c_bool
    L.anofox_hip_weighted_scores_device.argtypes = [C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p,
                                                    C.c_void_p, C.c_size_t, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                    C.c_void_p, C.c_void_p, P(AnofoxError)]
    L.anofox_hip_wrmsse_batch.restype = C.c_bool
    L.anofox_hip_wrmsse_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p,
                                          C.c_size_t, C.c_size_t, C.c_bool, C.c_size_t, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p,
                                          C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, P(C.c_size_t), P(C.c_size_t), P(AnofoxError)]
    # block 12: sample paths simulated from the fitted ETS models
    L.anofox_hip_batch_inspect_device.restype = C.c_bool
    L.anofox_hip_batch_inspect_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, P(AnofoxError)]
    L.anofox_hip_ets_innovations_device.restype = C.c_bool
    L.anofox_hip_ets_innovations_device.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t,
                                                    C.c_void_p, C.c_void_p, C.c_void_p, P(AnofoxError)]
    L.anofox_hip_ets_paths_device.restype = C.c_bool
    L.anofox_hip_ets_paths_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p, C.c_void_p, C.c_size_t,
                                              C.c_size_t, C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t, C.c_size_t,
                                              P(AnofoxHipEtsPathsOptions), C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p,
                                              C.c_void_p, P(AnofoxError)]
    L.anofox_hip_batch_ets_paths.restype = C.c_bool
    L.anofox_hip_batch_ets_paths.argtypes = [C.c_void_p, P(AnofoxHipEtsPathsOptions), C.c_size_t, C.c_size_t, C.c_void_p, C.c_size_t,
                                             C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, P(C.c_size_t),
                                             P(AnofoxError)]
    # block 13: sample paths simulated from the fitted AutoARIMA models
    L.anofox_hip_batch_arima_fit_device.restype = C.c_bool
    L.anofox_hip_batch_arima_fit_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, P(AnofoxError)]
    L.anofox_hip_arima_innovations_device.restype = C.c_bool
    L.anofox_hip_arima_innovations_device.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t,
                                                      C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, P(AnofoxError)]
    L.anofox_hip_arima_paths_device.restype = C.c_bool
    L.anofox_hip_arima_paths_device.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p,
                                                C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t, C.c_size_t, C.c_size_t,
                                                P(AnofoxHipArimaPathsOptions), C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p,
                                                C.c_void_p, P(AnofoxError)]
    L.anofox_hip_batch_arima_paths.restype = C.c_bool
    L.anofox_hip_batch_arima_paths.argtypes = [C.c_void_p, P(AnofoxHipArimaPathsOptions), C.c_size_t, C.c_size_t, C.c_void_p, C.c_size_t,
                                               C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, P(C.c_size_t),
                                               P(AnofoxError)]
    # block 4: columnar ingest (host side only; usable without a GPU up to pack_ingest)
    L.anofox_hip_ingest_create.restype = C.c_void_p
    L.anofox_hip_ingest_destroy.argtypes = [C.c_void_p]
    L.anofox_hip_ingest_append.restype = C.c_bool
    L.anofox_hip_ingest_append.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, P(AnofoxError)]
    L.anofox_hip_ingest_finish.restype = C.c_bool
    L.anofox_hip_ingest_finish.argtypes = [C.c_void_p, P(C.c_size_t), P(C.c_size_t), P(AnofoxError)]
    for fn, rt in (("group_keys", P(C.c_int64)), ("last_dates", P(C.c_int64)), ("lengths", P(C.c_size_t)),
                   ("values", P(P(C.c_double))), ("validity", P(P(C.c_uint64)))):
        f = getattr(L, "anofox_hip_ingest_" + fn)
        f.restype = rt
        f.argtypes = [C.c_void_p]
    L.anofox_hip_batch_pack_ingest.restype = C.c_bool
    L.anofox_hip_batch_pack_ingest.argtypes = [C.c_void_p, C.c_void_p, P(AnofoxError)]
    _lib = L
    return L


def make_options(model, horizon, *, ets_model="", seasonal_period=0, confidence_level=0.90, auto_detect=None,
                 include_fitted=False, include_residuals=False, window=0, model_pool="", seasonal_periods_str=""):
    """Option block as the reference binding fills it (src/scalar_functions/ts_forecast_scalar.cpp:439-468,
    src/table_functions/ts_forecast_native.cpp:612-645): memset 0, strncpy, defaults conf 0.90,
    auto_detect = (seasonal_period == 0 and no seasonal_periods)."""
    o = ForecastOptions()
    C.memset(C.byref(o), 0, C.sizeof(o))
    o.model = model.encode()[:31]
    o.ets_model = ets_model.encode()[:7]
    o.horizon = int(horizon)
    o.confidence_level = float(confidence_level)
    o.seasonal_period = int(seasonal_period)
    if auto_detect is None:
        auto_detect = (seasonal_period == 0 and not seasonal_periods_str)
    o.auto_detect_seasonality = bool(auto_detect)
    o.include_fitted = bool(include_fitted)
    o.include_residuals = bool(include_residuals)
    o.window = int(window)
    o.seasonal_periods_str = seasonal_periods_str.encode()[:63]
    o.model_pool = model_pool.encode()[:31]
    return o


def make_folds(folds):
    """AnofoxHipFold array from [(fold_id, train_start, train_end, test_start, test_end)] (api.backtest_fold_bounds) or from such an array."""
    if isinstance(folds, C.Array) and folds._type_ is AnofoxHipFold:
        return folds
    arr = (AnofoxHipFold * max(len(folds), 1))()
    for k, f in enumerate(folds):
        arr[k] = AnofoxHipFold(*[int(v) for v in f])
    return arr


def backtest_folds(n_dates, horizon, folds, window_type="expanding", min_train_size=1, gap=0, embargo=0, initial_train_size=-1,
                   skip_length=-1, clip_horizon=False):
    """anofox_hip_backtest_folds: the fold table as [(fold_id, train_start, train_end, test_start, test_end)] (host only, no device)."""
    L = load()
    code = BACKTEST_WINDOWS.get(window_type, 1) if isinstance(window_type, str) else int(window_type)
    args = (int(n_dates), int(horizon), int(folds), code, int(min_train_size), int(gap), int(embargo), int(initial_train_size),
            int(skip_length), bool(clip_horizon))
    n = L.anofox_hip_backtest_folds(*args, None, 0)
    arr = (AnofoxHipFold * max(n, 1))()
    L.anofox_hip_backtest_folds(*args, arr, n)
    return [(f.fold_id, f.train_start, f.train_end, f.test_start, f.test_end) for f in arr[:n]]


def backtest_sizes(folds, n_folds, n_series):
    """anofox_hip_backtest_sizes -> (t_train, n_pairs, ld_pairs)."""
    t, n, ld = C.c_size_t(), C.c_size_t(), C.c_size_t()
    err = AnofoxError()
    if not load().anofox_hip_backtest_sizes(folds, n_folds, n_series, C.byref(t), C.byref(n), C.byref(ld), C.byref(err)):
        raise ValueError(f"anofox_hip_backtest_sizes failed: [{err.code}] {err.message.decode()}")
    return t.value, n.value, ld.value


def make_options_table(methods):
    """A contiguous ForecastOptions array (the `methods` table of anofox_hip_select_batch) from a list of option blocks."""
    arr = (ForecastOptions * max(len(methods), 1))()
    for k, o in enumerate(methods):
        C.memmove(C.byref(arr[k]), C.byref(o), C.sizeof(ForecastOptions))
    return arr


def select_mode(mode):
    """The code of a selection mode given by name (SELECT_MODES) or by code."""
    if isinstance(mode, str):
        if mode not in SELECT_MODES:
            raise ValueError(f"unknown selection mode {mode!r}: one of {sorted(SELECT_MODES)}")
        return SELECT_MODES[mode]
    return int(mode)


def make_hierarchy_options(route="auto", tile_min_members=0):
    """AnofoxHipHierarchyOptions: route in HIERARCHY_ROUTES (or its code), tile_min_members 0 = the library's default."""
    o = AnofoxHipHierarchyOptions()
    o.route = HIERARCHY_ROUTES[route] if isinstance(route, str) else int(route)
    o.tile_min_members = int(tile_min_members)
    return o


def make_paths_options(mode="cumulative", joint=False, seed=0, route="auto"):
    """AnofoxHipPathsOptions: mode in PATHS_MODES and route in PATHS_ROUTES (or their codes; an unknown name raises ValueError, an
    unknown code is the library's to refuse), seed a uint64."""
    o = AnofoxHipPathsOptions()
    for name, value, table in (("mode", mode, PATHS_MODES), ("route", route, PATHS_ROUTES)):
        if isinstance(value, str):
            if value not in table:
                raise ValueError(f"unknown {name} {value!r}: one of {sorted(table)}")
            value = table[value]
        setattr(o, name, int(value))
    o.joint = int(joint)
    o.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    return o


def make_ets_paths_options(innovations="gaussian", joint=False, seed=0):
    """AnofoxHipEtsPathsOptions: innovations in ETS_PATHS_INNOVATIONS (or its code; an unknown name raises ValueError, an unknown code
    is the library's to refuse), seed a uint64."""
    o = AnofoxHipEtsPathsOptions()
    if isinstance(innovations, str):
        if innovations not in ETS_PATHS_INNOVATIONS:
            raise ValueError(f"unknown innovations {innovations!r}: one of {sorted(ETS_PATHS_INNOVATIONS)}")
        innovations = ETS_PATHS_INNOVATIONS[innovations]
    o.innovations = int(innovations)
    o.joint = int(joint)
    o.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    return o


def make_arima_paths_options(innovations="gaussian", joint=False, seed=0):
    """AnofoxHipArimaPathsOptions: innovations in ARIMA_PATHS_INNOVATIONS (or its code; an unknown name raises ValueError, an unknown
    code is the library's to refuse), seed a uint64."""
    o = AnofoxHipArimaPathsOptions()
    if isinstance(innovations, str):
        if innovations not in ARIMA_PATHS_INNOVATIONS:
            raise ValueError(f"unknown innovations {innovations!r}: one of {sorted(ARIMA_PATHS_INNOVATIONS)}")
        innovations = ARIMA_PATHS_INNOVATIONS[innovations]
    o.innovations = int(innovations)
    o.joint = int(joint)
    o.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    return o


def hierarchy_plan(column_of, n_series=None):
    """anofox_hip_hierarchy_plan: column_of int32 [n_groupings, n_series] (-1: none) -> (n_out, col_offsets int32 [n_out + 1], members
    int32 [nnz]), the members of a column ordered by (series, grouping).  Host only, no device."""
    import numpy as np
    co = np.ascontiguousarray(column_of, dtype=np.int32)
    if co.ndim == 1:
        co = co.reshape(1, -1) if n_series is None else co.reshape(-1, int(n_series))
    G, n = co.shape
    L = load()
    n_out, nnz = C.c_size_t(), C.c_size_t()
    err = AnofoxError()
    if not L.anofox_hip_hierarchy_plan(co.ctypes.data, G, n, C.byref(n_out), C.byref(nnz), None, None, C.byref(err)):
        raise ValueError(f"anofox_hip_hierarchy_plan failed: [{err.code}] {err.message.decode()}")
    offs = np.zeros(n_out.value + 1, dtype=np.int32)
    memb = np.zeros(max(nnz.value, 1), dtype=np.int32)
    if not L.anofox_hip_hierarchy_plan(co.ctypes.data, G, n, C.byref(n_out), C.byref(nnz), offs.ctypes.data, memb.ctypes.data, C.byref(err)):
        raise ValueError(f"anofox_hip_hierarchy_plan failed: [{err.code}] {err.message.decode()}")
    return n_out.value, offs, memb[:nnz.value]


def reconcile_method(method):
    """The code of a reconciliation method given by name (RECONCILE_METHODS) or by code."""
    if isinstance(method, str):
        if method not in RECONCILE_METHODS:
            raise ValueError(f"unknown reconciliation method {method!r}: one of {sorted(RECONCILE_METHODS)}")
        return RECONCILE_METHODS[method]
    return int(method)


def reconcile_mint_sizes(n_res, n_agg, n_rows):
    """anofox_hip_reconcile_mint_sizes: the element counts {"gram", "e", "factor", "work"} of the workspaces of the MinT-shrink device
    entries.  A size the entry refuses raises ValueError with its message."""
    L = load()
    vals = [C.c_size_t(0) for _ in range(4)]
    err = AnofoxError()
    if not L.anofox_hip_reconcile_mint_sizes(int(n_res), int(n_agg), int(n_rows), *[C.byref(v) for v in vals], C.byref(err)):
        raise ValueError(f"anofox_hip_reconcile_mint_sizes failed: [{err.code}] {err.message.decode()}")
    return dict(zip(("gram", "e", "factor", "work"), (int(v.value) for v in vals)))


def reconcile_plan(col_offsets, members, n_series):
    """anofox_hip_reconcile_plan on an aggregation plan (hierarchy_plan): {"bottom_col" int32 [n_series], "agg_cols" int32 [n_agg],
    "leaf_offsets" int32 [n_series + 1], "leaf_aggs" int32 [n_leaf], "struct_weights" fp64 [n_out], "n_agg", "n_leaf", "n_out", "nnz",
    "n_series", "col_offsets", "members"}.  Host only, no device; a plan the entry refuses raises ValueError with its message."""
    import numpy as np
    offs = np.ascontiguousarray(col_offsets, dtype=np.int32)
    memb = np.ascontiguousarray(members, dtype=np.int32)
    n_out, n = len(offs) - 1, int(n_series)
    L = load()
    n_agg, n_leaf, err = C.c_size_t(), C.c_size_t(), AnofoxError()
    mp = memb.ctypes.data if len(memb) else None
    if not L.anofox_hip_reconcile_plan(offs.ctypes.data, mp, n_out, n, C.byref(n_agg), C.byref(n_leaf), None, None, None, None, None, C.byref(err)):
        raise ValueError(f"anofox_hip_reconcile_plan failed: [{err.code}] {err.message.decode()}")
    bottom = np.zeros(max(n, 1), dtype=np.int32)
    aggs = np.zeros(max(n_agg.value, 1), dtype=np.int32)
    loffs = np.zeros(n + 1, dtype=np.int32)
    laggs = np.zeros(max(n_leaf.value, 1), dtype=np.int32)
    w = np.zeros(max(n_out, 1))
    if not L.anofox_hip_reconcile_plan(offs.ctypes.data, mp, n_out, n, C.byref(n_agg), C.byref(n_leaf), bottom.ctypes.data, aggs.ctypes.data,
                                       loffs.ctypes.data, laggs.ctypes.data, w.ctypes.data, C.byref(err)):
        raise ValueError(f"anofox_hip_reconcile_plan failed: [{err.code}] {err.message.decode()}")
    return {"bottom_col": bottom[:n], "agg_cols": aggs[:n_agg.value], "leaf_offsets": loffs, "leaf_aggs": laggs[:n_leaf.value],
            "struct_weights": w[:n_out], "n_agg": n_agg.value, "n_leaf": n_leaf.value, "n_out": n_out, "nnz": int(offs[n_out]) if n_out else 0,
            "n_series": n, "col_offsets": offs, "members": memb}


def make_prep_options(gaps=False, frequency_micros=0, frequency_type="FIXED", trim="none", fill="none", fill_value=0.0):
    """AnofoxHipPrepOptions from names: trim in PREP_TRIMS, fill in PREP_FILLS, frequency_type in FREQUENCY_TYPES."""
    o = AnofoxHipPrepOptions()
    o.gaps = 1 if gaps else 0
    o.frequency_type = FREQUENCY_TYPES[frequency_type]
    o.frequency_micros = int(frequency_micros)
    o.trim = PREP_TRIMS[trim]
    o.fill = PREP_FILLS[fill]
    o.fill_value = float(fill_value)
    return o


def make_options_exog(opts, exog=None):
    """ForecastOptionsExog with the fields of a ForecastOptions block and `exog` (a ctypes ExogenousData, kept alive by the caller)."""
    o = ForecastOptionsExog()
    C.memset(C.byref(o), 0, C.sizeof(o))
    for f, _ in ForecastOptions._fields_:
        setattr(o, f, getattr(opts, f))
    if exog is not None:
        o.exog = C.pointer(exog)
    return o


def set_devices(devices):
    """Devices the batch entry shards series ranges over (include/anofox_fcst_hip.h block 2); [] = the current device only."""
    L = load()
    arr = (C.c_int * len(devices))(*devices) if devices else None
    if not L.anofox_hip_set_devices(arr, len(devices)):
        raise ValueError(f"not visible devices: {devices!r}")


def shard_range(n_series, n_shards, shard):
    lo, hi = C.c_size_t(), C.c_size_t()
    load().anofox_hip_shard_range(n_series, n_shards, shard, C.byref(lo), C.byref(hi))
    return lo.value, hi.value


def feature_list():
    """anofox_ts_features_list: the 117 feature names in the order of the source's list_features (host only)."""
    L = load()
    names, count = C.c_void_p(), C.c_size_t()
    if not L.anofox_ts_features_list(C.byref(names), C.byref(count)):
        raise RuntimeError("anofox_ts_features_list failed")
    arr = C.cast(names, C.POINTER(C.c_char_p))
    out = [arr[i].decode() for i in range(count.value)]
    L.anofox_free_warnings(names, count.value)
    return out


def feature_names():
    """The 117 names in byte order: the order of anofox_ts_features, of out_features and of the presence bits."""
    return sorted(feature_list(), key=lambda s: s.encode())


def validate_feature_params(keys):
    """anofox_ts_validate_feature_params: one warning per key that is no feature name (host only)."""
    L = load()
    keys = [k.encode() for k in keys]
    arr = (C.c_char_p * max(len(keys), 1))(*keys)
    warnings, count = C.c_void_p(), C.c_size_t()
    if not L.anofox_ts_validate_feature_params(arr, len(keys), C.byref(warnings), C.byref(count)):
        raise RuntimeError("anofox_ts_validate_feature_params failed")
    w = C.cast(warnings, C.POINTER(C.c_char_p))
    out = [w[i].decode() for i in range(count.value)]
    L.anofox_free_warnings(warnings, count.value)
    return out
