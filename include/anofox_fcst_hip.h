/*
 * anofox_fcst_hip.h -- C ABI of the MI355X batch-forecasting backend.
 *
 * This is the drop-in boundary for the `ts_forecast_by` hot path of
 * DataZooDE/anofox-forecast.  The first block mirrors, byte for byte, the part
 * of the reference's cbindgen header that the path touches; the second block is
 * this backend's additive batch / device-resident interface.
 *
 * Reference interfaces replaced (file:line in /root/reference):
 *   ErrorCode            src/include/anofox_fcst_ffi.h:72-84
 *   AnofoxError          src/include/anofox_fcst_ffi.h:269-272
 *   ForecastOptions      src/include/anofox_fcst_ffi.h:1036-1095   (184 bytes)
 *   ForecastResult       src/include/anofox_fcst_ffi.h:1100-1145   (144 bytes)
 *   anofox_ts_forecast   src/include/anofox_fcst_ffi.h:2332-2337
 *                        (Rust body crates/anofox-fcst-ffi/src/lib.rs:3344-3550)
 *   anofox_free_forecast_result  anofox_fcst_ffi.h:2886 (lib.rs:5900-5930)
 *   anofox_fcst_version  anofox_fcst_ffi.h:3058
 *   ExogenousRegressor / ExogenousData / ForecastOptionsExog   anofox_fcst_ffi.h:1152-1249   (32 / 16 / 192 bytes)
 *   anofox_ts_forecast_exog      (Rust body crates/anofox-fcst-ffi/src/lib.rs:3580-3780)
 *
 * Plain C, SysV x86-64, no torch / HIP types in any signature: a device stream
 * is passed as an opaque `void *` (a hipStream_t), device buffers as `void *`.
 */
#ifndef ANOFOX_FCST_HIP_H
#define ANOFOX_FCST_HIP_H

#include <stdbool.h>
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------- */
/* Block 1: the reference's ABI for this path (layout-identical)              */
/* ------------------------------------------------------------------------- */

#ifndef ANOFOX_FCST_FFI_H /* the reference header defines the same names */

typedef enum ErrorCode {
    SUCCESS = 0,
    NULL_POINTER = 1,
    INVALID_INPUT = 2,
    COMPUTATION_ERROR = 3,
    ALLOCATION_ERROR = 4,
    INVALID_MODEL = 5,
    INSUFFICIENT_DATA = 6,
    INVALID_DATE_FORMAT = 7,
    INVALID_FREQUENCY = 8,
    PANIC_CAUGHT = 9,
    INTERNAL_ERROR = 10,
} ErrorCode;

typedef struct AnofoxError {
    enum ErrorCode code;
    char message[256]; /* NUL-terminated, truncated at 255 */
} AnofoxError;

typedef struct ForecastOptions {
    char model[32];                 /* method name, exact or alias            */
    char ets_model[8];              /* "AAA", "MNM", "AAdA"...; "" = no spec   */
    int horizon;
    double confidence_level;
    int seasonal_period;            /* 0 = not given                          */
    bool auto_detect_seasonality;
    bool include_fitted;
    bool include_residuals;
    int window;                     /* SMA window, 0 = default                */
    char seasonal_periods_str[64];  /* "[24, 168]"; multi-seasonal models only */
    char model_pool[32];            /* AutoETS pool; "" = complete            */
    char laplace_variant[16];       /* unused by this backend                 */
    bool laplace_seasonal_batch_init;
} ForecastOptions;

typedef struct ForecastResult {
    double *point_forecasts;        /* malloc'd, n_forecasts                  */
    double *lower_bounds;
    double *upper_bounds;
    double *fitted_values;          /* malloc'd, n_fitted, or NULL            */
    double *residuals;
    size_t n_forecasts;
    size_t n_fitted;
    char model_name[64];
    double aic;                     /* always NaN on this path                */
    double bic;
    double mse;                     /* NaN unless fitted values requested     */
} ForecastResult;

/*
 * Fit + forecast ONE series.  `values[length]` is sorted by date by the caller;
 * `validity` is a DuckDB bitmask (bit i%64 of word i/64, 1 = valid) or NULL.
 * Returns false and fills `out_error` (may be NULL) on failure; on success the
 * callee malloc()s the result arrays, released by anofox_free_forecast_result.
 * Runs on the GPU as a batch of one; there is no CPU fallback.
 */
bool anofox_ts_forecast(const double *values,
                        const uint64_t *validity,
                        size_t length,
                        const struct ForecastOptions *options,
                        struct ForecastResult *out_result,
                        struct AnofoxError *out_error);

void anofox_free_forecast_result(struct ForecastResult *result);

const char *anofox_fcst_version(void);

/*
 * MSTL decomposition result (layout of the reference's anofox_fcst_ffi.h).  The arrays are malloc()ed by the callee and
 * released by anofox_free_mstl_result; they are NULL when the decomposition was not applied.
 */
typedef struct MstlResult {
    double *trend;                 /* [n_observations] */
    double **seasonal_components;  /* [n_seasonal] arrays of n_observations */
    double *remainder;             /* [n_observations] */
    size_t n_observations;
    size_t n_seasonal;
    int *seasonal_periods;         /* [n_seasonal], longest first */
    bool decomposition_applied;
} MstlResult;

/*
 * MSTL decomposition of ONE series (the reference's moving-average MSTL: periods handled longest first, a period p is used
 * when p >= 2 and length >= 2p).  insufficient_data_mode: 0 = fail (COMPUTATION_ERROR when length < 2 * the smallest period),
 * 1 = trend only, 2 = not applied.  At most 8 periods (more: COMPUTATION_ERROR).  Runs on the GPU as a batch of one.
 */
bool anofox_ts_mstl_decomposition(const double *values,
                                  size_t length,
                                  const int *periods,
                                  size_t n_periods,
                                  int insufficient_data_mode,
                                  struct MstlResult *out_result,
                                  struct AnofoxError *out_error);

void anofox_free_mstl_result(struct MstlResult *result);

/*
 * Period detection (layouts of the reference's anofox_fcst_ffi.h: LombScargleResultFFI, AicPeriodResultFFI, SazedPeriodResultFFI and
 * FlatMultiPeriodResult, 64 / 72 / 56 / 120 bytes).  Only the three methods that the reference writes out in its own tree run here:
 * Lomb-Scargle, the AIC comparison of sinusoids, and SAZED.  The arrays of FlatMultiPeriodResult are malloc()ed by the callee
 * and released by anofox_free_flat_multi_period_result; they are NULL when n_periods is 0.
 */
typedef struct LombScargleResultFFI {
    double period;            /* 1 / frequency, NaN when no power exceeds zero */
    double frequency;
    double power;             /* normalised by the variance */
    double false_alarm_prob;
    char method[32];          /* "lomb_scargle" */
} LombScargleResultFFI;

typedef struct AicPeriodResultFFI {
    double period;
    double aic;
    double bic;
    double rss;
    double r_squared;
    char method[32];          /* "aic" */
} AicPeriodResultFFI;

typedef struct SazedPeriodResultFFI {
    double period;            /* NaN when the spectrum has no peak inside the period range */
    double power;
    double snr;
    char method[32];          /* "sazed" */
} SazedPeriodResultFFI;

typedef struct FlatMultiPeriodResult {
    double *period_values;
    double *confidence_values;
    double *strength_values;
    double *amplitude_values;
    double *phase_values;
    size_t *iteration_values;          /* 1-indexed */
    bool *matches_expected_values;
    double *matched_expected_values;   /* NaN: no match */
    double *match_deviation_values;    /* NaN: no match */
    size_t n_periods;
    double primary_period;             /* 0.0: nothing passed the confidence threshold */
    char method[32];
} FlatMultiPeriodResult;

/*
 * Period detection of ONE series, the reference's lomb_scargle / aic_comparison / sazed_period (periods.rs) behind its FFI
 * wrappers: an argument of zero (or below) means the source's default -- min_period 2, max_period (n - 1) / 2 (Lomb-Scargle),
 * n / 2 (AIC, SAZED), 1,000 frequencies, 50 candidates, zero_pad_factor 4.  NULL `values` or `out_result`: NULL_POINTER.  Fewer
 * than 4 / 8 / 16 observations: COMPUTATION_ERROR "Insufficient data: need at least 4 observations, got 3".  SAZED pads to the
 * next power of two of length * zero_pad_factor; a padded length above 16,777,216 fails with COMPUTATION_ERROR naming the limit.
 * Each runs on the GPU as a batch of one; the decisions (which frequency, candidate or bin) are the source's, the figures differ
 * from it by the rounding of sin / cos / ln / exp only.
 */
bool anofox_ts_lomb_scargle(const double *values,
                            size_t length,
                            double min_period,
                            double max_period,
                            size_t n_frequencies,
                            struct LombScargleResultFFI *out_result,
                            struct AnofoxError *out_error);

bool anofox_ts_aic_period(const double *values,
                          size_t length,
                          double min_period,
                          double max_period,
                          size_t n_candidates,
                          struct AicPeriodResultFFI *out_result,
                          struct AnofoxError *out_error);

bool anofox_ts_sazed_period(const double *values,
                            size_t length,
                            size_t min_period,
                            size_t max_period,
                            size_t zero_pad_factor,
                            struct SazedPeriodResultFFI *out_result,
                            struct AnofoxError *out_error);

/*
 * The reference's detect_periods_with_validation for ONE series.  `method` is parsed as its PeriodMethod::from_str does
 * (case-insensitive, aliases; NULL or an unknown string means "fft").  "lomb_scargle" / "lombscargle" / "lomb-scargle" / "ls",
 * "aic" / "aic_comparison" and "sazed" / "zero_padded" / "enhanced_dft" run with the source's defaults and give one period:
 * confidence = 1 - false_alarm_prob / r_squared / min(snr, 1), strength = power / r_squared / power, amplitude = phase = 0,
 * iteration = 1.  Every other method -- "fft" included, hence the default -- fails with INTERNAL_ERROR "... is not implemented
 * by the HIP backend".  max_period is accepted and, as in the source, ignored by these three methods.  min_confidence < 0 (or
 * NaN) means 0.3; 0 disables the filter; a period whose confidence is below the threshold (or NaN) is dropped, and when none
 * is left n_periods = 0, primary_period = 0.0 and the method reads "<method> (no seasonality)".  expected_periods (may be NULL)
 * marks a period that lies within `tolerance` (< 0 or NaN: 0.1) of an expected one, relative to the expected one.
 */
bool anofox_ts_detect_periods_flat(const double *values,
                                   size_t length,
                                   const char *method,
                                   size_t max_period,
                                   double min_confidence,
                                   const double *expected_periods,
                                   size_t n_expected,
                                   double tolerance,
                                   struct FlatMultiPeriodResult *out_result,
                                   struct AnofoxError *out_error);

void anofox_free_flat_multi_period_result(struct FlatMultiPeriodResult *result);

/*
 * Period detection by SSA and by STL strength (layouts of the reference's anofox_fcst_ffi.h: SsaPeriodResultFFI and
 * StlPeriodResultFFI, 56 bytes each; the eigenvalue and candidate vectors are dropped there, the batch and device entries return them).
 */
typedef struct SsaPeriodResultFFI {
    double period;            /* from the zero crossings of the first qualifying eigenvector; NaN when none qualifies */
    double variance_explained;
    size_t n_eigenvalues;
    char method[32];          /* "ssa" */
} SsaPeriodResultFFI;

typedef struct StlPeriodResultFFI {
    double period;            /* the candidate with the largest seasonal strength; NaN for a constant series */
    double seasonal_strength;
    double trend_strength;
    char method[32];          /* "stl" */
} StlPeriodResultFFI;

/*
 * ONE series through the reference's ssa_period / stl_period (periods.rs) behind its FFI wrappers: an argument of zero means the
 * source's default -- window_size n / 3 (then at most n / 2, at least 4), 10 components; min_period 4, max_period n / 3 (at most
 * n / 2), 20 candidates (at least 5).  NULL `values` or `out_result`: NULL_POINTER "Null pointer argument".  COMPUTATION_ERROR:
 * "Insufficient data: need at least 16 observations, got N", "Invalid input: min_period must be less than max_period", "Invalid
 * input: No valid candidate periods found", and an SSA window above 2,048 rows, naming that limit of this backend.  More than 32
 * components, more than 64 candidates or more than 65,536 observations: INVALID_INPUT naming the limit.  Each runs on the GPU as
 * a batch of one, and every figure equals the source's arithmetic bit for bit (sequential sums in index order, no fused
 * multiply-add), except for the sign of a zero result and NaN payloads.  The method dispatch by name (anofox_ts_detect_periods_flat
 * with "ssa" or "stl") keeps its not-implemented error.
 */
bool anofox_ts_ssa_period(const double *values,
                          size_t length,
                          size_t window_size,
                          size_t n_components,
                          struct SsaPeriodResultFFI *out_result,
                          struct AnofoxError *out_error);

bool anofox_ts_stl_period(const double *values,
                          size_t length,
                          size_t min_period,
                          size_t max_period,
                          size_t n_candidates,
                          struct StlPeriodResultFFI *out_result,
                          struct AnofoxError *out_error);

/*
 * Period detection by matrix profile (layout of the reference's anofox_fcst_ffi.h: MatrixProfilePeriodResultFFI, 64 bytes).
 */
typedef struct MatrixProfilePeriodResultFFI {
    double period;            /* the most frequent lag between a motif and its nearest neighbour; NaN when there is no motif */
    double confidence;        /* the share of the motifs that have this lag; 0.0 without motifs */
    size_t n_motifs;
    size_t subsequence_length;
    char method[32];          /* "matrix_profile" */
} MatrixProfilePeriodResultFFI;

/*
 * ONE series through the reference's matrix_profile_period (periods.rs) behind its FFI wrapper: an argument of zero means the
 * source's default -- subsequence_length m = n / 10 (then at least 4, at most n / 4), exclusion zone m / 4 (at least 1).  The
 * wrapper passes `n_best` on as the EXCLUSION ZONE; that is kept.  NULL `values` or `out_result`: NULL_POINTER "Null pointer
 * argument".  COMPUTATION_ERROR: "Insufficient data: need at least 32 observations, got N", and an effective subsequence length
 * above 2,048, naming that limit of this backend.  More than 65,536 observations: INVALID_INPUT naming the limit.  Runs on the GPU as
 * a batch of one.  confidence, n_motifs and subsequence_length equal the source's arithmetic bit for bit (every distance its own
 * sequential sum over k, no fused multiply-add, compared after the square root).  Where several lags share the highest count the
 * source returns one of them by the iteration order of a hash map; here the SMALLEST such lag is returned, always one of the
 * source's possible answers.  The method dispatch by name (anofox_ts_detect_periods_flat with "matrix_profile", "matrixprofile" or
 * "mp") keeps its not-implemented error.
 */
bool anofox_ts_matrix_profile_period(const double *values,
                                     size_t length,
                                     size_t subsequence_length,
                                     size_t n_best,
                                     struct MatrixProfilePeriodResultFFI *out_result,
                                     struct AnofoxError *out_error);

/*
 * Result of the Bayesian online changepoint detection (layout of the reference's anofox_fcst_ffi.h).  The arrays are malloc()ed
 * by the callee and released by anofox_free_bocpd_result; changepoint_indices is NULL when no point is flagged.
 */
typedef struct BocpdResult {
    bool *is_changepoint;            /* [n_points] */
    double *changepoint_probability; /* [n_points]; all zeros when include_probabilities is false */
    size_t n_points;
    size_t *changepoint_indices;     /* [n_changepoints] ascending, or NULL */
    size_t n_changepoints;
} BocpdResult;

/*
 * Bayesian online changepoint detection (BOCPD) of ONE series, the reference's detect_changepoints_bocpd: Normal-Gamma prior
 * mu0 = 0, kappa0 = alpha0 = beta0 = 0.01, constant hazard 1 / max(hazard_lambda, 1), Student-t predictive weights without their
 * normalising constant, at most 500 tracked run lengths.  changepoint_probability[t] is the normalised P(run length = 1) after
 * step t, is_changepoint[t] = probability > 0.5 && t > 0.  hazard_lambda <= 0 (or NaN) means 250.  NULL `values` or `out_result`:
 * NULL_POINTER; length < 3: COMPUTATION_ERROR "Insufficient data: need at least 3 observations, got N".  Non-finite values are
 * not special-cased, as in the reference: a NaN reaches the sums, the step's sum fails the `> 1e-300` test and the step stays
 * unnormalised, the probabilities from there on are NaN and a NaN is never flagged.  Runs on the GPU as a batch of one.
 */
bool anofox_ts_detect_changepoints_bocpd(const double *values,
                                         size_t length,
                                         double hazard_lambda,
                                         bool include_probabilities,
                                         struct BocpdResult *out_result,
                                         struct AnofoxError *out_error);

void anofox_free_bocpd_result(struct BocpdResult *result);

/*
 * Result of the PELT changepoint detection (layout of the reference's anofox_fcst_ffi.h).  `changepoints` is malloc()ed by the
 * callee and released by anofox_free_changepoint_result; it is NULL when there are none.
 */
typedef struct ChangepointResult {
    size_t *changepoints; /* [n_changepoints] ascending, or NULL */
    size_t n_changepoints;
    double cost;          /* f[n] of the recurrence; 0.0 for a series of fewer than 2 * min_size values */
} ChangepointResult;

/*
 * Changepoints of ONE series by the reference's detect_changepoints with the L2 cost ("PELT"; as written there it prunes nothing,
 * so it is the exact optimal partitioning): f[0] = -pen, f[t] = min over tau of (f[tau] + cost(tau, t)) + pen with
 * tau <= t - ms, tau == 0 or tau >= ms, cost = the sum of squared deviations of [tau, t) from its mean; the FIRST minimum in
 * ascending tau wins; the changepoints are the backtrack from n, `cost` is f[n].  ms = max(min_size, 1); a series of fewer than
 * 2 ms values has no changepoints and cost 0.0.  penalty > 0 is taken as given; anything else (0, negative, NaN) means
 * 2 ln(length).  The results equal the reference's BIT FOR BIT: every sum is its serial chain, no operation is fused.
 * Non-finite values are not special-cased: they follow the arithmetic (a NaN candidate is never the minimum; a step without a
 * finite candidate gets f = +inf).  NULL `values` or `out_result`: NULL_POINTER.  Runs on the GPU as a batch of one.
 */
bool anofox_ts_detect_changepoints(const double *values,
                                   size_t length,
                                   int min_size,
                                   double penalty,
                                   struct ChangepointResult *out_result,
                                   struct AnofoxError *out_error);

void anofox_free_changepoint_result(struct ChangepointResult *result);

/* How a frequency is counted in the date figures of the statistics (the reference's FrequencyType). */
typedef enum FrequencyType {
    FIXED = 0,     /* a fixed number of microseconds */
    MONTHLY = 1,   /* calendar months */
    QUARTERLY = 2, /* calendar quarters */
    YEARLY = 3     /* calendar years */
} FrequencyType;

/*
 * The 36 per-series figures of ts_stats (layout of the reference's anofox_fcst_ffi.h: sizeof == 296, n_zeros_start at 64, mean
 * at 96, expected_length at 272, has_date_metrics at 288).  Holds no pointer; anofox_free_ts_stats_result exists for symmetry.
 */
typedef struct TsStatsResult {
    size_t length, n_nulls, n_nan, n_zeros, n_positive, n_negative, n_unique_values;
    bool is_constant;
    size_t n_zeros_start, n_zeros_end, plateau_size, plateau_size_nonzero;
    double mean, median, std_dev, variance, min, max, range, sum, skewness, kurtosis, tail_index, bimodality_coef, trimmed_mean,
           coef_variation, q1, q3, iqr, autocorr_lag1, trend_strength, seasonality_strength, entropy, stability;
    size_t expected_length, n_gaps; /* 0 unless has_date_metrics */
    bool has_date_metrics;
} TsStatsResult;

/*
 * Statistics of ONE series, the reference's compute_ts_stats / compute_ts_stats_with_dates_and_type (stats.rs) behind its FFI
 * wrappers.  `validity` (bit i of word i / 64; NULL = all valid) marks NULLs; NULLs and NaNs are counted and dropped, every
 * other figure is computed on the remaining values in arrival order (infinities are ordinary values).  NULL `values`, `dates`
 * or `out_result`: NULL_POINTER.  length == 0: every count 0, every floating figure NaN, no date figures, and true.  A series
 * with no valid value: length, n_nulls, n_nan set, every other count 0 and every floating figure 0.0.  Date figures
 * (has_date_metrics): the dates are sorted inside the call; FIXED counts (last - first) / frequency_micros + 1 and a gap is a
 * step above (int64)(1.5 * frequency_micros), nothing is set when frequency_micros <= 0 and there are at least two dates; the
 * calendar types count month, quarter or year numbers of the UTC date.  anofox_ts_stats_with_dates is the FIXED rule.  Counts,
 * min, max, range, median, q1, q3, iqr are exact; the figures that are sums meet the reference within the data's own rounding
 * noise.  Each runs on the GPU as a batch of one.
 */
bool anofox_ts_stats(const double *values,
                     const uint64_t *validity,
                     size_t length,
                     struct TsStatsResult *out_result,
                     struct AnofoxError *out_error);

bool anofox_ts_stats_with_dates(const double *values,
                                const uint64_t *validity,
                                const int64_t *dates,
                                size_t length,
                                int64_t frequency_micros,
                                struct TsStatsResult *out_result,
                                struct AnofoxError *out_error);

bool anofox_ts_stats_with_dates_and_type(const double *values,
                                         const uint64_t *validity,
                                         const int64_t *dates,
                                         size_t length,
                                         int64_t frequency_micros,
                                         enum FrequencyType frequency_type,
                                         struct TsStatsResult *out_result,
                                         struct AnofoxError *out_error);

void anofox_free_ts_stats_result(struct TsStatsResult *result);

/*
 * The eight data quality figures of one series (layout of the reference's anofox_fcst_ffi.h: five doubles, two size_t and a bool,
 * sizeof == 64, n_gaps at 40, is_constant at 56).  Holds no pointer.
 */
typedef struct DataQualityResult {
    double structural_score, temporal_score, magnitude_score, behavioral_score, overall_score;
    size_t n_gaps;    /* always 0: the entry passes no dates, as the reference's */
    size_t n_missing; /* NULLs */
    bool is_constant;
} DataQualityResult;

/*
 * Data quality of ONE series, the reference's compute_data_quality(series, None) (quality.rs) behind its FFI wrapper.  `validity`
 * (bit i of word i / 64; NULL = all valid) marks NULLs.  With x the non-NULL values in row order and k their count: n_missing =
 * length - k, n_gaps = 0; is_constant: k < 2, or every |x_i - x_0| < DBL_EPSILON; structural = clamp(k / length * 0.7 +
 * min(k / 30, 1) * 0.3) (0 when k == 0); temporal = 1; magnitude = clamp(1 - 2 * outliers / k - 3 * extreme / k) with the outliers
 * beyond 1.5 interquartile ranges of sorted[(size_t)(k * 0.25)] and sorted[(size_t)(k * 0.75)] and the extremes beyond 4 population
 * deviations of the mean (0 when k == 0); behavioral = 0.5 when k < 3, 0 when the population variance is below DBL_EPSILON, 0.8
 * when the lag-1 autocorrelation exceeds 0.95 in magnitude, else 1; overall = the mean of the four.  length == 0: every figure 0,
 * is_constant false, and true.  Every sum runs left to right from 0.0 as the source's, so the figures equal the reference's bit
 * for bit.  +-inf are ordinary values.  A NaN among the valid values: false, COMPUTATION_ERROR "Invalid
 * input: a value is NaN" (the source leaves that answer to its sort's internals).  NULL `values` or `out_result`: NULL_POINTER.
 * Runs on the GPU as a batch of one.
 */
bool anofox_ts_data_quality(const double *values,
                            const uint64_t *validity,
                            size_t length,
                            struct DataQualityResult *out_result,
                            struct AnofoxError *out_error);

/*
 * Feature extraction result (layout of the reference's anofox_fcst_ffi.h: two pointers and a size_t, sizeof == 24).  `features`,
 * `feature_names` and every name are malloc'ed by the entry and released by anofox_free_features_result.
 */
typedef struct FeaturesResult {
    double *features;
    char **feature_names;
    size_t n_features;
} FeaturesResult;

#define ANOFOX_HIP_N_FEATURES 117
#define ANOFOX_HIP_FEATURES_MAX_ROWS 65536
#define ANOFOX_HIP_RECONCILE_MAX_AGG 16384      /* aggregate columns of a reconciliation plan: bounds the factor at 2 GiB */
#define ANOFOX_HIP_RECONCILE_MAX_RESIDUAL_ROWS 8192     /* residual rows of a MinT-shrink call: one n_res x n_res Gram plane is 512 MiB,
                                                           and the whole Gram workspace stays under 1 GiB for every n_res */

/*
 * The features of ONE series, the reference's extract_features (features.rs) behind its FFI wrapper: only the features the source
 * inserts (skewness and kurtosis need a deviation above DBL_EPSILON, the change features two values, a lag feature enough rows,
 * fft_coefficient_i a series longer than i), sorted by name in byte order.  Every sum runs left to right from 0.0 as the source's,
 * so counts, flags, locations, order statistics, sums and what one division or square root derives from them equal the reference's
 * bit for bit; the four entropies and lempel_ziv_complexity (ln) and the fft coefficients and spectral figures (sin / cos) agree to
 * a tolerance.  The source sums sum_of_reoccurring_values, sum_of_reoccurring_datapoints and the terms of
 * permutation_entropy in hash order; here the order is ascending over the distinct bit patterns (total order) and the lexicographic
 * order of the patterns.  length == 0: false, COMPUTATION_ERROR "Insufficient data: need at least 1 observations, got 0".  A NaN
 * among the values: false, COMPUTATION_ERROR "Invalid input: a value is NaN" (the source leaves its sorted figures to its sort's
 * internals).  More than 65,536 values: false, INVALID_INPUT, the text names the limit.  NULL `values` or `out_result`:
 * NULL_POINTER.  +-inf are ordinary values.  Runs on the GPU as a batch of one.
 */
bool anofox_ts_features(const double *values,
                        size_t length,
                        struct FeaturesResult *out_result,
                        struct AnofoxError *out_error);

void anofox_free_features_result(struct FeaturesResult *result);

/*
 * The 117 names in the order of the source's list_features.  As the reference's: *out_names receives a malloc'ed array of
 * *out_count malloc'ed strings (cast to char *); anofox_free_warnings(names, count) releases it.  Host only.
 */
bool anofox_ts_features_list(char **out_names, size_t *out_count);

/*
 * One warning "Unknown feature parameter key '<key>' - this parameter will be ignored" per key that is no feature name (NULL keys
 * are skipped).  *out_warnings is malloc'ed (NULL when there is none) and released by anofox_free_warnings.  false for a NULL
 * argument.  Host only.
 */
bool anofox_ts_validate_feature_params(const char *const *param_names,
                                       size_t n_params,
                                       char ***out_warnings,
                                       size_t *out_n_warnings);

void anofox_free_warnings(char **warnings, size_t n_warnings);

/*
 * Seasonality analysis of one series (layout of the reference's anofox_fcst_ffi.h: a pointer, a size_t, an int, two doubles; sizeof ==
 * 40, primary_period at 16, seasonal_strength at 24).  detected_periods is malloc'ed by the entry (NULL when n_periods == 0) and
 * released by anofox_free_seasonality_result.
 */
typedef struct SeasonalityResult {
    int *detected_periods;    /* strongest first, at most 5 */
    size_t n_periods;
    int primary_period;       /* detected_periods[0], or 0 */
    double seasonal_strength; /* the strength of the primary period, or 0 */
    double trend_strength;
} SeasonalityResult;

/*
 * Seasonal periods of ONE series, the reference's detect_seasonality (seasonality.rs).  With n = length, max_lag = min(max_period > 0
 * ? max_period : n / 2, n / 2), mean the sum of the values from 0.0 in order divided by n, d_i = x_i - mean, variance = sum d_i * d_i
 * and acf[lag] = (sum over i < n - lag of d_i * d_(i + lag)) / variance for lag = 1 .. max_lag, every sum sequential with multiply and
 * add separate: the periods are the lags 2 .. max_lag - 1 whose acf exceeds both neighbours and 0.1, ordered by acf descending (equal
 * values by ascending lag, as the source's stable sort leaves them), the first five.  max_lag < 2 or |variance| < DBL_EPSILON: none.
 * The periods are the reference's bit for bit.  *out_periods is malloc'ed (release with anofox_free_int_array),
 * NULL with *out_n_periods == 0 when there is none.  NULL `values`, `out_periods` or `out_n_periods`: NULL_POINTER.  length < 4:
 * COMPUTATION_ERROR "Insufficient data: need at least 4 observations, got N".  Non-finite values follow the arithmetic (no periods).
 * Runs on the GPU as a batch of one.
 */
bool anofox_ts_detect_seasonality(const double *values,
                                  size_t length,
                                  int max_period,
                                  int **out_periods,
                                  size_t *out_n_periods,
                                  struct AnofoxError *out_error);

/*
 * The reference's analyze_seasonality: the periods of anofox_ts_detect_seasonality; seasonal_strength = clamp(acf[primary], 0, 1) (0
 * without a period, and 0 when |variance| equals DBL_EPSILON exactly, as the source's second test is `>`); trend_strength =
 * clamp(sqrt(ss_xy^2 / (ss_xx * ss_yy)), 0, 1) of the regression on the row number, 0 when |ss_xx| or |ss_yy| < DBL_EPSILON, NaN
 * when the arithmetic gives NaN (non-finite values).  `timestamps` and `timestamps_len` are ignored, as the reference ignores them.
 * NULL `values` or `out_result`: NULL_POINTER.  length < 4: COMPUTATION_ERROR as above.  Runs on the GPU as a batch of one.
 */
bool anofox_ts_analyze_seasonality(const int64_t *timestamps,
                                   size_t timestamps_len,
                                   const double *values,
                                   size_t length,
                                   int max_period,
                                   struct SeasonalityResult *out_result,
                                   struct AnofoxError *out_error);

/* Frees detected_periods and clears it; NULL and zeroed structs are accepted. */
void anofox_free_seasonality_result(struct SeasonalityResult *result);

/* Frees an array returned by anofox_ts_detect_seasonality; NULL is accepted. */
void anofox_free_int_array(int *ptr);

/* Values with a validity bitmask (bit i of word i / 64), the reference's FilledValuesResult: sizeof == 24. */
typedef struct FilledValuesResult {
    double *values;
    uint64_t *validity;
    size_t length;
} FilledValuesResult;

/* Dates, values and validity after the gaps stage, the reference's GapFillResult: sizeof == 32. */
typedef struct GapFillResult {
    int64_t *dates;
    double *values;
    uint64_t *validity;
    size_t length;
} GapFillResult;

/*
 * The NULL fills of ONE series, the reference's imputation.rs behind its FFI wrappers.  `validity` (bit i of word i / 64; NULL =
 * all valid) marks NULLs.  const, mean and interpolate return *out_values, `length` doubles (malloc; anofox_free_double_array;
 * NULL for length 0): mean is the sum of the valid values in row order from 0.0 over their count, and NaN everywhere when there is
 * none; interpolate extends the edges with the first / last valid value, fills interior runs with prev + slope * j, slope =
 * (v - prev) / gap, and gives NaN everywhere when there is no valid value.  forward and backward keep leading / trailing NULLs:
 * they return values (NaN where NULL) with a validity bitmask (anofox_free_filled_values_result; both NULL for length 0).  NULL
 * `values` or output: NULL_POINTER "Null pointer argument".  Each runs on the GPU as a batch of one, through the kernels of
 * anofox_hip_prepare_device: the same bits.
 */
bool anofox_ts_fill_nulls_const(const double *values,
                                const uint64_t *validity,
                                size_t length,
                                double fill_value,
                                double **out_values,
                                struct AnofoxError *out_error);

bool anofox_ts_fill_nulls_mean(const double *values,
                               const uint64_t *validity,
                               size_t length,
                               double **out_values,
                               struct AnofoxError *out_error);

bool anofox_ts_fill_nulls_interpolate(const double *values,
                                      const uint64_t *validity,
                                      size_t length,
                                      double **out_values,
                                      struct AnofoxError *out_error);

bool anofox_ts_fill_nulls_forward(const double *values,
                                  const uint64_t *validity,
                                  size_t length,
                                  struct FilledValuesResult *out_result,
                                  struct AnofoxError *out_error);

bool anofox_ts_fill_nulls_backward(const double *values,
                                   const uint64_t *validity,
                                   size_t length,
                                   struct FilledValuesResult *out_result,
                                   struct AnofoxError *out_error);

/*
 * The gaps stage of ONE series (gaps.rs fill_gaps): the rows are stable-sorted by date, then for every pair of consecutive rows
 * FIXED inserts (d_i - d_prev) / frequency_micros - 1 NULL rows (truncating division) dated d_prev + step * frequency_micros,
 * and the calendar types insert one row per missing month, quarter or year, dated at the start of the previous row's period plus
 * `step` periods, 00:00:00 UTC.  Original rows keep their dates.  Inserted values are NaN with a clear validity bit.  FIXED with
 * frequency_micros <= 0: INVALID_FREQUENCY "Frequency must be positive for fixed intervals".  NULL dates, values or out_result:
 * NULL_POINTER.  length 0: all three arrays NULL.  A result above 16,777,216 rows: COMPUTATION_ERROR.
 */
bool anofox_ts_fill_gaps(const int64_t *dates,
                         const double *values,
                         const uint64_t *validity,
                         size_t length,
                         int64_t frequency_micros,
                         enum FrequencyType frequency_type,
                         struct GapFillResult *out_result,
                         struct AnofoxError *out_error);

void anofox_free_gap_fill_result(struct GapFillResult *result);
void anofox_free_filled_values_result(struct FilledValuesResult *result);
void anofox_free_double_array(double *ptr);

/* One exogenous regressor: `values[n_values]` aligned with the series, `future_values[n_future]` with the horizon. */
typedef struct ExogenousRegressor {
    const double *values;
    size_t n_values;                /* must equal the series' length          */
    const double *future_values;
    size_t n_future;                /* must equal the horizon                 */
} ExogenousRegressor;

typedef struct ExogenousData {
    const struct ExogenousRegressor *regressors;
    size_t n_regressors;            /* 0 = none                               */
} ExogenousData;

/* ForecastOptions with the regressors behind the three flags (the other fields as above). */
typedef struct ForecastOptionsExog {
    char model[32];
    char ets_model[8];
    int horizon;
    double confidence_level;
    int seasonal_period;
    bool auto_detect_seasonality;
    bool include_fitted;
    bool include_residuals;
    const struct ExogenousData *exog; /* NULL = no regressors                 */
    int window;
    char seasonal_periods_str[64];
    char model_pool[32];
    char laplace_variant[16];
    bool laplace_seasonal_batch_init;
} ForecastOptionsExog;

/*
 * Fit + forecast ONE series with exogenous regressors (forecast.rs forecast_with_exog).  Checks in the reference's order: NULL
 * pointers, the model name, every regressor's n_values against `length` and n_future against the horizon (INVALID_INPUT), then
 * the series' length.  With regressors, ARIMA and AutoARIMA run ARIMAX (model_name "ARIMAX"): least squares of y on the
 * regressors with an intercept, the ARIMA model's forecast of the residuals, plus intercept + sum beta_j future_j; an aliased
 * regressor (constant, duplicated, linearly dependent, or holding a non-finite value) is left out.  At most 8 regressors
 * (more: COMPUTATION_ERROR).  OptimizedTheta, DynamicTheta, MFLES and AutoMFLES with regressors (ThetaX, MFLESX) are
 * INTERNAL_ERROR: not implemented.  Without regressors, or with any other model, the call is anofox_ts_forecast on the series
 * (the regressors are ignored, as in the reference).  Intervals, fitted values, residuals and mse follow anofox_ts_forecast.
 * Runs on the GPU as a batch of one; results are released by anofox_free_forecast_result.
 */
bool anofox_ts_forecast_exog(const double *values,
                             const uint64_t *validity,
                             size_t length,
                             const struct ForecastOptionsExog *options,
                             struct ForecastResult *out_result,
                             struct AnofoxError *out_error);

#endif /* ANOFOX_FCST_FFI_H */

/* ------------------------------------------------------------------------- */
/* Block 2: batch entry (host buffers) -- additive, same per-series semantics */
/* ------------------------------------------------------------------------- */

/*
 * Fit + forecast `n_series` independent series with ONE shared option block in
 * one GPU pass.  Replaces the serial per-group loop of the reference binding
 * (src/table_functions/ts_forecast_native.cpp:586-740, one anofox_ts_forecast
 * call per group).  `horizons` may be NULL (= options->horizon for all) or give
 * a per-series horizon (cross-validation folds, ts_cv_forecast_native.cpp:676).
 * Per-series failures land in out_errors[i] with out_results[i] zeroed; the
 * return value is false only for batch-level failures (NULL pointers, no GPU).
 * INVALID_MODEL / INVALID_INPUT are uniform across the batch and are also
 * reported through `out_batch_error` (may be NULL).
 */
bool anofox_ts_forecast_batch(const double *const *values,
                              const uint64_t *const *validity,
                              const size_t *lengths,
                              size_t n_series,
                              const struct ForecastOptions *options,
                              const int *horizons,
                              struct ForecastResult *out_results,
                              struct AnofoxError *out_errors,
                              struct AnofoxError *out_batch_error);

/*
 * The batch form of anofox_ts_forecast_exog: `n_series` series, one shared option block and horizon, one shared number of
 * regressors K = n_regressors.  xreg[s * K + j] points at regressor j of series s (lengths[s] values), future_xreg[s * K + j] at
 * its options->horizon future values; regressors have no NULL masks (the reference has none: its callers pass 0.0).  Replaces the
 * per-group loop of the reference binding (src/table_functions/ts_forecast.cpp:245-337, one FFI call per group of
 * ts_forecast_exog_by).  K = 0, or a model that ignores regressors, forwards to anofox_ts_forecast_batch.  Per-series results
 * and errors and the batch error are those of anofox_ts_forecast_batch; more than 8 regressors, ThetaX and MFLESX fail the
 * whole call (false; the error is also written to every series that is long enough to be forecast).
 * out_coefficients (may be NULL): [n_series x (K + 1)] intercept, then beta_j (0.0 for a regressor that was left out; NaN for a
 * series that failed or did not take the ARIMAX path); out_used (may be NULL): [n_series] bit j = regressor j was used.
 * The ARIMAX path runs on the calling thread's current device (anofox_hip_set_devices does not shard it).
 */
bool anofox_ts_forecast_exog_batch(const double *const *values,
                                   const uint64_t *const *validity,
                                   const size_t *lengths,
                                   size_t n_series,
                                   const struct ForecastOptions *options,
                                   size_t n_regressors,
                                   const double *const *xreg,
                                   const double *const *future_xreg,
                                   struct ForecastResult *out_results,
                                   struct AnofoxError *out_errors,
                                   struct AnofoxError *out_batch_error,
                                   double *out_coefficients,
                                   uint32_t *out_used);

/*
 * MSTL decomposition of `n_series` series with one shared period list, in one GPU pass (same semantics as
 * anofox_ts_mstl_decomposition per series).  `validity` may be NULL; a NULL value counts as 0.0, as the reference's
 * ts_mstl_decomposition table function passes it.  With total = the sum of `lengths`, series i owns the range
 * [off_i, off_i + lengths[i]) of out_trend[total], out_remainder[total] and of each slot j of out_seasonal[n_periods * total]
 * (slot j = the j-th component the series got, longest period first); out_periods[i * n_periods + j] names the period of slot j
 * (0: unused slot, filled with NaN).  out_applied[i] = 1 when the decomposition was applied (trend and remainder written,
 * NaN otherwise).  Per-series failures (mode 0 and too short) land in out_errors[i] (may be NULL); the return value is false
 * only for batch-level failures (NULL pointers, more than 8 periods, no GPU), also reported through `out_batch_error`.
 */
bool anofox_hip_mstl_decompose_batch(const double *const *values,
                                     const uint64_t *const *validity,
                                     const size_t *lengths,
                                     size_t n_series,
                                     const int *periods,
                                     size_t n_periods,
                                     int insufficient_data_mode,
                                     double *out_trend,
                                     double *out_seasonal,
                                     double *out_remainder,
                                     int32_t *out_periods,
                                     int32_t *out_applied,
                                     struct AnofoxError *out_errors,
                                     struct AnofoxError *out_batch_error);

/*
 * The same on a device-resident time-major block: y[t * ld + s] (fp64, t < t_rows), lengths[n_series] (int32) and the outputs
 * are device pointers.  trend / remainder are [t_rows x ld], seasonal is [n_periods x t_rows x ld] with slot k = the k-th
 * period of the list sorted longest first (NaN where the series did not use it); info[s] = state << 8 | used, state 0 =
 * decomposed, 1 = trend only, 2 = not applied, 3 = failed (mode 0, too short), bit k of `used` = period k was used.  Rows
 * t >= lengths[s] are left untouched.  Runs on `stream` (NULL: the null stream) and returns after it has finished.
 */
bool anofox_hip_mstl_decompose_device(const double *y,
                                      size_t ld,
                                      const int32_t *lengths,
                                      size_t n_series,
                                      size_t t_rows,
                                      const int *periods,
                                      size_t n_periods,
                                      int insufficient_data_mode,
                                      double *trend,
                                      double *seasonal,
                                      double *remainder,
                                      int32_t *info,
                                      void *stream,
                                      struct AnofoxError *out_error);

/*
 * BOCPD of `n_series` series with one hazard_lambda, in one GPU pass (same semantics as anofox_ts_detect_changepoints_bocpd per
 * series, probabilities always included).  Replaces the single-threaded per-group loop of the reference's
 * _ts_detect_changepoints_by_native finalize.  `validity` may be NULL; a NULL value counts as 0.0, as that table function passes
 * it.  With total = the sum of `lengths`, series i owns [off_i, off_i + lengths[i]) of out_probability[total] and
 * out_is_changepoint[total] (0 / 1); out_n_changepoints[i] is its number of flagged points.  A series of fewer than 3 values
 * fails alone: out_errors[i] (may be NULL) gets the single entry's COMPUTATION_ERROR, out_n_changepoints[i] = -1, its
 * probabilities are NaN and its flags 0.  The return value is false only for batch-level failures (NULL pointers, no GPU), also
 * reported through `out_batch_error`.  Runs on the calling thread's current device (anofox_hip_set_devices does not shard it).
 */
bool anofox_hip_changepoints_batch(const double *const *values,
                                   const uint64_t *const *validity,
                                   const size_t *lengths,
                                   size_t n_series,
                                   double hazard_lambda,
                                   double *out_probability,
                                   uint8_t *out_is_changepoint,
                                   int32_t *out_n_changepoints,
                                   struct AnofoxError *out_errors,
                                   struct AnofoxError *out_batch_error);

/*
 * The same on a device-resident time-major block: y[t * ld + s] (fp64, t < t_rows), lengths[n_series] (int32) and the outputs
 * are device pointers.  probability (fp64) and flags (uint8) are [t_rows x ld], counts is [n_series] (int32).  Rows
 * t >= lengths[s] are left untouched; a series with lengths[s] < 3 gets counts[s] = -1 and is otherwise untouched; a length above
 * t_rows is cut to t_rows.  One wavefront per series, the run-length state in registers; the same bits on every run and through
 * every entry.  Runs on `stream` (NULL: the null stream) and returns after it has finished.
 */
bool anofox_hip_changepoints_device(const double *y,
                                    size_t ld,
                                    const int32_t *lengths,
                                    size_t n_series,
                                    size_t t_rows,
                                    double hazard_lambda,
                                    double *probability,
                                    uint8_t *flags,
                                    int32_t *counts,
                                    void *stream,
                                    struct AnofoxError *out_error);

/*
 * PELT of `n_series` series with one min_size and one penalty, in one GPU pass (per series the semantics and the bits of
 * anofox_ts_detect_changepoints; a default penalty is 2 ln of EACH series' own packed length).  `validity` may be NULL.  A NULL
 * value is DROPPED before the series is packed, as the reference's list scalar drops it (ExtractListAsDouble) -- unlike
 * anofox_hip_changepoints_batch, which counts it as 0.0 the way ITS table function does.  With total = the sum of `lengths`,
 * series i owns [off_i, off_i + lengths[i]) of out_flags[total] (0 / 1), indexed by position in the PACKED series: flag k of
 * series i is its k-th non-NULL value, and the positions a series lost to its NULLs, at the end of its range, are 0.
 * out_n_changepoints[i] and out_cost[i] are the count and f[n].  No series fails alone: out_errors[i] (may be NULL) is always
 * cleared.  At most 65,536 values per series.  The return value is false only for batch-level failures (NULL pointers, a series
 * too long, no GPU), also reported through `out_batch_error`.  Runs on the calling thread's current device
 * (anofox_hip_set_devices does not shard it).
 */
bool anofox_hip_pelt_batch(const double *const *values,
                           const uint64_t *const *validity,
                           const size_t *lengths,
                           size_t n_series,
                           int min_size,
                           double penalty,
                           uint8_t *out_flags,
                           int32_t *out_n_changepoints,
                           double *out_cost,
                           struct AnofoxError *out_errors,
                           struct AnofoxError *out_batch_error);

/*
 * The same on a device-resident time-major block: y[t * ld + s] (fp64, t < t_rows), lengths[n_series] (int32) and the outputs
 * are device pointers.  flags (uint8) is [t_rows x ld]: rows t < lengths[s] are written 0 / 1, rows t >= lengths[s] are left
 * untouched; counts (int32) and cost (fp64) are [n_series].  A length above t_rows is cut to t_rows; a series of fewer than
 * 2 * max(min_size, 1) rows gets count 0, cost 0.0 and zero flags; there is no per-series error.  t_rows <= 65,536.  One workgroup
 * per series: its arrays live in LDS up to 2,048 rows (the launch sizes the LDS from min(t_rows, 2,048)), in a global workspace
 * of the call beyond (28 bytes x (t_rows + 1) x min(n_series, 512), allocated whenever t_rows > 2,048, however few series are
 * that long: 29 MB at 2,049 rows, 940 MB at the row limit); the same bits either way, on every run and through every entry.  Runs on `stream` (NULL: the null stream)
 * and returns after it has finished.
 */
bool anofox_hip_pelt_device(const double *y,
                            size_t ld,
                            const int32_t *lengths,
                            size_t n_series,
                            size_t t_rows,
                            int min_size,
                            double penalty,
                            uint8_t *flags,
                            int32_t *counts,
                            double *cost,
                            void *stream,
                            struct AnofoxError *out_error);

/*
 * Statistics of `n_series` series in one GPU pass (per series the semantics of anofox_ts_stats_with_dates_and_type).  Replaces
 * the single-threaded per-group loop of the reference's _ts_stats_by_native finalize.  `validity` and `dates` may be NULL, and so
 * may validity[i] (all valid) and dates[i] (no date figures for series i).  out_results is TsStatsResult[n_series].  No
 * per-series failure exists; the return value is false only for batch-level failures (NULL pointers, no GPU), also reported
 * through `out_batch_error`.  Runs on the calling thread's current device (anofox_hip_set_devices does not shard it).
 */
bool anofox_hip_stats_batch(const double *const *values,
                            const uint64_t *const *validity,
                            const int64_t *const *dates,
                            const size_t *lengths,
                            size_t n_series,
                            int64_t frequency_micros,
                            enum FrequencyType frequency_type,
                            struct TsStatsResult *out_results,
                            struct AnofoxError *out_batch_error);

/*
 * The same on a device-resident time-major block: y[t * ld + s] (fp64, t < t_rows), lengths[n_series] (int32; a length above
 * t_rows is cut to it) and the outputs are device pointers.  `valid` (uint8 [t_rows x ld], 0 = NULL) and `dates` (int64
 * [t_rows x ld], microseconds) may be NULL.  out_int is int64 [14 x ld]: the 12 counts in struct order (is_constant as 0 / 1), then
 * expected_length and n_gaps (both -1 without date figures); out_fp is fp64 [22 x ld], mean to stability in struct order.
 * Columns s >= n_series are left untouched.  One wavefront per series: a series of at most 2,048 rows is sorted in LDS, a longer
 * one in a workspace in global memory that the call allocates (slower, the same figures).  The same bits on every run and
 * through every entry.  Runs on `stream` (NULL: the null stream) and returns after it has finished.
 */
bool anofox_hip_stats_device(const double *y,
                             const uint8_t *valid,
                             const int64_t *dates,
                             size_t ld,
                             const int32_t *lengths,
                             size_t n_series,
                             size_t t_rows,
                             int64_t frequency_micros,
                             enum FrequencyType frequency_type,
                             int64_t *out_int,
                             double *out_fp,
                             void *stream,
                             struct AnofoxError *out_error);

/*
 * Data quality of `n_series` series in one GPU pass (per series the semantics of anofox_ts_data_quality).  Replaces the reference's
 * one FFI call per group.  `validity` may be NULL, and so may validity[i] (all valid).  out_results is DataQualityResult[n_series],
 * out_status int32[n_series] (may be NULL): 0, or 2 for a series with a NaN among its valid values -- its five scores are NaN, its
 * n_missing, n_gaps and is_constant are set.  No other per-series failure exists; the return value is false only for batch-level
 * failures (NULL pointers, no GPU), also reported through `out_batch_error`.  Runs on the calling thread's current device
 * (anofox_hip_set_devices does not shard it).
 */
bool anofox_hip_quality_batch(const double *const *values,
                              const uint64_t *const *validity,
                              const size_t *lengths,
                              size_t n_series,
                              struct DataQualityResult *out_results,
                              int32_t *out_status,
                              struct AnofoxError *out_batch_error);

/*
 * The same on a device-resident time-major block, e.g. the output of anofox_hip_prepare_device: y[t * ld + s] (fp64, t < t_rows),
 * `valid` (uint8 [t_rows x ld], 0 = NULL; may be NULL), lengths[n_series] (int32; a length above t_rows is cut to it); the outputs
 * are device pointers.  out_fp is fp64 [5 x ld], the scores in struct order; out_int is int64 [4 x ld]: n_gaps, n_missing,
 * is_constant as 0 / 1, status (0 or 2).  Columns s >= n_series are left untouched.  One wavefront per series: a series of at most
 * 2,048 rows is sorted in LDS, a longer one in a workspace in global memory that the call allocates (slower, the same figures).
 * The same bits on every run and through every entry.  Runs on `stream` (NULL: the null stream) and returns after it has finished.
 */
bool anofox_hip_quality_device(const double *y,
                               const uint8_t *valid,
                               size_t ld,
                               const int32_t *lengths,
                               size_t n_series,
                               size_t t_rows,
                               double *out_fp,
                               int64_t *out_int,
                               void *stream,
                               struct AnofoxError *out_error);

/*
 * The features of `n_series` series in one GPU pass (per series the semantics of anofox_ts_features).  Replaces the reference's one
 * FFI call per group (_ts_features_native).  `validity` may be NULL, and so may validity[i] (all valid); NULL values are dropped.
 * out_features is fp64 [n_series x 117], series-major, the features in byte order of their names (the order of the single entry;
 * feature_names.inc); a feature the source does not insert is NaN there and its bit in out_present (uint64 [n_series x 2], bit
 * i % 64 of word i / 64 for feature i) is 0.  out_status is int32 [n_series] (may be NULL): 0; 1 for a series without a value
 * (every feature NaN, no bit); 2 for a series with a NaN among its values (`length` is written and is its only bit, every other
 * feature is NaN).  The return value is false only for batch-level failures (NULL pointers, no GPU, a series above 65,536 values),
 * also reported through `out_batch_error`.  Runs on the calling thread's current device.
 */
bool anofox_hip_features_batch(const double *const *values,
                               const uint64_t *const *validity,
                               const size_t *lengths,
                               size_t n_series,
                               double *out_features,
                               uint64_t *out_present,
                               int32_t *out_status,
                               struct AnofoxError *out_batch_error);

/*
 * The same on a device-resident time-major block: y[t * ld + s] (fp64, t < t_rows <= 65,536), `valid` (uint8 [t_rows x ld], 0 =
 * NULL; may be NULL), lengths[n_series] (int32; a length above t_rows is cut to it); the outputs are device pointers.  out_fp is
 * fp64 [117 x ld], row i the feature i; out_int is int64 [3 x ld]: the two presence words and the status.  Columns s >= n_series
 * are left untouched.  Five kernels, one per family (in-order chains, sort, counting scans, template matching, DFT), one wavefront
 * per series: a series of at most 2,048 rows lives in LDS, a longer one in a workspace in global memory that the call allocates
 * (slower, the same figures).  The same bits on every run and through every entry.  Runs on `stream` (NULL: the null stream) and
 * returns after it has finished.
 */
bool anofox_hip_features_device(const double *y,
                                const uint8_t *valid,
                                size_t ld,
                                const int32_t *lengths,
                                size_t n_series,
                                size_t t_rows,
                                double *out_fp,
                                int64_t *out_int,
                                void *stream,
                                struct AnofoxError *out_error);

/*
 * anofox_hip_features_device restricted to the families whose bit is set in `families` (bit 0 chains -- it writes out_int --, 1 sort,
 * 2 counting scans, 3 template matching, 4 DFT): the rows of the other families are left untouched.  For tests and timing.
 */
bool anofox_hip_features_families_device(const double *y,
                                         const uint8_t *valid,
                                         size_t ld,
                                         const int32_t *lengths,
                                         size_t n_series,
                                         size_t t_rows,
                                         unsigned families,
                                         double *out_fp,
                                         int64_t *out_int,
                                         void *stream,
                                         struct AnofoxError *out_error);

/*
 * The seasonality analysis of one series of a batch: sizeof == 128, no pointer.  Entries k >= n_periods of the arrays are 0.
 */
typedef struct AnofoxHipSeasonality {
    int32_t periods[5];       /* strongest first */
    int32_t n_periods;
    int32_t primary_period;   /* periods[0], or 0 */
    int32_t reserved;
    double strengths[5];      /* clamp(acf, 0, 1) of each period */
    double acf[5];            /* the autocorrelation at each period as computed */
    double seasonal_strength; /* strengths[0], or 0 */
    double trend_strength;
} AnofoxHipSeasonality;

/*
 * Seasonality analysis of `n_series` series in one GPU pass (per series the semantics of anofox_ts_analyze_seasonality, with all five
 * strengths).  Replaces the reference's one FFI call per series.  `validity` may be NULL, and so may validity[i] (all valid); a NULL
 * value is dropped, as the SQL scalars drop NULL list elements, so n is the count of valid values.  One `max_period` for the batch (<=
 * 0: n / 2 of each series).  out_results is AnofoxHipSeasonality[n_series], out_status int32[n_series] (may be NULL): 0, or 1 for a
 * series of fewer than 4 valid values, whose record is all zero.  No other per-series failure exists; the return value is false only
 * for batch-level failures (NULL pointers, no GPU), also reported through `out_batch_error`.  Runs on the calling thread's current
 * device (anofox_hip_set_devices does not shard it).
 */
bool anofox_hip_seasonality_batch(const double *const *values,
                                  const uint64_t *const *validity,
                                  const size_t *lengths,
                                  size_t n_series,
                                  int max_period,
                                  struct AnofoxHipSeasonality *out_results,
                                  int32_t *out_status,
                                  struct AnofoxError *out_batch_error);

/*
 * The same on a device-resident time-major block: y[t * ld + s] (fp64, t < t_rows), `valid` (uint8 [t_rows x ld], 0 = NULL; may be
 * NULL), lengths[n_series] (int32; a length above t_rows is cut to it); the outputs are device pointers.  out_int is int32 [8 x ld]:
 * periods[0..4] (0 beyond n_periods), n_periods, primary_period, status (0 or 1).  out_fp is fp64 [12 x ld]: strengths[0..4] (0.0
 * beyond n_periods), the five autocorrelation values as computed, seasonal_strength, trend_strength.  Columns s >= n_series are left
 * untouched.  One workgroup per series; a block of at most 5,120 rows is worked on in LDS, a higher one in a workspace in global
 * memory that the call allocates (slower, the same figures).  The same bits on every run and through every entry.  Runs on `stream`
 * (NULL: the null stream) and returns after it has finished.
 */
bool anofox_hip_seasonality_device(const double *y,
                                   const uint8_t *valid,
                                   size_t ld,
                                   const int32_t *lengths,
                                   size_t n_series,
                                   size_t t_rows,
                                   int max_period,
                                   int32_t *out_int,
                                   double *out_fp,
                                   void *stream,
                                   struct AnofoxError *out_error);

/* What anofox_hip_prepare_device / _batch run, in this fixed order: gaps, trim, fill.  Zero everywhere is "copy the rows". */
typedef struct AnofoxHipPrepOptions {
    int32_t gaps;             /* 1: the gaps stage of anofox_ts_fill_gaps runs (needs dates) */
    int32_t frequency_type;   /* FrequencyType of the gaps stage */
    int64_t frequency_micros; /* FIXED: > 0 */
    int32_t trim;             /* 0 none, 1 leading, 2 trailing, 3 edge: the ts_drop_*_zeros_by macros.  A row is non-zero when it
                                 is valid and y != 0 (-0.0 is a zero, NaN is non-zero, a NULL is not non-zero) */
    int32_t fill;             /* 0 none, 1 const, 2 forward, 3 backward, 4 mean, 5 interpolate: anofox_ts_fill_nulls_* */
    double fill_value;        /* const */
} AnofoxHipPrepOptions;

/*
 * Prepares every series of a device-resident time-major block for anofox_hip_batch_set_device_block without a host round trip.
 * Layout as anofox_hip_stats_device: y[t * ld + s] (fp64, t < t_rows), `valid` (uint8 [t_rows x ld], 0 = NULL; NULL pointer: all
 * valid), `dates` (int64 [t_rows x ld], microseconds; may be NULL unless options->gaps, then INVALID_INPUT), lengths[n_series]
 * (int32; cut to t_rows).  struct_size is sizeof(AnofoxHipPrepOptions) (anything else: INVALID_INPUT).  The entry does NOT sort: the
 * gaps stage walks the rows as they lie (descending or duplicate dates insert nothing).  Outputs: y_out, valid_out (may be NULL),
 * dates_out (may be NULL; written only when `dates` is given) are [t_out x ld] blocks, len_out is int32 [n_series]; a NULL output
 * row holds NaN and valid 0; output rows start at row 0 (dates move with their rows).  Outputs must not overlap inputs
 * (INVALID_INPUT).  Columns s >= n_series and rows >= len_out[s] are left untouched.
 *
 * out_int is int64 [8 x ld]: input rows, input NULLs, rows inserted by the gaps stage, rows trimmed at the front, rows trimmed
 * at the back, output NULLs, output rows that are valid and != 0, status.  out_fp is fp64 [2 x ld]: min and max of the valid
 * output values, NaN ranking above every number (both NaN without a valid value).  A series with no non-zero row is trimmed to
 * length 0 (counted at the front, for trailing-only at the back).  status 1: the result needs more than t_out rows; len_out[s] = 0,
 * nothing written, the counts hold (input rows + inserted - trimmed is the need), the output figures are 0 / NaN, and the
 * neighbours are unaffected.  status 2: more than 16,777,216 rows after the gaps stage; as status 1, in count mode too (the
 * inserted count saturates at 2^40).  y_out == NULL is count mode: len_out and all figures, no blocks; it sizes t_out.
 *
 * One lane per series, two sweeps (dataprep.hip); the same bits on every run and through every entry.  Runs on `stream` (NULL:
 * the null stream) on the calling thread's current device and returns after it has finished.
 */
bool anofox_hip_prepare_device(const double *y,
                               const uint8_t *valid,
                               const int64_t *dates,
                               size_t ld,
                               const int32_t *lengths,
                               size_t n_series,
                               size_t t_rows,
                               const AnofoxHipPrepOptions *options,
                               size_t struct_size,
                               size_t t_out,
                               double *y_out,
                               uint8_t *valid_out,
                               int64_t *dates_out,
                               int32_t *len_out,
                               int64_t *out_int,
                               double *out_fp,
                               void *stream,
                               struct AnofoxError *out_error);

/* One prepared series of anofox_hip_prepare_batch: malloc'd arrays (NULL for length 0; dates NULL when none were given). */
typedef struct AnofoxHipPrepared {
    int64_t *dates;
    double *values;
    uint64_t *validity;
    size_t length;
    int64_t figures[8];       /* out_int of anofox_hip_prepare_device */
    double min, max;
} AnofoxHipPrepared;

/*
 * The same for host series, in one pass (a count call sizes the output block).  `validity` and `dates` may be NULL, and so may
 * validity[i]; dates[i] must be given for every series or for none (INVALID_INPUT), and must be given when options->gaps.  With
 * dates, every series is stable-sorted by date first, as fill_gaps does.  out_results is AnofoxHipPrepared[n_series], released by
 * anofox_hip_free_prepared.  A series above the row limit gets status 2 and length 0.  Replaces the per-group loop of the
 * reference's _ts_fill_gaps_native finalize.  The return value is false only for batch-level failures, also reported through
 * `out_batch_error`.
 */
bool anofox_hip_prepare_batch(const double *const *values,
                              const uint64_t *const *validity,
                              const int64_t *const *dates,
                              const size_t *lengths,
                              size_t n_series,
                              const AnofoxHipPrepOptions *options,
                              size_t struct_size,
                              AnofoxHipPrepared *out_results,
                              struct AnofoxError *out_batch_error);

void anofox_hip_free_prepared(AnofoxHipPrepared *results, size_t n_series);

/*
 * Period detection of `n_series` series with ONE method and one parameter set, in one GPU pass.  Replaces the per-group calls of
 * the reference's ts_detect_periods_by.  method: 0 Lomb-Scargle, 1 AIC, 2 SAZED (anything else: INVALID_INPUT).  min_period /
 * max_period are doubles for all three (SAZED's are truncated to integers); n_grid is n_frequencies, n_candidates or
 * zero_pad_factor; zero or below means the source's default, as in the single entries.  out_figures is fp64 [5 x n_series],
 * figure j of series i at out_figures[j * n_series + i]: Lomb-Scargle period, frequency, power, false_alarm_prob; AIC period,
 * aic, bic, rss, r_squared; SAZED period, power, snr (unused rows are NaN).  out_index[i] (int32, may be NULL) is the selected
 * frequency, candidate or DFT bin, -1 when none.  A series that is too short (4 / 8 / 16) or whose SAZED padding exceeds
 * 16,777,216 fails alone: out_errors[i] (may be NULL) gets the single entry's COMPUTATION_ERROR and its figures are NaN.  The
 * return value is false only for batch-level failures, also reported through `out_batch_error`.  Runs on the calling thread's
 * current device (anofox_hip_set_devices does not shard it).
 */
bool anofox_hip_periods_batch(const double *const *values,
                              const size_t *lengths,
                              size_t n_series,
                              int method,
                              double min_period,
                              double max_period,
                              size_t n_grid,
                              double *out_figures,
                              int32_t *out_index,
                              struct AnofoxError *out_errors,
                              struct AnofoxError *out_batch_error);

/*
 * The same on a device-resident time-major block: y[t * ld + s] (fp64, t < t_rows), lengths[n_series] (int32; a length above
 * t_rows is cut to it) and the outputs are device pointers.  figures is fp64 [5 x ld] (figure j of series s at j * ld + s), index
 * and status are int32 [n_series]; status is 0 (done), 1 (too short) or 2 (SAZED padding above the limit), and nothing else is
 * written for a series whose status is not 0.  One wavefront per series, the series staged in LDS 2,048 rows at a time.  SAZED
 * keeps a spectrum of up to 4,096 bins in LDS; for longer ones the call allocates a workspace of at most 256 MiB, whatever
 * n_series is, and walks the batch in chunks.  The same bits on every run and through every entry.  Runs on `stream` (NULL: the
 * null stream) and returns after it has finished.
 */
bool anofox_hip_periods_device(const double *y,
                               size_t ld,
                               const int32_t *lengths,
                               size_t n_series,
                               size_t t_rows,
                               int method,
                               double min_period,
                               double max_period,
                               size_t n_grid,
                               double *figures,
                               int32_t *index,
                               int32_t *status,
                               void *stream,
                               struct AnofoxError *out_error);

/*
 * SSA and STL period detection of `n_series` series with one parameter set, in one GPU pass (the arguments of the single entries;
 * zero means the source's default).  Figure j of series i is at out_figures[j * n_series + i], fp64 [3 x n_series]: SSA period,
 * variance_explained, n_eigenvalues (as a double); STL period, seasonal_strength, trend_strength.  Optional outputs (may be NULL):
 * SSA out_eigenvalues fp64 [C x n_series] with C = n_components, or 10 for 0, and out_detected fp64 [4 x n_series] (the source's
 * detected_periods), both NaN beyond what exists; STL out_index int32 [n_series] (the winning candidate's place in the list, -1
 * for the constant-series return and for a failed series), out_candidates int32 [K x n_series] (-1 beyond the list) and
 * out_candidate_strengths fp64 [K x n_series] (NaN beyond it) with K = max(n_candidates or 20, 5).  A series that is too short,
 * whose SSA window exceeds 2,048 rows or whose STL candidate range is empty fails alone: out_errors[i] (may be NULL) gets the single
 * entry's COMPUTATION_ERROR and its outputs are NaN / -1.  More than 32 components, more than 64 candidates or a series above 65,536
 * rows: INVALID_INPUT naming the limit, for the whole call.  The return value is false only for batch-level failures, also reported
 * through `out_batch_error`.  Runs on the calling thread's current device (anofox_hip_set_devices does not shard it).
 */
bool anofox_hip_ssa_period_batch(const double *const *values,
                                 const size_t *lengths,
                                 size_t n_series,
                                 size_t window_size,
                                 size_t n_components,
                                 double *out_figures,
                                 double *out_eigenvalues,
                                 double *out_detected,
                                 struct AnofoxError *out_errors,
                                 struct AnofoxError *out_batch_error);

bool anofox_hip_stl_period_batch(const double *const *values,
                                 const size_t *lengths,
                                 size_t n_series,
                                 size_t min_period,
                                 size_t max_period,
                                 size_t n_candidates,
                                 double *out_figures,
                                 int32_t *out_index,
                                 int32_t *out_candidates,
                                 double *out_candidate_strengths,
                                 struct AnofoxError *out_errors,
                                 struct AnofoxError *out_batch_error);

/*
 * The same on a device-resident time-major block: y[t * ld + s] (fp64, t < t_rows <= 65,536), lengths[n_series] (int32; a length
 * above t_rows is cut to it) and the outputs are device pointers with row stride ld (figure j of series s at j * ld + s);
 * eigenvalues, detected, candidates and candidate_strengths may be NULL.  status is int32 [n_series]: 0 done, 1 too short, 2 SSA
 * window above 2,048, 3 STL "min_period must be less than max_period", 4 STL "No valid candidate periods found"; nothing else is
 * written for a series whose status is not 0.  One workgroup per series, persistent over the batch.  SSA keeps the L x L matrix in
 * LDS while it fits and otherwise in a workspace of at most 1 GiB whatever n_series is (one 32 MiB slice at the window limit, 330
 * slices of 3.25 MB at n = 1,913); `route` is 0 (windows up to 64 on one wavefront per series, the rest on 256 lanes) or
 * 1 (256 lanes for every window) and does not change a bit of the results.  STL keeps its rows in LDS up to 721
 * observations and otherwise in a workspace of at most 256 MiB.  The same bits on every run and through every entry.  Runs on
 * `stream` (NULL: the null stream) and returns after it has finished.
 */
bool anofox_hip_ssa_period_device(const double *y,
                                  size_t ld,
                                  const int32_t *lengths,
                                  size_t n_series,
                                  size_t t_rows,
                                  size_t window_size,
                                  size_t n_components,
                                  int route,
                                  double *figures,
                                  double *eigenvalues,
                                  double *detected,
                                  int32_t *status,
                                  void *stream,
                                  struct AnofoxError *out_error);

bool anofox_hip_stl_period_device(const double *y,
                                  size_t ld,
                                  const int32_t *lengths,
                                  size_t n_series,
                                  size_t t_rows,
                                  size_t min_period,
                                  size_t max_period,
                                  size_t n_candidates,
                                  double *figures,
                                  int32_t *index,
                                  int32_t *candidates,
                                  double *candidate_strengths,
                                  int32_t *status,
                                  void *stream,
                                  struct AnofoxError *out_error);

/*
 * Matrix-profile period detection of `n_series` series with one parameter set, in one GPU pass (the arguments of the single entry;
 * zero means the source's default, `n_best` is the exclusion zone).  Figure j of series i is at out_figures[j * n_series + i], fp64
 * [6 x n_series]: period, confidence, n_motifs, subsequence_length, best_count (the count of the winning lag) and n_tied (how many
 * lags share it; the smallest is the period).  Optional outputs (may be NULL): out_profile fp64 and out_profile_index int32, both
 * [P_max x n_series] with P_max the profile length n - m + 1 of the LONGEST series of the call (0 rows when that one has fewer than
 * 32 observations): the distance of every subsequence to its nearest neighbour outside the exclusion zone (+inf where it has none)
 * and that neighbour's index (the smallest among equal distances; 0 where there is none, as in the source), NaN / -1 beyond a
 * series' own profile and for a failed series.  A series that is too short or whose subsequence length exceeds 2,048 fails alone:
 * out_errors[i] (may be NULL) gets the single entry's COMPUTATION_ERROR and its figures are NaN.  A series above 65,536 rows:
 * INVALID_INPUT naming the limit, for the whole call.  Non-finite values get no status: a NaN distance never updates a profile
 * entry, and a profile without a finite value gives NaN / 0.0 / 0.  The return value is false only for batch-level failures, also
 * reported through `out_batch_error`.  Runs on the calling thread's current device (anofox_hip_set_devices does not shard it).
 */
bool anofox_hip_matrix_profile_batch(const double *const *values,
                                     const size_t *lengths,
                                     size_t n_series,
                                     size_t subsequence_length,
                                     size_t n_best,
                                     double *out_figures,
                                     double *out_profile,
                                     int32_t *out_profile_index,
                                     struct AnofoxError *out_errors,
                                     struct AnofoxError *out_batch_error);

/*
 * The same on a device-resident time-major block: y[t * ld + s] (fp64, t < t_rows <= 65,536), lengths[n_series] (int32; a length
 * above t_rows is cut to it) and the outputs are device pointers with row stride ld (figure j of series s at j * ld + s).  profile
 * and profile_index may be NULL; they have P_max rows, the profile length of a series of t_rows rows.  status is int32 [n_series]:
 * 0 done, 1 too short, 2 subsequence length above 2,048; the figures are not written for a series whose status is not 0, its
 * profile rows are NaN / -1.  One workgroup per series, persistent over the batch.  The series, its profile and its index live in
 * LDS up to 2,341 rows at the default subsequence length (2,203 with a forced length of 4) and otherwise in a workspace of at most
 * 256 MiB whatever n_series is.  The same bits on every run and through every entry.  Runs on `stream` (NULL: the null stream) on
 * the calling thread's current device and returns after it has finished.
 */
bool anofox_hip_matrix_profile_device(const double *y,
                                      size_t ld,
                                      const int32_t *lengths,
                                      size_t n_series,
                                      size_t t_rows,
                                      size_t subsequence_length,
                                      size_t n_best,
                                      double *figures,
                                      double *profile,
                                      int32_t *profile_index,
                                      int32_t *status,
                                      void *stream,
                                      struct AnofoxError *out_error);

/*
 * Forecast accuracy metrics, the reference's twelve functions of metrics.rs behind their FFI wrappers, with its signatures.  Each
 * call runs on the GPU as a batch of one group; the argument checks come first and need no device.  Any NULL pointer: NULL_POINTER
 * "Null pointer argument".  Different lengths, an empty input or a quantile outside [0, 1]: COMPUTATION_ERROR with the source's text
 * ("Invalid input: Actual and forecast arrays must have the same length: 3 vs 2", "... Actual and baseline arrays ...", "... Actual
 * and pred2 arrays ...", "Insufficient data: need at least 1 observations, got 0", "Invalid input: Quantile must be between 0 and
 * 1").  mqloss: n_levels == 0 is INVALID_INPUT "Must have at least one quantile level", a NULL quantiles[k] is COMPUTATION_ERROR
 * "Invalid input: Null pointer at quantile index k", and more than 16 levels is INVALID_INPUT naming that limit of this backend.
 * coverage of an empty input returns true and NaN.  The results equal the source's arithmetic bit for bit (sequential sums in row
 * order from 0.0), except for the sign of a zero result and NaN payloads.
 */
bool anofox_ts_mae(const double *actual,
                   size_t actual_len,
                   const double *forecast,
                   size_t forecast_len,
                   double *out_result,
                   struct AnofoxError *out_error);

bool anofox_ts_mse(const double *actual,
                   size_t actual_len,
                   const double *forecast,
                   size_t forecast_len,
                   double *out_result,
                   struct AnofoxError *out_error);

bool anofox_ts_rmse(const double *actual,
                    size_t actual_len,
                    const double *forecast,
                    size_t forecast_len,
                    double *out_result,
                    struct AnofoxError *out_error);

bool anofox_ts_mape(const double *actual,
                    size_t actual_len,
                    const double *forecast,
                    size_t forecast_len,
                    double *out_result,
                    struct AnofoxError *out_error);

bool anofox_ts_smape(const double *actual,
                     size_t actual_len,
                     const double *forecast,
                     size_t forecast_len,
                     double *out_result,
                     struct AnofoxError *out_error);

bool anofox_ts_r2(const double *actual,
                  size_t actual_len,
                  const double *forecast,
                  size_t forecast_len,
                  double *out_result,
                  struct AnofoxError *out_error);

bool anofox_ts_bias(const double *actual,
                    size_t actual_len,
                    const double *forecast,
                    size_t forecast_len,
                    double *out_result,
                    struct AnofoxError *out_error);

bool anofox_ts_rmae(const double *actual,
                    size_t actual_len,
                    const double *pred1,
                    size_t pred1_len,
                    const double *pred2,
                    size_t pred2_len,
                    double *out_result,
                    struct AnofoxError *out_error);

bool anofox_ts_mase(const double *actual,
                    size_t actual_len,
                    const double *forecast,
                    size_t forecast_len,
                    const double *baseline,
                    size_t baseline_len,
                    double *out_result,
                    struct AnofoxError *out_error);

bool anofox_ts_quantile_loss(const double *actual,
                             size_t actual_len,
                             const double *forecast,
                             size_t forecast_len,
                             double quantile,
                             double *out_result,
                             struct AnofoxError *out_error);

bool anofox_ts_mqloss(const double *actual,
                      size_t actual_len,
                      const double *const *quantiles,
                      size_t n_levels,
                      const double *levels,
                      double *out_result,
                      struct AnofoxError *out_error);

bool anofox_ts_coverage(const double *actual,
                        size_t actual_len,
                        const double *lower,
                        const double *upper,
                        double *out_result,
                        struct AnofoxError *out_error);

/*
 * Every requested figure of `n_groups` groups from ONE GPU pass over their rows.  Replaces the per-group, per-metric FFI calls of
 * the reference's _ts_metrics_native / _ts_mase_native / _ts_rmae_native / _ts_coverage_native / _ts_quantile_loss_native.
 *
 * Figure order (bit k of figures_mask, row k of the output) and the inputs each figure needs besides `actual`:
 *    0 mae, 1 mse, 2 rmse, 3 mape, 4 smape, 5 r2, 6 bias   forecast
 *    7 rmae, 8 mase                                        forecast and second (pred2 / baseline; both are forecast's MAE / second's MAE)
 *    9 quantile_loss                                       forecast, `quantile`
 *   10 mqloss                                              quantiles, levels, n_levels (1 .. 16)
 *   11 coverage                                            lower and upper
 * A requested figure whose input is NULL, an empty mask or a bit above 11: INVALID_INPUT; more than 16 levels: INVALID_INPUT naming
 * the limit; mqloss with n_levels == 0: INVALID_INPUT "Must have at least one quantile level".
 *
 * actual[i], forecast[i], second[i], lower[i], upper[i] point to the lengths[i] values of group i (an array that no requested
 * figure needs may be NULL as a whole); quantiles[k][i] points to level k's forecasts of group i.  drop_nan: a row in which any
 * SUPPLIED array holds a NaN is skipped for every figure and does not count -- the row filter of the reference's table functions,
 * which filter on exactly the columns their statement uses, so supply exactly those.  out_figures is fp64 [12 x n_groups], figure k
 * of group i at out_figures[k * n_groups + i]; figures that were not requested, or failed, are NaN.  Per-group errors
 * (out_errors[i], may be NULL) follow the single entries: a group with no row (left) is COMPUTATION_ERROR "Insufficient data: need
 * at least 1 observations, got 0" unless coverage is the only figure requested (NaN, no error); a quantile or level outside [0, 1]
 * fails quantile_loss / mqloss with COMPUTATION_ERROR "Invalid input: Quantile must be between 0 and 1" while the other figures are
 * computed; a NULL quantiles[k][i] fails group i with "Invalid input: Null pointer at quantile index k".  The return value is false
 * only for batch-level failures, also reported through `out_batch_error`.  Runs on the calling thread's current device
 * (anofox_hip_set_devices does not shard it).
 */
bool anofox_hip_metrics_batch(const double *const *actual,
                              const double *const *forecast,
                              const double *const *second,
                              const double *const *lower,
                              const double *const *upper,
                              const double *const *const *quantiles,
                              const double *levels,
                              size_t n_levels,
                              const size_t *lengths,
                              size_t n_groups,
                              uint32_t figures_mask,
                              double quantile,
                              bool drop_nan,
                              double *out_figures,
                              struct AnofoxError *out_errors,
                              struct AnofoxError *out_batch_error);

/*
 * The same on device-resident fp64 blocks.  Element (group s, row t) of every input block is at s * stride_s + t * stride_t:
 * stride_s = 1, stride_t = ld_in is the project's time-major block; stride_s = horizon, stride_t = 1 is the series-major
 * [n_series x horizon] layout of anofox_hip_batch_device_results, whose yhat / lower / upper can be scored where they lie.  Level
 * k's forecasts are the block at quantiles + k * stride_q.  `levels` is a HOST array.  lengths is int32 [n_groups] on the device
 * (a length above t_rows is cut to it).  figures is fp64 [12 x ld] (figure k of group s at k * ld + s; only the requested rows
 * and the columns s < n_groups are written), status is int32 [n_groups]: 0 done, 1 no row (left) -- every requested figure NaN.
 * Here a quantile or level outside [0, 1] fails the call (INVALID_INPUT).  One lane per group walks its rows in order; a
 * series-major block goes through LDS tiles of 64 groups, a time-major one is read directly, and both give the same bits.  Runs
 * on `stream` (NULL: the null stream) and returns after it has finished.
 */
bool anofox_hip_metrics_device(const double *actual,
                               const double *forecast,
                               const double *second,
                               const double *lower,
                               const double *upper,
                               const double *quantiles,
                               size_t stride_q,
                               const double *levels,
                               size_t n_levels,
                               size_t stride_s,
                               size_t stride_t,
                               const int32_t *lengths,
                               size_t n_groups,
                               size_t t_rows,
                               uint32_t figures_mask,
                               double quantile,
                               bool drop_nan,
                               double *figures,
                               size_t ld,
                               int32_t *status,
                               void *stream,
                               struct AnofoxError *out_error);

/*
 * Conformal prediction intervals per group on device-resident fp64 blocks (the reference's conformal.rs: conformal_learn,
 * conformal_apply, conformal_coverage / winkler_score / conformal_evaluate).  The contract is equality of bits with the source.
 * Element (group s, row t) of every block of a call is at s * stride_s + t * stride_t, as for anofox_hip_metrics_device: both the
 * time-major block and the series-major [n_series x horizon] layout of anofox_hip_batch_device_results work, with the same bits.
 * `alphas` is a HOST array of 1 .. 16 miscoverage rates, each in [0, 1) (0 is valid, as in the source); an alpha outside, no
 * alpha or more than 16 fail the call with INVALID_INPUT (the last one naming the limit).  Every call runs on `stream` (NULL: the
 * null stream) and returns after it has finished.  Runs on the calling thread's current device (anofox_hip_set_devices does not
 * shard it).  Outputs shaped [rows x ld] have only their columns s < n_groups written.
 *
 * method: 0 symmetric, 1 asymmetric, 2 adaptive.  status, int32 [n_groups]: 0 done; 1 no row (left), figures NaN; 2 a residual
 * is NaN, scores NaN (the source leaves the order of such a vector to its sort's internals); 3 a difficulty <= 0, bounds NaN.
 *
 * learn: the residual of row t is residual[..] or, when `residual` is NULL, actual[..] - forecast[..] (one fp64 subtraction).
 * valid (may be NULL) has one byte per element at the same offsets; a row whose byte is 0 is dropped.  lengths is int32
 * [n_groups] on the device (a length above t_rows is cut to it; pass the longest group's length as t_rows, the kernel's LDS tile is
 * sized from it).  Symmetric and adaptive: the conformity score of level k, compute_quantile(sorted |r|, clamp(ceil((n + 1)
 * (1 - alpha_k)) / n, 0, 1)), goes to scores_lower[k * ld + s] and scores_upper[k * ld + s].  Asymmetric: alpha_k / 2, the
 * positives (r > 0) give scores_upper, the magnitudes of the negatives (r < 0) scores_lower, an empty set gives 0.0.  sorted (may
 * be NULL) is a block with the inputs' strides whose rows 0 .. n_kept - 1 receive the ascending |r| of the group (Jackknife+'s
 * state vector; not written for status 2); n_kept (may be NULL) is int32 [n_groups].  One wavefront per group sorts in LDS; groups
 * above 2,048 rows sort in a global workspace.
 */
bool anofox_hip_conformal_learn_device(const double *residual,
                                       const double *actual,
                                       const double *forecast,
                                       const uint8_t *valid,
                                       size_t stride_s,
                                       size_t stride_t,
                                       const int32_t *lengths,
                                       size_t n_groups,
                                       size_t t_rows,
                                       const double *alphas,
                                       size_t n_alphas,
                                       int method,
                                       double *scores_lower,
                                       double *scores_upper,
                                       size_t ld,
                                       double *sorted,
                                       int32_t *n_kept,
                                       int32_t *status,
                                       void *stream,
                                       struct AnofoxError *out_error);

/*
 * apply: for level k and step t < lengths[s] (lengths NULL: every group has h_rows steps), lower = f - scores_lower[k * ld + s] * d
 * and upper = f + scores_upper[k * ld + s] * d, written to lower + k * stride_q and upper + k * stride_q at the forecast's offsets.
 * d = 1 (no multiplication) unless the method is adaptive; then d = difficulty / mean, the mean being the group's sequential sum
 * in row order divided by its count.  A difficulty <= 0 anywhere in the group: status 3 and NaN bounds.  A group with no step:
 * status 1.  The scores of a group that learn could not answer are NaN, and so are its bounds.
 */
bool anofox_hip_conformal_apply_device(const double *forecast,
                                       const double *difficulty,
                                       size_t stride_s,
                                       size_t stride_t,
                                       const int32_t *lengths,
                                       size_t n_groups,
                                       size_t h_rows,
                                       const double *scores_lower,
                                       const double *scores_upper,
                                       size_t ld,
                                       size_t n_alphas,
                                       int method,
                                       double *lower,
                                       double *upper,
                                       size_t stride_q,
                                       int32_t *status,
                                       void *stream,
                                       struct AnofoxError *out_error);

/*
 * evaluate: figures is fp64 [5 x ld]: 0 coverage (rows with lower <= actual <= upper over n), 1 violation_rate (1 - coverage),
 * 2 mean_width (sequential sum of upper - lower over n), 3 winkler_score (penalty 2 / alpha), 4 n_observations.  A group with no
 * row: status 1, figures NaN (n_observations 0).
 */
bool anofox_hip_conformal_evaluate_device(const double *actual,
                                          const double *lower,
                                          const double *upper,
                                          size_t stride_s,
                                          size_t stride_t,
                                          const int32_t *lengths,
                                          size_t n_groups,
                                          size_t t_rows,
                                          double alpha,
                                          double *figures,
                                          size_t ld,
                                          int32_t *status,
                                          void *stream,
                                          struct AnofoxError *out_error);

/* One group's answer of anofox_hip_conformal_batch; every array is owned by the result (anofox_hip_free_conformal). */
typedef struct AnofoxHipConformal {
    double *scores_lower;  /* [n_levels] conformity score of every level (asymmetric: from the negatives) */
    double *scores_upper;  /* [n_levels] the same value, or (asymmetric) the score from the positives     */
    double *sorted;        /* [n_residuals] ascending |residual| (Jackknife+'s state vector), NULL unless requested */
    size_t n_residuals;    /* residuals kept (not NULL)                                                    */
    double *lower;         /* [n_levels x n_forecasts] level k's lower bounds at k * n_forecasts           */
    double *upper;         /* [n_levels x n_forecasts]                                                      */
    size_t n_forecasts;
    size_t n_levels;
} AnofoxHipConformal;

/*
 * learn -> apply for many groups from host pointers in ONE call (the reference's conformalize, one FFI call per group there).
 * residuals[i] points to the residual_lengths[i] calibration residuals of group i; residual_validity (may be NULL, and so may
 * residual_validity[i]) is its validity bitmask, bit t of word t / 64 clear = NULL, dropped as the table macros' IS NOT NULL filter
 * does.  forecasts[i] points to the forecast_lengths[i] point forecasts (forecasts may be NULL as a whole: learn only, no bounds).
 * difficulty[i] (adaptive method only) has forecast_lengths[i] values.  strategy: 0 split, 1 cross-validation, 2 Jackknife+ --
 * the scores are the same for all three (as in the source); Jackknife+ with the asymmetric method is INVALID_INPUT.  want_sorted:
 * also return the sorted |residual| of every group.  Batch-level failures (a NULL argument, no alpha, more than 16, an alpha outside
 * [0, 1), an unknown method or strategy, a device failure) return false and are reported through out_batch_error.  Per-group
 * errors (out_errors[i], may be NULL; the result's arrays are NULL then) carry the source's texts: no residual (left)
 * "Insufficient data: need at least 1 observations, got 0"; no forecast "Invalid input: At least one forecast is required"; a
 * difficulty <= 0 "Invalid input: Difficulty scores must be positive"; a NaN residual "Invalid input: a residual is NaN" (this
 * backend's limit).  Release with anofox_hip_free_conformal(results, n_groups).
 */
bool anofox_hip_conformal_batch(const double *const *residuals,
                                const uint64_t *const *residual_validity,
                                const size_t *residual_lengths,
                                const double *const *forecasts,
                                const double *const *difficulty,
                                const size_t *forecast_lengths,
                                size_t n_groups,
                                const double *alphas,
                                size_t n_alphas,
                                int method,
                                int strategy,
                                bool want_sorted,
                                struct AnofoxHipConformal *out_results,
                                struct AnofoxError *out_errors,
                                struct AnofoxError *out_batch_error);
void anofox_hip_free_conformal(struct AnofoxHipConformal *results, size_t n_groups);

/*
 * The reference's conformal entries (anofox_fcst_ffi.h, lib.rs:4747-5400) with its signatures, struct layouts and error texts, each
 * a batch of one through the same kernels; the argument checks come first and need no device.  A NULL pointer: NULL_POINTER "Null
 * pointer argument" (anofox_ts_conformal_quantile's out_result: "Null output pointer").  `validity` / `residuals_validity` (may be
 * NULL) is the bitmask of the residuals, bit t of word t / 64 clear = NULL, dropped before anything else.  What the source's
 * functions refuse is COMPUTATION_ERROR with their text, in their order: "Insufficient data: need at least 1 observations, got 0",
 * "Invalid input: Alpha must be between 0 and 1 (exclusive)" (quantile, predict, predict_multi, predict_adaptive,
 * predict_asymmetric), "Invalid input: Alpha must be in (0, 1), got 1.5" (learn, evaluate), "Invalid input: At least one alpha value
 * is required", "Invalid input: At least one forecast is required" (apply), "Invalid input: Difficulty scores required for adaptive
 * method", "Invalid input: Difficulty length (4) must match residuals length (3)", "Invalid input: Difficulty scores must be
 * positive", "Invalid input: JackknifePlus strategy does not support asymmetric method".  This backend's own limits: more than 16
 * levels is INVALID_INPUT naming the limit, a NaN residual is COMPUTATION_ERROR "Invalid input: a residual is NaN" (DESIGN.md
 * section 7).  Arrays of a result are malloc'ed, NULL when empty, and released by the result's free function (anofox_ts_conformal_
 * intervals' two arrays by anofox_free_double_array).  anofox_ts_conformal_predict_per_step and the bootstrap entries are not
 * provided.
 */
#ifndef ANOFOX_FCST_FFI_H
typedef struct ConformalResultFFI {
    double *point;
    double *lower;
    double *upper;
    size_t n_forecasts;
    double coverage;          /* 1 - alpha */
    double conformity_score;
    char method[32];          /* "split_conformal", "adaptive_conformal", "asymmetric_conformal" */
} ConformalResultFFI;

typedef struct ConformalMultiResultFFI {
    double *point;
    size_t n_forecasts;
    double *coverage_levels;  /* [n_levels] */
    double *conformity_scores;/* [n_levels] */
    size_t n_levels;
    double *lower;            /* [n_levels x n_forecasts], level-major */
    double *upper;
} ConformalMultiResultFFI;

typedef enum ConformalMethodFFI { CONFORMAL_METHOD_SYMMETRIC = 0, CONFORMAL_METHOD_ASYMMETRIC = 1, CONFORMAL_METHOD_ADAPTIVE = 2 } ConformalMethodFFI;
typedef enum ConformalStrategyFFI { CONFORMAL_STRATEGY_SPLIT = 0, CONFORMAL_STRATEGY_CROSS_VAL = 1, CONFORMAL_STRATEGY_JACKKNIFE_PLUS = 2 } ConformalStrategyFFI;

typedef struct CalibrationProfileFFI {
    ConformalMethodFFI method;
    ConformalStrategyFFI strategy;
    double *alphas;           /* [n_levels] */
    double *state_vector;     /* split / crossval: scores_lower then scores_upper; jackknife+: the sorted |residual| */
    size_t state_vector_len;
    double *scores_lower;     /* [n_levels] */
    double *scores_upper;     /* [n_levels] */
    size_t n_levels;
    size_t n_residuals;
} CalibrationProfileFFI;

typedef struct PredictionIntervalsFFI {
    double *point;
    size_t n_forecasts;
    double *coverage;         /* [n_levels] 1 - alpha */
    size_t n_levels;
    double *lower;            /* [n_levels x n_forecasts], level-major */
    double *upper;
    ConformalMethodFFI method;
} PredictionIntervalsFFI;

typedef struct ConformalEvaluationFFI {
    double coverage;
    double violation_rate;
    double mean_width;
    double winkler_score;
    size_t n_observations;
} ConformalEvaluationFFI;
#endif /* ANOFOX_FCST_FFI_H */

bool anofox_ts_conformal_quantile(const double *residuals, const uint64_t *validity, size_t length, double alpha, double *out_result,
                                  struct AnofoxError *out_error);
bool anofox_ts_conformal_intervals(const double *forecasts, size_t length, double conformity_score, double **out_lower, double **out_upper,
                                   struct AnofoxError *out_error);
bool anofox_ts_conformal_predict(const double *residuals, const uint64_t *residuals_validity, size_t residuals_length,
                                 const double *forecasts, size_t forecasts_length, double alpha, struct ConformalResultFFI *out_result,
                                 struct AnofoxError *out_error);
bool anofox_ts_conformal_predict_multi(const double *residuals, const uint64_t *residuals_validity, size_t residuals_length,
                                       const double *forecasts, size_t forecasts_length, const double *alphas, size_t n_alphas,
                                       struct ConformalMultiResultFFI *out_result, struct AnofoxError *out_error);
bool anofox_ts_conformal_predict_adaptive(const double *residuals, const uint64_t *residuals_validity, size_t residuals_length,
                                          const double *forecasts, const double *difficulty, size_t forecasts_length, double alpha,
                                          struct ConformalResultFFI *out_result, struct AnofoxError *out_error);
bool anofox_ts_conformal_predict_asymmetric(const double *residuals, const uint64_t *residuals_validity, size_t residuals_length,
                                            const double *forecasts, size_t forecasts_length, double alpha,
                                            struct ConformalResultFFI *out_result, struct AnofoxError *out_error);
bool anofox_ts_mean_interval_width(const double *lower, const double *upper, size_t length, double *out_result,
                                   struct AnofoxError *out_error);
/* difficulty (may be NULL unless the method is adaptive) has residuals_length values */
bool anofox_ts_conformal_learn(const double *residuals, const uint64_t *residuals_validity, size_t residuals_length, const double *alphas,
                               size_t n_alphas, ConformalMethodFFI method, ConformalStrategyFFI strategy, const double *difficulty,
                               struct CalibrationProfileFFI *out_profile, struct AnofoxError *out_error);
/* difficulty (may be NULL unless the profile's method is adaptive) has n_forecasts values */
bool anofox_ts_conformal_apply(const double *forecasts, size_t n_forecasts, const struct CalibrationProfileFFI *profile,
                               const double *difficulty, struct PredictionIntervalsFFI *out_intervals, struct AnofoxError *out_error);
bool anofox_ts_conformal_coverage(const double *actuals, const double *lower, const double *upper, size_t length, double *out_coverage,
                                  struct AnofoxError *out_error);
bool anofox_ts_conformal_evaluate(const double *actuals, const double *lower, const double *upper, size_t length, double alpha,
                                  struct ConformalEvaluationFFI *out_eval, struct AnofoxError *out_error);
void anofox_free_conformal_result(struct ConformalResultFFI *result);
void anofox_free_conformal_multi_result(struct ConformalMultiResultFFI *result);
void anofox_free_calibration_profile(struct CalibrationProfileFFI *result);
void anofox_free_prediction_intervals(struct PredictionIntervalsFFI *result);

/*
 * Multi-device execution of the batch entry.  The reference's finalize loop is ONE process walking all groups
 * (src/table_functions/ts_forecast_native.cpp:559-800); series are independent, so anofox_ts_forecast_batch shards
 * contiguous series-id ranges [g * ceil(N / G), (g + 1) * ceil(N / G)) over the G devices named here: one host thread,
 * stream set and allocator cache per device, each range packed into its device's own pinned staging block, results
 * written straight into the caller's arrays (host side: no RCCL involved).  Default: the caller's current device only.
 * `devices` = ordinal list (a device may be listed more than once: its ranges then run as separate batches on it);
 * n_devices = 0 restores the default.  The environment variable ANOFOX_HIP_DEVICES ("0,1,2,3" or "all"), read once at
 * the first batch call, gives the initial list.  Batches smaller than `min_series_per_device` (default 2,048) per
 * device use fewer devices.  Returns false (nothing changed) when an ordinal is not a visible device.
 */
bool anofox_hip_set_devices(const int *devices, size_t n_devices);
size_t anofox_hip_get_devices(int *devices, size_t capacity);      /* returns the number of devices in use (0 = default) */
void anofox_hip_set_min_series_per_device(size_t min_series);
/* The range of shard `shard` of `n_shards`: [shard * ceil(N / n_shards), ...) clipped to N. */
void anofox_hip_shard_range(size_t n_series, size_t n_shards, size_t shard, size_t *begin, size_t *end);

/*
 * AutoARIMA estimation method -- a caller-visible choice (the reference's `AutoARIMAConfig::default()`,
 * forecast.rs:1447-1455, exposes none, and its measured cost, benchmark/README.md:55, leaves no room for an exact-likelihood
 * refit: DESIGN.md section 3).  ANOFOX_ARIMA_CSS (default): the selected model keeps the conditional-sum-of-squares
 * estimates of the search.  ANOFOX_ARIMA_CSS_ML: the selected model is re-estimated on the exact Gaussian likelihood
 * (Kalman filter of the Harvey state space, evaluated through the Chandrasekhar recursions: BASELINE.json's "Kalman
 * kernel").  The process default applies to anofox_ts_forecast / anofox_ts_forecast_batch and to batches created afterwards;
 * anofox_hip_batch_set_arima_method (block 3) overrides it per batch.
 */
enum { ANOFOX_ARIMA_CSS = 0, ANOFOX_ARIMA_CSS_ML = 1 };
bool anofox_hip_set_default_arima_method(int method);

/*
 * The library keeps idle device blocks (per device at most ANOFOX_HIP_CACHE_GB, default a quarter of the device, oldest
 * evicted first), pinned staging blocks (ANOFOX_HIP_PINNED_CACHE_GB, default 2), stream / event sets and up to 32 parked
 * single-series batches for re-use (a batch of the M5 shape is ~300 hipMalloc calls = 0.4 s without them).  This gives all of
 * it back: call it when the host wants the memory (another allocator in the process is short of HBM) or before unloading.
 * Safe while other threads run batches: only idle resources are touched.
 */
void anofox_hip_release_caches(void);

/* ------------------------------------------------------------------------- */
/* Block 3: device-resident batch (series block already in HBM)               */
/* ------------------------------------------------------------------------- */

typedef struct AnofoxHipBatch AnofoxHipBatch; /* opaque plan + HBM workspace */

/* Per-run measurements, filled by anofox_hip_batch_run. */
typedef struct AnofoxHipStats {
    uint64_t n_series;
    uint64_t t_max;
    uint64_t n_problems;        /* (series, candidate spec) optimiser problems */
    uint64_t total_passes;      /* streamed passes over a series (sum over problems) */
    uint64_t max_passes;        /* max over series of its summed passes          */
    uint64_t total_evals;       /* objective evaluations (>= passes)             */
    uint64_t algorithmic_bytes; /* sum_s 8*T_s*(P_s+1) + 24*h, SURVEY.md 8(d)    */
    double   fit_kernel_ms;     /* HIP-event time of the dominant (fit) kernel(s) */
    double   total_device_ms;   /* HIP-event time of the whole run on its stream  */
    uint32_t fit_kernel_launches;
    uint32_t y_storage;         /* what the ETS fit of the run streamed (round 6; the field was `reserved`, always 0): 0 the fp64 block,
                                   1 / 2 a float / uint16_t copy of it -- made when EVERY observation of the batch survives that type
                                   exactly (counts), so the fp64 arithmetic sees the same numbers; algorithmic_bytes keeps SURVEY.md's
                                   unit (8 bytes per observation and pass) whatever was streamed */
    uint64_t total_iters;       /* Nelder-Mead iterations summed over the ETS problems (each problem counts from 1: the initial
                                   simplex) -- the passes a one-pass-per-iteration schedule needs; 0 for models without spec slots */
    uint64_t min_pass_bytes;    /* sum over problems of 8*T_s*(iterations + 1 final pass) + 24*h per series: the algorithmic bytes
                                   of that schedule ("if the kernel evaluates k simplex vertices in one pass, that
                                   is one pass"), independent of which driver ran which round                                  */
} AnofoxHipStats;

/*
 * Lane-level efficiency of the Nelder-Mead round kernels of the last run (round 5).  A wave streams a pass as long as ONE of its 64
 * lanes still evaluates a trial point; a lane whose problem has converged, or that has used the round's budget, idles until the wave
 * leaves.  wave_passes = passes streamed by waves, live_lane_passes = lane-passes that evaluated a point of a running problem (the
 * four-lanes-per-problem and one-wave-per-problem drivers count every lane that evaluates a speculative point), so
 * live_lane_passes / (64 * wave_passes) is the share of issued lanes that did work.  Classes: 0 additive-class specs, 1 general-class
 * specs, 2 damped multiplicative-trend specs (b^phi every step).  Per slot: the spec id (error * 15 + trend * 3 + season; trend
 * 0 N, 1 A, 2 Ad, 3 M, 4 Md) and its two counters.  Versioned by size: pass sizeof(AnofoxHipLaneStats) of the header you compiled
 * against; the library writes min(struct_size, its own size) bytes and stores that number in `struct_size` (an older caller never
 * sees bytes it did not allocate -- what anofox_hip_batch_stats, whose struct grew in round 4, cannot promise).
 */
typedef struct AnofoxHipLaneStats {
    uint64_t struct_size;
    uint64_t wave_passes[3];
    uint64_t live_lane_passes[3];
    uint32_t n_slots;
    uint32_t reserved;
    int32_t  slot_spec_id[30];
    uint64_t slot_wave_passes[30];
    uint64_t slot_live_lane_passes[30];
} AnofoxHipLaneStats;

/* Device selection; returns number of visible devices or -1. */
int anofox_hip_device_count(void);
int anofox_hip_set_device(int device);

/*
 * Create a plan for `n_series` series of at most `t_max` observations.
 * Validates the option block exactly like anofox_ts_forecast would (model name,
 * ETS notation, pool, seasonal_period compatibility).  The packed layout is the
 * time-major block Y[t * ld + s] (fp64), ld = n_series rounded up to 64.
 */
bool anofox_hip_batch_create(size_t n_series, size_t t_max,
                             const struct ForecastOptions *options,
                             AnofoxHipBatch **out_batch,
                             struct AnofoxError *out_error);
void anofox_hip_batch_destroy(AnofoxHipBatch *batch);

size_t anofox_hip_batch_ld(const AnofoxHipBatch *batch);
size_t anofox_hip_batch_n_series(const AnofoxHipBatch *batch);

/*
 * ETS(spec) with GIVEN smoothing parameters (BASELINE.json configs[1]: "ETS(A,A,A) fixed smoothing params"): the batch
 * must have been created for model "ETS" with an explicit `ets_model`.  No optimiser runs: every series takes ONE
 * streamed pass (initial states as in the fitted path, then filter + forecast with these parameters).  Parameters are in
 * the model's own terms, as anofox_hip_batch_inspect reports them: 0 < alpha < 1, 0 <= beta <= alpha,
 * 0 <= gamma <= 1 - alpha, 0 < phi <= 1; the ones the spec does not have are ignored.  What the external crate's
 * `ETS::new(spec, m)` + explicit parameters would be for forecast.rs:1357-1367; additive, no reference entry exists.
 */
bool anofox_hip_batch_set_fixed_params(AnofoxHipBatch *batch, double alpha, double beta, double gamma, double phi,
                                       struct AnofoxError *out_error);

/* AutoARIMA estimation method of this batch: ANOFOX_ARIMA_CSS / ANOFOX_ARIMA_CSS_ML (see block 2). */
bool anofox_hip_batch_set_arima_method(AnofoxHipBatch *batch, int method, struct AnofoxError *out_error);

/* Host series -> HBM block (NULL interpolation, imputation.rs:61-114, then pack + H2D). */
bool anofox_hip_batch_pack_host(AnofoxHipBatch *batch,
                                const double *const *values,
                                const uint64_t *const *validity,
                                const size_t *lengths,
                                struct AnofoxError *out_error);

/*
 * Adopt a block that is already in HBM: `d_y` is [t_max x ld] fp64 time-major,
 * `d_len` is int32[n_series].  No copy; the caller keeps both alive.  The block
 * holds no NULLs.  With auto_detect_seasonality and seasonal_period 0 the periods
 * are detected here, on the device, as the host packer has them detected.
 */
bool anofox_hip_batch_set_device_block(AnofoxHipBatch *batch,
                                       const void *d_y, size_t ld,
                                       const void *d_len,
                                       struct AnofoxError *out_error);

/*
 * Adopt exogenous regressor blocks that are already in HBM, without a copy: `d_x` is [k x t_max x ld] fp64 with regressor j of
 * series s at d_x[(j * t_max + t) * ld + s] (the layout of the series block, once per regressor; rows t >= the series' length are
 * not read), `d_future` is [k x horizon x ld] with d_future[(j * horizon + i) * ld + s].  t_max, ld and horizon are the batch's
 * (anofox_hip_batch_create, anofox_hip_batch_ld); the pointers are 8-byte aligned device pointers, and both blocks must stay
 * alive and unchanged until every run that uses them has finished.  From then on anofox_hip_batch_run takes the ARIMAX path when
 * the batch's model is ARIMA or AutoARIMA (model_code 50 = "ARIMAX") and ignores the blocks for every other model, like the
 * reference.  k = 0 clears them: the batch runs its ordinary model again.  k > 8: COMPUTATION_ERROR.
 */
bool anofox_hip_batch_set_exog_device(AnofoxHipBatch *batch, const void *d_x, const void *d_future, size_t k,
                                      struct AnofoxError *out_error);

/*
 * The least-squares fit of the last ARIMAX run (waits for it): out_intercept[n_series], out_beta[n_series x k] (0.0 for a
 * regressor that was left out), out_used[n_series] (bit j = regressor j was used); each may be NULL.  Series that failed report
 * NaN / 0.  False when the last run did not take the ARIMAX path.
 */
bool anofox_hip_batch_exog_coefficients(AnofoxHipBatch *batch, double *out_intercept, double *out_beta, uint32_t *out_used,
                                        struct AnofoxError *out_error);

/*
 * The seasonal period every series of the packed / adopted block runs with: the caller's, or -- auto_detect_seasonality with
 * seasonal_period 0 -- the lag of the strongest autocorrelation peak (seasonality.rs:323-377 detect_seasonality_first, 1 when
 * there is none), found by detect_period_kernel on the resident block.  False before a block is set.
 */
bool anofox_hip_batch_periods(const AnofoxHipBatch *batch, int32_t *out_periods);

/*
 * Self test of the kernels' reciprocal (csrc/det_math.hpp dm_recip: v_rcp_f64 + two Newton steps + one correction, the division
 * expansion without range scaling and fix-up) against the compiled IEEE division on `n_operands` generated operands covering
 * [2^-1000, 2^1000] in both signs: *out_mismatches = operands whose two quotients differ in any bit (the parity contract needs 0:
 * oracle/ets.c divides), *out_first_bad (may be NULL) one such operand.  False when no device could run it.
 */
bool anofox_hip_selftest_recip(uint64_t n_operands, uint64_t seed, uint64_t *out_mismatches, double *out_first_bad);

/*
 * Self test of the kernels' elementary functions (csrc/det_math.hpp, csrc/det_trig.hpp): evaluates function `fn` on the device
 * at the caller's operands, one thread per operand, through the very inline functions the fit kernels call.  x, y, out, out2 are
 * HOST arrays of n doubles; y may be NULL where the function takes one operand, out2 is written by SINCOS only (NULL otherwise).
 *   LOG        out = dm_log(x)
 *   EXP        out = dm_exp(x)
 *   SCALBN     out = dm_scalbn(x, (int)y)
 *   POW_STEP   out = dm_pow_step(x, y)            x in [2^-1000, 2^1000], 0 < y <= 1; the tables are the workgroup's LDS copy
 *   POW_NEAR1  out = dm_pow_near1(x, coef(y))     x = r = b - 1, |r| <= 2^-4; the coefficients are dm_pow_near1_coef(y) on the device
 *   POW_POS    out = dm_pow_pos(x, y)
 *   SINCOS     out = sin x, out2 = cos x          per_sincos
 * block_threads is the workgroup size of the launch: 64 (the fit kernels' NM_BLOCK) or 256; anything else is refused.  The parity
 * contract: every result has the bits of oracle/det_math.h / oracle/det_trig.h at the same operand, whatever the workgroup size and n.
 * False with *err set for a bad argument, and when no device could run it.  Takes no environment switch, keeps no state.
 */
typedef enum AnofoxHipMathFn {
    ANOFOX_HIP_MATH_LOG = 0,
    ANOFOX_HIP_MATH_EXP = 1,
    ANOFOX_HIP_MATH_SCALBN = 2,
    ANOFOX_HIP_MATH_POW_STEP = 3,
    ANOFOX_HIP_MATH_POW_NEAR1 = 4,
    ANOFOX_HIP_MATH_POW_POS = 5,
    ANOFOX_HIP_MATH_SINCOS = 6,
    ANOFOX_HIP_MATH_FN_COUNT = 7,
} AnofoxHipMathFn;
bool anofox_hip_selftest_math(int fn, const double *x, const double *y, uint64_t n, int block_threads,
                              double *out, double *out2, struct AnofoxError *err);

/* Lane-level efficiency counters of the last run (waits for it); false before a run. */
bool anofox_hip_batch_lane_stats(AnofoxHipBatch *batch, AnofoxHipLaneStats *out, size_t struct_size);

/* Asynchronous fit + forecast, ordered on `stream` (a hipStream_t).  NULL is NOT the null stream: it means the batch's own non-blocking stream, which the null stream does not wait for -- wait for the batch (anofox_hip_batch_stats / _fetch, or a device-wide wait) before reading its results from another stream.
 * Host wait: with model IMAPA the call waits once on `stream`, after the first of its kernels, to read back the batch's largest aggregation level (it sizes the per-(level, series) buffer); the rest of the run stays asynchronous. */
bool anofox_hip_batch_run(AnofoxHipBatch *batch, void *stream,
                          struct AnofoxError *out_error);

/*
 * Run several batches side by side, one host thread each -- the device-resident counterpart of the multi-device batch
 * entry: create one batch per device (anofox_hip_set_device(d) before each create; a batch remembers its device and every
 * entry point makes it current for its own duration), adopt each device's block, run them together.  out_errors may be
 * NULL; returns false if any run failed.
 */
bool anofox_hip_batch_run_many(AnofoxHipBatch *const *batches, size_t n_batches, struct AnofoxError *out_errors);

/* Waits for the run, then fills `out_stats`. */
bool anofox_hip_batch_stats(AnofoxHipBatch *batch, AnofoxHipStats *out_stats);

/*
 * Device result pointers (valid until destroy): yhat/lower/upper are
 * [n_series x horizon] fp64 row-major; model_code int32[n_series] (see
 * anofox_hip_model_name); status int32[n_series] (ErrorCode per series).
 */
bool anofox_hip_batch_device_results(AnofoxHipBatch *batch,
                                     void **d_yhat, void **d_lower, void **d_upper,
                                     void **d_model_code, void **d_status);

/* D2H + per-series malloc'd results with reference ownership rules. */
bool anofox_hip_batch_fetch(AnofoxHipBatch *batch,
                            struct ForecastResult *out_results,
                            struct AnofoxError *out_errors);

/*
 * Fit-state snapshot of a batch that has been run (what ts_forecast_inspect_by /
 * ts_forecast_explain_by read out of a fitted model, forecast.rs:1739-1885, 1899-2017).  For AutoETS and ETS(spec):
 * the smoothing parameters in the model's own terms (beta = alpha beta*, gamma = gamma* (1 - alpha); NaN where the
 * spec has no such component), AIC / AICc / BIC, SSE, the final level and growth (growth NaN without a trend), optionally the
 * final seasonal states by phase (`seasonal`, row stride `seasonal_stride` >= period) and the one-step fitted values (`fitted`, [n_series x
 * t_max] row-major, NaN past a series' length).  A second streamed pass per candidate spec on the device produces
 * them; series that took the fallback chain, and every other model, report NaN (AutoARIMA reports its AICc; its orders
 * are in model_code).  The batch must have one seasonal period.
 */
typedef struct AnofoxHipInspection {
    int32_t model_code;      /* as in anofox_hip_batch_device_results */
    int32_t status;          /* ErrorCode of the series */
    int32_t seasonal_period;
    int32_t reserved;
    double alpha, beta, gamma, phi;
    double aic, aicc, bic, sse;
    double level, trend;     /* final states l_T, b_T */
} AnofoxHipInspection;
bool anofox_hip_batch_inspect(AnofoxHipBatch *batch, AnofoxHipInspection *out,
                              double *fitted, double *seasonal, size_t seasonal_stride,
                              struct AnofoxError *out_error);

/*
 * The selected AutoARIMA fit of every series of a batch that has been run: what a caller needs to evaluate the model itself.
 * Waits for the run; copies only, no kernel runs.  The coefficients are the ones the recursion reads -- the optimiser's
 * coordinates clipped to the box [-0.99, 0.99] -- in the convention (1 - phi(B))(1 - Phi(B^m)) w'_t = (1 - theta(B))(1 - Theta(B^m)) e_t
 * with w' = w - constant on the differenced series w (seasonal difference first, then the d ordinary ones); slots beyond the
 * orders are 0.0.  `aicc` is the criterion of the conditional sum of squares the model was selected and polished with,
 * n_diff log(css / (n_diff - p - m P)) + 2 k + 2 k (k + 1) / (n_diff - k - 1), k = p + q + P + Q + has_constant + 1; after an
 * ANOFOX_ARIMA_CSS_ML run the coefficients are the exact-likelihood refit's and `aicc` is still the CSS run's.  It reports what
 * the LAST run left.  A series nothing was fitted to (status != 0, or a model_code below 1000000) has zero orders and counters
 * and NaN in every double.  False with an error when the batch's model is not AutoARIMA, has not been run, or does not have one
 * seasonal period.
 */
typedef struct AnofoxHipArimaFit {
    int32_t status;          /* ErrorCode of the series */
    int32_t model_code;      /* as in anofox_hip_batch_device_results */
    int32_t seasonal_period; /* the period the series was fitted with */
    int32_t p, d, q, P, D, Q;
    int32_t has_constant;
    int32_t n_diff;          /* length of the differenced series: n - d - D m */
    int32_t models_tried;    /* candidates of the stepwise search */
    int32_t evals;           /* objective evaluations of the search, the polish and the refit */
    int32_t reserved;
    double phi[5], theta[5], Phi[2], Theta[2];
    double constant;         /* mean of the differenced series (0.0 without a constant) */
    double aicc;
} AnofoxHipArimaFit;
bool anofox_hip_batch_arima_fit(AnofoxHipBatch *batch, AnofoxHipArimaFit *out, struct AnofoxError *out_error);

/* Render a device model_code to the reference's model_name text (<= 63 chars). */
void anofox_hip_model_name(const struct ForecastOptions *options, int32_t model_code,
                           char out_name[64]);
/*
 * The same for a series of a batch: an AutoARIMA code is rendered with the period THAT SERIES was fitted with -- the given one,
 * or the one detect_period_kernel found on a resident block (anofox_hip_batch_periods) -- i.e. exactly the name
 * anofox_hip_batch_fetch writes ("AutoARIMA(p,d,q)(P,D,Q)[m]", forecast.rs:1469-1493).  anofox_hip_model_name only has the option
 * block, whose seasonal_period is 0 when periods are detected.
 */
void anofox_hip_batch_model_name(const AnofoxHipBatch *batch, size_t series, int32_t model_code, char out_name[64]);

/* ------------------------------------------------------------------------- */
/* Block 4: columnar ingest for the table-in-out caller (route B)              */
/* ------------------------------------------------------------------------- */
/*
 * Replaces the collection loop of _ts_forecast_native
 * (src/table_functions/ts_forecast_native.cpp:476-610: per-row GetValue into a
 * std::map<string, GroupData> under a mutex, per-group sort at finalize).
 * The binding appends each DataChunk as plain columns; `group_key` is the
 * dictionary id (or hash) of the group value -- the binding keeps id -> Value.
 * Rules kept: rows with a NULL date are dropped (:505); a NULL target is an
 * invalid slot (interpolated by the packer, imputation.rs:61-114); groups come
 * out in first-appearance order (:586); rows of a group are stably sorted by date.
 * append is thread-safe; validity bitmasks use DuckDB's layout (bit i%64 of word
 * i/64, 1 = valid) and may be NULL (= all valid).
 */
typedef struct AnofoxHipIngest AnofoxHipIngest;
AnofoxHipIngest *anofox_hip_ingest_create(void);
void anofox_hip_ingest_destroy(AnofoxHipIngest *ingest);
bool anofox_hip_ingest_append(AnofoxHipIngest *ingest,
                              const int64_t *group_key, const int64_t *date,
                              const uint64_t *date_valid,
                              const double *value, const uint64_t *value_valid,
                              size_t n_rows, struct AnofoxError *out_error);
bool anofox_hip_ingest_finish(AnofoxHipIngest *ingest, size_t *n_groups, size_t *t_max,
                              struct AnofoxError *out_error);
/* Valid after finish, owned by the ingest: [n_groups] each. */
const int64_t *anofox_hip_ingest_group_keys(const AnofoxHipIngest *ingest);
const int64_t *anofox_hip_ingest_last_dates(const AnofoxHipIngest *ingest);
const size_t *anofox_hip_ingest_lengths(const AnofoxHipIngest *ingest);
const double *const *anofox_hip_ingest_values(const AnofoxHipIngest *ingest);
const uint64_t *const *anofox_hip_ingest_validity(const AnofoxHipIngest *ingest);
/* Series of a finished ingest -> the batch's HBM block (batch created with n_groups, t_max). */
bool anofox_hip_batch_pack_ingest(AnofoxHipBatch *batch, const AnofoxHipIngest *ingest,
                                  struct AnofoxError *out_error);

/* ------------------------------------------------------------------------- */
/* Block 5: the walk-forward backtest of _ts_backtest_native on the device    */
/* ------------------------------------------------------------------------- */
/* One fold of ComputeFoldBoundaries (ts_backtest_native.cpp:623-711): inclusive row positions, the same for every series. */
typedef struct AnofoxHipFold {
    int64_t fold_id;          /* 1-based, as the operator's fold_id column */
    int64_t train_start, train_end;
    int64_t test_start, test_end;
} AnofoxHipFold;

/*
 * ComputeFoldBoundaries restated: the folds of `n_dates` distinct dates.  window_type: 0 expanding, 1 fixed, 2 sliding (both cut
 * the training window to min_train_size rows); initial_train_size <= 0: n_dates - horizon * folds (at least 1); skip_length <= 0:
 * horizon; embargo > 0 moves a later fold's train_start past the previous test window; clip_horizon cuts the last test windows
 * to the data instead of dropping their folds.  Writes the first `capacity` folds to out_folds (may be NULL: count call) and
 * returns their number.  Host only: no device is touched.
 */
size_t anofox_hip_backtest_folds(int64_t n_dates,
                                 int64_t horizon,
                                 int64_t folds,
                                 int window_type,
                                 int64_t min_train_size,
                                 int64_t gap,
                                 int64_t embargo,
                                 int64_t initial_train_size,
                                 int64_t skip_length,
                                 bool clip_horizon,
                                 AnofoxHipFold *out_folds,
                                 size_t capacity);

/*
 * Sizes of the expanded block of `n_series` series under a fold table: pair p = s * n_folds + f is series s in fold index f,
 * *n_pairs = n_series * n_folds, *ld_pairs = n_pairs rounded up to 64 (at least 64), *t_train = the longest training window,
 * max_f(train_end_f - train_start_f + 1) (at least 1).  With this pair order the batch's series-major result [n_pairs x h] is, as
 * it lies, the series-major block [n_series x n_folds * h] that anofox_hip_conformal_learn_device and anofox_hip_metrics_device
 * (stride_s = n_folds * h, stride_t = 1) take with one group per series.  Fails with INVALID_INPUT when a position is negative or
 * n_pairs exceeds 2^31 - 1.  The expanded block costs t_train * ld_pairs * 8 bytes.  Host only.
 */
bool anofox_hip_backtest_sizes(const AnofoxHipFold *folds,
                               size_t n_folds,
                               size_t n_series,
                               size_t *t_train,
                               size_t *n_pairs,
                               size_t *ld_pairs,
                               struct AnofoxError *out_error);

/*
 * Cuts every fold's training window out of a device-resident time-major block y[t * ld_src + s] (fp64, t < t_rows; the block holds
 * no NULLs, as for anofox_hip_batch_set_device_block; lengths int32 [n_series], cut to t_rows): `folds` is a HOST array, t_train and
 * ld_pairs are what anofox_hip_backtest_sizes returns (t_train may be larger).  A pair is live exactly when the operator keeps it
 * (:785-790): train_end < len, test_start < len and train_start <= train_end (and test_start <= test_end).  For a live pair rows t < L = train_end - train_start
 * + 1 of column p of y_out [t_train x ld_pairs] are y[(train_start + t) * ld_src + s], len_pairs[p] = L and n_test[p] =
 * min(test_end, len - 1) - test_start + 1.  EVERYTHING else in y_out is 0.0 and both counts are 0: rows past L, dead pairs, the
 * padding columns p >= n_pairs (len_pairs and n_test are int32 [ld_pairs]).  y_out and len_pairs are what
 * anofox_hip_batch_create(n_pairs, t_train, ...) + anofox_hip_batch_set_device_block take: a dead pair is a series of length 0
 * there (INSUFFICIENT_DATA).  No exogenous regressors; not sharded over devices.  Runs on `stream` (NULL: the null stream) on the
 * calling thread's current device and returns after it has finished.
 */
bool anofox_hip_backtest_expand_device(const double *y,
                                       size_t ld_src,
                                       const int32_t *lengths,
                                       size_t n_series,
                                       size_t t_rows,
                                       const AnofoxHipFold *folds,
                                       size_t n_folds,
                                       size_t t_train,
                                       double *y_out,
                                       size_t ld_pairs,
                                       int32_t *len_pairs,
                                       int32_t *n_test,
                                       void *stream,
                                       struct AnofoxError *out_error);

/*
 * After the batch has run: matches forecasts to test rows and scores the folds.  n_test is the expand entry's; status, yhat, lower,
 * upper are the batch's device results (anofox_hip_batch_device_results: int32 [n_pairs], fp64 [n_pairs x horizon] series-major;
 * lower and upper may be NULL, the coverage score is then NaN).  Row i of pair p exists when the pair is live, status[p] == 0 and
 * i < n_test[p].  For an existing row actual = y[(test_start + i) * ld_src + s], error = yhat - actual, abs_error = |error|; every
 * row that does not exist is NaN in all three blocks ([n_pairs x horizon]; the row filter of anofox_hip_metrics_device is
 * drop_nan) and 0 in `valid` (uint8 [n_pairs x horizon], may be NULL: the mask anofox_hip_conformal_learn_device takes);
 * n_rows[p] (int32 [n_pairs]) counts the existing rows.  scores (fp64 [n_folds], may be NULL) receives ComputeMetric (:280-373)
 * of `metric` -- "mae", "mse", "mape", "smape", "bias", "r2", "coverage", "rmse"; every other name is rmse -- per fold over its
 * existing rows in the operator's row order (series, then steps), every sum sequential in that order: the bits of the host
 * route.  A fold without a row scores NaN.  horizon >= 1.  Runs on `stream` and returns after it has finished.
 */
bool anofox_hip_backtest_collect_device(const double *y,
                                        size_t ld_src,
                                        size_t n_series,
                                        size_t t_rows,
                                        const AnofoxHipFold *folds,
                                        size_t n_folds,
                                        const int32_t *n_test,
                                        const int32_t *status,
                                        const double *yhat,
                                        const double *lower,
                                        const double *upper,
                                        size_t horizon,
                                        const char *metric,
                                        double *actual,
                                        double *error,
                                        double *abs_error,
                                        uint8_t *valid,
                                        int32_t *n_rows,
                                        double *scores,
                                        void *stream,
                                        struct AnofoxError *out_error);

/*
 * The whole backtest of `n_series` series held on the host (values[i] points to lengths[i] values, sorted by date, no NULLs: the
 * operator drops NULL rows at :534) -- what _ts_backtest_native's finalize would call instead of its serial loop over (fold, group)
 * (:873-880): pack the block, expand, ONE batch run of the n_series * n_folds pairs, collect, one copy back.  Outputs, pair p =
 * s * n_folds + f: out_n_rows and out_status int32 [n_pairs] (status: the ErrorCode of the pair's fit; a dead pair is
 * INSUFFICIENT_DATA with 0 rows), out_model_names char [n_pairs][64] (anofox_hip_batch_model_name; empty unless status is 0),
 * out_yhat, out_lower, out_upper, out_actual fp64 [n_pairs x horizon] (rows i >= out_n_rows[p]: actual is NaN), out_scores fp64
 * [n_folds].  Any output may be NULL.  An option block that anofox_hip_batch_create refuses (e.g. a "Method:model" string:
 * INVALID_MODEL) fails the call with that error and produces no row, as the host route does.  Limits: n_pairs <= 2^31 - 1; the
 * expanded block costs t_train * ld_pairs * 8 bytes of device memory (a failed allocation is a COMPUTATION_ERROR that names the
 * size); no exogenous regressors; runs on the calling thread's current device (anofox_hip_set_devices does not shard it).
 */
bool anofox_hip_backtest_batch(const double *const *values,
                               const size_t *lengths,
                               size_t n_series,
                               const struct ForecastOptions *options,
                               const AnofoxHipFold *folds,
                               size_t n_folds,
                               const char *metric,
                               int32_t *out_n_rows,
                               int32_t *out_status,
                               char (*out_model_names)[64],
                               double *out_yhat,
                               double *out_lower,
                               double *out_upper,
                               double *out_actual,
                               double *out_scores,
                               struct AnofoxError *out_batch_error);

/* ------------------------------------------------------------------------- */
/* Block 6: ts_aggregate_hierarchy on the device                               */
/* ------------------------------------------------------------------------- */
/*
 * The operator (ts_aggregate_hierarchy.cpp:246-386) adds every row's value to one cell (unique_id, date) per level in the order the
 * rows arrive: a cell is ((0.0 + v_a) + v_b) + ... over its rows in table order, and exists only if a row reached it.  These entries
 * restate that on a time-major block: series s holds consecutive positions first[s] .. first[s] + lengths[s] - 1 of a common date
 * grid, and output column c is the sum over members[col_offsets[c] .. col_offsets[c + 1]) IN THAT ORDER (a series listed twice is
 * added twice, one after the other).  The contract is equality of bits with that chain: additions only, from +0.0 (so -0.0 never
 * comes out), no level built from another level's sums.  The groupings are arbitrary, not only key prefixes.
 */
enum { ANOFOX_HIERARCHY_ROUTE_AUTO = 0, ANOFOX_HIERARCHY_ROUTE_LANE = 1, ANOFOX_HIERARCHY_ROUTE_TILE = 2 };
typedef struct AnofoxHipHierarchyOptions {
    int32_t route;               /* 0: by member count; 1: lane per output column; 2: LDS tiles, one wavefront per (column, 64 rows).  Same bits. */
    int32_t tile_min_members;    /* route 0: columns with at least this many members take the tile route; 0: the built-in default (64) */
    int32_t reserved[2];         /* 0 */
} AnofoxHipHierarchyOptions;

/*
 * The CSR plan of a table of groupings.  column_of int32 [n_groupings x n_series]: column_of[g * n_series + s] is the output column
 * of series s under grouping g, -1 for none.  *n_out = the largest column + 1; *nnz = the entries that are not -1; col_offsets int32
 * [n_out + 1]; members int32 [nnz], within a column ordered by (series, grouping) -- the order in which the operator's rows (a row,
 * then its levels) reach the cell; a stable counting sort.  A column nobody maps to is empty.  col_offsets and members may both be
 * NULL: the sizing call.  INVALID_INPUT: an entry below -1, n_out or nnz above 2^31 - 1, n_series above 2^31 - 1.  Host only.
 */
bool anofox_hip_hierarchy_plan(const int32_t *column_of,
                               size_t n_groupings,
                               size_t n_series,
                               size_t *n_out,
                               size_t *nnz,
                               int32_t *col_offsets,
                               int32_t *members,
                               struct AnofoxError *out_error);

/*
 * Aggregates a device-resident block y[t * ld + s] (fp64, t < t_rows, left-aligned with lengths int32 [n_series], cut to t_rows).
 * first int64 [n_series]: the grid position of each series' row 0 (NULL: all 0; |first| <= 2^61).  valid / present uint8
 * [t_rows x ld], each may be NULL: valid 0 is a NULL value -- it counts as 0.0 and the row exists (:291); present 0 means there is
 * no row at that position -- it adds nothing and does not make the cell exist.  col_offsets, members: the plan, in device memory.
 *
 * Outputs, all in device memory: lengths_out int32 [n_out] and first_out int64 [n_out] -- a column spans the smallest to the largest
 * grid position at which a member has a row (length 0, first 0 when there is none); y_out [t_out x ld_out] time-major, left-aligned,
 * and present_out uint8 [t_out x ld_out] (may be NULL): 0 and 0.0 where no member has a row inside the span, and in rows
 * lengths_out[c] .. t_out - 1.  ld_out >= n_out (n_out rounded up to 64 is what the batch layer takes); columns >= n_out are not
 * touched; rows >= t_out of a longer column are not written (lengths_out says so).  t_out = 0 (or y_out NULL) writes only
 * lengths_out and first_out: the sizing call, as in anofox_hip_prepare_device.  y_out and lengths_out are what
 * anofox_hip_batch_set_device_block takes when no column has a hole.
 *
 * The call only enqueues on `stream` (NULL: the null stream) and does NOT wait on the host.  What only the device can see is
 * therefore reported in lengths_out: a column whose offsets leave the plan, that has a member outside [0, n_series) or a |first|
 * above 2^61, or whose span exceeds 2^30 rows has length -1 and is written as an empty column -- never a cut sum.
 * INVALID_INPUT on the host: struct_size, an unknown route, ld < n_series, ld_out < n_out, n_out / nnz / n_series above 2^31 - 1,
 * t_rows or t_out above 2^30.
 */
bool anofox_hip_hierarchy_device(const double *y,
                                 const uint8_t *valid,
                                 const uint8_t *present,
                                 size_t ld,
                                 const int32_t *lengths,
                                 const int64_t *first,
                                 size_t n_series,
                                 size_t t_rows,
                                 const int32_t *col_offsets,
                                 const int32_t *members,
                                 size_t n_out,
                                 size_t nnz,
                                 const AnofoxHipHierarchyOptions *options,
                                 size_t struct_size,
                                 size_t t_out,
                                 double *y_out,
                                 uint8_t *present_out,
                                 size_t ld_out,
                                 int32_t *lengths_out,
                                 int64_t *first_out,
                                 void *stream,
                                 struct AnofoxError *out_error);

/*
 * The same for series held on the host -- what the operator's finalize would call instead of its map of maps: values[s] points to
 * lengths[s] values at grid positions first[s] + t (first may be NULL); validity[s] / present[s] are bit masks in DuckDB's layout
 * (bit t % 64 of word t / 64; 1 = valid / there is a row), each array and each entry may be NULL (= all ones).  column_of as for
 * anofox_hip_hierarchy_plan.  The call plans, sizes on the host, uploads, runs and reads back once.
 *
 * *out_n_out, *out_t_out (the longest column, at least 1) and *out_ld (n_out rounded up to 64, at least 64) are always written.
 * With out_y NULL that is all: the sizing call, which needs no device.  Otherwise t_out and ld_out must be what the sizing call
 * returned and the caller's arrays receive out_y fp64 [t_out x ld_out] and out_present uint8 [t_out x ld_out] (time-major, as on the
 * device; may be NULL), out_lengths int32 [n_out], out_first int64 [n_out].
 *
 * INVALID_INPUT, each naming its limit: n_out or nnz above 2^31 - 1, a column_of entry below -1, a series longer than 2^30 rows, a
 * |first| above 2^61, a column whose span exceeds 2^30 rows.  A failed device allocation is a COMPUTATION_ERROR that names the
 * size.  One device (the calling thread's current one); fp64 only.
 */
bool anofox_hip_hierarchy_batch(const double *const *values,
                                const uint64_t *const *validity,
                                const uint64_t *const *present,
                                const size_t *lengths,
                                const int64_t *first,
                                size_t n_series,
                                const int32_t *column_of,
                                size_t n_groupings,
                                const AnofoxHipHierarchyOptions *options,
                                size_t struct_size,
                                size_t t_out,
                                size_t ld_out,
                                double *out_y,
                                uint8_t *out_present,
                                int32_t *out_lengths,
                                int64_t *out_first,
                                size_t *out_n_out,
                                size_t *out_t_out,
                                size_t *out_ld,
                                struct AnofoxError *out_error);

/* ------------------------------------------------------------------------- */
/* Block 7: reconciliation of the forecasts of a hierarchy                     */
/* ------------------------------------------------------------------------- */
/*
 * The forecasts of the columns that anofox_hip_hierarchy_device builds do not add up; these entries make them coherent.  The
 * reference has no such function: the contract is the published method (Hyndman et al. 2011, OLS; Wickramasuriya et al. 2019, MinT
 * with a diagonal W) in its constraint form.  A plan is col_offsets / members as anofox_hip_hierarchy_plan returns them.  The BOTTOM
 * column of series s is the one column whose member list is exactly [s]; every other column with members is an AGGREGATE; a column
 * without members is copied through and takes no part.  A[i][s] = how often s occurs among the members of aggregate i (a series
 * listed twice counts twice), w > 0 one weight per column.  For one row of base forecasts yhat:
 *   1. r_i = yhat_i - (((0.0 + yhat_b(m0)) + yhat_b(m1)) + ...) over the members of i in plan order;
 *   2. M = diag(w_a) + A diag(w_b) A^T (n_agg x n_agg, symmetric positive definite), lambda = M^-1 r by Cholesky;
 *   3. btilde_s = yhat_b(s) + w_b(s) * (((0.0 + lambda_i0) + lambda_i1) + ...) over the aggregates that hold s, ascending, once per
 *      occurrence;
 *   4. the bottom columns receive btilde, aggregate column i the chain ((0.0 + btilde(m0)) + btilde(m1)) + ... in plan order.
 * Step 4 makes the output coherent to the bit: every aggregate is what anofox_hip_hierarchy_device computes from the bottoms.
 */
enum { ANOFOX_RECONCILE_BOTTOM_UP = 0,      /* lambda = 0: the bottoms keep their bits, no factor */
       ANOFOX_RECONCILE_OLS = 1,            /* w = 1 */
       ANOFOX_RECONCILE_WLS_STRUCT = 2,     /* w_c = the member entries of column c (struct_weights of the plan) */
       ANOFOX_RECONCILE_WLS_VAR = 3 };      /* the caller's weights, e.g. a per-column error variance */

/*
 * The reconciliation plan of an aggregation plan.  Host only.  *n_agg and *n_leaf (the entries of leaf_aggs: the member entries of
 * all aggregates) are always written; with bottom_col NULL that is all (the sizing call; then every output array must be NULL).
 * Otherwise: bottom_col int32 [n_series]; agg_cols int32 [n_agg] ascending; leaf_offsets int32 [n_series + 1] and leaf_aggs int32
 * [n_leaf], the transposed plan: for series s the indices into agg_cols of the aggregates that hold it, ascending, once per
 * occurrence; struct_weights fp64 [n_out]: the member entries of each column (may be NULL).
 * INVALID_INPUT, each naming what it found: a member outside [0, n_series), a series without a bottom column, a series with two,
 * offsets that do not ascend from 0, n_agg above ANOFOX_HIP_RECONCILE_MAX_AGG.
 */
bool anofox_hip_reconcile_plan(const int32_t *col_offsets,
                               const int32_t *members,
                               size_t n_out,
                               size_t n_series,
                               size_t *n_agg,
                               size_t *n_leaf,
                               int32_t *bottom_col,
                               int32_t *agg_cols,
                               int32_t *leaf_offsets,
                               int32_t *leaf_aggs,
                               double *struct_weights,
                               struct AnofoxError *out_error);

/*
 * The Cholesky factor L (lower) of M for method 1, 2 or 3, into factor fp64 [n_agg x ld_a], ld_a >= n_agg.  All arrays in device
 * memory; nnz = col_offsets[n_out], n_leaf as the planner returned it.  weights fp64 [n_out]: NULL for method 1, the planner's
 * struct_weights for method 2, the caller's for method 3.  Only the lower triangle is written: the strict upper part and the
 * columns from n_agg on keep what they held.  The call returns after the factor is finished.  A factor is a value: one factor
 * serves every block of the same plan and weights.  Every sum has a fixed order; the same inputs give the same bits.
 * INVALID_INPUT: an unknown method or method 0, ld_a < n_agg, n_agg above the limit, a weight of a column with members that is not
 * finite and positive (names the column).  COMPUTATION_ERROR: a pivot that is not positive (names the row).
 */
bool anofox_hip_reconcile_factor_device(const int32_t *col_offsets,
                                        const int32_t *members,
                                        size_t n_out,
                                        size_t nnz,
                                        size_t n_series,
                                        const int32_t *bottom_col,
                                        const int32_t *agg_cols,
                                        size_t n_agg,
                                        const int32_t *leaf_offsets,
                                        const int32_t *leaf_aggs,
                                        size_t n_leaf,
                                        int32_t method,
                                        const double *weights,
                                        double *factor,
                                        size_t ld_a,
                                        void *stream,
                                        struct AnofoxError *out_error);

/*
 * Reconciles n_rows rows of a device-resident block: element (column c, row t) of base and of out lies at c * stride_s + t *
 * stride_t, as anofox_hip_metrics_device takes its blocks -- a time-major block (stride_s 1, stride_t ld) and the series-major
 * [n_out x h] layout of anofox_hip_batch_device_results (stride_s h, stride_t 1) give the same bits.  Only columns < n_out and rows
 * < n_rows of out are written; base may not alias out.  factor / ld_a from anofox_hip_reconcile_factor_device and weights as given
 * there (both NULL for method 0); work fp64 [n_rows x n_agg] is the caller's scratch (NULL for method 0 or n_agg 0).
 * row_status int32 [n_rows]: 0 done; 2 a base forecast that is not finite in a column with members -- every bottom and aggregate
 * column of that row is NaN then, never a silent answer; the other rows are not affected.  An empty column is copied, whatever it
 * holds.  The call only enqueues on `stream` and does not wait on the host.
 * INVALID_INPUT: an unknown method, a factor missing for method 1-3, ld_a < n_agg, n_agg above the limit, sizes above 2^31 - 1.
 */
bool anofox_hip_reconcile_apply_device(const double *base,
                                       size_t stride_s,
                                       size_t stride_t,
                                       size_t n_rows,
                                       const int32_t *col_offsets,
                                       const int32_t *members,
                                       size_t n_out,
                                       size_t nnz,
                                       size_t n_series,
                                       const int32_t *bottom_col,
                                       const int32_t *agg_cols,
                                       size_t n_agg,
                                       const int32_t *leaf_offsets,
                                       const int32_t *leaf_aggs,
                                       size_t n_leaf,
                                       int32_t method,
                                       const double *weights,
                                       const double *factor,
                                       size_t ld_a,
                                       double *work,
                                       double *out,
                                       int32_t *row_status,
                                       void *stream,
                                       struct AnofoxError *out_error);

/*
 * The same for host buffers: column_of as for anofox_hip_hierarchy_plan, forecast and out fp64 series-major [n_out x h] (n_out as
 * that plan sizes it), weights fp64 [n_out] for method 3 (ignored otherwise; method 2 takes the plan's), out_row_status int32 [h].
 * The call plans, uploads, factors, applies and reads back once.  The planner's errors come first and need no device.  A failed
 * device allocation is a COMPUTATION_ERROR that names the size.  One device; fp64 only.
 */
bool anofox_hip_reconcile_batch(const int32_t *column_of,
                                size_t n_groupings,
                                size_t n_series,
                                const double *forecast,
                                size_t h,
                                int32_t method,
                                const double *weights,
                                double *out,
                                int32_t *out_row_status,
                                struct AnofoxError *out_error);

/*
 * MinT with the shrinkage covariance estimator (Wickramasuriya et al. 2019; Schaefer and Strimmer 2005), in the same constraint form.
 * These are entries of their own: the method enum above is not extended.  The residual block holds n_res rows of base-forecast
 * errors for every column of the plan, element (column c, row t) at c * res_stride_s + t * res_stride_t in both layouts that
 * anofox_hip_metrics_device takes (the `error` block of anofox_hip_backtest is series-major: res_stride_s = its row length,
 * res_stride_t = 1).  P = every bottom and every aggregate column, n_p = n_series + n_agg; an empty column is never read.
 *   1. v_c = ((((0.0 + x_0c^2) + x_1c^2) + ...) / n_res) for c in P: serial in row order, no fused multiply-add, no centring (the
 *      shrink.estim of the hts package).  Contract: equality of bits with that restatement.
 *   2. xs_tc = x_tc * (1 / sqrt(v_c)), G = Xs Xs^T (n_res x n_res, inner dimension over P: the bottoms in series order, then the
 *      aggregates), fro = sum G_tu^2, q = sum G_tt^2, f4 = sum xs_tc^4, each in one fixed order.
 *   3. T = n_res; sum_v = ((q - f4) - (fro - n_p T^2) / T) / (T (T - 1)); sum_d = fro / T^2 - n_p; shrinkage = min(max(sum_v / sum_d,
 *      0), 1), and 1 when sum_d is not finite and positive.  These are the sums of shrink.estim over all n_p^2 pairs of columns; no
 *      array of size n_p x n_p is formed.  A caller may pass its own intensity in [0, 1]; steps 2 and 3 are skipped then.
 *   4. E[t][i] = x_t,agg(i) - (((0.0 + x_t,b(m0)) + x_t,b(m1)) + ...): the residuals' own incoherence.
 *   5. M = shrinkage (diag(v_a) + A diag(v_b) A^T) + ((1 - shrinkage) / n_res) E^T E; every element takes its t terms in ascending
 *      order (fused multiply-adds); M = L L^T by the factor kernels of anofox_hip_reconcile_factor_device.
 *   6. For a forecast row: r and mu = M^-1 r as above; g_t = sum_i E[t][i] mu_i; btilde_s = (yhat_b(s) + (shrinkage v_b(s)) *
 *      chain(mu over the aggregates that hold s)) - ((1 - shrinkage) / n_res) * sum_t x_t,b(s) g_t.  Both sums are chains of fused
 *      multiply-adds from 0.0 in ascending index order.
 *   7. As step 4 above: the aggregates are the chain over the output's own bottoms, the output is coherent to the bit; empty columns
 *      are copied; row_status as anofox_hip_reconcile_apply_device.
 * No floating-point atomics: the same bits on every run, through every entry, in both layouts of the forecast block and both
 * layouts of the residual block.  With shrinkage 1 the result is that of method 3 with the variances as weights.
 *
 * The element counts (doubles) of what the caller of the device entries allocates.  Host only.  gram_elems: the workspace of the
 * estimate (a function of n_res alone; not needed when an intensity is passed in); e_elems = n_res * n_agg; factor_elems = n_agg *
 * n_agg; work_elems = n_rows * (n_agg + n_res), the work area of the apply.
 * INVALID_INPUT: n_res < 2 or above ANOFOX_HIP_RECONCILE_MAX_RESIDUAL_ROWS, n_agg above ANOFOX_HIP_RECONCILE_MAX_AGG.
 */
bool anofox_hip_reconcile_mint_sizes(size_t n_res,
                                     size_t n_agg,
                                     size_t n_rows,
                                     size_t *gram_elems,
                                     size_t *e_elems,
                                     size_t *factor_elems,
                                     size_t *work_elems,
                                     struct AnofoxError *out_error);

/*
 * Steps 1 to 5.  All arrays in device memory; the plan arrays as for anofox_hip_reconcile_factor_device.  shrinkage: NaN asks for the
 * estimate, a value in [0, 1] is taken as it is.  Outputs: variances fp64 [n_out] (0.0 in an empty column); e fp64 [n_res x ld_e],
 * ld_e >= n_agg -- a value the caller keeps beside the factor; factor fp64 [n_agg x ld_a]: only the lower triangle is written, and
 * only the first n_agg columns of e; *out_shrinkage (host memory) the intensity used.  gram_work fp64 [gram_elems] is scratch (may
 * be NULL when an intensity is passed in).  The call returns after everything is finished.
 * INVALID_INPUT: n_res outside [2, ANOFOX_HIP_RECONCILE_MAX_RESIDUAL_ROWS], an intensity outside [0, 1], ld_e or ld_a < n_agg, the
 * plan and size limits of the entries above.  COMPUTATION_ERROR, each naming the column or row: a residual of a participating
 * column that is not finite; a participating column whose variance is not finite and positive; a pivot that is not positive
 * (reachable with shrinkage 0 and n_res < n_agg).
 */
bool anofox_hip_reconcile_mint_factor_device(const double *residuals,
                                             size_t res_stride_s,
                                             size_t res_stride_t,
                                             size_t n_res,
                                             const int32_t *col_offsets,
                                             const int32_t *members,
                                             size_t n_out,
                                             size_t nnz,
                                             size_t n_series,
                                             const int32_t *bottom_col,
                                             const int32_t *agg_cols,
                                             size_t n_agg,
                                             const int32_t *leaf_offsets,
                                             const int32_t *leaf_aggs,
                                             size_t n_leaf,
                                             double shrinkage,
                                             double *variances,
                                             double *e,
                                             size_t ld_e,
                                             double *factor,
                                             size_t ld_a,
                                             double *gram_work,
                                             double *out_shrinkage,
                                             void *stream,
                                             struct AnofoxError *out_error);

/*
 * Steps 6 and 7 for n_rows rows of a device-resident forecast block (base, out, strides, row_status as for
 * anofox_hip_reconcile_apply_device).  residuals, variances, e, shrinkage and factor as the factor call took and returned them;
 * work fp64 [n_rows x (n_agg + n_res)] is the caller's scratch (NULL without aggregates).  The call only enqueues on `stream`.
 * INVALID_INPUT: as above, a NaN intensity, a factor missing.
 */
bool anofox_hip_reconcile_mint_apply_device(const double *base,
                                            size_t stride_s,
                                            size_t stride_t,
                                            size_t n_rows,
                                            const double *residuals,
                                            size_t res_stride_s,
                                            size_t res_stride_t,
                                            size_t n_res,
                                            const int32_t *col_offsets,
                                            const int32_t *members,
                                            size_t n_out,
                                            size_t nnz,
                                            size_t n_series,
                                            const int32_t *bottom_col,
                                            const int32_t *agg_cols,
                                            size_t n_agg,
                                            const int32_t *leaf_offsets,
                                            const int32_t *leaf_aggs,
                                            size_t n_leaf,
                                            const double *variances,
                                            const double *e,
                                            size_t ld_e,
                                            double shrinkage,
                                            const double *factor,
                                            size_t ld_a,
                                            double *work,
                                            double *out,
                                            int32_t *row_status,
                                            void *stream,
                                            struct AnofoxError *out_error);

/*
 * The same for host buffers: column_of as for anofox_hip_hierarchy_plan, forecast and out fp64 series-major [n_out x h], residuals
 * fp64 series-major [n_out x n_res], *shrinkage NaN (estimate) or a value in [0, 1] on entry and the intensity used on return,
 * out_row_status int32 [h], out_variances fp64 [n_out] (may be NULL).  The call plans, uploads, factors, applies and reads back
 * once.  The planner's errors and the limits come first and need no device.  A failed device allocation is a COMPUTATION_ERROR that
 * names the size.  One device; fp64 only.
 */
bool anofox_hip_reconcile_mint_batch(const int32_t *column_of,
                                     size_t n_groupings,
                                     size_t n_series,
                                     const double *forecast,
                                     size_t h,
                                     const double *residuals,
                                     size_t n_res,
                                     double *shrinkage,
                                     double *out,
                                     int32_t *out_row_status,
                                     double *out_variances,
                                     struct AnofoxError *out_error);

/* ------------------------------------------------------------------------- */
/* Block 8: the choice of a forecast method per series from backtest scores    */
/* ------------------------------------------------------------------------- */
/*
 * fit -> forecast -> backtest -> score -> CHOOSE -> calibrate.  The reference compares models with one backtest statement per
 * method and an AVG per model; it has no operator that chooses per series, so the names and the contract are this package's
 * (DESIGN.md section 3 "Selection"): every result equals a serial restatement bit for bit, and no new floating-point sum is
 * formed except the combine sums, whose order is the method order.  At most ANOFOX_HIP_SELECT_MAX_METHODS methods per call: more
 * fail with INVALID_INPUT naming the limit.  Scope: no exogenous regressors, no NULLs in the block, fp64, one device (the calling
 * thread's current device; anofox_hip_set_devices does not shard these entries).
 */
#define ANOFOX_HIP_SELECT_MAX_METHODS 16
enum { ANOFOX_SELECT_PICK = 0,              /* every series takes the forecast of its winner */
       ANOFOX_SELECT_MEAN = 1,              /* the live members added in method order from 0.0, divided by their number */
       ANOFOX_SELECT_MEDIAN = 2,            /* the middle live value; of an even number (a + b) * 0.5 of the two middle ones */
       ANOFOX_SELECT_INVERSE_SCORE = 3 };   /* sum(w y) / sum(w) with w = 1.0 / score, both sums in method order */

/*
 * The winner of every series and the stable partition of the series by winner.  scores is fp64 [n_methods x ld] (method m of
 * series s at m * ld + s: one figure row of anofox_hip_metrics_device per method), score_status int32 [n_methods x n_series].
 * Method m is admissible for series s when its status is 0 and its score is not NaN; +-inf are ordinary values.  The winner is the
 * admissible method with the smallest score, the lowest m among equals (-0.0 and +0.0 are equal); without an admissible method it
 * is `fallback`, an index in [-1, n_methods) (-1: none).  winner int32 [n_series]; best_score fp64 [n_series], NaN when the winner
 * came from the fallback or is -1; from_fallback uint8 [n_series].  offsets int32 [n_methods + 1] and members int32 [n_series]:
 * members[offsets[m] .. offsets[m + 1]) are the series method m won, ascending; only the first offsets[n_methods] entries of
 * members are written, a series with winner -1 appears nowhere.  Everything stays on the device: the caller reads the n_methods + 1
 * offsets.  Deterministic -- no atomic decides an order -- and correct for every n_series up to 2^31 - 1.  Runs on `stream` (NULL:
 * the null stream) and returns after it has finished.
 * INVALID_INPUT, each naming the offender: n_methods 0 or above the limit, fallback outside [-1, n_methods), ld < n_series.
 */
bool anofox_hip_select_winner_device(const double *scores,
                                     size_t ld,
                                     const int32_t *score_status,
                                     size_t n_methods,
                                     size_t n_series,
                                     int32_t fallback,
                                     int32_t *winner,
                                     double *best_score,
                                     uint8_t *from_fallback,
                                     int32_t *offsets,
                                     int32_t *members,
                                     void *stream,
                                     struct AnofoxError *out_error);

/*
 * The columns members[off .. off + n_m) of a time-major block y[t * ld_src + s] (t < t_rows, lengths int32 [n_series]) as a dense
 * block: y_out[t * ld_m + j] = y[t * ld_src + members[off + j]] and len_out[j] = the length of that series for j < n_m; columns
 * n_m <= j < ld_m are 0.0 with length 0 (y_out fp64 [t_rows x ld_m], len_out int32 [ld_m]).  With ld_m = n_m rounded up to 64 the
 * result is what anofox_hip_batch_create(n_m, t_rows, ...) + anofox_hip_batch_set_device_block take.  off and n_m are host values
 * (the caller has read offsets); a member outside [0, n_series) gives an empty column.  Returns after `stream` has finished.
 */
bool anofox_hip_select_gather_device(const double *y,
                                     size_t ld_src,
                                     const int32_t *lengths,
                                     size_t n_series,
                                     size_t t_rows,
                                     const int32_t *members,
                                     size_t off,
                                     size_t n_m,
                                     double *y_out,
                                     size_t ld_m,
                                     int32_t *len_out,
                                     void *stream,
                                     struct AnofoxError *out_error);

/*
 * The inverse for results: row j of the sub-batch's series-major yhat_m / lower_m / upper_m [n_m x horizon], code_m and status_m
 * [n_m] (anofox_hip_batch_device_results) goes to row members[off + j] of yhat / lower / upper [n_series x horizon], model_code
 * and status [n_series]; an output that is NULL is skipped.  With `winner` (int32 [n_series], may be NULL) the rows of every series
 * whose winner is -1 are written as well: NaN, model code 0, status INSUFFICIENT_DATA.  n_m may be 0.  Returns after `stream` has
 * finished.
 */
bool anofox_hip_select_scatter_device(const double *yhat_m,
                                      const double *lower_m,
                                      const double *upper_m,
                                      const int32_t *code_m,
                                      const int32_t *status_m,
                                      const int32_t *members,
                                      size_t off,
                                      size_t n_m,
                                      size_t horizon,
                                      const int32_t *winner,
                                      size_t n_series,
                                      double *yhat,
                                      double *lower,
                                      double *upper,
                                      int32_t *model_code,
                                      int32_t *status,
                                      void *stream,
                                      struct AnofoxError *out_error);

/*
 * Combines n_methods device blocks [n_rows x horizon] (row r, step i at r * horizon + i; `blocks` is a HOST array of the device
 * pointers) cell by cell into out [n_rows x horizon].  Row r belongs to group r / group_div: 1 for final forecasts, the number of
 * folds for the [n_pairs x horizon] backtest blocks.  member_status is int32 [n_methods x n_rows]; member m is live in a cell when
 * member_status[m * n_rows + r] is 0 and its value there is not NaN.
 *   mode 0: out = blocks[winner[g]] (winner int32 [groups]; -1: NaN) -- plain indexing, member_status is not consulted;
 *   mode 1: ((0.0 + y_m0) + y_m1) + ... over the live members in method order, divided by their number;
 *   mode 2: the live values sorted in the total order of their bit patterns (-0.0 below +0.0): the middle one, or (a + b) * 0.5;
 *   mode 3: weights fp64 [n_methods x ld_w] holds the SCORES (method m of group g at m * ld_w + g).  A live member whose score is
 *           not NaN takes part with w = 1.0 / score: out = (((0.0 + w0 * y0) + w1 * y1) + ...) / ((0.0 + w0) + w1 + ...), every
 *           product rounded before it is added.  If a member that takes part has score 0.0 the cell is instead the plain mean
 *           (as mode 1) of exactly the members with score 0.0 -- the limit of the weighting.
 * A cell without a live member is NaN.  row_status int32 [n_rows] (may be NULL): 1 when every cell of the row is NaN, else 0.
 * Returns after `stream` has finished.  INVALID_INPUT: n_methods 0 or above the limit, an unknown mode, horizon 0, group_div 0,
 * ld_w smaller than the number of groups.
 */
bool anofox_hip_select_combine_device(const double *const *blocks,
                                      size_t n_methods,
                                      size_t n_rows,
                                      size_t horizon,
                                      const int32_t *member_status,
                                      int32_t mode,
                                      const int32_t *winner,
                                      const double *weights,
                                      size_t ld_w,
                                      size_t group_div,
                                      double *out,
                                      int32_t *row_status,
                                      void *stream,
                                      struct AnofoxError *out_error);

/*
 * The whole chain for host buffers.  values[i] / lengths[i] as for anofox_hip_backtest_batch; methods is a table of n_methods
 * option blocks that share one horizon >= 1; folds as for anofox_hip_backtest_batch; criterion is "mae", "mse", "rmse", "mape" or
 * "smape" (unlike the backtest's fold score, every other name is an error here); mode is "pick", "mean", "median" or
 * "inverse_score"; fallback in [-1, n_methods).  The call packs once and expands ONCE; every method runs one batch on the shared
 * expanded block and is scored per series over the existing rows of its n_folds * horizon backtest cells (the bits of
 * anofox_hip_metrics_device with drop_nan).  "pick" then chooses, partitions, gathers, runs one sub-batch per method that won
 * something and scatters; the other modes run every method on the whole block and combine (no combined intervals: out_lower and
 * out_upper are NaN then, and out_model_names holds the mode's name).  Outputs, any of which may be NULL: out_winner int32 [n],
 * out_best_score fp64 [n], out_scores fp64 [n_methods x n] (method m of series s at m * n + s), out_yhat / out_lower / out_upper
 * fp64 [n x horizon], out_status int32 [n] (0, the sub-batch's status, or INSUFFICIENT_DATA where nothing was chosen or no member
 * gave a forecast), out_model_names char [n][64] (empty unless the status is 0), out_backtest_yhat / out_backtest_actual fp64
 * [n_pairs x horizon] -- the picked or combined backtest forecasts and their test values, NaN where a row does not exist, in
 * the pair order of anofox_hip_backtest_sizes -- and out_n_rows int32 [n_pairs], the cells of a pair that hold both.
 * An option block that anofox_hip_batch_create refuses fails the whole call with that error.  INVALID_INPUT, each naming the
 * offender: n_methods 0 or above the limit, methods of different horizons, a horizon below 1, an unknown criterion or mode, a
 * fallback out of range.  All argument errors come before the device is touched.
 */
bool anofox_hip_select_batch(const double *const *values,
                             const size_t *lengths,
                             size_t n_series,
                             const ForecastOptions *methods,
                             size_t n_methods,
                             const AnofoxHipFold *folds,
                             size_t n_folds,
                             const char *criterion,
                             const char *mode,
                             int32_t fallback,
                             int32_t *out_winner,
                             double *out_best_score,
                             double *out_scores,
                             double *out_yhat,
                             double *out_lower,
                             double *out_upper,
                             int32_t *out_status,
                             char (*out_model_names)[64],
                             double *out_backtest_yhat,
                             double *out_backtest_actual,
                             int32_t *out_n_rows,
                             struct AnofoxError *out_batch_error);

/* ------------------------------------------------------------------------- */
/* Block 9: bootstrap sample paths and their quantiles                         */
/* ------------------------------------------------------------------------- */
/*
 * Residual bootstrap with cumulative resampling, per series or jointly across series (Panagiotelis et al. 2023), and the quantiles
 * of a block of paths.  The names are this package's own; tests/paths_ref.py is the definition, bit for bit:
 *   - the draw of series s, path p, step k is output word k & 3 of Philox4x32-10 with counter {p, joint ? 0 : s, k >> 2, joint ? 1 : 0}
 *     and key {seed & 0xffffffff, seed >> 32}; the pool row is j = (u * n) >> 32 on 64-bit integers, n the pool length of the
 *     series (joint: pool_rows -- every series of a path takes the same row at a step); no rejection step, bias at most n / 2^32;
 *   - cumulative: acc = acc + e[j_k] from 0.0, path[k] = point[k] + acc; independent: path[k] = point[k] + e[j_k]; plain fp64
 *     additions in step order;
 *   - level q of n_paths values sorted by the total-order key (-0.0 below +0.0): s[lo] * (1 - frac) + s[up] * frac at index
 *     q * (n_paths - 1); q <= 0 the first value, q >= 1 the last.
 * Status per series (int32): 0 done; 1 empty pool; 2 a NaN among the pool's first `length` rows or in the point row; 3 joint mode
 * and a pool length other than pool_rows (in that order of precedence: 3, 1, 2).  Paths of a series whose status is not 0 are NaN.
 * +-inf are ordinary values.  Status per column of the quantile entry: 0, or 2 when any of its paths is NaN -- every quantile of
 * that column is then NaN.
 */
#define ANOFOX_HIP_PATHS_MAX_PATHS 2048
#define ANOFOX_HIP_PATHS_MAX_LEVELS 16
#define ANOFOX_HIP_PATHS_MAX_POOL_ROWS 1048576
enum { ANOFOX_PATHS_CUMULATIVE = 0, ANOFOX_PATHS_INDEPENDENT = 1 };
enum { ANOFOX_PATHS_ROUTE_AUTO = 0, ANOFOX_PATHS_ROUTE_LANE = 1 };
typedef struct AnofoxHipPathsOptions {
    int32_t mode;                /* ANOFOX_PATHS_CUMULATIVE or ANOFOX_PATHS_INDEPENDENT */
    int32_t joint;               /* 0: every series draws its own rows; 1: one row per path and step for all series */
    int32_t route;               /* 0: automatic; 1: lanes over series (the one route there is) */
    int32_t reserved;            /* 0 */
    uint64_t seed;
} AnofoxHipPathsOptions;

/*
 * Sample paths of a device-resident block.  Element (series s, row t) of `point` [n_series x horizon] is at s * point_stride_s +
 * t * point_stride_t, of `pool` [n_series x pool_rows] at s * pool_stride_s + t * pool_stride_t: stride_s = 1 is a time-major block,
 * stride_t = 1 a series-major one (the batch results' yhat; the error block of a backtest viewed as [n_series x n_folds * horizon]).
 * pool_lengths int32 [n_series] in device memory, cut to [0, pool_rows]; NULL: every pool has pool_rows rows.
 * Outputs, in device memory: paths_out fp64 [n_paths * horizon x ld_out] time-major, row p * horizon + k of column s -- what
 * anofox_hip_hierarchy_device takes as it lies with t_rows = n_paths * horizon; columns >= n_series are not touched; status int32
 * [n_series].  The call only enqueues on `stream` (NULL: the null stream) and does NOT wait on the host.
 * INVALID_INPUT, each naming its limit, before the device is touched: struct_size, an unknown mode or route, n_paths 0 or above
 * 2,048, horizon 0, n_paths * horizon above 2^30, pool_rows above 2^20, ld_out < n_series.
 */
bool anofox_hip_paths_device(const double *point,
                             size_t point_stride_s,
                             size_t point_stride_t,
                             const double *pool,
                             size_t pool_stride_s,
                             size_t pool_stride_t,
                             const int32_t *pool_lengths,
                             size_t pool_rows,
                             size_t n_series,
                             size_t horizon,
                             size_t n_paths,
                             const AnofoxHipPathsOptions *options,
                             size_t struct_size,
                             double *paths_out,
                             size_t ld_out,
                             int32_t *status,
                             void *stream,
                             struct AnofoxError *out_error);

/*
 * Quantiles of a device-resident block of paths [n_paths * horizon x ld] as anofox_hip_paths_device or the hierarchy entry wrote
 * it.  levels fp64 [n_levels] on the HOST, each in [0, 1].  Outputs, in device memory: out fp64 [n_levels x n_cols x horizon] (level
 * l of column c at step k at (l * n_cols + c) * horizon + k), status int32 [n_cols].  The call only enqueues on `stream`.
 * INVALID_INPUT, each naming its limit: n_paths 0 or above 2,048, horizon 0, n_paths * horizon above 2^30, n_levels 0 or above 16,
 * a level outside [0, 1] or NaN, ld < n_cols.
 */
bool anofox_hip_path_quantiles_device(const double *paths,
                                      size_t ld,
                                      size_t n_cols,
                                      size_t horizon,
                                      size_t n_paths,
                                      const double *levels,
                                      size_t n_levels,
                                      double *out,
                                      int32_t *status,
                                      void *stream,
                                      struct AnofoxError *out_error);

/*
 * The chain for host buffers: points fp64 [n_series x horizon] series-major, pools[s] points to pool_lengths[s] residuals (NULL
 * only where the length is 0); pool_rows is the longest pool.  column_of / n_groupings as for anofox_hip_hierarchy_plan; NULL (or
 * 0 groupings): the leaves only.  The call packs once, generates the paths, aggregates them up the plan with
 * anofox_hip_hierarchy_device when there is one -- every cell of an aggregated path is the serial sum of its members' paths in
 * plan order -- and takes the quantiles of the leaf block or of the aggregated block.
 *
 * *out_n_out (n_series, or the plan's columns) and *out_ld (n_out rounded up to 64, at least 64) are always written.  With
 * out_quantiles NULL that is all: the sizing call, which needs no device.  Otherwise ld must be what the sizing call returned and
 * the caller's arrays receive out_quantiles fp64 [n_levels x n_out x horizon], out_status int32 [n_out] (per output column),
 * out_series_status int32 [n_series] (may be NULL) and out_paths fp64 [n_paths * horizon x ld] (may be NULL): the block the
 * quantiles were taken of.
 *
 * INVALID_INPUT as for the two device entries and for the plan, all before the device is touched.  A failed device allocation is
 * a COMPUTATION_ERROR that names the size.  One device (the calling thread's current one); fp64 only.
 */
bool anofox_hip_paths_batch(const double *points,
                            const double *const *pools,
                            const size_t *pool_lengths,
                            size_t n_series,
                            size_t horizon,
                            size_t n_paths,
                            const AnofoxHipPathsOptions *options,
                            size_t struct_size,
                            const double *levels,
                            size_t n_levels,
                            const int32_t *column_of,
                            size_t n_groupings,
                            size_t ld,
                            double *out_quantiles,
                            int32_t *out_status,
                            int32_t *out_series_status,
                            double *out_paths,
                            size_t *out_n_out,
                            size_t *out_ld,
                            struct AnofoxError *out_error);

/* ------------------------------------------------------------------------- */
/* Block 10: scores of sample paths: CRPS, pinball, ranks and energy score     */
/* ------------------------------------------------------------------------- */
/*
 * How good a block of sample paths is, judged against the actuals where the paths lie.  The names are this package's own;
 * tests/path_scores_ref.py is the definition, bit for bit.  Plain fp64, one rounding per operation, nothing fused.
 *   - the wave sum W(t_0 .. t_{n-1}), the one order of addition of every sum over paths or over columns: a_l is the serial sum from
 *     0.0 of t_i with i = l (mod 64), ascending in i (an empty class gives 0.0); W = ((a_0 + a_1) + a_2) + ... + a_63;
 *   - per (column c, step k), y = actual[c, k], x_(0) <= ... <= x_(P-1) the P = n_paths values sorted by the total-order key of the
 *     quantile entry (-0.0 below +0.0), d_i = x_(i) - y:
 *       crps  = W(|d_i|) / P - W((2i - P + 1) * d_i) / (P * P)       -- the sorted form of E|X - y| - 1/2 E|X - X'|; P = 1: |x - y|
 *       below = the paths with x < y, equal = the paths with x == y (IEEE comparisons): the rank of the actual, ties kept apart
 *       quantile l = what anofox_hip_path_quantiles_device returns, the same bits; its pinball term is tau * e if e >= 0.0 else
 *       (tau - 1.0) * e with e = y - quantile;
 *   - per column: crps_mean and pinball_l are the serial sums from 0.0 over the steps that have an actual, in step order, divided by
 *     their count n_steps.  A NaN actual drops the step: its crps is NaN, its below and equal are -1 (its quantiles are computed);
 *   - status per column (int32): 0 done; 1 no step with an actual -- every mean is NaN; 2 a NaN among the column's paths -- every
 *     figure of the column is NaN, below and equal are -1; 2 takes precedence.  +-inf are ordinary values;
 *   - the energy score of the columns [col_begin, col_end) at step k, consecutive paths as the independent copy (Panagiotelis et al.
 *     2023): D1[p] = sqrt(W_c((x[p,k,c] - y[k,c])^2)), D2[p] = sqrt(W_c((x[p,k,c] - x[p+1,k,c])^2)) for p < P - 1, the terms indexed by
 *     c - col_begin, each square one rounded product, sqrt correctly rounded; S1, S2 the serial sums over p from 0.0;
 *     es[k] = S1 / P - S2 / (2 * (P - 1)), for P = 1 es[k] = S1.  A NaN (a path or an actual of the range) propagates by arithmetic
 *     into es[k].  es_mean is the serial sum of the non-NaN es[k] in step order over their count es_steps; NaN when that is 0.
 * Element (column c, step k) of `actual` is at c * actual_stride_c + k * actual_stride_k: stride_c = 1 is a time-major [horizon x ld]
 * block (what anofox_hip_hierarchy_device writes for aggregated actuals), stride_k = 1 a series-major one (a backtest's actual block).
 */
enum { ANOFOX_PATH_SCORES_OK = 0, ANOFOX_PATH_SCORES_NO_ACTUAL = 1, ANOFOX_PATH_SCORES_NAN = 2 };

/*
 * Scores of a device-resident block of paths [n_paths * horizon x ld].  levels fp64 [n_levels] on the HOST, each in [0, 1];
 * n_levels may be 0 (levels may then be NULL).  Outputs, in device memory, each but `status` may be NULL and is then skipped:
 * out_crps fp64 [n_cols x horizon] (column c, step k at c * horizon + k), out_below and out_equal int32 [n_cols x horizon],
 * out_quantiles fp64 [n_levels x n_cols x horizon] as the quantile entry writes them, out_column fp64 [(2 + n_levels) x ld_out] in
 * the rows crps_mean, n_steps (as double), pinball_l (row r of column c at r * ld_out + c), status int32 [n_cols].  One sort per
 * (column, step) serves every output.  The call only enqueues on `stream` (NULL: the null stream) and does NOT wait on the host.
 * INVALID_INPUT, each naming its limit, before the device is touched: n_paths 0 or above 2,048, horizon 0, n_paths * horizon above
 * 2^30, n_levels above 16, a level outside [0, 1] or NaN, ld < n_cols, out_column with ld_out < n_cols.
 */
bool anofox_hip_path_scores_device(const double *paths,
                                   size_t ld,
                                   size_t n_cols,
                                   size_t horizon,
                                   size_t n_paths,
                                   const double *actual,
                                   size_t actual_stride_c,
                                   size_t actual_stride_k,
                                   const double *levels,
                                   size_t n_levels,
                                   double *out_crps,
                                   int32_t *out_below,
                                   int32_t *out_equal,
                                   double *out_quantiles,
                                   double *out_column,
                                   size_t ld_out,
                                   int32_t *status,
                                   void *stream,
                                   struct AnofoxError *out_error);

/*
 * The doubles of the energy entry's workspace (2 * n_paths * horizon).  Host only; the limits of n_paths and horizon as above.
 */
bool anofox_hip_path_scores_sizes(size_t horizon,
                                  size_t n_paths,
                                  size_t *out_workspace_doubles,
                                  struct AnofoxError *out_error);

/*
 * The energy score of the columns [col_begin, col_end) of a device-resident block of paths.  workspace fp64
 * [anofox_hip_path_scores_sizes] in device memory receives D1 [n_paths x horizon] and D2 [n_paths x horizon] (row p, step k at
 * p * horizon + k; D2 of the last path is 0).  Outputs, in device memory: out_es fp64 [horizon], out_summary fp64 [2]: es_mean and
 * es_steps.  The path block is streamed once; the call only enqueues on `stream`.
 * INVALID_INPUT, each naming its limit: the limits of n_paths and horizon, an empty or reversed range, a range beyond ld.
 */
bool anofox_hip_path_energy_device(const double *paths,
                                   size_t ld,
                                   size_t col_begin,
                                   size_t col_end,
                                   size_t horizon,
                                   size_t n_paths,
                                   const double *actual,
                                   size_t actual_stride_c,
                                   size_t actual_stride_k,
                                   double *workspace,
                                   double *out_es,
                                   double *out_summary,
                                   void *stream,
                                   struct AnofoxError *out_error);

/*
 * The chain for host buffers: what anofox_hip_paths_batch takes, plus actuals fp64 [n_series x horizon] series-major with NaN for a
 * row that does not exist.  The call packs once, generates the paths and aggregates paths AND actuals up the plan when there is
 * one -- the actual of an aggregate is the serial sum of its members' actuals by the same anofox_hip_hierarchy_device, so a member's
 * NaN drops the step of the aggregate --, scores every output column and takes the energy score of every grouping's column range
 * -- [the smallest column the grouping maps a series to, the largest + 1): a plan's columns lie grouping by grouping -- and of the
 * whole [0, n_out).
 *
 * *out_n_out and *out_ld as for anofox_hip_paths_batch, always written.  With out_status NULL that is all: the sizing call, which
 * needs no device.  Otherwise ld must be what the sizing call returned and the caller's arrays receive, each but out_status optional
 * (NULL): out_crps fp64 [n_out x horizon], out_below and out_equal int32 [n_out x horizon], out_quantiles fp64 [n_levels x n_out x
 * horizon], out_column fp64 [(2 + n_levels) x ld], out_status int32 [n_out], out_series_status int32 [n_series] (of the generating
 * entry), out_energy fp64 [(n_groupings + 1) x (horizon + 2)] -- per range es[0 .. horizon), es_mean, es_steps; the whole is the
 * last row; without a plan there is that row alone; a grouping that maps no series has NaN -- and out_ranges int32 [(n_groupings +
 * 1) x 2], the ranges themselves.
 *
 * INVALID_INPUT as for the device entries and for the plan, all before the device is touched.  A failed device allocation is a
 * COMPUTATION_ERROR that names the size.  One device (the calling thread's current one); fp64 only.
 */
bool anofox_hip_path_scores_batch(const double *points,
                                  const double *const *pools,
                                  const size_t *pool_lengths,
                                  size_t n_series,
                                  size_t horizon,
                                  size_t n_paths,
                                  const AnofoxHipPathsOptions *options,
                                  size_t struct_size,
                                  const double *levels,
                                  size_t n_levels,
                                  const int32_t *column_of,
                                  size_t n_groupings,
                                  const double *actuals,
                                  size_t ld,
                                  double *out_crps,
                                  int32_t *out_below,
                                  int32_t *out_equal,
                                  double *out_quantiles,
                                  double *out_column,
                                  int32_t *out_status,
                                  int32_t *out_series_status,
                                  double *out_energy,
                                  int32_t *out_ranges,
                                  size_t *out_n_out,
                                  size_t *out_ld,
                                  struct AnofoxError *out_error);

/* ------------------------------------------------------------------------- */
/* Block 11: scaled, weighted scores of a hierarchy: RMSSE, SPL, WRMSSE, WSPL  */
/* ------------------------------------------------------------------------- */
/*
 * The scores a hierarchy such as M5 is judged by (Makridakis et al., The M5 competition, competitors' guide): a loss per column
 * divided by the column's in-sample scale, and the weighted mean of the scaled losses over the columns of a level.  The reference
 * has no such function; the names are this package's own and tests/scaled_scores_ref.py is the definition, bit for bit.  Plain
 * fp64, one rounding per operation, nothing fused: a product is rounded, then added.
 *   - the scale of a column y[0 .. n) (n = its length cut to t_rows): t0 = the first row with y != 0.0 when trim_leading_zeros
 *     (+0.0 and -0.0 are both zero; t0 = n when every row is) and 0 otherwise; for t = t0 + lag .. n - 1 in row order,
 *     d = y[t] - y[t - lag], sq = sq + d * d, ab = ab + |d|, both serial from 0.0; n_terms = n - t0 - lag, msd = sq / n_terms,
 *     mad = ab / n_terms.  msd is what RMSSE divides the mse by, mad what MASE and the scaled pinball loss divide by;
 *   - the weight mass: tail = the serial sum from 0.0 of w_src over the rows max(0, n - tail_rows) .. n - 1 in row order (w_src NULL:
 *     y itself; for M5 the aggregated units x price block and tail_rows = 28);
 *   - status per column (int32): 0 done; 1 n_terms <= 0 -- msd and mad are NaN, n_terms and tail are still written (tail is 0.0 for
 *     n = 0); 2 a NaN among the rows [0, n) of y or among the tail rows of w_src -- all four figures are NaN; 2 takes precedence;
 *     3 msd == 0.0 -- the series is constant after t0 and both scales are written as 0.0.  +-inf are ordinary values.  Rows >= n and
 *     columns >= n_cols never enter a result;
 *   - the scaled loss of (loss row r, column c): s = loss / scale (transform 0: SPL from a pinball row and mad, MASE from mae and
 *     mad) or s = sqrt(loss / scale) (transform 1: RMSSE from mse and msd; the correctly rounded root).  A column is LEFT OUT when
 *     col_status != 0, when its scale is not finite or is <= 0.0, when its weight is NaN or negative, or when s is not finite (that
 *     one per loss row): its out_scaled cell is NaN, it adds 0.0 to both sums and it is counted in out_left;
 *   - per (range g = [begin, end), loss row r): N = W_c(w_c * s_c), D = W_c(w_c), each product rounded once, W the wave sum of Block
 *     10 with the terms indexed by c - begin; score[g, r] = N / D, NaN when D is not positive;
 *   - total[r] = the serial sum from 0.0 of the non-NaN score[g, r] in range order, divided by their count (NaN when there is none):
 *     with M5's twelve ranges the 1/12 per level; total_mean = the serial sum over r of total[r], divided by n_loss: with the nine
 *     pinball rows the WSPL.
 */
enum { ANOFOX_SCALE_OK = 0, ANOFOX_SCALE_SHORT = 1, ANOFOX_SCALE_NAN = 2, ANOFOX_SCALE_CONSTANT = 3 };
enum { ANOFOX_SCALED_RATIO = 0, ANOFOX_SCALED_ROOT = 1 };       /* transform */
#define ANOFOX_HIP_SCALED_MAX_LOSS 16

/*
 * Scale and weight mass of every column of a device-resident block y[t * ld + c] (fp64, time-major, left-aligned, lengths int32
 * [n_cols] on the device, a length above t_rows is cut to it) -- the y_out and lengths_out of anofox_hip_hierarchy_device as they
 * lie.  w_src: a block in the same layout, or NULL for y itself.  Outputs, in device memory: out_scale fp64 [4 x ld_out] in the rows
 * msd, mad, n_terms (as double), tail (row r of column c at r * ld_out + c), out_first int32 [n_cols] (t0), status int32 [n_cols].
 * One lane per column; the loads of a block of rows are issued ahead of the serial chains that consume them.  The call only
 * enqueues on `stream` (NULL: the null stream) and does NOT wait on the host.
 * INVALID_INPUT, each naming its limit, before the device is touched: lag or tail_rows 0; lag, tail_rows or t_rows above 2^30;
 * ld < n_cols; ld_out < n_cols; n_cols above 2^31 - 1.
 */
bool anofox_hip_scale_device(const double *y,
                             size_t ld,
                             const int32_t *lengths,
                             size_t n_cols,
                             size_t t_rows,
                             const double *w_src,
                             size_t lag,
                             bool trim_leading_zeros,
                             size_t tail_rows,
                             double *out_scale,
                             size_t ld_out,
                             int32_t *out_first,
                             int32_t *status,
                             void *stream,
                             struct AnofoxError *out_error);

/*
 * Scaled losses and their weighted mean per column range.  All arrays in device memory: loss fp64 [n_loss x ld] (row r of column c
 * at r * ld + c) -- rows of `figures` of anofox_hip_metrics_device or of out_column of anofox_hip_path_scores_device are passed by
 * pointer offset, as they lie --, scale fp64 [n_cols] (one row of out_scale), weight fp64 [n_cols] (the tail row, or any non-negative
 * figure per column), col_status int32 [n_cols] or NULL, ranges int32 [n_ranges x 2], [begin, end) each.  Outputs: out_scaled fp64
 * [n_loss x ld] or NULL (written for the columns of the valid ranges; a cell no range covers is not touched), out_score and
 * out_weight_sum (D) fp64 [n_ranges x n_loss] (range g, row r at g * n_loss + r), out_left int32 [n_ranges x n_loss], out_total fp64
 * [n_loss + 1]: total[r], then total_mean.  A range that is empty, reversed or ends beyond n_cols is seen only on the device: its
 * out_left is -1, its score and weight sum are NaN -- never a cut sum -- and it does not enter the totals.  One wavefront per
 * (range, loss row), one small launch for the totals, no atomics.  The call only enqueues on `stream`.
 * INVALID_INPUT, each naming its limit: n_loss 0 or above 16, an unknown transform, ld < n_cols, n_ranges 0 or above 2^31 - 1,
 * n_cols above 2^31 - 1.
 */
bool anofox_hip_weighted_scores_device(const double *loss,
                                       size_t ld,
                                       size_t n_cols,
                                       size_t n_loss,
                                       const double *scale,
                                       const double *weight,
                                       const int32_t *col_status,
                                       const int32_t *ranges,
                                       size_t n_ranges,
                                       int32_t transform,
                                       double *out_scaled,
                                       double *out_score,
                                       double *out_weight_sum,
                                       int32_t *out_left,
                                       double *out_total,
                                       void *stream,
                                       struct AnofoxError *out_error);

/*
 * The WRMSSE of a set of forecasts, for host buffers.  values[s] points to the lengths[s] training values of series s; the series end
 * on the same date (a shorter one starts later).  prices: NULL (the weights come from the units) or one pointer per series to
 * lengths[s] prices (an entry may be NULL: the units): the weight source is then the rounded product value * price per leaf row.
 * forecast and actual fp64 [n_series x horizon] series-major, NaN for a row that does not exist.  column_of / n_groupings as for
 * anofox_hip_hierarchy_plan; NULL (or 0 groupings): the leaves alone, one range.
 *
 * The call packs once; aggregates training values, revenue, forecasts and actuals up the plan with anofox_hip_hierarchy_device (a
 * member's NaN forecast or actual drops that step of the aggregate); takes mse per column from anofox_hip_metrics_device with
 * drop_nan; computes the scales with anofox_hip_scale_device; scores one range per grouping by the rule of
 * anofox_hip_path_scores_batch -- [the smallest column the grouping maps a series to, the largest + 1) --, without a plan the whole;
 * runs anofox_hip_weighted_scores_device with transform 1, the msd row, the tail row and the scale's status; and reads back once.
 *
 * *out_n_out and *out_ld (n_out rounded up to 64, at least 64) are always written.  With out_status NULL that is all: the sizing
 * call, which needs no device.  Otherwise ld must be what the sizing call returned and the caller's arrays receive, each but
 * out_status optional (NULL): out_scale fp64 [4 x ld], out_rmsse fp64 [ld] (NaN for a column left out), out_status int32 [n_out] (of
 * the scale), out_score fp64 and out_left int32 [n_groupings, or 1 without a plan], out_ranges int32 [that many x 2], *out_total the
 * WRMSSE: the mean of the levels' scores.
 *
 * INVALID_INPUT as for the device entries and for the plan, and horizon 0 or above 2^30, a series above 2^30 rows, all before the
 * device is touched.  A failed device allocation is a COMPUTATION_ERROR that names the size.  One device (the calling thread's
 * current one); fp64 only.
 */
bool anofox_hip_wrmsse_batch(const double *const *values,
                             const size_t *lengths,
                             const double *const *prices,
                             size_t n_series,
                             const double *forecast,
                             const double *actual,
                             size_t horizon,
                             const int32_t *column_of,
                             size_t n_groupings,
                             size_t lag,
                             bool trim_leading_zeros,
                             size_t tail_rows,
                             size_t ld,
                             double *out_scale,
                             double *out_rmsse,
                             int32_t *out_status,
                             double *out_score,
                             int32_t *out_left,
                             int32_t *out_ranges,
                             double *out_total,
                             size_t *out_n_out,
                             size_t *out_ld,
                             struct AnofoxError *out_error);

/* ------------------------------------------------------------------------- */
/* Block 12: sample paths simulated from the fitted ETS models                 */
/* ------------------------------------------------------------------------- */
/*
 * The state equations of the fitted spec run forward from the final states: h steps for each of n_paths paths per series, with
 * innovations that are Gaussian or drawn from the model's own in-sample innovations (Hyndman, Koehler, Ord & Snyder 2008, section
 * 6.1: the forecast distribution of the multiplicative-error and multiplicative-trend specs has no closed form).  The names and the
 * contract are this package's own; tests/ets_paths_ref.py is the definition, bit for bit:
 *   - spec int32 [n_series]: error * 15 + trend * 3 + season (error 0 A, 1 M; trend 0 N, 1 A, 2 Ad, 3 M, 4 Md; season 0 N, 1 A, 2 M),
 *     the encoding of model_code - 100 of an AutoETS batch.  Anything that is not one of the 25 specs of the project (no
 *     multiplicative error with an additive season), and a series with lengths[s] < 1, has status 4 (NO_MODEL) and NaN paths;
 *   - info fp64 [8 x ld] (rows alpha, beta, gamma, phi, aic, aicc, bic, sse) and states fp64 [(2 + max(m, 1)) x ld] (rows level, growth,
 *     then the seasonal state of phase j in row 2 + j) as anofox_hip_batch_inspect_device writes them; the phase of step k = 0 .. h - 1
 *     is (lengths[s] + k) % m;
 *   - Gaussian innovations: sigma = sqrt(sse / n), two IEEE operations.  The draw of (series s, path p) for steps 4j .. 4j + 3 is the
 *     Philox4x32-10 block of counter {p, s, j, 2} under the key {seed & 0xffffffff, seed >> 32}: words (w0, w1) serve steps 4j and
 *     4j + 1, (w2, w3) steps 4j + 2 and 4j + 3; u1 = (wa + 0.5) 2^-32, u2 = (wb + 0.5) 2^-32, r = sqrt(-2 log u1), theta =
 *     6.283185307179586 u2; the even step takes z = r cos(theta), the odd one r sin(theta), e = sigma z (log, sin and cos are the
 *     library's own, anofox_hip_selftest_math LOG and SINCOS).  The 32-bit uniform cuts the tails at |z| = 6.76.  No joint mode;
 *   - bootstrap innovations: the index rule and the counters of block 9 unchanged (word k & 3 of counter {p, joint ? 0 : s, k >> 2,
 *     joint ? 1 : 0}, row j = (u * n) >> 32), on a pool in the model's own terms (anofox_hip_ets_innovations_device);
 *   - the step, with q = l, l + phi b, l b^phi, pt the trend's part of it (phi b, b^phi; phi = 1 undamped) and s the seasonal state of
 *     the step's phase: mu = q, q + s or q s.  Additive error: y = mu + e, l' = q + alpha e [e / s with a multiplicative season],
 *     b' = pt + beta e [e / s] (additive trend) or pt + beta e / l [e / (s l)] (multiplicative trend), s' = s + gamma e or
 *     s + gamma e / q.  Multiplicative error: y = mu (1 + e), l' = q (1 + alpha e), b' = pt + beta q e or pt (1 + beta e), s' = s (1 +
 *     gamma e).  Plain fp64, one rounding per operation, left to right, nothing fused.  b^phi of a damped multiplicative trend is
 *     the library's POW_POS; where b is not a finite positive number at that point the path is broken: that step and every later one
 *     are NaN.  Nothing else is clamped.
 * Status per series (int32): 0; 4 NO_MODEL; then those of block 9 for the pool (3, 1, 2 in that precedence); 2 also for a NaN in a
 * parameter or state the spec reads (Gaussian: in sigma).  n_broken int32 [n_series]: the paths of the series that hold a NaN.
 * Parameter uncertainty is not simulated.  One seasonal period per call, one device, fp64.
 */
#define ANOFOX_HIP_ETS_PATHS_MAX_PERIOD 2048
#define ANOFOX_HIP_ETS_PATHS_MAX_RING 128
enum { ANOFOX_ETS_PATHS_GAUSSIAN = 0, ANOFOX_ETS_PATHS_BOOTSTRAP = 1 };
enum { ANOFOX_ETS_PATHS_NO_MODEL = 4 };
typedef struct AnofoxHipEtsPathsOptions {
    int32_t innovations;         /* ANOFOX_ETS_PATHS_GAUSSIAN or ANOFOX_ETS_PATHS_BOOTSTRAP */
    int32_t joint;               /* bootstrap only: 1 = one pool row per path and step for all series */
    int32_t reserved[2];         /* 0 */
    uint64_t seed;
} AnofoxHipEtsPathsOptions;

/*
 * The fit state of an AutoETS or ETS(spec) batch that has been run, left on the device: the passes of anofox_hip_batch_inspect
 * write d_info fp64 [8 x ld], d_states fp64 [(2 + max(m, 1)) x ld] and, unless NULL, d_fitted fp64 [max(t_max, 1) x ld], all
 * time-major with ld = anofox_hip_batch_ld and NaN wherever a series or a spec has no value.  Nothing is copied to the host; the
 * call returns when the blocks are written.  The batch must have one seasonal period; any other model is INVALID_INPUT.
 */
bool anofox_hip_batch_inspect_device(AnofoxHipBatch *batch,
                                     double *d_info,
                                     double *d_states,
                                     double *d_fitted,
                                     struct AnofoxError *out_error);

/*
 * The in-sample innovations of a fitted block: pool[t * ld + s] = y - fitted for an additive error and (y - fitted) / fitted for a
 * multiplicative one, t < lengths[s]; rows past a series' length are not written.  pool_lengths[s] = lengths[s] cut to [0, t_rows],
 * 0 for a spec that is none of the project's.  y, fitted and pool are fp64 [t_rows x ld] time-major in device memory.  The call only
 * enqueues on `stream`.  INVALID_INPUT: ld < n_series, n_series or t_rows above 2^31 - 1.
 */
bool anofox_hip_ets_innovations_device(const double *y,
                                       const double *fitted,
                                       size_t ld,
                                       const int32_t *lengths,
                                       const int32_t *spec,
                                       size_t n_series,
                                       size_t t_rows,
                                       double *pool,
                                       int32_t *pool_lengths,
                                       void *stream,
                                       struct AnofoxError *out_error);

/*
 * The simulation.  All pointers but `options` are device memory.  The pool (bootstrap only) is addressed as in
 * anofox_hip_paths_device: element (s, t) at s * pool_stride_s + t * pool_stride_t, pool_lengths NULL = every pool has pool_rows
 * rows.  Outputs: paths_out fp64 [n_paths * horizon x ld_out], row p * horizon + k of column s, columns >= n_series not touched --
 * what anofox_hip_hierarchy_device, anofox_hip_path_quantiles_device and anofox_hip_path_scores_device take as it lies; status and
 * n_broken int32 [n_series].  The call only enqueues on `stream` (NULL: the null stream).
 * INVALID_INPUT, each naming its limit, before the device is touched: struct_size, an unknown innovations mode, joint with the
 * Gaussian mode, n_paths 0 or above 2,048, horizon 0, n_paths * horizon above 2^30, ld_out < n_series, ld < n_series, m < 1 or above
 * 2,048, R = min(m, horizon) above 128 (the seasonal states of a path live in 64 KiB of LDS), the bootstrap without a pool,
 * pool_rows above 2^20.
 */
bool anofox_hip_ets_paths_device(const int32_t *spec,
                                 const double *info,
                                 const double *states,
                                 size_t ld,
                                 size_t m,
                                 const int32_t *lengths,
                                 const double *pool,
                                 size_t pool_stride_s,
                                 size_t pool_stride_t,
                                 const int32_t *pool_lengths,
                                 size_t pool_rows,
                                 size_t n_series,
                                 size_t horizon,
                                 size_t n_paths,
                                 const AnofoxHipEtsPathsOptions *options,
                                 size_t struct_size,
                                 double *paths_out,
                                 size_t ld_out,
                                 int32_t *status,
                                 int32_t *n_broken,
                                 void *stream,
                                 struct AnofoxError *out_error);

/*
 * The chain for a batch that has been run (AutoETS or ETS(spec), one seasonal period): the fit state stays on the device
 * (anofox_hip_batch_inspect_device), the bootstrap takes the batch's own innovations (anofox_hip_ets_innovations_device), the
 * paths of the batch's horizon are simulated and anofox_hip_path_quantiles_device reads `levels` (host, up to 16 in [0, 1]) off them.
 * *out_ld (= anofox_hip_batch_ld) is always written.  With out_quantiles NULL that is all: the sizing call.  Otherwise ld must be
 * that value and the caller's host arrays receive out_quantiles fp64 [n_levels x n_series x horizon], out_status int32 [n_series]
 * (of the quantile entry: 2 where a path of the series holds a NaN), and, each optional (NULL), out_series_status int32 [n_series],
 * out_n_broken int32 [n_series] and out_paths fp64 [n_paths * horizon x ld].
 * The argument checks (options, n_paths, levels; then the batch; then horizon, period and R) come before the device is touched.  A
 * failed device allocation is a COMPUTATION_ERROR that names the size.
 */
bool anofox_hip_batch_ets_paths(AnofoxHipBatch *batch,
                                const AnofoxHipEtsPathsOptions *options,
                                size_t struct_size,
                                size_t n_paths,
                                const double *levels,
                                size_t n_levels,
                                size_t ld,
                                double *out_quantiles,
                                int32_t *out_status,
                                int32_t *out_series_status,
                                int32_t *out_n_broken,
                                double *out_paths,
                                size_t *out_ld,
                                struct AnofoxError *out_error);

/* ------------------------------------------------------------------------- */
/* Block 13: sample paths simulated from the fitted AutoARIMA models           */
/* ------------------------------------------------------------------------- */
/*
 * The fitted ARIMA recursion simulated forward from the tails of the differenced series and of its in-sample innovations, then the
 * differences integrated: h steps for each of n_paths paths per series (Box & Jenkins; Hyndman & Athanasopoulos, Forecasting:
 * Principles and Practice, "Prediction intervals from simulated paths").  The names and the contract are this package's own;
 * tests/arima_paths_ref.py is the definition, bit for bit:
 *   - the convention of AnofoxHipArimaFit, (1 - phi(B))(1 - Phi(B^m)) (w_t - c) = (1 - theta(B))(1 - Theta(B^m)) e_t on the differenced
 *     series w (the seasonal difference first, then the d ordinary ones, each a single subtraction), c the constant or 0.0;
 *   - the fit blocks, time-major with leading dimension ld: orders int32 [8 x ld] (rows p, d, q, P, D, Q, has_constant, n_diff) and
 *     coef fp64 [16 x ld] (rows phi 1..5, theta 1..5, Phi 1..2, Theta 1..2, constant, aicc), as anofox_hip_batch_arima_fit_device
 *     writes them;
 *   - the lag polynomials are not multiplied out: a side is the sum over the terms (i, j), 0 <= i <= p, 0 <= j <= P, without (0, 0),
 *     of coefficient x value at lag i + j m, the coefficient phi_i, Phi_j or -(phi_i Phi_j), added j-major and i-minor from 0.0; a
 *     value before the differenced series is 0.0.  x_t = w_t - c; in sample e_t = 0 for t < La = p + m P and e_t = (x_t - ar) + ma
 *     after; css = the serial sum of e_t^2, nu = n_diff - La, sigma = sqrt(css / nu).  A path: x_t = (ar + e_t) - ma, v = x_t + c,
 *     then last_d1 += v (d = 2), last_d0 += v (d >= 1) and + y of m steps before (D = 1), from the history or the path itself.
 *     Plain fp64, one rounding per operation, nothing fused, nothing clamped: a step whose value is not finite is NaN and so is
 *     every later step of that path;
 *   - Gaussian innovations: the rule of block 12 with the last counter word 3: counter {p, s, j, 3}, e = sigma z.  No joint mode;
 *   - bootstrap innovations: the index rule and the counters of block 9 on the series' own nu residuals; joint: draw j < pool_rows
 *     takes residual row nu - pool_rows + j of every series (the same date for series that end together).
 * Status per series (int32): 0; 4 NO_MODEL (orders outside p, q <= 5, P, Q <= 2, d <= 2, D <= 1, has_constant 0 / 1; lengths[s] < 1;
 * n_diff other than lengths[s] - d - D m, which includes the zero row of a series without a fit; nu < 1; resid_lengths[s] other
 * than nu); then 3 (joint: nu < pool_rows), 1 (joint: pool_rows 0), 2: a NaN in a coefficient the orders read, in sigma (Gaussian),
 * in the last La + d + D m observations, in the last min(nu, q + m Q) residuals or (bootstrap) in the rows of the pool.  The paths
 * of a series whose status is not 0 are NaN.  n_broken int32 [n_series]: the paths of the series that hold a NaN.
 * AutoARIMA only (the fixed-order ARIMA model has no fit readback); parameter uncertainty is not simulated.  One seasonal period
 * per call, one device, fp64.  The simulated values a later step reads at a seasonal lag live in LDS: 2 min(h, 2 m + 5) +
 * (m < h ? m : 0) rows of 512 bytes per wavefront, at most ANOFOX_HIP_ARIMA_PATHS_MAX_LDS_ROWS.
 */
#define ANOFOX_HIP_ARIMA_PATHS_MAX_PERIOD 2048
#define ANOFOX_HIP_ARIMA_PATHS_MAX_LDS_ROWS 128
enum { ANOFOX_ARIMA_PATHS_GAUSSIAN = 0, ANOFOX_ARIMA_PATHS_BOOTSTRAP = 1 };
enum { ANOFOX_ARIMA_PATHS_NO_MODEL = 4 };
typedef struct AnofoxHipArimaPathsOptions {
    int32_t innovations;         /* ANOFOX_ARIMA_PATHS_GAUSSIAN or ANOFOX_ARIMA_PATHS_BOOTSTRAP */
    int32_t joint;               /* bootstrap only: 1 = one residual row (counted from the end) per path and step for all series */
    int32_t reserved[2];         /* 0 */
    uint64_t seed;
} AnofoxHipArimaPathsOptions;

/*
 * The fit of an AutoARIMA batch that has been run, left on the device: d_orders int32 [8 x ld] and d_coef fp64 [16 x ld] with
 * ld = anofox_hip_batch_ld.  The coefficients are the ones the recursion reads (the box clip applied); zeros and NaN go exactly
 * where anofox_hip_batch_arima_fit puts them: a series nothing was fitted to has zero orders and NaN in every double, slots beyond
 * the orders are 0.0.  Nothing is copied to the host; the call returns when the blocks are written.  The error cases are those of
 * anofox_hip_batch_arima_fit.
 */
bool anofox_hip_batch_arima_fit_device(AnofoxHipBatch *batch,
                                       int32_t *d_orders,
                                       double *d_coef,
                                       struct AnofoxError *out_error);

/*
 * The in-sample innovations of the fitted models.  y fp64 [t_rows x ld] time-major, lengths int32 [n_series] (cut to [0, t_rows]).
 * Outputs: resid fp64 [t_rows x ld], compacted -- row j of column s is the residual of differenced index La + j, rows from nu on are
 * not written --, resid_lengths int32 [n_series] (nu; 0 where the series has no model) and sigma fp64 [n_series] (NaN there).  All
 * pointers are device memory.  The call only enqueues on `stream`.  INVALID_INPUT, each naming its limit, before the device is
 * touched: ld < n_series, n_series or t_rows above 2^31 - 1, m < 1 or above 2,048.
 */
bool anofox_hip_arima_innovations_device(const int32_t *orders,
                                         const double *coef,
                                         size_t ld,
                                         const double *y,
                                         const int32_t *lengths,
                                         size_t m,
                                         size_t n_series,
                                         size_t t_rows,
                                         double *resid,
                                         int32_t *resid_lengths,
                                         double *sigma,
                                         void *stream,
                                         struct AnofoxError *out_error);

/*
 * The simulation.  All pointers but `options` are device memory; y and resid are fp64 [t_rows x ld], sigma fp64 [n_series] (read by
 * the Gaussian mode only), pool_rows is read in joint mode only.  Outputs: paths_out fp64 [n_paths * horizon x ld_out], row
 * p * horizon + k of column s, columns >= n_series not touched -- what anofox_hip_hierarchy_device,
 * anofox_hip_path_quantiles_device and anofox_hip_path_scores_device take as it lies; status and n_broken int32 [n_series].  The
 * call only enqueues on `stream` (NULL: the null stream).
 * INVALID_INPUT, each naming its limit, before the device is touched: struct_size, an unknown innovations mode, joint with the
 * Gaussian mode, n_paths 0 or above 2,048, horizon 0, n_paths * horizon above 2^30, ld_out < n_series, ld < n_series, t_rows above
 * 2^31 - 1, m < 1 or above 2,048, 2 min(horizon, 2 m + 5) + (m < horizon ? m : 0) above 128 LDS rows, pool_rows above 2^20.
 */
bool anofox_hip_arima_paths_device(const int32_t *orders,
                                   const double *coef,
                                   size_t ld,
                                   const double *y,
                                   const int32_t *lengths,
                                   size_t t_rows,
                                   const double *resid,
                                   const int32_t *resid_lengths,
                                   const double *sigma,
                                   size_t m,
                                   size_t pool_rows,
                                   size_t n_series,
                                   size_t horizon,
                                   size_t n_paths,
                                   const AnofoxHipArimaPathsOptions *options,
                                   size_t struct_size,
                                   double *paths_out,
                                   size_t ld_out,
                                   int32_t *status,
                                   int32_t *n_broken,
                                   void *stream,
                                   struct AnofoxError *out_error);

/*
 * The chain for an AutoARIMA batch that has been run (one seasonal period): the fit stays on the device
 * (anofox_hip_batch_arima_fit_device), anofox_hip_arima_innovations_device gives residuals and sigma, the paths of the batch's
 * horizon are simulated (joint: pool_rows = the smallest nu among the fitted series) and anofox_hip_path_quantiles_device reads
 * `levels` (host, up to 16 in [0, 1]) off them.  Sizing call, outputs and the order of the checks as for anofox_hip_batch_ets_paths.
 */
bool anofox_hip_batch_arima_paths(AnofoxHipBatch *batch,
                                  const AnofoxHipArimaPathsOptions *options,
                                  size_t struct_size,
                                  size_t n_paths,
                                  const double *levels,
                                  size_t n_levels,
                                  size_t ld,
                                  double *out_quantiles,
                                  int32_t *out_status,
                                  int32_t *out_series_status,
                                  int32_t *out_n_broken,
                                  double *out_paths,
                                  size_t *out_ld,
                                  struct AnofoxError *out_error);

#ifdef __cplusplus
} /* extern "C" */
#endif

#endif /* ANOFOX_FCST_HIP_H */
