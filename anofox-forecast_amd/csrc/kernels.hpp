// kernels.hpp -- kernel argument blocks and launch entry points shared by the .hip units
// and the host layer.  Everything device-side is one-wave (64-thread) workgroups: lane <->
// series, so a workgroup covers 64 consecutive columns of the time-major block.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include <atomic>

#include <stdexcept>
#include <string>

namespace anofox {

// results of the runtime calls made while preparing a launch (raising a kernel's LDS limit, clearing a counter) are
// never discarded: a refused request would otherwise surface as a silent launch failure
inline void anofox_check_attr(hipError_t e)
{
    if (e != hipSuccess) throw std::runtime_error(std::string("launch preparation failed: ") + hipGetErrorString(e));
}

// per-series flag bits produced by the prep kernel
enum : uint32_t { SF_POSITIVE = 1u, SF_CONSTANT = 2u, SF_HAS_NAN = 4u };

// per-(series, spec) fit status
enum : int32_t { FIT_OK = 0, FIT_SHORT = 1, FIT_NONPOSITIVE = 2, FIT_NONFINITE = 3, FIT_PERIOD = 4, FIT_SKIPPED = 5 };

struct PrepArgs {
    const double *y; size_t ld; const int32_t *len; int n_series;
    int m;                 // seasonal period to prepare figures for (<= 1: none); with m_col: the LARGEST period of the block (sizes)
    const int32_t *m_col;  // [ld] period of every column, constant within each group of 64 columns (a merged batch of several periods); NULL = m
    double *mean, *sd;     // population mean / sd of the series (forecast.rs:2558-2591)
    uint32_t *flags;
    double *fig_add, *fig_mul;   // [m x ld] seasonal figures (additive / multiplicative)
    double *l0, *b0;       // [9 x ld]: index (season_type * 3 + trend_type)
    double *scratch;       // season_figures scratch for series too long for its LDS (season_scratch_doubles), else unused
    int pre_fig;           // 1: fig_add / fig_mul already hold the figures (launch_season_figures): no decomposition in the sweep
    int t_rows;            // rows of the block (the figures kernel sizes its LDS by it)
    int skip_sd;           // 1: the batch's ONE final pass computes sd (FitArgs::sd_out): prep_kernel is a single sweep then
    int skip_types;        // season types NO candidate spec of the batch has (bit 0 additive, bit 1 multiplicative): their figures and start
                           // states are not computed (the multiplicative figure is an IEEE division per time step)
};

// seasonal figures of every period but 7, one workgroup per series (prep.hip season_figures_kernel); `scratch`: season_scratch_doubles
// doubles when the series and its trend do not fit LDS (else unused)
size_t season_scratch_doubles(int n_series, int t_rows, int m_max);
void launch_season_figures(const PrepArgs &a, hipStream_t stream);

// Nelder-Mead state parked in HBM between rounds, indexed by series (stride ld)
struct NmStateBuf {
    double *sim;                 // [(D+1)*D x ld], vertex k coordinate i at row k*D+i
    double *fs;                  // [(D+1) x ld]
    int32_t *phase, *evals, *iters, *passes, *done;   // [ld]
};

struct FitArgs {
    const double *y; size_t ld; const int32_t *len; int n_series;
    int t_rows;                  // rows held by the blocks y and y_round (streaming loads clamp to the last one)
    // round-specific view: the block this round streams (original or gathered columns), the column ->
    // series map (NULL = identity) and the device-side count of running problems (NULL = n_series)
    const double *y_round; size_t ld_round;
    const int32_t *series_of;
    const int32_t *n_active;
    int budget, first_round;
    const int32_t *m_col;        // [ld] per-column seasonal period (constant within 64 columns) of a merged batch of several periods; NULL = m (then m is the size bound)
    int spec_below;              // device-side driver choice: the speculative kernel runs iff n_active <= spec_below,
                                 // the sequential one iff n_active > spec_below (both are enqueued; -1 = unconditional)
    const uint32_t *mask;        // SES / Holt / Holt-Winters / SeasonalES on the round kernels: run only where mask[s] == want (NULL = all series)
    uint32_t want;
    int min_len;                 // ... and fail shorter series (Holt-Winters and SeasonalES derive theirs from the period)
    int budget_seq;              // passes per round when the device-side choice (round_auto) lands on the sequential driver
    int spec2_below;             // ... and the one-problem-per-wave driver (two iterations per pass) iff n_active <= spec2_below
    int gathered;                // y_round holds the running problems' columns densely (column p), else index by series
    int gather_cap;              // columns y_round has room for: the gather (and this flag) only apply while n_active <= gather_cap
    NmStateBuf st;
    double *ring_scratch;        // periods above ETS_LDS_PERIOD: m * 64 doubles per workgroup of the launch (seasonal ring in HBM)
    size_t ring_scratch_doubles; //   doubles it holds: every launch checks that its workgroups fit (ets_round_launch; round 6 -- a scratch sized for
                                 //   fewer workgroups than a launch has is a stray device write, found as an intermittent memory fault)
    double *nm_scratch;          // PARK kernels (ets_fit_kernel.hpp RoundTraits): nm_lds_doubles<DIM>() doubles per workgroup of the launch,
    size_t nm_scratch_doubles;   //   where the lanes' simplices rest between passes (else they rest in LDS); doubles it holds
    int m, h;
    const double *l0, *b0;       // [ld] for this spec's (season, trend) class
    const double *fig; size_t fig_ld;
    const uint32_t *flags;
    int need_positive;           // spec has a multiplicative component
    int skip_constant;           // AutoETS: constant series go to the fallback chain
    int n_param;                 // k of the information criteria
    double *aicc;                // [ld]
    double *yhat;                // [n_series x h] for this spec
    int32_t *status;             // [ld]
    int32_t *evals, *iters, *passes; // [ld]
    // inspection pass of the final kernel (all NULL in a normal run): only series whose selected model is `insp_code` take part
    const int32_t *insp_sel;     // [n_series] selected model code
    int32_t insp_code;
    double *insp_fitted;         // [t_rows x ld] one-step fitted values (time-major)
    double *insp_states;         // [(2 + m) x ld] final level, growth, seasonal states by phase
    double *insp_info;           // [8 x ld] alpha, beta, gamma, phi, aic, aicc, bic, sse
    // lane-level efficiency of the round kernels (round 5; NULL = not counted): [0] += passes the wave streamed, [1] += lane-passes
    // that evaluated a trial point of a running problem -- live_lane_passes / (64 wave_passes) is the share of the issued lanes that
    // did work (a converged or parked lane idles until its wave leaves; a wave of the one-wave-per-problem driver counts 64 live lanes)
    unsigned long long *lane_stats;
    // a batch with ONE candidate spec (explicit ETS, fitted or with given parameters): its final pass is the second sweep of the intervals'
    // population sd (forecast.rs:2558-2591: sum of (y - mean)^2 in time order), so prep_kernel needs none (PrepArgs::skip_sd).  NULL otherwise.
    const double *mean;          // [ld] series means (prep_kernel)
    double *sd_out;              // [ld]
    // developer instrument (round 6; NULL = off: ANOFOX_HIP_TUNE wave_trace=<file>): every wave of a round kernel that streams at least one
    // pass appends one record {tag, start, end (s_memrealtime ticks, 100 MHz), HW_ID | XCC_ID << 32} -- who is resident when, and how long a
    // launch's waves wait for a SIMD with room.  wave_trace[0] = records used (atomic), [1] = capacity, records from [4] on.
    int wave_prio;               // issue priority of the round kernel's waves (s_setprio 0..3): the chains that end the step run ahead of their SIMD's other wave
    unsigned long long *wave_trace;
    unsigned long long wave_trace_tag;   // spec order index << 32 | round << 16 | workgroups of the launch are not needed: blockIdx goes in
};

struct SelectArgs {
    int n_series, h, n_slots;
    size_t ld;
    const int32_t *len;          // series with len <= 0 are not part of this group
    const double *aicc;          // [n_slots x ld]
    const double *yhat_slots;    // [n_slots x n_series x h]
    const int32_t *slot_spec;    // [n_slots] spec id
    const int32_t *status_slots; // [n_slots x ld]
    const int32_t *passes_slots; // [n_slots x ld]
    const int32_t *evals_slots;
    double *yhat;                // [n_series x h]
    int32_t *model_code;         // [n_series]
    int32_t *status;             // [n_series]  0 ok, -1 needs fallback
    uint32_t *fallback_mask;     // [n_series] 1 where the fallback chain must run
    int32_t *passes_total;       // [n_series] streamed passes summed over specs (+1 final each)
    int32_t *evals_total;
};

struct ClassicArgs {
    const double *y; size_t ld; const int32_t *len; int n_series;
    int m, h;
    int optimized;               // SES / SeasonalES: optimise alpha (else fixed_alpha)
    double fixed_alpha;
    const uint32_t *mask;        // NULL = all series; else run only where mask[s] == want
    uint32_t want;
    int min_len;                 // series shorter than this fail (status = FIT_SHORT)
    double *yhat;                // [n_series x h]
    int32_t *status;             // [n_series]
    int32_t *passes;             // [n_series] (accumulated)
    int32_t model_code;          // written to model_code[s] when not NULL
    int32_t *model_code_out;
    double *ring_scratch;        // periods whose K * m * 64 ring does not fit LDS: that many doubles per workgroup in HBM
    const int32_t *m_col;        // [ld] per-column period (constant within 64 columns) of a merged batch; NULL = m.  min_len is then 2 m (Holt-Winters) of the column's own period
};

enum SimpleKind { SK_NAIVE = 0, SK_SEASONAL_NAIVE = 1, SK_SMA = 2, SK_DRIFT = 3, SK_TOY_ARIMA = 4 };
struct SimpleArgs {
    const double *y; size_t ld; const int32_t *len; int n_series;
    int kind, h, period, window;
    double *yhat; int32_t *status;
};

// intermittent-demand models (fit_intermittent.hip)
enum IntermittentKind { IK_CROSTON = 0, IK_SBA = 1, IK_TSB = 2, IK_ADIDA = 3, IK_IMAPA = 4 };
struct IntermittentArgs {
    const double *y; size_t ld; const int32_t *len; int n_series;
    int kind, h;
    int n_groups;                // intermittent_groups(n_series): workgroups of 64 consecutive series
    double *yhat;                // [n_series x h]
    int32_t *detail;             // [ld] FIT_OK for every series with len > 0
    int32_t *level;              // [ld] aggregation level K of every series (0: no demand)
    int32_t *group_max;          // [n_groups + 1] largest K of each group, [n_groups]: of the batch (atomicMax: zeroed before croston)
    double *level_fc;            // IMAPA: [n_levels x ld], SESopt of level k / k at row k - 1
    int n_levels;                // IMAPA: rows of level_fc = largest K of the batch (read back after launch_croston)
};
int intermittent_groups(int n_series);
void launch_croston(const IntermittentArgs &, hipStream_t);   // every kind: sizes / intervals / demand SES, K, group maxima
void launch_agg_ses(const IntermittentArgs &, hipStream_t);   // ADIDA / IMAPA, after launch_croston

// dynamic Theta models (fit_theta.hip)
enum ThetaKind { TK_DSTM = 0, TK_DOTM = 1 };
struct ThetaArgs {
    const double *y; size_t ld; const int32_t *len; int n_series;
    int kind, h;
    int m;                       // seasonal period of the batch (<= 1: no season test); m_col: per column (merged batch), m its largest
    const int32_t *m_col;
    double *sidx;                // [m x ld] multiplicative seasonal indices of the adjusted series (m > 1)
    int32_t *adjusted;           // [ld] 1: the series is seasonally adjusted (written by theta_season_kernel, m > 1)
    double *yhat;                // [n_series x h]
    int32_t *detail;             // [ld] FIT_OK, or FIT_NONFINITE when a forecast is not finite
    int32_t *evals;              // [ld] objective evaluations (DOTM), or nullptr
};
void launch_theta(const ThetaArgs &, hipStream_t);

// MSTL decomposition and SeasonalWindowAverage (fit_mstl.hip)
constexpr int MSTL_MAX_PERIODS = 8;      // periods per call; more fail loudly (COMPUTATION_ERROR)
enum MstlMode { MSTL_MODE_FAIL = 0, MSTL_MODE_TREND = 1, MSTL_MODE_NONE = 2 };     // decomposition.rs InsufficientDataMode::from_int
enum MstlState { MSTL_APPLIED = 0, MSTL_TREND_ONLY = 1, MSTL_NOT_APPLIED = 2, MSTL_FAILED = 3 };
struct MstlArgs {
    const double *y; size_t ld; const int32_t *len; int n_series;
    size_t t_rows;               // rows of the output blocks
    int mode, min_period;        // insufficient_data_mode; smallest period > 0 of the call (0: none)
    int n_periods;               // <= MSTL_MAX_PERIODS, in descending order
    int periods[MSTL_MAX_PERIODS];
    int tab_off[MSTL_MAX_PERIODS];   // first row of period k's phase table in `tab`
    double *tab;                 // [sum of periods x ld] phase means avg_k
    double *mean;                // [MSTL_MAX_PERIODS x ld] mean of the periodic component of stage k
    int32_t *used;               // [ld] bit k: stage k ran for the series
    double *trend, *remainder;   // [t_rows x ld]
    double *seasonal;            // [n_periods x t_rows x ld], slot k = stage k (NaN where it did not run)
    int32_t *info;               // [ld] MstlState << 8 | used
};
void launch_mstl(const MstlArgs &, hipStream_t);      // one mstl_season_kernel per period, then mstl_final_kernel
void launch_swa(const SimpleArgs &, hipStream_t);     // SeasonalWindowAverage point forecasts

// Bayesian online changepoint detection (changepoint.rs detect_changepoints_bocpd; changepoint.hip)
constexpr int BOCPD_MAX_RUN = 500;       // run lengths tracked per series (changepoint.rs: max_keep)
struct ChangepointArgs {
    const double *y; size_t ld; const int32_t *len; int n_series;
    size_t t_rows;               // rows of the output blocks; a longer series is cut to it
    double hazard;               // 1 / max(hazard_lambda, 1)
    double *prob;                // [t_rows x ld] P(run length = 1) after step t; rows t >= len stay untouched
    uint8_t *flag;               // [t_rows x ld] prob > 0.5 && t > 0
    int32_t *count;              // [n_series] flagged points, -1 for a series of fewer than 3 observations (nothing else written)
};
void launch_bocpd(const ChangepointArgs &, hipStream_t);

// Changepoints by the optimal-partitioning recurrence with the L2 cost (changepoint.rs detect_changepoints, "PELT"; pelt.hip)
constexpr int PELT_RESIDENT = 2048;      // rows of the longest series whose arrays live in LDS; longer ones use the global workspace
constexpr size_t PELT_MAX_ROWS = (size_t)1 << 16;     // rows of a block: n^3 / 6 pair-steps per series; bounds the workspace (940 MB) and the penalty table
struct PeltArgs {
    const double *y; size_t ld; const int32_t *len; int n_series;
    size_t t_rows;               // rows of the flag block; a longer series is cut to it
    int64_t min_size;            // max(min_size, 1)
    double penalty;              // used when pen_tab is null
    const double *pen_tab;       // [t_rows + 1] 2 ln n as the host's libm rounds it (the default penalty), or null
    uint8_t *flag;               // [t_rows x ld] 1 at a changepoint, else 0; rows t >= len stay untouched
    int32_t *count;              // [n_series] changepoints
    double *cost;                // [n_series] f[n]; 0.0 for a series of fewer than 2 min_size rows
    int resident;                // pelt_resident(t_rows): rows the LDS of the launch holds
    double *work;                // [work_groups x work_stride] or null when t_rows <= PELT_RESIDENT
    size_t work_stride; int work_groups;
};
int pelt_resident(size_t t_rows);
size_t pelt_work_stride(size_t t_rows);  // doubles per workspace slice (0: no workspace needed)
int pelt_work_groups(int n_series);
void launch_pelt(const PeltArgs &, hipStream_t);

// Per-series statistics (stats.rs compute_ts_stats_with_dates_and_type; stats.hip)
constexpr int STATS_RESIDENT = 2048;     // rows of the longest series that is sorted in LDS; longer ones use the global workspace
constexpr int STATS_WORK_WAVES = 1024;   // waves (and workspace slices) that walk the longer series
constexpr int STATS_N_INT = 14, STATS_N_FP = 22;
constexpr int STATS_FREQ_FIXED = 0, STATS_FREQ_MONTHLY = 1, STATS_FREQ_QUARTERLY = 2, STATS_FREQ_YEARLY = 3;
struct StatsArgs {
    const double *y; const uint8_t *valid; const int64_t *dates;      // [t_rows x ld]; valid and dates may be null
    size_t ld; const int32_t *len; int n_series;
    size_t t_rows;               // a longer series is cut to it
    int64_t freq_us; int freq_type;
    int64_t *out_int;            // [STATS_N_INT x ld] the 12 counts in struct order, expected_length, n_gaps (-1: no date figures)
    double *out_fp;              // [STATS_N_FP x ld] mean .. stability in struct order
    uint64_t *work;              // [work_waves x work_stride] or null when t_rows <= STATS_RESIDENT
    size_t work_stride; int work_waves;
};
size_t stats_work_stride(size_t t_rows);  // words per workspace slice (0: no workspace needed)
int stats_work_waves(int n_series);
void launch_stats(const StatsArgs &, hipStream_t);

// Series preparation (gaps.rs fill_gaps, the ts_drop_*_zeros_by macros, imputation.rs; dataprep.hip)
constexpr int PREP_TRIM_NONE = 0, PREP_TRIM_LEADING = 1, PREP_TRIM_TRAILING = 2, PREP_TRIM_EDGE = 3;
constexpr int PREP_FILL_NONE = 0, PREP_FILL_CONST = 1, PREP_FILL_FORWARD = 2, PREP_FILL_BACKWARD = 3, PREP_FILL_MEAN = 4,
              PREP_FILL_INTERPOLATE = 5;
constexpr int PREP_N_INT = 8, PREP_N_FP = 2;
constexpr int64_t PREP_MAX_ROWS = (int64_t)1 << 24;      // rows of one series after the gaps stage; more: PREP_OVER_LIMIT
constexpr int64_t PREP_OK = 0, PREP_NO_ROOM = 1, PREP_OVER_LIMIT = 2;
struct DataprepArgs {
    const double *y; const uint8_t *valid; const int64_t *dates;      // [t_rows x ld]; valid and dates may be null
    size_t ld; const int32_t *len; int n_series;
    size_t t_rows;               // a longer series is cut to it
    int gaps, freq_type; int64_t freq_us;
    int trim, fill; double fill_value;
    size_t t_out;                // rows of the output blocks
    double *y_out; uint8_t *valid_out; int64_t *dates_out;            // [t_out x ld]; y_out null: count only; the others may be null
    int32_t *len_out;            // [n_series]
    int64_t *out_int;            // [PREP_N_INT x ld] input rows, input NULLs, inserted, trimmed front, trimmed back, output NULLs,
                                 //                   output rows valid and != 0, status
    double *out_fp;              // [PREP_N_FP x ld] min, max of the valid output values (NaN ranks above every number)
};
void launch_dataprep(const DataprepArgs &, hipStream_t);

// Period detection (periods.rs lomb_scargle, aic_comparison, sazed_period; periods.hip)
constexpr int PERIODS_LOMB_SCARGLE = 0, PERIODS_AIC = 1, PERIODS_SAZED = 2;
constexpr int PERIODS_TILE = 2048;       // rows of a series staged in LDS at a time; a longer series is walked tile by tile
constexpr int PERIODS_SPEC_LDS = 4096;   // SAZED power-spectrum bins kept in LDS; a longer spectrum lives in the global workspace
constexpr int64_t PERIODS_SAZED_MAX_PADDED = (int64_t)1 << 24;       // largest padded length of SAZED; a longer one fails loudly
constexpr size_t PERIODS_WORK_BYTES = (size_t)256 << 20;             // upper bound of the SAZED workspace, whatever n_series is
constexpr int PERIODS_N_FP = 5;
constexpr int32_t PERIODS_OK = 0, PERIODS_TOO_SHORT = 1, PERIODS_OVER_LIMIT = 2;
struct PeriodsArgs {
    const double *y; size_t ld; const int32_t *len; int n_series;
    size_t t_rows;               // a longer series is cut to it
    int method;
    double min_period, max_period;       // Lomb-Scargle / AIC: <= 0 means the source's default
    int64_t n_grid;              // frequencies (Lomb-Scargle) or candidates (AIC), the default already applied
    int64_t s_min, s_max, s_pad; // SAZED: min_period, max_period, zero_pad_factor; 0 means the source's default
    double *out_fp;              // [PERIODS_N_FP x ld]  LS: period, frequency, power, false_alarm_prob;  AIC: period, aic, bic, rss,
                                 //                      r_squared;  SAZED: period, power, snr
    int32_t *out_index;          // [n_series] the selected grid index (frequency, candidate or DFT bin), -1: none
    int32_t *status;             // [n_series] PERIODS_OK / _TOO_SHORT / _OVER_LIMIT (nothing else written unless OK)
    double *work; size_t work_stride; int work_blocks;   // SAZED spectra above PERIODS_SPEC_LDS bins: [work_blocks x work_stride]
};
size_t periods_work_stride(size_t t_rows, int64_t s_pad);   // doubles per workspace slice (0: every spectrum fits in LDS)
int periods_work_blocks(size_t work_stride, int n_series);
void launch_periods(const PeriodsArgs &, hipStream_t);

// Period search (periods.rs ssa_period :800-937 and stl_period :952-1120; period_search.hip).  Bit for bit the source's arithmetic.
constexpr int PSEARCH_TILE = 2048;           // rows of a series staged in LDS; a longer series is read from global memory
constexpr size_t PSEARCH_MAX_ROWS = 65536;   // t_rows of a call
constexpr int PSEARCH_LDS_DOUBLES = 7936;    // the LDS pool of a workgroup (62 KiB): vectors, the staged series and what else fits
constexpr int32_t PSEARCH_OK = 0, PSEARCH_TOO_SHORT = 1, PSEARCH_OVER_LIMIT = 2, PSEARCH_STL_RANGE = 3, PSEARCH_STL_NO_CANDIDATE = 4;
constexpr int SSA_MAX_WINDOW = 2048;         // a series whose effective window is larger fails alone (PSEARCH_OVER_LIMIT)
constexpr int SSA_MAX_COMPONENTS = 32;
constexpr int SSA_WAVE_WINDOW = 64;          // windows up to this run with one wavefront per series (matrix always in LDS)
constexpr int SSA_N_FIG = 3, SSA_N_DETECTED = 4;
constexpr int SSA_ROUTE_AUTO = 0, SSA_ROUTE_GROUP = 1;     // _AUTO: one wavefront where the window allows; _GROUP: 256 lanes for every window
constexpr size_t SSA_WORK_BYTES = (size_t)1 << 30;      // upper bound of the matrix workspace, whatever n_series is (one slice if a slice is larger)
constexpr int STL_MAX_CANDIDATES = 64;
constexpr int STL_WAVES = 4;                 // waves of a workgroup, one candidate at a time each
constexpr int STL_N_FIG = 3;
constexpr size_t STL_WORK_BYTES = (size_t)256 << 20;
struct SsaArgs {
    const double *y; size_t ld; const int32_t *len; int n_series;
    size_t t_rows;               // a longer series is cut to it
    int64_t window;              // 0: n / 3 of each series
    int n_components;            // resolved: 10 by default, <= SSA_MAX_COMPONENTS
    int route;
    double *out_fp;              // [SSA_N_FIG x ld] period, variance_explained, n_eigenvalues
    double *out_eig;             // [n_components x ld] or null: the eigenvalues, NaN beyond n_eigenvalues
    double *out_det;             // [SSA_N_DETECTED x ld] or null: detected_periods, NaN beyond what exists
    int32_t *status;             // [n_series] PSEARCH_OK / _TOO_SHORT / _OVER_LIMIT (nothing else written unless OK)
    double *work; size_t work_stride; int work_blocks;     // matrices that do not fit in LDS: [work_blocks x work_stride]
};
size_t ssa_work_stride(size_t t_rows, int64_t window);      // doubles per workspace slice: the square of the largest window of the call
int ssa_work_blocks(size_t work_stride, int n_series);
void launch_ssa_period(const SsaArgs &, hipStream_t);
struct StlPeriodArgs {
    const double *y; size_t ld; const int32_t *len; int n_series;
    size_t t_rows;
    int64_t min_period, max_period;      // 0: 4 and n / 3 of each series
    int n_cand;                  // resolved: max(n_candidates or 20, 5), <= STL_MAX_CANDIDATES
    double *out_fp;              // [STL_N_FIG x ld] period, seasonal_strength, trend_strength
    int32_t *out_index;          // [n_series] the winning candidate, -1 for the constant-series return
    int32_t *status;             // [n_series] PSEARCH_OK / _TOO_SHORT / _STL_RANGE / _STL_NO_CANDIDATE
    int32_t *out_cand;           // [n_cand x ld] or null: the candidate periods, -1 beyond the list
    double *out_strength;        // [n_cand x ld] or null: their seasonal strengths, NaN beyond the list
    double *work; size_t work_stride; int work_blocks;     // rows that do not fit in LDS: [work_blocks x work_stride]
};
size_t stl_period_work_stride(size_t t_rows);
int stl_period_work_blocks(size_t work_stride, int n_series);
void launch_stl_period(const StlPeriodArgs &, hipStream_t);

// Matrix profile period (periods.rs matrix_profile_period :1134-1244; matrix_profile.hip).  Bit for bit the source's arithmetic; among
// lags of equal best count the smallest wins (the source leaves that to its hash order).
constexpr size_t MPROF_MAX_ROWS = 65536;     // t_rows of a call
constexpr int MPROF_MIN_ROWS = 32;           // a shorter series fails alone (MPROF_TOO_SHORT)
constexpr int MPROF_MAX_M = 2048;            // a series whose effective subsequence length is larger fails alone (MPROF_OVER_LIMIT)
constexpr int MPROF_TILE = 64;               // rows and columns of a tile of pairs
constexpr int MPROF_KCHUNK = 16;             // steps of k whose z values a tile holds in LDS at a time
constexpr int MPROF_HOME_DOUBLES = 5504;     // the LDS a series, its profile and its index may take (43 KiB); else they live in the workspace
constexpr int MPROF_N_FIG = 6;               // period, confidence, n_motifs, subsequence_length, best_count, n_tied
constexpr int32_t MPROF_OK = 0, MPROF_TOO_SHORT = 1, MPROF_OVER_LIMIT = 2;
constexpr size_t MPROF_WORK_BYTES = (size_t)256 << 20;      // upper bound of the workspace, whatever n_series is (one slice if a slice is larger)
struct MatrixProfileArgs {
    const double *y; size_t ld; const int32_t *len; int n_series;
    size_t t_rows;               // a longer series is cut to it
    int64_t subsequence;         // 0: n / 10 of each series
    int64_t n_best;              // the exclusion zone (the reference's wrapper passes n_best on as that); 0: m / 4
    double *out_fp;              // [MPROF_N_FIG x ld]
    double *out_profile;         // [profile_rows x ld] or null: the nearest-neighbour distances, NaN beyond a series' P
    int32_t *out_index;          // [profile_rows x ld] or null: their indices, -1 beyond a series' P
    int profile_rows;            // P of a series of t_rows rows
    int32_t *status;             // [n_series] MPROF_OK / _TOO_SHORT / _OVER_LIMIT (the figures are not written unless OK)
    double *work; size_t work_stride; int work_blocks;     // means and stds, and what does not fit in LDS: [work_blocks x work_stride]
};
size_t matrix_profile_work_stride(size_t t_rows, int64_t subsequence);      // doubles per workspace slice
int matrix_profile_work_blocks(size_t work_stride, int n_series);
void launch_matrix_profile(const MatrixProfileArgs &, hipStream_t);

// Forecast accuracy metrics per group (metrics.rs mae .. coverage; metrics.hip)
constexpr int METRICS_N_FIG = 12;        // rows of `figures`, in this order:
enum { MF_MAE = 0, MF_MSE, MF_RMSE, MF_MAPE, MF_SMAPE, MF_R2, MF_BIAS, MF_RMAE, MF_MASE, MF_QUANTILE_LOSS, MF_MQLOSS, MF_COVERAGE };
constexpr int METRICS_MAX_LEVELS = 16;   // quantile levels of mqloss per call; more fail loudly
constexpr uint32_t METRICS_NEED_FORECAST = 0x3FFu, METRICS_NEED_SECOND = 0x180u;      // figures that read `forecast` / `second`
constexpr int32_t METRICS_OK = 0, METRICS_EMPTY = 1;
struct MetricsArgs {
    // element (group s, row t) of every input block at s * stride_s + t * stride_t; a block that no requested figure reads may be
    // null; with drop_nan every block that is NOT null takes part in the row filter
    const double *actual, *forecast, *second, *lower, *upper;
    const double *quant;         // level k's forecasts: the block at quant + k * stride_q
    size_t stride_s, stride_t, stride_q;
    const int32_t *len; int n_groups;
    size_t t_rows;               // a longer group is cut to it
    uint32_t mask;               // bit k: figure k is wanted
    int drop_nan;                // 1: a row with a NaN in any block is skipped and does not count
    int n_levels; double quantile; double levels[METRICS_MAX_LEVELS];
    double *figures; size_t ld;  // [METRICS_N_FIG x ld]; only the rows of `mask` and the columns s < n_groups are written
    int32_t *status;             // [n_groups] METRICS_OK, METRICS_EMPTY (no row left: every wanted figure is NaN)
    int staging;                 // -1: LDS staging when stride_t == 1 and stride_s != 1; 0: never (strided reads); 1: whenever stride_t == 1
};
void launch_metrics(const MetricsArgs &, hipStream_t);

// Conformal prediction intervals per group (conformal.rs learn / apply / evaluate; conformal.hip)
constexpr int CONFORMAL_MAX_LEVELS = 16;     // alphas per call; more fail loudly
constexpr int CONFORMAL_RESIDENT = 2048;     // keys of the longest group that is sorted in LDS; longer ones use the global workspace
constexpr int CONFORMAL_WORK_WAVES = 1024;   // waves (and workspace slices) that walk the longer groups
constexpr int CONFORMAL_N_EVAL = 5;          // rows of the evaluate figures: coverage, violation_rate, mean_width, winkler_score, n_observations
enum { CONFORMAL_SYMMETRIC = 0, CONFORMAL_ASYMMETRIC = 1, CONFORMAL_ADAPTIVE = 2 };
constexpr int32_t CONFORMAL_OK = 0, CONFORMAL_EMPTY = 1, CONFORMAL_NAN = 2, CONFORMAL_DIFFICULTY = 3;
// element (group s, row t) of every block of a call at s * stride_s + t * stride_t
struct ConformalLearnArgs {
    const double *residual;      // the residuals, or null: actual - forecast
    const double *actual, *forecast;
    const uint8_t *valid;        // null, or one byte per element: a row whose byte is 0 is dropped
    size_t stride_s, stride_t;
    const int32_t *len; int n_groups;
    size_t t_rows;               // a longer group is cut to it
    int method; int n_alphas; double alphas[CONFORMAL_MAX_LEVELS];
    double *scores_lower, *scores_upper; size_t ld;   // [n_alphas x ld]; only the columns s < n_groups are written
    double *sorted;              // null, or a block with the inputs' strides: rows 0 .. n_kept - 1 receive the sorted |residual|
    int32_t *n_kept;             // null, or [n_groups] rows kept
    int32_t *status;             // [n_groups]
    int tile;                    // keys per wave of the LDS kernel: a power of two, 64 .. CONFORMAL_RESIDENT
    uint64_t *work;              // [work_waves x work_stride] or null when t_rows <= CONFORMAL_RESIDENT
    size_t work_stride; int work_waves;
};
struct ConformalApplyArgs {
    const double *forecast, *difficulty;         // difficulty: read by the adaptive method only
    size_t stride_s, stride_t;
    const int32_t *len; int n_groups; int h_rows;            // len null: every group has h_rows steps
    const double *scores_lower, *scores_upper; size_t ld;    // [n_alphas x ld]
    int method; int n_alphas;
    double *lower, *upper; size_t stride_q;      // level k's block at + k * stride_q, the forecast's strides within it
    int32_t *status;             // [n_groups]
};
struct ConformalEvalArgs {
    const double *actual, *lower, *upper;
    size_t stride_s, stride_t;
    const int32_t *len; int n_groups; size_t t_rows;
    double alpha;
    double *figures; size_t ld;  // [CONFORMAL_N_EVAL x ld]
    int32_t *status;             // [n_groups]
};
int conformal_tile(size_t t_rows);               // the LDS tile of a batch whose longest group has t_rows rows
size_t conformal_work_stride(size_t t_rows);     // words per workspace slice (0: no workspace needed)
int conformal_work_waves(int n_groups);
void launch_conformal_learn(const ConformalLearnArgs &, hipStream_t);
void launch_conformal_apply(const ConformalApplyArgs &, hipStream_t);
void launch_conformal_evaluate(const ConformalEvalArgs &, hipStream_t);

// Data quality scores per series (quality.rs compute_data_quality without dates; quality.hip)
constexpr int QUALITY_RESIDENT = 2048;       // rows of the longest series that is sorted in LDS; longer ones use the global workspace
constexpr int QUALITY_WORK_WAVES = 1024;     // waves (and workspace slices) that walk the longer series
constexpr int QUALITY_N_FP = 5, QUALITY_N_INT = 4;
constexpr int64_t QUALITY_OK = 0, QUALITY_NAN = 2;
struct QualityArgs {
    const double *y; const uint8_t *valid;       // [t_rows x ld]; valid may be null
    size_t ld; const int32_t *len; int n_series;
    size_t t_rows;               // a longer series is cut to it
    double *out_fp;              // [QUALITY_N_FP x ld] structural, temporal, magnitude, behavioral, overall
    int64_t *out_int;            // [QUALITY_N_INT x ld] n_gaps, n_missing, is_constant (0 / 1), status (QUALITY_OK / QUALITY_NAN)
    int tile;                    // words per wave of the LDS kernel: a power of two, 64 .. QUALITY_RESIDENT
    uint64_t *work;              // [work_waves x work_stride] or null when t_rows <= QUALITY_RESIDENT
    size_t work_stride; int work_waves;
};
int quality_tile(size_t t_rows);                 // the LDS tile of a batch whose longest series has t_rows rows
size_t quality_work_stride(size_t t_rows);       // words per workspace slice (0: no workspace needed)
int quality_work_waves(int n_series);
void launch_quality(const QualityArgs &, hipStream_t);

// The 117 features per series (features.rs extract_features; features.hip): five kernels, one per family, each over every column of
// a time-major block.  Rows of out_fp and presence bits are in the byte order of the names (feature_names.inc).
constexpr int FEATURES_RESIDENT = 2048;      // rows of the longest series whose values live in LDS; longer ones use the global workspace
constexpr int FEATURES_WORK_WAVES = 256;     // waves (and workspace slices) that walk the longer series
constexpr size_t FEATURES_MAX_ROWS = (size_t)1 << 16;    // rows of a block: bounds the O(n^2) families and the workspace (256 MiB)
constexpr int FEATURES_N = 117, FEATURES_N_INT = 3;
constexpr int FEATURES_BENFORD = 9 * 309;    // the thresholds dEk, ascending
constexpr int64_t FEATURES_OK = 0, FEATURES_EMPTY = 1, FEATURES_NAN = 2;
constexpr int FEATURES_CHAINS = 0, FEATURES_SORT = 1, FEATURES_SCAN = 2, FEATURES_MATCH = 3, FEATURES_DFT = 4, FEATURES_FAMILIES = 5;
struct FeaturesArgs {
    const double *y; const uint8_t *valid;       // [t_rows x ld]; valid may be null
    size_t ld; const int32_t *len; int n_series;
    size_t t_rows;               // a longer series is cut to it
    double *out_fp;              // [FEATURES_N x ld]; NaN where the source inserts nothing
    int64_t *out_int;            // [FEATURES_N_INT x ld] presence bits 0..63, presence bits 64..116, status (written by the chains kernel)
    const double *benford;       // [FEATURES_BENFORD] correctly rounded thresholds (the scan kernel)
    int tile;                    // words of the LDS kernels: a power of two, 64 .. FEATURES_RESIDENT
    uint64_t *work;              // [work_waves x 2 work_stride] or null when t_rows <= FEATURES_RESIDENT
    size_t work_stride; int work_waves;
};
int features_tile(size_t t_rows);
size_t features_work_stride(size_t t_rows);      // words per half of a workspace slice (0: no workspace needed)
int features_work_waves(int n_series);
void launch_features(const FeaturesArgs &, hipStream_t, int families = (1 << FEATURES_FAMILIES) - 1);   // bit f: run family f

// Seasonality analysis per series (seasonality.rs detect_seasonality, analyze_seasonality, compute_trend_strength; seasonality.hip):
// the up to five strongest autocorrelation peaks, their strengths and the trend strength of every column of a time-major block
constexpr int SEASONALITY_LDS_ROWS = 5120;   // rows of the longest block whose working buffers live in LDS (63,504 bytes of it)
constexpr int SEASONALITY_LONG_GRID = 1024;  // workgroups (and workspace slices) of the global-memory variant
constexpr int SEASONALITY_TOP = 5;           // periods kept
constexpr int SEASONALITY_N_INT = 8, SEASONALITY_N_FP = 12;
constexpr int32_t SEASONALITY_OK = 0, SEASONALITY_SHORT = 1;
struct SeasonalityArgs {
    const double *y; const uint8_t *valid;       // [t_rows x ld]; valid may be null
    size_t ld; const int32_t *len; int n_series;
    int t_rows;                  // a longer series is cut to it
    int max_period;              // <= 0: n / 2 of each series
    int32_t *out_int;            // [SEASONALITY_N_INT x ld] periods[0..4], n_periods, primary_period, status
    double *out_fp;              // [SEASONALITY_N_FP x ld] strengths[0..4], acf[0..4], seasonal_strength, trend_strength
    double *work;                // [grid x seasonality_work_stride] or null when t_rows <= SEASONALITY_LDS_ROWS
};
size_t seasonality_work_stride(int t_rows);      // doubles per workgroup: the centred series, its zero tail and the lag sums
size_t seasonality_work_doubles(int n_series, int t_rows);     // 0: the block fits the LDS variant
void launch_seasonality(const SeasonalityArgs &, hipStream_t);

// Walk-forward backtest on a resident block (_ts_backtest_native's folds, cut by position; backtest.hip).  Pair p = s * n_folds + f
// is series s in fold f; ld_pairs is n_pairs rounded up to 64.
enum { BT_MAE = 0, BT_MSE = 1, BT_MAPE = 2, BT_SMAPE = 3, BT_BIAS = 4, BT_R2 = 5, BT_COVERAGE = 6, BT_RMSE = 7 };
struct BacktestFoldPos { int32_t train_start, train_end, test_start, test_end; };      // inclusive positions, all >= 0
struct BacktestArgs {
    const double *y; size_t ld_src;              // the source block [t_rows x ld_src]
    const int32_t *len; int n_series;            // [n_series]; a length above t_rows is cut to it
    size_t t_rows;
    const BacktestFoldPos *folds; int n_folds;   // [n_folds], in device memory
    int n_pairs; size_t ld_pairs;
    // expand
    size_t t_train; double *y_out;               // [t_train x ld_pairs]
    int32_t *len_pairs, *n_test;                 // [ld_pairs]
    // collect and score
    int h;
    const int32_t *status;                       // [n_pairs] of the batch run
    const double *yhat, *lower, *upper;          // [n_pairs x h] series-major; lower / upper may be null (coverage is then NaN)
    double *actual, *error, *abs_error;          // [n_pairs x h]
    uint8_t *valid;                              // null, or [n_pairs x h]: 1 where the row exists
    int32_t *n_rows;                             // [n_pairs]
    int metric; double *scores;                  // BT_*; null, or [n_folds]
};
void launch_backtest_expand(const BacktestArgs &, hipStream_t);
void launch_backtest_collect(const BacktestArgs &, hipStream_t);     // collect, then (scores != null) the fold scores

// Aggregation up a key hierarchy (ts_aggregate_hierarchy.cpp:246-386; hierarchy.hip).  Output column c is the sum over the series
// members[col_offsets[c] .. col_offsets[c + 1]) IN THAT ORDER, per position of a common date grid; first[s] is the grid position of
// series s' row 0.
enum { HIER_ROUTE_AUTO = 0, HIER_ROUTE_LANE = 1, HIER_ROUTE_TILE = 2 };
constexpr int64_t HIER_FIRST_MAX = (int64_t)1 << 61;    // |first[s]| above it marks the column invalid (position arithmetic stays in int64)
constexpr int64_t HIER_SPAN_MAX = (int64_t)1 << 30;      // rows of an output column
// columns with at least this many members take the tile route under HIER_ROUTE_AUTO.  Measured (profiles/hierarchy_m5.txt): on plans
// of equal-width columns the tile route is the faster one from 16 members on while there are enough columns to fill the chip with
// lanes, and the M5 plans give the same time for every threshold from 2 to 1,024 (their wide columns have 3,049 members or more,
// their narrow ones 10 or fewer); 64, one full tile, lies inside both ranges.
constexpr int HIER_TILE_MIN_MEMBERS = 64;
struct HierarchyArgs {
    const double *y; size_t ld;                  // the source block [t_rows x ld]
    const uint8_t *valid, *present;              // null, or [t_rows x ld]: valid 0 = NULL (adds 0.0), present 0 = no row there
    const int32_t *len; const int64_t *first;    // [n_series]; first may be null (all 0); a length above t_rows is cut to it
    int n_series; size_t t_rows;
    const int32_t *col_offsets, *members;        // CSR plan: [n_out + 1], [nnz]
    int n_out, nnz;
    int route, tile_min;                         // HIER_ROUTE_*; member count from which HIER_ROUTE_AUTO takes the tile route
    size_t t_out, ld_out;
    double *y_out; uint8_t *present_out;         // [t_out x ld_out]; null for the sizing call (present_out may be null alone)
    int32_t *len_out; int64_t *first_out;        // [n_out]
};
void launch_hierarchy(const HierarchyArgs &, hipStream_t);     // spans, then (y_out != null) the two routes

// Reconciliation of the forecasts of a hierarchy (DESIGN.md section 3 "Reconciliation"; reconcile.hip)
enum { RECONCILE_BOTTOM_UP = 0, RECONCILE_OLS = 1, RECONCILE_WLS_STRUCT = 2, RECONCILE_WLS_VAR = 3 };
enum { RECONCILE_TRAILING_FMA = 0, RECONCILE_TRAILING_MFMA = 1 };
constexpr int32_t RECONCILE_NONE = INT32_MAX;          // ReconcileFactorArgs::info: nothing to report
struct ReconcilePlan {                                 // everything in device memory
    const int32_t *col_offsets, *members; int n_out, nnz, n_series;      // the aggregation plan
    const int32_t *bottom_col;                         // [n_series] the column whose member list is exactly [s]
    const int32_t *agg_cols; int n_agg;                // [n_agg] ascending: the columns with members that are no bottom column
    const int32_t *leaf_offsets, *leaf_aggs; int n_leaf;      // the transposed plan: per series the aggregates (indices into agg_cols) that hold it
    const double *weights;                             // [n_out], null: all 1
};
struct ReconcileFactorArgs {
    ReconcilePlan p;
    double *L; size_t ld_a;                            // [n_agg x ld_a]: M, then its Cholesky factor, in the lower triangle; the rest is not touched
    int32_t *info;                                     // [2]: the smallest column with a bad weight, the first row with a pivot that is not positive
    int trailing;                                      // RECONCILE_TRAILING_*
};
struct ReconcileApplyArgs {
    ReconcilePlan p;
    int method;
    const double *base; double *out; size_t stride_s, stride_t, n_rows;  // element (column c, row t) at c * stride_s + t * stride_t
    const double *L; size_t ld_a;
    double *work; size_t ld_work;                      // [n_rows x ld_work], ld_work >= n_agg: the residuals, then lambda
    int32_t *row_status;                               // [n_rows]
};
void launch_reconcile_factor(const ReconcileFactorArgs &, hipStream_t);
void launch_reconcile_apply(const ReconcileApplyArgs &, hipStream_t);
// the steps of the two launches above, one by one, for reconcile_mint.hip: M = diag(w_a) + A diag(w_b) A^T into the lower triangle;
// the panels of the Cholesky factor (info[1]: the first pivot that is not positive); row_status; work = base_a - chain(base_b);
// the two substitutions on work; the aggregates of out as the chain over out's own bottoms
void launch_reconcile_assemble(const ReconcileFactorArgs &, hipStream_t);
void launch_reconcile_panels(const ReconcileFactorArgs &, hipStream_t);
void launch_reconcile_status(const ReconcileApplyArgs &, hipStream_t);
void launch_reconcile_incoherence(const ReconcileApplyArgs &, hipStream_t);
void launch_reconcile_substitute(const ReconcileApplyArgs &, hipStream_t);
void launch_reconcile_aggregates(const ReconcileApplyArgs &, hipStream_t);

// MinT with the shrinkage covariance (DESIGN.md section 3 "MinT-shrink"; reconcile_mint.hip)
enum { MINT_INFO_RESIDUAL = 0, MINT_INFO_VARIANCE = 1, MINT_INFO_WEIGHT = 2, MINT_INFO_PIVOT = 3 };    // ReconcileMintArgs::info
struct ReconcileMintArgs {
    ReconcilePlan p;                                   // (p.weights is not read: the variances stand in their place)
    const double *res; size_t res_stride_s, res_stride_t; int n_res;     // residual (column c, row t) at c * res_stride_s + t * res_stride_t
    double *var;                                       // [n_out] v_c of every column with members, 0.0 for an empty one
    double *rsd, *f4col;                               // [n_out] scratch: 1 / sqrt(v_c); the column sums of xs^4 (estimating only)
    double *E; size_t ld_e;                            // [n_res x ld_e] the residuals' incoherence
    double *gram; int gram_splits;                     // [gram_splits x n_res x n_res] partial Gram matrices, then [2 x tiles] partial sums (host_reconcile_mint.hpp sizes both); null: lambda is given
    double *lambda; double lambda_in;                  // [1] device: where the estimate goes, or (gram null) lambda_in is written
    double *L; size_t ld_a;
    int32_t *info;                                     // [4] MINT_INFO_*
    int trailing, ete;                                 // RECONCILE_TRAILING_* of the factor's trailing update and of the E^T E update
};
struct ReconcileMintApplyArgs {
    ReconcileApplyArgs a;                              // forecast block, factor, work [n_rows x ld_work] (r, then mu), out, row_status
    const double *res; size_t res_stride_s, res_stride_t; int n_res;
    const double *var, *E; size_t ld_e;
    double lambda;
    double *g;                                         // [n_rows x n_res] scratch: g = E mu
};
void launch_reconcile_mint_factor(const ReconcileMintArgs &, hipStream_t);
void launch_reconcile_mint_apply(const ReconcileMintApplyArgs &, hipStream_t);

// The choice of a method per series from backtest scores (DESIGN.md section 3 "Selection"; select.hip)
constexpr int SELECT_MAX_METHODS = 16;                 // the median's values and the partition's counters live in registers / LDS rows of 16
enum { SELECT_PICK = 0, SELECT_MEAN = 1, SELECT_MEDIAN = 2, SELECT_INVERSE_SCORE = 3 };
struct SelectWinnerArgs {
    const double *scores; size_t ld;                   // [n_methods x ld]: method m of series s at m * ld + s
    const int32_t *score_status;                       // [n_methods x n_series]: 0 = the score counts
    int n_methods, n_series, fallback;                 // fallback in [-1, n_methods)
    int32_t *winner; double *best_score; uint8_t *from_fallback;      // [n_series]
    int32_t *counts; size_t n_wg;                      // [select_counts_size(n_series, n_methods)] scratch; n_wg = select_workgroups(n_series)
    int32_t *offsets, *members;                        // [n_methods + 1], [n_series]
};
struct SelectMoveArgs {                                // gather (block) and scatter (results) by members[off .. off + n_m)
    const int32_t *members; size_t off, n_m; int n_series;
    // gather
    const double *y; size_t ld_src; const int32_t *len; size_t t_rows;
    double *y_out; size_t ld_m; int32_t *len_out;      // [t_rows x ld_m], [ld_m]
    // scatter
    int h;
    const double *yhat_m, *lower_m, *upper_m; const int32_t *code_m, *status_m;      // the sub-batch: [n_m x h], [n_m]
    const int32_t *winner;                             // null, or [n_series]: rows of winner -1 become NaN / INSUFFICIENT_DATA
    double *yhat, *lower, *upper; int32_t *model_code, *status;          // [n_series x h], [n_series]; each may be null
};
struct SelectCombineArgs {
    const double *const *blocks;                       // [n_methods] device pointers, the table itself in device memory: [n_rows x h] each
    int n_methods, h, mode;                            // SELECT_*
    size_t n_rows, group_div;                          // row r belongs to group r / group_div
    const int32_t *member_status;                      // [n_methods x n_rows]
    const int32_t *winner;                             // SELECT_PICK: [groups]
    const double *weights; size_t ld_w;                // SELECT_INVERSE_SCORE: the scores [n_methods x ld_w]
    double *out; int32_t *row_status;                  // [n_rows x h], [n_rows] (may be null)
};
size_t select_workgroups(size_t n_series);
size_t select_counts_size(size_t n_series, int n_methods);
void launch_select_winner(const SelectWinnerArgs &, hipStream_t);      // winners, the scan of the workgroup counts, the partition
void launch_select_gather(const SelectMoveArgs &, hipStream_t);
void launch_select_scatter(const SelectMoveArgs &, hipStream_t);       // the scatter, then (winner != null) the rows nobody won
void launch_select_combine(const SelectCombineArgs &, hipStream_t);

// ARIMAX: exogenous regressors (fit_exog.hip)
constexpr int EXOG_MAX_REGRESSORS = 8;   // regressors per call; more fail loudly (COMPUTATION_ERROR)
constexpr int32_t MODEL_CODE_ARIMAX = 50; // model_code of a series forecast by the ARIMAX path (model_name "ARIMAX")
struct ExogArgs {
    const double *y; size_t ld; const int32_t *len; int n_series;
    int k, h;                    // regressors (1 .. EXOG_MAX_REGRESSORS), horizon
    size_t t_rows;               // rows of every regressor's slice of x (>= the longest series)
    const double *x;             // [k x t_rows x ld] historical values, x[(j * t_rows + t) * ld + s]
    const double *f;             // [k x h x ld] future values, f[(j * h + i) * ld + s]
    double *yhat;                // [n_series x h]
    int32_t *status;             // [n_series] 0 for every series forecast here
    int32_t *model_code;         // [n_series] MODEL_CODE_ARIMAX
    double *b0, *beta;           // [ld] intercept, [k x ld] coefficients (0.0 where the regressor is not used)
    uint32_t *used;              // [ld] bit j: regressor j is used (not aliased)
};
void launch_exog_arimax(const ExogArgs &, hipStream_t);

struct IntervalArgs {
    int n_series, h;
    const double *yhat, *sd;
    const int32_t *status;
    double z;
    double *lower, *upper;
};

// ETS fit kernels, one per (spec id, ring variant).  ring: 0 = none / VGPR ring for the
// compile-time period given, -1 = LDS ring.  Returns NULL when not instantiated.
typedef void (*FitLaunchFn)(const FitArgs &, hipStream_t);
struct FitLaunchers { FitLaunchFn round_seq, round_spec, round_spec2, round_auto, final; size_t nm_scratch_per_wg; FitLaunchFn round_k4, round_auto_k4; };   // sequential / speculative / two-level speculative rounds, all three behind a device-side choice, final pass; doubles of global simplex scratch per workgroup (0: the simplex rests in LDS); the K4 forms of round_seq / round_auto (additive class, NULL otherwise: ets_fit_kernel.hpp)
// `m`: the period (7 and 12 have compile-time variants), or ETS_PERLANE_LDS / ETS_PERLANE_HBM for the round kernels of a merged
// batch of several periods (per-lane period, ring in LDS / in HBM scratch sized by the batch's largest period)
constexpr int ETS_PERLANE_LDS = -3, ETS_PERLANE_HBM = -4;
// `yt`: storage type of the block the kernels stream (ets_device.hpp YT_F64 / YT_F32 / YT_U16); every entry is NULL when the
// combination is not instantiated (compact types x per-lane period variants)
FitLaunchers ets_fit_launcher(int spec_id, int m, int yt = 0);
// Group rounds (launch_fit_slots, tune group_launch): round r of several specs of one class in ONE launch.  Slot k owns the
// workgroups [start[k], start[k + 1]) and runs the round of spec[k] on tab[k] -- the same body as that spec's own round kernel, with
// the driver picked per slot on the device (SPEC 3; k4[k] != 0: its K4 form).  The classes: the damped multiplicative-trend specs,
// the additive class (EtsCfg::ADDITIVE) and the rest of the general class.
constexpr int GROUP_MAX_SLOTS = 16;
enum { GROUP_DAMPED_MUL = 0, GROUP_GENERAL = 1, GROUP_ADDITIVE = 2, N_GROUP_CLASSES = 3 };
struct GroupRoundArgs {
    int n_slots;
    int spec[GROUP_MAX_SLOTS];
    int k4[GROUP_MAX_SLOTS];
    int start[GROUP_MAX_SLOTS + 1];     // prefix of the slots' one-wave workgroups; start[n_slots] = the launch's grid
};
// tab: [n_slots] this round's FitArgs of the slots, in device memory; m: the batch's period (1: none).  NULL: the combination is not
// instantiated (a merged batch of several periods, or an experiment build whose round kernels differ in residency or layout)
typedef void (*GroupLaunchFn)(const FitArgs *tab, const GroupRoundArgs &g, int m, hipStream_t);
GroupLaunchFn ets_group_launcher(int group_class, int m, int yt);
inline int ets_group_class(int spec_id)
{
    if (spec_id < 0 || spec_id >= 30 || (spec_id >= 15 && spec_id % 3 == 1)) return -1;      // (M,*,A: not a model)
    const int e = spec_id / 15, ti = (spec_id % 15) / 3, s = spec_id % 3;
    if (ti == 4) return GROUP_DAMPED_MUL;
    return (e == 0 && ti < 3 && s < 2) ? GROUP_ADDITIVE : GROUP_GENERAL;
}
FitLaunchers classic_fit_launcher(int kind, int m);          // fit_classic.hip: the SES / Holt / Holt-Winters / SeasonalES family on the round kernels (final = NULL)
struct ClassicArgs;
void launch_classic_final(int kind, const FitArgs &a, const ClassicArgs &c, hipStream_t stream);

// ... of every slot of a group round (launch_fit_slots) in one launch each: slot k in blockIdx.y (compaction) / blockIdx.z (gather).
// Each slot keeps its own map, counters and block; the launches are sized by the slots' largest counts and stride over the columns.
struct GroupCompactArgs {
    int n_slots, n_series;
    const int32_t *prev[GROUP_MAX_SLOTS], *n_prev[GROUP_MAX_SLOTS], *done[GROUP_MAX_SLOTS];
    int32_t *next[GROUP_MAX_SLOTS], *n_next[GROUP_MAX_SLOTS], *n_clear[GROUP_MAX_SLOTS];
};
void launch_group_compact(const GroupCompactArgs &g, hipStream_t);
// zero[k][0..3): the rotating counters of every slot, before the run's first compaction
void launch_group_zero3(int n, int32_t *const *zero, hipStream_t);
struct GroupGatherArgs {
    int n_slots, t_max, elem_bytes;
    const void *y; size_t ld;
    const int32_t *series_of[GROUP_MAX_SLOTS], *n_active[GROUP_MAX_SLOTS];
    void *out[GROUP_MAX_SLOTS]; size_t ld_out[GROUP_MAX_SLOTS]; int cap[GROUP_MAX_SLOTS];
};
void launch_group_gather(const GroupGatherArgs &g, int n_cols_max, hipStream_t);
// compaction of the unfinished problems: series_next[0..n_next) = the series of the previous map whose done flag
// is 0 (one ballot + one atomic per wave; the order of the survivors is not preserved, results do not depend on it)
void launch_compact(const int32_t *series_prev, const int32_t *n_prev, int n_series, const int32_t *done,
                    int32_t *series_next, int32_t *n_next, hipStream_t, int32_t *n_clear = nullptr);
// out[t * ld_out + p] = y[t * ld + series_of[p]] for p < *n_active, t < t_max
// seasonal period detection (first / strongest autocorrelation peak, 0 = none) of every column of a time-major block; series of up
// to DETECT_LDS_ROWS observations are held in LDS, longer ones in `scratch` (detect_scratch_doubles doubles, else unused)
constexpr int DETECT_LDS_ROWS = 8192;        // 1.5 x 8 B x 8,192 = 96 KB of the CU's 160 KB
constexpr int DETECT_LONG_GRID = 1024;       // workgroups of the scratch variant (each owns 1.5 t_rows doubles of scratch)
size_t detect_scratch_doubles(int n_series, int t_rows);
void launch_detect_periods(const double *y, size_t ld, const int32_t *len, int n_series, int t_rows, double *scratch, int32_t *period,
                           double *best_acf, hipStream_t stream);
// `cap`: columns `out` has room for -- the copy is skipped (the round kernel then indexes `y` by series) while more problems run
// `elem_bytes`: 8 (fp64 block), 4 or 2 (compact copy: ld / ld_out still count columns)
void launch_gather_columns(const void *y, size_t ld, const int32_t *series_of, const int32_t *n_active, int n_series,
                           int t_max, void *out, size_t ld_out, hipStream_t stream, int cap, int elem_bytes = 8);
// Compact copies of the time-major block for the round kernels (round 6): out32[t * ld + s] = (float)y, out16 = (uint16_t)y for every
// cell of the block, and misfit[0] / misfit[1] += the OBSERVATIONS (t < len[s]) that do not survive the round trip through float /
// uint16_t exactly.  A batch streams a compact copy only when its counter is zero (host_api.hip): bit-identical by construction.
void launch_compact_block(const double *y, size_t ld, const int32_t *len, int n_series, int t_rows, float *out32, unsigned short *out16,
                          unsigned int *misfit, hipStream_t stream);

// AutoARIMA (arima.hip): prep (D, d, differenced block), stepwise CSS search (advance / fit sweeps), forecast + integration
struct ArimaArgs {
    const double *y; size_t ld; const int32_t *len; int n_series;
    int m, h;
    int t_max;                          // rows of y (longest series of the batch)
    void *ws; size_t ws_bytes;          // search workspace, arima_workspace_bytes(n_series, t_max) bytes
    int32_t *wlen, *d, *D;              // [ld]
    double *wmean, *wsd, *last_d0, *last_d1;
    int32_t *order;                     // [5 x ld] p, q, P, Q, constant
    double *xbest;                      // [6 x ld] optimiser coordinates of the selected model
    double *aicc;
    int32_t *status, *evals, *passes, *models;
    double *yhat;                       // [n_series x h]
    int32_t *model_code;                // 1000000 + p*1e5 + d*1e4 + q*1e3 + P*100 + D*10 + Q
    int trace;                          // debugging: the refit kernel prints per-wave timings (ANOFOX_HIP_TUNE arima_trace=1|2)
    double lookahead, spec_factor;      // schedule knobs of the search (host_api.hip Tunables: lookahead once the queue fits the resident lanes
    int lookahead_depth;                //   this many times over; four lanes per problem below spec_factor x the resident groups)
    const std::atomic<int> *concurrent; // host only: AutoARIMA runs in flight in this process (the parts of a call with detected periods run side by side)
    double shared_chunk_rounds;         // ... with more than one, a fit launch takes at most this many rounds of the resident lanes (tune
                                        // arima_shared_chunk_rounds; 0 = whole queue): see launch_arima
    int prep_lanes;                     // series per wave of arima_prep_kernel (tune arima_prep_lanes; default 64 = one full wave per 64 series)
    int queue_sort;                     // order of the fit queue (tune arima_queue_sort; arima.hip ar_bucket): 0 as emitted, 1..3 by series within a bucket
    int refit_budget;                   // exact-likelihood refit: evaluations per series in the sequential launch before the speculative one takes over (0: one launch)
    double *long_scratch;               // seasonal period above 24: HBM scratch of arima_long_scratch_doubles() doubles (rings, polynomials), else NULL
    int ml_refit;                       // exact-likelihood (Kalman / Chandrasekhar) refit of the selected models; 0 keeps the CSS estimates
    const int32_t *m_col;               // [ld] merged batch of several LONG periods (all above 24): the period of every series; `m` is then the
                                        // largest (scratch sizes); NULL = one period `m` for the whole batch
};
size_t arima_workspace_bytes(int n_series, int t_max);
size_t arima_long_scratch_doubles(int n_series, int m, int max_fit_waves);   // 0 for periods whose rings live in LDS (m <= 24)
int arima_max_fit_waves();                                                  // resident waves of the fit kernels (what the scratch is sized for)
int launch_arima(const ArimaArgs &, hipStream_t);   // returns the number of kernel launches; synchronises the stream between sweeps

// dm_recip (det_math.hpp) against the compiled division on `n` generated operands of the admissible domain: the number of operands
// whose quotients differ (0 is the claim), ~0 when the device could not run it; *first_bad: one of them
unsigned long long recip_selftest(unsigned long long n, unsigned long long seed, double *first_bad, hipStream_t stream);

// the elementary functions of det_math.hpp / det_trig.hpp at the caller's operands (host arrays of n doubles; y may be NULL, out2 is
// SINCOS's cosine): fn is an AnofoxHipMathFn, block_threads 64 or 256 (the host entry checks both).  False when the device could not run it
bool math_selftest(int fn, const double *x, const double *y, unsigned long long n, int block_threads, double *out, double *out2, hipStream_t stream);

// Bootstrap sample paths and their quantiles (DESIGN.md section 3 "Sample paths"; paths.hip).  Element (series s, row t) of the
// point block and of the pool is at s * stride_s + t * stride_t, as for the metrics entries.
enum { PATHS_CUMULATIVE = 0, PATHS_INDEPENDENT = 1 };
enum { PATHS_ROUTE_AUTO = 0, PATHS_ROUTE_LANE = 1 };
constexpr int PATHS_MAX_PATHS = 2048;                  // paths per call: one column of keys is 16 KiB of LDS
constexpr int PATHS_MAX_LEVELS = 16;                   // quantile levels per call
constexpr size_t PATHS_MAX_POOL_ROWS = (size_t)1 << 20; // the index rule has no rejection step: its bias is at most n / 2^32
constexpr size_t PATHS_MAX_ROWS = (size_t)1 << 30;      // n_paths * horizon: the row limit of the hierarchy entry
constexpr int32_t PATHS_OK = 0, PATHS_EMPTY = 1, PATHS_NAN = 2, PATHS_RAGGED = 3;
struct PathsArgs {
    const double *point; size_t point_stride_s, point_stride_t;      // [n_series x horizon]
    const double *pool; size_t pool_stride_s, pool_stride_t;         // [n_series x pool_rows]
    const int32_t *pool_len;                     // [n_series], null: every pool has pool_rows rows; cut to [0, pool_rows]
    int pool_rows, n_series, horizon, n_paths;
    int mode, joint;                             // PATHS_*; joint: one pool row per (path, step) for all series
    uint32_t key0, key1;                         // the seed's low and high word
    double *paths; size_t ld_out;                // [n_paths * horizon x ld_out], row p * horizon + k
    int32_t *status;                             // [n_series]
    int path_groups;                             // set by launch_paths: groups of 4 paths a tile of 64 series is cut into
};
struct PathQuantilesArgs {
    const double *paths; size_t ld;              // [n_paths * horizon x ld]
    int n_cols, horizon, n_paths;
    int n_levels; double levels[PATHS_MAX_LEVELS];
    double *out;                                 // [n_levels x n_cols x horizon]
    int32_t *status;                             // [n_cols]
};
void launch_paths(const PathsArgs &, hipStream_t);                     // the statuses, then the paths
void launch_path_quantiles(const PathQuantilesArgs &, hipStream_t);

// Sample paths simulated from fitted ETS models (DESIGN.md section 3 "Model paths"; ets_paths.hip).  `info` [8 x ld] and `states`
// [(2 + max(m, 1)) x ld] are the blocks of the inspection pass (FitArgs::insp_info / insp_states); the pool is addressed as PathsArgs'.
enum { ETS_PATHS_GAUSSIAN = 0, ETS_PATHS_BOOTSTRAP = 1 };
constexpr int32_t ETS_PATHS_NO_MODEL = 4;              // beside PATHS_OK / _EMPTY / _NAN / _RAGGED
constexpr int ETS_PATHS_MAX_PERIOD = 2048;
constexpr int ETS_PATHS_MAX_RING = 128;                // R = min(m, horizon): 64 lanes x R x 8 bytes of LDS per wave within 64 KiB
struct EtsPathsArgs {
    const int32_t *spec;                         // [n_series] error * 15 + trend * 3 + season
    const double *info, *states; size_t ld;      // rows alpha, beta, gamma, phi, -, -, -, sse; rows level, growth, seasonal state of phase j
    int m;                                       // the batch's seasonal period
    const int32_t *lengths;                      // [n_series] observations: step k has phase (n + k) % m
    int innovations;                             // ETS_PATHS_*
    const double *pool; size_t pool_stride_s, pool_stride_t;
    const int32_t *pool_len;
    int pool_rows, joint;
    int n_series, horizon, n_paths;
    uint32_t key0, key1;
    double *paths; size_t ld_out;                // [n_paths * horizon x ld_out], row p * horizon + k
    int32_t *status, *n_broken;                  // [n_series]
    int path_groups, ring, waves;                // set by launch_ets_paths: groups of `waves` paths per tile, R, waves per workgroup
};
int ets_paths_waves(int ring);                                              // waves per workgroup of the simulation kernel at R = ring
void launch_ets_paths(const EtsPathsArgs &, hipStream_t);                   // the statuses, the paths, then n_broken
// pool[t * ld + s] = y - fitted (additive error) or (y - fitted) / fitted (multiplicative) for t < lengths[s]; pool_len[s] = lengths[s]
// (0 for a spec that is none of the project's)
void launch_ets_innovations(const double *y, const double *fitted, size_t ld, const int32_t *lengths, const int32_t *spec, int n_series,
                            int t_rows, double *pool, int32_t *pool_len, hipStream_t);
// spec[s] = status[s] == 0 ? (auto_ets ? model_code[s] - 100 : explicit_spec) : -1
void launch_ets_spec_of(const int32_t *model_code, const int32_t *status, int auto_ets, int explicit_spec, int n_series, int32_t *spec, hipStream_t);
void launch_fill_f64(double *p, size_t n, double value, hipStream_t);

// Sample paths simulated from fitted ARIMA models (DESIGN.md section 3 "ARIMA paths"; arima_paths.hip).  `orders` int32 [8 x ld] (rows
// p, d, q, P, D, Q, has_constant, n_diff) and `coef` fp64 [16 x ld] (rows phi 1..5, theta 1..5, Phi 1..2, Theta 1..2, constant, aicc)
// are the fit blocks; `resid` [t_rows x ld] is compacted: row j of a column is the residual of differenced index p + m P + j.
enum { ARIMA_PATHS_GAUSSIAN = 0, ARIMA_PATHS_BOOTSTRAP = 1 };
constexpr int32_t ARIMA_PATHS_NO_MODEL = 4;            // beside PATHS_OK / _EMPTY / _NAN / _RAGGED
constexpr int ARIMA_PATHS_MAX_PERIOD = 2048;
constexpr int ARIMA_PATHS_MAX_LDS_ROWS = 128;          // 2 min(h, 2 m + 5) + (m < h ? m : 0) rows of 64 lanes x 8 bytes per wave within 64 KiB
struct ArimaPathsArgs {
    const int32_t *orders; const double *coef; size_t ld;
    const double *y; const int32_t *lengths; int t_rows;      // the series block [t_rows x ld] and its lengths (cut to t_rows)
    const double *resid; const int32_t *resid_len; const double *sigma;
    int m, innovations, joint, pool_rows;        // ARIMA_PATHS_*; joint: draw j < pool_rows takes residual row nu - pool_rows + j of every series
    int n_series, horizon, n_paths;
    uint32_t key0, key1;
    double *paths; size_t ld_out;                // [n_paths * horizon x ld_out], row p * horizon + k
    int32_t *status, *n_broken;                  // [n_series]
    int waves;                                   // developer knob: waves per workgroup of the simulation kernel, 0 = as many as the LDS takes
    int path_groups, ring, yring;                // set by launch_arima_paths
};
int arima_paths_lds_rows(int m, int horizon);                              // the LDS rows of a wave
int arima_paths_waves(int lds_rows);                                       // waves per workgroup of the simulation kernel
void launch_arima_paths(const ArimaPathsArgs &, hipStream_t);              // the statuses, the paths, then n_broken
void launch_arima_innovations(const int32_t *orders, const double *coef, size_t ld, const double *y, const int32_t *lengths, int t_rows, int m,
                              int n_series, double *resid, int32_t *resid_len, double *sigma, hipStream_t);
// the batch's search state (arima.hip ArimaArgs: order [5 x ld], d, D, wlen, xbest [6 x ld], aicc) -> the two fit blocks
void launch_arima_fit_state(const int32_t *status, const int32_t *model_code, const int32_t *order, const int32_t *d, const int32_t *D,
                            const int32_t *wlen, const double *x, const double *aicc, size_t ld, int n_series, int32_t *orders, double *coef,
                            hipStream_t);

// Scores of a block of sample paths (DESIGN.md section 3 "Path scores"; path_scores.hip).  Element (column c, step k) of `actual` is
// at c * actual_stride_c + k * actual_stride_k; a NaN there drops the step.
constexpr int32_t PATH_SCORES_OK = 0, PATH_SCORES_NO_ACTUAL = 1, PATH_SCORES_NAN = 2;
struct PathScoresArgs {
    const double *paths; size_t ld;              // [n_paths * horizon x ld]
    int n_cols, horizon, n_paths;
    const double *actual; size_t actual_stride_c, actual_stride_k;
    int n_levels; double levels[PATHS_MAX_LEVELS];
    double *crps;                                // [n_cols x horizon] or null
    int32_t *below, *equal;                      // [n_cols x horizon] or null
    double *quantiles;                           // [n_levels x n_cols x horizon] or null
    double *column; size_t ld_column;            // [(2 + n_levels) x ld_column]: crps_mean, n_steps, pinball_l; or null
    int32_t *status;                             // [n_cols]
};
struct PathEnergyArgs {
    const double *paths; size_t ld;              // [n_paths * horizon x ld]
    int col_begin, col_end, horizon, n_paths;
    const double *actual; size_t actual_stride_c, actual_stride_k;
    double *workspace;                           // [2 x n_paths x horizon]: D1, D2
    double *es;                                  // [horizon]
    double *summary;                             // [2]: es_mean, es_steps
};
void launch_path_scores(const PathScoresArgs &, hipStream_t);
void launch_path_energy(const PathEnergyArgs &, hipStream_t);   // the rows, the steps, the mean

// Scaled, weighted scores of a hierarchy (DESIGN.md section 3 "Scaled scores"; scaled_scores.hip)
constexpr int32_t SCALE_OK = 0, SCALE_SHORT = 1, SCALE_NAN = 2, SCALE_CONSTANT = 3;
constexpr int SCALED_MAX_LOSS = 16;                    // loss rows per call: the project's level limit
struct ScaleArgs {
    const double *y; size_t ld;                  // [t_rows x ld] time-major, left-aligned
    const double *w_src;                         // the block the tail is summed over, laid out as y (never null: y itself by default)
    const int32_t *len;                          // [n_cols], cut to [0, t_rows]
    int n_cols, t_rows, lag, tail_rows, trim;
    double *out; size_t ld_out;                  // [4 x ld_out]: msd, mad, n_terms, tail
    int32_t *first, *status;                     // [n_cols]
};
struct WeightedScoresArgs {
    const double *loss; size_t ld;               // [n_loss x ld]
    const double *scale, *weight;                // [n_cols]
    const int32_t *col_status;                   // [n_cols] or null
    const int32_t *ranges;                       // [n_ranges x 2]
    int n_cols, n_loss, n_ranges, transform;     // 0: loss / scale; 1: sqrt(loss / scale)
    double *scaled;                              // [n_loss x ld] or null
    double *score, *weight_sum;                  // [n_ranges x n_loss]
    int32_t *left;                               // [n_ranges x n_loss]
    double *total;                               // [n_loss + 1]
};
void launch_scale(const ScaleArgs &, hipStream_t);
void launch_weighted_scores(const WeightedScoresArgs &, hipStream_t);   // the cells, the ranges, the totals

void launch_prep(const PrepArgs &, hipStream_t);
void launch_select(const SelectArgs &, hipStream_t);
void launch_classic(int kind, const ClassicArgs &, hipStream_t);
void launch_simple(const SimpleArgs &, hipStream_t);
void launch_intervals(const IntervalArgs &, hipStream_t);

} // namespace anofox
