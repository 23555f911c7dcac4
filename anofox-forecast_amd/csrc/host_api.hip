// host_api.hip -- the C-ABI host layer of the MI355X backend (include/anofox_fcst_hip.h).
//
// Replaces crates/anofox-fcst-ffi (lib.rs:3344-3550 anofox_ts_forecast, :5900-5930 free) and the
// wrapper decisions of crates/anofox-fcst-core/src/forecast.rs:512-733.  One batch = one
// time-major fp64 block in HBM; the per-series fit/forecast arithmetic runs ONLY on the GPU
// (kernels.hip, fit_*.hip).  There is no CPU fallback: without a HIP device every entry point
// fails with INTERNAL_ERROR.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cctype>
#include <atomic>
#include <memory>
#include <unordered_map>
#include <chrono>
#include <cmath>
#include <condition_variable>
#include <mutex>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <map>
#include <stdexcept>
#include <string>
#include <system_error>
#include <thread>
#include <vector>

#include "classic_device.hpp"
#include "host_semantics.hpp"
#include "kernels.hpp"

using namespace anofox;

namespace {

constexpr int TINY_BATCH_PROBLEMS = 1024;   // (series x specs) up to which every problem runs on a wave of its own in one launch

#include "host_resources.hpp"     // HipFail / HIPCHECK, the tunables, DeviceGuard, the device / pinned / stream caches, the device list
#include "host_scratch.hpp"       // Scratch (a call's device blocks), the shape and packing of a batch of series, the _device entry's checks and launch
#include "host_parts.hpp"         // how an auto-detected batch is cut into device batches (PartPlan), and how a batch's results reach the caller's arrays
#include "host_reconcile_plan.hpp" // the host-only planner of the reconciliation entries (bottom columns, aggregates, the transposed plan)
#include "host_reconcile_mint.hpp" // the host-only checks and workspace sizes of the MinT-shrink entries
#include "host_select_plan.hpp"   // the host-only logic of the selection entries (method table checks, criterion and mode names, sub-batch shapes)
#include "host_paths_plan.hpp"    // the host-only checks of the sample-path entries, each naming its limit, and the batch entry's shapes
#include "host_arima_paths_plan.hpp" // the host-only checks of the ARIMA model-path entries (options, period, the ring limit), each naming its limit
#include "host_ets_paths_plan.hpp" // the host-only checks of the model-path entries (options, period and ring, pool), each naming its limit
#include "host_path_scores_plan.hpp" // the host-only checks of the path-score entries, the energy workspace and a plan's column ranges
#include "host_scaled_scores_plan.hpp" // the host-only checks of the scaled-score entries and the ranges of the WRMSSE chain
#include "host_period_search.hpp" // the host-only logic of the SSA / STL period entries (defaults, window, candidate list, checks naming their limits)
#include "host_matrix_profile.hpp" // the host-only logic of the matrix-profile period entries (m and exclusion rule, homes, workspace, tile walk, checks)
#include "host_fit_schedule.hpp"  // the schedule of an ETS / AutoETS fit, decided from plain values (plan_fit_schedule): launch_fit_slots walks it

struct Plan {
    ModelType model;
    std::string ets_notation;   // explicit ETS spec ("" = none)
    int ets_spec_id = -1;
    int pool = 0;
    std::string static_name;    // model_name when model_code == 0
    double z = 1.645;
};

thread_local unsigned tl_host_thread_share = 1;   // > 1 while this thread runs one of several device shards of a batch call (the packer takes its share of the host threads)
std::atomic<int> g_default_arima_method{0};      // ANOFOX_ARIMA_CSS (anofox_hip_set_default_arima_method)
// The estimation method a CALL runs under is fixed when the call enters the library and handed to every host thread that works for
// it (shard, part and merged-batch workers; the leader of a coalesced group runs under the method its members were matched on) --
// a concurrent anofox_hip_set_default_arima_method never changes a call half way.  -1: no call in force, the process default.
std::atomic<int> g_arima_runs{0};       // AutoARIMA searches in flight (launch_arima shortens its launches when it shares the device)
thread_local int tl_arima_method = -1;
static int arima_method_in_force() { return tl_arima_method >= 0 ? tl_arima_method : g_default_arima_method.load(); }
struct ArimaMethodScope {
    int saved;
    explicit ArimaMethodScope(int m) : saved(tl_arima_method) { tl_arima_method = m; }
    ~ArimaMethodScope() { tl_arima_method = saved; }
};

} // namespace

struct AnofoxHipBatch {
    int dev = 0;                       // the device the batch lives on (the caller's current device when it was created): every
                                       // entry point makes it current for its own duration, so a host thread may drive batches of
                                       // several devices
    size_t n = 0, t_max = 0, ld = 0;
    int h = 0;
    ForecastOptions opt;
    Plan plan;
    bool has_block = false, owns_y = false;
    double *d_y = nullptr;
    int32_t *d_len = nullptr;          // lengths with unusable series zeroed
    bool owns_len = false;
    std::vector<int32_t> h_len;        // true lengths
    bool quiesced = true;              // nothing of this batch is in flight (set by the fetch's wait, cleared by a run): destroy need not wait
    std::vector<int32_t> h_period;     // per-series period
    std::vector<int32_t> h_base_status;
    std::vector<int32_t> h_slot_spec;
    double *h_stage = nullptr;         // pinned staging copy of the time-major block (packer output, H2D source)
    size_t h_stage_elems = 0;
    std::vector<double> h_clean;       // interpolated host copy (only when fitted values requested)
    std::vector<size_t> h_clean_off;
    // prep outputs
    double *d_mean = nullptr, *d_sd = nullptr, *d_fig_add = nullptr, *d_fig_mul = nullptr, *d_l0 = nullptr, *d_b0 = nullptr;
    uint32_t *d_flags = nullptr;
    int fig_m = 0;
    // spec slots
    int n_slots_cap = 0;
    double *d_aicc = nullptr, *d_yhat_slots = nullptr;
    int32_t *d_status_slots = nullptr, *d_evals_slots = nullptr, *d_iters_slots = nullptr, *d_passes_slots = nullptr, *d_slot_spec = nullptr;
    // compact copies of the series block for the ETS round / final kernels (round 6, ets_device.hpp YT_*): a float block and a uint16_t
    // block of t_max x ld cells each, remade by every run that fits (the caller may have rewritten a resident block), and the count of
    // observations that do not survive either round trip.  y_type: what THIS run's fit streams (YT_F64 unless a counter is zero).
    float *d_yc32 = nullptr;
    unsigned short *d_yc16 = nullptr;
    size_t yc_cells = 0;
    unsigned int *d_misfit = nullptr;
    unsigned int h_misfit[2] = {1u, 1u};
    int y_type = 0;
    unsigned long long *d_wave_trace = nullptr;    // developer instrument (tune wave_trace): 4 + 4 x WAVE_TRACE_RECORDS words, see FitArgs::wave_trace
    unsigned long long *d_lane_stats = nullptr;    // [n_slots_cap x 2] wave passes / live lane passes of every spec's round kernels (zeroed per run)
    // outputs
    double *d_yhat = nullptr, *d_lo = nullptr, *d_hi = nullptr;
    int32_t *d_model_code = nullptr, *d_status = nullptr, *d_detail = nullptr, *d_passes_total = nullptr, *d_evals_total = nullptr;
    uint32_t *d_mask = nullptr;
    int32_t *d_len_group = nullptr;
    int32_t *d_count = nullptr;
    // strictly positive series of the current group, dense: round 0 of the specs with a multiplicative component runs on it
    int32_t *d_pos_map = nullptr, *d_pos_cnt = nullptr, *d_notpos = nullptr;
    double *d_ypos = nullptr;
    bool use_pos = false;
    bool none_pos = false;             // the group has no strictly positive series: multiplicative specs are retired without a launch chain
    // what the inspection pass needs from the last fit: the final-kernel arguments of every spec, in launch order
    std::vector<anofox::FitArgs> insp_args;
    std::vector<anofox::FitLaunchers> insp_fns;
    std::vector<int> insp_spec, insp_stream;
    bool insp_ok = false;
    int insp_m = 1;
    int32_t live_pos = -1, live_all = -1;   // usable strictly positive / usable series of the current group (-1: not counted)
    // AutoARIMA workspace
    int arima_method = 0;            // ANOFOX_ARIMA_CSS: the search's own estimates; ANOFOX_ARIMA_CSS_ML: exact-likelihood refit of the
                                     // selected model (anofox_hip_batch_set_arima_method / anofox_hip_set_default_arima_method)
    size_t ar_ws_bytes = 0;
    double *ar_w = nullptr, *ar_wmean = nullptr, *ar_wsd = nullptr, *ar_l0 = nullptr, *ar_l1 = nullptr, *ar_x = nullptr, *ar_aicc = nullptr;
    int32_t *ar_wlen = nullptr, *ar_d = nullptr, *ar_D = nullptr, *ar_order = nullptr, *ar_status = nullptr, *ar_evals = nullptr, *ar_passes = nullptr, *ar_models = nullptr;
    // streams / events (borrowed from the process-wide pool: `sset`)
    StreamSet *sset = nullptr;
    hipStream_t own_stream = nullptr;
    hipStream_t aux[N_AUX_STREAMS] = {};
    hipEvent_t ev_start = nullptr, ev_stop = nullptr, ev_fit0 = nullptr, ev_fit1 = nullptr, ev_fork = nullptr;
    hipEvent_t ev_join[N_AUX_STREAMS] = {};
    // per aux stream: gathered block of the running problems, ping-pong column maps + counts, parked NM state
    struct Lane {
        double *ybuf = nullptr;          // allocated when a run first needs it (launch_fit_slots: only the specs that have anything to fit)
        size_t ybuf_cols = 0;            // columns it holds (<= ld)
        int32_t *map[2] = {nullptr, nullptr};
        int32_t *cnt = nullptr;          // [2]
        anofox::NmStateBuf st{};
        double *nm_scratch = nullptr;    // where the lanes' simplices rest between passes (kernels that keep them out of LDS: RoundTraits::PARK)
        size_t nm_scratch_doubles = 0;
    } lanes[N_AUX_STREAMS];
    // group rounds (launch_fit_slots): the [round][slot] arguments of a run's group launches, uploaded once per run from the pinned copy
    anofox::FitArgs *d_group_tab = nullptr, *h_group_tab = nullptr;
    size_t group_tab_cap = 0;
    hipEvent_t ev_group_tab = nullptr;     // recorded behind the upload: the pinned copy is rewritten only once it has been read
    hipStream_t last_stream = nullptr;
    bool ran = false, timed_fit = false;
    uint32_t fit_launches = 0;
    uint64_t n_problems = 0;
    Tunables tun;            // the environment knobs, read when the batch was created
    int seq_rounds = 3;      // rounds run by the sequential Nelder-Mead driver before switching to the speculative one
    int seq_rounds_env = -1; // tune seq_rounds override (-1 = decide from the number of live problems)
    int spec_below_md = 8192; // same, for the damped multiplicative-trend specs (their pass is ~10x longer: the stragglers matter more)
    // the SES / Holt / Holt-Winters / SeasonalES family on the round kernels: its own Nelder-Mead state, status and compaction lists
    // (the spec lanes keep the optima an inspection call re-reads)
    anofox::NmStateBuf classic_st{};
    int32_t *d_classic_status = nullptr, *classic_map[2] = {nullptr, nullptr}, *classic_cnt = nullptr;
    double *d_classic_ybuf = nullptr;
    size_t classic_ybuf_cols = 0;
    std::vector<void *> retired;  // blocks a run outgrew while kernels may still read them: handed back when the batch is destroyed
                                  // (freeing them on the spot needs a device-wide synchronisation, which couples every host thread's batch)
    int32_t *d_m_col = nullptr;   // merged batch of several seasonal periods (auto-detected): period of every column, constant within 64 columns
    int merged_m_max = 0;         // ... and its largest period (sizes)
    int spec2_below_md = 2048; // per spec: the last problems run one per wave, two iterations per pass (0 = never); damped multiplicative
                               // trend.  Measured on the 30-spec M5 batch (tools/spec2_sweep.sh): 0 / 256 / 1024 / 2048 / 4096 / 8192 -> 579 / 575 / 565 / 562 / 594 / 736 ms
    int spec2_below = 1024;    // same, other specs (single-spec ETS(A,A,A) fit: 22.5 -> 18.2 ms; all specs at 2048 / 4096: 588 / 673 ms)
    int spec_below = 8192;   // per spec: switch to the speculative driver once this few problems are still running
    bool use_gather = false; // rebuild a dense block of the running problems between rounds (else index y by series)
    double gather_budget = 0.0;  // bytes the gather blocks of one run may take together (55 % of the device): a block holds ld columns, or
                                 // fewer when the live specs' blocks would not fit (the gather then starts once that few problems still
                                 // run; until then the rounds index y by series)
    bool sd_in_final = false;        // this run's one-spec ETS batch: the final pass computes d_sd (prep_kernel ran one sweep)
    double *d_ring = nullptr;        // seasonal rings of periods above the LDS limit: one area per (candidate spec, workgroup)
    size_t ring_elems = 0;
    double *d_prep_scratch = nullptr;   // prep kernel's window ring + per-phase accumulators for such periods
    size_t prep_scratch_elems = 0;
    // BASELINE config 2: ETS(spec) with GIVEN smoothing parameters -- no optimiser, one streamed pass per series
    bool fixed_params = false;
    double fixed_x[4] = {0.0, 0.0, 0.0, 0.0};   // optimiser coordinates (alpha, beta*, gamma*, phi) of the given parameters
    // intermittent-demand models (fit_intermittent.hip): aggregation level of every series, largest level per group of 64 series
    // (+ the batch's), and IMAPA's per-(level, series) terms, grown on demand to the largest level a run meets
    int32_t *d_im_level = nullptr, *d_im_gmax = nullptr;
    double *d_im_fc = nullptr;
    size_t im_fc_elems = 0;
    // dynamic Theta models (fit_theta.hip): seasonal indices [m x ld], grown on demand to the largest period a run meets, and the
    // per-series "seasonally adjusted" flag
    double *d_th_sidx = nullptr;
    size_t th_sidx_elems = 0;
    int32_t *d_th_adj = nullptr;
    // exogenous regressors (fit_exog.hip): the historical block [k x t_max x ld] and the future block [k x h x ld], adopted from the
    // caller (anofox_hip_batch_set_exog_device) or owned (the host batch entry), and the per-series intercept, coefficients and used mask
    int exog_k = 0;
    const double *d_exog_x = nullptr, *d_exog_f = nullptr;
    bool owns_exog = false;
    double *d_exog_b0 = nullptr, *d_exog_beta = nullptr;
    uint32_t *d_exog_used = nullptr;
};

namespace {

// ---------------------------------------------------------------------------------------------
// option validation shared by every entry point (forecast.rs:512-565, 1278-1314, 1524-1556)
// ---------------------------------------------------------------------------------------------
bool make_plan(const ForecastOptions *o, Plan &p, AnofoxError *err)
{
    std::string mname = cstr_field(o->model, sizeof o->model);
    if (!parse_model(mname, p.model)) {
        set_error(err, INVALID_MODEL, "Invalid model: Unknown model: '" + mname + "'");
        return false;
    }
    if (o->horizon < 0) { set_error(err, PANIC_CAUGHT, "Panic in Rust code"); return false; }
    if (!o->auto_detect_seasonality && o->seasonal_period > 1 && is_non_seasonal_model(p.model)) {
        char buf[512];
        std::snprintf(buf, sizeof buf,
                      "Invalid input: Model '%s' does not use seasonal_period (got %d). For seasonal forecasting, use: "
                      "SeasonalNaive, HoltWinters, SeasonalES, AutoETS, AutoMFLES, AutoMSTL, or AutoTBATS.",
                      model_name(p.model), o->seasonal_period);
        set_error(err, INVALID_INPUT, buf);
        return false;
    }
    p.static_name = model_name(p.model);
    p.z = z_for_confidence(o->confidence_level);
    switch (p.model) {
    case M_Naive: case M_SeasonalNaive: case M_SMA: case M_RandomWalkDrift: case M_ARIMA:
    case M_SES: case M_SESOptimized: case M_Holt: case M_HoltWinters: case M_SeasonalES: case M_SeasonalESOptimized:
    case M_SeasonalWindowAverage:
    case M_CrostonClassic: case M_CrostonSBA: case M_TSB: case M_ADIDA: case M_IMAPA:
    case M_DynamicTheta: case M_DynamicOptimizedTheta:
        break;
    case M_ETS: {
        p.ets_notation = cstr_field(o->ets_model, sizeof o->ets_model);
        if (!p.ets_notation.empty()) {
            const std::string &nt = p.ets_notation;
            if (!valid_ets_notation(nt)) {
                set_error(err, INVALID_INPUT,
                          "Invalid input: Invalid ETS model specification '" + nt +
                              "'. Expected 3 or 4 character notation: Error(A/M) + Trend(A/M/N) + Seasonal(A/M/N), with optional 'd' "
                              "for damped trend. Examples: 'AAA' (additive), 'MNM' (multiplicative error, no trend), 'AAdA' (additive "
                              "damped trend). Valid characters: A=Additive, M=Multiplicative, N=None, d=Damped.");
                return false;
            }
            p.ets_spec_id = spec_id_from_notation(nt);
            if (!spec_is_valid(p.ets_spec_id)) {
                set_error(err, INVALID_INPUT,
                          "Invalid input: ETS model '" + nt +
                              "' is an unstable combination (multiplicative error with additive components). Try one of: 'AAA', 'ANA', "
                              "'AAdA', 'MNM', 'MAM', 'MAdM', 'MMM', 'MMdM', or use 'AutoETS' for automatic selection.");
                return false;
            }
            p.static_name = "ETS(" + nt + ")";
        }
        break;
    }
    case M_AutoARIMA:
        break;
    case M_AutoETS: {
        std::string pool = cstr_field(o->model_pool, sizeof o->model_pool);
        p.pool = 0;
        if (!pool.empty()) {
            p.pool = parse_model_pool(pool);
            if (p.pool < 0) {
                set_error(err, INVALID_INPUT,
                          "Invalid input: Unknown model_pool '" + pool +
                              "'. Valid options: complete, no_multiplicative_trend, damped_trend_only, match_error_seasonal, reduced");
                return false;
            }
        }
        break;
    }
    default:
        set_error(err, INTERNAL_ERROR,
                  std::string("Internal error: model '") + model_name(p.model) + "' is not implemented by the HIP backend");
        return false;
    }
    return true;
}

// imputation.rs:61-114
void fill_nulls_interpolate(const double *values, const uint64_t *validity, size_t n, double *out)
{
    auto valid = [&](size_t i) { return validity == nullptr || ((validity[i / 64] >> (i % 64)) & 1ull); };
    long first = -1, last = -1;
    for (size_t i = 0; i < n; i++)
        if (valid(i)) { if (first < 0) first = (long)i; last = (long)i; }
    for (size_t i = 0; i < n; i++) out[i] = std::nan("");
    if (first < 0) return;
    for (long i = 0; i < first; i++) out[i] = values[first];
    for (size_t i = (size_t)last + 1; i < n; i++) out[i] = values[last];
    long prev = first;
    double pv = values[first];
    out[first] = pv;
    for (long i = first + 1; i <= last; i++) {
        if (valid((size_t)i)) {
            double v = values[i];
            long gap = i - prev;
            if (gap > 1) {
                double slope = (v - pv) / (double)gap;
                for (long j = 1; j < gap; j++) out[prev + j] = pv + slope * (double)j;
            }
            out[i] = v;
            prev = i;
            pv = v;
        }
    }
}

// a batch borrows its streams and events from the process-wide pool (and hands them back while it is parked, see pool_give)
void batch_attach_streams(AnofoxHipBatch *b)
{
    if (b->sset) return;
    b->sset = stream_set_take();
    b->own_stream = b->sset->own;
    for (int i = 0; i < N_AUX_STREAMS; i++) { b->aux[i] = b->sset->aux[i]; b->ev_join[i] = b->sset->ev_join[i]; }
    b->ev_start = b->sset->ev_start; b->ev_stop = b->sset->ev_stop; b->ev_fit0 = b->sset->ev_fit0; b->ev_fit1 = b->sset->ev_fit1;
    b->ev_fork = b->sset->ev_fork;
}
void batch_detach_streams(AnofoxHipBatch *b)           // the caller has synchronised the set's streams (or nothing was ever launched on them)
{
    if (!b->sset) return;
    stream_set_give(b->sset);
    b->sset = nullptr; b->own_stream = nullptr; b->last_stream = nullptr; b->ran = false;
    for (auto &q : b->aux) q = nullptr;
}

void free_batch_buffers(AnofoxHipBatch *b)
{
    auto F = [](void *p) { dev_free(p, true); };             // the caller has synchronised the batch's streams
    if (b->owns_y) F(b->d_y);
    pin_free(b->h_stage);
    if (b->owns_len) F(b->d_len);
    F(b->d_mean); F(b->d_sd); F(b->d_fig_add); F(b->d_fig_mul); F(b->d_l0); F(b->d_b0); F(b->d_flags);
    F(b->d_aicc); F(b->d_yhat_slots); F(b->d_status_slots); F(b->d_evals_slots); F(b->d_iters_slots);
    F(b->d_passes_slots); F(b->d_slot_spec); F(b->d_lane_stats); F(b->d_wave_trace); F(b->d_yc32); F(b->d_yc16); F(b->d_misfit);
    F(b->d_yhat); F(b->d_lo); F(b->d_hi); F(b->d_model_code); F(b->d_status); F(b->d_detail);
    F(b->classic_st.sim); F(b->classic_st.fs); F(b->classic_st.phase); F(b->classic_st.evals); F(b->classic_st.iters); F(b->classic_st.passes); F(b->classic_st.done);
    F(b->d_classic_ybuf); F(b->d_classic_status); F(b->classic_map[0]); F(b->classic_map[1]); F(b->classic_cnt);
    for (void *p : b->retired) F(p);
    b->retired.clear();
    F(b->d_m_col); F(b->d_ring); F(b->d_prep_scratch);
    F(b->d_group_tab); pin_free(b->h_group_tab); b->d_group_tab = b->h_group_tab = nullptr; b->group_tab_cap = 0;
    if (b->ev_group_tab) { (void)hipEventDestroy(b->ev_group_tab); b->ev_group_tab = nullptr; }
    F(b->d_im_level); F(b->d_im_gmax); F(b->d_im_fc);
    F(b->d_th_sidx); F(b->d_th_adj);
    if (b->owns_exog) { F((void *)b->d_exog_x); F((void *)b->d_exog_f); }
    b->d_exog_x = b->d_exog_f = nullptr; b->owns_exog = false; b->exog_k = 0;
    F(b->d_exog_b0); F(b->d_exog_beta); F(b->d_exog_used);
    F(b->d_passes_total); F(b->d_evals_total); F(b->d_mask); F(b->d_len_group); F(b->d_count); F(b->d_pos_map); F(b->d_pos_cnt); F(b->d_notpos); F(b->d_ypos);
    F(b->ar_w); F(b->ar_wmean); F(b->ar_wsd); F(b->ar_l0); F(b->ar_l1); F(b->ar_x); F(b->ar_aicc); F(b->ar_wlen); F(b->ar_d); F(b->ar_D);
    F(b->ar_order); F(b->ar_status); F(b->ar_evals); F(b->ar_passes); F(b->ar_models);
    batch_detach_streams(b);
    for (auto &l : b->lanes) {
        F(l.ybuf); l.ybuf_cols = 0; F(l.map[0]); F(l.map[1]); F(l.cnt);
        F(l.st.sim); F(l.st.fs); F(l.st.phase); F(l.st.evals); F(l.st.iters); F(l.st.passes); F(l.st.done);
        F(l.nm_scratch); l.nm_scratch_doubles = 0;
    }
}

int max_slots_for(const Plan &p)
{
    if (p.model == M_AutoETS) return 30;
    if (p.model == M_ETS && p.ets_spec_id >= 0) return 1;
    return 0;
}

void alloc_common(AnofoxHipBatch *b)
{
    const size_t n = b->n, ld = b->ld, h = (size_t)std::max(b->h, 0);
    b->d_mean = dalloc<double>(ld);
    b->d_sd = dalloc<double>(ld);
    b->d_flags = dalloc<uint32_t>(ld);
    b->d_yhat = dalloc<double>(n * h);
    b->d_lo = dalloc<double>(n * h);
    b->d_hi = dalloc<double>(n * h);
    b->d_model_code = dalloc<int32_t>(ld);
    b->d_status = dalloc<int32_t>(ld);
    b->d_detail = dalloc<int32_t>(ld);
    b->d_passes_total = dalloc<int32_t>(ld);
    b->d_evals_total = dalloc<int32_t>(ld);
    b->d_mask = dalloc<uint32_t>(ld);
    b->d_len_group = dalloc<int32_t>(ld);
    b->d_count = dalloc<int32_t>(2);
    if (b->plan.model == M_AutoETS) {
        b->d_pos_map = dalloc<int32_t>(ld); b->d_pos_cnt = dalloc<int32_t>(2); b->d_notpos = dalloc<int32_t>(ld);
    }
    if (is_intermittent_model(b->plan.model)) {
        b->d_im_level = dalloc<int32_t>(ld);
        b->d_im_gmax = dalloc<int32_t>((size_t)intermittent_groups((int)n) + 1);
    }
    if (is_theta_model(b->plan.model)) b->d_th_adj = dalloc<int32_t>(ld);
    if (b->plan.model == M_AutoARIMA) {
        const size_t T = std::max<size_t>(b->t_max, 1);
        b->ar_ws_bytes = arima_workspace_bytes((int)b->n, (int)T);
        b->ar_w = (double *)dalloc<char>(b->ar_ws_bytes);     // search workspace: differenced rows, candidate cache, queues
        HIPCHECK(hipMemset(b->ar_w, 0, b->ar_ws_bytes));
        b->ar_wmean = dalloc<double>(ld); b->ar_wsd = dalloc<double>(ld); b->ar_l0 = dalloc<double>(ld); b->ar_l1 = dalloc<double>(ld);
        b->ar_x = dalloc<double>(6 * ld); b->ar_aicc = dalloc<double>(ld);
        b->ar_wlen = dalloc<int32_t>(ld); b->ar_d = dalloc<int32_t>(ld); b->ar_D = dalloc<int32_t>(ld); b->ar_order = dalloc<int32_t>(5 * ld);
        b->ar_status = dalloc<int32_t>(ld); b->ar_evals = dalloc<int32_t>(ld); b->ar_passes = dalloc<int32_t>(ld); b->ar_models = dalloc<int32_t>(ld);
        HIPCHECK(hipMemset(b->ar_wlen, 0, ld * sizeof(int32_t)));
    }
    HIPCHECK(hipMemset(b->d_model_code, 0, ld * sizeof(int32_t)));
    HIPCHECK(hipMemset(b->d_detail, 0, ld * sizeof(int32_t)));
    HIPCHECK(hipMemset(b->d_passes_total, 0, ld * sizeof(int32_t)));
    HIPCHECK(hipMemset(b->d_evals_total, 0, ld * sizeof(int32_t)));
    HIPCHECK(hipMemset(b->d_mask, 0, ld * sizeof(uint32_t)));
    b->n_slots_cap = max_slots_for(b->plan);
    if (b->n_slots_cap > 0) {
        const size_t S = (size_t)b->n_slots_cap;
        b->d_l0 = dalloc<double>(9 * ld);
        b->d_b0 = dalloc<double>(9 * ld);
        b->d_aicc = dalloc<double>(S * ld);
        b->d_yhat_slots = dalloc<double>(S * n * h);
        b->d_status_slots = dalloc<int32_t>(S * ld);
        b->d_evals_slots = dalloc<int32_t>(S * ld);
        b->d_iters_slots = dalloc<int32_t>(S * ld);
        b->d_passes_slots = dalloc<int32_t>(S * ld);
        b->d_slot_spec = dalloc<int32_t>(S);
        b->d_lane_stats = dalloc<unsigned long long>(2 * S);
        HIPCHECK(hipMemset(b->d_lane_stats, 0, 2 * S * sizeof(unsigned long long)));
        const int n_lanes = std::min<int>(N_AUX_STREAMS, b->n_slots_cap);
        for (int q = 0; q < n_lanes; q++) {
            auto &l = b->lanes[q];
            l.map[0] = dalloc<int32_t>(ld);
            l.map[1] = dalloc<int32_t>(ld);
            l.cnt = dalloc<int32_t>(3);
            l.st.sim = dalloc<double>(20 * ld);
            l.st.fs = dalloc<double>(5 * ld);
            l.st.phase = dalloc<int32_t>(ld);
            l.st.evals = dalloc<int32_t>(ld);
            l.st.iters = dalloc<int32_t>(ld);
            l.st.passes = dalloc<int32_t>(ld);
            l.st.done = dalloc<int32_t>(ld);
        }
    }
    batch_attach_streams(b);
}

void ensure_fig(AnofoxHipBatch *b, int m)
{
    if (m <= b->fig_m) return;
    if (b->d_fig_add) b->retired.push_back(b->d_fig_add);
    if (b->d_fig_mul) b->retired.push_back(b->d_fig_mul);
    b->d_fig_add = nullptr; b->d_fig_mul = nullptr; b->fig_m = 0;      // (an allocation below may throw: the retired blocks must not be freed twice)
    b->d_fig_add = dalloc<double>((size_t)m * b->ld);
    b->d_fig_mul = dalloc<double>((size_t)m * b->ld);
    b->fig_m = m;
}

// HBM scratch for seasonal periods whose rings do not fit LDS (ETS_LDS_PERIOD): grown on demand, kept for the batch
double *ensure_ring(AnofoxHipBatch *b, size_t elems)
{
    if (b->ring_elems < elems) {
        if (b->d_ring) b->retired.push_back(b->d_ring);
        b->d_ring = nullptr; b->ring_elems = 0;
        b->d_ring = dalloc<double>(elems);
        b->ring_elems = elems;
    }
    return b->d_ring;
}
double *ensure_prep_scratch(AnofoxHipBatch *b, size_t elems)
{
    if (b->prep_scratch_elems < elems) {
        if (b->d_prep_scratch) b->retired.push_back(b->d_prep_scratch);
        b->d_prep_scratch = nullptr; b->prep_scratch_elems = 0;
        b->d_prep_scratch = dalloc<double>(elems);
        b->prep_scratch_elems = elems;
    }
    return b->d_prep_scratch;
}

// Seasonal periods of the columns of a resident time-major block (kernels.hip detect_period_kernel): 0 = no autocorrelation peak.
void detect_periods_block(const double *d_y, size_t ld, const int32_t *d_len, size_t n, size_t t_rows, int32_t *h_out, hipStream_t st)
{
    if (n == 0) return;
    int32_t *d_per = dalloc<int32_t>(n);
    const size_t sc = detect_scratch_doubles((int)n, (int)t_rows);
    double *d_sc = sc ? dalloc<double>(sc) : nullptr;
    try {
        launch_detect_periods(d_y, ld, d_len, (int)n, (int)t_rows, d_sc, d_per, nullptr, st);
        LAUNCHCHECK("seasonal period detection");
        HIPCHECK(hipMemcpyAsync(h_out, d_per, n * sizeof(int32_t), hipMemcpyDeviceToHost, st));
        HIPCHECK(hipStreamSynchronize(st));
    } catch (...) { dev_free(d_per); dev_free(d_sc); throw; }
    dev_free(d_per, true);
    dev_free(d_sc, true);
}

// ... of host series (the batch entry with params := MAP{}, before the batch is split by period): packed 64 series per tile into
// pinned blocks of ~128 MB, two in flight, so that the packer threads work on one block while the other is copied and scanned
std::vector<int> detect_periods_host_series(const double *const *values, const uint64_t *const *validity, const size_t *lengths, size_t n_series)
{
    std::vector<int> out(n_series, 0);
    size_t t_all = 0;
    for (size_t s = 0; s < n_series; s++) t_all = std::max(t_all, lengths[s]);
    if (t_all < 4 || n_series == 0) return out;
    const size_t n_pad = (n_series + 63) / 64 * 64;
    const size_t cols = std::min(n_pad, std::max<size_t>(64, (size_t)(134217728.0 / (8.0 * (double)t_all)) / 64 * 64));
    struct Buf { double *h = nullptr, *d = nullptr, *sc = nullptr; int32_t *h_len = nullptr, *d_len = nullptr, *h_per = nullptr, *d_per = nullptr;
                 size_t s0 = 0, cnt = 0; bool busy = false; hipEvent_t done = nullptr; } buf[2];
    hipStream_t st = nullptr;
    auto release = [&]() {
        if (st) { (void)hipStreamSynchronize(st); (void)hipStreamDestroy(st); }
        for (auto &b : buf) {
            pin_free(b.h); pin_free(b.h_len); dev_free(b.d, true); dev_free(b.sc, true); dev_free(b.d_len, true); dev_free(b.d_per, true);
            if (b.done) (void)hipEventDestroy(b.done);
        }
    };
    try {
        HIPCHECK(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
        const size_t n_chunks = (n_series + cols - 1) / cols;
        for (int k = 0; k < (n_chunks > 1 ? 2 : 1); k++) {
            HIPCHECK(hipEventCreateWithFlags(&buf[k].done, hipEventDisableTiming));
            buf[k].h = (double *)pin_alloc_bytes(t_all * cols * sizeof(double));
            buf[k].h_len = (int32_t *)pin_alloc_bytes(2 * cols * sizeof(int32_t));
            buf[k].h_per = buf[k].h_len + cols;
            buf[k].d = dalloc<double>(t_all * cols);
            buf[k].d_len = dalloc<int32_t>(cols);
            buf[k].d_per = dalloc<int32_t>(cols);
            const size_t sc = detect_scratch_doubles((int)cols, (int)t_all);
            if (sc) buf[k].sc = dalloc<double>(sc);
        }
        auto collect = [&](Buf &b) {
            if (!b.busy) return;
            HIPCHECK(hipEventSynchronize(b.done));                // this block's copy back (the other block may still be in flight)
            for (size_t j = 0; j < b.cnt; j++) out[b.s0 + j] = b.h_per[j];
            b.busy = false;
        };
        unsigned n_thr = std::max(1u, std::min(std::thread::hardware_concurrency(), 32u));
        if (tl_host_thread_share > 1) n_thr = std::max(1u, n_thr / tl_host_thread_share);
        for (size_t ck = 0; ck < n_chunks; ck++) {
            Buf &b = buf[ck & 1];
            collect(b);
            b.s0 = ck * cols;
            b.cnt = std::min(cols, n_series - b.s0);
            size_t T = 0;
            for (size_t j = 0; j < b.cnt; j++) T = std::max(T, lengths[b.s0 + j]);
            T = std::max<size_t>(T, 1);
            const size_t ld = (b.cnt + 63) / 64 * 64, n_tiles = ld / 64;
            auto do_tiles = [&](size_t tile0, size_t tile1) {
                std::vector<double> clean(64 * T);
                for (size_t tile = tile0; tile < tile1; tile++) {
                    size_t len_of[64];
                    for (size_t j = 0; j < 64; j++) {
                        const size_t c = tile * 64 + j;
                        const size_t len = c < b.cnt ? lengths[b.s0 + c] : 0;
                        len_of[j] = len;
                        if (len) fill_nulls_interpolate(values[b.s0 + c], validity ? validity[b.s0 + c] : nullptr, len, clean.data() + j * T);
                        b.h_len[c] = len >= 3 ? (int32_t)len : 0;
                    }
                    for (size_t t = 0; t < T; t++) {
                        double *row = b.h + t * ld + tile * 64;
                        for (size_t j = 0; j < 64; j++) row[j] = t < len_of[j] ? clean[j * T + t] : 0.0;
                    }
                }
            };
            const unsigned thr = (unsigned)std::min<size_t>(n_thr, n_tiles);
            if (thr <= 1) do_tiles(0, n_tiles);
            else {
                std::atomic<bool> failed{false};
                parallel_shares(thr, [&](unsigned k) { try { do_tiles(n_tiles * k / thr, n_tiles * (k + 1) / thr); } catch (...) { failed = true; } });
                if (failed) throw HipFail{"period detection: packer thread failed (out of host memory)", true};
            }
            HIPCHECK(hipMemcpyAsync(b.d, b.h, T * ld * sizeof(double), hipMemcpyHostToDevice, st));
            HIPCHECK(hipMemcpyAsync(b.d_len, b.h_len, ld * sizeof(int32_t), hipMemcpyHostToDevice, st));
            launch_detect_periods(b.d, ld, b.d_len, (int)b.cnt, (int)T, b.sc, b.d_per, nullptr, st);
            LAUNCHCHECK("seasonal period detection");
            HIPCHECK(hipMemcpyAsync(b.h_per, b.d_per, b.cnt * sizeof(int32_t), hipMemcpyDeviceToHost, st));
            HIPCHECK(hipEventRecord(b.done, st));
            b.busy = true;
        }
        collect(buf[0]);
        collect(buf[1]);
    } catch (...) { release(); throw; }
    release();
    return out;
}

// Series that cannot be forecast at all (forecast.rs:516-525) and per-series periods.
void finalize_lengths(AnofoxHipBatch *b)
{
    const size_t n = b->n;
    b->h_base_status.assign(n, 0);
    std::vector<int32_t> eff(b->ld, 0);
    for (size_t s = 0; s < n; s++) {
        if (b->h_len[s] < 3) b->h_base_status[s] = INSUFFICIENT_DATA;
        else eff[s] = b->h_len[s];
    }
    if (!b->d_len) { b->d_len = dalloc<int32_t>(b->ld); b->owns_len = true; }
    HIPCHECK(hipMemcpy(b->d_len, eff.data(), b->ld * sizeof(int32_t), hipMemcpyHostToDevice));
}

// auto-detected periods of a batch's own block (after finalize_lengths: series shorter than three observations read as empty)
void batch_detect_periods(AnofoxHipBatch *b)
{
    std::vector<int32_t> per(b->n, 0);
    batch_attach_streams(b);
    detect_periods_block(b->d_y, b->ld, b->d_len, b->n, std::max<size_t>(b->t_max, 1), per.data(), b->own_stream);
    b->h_period.assign(b->n, 1);
    for (size_t s = 0; s < b->n; s++) b->h_period[s] = per[s] > 0 ? per[s] : 1;
}

// ---------------------------------------------------------------------------------------------
// the pipeline for one group of series sharing a seasonal period
// ---------------------------------------------------------------------------------------------
void run_classic(AnofoxHipBatch *b, int kind, const int32_t *d_len, int m, int optimized, double alpha, int min_len,
                 const uint32_t *mask, uint32_t want, int32_t code, bool write_code, hipStream_t st)
{
    ClassicArgs a{};
    a.y = b->d_y; a.ld = b->ld; a.len = d_len; a.n_series = (int)b->n;
    a.m = m; a.h = b->h; a.optimized = optimized; a.fixed_alpha = alpha;
    a.mask = mask; a.want = want; a.min_len = min_len;
    a.yhat = b->d_yhat; a.status = b->d_detail; a.passes = b->d_passes_total;
    a.model_code = code; a.model_code_out = write_code ? b->d_model_code : nullptr;
    a.ring_scratch = nullptr;
    a.m_col = (kind == CK_HW || kind == CK_SEASONAL_ES) ? b->d_m_col : nullptr;
    const bool optimise = kind == CK_HOLT || kind == CK_HW || optimized != 0;
    if (optimise) {
        // The optimised members of the family run on the ETS round kernels (ClassicCfg<KIND>, fit_classic.hip): resumable rounds
        // with compaction, the drivers picked from the device-side count, then one final pass.  One chain on `st`.
        const size_t n = b->n, ld = b->ld;
        if (!b->classic_st.sim) {
            b->classic_st.sim = dalloc<double>(12 * ld); b->classic_st.fs = dalloc<double>(4 * ld);
            b->classic_st.phase = dalloc<int32_t>(ld); b->classic_st.evals = dalloc<int32_t>(ld); b->classic_st.iters = dalloc<int32_t>(ld);
            b->classic_st.passes = dalloc<int32_t>(ld); b->classic_st.done = dalloc<int32_t>(ld);
            b->d_classic_status = dalloc<int32_t>(ld);
            b->classic_map[0] = dalloc<int32_t>(ld); b->classic_map[1] = dalloc<int32_t>(ld); b->classic_cnt = dalloc<int32_t>(3);
        }
        // dense re-gather between rounds: the spec lanes' block when there is one (free by now), else the family's own
        double *ybuf = (b->n_slots_cap > 0 && b->use_gather) ? b->lanes[0].ybuf : nullptr;
        size_t ybuf_cols = ybuf ? b->lanes[0].ybuf_cols : ld;
        if (!ybuf) {
            // the family's own block: up to 32 GiB of columns (the 1M x 1,024 block is 8.2 GB), fewer if the batch is larger still
            const double per_col = (double)std::max<size_t>(b->t_max, 1) * 8.0;
            const size_t cols = (size_t)std::min((double)ld, 32.0 * 1073741824.0 / per_col) / 64 * 64;
            if (cols >= 1024 || cols >= ld) {
                if (!b->d_classic_ybuf) { b->d_classic_ybuf = dalloc<double>(std::max<size_t>(b->t_max, 1) * cols); b->classic_ybuf_cols = cols; }
                ybuf = b->d_classic_ybuf;
                ybuf_cols = b->classic_ybuf_cols;
            }
        }
        const bool seasonal = kind == CK_HW || kind == CK_SEASONAL_ES;
        FitArgs f{};
        f.y = b->d_y; f.ld = ld; f.len = d_len; f.n_series = (int)n; f.t_rows = (int)std::max<size_t>(b->t_max, 1);
        f.m = seasonal ? std::max(m, 1) : 1; f.h = b->h;
        f.flags = b->d_flags; f.fig = nullptr; f.fig_ld = ld;
        f.status = b->d_classic_status; f.st = b->classic_st;
        f.mask = mask; f.want = want; f.min_len = min_len;
        f.m_col = a.m_col;
        const bool merged = f.m_col != nullptr;
        FitLaunchers fns = classic_fit_launcher(kind, (merged && f.m == 7) ? 8 : f.m);          // (7 has a register-ring variant: one period only)
        if (!fns.round_seq || !fns.round_spec || !fns.round_spec2 || !fns.round_auto) throw HipFail{"no round kernel for this model"};
        if (f.m > ETS_LDS_PERIOD) {
            const size_t wg = merged ? n : std::max<size_t>((n + 15) / 16, std::min<size_t>(n, 1024));
            f.ring_scratch = ensure_ring(b, wg * (size_t)f.m * 64u);
            f.ring_scratch_doubles = wg * (size_t)f.m * 64u;
        }
        static const int BUDGET[] = {24, 24, 24, 24, 48, 48, 96, 192, 1024};
        // a handful of series (one call per group from the scalar binding, the coalesced calls of a few workers): every problem
        // gets a WAVE from the start -- two iterations per pass -- and runs to completion in ONE launch instead of nine rounds of
        // compaction + gather + fit (one series through Holt-Winters: 8.6 ms of launches)
        const bool tiny = n <= TINY_BATCH_PROBLEMS;
        const int n_rounds = tiny ? 1 : (merged ? (n > 4096 ? 4 : 3) : (int)(sizeof BUDGET / sizeof BUDGET[0]));
        for (int r = 0; r < n_rounds; r++) {
            f.first_round = (r == 0);
            f.spec_below = -1; f.spec2_below = -1;
            f.gathered = 0;
            f.y_round = b->d_y; f.ld_round = ld; f.series_of = nullptr; f.n_active = nullptr;
            if (tiny) {
                f.budget = 1 << 30; f.budget_seq = f.budget;
                fns.round_spec2(f, st);
            } else if (merged) {
                // several periods in one block: every launch sweeps all columns in place (see launch_fit_slots)
                f.budget = r == 0 ? 64 : (r == 1 ? 128 : 256); f.budget_seq = f.budget;
                (r < n_rounds - 1 ? fns.round_spec : fns.round_spec2)(f, st);
            } else if (r == 0) {
                const bool seq0 = n >= 4u * 65536u;           // the chip is full with one lane per problem
                f.budget = seq0 ? (BUDGET[0] * 7) / 4 : BUDGET[0];
                (seq0 ? fns.round_seq : fns.round_spec)(f, st);
            } else {
                int32_t **map = b->classic_map, *cnt = b->classic_cnt;
                const int32_t *prev_map = (r == 1) ? nullptr : map[(r - 1) & 1];
                const int32_t *prev_cnt = (r == 1) ? nullptr : cnt + ((r - 1) % 3);
                if (r == 1) HIPCHECK(hipMemsetAsync(cnt, 0, 3 * sizeof(int32_t), st));
                launch_compact(prev_map, prev_cnt, (int)n, b->classic_st.done, map[r & 1], cnt + (r % 3), st, cnt + ((r + 1) % 3));
                f.series_of = map[r & 1]; f.n_active = cnt + (r % 3);
                if (ybuf) {
                    launch_gather_columns(b->d_y, ld, map[r & 1], cnt + (r % 3), (int)n, (int)b->t_max, ybuf, ybuf_cols, st, (int)ybuf_cols);
                    f.y_round = ybuf; f.ld_round = ybuf_cols; f.gathered = 1; f.gather_cap = (int)ybuf_cols;
                }
                f.spec_below = 8192; f.spec2_below = 1024;
                f.budget = BUDGET[r]; f.budget_seq = (BUDGET[r] * 7) / 4;
                fns.round_auto(f, st);
            }
            b->fit_launches++;
        }
        launch_classic_final(kind, f, a, st);
        return;
    }
    if ((kind == CK_HW || kind == CK_SEASONAL_ES) && m > 48)       // CLASSIC_LDS_PERIOD: four candidate rings per lane
        a.ring_scratch = ensure_ring(b, (size_t)((b->n + 63) / 64) * 4u * (size_t)m * 64u);
    launch_classic(kind, a, st);
}

// Start of a run, ONE launch (it was a status upload plus six fills: a fifth of the device time of the fixed-parameter step):
// usable series start as "not computed" and only a kernel turns that into success, the forecasts start as NaN (all bits set, as
// the 0xff fill wrote them), the per-series totals and the model codes as zero.
__global__ void seed_outputs_kernel(int n, int ld, size_t nh, const int32_t *len, int32_t *status, double *yhat, double *lo, double *hi,
                                    int32_t *passes_total, int32_t *evals_total, int32_t *model_code)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    const double nanv = __longlong_as_double(-1LL);
    if (i < nh) { yhat[i] = nanv; lo[i] = nanv; hi[i] = nanv; }
    if (i < (size_t)ld) { passes_total[i] = 0; evals_total[i] = 0; model_code[i] = 0; }
    if (i < (size_t)n) status[i] = len[i] > 0 ? (int32_t)STATUS_NOT_COMPUTED : (int32_t)INSUFFICIENT_DATA;      // (finalize_lengths: a series too short to forecast reads as empty)
}

__global__ void fill_i32_kernel(int n, int32_t *dst, int32_t v)
{
    int s = blockIdx.x * 256 + threadIdx.x;
    if (s < n) dst[s] = v;
}

// d_detail holds the per-series fit status of the last model stage; map it into ErrorCodes.
__global__ void finish_status_kernel(int n, const int32_t *len, const int32_t *detail, int32_t *status)
{
    int s = blockIdx.x * 256 + threadIdx.x;
    if (s >= n) return;
    if (len[s] <= 0) return;                 // not in this group / unusable: keep base status
    status[s] = detail[s] == FIT_OK ? 0 : COMPUTATION_ERROR;
}

__global__ void explicit_select_kernel(int n, int h, const int32_t *len, const int32_t *fit_status, const double *yhat_slot,
                                       const int32_t *passes, const int32_t *evals, double *yhat, int32_t *detail,
                                       int32_t *passes_total, int32_t *evals_total)
{
    // one thread per forecast value (a thread per series copied its h values 8 h bytes apart from its neighbour's: 14 us for the M5 batch)
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    const size_t hh = (size_t)(h > 0 ? h : 1);
    const size_t s = idx / hh;
    const int i = (int)(idx - s * hh);
    if (s >= (size_t)n || len[s] <= 0) return;
    const int32_t fs = fit_status[s];
    if (i == 0) {
        detail[s] = fs;
        passes_total[s] = passes[s];
        evals_total[s] = evals[s];
    }
    if (fs == FIT_OK && i < h) yhat[idx] = yhat_slot[idx];
}

// count[0] = usable strictly positive series, count[1] = usable series (one workgroup)
__global__ void count_positive_kernel(int n, const int32_t *len, const uint32_t *flags, int32_t *count)
{
    __shared__ int sp[1024], su[1024];
    int p = 0, u = 0;
    for (int s = threadIdx.x; s < n; s += 1024)
        if (len[s] > 0) { u++; if (flags[s] & SF_POSITIVE) p++; }
    sp[threadIdx.x] = p; su[threadIdx.x] = u;
    __syncthreads();
    for (int o = 512; o >= 1; o >>= 1) {
        if ((int)threadIdx.x < o) { sp[threadIdx.x] += sp[threadIdx.x + o]; su[threadIdx.x] += su[threadIdx.x + o]; }
        __syncthreads();
    }
    if (threadIdx.x == 0) { count[0] = sp[0]; count[1] = su[0]; }
}

// notpos[s] = 1 unless series s is usable and strictly positive
__global__ void mark_nonpositive_kernel(int n, const int32_t *len, const uint32_t *flags, int32_t *notpos)
{
    int s = blockIdx.x * 256 + threadIdx.x;
    if (s < n) notpos[s] = (len[s] > 0 && (flags[s] & SF_POSITIVE)) ? 0 : 1;
}

// per (spec with a multiplicative component): the series the dense first round never visits are retired here
__global__ void retire_nonpositive_kernel(int n, const int32_t *len, const int32_t *notpos, int32_t *status, int32_t *done, int32_t *passes,
                                          int32_t *evals, int32_t *iters, double *aicc = nullptr, int32_t *f_passes = nullptr,
                                          int32_t *f_evals = nullptr, int32_t *f_iters = nullptr)
{
    int s = blockIdx.x * 256 + threadIdx.x;
    if (s >= n || !notpos[s]) return;
    status[s] = len[s] > 0 ? FIT_NONPOSITIVE : FIT_SKIPPED;
    done[s] = 1; passes[s] = 0; evals[s] = 0; iters[s] = 0;
    // a spec without a launch chain: there is no final kernel to leave these behind
    if (aicc && len[s] > 0) { aicc[s] = __builtin_huge_val(); f_passes[s] = 0; f_evals[s] = 0; f_iters[s] = 0; }
}

// AutoETS fallback plan (forecast.rs:1327-1336): 1 Holt-Winters, 2 Holt, 3 SES(0.3)
__global__ void fallback_plan_kernel(int n, const int32_t *len, int period, uint32_t *mask, int32_t *detail, const int32_t *m_col)
{
    int s = blockIdx.x * 256 + threadIdx.x;
    if (s >= n) return;
    if (m_col) period = m_col[s];                  // merged batch: the column's own period
    const int L = len[s];
    if (L <= 0) { mask[s] = 0; return; }
    if (mask[s] == 0) { detail[s] = FIT_OK; return; }
    mask[s] = (period > 1 && L >= 2 * period) ? 1u : (L >= 10 ? 2u : 3u);
    detail[s] = FIT_PERIOD;      // until the planned stage fits the series (Holt-Winters with a period above ETS_MAX_PERIOD never runs)
}

// HoltWinters: 1 = two full seasons or more (seasonal fit), 2 = shorter (Holt); an unsupported period fails the long series
__global__ void holt_winters_plan_kernel(int n, const int32_t *len, int m, uint32_t *mask, int32_t *detail, const int32_t *m_col)
{
    int s = blockIdx.x * 256 + threadIdx.x;
    if (s >= n) return;
    if (m_col) m = m_col[s] > 2 ? m_col[s] : 2;    // merged batch: the column's own period
    const int L = len[s];
    mask[s] = L <= 0 ? 0u : (L >= 2 * m ? 1u : 2u);
    if (L > 0) detail[s] = FIT_PERIOD;        // overwritten by the stage that fits the series
}

// Fixed-parameter ETS (BASELINE config 2): what the first fit round would have decided about admissibility, and the given
// parameters parked where the final pass reads the optimum (vertex 0 of the simplex).  dim = number of coordinates.
__global__ void ets_fixed_setup_kernel(int n, size_t ld, const int32_t *len, const uint32_t *flags, int seasonal, int m, int n_param,
                                       int need_positive, int dim, double x0, double x1, double x2, double x3, int32_t *status,
                                       double *sim, int32_t *evals, int32_t *iters, int32_t *passes, int32_t *done)
{
    int s = blockIdx.x * 256 + threadIdx.x;
    if (s >= n) return;
    const int L = len[s];
    int st = FIT_OK;
    if (L <= 0) st = FIT_SKIPPED;
    else if (seasonal && L < 2 * m) st = FIT_SHORT;
    else if (L < n_param + 2) st = FIT_SHORT;
    else if (need_positive && !(flags[s] & SF_POSITIVE)) st = FIT_NONPOSITIVE;
    status[s] = st;
    const double x[4] = {x0, x1, x2, x3};
    for (int i = 0; i < dim; i++) sim[(size_t)i * ld + s] = x[i];
    evals[s] = 0; iters[s] = 0; passes[s] = 0; done[s] = 1;
}

// Compact storage of the series block (round 6; ets_device.hpp YT_*, kernels.hip compact_block_kernel).  The optimiser streams every
// series hundreds of times, so a batch of counts -- the M5 shape: integers, or anything else whose every observation survives the
// round trip through float or uint16_t bit for bit -- is streamed from a 4- or 2-byte copy of the block: half / a quarter of the bytes
// of a pass and of the registers the staged rows take (30,490 x 1,913, 25 specs: 450 -> 396 ms per step with the float copy, same
// passes, same bits).  begin: one sweep of the block makes both copies and counts the observations that do NOT survive (+ 0.15 ms for
// 467 MB); decide (after the host has synchronised the stream): a copy is used only when its counter is zero, so ONE inexact
// observation anywhere keeps the whole batch on the fp64 block.  Not for given parameters (one pass: the sweep would cost more than
// it saves) or a handful of series.
// tune compact: -1 auto (narrowest exact type; batches of at least 65,536 cells), 0 never, 1 float at most, 2 narrowest exact type (1 / 2: any size).
bool compact_storage_begin(AnofoxHipBatch *b, const int32_t *d_len, hipStream_t st)
{
    b->y_type = YT_F64;
    if (b->tun.compact == 0 || b->fixed_params) return false;
    if (b->tun.compact < 0 && b->n * (size_t)std::max<size_t>(b->t_max, 1) < (size_t)1 << 16) return false;      // (auto: not for a handful of short series)
    const size_t cells = b->ld * std::max<size_t>(b->t_max, 1);
    if (b->yc_cells < cells) {
        if (b->d_yc32) b->retired.push_back(b->d_yc32);
        if (b->d_yc16) b->retired.push_back(b->d_yc16);
        b->d_yc32 = nullptr; b->d_yc16 = nullptr; b->yc_cells = 0;
        try {
            b->d_yc32 = dalloc<float>(cells);
            b->d_yc16 = dalloc<unsigned short>(cells);
        } catch (const HipFail &f) {
            if (!f.oom) throw;
            if (b->d_yc32) { dev_free(b->d_yc32, true); b->d_yc32 = nullptr; }      // no room beside a co-resident allocator: the fp64 block serves
            return false;
        }
        b->yc_cells = cells;
    }
    if (!b->d_misfit) b->d_misfit = dalloc<unsigned int>(2);
    HIPCHECK(hipMemsetAsync(b->d_misfit, 0, 2 * sizeof(unsigned int), st));
    launch_compact_block(b->d_y, b->ld, d_len, (int)b->n, (int)std::max<size_t>(b->t_max, 1), b->d_yc32, b->d_yc16, b->d_misfit, st);
    b->h_misfit[0] = b->h_misfit[1] = 1u;
    HIPCHECK(hipMemcpyAsync(b->h_misfit, b->d_misfit, sizeof b->h_misfit, hipMemcpyDeviceToHost, st));
    return true;
}
// `m`: the batch's seasonal period (1: none).  The uint16_t kernels exist for the variants without a period and with the weekly ring
// in registers (fit_units.hpp ets_u16_variant); any other period -- and a merged batch of several -- streams the float copy.
void compact_storage_decide(AnofoxHipBatch *b, bool pending, hipStream_t st, int m)
{
    b->y_type = YT_F64;
    if (!pending) return;
    HIPCHECK(hipStreamSynchronize(st));          // (already drained when the caller has just read its own counters)
    const bool u16_kernels = b->d_m_col == nullptr && (m <= 1 || m == 7);
    if (b->h_misfit[1] == 0u && b->tun.compact != 1 && u16_kernels) b->y_type = YT_U16;
    else if (b->h_misfit[0] == 0u) b->y_type = YT_F32;
}

// The host side of every ETS / AutoETS fit.  WHAT runs where and when is decided by plan_fit_schedule (host_fit_schedule.hpp) from
// plain values; this function looks the launchers up, builds the per-slot arguments, sizes the scratches from the plan and walks
// the plan once.
static_assert(N_GROUP_CLASSES == FIT_GROUP_CLASSES && GROUP_DAMPED_MUL == 0 && GROUP_GENERAL == 1 && GROUP_ADDITIVE == 2, "host_fit_schedule.hpp names the group classes by number");
void launch_fit_slots(AnofoxHipBatch *b, const std::vector<int> &specs, const int32_t *d_len, int m, bool skip_constant,
                      hipStream_t st)
{
    const size_t n = b->n, ld = b->ld, n_spec = specs.size();
    // fork: aux streams wait for everything queued on `st` so far
    HIPCHECK(hipEventRecord(b->ev_fit0, st));
    // several periods in one block (columns grouped by period in blocks of 64): the round kernels read the period PER LANE, so the
    // batch runs the ordinary schedule -- compaction and the dense re-gather pack survivors of different periods into one wave;
    // the final pass sweeps the original blocks (one period each)
    const bool merged = b->d_m_col != nullptr;
    // what the kernels stream: the fp64 block, or a compact copy of it (compact_storage_decide: every observation survives the narrower type)
    const int yt = b->y_type;
    const void *ybase = yt == YT_F32 ? (const void *)b->d_yc32 : (yt == YT_U16 ? (const void *)b->d_yc16 : (const void *)b->d_y);
    const int ybytes = yt == YT_F32 ? 4 : (yt == YT_U16 ? 2 : 8);
    const int lds_limit = merged ? ETS_MERGED_LDS_PERIOD : ETS_LDS_PERIOD;      // largest period whose seasonal ring stays in LDS
    // the launchers of every spec and class, and the schedule's input: what the decisions read, as values
    std::vector<FitLaunchers> fns_of(n_spec);
    GroupLaunchFn group_fn[N_GROUP_CLASSES];
    FitScheduleInput in;
    in.n = n; in.ld = ld; in.t_max = b->t_max; in.m = m;
    for (size_t k = 0; k < n_spec; k++) {
        const int id = specs[k], ms = spec_season(id) != 0 ? m : 1;
        fns_of[k] = ets_fit_launcher(id, (merged && ms != 1) ? (ms > lds_limit ? ETS_PERLANE_HBM : ETS_PERLANE_LDS) : ms, yt);
        if (!fns_of[k].round_seq || !fns_of[k].round_spec || !fns_of[k].round_auto || !fns_of[k].final) throw HipFail{"no kernel for ETS spec id " + std::to_string(id)};
        in.specs.push_back(FitSpec{id, spec_has_mult(id), spec_trend_idx(id) == 4, spec_season(id) != 0, fns_of[k].round_k4 && fns_of[k].round_auto_k4,
                                   fns_of[k].nm_scratch_per_wg, ets_group_class(id)});
    }
    for (int c = 0; c < N_GROUP_CLASSES; c++) { group_fn[c] = ets_group_launcher(c, m, yt); in.group_launcher[c] = group_fn[c] != nullptr; }
    in.live_pos = b->live_pos; in.live_all = b->live_all; in.use_pos = b->use_pos; in.none_pos = b->none_pos;
    in.fixed_params = b->fixed_params; in.merged = merged; in.fp64 = yt == YT_F64; in.use_gather = b->use_gather; in.gather_budget = b->gather_budget;
    in.seq_rounds = b->seq_rounds; in.seq_rounds_env = b->seq_rounds_env;
    in.spec_below = b->spec_below; in.spec_below_md = b->spec_below_md; in.spec2_below = b->spec2_below; in.spec2_below_md = b->spec2_below_md;
    in.n_lanes = std::min<int>(N_AUX_STREAMS, b->n_slots_cap);
    {
        const Tunables &t = b->tun;
        in.budgets = t.budgets; in.k4 = t.k4; in.k4_top = t.k4_top; in.k4_top_below = t.k4_top_below;
        in.fill_policy = t.fill_policy; in.fill_target = t.fill_target; in.fill_late_div = t.fill_late_div; in.fill_s2_div = t.fill_s2_div;
        in.top_boost_n = t.top_boost_n; in.top_boost_pct = t.top_boost_pct; in.prio_top = t.prio_top;
        in.group_launch = t.group_launch; in.group_split = t.group_split; in.dm_head_rounds = t.dm_head_rounds; in.gather_cols = t.gather_cols;
    }
    in.lim = FitLimits{NM_BLOCK, NM_K, GROUP_MAX_SLOTS, N_AUX_STREAMS, TINY_BATCH_PROBLEMS, lds_limit, 2 * 1024 * 64};
    const FitSchedule plan = plan_fit_schedule(in);
    if (!plan.error.empty()) throw HipFail{plan.error};
    auto spec_stream = [&](size_t oi) -> hipStream_t { return plan.inline_stream ? st : b->aux[plan.stream_of[oi]]; };
    std::vector<FitArgs> args(n_spec);
    std::vector<FitLaunchers> fns(n_spec);
    for (size_t oi = 0; oi < n_spec; oi++) {
        const size_t k = plan.order[oi];
        const int id = specs[k];
        auto &lane = b->lanes[plan.lane_of[oi]];
        const int se = spec_season(id), ti = spec_trend_idx(id);
        const int tt = ti == 0 ? 0 : (ti <= 2 ? 1 : 2);
        FitArgs &a = args[oi];
        a = FitArgs{};
        a.y = (const double *)ybase; a.ld = ld; a.len = d_len; a.n_series = (int)n; a.t_rows = (int)std::max<size_t>(b->t_max, 1);
        a.m = se != 0 ? m : 1; a.h = b->h;
        a.l0 = b->d_l0 + (size_t)(se * 3 + tt) * ld;
        a.b0 = b->d_b0 + (size_t)(se * 3 + tt) * ld;
        a.fig = se == 1 ? b->d_fig_add : (se == 2 ? b->d_fig_mul : nullptr);
        a.fig_ld = ld;
        a.flags = b->d_flags;
        a.need_positive = spec_has_mult(id) ? 1 : 0;
        a.skip_constant = skip_constant ? 1 : 0;
        a.n_param = spec_n_param(id, a.m);
        a.aicc = b->d_aicc + k * ld;
        a.yhat = b->d_yhat_slots + k * n * (size_t)b->h;
        a.status = b->d_status_slots + k * ld;
        a.evals = b->d_evals_slots + k * ld;
        a.iters = b->d_iters_slots + k * ld;
        a.passes = b->d_passes_slots + k * ld;
        a.st = lane.st;
        a.ring_scratch = nullptr;
        a.m_col = b->d_m_col;
        if (b->sd_in_final && n_spec == 1) { a.mean = b->d_mean; a.sd_out = b->d_sd; }
        a.lane_stats = b->d_lane_stats ? b->d_lane_stats + 2 * k : nullptr;
        a.wave_trace = b->d_wave_trace;
        fns[oi] = fns_of[k];
    }
    // Periods above the LDS limit keep the seasonal ring of every lane in HBM: one area per (spec, workgroup of the widest launch)
    {
        size_t n_long = 0;
        for (size_t oi = 0; oi < n_spec; oi++) if (args[oi].m > lds_limit) n_long++;
        if (n_long) {
            const size_t per_spec = plan.scratch_workgroups * (size_t)m * 64u;
            if ((double)n_long * (double)per_spec * 8.0 > 64.0 * 1073741824.0)
                throw HipFail{"seasonal period " + std::to_string(m) + " on " + std::to_string(n) + " series needs more than 64 GiB of ring scratch: shard the batch"};
            double *base = ensure_ring(b, n_long * per_spec);
            size_t k = 0;
            for (size_t oi = 0; oi < n_spec; oi++) if (args[oi].m > lds_limit) { args[oi].ring_scratch = base + (k++) * per_spec; args[oi].ring_scratch_doubles = per_spec; }
        }
    }
    // Specs whose round kernels keep the Nelder-Mead simplex out of LDS: a global scratch per stream, one slice per workgroup of the
    // widest launch
    for (size_t oi = 0; oi < n_spec; oi++) {
        if (!fns[oi].nm_scratch_per_wg) continue;
        auto &lane = b->lanes[plan.lane_of[oi]];
        const size_t need = (plan.scratch_workgroups + 8) * fns[oi].nm_scratch_per_wg;         // (+ the waves that round a launch up to whole workgroups)
        if (lane.nm_scratch_doubles < need) {
            if (lane.nm_scratch) b->retired.push_back(lane.nm_scratch);
            lane.nm_scratch = nullptr; lane.nm_scratch_doubles = 0;
            lane.nm_scratch = dalloc<double>(need);
            lane.nm_scratch_doubles = need;
        }
        args[oi].nm_scratch = lane.nm_scratch; args[oi].nm_scratch_doubles = lane.nm_scratch_doubles;
    }
    // the gather blocks the plan asks for (none without the gather)
    for (size_t oi = 0; oi < n_spec; oi++) {
        auto &lane = b->lanes[plan.lane_of[oi]];
        size_t cols = plan.gather_cols[oi];
        if (cols == 0 || (lane.ybuf && lane.ybuf_cols >= cols)) continue;             // (a larger block from an earlier run serves as well)
        if (lane.ybuf) {
            HIPCHECK(hipDeviceSynchronize());                                          // an earlier run of this batch may still read the old block
            dev_free(lane.ybuf, true);
            lane.ybuf = nullptr; lane.ybuf_cols = 0;
        }
        while (cols >= 64) {
            try { lane.ybuf = dalloc<double>(std::max<size_t>(b->t_max, 1) * cols); lane.ybuf_cols = cols; break; }
            catch (const HipFail &f) {
                if (!f.oom) throw;
                cols = cols / 2 / 64 * 64;                 // a co-resident allocator holds memory: half the columns, in the end none
                if (cols < 1024) cols = 0;
            }
        }
    }
    // what round r of slot oi runs on: its step of the plan, and the series list and block its lane holds by then
    auto set_round = [&](FitArgs &a, const size_t oi, const int r) {
        const RoundStep &s = plan.steps[oi][(size_t)r];
        const auto &lane = b->lanes[plan.lane_of[oi]];
        a.first_round = (r == 0);
        a.wave_trace_tag = ((unsigned long long)specs[plan.order[oi]] << 32) | ((unsigned long long)r << 16);
        a.wave_prio = s.wave_prio;
        a.budget = s.budget; a.budget_seq = s.budget_seq; a.spec_below = s.spec_below; a.spec2_below = s.spec2_below;
        a.y_round = a.y; a.ld_round = ld; a.series_of = nullptr; a.n_active = nullptr; a.gathered = 0;
        if (s.source == SRC_POSITIVE) {
            // mixed batch: this spec is admissible for the strictly positive series only -- its first round runs on their dense list
            // (built once per group) instead of sweeping every wave for a few live lanes
            a.series_of = b->d_pos_map; a.n_active = b->d_pos_cnt;
            if (b->d_ypos) { a.y_round = b->d_ypos; a.gathered = 1; a.gather_cap = (int)ld; }
        } else if (s.source == SRC_COMPACTED) {
            a.series_of = lane.map[r & 1]; a.n_active = lane.cnt + (r % 3);
            if (b->use_gather && lane.ybuf) { a.y_round = lane.ybuf; a.ld_round = lane.ybuf_cols; a.gathered = 1; a.gather_cap = (int)lane.ybuf_cols; }
        }
    };
    auto retire_nonpositive = [&](const size_t oi, hipStream_t sq) {
        const auto &lane = b->lanes[plan.lane_of[oi]];
        hipLaunchKernelGGL(retire_nonpositive_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, sq, (int)n, d_len, b->d_notpos,
                           args[oi].status, lane.st.done, lane.st.passes, lane.st.evals, lane.st.iters);
    };
    if (plan.grouped) {
        // every argument of every group round is known: the [round][slot] table goes to the device in one copy, ahead of
        // everything the group streams run
        const size_t cells = (size_t)plan.total_rounds * plan.n_slots;
        if (b->ev_group_tab) HIPCHECK(hipEventSynchronize(b->ev_group_tab));      // (the previous run's copy has been read)
        else HIPCHECK(hipEventCreateWithFlags(&b->ev_group_tab, hipEventDisableTiming));
        if (b->group_tab_cap < cells) {
            if (b->d_group_tab) b->retired.push_back(b->d_group_tab);            // (an earlier run's launches may still read it)
            pin_free(b->h_group_tab);
            b->d_group_tab = nullptr; b->h_group_tab = nullptr; b->group_tab_cap = 0;
            b->d_group_tab = dalloc<FitArgs>(cells);
            b->h_group_tab = (FitArgs *)pin_alloc_bytes(cells * sizeof(FitArgs));
            b->group_tab_cap = cells;
        }
        for (size_t oi = 0; oi < n_spec; oi++) {
            if (plan.dead[oi]) continue;
            FitArgs t = args[oi];
            for (int r = 0; r < plan.total_rounds; r++) { set_round(t, oi, r); b->h_group_tab[(size_t)r * plan.n_slots + plan.slot_of[oi]] = t; }
        }
        HIPCHECK(hipMemcpyAsync(b->d_group_tab, b->h_group_tab, cells * sizeof(FitArgs), hipMemcpyHostToDevice, st));
        HIPCHECK(hipEventRecord(b->ev_group_tab, st));
        HIPCHECK(hipEventRecord(b->ev_fork, st));
    }
    for (int q : plan.fork_streams) HIPCHECK(hipStreamWaitEvent(b->aux[q], plan.grouped ? b->ev_fork : b->ev_fit0, 0));
    // the specs with nothing to fit: their per-series outputs
    for (size_t oi = 0; oi < n_spec; oi++)
        if (plan.dead[oi]) {
            const FitArgs &a = args[oi];
            hipLaunchKernelGGL(retire_nonpositive_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, spec_stream(oi), (int)n, d_len,
                               b->d_notpos, a.status, a.st.done, a.st.passes, a.st.evals, a.st.iters, a.aicc, a.passes, a.evals, a.iters);
        }
    if (b->fixed_params) {
        // given smoothing parameters: no rounds at all -- admissibility + parameters, then the final pass below
        for (size_t oi = 0; oi < n_spec; oi++) {
            const int id = specs[plan.order[oi]];
            FitArgs &a = args[oi];
            // coordinates present in this spec, in optimiser order (alpha, [beta*], [gamma*], [phi])
            double x[4] = {0.0, 0.0, 0.0, 0.0};
            int d = 0;
            x[d++] = b->fixed_x[0];
            if (spec_trend_idx(id) != 0) x[d++] = b->fixed_x[1];
            if (spec_season(id) != 0) x[d++] = b->fixed_x[2];
            if (spec_trend_idx(id) == 2 || spec_trend_idx(id) == 4) x[d++] = b->fixed_x[3];
            hipLaunchKernelGGL(ets_fixed_setup_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, spec_stream(oi), (int)n, ld, d_len,
                               b->d_flags, spec_season(id) != 0 ? 1 : 0, a.m, a.n_param, a.need_positive, d, x[0], x[1], x[2], x[3], a.status,
                               a.st.sim, a.st.evals, a.st.iters, a.st.passes, a.st.done);
        }
        LAUNCHCHECK("ETS fixed-parameter setup");
    }
    // round r of a spec with a launch chain of its own: the compaction and gather of its running problems, then its round launch
    auto enqueue_round = [&](const int r, const size_t oi) {
        if (plan.dead[oi]) return;
        const RoundStep &s = plan.steps[oi][(size_t)r];
        auto &lane = b->lanes[plan.lane_of[oi]];
        hipStream_t sq = spec_stream(oi);
        FitArgs &a = args[oi];
        set_round(a, oi, r);
        if (s.source == SRC_POSITIVE) retire_nonpositive(oi, sq);
        else if (s.source == SRC_COMPACTED) {
            const int32_t *prev_map = (r == 1) ? nullptr : lane.map[(r - 1) & 1];
            const int32_t *prev_cnt = (r == 1) ? nullptr : lane.cnt + ((r - 1) % 3);
            if (r == 1) HIPCHECK(hipMemsetAsync(lane.cnt, 0, 3 * sizeof(int32_t), sq));      // then the counters rotate: no more memsets
            launch_compact(prev_map, prev_cnt, (int)n, lane.st.done, lane.map[r & 1], lane.cnt + (r % 3), sq, lane.cnt + ((r + 1) % 3));
            if (a.gathered)
                launch_gather_columns(a.y, ld, lane.map[r & 1], lane.cnt + (r % 3), (int)n, (int)b->t_max, lane.ybuf, lane.ybuf_cols, sq,
                                      (int)lane.ybuf_cols, ybytes);
        }
        const FitLaunchFn f = s.kind == RK_SEQ ? fns[oi].round_seq : s.kind == RK_SPEC ? fns[oi].round_spec : s.kind == RK_SPEC2 ? fns[oi].round_spec2 :
                              s.kind == RK_AUTO ? fns[oi].round_auto : s.kind == RK_K4 ? fns[oi].round_k4 : fns[oi].round_auto_k4;
        f(a, sq);
        b->fit_launches++;
    };
    // round r of group g, on the group's stream: ONE compaction and ONE gather launch for all its slots, then the one group launch
    auto enqueue_group_round = [&](const int r, const size_t g) {
        const std::vector<size_t> &slots = plan.groups[g].slots;
        hipStream_t sg = b->aux[plan.groups[g].stream];
        if (r == 0) {
            // the slots' rotating counters, cleared once before the first compaction (the per-spec chains' memsets)
            int32_t *zero[GROUP_MAX_SLOTS] = {};
            for (size_t k = 0; k < slots.size(); k++) zero[k] = b->lanes[plan.lane_of[slots[k]]].cnt;
            launch_group_zero3((int)slots.size(), zero, sg);
        }
        GroupCompactArgs gc{}; gc.n_series = (int)n;
        GroupGatherArgs gg{}; gg.t_max = (int)b->t_max; gg.elem_bytes = ybytes; gg.y = ybase; gg.ld = ld;
        int gg_cols = 0;
        GroupRoundArgs ga{};
        ga.n_slots = (int)slots.size();
        for (int k = 0; k < ga.n_slots; k++) {
            const size_t oi = slots[(size_t)k];
            const RoundStep &s = plan.steps[oi][(size_t)r];
            auto &lane = b->lanes[plan.lane_of[oi]];
            if (s.source == SRC_POSITIVE) retire_nonpositive(oi, sg);
            else if (s.source == SRC_COMPACTED) {
                const int c = gc.n_slots++;
                gc.prev[c] = (r == 1) ? nullptr : lane.map[(r - 1) & 1]; gc.n_prev[c] = (r == 1) ? nullptr : lane.cnt + ((r - 1) % 3); gc.done[c] = lane.st.done;
                gc.next[c] = lane.map[r & 1]; gc.n_next[c] = lane.cnt + (r % 3); gc.n_clear[c] = lane.cnt + ((r + 1) % 3);
                if (b->use_gather && lane.ybuf) {
                    const int j = gg.n_slots++;
                    gg.series_of[j] = lane.map[r & 1]; gg.n_active[j] = lane.cnt + (r % 3);
                    gg.out[j] = lane.ybuf; gg.ld_out[j] = lane.ybuf_cols; gg.cap[j] = (int)lane.ybuf_cols;
                    gg_cols = std::max(gg_cols, (int)std::min<size_t>(n, lane.ybuf_cols));
                }
            }
            ga.spec[k] = specs[plan.order[oi]];
            ga.k4[k] = s.k4 ? 1 : 0;
            ga.start[k + 1] = ga.start[k] + s.workgroups;
        }
        if (gc.n_slots > 0) launch_group_compact(gc, sg);
        if (gg.n_slots > 0) launch_group_gather(gg, gg_cols, sg);
        group_fn[plan.groups[g].cls](b->d_group_tab + (size_t)r * plan.n_slots + plan.slot_of[slots[0]], ga, m, sg);
        b->fit_launches++;
    };
    // the head start of the damped multiplicative-trend chains: their first rounds, then the other streams wait behind them
    if (plan.head_rounds > 0) {
        for (int r = 0; r < plan.head_rounds; r++) {
            if (plan.grouped) enqueue_group_round(r, 0);
            else for (size_t oi = 0; oi < n_spec; oi++) if (plan.head[oi]) enqueue_round(r, oi);
        }
        LAUNCHCHECK("ETS fit head rounds");
        if (plan.grouped) {
            HIPCHECK(hipEventRecord(b->ev_join[0], b->aux[0]));
            for (size_t g = 1; g < plan.groups.size(); g++) HIPCHECK(hipStreamWaitEvent(b->aux[plan.groups[g].stream], b->ev_join[0], 0));
        } else {
            for (size_t od = 0; od < n_spec; od++) if (plan.head[od]) HIPCHECK(hipEventRecord(b->ev_join[plan.stream_of[od]], spec_stream(od)));
            for (size_t oi = 0; oi < n_spec; oi++) {
                if (plan.dead[oi] || plan.head[oi]) continue;
                for (size_t od = 0; od < n_spec; od++) if (plan.head[od]) HIPCHECK(hipStreamWaitEvent(spec_stream(oi), b->ev_join[plan.stream_of[od]], 0));
            }
        }
    }
    for (int r = 0; r < plan.total_rounds; r++) {
        const bool ahead = r < plan.head_rounds;          // (the head slots' round is already enqueued)
        if (plan.grouped) {
            for (size_t g = 0; g < plan.groups.size(); g++) if (!(ahead && plan.head[plan.groups[g].slots[0]])) enqueue_group_round(r, g);
        } else
            for (size_t oi = 0; oi < n_spec; oi++) if (!(ahead && plan.head[oi])) enqueue_round(r, oi);
        LAUNCHCHECK("ETS fit round");
    }
    // fixed parameters: the one streamed pass IS the workload -- the fit events bracket exactly that launch, on its stream
    if (b->fixed_params && n_spec == 1) HIPCHECK(hipEventRecord(b->ev_fit0, spec_stream(0)));
    for (size_t oi = 0; oi < n_spec; oi++) if (!plan.dead[oi]) fns[oi].final(args[oi], spec_stream(oi));
    if (b->fixed_params && n_spec == 1) HIPCHECK(hipEventRecord(b->ev_fit1, spec_stream(0)));
    LAUNCHCHECK("ETS final pass");
    for (int q : plan.fork_streams) {
        HIPCHECK(hipEventRecord(b->ev_join[q], b->aux[q]));
        HIPCHECK(hipStreamWaitEvent(st, b->ev_join[q], 0));
    }
    if (!(b->fixed_params && n_spec == 1)) HIPCHECK(hipEventRecord(b->ev_fit1, st));
    b->timed_fit = true;
    b->n_problems += (uint64_t)n_spec * n;
    b->insp_args = args; b->insp_fns = fns; b->insp_stream = plan.stream_of; b->insp_m = m;
    b->insp_spec.resize(n_spec);
    for (size_t oi = 0; oi < n_spec; oi++) b->insp_spec[oi] = specs[plan.order[oi]];
    b->insp_ok = true;
}

// CrostonClassic / CrostonSBA / TSB: one streamed pass (croston_kernel).  ADIDA / IMAPA: that pass gives every series' aggregation
// level K, then SESopt on the level sums (agg_ses_kernel).  IMAPA sizes its per-(level, series) terms by the batch's largest K, read
// back once: the one host wait of these models (include/anofox_fcst_hip.h, anofox_hip_batch_run).
void run_intermittent(AnofoxHipBatch *b, const int32_t *d_len, hipStream_t st)
{
    const ModelType m = b->plan.model;
    IntermittentArgs a{};
    a.y = b->d_y; a.ld = b->ld; a.len = d_len; a.n_series = (int)b->n;
    a.kind = m == M_CrostonClassic ? IK_CROSTON : m == M_CrostonSBA ? IK_SBA : m == M_TSB ? IK_TSB : m == M_ADIDA ? IK_ADIDA : IK_IMAPA;
    a.h = b->h;
    a.n_groups = intermittent_groups((int)b->n);
    a.yhat = b->d_yhat; a.detail = b->d_detail; a.level = b->d_im_level; a.group_max = b->d_im_gmax;
    HIPCHECK(hipMemsetAsync(b->d_im_gmax, 0, ((size_t)a.n_groups + 1) * sizeof(int32_t), st));
    launch_croston(a, st);
    if (a.kind == IK_ADIDA) launch_agg_ses(a, st);
    if (a.kind == IK_IMAPA) {
        int32_t k_max = 0;
        HIPCHECK(hipMemcpyAsync(&k_max, b->d_im_gmax + a.n_groups, sizeof k_max, hipMemcpyDeviceToHost, st));
        HIPCHECK(hipStreamSynchronize(st));
        const size_t need = (size_t)std::max(k_max, 0) * b->ld;
        if (b->im_fc_elems < need) {
            if (b->d_im_fc) b->retired.push_back(b->d_im_fc);
            b->d_im_fc = nullptr; b->im_fc_elems = 0;
            b->d_im_fc = dalloc<double>(need);
            b->im_fc_elems = need;
        }
        a.level_fc = b->d_im_fc; a.n_levels = k_max;
        try { launch_agg_ses(a, st); }
        catch (const std::exception &e) { throw HipFail{e.what()}; }
    }
    b->n_problems += b->n;
}

// DynamicTheta / DynamicOptimizedTheta: for a period m > 1 the season test and the indices first (theta_season_kernel, into a
// [m x ld] buffer grown on demand, no host wait), then one fit per series (theta_fit_kernel).
void run_theta(AnofoxHipBatch *b, int period, const int32_t *d_len, hipStream_t st)
{
    ThetaArgs a{};
    a.y = b->d_y; a.ld = b->ld; a.len = d_len; a.n_series = (int)b->n;
    a.kind = b->plan.model == M_DynamicOptimizedTheta ? TK_DOTM : TK_DSTM;
    a.h = b->h;
    a.m = period > 1 ? period : 1;                          // <= ETS_MAX_PERIOD here: longer periods failed loudly in run_group
    a.m_col = (b->d_m_col && a.m > 1) ? b->d_m_col : nullptr;
    if (a.m > 1) {
        const size_t need = (size_t)a.m * b->ld;
        if (b->th_sidx_elems < need) {
            if (b->d_th_sidx) b->retired.push_back(b->d_th_sidx);      // (an earlier group's launches may still read it)
            b->d_th_sidx = nullptr; b->th_sidx_elems = 0;
            b->d_th_sidx = dalloc<double>(need);
            b->th_sidx_elems = need;
        }
    }
    a.sidx = b->d_th_sidx; a.adjusted = b->d_th_adj;
    a.yhat = b->d_yhat; a.detail = b->d_detail; a.evals = b->d_evals_total;
    launch_theta(a, st);
    b->n_problems += b->n;
}

// the regressors take part for ARIMA / AutoARIMA only (forecast.rs forecast_with_exog: every other model ignores them)
bool exog_in_force(const AnofoxHipBatch *b) { return b->exog_k > 0 && (b->plan.model == M_ARIMA || b->plan.model == M_AutoARIMA); }

// ARIMAX: one kernel per batch (three sweeps per series); the per-series coefficient buffers are allocated by the first run
void run_exog(AnofoxHipBatch *b, const int32_t *d_len, hipStream_t st)
{
    if (!b->d_exog_b0) {
        b->d_exog_b0 = dalloc<double>(b->ld);
        b->d_exog_beta = dalloc<double>((size_t)EXOG_MAX_REGRESSORS * b->ld);
        b->d_exog_used = dalloc<uint32_t>(b->ld);
    }
    ExogArgs a{};
    a.y = b->d_y; a.ld = b->ld; a.len = d_len; a.n_series = (int)b->n;
    a.k = b->exog_k; a.h = b->h; a.t_rows = std::max<size_t>(b->t_max, 1);
    a.x = b->d_exog_x; a.f = b->d_exog_f;
    a.yhat = b->d_yhat; a.status = b->d_status; a.model_code = b->d_model_code;
    a.b0 = b->d_exog_b0; a.beta = b->d_exog_beta; a.used = b->d_exog_used;
    try { launch_exog_arimax(a, st); }
    catch (const std::exception &e) { throw HipFail{e.what()}; }
    b->n_problems += b->n;
}

void run_group(AnofoxHipBatch *b, int period, const int32_t *d_len, hipStream_t st)
{
    const Plan &p = b->plan;
    const size_t n = b->n, ld = b->ld;
    const int blocks256 = (int)((n + 255) / 256);
    // sd_in_final: the batch has ONE candidate spec, whose final pass carries the second sweep of the intervals' sd (FitArgs::sd_out)
    b->sd_in_final = false;
    auto prep = [&](int m, bool states, bool sd_in_final = false, int skip_types = 0) {
        PrepArgs a{};
        a.skip_sd = sd_in_final ? 1 : 0;
        a.skip_types = skip_types;
        b->sd_in_final = sd_in_final;
        a.y = b->d_y; a.ld = ld; a.len = d_len; a.n_series = (int)n; a.m = m;
        a.m_col = (states && m >= 2) ? b->d_m_col : nullptr;
        a.mean = b->d_mean; a.sd = b->d_sd; a.flags = b->d_flags;
        a.scratch = nullptr;
        if (states) {
            if (m >= 2) ensure_fig(b, m);
            a.fig_add = b->d_fig_add; a.fig_mul = b->d_fig_mul; a.l0 = b->d_l0; a.b0 = b->d_b0;
            a.t_rows = (int)std::max<size_t>(b->t_max, 1);
            if (m >= 2 && m <= ETS_MAX_PERIOD && !(m == 7 && !a.m_col)) {       // season_figures_kernel: series longer than its LDS use a scratch
                const size_t sc = season_scratch_doubles((int)n, a.t_rows, m);
                if (sc) a.scratch = ensure_prep_scratch(b, sc);
            }
        }
        launch_prep(a, st);
    };
    auto simple = [&](int kind, int per, int window) {
        SimpleArgs a{};
        a.y = b->d_y; a.ld = ld; a.len = d_len; a.n_series = (int)n;
        a.kind = kind; a.h = b->h; a.period = per; a.window = window;
        a.yhat = b->d_yhat; a.status = b->d_status;
        launch_simple(a, st);
    };
    auto finish = [&]() { hipLaunchKernelGGL(finish_status_kernel, dim3(blocks256), dim3(256), 0, st, (int)n, d_len, b->d_detail, b->d_status); };

    // A period the kernels cannot hold fails the group's series loudly (COMPUTATION_ERROR naming the cap) -- never a silent
    // non-seasonal fit.  The reference takes any period (forecast.rs:528-537); 2,048 covers every calendar period.
    if (exog_in_force(b)) {              // ARIMAX: the intervals' mean / sd come from y, as for every model
        prep(1, false);
        run_exog(b, d_len, st);
        LAUNCHCHECK("ARIMAX");
        return;
    }
    const bool uses_period = p.model == M_AutoETS || p.model == M_HoltWinters || p.model == M_SeasonalES || p.model == M_SeasonalESOptimized || is_theta_model(p.model) ||
                             (p.model == M_ETS && (p.ets_spec_id < 0 || spec_season(p.ets_spec_id) != 0));
    const bool arima_period = p.model == M_AutoARIMA && period > ETS_MAX_PERIOD;      // seasonal ARIMA terms: LDS rings up to m = 24, an HBM scratch ring up to 2,048
    if ((uses_period && period > ETS_MAX_PERIOD) || arima_period) {
        prep(1, false);
        HIPCHECK(hipMemsetAsync(b->d_detail, 0, ld * sizeof(int32_t), st));
        hipLaunchKernelGGL(fill_i32_kernel, dim3(blocks256), dim3(256), 0, st, (int)n, b->d_detail, (int32_t)FIT_PERIOD);
        finish();
        LAUNCHCHECK("period cap");
        return;
    }

    switch (p.model) {
    case M_Naive: prep(1, false); simple(SK_NAIVE, 1, 0); break;
    case M_SeasonalNaive: prep(1, false); simple(SK_SEASONAL_NAIVE, period, 0); break;
    case M_SMA: prep(1, false); simple(SK_SMA, 1, b->opt.window > 0 ? b->opt.window : std::max(period, 3)); break;
    case M_RandomWalkDrift: prep(1, false); simple(SK_DRIFT, 1, 0); break;
    case M_ARIMA: prep(1, false); simple(SK_TOY_ARIMA, 1, 0); break;
    case M_SeasonalWindowAverage: {
        prep(1, false);
        SimpleArgs a{};
        a.y = b->d_y; a.ld = ld; a.len = d_len; a.n_series = (int)n;
        a.h = b->h; a.period = period;
        a.yhat = b->d_yhat; a.status = b->d_status;
        launch_swa(a, st);
        break;
    }
    case M_SES: prep(1, false); run_classic(b, CK_SES, d_len, 1, 0, 0.3, 0, nullptr, 0, 0, false, st); finish(); break;
    case M_SESOptimized: prep(1, false); run_classic(b, CK_SES, d_len, 1, 1, 0.0, 0, nullptr, 0, 0, false, st); finish(); break;
    case M_Holt: prep(1, false); run_classic(b, CK_HOLT, d_len, 1, 1, 0.0, 0, nullptr, 0, 0, false, st); finish(); break;
    case M_HoltWinters: {
        int m = std::max(period, 2);
        prep(1, false);
        // fewer than two seasons -> Holt's linear trend under the same name (the crate's fallback, pinned by
        // test/sql/ts_forecast_exp_smoothing.test:498-503 and ts_forecast_params.test:203-207)
        hipLaunchKernelGGL(holt_winters_plan_kernel, dim3(blocks256), dim3(256), 0, st, (int)n, d_len, m, b->d_mask, b->d_detail, (const int32_t *)b->d_m_col);
        if (m <= ETS_MAX_PERIOD) run_classic(b, CK_HW, d_len, m, 1, 0.0, 2 * m, b->d_mask, 1u, 0, false, st);
        run_classic(b, CK_HOLT, d_len, 1, 1, 0.0, 0, b->d_mask, 2u, 0, false, st);
        finish();
        break;
    }
    case M_SeasonalES: case M_SeasonalESOptimized: {
        int m = std::max(period, 2);
        prep(1, false);
        if (m > ETS_MAX_PERIOD) HIPCHECK(hipMemsetAsync(b->d_detail, 0xff, ld * sizeof(int32_t), st));
        else run_classic(b, CK_SEASONAL_ES, d_len, m, p.model == M_SeasonalESOptimized ? 1 : 0, 0.1, m, nullptr, 0, 0, false, st);
        finish();
        break;
    }
    case M_ETS:
        if (p.ets_spec_id >= 0) {
            int id = p.ets_spec_id;
            int m = 1;
            if (spec_season(id) != 0 && period > 1) m = period;
            else id = id - spec_season(id);             // forecast.rs:1347-1351: no usable period -> non-seasonal
            // (one candidate spec: its final pass carries the intervals' sd, and only its own season type is prepared)
            prep(m, true, !(spec_season(id) != 0 && m > ETS_MAX_PERIOD), spec_season(id) == 2 ? 0 : 2);
            if (spec_season(id) != 0 && m > ETS_MAX_PERIOD) {
                HIPCHECK(hipMemsetAsync(b->d_detail, 0x04, ld * sizeof(int32_t), st));   // != FIT_OK: unsupported period
                finish();
                break;
            }
            std::vector<int> specs{id};
            compact_storage_decide(b, compact_storage_begin(b, d_len, st), st, m);
            launch_fit_slots(b, specs, d_len, m, false, st);
            hipLaunchKernelGGL(explicit_select_kernel, dim3((unsigned)((n * (size_t)std::max(b->h, 1) + 255) / 256)), dim3(256), 0, st, (int)n, b->h, d_len, b->d_status_slots,
                               b->d_yhat_slots, b->d_passes_slots, b->d_evals_slots, b->d_yhat, b->d_detail, b->d_passes_total,
                               b->d_evals_total);
            finish();
        } else {
            prep(1, false);
            // default chain decided by length only: mark every usable series for fallback
            HIPCHECK(hipMemsetAsync(b->d_mask, 0x01, ld * sizeof(uint32_t), st));
            hipLaunchKernelGGL(fallback_plan_kernel, dim3(blocks256), dim3(256), 0, st, (int)n, d_len, period, b->d_mask, b->d_detail, (const int32_t *)nullptr);
            if (period > 1 && period <= ETS_MAX_PERIOD)
                run_classic(b, CK_HW, d_len, period, 1, 0.0, 2 * period, b->d_mask, 1u, 0, false, st);
            run_classic(b, CK_HOLT, d_len, 1, 1, 0.0, 0, b->d_mask, 2u, 0, false, st);
            run_classic(b, CK_SES, d_len, 1, 0, 0.3, 0, b->d_mask, 3u, 0, false, st);
            finish();
        }
        break;
    case M_AutoETS: {
        int m = (period > 1 && period <= ETS_MAX_PERIOD) ? period : 1;
        prep(m, true);
        const bool compact_pending = compact_storage_begin(b, d_len, st);
        std::vector<int> specs;
        for (int id = 0; id < 30; id++) {
            if (spec_season(id) != 0 && m <= 1) continue;
            if (!spec_is_valid(id) || !pool_allows(p.pool, id)) continue;
            specs.push_back(id);
        }
        // slot order = spec-id order (first minimum wins ties in the selection)
        b->h_slot_spec.assign(specs.begin(), specs.end());
        HIPCHECK(hipMemcpyAsync(b->d_slot_spec, b->h_slot_spec.data(), b->h_slot_spec.size() * sizeof(int32_t), hipMemcpyHostToDevice, st));
        if (b->seq_rounds_env < 0) {
            // Choose the Nelder-Mead driver of the early rounds from the number of LIVE problems: strictly
            // positive series run every spec, the others only the additive ones.  One 4-byte read-back.
            hipLaunchKernelGGL(count_positive_kernel, dim3(1), dim3(1024), 0, st, (int)n, d_len, b->d_flags, b->d_count);
            int32_t cnt[2] = {0, 0};
            HIPCHECK(hipMemcpyAsync(cnt, b->d_count, sizeof cnt, hipMemcpyDeviceToHost, st));
            HIPCHECK(hipStreamSynchronize(st));             // (the compact copies' misfit counters have arrived too)
            size_t n_add = 0;
            for (int id : specs) if (!spec_has_mult(id)) n_add++;
            const double live = (double)cnt[0] * (double)specs.size() + (double)(cnt[1] - cnt[0]) * (double)n_add;
            b->seq_rounds = live >= 8.0 * 65536.0 ? 4 : 0;         // >= 8 problems per SIMD lane-slot: VALU-bound, go sequential
            b->use_pos = cnt[0] > 0 && (double)cnt[0] < 0.7 * (double)cnt[1];
            b->live_pos = cnt[0]; b->live_all = cnt[1];
        } else {
            b->use_pos = false;
            b->live_pos = b->live_all = -1;
        }
        compact_storage_decide(b, compact_pending, st, m);
        b->none_pos = b->live_all >= 0 && b->live_pos == 0;       // no strictly positive series at all: the 19 specs with a multiplicative component have nothing to fit
        if (b->use_pos || b->none_pos)
            hipLaunchKernelGGL(mark_nonpositive_kernel, dim3((unsigned)blocks256), dim3(256), 0, st, (int)n, d_len, b->d_flags, b->d_notpos);
        if (b->use_pos) {
            launch_compact(nullptr, nullptr, (int)n, b->d_notpos, b->d_pos_map, b->d_pos_cnt, st);
            if (b->use_gather) {
                if (!b->d_ypos) b->d_ypos = dalloc<double>(std::max<size_t>(b->t_max, 1) * ld);
                // (the strictly positive columns, in the storage type the fit streams)
                const int yt = b->y_type;
                launch_gather_columns(yt == YT_F32 ? (const void *)b->d_yc32 : (yt == YT_U16 ? (const void *)b->d_yc16 : (const void *)b->d_y), ld, b->d_pos_map,
                                      b->d_pos_cnt, (int)n, (int)b->t_max, b->d_ypos, ld, st, (int)ld, yt == YT_F32 ? 4 : (yt == YT_U16 ? 2 : 8));
            }
        }
        launch_fit_slots(b, specs, d_len, m, true, st);
        SelectArgs sa{};
        sa.n_series = (int)n; sa.h = b->h; sa.n_slots = (int)specs.size(); sa.ld = ld; sa.len = d_len;
        sa.aicc = b->d_aicc; sa.yhat_slots = b->d_yhat_slots; sa.slot_spec = b->d_slot_spec;
        sa.status_slots = b->d_status_slots; sa.passes_slots = b->d_passes_slots; sa.evals_slots = b->d_evals_slots;
        sa.yhat = b->d_yhat; sa.model_code = b->d_model_code; sa.status = b->d_detail; sa.fallback_mask = b->d_mask;
        sa.passes_total = b->d_passes_total; sa.evals_total = b->d_evals_total;
        launch_select(sa, st);
        hipLaunchKernelGGL(fallback_plan_kernel, dim3(blocks256), dim3(256), 0, st, (int)n, d_len, period, b->d_mask, b->d_detail, (const int32_t *)b->d_m_col);
        if (period > 1 && period <= ETS_MAX_PERIOD)
            run_classic(b, CK_HW, d_len, period, 1, 0.0, 2 * period, b->d_mask, 1u, 0, true, st);
        run_classic(b, CK_HOLT, d_len, 1, 1, 0.0, 0, b->d_mask, 2u, 0, true, st);
        run_classic(b, CK_SES, d_len, 1, 0, 0.3, 0, b->d_mask, 3u, 0, true, st);
        finish();
        break;
    }
    case M_AutoARIMA: {
        prep(1, false);
        ArimaArgs aa{};
        aa.y = b->d_y; aa.ld = ld; aa.len = d_len; aa.n_series = (int)n;
        aa.m = period > 1 ? period : 1;                        // <= 2,048 here: longer periods failed loudly above
        aa.long_scratch = nullptr;
        aa.m_col = (b->d_m_col && aa.m > 24) ? b->d_m_col : nullptr;      // merged batch of long periods: `period` is the largest
        if (aa.m > 24) aa.long_scratch = ensure_ring(b, arima_long_scratch_doubles((int)n, aa.m, arima_max_fit_waves()));
        aa.h = b->h;
        aa.ws = b->ar_w; aa.ws_bytes = b->ar_ws_bytes; aa.t_max = (int)std::max<size_t>(b->t_max, 1); aa.wlen = b->ar_wlen; aa.d = b->ar_d; aa.D = b->ar_D; aa.wmean = b->ar_wmean; aa.wsd = b->ar_wsd;
        aa.last_d0 = b->ar_l0; aa.last_d1 = b->ar_l1; aa.order = b->ar_order; aa.xbest = b->ar_x; aa.aicc = b->ar_aicc;
        aa.status = b->d_detail; aa.evals = b->d_evals_total; aa.passes = b->d_passes_total; aa.models = b->ar_models;
        aa.yhat = b->d_yhat; aa.model_code = b->d_model_code;
        aa.ml_refit = b->arima_method == ANOFOX_ARIMA_CSS_ML ? 1 : 0;
        aa.trace = b->tun.arima_trace;
        aa.lookahead = b->tun.arima_lookahead; aa.lookahead_depth = b->tun.arima_lookahead_depth; aa.spec_factor = b->tun.arima_spec_factor; aa.refit_budget = b->tun.arima_refit_budget; aa.queue_sort = b->tun.arima_queue_sort;
        aa.prep_lanes = b->tun.arima_prep_lanes < 1 ? 1 : (b->tun.arima_prep_lanes > 64 ? 64 : b->tun.arima_prep_lanes);
        aa.concurrent = &g_arima_runs; aa.shared_chunk_rounds = b->tun.arima_shared_chunk_rounds;
        HIPCHECK(hipEventRecord(b->ev_fit0, st));
        struct RunCount { RunCount() { g_arima_runs.fetch_add(1); } ~RunCount() { g_arima_runs.fetch_sub(1); } } run_count;
        try { b->fit_launches += launch_arima(aa, st); }
        catch (const std::exception &e) { throw HipFail{e.what()}; }
        HIPCHECK(hipEventRecord(b->ev_fit1, st));
        b->timed_fit = true;
        b->n_problems += n;
        finish();
        break;
    }
    case M_CrostonClassic: case M_CrostonSBA: case M_TSB: case M_ADIDA: case M_IMAPA: {
        prep(1, false);
        run_intermittent(b, d_len, st);
        finish();
        break;
    }
    case M_DynamicTheta: case M_DynamicOptimizedTheta: {
        prep(1, false);
        run_theta(b, period, d_len, st);
        finish();
        break;
    }
    default: throw HipFail{"model not implemented"};
    }
    LAUNCHCHECK(model_name(p.model));
}

void run_batch(AnofoxHipBatch *b, hipStream_t st)
{
    const size_t n = b->n, ld = b->ld;
    (void)hipGetLastError();     // the launch checks below must only see THIS run's errors (an earlier, already reported failure is sticky)
    b->fit_launches = 0;
    b->n_problems = 0;
    b->timed_fit = false;
    b->insp_ok = false;
    b->quiesced = false;         // (from here on, also when a launch below fails)
    b->last_stream = st;
    HIPCHECK(hipEventRecord(b->ev_start, st));
    if (b->d_lane_stats) HIPCHECK(hipMemsetAsync(b->d_lane_stats, 0, 2 * (size_t)b->n_slots_cap * sizeof(unsigned long long), st));
    if (!b->tun.wave_trace.empty() && b->n_slots_cap > 0) {
        constexpr size_t WAVE_TRACE_RECORDS = 4u << 20;
        if (!b->d_wave_trace) b->d_wave_trace = dalloc<unsigned long long>(4 + 4 * WAVE_TRACE_RECORDS);
        const unsigned long long head[4] = {0ull, (unsigned long long)WAVE_TRACE_RECORDS, 0ull, 0ull};
        HIPCHECK(hipMemcpyAsync(b->d_wave_trace, head, sizeof head, hipMemcpyHostToDevice, st));
        HIPCHECK(hipStreamSynchronize(st));        // (`head` is a stack array)
    }
    {
        const size_t nh = n * (size_t)std::max(b->h, 0);
        const size_t cover = std::max<size_t>(std::max(nh, ld), 1);
        hipLaunchKernelGGL(seed_outputs_kernel, dim3((unsigned)((cover + 255) / 256)), dim3(256), 0, st, (int)n, (int)ld, nh, (const int32_t *)b->d_len, b->d_status,
                           b->d_yhat, b->d_lo, b->d_hi, b->d_passes_total, b->d_evals_total, b->d_model_code);
        LAUNCHCHECK("output seeding");
    }
    // group series by seasonal period (all equal unless auto-detection ran).  Detection gives ~140 distinct periods per
    // thousand M5-like series and every group is one run of the whole pipeline, so series are grouped by the period the
    // model actually USES: none for the non-seasonal models.
    auto used_period = [&](int period) {
        switch (b->plan.model) {
        case M_Naive: case M_RandomWalkDrift: case M_ARIMA: case M_SES: case M_SESOptimized: case M_Holt: return 1;
        case M_CrostonClassic: case M_CrostonSBA: case M_TSB: case M_ADIDA: case M_IMAPA: return 1;
        case M_AutoARIMA:
            if (exog_in_force(b)) return 1;      // ARIMAX is not the seasonal search
            // a DETECTED period goes to the seasonal search exactly like an explicit one (forecast.rs:528-537 hands it to
            // forecast_auto_arima, :1448-1452 passes any period > 1 to with_seasonal_period): used up to 2,048 (rings in LDS up to
            // 24, in HBM scratch above), failing loudly beyond.  Rounds 2-3 made detected periods above 24 non-seasonal -- a
            // product limit the oracle had been written to share; both are gone.
            return period > ETS_MAX_PERIOD ? ETS_MAX_PERIOD + 1 : (period > 1 ? period : 1);
        default: return period;
        }
    };
    std::map<int, std::vector<size_t>> groups;
    bool uniform = true;
    for (size_t s = 1; s < n; s++) if (used_period(b->h_period[s]) != used_period(b->h_period[0])) { uniform = false; break; }
    if (b->d_m_col) run_group(b, b->merged_m_max, b->d_len, st);        // several periods, one run: the kernels read the period per column
    else if (uniform) run_group(b, n ? used_period(b->h_period[0]) : 1, b->d_len, st);
    else {
        for (size_t s = 0; s < n; s++) groups[used_period(b->h_period[s])].push_back(s);
        std::vector<int32_t> eff(ld);
        for (auto &g : groups) {
            std::fill(eff.begin(), eff.end(), 0);
            for (size_t s : g.second) if (b->h_base_status[s] == 0) eff[s] = b->h_len[s];
            HIPCHECK(hipStreamSynchronize(st));   // d_len_group is reused between groups
            HIPCHECK(hipMemcpy(b->d_len_group, eff.data(), ld * sizeof(int32_t), hipMemcpyHostToDevice));
            run_group(b, g.first, b->d_len_group, st);
        }
    }
    IntervalArgs ia{};
    ia.n_series = (int)n; ia.h = b->h; ia.yhat = b->d_yhat; ia.sd = b->d_sd; ia.status = b->d_status; ia.z = b->plan.z;
    ia.lower = b->d_lo; ia.upper = b->d_hi;
    launch_intervals(ia, st);
    LAUNCHCHECK("intervals");
    HIPCHECK(hipEventRecord(b->ev_stop, st));
    b->last_stream = st;
    b->ran = true;
    b->quiesced = false;
}

std::string series_error_message(const AnofoxHipBatch *b, size_t s, int code, int detail)
{
    char buf[512];
    if (code == INTERNAL_ERROR) return "Internal error: the device never computed this series (kernel did not run)";
    if (code == INSUFFICIENT_DATA) {
        int got = b->h_len[s];
        std::snprintf(buf, sizeof buf, "Insufficient data: need at least %d observations, got %d", got == 0 ? 1 : 3, got);
        return buf;
    }
    const char *why = detail == FIT_SHORT ? "not enough observations for this model"
                      : detail == FIT_NONPOSITIVE ? "multiplicative components require strictly positive data"
                      : detail == FIT_NONFINITE ? "likelihood is not finite"
                      : "unsupported seasonal period (periods above 2048 are not supported)";
    switch (b->plan.model) {
    case M_ETS:
        if (b->plan.ets_spec_id >= 0) {
            std::snprintf(buf, sizeof buf, "Computation error: ETS model '%s' failed to fit: Computation error: Failed to fit ETS model: %s",
                          b->plan.ets_notation.c_str(), why);
            return buf;
        }
        // fallthrough
    default:
        std::snprintf(buf, sizeof buf, "Computation error: %s fit failed: %s", model_name(b->plan.model), why);
        return buf;
    }
}

void fitted_values_host(const double *y, size_t n, ModelType model, size_t period, double *f)
{
    // forecast.rs:2593-2643
    if (model == M_Naive) {
        f[0] = y[0];
        for (size_t i = 1; i < n; i++) f[i] = y[i - 1];
    } else if (model == M_SeasonalNaive) {
        size_t p = std::min(std::max<size_t>(period, 1), n);
        for (size_t i = 0; i < p; i++) f[i] = y[0];
        for (size_t i = p; i < n; i++) f[i] = y[i - p];
    } else if (model == M_SeasonalWindowAverage) {
        // the running mean of the earlier values at the same phase (the value itself where there is none yet)
        size_t p = std::min(std::max<size_t>(period, 1), n);
        std::vector<double> sum(p, 0.0);
        std::vector<size_t> cnt(p, 0);
        for (size_t i = 0; i < n; i++) {
            const size_t pos = i % p;
            f[i] = cnt[pos] > 0 ? sum[pos] / (double)cnt[pos] : y[i];
            sum[pos] += y[i];
            cnt[pos]++;
        }
    } else {
        double level = y[0];
        f[0] = level;
        for (size_t i = 1; i < n; i++) { f[i] = level; level = 0.3 * y[i] + (1.0 - 0.3) * level; }
    }
}

// The candidate specs of a batch run on at most four concurrent streams (launch_fit_slots, group schedule): ROCm's default of
// GPU_MAX_HW_QUEUES=4 hardware queues is enough.  The library does NOT touch the process environment (Environment).
bool device_ready(AnofoxError *err)
{
    int cnt = 0;
    hipError_t e = hipGetDeviceCount(&cnt);
    if (e != hipSuccess || cnt <= 0) {
        set_error(err, INTERNAL_ERROR, "Internal error: no HIP device available (the MI355X backend has no CPU fallback)");
        return false;
    }
    return true;
}

// Route A (the shipped macro) calls anofox_ts_forecast once per group from every DuckDB worker thread
// (ts_forecast_scalar.cpp:298-523).  Creating a device batch costs ~30 ms of allocator / stream calls that serialise across
// threads -- far more than a single-series fit -- so idle single-series batches are kept in a small process-wide pool, keyed
// by the option block and the device: a call takes a matching batch (or creates one with room for 2x its length), re-packs
// it, runs, fetches and gives it back.  Entries are never destroyed at process exit (the HIP runtime may be gone by then).
struct PooledBatch { ForecastOptions opt; int device; AnofoxHipBatch *b; };
std::mutex g_pool_mu;
std::vector<PooledBatch> g_pool;
constexpr size_t POOL_MAX_IDLE = 32;

AnofoxHipBatch *pool_take(const ForecastOptions &o, size_t length, int device)
{
    std::lock_guard<std::mutex> lock(g_pool_mu);
    for (size_t i = 0; i < g_pool.size(); i++)
        if (g_pool[i].device == device && g_pool[i].b->t_max >= length && std::memcmp(&g_pool[i].opt, &o, sizeof o) == 0) {
            AnofoxHipBatch *b = g_pool[i].b;
            g_pool.erase(g_pool.begin() + (long)i);
            return b;                                   // (the caller attaches a stream set again)
        }
    return nullptr;
}

void pool_give(const ForecastOptions &o, int device, AnofoxHipBatch *b)
{
    // a parked batch keeps its device blocks but not its 33 streams: an early single-series call would otherwise sit on the
    // process's first (favourably mapped, high-priority) stream set for as long as it stays in the pool
    batch_detach_streams(b);
    AnofoxHipBatch *evict = nullptr;
    {
        std::lock_guard<std::mutex> lock(g_pool_mu);
        if (g_pool.size() >= POOL_MAX_IDLE) { evict = g_pool.front().b; g_pool.erase(g_pool.begin()); }
        g_pool.push_back(PooledBatch{o, device, b});
    }
    if (evict) anofox_hip_batch_destroy(evict);
}

void pool_drain(std::vector<AnofoxHipBatch *> &out)
{
    std::lock_guard<std::mutex> lock(g_pool_mu);
    for (auto &e : g_pool) out.push_back(e.b);
    g_pool.clear();
}

} // namespace

// =============================================================================================
// C ABI
// =============================================================================================
extern "C" {

const char *anofox_fcst_version(void) { return "0.1.0-hip-gfx950"; }

int anofox_hip_device_count(void)
{
    int cnt = 0;
    if (hipGetDeviceCount(&cnt) != hipSuccess) return -1;
    return cnt;
}

int anofox_hip_set_device(int device) { return hipSetDevice(device) == hipSuccess ? 0 : -1; }

void anofox_hip_release_caches(void)
{
    // parked single-series batches first (their blocks go back to the caches), then the caches themselves
    std::vector<AnofoxHipBatch *> parked;
    pool_drain(parked);
    for (AnofoxHipBatch *b : parked) anofox_hip_batch_destroy(b);
    dev_cache_release_all();
    pin_cache_release_all();
    stream_pool_release_all();
}

bool anofox_hip_set_default_arima_method(int method)
{
    if (method != ANOFOX_ARIMA_CSS && method != ANOFOX_ARIMA_CSS_ML) return false;
    g_default_arima_method.store(method);
    return true;
}

bool anofox_hip_batch_set_arima_method(AnofoxHipBatch *b, int method, AnofoxError *out_error)
{
    clear_error(out_error);
    if (!b) { set_error(out_error, NULL_POINTER, "Null pointer argument"); return false; }
    if (method != ANOFOX_ARIMA_CSS && method != ANOFOX_ARIMA_CSS_ML) {
        set_error(out_error, INVALID_INPUT, "Invalid input: unknown ARIMA estimation method (0 = CSS, 1 = CSS-ML)");
        return false;
    }
    b->arima_method = method;
    return true;
}

bool anofox_hip_batch_create(size_t n_series, size_t t_max, const ForecastOptions *options, AnofoxHipBatch **out_batch,
                             AnofoxError *out_error)
{
    clear_error(out_error);
    if (!options || !out_batch) { set_error(out_error, NULL_POINTER, "Null pointer argument"); return false; }
    Plan plan;
    if (!make_plan(options, plan, out_error)) return false;
    if (!device_ready(out_error)) return false;
    AnofoxHipBatch *b = new AnofoxHipBatch();
    try {
        HIPCHECK(hipGetDevice(&b->dev));
        b->n = n_series;
        b->t_max = t_max;
        b->ld = (n_series + 63) / 64 * 64;
        if (b->ld == 0) b->ld = 64;
        // the streamed loads address a block of <= 32 rows with 32-bit offsets (buffer loads): 33 rows must stay under 4 GiB
        if ((double)b->ld * 8.0 * 33.0 >= 4294967296.0) throw HipFail{"batch too wide for one launch (more than ~16 million series): shard it"};
        b->h = options->horizon;
        b->opt = *options;
        b->plan = plan;
        b->tun = Tunables::from_env();
        if (b->tun.seq_rounds >= 0) { b->seq_rounds_env = b->tun.seq_rounds; b->seq_rounds = b->seq_rounds_env; }
        // dense re-gather of the running problems between rounds (up to 2x on a large batch) costs one block copy per
        // candidate spec (sized below)
        {
            // one block per candidate spec THAT HAS ANYTHING TO FIT, allocated by the first run that needs it (launch_fit_slots): together
            // at most 55 % of the device (158 GB of the MI355X's 288).  The 1M x 1,024 stress configuration on ONE GPU: 6 admissible specs
            // on intermittent counts -> six full blocks of 8.2 GB; with all 25 specs live, blocks of 772k of the 1M columns (1.34 s per
            // step against 2.75 s without any gather, which is what the old all-or-nothing 96 GiB rule gave)
            size_t free_b = 0, total_b = 0;
            b->gather_budget = hipMemGetInfo(&free_b, &total_b) == hipSuccess ? std::max(96.0 * 1073741824.0, 0.55 * (double)total_b) : 96.0 * 1073741824.0;
            b->use_gather = true;
        }
        if (b->tun.gather >= 0) b->use_gather = b->tun.gather != 0;
        b->spec_below = b->tun.spec_below; b->spec_below_md = b->tun.spec_below_md;
        b->spec2_below = b->tun.spec2_below; b->spec2_below_md = b->tun.spec2_below_md;
        b->arima_method = arima_method_in_force();
        alloc_common(b);
    } catch (const HipFail &f) {
        report_hip_failure(out_error, f);
        free_batch_buffers(b);
        delete b;
        return false;
    } catch (const std::exception &e) {
        set_error(out_error, INTERNAL_ERROR, std::string("Internal error: ") + e.what());
        free_batch_buffers(b);
        delete b;
        return false;
    }
    *out_batch = b;
    return true;
}

void anofox_hip_batch_destroy(AnofoxHipBatch *b)
{
    if (!b) return;
    DeviceGuard guard(b->dev);
    // wait for this batch's own work only (other batches may be running from other host threads)
    const bool timing = b->tun.timing;
    const auto t0 = std::chrono::steady_clock::now();
    // (a wait on an idle stream is not free either: with more streams than hardware queues it queues behind whatever other
    //  batches run on the shared queue -- 200-550 ms per destroy measured beside two running batches -- so a batch whose last run
    //  has been waited for skips them: its auxiliary streams had joined the run's stream before that wait returned)
    if (!b->quiesced) {
        if (b->last_stream) (void)hipStreamSynchronize(b->last_stream);
        if (b->own_stream) (void)hipStreamSynchronize(b->own_stream);
        for (auto &q : b->aux) if (q) (void)hipStreamSynchronize(q);
    }
    const auto t1 = std::chrono::steady_clock::now();
    const size_t n = b->n;
    free_batch_buffers(b);
    delete b;
    if (timing) {
        const auto t2 = std::chrono::steady_clock::now();
        if (std::chrono::duration<double, std::milli>(t2 - t0).count() > 20.0)
            std::fprintf(stderr, "[anofox-hip] destroy of a batch of %zu: stream waits %.1f ms, buffers %.1f ms\n", n,
                         std::chrono::duration<double, std::milli>(t1 - t0).count(), std::chrono::duration<double, std::milli>(t2 - t1).count());
    }
}

size_t anofox_hip_batch_ld(const AnofoxHipBatch *b) { return b ? b->ld : 0; }
size_t anofox_hip_batch_n_series(const AnofoxHipBatch *b) { return b ? b->n : 0; }

bool anofox_hip_batch_periods(const AnofoxHipBatch *b, int32_t *out_periods)
{
    if (!b || !out_periods || !b->has_block || b->h_period.size() < b->n) return false;
    for (size_t s = 0; s < b->n; s++) out_periods[s] = b->h_period[s];
    return true;
}

bool anofox_hip_batch_set_fixed_params(AnofoxHipBatch *b, double alpha, double beta, double gamma, double phi, AnofoxError *out_error)
{
    clear_error(out_error);
    if (!b) { set_error(out_error, NULL_POINTER, "Null pointer argument"); return false; }
    if (!(b->plan.model == M_ETS && b->plan.ets_spec_id >= 0)) {
        set_error(out_error, INVALID_INPUT, "Invalid input: fixed smoothing parameters need model 'ETS' with an explicit ets_model");
        return false;
    }
    const int id = b->plan.ets_spec_id;
    const bool has_trend = spec_trend_idx(id) != 0, has_season = spec_season(id) != 0;
    const bool damped = spec_trend_idx(id) == 2 || spec_trend_idx(id) == 4;
    // the model's own parameters: 0 < alpha < 1, 0 <= beta <= alpha, 0 <= gamma <= 1 - alpha, 0 < phi <= 1
    bool ok = alpha > 0.0 && alpha < 1.0;
    if (has_trend) ok = ok && beta >= 0.0 && beta <= alpha;
    if (has_season) ok = ok && gamma >= 0.0 && gamma <= 1.0 - alpha;
    if (damped) ok = ok && phi > 0.0 && phi <= 1.0;
    if (!ok) {
        set_error(out_error, INVALID_INPUT,
                  "Invalid input: smoothing parameters out of range (0 < alpha < 1, 0 <= beta <= alpha, 0 <= gamma <= 1 - alpha, 0 < phi <= 1)");
        return false;
    }
    // optimiser coordinates of the recursion (ets_device.hpp ets_unpack): beta = alpha beta*, gamma = gamma* (1 - alpha)
    b->fixed_x[0] = alpha;
    b->fixed_x[1] = has_trend ? beta / alpha : 0.0;
    b->fixed_x[2] = has_season ? gamma / (1.0 - alpha) : 0.0;
    b->fixed_x[3] = damped ? phi : 1.0;
    b->fixed_params = true;
    return true;
}

bool anofox_hip_batch_pack_host(AnofoxHipBatch *b, const double *const *values, const uint64_t *const *validity,
                                const size_t *lengths, AnofoxError *out_error)
{
    if (!b || !values || !lengths) { set_error(out_error, NULL_POINTER, "Null pointer argument"); return false; }
    DeviceGuard guard(b->dev);
    try {
        const size_t n = b->n, ld = b->ld, T = std::max<size_t>(b->t_max, 1);
        for (size_t s = 0; s < n; s++)
            if (lengths[s] > b->t_max) throw HipFail{"series longer than the plan's t_max"};
        // The packer is the host half of the batch entry and easily costs more than the fit: it runs on all host threads, 64 series
        // (one 512-byte row segment of the time-major block) per tile, into pinned staging.  The block goes over in column chunks
        // of ~512 MB through TWO staging buffers (kept by the batch): while one chunk is copied -- a pitched copy into its columns of
        // the device block, on the batch's own stream (the legacy default stream of a synchronous hipMemcpy is shared by every host
        // thread of the process) -- the packer threads fill the other, and no staging block of the size of the batch is ever pinned
        // (8.2 GB for the 1M x 1,024 configuration).
        constexpr size_t TILE = 64;
        const size_t n_tiles = ld / TILE;
        // (512 MB chunks: the M5 block -- 467 MB -- stays one contiguous copy, which measured faster than four pitched ones: 13 against 20 ms)
        const size_t chunk_tiles = std::min(n_tiles, std::max<size_t>(1, (size_t)(536870912.0 / (8.0 * (double)T)) / TILE));
        const size_t chunk_cols = chunk_tiles * TILE;
        const size_t n_chunks = (n_tiles + chunk_tiles - 1) / chunk_tiles;
        const size_t n_bufs = n_chunks > 1 ? 2 : 1;
        const auto tp0 = std::chrono::steady_clock::now();
        double fill_ms = 0.0;
        if (b->h_stage_elems < n_bufs * T * chunk_cols) {
            pin_free(b->h_stage);
            b->h_stage = nullptr; b->h_stage_elems = 0;
            b->h_stage = (double *)pin_alloc_bytes(n_bufs * T * chunk_cols * sizeof(double));
            b->h_stage_elems = n_bufs * T * chunk_cols;
        }
        b->h_len.assign(n, 0);
        b->h_period.assign(n, 1);
        const bool keep = b->opt.include_fitted || b->opt.include_residuals;
        if (keep) {
            b->h_clean_off.assign(n + 1, 0);
            for (size_t s = 0; s < n; s++) b->h_clean_off[s + 1] = b->h_clean_off[s] + lengths[s];
            b->h_clean.assign(b->h_clean_off[n], 0.0);
        }
        const bool detect = b->opt.auto_detect_seasonality && b->opt.seasonal_period == 0;
        // tiles [tile0, tile1) of the chunk that starts at tile `base` -> stage (row stride `cols` doubles)
        auto do_tiles = [&](double *stage, size_t cols, size_t base, size_t tile0, size_t tile1) {
            std::vector<double> clean(TILE * T);
            for (size_t tile = tile0; tile < tile1; tile++) {
                const size_t s0 = tile * TILE;
                size_t len_of[TILE];
                for (size_t j = 0; j < TILE; j++) {
                    const size_t s = s0 + j;
                    const size_t len = s < n ? lengths[s] : 0;
                    len_of[j] = len;
                    double *c = clean.data() + j * T;
                    if (len) fill_nulls_interpolate(values[s], validity ? validity[s] : nullptr, len, c);
                    if (s < n) {
                        b->h_len[s] = (int32_t)len;
                        b->h_period[s] = (!detect && b->opt.seasonal_period > 0) ? b->opt.seasonal_period : 1;      // (detected periods: below, on the device)
                        if (keep && len) std::memcpy(b->h_clean.data() + b->h_clean_off[s], c, len * sizeof(double));
                    }
                }
                for (size_t t = 0; t < T; t++) {
                    double *row = stage + t * cols + (tile - base) * TILE;
                    for (size_t j = 0; j < TILE; j++) row[j] = t < len_of[j] ? clean[j * T + t] : 0.0;
                }
            }
        };
        const auto tp1 = std::chrono::steady_clock::now();
        unsigned n_thr = std::thread::hardware_concurrency();
        if (tl_host_thread_share > 1) n_thr = std::max(1u, n_thr / tl_host_thread_share);     // one of several device shards packing side by side
        if (b->tun.pack_threads > 0) n_thr = (unsigned)b->tun.pack_threads;
        n_thr = std::max(1u, std::min(n_thr, 32u));
        if (!b->d_y || !b->owns_y) { b->d_y = dalloc<double>(T * ld); b->owns_y = true; }
        batch_attach_streams(b);
        hipEvent_t copied[2] = {nullptr, nullptr};
        struct EvGuard { hipEvent_t (&e)[2]; ~EvGuard() { for (auto x : e) if (x) (void)hipEventDestroy(x); } } ev_guard{copied};
        for (size_t k = 0; k < n_bufs; k++) HIPCHECK(hipEventCreateWithFlags(&copied[k], hipEventDisableTiming));
        try {
            for (size_t ck = 0; ck < n_chunks; ck++) {
                const size_t base = ck * chunk_tiles, tiles = std::min(chunk_tiles, n_tiles - base), cols = tiles * TILE;
                double *stage = b->h_stage + (ck % n_bufs) * T * chunk_cols;
                if (ck >= n_bufs) HIPCHECK(hipEventSynchronize(copied[ck % n_bufs]));       // the copy that last read this buffer
                const unsigned thr = (unsigned)std::min<size_t>(n_thr, tiles);
                const auto tf0 = std::chrono::steady_clock::now();
                if (thr <= 1 || tiles < 8) do_tiles(stage, cols, base, base, base + tiles);
                else {
                    std::vector<std::string> fails(thr);
                    parallel_shares(thr, [&](unsigned k) {
                        try { do_tiles(stage, cols, base, base + tiles * k / thr, base + tiles * (k + 1) / thr); }
                        catch (const std::exception &e) { try { fails[k] = e.what(); } catch (...) { fails[k].assign(1, '?'); } }
                        catch (...) { try { fails[k] = "packer thread failed"; } catch (...) { fails[k].assign(1, '?'); } }
                    });
                    for (auto &f : fails) if (!f.empty()) throw HipFail{f};
                }
                fill_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tf0).count();
                HIPCHECK(hipMemcpy2DAsync(b->d_y + base * TILE, ld * sizeof(double), stage, cols * sizeof(double), cols * sizeof(double), T,
                                          hipMemcpyHostToDevice, b->own_stream));
                HIPCHECK(hipEventRecord(copied[ck % n_bufs], b->own_stream));
            }
            HIPCHECK(hipStreamSynchronize(b->own_stream));
        } catch (...) { (void)hipStreamSynchronize(b->own_stream); throw; }       // nothing may still read the staging buffers
        if (b->tun.timing) {
            const auto tp2 = std::chrono::steady_clock::now();
            std::fprintf(stderr, "[anofox-hip] pack of %zu columns: staging + bookkeeping %.1f ms, %u threads filled %zu tiles in %.1f ms, device block + copies %.1f ms\n", ld,
                         std::chrono::duration<double, std::milli>(tp1 - tp0).count(), n_thr, n_tiles, fill_ms,
                         std::chrono::duration<double, std::milli>(tp2 - tp1).count() - fill_ms);
        }
        finalize_lengths(b);
        if (detect) batch_detect_periods(b);
        b->has_block = true;
    } catch (const HipFail &f) {
        report_hip_failure(out_error, f);
        return false;
    } catch (const std::exception &e) {
        set_error(out_error, INTERNAL_ERROR, std::string("Internal error: ") + e.what());
        return false;
    }
    return true;
}

bool anofox_hip_batch_set_device_block(AnofoxHipBatch *b, const void *d_y, size_t ld, const void *d_len, AnofoxError *out_error)
{
    if (!b || !d_y || !d_len) { set_error(out_error, NULL_POINTER, "Null pointer argument"); return false; }
    if (ld != b->ld) { set_error(out_error, INVALID_INPUT, "Invalid input: leading dimension must equal anofox_hip_batch_ld()"); return false; }
    DeviceGuard guard(b->dev);
    try {
        if (b->owns_y && b->d_y) { dev_free(b->d_y); }
        b->d_y = (double *)d_y;
        b->owns_y = false;
        b->h_len.assign(b->n, 0);
        HIPCHECK(hipMemcpy(b->h_len.data(), d_len, b->n * sizeof(int32_t), hipMemcpyDeviceToHost));
        b->h_period.assign(b->n, b->opt.seasonal_period > 0 ? b->opt.seasonal_period : 1);
        finalize_lengths(b);
        if (b->opt.auto_detect_seasonality && b->opt.seasonal_period == 0) {
            // the block holds no NULLs: nothing to interpolate.  The scan runs now, on the batch's own stream: whatever stream the
            // caller filled the block on must have finished (the run itself is ordered by the stream the caller passes to it)
            HIPCHECK(hipDeviceSynchronize());
            batch_detect_periods(b);
        }
        b->has_block = true;
    } catch (const HipFail &f) {
        report_hip_failure(out_error, f);
        return false;
    } catch (const std::exception &e) {
        set_error(out_error, INTERNAL_ERROR, std::string("Internal error: ") + e.what());
        return false;
    }
    return true;
}

bool anofox_hip_batch_run(AnofoxHipBatch *b, void *stream, AnofoxError *out_error)
{
    if (!b) { set_error(out_error, NULL_POINTER, "Null pointer argument"); return false; }
    if (!b->has_block) { set_error(out_error, INVALID_INPUT, "Invalid input: batch has no series block"); return false; }
    DeviceGuard guard(b->dev);
    try {
        run_batch(b, stream ? (hipStream_t)stream : b->own_stream);
    } catch (const HipFail &f) {
        report_hip_failure(out_error, f);
        return false;
    } catch (const std::exception &e) {
        set_error(out_error, INTERNAL_ERROR, std::string("Internal error: ") + e.what());
        return false;
    }
    return true;
}

bool anofox_hip_batch_stats(AnofoxHipBatch *b, AnofoxHipStats *out)
{
    if (!b || !out || !b->ran) return false;
    DeviceGuard guard(b->dev);
    std::memset(out, 0, sizeof *out);
    if (hipEventSynchronize(b->ev_stop) != hipSuccess) return false;
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, b->ev_start, b->ev_stop) == hipSuccess) out->total_device_ms = ms;
    if (b->timed_fit && hipEventElapsedTime(&ms, b->ev_fit0, b->ev_fit1) == hipSuccess) out->fit_kernel_ms = ms;
    std::vector<int32_t> passes(b->n), evals(b->n);
    if (hipMemcpy(passes.data(), b->d_passes_total, b->n * sizeof(int32_t), hipMemcpyDeviceToHost) != hipSuccess) return false;
    if (hipMemcpy(evals.data(), b->d_evals_total, b->n * sizeof(int32_t), hipMemcpyDeviceToHost) != hipSuccess) return false;
    out->n_series = b->n;
    out->t_max = b->t_max;
    out->n_problems = b->n_problems;
    out->fit_kernel_launches = b->fit_launches;
    out->y_storage = (uint32_t)(b->insp_ok ? b->y_type : 0);
    for (size_t s = 0; s < b->n; s++) {
        uint64_t p = (uint64_t)std::max(passes[s], 0);
        out->total_passes += p;
        out->max_passes = std::max<uint64_t>(out->max_passes, p);
        out->total_evals += (uint64_t)std::max(evals[s], 0);
        out->algorithmic_bytes += 8ull * (uint64_t)b->h_len[s] * p + 24ull * (uint64_t)std::max(b->h, 0);
    }
    // the one-pass-per-iteration count of the same run (the spec slots of the last fit: iterations per problem, + 1 final pass each)
    if (b->insp_ok && b->d_iters_slots && b->d_status_slots && !b->fixed_params) {
        const size_t n_used = b->insp_spec.size(), ld = b->ld;
        std::vector<int32_t> it(n_used * ld), stt(n_used * ld);
        if (hipMemcpy(it.data(), b->d_iters_slots, it.size() * sizeof(int32_t), hipMemcpyDeviceToHost) != hipSuccess) return false;
        if (hipMemcpy(stt.data(), b->d_status_slots, stt.size() * sizeof(int32_t), hipMemcpyDeviceToHost) != hipSuccess) return false;
        for (size_t s = 0; s < b->n; s++) {
            uint64_t q = 0;
            for (size_t k = 0; k < n_used; k++)
                if (stt[k * ld + s] == anofox::FIT_OK) q += (uint64_t)std::max(it[k * ld + s], 0) + 1;
            out->total_iters += q;
            out->min_pass_bytes += 8ull * (uint64_t)b->h_len[s] * q + 24ull * (uint64_t)std::max(b->h, 0);
        }
    }
    return true;
}

bool anofox_hip_selftest_recip(uint64_t n_operands, uint64_t seed, uint64_t *out_mismatches, double *out_first_bad)
{
    if (!out_mismatches) return false;
    AnofoxError err;
    if (!device_ready(&err)) return false;
    double fb = 0.0;
    const unsigned long long r = anofox::recip_selftest(n_operands, seed, &fb, nullptr);
    if (r == ~0ull) return false;
    *out_mismatches = r;
    if (out_first_bad) *out_first_bad = fb;
    return true;
}

bool anofox_hip_selftest_math(int fn, const double *x, const double *y, uint64_t n, int block_threads, double *out, double *out2, AnofoxError *err)
{
    static_assert(anofox::NM_BLOCK == 64, "the header names 64 as the fit kernels' workgroup size");
    if (fn < 0 || fn >= ANOFOX_HIP_MATH_FN_COUNT) { set_error(err, INVALID_INPUT, "Invalid input: fn is not an AnofoxHipMathFn"); return false; }
    if (block_threads != anofox::NM_BLOCK && block_threads != 256) { set_error(err, INVALID_INPUT, "Invalid input: block_threads must be 64 or 256"); return false; }
    if (n > ((uint64_t)1 << 28)) { set_error(err, INVALID_INPUT, "Invalid input: more than 2^28 operands"); return false; }
    const bool needs_y = fn == ANOFOX_HIP_MATH_SCALBN || fn == ANOFOX_HIP_MATH_POW_STEP || fn == ANOFOX_HIP_MATH_POW_NEAR1 || fn == ANOFOX_HIP_MATH_POW_POS;
    if (n > 0 && (!x || !out || (needs_y && !y) || (fn == ANOFOX_HIP_MATH_SINCOS && !out2))) { set_error(err, NULL_POINTER, "Null pointer argument"); return false; }
    if (!device_ready(err)) return false;
    if (!anofox::math_selftest(fn, x, needs_y ? y : nullptr, n, block_threads, out, out2, nullptr)) {
        set_error(err, INTERNAL_ERROR, "Internal error: the device could not run the math self test");
        return false;
    }
    return true;
}

bool anofox_hip_batch_lane_stats(AnofoxHipBatch *b, AnofoxHipLaneStats *out, size_t struct_size)
{
    if (!b || !out || !b->ran || struct_size < sizeof(uint64_t)) return false;
    DeviceGuard guard(b->dev);
    AnofoxHipLaneStats r;
    std::memset(&r, 0, sizeof r);
    r.struct_size = sizeof r;
    if (hipEventSynchronize(b->ev_stop) != hipSuccess) return false;
    if (b->d_wave_trace && !b->tun.wave_trace.empty()) {
        unsigned long long head[4] = {0, 0, 0, 0};
        if (hipMemcpy(head, b->d_wave_trace, sizeof head, hipMemcpyDeviceToHost) != hipSuccess) return false;
        const size_t used = (size_t)std::min(head[0], head[1]);
        std::vector<unsigned long long> rec(4 * used);
        if (used && hipMemcpy(rec.data(), b->d_wave_trace + 4, rec.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost) != hipSuccess) return false;
        if (FILE *f = std::fopen(b->tun.wave_trace.c_str(), "wb")) {
            std::fwrite(head, sizeof head, 1, f);
            if (used) std::fwrite(rec.data(), sizeof(unsigned long long), rec.size(), f);
            std::fclose(f);
        }
    }
    if (b->insp_ok && b->d_lane_stats && !b->fixed_params) {
        std::vector<unsigned long long> c(2 * (size_t)b->n_slots_cap);
        if (hipMemcpy(c.data(), b->d_lane_stats, c.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost) != hipSuccess) return false;
        // insp_spec[oi] = spec id in launch order; the counters are indexed by the slot k the spec was given (order[oi] = k): rebuild k
        // from h_slot_spec (slot -> spec id)
        for (size_t k = 0; k < b->h_slot_spec.size() && k < (size_t)b->n_slots_cap; k++) {
            const int id = b->h_slot_spec[k];
            const int cls = !spec_has_mult(id) ? 0 : (spec_trend_idx(id) == 4 ? 2 : 1);
            r.wave_passes[cls] += c[2 * k];
            r.live_lane_passes[cls] += c[2 * k + 1];
            if (k < 30) { r.slot_spec_id[k] = id; r.slot_wave_passes[k] = c[2 * k]; r.slot_live_lane_passes[k] = c[2 * k + 1]; r.n_slots = (uint32_t)(k + 1); }
        }
    }
    // the caller's struct may be older (smaller) or newer (larger) than this library's: copy what both know, report what was written
    const size_t nbytes = std::min(struct_size, sizeof r);
    r.struct_size = nbytes;
    std::memcpy(out, &r, nbytes);
    return true;
}

bool anofox_hip_batch_device_results(AnofoxHipBatch *b, void **d_yhat, void **d_lower, void **d_upper, void **d_model_code,
                                     void **d_status)
{
    if (!b) return false;
    if (d_yhat) *d_yhat = b->d_yhat;
    if (d_lower) *d_lower = b->d_lo;
    if (d_upper) *d_upper = b->d_hi;
    if (d_model_code) *d_model_code = b->d_model_code;
    if (d_status) *d_status = b->d_status;
    return true;
}

void anofox_hip_model_name(const ForecastOptions *options, int32_t model_code, char out_name[64])
{
    out_name[0] = 0;
    if (model_code >= 1000000) { auto_arima_name(model_code, options ? options->seasonal_period : 1, out_name); return; }
    if (model_code >= 100 && model_code < 130) { auto_ets_name(model_code - 100, out_name); return; }
    if (model_code == MODEL_CODE_ARIMAX) { std::snprintf(out_name, 64, "ARIMAX"); return; }
    Plan p;
    AnofoxError e;
    if (options && make_plan(options, p, &e)) {
        std::snprintf(out_name, 64, "%s", p.static_name.c_str());
    }
}

void anofox_hip_batch_model_name(const AnofoxHipBatch *b, size_t series, int32_t model_code, char out_name[64])
{
    out_name[0] = 0;
    if (!b) return;
    // the period the series was fitted with (given, or detected on the resident block): what anofox_hip_batch_fetch names it with
    if (model_code >= 1000000) {
        const int period = (series < b->h_period.size()) ? b->h_period[series] : (b->opt.seasonal_period > 0 ? b->opt.seasonal_period : 1);
        auto_arima_name(model_code, period, out_name);
        return;
    }
    anofox_hip_model_name(&b->opt, model_code, out_name);
}

bool anofox_hip_batch_fetch(AnofoxHipBatch *b, ForecastResult *out_results, AnofoxError *out_errors)
{
    if (!b || !out_results || !b->ran) return false;
    DeviceGuard guard(b->dev);
    const size_t n = b->n, h = (size_t)std::max(b->h, 0);
    if (hipStreamSynchronize(b->last_stream) != hipSuccess) return false;
    b->quiesced = true;
    // results come back through ONE pinned block (a copy into pageable memory is staged by the runtime at a fraction of the link
    // speed: 672 MB of forecasts for 1M series), on the stream of the run
    const size_t nh = n * h;
    struct PinBlock { void *p = nullptr; ~PinBlock() { pin_free(p); } } pin;
    try { pin.p = pin_alloc_bytes(std::max<size_t>(3 * nh * sizeof(double) + 3 * n * sizeof(int32_t), 64)); }
    catch (...) { return false; }
    double *const yhat = (double *)pin.p, *const lo = yhat + nh, *const hi = lo + nh;
    int32_t *const status = (int32_t *)(hi + nh), *const code = status + n, *const detail = code + n;
    bool ok = true;
    hipStream_t cs = b->last_stream;
    if (nh) {
        ok &= hipMemcpyAsync(yhat, b->d_yhat, nh * sizeof(double), hipMemcpyDeviceToHost, cs) == hipSuccess;
        ok &= hipMemcpyAsync(lo, b->d_lo, nh * sizeof(double), hipMemcpyDeviceToHost, cs) == hipSuccess;
        ok &= hipMemcpyAsync(hi, b->d_hi, nh * sizeof(double), hipMemcpyDeviceToHost, cs) == hipSuccess;
    }
    ok &= hipMemcpyAsync(status, b->d_status, n * sizeof(int32_t), hipMemcpyDeviceToHost, cs) == hipSuccess;
    ok &= hipMemcpyAsync(code, b->d_model_code, n * sizeof(int32_t), hipMemcpyDeviceToHost, cs) == hipSuccess;
    ok &= hipMemcpyAsync(detail, b->d_detail, n * sizeof(int32_t), hipMemcpyDeviceToHost, cs) == hipSuccess;
    ok &= hipStreamSynchronize(cs) == hipSuccess;
    if (!ok) return false;
    // the per-series result records (three allocations each, the reference's ownership contract): on several host threads for a large
    // batch -- 1M series spent 0.47 s here on one
    auto do_range = [&](size_t s_lo, size_t s_hi) {
    for (size_t s = s_lo; s < s_hi; s++) {
        ForecastResult &r = out_results[s];
        std::memset(&r, 0, sizeof r);
        if (out_errors) clear_error(&out_errors[s]);
        if (status[s] == STATUS_NOT_COMPUTED) status[s] = INTERNAL_ERROR;
        if (status[s] != 0) {
            if (out_errors) set_error(&out_errors[s], status[s], series_error_message(b, s, status[s], detail[s]));
            continue;
        }
        r.n_forecasts = h;
        if (h) {
            r.point_forecasts = (double *)std::malloc(h * sizeof(double));
            r.lower_bounds = (double *)std::malloc(h * sizeof(double));
            r.upper_bounds = (double *)std::malloc(h * sizeof(double));
            if (!r.point_forecasts || !r.lower_bounds || !r.upper_bounds) {
                std::free(r.point_forecasts); std::free(r.lower_bounds); std::free(r.upper_bounds);
                std::memset(&r, 0, sizeof r);
                if (out_errors) set_error(&out_errors[s], ALLOCATION_ERROR, "Failed to allocate point forecasts");
                continue;
            }
            std::memcpy(r.point_forecasts, &yhat[s * h], h * sizeof(double));
            std::memcpy(r.lower_bounds, &lo[s * h], h * sizeof(double));
            std::memcpy(r.upper_bounds, &hi[s * h], h * sizeof(double));
        }
        if (code[s] >= 1000000) auto_arima_name(code[s], b->h_period[s], r.model_name);
        else if (code[s] >= 100) auto_ets_name(code[s] - 100, r.model_name);
        else if (code[s] == MODEL_CODE_ARIMAX) std::snprintf(r.model_name, 64, "ARIMAX");
        else std::snprintf(r.model_name, 64, "%s", b->plan.static_name.c_str());
        r.aic = std::nan(""); r.bic = std::nan(""); r.mse = std::nan("");
        if ((b->opt.include_fitted || b->opt.include_residuals) && !b->h_clean_off.empty()) {
            const size_t len = (size_t)b->h_len[s];
            const double *y = b->h_clean.data() + b->h_clean_off[s];
            double *f = (double *)std::malloc(len * sizeof(double));
            fitted_values_host(y, len, b->plan.model, (size_t)b->h_period[s], f);
            double sse = 0.0;
            for (size_t i = 0; i < len; i++) { double d = y[i] - f[i]; sse += d * d; }
            r.mse = sse / (double)len;
            if (b->opt.include_residuals) {
                r.residuals = (double *)std::malloc(len * sizeof(double));
                for (size_t i = 0; i < len; i++) r.residuals[i] = y[i] - f[i];
            }
            if (b->opt.include_fitted) { r.fitted_values = f; r.n_fitted = len; }
            else std::free(f);
        }
    }
    };
    unsigned n_thr = (unsigned)std::min<size_t>({(size_t)std::max(1u, std::thread::hardware_concurrency()), 16, n / 8192});
    if (tl_host_thread_share > 1) n_thr = std::max(1u, n_thr / tl_host_thread_share);
    if (n_thr <= 1) do_range(0, n);
    else {
        std::atomic<bool> failed{false};
        parallel_shares(n_thr, [&](unsigned k) { try { do_range(n * k / n_thr, n * (k + 1) / n_thr); } catch (...) { failed = true; } });
        if (failed) return false;
    }
    return true;
}

void anofox_free_forecast_result(ForecastResult *r)
{
    if (r) free_result_arrays(*r);
}

namespace {

// a batch whose fit state the inspection passes can re-read: AutoETS or ETS(spec), run, with its final-kernel arguments kept
bool inspectable_ets(const AnofoxHipBatch *b)
{
    return (b->plan.model == M_AutoETS || (b->plan.model == M_ETS && b->plan.ets_spec_id >= 0)) && b->insp_ok;
}

// The inspection passes of an ETS batch, enqueued on the stream of its last run: d_info [8 x ld], d_states [(2 + max(m, 1)) x ld] and
// d_fit [max(t_max, 1) x ld] (may be null) are filled with NaN, then the final kernel of every spec writes the series it was selected
// for.  Nothing is copied and nothing is waited for.
void inspect_ets_passes(AnofoxHipBatch *b, double *d_info, double *d_states, double *d_fit)
{
    for (size_t s = 1; s < b->n; s++)
        if (b->h_period[s] != b->h_period[0]) throw HipFail{"inspection needs one seasonal period for the whole batch"};
    const size_t ld = b->ld, T = std::max<size_t>(b->t_max, 1), rows = (size_t)(2 + std::max(b->insp_m, 1));
    hipStream_t st = b->last_stream;
    const double nan = std::nan("");
    (void)hipGetLastError();
    if (d_fit) launch_fill_f64(d_fit, T * ld, nan, st);
    launch_fill_f64(d_states, rows * ld, nan, st);
    launch_fill_f64(d_info, 8 * ld, nan, st);
    LAUNCHCHECK("inspection fill");
    for (size_t oi = 0; oi < b->insp_args.size(); oi++) {
        FitArgs a = b->insp_args[oi];
        a.insp_sel = b->d_model_code;
        a.insp_code = b->plan.model == M_AutoETS ? 100 + b->insp_spec[oi] : 0;
        a.insp_fitted = d_fit; a.insp_states = d_states; a.insp_info = d_info;
        b->insp_fns[oi].final(a, st);
    }
}

} // namespace

bool anofox_hip_batch_inspect_device(AnofoxHipBatch *b, double *d_info, double *d_states, double *d_fitted, AnofoxError *out_error)
{
    clear_error(out_error);
    if (!b || !d_info || !d_states) { set_error(out_error, NULL_POINTER, "Null pointer argument"); return false; }
    if (!b->ran) { set_error(out_error, INVALID_INPUT, "Invalid input: the batch has not been run"); return false; }
    if (!inspectable_ets(b)) {
        set_error(out_error, INVALID_INPUT, "Invalid input: the device inspection needs an AutoETS or ETS(spec) batch");
        return false;
    }
    DeviceGuard guard(b->dev);
    try {
        b->quiesced = false;
        inspect_ets_passes(b, d_info, d_states, d_fitted);
        HIPCHECK(hipStreamSynchronize(b->last_stream));
    } catch (const HipFail &f) {
        report_hip_failure(out_error, f);
        return false;
    } catch (const std::exception &e) {
        set_error(out_error, INTERNAL_ERROR, std::string("Internal error: ") + e.what());
        return false;
    }
    return true;
}

bool anofox_hip_batch_inspect(AnofoxHipBatch *b, AnofoxHipInspection *out, double *fitted, double *seasonal, size_t seasonal_stride,
                              AnofoxError *out_error)
{
    if (!b || !out) { set_error(out_error, NULL_POINTER, "Null pointer argument"); return false; }
    if (!b->ran) { set_error(out_error, INVALID_INPUT, "Invalid input: the batch has not been run"); return false; }
    DeviceGuard guard(b->dev);
    const size_t n = b->n, ld = b->ld, T = std::max<size_t>(b->t_max, 1);
    try {
        HIPCHECK(hipStreamSynchronize(b->last_stream));
        b->quiesced = false;             // the inspection passes below run on the auxiliary streams
        std::vector<int32_t> code(n), status(n);
        HIPCHECK(hipMemcpy(code.data(), b->d_model_code, n * sizeof(int32_t), hipMemcpyDeviceToHost));
        HIPCHECK(hipMemcpy(status.data(), b->d_status, n * sizeof(int32_t), hipMemcpyDeviceToHost));
        for (size_t s = 0; s < n; s++) {
            AnofoxHipInspection &o = out[s];
            o.model_code = code[s]; o.status = status[s]; o.seasonal_period = b->h_period.empty() ? 1 : b->h_period[s];
            o.alpha = o.beta = o.gamma = o.phi = o.aic = o.aicc = o.bic = o.sse = o.level = o.trend = std::nan("");
        }
        if (fitted) for (size_t i = 0; i < n * T; i++) fitted[i] = std::nan("");
        if (inspectable_ets(b)) {
            const int m = b->insp_m;
            const size_t rows = (size_t)(2 + std::max(m, 1));
            Scratch scratch;
            double *d_fit = fitted ? scratch.get<double>(T * ld) : nullptr, *d_states = scratch.get<double>(rows * ld), *d_info = scratch.get<double>(8 * ld);
            inspect_ets_passes(b, d_info, d_states, d_fit);
            HIPCHECK(hipStreamSynchronize(b->last_stream));
            scratch.settled();
            std::vector<double> info(8 * ld), states(rows * ld), fit;
            HIPCHECK(hipMemcpy(info.data(), d_info, 8 * ld * sizeof(double), hipMemcpyDeviceToHost));
            HIPCHECK(hipMemcpy(states.data(), d_states, rows * ld * sizeof(double), hipMemcpyDeviceToHost));
            if (fitted) { fit.resize(T * ld); HIPCHECK(hipMemcpy(fit.data(), d_fit, T * ld * sizeof(double), hipMemcpyDeviceToHost)); }
            for (size_t s = 0; s < n; s++) {
                AnofoxHipInspection &o = out[s];
                o.alpha = info[0 * ld + s]; o.beta = info[1 * ld + s]; o.gamma = info[2 * ld + s]; o.phi = info[3 * ld + s];
                o.aic = info[4 * ld + s]; o.aicc = info[5 * ld + s]; o.bic = info[6 * ld + s]; o.sse = info[7 * ld + s];
                o.level = states[0 * ld + s]; o.trend = states[1 * ld + s];
                if (seasonal) for (int j = 0; j < m && (size_t)j < seasonal_stride; j++) seasonal[s * seasonal_stride + j] = states[(size_t)(2 + j) * ld + s];
                if (fitted) { const size_t len = (size_t)std::max(b->h_len[s], 0); for (size_t t = 0; t < len; t++) fitted[s * T + t] = fit[t * ld + s]; }
            }
        } else if (b->plan.model == M_AutoARIMA) {
            std::vector<double> aicc(n);
            std::vector<int32_t> ord(5 * ld), wlen(n);
            HIPCHECK(hipMemcpy(aicc.data(), b->ar_aicc, n * sizeof(double), hipMemcpyDeviceToHost));
            HIPCHECK(hipMemcpy(ord.data(), b->ar_order, 5 * ld * sizeof(int32_t), hipMemcpyDeviceToHost));
            HIPCHECK(hipMemcpy(wlen.data(), b->ar_wlen, n * sizeof(int32_t), hipMemcpyDeviceToHost));
            for (size_t s = 0; s < n; s++)
                if (code[s] >= 1000000) {
                    const double k = 1.0 + ord[0 * ld + s] + ord[1 * ld + s] + ord[2 * ld + s] + ord[3 * ld + s] + ord[4 * ld + s];
                    const double nn = (double)wlen[s];
                    out[s].aicc = aicc[s];
                    out[s].aic = aicc[s] - 2.0 * k * (k + 1.0) / (nn - k - 1.0);
                    out[s].bic = out[s].aic - 2.0 * k + k * std::log(nn);
                    out[s].reserved = ord[4 * ld + s];          // 1: the model has a constant
                }
        }
    } catch (const HipFail &f) {
        report_hip_failure(out_error, f);
        return false;
    } catch (const std::exception &e) {
        set_error(out_error, INTERNAL_ERROR, std::string("Internal error: ") + e.what());
        return false;
    }
    return true;
}

// The selected AutoARIMA fit of every series of the last run: orders, the coefficients as the recursion reads them (ar_pacf's box clip
// of the optimiser's coordinates, applied here), criterion and search counters.  Copies only; no kernel runs.
bool anofox_hip_batch_arima_fit(AnofoxHipBatch *b, AnofoxHipArimaFit *out, AnofoxError *out_error)
{
    if (!b || !out) { set_error(out_error, NULL_POINTER, "Null pointer argument"); return false; }
    if (!b->ran) { set_error(out_error, INVALID_INPUT, "Invalid input: the batch has not been run"); return false; }
    if (b->plan.model != M_AutoARIMA) { set_error(out_error, INVALID_INPUT, "Invalid input: the ARIMA fit readback needs an AutoARIMA batch"); return false; }
    DeviceGuard guard(b->dev);
    const size_t n = b->n, ld = b->ld;
    try {
        if (b->h_period.size() < n) throw HipFail{"the batch has no series block"};
        for (size_t s = 1; s < n; s++)
            if (b->h_period[s] != b->h_period[0]) throw HipFail{"the ARIMA fit readback needs one seasonal period for the whole batch"};
        HIPCHECK(hipStreamSynchronize(b->last_stream));
        std::vector<int32_t> code(n), status(n), ord(5 * ld), dd(n), DD(n), wlen(n), models(n), evals(n);
        std::vector<double> x(6 * ld), aicc(n);
        HIPCHECK(hipMemcpy(code.data(), b->d_model_code, n * sizeof(int32_t), hipMemcpyDeviceToHost));
        HIPCHECK(hipMemcpy(status.data(), b->d_status, n * sizeof(int32_t), hipMemcpyDeviceToHost));
        HIPCHECK(hipMemcpy(ord.data(), b->ar_order, 5 * ld * sizeof(int32_t), hipMemcpyDeviceToHost));
        HIPCHECK(hipMemcpy(dd.data(), b->ar_d, n * sizeof(int32_t), hipMemcpyDeviceToHost));
        HIPCHECK(hipMemcpy(DD.data(), b->ar_D, n * sizeof(int32_t), hipMemcpyDeviceToHost));
        HIPCHECK(hipMemcpy(wlen.data(), b->ar_wlen, n * sizeof(int32_t), hipMemcpyDeviceToHost));
        HIPCHECK(hipMemcpy(models.data(), b->ar_models, n * sizeof(int32_t), hipMemcpyDeviceToHost));
        HIPCHECK(hipMemcpy(evals.data(), b->d_evals_total, n * sizeof(int32_t), hipMemcpyDeviceToHost));
        HIPCHECK(hipMemcpy(x.data(), b->ar_x, 6 * ld * sizeof(double), hipMemcpyDeviceToHost));
        HIPCHECK(hipMemcpy(aicc.data(), b->ar_aicc, n * sizeof(double), hipMemcpyDeviceToHost));
        const double nan = std::nan("");
        for (size_t s = 0; s < n; s++) {
            AnofoxHipArimaFit &o = out[s];
            std::memset(&o, 0, sizeof o);
            o.status = status[s]; o.model_code = code[s]; o.seasonal_period = b->h_period[s];
            if (!(status[s] == 0 && code[s] >= 1000000)) {      // nothing was fitted (or the fallback chain forecast it): no stale values
                for (double &v : o.phi) v = nan;
                for (double &v : o.theta) v = nan;
                o.Phi[0] = o.Phi[1] = o.Theta[0] = o.Theta[1] = o.constant = o.aicc = nan;
                continue;
            }
            o.p = ord[0 * ld + s]; o.q = ord[1 * ld + s]; o.P = ord[2 * ld + s]; o.Q = ord[3 * ld + s]; o.has_constant = ord[4 * ld + s];
            o.d = dd[s]; o.D = DD[s];
            o.n_diff = wlen[s]; o.models_tried = models[s]; o.evals = evals[s];
            auto box = [](double a) { return a < -0.99 ? -0.99 : (a > 0.99 ? 0.99 : a); };      // arima.hip AR_COEF_BOX
            size_t k = 0;
            for (int i = 0; i < o.p && i < 5; i++) o.phi[i] = box(x[(k++) * ld + s]);
            for (int i = 0; i < o.q && i < 5; i++) o.theta[i] = box(x[(k++) * ld + s]);
            for (int i = 0; i < o.P && i < 2; i++) o.Phi[i] = box(x[(k++) * ld + s]);
            for (int i = 0; i < o.Q && i < 2; i++) o.Theta[i] = box(x[(k++) * ld + s]);
            o.constant = (o.has_constant && k < 6) ? x[k * ld + s] : 0.0;
            o.aicc = aicc[s];
        }
    } catch (const HipFail &f) {
        report_hip_failure(out_error, f);
        return false;
    } catch (const std::exception &e) {
        set_error(out_error, INTERNAL_ERROR, std::string("Internal error: ") + e.what());
        return false;
    }
    return true;
}

// ---------------------------------------------------------------------------------------------
// The batch entry on one device.  Every route -- one period given, merged periods, a part on a worker's reused batch, a single
// pooled series, a batch with regressors -- creates its device batch its own way (they differ in what a refused option block
// means) and then shares run_batch below and the deliver step of host_parts.hpp.
// ---------------------------------------------------------------------------------------------
extern "C++" {

using Clock = std::chrono::steady_clock;
static double ms_between(Clock::time_point a, Clock::time_point z) { return std::chrono::duration<double, std::milli>(z - a).count(); }

struct BatchPhases { Clock::time_point packed, ran, fetched; };       // when the phases of run_batch ended (ANOFOX_HIP_TIMING lines)

// Pack -> `between` (what a caller uploads beside the series: the per-column periods of a merged batch, the regressors of an
// exog batch) -> run -> fetch, on a batch that exists.  false: *e says why ("device batch failed" when no step did) and whatever
// the fetch had allocated is freed again; res must hold b->n zeroed or fetched results.
template <class Between>
static bool run_batch(AnofoxHipBatch *b, const double *const *values, const uint64_t *const *validity, const size_t *lengths, ForecastResult *res,
                      AnofoxError *errs, AnofoxError *e, BatchPhases *phases, Between &&between)
{
    clear_error(e);
    bool ok = anofox_hip_batch_pack_host(b, values, validity, lengths, e);
    const auto packed = Clock::now();
    if (ok) {
        try { between(); }
        catch (const HipFail &f) { report_hip_failure(e, f); ok = false; }
        catch (const std::exception &x) { set_error(e, INTERNAL_ERROR, std::string("Internal error: ") + x.what()); ok = false; }
    }
    ok = ok && anofox_hip_batch_run(b, nullptr, e);
    if (ok && b->tun.timing) (void)hipStreamSynchronize(b->last_stream);        // (the run's time, not the fetch's)
    const auto ran = Clock::now();
    ok = ok && anofox_hip_batch_fetch(b, res, errs);
    if (phases) *phases = BatchPhases{packed, ran, Clock::now()};
    if (!ok) {
        if (e->code == SUCCESS) set_error(e, INTERNAL_ERROR, "Internal error: device batch failed");
        free_results(res, b->n);
    }
    return ok;
}

// One plan, one device batch: create, pack, run, fetch (the whole of the batch entry unless periods are auto-detected).  The
// caller's arrays go straight through: no per-series copy, the fetch writes into out_results.
static bool forecast_batch_uniform(const double *const *values, const uint64_t *const *validity, const size_t *lengths, size_t n_series,
                                   const ForecastOptions *options, const int *horizons, ForecastResult *out_results,
                                   AnofoxError *out_errors, AnofoxError *out_batch_error)
{
    ForecastOptions opt = *options;
    size_t t_max = 0;
    for (size_t s = 0; s < n_series; s++) {
        t_max = std::max(t_max, lengths[s]);
        if (horizons) opt.horizon = std::max(opt.horizon, horizons[s]);
    }
    AnofoxHipBatch *b = nullptr;
    AnofoxError e;
    const auto t0 = Clock::now();
    if (!anofox_hip_batch_create(n_series, t_max, &opt, &b, &e)) {
        // (a rejected option block is every long-enough series' own error: a batch made only of short series does not abort the statement)
        if (e.code == INVALID_INPUT) { option_error_per_series(out_errors, lengths, n_series, e); return true; }
        if (out_batch_error) *out_batch_error = e;
        if (out_errors) for (size_t s = 0; s < n_series; s++) out_errors[s] = e;
        return false;
    }
    const bool timing = b->tun.timing;     // ANOFOX_HIP_TIMING: phase times of the batch entry on stderr
    const auto t1 = Clock::now();
    BatchPhases ph;
    const bool ok = run_batch(b, values, validity, lengths, out_results, out_errors, &e, &ph, [] {});
    if (!ok) { if (out_batch_error) *out_batch_error = e; }
    else if (horizons) for (size_t s = 0; s < n_series; s++) truncate_to_horizon(out_results[s], horizons[s]);
    anofox_hip_batch_destroy(b);
    if (timing)
        std::fprintf(stderr, "[anofox-hip] batch of %zu: create %.1f ms, pack + H2D %.1f ms, run %.1f ms, fetch %.1f ms, destroy %.1f ms\n", n_series,
                     ms_between(t0, t1), ms_between(t1, ph.packed), ms_between(ph.packed, ph.ran), ms_between(ph.ran, ph.fetched), ms_between(ph.fetched, Clock::now()));
    return ok;
}

namespace {

// the caller's arrays of one batch call
struct BatchCall {
    const double *const *values; const uint64_t *const *validity; const size_t *lengths; size_t n_series;
    const ForecastOptions *options; const int *horizons; ForecastResult *out_results; AnofoxError *out_errors;
};

// The first failure among the batches that run side by side for one call speaks for the call.
struct FirstError {
    std::mutex mu; bool ok = true; AnofoxError first;
    FirstError() { clear_error(&first); }
    void fail(const AnofoxError &e)
    {
        std::lock_guard<std::mutex> lock(mu);
        if (ok) first = e;
        ok = false;
    }
    void fail(const std::string &msg) { AnofoxError e; clear_error(&e); set_error(&e, INTERNAL_ERROR, msg); fail(e); }
};

// The host threads of one call: joined before the call returns, whatever the way out.
struct ThreadJoiner {
    std::vector<std::thread> threads;
    ~ThreadJoiner() { join(); }
    void join() { for (auto &t : threads) if (t.joinable()) t.join(); }
    // false: the host's thread limit (EAGAIN) -- the caller does the work on its own thread
    template <class Work> bool start(const Work &work) { try { threads.emplace_back(work); return true; } catch (const std::system_error &) { return false; } }
};

// What a host thread that works for a call runs under: the call's device (a per-thread setting) and the ARIMA method that was in
// force when the call came in.  Nothing may leave a worker thread.
template <class Body> void call_worker(int device, int method, FirstError &errors, Body &&body)
{
    ArimaMethodScope method_scope(method);
    try {
        (void)hipSetDevice(device);
        body();
    } catch (const std::exception &e) { errors.fail(std::string("Internal error: ") + e.what()); }
    catch (...) { errors.fail("Internal error: worker failed"); }
}

const double EMPTY_SERIES = 0.0;        // what a padding column points at (length 0)

// The series behind the columns of one device batch -- src[j] is the caller's series of column j, PAD_COLUMN an empty one -- and
// the room for their results.
struct Columns {
    std::vector<size_t> src, len;
    std::vector<const double *> v;
    std::vector<const uint64_t *> m;
    std::vector<ForecastResult> res;
    std::vector<AnofoxError> errs;
    size_t t_max = 0;           // the longest series
    int h_max = 0;              // the largest horizon: the call's, or a series' own

    void gather(const BatchCall &c)
    {
        const size_t n = src.size();
        v.resize(n); m.resize(n); len.resize(n); res.resize(n); errs.resize(n);
        t_max = 0;
        h_max = c.options->horizon;
        for (size_t j = 0; j < n; j++) {
            const size_t s = src[j];
            const bool pad = s == PAD_COLUMN;
            v[j] = pad ? &EMPTY_SERIES : c.values[s];
            m[j] = pad || !c.validity ? nullptr : c.validity[s];
            len[j] = pad ? 0 : c.lengths[s];
            std::memset(&res[j], 0, sizeof(ForecastResult));
            clear_error(&errs[j]);
            t_max = std::max(t_max, len[j]);
            if (!pad && c.horizons) h_max = std::max(h_max, c.horizons[s]);
        }
    }
    const uint64_t *const *masks(const BatchCall &c) const { return c.validity ? m.data() : nullptr; }
    void deliver(const BatchCall &c) { deliver_results(res.data(), errs.data(), src.data(), src.size(), c.horizons, c.options->horizon, c.out_results, c.out_errors); }
};

// the option block of a batch that names its period: forecast() sees the same period either way (forecast.rs:527-539)
ForecastOptions part_options(const ForecastOptions *options, int period, int horizon)
{
    ForecastOptions o = *options;
    o.auto_detect_seasonality = false;
    o.seasonal_period = period > 1 ? period : 0;           // 0 with detection off: period 1
    o.horizon = horizon;
    return o;
}

// the period a model uses for a series whose detected period is `period`
int used_period(ModelType model, int period)
{
    switch (model) {
    case M_Naive: case M_RandomWalkDrift: case M_ARIMA: case M_SES: case M_SESOptimized: case M_Holt: return 1;
    case M_CrostonClassic: case M_CrostonSBA: case M_TSB: case M_ADIDA: case M_IMAPA: return 1;
    case M_AutoARIMA: return period > ETS_MAX_PERIOD ? ETS_MAX_PERIOD + 1 : (period > 1 ? period : 1);      // (forecast.rs:528-537, 1448-1452: any detected period is seasonal)
    default: return period;
    }
}

std::vector<int> detect_used_periods(const BatchCall &c, ModelType model, bool timing)
{
    const auto t0 = Clock::now();
    const std::vector<int> raw = detect_periods_host_series(c.values, c.validity, c.lengths, c.n_series);
    std::vector<int> period(c.n_series, 1);
    for (size_t s = 0; s < c.n_series; s++) period[s] = c.lengths[s] < 3 ? 1 : used_period(model, raw[s] > 0 ? raw[s] : 1);
    if (timing) std::fprintf(stderr, "[anofox-hip] period detection of %zu series: %.1f ms\n", c.n_series, ms_between(t0, Clock::now()));
    return period;
}

// AutoETS and the seasonal smoothing family: the small parts of a ring class run as ONE batch (138 tiny batches x 25 spec chains
// on 16 hardware queues were latency bound end to end).  AutoARIMA: every detected period is seasonal (forecast.rs:528-537,
// 1448-1452) -- ~400 distinct ones on the M5 shape, each a latency-bound batch of its own (13 sweeps with a host round trip
// apiece: 8.2 s for the 30,490 series) -- so the periods above 24 (ring of seasonal lags in the HBM scratch) run as ONE batch
// with the period per series (arima.hip pass variant 6).
MergeRule merge_rule(const Plan &plan, const Tunables &tun)
{
    if (!tun.merge_periods) return MergeRule::None;
    if (plan.model == M_AutoARIMA) return MergeRule::AutoArima;
    const bool seasonal_ets = plan.model == M_AutoETS || plan.model == M_HoltWinters || plan.model == M_SeasonalES || plan.model == M_SeasonalESOptimized ||
                              (plan.model == M_ETS && plan.ets_spec_id >= 0 && spec_season(plan.ets_spec_id) != 0);
    return seasonal_ets ? MergeRule::EtsLike : MergeRule::None;
}

// a part as a device batch of its own through the plain path, which also reports what is wrong with the option block
void run_part(const BatchCall &c, const Part &part, FirstError &errors)
{
    Columns col;
    col.src = part.series;
    col.gather(c);
    const ForecastOptions o = part_options(c.options, part.period, col.h_max);
    AnofoxError be;
    const bool ok = forecast_batch_uniform(col.v.data(), col.masks(c), col.len.data(), col.src.size(), &o, nullptr, col.res.data(), col.errs.data(), &be);
    col.deliver(c);             // (after a failure: the per-series errors, no arrays)
    if (!ok) errors.fail(be);
}

// the parts of one ring class as ONE batch whose 64-column blocks each have their own period
void run_merged(const BatchCall &c, const MergedBatch &batch, bool timing, FirstError &errors)
{
    MergedColumns mc = merged_columns(batch);
    Columns col;
    col.src = std::move(mc.src);
    col.gather(c);
    const size_t nc = col.src.size();
    const ForecastOptions o = part_options(c.options, mc.m_max, col.h_max);
    AnofoxHipBatch *mb = nullptr;
    AnofoxError be;
    clear_error(&be);
    const auto t0 = Clock::now();
    bool ok = anofox_hip_batch_create(nc, col.t_max, &o, &mb, &be);
    const auto t1 = Clock::now();
    BatchPhases ph{t1, t1, t1};
    if (ok) {
        ok = run_batch(mb, col.v.data(), col.masks(c), col.len.data(), col.res.data(), col.errs.data(), &be, &ph, [&] {
            mc.period.resize(mb->ld, mc.period.back());
            mb->d_m_col = dalloc<int32_t>(mb->ld);
            HIPCHECK(hipMemcpy(mb->d_m_col, mc.period.data(), mb->ld * sizeof(int32_t), hipMemcpyHostToDevice));
            mb->merged_m_max = mc.m_max;
            for (size_t j = 0; j < nc; j++) mb->h_period[j] = mc.period[j];     // what the host-side fitted values use
        });
        anofox_hip_batch_destroy(mb);
    } else if (be.code == SUCCESS) set_error(&be, INTERNAL_ERROR, "Internal error: device batch failed");
    if (timing)
        std::fprintf(stderr, "[anofox-hip] merged batch: %zu parts with periods %d..%d in %zu columns: %.1f ms (create %.1f, pack %.1f, run %.1f, fetch + destroy %.1f)\n",
                     batch.size(), batch.front().period, mc.m_max, nc, ms_between(t0, Clock::now()), ms_between(t0, t1), ms_between(t1, ph.packed),
                     ms_between(ph.packed, ph.ran), ms_between(ph.ran, Clock::now()));
    if (ok) col.deliver(c);
    else errors.fail(be);
}

// The small parts, pulled from a shared counter.  A worker keeps ONE device batch for all its parts (creating and destroying a
// batch costs ~30 ms of allocator calls that serialise across threads -- as much as the part's own run): capacity = the largest
// small part, short parts are padded with empty series, the period is set before every pack.
void run_small_parts(const BatchCall &c, const std::vector<Part> &small, std::atomic<size_t> &next, size_t t_cap, int h_cap, bool timing,
                     Clock::time_point t_start, FirstError &errors)
{
    if (small.empty()) return;
    const size_t cap = small.front().series.size();
    AnofoxHipBatch *wb = nullptr;
    Columns col;
    for (size_t g = next.fetch_add(1); g < small.size(); g = next.fetch_add(1)) {
        const Part &part = small[g];
        AnofoxError be;
        if (!wb) {
            const ForecastOptions o = part_options(c.options, part.period, h_cap);
            if (!anofox_hip_batch_create(cap, t_cap, &o, &wb, &be)) { wb = nullptr; run_part(c, part, errors); continue; }   // the plain path reports it
        }
        wb->opt.seasonal_period = part.period > 1 ? part.period : 0;
        col.src = part.series;
        col.src.resize(cap, PAD_COLUMN);
        col.gather(c);
        const auto tw0 = Clock::now();
        const bool ok = run_batch(wb, col.v.data(), col.masks(c), col.len.data(), col.res.data(), col.errs.data(), &be, nullptr, [] {});
        if (timing)
            std::fprintf(stderr, "[anofox-hip] small part: period %d, %zu series: %.1f ms (started at %.1f ms)\n", part.period, part.series.size(),
                         ms_between(tw0, Clock::now()), ms_between(t_start, tw0));
        if (ok) col.deliver(c);
        else errors.fail(be);
    }
    if (wb) anofox_hip_batch_destroy(wb);
}

} // namespace
} // extern "C++"

// The batch entry on the calling thread's current device.  Per-series period detection (params := MAP{}): every distinct period a
// model uses is its own run of the pipeline, latency bound and tiny (~140 distinct periods per thousand M5-like series).  Detect
// the periods, plan how the batch is cut (host_parts.hpp) and run the pieces side by side from a few host threads, each as a
// batch that names its period(s) -- forecast() sees the same period either way (forecast.rs:527-539), so the results are unchanged.
static bool forecast_batch_one_device(const double *const *values, const uint64_t *const *validity, const size_t *lengths, size_t n_series,
                                      const ForecastOptions *options, const int *horizons, ForecastResult *out_results,
                                      AnofoxError *out_errors, AnofoxError *out_batch_error)
{
    Plan plan;
    AnofoxError pe;
    const bool detect = options->auto_detect_seasonality && options->seasonal_period == 0 && n_series >= 2;
    if (!detect || !make_plan(options, plan, &pe))
        return forecast_batch_uniform(values, validity, lengths, n_series, options, horizons, out_results, out_errors, out_batch_error);
    const BatchCall c{values, validity, lengths, n_series, options, horizons, out_results, out_errors};
    try {
        EvictionDeferral park_evictions;                 // several batches run side by side below
        const Tunables tun = Tunables::from_env();
        const PartPlan parts = plan_parts(parts_by_period(detect_used_periods(c, plan.model, tun.timing)), merge_rule(plan, tun),
                                          PartLimits{ETS_MERGED_LDS_PERIOD, ETS_MAX_PERIOD});
        if (tun.timing) {
            std::string desc;
            for (const auto *list : {&parts.big, &parts.small})
                for (const Part &part : *list) desc += " " + std::to_string(part.period) + "x" + std::to_string(part.series.size());
            std::fprintf(stderr, "[anofox-hip] remaining parts (period x series):%s\n", desc.c_str());
        }
        FirstError errors;
        const int method = arima_method_in_force();
        int device = 0;
        (void)hipGetDevice(&device);
        size_t t_cap = 0;                                // what a worker's reused batch must hold
        int h_cap = options->horizon;
        for (size_t s = 0; s < n_series; s++) { t_cap = std::max(t_cap, lengths[s]); if (horizons) h_cap = std::max(h_cap, horizons[s]); }
        std::atomic<size_t> next_small{0}, next_big{0};
        const auto t_small0 = Clock::now();
        // The big parts fill the chip on their own and hold the most memory: up to four side by side (one is throttled by whatever
        // else runs; one after the other they were the critical path of the call), largest first, each a batch of its own.
        auto big_work = [&] {
            call_worker(device, method, errors, [&] { for (size_t g = next_big.fetch_add(1); g < parts.big.size(); g = next_big.fetch_add(1)) run_part(c, parts.big[g], errors); });
        };
        // The small parts run side by side on the workers.  (A small part is a chain of latency-bound launches with host round trips
        // in between -- AutoARIMA: ~13 sweeps of advance / read-back / fit, ~0.2 s whatever its size -- so the number of parts in
        // flight is what the call's duration divides by; it hardly slows a big one.)
        auto small_work = [&] {
            call_worker(device, method, errors, [&] { run_small_parts(c, parts.small, next_small, t_cap, h_cap, tun.timing, t_small0, errors); });
        };
        const size_t part_threads = (size_t)std::max(1, tun.part_threads);
        const size_t n_small_thr = std::max<size_t>(1, std::min<size_t>({(size_t)std::thread::hardware_concurrency(), part_threads, parts.small.size()}));
        const size_t n_big_thr = std::min<size_t>(parts.big.size(), 4);

        ThreadJoiner threads;
        // The merged batches of a group one after the other; the groups side by side (each is latency bound by its slowest fit and
        // far from filling the chip) and beside the parts that stay separate.
        for (const std::vector<MergedBatch> &group : parts.merged_groups) {
            auto work = [&, g = &group] { call_worker(device, method, errors, [&] { for (const MergedBatch &batch : *g) run_merged(c, batch, tun.timing, errors); }); };
            if (!threads.start(work)) work();            // (a group that finds no thread runs here, before the parts)
        }
        // (workers pull parts from shared counters: the ones that cannot be started are not missed, this thread takes what is left)
        for (size_t i = n_big_thr ? 0 : 1; i < n_small_thr; i++) if (!threads.start(small_work)) break;
        for (size_t i = 1; i < n_big_thr; i++) if (!threads.start(big_work)) break;
        if (n_big_thr) big_work();
        small_work();
        threads.join();
        if (!errors.ok && out_batch_error) *out_batch_error = errors.first;
        return errors.ok;
    } catch (const std::exception &e) {
        set_error(out_batch_error, INTERNAL_ERROR, std::string("Internal error: ") + e.what());
        return false;
    }
}

// ---------------------------------------------------------------------------------------------
// Multi-device batch entry (north star: "series-id ranges shard trivially across the 8 GPUs of one node", behind ts_forecast_by;
// replaces the ONE-thread finalize loop of ts_forecast_native.cpp:559-800 with one host thread per device)
// ---------------------------------------------------------------------------------------------
bool anofox_hip_set_devices(const int *devices, size_t n_devices)
{
    std::vector<int> v;
    if (n_devices) {
        if (!devices) return false;
        int cnt = 0;
        if (hipGetDeviceCount(&cnt) != hipSuccess) return false;
        for (size_t i = 0; i < n_devices; i++) { if (devices[i] < 0 || devices[i] >= cnt) return false; v.push_back(devices[i]); }
    }
    DeviceList &d = device_list();
    std::lock_guard<std::mutex> lock(d.mu);
    d.env_read = true;
    d.devs = v;
    return true;
}

size_t anofox_hip_get_devices(int *devices, size_t capacity)
{
    const std::vector<int> v = devices_in_use(nullptr);
    for (size_t i = 0; i < v.size() && i < capacity && devices; i++) devices[i] = v[i];
    return v.size();
}

void anofox_hip_set_min_series_per_device(size_t min_series)
{
    DeviceList &d = device_list();
    std::lock_guard<std::mutex> lock(d.mu);
    d.min_series = std::max<size_t>(min_series, 1);
}

// contiguous ranges [g * ceil(N / G), (g + 1) * ceil(N / G)) -- SURVEY.md section 8(e), the same rule as dist.shard_range
void anofox_hip_shard_range(size_t n_series, size_t n_shards, size_t shard, size_t *begin, size_t *end)
{
    const size_t per = n_shards ? (n_series + n_shards - 1) / n_shards : n_series;
    const size_t lo = std::min(n_series, shard * per), hi = std::min(n_series, lo + per);
    if (begin) *begin = lo;
    if (end) *end = hi;
}

bool anofox_ts_forecast_batch(const double *const *values, const uint64_t *const *validity, const size_t *lengths, size_t n_series,
                              const ForecastOptions *options, const int *horizons, ForecastResult *out_results,
                              AnofoxError *out_errors, AnofoxError *out_batch_error)
{
    clear_error(out_batch_error);
    if (!values || !lengths || !options || !out_results) { set_error(out_batch_error, NULL_POINTER, "Null pointer argument"); return false; }
    for (size_t s = 0; s < n_series; s++) {
        std::memset(&out_results[s], 0, sizeof(ForecastResult));
        if (!values[s]) { set_error(out_batch_error, NULL_POINTER, "Null pointer argument"); return false; }
    }
    size_t min_series = 2048;
    const std::vector<int> devs = devices_in_use(&min_series);
    // as many shards as there are listed devices, but none smaller than min_series (a shard that does not fill its device
    // finishes no sooner than a larger one: the fit is bound by its slowest problems)
    const size_t G = devs.empty() ? 1 : std::max<size_t>(1, std::min(devs.size(), n_series / std::max<size_t>(min_series, 1)));
    if (devs.empty()) {
        const auto tb0 = std::chrono::steady_clock::now();
        const bool r = forecast_batch_one_device(values, validity, lengths, n_series, options, horizons, out_results, out_errors, out_batch_error);
        if (Tunables::from_env().timing)
            std::fprintf(stderr, "[anofox-hip] anofox_ts_forecast_batch: %zu series in %.1f ms\n", n_series,
                         std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tb0).count());
        return r;
    }
    if (G == 1) {
        DeviceGuard guard(devs[0]);
        return forecast_batch_one_device(values, validity, lengths, n_series, options, horizons, out_results, out_errors, out_batch_error);
    }
    // one host thread per shard: its device made current, its own batch (stream set, allocator cache entries and pinned
    // staging block of that device), its slice of the caller's arrays -- the shards share nothing but the option block
    std::vector<AnofoxError> berr(G);
    std::vector<char> ok(G, 1);
    const bool timing = std::getenv("ANOFOX_HIP_TIMING") != nullptr;
    const auto t0 = std::chrono::steady_clock::now();
    const int method_in_force = arima_method_in_force();
    auto shard = [&](size_t g) {
        ArimaMethodScope method_scope(method_in_force);
        berr[g].code = SUCCESS; berr[g].message[0] = 0;
        try {
            size_t lo = 0, hi = 0;
            anofox_hip_shard_range(n_series, G, g, &lo, &hi);
            if (hi <= lo) return;
            if (hipSetDevice(devs[g]) != hipSuccess) { set_error(&berr[g], INTERNAL_ERROR, "Internal error: cannot select device " + std::to_string(devs[g])); ok[g] = 0; return; }
            tl_host_thread_share = (unsigned)G;
            ok[g] = forecast_batch_one_device(values + lo, validity ? validity + lo : nullptr, lengths + lo, hi - lo, options, horizons ? horizons + lo : nullptr,
                                              out_results + lo, out_errors ? out_errors + lo : nullptr, &berr[g]) ? 1 : 0;
            tl_host_thread_share = 1;
        } catch (const std::exception &e) {           // nothing may leave a worker thread
            set_error(&berr[g], INTERNAL_ERROR, std::string("Internal error: ") + e.what()); ok[g] = 0;
        } catch (...) { set_error(&berr[g], INTERNAL_ERROR, "Internal error: device shard failed"); ok[g] = 0; }
    };
    int caller_dev = 0;
    (void)hipGetDevice(&caller_dev);
    parallel_shares((unsigned)G, [&](unsigned g) { shard((size_t)g); });       // (a shard that finds no thread runs after shard 0, on this one)
    (void)hipSetDevice(caller_dev);
    if (timing)
        std::fprintf(stderr, "[anofox-hip] batch of %zu over %zu device shards: %.1f ms\n", n_series, G,
                     std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
    bool all_ok = true;
    for (size_t g = 0; g < G; g++)
        if (!ok[g] || berr[g].code != SUCCESS) {
            // the option errors (INVALID_MODEL / INVALID_INPUT) are uniform across the shards: the first one speaks for the batch
            if (out_batch_error && out_batch_error->code == SUCCESS) *out_batch_error = berr[g];
            if (!ok[g]) all_ok = false;
        }
    return all_ok;
}

// Block 3 counterpart: run several device-resident batches -- typically one per device, each created after
// anofox_hip_set_device(d) -- side by side, one host thread per batch (a run synchronises its stream a few times, so one thread
// cannot drive several devices concurrently).  Returns false if any run failed; out_errors (may be NULL) is per batch.
bool anofox_hip_batch_run_many(AnofoxHipBatch *const *batches, size_t n_batches, AnofoxError *out_errors)
{
    if (!batches && n_batches) return false;
    std::vector<char> ok(n_batches, 1);
    auto one = [&](size_t i) {
        AnofoxError e;
        clear_error(&e);
        try { ok[i] = anofox_hip_batch_run(batches[i], nullptr, &e) ? 1 : 0; }
        catch (...) { ok[i] = 0; set_error(&e, INTERNAL_ERROR, "Internal error: batch run failed"); }
        if (out_errors) out_errors[i] = e;
    };
    parallel_shares((unsigned)n_batches, [&](unsigned i) { one((size_t)i); });
    for (size_t i = 0; i < n_batches; i++) if (!ok[i]) return false;
    return true;
}

// one series on a parked one-series device batch (or a new one): pack, run, fetch, park again
static bool forecast_one_pooled(const double *values, const uint64_t *validity, size_t length, const ForecastOptions *options, const ForecastOptions &key,
                                ForecastResult *out_result, AnofoxError *out_error)
{
    AnofoxError e, se;
    clear_error(&e);
    clear_error(&se);
    const double *vals[1] = {values};
    const uint64_t *valid[1] = {validity};
    size_t lens[1] = {length};
    ForecastResult r;
    std::memset(&r, 0, sizeof r);
    // a pooled single-series batch: the option block is the key, the capacity covers series up to twice this length
    int device = 0;
    (void)hipGetDevice(&device);
    AnofoxHipBatch *b = pool_take(key, length, device);
    if (b) {
        try { batch_attach_streams(b); }
        catch (const HipFail &f) { report_hip_failure(out_error, f); anofox_hip_batch_destroy(b); return false; }
        b->arima_method = arima_method_in_force();      // a parked batch predates the method of this call
        b->tun = Tunables::from_env();
    }
    if (!b) {
        size_t cap = 256;
        while (cap < 2 * length) cap *= 2;
        if (!anofox_hip_batch_create(1, cap, options, &b, &e)) {
            if (out_error) *out_error = e;                     // INVALID_INPUT etc.: the series is long enough, so the option error is its error
            return false;
        }
    }
    if (!run_batch(b, vals, validity ? valid : nullptr, lens, &r, &se, &e, nullptr, [] {})) {
        anofox_hip_batch_destroy(b);                            // a batch that failed is not reused
        if (out_error) *out_error = e;
        return false;
    }
    pool_give(key, device, b);
    if (se.code != SUCCESS) { if (out_error) *out_error = se; return false; }
    *out_result = r;
    return true;
}

// Route A coalescing (ts_forecast_scalar.cpp:298-523: every DuckDB worker thread calls anofox_ts_forecast once per group of its
// chunk, concurrently): a one-series fit is latency bound -- 5 ms for AutoETS, the chip all but idle -- so calls that are inside the
// library AT THE SAME TIME with an equal option block join ONE multi-series batch.  The first caller of a key opens a group and
// leads it: it waits until every call currently inside the library has joined or at most ANOFOX_HIP_COALESCE_US (default 1,000 us;
// a lone caller does not wait at all), closes the group and runs it through the batch entry; the followers sleep on the group and
// pick up their own result and their own error (per-series isolation is the batch entry's: out_errors).  Results are those of
// single calls bit for bit -- a series' result does not depend on the batch it is in (test_concurrent_single_series_calls).
struct CoalesceReq { const double *values; const uint64_t *validity; size_t length; ForecastResult res; AnofoxError err; bool ok = false; };
struct CoalesceGroup {
    ForecastOptions key; int device = 0; int method = 0;
    std::vector<CoalesceReq *> reqs;
    bool closed = false, done = false;
    std::condition_variable cv;
};
static std::mutex g_co_mu;
static std::vector<std::shared_ptr<CoalesceGroup>> g_co_open;
static int g_co_inflight = 0;                     // calls inside anofox_ts_forecast past their argument checks (under g_co_mu)
static int g_co_recent_width = 1;                 // the largest number of concurrent calls seen in the last 20 ms, and when: workers that call
static std::chrono::steady_clock::time_point g_co_recent_time;   // again and again arrive a few microseconds apart, so the first one back waits for its peers
constexpr size_t COALESCE_MAX = 256;

bool anofox_ts_forecast(const double *values, const uint64_t *validity, size_t length, const ForecastOptions *options,
                        ForecastResult *out_result, AnofoxError *out_error)
{
    clear_error(out_error);
    if (!values || !options || !out_result) { set_error(out_error, NULL_POINTER, "Null pointer argument"); return false; }
    // argument errors come first, exactly like the reference (lib.rs:3368-3380, forecast.rs:514-565)
    {
        std::string mname = cstr_field(options->model, sizeof options->model);
        ModelType mt;
        if (!parse_model(mname, mt)) { set_error(out_error, INVALID_MODEL, "Invalid model: Unknown model: '" + mname + "'"); return false; }
        if (options->horizon < 0) { set_error(out_error, PANIC_CAUGHT, "Panic in Rust code"); return false; }
        if (series_too_short(out_error, length)) return false;
    }
    // the option block is the key (every byte of it: callers memset it first, ts_forecast_scalar.cpp:440)
    ForecastOptions key;                       // normalised copy: padding and the bytes behind a string's NUL do not take part
    std::memset(&key, 0, sizeof key);
    auto copy_str = [](char *dst, const char *src, size_t cap) { for (size_t i = 0; i + 1 < cap && src[i]; i++) dst[i] = src[i]; };
    copy_str(key.model, options->model, sizeof key.model);
    copy_str(key.ets_model, options->ets_model, sizeof key.ets_model);
    copy_str(key.seasonal_periods_str, options->seasonal_periods_str, sizeof key.seasonal_periods_str);
    copy_str(key.model_pool, options->model_pool, sizeof key.model_pool);
    copy_str(key.laplace_variant, options->laplace_variant, sizeof key.laplace_variant);
    key.horizon = options->horizon; key.confidence_level = options->confidence_level; key.seasonal_period = options->seasonal_period;
    key.auto_detect_seasonality = options->auto_detect_seasonality; key.include_fitted = options->include_fitted;
    key.include_residuals = options->include_residuals; key.window = options->window;
    key.laplace_seasonal_batch_init = options->laplace_seasonal_batch_init;

    const double window_us = ProcessTunables::get().coalesce_us;
    if (!(window_us > 0.0)) return forecast_one_pooled(values, validity, length, options, key, out_result, out_error);
    int device = 0;
    (void)hipGetDevice(&device);
    const int method = g_default_arima_method.load();
    CoalesceReq req;
    req.values = values; req.validity = validity; req.length = length;
    std::memset(&req.res, 0, sizeof req.res);
    req.err.code = SUCCESS; req.err.message[0] = 0;
    std::shared_ptr<CoalesceGroup> grp;
    bool leader = false;
    {
        std::unique_lock<std::mutex> lock(g_co_mu);
        g_co_inflight++;
        const auto now = std::chrono::steady_clock::now();
        const bool recent = now - g_co_recent_time < std::chrono::milliseconds(20);
        if (g_co_inflight > 1 && (g_co_inflight >= g_co_recent_width || !recent)) { g_co_recent_width = g_co_inflight; g_co_recent_time = now; }
        else if (g_co_inflight > 1 && recent) g_co_recent_time = now;
        for (auto &g : g_co_open)
            if (!g->closed && g->device == device && g->method == method && g->reqs.size() < COALESCE_MAX && std::memcmp(&g->key, &key, sizeof key) == 0) { grp = g; break; }
        if (grp) {
            grp->reqs.push_back(&req);
            grp->cv.notify_all();                                  // the leader re-checks "has everyone inside joined?"
            grp->cv.wait(lock, [&] { return grp->done; });
            g_co_inflight--;
        } else {
            leader = true;
            grp = std::make_shared<CoalesceGroup>();
            grp->key = key; grp->device = device; grp->method = method;
            grp->reqs.push_back(&req);
            g_co_open.push_back(grp);
            const int expect = recent ? std::max(g_co_inflight, g_co_recent_width) : g_co_inflight;
            if (expect > 1) {
                // other calls are inside the library right now, or were a moment ago: give them the window to join (those of another
                // key never will: the window bounds what their presence costs; a caller that has always been alone never waits)
                const auto deadline = now + std::chrono::nanoseconds((long long)(window_us * 1000.0));
                grp->cv.wait_until(lock, deadline, [&] { return (int)grp->reqs.size() >= std::max(expect, g_co_inflight) || grp->reqs.size() >= COALESCE_MAX; });
            }
            grp->closed = true;
            g_co_open.erase(std::find(g_co_open.begin(), g_co_open.end(), grp));
        }
    }
    if (!leader) {
        if (!req.ok) { if (out_error) *out_error = req.err; return false; }
        *out_result = req.res;
        return true;
    }
    // ---- the leader runs the group (its members are blocked on the group; their request records live on their stacks) ----
    // Whatever happens below -- a refused allocation of the argument vectors included -- every member gets an answer and is woken:
    // the guard fills the requests nobody answered with INTERNAL_ERROR, marks the group done and gives the in-flight count back.
    const size_t k = grp->reqs.size();
    char answered[COALESCE_MAX] = {0};          // (no allocation outside the try block; k <= COALESCE_MAX)
    struct LeaderGuard {
        std::shared_ptr<CoalesceGroup> &grp;
        char *answered;
        ~LeaderGuard()
        {
            for (size_t j = 0; j < grp->reqs.size() && j < COALESCE_MAX; j++)
                if (!answered[j]) {
                    CoalesceReq *q = grp->reqs[j];
                    q->ok = false;
                    set_error(&q->err, INTERNAL_ERROR, "Internal error: coalesced batch failed");
                }
            std::lock_guard<std::mutex> lock(g_co_mu);
            grp->done = true;
            g_co_inflight--;
            grp->cv.notify_all();
        }
    };
    bool my_ok = false;
    try {
        LeaderGuard guard{grp, answered};
        ArimaMethodScope method_scope(grp->method);        // the method the members were matched on, not a re-read of the process default
        if (k == 1) {
            my_ok = forecast_one_pooled(values, validity, length, options, key, &req.res, &req.err);
            req.ok = my_ok;
            answered[0] = 1;
        } else {
            std::vector<const double *> v(k);
            std::vector<const uint64_t *> m(k);
            std::vector<size_t> len(k);
            bool any_mask = false;
            for (size_t j = 0; j < k; j++) { v[j] = grp->reqs[j]->values; m[j] = grp->reqs[j]->validity; len[j] = grp->reqs[j]->length; any_mask |= m[j] != nullptr; }
            std::vector<ForecastResult> res(k);
            std::vector<AnofoxError> errs(k);
            for (size_t j = 0; j < k; j++) { std::memset(&res[j], 0, sizeof(ForecastResult)); clear_error(&errs[j]); }
            AnofoxError be;
            clear_error(&be);
            bool ok = false;
            try {
                ok = forecast_batch_one_device(v.data(), any_mask ? m.data() : nullptr, len.data(), k, options, nullptr, res.data(), errs.data(), &be);
            } catch (...) { ok = false; }
            if (!ok && be.code == SUCCESS) set_error(&be, INTERNAL_ERROR, "Internal error: device batch failed");
            for (size_t j = 0; j < k; j++) {
                CoalesceReq *q = grp->reqs[j];
                if (!ok) { anofox_free_forecast_result(&res[j]); q->ok = false; q->err = be; }
                else if (errs[j].code != SUCCESS) { anofox_free_forecast_result(&res[j]); q->ok = false; q->err = errs[j]; }
                else { q->ok = true; q->res = res[j]; }
                answered[j] = 1;
            }
            my_ok = req.ok;
        }
    } catch (...) {
        // (the guard has answered and woken everyone; nothing leaves the C ABI)
        my_ok = false;
        if (req.err.code == SUCCESS) set_error(&req.err, INTERNAL_ERROR, "Internal error: coalesced batch failed (out of host memory)");
    }
    if (!my_ok) { if (out_error) *out_error = req.err; return false; }
    *out_result = req.res;
    return true;
}

// ------------------------------------------------------------------------------------------------------------------------------
// MSTL decomposition (decomposition.rs mstl_decompose; fit_mstl.hip)
// ------------------------------------------------------------------------------------------------------------------------------
bool anofox_hip_mstl_decompose_device(const double *y, size_t ld, const int32_t *lengths, size_t n_series, size_t t_rows,
                                      const int *periods, size_t n_periods, int insufficient_data_mode, double *trend,
                                      double *seasonal, double *remainder, int32_t *info, void *stream, AnofoxError *out_error)
{
    clear_error(out_error);
    if (!y || !lengths || !trend || !remainder || !info || (n_periods > 0 && (!periods || !seasonal))) {
        set_error(out_error, NULL_POINTER, "Null pointer argument");
        return false;
    }
    if (n_periods > (size_t)MSTL_MAX_PERIODS) {
        set_error(out_error, COMPUTATION_ERROR, "Computation error: MSTL takes at most " + std::to_string(MSTL_MAX_PERIODS) +
                                                    " seasonal periods, got " + std::to_string(n_periods));
        return false;
    }
    if (ld < n_series) { set_error(out_error, INVALID_INPUT, "Invalid input: ld is smaller than n_series"); return false; }
    if (!device_ready(out_error)) return false;
    MstlArgs a{};
    a.y = y; a.ld = ld; a.len = lengths; a.n_series = (int)n_series; a.t_rows = t_rows;
    a.mode = (insufficient_data_mode == 1 || insufficient_data_mode == 2) ? insufficient_data_mode : MSTL_MODE_FAIL;
    std::vector<int> ps(periods, periods + n_periods);
    std::sort(ps.begin(), ps.end(), std::greater<int>());          // longest first (decomposition.rs:235-236)
    // A period above t_rows / 2 + 1 is lowered to it: no series of the block holds two of its seasons either way (n <= t_rows <
    // 2 p), so every test the kernels make on it keeps its outcome, and 2 p stays far from the int range.
    const long long p_cap = (long long)(t_rows / 2) + 1;
    auto capped = [&](int p) { return (long long)p > p_cap ? (int)p_cap : p; };
    a.n_periods = (int)n_periods;
    a.min_period = 0;
    size_t rows = 0;
    for (size_t k = 0; k < n_periods; k++) {
        a.periods[k] = capped(ps[k]);
        if (ps[k] > 0 && (a.min_period == 0 || capped(ps[k]) < a.min_period)) a.min_period = capped(ps[k]);
        a.tab_off[k] = (int)std::min<size_t>(rows, (size_t)INT32_MAX);
        // a phase table only for a period some series can hold (p >= 2, 2 p <= t_rows); the kernels never run the others
        if (ps[k] >= 2 && (size_t)ps[k] <= t_rows / 2) rows += (size_t)ps[k];
    }
    a.trend = trend; a.remainder = remainder; a.seasonal = seasonal; a.info = info;
    hipStream_t st = (hipStream_t)stream;
    Scratch scratch;
    const bool ok = launch_and_wait("mstl", st, out_error, [&] {
        a.tab = rows ? scratch.get<double>(rows * ld) : nullptr;
        a.mean = scratch.get<double>((size_t)MSTL_MAX_PERIODS * ld);
        a.used = scratch.get<int32_t>(ld);
        launch_mstl(a, st);
    });
    if (ok) scratch.settled();
    return ok;
}

bool anofox_hip_mstl_decompose_batch(const double *const *values, const uint64_t *const *validity, const size_t *lengths, size_t n_series,
                                     const int *periods, size_t n_periods, int insufficient_data_mode, double *out_trend,
                                     double *out_seasonal, double *out_remainder, int32_t *out_periods, int32_t *out_applied,
                                     AnofoxError *out_errors, AnofoxError *out_batch_error)
{
    clear_error(out_batch_error);
    if ((n_series > 0 && (!values || !lengths || !out_applied)) || (n_periods > 0 && !periods)) {
        set_error(out_batch_error, NULL_POINTER, "Null pointer argument");
        return false;
    }
    BlockShape shape;
    if (!series_shape(values, validity, lengths, n_series, SIZE_MAX, &shape, out_batch_error)) return false;
    const size_t total = shape.total;
    if (total > 0 && (!out_trend || !out_remainder || (n_periods > 0 && !out_seasonal))) {
        set_error(out_batch_error, NULL_POINTER, "Null pointer argument");
        return false;
    }
    if (n_periods > (size_t)MSTL_MAX_PERIODS) {
        set_error(out_batch_error, COMPUTATION_ERROR, "Computation error: MSTL takes at most " + std::to_string(MSTL_MAX_PERIODS) +
                                                          " seasonal periods, got " + std::to_string(n_periods));
        return false;
    }
    if (n_series == 0) return true;
    const size_t ld = shape.ld, T = shape.T, K = n_periods;
    std::vector<int> ps(periods, periods + n_periods);
    std::sort(ps.begin(), ps.end(), std::greater<int>());
    int min_period = 0;
    for (int p : ps) if (p > 0 && (min_period == 0 || p < min_period)) min_period = p;
    // settled once the device entry has waited for its stream and the synchronous copies are back
    Scratch scratch;
    std::vector<int32_t> info(n_series);
    std::vector<double> trend, seas, rem;
    try {
        if (!device_ready(out_batch_error)) return false;
        // time-major block; a NULL counts as 0.0, as the reference's table function passes it (ts_mstl_decomposition_native.cpp:215)
        std::vector<double> yb(T * ld, 0.0);
        const std::vector<int32_t> len = block_lengths(lengths, n_series, ld);
        for (size_t s = 0; s < n_series; s++) {
            const uint64_t *m = validity ? validity[s] : nullptr;
            for (size_t t = 0; t < lengths[s]; t++) yb[t * ld + s] = (m && !valid_bit(m, t)) ? 0.0 : values[s][t];
        }
        double *d_y = scratch.get<double>(T * ld);
        int32_t *d_len = scratch.get<int32_t>(ld), *d_info = scratch.get<int32_t>(ld);
        double *d_trend = scratch.get<double>(T * ld), *d_rem = scratch.get<double>(T * ld);
        double *d_seas = scratch.get<double>(std::max<size_t>(K, 1) * T * ld);
        HIPCHECK(hipMemcpy(d_y, yb.data(), T * ld * sizeof(double), hipMemcpyHostToDevice));
        HIPCHECK(hipMemcpy(d_len, len.data(), ld * sizeof(int32_t), hipMemcpyHostToDevice));
        if (!anofox_hip_mstl_decompose_device(d_y, ld, d_len, n_series, T, ps.data(), K, insufficient_data_mode, d_trend, d_seas, d_rem,
                                              d_info, nullptr, out_batch_error))
            return false;
        trend.resize(T * ld); rem.resize(T * ld); seas.resize(K * T * ld);
        HIPCHECK(hipMemcpy(info.data(), d_info, n_series * sizeof(int32_t), hipMemcpyDeviceToHost));
        HIPCHECK(hipMemcpy(trend.data(), d_trend, T * ld * sizeof(double), hipMemcpyDeviceToHost));
        HIPCHECK(hipMemcpy(rem.data(), d_rem, T * ld * sizeof(double), hipMemcpyDeviceToHost));
        if (K) HIPCHECK(hipMemcpy(seas.data(), d_seas, K * T * ld * sizeof(double), hipMemcpyDeviceToHost));
        scratch.settled();
    } catch (const HipFail &f) {
        report_hip_failure(out_batch_error, f);
        return false;
    }
    // series i owns [off_i, off_i + lengths[i]) of every output; seasonal slot j holds the j-th component the series got
    const double nan = std::numeric_limits<double>::quiet_NaN();
    size_t off = 0;
    for (size_t s = 0; s < n_series; s++) {
        const size_t n = lengths[s];
        const int state = info[s] >> 8, used = info[s] & 0xff;
        if (out_errors) clear_error(&out_errors[s]);
        const bool applied = state == MSTL_APPLIED || state == MSTL_TREND_ONLY;
        out_applied[s] = applied ? 1 : 0;
        if (state == MSTL_FAILED && out_errors)
            set_error(&out_errors[s], COMPUTATION_ERROR, "Insufficient data: need at least " + std::to_string(n == 0 ? 1LL : 2LL * min_period) +
                                                             " observations, got " + std::to_string(n));
        for (size_t t = 0; t < n; t++) {
            out_trend[off + t] = applied ? trend[t * ld + s] : nan;
            out_remainder[off + t] = applied ? rem[t * ld + s] : nan;
        }
        size_t j = 0;
        for (size_t k = 0; k < K; k++) {
            if (!(state == MSTL_APPLIED && ((used >> k) & 1))) continue;
            for (size_t t = 0; t < n; t++) out_seasonal[j * total + off + t] = seas[(k * T + t) * ld + s];
            if (out_periods) out_periods[s * K + j] = ps[k];
            j++;
        }
        for (size_t jj = j; jj < K; jj++) {
            for (size_t t = 0; t < n; t++) out_seasonal[jj * total + off + t] = nan;
            if (out_periods) out_periods[s * K + jj] = 0;
        }
        off += n;
    }
    return true;
}

bool anofox_ts_mstl_decomposition(const double *values, size_t length, const int *periods, size_t n_periods, int insufficient_data_mode,
                                  MstlResult *out_result, AnofoxError *out_error)
{
    clear_error(out_error);
    if (!values || !out_result) { set_error(out_error, NULL_POINTER, "Null pointer argument"); return false; }
    const size_t K = (periods && n_periods) ? n_periods : 0;        // (lib.rs: a NULL list is no periods)
    std::vector<double> tr(std::max<size_t>(length, 1)), rm(std::max<size_t>(length, 1)), se(std::max<size_t>(K * length, 1));
    std::vector<int32_t> per(std::max<size_t>(K, 1), 0);
    int32_t applied = 0;
    AnofoxError serr, berr;
    const double *v[1] = {values};
    const size_t len[1] = {length};
    if (!anofox_hip_mstl_decompose_batch(v, nullptr, len, 1, K ? periods : nullptr, K, insufficient_data_mode, tr.data(), se.data(), rm.data(),
                                         per.data(), &applied, &serr, &berr)) {
        if (out_error) *out_error = berr;
        return false;
    }
    if (serr.code != SUCCESS) { if (out_error) *out_error = serr; return false; }
    std::memset(out_result, 0, sizeof *out_result);
    out_result->decomposition_applied = applied != 0;
    out_result->n_observations = length;
    if (!applied) return true;
    auto copy = [&](const double *src) -> double * {
        double *p = (double *)std::malloc(std::max<size_t>(length, 1) * sizeof(double));
        if (p && length) std::memcpy(p, src, length * sizeof(double));
        return p;
    };
    size_t ns = 0;
    while (ns < K && per[ns] != 0) ns++;
    bool ok = (out_result->trend = copy(tr.data())) && (out_result->remainder = copy(rm.data()));
    if (ok && ns) {
        out_result->seasonal_periods = (int *)std::malloc(ns * sizeof(int));
        out_result->seasonal_components = (double **)std::calloc(ns, sizeof(double *));
        ok = out_result->seasonal_periods && out_result->seasonal_components;
        for (size_t j = 0; ok && j < ns; j++) {
            out_result->seasonal_periods[j] = per[j];
            ok = (out_result->seasonal_components[j] = copy(se.data() + j * length)) != nullptr;
        }
        out_result->n_seasonal = ns;
    }
    if (!ok) {
        anofox_free_mstl_result(out_result);
        set_error(out_error, ALLOCATION_ERROR, "Failed to allocate MSTL result");
        return false;
    }
    return true;
}

void anofox_free_mstl_result(MstlResult *result)
{
    if (!result) return;
    std::free(result->trend);
    std::free(result->remainder);
    if (result->seasonal_components)
        for (size_t j = 0; j < result->n_seasonal; j++) std::free(result->seasonal_components[j]);
    std::free(result->seasonal_components);
    std::free(result->seasonal_periods);
    result->trend = result->remainder = nullptr;
    result->seasonal_components = nullptr;
    result->seasonal_periods = nullptr;
    result->n_seasonal = 0;
}

// ------------------------------------------------------------------------------------------------------------------------------
// Bayesian online changepoint detection (changepoint.rs detect_changepoints_bocpd; changepoint.hip)
// ------------------------------------------------------------------------------------------------------------------------------
bool anofox_hip_changepoints_device(const double *y, size_t ld, const int32_t *lengths, size_t n_series, size_t t_rows, double hazard_lambda,
                                    double *probability, uint8_t *flags, int32_t *counts, void *stream, AnofoxError *out_error)
{
    clear_error(out_error);
    if (!y || !lengths || !probability || !flags || !counts) {
        set_error(out_error, NULL_POINTER, "Null pointer argument");
        return false;
    }
    if (!block_args_ok(ld, n_series, "n_series", t_rows, (size_t)INT32_MAX, out_error)) return false;
    if (!device_ready(out_error)) return false;
    const double lambda = hazard_lambda > 0.0 ? hazard_lambda : 250.0;       // the FFI wrapper (lib.rs:3077-3081)
    ChangepointArgs a{};
    a.y = y; a.ld = ld; a.len = lengths; a.n_series = (int)n_series; a.t_rows = t_rows;
    a.hazard = 1.0 / std::fmax(lambda, 1.0);                                 // changepoint.rs:210
    a.prob = probability; a.flag = flags; a.count = counts;
    hipStream_t st = (hipStream_t)stream;
    return launch_and_wait("bocpd", st, out_error, [&] { launch_bocpd(a, st); });
}

bool anofox_hip_changepoints_batch(const double *const *values, const uint64_t *const *validity, const size_t *lengths, size_t n_series,
                                   double hazard_lambda, double *out_probability, uint8_t *out_is_changepoint, int32_t *out_n_changepoints,
                                   AnofoxError *out_errors, AnofoxError *out_batch_error)
{
    clear_error(out_batch_error);
    if (n_series > 0 && (!values || !lengths || !out_n_changepoints)) {
        set_error(out_batch_error, NULL_POINTER, "Null pointer argument");
        return false;
    }
    BlockShape shape;
    if (!series_shape(values, validity, lengths, n_series, (size_t)INT32_MAX, &shape, out_batch_error)) return false;
    if (shape.total > 0 && (!out_probability || !out_is_changepoint)) {
        set_error(out_batch_error, NULL_POINTER, "Null pointer argument");
        return false;
    }
    if (n_series == 0) return true;
    const size_t ld = shape.ld, T = shape.T;
    Scratch scratch;
    std::vector<int32_t> cnt(n_series);
    std::vector<double> prob;
    std::vector<uint8_t> flag;
    try {
        if (!device_ready(out_batch_error)) return false;
        // time-major block; a NULL counts as 0.0, as the reference's table function passes it (ts_changepoints.cpp:599)
        std::vector<double> yb(T * ld, 0.0);
        const std::vector<int32_t> len = block_lengths(lengths, n_series, ld);
        for (size_t s = 0; s < n_series; s++) {
            const uint64_t *m = validity ? validity[s] : nullptr;
            for (size_t t = 0; t < lengths[s]; t++) yb[t * ld + s] = (m && !valid_bit(m, t)) ? 0.0 : values[s][t];
        }
        double *d_y = scratch.get<double>(T * ld);
        int32_t *d_len = scratch.get<int32_t>(ld), *d_cnt = scratch.get<int32_t>(ld);
        double *d_prob = scratch.get<double>(T * ld);
        uint8_t *d_flag = scratch.get<uint8_t>(T * ld);
        HIPCHECK(hipMemcpy(d_y, yb.data(), T * ld * sizeof(double), hipMemcpyHostToDevice));
        HIPCHECK(hipMemcpy(d_len, len.data(), ld * sizeof(int32_t), hipMemcpyHostToDevice));
        if (!anofox_hip_changepoints_device(d_y, ld, d_len, n_series, T, hazard_lambda, d_prob, d_flag, d_cnt, nullptr, out_batch_error))
            return false;
        prob.resize(T * ld); flag.resize(T * ld);
        HIPCHECK(hipMemcpy(cnt.data(), d_cnt, n_series * sizeof(int32_t), hipMemcpyDeviceToHost));
        HIPCHECK(hipMemcpy(prob.data(), d_prob, T * ld * sizeof(double), hipMemcpyDeviceToHost));
        HIPCHECK(hipMemcpy(flag.data(), d_flag, T * ld * sizeof(uint8_t), hipMemcpyDeviceToHost));
        scratch.settled();
    } catch (const HipFail &f) {
        report_hip_failure(out_batch_error, f);
        return false;
    }
    const double nan = std::numeric_limits<double>::quiet_NaN();
    size_t off = 0;
    for (size_t s = 0; s < n_series; s++) {
        const size_t n = lengths[s];
        const bool ok = cnt[s] >= 0;
        if (out_errors) clear_error(&out_errors[s]);
        if (!ok && out_errors)      // ForecastError::InsufficientData { needed: 3, got: n } (changepoint.rs:205-207)
            set_error(&out_errors[s], COMPUTATION_ERROR, "Insufficient data: need at least 3 observations, got " + std::to_string(n));
        out_n_changepoints[s] = ok ? cnt[s] : -1;
        for (size_t t = 0; t < n; t++) {
            out_probability[off + t] = ok ? prob[t * ld + s] : nan;
            out_is_changepoint[off + t] = ok ? flag[t * ld + s] : 0;
        }
        off += n;
    }
    return true;
}

bool anofox_ts_detect_changepoints_bocpd(const double *values, size_t length, double hazard_lambda, bool include_probabilities,
                                         BocpdResult *out_result, AnofoxError *out_error)
{
    clear_error(out_error);
    if (!values || !out_result) { set_error(out_error, NULL_POINTER, "Null pointer argument"); return false; }
    std::vector<double> pr(std::max<size_t>(length, 1));
    std::vector<uint8_t> fl(std::max<size_t>(length, 1));
    int32_t n_cp = 0;
    AnofoxError serr, berr;
    const double *v[1] = {values};
    const size_t len[1] = {length};
    if (!anofox_hip_changepoints_batch(v, nullptr, len, 1, hazard_lambda, pr.data(), fl.data(), &n_cp, &serr, &berr)) {
        if (out_error) *out_error = berr;
        return false;
    }
    if (serr.code != SUCCESS) { if (out_error) *out_error = serr; return false; }
    std::memset(out_result, 0, sizeof *out_result);
    out_result->n_points = length;
    out_result->n_changepoints = (size_t)n_cp;
    out_result->is_changepoint = (bool *)std::malloc(length * sizeof(bool));
    out_result->changepoint_probability = (double *)std::calloc(length, sizeof(double));     // zeros unless asked for (changepoint.rs:347-349)
    if (n_cp > 0) out_result->changepoint_indices = (size_t *)std::malloc((size_t)n_cp * sizeof(size_t));
    if (!out_result->is_changepoint || !out_result->changepoint_probability || (n_cp > 0 && !out_result->changepoint_indices)) {
        anofox_free_bocpd_result(out_result);
        set_error(out_error, ALLOCATION_ERROR, "Failed to allocate BOCPD result");
        return false;
    }
    size_t k = 0;
    for (size_t t = 0; t < length; t++) {
        out_result->is_changepoint[t] = fl[t] != 0;
        if (include_probabilities) out_result->changepoint_probability[t] = pr[t];
        if (fl[t] && k < (size_t)n_cp) out_result->changepoint_indices[k++] = t;
    }
    return true;
}

void anofox_free_bocpd_result(BocpdResult *result)
{
    if (!result) return;
    std::free(result->is_changepoint);
    std::free(result->changepoint_probability);
    std::free(result->changepoint_indices);
    result->is_changepoint = nullptr;
    result->changepoint_probability = nullptr;
    result->changepoint_indices = nullptr;
    result->n_points = 0;
    result->n_changepoints = 0;
}

// ------------------------------------------------------------------------------------------------------------------------------
// Changepoints by the optimal-partitioning recurrence, L2 cost (changepoint.rs detect_changepoints, "PELT"; pelt.hip)
// ------------------------------------------------------------------------------------------------------------------------------
bool anofox_hip_pelt_device(const double *y, size_t ld, const int32_t *lengths, size_t n_series, size_t t_rows, int min_size, double penalty,
                            uint8_t *flags, int32_t *counts, double *cost, void *stream, AnofoxError *out_error)
{
    clear_error(out_error);
    if (!y || !lengths || !flags || !counts || !cost) {
        set_error(out_error, NULL_POINTER, "Null pointer argument");
        return false;
    }
    if (!block_args_ok(ld, n_series, "n_series", t_rows, PELT_MAX_ROWS, out_error)) return false;
    if (!device_ready(out_error)) return false;
    PeltArgs a{};
    a.y = y; a.ld = ld; a.len = lengths; a.n_series = (int)n_series; a.t_rows = t_rows;
    a.min_size = std::max<int64_t>((int64_t)min_size, 1);                    // the FFI wrapper: min_size.max(1) (lib.rs:3012)
    a.penalty = penalty;
    a.flag = flags; a.count = counts; a.cost = cost;
    a.resident = pelt_resident(t_rows);
    a.work_stride = pelt_work_stride(t_rows);
    a.work_groups = a.work_stride ? pelt_work_groups((int)n_series) : 0;
    // `if penalty > 0.0` (lib.rs:3009): NaN, zero and negative values take the default 2 ln n (changepoint.rs:118), rounded as the
    // host's libm rounds it -- what the source's f64::ln calls -- so it is a table by length, not a device logarithm
    // (kept per host thread and only ever extended, so that the batch-of-one entry does not pay t_rows logarithms per call)
    static thread_local std::vector<double> log_tab;
    const bool default_pen = !(penalty > 0.0);
    if (default_pen)
        for (size_t n = log_tab.size(); n <= t_rows; n++) log_tab.push_back(std::log((double)n) * 2.0);
    hipStream_t st = (hipStream_t)stream;
    Scratch scratch;
    const bool ok = launch_and_wait("pelt", st, out_error, [&] {
        if (default_pen) {
            double *d_tab = scratch.get<double>(t_rows + 1);
            HIPCHECK(hipMemcpyAsync(d_tab, log_tab.data(), (t_rows + 1) * sizeof(double), hipMemcpyHostToDevice, st));
            a.pen_tab = d_tab;
        }
        if (a.work_stride && a.work_groups > 0) a.work = scratch.get<double>(a.work_stride * (size_t)a.work_groups);
        launch_pelt(a, st);
    });
    if (ok) scratch.settled();
    return ok;
}

bool anofox_hip_pelt_batch(const double *const *values, const uint64_t *const *validity, const size_t *lengths, size_t n_series, int min_size,
                           double penalty, uint8_t *out_flags, int32_t *out_n_changepoints, double *out_cost, AnofoxError *out_errors,
                           AnofoxError *out_batch_error)
{
    clear_error(out_batch_error);
    if (n_series > 0 && (!values || !lengths || !out_n_changepoints || !out_cost)) {
        set_error(out_batch_error, NULL_POINTER, "Null pointer argument");
        return false;
    }
    BlockShape shape;
    if (!series_shape(values, validity, lengths, n_series, PELT_MAX_ROWS, &shape, out_batch_error)) return false;
    if (shape.total > 0 && !out_flags) {
        set_error(out_batch_error, NULL_POINTER, "Null pointer argument");
        return false;
    }
    if (n_series == 0) return true;
    // a NULL value is DROPPED before the series is packed, as ExtractListAsDouble does for the scalar (ts_changepoints.cpp:45-50)
    std::vector<std::vector<double>> kept(n_series);
    std::vector<const double *> rows(n_series);
    std::vector<size_t> packed(n_series);
    size_t T = 1;
    for (size_t s = 0; s < n_series; s++) {
        const uint64_t *m = validity ? validity[s] : nullptr;
        rows[s] = values[s];
        packed[s] = lengths[s];
        if (m && lengths[s] > 0) {
            kept[s].reserve(lengths[s]);
            for (size_t t = 0; t < lengths[s]; t++)
                if (valid_bit(m, t)) kept[s].push_back(values[s][t]);
            rows[s] = kept[s].data();
            packed[s] = kept[s].size();
        }
        T = std::max(T, packed[s]);
    }
    const size_t ld = shape.ld;
    Scratch scratch;
    std::vector<int32_t> cnt(n_series);
    std::vector<uint8_t> flag;
    try {
        if (!device_ready(out_batch_error)) return false;
        std::vector<double> yb(T * ld, 0.0);
        pack_time_major(yb.data(), ld, rows.data(), packed.data(), n_series);
        const std::vector<int32_t> len = block_lengths(packed.data(), n_series, ld);
        double *d_y = scratch.get<double>(T * ld);
        int32_t *d_len = scratch.get<int32_t>(ld), *d_cnt = scratch.get<int32_t>(ld);
        double *d_cost = scratch.get<double>(ld);
        uint8_t *d_flag = scratch.get<uint8_t>(T * ld);
        HIPCHECK(hipMemcpy(d_y, yb.data(), T * ld * sizeof(double), hipMemcpyHostToDevice));
        HIPCHECK(hipMemcpy(d_len, len.data(), ld * sizeof(int32_t), hipMemcpyHostToDevice));
        if (!anofox_hip_pelt_device(d_y, ld, d_len, n_series, T, min_size, penalty, d_flag, d_cnt, d_cost, nullptr, out_batch_error))
            return false;
        flag.resize(T * ld);
        HIPCHECK(hipMemcpy(cnt.data(), d_cnt, n_series * sizeof(int32_t), hipMemcpyDeviceToHost));
        HIPCHECK(hipMemcpy(out_cost, d_cost, n_series * sizeof(double), hipMemcpyDeviceToHost));
        HIPCHECK(hipMemcpy(flag.data(), d_flag, T * ld * sizeof(uint8_t), hipMemcpyDeviceToHost));
        scratch.settled();
    } catch (const HipFail &f) {
        report_hip_failure(out_batch_error, f);
        return false;
    }
    // flags by position in the PACKED series; the positions a series lost to its NULLs (the tail of its range) are 0
    size_t off = 0;
    for (size_t s = 0; s < n_series; s++) {
        if (out_errors) clear_error(&out_errors[s]);
        out_n_changepoints[s] = cnt[s];
        for (size_t t = 0; t < lengths[s]; t++) out_flags[off + t] = t < packed[s] ? flag[t * ld + s] : 0;
        off += lengths[s];
    }
    return true;
}

bool anofox_ts_detect_changepoints(const double *values, size_t length, int min_size, double penalty, ChangepointResult *out_result,
                                   AnofoxError *out_error)
{
    clear_error(out_error);
    if (!values || !out_result) { set_error(out_error, NULL_POINTER, "Null pointer argument"); return false; }
    std::vector<uint8_t> fl(std::max<size_t>(length, 1));
    int32_t n_cp = 0;
    double cost = 0.0;
    AnofoxError berr;
    const double *v[1] = {values};
    const size_t len[1] = {length};
    if (!anofox_hip_pelt_batch(v, nullptr, len, 1, min_size, penalty, fl.data(), &n_cp, &cost, nullptr, &berr)) {
        if (out_error) *out_error = berr;
        return false;
    }
    out_result->changepoints = nullptr;
    out_result->n_changepoints = (size_t)n_cp;
    out_result->cost = cost;
    if (n_cp > 0) {
        out_result->changepoints = (size_t *)std::malloc((size_t)n_cp * sizeof(size_t));
        if (!out_result->changepoints) {
            out_result->n_changepoints = 0;
            set_error(out_error, ALLOCATION_ERROR, "Failed to allocate changepoint result");
            return false;
        }
        size_t k = 0;
        for (size_t t = 0; t < length && k < (size_t)n_cp; t++)
            if (fl[t]) out_result->changepoints[k++] = t;
    }
    return true;
}

void anofox_free_changepoint_result(ChangepointResult *result)
{
    if (!result) return;
    std::free(result->changepoints);
    result->changepoints = nullptr;
    result->n_changepoints = 0;
}

// ------------------------------------------------------------------------------------------------------------------------------
// Per-series statistics (stats.rs compute_ts_stats_with_dates_and_type; stats.hip)
// ------------------------------------------------------------------------------------------------------------------------------
static_assert(sizeof(TsStatsResult) == 296 && offsetof(TsStatsResult, n_zeros_start) == 64 && offsetof(TsStatsResult, mean) == 96 &&
              offsetof(TsStatsResult, expected_length) == 272 && offsetof(TsStatsResult, has_date_metrics) == 288, "TsStatsResult layout");

bool anofox_hip_stats_device(const double *y, const uint8_t *valid, const int64_t *dates, size_t ld, const int32_t *lengths, size_t n_series,
                             size_t t_rows, int64_t frequency_micros, FrequencyType frequency_type, int64_t *out_int, double *out_fp,
                             void *stream, AnofoxError *out_error)
{
    clear_error(out_error);
    if (!y || !lengths || !out_int || !out_fp) {
        set_error(out_error, NULL_POINTER, "Null pointer argument");
        return false;
    }
    if (!block_args_ok(ld, n_series, "n_series", t_rows, (size_t)1 << 30, out_error)) return false;
    if ((int)frequency_type < STATS_FREQ_FIXED || (int)frequency_type > STATS_FREQ_YEARLY) {
        set_error(out_error, INVALID_INPUT, "Invalid input: unknown frequency type");
        return false;
    }
    if (!device_ready(out_error)) return false;
    StatsArgs a{};
    a.y = y; a.valid = valid; a.dates = dates; a.ld = ld; a.len = lengths; a.n_series = (int)n_series; a.t_rows = t_rows;
    a.freq_us = frequency_micros; a.freq_type = (int)frequency_type;
    a.out_int = out_int; a.out_fp = out_fp;
    a.work_stride = stats_work_stride(t_rows);
    a.work_waves = a.work_stride ? stats_work_waves((int)n_series) : 0;
    hipStream_t st = (hipStream_t)stream;
    Scratch scratch;
    const bool ok = launch_and_wait("stats", st, out_error, [&] {
        if (a.work_stride && a.work_waves > 0) a.work = scratch.get<uint64_t>(a.work_stride * (size_t)a.work_waves);
        launch_stats(a, st);
    });
    if (ok) scratch.settled();
    return ok;
}

bool anofox_hip_stats_batch(const double *const *values, const uint64_t *const *validity, const int64_t *const *dates, const size_t *lengths,
                            size_t n_series, int64_t frequency_micros, FrequencyType frequency_type, TsStatsResult *out_results,
                            AnofoxError *out_batch_error)
{
    clear_error(out_batch_error);
    if (n_series > 0 && (!values || !lengths || !out_results)) {
        set_error(out_batch_error, NULL_POINTER, "Null pointer argument");
        return false;
    }
    BlockShape shape;
    if (!series_shape(values, validity, lengths, n_series, (size_t)1 << 30, &shape, out_batch_error)) return false;
    bool any_dates = false;
    for (size_t s = 0; s < n_series; s++) any_dates = any_dates || (dates && dates[s] && lengths[s] > 0);
    if (n_series == 0) return true;
    const size_t ld = shape.ld, T = shape.T;
    const bool any_mask = shape.any_mask;
    Scratch scratch;
    std::vector<int64_t> oi(STATS_N_INT * ld);
    std::vector<double> of(STATS_N_FP * ld);
    try {
        if (!device_ready(out_batch_error)) return false;
        std::vector<double> yb(T * ld, 0.0);
        std::vector<uint8_t> vb(any_mask ? T * ld : 0, 1);
        std::vector<int64_t> db(any_dates ? T * ld : 0, 0);
        const std::vector<int32_t> len = block_lengths(lengths, n_series, ld);
        pack_time_major(yb.data(), ld, values, lengths, n_series);
        if (any_mask) pack_validity(vb.data(), ld, validity, lengths, n_series);
        if (any_dates) pack_time_major(db.data(), ld, dates, lengths, n_series);
        double *d_y = scratch.get<double>(T * ld);
        int32_t *d_len = scratch.get<int32_t>(ld);
        int64_t *d_int = scratch.get<int64_t>(STATS_N_INT * ld), *d_dates = nullptr;
        double *d_fp = scratch.get<double>(STATS_N_FP * ld);
        uint8_t *d_valid = nullptr;
        HIPCHECK(hipMemcpy(d_y, yb.data(), T * ld * sizeof(double), hipMemcpyHostToDevice));
        HIPCHECK(hipMemcpy(d_len, len.data(), ld * sizeof(int32_t), hipMemcpyHostToDevice));
        if (any_mask) {
            d_valid = scratch.get<uint8_t>(T * ld);
            HIPCHECK(hipMemcpy(d_valid, vb.data(), T * ld, hipMemcpyHostToDevice));
        }
        if (any_dates) {
            d_dates = scratch.get<int64_t>(T * ld);
            HIPCHECK(hipMemcpy(d_dates, db.data(), T * ld * sizeof(int64_t), hipMemcpyHostToDevice));
        }
        if (!anofox_hip_stats_device(d_y, d_valid, d_dates, ld, d_len, n_series, T, frequency_micros, frequency_type, d_int, d_fp, nullptr,
                                     out_batch_error))
            return false;
        HIPCHECK(hipMemcpy(oi.data(), d_int, oi.size() * sizeof(int64_t), hipMemcpyDeviceToHost));
        HIPCHECK(hipMemcpy(of.data(), d_fp, of.size() * sizeof(double), hipMemcpyDeviceToHost));
        scratch.settled();
    } catch (const HipFail &f) {
        report_hip_failure(out_batch_error, f);
        return false;
    }
    for (size_t s = 0; s < n_series; s++) {
        TsStatsResult &r = out_results[s];
        std::memset(&r, 0, sizeof r);
        size_t *cnt[12] = {&r.length, &r.n_nulls, &r.n_nan, &r.n_zeros, &r.n_positive, &r.n_negative, &r.n_unique_values, nullptr,
                           &r.n_zeros_start, &r.n_zeros_end, &r.plateau_size, &r.plateau_size_nonzero};
        for (int i = 0; i < 12; i++)
            if (cnt[i]) *cnt[i] = (size_t)oi[i * ld + s];
        r.is_constant = oi[7 * ld + s] != 0;
        double *fp = &r.mean;                                     // 22 consecutive doubles, mean .. stability
        for (int i = 0; i < STATS_N_FP; i++) fp[i] = of[i * ld + s];
        // has_date_metrics as the source sets it (stats.rs:322-359): dates given, and not the FIXED rule with a frequency <= 0 on
        // two or more dates
        const size_t n = lengths[s];
        const bool dated = dates && dates[s] && n > 0 && (n < 2 || frequency_type != FIXED || frequency_micros > 0);
        r.has_date_metrics = dated;
        r.expected_length = dated ? (size_t)oi[12 * ld + s] : 0;
        r.n_gaps = dated ? (size_t)oi[13 * ld + s] : 0;
    }
    return true;
}

bool anofox_ts_stats_with_dates_and_type(const double *values, const uint64_t *validity, const int64_t *dates, size_t length,
                                         int64_t frequency_micros, FrequencyType frequency_type, TsStatsResult *out_result,
                                         AnofoxError *out_error)
{
    clear_error(out_error);
    if (!values || !dates || !out_result) { set_error(out_error, NULL_POINTER, "Null pointer argument"); return false; }
    const double *v[1] = {values};
    const uint64_t *m[1] = {validity};
    const int64_t *d[1] = {dates};
    const size_t len[1] = {length};
    return anofox_hip_stats_batch(v, m, d, len, 1, frequency_micros, frequency_type, out_result, out_error);
}

bool anofox_ts_stats_with_dates(const double *values, const uint64_t *validity, const int64_t *dates, size_t length, int64_t frequency_micros,
                                TsStatsResult *out_result, AnofoxError *out_error)
{
    return anofox_ts_stats_with_dates_and_type(values, validity, dates, length, frequency_micros, FIXED, out_result, out_error);
}

bool anofox_ts_stats(const double *values, const uint64_t *validity, size_t length, TsStatsResult *out_result, AnofoxError *out_error)
{
    clear_error(out_error);
    if (!values || !out_result) { set_error(out_error, NULL_POINTER, "Null pointer argument"); return false; }
    const double *v[1] = {values};
    const uint64_t *m[1] = {validity};
    const size_t len[1] = {length};
    return anofox_hip_stats_batch(v, m, nullptr, len, 1, 0, FIXED, out_result, out_error);
}

void anofox_free_ts_stats_result(TsStatsResult *result) { (void)result; }      // the struct owns no memory (as the reference's)

// ------------------------------------------------------------------------------------------------------------------------------
// Data quality per series (quality.rs compute_data_quality without dates; quality.hip)
// ------------------------------------------------------------------------------------------------------------------------------
static_assert(sizeof(DataQualityResult) == 64 && offsetof(DataQualityResult, overall_score) == 32 && offsetof(DataQualityResult, n_gaps) == 40 &&
              offsetof(DataQualityResult, n_missing) == 48 && offsetof(DataQualityResult, is_constant) == 56, "DataQualityResult layout");
static const char *const QUALITY_NAN_TEXT = "Invalid input: a value is NaN";

bool anofox_hip_quality_device(const double *y, const uint8_t *valid, size_t ld, const int32_t *lengths, size_t n_series, size_t t_rows,
                               double *out_fp, int64_t *out_int, void *stream, AnofoxError *out_error)
{
    clear_error(out_error);
    if (!y || !lengths || !out_fp || !out_int) {
        set_error(out_error, NULL_POINTER, "Null pointer argument");
        return false;
    }
    if (!block_args_ok(ld, n_series, "n_series", t_rows, (size_t)1 << 30, out_error)) return false;
    if (n_series == 0) return true;
    if (!device_ready(out_error)) return false;
    QualityArgs a{};
    a.y = y; a.valid = valid; a.ld = ld; a.len = lengths; a.n_series = (int)n_series; a.t_rows = t_rows;
    a.out_fp = out_fp; a.out_int = out_int;
    a.tile = quality_tile(t_rows);
    a.work_stride = quality_work_stride(t_rows);
    a.work_waves = a.work_stride ? quality_work_waves((int)n_series) : 0;
    hipStream_t st = (hipStream_t)stream;
    Scratch scratch;
    const bool ok = launch_and_wait("quality", st, out_error, [&] {
        if (a.work_stride && a.work_waves > 0) a.work = scratch.get<uint64_t>(a.work_stride * (size_t)a.work_waves);
        launch_quality(a, st);
    });
    if (ok) scratch.settled();
    return ok;
}

bool anofox_hip_quality_batch(const double *const *values, const uint64_t *const *validity, const size_t *lengths, size_t n_series,
                              DataQualityResult *out_results, int32_t *out_status, AnofoxError *out_batch_error)
{
    clear_error(out_batch_error);
    if (n_series > 0 && (!values || !lengths || !out_results)) {
        set_error(out_batch_error, NULL_POINTER, "Null pointer argument");
        return false;
    }
    BlockShape shape;
    if (!series_shape(values, validity, lengths, n_series, (size_t)1 << 30, &shape, out_batch_error)) return false;
    if (n_series == 0) return true;
    const size_t ld = shape.ld, T = shape.T;
    const bool any_mask = shape.any_mask;
    Scratch scratch;
    std::vector<int64_t> oi(QUALITY_N_INT * ld);
    std::vector<double> of(QUALITY_N_FP * ld);
    try {
        if (!device_ready(out_batch_error)) return false;
        std::vector<double> yb(T * ld, 0.0);
        std::vector<uint8_t> vb(any_mask ? T * ld : 0, 1);
        const std::vector<int32_t> len = block_lengths(lengths, n_series, ld);
        pack_time_major(yb.data(), ld, values, lengths, n_series);
        if (any_mask) pack_validity(vb.data(), ld, validity, lengths, n_series);
        double *d_y = scratch.get<double>(T * ld);
        int32_t *d_len = scratch.get<int32_t>(ld);
        int64_t *d_int = scratch.get<int64_t>(QUALITY_N_INT * ld);
        double *d_fp = scratch.get<double>(QUALITY_N_FP * ld);
        uint8_t *d_valid = nullptr;
        HIPCHECK(hipMemcpy(d_y, yb.data(), T * ld * sizeof(double), hipMemcpyHostToDevice));
        HIPCHECK(hipMemcpy(d_len, len.data(), ld * sizeof(int32_t), hipMemcpyHostToDevice));
        if (any_mask) {
            d_valid = scratch.get<uint8_t>(T * ld);
            HIPCHECK(hipMemcpy(d_valid, vb.data(), T * ld, hipMemcpyHostToDevice));
        }
        if (!anofox_hip_quality_device(d_y, d_valid, ld, d_len, n_series, T, d_fp, d_int, nullptr, out_batch_error)) return false;
        HIPCHECK(hipMemcpy(oi.data(), d_int, oi.size() * sizeof(int64_t), hipMemcpyDeviceToHost));
        HIPCHECK(hipMemcpy(of.data(), d_fp, of.size() * sizeof(double), hipMemcpyDeviceToHost));
        scratch.settled();
    } catch (const HipFail &f) {
        report_hip_failure(out_batch_error, f);
        return false;
    }
    for (size_t s = 0; s < n_series; s++) {
        DataQualityResult &r = out_results[s];
        std::memset(&r, 0, sizeof r);
        double *fp = &r.structural_score;                         // five consecutive doubles, structural .. overall
        for (int i = 0; i < QUALITY_N_FP; i++) fp[i] = of[i * ld + s];
        r.n_gaps = (size_t)oi[0 * ld + s];
        r.n_missing = (size_t)oi[1 * ld + s];
        r.is_constant = oi[2 * ld + s] != 0;
        if (out_status) out_status[s] = (int32_t)oi[3 * ld + s];
    }
    return true;
}

bool anofox_ts_data_quality(const double *values, const uint64_t *validity, size_t length, DataQualityResult *out_result, AnofoxError *out_error)
{
    clear_error(out_error);
    if (!values || !out_result) { set_error(out_error, NULL_POINTER, "Null pointer argument"); return false; }
    const double *v[1] = {values};
    const uint64_t *m[1] = {validity};
    const size_t len[1] = {length};
    DataQualityResult r;
    int32_t status = 0;
    if (!anofox_hip_quality_batch(v, m, len, 1, &r, &status, out_error)) return false;
    if (status == (int32_t)QUALITY_NAN) { set_error(out_error, COMPUTATION_ERROR, QUALITY_NAN_TEXT); return false; }
    *out_result = r;
    return true;
}

// ------------------------------------------------------------------------------------------------------------------------------
// The 117 features per series (features.rs extract_features; features.hip)
// ------------------------------------------------------------------------------------------------------------------------------
static_assert(sizeof(FeaturesResult) == 24 && offsetof(FeaturesResult, feature_names) == 8 && offsetof(FeaturesResult, n_features) == 16,
              "FeaturesResult layout");
static_assert(ANOFOX_HIP_N_FEATURES == FEATURES_N && ANOFOX_HIP_FEATURES_MAX_ROWS == FEATURES_MAX_ROWS, "the header's feature constants");
static const char *const FEATURES_TOO_LONG_TEXT = "Invalid input: a series has more than 65536 rows, the limit of the feature kernels";

// the names in byte order (the rows of the kernels) and in the order of the source's list_features
static const char *const FEATURE_NAMES_SORTED[FEATURES_N] = {
#define X(id, name, pos) name,
#include "feature_names.inc"
#undef X
};
static const int FEATURE_LIST_POS[FEATURES_N] = {
#define X(id, name, pos) pos,
#include "feature_names.inc"
#undef X
};

// the thresholds dEk (d = 1 .. 9, k = 0 .. 308) as strtod rounds them, ascending: Rust's shortest round-trip to_string() of v >= 1
// starts with d exactly when strtod("dEk") <= v < strtod("(d+1)Ek")
static const std::vector<double> &benford_thresholds()
{
    static const std::vector<double> table = [] {
        std::vector<double> t;
        t.reserve(FEATURES_BENFORD);
        char text[16];
        for (int k = 0; k < 309; k++)
            for (int d = 1; d <= 9; d++) {
                std::snprintf(text, sizeof text, "%de%d", d, k);
                t.push_back(std::strtod(text, nullptr));
            }
        return t;
    }();
    return table;
}

static char *c_string_copy(const std::string &s)
{
    char *p = (char *)std::malloc(s.size() + 1);
    if (p) std::memcpy(p, s.c_str(), s.size() + 1);
    return p;
}

bool anofox_hip_features_families_device(const double *y, const uint8_t *valid, size_t ld, const int32_t *lengths, size_t n_series, size_t t_rows,
                                         unsigned families, double *out_fp, int64_t *out_int, void *stream, AnofoxError *out_error)
{
    clear_error(out_error);
    if (!y || !lengths || !out_fp || !out_int) {
        set_error(out_error, NULL_POINTER, "Null pointer argument");
        return false;
    }
    if (t_rows > FEATURES_MAX_ROWS) { set_error(out_error, INVALID_INPUT, FEATURES_TOO_LONG_TEXT); return false; }
    if (!block_args_ok(ld, n_series, "n_series", t_rows, FEATURES_MAX_ROWS, out_error)) return false;
    if (n_series == 0) return true;
    if (!device_ready(out_error)) return false;
    FeaturesArgs a{};
    a.y = y; a.valid = valid; a.ld = ld; a.len = lengths; a.n_series = (int)n_series; a.t_rows = t_rows;
    a.out_fp = out_fp; a.out_int = out_int;
    a.tile = features_tile(t_rows);
    a.work_stride = features_work_stride(t_rows);
    a.work_waves = a.work_stride ? features_work_waves((int)n_series) : 0;
    hipStream_t st = (hipStream_t)stream;
    Scratch scratch;
    const std::vector<double> &table = benford_thresholds();
    const bool ok = launch_and_wait("features", st, out_error, [&] {
        double *d_table = scratch.get<double>(FEATURES_BENFORD);
        HIPCHECK(hipMemcpyAsync(d_table, table.data(), FEATURES_BENFORD * sizeof(double), hipMemcpyHostToDevice, st));
        a.benford = d_table;
        if (a.work_stride && a.work_waves > 0) a.work = scratch.get<uint64_t>(2 * a.work_stride * (size_t)a.work_waves);
        launch_features(a, st, (int)(families & ((1u << FEATURES_FAMILIES) - 1u)));
    });
    if (ok) scratch.settled();
    return ok;
}

bool anofox_hip_features_device(const double *y, const uint8_t *valid, size_t ld, const int32_t *lengths, size_t n_series, size_t t_rows,
                                double *out_fp, int64_t *out_int, void *stream, AnofoxError *out_error)
{
    return anofox_hip_features_families_device(y, valid, ld, lengths, n_series, t_rows, (1u << FEATURES_FAMILIES) - 1u, out_fp, out_int, stream,
                                               out_error);
}

bool anofox_hip_features_batch(const double *const *values, const uint64_t *const *validity, const size_t *lengths, size_t n_series,
                               double *out_features, uint64_t *out_present, int32_t *out_status, AnofoxError *out_batch_error)
{
    clear_error(out_batch_error);
    if (n_series > 0 && (!values || !lengths || !out_features || !out_present)) {
        set_error(out_batch_error, NULL_POINTER, "Null pointer argument");
        return false;
    }
    for (size_t s = 0; s < n_series; s++)
        if (lengths[s] > FEATURES_MAX_ROWS) { set_error(out_batch_error, INVALID_INPUT, FEATURES_TOO_LONG_TEXT); return false; }
    BlockShape shape;
    if (!series_shape(values, validity, lengths, n_series, FEATURES_MAX_ROWS, &shape, out_batch_error)) return false;
    if (n_series == 0) return true;
    const size_t ld = shape.ld, T = shape.T;
    const bool any_mask = shape.any_mask;
    Scratch scratch;
    std::vector<int64_t> oi(FEATURES_N_INT * ld);
    std::vector<double> of((size_t)FEATURES_N * ld);
    try {
        if (!device_ready(out_batch_error)) return false;
        std::vector<double> yb(T * ld, 0.0);
        std::vector<uint8_t> vb(any_mask ? T * ld : 0, 1);
        const std::vector<int32_t> len = block_lengths(lengths, n_series, ld);
        pack_time_major(yb.data(), ld, values, lengths, n_series);
        if (any_mask) pack_validity(vb.data(), ld, validity, lengths, n_series);
        double *d_y = scratch.get<double>(T * ld);
        int32_t *d_len = scratch.get<int32_t>(ld);
        int64_t *d_int = scratch.get<int64_t>(FEATURES_N_INT * ld);
        double *d_fp = scratch.get<double>((size_t)FEATURES_N * ld);
        uint8_t *d_valid = nullptr;
        HIPCHECK(hipMemcpy(d_y, yb.data(), T * ld * sizeof(double), hipMemcpyHostToDevice));
        HIPCHECK(hipMemcpy(d_len, len.data(), ld * sizeof(int32_t), hipMemcpyHostToDevice));
        if (any_mask) {
            d_valid = scratch.get<uint8_t>(T * ld);
            HIPCHECK(hipMemcpy(d_valid, vb.data(), T * ld, hipMemcpyHostToDevice));
        }
        if (!anofox_hip_features_device(d_y, d_valid, ld, d_len, n_series, T, d_fp, d_int, nullptr, out_batch_error)) return false;
        HIPCHECK(hipMemcpy(oi.data(), d_int, oi.size() * sizeof(int64_t), hipMemcpyDeviceToHost));
        HIPCHECK(hipMemcpy(of.data(), d_fp, of.size() * sizeof(double), hipMemcpyDeviceToHost));
        scratch.settled();
    } catch (const HipFail &f) {
        report_hip_failure(out_batch_error, f);
        return false;
    }
    for (size_t s = 0; s < n_series; s++) {
        for (int i = 0; i < FEATURES_N; i++) out_features[s * FEATURES_N + i] = of[(size_t)i * ld + s];
        out_present[2 * s] = (uint64_t)oi[0 * ld + s];
        out_present[2 * s + 1] = (uint64_t)oi[1 * ld + s];
        if (out_status) out_status[s] = (int32_t)oi[2 * ld + s];
    }
    return true;
}

bool anofox_ts_features(const double *values, size_t length, FeaturesResult *out_result, AnofoxError *out_error)
{
    clear_error(out_error);
    if (!values || !out_result) { set_error(out_error, NULL_POINTER, "Null pointer argument"); return false; }
    if (length == 0) { set_error(out_error, COMPUTATION_ERROR, "Insufficient data: need at least 1 observations, got 0"); return false; }
    const double *v[1] = {values};
    const size_t len[1] = {length};
    std::vector<double> f(FEATURES_N);
    uint64_t present[2] = {0, 0};
    int32_t status = 0;
    if (!anofox_hip_features_batch(v, nullptr, len, 1, f.data(), present, &status, out_error)) return false;
    if (status == (int32_t)FEATURES_NAN) { set_error(out_error, COMPUTATION_ERROR, QUALITY_NAN_TEXT); return false; }
    const size_t n = (size_t)(__builtin_popcountll(present[0]) + __builtin_popcountll(present[1]));
    out_result->n_features = n;
    out_result->features = nullptr;
    out_result->feature_names = nullptr;
    if (n == 0) return true;
    double *fp = (double *)std::malloc(n * sizeof(double));
    char **names = (char **)std::calloc(n, sizeof(char *));
    if (!fp || !names) {
        std::free(fp); std::free(names);
        out_result->n_features = 0;
        set_error(out_error, ALLOCATION_ERROR, "Allocation failed");
        return false;
    }
    size_t j = 0;
    for (int i = 0; i < FEATURES_N; i++)
        if ((present[i >> 6] >> (i & 63)) & 1ull) {
            fp[j] = f[i];
            names[j++] = c_string_copy(FEATURE_NAMES_SORTED[i]);
        }
    out_result->features = fp;
    out_result->feature_names = names;
    return true;
}

void anofox_free_features_result(FeaturesResult *result)
{
    if (!result) return;
    if (result->feature_names)
        for (size_t i = 0; i < result->n_features; i++) std::free(result->feature_names[i]);
    std::free(result->feature_names);
    std::free(result->features);
    result->features = nullptr;
    result->feature_names = nullptr;
    result->n_features = 0;
}

bool anofox_ts_features_list(char **out_names, size_t *out_count)
{
    if (!out_names || !out_count) return false;
    char **names = (char **)std::calloc(FEATURES_N, sizeof(char *));
    if (!names) return false;
    for (int i = 0; i < FEATURES_N; i++) names[FEATURE_LIST_POS[i]] = c_string_copy(FEATURE_NAMES_SORTED[i]);
    *out_count = FEATURES_N;
    *out_names = (char *)names;                               // (the reference's cast: the caller reads a char ** out of it)
    return true;
}

bool anofox_ts_validate_feature_params(const char *const *param_names, size_t n_params, char ***out_warnings, size_t *out_n_warnings)
{
    if (!param_names || !out_warnings || !out_n_warnings) return false;
    std::vector<std::string> warnings;
    for (size_t i = 0; i < n_params; i++) {
        if (!param_names[i]) continue;
        bool known = false;
        for (int f = 0; f < FEATURES_N && !known; f++) known = std::strcmp(param_names[i], FEATURE_NAMES_SORTED[f]) == 0;
        if (!known) warnings.push_back(std::string("Unknown feature parameter key '") + param_names[i] + "' - this parameter will be ignored");
    }
    *out_n_warnings = warnings.size();
    *out_warnings = nullptr;
    if (warnings.empty()) return true;
    char **w = (char **)std::calloc(warnings.size(), sizeof(char *));
    if (!w) return false;
    for (size_t i = 0; i < warnings.size(); i++) w[i] = c_string_copy(warnings[i]);
    *out_warnings = w;
    return true;
}

void anofox_free_warnings(char **warnings, size_t n_warnings)
{
    if (!warnings) return;
    for (size_t i = 0; i < n_warnings; i++) std::free(warnings[i]);
    std::free(warnings);
}

// ------------------------------------------------------------------------------------------------------------------------------
// Seasonality analysis per series (seasonality.rs detect_seasonality / analyze_seasonality / compute_trend_strength; seasonality.hip)
// ------------------------------------------------------------------------------------------------------------------------------
static_assert(sizeof(SeasonalityResult) == 40 && offsetof(SeasonalityResult, n_periods) == 8 && offsetof(SeasonalityResult, primary_period) == 16 &&
              offsetof(SeasonalityResult, seasonal_strength) == 24 && offsetof(SeasonalityResult, trend_strength) == 32, "SeasonalityResult layout");
static_assert(sizeof(AnofoxHipSeasonality) == 128 && offsetof(AnofoxHipSeasonality, n_periods) == 20 && offsetof(AnofoxHipSeasonality, primary_period) == 24 &&
              offsetof(AnofoxHipSeasonality, strengths) == 32 && offsetof(AnofoxHipSeasonality, acf) == 72 &&
              offsetof(AnofoxHipSeasonality, seasonal_strength) == 112 && offsetof(AnofoxHipSeasonality, trend_strength) == 120, "AnofoxHipSeasonality layout");

bool anofox_hip_seasonality_device(const double *y, const uint8_t *valid, size_t ld, const int32_t *lengths, size_t n_series, size_t t_rows,
                                   int max_period, int32_t *out_int, double *out_fp, void *stream, AnofoxError *out_error)
{
    clear_error(out_error);
    if (!y || !lengths || !out_fp || !out_int) {
        set_error(out_error, NULL_POINTER, "Null pointer argument");
        return false;
    }
    if (!block_args_ok(ld, n_series, "n_series", t_rows, (size_t)1 << 30, out_error)) return false;
    if (n_series == 0) return true;
    if (!device_ready(out_error)) return false;
    SeasonalityArgs a{};
    a.y = y; a.valid = valid; a.ld = ld; a.len = lengths; a.n_series = (int)n_series; a.t_rows = (int)t_rows;
    a.max_period = max_period; a.out_int = out_int; a.out_fp = out_fp;
    hipStream_t st = (hipStream_t)stream;
    Scratch scratch;
    try {
        const bool ok = launch_and_wait("seasonality", st, out_error, [&] {
            const size_t need = seasonality_work_doubles(a.n_series, a.t_rows);
            if (need) a.work = scratch.get<double>(need);
            launch_seasonality(a, st);
        });
        if (ok) scratch.settled();
        return ok;
    } catch (const std::runtime_error &e) {
        set_error(out_error, COMPUTATION_ERROR, e.what());
        return false;
    }
}

bool anofox_hip_seasonality_batch(const double *const *values, const uint64_t *const *validity, const size_t *lengths, size_t n_series,
                                  int max_period, AnofoxHipSeasonality *out_results, int32_t *out_status, AnofoxError *out_batch_error)
{
    clear_error(out_batch_error);
    if (n_series > 0 && (!values || !lengths || !out_results)) {
        set_error(out_batch_error, NULL_POINTER, "Null pointer argument");
        return false;
    }
    BlockShape shape;
    if (!series_shape(values, validity, lengths, n_series, (size_t)1 << 30, &shape, out_batch_error)) return false;
    if (n_series == 0) return true;
    const size_t ld = shape.ld, T = shape.T;
    const bool any_mask = shape.any_mask;
    Scratch scratch;
    std::vector<int32_t> oi(SEASONALITY_N_INT * ld);
    std::vector<double> of(SEASONALITY_N_FP * ld);
    try {
        if (!device_ready(out_batch_error)) return false;
        std::vector<double> yb(T * ld, 0.0);
        std::vector<uint8_t> vb(any_mask ? T * ld : 0, 1);
        const std::vector<int32_t> len = block_lengths(lengths, n_series, ld);
        pack_time_major(yb.data(), ld, values, lengths, n_series);
        if (any_mask) pack_validity(vb.data(), ld, validity, lengths, n_series);
        double *d_y = scratch.get<double>(T * ld);
        int32_t *d_len = scratch.get<int32_t>(ld);
        int32_t *d_int = scratch.get<int32_t>(SEASONALITY_N_INT * ld);
        double *d_fp = scratch.get<double>(SEASONALITY_N_FP * ld);
        uint8_t *d_valid = nullptr;
        HIPCHECK(hipMemcpy(d_y, yb.data(), T * ld * sizeof(double), hipMemcpyHostToDevice));
        HIPCHECK(hipMemcpy(d_len, len.data(), ld * sizeof(int32_t), hipMemcpyHostToDevice));
        if (any_mask) {
            d_valid = scratch.get<uint8_t>(T * ld);
            HIPCHECK(hipMemcpy(d_valid, vb.data(), T * ld, hipMemcpyHostToDevice));
        }
        if (!anofox_hip_seasonality_device(d_y, d_valid, ld, d_len, n_series, T, max_period, d_int, d_fp, nullptr, out_batch_error)) return false;
        HIPCHECK(hipMemcpy(oi.data(), d_int, oi.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
        HIPCHECK(hipMemcpy(of.data(), d_fp, of.size() * sizeof(double), hipMemcpyDeviceToHost));
        scratch.settled();
    } catch (const HipFail &f) {
        report_hip_failure(out_batch_error, f);
        return false;
    }
    for (size_t s = 0; s < n_series; s++) {
        AnofoxHipSeasonality &r = out_results[s];
        std::memset(&r, 0, sizeof r);
        for (int k = 0; k < SEASONALITY_TOP; k++) {
            r.periods[k] = oi[k * ld + s];
            r.strengths[k] = of[k * ld + s];
            r.acf[k] = of[(SEASONALITY_TOP + k) * ld + s];
        }
        r.n_periods = oi[5 * ld + s];
        r.primary_period = oi[6 * ld + s];
        r.seasonal_strength = of[10 * ld + s];
        r.trend_strength = of[11 * ld + s];
        if (out_status) out_status[s] = oi[7 * ld + s];
    }
    return true;
}

// one series through the kernel; false with the source's error when it is too short
static bool seasonality_single(const double *values, size_t length, int max_period, AnofoxHipSeasonality *r, AnofoxError *out_error)
{
    const double *v[1] = {values};
    const size_t len[1] = {length};
    int32_t status = 0;
    if (!anofox_hip_seasonality_batch(v, nullptr, len, 1, max_period, r, &status, out_error)) return false;
    if (status == SEASONALITY_SHORT) {
        set_error(out_error, COMPUTATION_ERROR, "Insufficient data: need at least 4 observations, got " + std::to_string(length));
        return false;
    }
    return true;
}

static bool seasonality_periods(const AnofoxHipSeasonality &r, int **out, AnofoxError *out_error)
{
    *out = nullptr;
    if (r.n_periods <= 0) return true;
    int *p = (int *)std::malloc((size_t)r.n_periods * sizeof(int));
    if (!p) { set_error(out_error, ALLOCATION_ERROR, "Memory allocation failed"); return false; }
    for (int k = 0; k < r.n_periods; k++) p[k] = r.periods[k];
    *out = p;
    return true;
}

bool anofox_ts_detect_seasonality(const double *values, size_t length, int max_period, int **out_periods, size_t *out_n_periods, AnofoxError *out_error)
{
    clear_error(out_error);
    if (!values || !out_periods || !out_n_periods) { set_error(out_error, NULL_POINTER, "Null pointer argument"); return false; }
    AnofoxHipSeasonality r;
    if (!seasonality_single(values, length, max_period, &r, out_error)) return false;
    if (!seasonality_periods(r, out_periods, out_error)) return false;
    *out_n_periods = (size_t)r.n_periods;
    return true;
}

bool anofox_ts_analyze_seasonality(const int64_t *timestamps, size_t timestamps_len, const double *values, size_t length, int max_period,
                                   SeasonalityResult *out_result, AnofoxError *out_error)
{
    (void)timestamps; (void)timestamps_len;                  // ignored, as the reference ignores them
    clear_error(out_error);
    if (!values || !out_result) { set_error(out_error, NULL_POINTER, "Null pointer argument"); return false; }
    AnofoxHipSeasonality r;
    if (!seasonality_single(values, length, max_period, &r, out_error)) return false;
    int *p = nullptr;
    if (!seasonality_periods(r, &p, out_error)) return false;
    out_result->detected_periods = p;
    out_result->n_periods = (size_t)r.n_periods;
    out_result->primary_period = r.primary_period;
    out_result->seasonal_strength = r.seasonal_strength;
    out_result->trend_strength = r.trend_strength;
    return true;
}

void anofox_free_seasonality_result(SeasonalityResult *result)
{
    if (!result) return;
    std::free(result->detected_periods);
    result->detected_periods = nullptr;
    result->n_periods = 0;
}

void anofox_free_int_array(int *ptr) { std::free(ptr); }

// ------------------------------------------------------------------------------------------------------------------------------
// Series preparation: gaps, zero trimming, NULL fills (gaps.rs, ts_macros.cpp:208-256, imputation.rs; dataprep.hip)
// ------------------------------------------------------------------------------------------------------------------------------
static_assert(sizeof(GapFillResult) == 32 && offsetof(GapFillResult, values) == 8 && offsetof(GapFillResult, validity) == 16 &&
              offsetof(GapFillResult, length) == 24, "GapFillResult layout");
static_assert(sizeof(FilledValuesResult) == 24 && offsetof(FilledValuesResult, validity) == 8 && offsetof(FilledValuesResult, length) == 16,
              "FilledValuesResult layout");
static_assert(sizeof(AnofoxHipPrepOptions) == 32 && offsetof(AnofoxHipPrepOptions, frequency_micros) == 8 &&
              offsetof(AnofoxHipPrepOptions, trim) == 16 && offsetof(AnofoxHipPrepOptions, fill_value) == 24, "AnofoxHipPrepOptions layout");

static bool prep_options_ok(const AnofoxHipPrepOptions *o, size_t struct_size, AnofoxError *err)
{
    if (struct_size != sizeof(AnofoxHipPrepOptions)) {
        set_error(err, INVALID_INPUT, "Invalid input: struct_size is not sizeof(AnofoxHipPrepOptions)");
        return false;
    }
    if (o->frequency_type < STATS_FREQ_FIXED || o->frequency_type > STATS_FREQ_YEARLY) {
        set_error(err, INVALID_INPUT, "Invalid input: unknown frequency type");
        return false;
    }
    if (o->trim < PREP_TRIM_NONE || o->trim > PREP_TRIM_EDGE || o->fill < PREP_FILL_NONE || o->fill > PREP_FILL_INTERPOLATE ||
        (o->gaps != 0 && o->gaps != 1)) {
        set_error(err, INVALID_INPUT, "Invalid input: unknown gaps, trim or fill mode");
        return false;
    }
    if (o->gaps && o->frequency_type == STATS_FREQ_FIXED && o->frequency_micros <= 0) {
        set_error(err, INVALID_FREQUENCY, "Frequency must be positive for fixed intervals");
        return false;
    }
    return true;
}

bool anofox_hip_prepare_device(const double *y, const uint8_t *valid, const int64_t *dates, size_t ld, const int32_t *lengths, size_t n_series,
                               size_t t_rows, const AnofoxHipPrepOptions *options, size_t struct_size, size_t t_out, double *y_out,
                               uint8_t *valid_out, int64_t *dates_out, int32_t *len_out, int64_t *out_int, double *out_fp, void *stream,
                               AnofoxError *out_error)
{
    clear_error(out_error);
    if (!y || !lengths || !options || !len_out || !out_int || !out_fp) {
        set_error(out_error, NULL_POINTER, "Null pointer argument");
        return false;
    }
    if (!block_args_ok(ld, n_series, "n_series", std::max(t_rows, t_out), (size_t)1 << 30, out_error)) return false;
    if (!prep_options_ok(options, struct_size, out_error)) return false;
    if (options->gaps && !dates) { set_error(out_error, INVALID_INPUT, "Invalid input: the gaps stage needs dates"); return false; }
    if (y_out) {
        // byte ranges of the blocks: no output may overlap an input (a lane reads rows that another lane's shifted store would hit)
        struct Range { const char *p; size_t bytes; };
        const Range in[3] = {{(const char *)y, t_rows * ld * 8}, {(const char *)valid, t_rows * ld}, {(const char *)dates, t_rows * ld * 8}};
        const Range out[3] = {{(const char *)y_out, t_out * ld * 8}, {(const char *)valid_out, t_out * ld}, {(const char *)dates_out, t_out * ld * 8}};
        for (const Range &o : out)
            for (const Range &i : in)
                if (o.p && i.p && o.bytes && i.bytes && o.p < i.p + i.bytes && i.p < o.p + o.bytes) {
                    set_error(out_error, INVALID_INPUT, "Invalid input: an output block overlaps an input block");
                    return false;
                }
    }
    if (!device_ready(out_error)) return false;
    DataprepArgs a{};
    a.y = y; a.valid = valid; a.dates = dates; a.ld = ld; a.len = lengths; a.n_series = (int)n_series; a.t_rows = t_rows;
    a.gaps = options->gaps; a.freq_type = options->frequency_type; a.freq_us = options->frequency_micros;
    a.trim = options->trim; a.fill = options->fill; a.fill_value = options->fill_value;
    a.t_out = t_out; a.y_out = y_out; a.valid_out = y_out ? valid_out : nullptr; a.dates_out = y_out ? dates_out : nullptr;
    a.len_out = len_out; a.out_int = out_int; a.out_fp = out_fp;
    hipStream_t st = (hipStream_t)stream;
    return launch_and_wait("dataprep", st, out_error, [&] { launch_dataprep(a, st); });
}

void anofox_hip_free_prepared(AnofoxHipPrepared *results, size_t n_series)
{
    if (!results) return;
    for (size_t s = 0; s < n_series; s++) {
        std::free(results[s].dates); std::free(results[s].values); std::free(results[s].validity);
        results[s].dates = nullptr; results[s].values = nullptr; results[s].validity = nullptr;
        results[s].length = 0;
    }
}

bool anofox_hip_prepare_batch(const double *const *values, const uint64_t *const *validity, const int64_t *const *dates, const size_t *lengths,
                              size_t n_series, const AnofoxHipPrepOptions *options, size_t struct_size, AnofoxHipPrepared *out_results,
                              AnofoxError *out_batch_error)
{
    clear_error(out_batch_error);
    if (!options || (n_series > 0 && (!values || !lengths || !out_results))) {
        set_error(out_batch_error, NULL_POINTER, "Null pointer argument");
        return false;
    }
    if (!prep_options_ok(options, struct_size, out_batch_error)) return false;
    BlockShape shape;
    if (!series_shape(values, validity, lengths, n_series, (size_t)PREP_MAX_ROWS, &shape, out_batch_error)) return false;
    size_t n_dated = 0, n_nonempty = 0;
    for (size_t s = 0; s < n_series; s++)
        if (lengths[s] > 0) { n_nonempty++; if (dates && dates[s]) n_dated++; }
    if (n_dated != 0 && n_dated != n_nonempty) {
        set_error(out_batch_error, INVALID_INPUT, "Invalid input: dates must be given for every series or for none");
        return false;
    }
    const bool dated = dates != nullptr && (n_dated > 0 || n_nonempty == 0);     // (only empty series: the block still has its date plane)
    if (options->gaps && !dated && n_nonempty > 0) {
        set_error(out_batch_error, INVALID_INPUT, "Invalid input: the gaps stage needs dates");
        return false;
    }
    for (size_t s = 0; s < n_series; s++) std::memset(&out_results[s], 0, sizeof out_results[s]);
    if (n_series == 0) return true;
    const size_t ld = shape.ld, T = shape.T;
    const bool any_mask = shape.any_mask;
    Scratch scratch;
    std::vector<int64_t> oi(PREP_N_INT * ld);
    std::vector<double> of(PREP_N_FP * ld), yo;
    std::vector<uint8_t> vo;
    std::vector<int64_t> dto;
    std::vector<int32_t> lo(n_series, 0);
    size_t t_out = 1;
    try {
        if (!device_ready(out_batch_error)) return false;
        std::vector<double> yb(T * ld, 0.0);
        std::vector<uint8_t> vb(any_mask ? T * ld : 0, 1);
        std::vector<int64_t> db(dated ? T * ld : 0, 0);
        const std::vector<int32_t> len = block_lengths(lengths, n_series, ld);
        std::vector<size_t> order;
        for (size_t s = 0; s < n_series; s++) {
            const size_t n = lengths[s];
            const uint64_t *m = validity ? validity[s] : nullptr;
            const int64_t *d = dated ? dates[s] : nullptr;
            order.resize(n);
            for (size_t t = 0; t < n; t++) order[t] = t;
            if (d) std::stable_sort(order.begin(), order.end(), [d](size_t i, size_t j) { return d[i] < d[j]; });     // gaps.rs:98-101
            for (size_t t = 0; t < n; t++) {
                const size_t i = order[t];
                yb[t * ld + s] = values[s][i];
                if (m) vb[t * ld + s] = (uint8_t)valid_bit(m, i);
                if (d) db[t * ld + s] = d[i];
            }
        }
        double *d_y = scratch.get<double>(T * ld);
        int32_t *d_len = scratch.get<int32_t>(ld), *d_lo = scratch.get<int32_t>(ld);
        int64_t *d_int = scratch.get<int64_t>(PREP_N_INT * ld), *d_dates = nullptr, *d_do = nullptr;
        double *d_fp = scratch.get<double>(PREP_N_FP * ld);
        uint8_t *d_valid = nullptr;
        HIPCHECK(hipMemcpy(d_y, yb.data(), T * ld * sizeof(double), hipMemcpyHostToDevice));
        HIPCHECK(hipMemcpy(d_len, len.data(), ld * sizeof(int32_t), hipMemcpyHostToDevice));
        if (any_mask) {
            d_valid = scratch.get<uint8_t>(T * ld);
            HIPCHECK(hipMemcpy(d_valid, vb.data(), T * ld, hipMemcpyHostToDevice));
        }
        if (dated) {
            d_dates = scratch.get<int64_t>(T * ld);
            HIPCHECK(hipMemcpy(d_dates, db.data(), T * ld * sizeof(int64_t), hipMemcpyHostToDevice));
        }
        // count, size the output block, run
        if (!anofox_hip_prepare_device(d_y, d_valid, d_dates, ld, d_len, n_series, T, options, struct_size, 0, nullptr, nullptr, nullptr, d_lo,
                                       d_int, d_fp, nullptr, out_batch_error))
            return false;
        HIPCHECK(hipMemcpy(lo.data(), d_lo, n_series * sizeof(int32_t), hipMemcpyDeviceToHost));
        for (size_t s = 0; s < n_series; s++) t_out = std::max(t_out, (size_t)lo[s]);
        double *d_yo = scratch.get<double>(t_out * ld);
        uint8_t *d_vo = scratch.get<uint8_t>(t_out * ld);
        if (dated) d_do = scratch.get<int64_t>(t_out * ld);
        if (!anofox_hip_prepare_device(d_y, d_valid, d_dates, ld, d_len, n_series, T, options, struct_size, t_out, d_yo, d_vo, d_do, d_lo, d_int,
                                       d_fp, nullptr, out_batch_error))
            return false;
        yo.resize(t_out * ld); vo.resize(t_out * ld);
        HIPCHECK(hipMemcpy(lo.data(), d_lo, n_series * sizeof(int32_t), hipMemcpyDeviceToHost));
        HIPCHECK(hipMemcpy(oi.data(), d_int, oi.size() * sizeof(int64_t), hipMemcpyDeviceToHost));
        HIPCHECK(hipMemcpy(of.data(), d_fp, of.size() * sizeof(double), hipMemcpyDeviceToHost));
        HIPCHECK(hipMemcpy(yo.data(), d_yo, yo.size() * sizeof(double), hipMemcpyDeviceToHost));
        HIPCHECK(hipMemcpy(vo.data(), d_vo, vo.size(), hipMemcpyDeviceToHost));
        if (dated) {
            dto.resize(t_out * ld);
            HIPCHECK(hipMemcpy(dto.data(), d_do, dto.size() * sizeof(int64_t), hipMemcpyDeviceToHost));
        }
        scratch.settled();
    } catch (const HipFail &f) {
        report_hip_failure(out_batch_error, f);
        return false;
    }
    for (size_t s = 0; s < n_series; s++) {
        AnofoxHipPrepared &r = out_results[s];
        for (int i = 0; i < PREP_N_INT; i++) r.figures[i] = oi[i * ld + s];
        r.min = of[s]; r.max = of[ld + s];
        const size_t n = (size_t)lo[s];
        r.length = n;
        if (n == 0) continue;
        r.values = (double *)std::malloc(n * sizeof(double));
        r.validity = (uint64_t *)std::calloc((n + 63) / 64, sizeof(uint64_t));
        if (dated) r.dates = (int64_t *)std::malloc(n * sizeof(int64_t));
        if (!r.values || !r.validity || (dated && !r.dates)) {
            anofox_hip_free_prepared(out_results, n_series);
            set_error(out_batch_error, ALLOCATION_ERROR, "Failed to allocate prepared series");
            return false;
        }
        for (size_t t = 0; t < n; t++) {
            r.values[t] = yo[t * ld + s];
            if (vo[t * ld + s]) r.validity[t >> 6] |= 1ull << (t & 63);
            if (dated) r.dates[t] = dto[t * ld + s];
        }
    }
    return true;
}

// one series through anofox_hip_prepare_batch with one stage on
static bool prep_single(const double *values, const uint64_t *validity, const int64_t *dates, size_t length, const AnofoxHipPrepOptions &o,
                        AnofoxHipPrepared *r, AnofoxError *out_error)
{
    const double *v[1] = {values};
    const uint64_t *m[1] = {validity};
    const int64_t *d[1] = {dates};
    const size_t len[1] = {length};
    if (!anofox_hip_prepare_batch(v, m, dates ? d : nullptr, len, 1, &o, sizeof o, r, out_error)) return false;
    if (r->figures[7] != PREP_OK) {
        anofox_hip_free_prepared(r, 1);
        set_error(out_error, COMPUTATION_ERROR, "Computation error: the gap-filled series exceeds 16777216 rows");
        return false;
    }
    return true;
}

static bool prep_fill_values(const double *values, const uint64_t *validity, size_t length, int fill, double fill_value, double **out_values,
                             AnofoxError *out_error)
{
    clear_error(out_error);
    if (!values || !out_values) { set_error(out_error, NULL_POINTER, "Null pointer argument"); return false; }
    AnofoxHipPrepOptions o{};
    o.fill = fill; o.fill_value = fill_value;
    AnofoxHipPrepared r;
    if (!prep_single(values, validity, nullptr, length, o, &r, out_error)) return false;
    *out_values = r.values;
    std::free(r.validity);
    return true;
}

bool anofox_ts_fill_nulls_const(const double *values, const uint64_t *validity, size_t length, double fill_value, double **out_values,
                                AnofoxError *out_error)
{
    return prep_fill_values(values, validity, length, PREP_FILL_CONST, fill_value, out_values, out_error);
}

bool anofox_ts_fill_nulls_mean(const double *values, const uint64_t *validity, size_t length, double **out_values, AnofoxError *out_error)
{
    return prep_fill_values(values, validity, length, PREP_FILL_MEAN, 0.0, out_values, out_error);
}

bool anofox_ts_fill_nulls_interpolate(const double *values, const uint64_t *validity, size_t length, double **out_values, AnofoxError *out_error)
{
    return prep_fill_values(values, validity, length, PREP_FILL_INTERPOLATE, 0.0, out_values, out_error);
}

static bool prep_fill_masked(const double *values, const uint64_t *validity, size_t length, int fill, FilledValuesResult *out_result,
                             AnofoxError *out_error)
{
    clear_error(out_error);
    if (!values || !out_result) { set_error(out_error, NULL_POINTER, "Null pointer argument"); return false; }
    AnofoxHipPrepOptions o{};
    o.fill = fill;
    AnofoxHipPrepared r;
    if (!prep_single(values, validity, nullptr, length, o, &r, out_error)) return false;
    out_result->values = r.values; out_result->validity = r.validity; out_result->length = r.length;
    return true;
}

bool anofox_ts_fill_nulls_forward(const double *values, const uint64_t *validity, size_t length, FilledValuesResult *out_result,
                                  AnofoxError *out_error)
{
    return prep_fill_masked(values, validity, length, PREP_FILL_FORWARD, out_result, out_error);
}

bool anofox_ts_fill_nulls_backward(const double *values, const uint64_t *validity, size_t length, FilledValuesResult *out_result,
                                   AnofoxError *out_error)
{
    return prep_fill_masked(values, validity, length, PREP_FILL_BACKWARD, out_result, out_error);
}

bool anofox_ts_fill_gaps(const int64_t *dates, const double *values, const uint64_t *validity, size_t length, int64_t frequency_micros,
                         FrequencyType frequency_type, GapFillResult *out_result, AnofoxError *out_error)
{
    clear_error(out_error);
    if (!dates || !values || !out_result) { set_error(out_error, NULL_POINTER, "Null pointer argument"); return false; }
    if (frequency_type == FIXED && frequency_micros <= 0) {
        set_error(out_error, INVALID_FREQUENCY, "Frequency must be positive for fixed intervals");
        return false;
    }
    AnofoxHipPrepOptions o{};
    o.gaps = 1; o.frequency_type = (int32_t)frequency_type; o.frequency_micros = frequency_micros;
    AnofoxHipPrepared r;
    if (!prep_single(values, validity, dates, length, o, &r, out_error)) return false;
    out_result->dates = r.dates; out_result->values = r.values; out_result->validity = r.validity; out_result->length = r.length;
    return true;
}

void anofox_free_gap_fill_result(GapFillResult *result)
{
    if (!result) return;
    std::free(result->dates); std::free(result->values); std::free(result->validity);
    result->dates = nullptr; result->values = nullptr; result->validity = nullptr; result->length = 0;
}

void anofox_free_filled_values_result(FilledValuesResult *result)
{
    if (!result) return;
    std::free(result->values); std::free(result->validity);
    result->values = nullptr; result->validity = nullptr; result->length = 0;
}

void anofox_free_double_array(double *ptr) { std::free(ptr); }

// ------------------------------------------------------------------------------------------------------------------------------
// Period detection (periods.rs lomb_scargle, aic_comparison, sazed_period, detect_periods_with_validation; periods.hip)
// ------------------------------------------------------------------------------------------------------------------------------
static_assert(sizeof(LombScargleResultFFI) == 64 && offsetof(LombScargleResultFFI, false_alarm_prob) == 24 &&
              offsetof(LombScargleResultFFI, method) == 32, "LombScargleResultFFI layout");
static_assert(sizeof(AicPeriodResultFFI) == 72 && offsetof(AicPeriodResultFFI, r_squared) == 32 && offsetof(AicPeriodResultFFI, method) == 40,
              "AicPeriodResultFFI layout");
static_assert(sizeof(SazedPeriodResultFFI) == 56 && offsetof(SazedPeriodResultFFI, snr) == 16 && offsetof(SazedPeriodResultFFI, method) == 24,
              "SazedPeriodResultFFI layout");
static_assert(sizeof(FlatMultiPeriodResult) == 120 && offsetof(FlatMultiPeriodResult, iteration_values) == 40 &&
              offsetof(FlatMultiPeriodResult, n_periods) == 72 && offsetof(FlatMultiPeriodResult, primary_period) == 80 &&
              offsetof(FlatMultiPeriodResult, method) == 88, "FlatMultiPeriodResult layout");

extern "C++" {
namespace {

const char *const PERIODS_METHOD_NAME[3] = {"lomb_scargle", "aic", "sazed"};
constexpr size_t PERIODS_NEEDED[3] = {4, 8, 16};

// PeriodMethod::from_str (periods.rs:47-68): 0 .. 2 the methods of this backend, -1 one of the other ten; `canonical` names it
int parse_period_method(const char *method, std::string &canonical)
{
    std::string m = method ? method : "fft";
    for (char &c : m) c = (char)std::tolower((unsigned char)c);
    struct Alias { const char *name; const char *canonical; int id; };
    static const Alias table[] = {
        {"fft", "fft", -1}, {"periodogram", "fft", -1}, {"acf", "acf", -1}, {"autocorrelation", "acf", -1},
        {"regression", "regression", -1}, {"fourier", "regression", -1}, {"multi", "multi", -1}, {"multiple", "multi", -1},
        {"auto", "auto", -1}, {"autoperiod", "autoperiod", -1}, {"ap", "autoperiod", -1},
        {"cfd", "cfd_autoperiod", -1}, {"cfdautoperiod", "cfd_autoperiod", -1}, {"cfd_autoperiod", "cfd_autoperiod", -1},
        {"lombscargle", "lomb_scargle", PERIODS_LOMB_SCARGLE}, {"lomb_scargle", "lomb_scargle", PERIODS_LOMB_SCARGLE},
        {"lomb-scargle", "lomb_scargle", PERIODS_LOMB_SCARGLE}, {"ls", "lomb_scargle", PERIODS_LOMB_SCARGLE},
        {"aic", "aic", PERIODS_AIC}, {"aic_comparison", "aic", PERIODS_AIC},
        {"ssa", "ssa", -1}, {"singular_spectrum", "ssa", -1}, {"stl", "stl", -1}, {"stl_period", "stl", -1}, {"seasonal_trend", "stl", -1},
        {"matrix_profile", "matrix_profile", -1}, {"matrixprofile", "matrix_profile", -1}, {"mp", "matrix_profile", -1},
        {"sazed", "sazed", PERIODS_SAZED}, {"zero_padded", "sazed", PERIODS_SAZED}, {"enhanced_dft", "sazed", PERIODS_SAZED},
    };
    for (const Alias &a : table)
        if (m == a.name) { canonical = a.canonical; return a.id; }
    canonical = "fft";                                             // the source's fallback for an unknown string
    return -1;
}

void copy_method(char (&dst)[32], const std::string &src)
{
    std::memset(dst, 0, sizeof dst);
    std::memcpy(dst, src.data(), std::min(src.size(), sizeof dst - 1));
}

std::string periods_series_error(int method, int32_t status, size_t n)
{
    if (status == PERIODS_TOO_SHORT)                               // ForecastError::InsufficientData { needed, got }
        return "Insufficient data: need at least " + std::to_string(PERIODS_NEEDED[method]) + " observations, got " + std::to_string(n);
    return "SAZED: the zero-padded length of a series of " + std::to_string(n) + " observations exceeds the limit of " +
           std::to_string((long long)PERIODS_SAZED_MAX_PADDED) + " of the HIP backend";
}

// one series through the batch entry; false with out_error set on any failure
bool periods_single(int method, const double *values, size_t length, double min_period, double max_period, size_t n_grid, double (&fig)[PERIODS_N_FP],
                    AnofoxError *out_error)
{
    AnofoxError serr, berr;
    const double *v[1] = {values};
    const size_t len[1] = {length};
    int32_t idx = -1;
    if (!anofox_hip_periods_batch(v, len, 1, method, min_period, max_period, n_grid, fig, &idx, &serr, &berr)) {
        if (out_error) *out_error = berr;
        return false;
    }
    if (serr.code != SUCCESS) { if (out_error) *out_error = serr; return false; }
    return true;
}

} // namespace
} // extern "C++"

bool anofox_hip_periods_device(const double *y, size_t ld, const int32_t *lengths, size_t n_series, size_t t_rows, int method, double min_period,
                               double max_period, size_t n_grid, double *figures, int32_t *index, int32_t *status, void *stream,
                               AnofoxError *out_error)
{
    clear_error(out_error);
    if (!y || !lengths || !figures || !index || !status) {
        set_error(out_error, NULL_POINTER, "Null pointer argument");
        return false;
    }
    if (method < PERIODS_LOMB_SCARGLE || method > PERIODS_SAZED) {
        set_error(out_error, INVALID_INPUT, "Invalid input: unknown period detection method " + std::to_string(method));
        return false;
    }
    if (!block_args_ok(ld, n_series, "n_series", t_rows, (size_t)INT32_MAX, out_error)) return false;
    if (method != PERIODS_SAZED && n_grid > (size_t)INT32_MAX) {
        set_error(out_error, INVALID_INPUT, "Invalid input: more than 2147483647 frequencies or candidates");
        return false;
    }
    if (!device_ready(out_error)) return false;
    PeriodsArgs a{};
    a.y = y; a.ld = ld; a.len = lengths; a.n_series = (int)n_series; a.t_rows = t_rows; a.method = method;
    a.out_fp = figures; a.out_index = index; a.status = status;
    if (method == PERIODS_SAZED) {
        // the wrapper's size_t arguments (lib.rs:1967-1983): zero means the default; values beyond any length act like the largest
        auto whole = [](double v) { return v > 0.0 ? (int64_t)std::fmin(v, 4e18) : (int64_t)0; };
        a.s_min = whole(min_period); a.s_max = whole(max_period);
        a.s_pad = (int64_t)std::min<size_t>(n_grid, (size_t)PERIODS_SAZED_MAX_PADDED + 1);
        a.work_stride = periods_work_stride(t_rows, a.s_pad);
        a.work_blocks = periods_work_blocks(a.work_stride, (int)n_series);
    } else {
        a.min_period = min_period; a.max_period = max_period;        // > 0.0 or the default (lib.rs:1635-1649, 1707-1721)
        a.n_grid = n_grid > 0 ? (int64_t)n_grid : (method == PERIODS_LOMB_SCARGLE ? 1000 : 50);
    }
    hipStream_t st = (hipStream_t)stream;
    Scratch scratch;
    const bool ok = launch_and_wait("periods", st, out_error, [&] {
        if (a.work_stride && a.work_blocks > 0) a.work = scratch.get<double>(a.work_stride * (size_t)a.work_blocks);
        launch_periods(a, st);
    });
    if (ok) scratch.settled();
    return ok;
}

bool anofox_hip_periods_batch(const double *const *values, const size_t *lengths, size_t n_series, int method, double min_period, double max_period,
                              size_t n_grid, double *out_figures, int32_t *out_index, AnofoxError *out_errors, AnofoxError *out_batch_error)
{
    clear_error(out_batch_error);
    if (n_series > 0 && (!values || !lengths || !out_figures)) {
        set_error(out_batch_error, NULL_POINTER, "Null pointer argument");
        return false;
    }
    if (method < PERIODS_LOMB_SCARGLE || method > PERIODS_SAZED) {
        set_error(out_batch_error, INVALID_INPUT, "Invalid input: unknown period detection method " + std::to_string(method));
        return false;
    }
    BlockShape shape;
    if (!series_shape(values, nullptr, lengths, n_series, (size_t)INT32_MAX, &shape, out_batch_error)) return false;
    if (n_series == 0) return true;
    const size_t ld = shape.ld, T = shape.T;
    Scratch scratch;
    std::vector<double> fp(PERIODS_N_FP * ld);
    std::vector<int32_t> idx(n_series), status(n_series);
    try {
        if (!device_ready(out_batch_error)) return false;
        std::vector<double> yb(T * ld, 0.0);
        const std::vector<int32_t> len = block_lengths(lengths, n_series, ld);
        pack_time_major(yb.data(), ld, values, lengths, n_series);
        double *d_y = scratch.get<double>(T * ld);
        int32_t *d_len = scratch.get<int32_t>(ld);
        double *d_fp = scratch.get<double>(PERIODS_N_FP * ld);
        int32_t *d_idx = scratch.get<int32_t>(ld), *d_st = scratch.get<int32_t>(ld);
        HIPCHECK(hipMemcpy(d_y, yb.data(), T * ld * sizeof(double), hipMemcpyHostToDevice));
        HIPCHECK(hipMemcpy(d_len, len.data(), ld * sizeof(int32_t), hipMemcpyHostToDevice));
        if (!anofox_hip_periods_device(d_y, ld, d_len, n_series, T, method, min_period, max_period, n_grid, d_fp, d_idx, d_st, nullptr,
                                       out_batch_error))
            return false;
        HIPCHECK(hipMemcpy(fp.data(), d_fp, fp.size() * sizeof(double), hipMemcpyDeviceToHost));
        HIPCHECK(hipMemcpy(idx.data(), d_idx, n_series * sizeof(int32_t), hipMemcpyDeviceToHost));
        HIPCHECK(hipMemcpy(status.data(), d_st, n_series * sizeof(int32_t), hipMemcpyDeviceToHost));
        scratch.settled();
    } catch (const HipFail &f) {
        report_hip_failure(out_batch_error, f);
        return false;
    }
    const double nan = std::numeric_limits<double>::quiet_NaN();
    const int used = method == PERIODS_LOMB_SCARGLE ? 4 : (method == PERIODS_AIC ? 5 : 3);
    for (size_t s = 0; s < n_series; s++) {
        const bool ok = status[s] == PERIODS_OK;
        if (out_errors) clear_error(&out_errors[s]);
        if (!ok && out_errors) set_error(&out_errors[s], COMPUTATION_ERROR, periods_series_error(method, status[s], lengths[s]));
        for (int j = 0; j < PERIODS_N_FP; j++) out_figures[(size_t)j * n_series + s] = (ok && j < used) ? fp[(size_t)j * ld + s] : nan;
        if (out_index) out_index[s] = ok ? idx[s] : -1;
    }
    return true;
}

bool anofox_ts_lomb_scargle(const double *values, size_t length, double min_period, double max_period, size_t n_frequencies,
                            LombScargleResultFFI *out_result, AnofoxError *out_error)
{
    clear_error(out_error);
    if (!values || !out_result) { set_error(out_error, NULL_POINTER, "Null pointer argument"); return false; }
    double fig[PERIODS_N_FP];
    if (!periods_single(PERIODS_LOMB_SCARGLE, values, length, min_period, max_period, n_frequencies, fig, out_error)) return false;
    out_result->period = fig[0]; out_result->frequency = fig[1]; out_result->power = fig[2]; out_result->false_alarm_prob = fig[3];
    copy_method(out_result->method, PERIODS_METHOD_NAME[PERIODS_LOMB_SCARGLE]);
    return true;
}

bool anofox_ts_aic_period(const double *values, size_t length, double min_period, double max_period, size_t n_candidates,
                          AicPeriodResultFFI *out_result, AnofoxError *out_error)
{
    clear_error(out_error);
    if (!values || !out_result) { set_error(out_error, NULL_POINTER, "Null pointer argument"); return false; }
    double fig[PERIODS_N_FP];
    if (!periods_single(PERIODS_AIC, values, length, min_period, max_period, n_candidates, fig, out_error)) return false;
    out_result->period = fig[0]; out_result->aic = fig[1]; out_result->bic = fig[2]; out_result->rss = fig[3]; out_result->r_squared = fig[4];
    copy_method(out_result->method, PERIODS_METHOD_NAME[PERIODS_AIC]);
    return true;
}

bool anofox_ts_sazed_period(const double *values, size_t length, size_t min_period, size_t max_period, size_t zero_pad_factor,
                            SazedPeriodResultFFI *out_result, AnofoxError *out_error)
{
    clear_error(out_error);
    if (!values || !out_result) { set_error(out_error, NULL_POINTER, "Null pointer argument"); return false; }
    double fig[PERIODS_N_FP];
    // periods beyond 2^53 act like any period beyond the series' length, so the conversion to double loses nothing that matters
    if (!periods_single(PERIODS_SAZED, values, length, (double)min_period, (double)max_period, zero_pad_factor, fig, out_error)) return false;
    out_result->period = fig[0]; out_result->power = fig[1]; out_result->snr = fig[2];
    copy_method(out_result->method, PERIODS_METHOD_NAME[PERIODS_SAZED]);
    return true;
}

bool anofox_ts_detect_periods_flat(const double *values, size_t length, const char *method, size_t max_period, double min_confidence,
                                   const double *expected_periods, size_t n_expected, double tolerance, FlatMultiPeriodResult *out_result,
                                   AnofoxError *out_error)
{
    clear_error(out_error);
    if (!values || !out_result) { set_error(out_error, NULL_POINTER, "Null pointer argument"); return false; }
    (void)max_period;                                              // detect_periods_internal passes it to fft / acf / auto only
    std::string name;
    const int m = parse_period_method(method, name);
    if (m < 0) {
        set_error(out_error, INTERNAL_ERROR, "Internal error: period detection method '" + name + "' is not implemented by the HIP backend");
        return false;
    }
    double fig[PERIODS_N_FP];
    if (!periods_single(m, values, length, 0.0, 0.0, 0, fig, out_error)) return false;
    // one DetectedPeriod per method (periods.rs:1651-1686, 1741-1758)
    const double period = fig[0];
    double confidence, strength;
    if (m == PERIODS_LOMB_SCARGLE) { confidence = 1.0 - fig[3]; strength = fig[2]; }
    else if (m == PERIODS_AIC) { confidence = fig[4]; strength = fig[4]; }
    else { confidence = std::fmin(fig[2], 1.0); strength = fig[1]; }
    // detect_periods (periods.rs:1494-1517): these methods use the 0.3 threshold; 0 or below disables the filter
    const double threshold = (min_confidence < 0.0 || std::isnan(min_confidence)) ? 0.3 : min_confidence;
    const bool kept = !(threshold > 0.0) || confidence >= threshold;
    std::memset(out_result, 0, sizeof *out_result);
    if (!kept) {
        out_result->primary_period = 0.0;
        copy_method(out_result->method, name + " (no seasonality)");
        return true;
    }
    const double nan = std::numeric_limits<double>::quiet_NaN();
    bool matches = false;
    double matched = nan, deviation = nan;
    if (expected_periods && n_expected > 0) {                      // validate_period (periods.rs:1385-1421)
        const double tol = (tolerance < 0.0 || std::isnan(tolerance)) ? 0.1 : tolerance;
        for (size_t i = 0; i < n_expected; i++) {
            const double e = expected_periods[i];
            if (e <= 0.0) continue;
            const double dev = std::fabs(period - e) / e;
            if (dev <= tol && (!matches || dev < deviation)) { matches = true; matched = e; deviation = dev; }
        }
    }
    double *d[7];
    for (double *&q : d) q = (double *)std::malloc(sizeof(double));
    out_result->iteration_values = (size_t *)std::malloc(sizeof(size_t));
    out_result->matches_expected_values = (bool *)std::malloc(sizeof(bool));
    out_result->period_values = d[0]; out_result->confidence_values = d[1]; out_result->strength_values = d[2];
    out_result->amplitude_values = d[3]; out_result->phase_values = d[4];
    out_result->matched_expected_values = d[5]; out_result->match_deviation_values = d[6];
    bool ok = out_result->iteration_values && out_result->matches_expected_values;
    for (double *q : d) ok = ok && q;
    if (!ok) {
        anofox_free_flat_multi_period_result(out_result);
        set_error(out_error, ALLOCATION_ERROR, "Failed to allocate period detection result");
        return false;
    }
    *d[0] = period; *d[1] = confidence; *d[2] = strength; *d[3] = 0.0; *d[4] = 0.0; *d[5] = matched; *d[6] = deviation;
    out_result->iteration_values[0] = 1;
    out_result->matches_expected_values[0] = matches;
    out_result->n_periods = 1;
    out_result->primary_period = period;
    copy_method(out_result->method, name);
    return true;
}

void anofox_free_flat_multi_period_result(FlatMultiPeriodResult *result)
{
    if (!result) return;
    std::free(result->period_values); std::free(result->confidence_values); std::free(result->strength_values);
    std::free(result->amplitude_values); std::free(result->phase_values); std::free(result->iteration_values);
    std::free(result->matches_expected_values); std::free(result->matched_expected_values); std::free(result->match_deviation_values);
    result->period_values = result->confidence_values = result->strength_values = result->amplitude_values = result->phase_values = nullptr;
    result->matched_expected_values = result->match_deviation_values = nullptr;
    result->iteration_values = nullptr;
    result->matches_expected_values = nullptr;
    result->n_periods = 0;
}

// ------------------------------------------------------------------------------------------------------------------------------
// Period search: SSA and STL strength (periods.rs ssa_period, stl_period behind lib.rs:1755-1878; period_search.hip).  Entries of
// their own: the dispatch by method name above keeps its not-implemented error for 'ssa' and 'stl' (DESIGN.md section 7).
// ------------------------------------------------------------------------------------------------------------------------------
static_assert(sizeof(SsaPeriodResultFFI) == 56 && offsetof(SsaPeriodResultFFI, n_eigenvalues) == 16 && offsetof(SsaPeriodResultFFI, method) == 24,
              "SsaPeriodResultFFI layout");
static_assert(sizeof(StlPeriodResultFFI) == 56 && offsetof(StlPeriodResultFFI, trend_strength) == 16 && offsetof(StlPeriodResultFFI, method) == 24,
              "StlPeriodResultFFI layout");

extern "C++" {
namespace {

bool psearch_check(PSearchCheck c, const std::string &text, AnofoxError *err)
{
    if (c == PSEARCH_CHECK_OK) return true;
    if (c == PSEARCH_CHECK_NULL) set_error(err, NULL_POINTER, "Null pointer argument");
    else set_error(err, INVALID_INPUT, text);
    return false;
}

// a batch of host series on the device: the block, the lengths and the status column every period-search batch entry needs
struct PSearchBlock {
    size_t ld = 0, T = 1;
    double *d_y = nullptr;
    int32_t *d_len = nullptr, *d_st = nullptr;
};

PSearchBlock psearch_upload(Scratch &scratch, const BlockShape &shape, const double *const *values, const size_t *lengths, size_t n_series)
{
    PSearchBlock b;
    b.ld = shape.ld; b.T = shape.T;
    std::vector<double> yb(b.T * b.ld, 0.0);
    const std::vector<int32_t> len = block_lengths(lengths, n_series, b.ld);
    pack_time_major(yb.data(), b.ld, values, lengths, n_series);
    b.d_y = scratch.get<double>(b.T * b.ld);
    b.d_len = scratch.get<int32_t>(b.ld);
    b.d_st = scratch.get<int32_t>(b.ld);
    HIPCHECK(hipMemcpy(b.d_y, yb.data(), b.T * b.ld * sizeof(double), hipMemcpyHostToDevice));
    HIPCHECK(hipMemcpy(b.d_len, len.data(), b.ld * sizeof(int32_t), hipMemcpyHostToDevice));
    return b;
}

template <class T> std::vector<T> psearch_fetch(const T *d, size_t count)
{
    std::vector<T> h(count);
    if (count) HIPCHECK(hipMemcpy(h.data(), d, count * sizeof(T), hipMemcpyDeviceToHost));
    return h;
}

} // namespace
} // extern "C++"

bool anofox_hip_ssa_period_device(const double *y, size_t ld, const int32_t *lengths, size_t n_series, size_t t_rows, size_t window_size,
                                  size_t n_components, int route, double *figures, double *eigenvalues, double *detected, int32_t *status,
                                  void *stream, AnofoxError *out_error)
{
    clear_error(out_error);
    if (!y || !lengths || !figures || !status) {
        set_error(out_error, NULL_POINTER, "Null pointer argument");
        return false;
    }
    std::string text;
    if (!psearch_check(ssa_args_check(t_rows, n_components, &text), text, out_error)) return false;
    if (route < SSA_ROUTE_AUTO || route > SSA_ROUTE_GROUP) {
        set_error(out_error, INVALID_INPUT, "Invalid input: route " + std::to_string(route) + " is unknown: 0 (automatic) or 1 (256 lanes for every window)");
        return false;
    }
    if (!block_args_ok(ld, n_series, "n_series", t_rows, PSEARCH_MAX_ROWS, out_error)) return false;
    if (!device_ready(out_error)) return false;
    SsaArgs a{};
    a.y = y; a.ld = ld; a.len = lengths; a.n_series = (int)n_series; a.t_rows = t_rows;
    a.window = psearch_arg(window_size); a.n_components = ssa_components(n_components); a.route = route;
    a.out_fp = figures; a.out_eig = eigenvalues; a.out_det = detected; a.status = status;
    a.work_stride = ssa_work_stride(t_rows, a.window);
    a.work_blocks = ssa_work_blocks(a.work_stride, (int)n_series);
    hipStream_t st = (hipStream_t)stream;
    Scratch scratch;
    const bool ok = launch_and_wait("ssa_period", st, out_error, [&] {
        if (a.work_stride && a.work_blocks > 0) a.work = scratch.get<double>(a.work_stride * (size_t)a.work_blocks);
        launch_ssa_period(a, st);
    });
    if (ok) scratch.settled();
    return ok;
}

bool anofox_hip_stl_period_device(const double *y, size_t ld, const int32_t *lengths, size_t n_series, size_t t_rows, size_t min_period,
                                  size_t max_period, size_t n_candidates, double *figures, int32_t *index, int32_t *candidates,
                                  double *candidate_strengths, int32_t *status, void *stream, AnofoxError *out_error)
{
    clear_error(out_error);
    if (!y || !lengths || !figures || !index || !status) {
        set_error(out_error, NULL_POINTER, "Null pointer argument");
        return false;
    }
    std::string text;
    if (!psearch_check(stl_args_check(t_rows, n_candidates, &text), text, out_error)) return false;
    if (!block_args_ok(ld, n_series, "n_series", t_rows, PSEARCH_MAX_ROWS, out_error)) return false;
    if (!device_ready(out_error)) return false;
    StlPeriodArgs a{};
    a.y = y; a.ld = ld; a.len = lengths; a.n_series = (int)n_series; a.t_rows = t_rows;
    a.min_period = psearch_arg(min_period); a.max_period = psearch_arg(max_period); a.n_cand = stl_candidate_count(n_candidates);
    a.out_fp = figures; a.out_index = index; a.status = status; a.out_cand = candidates; a.out_strength = candidate_strengths;
    a.work_stride = stl_period_work_stride(t_rows);
    a.work_blocks = stl_period_work_blocks(a.work_stride, (int)n_series);
    hipStream_t st = (hipStream_t)stream;
    Scratch scratch;
    const bool ok = launch_and_wait("stl_period", st, out_error, [&] {
        if (a.work_stride && a.work_blocks > 0) a.work = scratch.get<double>(a.work_stride * (size_t)a.work_blocks);
        launch_stl_period(a, st);
    });
    if (ok) scratch.settled();
    return ok;
}

bool anofox_hip_ssa_period_batch(const double *const *values, const size_t *lengths, size_t n_series, size_t window_size, size_t n_components,
                                 double *out_figures, double *out_eigenvalues, double *out_detected, AnofoxError *out_errors,
                                 AnofoxError *out_batch_error)
{
    clear_error(out_batch_error);
    if (n_series > 0 && (!values || !lengths || !out_figures)) {
        set_error(out_batch_error, NULL_POINTER, "Null pointer argument");
        return false;
    }
    std::string text;
    size_t longest = 0;
    if (!psearch_check(ssa_args_check(0, n_components, &text), text, out_batch_error)) return false;
    if (!psearch_check(psearch_batch_rows(lengths, n_series, &longest, &text), text, out_batch_error)) return false;
    BlockShape shape;
    if (!series_shape(values, nullptr, lengths, n_series, PSEARCH_MAX_ROWS, &shape, out_batch_error)) return false;
    if (n_series == 0) return true;
    const size_t ld = shape.ld, C = (size_t)ssa_components(n_components);
    std::vector<double> fp, eig, det;
    std::vector<int32_t> status;
    Scratch scratch;
    try {
        if (!device_ready(out_batch_error)) return false;
        const PSearchBlock b = psearch_upload(scratch, shape, values, lengths, n_series);
        double *d_fp = scratch.get<double>(SSA_N_FIG * ld);
        double *d_eig = out_eigenvalues ? scratch.get<double>(C * ld) : nullptr;
        double *d_det = out_detected ? scratch.get<double>(SSA_N_DETECTED * ld) : nullptr;
        if (!anofox_hip_ssa_period_device(b.d_y, ld, b.d_len, n_series, b.T, window_size, n_components, SSA_ROUTE_AUTO, d_fp, d_eig, d_det, b.d_st,
                                          nullptr, out_batch_error))
            return false;
        fp = psearch_fetch(d_fp, SSA_N_FIG * ld);
        if (d_eig) eig = psearch_fetch(d_eig, C * ld);
        if (d_det) det = psearch_fetch(d_det, SSA_N_DETECTED * ld);
        status = psearch_fetch(b.d_st, n_series);
        scratch.settled();
    } catch (const HipFail &f) {
        report_hip_failure(out_batch_error, f);
        return false;
    }
    const double nan = std::numeric_limits<double>::quiet_NaN();
    for (size_t s = 0; s < n_series; s++) {
        const bool ok = status[s] == PSEARCH_OK;
        if (out_errors) clear_error(&out_errors[s]);
        if (!ok && out_errors) set_error(&out_errors[s], COMPUTATION_ERROR, psearch_series_error(status[s], lengths[s], psearch_arg(window_size)));
        for (size_t j = 0; j < (size_t)SSA_N_FIG; j++) out_figures[j * n_series + s] = ok ? fp[j * ld + s] : nan;
        if (out_eigenvalues)
            for (size_t j = 0; j < C; j++) out_eigenvalues[j * n_series + s] = ok ? eig[j * ld + s] : nan;
        if (out_detected)
            for (size_t j = 0; j < (size_t)SSA_N_DETECTED; j++) out_detected[j * n_series + s] = ok ? det[j * ld + s] : nan;
    }
    return true;
}

bool anofox_hip_stl_period_batch(const double *const *values, const size_t *lengths, size_t n_series, size_t min_period, size_t max_period,
                                 size_t n_candidates, double *out_figures, int32_t *out_index, int32_t *out_candidates,
                                 double *out_candidate_strengths, AnofoxError *out_errors, AnofoxError *out_batch_error)
{
    clear_error(out_batch_error);
    if (n_series > 0 && (!values || !lengths || !out_figures)) {
        set_error(out_batch_error, NULL_POINTER, "Null pointer argument");
        return false;
    }
    std::string text;
    size_t longest = 0;
    if (!psearch_check(stl_args_check(0, n_candidates, &text), text, out_batch_error)) return false;
    if (!psearch_check(psearch_batch_rows(lengths, n_series, &longest, &text), text, out_batch_error)) return false;
    BlockShape shape;
    if (!series_shape(values, nullptr, lengths, n_series, PSEARCH_MAX_ROWS, &shape, out_batch_error)) return false;
    if (n_series == 0) return true;
    const size_t ld = shape.ld, K = (size_t)stl_candidate_count(n_candidates);
    std::vector<double> fp, strength;
    std::vector<int32_t> status, idx, cand;
    Scratch scratch;
    try {
        if (!device_ready(out_batch_error)) return false;
        const PSearchBlock b = psearch_upload(scratch, shape, values, lengths, n_series);
        double *d_fp = scratch.get<double>(STL_N_FIG * ld);
        int32_t *d_idx = scratch.get<int32_t>(ld);
        int32_t *d_cand = out_candidates ? scratch.get<int32_t>(K * ld) : nullptr;
        double *d_str = out_candidate_strengths ? scratch.get<double>(K * ld) : nullptr;
        if (!anofox_hip_stl_period_device(b.d_y, ld, b.d_len, n_series, b.T, min_period, max_period, n_candidates, d_fp, d_idx, d_cand, d_str, b.d_st,
                                          nullptr, out_batch_error))
            return false;
        fp = psearch_fetch(d_fp, STL_N_FIG * ld);
        idx = psearch_fetch(d_idx, n_series);
        if (d_cand) cand = psearch_fetch(d_cand, K * ld);
        if (d_str) strength = psearch_fetch(d_str, K * ld);
        status = psearch_fetch(b.d_st, n_series);
        scratch.settled();
    } catch (const HipFail &f) {
        report_hip_failure(out_batch_error, f);
        return false;
    }
    const double nan = std::numeric_limits<double>::quiet_NaN();
    for (size_t s = 0; s < n_series; s++) {
        const bool ok = status[s] == PSEARCH_OK;
        if (out_errors) clear_error(&out_errors[s]);
        if (!ok && out_errors) set_error(&out_errors[s], COMPUTATION_ERROR, psearch_series_error(status[s], lengths[s], 0));
        for (size_t j = 0; j < (size_t)STL_N_FIG; j++) out_figures[j * n_series + s] = ok ? fp[j * ld + s] : nan;
        if (out_index) out_index[s] = ok ? idx[s] : -1;
        if (out_candidates)
            for (size_t j = 0; j < K; j++) out_candidates[j * n_series + s] = ok ? cand[j * ld + s] : -1;
        if (out_candidate_strengths)
            for (size_t j = 0; j < K; j++) out_candidate_strengths[j * n_series + s] = ok ? strength[j * ld + s] : nan;
    }
    return true;
}

bool anofox_ts_ssa_period(const double *values, size_t length, size_t window_size, size_t n_components, SsaPeriodResultFFI *out_result,
                          AnofoxError *out_error)
{
    clear_error(out_error);
    if (!values || !out_result) { set_error(out_error, NULL_POINTER, "Null pointer argument"); return false; }
    AnofoxError serr, berr;
    const double *v[1] = {values};
    const size_t len[1] = {length};
    double fig[SSA_N_FIG];
    if (!anofox_hip_ssa_period_batch(v, len, 1, window_size, n_components, fig, nullptr, nullptr, &serr, &berr)) {
        if (out_error) *out_error = berr;
        return false;
    }
    if (serr.code != SUCCESS) { if (out_error) *out_error = serr; return false; }
    out_result->period = fig[0]; out_result->variance_explained = fig[1]; out_result->n_eigenvalues = (size_t)fig[2];
    copy_method(out_result->method, "ssa");
    return true;
}

bool anofox_ts_stl_period(const double *values, size_t length, size_t min_period, size_t max_period, size_t n_candidates,
                          StlPeriodResultFFI *out_result, AnofoxError *out_error)
{
    clear_error(out_error);
    if (!values || !out_result) { set_error(out_error, NULL_POINTER, "Null pointer argument"); return false; }
    AnofoxError serr, berr;
    const double *v[1] = {values};
    const size_t len[1] = {length};
    double fig[STL_N_FIG];
    if (!anofox_hip_stl_period_batch(v, len, 1, min_period, max_period, n_candidates, fig, nullptr, nullptr, nullptr, &serr, &berr)) {
        if (out_error) *out_error = berr;
        return false;
    }
    if (serr.code != SUCCESS) { if (out_error) *out_error = serr; return false; }
    out_result->period = fig[0]; out_result->seasonal_strength = fig[1]; out_result->trend_strength = fig[2];
    copy_method(out_result->method, "stl");
    return true;
}

// ------------------------------------------------------------------------------------------------------------------------------
// Period by matrix profile (periods.rs matrix_profile_period behind lib.rs:1888; matrix_profile.hip).  Entries of its own: the
// dispatch by method name above keeps its not-implemented error for 'matrix_profile' (DESIGN.md section 7).
// ------------------------------------------------------------------------------------------------------------------------------
static_assert(sizeof(MatrixProfilePeriodResultFFI) == 64 && offsetof(MatrixProfilePeriodResultFFI, n_motifs) == 16 &&
              offsetof(MatrixProfilePeriodResultFFI, method) == 32, "MatrixProfilePeriodResultFFI layout");

bool anofox_hip_matrix_profile_device(const double *y, size_t ld, const int32_t *lengths, size_t n_series, size_t t_rows, size_t subsequence_length,
                                      size_t n_best, double *figures, double *profile, int32_t *profile_index, int32_t *status, void *stream,
                                      AnofoxError *out_error)
{
    clear_error(out_error);
    if (!y || !lengths || !figures || !status) {
        set_error(out_error, NULL_POINTER, "Null pointer argument");
        return false;
    }
    std::string text;
    if (mprof_args_check(t_rows, &text) != MPROF_CHECK_OK) {
        set_error(out_error, INVALID_INPUT, text);
        return false;
    }
    if (!block_args_ok(ld, n_series, "n_series", t_rows, MPROF_MAX_ROWS, out_error)) return false;
    if (!device_ready(out_error)) return false;
    MatrixProfileArgs a{};
    a.y = y; a.ld = ld; a.len = lengths; a.n_series = (int)n_series; a.t_rows = t_rows;
    a.subsequence = mprof_arg(subsequence_length); a.n_best = mprof_arg(n_best);
    a.out_fp = figures; a.out_profile = profile; a.out_index = profile_index; a.status = status;
    a.profile_rows = (int)mprof_profile_len((int64_t)t_rows, a.subsequence);
    a.work_stride = matrix_profile_work_stride(t_rows, a.subsequence);
    a.work_blocks = matrix_profile_work_blocks(a.work_stride, (int)n_series);
    hipStream_t st = (hipStream_t)stream;
    Scratch scratch;
    const bool ok = launch_and_wait("matrix_profile", st, out_error, [&] {
        if (a.work_stride && a.work_blocks > 0) a.work = scratch.get<double>(a.work_stride * (size_t)a.work_blocks);
        launch_matrix_profile(a, st);
    });
    if (ok) scratch.settled();
    return ok;
}

bool anofox_hip_matrix_profile_batch(const double *const *values, const size_t *lengths, size_t n_series, size_t subsequence_length, size_t n_best,
                                     double *out_figures, double *out_profile, int32_t *out_profile_index, AnofoxError *out_errors,
                                     AnofoxError *out_batch_error)
{
    clear_error(out_batch_error);
    if (n_series > 0 && (!values || !lengths || !out_figures)) {
        set_error(out_batch_error, NULL_POINTER, "Null pointer argument");
        return false;
    }
    std::string text;
    size_t longest = 0;
    const MProfCheck rows = mprof_batch_rows(lengths, n_series, &longest, &text);
    if (rows != MPROF_CHECK_OK) {
        if (rows == MPROF_CHECK_NULL) set_error(out_batch_error, NULL_POINTER, "Null pointer argument");
        else set_error(out_batch_error, INVALID_INPUT, text);
        return false;
    }
    BlockShape shape;
    if (!series_shape(values, nullptr, lengths, n_series, MPROF_MAX_ROWS, &shape, out_batch_error)) return false;
    if (n_series == 0) return true;
    const size_t ld = shape.ld, P = (size_t)mprof_profile_len((int64_t)longest, mprof_arg(subsequence_length));
    std::vector<double> fp, prof;
    std::vector<int32_t> status, index;
    Scratch scratch;
    try {
        if (!device_ready(out_batch_error)) return false;
        const PSearchBlock b = psearch_upload(scratch, shape, values, lengths, n_series);
        double *d_fp = scratch.get<double>(MPROF_N_FIG * ld);
        double *d_prof = out_profile && P ? scratch.get<double>(P * ld) : nullptr;
        int32_t *d_idx = out_profile_index && P ? scratch.get<int32_t>(P * ld) : nullptr;
        if (!anofox_hip_matrix_profile_device(b.d_y, ld, b.d_len, n_series, b.T, subsequence_length, n_best, d_fp, d_prof, d_idx, b.d_st, nullptr,
                                              out_batch_error))
            return false;
        fp = psearch_fetch(d_fp, MPROF_N_FIG * ld);
        if (d_prof) prof = psearch_fetch(d_prof, P * ld);
        if (d_idx) index = psearch_fetch(d_idx, P * ld);
        status = psearch_fetch(b.d_st, n_series);
        scratch.settled();
    } catch (const HipFail &f) {
        report_hip_failure(out_batch_error, f);
        return false;
    }
    const double nan = std::numeric_limits<double>::quiet_NaN();
    for (size_t s = 0; s < n_series; s++) {
        const bool ok = status[s] == MPROF_OK;
        if (out_errors) clear_error(&out_errors[s]);
        if (!ok && out_errors) set_error(&out_errors[s], COMPUTATION_ERROR, mprof_series_error(status[s], lengths[s], mprof_arg(subsequence_length)));
        for (size_t j = 0; j < (size_t)MPROF_N_FIG; j++) out_figures[j * n_series + s] = ok ? fp[j * ld + s] : nan;
        if (out_profile)
            for (size_t j = 0; j < P; j++) out_profile[j * n_series + s] = ok ? prof[j * ld + s] : nan;
        if (out_profile_index)
            for (size_t j = 0; j < P; j++) out_profile_index[j * n_series + s] = ok ? index[j * ld + s] : -1;
    }
    return true;
}

bool anofox_ts_matrix_profile_period(const double *values, size_t length, size_t subsequence_length, size_t n_best,
                                     MatrixProfilePeriodResultFFI *out_result, AnofoxError *out_error)
{
    clear_error(out_error);
    if (!values || !out_result) { set_error(out_error, NULL_POINTER, "Null pointer argument"); return false; }
    AnofoxError serr, berr;
    const double *v[1] = {values};
    const size_t len[1] = {length};
    double fig[MPROF_N_FIG];
    if (!anofox_hip_matrix_profile_batch(v, len, 1, subsequence_length, n_best, fig, nullptr, nullptr, &serr, &berr)) {
        if (out_error) *out_error = berr;
        return false;
    }
    if (serr.code != SUCCESS) { if (out_error) *out_error = serr; return false; }
    out_result->period = fig[0]; out_result->confidence = fig[1]; out_result->n_motifs = (size_t)fig[2]; out_result->subsequence_length = (size_t)fig[3];
    copy_method(out_result->method, "matrix_profile");
    return true;
}

// ------------------------------------------------------------------------------------------------------------------------------
// Forecast accuracy metrics (metrics.rs mae .. coverage behind lib.rs:303-800; metrics.hip)
// ------------------------------------------------------------------------------------------------------------------------------
extern "C++" {
namespace {

const char *const METRICS_FIGURE_NAME[METRICS_N_FIG] = {"mae", "mse", "rmse", "mape", "smape", "r2", "bias", "rmae", "mase", "quantile_loss",
                                                        "mqloss", "coverage"};
const char *const METRICS_EMPTY_TEXT = "Insufficient data: need at least 1 observations, got 0";       // ForecastError::InsufficientData
const char *const METRICS_QUANTILE_TEXT = "Invalid input: Quantile must be between 0 and 1";            // metrics.rs:278-282
constexpr uint32_t METRICS_ALL = (1u << METRICS_N_FIG) - 1;

bool metrics_unit_interval(double q) { return q >= 0.0 && q <= 1.0; }       // (0.0..=1.0).contains: false for a NaN

// what the batch and the device entry check alike: the mask, the level count, and that every requested figure has its blocks
bool metrics_check_request(uint32_t mask, bool has_f, bool has_s, bool has_l, bool has_u, bool has_q, size_t n_levels, const double *levels,
                           AnofoxError *err)
{
    if (mask == 0 || (mask & ~METRICS_ALL)) {
        set_error(err, INVALID_INPUT, "Invalid input: the figure mask must name at least one of the 12 figures and nothing else");
        return false;
    }
    if (n_levels > (size_t)METRICS_MAX_LEVELS) {
        set_error(err, INVALID_INPUT, "Invalid input: at most " + std::to_string(METRICS_MAX_LEVELS) + " quantile levels per call, got " +
                                          std::to_string(n_levels));
        return false;
    }
    for (int k = 0; k < METRICS_N_FIG; k++) {
        if (!(mask >> k & 1u)) continue;
        const char *missing = nullptr;
        if ((METRICS_NEED_FORECAST >> k & 1u) && !has_f) missing = "forecast";
        else if ((METRICS_NEED_SECOND >> k & 1u) && !has_s) missing = "second";
        else if (k == MF_COVERAGE && !(has_l && has_u)) missing = "lower and upper";
        else if (k == MF_MQLOSS && n_levels > 0 && !(has_q && levels)) missing = "quantiles and levels";
        if (missing) {
            set_error(err, INVALID_INPUT, std::string("Invalid input: figure '") + METRICS_FIGURE_NAME[k] + "' needs " + missing);
            return false;
        }
    }
    if ((mask >> MF_MQLOSS & 1u) && n_levels == 0) {
        set_error(err, INVALID_INPUT, "Must have at least one quantile level");        // lib.rs:700-708
        return false;
    }
    return true;
}

// one group, one figure, through the batch entry (the argument checks of the single entries come before it and need no device)
bool metrics_single(int figure, const double *actual, size_t n, const double *forecast, const double *second, const double *lower,
                    const double *upper, const double *const *quantiles, const double *levels, size_t n_levels, double quantile,
                    double *out_result, AnofoxError *out_error)
{
    AnofoxError gerr, berr;
    const double *a[1] = {actual}, *f[1] = {forecast}, *s[1] = {second}, *l[1] = {lower}, *u[1] = {upper};
    const double *qcol[METRICS_MAX_LEVELS];
    const double *const *qq[METRICS_MAX_LEVELS];
    for (size_t k = 0; k < n_levels && k < (size_t)METRICS_MAX_LEVELS; k++) { qcol[k] = quantiles[k]; qq[k] = &qcol[k]; }
    const size_t len[1] = {n};
    double fig[METRICS_N_FIG];
    if (!anofox_hip_metrics_batch(a, forecast ? f : nullptr, second ? s : nullptr, lower ? l : nullptr, upper ? u : nullptr,
                                  quantiles ? qq : nullptr, levels, n_levels, len, 1, 1u << figure, quantile, false, fig, &gerr, &berr)) {
        if (out_error) *out_error = berr;
        return false;
    }
    if (gerr.code != SUCCESS) { if (out_error) *out_error = gerr; return false; }
    *out_result = fig[figure];
    return true;
}

// validate_inputs (metrics.rs:364-375) as the FFI wrappers report it
bool metrics_validate(size_t n_actual, size_t n_forecast, AnofoxError *err)
{
    if (n_actual != n_forecast) {
        set_error(err, COMPUTATION_ERROR, "Invalid input: Actual and forecast arrays must have the same length: " + std::to_string(n_actual) +
                                              " vs " + std::to_string(n_forecast));
        return false;
    }
    if (n_actual == 0) { set_error(err, COMPUTATION_ERROR, METRICS_EMPTY_TEXT); return false; }
    return true;
}

bool metrics_two(int figure, const double *actual, size_t actual_len, const double *forecast, size_t forecast_len, double *out_result,
                 AnofoxError *out_error)
{
    clear_error(out_error);
    if (!actual || !forecast || !out_result) { set_error(out_error, NULL_POINTER, "Null pointer argument"); return false; }
    if (!metrics_validate(actual_len, forecast_len, out_error)) return false;
    return metrics_single(figure, actual, actual_len, forecast, nullptr, nullptr, nullptr, nullptr, nullptr, 0, 0.5, out_result, out_error);
}

bool metrics_three(int figure, const char *third_name, const double *actual, size_t actual_len, const double *forecast, size_t forecast_len,
                   const double *third, size_t third_len, double *out_result, AnofoxError *out_error)
{
    clear_error(out_error);
    if (!actual || !forecast || !third || !out_result) { set_error(out_error, NULL_POINTER, "Null pointer argument"); return false; }
    if (!metrics_validate(actual_len, forecast_len, out_error)) return false;
    if (actual_len != third_len) {                                 // metrics.rs:168-173, 238-243
        set_error(out_error, COMPUTATION_ERROR, std::string("Invalid input: Actual and ") + third_name + " arrays must have the same length: " +
                                                    std::to_string(actual_len) + " vs " + std::to_string(third_len));
        return false;
    }
    return metrics_single(figure, actual, actual_len, forecast, third, nullptr, nullptr, nullptr, nullptr, 0, 0.5, out_result, out_error);
}

} // namespace
} // extern "C++"

bool anofox_hip_metrics_device(const double *actual, const double *forecast, const double *second, const double *lower, const double *upper,
                               const double *quantiles, size_t stride_q, const double *levels, size_t n_levels, size_t stride_s,
                               size_t stride_t, const int32_t *lengths, size_t n_groups, size_t t_rows, uint32_t figures_mask, double quantile,
                               bool drop_nan, double *figures, size_t ld, int32_t *status, void *stream, AnofoxError *out_error)
{
    clear_error(out_error);
    if (!actual || !lengths || !figures || !status) { set_error(out_error, NULL_POINTER, "Null pointer argument"); return false; }
    if (!metrics_check_request(figures_mask, forecast, second, lower, upper, quantiles, n_levels, levels, out_error)) return false;
    if ((figures_mask >> MF_QUANTILE_LOSS & 1u) && !metrics_unit_interval(quantile)) {
        set_error(out_error, INVALID_INPUT, METRICS_QUANTILE_TEXT);
        return false;
    }
    const bool use_q = quantiles && levels && n_levels > 0;
    if (figures_mask >> MF_MQLOSS & 1u)
        for (size_t k = 0; k < n_levels; k++)
            if (!metrics_unit_interval(levels[k])) { set_error(out_error, INVALID_INPUT, METRICS_QUANTILE_TEXT); return false; }
    if (!block_args_ok(ld, n_groups, "n_groups", t_rows, (size_t)INT32_MAX, out_error)) return false;
    if (n_groups == 0) return true;
    if (!device_ready(out_error)) return false;
    MetricsArgs a{};
    a.actual = actual; a.forecast = forecast; a.second = second; a.lower = lower; a.upper = upper;
    a.quant = use_q ? quantiles : nullptr; a.n_levels = use_q ? (int)n_levels : 0; a.stride_q = stride_q;
    for (int k = 0; k < a.n_levels; k++) a.levels[k] = levels[k];
    a.stride_s = stride_s; a.stride_t = stride_t; a.len = lengths; a.n_groups = (int)n_groups; a.t_rows = t_rows;
    a.mask = figures_mask; a.drop_nan = drop_nan ? 1 : 0; a.quantile = quantile;
    a.figures = figures; a.ld = ld; a.status = status;
    a.staging = -1;
    {                                                              // developer knob of tools/time_metrics.py: 0 strided reads, 1 LDS staging
        const std::map<std::string, std::string> kv = Tunables::tune_map();
        auto it = kv.find("metrics_staging");
        if (it != kv.end()) a.staging = std::atoi(it->second.c_str());
    }
    hipStream_t st = (hipStream_t)stream;
    return launch_and_wait("metrics", st, out_error, [&] { launch_metrics(a, st); });
}

bool anofox_hip_metrics_batch(const double *const *actual, const double *const *forecast, const double *const *second, const double *const *lower,
                              const double *const *upper, const double *const *const *quantiles, const double *levels, size_t n_levels,
                              const size_t *lengths, size_t n_groups, uint32_t figures_mask, double quantile, bool drop_nan,
                              double *out_figures, AnofoxError *out_errors, AnofoxError *out_batch_error)
{
    clear_error(out_batch_error);
    if (n_groups > 0 && (!actual || !lengths || !out_figures)) { set_error(out_batch_error, NULL_POINTER, "Null pointer argument"); return false; }
    if (!metrics_check_request(figures_mask, forecast, second, lower, upper, quantiles, n_levels, levels, out_batch_error)) return false;
    const size_t nq = (quantiles && levels) ? n_levels : 0;
    for (size_t k = 0; k < nq; k++)
        if (!quantiles[k]) { set_error(out_batch_error, NULL_POINTER, "Null pointer argument"); return false; }
    size_t t_max = 0;
    std::vector<int> null_level(n_groups, -1);                     // a group whose level k forecasts are NULL fails alone (lib.rs:716-723)
    for (size_t s = 0; s < n_groups; s++) {
        if (lengths[s] == 0) continue;
        if (!actual[s] || (forecast && !forecast[s]) || (second && !second[s]) || (lower && !lower[s]) || (upper && !upper[s])) {
            set_error(out_batch_error, NULL_POINTER, "Null pointer argument");
            return false;
        }
        if (lengths[s] > (size_t)INT32_MAX) { set_error(out_batch_error, INVALID_INPUT, "Invalid input: a group is too long"); return false; }
        for (size_t k = 0; k < nq && null_level[s] < 0; k++)
            if (!quantiles[k][s]) null_level[s] = (int)k;
        if (null_level[s] < 0) t_max = std::max(t_max, lengths[s]);
    }
    if (n_groups == 0) return true;
    // a quantile or level outside [0, 1] fails the figure that uses it, per group as the single entries do; the others are computed
    uint32_t mask = figures_mask;
    const bool ql_bad = (mask >> MF_QUANTILE_LOSS & 1u) && !metrics_unit_interval(quantile);
    bool mql_bad = false;
    if (mask >> MF_MQLOSS & 1u)
        for (size_t k = 0; k < nq; k++) mql_bad = mql_bad || !metrics_unit_interval(levels[k]);
    if (ql_bad) mask &= ~(1u << MF_QUANTILE_LOSS);
    if (mql_bad) mask &= ~(1u << MF_MQLOSS);
    const size_t ld = (n_groups + 63) / 64 * 64, T = std::max<size_t>(t_max, 1);
    std::vector<double> fig((size_t)METRICS_N_FIG * ld, std::numeric_limits<double>::quiet_NaN());
    std::vector<int32_t> status(n_groups, METRICS_OK), len(ld, 0);
    for (size_t s = 0; s < n_groups; s++) {
        len[s] = null_level[s] < 0 ? (int32_t)lengths[s] : 0;
        status[s] = len[s] > 0 ? METRICS_OK : METRICS_EMPTY;
    }
    if (mask != 0) {
        const double *const *src[5] = {actual, forecast, second, lower, upper};
        const bool use_q = nq > 0 && (mask >> MF_MQLOSS & 1u);
        const size_t n_blocks = 5 + (use_q ? nq : 0);
        std::vector<double *> d_in(6, nullptr);                    // actual .. upper, and every level's block in one (level k at k * T * ld)
        Scratch scratch;
        try {
            if (!device_ready(out_batch_error)) return false;
            std::vector<double> blk(T * ld);
            if (use_q) d_in[5] = scratch.get<double>(nq * T * ld);
            for (size_t b = 0; b < n_blocks; b++) {
                const double *const *col = b < 5 ? src[b] : quantiles[b - 5];
                if (!col) continue;
                std::fill(blk.begin(), blk.end(), 0.0);
                pack_time_major(blk.data(), ld, col, len.data(), n_groups);        // (len: 0 for a group that fails alone)
                double *dst = b < 5 ? (d_in[b] = scratch.get<double>(T * ld)) : d_in[5] + (b - 5) * T * ld;
                HIPCHECK(hipMemcpy(dst, blk.data(), T * ld * sizeof(double), hipMemcpyHostToDevice));
            }
            double *d_fig = scratch.get<double>((size_t)METRICS_N_FIG * ld);
            int32_t *d_len = scratch.get<int32_t>(ld), *d_st = scratch.get<int32_t>(ld);
            HIPCHECK(hipMemcpy(d_fig, fig.data(), fig.size() * sizeof(double), hipMemcpyHostToDevice));
            HIPCHECK(hipMemcpy(d_len, len.data(), ld * sizeof(int32_t), hipMemcpyHostToDevice));
            if (!anofox_hip_metrics_device(d_in[0], d_in[1], d_in[2], d_in[3], d_in[4], use_q ? d_in[5] : nullptr, T * ld, levels, use_q ? nq : 0, 1,
                                           ld, d_len, n_groups, T, mask, ql_bad ? 0.5 : quantile, drop_nan, d_fig, ld, d_st, nullptr,
                                           out_batch_error))
                return false;
            HIPCHECK(hipMemcpy(fig.data(), d_fig, fig.size() * sizeof(double), hipMemcpyDeviceToHost));
            HIPCHECK(hipMemcpy(status.data(), d_st, n_groups * sizeof(int32_t), hipMemcpyDeviceToHost));
            scratch.settled();
        } catch (const HipFail &f) {
            report_hip_failure(out_batch_error, f);
            return false;
        }
    }
    const double nan = std::numeric_limits<double>::quiet_NaN();
    for (size_t s = 0; s < n_groups; s++) {
        const bool empty = status[s] != METRICS_OK;
        for (int k = 0; k < METRICS_N_FIG; k++)
            out_figures[(size_t)k * n_groups + s] = (!empty && (mask >> k & 1u)) ? fig[(size_t)k * ld + s] : nan;
        if (!out_errors) continue;
        clear_error(&out_errors[s]);
        if (null_level[s] >= 0) set_error(&out_errors[s], COMPUTATION_ERROR, "Invalid input: Null pointer at quantile index " + std::to_string(null_level[s]));
        else if (empty && (figures_mask & ~(1u << MF_COVERAGE))) set_error(&out_errors[s], COMPUTATION_ERROR, METRICS_EMPTY_TEXT);   // coverage of nothing is NaN, no error
        else if (!empty && (ql_bad || mql_bad)) set_error(&out_errors[s], COMPUTATION_ERROR, METRICS_QUANTILE_TEXT);
    }
    return true;
}

bool anofox_ts_mae(const double *actual, size_t actual_len, const double *forecast, size_t forecast_len, double *out_result, AnofoxError *out_error)
{ return metrics_two(MF_MAE, actual, actual_len, forecast, forecast_len, out_result, out_error); }
bool anofox_ts_mse(const double *actual, size_t actual_len, const double *forecast, size_t forecast_len, double *out_result, AnofoxError *out_error)
{ return metrics_two(MF_MSE, actual, actual_len, forecast, forecast_len, out_result, out_error); }
bool anofox_ts_rmse(const double *actual, size_t actual_len, const double *forecast, size_t forecast_len, double *out_result, AnofoxError *out_error)
{ return metrics_two(MF_RMSE, actual, actual_len, forecast, forecast_len, out_result, out_error); }
bool anofox_ts_mape(const double *actual, size_t actual_len, const double *forecast, size_t forecast_len, double *out_result, AnofoxError *out_error)
{ return metrics_two(MF_MAPE, actual, actual_len, forecast, forecast_len, out_result, out_error); }
bool anofox_ts_smape(const double *actual, size_t actual_len, const double *forecast, size_t forecast_len, double *out_result, AnofoxError *out_error)
{ return metrics_two(MF_SMAPE, actual, actual_len, forecast, forecast_len, out_result, out_error); }
bool anofox_ts_r2(const double *actual, size_t actual_len, const double *forecast, size_t forecast_len, double *out_result, AnofoxError *out_error)
{ return metrics_two(MF_R2, actual, actual_len, forecast, forecast_len, out_result, out_error); }
bool anofox_ts_bias(const double *actual, size_t actual_len, const double *forecast, size_t forecast_len, double *out_result, AnofoxError *out_error)
{ return metrics_two(MF_BIAS, actual, actual_len, forecast, forecast_len, out_result, out_error); }

bool anofox_ts_rmae(const double *actual, size_t actual_len, const double *pred1, size_t pred1_len, const double *pred2, size_t pred2_len,
                    double *out_result, AnofoxError *out_error)
{ return metrics_three(MF_RMAE, "pred2", actual, actual_len, pred1, pred1_len, pred2, pred2_len, out_result, out_error); }

bool anofox_ts_mase(const double *actual, size_t actual_len, const double *forecast, size_t forecast_len, const double *baseline, size_t baseline_len,
                    double *out_result, AnofoxError *out_error)
{ return metrics_three(MF_MASE, "baseline", actual, actual_len, forecast, forecast_len, baseline, baseline_len, out_result, out_error); }

bool anofox_ts_quantile_loss(const double *actual, size_t actual_len, const double *forecast, size_t forecast_len, double quantile,
                             double *out_result, AnofoxError *out_error)
{
    clear_error(out_error);
    if (!actual || !forecast || !out_result) { set_error(out_error, NULL_POINTER, "Null pointer argument"); return false; }
    if (!metrics_validate(actual_len, forecast_len, out_error)) return false;
    if (!metrics_unit_interval(quantile)) { set_error(out_error, COMPUTATION_ERROR, METRICS_QUANTILE_TEXT); return false; }
    return metrics_single(MF_QUANTILE_LOSS, actual, actual_len, forecast, nullptr, nullptr, nullptr, nullptr, nullptr, 0, quantile, out_result,
                          out_error);
}

bool anofox_ts_mqloss(const double *actual, size_t actual_len, const double *const *quantiles, size_t n_levels, const double *levels,
                      double *out_result, AnofoxError *out_error)
{
    clear_error(out_error);
    if (!actual || !quantiles || !levels || !out_result) { set_error(out_error, NULL_POINTER, "Null pointer argument"); return false; }
    if (n_levels == 0) { set_error(out_error, INVALID_INPUT, "Must have at least one quantile level"); return false; }
    if (n_levels > (size_t)METRICS_MAX_LEVELS) {                   // the backend's limit
        set_error(out_error, INVALID_INPUT, "Invalid input: at most " + std::to_string(METRICS_MAX_LEVELS) + " quantile levels per call, got " +
                                                std::to_string(n_levels));
        return false;
    }
    for (size_t k = 0; k < n_levels; k++)
        if (!quantiles[k]) {
            set_error(out_error, COMPUTATION_ERROR, "Invalid input: Null pointer at quantile index " + std::to_string(k));
            return false;
        }
    // mqloss walks the levels in order (metrics.rs:319-322): quantile_loss validates its inputs, then its level
    if (actual_len == 0) { set_error(out_error, COMPUTATION_ERROR, METRICS_EMPTY_TEXT); return false; }
    for (size_t k = 0; k < n_levels; k++)
        if (!metrics_unit_interval(levels[k])) { set_error(out_error, COMPUTATION_ERROR, METRICS_QUANTILE_TEXT); return false; }
    return metrics_single(MF_MQLOSS, actual, actual_len, nullptr, nullptr, nullptr, nullptr, quantiles, levels, n_levels, 0.5, out_result, out_error);
}

bool anofox_ts_coverage(const double *actual, size_t actual_len, const double *lower, const double *upper, double *out_result,
                        AnofoxError *out_error)
{
    clear_error(out_error);
    if (!actual || !lower || !upper || !out_result) { set_error(out_error, NULL_POINTER, "Null pointer argument"); return false; }
    if (actual_len == 0) { *out_result = std::numeric_limits<double>::quiet_NaN(); return true; }       // metrics.rs:350-352
    return metrics_single(MF_COVERAGE, actual, actual_len, nullptr, nullptr, lower, upper, nullptr, nullptr, 0, 0.5, out_result, out_error);
}

// ------------------------------------------------------------------------------------------------------------------------------
// Conformal prediction intervals (conformal.rs conformal_learn / conformal_apply / conformal_evaluate; conformal.hip)
// ------------------------------------------------------------------------------------------------------------------------------
extern "C++" {
namespace {

const char *const CONFORMAL_EMPTY_TEXT = "Insufficient data: need at least 1 observations, got 0";     // ForecastError::InsufficientData
const char *const CONFORMAL_NO_ALPHA_TEXT = "Invalid input: At least one alpha value is required";     // conformal.rs:706-710
const char *const CONFORMAL_NO_FORECAST_TEXT = "Invalid input: At least one forecast is required";     // conformal.rs:897-901
const char *const CONFORMAL_DIFFICULTY_TEXT = "Invalid input: Difficulty scores must be positive";     // conformal.rs:736-740, 918-922
const char *const CONFORMAL_NEED_DIFFICULTY_TEXT = "Invalid input: Difficulty scores required for adaptive method";
const char *const CONFORMAL_NAN_TEXT = "Invalid input: a residual is NaN";                             // the backend's limit

bool conformal_alpha_ok(double a) { return a >= 0.0 && a < 1.0; }            // (0.0..1.0).contains: 0 is in, a NaN is not

// Rust's `{}` of an f64: the shortest decimal that reads back the same, never with an exponent ("1", "1.5", "0.0000001", "NaN", "inf")
std::string conformal_show(double v)
{
    if (v != v) return "NaN";
    if (std::isinf(v)) return v > 0 ? "inf" : "-inf";
    char buf[1200];
    for (int decimals = 0; decimals <= 780; decimals++) {
        std::snprintf(buf, sizeof buf, "%.*f", decimals, v);
        if (std::strtod(buf, nullptr) == v) break;
    }
    return buf;
}

bool conformal_check_levels(const double *alphas, size_t n_alphas, bool need, AnofoxError *err)
{
    if (n_alphas > (size_t)CONFORMAL_MAX_LEVELS) {
        set_error(err, INVALID_INPUT, "Invalid input: at most " + std::to_string(CONFORMAL_MAX_LEVELS) + " coverage levels per call, got " +
                                          std::to_string(n_alphas));
        return false;
    }
    if (n_alphas == 0) { set_error(err, INVALID_INPUT, CONFORMAL_NO_ALPHA_TEXT); return false; }
    if (!need) return true;
    if (!alphas) { set_error(err, NULL_POINTER, "Null pointer argument"); return false; }
    for (size_t k = 0; k < n_alphas; k++)
        if (!conformal_alpha_ok(alphas[k])) {
            set_error(err, INVALID_INPUT, "Invalid input: Alpha must be in (0, 1), got " + conformal_show(alphas[k]));     // conformal.rs:712-719
            return false;
        }
    return true;
}

bool conformal_check_method(int method, AnofoxError *err)
{
    if (method == CONFORMAL_SYMMETRIC || method == CONFORMAL_ASYMMETRIC || method == CONFORMAL_ADAPTIVE) return true;
    set_error(err, INVALID_INPUT, "Invalid input: unknown conformal method (0 symmetric, 1 asymmetric, 2 adaptive)");
    return false;
}

} // namespace
} // extern "C++"

bool anofox_hip_conformal_learn_device(const double *residual, const double *actual, const double *forecast, const uint8_t *valid,
                                       size_t stride_s, size_t stride_t, const int32_t *lengths, size_t n_groups, size_t t_rows,
                                       const double *alphas, size_t n_alphas, int method, double *scores_lower, double *scores_upper,
                                       size_t ld, double *sorted, int32_t *n_kept, int32_t *status, void *stream, AnofoxError *out_error)
{
    clear_error(out_error);
    if ((!residual && !(actual && forecast)) || !lengths || !scores_lower || !scores_upper || !status) {
        set_error(out_error, NULL_POINTER, "Null pointer argument");
        return false;
    }
    if (!conformal_check_levels(alphas, n_alphas, true, out_error) || !conformal_check_method(method, out_error)) return false;
    if (!block_args_ok(ld, n_groups, "n_groups", t_rows, (size_t)1 << 30, out_error)) return false;
    if (n_groups == 0) return true;
    if (!device_ready(out_error)) return false;
    ConformalLearnArgs a{};
    a.residual = residual; a.actual = actual; a.forecast = forecast; a.valid = valid;
    a.stride_s = stride_s; a.stride_t = stride_t; a.len = lengths; a.n_groups = (int)n_groups; a.t_rows = t_rows;
    a.method = method; a.n_alphas = (int)n_alphas;
    for (size_t k = 0; k < n_alphas; k++) a.alphas[k] = alphas[k];
    a.scores_lower = scores_lower; a.scores_upper = scores_upper; a.ld = ld;
    a.sorted = sorted; a.n_kept = n_kept; a.status = status;
    a.tile = conformal_tile(t_rows);
    a.work_stride = conformal_work_stride(t_rows);
    a.work_waves = a.work_stride ? conformal_work_waves((int)n_groups) : 0;
    hipStream_t st = (hipStream_t)stream;
    Scratch scratch;
    const bool ok = launch_and_wait("conformal_learn", st, out_error, [&] {
        if (a.work_stride && a.work_waves > 0) a.work = scratch.get<uint64_t>(a.work_stride * (size_t)a.work_waves);
        launch_conformal_learn(a, st);
    });
    if (ok) scratch.settled();
    return ok;
}

bool anofox_hip_conformal_apply_device(const double *forecast, const double *difficulty, size_t stride_s, size_t stride_t,
                                       const int32_t *lengths, size_t n_groups, size_t h_rows, const double *scores_lower,
                                       const double *scores_upper, size_t ld, size_t n_alphas, int method, double *lower, double *upper,
                                       size_t stride_q, int32_t *status, void *stream, AnofoxError *out_error)
{
    clear_error(out_error);
    if (!forecast || !scores_lower || !scores_upper || !lower || !upper || !status) {
        set_error(out_error, NULL_POINTER, "Null pointer argument");
        return false;
    }
    if (!conformal_check_levels(nullptr, n_alphas, false, out_error) || !conformal_check_method(method, out_error)) return false;
    if (method == CONFORMAL_ADAPTIVE && !difficulty) { set_error(out_error, INVALID_INPUT, CONFORMAL_NEED_DIFFICULTY_TEXT); return false; }
    if (!block_args_ok(ld, n_groups, "n_groups", h_rows, (size_t)1 << 30, out_error)) return false;
    if (h_rows == 0) { set_error(out_error, INVALID_INPUT, CONFORMAL_NO_FORECAST_TEXT); return false; }
    if (n_groups == 0) return true;
    if (!device_ready(out_error)) return false;
    ConformalApplyArgs a{};
    a.forecast = forecast; a.difficulty = difficulty; a.stride_s = stride_s; a.stride_t = stride_t;
    a.len = lengths; a.n_groups = (int)n_groups; a.h_rows = (int)h_rows;
    a.scores_lower = scores_lower; a.scores_upper = scores_upper; a.ld = ld;
    a.method = method; a.n_alphas = (int)n_alphas;
    a.lower = lower; a.upper = upper; a.stride_q = stride_q; a.status = status;
    hipStream_t st = (hipStream_t)stream;
    return launch_and_wait("conformal_apply", st, out_error, [&] { launch_conformal_apply(a, st); });
}

bool anofox_hip_conformal_evaluate_device(const double *actual, const double *lower, const double *upper, size_t stride_s, size_t stride_t,
                                          const int32_t *lengths, size_t n_groups, size_t t_rows, double alpha, double *figures, size_t ld,
                                          int32_t *status, void *stream, AnofoxError *out_error)
{
    clear_error(out_error);
    if (!actual || !lower || !upper || !lengths || !figures || !status) {
        set_error(out_error, NULL_POINTER, "Null pointer argument");
        return false;
    }
    if (!conformal_check_levels(&alpha, 1, true, out_error)) return false;
    if (!block_args_ok(ld, n_groups, "n_groups", t_rows, (size_t)1 << 30, out_error)) return false;
    if (n_groups == 0) return true;
    if (!device_ready(out_error)) return false;
    ConformalEvalArgs a{};
    a.actual = actual; a.lower = lower; a.upper = upper; a.stride_s = stride_s; a.stride_t = stride_t;
    a.len = lengths; a.n_groups = (int)n_groups; a.t_rows = t_rows; a.alpha = alpha;
    a.figures = figures; a.ld = ld; a.status = status;
    hipStream_t st = (hipStream_t)stream;
    return launch_and_wait("conformal_evaluate", st, out_error, [&] { launch_conformal_evaluate(a, st); });
}

void anofox_hip_free_conformal(AnofoxHipConformal *results, size_t n_groups)
{
    if (!results) return;
    for (size_t s = 0; s < n_groups; s++) {
        AnofoxHipConformal &r = results[s];
        std::free(r.scores_lower); std::free(r.scores_upper); std::free(r.sorted); std::free(r.lower); std::free(r.upper);
        std::memset(&r, 0, sizeof r);
    }
}

bool anofox_hip_conformal_batch(const double *const *residuals, const uint64_t *const *residual_validity, const size_t *residual_lengths,
                                const double *const *forecasts, const double *const *difficulty, const size_t *forecast_lengths,
                                size_t n_groups, const double *alphas, size_t n_alphas, int method, int strategy, bool want_sorted,
                                AnofoxHipConformal *out_results, AnofoxError *out_errors, AnofoxError *out_batch_error)
{
    clear_error(out_batch_error);
    if (n_groups > 0 && (!residuals || !residual_lengths || !out_results || (forecasts && !forecast_lengths))) {
        set_error(out_batch_error, NULL_POINTER, "Null pointer argument");
        return false;
    }
    if (!conformal_check_levels(alphas, n_alphas, true, out_batch_error) || !conformal_check_method(method, out_batch_error)) return false;
    if (strategy < 0 || strategy > 2) {
        set_error(out_batch_error, INVALID_INPUT, "Invalid input: unknown conformal strategy (0 split, 1 crossval, 2 jackknife+)");
        return false;
    }
    if (strategy == 2 && method == CONFORMAL_ASYMMETRIC) {          // conformal.rs:746-750
        set_error(out_batch_error, INVALID_INPUT, "Invalid input: JackknifePlus strategy does not support asymmetric method");
        return false;
    }
    if (forecasts && method == CONFORMAL_ADAPTIVE && !difficulty) {
        set_error(out_batch_error, INVALID_INPUT, CONFORMAL_NEED_DIFFICULTY_TEXT);
        return false;
    }
    size_t t_max = 0, h_max = 0;
    for (size_t s = 0; s < n_groups; s++) {
        const size_t h = forecasts ? forecast_lengths[s] : 0;
        if ((residual_lengths[s] > 0 && !residuals[s]) || (h > 0 && (!forecasts[s] || (method == CONFORMAL_ADAPTIVE && !difficulty[s])))) {
            set_error(out_batch_error, NULL_POINTER, "Null pointer argument");
            return false;
        }
        if (residual_lengths[s] > (size_t)(1u << 30) || h > (size_t)(1u << 30)) {
            set_error(out_batch_error, INVALID_INPUT, "Invalid input: a group is too long");
            return false;
        }
        t_max = std::max(t_max, residual_lengths[s]);
        h_max = std::max(h_max, h);
    }
    if (n_groups == 0) return true;
    for (size_t s = 0; s < n_groups; s++) std::memset(&out_results[s], 0, sizeof out_results[s]);
    const size_t ld = (n_groups + 63) / 64 * 64, T = std::max<size_t>(t_max, 1), H = h_max, K = n_alphas;
    const bool adaptive = method == CONFORMAL_ADAPTIVE;
    std::vector<double> sl(K * ld), su(K * ld), sorted, lower, upper;
    std::vector<int32_t> len(ld, 0), hlen(ld, 0), kept(n_groups, 0), st_learn(n_groups, CONFORMAL_OK), st_apply(n_groups, CONFORMAL_OK);
    Scratch scratch;
    try {
        if (!device_ready(out_batch_error)) return false;
        // time-major blocks [T x ld] and [H x ld]
        std::vector<double> blk(T * ld, 0.0);
        std::vector<uint8_t> vb;
        bool any_mask = false;
        for (size_t s = 0; s < n_groups; s++) any_mask = any_mask || (residual_validity && residual_validity[s] && residual_lengths[s] > 0);
        if (any_mask) vb.assign(T * ld, 1);
        for (size_t s = 0; s < n_groups; s++) len[s] = (int32_t)residual_lengths[s];
        pack_time_major(blk.data(), ld, residuals, residual_lengths, n_groups);
        if (any_mask) pack_validity(vb.data(), ld, residual_validity, residual_lengths, n_groups);
        double *d_r = scratch.get<double>(T * ld), *d_sl = scratch.get<double>(K * ld), *d_su = scratch.get<double>(K * ld);
        int32_t *d_len = scratch.get<int32_t>(ld), *d_kept = scratch.get<int32_t>(ld), *d_st = scratch.get<int32_t>(ld);
        uint8_t *d_valid = nullptr;
        double *d_sorted = nullptr;
        HIPCHECK(hipMemcpy(d_r, blk.data(), T * ld * sizeof(double), hipMemcpyHostToDevice));
        HIPCHECK(hipMemcpy(d_len, len.data(), ld * sizeof(int32_t), hipMemcpyHostToDevice));
        if (any_mask) {
            d_valid = scratch.get<uint8_t>(T * ld);
            HIPCHECK(hipMemcpy(d_valid, vb.data(), T * ld, hipMemcpyHostToDevice));
        }
        if (want_sorted) d_sorted = scratch.get<double>(T * ld);
        if (!anofox_hip_conformal_learn_device(d_r, nullptr, nullptr, d_valid, 1, ld, d_len, n_groups, T, alphas, K, method, d_sl, d_su, ld,
                                               d_sorted, d_kept, d_st, nullptr, out_batch_error))
            return false;
        HIPCHECK(hipMemcpy(sl.data(), d_sl, K * ld * sizeof(double), hipMemcpyDeviceToHost));
        HIPCHECK(hipMemcpy(su.data(), d_su, K * ld * sizeof(double), hipMemcpyDeviceToHost));
        HIPCHECK(hipMemcpy(kept.data(), d_kept, n_groups * sizeof(int32_t), hipMemcpyDeviceToHost));
        HIPCHECK(hipMemcpy(st_learn.data(), d_st, n_groups * sizeof(int32_t), hipMemcpyDeviceToHost));
        if (want_sorted) {
            sorted.resize(T * ld);
            HIPCHECK(hipMemcpy(sorted.data(), d_sorted, T * ld * sizeof(double), hipMemcpyDeviceToHost));
        }
        if (forecasts && H > 0) {
            std::vector<double> fb(H * ld, 0.0), db;
            if (adaptive) db.assign(H * ld, 1.0);
            for (size_t s = 0; s < n_groups; s++) hlen[s] = (int32_t)forecast_lengths[s];
            pack_time_major(fb.data(), ld, forecasts, forecast_lengths, n_groups);
            if (adaptive) pack_time_major(db.data(), ld, difficulty, forecast_lengths, n_groups);
            double *d_f = scratch.get<double>(H * ld), *d_lo = scratch.get<double>(K * H * ld), *d_up = scratch.get<double>(K * H * ld), *d_d = nullptr;
            int32_t *d_hlen = scratch.get<int32_t>(ld);
            HIPCHECK(hipMemcpy(d_f, fb.data(), H * ld * sizeof(double), hipMemcpyHostToDevice));
            HIPCHECK(hipMemcpy(d_hlen, hlen.data(), ld * sizeof(int32_t), hipMemcpyHostToDevice));
            if (adaptive) {
                d_d = scratch.get<double>(H * ld);
                HIPCHECK(hipMemcpy(d_d, db.data(), H * ld * sizeof(double), hipMemcpyHostToDevice));
            }
            if (!anofox_hip_conformal_apply_device(d_f, d_d, 1, ld, d_hlen, n_groups, H, d_sl, d_su, ld, K, method, d_lo, d_up, H * ld, d_st,
                                                   nullptr, out_batch_error))
                return false;
            lower.resize(K * H * ld); upper.resize(K * H * ld);
            HIPCHECK(hipMemcpy(lower.data(), d_lo, lower.size() * sizeof(double), hipMemcpyDeviceToHost));
            HIPCHECK(hipMemcpy(upper.data(), d_up, upper.size() * sizeof(double), hipMemcpyDeviceToHost));
            HIPCHECK(hipMemcpy(st_apply.data(), d_st, n_groups * sizeof(int32_t), hipMemcpyDeviceToHost));
        }
        scratch.settled();
    } catch (const HipFail &f) {
        report_hip_failure(out_batch_error, f);
        return false;
    }
    auto copy_out = [](size_t n) { return (double *)std::malloc(std::max<size_t>(n, 1) * sizeof(double)); };
    for (size_t s = 0; s < n_groups; s++) {
        AnofoxError *e = out_errors ? &out_errors[s] : nullptr;
        clear_error(e);
        const size_t h = forecasts ? forecast_lengths[s] : 0;
        // the order of the source's checks: conformal_learn first (no residual; the difficulty of the calibration set is not part of
        // this entry), then conformal_apply (no forecast, then the difficulty)
        if (st_learn[s] == CONFORMAL_EMPTY) { set_error(e, COMPUTATION_ERROR, CONFORMAL_EMPTY_TEXT); continue; }
        if (st_learn[s] == CONFORMAL_NAN) { set_error(e, COMPUTATION_ERROR, CONFORMAL_NAN_TEXT); continue; }
        if (forecasts && h == 0) { set_error(e, COMPUTATION_ERROR, CONFORMAL_NO_FORECAST_TEXT); continue; }
        if (forecasts && st_apply[s] == CONFORMAL_DIFFICULTY) { set_error(e, COMPUTATION_ERROR, CONFORMAL_DIFFICULTY_TEXT); continue; }
        AnofoxHipConformal r{};
        r.n_levels = K; r.n_residuals = (size_t)kept[s]; r.n_forecasts = h;
        r.scores_lower = copy_out(K); r.scores_upper = copy_out(K);
        if (want_sorted) r.sorted = copy_out(r.n_residuals);
        if (forecasts) { r.lower = copy_out(K * h); r.upper = copy_out(K * h); }
        if (!r.scores_lower || !r.scores_upper || (want_sorted && !r.sorted) || (forecasts && (!r.lower || !r.upper))) {
            anofox_hip_free_conformal(&r, 1);
            set_error(e, ALLOCATION_ERROR, "Failed to allocate the conformal result");
            continue;
        }
        for (size_t k = 0; k < K; k++) {
            r.scores_lower[k] = sl[k * ld + s]; r.scores_upper[k] = su[k * ld + s];
            for (size_t t = 0; t < h; t++) {
                r.lower[k * h + t] = lower[k * H * ld + t * ld + s];
                r.upper[k * h + t] = upper[k * H * ld + t * ld + s];
            }
        }
        for (size_t t = 0; want_sorted && t < r.n_residuals; t++) r.sorted[t] = sorted[t * ld + s];
        out_results[s] = r;
    }
    return true;
}

// ---- the reference's entries (lib.rs:4747-5400): each a batch of one through the same kernels ----
extern "C++" {
namespace {

const char *const CONFORMAL_ALPHA_V1_TEXT = "Invalid input: Alpha must be between 0 and 1 (exclusive)";      // conformal.rs:123-127


size_t conformal_count_valid(const uint64_t *validity, size_t n)
{
    if (!validity) return n;
    size_t c = 0;
    for (size_t t = 0; t < n; t++) c += (size_t)valid_bit(validity, t);
    return c;
}

// a malloc'ed copy, NULL for an empty array (vec_to_c_double_array)
double *conformal_copy(const double *p, size_t n)
{
    if (n == 0) return nullptr;
    double *q = (double *)std::malloc(n * sizeof(double));
    if (q) std::memcpy(q, p, n * sizeof(double));
    return q;
}

// learn (and apply, when forecasts != NULL) for ONE group through anofox_hip_conformal_batch; a failure of either kind -> out_error
bool conformal_one(const double *residuals, const uint64_t *validity, size_t n, const double *forecasts, const double *difficulty, size_t h,
                   const double *alphas, size_t n_alphas, int method, int strategy, bool want_sorted, AnofoxHipConformal *out,
                   AnofoxError *out_error)
{
    AnofoxError gerr, berr;
    const double *r[1] = {residuals}, *f[1] = {forecasts}, *d[1] = {difficulty};
    const uint64_t *v[1] = {validity};
    const size_t rl[1] = {n}, fl[1] = {h};
    if (!anofox_hip_conformal_batch(r, validity ? v : nullptr, rl, forecasts ? f : nullptr, difficulty ? d : nullptr, fl, 1, alphas, n_alphas, method,
                                    strategy, want_sorted, out, &gerr, &berr)) {
        if (out_error) *out_error = berr;
        return false;
    }
    if (gerr.code != SUCCESS) { if (out_error) *out_error = gerr; return false; }
    return true;
}

// apply alone for ONE group: bounds of every level around `forecasts` from host scores, through anofox_hip_conformal_apply_device
bool conformal_apply_one(const double *forecasts, const double *difficulty, size_t h, const double *scores_lower, const double *scores_upper,
                         size_t K, int method, std::vector<double> &lower, std::vector<double> &upper, int32_t &status, AnofoxError *out_error)
{
    lower.assign(K * h, 0.0); upper.assign(K * h, 0.0);
    status = CONFORMAL_OK;
    if (h == 0 || K == 0) return true;
    const size_t ld = 64;
    std::vector<double> sl(K * ld, 0.0), su(K * ld, 0.0);
    for (size_t k = 0; k < K; k++) { sl[k * ld] = scores_lower[k]; su[k * ld] = scores_upper[k]; }
    Scratch scratch;
    try {
        if (!device_ready(out_error)) return false;
        double *d_f = scratch.get<double>(h), *d_sl = scratch.get<double>(K * ld), *d_su = scratch.get<double>(K * ld), *d_d = nullptr;
        double *d_lo = scratch.get<double>(K * h), *d_up = scratch.get<double>(K * h);
        int32_t *d_st = scratch.get<int32_t>(ld);
        HIPCHECK(hipMemcpy(d_f, forecasts, h * sizeof(double), hipMemcpyHostToDevice));
        HIPCHECK(hipMemcpy(d_sl, sl.data(), K * ld * sizeof(double), hipMemcpyHostToDevice));
        HIPCHECK(hipMemcpy(d_su, su.data(), K * ld * sizeof(double), hipMemcpyHostToDevice));
        if (method == CONFORMAL_ADAPTIVE) {
            d_d = scratch.get<double>(h);
            HIPCHECK(hipMemcpy(d_d, difficulty, h * sizeof(double), hipMemcpyHostToDevice));
        }
        // one group, series-major: its steps are neighbours
        if (!anofox_hip_conformal_apply_device(d_f, d_d, h, 1, nullptr, 1, h, d_sl, d_su, ld, K, method, d_lo, d_up, h, d_st, nullptr, out_error))
            return false;
        HIPCHECK(hipMemcpy(lower.data(), d_lo, K * h * sizeof(double), hipMemcpyDeviceToHost));
        HIPCHECK(hipMemcpy(upper.data(), d_up, K * h * sizeof(double), hipMemcpyDeviceToHost));
        HIPCHECK(hipMemcpy(&status, d_st, sizeof(int32_t), hipMemcpyDeviceToHost));
        scratch.settled();
    } catch (const HipFail &f) {
        report_hip_failure(out_error, f);
        return false;
    }
    return true;
}

// the five evaluation figures of ONE group through anofox_hip_conformal_evaluate_device (n > 0)
bool conformal_evaluate_one(const double *actuals, const double *lower, const double *upper, size_t n, double alpha, double *fig,
                            AnofoxError *out_error)
{
    const size_t ld = 64;
    Scratch scratch;
    try {
        if (!device_ready(out_error)) return false;
        const int32_t len = (int32_t)n;
        double *d_a = scratch.get<double>(n), *d_l = scratch.get<double>(n), *d_u = scratch.get<double>(n);
        double *d_fig = scratch.get<double>(CONFORMAL_N_EVAL * ld);
        int32_t *d_len = scratch.get<int32_t>(ld), *d_st = scratch.get<int32_t>(ld);
        HIPCHECK(hipMemcpy(d_a, actuals, n * sizeof(double), hipMemcpyHostToDevice));
        HIPCHECK(hipMemcpy(d_l, lower, n * sizeof(double), hipMemcpyHostToDevice));
        HIPCHECK(hipMemcpy(d_u, upper, n * sizeof(double), hipMemcpyHostToDevice));
        HIPCHECK(hipMemcpy(d_len, &len, sizeof len, hipMemcpyHostToDevice));
        if (!anofox_hip_conformal_evaluate_device(d_a, d_l, d_u, n, 1, d_len, 1, n, alpha, d_fig, ld, d_st, nullptr, out_error)) return false;
        for (int k = 0; k < CONFORMAL_N_EVAL; k++) HIPCHECK(hipMemcpy(&fig[k], d_fig + (size_t)k * ld, sizeof(double), hipMemcpyDeviceToHost));
        scratch.settled();
    } catch (const HipFail &f) {
        report_hip_failure(out_error, f);
        return false;
    }
    return true;
}

bool conformal_too_many(size_t n_alphas, AnofoxError *err)
{
    if (n_alphas <= (size_t)CONFORMAL_MAX_LEVELS) return false;
    set_error(err, INVALID_INPUT, "Invalid input: at most " + std::to_string(CONFORMAL_MAX_LEVELS) + " coverage levels per call, got " +
                                      std::to_string(n_alphas));
    return true;
}

void conformal_method_name(ConformalResultFFI *out, const char *name)
{
    std::memset(out->method, 0, sizeof out->method);
    std::strncpy(out->method, name, sizeof out->method - 1);
}

// conformal_predict / _adaptive / _asymmetric behind their checks: one alpha, one group
bool conformal_predict_one(const double *residuals, const uint64_t *validity, size_t n, const double *forecasts, const double *difficulty,
                           size_t h, double alpha, int method, const char *name, ConformalResultFFI *out, AnofoxError *out_error)
{
    if (conformal_count_valid(validity, n) == 0) { set_error(out_error, COMPUTATION_ERROR, CONFORMAL_EMPTY_TEXT); return false; }
    if (!conformal_alpha_ok(alpha)) { set_error(out_error, COMPUTATION_ERROR, CONFORMAL_ALPHA_V1_TEXT); return false; }
    AnofoxHipConformal r{};
    // a forecast list may be empty here (the source answers with empty bounds): learn alone then
    if (!conformal_one(residuals, validity, n, h ? forecasts : nullptr, h ? difficulty : nullptr, h, &alpha, 1, method, 0, false, &r, out_error))
        return false;
    std::memset(out, 0, sizeof *out);
    out->point = conformal_copy(forecasts, h);
    out->lower = conformal_copy(r.lower, h);
    out->upper = conformal_copy(r.upper, h);
    out->n_forecasts = h;
    out->coverage = 1.0 - alpha;
    out->conformity_score = method == CONFORMAL_ASYMMETRIC ? (r.scores_upper[0] + r.scores_lower[0]) / 2.0 : r.scores_lower[0];
    conformal_method_name(out, name);
    anofox_hip_free_conformal(&r, 1);
    if (h > 0 && (!out->point || !out->lower || !out->upper)) {
        anofox_free_conformal_result(out);
        set_error(out_error, ALLOCATION_ERROR, "Failed to allocate the conformal result");
        return false;
    }
    return true;
}

} // namespace
} // extern "C++"

void anofox_free_conformal_result(ConformalResultFFI *r)
{
    if (!r) return;
    std::free(r->point); r->point = nullptr;
    std::free(r->lower); r->lower = nullptr;
    std::free(r->upper); r->upper = nullptr;
}

void anofox_free_conformal_multi_result(ConformalMultiResultFFI *r)
{
    if (!r) return;
    std::free(r->point); r->point = nullptr;
    std::free(r->coverage_levels); r->coverage_levels = nullptr;
    std::free(r->conformity_scores); r->conformity_scores = nullptr;
    std::free(r->lower); r->lower = nullptr;
    std::free(r->upper); r->upper = nullptr;
}

void anofox_free_calibration_profile(CalibrationProfileFFI *r)
{
    if (!r) return;
    std::free(r->alphas); r->alphas = nullptr;
    std::free(r->state_vector); r->state_vector = nullptr;
    std::free(r->scores_lower); r->scores_lower = nullptr;
    std::free(r->scores_upper); r->scores_upper = nullptr;
}

void anofox_free_prediction_intervals(PredictionIntervalsFFI *r)
{
    if (!r) return;
    std::free(r->point); r->point = nullptr;
    std::free(r->coverage); r->coverage = nullptr;
    std::free(r->lower); r->lower = nullptr;
    std::free(r->upper); r->upper = nullptr;
}

bool anofox_ts_conformal_quantile(const double *residuals, const uint64_t *validity, size_t length, double alpha, double *out_result,
                                  AnofoxError *out_error)
{
    clear_error(out_error);
    if (!residuals) { set_error(out_error, NULL_POINTER, "Null pointer argument"); return false; }
    if (!out_result) { set_error(out_error, NULL_POINTER, "Null output pointer"); return false; }
    if (conformal_count_valid(validity, length) == 0) { set_error(out_error, COMPUTATION_ERROR, CONFORMAL_EMPTY_TEXT); return false; }
    if (!conformal_alpha_ok(alpha)) { set_error(out_error, COMPUTATION_ERROR, CONFORMAL_ALPHA_V1_TEXT); return false; }
    AnofoxHipConformal r{};
    if (!conformal_one(residuals, validity, length, nullptr, nullptr, 0, &alpha, 1, CONFORMAL_SYMMETRIC, 0, false, &r, out_error)) return false;
    *out_result = r.scores_lower[0];
    anofox_hip_free_conformal(&r, 1);
    return true;
}

bool anofox_ts_conformal_intervals(const double *forecasts, size_t length, double conformity_score, double **out_lower, double **out_upper,
                                   AnofoxError *out_error)
{
    clear_error(out_error);
    if (!forecasts || !out_lower || !out_upper) { set_error(out_error, NULL_POINTER, "Null pointer argument"); return false; }
    std::vector<double> lo, up;
    int32_t status;
    if (!conformal_apply_one(forecasts, nullptr, length, &conformity_score, &conformity_score, 1, CONFORMAL_SYMMETRIC, lo, up, status, out_error))
        return false;
    double *l = conformal_copy(lo.data(), length), *u = conformal_copy(up.data(), length);
    if (length > 0 && (!l || !u)) {
        std::free(l); std::free(u);
        set_error(out_error, ALLOCATION_ERROR, l ? "Failed to allocate upper bounds" : "Failed to allocate lower bounds");
        return false;
    }
    *out_lower = l; *out_upper = u;
    return true;
}

bool anofox_ts_conformal_predict(const double *residuals, const uint64_t *residuals_validity, size_t residuals_length, const double *forecasts,
                                 size_t forecasts_length, double alpha, ConformalResultFFI *out_result, AnofoxError *out_error)
{
    clear_error(out_error);
    if (!residuals || !forecasts || !out_result) { set_error(out_error, NULL_POINTER, "Null pointer argument"); return false; }
    return conformal_predict_one(residuals, residuals_validity, residuals_length, forecasts, nullptr, forecasts_length, alpha, CONFORMAL_SYMMETRIC,
                                 "split_conformal", out_result, out_error);
}

bool anofox_ts_conformal_predict_adaptive(const double *residuals, const uint64_t *residuals_validity, size_t residuals_length,
                                          const double *forecasts, const double *difficulty, size_t forecasts_length, double alpha,
                                          ConformalResultFFI *out_result, AnofoxError *out_error)
{
    clear_error(out_error);
    if (!residuals || !forecasts || !difficulty || !out_result) { set_error(out_error, NULL_POINTER, "Null pointer argument"); return false; }
    for (size_t t = 0; t < forecasts_length; t++)                  // before the quantile's own checks (conformal.rs:315-323)
        if (difficulty[t] <= 0.0) { set_error(out_error, COMPUTATION_ERROR, CONFORMAL_DIFFICULTY_TEXT); return false; }
    return conformal_predict_one(residuals, residuals_validity, residuals_length, forecasts, difficulty, forecasts_length, alpha, CONFORMAL_ADAPTIVE,
                                 "adaptive_conformal", out_result, out_error);
}

bool anofox_ts_conformal_predict_asymmetric(const double *residuals, const uint64_t *residuals_validity, size_t residuals_length,
                                            const double *forecasts, size_t forecasts_length, double alpha, ConformalResultFFI *out_result,
                                            AnofoxError *out_error)
{
    clear_error(out_error);
    if (!residuals || !forecasts || !out_result) { set_error(out_error, NULL_POINTER, "Null pointer argument"); return false; }
    return conformal_predict_one(residuals, residuals_validity, residuals_length, forecasts, nullptr, forecasts_length, alpha, CONFORMAL_ASYMMETRIC,
                                 "asymmetric_conformal", out_result, out_error);
}

bool anofox_ts_conformal_predict_multi(const double *residuals, const uint64_t *residuals_validity, size_t residuals_length,
                                       const double *forecasts, size_t forecasts_length, const double *alphas, size_t n_alphas,
                                       ConformalMultiResultFFI *out_result, AnofoxError *out_error)
{
    clear_error(out_error);
    if (!residuals || !forecasts || !alphas || !out_result) { set_error(out_error, NULL_POINTER, "Null pointer argument"); return false; }
    if (conformal_too_many(n_alphas, out_error)) return false;
    if (n_alphas == 0) { set_error(out_error, COMPUTATION_ERROR, CONFORMAL_NO_ALPHA_TEXT); return false; }
    if (conformal_count_valid(residuals_validity, residuals_length) == 0) { set_error(out_error, COMPUTATION_ERROR, CONFORMAL_EMPTY_TEXT); return false; }
    for (size_t k = 0; k < n_alphas; k++)
        if (!conformal_alpha_ok(alphas[k])) { set_error(out_error, COMPUTATION_ERROR, CONFORMAL_ALPHA_V1_TEXT); return false; }
    const size_t h = forecasts_length;
    AnofoxHipConformal r{};
    if (!conformal_one(residuals, residuals_validity, residuals_length, h ? forecasts : nullptr, nullptr, h, alphas, n_alphas, CONFORMAL_SYMMETRIC, 0,
                       false, &r, out_error))
        return false;
    std::memset(out_result, 0, sizeof *out_result);
    out_result->point = conformal_copy(forecasts, h);
    out_result->n_forecasts = h;
    out_result->n_levels = n_alphas;
    out_result->coverage_levels = (double *)std::malloc(n_alphas * sizeof(double));
    out_result->conformity_scores = conformal_copy(r.scores_lower, n_alphas);
    out_result->lower = conformal_copy(r.lower, n_alphas * h);
    out_result->upper = conformal_copy(r.upper, n_alphas * h);
    anofox_hip_free_conformal(&r, 1);
    if (!out_result->coverage_levels || !out_result->conformity_scores || (h > 0 && (!out_result->point || !out_result->lower || !out_result->upper))) {
        anofox_free_conformal_multi_result(out_result);
        set_error(out_error, ALLOCATION_ERROR, "Failed to allocate the conformal result");
        return false;
    }
    for (size_t k = 0; k < n_alphas; k++) out_result->coverage_levels[k] = 1.0 - alphas[k];
    return true;
}

bool anofox_ts_mean_interval_width(const double *lower, const double *upper, size_t length, double *out_result, AnofoxError *out_error)
{
    clear_error(out_error);
    if (!lower || !upper || !out_result) { set_error(out_error, NULL_POINTER, "Null pointer argument"); return false; }
    if (length == 0) { *out_result = std::numeric_limits<double>::quiet_NaN(); return true; }          // conformal.rs:461-463
    double fig[CONFORMAL_N_EVAL];
    if (!conformal_evaluate_one(lower, lower, upper, length, 0.5, fig, out_error)) return false;
    *out_result = fig[2];
    return true;
}

bool anofox_ts_conformal_learn(const double *residuals, const uint64_t *residuals_validity, size_t residuals_length, const double *alphas,
                               size_t n_alphas, ConformalMethodFFI method, ConformalStrategyFFI strategy, const double *difficulty,
                               CalibrationProfileFFI *out_profile, AnofoxError *out_error)
{
    clear_error(out_error);
    if (!residuals || !alphas || !out_profile) { set_error(out_error, NULL_POINTER, "Null pointer argument"); return false; }
    if (conformal_too_many(n_alphas, out_error) || !conformal_check_method((int)method, out_error)) return false;
    if ((int)strategy < 0 || (int)strategy > 2) {
        set_error(out_error, INVALID_INPUT, "Invalid input: unknown conformal strategy (0 split, 1 crossval, 2 jackknife+)");
        return false;
    }
    // conformal_learn's checks in its order (conformal.rs:702-750)
    const size_t kept = conformal_count_valid(residuals_validity, residuals_length);
    if (kept == 0) { set_error(out_error, COMPUTATION_ERROR, CONFORMAL_EMPTY_TEXT); return false; }
    if (n_alphas == 0) { set_error(out_error, COMPUTATION_ERROR, CONFORMAL_NO_ALPHA_TEXT); return false; }
    for (size_t k = 0; k < n_alphas; k++)
        if (!conformal_alpha_ok(alphas[k])) {
            set_error(out_error, COMPUTATION_ERROR, "Invalid input: Alpha must be in (0, 1), got " + conformal_show(alphas[k]));
            return false;
        }
    if ((int)method == CONFORMAL_ADAPTIVE) {
        if (!difficulty) { set_error(out_error, COMPUTATION_ERROR, CONFORMAL_NEED_DIFFICULTY_TEXT); return false; }
        if (residuals_length != kept) {                            // the difficulty keeps the list's length, the residuals lost their NULLs
            set_error(out_error, COMPUTATION_ERROR, "Invalid input: Difficulty length (" + std::to_string(residuals_length) +
                                                        ") must match residuals length (" + std::to_string(kept) + ")");
            return false;
        }
        for (size_t t = 0; t < residuals_length; t++)
            if (difficulty[t] <= 0.0) { set_error(out_error, COMPUTATION_ERROR, CONFORMAL_DIFFICULTY_TEXT); return false; }
    }
    if ((int)strategy == 2 && (int)method == CONFORMAL_ASYMMETRIC) {
        set_error(out_error, COMPUTATION_ERROR, "Invalid input: JackknifePlus strategy does not support asymmetric method");
        return false;
    }
    const bool jk = (int)strategy == 2;
    AnofoxHipConformal r{};
    if (!conformal_one(residuals, residuals_validity, residuals_length, nullptr, nullptr, 0, alphas, n_alphas, (int)method, (int)strategy, jk, &r,
                       out_error))
        return false;
    std::memset(out_profile, 0, sizeof *out_profile);
    out_profile->method = method; out_profile->strategy = strategy;
    out_profile->alphas = conformal_copy(alphas, n_alphas);
    out_profile->scores_lower = conformal_copy(r.scores_lower, n_alphas);
    out_profile->scores_upper = conformal_copy(r.scores_upper, n_alphas);
    out_profile->n_levels = n_alphas;
    out_profile->n_residuals = r.n_residuals;
    if (jk) {
        out_profile->state_vector_len = r.n_residuals;
        out_profile->state_vector = conformal_copy(r.sorted, r.n_residuals);
    } else {
        out_profile->state_vector_len = 2 * n_alphas;
        out_profile->state_vector = (double *)std::malloc(2 * n_alphas * sizeof(double));
        if (out_profile->state_vector) {
            std::memcpy(out_profile->state_vector, r.scores_lower, n_alphas * sizeof(double));
            std::memcpy(out_profile->state_vector + n_alphas, r.scores_upper, n_alphas * sizeof(double));
        }
    }
    anofox_hip_free_conformal(&r, 1);
    if (!out_profile->alphas || !out_profile->scores_lower || !out_profile->scores_upper || !out_profile->state_vector) {
        anofox_free_calibration_profile(out_profile);
        set_error(out_error, ALLOCATION_ERROR, "Failed to allocate the calibration profile");
        return false;
    }
    return true;
}

bool anofox_ts_conformal_apply(const double *forecasts, size_t n_forecasts, const CalibrationProfileFFI *profile, const double *difficulty,
                               PredictionIntervalsFFI *out_intervals, AnofoxError *out_error)
{
    clear_error(out_error);
    if (!forecasts || !profile || !out_intervals) { set_error(out_error, NULL_POINTER, "Null pointer argument"); return false; }
    const size_t K = profile->n_levels, h = n_forecasts;
    const int method = (int)profile->method;
    if (conformal_too_many(K, out_error) || !conformal_check_method(method, out_error)) return false;
    if (K > 0 && (!profile->alphas || !profile->scores_lower || !profile->scores_upper)) {
        set_error(out_error, NULL_POINTER, "Null pointer argument");
        return false;
    }
    // conformal_apply's checks in its order (conformal.rs:897-925)
    if (h == 0) { set_error(out_error, COMPUTATION_ERROR, CONFORMAL_NO_FORECAST_TEXT); return false; }
    if (method == CONFORMAL_ADAPTIVE) {
        if (!difficulty) { set_error(out_error, COMPUTATION_ERROR, CONFORMAL_NEED_DIFFICULTY_TEXT); return false; }
        for (size_t t = 0; t < h; t++)
            if (difficulty[t] <= 0.0) { set_error(out_error, COMPUTATION_ERROR, CONFORMAL_DIFFICULTY_TEXT); return false; }
    }
    std::vector<double> sl(profile->scores_lower, profile->scores_lower + K), su(profile->scores_upper, profile->scores_upper + K), lo, up;
    if ((int)profile->strategy == 2 && K > 0) {
        // Jackknife+: the scores come from the stored residual distribution at apply time (conformal.rs:941-954); it is sorted and not
        // negative, so learning from it sorts it into itself
        if (profile->state_vector && profile->state_vector_len > 0) {
            AnofoxHipConformal r{};
            if (!conformal_one(profile->state_vector, nullptr, profile->state_vector_len, nullptr, nullptr, 0, profile->alphas, K, CONFORMAL_SYMMETRIC,
                               0, false, &r, out_error))
                return false;
            for (size_t k = 0; k < K; k++) sl[k] = su[k] = r.scores_lower[k];
            anofox_hip_free_conformal(&r, 1);
        } else {
            for (size_t k = 0; k < K; k++) sl[k] = su[k] = std::numeric_limits<double>::quiet_NaN();   // compute_quantile of nothing
        }
    }
    int32_t status;
    if (!conformal_apply_one(forecasts, difficulty, h, sl.data(), su.data(), K, method, lo, up, status, out_error)) return false;
    std::memset(out_intervals, 0, sizeof *out_intervals);
    out_intervals->point = conformal_copy(forecasts, h);
    out_intervals->n_forecasts = h;
    out_intervals->n_levels = K;
    out_intervals->coverage = (double *)std::malloc(std::max<size_t>(K, 1) * sizeof(double));
    out_intervals->lower = (double *)std::malloc(std::max<size_t>(K * h, 1) * sizeof(double));
    out_intervals->upper = (double *)std::malloc(std::max<size_t>(K * h, 1) * sizeof(double));
    out_intervals->method = profile->method;
    if (!out_intervals->point || !out_intervals->coverage || !out_intervals->lower || !out_intervals->upper) {
        anofox_free_prediction_intervals(out_intervals);
        set_error(out_error, ALLOCATION_ERROR, "Failed to allocate the prediction intervals");
        return false;
    }
    for (size_t k = 0; k < K; k++) out_intervals->coverage[k] = 1.0 - profile->alphas[k];
    std::memcpy(out_intervals->lower, lo.data(), K * h * sizeof(double));
    std::memcpy(out_intervals->upper, up.data(), K * h * sizeof(double));
    return true;
}

bool anofox_ts_conformal_coverage(const double *actuals, const double *lower, const double *upper, size_t length, double *out_coverage,
                                  AnofoxError *out_error)
{
    clear_error(out_error);
    if (!actuals || !lower || !upper || !out_coverage) { set_error(out_error, NULL_POINTER, "Null pointer argument"); return false; }
    if (length == 0) { set_error(out_error, COMPUTATION_ERROR, CONFORMAL_EMPTY_TEXT); return false; }
    double fig[CONFORMAL_N_EVAL];
    if (!conformal_evaluate_one(actuals, lower, upper, length, 0.5, fig, out_error)) return false;
    *out_coverage = fig[0];
    return true;
}

bool anofox_ts_conformal_evaluate(const double *actuals, const double *lower, const double *upper, size_t length, double alpha,
                                  ConformalEvaluationFFI *out_eval, AnofoxError *out_error)
{
    clear_error(out_error);
    if (!actuals || !lower || !upper || !out_eval) { set_error(out_error, NULL_POINTER, "Null pointer argument"); return false; }
    if (length == 0) { set_error(out_error, COMPUTATION_ERROR, CONFORMAL_EMPTY_TEXT); return false; }
    if (!conformal_alpha_ok(alpha)) {                              // winkler_score's check, after coverage has succeeded (conformal.rs:1123-1128)
        set_error(out_error, COMPUTATION_ERROR, "Invalid input: Alpha must be in (0, 1), got " + conformal_show(alpha));
        return false;
    }
    double fig[CONFORMAL_N_EVAL];
    if (!conformal_evaluate_one(actuals, lower, upper, length, alpha, fig, out_error)) return false;
    out_eval->coverage = fig[0]; out_eval->violation_rate = fig[1]; out_eval->mean_width = fig[2]; out_eval->winkler_score = fig[3];
    out_eval->n_observations = length;
    return true;
}

// ------------------------------------------------------------------------------------------------------------------------------
// Exogenous regressors: ARIMAX (forecast.rs forecast_with_exog; fit_exog.hip)
// ------------------------------------------------------------------------------------------------------------------------------
} // extern "C"

namespace {

// what forecast_with_exog does with a model when regressors are present (forecast.rs:803-840)
enum ExogRoute { EXOG_IGNORED = 0, EXOG_ARIMAX = 1, EXOG_NOT_IMPLEMENTED = 2 };
ExogRoute exog_route(ModelType m)
{
    switch (m) {
    case M_ARIMA: case M_AutoARIMA: return EXOG_ARIMAX;
    case M_OptimizedTheta: case M_DynamicTheta: case M_MFLES: case M_AutoMFLES: return EXOG_NOT_IMPLEMENTED;     // ThetaX / MFLESX: DESIGN section 7
    default: return EXOG_IGNORED;
    }
}

std::string exog_not_implemented_message(ModelType m)
{
    return std::string("Internal error: model '") + model_name(m) + "' with exogenous regressors (" +
           ((m == M_MFLES || m == M_AutoMFLES) ? "MFLESX" : "ThetaX") + ") is not implemented by the HIP backend";
}

std::string exog_cap_message(size_t k)
{
    return "Computation error: ARIMAX takes at most " + std::to_string(EXOG_MAX_REGRESSORS) + " exogenous regressors, got " + std::to_string(k);
}


// host regressors -> the batch's own device blocks, through one pinned staging block per regressor slice (cells past a series' end: 0.0)
void batch_pack_exog_host(AnofoxHipBatch *b, const double *const *xreg, const double *const *future_xreg, const size_t *lengths, size_t k)
{
    const size_t n = b->n, ld = b->ld, T = std::max<size_t>(b->t_max, 1), h = (size_t)std::max(b->h, 0);
    double *d_x = dalloc<double>(k * T * ld), *d_f = nullptr;
    void *stage = nullptr;
    try {
        d_f = dalloc<double>(k * h * ld);
        stage = pin_alloc_bytes(std::max(T, k * h) * ld * sizeof(double));
        double *st = (double *)stage;
        batch_attach_streams(b);
        unsigned n_thr = std::max(1u, std::min(std::thread::hardware_concurrency(), 16u));
        if (tl_host_thread_share > 1) n_thr = std::max(1u, n_thr / tl_host_thread_share);
        if (T * ld < (1u << 20)) n_thr = 1;
        const size_t n_tiles = ld / 64;
        for (size_t j = 0; j < k; j++) {
            auto fill = [&](size_t tile0, size_t tile1) {
                for (size_t tile = tile0; tile < tile1; tile++)
                    for (size_t t = 0; t < T; t++) {
                        double *row = st + t * ld + tile * 64;
                        for (size_t c = 0; c < 64; c++) {
                            const size_t s = tile * 64 + c;
                            row[c] = (s < n && t < lengths[s]) ? xreg[s * k + j][t] : 0.0;
                        }
                    }
            };
            if (n_thr <= 1) fill(0, n_tiles);
            else parallel_shares(n_thr, [&](unsigned q) { fill(n_tiles * q / n_thr, n_tiles * (q + 1) / n_thr); });
            HIPCHECK(hipMemcpyAsync(d_x + j * T * ld, st, T * ld * sizeof(double), hipMemcpyHostToDevice, b->own_stream));
            HIPCHECK(hipStreamSynchronize(b->own_stream));         // the staging block is refilled for the next regressor
        }
        if (h) {
            for (size_t j = 0; j < k; j++)
                for (size_t i = 0; i < h; i++)
                    for (size_t s = 0; s < ld; s++) st[(j * h + i) * ld + s] = s < n ? future_xreg[s * k + j][i] : 0.0;
            HIPCHECK(hipMemcpyAsync(d_f, st, k * h * ld * sizeof(double), hipMemcpyHostToDevice, b->own_stream));
            HIPCHECK(hipStreamSynchronize(b->own_stream));
        }
    } catch (...) {
        (void)hipStreamSynchronize(b->own_stream);
        pin_free(stage);
        dev_free(d_x); dev_free(d_f);
        throw;
    }
    pin_free(stage);
    if (b->owns_exog) { dev_free((void *)b->d_exog_x); dev_free((void *)b->d_exog_f); }
    b->d_exog_x = d_x; b->d_exog_f = d_f; b->owns_exog = true; b->exog_k = (int)k;
}

} // namespace

extern "C" {

bool anofox_hip_batch_set_exog_device(AnofoxHipBatch *b, const void *d_x, const void *d_future, size_t k, AnofoxError *out_error)
{
    clear_error(out_error);
    if (!b) { set_error(out_error, NULL_POINTER, "Null pointer argument"); return false; }
    if (k > 0 && (!d_x || (!d_future && b->h > 0))) { set_error(out_error, NULL_POINTER, "Null pointer argument"); return false; }
    if (k > (size_t)EXOG_MAX_REGRESSORS) { set_error(out_error, COMPUTATION_ERROR, exog_cap_message(k)); return false; }
    DeviceGuard guard(b->dev);
    if (b->owns_exog) {
        // (a run that reads the owned blocks may still be in flight)
        if (!b->quiesced && b->last_stream) (void)hipStreamSynchronize(b->last_stream);
        dev_free((void *)b->d_exog_x); dev_free((void *)b->d_exog_f);
        b->owns_exog = false;
    }
    b->d_exog_x = k ? (const double *)d_x : nullptr;
    b->d_exog_f = k ? (const double *)d_future : nullptr;
    b->exog_k = (int)k;
    return true;
}

bool anofox_hip_batch_exog_coefficients(AnofoxHipBatch *b, double *out_intercept, double *out_beta, uint32_t *out_used, AnofoxError *out_error)
{
    clear_error(out_error);
    if (!b) { set_error(out_error, NULL_POINTER, "Null pointer argument"); return false; }
    if (!b->ran || !exog_in_force(b) || !b->d_exog_b0) {
        set_error(out_error, INVALID_INPUT, "Invalid input: the batch's last run did not take the ARIMAX path");
        return false;
    }
    DeviceGuard guard(b->dev);
    try {
        const size_t n = b->n, ld = b->ld, k = (size_t)b->exog_k;
        HIPCHECK(hipStreamSynchronize(b->last_stream));
        std::vector<int32_t> status(n);
        HIPCHECK(hipMemcpy(status.data(), b->d_status, n * sizeof(int32_t), hipMemcpyDeviceToHost));
        const double nan = std::numeric_limits<double>::quiet_NaN();
        if (out_intercept) {
            HIPCHECK(hipMemcpy(out_intercept, b->d_exog_b0, n * sizeof(double), hipMemcpyDeviceToHost));
            for (size_t s = 0; s < n; s++) if (status[s] != 0) out_intercept[s] = nan;
        }
        if (out_beta) {
            std::vector<double> beta(k * ld);
            HIPCHECK(hipMemcpy(beta.data(), b->d_exog_beta, k * ld * sizeof(double), hipMemcpyDeviceToHost));
            for (size_t s = 0; s < n; s++)
                for (size_t j = 0; j < k; j++) out_beta[s * k + j] = status[s] != 0 ? nan : beta[j * ld + s];
        }
        if (out_used) {
            HIPCHECK(hipMemcpy(out_used, b->d_exog_used, n * sizeof(uint32_t), hipMemcpyDeviceToHost));
            for (size_t s = 0; s < n; s++) if (status[s] != 0) out_used[s] = 0u;
        }
    } catch (const HipFail &f) {
        report_hip_failure(out_error, f);
        return false;
    }
    return true;
}

bool anofox_ts_forecast_exog_batch(const double *const *values, const uint64_t *const *validity, const size_t *lengths, size_t n_series,
                                   const ForecastOptions *options, size_t n_regressors, const double *const *xreg,
                                   const double *const *future_xreg, ForecastResult *out_results, AnofoxError *out_errors,
                                   AnofoxError *out_batch_error, double *out_coefficients, uint32_t *out_used)
{
    clear_error(out_batch_error);
    if (!values || !lengths || !options || !out_results) { set_error(out_batch_error, NULL_POINTER, "Null pointer argument"); return false; }
    ModelType mt = M_Naive;
    {
        const std::string mname = cstr_field(options->model, sizeof options->model);
        if (!parse_model(mname, mt)) {
            AnofoxError me;
            set_error(&me, INVALID_MODEL, "Invalid model: Unknown model: '" + mname + "'");
            if (out_batch_error) *out_batch_error = me;
            for (size_t s = 0; s < n_series; s++) { std::memset(&out_results[s], 0, sizeof(ForecastResult)); if (out_errors) out_errors[s] = me; }
            return false;
        }
    }
    const size_t K = n_regressors;
    const ExogRoute route = K == 0 ? EXOG_IGNORED : exog_route(mt);
    // no regressors, or a model that ignores them: the ordinary batch path (forecast.rs:840-855)
    if (route == EXOG_IGNORED) {
        if (out_coefficients) for (size_t i = 0; i < n_series * (K + 1); i++) out_coefficients[i] = std::numeric_limits<double>::quiet_NaN();
        if (out_used) for (size_t s = 0; s < n_series; s++) out_used[s] = 0u;
        return anofox_ts_forecast_batch(values, validity, lengths, n_series, options, nullptr, out_results, out_errors, out_batch_error);
    }
    for (size_t s = 0; s < n_series; s++) {
        std::memset(&out_results[s], 0, sizeof(ForecastResult));
        clear_error(out_errors ? &out_errors[s] : nullptr);
    }
    auto fail_all = [&](int code, const std::string &msg) {
        AnofoxError fe;
        clear_error(&fe);
        set_error(&fe, code, msg);
        if (out_batch_error) *out_batch_error = fe;
        option_error_per_series(out_errors, lengths, n_series, fe);        // the length checks come before the model's own
        return false;
    };
    if (options->horizon < 0) return fail_all(PANIC_CAUGHT, "Panic in Rust code");
    if (!xreg || (!future_xreg && options->horizon > 0)) { set_error(out_batch_error, NULL_POINTER, "Null pointer argument"); return false; }
    for (size_t s = 0; s < n_series; s++) {
        if (!values[s]) { set_error(out_batch_error, NULL_POINTER, "Null pointer argument"); return false; }
        for (size_t j = 0; j < K; j++)
            if ((!xreg[s * K + j] && lengths[s] > 0) || (options->horizon > 0 && !future_xreg[s * K + j])) {
                set_error(out_batch_error, NULL_POINTER, "Null pointer argument");
                return false;
            }
    }
    if (route == EXOG_NOT_IMPLEMENTED) return fail_all(INTERNAL_ERROR, exog_not_implemented_message(mt));
    if (K > (size_t)EXOG_MAX_REGRESSORS) return fail_all(COMPUTATION_ERROR, exog_cap_message(K));
    if (n_series == 0) return true;
    // ARIMAX is the same for ARIMA and AutoARIMA (no search, no period), and so are their fitted values (forecast.rs:2593-2643): the
    // batch is planned as ARIMA, which spares AutoARIMA's search workspace; forecast_with_model takes no seasonal_period check
    ForecastOptions opt = *options;
    std::memset(opt.model, 0, sizeof opt.model);
    std::snprintf(opt.model, sizeof opt.model, "%s", "ARIMA");
    opt.seasonal_period = 0;
    opt.auto_detect_seasonality = false;
    size_t t_max = 0;
    for (size_t s = 0; s < n_series; s++) t_max = std::max(t_max, lengths[s]);
    AnofoxHipBatch *b = nullptr;
    AnofoxError e;
    clear_error(&e);
    if (!anofox_hip_batch_create(n_series, t_max, &opt, &b, &e)) return fail_all(e.code, e.message);
    bool ok = run_batch(b, values, validity, lengths, out_results, out_errors, &e, nullptr, [&] {
        DeviceGuard guard(b->dev);
        batch_pack_exog_host(b, xreg, future_xreg, lengths, K);
    });
    if (ok && (out_coefficients || out_used)) {
        std::vector<double> b0(n_series), beta(n_series * K);
        ok = anofox_hip_batch_exog_coefficients(b, b0.data(), beta.data(), out_used, &e);
        if (ok && out_coefficients)
            for (size_t s = 0; s < n_series; s++) {
                out_coefficients[s * (K + 1)] = b0[s];
                for (size_t j = 0; j < K; j++) out_coefficients[s * (K + 1) + 1 + j] = beta[s * K + j];
            }
    }
    anofox_hip_batch_destroy(b);
    if (!ok) {
        if (e.code == SUCCESS) set_error(&e, INTERNAL_ERROR, "Internal error: device batch failed");
        if (out_batch_error) *out_batch_error = e;
        return false;
    }
    return true;
}

bool anofox_ts_forecast_exog(const double *values, const uint64_t *validity, size_t length, const ForecastOptionsExog *options,
                             ForecastResult *out_result, AnofoxError *out_error)
{
    clear_error(out_error);
    if (!values || !options || !out_result) { set_error(out_error, NULL_POINTER, "Null pointer argument"); return false; }
    // the order of the reference (lib.rs:3603-3668, forecast.rs:772-789): model name, regressor lengths, series length
    const std::string mname = cstr_field(options->model, sizeof options->model);
    ModelType mt;
    if (!parse_model(mname, mt)) { set_error(out_error, INVALID_MODEL, "Invalid model: Unknown model: '" + mname + "'"); return false; }
    if (options->horizon < 0) { set_error(out_error, PANIC_CAUGHT, "Panic in Rust code"); return false; }
    size_t K = 0;
    if (options->exog && options->exog->n_regressors > 0) {
        K = options->exog->n_regressors;
        if (!options->exog->regressors) { set_error(out_error, NULL_POINTER, "Null pointer argument"); return false; }
        for (size_t i = 0; i < K; i++) {
            const ExogenousRegressor &r = options->exog->regressors[i];
            if (r.n_values != length) {
                set_error(out_error, INVALID_INPUT, "Invalid input: Exogenous regressor " + std::to_string(i) + " has " + std::to_string(r.n_values) +
                                                        " values but y has " + std::to_string(length) + " values");
                return false;
            }
            if (r.n_future != (size_t)options->horizon) {
                set_error(out_error, INVALID_INPUT, "Invalid input: Exogenous regressor " + std::to_string(i) + " has " + std::to_string(r.n_future) +
                                                        " future values but horizon is " + std::to_string(options->horizon));
                return false;
            }
            if ((!r.values && r.n_values > 0) || (!r.future_values && r.n_future > 0)) { set_error(out_error, NULL_POINTER, "Null pointer argument"); return false; }
        }
    }
    if (series_too_short(out_error, length)) return false;
    ForecastOptions opt;
    std::memset(&opt, 0, sizeof opt);
    std::memcpy(opt.model, options->model, sizeof opt.model);
    std::memcpy(opt.ets_model, options->ets_model, sizeof opt.ets_model);
    opt.horizon = options->horizon; opt.confidence_level = options->confidence_level; opt.seasonal_period = options->seasonal_period;
    opt.auto_detect_seasonality = options->auto_detect_seasonality; opt.include_fitted = options->include_fitted;
    opt.include_residuals = options->include_residuals; opt.window = options->window;
    std::memcpy(opt.seasonal_periods_str, options->seasonal_periods_str, sizeof opt.seasonal_periods_str);
    std::memcpy(opt.model_pool, options->model_pool, sizeof opt.model_pool);
    std::memcpy(opt.laplace_variant, options->laplace_variant, sizeof opt.laplace_variant);
    opt.laplace_seasonal_batch_init = options->laplace_seasonal_batch_init;
    const ExogRoute route = K == 0 ? EXOG_IGNORED : exog_route(mt);
    if (route == EXOG_IGNORED) return anofox_ts_forecast(values, validity, length, &opt, out_result, out_error);
    if (route == EXOG_NOT_IMPLEMENTED) { set_error(out_error, INTERNAL_ERROR, exog_not_implemented_message(mt)); return false; }
    if (K > (size_t)EXOG_MAX_REGRESSORS) { set_error(out_error, COMPUTATION_ERROR, exog_cap_message(K)); return false; }
    std::vector<const double *> xr(K), fx(K);
    for (size_t i = 0; i < K; i++) { xr[i] = options->exog->regressors[i].values; fx[i] = options->exog->regressors[i].future_values; }
    // (a horizon of 0 has no future values to point at: the batch entry does not read them)
    const double *vals[1] = {values};
    const uint64_t *valid[1] = {validity};
    const size_t lens[1] = {length};
    ForecastResult r;
    AnofoxError se, be;
    clear_error(&se); clear_error(&be);
    if (!anofox_ts_forecast_exog_batch(vals, validity ? valid : nullptr, lens, 1, &opt, K, xr.data(), fx.data(), &r, &se, &be, nullptr, nullptr)) {
        if (out_error) *out_error = be.code != SUCCESS ? be : se;
        return false;
    }
    if (se.code != SUCCESS) { anofox_free_forecast_result(&r); if (out_error) *out_error = se; return false; }
    *out_result = r;
    return true;
}

} // extern "C"

// ------------------------------------------------------------------------------------------------------------------------------
// Walk-forward backtest on a resident block (_ts_backtest_native: ts_backtest_native.cpp:623-711, 768-880, 280-373; backtest.hip)
// ------------------------------------------------------------------------------------------------------------------------------
namespace {

constexpr int64_t BT_POS_MAX = (int64_t)INT32_MAX - 1;       // a position at or above it lies behind every block (t_rows <= 2^30)

// the host fold table -> the kernels' int32 table; *t_train = the longest training window (at least 1)
bool backtest_fold_table(const AnofoxHipFold *folds, size_t n_folds, std::vector<BacktestFoldPos> *out, size_t *t_train, AnofoxError *err)
{
    if (n_folds > 0 && !folds) { set_error(err, NULL_POINTER, "Null pointer argument"); return false; }
    if (n_folds > (size_t)INT32_MAX) { set_error(err, INVALID_INPUT, "Invalid input: too many folds"); return false; }
    size_t longest = 1;
    if (out) out->resize(n_folds);
    for (size_t f = 0; f < n_folds; f++) {
        const AnofoxHipFold &q = folds[f];
        if (q.train_start < 0 || q.train_end < 0 || q.test_start < 0 || q.test_end < 0) {
            set_error(err, INVALID_INPUT, "Invalid input: a fold position is negative");
            return false;
        }
        if (q.train_start <= q.train_end) {
            const int64_t w = q.train_end - q.train_start + 1;
            if (w > (int64_t)(1u << 30)) { set_error(err, INVALID_INPUT, "Invalid input: a training window is too long"); return false; }
            longest = std::max(longest, (size_t)w);
        }
        if (out)
            (*out)[f] = BacktestFoldPos{(int32_t)std::min(q.train_start, BT_POS_MAX), (int32_t)std::min(q.train_end, BT_POS_MAX),
                                        (int32_t)std::min(q.test_start, BT_POS_MAX), (int32_t)std::min(q.test_end, BT_POS_MAX)};
    }
    if (t_train) *t_train = longest;
    return true;
}

} // namespace

extern "C" {

static_assert(sizeof(AnofoxHipFold) == 40 && offsetof(AnofoxHipFold, test_end) == 32, "AnofoxHipFold layout");

size_t anofox_hip_backtest_folds(int64_t n_dates, int64_t horizon, int64_t folds, int window_type, int64_t min_train_size, int64_t gap,
                                 int64_t embargo, int64_t initial_train_size, int64_t skip_length, bool clip_horizon, AnofoxHipFold *out_folds,
                                 size_t capacity)
{
    return backtest_folds(n_dates, horizon, folds, window_type, min_train_size, gap, embargo, initial_train_size, skip_length, clip_horizon,
                          out_folds, capacity);
}

bool anofox_hip_backtest_sizes(const AnofoxHipFold *folds, size_t n_folds, size_t n_series, size_t *t_train, size_t *n_pairs, size_t *ld_pairs,
                               AnofoxError *out_error)
{
    clear_error(out_error);
    size_t longest = 1;
    if (!backtest_fold_table(folds, n_folds, nullptr, &longest, out_error)) return false;
    if (n_series > (size_t)INT32_MAX || (n_folds > 0 && n_series > (size_t)INT32_MAX / n_folds)) {
        set_error(out_error, INVALID_INPUT, "Invalid input: more than 2^31 - 1 (series, fold) pairs");
        return false;
    }
    const size_t np = n_series * n_folds;
    if (t_train) *t_train = longest;
    if (n_pairs) *n_pairs = np;
    if (ld_pairs) *ld_pairs = std::max<size_t>((np + 63) / 64 * 64, 64);
    return true;
}

bool anofox_hip_backtest_expand_device(const double *y, size_t ld_src, const int32_t *lengths, size_t n_series, size_t t_rows,
                                       const AnofoxHipFold *folds, size_t n_folds, size_t t_train, double *y_out, size_t ld_pairs,
                                       int32_t *len_pairs, int32_t *n_test, void *stream, AnofoxError *out_error)
{
    clear_error(out_error);
    if (!y_out || !len_pairs || !n_test || (n_series > 0 && (!y || !lengths))) { set_error(out_error, NULL_POINTER, "Null pointer argument"); return false; }
    if (ld_src < n_series) { set_error(out_error, INVALID_INPUT, "Invalid input: ld_src is smaller than n_series"); return false; }
    if (t_rows > (size_t)(1u << 30)) { set_error(out_error, INVALID_INPUT, "Invalid input: the block is too large"); return false; }
    std::vector<BacktestFoldPos> tab;
    size_t need_t = 1, np = 0, need_ld = 64;
    if (!backtest_fold_table(folds, n_folds, &tab, nullptr, out_error)) return false;
    if (!anofox_hip_backtest_sizes(folds, n_folds, n_series, &need_t, &np, &need_ld, out_error)) return false;
    if (ld_pairs != need_ld || t_train < need_t) {
        set_error(out_error, INVALID_INPUT, "Invalid input: t_train or ld_pairs is not what anofox_hip_backtest_sizes returns");
        return false;
    }
    if (!device_ready(out_error)) return false;
    hipStream_t st = (hipStream_t)stream;
    Scratch scratch;
    const bool ok = launch_and_wait("backtest expand", st, out_error, [&] {
        BacktestFoldPos *d_tab = scratch.get<BacktestFoldPos>(n_folds);
        if (n_folds) HIPCHECK(hipMemcpyAsync(d_tab, tab.data(), n_folds * sizeof(BacktestFoldPos), hipMemcpyHostToDevice, st));
        BacktestArgs a{};
        a.y = y; a.ld_src = ld_src; a.len = lengths; a.n_series = (int)n_series; a.t_rows = t_rows;
        a.folds = d_tab; a.n_folds = (int)std::max<size_t>(n_folds, 1); a.n_pairs = (int)np; a.ld_pairs = ld_pairs;
        a.t_train = t_train; a.y_out = y_out; a.len_pairs = len_pairs; a.n_test = n_test;
        launch_backtest_expand(a, st);
    });
    if (ok) scratch.settled();
    return ok;
}

bool anofox_hip_backtest_collect_device(const double *y, size_t ld_src, size_t n_series, size_t t_rows, const AnofoxHipFold *folds,
                                        size_t n_folds, const int32_t *n_test, const int32_t *status, const double *yhat, const double *lower,
                                        const double *upper, size_t horizon, const char *metric, double *actual, double *error,
                                        double *abs_error, uint8_t *valid, int32_t *n_rows, double *scores, void *stream, AnofoxError *out_error)
{
    clear_error(out_error);
    std::vector<BacktestFoldPos> tab;
    size_t np = 0;
    if (!backtest_fold_table(folds, n_folds, &tab, nullptr, out_error)) return false;
    if (!anofox_hip_backtest_sizes(folds, n_folds, n_series, nullptr, &np, nullptr, out_error)) return false;
    if (np > 0 && (!y || !n_test || !status || !yhat || !actual || !error || !abs_error || !n_rows)) {
        set_error(out_error, NULL_POINTER, "Null pointer argument");
        return false;
    }
    if (ld_src < n_series) { set_error(out_error, INVALID_INPUT, "Invalid input: ld_src is smaller than n_series"); return false; }
    if (t_rows > (size_t)(1u << 30)) { set_error(out_error, INVALID_INPUT, "Invalid input: the block is too large"); return false; }
    if (horizon < 1 || horizon > (size_t)(1u << 30) || (double)np * (double)horizon >= 256.0 * 2147483647.0) {
        set_error(out_error, INVALID_INPUT, "Invalid input: horizon must be at least 1 (and n_pairs x horizon below 2^39)");
        return false;
    }
    if (n_folds == 0) return true;
    if (!device_ready(out_error)) return false;
    hipStream_t st = (hipStream_t)stream;
    Scratch scratch;
    const bool ok = launch_and_wait("backtest collect", st, out_error, [&] {
        BacktestFoldPos *d_tab = scratch.get<BacktestFoldPos>(n_folds);
        HIPCHECK(hipMemcpyAsync(d_tab, tab.data(), n_folds * sizeof(BacktestFoldPos), hipMemcpyHostToDevice, st));
        BacktestArgs a{};
        a.y = y; a.ld_src = ld_src; a.n_series = (int)n_series; a.t_rows = t_rows;
        a.folds = d_tab; a.n_folds = (int)n_folds; a.n_pairs = (int)np;
        a.h = (int)horizon; a.n_test = (int32_t *)n_test; a.status = status; a.yhat = yhat; a.lower = lower; a.upper = upper;
        a.actual = actual; a.error = error; a.abs_error = abs_error; a.valid = valid; a.n_rows = n_rows;
        a.metric = backtest_metric_code(metric); a.scores = scores;
        launch_backtest_collect(a, st);
    });
    if (ok) scratch.settled();
    return ok;
}

bool anofox_hip_backtest_batch(const double *const *values, const size_t *lengths, size_t n_series, const ForecastOptions *options,
                               const AnofoxHipFold *folds, size_t n_folds, const char *metric, int32_t *out_n_rows, int32_t *out_status,
                               char (*out_model_names)[64], double *out_yhat, double *out_lower, double *out_upper, double *out_actual,
                               double *out_scores, AnofoxError *out_batch_error)
{
    clear_error(out_batch_error);
    if (!options || (n_series > 0 && (!values || !lengths))) { set_error(out_batch_error, NULL_POINTER, "Null pointer argument"); return false; }
    size_t t_train = 1, np = 0, ld_pairs = 64;
    if (!anofox_hip_backtest_sizes(folds, n_folds, n_series, &t_train, &np, &ld_pairs, out_batch_error)) return false;
    BlockShape shape;
    if (!series_shape(values, nullptr, lengths, n_series, (size_t)1 << 30, &shape, out_batch_error)) return false;
    if (options->horizon < 1) { set_error(out_batch_error, INVALID_INPUT, "Invalid input: horizon must be at least 1"); return false; }
    if (np == 0) return true;
    const size_t h = (size_t)options->horizon, nh = np * h, ld_src = shape.ld, T = shape.T;
    AnofoxHipBatch *b = nullptr;
    if (!anofox_hip_batch_create(np, t_train, options, &b, out_batch_error)) return false;      // e.g. "ETS:AAA": INVALID_MODEL, no rows
    bool ok = true;
    // ONE arena of results, so that one copy brings them back: yhat, lower, upper, actual, the scores, then error and abs_error
    // (fp64), then n_rows, status, model_code [np] and, not copied, len_pairs and n_test [ld_pairs] (int32)
    const size_t n_fp_back = 4 * nh + n_folds;
    std::vector<double> back(n_fp_back + (3 * np + 1) / 2);      // the doubles that go back, then the three int32 arrays
    try {
        DeviceGuard guard(b->dev);
        hipStream_t st = b->own_stream;
        Scratch scratch;
        double *d_src = scratch.get<double>(T * ld_src), *d_exp = nullptr;
        int32_t *d_len = scratch.get<int32_t>(ld_src);
        {
            std::vector<double> yb(T * ld_src, 0.0);
            const std::vector<int32_t> len = block_lengths(lengths, n_series, ld_src);
            pack_time_major(yb.data(), ld_src, values, lengths, n_series);
            HIPCHECK(hipMemcpy(d_src, yb.data(), T * ld_src * sizeof(double), hipMemcpyHostToDevice));
            HIPCHECK(hipMemcpy(d_len, len.data(), ld_src * sizeof(int32_t), hipMemcpyHostToDevice));
        }
        try { d_exp = scratch.get<double>(t_train * ld_pairs); }
        catch (const HipFail &f) {
            if (!f.oom) throw;
            set_error(out_batch_error, COMPUTATION_ERROR, "Computation error: the expanded backtest block of " + std::to_string(t_train) + " x " +
                      std::to_string(ld_pairs) + " values needs " + std::to_string(t_train * ld_pairs * sizeof(double)) + " bytes of device memory");
            ok = false;
        }
        if (ok) {
            double *d_fp = scratch.get<double>(n_fp_back + (3 * np + 1) / 2);
            int32_t *d_int = scratch.get<int32_t>(2 * ld_pairs);
            double *d_work = scratch.get<double>(2 * nh);
            int32_t *d_rows = (int32_t *)(d_fp + n_fp_back), *d_stat = d_rows + np, *d_code = d_rows + 2 * np, *d_lenp = d_int, *d_ntest = d_int + ld_pairs;
            double *d_yh = d_fp, *d_lo = d_fp + nh, *d_hi = d_fp + 2 * nh, *d_act = d_fp + 3 * nh, *d_sc = d_fp + 4 * nh, *d_err = d_work,
                   *d_abs = d_work + nh;
            ok = anofox_hip_backtest_expand_device(d_src, ld_src, d_len, n_series, T, folds, n_folds, t_train, d_exp, ld_pairs, d_lenp, d_ntest, st,
                                                   out_batch_error) &&
                 anofox_hip_batch_set_device_block(b, d_exp, ld_pairs, d_lenp, out_batch_error) && anofox_hip_batch_run(b, nullptr, out_batch_error);
            if (ok) {
                HIPCHECK(hipStreamSynchronize(b->last_stream));
                b->quiesced = true;
                ok = anofox_hip_backtest_collect_device(d_src, ld_src, n_series, T, folds, n_folds, d_ntest, b->d_status, b->d_yhat, b->d_lo, b->d_hi, h,
                                                        metric, d_act, d_err, d_abs, nullptr, d_rows, d_sc, st, out_batch_error);
            }
            if (ok) {
                HIPCHECK(hipMemcpyAsync(d_yh, b->d_yhat, nh * sizeof(double), hipMemcpyDeviceToDevice, st));
                HIPCHECK(hipMemcpyAsync(d_lo, b->d_lo, nh * sizeof(double), hipMemcpyDeviceToDevice, st));
                HIPCHECK(hipMemcpyAsync(d_hi, b->d_hi, nh * sizeof(double), hipMemcpyDeviceToDevice, st));
                HIPCHECK(hipMemcpyAsync(d_stat, b->d_status, np * sizeof(int32_t), hipMemcpyDeviceToDevice, st));
                HIPCHECK(hipMemcpyAsync(d_code, b->d_model_code, np * sizeof(int32_t), hipMemcpyDeviceToDevice, st));
                HIPCHECK(hipStreamSynchronize(st));
                HIPCHECK(hipMemcpy(back.data(), d_fp, back.size() * sizeof(double), hipMemcpyDeviceToHost));
            }
        }
        if (ok) scratch.settled();
    } catch (const HipFail &f) {
        report_hip_failure(out_batch_error, f);
        anofox_hip_batch_destroy(b);
        return false;
    }
    if (ok) {
        const double *fp = back.data();
        const int32_t *rows = (const int32_t *)(fp + n_fp_back), *stat = rows + np, *code = rows + 2 * np;
        for (size_t p = 0; p < np; p++) {
            const int32_t st_p = stat[p] == STATUS_NOT_COMPUTED ? (int32_t)INTERNAL_ERROR : stat[p];
            if (out_n_rows) out_n_rows[p] = rows[p];
            if (out_status) out_status[p] = st_p;
            if (out_model_names) {
                out_model_names[p][0] = 0;
                if (st_p == 0) anofox_hip_batch_model_name(b, p, code[p], out_model_names[p]);
            }
        }
        if (out_yhat) std::memcpy(out_yhat, fp, nh * sizeof(double));
        if (out_lower) std::memcpy(out_lower, fp + nh, nh * sizeof(double));
        if (out_upper) std::memcpy(out_upper, fp + 2 * nh, nh * sizeof(double));
        if (out_actual) std::memcpy(out_actual, fp + 3 * nh, nh * sizeof(double));
        if (out_scores) std::memcpy(out_scores, fp + 4 * nh, n_folds * sizeof(double));
    } else if (out_batch_error && out_batch_error->code == SUCCESS) {
        set_error(out_batch_error, INTERNAL_ERROR, "Internal error: device batch failed");
    }
    anofox_hip_batch_destroy(b);
    return ok;
}

} // extern "C"

// ------------------------------------------------------------------------------------------------------------------------------
// Aggregation up a key hierarchy on a resident block (ts_aggregate_hierarchy.cpp:246-386; hierarchy.hip)
// ------------------------------------------------------------------------------------------------------------------------------
namespace {

bool hierarchy_options_ok(const AnofoxHipHierarchyOptions *o, size_t struct_size, AnofoxError *err)
{
    if (!o) { set_error(err, NULL_POINTER, "Null pointer argument"); return false; }
    if (struct_size != sizeof(AnofoxHipHierarchyOptions)) {
        set_error(err, INVALID_INPUT, "Invalid input: struct_size is not sizeof(AnofoxHipHierarchyOptions)");
        return false;
    }
    if (o->route < HIER_ROUTE_AUTO || o->route > HIER_ROUTE_TILE || o->tile_min_members < 0) {
        set_error(err, INVALID_INPUT, "Invalid input: route must be 0 (automatic), 1 (lane per column) or 2 (tile), tile_min_members >= 0");
        return false;
    }
    return true;
}

// first and last set bit of a DuckDB mask among rows [0, n); false when there is none.  A NULL mask is all ones.
bool hierarchy_mask_range(const uint64_t *m, size_t n, size_t *t0, size_t *t1)
{
    if (n == 0) return false;
    if (!m) { *t0 = 0; *t1 = n - 1; return true; }
    size_t a = 0, b = n;
    while (a < n && !valid_bit(m, a)) a++;
    if (a == n) return false;
    while (!valid_bit(m, b - 1)) b--;
    *t0 = a; *t1 = b - 1;
    return true;
}

} // namespace

extern "C" {

static_assert(sizeof(AnofoxHipHierarchyOptions) == 16 && offsetof(AnofoxHipHierarchyOptions, tile_min_members) == 4, "AnofoxHipHierarchyOptions layout");

bool anofox_hip_hierarchy_plan(const int32_t *column_of, size_t n_groupings, size_t n_series, size_t *n_out, size_t *nnz, int32_t *col_offsets,
                               int32_t *members, AnofoxError *out_error)
{
    clear_error(out_error);
    if (n_series > (size_t)INT32_MAX) { set_error(out_error, INVALID_INPUT, "Invalid input: more than 2^31 - 1 series"); return false; }
    const bool cells = n_groupings > 0 && n_series > 0;
    if (cells && !column_of) { set_error(out_error, NULL_POINTER, "Null pointer argument"); return false; }
    if ((col_offsets == nullptr) != (members == nullptr)) { set_error(out_error, NULL_POINTER, "Null pointer argument"); return false; }
    int64_t largest = -1;
    size_t count = 0;
    if (cells)
        for (size_t g = 0; g < n_groupings; g++)
            for (size_t s = 0; s < n_series; s++) {
                const int32_t c = column_of[g * n_series + s];
                if (c < -1) { set_error(out_error, INVALID_INPUT, "Invalid input: a column_of entry is below -1"); return false; }
                if (c >= 0) { count++; largest = std::max<int64_t>(largest, c); }
            }
    if (largest + 1 > (int64_t)INT32_MAX) {
        set_error(out_error, INVALID_INPUT, "Invalid input: n_out exceeds the limit of 2^31 - 1 output columns");
        return false;
    }
    if (count > (size_t)INT32_MAX) {
        set_error(out_error, INVALID_INPUT, "Invalid input: nnz exceeds the limit of 2^31 - 1 plan entries");
        return false;
    }
    const size_t no = (size_t)(largest + 1);
    if (n_out) *n_out = no;
    if (nnz) *nnz = count;
    if (!col_offsets) return true;
    // stable counting sort by column: entries are visited by (series, grouping), so that is their order within a column
    std::vector<int32_t> at(no + 1, 0);
    if (cells)
        for (size_t i = 0; i < n_groupings * n_series; i++)
            if (column_of[i] >= 0) at[(size_t)column_of[i] + 1]++;
    for (size_t c = 0; c < no; c++) at[c + 1] += at[c];
    std::memcpy(col_offsets, at.data(), (no + 1) * sizeof(int32_t));
    if (cells)
        for (size_t s = 0; s < n_series; s++)
            for (size_t g = 0; g < n_groupings; g++) {
                const int32_t c = column_of[g * n_series + s];
                if (c >= 0) members[at[(size_t)c]++] = (int32_t)s;
            }
    return true;
}

bool anofox_hip_hierarchy_device(const double *y, const uint8_t *valid, const uint8_t *present, size_t ld, const int32_t *lengths,
                                 const int64_t *first, size_t n_series, size_t t_rows, const int32_t *col_offsets, const int32_t *members,
                                 size_t n_out, size_t nnz, const AnofoxHipHierarchyOptions *options, size_t struct_size, size_t t_out,
                                 double *y_out, uint8_t *present_out, size_t ld_out, int32_t *lengths_out, int64_t *first_out, void *stream,
                                 AnofoxError *out_error)
{
    clear_error(out_error);
    if (!hierarchy_options_ok(options, struct_size, out_error)) return false;
    if ((n_out > 0 && (!col_offsets || !lengths_out || !first_out)) || (nnz > 0 && (!members || !y || !lengths))) {
        set_error(out_error, NULL_POINTER, "Null pointer argument");
        return false;
    }
    if (n_out > (size_t)INT32_MAX || nnz > (size_t)INT32_MAX || n_series > (size_t)INT32_MAX) {
        set_error(out_error, INVALID_INPUT, "Invalid input: n_out, nnz and n_series are limited to 2^31 - 1");
        return false;
    }
    if (ld < n_series) { set_error(out_error, INVALID_INPUT, "Invalid input: ld is smaller than n_series"); return false; }
    if (t_rows > (size_t)HIER_SPAN_MAX || t_out > (size_t)HIER_SPAN_MAX) {
        set_error(out_error, INVALID_INPUT, "Invalid input: t_rows and t_out are limited to 2^30 rows");
        return false;
    }
    const bool full = y_out != nullptr && t_out > 0;
    if (full && ld_out < n_out) { set_error(out_error, INVALID_INPUT, "Invalid input: ld_out is smaller than n_out"); return false; }
    if (n_out == 0) return true;
    if (!device_ready(out_error)) return false;
    HierarchyArgs a{};
    a.y = y; a.ld = ld; a.valid = valid; a.present = present; a.len = lengths; a.first = first; a.n_series = (int)n_series; a.t_rows = t_rows;
    a.col_offsets = col_offsets; a.members = members; a.n_out = (int)n_out; a.nnz = (int)nnz;
    a.route = options->route; a.tile_min = options->tile_min_members > 0 ? options->tile_min_members : HIER_TILE_MIN_MEMBERS;
    a.t_out = full ? t_out : 0; a.ld_out = ld_out; a.y_out = full ? y_out : nullptr; a.present_out = full ? present_out : nullptr;
    a.len_out = lengths_out; a.first_out = first_out;
    try {
        (void)hipGetLastError();
        launch_hierarchy(a, (hipStream_t)stream);
        LAUNCHCHECK("hierarchy");
    } catch (const HipFail &f) {
        report_hip_failure(out_error, f);
        return false;
    }
    return true;
}

bool anofox_hip_hierarchy_batch(const double *const *values, const uint64_t *const *validity, const uint64_t *const *present,
                                const size_t *lengths, const int64_t *first, size_t n_series, const int32_t *column_of, size_t n_groupings,
                                const AnofoxHipHierarchyOptions *options, size_t struct_size, size_t t_out, size_t ld_out, double *out_y,
                                uint8_t *out_present, int32_t *out_lengths, int64_t *out_first, size_t *out_n_out, size_t *out_t_out,
                                size_t *out_ld, AnofoxError *out_error)
{
    clear_error(out_error);
    if (!hierarchy_options_ok(options, struct_size, out_error)) return false;
    if (n_series > 0 && (!values || !lengths)) { set_error(out_error, NULL_POINTER, "Null pointer argument"); return false; }
    size_t n_out = 0, nnz = 0, T = 1;
    if (!anofox_hip_hierarchy_plan(column_of, n_groupings, n_series, &n_out, &nnz, nullptr, nullptr, out_error)) return false;
    std::vector<int32_t> offs(n_out + 1), memb(std::max<size_t>(nnz, 1));
    if (!anofox_hip_hierarchy_plan(column_of, n_groupings, n_series, &n_out, &nnz, offs.data(), memb.data(), out_error)) return false;
    // the span of every series, then of every column: the sizes come from the host's copy, the device only confirms them
    std::vector<int64_t> s_lo(n_series, 0), s_hi(n_series, -1);
    bool any_valid = false, any_present = false;
    for (size_t s = 0; s < n_series; s++) {
        const size_t n = lengths[s];
        if (n > 0 && !values[s]) { set_error(out_error, NULL_POINTER, "Null pointer argument"); return false; }
        if (n > (size_t)HIER_SPAN_MAX) { set_error(out_error, INVALID_INPUT, "Invalid input: a series is longer than the limit of 2^30 rows"); return false; }
        const int64_t f = first ? first[s] : 0;
        if (f > HIER_FIRST_MAX || f < -HIER_FIRST_MAX) {
            set_error(out_error, INVALID_INPUT, "Invalid input: a first position is outside the limit of +-2^61");
            return false;
        }
        T = std::max(T, n);
        any_valid = any_valid || (validity && validity[s] && n > 0);
        any_present = any_present || (present && present[s] && n > 0);
        size_t t0 = 0, t1 = 0;
        if (hierarchy_mask_range(present ? present[s] : nullptr, n, &t0, &t1)) { s_lo[s] = f + (int64_t)t0; s_hi[s] = f + (int64_t)t1; }
        else { s_lo[s] = 0; s_hi[s] = -1; }
    }
    std::vector<int32_t> c_len(n_out, 0);
    std::vector<int64_t> c_first(n_out, 0);
    size_t longest = 1;
    for (size_t c = 0; c < n_out; c++) {
        int64_t lo = INT64_MAX, hi = INT64_MIN;
        for (int32_t i = offs[c]; i < offs[c + 1]; i++) {
            const size_t s = (size_t)memb[(size_t)i];
            if (s_lo[s] > s_hi[s]) continue;
            lo = std::min(lo, s_lo[s]); hi = std::max(hi, s_hi[s]);
        }
        if (lo > hi) continue;
        if (hi - lo + 1 > HIER_SPAN_MAX) {
            set_error(out_error, INVALID_INPUT, "Invalid input: output column " + std::to_string(c) + " spans " + std::to_string(hi - lo + 1) +
                      " rows, above the limit of 2^30");
            return false;
        }
        c_len[c] = (int32_t)(hi - lo + 1); c_first[c] = lo;
        longest = std::max(longest, (size_t)c_len[c]);
    }
    const size_t need_ld = std::max<size_t>((n_out + 63) / 64 * 64, 64);
    if (out_n_out) *out_n_out = n_out;
    if (out_t_out) *out_t_out = longest;
    if (out_ld) *out_ld = need_ld;
    if (!out_y) return true;
    if (t_out != longest || ld_out != need_ld) {
        set_error(out_error, INVALID_INPUT, "Invalid input: t_out or ld_out is not what the sizing call returns");
        return false;
    }
    if (!out_lengths || !out_first) { set_error(out_error, NULL_POINTER, "Null pointer argument"); return false; }
    if (n_out == 0) return true;
    if (!device_ready(out_error)) return false;
    const size_t ld = (std::max<size_t>(n_series, 1) + 63) / 64 * 64;
    // ONE arena of results, so that one copy brings them back: y, first (8-byte items), lengths, then the present bytes
    const size_t cells = t_out * ld_out, back_bytes = cells * 8 + ld_out * 8 + ld_out * 4 + cells;
    double *d_y = nullptr;
    uint8_t *d_valid = nullptr, *d_present = nullptr, *d_back = nullptr;
    Scratch scratch;
    std::vector<uint8_t> back(back_bytes);
    bool ok = true;
    try {
        std::vector<double> yb(T * ld, 0.0);
        std::vector<uint8_t> vb(any_valid ? T * ld : 0, 1), pb(any_present ? T * ld : 0, 1);
        const std::vector<int32_t> len = block_lengths(lengths, n_series, ld);
        std::vector<int64_t> fst(ld, 0);
        for (size_t s = 0; s < n_series; s++) fst[s] = first ? first[s] : 0;
        pack_time_major(yb.data(), ld, values, lengths, n_series);
        if (any_valid) pack_validity(vb.data(), ld, validity, lengths, n_series);
        if (any_present) pack_validity(pb.data(), ld, present, lengths, n_series);
        try {
            d_y = scratch.get<double>(T * ld);
            if (any_valid) d_valid = scratch.get<uint8_t>(T * ld);
            if (any_present) d_present = scratch.get<uint8_t>(T * ld);
            d_back = scratch.get<uint8_t>(back_bytes);
        } catch (const HipFail &f) {
            if (!f.oom) throw;
            set_error(out_error, COMPUTATION_ERROR, "Computation error: the source block of " + std::to_string(T) + " x " + std::to_string(ld) +
                      " values and the aggregated block of " + std::to_string(t_out) + " x " + std::to_string(ld_out) + " values need " +
                      std::to_string(T * ld * (8 + (any_valid ? 1 : 0) + (any_present ? 1 : 0)) + back_bytes) + " bytes of device memory");
            ok = false;
        }
        if (ok) {
            int32_t *d_len = scratch.get<int32_t>(ld);
            int64_t *d_first = scratch.get<int64_t>(ld);
            int32_t *d_plan = scratch.get<int32_t>(n_out + 1 + nnz);
            HIPCHECK(hipMemcpy(d_y, yb.data(), T * ld * sizeof(double), hipMemcpyHostToDevice));
            if (any_valid) HIPCHECK(hipMemcpy(d_valid, vb.data(), T * ld, hipMemcpyHostToDevice));
            if (any_present) HIPCHECK(hipMemcpy(d_present, pb.data(), T * ld, hipMemcpyHostToDevice));
            HIPCHECK(hipMemcpy(d_len, len.data(), ld * sizeof(int32_t), hipMemcpyHostToDevice));
            HIPCHECK(hipMemcpy(d_first, fst.data(), ld * sizeof(int64_t), hipMemcpyHostToDevice));
            HIPCHECK(hipMemcpy(d_plan, offs.data(), (n_out + 1) * sizeof(int32_t), hipMemcpyHostToDevice));
            if (nnz) HIPCHECK(hipMemcpy(d_plan + n_out + 1, memb.data(), nnz * sizeof(int32_t), hipMemcpyHostToDevice));
            double *d_yo = (double *)d_back;
            int64_t *d_fo = (int64_t *)(d_back + cells * 8);
            int32_t *d_lo = (int32_t *)(d_back + cells * 8 + ld_out * 8);
            uint8_t *d_po = d_back + cells * 8 + ld_out * 8 + ld_out * 4;
            HIPCHECK(hipMemset(d_back, 0, back_bytes));                    // the padding columns of the arena
            ok = anofox_hip_hierarchy_device(d_y, d_valid, d_present, ld, d_len, d_first, n_series, T, d_plan, d_plan + n_out + 1, n_out, nnz,
                                             options, struct_size, t_out, d_yo, d_po, ld_out, d_lo, d_fo, nullptr, out_error);
            if (ok) HIPCHECK(hipMemcpy(back.data(), d_back, back_bytes, hipMemcpyDeviceToHost));      // waits for the null stream
            else HIPCHECK(hipDeviceSynchronize());
        }
        scratch.settled();                                                 // (either way the device has been waited for)
    } catch (const HipFail &f) {
        report_hip_failure(out_error, f);
        return false;
    }
    if (!ok) return false;
    const int64_t *fo = (const int64_t *)(back.data() + cells * 8);
    const int32_t *lo = (const int32_t *)(back.data() + cells * 8 + ld_out * 8);
    for (size_t c = 0; c < n_out; c++)
        if (lo[c] != c_len[c] || fo[c] != c_first[c]) {
            set_error(out_error, INTERNAL_ERROR, "Internal error: the device sized output column " + std::to_string(c) + " differently from the host");
            return false;
        }
    std::memcpy(out_y, back.data(), cells * 8);
    std::memcpy(out_first, fo, n_out * sizeof(int64_t));
    std::memcpy(out_lengths, lo, n_out * sizeof(int32_t));
    if (out_present) std::memcpy(out_present, back.data() + cells * 8 + ld_out * 8 + ld_out * 4, cells);
    return true;
}

} // extern "C"

// ------------------------------------------------------------------------------------------------------------------------------
// Reconciliation of the forecasts of a hierarchy (DESIGN.md section 3 "Reconciliation"; reconcile.hip)
// ------------------------------------------------------------------------------------------------------------------------------
namespace {

// what the two device entries share: the sizes, then the plan pointers where there is something to read through them
bool reconcile_plan_args(const int32_t *col_offsets, const int32_t *members, size_t n_out, size_t nnz, size_t n_series, const int32_t *bottom_col,
                         const int32_t *agg_cols, size_t n_agg, const int32_t *leaf_offsets, const int32_t *leaf_aggs, size_t n_leaf,
                         const double *weights, ReconcilePlan *p, AnofoxError *err)
{
    if (n_out > (size_t)INT32_MAX || nnz > (size_t)INT32_MAX || n_series > (size_t)INT32_MAX || n_leaf > (size_t)INT32_MAX) {
        set_error(err, INVALID_INPUT, "Invalid input: n_out, nnz, n_series and n_leaf are limited to 2^31 - 1");
        return false;
    }
    if (n_agg > (size_t)ANOFOX_HIP_RECONCILE_MAX_AGG) {
        set_error(err, INVALID_INPUT, "Invalid input: n_agg " + std::to_string(n_agg) + " exceeds the limit of " +
                  std::to_string(ANOFOX_HIP_RECONCILE_MAX_AGG) + " aggregate columns");
        return false;
    }
    if ((n_out > 0 && !col_offsets) || (nnz > 0 && !members) || (n_series > 0 && (!bottom_col || !leaf_offsets)) || (n_agg > 0 && !agg_cols) ||
        (n_leaf > 0 && !leaf_aggs)) {
        set_error(err, NULL_POINTER, "Null pointer argument");
        return false;
    }
    p->col_offsets = col_offsets; p->members = members; p->n_out = (int)n_out; p->nnz = (int)nnz; p->n_series = (int)n_series;
    p->bottom_col = bottom_col; p->agg_cols = agg_cols; p->n_agg = (int)n_agg;
    p->leaf_offsets = leaf_offsets; p->leaf_aggs = leaf_aggs; p->n_leaf = (int)n_leaf; p->weights = weights;
    return true;
}

bool reconcile_method_ok(int32_t method, bool allow_bottom_up, AnofoxError *err)
{
    if (method < (allow_bottom_up ? RECONCILE_BOTTOM_UP : RECONCILE_OLS) || method > RECONCILE_WLS_VAR) {
        set_error(err, INVALID_INPUT, allow_bottom_up ? "Invalid input: method must be 0 (bottom_up), 1 (ols), 2 (wls_struct) or 3 (wls_var)"
                                                      : "Invalid input: a factor exists for method 1 (ols), 2 (wls_struct) or 3 (wls_var) only");
        return false;
    }
    return true;
}

} // namespace

extern "C" {

static_assert(ANOFOX_RECONCILE_BOTTOM_UP == RECONCILE_BOTTOM_UP && ANOFOX_RECONCILE_WLS_VAR == RECONCILE_WLS_VAR, "reconciliation method codes");

bool anofox_hip_reconcile_plan(const int32_t *col_offsets, const int32_t *members, size_t n_out, size_t n_series, size_t *n_agg, size_t *n_leaf,
                               int32_t *bottom_col, int32_t *agg_cols, int32_t *leaf_offsets, int32_t *leaf_aggs, double *struct_weights,
                               AnofoxError *out_error)
{
    clear_error(out_error);
    std::string message;
    const ReconcilePlanResult r = reconcile_plan_host(col_offsets, members, n_out, n_series, (size_t)ANOFOX_HIP_RECONCILE_MAX_AGG, n_agg, n_leaf,
                                                      bottom_col, agg_cols, leaf_offsets, leaf_aggs, struct_weights, &message);
    if (r == RECONCILE_PLAN_NULL) set_error(out_error, NULL_POINTER, "Null pointer argument");
    else if (r == RECONCILE_PLAN_INVALID) set_error(out_error, INVALID_INPUT, message);
    return r == RECONCILE_PLAN_OK;
}

bool anofox_hip_reconcile_factor_device(const int32_t *col_offsets, const int32_t *members, size_t n_out, size_t nnz, size_t n_series,
                                        const int32_t *bottom_col, const int32_t *agg_cols, size_t n_agg, const int32_t *leaf_offsets,
                                        const int32_t *leaf_aggs, size_t n_leaf, int32_t method, const double *weights, double *factor,
                                        size_t ld_a, void *stream, AnofoxError *out_error)
{
    clear_error(out_error);
    if (!reconcile_method_ok(method, false, out_error)) return false;
    ReconcileFactorArgs a{};
    if (!reconcile_plan_args(col_offsets, members, n_out, nnz, n_series, bottom_col, agg_cols, n_agg, leaf_offsets, leaf_aggs, n_leaf,
                             method == RECONCILE_OLS ? nullptr : weights, &a.p, out_error))
        return false;
    if (method != RECONCILE_OLS && n_out > 0 && !weights) { set_error(out_error, NULL_POINTER, "Null pointer argument"); return false; }
    if (n_agg > 0 && !factor) { set_error(out_error, NULL_POINTER, "Null pointer argument"); return false; }
    if (ld_a < n_agg) { set_error(out_error, INVALID_INPUT, "Invalid input: ld_a is smaller than n_agg"); return false; }
    if (!device_ready(out_error)) return false;
    a.L = factor; a.ld_a = ld_a;
    a.trailing = RECONCILE_TRAILING_MFMA;                          // the faster tile on the 12,350-row system (profiles/reconcile_m5.txt)
    {                                                              // developer knob of tools/time_reconcile.py: 0 plain FMA tile, 1 MFMA
        const std::map<std::string, std::string> kv = Tunables::tune_map();
        auto it = kv.find("reconcile_trailing");
        if (it != kv.end()) a.trailing = std::atoi(it->second.c_str()) == 0 ? RECONCILE_TRAILING_FMA : RECONCILE_TRAILING_MFMA;
    }
    hipStream_t st = (hipStream_t)stream;
    Scratch scratch;
    int32_t info[2] = {RECONCILE_NONE, RECONCILE_NONE};
    const bool ok = launch_and_wait("reconcile factor", st, out_error, [&] {
        a.info = scratch.get<int32_t>(2);
        launch_reconcile_factor(a, st);
        HIPCHECK(hipMemcpyAsync(info, a.info, sizeof(info), hipMemcpyDeviceToHost, st));
    });
    if (!ok) return false;
    scratch.settled();
    if (info[0] != RECONCILE_NONE) {
        set_error(out_error, INVALID_INPUT, "Invalid input: the weight of column " + std::to_string(info[0]) + " is not finite and positive");
        return false;
    }
    if (info[1] != RECONCILE_NONE) {
        set_error(out_error, COMPUTATION_ERROR, "Computation error: the pivot of row " + std::to_string(info[1]) + " of the reconciliation system is not positive");
        return false;
    }
    return true;
}

bool anofox_hip_reconcile_apply_device(const double *base, size_t stride_s, size_t stride_t, size_t n_rows, const int32_t *col_offsets,
                                       const int32_t *members, size_t n_out, size_t nnz, size_t n_series, const int32_t *bottom_col,
                                       const int32_t *agg_cols, size_t n_agg, const int32_t *leaf_offsets, const int32_t *leaf_aggs, size_t n_leaf,
                                       int32_t method, const double *weights, const double *factor, size_t ld_a, double *work, double *out,
                                       int32_t *row_status, void *stream, AnofoxError *out_error)
{
    clear_error(out_error);
    if (!reconcile_method_ok(method, true, out_error)) return false;
    ReconcileApplyArgs a{};
    const bool solve = method != RECONCILE_BOTTOM_UP && n_agg > 0;
    if (!reconcile_plan_args(col_offsets, members, n_out, nnz, n_series, bottom_col, agg_cols, n_agg, leaf_offsets, leaf_aggs, n_leaf,
                             (method == RECONCILE_OLS || method == RECONCILE_BOTTOM_UP) ? nullptr : weights, &a.p, out_error))
        return false;
    if (n_rows > (size_t)INT32_MAX) { set_error(out_error, INVALID_INPUT, "Invalid input: n_rows is limited to 2^31 - 1"); return false; }
    if (n_rows > 0 && (!row_status || (n_out > 0 && (!base || !out)))) { set_error(out_error, NULL_POINTER, "Null pointer argument"); return false; }
    if (solve && !factor) { set_error(out_error, INVALID_INPUT, "Invalid input: methods 1 to 3 need the factor of anofox_hip_reconcile_factor_device"); return false; }
    if (solve && n_rows > 0 && !work) { set_error(out_error, NULL_POINTER, "Null pointer argument"); return false; }
    if (solve && method != RECONCILE_OLS && !weights) { set_error(out_error, NULL_POINTER, "Null pointer argument"); return false; }
    if (solve && ld_a < n_agg) { set_error(out_error, INVALID_INPUT, "Invalid input: ld_a is smaller than n_agg"); return false; }
    if (n_rows == 0) return true;
    if (!device_ready(out_error)) return false;
    a.method = method; a.base = base; a.out = out; a.stride_s = stride_s; a.stride_t = stride_t; a.n_rows = n_rows;
    a.L = factor; a.ld_a = ld_a; a.work = work; a.ld_work = n_agg; a.row_status = row_status;
    try {
        (void)hipGetLastError();
        launch_reconcile_apply(a, (hipStream_t)stream);
        LAUNCHCHECK("reconcile apply");
    } catch (const HipFail &f) {
        report_hip_failure(out_error, f);
        return false;
    }
    return true;
}

bool anofox_hip_reconcile_batch(const int32_t *column_of, size_t n_groupings, size_t n_series, const double *forecast, size_t h, int32_t method,
                                const double *weights, double *out, int32_t *out_row_status, AnofoxError *out_error)
{
    clear_error(out_error);
    if (!reconcile_method_ok(method, true, out_error)) return false;
    size_t n_out = 0, nnz = 0, n_agg = 0, n_leaf = 0;
    if (!anofox_hip_hierarchy_plan(column_of, n_groupings, n_series, &n_out, &nnz, nullptr, nullptr, out_error)) return false;
    std::vector<int32_t> offs(n_out + 1), memb(std::max<size_t>(nnz, 1));
    if (!anofox_hip_hierarchy_plan(column_of, n_groupings, n_series, &n_out, &nnz, offs.data(), memb.data(), out_error)) return false;
    if (!anofox_hip_reconcile_plan(offs.data(), memb.data(), n_out, n_series, &n_agg, &n_leaf, nullptr, nullptr, nullptr, nullptr, nullptr, out_error))
        return false;
    std::vector<int32_t> bottom(std::max<size_t>(n_series, 1)), aggs(std::max<size_t>(n_agg, 1)), loffs(n_series + 1), laggs(std::max<size_t>(n_leaf, 1));
    std::vector<double> w(std::max<size_t>(n_out, 1), 1.0);
    if (!anofox_hip_reconcile_plan(offs.data(), memb.data(), n_out, n_series, &n_agg, &n_leaf, bottom.data(), aggs.data(), loffs.data(), laggs.data(),
                                   w.data(), out_error))
        return false;
    if (n_out > 0 && h > 0 && (!forecast || !out || !out_row_status)) { set_error(out_error, NULL_POINTER, "Null pointer argument"); return false; }
    if (method == RECONCILE_WLS_VAR) {
        if (n_out > 0 && !weights) { set_error(out_error, NULL_POINTER, "Null pointer argument"); return false; }
        for (size_t c = 0; c < n_out; c++) w[c] = weights[c];
    }
    if (n_out == 0 || h == 0) return true;
    if (!device_ready(out_error)) return false;
    const bool solve = method != RECONCILE_BOTTOM_UP && n_agg > 0;
    // ONE arena of int32 plan arrays: offsets, members, bottom_col, agg_cols, leaf_offsets, leaf_aggs
    const size_t n_int = (n_out + 1) + nnz + n_series + n_agg + (n_series + 1) + n_leaf, cells = n_out * h;
    const size_t bytes = n_int * 4 + (2 * cells + n_out + (solve ? n_agg * n_agg + h * n_agg : 0)) * 8 + h * 4;
    Scratch scratch;
    bool ok = true;
    try {
        int32_t *d_int = nullptr, *d_status = nullptr;
        double *d_base = nullptr, *d_out = nullptr, *d_w = nullptr, *d_L = nullptr, *d_work = nullptr;
        try {
            d_int = scratch.get<int32_t>(n_int);
            d_base = scratch.get<double>(cells);
            d_out = scratch.get<double>(cells);
            d_w = scratch.get<double>(n_out);
            d_status = scratch.get<int32_t>(h);
            if (solve) { d_L = scratch.get<double>(n_agg * n_agg); d_work = scratch.get<double>(h * n_agg); }
        } catch (const HipFail &f) {
            if (!f.oom) throw;
            set_error(out_error, COMPUTATION_ERROR, "Computation error: the plan, two blocks of " + std::to_string(n_out) + " x " + std::to_string(h) +
                      " values and the factor of " + std::to_string(n_agg) + " x " + std::to_string(n_agg) + " values need " + std::to_string(bytes) +
                      " bytes of device memory");
            ok = false;
        }
        if (ok) {
            std::vector<int32_t> plan;
            plan.reserve(n_int);
            plan.insert(plan.end(), offs.begin(), offs.end());
            plan.insert(plan.end(), memb.begin(), memb.begin() + nnz);
            plan.insert(plan.end(), bottom.begin(), bottom.begin() + n_series);
            plan.insert(plan.end(), aggs.begin(), aggs.begin() + n_agg);
            plan.insert(plan.end(), loffs.begin(), loffs.end());
            plan.insert(plan.end(), laggs.begin(), laggs.begin() + n_leaf);
            const int32_t *d_offs = d_int, *d_memb = d_offs + n_out + 1, *d_bottom = d_memb + nnz, *d_aggs = d_bottom + n_series,
                          *d_loffs = d_aggs + n_agg, *d_laggs = d_loffs + n_series + 1;
            HIPCHECK(hipMemcpy(d_int, plan.data(), n_int * sizeof(int32_t), hipMemcpyHostToDevice));
            HIPCHECK(hipMemcpy(d_base, forecast, cells * sizeof(double), hipMemcpyHostToDevice));
            HIPCHECK(hipMemcpy(d_w, w.data(), n_out * sizeof(double), hipMemcpyHostToDevice));
            if (solve)
                ok = anofox_hip_reconcile_factor_device(d_offs, d_memb, n_out, nnz, n_series, d_bottom, d_aggs, n_agg, d_loffs, d_laggs, n_leaf, method,
                                                        d_w, d_L, n_agg, nullptr, out_error);
            if (ok)
                ok = anofox_hip_reconcile_apply_device(d_base, h, 1, h, d_offs, d_memb, n_out, nnz, n_series, d_bottom, d_aggs, n_agg, d_loffs, d_laggs,
                                                       n_leaf, method, d_w, d_L, n_agg, d_work, d_out, d_status, nullptr, out_error);
            if (ok) {
                HIPCHECK(hipMemcpy(out, d_out, cells * sizeof(double), hipMemcpyDeviceToHost));          // waits for the null stream
                HIPCHECK(hipMemcpy(out_row_status, d_status, h * sizeof(int32_t), hipMemcpyDeviceToHost));
            } else {
                HIPCHECK(hipDeviceSynchronize());
            }
        }
        scratch.settled();
    } catch (const HipFail &f) {
        report_hip_failure(out_error, f);
        return false;
    }
    return ok;
}

} // extern "C"

// ------------------------------------------------------------------------------------------------------------------------------
// MinT with the shrinkage covariance (DESIGN.md section 3 "MinT-shrink"; reconcile_mint.hip)
// ------------------------------------------------------------------------------------------------------------------------------
namespace {

static_assert(RECONCILE_MINT_MAX_RESIDUAL_ROWS == (size_t)ANOFOX_HIP_RECONCILE_MAX_RESIDUAL_ROWS, "the limit of residual rows");
static_assert(RECONCILE_MINT_TILE == (size_t)64, "the Gram tile of reconcile_mint.hip");

bool reconcile_mint_report(ReconcileMintResult r, const std::string &message, AnofoxError *err)
{
    if (r == RECONCILE_MINT_NULL) set_error(err, NULL_POINTER, "Null pointer argument");
    else if (r == RECONCILE_MINT_INVALID) set_error(err, INVALID_INPUT, message);
    return r == RECONCILE_MINT_OK;
}

// developer knob `name` of ANOFOX_HIP_TUNE: 0 plain FMA tile, anything else (and the default) MFMA
int reconcile_tile_variant(const char *name)
{
    const std::map<std::string, std::string> kv = Tunables::tune_map();
    auto it = kv.find(name);
    return (it != kv.end() && std::atoi(it->second.c_str()) == 0) ? RECONCILE_TRAILING_FMA : RECONCILE_TRAILING_MFMA;
}

} // namespace

extern "C" {

bool anofox_hip_reconcile_mint_sizes(size_t n_res, size_t n_agg, size_t n_rows, size_t *gram_elems, size_t *e_elems, size_t *factor_elems,
                                     size_t *work_elems, AnofoxError *out_error)
{
    clear_error(out_error);
    std::string message;
    return reconcile_mint_report(reconcile_mint_sizes_host(n_res, n_agg, n_rows, (size_t)ANOFOX_HIP_RECONCILE_MAX_AGG, gram_elems, e_elems,
                                                           factor_elems, work_elems, &message), message, out_error);
}

bool anofox_hip_reconcile_mint_factor_device(const double *residuals, size_t res_stride_s, size_t res_stride_t, size_t n_res,
                                             const int32_t *col_offsets, const int32_t *members, size_t n_out, size_t nnz, size_t n_series,
                                             const int32_t *bottom_col, const int32_t *agg_cols, size_t n_agg, const int32_t *leaf_offsets,
                                             const int32_t *leaf_aggs, size_t n_leaf, double shrinkage, double *variances, double *e, size_t ld_e,
                                             double *factor, size_t ld_a, double *gram_work, double *out_shrinkage, void *stream,
                                             AnofoxError *out_error)
{
    clear_error(out_error);
    std::string message;
    bool estimate = false;
    if (!reconcile_mint_report(reconcile_mint_rows_check(n_res, &message), message, out_error)) return false;
    if (!reconcile_mint_report(reconcile_mint_lambda_check(shrinkage, true, &estimate, &message), message, out_error)) return false;
    ReconcileMintArgs a{};
    if (!reconcile_plan_args(col_offsets, members, n_out, nnz, n_series, bottom_col, agg_cols, n_agg, leaf_offsets, leaf_aggs, n_leaf, nullptr, &a.p,
                             out_error))
        return false;
    if (!reconcile_mint_report(reconcile_mint_dims_check(n_series, n_agg, (size_t)ANOFOX_HIP_RECONCILE_MAX_AGG, ld_e, ld_a, &message), message, out_error))
        return false;
    if (!out_shrinkage || (n_out > 0 && (!residuals || !variances)) || (n_agg > 0 && (!factor || !e)) || (estimate && n_out > 0 && !gram_work)) {
        set_error(out_error, NULL_POINTER, "Null pointer argument");
        return false;
    }
    if (!device_ready(out_error)) return false;
    a.res = residuals; a.res_stride_s = res_stride_s; a.res_stride_t = res_stride_t; a.n_res = (int)n_res;
    a.var = variances; a.E = e; a.ld_e = ld_e; a.L = factor; a.ld_a = ld_a;
    a.gram = estimate ? gram_work : nullptr; a.gram_splits = (int)reconcile_mint_gram_splits(n_res); a.lambda_in = shrinkage;
    a.trailing = reconcile_tile_variant("reconcile_trailing");
    a.ete = reconcile_tile_variant("reconcile_mint_ete");
    hipStream_t st = (hipStream_t)stream;
    Scratch scratch;
    int32_t info[4] = {RECONCILE_NONE, RECONCILE_NONE, RECONCILE_NONE, RECONCILE_NONE};
    double lam = shrinkage;
    const bool ok = launch_and_wait("reconcile mint factor", st, out_error, [&] {
        a.info = scratch.get<int32_t>(4);
        double *d = scratch.get<double>(2 * std::max<size_t>(n_out, 1) + 1);
        a.rsd = d; a.f4col = d + std::max<size_t>(n_out, 1); a.lambda = d + 2 * std::max<size_t>(n_out, 1);
        launch_reconcile_mint_factor(a, st);
        HIPCHECK(hipMemcpyAsync(info, a.info, sizeof(info), hipMemcpyDeviceToHost, st));
        if (n_out > 0) HIPCHECK(hipMemcpyAsync(&lam, a.lambda, sizeof(double), hipMemcpyDeviceToHost, st));
    });
    if (!ok) return false;
    scratch.settled();
    if (info[MINT_INFO_RESIDUAL] != RECONCILE_NONE) {
        set_error(out_error, COMPUTATION_ERROR, "Computation error: a residual of column " + std::to_string(info[MINT_INFO_RESIDUAL]) + " is not finite");
        return false;
    }
    if (info[MINT_INFO_VARIANCE] != RECONCILE_NONE) {
        set_error(out_error, COMPUTATION_ERROR, "Computation error: the residual variance of column " + std::to_string(info[MINT_INFO_VARIANCE]) +
                  " is not finite and positive");
        return false;
    }
    if (info[MINT_INFO_PIVOT] != RECONCILE_NONE) {
        set_error(out_error, COMPUTATION_ERROR, "Computation error: the pivot of row " + std::to_string(info[MINT_INFO_PIVOT]) +
                  " of the reconciliation system is not positive");
        return false;
    }
    if (estimate && n_out == 0) lam = 1.0;                          // (no column at all: nothing to estimate from)
    *out_shrinkage = lam;
    return true;
}

bool anofox_hip_reconcile_mint_apply_device(const double *base, size_t stride_s, size_t stride_t, size_t n_rows, const double *residuals,
                                            size_t res_stride_s, size_t res_stride_t, size_t n_res, const int32_t *col_offsets,
                                            const int32_t *members, size_t n_out, size_t nnz, size_t n_series, const int32_t *bottom_col,
                                            const int32_t *agg_cols, size_t n_agg, const int32_t *leaf_offsets, const int32_t *leaf_aggs,
                                            size_t n_leaf, const double *variances, const double *e, size_t ld_e, double shrinkage,
                                            const double *factor, size_t ld_a, double *work, double *out, int32_t *row_status, void *stream,
                                            AnofoxError *out_error)
{
    clear_error(out_error);
    std::string message;
    if (!reconcile_mint_report(reconcile_mint_rows_check(n_res, &message), message, out_error)) return false;
    if (!reconcile_mint_report(reconcile_mint_lambda_check(shrinkage, false, nullptr, &message), message, out_error)) return false;
    ReconcileMintApplyArgs m{};
    if (!reconcile_plan_args(col_offsets, members, n_out, nnz, n_series, bottom_col, agg_cols, n_agg, leaf_offsets, leaf_aggs, n_leaf, nullptr, &m.a.p,
                             out_error))
        return false;
    if (!reconcile_mint_report(reconcile_mint_dims_check(n_series, n_agg, (size_t)ANOFOX_HIP_RECONCILE_MAX_AGG, ld_e, ld_a, &message), message, out_error))
        return false;
    if (n_rows > (size_t)INT32_MAX) { set_error(out_error, INVALID_INPUT, "Invalid input: n_rows is limited to 2^31 - 1"); return false; }
    if (n_rows > 0 && (!row_status || (n_out > 0 && (!base || !out)))) { set_error(out_error, NULL_POINTER, "Null pointer argument"); return false; }
    if (n_agg > 0 && !factor) {
        set_error(out_error, INVALID_INPUT, "Invalid input: the apply needs the factor of anofox_hip_reconcile_mint_factor_device");
        return false;
    }
    if (n_agg > 0 && n_rows > 0 && (!work || !residuals || !variances || !e)) { set_error(out_error, NULL_POINTER, "Null pointer argument"); return false; }
    if (n_rows == 0) return true;
    if (!device_ready(out_error)) return false;
    ReconcileApplyArgs &a = m.a;
    a.method = RECONCILE_WLS_VAR; a.base = base; a.out = out; a.stride_s = stride_s; a.stride_t = stride_t; a.n_rows = n_rows;
    a.L = factor; a.ld_a = ld_a; a.work = work; a.ld_work = n_agg; a.row_status = row_status;
    m.res = residuals; m.res_stride_s = res_stride_s; m.res_stride_t = res_stride_t; m.n_res = (int)n_res;
    m.var = variances; m.E = e; m.ld_e = ld_e; m.lambda = shrinkage; m.g = work ? work + n_rows * n_agg : nullptr;
    try {
        (void)hipGetLastError();
        launch_reconcile_mint_apply(m, (hipStream_t)stream);
        LAUNCHCHECK("reconcile mint apply");
    } catch (const HipFail &f) {
        report_hip_failure(out_error, f);
        return false;
    }
    return true;
}

bool anofox_hip_reconcile_mint_batch(const int32_t *column_of, size_t n_groupings, size_t n_series, const double *forecast, size_t h,
                                     const double *residuals, size_t n_res, double *shrinkage, double *out, int32_t *out_row_status,
                                     double *out_variances, AnofoxError *out_error)
{
    clear_error(out_error);
    std::string message;
    bool estimate = false;
    if (!shrinkage) { set_error(out_error, NULL_POINTER, "Null pointer argument"); return false; }
    if (!reconcile_mint_report(reconcile_mint_rows_check(n_res, &message), message, out_error)) return false;
    if (!reconcile_mint_report(reconcile_mint_lambda_check(*shrinkage, true, &estimate, &message), message, out_error)) return false;
    size_t n_out = 0, nnz = 0, n_agg = 0, n_leaf = 0;
    if (!anofox_hip_hierarchy_plan(column_of, n_groupings, n_series, &n_out, &nnz, nullptr, nullptr, out_error)) return false;
    std::vector<int32_t> offs(n_out + 1), memb(std::max<size_t>(nnz, 1));
    if (!anofox_hip_hierarchy_plan(column_of, n_groupings, n_series, &n_out, &nnz, offs.data(), memb.data(), out_error)) return false;
    if (!anofox_hip_reconcile_plan(offs.data(), memb.data(), n_out, n_series, &n_agg, &n_leaf, nullptr, nullptr, nullptr, nullptr, nullptr, out_error))
        return false;
    std::vector<int32_t> bottom(std::max<size_t>(n_series, 1)), aggs(std::max<size_t>(n_agg, 1)), loffs(n_series + 1), laggs(std::max<size_t>(n_leaf, 1));
    if (!anofox_hip_reconcile_plan(offs.data(), memb.data(), n_out, n_series, &n_agg, &n_leaf, bottom.data(), aggs.data(), loffs.data(), laggs.data(),
                                   nullptr, out_error))
        return false;
    if (n_out > 0 && (!residuals || (h > 0 && (!forecast || !out || !out_row_status)))) { set_error(out_error, NULL_POINTER, "Null pointer argument"); return false; }
    if (n_out == 0) return true;
    if (!device_ready(out_error)) return false;
    size_t gram_elems = 0, e_elems = 0, factor_elems = 0, work_elems = 0;
    if (!anofox_hip_reconcile_mint_sizes(n_res, n_agg, h, &gram_elems, &e_elems, &factor_elems, &work_elems, out_error)) return false;
    if (!estimate) gram_elems = 0;
    const size_t n_int = (n_out + 1) + nnz + n_series + n_agg + (n_series + 1) + n_leaf, cells = n_out * h, rcells = n_out * n_res;
    const size_t n_dbl = 2 * cells + rcells + n_out + gram_elems + e_elems + factor_elems + work_elems;
    Scratch scratch;
    bool ok = true;
    try {
        int32_t *d_int = nullptr, *d_status = nullptr;
        double *d_all = nullptr;
        try {
            d_int = scratch.get<int32_t>(n_int);
            d_status = scratch.get<int32_t>(std::max<size_t>(h, 1));
            d_all = scratch.get<double>(std::max<size_t>(n_dbl, 1));
        } catch (const HipFail &f) {
            if (!f.oom) throw;
            set_error(out_error, COMPUTATION_ERROR, "Computation error: the plan, two blocks of " + std::to_string(n_out) + " x " + std::to_string(h) +
                      " values, the residual block of " + std::to_string(n_out) + " x " + std::to_string(n_res) + " values, the factor of " +
                      std::to_string(n_agg) + " x " + std::to_string(n_agg) + " values and the workspaces need " +
                      std::to_string(n_int * 4 + h * 4 + n_dbl * 8) + " bytes of device memory");
            ok = false;
        }
        if (ok) {
            std::vector<int32_t> plan;
            plan.reserve(n_int);
            plan.insert(plan.end(), offs.begin(), offs.end());
            plan.insert(plan.end(), memb.begin(), memb.begin() + nnz);
            plan.insert(plan.end(), bottom.begin(), bottom.begin() + n_series);
            plan.insert(plan.end(), aggs.begin(), aggs.begin() + n_agg);
            plan.insert(plan.end(), loffs.begin(), loffs.end());
            plan.insert(plan.end(), laggs.begin(), laggs.begin() + n_leaf);
            const int32_t *d_offs = d_int, *d_memb = d_offs + n_out + 1, *d_bottom = d_memb + nnz, *d_aggs = d_bottom + n_series,
                          *d_loffs = d_aggs + n_agg, *d_laggs = d_loffs + n_series + 1;
            double *d_base = d_all, *d_out = d_base + cells, *d_res = d_out + cells, *d_var = d_res + rcells, *d_gram = d_var + n_out,
                   *d_e = d_gram + gram_elems, *d_L = d_e + e_elems, *d_work = d_L + factor_elems;
            HIPCHECK(hipMemcpy(d_int, plan.data(), n_int * sizeof(int32_t), hipMemcpyHostToDevice));
            if (cells) HIPCHECK(hipMemcpy(d_base, forecast, cells * sizeof(double), hipMemcpyHostToDevice));
            HIPCHECK(hipMemcpy(d_res, residuals, rcells * sizeof(double), hipMemcpyHostToDevice));
            double lam = *shrinkage;
            ok = anofox_hip_reconcile_mint_factor_device(d_res, n_res, 1, n_res, d_offs, d_memb, n_out, nnz, n_series, d_bottom, d_aggs, n_agg, d_loffs,
                                                         d_laggs, n_leaf, lam, d_var, d_e, n_agg, d_L, n_agg, estimate ? d_gram : nullptr, &lam, nullptr,
                                                         out_error);
            if (ok && h > 0)
                ok = anofox_hip_reconcile_mint_apply_device(d_base, h, 1, h, d_res, n_res, 1, n_res, d_offs, d_memb, n_out, nnz, n_series, d_bottom, d_aggs,
                                                            n_agg, d_loffs, d_laggs, n_leaf, d_var, d_e, n_agg, lam, d_L, n_agg, d_work, d_out, d_status,
                                                            nullptr, out_error);
            if (ok) {
                if (cells) HIPCHECK(hipMemcpy(out, d_out, cells * sizeof(double), hipMemcpyDeviceToHost));     // waits for the null stream
                if (h) HIPCHECK(hipMemcpy(out_row_status, d_status, h * sizeof(int32_t), hipMemcpyDeviceToHost));
                if (out_variances) HIPCHECK(hipMemcpy(out_variances, d_var, n_out * sizeof(double), hipMemcpyDeviceToHost));
                *shrinkage = lam;
            } else {
                HIPCHECK(hipDeviceSynchronize());
            }
        }
        scratch.settled();
    } catch (const HipFail &f) {
        report_hip_failure(out_error, f);
        return false;
    }
    return ok;
}

} // extern "C"

// ------------------------------------------------------------------------------------------------------------------------------
// The choice of a method per series from backtest scores (DESIGN.md section 3 "Selection"; select.hip)
// ------------------------------------------------------------------------------------------------------------------------------
namespace {

static_assert(SELECT_PLAN_MAX_METHODS == (size_t)SELECT_MAX_METHODS && ANOFOX_HIP_SELECT_MAX_METHODS == SELECT_MAX_METHODS, "the limit of methods");
static_assert(ANOFOX_SELECT_PICK == SELECT_PICK && ANOFOX_SELECT_INVERSE_SCORE == SELECT_INVERSE_SCORE, "selection mode codes");

constexpr double SELECT_MAX_CELLS = 256.0 * 2147483647.0;         // cells of a [rows x horizon] block: the grid of one launch

bool select_plan_report(SelectPlanResult r, const std::string &message, AnofoxError *err)
{
    if (r == SELECT_PLAN_NULL) set_error(err, NULL_POINTER, "Null pointer argument");
    else if (r == SELECT_PLAN_INVALID) set_error(err, INVALID_INPUT, message);
    return r == SELECT_PLAN_OK;
}

// a batch that lives as long as this object
struct BatchOwner {
    AnofoxHipBatch *b = nullptr;
    BatchOwner() = default;
    BatchOwner(const BatchOwner &) = delete;
    BatchOwner &operator=(const BatchOwner &) = delete;
    ~BatchOwner() { if (b) anofox_hip_batch_destroy(b); }
};

// one batch of n columns on a resident block: create, adopt the block, run, wait
bool select_run_batch(const ForecastOptions *o, size_t n, size_t t_rows, const double *d_y, size_t ld, const int32_t *d_len, BatchOwner *own,
                      AnofoxError *err)
{
    if (!anofox_hip_batch_create(n, t_rows, o, &own->b, err)) return false;
    if (!anofox_hip_batch_set_device_block(own->b, d_y, ld, d_len, err) || !anofox_hip_batch_run(own->b, nullptr, err)) return false;
    HIPCHECK(hipStreamSynchronize(own->b->last_stream));
    own->b->quiesced = true;
    return true;
}

} // namespace

extern "C" {

bool anofox_hip_select_winner_device(const double *scores, size_t ld, const int32_t *score_status, size_t n_methods, size_t n_series,
                                     int32_t fallback, int32_t *winner, double *best_score, uint8_t *from_fallback, int32_t *offsets,
                                     int32_t *members, void *stream, AnofoxError *out_error)
{
    clear_error(out_error);
    std::string message;
    if (!select_plan_report(select_counts_check(n_methods, fallback, &message), message, out_error)) return false;
    if (!offsets || (n_series > 0 && (!scores || !score_status || !winner || !best_score || !from_fallback || !members))) {
        set_error(out_error, NULL_POINTER, "Null pointer argument");
        return false;
    }
    if (!block_args_ok(ld, n_series, "n_series", 0, 0, out_error)) return false;
    if (!device_ready(out_error)) return false;
    hipStream_t st = (hipStream_t)stream;
    Scratch scratch;
    const bool ok = launch_and_wait("select winner", st, out_error, [&] {
        if (n_series == 0) {
            HIPCHECK(hipMemsetAsync(offsets, 0, (n_methods + 1) * sizeof(int32_t), st));
            return;
        }
        SelectWinnerArgs a{};
        a.scores = scores; a.ld = ld; a.score_status = score_status;
        a.n_methods = (int)n_methods; a.n_series = (int)n_series; a.fallback = fallback;
        a.winner = winner; a.best_score = best_score; a.from_fallback = from_fallback;
        a.n_wg = select_workgroups(n_series);
        a.counts = scratch.get<int32_t>(select_counts_size(n_series, (int)n_methods));
        a.offsets = offsets; a.members = members;
        launch_select_winner(a, st);
    });
    if (ok) scratch.settled();
    return ok;
}

bool anofox_hip_select_gather_device(const double *y, size_t ld_src, const int32_t *lengths, size_t n_series, size_t t_rows,
                                     const int32_t *members, size_t off, size_t n_m, double *y_out, size_t ld_m, int32_t *len_out, void *stream,
                                     AnofoxError *out_error)
{
    clear_error(out_error);
    if ((ld_m > 0 && (!len_out || (t_rows > 0 && !y_out))) || (n_m > 0 && (!y || !lengths || !members))) {
        set_error(out_error, NULL_POINTER, "Null pointer argument");
        return false;
    }
    if (!block_args_ok(ld_src, n_series, "n_series", t_rows, (size_t)1 << 30, out_error)) return false;
    if (ld_m < n_m) { set_error(out_error, INVALID_INPUT, "Invalid input: ld_m is smaller than n_m"); return false; }
    if (off > n_series || n_m > n_series - off) {
        set_error(out_error, INVALID_INPUT, "Invalid input: members[off .. off + n_m) lies outside the n_series entries of the partition");
        return false;
    }
    if (ld_m > (size_t)INT32_MAX) { set_error(out_error, INVALID_INPUT, "Invalid input: the block is too large"); return false; }
    if (ld_m == 0) return true;
    if (!device_ready(out_error)) return false;
    SelectMoveArgs a{};
    a.members = members; a.off = off; a.n_m = n_m; a.n_series = (int)n_series;
    a.y = y; a.ld_src = ld_src; a.len = lengths; a.t_rows = t_rows; a.y_out = y_out; a.ld_m = ld_m; a.len_out = len_out;
    hipStream_t st = (hipStream_t)stream;
    return launch_and_wait("select gather", st, out_error, [&] { launch_select_gather(a, st); });
}

bool anofox_hip_select_scatter_device(const double *yhat_m, const double *lower_m, const double *upper_m, const int32_t *code_m,
                                      const int32_t *status_m, const int32_t *members, size_t off, size_t n_m, size_t horizon,
                                      const int32_t *winner, size_t n_series, double *yhat, double *lower, double *upper, int32_t *model_code,
                                      int32_t *status, void *stream, AnofoxError *out_error)
{
    clear_error(out_error);
    if (n_m > 0 && (!members || (yhat && !yhat_m) || (lower && !lower_m) || (upper && !upper_m) || (model_code && !code_m) || (status && !status_m))) {
        set_error(out_error, NULL_POINTER, "Null pointer argument");
        return false;
    }
    if (n_series > (size_t)INT32_MAX) { set_error(out_error, INVALID_INPUT, "Invalid input: n_series is limited to 2^31 - 1"); return false; }
    if (horizon < 1 || horizon > (size_t)(1u << 30) || (double)n_series * (double)horizon >= SELECT_MAX_CELLS) {
        set_error(out_error, INVALID_INPUT, "Invalid input: horizon must be at least 1 (and n_series x horizon below 2^39)");
        return false;
    }
    if (off > n_series || n_m > n_series - off) {
        set_error(out_error, INVALID_INPUT, "Invalid input: members[off .. off + n_m) lies outside the n_series entries of the partition");
        return false;
    }
    if (n_series == 0 || (n_m == 0 && !winner)) return true;
    if (!device_ready(out_error)) return false;
    SelectMoveArgs a{};
    a.members = members; a.off = off; a.n_m = n_m; a.n_series = (int)n_series; a.h = (int)horizon;
    a.yhat_m = yhat_m; a.lower_m = lower_m; a.upper_m = upper_m; a.code_m = code_m; a.status_m = status_m; a.winner = winner;
    a.yhat = yhat; a.lower = lower; a.upper = upper; a.model_code = model_code; a.status = status;
    hipStream_t st = (hipStream_t)stream;
    return launch_and_wait("select scatter", st, out_error, [&] { launch_select_scatter(a, st); });
}

bool anofox_hip_select_combine_device(const double *const *blocks, size_t n_methods, size_t n_rows, size_t horizon, const int32_t *member_status,
                                      int32_t mode, const int32_t *winner, const double *weights, size_t ld_w, size_t group_div, double *out,
                                      int32_t *row_status, void *stream, AnofoxError *out_error)
{
    clear_error(out_error);
    std::string message;
    if (!select_plan_report(select_counts_check(n_methods, -1, &message), message, out_error)) return false;
    if (mode < SELECT_PICK || mode > SELECT_INVERSE_SCORE) {
        set_error(out_error, INVALID_INPUT, "Invalid input: mode must be 0 (pick), 1 (mean), 2 (median) or 3 (inverse_score)");
        return false;
    }
    if (!blocks) { set_error(out_error, NULL_POINTER, "Null pointer argument"); return false; }
    if (horizon < 1 || horizon > (size_t)(1u << 30) || n_rows > (size_t)INT32_MAX || (double)n_rows * (double)horizon >= SELECT_MAX_CELLS) {
        set_error(out_error, INVALID_INPUT, "Invalid input: horizon must be at least 1 (and n_rows x horizon below 2^39)");
        return false;
    }
    if (group_div < 1) { set_error(out_error, INVALID_INPUT, "Invalid input: group_div must be at least 1"); return false; }
    if (n_rows > 0) {
        bool null = !out || (mode != SELECT_PICK && !member_status) || (mode == SELECT_PICK && !winner) || (mode == SELECT_INVERSE_SCORE && !weights);
        for (size_t m = 0; m < n_methods; m++) null = null || !blocks[m];
        if (null) { set_error(out_error, NULL_POINTER, "Null pointer argument"); return false; }
        if (mode == SELECT_INVERSE_SCORE && ld_w < (n_rows + group_div - 1) / group_div) {
            set_error(out_error, INVALID_INPUT, "Invalid input: ld_w is smaller than the number of groups");
            return false;
        }
    }
    if (n_rows == 0) return true;
    if (!device_ready(out_error)) return false;
    hipStream_t st = (hipStream_t)stream;
    Scratch scratch;
    const bool ok = launch_and_wait("select combine", st, out_error, [&] {
        const double **d_tab = scratch.get<const double *>(n_methods);
        HIPCHECK(hipMemcpyAsync(d_tab, blocks, n_methods * sizeof(const double *), hipMemcpyHostToDevice, st));
        SelectCombineArgs a{};
        a.blocks = d_tab; a.n_methods = (int)n_methods; a.h = (int)horizon; a.mode = mode;
        a.n_rows = n_rows; a.group_div = group_div; a.member_status = member_status; a.winner = winner;
        a.weights = weights; a.ld_w = ld_w; a.out = out; a.row_status = row_status;
        launch_select_combine(a, st);
    });
    if (ok) scratch.settled();
    return ok;
}

bool anofox_hip_select_batch(const double *const *values, const size_t *lengths, size_t n_series, const ForecastOptions *methods, size_t n_methods,
                             const AnofoxHipFold *folds, size_t n_folds, const char *criterion, const char *mode, int32_t fallback,
                             int32_t *out_winner, double *out_best_score, double *out_scores, double *out_yhat, double *out_lower,
                             double *out_upper, int32_t *out_status, char (*out_model_names)[64], double *out_backtest_yhat,
                             double *out_backtest_actual, int32_t *out_n_rows, AnofoxError *out_batch_error)
{
    AnofoxError *const err = out_batch_error;
    clear_error(err);
    std::string message;
    if (!select_plan_report(select_counts_check(n_methods, fallback, &message), message, err)) return false;
    if (!methods || !criterion || !mode || (n_series > 0 && (!values || !lengths))) { set_error(err, NULL_POINTER, "Null pointer argument"); return false; }
    int figure = -1, mode_code = -1;
    {
        int horizons[SELECT_PLAN_MAX_METHODS];
        for (size_t m = 0; m < n_methods; m++) horizons[m] = methods[m].horizon;
        if (!select_plan_report(select_request_check(n_methods, horizons, criterion, mode, fallback, &figure, &mode_code, &message), message, err))
            return false;
    }
    size_t t_train = 1, np = 0, ld_pairs = 64;
    if (!anofox_hip_backtest_sizes(folds, n_folds, n_series, &t_train, &np, &ld_pairs, err)) return false;
    BlockShape shape;
    if (!series_shape(values, nullptr, lengths, n_series, (size_t)1 << 30, &shape, err)) return false;
    for (size_t m = 0; m < n_methods; m++) {                     // an option block anofox_hip_batch_create refuses fails the whole call
        Plan plan;
        if (!make_plan(&methods[m], plan, err)) return false;
    }
    const size_t M = n_methods, N = n_series, F = n_folds, h = (size_t)methods[0].horizon, nh = np * h, Nh = N * h;
    if ((double)np * (double)h >= SELECT_MAX_CELLS || F * h > (size_t)INT32_MAX) {
        set_error(err, INVALID_INPUT, "Invalid input: n_pairs x horizon must stay below 2^39");
        return false;
    }
    if (N == 0) return true;
    if (!device_ready(err)) return false;
    const size_t ld_src = shape.ld, T = shape.T, ldN = ld_src;
    const bool pick = mode_code == SELECT_PICK;
    // what goes back, in two arenas: fp64 -- yhat, lower, upper [N x h], the selected backtest yhat and actual [np x h], best_score [N],
    // scores [M x ldN] -- and int32 -- winner, status, model_code, members [N], offsets [M + 1]
    const size_t n_fp = 3 * Nh + 2 * nh + N + M * ldN, n_int = 4 * N + M + 1;
    std::vector<double> fp(n_fp);
    std::vector<int32_t> in(n_int);
    std::vector<std::string> names(out_model_names ? N : 0);
    bool ok = true;
    try {
        int dev = 0;
        HIPCHECK(hipGetDevice(&dev));
        DeviceGuard guard(dev);
        hipStream_t st = nullptr;
        Scratch scratch;                                         // (declared before every batch: a batch adopts blocks of it)
        double *d_src = scratch.get<double>(T * ld_src), *d_exp = nullptr;
        int32_t *d_len = scratch.get<int32_t>(ld_src);
        {
            std::vector<double> yb(T * ld_src, 0.0);
            const std::vector<int32_t> len = block_lengths(lengths, N, ld_src);
            pack_time_major(yb.data(), ld_src, values, lengths, N);
            HIPCHECK(hipMemcpy(d_src, yb.data(), T * ld_src * sizeof(double), hipMemcpyHostToDevice));
            HIPCHECK(hipMemcpy(d_len, len.data(), ld_src * sizeof(int32_t), hipMemcpyHostToDevice));
        }
        try { d_exp = scratch.get<double>(t_train * ld_pairs); }
        catch (const HipFail &f) {
            if (!f.oom) throw;
            set_error(err, COMPUTATION_ERROR, "Computation error: the expanded backtest block of " + std::to_string(t_train) + " x " +
                      std::to_string(ld_pairs) + " values needs " + std::to_string(t_train * ld_pairs * sizeof(double)) + " bytes of device memory");
            ok = false;
        }
        if (ok) {
            double *d_fp = scratch.get<double>(n_fp);
            int32_t *d_in = scratch.get<int32_t>(n_int);
            double *d_yh = d_fp, *d_lo = d_fp + Nh, *d_hi = d_fp + 2 * Nh, *d_sel_yh = d_fp + 3 * Nh, *d_sel_act = d_sel_yh + nh,
                   *d_best = d_sel_act + nh, *d_scores = d_best + N;
            int32_t *d_winner = d_in, *d_stat = d_in + N, *d_code = d_in + 2 * N, *d_members = d_in + 3 * N, *d_offsets = d_in + 4 * N;
            int32_t *d_lenp = scratch.get<int32_t>(ld_pairs), *d_ntest = scratch.get<int32_t>(ld_pairs), *d_rows = scratch.get<int32_t>(std::max<size_t>(np, 1));
            double *d_bt_yh = scratch.get<double>(M * nh), *d_bt_act = scratch.get<double>(M * nh), *d_work = scratch.get<double>(2 * nh);
            int32_t *d_bt_stat = scratch.get<int32_t>(M * std::max<size_t>(np, 1)), *d_sstat = scratch.get<int32_t>(M * N);
            int32_t *d_flen = scratch.get<int32_t>(N);
            double *d_fig = scratch.get<double>((size_t)METRICS_N_FIG * ldN);
            uint8_t *d_ff = scratch.get<uint8_t>(N);
            {
                const std::vector<int32_t> flen(N, (int32_t)(F * h));
                HIPCHECK(hipMemcpy(d_flen, flen.data(), N * sizeof(int32_t), hipMemcpyHostToDevice));
                // a score row that is never written (no fold: nothing to score) is NaN with status 1
                const std::vector<double> nan_row(M * ldN, std::numeric_limits<double>::quiet_NaN());
                const std::vector<int32_t> one(M * N, 1);
                HIPCHECK(hipMemcpy(d_scores, nan_row.data(), M * ldN * sizeof(double), hipMemcpyHostToDevice));
                HIPCHECK(hipMemcpy(d_sstat, one.data(), M * N * sizeof(int32_t), hipMemcpyHostToDevice));
            }
            // ---- the backtest of every method on ONE expanded block, scored per series ----
            if (np > 0)
                ok = anofox_hip_backtest_expand_device(d_src, ld_src, d_len, N, T, folds, F, t_train, d_exp, ld_pairs, d_lenp, d_ntest, st, err);
            for (size_t m = 0; ok && np > 0 && m < M; m++) {
                BatchOwner own;
                ok = select_run_batch(&methods[m], np, t_train, d_exp, ld_pairs, d_lenp, &own, err) &&
                     anofox_hip_backtest_collect_device(d_src, ld_src, N, T, folds, F, d_ntest, own.b->d_status, own.b->d_yhat, nullptr, nullptr, h,
                                                        criterion, d_bt_act + m * nh, d_work, d_work + nh, nullptr, d_rows, nullptr, st, err);
                if (!ok) break;
                HIPCHECK(hipMemcpy(d_bt_yh + m * nh, own.b->d_yhat, nh * sizeof(double), hipMemcpyDeviceToDevice));
                HIPCHECK(hipMemcpy(d_bt_stat + m * np, own.b->d_status, np * sizeof(int32_t), hipMemcpyDeviceToDevice));
                ok = anofox_hip_metrics_device(d_bt_act + m * nh, d_bt_yh + m * nh, nullptr, nullptr, nullptr, nullptr, 0, nullptr, 0, F * h, 1, d_flen,
                                               N, F * h, 1u << figure, 0.5, true, d_fig, ldN, d_sstat + m * N, st, err);
                if (ok) HIPCHECK(hipMemcpy(d_scores + m * ldN, d_fig + (size_t)figure * ldN, N * sizeof(double), hipMemcpyDeviceToDevice));
            }
            // ---- the choice ----
            if (ok)
                ok = anofox_hip_select_winner_device(d_scores, ldN, d_sstat, M, N, fallback, d_winner, d_best, d_ff, d_offsets, d_members, st, err);
            std::vector<int32_t> offs(M + 1, 0), memb(N, 0);
            if (ok) {
                HIPCHECK(hipMemcpy(offs.data(), d_offsets, (M + 1) * sizeof(int32_t), hipMemcpyDeviceToHost));
                HIPCHECK(hipMemcpy(memb.data(), d_members, N * sizeof(int32_t), hipMemcpyDeviceToHost));
            }
            if (ok && pick) {
                // ---- winners only: one dense sub-batch per method that won something, scattered back to series order ----
                std::vector<SelectSubBatch> subs;
                ok = select_plan_report(select_sub_batches(offs.data(), M, N, &subs, &message), message, err);
                for (size_t k = 0; ok && k < subs.size(); k++) {
                    const SelectSubBatch &sb = subs[k];
                    double *d_sub = scratch.get<double>(T * sb.ld_m);
                    int32_t *d_sublen = scratch.get<int32_t>(sb.ld_m);
                    BatchOwner own;
                    ok = anofox_hip_select_gather_device(d_src, ld_src, d_len, N, T, d_members, sb.off, sb.n_m, d_sub, sb.ld_m, d_sublen, st, err) &&
                         select_run_batch(&methods[sb.method], sb.n_m, T, d_sub, sb.ld_m, d_sublen, &own, err) &&
                         anofox_hip_select_scatter_device(own.b->d_yhat, own.b->d_lo, own.b->d_hi, own.b->d_model_code, own.b->d_status, d_members, sb.off,
                                                          sb.n_m, h, nullptr, N, d_yh, d_lo, d_hi, d_code, d_stat, st, err);
                    if (ok && out_model_names) {
                        std::vector<int32_t> code(sb.n_m), stat(sb.n_m);
                        HIPCHECK(hipMemcpy(code.data(), own.b->d_model_code, sb.n_m * sizeof(int32_t), hipMemcpyDeviceToHost));
                        HIPCHECK(hipMemcpy(stat.data(), own.b->d_status, sb.n_m * sizeof(int32_t), hipMemcpyDeviceToHost));
                        for (size_t j = 0; j < sb.n_m; j++) {
                            char name[64];
                            name[0] = 0;
                            if (stat[j] == 0) anofox_hip_batch_model_name(own.b, j, code[j], name);
                            names[(size_t)memb[sb.off + j]] = name;
                        }
                    }
                }
                if (ok)                                           // the series nobody won
                    ok = anofox_hip_select_scatter_device(nullptr, nullptr, nullptr, nullptr, nullptr, d_members, 0, 0, h, d_winner, N, d_yh, d_lo, d_hi,
                                                          d_code, d_stat, st, err);
            } else if (ok) {
                // ---- an ensemble: every method on the whole block, combined per cell; no combined intervals (lower and upper are NaN) ----
                double *d_full = scratch.get<double>(M * Nh);
                int32_t *d_fstat = scratch.get<int32_t>(M * N);
                for (size_t m = 0; ok && m < M; m++) {
                    BatchOwner own;
                    ok = select_run_batch(&methods[m], N, T, d_src, ld_src, d_len, &own, err);
                    if (!ok) break;
                    HIPCHECK(hipMemcpy(d_full + m * Nh, own.b->d_yhat, Nh * sizeof(double), hipMemcpyDeviceToDevice));
                    HIPCHECK(hipMemcpy(d_fstat + m * N, own.b->d_status, N * sizeof(int32_t), hipMemcpyDeviceToDevice));
                }
                if (ok) {
                    const double *tab[SELECT_MAX_METHODS];
                    for (size_t m = 0; m < M; m++) tab[m] = d_full + m * Nh;
                    ok = anofox_hip_select_combine_device(tab, M, N, h, d_fstat, mode_code, d_winner, d_scores, ldN, 1, d_yh, d_stat, st, err);
                }
                if (ok) {
                    const std::vector<double> nan_block(2 * Nh, std::numeric_limits<double>::quiet_NaN());
                    HIPCHECK(hipMemcpy(d_lo, nan_block.data(), 2 * Nh * sizeof(double), hipMemcpyHostToDevice));
                    HIPCHECK(hipMemset(d_code, 0, N * sizeof(int32_t)));
                }
            }
            // ---- the picked or combined backtest forecasts, in the layout of the methods' own ----
            if (ok && np > 0) {
                const double *tab[SELECT_MAX_METHODS];
                for (size_t m = 0; m < M; m++) tab[m] = d_bt_yh + m * nh;
                ok = anofox_hip_select_combine_device(tab, M, np, h, d_bt_stat, mode_code, d_winner, d_scores, ldN, F, d_sel_yh, nullptr, st, err);
                if (ok && pick) {
                    for (size_t m = 0; m < M; m++) tab[m] = d_bt_act + m * nh;
                    ok = anofox_hip_select_combine_device(tab, M, np, h, d_bt_stat, SELECT_PICK, d_winner, nullptr, 0, F, d_sel_act, nullptr, st, err);
                } else if (ok) {                                  // the test rows of every live pair, whatever became of its forecasts
                    int32_t *d_zero = scratch.get<int32_t>(np);
                    HIPCHECK(hipMemset(d_zero, 0, np * sizeof(int32_t)));
                    ok = anofox_hip_backtest_collect_device(d_src, ld_src, N, T, folds, F, d_ntest, d_zero, d_sel_yh, nullptr, nullptr, h, criterion,
                                                            d_sel_act, d_work, d_work + nh, nullptr, d_rows, nullptr, st, err);
                }
            }
            if (ok) {
                HIPCHECK(hipMemcpy(fp.data(), d_fp, n_fp * sizeof(double), hipMemcpyDeviceToHost));
                HIPCHECK(hipMemcpy(in.data(), d_in, n_int * sizeof(int32_t), hipMemcpyDeviceToHost));
            } else {
                HIPCHECK(hipDeviceSynchronize());
            }
        }
        scratch.settled();
    } catch (const HipFail &f) {
        report_hip_failure(err, f);
        return false;
    }
    if (!ok) {
        if (err && err->code == SUCCESS) set_error(err, INTERNAL_ERROR, "Internal error: device batch failed");
        return false;
    }
    const double *yh = fp.data(), *lo = yh + Nh, *hi = yh + 2 * Nh, *sel_yh = yh + 3 * Nh, *sel_act = sel_yh + nh, *best = sel_act + nh,
                 *scores = best + N;
    const int32_t *winner = in.data(), *stat = winner + N;
    if (out_winner) std::memcpy(out_winner, winner, N * sizeof(int32_t));
    if (out_best_score) std::memcpy(out_best_score, best, N * sizeof(double));
    if (out_scores)
        for (size_t m = 0; m < M; m++) std::memcpy(out_scores + m * N, scores + m * ldN, N * sizeof(double));
    if (out_yhat) std::memcpy(out_yhat, yh, Nh * sizeof(double));
    if (out_lower) std::memcpy(out_lower, lo, Nh * sizeof(double));
    if (out_upper) std::memcpy(out_upper, hi, Nh * sizeof(double));
    for (size_t s = 0; s < N; s++) {
        // pick: the sub-batch's status; an ensemble: the combine's row status (1: no member gave a forecast)
        const int32_t st_s = pick ? (stat[s] == STATUS_NOT_COMPUTED ? (int32_t)INTERNAL_ERROR : stat[s]) : (stat[s] == 0 ? 0 : (int32_t)INSUFFICIENT_DATA);
        if (out_status) out_status[s] = st_s;
        if (out_model_names) {
            out_model_names[s][0] = 0;
            if (st_s == 0) std::snprintf(out_model_names[s], 64, "%s", pick ? names[s].c_str() : mode);
        }
    }
    if (out_backtest_yhat && nh) std::memcpy(out_backtest_yhat, sel_yh, nh * sizeof(double));
    if (out_backtest_actual && nh) std::memcpy(out_backtest_actual, sel_act, nh * sizeof(double));
    if (out_n_rows)
        for (size_t p = 0; p < np; p++) {
            int32_t k = 0;
            for (size_t i = 0; i < h; i++) k += (sel_yh[p * h + i] == sel_yh[p * h + i] && sel_act[p * h + i] == sel_act[p * h + i]) ? 1 : 0;
            out_n_rows[p] = k;
        }
    return true;
}

} // extern "C"

// ------------------------------------------------------------------------------------------------------------------------------
// Bootstrap sample paths and their quantiles (DESIGN.md section 3 "Sample paths"; paths.hip, host_paths_plan.hpp)
// ------------------------------------------------------------------------------------------------------------------------------
namespace {

bool paths_plan_report(PathsPlanResult r, const std::string &message, AnofoxError *err)
{
    if (r == PATHS_PLAN_OK) return true;
    if (r == PATHS_PLAN_NULL) set_error(err, NULL_POINTER, "Null pointer argument");
    else set_error(err, INVALID_INPUT, message);
    return false;
}

bool paths_options_ok(const AnofoxHipPathsOptions *o, size_t struct_size, AnofoxError *err)
{
    std::string message;
    // (the fields are read only once the size has been found right)
    const bool readable = o && struct_size == sizeof(AnofoxHipPathsOptions);
    return paths_plan_report(paths_options_check(o != nullptr, struct_size, sizeof(AnofoxHipPathsOptions), readable ? o->mode : 0,
                                                 readable ? o->joint : 0, readable ? o->route : 0, &message), message, err);
}

} // namespace

extern "C" {

static_assert(sizeof(AnofoxHipPathsOptions) == 24 && offsetof(AnofoxHipPathsOptions, seed) == 16, "AnofoxHipPathsOptions layout");
static_assert(PATHS_PLAN_MAX_PATHS == (size_t)PATHS_MAX_PATHS && PATHS_PLAN_MAX_LEVELS == (size_t)PATHS_MAX_LEVELS &&
              PATHS_PLAN_MAX_POOL_ROWS == PATHS_MAX_POOL_ROWS && PATHS_PLAN_MAX_ROWS == PATHS_MAX_ROWS &&
              PATHS_MAX_PATHS == ANOFOX_HIP_PATHS_MAX_PATHS && PATHS_MAX_LEVELS == ANOFOX_HIP_PATHS_MAX_LEVELS &&
              PATHS_MAX_POOL_ROWS == ANOFOX_HIP_PATHS_MAX_POOL_ROWS && PATHS_MAX_ROWS == (size_t)HIER_SPAN_MAX, "the limits of the sample-path entries");

bool anofox_hip_paths_device(const double *point, size_t point_stride_s, size_t point_stride_t, const double *pool, size_t pool_stride_s,
                             size_t pool_stride_t, const int32_t *pool_lengths, size_t pool_rows, size_t n_series, size_t horizon, size_t n_paths,
                             const AnofoxHipPathsOptions *options, size_t struct_size, double *paths_out, size_t ld_out, int32_t *status,
                             void *stream, AnofoxError *out_error)
{
    clear_error(out_error);
    std::string message;
    if (!paths_options_ok(options, struct_size, out_error)) return false;
    if (!point || !paths_out || !status || (pool_rows > 0 && !pool)) { set_error(out_error, NULL_POINTER, "Null pointer argument"); return false; }
    if (!paths_plan_report(paths_rows_check(horizon, n_paths, &message), message, out_error)) return false;
    if (!paths_plan_report(paths_pool_check(pool_rows, &message), message, out_error)) return false;
    if (!paths_plan_report(paths_block_check(ld_out, n_series, "ld_out", "n_series", &message), message, out_error)) return false;
    if (n_series == 0) return true;
    if (!device_ready(out_error)) return false;
    PathsArgs a{};
    a.point = point; a.point_stride_s = point_stride_s; a.point_stride_t = point_stride_t;
    a.pool = pool; a.pool_stride_s = pool_stride_s; a.pool_stride_t = pool_stride_t; a.pool_len = pool_lengths;
    a.pool_rows = (int)pool_rows; a.n_series = (int)n_series; a.horizon = (int)horizon; a.n_paths = (int)n_paths;
    a.mode = options->mode; a.joint = options->joint;
    a.key0 = (uint32_t)(options->seed & 0xffffffffull); a.key1 = (uint32_t)(options->seed >> 32);
    a.paths = paths_out; a.ld_out = ld_out; a.status = status;
    try {
        (void)hipGetLastError();
        launch_paths(a, (hipStream_t)stream);
        LAUNCHCHECK("paths");
    } catch (const HipFail &f) {
        report_hip_failure(out_error, f);
        return false;
    }
    return true;
}

bool anofox_hip_path_quantiles_device(const double *paths, size_t ld, size_t n_cols, size_t horizon, size_t n_paths, const double *levels,
                                      size_t n_levels, double *out, int32_t *status, void *stream, AnofoxError *out_error)
{
    clear_error(out_error);
    std::string message;
    if (!paths || !out || !status) { set_error(out_error, NULL_POINTER, "Null pointer argument"); return false; }
    if (!paths_plan_report(paths_rows_check(horizon, n_paths, &message), message, out_error)) return false;
    if (!paths_plan_report(paths_levels_check(levels, n_levels, &message), message, out_error)) return false;
    if (!paths_plan_report(paths_block_check(ld, n_cols, "ld", "n_cols", &message), message, out_error)) return false;
    if (n_cols == 0) return true;
    if (!device_ready(out_error)) return false;
    PathQuantilesArgs a{};
    a.paths = paths; a.ld = ld; a.n_cols = (int)n_cols; a.horizon = (int)horizon; a.n_paths = (int)n_paths;
    a.n_levels = (int)n_levels;
    for (size_t k = 0; k < n_levels; k++) a.levels[k] = levels[k];
    a.out = out; a.status = status;
    try {
        (void)hipGetLastError();
        launch_path_quantiles(a, (hipStream_t)stream);
        LAUNCHCHECK("path quantiles");
    } catch (const HipFail &f) {
        report_hip_failure(out_error, f);
        return false;
    }
    return true;
}

bool anofox_hip_paths_batch(const double *points, const double *const *pools, const size_t *pool_lengths, size_t n_series, size_t horizon,
                            size_t n_paths, const AnofoxHipPathsOptions *options, size_t struct_size, const double *levels, size_t n_levels,
                            const int32_t *column_of, size_t n_groupings, size_t ld, double *out_quantiles, int32_t *out_status,
                            int32_t *out_series_status, double *out_paths, size_t *out_n_out, size_t *out_ld, AnofoxError *out_error)
{
    clear_error(out_error);
    std::string message;
    if (!paths_options_ok(options, struct_size, out_error)) return false;
    if (n_series > 0 && (!points || !pools || !pool_lengths)) { set_error(out_error, NULL_POINTER, "Null pointer argument"); return false; }
    if (!paths_plan_report(paths_rows_check(horizon, n_paths, &message), message, out_error)) return false;
    if (!paths_plan_report(paths_levels_check(levels, n_levels, &message), message, out_error)) return false;
    if (!paths_plan_report(paths_block_check(SIZE_MAX, n_series, "ld", "n_series", &message), message, out_error)) return false;
    size_t pool_rows = 0;
    if (!paths_plan_report(paths_batch_pools(pool_lengths, n_series, &pool_rows, &message), message, out_error)) return false;
    for (size_t s = 0; s < n_series; s++)
        if (pool_lengths[s] > 0 && !pools[s]) { set_error(out_error, NULL_POINTER, "Null pointer argument"); return false; }
    const bool planned = column_of != nullptr && n_groupings > 0;
    size_t n_out = n_series, nnz = 0;
    std::vector<int32_t> offs, memb;
    if (planned) {
        if (!anofox_hip_hierarchy_plan(column_of, n_groupings, n_series, &n_out, &nnz, nullptr, nullptr, out_error)) return false;
        offs.resize(n_out + 1);
        memb.resize(std::max<size_t>(nnz, 1));
        if (!anofox_hip_hierarchy_plan(column_of, n_groupings, n_series, &n_out, &nnz, offs.data(), memb.data(), out_error)) return false;
    }
    const size_t need_ld = paths_ld(n_out);
    if (out_n_out) *out_n_out = n_out;
    if (out_ld) *out_ld = need_ld;
    if (!out_quantiles) return true;
    if (ld != need_ld) { set_error(out_error, INVALID_INPUT, "Invalid input: ld is not what the sizing call returns"); return false; }
    if (!out_status) { set_error(out_error, NULL_POINTER, "Null pointer argument"); return false; }
    if (n_series == 0 || n_out == 0) return true;
    if (!device_ready(out_error)) return false;

    const size_t ld_s = paths_ld(n_series), rows = n_paths * horizon, pool_t = std::max<size_t>(pool_rows, 1);
    const size_t leaf_cells = rows * ld_s, out_cells = planned ? rows * need_ld : 0, q_cells = n_levels * n_out * horizon;
    Scratch scratch;
    bool ok = true;
    try {
        std::vector<double> pool_block(pool_t * ld_s, 0.0);
        const std::vector<int32_t> len = block_lengths(pool_lengths, n_series, ld_s);
        pack_time_major(pool_block.data(), ld_s, pools, pool_lengths, n_series);
        double *d_paths = nullptr, *d_agg = nullptr;
        try {
            d_paths = scratch.get<double>(leaf_cells);
            if (planned) d_agg = scratch.get<double>(out_cells);
        } catch (const HipFail &f) {
            if (!f.oom) throw;
            set_error(out_error, COMPUTATION_ERROR, "Computation error: the path block of " + std::to_string(rows) + " x " + std::to_string(ld_s) +
                      " values" + (planned ? " and its aggregate of " + std::to_string(rows) + " x " + std::to_string(need_ld) + " values" : std::string()) +
                      " need " + std::to_string((leaf_cells + out_cells) * sizeof(double)) + " bytes of device memory");
            ok = false;
        }
        if (ok) {
            double *d_point = scratch.get<double>(n_series * horizon);
            double *d_pool = scratch.get<double>(pool_t * ld_s);
            int32_t *d_len = scratch.get<int32_t>(ld_s);
            int32_t *d_status = scratch.get<int32_t>(ld_s);
            double *d_q = scratch.get<double>(q_cells);
            int32_t *d_qstatus = scratch.get<int32_t>(need_ld);
            HIPCHECK(hipMemcpy(d_point, points, n_series * horizon * sizeof(double), hipMemcpyHostToDevice));
            HIPCHECK(hipMemcpy(d_pool, pool_block.data(), pool_t * ld_s * sizeof(double), hipMemcpyHostToDevice));
            HIPCHECK(hipMemcpy(d_len, len.data(), ld_s * sizeof(int32_t), hipMemcpyHostToDevice));
            HIPCHECK(hipMemset(d_paths, 0, leaf_cells * sizeof(double)));          // the padding columns
            ok = anofox_hip_paths_device(d_point, horizon, 1, d_pool, 1, ld_s, d_len, pool_rows, n_series, horizon, n_paths, options, struct_size,
                                         d_paths, ld_s, d_status, nullptr, out_error);
            const double *d_block = d_paths;
            size_t ld_block = ld_s;
            if (ok && planned) {
                AnofoxHipHierarchyOptions ho{};
                std::vector<int32_t> full(ld_s, 0);
                for (size_t s = 0; s < n_series; s++) full[s] = (int32_t)rows;
                int32_t *d_rows = scratch.get<int32_t>(ld_s);
                int32_t *d_plan = scratch.get<int32_t>(n_out + 1 + nnz);
                int32_t *d_len_out = scratch.get<int32_t>(need_ld);
                int64_t *d_first_out = scratch.get<int64_t>(need_ld);
                HIPCHECK(hipMemcpy(d_rows, full.data(), ld_s * sizeof(int32_t), hipMemcpyHostToDevice));
                HIPCHECK(hipMemcpy(d_plan, offs.data(), (n_out + 1) * sizeof(int32_t), hipMemcpyHostToDevice));
                if (nnz) HIPCHECK(hipMemcpy(d_plan + n_out + 1, memb.data(), nnz * sizeof(int32_t), hipMemcpyHostToDevice));
                HIPCHECK(hipMemset(d_agg, 0, out_cells * sizeof(double)));
                ok = anofox_hip_hierarchy_device(d_paths, nullptr, nullptr, ld_s, d_rows, nullptr, n_series, rows, d_plan, d_plan + n_out + 1, n_out,
                                                 nnz, &ho, sizeof ho, rows, d_agg, nullptr, need_ld, d_len_out, d_first_out, nullptr, out_error);
                d_block = d_agg;
                ld_block = need_ld;
            }
            if (ok)
                ok = anofox_hip_path_quantiles_device(d_block, ld_block, n_out, horizon, n_paths, levels, n_levels, d_q, d_qstatus, nullptr,
                                                      out_error);
            if (ok) {
                HIPCHECK(hipMemcpy(out_quantiles, d_q, q_cells * sizeof(double), hipMemcpyDeviceToHost));      // waits for the null stream
                HIPCHECK(hipMemcpy(out_status, d_qstatus, n_out * sizeof(int32_t), hipMemcpyDeviceToHost));
                if (out_series_status) HIPCHECK(hipMemcpy(out_series_status, d_status, n_series * sizeof(int32_t), hipMemcpyDeviceToHost));
                if (out_paths) HIPCHECK(hipMemcpy(out_paths, d_block, rows * ld_block * sizeof(double), hipMemcpyDeviceToHost));
            } else HIPCHECK(hipDeviceSynchronize());
        }
        scratch.settled();                                                 // (either way the device has been waited for)
    } catch (const HipFail &f) {
        report_hip_failure(out_error, f);
        return false;
    }
    return ok;
}

} // extern "C"

// ------------------------------------------------------------------------------------------------------------------------------
// Sample paths simulated from the fitted ETS models (DESIGN.md section 3 "Model paths"; ets_paths.hip, host_ets_paths_plan.hpp)
// ------------------------------------------------------------------------------------------------------------------------------
namespace {

bool ets_paths_options_ok(const AnofoxHipEtsPathsOptions *o, size_t struct_size, AnofoxError *err)
{
    std::string message;
    // (the fields are read only once the size has been found right)
    const bool readable = o && struct_size == sizeof(AnofoxHipEtsPathsOptions);
    return paths_plan_report(ets_paths_options_check(o != nullptr, struct_size, sizeof(AnofoxHipEtsPathsOptions), readable ? o->innovations : 0,
                                                     readable ? o->joint : 0, &message), message, err);
}

} // namespace

extern "C" {

static_assert(sizeof(AnofoxHipEtsPathsOptions) == 24 && offsetof(AnofoxHipEtsPathsOptions, seed) == 16, "AnofoxHipEtsPathsOptions layout");
static_assert(ETS_PATHS_PLAN_MAX_PERIOD == (size_t)ETS_PATHS_MAX_PERIOD && ETS_PATHS_PLAN_MAX_RING == (size_t)ETS_PATHS_MAX_RING &&
              ETS_PATHS_MAX_PERIOD == ANOFOX_HIP_ETS_PATHS_MAX_PERIOD && ETS_PATHS_MAX_RING == ANOFOX_HIP_ETS_PATHS_MAX_RING &&
              ETS_PATHS_GAUSSIAN == ANOFOX_ETS_PATHS_GAUSSIAN && ETS_PATHS_BOOTSTRAP == ANOFOX_ETS_PATHS_BOOTSTRAP &&
              ETS_PATHS_NO_MODEL == ANOFOX_ETS_PATHS_NO_MODEL, "the limits and codes of the model-path entries");

bool anofox_hip_ets_innovations_device(const double *y, const double *fitted, size_t ld, const int32_t *lengths, const int32_t *spec,
                                       size_t n_series, size_t t_rows, double *pool, int32_t *pool_lengths, void *stream, AnofoxError *out_error)
{
    clear_error(out_error);
    std::string message;
    if (!y || !fitted || !lengths || !spec || !pool || !pool_lengths) { set_error(out_error, NULL_POINTER, "Null pointer argument"); return false; }
    if (!paths_plan_report(paths_block_check(ld, n_series, "ld", "n_series", &message), message, out_error)) return false;
    if (t_rows > (size_t)INT32_MAX) { set_error(out_error, INVALID_INPUT, "Invalid input: t_rows exceeds the limit of 2^31 - 1"); return false; }
    if (n_series == 0) return true;
    if (!device_ready(out_error)) return false;
    try {
        (void)hipGetLastError();
        launch_ets_innovations(y, fitted, ld, lengths, spec, (int)n_series, (int)t_rows, pool, pool_lengths, (hipStream_t)stream);
        LAUNCHCHECK("ets innovations");
    } catch (const HipFail &f) {
        report_hip_failure(out_error, f);
        return false;
    }
    return true;
}

bool anofox_hip_ets_paths_device(const int32_t *spec, const double *info, const double *states, size_t ld, size_t m, const int32_t *lengths,
                                 const double *pool, size_t pool_stride_s, size_t pool_stride_t, const int32_t *pool_lengths, size_t pool_rows,
                                 size_t n_series, size_t horizon, size_t n_paths, const AnofoxHipEtsPathsOptions *options, size_t struct_size,
                                 double *paths_out, size_t ld_out, int32_t *status, int32_t *n_broken, void *stream, AnofoxError *out_error)
{
    clear_error(out_error);
    std::string message;
    if (!ets_paths_options_ok(options, struct_size, out_error)) return false;
    if (!spec || !info || !states || !lengths || !paths_out || !status || !n_broken) { set_error(out_error, NULL_POINTER, "Null pointer argument"); return false; }
    if (!paths_plan_report(paths_rows_check(horizon, n_paths, &message), message, out_error)) return false;
    if (!paths_plan_report(paths_block_check(ld_out, n_series, "ld_out", "n_series", &message), message, out_error)) return false;
    if (!paths_plan_report(paths_block_check(ld, n_series, "ld", "n_series", &message), message, out_error)) return false;
    if (!paths_plan_report(ets_paths_period_check(m, horizon, &message), message, out_error)) return false;
    if (!paths_plan_report(ets_paths_pool_check(options->innovations, pool != nullptr, pool_rows, &message), message, out_error)) return false;
    if (n_series == 0) return true;
    if (!device_ready(out_error)) return false;
    const bool boot = options->innovations == ETS_PATHS_BOOTSTRAP;
    EtsPathsArgs a{};
    a.spec = spec; a.info = info; a.states = states; a.ld = ld; a.m = (int)m; a.lengths = lengths;
    a.innovations = options->innovations;
    a.pool = boot ? pool : nullptr; a.pool_stride_s = pool_stride_s; a.pool_stride_t = pool_stride_t;
    a.pool_len = boot ? pool_lengths : nullptr; a.pool_rows = boot ? (int)pool_rows : 0; a.joint = boot ? options->joint : 0;
    a.n_series = (int)n_series; a.horizon = (int)horizon; a.n_paths = (int)n_paths;
    a.key0 = (uint32_t)(options->seed & 0xffffffffull); a.key1 = (uint32_t)(options->seed >> 32);
    a.paths = paths_out; a.ld_out = ld_out; a.status = status; a.n_broken = n_broken;
    try {
        (void)hipGetLastError();
        launch_ets_paths(a, (hipStream_t)stream);
        LAUNCHCHECK("ets paths");
    } catch (const HipFail &f) {
        report_hip_failure(out_error, f);
        return false;
    }
    return true;
}

bool anofox_hip_batch_ets_paths(AnofoxHipBatch *b, const AnofoxHipEtsPathsOptions *options, size_t struct_size, size_t n_paths, const double *levels,
                                size_t n_levels, size_t ld, double *out_quantiles, int32_t *out_status, int32_t *out_series_status,
                                int32_t *out_n_broken, double *out_paths, size_t *out_ld, AnofoxError *out_error)
{
    clear_error(out_error);
    std::string message;
    if (!ets_paths_options_ok(options, struct_size, out_error)) return false;
    if (!paths_plan_report(paths_rows_check(1, n_paths, &message), message, out_error)) return false;
    if (!paths_plan_report(paths_levels_check(levels, n_levels, &message), message, out_error)) return false;
    if (!b) { set_error(out_error, NULL_POINTER, "Null pointer argument"); return false; }
    if (!b->ran) { set_error(out_error, INVALID_INPUT, "Invalid input: the batch has not been run"); return false; }
    if (!inspectable_ets(b)) {
        set_error(out_error, INVALID_INPUT, "Invalid input: model paths need an AutoETS or ETS(spec) batch");
        return false;
    }
    const size_t n = b->n, horizon = (size_t)std::max(b->h, 0), m = (size_t)std::max(b->insp_m, 1), need_ld = b->ld;
    if (!paths_plan_report(paths_rows_check(horizon, n_paths, &message), message, out_error)) return false;
    if (!paths_plan_report(ets_paths_period_check(m, horizon, &message), message, out_error)) return false;
    if (out_ld) *out_ld = need_ld;
    if (!out_quantiles) return true;
    if (ld != need_ld) { set_error(out_error, INVALID_INPUT, "Invalid input: ld is not what the sizing call returns"); return false; }
    if (!out_status) { set_error(out_error, NULL_POINTER, "Null pointer argument"); return false; }
    if (n == 0) return true;
    DeviceGuard guard(b->dev);

    const bool boot = options->innovations == ETS_PATHS_BOOTSTRAP;
    const size_t T = std::max<size_t>(b->t_max, 1), rows = n_paths * horizon, cells = rows * need_ld, q_cells = n_levels * n * horizon;
    Scratch scratch;
    bool ok = true;
    try {
        double *d_paths = nullptr;
        try {
            d_paths = scratch.get<double>(cells);
        } catch (const HipFail &f) {
            if (!f.oom) throw;
            set_error(out_error, COMPUTATION_ERROR, "Computation error: the path block of " + std::to_string(rows) + " x " + std::to_string(need_ld) +
                      " values needs " + std::to_string(cells * sizeof(double)) + " bytes of device memory");
            ok = false;
        }
        if (ok) {
            double *d_info = scratch.get<double>(8 * need_ld), *d_states = scratch.get<double>((2 + m) * need_ld);
            double *d_fit = boot ? scratch.get<double>(T * need_ld) : nullptr, *d_pool = boot ? scratch.get<double>(T * need_ld) : nullptr;
            int32_t *d_spec = scratch.get<int32_t>(need_ld), *d_plen = scratch.get<int32_t>(need_ld), *d_status = scratch.get<int32_t>(need_ld);
            int32_t *d_broken = scratch.get<int32_t>(need_ld), *d_qstatus = scratch.get<int32_t>(need_ld);
            double *d_q = scratch.get<double>(q_cells);
            b->quiesced = false;
            inspect_ets_passes(b, d_info, d_states, d_fit);
            HIPCHECK(hipStreamSynchronize(b->last_stream));
            (void)hipGetLastError();
            // (ETS(spec): the spec that was fitted -- a seasonal one without a usable period ran as its non-seasonal sibling)
            launch_ets_spec_of(b->d_model_code, b->d_status, b->plan.model == M_AutoETS ? 1 : 0, b->insp_spec.empty() ? -1 : b->insp_spec[0], (int)n,
                               d_spec, nullptr);
            LAUNCHCHECK("ets spec");
            HIPCHECK(hipMemset(d_paths, 0, cells * sizeof(double)));            // the padding columns
            if (boot)
                ok = anofox_hip_ets_innovations_device(b->d_y, d_fit, need_ld, b->d_len, d_spec, n, T, d_pool, d_plen, nullptr, out_error);
            if (ok)
                ok = anofox_hip_ets_paths_device(d_spec, d_info, d_states, need_ld, m, b->d_len, d_pool, 1, need_ld, boot ? d_plen : nullptr,
                                                 boot ? T : 0, n, horizon, n_paths, options, struct_size, d_paths, need_ld, d_status, d_broken,
                                                 nullptr, out_error);
            if (ok)
                ok = anofox_hip_path_quantiles_device(d_paths, need_ld, n, horizon, n_paths, levels, n_levels, d_q, d_qstatus, nullptr, out_error);
            if (ok) {
                HIPCHECK(hipMemcpy(out_quantiles, d_q, q_cells * sizeof(double), hipMemcpyDeviceToHost));      // waits for the null stream
                HIPCHECK(hipMemcpy(out_status, d_qstatus, n * sizeof(int32_t), hipMemcpyDeviceToHost));
                if (out_series_status) HIPCHECK(hipMemcpy(out_series_status, d_status, n * sizeof(int32_t), hipMemcpyDeviceToHost));
                if (out_n_broken) HIPCHECK(hipMemcpy(out_n_broken, d_broken, n * sizeof(int32_t), hipMemcpyDeviceToHost));
                if (out_paths) HIPCHECK(hipMemcpy(out_paths, d_paths, cells * sizeof(double), hipMemcpyDeviceToHost));
            } else HIPCHECK(hipDeviceSynchronize());
        }
        scratch.settled();                                                 // (either way the device has been waited for)
    } catch (const HipFail &f) {
        report_hip_failure(out_error, f);
        return false;
    } catch (const std::exception &e) {
        set_error(out_error, INTERNAL_ERROR, std::string("Internal error: ") + e.what());
        return false;
    }
    return ok;
}

} // extern "C"

// ------------------------------------------------------------------------------------------------------------------------------
// Sample paths simulated from the fitted AutoARIMA models (DESIGN.md section 3 "ARIMA paths"; arima_paths.hip,
// host_arima_paths_plan.hpp)
// ------------------------------------------------------------------------------------------------------------------------------
namespace {

bool arima_paths_options_ok(const AnofoxHipArimaPathsOptions *o, size_t struct_size, AnofoxError *err)
{
    std::string message;
    // (the fields are read only once the size has been found right)
    const bool readable = o && struct_size == sizeof(AnofoxHipArimaPathsOptions);
    return paths_plan_report(arima_paths_options_check(o != nullptr, struct_size, sizeof(AnofoxHipArimaPathsOptions), readable ? o->innovations : 0,
                                                       readable ? o->joint : 0, &message), message, err);
}

// developer knob arima_paths_waves of ANOFOX_HIP_TUNE: waves per workgroup of the simulation kernel (0, the default: as many as the LDS takes)
int arima_paths_waves_knob()
{
    const std::map<std::string, std::string> kv = Tunables::tune_map();
    auto it = kv.find("arima_paths_waves");
    const int w = it != kv.end() ? std::atoi(it->second.c_str()) : 0;
    return w < 0 ? 0 : w;
}

// what anofox_hip_batch_arima_fit asks of a batch; throws HipFail for the cases that entry reports that way
bool arima_fit_batch_ok(AnofoxHipBatch *b, const char *what, AnofoxError *out_error)
{
    if (!b->ran) { set_error(out_error, INVALID_INPUT, "Invalid input: the batch has not been run"); return false; }
    if (b->plan.model != M_AutoARIMA) { set_error(out_error, INVALID_INPUT, std::string("Invalid input: ") + what + " needs an AutoARIMA batch"); return false; }
    if (b->h_period.size() < b->n) throw HipFail{"the batch has no series block"};
    for (size_t s = 1; s < b->n; s++)
        if (b->h_period[s] != b->h_period[0]) throw HipFail{"the ARIMA fit readback needs one seasonal period for the whole batch"};
    return true;
}

// enqueues the fit-state kernel behind the batch's run
void arima_fit_state_pass(AnofoxHipBatch *b, int32_t *d_orders, double *d_coef)
{
    (void)hipGetLastError();
    launch_arima_fit_state(b->d_status, b->d_model_code, b->ar_order, b->ar_d, b->ar_D, b->ar_wlen, b->ar_x, b->ar_aicc, b->ld, (int)b->n,
                           d_orders, d_coef, b->last_stream);
    LAUNCHCHECK("arima fit state");
}

} // namespace

extern "C" {

static_assert(sizeof(AnofoxHipArimaPathsOptions) == 24 && offsetof(AnofoxHipArimaPathsOptions, seed) == 16, "AnofoxHipArimaPathsOptions layout");
static_assert(ARIMA_PATHS_PLAN_MAX_PERIOD == (size_t)ARIMA_PATHS_MAX_PERIOD && ARIMA_PATHS_PLAN_MAX_LDS_ROWS == (size_t)ARIMA_PATHS_MAX_LDS_ROWS &&
              ARIMA_PATHS_MAX_PERIOD == ANOFOX_HIP_ARIMA_PATHS_MAX_PERIOD && ARIMA_PATHS_MAX_LDS_ROWS == ANOFOX_HIP_ARIMA_PATHS_MAX_LDS_ROWS &&
              ARIMA_PATHS_GAUSSIAN == ANOFOX_ARIMA_PATHS_GAUSSIAN && ARIMA_PATHS_BOOTSTRAP == ANOFOX_ARIMA_PATHS_BOOTSTRAP &&
              ARIMA_PATHS_NO_MODEL == ANOFOX_ARIMA_PATHS_NO_MODEL, "the limits and codes of the ARIMA model-path entries");

bool anofox_hip_batch_arima_fit_device(AnofoxHipBatch *b, int32_t *d_orders, double *d_coef, AnofoxError *out_error)
{
    clear_error(out_error);
    if (!b || !d_orders || !d_coef) { set_error(out_error, NULL_POINTER, "Null pointer argument"); return false; }
    try {
        if (!arima_fit_batch_ok(b, "the ARIMA fit readback", out_error)) return false;
        if (b->n == 0) return true;
        DeviceGuard guard(b->dev);
        arima_fit_state_pass(b, d_orders, d_coef);
        HIPCHECK(hipStreamSynchronize(b->last_stream));
    } catch (const HipFail &f) {
        report_hip_failure(out_error, f);
        return false;
    } catch (const std::exception &e) {
        set_error(out_error, INTERNAL_ERROR, std::string("Internal error: ") + e.what());
        return false;
    }
    return true;
}

bool anofox_hip_arima_innovations_device(const int32_t *orders, const double *coef, size_t ld, const double *y, const int32_t *lengths, size_t m,
                                         size_t n_series, size_t t_rows, double *resid, int32_t *resid_lengths, double *sigma, void *stream,
                                         AnofoxError *out_error)
{
    clear_error(out_error);
    std::string message;
    if (!orders || !coef || !y || !lengths || !resid || !resid_lengths || !sigma) { set_error(out_error, NULL_POINTER, "Null pointer argument"); return false; }
    if (!paths_plan_report(paths_block_check(ld, n_series, "ld", "n_series", &message), message, out_error)) return false;
    if (!paths_plan_report(arima_paths_rows_limit_check(t_rows, &message), message, out_error)) return false;
    if (!paths_plan_report(arima_paths_period_check(m, &message), message, out_error)) return false;
    if (n_series == 0) return true;
    if (!device_ready(out_error)) return false;
    try {
        (void)hipGetLastError();
        launch_arima_innovations(orders, coef, ld, y, lengths, (int)t_rows, (int)m, (int)n_series, resid, resid_lengths, sigma, (hipStream_t)stream);
        LAUNCHCHECK("arima innovations");
    } catch (const HipFail &f) {
        report_hip_failure(out_error, f);
        return false;
    }
    return true;
}

bool anofox_hip_arima_paths_device(const int32_t *orders, const double *coef, size_t ld, const double *y, const int32_t *lengths, size_t t_rows,
                                   const double *resid, const int32_t *resid_lengths, const double *sigma, size_t m, size_t pool_rows,
                                   size_t n_series, size_t horizon, size_t n_paths, const AnofoxHipArimaPathsOptions *options, size_t struct_size,
                                   double *paths_out, size_t ld_out, int32_t *status, int32_t *n_broken, void *stream, AnofoxError *out_error)
{
    clear_error(out_error);
    std::string message;
    if (!arima_paths_options_ok(options, struct_size, out_error)) return false;
    if (!orders || !coef || !y || !lengths || !resid || !resid_lengths || !sigma || !paths_out || !status || !n_broken) {
        set_error(out_error, NULL_POINTER, "Null pointer argument");
        return false;
    }
    if (!paths_plan_report(paths_rows_check(horizon, n_paths, &message), message, out_error)) return false;
    if (!paths_plan_report(paths_block_check(ld_out, n_series, "ld_out", "n_series", &message), message, out_error)) return false;
    if (!paths_plan_report(paths_block_check(ld, n_series, "ld", "n_series", &message), message, out_error)) return false;
    if (!paths_plan_report(arima_paths_rows_limit_check(t_rows, &message), message, out_error)) return false;
    if (!paths_plan_report(arima_paths_ring_check(m, horizon, &message), message, out_error)) return false;
    if (!paths_plan_report(arima_paths_pool_check(options->joint, pool_rows, &message), message, out_error)) return false;
    if (n_series == 0) return true;
    if (!device_ready(out_error)) return false;
    const bool boot = options->innovations == ARIMA_PATHS_BOOTSTRAP;
    ArimaPathsArgs a{};
    a.orders = orders; a.coef = coef; a.ld = ld; a.y = y; a.lengths = lengths; a.t_rows = (int)t_rows;
    a.resid = resid; a.resid_len = resid_lengths; a.sigma = sigma;
    a.m = (int)m; a.innovations = options->innovations; a.joint = boot ? options->joint : 0; a.pool_rows = a.joint ? (int)pool_rows : 0;
    a.n_series = (int)n_series; a.horizon = (int)horizon; a.n_paths = (int)n_paths;
    a.key0 = (uint32_t)(options->seed & 0xffffffffull); a.key1 = (uint32_t)(options->seed >> 32);
    a.paths = paths_out; a.ld_out = ld_out; a.status = status; a.n_broken = n_broken;
    a.waves = arima_paths_waves_knob();
    try {
        (void)hipGetLastError();
        launch_arima_paths(a, (hipStream_t)stream);
        LAUNCHCHECK("arima paths");
    } catch (const HipFail &f) {
        report_hip_failure(out_error, f);
        return false;
    }
    return true;
}

bool anofox_hip_batch_arima_paths(AnofoxHipBatch *b, const AnofoxHipArimaPathsOptions *options, size_t struct_size, size_t n_paths,
                                  const double *levels, size_t n_levels, size_t ld, double *out_quantiles, int32_t *out_status,
                                  int32_t *out_series_status, int32_t *out_n_broken, double *out_paths, size_t *out_ld, AnofoxError *out_error)
{
    clear_error(out_error);
    std::string message;
    if (!arima_paths_options_ok(options, struct_size, out_error)) return false;
    if (!paths_plan_report(paths_rows_check(1, n_paths, &message), message, out_error)) return false;
    if (!paths_plan_report(paths_levels_check(levels, n_levels, &message), message, out_error)) return false;
    if (!b) { set_error(out_error, NULL_POINTER, "Null pointer argument"); return false; }
    Scratch scratch;
    bool ok = true;
    try {
        if (!arima_fit_batch_ok(b, "ARIMA model paths", out_error)) return false;
        const size_t n = b->n, horizon = (size_t)std::max(b->h, 0), m = (size_t)std::max(n ? b->h_period[0] : 1, 1), need_ld = b->ld;
        if (!paths_plan_report(paths_rows_check(horizon, n_paths, &message), message, out_error)) return false;
        if (!paths_plan_report(arima_paths_ring_check(m, horizon, &message), message, out_error)) return false;
        if (out_ld) *out_ld = need_ld;
        if (!out_quantiles) return true;
        if (ld != need_ld) { set_error(out_error, INVALID_INPUT, "Invalid input: ld is not what the sizing call returns"); return false; }
        if (!out_status) { set_error(out_error, NULL_POINTER, "Null pointer argument"); return false; }
        if (n == 0) return true;
        DeviceGuard guard(b->dev);
        const size_t T = std::max<size_t>(b->t_max, 1), rows = n_paths * horizon, cells = rows * need_ld, q_cells = n_levels * n * horizon;
        double *d_paths = nullptr;
        try {
            d_paths = scratch.get<double>(cells);
        } catch (const HipFail &f) {
            if (!f.oom) throw;
            set_error(out_error, COMPUTATION_ERROR, "Computation error: the path block of " + std::to_string(rows) + " x " + std::to_string(need_ld) +
                      " values needs " + std::to_string(cells * sizeof(double)) + " bytes of device memory");
            ok = false;
        }
        if (ok) {
            int32_t *d_orders = scratch.get<int32_t>(8 * need_ld), *d_rlen = scratch.get<int32_t>(need_ld), *d_status = scratch.get<int32_t>(need_ld);
            int32_t *d_broken = scratch.get<int32_t>(need_ld), *d_qstatus = scratch.get<int32_t>(need_ld);
            double *d_coef = scratch.get<double>(16 * need_ld), *d_resid = scratch.get<double>(T * need_ld), *d_sigma = scratch.get<double>(need_ld);
            double *d_q = scratch.get<double>(q_cells);
            arima_fit_state_pass(b, d_orders, d_coef);
            HIPCHECK(hipStreamSynchronize(b->last_stream));
            HIPCHECK(hipMemset(d_paths, 0, cells * sizeof(double)));            // the padding columns
            ok = anofox_hip_arima_innovations_device(d_orders, d_coef, need_ld, b->d_y, b->d_len, m, n, T, d_resid, d_rlen, d_sigma, nullptr, out_error);
            size_t pool_rows = 0;
            if (ok && options->joint) {                                        // the smallest nu among the fitted series
                std::vector<int32_t> rlen(n);
                HIPCHECK(hipMemcpy(rlen.data(), d_rlen, n * sizeof(int32_t), hipMemcpyDeviceToHost));      // waits for the null stream
                int32_t least = 0;
                for (size_t s = 0; s < n; s++)
                    if (rlen[s] > 0 && (least == 0 || rlen[s] < least)) least = rlen[s];
                pool_rows = (size_t)least;
            }
            if (ok)
                ok = anofox_hip_arima_paths_device(d_orders, d_coef, need_ld, b->d_y, b->d_len, T, d_resid, d_rlen, d_sigma, m, pool_rows, n, horizon,
                                                   n_paths, options, struct_size, d_paths, need_ld, d_status, d_broken, nullptr, out_error);
            if (ok)
                ok = anofox_hip_path_quantiles_device(d_paths, need_ld, n, horizon, n_paths, levels, n_levels, d_q, d_qstatus, nullptr, out_error);
            if (ok) {
                HIPCHECK(hipMemcpy(out_quantiles, d_q, q_cells * sizeof(double), hipMemcpyDeviceToHost));      // waits for the null stream
                HIPCHECK(hipMemcpy(out_status, d_qstatus, n * sizeof(int32_t), hipMemcpyDeviceToHost));
                if (out_series_status) HIPCHECK(hipMemcpy(out_series_status, d_status, n * sizeof(int32_t), hipMemcpyDeviceToHost));
                if (out_n_broken) HIPCHECK(hipMemcpy(out_n_broken, d_broken, n * sizeof(int32_t), hipMemcpyDeviceToHost));
                if (out_paths) HIPCHECK(hipMemcpy(out_paths, d_paths, cells * sizeof(double), hipMemcpyDeviceToHost));
            } else HIPCHECK(hipDeviceSynchronize());
        }
        scratch.settled();                                                 // (either way the device has been waited for)
    } catch (const HipFail &f) {
        report_hip_failure(out_error, f);
        return false;
    } catch (const std::exception &e) {
        set_error(out_error, INTERNAL_ERROR, std::string("Internal error: ") + e.what());
        return false;
    }
    return ok;
}

} // extern "C"

// ------------------------------------------------------------------------------------------------------------------------------
// Scores of sample paths: CRPS, pinball, ranks and energy score (DESIGN.md section 3 "Path scores"; path_scores.hip,
// host_path_scores_plan.hpp)
// ------------------------------------------------------------------------------------------------------------------------------
extern "C" {

static_assert(PATH_SCORES_OK == ANOFOX_PATH_SCORES_OK && PATH_SCORES_NO_ACTUAL == ANOFOX_PATH_SCORES_NO_ACTUAL &&
              PATH_SCORES_NAN == ANOFOX_PATH_SCORES_NAN, "the statuses of the path-score entries");

bool anofox_hip_path_scores_device(const double *paths, size_t ld, size_t n_cols, size_t horizon, size_t n_paths, const double *actual,
                                   size_t actual_stride_c, size_t actual_stride_k, const double *levels, size_t n_levels, double *out_crps,
                                   int32_t *out_below, int32_t *out_equal, double *out_quantiles, double *out_column, size_t ld_out,
                                   int32_t *status, void *stream, AnofoxError *out_error)
{
    clear_error(out_error);
    std::string message;
    if (!paths || !actual || !status) { set_error(out_error, NULL_POINTER, "Null pointer argument"); return false; }
    if (!paths_plan_report(paths_rows_check(horizon, n_paths, &message), message, out_error)) return false;
    if (!paths_plan_report(path_scores_levels_check(levels, n_levels, &message), message, out_error)) return false;
    if (!paths_plan_report(paths_block_check(ld, n_cols, "ld", "n_cols", &message), message, out_error)) return false;
    if (out_column && !paths_plan_report(paths_block_check(ld_out, n_cols, "ld_out", "n_cols", &message), message, out_error)) return false;
    if (n_cols == 0) return true;
    if (!device_ready(out_error)) return false;
    PathScoresArgs a{};
    a.paths = paths; a.ld = ld; a.n_cols = (int)n_cols; a.horizon = (int)horizon; a.n_paths = (int)n_paths;
    a.actual = actual; a.actual_stride_c = actual_stride_c; a.actual_stride_k = actual_stride_k;
    a.n_levels = (int)n_levels;
    for (size_t k = 0; k < n_levels; k++) a.levels[k] = levels[k];
    a.crps = out_crps; a.below = out_below; a.equal = out_equal; a.quantiles = n_levels ? out_quantiles : nullptr;
    a.column = out_column; a.ld_column = ld_out; a.status = status;
    try {
        (void)hipGetLastError();
        launch_path_scores(a, (hipStream_t)stream);
        LAUNCHCHECK("path scores");
    } catch (const HipFail &f) {
        report_hip_failure(out_error, f);
        return false;
    }
    return true;
}

bool anofox_hip_path_scores_sizes(size_t horizon, size_t n_paths, size_t *out_workspace_doubles, AnofoxError *out_error)
{
    clear_error(out_error);
    std::string message;
    if (!out_workspace_doubles) { set_error(out_error, NULL_POINTER, "Null pointer argument"); return false; }
    if (!paths_plan_report(paths_rows_check(horizon, n_paths, &message), message, out_error)) return false;
    *out_workspace_doubles = path_energy_workspace(horizon, n_paths);
    return true;
}

bool anofox_hip_path_energy_device(const double *paths, size_t ld, size_t col_begin, size_t col_end, size_t horizon, size_t n_paths,
                                   const double *actual, size_t actual_stride_c, size_t actual_stride_k, double *workspace, double *out_es,
                                   double *out_summary, void *stream, AnofoxError *out_error)
{
    clear_error(out_error);
    std::string message;
    if (!paths || !actual || !workspace || !out_es || !out_summary) { set_error(out_error, NULL_POINTER, "Null pointer argument"); return false; }
    if (!paths_plan_report(paths_rows_check(horizon, n_paths, &message), message, out_error)) return false;
    if (!paths_plan_report(path_energy_range_check(ld, col_begin, col_end, &message), message, out_error)) return false;
    if (!device_ready(out_error)) return false;
    PathEnergyArgs a{};
    a.paths = paths; a.ld = ld; a.col_begin = (int)col_begin; a.col_end = (int)col_end; a.horizon = (int)horizon; a.n_paths = (int)n_paths;
    a.actual = actual; a.actual_stride_c = actual_stride_c; a.actual_stride_k = actual_stride_k;
    a.workspace = workspace; a.es = out_es; a.summary = out_summary;
    try {
        (void)hipGetLastError();
        launch_path_energy(a, (hipStream_t)stream);
        LAUNCHCHECK("path energy");
    } catch (const HipFail &f) {
        report_hip_failure(out_error, f);
        return false;
    }
    return true;
}

bool anofox_hip_path_scores_batch(const double *points, const double *const *pools, const size_t *pool_lengths, size_t n_series, size_t horizon,
                                  size_t n_paths, const AnofoxHipPathsOptions *options, size_t struct_size, const double *levels, size_t n_levels,
                                  const int32_t *column_of, size_t n_groupings, const double *actuals, size_t ld, double *out_crps,
                                  int32_t *out_below, int32_t *out_equal, double *out_quantiles, double *out_column, int32_t *out_status,
                                  int32_t *out_series_status, double *out_energy, int32_t *out_ranges, size_t *out_n_out, size_t *out_ld,
                                  AnofoxError *out_error)
{
    clear_error(out_error);
    std::string message;
    if (!paths_options_ok(options, struct_size, out_error)) return false;
    if (n_series > 0 && (!points || !pools || !pool_lengths || !actuals)) { set_error(out_error, NULL_POINTER, "Null pointer argument"); return false; }
    if (!paths_plan_report(paths_rows_check(horizon, n_paths, &message), message, out_error)) return false;
    if (!paths_plan_report(path_scores_levels_check(levels, n_levels, &message), message, out_error)) return false;
    if (!paths_plan_report(paths_block_check(SIZE_MAX, n_series, "ld", "n_series", &message), message, out_error)) return false;
    size_t pool_rows = 0;
    if (!paths_plan_report(paths_batch_pools(pool_lengths, n_series, &pool_rows, &message), message, out_error)) return false;
    for (size_t s = 0; s < n_series; s++)
        if (pool_lengths[s] > 0 && !pools[s]) { set_error(out_error, NULL_POINTER, "Null pointer argument"); return false; }
    const bool planned = column_of != nullptr && n_groupings > 0;
    size_t n_out = n_series, nnz = 0;
    std::vector<int32_t> offs, memb;
    if (planned) {
        if (!anofox_hip_hierarchy_plan(column_of, n_groupings, n_series, &n_out, &nnz, nullptr, nullptr, out_error)) return false;
        offs.resize(n_out + 1);
        memb.resize(std::max<size_t>(nnz, 1));
        if (!anofox_hip_hierarchy_plan(column_of, n_groupings, n_series, &n_out, &nnz, offs.data(), memb.data(), out_error)) return false;
    }
    const size_t need_ld = paths_ld(n_out);
    if (out_n_out) *out_n_out = n_out;
    if (out_ld) *out_ld = need_ld;
    if (!out_status) return true;
    if (ld != need_ld) { set_error(out_error, INVALID_INPUT, "Invalid input: ld is not what the sizing call returns"); return false; }
    const size_t n_ranges = (planned ? n_groupings : 0) + 1, e_row = horizon + 2;
    std::vector<size_t> ranges(2 * n_ranges);
    path_scores_ranges(planned ? column_of : nullptr, n_groupings, n_series, n_out, ranges.data());
    if (out_ranges)
        for (size_t r = 0; r < 2 * n_ranges; r++) out_ranges[r] = (int32_t)ranges[r];
    if (out_energy)
        for (size_t r = 0; r < n_ranges * e_row; r++) out_energy[r] = std::numeric_limits<double>::quiet_NaN();
    if (n_series == 0 || n_out == 0) return true;
    if (!device_ready(out_error)) return false;

    const size_t ld_s = paths_ld(n_series), rows = n_paths * horizon, pool_t = std::max<size_t>(pool_rows, 1);
    const size_t leaf_cells = rows * ld_s, out_cells = planned ? rows * need_ld : 0, cells = n_out * horizon, q_cells = n_levels * cells;
    Scratch scratch;
    bool ok = true;
    try {
        std::vector<double> pool_block(pool_t * ld_s, 0.0);
        const std::vector<int32_t> len = block_lengths(pool_lengths, n_series, ld_s);
        pack_time_major(pool_block.data(), ld_s, pools, pool_lengths, n_series);
        double *d_paths = nullptr, *d_agg = nullptr;
        try {
            d_paths = scratch.get<double>(leaf_cells);
            if (planned) d_agg = scratch.get<double>(out_cells);
        } catch (const HipFail &f) {
            if (!f.oom) throw;
            set_error(out_error, COMPUTATION_ERROR, "Computation error: the path block of " + std::to_string(rows) + " x " + std::to_string(ld_s) +
                      " values" + (planned ? " and its aggregate of " + std::to_string(rows) + " x " + std::to_string(need_ld) + " values" : std::string()) +
                      " need " + std::to_string((leaf_cells + out_cells) * sizeof(double)) + " bytes of device memory");
            ok = false;
        }
        if (ok) {
            double *d_point = scratch.get<double>(n_series * horizon);
            double *d_pool = scratch.get<double>(pool_t * ld_s);
            int32_t *d_len = scratch.get<int32_t>(ld_s);
            int32_t *d_status = scratch.get<int32_t>(ld_s);
            double *d_crps = scratch.get<double>(cells);
            int32_t *d_below = scratch.get<int32_t>(cells), *d_equal = scratch.get<int32_t>(cells);
            double *d_q = scratch.get<double>(std::max<size_t>(q_cells, 1));
            double *d_column = scratch.get<double>((2 + n_levels) * need_ld);
            int32_t *d_cstatus = scratch.get<int32_t>(need_ld);
            double *d_work = scratch.get<double>(path_energy_workspace(horizon, n_paths));
            double *d_energy = scratch.get<double>(n_ranges * e_row);
            HIPCHECK(hipMemcpy(d_point, points, n_series * horizon * sizeof(double), hipMemcpyHostToDevice));
            HIPCHECK(hipMemcpy(d_pool, pool_block.data(), pool_t * ld_s * sizeof(double), hipMemcpyHostToDevice));
            HIPCHECK(hipMemcpy(d_len, len.data(), ld_s * sizeof(int32_t), hipMemcpyHostToDevice));
            HIPCHECK(hipMemset(d_paths, 0, leaf_cells * sizeof(double)));          // the padding columns
            HIPCHECK(hipMemset(d_column, 0, (2 + n_levels) * need_ld * sizeof(double)));
            ok = anofox_hip_paths_device(d_point, horizon, 1, d_pool, 1, ld_s, d_len, pool_rows, n_series, horizon, n_paths, options, struct_size,
                                         d_paths, ld_s, d_status, nullptr, out_error);
            const double *d_block = d_paths, *d_actual = nullptr;
            size_t ld_block = ld_s, stride_c = horizon, stride_k = 1;
            if (ok && !planned) {
                double *d_act = scratch.get<double>(n_series * horizon);
                HIPCHECK(hipMemcpy(d_act, actuals, n_series * horizon * sizeof(double), hipMemcpyHostToDevice));
                d_actual = d_act;
            }
            if (ok && planned) {
                AnofoxHipHierarchyOptions ho{};
                std::vector<int32_t> full(ld_s, 0), steps(ld_s, 0);
                for (size_t s = 0; s < n_series; s++) { full[s] = (int32_t)rows; steps[s] = (int32_t)horizon; }
                std::vector<double> act_block(horizon * ld_s, 0.0);              // the actuals, time-major as the path block is
                for (size_t s = 0; s < n_series; s++)
                    for (size_t k = 0; k < horizon; k++) act_block[k * ld_s + s] = actuals[s * horizon + k];
                int32_t *d_rows = scratch.get<int32_t>(ld_s), *d_steps = scratch.get<int32_t>(ld_s);
                int32_t *d_plan = scratch.get<int32_t>(n_out + 1 + nnz);
                int32_t *d_len_out = scratch.get<int32_t>(need_ld);
                int64_t *d_first_out = scratch.get<int64_t>(need_ld);
                double *d_act = scratch.get<double>(horizon * ld_s), *d_act_agg = scratch.get<double>(horizon * need_ld);
                HIPCHECK(hipMemcpy(d_rows, full.data(), ld_s * sizeof(int32_t), hipMemcpyHostToDevice));
                HIPCHECK(hipMemcpy(d_steps, steps.data(), ld_s * sizeof(int32_t), hipMemcpyHostToDevice));
                HIPCHECK(hipMemcpy(d_act, act_block.data(), horizon * ld_s * sizeof(double), hipMemcpyHostToDevice));
                HIPCHECK(hipMemcpy(d_plan, offs.data(), (n_out + 1) * sizeof(int32_t), hipMemcpyHostToDevice));
                if (nnz) HIPCHECK(hipMemcpy(d_plan + n_out + 1, memb.data(), nnz * sizeof(int32_t), hipMemcpyHostToDevice));
                HIPCHECK(hipMemset(d_agg, 0, out_cells * sizeof(double)));
                HIPCHECK(hipMemset(d_act_agg, 0, horizon * need_ld * sizeof(double)));
                ok = anofox_hip_hierarchy_device(d_paths, nullptr, nullptr, ld_s, d_rows, nullptr, n_series, rows, d_plan, d_plan + n_out + 1, n_out,
                                                 nnz, &ho, sizeof ho, rows, d_agg, nullptr, need_ld, d_len_out, d_first_out, nullptr, out_error);
                if (ok)
                    ok = anofox_hip_hierarchy_device(d_act, nullptr, nullptr, ld_s, d_steps, nullptr, n_series, horizon, d_plan, d_plan + n_out + 1,
                                                     n_out, nnz, &ho, sizeof ho, horizon, d_act_agg, nullptr, need_ld, d_len_out, d_first_out, nullptr,
                                                     out_error);
                d_block = d_agg;
                ld_block = need_ld;
                d_actual = d_act_agg;
                stride_c = 1;
                stride_k = need_ld;
            }
            if (ok)
                ok = anofox_hip_path_scores_device(d_block, ld_block, n_out, horizon, n_paths, d_actual, stride_c, stride_k, levels, n_levels, d_crps,
                                                   d_below, d_equal, d_q, d_column, need_ld, d_cstatus, nullptr, out_error);
            for (size_t r = 0; ok && out_energy && r < n_ranges; r++) {
                if (ranges[2 * r + 1] <= ranges[2 * r]) continue;                 // a grouping that maps no series: NaN
                ok = anofox_hip_path_energy_device(d_block, ld_block, ranges[2 * r], ranges[2 * r + 1], horizon, n_paths, d_actual, stride_c, stride_k,
                                                   d_work, d_energy + r * e_row, d_energy + r * e_row + horizon, nullptr, out_error);
            }
            if (ok) {
                if (out_crps) HIPCHECK(hipMemcpy(out_crps, d_crps, cells * sizeof(double), hipMemcpyDeviceToHost));      // waits for the null stream
                if (out_below) HIPCHECK(hipMemcpy(out_below, d_below, cells * sizeof(int32_t), hipMemcpyDeviceToHost));
                if (out_equal) HIPCHECK(hipMemcpy(out_equal, d_equal, cells * sizeof(int32_t), hipMemcpyDeviceToHost));
                if (out_quantiles && q_cells) HIPCHECK(hipMemcpy(out_quantiles, d_q, q_cells * sizeof(double), hipMemcpyDeviceToHost));
                if (out_column) HIPCHECK(hipMemcpy(out_column, d_column, (2 + n_levels) * need_ld * sizeof(double), hipMemcpyDeviceToHost));
                HIPCHECK(hipMemcpy(out_status, d_cstatus, n_out * sizeof(int32_t), hipMemcpyDeviceToHost));
                if (out_series_status) HIPCHECK(hipMemcpy(out_series_status, d_status, n_series * sizeof(int32_t), hipMemcpyDeviceToHost));
                if (out_energy)
                    for (size_t r = 0; r < n_ranges; r++)
                        if (ranges[2 * r + 1] > ranges[2 * r])
                            HIPCHECK(hipMemcpy(out_energy + r * e_row, d_energy + r * e_row, e_row * sizeof(double), hipMemcpyDeviceToHost));
            } else HIPCHECK(hipDeviceSynchronize());
        }
        scratch.settled();                                                 // (either way the device has been waited for)
    } catch (const HipFail &f) {
        report_hip_failure(out_error, f);
        return false;
    }
    return ok;
}

} // extern "C"

// ------------------------------------------------------------------------------------------------------------------------------
// Scaled, weighted scores of a hierarchy: the in-sample scale, RMSSE / MASE / SPL and their weighted means, WRMSSE and WSPL
// (DESIGN.md section 3 "Scaled scores"; scaled_scores.hip, host_scaled_scores_plan.hpp)
// ------------------------------------------------------------------------------------------------------------------------------
extern "C" {

static_assert(SCALE_OK == ANOFOX_SCALE_OK && SCALE_SHORT == ANOFOX_SCALE_SHORT && SCALE_NAN == ANOFOX_SCALE_NAN &&
              SCALE_CONSTANT == ANOFOX_SCALE_CONSTANT && SCALED_MAX_LOSS == ANOFOX_HIP_SCALED_MAX_LOSS, "the constants of the scaled-score entries");

bool anofox_hip_scale_device(const double *y, size_t ld, const int32_t *lengths, size_t n_cols, size_t t_rows, const double *w_src, size_t lag,
                             bool trim_leading_zeros, size_t tail_rows, double *out_scale, size_t ld_out, int32_t *out_first, int32_t *status,
                             void *stream, AnofoxError *out_error)
{
    clear_error(out_error);
    std::string message;
    if (!y || !lengths || !out_scale || !out_first || !status) { set_error(out_error, NULL_POINTER, "Null pointer argument"); return false; }
    if (!paths_plan_report(scale_check(ld, n_cols, t_rows, lag, tail_rows, ld_out, &message), message, out_error)) return false;
    if (n_cols == 0) return true;
    if (!device_ready(out_error)) return false;
    ScaleArgs a{};
    a.y = y; a.ld = ld; a.w_src = w_src ? w_src : y; a.len = lengths; a.n_cols = (int)n_cols; a.t_rows = (int)t_rows; a.lag = (int)lag;
    a.tail_rows = (int)tail_rows; a.trim = trim_leading_zeros ? 1 : 0; a.out = out_scale; a.ld_out = ld_out; a.first = out_first; a.status = status;
    try {
        (void)hipGetLastError();
        launch_scale(a, (hipStream_t)stream);
        LAUNCHCHECK("scale");
    } catch (const HipFail &f) {
        report_hip_failure(out_error, f);
        return false;
    }
    return true;
}

bool anofox_hip_weighted_scores_device(const double *loss, size_t ld, size_t n_cols, size_t n_loss, const double *scale, const double *weight,
                                       const int32_t *col_status, const int32_t *ranges, size_t n_ranges, int32_t transform, double *out_scaled,
                                       double *out_score, double *out_weight_sum, int32_t *out_left, double *out_total, void *stream,
                                       AnofoxError *out_error)
{
    clear_error(out_error);
    std::string message;
    if (!loss || !scale || !weight || !ranges || !out_score || !out_weight_sum || !out_left || !out_total) {
        set_error(out_error, NULL_POINTER, "Null pointer argument");
        return false;
    }
    if (!paths_plan_report(weighted_scores_check(ld, n_cols, n_loss, n_ranges, transform, &message), message, out_error)) return false;
    if (!device_ready(out_error)) return false;
    WeightedScoresArgs a{};
    a.loss = loss; a.ld = ld; a.scale = scale; a.weight = weight; a.col_status = col_status; a.ranges = ranges; a.n_cols = (int)n_cols;
    a.n_loss = (int)n_loss; a.n_ranges = (int)n_ranges; a.transform = transform; a.scaled = out_scaled; a.score = out_score;
    a.weight_sum = out_weight_sum; a.left = out_left; a.total = out_total;
    try {
        (void)hipGetLastError();
        launch_weighted_scores(a, (hipStream_t)stream);
        LAUNCHCHECK("weighted scores");
    } catch (const HipFail &f) {
        report_hip_failure(out_error, f);
        return false;
    }
    return true;
}

bool anofox_hip_wrmsse_batch(const double *const *values, const size_t *lengths, const double *const *prices, size_t n_series,
                             const double *forecast, const double *actual, size_t horizon, const int32_t *column_of, size_t n_groupings,
                             size_t lag, bool trim_leading_zeros, size_t tail_rows, size_t ld, double *out_scale, double *out_rmsse,
                             int32_t *out_status, double *out_score, int32_t *out_left, int32_t *out_ranges, double *out_total,
                             size_t *out_n_out, size_t *out_ld, AnofoxError *out_error)
{
    clear_error(out_error);
    std::string message;
    if (n_series > 0 && (!values || !lengths || !forecast || !actual)) { set_error(out_error, NULL_POINTER, "Null pointer argument"); return false; }
    if (horizon < 1) { set_error(out_error, INVALID_INPUT, "Invalid input: horizon must be at least 1"); return false; }
    if (horizon > SCALED_PLAN_MAX_ROWS) {
        set_error(out_error, INVALID_INPUT, "Invalid input: horizon " + std::to_string(horizon) + " exceeds the limit of 2^30 rows");
        return false;
    }
    if (!paths_plan_report(scale_check(SIZE_MAX, n_series, 0, lag, tail_rows, SIZE_MAX, &message), message, out_error)) return false;
    size_t T = 1;
    for (size_t s = 0; s < n_series; s++) {
        if (lengths[s] > 0 && !values[s]) { set_error(out_error, NULL_POINTER, "Null pointer argument"); return false; }
        if (lengths[s] > SCALED_PLAN_MAX_ROWS) {
            set_error(out_error, INVALID_INPUT, "Invalid input: series " + std::to_string(s) + " is longer than the limit of 2^30 rows");
            return false;
        }
        T = std::max(T, lengths[s]);
    }
    const bool planned = column_of != nullptr && n_groupings > 0;
    size_t n_out = n_series, nnz = 0;
    std::vector<int32_t> offs, memb;
    if (planned) {
        if (!anofox_hip_hierarchy_plan(column_of, n_groupings, n_series, &n_out, &nnz, nullptr, nullptr, out_error)) return false;
        offs.resize(n_out + 1);
        memb.resize(std::max<size_t>(nnz, 1));
        if (!anofox_hip_hierarchy_plan(column_of, n_groupings, n_series, &n_out, &nnz, offs.data(), memb.data(), out_error)) return false;
    }
    const size_t need_ld = paths_ld(n_out);
    if (out_n_out) *out_n_out = n_out;
    if (out_ld) *out_ld = need_ld;
    if (!out_status) return true;
    if (ld != need_ld) { set_error(out_error, INVALID_INPUT, "Invalid input: ld is not what the sizing call returns"); return false; }
    const size_t R = wrmsse_n_ranges(planned, n_groupings);
    const double nan = std::numeric_limits<double>::quiet_NaN();
    std::vector<int32_t> ranges(2 * R);
    wrmsse_ranges(planned ? column_of : nullptr, n_groupings, n_series, n_out, ranges.data());
    if (out_ranges) std::memcpy(out_ranges, ranges.data(), 2 * R * sizeof(int32_t));
    if (out_total) *out_total = nan;
    for (size_t r = 0; r < R; r++) {
        if (out_score) out_score[r] = nan;
        if (out_left) out_left[r] = -1;
    }
    if (n_series == 0 || n_out == 0) return true;
    if (!device_ready(out_error)) return false;

    const size_t ld_s = paths_ld(n_series);
    // ONE arena of results, so that one copy brings them back: scale [4 x ld], rmsse [ld], score [R], total [2], then status [ld], left [R]
    const size_t back_doubles = 5 * need_ld + R + 2, back_bytes = back_doubles * 8 + (need_ld + R) * 4;
    std::vector<uint8_t> back(back_bytes);
    Scratch scratch;
    bool ok = true;
    try {
        std::vector<double> yb(T * ld_s, 0.0), rb(prices ? T * ld_s : 0, 0.0), fb(horizon * ld_s, 0.0), ab(horizon * ld_s, 0.0);
        const std::vector<int32_t> len = block_lengths(lengths, n_series, ld_s);
        std::vector<int32_t> steps(ld_s, 0);
        std::vector<int64_t> fst(ld_s, 0);                                     // the series end on the same date
        pack_time_major(yb.data(), ld_s, values, lengths, n_series);
        for (size_t s = 0; s < n_series; s++) {
            steps[s] = (int32_t)horizon;
            fst[s] = (int64_t)(T - std::max<size_t>(lengths[s], lengths[s] ? 0 : T));
            for (size_t k = 0; k < horizon; k++) { fb[k * ld_s + s] = forecast[s * horizon + k]; ab[k * ld_s + s] = actual[s * horizon + k]; }
            if (prices)
                for (size_t t = 0; t < lengths[s]; t++) rb[t * ld_s + s] = prices[s] ? values[s][t] * prices[s][t] : values[s][t];
        }
        const size_t n_blocks = planned ? (prices ? 2 : 1) : 0;
        double *d_y = nullptr, *d_rev = nullptr, *d_agg = nullptr;
        try {
            d_y = scratch.get<double>(T * ld_s);
            if (prices) d_rev = scratch.get<double>(T * ld_s);
            if (n_blocks) d_agg = scratch.get<double>(n_blocks * T * need_ld);
        } catch (const HipFail &f) {
            if (!f.oom) throw;
            set_error(out_error, COMPUTATION_ERROR, "Computation error: the training block" + std::string(prices ? "s" : "") + " of " + std::to_string(T) +
                      " x " + std::to_string(ld_s) + " values" + (planned ? " and the aggregate of " + std::to_string(T) + " x " +
                      std::to_string(need_ld) + " values" : std::string()) + " need " +
                      std::to_string(((prices ? 2 : 1) * T * ld_s + n_blocks * T * need_ld) * sizeof(double)) + " bytes of device memory");
            ok = false;
        }
        if (ok) {
            double *d_f = scratch.get<double>(horizon * ld_s), *d_a = scratch.get<double>(horizon * ld_s);
            int32_t *d_len = scratch.get<int32_t>(ld_s), *d_steps = scratch.get<int32_t>(ld_s);
            double *d_fig = scratch.get<double>(12 * need_ld);
            int32_t *d_mstatus = scratch.get<int32_t>(need_ld), *d_first = scratch.get<int32_t>(need_ld), *d_ranges = scratch.get<int32_t>(2 * R);
            double *d_wsum = scratch.get<double>(R);
            uint8_t *d_back = scratch.get<uint8_t>(back_bytes);
            double *d_scale = (double *)d_back, *d_rmsse = d_scale + 4 * need_ld, *d_score = d_rmsse + need_ld, *d_total = d_score + R;
            int32_t *d_status = (int32_t *)(d_back + back_doubles * 8), *d_left = d_status + need_ld;
            HIPCHECK(hipMemcpy(d_y, yb.data(), T * ld_s * sizeof(double), hipMemcpyHostToDevice));
            if (prices) HIPCHECK(hipMemcpy(d_rev, rb.data(), T * ld_s * sizeof(double), hipMemcpyHostToDevice));
            HIPCHECK(hipMemcpy(d_f, fb.data(), horizon * ld_s * sizeof(double), hipMemcpyHostToDevice));
            HIPCHECK(hipMemcpy(d_a, ab.data(), horizon * ld_s * sizeof(double), hipMemcpyHostToDevice));
            HIPCHECK(hipMemcpy(d_len, len.data(), ld_s * sizeof(int32_t), hipMemcpyHostToDevice));
            HIPCHECK(hipMemcpy(d_steps, steps.data(), ld_s * sizeof(int32_t), hipMemcpyHostToDevice));
            HIPCHECK(hipMemcpy(d_ranges, ranges.data(), 2 * R * sizeof(int32_t), hipMemcpyHostToDevice));
            HIPCHECK(hipMemset(d_back, 0xFF, back_doubles * 8));               // NaN in every figure of the padding columns
            HIPCHECK(hipMemset(d_back + back_doubles * 8, 0, (need_ld + R) * 4));
            const double *d_train = d_y, *d_weight = d_rev, *d_fc = d_f, *d_act = d_a;
            const int32_t *d_tlen = d_len, *d_hlen = d_steps;
            if (planned) {
                AnofoxHipHierarchyOptions ho{};
                int32_t *d_plan = scratch.get<int32_t>(n_out + 1 + nnz);
                int64_t *d_fst = scratch.get<int64_t>(ld_s), *d_first_out = scratch.get<int64_t>(need_ld);
                int32_t *d_len_agg = scratch.get<int32_t>(need_ld), *d_len_rev = scratch.get<int32_t>(need_ld), *d_len_h = scratch.get<int32_t>(need_ld);
                double *d_fa = scratch.get<double>(2 * horizon * need_ld);
                HIPCHECK(hipMemcpy(d_plan, offs.data(), (n_out + 1) * sizeof(int32_t), hipMemcpyHostToDevice));
                if (nnz) HIPCHECK(hipMemcpy(d_plan + n_out + 1, memb.data(), nnz * sizeof(int32_t), hipMemcpyHostToDevice));
                HIPCHECK(hipMemcpy(d_fst, fst.data(), ld_s * sizeof(int64_t), hipMemcpyHostToDevice));
                HIPCHECK(hipMemset(d_agg, 0, n_blocks * T * need_ld * sizeof(double)));
                HIPCHECK(hipMemset(d_fa, 0, 2 * horizon * need_ld * sizeof(double)));
                HIPCHECK(hipMemset(d_len_agg, 0, need_ld * sizeof(int32_t)));
                HIPCHECK(hipMemset(d_len_h, 0, need_ld * sizeof(int32_t)));
                const int32_t *d_memb = d_plan + n_out + 1;
                ok = anofox_hip_hierarchy_device(d_y, nullptr, nullptr, ld_s, d_len, d_fst, n_series, T, d_plan, d_memb, n_out, nnz, &ho, sizeof ho, T,
                                                 d_agg, nullptr, need_ld, d_len_agg, d_first_out, nullptr, out_error);
                if (ok && prices)
                    ok = anofox_hip_hierarchy_device(d_rev, nullptr, nullptr, ld_s, d_len, d_fst, n_series, T, d_plan, d_memb, n_out, nnz, &ho, sizeof ho,
                                                     T, d_agg + T * need_ld, nullptr, need_ld, d_len_rev, d_first_out, nullptr, out_error);
                if (ok)
                    ok = anofox_hip_hierarchy_device(d_f, nullptr, nullptr, ld_s, d_steps, nullptr, n_series, horizon, d_plan, d_memb, n_out, nnz, &ho,
                                                     sizeof ho, horizon, d_fa, nullptr, need_ld, d_len_h, d_first_out, nullptr, out_error);
                if (ok)
                    ok = anofox_hip_hierarchy_device(d_a, nullptr, nullptr, ld_s, d_steps, nullptr, n_series, horizon, d_plan, d_memb, n_out, nnz, &ho,
                                                     sizeof ho, horizon, d_fa + horizon * need_ld, nullptr, need_ld, d_len_h, d_first_out, nullptr,
                                                     out_error);
                d_train = d_agg; d_weight = prices ? d_agg + T * need_ld : nullptr; d_fc = d_fa; d_act = d_fa + horizon * need_ld;
                d_tlen = d_len_agg; d_hlen = d_len_h;
            }
            const size_t ld_b = planned ? need_ld : ld_s;                       // (the same number without a plan)
            if (ok)
                ok = anofox_hip_metrics_device(d_act, d_fc, nullptr, nullptr, nullptr, nullptr, 0, nullptr, 0, 1, ld_b, d_hlen, n_out, horizon,
                                               1u << MF_MSE, 0.5, true, d_fig, need_ld, d_mstatus, nullptr, out_error);
            if (ok)
                ok = anofox_hip_scale_device(d_train, ld_b, d_tlen, n_out, T, d_weight, lag, trim_leading_zeros, tail_rows, d_scale, need_ld, d_first,
                                             d_status, nullptr, out_error);
            if (ok)
                ok = anofox_hip_weighted_scores_device(d_fig + (size_t)MF_MSE * need_ld, need_ld, n_out, 1, d_scale, d_scale + 3 * need_ld, d_status,
                                                       d_ranges, R, 1, d_rmsse, d_score, d_wsum, d_left, d_total, nullptr, out_error);
            if (ok) HIPCHECK(hipMemcpy(back.data(), d_back, back_bytes, hipMemcpyDeviceToHost));          // waits for the null stream
            else HIPCHECK(hipDeviceSynchronize());
        }
        scratch.settled();                                                 // (either way the device has been waited for)
    } catch (const HipFail &f) {
        report_hip_failure(out_error, f);
        return false;
    }
    if (!ok) return false;
    const double *b_scale = (const double *)back.data(), *b_rmsse = b_scale + 4 * need_ld, *b_score = b_rmsse + need_ld, *b_total = b_score + R;
    const int32_t *b_status = (const int32_t *)(back.data() + back_doubles * 8), *b_left = b_status + need_ld;
    if (out_scale) std::memcpy(out_scale, b_scale, 4 * need_ld * sizeof(double));
    if (out_rmsse) std::memcpy(out_rmsse, b_rmsse, need_ld * sizeof(double));
    std::memcpy(out_status, b_status, n_out * sizeof(int32_t));
    if (out_score) std::memcpy(out_score, b_score, R * sizeof(double));
    if (out_left) std::memcpy(out_left, b_left, R * sizeof(int32_t));
    if (out_total) *out_total = b_total[1];
    return true;
}

} // extern "C"
