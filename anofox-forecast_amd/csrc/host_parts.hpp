// host_parts.hpp -- how the batch entry cuts an auto-detected batch (params := MAP{}: every series has its own detected period) into
// device batches, and how the results of a device batch go back to the caller's arrays.  Integer logic and result bookkeeping only:
// no HIP call, no kernel header.  Included by host_api.hip INSIDE its anonymous namespace; the two ring-class limits of the
// kernels (ets_device.hpp) come in as PartLimits, so tests/c_abi/parts_san.cpp compiles THIS file with a plain g++ and checks
// every decision against a brute-force restatement under ASan + UBSan.
//
// The plan: series with one used period form a Part.  Small parts of the same ring class merge into ONE device batch whose
// columns are grouped by period in blocks of 64 (the kernels read the period per block): hundreds of tiny latency-bound batches
// were the whole duration of such a call.  What is not merged runs as ordinary batches that name their period: the big parts
// (they fill the chip on their own) a few side by side, the small ones on workers that each keep one device batch.
#pragma once

struct Part {
    int period = 1;                 // the period the model uses for these series (1: none)
    std::vector<size_t> series;     // indices into the caller's arrays
};

enum class MergeRule {
    None,           // every part is a batch of its own (ANOFOX_HIP_TUNE merge_periods=0, or a model without a merged kernel)
    EtsLike,        // periods from 2 up: the LDS-ring class and the HBM-ring class
    AutoArima       // periods above ARIMA_MERGE_ABOVE only: the ones below keep their compile-time / LDS-ring kernels, one batch each
};

struct PartLimits {
    int lds_period;     // the largest period of a merged batch whose seasonal ring lives in LDS (ETS_MERGED_LDS_PERIOD)
    int max_period;     // the largest period the kernels take at all (ETS_MAX_PERIOD)
};

constexpr int ARIMA_MERGE_ABOVE = 24;
constexpr size_t BIG_PART_SERIES = 2048;            // from here a part fills the chip on its own: never merged, run beside the workers
constexpr size_t PART_PAD_COLUMNS = 64;             // a part of a merged batch is whole 64-column blocks
constexpr double RING_SCRATCH_LIMIT = 2.0 * 1073741824.0;      // bytes per seasonal spec
constexpr size_t PAD_COLUMN = SIZE_MAX;             // the source index of a column that belongs to no series

using MergedBatch = std::vector<Part>;              // ascending period, at least two parts

struct PartPlan {
    // one host thread per group, its batches one after the other: every LDS-ring batch is a group of its own, all HBM-ring
    // batches form ONE group (they share the ring scratch)
    std::vector<std::vector<MergedBatch>> merged_groups;
    std::vector<Part> big, small;                   // what stays separate: at least / fewer than BIG_PART_SERIES series, largest first
};

// one part per distinct period, ascending
inline std::vector<Part> parts_by_period(const std::vector<int> &period)
{
    std::map<int, std::vector<size_t>> groups;
    for (size_t s = 0; s < period.size(); s++) groups[period[s]].push_back(s);
    std::vector<Part> parts;
    parts.reserve(groups.size());
    for (auto &g : groups) parts.push_back(Part{g.first, std::move(g.second)});
    return parts;
}

// The ring class a part merges into: 0 (ring in LDS), 1 (ring in an HBM scratch, sized by the class's largest period), -1 none.
// (The LDS ring of a round kernel is sized by the batch's largest period, for every wave: periods up to 64 in one batch left
//  three waves per CU -- a tenth of the uniform batch's rate per series -- so a merged batch keeps periods above lds_period in
//  the HBM ring, which streams like y; more, finer classes only multiply the streams that share the hardware queues.)
inline int ring_class(const Part &part, MergeRule rule, PartLimits lim)
{
    if (rule == MergeRule::None || part.series.size() >= BIG_PART_SERIES || part.period > lim.max_period) return -1;
    if (rule == MergeRule::AutoArima) return part.period > ARIMA_MERGE_ABOVE ? 1 : -1;
    if (part.period < 2) return -1;
    return part.period <= lim.lds_period ? 0 : 1;
}

// The ring scratch of an HBM-ring batch, per seasonal spec: workgroups of the widest launch x largest period x 512 B.  The widest
// launch is the speculative driver's 16 problems per workgroup, or one wave per problem for the last 2,048.
inline double ring_scratch_bytes(size_t cols, int m_hi)
{
    return (double)std::max<size_t>((cols + 15) / 16, std::min<size_t>(cols, 2048)) * (double)m_hi * 512.0;
}

inline size_t padded_columns(const Part &part) { return (part.series.size() + PART_PAD_COLUMNS - 1) / PART_PAD_COLUMNS * PART_PAD_COLUMNS; }

inline PartPlan plan_parts(std::vector<Part> parts, MergeRule rule, PartLimits lim)
{
    PartPlan plan;
    std::vector<Part> keep, cls[2];
    for (Part &part : parts) {
        const int c = ring_class(part, rule, lim);
        (c >= 0 ? cls[c] : keep).push_back(std::move(part));
    }
    // The HBM-ring class is cut where its ring scratch would pass the limit: many rare long periods otherwise ask for tens of GB
    // (100 GB for 8,192 series failed a whole call).  A batch left with one part has nothing to merge: the part stays separate.
    std::vector<MergedBatch> hbm;
    for (int c = 0; c < 2; c++) {
        std::sort(cls[c].begin(), cls[c].end(), [](const Part &x, const Part &y) { return x.period < y.period; });
        std::vector<MergedBatch> cut;
        MergedBatch cur;
        size_t cols = 0;
        for (Part &part : cls[c]) {
            const size_t pc = padded_columns(part);
            if (c == 1 && !cur.empty() && ring_scratch_bytes(cols + pc, part.period) > RING_SCRATCH_LIMIT) {
                cut.push_back(std::move(cur));
                cur.clear();
                cols = 0;
            }
            cols += pc;
            cur.push_back(std::move(part));
        }
        if (!cur.empty()) cut.push_back(std::move(cur));
        for (MergedBatch &batch : cut) {
            if (batch.size() < 2) keep.push_back(std::move(batch.front()));
            else if (c == 0) plan.merged_groups.push_back(std::vector<MergedBatch>{std::move(batch)});
            else hbm.push_back(std::move(batch));
        }
    }
    if (!hbm.empty()) plan.merged_groups.push_back(std::move(hbm));
    std::sort(keep.begin(), keep.end(), [](const Part &x, const Part &y) { return x.series.size() > y.series.size(); });
    for (Part &part : keep) (part.series.size() >= BIG_PART_SERIES ? plan.big : plan.small).push_back(std::move(part));
    return plan;
}

// The columns of one merged batch: the parts in order, each padded to whole 64-column blocks.  Per column the caller's series
// index (PAD_COLUMN for padding) and the period; m_max is the largest period.
struct MergedColumns { std::vector<size_t> src; std::vector<int32_t> period; int m_max = 0; };

inline MergedColumns merged_columns(const MergedBatch &batch)
{
    MergedColumns c;
    for (const Part &part : batch) {
        c.src.insert(c.src.end(), part.series.begin(), part.series.end());
        c.src.resize(c.src.size() + (padded_columns(part) - part.series.size()), PAD_COLUMN);
        c.period.resize(c.src.size(), (int32_t)part.period);
        c.m_max = std::max(c.m_max, part.period);
    }
    return c;
}

// ---- the results of a device batch -> the caller's arrays ----

inline void free_result_arrays(ForecastResult &r)
{
    std::free(r.point_forecasts); r.point_forecasts = nullptr;
    std::free(r.lower_bounds); r.lower_bounds = nullptr;
    std::free(r.upper_bounds); r.upper_bounds = nullptr;
    std::free(r.fitted_values); r.fitted_values = nullptr;
    std::free(r.residuals); r.residuals = nullptr;
}

inline void free_results(ForecastResult *res, size_t n) { for (size_t j = 0; j < n; j++) free_result_arrays(res[j]); }

// A batch runs with the largest horizon of its series; forecasts are prefix-consistent, so a series' own horizon is a prefix cut
// (ts_cv_forecast_native.cpp:676-677).  Horizon 0 leaves no arrays.
inline void truncate_to_horizon(ForecastResult &r, int horizon)
{
    if (!r.point_forecasts || horizon < 0 || (size_t)horizon >= r.n_forecasts) return;
    r.n_forecasts = (size_t)horizon;
    if (horizon == 0) {
        std::free(r.point_forecasts); std::free(r.lower_bounds); std::free(r.upper_bounds);
        r.point_forecasts = r.lower_bounds = r.upper_bounds = nullptr;
    }
}

// Column j of a fetched batch belongs to the caller's series src[j]: its result, cut to that series' own horizon (horizons may be
// NULL: `horizon` for all), and its error (out_errors may be NULL) move there.  A padding column is freed and written nowhere.
inline void deliver_results(ForecastResult *res, const AnofoxError *errs, const size_t *src, size_t n_cols, const int *horizons, int horizon,
                            ForecastResult *out_results, AnofoxError *out_errors)
{
    for (size_t j = 0; j < n_cols; j++) {
        if (src[j] == PAD_COLUMN) { free_result_arrays(res[j]); continue; }
        truncate_to_horizon(res[j], horizons ? horizons[src[j]] : horizon);
        out_results[src[j]] = res[j];
        if (out_errors) out_errors[src[j]] = errs[j];
    }
}
