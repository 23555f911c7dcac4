// host_scaled_scores_plan.hpp -- the host-only logic of the scaled-score entries (DESIGN.md section 3 "Scaled scores"): the argument
// checks that come before the device is touched, each with a text that names its limit, and the column ranges the batch entry
// scores.  Plain C++ without HIP, on top of host_paths_plan.hpp and host_path_scores_plan.hpp: host_api.hip includes it inside its
// anonymous namespace, and tests/c_abi/scaled_scores_san.cpp compiles THIS file on its own and runs it under ASan + UBSan.
#pragma once

constexpr size_t SCALED_PLAN_MAX_ROWS = (size_t)1 << 30;            // lag, tail_rows, t_rows: the row limit of the hierarchy entry
constexpr size_t SCALED_PLAN_MAX_LOSS = 16;                         // (= SCALED_MAX_LOSS of kernels.hpp: the project's level limit)

// lag, tail_rows, t_rows and the two blocks of anofox_hip_scale_device
inline PathsPlanResult scale_check(size_t ld, size_t n_cols, size_t t_rows, size_t lag, size_t tail_rows, size_t ld_out, std::string *message)
{
    auto invalid = [&](const std::string &text) { *message = "Invalid input: " + text; return PATHS_PLAN_INVALID; };
    if (lag < 1) return invalid("lag is 0, the smallest lag is 1");
    if (tail_rows < 1) return invalid("tail_rows is 0, the weight mass needs at least 1 row");
    if (lag > SCALED_PLAN_MAX_ROWS) return invalid("lag " + std::to_string(lag) + " exceeds the limit of 2^30 rows");
    if (tail_rows > SCALED_PLAN_MAX_ROWS) return invalid("tail_rows " + std::to_string(tail_rows) + " exceeds the limit of 2^30 rows");
    if (t_rows > SCALED_PLAN_MAX_ROWS) return invalid("t_rows " + std::to_string(t_rows) + " exceeds the limit of 2^30 rows");
    const PathsPlanResult r = paths_block_check(ld, n_cols, "ld", "n_cols", message);
    if (r != PATHS_PLAN_OK) return r;
    return paths_block_check(ld_out, n_cols, "ld_out", "n_cols", message);
}

// the shapes of anofox_hip_weighted_scores_device
inline PathsPlanResult weighted_scores_check(size_t ld, size_t n_cols, size_t n_loss, size_t n_ranges, int transform, std::string *message)
{
    auto invalid = [&](const std::string &text) { *message = "Invalid input: " + text; return PATHS_PLAN_INVALID; };
    if (n_loss < 1) return invalid("n_loss is 0, a call needs at least 1 loss row");
    if (n_loss > SCALED_PLAN_MAX_LOSS)
        return invalid("n_loss " + std::to_string(n_loss) + " exceeds the limit of " + std::to_string(SCALED_PLAN_MAX_LOSS) + " loss rows per call");
    if (transform < 0 || transform > 1)
        return invalid("transform " + std::to_string(transform) + " is unknown: 0 (loss / scale) or 1 (sqrt(loss / scale))");
    if (n_ranges < 1) return invalid("n_ranges is 0, a call needs at least 1 range");
    if (n_ranges > (size_t)INT32_MAX) return invalid("n_ranges exceeds the limit of 2^31 - 1");
    return paths_block_check(ld, n_cols, "ld", "n_cols", message);
}

// The column ranges anofox_hip_wrmsse_batch scores: one per grouping by the rule of path_scores_ranges -- [its smallest column, its
// largest + 1); {0, 0} for a grouping that maps no series --, without a plan the whole [0, n_out) alone.  ranges: 2 * wrmsse_n_ranges
inline size_t wrmsse_n_ranges(bool planned, size_t n_groupings) { return planned ? n_groupings : 1; }
inline void wrmsse_ranges(const int32_t *column_of, size_t n_groupings, size_t n_series, size_t n_out, int32_t *ranges)
{
    if (!column_of) { ranges[0] = 0; ranges[1] = (int32_t)n_out; return; }
    std::vector<size_t> all(2 * (n_groupings + 1));                  // (the rule's last range is the whole: not scored here)
    path_scores_ranges(column_of, n_groupings, n_series, n_out, all.data());
    for (size_t r = 0; r < 2 * n_groupings; r++) ranges[r] = (int32_t)all[r];
}
