// host_path_scores_plan.hpp -- the host-only logic of the path-score entries (DESIGN.md section 3 "Path scores"): the argument checks
// that come before the device is touched, each with a text that names its limit, the workspace size and the column ranges of a plan's
// groupings.  Plain C++ without HIP, on top of host_paths_plan.hpp: host_api.hip includes it inside its anonymous namespace, and
// tests/c_abi/path_scores_san.cpp compiles THIS file on its own and runs it under ASan + UBSan.
#pragma once

// the levels of the scores entry: none is allowed, otherwise the checks of the quantile entry
inline PathsPlanResult path_scores_levels_check(const double *levels, size_t n_levels, std::string *message)
{
    if (n_levels == 0) return PATHS_PLAN_OK;
    return paths_levels_check(levels, n_levels, message);
}

// the column range [col_begin, col_end) of the energy score inside a block of ld columns
inline PathsPlanResult path_energy_range_check(size_t ld, size_t col_begin, size_t col_end, std::string *message)
{
    auto invalid = [&](const std::string &text) { *message = "Invalid input: " + text; return PATHS_PLAN_INVALID; };
    const std::string range = "the column range [" + std::to_string(col_begin) + ", " + std::to_string(col_end) + ")";
    if (col_end <= col_begin) return invalid(range + " is empty or reversed");
    if (col_end > ld) return invalid(range + " ends beyond ld = " + std::to_string(ld));
    if (col_end > (size_t)INT32_MAX) return invalid(range + " exceeds the limit of 2^31 - 1 columns");
    return PATHS_PLAN_OK;
}

// doubles of the energy entry's workspace: D1 and D2, [n_paths x horizon] each (the rows check comes first: no overflow)
inline size_t path_energy_workspace(size_t horizon, size_t n_paths) { return 2 * horizon * n_paths; }

// The column ranges the batch entry takes the energy score of: one per grouping -- [its smallest column, its largest + 1); {0, 0} for
// a grouping that maps no series -- and the whole [0, n_out) last.  column_of NULL (no plan): the whole alone.  ranges: 2 * (n_groupings + 1)
inline void path_scores_ranges(const int32_t *column_of, size_t n_groupings, size_t n_series, size_t n_out, size_t *ranges)
{
    const size_t groupings = column_of ? n_groupings : 0;
    for (size_t g = 0; g < groupings; g++) {
        size_t lo = SIZE_MAX, hi = 0;
        for (size_t s = 0; s < n_series; s++) {
            const int32_t c = column_of[g * n_series + s];
            if (c < 0) continue;
            lo = (size_t)c < lo ? (size_t)c : lo;
            hi = (size_t)c + 1 > hi ? (size_t)c + 1 : hi;
        }
        ranges[2 * g] = hi ? lo : 0;
        ranges[2 * g + 1] = hi;
    }
    ranges[2 * groupings] = 0;
    ranges[2 * groupings + 1] = n_out;
}
