// host_paths_plan.hpp -- the host-only logic of the sample-path entries (DESIGN.md section 3 "Sample paths"): the argument checks
// that come before the device is touched, each with a text that names its limit, and the output shape of the batch entry.  Plain
// C++ without HIP: host_api.hip includes it inside its anonymous namespace, and tests/c_abi/paths_san.cpp compiles THIS file on its
// own and runs it under ASan + UBSan.
#pragma once

enum PathsPlanResult { PATHS_PLAN_OK = 0, PATHS_PLAN_NULL = 1, PATHS_PLAN_INVALID = 2 };

constexpr size_t PATHS_PLAN_MAX_PATHS = 2048;                       // (= PATHS_MAX_PATHS of kernels.hpp and ANOFOX_HIP_PATHS_MAX_PATHS of the header)
constexpr size_t PATHS_PLAN_MAX_LEVELS = 16;                        // (= PATHS_MAX_LEVELS)
constexpr size_t PATHS_PLAN_MAX_POOL_ROWS = (size_t)1 << 20;        // (= PATHS_MAX_POOL_ROWS)
constexpr size_t PATHS_PLAN_MAX_ROWS = (size_t)1 << 30;             // (= PATHS_MAX_ROWS)

// "cumulative" 0, "independent" 1; -1 for every other name
inline int paths_mode_code(const char *name)
{
    static const char *const names[2] = {"cumulative", "independent"};
    if (!name) return -1;
    for (int k = 0; k < 2; k++)
        if (std::strcmp(name, names[k]) == 0) return k;
    return -1;
}

// the options block, field by field (the struct itself belongs to the C header)
inline PathsPlanResult paths_options_check(bool have_options, size_t struct_size, size_t expected_size, int mode, int joint, int route,
                                           std::string *message)
{
    auto invalid = [&](const std::string &text) { *message = "Invalid input: " + text; return PATHS_PLAN_INVALID; };
    if (!have_options) return PATHS_PLAN_NULL;
    if (struct_size != expected_size) return invalid("struct_size is not sizeof(AnofoxHipPathsOptions)");
    if (mode < 0 || mode > 1) return invalid("mode " + std::to_string(mode) + " is unknown: 0 (cumulative) or 1 (independent)");
    if (joint < 0 || joint > 1) return invalid("joint " + std::to_string(joint) + " is neither 0 nor 1");
    if (route < 0 || route > 1) return invalid("route " + std::to_string(route) + " is unknown: 0 (automatic) or 1 (lanes over series)");
    return PATHS_PLAN_OK;
}

// horizon and n_paths, as the generating and the quantile entries both check them
inline PathsPlanResult paths_rows_check(size_t horizon, size_t n_paths, std::string *message)
{
    auto invalid = [&](const std::string &text) { *message = "Invalid input: " + text; return PATHS_PLAN_INVALID; };
    if (n_paths < 1) return invalid("n_paths is 0, a call needs at least 1 path");
    if (n_paths > PATHS_PLAN_MAX_PATHS)
        return invalid("n_paths " + std::to_string(n_paths) + " exceeds the limit of " + std::to_string(PATHS_PLAN_MAX_PATHS) + " paths per call");
    if (horizon < 1) return invalid("horizon must be at least 1");
    if (horizon > PATHS_PLAN_MAX_ROWS / n_paths)
        return invalid("n_paths * horizon = " + std::to_string(n_paths) + " * " + std::to_string(horizon) + " exceeds the limit of 2^30 rows");
    return PATHS_PLAN_OK;
}

// the block of columns: `columns` names n_cols in the message
inline PathsPlanResult paths_block_check(size_t ld, size_t n_cols, const char *ld_name, const char *columns, std::string *message)
{
    auto invalid = [&](const std::string &text) { *message = "Invalid input: " + text; return PATHS_PLAN_INVALID; };
    if (n_cols > (size_t)INT32_MAX) return invalid(std::string(columns) + " exceeds the limit of 2^31 - 1");
    if (ld < n_cols) return invalid(std::string(ld_name) + " is smaller than " + columns);
    return PATHS_PLAN_OK;
}

inline PathsPlanResult paths_pool_check(size_t pool_rows, std::string *message)
{
    if (pool_rows > PATHS_PLAN_MAX_POOL_ROWS) {
        *message = "Invalid input: pool_rows " + std::to_string(pool_rows) + " exceeds the limit of 2^20 = " + std::to_string(PATHS_PLAN_MAX_POOL_ROWS) +
                   " rows per pool";
        return PATHS_PLAN_INVALID;
    }
    return PATHS_PLAN_OK;
}

inline PathsPlanResult paths_levels_check(const double *levels, size_t n_levels, std::string *message)
{
    auto invalid = [&](const std::string &text) { *message = "Invalid input: " + text; return PATHS_PLAN_INVALID; };
    if (n_levels < 1) return invalid("n_levels is 0, a call needs at least 1 level");
    if (n_levels > PATHS_PLAN_MAX_LEVELS)
        return invalid("n_levels " + std::to_string(n_levels) + " exceeds the limit of " + std::to_string(PATHS_PLAN_MAX_LEVELS) + " levels per call");
    if (!levels) return PATHS_PLAN_NULL;
    for (size_t k = 0; k < n_levels; k++)
        if (!(levels[k] >= 0.0 && levels[k] <= 1.0)) {             // (a NaN fails both comparisons)
            char text[96];
            std::snprintf(text, sizeof text, "level %zu is %g, outside [0, 1]", k, levels[k]);
            return invalid(text);
        }
    return PATHS_PLAN_OK;
}

// the request of anofox_hip_paths_batch: the lengths of the pools -> pool_rows (the longest; 0 when every pool is empty)
inline PathsPlanResult paths_batch_pools(const size_t *pool_lengths, size_t n_series, size_t *pool_rows, std::string *message)
{
    if (n_series > 0 && !pool_lengths) return PATHS_PLAN_NULL;
    if (!pool_rows) return PATHS_PLAN_NULL;
    size_t longest = 0;
    for (size_t s = 0; s < n_series; s++) longest = pool_lengths[s] > longest ? pool_lengths[s] : longest;
    const PathsPlanResult r = paths_pool_check(longest, message);
    if (r != PATHS_PLAN_OK) return r;
    *pool_rows = longest;
    return PATHS_PLAN_OK;
}

// columns of a block rounded up to whole wavefronts, at least one
inline size_t paths_ld(size_t n_cols) { return n_cols == 0 ? 64 : (n_cols + 63) / 64 * 64; }
