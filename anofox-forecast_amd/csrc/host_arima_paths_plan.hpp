// host_arima_paths_plan.hpp -- the host-only checks of the ARIMA model-path entries (DESIGN.md section 3 "ARIMA paths"), each with a
// text that names its limit; they come before the device is touched.  Plain C++ without HIP, on top of host_paths_plan.hpp (the
// limits of n_paths, horizon, the block and the pool are those of the bootstrap entries): host_api.hip includes it inside its
// anonymous namespace.
#pragma once

constexpr size_t ARIMA_PATHS_PLAN_MAX_PERIOD = 2048;                // (= ARIMA_PATHS_MAX_PERIOD of kernels.hpp and ANOFOX_HIP_ARIMA_PATHS_MAX_PERIOD)
constexpr size_t ARIMA_PATHS_PLAN_MAX_LDS_ROWS = 128;               // (= ARIMA_PATHS_MAX_LDS_ROWS and ANOFOX_HIP_ARIMA_PATHS_MAX_LDS_ROWS)

// the options block, field by field (the struct itself belongs to the C header)
inline PathsPlanResult arima_paths_options_check(bool have_options, size_t struct_size, size_t expected_size, int innovations, int joint,
                                                 std::string *message)
{
    auto invalid = [&](const std::string &text) { *message = "Invalid input: " + text; return PATHS_PLAN_INVALID; };
    if (!have_options) return PATHS_PLAN_NULL;
    if (struct_size != expected_size) return invalid("struct_size is not sizeof(AnofoxHipArimaPathsOptions)");
    if (innovations < 0 || innovations > 1)
        return invalid("innovations " + std::to_string(innovations) + " is unknown: 0 (Gaussian) or 1 (bootstrap)");
    if (joint < 0 || joint > 1) return invalid("joint " + std::to_string(joint) + " is neither 0 nor 1");
    if (joint == 1 && innovations == 0)
        return invalid("joint = 1 needs the bootstrap: there is no joint Gaussian mode (innovations 0 draws every series on its own)");
    return PATHS_PLAN_OK;
}

inline PathsPlanResult arima_paths_period_check(size_t m, std::string *message)
{
    auto invalid = [&](const std::string &text) { *message = "Invalid input: " + text; return PATHS_PLAN_INVALID; };
    if (m < 1) return invalid("the seasonal period m is 0, it must be at least 1");
    if (m > ARIMA_PATHS_PLAN_MAX_PERIOD)
        return invalid("the seasonal period m = " + std::to_string(m) + " exceeds the limit of " + std::to_string(ARIMA_PATHS_PLAN_MAX_PERIOD));
    return PATHS_PLAN_OK;
}

// the LDS rows of a wavefront: the rings of simulated x and e, min(horizon, 2 m + 5) slots each, and the y ring of m slots when m < horizon
inline size_t arima_paths_rows(size_t m, size_t horizon)
{
    const size_t ring = horizon < 2 * m + 5 ? horizon : 2 * m + 5;
    return 2 * ring + (m < horizon ? m : 0);
}

// the period and the simulated values a path keeps
inline PathsPlanResult arima_paths_ring_check(size_t m, size_t horizon, std::string *message)
{
    const PathsPlanResult r = arima_paths_period_check(m, message);
    if (r != PATHS_PLAN_OK) return r;
    const size_t rows = arima_paths_rows(m, horizon);
    if (rows > ARIMA_PATHS_PLAN_MAX_LDS_ROWS) {
        *message = "Invalid input: 2 min(horizon, 2 m + 5) + (m < horizon ? m : 0) = " + std::to_string(rows) + " exceeds the limit of " +
                   std::to_string(ARIMA_PATHS_PLAN_MAX_LDS_ROWS) + " LDS rows per path (the ring limit)";
        return PATHS_PLAN_INVALID;
    }
    return PATHS_PLAN_OK;
}

// pool_rows is read in joint mode only
inline PathsPlanResult arima_paths_pool_check(int joint, size_t pool_rows, std::string *message)
{
    return joint == 1 ? paths_pool_check(pool_rows, message) : PATHS_PLAN_OK;
}

inline PathsPlanResult arima_paths_rows_limit_check(size_t t_rows, std::string *message)
{
    if (t_rows > (size_t)INT32_MAX) {
        *message = "Invalid input: t_rows exceeds the limit of 2^31 - 1";
        return PATHS_PLAN_INVALID;
    }
    return PATHS_PLAN_OK;
}
