// host_ets_paths_plan.hpp -- the host-only checks of the model-path entries (DESIGN.md section 3 "Model paths"), each with a text that
// names its limit; they come before the device is touched.  Plain C++ without HIP, on top of host_paths_plan.hpp (the limits of
// n_paths, horizon, the block and the pool are those of the bootstrap entries): host_api.hip includes it inside its anonymous
// namespace.
#pragma once

constexpr size_t ETS_PATHS_PLAN_MAX_PERIOD = 2048;                  // (= ETS_PATHS_MAX_PERIOD of kernels.hpp and ANOFOX_HIP_ETS_PATHS_MAX_PERIOD)
constexpr size_t ETS_PATHS_PLAN_MAX_RING = 128;                     // (= ETS_PATHS_MAX_RING and ANOFOX_HIP_ETS_PATHS_MAX_RING)

// the options block, field by field (the struct itself belongs to the C header)
inline PathsPlanResult ets_paths_options_check(bool have_options, size_t struct_size, size_t expected_size, int innovations, int joint,
                                               std::string *message)
{
    auto invalid = [&](const std::string &text) { *message = "Invalid input: " + text; return PATHS_PLAN_INVALID; };
    if (!have_options) return PATHS_PLAN_NULL;
    if (struct_size != expected_size) return invalid("struct_size is not sizeof(AnofoxHipEtsPathsOptions)");
    if (innovations < 0 || innovations > 1)
        return invalid("innovations " + std::to_string(innovations) + " is unknown: 0 (Gaussian) or 1 (bootstrap)");
    if (joint < 0 || joint > 1) return invalid("joint " + std::to_string(joint) + " is neither 0 nor 1");
    if (joint == 1 && innovations == 0)
        return invalid("joint = 1 needs the bootstrap: there is no joint Gaussian mode (innovations 0 draws every series on its own)");
    return PATHS_PLAN_OK;
}

// the seasonal period and the phases a path touches, R = min(m, horizon)
inline PathsPlanResult ets_paths_period_check(size_t m, size_t horizon, std::string *message)
{
    auto invalid = [&](const std::string &text) { *message = "Invalid input: " + text; return PATHS_PLAN_INVALID; };
    if (m < 1) return invalid("the seasonal period m is 0, it must be at least 1");
    if (m > ETS_PATHS_PLAN_MAX_PERIOD)
        return invalid("the seasonal period m = " + std::to_string(m) + " exceeds the limit of " + std::to_string(ETS_PATHS_PLAN_MAX_PERIOD));
    const size_t ring = m < horizon ? m : horizon;
    if (ring > ETS_PATHS_PLAN_MAX_RING)
        return invalid("R = min(m, horizon) = " + std::to_string(ring) + " exceeds the limit of " + std::to_string(ETS_PATHS_PLAN_MAX_RING) +
                       " seasonal states per path");
    return PATHS_PLAN_OK;
}

inline PathsPlanResult ets_paths_pool_check(int innovations, bool have_pool, size_t pool_rows, std::string *message)
{
    if (innovations != 1) return PATHS_PLAN_OK;
    if (!have_pool) {
        *message = "Invalid input: the bootstrap needs a pool of innovations (pool is NULL)";
        return PATHS_PLAN_INVALID;
    }
    return paths_pool_check(pool_rows, message);
}
