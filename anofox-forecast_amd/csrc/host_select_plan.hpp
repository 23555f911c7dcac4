// host_select_plan.hpp -- the host-only logic of the selection entries (DESIGN.md section 3 "Selection"): the checks of the method
// table, the names of the criterion and of the mode, and the shapes of the winners' sub-batches from the partition's offsets.  Plain
// C++ without HIP: host_api.hip includes it inside its anonymous namespace, and tests/c_abi/select_san.cpp compiles THIS file on its
// own and runs it under ASan + UBSan.
#pragma once

enum SelectPlanResult { SELECT_PLAN_OK = 0, SELECT_PLAN_NULL = 1, SELECT_PLAN_INVALID = 2 };

constexpr size_t SELECT_PLAN_MAX_METHODS = 16;         // (= SELECT_MAX_METHODS of kernels.hpp and ANOFOX_HIP_SELECT_MAX_METHODS of the header)

// the criterion -> its row of anofox_hip_metrics_device's figures; -1 for every other name (mase and rmae need a baseline block)
inline int select_criterion_figure(const char *name)
{
    static const char *const names[5] = {"mae", "mse", "rmse", "mape", "smape"};
    if (!name) return -1;
    for (int k = 0; k < 5; k++)
        if (std::strcmp(name, names[k]) == 0) return k;
    return -1;
}

// "pick" 0, "mean" 1, "median" 2, "inverse_score" 3; -1 for every other name
inline int select_mode_code(const char *name)
{
    static const char *const names[4] = {"pick", "mean", "median", "inverse_score"};
    if (!name) return -1;
    for (int k = 0; k < 4; k++)
        if (std::strcmp(name, names[k]) == 0) return k;
    return -1;
}

// the number of methods and the fallback, as every selection entry checks them
inline SelectPlanResult select_counts_check(size_t n_methods, int64_t fallback, std::string *message)
{
    auto invalid = [&](const std::string &text) { *message = "Invalid input: " + text; return SELECT_PLAN_INVALID; };
    if (n_methods < 1) return invalid("n_methods is 0, a selection needs at least 1 method");
    if (n_methods > SELECT_PLAN_MAX_METHODS)
        return invalid("n_methods " + std::to_string(n_methods) + " exceeds the limit of " + std::to_string(SELECT_PLAN_MAX_METHODS) + " methods");
    if (fallback < -1 || fallback >= (int64_t)n_methods)
        return invalid("fallback " + std::to_string(fallback) + " is outside [-1, " + std::to_string(n_methods) + ")");
    return SELECT_PLAN_OK;
}

// the request of anofox_hip_select_batch: horizons[m] is the horizon of method m's option block.  *figure and *mode are written on
// success; `message` names what SELECT_PLAN_INVALID found.
inline SelectPlanResult select_request_check(size_t n_methods, const int *horizons, const char *criterion, const char *mode_name, int64_t fallback,
                                             int *figure, int *mode, std::string *message)
{
    auto invalid = [&](const std::string &text) { *message = "Invalid input: " + text; return SELECT_PLAN_INVALID; };
    const SelectPlanResult r = select_counts_check(n_methods, fallback, message);
    if (r != SELECT_PLAN_OK) return r;
    if (!horizons || !criterion || !mode_name || !figure || !mode) return SELECT_PLAN_NULL;
    if (horizons[0] < 1) return invalid("horizon must be at least 1, method 0 has " + std::to_string(horizons[0]));
    for (size_t m = 1; m < n_methods; m++)
        if (horizons[m] != horizons[0])
            return invalid("all methods share one horizon, method " + std::to_string(m) + " has " + std::to_string(horizons[m]) + " and method 0 has " +
                           std::to_string(horizons[0]));
    const int fig = select_criterion_figure(criterion);
    if (fig < 0) return invalid(std::string("unknown criterion '") + criterion + "' (one of mae, mse, rmse, mape, smape)");
    const int mc = select_mode_code(mode_name);
    if (mc < 0) return invalid(std::string("unknown mode '") + mode_name + "' (one of pick, mean, median, inverse_score)");
    *figure = fig;
    *mode = mc;
    return SELECT_PLAN_OK;
}

struct SelectSubBatch { int method; size_t off, n_m, ld_m; };         // members[off .. off + n_m) run as one batch of ld_m columns

// the sub-batches of the methods that won something, in method order, from the partition's offsets [n_methods + 1]
inline SelectPlanResult select_sub_batches(const int32_t *offsets, size_t n_methods, size_t n_series, std::vector<SelectSubBatch> *out,
                                           std::string *message)
{
    auto invalid = [&](const std::string &text) { *message = "Invalid input: " + text; return SELECT_PLAN_INVALID; };
    if (!offsets || !out) return SELECT_PLAN_NULL;
    out->clear();
    if (n_methods < 1 || n_methods > SELECT_PLAN_MAX_METHODS) return invalid("n_methods is outside [1, " + std::to_string(SELECT_PLAN_MAX_METHODS) + "]");
    if (offsets[0] != 0) return invalid("offsets does not start at 0");
    for (size_t m = 0; m < n_methods; m++)
        if (offsets[m + 1] < offsets[m]) return invalid("offsets descends at method " + std::to_string(m));
    if ((size_t)offsets[n_methods] > n_series)
        return invalid("offsets ends at " + std::to_string(offsets[n_methods]) + ", beyond the " + std::to_string(n_series) + " series");
    for (size_t m = 0; m < n_methods; m++) {
        const size_t n_m = (size_t)(offsets[m + 1] - offsets[m]);
        if (n_m == 0) continue;
        out->push_back(SelectSubBatch{(int)m, (size_t)offsets[m], n_m, (n_m + 63) / 64 * 64});
    }
    return SELECT_PLAN_OK;
}
