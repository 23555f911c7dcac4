// select_san.cpp -- TEST INFRASTRUCTURE.  csrc/host_select_plan.hpp (the host-only logic of the selection entries) compiled on its
// own, without HIP, and run under ASan + UBSan:
//   * the criterion and mode names map to their codes, every other name (and NULL) to -1;
//   * the request check accepts 1 .. 16 methods of one horizon and refuses, naming the offender, M = 0, M = 17, mixed horizons, a
//     horizon below 1, an unknown criterion, an unknown mode, a fallback outside [-1, M), and NULL arrays;
//   * the sub-batches of seeded offsets equal a restatement written here (methods that won nothing are left out, ld_m is n_m rounded
//     up to 64, the ranges tile [0, offsets[M])), and offsets that descend, do not start at 0 or end beyond n_series are refused.
// The vectors handed in are sized exactly, so a read past an end is a report.  Built by tests/test_select_cpu.py with
// g++ -fsanitize=address,undefined; exit code 0 = all checks passed.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

namespace {
#include "../../anofox-forecast_amd/csrc/host_select_plan.hpp"
}

static int failures = 0;
#define CHECK(cond)                                                                       \
    do {                                                                                  \
        if (!(cond)) { std::fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); failures++; } \
    } while (0)

static bool has(const std::string &text, const char *part) { return text.find(part) != std::string::npos; }

static void names()
{
    const char *crit[5] = {"mae", "mse", "rmse", "mape", "smape"};
    for (int k = 0; k < 5; k++) CHECK(select_criterion_figure(crit[k]) == k);
    for (const char *bad : {"mase", "rmae", "r2", "bias", "coverage", "RMSE", "", "rmse "}) CHECK(select_criterion_figure(bad) == -1);
    CHECK(select_criterion_figure(nullptr) == -1);
    const char *mode[4] = {"pick", "mean", "median", "inverse_score"};
    for (int k = 0; k < 4; k++) CHECK(select_mode_code(mode[k]) == k);
    for (const char *bad : {"best", "Pick", "", "inverse"}) CHECK(select_mode_code(bad) == -1);
    CHECK(select_mode_code(nullptr) == -1);
}

static void requests()
{
    std::string msg;
    int fig = -7, mode = -7;
    for (size_t M = 1; M <= SELECT_PLAN_MAX_METHODS; M++) {
        std::vector<int> h(M, 3);                              // exactly M entries
        for (int64_t fb = -1; fb < (int64_t)M; fb++) {
            CHECK(select_request_check(M, h.data(), "smape", "median", fb, &fig, &mode, &msg) == SELECT_PLAN_OK);
            CHECK(fig == 4 && mode == 2);
        }
        CHECK(select_request_check(M, h.data(), "rmse", "pick", (int64_t)M, &fig, &mode, &msg) == SELECT_PLAN_INVALID);
        CHECK(has(msg, "fallback") && has(msg, ("[-1, " + std::to_string(M) + ")").c_str()));
        CHECK(select_request_check(M, h.data(), "rmse", "pick", -2, &fig, &mode, &msg) == SELECT_PLAN_INVALID && has(msg, "fallback -2"));
        if (M >= 2) {
            h[M - 1] = 4;
            CHECK(select_request_check(M, h.data(), "rmse", "pick", -1, &fig, &mode, &msg) == SELECT_PLAN_INVALID);
            CHECK(has(msg, "share one horizon") && has(msg, ("method " + std::to_string(M - 1) + " has 4").c_str()));
        }
    }
    std::vector<int> h17(17, 2), h1(1, 0);
    CHECK(select_request_check(0, h1.data(), "rmse", "pick", -1, &fig, &mode, &msg) == SELECT_PLAN_INVALID && has(msg, "n_methods is 0"));
    CHECK(select_request_check(17, h17.data(), "rmse", "pick", -1, &fig, &mode, &msg) == SELECT_PLAN_INVALID);
    CHECK(has(msg, "n_methods 17 exceeds the limit of 16 methods"));
    CHECK(select_counts_check(17, -1, &msg) == SELECT_PLAN_INVALID && has(msg, "limit of 16"));
    CHECK(select_request_check(1, h1.data(), "rmse", "pick", -1, &fig, &mode, &msg) == SELECT_PLAN_INVALID && has(msg, "horizon must be at least 1"));
    h1[0] = 5;
    CHECK(select_request_check(1, h1.data(), "mase", "pick", -1, &fig, &mode, &msg) == SELECT_PLAN_INVALID && has(msg, "unknown criterion 'mase'"));
    CHECK(select_request_check(1, h1.data(), "mae", "best", -1, &fig, &mode, &msg) == SELECT_PLAN_INVALID && has(msg, "unknown mode 'best'"));
    CHECK(select_request_check(1, nullptr, "mae", "pick", -1, &fig, &mode, &msg) == SELECT_PLAN_NULL);
    CHECK(select_request_check(1, h1.data(), nullptr, "pick", -1, &fig, &mode, &msg) == SELECT_PLAN_NULL);
    CHECK(select_request_check(1, h1.data(), "mae", nullptr, -1, &fig, &mode, &msg) == SELECT_PLAN_NULL);
    CHECK(select_request_check(1, h1.data(), "mae", "pick", -1, nullptr, &mode, &msg) == SELECT_PLAN_NULL);
}

static void sub_batches()
{
    std::mt19937 rng(20260);
    std::string msg;
    std::vector<SelectSubBatch> subs;
    for (int round = 0; round < 400; round++) {
        const size_t M = 1 + rng() % SELECT_PLAN_MAX_METHODS, n_series = rng() % 500;
        std::vector<int32_t> offs(M + 1, 0);                   // exactly M + 1 entries
        std::vector<size_t> cuts;
        for (size_t m = 0; m < M; m++) cuts.push_back(n_series ? rng() % (n_series + 1) : 0);
        if (round % 3 == 0) for (size_t m = 0; m + 1 < M; m += 2) cuts[m + 1] = cuts[m];      // methods that won nothing
        std::sort(cuts.begin(), cuts.end());
        for (size_t m = 0; m < M; m++) offs[m + 1] = (int32_t)cuts[m];
        CHECK(select_sub_batches(offs.data(), M, n_series, &subs, &msg) == SELECT_PLAN_OK);
        size_t k = 0, at = 0;
        for (size_t m = 0; m < M; m++) {
            const size_t n_m = (size_t)(offs[m + 1] - offs[m]);
            if (n_m == 0) continue;
            CHECK(k < subs.size());
            if (k >= subs.size()) break;
            CHECK(subs[k].method == (int)m && subs[k].off == at && subs[k].n_m == n_m);
            CHECK(subs[k].ld_m % 64 == 0 && subs[k].ld_m >= n_m && subs[k].ld_m < n_m + 64);
            at += n_m;
            k++;
        }
        CHECK(k == subs.size() && at == (size_t)offs[M]);
    }
    int32_t bad_start[3] = {1, 2, 3}, descends[4] = {0, 5, 4, 6}, beyond[3] = {0, 4, 11};
    CHECK(select_sub_batches(bad_start, 2, 10, &subs, &msg) == SELECT_PLAN_INVALID && has(msg, "does not start at 0") && subs.empty());
    CHECK(select_sub_batches(descends, 3, 10, &subs, &msg) == SELECT_PLAN_INVALID && has(msg, "descends at method 1") && subs.empty());
    CHECK(select_sub_batches(beyond, 2, 10, &subs, &msg) == SELECT_PLAN_INVALID && has(msg, "ends at 11") && subs.empty());
    CHECK(select_sub_batches(nullptr, 2, 10, &subs, &msg) == SELECT_PLAN_NULL);
    CHECK(select_sub_batches(beyond, 2, 10, nullptr, &msg) == SELECT_PLAN_NULL);
    CHECK(select_sub_batches(beyond, 0, 10, &subs, &msg) == SELECT_PLAN_INVALID);
    CHECK(select_sub_batches(beyond, 17, 10, &subs, &msg) == SELECT_PLAN_INVALID);
}

int main()
{
    names();
    requests();
    sub_batches();
    if (failures) { std::printf("select_san: %d failures\n", failures); return 1; }
    std::printf("select_san: ok\n");
    return 0;
}
