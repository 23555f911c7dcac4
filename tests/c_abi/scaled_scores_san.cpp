// scaled_scores_san.cpp -- TEST INFRASTRUCTURE.  csrc/host_scaled_scores_plan.hpp (the host-only logic of the scaled-score entries, on
// top of csrc/host_paths_plan.hpp and csrc/host_path_scores_plan.hpp) compiled on its own, without HIP, and run under ASan + UBSan:
//   * lag or tail_rows 0, lag / tail_rows / t_rows above 2^30, ld or ld_out below n_cols and n_cols above 2^31 - 1 are refused, each
//     naming its limit; the limits themselves pass;
//   * n_loss 0 or 17, an unknown transform, n_ranges 0 or 2^31, ld below n_cols are refused; 16 rows and 2^31 - 1 ranges pass;
//   * the ranges of the WRMSSE chain are one per grouping, [smallest column, largest + 1), {0, 0} for a grouping that maps no
//     series, and without a plan the whole alone.
// The vectors handed in are sized exactly, so a read or a write past an end is a report.  Built by tests/test_scaled_scores_cpu.py
// with g++ -fsanitize=address,undefined; exit code 0 = all checks passed.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

namespace {
#include "../../anofox-forecast_amd/csrc/host_paths_plan.hpp"
#include "../../anofox-forecast_amd/csrc/host_path_scores_plan.hpp"
#include "../../anofox-forecast_amd/csrc/host_scaled_scores_plan.hpp"
}

static int failures = 0;
#define CHECK(cond)                                                                       \
    do {                                                                                  \
        if (!(cond)) { std::fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); failures++; } \
    } while (0)

static bool has(const std::string &text, const char *part) { return text.find(part) != std::string::npos; }

static void scale()
{
    std::string msg;
    const size_t big = ((size_t)1 << 30) + 1, most = (size_t)1 << 30;
    CHECK(scale_check(64, 10, 5, 1, 28, 64, &msg) == PATHS_PLAN_OK);
    CHECK(scale_check(64, 64, most, most, most, 64, &msg) == PATHS_PLAN_OK);
    CHECK(scale_check(64, 0, 0, 1, 1, 0, &msg) == PATHS_PLAN_OK);
    CHECK(scale_check(64, 10, 5, 0, 28, 64, &msg) == PATHS_PLAN_INVALID && has(msg, "lag is 0, the smallest lag is 1"));
    CHECK(scale_check(64, 10, 5, 1, 0, 64, &msg) == PATHS_PLAN_INVALID && has(msg, "tail_rows is 0"));
    CHECK(scale_check(64, 10, 5, big, 28, 64, &msg) == PATHS_PLAN_INVALID && has(msg, "lag 1073741825 exceeds the limit of 2^30 rows"));
    CHECK(scale_check(64, 10, 5, 1, big, 64, &msg) == PATHS_PLAN_INVALID && has(msg, "tail_rows 1073741825 exceeds the limit of 2^30 rows"));
    CHECK(scale_check(64, 10, big, 1, 28, 64, &msg) == PATHS_PLAN_INVALID && has(msg, "t_rows 1073741825 exceeds the limit of 2^30 rows"));
    CHECK(scale_check(9, 10, 5, 1, 28, 64, &msg) == PATHS_PLAN_INVALID && has(msg, "ld is smaller than n_cols"));
    CHECK(scale_check(64, 10, 5, 1, 28, 9, &msg) == PATHS_PLAN_INVALID && has(msg, "ld_out is smaller than n_cols"));
    CHECK(scale_check(SIZE_MAX, (size_t)INT32_MAX + 1, 5, 1, 28, SIZE_MAX, &msg) == PATHS_PLAN_INVALID && has(msg, "n_cols exceeds the limit of 2^31 - 1"));
    CHECK(scale_check(SIZE_MAX, (size_t)INT32_MAX, 5, 1, 28, SIZE_MAX, &msg) == PATHS_PLAN_OK);
}

static void weighted()
{
    std::string msg;
    CHECK(weighted_scores_check(64, 10, 1, 1, 0, &msg) == PATHS_PLAN_OK);
    CHECK(weighted_scores_check(64, 64, 16, (size_t)INT32_MAX, 1, &msg) == PATHS_PLAN_OK);
    CHECK(weighted_scores_check(64, 10, 0, 1, 0, &msg) == PATHS_PLAN_INVALID && has(msg, "n_loss is 0"));
    CHECK(weighted_scores_check(64, 10, 17, 1, 0, &msg) == PATHS_PLAN_INVALID && has(msg, "n_loss 17 exceeds the limit of 16 loss rows per call"));
    CHECK(weighted_scores_check(64, 10, 1, 1, 2, &msg) == PATHS_PLAN_INVALID && has(msg, "transform 2 is unknown"));
    CHECK(weighted_scores_check(64, 10, 1, 1, -1, &msg) == PATHS_PLAN_INVALID && has(msg, "transform -1 is unknown"));
    CHECK(weighted_scores_check(64, 10, 1, 0, 0, &msg) == PATHS_PLAN_INVALID && has(msg, "n_ranges is 0"));
    CHECK(weighted_scores_check(64, 10, 1, (size_t)INT32_MAX + 1, 0, &msg) == PATHS_PLAN_INVALID && has(msg, "n_ranges exceeds the limit of 2^31 - 1"));
    CHECK(weighted_scores_check(9, 10, 1, 1, 0, &msg) == PATHS_PLAN_INVALID && has(msg, "ld is smaller than n_cols"));
}

static void ranges()
{
    // three groupings over five series: the total, two groups, the leaves; the second grouping of the next plan maps nobody
    const std::vector<int32_t> column_of = {0, 0, 0, 0, 0, 1, 1, 2, 2, 2, 3, 4, 5, 6, 7};
    CHECK(wrmsse_n_ranges(true, 3) == 3 && wrmsse_n_ranges(false, 3) == 1 && wrmsse_n_ranges(false, 0) == 1);
    std::vector<int32_t> r(6, -7);
    wrmsse_ranges(column_of.data(), 3, 5, 8, r.data());
    CHECK((r == std::vector<int32_t>{0, 1, 1, 3, 3, 8}));
    const std::vector<int32_t> holes = {2, 2, 2, -1, -1, -1};
    std::vector<int32_t> h(4, -7);
    wrmsse_ranges(holes.data(), 2, 3, 3, h.data());
    CHECK((h == std::vector<int32_t>{2, 3, 0, 0}));
    std::vector<int32_t> whole(2, -7);
    wrmsse_ranges(nullptr, 0, 5, 5, whole.data());
    CHECK((whole == std::vector<int32_t>{0, 5}));
    wrmsse_ranges(nullptr, 4, 0, 0, whole.data());
    CHECK((whole == std::vector<int32_t>{0, 0}));
}

int main()
{
    scale();
    weighted();
    ranges();
    if (failures) { std::fprintf(stderr, "scaled_scores_san: %d check(s) failed\n", failures); return 1; }
    std::printf("scaled_scores_san: ok\n");
    return 0;
}
