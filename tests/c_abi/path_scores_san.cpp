// path_scores_san.cpp -- TEST INFRASTRUCTURE.  csrc/host_path_scores_plan.hpp (the host-only logic of the path-score entries, on top
// of csrc/host_paths_plan.hpp) compiled on its own, without HIP, and run under ASan + UBSan:
//   * no level passes (also with a NULL vector); otherwise the checks of the quantile entry: 17 levels, a level outside [0, 1];
//   * an empty, a reversed and an overlong column range are refused, each naming the range; the whole block and one column pass;
//   * the workspace is 2 * n_paths * horizon doubles;
//   * the ranges of a plan's groupings are [smallest column, largest + 1) per grouping and the whole last; a grouping that maps no
//     series is {0, 0}; without a plan there is the whole alone.
// The vectors handed in are sized exactly, so a read or a write past an end is a report.  Built by tests/test_path_scores_cpu.py
// with g++ -fsanitize=address,undefined; exit code 0 = all checks passed.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <random>
#include <string>
#include <vector>

namespace {
#include "../../anofox-forecast_amd/csrc/host_paths_plan.hpp"
#include "../../anofox-forecast_amd/csrc/host_path_scores_plan.hpp"
}

static int failures = 0;
#define CHECK(cond)                                                                       \
    do {                                                                                  \
        if (!(cond)) { std::fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); failures++; } \
    } while (0)

static bool has(const std::string &text, const char *part) { return text.find(part) != std::string::npos; }

static void levels()
{
    std::string msg;
    CHECK(path_scores_levels_check(nullptr, 0, &msg) == PATHS_PLAN_OK);
    std::vector<double> sixteen(16);
    for (int k = 0; k < 16; k++) sixteen[k] = k / 15.0;
    for (size_t n = 0; n <= 16; n++) {
        std::vector<double> exact(sixteen.begin(), sixteen.begin() + n);
        CHECK(path_scores_levels_check(exact.data(), n, &msg) == PATHS_PLAN_OK);
    }
    std::vector<double> seventeen(17, 0.5);
    CHECK(path_scores_levels_check(seventeen.data(), 17, &msg) == PATHS_PLAN_INVALID && has(msg, "n_levels 17 exceeds the limit of 16 levels per call"));
    CHECK(path_scores_levels_check(nullptr, 3, &msg) == PATHS_PLAN_NULL);
    std::vector<double> bad{0.1, 1.5, 0.9};
    CHECK(path_scores_levels_check(bad.data(), 3, &msg) == PATHS_PLAN_INVALID && has(msg, "level 1 is 1.5, outside [0, 1]"));
}

static void ranges()
{
    std::string msg;
    CHECK(path_energy_range_check(64, 0, 64, &msg) == PATHS_PLAN_OK && path_energy_range_check(64, 63, 64, &msg) == PATHS_PLAN_OK);
    CHECK(path_energy_range_check(64, 5, 5, &msg) == PATHS_PLAN_INVALID && has(msg, "the column range [5, 5) is empty or reversed"));
    CHECK(path_energy_range_check(64, 7, 3, &msg) == PATHS_PLAN_INVALID && has(msg, "the column range [7, 3) is empty or reversed"));
    CHECK(path_energy_range_check(64, 3, 65, &msg) == PATHS_PLAN_INVALID && has(msg, "the column range [3, 65) ends beyond ld = 64"));
    CHECK(path_energy_range_check(std::numeric_limits<size_t>::max(), 0, (size_t)INT32_MAX + 1, &msg) == PATHS_PLAN_INVALID &&
          has(msg, "exceeds the limit of 2^31 - 1 columns"));
    CHECK(path_energy_workspace(28, 1000) == 56000 && path_energy_workspace(1, 1) == 2);
    CHECK(path_energy_workspace(((size_t)1 << 30) / 2048, 2048) == (size_t)1 << 31);
    // three levels over 12 leaves: the total, 3 groups of 4, the leaves
    std::vector<int32_t> co(3 * 12);
    for (int s = 0; s < 12; s++) { co[s] = 0; co[12 + s] = 1 + s / 4; co[24 + s] = 4 + s; }
    std::vector<size_t> r(8, 99);
    path_scores_ranges(co.data(), 3, 12, 16, r.data());
    const size_t want[8] = {0, 1, 1, 4, 4, 16, 0, 16};
    for (int k = 0; k < 8; k++) CHECK(r[k] == want[k]);
    for (int s = 0; s < 12; s++) co[12 + s] = -1;             // a grouping that maps no series
    path_scores_ranges(co.data(), 3, 12, 16, r.data());
    CHECK(r[2] == 0 && r[3] == 0 && r[4] == 4 && r[5] == 16);
    std::vector<size_t> whole(2, 99);
    path_scores_ranges(nullptr, 3, 12, 12, whole.data());
    CHECK(whole[0] == 0 && whole[1] == 12);
    std::mt19937 rng(20262);
    for (int round = 0; round < 200; round++) {
        const size_t G = 1 + rng() % 4, n = 1 + rng() % 50;
        std::vector<int32_t> c(G * n);                        // exactly G * n entries
        for (auto &v : c) v = (int32_t)(rng() % 40) - 1;
        std::vector<size_t> out(2 * (G + 1), 99);             // exactly 2 * (G + 1) entries
        path_scores_ranges(c.data(), G, n, 39, out.data());
        for (size_t g = 0; g < G; g++) {
            CHECK(out[2 * g] <= out[2 * g + 1] && out[2 * g + 1] <= 39);
            for (size_t s = 0; s < n; s++)
                if (c[g * n + s] >= 0) CHECK(out[2 * g] <= (size_t)c[g * n + s] && (size_t)c[g * n + s] < out[2 * g + 1]);
        }
        CHECK(out[2 * G] == 0 && out[2 * G + 1] == 39);
    }
}

int main()
{
    levels();
    ranges();
    if (failures) { std::printf("path_scores_san: %d failures\n", failures); return 1; }
    std::printf("path_scores_san: ok\n");
    return 0;
}
