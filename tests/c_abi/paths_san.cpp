// paths_san.cpp -- TEST INFRASTRUCTURE.  csrc/host_paths_plan.hpp (the host-only checks of the sample-path entries) compiled on its
// own, without HIP, and run under ASan + UBSan:
//   * the mode names map to their codes, every other name (and NULL) to -1;
//   * the options check refuses a missing block, a wrong struct_size, an unknown mode, joint and route, each naming the offender;
//   * n_paths 0 and 2,049, horizon 0 and a product above 2^30 rows are refused with their limits, the limits themselves pass;
//   * 0 and 17 levels, a level below 0, above 1 and NaN are refused; 16 levels of an exactly sized vector pass;
//   * pool_rows 2^20 passes and 2^20 + 1 names the limit; the batch entry's pool_rows is the longest pool of an exactly sized vector;
//   * ld below the columns is refused under the name it is given; ld of a batch is the columns rounded up to 64, at least 64.
// The vectors handed in are sized exactly, so a read past an end is a report.  Built by tests/test_paths_cpu.py with
// g++ -fsanitize=address,undefined; exit code 0 = all checks passed.
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
}

static int failures = 0;
#define CHECK(cond)                                                                       \
    do {                                                                                  \
        if (!(cond)) { std::fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); failures++; } \
    } while (0)

static bool has(const std::string &text, const char *part) { return text.find(part) != std::string::npos; }

static void options()
{
    std::string msg;
    CHECK(paths_mode_code("cumulative") == 0 && paths_mode_code("independent") == 1);
    for (const char *bad : {"Cumulative", "", "joint", "cumulative "}) CHECK(paths_mode_code(bad) == -1);
    CHECK(paths_mode_code(nullptr) == -1);
    for (int mode = 0; mode <= 1; mode++)
        for (int joint = 0; joint <= 1; joint++)
            for (int route = 0; route <= 1; route++) CHECK(paths_options_check(true, 24, 24, mode, joint, route, &msg) == PATHS_PLAN_OK);
    CHECK(paths_options_check(false, 24, 24, 0, 0, 0, &msg) == PATHS_PLAN_NULL);
    CHECK(paths_options_check(true, 16, 24, 0, 0, 0, &msg) == PATHS_PLAN_INVALID && has(msg, "struct_size is not sizeof(AnofoxHipPathsOptions)"));
    CHECK(paths_options_check(true, 24, 24, 2, 0, 0, &msg) == PATHS_PLAN_INVALID && has(msg, "mode 2 is unknown"));
    CHECK(paths_options_check(true, 24, 24, -1, 0, 0, &msg) == PATHS_PLAN_INVALID && has(msg, "mode -1 is unknown"));
    CHECK(paths_options_check(true, 24, 24, 0, 2, 0, &msg) == PATHS_PLAN_INVALID && has(msg, "joint 2 is neither 0 nor 1"));
    CHECK(paths_options_check(true, 24, 24, 0, 0, 2, &msg) == PATHS_PLAN_INVALID && has(msg, "route 2 is unknown"));
}

static void rows()
{
    std::string msg;
    CHECK(paths_rows_check(1, 1, &msg) == PATHS_PLAN_OK);
    CHECK(paths_rows_check(28, 2048, &msg) == PATHS_PLAN_OK);
    CHECK(paths_rows_check(((size_t)1 << 30) / 2048, 2048, &msg) == PATHS_PLAN_OK);                    // exactly 2^30 rows
    CHECK(paths_rows_check(((size_t)1 << 30) / 2048 + 1, 2048, &msg) == PATHS_PLAN_INVALID && has(msg, "exceeds the limit of 2^30 rows"));
    CHECK(paths_rows_check(std::numeric_limits<size_t>::max(), 3, &msg) == PATHS_PLAN_INVALID && has(msg, "2^30 rows"));      // no overflow
    CHECK(paths_rows_check(28, 0, &msg) == PATHS_PLAN_INVALID && has(msg, "n_paths is 0"));
    CHECK(paths_rows_check(28, 2049, &msg) == PATHS_PLAN_INVALID && has(msg, "n_paths 2049 exceeds the limit of 2048 paths per call"));
    CHECK(paths_rows_check(0, 100, &msg) == PATHS_PLAN_INVALID && has(msg, "horizon must be at least 1"));
}

static void levels()
{
    std::string msg;
    std::vector<double> sixteen(16);                          // exactly 16 entries
    for (int k = 0; k < 16; k++) sixteen[k] = k / 15.0;
    for (size_t n = 1; n <= 16; n++) {
        std::vector<double> exact(sixteen.begin(), sixteen.begin() + n);
        CHECK(paths_levels_check(exact.data(), n, &msg) == PATHS_PLAN_OK);
    }
    std::vector<double> seventeen(17, 0.5);
    CHECK(paths_levels_check(seventeen.data(), 17, &msg) == PATHS_PLAN_INVALID && has(msg, "n_levels 17 exceeds the limit of 16 levels per call"));
    CHECK(paths_levels_check(sixteen.data(), 0, &msg) == PATHS_PLAN_INVALID && has(msg, "n_levels is 0"));
    CHECK(paths_levels_check(nullptr, 3, &msg) == PATHS_PLAN_NULL);
    std::vector<double> bad{0.1, -0.25, 0.9};
    CHECK(paths_levels_check(bad.data(), 3, &msg) == PATHS_PLAN_INVALID && has(msg, "level 1 is -0.25, outside [0, 1]"));
    bad[1] = 1.5;
    CHECK(paths_levels_check(bad.data(), 3, &msg) == PATHS_PLAN_INVALID && has(msg, "level 1 is 1.5, outside [0, 1]"));
    bad[1] = 0.5; bad[2] = std::nan("");
    CHECK(paths_levels_check(bad.data(), 3, &msg) == PATHS_PLAN_INVALID && has(msg, "level 2 is") && has(msg, "outside [0, 1]"));
    bad[2] = 1.0; bad[0] = 0.0;
    CHECK(paths_levels_check(bad.data(), 3, &msg) == PATHS_PLAN_OK);
}

static void pools_and_blocks()
{
    std::string msg;
    CHECK(paths_pool_check(0, &msg) == PATHS_PLAN_OK && paths_pool_check((size_t)1 << 20, &msg) == PATHS_PLAN_OK);
    CHECK(paths_pool_check(((size_t)1 << 20) + 1, &msg) == PATHS_PLAN_INVALID && has(msg, "pool_rows 1048577 exceeds the limit of 2^20 = 1048576 rows per pool"));
    std::mt19937 rng(20261);
    for (int round = 0; round < 200; round++) {
        const size_t n = rng() % 300;
        std::vector<size_t> len(n);                           // exactly n entries
        size_t longest = 0;
        for (size_t s = 0; s < n; s++) { len[s] = rng() % 2000; longest = len[s] > longest ? len[s] : longest; }
        size_t rows = 77;
        CHECK(paths_batch_pools(n ? len.data() : nullptr, n, &rows, &msg) == PATHS_PLAN_OK && rows == longest);
        if (n) {
            len[rng() % n] = ((size_t)1 << 20) + 1 + rng() % 5;
            CHECK(paths_batch_pools(len.data(), n, &rows, &msg) == PATHS_PLAN_INVALID && has(msg, "exceeds the limit of 2^20"));
        }
    }
    size_t rows = 0;
    CHECK(paths_batch_pools(nullptr, 3, &rows, &msg) == PATHS_PLAN_NULL);
    std::vector<size_t> one(1, 5);
    CHECK(paths_batch_pools(one.data(), 1, nullptr, &msg) == PATHS_PLAN_NULL);
    CHECK(paths_block_check(64, 64, "ld_out", "n_series", &msg) == PATHS_PLAN_OK);
    CHECK(paths_block_check(63, 64, "ld_out", "n_series", &msg) == PATHS_PLAN_INVALID && has(msg, "ld_out is smaller than n_series"));
    CHECK(paths_block_check(9, 10, "ld", "n_cols", &msg) == PATHS_PLAN_INVALID && has(msg, "ld is smaller than n_cols"));
    CHECK(paths_block_check(std::numeric_limits<size_t>::max(), (size_t)INT32_MAX + 1, "ld", "n_cols", &msg) == PATHS_PLAN_INVALID &&
          has(msg, "n_cols exceeds the limit of 2^31 - 1"));
    CHECK(paths_ld(0) == 64 && paths_ld(1) == 64 && paths_ld(64) == 64 && paths_ld(65) == 128 && paths_ld(30490) == 30528);
}

int main()
{
    options();
    rows();
    levels();
    pools_and_blocks();
    if (failures) { std::printf("paths_san: %d failures\n", failures); return 1; }
    std::printf("paths_san: ok\n");
    return 0;
}
