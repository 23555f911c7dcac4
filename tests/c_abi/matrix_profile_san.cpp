// matrix_profile_san.cpp -- TEST INFRASTRUCTURE.  csrc/host_matrix_profile.hpp (the host-only logic of the matrix-profile period
// entries) compiled on its own, without HIP, and run under ASan + UBSan:
//   * the m / exclusion rule (defaults, the clamps, a wrapped BIGINT), the profile length and that it never falls as n grows;
//   * where the arrays live, on both sides of the boundary, and the workspace sizes and slice counts at their bounds;
//   * the tile walk against a brute-force count of the tiles that hold an admissible pair; the chunks of k;
//   * the argument checks, each naming its limit, with the limits themselves passing; the batch entry's longest series of an exactly
//     sized vector; the per-series error texts.
// The vectors handed in are sized exactly, so a read past an end is a report.  Built by tests/test_matrix_profile_cpu.py with
// g++ -fsanitize=address,undefined; exit code 0 = all checks passed.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <string>
#include <vector>

namespace {
#include "../../anofox-forecast_amd/csrc/host_matrix_profile.hpp"
}

static int failures = 0;
#define CHECK(cond)                                                                       \
    do {                                                                                  \
        if (!(cond)) { std::fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); failures++; } \
    } while (0)

static bool has(const std::string &text, const char *part) { return text.find(part) != std::string::npos; }

static void rule()
{
    CHECK(mprof_subsequence(32, 0) == 4 && mprof_subsequence(1913, 0) == 191 && mprof_subsequence(100, 0) == 10 && mprof_subsequence(39, 0) == 4);
    CHECK(mprof_subsequence(100, 1) == 4 && mprof_subsequence(100, 25) == 25 && mprof_subsequence(100, 26) == 25 && mprof_subsequence(2300, 1000000) == 575);
    CHECK(mprof_arg(0) == 0 && mprof_arg(7) == 7 && mprof_arg(std::numeric_limits<uint64_t>::max()) == MPROF_HOST_ARG_CAP);
    CHECK(mprof_subsequence(4200, mprof_arg((uint64_t)-1)) == 1050);                  // static_cast<size_t> of a negative BIGINT
    CHECK(mprof_exclusion(4, 0) == 1 && mprof_exclusion(191, 0) == 47 && mprof_exclusion(3, 0) == 1 && mprof_exclusion(191, 5) == 5);
    CHECK(mprof_exclusion(8, mprof_arg((uint64_t)-1)) == MPROF_HOST_ARG_CAP);
    CHECK(mprof_profile_len(31, 0) == 0 && mprof_profile_len(32, 0) == 29 && mprof_profile_len(1913, 0) == 1723 && mprof_profile_len(8192, 2048) == 6145);
    CHECK(mprof_subsequence(8196, 2049) == 2049 && mprof_subsequence(8195, 2049) == 2048);
    for (int64_t sub : {(int64_t)0, (int64_t)4, (int64_t)17, (int64_t)2048, MPROF_HOST_ARG_CAP}) {
        int64_t last = 0;
        for (int64_t n = 0; n <= 9000; n++) {
            const int64_t p = mprof_profile_len(n, sub);
            CHECK(p >= last && (n < 32 ? p == 0 : p >= 25));                          // the source's second check cannot be reached
            last = p;
        }
    }
}

static void homes_and_workspace()
{
    CHECK(mprof_in_lds(2341, 0) && !mprof_in_lds(2342, 0) && mprof_in_lds(2203, 4) && !mprof_in_lds(2204, 4) && mprof_in_lds(1913, 0));
    CHECK(mprof_in_lds(0, 0) && mprof_in_lds(31, 0) && !mprof_in_lds(65536, 0));
    CHECK(mprof_home_doubles(2203, 2200) == 5503 && mprof_home_doubles(2204, 2201) == 5506);
    for (int64_t n = 32; n < 9000; n++)
        CHECK(!mprof_in_lds(n, 4) || mprof_in_lds(n - 1, 4));                         // no longer series fits where a shorter one does not
    CHECK(mprof_work_stride(0, 0) == 0 && mprof_work_stride(1913, 0) == 2 * 1913 && mprof_work_stride(2203, 4) == 2 * 2203);
    CHECK(mprof_work_stride(2204, 4) == 4 * 2204 + 1102 + 552 && mprof_work_stride(65536, 0) == 4 * 65536 + 32768 + 16385);
    CHECK(mprof_work_blocks(0, 10) == 0 && mprof_work_blocks(100, 0) == 0 && mprof_work_blocks(2 * 1913, 30490) == 512 && mprof_work_blocks(2 * 1913, 7) == 7);
    const size_t big = mprof_work_stride(65536, 0);
    CHECK(mprof_work_blocks(big, 30490) == (int)(MPROF_HOST_WORK_BYTES / (big * 8)) && mprof_work_blocks(big, 30490) >= 1);
    CHECK((size_t)mprof_work_blocks(big, 30490) * big * 8 <= MPROF_HOST_WORK_BYTES);
    CHECK(mprof_work_blocks((size_t)1 << 40, 5) == 1);                                 // one slice where a single one is larger than the bound
}

static void tiles()
{
    CHECK(mprof_tiles(1) == 1 && mprof_tiles(64) == 1 && mprof_tiles(65) == 2 && mprof_tiles(1723) == 27);
    CHECK(mprof_first_col_tile(0, 1) == 0 && mprof_first_col_tile(1, 1) == 1 && mprof_first_col_tile(0, 63) == 0 && mprof_first_col_tile(0, 64) == 1);
    CHECK(mprof_first_col_tile(3, 47) == 3 && mprof_first_col_tile(3, 70) == 4 && mprof_first_col_tile(0, MPROF_HOST_ARG_CAP) > 1000);
    CHECK(mprof_k_chunks(4) == 1 && mprof_k_chunks(16) == 1 && mprof_k_chunks(17) == 2 && mprof_k_chunks(2048) == 128);
    for (int64_t p : {(int64_t)25, (int64_t)63, (int64_t)64, (int64_t)65, (int64_t)129, (int64_t)500}) {
        for (int64_t excl : {(int64_t)1, (int64_t)2, (int64_t)63, (int64_t)64, (int64_t)65, (int64_t)130, p - 1, p, p + 7}) {
            if (excl < 1) continue;
            const int64_t t = mprof_tiles(p);
            int64_t brute = 0;
            std::vector<char> holds((size_t)(t * t), 0);
            for (int64_t i = 0; i < p; i++)
                for (int64_t j = i + excl; j < p; j++) holds[(size_t)((i / 64) * t + j / 64)] = 1;
            for (int64_t r = 0; r < t; r++) {
                const int64_t first = mprof_first_col_tile(r, excl);
                for (int64_t c = 0; c < t; c++) {
                    if (holds[(size_t)(r * t + c)]) CHECK(c >= first);                 // the walk visits every tile that holds a pair
                    brute += c >= first ? 1 : 0;
                }
            }
            CHECK(mprof_tile_count(p, excl) == brute);
        }
    }
    CHECK(mprof_tile_count(1723, 47) == 27 * 28 / 2);
}

static void checks_and_texts()
{
    std::string text;
    CHECK(mprof_args_check(65536, &text) == MPROF_CHECK_OK && mprof_args_check(0, &text) == MPROF_CHECK_OK && text.empty());
    CHECK(mprof_args_check(65537, &text) == MPROF_CHECK_INVALID && has(text, "Invalid input: t_rows 65537 exceeds the limit of 65536 rows per series"));
    size_t rows = 99;
    std::vector<size_t> lengths = {5, 65536, 0, 40};
    CHECK(mprof_batch_rows(lengths.data(), lengths.size(), &rows, &text) == MPROF_CHECK_OK && rows == 65536);
    lengths.push_back(65537);
    CHECK(mprof_batch_rows(lengths.data(), lengths.size(), &rows, &text) == MPROF_CHECK_INVALID && rows == 65537);
    CHECK(has(text, "a series of 65537 rows exceeds the limit of 65536 rows per series"));
    CHECK(mprof_batch_rows(nullptr, 0, &rows, &text) == MPROF_CHECK_OK && rows == 0);
    CHECK(mprof_batch_rows(nullptr, 2, &rows, &text) == MPROF_CHECK_NULL && mprof_batch_rows(lengths.data(), 1, nullptr, &text) == MPROF_CHECK_NULL);
    CHECK(mprof_series_error(1, 31, 0) == "Insufficient data: need at least 32 observations, got 31");
    CHECK(mprof_series_error(1, 0, 9) == "Insufficient data: need at least 32 observations, got 0");
    CHECK(mprof_series_error(2, 8196, 2049) ==
          "Matrix profile: the subsequence length of 2049 rows of a series of 8196 observations exceeds the limit of 2048 of the HIP backend");
    CHECK(has(mprof_series_error(2, 40000, 0), "subsequence length of 4000 rows"));
}

int main()
{
    rule();
    homes_and_workspace();
    tiles();
    checks_and_texts();
    if (failures) { std::printf("matrix_profile_san: %d check(s) failed\n", failures); return 1; }
    std::printf("matrix_profile_san: ok\n");
    return 0;
}
