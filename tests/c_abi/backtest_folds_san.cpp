// Sanitizer harness for the fold table of the device backtest, CPU only: anofox::backtest_folds (csrc/host_semantics.hpp, what
// anofox_hip_backtest_folds calls) is plain host C++, so it is compiled here with g++ -fsanitize=address,undefined and walked
// over the grid of tests/test_backtest_cpu.py and over large arguments.  Checked: the count call, the capacity rule (nothing is
// written past `capacity`), and the properties every table has -- fold ids 1, 2, ..; train_end + 1 + gap = test_start; test windows
// inside the data and `horizon` rows long unless clipped; training windows that start at 0 (expanding, no embargo) or hold at most
// min_train_size rows; an embargo that keeps a later training window behind the previous test window.
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all backtest_folds_san.cpp
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../anofox-forecast_amd/csrc/host_semantics.hpp"

#define CHECK(c) do { if (!(c)) { std::fprintf(stderr, "FAIL %s:%d %s (n=%lld h=%lld folds=%lld w=%d mts=%lld gap=%lld emb=%lld init=%lld skip=%lld clip=%d)\n", \
    __FILE__, __LINE__, #c, (long long)n, (long long)h, (long long)k, w, (long long)mts, (long long)gap, (long long)emb, (long long)init, (long long)skip, (int)clip); return 1; } } while (0)

static int one(int64_t n, int64_t h, int64_t k, int w, int64_t mts, int64_t gap, int64_t emb, int64_t init, int64_t skip, bool clip)
{
    const size_t cnt = anofox::backtest_folds(n, h, k, w, mts, gap, emb, init, skip, clip, nullptr, 0);
    CHECK(cnt <= (size_t)(k > 0 ? k : 0));
    CHECK(n >= 2 || cnt == 0);
    const size_t room = cnt < 64 ? cnt : 64;
    std::vector<AnofoxHipFold> out(room + 2);                // heap blocks of the exact size: a write past them is an ASan report
    for (size_t cap : {(size_t)0, room / 2, room}) {
        for (auto &f : out) f = AnofoxHipFold{-7, -7, -7, -7, -7};
        CHECK(anofox::backtest_folds(n, h, k, w, mts, gap, emb, init, skip, clip, out.data(), cap) == cnt);
        for (size_t i = cap; i < out.size(); i++) CHECK(out[i].fold_id == -7 && out[i].test_end == -7);
    }
    const int64_t step = skip > 0 ? skip : h;
    for (size_t i = 0; i < room; i++) {
        const AnofoxHipFold &f = out[i];
        CHECK(f.fold_id == (int64_t)i + 1);
        CHECK(f.test_start == f.train_end + 1 + gap);
        CHECK(f.test_start < n && f.test_end < n);
        CHECK(f.test_end == f.test_start + h - 1 || (clip && f.test_end == n - 1 && f.test_start + h - 1 >= n));
        CHECK(f.train_start >= 0);
        if (i > 0) CHECK(f.train_end == out[i - 1].train_end + step);
        if (w == 0 && (emb <= 0 || i == 0)) CHECK(f.train_start == 0);
        if (w != 0 && f.train_start <= f.train_end && mts > 0) CHECK(f.train_end - f.train_start + 1 <= (mts > f.train_end + 1 ? f.train_end + 1 : mts));
        if (i > 0 && emb > 0) CHECK(f.train_start >= out[i - 1].test_end + 1 + emb);
    }
    return 0;
}

int main()
{
    long long calls = 0;
    for (int64_t n = 0; n <= 40; n++)
        for (int64_t h = 1; h <= 5; h++)
            for (int64_t k = 1; k <= 6; k++)
                for (int w = 0; w < 3; w++)
                    for (int64_t mts : {1, 3, 50})
                        for (int64_t gap : {0, 1, 2})
                            for (int64_t emb : {0, 1, 2})
                                for (int64_t init : {-1, 1, 10})
                                    for (int64_t skip : {-1, 1, 3})
                                        for (int clip = 0; clip < 2; clip++) {
                                            if (one(n, h, k, w, mts, gap, emb, init, skip, clip != 0)) return 1;
                                            calls++;
                                        }
    // large arguments: nothing overflows (UBSan), nothing is written past the capacity (ASan)
    const int64_t big = 2147483647;
    for (int64_t h : {(int64_t)1, (int64_t)28, (int64_t)1048576, big})
        for (int64_t k : {(int64_t)1, (int64_t)5, (int64_t)1000})
            for (int w = 0; w < 3; w++)
                for (int clip = 0; clip < 2; clip++) {
                    if (one(big, h, k, w, big, 0, 0, -1, -1, clip != 0)) return 1;
                    if (one(big, h, k, w, 7, 3, 2, big / 2, 1000, clip != 0)) return 1;
                    if (one(1913, h, k, w, 100, 0, 1, -1, -1, clip != 0)) return 1;
                    calls += 3;
                }
    if (anofox::backtest_metric_code("mae") != 0 || anofox::backtest_metric_code("coverage") != 6 || anofox::backtest_metric_code("rmse") != 7 ||
        anofox::backtest_metric_code("no such metric") != 7 || anofox::backtest_metric_code(nullptr) != 7 || anofox::backtest_metric_code("") != 7) {
        std::fprintf(stderr, "FAIL metric codes\n");
        return 1;
    }
    std::printf("OK %lld tables\n", calls);
    return 0;
}
