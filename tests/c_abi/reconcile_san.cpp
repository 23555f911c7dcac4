// reconcile_san.cpp -- TEST INFRASTRUCTURE.  csrc/host_reconcile_plan.hpp (the host-only planner of the reconciliation entries)
// compiled on its own, without HIP, and run under ASan + UBSan.  Every output array is allocated at exactly the size the sizing
// call returns, so a write past an end is a report; the plan is checked against a brute-force restatement written here:
//   * bottom_col[s] is the one column whose member list is exactly [s]; agg_cols holds every other column with members, ascending;
//   * leaf_aggs of series s lists the aggregates that hold it, ascending, once per occurrence; the lists tile [0, n_leaf);
//   * struct_weights is the member count of every column, empty columns included;
//   * each refusal names what it found and writes no array: a member outside [0, n_series), a series without a bottom column, a
//     series with two, offsets that descend or do not start at 0, n_agg above the limit; null arrays where sizes ask for them.
// Built by tests/test_reconcile_cpu.py with g++ -fsanitize=address,undefined; exit code 0 = all checks passed.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

namespace {
#include "../../anofox-forecast_amd/csrc/host_reconcile_plan.hpp"
}

static int failures = 0;
#define CHECK(cond)                                                                       \
    do {                                                                                  \
        if (!(cond)) { std::fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); failures++; } \
    } while (0)

struct Plan { std::vector<int32_t> offs, memb; size_t n_series; };

// bottoms and aggregates in a shuffled column order, with empty columns in between
static Plan random_plan(std::mt19937 &rng, size_t n_series, size_t n_agg, size_t n_empty)
{
    std::vector<std::vector<int32_t>> cols;
    for (size_t s = 0; s < n_series; s++) cols.push_back({(int32_t)s});
    for (size_t a = 0; a < n_agg; a++) {
        std::vector<int32_t> ms;
        const size_t width = 2 + rng() % 6;
        for (size_t k = 0; k < width; k++) ms.push_back((int32_t)(rng() % n_series));      // repeats allowed: a series listed twice
        std::sort(ms.begin(), ms.end());
        cols.push_back(ms);
    }
    for (size_t e = 0; e < n_empty; e++) cols.push_back({});
    std::shuffle(cols.begin(), cols.end(), rng);
    Plan p;
    p.n_series = n_series;
    p.offs.push_back(0);
    for (auto &c : cols) {
        p.memb.insert(p.memb.end(), c.begin(), c.end());
        p.offs.push_back((int32_t)p.memb.size());
    }
    return p;
}

static void check_plan(const Plan &p)
{
    const size_t n_out = p.offs.size() - 1;
    size_t n_agg = 99, n_leaf = 99;
    std::string msg;
    CHECK(reconcile_plan_host(p.offs.data(), p.memb.data(), n_out, p.n_series, 16384, &n_agg, &n_leaf, nullptr, nullptr, nullptr, nullptr, nullptr,
                              &msg) == RECONCILE_PLAN_OK);
    // exactly sized heap arrays: ASan sees one element too many
    int32_t *bottom = new int32_t[p.n_series], *aggs = new int32_t[n_agg], *loffs = new int32_t[p.n_series + 1], *laggs = new int32_t[n_leaf];
    double *w = new double[n_out];
    size_t n_agg2 = 0, n_leaf2 = 0;
    CHECK(reconcile_plan_host(p.offs.data(), p.memb.data(), n_out, p.n_series, 16384, &n_agg2, &n_leaf2, bottom, aggs, loffs, laggs, w, &msg) ==
          RECONCILE_PLAN_OK);
    CHECK(n_agg2 == n_agg && n_leaf2 == n_leaf);
    // the restatement
    std::vector<int32_t> want_aggs;
    std::vector<std::vector<int32_t>> held(p.n_series);
    size_t entries = 0;
    for (size_t c = 0; c < n_out; c++) {
        const int32_t o0 = p.offs[c], o1 = p.offs[c + 1];
        CHECK(w[c] == (double)(o1 - o0));
        if (o1 - o0 == 1) { CHECK(bottom[p.memb[o0]] == (int32_t)c); continue; }
        if (o1 == o0) continue;
        for (int32_t k = o0; k < o1; k++) held[p.memb[k]].push_back((int32_t)want_aggs.size());
        want_aggs.push_back((int32_t)c);
        entries += (size_t)(o1 - o0);
    }
    CHECK(want_aggs.size() == n_agg && entries == n_leaf);
    for (size_t a = 0; a < n_agg && a < want_aggs.size(); a++) CHECK(aggs[a] == want_aggs[a]);
    CHECK(loffs[0] == 0 && (size_t)loffs[p.n_series] == n_leaf);
    for (size_t s = 0; s < p.n_series; s++) {
        CHECK((size_t)(loffs[s + 1] - loffs[s]) == held[s].size());
        for (size_t k = 0; k < held[s].size() && (size_t)(loffs[s + 1] - loffs[s]) == held[s].size(); k++) CHECK(laggs[loffs[s] + k] == held[s][k]);
    }
    delete[] bottom; delete[] aggs; delete[] loffs; delete[] laggs; delete[] w;
}

static void check_refusal(std::vector<int32_t> offs, std::vector<int32_t> memb, size_t n_series, size_t max_agg, const char *needle)
{
    // sentinel-filled arrays: a refusal writes nothing
    std::vector<int32_t> bottom(n_series + 1, -7), aggs(offs.size(), -7), loffs(n_series + 2, -7), laggs(memb.size() + 1, -7);
    std::vector<double> w(offs.size(), -7.0);
    size_t n_agg = 0, n_leaf = 0;
    std::string msg;
    const ReconcilePlanResult r = reconcile_plan_host(offs.data(), memb.data(), offs.size() - 1, n_series, max_agg, &n_agg, &n_leaf, bottom.data(),
                                                      aggs.data(), loffs.data(), laggs.data(), w.data(), &msg);
    CHECK(r == RECONCILE_PLAN_INVALID);
    if (msg.find(needle) == std::string::npos) { std::fprintf(stderr, "FAILED: '%s' lacks '%s'\n", msg.c_str(), needle); failures++; }
    for (int32_t v : bottom) CHECK(v == -7);
    for (int32_t v : aggs) CHECK(v == -7);
    for (int32_t v : loffs) CHECK(v == -7);
    for (int32_t v : laggs) CHECK(v == -7);
    for (double v : w) CHECK(v == -7.0);
}

int main()
{
    std::mt19937 rng(20241);
    for (size_t n_series : {1u, 2u, 7u, 64u, 300u})
        for (size_t n_agg : {0u, 1u, 5u, 130u})
            for (size_t n_empty : {0u, 3u}) check_plan(random_plan(rng, n_series, n_agg, n_empty));
    {                                                           // no columns at all; a single leaf listed twice
        Plan none; none.offs = {0}; none.n_series = 0;
        check_plan(none);
        Plan twice; twice.offs = {0, 2, 3}; twice.memb = {0, 0, 0}; twice.n_series = 1;
        check_plan(twice);
    }
    check_refusal({0, 1, 3}, {0, 0, 2}, 2, 16384, "names series 2, outside [0, 2)");
    check_refusal({0, 1, 3}, {0, 0, -1}, 2, 16384, "names series -1");
    check_refusal({0, 1, 3}, {0, 0, 1}, 2, 16384, "series 1 has no bottom column");
    check_refusal({0, 1, 2, 3}, {0, 1, 0}, 2, 16384, "series 0 has two bottom columns, 0 and 2");
    check_refusal({0, 2, 1, 3}, {0, 1, 0}, 2, 16384, "col_offsets descends at column 1");
    check_refusal({1, 2, 3}, {0, 0, 1}, 2, 16384, "does not start at 0");
    check_refusal({0, 1, 2, 4, 6}, {0, 1, 0, 1, 0, 1}, 2, 1, "n_agg 2 exceeds the limit of 1 aggregate columns");
    {                                                           // null arrays
        const int32_t offs[] = {0, 1, 3}, memb[] = {0, 0, 0};
        int32_t one[4];
        size_t a = 0, l = 0;
        std::string msg;
        CHECK(reconcile_plan_host(nullptr, memb, 2, 1, 16384, &a, &l, nullptr, nullptr, nullptr, nullptr, nullptr, &msg) == RECONCILE_PLAN_NULL);
        CHECK(reconcile_plan_host(offs, nullptr, 2, 1, 16384, &a, &l, nullptr, nullptr, nullptr, nullptr, nullptr, &msg) == RECONCILE_PLAN_NULL);
        CHECK(reconcile_plan_host(offs, memb, 2, 1, 16384, &a, &l, nullptr, one, nullptr, nullptr, nullptr, &msg) == RECONCILE_PLAN_NULL);
        CHECK(reconcile_plan_host(offs, memb, 2, 1, 16384, &a, &l, one, nullptr, one, one, nullptr, &msg) == RECONCILE_PLAN_NULL);
        CHECK(reconcile_plan_host(offs, memb, 2, 1, 16384, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, &msg) == RECONCILE_PLAN_OK);
    }
    if (failures) { std::fprintf(stderr, "reconcile_san: %d check(s) failed\n", failures); return 1; }
    std::printf("reconcile_san: ok\n");
    return 0;
}
