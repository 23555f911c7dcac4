// parts_san.cpp -- TEST INFRASTRUCTURE.  csrc/host_parts.hpp (how the batch entry cuts an auto-detected batch into device batches,
// and how the results of a device batch reach the caller's arrays) compiled on its own, without HIP.  The GPU suites hold every
// route of the forecast entry to the oracle bit for bit, but reach the planning rules only through forecasts; this program checks
// the plan itself against a brute-force restatement (written here from the rules, with integer arithmetic and no shared code):
//   * every series is in exactly one batch, exactly once; a part of a merged batch is whole 64-column blocks, padded at its end only;
//   * the period is constant within a block and ascending along a merged batch; no batch mixes the LDS-ring and the HBM-ring class;
//   * the AutoARIMA rule merges periods 25..2048 only; a part of 2,048 series or more is never merged; a class (or a cut of it) left
//     with one part goes back to the separate parts;
//   * an HBM-ring batch stays within 2 GiB of ring scratch per spec, and is cut only where the next part would have crossed it;
//   * the separate parts are split at 2,048 series, both lists largest first; the thread groups are one per LDS-ring batch and ONE
//     for all HBM-ring batches;
// and the result helpers with malloc'ed arrays, where ASan's leak check is the proof of "freed once, nothing lost": horizon 0 frees
// and nulls the three forecast arrays, a horizon at or past n_forecasts changes nothing, padding columns are freed and written
// nowhere, a failed run frees every result.
// Built by tests/test_abi_cpu.py with g++ -fsanitize=address,undefined; exit code 0 = all checks passed.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <random>
#include <set>
#include <string>
#include <vector>

#include "../../include/anofox_fcst_hip.h"
namespace {
#include "../../anofox-forecast_amd/csrc/host_parts.hpp"
}

static int failures = 0;
#define CHECK(cond)                                                                       \
    do {                                                                                  \
        if (!(cond)) { std::fprintf(stderr, "FAILED %s:%d: %s  [%s]\n", __FILE__, __LINE__, #cond, g_case.c_str()); failures++; } \
    } while (0)
static std::string g_case;

static const PartLimits LIMITS{16, 2048};          // ETS_MERGED_LDS_PERIOD, ETS_MAX_PERIOD (ets_device.hpp)

// ---- the rules, restated ------------------------------------------------------------------------------------------------------
static bool ring_scratch_too_large(uint64_t cols, uint64_t m_hi)
{
    const uint64_t workgroups = std::max<uint64_t>((cols + 15) / 16, std::min<uint64_t>(cols, 2048));
    return workgroups * m_hi * 512 > (uint64_t)2 << 30;
}
static uint64_t pad64(uint64_t n) { return (n + 63) / 64 * 64; }

struct Expected {
    std::vector<std::vector<int>> lds, hbm;        // the periods of every merged batch, ascending
    std::set<int> separate;                        // the periods that run as batches of their own
};

static Expected brute_force(const std::map<int, size_t> &count, MergeRule rule)
{
    Expected x;
    std::vector<int> lo, hi;
    for (const auto &kv : count) {
        const int p = kv.first;
        const bool small = kv.second < 2048;
        bool is_lo = false, is_hi = false;
        if (rule == MergeRule::EtsLike && small) { is_lo = p >= 2 && p <= 16; is_hi = p >= 17 && p <= 2048; }
        if (rule == MergeRule::AutoArima && small) is_hi = p >= 25 && p <= 2048;
        if (is_lo) lo.push_back(p);
        else if (is_hi) hi.push_back(p);
        else x.separate.insert(p);
    }
    if (lo.size() >= 2) x.lds.push_back(lo);
    else for (int p : lo) x.separate.insert(p);
    std::vector<std::vector<int>> cuts(1);
    uint64_t cols = 0;
    for (int p : hi) {                             // (a std::map walks its keys in ascending order)
        const uint64_t pc = pad64(count.at(p));
        if (!cuts.back().empty() && ring_scratch_too_large(cols + pc, (uint64_t)p)) { cuts.emplace_back(); cols = 0; }
        cols += pc;
        cuts.back().push_back(p);
    }
    for (auto &cut : cuts) {
        if (cut.size() >= 2) x.hbm.push_back(cut);
        else for (int p : cut) x.separate.insert(p);
    }
    return x;
}

// ---- one case: a period per series, under every rule ----------------------------------------------------------------------------
static void check_plan(const std::string &name, const std::vector<int> &period, size_t min_cuts = 0)
{
    std::map<int, size_t> count;
    for (int p : period) count[p]++;
    const MergeRule rules[3] = {MergeRule::None, MergeRule::EtsLike, MergeRule::AutoArima};
    const char *rule_names[3] = {"none", "ets-like", "autoarima"};
    for (int ri = 0; ri < 3; ri++) {
        g_case = name + " / " + rule_names[ri];
        const MergeRule rule = rules[ri];
        const std::vector<Part> by_period = parts_by_period(period);
        CHECK(by_period.size() == count.size());
        for (const Part &part : by_period) {
            CHECK(count.count(part.period) && part.series.size() == count[part.period]);
            for (size_t s : part.series) CHECK(s < period.size() && period[s] == part.period);
        }
        const PartPlan plan = plan_parts(by_period, rule, LIMITS);
        const Expected want = brute_force(count, rule);

        std::vector<int> seen(period.size(), 0);
        std::vector<std::vector<int>> got_lds, got_hbm;
        size_t hbm_groups = 0;
        for (const std::vector<MergedBatch> &group : plan.merged_groups) {
            CHECK(!group.empty());
            bool group_is_hbm = false;
            for (const MergedBatch &batch : group) {
                CHECK(batch.size() >= 2);                              // a batch of one part is no merged batch
                std::vector<int> periods;
                for (const Part &part : batch) periods.push_back(part.period);
                CHECK(std::is_sorted(periods.begin(), periods.end()) && std::adjacent_find(periods.begin(), periods.end()) == periods.end());
                const bool is_hbm = periods.back() > 16;
                CHECK(is_hbm ? periods.front() > 16 : periods.back() <= 16);       // no mix of the ring classes
                group_is_hbm = group_is_hbm || is_hbm;
                (is_hbm ? got_hbm : got_lds).push_back(periods);
                if (rule == MergeRule::AutoArima) CHECK(periods.front() >= 25 && periods.back() <= 2048);
                CHECK(periods.front() >= 2 && periods.back() <= 2048);
                // the columns
                const MergedColumns mc = merged_columns(batch);
                CHECK(mc.src.size() == mc.period.size() && mc.src.size() % 64 == 0 && mc.m_max == periods.back());
                size_t off = 0;
                for (const Part &part : batch) {
                    const size_t k = part.series.size(), padded = (size_t)pad64(k);
                    CHECK(k < 2048 && k > 0 && padded - k < 64);
                    if (off + padded > mc.src.size()) { CHECK(!"a part runs past the batch"); break; }
                    for (size_t j = 0; j < padded; j++) {
                        CHECK(mc.period[off + j] == part.period);
                        if (j < k) { CHECK(mc.src[off + j] == part.series[j]); if (mc.src[off + j] < seen.size()) seen[mc.src[off + j]]++; }
                        else CHECK(mc.src[off + j] == PAD_COLUMN);     // padding only at the end of a part
                    }
                    off += padded;
                }
                CHECK(off == mc.src.size());
                for (size_t j = 0; j < mc.src.size(); j++) CHECK(mc.period[j] == mc.period[j / 64 * 64]);        // one period per block
                CHECK(std::is_sorted(mc.period.begin(), mc.period.end()));
                if (is_hbm) CHECK(!ring_scratch_too_large(mc.src.size(), (uint64_t)mc.m_max));
            }
            if (group_is_hbm) hbm_groups++;
            else CHECK(group.size() == 1);                             // an LDS-ring batch is a group of its own
        }
        CHECK(hbm_groups <= 1);                                        // all HBM-ring batches run one after the other
        if (rule == MergeRule::None) CHECK(plan.merged_groups.empty());
        std::sort(got_lds.begin(), got_lds.end());
        std::sort(got_hbm.begin(), got_hbm.end());
        CHECK(got_lds == want.lds && got_hbm == want.hbm);             // the cuts fall where the restatement puts them
        // a cut falls only where the next part would have crossed the limit
        // (the part that follows a batch in its class -- the next period up with fewer than 2,048 series -- did not fit)
        size_t cuts_seen = 0;
        for (const std::vector<int> &periods : got_hbm) {
            uint64_t cols = 0;
            for (int p : periods) cols += pad64(count[p]);
            auto next = count.upper_bound(periods.back());
            while (next != count.end() && next->second >= 2048) ++next;
            if (next == count.end() || next->first > 2048) continue;
            CHECK(ring_scratch_too_large(cols + pad64(next->second), (uint64_t)next->first));
            cuts_seen++;
        }
        CHECK(rule == MergeRule::None || cuts_seen >= min_cuts);       // (the case really reaches the cut)
        // the separate parts
        std::set<int> got_separate;
        for (const Part &part : plan.big) { CHECK(part.series.size() >= 2048); got_separate.insert(part.period); }
        for (const Part &part : plan.small) { CHECK(part.series.size() < 2048); got_separate.insert(part.period); }
        CHECK(got_separate == want.separate && got_separate.size() == plan.big.size() + plan.small.size());
        for (const auto *list : {&plan.big, &plan.small}) {
            CHECK(std::is_sorted(list->begin(), list->end(), [](const Part &a, const Part &b) { return a.series.size() > b.series.size(); }));
            for (const Part &part : *list) {
                CHECK(count[part.period] == part.series.size());
                for (size_t s : part.series) if (s < seen.size()) seen[s]++;
            }
        }
        for (const auto &kv : count) if (kv.second >= 2048) CHECK(got_separate.count(kv.first));      // never merged
        for (size_t s = 0; s < seen.size(); s++) if (seen[s] != 1) { CHECK(!"a series is missing or repeated"); break; }
    }
}

// ---- results with malloc'ed arrays ----------------------------------------------------------------------------------------------
static double *numbers(size_t n, double first)
{
    double *p = (double *)std::malloc(std::max<size_t>(n, 1) * sizeof(double));
    for (size_t i = 0; i < n; i++) p[i] = first + (double)i;
    return p;
}
static ForecastResult make_result(size_t h, size_t n_fitted, double first)
{
    ForecastResult r;
    std::memset(&r, 0, sizeof r);
    r.n_forecasts = h;
    r.point_forecasts = numbers(h, first); r.lower_bounds = numbers(h, first - 1.0); r.upper_bounds = numbers(h, first + 1.0);
    r.n_fitted = n_fitted;
    r.fitted_values = numbers(n_fitted, first); r.residuals = numbers(n_fitted, -first);
    return r;
}

static void check_results()
{
    g_case = "results";
    {   // horizon 0 frees and nulls the three forecast arrays (and nothing else)
        ForecastResult r = make_result(5, 7, 10.0);
        truncate_to_horizon(r, 0);
        CHECK(r.n_forecasts == 0 && !r.point_forecasts && !r.lower_bounds && !r.upper_bounds && r.fitted_values && r.residuals && r.n_fitted == 7);
        free_result_arrays(r);
        CHECK(!r.fitted_values && !r.residuals);
        free_result_arrays(r);                     // (a second free finds nothing)
    }
    {   // a prefix keeps the arrays; a horizon at or past n_forecasts, or a negative one, changes nothing
        ForecastResult r = make_result(5, 0, 20.0);
        const ForecastResult before = r;
        truncate_to_horizon(r, 5);
        truncate_to_horizon(r, 9);
        truncate_to_horizon(r, -1);
        CHECK(std::memcmp(&r, &before, sizeof r) == 0);
        truncate_to_horizon(r, 3);
        CHECK(r.n_forecasts == 3 && r.point_forecasts == before.point_forecasts && r.point_forecasts[2] == 22.0 && r.upper_bounds[0] == 21.0);
        free_result_arrays(r);
        ForecastResult none;                       // a series that failed: no arrays, nothing to cut
        std::memset(&none, 0, sizeof none);
        truncate_to_horizon(none, 0);
        CHECK(none.n_forecasts == 0 && !none.point_forecasts);
    }
    {   // deliver: six columns of a batch for four of the caller's five series, two of them padding that was given arrays
        const size_t src[6] = {3, 0, PAD_COLUMN, 4, PAD_COLUMN, 1};
        const int horizons[5] = {2, 0, 99, 7, 4};
        ForecastResult res[6];
        AnofoxError errs[6];
        for (size_t j = 0; j < 6; j++) {
            res[j] = make_result(4, j % 2 ? 3 : 0, 100.0 * (double)(j + 1));
            std::memset(&errs[j], 0, sizeof errs[j]);
            errs[j].code = (ErrorCode)(j == 5 ? 3 : 0);
        }
        ForecastResult out[5];
        AnofoxError out_errs[5];
        std::memset(out, 0x5a, sizeof out);
        std::memset(out_errs, 0x5a, sizeof out_errs);
        ForecastResult untouched;
        std::memset(&untouched, 0x5a, sizeof untouched);
        const ForecastResult col0 = res[0], col1 = res[1], col3 = res[3];
        deliver_results(res, errs, src, 6, horizons, 4, out, out_errs);
        CHECK(std::memcmp(&out[2], &untouched, sizeof untouched) == 0);                    // nobody's series: written nowhere
        CHECK(!res[2].point_forecasts && !res[2].fitted_values && !res[4].point_forecasts && !res[4].residuals);      // padding: freed
        CHECK(out[3].point_forecasts == col0.point_forecasts && out[3].n_forecasts == 4);  // horizon 7 of 4: whole
        CHECK(out[0].point_forecasts == col1.point_forecasts && out[0].n_forecasts == 2 && out[0].fitted_values == col1.fitted_values);
        CHECK(out[4].point_forecasts == col3.point_forecasts && out[4].n_forecasts == 4);
        CHECK(out[1].n_forecasts == 0 && !out[1].point_forecasts && !out[1].lower_bounds && !out[1].upper_bounds && out[1].fitted_values);
        CHECK(out_errs[1].code == (ErrorCode)3 && out_errs[0].code == (ErrorCode)0 && (unsigned char)out_errs[2].message[0] == 0x5a);
        for (size_t s : {(size_t)0, (size_t)1, (size_t)3, (size_t)4}) free_result_arrays(out[s]);
        // without per-series horizons the call's horizon cuts; without out_errors only results move
        ForecastResult one = make_result(6, 0, 1.0), got;
        const size_t first = 0;
        deliver_results(&one, errs, &first, 1, nullptr, 2, &got, nullptr);
        CHECK(got.n_forecasts == 2 && got.point_forecasts[1] == 2.0);
        free_result_arrays(got);
    }
    {   // a failed run frees every result
        ForecastResult res[3] = {make_result(3, 2, 1.0), make_result(0, 0, 2.0), make_result(8, 8, 3.0)};
        free_results(res, 3);
        for (const ForecastResult &r : res) CHECK(!r.point_forecasts && !r.lower_bounds && !r.upper_bounds && !r.fitted_values && !r.residuals);
        free_results(res, 0);
        free_results(nullptr, 0);
    }
}

int main()
{
    std::mt19937_64 rng(20261019);
    auto shuffled = [&](std::vector<int> v) { std::shuffle(v.begin(), v.end(), rng); return v; };
    auto repeat = [](std::vector<int> &v, int p, size_t n) { v.insert(v.end(), n, p); };

    check_plan("empty", {});
    check_plan("one series", {7});
    check_plan("one period", std::vector<int>(300, 12));
    check_plan("one period, big", std::vector<int>(5000, 1));
    {
        std::vector<int> v;
        repeat(v, 7, 3000);
        for (int k = 0; k < 40; k++) repeat(v, 2 + 13 * k + (int)(rng() % 5), 1 + rng() % 90);       // 40 rare periods 2..~515
        check_plan("3000 of period 7 beside 40 rare periods", shuffled(v));
    }
    {
        std::vector<int> v;
        for (int p : {1, 2, 15, 16, 17, 23, 24, 25, 26, 63, 64, 65, 2047, 2048, 2049}) repeat(v, p, 1 + rng() % 130);
        check_plan("both sides of 16, 24, 64 and 2048", shuffled(v));
        check_plan("the lone period of a class", {5, 5, 5, 30, 30, 1, 1, 2049});
        check_plan("two classes of two", {5, 5, 9, 30, 31, 31, 1});
        check_plan("AutoARIMA: 24 and 25", {24, 24, 25, 26, 26, 26});
    }
    {
        std::vector<int> v;
        for (int k = 0; k < 72; k++) repeat(v, 556 + 2 * k, 1);
        check_plan("72 distinct long periods 556..698", v);
    }
    {
        std::vector<int> v;
        repeat(v, 7, 2047); repeat(v, 12, 2048); repeat(v, 30, 2047); repeat(v, 52, 2048); repeat(v, 9, 3); repeat(v, 90, 64); repeat(v, 91, 65);
        check_plan("parts of exactly 2,047 and 2,048 series", shuffled(v));
    }
    {
        // many rare long periods: the HBM-ring class has to be cut.  One series per period from 1349 up: the restatement finds the
        // first cut, and the cases end one part past it (a cut that leaves ONE part: it goes back), two past it, and far past it
        size_t first_cut = 0;
        for (uint64_t k = 1; k <= 700 && !first_cut; k++) if (ring_scratch_too_large(64 * k, 1348 + k)) first_cut = (size_t)k - 1;
        g_case = "the first cut";
        CHECK(first_cut > 100 && first_cut < 690);
        for (size_t n : {first_cut, first_cut + 1, first_cut + 2, (size_t)700}) {
            std::vector<int> v;
            for (size_t k = 0; k < n; k++) repeat(v, 1349 + (int)k, 1);
            check_plan("long periods 1349.., " + std::to_string(n) + " of them", shuffled(v), n > first_cut ? 1 : 0);
        }
        std::vector<int> v;                        // wider parts: cuts at several places, periods up to the cap
        for (int p = 1200; p <= 2048; p++) repeat(v, p, 1 + (size_t)(p % 7) * 40);
        check_plan("wide long parts 1200..2048", v, 2);
    }
    for (int round = 0; round < 20; round++) {
        std::vector<int> v;
        const size_t n_periods = 1 + rng() % 60;
        for (size_t k = 0; k < n_periods; k++) repeat(v, 1 + (int)(rng() % (round % 2 ? 2100 : 70)), 1 + rng() % (round % 5 ? 200 : 2500));
        check_plan("random " + std::to_string(round), shuffled(v));
    }
    check_results();

    if (failures) { std::fprintf(stderr, "%d check(s) failed\n", failures); return 1; }
    std::printf("parts_san: ok\n");
    return 0;
}
