// fit_schedule_san.cpp -- TEST INFRASTRUCTURE.  csrc/host_fit_schedule.hpp (the schedule of an ETS / AutoETS fit: order, streams,
// retired specs, drivers, groups, head start, and the driver, budgets, thresholds and workgroups of every round of every spec)
// compiled on its own, without HIP.  The GPU suites hold every schedule to the oracle bit for bit, but reach the decisions only
// through forecasts; this program checks the plan itself against a restatement of the rules (written here, sharing no code with the
// header) over seeded inputs: every batch size at which a rule changes (1 .. 125,000 series), one spec / the additive six / the ten
// without a season / all 25, no / a third / all series strictly positive, periods 1, 7, 24 and one above the LDS limit, merged
// batches, given parameters, compact storage, and every schedule knob at its default and at the values the GPU tests set.
//   * every live spec has exactly total_rounds steps, a retired one none; retired = no positive series, fitted, a multiplicative component;
//   * a tiny batch (series x specs <= 1,024) is ONE one-wave-per-problem round to completion; given parameters have no round;
//   * the group schedule holds exactly under its conditions; every live spec is in one group of one class, of at most GROUP_MAX_SLOTS
//     slots on consecutive table columns; group streams are distinct, the damped-M groups first on the low streams, the others
//     from the far end;
//   * NO step launches more workgroups than the ring and simplex scratches are sized for -- the recorded GPU memory fault (24 series,
//     spec2_below = 20) was exactly that.  With top_boost_n > 0 the boosted one-wave threshold CAN outgrow the scratch (see main):
//     then a grouped long-period slot must be refused by the plan;
//   * K4, the fill policy and its lane total, the budgets (BUDGET[r], 7/4 of it when sequential), thresholds, wave priorities and
//     the source of every round's series follow the written rules.
// Built by tests/test_abi_cpu.py with g++ -fsanitize=address,undefined; exit code 0 = all checks passed.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <set>
#include <string>
#include <vector>

namespace {
#include "../../anofox-forecast_amd/csrc/host_fit_schedule.hpp"
}

static int failures = 0;
static std::string g_case;
#define CHECK(cond)                                                                       \
    do {                                                                                  \
        if (!(cond)) { if (failures < 40) std::fprintf(stderr, "FAILED %s:%d: %s  [%s]\n", __FILE__, __LINE__, #cond, g_case.c_str()); failures++; } \
    } while (0)

// ---- the rules, restated ------------------------------------------------------------------------------------------------------
// spec id = 15 error + 3 trend + season; error A M; trend N A Ad M Md; season N A M
static int x_trend(int id) { return id % 15 / 3; }
static int x_season(int id) { return id % 3; }
static bool x_valid(int id) { return !(id >= 15 && x_season(id) == 1); }
static bool x_mult(int id) { return id >= 15 || x_trend(id) == 3 || x_trend(id) == 4 || x_season(id) == 2; }
static int x_class(int id) { return x_trend(id) == 4 ? 0 : (!x_mult(id) ? 2 : 1); }      // damped-M, general, additive
static const int X_COST[30] = {3, 8, 14, 7, 13, 27, 17, 29, 41, 14, 26, 22, 63, 92, 84, 7, 1, 15, 18, 1, 29, 33, 1, 48, 16, 1, 28, 65, 1, 95};
static const int MAXI = 2147483647;

static int64_t cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }

struct Expect { int kind, budget, budget_seq, sb, s2; };

static std::vector<std::vector<int>> spec_sets(std::mt19937 &rng)
{
    std::vector<std::vector<int>> sets(4);
    std::vector<int> valid;
    for (int id = 0; id < 30; id++) if (x_valid(id)) valid.push_back(id);
    sets[0] = {valid[rng() % valid.size()]};
    sets[1] = {0, 1, 3, 4, 6, 7};
    for (int id = 0; id < 30; id += 3) sets[2].push_back(id);
    sets[3] = valid;
    return sets;
}

static long n_plans = 0, n_steps = 0, n_grouped = 0, n_tiny = 0, n_fill = 0, n_k4 = 0, n_head = 0, n_errors = 0, n_boost_over = 0, n_boost_refused = 0;
static std::string boost_example;

static void check_plan(const FitScheduleInput &in)
{
    const FitSchedule p = plan_fit_schedule(in);
    n_plans++;
    const size_t S = in.specs.size();
    const int64_t n = (int64_t)in.n;
    auto id_of = [&](size_t oi) { return in.specs[p.order[oi]].id; };
    auto live_of = [&](size_t oi) -> int64_t { return (x_mult(id_of(oi)) && in.live_pos >= 0) ? in.live_pos : (in.live_all >= 0 ? in.live_all : n); };
    auto work_of = [&](int id) { return (double)X_COST[id] * ((in.live_all < 0 ? 1.0 : (x_mult(id) ? (double)in.live_pos : (double)in.live_all)) + 1.0); };
    const bool tiny = (uint64_t)in.n * S <= 1024;
    const int R = in.fixed_params ? 0 : (tiny ? 1 : (int)in.budgets.size());
    const int64_t sized = std::max<int64_t>(cdiv(n, 16), std::min<int64_t>(n, tiny ? n : (int64_t)(size_t)std::max(in.spec2_below, in.spec2_below_md)));
    const bool long_ring = in.m > in.lim.lds_period;

    // order: a permutation by expected work, most first, ties in the caller's order; lanes round-robin
    CHECK(p.order.size() == S);
    {
        std::set<size_t> seen(p.order.begin(), p.order.end());
        CHECK(seen.size() == S && (S == 0 || *seen.rbegin() == S - 1));
        for (size_t oi = 1; oi < S; oi++) {
            const double a = work_of(id_of(oi - 1)), b = work_of(id_of(oi));
            CHECK(a > b || (a == b && p.order[oi - 1] < p.order[oi]));
        }
        for (size_t oi = 0; oi < S; oi++) CHECK(p.lane_of[oi] == (int)(oi % (size_t)in.n_lanes));
    }
    // the group partition (the errors of the plan come from here and from the ring check below)
    std::vector<int> dead(S);
    for (size_t oi = 0; oi < S; oi++) dead[oi] = in.none_pos && !in.fixed_params && x_mult(id_of(oi));
    bool want_grouped = in.group_launch > 0 && S > 1 && !tiny && !in.merged && !in.fixed_params && R > 0;
    size_t n_live = 0, per_class[3] = {0, 0, 0};
    for (size_t oi = 0; oi < S; oi++) {
        if (dead[oi]) continue;
        n_live++;
        const FitSpec &sp = in.specs[p.order[oi]];
        CHECK(sp.group_class == x_class(sp.id));
        per_class[x_class(sp.id)]++;
        if (!in.group_launcher[x_class(sp.id)] || sp.nm_scratch_per_wg != 0) want_grouped = false;
    }
    if (n_live == 0) want_grouped = false;
    if (!p.error.empty()) {
        n_errors++;
        const bool too_many = p.error == "launch_fit_slots: more specs in one group than GROUP_MAX_SLOTS";
        const bool ring = p.error == "launch_fit_slots: the seasonal-ring scratch does not cover a group slot";
        CHECK(too_many || ring);
        CHECK(want_grouped);
        // a group can only be too large if its class is (an unsplit class: exactly then)
        if (too_many) {
            bool some = false;
            for (int c = 0; c < 3; c++) if (per_class[c] > (size_t)in.lim.group_max_slots) some = true;
            CHECK(some);
        }
        // the ring refusal needs a long period and a boosted threshold: never with top_boost_n = 0
        if (ring) { CHECK(long_ring && in.top_boost_n > 0); n_boost_refused++; }
        return;
    }
    for (int c = 0; c < 3; c++)          // (an unsplit class that is too large must have been refused)
        if (want_grouped && !(in.group_split == 1 + c && c < 2)) CHECK(per_class[c] <= (size_t)in.lim.group_max_slots);

    CHECK(p.tiny == tiny && p.total_rounds == R);
    CHECK(p.grouped == want_grouped);
    CHECK((int64_t)p.scratch_workgroups == sized);
    CHECK(p.inline_stream == (S == 1));
    n_tiny += tiny; n_grouped += p.grouped;

    // K4
    bool all_additive = true;
    int64_t additive_live = 0, all_live = 0;
    for (size_t oi = 0; oi < S; oi++) {
        if (dead[oi]) continue;
        if (x_mult(id_of(oi))) { if (!(in.live_all > 0 && in.live_pos >= 0 && 2 * (int64_t)in.live_pos < (int64_t)in.live_all)) all_additive = false; }
        else additive_live += live_of(oi);
        all_live += live_of(oi);
    }
    const bool k4_on = in.k4 > 0 || (in.k4 < 0 && in.fp64 && ((all_additive && additive_live >= 131072) || all_live >= 524288));
    for (size_t oi = 0; oi < S; oi++) {
        CHECK((p.dead[oi] != 0) == (dead[oi] != 0));
        const bool want = k4_on && !dead[oi] && !in.fixed_params && !x_mult(id_of(oi)) && in.specs[p.order[oi]].has_k4;
        CHECK((p.k4[oi] != 0) == want);
        n_k4 += want;
    }
    // fill policy: four lanes per live problem exceed eight times the resident lanes; the lane total never passes the target
    const int64_t resident = 2 * 1024 * 64;
    const bool fill = in.fill_policy > 0 && !tiny && !in.fixed_params && S > 1 && in.seq_rounds_env < 0 && in.seq_rounds == 0 && 4 * all_live > 8 * resident;
    CHECK(p.fill_mode == fill);
    n_fill += fill;
    {
        int64_t lanes = all_live;
        const int64_t target = resident * in.fill_target / 100;
        for (size_t oi = 0; oi < S; oi++) {
            bool want = false;
            if (fill && !dead[oi] && !p.k4[oi] && lanes + 3 * live_of(oi) <= target) { want = true; lanes += 3 * live_of(oi); }
            CHECK((p.fill_spec4[oi] != 0) == want);
            if (want) CHECK(lanes <= target);
        }
    }
    // groups
    if (p.grouped) {
        std::vector<int> in_group(S, 0);
        std::set<int> streams;
        size_t col = 0, n_dm_groups = 0;
        bool seen_other = false;
        CHECK(!p.groups.empty() && p.groups.size() <= 4);
        for (size_t g = 0; g < p.groups.size(); g++) {
            const FitGroup &G = p.groups[g];
            CHECK(!G.slots.empty() && G.slots.size() <= (size_t)in.lim.group_max_slots);
            CHECK(streams.insert(G.stream).second && G.stream >= 0 && G.stream < in.lim.n_aux_streams);
            const bool dm = G.cls == 0;
            if (dm) { CHECK(!seen_other); CHECK(G.stream == (int)g); n_dm_groups++; }
            else { seen_other = true; CHECK(G.stream == in.lim.n_aux_streams - 1 - (int)g); }
            for (size_t k = 0; k < G.slots.size(); k++) {
                const size_t oi = G.slots[k];
                CHECK(oi < S && !dead[oi]);
                in_group[oi]++;
                CHECK(x_class(id_of(oi)) == G.cls);
                CHECK(p.slot_of[oi] == col++);                                   // consecutive columns, in group order
                CHECK(p.stream_of[oi] == G.stream);
                if (k > 0) CHECK(G.slots[k - 1] < oi);                            // heaviest first
            }
        }
        for (size_t oi = 0; oi < S; oi++) { CHECK(in_group[oi] == (dead[oi] ? 0 : 1)); if (dead[oi]) CHECK(p.stream_of[oi] == p.groups[0].stream); }
        CHECK(p.n_slots == n_live && col == n_live);
        CHECK(n_dm_groups == (per_class[0] == 0 ? 0u : ((in.group_split == 1 && per_class[0] > 1) ? 2u : 1u)));
        std::vector<int> fs = p.fork_streams, gs;
        for (const FitGroup &G : p.groups) gs.push_back(G.stream);
        CHECK(fs == gs);
    } else {
        CHECK(p.groups.empty() && p.n_slots == 0);
        for (size_t oi = 0; oi < S; oi++) CHECK(p.stream_of[oi] == (int)(oi % (size_t)in.n_lanes));
        CHECK(p.fork_streams.size() == (S == 1 ? 0u : (size_t)in.n_lanes));
        for (size_t i = 0; i < p.fork_streams.size(); i++) CHECK(p.fork_streams[i] == (int)i);
    }
    // head start: the damped-M chains, when there are other live chains, on a schedule of several streams
    {
        size_t dm = 0, rest = 0;
        for (size_t oi = 0; oi < S; oi++) if (!dead[oi]) (x_trend(id_of(oi)) == 4 ? dm : rest)++;
        const bool others = p.grouped ? p.groups.size() > 1 : rest > 0;          // (grouped: the second half of a split damped-M class waits too)
        const bool want = in.dm_head_rounds > 0 && R > 0 && !tiny && S > 1 && dm > 0 && others;
        CHECK(p.head_rounds == (want ? std::min(in.dm_head_rounds, R) : 0));
        for (size_t oi = 0; oi < S; oi++) {
            bool h = want && !dead[oi] && x_trend(id_of(oi)) == 4;
            if (h && p.grouped) h = p.stream_of[oi] == 0;                        // (the first damped-M group alone)
            CHECK((p.head[oi] != 0) == h);
        }
        n_head += want;
    }
    // gather columns
    {
        const bool on = in.use_gather && !in.fixed_params;
        double total = 0.0;
        std::vector<int64_t> need(S, 0);
        for (size_t oi = 0; oi < S; oi++) {
            if (!on || dead[oi]) continue;
            const int64_t c = (in.use_pos && x_mult(id_of(oi)) && in.live_pos >= 0) ? in.live_pos : n;
            need[oi] = std::min<int64_t>((int64_t)in.ld, cdiv(c, 64) * 64);
            total += (double)need[oi] * (double)std::max<size_t>(in.t_max, 1) * 8.0;
        }
        for (size_t oi = 0; oi < S; oi++) {
            CHECK(p.gather_cols[oi] <= (size_t)need[oi] && p.gather_cols[oi] % 64 == 0);
            if (!on || dead[oi]) { CHECK(p.gather_cols[oi] == 0); continue; }
            if (in.gather_cols > 0) CHECK((int64_t)p.gather_cols[oi] == std::min<int64_t>(need[oi], in.gather_cols / 64 * 64));
            else if (total <= in.gather_budget) CHECK((int64_t)p.gather_cols[oi] == need[oi]);
            else CHECK(p.gather_cols[oi] == 0 || p.gather_cols[oi] >= 1024);
        }
        double got = 0.0;
        for (size_t oi = 0; oi < S; oi++) got += (double)p.gather_cols[oi] * (double)std::max<size_t>(in.t_max, 1) * 8.0;
        if (on && in.gather_cols <= 0) CHECK(got <= std::max(in.gather_budget, 0.0) * (1.0 + 1e-12) || total <= in.gather_budget);
    }
    // the steps
    CHECK(p.steps.size() == S);
    for (size_t oi = 0; oi < S && oi < p.steps.size(); oi++) {
        const int id = id_of(oi);
        CHECK(p.steps[oi].size() == (dead[oi] ? 0u : (size_t)R));
        if (dead[oi] || p.steps[oi].size() != (size_t)R) continue;
        const int s2 = x_trend(id) == 4 ? in.spec2_below_md : in.spec2_below;
        const int64_t live = live_of(oi);
        for (int r = 0; r < R; r++) {
            const RoundStep &s = p.steps[oi][(size_t)r];
            n_steps++;
            Expect e{RK_SEQ, 0, 0, -1, -1};
            if (tiny) { e.kind = RK_SPEC2; e.budget = e.budget_seq = 1 << 30; }
            else {
                const int B = in.budgets[(size_t)r], B74 = B * 7 / 4;
                if (fill && !p.k4[oi]) {
                    if (r == 0) { e.kind = p.fill_spec4[oi] ? RK_SPEC : RK_SEQ; e.budget = e.budget_seq = p.fill_spec4[oi] ? B : B74; }
                    else {
                        e.kind = RK_AUTO; e.budget = B; e.budget_seq = B74;
                        e.sb = p.fill_spec4[oi] ? MAXI : (int)std::max<int64_t>(64, live / std::max(1, in.fill_late_div));
                        e.s2 = (int)std::max<int64_t>(32, std::min<int64_t>(s2 > 0 ? s2 : 32, live / std::max(1, in.fill_s2_div)));
                    }
                } else if (p.k4[oi]) {
                    const int sb = ((int)oi < in.k4_top && in.k4_top_below > 0) ? in.k4_top_below : in.spec_below;
                    e.budget = e.budget_seq = B;
                    if (r == 0) e.kind = live > sb ? RK_K4 : RK_SPEC;
                    else { e.kind = RK_AUTO_K4; e.sb = sb; e.s2 = s2 > 0 ? s2 : -1; }
                } else if (r == 0 || in.seq_rounds_env >= 0 || in.seq_rounds == 0) {
                    const bool four = r >= in.seq_rounds;
                    e.budget = e.budget_seq = four ? B : B74;
                    if (four && r > 0 && s2 > 0) { e.kind = RK_AUTO; e.sb = MAXI; e.s2 = s2; }
                    else e.kind = four ? RK_SPEC : RK_SEQ;
                } else {
                    e.kind = RK_AUTO; e.budget = B; e.budget_seq = B74;
                    e.sb = x_trend(id) == 4 ? in.spec_below_md : in.spec_below;
                    e.s2 = s2 > 0 ? s2 : -1;
                    if ((int)oi < in.top_boost_n) {
                        e.sb = (int)std::min<int64_t>(MAXI, (int64_t)e.sb * in.top_boost_pct / 100);
                        if (e.s2 > 0) e.s2 = (int)std::min<int64_t>(MAXI, (int64_t)e.s2 * in.top_boost_pct / 100);
                    }
                }
                // the group form: the device-side choice must land on the driver the host picked
                if (p.grouped && e.kind == RK_SPEC) e.sb = MAXI;
            }
            CHECK(s.kind == e.kind && s.budget == e.budget && s.budget_seq == e.budget_seq && s.spec_below == e.sb && s.spec2_below == e.s2);
            if (p.grouped) CHECK(s.kind != RK_SPEC2);
            CHECK(s.k4 == (e.kind == RK_K4 || e.kind == RK_AUTO_K4));
            CHECK(s.wave_prio == ((int)oi < in.prio_top ? std::max(1, 3 - (int)oi) : 0));
            CHECK(s.source == (tiny ? SRC_ALL : r > 0 ? SRC_COMPACTED : (in.use_pos && x_mult(id)) ? SRC_POSITIVE : SRC_ALL));
            // workgroups: sequential n / 64, four lanes n / 16, one wave per problem n; the device-side choice: enough for each driver it may pick
            int64_t wg = cdiv(n, 64);
            if (e.kind == RK_SPEC) wg = cdiv(n, 16);
            else if (e.kind == RK_SPEC2) wg = n;
            else if (e.kind == RK_AUTO || e.kind == RK_AUTO_K4)
                wg = std::max(wg, std::max(cdiv(std::min<int64_t>(n, std::max(e.sb, 0)), 16), std::min<int64_t>(n, std::max(e.s2, 0))));
            CHECK(s.workgroups == wg);
            // THE invariant: no launch is wider than the scratches are sized for
            const bool over = s.workgroups > sized;
            if (in.top_boost_n == 0) CHECK(!over);
            else if (over) {
                n_boost_over++;
                CHECK(!(p.grouped && long_ring && x_season(id) != 0));            // (the plan refuses that slot: counted above)
                if (boost_example.empty()) boost_example = g_case + " slot " + std::to_string(oi) + " round " + std::to_string(r) + ": " +
                                                           std::to_string(s.workgroups) + " workgroups, scratch sized for " + std::to_string(sized);
            }
        }
    }
}

int main()
{
    std::mt19937 rng(20261019u);
    const size_t NS[] = {1, 12, 24, 40, 41, 130, 1024, 4000, 15245, 30490, 125000};
    const int MS[] = {1, 7, 24, 70};
    auto pick = [&](std::initializer_list<int> v) { return *(v.begin() + rng() % v.size()); };
    for (int rep = 0; rep < 6; rep++) {
        const auto sets = spec_sets(rng);
        for (size_t n : NS) for (size_t si = 0; si < sets.size(); si++) for (int lp = 0; lp < 4; lp++) for (int m : MS)
        for (int flags = 0; flags < 8; flags++) {
            FitScheduleInput in;
            in.n = n; in.ld = (n + 63) / 64 * 64; in.t_max = (size_t)pick({90, 400, 1913}); in.m = m;
            in.merged = flags & 1; in.fixed_params = (flags & 2) != 0; in.fp64 = !(flags & 4);
            if (in.merged && m == 1) continue;
            in.lim = FitLimits{64, 4, rng() % 8 == 0 ? 8 : 16, 32, 1024, in.merged ? 16 : 64, 2 * 1024 * 64};
            in.live_pos = lp == 0 ? -1 : lp == 1 ? 0 : lp == 2 ? (int32_t)(n / 3) : (int32_t)n;
            in.live_all = lp == 0 ? -1 : (int32_t)n;
            in.none_pos = in.live_pos == 0; in.use_pos = in.live_pos > 0 && (size_t)in.live_pos < n;
            for (int id : sets[si]) {
                const bool additive = !x_mult(id);
                FitSpec sp{id, x_mult(id), x_trend(id) == 4, x_season(id) != 0, additive && !in.merged && (x_season(id) == 0 || m == 7),
                           (size_t)((id == 13 && rng() % 6 == 0) ? 320 : 0), x_class(id)};
                in.specs.push_back(sp);
            }
            in.n_lanes = (int)std::min<size_t>(32, in.specs.size());
            for (int c = 0; c < 3; c++) in.group_launcher[c] = !in.merged && rng() % 16 != 0;
            // the knobs: defaults, and the values the GPU tests set
            in.budgets = rng() % 4 ? std::vector<int>{24, 24, 24, 24, 24, 24, 48, 48, 96, 96, 192, 1024} : std::vector<int>{10, 30, 1024};
            const int sr = pick({-1, -1, 0, 2, 3, 6});
            in.seq_rounds_env = sr; in.seq_rounds = sr >= 0 ? sr : pick({0, 3});
            in.k4 = pick({-1, -1, 0, 1});
            switch (rng() % 5) {
            case 0: break;
            case 1: in.k4_top = 1; in.k4_top_below = 60; break;
            case 2: in.k4_top = 2; in.k4_top_below = 100000; break;
            case 3: in.k4_top = 6; in.k4_top_below = 150; in.spec_below = in.spec_below_md = 40; break;
            case 4: in.k4_top_below = 0; break;
            }
            const int s2 = pick({-2, -2, 0, 20, 100000});
            if (s2 > -2) in.spec2_below = in.spec2_below_md = s2;
            in.group_launch = pick({1, 1, 0}); in.group_split = pick({1, 1, 0, 2}); in.dm_head_rounds = pick({0, 0, 2});
            in.top_boost_n = pick({0, 0, 0, 2}); in.prio_top = pick({0, 0, 3});
            in.fill_policy = pick({1, 1, 1, 0});
            in.use_gather = rng() % 4 != 0; in.gather_cols = pick({0, 0, 128});
            in.gather_budget = rng() % 3 ? 1e11 : 2e8;
            g_case = "n=" + std::to_string(n) + " set=" + std::to_string(si) + " live_pos=" + std::to_string(in.live_pos) + " m=" + std::to_string(m) +
                     " flags=" + std::to_string(flags) + " seq=" + std::to_string(in.seq_rounds_env) + "/" + std::to_string(in.seq_rounds) + " k4=" + std::to_string(in.k4) +
                     " k4_top=" + std::to_string(in.k4_top) + "/" + std::to_string(in.k4_top_below) + " spec2_below=" + std::to_string(in.spec2_below) + "/" +
                     std::to_string(in.spec2_below_md) + " group=" + std::to_string(in.group_launch) + "/" + std::to_string(in.group_split) +
                     " head=" + std::to_string(in.dm_head_rounds) + " boost=" + std::to_string(in.top_boost_n) + " prio=" + std::to_string(in.prio_top) +
                     " max_slots=" + std::to_string(in.lim.group_max_slots);
            check_plan(in);
        }
    }
    // the recorded fault: 24 series of a long period, spec2_below = 20, all 25 specs -- a tiny batch runs every problem on a wave of its own
    {
        std::mt19937 r2(1);
        FitScheduleInput in;
        in.n = 24; in.ld = 64; in.t_max = 300; in.m = 70; in.live_pos = in.live_all = 24;
        const auto sets = spec_sets(r2);
        for (int id : sets[3]) in.specs.push_back(FitSpec{id, x_mult(id), x_trend(id) == 4, x_season(id) != 0, false, 0, x_class(id)});
        in.n_lanes = 25; in.spec2_below = in.spec2_below_md = 20;
        in.budgets = {24, 24, 24, 24, 24, 24, 48, 48, 96, 96, 192, 1024};
        in.group_launcher[0] = in.group_launcher[1] = in.group_launcher[2] = true;
        in.lim = FitLimits{64, 4, 16, 32, 1024, 64, 2 * 1024 * 64};
        g_case = "24 series, spec2_below=20";
        const FitSchedule p = plan_fit_schedule(in);
        CHECK(p.tiny && p.scratch_workgroups == 24 && p.steps[0].size() == 1 && p.steps[0][0].workgroups == 24);
        check_plan(in);
    }
    // every path must have been reached for the run to mean anything
    CHECK(n_tiny > 0 && n_grouped > 0 && n_fill > 0 && n_k4 > 0 && n_head > 0 && n_errors > 0 && n_steps > 100000);
    if (failures) { std::fprintf(stderr, "%d check(s) failed\n", failures); return 1; }
    std::printf("fit_schedule_san: ok (%ld plans, %ld steps; %ld grouped, %ld tiny, %ld fill, %ld K4 slots, %ld head starts, %ld refused; boosted thresholds: %ld steps wider than "
                "the scratch, %ld plans refused for it)\n", n_plans, n_steps, n_grouped, n_tiny, n_fill, n_k4, n_head, n_errors, n_boost_over, n_boost_refused);
    if (!boost_example.empty()) std::printf("  first boosted step wider than the scratch: %s\n", boost_example.c_str());
    return 0;
}
