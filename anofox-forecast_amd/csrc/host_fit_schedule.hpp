// host_fit_schedule.hpp -- the schedule of an ETS / AutoETS fit, decided from plain values before anything is enqueued: the order,
// stream and lane of every candidate spec, the specs retired without a launch chain, the drivers (K4, fill policy), the group
// partition and its streams, the tiny-batch path, the head start of the damped multiplicative-trend chains, and for every (round,
// live spec) the driver, budgets, thresholds and workgroups of its launch.  Integer logic only: no HIP call, no kernel header, no
// device pointer.  Included by host_api.hip INSIDE its anonymous namespace (launch_fit_slots builds the input, sizes the scratches
// from the plan and walks it once); the constants of the kernel headers come in as FitLimits, so tests/c_abi/fit_schedule_san.cpp
// compiles THIS file with a plain g++ and checks every decision against a restatement under ASan + UBSan.
// None of it changes a result: every schedule walks the same Nelder-Mead iterates (test_schedule_variants_are_bit_identical).
#pragma once

enum RoundKind { RK_SEQ, RK_SPEC, RK_SPEC2, RK_AUTO, RK_K4, RK_AUTO_K4 };   // sequential / four lanes per problem / one wave per problem / device-side choice; K4 forms
enum SeriesSource { SRC_ALL, SRC_POSITIVE, SRC_COMPACTED };                  // every series / the dense list of the strictly positive ones / the round's compacted list
constexpr int FIT_GROUP_CLASSES = 3;      // kernels.hpp: 0 the damped multiplicative-trend specs, 1 the other general-class specs, 2 the additive class

struct FitLimits {                        // constants of the kernel headers and of the stream pool
    int nm_block, nm_k;                   // lanes of a one-wave workgroup, trial points of an iteration (NM_BLOCK, NM_K)
    int group_max_slots;                  // GROUP_MAX_SLOTS
    int n_aux_streams;                    // N_AUX_STREAMS
    int tiny_batch_problems;              // TINY_BATCH_PROBLEMS
    int lds_period;                       // the largest period whose seasonal ring stays in LDS, for THIS run (merged or not)
    int64_t resident_lanes;               // 2 waves x 1,024 SIMDs x 64 lanes
};

struct FitSpec {
    int id;                               // ETS spec id (0..29)
    bool has_mult, damped_mul, seasonal;  // spec_has_mult, trend index 4, a season component
    bool has_k4;                          // the launcher table has both K4 round forms
    size_t nm_scratch_per_wg;             // doubles of global simplex scratch per workgroup (0: the simplex rests in LDS)
    int group_class;                      // ets_group_class (-1: none)
};

struct FitScheduleInput {
    size_t n = 0, ld = 0, t_max = 0;
    int m = 1;
    std::vector<FitSpec> specs;           // caller order
    int32_t live_pos = -1, live_all = -1; // usable strictly positive / usable series (-1: not counted)
    bool use_pos = false, none_pos = false, fixed_params = false, merged = false, fp64 = true, use_gather = false;
    double gather_budget = 0.0;
    int seq_rounds = 3, seq_rounds_env = -1;
    int spec_below = 8192, spec_below_md = 8192, spec2_below = 1024, spec2_below_md = 2048;
    int n_lanes = 1;                      // min(N_AUX_STREAMS, slots the batch has)
    // the schedule knobs (Tunables)
    std::vector<int> budgets;
    int k4 = -1, k4_top = 1, k4_top_below = 20480;
    int fill_policy = 1, fill_target = 150, fill_late_div = 2, fill_s2_div = 16;
    int top_boost_n = 0, top_boost_pct = 200, prio_top = 0;
    int group_launch = 1, group_split = 1, dm_head_rounds = 0, gather_cols = 0;
    bool group_launcher[FIT_GROUP_CLASSES] = {false, false, false};      // a group kernel exists for this period and storage type
    FitLimits lim{};
};

struct RoundStep {
    int kind;                             // RoundKind
    int budget, budget_seq;               // passes of the round; ... when the device-side choice lands on the sequential driver
    int spec_below, spec2_below;          // FitArgs thresholds (-1: unconditional); a grouped slot: set so that the device lands on `kind`
    int wave_prio;
    int source;                           // SeriesSource
    int workgroups;                       // one-wave workgroups of the launch (ets_round_launch rounds them up to whole real ones)
    bool k4;
};

struct FitGroup { std::vector<size_t> slots; int stream; int cls; };      // slots heaviest first

struct FitSchedule {
    std::string error;                    // not empty: no schedule (the caller throws it)
    std::vector<size_t> order;            // slot -> index into the caller's specs, by expected work, most first
    std::vector<int> stream_of, lane_of;  // per slot
    bool inline_stream = false;           // ONE spec: its launches go on the run's own stream, no fork and no join
    std::vector<int> fork_streams;        // the aux streams that wait for the run's stream and are joined to it
    std::vector<char> dead, k4, fill_spec4, head;      // per slot; head: its first head_rounds rounds are enqueued ahead of the others
    bool fill_mode = false, tiny = false, grouped = false;
    int total_rounds = 0, head_rounds = 0;
    std::vector<FitGroup> groups;
    std::vector<size_t> slot_of;          // per slot: its column in a round's row of the group table
    size_t n_slots = 0;
    size_t scratch_workgroups = 0;        // what the ring scratch (per long-period spec) and the simplex scratch (+ 8) are sized for
    std::vector<size_t> gather_cols;      // per slot: columns of the gather block it asks for (0: none)
    std::vector<std::vector<RoundStep>> steps;      // per slot: total_rounds steps (none for a dead slot)
};

// relative wave-time of one fitted problem of each spec, measured on the M5 shape with the wave trace (profiles/r06_wave_residency_base.txt:
// resident wave-milliseconds per spec over a 30,490-series step, in thousands; the damped multiplicative-trend specs lead, and
// among them the additive-season one needs the most iterations, not the one with the longest step)
inline int fit_cost(int id)
{
    static const int measured[30] = {/* A,N,* */ 3, 8, 14, /* A,A,* */ 7, 13, 27, /* A,Ad,* */ 17, 29, 41, /* A,M,* */ 14, 26, 22, /* A,Md,* */ 63, 92, 84,
                                     /* M,N,* */ 7, 0, 15, /* M,A,* */ 18, 0, 29, /* M,Ad,* */ 33, 0, 48, /* M,M,* */ 16, 0, 28, /* M,Md,* */ 65, 0, 95};
    return (id >= 0 && id < 30 && measured[id] > 0) ? measured[id] : 1;
}
// expected work of a spec on THIS batch: a spec with a multiplicative component only runs on the strictly positive series
inline double work(const FitScheduleInput &in, const FitSpec &s)
{
    const double live = (in.live_all >= 0 && s.has_mult) ? (double)in.live_pos : (in.live_all >= 0 ? (double)in.live_all : 1.0);
    return (double)fit_cost(s.id) * (live + 1.0);
}
// live problems of a spec
inline int64_t live_problems(const FitScheduleInput &in, const FitSpec &s)
{
    return (s.has_mult && in.live_pos >= 0) ? (int64_t)in.live_pos : (in.live_all >= 0 ? (int64_t)in.live_all : (int64_t)in.n);
}
// a handful of series: one launch per spec, every problem on a wave of its own (two iterations per pass) to completion -- one
// series through AutoETS was 12 rounds x 3 launches x 25 specs
inline bool tiny_batch(const FitScheduleInput &in) { return (uint64_t)in.n * in.specs.size() <= (uint64_t)in.lim.tiny_batch_problems; }
// One-wave workgroups of the widest launch a run can make: four lanes per problem for every series, or one wave per problem for the
// last spec2_below -- or for ALL of a tiny batch, whatever the thresholds say (a scratch sized for 20 of 24 one-wave workgroups was
// an intermittent GPU memory fault: docs/history/r06_round_log.md section E).
inline size_t widest_launch_workgroups(const FitScheduleInput &in)
{
    const size_t n = in.n;
    return std::max<size_t>((n + 15) / 16, std::min<size_t>(n, tiny_batch(in) ? n : (size_t)std::max(in.spec2_below, in.spec2_below_md)));
}
// One-wave workgroups of a round launch (ets_round_launch): n / 64 sequential, n / 16 with four lanes per problem, one per problem;
// the device-side choice takes enough for whichever driver its thresholds allow.  A grouped slot (always the device-side choice,
// thresholds rewritten to land on `kind`) gets the same count from either reading.
inline int step_workgroups(const FitScheduleInput &in, const RoundStep &s)
{
    const int64_t n = (int64_t)in.n, per_spec = in.lim.nm_block / in.lim.nm_k;
    const int64_t g_seq = (n + in.lim.nm_block - 1) / in.lim.nm_block;
    if (s.kind == RK_SEQ || s.kind == RK_K4) return (int)g_seq;
    if (s.kind == RK_SPEC) return (int)((n + per_spec - 1) / per_spec);
    if (s.kind == RK_SPEC2) return (int)n;
    const int64_t g_spec = (std::min<int64_t>(n, std::max(s.spec_below, 0)) + per_spec - 1) / per_spec;
    const int64_t g_spec2 = std::min<int64_t>(n, std::max(s.spec2_below, 0));
    return (int)std::max(g_seq, std::max(g_spec, g_spec2));
}

inline FitSchedule plan_fit_schedule(const FitScheduleInput &in)
{
    FitSchedule p;
    const size_t n_spec = in.specs.size();
    const std::vector<int> &BUDGET = in.budgets;
    const int unconditional = 0x7fffffff;
    // enqueue order: most expensive specs first, dealt round-robin over the streams, so the long multiplicative / damped / seasonal
    // fits start together instead of queueing behind each other
    p.order.resize(n_spec);
    for (size_t i = 0; i < n_spec; i++) p.order[i] = i;
    std::stable_sort(p.order.begin(), p.order.end(), [&](size_t x, size_t y) { return work(in, in.specs[x]) > work(in, in.specs[y]); });
    auto spec = [&](size_t oi) -> const FitSpec & { return in.specs[p.order[oi]]; };
    // one stream per spec (the runtime maps them onto the hardware queues; two explicit pairing schemes -- dedicated queues for the
    // heaviest specs, heaviest-with-lightest -- both measured 14 % slower on the 30-spec batch).  ONE spec (ETS with an explicit
    // model, fitted or with given parameters): no fork, no join.  A cross-stream event wait is cheap when the host has just
    // synchronised and expensive inside a pipeline of runs: twenty fixed-parameter steps enqueued back to back took 1.4 ms each
    // with the fork / join against 0.5 ms with a host wait in between.
    p.inline_stream = n_spec == 1;
    p.lane_of.resize(n_spec);
    for (size_t oi = 0; oi < n_spec; oi++) p.lane_of[oi] = (int)(oi % (size_t)in.n_lanes);
    p.stream_of = p.lane_of;
    p.tiny = tiny_batch(in);
    p.total_rounds = in.fixed_params ? 0 : (p.tiny ? 1 : (int)BUDGET.size());
    p.scratch_workgroups = widest_launch_workgroups(in);
    // specs that are inadmissible for EVERY series of the group (a multiplicative component, no strictly positive series: the raw
    // M5 counts) get their per-series outputs from one small kernel and no launch chain at all -- 19 of the 25 chains of the
    // intermittent batch used to be compaction / gather / round launches over empty lists, queueing in front of the live ones
    p.dead.assign(n_spec, 0);
    if (in.none_pos && !in.fixed_params)
        for (size_t oi = 0; oi < n_spec; oi++) if (spec(oi).has_mult) p.dead[oi] = 1;
    // additive-class specs, one lane per problem: four trial points per pass (K4).  Their pass is memory bound (6-10 instructions per
    // 8-byte load): against the sequential driver K4 is one pass per iteration instead of ~1.7, against four lanes per problem it is
    // the same bytes through a quarter of the load instructions (512 instead of 128 bytes each)
    p.k4.assign(n_spec, 0);
    {
        bool all_additive = true;           // (-1: only when the general-class specs see under half of the series)
        int64_t additive_live = 0, all_live = 0;
        for (size_t oi = 0; oi < n_spec; oi++) {
            if (p.dead[oi]) continue;
            if (spec(oi).has_mult && !(in.live_all > 0 && in.live_pos >= 0 && 2 * (int64_t)in.live_pos < (int64_t)in.live_all)) all_additive = false;
            // ... and enough of them to fill the chip one lane per problem: two K4 waves per SIMD
            if (!spec(oi).has_mult) additive_live += live_problems(in, spec(oi));
            all_live += live_problems(in, spec(oi));
        }
        // ... or (round 5) the batch oversubscribes the chip whatever its mix: with the general-class steps a third shorter (error-correction
        // form) the 25-spec batch of strictly positive series is no longer bound by fp64 issue alone, and the additive specs' ~41 % fewer
        // passes are worth their arithmetic -- 477.6 -> 450.9 ms on the 30,490-series batch, same box (profiles/r05_tune_sweep.txt).  One
        // lane per problem fills two waves per SIMD from 131,072 live problems on; below four times that the chains' latency decides
        // (round 6) ... as long as the run streams the fp64 block.  K4 buys 41 % fewer passes with four times the arithmetic: a trade for a
        // pass bound by its BYTES.  Over a compact copy (2 or 4 bytes per observation) the additive pass is bound by its instructions like
        // every other, and K4 loses: intermittent M5 batch 58.0 -> 53.8 ms, 125k x 1,024 99.9 -> 75.5 ms, 125k x 256 with all 25 specs
        // 148-156 -> 141-142 ms, the 25-spec M5 batch unchanged (profiles/r06_k4_shapes.txt)
        const bool on = in.k4 > 0 || (in.k4 < 0 && in.fp64 && ((all_additive && additive_live >= 131072) || all_live >= 524288));
        for (size_t oi = 0; oi < n_spec; oi++) p.k4[oi] = on && !p.dead[oi] && !in.fixed_params && !spec(oi).has_mult && spec(oi).has_k4;
    }
    // Mid-size batches (round 6): fewer than 524,288 live problems (below that the first rounds run four lanes per problem for EVERY
    // spec) but so many that four lanes for everybody oversubscribe the resident lanes more than eight times -- the 15,245-series
    // shard of a 2-GPU M5 job: 381k problems, 1.5 M lanes on 131k.  There the first round's lanes are dealt by expected work: specs
    // in cost order get four lanes per problem while the total stays under fill_target x the resident lanes, the rest start one
    // lane per problem (the least arithmetic) and switch to four lanes when 1 / fill_late_div of their problems are left; one wave
    // per problem at 1 / fill_s2_div.  Measured (profiles/r06_shard_policy.txt, shard of a 2-rank job alone on one GPU): 314 -> 280 ms.
    // SMALLER batches keep four lanes for everybody: the 7,623- and 3,812-series shards (4 / 8 ranks) are bound by their longest
    // chain from the first round, and dealing them fewer lanes makes it longer (204 -> 246-320 ms, 173 -> 187-215 ms) -- the chip
    // absorbs three to six times its resident lanes of speculative work better than a chain absorbs 1.7 passes per iteration.
    // Same trajectories whatever the driver (test_schedule_variants_are_bit_identical).
    p.fill_spec4.assign(n_spec, 0);
    {
        int64_t lanes = 0;
        for (size_t oi = 0; oi < n_spec; oi++) if (!p.dead[oi]) lanes += live_problems(in, spec(oi));
        p.fill_mode = in.fill_policy > 0 && !p.tiny && !in.fixed_params && n_spec > 1 && in.seq_rounds_env < 0 && in.seq_rounds == 0 &&
                      lanes * 4 > 8 * in.lim.resident_lanes;
        if (p.fill_mode) {
            const int64_t target = in.lim.resident_lanes * (int64_t)in.fill_target / 100;
            for (size_t oi = 0; oi < n_spec; oi++) {                        // `order` is by expected work, most first
                if (p.dead[oi] || p.k4[oi]) continue;
                const int64_t more = 3 * live_problems(in, spec(oi));
                if (lanes + more <= target) { p.fill_spec4[oi] = 1; lanes += more; }
            }
        }
    }
    // gather blocks of the specs that have something to fit: as many columns as the spec can ever have running (the strictly
    // positive series for a spec with a multiplicative component), scaled down together if that exceeds the budget
    p.gather_cols.assign(n_spec, 0);
    if (in.use_gather && !in.fixed_params) {
        const size_t T = std::max<size_t>(in.t_max, 1);
        std::vector<size_t> need(n_spec, 0);
        double total = 0.0;
        for (size_t oi = 0; oi < n_spec; oi++) {
            if (p.dead[oi]) continue;
            const size_t c = (in.use_pos && spec(oi).has_mult && in.live_pos >= 0) ? (size_t)in.live_pos : in.n;
            need[oi] = std::min(in.ld, (c + 63) / 64 * 64);
            total += (double)need[oi] * (double)T * 8.0;
        }
        const double scale = total > in.gather_budget ? in.gather_budget / total : 1.0;
        for (size_t oi = 0; oi < n_spec; oi++) {
            if (p.dead[oi]) continue;
            size_t cols = scale < 1.0 ? (size_t)((double)need[oi] * scale) / 64 * 64 : need[oi];
            if (in.gather_cols > 0) cols = std::min<size_t>(need[oi], (size_t)in.gather_cols / 64 * 64);
            if (cols < need[oi] && cols < 1024 && in.gather_cols <= 0) cols = 0;      // (a block for a few hundred stragglers is not worth its launches)
            p.gather_cols[oi] = cols;
        }
    }
    // Group schedule (tune group_launch, the default): the live specs are dealt by class into at most four groups -- the damped
    // multiplicative-trend specs (the step's critical path: two groups of similar expected work, on the priority streams), the other
    // general-class specs and the additive class -- and round r of a group is ONE launch of its class's group kernel
    // (ets_group_kernel.hpp) on the group's stream, behind one compaction and one gather launch for all its slots.  So the fit needs
    // four streams whatever GPU_MAX_HW_QUEUES the host exports: with one stream per spec, 25 chains shared the runtime's default of
    // four hardware queues (453 ms per step on the M5 batch, 372 ms with 16 queues; the group schedule: 377 and 376 ms,
    // profiles/group_schedule_ab.txt).  Every argument of every round is known here, so the [round][slot] table goes to the device
    // in one copy at the start of the run.  The per-spec schedule stays for one spec, a tiny batch (one launch per spec), given
    // parameters and merged batches of several periods (per-lane period variants, which have no group kernels).
    p.slot_of.assign(n_spec, 0);
    p.grouped = in.group_launch > 0 && !p.inline_stream && !p.tiny && !in.merged && !in.fixed_params && p.total_rounds > 0;
    if (p.grouped) {
        std::vector<size_t> of_class[FIT_GROUP_CLASSES];
        for (size_t oi = 0; oi < n_spec && p.grouped; oi++) {
            if (p.dead[oi]) continue;
            const int c = spec(oi).group_class;
            if (c < 0 || c >= FIT_GROUP_CLASSES || !in.group_launcher[c] || spec(oi).nm_scratch_per_wg != 0) p.grouped = false;
            else of_class[c].push_back(oi);
        }
        auto add = [&](const std::vector<size_t> &sl, int c) {
            if (sl.empty()) return;
            if (sl.size() > (size_t)in.lim.group_max_slots) p.error = "launch_fit_slots: more specs in one group than GROUP_MAX_SLOTS";
            p.groups.push_back(FitGroup{sl, 0, c});
        };
        // one class in two groups (tune group_split: 1 the damped-M class, 2 the other general-class specs), each spec (heaviest
        // first) to the half with less expected work so far
        auto add_class = [&](int c, bool split) {
            if (!split) { add(of_class[c], c); return; }
            std::vector<size_t> half[2];
            double w[2] = {0.0, 0.0};
            for (size_t oi : of_class[c]) {
                const int j = w[1] < w[0] ? 1 : 0;
                half[j].push_back(oi); w[j] += work(in, spec(oi));
            }
            add(half[0], c); add(half[1], c);
        };
        if (p.grouped) {
            add_class(0, in.group_split == 1);
            add_class(1, in.group_split == 2);
            add_class(2, false);
            if (!p.error.empty()) return p;
            p.grouped = !p.groups.empty();
        }
        // streams: the damped-M group (when there is one) on the first, which is the priority stream where the set has one; the
        // others from the far end of the set, which never is
        for (size_t g = 0; g < p.groups.size(); g++) {
            const bool dm = spec(p.groups[g].slots[0]).damped_mul;
            p.groups[g].stream = dm ? (int)g : in.lim.n_aux_streams - 1 - (int)g;      // (the damped-M groups come first)
            for (size_t oi : p.groups[g].slots) { p.stream_of[oi] = p.groups[g].stream; p.slot_of[oi] = p.n_slots++; }
        }
        // the specs with nothing to fit only get their outputs written: on the first group's stream
        if (p.grouped) for (size_t oi = 0; oi < n_spec; oi++) if (p.dead[oi]) p.stream_of[oi] = p.groups[0].stream;
    }
    if (p.grouped) for (const FitGroup &g : p.groups) p.fork_streams.push_back(g.stream);
    else if (!p.inline_stream) for (int i = 0; i < in.n_lanes; i++) p.fork_streams.push_back(i);
    // Head start of the damped multiplicative-trend chains (tune dm_head_rounds, round 5): their fits are the step's critical path -- alone
    // on the chip one of them takes 185-280 ms of a 450 ms step (profiles/r05_step_anatomy.txt) -- and while all 25 chains start together
    // their early, full rounds share every SIMD with the cheap specs' waves.  With a head start their first rounds are enqueued alone,
    // the other specs' streams wait for an event recorded behind them, and fill the chip once those chains thin out.
    p.head.assign(n_spec, 0);
    if (in.dm_head_rounds > 0 && p.total_rounds > 0 && !p.tiny && !p.inline_stream) {
        size_t n_dm = 0, n_rest = 0;
        if (p.grouped) {            // (the damped-M group on the first stream: its first rounds alone, the other groups' streams wait behind them)
            if (p.groups.size() > 1 && p.groups[0].stream == 0 && spec(p.groups[0].slots[0]).damped_mul) {
                for (size_t oi : p.groups[0].slots) p.head[oi] = 1;
                n_dm = n_rest = 1;
            }
        } else
            for (size_t oi = 0; oi < n_spec; oi++) {
                if (p.dead[oi]) continue;
                if (spec(oi).damped_mul) { p.head[oi] = 1; n_dm++; } else n_rest++;
            }
        if (n_dm && n_rest) p.head_rounds = std::min(in.dm_head_rounds, p.total_rounds);
        else p.head.assign(n_spec, 0);
    }
    // Round-major submission: round r of every spec is enqueued before round r+1 of any, so that all specs advance together and the
    // hardware queues never hold a long spec behind another one.  Early rounds run the sequential driver (least arithmetic while
    // problems outnumber lanes), late rounds the speculative one (shortest critical path for the stragglers).
    p.steps.resize(n_spec);
    for (size_t oi = 0; oi < n_spec; oi++) {
        if (p.dead[oi]) continue;
        const FitSpec &sp = spec(oi);
        const int64_t live = live_problems(in, sp);
        const int s2 = sp.damped_mul ? in.spec2_below_md : in.spec2_below;
        for (int r = 0; r < p.total_rounds; r++) {
            RoundStep s{};
            s.wave_prio = (int)oi < in.prio_top ? std::max(1, 3 - (int)oi) : 0;
            s.spec_below = -1; s.spec2_below = -1;
            // a mixed batch: a spec with a multiplicative component runs its first round on the dense list of the strictly positive series
            s.source = (p.tiny || (r == 0 && !(in.use_pos && sp.has_mult))) ? SRC_ALL : (r == 0 ? SRC_POSITIVE : SRC_COMPACTED);
            if (p.tiny) {
                s.kind = RK_SPEC2; s.budget = 1 << 30;
            } else if (p.fill_mode && !p.k4[oi]) {
                s.budget = BUDGET[r];
                if (r == 0) {
                    s.kind = p.fill_spec4[oi] ? RK_SPEC : RK_SEQ;
                    if (!p.fill_spec4[oi]) s.budget = (BUDGET[r] * 7) / 4;
                } else {
                    s.kind = RK_AUTO; s.budget_seq = (BUDGET[r] * 7) / 4;
                    s.spec_below = p.fill_spec4[oi] ? unconditional : (int)std::max<int64_t>(64, live / std::max(1, in.fill_late_div));
                    s.spec2_below = (int)std::max<int64_t>(32, std::min<int64_t>(s2 > 0 ? s2 : 32, live / std::max(1, in.fill_s2_div)));
                }
            } else if (p.k4[oi]) {
                // additive spec of a memory-bound run: one lane per problem with four trial points per pass wherever four LANES per
                // problem would otherwise run -- the same bytes per iteration through a quarter of the load instructions (a wave of
                // four-lane groups moves 128 bytes per load, and it is the CU's address pipeline that such a run saturates) -- as
                // long as the spec still has more problems than `spec_below`; fewer are a latency problem again: four lanes, then
                // one wave per problem.
                // The most expensive spec (`k4_top` of them) switches to four lanes per problem EARLIER, at `k4_top_below` live problems
                // (20,480; every other spec at spec_below = 8,192): its chain ends the step, alone on the chip for the last 10-25 ms of
                // the intermittent M5 batch with 477 one-lane waves on 1,024 SIMDs -- four lanes per problem are the same arithmetic on
                // four times the waves.  70.6-71.7 -> 66.1-68.1 ms on that batch (thresholds 14,336-24,576: the same; 12,288 and 32,768:
                // no gain -- at 32,768 the first round already runs four lanes while all six chains still fill the chip), 125k x 1,024:
                // 138-142 -> 132-139 ms, batches with general-class specs: unchanged (profiles/r04_ab_experiments.txt).
                const int sb = ((int)oi < in.k4_top && in.k4_top_below > 0) ? in.k4_top_below : in.spec_below;
                s.budget = BUDGET[r];
                if (r == 0) s.kind = live > sb ? RK_K4 : RK_SPEC;
                else { s.kind = RK_AUTO_K4; s.budget_seq = BUDGET[r]; s.spec_below = sb; s.spec2_below = s2 > 0 ? s2 : -1; }
            } else if (r == 0 || in.seq_rounds_env >= 0 || in.seq_rounds == 0) {
                // first round (no device count yet) or a forced schedule: the host picks the driver
                const bool spec_mode = r >= in.seq_rounds;
                s.budget = spec_mode ? BUDGET[r] : (BUDGET[r] * 7) / 4;     // ~1.7 passes per iteration when sequential
                // ... but the last s2 problems still go one per wave (device-side count), in the same launch
                if (spec_mode && r > 0 && s2 > 0) { s.kind = RK_AUTO; s.budget_seq = s.budget; s.spec_below = unconditional; s.spec2_below = s2; }
                else s.kind = spec_mode ? RK_SPEC : RK_SEQ;
            } else {
                // later rounds: the device-side count of running problems picks the driver -- sequential (least arithmetic)
                // while this spec still fills >= 1/8 of the chip, then speculative (one pass per iteration), then two-level
                // speculative (one problem per wave, two iterations per pass).  ONE launch: a launch whose workgroups only find
                // out that another driver owns the round still has to be dispatched
                s.kind = RK_AUTO; s.budget = BUDGET[r]; s.budget_seq = (BUDGET[r] * 7) / 4;
                s.spec_below = sp.damped_mul ? in.spec_below_md : in.spec_below;
                s.spec2_below = s2 > 0 ? s2 : -1;
                if ((int)oi < in.top_boost_n) {         // (experiment: the chains that end the step get their parallelism earlier)
                    s.spec_below = (int)std::min<int64_t>(unconditional, (int64_t)s.spec_below * in.top_boost_pct / 100);
                    if (s.spec2_below > 0) s.spec2_below = (int)std::min<int64_t>(unconditional, (int64_t)s.spec2_below * in.top_boost_pct / 100);
                }
            }
            if (s.kind != RK_AUTO && s.kind != RK_AUTO_K4) s.budget_seq = s.budget;      // (one driver: the launch reads `budget` alone)
            s.k4 = s.kind == RK_K4 || s.kind == RK_AUTO_K4;
            if (p.grouped) {
                // the slot runs the device-side choice with the thresholds set so that it lands on the driver picked here
                if (s.kind == RK_SPEC) s.spec_below = unconditional;
                else if (s.kind == RK_SPEC2) { p.error = "launch_fit_slots: the one-wave-per-problem round of a tiny batch has no group form"; return p; }
            }
            s.workgroups = step_workgroups(in, s);
            // (the ungrouped launches check the same against the scratch they are handed: ets_round_launch)
            if (p.grouped && sp.seasonal && in.m > in.lim.lds_period && (size_t)s.workgroups > p.scratch_workgroups) {
                p.error = "launch_fit_slots: the seasonal-ring scratch does not cover a group slot"; return p;
            }
            p.steps[oi].push_back(s);
        }
    }
    return p;
}
