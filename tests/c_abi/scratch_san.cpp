// scratch_san.cpp -- TEST INFRASTRUCTURE.  csrc/host_scratch.hpp (the scratch owner, the series packer and the shape function that
// the entry families of the host layer share) compiled against tests/c_abi/fake_hip.h.  The GPU suites cover the success paths of
// every entry bit for bit; this program runs what no GPU test can reach:
//   * the owner frees every block exactly once -- after settled() without a device-wide wait, otherwise with exactly one, also
//     when a HipFail is thrown through it, and when the allocator refuses the third block of a call;
//   * an owner that never allocated touches nothing;
//   * the packer against a three-line loop: ragged lengths, NULLs on both sides of a 64-bit mask word, a series without a mask among
//     masked ones, the fill in the padding columns and past every series' end;
//   * the shape function's two refusals, code and text.
// The stand-in's device memory is a 64-byte token, so nothing is ever copied to a "device" block.
// Built by tests/test_abi_cpu.py with g++ -fsanitize=address,undefined on a "device" of 8 MB; exit code 0 = all checks passed.
#include "fake_hip.h"

#include <algorithm>
#include <atomic>
#include <chrono>
#include <climits>
#include <cmath>
#include <condition_variable>
#include <cstdint>
#include <map>
#include <memory>
#include <mutex>
#include <stdexcept>
#include <string>
#include <system_error>
#include <thread>
#include <unordered_map>
#include <vector>

#include "../../anofox-forecast_amd/csrc/host_semantics.hpp"
using namespace anofox;
namespace {
#include "../../anofox-forecast_amd/csrc/host_resources.hpp"
#include "../../anofox-forecast_amd/csrc/host_scratch.hpp"
}

static int failures = 0;
#define CHECK(cond)                                                                       \
    do {                                                                                  \
        if (!(cond)) { std::fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); failures++; } \
    } while (0)

static size_t live_blocks()
{
    DevCache &c = dev_cache();
    std::lock_guard<std::mutex> lock(c.mu);
    return c.live.size();
}

int main()
{
    FakeHip &F = fake_hip();
    CHECK(F.capacity == (size_t)8 << 20);                 // the sizes below are chosen for it

    // ---- an owner that never allocated ------------------------------------------------------------------------
    {
        const long syncs = F.n_sync, mallocs = F.n_malloc, frees = F.n_free;
        { Scratch none; }
        { Scratch none; none.settled(); }
        CHECK(F.n_sync == syncs && F.n_malloc == mallocs && F.n_free == frees && live_blocks() == 0);
    }

    // ---- success: three blocks, settled -> no device-wide wait ---------------------------------------------------
    {
        const long syncs = F.n_sync;
        {
            Scratch s;
            double *a = s.get<double>(100);
            int32_t *b = s.get<int32_t>(64);
            uint8_t *c = s.get<uint8_t>(0);                // (as dalloc: at least one item)
            CHECK(a && b && c && (void *)a != (void *)b && (void *)b != (void *)c && live_blocks() == 3);
            s.settled();
        }
        CHECK(F.n_sync == syncs && live_blocks() == 0 && F.n_bad_free == 0);
    }

    // ---- failure: an unsettled owner waits exactly once, destroyed normally and by a HipFail thrown through it --------
    {
        const long syncs = F.n_sync;
        {
            Scratch s;
            (void)s.get<double>(100); (void)s.get<double>(200); (void)s.get<int32_t>(64);
        }
        CHECK(F.n_sync == syncs + 1 && live_blocks() == 0 && F.n_bad_free == 0);
        bool caught = false;
        try {
            Scratch s;
            (void)s.get<double>(100); (void)s.get<double>(200); (void)s.get<int32_t>(64);
            throw HipFail{"a copy failed", false};
        } catch (const HipFail &f) { caught = !f.oom; }
        CHECK(caught && F.n_sync == syncs + 2 && live_blocks() == 0 && F.n_bad_free == 0);
    }

    // ---- the allocator refuses the third block of a call -----------------------------------------------------------
    {
        const long syncs = F.n_sync;
        bool refused = false;
        size_t live_at_refusal = 0;
        try {
            Scratch s;
            (void)s.get<double>((size_t)3 << 17);          // 3 MB, rounded to 4 MB: two of them fill the 8 MB device
            (void)s.get<double>((size_t)3 << 17);
            live_at_refusal = live_blocks();
            (void)s.get<double>((size_t)3 << 17);
            CHECK(!"the third block must not fit");
        } catch (const HipFail &f) { refused = f.oom; }
        (void)hipGetLastError();
        CHECK(refused && live_at_refusal == 2 && live_blocks() == 0 && F.n_sync <= syncs + 1 && F.n_bad_free == 0);
        std::lock_guard<std::mutex> lock(F.mu);
        CHECK(F.used[0] <= (size_t)2 << 20);               // (at most what the cache keeps: the cap is a quarter of the device)
    }

    // ---- the packer ------------------------------------------------------------------------------------------------
    {
        const size_t n = 65, ld = 128, pattern[6] = {0, 1, 3, 64, 65, 70};
        std::vector<size_t> len(n);
        std::vector<std::vector<double>> val(n);
        std::vector<std::vector<uint64_t>> bits(n);
        std::vector<const double *> vp(n);
        std::vector<const uint64_t *> mp(n);
        size_t T = 1;
        for (size_t s = 0; s < n; s++) {
            len[s] = pattern[s % 6];
            T = std::max(T, len[s]);
            val[s].resize(len[s]);
            for (size_t t = 0; t < len[s]; t++) val[s][t] = 1000.0 * (double)s + (double)t + 0.5;
            bits[s].assign(2, ~0ull);
            for (size_t t : {(size_t)0, (size_t)63, (size_t)64, (size_t)69})
                if ((s % 4) != 2) bits[s][t >> 6] &= ~(1ull << (t & 63));          // (three series in four carry the NULLs)
            vp[s] = len[s] ? val[s].data() : nullptr;
            mp[s] = bits[s].data();
        }
        mp[5] = nullptr;                                   // length 70, no mask, among masked ones
        CHECK(len[5] == 70 && len[4] == 65);

        BlockShape shape;
        AnofoxError err;
        CHECK(series_shape(vp.data(), mp.data(), len.data(), n, (size_t)1 << 30, &shape, &err));
        size_t total = 0;
        for (size_t s = 0; s < n; s++) total += len[s];
        CHECK(shape.ld == ld && shape.T == 70 && T == 70 && shape.total == total && shape.any_mask);

        const double fill = -7.0;
        std::vector<double> yb(T * ld, fill);
        std::vector<uint8_t> vb(T * ld, 9);
        pack_time_major(yb.data(), ld, vp.data(), len.data(), n);
        pack_validity(vb.data(), ld, mp.data(), len.data(), n);
        const std::vector<int32_t> l32 = block_lengths(len.data(), n, ld);
        size_t nulls = 0;
        for (size_t t = 0; t < T; t++)
            for (size_t s = 0; s < ld; s++) {
                const bool inside = s < n && t < len[s];
                const double want_y = inside ? val[s][t] : fill;
                const uint8_t want_v = (inside && mp[s]) ? (uint8_t)((bits[s][t / 64] >> (t % 64)) & 1) : 9;
                if (yb[t * ld + s] != want_y || vb[t * ld + s] != want_v) { CHECK(!"packed cell"); t = T; break; }
                nulls += want_v == 0;
            }
        CHECK(nulls > 0 && vb[0 * ld + 4] == 0 && vb[63 * ld + 4] == 0 && vb[64 * ld + 4] == 0 && vb[62 * ld + 4] == 1 && vb[69 * ld + 5] == 9);
        for (size_t s = 0; s < ld; s++) CHECK(l32[s] == (s < n ? (int32_t)len[s] : 0));
        // without masks nothing is written; the kernels' int32 lengths pack the same cells
        std::vector<uint8_t> untouched(T * ld, 9);
        pack_validity(untouched.data(), ld, nullptr, len.data(), n);
        CHECK(untouched == std::vector<uint8_t>(T * ld, 9));
        std::vector<double> yb32(T * ld, fill);
        pack_time_major(yb32.data(), ld, vp.data(), l32.data(), n);
        CHECK(yb32 == yb);
        CHECK(valid_bit(bits[0].data(), 1) && !valid_bit(bits[0].data(), 63) && !valid_bit(bits[0].data(), 64) && valid_bit(bits[0].data(), 65));

        // ---- the shape function's refusals ---------------------------------------------------------------------------
        BlockShape kept = shape;
        vp[4] = nullptr;                                   // length 65 without values
        clear_error(&err);
        CHECK(!series_shape(vp.data(), mp.data(), len.data(), n, (size_t)1 << 30, &shape, &err));
        CHECK(err.code == NULL_POINTER && std::string(err.message) == "Null pointer argument");
        vp[4] = val[4].data();
        CHECK(vp[0] == nullptr && len[0] == 0);            // ... while a NULL series of length 0 was accepted above
        clear_error(&err);
        CHECK(!series_shape(vp.data(), mp.data(), len.data(), n, 69, &shape, &err));
        CHECK(err.code == INVALID_INPUT && std::string(err.message) == "Invalid input: a series is too long");
        CHECK(shape.ld == kept.ld && shape.T == kept.T && shape.total == kept.total);          // a refusal leaves the shape alone
        clear_error(&err);
        CHECK(series_shape(vp.data(), nullptr, len.data(), n, 70, &shape, &err) && err.code == SUCCESS && !shape.any_mask);
        CHECK(series_shape(nullptr, nullptr, nullptr, 0, SIZE_MAX, &shape, &err) && shape.ld == 0 && shape.T == 1 && shape.total == 0);
        // the block checks of a _device entry
        clear_error(&err);
        CHECK(!block_args_ok(64, 65, "n_groups", 1, 10, &err));
        CHECK(err.code == INVALID_INPUT && std::string(err.message) == "Invalid input: ld is smaller than n_groups");
        CHECK(!block_args_ok(128, 65, "n_series", 11, 10, &err));
        CHECK(err.code == INVALID_INPUT && std::string(err.message) == "Invalid input: the block is too large");
        CHECK(block_args_ok(128, 65, "n_series", 10, 10, &err));
    }

    // ---- nothing leaks ---------------------------------------------------------------------------------------------------
    dev_cache_release_all();
    {
        std::lock_guard<std::mutex> lock(F.mu);
        CHECK(F.dev_allocs.empty());
        for (auto &kv : F.used) CHECK(kv.second == 0);
    }
    CHECK(F.n_bad_free == 0 && F.n_malloc == F.n_free);
    if (failures) { std::fprintf(stderr, "%d check(s) failed\n", failures); return 1; }
    std::printf("scratch_san: ok (%ld hipMalloc, %ld hipFree, %ld refused, %ld device-wide waits)\n", (long)F.n_malloc, (long)F.n_free,
                (long)F.n_oom, (long)F.n_sync);
    return 0;
}
