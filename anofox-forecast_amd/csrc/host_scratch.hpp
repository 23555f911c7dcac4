// host_scratch.hpp -- what every entry family of the host layer shares around its kernels: the owner of a call's device scratch,
// the shape and the time-major packing of a batch of host series, and the block checks and the launch sequence of a _device entry.
// Included by host_api.hip INSIDE its anonymous namespace, right after host_resources.hpp (HipFail, HIPCHECK, LAUNCHCHECK, dalloc,
// dev_free).  It calls nothing of the HIP API that tests/c_abi/fake_hip.h does not provide: tests/c_abi/scratch_san.cpp compiles
// THIS file against that stand-in and runs the paths no GPU test reaches (an allocation refused half way, a failure thrown through
// the owner) under ASan + UBSan.
#pragma once

// The device blocks of one call.  Whatever way the call ends -- a return, an early `return false`, a HipFail on its way to the
// entry's handler -- every block goes back to the allocator, so a block can no longer be missing from a hand-kept list.
//
// Why ONE wait is enough: a block may only return to the cache once no kernel or copy can still touch it.  An entry that has
// synchronised its stream (and whose copies are synchronous) says so with settled(), and nothing waits.  Otherwise nobody knows
// what is in flight, and the first free synchronises the whole device; after that wait nothing of this call is in flight any
// more, and the call itself enqueues nothing further, so the other blocks need no second wait.
class Scratch {
    std::vector<void *> blocks;
    bool quiesced = false;

public:
    Scratch() = default;
    Scratch(const Scratch &) = delete;
    Scratch &operator=(const Scratch &) = delete;
    ~Scratch()
    {
        for (void *p : blocks) {
            dev_free(p, quiesced);
            quiesced = true;
        }
    }
    template <class T> T *get(size_t n)
    {
        blocks.reserve(blocks.size() + 1);                 // (so that the block is on the list once it exists)
        blocks.push_back(dalloc<T>(n));
        return (T *)blocks.back();
    }
    void settled() { quiesced = true; }
};

// ---- a batch of host series -> one time-major block ----

inline bool valid_bit(const uint64_t *mask, size_t t) { return (mask[t >> 6] >> (t & 63)) & 1; }       // DuckDB's validity mask

struct BlockShape {
    size_t ld = 0;             // columns of the block: n_series rounded up to whole waves
    size_t T = 1;              // rows: the longest series, at least 1
    size_t total = 0;          // values in all series together
    bool any_mask = false;     // some series with values has a validity mask
};

// The per-series argument loop of a _batch entry: values[s] may be NULL only where lengths[s] is 0, and no series is longer than
// max_len.  (An entry without a limit passes SIZE_MAX; one without masks passes validity = NULL.)
inline bool series_shape(const double *const *values, const uint64_t *const *validity, const size_t *lengths, size_t n_series, size_t max_len,
                         BlockShape *shape, AnofoxError *err)
{
    BlockShape b;
    size_t t_max = 0;
    for (size_t s = 0; s < n_series; s++) {
        if (lengths[s] > 0 && !values[s]) { set_error(err, NULL_POINTER, "Null pointer argument"); return false; }
        if (lengths[s] > max_len) { set_error(err, INVALID_INPUT, "Invalid input: a series is too long"); return false; }
        b.total += lengths[s];
        t_max = std::max(t_max, lengths[s]);
        b.any_mask = b.any_mask || (validity && validity[s] && lengths[s] > 0);
    }
    b.ld = (n_series + 63) / 64 * 64;
    b.T = std::max<size_t>(t_max, 1);
    *shape = b;
    return true;
}

// the lengths as the kernels take them: one int32 per column, 0 in the padding columns
inline std::vector<int32_t> block_lengths(const size_t *lengths, size_t n_series, size_t ld)
{
    std::vector<int32_t> len(ld, 0);
    for (size_t s = 0; s < n_series; s++) len[s] = (int32_t)lengths[s];
    return len;
}

// series s, step t -> block[t * ld + s]; the caller has filled the block: cells past a series' length and the column of a NULL
// series (dates are optional per series) keep that fill
template <class T, class Length> void pack_time_major(T *block, size_t ld, const T *const *series, const Length *lengths, size_t n_series)
{
    for (size_t s = 0; s < n_series; s++) {
        const T *v = series[s];
        if (!v) continue;
        for (size_t t = 0; t < (size_t)lengths[s]; t++) block[t * ld + s] = v[t];
    }
}

// the same cells for the validity bits, one byte each; a series without a mask (or masks == NULL) keeps the fill
inline void pack_validity(uint8_t *block, size_t ld, const uint64_t *const *masks, const size_t *lengths, size_t n_series)
{
    if (!masks) return;
    for (size_t s = 0; s < n_series; s++) {
        const uint64_t *m = masks[s];
        if (!m) continue;
        for (size_t t = 0; t < lengths[s]; t++) block[t * ld + s] = (uint8_t)valid_bit(m, t);
    }
}

// ---- a _device entry ----

// the block arguments: `columns` names n_cols in the message ("n_series", "n_groups"), t_limit is the kernel's row limit
inline bool block_args_ok(size_t ld, size_t n_cols, const char *columns, size_t t_rows, size_t t_limit, AnofoxError *err)
{
    if (ld < n_cols) { set_error(err, INVALID_INPUT, std::string("Invalid input: ld is smaller than ") + columns); return false; }
    if (n_cols > (size_t)INT32_MAX || t_rows > t_limit) {
        set_error(err, INVALID_INPUT, "Invalid input: the block is too large");
        return false;
    }
    return true;
}

// Runs `launch` (the entry's scratch allocations and its kernel launches on `st`) and waits for the stream: true once the results
// are in place.  The sticky error of an earlier call is dropped first, so that the check after the launch reports this launch.
// (Stream is a template parameter only so that this header also compiles against a runtime stand-in without stream calls.)
template <class Stream, class Launch> bool launch_and_wait(const char *what, Stream st, AnofoxError *err, Launch &&launch)
{
    try {
        (void)hipGetLastError();
        launch();
        LAUNCHCHECK(what);
        HIPCHECK(hipStreamSynchronize(st));
    } catch (const HipFail &f) {
        report_hip_failure(err, f);
        return false;
    }
    return true;
}
