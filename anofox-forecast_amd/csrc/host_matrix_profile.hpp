// host_matrix_profile.hpp -- the host-only logic of the matrix-profile period entries (matrix_profile_period):
// how the arguments resolve to the source's defaults (the subsequence length m, the exclusion zone), how long a profile is, where a
// series' arrays live, the workspace size, the tile walk, and the argument checks that come before the device is touched, each with
// a text that names its limit.  Plain C++ without HIP: host_api.hip includes it inside its anonymous namespace, matrix_profile.hip
// uses its constexpr rules in the kernel, and tests/c_abi/matrix_profile_san.cpp compiles THIS file on its own and runs it under
// ASan + UBSan.
//
// The source's second check (a profile shorter than 10 gives "Insufficient data: need at least m + 10") cannot be reached: with
// n >= 32 and m <= n / 4 the profile has n - m + 1 >= 25 entries.  There is no status and no text for it.
#pragma once

enum MProfCheck { MPROF_CHECK_OK = 0, MPROF_CHECK_NULL = 1, MPROF_CHECK_INVALID = 2 };

constexpr size_t MPROF_HOST_MAX_ROWS = 65536;                   // (= MPROF_MAX_ROWS of kernels.hpp)
constexpr int64_t MPROF_HOST_MIN_ROWS = 32;                     // (= MPROF_MIN_ROWS)
constexpr int64_t MPROF_HOST_MAX_M = 2048;                      // (= MPROF_MAX_M)
constexpr int64_t MPROF_HOST_TILE = 64;                         // (= MPROF_TILE)
constexpr int64_t MPROF_HOST_KCHUNK = 16;                       // (= MPROF_KCHUNK)
constexpr int64_t MPROF_HOST_HOME_DOUBLES = 5504;               // (= MPROF_HOME_DOUBLES)
constexpr size_t MPROF_HOST_WORK_BYTES = (size_t)256 << 20;     // (= MPROF_WORK_BYTES)
constexpr int MPROF_HOST_MAX_BLOCKS = 512;                      // persistent workgroups of a launch: two for each of the 256 compute units
constexpr int64_t MPROF_HOST_ARG_CAP = (int64_t)1 << 40;        // a size_t argument beyond it acts like any value beyond a series' length

// a size_t argument of the reference's wrapper as the kernel takes it: 0 stays the default, everything else is positive
constexpr int64_t mprof_arg(uint64_t v) { return v > (uint64_t)MPROF_HOST_ARG_CAP ? MPROF_HOST_ARG_CAP : (int64_t)v; }

// m = subsequence_length.unwrap_or(n / 10).max(4).min(n / 4); `subsequence` 0 is None
constexpr int64_t mprof_subsequence(int64_t n, int64_t subsequence)
{
    int64_t m = subsequence > 0 ? subsequence : n / 10;
    if (m < 4) m = 4;
    if (m > n / 4) m = n / 4;
    return m;
}

// exclusion = exclusion_zone.unwrap_or(m / 4).max(1); the wrapper passes n_best on as the exclusion zone, `n_best` 0 is None
constexpr int64_t mprof_exclusion(int64_t m, int64_t n_best)
{
    const int64_t e = n_best > 0 ? n_best : m / 4;
    return e < 1 ? 1 : e;
}

// the number of subsequences P = n - m + 1 of a series that is long enough (never below 25), else 0; it never falls as n grows
constexpr int64_t mprof_profile_len(int64_t n, int64_t subsequence)
{
    return n < MPROF_HOST_MIN_ROWS ? 0 : n - mprof_subsequence(n, subsequence) + 1;
}

// a series (n doubles; the lag histogram of n / 2 counts takes its place once the profile is complete), its profile (P doubles) and
// its index (P int32) live in LDS while they fit into MPROF_HOME_DOUBLES, else in the workgroup's slice of the workspace.  With the
// default m = n / 10 the boundary is n = 2,341 rows; with a forced m = 4 it is n = 2,203.
constexpr int64_t mprof_home_doubles(int64_t n, int64_t p) { return n + p + (p + 1) / 2; }
constexpr bool mprof_in_lds(int64_t n, int64_t subsequence)
{
    return mprof_home_doubles(n, mprof_profile_len(n, subsequence)) <= MPROF_HOST_HOME_DOUBLES;
}

// a workspace slice: the means and stds of every subsequence always (2 t_rows), and when a series of t_rows rows does not fit in LDS
// the series, the profile, the index and the histogram as well
constexpr size_t mprof_work_stride(size_t t_rows, int64_t subsequence)
{
    return 2 * t_rows + (mprof_in_lds((int64_t)t_rows, subsequence) ? 0 : 2 * t_rows + (t_rows + 1) / 2 + (t_rows / 2 + 2) / 2);
}

// the slices of a call: bounded by MPROF_WORK_BYTES whatever n_series is (one slice where a single one is larger), never more than
// the persistent workgroups of a launch
inline int mprof_work_blocks(size_t work_stride, size_t n_series)
{
    if (!work_stride || !n_series) return 0;
    size_t blocks = MPROF_HOST_WORK_BYTES / (work_stride * sizeof(double));
    if (blocks < 1) blocks = 1;
    if (blocks > (size_t)MPROF_HOST_MAX_BLOCKS) blocks = (size_t)MPROF_HOST_MAX_BLOCKS;
    if (blocks > n_series) blocks = n_series;
    return (int)blocks;
}

// the tile walk: row tile r covers i in [64 r, 64 r + 64); its first column tile is the first that holds a pair with j - i >= excl
// (j0 + 63 - i0 >= excl), and the walk goes on to the last tile of the profile
constexpr int64_t mprof_tiles(int64_t p) { return (p + MPROF_HOST_TILE - 1) / MPROF_HOST_TILE; }
constexpr int64_t mprof_first_col_tile(int64_t row_tile, int64_t excl)
{
    const int64_t need = row_tile * MPROF_HOST_TILE + excl - (MPROF_HOST_TILE - 1);      // the smallest admissible j0
    return need <= 0 ? 0 : (need + MPROF_HOST_TILE - 1) / MPROF_HOST_TILE;
}
inline int64_t mprof_tile_count(int64_t p, int64_t excl)
{
    const int64_t t = mprof_tiles(p);
    int64_t count = 0;
    for (int64_t r = 0; r < t; r++) {
        const int64_t first = mprof_first_col_tile(r, excl);
        if (first < t) count += t - first;
    }
    return count;
}
constexpr int64_t mprof_k_chunks(int64_t m) { return (m + MPROF_HOST_KCHUNK - 1) / MPROF_HOST_KCHUNK; }

inline MProfCheck mprof_args_check(size_t t_rows, std::string *message)
{
    if (t_rows > MPROF_HOST_MAX_ROWS) {
        *message = "Invalid input: t_rows " + std::to_string(t_rows) + " exceeds the limit of " + std::to_string(MPROF_HOST_MAX_ROWS) + " rows per series";
        return MPROF_CHECK_INVALID;
    }
    return MPROF_CHECK_OK;
}

// the longest series of a batch call, checked against the row limit (the batch entry has no t_rows argument)
inline MProfCheck mprof_batch_rows(const size_t *lengths, size_t n_series, size_t *rows, std::string *message)
{
    if (!rows || (n_series > 0 && !lengths)) return MPROF_CHECK_NULL;
    size_t longest = 0;
    for (size_t s = 0; s < n_series; s++) longest = lengths[s] > longest ? lengths[s] : longest;
    *rows = longest;
    if (longest > MPROF_HOST_MAX_ROWS) {
        *message = "Invalid input: a series of " + std::to_string(longest) + " rows exceeds the limit of " + std::to_string(MPROF_HOST_MAX_ROWS) +
                   " rows per series";
        return MPROF_CHECK_INVALID;
    }
    return MPROF_CHECK_OK;
}

inline std::string mprof_series_error(int32_t status, size_t n, int64_t subsequence)
{
    if (status == 1) return "Insufficient data: need at least 32 observations, got " + std::to_string(n);
    return "Matrix profile: the subsequence length of " + std::to_string((long long)mprof_subsequence((int64_t)n, subsequence)) +
           " rows of a series of " + std::to_string(n) + " observations exceeds the limit of " + std::to_string((long long)MPROF_HOST_MAX_M) +
           " of the HIP backend";
}
