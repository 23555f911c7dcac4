// host_period_search.hpp -- the host-only logic of the period-search entries (ssa_period / stl_period): how
// the arguments resolve to the source's defaults, the effective SSA window, where the lag-covariance matrix lives, the STL candidate
// list, and the argument checks that come before the device is touched, each with a text that names its limit.  Plain C++ without
// HIP: host_api.hip includes it inside its anonymous namespace, period_search.hip uses its constexpr rules in the kernels, and
// tests/c_abi/period_search_san.cpp compiles THIS file on its own and runs it under ASan + UBSan.
#pragma once

enum PSearchCheck { PSEARCH_CHECK_OK = 0, PSEARCH_CHECK_NULL = 1, PSEARCH_CHECK_INVALID = 2 };

constexpr size_t PSEARCH_HOST_MAX_ROWS = 65536;                 // (= PSEARCH_MAX_ROWS of kernels.hpp)
constexpr size_t PSEARCH_HOST_MAX_COMPONENTS = 32;              // (= SSA_MAX_COMPONENTS)
constexpr size_t PSEARCH_HOST_MAX_CANDIDATES = 64;              // (= STL_MAX_CANDIDATES)
constexpr int64_t PSEARCH_HOST_MAX_WINDOW = 2048;               // (= SSA_MAX_WINDOW)
constexpr int64_t PSEARCH_HOST_TILE = 2048;                     // (= PSEARCH_TILE)
constexpr int64_t PSEARCH_HOST_LDS_DOUBLES = 7936;              // (= PSEARCH_LDS_DOUBLES)
constexpr int64_t PSEARCH_HOST_ARG_CAP = (int64_t)1 << 40;      // a size_t argument beyond it acts like any value beyond a series' length
constexpr int PSEARCH_HOST_STL_WAVES = 4;                       // (= STL_WAVES)

// a size_t argument of the reference's wrappers as the kernels take it: 0 stays the default, everything else is positive
constexpr int64_t psearch_arg(uint64_t v) { return v > (uint64_t)PSEARCH_HOST_ARG_CAP ? PSEARCH_HOST_ARG_CAP : (int64_t)v; }

// ssa_period: l = window_size.unwrap_or(n / 3).min(n / 2).max(4); `window` 0 is None
constexpr int64_t ssa_window(int64_t n, int64_t window)
{
    int64_t l = window > 0 ? window : n / 3;
    if (l > n / 2) l = n / 2;
    if (l < 4) l = 4;
    return l;
}

// the LDS pool of an SSA workgroup of 256 lanes holds the three iteration vectors, the series when it has at most 2,048 rows, and the
// matrix when the rest has room for it; otherwise the matrix lives in the workgroup's slice of the global workspace
constexpr bool ssa_series_in_lds(int64_t n) { return n <= PSEARCH_HOST_TILE; }
constexpr bool ssa_matrix_in_lds(int64_t n, int64_t l)
{
    return l * l + 3 * l + (ssa_series_in_lds(n) ? n : 0) <= PSEARCH_HOST_LDS_DOUBLES;
}

// stl_period keeps per wave the rows `current` and `trend` and the phase table (at most n / 2 entries), beside the series itself
constexpr int64_t stl_wave_doubles(int64_t n) { return 2 * n + n / 2; }
constexpr bool stl_series_in_lds(int64_t n) { return n <= PSEARCH_HOST_TILE; }
constexpr bool stl_rows_in_lds(int64_t n)
{
    return PSEARCH_HOST_STL_WAVES * stl_wave_doubles(n) + (stl_series_in_lds(n) ? n : 0) <= PSEARCH_HOST_LDS_DOUBLES;
}

inline int ssa_components(size_t n_components) { return n_components > 0 ? (int)n_components : 10; }                 // unwrap_or(10)
inline int stl_candidate_count(size_t n_candidates) { const size_t c = n_candidates > 0 ? n_candidates : 20; return (int)(c < 5 ? 5 : c); }

inline PSearchCheck ssa_args_check(size_t t_rows, size_t n_components, std::string *message)
{
    auto invalid = [&](const std::string &text) { *message = "Invalid input: " + text; return PSEARCH_CHECK_INVALID; };
    if (n_components > PSEARCH_HOST_MAX_COMPONENTS)
        return invalid("n_components " + std::to_string(n_components) + " exceeds the limit of " + std::to_string(PSEARCH_HOST_MAX_COMPONENTS) +
                       " components per call");
    if (t_rows > PSEARCH_HOST_MAX_ROWS)
        return invalid("t_rows " + std::to_string(t_rows) + " exceeds the limit of " + std::to_string(PSEARCH_HOST_MAX_ROWS) + " rows per series");
    return PSEARCH_CHECK_OK;
}

inline PSearchCheck stl_args_check(size_t t_rows, size_t n_candidates, std::string *message)
{
    auto invalid = [&](const std::string &text) { *message = "Invalid input: " + text; return PSEARCH_CHECK_INVALID; };
    if (n_candidates > PSEARCH_HOST_MAX_CANDIDATES)
        return invalid("n_candidates " + std::to_string(n_candidates) + " exceeds the limit of " + std::to_string(PSEARCH_HOST_MAX_CANDIDATES) +
                       " candidates per call");
    if (t_rows > PSEARCH_HOST_MAX_ROWS)
        return invalid("t_rows " + std::to_string(t_rows) + " exceeds the limit of " + std::to_string(PSEARCH_HOST_MAX_ROWS) + " rows per series");
    return PSEARCH_CHECK_OK;
}

// the longest series of a batch call, checked against the row limit (the batch entries have no t_rows argument)
inline PSearchCheck psearch_batch_rows(const size_t *lengths, size_t n_series, size_t *rows, std::string *message)
{
    if (!rows || (n_series > 0 && !lengths)) return PSEARCH_CHECK_NULL;
    size_t longest = 0;
    for (size_t s = 0; s < n_series; s++) longest = lengths[s] > longest ? lengths[s] : longest;
    *rows = longest;
    if (longest > PSEARCH_HOST_MAX_ROWS) {
        *message = "Invalid input: a series of " + std::to_string(longest) + " rows exceeds the limit of " + std::to_string(PSEARCH_HOST_MAX_ROWS) +
                   " rows per series";
        return PSEARCH_CHECK_INVALID;
    }
    return PSEARCH_CHECK_OK;
}

// stl_period's candidate list of a series of n >= 16 rows (`min_period` / `max_period` 0 are None): 0 and the ascending list, or
// 3 (min_period must be less than max_period) or 4 (no valid candidate), the statuses of the device entry
inline int stl_candidates(int64_t n, int64_t min_period, int64_t max_period, int n_cand, std::vector<int> *out)
{
    out->clear();
    int64_t min_p = min_period > 0 ? min_period : 4;
    if (min_p < 2) min_p = 2;
    int64_t max_p = max_period > 0 ? max_period : n / 3;
    if (max_p > n / 2) max_p = n / 2;
    if (min_p >= max_p) return 3;
    double step = (double)(max_p - min_p) / (double)n_cand;
    if (!(step >= 1.0)) step = 1.0;                             // f64::max(1.0)
    int64_t last = -1;
    for (int i = 0; i < n_cand; i++) {
        const double x = (double)min_p + (double)i * step;
        const double f = std::floor(x);
        const int64_t p = (int64_t)f + (x - f >= 0.5 ? 1 : 0);  // f64::round of a positive value: halves away from zero
        if (p >= min_p && p <= max_p && p >= 2 && n >= 2 * p && p != last) {      // (the values never decrease, so equal ones are neighbours)
            out->push_back((int)p);
            last = p;
        }
    }
    return out->empty() ? 4 : 0;
}

inline std::string psearch_series_error(int32_t status, size_t n, int64_t window)
{
    if (status == 1) return "Insufficient data: need at least 16 observations, got " + std::to_string(n);
    if (status == 2)
        return "SSA: the window of " + std::to_string((long long)ssa_window((int64_t)n, window)) + " rows of a series of " + std::to_string(n) +
               " observations exceeds the limit of " + std::to_string((long long)PSEARCH_HOST_MAX_WINDOW) + " of the HIP backend";
    if (status == 3) return "Invalid input: min_period must be less than max_period";
    return "Invalid input: No valid candidate periods found";
}
