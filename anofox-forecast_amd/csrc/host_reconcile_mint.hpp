// host_reconcile_mint.hpp -- the host-only logic of the MinT-shrink entries (DESIGN.md section 3 "MinT-shrink"): the argument checks
// that come before the device is touched, each with a text that names what it found, and the sizes of the workspaces.  Plain C++
// without HIP: host_api.hip includes it inside its anonymous namespace, and tests/c_abi/reconcile_mint_san.cpp compiles THIS file on
// its own and runs it under ASan + UBSan.
#pragma once

enum ReconcileMintResult { RECONCILE_MINT_OK = 0, RECONCILE_MINT_NULL = 1, RECONCILE_MINT_INVALID = 2 };

constexpr size_t RECONCILE_MINT_MAX_RESIDUAL_ROWS = 8192;   // (= ANOFOX_HIP_RECONCILE_MAX_RESIDUAL_ROWS: one n_res x n_res plane is 512 MiB)
constexpr size_t RECONCILE_MINT_TILE = 64;                  // the edge of a Gram tile (RB of reconcile_device.hpp)
constexpr size_t RECONCILE_MINT_MAX_SPLITS = 64;            // slices of the Gram's inner dimension
constexpr size_t RECONCILE_MINT_TARGET_GROUPS = 2048;       // workgroups the Gram launch aims at

inline size_t reconcile_mint_gram_tiles(size_t n_res)
{
    const size_t nt = (n_res + RECONCILE_MINT_TILE - 1) / RECONCILE_MINT_TILE;
    return nt * (nt + 1) / 2;
}

// The inner dimension of the Gram product is cut into this many slices, so that a short residual block still fills the device.  A
// function of n_res alone: the workspace can be sized without a plan, and the same block gives the same bits through every entry.
inline size_t reconcile_mint_gram_splits(size_t n_res)
{
    const size_t tiles = reconcile_mint_gram_tiles(n_res);
    if (tiles == 0) return 1;
    const size_t s = (RECONCILE_MINT_TARGET_GROUPS + tiles - 1) / tiles;
    return s < 1 ? 1 : s > RECONCILE_MINT_MAX_SPLITS ? RECONCILE_MINT_MAX_SPLITS : s;
}

// doubles of the Gram workspace: one n_res x n_res plane per slice, then two partial sums per tile of the lower triangle
inline size_t reconcile_mint_gram_elems(size_t n_res)
{
    return reconcile_mint_gram_splits(n_res) * n_res * n_res + 2 * reconcile_mint_gram_tiles(n_res);
}

inline ReconcileMintResult reconcile_mint_rows_check(size_t n_res, std::string *message)
{
    auto invalid = [&](const std::string &text) { *message = "Invalid input: " + text; return RECONCILE_MINT_INVALID; };
    if (n_res < 2) return invalid("n_res is " + std::to_string(n_res) + ", a variance and a shrinkage intensity need at least 2 residual rows");
    if (n_res > RECONCILE_MINT_MAX_RESIDUAL_ROWS)
        return invalid("n_res " + std::to_string(n_res) + " exceeds the limit of " + std::to_string(RECONCILE_MINT_MAX_RESIDUAL_ROWS) + " residual rows");
    return RECONCILE_MINT_OK;
}

// a passed intensity; NaN asks for the estimate where `may_estimate`
inline ReconcileMintResult reconcile_mint_lambda_check(double lambda, bool may_estimate, bool *estimate, std::string *message)
{
    auto invalid = [&](const std::string &text) { *message = "Invalid input: " + text; return RECONCILE_MINT_INVALID; };
    const bool nan = lambda != lambda;
    if (estimate) *estimate = nan;
    if (nan) return may_estimate ? RECONCILE_MINT_OK : invalid("the shrinkage intensity is NaN: the apply takes the value the factor call returned");
    if (!(lambda >= 0.0 && lambda <= 1.0)) return invalid("the shrinkage intensity " + std::to_string(lambda) + " lies outside [0, 1]");
    return RECONCILE_MINT_OK;
}

// the leading dimensions and the participating columns of the device entries
inline ReconcileMintResult reconcile_mint_dims_check(size_t n_series, size_t n_agg, size_t max_agg, size_t ld_e, size_t ld_a, std::string *message)
{
    auto invalid = [&](const std::string &text) { *message = "Invalid input: " + text; return RECONCILE_MINT_INVALID; };
    if (n_agg > max_agg) return invalid("n_agg " + std::to_string(n_agg) + " exceeds the limit of " + std::to_string(max_agg) + " aggregate columns");
    if (n_series > (size_t)INT32_MAX - n_agg) return invalid("n_series + n_agg, the participating columns, are limited to 2^31 - 1");
    if (ld_e < n_agg) return invalid("ld_e is smaller than n_agg");
    if (ld_a < n_agg) return invalid("ld_a is smaller than n_agg");
    return RECONCILE_MINT_OK;
}

// Element counts (doubles) of what a caller of the device entries allocates: the Gram workspace of the factor call (not needed when
// the intensity is passed in), E [n_res x n_agg], the factor [n_agg x n_agg], the work area of the apply [n_rows x (n_agg + n_res)].
inline ReconcileMintResult reconcile_mint_sizes_host(size_t n_res, size_t n_agg, size_t n_rows, size_t max_agg, size_t *gram_elems, size_t *e_elems,
                                                     size_t *factor_elems, size_t *work_elems, std::string *message)
{
    auto invalid = [&](const std::string &text) { *message = "Invalid input: " + text; return RECONCILE_MINT_INVALID; };
    if (!gram_elems || !e_elems || !factor_elems || !work_elems) return RECONCILE_MINT_NULL;
    const ReconcileMintResult r = reconcile_mint_rows_check(n_res, message);
    if (r != RECONCILE_MINT_OK) return r;
    if (n_agg > max_agg) return invalid("n_agg " + std::to_string(n_agg) + " exceeds the limit of " + std::to_string(max_agg) + " aggregate columns");
    if (n_rows > (size_t)INT32_MAX) return invalid("n_rows is limited to 2^31 - 1");
    *gram_elems = reconcile_mint_gram_elems(n_res);
    *e_elems = n_res * n_agg;
    *factor_elems = n_agg * n_agg;
    *work_elems = n_rows * (n_agg + n_res);
    return RECONCILE_MINT_OK;
}
