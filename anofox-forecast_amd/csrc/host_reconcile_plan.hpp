// host_reconcile_plan.hpp -- the host-only planner of the reconciliation entries: from an aggregation plan (col_offsets / members as
// anofox_hip_hierarchy_plan returns them) the bottom column of every series, the aggregate columns, the transposed plan (for each
// series the aggregates that hold it) and the structural weights.  Plain C++ without HIP: host_api.hip includes it inside its
// anonymous namespace, and tests/c_abi/reconcile_san.cpp compiles THIS file on its own and runs it under ASan + UBSan.
#pragma once

enum ReconcilePlanResult { RECONCILE_PLAN_OK = 0, RECONCILE_PLAN_NULL = 1, RECONCILE_PLAN_INVALID = 2 };

// A column whose member list is exactly [s] is the bottom column of s; every other column with members is an aggregate.  *n_agg and
// *n_leaf are written once the plan is known to be well formed; the arrays only when bottom_col is not null.  `message` names what
// RECONCILE_PLAN_INVALID found.
inline ReconcilePlanResult reconcile_plan_host(const int32_t *col_offsets, const int32_t *members, size_t n_out, size_t n_series, size_t max_agg,
                                               size_t *n_agg, size_t *n_leaf, int32_t *bottom_col, int32_t *agg_cols, int32_t *leaf_offsets,
                                               int32_t *leaf_aggs, double *struct_weights, std::string *message)
{
    auto invalid = [&](const std::string &text) { *message = "Invalid input: " + text; return RECONCILE_PLAN_INVALID; };
    if (n_out > (size_t)INT32_MAX || n_series > (size_t)INT32_MAX) return invalid("n_out and n_series are limited to 2^31 - 1");
    if (n_out > 0 && !col_offsets) return RECONCILE_PLAN_NULL;
    if (!bottom_col && (agg_cols || leaf_offsets || leaf_aggs || struct_weights)) return RECONCILE_PLAN_NULL;
    if (n_out > 0 && col_offsets[0] != 0) return invalid("col_offsets does not start at 0");
    for (size_t c = 0; c < n_out; c++)
        if (col_offsets[c + 1] < col_offsets[c]) return invalid("col_offsets descends at column " + std::to_string(c));
    const size_t nnz = n_out ? (size_t)col_offsets[n_out] : 0;
    if (nnz > 0 && !members) return RECONCILE_PLAN_NULL;
    for (size_t k = 0; k < nnz; k++)
        if (members[k] < 0 || (size_t)members[k] >= n_series)
            return invalid("plan entry " + std::to_string(k) + " names series " + std::to_string(members[k]) + ", outside [0, " +
                           std::to_string(n_series) + ")");
    std::vector<int32_t> bottom(n_series, -1);
    for (size_t c = 0; c < n_out; c++) {
        if (col_offsets[c + 1] - col_offsets[c] != 1) continue;
        const size_t s = (size_t)members[col_offsets[c]];
        if (bottom[s] >= 0)
            return invalid("series " + std::to_string(s) + " has two bottom columns, " + std::to_string(bottom[s]) + " and " + std::to_string(c));
        bottom[s] = (int32_t)c;
    }
    for (size_t s = 0; s < n_series; s++)
        if (bottom[s] < 0) return invalid("series " + std::to_string(s) + " has no bottom column (a column whose only member it is)");
    auto takes_part = [&](size_t c) { return col_offsets[c + 1] - col_offsets[c] > 1; };      // (a column of one member is a bottom column here)
    size_t na = 0, nl = 0;
    for (size_t c = 0; c < n_out; c++)
        if (takes_part(c)) { na++; nl += (size_t)(col_offsets[c + 1] - col_offsets[c]); }
    if (n_agg) *n_agg = na;
    if (n_leaf) *n_leaf = nl;
    if (na > max_agg)
        return invalid("n_agg " + std::to_string(na) + " exceeds the limit of " + std::to_string(max_agg) + " aggregate columns");
    if (!bottom_col) return RECONCILE_PLAN_OK;
    if ((na > 0 && !agg_cols) || !leaf_offsets || (nl > 0 && !leaf_aggs)) return RECONCILE_PLAN_NULL;
    if (n_series) std::memcpy(bottom_col, bottom.data(), n_series * sizeof(int32_t));
    // the transpose: a counting sort by series; the aggregates are visited in ascending order, so every list ascends
    std::vector<int32_t> at(n_series + 1, 0);
    size_t i = 0;
    for (size_t c = 0; c < n_out; c++) {
        if (struct_weights) struct_weights[c] = (double)(col_offsets[c + 1] - col_offsets[c]);
        if (!takes_part(c)) continue;
        agg_cols[i++] = (int32_t)c;
        for (int32_t k = col_offsets[c]; k < col_offsets[c + 1]; k++) at[(size_t)members[k] + 1]++;
    }
    for (size_t s = 0; s < n_series; s++) at[s + 1] += at[s];
    std::memcpy(leaf_offsets, at.data(), (n_series + 1) * sizeof(int32_t));
    for (size_t a = 0; a < na; a++) {
        const int32_t c = agg_cols[a];
        for (int32_t k = col_offsets[c]; k < col_offsets[c + 1]; k++) leaf_aggs[at[(size_t)members[k]]++] = (int32_t)a;
    }
    return RECONCILE_PLAN_OK;
}
