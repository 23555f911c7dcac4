// reconcile_device.hpp -- what the kernels of reconcile.hip and reconcile_mint.hip share: the tile sizes and the guarded reads of a
// reconciliation plan (a plan that is not what the planner wrote yields empty ranges, never an address outside its arrays).
#pragma once
#include "kernels.hpp"

namespace anofox {

constexpr int RB = 64;                       // panel width of the factor and of the substitution; the edge of every 64 x 64 tile
constexpr int RP = RB + 1;                   // pitch of a 64 x 64 LDS tile read down a column
constexpr int RC = 32;                       // right-hand sides per workgroup of the substitution
constexpr int RK = 32;                       // K of one staging step of a symmetric update
constexpr int KP = RK + 1;                   // pitch of its staged tiles [row][k]: the stores run along k, the reads down the rows
constexpr unsigned REC_MAX_GRID_Y = 65535u;

typedef double rec_double4 __attribute__((ext_vector_type(4)));

// the member range of column c; an empty range when the offsets do not lie inside the plan
__device__ __forceinline__ void rec_column(const ReconcilePlan &p, int c, int &o0, int &o1)
{
    o0 = o1 = 0;
    if (c < 0 || c >= p.n_out) return;
    const int a = p.col_offsets[c], b = p.col_offsets[c + 1];
    if (a < 0 || b < a || b > p.nnz) return;
    o0 = a; o1 = b;
}

// the bottom column of member s, -1 when the plan is not what the planner wrote
__device__ __forceinline__ int rec_bottom_of(const ReconcilePlan &p, int s)
{
    if (s < 0 || s >= p.n_series) return -1;
    const int c = p.bottom_col[s];
    return (c < 0 || c >= p.n_out) ? -1 : c;
}

__device__ __forceinline__ void rec_leaf_range(const ReconcilePlan &p, int s, int &e0, int &e1)
{
    e0 = e1 = 0;
    if (s < 0 || s >= p.n_series) return;
    const int a = p.leaf_offsets[s], b = p.leaf_offsets[s + 1];
    if (a < 0 || b < a || b > p.n_leaf) return;
    e0 = a; e1 = b;
}

} // namespace anofox
