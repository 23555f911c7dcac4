// hierarchy.hip -- ts_aggregate_hierarchy (ts_aggregate_hierarchy.cpp:246-386) on a resident time-major block.  The operator adds
// every row's value to one cell (unique_id, date) per level, `aggregations[unique_id][date] += value`, in the order the rows arrive:
// a cell is ((0.0 + v_a) + v_b) + ... over its rows in table order.  Here the rows are the block's cells: series s holds consecutive
// positions first[s] .. first[s] + len[s] - 1 of a common date grid, and output column c is the sum over the series
// members[col_offsets[c] .. col_offsets[c + 1]) -- a CSR plan whose member order IS the order of the additions.  The contract is
// equality of bits with that chain: every cell is one serial sum from +0.0 in member order, nothing is reordered, no level is built
// from another level's sums (-ffp-contract=off, no fast-math: the compiler may not reassociate either).
//
//   hier_span_kernel   one wavefront per column: the smallest and the largest grid position at which a member has a row (a row
//                      exists where `present` is non-zero; without the mask every row of the series exists) -> first_out, len_out.
//                      A column without a row has length 0.  A column that cannot be computed -- offsets outside the plan, a member
//                      outside [0, n_series), |first| above 2^61, a span above 2^30 rows -- has length -1 and is written as an empty
//                      column by the two routes: the marker is the report, the device entry does not wait on the host.
//   hier_lane_kernel   lane per output column (narrow columns).  A lane keeps HL_ROWS running sums in registers and walks its members
//                      once per row tile: one load of (member, first, len) per member and tile, HL_ROWS additions.  Neighbouring lanes
//                      are neighbouring columns: the stores are coalesced, and with a key-sorted block neighbouring leaf columns read
//                      neighbouring series.
//   hier_tile_kernel   wide columns: one wavefront owns (column, 64 grid rows).  Per 64 members it stages a tile of 64 rows x 64 members
//                      in LDS with lanes over MEMBERS on the load (members that are consecutive series with equal `first` make that a
//                      512-byte contiguous read per row; anything else is a gather; the loads are unconditional, to clamped
//                      addresses, 32 rows in flight at a time), then lane <-> row walks the tile's members in order and
//                      carries the running sum to the next tile in a register.  A tile row is 65 doubles long: with that odd
//                      pitch the stores (lanes along a row) and the loads (lanes down a column) both touch 32 distinct bank pairs per
//                      half wave, as metrics.hip does for series-major blocks.  A member without a row at a position stages +0.0: the
//                      running sum can never be -0.0 (it starts at +0.0, and x + y is -0.0 only when both are), so adding +0.0
//                      leaves every bit as it is, and the chain needs no branch.
// Both routes give the same bits: HierarchyArgs::route forces either, HIER_ROUTE_AUTO sends columns with at least `tile_min` members
// to the tile route.
#include "kernels.hpp"

namespace anofox {

namespace {

constexpr int HL_COLS = 256;                 // columns (threads) per workgroup of the lane route
constexpr int HL_ROWS = 16;                  // rows per tile of the lane route: the running sums a lane keeps in registers
constexpr int HT = 64;                       // the tile route's tile: HT rows x HT members
constexpr int HT_PITCH = HT + 1;
constexpr unsigned HIER_MAX_GRID_Y = 65535u;

__device__ __forceinline__ int hier_length(const HierarchyArgs &a, int s)
{
    int n = a.len[s];
    if (n < 0) n = 0;
    if ((size_t)n > a.t_rows) n = (int)a.t_rows;
    return n;
}

// the member range of column c; false (and an empty range) when the offsets do not lie inside the plan
__device__ __forceinline__ bool hier_column(const HierarchyArgs &a, int c, int &o0, int &o1)
{
    o0 = a.col_offsets[c];
    o1 = a.col_offsets[c + 1];
    if (o0 < 0 || o1 < o0 || o1 > a.nnz) { o0 = o1 = 0; return false; }
    return true;
}

__device__ __forceinline__ bool hier_takes_tile(const HierarchyArgs &a, int width)
{
    return a.route == HIER_ROUTE_TILE || (a.route == HIER_ROUTE_AUTO && width >= a.tile_min);
}

// rows of column c that the routes compute: len_out cut to [0, t_out]
__device__ __forceinline__ size_t hier_rows(const HierarchyArgs &a, int c)
{
    const int L = a.len_out[c];
    if (L <= 0) return 0;
    return (size_t)L < a.t_out ? (size_t)L : a.t_out;
}

__global__ __launch_bounds__(64) void hier_span_kernel(const HierarchyArgs a)
{
    const int c = blockIdx.x, lane = threadIdx.x;
    if (c >= a.n_out) return;
    int o0, o1;
    bool bad = !hier_column(a, c, o0, o1);
    long long lo = INT64_MAX, hi = INT64_MIN;
    for (int i = o0 + lane; i < o1; i += 64) {
        const int s = a.members[i];
        if (s < 0 || s >= a.n_series) { bad = true; continue; }
        const long long f = a.first ? (long long)a.first[s] : 0ll;
        if (f > HIER_FIRST_MAX || f < -HIER_FIRST_MAX) { bad = true; continue; }
        const int n = hier_length(a, s);
        if (n == 0) continue;
        int t0 = 0, t1 = n - 1;
        if (a.present) {
            while (t0 < n && !a.present[(size_t)t0 * a.ld + (size_t)s]) t0++;
            if (t0 == n) continue;
            while (!a.present[(size_t)t1 * a.ld + (size_t)s]) t1--;          // (stops at t0 at the latest)
        }
        if (f + t0 < lo) lo = f + t0;
        if (f + t1 > hi) hi = f + t1;
    }
    for (int d = 32; d >= 1; d >>= 1) {
        const long long lo2 = __shfl_xor(lo, d), hi2 = __shfl_xor(hi, d);
        if (lo2 < lo) lo = lo2;
        if (hi2 > hi) hi = hi2;
    }
    bad = __ballot(bad) != 0ull;
    if (lane != 0) return;
    int32_t L = 0;
    int64_t fo = 0;
    if (bad) L = -1;
    else if (lo <= hi) {
        const long long span = hi - lo + 1;                  // (|lo|, |hi| <= 2^61 + 2^30)
        if (span > HIER_SPAN_MAX) L = -1;
        else { L = (int32_t)span; fo = lo; }
    }
    a.len_out[c] = L;
    a.first_out[c] = fo;
}

__global__ __launch_bounds__(HL_COLS) void hier_lane_kernel(const HierarchyArgs a)
{
    const size_t cc = (size_t)blockIdx.x * HL_COLS + threadIdx.x;
    if (cc >= (size_t)a.n_out) return;
    const int c = (int)cc;
    int o0, o1;
    hier_column(a, c, o0, o1);
    if (hier_takes_tile(a, o1 - o0)) return;
    const size_t L = hier_rows(a, c);
    const long long fo = a.first_out[c];
    const size_t n_tiles = (a.t_out + HL_ROWS - 1) / HL_ROWS;
    for (size_t tile = blockIdx.y; tile < n_tiles; tile += gridDim.y) {
        const size_t r0 = tile * HL_ROWS;
        double acc[HL_ROWS];
        unsigned exists = 0u;
#pragma unroll
        for (int k = 0; k < HL_ROWS; k++) acc[k] = 0.0;
        if (r0 < L) {
            for (int i = o0; i < o1; i++) {
                const int s = a.members[i];
                if (s < 0 || s >= a.n_series) continue;                  // (the span kernel marked the column: L is 0)
                const long long n = hier_length(a, s);
                const long long base = fo + (long long)r0 - (a.first ? (long long)a.first[s] : 0ll);     // the series' row at grid row r0
#pragma unroll
                for (int k = 0; k < HL_ROWS; k++) {
                    const long long t = base + k;
                    if (t < 0 || t >= n || r0 + k >= L) continue;
                    const size_t at = (size_t)t * a.ld + (size_t)s;      // t < len <= t_rows, s < n_series <= ld
                    if (a.present && !a.present[at]) continue;
                    exists |= 1u << k;
                    acc[k] += (!a.valid || a.valid[at]) ? a.y[at] : 0.0;
                }
            }
        }
#pragma unroll
        for (int k = 0; k < HL_ROWS; k++) {
            const size_t r = r0 + k;
            if (r >= a.t_out) break;
            a.y_out[r * a.ld_out + cc] = acc[k];
            if (a.present_out) a.present_out[r * a.ld_out + cc] = (uint8_t)((exists >> k) & 1u);
        }
    }
}

// stages one tile: rows r0 .. r0 + 63 of the member this lane holds (series s, n rows, `base` = its row at grid row r0) go to
// tile[row][lane].  Branch-free on purpose: every load goes to an address clamped into the series' rows and the value is selected
// afterwards, 32 rows at a time, so that those loads are in flight together -- with a conditional load per row the wave
// waited out one memory latency per row.  (The caller stages only while some member has a row, so the block has at least one row
// and row 0 of series s can be read; what a clamped load returns for a row that does not exist is dropped by the select.)
// Returns, in lane k, the ballot of the members that have a row at grid row r0 + k.
template <bool HAS_VALID, bool HAS_PRESENT>
__device__ __forceinline__ uint64_t hier_stage_tile(const HierarchyArgs &a, int s, long long n, long long base, size_t r0, size_t L, int lane,
                                                    double *tile)
{
    constexpr int B = 32;                                                // rows in flight: 8 took 25 us per tile, one latency per batch
    const long long last = n > 0 ? n - 1 : 0;
    uint64_t my_rows = 0;
#pragma unroll 1
    for (int k0 = 0; k0 < HT; k0 += B) {
        double v[B];
        bool ok[B];
#pragma unroll
        for (int j = 0; j < B; j++) {
            const long long t = base + k0 + j;
            const long long tc = t < 0 ? 0 : (t > last ? last : t);
            const size_t at = (size_t)tc * a.ld + (size_t)s;
            const double x = a.y[at];
            const uint8_t pr = HAS_PRESENT ? a.present[at] : (uint8_t)1;
            const uint8_t va = HAS_VALID ? a.valid[at] : (uint8_t)1;
            ok[j] = (t >= 0) & (t < n) & (r0 + (size_t)(k0 + j) < L) & (pr != 0);
            v[j] = (ok[j] & (va != 0)) ? x : 0.0;
        }
#pragma unroll
        for (int j = 0; j < B; j++) {
            tile[(k0 + j) * HT_PITCH + lane] = v[j];
            const uint64_t m = __ballot(ok[j]);
            if (lane == k0 + j) my_rows = m;
        }
    }
    return my_rows;
}

// column c, grid rows r0 .. r0 + 63 of it: lane <-> member while a tile is staged, lane <-> row while it is summed
__device__ __forceinline__ void hier_tile_column(const HierarchyArgs &a, int c, size_t r0, int lane, double *tile)
{
    int o0, o1;
    hier_column(a, c, o0, o1);
    const size_t L = hier_rows(a, c);
    const long long fo = a.first_out[c];
    double sum = 0.0;
    bool exists = false;
    if (r0 < L) {
        for (int m0 = o0; m0 < o1; m0 += HT) {
            const int cnt = o1 - m0 < HT ? o1 - m0 : HT;
            int s = 0;
            long long n = 0, base = 0;
            if (lane < cnt) {
                s = a.members[m0 + lane];
                if (s < 0 || s >= a.n_series) s = 0;                     // (n stays 0: no row)
                else {
                    n = hier_length(a, s);
                    base = fo + (long long)r0 - (a.first ? (long long)a.first[s] : 0ll);
                }
            }
            __syncthreads();                                             // every lane has summed the previous tile
            uint64_t my_rows;                                            // lane k: the members that have a row at grid row r0 + k
            if (a.present) {
                my_rows = a.valid ? hier_stage_tile<true, true>(a, s, n, base, r0, L, lane, tile)
                                  : hier_stage_tile<false, true>(a, s, n, base, r0, L, lane, tile);
            } else {
                my_rows = a.valid ? hier_stage_tile<true, false>(a, s, n, base, r0, L, lane, tile)
                                  : hier_stage_tile<false, false>(a, s, n, base, r0, L, lane, tile);
            }
            __syncthreads();
            exists = exists || my_rows != 0ull;
            const double *row = tile + lane * HT_PITCH;
#pragma unroll 8
            for (int j = 0; j < cnt; j++) sum += row[j];
        }
    }
    const size_t r = r0 + (size_t)lane;
    if (r < a.t_out) {
        a.y_out[r * a.ld_out + (size_t)c] = sum;                         // (+0.0 where no member had a row)
        if (a.present_out) a.present_out[r * a.ld_out + (size_t)c] = exists ? 1 : 0;
    }
}

__global__ __launch_bounds__(64) void hier_tile_kernel(const HierarchyArgs a)
{
    __shared__ double tile[HT * HT_PITCH];
    const int lane = threadIdx.x;
    const size_t r0 = (size_t)blockIdx.x * HT;
    const size_t n_chunks = ((size_t)a.n_out + 63) / 64;
    for (size_t chunk = blockIdx.y; chunk < n_chunks; chunk += gridDim.y) {
        const size_t cl = chunk * 64 + (size_t)lane;
        bool mine = false;
        if (cl < (size_t)a.n_out) {
            int o0, o1;
            hier_column(a, (int)cl, o0, o1);
            mine = hier_takes_tile(a, o1 - o0);
        }
        uint64_t todo = __ballot(mine);
        while (todo) {
            const int b = __ffsll((unsigned long long)todo) - 1;
            todo &= todo - 1;
            hier_tile_column(a, (int)(chunk * 64) + b, r0, lane, tile);
        }
    }
}

} // namespace

void launch_hierarchy(const HierarchyArgs &a, hipStream_t stream)
{
    if (a.n_out <= 0) return;
    hipLaunchKernelGGL(hier_span_kernel, dim3((unsigned)a.n_out), dim3(64), 0, stream, a);
    if (!a.y_out || a.t_out == 0) return;
    if (a.route != HIER_ROUTE_TILE) {
        const size_t n_tiles = (a.t_out + HL_ROWS - 1) / HL_ROWS;
        const unsigned gy = (unsigned)(n_tiles > HIER_MAX_GRID_Y ? HIER_MAX_GRID_Y : n_tiles);
        hipLaunchKernelGGL(hier_lane_kernel, dim3((unsigned)(((size_t)a.n_out + HL_COLS - 1) / HL_COLS), gy), dim3(HL_COLS), 0, stream, a);
    }
    if (a.route != HIER_ROUTE_LANE) {
        const size_t n_chunks = ((size_t)a.n_out + 63) / 64;
        const unsigned gy = (unsigned)(n_chunks > HIER_MAX_GRID_Y ? HIER_MAX_GRID_Y : n_chunks);
        hipLaunchKernelGGL(hier_tile_kernel, dim3((unsigned)((a.t_out + HT - 1) / HT), gy), dim3(64), 0, stream, a);
    }
}

} // namespace anofox
