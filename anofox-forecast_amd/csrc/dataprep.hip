// dataprep.hip -- what the reference runs in front of ts_forecast_by, for every series of a time-major block: the gaps stage
// (gaps.rs:78-259 fill_gaps, the four FrequencyTypes), the zero trimmers (ts_drop_leading_zeros_by / _trailing_ / _edge_,
// ts_macros.cpp:208-256) and the NULL fills of imputation.rs, in this fixed order, then eight counts and min / max per series.
//
// One lane per series, the lanes of a wave own adjacent columns: every row of the INPUT blocks is read as one contiguous segment
// per wave (512 B of fp64 / int64, 64 B of validity), DP_ROWS rows requested before the first is consumed.  The kernel is two
// sweeps over the input rows of the lane's series and keeps nothing but scalars between them:
//
//   sweep 1 (count)  the rows the gaps stage inserts in front of every row (arithmetic on two dates, no loop), the position of the
//                    first and the last non-zero row of the gap-filled series, the input NULLs, and the mean fill's sum: the valid
//                    values added in row order from 0.0.  The window the trim leaves is known only at the end, so the sum and its
//                    count are snapshot at every non-zero row (what follows the last one is trimmed), and start at the first one
//                    when the front is trimmed (what precedes it is zeros: 0.0 + -0.0 = 0.0, the sum would not have moved).
//   sweep 2 (write)  walks the gap-filled series again -- inserted rows by a loop per input row -- and stores row e at output row
//                    e - front.  const, mean and forward fill a NULL where it stands; backward and interpolate fill a run of NULLs
//                    when the valid row that ends it arrives (prev + slope * j, slope = (v - prev) / gap, as imputation.rs:99-113;
//                    -ffp-contract=off: no FMA), the trailing run after the sweep.  The output figures are counted here, so a call
//                    without output blocks (count mode) runs the same sweep with its stores switched off.
//
// The stores of sweep 2 go to row e - front of the lane's own column: lanes with different shifts, or at different places of an
// inserted run, write different rows, 8 B of a 64-B line each.  That is the price of a per-series shift in a time-major block and
// is accepted; the neighbouring lanes' stores to the same row merge in L2.  Nothing crosses lanes, no LDS, no
// atomics: the same bits on every run and through every entry.
#include "kernels.hpp"
#include "civil_date.hpp"

namespace anofox {

namespace {

constexpr int DP_ROWS = 4;                                   // input rows in flight per lane and block
constexpr int64_t DP_SATURATE = (int64_t)1 << 40;            // the inserted-row count stops growing here (far above PREP_MAX_ROWS)

// period index (year * 12 + month, year * 4 + quarter, year) and the first month of the period, of micros_to_datetime(us)
struct DpPeriod { int64_t index, year, month0; };
__host__ __device__ __forceinline__ DpPeriod dp_period(int64_t us, int type)
{
    int64_t y, m;
    cd_year_month(us, y, m);
    DpPeriod p;
    p.year = y;
    if (type == STATS_FREQ_MONTHLY) { p.index = y * 12 + m; p.month0 = m; }
    else if (type == STATS_FREQ_QUARTERLY) { p.index = y * 4 + (m - 1) / 3; p.month0 = ((m - 1) / 3) * 3 + 1; }
    else { p.index = y; p.month0 = 1; }
    return p;
}

// rows the gaps stage inserts between two consecutive rows (gaps.rs:123-136, 154-174)
__host__ __device__ __forceinline__ int64_t dp_inserted(const DataprepArgs &a, int64_t d_prev, int64_t d_cur, const DpPeriod &p_prev, const DpPeriod &p_cur)
{
    int64_t steps;
    if (a.freq_type == STATS_FREQ_FIXED) steps = (int64_t)((uint64_t)d_cur - (uint64_t)d_prev) / a.freq_us;
    else steps = p_cur.index - p_prev.index;
    return steps > 1 ? steps - 1 : 0;
}

// date of inserted row `step` (1 ..) after the row dated d_prev
__host__ __device__ __forceinline__ int64_t dp_inserted_date(const DataprepArgs &a, int64_t d_prev, const DpPeriod &p_prev, int64_t step)
{
    if (a.freq_type == STATS_FREQ_FIXED) return (int64_t)((uint64_t)d_prev + (uint64_t)step * (uint64_t)a.freq_us);
    const int64_t k = a.freq_type == STATS_FREQ_MONTHLY ? 1 : a.freq_type == STATS_FREQ_QUARTERLY ? 3 : 12;
    const int64_t idx = p_prev.year * 12 + (p_prev.month0 - 1) + step * k;
    const int64_t yy = cd_floor_div(idx, 12);
    return cd_month_start_micros(yy, idx - yy * 12 + 1);
}

// the lane's state in sweep 2
struct DpOut {
    int64_t front, L;            // output row = position - front, kept when 0 <= row < L
    bool store;
    size_t ld; int s;
    double *y; uint8_t *valid; int64_t *dates;
    int fill; double fill_value, mean;
    bool have_prev; double pv; int64_t po;       // the last valid row of the window: value, output row
    int64_t n_null, n_nonzero, n_num; bool any_nan; double vmin, vmax;
};
__host__ __device__ __forceinline__ void dp_emit(DpOut &o, int64_t row, double v)       // a valid output row
{
    if (o.store) {
        o.y[(size_t)row * o.ld + o.s] = v;
        if (o.valid) o.valid[(size_t)row * o.ld + o.s] = 1;
    }
    if (!(v == 0.0)) o.n_nonzero++;
    if (v != v) o.any_nan = true;
    else {
        if (o.n_num == 0 || v < o.vmin) o.vmin = v;
        if (o.n_num == 0 || v > o.vmax) o.vmax = v;
        o.n_num++;
    }
}
__host__ __device__ __forceinline__ void dp_emit_null(DpOut &o, int64_t row)
{
    if (o.store) {
        o.y[(size_t)row * o.ld + o.s] = __builtin_nan("");
        if (o.valid) o.valid[(size_t)row * o.ld + o.s] = 0;
    }
    o.n_null++;
}
// a NULL at output row `row` (an inserted row, or an input NULL)
__host__ __device__ __forceinline__ void dp_null_row(DpOut &o, int64_t row)
{
    switch (o.fill) {
    case PREP_FILL_NONE: dp_emit_null(o, row); break;
    case PREP_FILL_CONST: dp_emit(o, row, o.fill_value); break;
    case PREP_FILL_MEAN: dp_emit(o, row, o.mean); break;
    case PREP_FILL_FORWARD: if (o.have_prev) dp_emit(o, row, o.pv); else dp_emit_null(o, row); break;
    default: break;                                          // backward, interpolate: when the run ends
    }
}
// a valid value at output row `row`: first the run of NULLs it ends
__host__ __device__ __forceinline__ void dp_valid_row(DpOut &o, int64_t row, double v)
{
    if (o.fill == PREP_FILL_INTERPOLATE) {
        if (o.have_prev) {
            const int64_t gap = row - o.po;
            if (gap > 1) {
                const double slope = (v - o.pv) / (double)gap;
                for (int64_t j = 1; j < gap; j++) dp_emit(o, o.po + j, o.pv + slope * (double)j);
            }
        } else {
            for (int64_t k = 0; k < row; k++) dp_emit(o, k, v);
        }
    } else if (o.fill == PREP_FILL_BACKWARD) {
        for (int64_t k = o.have_prev ? o.po + 1 : 0; k < row; k++) dp_emit(o, k, v);
    }
    dp_emit(o, row, v);
    o.have_prev = true; o.pv = v; o.po = row;
}

// both sweeps of series s (host-callable too: the body is plain C++, so a CPU harness can run it under a sanitizer)
__host__ __device__ __forceinline__ void dp_series(const DataprepArgs &a, const int s)
{
    const size_t ld = a.ld;
    int n = a.len[s];
    if (n < 0) n = 0;
    if ((size_t)n > a.t_rows) n = (int)a.t_rows;
    const bool gaps = a.gaps != 0, calendar = a.freq_type != STATS_FREQ_FIXED;
    const bool lead = (a.trim & PREP_TRIM_LEADING) != 0, trail = (a.trim & PREP_TRIM_TRAILING) != 0;
    const double *yc = a.y + s;
    const uint8_t *vc = a.valid ? a.valid + s : nullptr;
    const int64_t *dc = a.dates ? a.dates + s : nullptr;

    // ---- sweep 1: count ----
    int64_t e = 0, inserted = 0, n_null_in = 0, first_nz = -1, last_nz = -1;
    double msum = 0.0, msum_nz = 0.0;
    int64_t mcnt = 0, mcnt_nz = 0;
    {
        int64_t d_prev = 0;
        DpPeriod p_prev{0, 1970, 1};
        for (int t0 = 0; t0 < n; t0 += DP_ROWS) {
            double v[DP_ROWS]; bool ok[DP_ROWS]; int64_t d[DP_ROWS];
#pragma unroll
            for (int k = 0; k < DP_ROWS; k++) {
                const bool in = t0 + k < n;
                const size_t at = (size_t)(t0 + k) * ld;
                v[k] = in ? yc[at] : 0.0;
                ok[k] = in && (!vc || vc[at] != 0);
                d[k] = (in && dc) ? dc[at] : 0;
            }
#pragma unroll
            for (int k = 0; k < DP_ROWS; k++) {
                if (t0 + k >= n) break;
                if (gaps) {
                    DpPeriod p_cur{0, 1970, 1};
                    if (calendar) p_cur = dp_period(d[k], a.freq_type);
                    if (t0 + k > 0) {
                        const int64_t ins = dp_inserted(a, d_prev, d[k], p_prev, p_cur);
                        inserted += ins;
                        if (inserted > DP_SATURATE) inserted = DP_SATURATE;
                        e += ins;
                        if (e > DP_SATURATE) e = DP_SATURATE;
                    }
                    d_prev = d[k]; p_prev = p_cur;
                }
                if (!ok[k]) n_null_in++;
                const bool nz = ok[k] && !(v[k] == 0.0);
                if (nz) { if (first_nz < 0) first_nz = e; last_nz = e; }
                if (ok[k] && (!lead || first_nz >= 0)) { msum += v[k]; mcnt++; }
                if (nz) { msum_nz = msum; mcnt_nz = mcnt; }
                e++;
            }
        }
    }
    const int64_t E = e;
    int64_t front = 0, back = 0;
    if (a.trim != PREP_TRIM_NONE) {
        if (first_nz < 0) { if (lead) front = E; else back = E; }
        else { front = lead ? first_nz : 0; back = trail ? E - 1 - last_nz : 0; }
    }
    const int64_t L = E - front - back;
    if (trail) { msum = msum_nz; mcnt = mcnt_nz; }
    const double mean = mcnt > 0 ? msum / (double)mcnt : __builtin_nan("");

    int64_t status = PREP_OK;
    if (E > PREP_MAX_ROWS) status = PREP_OVER_LIMIT;
    else if (a.y_out && (uint64_t)L > (uint64_t)a.t_out) status = PREP_NO_ROOM;

    // ---- sweep 2: write ----
    DpOut o;
    o.front = front; o.L = L; o.store = a.y_out != nullptr && status == PREP_OK;
    o.ld = ld; o.s = s; o.y = a.y_out; o.valid = a.valid_out; o.dates = dc ? a.dates_out : nullptr;
    o.fill = a.fill; o.fill_value = a.fill_value; o.mean = mean;
    o.have_prev = false; o.pv = 0.0; o.po = -1;
    o.n_null = 0; o.n_nonzero = 0; o.n_num = 0; o.any_nan = false; o.vmin = 0.0; o.vmax = 0.0;
    if (status == PREP_OK && L > 0) {
        int64_t pos = 0, d_prev = 0;
        DpPeriod p_prev{0, 1970, 1};
        for (int t0 = 0; t0 < n; t0 += DP_ROWS) {
            double v[DP_ROWS]; bool ok[DP_ROWS]; int64_t d[DP_ROWS];
#pragma unroll
            for (int k = 0; k < DP_ROWS; k++) {
                const bool in = t0 + k < n;
                const size_t at = (size_t)(t0 + k) * ld;
                v[k] = in ? yc[at] : 0.0;
                ok[k] = in && (!vc || vc[at] != 0);
                d[k] = (in && dc) ? dc[at] : 0;
            }
#pragma unroll
            for (int k = 0; k < DP_ROWS; k++) {
                if (t0 + k >= n) break;
                if (gaps) {
                    DpPeriod p_cur{0, 1970, 1};
                    if (calendar) p_cur = dp_period(d[k], a.freq_type);
                    if (t0 + k > 0) {
                        const int64_t ins = dp_inserted(a, d_prev, d[k], p_prev, p_cur);
                        // inserted rows pos .. pos + ins - 1 (step = row - pos + 1): only those inside the window
                        int64_t r0 = pos > front ? pos : front, r1 = pos + ins < front + L ? pos + ins : front + L;
                        for (int64_t r = r0; r < r1; r++) {
                            if (o.store && o.dates) o.dates[(size_t)(r - front) * ld + s] = dp_inserted_date(a, d_prev, p_prev, r - pos + 1);
                            dp_null_row(o, r - front);
                        }
                        pos += ins;
                    }
                    d_prev = d[k]; p_prev = p_cur;
                }
                const int64_t row = pos - front;
                if (row >= 0 && row < L) {
                    if (o.store && o.dates) o.dates[(size_t)row * ld + s] = d[k];
                    if (ok[k]) dp_valid_row(o, row, v[k]); else dp_null_row(o, row);
                }
                pos++;
            }
        }
        // the run of NULLs that no valid row ended
        if (o.fill == PREP_FILL_INTERPOLATE) {
            const double tailv = o.have_prev ? o.pv : __builtin_nan("");
            for (int64_t k = o.po + 1; k < L; k++) dp_emit(o, k, tailv);
        } else if (o.fill == PREP_FILL_BACKWARD) {
            for (int64_t k = o.po + 1; k < L; k++) dp_emit_null(o, k);
        }
    }

    a.len_out[s] = status == PREP_OK ? (int32_t)L : 0;
    const double nan = __builtin_nan("");
    const int64_t iv[PREP_N_INT] = {n, n_null_in, inserted, front, back, o.n_null, o.n_nonzero, status};
#pragma unroll
    for (int i = 0; i < PREP_N_INT; i++) a.out_int[(size_t)i * ld + s] = iv[i];
    a.out_fp[s] = o.n_num > 0 ? o.vmin : nan;                           // NaN above every number: the minimum is NaN only when nothing else is there
    a.out_fp[ld + s] = o.any_nan ? nan : o.n_num > 0 ? o.vmax : nan;
}

__global__ __launch_bounds__(64) void dataprep_kernel(const DataprepArgs a)
{
    const int s = blockIdx.x * 64 + threadIdx.x;
    if (s >= a.n_series) return;
    dp_series(a, s);
}

} // namespace

void launch_dataprep(const DataprepArgs &a, hipStream_t stream)
{
    if (a.n_series <= 0) return;
    hipLaunchKernelGGL(dataprep_kernel, dim3((a.n_series + 63) / 64), dim3(64), 0, stream, a);
}

} // namespace anofox
