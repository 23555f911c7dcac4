// civil_date.hpp -- the calendar arithmetic of the reference's micros_to_datetime (stats.rs:365-371, gaps.rs:8-14) and its way back,
// shared by the date figures of stats.hip and the gaps stage of dataprep.hip.  Proleptic Gregorian, UTC, days counted from
// 1970-01-01 (the era / day-of-era decomposition of the civil-from-days algorithm).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace anofox {

__host__ __device__ __forceinline__ int64_t cd_floor_div(int64_t a, int64_t b)    // b > 0
{
    const int64_t q = a / b;
    return (a % b < 0) ? q - 1 : q;
}

// year and month (1..12) of micros_to_datetime(us): seconds by truncating division; a negative remainder makes the nanosecond
// argument invalid, and the source then falls back to 1970-01-01, as for a date outside chrono's range
__host__ __device__ __forceinline__ void cd_year_month(int64_t us, int64_t &year, int64_t &month)
{
    year = 1970; month = 1;
    const int64_t secs = us / 1000000, rem = us % 1000000;
    if (rem >= 0) {
        const int64_t z = cd_floor_div(secs, 86400) + 719468;
        const int64_t era = cd_floor_div(z, 146097);
        const int64_t doe = z - era * 146097;
        const int64_t yoe = (doe - doe / 1460 + doe / 36524 - doe / 146096) / 365;
        const int64_t doy = doe - (365 * yoe + yoe / 4 - yoe / 100);
        const int64_t mp = (5 * doy + 2) / 153;
        const int64_t mm = mp < 10 ? mp + 3 : mp - 9;
        const int64_t yy = yoe + era * 400 + (mm <= 2 ? 1 : 0);
        if (yy >= -262143 && yy <= 262142) { year = yy; month = mm; }
    }
}

// microseconds of year-month-01 00:00:00 (datetime_to_micros of a start_of_month); month 1..12
__host__ __device__ __forceinline__ int64_t cd_month_start_micros(int64_t year, int64_t month)
{
    const int64_t y = year - (month <= 2 ? 1 : 0);
    const int64_t era = cd_floor_div(y, 400);
    const int64_t yoe = y - era * 400;
    const int64_t doy = (153 * (month > 2 ? month - 3 : month + 9) + 2) / 5;
    const int64_t doe = yoe * 365 + yoe / 4 - yoe / 100 + doy;
    return (era * 146097 + doe - 719468) * 86400000000ll;
}

} // namespace anofox
