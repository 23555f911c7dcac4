// Group round kernels of the damped multiplicative-trend specs (ets_group_kernel.hpp).
#include "ets_group_kernel.hpp"
namespace anofox {
GroupLaunchFn fit_group_damped_mul(int m, int yt) { return group_launcher_of<12, 13, 14, 27, 29>(m, yt); }
} // namespace anofox
