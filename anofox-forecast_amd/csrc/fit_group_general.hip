// Group round kernels of the general-class specs without a damped multiplicative trend (ets_group_kernel.hpp).
#include "ets_group_kernel.hpp"
namespace anofox {
GroupLaunchFn fit_group_general(int m, int yt) { return group_launcher_of<2, 5, 8, 9, 10, 11, 15, 17, 18, 20, 21, 23, 24, 26>(m, yt); }
} // namespace anofox
