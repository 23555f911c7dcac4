// Group round kernels of the additive class (ets_group_kernel.hpp).
#include "ets_group_kernel.hpp"
namespace anofox {
GroupLaunchFn fit_group_additive(int m, int yt) { return group_launcher_of<0, 1, 3, 4, 6, 7>(m, yt); }
} // namespace anofox
