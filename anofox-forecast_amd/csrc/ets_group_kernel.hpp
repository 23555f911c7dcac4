// ets_group_kernel.hpp -- the group round kernel: round r of several ETS specs of one class in one launch (kernels.hpp
// GroupRoundArgs).  Each workgroup finds its slot from the prefix of the slots' workgroup counts, reads the slot's FitArgs from the
// table launch_fit_slots uploaded at the start of the run and runs that spec's round body (ets_fit_kernel.hpp) with the device-side
// driver choice, so a slot's problems take exactly the iterates they take in the spec's own launch chain.
// The specs of a class are a compile-time list (fit_group_*.hip, one compile unit per class); the kernel's registers are the most any
// member's body needs and its dynamic LDS the most any member asks for.
#pragma once
#include "fit_units.hpp"

namespace anofox {

// the period variant a member's round kernels use for the group's variant MSG -- what its own unit picks (fit_unit_impl.inc): none
// without a season, and only the additive-season specs have a compile-time ring of 12
template <int ID, int MSG> constexpr int group_member_ms()
{
    if constexpr (SpecOf<ID>::s == 0) return 0;
    else if constexpr (MSG == 12 && !SpecOf<ID>::Cfg::ADDITIVE) return -1;
    else return MSG;
}
template <int ID, int MSG> constexpr bool group_member_k4() { return SpecOf<ID>::Cfg::ADDITIVE && (group_member_ms<ID, MSG>() == 0 || group_member_ms<ID, MSG>() == 7); }

// the members must share the one-wave workgroup and residency of their own kernels (an experiment build with PARK or WPB > 1 has none)
template <class YT, int... IDS> struct GroupTraits {
    static constexpr bool OK = ((RoundTraits<typename SpecOf<IDS>::Cfg, YT>::WAVES == RoundTraits<typename SpecOf<0>::Cfg, YT>::WAVES &&
                                 RoundTraits<typename SpecOf<IDS>::Cfg>::WPB == 1 && !RoundTraits<typename SpecOf<IDS>::Cfg>::PARK) && ...);
};

template <class YT> constexpr int group_waves = RoundTraits<typename SpecOf<0>::Cfg, YT>::WAVES;      // (every member's: GroupTraits::OK)

template <int ID, int MSG, class YT>
__device__ __forceinline__ void ets_group_slot(const FitArgs &a, const int k4, const int vblock, const int vgrid, double *const lds)
{
    using Cfg = typename SpecOf<ID>::Cfg;
    constexpr int MS = group_member_ms<ID, MSG>();
    if constexpr (SpecOf<ID>::s != 0 && MSG == 0) return;                       // (a batch without a period has no seasonal spec)
    else {
        if constexpr (group_member_k4<ID, MSG>())
            if (k4) { ets_round_body<Cfg, MS, 3, true, YT>(a, vblock, vgrid, 0, lds); return; }
        ets_round_body<Cfg, MS, 3, false, YT>(a, vblock, vgrid, 0, lds);
    }
}

template <int MSG, class YT, int... IDS>
__global__ __launch_bounds__(NM_BLOCK, group_waves<YT>) void ets_group_round_kernel(const FitArgs *__restrict__ tab, const GroupRoundArgs g)
{
    extern __shared__ double lds_all[];
    const int b = (int)blockIdx.x;
    int k = 0;
    while (k + 1 < g.n_slots && b >= g.start[k + 1]) k++;
    // the table is read-only while the kernel runs: through the constant address space its fields load like a kernel argument's
    // (scalar, reloaded where needed) instead of being held in registers across the round
    const FitArgs &a = *(const FitArgs *)((const __attribute__((address_space(4))) FitArgs *)tab + k);
    const int vblock = b - g.start[k], vgrid = g.start[k + 1] - g.start[k], id = g.spec[k], k4 = g.k4[k];
    (void)((id == IDS && (ets_group_slot<IDS, MSG, YT>(a, k4, vblock, vgrid, lds_all), true)) || ...);
}

template <int MSG, class YT, int... IDS>
void ets_group_round_launch(const FitArgs *tab, const GroupRoundArgs &g, int m, hipStream_t stream)
{
    const int blocks = g.start[g.n_slots];
    if (blocks <= 0) return;
    // dynamic LDS: the most any member asks for (simplex store, plus the seasonal ring of a run-time period in LDS)
    size_t lds_doubles = 0;
    ((lds_doubles = std::max(lds_doubles, (size_t)nm_lds_doubles<SpecOf<IDS>::Cfg::DIM>() +
                                              (group_member_ms<IDS, MSG>() == -1 ? (size_t)m * NM_BLOCK : 0))), ...);
    const size_t lds_bytes = sizeof(double) * lds_doubles;
    if (lds_bytes > 48 * 1024)
        anofox_check_attr(hipFuncSetAttribute((const void *)ets_group_round_kernel<MSG, YT, IDS...>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes));
    hipLaunchKernelGGL((ets_group_round_kernel<MSG, YT, IDS...>), dim3(blocks), dim3(NM_BLOCK), lds_bytes, stream, tab, g);
}

template <int MSG, int... IDS> GroupLaunchFn group_launcher_of_yt(int yt)
{
    if constexpr (!GroupTraits<double, IDS...>::OK || !GroupTraits<float, IDS...>::OK) return nullptr;
    else {
        if (yt == YT_U16) {
            if constexpr (ets_u16_variant(MSG) && GroupTraits<unsigned short, IDS...>::OK) return &ets_group_round_launch<MSG, unsigned short, IDS...>;
            else return nullptr;
        }
        if (yt == YT_F32) return &ets_group_round_launch<MSG, float, IDS...>;
        return &ets_group_round_launch<MSG, double, IDS...>;
    }
}
// m: the batch's period (1: none), mapped to the variants the members' own units pick; a merged batch of several periods has none
template <int... IDS> GroupLaunchFn group_launcher_of(int m, int yt)
{
    if (m <= 1) return group_launcher_of_yt<0, IDS...>(yt);
    if (m == 7) return group_launcher_of_yt<7, IDS...>(yt);
    constexpr bool ring12 = ((SpecOf<IDS>::s != 0 && SpecOf<IDS>::Cfg::ADDITIVE) || ...);      // (else 12 is the run-time LDS variant)
    if (m == 12 && ring12) return group_launcher_of_yt<12, IDS...>(yt);
    if (m > ETS_LDS_PERIOD) return group_launcher_of_yt<-2, IDS...>(yt);
    return group_launcher_of_yt<-1, IDS...>(yt);
}

} // namespace anofox
