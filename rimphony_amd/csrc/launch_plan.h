// launch_plan.h -- the geometry of a persistent launch as integer arithmetic on numbers the host already has.
// Host only and free of HIP, so that the CPU tests pin it (tests/support/devfn_host.cpp, tests/test_host_side.py).
#ifndef RIM_LAUNCH_PLAN_H
#define RIM_LAUNCH_PLAN_H

#include <cstddef>

struct RimGridPlan {
    int resident_per_cu;            // workgroups (= waves) of the kernel a CU is asked to hold
    unsigned grid;                  // single-wave workgroups of the launch
    // the squad that serves the longest chain from the start (coop_common.h); 0 / 1 / 1: none
    unsigned early_squad, early_stride, early_classes;
};

// n_cu              compute units of the device
// ntasks            tasks of the launch
// occupancy_blocks  what hipOccupancyMaxActiveBlocksPerMultiprocessor answered for the kernel (< 1: the query failed)
// static_lds, dyn_lds  LDS bytes of a workgroup (0, 0: not known)
// waves             waves per SIMD the kernel's launch bounds ask for
// want_squad        squad size asked for (the kind's default or RIMPHONY_EARLY_SQUAD); early_help: the kernel has the protocol
inline RimGridPlan rim_plan_grid(int n_cu, unsigned long long ntasks, int occupancy_blocks, size_t static_lds, size_t dyn_lds,
                                 int waves, bool shared_mode, bool no_assist, unsigned want_squad, bool early_help)
{
    RimGridPlan p;
    // Every wave of the grid should be resident: an idle wave waits for the waves that still own a task.  The runtime
    // says how many of these workgroups a CU really holds (registers, LDS) instead of the launch bounds being trusted;
    // a failed query counts as one wave per SIMD.  The query knows nothing of other work on the device: should part of
    // the grid not be resident after all, helpers leave after 2 s without work and an owner that waits in vain
    // recomputes its batch itself, so every wait ends and no result changes.
    const int nb = occupancy_blocks < 1 ? 4 : occupancy_blocks;
    p.resident_per_cu = nb < 4 * waves ? nb : 4 * waves;
    // The occupancy query has been seen to count one workgroup too many when the grid is LDS-bound to the last
    // granule (a grid with non-resident waves does not fail, it stalls: every helper's 2 s idle bound).  Re-derive
    // the LDS limit here with the 512-byte allocation granule and one granule of slack.
    const size_t lds = ((static_lds + dyn_lds + 511) / 512) * 512;
    if (lds > 0) {
        const int by_lds = (int) ((160 * 1024 - 512) / lds);
        if (by_lds >= 1 && by_lds < p.resident_per_cu) p.resident_per_cu = by_lds;
    }
    if (shared_mode) p.resident_per_cu = p.resident_per_cu >= 8 ? p.resident_per_cu / 4 : 2;   // leave room for the other tenant
    // more waves than tasks on small batches: the surplus waves start as helpers right away
    const unsigned long long want_waves = (ntasks > (1ull << 40) || no_assist) ? ntasks : ntasks * 64ull;
    unsigned long long g = (unsigned long long) n_cu * (unsigned) p.resident_per_cu;
    if (g > want_waves) g = want_waves;
    if (g < 1) g = 1;
    p.grid = (unsigned) g;
    // the squad: only where there is a bulk to overlap with (many more tasks than waves) and the GPU is this context's
    // own; blocks k * stride with an odd stride, so that the squad is spread over the XCDs (blocks go to them
    // round-robin) and their CUs
    p.early_squad = 0;
    p.early_stride = 1;
    p.early_classes = 1;
    if (early_help && !no_assist && !shared_mode && want_squad && ntasks >= 4ull * p.grid && p.grid >= 16u * want_squad) {
        p.early_stride = (p.grid / want_squad) | 1u;
        const unsigned fit = (p.grid - 1u) / p.early_stride + 1u;
        p.early_squad = want_squad < fit ? want_squad : fit;
        // one title per 64 waves of the squad (a batch has up to 62 requests), at most four
        p.early_classes = p.early_squad >= 256u ? 4u : p.early_squad >= 128u ? 2u : 1u;
    }
    return p;
}

#endif
