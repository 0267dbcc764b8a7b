// rimphony_tab_family_group.hip -- group_kernel<P> (group_kernel.h) for the tabulated distribution as a family of isotropic
// energy tables (rimphony_ctx_set_tables_family without sin_k; gfx950 only): the Symphony coefficients of a parameter point in
// lock-step, the blended spline lookup of a sample made once for all members that need it.
//
// A translation unit of its own, as rimphony_tab_2d_pitchy_group.hip is and for the same reason: this kernel must not move those
// of rimphony_tab_group.hip.  It lives with their budget: RIM_GROUP_WAVES waves per SIMD and the same LDS block.
#include "group_kernel.h"
#include "tab_launch.h"

const void *rim_tab_family_group_kernel()
{
    return reinterpret_cast<const void *>(group_kernel<SymGroupProblem<DIST_TABULATED_FAMILY>>);
}
