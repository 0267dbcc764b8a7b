// rimphony_tab_family_pitchy_group.hip -- group_kernel<P> (group_kernel.h) for the tabulated distribution as a family of energy
// tables with a sin^k xi prefactor per table (rimphony_ctx_set_tables_family with sin_k; gfx950 only): the Symphony coefficients
// of a parameter point in lock-step, the blended spline lookup and the pow of a sample made once for all members that need them.
//
// A translation unit of its own, as rimphony_tab_family_group.hip is and for the same reason.
#include "group_kernel.h"
#include "tab_launch.h"

const void *rim_tab_family_pitchy_group_kernel()
{
    return reinterpret_cast<const void *>(group_kernel<SymGroupProblem<DIST_TABULATED_FAMILY_PITCHY>>);
}
