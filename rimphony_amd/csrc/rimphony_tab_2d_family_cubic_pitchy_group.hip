// rimphony_tab_2d_family_cubic_pitchy_group.hip -- group_kernel<P> (group_kernel.h) for the tabulated distribution as a family of
// 2-D surfaces with a sin^k xi prefactor per table, blended cubically across its tables (rimphony_ctx_set_tables_2d_family_cubic
// with a sin_k; gfx950 only): the Symphony coefficients of a parameter point in lock-step, the two interval searches and the
// four-table bicubic of a sample (dev_symphony.h: tab_bicubic_family_cubic) made once for all members that need them.
//
// A translation unit of its own, as rimphony_tab_2d_family_group.hip is and for the same reason.
#include "group_kernel.h"
#include "tab_launch.h"

const void *rim_tab_2d_family_cubic_pitchy_group_kernel()
{
    return reinterpret_cast<const void *>(group_kernel<SymGroupProblem<DIST_TABULATED_2D_FAMILY_CUBIC_PITCHY>>);
}
