// rimphony_tab_grid_group.hip -- group_kernel<P> (group_kernel.h) for the tabulated distribution on given gamma nodes
// (rimphony_ctx_set_tables_grid; gfx950 only): the Symphony coefficients of a parameter point in lock-step, the interval
// search of a sample (dev_symphony.h: tab_grid_interval) made once for all members that need the lookup.
//
// A translation unit of its own, as rimphony_tab_group.hip is one beside rimphony_group.hip and for the same reason: hipcc's
// code generation for a kernel of this size depends on what else is in the unit (rimphony_internal.h), so this one must not
// move the four of that unit.  It lives with their budget: RIM_GROUP_WAVES waves per SIMD and the same LDS block.
#include "group_kernel.h"
#include "tab_launch.h"

const void *rim_tab_grid_group_kernel()
{
    return reinterpret_cast<const void *>(group_kernel<SymGroupProblem<DIST_TABULATED_GRID>>);
}
