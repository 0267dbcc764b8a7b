// rimphony_tab_2d_nodes_pitchy_group.hip -- group_kernel<P> (group_kernel.h) for the tabulated distribution as a 2-D set with a
// sin^k xi prefactor on gamma nodes and mu nodes of the caller's choosing (rimphony_ctx_set_tables_2d_nodes with a sin_k;
// gfx950 only): the Symphony coefficients of a parameter point in lock-step, the two interval searches, the bicubic and the
// pow of a sample made once for all members that need them.
//
// A translation unit of its own, as rimphony_tab_2d_grid_group.hip is and for the same reason.  It lives with the same
// budget: RIM_GROUP_WAVES waves per SIMD and the same LDS block.
#include "group_kernel.h"
#include "tab_launch.h"

const void *rim_tab_2d_nodes_pitchy_group_kernel()
{
    return reinterpret_cast<const void *>(group_kernel<SymGroupProblem<DIST_TABULATED_2D_NODES_PITCHY>>);
}
