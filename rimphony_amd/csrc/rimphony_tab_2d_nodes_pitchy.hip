// rimphony_tab_2d_nodes_pitchy.hip -- the kernels of the tabulated distribution as a 2-D set with a sin^k xi prefactor on gamma
// nodes and mu nodes of the caller's choosing (rimphony_ctx_set_tables_2d_nodes with a sin_k, DIST_TABULATED_2D_NODES_PITCHY;
// gfx950 only): the normalisation of the set's tables, the one-wave-per-coefficient Symphony and Faraday kernels and the two
// unit seams of coop_kernel.h.  A sample reads what a sample of rimphony_tab_2d_nodes.hip reads, and k, one wave-uniform word
// of its table's header.
//
// A translation unit of its own, as rimphony_tab_2d_grid.hip is and for the same reason; the text is tab_2d_pitchy_unit.h's,
// which serves any 2-D form.  The form's group kernel is rimphony_tab_2d_nodes_pitchy_group.hip's.
#define RIM_T2P_KIND DIST_TABULATED_2D_NODES_PITCHY
#define RIM_T2P_NORM_KERNEL tab2d_nodes_pitchy_table_norm_kernel
#define RIM_T2P_LAUNCH_TABLE_NORMS rim_tab_2d_nodes_pitchy_launch_table_norms
#define RIM_T2P_COOP_KERNEL rim_tab_2d_nodes_pitchy_coop_kernel
#define RIM_T2P_LAUNCH_INTEGRAND rim_tab_2d_nodes_pitchy_launch_integrand
#define RIM_T2P_LAUNCH_GAMMA_INTEGRAL rim_tab_2d_nodes_pitchy_launch_gamma_integral
#include "tab_2d_pitchy_unit.h"
