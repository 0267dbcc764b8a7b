// rimphony_tab_2d_nodes.hip -- the kernels of the tabulated distribution as a 2-D set on gamma nodes and mu nodes of the
// caller's choosing (rimphony_ctx_set_tables_2d_nodes with a null sin_k, DIST_TABULATED_2D_NODES; gfx950 only): the
// normalisation of the set's tables, the one-wave-per-coefficient Symphony and Faraday kernels and the two unit seams of
// coop_kernel.h.  A sample reads what a sample of a 2-D set on given gamma nodes reads, and for its mu interval two guide
// words and at most ten mu node words (dev_symphony.h: tab_bicubic_nodes).
//
// A translation unit of its own, as rimphony_tab_2d_grid.hip is and for the same reason; the text is tab_2d_pitchy_unit.h's,
// which serves any 2-D form.  The form's group kernel is rimphony_tab_2d_nodes_group.hip's.
#define RIM_T2P_KIND DIST_TABULATED_2D_NODES
#define RIM_T2P_NORM_KERNEL tab2d_nodes_table_norm_kernel
#define RIM_T2P_LAUNCH_TABLE_NORMS rim_tab_2d_nodes_launch_table_norms
#define RIM_T2P_COOP_KERNEL rim_tab_2d_nodes_coop_kernel
#define RIM_T2P_LAUNCH_INTEGRAND rim_tab_2d_nodes_launch_integrand
#define RIM_T2P_LAUNCH_GAMMA_INTEGRAL rim_tab_2d_nodes_launch_gamma_integral
#include "tab_2d_pitchy_unit.h"
