// rimphony_tab_2d_family.hip -- the kernels of the tabulated distribution as a FAMILY of 2-D surfaces on gamma nodes and mu nodes
// of the caller's choosing (rimphony_ctx_set_tables_2d_family with a null sin_k, DIST_TABULATED_2D_FAMILY; gfx950 only): the
// prologue that writes the rows' lines, the per-row normalisation, the one-wave-per-coefficient Symphony and Faraday kernels
// and the two unit seams of coop_kernel.h.  A sample finds its cell as a sample of rimphony_tab_2d_nodes.hip does, reads the
// cell's sixteen node words from two tables, blends them with the row's weight and evaluates one bicubic (dev_symphony.h:
// tab_bicubic_family); the weight and the distance to the upper table are two wave-uniform words of the row's line.
//
// A translation unit of its own: rimphony_tab.hip keeps its kernels instruction for instruction, and its dispatches hand this
// form on to the functions here (tab_launch.h).  The form's group kernel is rimphony_tab_2d_family_group.hip's.
#define RIM_T2F_KIND DIST_TABULATED_2D_FAMILY
#define RIM_T2F_LAUNCH_NORM rim_tab_2d_family_launch_norm
#define RIM_T2F_COOP_KERNEL rim_tab_2d_family_coop_kernel
#define RIM_T2F_LAUNCH_INTEGRAND rim_tab_2d_family_launch_integrand
#define RIM_T2F_LAUNCH_GAMMA_INTEGRAL rim_tab_2d_family_launch_gamma_integral
#include "tab_2d_family_unit.h"
