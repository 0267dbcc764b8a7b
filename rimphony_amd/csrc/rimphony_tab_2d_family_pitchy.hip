// rimphony_tab_2d_family_pitchy.hip -- the kernels of the tabulated distribution as a FAMILY of 2-D surfaces with a sin^k xi
// prefactor per table, on gamma nodes and mu nodes of the caller's choosing (rimphony_ctx_set_tables_2d_family with a sin_k,
// DIST_TABULATED_2D_FAMILY_PITCHY; gfx950 only): the prologue that writes the rows' lines, the per-row normalisation, the
// one-wave-per-coefficient Symphony and Faraday kernels and the two unit seams of coop_kernel.h.  A sample reads what a sample
// of rimphony_tab_2d_family.hip reads, and the blended k, one more wave-uniform word of its row's line.
//
// A translation unit of its own, as rimphony_tab_2d_family.hip is and for the same reason.  The form's group kernel is
// rimphony_tab_2d_family_pitchy_group.hip's.
#define RIM_T2F_KIND DIST_TABULATED_2D_FAMILY_PITCHY
#define RIM_T2F_LAUNCH_NORM rim_tab_2d_family_pitchy_launch_norm
#define RIM_T2F_COOP_KERNEL rim_tab_2d_family_pitchy_coop_kernel
#define RIM_T2F_LAUNCH_INTEGRAND rim_tab_2d_family_pitchy_launch_integrand
#define RIM_T2F_LAUNCH_GAMMA_INTEGRAL rim_tab_2d_family_pitchy_launch_gamma_integral
#include "tab_2d_family_unit.h"
