// rimphony_tab_2d_family_cubic_pitchy.hip -- the kernels of the tabulated distribution as a family of 2-D surfaces with a sin^k xi
// prefactor per table, blended CUBICALLY across its tables (rimphony_ctx_set_tables_2d_family_cubic with a sin_k,
// DIST_TABULATED_2D_FAMILY_CUBIC_PITCHY; gfx950 only): the prologue that writes the rows' 128-byte lines, the per-row
// normalisation, the one-wave-per-coefficient Symphony and Faraday kernels and the two unit seams of coop_kernel.h.  A sample
// finds its cell as a sample of rimphony_tab_2d_family.hip does, reads the cell's sixteen node words from four tables, blends
// them with the row's four Lagrange weights and evaluates one bicubic (dev_symphony.h: tab_bicubic_family_cubic); the weights,
// the blended k and the table stride are wave-uniform words of the row's line.
//
// A translation unit of its own, as rimphony_tab_2d_family.hip is and for the same reason: no existing kernel moves.  The
// form's group kernel is rimphony_tab_2d_family_cubic_pitchy_group.hip's.
#define RIM_T2F_KIND DIST_TABULATED_2D_FAMILY_CUBIC_PITCHY
#define RIM_T2F_LAUNCH_NORM rim_tab_2d_family_cubic_pitchy_launch_norm
#define RIM_T2F_COOP_KERNEL rim_tab_2d_family_cubic_pitchy_coop_kernel
#define RIM_T2F_LAUNCH_INTEGRAND rim_tab_2d_family_cubic_pitchy_launch_integrand
#define RIM_T2F_LAUNCH_GAMMA_INTEGRAL rim_tab_2d_family_cubic_pitchy_launch_gamma_integral
#include "tab_2d_family_unit.h"
