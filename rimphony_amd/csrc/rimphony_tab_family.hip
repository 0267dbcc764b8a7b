// rimphony_tab_family.hip -- the kernels of the tabulated distribution as a FAMILY of isotropic energy tables on nodes uniform
// in ln gamma (rimphony_ctx_set_tables_family without sin_k, DIST_TABULATED_FAMILY; gfx950 only): the per-row normalisation,
// the one-wave-per-coefficient Symphony and Faraday kernels and the two unit seams of coop_kernel.h.  A sample reads the four
// spline words of its interval from two rows, blends them with the row's weight and evaluates one cubic (dev_symphony.h:
// tab_spline_family); the weight travels in par[0].
//
// A translation unit of its own: rimphony_tab.hip keeps its kernels instruction for instruction, and its dispatches hand this
// form on to the functions here (tab_launch.h).  The form's group kernel is rimphony_tab_family_group.hip's.
#define RIM_TF_KIND 14          // DIST_TABULATED_FAMILY (the preprocessor compares it: tab_family_unit.h)
#define RIM_TF_LAUNCH_NORM rim_tab_family_launch_norm
#define RIM_TF_COOP_KERNEL rim_tab_family_coop_kernel
#define RIM_TF_LAUNCH_INTEGRAND rim_tab_family_launch_integrand
#define RIM_TF_LAUNCH_GAMMA_INTEGRAL rim_tab_family_launch_gamma_integral
#include "tab_family_unit.h"
static_assert(RIM_TF_KIND == DIST_TABULATED_FAMILY, "the form of this unit");
