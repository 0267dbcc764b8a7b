// rimphony_tab_family_pitchy.hip -- the kernels of the tabulated distribution as a FAMILY of energy tables with a sin^k xi
// prefactor per table (rimphony_ctx_set_tables_family with sin_k, DIST_TABULATED_FAMILY_PITCHY; gfx950 only): the prologue
// that writes the rows' lines, the per-row normalisation, the one-wave-per-coefficient Symphony and Faraday kernels and the
// two unit seams of coop_kernel.h.  A sample reads what a sample of an isotropic family reads, and the blended k and the
// weight, two wave-uniform words of its row's line.
//
// A translation unit of its own, as rimphony_tab_family.hip is and for the same reason.  The form's group kernel is
// rimphony_tab_family_pitchy_group.hip's.
#define RIM_TF_KIND 15          // DIST_TABULATED_FAMILY_PITCHY (the preprocessor compares it: tab_family_unit.h)
#define RIM_TF_LAUNCH_NORM rim_tab_family_pitchy_launch_norm
#define RIM_TF_COOP_KERNEL rim_tab_family_pitchy_coop_kernel
#define RIM_TF_LAUNCH_INTEGRAND rim_tab_family_pitchy_launch_integrand
#define RIM_TF_LAUNCH_GAMMA_INTEGRAL rim_tab_family_pitchy_launch_gamma_integral
#include "tab_family_unit.h"
static_assert(RIM_TF_KIND == DIST_TABULATED_FAMILY_PITCHY, "the form of this unit");
