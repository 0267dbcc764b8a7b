// tab_launch.h -- what rimphony_hip.hip asks of rimphony_tab.hip and rimphony_tab_group.hip, the translation units that hold
// the kernels of the tabulated distribution (coop_kernel.h and group_kernel.h say why they have units of their own).
#ifndef RIM_TAB_LAUNCH_H
#define RIM_TAB_LAUNCH_H

#include "rimphony_internal.h"
#include "coop_common.h"

// what the persistent launch needs to know about a coop_kernel<P> instantiation
struct RimCoopKernelInfo {
    const void *fn;
    int waves;
    bool early_help;
    unsigned early_squad;
};

// the form of the installed table set, which chooses the instantiation: isotropic, with pitch rows, two-dimensional, with a
// sin^k xi prefactor (and pitch rows or none), on gamma nodes of its own (with both of those or neither)
enum { RIM_TAB_FORM_ISO = 0, RIM_TAB_FORM_PITCH = 1, RIM_TAB_FORM_2D = 2, RIM_TAB_FORM_PITCHY = 3, RIM_TAB_FORM_GRID = 4 };

// coop_kernel<SymphonyProblem<K>> (problem 0) or coop_kernel<HeyvaertsProblem<K>> (1); K = DIST_TABULATED for a table set with
// pitch rows, DIST_TABULATED_ISO (dev_symphony.h) for one without, DIST_TABULATED_2D for a 2-D set, DIST_TABULATED_PITCHY for one with a sin^k prefactor,
// DIST_TABULATED_GRID for one on given gamma nodes
RimCoopKernelInfo rim_tab_coop_kernel(int problem, int form);
// group_kernel<SymGroupProblem<K>> of a form, K as above (rimphony_tab_group.hip): the Symphony coefficients of a point in
// lock-step.  Launched with the grid and the arguments of the analytic kinds' (group_launch.h); the kind has no Faraday group.
const void *rim_tab_group_kernel(int form);
// ... of a set on given gamma nodes (RIM_TAB_FORM_GRID), which has a unit of its own: rimphony_tab_grid_group.hip
const void *rim_tab_grid_group_kernel();
// norm_kernel, integrand_kernel_n and gamma_integral_kernel of the kind: enqueue only, the caller asks hipGetLastError().
// (The rows of a 2-D set read their table's normalisation, which rim_tab_launch_table_norms computed when the set came in:
// one wave per table, `grid` waves, each with its region of `spill`.)
void rim_tab_launch_norm(int form, unsigned grid, hipStream_t st, const ParamPtrs &pp, size_t n, double *d_norm,
                         unsigned long long *queue, double *spill);
void rim_tab_launch_integrand(int form, unsigned grid, hipStream_t st, const PointArgs &pa, const double *d_norm, size_t count,
                              const double *d_n, const double *d_gamma, double *d_out);
void rim_tab_launch_gamma_integral(int form, unsigned grid, hipStream_t st, const PointArgs &pa, const double *d_norm, size_t count,
                                   const double *d_n, double *d_out, double *spill);
void rim_tab_launch_table_norms(unsigned grid, hipStream_t st, double *d_set, double *spill);
// P of every table of a sin^k set WITH pitch rows, into the tables' headers: one wave per table, as the line above.  (A set
// on given nodes passes the header of its tail, which reads as such a set: dev_symphony.h, tab_grid_tail.)
void rim_tab_launch_pitchy_p(unsigned grid, hipStream_t st, double *d_set, double *spill);

#endif
