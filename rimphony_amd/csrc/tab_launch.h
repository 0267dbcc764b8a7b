// tab_launch.h -- what rimphony_hip.hip asks of rimphony_tab.hip and rimphony_tab_group.hip, the translation units that hold
// the kernels of the tabulated distribution (coop_kernel.h and group_kernel.h say why they have units of their own), and what
// those two ask of the units that hold the kernels of one form each.
#ifndef RIM_TAB_LAUNCH_H
#define RIM_TAB_LAUNCH_H

#include "rimphony_internal.h"
#include "coop_common.h"
#include "tab_install.h"

// what the persistent launch needs to know about a coop_kernel<P> instantiation
struct RimCoopKernelInfo {
    const void *fn;
    int waves;
    bool early_help;
    unsigned early_squad;
};

// Every function takes the form of the installed table set as its DIST_TABULATED* value (dev_symphony.h), `tab_kind`, which
// chooses the instantiation K: DIST_TABULATED for a set with pitch rows, DIST_TABULATED_ISO for an isotropic one,
// DIST_TABULATED_2D for a 2-D set, DIST_TABULATED_PITCHY for one with a sin^k xi prefactor (and pitch rows or none),
// DIST_TABULATED_GRID for one on gamma nodes of its own (with both of those or neither), DIST_TABULATED_2D_GRID for a 2-D set
// on gamma nodes of its own, DIST_TABULATED_2D_PITCHY and DIST_TABULATED_2D_GRID_PITCHY for those two with a sin^k xi prefactor,
// DIST_TABULATED_2D_NODES and DIST_TABULATED_2D_NODES_PITCHY for a 2-D set on gamma and mu nodes of its own, without and with one,
// DIST_TABULATED_FAMILY and DIST_TABULATED_FAMILY_PITCHY for a family of energy tables, without and with one,
// DIST_TABULATED_2D_FAMILY and DIST_TABULATED_2D_FAMILY_PITCHY for a family of 2-D surfaces on given nodes, without and with one,
// DIST_TABULATED_2D_FAMILY_CUBIC and DIST_TABULATED_2D_FAMILY_CUBIC_PITCHY for such a family blended cubically across its tables.

// coop_kernel<SymphonyProblem<K>> (problem 0) or coop_kernel<HeyvaertsProblem<K>> (1)
RimCoopKernelInfo rim_tab_coop_kernel(int problem, int tab_kind);
// group_kernel<SymGroupProblem<K>>: the Symphony coefficients of a point in lock-step.  Launched with the grid and the
// arguments of the analytic kinds' (group_launch.h); the kind has no Faraday group.  Defined in rimphony_tab_group.hip, which
// asks rimphony_tab_grid_group.hip for the instantiation of DIST_TABULATED_GRID: that one has a unit of its own.
// DIST_TABULATED_2D_GRID's likewise: rimphony_tab_2d_grid_group.hip.
const void *rim_tab_group_kernel(int tab_kind);
const void *rim_tab_grid_group_kernel();
const void *rim_tab_2d_grid_group_kernel();
const void *rim_tab_2d_pitchy_group_kernel();           // rimphony_tab_2d_pitchy_group.hip
const void *rim_tab_2d_grid_pitchy_group_kernel();      // rimphony_tab_2d_grid_pitchy_group.hip
const void *rim_tab_2d_nodes_group_kernel();            // rimphony_tab_2d_nodes_group.hip
const void *rim_tab_2d_nodes_pitchy_group_kernel();     // rimphony_tab_2d_nodes_pitchy_group.hip
const void *rim_tab_family_group_kernel();              // rimphony_tab_family_group.hip
const void *rim_tab_family_pitchy_group_kernel();       // rimphony_tab_family_pitchy_group.hip
const void *rim_tab_2d_family_group_kernel();           // rimphony_tab_2d_family_group.hip
const void *rim_tab_2d_family_pitchy_group_kernel();    // rimphony_tab_2d_family_pitchy_group.hip
const void *rim_tab_2d_family_cubic_group_kernel();     // rimphony_tab_2d_family_cubic_group.hip
const void *rim_tab_2d_family_cubic_pitchy_group_kernel();      // rimphony_tab_2d_family_cubic_pitchy_group.hip
// norm_kernel, integrand_kernel_n and gamma_integral_kernel of the kind: enqueue only, the caller asks hipGetLastError().
// An isotropic set runs their DIST_TABULATED instantiations (rimphony_internal.h: rim_tab_seam_kind).  (The rows of a 2-D set
// read their table's normalisation, which rim_tab_launch_table_norms computed when the set came in: one wave per table,
// `grid` waves, each with its region of `spill`.)
void rim_tab_launch_norm(int tab_kind, unsigned grid, hipStream_t st, const ParamPtrs &pp, size_t n, double *d_norm,
                         unsigned long long *queue, double *spill);
void rim_tab_launch_integrand(int tab_kind, unsigned grid, hipStream_t st, const PointArgs &pa, const double *d_norm, size_t count,
                              const double *d_n, const double *d_gamma, double *d_out);
void rim_tab_launch_gamma_integral(int tab_kind, unsigned grid, hipStream_t st, const PointArgs &pa, const double *d_norm, size_t count,
                                   const double *d_n, double *d_out, double *spill);
void rim_tab_launch_table_norms(unsigned grid, hipStream_t st, double *d_set, double *spill);
// P of every table of a sin^k set WITH pitch rows, into the tables' headers: one wave per table, as the line above.  (A set
// on given nodes passes the header of its tail, which reads as such a set: dev_symphony.h, tab_grid_tail.)
void rim_tab_launch_pitchy_p(unsigned grid, hipStream_t st, double *d_set, double *spill);

// The kernels of a 2-D set on given gamma nodes (DIST_TABULATED_2D_GRID) live in rimphony_tab_2d_grid.hip: the functions above
// hand that form on to these.  Its rows read their table's normalisation as those of a 2-D set do (tab2d_row_norm_kernel);
// rim_tab_2d_grid_launch_table_norms is the form's rim_tab_launch_table_norms.
RimCoopKernelInfo rim_tab_2d_grid_coop_kernel(int problem);
void rim_tab_2d_grid_launch_integrand(unsigned grid, hipStream_t st, const PointArgs &pa, const double *d_norm, size_t count,
                                      const double *d_n, const double *d_gamma, double *d_out);
void rim_tab_2d_grid_launch_gamma_integral(unsigned grid, hipStream_t st, const PointArgs &pa, const double *d_norm, size_t count,
                                           const double *d_n, double *d_out, double *spill);
void rim_tab_2d_grid_launch_table_norms(unsigned grid, hipStream_t st, double *d_set, double *spill);

// The same for the 2-D forms with a sin^k xi prefactor: DIST_TABULATED_2D_PITCHY in rimphony_tab_2d_pitchy.hip,
// DIST_TABULATED_2D_GRID_PITCHY in rimphony_tab_2d_grid_pitchy.hip (one text, tab_2d_pitchy_unit.h).
RimCoopKernelInfo rim_tab_2d_pitchy_coop_kernel(int problem);
void rim_tab_2d_pitchy_launch_integrand(unsigned grid, hipStream_t st, const PointArgs &pa, const double *d_norm, size_t count,
                                        const double *d_n, const double *d_gamma, double *d_out);
void rim_tab_2d_pitchy_launch_gamma_integral(unsigned grid, hipStream_t st, const PointArgs &pa, const double *d_norm, size_t count,
                                             const double *d_n, double *d_out, double *spill);
void rim_tab_2d_pitchy_launch_table_norms(unsigned grid, hipStream_t st, double *d_set, double *spill);
RimCoopKernelInfo rim_tab_2d_grid_pitchy_coop_kernel(int problem);
void rim_tab_2d_grid_pitchy_launch_integrand(unsigned grid, hipStream_t st, const PointArgs &pa, const double *d_norm, size_t count,
                                             const double *d_n, const double *d_gamma, double *d_out);
void rim_tab_2d_grid_pitchy_launch_gamma_integral(unsigned grid, hipStream_t st, const PointArgs &pa, const double *d_norm, size_t count,
                                                  const double *d_n, double *d_out, double *spill);
void rim_tab_2d_grid_pitchy_launch_table_norms(unsigned grid, hipStream_t st, double *d_set, double *spill);

// The same for the 2-D form on given gamma and mu nodes: DIST_TABULATED_2D_NODES in rimphony_tab_2d_nodes.hip,
// DIST_TABULATED_2D_NODES_PITCHY in rimphony_tab_2d_nodes_pitchy.hip (the same text).
RimCoopKernelInfo rim_tab_2d_nodes_coop_kernel(int problem);
void rim_tab_2d_nodes_launch_integrand(unsigned grid, hipStream_t st, const PointArgs &pa, const double *d_norm, size_t count,
                                       const double *d_n, const double *d_gamma, double *d_out);
void rim_tab_2d_nodes_launch_gamma_integral(unsigned grid, hipStream_t st, const PointArgs &pa, const double *d_norm, size_t count,
                                            const double *d_n, double *d_out, double *spill);
void rim_tab_2d_nodes_launch_table_norms(unsigned grid, hipStream_t st, double *d_set, double *spill);
RimCoopKernelInfo rim_tab_2d_nodes_pitchy_coop_kernel(int problem);
void rim_tab_2d_nodes_pitchy_launch_integrand(unsigned grid, hipStream_t st, const PointArgs &pa, const double *d_norm, size_t count,
                                              const double *d_n, const double *d_gamma, double *d_out);
void rim_tab_2d_nodes_pitchy_launch_gamma_integral(unsigned grid, hipStream_t st, const PointArgs &pa, const double *d_norm, size_t count,
                                                   const double *d_n, double *d_out, double *spill);
void rim_tab_2d_nodes_pitchy_launch_table_norms(unsigned grid, hipStream_t st, double *d_set, double *spill);

// The same for a family of energy tables (a real index per row): DIST_TABULATED_FAMILY in rimphony_tab_family.hip,
// DIST_TABULATED_FAMILY_PITCHY in rimphony_tab_family_pitchy.hip (one text, tab_family_unit.h).  A family's normalisation is
// per row, norm_kernel's; with a prefactor the launch writes the rows' lines first, into pp.p[2] (tab_family_line).
RimCoopKernelInfo rim_tab_family_coop_kernel(int problem);
void rim_tab_family_launch_norm(unsigned grid, hipStream_t st, const ParamPtrs &pp, size_t n, double *d_norm, unsigned long long *queue,
                                double *spill);
void rim_tab_family_launch_integrand(unsigned grid, hipStream_t st, const PointArgs &pa, const double *d_norm, size_t count,
                                     const double *d_n, const double *d_gamma, double *d_out);
void rim_tab_family_launch_gamma_integral(unsigned grid, hipStream_t st, const PointArgs &pa, const double *d_norm, size_t count,
                                          const double *d_n, double *d_out, double *spill);
RimCoopKernelInfo rim_tab_family_pitchy_coop_kernel(int problem);
void rim_tab_family_pitchy_launch_norm(unsigned grid, hipStream_t st, const ParamPtrs &pp, size_t n, double *d_norm,
                                       unsigned long long *queue, double *spill);
void rim_tab_family_pitchy_launch_integrand(unsigned grid, hipStream_t st, const PointArgs &pa, const double *d_norm, size_t count,
                                            const double *d_n, const double *d_gamma, double *d_out);
void rim_tab_family_pitchy_launch_gamma_integral(unsigned grid, hipStream_t st, const PointArgs &pa, const double *d_norm, size_t count,
                                                 const double *d_n, double *d_out, double *spill);

// The same for a family of 2-D surfaces on given gamma and mu nodes: DIST_TABULATED_2D_FAMILY in rimphony_tab_2d_family.hip,
// DIST_TABULATED_2D_FAMILY_PITCHY in rimphony_tab_2d_family_pitchy.hip (one text, tab_2d_family_unit.h).  The normalisation is
// per row, norm_kernel's; both forms' launches write the rows' lines first, into pp.p[2] (tab_2d_family_line).
RimCoopKernelInfo rim_tab_2d_family_coop_kernel(int problem);
void rim_tab_2d_family_launch_norm(unsigned grid, hipStream_t st, const ParamPtrs &pp, size_t n, double *d_norm, unsigned long long *queue,
                                   double *spill);
void rim_tab_2d_family_launch_integrand(unsigned grid, hipStream_t st, const PointArgs &pa, const double *d_norm, size_t count,
                                        const double *d_n, const double *d_gamma, double *d_out);
void rim_tab_2d_family_launch_gamma_integral(unsigned grid, hipStream_t st, const PointArgs &pa, const double *d_norm, size_t count,
                                             const double *d_n, double *d_out, double *spill);
RimCoopKernelInfo rim_tab_2d_family_pitchy_coop_kernel(int problem);
void rim_tab_2d_family_pitchy_launch_norm(unsigned grid, hipStream_t st, const ParamPtrs &pp, size_t n, double *d_norm,
                                          unsigned long long *queue, double *spill);
void rim_tab_2d_family_pitchy_launch_integrand(unsigned grid, hipStream_t st, const PointArgs &pa, const double *d_norm, size_t count,
                                               const double *d_n, const double *d_gamma, double *d_out);
void rim_tab_2d_family_pitchy_launch_gamma_integral(unsigned grid, hipStream_t st, const PointArgs &pa, const double *d_norm, size_t count,
                                                    const double *d_n, double *d_out, double *spill);

// The same for such a family blended cubically across its tables: DIST_TABULATED_2D_FAMILY_CUBIC in
// rimphony_tab_2d_family_cubic.hip, DIST_TABULATED_2D_FAMILY_CUBIC_PITCHY in rimphony_tab_2d_family_cubic_pitchy.hip (the same
// text, tab_2d_family_unit.h); the rows' lines are 128 bytes each (tab_2d_family_cubic_line).
RimCoopKernelInfo rim_tab_2d_family_cubic_coop_kernel(int problem);
void rim_tab_2d_family_cubic_launch_norm(unsigned grid, hipStream_t st, const ParamPtrs &pp, size_t n, double *d_norm, unsigned long long *queue,
                                         double *spill);
void rim_tab_2d_family_cubic_launch_integrand(unsigned grid, hipStream_t st, const PointArgs &pa, const double *d_norm, size_t count,
                                              const double *d_n, const double *d_gamma, double *d_out);
void rim_tab_2d_family_cubic_launch_gamma_integral(unsigned grid, hipStream_t st, const PointArgs &pa, const double *d_norm, size_t count,
                                                   const double *d_n, double *d_out, double *spill);
RimCoopKernelInfo rim_tab_2d_family_cubic_pitchy_coop_kernel(int problem);
void rim_tab_2d_family_cubic_pitchy_launch_norm(unsigned grid, hipStream_t st, const ParamPtrs &pp, size_t n, double *d_norm,
                                                unsigned long long *queue, double *spill);
void rim_tab_2d_family_cubic_pitchy_launch_integrand(unsigned grid, hipStream_t st, const PointArgs &pa, const double *d_norm, size_t count,
                                                     const double *d_n, const double *d_gamma, double *d_out);
void rim_tab_2d_family_cubic_pitchy_launch_gamma_integral(unsigned grid, hipStream_t st, const PointArgs &pa, const double *d_norm, size_t count,
                                                          const double *d_n, double *d_out, double *spill);

// A 2-D set installed from device memory (rimphony_tab_install.hip, tab_install.h): *d_flag, zeroed by the caller, becomes 1
// where one of the `count` values at d_log_n is not finite; the three families of sweeps that fill the node data of `s`, in
// order on `st`.  Enqueue only, as everything here.
void rim_tab_install_launch_finite(hipStream_t st, const double *d_log_n, size_t count, unsigned *d_flag);
void rim_tab_install_launch_sweeps(hipStream_t st, const RimTabInstall &s);

// RimCoopKernelInfo of coop_kernel<P>, `fn`
template <class P>
RimCoopKernelInfo rim_coop_info(const void *fn)
{
    RimCoopKernelInfo k;
    k.fn = fn;
    k.waves = (int) P::WAVES; k.early_help = P::EARLY_HELP != 0; k.early_squad = (unsigned) P::EARLY_SQUAD;
    return k;
}

#endif
