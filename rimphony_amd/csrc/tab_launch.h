// tab_launch.h -- what rimphony_hip.hip asks of rimphony_tab.hip, the translation unit that holds the kernels of the
// tabulated distribution (coop_kernel.h says why they have a unit of their own).
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

// coop_kernel<SymphonyProblem<K>> (problem 0) or coop_kernel<HeyvaertsProblem<K>> (1); K = DIST_TABULATED for a table set with
// pitch rows, DIST_TABULATED_ISO (dev_symphony.h) for one without
RimCoopKernelInfo rim_tab_coop_kernel(int problem, bool pitch);
// norm_kernel, integrand_kernel_n and gamma_integral_kernel of the kind: enqueue only, the caller asks hipGetLastError()
void rim_tab_launch_norm(unsigned grid, hipStream_t st, const ParamPtrs &pp, size_t n, double *d_norm, unsigned long long *queue,
                         double *spill);
void rim_tab_launch_integrand(unsigned grid, hipStream_t st, const PointArgs &pa, const double *d_norm, size_t count,
                              const double *d_n, const double *d_gamma, double *d_out);
void rim_tab_launch_gamma_integral(unsigned grid, hipStream_t st, const PointArgs &pa, const double *d_norm, size_t count,
                                   const double *d_n, double *d_out, double *spill);

#endif
