// rimphony_tab.hip -- the kernels of the tabulated distribution (RIMPHONY_TABULATED; gfx950 only): its normalisation,
// the one-wave-per-coefficient Symphony and Faraday kernels and the two unit seams of coop_kernel.h.  The kind never runs
// on the group kernel (rimphony_group.hip keeps its four instantiations); a sample reads its four spline words with plain
// global loads -- a 4096-node table is 64 KB and stays in cache.
#include <hip/hip_runtime.h>
#include "coop_kernel.h"
#include "tab_launch.h"

RimCoopKernelInfo rim_tab_coop_kernel(int problem)
{
    RimCoopKernelInfo k;
    if (problem) {
        typedef HeyvaertsProblem<DIST_TABULATED> P;
        k.fn = reinterpret_cast<const void *>(coop_kernel<P>);
        k.waves = (int) P::WAVES; k.early_help = P::EARLY_HELP != 0; k.early_squad = (unsigned) P::EARLY_SQUAD;
    } else {
        typedef SymphonyProblem<DIST_TABULATED> P;
        k.fn = reinterpret_cast<const void *>(coop_kernel<P>);
        k.waves = (int) P::WAVES; k.early_help = P::EARLY_HELP != 0; k.early_squad = (unsigned) P::EARLY_SQUAD;
    }
    return k;
}

void rim_tab_launch_norm(unsigned grid, hipStream_t st, const ParamPtrs &pp, size_t n, double *d_norm, unsigned long long *queue,
                         double *spill)
{
    hipLaunchKernelGGL(norm_kernel<DIST_TABULATED>, dim3(grid), dim3(64), RIM_DYN_LDS, st, pp, n, d_norm, queue, spill);
}

void rim_tab_launch_integrand(unsigned grid, hipStream_t st, const PointArgs &pa, const double *d_norm, size_t count,
                              const double *d_n, const double *d_gamma, double *d_out)
{
    hipLaunchKernelGGL(integrand_kernel_n<DIST_TABULATED>, dim3(grid), dim3(64), RIM_DYN_LDS, st, pa, d_norm, count, d_n, d_gamma, d_out);
}

void rim_tab_launch_gamma_integral(unsigned grid, hipStream_t st, const PointArgs &pa, const double *d_norm, size_t count,
                                   const double *d_n, double *d_out, double *spill)
{
    hipLaunchKernelGGL(gamma_integral_kernel<DIST_TABULATED>, dim3(grid), dim3(64), RIM_DYN_LDS, st, pa, d_norm, count, d_n, d_out, spill);
}
