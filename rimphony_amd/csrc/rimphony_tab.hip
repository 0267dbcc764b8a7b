// rimphony_tab.hip -- the kernels of the tabulated distribution (RIMPHONY_TABULATED; gfx950 only): its normalisation,
// the one-wave-per-coefficient Symphony and Faraday kernels and the two unit seams of coop_kernel.h.  The kind never runs
// on the group kernel (rimphony_group.hip keeps its four instantiations); a sample reads its four spline words with plain
// global loads -- a 4096-node table is 64 KB and stays in cache.  A table with a pitch-angle factor g(cos xi) reads four more
// from its pitch row, whose address travels in par[0] (dev_symphony.h: dist_prepare<DIST_TABULATED>, tab_pitch_spline).
// The two persistent kernels exist twice: for sets with pitch rows and, "no pitch row" known at compile time, for sets without.
#include <hip/hip_runtime.h>
#include "coop_kernel.h"
#include "tab_launch.h"

template <class P>
static RimCoopKernelInfo coop_info()
{
    RimCoopKernelInfo k;
    k.fn = reinterpret_cast<const void *>(coop_kernel<P>);
    k.waves = (int) P::WAVES; k.early_help = P::EARLY_HELP != 0; k.early_squad = (unsigned) P::EARLY_SQUAD;
    return k;
}

// A set without pitch rows runs the instantiations that know so at compile time (DIST_TABULATED_ISO): the code isotropic
// tables had before the pitch factor existed.  Same bits either way.
RimCoopKernelInfo rim_tab_coop_kernel(int problem, bool pitch)
{
    if (problem) return pitch ? coop_info<HeyvaertsProblem<DIST_TABULATED>>() : coop_info<HeyvaertsProblem<DIST_TABULATED_ISO>>();
    return pitch ? coop_info<SymphonyProblem<DIST_TABULATED>>() : coop_info<SymphonyProblem<DIST_TABULATED_ISO>>();
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
