// tab_family_unit.h -- the text of the two units that hold the kernels of a FAMILY of energy tables, where a row of a batch
// names a real index and every sample blends two tables (rimphony_tab_family.hip: DIST_TABULATED_FAMILY, isotropic;
// rimphony_tab_family_pitchy.hip: DIST_TABULATED_FAMILY_PITCHY, with a sin^k xi prefactor per table).  The unit defines
// RIM_TF_KIND and the names of its four host functions (tab_launch.h), then includes this: the two differ in the form alone.
//
// The normalisation is per row, norm_kernel's: the gamma integral runs over the blended spline.  With a prefactor a prologue
// kernel writes one 64-byte line per row first -- {k, 0, w, spare | 0, 0, 0, P(k)}, the blended k and the closed form at it
// (dev_symphony.h: tab_family_line) --, which norm_kernel and every later kernel of the batch read as they read the header
// of a sin^k table.
#include <hip/hip_runtime.h>
#include "coop_kernel.h"
#include "tab_launch.h"

#if RIM_TF_KIND == 15
// one thread per row.  A row whose index names no table gets k of table 0 and a NaN P; norm_kernel gives it a NaN anyway.
__global__ void tab_family_lines_kernel(ParamPtrs pp, size_t n, double *lines)
{
    const size_t i = (size_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double *set = pp.p[1];
    size_t a;
    double w;
    const bool ok = tab_family_row(set, pp.p[0][i], a, w);
    const double k = tab_family_k(set, a, w);
    tab_family_line(lines + i * TAB_FAMILY_LINE, k, w, ok ? hyperg_2F1_at_1(0.5, -0.5 * k, 1.5) : RIM_NAN);
}
#endif

void RIM_TF_LAUNCH_NORM(unsigned grid, hipStream_t st, const ParamPtrs &pp, size_t n, double *d_norm, unsigned long long *queue,
                        double *spill)
{
#if RIM_TF_KIND == 15
    hipLaunchKernelGGL(tab_family_lines_kernel, dim3((unsigned) ((n + 255) / 256)), dim3(256), RIM_DYN_LDS, st, pp, n,
                       const_cast<double *>(pp.p[2]));
#endif
    hipLaunchKernelGGL(norm_kernel<RIM_TF_KIND>, dim3(grid), dim3(64), RIM_DYN_LDS, st, pp, n, d_norm, queue, spill);
}

RimCoopKernelInfo RIM_TF_COOP_KERNEL(int problem)
{
    typedef SymphonyProblem<RIM_TF_KIND> S;
    typedef HeyvaertsProblem<RIM_TF_KIND> H;
    return problem ? rim_coop_info<H>(reinterpret_cast<const void *>(coop_kernel<H>))
                   : rim_coop_info<S>(reinterpret_cast<const void *>(coop_kernel<S>));
}

void RIM_TF_LAUNCH_INTEGRAND(unsigned grid, hipStream_t st, const PointArgs &pa, const double *d_norm, size_t count,
                             const double *d_n, const double *d_gamma, double *d_out)
{
    hipLaunchKernelGGL(integrand_kernel_n<RIM_TF_KIND>, dim3(grid), dim3(64), RIM_DYN_LDS, st, pa, d_norm, count, d_n, d_gamma, d_out);
}

void RIM_TF_LAUNCH_GAMMA_INTEGRAL(unsigned grid, hipStream_t st, const PointArgs &pa, const double *d_norm, size_t count,
                                  const double *d_n, double *d_out, double *spill)
{
    hipLaunchKernelGGL(gamma_integral_kernel<RIM_TF_KIND>, dim3(grid), dim3(64), RIM_DYN_LDS, st, pa, d_norm, count, d_n, d_out, spill);
}
