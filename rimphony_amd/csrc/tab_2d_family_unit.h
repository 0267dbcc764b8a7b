// tab_2d_family_unit.h -- the text of the two units that hold the kernels of a FAMILY of 2-D surfaces on given gamma and mu
// nodes, where a row of a batch names a real index and every sample blends two tables (rimphony_tab_2d_family.hip:
// DIST_TABULATED_2D_FAMILY; rimphony_tab_2d_family_pitchy.hip: DIST_TABULATED_2D_FAMILY_PITCHY, with a sin^k xi prefactor per
// table).  The unit defines RIM_T2F_KIND and the names of its four host functions (tab_launch.h), then includes this: the two
// differ in the form alone.
//
// A prologue kernel writes one 64-byte line per batch row, laid out as a table header (dev_symphony.h: tab_2d_family_line):
// the mu geometry, the weight, the blended k, the way from the line to the set's mu guide and mu nodes and the distance to the
// upper table.  The normalisation is per row, norm_kernel's, over the blended surface: norm = 1 / (4 pi int nbar dgamma) with
// nbar(gamma) = 1/2 int (1 - mu^2)^(k/2) exp(S) dmu by the Kronrod rule on every mu cell, the end cells of a set with a
// prefactor under 1 - |mu| = h v^4 -- the quadrature the plain form runs once per table as the set comes in
// (tab_2d_pitchy_unit.h), run here once per row.  Every later kernel of the batch reads the line as it reads a table's header.
//
// The units of the CUBIC blend across the tables include this too (rimphony_tab_2d_family_cubic.hip:
// DIST_TABULATED_2D_FAMILY_CUBIC; rimphony_tab_2d_family_cubic_pitchy.hip: DIST_TABULATED_2D_FAMILY_CUBIC_PITCHY): their
// prologue writes a 128-byte line per row -- the same eight words, then the four Lagrange weights, the stencil's base table
// and the row's parameter (tab_2d_family_cubic_line) --, and a sample blends four tables (tab_bicubic_family_cubic).
#include <hip/hip_runtime.h>
#include "coop_kernel.h"
#include "tab_launch.h"
#include "gk31_table.h"

static __device__ const double c_tab_xgk[32] = RIM_GK31_X;
static __device__ const double c_tab_wgk[32] = RIM_GK31_WK;

template <int KIND>
__device__ double tab_2d_family_nbar(const DistParams &d, double g)
{
    return tab_2d_norm_integrand<KIND>(d, g, c_tab_xgk, c_tab_wgk);
}

// one thread per row.  A row whose index names no table gets the line of table 0 at weight 0; norm_kernel gives it a NaN.
// (A template, so that the two units each have one of their own.)
template <int KIND>
__global__ void tab_2d_family_lines_kernel(ParamPtrs pp, size_t n, double *lines)
{
    const size_t i = (size_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double *set = pp.p[1];
    size_t a;
    double w;
    tab_family_row(set, pp.p[0][i], a, w);
    if constexpr (tab_kind_2d_family_cubic(KIND)) tab_2d_family_cubic_line(lines + i * TAB_2D_CUBIC_LINE, set, a, w);
    else tab_2d_family_line(lines + i * TAB_2D_HDR, set, a, w);
}

void RIM_T2F_LAUNCH_NORM(unsigned grid, hipStream_t st, const ParamPtrs &pp, size_t n, double *d_norm, unsigned long long *queue,
                         double *spill)
{
    hipLaunchKernelGGL(tab_2d_family_lines_kernel<RIM_T2F_KIND>, dim3((unsigned) ((n + 255) / 256)), dim3(256), RIM_DYN_LDS, st, pp, n,
                       const_cast<double *>(pp.p[2]));
    hipLaunchKernelGGL(norm_kernel<RIM_T2F_KIND>, dim3(grid), dim3(64), RIM_DYN_LDS, st, pp, n, d_norm, queue, spill);
}

RimCoopKernelInfo RIM_T2F_COOP_KERNEL(int problem)
{
    typedef SymphonyProblem<RIM_T2F_KIND> S;
    typedef HeyvaertsProblem<RIM_T2F_KIND> H;
    return problem ? rim_coop_info<H>(reinterpret_cast<const void *>(coop_kernel<H>))
                   : rim_coop_info<S>(reinterpret_cast<const void *>(coop_kernel<S>));
}

void RIM_T2F_LAUNCH_INTEGRAND(unsigned grid, hipStream_t st, const PointArgs &pa, const double *d_norm, size_t count,
                              const double *d_n, const double *d_gamma, double *d_out)
{
    hipLaunchKernelGGL(integrand_kernel_n<RIM_T2F_KIND>, dim3(grid), dim3(64), RIM_DYN_LDS, st, pa, d_norm, count, d_n, d_gamma, d_out);
}

void RIM_T2F_LAUNCH_GAMMA_INTEGRAL(unsigned grid, hipStream_t st, const PointArgs &pa, const double *d_norm, size_t count,
                                   const double *d_n, double *d_out, double *spill)
{
    hipLaunchKernelGGL(gamma_integral_kernel<RIM_T2F_KIND>, dim3(grid), dim3(64), RIM_DYN_LDS, st, pa, d_norm, count, d_n, d_out, spill);
}
