// tab_2d_pitchy_unit.h -- the text of the two units that hold the kernels of a 2-D table set with a sin^k xi prefactor
// (rimphony_tab_2d_pitchy.hip: DIST_TABULATED_2D_PITCHY; rimphony_tab_2d_grid_pitchy.hip: DIST_TABULATED_2D_GRID_PITCHY).  The
// unit defines RIM_T2P_KIND, the name of its norm kernel and the names of its four host functions (tab_launch.h), then
// includes this: the two differ in the form alone.  The units of the 2-D form on given gamma and mu nodes include it too
// (rimphony_tab_2d_nodes.hip: DIST_TABULATED_2D_NODES, whose nbar has no factor and no end-cell treatment;
// rimphony_tab_2d_nodes_pitchy.hip: DIST_TABULATED_2D_NODES_PITCHY): nothing below depends on the prefactor.
//
// The normalisation of every table, one wave per table: norm = 1 / (4 pi int nbar dgamma) over the table's range with the
// settings of norm_kernel (eps_rel 1e-8, 1000 subintervals), nbar(gamma) = 1/2 int (1 - mu^2)^(k/2) exp(S) dmu by the Kronrod
// rule on every mu cell, the two end cells under 1 - |mu| = h v^4 (dev_symphony.h: tab_2d_norm_integrand).  Written into the
// table's header, the word a 2-D table keeps it in; a quadrature that fails leaves NaN there, for that table only.
#include <hip/hip_runtime.h>
#include "coop_kernel.h"
#include "tab_launch.h"
#include "gk31_table.h"

static __device__ const double c_tab_xgk[32] = RIM_GK31_X;
static __device__ const double c_tab_wgk[32] = RIM_GK31_WK;

__global__ __launch_bounds__(64) void RIM_T2P_NORM_KERNEL(double *set, double *spill_base)
{
    __shared__ double s_tab[96];
    __shared__ double s_store[RIM_ISTORE_DOUBLES(CAP_NORM)];
    const GKLane g = gk_lane_init(s_tab);
    const IStore st = istore_carve(s_store, CAP_NORM, spill_base + (size_t) blockIdx.x * SPILL_DOUBLES_PER_WAVE, SPILL_INNER);
    __shared__ QagPark s_qpark;
    if (threadIdx.x == 0) { s_qpark.ctr = WaveCounters{0, 0, 0}; s_qpark.hb = nullptr; }
    const size_t n_tables = (size_t) set[TAB_HDR_NTABLES];
    for (size_t t = blockIdx.x; t < n_tables; t += gridDim.x) {
        DistParams d;
        d.par[0] = (double) t;
        d.par[1] = rim_frombits((uint64_t) (uintptr_t) set);
        d.par[2] = 0.; d.par[3] = 0.; d.par[4] = 0.;
        dist_prepare<RIM_T2P_KIND>(d, RIM_NAN);
        auto f = [&](double x, bool active) -> double {
            return active ? tab_2d_norm_integrand<RIM_T2P_KIND>(d, x, c_tab_xgk, c_tab_wgk) : 0.;
        };
        QagState q;
        wave_qag(f, g, st, d.inv_kappa_width, d.neg_inverse_t, 0., 1e-8, 1000, q, &s_qpark);
        double v = RIM_NAN;
        if (q.status == QAG_SUCCESS) v = 1. / (2. * RIM_TWO_PI * q.result);
        if (g.lane == 0) set[TAB_HDR_DOUBLES + t * TAB_2D_HDR + TAB_2D_NORM] = v;
    }
}

void RIM_T2P_LAUNCH_TABLE_NORMS(unsigned grid, hipStream_t st, double *d_set, double *spill)
{
    hipLaunchKernelGGL(RIM_T2P_NORM_KERNEL, dim3(grid), dim3(64), RIM_DYN_LDS, st, d_set, spill);
}

RimCoopKernelInfo RIM_T2P_COOP_KERNEL(int problem)
{
    typedef SymphonyProblem<RIM_T2P_KIND> S;
    typedef HeyvaertsProblem<RIM_T2P_KIND> H;
    return problem ? rim_coop_info<H>(reinterpret_cast<const void *>(coop_kernel<H>))
                   : rim_coop_info<S>(reinterpret_cast<const void *>(coop_kernel<S>));
}

void RIM_T2P_LAUNCH_INTEGRAND(unsigned grid, hipStream_t st, const PointArgs &pa, const double *d_norm, size_t count,
                              const double *d_n, const double *d_gamma, double *d_out)
{
    hipLaunchKernelGGL(integrand_kernel_n<RIM_T2P_KIND>, dim3(grid), dim3(64), RIM_DYN_LDS, st, pa, d_norm, count, d_n, d_gamma, d_out);
}

void RIM_T2P_LAUNCH_GAMMA_INTEGRAL(unsigned grid, hipStream_t st, const PointArgs &pa, const double *d_norm, size_t count,
                                   const double *d_n, double *d_out, double *spill)
{
    hipLaunchKernelGGL(gamma_integral_kernel<RIM_T2P_KIND>, dim3(grid), dim3(64), RIM_DYN_LDS, st, pa, d_norm, count, d_n, d_out, spill);
}
