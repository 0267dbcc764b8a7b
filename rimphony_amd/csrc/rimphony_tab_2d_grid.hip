// rimphony_tab_2d_grid.hip -- the kernels of the tabulated distribution as a 2-D set on given gamma nodes
// (rimphony_ctx_set_tables_2d_grid, DIST_TABULATED_2D_GRID; gfx950 only): the normalisation of the set's tables, the
// one-wave-per-coefficient Symphony and Faraday kernels and the two unit seams of coop_kernel.h.  A sample reads two guide
// words, bisects over the set's u nodes, reads the 32 bytes of the interval's two u nodes and then what a sample of a 2-D set
// reads, two runs of 64 bytes, for one bicubic with the cell's own step (dev_symphony.h: tab_bicubic_grid).
//
// A translation unit of its own: rimphony_tab.hip keeps its kernels instruction for instruction, and its dispatches hand this
// form on to the functions here (tab_launch.h).  The form's group kernel is rimphony_tab_2d_grid_group.hip's.
#include <hip/hip_runtime.h>
#include "coop_kernel.h"
#include "tab_launch.h"
#include "gk31_table.h"

static __device__ const double c_tab_xgk[32] = RIM_GK31_X;
static __device__ const double c_tab_wgk[32] = RIM_GK31_WK;

// tab2d_table_norm_kernel (rimphony_tab.hip) for this form, one wave per table: norm = 1 / (4 pi int nbar dgamma) over
// [gamma_0, gamma_last] with the settings of norm_kernel (eps_rel 1e-8, 1000 subintervals), nbar by the Kronrod rule on every
// mu cell through the form's bicubic.  Written into the table's header, the word a 2-D table keeps it in; a quadrature that
// fails leaves NaN there, for that table only.
__global__ __launch_bounds__(64) void tab2d_grid_table_norm_kernel(double *set, double *spill_base)
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
        dist_prepare<DIST_TABULATED_2D_GRID>(d, RIM_NAN);
        auto f = [&](double x, bool active) -> double {
            return active ? tab_2d_norm_integrand<DIST_TABULATED_2D_GRID>(d, x, c_tab_xgk, c_tab_wgk) : 0.;
        };
        QagState q;
        wave_qag(f, g, st, d.inv_kappa_width, d.neg_inverse_t, 0., 1e-8, 1000, q, &s_qpark);
        double v = RIM_NAN;
        if (q.status == QAG_SUCCESS) v = 1. / (2. * RIM_TWO_PI * q.result);
        if (g.lane == 0) set[TAB_HDR_DOUBLES + t * TAB_2D_HDR + TAB_2D_NORM] = v;
    }
}

void rim_tab_2d_grid_launch_table_norms(unsigned grid, hipStream_t st, double *d_set, double *spill)
{
    hipLaunchKernelGGL(tab2d_grid_table_norm_kernel, dim3(grid), dim3(64), RIM_DYN_LDS, st, d_set, spill);
}

RimCoopKernelInfo rim_tab_2d_grid_coop_kernel(int problem)
{
    typedef SymphonyProblem<DIST_TABULATED_2D_GRID> S;
    typedef HeyvaertsProblem<DIST_TABULATED_2D_GRID> H;
    return problem ? rim_coop_info<H>(reinterpret_cast<const void *>(coop_kernel<H>))
                   : rim_coop_info<S>(reinterpret_cast<const void *>(coop_kernel<S>));
}

void rim_tab_2d_grid_launch_integrand(unsigned grid, hipStream_t st, const PointArgs &pa, const double *d_norm, size_t count,
                                      const double *d_n, const double *d_gamma, double *d_out)
{
    hipLaunchKernelGGL(integrand_kernel_n<DIST_TABULATED_2D_GRID>, dim3(grid), dim3(64), RIM_DYN_LDS, st, pa, d_norm, count, d_n,
                       d_gamma, d_out);
}

void rim_tab_2d_grid_launch_gamma_integral(unsigned grid, hipStream_t st, const PointArgs &pa, const double *d_norm, size_t count,
                                           const double *d_n, double *d_out, double *spill)
{
    hipLaunchKernelGGL(gamma_integral_kernel<DIST_TABULATED_2D_GRID>, dim3(grid), dim3(64), RIM_DYN_LDS, st, pa, d_norm, count, d_n,
                       d_out, spill);
}
