// rimphony_tab.hip -- the kernels of the tabulated distribution (RIMPHONY_TABULATED; gfx950 only): its normalisation,
// the one-wave-per-coefficient Symphony and Faraday kernels and the two unit seams of coop_kernel.h.  The kind's group
// kernels -- the Symphony coefficients of a point in lock-step -- have a unit of their own, rimphony_tab_group.hip
// (rimphony_group.hip keeps its four instantiations); which of the two runs the Symphony slots of a form is
// RIM_TAB_GROUP_DEFAULT's and RIMPHONY_TAB_GROUP's matter (rimphony_hip.hip).  Every host function here takes the form of the
// installed set as its DIST_TABULATED* value and is one dispatch over it (rimphony_internal.h: rim_with_tab_kind).  A sample reads its four spline words with plain
// global loads -- a 4096-node table is 64 KB and stays in cache.  A table with a pitch-angle factor g(cos xi) reads four more
// from its pitch row, whose address travels in par[0] (dev_symphony.h: dist_prepare<DIST_TABULATED>, tab_pitch_spline).
// The two persistent kernels exist twice: for sets with pitch rows and, "no pitch row" known at compile time, for sets without.
// A 2-D set, ln n(gamma, mu) on a grid, runs a third family (DIST_TABULATED_2D): a sample reads two runs of 64 bytes, the
// nodes (i, j), (i, j + 1) and (i + 1, j), (i + 1, j + 1), and evaluates one bicubic (tab_bicubic).  Its normalisation is a
// property of the table: tab2d_table_norm_kernel integrates it once, when the set is installed, and a row's normalisation
// is a load (tab2d_row_norm_kernel).
// A set with a sin^k xi prefactor runs a fourth family (DIST_TABULATED_PITCHY): k is one more wave-uniform load from the
// table's header.  Where its tables have a g, P = 1/2 int (1 - mu^2)^(k/2) g dmu is integrated adaptively when the set is
// installed (tab_pitchy_table_p_kernel): the integrand's derivative is singular at both ends for a non-integer k.
// A set on given gamma nodes runs a fifth (DIST_TABULATED_GRID): the sin^k family with tab_spline_grid for the energy
// table -- two guide words, a short bisection over the nodes' u_j, then the 64 bytes of the interval's two nodes.
// A 2-D set on given gamma nodes (DIST_TABULATED_2D_GRID) has its kernels in a unit of its own, rimphony_tab_2d_grid.hip, for the
// reason the group kernels have theirs; the dispatches here hand the form on.  Its rows read their normalisation with
// tab2d_row_norm_kernel, as a 2-D set's do.
// The 2-D forms with a sin^k xi prefactor (DIST_TABULATED_2D_PITCHY, DIST_TABULATED_2D_GRID_PITCHY) likewise:
// rimphony_tab_2d_pitchy.hip, rimphony_tab_2d_grid_pitchy.hip.  And the 2-D form on given gamma and mu nodes
// (DIST_TABULATED_2D_NODES, DIST_TABULATED_2D_NODES_PITCHY): rimphony_tab_2d_nodes.hip, rimphony_tab_2d_nodes_pitchy.hip.
// And the families of energy tables, where a row names a real index and a sample blends two tables (DIST_TABULATED_FAMILY,
// DIST_TABULATED_FAMILY_PITCHY): rimphony_tab_family.hip, rimphony_tab_family_pitchy.hip, norm_kernel included.
// And the families of 2-D surfaces on given nodes (DIST_TABULATED_2D_FAMILY, DIST_TABULATED_2D_FAMILY_PITCHY):
// rimphony_tab_2d_family.hip, rimphony_tab_2d_family_pitchy.hip, norm_kernel included.
// And the same families blended cubically across their tables (DIST_TABULATED_2D_FAMILY_CUBIC, .._CUBIC_PITCHY):
// rimphony_tab_2d_family_cubic.hip, rimphony_tab_2d_family_cubic_pitchy.hip, norm_kernel included.
#include <hip/hip_runtime.h>
#include "coop_kernel.h"
#include "tab_launch.h"
#include "gk31_table.h"

static __device__ const double c_tab_xgk[32] = RIM_GK31_X;
static __device__ const double c_tab_wgk[32] = RIM_GK31_WK;

// The normalisation of every table of a 2-D set, one wave per table: norm = 1 / (4 pi int nbar dgamma) over the table's
// range with the settings of norm_kernel (eps_rel 1e-8, 1000 subintervals), nbar(gamma) = 1/2 int exp(S) dmu by the Kronrod
// rule on every mu cell (tab_2d_norm_integrand).  Written into the table's header; a quadrature that fails leaves NaN
// there, for that table only.
__global__ __launch_bounds__(64) void tab2d_table_norm_kernel(double *set, double *spill_base)
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
        dist_prepare<DIST_TABULATED_2D>(d, RIM_NAN);
        auto f = [&](double x, bool active) -> double {
            return active ? tab_2d_norm_integrand(d, x, c_tab_xgk, c_tab_wgk) : 0.;
        };
        QagState q;
        wave_qag(f, g, st, d.inv_kappa_width, d.neg_inverse_t, 0., 1e-8, 1000, q, &s_qpark);
        double v = RIM_NAN;
        if (q.status == QAG_SUCCESS) v = 1. / (2. * RIM_TWO_PI * q.result);
        if (g.lane == 0) set[TAB_HDR_DOUBLES + t * TAB_2D_HDR + TAB_2D_NORM] = v;
    }
}

// the normalisation of the rows of a batch on a 2-D set: the table's, or NaN for an index that names no table
__global__ void tab2d_row_norm_kernel(ParamPtrs pp, size_t n, double *norm)
{
    const size_t i = (size_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double *set = pp.p[1];
    const double idx = pp.p[0][i];
    norm[i] = tab_row_ok(set, idx) ? set[TAB_HDR_DOUBLES + (size_t) idx * TAB_2D_HDR + TAB_2D_NORM] : RIM_NAN;
}

void rim_tab_launch_table_norms(unsigned grid, hipStream_t st, double *d_set, double *spill)
{
    hipLaunchKernelGGL(tab2d_table_norm_kernel, dim3(grid), dim3(64), RIM_DYN_LDS, st, d_set, spill);
}

// P of every table of a sin^k set with pitch rows, one wave per table: 1/2 int_-1^+1 (1 - mu^2)^(k/2) exp(G(mu)) dmu,
// eps_rel 1e-8, 1000 subintervals.  Written into the table's header; a quadrature that fails leaves NaN there, for that
// table only, and norm_kernel hands it on to the table's rows.
__global__ __launch_bounds__(64) void tab_pitchy_table_p_kernel(double *set, double *spill_base)
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
        dist_prepare<DIST_TABULATED_PITCHY>(d, RIM_NAN);
        auto f = [&](double x, bool active) -> double { return active ? tab_pitchy_p_integrand(d, x) : 0.; };
        QagState q;
        wave_qag(f, g, st, -1., 1., 0., 1e-8, 1000, q, &s_qpark);
        double v = RIM_NAN;
        if (q.status == QAG_SUCCESS) v = 0.5 * q.result;
        if (g.lane == 0) ((double *) (uintptr_t) rim_bits(d.par[0]))[TAB_PITCH_P] = v;
    }
}

void rim_tab_launch_pitchy_p(unsigned grid, hipStream_t st, double *d_set, double *spill)
{
    hipLaunchKernelGGL(tab_pitchy_table_p_kernel, dim3(grid), dim3(64), RIM_DYN_LDS, st, d_set, spill);
}

template <class P>
static RimCoopKernelInfo coop_info() { return rim_coop_info<P>(reinterpret_cast<const void *>(coop_kernel<P>)); }

// A set without pitch rows runs the instantiations that know so at compile time (DIST_TABULATED_ISO): the code isotropic
// tables had before the pitch factor existed.  Same bits either way.
RimCoopKernelInfo rim_tab_coop_kernel(int problem, int tab_kind)
{
    return rim_with_tab_kind(tab_kind, [&](auto K) {
        constexpr int KIND = decltype(K)::value;
        if constexpr (KIND == DIST_TABULATED_2D_GRID) return rim_tab_2d_grid_coop_kernel(problem);
        else if constexpr (KIND == DIST_TABULATED_2D_PITCHY) return rim_tab_2d_pitchy_coop_kernel(problem);
        else if constexpr (KIND == DIST_TABULATED_2D_GRID_PITCHY) return rim_tab_2d_grid_pitchy_coop_kernel(problem);
        else if constexpr (KIND == DIST_TABULATED_2D_NODES) return rim_tab_2d_nodes_coop_kernel(problem);
        else if constexpr (KIND == DIST_TABULATED_2D_NODES_PITCHY) return rim_tab_2d_nodes_pitchy_coop_kernel(problem);
        else if constexpr (KIND == DIST_TABULATED_FAMILY) return rim_tab_family_coop_kernel(problem);
        else if constexpr (KIND == DIST_TABULATED_FAMILY_PITCHY) return rim_tab_family_pitchy_coop_kernel(problem);
        else if constexpr (KIND == DIST_TABULATED_2D_FAMILY) return rim_tab_2d_family_coop_kernel(problem);
        else if constexpr (KIND == DIST_TABULATED_2D_FAMILY_PITCHY) return rim_tab_2d_family_pitchy_coop_kernel(problem);
        else if constexpr (KIND == DIST_TABULATED_2D_FAMILY_CUBIC) return rim_tab_2d_family_cubic_coop_kernel(problem);
        else if constexpr (KIND == DIST_TABULATED_2D_FAMILY_CUBIC_PITCHY) return rim_tab_2d_family_cubic_pitchy_coop_kernel(problem);
        else return problem ? coop_info<HeyvaertsProblem<KIND>>() : coop_info<SymphonyProblem<KIND>>();
    });
}

// The next three kernels have no DIST_TABULATED_ISO instantiation: an isotropic set runs DIST_TABULATED's
// (rim_tab_seam_kind).  The rows of a 2-D set read their table's normalisation; no norm_kernel exists for that form.
void rim_tab_launch_norm(int tab_kind, unsigned grid, hipStream_t st, const ParamPtrs &pp, size_t n, double *d_norm,
                         unsigned long long *queue, double *spill)
{
    rim_with_tab_kind(tab_kind, [&](auto K) {
        constexpr int KIND = rim_tab_seam_kind(decltype(K)::value);
        if constexpr (tab_kind_2d_uniform(KIND) || tab_kind_2d_on_grid(KIND) || tab_kind_2d_nodes(KIND))
            hipLaunchKernelGGL(tab2d_row_norm_kernel, dim3((unsigned) ((n + 255) / 256)), dim3(256), RIM_DYN_LDS, st, pp, n, d_norm);
        else if constexpr (KIND == DIST_TABULATED_FAMILY) rim_tab_family_launch_norm(grid, st, pp, n, d_norm, queue, spill);
        else if constexpr (KIND == DIST_TABULATED_FAMILY_PITCHY) rim_tab_family_pitchy_launch_norm(grid, st, pp, n, d_norm, queue, spill);
        else if constexpr (KIND == DIST_TABULATED_2D_FAMILY) rim_tab_2d_family_launch_norm(grid, st, pp, n, d_norm, queue, spill);
        else if constexpr (KIND == DIST_TABULATED_2D_FAMILY_PITCHY) rim_tab_2d_family_pitchy_launch_norm(grid, st, pp, n, d_norm, queue, spill);
        else if constexpr (KIND == DIST_TABULATED_2D_FAMILY_CUBIC) rim_tab_2d_family_cubic_launch_norm(grid, st, pp, n, d_norm, queue, spill);
        else if constexpr (KIND == DIST_TABULATED_2D_FAMILY_CUBIC_PITCHY) rim_tab_2d_family_cubic_pitchy_launch_norm(grid, st, pp, n, d_norm, queue, spill);
        else
            hipLaunchKernelGGL(norm_kernel<KIND>, dim3(grid), dim3(64), RIM_DYN_LDS, st, pp, n, d_norm, queue, spill);
    });
}

void rim_tab_launch_integrand(int tab_kind, unsigned grid, hipStream_t st, const PointArgs &pa, const double *d_norm, size_t count,
                              const double *d_n, const double *d_gamma, double *d_out)
{
    rim_with_tab_kind(tab_kind, [&](auto K) {
        constexpr int KIND = rim_tab_seam_kind(decltype(K)::value);
        if constexpr (KIND == DIST_TABULATED_2D_GRID) rim_tab_2d_grid_launch_integrand(grid, st, pa, d_norm, count, d_n, d_gamma, d_out);
        else if constexpr (KIND == DIST_TABULATED_2D_PITCHY) rim_tab_2d_pitchy_launch_integrand(grid, st, pa, d_norm, count, d_n, d_gamma, d_out);
        else if constexpr (KIND == DIST_TABULATED_2D_GRID_PITCHY) rim_tab_2d_grid_pitchy_launch_integrand(grid, st, pa, d_norm, count, d_n, d_gamma, d_out);
        else if constexpr (KIND == DIST_TABULATED_2D_NODES) rim_tab_2d_nodes_launch_integrand(grid, st, pa, d_norm, count, d_n, d_gamma, d_out);
        else if constexpr (KIND == DIST_TABULATED_2D_NODES_PITCHY) rim_tab_2d_nodes_pitchy_launch_integrand(grid, st, pa, d_norm, count, d_n, d_gamma, d_out);
        else if constexpr (KIND == DIST_TABULATED_FAMILY) rim_tab_family_launch_integrand(grid, st, pa, d_norm, count, d_n, d_gamma, d_out);
        else if constexpr (KIND == DIST_TABULATED_FAMILY_PITCHY) rim_tab_family_pitchy_launch_integrand(grid, st, pa, d_norm, count, d_n, d_gamma, d_out);
        else if constexpr (KIND == DIST_TABULATED_2D_FAMILY) rim_tab_2d_family_launch_integrand(grid, st, pa, d_norm, count, d_n, d_gamma, d_out);
        else if constexpr (KIND == DIST_TABULATED_2D_FAMILY_PITCHY) rim_tab_2d_family_pitchy_launch_integrand(grid, st, pa, d_norm, count, d_n, d_gamma, d_out);
        else if constexpr (KIND == DIST_TABULATED_2D_FAMILY_CUBIC) rim_tab_2d_family_cubic_launch_integrand(grid, st, pa, d_norm, count, d_n, d_gamma, d_out);
        else if constexpr (KIND == DIST_TABULATED_2D_FAMILY_CUBIC_PITCHY) rim_tab_2d_family_cubic_pitchy_launch_integrand(grid, st, pa, d_norm, count, d_n, d_gamma, d_out);
        else hipLaunchKernelGGL(integrand_kernel_n<KIND>, dim3(grid), dim3(64), RIM_DYN_LDS, st, pa, d_norm, count, d_n, d_gamma, d_out);
    });
}

void rim_tab_launch_gamma_integral(int tab_kind, unsigned grid, hipStream_t st, const PointArgs &pa, const double *d_norm, size_t count,
                                   const double *d_n, double *d_out, double *spill)
{
    rim_with_tab_kind(tab_kind, [&](auto K) {
        constexpr int KIND = rim_tab_seam_kind(decltype(K)::value);
        if constexpr (KIND == DIST_TABULATED_2D_GRID) rim_tab_2d_grid_launch_gamma_integral(grid, st, pa, d_norm, count, d_n, d_out, spill);
        else if constexpr (KIND == DIST_TABULATED_2D_PITCHY) rim_tab_2d_pitchy_launch_gamma_integral(grid, st, pa, d_norm, count, d_n, d_out, spill);
        else if constexpr (KIND == DIST_TABULATED_2D_GRID_PITCHY) rim_tab_2d_grid_pitchy_launch_gamma_integral(grid, st, pa, d_norm, count, d_n, d_out, spill);
        else if constexpr (KIND == DIST_TABULATED_2D_NODES) rim_tab_2d_nodes_launch_gamma_integral(grid, st, pa, d_norm, count, d_n, d_out, spill);
        else if constexpr (KIND == DIST_TABULATED_2D_NODES_PITCHY) rim_tab_2d_nodes_pitchy_launch_gamma_integral(grid, st, pa, d_norm, count, d_n, d_out, spill);
        else if constexpr (KIND == DIST_TABULATED_FAMILY) rim_tab_family_launch_gamma_integral(grid, st, pa, d_norm, count, d_n, d_out, spill);
        else if constexpr (KIND == DIST_TABULATED_FAMILY_PITCHY) rim_tab_family_pitchy_launch_gamma_integral(grid, st, pa, d_norm, count, d_n, d_out, spill);
        else if constexpr (KIND == DIST_TABULATED_2D_FAMILY) rim_tab_2d_family_launch_gamma_integral(grid, st, pa, d_norm, count, d_n, d_out, spill);
        else if constexpr (KIND == DIST_TABULATED_2D_FAMILY_PITCHY) rim_tab_2d_family_pitchy_launch_gamma_integral(grid, st, pa, d_norm, count, d_n, d_out, spill);
        else if constexpr (KIND == DIST_TABULATED_2D_FAMILY_CUBIC) rim_tab_2d_family_cubic_launch_gamma_integral(grid, st, pa, d_norm, count, d_n, d_out, spill);
        else if constexpr (KIND == DIST_TABULATED_2D_FAMILY_CUBIC_PITCHY) rim_tab_2d_family_cubic_pitchy_launch_gamma_integral(grid, st, pa, d_norm, count, d_n, d_out, spill);
        else hipLaunchKernelGGL(gamma_integral_kernel<KIND>, dim3(grid), dim3(64), RIM_DYN_LDS, st, pa, d_norm, count, d_n, d_out, spill);
    });
}
