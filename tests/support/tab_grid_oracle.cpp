// CPU oracle of the tabulated distribution (RIMPHONY_TABULATED) on a table set on given gamma nodes, for the tests only:
// the counterpart of tab_pitchy_oracle.cpp for rimphony_ctx_set_tables_grid.
//
// The oracle's calculators (oracle/rimo_symphony.c, rimo_heyvaerts.c) reach a distribution through three symbols only:
// rimo_dist_init, rimo_calc_f and rimo_calc_f_derivatives (oracle/rimo_dist.c).  This file defines the three for kind 4 on
// top of the HOST build of the very device functions the kernels inline (dev_symphony.h:
// tab_calc_f_both<DIST_TABULATED_GRID>, with tab_spline_grid and its interval search) and of the library's own check and
// build (tab_spline.h: rim_tab_check_grid, rim_tab_build_grid); linked with the unchanged calculators it gives
// liboracle_tabgrid.so, which is comparable with the GPU bit for bit.  P of a table with a pitch row is integrated when the
// set is installed, as the library does it: rimo_qag over mu in [-1, 1] (eps_rel 1e-8, 1000 subintervals) on
// tab_pitchy_p_integrand.  The table set is process-global, as a context holds one set at a time.
// Not part of the product library.
#include <cstring>
#include <vector>
#include "../../rimphony_amd/csrc/dev_symphony.h"
#include "../../rimphony_amd/csrc/tab_spline.h"
#include "../../oracle/rimo.h"

using namespace rim;

static std::vector<double> g_blob;      // the table set as the kernels read it
static int g_p_intervals = 0;           // the most subintervals a P quadrature of the last set used
static long long g_reads = 0;           // node words the last tabo_grid_interval read in its bisection

static DistParams params_in(const std::vector<double> &blob, double index, double norm)
{
    DistParams p;
    p.par[0] = index;
    p.par[1] = rim_frombits((uint64_t) (uintptr_t) blob.data());
    p.par[2] = 0.; p.par[3] = 0.; p.par[4] = 0.;
    dist_prepare<DIST_TABULATED_GRID>(p, norm);
    return p;
}

static DistParams dev_params(double index, double norm) { return params_in(g_blob, index, norm); }

static double norm_fn(double g, void *ctx) { return tab_norm_integrand<DIST_TABULATED_GRID>(*(const DistParams *) ctx, g); }
static double p_fn(double mu, void *ctx) { return tab_pitchy_p_integrand(*(const DistParams *) ctx, mu); }

static const int SLOT_COEFF[8] = { RIMO_EMISSION, RIMO_ABSORPTION, RIMO_EMISSION, RIMO_ABSORPTION,
                                   RIMO_EMISSION, RIMO_ABSORPTION, RIMO_FARADAY, RIMO_FARADAY };
static const int SLOT_STOKES[8] = { RIMO_STOKES_I, RIMO_STOKES_I, RIMO_STOKES_Q, RIMO_STOKES_Q,
                                    RIMO_STOKES_V, RIMO_STOKES_V, RIMO_STOKES_Q, RIMO_STOKES_V };

extern "C" {

// the counterpart of rimphony_ctx_set_tables_grid: 0, or -1 for a table set the library refuses (the previous set stays)
int tabo_set_tables_grid(size_t n_tables, size_t n_nodes, const double *gamma, const double *log_n, size_t n_mu,
                         const double *log_g, const double *sin_k)
{
    if (n_tables == 0) { g_blob.clear(); return 0; }
    if (rim_tab_check_grid(n_tables, n_nodes, gamma, log_n, n_mu, log_g, sin_k)) return -1;
    std::vector<double> blob;
    rim_tab_build_grid(n_tables, n_nodes, gamma, log_n, n_mu, log_g, sin_k, blob);
    g_p_intervals = 0;
    if (log_g) {
        rimo_workspace *ws = rimo_workspace_alloc(1000);
        for (size_t t = 0; t < n_tables; t++) {
            DistParams p = params_in(blob, (double) t, RIM_NAN);
            double integral = 0., abserr = 0.;
            const int st = rimo_qag(p_fn, &p, -1., 1., 0., 1e-8, 1000, ws, &integral, &abserr, NULL);
            ((double *) (uintptr_t) rim_bits(p.par[0]))[TAB_PITCH_P] = st ? RIM_NAN : 0.5 * integral;
            if ((int) ws->size > g_p_intervals) g_p_intervals = (int) ws->size;
        }
        rimo_workspace_free(ws);
    }
    g_blob.swap(blob);
    return 0;
}

// rim_tab_check_grid alone: 0 or -1
int tabo_check_grid(size_t n_tables, size_t n_nodes, const double *gamma, const double *log_n, size_t n_mu, const double *log_g,
                    const double *sin_k)
{
    return rim_tab_check_grid(n_tables, n_nodes, gamma, log_n, n_mu, log_g, sin_k);
}

// The seam of the lookup: the interval the device function finds for gamma in table 0 of the set (-1: no set).  It also
// counts what a sample of that gamma reads on the way (tabo_grid_reads): the guide's two words say how long the bisection is.
long long tabo_grid_interval(double gamma)
{
    if (g_blob.empty()) return -1;
    const DistParams p = dev_params(0., 1.);
    const double u = rim_log(gamma);
    const unsigned *guide = (const unsigned *) (uintptr_t) rim_bits(p.inv_gamma_cutoff);
    const long long c = tab_grid_cell(u, p.par[2], p.par[3], p.par[4]);
    long long span = (long long) guide[c + 1] - (long long) guide[c], steps = 0;
    while (span > 0) { steps++; span >>= 1; }
    g_reads = steps;
    return tab_grid_interval(p, u);
}

long long tabo_grid_reads(void) { return g_reads; }

// u = rim_log(gamma) as the lookup forms it
double tabo_log(double gamma) { return rim_log(gamma); }

// H(ln gamma) and dH/du of table `index` through tab_spline_grid, over an array
int tabo_grid_spline(double index, size_t count, const double *gamma, double *hval, double *dhdu)
{
    if (g_blob.empty() || !tab_row_ok(g_blob.data(), index)) return -1;
    const DistParams p = dev_params(index, 1.);
    for (size_t i = 0; i < count; i++) tab_spline_grid(p, gamma[i], hval[i], dhdu[i]);
    return 0;
}

// The slopes of the natural spline through (u[j], y[j]) by the library's sweep (mutated = 0) or by a copy of it with
// h_{j-1} and h_j swapped in the right-hand side (mutated = 1): a test of the tests, which must tell the two apart on nodes
// that are not uniform and cannot on nodes that are.
void tabo_grid_slopes(size_t n, const double *u, const double *y, int mutated, double *m)
{
    std::vector<double> h(n), ih(n), cp(n), dp(n);
    for (size_t j = 0; j + 1 < n; j++) { h[j] = u[j + 1] - u[j]; ih[j] = 1. / h[j]; }
    if (!mutated) { rim_tab_spline_row_grid(y, n, h.data(), ih.data(), m, cp.data(), dp.data()); return; }
    const size_t last = n - 1;
    cp[0] = 0.5;
    dp[0] = 3. * ((y[1] - y[0]) / h[0]) / 2.;
    for (size_t j = 1; j < last; j++) {
        const double sl = (y[j] - y[j - 1]) / h[j - 1], sr = (y[j + 1] - y[j]) / h[j];
        const double rhs = 3. * (sl * ih[j] + sr * ih[j - 1]);
        const double den = 2. * (ih[j - 1] + ih[j]) - ih[j - 1] * cp[j - 1];
        cp[j] = ih[j] / den;
        dp[j] = (rhs - ih[j - 1] * dp[j - 1]) / den;
    }
    m[last] = (3. * ((y[last] - y[last - 1]) / h[last - 1]) - dp[last - 1]) / (2. - cp[last - 1]);
    for (size_t j = last; j-- > 0;) m[j] = dp[j] - cp[j] * m[j + 1];
}

// the most subintervals a P quadrature of the last set took (0: none ran)
int tabo_p_intervals(void) { return g_p_intervals; }

// (k, P) of a table of the set: its header as the kernels read it
int tabo_table_k_p(double index, double *k, double *pa)
{
    if (g_blob.empty() || !tab_row_ok(g_blob.data(), index)) return -1;
    const DistParams p = dev_params(index, 1.);
    const double *ph = (const double *) (uintptr_t) rim_bits(p.par[0]);
    *k = ph[TAB_PITCHY_K];
    *pa = ph[TAB_PITCH_P];
    return 0;
}

// the laid-out set: out may be null to ask for the length
size_t tabo_get_blob(double *out, size_t cap)
{
    if (out) memcpy(out, g_blob.data(), (cap < g_blob.size() ? cap : g_blob.size()) * sizeof(double));
    return g_blob.size();
}

// new() + full_calculation() of kind 4, params = {table index}: the normalisation of norm_kernel -- same integrand,
// limits, tolerance and subinterval limit, and P of the table's header
int rimo_dist_init(rimo_dist *d, int kind, const double *params)
{
    d->kind = kind;
    for (int i = 0; i < RIMO_MAX_PARAMS; i++) d->par[i] = 0.;
    d->inv_gamma_cutoff = 0.;
    d->inv_kappa_width = 0.;
    d->neg_inverse_t = 0.;
    d->norm = RIM_NAN;
    if (kind != DIST_TABULATED || g_blob.empty()) return 4;
    d->par[0] = params[0];
    if (!tab_row_ok(g_blob.data(), params[0])) return 4;
    DistParams p = dev_params(params[0], RIM_NAN);
    const bool pitch = tab_has_pitch(p);
    const double pa = pitch ? ((const double *) (uintptr_t) rim_bits(p.par[0]))[TAB_PITCH_P] : 1.;
    double integral = 0., abserr = 0.;
    rimo_workspace *ws = rimo_workspace_alloc(1000);
    const int st = rimo_qag(norm_fn, &p, p.inv_kappa_width, p.neg_inverse_t, 0., 1e-8, 1000, ws, &integral, &abserr, NULL);
    rimo_workspace_free(ws);
    if (!st) d->norm = pitch ? 1. / (2. * (2. * RIM_PI) * pa * integral) : 1. / (2. * (2. * RIM_PI) * integral);
    if (!st && rim_isnan(d->norm)) return RIMO_EFAILED;
    return st;
}

double rimo_calc_f(const rimo_dist *d, double gamma, double cos_xi)
{
    const DistParams p = dev_params(d->par[0], d->norm);
    return calc_f<DIST_TABULATED_GRID>(p, gamma, cos_xi);
}

void rimo_calc_f_derivatives(const rimo_dist *d, double gamma, double cos_xi, double *dfdg, double *dfdcx)
{
    const DistParams p = dev_params(d->par[0], d->norm);
    calc_f_derivatives<DIST_TABULATED_GRID>(p, gamma, cos_xi, *dfdg, *dfdcx);
}

// rimo_batch for kind 4: out [n][8], work [n][8] = integrand samples per coefficient (may be null)
int tabo_batch(size_t n, const double *s, const double *theta, const double *index, uint32_t coeff_mask, double *out,
               uint64_t *work, int nthreads)
{
    if (g_blob.empty()) return -1;
    if (nthreads < 1) nthreads = 1;
#pragma omp parallel for schedule(dynamic, 1) num_threads(nthreads)
    for (long long i = 0; i < (long long) n; i++) {
        rimo_dist d;
        const int st = rimo_dist_init(&d, DIST_TABULATED, &index[i]);
        for (int k = 0; k < 8; k++) {
            double v = RIM_NAN;
            rimo_counters c;
            memset(&c, 0, sizeof c);
            if ((coeff_mask & (1u << k)) && !st) v = rimo_compute_dimensionless(&d, SLOT_COEFF[k], SLOT_STOKES[k], s[i], theta[i], &c);
            out[i * 8 + k] = v;
            if (work) work[i * 8 + k] = c.integrand_evals;
        }
    }
    return 0;
}

int tabo_batch_norm(size_t n, const double *index, double *norm)
{
    if (g_blob.empty()) return -1;
    for (size_t i = 0; i < n; i++) {
        rimo_dist d;
        const int st = rimo_dist_init(&d, DIST_TABULATED, &index[i]);
        norm[i] = st ? RIM_NAN : d.norm;
    }
    return 0;
}

// calc_f / calc_f_derivatives of the DEVICE functions over arrays for table par[0]: what rimphony_calc_f_batch returns,
// given the normalisation.  (kind: 4, as the other table oracles take it.)
int tabo_dev_calc_f(int kind, const double *par, double norm, size_t count, const double *gamma, const double *cos_xi,
                    double *f, double *dfdg, double *dfdcx)
{
    if (kind != DIST_TABULATED || g_blob.empty()) return -1;
    rimo_dist d;
    d.par[0] = par[0];
    d.norm = norm;
    for (size_t i = 0; i < count; i++) {
        f[i] = rimo_calc_f(&d, gamma[i], cos_xi[i]);
        rimo_calc_f_derivatives(&d, gamma[i], cos_xi[i], &dfdg[i], &dfdcx[i]);
    }
    return 0;
}

}
