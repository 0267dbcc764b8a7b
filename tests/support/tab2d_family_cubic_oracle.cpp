// CPU oracle of the tabulated distribution (RIMPHONY_TABULATED) on a family of 2-D surfaces blended CUBICALLY across its tables,
// for the tests only: the counterpart of tab2d_family_oracle.cpp for rimphony_ctx_set_tables_2d_family_cubic.
//
// The oracle's calculators (oracle/rimo_symphony.c, rimo_heyvaerts.c) reach a distribution through three symbols only:
// rimo_dist_init, rimo_calc_f and rimo_calc_f_derivatives (oracle/rimo_dist.c).  This file defines the three for kind 4 on
// top of the HOST build of the very device functions the kernels inline (dev_symphony.h: tab_family_row,
// tab_2d_family_cubic_line, tab_bicubic_family_cubic, tab_2d_norm_integrand and tab_calc_f_both of
// DIST_TABULATED_2D_FAMILY_CUBIC / _PITCHY) and of the library's own check and build (tab_spline.h:
// rim_tab_check_2d_family_cubic, rim_tab_build_2d_family_cubic); linked with the unchanged calculators it gives
// liboracle_tab2dfamilycubic.so, which is comparable with the GPU bit for bit.  The line of a row is formed per call as the
// library's prologue kernel forms it; the normalisation is integrated per row, rimo_qag over gamma (eps_rel 1e-8, 1000
// subintervals) on the integrand norm_kernel uses; a row whose blended k leaves [0, 100] is refused as norm_kernel refuses
// it.  The table set is process-global, as a context holds one set at a time.  Not part of the product library.
#include <cstring>
#include <vector>
#include "../../rimphony_amd/csrc/dev_symphony.h"
#include "../../rimphony_amd/csrc/tab_spline.h"
#include "../../oracle/rimo.h"

using namespace rim;

static std::vector<double> g_blob;      // the family as the kernels read it
static bool g_pitchy = false;           // the family has a sin^k prefactor
static const double XGK[32] = RIM_GK31_X, WGK[32] = RIM_GK31_WK;

// the row's line, as tab_2d_family_lines_kernel writes it
static void row_line(double x, double *line)
{
    size_t a;
    double w;
    tab_family_row(g_blob.data(), x, a, w);
    tab_2d_family_cubic_line(line, g_blob.data(), a, w);
}

// `line`: TAB_2D_CUBIC_LINE doubles of the caller's, which the returned parameters point into
static DistParams dev_params(double x, double norm, double *line)
{
    DistParams p;
    p.par[0] = x;
    p.par[1] = rim_frombits((uint64_t) (uintptr_t) g_blob.data());
    row_line(x, line);
    p.par[2] = rim_frombits((uint64_t) (uintptr_t) line);
    p.par[3] = 0.; p.par[4] = 0.;
    if (g_pitchy) dist_prepare<DIST_TABULATED_2D_FAMILY_CUBIC_PITCHY>(p, norm);
    else dist_prepare<DIST_TABULATED_2D_FAMILY_CUBIC>(p, norm);
    return p;
}

static double norm_fn(double g, void *ctx)
{
    return g_pitchy ? tab_2d_norm_integrand<DIST_TABULATED_2D_FAMILY_CUBIC_PITCHY>(*(const DistParams *) ctx, g, XGK, WGK)
                    : tab_2d_norm_integrand<DIST_TABULATED_2D_FAMILY_CUBIC>(*(const DistParams *) ctx, g, XGK, WGK);
}

static const int SLOT_COEFF[8] = { RIMO_EMISSION, RIMO_ABSORPTION, RIMO_EMISSION, RIMO_ABSORPTION,
                                   RIMO_EMISSION, RIMO_ABSORPTION, RIMO_FARADAY, RIMO_FARADAY };
static const int SLOT_STOKES[8] = { RIMO_STOKES_I, RIMO_STOKES_I, RIMO_STOKES_Q, RIMO_STOKES_Q,
                                    RIMO_STOKES_V, RIMO_STOKES_V, RIMO_STOKES_Q, RIMO_STOKES_V };

extern "C" {

// the counterpart of rimphony_ctx_set_tables_2d_family_cubic: 0, or -1 for a set the library refuses (the previous set stays)
int tabo_set_tables_2d_family_cubic(size_t n_tables, size_t n_nodes, const double *gamma, size_t n_mu, const double *mu,
                                    const double *log_n, const double *sin_k, int ends_gamma, int ends_mu, const double *param)
{
    if (rim_tab_check_ends(ends_gamma, ends_mu)) return -1;
    if (n_tables == 0) { g_blob.clear(); return 0; }
    if (rim_tab_check_2d_family_cubic(n_tables, n_nodes, gamma, n_mu, mu, log_n, sin_k, param)) return -1;
    std::vector<double> blob;
    rim_tab_build_2d_family_cubic(n_tables, n_nodes, gamma, n_mu, mu, log_n, sin_k, param, blob, ends_gamma, ends_mu);
    g_pitchy = sin_k != nullptr;
    g_blob.swap(blob);
    return 0;
}

// (w, k, the table stride in doubles) of the line of a row at index x, the mu geometry words, which are the set's, and
// cubic[6] = the four weights, the stencil's base table and the row's parameter p
int tabo_row_line(double x, double *w, double *k, double *to_b, double *geometry, double *cubic)
{
    if (g_blob.empty()) return -1;
    double line[TAB_2D_CUBIC_LINE];
    row_line(x, line);
    *w = line[TAB_2D_NORM];
    *k = line[TAB_2D_K];
    *to_b = line[TAB_2D_ENDS];
    geometry[0] = line[TAB_2D_LAST]; geometry[1] = line[TAB_2D_INVH]; geometry[2] = line[TAB_2D_H];
    for (int i = 0; i < 4; i++) cubic[i] = line[TAB_2D_CUBIC_L + i];
    cubic[4] = line[TAB_2D_CUBIC_BASE]; cubic[5] = line[TAB_2D_CUBIC_P];
    return 0;
}

// the laid-out set: out may be null to ask for the length
size_t tabo_get_blob(double *out, size_t cap)
{
    if (out) memcpy(out, g_blob.data(), (cap < g_blob.size() ? cap : g_blob.size()) * sizeof(double));
    return g_blob.size();
}

// new() + full_calculation() of kind 4, params = {x}: the normalisation of norm_kernel -- nbar of the blended surface at the
// blended k, the same limits, tolerance and subinterval limit
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
    size_t a;
    double w;
    if (!tab_family_row(g_blob.data(), params[0], a, w)) return 4;
    double line[TAB_2D_CUBIC_LINE];
    DistParams p = dev_params(params[0], RIM_NAN, line);
    if (g_pitchy && !tab_2d_family_cubic_k_ok(line)) return 4;
    double integral = 0., abserr = 0.;
    rimo_workspace *ws = rimo_workspace_alloc(1000);
    const int st = rimo_qag(norm_fn, &p, p.inv_kappa_width, p.neg_inverse_t, 0., 1e-8, 1000, ws, &integral, &abserr, NULL);
    rimo_workspace_free(ws);
    if (!st) d->norm = 1. / (2. * (2. * RIM_PI) * integral);
    if (!st && rim_isnan(d->norm)) return RIMO_EFAILED;
    return st;
}

double rimo_calc_f(const rimo_dist *d, double gamma, double cos_xi)
{
    double line[TAB_2D_CUBIC_LINE];
    const DistParams p = dev_params(d->par[0], d->norm, line);
    return g_pitchy ? calc_f<DIST_TABULATED_2D_FAMILY_CUBIC_PITCHY>(p, gamma, cos_xi) : calc_f<DIST_TABULATED_2D_FAMILY_CUBIC>(p, gamma, cos_xi);
}

void rimo_calc_f_derivatives(const rimo_dist *d, double gamma, double cos_xi, double *dfdg, double *dfdcx)
{
    double line[TAB_2D_CUBIC_LINE];
    const DistParams p = dev_params(d->par[0], d->norm, line);
    if (g_pitchy) calc_f_derivatives<DIST_TABULATED_2D_FAMILY_CUBIC_PITCHY>(p, gamma, cos_xi, *dfdg, *dfdcx);
    else calc_f_derivatives<DIST_TABULATED_2D_FAMILY_CUBIC>(p, gamma, cos_xi, *dfdg, *dfdcx);
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
#pragma omp parallel for schedule(dynamic, 1)
    for (long long i = 0; i < (long long) n; i++) {
        rimo_dist d;
        const int st = rimo_dist_init(&d, DIST_TABULATED, &index[i]);
        norm[i] = st ? RIM_NAN : d.norm;
    }
    return 0;
}

// calc_f / calc_f_derivatives of the DEVICE functions over arrays for the row at x = par[0]: what rimphony_calc_f_batch
// returns, given the normalisation.  (kind: 4, as the other table oracles take it.)
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
