// CPU oracle of the tabulated distribution (RIMPHONY_TABULATED) on a 2-D table set on gamma nodes and mu nodes of the caller's
// choosing, with or without a sin^k xi prefactor per table, for the tests only: the counterpart of tab2d_grid_oracle.cpp and
// tab2d_pitchy_oracle.cpp for rimphony_ctx_set_tables_2d_nodes.
//
// The oracle's calculators (oracle/rimo_symphony.c, rimo_heyvaerts.c) reach a distribution through three symbols only:
// rimo_dist_init, rimo_calc_f and rimo_calc_f_derivatives (oracle/rimo_dist.c).  This file defines the three for kind 4 on
// top of the HOST build of the very device functions the kernels inline (dev_symphony.h: tab_calc_f_both and
// tab_2d_norm_integrand of DIST_TABULATED_2D_NODES and DIST_TABULATED_2D_NODES_PITCHY) and of the library's own check and build
// (tab_spline.h: rim_tab_check_2d_nodes, rim_tab_build_2d_nodes); linked with the unchanged calculators it gives
// liboracle_tab2dnodes.so, which is comparable with the GPU bit for bit.  The normalisation of a table is integrated when the
// set is installed, as the library does it: rimo_qag over gamma (eps_rel 1e-8, 1000 subintervals) on the integrand the
// device uses.  The table set is process-global, as a context holds one set at a time, and so is its form.
// This build counts the mu node words a search reads (RIM_TAB_2D_NODES_COUNT): tabo_mu_interval reports them per abscissa.
// Compiled with -DRIM_TAB_2D_PITCHY_PLAIN_ENDS, the end cells of nbar get the plain rule: what a test of the tests needs.
// Not part of the product library.
#include <cstring>
#include <type_traits>
#include <vector>

static thread_local unsigned long long g_mu_node_reads = 0;
#define RIM_TAB_2D_NODES_COUNT g_mu_node_reads

#include "../../rimphony_amd/csrc/dev_symphony.h"
#include "../../rimphony_amd/csrc/tab_spline.h"
#include "../../oracle/rimo.h"

using namespace rim;

static std::vector<double> g_blob;      // the table set as the kernels read it
static int g_form = DIST_TABULATED_2D_NODES;    // its form
static const double XGK[32] = RIM_GK31_X, WGK[32] = RIM_GK31_WK;

template <int KIND>
static DistParams params_in(const std::vector<double> &blob, double index, double norm)
{
    DistParams p;
    p.par[0] = index;
    p.par[1] = rim_frombits((uint64_t) (uintptr_t) blob.data());
    p.par[2] = 0.; p.par[3] = 0.; p.par[4] = 0.;
    dist_prepare<KIND>(p, norm);
    return p;
}

// f(std::integral_constant<int, KIND>) for the form `form`
template <class F>
static auto with_form(int form, F &&f)
{
    if (form == DIST_TABULATED_2D_NODES_PITCHY) return f(std::integral_constant<int, DIST_TABULATED_2D_NODES_PITCHY>{});
    return f(std::integral_constant<int, DIST_TABULATED_2D_NODES>{});
}

template <int KIND>
static double norm_fn(double g, void *ctx) { return tab_2d_norm_integrand<KIND>(*(const DistParams *) ctx, g, XGK, WGK); }

static double table_norm(double index) { return g_blob[TAB_HDR_DOUBLES + (size_t) index * TAB_2D_HDR + TAB_2D_NORM]; }

static void integrate_norms(std::vector<double> &blob, int form, size_t n_tables)
{
    rimo_workspace *ws = rimo_workspace_alloc(1000);
    for (size_t t = 0; t < n_tables; t++) {
        with_form(form, [&](auto K) {
            constexpr int KIND = decltype(K)::value;
            DistParams p = params_in<KIND>(blob, (double) t, RIM_NAN);
            double integral = 0., abserr = 0.;
            const int st = rimo_qag(norm_fn<KIND>, &p, p.inv_kappa_width, p.neg_inverse_t, 0., 1e-8, 1000, ws, &integral, &abserr, NULL);
            blob[TAB_HDR_DOUBLES + t * TAB_2D_HDR + TAB_2D_NORM] = st ? RIM_NAN : 1. / (2. * (2. * RIM_PI) * integral);
            return 0;
        });
    }
    rimo_workspace_free(ws);
}

static const int SLOT_COEFF[8] = { RIMO_EMISSION, RIMO_ABSORPTION, RIMO_EMISSION, RIMO_ABSORPTION,
                                   RIMO_EMISSION, RIMO_ABSORPTION, RIMO_FARADAY, RIMO_FARADAY };
static const int SLOT_STOKES[8] = { RIMO_STOKES_I, RIMO_STOKES_I, RIMO_STOKES_Q, RIMO_STOKES_Q,
                                    RIMO_STOKES_V, RIMO_STOKES_V, RIMO_STOKES_Q, RIMO_STOKES_V };

extern "C" {

// the host check alone, as the library applies it: 0 or -1
int tabo_check_2d_nodes(size_t n_tables, size_t n_nodes, const double *gamma, size_t n_mu, const double *mu, const double *log_n,
                        const double *sin_k)
{
    return rim_tab_check_2d_nodes(n_tables, n_nodes, gamma, n_mu, mu, log_n, sin_k);
}

// the counterpart of rimphony_ctx_set_tables_2d_nodes: 0, or -1 for a table set the library refuses (the previous set
// stays).  with_norm = 0 leaves the normalisations at 0.
int tabo_set_tables_2d_nodes(size_t n_tables, size_t n_nodes, const double *gamma, size_t n_mu, const double *mu, const double *log_n,
                             const double *sin_k, int with_norm)
{
    if (n_tables == 0) { g_blob.clear(); return 0; }
    if (rim_tab_check_2d_nodes(n_tables, n_nodes, gamma, n_mu, mu, log_n, sin_k)) return -1;
    std::vector<double> blob;
    rim_tab_build_2d_nodes(n_tables, n_nodes, gamma, n_mu, mu, log_n, sin_k, blob);
    const int form = sin_k ? DIST_TABULATED_2D_NODES_PITCHY : DIST_TABULATED_2D_NODES;
    if (with_norm) integrate_norms(blob, form, n_tables);
    g_blob.swap(blob);
    g_form = form;
    return 0;
}

// The normalisations of the installed set's tables from a record of them (the fixture's, which this oracle computed)
int tabo_put_norms(size_t n_tables, const double *norms)
{
    if (g_blob.empty() || n_tables != (size_t) g_blob[TAB_HDR_NTABLES]) return -1;
    for (size_t t = 0; t < n_tables; t++) g_blob[TAB_HDR_DOUBLES + t * TAB_2D_HDR + TAB_2D_NORM] = norms[t];
    return 0;
}

// the laid-out set: out may be null to ask for the length
size_t tabo_get_blob(double *out, size_t cap)
{
    if (out) memcpy(out, g_blob.data(), (cap < g_blob.size() ? cap : g_blob.size()) * sizeof(double));
    return g_blob.size();
}

// the form of the installed set as its DIST_TABULATED* value
int tabo_form(void) { return g_form; }

// new() + full_calculation() of kind 4, params = {table index}: the table's normalisation, as the rows of a batch read it
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
    d->norm = table_norm(params[0]);
    return rim_isnan(d->norm) ? RIMO_EFAILED : 0;
}

double rimo_calc_f(const rimo_dist *d, double gamma, double cos_xi)
{
    return with_form(g_form, [&](auto K) {
        constexpr int KIND = decltype(K)::value;
        const DistParams p = params_in<KIND>(g_blob, d->par[0], d->norm);
        return calc_f<KIND>(p, gamma, cos_xi);
    });
}

void rimo_calc_f_derivatives(const rimo_dist *d, double gamma, double cos_xi, double *dfdg, double *dfdcx)
{
    with_form(g_form, [&](auto K) {
        constexpr int KIND = decltype(K)::value;
        const DistParams p = params_in<KIND>(g_blob, d->par[0], d->norm);
        calc_f_derivatives<KIND>(p, gamma, cos_xi, *dfdg, *dfdcx);
        return 0;
    });
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
    return with_form(g_form, [&](auto K) {
        constexpr int KIND = decltype(K)::value;
        const DistParams p = params_in<KIND>(g_blob, par[0], norm);
        for (size_t i = 0; i < count; i++) {
            f[i] = calc_f<KIND>(p, gamma[i], cos_xi[i]);
            calc_f_derivatives<KIND>(p, gamma[i], cos_xi[i], dfdg[i], dfdcx[i]);
        }
        return 0;
    });
}

// the form's bicubic itself over arrays: S, dS/du, dS/dmu of table `index`
int tabo_bicubic(double index, size_t count, const double *gamma, const double *mu, double *s, double *dsdu, double *dsdmu)
{
    if (g_blob.empty() || !tab_row_ok(g_blob.data(), index)) return -1;
    const DistParams p = params_in<DIST_TABULATED_2D_NODES>(g_blob, index, 1.);
    for (size_t i = 0; i < count; i++) tab_bicubic_nodes(p, gamma[i], mu[i], s[i], dsdu[i], dsdmu[i]);
    return 0;
}

// the mu interval of the installed set over arrays, as the device finds it, and the mu node words each search read
int tabo_mu_interval(size_t count, const double *mu, long long *interval, unsigned long long *reads)
{
    if (g_blob.empty()) return -1;
    const double *th = g_blob.data() + TAB_HDR_DOUBLES;
    const double *mn = th + (long long) th[TAB_2D_MU_NODES];
    for (size_t i = 0; i < count; i++) {
        const unsigned long long before = g_mu_node_reads;
        interval[i] = tab_2d_nodes_mu_interval(th, mn, mu[i]);
        reads[i] = g_mu_node_reads - before;
    }
    return 0;
}

// nbar(gamma) = 1/2 int (1 - mu^2)^(k/2) exp(S) dmu of table `index` as the normalisation integrates it
int tabo_nbar(double index, size_t count, const double *gamma, double *nbar)
{
    if (g_blob.empty() || !tab_row_ok(g_blob.data(), index)) return -1;
    return with_form(g_form, [&](auto K) {
        constexpr int KIND = decltype(K)::value;
        const DistParams p = params_in<KIND>(g_blob, index, 1.);
        for (size_t i = 0; i < count; i++) nbar[i] = tab_2d_norm_integrand<KIND>(p, gamma[i], XGK, WGK);
        return 0;
    });
}

}
