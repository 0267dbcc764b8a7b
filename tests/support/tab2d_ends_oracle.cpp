// CPU oracle of the tabulated distribution (RIMPHONY_TABULATED) on a 2-D table set of any of the six forms with a choice of the
// spline's ends per axis, for the tests only: the counterpart of rimphony_ctx_set_tables_2d_ends and of
// rimphony_ctx_set_tables_2d_device_ends.
//
// The oracle's calculators (oracle/rimo_symphony.c, rimo_heyvaerts.c) reach a distribution through three symbols only:
// rimo_dist_init, rimo_calc_f and rimo_calc_f_derivatives (oracle/rimo_dist.c).  This file defines the three for kind 4 on
// top of the HOST build of the very device functions the kernels inline (dev_symphony.h: calc_f, calc_f_derivatives and
// tab_2d_norm_integrand of the six 2-D kinds) and of the library's own checks and builders with their trailing arguments
// (tab_spline.h: rim_tab_check_ends, rim_tab_build_2d*); linked with the unchanged calculators it gives liboracle_tab2dends.so,
// which is comparable with the GPU bit for bit.  The normalisation of a table is integrated when the set is installed, as the
// library does it: rimo_qag over gamma (eps_rel 1e-8, 1000 subintervals) on the integrand the device uses.  The table set is
// process-global, as a context holds one set at a time, and so is its form.
// It also holds the host build of tab_install.h, looped over the lines of the three families in order: what the device entry
// runs per lane.  Not part of the product library.
#include <cstring>
#include <type_traits>
#include <vector>

#include "../../rimphony_amd/csrc/dev_symphony.h"
#include "../../rimphony_amd/csrc/tab_spline.h"
#include "../../rimphony_amd/csrc/tab_install.h"
#include "../../oracle/rimo.h"

using namespace rim;

static std::vector<double> g_blob;      // the table set as the kernels read it
static int g_form = DIST_TABULATED_2D;  // its form
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
    switch (form) {
    case DIST_TABULATED_2D_PITCHY: return f(std::integral_constant<int, DIST_TABULATED_2D_PITCHY>{});
    case DIST_TABULATED_2D_GRID: return f(std::integral_constant<int, DIST_TABULATED_2D_GRID>{});
    case DIST_TABULATED_2D_GRID_PITCHY: return f(std::integral_constant<int, DIST_TABULATED_2D_GRID_PITCHY>{});
    case DIST_TABULATED_2D_NODES: return f(std::integral_constant<int, DIST_TABULATED_2D_NODES>{});
    case DIST_TABULATED_2D_NODES_PITCHY: return f(std::integral_constant<int, DIST_TABULATED_2D_NODES_PITCHY>{});
    default: return f(std::integral_constant<int, DIST_TABULATED_2D>{});
    }
}

// the form the arguments select, as the library's entries select it
static int form_of(const double *gamma, const double *mu, const double *sin_k)
{
    if (mu) return sin_k ? DIST_TABULATED_2D_NODES_PITCHY : DIST_TABULATED_2D_NODES;
    if (gamma) return sin_k ? DIST_TABULATED_2D_GRID_PITCHY : DIST_TABULATED_2D_GRID;
    return sin_k ? DIST_TABULATED_2D_PITCHY : DIST_TABULATED_2D;
}

// what rimphony_ctx_set_tables_2d_ends refuses: 0 or -1
static int check_all(size_t nt, size_t nn, const double *gamma, double glo, double ghi, size_t nmu, const double *mu,
                     const double *log_n, const double *sin_k, int ends_u, int ends_mu)
{
    if (rim_tab_check_ends(ends_u, ends_mu)) return -1;
    if (!gamma && mu) return -1;
    if (mu) return rim_tab_check_2d_nodes(nt, nn, gamma, nmu, mu, log_n, sin_k);
    if (gamma ? rim_tab_check_2d_grid(nt, nn, gamma, nmu, log_n) : rim_tab_check_2d(nt, nn, glo, ghi, nmu, log_n)) return -1;
    return sin_k ? rim_tab_check_sin_k(nt, sin_k) : 0;
}

static void build_all(size_t nt, size_t nn, const double *gamma, double glo, double ghi, size_t nmu, const double *mu,
                      const double *log_n, const double *sin_k, int ends_u, int ends_mu, std::vector<double> &blob)
{
    if (mu) rim_tab_build_2d_nodes(nt, nn, gamma, nmu, mu, log_n, sin_k, blob, ends_u, ends_mu);
    else if (gamma && sin_k) rim_tab_build_2d_grid_pitchy(nt, nn, gamma, nmu, log_n, sin_k, blob, ends_u, ends_mu);
    else if (gamma) rim_tab_build_2d_grid(nt, nn, gamma, nmu, log_n, blob, ends_u, ends_mu);
    else if (sin_k) rim_tab_build_2d_pitchy(nt, nn, glo, ghi, nmu, log_n, sin_k, blob, ends_u, ends_mu);
    else rim_tab_build_2d(nt, nn, glo, ghi, nmu, log_n, blob, ends_u, ends_mu);
}

// the same set through the builders as they were before they knew of a choice: no trailing arguments
static void build_old(size_t nt, size_t nn, const double *gamma, double glo, double ghi, size_t nmu, const double *mu,
                      const double *log_n, const double *sin_k, std::vector<double> &blob)
{
    if (mu) rim_tab_build_2d_nodes(nt, nn, gamma, nmu, mu, log_n, sin_k, blob);
    else if (gamma && sin_k) rim_tab_build_2d_grid_pitchy(nt, nn, gamma, nmu, log_n, sin_k, blob);
    else if (gamma) rim_tab_build_2d_grid(nt, nn, gamma, nmu, log_n, blob);
    else if (sin_k) rim_tab_build_2d_pitchy(nt, nn, glo, ghi, nmu, log_n, sin_k, blob);
    else rim_tab_build_2d(nt, nn, glo, ghi, nmu, log_n, blob);
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

// the host checks alone, as the two entries apply them: 0 or -1
int tabo_check_2d_ends(size_t n_tables, size_t n_nodes, const double *gamma, double gamma_lo, double gamma_hi, size_t n_mu,
                       const double *mu, const double *log_n, const double *sin_k, int ends_gamma, int ends_mu)
{
    return check_all(n_tables, n_nodes, gamma, gamma_lo, gamma_hi, n_mu, mu, log_n, sin_k, ends_gamma, ends_mu);
}

// the counterpart of rimphony_ctx_set_tables_2d_ends: 0, or -1 for a call the library refuses (the previous set stays).
// with_norm = 0 leaves the normalisations at 0.
int tabo_set_tables_2d_ends(size_t n_tables, size_t n_nodes, const double *gamma, double gamma_lo, double gamma_hi, size_t n_mu,
                            const double *mu, const double *log_n, const double *sin_k, int ends_gamma, int ends_mu, int with_norm)
{
    if (rim_tab_check_ends(ends_gamma, ends_mu)) return -1;
    if (n_tables == 0) { g_blob.clear(); return 0; }
    if (check_all(n_tables, n_nodes, gamma, gamma_lo, gamma_hi, n_mu, mu, log_n, sin_k, ends_gamma, ends_mu)) return -1;
    std::vector<double> blob;
    build_all(n_tables, n_nodes, gamma, gamma_lo, gamma_hi, n_mu, mu, log_n, sin_k, ends_gamma, ends_mu, blob);
    const int form = form_of(gamma, mu, sin_k);
    if (with_norm) integrate_norms(blob, form, n_tables);
    g_blob.swap(blob);
    g_form = form;
    return 0;
}

// The set of the same call as the builders lay it out where the trailing arguments are left out (what every entry that knows
// of no choice installs), normalisations 0: its size in doubles; written to `out` where cap holds it; -1 for a refused call.
long long tabo_build_2d_without_ends(size_t n_tables, size_t n_nodes, const double *gamma, double gamma_lo, double gamma_hi, size_t n_mu,
                                     const double *mu, const double *log_n, const double *sin_k, double *out, size_t cap)
{
    if (check_all(n_tables, n_nodes, gamma, gamma_lo, gamma_hi, n_mu, mu, log_n, sin_k, 0, 0)) return -1;
    std::vector<double> blob;
    build_old(n_tables, n_nodes, gamma, gamma_lo, gamma_hi, n_mu, mu, log_n, sin_k, blob);
    if (out && cap >= blob.size()) memcpy(out, blob.data(), blob.size() * sizeof(double));
    return (long long) blob.size();
}

// The set of the same call as the device entry solves it -- the front of the form, the axis blocks of rim_tab_install_axis,
// then every line of the families 0, 1 and 2, in that order, through rim_tab_install_family_line -- normalisations 0: its size
// in doubles; written to `out` (NaN-filled first, so that a word the lines leave out shows) where cap holds it; -1 for a
// refused call.
long long tabo_lines_2d_ends(size_t nt, size_t nn, const double *gamma, double glo, double ghi, size_t nmu, const double *mu,
                             const double *log_n, const double *sin_k, int ends_gamma, int ends_mu, double *out, size_t cap)
{
    if (check_all(nt, nn, gamma, glo, ghi, nmu, mu, log_n, sin_k, ends_gamma, ends_mu)) return -1;
    const int ends = ends_gamma + 2 * ends_mu;
    std::vector<double> front, h, ih, hm, ihm;
    double hu = 0., hmu = 0.;
    if (mu) rim_tab_front_2d_nodes(nt, nn, gamma, nmu, mu, sin_k, front, h, ih, hm, ihm, ends);
    else if (gamma) rim_tab_front_2d_grid(nt, nn, gamma, nmu, front, h, ih, hmu, ends);
    else rim_tab_front_2d(nt, nn, glo, ghi, nmu, front, hu, hmu, ends);
    if (sin_k && !mu) rim_tab_put_2d_sin_k(nt, sin_k, front);
    const size_t total = front.size() + nt * nn * nmu * 4;
    if (!out || cap < total) return (long long) total;
    std::vector<double> axes(rim_tab_axis_doubles(nn) + rim_tab_axis_doubles(nmu), 0.);
    rim_tab_install_axis(nn, hu, gamma ? h.data() : nullptr, gamma ? ih.data() : nullptr, axes.data(), ends_gamma);
    rim_tab_install_axis(nmu, hmu, mu ? hm.data() : nullptr, mu ? ihm.data() : nullptr, axes.data() + rim_tab_axis_doubles(nn), ends_mu);
    memset(out, 0xff, total * sizeof(double));
    memcpy(out, front.data(), front.size() * sizeof(double));
    RimTabInstall s;
    s.log_n = log_n;
    s.nodes = out + front.size();
    s.n_tables = nt; s.n_nodes = nn; s.n_mu = nmu;
    s.au = rim_tab_axis_of(axes.data(), nn, hu, gamma != nullptr, ends_gamma);
    s.amu = rim_tab_axis_of(axes.data() + rim_tab_axis_doubles(nn), nmu, hmu, mu != nullptr, ends_mu);
    for (int family = 0; family < 3; family++) {
        const size_t lines = rim_tab_install_lines(s, family);
        for (size_t line = 0; line < lines; line++) rim_tab_install_family_line(s, family, line);
    }
    return (long long) total;
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

// the installed form's bicubic itself over arrays: S, dS/du, dS/dmu of table `index`
int tabo_bicubic(double index, size_t count, const double *gamma, const double *mu, double *s, double *dsdu, double *dsdmu)
{
    if (g_blob.empty() || !tab_row_ok(g_blob.data(), index)) return -1;
    return with_form(g_form, [&](auto K) {
        constexpr int KIND = decltype(K)::value;
        const DistParams p = params_in<KIND>(g_blob, index, 1.);
        for (size_t i = 0; i < count; i++) {
            if (tab_kind_2d_nodes(KIND)) tab_bicubic_nodes(p, gamma[i], mu[i], s[i], dsdu[i], dsdmu[i]);
            else if (tab_kind_2d_on_grid(KIND)) tab_bicubic_grid(p, gamma[i], mu[i], s[i], dsdu[i], dsdmu[i]);
            else tab_bicubic(p, gamma[i], mu[i], s[i], dsdu[i], dsdmu[i]);
        }
        return 0;
    });
}

}
