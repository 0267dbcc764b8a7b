// CPU oracle of an ANALYTIC non-separable distribution, for the tests only: a power law whose index depends on the pitch
// angle, times an exponential beam,
//
//   n(gamma, mu) = gamma^(-p + q mu) exp(-gamma / gamma_cutoff) exp(a mu)                       on [gamma_min, gamma_max],
//   f = norm n / (gamma^2 beta),   norm = 1 / (4 pi int nbar dgamma),   nbar(gamma) = 1/2 int_{-1}^{+1} n dmu,
//   df/dgamma = f ((-p + q mu) / gamma - 1 / gamma_cutoff - 1 / gamma - gamma / (gamma^2 - 1)),   df/dmu = f (q ln gamma + a),
//
// params {p, gamma_min, gamma_max, gamma_cutoff, a, q}.  ln n is bilinear in (ln gamma, mu) but for the cutoff: what a 2-D
// table of it is compared with.  Three further terms, off unless tilto_set_extra() turns them on, make it the closed form
// of the tests' other tables too (tab2d_bind.py):
//   ln n += -g1 / gamma + (c1 mu + c2 mu^2) (u - u_min) / (u_max - u_min),   u = ln gamma,
// a roll-off at the low end and an anisotropy that grows with energy, with their terms in both derivatives.
// Written from these formulas with the C library's functions and none of the table code; the normalisation is its own nested
// quadrature (mu inside gamma).  It supplies the three symbols the oracle's calculators reach a distribution through
// (oracle/rimo_dist.c) and, linked with the unchanged calculators, gives liboracle_tilt.so.
// Not part of the product library.
#include <cmath>
#include <cstring>
#include "../../oracle/rimo.h"

static double g_extra[3] = { 0., 0., 0. };      // g1, c1, c2

static double log_n(const rimo_dist *d, double gamma, double mu)
{
    const double u = std::log(gamma), u0 = std::log(d->par[1]), u1 = std::log(d->par[2]);
    return (-d->par[0] + d->par[5] * mu) * u - gamma * d->inv_gamma_cutoff + d->par[4] * mu - g_extra[0] / gamma +
        (g_extra[1] * mu + g_extra[2] * mu * mu) * (u - u0) / (u1 - u0);
}

struct MuCtx { const rimo_dist *d; double gamma; };

static double mu_fn(double mu, void *ctx)
{
    const MuCtx *m = (const MuCtx *) ctx;
    return std::exp(log_n(m->d, m->gamma, mu));
}

static double gamma_fn(double g, void *ctx)
{
    MuCtx m = { (const rimo_dist *) ctx, g };
    double integral = 0., abserr = 0.;
    rimo_workspace *ws = rimo_workspace_alloc(200);
    const int st = rimo_qag(mu_fn, &m, -1., 1., 0., 1e-12, 200, ws, &integral, &abserr, NULL);
    rimo_workspace_free(ws);
    // (a tolerance the rounding of the sum does not reach is no failure of the value)
    return (st && st != RIMO_EROUND) ? NAN : 0.5 * integral;
}

static const int SLOT_COEFF[8] = { RIMO_EMISSION, RIMO_ABSORPTION, RIMO_EMISSION, RIMO_ABSORPTION,
                                   RIMO_EMISSION, RIMO_ABSORPTION, RIMO_FARADAY, RIMO_FARADAY };
static const int SLOT_STOKES[8] = { RIMO_STOKES_I, RIMO_STOKES_I, RIMO_STOKES_Q, RIMO_STOKES_Q,
                                    RIMO_STOKES_V, RIMO_STOKES_V, RIMO_STOKES_Q, RIMO_STOKES_V };

extern "C" {

void tilto_set_extra(double g1, double c1, double c2) { g_extra[0] = g1; g_extra[1] = c1; g_extra[2] = c2; }

int rimo_dist_init(rimo_dist *d, int kind, const double *params)
{
    d->kind = kind;
    for (int i = 0; i < RIMO_MAX_PARAMS; i++) d->par[i] = params[i];
    d->inv_gamma_cutoff = 1. / params[3];
    d->inv_kappa_width = 0.;
    d->neg_inverse_t = 0.;
    d->norm = NAN;
    double integral = 0., abserr = 0.;
    rimo_workspace *ws = rimo_workspace_alloc(1000);
    const int st = rimo_qag(gamma_fn, d, d->par[1], d->par[2], 0., 1e-10, 1000, ws, &integral, &abserr, NULL);
    rimo_workspace_free(ws);
    if (!st && std::isfinite(integral)) d->norm = 1. / (2. * (2. * M_PI) * integral);
    return st ? st : (std::isfinite(integral) ? 0 : RIMO_EFAILED);
}

double rimo_calc_f(const rimo_dist *d, double gamma, double cos_xi)
{
    if (gamma < d->par[1] || gamma > d->par[2]) return 0.;
    const double beta = std::sqrt(1. - 1. / (gamma * gamma));
    return d->norm * std::exp(log_n(d, gamma, cos_xi)) / (gamma * gamma * beta);
}

void rimo_calc_f_derivatives(const rimo_dist *d, double gamma, double cos_xi, double *dfdg, double *dfdcx)
{
    if (gamma < d->par[1] || gamma > d->par[2]) { *dfdg = 0.; *dfdcx = 0.; return; }
    const double f = rimo_calc_f(d, gamma, cos_xi), mu = cos_xi;
    const double u = std::log(gamma), u0 = std::log(d->par[1]), u1 = std::log(d->par[2]);
    const double dlogn_dg = (-d->par[0] + d->par[5] * mu) / gamma - d->inv_gamma_cutoff + g_extra[0] / (gamma * gamma) +
        (g_extra[1] * mu + g_extra[2] * mu * mu) / (gamma * (u1 - u0));
    *dfdg = f * (dlogn_dg - 1. / gamma - gamma / (gamma * gamma - 1.));
    *dfdcx = f * (d->par[5] * u + d->par[4] + (g_extra[1] + 2. * g_extra[2] * mu) * (u - u0) / (u1 - u0));
}

// N x (full_calculation + the selected coefficients) of ONE distribution: par [6], out [n][8]
int tilto_batch(size_t n, const double *s, const double *theta, const double *par, uint32_t coeff_mask, double *out, int nthreads)
{
    if (nthreads < 1) nthreads = 1;
    rimo_dist d0;
    const int st = rimo_dist_init(&d0, 0, par);
#pragma omp parallel for schedule(dynamic, 1) num_threads(nthreads)
    for (long long i = 0; i < (long long) n; i++) {
        rimo_dist d = d0;
        for (int k = 0; k < 8; k++) {
            double v = NAN;
            rimo_counters c;
            memset(&c, 0, sizeof c);
            if ((coeff_mask & (1u << k)) && !st) v = rimo_compute_dimensionless(&d, SLOT_COEFF[k], SLOT_STOKES[k], s[i], theta[i], &c);
            out[i * 8 + k] = v;
        }
    }
    return 0;
}

double tilto_norm(const double *par)
{
    rimo_dist d;
    return rimo_dist_init(&d, 0, par) ? NAN : d.norm;
}

void tilto_calc_f(const double *par, double norm, size_t count, const double *gamma, const double *cos_xi, double *f, double *dfdg,
                  double *dfdcx)
{
    rimo_dist d;
    memset(&d, 0, sizeof d);
    for (int i = 0; i < 6; i++) d.par[i] = par[i];
    d.inv_gamma_cutoff = 1. / par[3];
    d.norm = norm;
    for (size_t i = 0; i < count; i++) {
        f[i] = rimo_calc_f(&d, gamma[i], cos_xi[i]);
        rimo_calc_f_derivatives(&d, gamma[i], cos_xi[i], &dfdg[i], &dfdcx[i]);
    }
}

}
