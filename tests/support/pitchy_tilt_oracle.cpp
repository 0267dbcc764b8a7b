// CPU oracle of an ANALYTIC non-separable distribution with a sin^k xi prefactor, for the tests only: the tilted power law of
// tilt_oracle.cpp times sin^k xi,
//
//   n(gamma, mu) = (1 - mu^2)^(k/2) gamma^(-p + q mu) exp(-gamma / gamma_cutoff) exp(a mu)      on [gamma_min, gamma_max],
//   f = norm n / (gamma^2 beta),   norm = 1 / (4 pi int nbar dgamma),   nbar(gamma) = 1/2 int_{-1}^{+1} n dmu,
//   df/dgamma = f ((-p + q mu) / gamma - 1 / gamma_cutoff - 1 / gamma - gamma / (gamma^2 - 1)),
//   df/dmu = f (q ln gamma + a - k mu / (1 - mu^2)),
//
// params {p, gamma_min, gamma_max, gamma_cutoff, a, q}; k is set with ptilto_set_k().  The smooth remainder n / sin^k xi has a
// logarithm bilinear in (ln gamma, mu) but for the cutoff: what a 2-D table with a sin^k prefactor is compared with.
// Written from these formulas with the C library's functions and none of the table code; the normalisation is its own nested
// quadrature (mu inside gamma), the mu integral adaptive over the singular ends.  It supplies the three symbols the oracle's
// calculators reach a distribution through (oracle/rimo_dist.c) and, linked with the unchanged calculators, gives
// liboracle_pitchy_tilt.so.
// Not part of the product library.
#include <cmath>
#include <cstring>
#include "../../oracle/rimo.h"

static double g_k = 0.;

static double log_rest(const rimo_dist *d, double gamma, double mu)
{
    return (-d->par[0] + d->par[5] * mu) * std::log(gamma) - gamma * d->inv_gamma_cutoff + d->par[4] * mu;
}

struct MuCtx { const rimo_dist *d; double gamma; };

static double mu_fn(double mu, void *ctx)
{
    const MuCtx *m = (const MuCtx *) ctx;
    return std::pow(1. - mu * mu, 0.5 * g_k) * std::exp(log_rest(m->d, m->gamma, mu));
}

static double gamma_fn(double g, void *ctx)
{
    MuCtx m = { (const rimo_dist *) ctx, g };
    double integral = 0., abserr = 0.;
    rimo_workspace *ws = rimo_workspace_alloc(1000);
    const int st = rimo_qag(mu_fn, &m, -1., 1., 0., 1e-12, 1000, ws, &integral, &abserr, NULL);
    rimo_workspace_free(ws);
    // (a tolerance the rounding of the sum does not reach is no failure of the value)
    return (st && st != RIMO_EROUND) ? NAN : 0.5 * integral;
}

static const int SLOT_COEFF[8] = { RIMO_EMISSION, RIMO_ABSORPTION, RIMO_EMISSION, RIMO_ABSORPTION,
                                   RIMO_EMISSION, RIMO_ABSORPTION, RIMO_FARADAY, RIMO_FARADAY };
static const int SLOT_STOKES[8] = { RIMO_STOKES_I, RIMO_STOKES_I, RIMO_STOKES_Q, RIMO_STOKES_Q,
                                    RIMO_STOKES_V, RIMO_STOKES_V, RIMO_STOKES_Q, RIMO_STOKES_V };

extern "C" {

void ptilto_set_k(double k) { g_k = k; }

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
    return d->norm * std::pow(std::sqrt(1. - cos_xi * cos_xi), g_k) * std::exp(log_rest(d, gamma, cos_xi)) / (gamma * gamma * beta);
}

void rimo_calc_f_derivatives(const rimo_dist *d, double gamma, double cos_xi, double *dfdg, double *dfdcx)
{
    if (gamma < d->par[1] || gamma > d->par[2]) { *dfdg = 0.; *dfdcx = 0.; return; }
    const double f = rimo_calc_f(d, gamma, cos_xi), mu = cos_xi;
    const double dlogn_dg = (-d->par[0] + d->par[5] * mu) / gamma - d->inv_gamma_cutoff;
    *dfdg = f * (dlogn_dg - 1. / gamma - gamma / (gamma * gamma - 1.));
    *dfdcx = f * (d->par[5] * std::log(gamma) + d->par[4] - g_k * mu / (1. - mu * mu));
}

// N x (full_calculation + the selected coefficients) of ONE distribution: par [6], out [n][8]
int ptilto_batch(size_t n, const double *s, const double *theta, const double *par, uint32_t coeff_mask, double *out, int nthreads)
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

double ptilto_norm(const double *par)
{
    rimo_dist d;
    return rimo_dist_init(&d, 0, par) ? NAN : d.norm;
}

}
