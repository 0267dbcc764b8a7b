// CPU oracle of an ANALYTIC anisotropic distribution, for the tests only: a power law times sin^k xi times an exponential
// beam,
//
//   f(gamma, mu) = norm gamma^-p exp(-gamma / gamma_cutoff) (1 - mu^2)^(k/2) exp(a mu) / (gamma^2 beta)   on [gamma_min, gamma_max],
//   norm = 1 / (4 pi P int gamma^-p exp(-gamma / gamma_cutoff) dgamma),   P = 1/2 int_{-1}^{+1} (1 - mu^2)^(k/2) exp(a mu) dmu,
//   df/dmu = f (a - k mu / (1 - mu^2)),   df/dgamma = -f ((p + 1) / gamma + gamma / (gamma^2 - 1) + 1 / gamma_cutoff),
//
// params {p, gamma_min, gamma_max, gamma_cutoff, a, k}.  Written from these formulas with the C library's functions and none
// of the table code: what a tabulated distribution with a sin^k prefactor and G = a mu is compared with.  It supplies the
// three symbols the oracle's calculators reach a distribution through (oracle/rimo_dist.c) and, linked with the unchanged
// calculators, gives liboracle_pitchy_beam.so.  The gamma normalisation follows power_law.rs:93-103, the pitch factor
// pitchy_pl.rs:98-111 with a quadrature at eps_rel 1e-10 in the place of the closed form.
// Not part of the product library.
#include <cmath>
#include <cstring>
#include "../../oracle/rimo.h"

static double gamma_norm_fn(double g, void *ctx)
{
    const rimo_dist *d = (const rimo_dist *) ctx;
    return std::pow(g, -d->par[0]) * std::exp(-g * d->inv_gamma_cutoff);
}

static double pitch_fn(double mu, void *ctx)
{
    const rimo_dist *d = (const rimo_dist *) ctx;
    return std::pow(1. - mu * mu, 0.5 * d->par[5]) * std::exp(d->par[4] * mu);
}

static const int SLOT_COEFF[8] = { RIMO_EMISSION, RIMO_ABSORPTION, RIMO_EMISSION, RIMO_ABSORPTION,
                                   RIMO_EMISSION, RIMO_ABSORPTION, RIMO_FARADAY, RIMO_FARADAY };
static const int SLOT_STOKES[8] = { RIMO_STOKES_I, RIMO_STOKES_I, RIMO_STOKES_Q, RIMO_STOKES_Q,
                                    RIMO_STOKES_V, RIMO_STOKES_V, RIMO_STOKES_Q, RIMO_STOKES_V };

extern "C" {

// P = 1/2 int (1 - mu^2)^(k/2) exp(a mu) dmu by a quadrature at epsrel 1e-10; NaN if that fails
double pbeamo_pitch_integral(double a, double k)
{
    rimo_dist d;
    memset(&d, 0, sizeof d);
    d.par[4] = a; d.par[5] = k;
    double integral = 0., abserr = 0.;
    rimo_workspace *ws = rimo_workspace_alloc(1000);
    const int st = rimo_qag(pitch_fn, &d, -1., 1., 0., 1e-10, 1000, ws, &integral, &abserr, NULL);
    rimo_workspace_free(ws);
    return st ? NAN : 0.5 * integral;
}

int rimo_dist_init(rimo_dist *d, int kind, const double *params)
{
    d->kind = kind;
    for (int i = 0; i < RIMO_MAX_PARAMS; i++) d->par[i] = params[i];
    d->inv_gamma_cutoff = 1. / params[3];
    d->inv_kappa_width = 0.;
    d->neg_inverse_t = 0.;
    d->norm = NAN;
    const double pa_integral = pbeamo_pitch_integral(params[4], params[5]);
    if (!std::isfinite(pa_integral)) return RIMO_EFAILED;
    double integral = 0., abserr = 0.;
    rimo_workspace *ws = rimo_workspace_alloc(1000);
    const int st = rimo_qag(gamma_norm_fn, d, d->par[1], d->par[2], 0., 1e-8, 1000, ws, &integral, &abserr, NULL);
    rimo_workspace_free(ws);
    if (!st) d->norm = 1. / (2. * (2. * M_PI) * pa_integral * integral);
    return st;
}

double rimo_calc_f(const rimo_dist *d, double gamma, double cos_xi)
{
    if (gamma < d->par[1] || gamma > d->par[2]) return 0.;
    const double beta = std::sqrt(1. - 1. / (gamma * gamma));
    const double gamma_term = std::pow(gamma, -d->par[0]) * std::exp(-gamma * d->inv_gamma_cutoff);
    return d->norm * gamma_term * pitch_fn(cos_xi, (void *) d) / (gamma * gamma * beta);
}

void rimo_calc_f_derivatives(const rimo_dist *d, double gamma, double cos_xi, double *dfdg, double *dfdcx)
{
    if (gamma < d->par[1] || gamma > d->par[2]) { *dfdg = 0.; *dfdcx = 0.; return; }
    const double f = rimo_calc_f(d, gamma, cos_xi);
    *dfdg = -f * ((d->par[0] + 1.) / gamma + gamma / (gamma * gamma - 1.) + d->inv_gamma_cutoff);
    *dfdcx = f * (d->par[4] - d->par[5] * cos_xi / (1. - cos_xi * cos_xi));
}

// N x (full_calculation + the selected coefficients): par [n][6] row-major, out [n][8]
int pbeamo_batch(size_t n, const double *s, const double *theta, const double *par, uint32_t coeff_mask, double *out, int nthreads)
{
    if (nthreads < 1) nthreads = 1;
#pragma omp parallel for schedule(dynamic, 1) num_threads(nthreads)
    for (long long i = 0; i < (long long) n; i++) {
        rimo_dist d;
        const int st = rimo_dist_init(&d, 0, par + i * 6);
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

double pbeamo_norm(const double *par)
{
    rimo_dist d;
    return rimo_dist_init(&d, 0, par) ? NAN : d.norm;
}

}
