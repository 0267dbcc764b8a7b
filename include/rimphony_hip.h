/* rimphony_hip.h -- C ABI of the MI355X-native batched synchrotron-coefficient
 * integrator (librimphony_hip.so).
 *
 * Scope: the per-parameter-point hot path of pkgw/rimphony, i.e. N times
 *     D::new(..).gamma_limits(..).full_calculation(log)        (power_law.rs:71-111,
 *         thermal_juettner.rs:45-72, pitchy_pl.rs:73-115, pitchy_kappa.rs:70-125)
 *     .compute_all_dimensionless(s, theta)                     (src/lib.rs:178-191)
 * evaluated on the GPU for a closed set of distribution functions.  The
 * reference has no batch/FFI interface for this path; its two existing FFI
 * seams are the leung-bessel extern block (leung-bessel/src/lib.rs:36-42) and
 * the GSL callback trampoline (src/gsl.rs:111-117).  A device kernel cannot
 * call back into a host closure, so the second seam is replaced by the
 * `dist_kind` + SoA parameter arrays below; the first is kept as a batched
 * entry point (rimphony_bessel_batch_device).  INTEGRATION.md shows the
 * `-sys` crate a maintainer would add on the Rust side.
 *
 * Conventions
 *   - plain pointers and sizes only; `stream` is a hipStream_t passed as void*
 *     (NULL = the default stream); `d_*` arguments are DEVICE pointers.
 *   - return value: 0 on success, a negative RIMPHONY_E* code on API misuse or
 *     a HIP failure (rimphony_strerror()).  Numerical failure is never an
 *     error: as in the reference (symphony.rs:115-117,127,380) the affected
 *     coefficient is NaN, and the optional status array says why.
 *   - output slot order is that of lib.rs:176-177:
 *         [j_I, alpha_I, j_Q, alpha_Q, j_V, alpha_V, rho_Q, rho_V]
 *     Slots not selected in coeff_mask are written as NaN.
 *   - results depend only on the inputs of a point, never on batch size,
 *     launch geometry or which GPU evaluated it.
 *   - the caller owns every buffer it passes; the library owns its workspace
 *     through the opaque context and never returns memory to the caller.
 */
#ifndef RIMPHONY_HIP_H
#define RIMPHONY_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* enum Stokes (lib.rs:74-87) and enum Coefficient (lib.rs:91-107) */
enum { RIMPHONY_STOKES_I = 0, RIMPHONY_STOKES_Q = 1, RIMPHONY_STOKES_V = 2 };
enum { RIMPHONY_EMISSION = 0, RIMPHONY_ABSORPTION = 1, RIMPHONY_FARADAY = 2 };

/* Distribution kinds; params are SoA arrays, one per parameter, in this order:
 *   POWER_LAW         p, gamma_min, gamma_max, gamma_cutoff          (power_law.rs:27-33, 82-87)
 *   THERMAL_JUETTNER  T                                              (thermal_juettner.rs:45-50)
 *   PITCHY_PL         p, k, gamma_min, gamma_max, gamma_cutoff       (pitchy_pl.rs:73-90)
 *   PITCHY_KAPPA      kappa, width, k, gamma_cutoff                  (pitchy_kappa.rs:70-85)
 *   TABULATED         table index (as a double)                      (the open DistributionFunction trait, lib.rs:111-146,
 *                     as data: rimphony_ctx_set_tables below) */
enum {
    RIMPHONY_POWER_LAW = 0,
    RIMPHONY_THERMAL_JUETTNER = 1,
    RIMPHONY_PITCHY_PL = 2,
    RIMPHONY_PITCHY_KAPPA = 3,
    RIMPHONY_TABULATED = 4
};
int rimphony_dist_nparams(int dist_kind);   /* 4, 1, 5, 4, 1; negative for an unknown kind */

/* coeff_mask bits = output slots */
#define RIMPHONY_SLOT_J_I      (1u << 0)
#define RIMPHONY_SLOT_ALPHA_I  (1u << 1)
#define RIMPHONY_SLOT_J_Q      (1u << 2)
#define RIMPHONY_SLOT_ALPHA_Q  (1u << 3)
#define RIMPHONY_SLOT_J_V      (1u << 4)
#define RIMPHONY_SLOT_ALPHA_V  (1u << 5)
#define RIMPHONY_SLOT_RHO_Q    (1u << 6)
#define RIMPHONY_SLOT_RHO_V    (1u << 7)
#define RIMPHONY_SLOTS_ALL     0xffu

/* per-coefficient status bits (0 = clean) */
#define RIMPHONY_ST_INNER_FAIL  1   /* an inner QAG returned a GSL error -> NaN sample (symphony.rs:380) */
#define RIMPHONY_ST_OUTER_FAIL  2   /* an outer (n / Heyvaerts) QAG failed (symphony.rs:269 `?`)        */
#define RIMPHONY_ST_CHUNK_CAP   4   /* chunk-marching iteration cap hit                                  */
#define RIMPHONY_ST_STORE_FULL  8   /* LDS subinterval store exhausted                                   */
#define RIMPHONY_ST_NONFINITE   16  /* the coefficient is NaN                                            */
#define RIMPHONY_ST_NORM_FAIL   32  /* normalisation integral failed (the reference would panic)         */
#define RIMPHONY_ST_NOT_COMPUTED 64 /* slot not selected / not available                                 */

/* error codes */
#define RIMPHONY_OK         0
#define RIMPHONY_EINVAL    -1
#define RIMPHONY_EHIP      -2
#define RIMPHONY_ENOMEM    -3
#define RIMPHONY_ENODEVICE -4
#define RIMPHONY_EBUSY     -5   /* RIMPHONY_EXCLUSIVE=1 and another context already has the device */
#define RIMPHONY_ENOTSUP   -6   /* e.g. a `precision` this build does not implement; librccl not loadable */
#define RIMPHONY_ERCCL     -7   /* an RCCL call failed (rimphony_last_error() has RCCL's text) */

/* `precision` of the _ex / _multi entry points.  F64 is the reference's arithmetic (bit-identical to the
 * oracle) and the only precision offered.  F32_INTEGRAND (BASELINE configs[4]: the bodies of the elementary functions of
 * the Symphony integrand in single precision on the hardware transcendental unit, every difference, every product with
 * the harmonic number and every quadrature sum in fp64) returns RIMPHONY_ENOTSUP for EVERY distribution, as does any
 * other value: measured, it is slower AND lossier than F64 -- on pitchy_kappa (the distribution configs[4] names) 1.53 x
 * the fp64 time with 1.9 % new NaNs, because its non-smooth 1e-7 noise trips GSL's round-off detectors on integrals that
 * cancel; on the power-law and thermal distributions 0.90 / 0.96 of the fp64 time of the round-2 kernel it is built on,
 * i.e. 1.36 / 1.43 x the time of the fp64 default since that moved to the group kernel (round 3), with ~1e-6 p99
 * differences.  The kernels stay in the library behind a measurement hook -- a context created with
 * RIMPHONY_F32_VARIANT=1 in the environment accepts F32_INTEGRAND for POWER_LAW and THERMAL_JUETTNER
 * (tools/f32_variant.py) -- so that the statement above can be re-measured; configs[4]'s table itself runs in F64. */
#define RIMPHONY_PRECISION_F64            0
#define RIMPHONY_PRECISION_F32_INTEGRAND  1

typedef struct rimphony_ctx rimphony_ctx;

/* Create / destroy a context bound to one HIP device.  Fails with
 * RIMPHONY_ENODEVICE when no GPU is present (there is no CPU fallback).
 * Environment, read once here: RIMPHONY_NO_ASSIST=1 turns the cooperative tail of the kernels off (one
 * wavefront per task to the end; same results bit for bit, used for A/B measurements and by the tests).
 * One context per GPU is the supported configuration: its persistent grids fill the device.  The first context
 * on a device (in any process) takes an exclusive flock on /dev/shm/rimphony_hip.<pci bus id>.lock for its
 * lifetime; a context created while that lock is held runs in SHARED mode (quarter-size grids, cooperative tail
 * off: slower, same results) or, with RIMPHONY_EXCLUSIVE=1 in the environment, is refused with RIMPHONY_EBUSY.
 * Calls on one context are serialised and ordered on the device whatever streams they name; different contexts
 * may be used from different threads freely.
 * RIMPHONY_SYM_SOLO=1 runs the six Symphony coefficients one wave per (point, coefficient) as until round 2 instead of
 * the coefficients of a point in lock-step; RIMPHONY_FARADAY_GROUP=1 runs rho_Q and rho_V of a point in lock-step as well
 * (measured slower than one wave per coefficient, hence off).  Both for A/B measurements: the tables do not change.
 * RIMPHONY_TAB_GROUP=1 / =0 runs the Symphony coefficients of RIMPHONY_TABULATED in lock-step on the group kernel / one wave
 * per coefficient whatever the form of the table set (unset or negative: the form's default, at rimphony_ctx_set_tables);
 * RIMPHONY_SYM_SOLO=1 wins.  The tables do not change either.
 * RIMPHONY_EARLY_SQUAD=<n> sets how many waves of the Faraday kernel's grid serve the longest outer quadratures of a
 * launch from its first cycle instead of fetching tasks (0: none; default 64 for the power-law family, 256 for pitchy kappa,
 * 0 for the other two distributions; only on launches with at least four tasks per wave, never in shared mode),
 * RIMPHONY_EARLY_MIN=<n> the size from which an outer quadrature competes for them (16), RIMPHONY_FARADAY_ORDER=symphony
 * makes the Faraday launch visit the points in the Symphony launch's order; RIMPHONY_ROUNDS=0 makes a long outer
 * quadrature of the pitchy-kappa Faraday kernel evaluate one interval per batch (default: the children of up to four, their
 * rule sums filed ahead of qag.c's picks; the other distributions' kernels are built without rounds).  Scheduling only: the tables do not change.
 * RIMPHONY_OWNER_WAIT_US=<n> (test hook) shortens the 120 s an owner wave waits for its helpers before it recomputes
 * a published batch itself; results do not depend on it. */
int rimphony_ctx_create(int device, rimphony_ctx **out);
void rimphony_ctx_destroy(rimphony_ctx *ctx);
int rimphony_ctx_shared_mode(const rimphony_ctx *ctx);   /* 0: owns the device, 1: shared mode */
int rimphony_ctx_device(const rimphony_ctx *ctx, int *device);   /* the HIP device the context is bound to */
const char *rimphony_strerror(int code);
/* Text of the most recent failure on the calling thread (which HIP call failed and why); "" if none.  The library
 * never prints. */
const char *rimphony_last_error(void);
const char *rimphony_version(void);

/* Tabulated distributions (RIMPHONY_TABULATED): isotropic f(gamma) given as tables of ln n(gamma), n = dN/dgamma up to a
 * constant factor -- the convention of the power law's gamma^-p exp(-gamma / gamma_cutoff); the normalisation
 * 1 / (4 pi int n dgamma) over [gamma_lo, gamma_hi] is computed per row like every other kind's (power_law.rs:93-103).
 *   log_n   HOST, [n_tables][n_nodes]: ln n at nodes uniform in ln gamma from ln gamma_lo to ln gamma_hi;
 *           8 <= n_nodes <= 65536, 1 <= gamma_lo < gamma_hi, every value finite -- else RIMPHONY_EINVAL (checked on the host).
 * Between the nodes the library evaluates the natural cubic spline in (ln gamma, ln n), so f and df/dgamma are smooth for
 * the quadratures and a straight line -- a pure power law -- is reproduced exactly; f = norm n / (gamma^2 beta) inside the
 * table, f = 0 outside (the rule of power_law.rs:38,49).  A table that ENDS at a non-negligible n therefore behaves like the
 * power law's gamma limits: a step in f, on which the reference's quadratures report round-off (NaN) for part of the
 * coefficients.  Taper the table so that n is negligible at both ends.
 * A context holds one table set at a time: the call copies it to the device (the slopes of the splines are solved on the
 * host, once), replaces the previous set and returns after the context's earlier work has finished; n_tables = 0 clears
 * the set.  Whatever its form, the new set is complete on the device before the previous one is let go: a call that is
 * refused or fails leaves the previous set in place, and for the length of the call both sets are resident.  A row of a batch names its table by index (the kind's one parameter, a double); a row whose index is not an
 * integer in [0, n_tables) gets a NaN normalisation: all its selected slots are NaN with RIMPHONY_ST_NORM_FAIL.  With no
 * table set every entry refuses the kind with RIMPHONY_EINVAL.  In the _multi entries each context uses its OWN table
 * set: give every context the same tables.  The six Symphony coefficients of a point run in lock-step on the group kernel,
 * as for the analytic kinds, where that is the form's default -- every form, until profiles/tabulated_group_times.txt holds a measurement -- and one
 * wave per coefficient otherwise; RIMPHONY_TAB_GROUP=1 / =0 in the environment of rimphony_ctx_create chooses for every form.  Same
 * values, status words and work counters either way; rimphony_last_work().passes and the group statistics of
 * rimphony_last_tail say which ran.  If the group kernel's workspace cannot be allocated (4.4 GB for a full grid) the batch
 * runs one wave per coefficient instead of failing.  The Faraday pair always runs one wave per coefficient
 * (RIMPHONY_FARADAY_GROUP does not apply to the kind).  RIMPHONY_PRECISION_F32_INTEGRAND is RIMPHONY_ENOTSUP and the
 * high-frequency closed forms RIMPHONY_EINVAL, as for every kind without them. */
int rimphony_ctx_set_tables(rimphony_ctx *ctx, size_t n_tables, size_t n_nodes, double gamma_lo, double gamma_hi,
                            const double *log_n);

/* Tabulated distributions with a pitch-angle factor per table (the entry above is the isotropic case):
 * f(gamma, mu) = norm n(gamma) g(mu) / (gamma^2 beta), mu = cos xi, separable, norm = 1 / (4 pi P int n dgamma) with
 * P = 1/2 int_{-1}^{+1} g dmu (pitchy_pl.rs:98-111), df/dmu = f G'(mu), G = ln g.
 *   log_g   HOST, [n_tables][n_mu]: ln g at nodes uniform in mu from -1 to +1, end points included; 8 <= n_mu <= 65536,
 *           every value finite -- else RIMPHONY_EINVAL.  Only the shape of a row matters: P absorbs an added constant.
 * log_g == NULL with n_mu == 0 is rimphony_ctx_set_tables exactly (isotropic; the same bits); exactly one of the two given
 * is RIMPHONY_EINVAL.  Between the nodes the library evaluates the natural cubic spline in (mu, ln g): g > 0 everywhere and
 * a straight line G = a mu -- an exponential beam -- is reproduced exactly, the counterpart of the power law in gamma.  P is
 * the integral of that spline, computed on the host once per table.  A mu a rounding beyond +-1 extrapolates the end
 * cubic; a NaN mu gives NaN.
 * A ln g that DIVERGES at mu = +-1 (sin^k xi: ln g = (k/2) ln(1 - mu^2)) is hostile to the spline.  Floored as
 * (k/2) ln(1 - mu^2 + 1e-6) with k = 2, 257 nodes give g to 5e-6 for |mu| < 0.9 but ring by order one at |mu| = 0.99, and
 * 1025 nodes still leave 3e-3 there: give such a factor as an exponent instead (rimphony_ctx_set_tables_pitchy below),
 * or use RIMPHONY_PITCHY_PL / _KAPPA where their energy part serves.
 * The results are the reference's algorithms applied to the f given: its DistributionFunction trait accepts any
 * f(gamma, cos xi), one that is asymmetric in mu included; whether that is physically meaningful is the caller's matter.
 * Everything else -- rows and their index, the refusals, the kernels used (the group kernel or one wave per coefficient for
 * the Symphony coefficients: RIMPHONY_TAB_GROUP) -- is as for rimphony_ctx_set_tables. */
int rimphony_ctx_set_tables_pitch(rimphony_ctx *ctx, size_t n_tables, size_t n_nodes, double gamma_lo, double gamma_hi,
                                  const double *log_n, size_t n_mu, const double *log_g);

/* Tabulated distributions given as a SURFACE, ln n(gamma, mu) on a grid: any f(gamma, cos xi), one that is not a product
 * n(gamma) g(mu) included -- an anisotropy that grows with energy, a beam on an isotropic core, a loss cone above some gamma.
 * f(gamma, mu) = norm exp(S(ln gamma, mu)) / (gamma^2 beta) inside [gamma_lo, gamma_hi], 0 outside;
 * df/dgamma = f (S_u / gamma - 1 / gamma - gamma / (gamma^2 - 1)), df/dmu = f S_mu;
 * norm = 1 / (4 pi int nbar dgamma), nbar(gamma) = 1/2 int_{-1}^{+1} exp(S(ln gamma, mu)) dmu.
 *   log_n   HOST, [n_tables][n_nodes][n_mu], mu fastest: ln n at nodes uniform in ln gamma from ln gamma_lo to ln gamma_hi
 *           and uniform in mu from -1 to +1, end points included; 8 <= n_nodes <= 65536, 8 <= n_mu <= 1024,
 *           n_nodes n_mu <= 2^20 (32 MiB per table on the device), 1 <= gamma_lo < gamma_hi, every value finite -- else
 *           RIMPHONY_EINVAL, checked on the host, and the previous set stays.
 * S is the tensor-product natural cubic spline through the nodes, evaluated as a bicubic on the cell.  A surface bilinear
 * in (ln gamma, mu), ln n = c - p u + a mu + q u mu -- a power law whose index depends on the pitch angle, times an exponential
 * beam -- is reproduced exactly; a sum H(ln gamma) + G(mu) gives the function rimphony_ctx_set_tables_pitch makes of (H, G),
 * in other arithmetic (agreement to rounding, not to the bit).  A mu a rounding beyond +-1 extrapolates the end cell; a NaN
 * gives NaN.  The natural end condition (second derivative 0 across every edge of the grid) costs accuracy where the surface
 * is curved at an edge: there the error falls with the fourth power of the spacing only in the interior.  g -> 0 at mu = +-1
 * cannot be held in ln n: give it as a sin^k xi prefactor (rimphony_ctx_set_tables_2d_pitchy below), or floor it, as for a pitch
 * row.  A table that ends at a non-negligible n behaves like gamma limits.
 * The normalisation is a property of a table, not of a row: the call integrates it once per table on the device (the
 * 31-point Kronrod rule on every mu cell inside an adaptive quadrature over gamma, eps_rel 1e-8) and keeps it beside the
 * table; rimphony_batch_norm* and the coefficient entries read it.  A table whose quadrature fails has a NaN
 * normalisation: its rows are NaN with RIMPHONY_ST_NORM_FAIL, the other tables are unaffected.  The call therefore takes
 * from about 20 ms (512 x 64 nodes) to a third of a second (1024 x 1024) per table.
 * A context holds one set at a time, of one form: installing a 2-D set replaces an isotropic or pitch set and the other way
 * round; n_tables = 0 clears the set.  A device allocation that fails is RIMPHONY_ENOMEM and the previous set stays.
 * Everything else -- rows and their index, a bad index, the precisions and closed forms refused, the _multi entries, the
 * choice between the group kernel and one wave per coefficient (RIMPHONY_TAB_GROUP) -- is as for rimphony_ctx_set_tables_pitch. */
int rimphony_ctx_set_tables_2d(rimphony_ctx *ctx, size_t n_tables, size_t n_nodes, double gamma_lo, double gamma_hi,
                               size_t n_mu, const double *log_n);

/* Tabulated distributions with a sin^k xi prefactor per table, the anisotropy of RIMPHONY_PITCHY_PL and _KAPPA
 * (pitchy_pl.rs, pitchy_kappa.rs), which no pitch row can hold because its logarithm diverges at mu = +-1:
 * f(gamma, mu) = norm n(gamma) sin^k xi g(mu) / (gamma^2 beta) inside the table, 0 outside;
 * df/dmu = f (G'(mu) - k mu / sin^2 xi), df/dgamma as for the other forms;
 * norm = 1 / (4 pi P int n dgamma), P = 1/2 int_{-1}^{+1} (1 - mu^2)^(k/2) g(mu) dmu.
 *   log_n, n_mu, log_g   exactly as for rimphony_ctx_set_tables_pitch; log_g == NULL with n_mu == 0: no g;
 *   sin_k   HOST, [n_tables]: the exponent k of each table, finite with 0 <= k <= 100 -- else RIMPHONY_EINVAL, checked on
 *           the host, and the previous set stays.
 * sin_k == NULL is rimphony_ctx_set_tables_pitch exactly: the same form, the same kernels, the same bits.  n_tables = 0
 * clears the set.
 * The factor is formed as the pitchy kinds form it, pow(sqrt(1 - mu^2), k), and df/dmu has the form of pitchy_pl.rs:56-61
 * with what that form gives at |mu| = 1: f = 0 and df/dmu = NaN (0 x inf) for k > 0; for k = 0 the factor is 1 and the
 * term 0 mu / 0 is NaN there too.  A mu a rounding beyond +-1 gives NaN (the square root of a negative number), as for
 * the pitchy kinds.
 * Without g, P is the closed form of the pitchy kinds, Gamma(3/2) Gamma(1 + k/2) / Gamma(3/2 + k/2) (pitchy_pl.rs:98).
 * With g the call integrates P once per table on the device, adaptively (eps_rel 1e-8, 1000 subintervals; the integrand's
 * derivative is singular at both ends for a non-integer k), and keeps it beside the table.  A table whose quadrature
 * fails has a NaN P: its rows are NaN with RIMPHONY_ST_NORM_FAIL, the other tables are unaffected.
 * A row is still RIMPHONY_TABULATED with one parameter, the table index.  A context holds one set at a time, of one form:
 * installing this form replaces any other and the other way round.  Everything else -- a bad index, the precisions and
 * closed forms refused, the _multi entries, the choice between the group kernel and one wave per coefficient
 * (RIMPHONY_TAB_GROUP) -- is as for rimphony_ctx_set_tables_pitch. */
int rimphony_ctx_set_tables_pitchy(rimphony_ctx *ctx, size_t n_tables, size_t n_nodes, double gamma_lo, double gamma_hi,
                                   const double *log_n, size_t n_mu, const double *log_g, const double *sin_k);

/* Tabulated distributions on gamma nodes of the caller's choosing, for what nodes uniform in ln gamma cannot resolve: a
 * cold or mildly relativistic core, where ln gamma ~ gamma - 1 and the whole sub-relativistic range falls into the first few
 * intervals of a uniform grid.  Everything else is rimphony_ctx_set_tables_pitchy's:
 * f(gamma, mu) = norm n(gamma) sin^k xi g(mu) / (gamma^2 beta) inside [gamma[0], gamma[n_nodes - 1]], 0 outside.
 *   gamma   HOST, [n_nodes], 8 <= n_nodes <= 65536: the nodes, shared by the tables of the set; finite,
 *           1 <= gamma[0] < gamma[1] < ..., and their logarithms as the library forms them strictly increasing too (two
 *           gamma a rounding apart can share a logarithm: refused);
 *   log_n   HOST, [n_tables][n_nodes]: ln n at the nodes;
 *   n_mu, log_g   as for rimphony_ctx_set_tables_pitch, or 0 / NULL: no g;
 *   sin_k   HOST, [n_tables], each finite in [0, 100], or NULL: no prefactor (k = 0).
 * RIMPHONY_EINVAL, checked on the host, for a null gamma or log_n, a non-finite value, gamma[0] < 1, too few or too many
 * nodes, nodes or logarithms not strictly increasing, and whatever rimphony_ctx_set_tables_pitchy refuses in log_g, n_mu and
 * sin_k: the previous set stays.  n_tables = 0 clears the set.  The call replaces a set of any form and a set of any form
 * replaces it.
 * The interpolant is the natural cubic spline through (ln gamma_j, ln n_j), solved on the host on the non-uniform nodes; a
 * straight line in (ln gamma, ln n) comes back as itself.  A sample finds its interval -- the last node at or below it,
 * whatever the search does to get there -- through a guide of cells uniform in ln gamma and a bisection inside the cell:
 * two guide words and at most 16 node words, 0 to 2 where the nodes are about as dense as the cells.
 * An isotropic set of this form (no g, no sin_k) is computed with the general absorption term, as a set with k = 0 is:
 * the same numbers as the isotropic form to the rounding of the extra term, not the same bits.
 * With g, P is integrated on the device when the set is installed, as for rimphony_ctx_set_tables_pitchy.  A row is still
 * RIMPHONY_TABULATED with one parameter, the table index; everything else is as for rimphony_ctx_set_tables_pitchy. */
int rimphony_ctx_set_tables_grid(rimphony_ctx *ctx, size_t n_tables, size_t n_nodes, const double *gamma, const double *log_n,
                                 size_t n_mu, const double *log_g, const double *sin_k);

/* Tabulated distributions as 2-D surfaces on gamma nodes of the caller's choosing: what rimphony_ctx_set_tables_2d holds -- an
 * anisotropy that grows with energy, a beam on an isotropic core, a loss cone above some gamma -- on the nodes
 * rimphony_ctx_set_tables_grid takes, for a cold or mildly relativistic core under an anisotropic tail (a PIC or Fokker-Planck
 * histogram), which a grid uniform in ln gamma cannot resolve within the 2-D form's node limit.
 * f(gamma, mu) = norm exp(S(ln gamma, mu)) / (gamma^2 beta) inside [gamma[0], gamma[n_nodes - 1]], +0 outside;
 * df/dgamma = f (S_u / gamma - 1 / gamma - gamma / (gamma^2 - 1)), df/dmu = f S_mu; the normalisation as for the 2-D form.
 *   gamma   HOST, [n_nodes], 8 <= n_nodes <= 65536: the nodes, shared by the tables of the set, exactly as for
 *           rimphony_ctx_set_tables_grid: finite, 1 <= gamma[0] < gamma[1] < ..., their logarithms as the library forms them
 *           strictly increasing too;
 *   log_n   HOST, [n_tables][n_nodes][n_mu], mu fastest: ln n at (gamma_i, mu_j), the mu nodes uniform from -1 to +1, end
 *           points included; 8 <= n_mu <= 1024, n_nodes n_mu <= 2^20, every value finite.
 * Anything else is RIMPHONY_EINVAL, checked on the host, and the previous set stays; so it does when a device allocation
 * fails (RIMPHONY_ENOMEM).  n_tables = 0 clears the set.  The call replaces a set of any form and a set of any form replaces it.
 * S is the tensor-product natural cubic spline through the data at (u_i = ln gamma_i, mu_j), solved on the host on the
 * non-uniform u nodes, evaluated as a bicubic on the cell with the cell's own width.  A surface bilinear in (ln gamma, mu)
 * comes back as itself; on nodes uniform in ln gamma the form gives what rimphony_ctx_set_tables_2d gives, and a sum
 * y(gamma_i) + G(mu_j) what rimphony_ctx_set_tables_grid makes of (y, G), each in other arithmetic (agreement to rounding, not
 * to the bit).  A sample finds its interval in u as for rimphony_ctx_set_tables_grid -- the last node at or below it, through
 * two guide words and a bisection of at most 16 node words -- and its mu cell as for the 2-D form: a mu a rounding beyond +-1
 * extrapolates the end cell, a NaN gives NaN.
 * The normalisation of each table is integrated once, on the device, when the set is installed, as for the 2-D form; a table
 * whose quadrature fails has a NaN normalisation and its rows are NaN with RIMPHONY_ST_NORM_FAIL, the other tables are
 * unaffected.  A row is still RIMPHONY_TABULATED with one parameter, the table index.  Everything else -- a bad index, the
 * precisions and closed forms refused, the _multi entries, RIMPHONY_TAB_GROUP (this form follows the 2-D form's default) -- is
 * as for rimphony_ctx_set_tables_2d.  mu nodes of the caller's choosing: rimphony_ctx_set_tables_2d_nodes below.  Not offered:
 * a grid per table. */
int rimphony_ctx_set_tables_2d_grid(rimphony_ctx *ctx, size_t n_tables, size_t n_nodes, const double *gamma, size_t n_mu,
                                    const double *log_n);

/* The two 2-D forms with a sin^k xi prefactor per table, for a distribution that vanishes along the field and whose
 * anisotropy changes with energy -- a loss cone whose depth grows with gamma.  ln n of such a distribution diverges at mu =
 * +-1 and no surface can hold it; the caller divides the histogram by sin^k xi and tabulates the smooth remainder:
 * f(gamma, mu) = norm sin^k xi exp(S(ln gamma, mu)) / (gamma^2 beta) inside the table, +0 outside;
 * df/dmu = f (S_mu - k mu / sin^2 xi), df/dgamma as for the 2-D form it extends;
 * norm = 1 / (4 pi int nbar dgamma), nbar(gamma) = 1/2 int_{-1}^{+1} (1 - mu^2)^(k/2) exp(S) dmu.
 *   sin_k   HOST, [n_tables]: the exponent k of each table, finite with 0 <= k <= 100 -- else RIMPHONY_EINVAL, checked on
 *           the host, and the previous set stays;
 *   everything else exactly as for rimphony_ctx_set_tables_2d and rimphony_ctx_set_tables_2d_grid: shapes, limits, n_nodes n_mu
 *           <= 2^20, n_tables = 0 clearing the set, replacing a set of any form, RIMPHONY_ENOMEM leaving the previous set.
 * sin_k == NULL is the entry without _pitchy exactly: the same form, the same kernels, the same bits.
 * The factor is formed as the pitchy kinds and rimphony_ctx_set_tables_pitchy form it, pow(sqrt(1 - mu^2), k).  At |mu| = 1
 * that form gives f = 0 and df/dmu = NaN (0 x inf) for k > 0; for k = 0 given explicitly the factor is 1 and the term 0 mu /
 * 0 is NaN there too.  A mu a rounding beyond +-1 gives NaN (the square root of a negative number), where the plain 2-D
 * forms extrapolate the end cell.
 * The normalisation of each table is integrated once, on the device, when the set is installed: over gamma adaptively (eps_rel
 * 1e-8, 1000 subintervals), nbar by the 31-point Kronrod rule on every mu cell, the two end cells under the substitution 1 -
 * |mu| = h v^4, which takes the singular derivative of the factor at mu = +-1 out of the integrand for every k (DESIGN.md
 * section 5).  A table whose quadrature fails has a NaN normalisation and its rows are NaN with RIMPHONY_ST_NORM_FAIL.
 * A row is still RIMPHONY_TABULATED with one parameter, the table index; RIMPHONY_TAB_GROUP follows the 2-D form's default.
 * mu nodes of the caller's choosing: rimphony_ctx_set_tables_2d_nodes below.  Not offered: a grid per table, an exponent per
 * row. */
int rimphony_ctx_set_tables_2d_pitchy(rimphony_ctx *ctx, size_t n_tables, size_t n_nodes, double gamma_lo, double gamma_hi,
                                      size_t n_mu, const double *log_n, const double *sin_k);
int rimphony_ctx_set_tables_2d_grid_pitchy(rimphony_ctx *ctx, size_t n_tables, size_t n_nodes, const double *gamma, size_t n_mu,
                                           const double *log_n, const double *sin_k);

/* Tabulated distributions as 2-D surfaces on gamma nodes AND mu nodes of the caller's choosing, with or without a sin^k xi
 * prefactor: what the 2-D forms above hold, for an anisotropy that nodes uniform in mu cannot resolve within 1024 of them --
 * a pitch-angle histogram with bins uniform in xi (finest at mu = +-1, where a uniform mu grid is coarsest in angle), a
 * field-aligned beam, a ring at one pitch angle, the edge of a loss cone.
 * f(gamma, mu) = norm sin^k xi exp(S(ln gamma, mu)) / (gamma^2 beta) inside [gamma[0], gamma[n_nodes - 1]], +0 outside;
 * df/dgamma and df/dmu as for the 2-D forms.
 *   gamma   HOST, [n_nodes]: exactly as for rimphony_ctx_set_tables_2d_grid (nodes uniform in ln gamma are simply passed in);
 *   mu      HOST, [n_mu], shared by the tables of the set: 8 <= n_mu <= 1024, n_nodes n_mu <= 2^20, every value finite and
 *           strictly increasing, mu[0] == -1.0 and mu[n_mu - 1] == +1.0 exactly -- the surface covers the whole range, and the
 *           normalisation needs no extrapolation;
 *   log_n   HOST, [n_tables][n_nodes][n_mu], mu fastest: ln n (with sin_k: of the smooth remainder n / sin^k xi) at (gamma_i,
 *           mu_j), every value finite;
 *   sin_k   NULL, or HOST [n_tables], each finite with 0 <= k <= 100, with the semantics of the _2d*_pitchy entries: a mu a
 *           rounding beyond +-1 is NaN, df/dmu is NaN at |mu| = 1.  sin_k == NULL is the plain function: the end cell
 *           extrapolates for a mu a rounding beyond +-1, a NaN gives NaN.
 * Anything else -- a null pointer, a non-finite value, mu not strictly increasing, wrong end nodes, a bad n_mu, gamma, log_n or
 * sin_k -- is RIMPHONY_EINVAL, checked on the host before any lock or HIP call, and the previous set stays; so it does when
 * a device allocation fails (RIMPHONY_ENOMEM).  n_tables = 0 clears the set.  The call replaces a set of any form and a set
 * of any form replaces it.
 * S is the tensor-product natural cubic spline through the data at (rim_log(gamma_i), mu_j), solved on the host on both
 * non-uniform node sets, evaluated as a bicubic on the cell with the cell's own widths.  A surface bilinear in (ln gamma, mu)
 * comes back as itself on any node set; on mu nodes -1 + j 2 / (n_mu - 1) the form gives what rimphony_ctx_set_tables_2d_grid
 * (and, with sin_k, rimphony_ctx_set_tables_2d_grid_pitchy) gives, in other arithmetic: agreement to rounding, not to the bit.
 * A sample finds its mu interval as it finds its gamma interval: the largest j <= n_mu - 2 with mu_j <= mu (0 where there is
 * none or mu is a NaN), through two words of a guide over cells uniform in mu and a bisection of at most 10 node words.
 * The normalisation of each table is integrated once, on the device, when the set is installed: the 31-point Kronrod rule
 * on every mu cell with that cell's centre and half width and, under sin^k, the two end cells under 1 - |mu| = h v^4 with h
 * the end cell's own width.  A table whose quadrature fails has a NaN normalisation and its rows are NaN with
 * RIMPHONY_ST_NORM_FAIL.  A row is still RIMPHONY_TABULATED with one parameter, the table index; a bad index, the refused
 * precision, the refused closed forms and the _multi entries behave as for the 2-D forms; RIMPHONY_TAB_GROUP follows the 2-D
 * form's default.  Not offered: a grid per table, an exponent per row. */
int rimphony_ctx_set_tables_2d_nodes(rimphony_ctx *ctx, size_t n_tables, size_t n_nodes, const double *gamma, size_t n_mu,
                                     const double *mu, const double *log_n, const double *sin_k);

/* Any of the six 2-D forms above from ln n in DEVICE memory: for a caller whose ln n(gamma, mu) is made on the GPU (a PIC or
 * Fokker-Planck post-processing step) and who would otherwise copy it to the host, wait for the host's serial spline solve
 * and have four times as much copied back.
 *   gamma     NULL: nodes uniform in ln gamma from gamma_lo to gamma_hi; or HOST [n_nodes], as for
 *             rimphony_ctx_set_tables_2d_grid (gamma_lo and gamma_hi are then not read);
 *   mu        NULL: nodes uniform in mu from -1 to +1; or HOST [n_mu], as for rimphony_ctx_set_tables_2d_nodes.  mu without
 *             gamma is no form: RIMPHONY_EINVAL;
 *   d_log_n   DEVICE, on the context's GPU, [n_tables][n_nodes][n_mu], mu fastest, every value finite;
 *   sin_k     NULL, or HOST [n_tables], as for the entries with a prefactor;
 *   stream    the stream that produced d_log_n: the install runs on it, behind that work.
 * So gamma == NULL, mu == NULL installs what rimphony_ctx_set_tables_2d (sin_k: _2d_pitchy) installs, gamma alone what
 * rimphony_ctx_set_tables_2d_grid (_2d_grid_pitchy) installs, both what rimphony_ctx_set_tables_2d_nodes installs: the set on
 * the device is that entry's set from the same numbers WORD FOR WORD -- headers, guides, node words, the four words per node
 * and the normalisations -- so everything said of that form above holds unchanged.  The headers, guides and node words are
 * built on the host as ever; the node data are solved on the device, one lane per spline line, with the swept diagonals of the
 * two axes formed once on the host and every operation in the host solver's form; the normalisations are integrated by the
 * form's own kernel.
 * Refused with RIMPHONY_EINVAL, the previous set staying in place: the geometry the form's host entry refuses; a null
 * d_log_n; a d_log_n that the runtime does not report as memory of the context's GPU holding the whole array (a host pointer,
 * another GPU's memory); a non-finite value anywhere in d_log_n, which a kernel looks for before anything is built.
 * RIMPHONY_ENOMEM likewise.  n_tables = 0 clears the set.  Synchronous like the host entries: `stream` has been synchronised
 * when the call returns.  For the length of the call the new set, the previous one and d_log_n are all resident.  Not
 * offered: the 1-D forms (their sets are small), an asynchronous install. */
int rimphony_ctx_set_tables_2d_device(rimphony_ctx *ctx, size_t n_tables, size_t n_nodes, const double *gamma, double gamma_lo,
                                      double gamma_hi, size_t n_mu, const double *mu, const double *d_log_n, const double *sin_k,
                                      void *stream);

/* The ends of the spline of a 2-D set, a choice per axis.  Every 2-D entry above interpolates with NATURAL ends: the second
 * derivative of S across an end node is 0 -- S_uu = 0 at both ends of the gamma nodes, S_mumu = 0 at mu = +-1.  Along gamma the
 * caller tapers the table and the ends carry nothing.  Along mu there is nothing to taper: mu = +-1 is the field direction,
 * and a smooth distribution on the sphere generally has curvature there (a bi-Maxwellian's ln n is quadratic in mu).  With
 * natural ends the error of S_mu near the pole falls only like the node distance, and S_mu is what df/dmu = f S_mu feeds into
 * every absorption coefficient and into rho_Q and rho_V.  NOT-A-KNOT ends make the third derivative of S continuous across
 * the second and the second-to-last node instead: every cubic along the axis comes back as itself, and the error is O(h^4) up
 * to the edge (profiles/tabulated_2d_ends_accuracy.txt has the figures).
 * The two entries below are rimphony_ctx_set_tables_2d_device's shape, for ln n in HOST memory and in DEVICE memory: one entry
 * for all six 2-D forms, gamma, mu and sin_k NULL or given with the meaning they have there.
 *   ends_gamma   governs the sweeps along ln gamma (S_u and S_umu), ends_mu the sweeps along mu (S_mu): each
 *                RIMPHONY_TAB_ENDS_NATURAL or RIMPHONY_TAB_ENDS_NOT_A_KNOT.  Any other value is RIMPHONY_EINVAL, and the
 *                previous set stays;
 *   everything else as for the form's own entry, which is what checks and builds the set: what it refuses is refused here,
 *                n_tables = 0 clears, a set of any form is replaced.
 * With natural ends on both axes each installs exactly the set of the form's existing entry, word for word; the device entry
 * installs the host entry's set word for word for every choice.  The choice costs nothing per sample: the kernels read {S,
 * S_u, S_mu, S_umu} per node and never ask how they were solved.  It is recorded in a spare word of each table's header
 * (ends_gamma + 2 ends_mu; rimphony_debug_tables shows it) that no kernel reads.
 * Not offered: the 1-D forms (a separable table can be given as a surface); clamped ends with slopes given by the caller; a
 * choice per table. */
#define RIMPHONY_TAB_ENDS_NATURAL 0
#define RIMPHONY_TAB_ENDS_NOT_A_KNOT 1
int rimphony_ctx_set_tables_2d_ends(rimphony_ctx *ctx, size_t n_tables, size_t n_nodes, const double *gamma, double gamma_lo,
                                    double gamma_hi, size_t n_mu, const double *mu, const double *log_n, const double *sin_k,
                                    int ends_gamma, int ends_mu);
int rimphony_ctx_set_tables_2d_device_ends(rimphony_ctx *ctx, size_t n_tables, size_t n_nodes, const double *gamma, double gamma_lo,
                                           double gamma_hi, size_t n_mu, const double *mu, const double *d_log_n,
                                           const double *sin_k, int ends_gamma, int ends_mu, void *stream);

/* Tabulated distributions as a FAMILY with a continuous index per row: a set of energy tables on nodes uniform in ln gamma,
 * optionally with a sin^k xi exponent per table, where the one parameter of a RIMPHONY_TABULATED row is a REAL index x and
 * every sample blends two neighbouring tables -- a Fokker-Planck run stored at 64 times, a cooling sequence, a scan over
 * magnetisation, evaluated between the stored states.
 *   log_n   HOST, [n_tables][n_nodes]: ln n at the nodes, shapes and limits exactly as for rimphony_ctx_set_tables;
 *   sin_k   NULL, or HOST [n_tables]: the exponent of each table, range and meaning as for rimphony_ctx_set_tables_pitchy
 *           (there is no log_g here).
 * Checked with the plain forms' own checks (RIMPHONY_EINVAL, the previous set stays); n_tables = 0 clears the set; the call
 * replaces a set of any form and a set of any form replaces it; rimphony_debug_tables reads the set back.
 * The index rule of a row:
 *   valid   x finite and 0 <= x <= n_tables - 1; -0.0 counts as 0;
 *   tables  a = (long long) x the lower one, b = a + 1 the upper one -- except at a == n_tables - 1, where b = a;
 *   weight  w = x - a;
 *   blend   H = H_a + w (H_b - H_a) for the spline and k = k_a + w (k_b - k_a) for the exponent, each as one
 *           fma(w, q_b - q_a, q_a) per quantity -- the four node words of the sample's interval, then ONE cubic --, so that
 *           w = 0 gives q_a itself;
 *   f       = norm e^H sin^k xi / (gamma^2 beta) inside the table, 0 outside, with the derivatives of the plain forms;
 *   else    a NaN, an index out of range or a non-integer beyond the last table is a NaN normalisation: every selected slot
 *           of the row is NaN with RIMPHONY_ST_NORM_FAIL, as for a bad index of the other forms.
 * The normalisation is per row: norm = 1 / (4 pi P(k) int e^H dgamma) over the blended spline with the settings of the plain
 * forms, P(k) the closed form of the pitchy kinds at the blended k (1 without sin_k).  Nothing is integrated at install.
 * A row at an integer x carries the BITS of the same table installed through rimphony_ctx_set_tables (no sin_k) or
 * rimphony_ctx_set_tables_pitchy (sin_k, no g): values, status words, work counters, the normalisation and calc_f.  The
 * existing entries keep refusing a non-integer index.
 * The blend is linear in the index, and exact where ln n is linear in the parameter the tables are spaced in: ln n of a power
 * law in p, ln n of a Juettner shape in 1 / T, ln sin^k xi in k.  Two tables reproduce the analytic power law at every p
 * between them (and with sin_k the pitchy power law at every (p, k)) to the accuracy of the plain form.  Elsewhere the error
 * is that of linear interpolation of ln n between neighbouring tables.
 * RIMPHONY_TAB_GROUP chooses between the group kernel and one wave per coefficient as for the other forms (the same bits).
 * Not offered: families of the forms with g or on given gamma nodes (2-D surfaces: rimphony_ctx_set_tables_2d_family); families
 * in two parameters; higher-order blending across the tables of this form, which stays linear (2-D surfaces:
 * rimphony_ctx_set_tables_2d_family_cubic); a crank-out subcommand; a bench leg. */
int rimphony_ctx_set_tables_family(rimphony_ctx *ctx, size_t n_tables, size_t n_nodes, double gamma_lo, double gamma_hi,
                                   const double *log_n, const double *sin_k);

/* Tabulated distributions as a FAMILY OF 2-D SURFACES with a continuous index per row: a set of surfaces ln n(gamma, mu) on
 * gamma nodes and mu nodes of the caller's choosing, optionally with a sin^k xi exponent per table, where the one parameter
 * of a RIMPHONY_TABULATED row is a REAL index x and every sample blends two neighbouring surfaces -- a PIC or Fokker-Planck
 * run whose anisotropy changes with energy, stored at 64 times and evaluated between them.
 *   gamma, mu, log_n [n_tables][n_nodes][n_mu], sin_k (NULL, or HOST [n_tables])
 *           exactly what rimphony_ctx_set_tables_2d_nodes accepts, with its limits: 8 .. 65536 gamma nodes, 8 .. 1024 mu
 *           nodes from exactly -1 to exactly +1, n_nodes * n_mu <= 2^20 per table, k in [0, 100].  Nodes uniform in ln gamma
 *           or in mu are a special case: pass them;
 *   ends_gamma, ends_mu
 *           RIMPHONY_TAB_ENDS_NATURAL or RIMPHONY_TAB_ENDS_NOT_A_KNOT per axis, as for rimphony_ctx_set_tables_2d_ends.
 * Checked with the plain form's own check (RIMPHONY_EINVAL, the previous set stays); n_tables = 0 clears the set; the call
 * replaces a set of any form and a set of any form replaces it; rimphony_debug_tables reads the set back: the set of
 * rimphony_ctx_set_tables_2d_nodes word for word, but for the normalisation word of every table header, which is a NaN (no
 * trailing copy of the last table).
 * The index rule of a row is that of rimphony_ctx_set_tables_family:
 *   valid   x finite and 0 <= x <= n_tables - 1; -0.0 counts as 0;
 *   tables  a = (long long) x the lower one, b = a + 1 the upper one -- except at a == n_tables - 1, where b = a;
 *   weight  w = x - a;
 *   blend   the gamma interval and the mu interval of a sample are found once; the sixteen node words {S, S_u, S_mu, S_umu}
 *           of the cell's four corners are read from table a and from table b, each pair blended with one
 *           fma(w, q_b - q_a, q_a), then ONE bicubic; k = fma(w, k_b - k_a, k_a).  The bicubic is linear in its node words
 *           and the spline solve is linear in the data, for either kind of ends: this is the spline of the blended data;
 *   f       = norm sin^k xi e^S / (gamma^2 beta) inside the table, 0 outside, with the derivatives of the plain form -- the
 *           NaN at |mu| = 1 with a prefactor included;
 *   else    a NaN, or an index out of range, is a NaN normalisation: every selected slot of the row is NaN with
 *           RIMPHONY_ST_NORM_FAIL.
 * The normalisation is per row and nothing is integrated at install: norm = 1 / (4 pi int nbar dgamma) over [gamma_0,
 * gamma_last] with nbar(gamma) = 1/2 int (1 - mu^2)^(k/2) e^S dmu over the blended surface at the blended k, the quadrature
 * the plain form runs once per table as the set comes in (31 Kronrod points on every mu cell, the end cells of a set with a
 * prefactor under their substitution).  Its cost is linear in n_mu: 56, 512 and 2080 ms for 4096 rows on 8, 64 and 256 mu
 * nodes of a 128-node family on an MI355X (50, 466, 1903 ms with a prefactor), where the two persistent kernels of such a
 * batch take 473 ms (941 ms); per sample the blend costs +14 % (Symphony, group kernel) and +44 % (Faraday) on the plain
 * nodes form, +36 % and +51 % with a prefactor (profiles/tabulated_2d_family_times.txt).  Keep the mu nodes few.
 * A row at an integer x carries the BITS of the same table installed through rimphony_ctx_set_tables_2d_ends on the same
 * nodes with the same sin_k and ends: values, status words, work counters, the normalisation and calc_f -- with one caveat:
 * fma(0, d, -0.0) is +0.0, so a node word that is -0.0 enters the bicubic as +0.0 (the sign of a zero node word is not kept).
 * The existing entries keep refusing a non-integer index.
 * The blend is linear in the index, exact where ln n is linear in the parameter the tables are spaced in, and elsewhere has
 * the error of linear interpolation of ln n between neighbouring tables (profiles/tabulated_2d_family_accuracy.txt).
 * RIMPHONY_TAB_GROUP chooses between the group kernel and one wave per coefficient as for the other forms (the same bits).
 * Not offered: families of the uniform-grid 2-D forms as forms of their own (pass the nodes); families of the 1-D forms with
 * g or on given gamma nodes; install from device memory; families in two parameters; a blend of higher order than cubic
 * (cubic: rimphony_ctx_set_tables_2d_family_cubic); one normalisation shared by rows with equal x. */
int rimphony_ctx_set_tables_2d_family(rimphony_ctx *ctx, size_t n_tables, size_t n_nodes, const double *gamma, size_t n_mu,
                                      const double *mu, const double *log_n, const double *sin_k, int ends_gamma, int ends_mu);

/* The family of 2-D surfaces of rimphony_ctx_set_tables_2d_family blended CUBICALLY across its tables: a 4-point Lagrange cubic
 * in the parameter the tables are spaced in, chosen at install, per set.  For a simulation stored at a handful of snapshots,
 * where the linear blend's error -- a quarter per doubling of the tables -- cannot be bought down with more tables.
 *   n_tables .. ends_mu
 *           exactly what rimphony_ctx_set_tables_2d_family accepts, with n_tables >= 4;
 *   param   NULL, or HOST [n_tables]: the knots c_t the tables are spaced in (a temperature, 1 / T, a time), finite and strictly
 *           monotonic, increasing or decreasing.  NULL: c_t = t.
 * Checked as the linear entry checks (RIMPHONY_EINVAL, the previous set stays) -- fewer than four tables and knots that are
 * not finite or not monotonic included; n_tables = 0 clears the set; the call replaces a set of any form and a set of any form
 * replaces it; rimphony_debug_tables reads the set back: the set of rimphony_ctx_set_tables_2d_family word for word, followed
 * by the n_tables knot words.  No new solve and no extra memory per table: the bicubic is linear in its node words and the
 * spline solve is linear in the data, so a fixed combination of solved tables is the solved combination.
 * The parameter of a row stays the real index x, with the rule of the linear entry: valid where x is finite and
 * 0 <= x <= n_tables - 1, a = (long long) x, w = x - a, b = a + 1 (b = a at the last table).  Then, per row:
 *   p       = fma(w, c_b - c_a, c_a): at an integer x a knot, bit for bit;
 *   stencil the tables s .. s + 3 with s = min(max(a - 1, 0), n_tables - 4);
 *   weights L_i = prod over j != i, j ascending, starting from 1, of (p - c_{s+j}) / (c_{s+i} - c_{s+j}): at a knot exactly 1
 *           for that table and a zero for the others;
 *   k       with sin_k, fma(L_3, k_3, fma(L_2, k_2, fma(L_1, k_1, L_0 k_0))) over the stencil.  A cubic may overshoot: a row
 *           whose blended k is not in [0, 100] is a NaN row with RIMPHONY_ST_NORM_FAIL.  Space sin_k smoothly;
 *   blend   the gamma interval and the mu interval of a sample are found once; each of the cell's sixteen node words is
 *           fma(L_3, q_3, fma(L_2, q_2, fma(L_1, q_1, L_0 q_0))) of the stencil's four tables, then ONE bicubic;
 *   f, the NaN rows and the per-row normalisation: as for the linear entry, over the blended surface at the blended k.
 * A row at an integer x carries the BITS of that table installed through rimphony_ctx_set_tables_2d_ends with the same nodes,
 * sin_k and ends -- values, status words, work counters, the normalisation and calc_f --, with the linear entry's caveat: the
 * sign of a zero node word is not kept.
 * Accuracy and cost (profiles/tabulated_2d_family_cubic_accuracy.txt, profiles/tabulated_2d_family_cubic_times.txt): exact,
 * to the accuracy of the plain form, where ln n is a cubic polynomial in the knots; elsewhere the error of 4-point
 * interpolation, fourth order in the spacing: on a Juettner shape whose anisotropy depends on T, spaced in 1 / T, 1.4e-3 on 4
 * tables and 1.1e-4 on 8 where the linear blend has 1.1e-2 and 2.6e-3 -- four tables blended cubically beat eight blended
 * linearly.  A sample reads four runs of node words instead of two: measured on an MI355X against the linear blend of the same
 * four 1 MiB tables at the same x, +21 % per Symphony sample (group kernel) and +40 % per Faraday sample; with a prefactor 2.3 x
 * on both (its kernels spill 300 B more per lane); the per-row normalisation of 4096 rows 81 against 56 ms on 8 mu nodes and 741
 * against 515 ms on 64 (84 / 50 and 777 / 470 ms with a prefactor).
 * RIMPHONY_TAB_GROUP chooses between the group kernel and one wave per coefficient as for the other forms (the same bits).
 * Not offered: cubic blending for the families of energy tables (rimphony_ctx_set_tables_family stays linear); what the linear
 * entry does not offer. */
int rimphony_ctx_set_tables_2d_family_cubic(rimphony_ctx *ctx, size_t n_tables, size_t n_nodes, const double *gamma, size_t n_mu,
                                            const double *mu, const double *log_n, const double *sin_k, int ends_gamma, int ends_mu,
                                            const double *param);

/* Diagnostics: the installed table set as the kernels read it, copied to `out` (HOST, `cap` doubles).  *n_doubles is the
 * size of the set in doubles, 0 (and nothing copied) where the context has none; RIMPHONY_EINVAL, with *n_doubles still set,
 * where cap is smaller.  The set holds offsets, never addresses, so two installs of the same numbers -- through a host entry
 * and through rimphony_ctx_set_tables_2d_device, say -- compare word for word. */
int rimphony_debug_tables(rimphony_ctx *ctx, double *out, size_t cap, size_t *n_doubles);

/* Work counters of the most recent batch call on this context (device-side
 * counts, read back synchronously): integrand samples, wave-wide evaluation
 * passes, inner QAG calls. */
typedef struct {
    uint64_t samples;               /* Symphony kernel */
    uint64_t passes;
    uint64_t inner_qags;
    uint64_t faraday_samples;       /* Heyvaerts kernel */
    uint64_t faraday_passes;
    uint64_t faraday_inner_qags;
} rimphony_work;
int rimphony_last_work(rimphony_ctx *ctx, rimphony_work *out);

/* The tail of the most recent batch call (device-side, read back synchronously).  Per-task cost has a heavy tail and the
 * reference's chunk marching is sequential: the task with the longest CHAIN of batches (each waits for its slowest
 * gamma-integral / inner integral) bounds how early a launch can end, whatever the cooperative tail spreads out.
 *   out[0], out[1]   Symphony: batches of the heaviest coefficient, and its row (rows to 2^40)
 *   out[2], out[3]   Faraday: the same
 *   out[4]           Symphony group kernel: passes the coefficients would have executed one by one (out[4] / passes of
 *                    rimphony_last_work = how many coefficients an executed pass served on average)
 *   out[5]           ... rule sums filed ahead of a coefficient's own pick (the stash of symphony_group.h)
 *   out[6], out[7]   the same two for the Faraday pair (heyvaerts_group.h) */
int rimphony_last_tail(rimphony_ctx *ctx, uint64_t out[8]);

/* Duration of the most recent Symphony kernel launch of this context, measured
 * with HIP events recorded on the stream the kernel was launched on (waits for
 * the kernel to finish). */
int rimphony_last_symphony_ms(rimphony_ctx *ctx, float *ms);
/* Same for the Faraday (Heyvaerts) launch of the most recent batch call. */
int rimphony_last_faraday_ms(rimphony_ctx *ctx, float *ms);

/* Diagnostics: 16 heartbeat words in host-mapped memory, updated by the wave that
 * works on task number `task` (= point * nslots + slot index) of subsequent
 * batch calls while the kernel runs -- the counterpart of the reference drivers'
 * "write the parameters before computing so a hang can be reconstructed"
 * (examples/crank-out-pitchykappa.rs:193-200).  Words: [0] task+1, [1] batches,
 * [2] phase, [3] integrand passes, [4] inner QAG iteration, [5] chunks,
 * [6] n_start bits, [7] delta_n bits, [8] lane of the running gamma-integral,
 * [9] its n (bits), [10] 1 when the task has finished.  Tasks of the Heyvaerts kernel
 * are addressed as task | (1 << 62).  Symphony tasks are watched in the one-wave-per-coefficient kernel only
 * (RIMPHONY_SYM_SOLO=1 when the context is created); the group kernel does not write heartbeats, so for a Symphony
 * task of a context without that setting the call returns RIMPHONY_ENOTSUP instead of handing out words that would
 * never change. */
int rimphony_debug_heartbeat(rimphony_ctx *ctx, uint64_t task, uint64_t **host_words);

/* Diagnostics: the 16 raw device counter words of the most recent batch call: [0] task head,
 * [1..3] Symphony samples / passes / inner QAGs, [4] Faraday task head, [5..7] Faraday work,
 * [8] batches published on the assist board, [9] requests evaluated by helper waves,
 * [10] requests of published batches evaluated by their owner, [11] owner wait (100 MHz ticks),
 * [12] helper polls, [13] helper visits that found every request already claimed, [14] ticks spent
 * evaluating requests, [15] the task with the most batches as (batches << 24) | point index.  Words 8..15 are only counted by a library built with
 * -DRIM_COOP_DIAG (tools/ab_assist.py); they are 0 otherwise.  `out` must hold 32 words (a -DRIM_PROF build
 * returns its 32 region timers instead, tools/region_profile.py). */
int rimphony_debug_counters(rimphony_ctx *ctx, uint64_t out[32]);

/* The batched compute(): N x (full_calculation + compute_all_dimensionless).
 *   d_s, d_theta   [n]                device
 *   d_params       host array of rimphony_dist_nparams(kind) DEVICE pointers, each [n]
 *   d_out          [n][8] row-major   device
 *   d_status       [n][8] int32 or NULL
 * Asynchronous on `stream`. */
int rimphony_batch_compute_device(rimphony_ctx *ctx, int dist_kind, size_t n,
                                  const double *d_s, const double *d_theta,
                                  const double *const *d_params, uint32_t coeff_mask,
                                  double *d_out, int32_t *d_status, void *stream);

/* Same with HOST buffers (copies in, computes, copies out, synchronises). */
int rimphony_batch_compute(rimphony_ctx *ctx, int dist_kind, size_t n,
                           const double *s, const double *theta,
                           const double *const *params, uint32_t coeff_mask,
                           double *out, int32_t *status);

/* The same two with the remaining arguments of SURVEY 8b's batch ABI:
 *   precision   RIMPHONY_PRECISION_*
 *   d_work/work optional [n][8] uint64: integrand samples spent on each coefficient (0 for unselected slots) --
 *               the per-point counterpart of the reference's per-call trace lines (symphony.rs:69-75, 217-223,
 *               272-275) and of the crank-out drivers' per-row `time_ms(meta)` column
 *               (examples/crank-out-pitchypl.rs:167-173): cost in units that do not depend on what else ran. */
int rimphony_batch_compute_device_ex(rimphony_ctx *ctx, int dist_kind, size_t n,
                                     const double *d_s, const double *d_theta,
                                     const double *const *d_params, uint32_t coeff_mask, int precision,
                                     double *d_out, int32_t *d_status, uint64_t *d_work, void *stream);
int rimphony_batch_compute_ex(rimphony_ctx *ctx, int dist_kind, size_t n,
                              const double *s, const double *theta,
                              const double *const *params, uint32_t coeff_mask, int precision,
                              double *out, int32_t *status, uint64_t *work);

/* Multi-GPU batch (SURVEY 8b `n_devices`, 8e): HOST buffers, one context per device in ctxs[0..n_ctx-1].  Row i is
 * evaluated by ctxs[i mod n_ctx] (interleaved sharding; one host thread per context; no exchange between devices
 * while they compute) and lands in row i of out / status / work.  The table does not depend on n_ctx.  This is the
 * in-process form; the one-process-per-GPU form with an RCCL gather is rimphony_amd/sharding.py + bench.py. */
int rimphony_batch_compute_multi(rimphony_ctx *const *ctxs, int n_ctx, int dist_kind, size_t n,
                                 const double *s, const double *theta, const double *const *params,
                                 uint32_t coeff_mask, int precision, double *out, int32_t *status, uint64_t *work);

/* The same with DEVICE buffers: ctxs[r] (bound to its own device) evaluates the n_local[r] rows its arrays hold --
 * d_s[r], d_theta[r], d_params[r][k], d_out[r] ([n_local[r]][8]), optionally d_status[r], d_work[r], on streams[r] (or the
 * null stream if `streams` is NULL).  All launches are issued from the calling thread before anything is waited for; with
 * `synchronize` != 0 the call returns when every device has finished, otherwise it is asynchronous on the given streams.
 * Which rows a context holds is the caller's choice; rimphony_rccl_gather_table assumes the interleaved convention
 * (row i of the table on rank i mod world).  Replaces N concurrent calls of lib.rs:178-191's loop body. */
int rimphony_batch_compute_multi_device(rimphony_ctx *const *ctxs, int n_ctx, int dist_kind, const size_t *n_local,
                                        const double *const *d_s, const double *const *d_theta,
                                        const double *const *const *d_params, uint32_t coeff_mask, int precision,
                                        double *const *d_out, int32_t *const *d_status, uint64_t *const *d_work,
                                        void *const *streams, int synchronize);

/* The one collective of the path, for a host that is not Python (north_star: "RCCL gather over xGMI for the output
 * table"; the Python form is rimphony_amd/sharding.py).  librccl.so.1 is dlopen'ed on the first of these calls
 * (RIMPHONY_RCCL_LIB overrides the name); the library does not link against it.  One process per GPU:
 *   rimphony_rccl_available()        1 if librccl could be loaded, else 0 (rimphony_last_error() says why)
 *   rimphony_rccl_unique_id(id)      rank 0: fill 128 bytes, to be handed to the other ranks by the caller's own means
 *   rimphony_rccl_comm_create(..)    ncclCommInitRank on the context's device; *comm is an ncclComm_t
 *   rimphony_rccl_gather_table(..)   every rank: d_shard = its [ceil((n_total - rank) / world)][8] rows of the interleaved
 *                                    table (device); root: d_table [n_total][8] (device) receives row i from rank i mod
 *                                    world.  One grouped send / receive per rank (the root sends to itself too, so a world
 *                                    of one runs the same RCCL calls) and an un-interleave kernel, all on `stream`.
 *                                    d_scratch: n_total * 8 doubles on the root (ignored elsewhere); NULL = allocated
 *                                    and freed inside, and the call then returns synchronised.
 *   rimphony_rccl_comm_destroy(comm)
 * A comm created elsewhere (the caller's own RCCL binding) is accepted as well: it is only passed through. */
int rimphony_rccl_available(void);
int rimphony_rccl_unique_id(void *id128);
int rimphony_rccl_comm_create(rimphony_ctx *ctx, int rank, int world, const void *id128, void **comm);
int rimphony_rccl_comm_destroy(void *comm);
int rimphony_rccl_gather_table(rimphony_ctx *ctx, void *comm, int rank, int world, int root, size_t n_total,
                               const double *d_shard, double *d_table, double *d_scratch, void *stream);

/* Status histogram of a computed table: hist[slot * 8 + b] = rows whose status word of `slot` has bit b set
 * (b = 0..6, the RIMPHONY_ST_* bits in order), hist[slot * 8 + 7] = rows with status 0.  Synchronous. */
int rimphony_status_histogram_device(rimphony_ctx *ctx, size_t n, const int32_t *d_status, uint64_t hist[64], void *stream);

/* full_calculation() alone: the normalisation constant of each point
 * (power_law.rs:93-103 etc.); NaN where the integral failed. */
int rimphony_batch_norm_device(rimphony_ctx *ctx, int dist_kind, size_t n,
                               const double *const *d_params, double *d_norm, void *stream);

/* leung-bessel seam (leung-bessel/src/lib.rs:36-42), batched:
 * d_j[i] = pkgw_bessel_j(d_n[i], d_x[i]), d_dj[i] = pkgw_bessel_dj(d_n[i], d_x[i]);
 * either output may be NULL. */
int rimphony_bessel_batch_device(rimphony_ctx *ctx, size_t count, const double *d_n, const double *d_x,
                                 double *d_j, double *d_dj, void *stream);

/* Diagnostic seam: FullSynchrotronCalculator::diagnostic_symphony_gamma_integrand
 * (lib.rs:278-285), batched over (n, gamma) pairs for ONE parameter point given
 * as host scalars.  params: host array of the kind's parameters. */
int rimphony_gamma_integrand_batch_device(rimphony_ctx *ctx, int dist_kind, const double *params,
                                          int coeff, int stokes, double s, double theta,
                                          size_t count, const double *d_n, const double *d_gamma,
                                          double *d_out, void *stream);

/* Diagnostic seam: diagnostic_symphony_gamma_integral (lib.rs:266-272), batched
 * over orders n for one parameter point; negative_lobe selects the Stokes-V lobe. */
int rimphony_gamma_integral_batch_device(rimphony_ctx *ctx, int dist_kind, const double *params,
                                         int coeff, int stokes, int negative_lobe, double s, double theta,
                                         size_t count, const double *d_n, double *d_out, void *stream);

/* Unit seam: one leaf function of rimphony_amd/csrc/detmath.h over arrays, as the kernels evaluate it
 * (the parity contract is that gcc/x86-64 and hipcc/gfx950 give the same bits for these).
 * op: 0 exp, 1 log, 2 log10, 3 pow(x, y), 4 sqrt, 5 log10_region, 6 lgamma (x > 0), 7 sin, 8 cos,
 * 9 rim_div_by(x, y, 1/y), 10 cbrt (positive normal x), 11 1/Gamma(x) (-8.5 < x < 9.5), 12 rim_third_powers(x)[(int) y],
 * 13 x^(-1/4) (positive normal x), 14 rim_powexp_normal(x, y, -x/1000).  d_y is only read by ops 3, 9, 12 and 14. */
int rimphony_detmath_batch_device(rimphony_ctx *ctx, int op, size_t n, const double *d_x, const double *d_y,
                                  double *d_out, void *stream);

/* The reference's own scalar FFI seam, leung-bessel/src/lib.rs:36-42
 *   extern { fn pkgw_bessel_j(n: c_double, x: c_double) -> c_double; fn pkgw_bessel_dj(...) -> c_double; }
 * exported under the same names so that crate can link this library in place of leung-bessel/src/bessel.c.
 * HOST code (the host build of the device function): no HIP call, works without a GPU, reentrant; returns the
 * same bits as rimphony_bessel_batch_device.  Failure -> NaN (the seam's convention, bessel.c:327-333, 382-388). */
double pkgw_bessel_j(double n, double x);
double pkgw_bessel_dj(double n, double x);

/* High-frequency closed-form Faraday coefficients: `high_freq_approximation()` of
 * PowerLawDistribution (power_law.rs:117-170; d_params = {p, gamma_min, ...}) and of
 * ThermalJuettnerDistribution (thermal_juettner.rs:78-142; d_params = {T}).  Other kinds: RIMPHONY_EINVAL
 * (the reference has none).  d_out is [n][2] = {rho_Q, rho_V}, dimensionless.  As in the reference no
 * check is made that the parameters lie where the approximation is good. */
int rimphony_highfreq_batch_device(rimphony_ctx *ctx, int dist_kind, size_t n, const double *d_s, const double *d_theta,
                                   const double *const *d_params, double *d_out, void *stream);
/* The same with host buffers (synchronous). */
int rimphony_highfreq_batch(rimphony_ctx *ctx, int dist_kind, size_t n, const double *s, const double *theta,
                            const double *const *params, double *out);

/* Diagnostic seam: diagnostic_symphony_n_integral (lib.rs:254-260 -> symphony.rs:298-307), the QAG over the
 * harmonic number n in [n_lo[i], n_hi[i]] of the gamma-integral, for one parameter point.  A GSL error of the
 * reference (its Err) is NaN here. */
int rimphony_n_integral_batch_device(rimphony_ctx *ctx, int dist_kind, const double *params,
                                     int coeff, int stokes, int negative_lobe, double s, double theta,
                                     size_t count, const double *d_n_lo, const double *d_n_hi, double *d_out, void *stream);

/* Unit seam for gsl::deriv_central (gsl.rs:233-257 -> gsl_deriv_central: 5-point central difference with one step-size
 * refinement) as n_integration drives it (symphony.rs:238-240): d_out[i] = the accepted derivative estimate of the
 * gamma-integral with respect to the harmonic number at d_n_start[i], step h = 1e-10 n_start, computed by the
 * derivative-probe phases of the coefficient's state machine (the code the product kernels run). */
int rimphony_deriv_probe_batch_device(rimphony_ctx *ctx, int dist_kind, const double *params,
                                      int coeff, int stokes, int negative_lobe, double s, double theta,
                                      size_t count, const double *d_n_start, double *d_out, void *stream);

/* Diagnostic seam: diagnostic_symphony_gamma_contribution (lib.rs:288-296 -> symphony.rs:491-567), the
 * contribution of all harmonics at fixed gamma (cgs-scaled like a coefficient), for one parameter point. */
int rimphony_gamma_contribution_batch_device(rimphony_ctx *ctx, int dist_kind, const double *params, int coeff, int stokes,
                                             double s, double theta, size_t count, const double *d_gamma, double *d_out,
                                             void *stream);

/* The DistributionFunction trait (lib.rs:111-146): calc_f(gamma, cos_xi) and calc_f_derivatives(gamma, cos_xi) of ONE
 * distribution (host `params`, kind-specific as above) over device arrays of count (gamma, cos_xi) pairs.  Any of
 * d_f, d_dfdg, d_dfdcx may be NULL.  norm_override: NaN = the distribution's own normalisation (what
 * full_calculation computes); any other value is used as the normalisation constant -- the reference's derivative
 * tests set it to 1 (pitchy_pl.rs:216-217, pitchy_kappa.rs:149-150). */
int rimphony_calc_f_batch_device(rimphony_ctx *ctx, int dist_kind, const double *params, double norm_override,
                                 size_t count, const double *d_gamma, const double *d_cos_xi,
                                 double *d_f, double *d_dfdg, double *d_dfdcx, void *stream);
/* the same with host buffers (synchronous) */
int rimphony_calc_f_batch(rimphony_ctx *ctx, int dist_kind, const double *params, double norm_override, size_t count,
                          const double *gamma, const double *cos_xi, double *f, double *dfdg, double *dfdcx);

/* Unit seams of the Heyvaerts (Faraday) path for ONE parameter point (host `params`), stokes = RIMPHONY_STOKES_Q (the
 * "h" elements, rho_Q) or _V (the "f" elements, rho_V):
 *   element: the inner integrand -- qr != 0: h_qr / f_qr_element at sigma = d_fixed[i], pomega = d_v[i]
 *            (heyvaerts.rs:302-373, 400-447); qr == 0: h_nr / f_nr_element at pomega = d_fixed[i], sigma = d_v[i]
 *            (heyvaerts.rs:379-394, 453-468);
 *   outer:   the outer integrand = one inner integral -- qr_outer_integrand(sigma = d_u[i]) / nr_outer_integrand(pomega =
 *            d_u[i]) (heyvaerts.rs:213-250, 262-296); NaN where the inner QAG fails. */
int rimphony_hey_element_batch_device(rimphony_ctx *ctx, int dist_kind, const double *params, int stokes, double s, double theta,
                                      int qr, size_t count, const double *d_fixed, const double *d_v, double *d_out, void *stream);
int rimphony_hey_outer_batch_device(rimphony_ctx *ctx, int dist_kind, const double *params, int stokes, double s, double theta,
                                    int qr, size_t count, const double *d_u, double *d_out, void *stream);

/* Self-test seam for the wavefront QAG (gsl.rs:156-207 semantics) on built-in
 * integrands made of + - * / sqrt only, so CPU and GPU agree bit for bit:
 *   family 0: 1 / (1 + ((x - p0) * p1)^2)         family 1: sqrt(|x - p0|) * p1
 *   family 2: x^2 * (p0 + x * p1)                  family 3: 1 / sqrt(|x - p0| + p1)
 *   family 4: p1 * |frac(x * p0) - 1/2|  (triangle wave: forces long subinterval lists)
 * Arrays of `count` problems; outputs result, abserr, status, size. */
int rimphony_qag_selftest_device(rimphony_ctx *ctx, size_t count, const int32_t *d_family,
                                 const double *d_p0, const double *d_p1, const double *d_a, const double *d_b,
                                 double epsabs, double epsrel, int32_t limit,
                                 double *d_result, double *d_abserr, int32_t *d_qstatus, int32_t *d_size,
                                 void *stream);

#ifdef __cplusplus
}
#endif
#endif
