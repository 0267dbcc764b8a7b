// rimphony.hpp -- C++ host-side mirror of rimphony's public API over the C ABI of
// include/rimphony_hip.h (header-only).  The reference's host language is Rust,
// which this image lacks; this header keeps the same names, argument meaning and
// error behaviour so a user of the crate finds what they expect:
//
//   enum Stokes / Coefficient                                   lib.rs:74-107
//   trait SynchrotronCalculator { compute_dimensionless, compute_cgs,
//       compute_all_dimensionless, compute_all_cgs }           lib.rs:150-210
//   PowerLawDistribution::new(p).gamma_limits(..).full_calculation(..)   power_law.rs:71-111
//   ThermalJuettnerDistribution::new(t).full_calculation(..)             thermal_juettner.rs:45-72
//   PitchyPowerLawDistribution::new(p,k).gamma_limits(..)...             pitchy_pl.rs:73-115
//   PitchyKappaDistribution::new(kappa,width,k).gamma_cutoff(..)...      pitchy_kappa.rs:70-125
//   TabulatedDistribution(gamma_lo, gamma_hi, log_n)                     the open trait of lib.rs:111-146, as a table
//   trait DistributionFunction { calc_f, calc_f_derivatives }            lib.rs:111-146
//
// plus the batched entry the GPU path exists for: BatchCalculator::compute().
// Numerical failure is NaN, never an exception (symphony.rs:115-117); API misuse
// and HIP errors throw std::runtime_error.  No CPU fallback.
#ifndef RIMPHONY_HPP
#define RIMPHONY_HPP

#include <array>
#include <cmath>
#include <cstdint>
#include <limits>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/rimphony_hip.h"

namespace rimphony {

constexpr double PI = 3.14159265358979323846;
constexpr double TWO_PI = 2. * PI;
constexpr double MASS_ELECTRON = 9.1093826e-28;
constexpr double SPEED_LIGHT = 2.99792458e10;
constexpr double ELECTRON_CHARGE = 4.80320680e-10;

enum class Stokes { I = 0, Q = 1, V = 2 };
enum class Coefficient { Emission = 0, Absorption = 1, Faraday = 2 };

enum class Precision { F64 = RIMPHONY_PRECISION_F64, F32Integrand = RIMPHONY_PRECISION_F32_INTEGRAND };

inline void check(int rc, const char *what)
{
    if (rc == RIMPHONY_OK) return;
    std::string msg = std::string(what) + ": " + rimphony_strerror(rc);
    // the HIP call that failed (thread-local text): only a RIMPHONY_EHIP return is described by it
    const char *detail = rc == RIMPHONY_EHIP ? rimphony_last_error() : nullptr;
    if (detail && *detail) msg += std::string(" -- ") + detail;
    throw std::runtime_error(msg);
}

class Context {
public:
    explicit Context(int device = 0) { check(rimphony_ctx_create(device, &ctx_), "rimphony_ctx_create"); }
    ~Context() { rimphony_ctx_destroy(ctx_); }
    Context(const Context &) = delete;
    Context &operator=(const Context &) = delete;
    rimphony_ctx *get() const { return ctx_; }
    // true when another context (this process or another) already owned the device at creation: the persistent grids are
    // then a quarter of the device and the cooperative tail is off (include/rimphony_hip.h, "context")
    bool shared_mode() const { return rimphony_ctx_shared_mode(ctx_) != 0; }
    // The context's table set for RIMPHONY_TABULATED (include/rimphony_hip.h): log_n = ln n(gamma), [n_tables][n_nodes]
    // row-major, at nodes uniform in ln gamma from gamma_lo to gamma_hi.  Replaces the previous set; n_tables = 0 clears it.
    void set_tables(size_t n_tables, size_t n_nodes, double gamma_lo, double gamma_hi, const std::vector<double> &log_n) const
    {
        if (log_n.size() != n_tables * n_nodes) throw std::runtime_error("set_tables: log_n must hold n_tables * n_nodes values");
        check(rimphony_ctx_set_tables(ctx_, n_tables, n_nodes, gamma_lo, gamma_hi, n_tables ? log_n.data() : nullptr),
              "rimphony_ctx_set_tables");
    }
    // The same with a pitch-angle factor per table: log_g = ln g(mu), [n_tables][n_mu] row-major, at nodes uniform in
    // mu = cos xi from -1 to +1 (rimphony_ctx_set_tables_pitch); an empty log_g with n_mu = 0 is the isotropic set.
    void set_tables(size_t n_tables, size_t n_nodes, double gamma_lo, double gamma_hi, const std::vector<double> &log_n,
                    size_t n_mu, const std::vector<double> &log_g) const
    {
        if (log_n.size() != n_tables * n_nodes) throw std::runtime_error("set_tables: log_n must hold n_tables * n_nodes values");
        if (log_g.size() != n_tables * n_mu) throw std::runtime_error("set_tables: log_g must hold n_tables * n_mu values");
        check(rimphony_ctx_set_tables_pitch(ctx_, n_tables, n_nodes, gamma_lo, gamma_hi, n_tables ? log_n.data() : nullptr, n_mu,
                                            log_g.empty() ? nullptr : log_g.data()),
              "rimphony_ctx_set_tables_pitch");
    }
    // The same with a sin^k xi prefactor per table: sin_k [n_tables], each in [0, 100] (rimphony_ctx_set_tables_pitchy);
    // log_g may be empty with n_mu = 0.  f = norm n sin^k xi g / (gamma^2 beta).
    void set_tables(size_t n_tables, size_t n_nodes, double gamma_lo, double gamma_hi, const std::vector<double> &log_n,
                    size_t n_mu, const std::vector<double> &log_g, const std::vector<double> &sin_k) const
    {
        if (log_n.size() != n_tables * n_nodes) throw std::runtime_error("set_tables: log_n must hold n_tables * n_nodes values");
        if (log_g.size() != n_tables * n_mu) throw std::runtime_error("set_tables: log_g must hold n_tables * n_mu values");
        if (sin_k.size() != n_tables) throw std::runtime_error("set_tables: sin_k must hold n_tables values");
        check(rimphony_ctx_set_tables_pitchy(ctx_, n_tables, n_nodes, gamma_lo, gamma_hi, n_tables ? log_n.data() : nullptr, n_mu,
                                             log_g.empty() ? nullptr : log_g.data(), n_tables ? sin_k.data() : nullptr),
              "rimphony_ctx_set_tables_pitchy");
    }
    // A FAMILY of energy tables (rimphony_ctx_set_tables_family): log_n [n_tables][n_nodes] as for set_tables, sin_k empty or
    // [n_tables].  The one parameter of a RIMPHONY_TABULATED row is then a real index x in [0, n_tables - 1]; every sample
    // blends tables floor(x) and floor(x) + 1 with the weight x - floor(x), and k likewise.
    void set_tables_family(size_t n_tables, size_t n_nodes, double gamma_lo, double gamma_hi, const std::vector<double> &log_n,
                           const std::vector<double> &sin_k = {}) const
    {
        if (log_n.size() != n_tables * n_nodes) throw std::runtime_error("set_tables_family: log_n must hold n_tables * n_nodes values");
        if (!sin_k.empty() && sin_k.size() != n_tables) throw std::runtime_error("set_tables_family: sin_k must hold n_tables values");
        check(rimphony_ctx_set_tables_family(ctx_, n_tables, n_nodes, gamma_lo, gamma_hi, n_tables ? log_n.data() : nullptr,
                                             sin_k.empty() ? nullptr : sin_k.data()),
              "rimphony_ctx_set_tables_family");
    }
    // A set on gamma nodes of the caller's choosing (rimphony_ctx_set_tables_grid): gamma [n_nodes] strictly increasing from
    // >= 1, shared by the tables; log_n [n_tables][n_nodes]; log_g [n_tables][n_mu] and sin_k [n_tables] may be empty.
    void set_tables_grid(size_t n_tables, const std::vector<double> &gamma, const std::vector<double> &log_n, size_t n_mu = 0,
                         const std::vector<double> &log_g = {}, const std::vector<double> &sin_k = {}) const
    {
        if (log_n.size() != n_tables * gamma.size()) throw std::runtime_error("set_tables_grid: log_n must hold n_tables * n_nodes values");
        if (log_g.size() != n_tables * n_mu) throw std::runtime_error("set_tables_grid: log_g must hold n_tables * n_mu values");
        if (!sin_k.empty() && sin_k.size() != n_tables) throw std::runtime_error("set_tables_grid: sin_k must hold n_tables values");
        check(rimphony_ctx_set_tables_grid(ctx_, n_tables, gamma.size(), n_tables ? gamma.data() : nullptr,
                                           n_tables ? log_n.data() : nullptr, n_mu, log_g.empty() ? nullptr : log_g.data(),
                                           sin_k.empty() ? nullptr : sin_k.data()),
              "rimphony_ctx_set_tables_grid");
    }
    // A 2-D set: log_n [n_tables][n_nodes][n_mu], mu fastest, = ln n(gamma, mu) at nodes uniform in ln gamma and in mu from -1
    // to +1 (rimphony_ctx_set_tables_2d): any f(gamma, cos xi), a non-separable one included.
    void set_tables_2d(size_t n_tables, size_t n_nodes, double gamma_lo, double gamma_hi, size_t n_mu,
                       const std::vector<double> &log_n) const
    {
        if (log_n.size() != n_tables * n_nodes * n_mu)
            throw std::runtime_error("set_tables_2d: log_n must hold n_tables * n_nodes * n_mu values");
        check(rimphony_ctx_set_tables_2d(ctx_, n_tables, n_nodes, gamma_lo, gamma_hi, n_mu, n_tables ? log_n.data() : nullptr),
              "rimphony_ctx_set_tables_2d");
    }
    // The same with a sin^k xi prefactor per table: sin_k [n_tables], each in [0, 100] (rimphony_ctx_set_tables_2d_pitchy);
    // f = norm sin^k xi exp(S) / (gamma^2 beta), log_n the smooth remainder ln(n / sin^k xi).
    void set_tables_2d(size_t n_tables, size_t n_nodes, double gamma_lo, double gamma_hi, size_t n_mu,
                       const std::vector<double> &log_n, const std::vector<double> &sin_k) const
    {
        if (log_n.size() != n_tables * n_nodes * n_mu)
            throw std::runtime_error("set_tables_2d: log_n must hold n_tables * n_nodes * n_mu values");
        if (sin_k.size() != n_tables) throw std::runtime_error("set_tables_2d: sin_k must hold n_tables values");
        check(rimphony_ctx_set_tables_2d_pitchy(ctx_, n_tables, n_nodes, gamma_lo, gamma_hi, n_mu, n_tables ? log_n.data() : nullptr,
                                                n_tables ? sin_k.data() : nullptr),
              "rimphony_ctx_set_tables_2d_pitchy");
    }
    // A 2-D set on gamma nodes of the caller's choosing (rimphony_ctx_set_tables_2d_grid): gamma [n_nodes] strictly increasing
    // from >= 1, shared by the tables; log_n [n_tables][n_nodes][n_mu], mu fastest, the mu nodes uniform from -1 to +1.
    void set_tables_2d_grid(size_t n_tables, const std::vector<double> &gamma, size_t n_mu, const std::vector<double> &log_n) const
    {
        if (log_n.size() != n_tables * gamma.size() * n_mu)
            throw std::runtime_error("set_tables_2d_grid: log_n must hold n_tables * n_nodes * n_mu values");
        check(rimphony_ctx_set_tables_2d_grid(ctx_, n_tables, gamma.size(), n_tables ? gamma.data() : nullptr, n_mu,
                                              n_tables ? log_n.data() : nullptr),
              "rimphony_ctx_set_tables_2d_grid");
    }
    // The same with a sin^k xi prefactor per table, sin_k [n_tables] (rimphony_ctx_set_tables_2d_grid_pitchy).
    void set_tables_2d_grid(size_t n_tables, const std::vector<double> &gamma, size_t n_mu, const std::vector<double> &log_n,
                            const std::vector<double> &sin_k) const
    {
        if (log_n.size() != n_tables * gamma.size() * n_mu)
            throw std::runtime_error("set_tables_2d_grid: log_n must hold n_tables * n_nodes * n_mu values");
        if (sin_k.size() != n_tables) throw std::runtime_error("set_tables_2d_grid: sin_k must hold n_tables values");
        check(rimphony_ctx_set_tables_2d_grid_pitchy(ctx_, n_tables, gamma.size(), n_tables ? gamma.data() : nullptr, n_mu,
                                                     n_tables ? log_n.data() : nullptr, n_tables ? sin_k.data() : nullptr),
              "rimphony_ctx_set_tables_2d_grid_pitchy");
    }
    // A 2-D set on gamma nodes and mu nodes of the caller's choosing (rimphony_ctx_set_tables_2d_nodes): gamma as for
    // set_tables_2d_grid; mu [n_mu] strictly increasing from exactly -1 to exactly +1, shared by the tables; log_n
    // [n_tables][n_nodes][n_mu], mu fastest; sin_k empty (the plain form) or [n_tables], each in [0, 100].
    void set_tables_2d_nodes(size_t n_tables, const std::vector<double> &gamma, const std::vector<double> &mu,
                             const std::vector<double> &log_n, const std::vector<double> &sin_k = {}) const
    {
        if (log_n.size() != n_tables * gamma.size() * mu.size())
            throw std::runtime_error("set_tables_2d_nodes: log_n must hold n_tables * n_nodes * n_mu values");
        if (!sin_k.empty() && sin_k.size() != n_tables)
            throw std::runtime_error("set_tables_2d_nodes: sin_k must be empty or hold n_tables values");
        check(rimphony_ctx_set_tables_2d_nodes(ctx_, n_tables, gamma.size(), n_tables ? gamma.data() : nullptr, mu.size(),
                                               n_tables ? mu.data() : nullptr, n_tables ? log_n.data() : nullptr,
                                               sin_k.empty() ? nullptr : sin_k.data()),
              "rimphony_ctx_set_tables_2d_nodes");
    }
    // A FAMILY of 2-D surfaces (rimphony_ctx_set_tables_2d_family): gamma, mu, log_n [n_tables][n_nodes][n_mu] and sin_k as for
    // set_tables_2d_nodes, the ends as for set_tables_2d_ends.  The one parameter of a RIMPHONY_TABULATED row is then a real
    // index x in [0, n_tables - 1]; every sample blends the node words of tables floor(x) and floor(x) + 1 with the weight
    // x - floor(x), and k likewise; the normalisation is integrated per row.
    void set_tables_2d_family(size_t n_tables, const std::vector<double> &gamma, const std::vector<double> &mu,
                              const std::vector<double> &log_n, const std::vector<double> &sin_k = {},
                              int ends_gamma = RIMPHONY_TAB_ENDS_NATURAL, int ends_mu = RIMPHONY_TAB_ENDS_NATURAL) const
    {
        if (log_n.size() != n_tables * gamma.size() * mu.size())
            throw std::runtime_error("set_tables_2d_family: log_n must hold n_tables * n_nodes * n_mu values");
        if (!sin_k.empty() && sin_k.size() != n_tables)
            throw std::runtime_error("set_tables_2d_family: sin_k must be empty or hold n_tables values");
        check(rimphony_ctx_set_tables_2d_family(ctx_, n_tables, gamma.size(), n_tables ? gamma.data() : nullptr, mu.size(),
                                                n_tables ? mu.data() : nullptr, n_tables ? log_n.data() : nullptr,
                                                sin_k.empty() ? nullptr : sin_k.data(), ends_gamma, ends_mu),
              "rimphony_ctx_set_tables_2d_family");
    }
    // The same family blended CUBICALLY across its tables (rimphony_ctx_set_tables_2d_family_cubic): at least four tables; param
    // empty (the knots are the indices) or one finite knot per table, strictly monotonic.  The parameter of a row stays the
    // real index; every sample blends the node words of four neighbouring tables with the row's Lagrange weights.
    void set_tables_2d_family_cubic(size_t n_tables, const std::vector<double> &gamma, const std::vector<double> &mu,
                                    const std::vector<double> &log_n, const std::vector<double> &sin_k = {},
                                    int ends_gamma = RIMPHONY_TAB_ENDS_NATURAL, int ends_mu = RIMPHONY_TAB_ENDS_NATURAL,
                                    const std::vector<double> &param = {}) const
    {
        if (log_n.size() != n_tables * gamma.size() * mu.size())
            throw std::runtime_error("set_tables_2d_family_cubic: log_n must hold n_tables * n_nodes * n_mu values");
        if (!sin_k.empty() && sin_k.size() != n_tables)
            throw std::runtime_error("set_tables_2d_family_cubic: sin_k must be empty or hold n_tables values");
        if (!param.empty() && param.size() != n_tables)
            throw std::runtime_error("set_tables_2d_family_cubic: param must be empty or hold n_tables values");
        check(rimphony_ctx_set_tables_2d_family_cubic(ctx_, n_tables, gamma.size(), n_tables ? gamma.data() : nullptr, mu.size(),
                                                      n_tables ? mu.data() : nullptr, n_tables ? log_n.data() : nullptr,
                                                      sin_k.empty() ? nullptr : sin_k.data(), ends_gamma, ends_mu,
                                                      param.empty() ? nullptr : param.data()),
              "rimphony_ctx_set_tables_2d_family_cubic");
    }
    // Any 2-D form from ln n in device memory (rimphony_ctx_set_tables_2d_device): d_log_n [n_tables][n_nodes][n_mu] on this
    // context's GPU, produced on `stream`.  gamma empty: n_nodes nodes uniform in ln gamma from gamma_lo to gamma_hi, else
    // gamma holds the nodes and the two are not read; mu empty: n_mu nodes uniform in mu, else mu holds them (mu without
    // gamma is refused); sin_k empty or [n_tables].  The set is the host entry's, word for word.  Synchronous.
    void set_tables_2d_device(size_t n_tables, size_t n_nodes, const std::vector<double> &gamma, double gamma_lo, double gamma_hi,
                              size_t n_mu, const std::vector<double> &mu, const double *d_log_n,
                              const std::vector<double> &sin_k = {}, void *stream = nullptr) const
    {
        if ((!gamma.empty() && gamma.size() != n_nodes) || (!mu.empty() && mu.size() != n_mu))
            throw std::runtime_error("set_tables_2d_device: gamma and mu must be empty or hold n_nodes and n_mu values");
        if (!sin_k.empty() && sin_k.size() != n_tables)
            throw std::runtime_error("set_tables_2d_device: sin_k must be empty or hold n_tables values");
        check(rimphony_ctx_set_tables_2d_device(ctx_, n_tables, n_nodes, gamma.empty() ? nullptr : gamma.data(), gamma_lo, gamma_hi,
                                                n_mu, mu.empty() ? nullptr : mu.data(), d_log_n,
                                                sin_k.empty() ? nullptr : sin_k.data(), stream),
              "rimphony_ctx_set_tables_2d_device");
    }
    // Any 2-D form from ln n in host memory with a choice of the spline's ends per axis (rimphony_ctx_set_tables_2d_ends):
    // ends_gamma and ends_mu are RIMPHONY_TAB_ENDS_NATURAL or RIMPHONY_TAB_ENDS_NOT_A_KNOT; gamma, mu and sin_k empty or given
    // as for set_tables_2d_device.  Natural ends on both axes install what the form's own set_tables_2d* installs; not-a-knot
    // ends along mu are for a surface curved at mu = +-1.
    void set_tables_2d_ends(size_t n_tables, size_t n_nodes, const std::vector<double> &gamma, double gamma_lo, double gamma_hi,
                            size_t n_mu, const std::vector<double> &mu, const std::vector<double> &log_n,
                            const std::vector<double> &sin_k, int ends_gamma, int ends_mu) const
    {
        if ((!gamma.empty() && gamma.size() != n_nodes) || (!mu.empty() && mu.size() != n_mu))
            throw std::runtime_error("set_tables_2d_ends: gamma and mu must be empty or hold n_nodes and n_mu values");
        if (log_n.size() != n_tables * n_nodes * n_mu)
            throw std::runtime_error("set_tables_2d_ends: log_n must hold n_tables * n_nodes * n_mu values");
        if (!sin_k.empty() && sin_k.size() != n_tables)
            throw std::runtime_error("set_tables_2d_ends: sin_k must be empty or hold n_tables values");
        check(rimphony_ctx_set_tables_2d_ends(ctx_, n_tables, n_nodes, gamma.empty() ? nullptr : gamma.data(), gamma_lo, gamma_hi, n_mu,
                                              mu.empty() ? nullptr : mu.data(), n_tables ? log_n.data() : nullptr,
                                              sin_k.empty() ? nullptr : sin_k.data(), ends_gamma, ends_mu),
              "rimphony_ctx_set_tables_2d_ends");
    }
    // The same from ln n in device memory, produced on `stream` (rimphony_ctx_set_tables_2d_device_ends): the set of
    // set_tables_2d_ends, word for word.
    void set_tables_2d_device_ends(size_t n_tables, size_t n_nodes, const std::vector<double> &gamma, double gamma_lo, double gamma_hi,
                                   size_t n_mu, const std::vector<double> &mu, const double *d_log_n, const std::vector<double> &sin_k,
                                   int ends_gamma, int ends_mu, void *stream = nullptr) const
    {
        if ((!gamma.empty() && gamma.size() != n_nodes) || (!mu.empty() && mu.size() != n_mu))
            throw std::runtime_error("set_tables_2d_device_ends: gamma and mu must be empty or hold n_nodes and n_mu values");
        if (!sin_k.empty() && sin_k.size() != n_tables)
            throw std::runtime_error("set_tables_2d_device_ends: sin_k must be empty or hold n_tables values");
        check(rimphony_ctx_set_tables_2d_device_ends(ctx_, n_tables, n_nodes, gamma.empty() ? nullptr : gamma.data(), gamma_lo, gamma_hi,
                                                     n_mu, mu.empty() ? nullptr : mu.data(), d_log_n,
                                                     sin_k.empty() ? nullptr : sin_k.data(), ends_gamma, ends_mu, stream),
              "rimphony_ctx_set_tables_2d_device_ends");
    }
    // the installed set as the kernels read it, copied to the host (rimphony_debug_tables); empty without a set
    std::vector<double> tables_blob() const
    {
        size_t n = 0;
        const int rc = rimphony_debug_tables(ctx_, nullptr, 0, &n);
        if (!n) { check(rc, "rimphony_debug_tables"); return {}; }
        std::vector<double> out(n);
        check(rimphony_debug_tables(ctx_, out.data(), out.size(), &n), "rimphony_debug_tables");
        return out;
    }
private:
    rimphony_ctx *ctx_ = nullptr;
};

// slot order of compute_all_dimensionless (lib.rs:176-177)
inline int slot_of(Coefficient c, Stokes s)
{
    if (c == Coefficient::Faraday) return s == Stokes::Q ? 6 : s == Stokes::V ? 7 : -1;
    return 2 * static_cast<int>(s) + static_cast<int>(c);
}

// N x (full_calculation + compute_all_dimensionless): host SoA arrays in, [n][8] out.
class BatchCalculator {
public:
    BatchCalculator(std::shared_ptr<Context> ctx, int dist_kind) : ctx_(std::move(ctx)), kind_(dist_kind)
    {
        if (rimphony_dist_nparams(kind_) < 0) throw std::runtime_error("unknown distribution kind");
    }
    // status: optional [n][8] RIMPHONY_ST_* words; work: optional [n][8] integrand samples spent per coefficient
    std::vector<double> compute(const std::vector<double> &s, const std::vector<double> &theta,
                                const std::vector<std::vector<double>> &params, uint32_t mask = RIMPHONY_SLOTS_ALL,
                                std::vector<int32_t> *status = nullptr, std::vector<uint64_t> *work = nullptr,
                                Precision precision = Precision::F64) const
    {
        const size_t n = s.size();
        const std::vector<const double *> pp = columns(kind_, n, theta, params);
        std::vector<double> out(n * 8, std::numeric_limits<double>::quiet_NaN());
        if (status) status->assign(n * 8, 0);
        if (work) work->assign(n * 8, 0);
        check(rimphony_batch_compute_ex(ctx_->get(), kind_, n, s.data(), theta.data(), pp.data(), mask,
                                        static_cast<int>(precision), out.data(), status ? status->data() : nullptr,
                                        work ? work->data() : nullptr), "rimphony_batch_compute_ex");
        return out;
    }
    // The same table from several devices: row i is evaluated by contexts[i mod N] (one host thread per context) and
    // lands in row i -- the table does not depend on N.
    static std::vector<double> compute_multi(const std::vector<std::shared_ptr<Context>> &contexts, int dist_kind,
                                             const std::vector<double> &s, const std::vector<double> &theta,
                                             const std::vector<std::vector<double>> &params,
                                             uint32_t mask = RIMPHONY_SLOTS_ALL, std::vector<int32_t> *status = nullptr,
                                             std::vector<uint64_t> *work = nullptr, Precision precision = Precision::F64)
    {
        const size_t n = s.size();
        const std::vector<const double *> pp = columns(dist_kind, n, theta, params);
        std::vector<rimphony_ctx *> raw;
        for (const auto &c : contexts) raw.push_back(c->get());
        std::vector<double> out(n * 8, std::numeric_limits<double>::quiet_NaN());
        if (status) status->assign(n * 8, 0);
        if (work) work->assign(n * 8, 0);
        check(rimphony_batch_compute_multi(raw.data(), static_cast<int>(raw.size()), dist_kind, n, s.data(), theta.data(),
                                           pp.data(), mask, static_cast<int>(precision), out.data(),
                                           status ? status->data() : nullptr, work ? work->data() : nullptr),
              "rimphony_batch_compute_multi");
        return out;
    }
private:
    static std::vector<const double *> columns(int kind, size_t n, const std::vector<double> &theta,
                                               const std::vector<std::vector<double>> &params)
    {
        if (rimphony_dist_nparams(kind) < 0) throw std::runtime_error("unknown distribution kind");
        if (theta.size() != n || static_cast<int>(params.size()) != rimphony_dist_nparams(kind))
            throw std::runtime_error("compute: array shapes do not match");
        std::vector<const double *> pp;
        for (const auto &p : params) {
            if (p.size() != n) throw std::runtime_error("compute: parameter array length");
            pp.push_back(p.data());
        }
        return pp;
    }
    std::shared_ptr<Context> ctx_;
    int kind_;
};

// trait SynchrotronCalculator for one parameter point (each call is a 1-point batch)
class FullSynchrotronCalculator {
public:
    FullSynchrotronCalculator(std::shared_ptr<Context> ctx, int kind, std::vector<double> params)
        : batch_(std::move(ctx), kind), params_(std::move(params)) {}

    double compute_dimensionless(Coefficient coeff, Stokes stokes, double s, double theta) const
    {
        const int k = slot_of(coeff, stokes);
        if (k < 0) return std::numeric_limits<double>::quiet_NaN();    // (Faraday, I): lib.rs:239-240
        return run(s, theta, 1u << k)[k];
    }
    double compute_cgs(Coefficient coeff, Stokes stokes, double nu, double b, double n_e, double theta) const
    {
        const double nu_c = ELECTRON_CHARGE * b / (TWO_PI * MASS_ELECTRON * SPEED_LIGHT);
        const double val = compute_dimensionless(coeff, stokes, nu / nu_c, theta);
        return coeff == Coefficient::Emission ? val * n_e * nu : val * n_e / nu;
    }
    std::array<double, 8> compute_all_dimensionless(double s, double theta) const
    {
        const auto v = run(s, theta, RIMPHONY_SLOTS_ALL);
        std::array<double, 8> rv;
        for (int k = 0; k < 8; k++) rv[k] = v[k];
        return rv;
    }
    std::array<double, 8> compute_all_cgs(double nu, double b, double n_e, double theta) const
    {
        const double nu_c = ELECTRON_CHARGE * b / (TWO_PI * MASS_ELECTRON * SPEED_LIGHT);
        auto rv = compute_all_dimensionless(nu / nu_c, theta);
        for (int k = 0; k < 8; k++) rv[k] = (k == 0 || k == 2 || k == 4) ? rv[k] * n_e * nu : rv[k] * n_e / nu;
        return rv;
    }
private:
    std::vector<double> run(double s, double theta, uint32_t mask) const
    {
        std::vector<std::vector<double>> pp;
        for (double p : params_) pp.push_back({p});
        return batch_.compute({s}, {theta}, pp, mask);
    }
    BatchCalculator batch_;
    std::vector<double> params_;
};

// `high_freq_approximation()` of the reference (power_law.rs:117-170, thermal_juettner.rs:78-142): the closed-form
// (Faraday, Q) and (Faraday, V); every other coefficient is NaN.
class HighFrequencyApproximation {
public:
    HighFrequencyApproximation(std::shared_ptr<Context> ctx, int kind, std::vector<double> params)
        : ctx_(std::move(ctx)), kind_(kind), params_(std::move(params)) {}
    double compute_dimensionless(Coefficient coeff, Stokes stokes, double s, double theta) const
    {
        if (coeff != Coefficient::Faraday || stokes == Stokes::I) return std::numeric_limits<double>::quiet_NaN();
        std::vector<const double *> pp;
        for (const double &p : params_) pp.push_back(&p);
        double out[2];
        check(rimphony_highfreq_batch(ctx_->get(), kind_, 1, &s, &theta, pp.data(), out), "rimphony_highfreq_batch");
        return stokes == Stokes::Q ? out[0] : out[1];
    }
private:
    std::shared_ptr<Context> ctx_;
    int kind_;
    std::vector<double> params_;
};

// The DistributionFunction trait (lib.rs:111-146): calc_f and calc_f_derivatives, evaluated by the HIP library.
// `norm` mirrors the public field of the reference's structs (its tests overwrite it, pitchy_pl.rs:216-217): NaN
// (the default) means "the normalisation full_calculation computes".
class DistributionFunction {
public:
    virtual ~DistributionFunction() = default;
    double norm = std::numeric_limits<double>::quiet_NaN();
    double calc_f(const Context &ctx, double gamma, double cos_xi) const
    {
        double f;
        const std::vector<double> p = abi_params();
        check(rimphony_calc_f_batch(ctx.get(), abi_kind(), p.data(), norm, 1, &gamma, &cos_xi, &f, nullptr, nullptr),
              "rimphony_calc_f_batch");
        return f;
    }
    std::array<double, 2> calc_f_derivatives(const Context &ctx, double gamma, double cos_xi) const
    {
        std::array<double, 2> d;
        const std::vector<double> p = abi_params();
        check(rimphony_calc_f_batch(ctx.get(), abi_kind(), p.data(), norm, 1, &gamma, &cos_xi, nullptr, &d[0], &d[1]),
              "rimphony_calc_f_batch");
        return d;
    }
protected:
    virtual int abi_kind() const = 0;
    virtual std::vector<double> abi_params() const = 0;
};

class PowerLawDistribution : public DistributionFunction {
protected:
    int abi_kind() const override { return RIMPHONY_POWER_LAW; }
    std::vector<double> abi_params() const override { return {p_, gmin_, gmax_, gcut_}; }
public:
    explicit PowerLawDistribution(double p) : p_(p) {}
    PowerLawDistribution &gamma_limits(double gmin, double gmax, double gcut) { gmin_ = gmin; gmax_ = gmax; gcut_ = gcut; return *this; }
    FullSynchrotronCalculator full_calculation(std::shared_ptr<Context> ctx) const
    { return FullSynchrotronCalculator(std::move(ctx), RIMPHONY_POWER_LAW, {p_, gmin_, gmax_, gcut_}); }
    HighFrequencyApproximation high_freq_approximation(std::shared_ptr<Context> ctx) const
    { return HighFrequencyApproximation(std::move(ctx), RIMPHONY_POWER_LAW, {p_, gmin_}); }
private:
    double p_, gmin_ = 1., gmax_ = 1e12, gcut_ = 1e10;     // defaults: power_law.rs:71-79
};

class ThermalJuettnerDistribution : public DistributionFunction {
protected:
    int abi_kind() const override { return RIMPHONY_THERMAL_JUETTNER; }
    std::vector<double> abi_params() const override { return {t_}; }
public:
    explicit ThermalJuettnerDistribution(double t) : t_(t) {}
    FullSynchrotronCalculator full_calculation(std::shared_ptr<Context> ctx) const
    { return FullSynchrotronCalculator(std::move(ctx), RIMPHONY_THERMAL_JUETTNER, {t_}); }
    HighFrequencyApproximation high_freq_approximation(std::shared_ptr<Context> ctx) const
    { return HighFrequencyApproximation(std::move(ctx), RIMPHONY_THERMAL_JUETTNER, {t_}); }
private:
    double t_;
};

class PitchyPowerLawDistribution : public DistributionFunction {
protected:
    int abi_kind() const override { return RIMPHONY_PITCHY_PL; }
    std::vector<double> abi_params() const override { return {p_, k_, gmin_, gmax_, gcut_}; }
public:
    PitchyPowerLawDistribution(double p, double k) : p_(p), k_(k) {}
    PitchyPowerLawDistribution &gamma_limits(double gmin, double gmax, double gcut) { gmin_ = gmin; gmax_ = gmax; gcut_ = gcut; return *this; }
    FullSynchrotronCalculator full_calculation(std::shared_ptr<Context> ctx) const
    { return FullSynchrotronCalculator(std::move(ctx), RIMPHONY_PITCHY_PL, {p_, k_, gmin_, gmax_, gcut_}); }
private:
    double p_, k_, gmin_ = 1., gmax_ = 1e12, gcut_ = 1e10;
};

class PitchyKappaDistribution : public DistributionFunction {
protected:
    int abi_kind() const override { return RIMPHONY_PITCHY_KAPPA; }
    std::vector<double> abi_params() const override { return {kappa_, width_, k_, gcut_}; }
public:
    PitchyKappaDistribution(double kappa, double width, double k) : kappa_(kappa), width_(width), k_(k) {}
    PitchyKappaDistribution &gamma_cutoff(double gcut) { gcut_ = gcut; return *this; }
    FullSynchrotronCalculator full_calculation(std::shared_ptr<Context> ctx) const
    { return FullSynchrotronCalculator(std::move(ctx), RIMPHONY_PITCHY_KAPPA, {kappa_, width_, k_, gcut_}); }
private:
    double kappa_, width_, k_, gcut_ = 1e10;
};

// A distribution given as a table of ln n(gamma) at nodes uniform in ln gamma (n = dN/dgamma up to a factor;
// the library interpolates with the natural cubic spline in (ln gamma, ln n); f = 0 outside the table, so let n roll off
// to a negligible value at both ends).  Isotropic, unless log_g = ln g(mu) at nodes uniform in mu = cos xi from -1 to +1
// gives it a pitch-angle factor: f = norm n g / (gamma^2 beta) (include/rimphony_hip.h).  A context holds ONE table set at a time: calc_f, calc_f_derivatives and
// full_calculation install this object's table in the context they are given, and the calculator computes with whatever
// set the context holds when it is used -- call install() again after another table has used the context.
class TabulatedDistribution : public DistributionFunction {
protected:
    int abi_kind() const override { return RIMPHONY_TABULATED; }
    std::vector<double> abi_params() const override { return {0.}; }      // the table index
public:
    TabulatedDistribution(double gamma_lo, double gamma_hi, std::vector<double> log_n)
        : glo_(gamma_lo), ghi_(gamma_hi), log_n_(std::move(log_n)) {}
    TabulatedDistribution(double gamma_lo, double gamma_hi, std::vector<double> log_n, std::vector<double> log_g)
        : glo_(gamma_lo), ghi_(gamma_hi), log_n_(std::move(log_n)), log_g_(std::move(log_g)) {}
    // ... times sin^k xi in closed form, 0 <= sin_k <= 100; log_g may be empty
    TabulatedDistribution(double gamma_lo, double gamma_hi, std::vector<double> log_n, std::vector<double> log_g, double sin_k)
        : glo_(gamma_lo), ghi_(gamma_hi), log_n_(std::move(log_n)), log_g_(std::move(log_g)), sin_k_{sin_k} {}
    void install(const Context &ctx) const
    {
        if (sin_k_.empty()) ctx.set_tables(1, log_n_.size(), glo_, ghi_, log_n_, log_g_.size(), log_g_);
        else ctx.set_tables(1, log_n_.size(), glo_, ghi_, log_n_, log_g_.size(), log_g_, sin_k_);
    }
    double calc_f(const Context &ctx, double gamma, double cos_xi) const
    { install(ctx); return DistributionFunction::calc_f(ctx, gamma, cos_xi); }
    std::array<double, 2> calc_f_derivatives(const Context &ctx, double gamma, double cos_xi) const
    { install(ctx); return DistributionFunction::calc_f_derivatives(ctx, gamma, cos_xi); }
    FullSynchrotronCalculator full_calculation(std::shared_ptr<Context> ctx) const
    {
        install(*ctx);
        return FullSynchrotronCalculator(std::move(ctx), RIMPHONY_TABULATED, {0.});
    }
private:
    double glo_, ghi_;
    std::vector<double> log_n_, log_g_, sin_k_;
};

// A family of tabulated distributions with a continuous parameter (include/rimphony_hip.h: rimphony_ctx_set_tables_family):
// log_n [n_tables][n_nodes] at nodes uniform in ln gamma, table i belonging to param[i] (strictly monotonic; empty: the index
// itself), sin_k empty or one exponent per table.  The library blends ln n and k linearly in the index, and index() is
// piecewise linear in param: exact where ln n is linear in param (a power law stored by p; a Juettner shape stored by 1 / T,
// so space param in 1 / T to be exact there).  at(value) is the member at that value, used as TabulatedDistribution is.
class TabulatedFamily {
public:
    class Member : public DistributionFunction {
    protected:
        int abi_kind() const override { return RIMPHONY_TABULATED; }
        std::vector<double> abi_params() const override { return {x_}; }      // the real index
    public:
        Member(const TabulatedFamily &family, double x) : family_(family), x_(x) {}
        double index() const { return x_; }
        void install(const Context &ctx) const { family_.install(ctx); }
        double calc_f(const Context &ctx, double gamma, double cos_xi) const
        { install(ctx); return DistributionFunction::calc_f(ctx, gamma, cos_xi); }
        std::array<double, 2> calc_f_derivatives(const Context &ctx, double gamma, double cos_xi) const
        { install(ctx); return DistributionFunction::calc_f_derivatives(ctx, gamma, cos_xi); }
        FullSynchrotronCalculator full_calculation(std::shared_ptr<Context> ctx) const
        {
            install(*ctx);
            return FullSynchrotronCalculator(std::move(ctx), RIMPHONY_TABULATED, {x_});
        }
    private:
        const TabulatedFamily &family_;
        double x_;
    };
    TabulatedFamily(double gamma_lo, double gamma_hi, size_t n_tables, std::vector<double> log_n, std::vector<double> sin_k = {},
                    std::vector<double> param = {})
        : glo_(gamma_lo), ghi_(gamma_hi), n_tables_(n_tables), log_n_(std::move(log_n)), sin_k_(std::move(sin_k)), param_(std::move(param))
    {
        if (n_tables_ == 0 || log_n_.size() % n_tables_ != 0) throw std::runtime_error("TabulatedFamily: log_n must hold n_tables rows");
        if (param_.empty()) for (size_t i = 0; i < n_tables_; i++) param_.push_back((double) i);
        if (param_.size() != n_tables_) throw std::runtime_error("TabulatedFamily: param must hold n_tables values");
        for (size_t i = 1; i + 1 < n_tables_; i++)
            if (!((param_[i] - param_[i - 1]) * (param_[i + 1] - param_[i]) > 0.)) throw std::runtime_error("TabulatedFamily: param must be strictly monotonic");
        if (n_tables_ == 2 && !(param_[0] != param_[1])) throw std::runtime_error("TabulatedFamily: param must be strictly monotonic");
    }
    void install(const Context &ctx) const { ctx.set_tables_family(n_tables_, log_n_.size() / n_tables_, glo_, ghi_, log_n_, sin_k_); }
    // the real index of a value: piecewise linear in param; throws outside it
    double index(double value) const
    {
        if (n_tables_ == 1) { if (value == param_[0]) return 0.; throw std::runtime_error("TabulatedFamily: value outside param"); }
        const bool up = param_[0] < param_[1];
        for (size_t i = 0; i + 1 < n_tables_; i++) {
            const double a = param_[i], b = param_[i + 1];
            if (up ? (value >= a && value <= b) : (value <= a && value >= b)) return (double) i + (value - a) / (b - a);
        }
        throw std::runtime_error("TabulatedFamily: value outside param");
    }
    Member at(double value) const { return Member(*this, index(value)); }
private:
    double glo_, ghi_;
    size_t n_tables_;
    std::vector<double> log_n_, sin_k_, param_;
};

// A family of tabulated SURFACES with a continuous parameter (include/rimphony_hip.h: rimphony_ctx_set_tables_2d_family): log_n
// [n_tables][n_nodes][n_mu], mu fastest, on the gamma and mu nodes of set_tables_2d_nodes, table i belonging to param[i]
// (strictly monotonic; empty: the index itself), sin_k empty or one exponent per table, the ends of the spline per axis.
// index() and at() as TabulatedFamily has them.  cubic: blend four neighbouring tables with a 4-point Lagrange cubic in param
// instead of two linearly (rimphony_ctx_set_tables_2d_family_cubic; at least four tables).
class TabulatedFamily2D {
public:
    class Member : public DistributionFunction {
    protected:
        int abi_kind() const override { return RIMPHONY_TABULATED; }
        std::vector<double> abi_params() const override { return {x_}; }      // the real index
    public:
        Member(const TabulatedFamily2D &family, double x) : family_(family), x_(x) {}
        double index() const { return x_; }
        void install(const Context &ctx) const { family_.install(ctx); }
        double calc_f(const Context &ctx, double gamma, double cos_xi) const
        { install(ctx); return DistributionFunction::calc_f(ctx, gamma, cos_xi); }
        std::array<double, 2> calc_f_derivatives(const Context &ctx, double gamma, double cos_xi) const
        { install(ctx); return DistributionFunction::calc_f_derivatives(ctx, gamma, cos_xi); }
        FullSynchrotronCalculator full_calculation(std::shared_ptr<Context> ctx) const
        {
            install(*ctx);
            return FullSynchrotronCalculator(std::move(ctx), RIMPHONY_TABULATED, {x_});
        }
    private:
        const TabulatedFamily2D &family_;
        double x_;
    };
    TabulatedFamily2D(std::vector<double> gamma, std::vector<double> mu, size_t n_tables, std::vector<double> log_n,
                      std::vector<double> sin_k = {}, std::vector<double> param = {}, int ends_gamma = RIMPHONY_TAB_ENDS_NATURAL,
                      int ends_mu = RIMPHONY_TAB_ENDS_NATURAL, bool cubic = false)
        : gamma_(std::move(gamma)), mu_(std::move(mu)), n_tables_(n_tables), log_n_(std::move(log_n)), sin_k_(std::move(sin_k)),
          param_(std::move(param)), ends_gamma_(ends_gamma), ends_mu_(ends_mu), cubic_(cubic)
    {
        if (cubic_ && n_tables_ < 4) throw std::runtime_error("TabulatedFamily2D: the cubic blend needs at least 4 tables");
        if (n_tables_ == 0 || log_n_.size() != n_tables_ * gamma_.size() * mu_.size())
            throw std::runtime_error("TabulatedFamily2D: log_n must hold n_tables * n_nodes * n_mu values");
        if (param_.empty()) for (size_t i = 0; i < n_tables_; i++) param_.push_back((double) i);
        if (param_.size() != n_tables_) throw std::runtime_error("TabulatedFamily2D: param must hold n_tables values");
        for (size_t i = 1; i + 1 < n_tables_; i++)
            if (!((param_[i] - param_[i - 1]) * (param_[i + 1] - param_[i]) > 0.)) throw std::runtime_error("TabulatedFamily2D: param must be strictly monotonic");
        if (n_tables_ == 2 && !(param_[0] != param_[1])) throw std::runtime_error("TabulatedFamily2D: param must be strictly monotonic");
    }
    void install(const Context &ctx) const
    {
        if (cubic_) ctx.set_tables_2d_family_cubic(n_tables_, gamma_, mu_, log_n_, sin_k_, ends_gamma_, ends_mu_, param_);
        else ctx.set_tables_2d_family(n_tables_, gamma_, mu_, log_n_, sin_k_, ends_gamma_, ends_mu_);
    }
    // the real index of a value: piecewise linear in param; throws outside it
    double index(double value) const
    {
        if (n_tables_ == 1) { if (value == param_[0]) return 0.; throw std::runtime_error("TabulatedFamily2D: value outside param"); }
        const bool up = param_[0] < param_[1];
        for (size_t i = 0; i + 1 < n_tables_; i++) {
            const double a = param_[i], b = param_[i + 1];
            if (up ? (value >= a && value <= b) : (value <= a && value >= b)) return (double) i + (value - a) / (b - a);
        }
        throw std::runtime_error("TabulatedFamily2D: value outside param");
    }
    Member at(double value) const { return Member(*this, index(value)); }
private:
    std::vector<double> gamma_, mu_;
    size_t n_tables_;
    std::vector<double> log_n_, sin_k_, param_;
    int ends_gamma_, ends_mu_;
    bool cubic_;
};

// A distribution given as a surface: log_n [n_nodes][n_mu], mu fastest, = ln n(gamma, mu) at nodes uniform in ln gamma and
// in mu = cos xi from -1 to +1; f = norm exp(S) / (gamma^2 beta) with S the tensor-product natural cubic spline, 0 outside
// the table (include/rimphony_hip.h: rimphony_ctx_set_tables_2d).  Used as TabulatedDistribution is.
class TabulatedDistribution2D : public DistributionFunction {
protected:
    int abi_kind() const override { return RIMPHONY_TABULATED; }
    std::vector<double> abi_params() const override { return {0.}; }      // the table index
public:
    TabulatedDistribution2D(double gamma_lo, double gamma_hi, size_t n_nodes, size_t n_mu, std::vector<double> log_n)
        : glo_(gamma_lo), ghi_(gamma_hi), n_nodes_(n_nodes), n_mu_(n_mu), log_n_(std::move(log_n)) {}
    // ... times sin^k xi in closed form, 0 <= sin_k <= 100: log_n is the smooth remainder ln(n / sin^k xi)
    TabulatedDistribution2D(double gamma_lo, double gamma_hi, size_t n_nodes, size_t n_mu, std::vector<double> log_n, double sin_k)
        : glo_(gamma_lo), ghi_(gamma_hi), n_nodes_(n_nodes), n_mu_(n_mu), log_n_(std::move(log_n)), sin_k_{sin_k} {}
    void install(const Context &ctx) const
    {
        if (sin_k_.empty()) ctx.set_tables_2d(1, n_nodes_, glo_, ghi_, n_mu_, log_n_);
        else ctx.set_tables_2d(1, n_nodes_, glo_, ghi_, n_mu_, log_n_, sin_k_);
    }
    double calc_f(const Context &ctx, double gamma, double cos_xi) const
    { install(ctx); return DistributionFunction::calc_f(ctx, gamma, cos_xi); }
    std::array<double, 2> calc_f_derivatives(const Context &ctx, double gamma, double cos_xi) const
    { install(ctx); return DistributionFunction::calc_f_derivatives(ctx, gamma, cos_xi); }
    FullSynchrotronCalculator full_calculation(std::shared_ptr<Context> ctx) const
    {
        install(*ctx);
        return FullSynchrotronCalculator(std::move(ctx), RIMPHONY_TABULATED, {0.});
    }
private:
    double glo_, ghi_;
    size_t n_nodes_, n_mu_;
    std::vector<double> log_n_, sin_k_;
};

// A distribution given as a surface on gamma nodes of its own: log_n [n_nodes][n_mu], mu fastest, = ln n(gamma_i, mu_j) at
// the strictly increasing gamma [n_nodes] and at mu nodes uniform from -1 to +1 (include/rimphony_hip.h:
// rimphony_ctx_set_tables_2d_grid): TabulatedDistribution2D on the nodes of TabulatedDistributionGrid.  Used as those are.
class TabulatedDistribution2DGrid : public DistributionFunction {
protected:
    int abi_kind() const override { return RIMPHONY_TABULATED; }
    std::vector<double> abi_params() const override { return {0.}; }      // the table index
public:
    TabulatedDistribution2DGrid(std::vector<double> gamma, size_t n_mu, std::vector<double> log_n)
        : gamma_(std::move(gamma)), n_mu_(n_mu), log_n_(std::move(log_n)) {}
    // ... times sin^k xi in closed form, as TabulatedDistribution2D takes it
    TabulatedDistribution2DGrid(std::vector<double> gamma, size_t n_mu, std::vector<double> log_n, double sin_k)
        : gamma_(std::move(gamma)), n_mu_(n_mu), log_n_(std::move(log_n)), sin_k_{sin_k} {}
    void install(const Context &ctx) const
    {
        if (sin_k_.empty()) ctx.set_tables_2d_grid(1, gamma_, n_mu_, log_n_);
        else ctx.set_tables_2d_grid(1, gamma_, n_mu_, log_n_, sin_k_);
    }
    double calc_f(const Context &ctx, double gamma, double cos_xi) const
    { install(ctx); return DistributionFunction::calc_f(ctx, gamma, cos_xi); }
    std::array<double, 2> calc_f_derivatives(const Context &ctx, double gamma, double cos_xi) const
    { install(ctx); return DistributionFunction::calc_f_derivatives(ctx, gamma, cos_xi); }
    FullSynchrotronCalculator full_calculation(std::shared_ptr<Context> ctx) const
    {
        install(*ctx);
        return FullSynchrotronCalculator(std::move(ctx), RIMPHONY_TABULATED, {0.});
    }
private:
    std::vector<double> gamma_;
    size_t n_mu_;
    std::vector<double> log_n_, sin_k_;
};

// A distribution given as a surface on gamma nodes and mu nodes of its own: log_n [n_nodes][n_mu], mu fastest, = ln n(gamma_i,
// mu_j) at the strictly increasing gamma [n_nodes] and mu [n_mu], mu from exactly -1 to exactly +1 (include/rimphony_hip.h:
// rimphony_ctx_set_tables_2d_nodes): TabulatedDistribution2DGrid on mu nodes graded towards a beam, a ring or the edge of a
// loss cone, or uniform in xi.  Used as that one is.
class TabulatedDistribution2DNodes : public DistributionFunction {
protected:
    int abi_kind() const override { return RIMPHONY_TABULATED; }
    std::vector<double> abi_params() const override { return {0.}; }      // the table index
public:
    TabulatedDistribution2DNodes(std::vector<double> gamma, std::vector<double> mu, std::vector<double> log_n)
        : gamma_(std::move(gamma)), mu_(std::move(mu)), log_n_(std::move(log_n)) {}
    // ... times sin^k xi in closed form, as TabulatedDistribution2D takes it
    TabulatedDistribution2DNodes(std::vector<double> gamma, std::vector<double> mu, std::vector<double> log_n, double sin_k)
        : gamma_(std::move(gamma)), mu_(std::move(mu)), log_n_(std::move(log_n)), sin_k_{sin_k} {}
    void install(const Context &ctx) const { ctx.set_tables_2d_nodes(1, gamma_, mu_, log_n_, sin_k_); }
    double calc_f(const Context &ctx, double gamma, double cos_xi) const
    { install(ctx); return DistributionFunction::calc_f(ctx, gamma, cos_xi); }
    std::array<double, 2> calc_f_derivatives(const Context &ctx, double gamma, double cos_xi) const
    { install(ctx); return DistributionFunction::calc_f_derivatives(ctx, gamma, cos_xi); }
    FullSynchrotronCalculator full_calculation(std::shared_ptr<Context> ctx) const
    {
        install(*ctx);
        return FullSynchrotronCalculator(std::move(ctx), RIMPHONY_TABULATED, {0.});
    }
private:
    std::vector<double> gamma_, mu_, log_n_, sin_k_;
};

// A distribution given as a table on gamma nodes of its own: log_n [n_nodes] = ln n at the strictly increasing gamma
// [n_nodes] (include/rimphony_hip.h: rimphony_ctx_set_tables_grid), for what nodes uniform in ln gamma cannot resolve.
// log_g (ln g at nodes uniform in mu) may be empty; sin_k < 0: no prefactor.  Used as TabulatedDistribution is.
class TabulatedDistributionGrid : public DistributionFunction {
protected:
    int abi_kind() const override { return RIMPHONY_TABULATED; }
    std::vector<double> abi_params() const override { return {0.}; }      // the table index
public:
    TabulatedDistributionGrid(std::vector<double> gamma, std::vector<double> log_n, std::vector<double> log_g = {}, double sin_k = -1.)
        : gamma_(std::move(gamma)), log_n_(std::move(log_n)), log_g_(std::move(log_g))
    { if (sin_k >= 0.) sin_k_.push_back(sin_k); }
    void install(const Context &ctx) const { ctx.set_tables_grid(1, gamma_, log_n_, log_g_.size(), log_g_, sin_k_); }
    double calc_f(const Context &ctx, double gamma, double cos_xi) const
    { install(ctx); return DistributionFunction::calc_f(ctx, gamma, cos_xi); }
    std::array<double, 2> calc_f_derivatives(const Context &ctx, double gamma, double cos_xi) const
    { install(ctx); return DistributionFunction::calc_f_derivatives(ctx, gamma, cos_xi); }
    FullSynchrotronCalculator full_calculation(std::shared_ptr<Context> ctx) const
    {
        install(*ctx);
        return FullSynchrotronCalculator(std::move(ctx), RIMPHONY_TABULATED, {0.});
    }
private:
    std::vector<double> gamma_, log_n_, log_g_, sin_k_;
};

}  // namespace rimphony
#endif
