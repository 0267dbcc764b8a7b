// tab_spline.h -- host side of the tabulated distribution: checks a table set and lays it out as the kernels read it
// (dev_symphony.h, TAB_HDR_*): a header, then per table and node the value y_j = ln n(gamma_j) and the slope m_j = dy/du
// of the natural cubic spline through the nodes, which are uniform in u = ln gamma.  The slopes are solved here once, in
// fp64: m_{j-1} + 4 m_j + m_{j+1} = 3 (y_{j+1} - y_{j-1}) / h inside, 2 m_0 + m_1 = 3 (y_1 - y_0) / h and its mirror at the
// ends (second derivative 0 there).  A straight line in (u, y) -- a pure power law -- comes back as itself.
//
// A set may carry a pitch-angle factor g(mu), mu = cos xi, per table (rim_tab_check_pitch, rim_tab_build_pitch): G = ln g
// at n_mu nodes uniform in mu from -1 to +1, the same natural spline in (mu, G) -- a straight line, an exponential beam,
// comes back as itself -- and P = 1/2 int g dmu of the spline, which the normalisation divides by.  The pitch rows follow
// the gamma rows; an isotropic set is laid out as it always was.
//
// A set may instead be two-dimensional (rim_tab_check_2d, rim_tab_build_2d): ln n(gamma, mu) on a grid uniform in u and in
// mu, interpolated by the tensor-product natural cubic spline S(u, mu).  Per node the four words {S, S_u, S_mu, S_umu} of
// the bicubic Hermite form, all from the same Thomas sweep; a surface bilinear in (u, mu) comes back as itself, a sum
// H(u) + G(mu) as the two 1-D splines.  The normalisation of a 2-D table is a word of its header, which the caller fills
// (the library on the device, the tests' oracle with its own QAG): 0 as built.
//
// A set may carry a sin^k xi prefactor per table, with or without g (rim_tab_check_pitchy, rim_tab_build_pitchy): the
// layout of dev_symphony.h's TAB_PITCHY_*.  Without g, P = 1/2 int (1 - mu^2)^(k/2) dmu is the closed form of the pitchy
// kinds, set here; with g it is 0 as built and the caller fills it (the library on the device, the tests' oracle with its
// own QAG), as the normalisation of a 2-D table.
//
// A set may stand on gamma nodes of its own choosing (rim_tab_check_grid, rim_tab_build_grid): strictly increasing, shared
// by the tables of the set, with everything a sin^k set carries.  The natural cubic spline through (u_j, y_j), u_j =
// rim_log(gamma_j), from the Thomas sweep on the non-uniform system; the layout of dev_symphony.h's tab_grid_*, with the
// guide that tells a sample where to look for its interval.
//
// A 2-D set may stand on given gamma nodes too (rim_tab_check_2d_grid, rim_tab_build_2d_grid): the same four words per node,
// the sweeps along u on the non-uniform system, the guide of a set on given nodes and one array of u nodes per set
// (dev_symphony.h: tab_2d_grid_*).
//
// A 2-D set of either form may carry a sin^k xi prefactor per table (rim_tab_check_2d_pitchy, rim_tab_build_2d_pitchy and
// their _grid_ counterparts): the form's blob with k in a spare word of each table's header (TAB_2D_K).
//
// A 2-D set may stand on mu nodes of the caller's choosing as well (rim_tab_check_2d_nodes, rim_tab_build_2d_nodes): the 2-D
// set on given gamma nodes with the sweeps along mu on the non-uniform system too, a mu guide and one array of mu nodes per
// set (dev_symphony.h: tab_2d_nodes_*), with or without a sin^k xi prefactor.
//
// The three 2-D builders begin with the FRONT of their set -- header, table headers, guides, node words: everything that does
// not depend on log_n (rim_tab_front_2d, rim_tab_front_2d_grid, rim_tab_front_2d_nodes) -- and the three 2-D checks with a
// geometry-only part (rim_tab_check_2d_geometry and its _grid_ and _nodes_ counterparts).  A set whose log_n lies in device
// memory uses those parts alone and solves the node data on the device, to the same bits (tab_install.h).
//
// The ends of the spline of a 2-D set are a choice per axis (RIM_TAB_ENDS_NATURAL, RIM_TAB_ENDS_NOT_A_KNOT: the trailing
// arguments of both line solvers and of the 2-D builders, natural where they are left out).  Natural ends force a second
// derivative of 0 at the end nodes; not-a-knot ends make the third derivative continuous across the second and the
// second-to-last node, so that every cubic comes back as itself and the error stays O(h^4) up to the edge.  The choice is a
// word of each table's header (TAB_2D_ENDS = ends_u + 2 ends_mu) that no kernel reads: the kernels see {S, S_u, S_mu, S_umu}
// and never ask how they were solved.
//
// A set of energy tables on nodes uniform in ln gamma may be a FAMILY (rim_tab_check_family, rim_tab_build_family): a row of a
// batch names a real index x and its samples blend the node words of tables floor(x) and floor(x) + 1.  The rows of an
// isotropic set with the last one repeated, and the headers of a sin^k set without g where the family has a prefactor.
//
// A 2-D set on given gamma and mu nodes may be a family too (rim_tab_check_2d_family, rim_tab_build_2d_family): the set of
// rim_tab_build_2d_nodes with every table's normalisation word a NaN -- a row's samples blend the node words of two tables and
// its normalisation is integrated per row.
//
// Plain C++ with the elementary functions of detmath.h, so that the library (hipcc's host pass) and the tests' table
// oracle (g++) produce the same bits from the same table.
#ifndef RIM_TAB_SPLINE_H
#define RIM_TAB_SPLINE_H

#include <cstddef>
#include <vector>
#include "dev_symphony.h"
#include "gk31_table.h"

#define RIM_TAB_MIN_NODES 8
#define RIM_TAB_MAX_NODES 65536

// the checks say 0, or -1 for bad geometry or a non-finite value.  The range of a set: finite, 1 <= gamma_lo < gamma_hi
inline int rim_tab_check_range(double gamma_lo, double gamma_hi)
{
    return (!rim_isfinite(gamma_lo) || !rim_isfinite(gamma_hi) || !(gamma_lo >= 1.) || !(gamma_lo < gamma_hi)) ? -1 : 0;
}

inline int rim_tab_check(size_t n_tables, size_t n_nodes, double gamma_lo, double gamma_hi, const double *log_n)
{
    if (n_tables < 1 || n_nodes < RIM_TAB_MIN_NODES || n_nodes > RIM_TAB_MAX_NODES || !log_n) return -1;
    if (n_tables > ((size_t) 1 << 40) / n_nodes) return -1;
    if (rim_tab_check_range(gamma_lo, gamma_hi)) return -1;
    for (size_t i = 0; i < n_tables * n_nodes; i++)
        if (!rim_isfinite(log_n[i])) return -1;
    return 0;
}

#define RIM_TAB_ENDS_NATURAL 0
#define RIM_TAB_ENDS_NOT_A_KNOT 1

// an end condition per axis of a 2-D set: each RIM_TAB_ENDS_NATURAL or RIM_TAB_ENDS_NOT_A_KNOT
inline int rim_tab_check_ends(int ends_u, int ends_mu)
{
    return ((ends_u != RIM_TAB_ENDS_NATURAL && ends_u != RIM_TAB_ENDS_NOT_A_KNOT) ||
            (ends_mu != RIM_TAB_ENDS_NATURAL && ends_mu != RIM_TAB_ENDS_NOT_A_KNOT)) ? -1 : 0;
}

// The slopes of the natural cubic spline through y[0 .. n-1] at nodes h apart, written with the values as {y_j, m_j} pairs
// to row[2 j], row[2 j + 1].  cp, dp: n doubles each, the swept upper diagonal and right-hand side of the Thomas algorithm.
// ends = RIM_TAB_ENDS_NOT_A_KNOT: the first row is m_0 + 2 m_1 = (5 s_0 + s_1) / 2, s_j = (y_{j+1} - y_j) / h -- the third
// derivatives 6 (m_j + m_{j+1} - 2 s_j) / h^2 of the first two pieces set equal, m_2 eliminated with the row of node 1 -- and
// the last row its mirror, 2 m_{n-2} + m_{n-1} = (5 s_{n-2} + s_{n-3}) / 2.  The sweep needs no pivoting: its denominators are
// 2 at node 1, 3.5 .. 3.74 inside and 1 - 2 cp > 0.46 in the last row.
inline void rim_tab_spline_row(const double *y, size_t n, double h, double *row, double *cp, double *dp, int ends = RIM_TAB_ENDS_NATURAL)
{
    const size_t last = n - 1;
    if (ends) {
        cp[0] = 2.;
        dp[0] = (5. * ((y[1] - y[0]) / h) + (y[2] - y[1]) / h) / 2.;
    } else {
        cp[0] = 0.5;
        dp[0] = 3. * (y[1] - y[0]) / h / 2.;
    }
    for (size_t j = 1; j <= last; j++) {
        if (ends && j == last) {
            const double rhs = (5. * ((y[last] - y[last - 1]) / h) + (y[last - 1] - y[last - 2]) / h) / 2.;
            const double den = 1. - 2. * cp[j - 1];
            cp[j] = 1. / den;
            dp[j] = (rhs - 2. * dp[j - 1]) / den;
            break;
        }
        const double diag = j < last ? 4. : 2.;
        const double rhs = j < last ? 3. * (y[j + 1] - y[j - 1]) / h : 3. * (y[last] - y[last - 1]) / h;
        const double den = diag - cp[j - 1];
        cp[j] = 1. / den;
        dp[j] = (rhs - dp[j - 1]) / den;
    }
    row[2 * last + 1] = dp[last];
    for (size_t j = last; j-- > 0;) row[2 * j + 1] = dp[j] - cp[j] * row[2 * (j + 1) + 1];
    for (size_t j = 0; j <= last; j++) row[2 * j] = y[j];
}

// the eight words every set begins with (dev_symphony.h, TAB_HDR_*)
inline void rim_tab_set_header(double *hdr, size_t n_tables, size_t n_nodes, double gamma_lo, double gamma_hi, double u_lo,
                               double inv_h, double h, double n_mu)
{
    using namespace rim;
    hdr[TAB_HDR_NTABLES] = (double) n_tables;
    hdr[TAB_HDR_NNODES] = (double) n_nodes;
    hdr[TAB_HDR_GLO] = gamma_lo;
    hdr[TAB_HDR_GHI] = gamma_hi;
    hdr[TAB_HDR_ULO] = u_lo;
    hdr[TAB_HDR_INVH] = inv_h;
    hdr[TAB_HDR_H] = h;
    hdr[TAB_HDR_NMU] = n_mu;
}

// the table set as one block of doubles; rim_tab_check() has passed
inline void rim_tab_build(size_t n_tables, size_t n_nodes, double gamma_lo, double gamma_hi, const double *log_n,
                          std::vector<double> &blob)
{
    using namespace rim;
    const double u_lo = rim_log(gamma_lo), u_hi = rim_log(gamma_hi);
    const double h = (u_hi - u_lo) / (double) (n_nodes - 1);
    blob.assign((size_t) TAB_HDR_DOUBLES + n_tables * n_nodes * 2, 0.);
    rim_tab_set_header(blob.data(), n_tables, n_nodes, gamma_lo, gamma_hi, u_lo, 1. / h, h, 0.);
    std::vector<double> cp(n_nodes), dp(n_nodes);
    for (size_t t = 0; t < n_tables; t++)
        rim_tab_spline_row(log_n + t * n_nodes, n_nodes, h, blob.data() + TAB_HDR_DOUBLES + t * n_nodes * 2, cp.data(), dp.data());
}

// rim_tab_check() for a set with an optional pitch-angle factor: log_g [n_tables][n_mu] = ln g at nodes uniform in mu, or
// null with n_mu = 0 for an isotropic set
inline int rim_tab_check_pitch(size_t n_tables, size_t n_nodes, double gamma_lo, double gamma_hi, const double *log_n,
                               size_t n_mu, const double *log_g)
{
    if (rim_tab_check(n_tables, n_nodes, gamma_lo, gamma_hi, log_n)) return -1;
    if (!log_g && n_mu == 0) return 0;
    if (!log_g || n_mu < RIM_TAB_MIN_NODES || n_mu > RIM_TAB_MAX_NODES) return -1;
    if (n_tables > ((size_t) 1 << 40) / n_mu) return -1;
    for (size_t i = 0; i < n_tables * n_mu; i++)
        if (!rim_isfinite(log_g[i])) return -1;
    return 0;
}

// rim_tab_build() for such a set; rim_tab_check_pitch() has passed.  Without log_g the blob is rim_tab_build()'s.
inline void rim_tab_build_pitch(size_t n_tables, size_t n_nodes, double gamma_lo, double gamma_hi, const double *log_n,
                                size_t n_mu, const double *log_g, std::vector<double> &blob)
{
    using namespace rim;
    rim_tab_build(n_tables, n_nodes, gamma_lo, gamma_hi, log_n, blob);
    if (!log_g) return;
    static const double xgk[32] = RIM_GK31_X, wgk[32] = RIM_GK31_WK;
    const size_t base = blob.size(), stride = (size_t) TAB_PITCH_HDR + n_mu * 2;
    blob.resize(base + n_tables * stride, 0.);
    blob[TAB_HDR_NMU] = (double) n_mu;
    const double h = 2. / (double) (n_mu - 1);
    std::vector<double> cp(n_mu), dp(n_mu);
    for (size_t t = 0; t < n_tables; t++) {
        double *ph = blob.data() + base + t * stride;
        ph[TAB_PITCH_LAST] = (double) (n_mu - 2);
        ph[TAB_PITCH_INVH] = 1. / h;
        ph[TAB_PITCH_H] = h;
        rim_tab_spline_row(log_g + t * n_mu, n_mu, h, ph + TAB_PITCH_HDR, cp.data(), dp.data());
        // P = 1/2 int g dmu of the spline as the kernels evaluate it: the 31-point Kronrod rule on each node interval,
        // summed in node order
        DistParams d;
        d.par[0] = rim_frombits((uint64_t) (uintptr_t) ph);
        double sum = 0.;
        for (size_t j = 0; j + 1 < n_mu; j++) {
            const double half = 0.5 * h, centre = -1. + ((double) j + 0.5) * h;
            double acc = 0.;
            for (int k = 0; k < 31; k++) {
                double gval, dgdmu;
                tab_pitch_spline(d, centre + half * xgk[k], gval, dgdmu);
                acc += wgk[k] * rim_exp(gval);
            }
            sum += half * acc;
        }
        ph[TAB_PITCH_P] = 0.5 * sum;
    }
}

#define RIM_TAB_MAX_SIN_K 100.

// sin_k [n_tables]: every k finite and in [0, RIM_TAB_MAX_SIN_K]
inline int rim_tab_check_sin_k(size_t n_tables, const double *sin_k)
{
    for (size_t t = 0; t < n_tables; t++)
        if (!rim_isfinite(sin_k[t]) || !(sin_k[t] >= 0.) || !(sin_k[t] <= RIM_TAB_MAX_SIN_K)) return -1;
    return 0;
}

// rim_tab_check_pitch() for a set with a sin^k xi prefactor, sin_k as above
inline int rim_tab_check_pitchy(size_t n_tables, size_t n_nodes, double gamma_lo, double gamma_hi, const double *log_n,
                                size_t n_mu, const double *log_g, const double *sin_k)
{
    if (rim_tab_check_pitch(n_tables, n_nodes, gamma_lo, gamma_hi, log_n, n_mu, log_g) || !sin_k) return -1;
    return rim_tab_check_sin_k(n_tables, sin_k);
}

// 1/2 int (1 - mu^2)^(k/2) dmu = Gamma(3/2) Gamma(1 + k/2) / Gamma(3/2 + k/2): hyperg_2F1_at_1(0.5, -0.5 k, 1.5) of
// coop_kernel.h (pitchy_pl.rs:98), the same operations in the same order, here for the host
inline double rim_tab_sin_k_integral(double k)
{
    using namespace rim;
    const double a = 0.5, b = -0.5 * k, c = 1.5;
    const double lc = rim_lgamma_pos(c);
    const double lcab = rim_lgamma_pos(c - a - b);
    const double lca = rim_lgamma_pos(c - a);
    const double lcb = rim_lgamma_pos(c - b);
    return rim_exp(lc + lcab - lca - lcb);
}

// Table t of the sin^k tables that start at `tables` (dev_symphony.h: TAB_PITCHY_*): its k and, for n_mu > 0, its pitch
// row from log_g at nodes hm apart (P is 0 as built), else the closed form of P.  cp, dp: n_mu doubles.
inline void rim_tab_build_pitchy_table(double *tables, size_t t, double k, size_t n_mu, const double *log_g, double hm,
                                       double *cp, double *dp)
{
    using namespace rim;
    double *ph = tables + t * ((size_t) TAB_PITCHY_PRE + TAB_PITCH_HDR + n_mu * 2) + TAB_PITCHY_PRE;
    ph[TAB_PITCHY_K] = k;
    ph[TAB_PITCHY_NMU] = (double) n_mu;
    if (!n_mu) {
        ph[TAB_PITCH_P] = rim_tab_sin_k_integral(k);
        return;
    }
    ph[TAB_PITCH_LAST] = (double) (n_mu - 2);
    ph[TAB_PITCH_INVH] = 1. / hm;
    ph[TAB_PITCH_H] = hm;
    rim_tab_spline_row(log_g + t * n_mu, n_mu, hm, ph + TAB_PITCH_HDR, cp, dp);
}

// the set with a sin^k prefactor as one block of doubles (dev_symphony.h: TAB_PITCHY_*); rim_tab_check_pitchy() has passed
inline void rim_tab_build_pitchy(size_t n_tables, size_t n_nodes, double gamma_lo, double gamma_hi, const double *log_n,
                                 size_t n_mu, const double *log_g, const double *sin_k, std::vector<double> &blob)
{
    using namespace rim;
    rim_tab_build(n_tables, n_nodes, gamma_lo, gamma_hi, log_n, blob);
    if (!log_g) n_mu = 0;
    const size_t base = blob.size();
    blob.resize(base + n_tables * ((size_t) TAB_PITCHY_PRE + TAB_PITCH_HDR + n_mu * 2), 0.);
    blob[TAB_HDR_NMU] = (double) n_mu;
    const double h = n_mu ? 2. / (double) (n_mu - 1) : 0.;
    std::vector<double> cp(n_mu), dp(n_mu);
    for (size_t t = 0; t < n_tables; t++)
        rim_tab_build_pitchy_table(blob.data() + base, t, sin_k[t], n_mu, log_g, h, cp.data(), dp.data());
}

// the nodes of a set on given nodes: gamma [n_nodes], finite, 1 <= gamma[0], strictly increasing, and so are their
// logarithms as the build forms them (two gamma a rounding apart may share one: h_j = 0)
inline int rim_tab_check_gamma_nodes(size_t n_nodes, const double *gamma)
{
    using namespace rim;
    if (!gamma || n_nodes < RIM_TAB_MIN_NODES || n_nodes > RIM_TAB_MAX_NODES) return -1;
    for (size_t j = 0; j < n_nodes; j++)
        if (!rim_isfinite(gamma[j])) return -1;
    if (!(gamma[0] >= 1.)) return -1;
    for (size_t j = 0; j + 1 < n_nodes; j++) {
        if (!(gamma[j] < gamma[j + 1])) return -1;
        if (!(rim_log(gamma[j]) < rim_log(gamma[j + 1]))) return -1;
    }
    return 0;
}

// rim_tab_check_pitchy() for a set on given nodes.  log_g, n_mu as for rim_tab_check_pitch; sin_k may be null (no prefactor).
inline int rim_tab_check_grid(size_t n_tables, size_t n_nodes, const double *gamma, const double *log_n, size_t n_mu,
                              const double *log_g, const double *sin_k)
{
    if (rim_tab_check_gamma_nodes(n_nodes, gamma)) return -1;
    if (rim_tab_check_pitch(n_tables, n_nodes, gamma[0], gamma[n_nodes - 1], log_n, n_mu, log_g)) return -1;
    return sin_k ? rim_tab_check_sin_k(n_tables, sin_k) : 0;
}

// The slopes m[0 .. n-1] of the natural cubic spline through (u_j, y[j]) on nodes h[j] = u_{j+1} - u_j apart, ih[j] = 1 / h[j]:
//   ih[j-1] m_{j-1} + 2 (ih[j-1] + ih[j]) m_j + ih[j] m_{j+1} = 3 (s_{j-1} ih[j-1] + s_j ih[j]),  s_j = (y_{j+1} - y_j) / h[j],
// 2 m_0 + m_1 = 3 s_0 and its mirror at the ends.  One fixed order of operations: the bits depend on it.  cp, dp: n doubles.
// ends = RIM_TAB_ENDS_NOT_A_KNOT: (m_0 + m_1 - 2 s_0) / h_0^2 = (m_1 + m_2 - 2 s_1) / h_1^2, with m_2 eliminated by the row of
// node 1, is the first row of de Boor's CUBSPL,
//   h_1 m_0 + (h_0 + h_1) m_1 = ((3 h_0 + 2 h_1) h_1 s_0 + h_0^2 s_1) / (h_0 + h_1),
// and the last row is its mirror.  No pivoting: the denominator at node 1 is ih_0 + ih_1, those behind it exceed ih[j-1] +
// 2 ih[j], and the last one, h_{n-3} - (h_{n-2} + h_{n-3}) cp[n-2], stays above h_{n-3}^2 / (h_{n-2} + 2 h_{n-3}).
inline void rim_tab_spline_row_grid(const double *y, size_t n, const double *h, const double *ih, double *m, double *cp, double *dp,
                                    int ends = RIM_TAB_ENDS_NATURAL)
{
    const size_t last = n - 1;
    if (ends) {
        const double s0 = (y[1] - y[0]) / h[0], s1 = (y[2] - y[1]) / h[1], w = h[0] + h[1];
        cp[0] = w / h[1];
        dp[0] = ((3. * h[0] + 2. * h[1]) * h[1] * s0 + h[0] * h[0] * s1) / w / h[1];
    } else {
        cp[0] = 0.5;
        dp[0] = 3. * ((y[1] - y[0]) / h[0]) / 2.;
    }
    for (size_t j = 1; j < last; j++) {
        const double sl = (y[j] - y[j - 1]) / h[j - 1], sr = (y[j + 1] - y[j]) / h[j];
        const double rhs = 3. * (sl * ih[j - 1] + sr * ih[j]);
        const double den = 2. * (ih[j - 1] + ih[j]) - ih[j - 1] * cp[j - 1];
        cp[j] = ih[j] / den;
        dp[j] = (rhs - ih[j - 1] * dp[j - 1]) / den;
    }
    if (ends) {
        const double sl = (y[last - 1] - y[last - 2]) / h[last - 2], sr = (y[last] - y[last - 1]) / h[last - 1];
        const double w = h[last - 1] + h[last - 2];
        const double rhs = ((3. * h[last - 1] + 2. * h[last - 2]) * h[last - 2] * sr + h[last - 1] * h[last - 1] * sl) / w;
        m[last] = (rhs - w * dp[last - 1]) / (h[last - 2] - w * cp[last - 1]);
    } else {
        m[last] = (3. * ((y[last] - y[last - 1]) / h[last - 1]) - dp[last - 1]) / (2. - cp[last - 1]);
    }
    for (size_t j = last; j-- > 0;) m[j] = dp[j] - cp[j] * m[j + 1];
}

// the guide of a set on the nodes u[0 .. n_nodes-1] (dev_symphony.h: tab_grid_cell): word c = min(the last node in a cell
// below c, n_nodes - 2), 0 where there is none; cells + 1 words
inline void rim_tab_fill_guide(const double *u, size_t n_nodes, size_t cells, double inv_cell, uint32_t *guide)
{
    using namespace rim;
    size_t j = 0;
    for (size_t c = 0; c <= cells; c++) {
        while (j < n_nodes && (size_t) tab_grid_cell(u[j], u[0], inv_cell, (double) (cells - 1)) < c) j++;
        size_t w = j ? j - 1 : 0;
        if (w > n_nodes - 2) w = n_nodes - 2;
        guide[c] = (uint32_t) w;
    }
}

// the set on given nodes as one block of doubles (dev_symphony.h: tab_grid_*); rim_tab_check_grid() has passed.  sin_k
// null: k = 0 for every table.  P of a table with a pitch row is 0 as built and the caller fills it, as for a sin^k set.
inline void rim_tab_build_grid(size_t n_tables, size_t n_nodes, const double *gamma, const double *log_n, size_t n_mu,
                               const double *log_g, const double *sin_k, std::vector<double> &blob)
{
    using namespace rim;
    if (!log_g) n_mu = 0;
    size_t cells = 8;
    while (cells < n_nodes) cells *= 2;
    const size_t tail = tab_grid_tail(n_tables, n_nodes, cells);
    const size_t stride = (size_t) TAB_PITCHY_PRE + TAB_PITCH_HDR + n_mu * 2;
    blob.assign(tail + TAB_HDR_DOUBLES + n_tables * stride, 0.);
    std::vector<double> u(n_nodes), h(n_nodes), ih(n_nodes), m(n_nodes), cp(n_nodes), dp(n_nodes);
    for (size_t j = 0; j < n_nodes; j++) u[j] = rim_log(gamma[j]);
    for (size_t j = 0; j + 1 < n_nodes; j++) { h[j] = u[j + 1] - u[j]; ih[j] = 1. / h[j]; }
    h[n_nodes - 1] = 0.; ih[n_nodes - 1] = 0.;
    const double inv_cell = (double) cells / (u[n_nodes - 1] - u[0]);
    rim_tab_set_header(blob.data(), n_tables, n_nodes, gamma[0], gamma[n_nodes - 1], u[0], inv_cell, (double) cells, (double) n_mu);
    rim_tab_fill_guide(u.data(), n_nodes, cells, inv_cell, (uint32_t *) (blob.data() + TAB_HDR_DOUBLES));
    for (size_t t = 0; t < n_tables; t++) {
        const double *y = log_n + t * n_nodes;
        double *row = blob.data() + TAB_HDR_DOUBLES + tab_grid_guide_doubles(cells) + t * n_nodes * 4;
        rim_tab_spline_row_grid(y, n_nodes, h.data(), ih.data(), m.data(), cp.data(), dp.data());
        for (size_t i = 0; i < n_nodes; i++) {
            row[4 * i] = u[i];
            row[4 * i + 1] = y[i];
            row[4 * i + 2] = m[i];
            row[4 * i + 3] = ih[i];
        }
    }
    // the tail: a sin^k set's table headers and pitch rows behind a header that names no gamma nodes
    double *th = blob.data() + tail;
    rim_tab_set_header(th, n_tables, 0, gamma[0], gamma[n_nodes - 1], 0., 0., 0., (double) n_mu);
    const double hm = n_mu ? 2. / (double) (n_mu - 1) : 0.;
    std::vector<double> cpm(n_mu), dpm(n_mu);
    for (size_t t = 0; t < n_tables; t++)
        rim_tab_build_pitchy_table(th + TAB_HDR_DOUBLES, t, sin_k ? sin_k[t] : 0., n_mu, log_g, hm, cpm.data(), dpm.data());
}

#define RIM_TAB_2D_MIN_MU 8
#define RIM_TAB_2D_MAX_MU 1024
#define RIM_TAB_2D_MAX_CELLS ((size_t) 1 << 20)

// what rim_tab_check_2d asks of everything but the values: for a caller whose log_n the host cannot read (tab_install.h)
inline int rim_tab_check_2d_geometry(size_t n_tables, size_t n_nodes, double gamma_lo, double gamma_hi, size_t n_mu)
{
    if (n_tables < 1 || n_nodes < RIM_TAB_MIN_NODES || n_nodes > RIM_TAB_MAX_NODES) return -1;
    if (n_mu < RIM_TAB_2D_MIN_MU || n_mu > RIM_TAB_2D_MAX_MU || n_nodes * n_mu > RIM_TAB_2D_MAX_CELLS) return -1;
    if (n_tables > ((size_t) 1 << 40) / (n_nodes * n_mu)) return -1;
    return rim_tab_check_range(gamma_lo, gamma_hi);
}

// a 2-D set: log_n [n_tables][n_nodes][n_mu], mu fastest.  0, or -1 for bad geometry or a non-finite value
inline int rim_tab_check_2d(size_t n_tables, size_t n_nodes, double gamma_lo, double gamma_hi, size_t n_mu, const double *log_n)
{
    if (!log_n || rim_tab_check_2d_geometry(n_tables, n_nodes, gamma_lo, gamma_hi, n_mu)) return -1;
    for (size_t i = 0; i < n_tables * n_nodes * n_mu; i++)
        if (!rim_isfinite(log_n[i])) return -1;
    return 0;
}

// What a 2-D set holds in front of its node data, the words that do not depend on log_n: the header and the table headers
// (normalisations 0).  h, hm: the node spacings along u and mu as the sweeps use them.  rim_tab_build_2d begins with it.
inline void rim_tab_front_2d(size_t n_tables, size_t n_nodes, double gamma_lo, double gamma_hi, size_t n_mu, std::vector<double> &blob,
                             double &h, double &hm, int ends = 0)
{
    using namespace rim;
    const double u_lo = rim_log(gamma_lo), u_hi = rim_log(gamma_hi);
    h = (u_hi - u_lo) / (double) (n_nodes - 1);
    hm = 2. / (double) (n_mu - 1);
    blob.assign((size_t) TAB_HDR_DOUBLES + n_tables * TAB_2D_HDR, 0.);
    rim_tab_set_header(blob.data(), n_tables, n_nodes, gamma_lo, gamma_hi, u_lo, 1. / h, h, -(double) n_mu);
    for (size_t t = 0; t < n_tables; t++) {
        double *th = blob.data() + TAB_HDR_DOUBLES + t * TAB_2D_HDR;
        th[TAB_2D_LAST] = (double) (n_mu - 2);
        th[TAB_2D_INVH] = 1. / hm;
        th[TAB_2D_H] = hm;
        th[TAB_2D_ENDS] = (double) ends;
    }
}

// the 2-D set as one block of doubles (dev_symphony.h: TAB_2D_*); rim_tab_check_2d() has passed.  The order of the three
// families of sweeps is fixed, because the bits depend on it: S_u along u for each mu column, S_mu along mu for each u row,
// S_umu along u through the S_mu values of a column.
inline void rim_tab_build_2d(size_t n_tables, size_t n_nodes, double gamma_lo, double gamma_hi, size_t n_mu, const double *log_n,
                             std::vector<double> &blob, int ends_u = 0, int ends_mu = 0)
{
    using namespace rim;
    double h, hm;
    rim_tab_front_2d(n_tables, n_nodes, gamma_lo, gamma_hi, n_mu, blob, h, hm, ends_u + 2 * ends_mu);
    const size_t per_table = n_nodes * n_mu * 4;
    blob.resize(blob.size() + n_tables * per_table, 0.);
    const size_t longest = n_nodes > n_mu ? n_nodes : n_mu;
    std::vector<double> y(longest), pairs(2 * longest), cp(longest), dp(longest);
    for (size_t t = 0; t < n_tables; t++) {
        const double *src = log_n + t * n_nodes * n_mu;
        double *nodes = blob.data() + TAB_HDR_DOUBLES + n_tables * TAB_2D_HDR + t * per_table;
        for (size_t j = 0; j < n_mu; j++) {
            for (size_t i = 0; i < n_nodes; i++) y[i] = src[i * n_mu + j];
            rim_tab_spline_row(y.data(), n_nodes, h, pairs.data(), cp.data(), dp.data(), ends_u);
            for (size_t i = 0; i < n_nodes; i++) {
                nodes[(i * n_mu + j) * 4] = pairs[2 * i];
                nodes[(i * n_mu + j) * 4 + 1] = pairs[2 * i + 1];
            }
        }
        for (size_t i = 0; i < n_nodes; i++) {
            rim_tab_spline_row(src + i * n_mu, n_mu, hm, pairs.data(), cp.data(), dp.data(), ends_mu);
            for (size_t j = 0; j < n_mu; j++) nodes[(i * n_mu + j) * 4 + 2] = pairs[2 * j + 1];
        }
        for (size_t j = 0; j < n_mu; j++) {
            for (size_t i = 0; i < n_nodes; i++) y[i] = nodes[(i * n_mu + j) * 4 + 2];
            rim_tab_spline_row(y.data(), n_nodes, h, pairs.data(), cp.data(), dp.data(), ends_u);
            for (size_t i = 0; i < n_nodes; i++) nodes[(i * n_mu + j) * 4 + 3] = pairs[2 * i + 1];
        }
    }
}

// rim_tab_check_2d() for a 2-D set on given nodes: gamma [n_nodes] as rim_tab_check_grid demands it, log_n
// [n_tables][n_nodes][n_mu] and n_mu within the 2-D form's limits; the _geometry form asks everything but the values
inline int rim_tab_check_2d_grid_geometry(size_t n_tables, size_t n_nodes, const double *gamma, size_t n_mu)
{
    if (rim_tab_check_gamma_nodes(n_nodes, gamma)) return -1;
    return rim_tab_check_2d_geometry(n_tables, n_nodes, gamma[0], gamma[n_nodes - 1], n_mu);
}

inline int rim_tab_check_2d_grid(size_t n_tables, size_t n_nodes, const double *gamma, size_t n_mu, const double *log_n)
{
    if (rim_tab_check_gamma_nodes(n_nodes, gamma)) return -1;
    return rim_tab_check_2d(n_tables, n_nodes, gamma[0], gamma[n_nodes - 1], n_mu, log_n);
}

// What a 2-D set on given gamma nodes holds in front of its node data: the header, the table headers (normalisations 0), the
// guide and the u nodes.  h, ih [n_nodes]: u_{i+1} - u_i and its reciprocal as the sweeps along u use them (0 in the last
// word); hm: the spacing of the mu nodes.  rim_tab_build_2d_grid begins with it.
inline void rim_tab_front_2d_grid(size_t n_tables, size_t n_nodes, const double *gamma, size_t n_mu, std::vector<double> &blob,
                                  std::vector<double> &h, std::vector<double> &ih, double &hm, int ends = 0)
{
    using namespace rim;
    size_t cells = 8;
    while (cells < n_nodes) cells *= 2;
    hm = 2. / (double) (n_mu - 1);
    blob.assign(tab_2d_grid_nodes_at(n_tables, n_nodes, cells), 0.);
    std::vector<double> u(n_nodes);
    h.assign(n_nodes, 0.); ih.assign(n_nodes, 0.);
    for (size_t j = 0; j < n_nodes; j++) u[j] = rim_log(gamma[j]);
    for (size_t j = 0; j + 1 < n_nodes; j++) { h[j] = u[j + 1] - u[j]; ih[j] = 1. / h[j]; }
    h[n_nodes - 1] = 0.; ih[n_nodes - 1] = 0.;
    const double inv_cell = (double) cells / (u[n_nodes - 1] - u[0]);
    rim_tab_set_header(blob.data(), n_tables, n_nodes, gamma[0], gamma[n_nodes - 1], u[0], inv_cell, (double) cells, -(double) n_mu);
    rim_tab_fill_guide(u.data(), n_nodes, cells, inv_cell, (uint32_t *) (blob.data() + tab_2d_grid_guide_at(n_tables)));
    double *un = blob.data() + tab_2d_grid_guide_at(n_tables) + tab_grid_guide_doubles(cells);
    for (size_t i = 0; i < n_nodes; i++) { un[2 * i] = u[i]; un[2 * i + 1] = ih[i]; }
    for (size_t t = 0; t < n_tables; t++) {
        double *th = blob.data() + TAB_HDR_DOUBLES + t * TAB_2D_HDR;
        th[TAB_2D_LAST] = (double) (n_mu - 2);
        th[TAB_2D_INVH] = 1. / hm;
        th[TAB_2D_H] = hm;
        th[TAB_2D_ENDS] = (double) ends;
    }
}

// the 2-D set on given nodes as one block of doubles (dev_symphony.h: tab_2d_grid_*); rim_tab_check_2d_grid() has passed.
// The three families of sweeps in rim_tab_build_2d's order, those along u through rim_tab_spline_row_grid on h_i = u_{i+1} -
// u_i; the guide as rim_tab_build_grid fills it.  The normalisation of a table is 0 as built and the caller fills it.
inline void rim_tab_build_2d_grid(size_t n_tables, size_t n_nodes, const double *gamma, size_t n_mu, const double *log_n,
                                  std::vector<double> &blob)
{
    using namespace rim;
    std::vector<double> h, ih;
    double hm;
    rim_tab_front_2d_grid(n_tables, n_nodes, gamma, n_mu, blob, h, ih, hm);
    const size_t per_table = n_nodes * n_mu * 4, nodes_at = blob.size();
    blob.resize(nodes_at + n_tables * per_table, 0.);
    const size_t longest = n_nodes > n_mu ? n_nodes : n_mu;
    std::vector<double> m(n_nodes), y(longest), pairs(2 * longest), cp(longest), dp(longest);
    for (size_t t = 0; t < n_tables; t++) {
        const double *src = log_n + t * n_nodes * n_mu;
        double *nodes = blob.data() + nodes_at + t * per_table;
        for (size_t j = 0; j < n_mu; j++) {
            for (size_t i = 0; i < n_nodes; i++) y[i] = src[i * n_mu + j];
            rim_tab_spline_row_grid(y.data(), n_nodes, h.data(), ih.data(), m.data(), cp.data(), dp.data());
            for (size_t i = 0; i < n_nodes; i++) {
                nodes[(i * n_mu + j) * 4] = y[i];
                nodes[(i * n_mu + j) * 4 + 1] = m[i];
            }
        }
        for (size_t i = 0; i < n_nodes; i++) {
            rim_tab_spline_row(src + i * n_mu, n_mu, hm, pairs.data(), cp.data(), dp.data());
            for (size_t j = 0; j < n_mu; j++) nodes[(i * n_mu + j) * 4 + 2] = pairs[2 * j + 1];
        }
        for (size_t j = 0; j < n_mu; j++) {
            for (size_t i = 0; i < n_nodes; i++) y[i] = nodes[(i * n_mu + j) * 4 + 2];
            rim_tab_spline_row_grid(y.data(), n_nodes, h.data(), ih.data(), m.data(), cp.data(), dp.data());
            for (size_t i = 0; i < n_nodes; i++) nodes[(i * n_mu + j) * 4 + 3] = m[i];
        }
    }
}

// The same with a choice of the spline's ends along u and along mu (RIM_TAB_ENDS_*), an overload and not a defaulted argument:
// the text above stays as it was written, because a test of the tests builds a mutant of it
// (tests/test_tabulated_2d_grid_host.py).  Natural ends on both axes give the set above, word for word.
inline void rim_tab_build_2d_grid(size_t n_tables, size_t n_nodes, const double *gamma, size_t n_mu, const double *log_n,
                                  std::vector<double> &blob, int ends_u, int ends_mu)
{
    using namespace rim;
    std::vector<double> h, ih;
    double hm;
    rim_tab_front_2d_grid(n_tables, n_nodes, gamma, n_mu, blob, h, ih, hm, ends_u + 2 * ends_mu);
    const size_t per_table = n_nodes * n_mu * 4, nodes_at = blob.size();
    blob.resize(nodes_at + n_tables * per_table, 0.);
    const size_t longest = n_nodes > n_mu ? n_nodes : n_mu;
    std::vector<double> m(n_nodes), y(longest), pairs(2 * longest), cp(longest), dp(longest);
    for (size_t t = 0; t < n_tables; t++) {
        const double *src = log_n + t * n_nodes * n_mu;
        double *nodes = blob.data() + nodes_at + t * per_table;
        for (size_t j = 0; j < n_mu; j++) {
            for (size_t i = 0; i < n_nodes; i++) y[i] = src[i * n_mu + j];
            rim_tab_spline_row_grid(y.data(), n_nodes, h.data(), ih.data(), m.data(), cp.data(), dp.data(), ends_u);
            for (size_t i = 0; i < n_nodes; i++) {
                nodes[(i * n_mu + j) * 4] = y[i];
                nodes[(i * n_mu + j) * 4 + 1] = m[i];
            }
        }
        for (size_t i = 0; i < n_nodes; i++) {
            rim_tab_spline_row(src + i * n_mu, n_mu, hm, pairs.data(), cp.data(), dp.data(), ends_mu);
            for (size_t j = 0; j < n_mu; j++) nodes[(i * n_mu + j) * 4 + 2] = pairs[2 * j + 1];
        }
        for (size_t j = 0; j < n_mu; j++) {
            for (size_t i = 0; i < n_nodes; i++) y[i] = nodes[(i * n_mu + j) * 4 + 2];
            rim_tab_spline_row_grid(y.data(), n_nodes, h.data(), ih.data(), m.data(), cp.data(), dp.data(), ends_u);
            for (size_t i = 0; i < n_nodes; i++) nodes[(i * n_mu + j) * 4 + 3] = m[i];
        }
    }
}

// A 2-D set of either form with a sin^k xi prefactor per table: the form's own check and sin_k as rim_tab_check_sin_k
// demands it; the form's own blob with k in the word TAB_2D_K of each table's header, which is 0 as the form builds it (the
// table headers of both forms start TAB_HDR_DOUBLES words into the set).  The normalisation is 0 as built, as ever.
inline int rim_tab_check_2d_pitchy(size_t n_tables, size_t n_nodes, double gamma_lo, double gamma_hi, size_t n_mu, const double *log_n,
                                   const double *sin_k)
{
    if (rim_tab_check_2d(n_tables, n_nodes, gamma_lo, gamma_hi, n_mu, log_n) || !sin_k) return -1;
    return rim_tab_check_sin_k(n_tables, sin_k);
}

inline int rim_tab_check_2d_grid_pitchy(size_t n_tables, size_t n_nodes, const double *gamma, size_t n_mu, const double *log_n,
                                        const double *sin_k)
{
    if (rim_tab_check_2d_grid(n_tables, n_nodes, gamma, n_mu, log_n) || !sin_k) return -1;
    return rim_tab_check_sin_k(n_tables, sin_k);
}

inline void rim_tab_put_2d_sin_k(size_t n_tables, const double *sin_k, std::vector<double> &blob)
{
    using namespace rim;
    for (size_t t = 0; t < n_tables; t++) blob[(size_t) TAB_HDR_DOUBLES + t * TAB_2D_HDR + TAB_2D_K] = sin_k[t];
}

inline void rim_tab_build_2d_pitchy(size_t n_tables, size_t n_nodes, double gamma_lo, double gamma_hi, size_t n_mu,
                                    const double *log_n, const double *sin_k, std::vector<double> &blob, int ends_u = 0, int ends_mu = 0)
{
    rim_tab_build_2d(n_tables, n_nodes, gamma_lo, gamma_hi, n_mu, log_n, blob, ends_u, ends_mu);
    rim_tab_put_2d_sin_k(n_tables, sin_k, blob);
}

inline void rim_tab_build_2d_grid_pitchy(size_t n_tables, size_t n_nodes, const double *gamma, size_t n_mu, const double *log_n,
                                         const double *sin_k, std::vector<double> &blob, int ends_u = 0, int ends_mu = 0)
{
    rim_tab_build_2d_grid(n_tables, n_nodes, gamma, n_mu, log_n, blob, ends_u, ends_mu);
    rim_tab_put_2d_sin_k(n_tables, sin_k, blob);
}

// the mu nodes of a 2-D set on given mu nodes: mu [n_mu], n_mu within the 2-D form's limits, every value finite, strictly
// increasing, mu[0] == -1 and mu[n_mu - 1] == +1 exactly (the surface covers the whole range: no extrapolation in the
// normalisation, and the guide's cells are exact)
inline int rim_tab_check_mu_nodes(size_t n_mu, const double *mu)
{
    if (!mu || n_mu < RIM_TAB_2D_MIN_MU || n_mu > RIM_TAB_2D_MAX_MU) return -1;
    for (size_t j = 0; j < n_mu; j++)
        if (!rim_isfinite(mu[j])) return -1;
    if (mu[0] != -1. || mu[n_mu - 1] != 1.) return -1;
    for (size_t j = 0; j + 1 < n_mu; j++)
        if (!(mu[j] < mu[j + 1])) return -1;
    return 0;
}

// rim_tab_check_2d_grid() for a set on given mu nodes too; sin_k may be null (no prefactor).  The _geometry form asks
// everything but the values.
inline int rim_tab_check_2d_nodes_geometry(size_t n_tables, size_t n_nodes, const double *gamma, size_t n_mu, const double *mu,
                                           const double *sin_k)
{
    if (rim_tab_check_mu_nodes(n_mu, mu)) return -1;
    if (rim_tab_check_2d_grid_geometry(n_tables, n_nodes, gamma, n_mu)) return -1;
    return sin_k ? rim_tab_check_sin_k(n_tables, sin_k) : 0;
}

inline int rim_tab_check_2d_nodes(size_t n_tables, size_t n_nodes, const double *gamma, size_t n_mu, const double *mu,
                                  const double *log_n, const double *sin_k)
{
    if (rim_tab_check_mu_nodes(n_mu, mu)) return -1;
    if (rim_tab_check_2d_grid(n_tables, n_nodes, gamma, n_mu, log_n)) return -1;
    return sin_k ? rim_tab_check_sin_k(n_tables, sin_k) : 0;
}

// What a 2-D set on given gamma and mu nodes holds in front of its node data: the header, the table headers with sin_k (null:
// 0) and normalisations 0, both guides and both node arrays.  h, ih [n_nodes] and hm, ihm [n_mu]: the node distances and their
// reciprocals as the sweeps use them (0 in the last word).  rim_tab_build_2d_nodes begins with it.
inline void rim_tab_front_2d_nodes(size_t n_tables, size_t n_nodes, const double *gamma, size_t n_mu, const double *mu,
                                   const double *sin_k, std::vector<double> &blob, std::vector<double> &h, std::vector<double> &ih,
                                   std::vector<double> &hm, std::vector<double> &ihm, int ends = 0)
{
    using namespace rim;
    size_t cells = 8, mu_cells = 8;
    while (cells < n_nodes) cells *= 2;
    while (mu_cells < n_mu) mu_cells *= 2;
    const size_t mu_guide_at = tab_2d_nodes_mu_guide_at(n_tables, n_nodes, cells);
    const size_t mu_nodes_at = mu_guide_at + tab_grid_guide_doubles(mu_cells);
    blob.assign(tab_2d_nodes_nodes_at(n_tables, n_nodes, cells, n_mu, mu_cells), 0.);
    std::vector<double> u(n_nodes);
    h.assign(n_nodes, 0.); ih.assign(n_nodes, 0.); hm.assign(n_mu, 0.); ihm.assign(n_mu, 0.);
    for (size_t j = 0; j < n_nodes; j++) u[j] = rim_log(gamma[j]);
    for (size_t j = 0; j + 1 < n_nodes; j++) { h[j] = u[j + 1] - u[j]; ih[j] = 1. / h[j]; }
    h[n_nodes - 1] = 0.; ih[n_nodes - 1] = 0.;
    for (size_t j = 0; j + 1 < n_mu; j++) { hm[j] = mu[j + 1] - mu[j]; ihm[j] = 1. / hm[j]; }
    hm[n_mu - 1] = 0.; ihm[n_mu - 1] = 0.;
    const double inv_cell = (double) cells / (u[n_nodes - 1] - u[0]);
    const double inv_mu_cell = (double) mu_cells / (mu[n_mu - 1] - mu[0]);
    rim_tab_set_header(blob.data(), n_tables, n_nodes, gamma[0], gamma[n_nodes - 1], u[0], inv_cell, (double) cells, -(double) n_mu);
    rim_tab_fill_guide(u.data(), n_nodes, cells, inv_cell, (uint32_t *) (blob.data() + tab_2d_grid_guide_at(n_tables)));
    double *un = blob.data() + tab_2d_grid_guide_at(n_tables) + tab_grid_guide_doubles(cells);
    for (size_t i = 0; i < n_nodes; i++) { un[2 * i] = u[i]; un[2 * i + 1] = ih[i]; }
    rim_tab_fill_guide(mu, n_mu, mu_cells, inv_mu_cell, (uint32_t *) (blob.data() + mu_guide_at));
    double *mn = blob.data() + mu_nodes_at;
    for (size_t j = 0; j < n_mu; j++) { mn[2 * j] = mu[j]; mn[2 * j + 1] = ihm[j]; }
    for (size_t t = 0; t < n_tables; t++) {
        const size_t th_at = (size_t) TAB_HDR_DOUBLES + t * TAB_2D_HDR;
        double *th = blob.data() + th_at;
        th[TAB_2D_LAST] = (double) (n_mu - 2);
        th[TAB_2D_INVH] = inv_mu_cell;
        th[TAB_2D_H] = (double) mu_cells;
        th[TAB_2D_K] = sin_k ? sin_k[t] : 0.;
        th[TAB_2D_MU_GUIDE] = (double) (mu_guide_at - th_at);
        th[TAB_2D_MU_NODES] = (double) (mu_nodes_at - th_at);
        th[TAB_2D_ENDS] = (double) ends;
    }
}

// the 2-D set on given gamma and mu nodes as one block of doubles (dev_symphony.h: tab_2d_nodes_*); rim_tab_check_2d_nodes()
// has passed.  The three families of sweeps in rim_tab_build_2d's order, all of them through rim_tab_spline_row_grid: along u
// on h_i = u_{i+1} - u_i, along mu on h_j = mu_{j+1} - mu_j, each with its 1 / h formed once per set.  Both guides as
// rim_tab_build_grid fills its one.  sin_k null: TAB_2D_K stays 0.  The normalisation of a table is 0 as built.
inline void rim_tab_build_2d_nodes(size_t n_tables, size_t n_nodes, const double *gamma, size_t n_mu, const double *mu,
                                   const double *log_n, const double *sin_k, std::vector<double> &blob, int ends_u = 0, int ends_mu = 0)
{
    using namespace rim;
    std::vector<double> h, ih, hm, ihm;
    rim_tab_front_2d_nodes(n_tables, n_nodes, gamma, n_mu, mu, sin_k, blob, h, ih, hm, ihm, ends_u + 2 * ends_mu);
    const size_t per_table = n_nodes * n_mu * 4, nodes_at = blob.size();
    blob.resize(nodes_at + n_tables * per_table, 0.);
    const size_t longest = n_nodes > n_mu ? n_nodes : n_mu;
    std::vector<double> col(longest), m(longest), cp(longest), dp(longest);
    for (size_t t = 0; t < n_tables; t++) {
        const double *src = log_n + t * n_nodes * n_mu;
        double *nodes = blob.data() + nodes_at + t * per_table;
        for (size_t j = 0; j < n_mu; j++) {
            for (size_t i = 0; i < n_nodes; i++) col[i] = src[i * n_mu + j];
            rim_tab_spline_row_grid(col.data(), n_nodes, h.data(), ih.data(), m.data(), cp.data(), dp.data(), ends_u);
            for (size_t i = 0; i < n_nodes; i++) {
                nodes[(i * n_mu + j) * 4] = col[i];
                nodes[(i * n_mu + j) * 4 + 1] = m[i];
            }
        }
        for (size_t i = 0; i < n_nodes; i++) {
            rim_tab_spline_row_grid(src + i * n_mu, n_mu, hm.data(), ihm.data(), m.data(), cp.data(), dp.data(), ends_mu);
            for (size_t j = 0; j < n_mu; j++) nodes[(i * n_mu + j) * 4 + 2] = m[j];
        }
        for (size_t j = 0; j < n_mu; j++) {
            for (size_t i = 0; i < n_nodes; i++) col[i] = nodes[(i * n_mu + j) * 4 + 2];
            rim_tab_spline_row_grid(col.data(), n_nodes, h.data(), ih.data(), m.data(), cp.data(), dp.data(), ends_u);
            for (size_t i = 0; i < n_nodes; i++) nodes[(i * n_mu + j) * 4 + 3] = m[i];
        }
    }
}

// A FAMILY of energy tables on nodes uniform in ln gamma (dev_symphony.h: tab_family_*), with or without a sin^k xi prefactor
// per table (sin_k null: without).  The checks are the plain forms' own: rim_tab_check, rim_tab_check_sin_k.
inline int rim_tab_check_family(size_t n_tables, size_t n_nodes, double gamma_lo, double gamma_hi, const double *log_n,
                                const double *sin_k)
{
    if (rim_tab_check(n_tables, n_nodes, gamma_lo, gamma_hi, log_n)) return -1;
    return sin_k ? rim_tab_check_sin_k(n_tables, sin_k) : 0;
}

// The family as one block of doubles; rim_tab_check_family() has passed.  The rows are rim_tab_build()'s, table by table --
// the spline solve is linear in the data, so a blend of two solved rows is the solved blend --, then the last row once more,
// then the headers of a sin^k set without g (rim_tab_build_pitchy_table), P the closed form.
inline void rim_tab_build_family(size_t n_tables, size_t n_nodes, double gamma_lo, double gamma_hi, const double *log_n,
                                 const double *sin_k, std::vector<double> &blob)
{
    using namespace rim;
    rim_tab_build(n_tables, n_nodes, gamma_lo, gamma_hi, log_n, blob);
    const size_t row = n_nodes * 2, rows_end = blob.size();
    blob.resize(rows_end + row + (sin_k ? n_tables * (size_t) TAB_FAMILY_LINE : 0), 0.);
    for (size_t j = 0; j < row; j++) blob[rows_end + j] = blob[rows_end - row + j];
    if (!sin_k) return;
    for (size_t t = 0; t < n_tables; t++)
        rim_tab_build_pitchy_table(blob.data() + rows_end + row, t, sin_k[t], 0, nullptr, 0., nullptr, nullptr);
}

// A FAMILY of 2-D surfaces on given gamma and mu nodes (dev_symphony.h: tab_2d_family_line, tab_bicubic_family), with or
// without a sin^k xi prefactor per table (sin_k null: without).  The check is the plain form's own.
inline int rim_tab_check_2d_family(size_t n_tables, size_t n_nodes, const double *gamma, size_t n_mu, const double *mu,
                                   const double *log_n, const double *sin_k)
{
    return rim_tab_check_2d_nodes(n_tables, n_nodes, gamma, n_mu, mu, log_n, sin_k);
}

// The family as one block of doubles; rim_tab_check_2d_family() has passed.  The set of rim_tab_build_2d_nodes word for word
// -- the tensor-product solve is linear in the data for either kind of ends, so a blend of two solved tables is the solved
// blend; no trailing copy: a row at the last table blends it with itself --, but for TAB_2D_NORM of every table header, which
// is a NaN and stays one: the normalisation is per row.  TAB_2D_ENDS records the ends as ever.
inline void rim_tab_build_2d_family(size_t n_tables, size_t n_nodes, const double *gamma, size_t n_mu, const double *mu,
                                    const double *log_n, const double *sin_k, std::vector<double> &blob, int ends_u = 0, int ends_mu = 0)
{
    using namespace rim;
    rim_tab_build_2d_nodes(n_tables, n_nodes, gamma, n_mu, mu, log_n, sin_k, blob, ends_u, ends_mu);
    for (size_t t = 0; t < n_tables; t++) blob[(size_t) TAB_HDR_DOUBLES + t * TAB_2D_HDR + TAB_2D_NORM] = RIM_NAN;
}

// The same family blended CUBICALLY across its tables (dev_symphony.h: tab_2d_family_cubic_line, tab_bicubic_family_cubic).
// The linear family's check; at least four tables, the stencil of a 4-point Lagrange cubic; `param`, where given, the knots
// the tables are spaced in: finite and strictly monotonic, increasing or decreasing (null: the index itself).
inline int rim_tab_check_2d_family_cubic(size_t n_tables, size_t n_nodes, const double *gamma, size_t n_mu, const double *mu,
                                         const double *log_n, const double *sin_k, const double *param)
{
    if (n_tables < 4) return 1;
    if (rim_tab_check_2d_family(n_tables, n_nodes, gamma, n_mu, mu, log_n, sin_k)) return 1;
    if (!param) return 0;
    for (size_t t = 0; t < n_tables; t++)
        if (!(param[t] - param[t] == 0.)) return 1;         // NaN or infinite
    const bool up = param[1] > param[0];
    for (size_t t = 0; t + 1 < n_tables; t++)
        if (!(up ? param[t + 1] > param[t] : param[t + 1] < param[t])) return 1;
    return 0;
}

// That family as one block of doubles; rim_tab_check_2d_family_cubic() has passed.  The set of rim_tab_build_2d_family word for
// word -- any fixed linear combination of solved tables is the solved combination, so the cubic needs no solve of its own --
// followed by the n_tables knot words.
inline void rim_tab_build_2d_family_cubic(size_t n_tables, size_t n_nodes, const double *gamma, size_t n_mu, const double *mu,
                                          const double *log_n, const double *sin_k, const double *param, std::vector<double> &blob,
                                          int ends_u = 0, int ends_mu = 0)
{
    rim_tab_build_2d_family(n_tables, n_nodes, gamma, n_mu, mu, log_n, sin_k, blob, ends_u, ends_mu);
    for (size_t t = 0; t < n_tables; t++) blob.push_back(param ? param[t] : (double) t);
}

#endif
