// tab_install.h -- the node data of a 2-D table set solved line by line, for a set whose ln n(gamma, mu) is in device
// memory (rimphony_ctx_set_tables_2d_device): what rim_tab_build_2d, rim_tab_build_2d_grid and rim_tab_build_2d_nodes
// (tab_spline.h) write behind the front of their sets, word for word.
//
// The Thomas sweep of both line solvers of tab_spline.h splits into what depends on the axis and what depends on the line.
// The swept diagonal cp[j] and the denominators den[j] depend on the axis only: rim_tab_install_axis forms them once per set
// and axis, on the host, with the host solver's own expressions.  The forward sweep's dp[j] of a line is written into the
// very word that will hold the slope and the backward sweep overwrites it in place, so a line needs no workspace beyond the
// set.  Every operation keeps the host's form -- a division by den stays a division, 3. * (...) / h / 2. stays as written --
// and no multiply-add fuses (-ffp-contract=off, as for everything here): the bits are the host's.
//
// rim_tab_install_line solves one line; rim_tab_install_family_line says which line of which family of sweeps a line index
// is.  The kernels of rimphony_tab_install.hip call it with their lane's index; the tests loop the host build of the same
// text over the indices.  The families, in rim_tab_build_2d's order, because the bits depend on it:
//   0  the values and S_u along u for every (table, mu column); the input stride is n_mu
//   1  S_mu along mu for every (table, gamma row)
//   2  S_umu along u through the S_mu words of a column -- it reads what family 1 wrote, so it runs after it
// All indices are size_t.
//
// An axis with not-a-knot ends (RimTabAxis::ends, tab_spline.h: RIM_TAB_ENDS_NOT_A_KNOT) differs in its first and last rows
// only: cp[0] and den[n - 1] of the axis block are the host's for those rows, and the line forms their right-hand sides from
// y_2 and y_{n-3} as well -- the first it reads ahead, the second it keeps from the pass -- with the host's expressions.
#ifndef RIM_TAB_INSTALL_H
#define RIM_TAB_INSTALL_H

#include <cstddef>
#include "dev_bessel.h"     // RIM_DEV

// One axis of a set as the line solver reads it: n nodes, either `hu` apart (grid == 0: rim_tab_spline_row) or h[j] = x_{j+1}
// - x_j apart with ih[j] = 1 / h[j] (grid != 0: rim_tab_spline_row_grid).  cp, den: n doubles each, rim_tab_install_axis.
// ends: 0 natural, 1 not-a-knot.
struct RimTabAxis {
    const double *cp, *den, *h, *ih;
    double hu;
    size_t n;
    int grid, ends;
};

// doubles of an axis block {cp[n], den[n], h[n], ih[n]}; the last two rows stay 0 for a uniform axis
inline size_t rim_tab_axis_doubles(size_t n) { return 4 * n; }

// The axis block at `blk` (rim_tab_axis_doubles(n) doubles) for n nodes hu apart (h, ih null) or h[], ih[] apart: cp and den
// as the host's sweep forms them, in its own expressions, for the ends `ends` of the axis.  den[0] is never read; a set on
// given nodes never reads cp[n - 1].
inline void rim_tab_install_axis(size_t n, double hu, const double *h, const double *ih, double *blk, int ends = 0)
{
    double *cp = blk, *den = blk + n, *bh = blk + 2 * n, *bih = blk + 3 * n;
    const size_t last = n - 1;
    cp[0] = ends ? 2. : 0.5;
    den[0] = 0.;
    if (!h) {
        (void) hu;
        for (size_t j = 1; j <= last; j++) {
            const double diag = j < last ? 4. : 2.;
            den[j] = (ends && j == last) ? 1. - 2. * cp[j - 1] : diag - cp[j - 1];
            cp[j] = 1. / den[j];
            bh[j] = 0.; bih[j] = 0.;
        }
        bh[0] = 0.; bih[0] = 0.;
        return;
    }
    if (ends) cp[0] = (h[0] + h[1]) / h[1];
    for (size_t j = 1; j < last; j++) {
        den[j] = 2. * (ih[j - 1] + ih[j]) - ih[j - 1] * cp[j - 1];
        cp[j] = ih[j] / den[j];
    }
    den[last] = ends ? h[last - 2] - (h[last - 1] + h[last - 2]) * cp[last - 1] : 2. - cp[last - 1];
    cp[last] = 0.;
    for (size_t j = 0; j < n; j++) { bh[j] = h[j]; bih[j] = ih[j]; }
}

// the axis over a block rim_tab_install_axis filled (on the device: over its copy there)
RIM_DEV RimTabAxis rim_tab_axis_of(const double *blk, size_t n, double hu, int grid, int ends = 0)
{
    RimTabAxis a;
    a.cp = blk; a.den = blk + n; a.h = blk + 2 * n; a.ih = blk + 3 * n;
    a.hu = hu; a.n = n; a.grid = grid; a.ends = ends;
    return a;
}

// One line: the slopes of the cubic spline through y_j = src[j * sstride] on the axis, with the axis's ends, into
// slope[j * ostride]; where `val` is not null, the values into val[j * ostride] as well.  src and slope never share a word.
RIM_DEV void rim_tab_install_line(const RimTabAxis &ax, const double *src, size_t sstride, double *val, double *slope, size_t ostride)
{
    const size_t last = ax.n - 1;
    double ym = src[0], yc = src[sstride];          // y[j - 1], y[j] of the step to come
    if (val) val[0] = ym;
    double dp, m;
    if (!ax.grid) {
        const double h = ax.hu;
        if (ax.ends) dp = (5. * ((yc - ym) / h) + (src[2 * sstride] - yc) / h) / 2.;
        else dp = 3. * (yc - ym) / h / 2.;
        slope[0] = dp;
        double yb = ym;                             // y[j - 2] of the last step
        for (size_t j = 1; j <= last; j++) {
            double rhs, yp = 0.;
            if (j < last) {
                yp = src[(j + 1) * sstride];
                rhs = 3. * (yp - ym) / h;
                dp = (rhs - dp) / ax.den[j];
            } else if (ax.ends) {
                rhs = (5. * ((yc - ym) / h) + (ym - yb) / h) / 2.;
                dp = (rhs - 2. * dp) / ax.den[j];
            } else {
                rhs = 3. * (yc - ym) / h;
                dp = (rhs - dp) / ax.den[j];
            }
            slope[j * ostride] = dp;
            if (val) val[j * ostride] = yc;
            yb = ym; ym = yc; yc = yp;
        }
        m = dp;
    } else {
        double sl = (yc - ym) / ax.h[0];            // (y[j] - y[j - 1]) / h[j - 1]
        double sb = sl;                             // (y[j - 1] - y[j - 2]) / h[j - 2] of the last step
        if (ax.ends) {
            const double s1 = (src[2 * sstride] - yc) / ax.h[1], w = ax.h[0] + ax.h[1];
            dp = ((3. * ax.h[0] + 2. * ax.h[1]) * ax.h[1] * sl + ax.h[0] * ax.h[0] * s1) / w / ax.h[1];
        } else {
            dp = 3. * sl / 2.;
        }
        slope[0] = dp;
        for (size_t j = 1; j < last; j++) {
            const double yp = src[(j + 1) * sstride];
            const double sr = (yp - yc) / ax.h[j];
            const double rhs = 3. * (sl * ax.ih[j - 1] + sr * ax.ih[j]);
            dp = (rhs - ax.ih[j - 1] * dp) / ax.den[j];
            slope[j * ostride] = dp;
            if (val) val[j * ostride] = yc;
            ym = yc; yc = yp; sb = sl; sl = sr;
        }
        if (ax.ends) {
            const double hl = ax.h[last - 1], hk = ax.h[last - 2], w = hl + hk;
            const double rhs = ((3. * hl + 2. * hk) * hk * sl + hl * hl * sb) / w;
            m = (rhs - w * dp) / ax.den[last];
        } else {
            m = (3. * sl - dp) / ax.den[last];
        }
        slope[last * ostride] = m;
        if (val) val[last * ostride] = yc;
    }
    for (size_t j = last; j-- > 0;) {
        m = slope[j * ostride] - ax.cp[j] * m;
        slope[j * ostride] = m;
    }
}

// what the three families of a set share: the input, the node data and both axes
struct RimTabInstall {
    const double *log_n;        // [n_tables][n_nodes][n_mu]
    double *nodes;              // [n_tables][n_nodes][n_mu][4] = {S, S_u, S_mu, S_umu}
    size_t n_tables, n_nodes, n_mu;
    RimTabAxis au, amu;
};

// lines of a family: one per (table, mu column) along u, one per (table, gamma row) along mu
RIM_DEV size_t rim_tab_install_lines(const RimTabInstall &s, int family)
{
    return s.n_tables * (family == 1 ? s.n_nodes : s.n_mu);
}

// line `line` (< rim_tab_install_lines) of family 0, 1 or 2
RIM_DEV void rim_tab_install_family_line(const RimTabInstall &s, int family, size_t line)
{
    const size_t per_table = s.n_nodes * s.n_mu;
    if (family == 1) {
        // line = t * n_nodes + i: the row is contiguous in log_n, its nodes 4 words apart
        rim_tab_install_line(s.amu, s.log_n + line * s.n_mu, 1, nullptr, s.nodes + line * s.n_mu * 4 + 2, 4);
        return;
    }
    const size_t t = line / s.n_mu, j = line - t * s.n_mu;
    double *col = s.nodes + (t * per_table + j) * 4;
    if (family == 0) rim_tab_install_line(s.au, s.log_n + t * per_table + j, s.n_mu, col, col + 1, s.n_mu * 4);
    else rim_tab_install_line(s.au, col + 2, s.n_mu * 4, nullptr, col + 3, s.n_mu * 4);
}

#endif
