// tab_spline.h -- host side of the tabulated distribution: checks a table set and lays it out as the kernels read it
// (dev_symphony.h, TAB_HDR_*): a header, then per table and node the value y_j = ln n(gamma_j) and the slope m_j = dy/du
// of the natural cubic spline through the nodes, which are uniform in u = ln gamma.  The slopes are solved here once, in
// fp64: m_{j-1} + 4 m_j + m_{j+1} = 3 (y_{j+1} - y_{j-1}) / h inside, 2 m_0 + m_1 = 3 (y_1 - y_0) / h and its mirror at the
// ends (second derivative 0 there).  A straight line in (u, y) -- a pure power law -- comes back as itself.
//
// Plain C++ with the elementary functions of detmath.h, so that the library (hipcc's host pass) and the tests' table
// oracle (g++) produce the same bits from the same table.
#ifndef RIM_TAB_SPLINE_H
#define RIM_TAB_SPLINE_H

#include <cstddef>
#include <vector>
#include "dev_symphony.h"

#define RIM_TAB_MIN_NODES 8
#define RIM_TAB_MAX_NODES 65536

// 0, or -1 for bad geometry or a non-finite value
inline int rim_tab_check(size_t n_tables, size_t n_nodes, double gamma_lo, double gamma_hi, const double *log_n)
{
    if (n_tables < 1 || n_nodes < RIM_TAB_MIN_NODES || n_nodes > RIM_TAB_MAX_NODES || !log_n) return -1;
    if (n_tables > ((size_t) 1 << 40) / n_nodes) return -1;
    if (!rim_isfinite(gamma_lo) || !rim_isfinite(gamma_hi) || !(gamma_lo >= 1.) || !(gamma_lo < gamma_hi)) return -1;
    for (size_t i = 0; i < n_tables * n_nodes; i++)
        if (!rim_isfinite(log_n[i])) return -1;
    return 0;
}

// the table set as one block of doubles; rim_tab_check() has passed
inline void rim_tab_build(size_t n_tables, size_t n_nodes, double gamma_lo, double gamma_hi, const double *log_n,
                          std::vector<double> &blob)
{
    using namespace rim;
    const double u_lo = rim_log(gamma_lo), u_hi = rim_log(gamma_hi);
    const double h = (u_hi - u_lo) / (double) (n_nodes - 1);
    blob.assign((size_t) TAB_HDR_DOUBLES + n_tables * n_nodes * 2, 0.);
    blob[TAB_HDR_NTABLES] = (double) n_tables;
    blob[TAB_HDR_NNODES] = (double) n_nodes;
    blob[TAB_HDR_GLO] = gamma_lo;
    blob[TAB_HDR_GHI] = gamma_hi;
    blob[TAB_HDR_ULO] = u_lo;
    blob[TAB_HDR_INVH] = 1. / h;
    blob[TAB_HDR_H] = h;
    std::vector<double> cp(n_nodes), dp(n_nodes);       // Thomas algorithm: the swept upper diagonal and right-hand side
    for (size_t t = 0; t < n_tables; t++) {
        const double *y = log_n + t * n_nodes;
        double *row = blob.data() + TAB_HDR_DOUBLES + t * n_nodes * 2;
        const size_t last = n_nodes - 1;
        cp[0] = 0.5;
        dp[0] = 3. * (y[1] - y[0]) / h / 2.;
        for (size_t j = 1; j <= last; j++) {
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
}

#endif
