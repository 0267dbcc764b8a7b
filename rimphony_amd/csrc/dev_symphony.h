// dev_symphony.h -- per-sample device functions of the Symphony path:
// the distribution functions (four analytic ones and the tabulated one) and gamma_integrand.
//
//   DistributionFunction::calc_f / calc_f_derivatives
//       power_law.rs:36-62, thermal_juettner.rs:29-39, pitchy_pl.rs:32-64,
//       pitchy_kappa.rs:38-62
//   CalculationState::gamma_integrand      symphony.rs:398-479
//
// The reference reaches these through a GSL callback trampoline per sample
// (gsl.rs:111-117); here they are inlined into the wavefront quadrature, one
// sample per lane.  Operation order matches oracle/rimo_dist.c and
// oracle/rimo_symphony.c exactly (bit-for-bit parity is tested).
#ifndef RIM_DEV_SYMPHONY_H
#define RIM_DEV_SYMPHONY_H

#include <stddef.h>
#include "dev_bessel.h"

namespace rim {

enum { DIST_POWER_LAW = 0, DIST_THERMAL_JUETTNER = 1, DIST_PITCHY_PL = 2, DIST_PITCHY_KAPPA = 3, DIST_TABULATED = 4,
       // not a kind of the C ABI: the tabulated kind where the table set is KNOWN to have no pitch rows, so that the test for
       // one and everything behind it leave the code.  Same values as DIST_TABULATED on such a set, bit for bit; the two
       // persistent kernels are instantiated for it (rimphony_tab.hip), so that isotropic tables run the code they always ran.
       DIST_TABULATED_ISO = 5,
       // nor is this one: the tabulated kind where the set is a 2-D one, ln n(gamma, mu) on a grid (rim_tab_build_2d).  The host
       // chooses it by the form of the installed set; a row is still RIMPHONY_TABULATED with a table index.
       DIST_TABULATED_2D = 6,
       // nor this one: the tabulated kind where every table carries a sin^k xi prefactor (rim_tab_build_pitchy), with or
       // without a pitch row.  Chosen by the host in the same way.
       DIST_TABULATED_PITCHY = 7,
       // nor this one: the tabulated kind where the gamma nodes of the set are given, not uniform in ln gamma
       // (rim_tab_build_grid); it carries a sin^k prefactor and a pitch row as DIST_TABULATED_PITCHY does.
       DIST_TABULATED_GRID = 8,
       // nor this one: the tabulated kind where the set is a 2-D one on given gamma nodes (rim_tab_build_2d_grid): the surface
       // of DIST_TABULATED_2D, the lookup of DIST_TABULATED_GRID.
       DIST_TABULATED_2D_GRID = 9,
       // nor these two: the 2-D forms where every table carries a sin^k xi prefactor (rim_tab_build_2d with sin_k), k a word
       // of the table's header (TAB_2D_K): f = norm sin^k xi exp(S) / (gamma^2 beta).  The surface and the lookup of
       // DIST_TABULATED_2D and of DIST_TABULATED_2D_GRID; those two keep the code they always ran.
       DIST_TABULATED_2D_PITCHY = 10, DIST_TABULATED_2D_GRID_PITCHY = 11,
       // nor these two: the 2-D form on gamma nodes AND mu nodes of the caller's choosing (rim_tab_build_2d_nodes), without
       // and with a sin^k xi prefactor.  The surface of the other 2-D forms, the gamma lookup of DIST_TABULATED_2D_GRID and the
       // same kind of lookup along mu (tab_2d_nodes_mu_interval); the older forms keep the code they always ran.
       DIST_TABULATED_2D_NODES = 12, DIST_TABULATED_2D_NODES_PITCHY = 13,
       // nor these two: the tabulated kind where the set is a FAMILY (rim_tab_build_family): energy tables on nodes uniform in
       // ln gamma, without and with a sin^k xi prefactor per table, and a row's parameter a REAL index x into them.  A sample
       // blends the node words of tables a = floor(x) and a + 1 with the weight w = x - a and evaluates one cubic
       // (tab_spline_family); with a prefactor k is blended likewise.  The older forms keep the code they always ran.
       DIST_TABULATED_FAMILY = 14, DIST_TABULATED_FAMILY_PITCHY = 15,
       // nor these two: a FAMILY of 2-D surfaces on given gamma and mu nodes (rim_tab_build_2d_family), without and with a
       // sin^k xi prefactor per table.  The set and the lookup of DIST_TABULATED_2D_NODES; a row's parameter is a real index x
       // as in the families above, and a sample blends the sixteen node words of its cell from tables a = floor(x) and a + 1
       // and evaluates one bicubic (tab_bicubic_family).  The older forms keep the code they always ran.
       DIST_TABULATED_2D_FAMILY = 16, DIST_TABULATED_2D_FAMILY_PITCHY = 17,
       // nor these two: the same family blended CUBICALLY across its tables (rim_tab_build_2d_family_cubic), without and with a
       // sin^k xi prefactor per table.  The set of DIST_TABULATED_2D_FAMILY followed by one knot word per table; a sample blends
       // the sixteen node words of its cell from FOUR neighbouring tables with the Lagrange weights of the row's line
       // (tab_2d_family_cubic_line) and evaluates one bicubic (tab_bicubic_family_cubic).  The linear forms keep their code.
       DIST_TABULATED_2D_FAMILY_CUBIC = 18, DIST_TABULATED_2D_FAMILY_CUBIC_PITCHY = 19 };
constexpr bool tab_kind_family(int kind) { return kind == DIST_TABULATED_FAMILY || kind == DIST_TABULATED_FAMILY_PITCHY; }
constexpr bool tab_kind_2d_family_cubic(int kind)
{
    return kind == DIST_TABULATED_2D_FAMILY_CUBIC || kind == DIST_TABULATED_2D_FAMILY_CUBIC_PITCHY;
}
// (a family of 2-D surfaces under either blending rule: what the two rules share -- the set, the index rule, the per-row
// normalisation -- asks this; what they do not asks tab_kind_2d_family_cubic)
constexpr bool tab_kind_2d_family(int kind)
{
    return kind == DIST_TABULATED_2D_FAMILY || kind == DIST_TABULATED_2D_FAMILY_PITCHY || tab_kind_2d_family_cubic(kind);
}
constexpr bool dist_is_tab(int kind)
{
    return kind == DIST_TABULATED || kind == DIST_TABULATED_ISO || kind == DIST_TABULATED_2D || kind == DIST_TABULATED_PITCHY ||
        kind == DIST_TABULATED_GRID || kind == DIST_TABULATED_2D_GRID || kind == DIST_TABULATED_2D_PITCHY ||
        kind == DIST_TABULATED_2D_GRID_PITCHY || kind == DIST_TABULATED_2D_NODES || kind == DIST_TABULATED_2D_NODES_PITCHY ||
        tab_kind_family(kind) || tab_kind_2d_family(kind);
}
// the 2-D forms: on nodes uniform in ln gamma, on given gamma nodes (mu uniform), on given gamma and mu nodes, and which of
// them carry a sin^k prefactor
constexpr bool tab_kind_2d_uniform(int kind) { return kind == DIST_TABULATED_2D || kind == DIST_TABULATED_2D_PITCHY; }
constexpr bool tab_kind_2d_on_grid(int kind) { return kind == DIST_TABULATED_2D_GRID || kind == DIST_TABULATED_2D_GRID_PITCHY; }
constexpr bool tab_kind_2d_nodes(int kind) { return kind == DIST_TABULATED_2D_NODES || kind == DIST_TABULATED_2D_NODES_PITCHY; }
constexpr bool tab_kind_2d_pitchy(int kind)
{
    return kind == DIST_TABULATED_2D_PITCHY || kind == DIST_TABULATED_2D_GRID_PITCHY || kind == DIST_TABULATED_2D_NODES_PITCHY ||
        kind == DIST_TABULATED_2D_FAMILY_PITCHY || kind == DIST_TABULATED_2D_FAMILY_CUBIC_PITCHY;
}
enum { STOKES_I = 0, STOKES_Q = 1, STOKES_V = 2 };
enum { COEFF_EMISSION = 0, COEFF_ABSORPTION = 1, COEFF_FARADAY = 2 };

// Distribution parameters of one point (wave-uniform).  par[] follows the C ABI:
//   power_law {p, gmin, gmax, gcut}; thermal {T}; pitchy_pl {p, k, gmin, gmax, gcut};
//   pitchy_kappa {kappa, width, k, gcut}; tabulated {table index} (the other fields: dist_prepare<DIST_TABULATED>, which
//   also replaces the index by the address of the table's pitch row).
struct DistParams {
    double par[5];
    double inv_gamma_cutoff;
    double inv_kappa_width;
    double neg_inverse_t;
    double norm;
};

// ---- tabulated distribution: a table set in memory (rim_tab_build of tab_spline.h lays it out) ----
// TAB_HDR_DOUBLES header words, then [n_tables][n_nodes][2] = {y_j = ln n(gamma_j), m_j = dy/du at the node} of the natural
// cubic spline in u = ln gamma; the nodes are uniform in u.  A set with a pitch-angle factor g(mu), mu = cos xi, says so in
// TAB_HDR_NMU (0: isotropic, nothing follows) and appends one pitch row per table: TAB_PITCH_HDR words {n_mu - 2, 1 / h_mu,
// h_mu, P = 1/2 int g dmu}, then [n_mu][2] = {G_j = ln g(mu_j), M_j = dG/dmu at the node} of the natural cubic spline in mu;
// the nodes are uniform in mu from -1 to +1.
enum { TAB_HDR_NTABLES = 0, TAB_HDR_NNODES = 1, TAB_HDR_GLO = 2, TAB_HDR_GHI = 3, TAB_HDR_ULO = 4, TAB_HDR_INVH = 5, TAB_HDR_H = 6,
       TAB_HDR_NMU = 7, TAB_HDR_DOUBLES = 8 };
enum { TAB_PITCH_LAST = 0, TAB_PITCH_INVH = 1, TAB_PITCH_H = 2, TAB_PITCH_P = 3, TAB_PITCH_HDR = 4 };
// A 2-D set, ln n(gamma, mu) on a grid (rim_tab_build_2d), marks itself by a NEGATIVE TAB_HDR_NMU, -n_mu.  After the header
// come n_tables table headers of TAB_2D_HDR words {n_mu - 2, 1 / h_mu, h_mu, the table's normalisation, four spare words: a
// table header is one 64-byte line and the node data stay aligned to one}, then [n_tables][n_nodes][n_mu][4] =
// {S, S_u, S_mu, S_umu} of the tensor-product natural cubic spline S(u, mu) at the node, mu fastest: the nodes (i, j) and
// (i, j + 1) are 64 contiguous bytes and a sample reads two such runs.  A set with a sin^k xi prefactor keeps the table's k
// in the first of the spare words, TAB_2D_K (0 as built without one: only the kinds with a prefactor read it).  A set on
// given mu nodes (tab_2d_nodes_* below) uses two more, TAB_2D_MU_GUIDE and TAB_2D_MU_NODES.  The last one, TAB_2D_ENDS, records
// how the spline was solved -- ends_u + 2 ends_mu, each 0 for natural ends and 1 for not-a-knot ends (tab_spline.h) -- for
// whoever reads a set back: no kernel reads it.
enum { TAB_2D_LAST = 0, TAB_2D_INVH = 1, TAB_2D_H = 2, TAB_2D_NORM = 3, TAB_2D_K = 4, TAB_2D_MU_GUIDE = 5, TAB_2D_MU_NODES = 6,
       TAB_2D_ENDS = 7, TAB_2D_HDR = 8 };
RIM_DEV bool tab_set_is_2d(const double *hdr) { return hdr[TAB_HDR_NMU] < 0.; }
// A set with a sin^k xi prefactor (rim_tab_build_pitchy): header and gamma rows as ever, TAB_HDR_NMU = n_mu (0: no g), then
// per table TAB_PITCHY_PRE words {k, n_mu, two spare} and, straight behind them, what a pitch row is: TAB_PITCH_HDR words
// {n_mu - 2, 1 / h_mu, h_mu, P = 1/2 int (1 - mu^2)^(k/2) g dmu} and, where there is a g, [n_mu][2] = {G_j, M_j}.  A row
// carries the address of the pitch-row part, so tab_pitch_spline serves it as it is; k and n_mu sit at negative offsets
// from there.  A table header is one 64-byte line.
enum { TAB_PITCHY_PRE = 4, TAB_PITCHY_K = -4, TAB_PITCHY_NMU = -3 };
// A set on given gamma nodes (rim_tab_build_grid): the header with TAB_HDR_ULO = u_0 = ln gamma_0, TAB_HDR_INVH = 1 / (the
// width of a guide cell), TAB_HDR_H = G, the number of guide cells (a power of two >= n_nodes), TAB_HDR_NMU = n_mu.  Then
// the guide, G + 1 32-bit words padded to a multiple of 64 bytes (tab_grid_guide_doubles): the cells are uniform in u over
// [u_0, u_last], a u belongs to the cell tab_grid_cell() says, and word c holds min(the index of the last node in a cell
// below c, n_nodes - 2) -- 0 where there is none --, so that the interval of a sample lies between words c and c + 1 of its
// cell.  Then [n_tables][n_nodes][4] = {u_j, y_j, m_j, 1 / h_j} (h_j = u_{j+1} - u_j; 0 at the last node): the two nodes of
// an interval are 64 contiguous bytes.  Then what follows the gamma rows of a sin^k set, with a header of its own in front:
// TAB_HDR_DOUBLES words {n_tables, 0, gamma_0, gamma_last, 0, 0, 0, n_mu} and per table {k, n_mu, two spare}, the pitch
// row's header and, where there is a g, its nodes.  Read as a set of no gamma nodes, that tail is a sin^k set's:
// tab_pitchy_table_p_kernel integrates P into it as it stands.
RIM_DEV size_t tab_grid_guide_doubles(size_t cells) { return ((cells + 2) / 2 + 7) & ~(size_t) 7; }
RIM_DEV size_t tab_grid_tail(size_t n_tables, size_t n_nodes, size_t cells)
{
    return (size_t) TAB_HDR_DOUBLES + tab_grid_guide_doubles(cells) + n_tables * n_nodes * 4;
}
// the guide cell of u: u0 = u_0, inv_cell = 1 / (cell width), last_cell = G - 1.  Monotone in u, and formed from a clamped
// copy: a NaN belongs to cell 0.  The host fills the guide with this very function, so a rounding in it moves a node and
// the samples around it together.
RIM_DEV long long tab_grid_cell(double u, double u0, double inv_cell, double last_cell)
{
    double xc = (u - u0) * inv_cell;
    if (!(xc >= 0.)) xc = 0.;
    if (xc > last_cell) xc = last_cell;
    return (long long) xc;
}

// A 2-D set on given gamma nodes (rim_tab_build_2d_grid): the header of a set on given nodes -- TAB_HDR_ULO = u_0, TAB_HDR_INVH
// = 1 / (the width of a guide cell), TAB_HDR_H = G, the number of guide cells -- with TAB_HDR_NMU = -n_mu as a 2-D set has it.
// Then, where a 2-D set has them, n_tables table headers of TAB_2D_HDR words (the mu geometry and the table's normalisation
// in TAB_2D_NORM: tab2d_row_norm_kernel reads either form).  Then the guide of a set on given nodes, G + 1 32-bit words padded
// to a multiple of 64 bytes, and straight behind it the u nodes of the set, [n_nodes][2] = {u_i, 1 / h_i} (h_i = u_{i+1} - u_i;
// 0 at the last node), padded likewise (tab_2d_grid_unode_doubles): a row carries the address of the guide and that of the u
// nodes, whose first word is u_0.  Then [n_tables][n_nodes][n_mu][4] = {S, S_u, S_mu, S_umu}, mu fastest, as in a 2-D set.
RIM_DEV size_t tab_2d_grid_unode_doubles(size_t n_nodes) { return (2 * n_nodes + 7) & ~(size_t) 7; }
RIM_DEV size_t tab_2d_grid_guide_at(size_t n_tables) { return (size_t) TAB_HDR_DOUBLES + n_tables * TAB_2D_HDR; }
RIM_DEV size_t tab_2d_grid_nodes_at(size_t n_tables, size_t n_nodes, size_t cells)
{
    return tab_2d_grid_guide_at(n_tables) + tab_grid_guide_doubles(cells) + tab_2d_grid_unode_doubles(n_nodes);
}

// A 2-D set on given gamma nodes and given mu nodes (rim_tab_build_2d_nodes): the layout of a 2-D set on given gamma nodes up
// to and including the u nodes.  Then, where that form's node data begin, the mu guide -- M + 1 32-bit words padded to a
// multiple of 64 bytes, M the smallest power of two >= n_mu (at least 8), the guide cells uniform in mu over [-1, +1], filled
// and read as the u guide is (tab_grid_cell with u_0 = -1) -- and straight behind it the mu nodes of the set, [n_mu][2] =
// {mu_j, 1 / h_j} (h_j = mu_{j+1} - mu_j; 0 at the last node), padded likewise.  Then [n_tables][n_nodes][n_mu][4] as in every
// 2-D set.  A table header says TAB_2D_LAST = n_mu - 2 as ever, TAB_2D_INVH = 1 / (the width of a mu guide cell) = M / 2,
// TAB_2D_H = M, and in TAB_2D_MU_GUIDE / TAB_2D_MU_NODES the distance in doubles from the header itself to the mu guide and
// to the mu nodes: a row carries the address of its table's header and needs no further field.
RIM_DEV size_t tab_2d_nodes_munode_doubles(size_t n_mu) { return (2 * n_mu + 7) & ~(size_t) 7; }
RIM_DEV size_t tab_2d_nodes_mu_guide_at(size_t n_tables, size_t n_nodes, size_t cells)
{
    return tab_2d_grid_nodes_at(n_tables, n_nodes, cells);
}
RIM_DEV size_t tab_2d_nodes_nodes_at(size_t n_tables, size_t n_nodes, size_t cells, size_t n_mu, size_t mu_cells)
{
    return tab_2d_nodes_mu_guide_at(n_tables, n_nodes, cells) + tab_grid_guide_doubles(mu_cells) + tab_2d_nodes_munode_doubles(n_mu);
}
// (the tests' oracle counts the node words a mu search reads: RIM_TAB_2D_NODES_COUNT names its counter)
#if defined(RIM_TAB_2D_NODES_COUNT)
#define RIM_TAB_2D_NODES_READ() ((void) ++RIM_TAB_2D_NODES_COUNT)
#else
#define RIM_TAB_2D_NODES_READ() ((void) 0)
#endif

// is `idx` (par[0] of a row) the index of a table of the set?
RIM_DEV bool tab_row_ok(const double *hdr, double idx)
{
    return idx >= 0. && idx < hdr[TAB_HDR_NTABLES] && (double) (long long) idx == idx;
}

// A family (rim_tab_build_family): the header of an isotropic set, TAB_HDR_NTABLES = n_tables, then n_tables + 1 gamma rows
// of [n_nodes][2] = {y_j, m_j} -- the last one a copy of the row before it, so that the row "one further on" of every table
// exists and a sample never asks whether it does --, then, where the set has a sin^k xi prefactor, one header of TAB_PITCHY_PRE
// + TAB_PITCH_HDR words per table as a sin^k set without g has them: {k, 0, two spare | three spare, P(k)}.
// The index rule of a row: x finite with 0 <= x <= n_tables - 1 (-0.0 counts as 0), a = (long long) x, w = x - a; anything
// else names no table.  `a` is 0 and w is 0 for such a row, so that every read stays inside the set.
RIM_DEV bool tab_family_row(const double *hdr, double x, size_t &a, double &w)
{
    const bool ok = x >= 0. && x <= hdr[TAB_HDR_NTABLES] - 1.;
    a = ok ? (size_t) (long long) x : 0;
    w = ok ? x - (double) a : 0.;
    return ok;
}
RIM_DEV const double *tab_family_k_headers(const double *hdr)
{
    return hdr + TAB_HDR_DOUBLES + ((size_t) hdr[TAB_HDR_NTABLES] + 1) * (size_t) hdr[TAB_HDR_NNODES] * 2;
}
// k of a row of a family with a prefactor: k_a + w (k_b - k_a), b = a + 1 or, at the last table, a
RIM_DEV double tab_family_k(const double *hdr, size_t a, double w)
{
    const double *kh = tab_family_k_headers(hdr);
    const size_t b = a + 1 < (size_t) hdr[TAB_HDR_NTABLES] ? a + 1 : a;
    const double ka = kh[a * (TAB_PITCHY_PRE + TAB_PITCH_HDR)], kb = kh[b * (TAB_PITCHY_PRE + TAB_PITCH_HDR)];
    return rim_fma(w, kb - ka, ka);
}
// The 64-byte line of a batch row of such a family, laid out as the header of a sin^k table without g, so that what reads
// TAB_PITCHY_K and TAB_PITCH_P from a table's header reads them from here: {k, 0, w, spare | 0, 0, 0, P}.  par[0] of the
// row names word TAB_PITCHY_PRE of it; w sits where a table's header has a spare word.
enum { TAB_FAMILY_LINE = TAB_PITCHY_PRE + TAB_PITCH_HDR, TAB_FAMILY_W = -2 };
RIM_DEV void tab_family_line(double *line, double k, double w, double pa)
{
    line[0] = k; line[1] = 0.; line[2] = w; line[3] = 0.;
    line[4] = 0.; line[5] = 0.; line[6] = 0.; line[7] = pa;
}

// A family of 2-D surfaces (rim_tab_build_2d_family): the set of rim_tab_build_2d_nodes word for word -- header, table headers,
// both guides, both node arrays, [n_tables][n_nodes][n_mu][4] node data, no trailing copy -- with TAB_2D_NORM of every table
// header a NaN: nothing is integrated at install.  The index rule of a row is tab_family_row's.  Every batch row has a
// 64-byte line, laid out as a table header, so that what reads a table's header reads the line:
//   TAB_2D_LAST, TAB_2D_INVH, TAB_2D_H   the mu geometry of the set (the same in every table header);
//   TAB_2D_NORM                          the weight w (a row's normalisation travels in d.norm);
//   TAB_2D_K                             k_a + w (k_b - k_a), b = a + 1 or, at the last table, a (0 without a prefactor);
//   TAB_2D_MU_GUIDE, TAB_2D_MU_NODES     the distance in doubles from THE LINE to the set's mu guide and mu nodes;
//   TAB_2D_ENDS                          the distance in doubles from the node data of table a to those of table b: one
//                                        table's worth, or 0 at the last table.
// par[0] of a prepared row names the line.  A row whose index names no table gets a = 0, w = 0: every read stays inside the set.
RIM_DEV double tab_family_blend(double w, double qa, double qb) { return rim_fma(w, qb - qa, qa); }
RIM_DEV void tab_2d_family_line(double *line, const double *hdr, size_t a, double w)
{
    const size_t nt = (size_t) hdr[TAB_HDR_NTABLES], nn = (size_t) hdr[TAB_HDR_NNODES], nmu = (size_t) -hdr[TAB_HDR_NMU];
    const size_t b = a + 1 < nt ? a + 1 : a;
    const double *tha = hdr + TAB_HDR_DOUBLES + a * TAB_2D_HDR, *thb = hdr + TAB_HDR_DOUBLES + b * TAB_2D_HDR;
    const long long to_set = ((long long) (uintptr_t) tha - (long long) (uintptr_t) line) / (long long) sizeof(double);
    line[TAB_2D_LAST] = tha[TAB_2D_LAST];
    line[TAB_2D_INVH] = tha[TAB_2D_INVH];
    line[TAB_2D_H] = tha[TAB_2D_H];
    line[TAB_2D_NORM] = w;
    line[TAB_2D_K] = tab_family_blend(w, tha[TAB_2D_K], thb[TAB_2D_K]);
    line[TAB_2D_MU_GUIDE] = (double) (to_set + (long long) tha[TAB_2D_MU_GUIDE]);
    line[TAB_2D_MU_NODES] = (double) (to_set + (long long) tha[TAB_2D_MU_NODES]);
    line[TAB_2D_ENDS] = (double) ((b - a) * nn * nmu * 4);
}

// The same family blended CUBICALLY across its tables (rim_tab_build_2d_family_cubic): the set above word for word, followed
// by n_tables >= 4 knot words c_t, finite and strictly monotonic -- the parameter the tables are spaced in.  The index rule of
// a row stays tab_family_row's.  Every batch row has a line of TAB_2D_CUBIC_LINE words (128 bytes): the eight words of the
// line above, then the four Lagrange weights, the base table of the stencil and the row's parameter p.  Of the first eight,
//   TAB_2D_K        is fma(L_3, k_3, fma(L_2, k_2, fma(L_1, k_1, L_0 k_0))) over the stencil's tables (0 without a prefactor);
//   TAB_2D_ENDS     the distance in doubles between the node data of neighbouring tables: always one table's worth;
// the others are as above (TAB_2D_NORM keeps w, for whoever reads a line back).  The rule, whose order defines the bits:
//   p    = fma(w, c_b - c_a, c_a), b = a + 1 or, at the last table, a: at an integer x a knot, bit for bit;
//   s    = min(max(a - 1, 0), n_tables - 4), the stencil is tables s .. s + 3;
//   L_i  = prod over j != i, j ascending, starting from 1, of (p - c_{s+j}) / (c_{s+i} - c_{s+j}): at a knot exactly 1 for
//          that knot's table and a zero for the others.
// A row whose index names no table gets a = 0, w = 0, so s = 0 and p = c_0: every read stays inside the set.
enum { TAB_2D_CUBIC_L = TAB_2D_HDR, TAB_2D_CUBIC_BASE = TAB_2D_HDR + 4, TAB_2D_CUBIC_P = TAB_2D_HDR + 5, TAB_2D_CUBIC_LINE = 16 };
RIM_DEV size_t tab_2d_family_cubic_base(size_t nt, size_t a) { const size_t s = a > 0 ? a - 1 : 0; return s + 4 > nt ? nt - 4 : s; }
RIM_DEV double tab_family_blend4(const double *l, double q0, double q1, double q2, double q3)
{
    return rim_fma(l[3], q3, rim_fma(l[2], q2, rim_fma(l[1], q1, l[0] * q0)));
}
// the knot words of such a set: straight behind the node data
RIM_DEV const double *tab_2d_family_cubic_knots(const double *hdr)
{
    const size_t nt = (size_t) hdr[TAB_HDR_NTABLES], nn = (size_t) hdr[TAB_HDR_NNODES], cells = (size_t) hdr[TAB_HDR_H];
    const size_t nmu = (size_t) -hdr[TAB_HDR_NMU];
    return hdr + tab_2d_nodes_nodes_at(nt, nn, cells, nmu, (size_t) hdr[TAB_HDR_DOUBLES + TAB_2D_H]) + nt * nn * nmu * 4;
}
RIM_DEV void tab_2d_family_cubic_line(double *line, const double *hdr, size_t a, double w)
{
    const size_t nt = (size_t) hdr[TAB_HDR_NTABLES], nn = (size_t) hdr[TAB_HDR_NNODES], nmu = (size_t) -hdr[TAB_HDR_NMU];
    const size_t b = a + 1 < nt ? a + 1 : a;
    const size_t s = tab_2d_family_cubic_base(nt, a);
    const double *c = tab_2d_family_cubic_knots(hdr);
    const double *th = hdr + TAB_HDR_DOUBLES + s * TAB_2D_HDR;
    const long long to_set = ((long long) (uintptr_t) th - (long long) (uintptr_t) line) / (long long) sizeof(double);
    const double p = rim_fma(w, c[b] - c[a], c[a]);
    double *l = line + TAB_2D_CUBIC_L;
    for (int i = 0; i < 4; i++) {
        double v = 1.;
        for (int j = 0; j < 4; j++)
            if (j != i) v = v * ((p - c[s + j]) / (c[s + i] - c[s + j]));
        l[i] = v;
    }
    line[TAB_2D_LAST] = th[TAB_2D_LAST];
    line[TAB_2D_INVH] = th[TAB_2D_INVH];
    line[TAB_2D_H] = th[TAB_2D_H];
    line[TAB_2D_NORM] = w;
    line[TAB_2D_K] = tab_family_blend4(l, th[TAB_2D_K], th[TAB_2D_HDR + TAB_2D_K], th[2 * TAB_2D_HDR + TAB_2D_K],
                                       th[3 * TAB_2D_HDR + TAB_2D_K]);
    line[TAB_2D_MU_GUIDE] = (double) (to_set + (long long) th[TAB_2D_MU_GUIDE]);
    line[TAB_2D_MU_NODES] = (double) (to_set + (long long) th[TAB_2D_MU_NODES]);
    line[TAB_2D_ENDS] = (double) (nn * nmu * 4);
    line[TAB_2D_CUBIC_BASE] = (double) s;
    line[TAB_2D_CUBIC_P] = p;
    line[TAB_2D_CUBIC_P + 1] = 0.; line[TAB_2D_CUBIC_P + 2] = 0.;
}
// is the blended k of a row's line an exponent the prefactor takes?  A cubic may overshoot between knots; such a row is a NaN
// row (norm_kernel and the tests' oracle ask this).  Without a prefactor the word is 0.
RIM_DEV bool tab_2d_family_cubic_k_ok(const double *line) { return line[TAB_2D_K] >= 0. && line[TAB_2D_K] <= 100.; }

template <int KIND>
RIM_DEV void dist_prepare(DistParams &d, double norm)
{
    if (tab_kind_2d_family(KIND)) {
        // In: par[0] the real index x, par[1] the bit pattern of the set's address, par[2] that of the row's line
        // (tab_2d_family_line).  Out: what a row of a 2-D set on given nodes carries, with the line where the table's header
        // is: par[0] the line, par[1] the node data of table a -- those of table b lie line[TAB_2D_ENDS] doubles further on --,
        // par[2] the set's u nodes, par[3] 1 / (cell width), par[4] the index of the last guide cell, inv_gamma_cutoff the
        // guide's address.  DistParams does not grow.  (The cubic blend: par[2] names a line of tab_2d_family_cubic_line, and
        // par[1] the node data of the stencil's base table.)
        const double *hdr = (const double *) (uintptr_t) rim_bits(d.par[1]);
        size_t a;
        double w;
        const bool ok = tab_family_row(hdr, d.par[0], a, w);
        const size_t nt = (size_t) hdr[TAB_HDR_NTABLES], nn = (size_t) hdr[TAB_HDR_NNODES], cells = (size_t) hdr[TAB_HDR_H];
        const size_t nmu = (size_t) -hdr[TAB_HDR_NMU];
        const double *guide = hdr + tab_2d_grid_guide_at(nt);
        const size_t at = tab_2d_nodes_nodes_at(nt, nn, cells, nmu, (size_t) hdr[TAB_HDR_DOUBLES + TAB_2D_H]);
        d.par[0] = d.par[2];
        const size_t first = tab_kind_2d_family_cubic(KIND) ? tab_2d_family_cubic_base(nt, a) : a;
        d.par[1] = rim_frombits((uint64_t) (uintptr_t) (hdr + at + first * nn * nmu * 4));
        d.par[2] = rim_frombits((uint64_t) (uintptr_t) (guide + tab_grid_guide_doubles(cells)));
        d.par[3] = hdr[TAB_HDR_INVH];
        d.par[4] = hdr[TAB_HDR_H] - 1.;
        d.inv_gamma_cutoff = rim_frombits((uint64_t) (uintptr_t) guide);
        d.inv_kappa_width = hdr[TAB_HDR_GLO];
        d.neg_inverse_t = hdr[TAB_HDR_GHI];
        d.norm = ok ? norm : RIM_NAN;
        return;
    }
    if (tab_kind_family(KIND)) {
        // In: par[0] the real index x, par[1] the bit pattern of the set's address and, with a prefactor, par[2] that of the
        // row's line (tab_family_line).  Out: what an isotropic row carries, par[1] the address of row a -- row b is the
        // next one, (par[4] + 2) * 2 doubles further on -- and par[0] the weight w itself or, with a prefactor, the address
        // of the line's pitch-row part, where w is word TAB_FAMILY_W.  DistParams does not grow.
        const double *hdr = (const double *) (uintptr_t) rim_bits(d.par[1]);
        size_t a;
        double w;
        const bool ok = tab_family_row(hdr, d.par[0], a, w);
        const size_t nn = (size_t) hdr[TAB_HDR_NNODES];
        if (KIND == DIST_TABULATED_FAMILY_PITCHY)
            d.par[0] = rim_frombits((uint64_t) (uintptr_t) ((const double *) (uintptr_t) rim_bits(d.par[2]) + TAB_PITCHY_PRE));
        else d.par[0] = w;
        d.par[1] = rim_frombits((uint64_t) (uintptr_t) (hdr + TAB_HDR_DOUBLES + a * nn * 2));
        d.par[2] = hdr[TAB_HDR_ULO];
        d.par[3] = hdr[TAB_HDR_INVH];
        d.par[4] = hdr[TAB_HDR_NNODES] - 2.;           // the index of the last interval
        d.inv_gamma_cutoff = hdr[TAB_HDR_H];
        d.inv_kappa_width = hdr[TAB_HDR_GLO];
        d.neg_inverse_t = hdr[TAB_HDR_GHI];
        d.norm = ok ? norm : RIM_NAN;
        return;
    }
    if (dist_is_tab(KIND)) {
        // In: par[0] the table index, par[1] the bit pattern of the table set's address.  The kind has one parameter, so the
        // fields the others use carry what a sample needs (DistParams does not grow): par[1] the bit pattern of the row's
        // address, par[2] u_lo, par[3] 1 / h, par[4] the index of the last interval; inv_gamma_cutoff h, inv_kappa_width
        // gamma_lo, neg_inverse_t gamma_hi.  A row whose index names no table keeps table 0 (every read stays inside the
        // set) and gets a NaN normalisation.  Out: par[0], no longer needed once the row is found, is the bit pattern of
        // the address of the table's pitch row, or +0 for a set without pitch rows (isotropic).
        const double *hdr = (const double *) (uintptr_t) rim_bits(d.par[1]);
        const bool ok = tab_row_ok(hdr, d.par[0]);
        const size_t nn = (size_t) hdr[TAB_HDR_NNODES];
        const size_t row = ok ? (size_t) d.par[0] : 0;
        if (tab_kind_2d_uniform(KIND)) {
            // a 2-D set: par[0] the address of the table's header (the mu geometry, as a pitch row's), par[1] that of its
            // node data; the rest as for the other two forms
            const size_t nt = (size_t) hdr[TAB_HDR_NTABLES], nmu2 = (size_t) -hdr[TAB_HDR_NMU];
            d.par[0] = rim_frombits((uint64_t) (uintptr_t) (hdr + TAB_HDR_DOUBLES + row * TAB_2D_HDR));
            d.par[1] = rim_frombits((uint64_t) (uintptr_t) (hdr + TAB_HDR_DOUBLES + nt * TAB_2D_HDR + row * nn * nmu2 * 4));
            d.par[2] = hdr[TAB_HDR_ULO];
            d.par[3] = hdr[TAB_HDR_INVH];
            d.par[4] = hdr[TAB_HDR_NNODES] - 2.;        // the index of the last interval in u
            d.inv_gamma_cutoff = hdr[TAB_HDR_H];
            d.inv_kappa_width = hdr[TAB_HDR_GLO];
            d.neg_inverse_t = hdr[TAB_HDR_GHI];
            d.norm = ok ? norm : RIM_NAN;
            return;
        }
        if (tab_kind_2d_on_grid(KIND) || tab_kind_2d_nodes(KIND)) {
            // a 2-D set on given nodes: par[0] the table's header and par[1] its node data, as for a 2-D set; par[2] the
            // address of the set's u nodes (u_0 is their first word), par[3] 1 / (cell width), par[4] the index of the last
            // guide cell; inv_gamma_cutoff the bit pattern of the guide's address, as for a set on given nodes.  (On given mu
            // nodes too: the mu guide and the mu nodes lie before the node data, and the table's header says where.)
            const size_t nt = (size_t) hdr[TAB_HDR_NTABLES], cells = (size_t) hdr[TAB_HDR_H], nmu9 = (size_t) -hdr[TAB_HDR_NMU];
            const double *guide = hdr + tab_2d_grid_guide_at(nt);
            d.par[0] = rim_frombits((uint64_t) (uintptr_t) (hdr + TAB_HDR_DOUBLES + row * TAB_2D_HDR));
            if (tab_kind_2d_nodes(KIND)) {
                const size_t at = tab_2d_nodes_nodes_at(nt, nn, cells, nmu9, (size_t) hdr[TAB_HDR_DOUBLES + TAB_2D_H]);
                d.par[1] = rim_frombits((uint64_t) (uintptr_t) (hdr + at + row * nn * nmu9 * 4));
            } else {
                d.par[1] = rim_frombits((uint64_t) (uintptr_t) (hdr + tab_2d_grid_nodes_at(nt, nn, cells) + row * nn * nmu9 * 4));
            }
            d.par[2] = rim_frombits((uint64_t) (uintptr_t) (guide + tab_grid_guide_doubles(cells)));
            d.par[3] = hdr[TAB_HDR_INVH];
            d.par[4] = hdr[TAB_HDR_H] - 1.;
            d.inv_gamma_cutoff = rim_frombits((uint64_t) (uintptr_t) guide);
            d.inv_kappa_width = hdr[TAB_HDR_GLO];
            d.neg_inverse_t = hdr[TAB_HDR_GHI];
            d.norm = ok ? norm : RIM_NAN;
            return;
        }
        if (KIND == DIST_TABULATED_GRID) {
            // a set on given nodes: par[0] the pitch-row part of the table's header in the tail (k: TAB_PITCHY_K from there),
            // par[1] the table's nodes, par[2] u_0, par[3] 1 / (cell width), par[4] the index of the last guide cell;
            // inv_gamma_cutoff, which carries the uniform step of the other forms, the bit pattern of the guide's address
            const size_t nt = (size_t) hdr[TAB_HDR_NTABLES], cells = (size_t) hdr[TAB_HDR_H], nmu8 = (size_t) hdr[TAB_HDR_NMU];
            const double *guide = hdr + TAB_HDR_DOUBLES;
            d.par[0] = rim_frombits((uint64_t) (uintptr_t) (hdr + tab_grid_tail(nt, nn, cells) + TAB_HDR_DOUBLES +
                                                            row * (TAB_PITCHY_PRE + TAB_PITCH_HDR + nmu8 * 2) + TAB_PITCHY_PRE));
            d.par[1] = rim_frombits((uint64_t) (uintptr_t) (guide + tab_grid_guide_doubles(cells) + row * nn * 4));
            d.par[2] = hdr[TAB_HDR_ULO];
            d.par[3] = hdr[TAB_HDR_INVH];
            d.par[4] = hdr[TAB_HDR_H] - 1.;
            d.inv_gamma_cutoff = rim_frombits((uint64_t) (uintptr_t) guide);
            d.inv_kappa_width = hdr[TAB_HDR_GLO];
            d.neg_inverse_t = hdr[TAB_HDR_GHI];
            d.norm = ok ? norm : RIM_NAN;
            return;
        }
        const size_t nmu = KIND == DIST_TABULATED_ISO ? 0 : (size_t) hdr[TAB_HDR_NMU];
        d.par[0] = 0.;
        if (KIND == DIST_TABULATED_PITCHY) {
            // a sin^k set: every table has a header, whose pitch-row part par[0] names (k: TAB_PITCHY_K from there)
            const size_t nt = (size_t) hdr[TAB_HDR_NTABLES];
            d.par[0] = rim_frombits((uint64_t) (uintptr_t) (hdr + TAB_HDR_DOUBLES + nt * nn * 2 +
                                                            row * (TAB_PITCHY_PRE + TAB_PITCH_HDR + nmu * 2) + TAB_PITCHY_PRE));
        } else if (nmu) {
            const size_t nt = (size_t) hdr[TAB_HDR_NTABLES];
            d.par[0] = rim_frombits((uint64_t) (uintptr_t) (hdr + TAB_HDR_DOUBLES + nt * nn * 2 + row * (TAB_PITCH_HDR + nmu * 2)));
        }
        d.par[1] = rim_frombits((uint64_t) (uintptr_t) (hdr + TAB_HDR_DOUBLES + row * nn * 2));
        d.par[2] = hdr[TAB_HDR_ULO];
        d.par[3] = hdr[TAB_HDR_INVH];
        d.par[4] = (double) (nn - 2);
        d.inv_gamma_cutoff = hdr[TAB_HDR_H];
        d.inv_kappa_width = hdr[TAB_HDR_GLO];
        d.neg_inverse_t = hdr[TAB_HDR_GHI];
        d.norm = ok ? norm : RIM_NAN;
        return;
    }
    d.inv_gamma_cutoff = 0.;
    d.inv_kappa_width = 0.;
    d.neg_inverse_t = 0.;
    d.norm = norm;
    if (KIND == DIST_POWER_LAW) d.inv_gamma_cutoff = 1. / d.par[3];
    if (KIND == DIST_THERMAL_JUETTNER) d.neg_inverse_t = -1. / d.par[0];
    if (KIND == DIST_PITCHY_PL) d.inv_gamma_cutoff = 1. / d.par[4];
    if (KIND == DIST_PITCHY_KAPPA) {
        d.inv_kappa_width = 1. / (d.par[0] * d.par[1]);
        d.inv_gamma_cutoff = 1. / d.par[3];
        // par[4] (unused by this distribution in the C ABI) flags the points whose kappa term may use the
        // restricted power function: a finite exponent and 1 + (gamma - 1) / (kappa width) a positive normal
        // number for every gamma >= 1.  Anything else -- kappa = +-inf (1^inf), kappa width < 0 (negative base) --
        // takes the general rim_pow, as the reference's powf would treat it (tools/hostile_sweep.py).
        const double kw = d.par[0] * d.par[1];
        d.par[4] = (rim_isfinite(d.par[0]) && kw > 1e-100 && kw < 1e100) ? 1. : 0.;
    }
}

// (1 + (gamma - 1) / (kappa width))^-(kappa + 1) exp(-gamma / gamma_cutoff) of the pitchy-kappa distribution
template <int PREC = 0>
RIM_DEV double kappa_gamma_term(const DistParams &d, double gamma)
{
    const double base = 1. + (gamma - 1.) * d.inv_kappa_width;
    const double y = -(d.par[0] + 1.);
    if (rim_bits(d.par[4]) != 0) return RimMath<PREC>::powexp_normal(base, y, -gamma * d.inv_gamma_cutoff);     // wave-uniform test
    return rim_pow(base, y) * RimMath<PREC>::exp(-gamma * d.inv_gamma_cutoff);
}

// Cubic Hermite on one interval of width h: q = {y0, m0, y1, m1}, the node values and slopes a lane reads as four
// consecutive doubles, t in [0, 1) the position in it.  The value and the derivative with respect to t.
RIM_DEV void tab_hermite(const double *q, double h, double t, double &val, double &dvaldt)
{
    const double y0 = q[0], m0 = q[1], y1 = q[2], m1 = q[3];
    const double b0 = h * m0, b1 = h * m1, dy = y1 - y0;
    const double c2 = 3. * dy - 2. * b0 - b1;
    const double c3 = b0 + b1 - 2. * dy;
    val = rim_fma(t, rim_fma(t, rim_fma(t, c3, c2), b0), y0);
    dvaldt = rim_fma(t, rim_fma(t, 3. * c3, 2. * c2), b0);
}

// The spline H(u) of a tabulated distribution and dH/du at u = ln gamma.  gamma outside the table only ever gets here as
// a NaN (the callers return 0 there first): the interval index is formed from a clamped copy, so every read stays inside
// the row.
RIM_DEV void tab_spline(const DistParams &d, double gamma, double &hval, double &dhdu)
{
    const double *row = (const double *) (uintptr_t) rim_bits(d.par[1]);
    const double x = (rim_log(gamma) - d.par[2]) * d.par[3];
    double xc = x;
    if (!(xc >= 0.)) xc = 0.;
    if (xc > d.par[4]) xc = d.par[4];
    const long long j = (long long) xc;
    const double t = x - (double) j;
    double dhdt;
    tab_hermite(row + 2 * j, d.inv_gamma_cutoff, t, hval, dhdt);
    dhdu = dhdt * d.par[3];
}

// tab_spline for a row of a family (d: dist_prepare<DIST_TABULATED_FAMILY> or <DIST_TABULATED_FAMILY_PITCHY>): the four node
// words {y0, m0, y1, m1} of the interval from row a and from the row behind it, each blended with one rim_fma(w, q_b - q_a, q_a)
// -- w = 0 gives q_a itself --, then ONE Hermite cubic: the interpolant is linear in its node words.  The index as in
// tab_spline; every read stays inside the two rows.
template <int KIND>
RIM_DEV void tab_spline_family(const DistParams &d, double gamma, double &hval, double &dhdu)
{
    const double *row = (const double *) (uintptr_t) rim_bits(d.par[1]);
    const double w = KIND == DIST_TABULATED_FAMILY_PITCHY ? ((const double *) (uintptr_t) rim_bits(d.par[0]))[TAB_FAMILY_W] : d.par[0];
    const double x = (rim_log(gamma) - d.par[2]) * d.par[3];
    double xc = x;
    if (!(xc >= 0.)) xc = 0.;
    if (xc > d.par[4]) xc = d.par[4];
    const long long j = (long long) xc;
    const double t = x - (double) j;
    const double *qa = row + 2 * j;
    const double *qb = qa + 2 * ((long long) d.par[4] + 2);
    double q[4];
    q[0] = rim_fma(w, qb[0] - qa[0], qa[0]);
    q[1] = rim_fma(w, qb[1] - qa[1], qa[1]);
    q[2] = rim_fma(w, qb[2] - qa[2], qa[2]);
    q[3] = rim_fma(w, qb[3] - qa[3], qa[3]);
    double dhdt;
    tab_hermite(q, d.inv_gamma_cutoff, t, hval, dhdt);
    dhdu = dhdt * d.par[3];
}

// does the row have a pitch-angle factor?  (wave-uniform; DIST_TABULATED_ISO: known not to at compile time)
RIM_DEV bool tab_has_pitch(const DistParams &d) { return rim_bits(d.par[0]) != 0; }
// the same where the normalisation asks (norm_kernel): par[0] of a family without a prefactor is a weight, not an address
template <int KIND>
RIM_DEV bool tab_norm_has_pitch(const DistParams &d)
{
    // (nor is that of a family of 2-D surfaces a pitch row: it names the row's line, and the factor is under the integral)
    return KIND == DIST_TABULATED_FAMILY || tab_kind_2d_family(KIND) ? false : tab_has_pitch(d);
}
template <int KIND>
RIM_DEV bool tab_kind_has_pitch(const DistParams &d)
{
    // (a 2-D table and one with a sin^k prefactor always have a live d f / d mu: they take the general forms, as a pitch
    // row does)
    return KIND == DIST_TABULATED_2D || KIND == DIST_TABULATED_PITCHY || KIND == DIST_TABULATED_GRID ||
        KIND == DIST_TABULATED_2D_GRID || tab_kind_2d_pitchy(KIND) || KIND == DIST_TABULATED_2D_NODES ||
        KIND == DIST_TABULATED_FAMILY_PITCHY || KIND == DIST_TABULATED_2D_FAMILY || KIND == DIST_TABULATED_2D_FAMILY_CUBIC ||
        (KIND != DIST_TABULATED_ISO && KIND != DIST_TABULATED_FAMILY && tab_has_pitch(d));
}

// The spline G(mu) = ln g of a pitch row (tab_has_pitch) and dG/dmu at mu = cos xi.  The interval index is formed from a
// clamped copy, as in tab_spline: a mu a rounding beyond +-1 extrapolates the end cubic, a NaN mu gives NaN, and every
// read stays inside the row.
RIM_DEV void tab_pitch_spline(const DistParams &d, double mu, double &gval, double &dgdmu)
{
    const double *ph = (const double *) (uintptr_t) rim_bits(d.par[0]);
    const double last = ph[TAB_PITCH_LAST], invh = ph[TAB_PITCH_INVH];
    const double x = (mu + 1.) * invh;
    double xc = x;
    if (!(xc >= 0.)) xc = 0.;
    if (xc > last) xc = last;
    const long long j = (long long) xc;
    const double t = x - (double) j;
    double dgdt;
    tab_hermite(ph + TAB_PITCH_HDR + 2 * j, ph[TAB_PITCH_H], t, gval, dgdt);
    dgdmu = dgdt * invh;
}

// The integrand of P of a table with a sin^k prefactor and a pitch row: (1 - mu^2)^(k/2) g(mu), the factor formed as
// tab_calc_f_both<DIST_TABULATED_PITCHY> forms it.  d: dist_prepare<DIST_TABULATED_PITCHY>'s.
RIM_DEV double tab_pitchy_p_integrand(const DistParams &d, double mu)
{
    const double *ph = (const double *) (uintptr_t) rim_bits(d.par[0]);
    double gval, dgdmu;
    tab_pitch_spline(d, mu, gval, dgdmu);
    return RimMath<0>::pow(rim_sqrt(1. - mu * mu), ph[TAB_PITCHY_K]) * rim_exp(gval);
}

// The same Hermite cubic from four values that do not sit side by side: the value and the derivative with respect to t.
RIM_DEV void tab_hermite4(double y0, double m0, double y1, double m1, double h, double t, double &val, double &dvaldt)
{
    const double b0 = h * m0, b1 = h * m1, dy = y1 - y0;
    const double c2 = 3. * dy - 2. * b0 - b1;
    const double c3 = b0 + b1 - 2. * dy;
    val = rim_fma(t, rim_fma(t, rim_fma(t, c3, c2), b0), y0);
    dvaldt = rim_fma(t, rim_fma(t, 3. * c3, 2. * c2), b0);
}

// The interval of u in a table on given nodes (d: dist_prepare<DIST_TABULATED_GRID>'s): the largest j <= n_nodes - 2 with
// u_j <= u, 0 where there is none or u is a NaN.  The data alone define it; the guide only says where to look.  The
// sample's cell c names two guide words: every node in a cell below c lies below u and every node in a cell above c above
// it (tab_grid_cell is monotone), so the interval is one of guide[c] .. guide[c + 1], and a bisection over the u_j of the
// row finds it.  Reads: the two guide words, then ceil(log2(guide[c + 1] - guide[c] + 1)) node words, 16 at the most.
RIM_DEV long long tab_grid_interval(const DistParams &d, double u)
{
    const double *row = (const double *) (uintptr_t) rim_bits(d.par[1]);
    const unsigned *guide = (const unsigned *) (uintptr_t) rim_bits(d.inv_gamma_cutoff);
    const long long c = tab_grid_cell(u, d.par[2], d.par[3], d.par[4]);
    long long lo = (long long) guide[c], hi = (long long) guide[c + 1];
    while (lo < hi) {
        const long long mid = (lo + hi + 1) >> 1;
        if (row[4 * mid] <= u) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// tab_spline for a table on given nodes: H(u) and dH/du at u = ln gamma.  t = (u - u_j) (1 / h_j) on the interval found,
// the Hermite cubic with h_j = u_{j+1} - u_j formed from the two node words as the host formed it.  A NaN gives NaN from
// interval 0; every read stays inside the set.  Only rim_log, explicit rim_fma and + - * here.
RIM_DEV void tab_spline_grid(const DistParams &d, double gamma, double &hval, double &dhdu)
{
    const double *row = (const double *) (uintptr_t) rim_bits(d.par[1]);
    const double u = rim_log(gamma);
    const double *q = row + 4 * tab_grid_interval(d, u);
    const double invh = q[3];
    const double t = (u - q[0]) * invh;
    double dhdt;
    tab_hermite4(q[1], q[2], q[5], q[6], q[4] - q[0], t, hval, dhdt);
    dhdu = dhdt * invh;
}

// n(gamma) = exp(H(ln gamma)) of the table: the integrand of the normalisation (power_law.rs:95-96 for a table)
template <int KIND = DIST_TABULATED>
RIM_DEV double tab_norm_integrand(const DistParams &d, double g)
{
    double hval, dhdu;
    if (KIND == DIST_TABULATED_GRID) tab_spline_grid(d, g, hval, dhdu);
    else if (tab_kind_family(KIND)) tab_spline_family<KIND>(d, g, hval, dhdu);
    else tab_spline(d, g, hval, dhdu);
    return rim_exp(hval);
}

// The surface S(u, mu) = ln n of a 2-D table at u = ln gamma, mu = cos xi, with dS/du and dS/dmu: bicubic Hermite on the
// cell, the tensor-product natural spline whose node data {S, S_u, S_mu, S_umu} rim_tab_build_2d solved.  Along mu first,
// on the cell's two u edges -- the value and the u slope, each with its mu derivative --, then along u through the two
// edges.  Both interval indices are formed from clamped copies, as in tab_spline / tab_pitch_spline: a mu a rounding
// beyond +-1 extrapolates the end cell, a NaN gives NaN, and every read stays inside the table.  Only rim_log, explicit
// rim_fma and + - * /: gcc and hipcc agree to the bit.
RIM_DEV void tab_bicubic(const DistParams &d, double gamma, double mu, double &sval, double &dsdu, double &dsdmu)
{
    const double *th = (const double *) (uintptr_t) rim_bits(d.par[0]);
    const double *nodes = (const double *) (uintptr_t) rim_bits(d.par[1]);
    const double mlast = th[TAB_2D_LAST], minvh = th[TAB_2D_INVH], mh = th[TAB_2D_H];
    const double x = (rim_log(gamma) - d.par[2]) * d.par[3];
    double xc = x;
    if (!(xc >= 0.)) xc = 0.;
    if (xc > d.par[4]) xc = d.par[4];
    const long long i = (long long) xc;
    const double tu = x - (double) i;
    const double z = (mu + 1.) * minvh;
    double zc = z;
    if (!(zc >= 0.)) zc = 0.;
    if (zc > mlast) zc = mlast;
    const long long j = (long long) zc;
    const double tm = z - (double) j;
    const long long nmu = (long long) mlast + 2;
    const double *a = nodes + (i * nmu + j) * 4;        // nodes (i, j), (i, j + 1)
    const double *b = a + nmu * 4;                      // nodes (i + 1, j), (i + 1, j + 1)
    // along mu on the edge u_i and on the edge u_{i+1}: the value v and the u slope w, d./dt_mu of each
    double va, dva, wa, dwa, vb, dvb, wb, dwb;
    tab_hermite4(a[0], a[2], a[4], a[6], mh, tm, va, dva);
    tab_hermite4(a[1], a[3], a[5], a[7], mh, tm, wa, dwa);
    tab_hermite4(b[0], b[2], b[4], b[6], mh, tm, vb, dvb);
    tab_hermite4(b[1], b[3], b[5], b[7], mh, tm, wb, dwb);
    // along u through the two edges: S and dS/dt_u from (v, w), dS/dt_mu from their mu derivatives
    double dsdtu, dsdtm, unused;
    tab_hermite4(va, wa, vb, wb, d.inv_gamma_cutoff, tu, sval, dsdtu);
    tab_hermite4(dva, dwa, dvb, dwb, d.inv_gamma_cutoff, tu, dsdtm, unused);
    dsdu = dsdtu * d.par[3];
    dsdmu = dsdtm * minvh;
}

// The interval of u in a 2-D set on given nodes (d: dist_prepare<DIST_TABULATED_2D_GRID>'s): tab_grid_interval on the set's
// u nodes, two words apart.  The largest i <= n_nodes - 2 with u_i <= u, 0 where there is none or u is a NaN; the data alone
// define it.  Reads: the two guide words, then at most 16 node words.
RIM_DEV long long tab_2d_grid_interval(const DistParams &d, double u)
{
    const double *un = (const double *) (uintptr_t) rim_bits(d.par[2]);
    const unsigned *guide = (const unsigned *) (uintptr_t) rim_bits(d.inv_gamma_cutoff);
    const long long c = tab_grid_cell(u, un[0], d.par[3], d.par[4]);
    long long lo = (long long) guide[c], hi = (long long) guide[c + 1];
    while (lo < hi) {
        const long long mid = (lo + hi + 1) >> 1;
        if (un[2 * mid] <= u) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// tab_bicubic for a 2-D set on given nodes: the same bicubic on the cell found by tab_2d_grid_interval, with the cell's own
// h_i = u_{i+1} - u_i, formed from the two node words as the host formed it, and its 1 / h_i in the two Hermite steps along u
// and in dS/du; t_u = (u - u_i) (1 / h_i).  The mu index from a clamped copy; a NaN gives NaN from cell 0; every read stays
// inside the set.  Only rim_log, explicit rim_fma and + - * /.
RIM_DEV void tab_bicubic_grid(const DistParams &d, double gamma, double mu, double &sval, double &dsdu, double &dsdmu)
{
    const double *th = (const double *) (uintptr_t) rim_bits(d.par[0]);
    const double *nodes = (const double *) (uintptr_t) rim_bits(d.par[1]);
    const double *un = (const double *) (uintptr_t) rim_bits(d.par[2]);
    const double mlast = th[TAB_2D_LAST], minvh = th[TAB_2D_INVH], mh = th[TAB_2D_H];
    const double u = rim_log(gamma);
    const long long i = tab_2d_grid_interval(d, u);
    const double *q = un + 2 * i;
    const double uinvh = q[1], uh = q[2] - q[0];
    const double tu = (u - q[0]) * uinvh;
    const double z = (mu + 1.) * minvh;
    double zc = z;
    if (!(zc >= 0.)) zc = 0.;
    if (zc > mlast) zc = mlast;
    const long long j = (long long) zc;
    const double tm = z - (double) j;
    const long long nmu = (long long) mlast + 2;
    const double *a = nodes + (i * nmu + j) * 4;        // nodes (i, j), (i, j + 1)
    const double *b = a + nmu * 4;                      // nodes (i + 1, j), (i + 1, j + 1)
    double va, dva, wa, dwa, vb, dvb, wb, dwb;
    tab_hermite4(a[0], a[2], a[4], a[6], mh, tm, va, dva);
    tab_hermite4(a[1], a[3], a[5], a[7], mh, tm, wa, dwa);
    tab_hermite4(b[0], b[2], b[4], b[6], mh, tm, vb, dvb);
    tab_hermite4(b[1], b[3], b[5], b[7], mh, tm, wb, dwb);
    double dsdtu, dsdtm, unused;
    tab_hermite4(va, wa, vb, wb, uh, tu, sval, dsdtu);
    tab_hermite4(dva, dwa, dvb, dwb, uh, tu, dsdtm, unused);
    dsdu = dsdtu * uinvh;
    dsdmu = dsdtm * minvh;
}

// The interval of mu in a 2-D set on given mu nodes (th: the table's header, mn: the set's mu nodes): the largest j <= n_mu - 2
// with mu_j <= mu, 0 where there is none or mu is a NaN.  The data alone define it, as tab_grid_interval says for gamma; the
// guide only says where to look.  Reads: the two guide words, then ceil(log2(guide[c + 1] - guide[c] + 1)) node words, 10
// at the most (n_mu <= 1024: no two guide words are further apart than 1022).  mu_0 = -1 by the check of the set.
RIM_DEV long long tab_2d_nodes_mu_interval(const double *th, const double *mn, double mu)
{
    const unsigned *guide = (const unsigned *) (th + (long long) th[TAB_2D_MU_GUIDE]);
    const long long c = tab_grid_cell(mu, -1., th[TAB_2D_INVH], th[TAB_2D_H] - 1.);
    long long lo = (long long) guide[c], hi = (long long) guide[c + 1];
    while (lo < hi) {
        const long long mid = (lo + hi + 1) >> 1;
        RIM_TAB_2D_NODES_READ();
        if (mn[2 * mid] <= mu) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// tab_bicubic_grid for a 2-D set on given mu nodes as well: the same bicubic on the cell found by tab_2d_grid_interval and
// tab_2d_nodes_mu_interval.  Along mu the four Hermite steps use the cell's own h_j = mu_{j+1} - mu_j, formed from the two node
// words as the host formed it; t_mu = (mu - mu_j) (1 / h_j), dS/dmu = dS/dt_mu (1 / h_j).  A mu a rounding beyond +-1
// extrapolates the end cell; a NaN gives NaN from cell 0; every read stays inside the set.  Only rim_log, explicit rim_fma
// and + - * /.
RIM_DEV void tab_bicubic_nodes(const DistParams &d, double gamma, double mu, double &sval, double &dsdu, double &dsdmu)
{
    const double *th = (const double *) (uintptr_t) rim_bits(d.par[0]);
    const double *nodes = (const double *) (uintptr_t) rim_bits(d.par[1]);
    const double *un = (const double *) (uintptr_t) rim_bits(d.par[2]);
    const double *mn = th + (long long) th[TAB_2D_MU_NODES];
    const double u = rim_log(gamma);
    const long long i = tab_2d_grid_interval(d, u);
    const double *q = un + 2 * i;
    const double uinvh = q[1], uh = q[2] - q[0];
    const double tu = (u - q[0]) * uinvh;
    const long long j = tab_2d_nodes_mu_interval(th, mn, mu);
    const double *r = mn + 2 * j;
    const double minvh = r[1], mh = r[2] - r[0];
    const double tm = (mu - r[0]) * minvh;
    const long long nmu = (long long) th[TAB_2D_LAST] + 2;
    const double *a = nodes + (i * nmu + j) * 4;        // nodes (i, j), (i, j + 1)
    const double *b = a + nmu * 4;                      // nodes (i + 1, j), (i + 1, j + 1)
    double va, dva, wa, dwa, vb, dvb, wb, dwb;
    tab_hermite4(a[0], a[2], a[4], a[6], mh, tm, va, dva);
    tab_hermite4(a[1], a[3], a[5], a[7], mh, tm, wa, dwa);
    tab_hermite4(b[0], b[2], b[4], b[6], mh, tm, vb, dvb);
    tab_hermite4(b[1], b[3], b[5], b[7], mh, tm, wb, dwb);
    double dsdtu, dsdtm, unused;
    tab_hermite4(va, wa, vb, wb, uh, tu, sval, dsdtu);
    tab_hermite4(dva, dwa, dvb, dwb, uh, tu, dsdtm, unused);
    dsdu = dsdtu * uinvh;
    dsdmu = dsdtm * minvh;
}

// tab_bicubic_nodes for a row of a family of 2-D surfaces (d: dist_prepare<DIST_TABULATED_2D_FAMILY> or <.._PITCHY>): the cell is
// found once, as tab_bicubic_nodes finds it; then, Hermite step by Hermite step along mu, the four node words of the step are
// read from table a and from table b, each pair blended with one rim_fma(w, q_b - q_a, q_a) -- w = 0 gives q_a itself, but for
// the sign of a zero --, and the step evaluated: eight words in flight, not thirty-two.  The bicubic is linear in its node
// words and the spline solve is linear in the data, so this is the spline of the blended data.  w and the distance to table b
// are two wave-uniform words of the row's line.  Every read stays inside the set.
RIM_DEV void tab_bicubic_family(const DistParams &d, double gamma, double mu, double &sval, double &dsdu, double &dsdmu)
{
    const double *th = (const double *) (uintptr_t) rim_bits(d.par[0]);
    const double *nodes = (const double *) (uintptr_t) rim_bits(d.par[1]);
    const double *un = (const double *) (uintptr_t) rim_bits(d.par[2]);
    const double *mn = th + (long long) th[TAB_2D_MU_NODES];
    const double w = th[TAB_2D_NORM];
    const long long to_b = (long long) th[TAB_2D_ENDS];
    const double u = rim_log(gamma);
    const long long i = tab_2d_grid_interval(d, u);
    const double *q = un + 2 * i;
    const double uinvh = q[1], uh = q[2] - q[0];
    const double tu = (u - q[0]) * uinvh;
    const long long j = tab_2d_nodes_mu_interval(th, mn, mu);
    const double *r = mn + 2 * j;
    const double minvh = r[1], mh = r[2] - r[0];
    const double tm = (mu - r[0]) * minvh;
    const long long nmu = (long long) th[TAB_2D_LAST] + 2;
    const double *a = nodes + (i * nmu + j) * 4;        // nodes (i, j), (i, j + 1) of table a
    const double *b = a + nmu * 4;                      // nodes (i + 1, j), (i + 1, j + 1) of table a
    const double *a2 = a + to_b, *b2 = b + to_b;        // the same of table b
    double va, dva, wa, dwa, vb, dvb, wb, dwb;
    tab_hermite4(tab_family_blend(w, a[0], a2[0]), tab_family_blend(w, a[2], a2[2]), tab_family_blend(w, a[4], a2[4]),
                 tab_family_blend(w, a[6], a2[6]), mh, tm, va, dva);
    tab_hermite4(tab_family_blend(w, a[1], a2[1]), tab_family_blend(w, a[3], a2[3]), tab_family_blend(w, a[5], a2[5]),
                 tab_family_blend(w, a[7], a2[7]), mh, tm, wa, dwa);
    tab_hermite4(tab_family_blend(w, b[0], b2[0]), tab_family_blend(w, b[2], b2[2]), tab_family_blend(w, b[4], b2[4]),
                 tab_family_blend(w, b[6], b2[6]), mh, tm, vb, dvb);
    tab_hermite4(tab_family_blend(w, b[1], b2[1]), tab_family_blend(w, b[3], b2[3]), tab_family_blend(w, b[5], b2[5]),
                 tab_family_blend(w, b[7], b2[7]), mh, tm, wb, dwb);
    double dsdtu, dsdtm, unused;
    tab_hermite4(va, wa, vb, wb, uh, tu, sval, dsdtu);
    tab_hermite4(dva, dwa, dvb, dwb, uh, tu, dsdtm, unused);
    dsdu = dsdtu * uinvh;
    dsdmu = dsdtm * minvh;
}

// tab_bicubic_family under the CUBIC blend (d: dist_prepare<DIST_TABULATED_2D_FAMILY_CUBIC> or <.._PITCHY>): the cell is found
// once; then, Hermite step by Hermite step along mu, the four node words of the step are read from the stencil's four tables
// and blended with the row's Lagrange weights, fma(L_3, q_3, fma(L_2, q_2, fma(L_1, q_1, L_0 q_0))): sixteen words in flight,
// not sixty-four.  Weights 0, 1, 0, 0 in some order give that table's word itself, but for the sign of a zero.  The weights
// and the table stride are five wave-uniform words of the row's line.  Every read stays inside the set.
RIM_DEV void tab_bicubic_family_cubic(const DistParams &d, double gamma, double mu, double &sval, double &dsdu, double &dsdmu)
{
    const double *th = (const double *) (uintptr_t) rim_bits(d.par[0]);
    const double *nodes = (const double *) (uintptr_t) rim_bits(d.par[1]);
    const double *un = (const double *) (uintptr_t) rim_bits(d.par[2]);
    const double *mn = th + (long long) th[TAB_2D_MU_NODES];
    const double l[4] = { th[TAB_2D_CUBIC_L], th[TAB_2D_CUBIC_L + 1], th[TAB_2D_CUBIC_L + 2], th[TAB_2D_CUBIC_L + 3] };
    const long long st = (long long) th[TAB_2D_ENDS];
    const double u = rim_log(gamma);
    const long long i = tab_2d_grid_interval(d, u);
    const double *q = un + 2 * i;
    const double uinvh = q[1], uh = q[2] - q[0];
    const double tu = (u - q[0]) * uinvh;
    const long long j = tab_2d_nodes_mu_interval(th, mn, mu);
    const double *r = mn + 2 * j;
    const double minvh = r[1], mh = r[2] - r[0];
    const double tm = (mu - r[0]) * minvh;
    const long long nmu = (long long) th[TAB_2D_LAST] + 2;
    const double *a = nodes + (i * nmu + j) * 4;        // nodes (i, j), (i, j + 1) of the stencil's base table
    const double *b = a + nmu * 4;                      // nodes (i + 1, j), (i + 1, j + 1) of it
    const double *a1 = a + st, *a2 = a1 + st, *a3 = a2 + st;    // the same of the three tables above it
    const double *b1 = b + st, *b2 = b1 + st, *b3 = b2 + st;
    double va, dva, wa, dwa, vb, dvb, wb, dwb;
    tab_hermite4(tab_family_blend4(l, a[0], a1[0], a2[0], a3[0]), tab_family_blend4(l, a[2], a1[2], a2[2], a3[2]),
                 tab_family_blend4(l, a[4], a1[4], a2[4], a3[4]), tab_family_blend4(l, a[6], a1[6], a2[6], a3[6]), mh, tm, va, dva);
    tab_hermite4(tab_family_blend4(l, a[1], a1[1], a2[1], a3[1]), tab_family_blend4(l, a[3], a1[3], a2[3], a3[3]),
                 tab_family_blend4(l, a[5], a1[5], a2[5], a3[5]), tab_family_blend4(l, a[7], a1[7], a2[7], a3[7]), mh, tm, wa, dwa);
    tab_hermite4(tab_family_blend4(l, b[0], b1[0], b2[0], b3[0]), tab_family_blend4(l, b[2], b1[2], b2[2], b3[2]),
                 tab_family_blend4(l, b[4], b1[4], b2[4], b3[4]), tab_family_blend4(l, b[6], b1[6], b2[6], b3[6]), mh, tm, vb, dvb);
    tab_hermite4(tab_family_blend4(l, b[1], b1[1], b2[1], b3[1]), tab_family_blend4(l, b[3], b1[3], b2[3], b3[3]),
                 tab_family_blend4(l, b[5], b1[5], b2[5], b3[5]), tab_family_blend4(l, b[7], b1[7], b2[7], b3[7]), mh, tm, wb, dwb);
    double dsdtu, dsdtm, unused;
    tab_hermite4(va, wa, vb, wb, uh, tu, sval, dsdtu);
    tab_hermite4(dva, dwa, dvb, dwb, uh, tu, dsdtm, unused);
    dsdu = dsdtu * uinvh;
    dsdmu = dsdtm * minvh;
}

// nbar(gamma) = 1/2 int exp(S(ln gamma, mu)) dmu of a 2-D table: the integrand of its normalisation.  The 31-point Kronrod
// rule (xgk, wgk: gk31_table.h) on every mu cell, summed in node order -- the rule P of a pitch row uses.  KIND: the form
// of the set, one of the six 2-D forms.
//
// With a sin^k prefactor nbar = 1/2 int (1 - mu^2)^(k/2) exp(S) dmu, and the derivative of the integrand is singular at mu =
// +-1 for a non-integer k or k < 2: the plain rule on an end cell is left with 4e-6 at k = 0.5 on 8 nodes.  The two end
// cells are integrated under 1 - |mu| = omega = h v^4, v in [0, 1] on the same 31 nodes, Jacobian 4 h v^3: the integrand in
// v goes as v^(2k+3) and the rule is at rounding for every k.  omega travels next to the node, so that sin^2 xi = omega (2 -
// omega) is formed without cancellation.  Interior cells keep the plain rule with the factor as tab_calc_f_both forms it.
//
// On given mu nodes every cell has its own centre and half width, from its two node words, and h of the substitution is the
// end cell's own width: a graded set may make that cell 1e-5 wide, and the singular derivative is inside it all the same.
//
// A family of 2-D surfaces takes the same path on its row's line: the blended surface, the blended k.
template <int KIND = DIST_TABULATED_2D>
RIM_DEV double tab_2d_norm_integrand(const DistParams &d, double g, const double *xgk, const double *wgk)
{
    const double *th = (const double *) (uintptr_t) rim_bits(d.par[0]);
    const long long cells = (long long) th[TAB_2D_LAST] + 1;
    const double h = th[TAB_2D_H];
    double sum = 0.;
    if (tab_kind_2d_nodes(KIND) || tab_kind_2d_family(KIND)) {
        const double *mn = th + (long long) th[TAB_2D_MU_NODES];
        const double sk = tab_kind_2d_pitchy(KIND) ? th[TAB_2D_K] : 0.;
        for (long long j = 0; j < cells; j++) {
            const double w = mn[2 * j + 2] - mn[2 * j];
            const double half = 0.5 * w, centre = mn[2 * j] + half;
#if defined(RIM_TAB_2D_PITCHY_PLAIN_ENDS)
            const bool end = false;
#else
            const bool end = tab_kind_2d_pitchy(KIND) && (j == 0 || j == cells - 1);
#endif
            double acc = 0.;
            for (int k = 0; k < 31; k++) {
                double sval, dsdu, dsdmu, mu, sin2 = 1., jac = 1.;
                if (end) {
                    const double v = 0.5 + 0.5 * xgk[k];
                    const double v2 = v * v;
                    const double omega = w * (v2 * v2);
                    mu = j == 0 ? -1. + omega : 1. - omega;
                    sin2 = omega * (2. - omega);
                    jac = 4. * (v2 * v);
                } else {
                    mu = centre + half * xgk[k];
                    if (tab_kind_2d_pitchy(KIND)) sin2 = 1. - mu * mu;
                }
                if (tab_kind_2d_family_cubic(KIND)) tab_bicubic_family_cubic(d, g, mu, sval, dsdu, dsdmu);
                else if (tab_kind_2d_family(KIND)) tab_bicubic_family(d, g, mu, sval, dsdu, dsdmu);
                else tab_bicubic_nodes(d, g, mu, sval, dsdu, dsdmu);
                if (tab_kind_2d_pitchy(KIND)) acc += wgk[k] * (jac * (RimMath<0>::pow(rim_sqrt(sin2), sk) * rim_exp(sval)));
                else acc += wgk[k] * rim_exp(sval);
            }
            sum += half * acc;
        }
        return 0.5 * sum;
    }
    if (tab_kind_2d_pitchy(KIND)) {
        const double sk = th[TAB_2D_K];
        for (long long j = 0; j < cells; j++) {
            const double half = 0.5 * h, centre = -1. + ((double) j + 0.5) * h;
#if defined(RIM_TAB_2D_PITCHY_PLAIN_ENDS)
            const bool end = false;         // (a private build of the tests: what the plain rule leaves on the end cells)
#else
            const bool end = j == 0 || j == cells - 1;
#endif
            double acc = 0.;
            for (int k = 0; k < 31; k++) {
                double sval, dsdu, dsdmu, mu, sin2, jac;
                if (end) {
                    const double v = 0.5 + 0.5 * xgk[k];
                    const double v2 = v * v;
                    const double omega = h * (v2 * v2);
                    mu = j == 0 ? -1. + omega : 1. - omega;
                    sin2 = omega * (2. - omega);
                    jac = 4. * (v2 * v);            // (times h / 2 below: dmu = 4 h v^3 dv, dv = 1/2 dx)
                } else {
                    mu = centre + half * xgk[k];
                    sin2 = 1. - mu * mu;
                    jac = 1.;
                }
                if (tab_kind_2d_on_grid(KIND)) tab_bicubic_grid(d, g, mu, sval, dsdu, dsdmu);
                else tab_bicubic(d, g, mu, sval, dsdu, dsdmu);
                acc += wgk[k] * (jac * (RimMath<0>::pow(rim_sqrt(sin2), sk) * rim_exp(sval)));
            }
            sum += half * acc;
        }
        return 0.5 * sum;
    }
    for (long long j = 0; j < cells; j++) {
        const double half = 0.5 * h, centre = -1. + ((double) j + 0.5) * h;
        double acc = 0.;
        for (int k = 0; k < 31; k++) {
            double sval, dsdu, dsdmu;
            if (KIND == DIST_TABULATED_2D_GRID) tab_bicubic_grid(d, g, centre + half * xgk[k], sval, dsdu, dsdmu);
            else tab_bicubic(d, g, centre + half * xgk[k], sval, dsdu, dsdmu);
            acc += wgk[k] * rim_exp(sval);
        }
        sum += half * acc;
    }
    return 0.5 * sum;
}

// calc_f and calc_f_derivatives of the tabulated distribution, one body for all three entries below:
// f = norm n(gamma) g(mu) / (gamma^2 beta), 0 outside the table (the rule of power_law.rs:38,49), d f / d mu = f G'(mu).
// A row without a pitch factor is isotropic: no further load, the arithmetic of n(gamma) alone, d f / d mu = +0.
template <int KIND = DIST_TABULATED>
RIM_DEV void tab_calc_f_both(const DistParams &d, double gamma, double cos_xi, double &f, double &dfdg, double &dfdcx)
{
    f = 0.; dfdg = 0.; dfdcx = 0.;
    if (gamma < d.inv_kappa_width || gamma > d.neg_inverse_t) return;
    if (KIND == DIST_TABULATED_2D || KIND == DIST_TABULATED_2D_GRID || KIND == DIST_TABULATED_2D_NODES ||
        KIND == DIST_TABULATED_2D_FAMILY || KIND == DIST_TABULATED_2D_FAMILY_CUBIC) {
        // f = norm exp(S(ln gamma, mu)) / (gamma^2 beta), d f / d mu = f S_mu: one exponential per sample
        double sval, dsdu, dsdmu;
        if (KIND == DIST_TABULATED_2D_FAMILY_CUBIC) tab_bicubic_family_cubic(d, gamma, cos_xi, sval, dsdu, dsdmu);
        else if (KIND == DIST_TABULATED_2D_FAMILY) tab_bicubic_family(d, gamma, cos_xi, sval, dsdu, dsdmu);
        else if (KIND == DIST_TABULATED_2D_NODES) tab_bicubic_nodes(d, gamma, cos_xi, sval, dsdu, dsdmu);
        else if (KIND == DIST_TABULATED_2D_GRID) tab_bicubic_grid(d, gamma, cos_xi, sval, dsdu, dsdmu);
        else tab_bicubic(d, gamma, cos_xi, sval, dsdu, dsdmu);
        const double beta2 = rim_sqrt(1. - rim_div_moderate(1., gamma * gamma));
        f = d.norm * rim_exp(sval) / (gamma * gamma * beta2);
        dfdg = f * (dsdu / gamma - 1. / gamma - gamma / (gamma * gamma - 1.));
        dfdcx = f * dsdmu;
        return;
    }
    if (tab_kind_2d_pitchy(KIND)) {
        // f = norm sin^k xi exp(S) / (gamma^2 beta), d f / d mu = f (S_mu - k mu / sin^2 xi): the factor and its term as the
        // pitchy kinds and DIST_TABULATED_PITCHY form them, k a wave-uniform load from the table's header.  A mu a rounding
        // beyond +-1 is a NaN here (the square root), where the plain 2-D forms extrapolate the end cell.  (A family: the
        // blended k of the row's line.)
        const double *th = (const double *) (uintptr_t) rim_bits(d.par[0]);
        const double k = th[TAB_2D_K];
        double sval, dsdu, dsdmu;
        if (tab_kind_2d_family_cubic(KIND)) tab_bicubic_family_cubic(d, gamma, cos_xi, sval, dsdu, dsdmu);
        else if (tab_kind_2d_family(KIND)) tab_bicubic_family(d, gamma, cos_xi, sval, dsdu, dsdmu);
        else if (tab_kind_2d_nodes(KIND)) tab_bicubic_nodes(d, gamma, cos_xi, sval, dsdu, dsdmu);
        else if (tab_kind_2d_on_grid(KIND)) tab_bicubic_grid(d, gamma, cos_xi, sval, dsdu, dsdmu);
        else tab_bicubic(d, gamma, cos_xi, sval, dsdu, dsdmu);
        const double sin_xi = rim_sqrt(1. - cos_xi * cos_xi);
        const double pa_term = RimMath<0>::pow(sin_xi, k);
        const double beta2 = rim_sqrt(1. - rim_div_moderate(1., gamma * gamma));
        f = d.norm * pa_term * rim_exp(sval) / (gamma * gamma * beta2);
        dfdg = f * (dsdu / gamma - 1. / gamma - gamma / (gamma * gamma - 1.));
        dfdcx = f * (dsdmu - k * cos_xi / (sin_xi * sin_xi));
        return;
    }
    double hval, dhdu;
    if (KIND == DIST_TABULATED_GRID) tab_spline_grid(d, gamma, hval, dhdu);
    else if (tab_kind_family(KIND)) tab_spline_family<KIND>(d, gamma, hval, dhdu);
    else tab_spline(d, gamma, hval, dhdu);
    const double beta = rim_sqrt(1. - rim_div_moderate(1., gamma * gamma));
    if (KIND == DIST_TABULATED_PITCHY || KIND == DIST_TABULATED_GRID || KIND == DIST_TABULATED_FAMILY_PITCHY) {
        // f = norm n(gamma) sin^k xi g(mu) / (gamma^2 beta), d f / d mu = f (G' - k mu / sin^2 xi): the factor and its term as
        // the pitchy kinds form them (pitchy_pl.rs:56-61), k a wave-uniform load; without a pitch row G = G' = 0
        const double *ph = (const double *) (uintptr_t) rim_bits(d.par[0]);
        const double k = ph[TAB_PITCHY_K];
        const double sin_xi = rim_sqrt(1. - cos_xi * cos_xi);
        const double pa_term = RimMath<0>::pow(sin_xi, k);
        double gval = 0., dgdmu = 0.;
        if (ph[TAB_PITCHY_NMU] != 0.) tab_pitch_spline(d, cos_xi, gval, dgdmu);
        f = d.norm * pa_term * rim_exp(hval + gval) / (gamma * gamma * beta);
        dfdcx = f * (dgdmu - k * cos_xi / (sin_xi * sin_xi));
    } else if (tab_kind_has_pitch<KIND>(d)) {
        double gval, dgdmu;
        tab_pitch_spline(d, cos_xi, gval, dgdmu);
        f = d.norm * rim_exp(hval + gval) / (gamma * gamma * beta);
        dfdcx = f * dgdmu;
    } else {
        f = d.norm * rim_exp(hval) / (gamma * gamma * beta);
    }
    dfdg = f * (dhdu / gamma - 1. / gamma - gamma / (gamma * gamma - 1.));
}

template <int KIND, int PREC = 0>
RIM_DEV double calc_f(const DistParams &d, double gamma, double cos_xi)
{
    typedef RimMath<PREC> M;
    if (dist_is_tab(KIND)) {
        double f, dfdg, dfdcx;
        tab_calc_f_both<KIND>(d, gamma, cos_xi, f, dfdg, dfdcx);
        return f;
    }
    if (KIND == DIST_POWER_LAW) {
        if (gamma < d.par[1] || gamma > d.par[2]) return 0.;
        RIM_HIT(19);
        const double beta = rim_sqrt(1. - rim_div_moderate(1., gamma * gamma));
        return d.norm * M::powexp_normal(gamma, -d.par[0], -gamma * d.inv_gamma_cutoff) / (gamma * gamma * beta);
    } else if (KIND == DIST_THERMAL_JUETTNER) {
        return d.norm * M::exp(d.neg_inverse_t * gamma);
    } else if (KIND == DIST_PITCHY_PL) {
        if (gamma < d.par[2] || gamma > d.par[3]) return 0.;
        const double sin_xi = rim_sqrt(1. - cos_xi * cos_xi);
        const double pa_term = M::pow(sin_xi, d.par[1]);
        const double beta = rim_sqrt(1. - rim_div_moderate(1., gamma * gamma));
        const double gamma_term = M::powexp_normal(gamma, -d.par[0], -gamma * d.inv_gamma_cutoff);
        return d.norm * pa_term * gamma_term / (gamma * gamma * beta);
    } else {
        const double sin_xi = rim_sqrt(1. - cos_xi * cos_xi);
        const double pa_term = M::pow(sin_xi, d.par[2]);
        const double gamma_term = kappa_gamma_term<PREC>(d, gamma);
        return d.norm * pa_term * gamma_term;
    }
}

template <int KIND, int PREC = 0>
RIM_DEV void calc_f_derivatives(const DistParams &d, double gamma, double cos_xi, double &dfdg, double &dfdcx)
{
    typedef RimMath<PREC> M;
    if (dist_is_tab(KIND)) {
        double f;
        tab_calc_f_both<KIND>(d, gamma, cos_xi, f, dfdg, dfdcx);
        return;
    }
    if (KIND == DIST_POWER_LAW) {
        if (gamma < d.par[1] || gamma > d.par[2]) { dfdg = 0.; dfdcx = 0.; return; }
        RIM_HIT(20);
        const double p_plus_1 = d.par[0] + 1.;
        const double g2_minus_1 = gamma * gamma - 1.;
        dfdg = -d.norm * M::powexp_normal(gamma, -p_plus_1, -gamma * d.inv_gamma_cutoff) / rim_sqrt(g2_minus_1) *
            (p_plus_1 / gamma + gamma / g2_minus_1 + d.inv_gamma_cutoff);
        dfdcx = 0.;
    } else if (KIND == DIST_THERMAL_JUETTNER) {
        dfdg = d.norm * M::exp(d.neg_inverse_t * gamma) * d.neg_inverse_t;
        dfdcx = 0.;
    } else if (KIND == DIST_PITCHY_PL) {
        if (gamma < d.par[2] || gamma > d.par[3]) { dfdg = 0.; dfdcx = 0.; return; }
        const double p = d.par[0], k = d.par[1];
        const double sin_xi = rim_sqrt(1. - cos_xi * cos_xi);
        const double pa_term = M::pow(sin_xi, k);
        const double beta = rim_sqrt(1. - rim_div_moderate(1., gamma * gamma));
        const double gamma_term = M::powexp_normal(gamma, -p, -gamma * d.inv_gamma_cutoff);
        const double f = d.norm * pa_term * gamma_term / (gamma * gamma * beta);
        dfdg = -f * ((p + 1.) / gamma + gamma / (gamma * gamma - 1.) + d.inv_gamma_cutoff);
        dfdcx = -f * k * cos_xi / (sin_xi * sin_xi);
    } else {
        const double kappa = d.par[0], width = d.par[1], k = d.par[2];
        const double sin_xi = rim_sqrt(1. - cos_xi * cos_xi);
        const double pa_term = M::pow(sin_xi, k);
        const double gamma_term = kappa_gamma_term<PREC>(d, gamma);
        const double f = d.norm * pa_term * gamma_term;
        dfdg = -f * ((kappa + 1.) / (kappa * width + gamma - 1.) + d.inv_gamma_cutoff);
        dfdcx = -f * k * cos_xi / (sin_xi * sin_xi);
    }
}

// Observer/point data shared by all samples of a coefficient (wave-uniform).
struct SymPoint {
    double s, cos_th, sin_th;
    int coeff, stokes;
};

// Order data for one gamma-integral: J_n and J_{n+1} at fixed n (wave-uniform).
// The two LeungOrder records live in memory the caller provides -- LDS in the wave kernels -- and
// are read where they are used: held in registers they would cost 56 SGPRs for the whole integrand
// (the kernel then spills SGPRs into VGPR lanes inside the hot loop).
struct SymOrder {
    double n;
    bool small;         // integer n < 30: Miller recurrence instead of the Leung expansions
    bool np1_small;     // n + 1 < 30
    bool dj_nan;        // n >= 1e15 (bessel.c:382-388)
    const LeungOrder *o;  // [2]: orders n and n + 1 (valid when >= 30)
};

RIM_DEV SymOrder sym_order(double n, LeungOrder *store)
{
    SymOrder so;
    so.n = n;
    so.small = n < 30.;
    so.np1_small = (n + 1.) < 30.;
    so.dj_nan = n >= 1e15;
    store[0] = LeungOrder();
    store[1] = LeungOrder();
    if (!so.small) store[0] = leung_order(n);
    if (!so.np1_small) store[1] = leung_order(n + 1.);
    so.o = store;
    return so;
}

// J_n(z) and J'_n(z) as the reference's pkgw_bessel_j / pkgw_bessel_dj pair would
// return them.  The two Leung evaluations (orders n and n+1) run through one
// loop body so the expansions are inlined once.
template <int PREC = 0>
RIM_DEV void sym_bessel_pair(const SymOrder &so, double z, double &jn, double &djn)
{
    const double n = so.n;
    double jv0 = 0., jv1 = 0.;
    if (!so.np1_small) {
        // which expansions do the two orders need at this z?  (order n only if it is >= 30)
        RIM_PROF_T(t_sel);
        double pos0 = 0., pos1 = 0.;
        int c0 = 0;
        if (!so.small) c0 = leung_select_code(so.o[0], z, pos0);
        const int c1 = leung_select_code(so.o[1], z, pos1);
        RIM_PROF_ADD(3, t_sel);
        RIM_LANES(30, true);
        RIM_LANES(26, ((c0 | c1) & LSEL_DEBYE) != 0);
        RIM_LANES(27, (c0 & LSEL_MEISSEL) != 0);
        RIM_LANES(28, (c1 & LSEL_MEISSEL) != 0);
        RIM_LANES(29, (c1 & LSEL_BLEND) != 0);
        // Debye for both orders in one go (they share everything but x - n), Meissel order by order
        RIM_PROF_T(t_deb);
        double deb0 = 0., deb1 = 0.;
        if ((c0 | c1) & LSEL_DEBYE) debye_eps_pair<PREC>(so.o[0].n, so.o[1].n, z, &deb0, &deb1);
        RIM_PROF_ADD(4, t_deb);
        RIM_PROF_T(t_mei);
        double mei0 = 0., mei1 = 0.;
        if (c0 & LSEL_MEISSEL) mei0 = meissel_first<PREC, true>(so.o[0], z);
        if (c1 & LSEL_MEISSEL) mei1 = meissel_first<PREC, true>(so.o[1], z);
        RIM_PROF_ADD(5, t_mei);
        if (!so.small) jv0 = leung_combine_code(c0, pos0, deb0, mei0);
        jv1 = leung_combine_code(c1, pos1, deb1, mei1);
    }
    if (so.small) {
        // the reference returns NaN for non-integer n < 30 (bessel.c:327-331)
        const int n_int = (int) n;
        if (!(n >= 0 && z >= 0) || (double) n_int != n) {
            jv0 = RIM_NAN; jv1 = RIM_NAN;
        } else {
            double a, b;
            RIM_HIT(16);
            RIM_PROF_T(t_mil);
            jn_int_pair(n_int, z, &a, &b);
            RIM_PROF_ADD(8, t_mil);
            jv0 = a;
            if (so.np1_small) jv1 = b;
        }
    }
    jn = jv0;
    const double jnp1 = jv1;
    if (so.dj_nan) { djn = RIM_NAN; return; }
    if (z == 0.) {
        if (n >= 2.) djn = 0.;
        else if (n == 0.) djn = -jnp1;
        else djn = n * jn / RIM_DBL_MIN - jnp1;
        return;
    }
    djn = n * jn / z - jnp1;
}

// The same pair from the complete functions of the Bessel seam (bessel_j / bessel_dj: any z, as the reference's
// pkgw_bessel_j / pkgw_bessel_dj).  sym_bessel_pair above covers what the kinematics allow, z <= n (and z <= 5e4 below
// order 30), and answers NaN beyond; where both are defined they return the same bits.  Selected by the type of the
// order record, so that gamma_integrand_shared is one text for both.
struct SymOrderFull { double n; };

template <int PREC = 0>
RIM_DEV void sym_bessel_pair(const SymOrderFull &so, double z, double &jn, double &djn)
{
    jn = bessel_j(so.n, z);
    djn = bessel_dj(so.n, z);
}

// gamma_integrand (symphony.rs:398-479) in three pieces, so that the coefficients of one parameter point can share
// the part that depends on (s, theta, n, gamma) only -- the kinematics and the Bessel pair, symphony.rs:406-442 -- and
// differ in the polarisation term (:444-448) and the distribution term (:455-463): symphony_group.h.
struct GiShared {
    double gamma, beta, cos_xi;
    double mj, njp;             // M J_n(z), N J'_n(z)
};

// ORDER: SymOrder, or SymOrderFull for the complete functions of the Bessel seam (sym_bessel_pair above).
template <int PREC = 0, class ORDER = SymOrder>
RIM_DEV GiShared gamma_integrand_shared(double s, double cos_th, double sin_th, const ORDER &so, double gamma)
{
    const double n = so.n;

    const double beta = rim_sqrt(1. - rim_div_moderate(1., gamma * gamma));
    // (numerators that can be exactly 0 give the IEEE signed zero through the bare sequence too)
    const double cos_xi = rim_div_moderate(s * gamma - n, s * gamma * beta * cos_th);
    const double sin_xi = rim_sqrt(1. - cos_xi * cos_xi);
    const double m = rim_div_moderate(cos_th - beta * cos_xi, sin_th);
    const double big_n = beta * sin_xi;

    double gamma_sin_xi;
    if (beta < 0.1) {
        RIM_HIT(14);
        gamma_sin_xi = gamma * sin_xi;
    } else {
        RIM_HIT(15);
        const double bc = beta * cos_th;
        const double beta2_costh2 = bc * bc;
        const double s_on_r = rim_div_moderate(2. * n, s * (beta2_costh2 - 1.));
        const double r = 1. - rim_div_moderate(1., beta2_costh2);
        gamma_sin_xi = rim_sqrt(r * (gamma * (gamma + s_on_r)) - rim_div_moderate(n * n, s * s * beta2_costh2));
    }

    const double z = s * beta * sin_th * gamma_sin_xi;

    double jn, djn;
    { RIM_PROF_T(t_cal); RIM_PROF_ADD(10, t_cal); }     // empty region: the timers' own cost
    RIM_PROF_T(t_bes);
    sym_bessel_pair<PREC>(so, z, jn, djn);
    RIM_PROF_ADD(2, t_bes);
    GiShared sh;
    sh.gamma = gamma; sh.beta = beta; sh.cos_xi = cos_xi;
    sh.mj = m * jn;
    sh.njp = big_n * djn;
    return sh;
}

RIM_DEV double gamma_integrand_pol_term(int stokes, double mj, double njp)
{
    if (stokes == STOKES_I) return mj * mj + njp * njp;
    if (stokes == STOKES_Q) return mj * mj - njp * njp;
    return 2. * mj * njp;
}

template <int KIND, int PREC = 0>
RIM_DEV double gamma_integrand_f_term(int coeff, const DistParams &d, double cos_th, const GiShared &sh)
{
    const double gamma = sh.gamma, beta = sh.beta, cos_xi = sh.cos_xi;
    if (coeff == COEFF_EMISSION) {
        RIM_HIT(24);
        return calc_f<KIND, PREC>(d, gamma, cos_xi);
    }
    double dfdg, dfdcx;
    RIM_HIT(25);
    calc_f_derivatives<KIND, PREC>(d, gamma, cos_xi, dfdg, dfdcx);
    if (KIND == DIST_POWER_LAW || KIND == DIST_THERMAL_JUETTNER || (dist_is_tab(KIND) && !tab_kind_has_pitch<KIND>(d))) {
        // dfdcx is the constant +0 (isotropic distributions; a table with a pitch row takes the general form below):
        // dfdcx_factor * dfdcx is a zero with the sign of the factor (a NaN only where the sample is a NaN through cos_xi
        // anyway), and for gamma > 0 the factor (beta cos_th - cos_xi) / (gamma - 1 / gamma) has the sign of
        // (beta cos_th - cos_xi) (gamma - 1): the same bits -- signed zeros of f_term included -- without the two divisions.
        return dfdg + ((beta * cos_th - cos_xi) * dfdcx) * (gamma - 1.);
    }
    const double dfdcx_factor = (beta * cos_th - cos_xi) / (gamma - 1. / gamma);
    return dfdg + dfdcx_factor * dfdcx;
}

// calc_f AND calc_f_derivatives of one sample (the emission and absorption members of a group, symphony_group.h): the
// values calc_f / calc_f_derivatives return, bit for bit, with what the two have in common computed once -- the
// double-double logarithm of gamma of the power-law energy factor (rim_powexp_from_log), the exponential of the thermal
// distribution, and for the anisotropic distributions f itself, which calc_f_derivatives forms by calc_f's own expression
// (pitchy_pl.rs:56-61, pitchy_kappa.rs:53-58).
template <int KIND>
RIM_DEV void calc_f_both(const DistParams &d, double gamma, double cos_xi, double &f, double &dfdg, double &dfdcx)
{
    if (dist_is_tab(KIND)) {
        tab_calc_f_both<KIND>(d, gamma, cos_xi, f, dfdg, dfdcx);
        return;
    }
    if (KIND == DIST_POWER_LAW) {
        f = 0.; dfdg = 0.; dfdcx = 0.;
        if (gamma < d.par[1] || gamma > d.par[2]) return;
        RIM_HIT(19); RIM_HIT(20);
        double ll;
        const double lh = rim_log_dd_normal(gamma, &ll);
        const double e = -gamma * d.inv_gamma_cutoff;
        const double beta = rim_sqrt(1. - rim_div_moderate(1., gamma * gamma));
        f = d.norm * rim_powexp_from_log(lh, ll, -d.par[0], e) / (gamma * gamma * beta);
        const double p_plus_1 = d.par[0] + 1.;
        const double g2_minus_1 = gamma * gamma - 1.;
        dfdg = -d.norm * rim_powexp_from_log(lh, ll, -p_plus_1, e) / rim_sqrt(g2_minus_1) *
            (p_plus_1 / gamma + gamma / g2_minus_1 + d.inv_gamma_cutoff);
    } else if (KIND == DIST_THERMAL_JUETTNER) {
        f = d.norm * RimMath<0>::exp(d.neg_inverse_t * gamma);
        dfdg = f * d.neg_inverse_t;
        dfdcx = 0.;
    } else if (KIND == DIST_PITCHY_PL) {
        f = 0.; dfdg = 0.; dfdcx = 0.;
        if (gamma < d.par[2] || gamma > d.par[3]) return;
        const double p = d.par[0], k = d.par[1];
        const double sin_xi = rim_sqrt(1. - cos_xi * cos_xi);
        const double pa_term = RimMath<0>::pow(sin_xi, k);
        const double beta = rim_sqrt(1. - rim_div_moderate(1., gamma * gamma));
        const double gamma_term = RimMath<0>::powexp_normal(gamma, -p, -gamma * d.inv_gamma_cutoff);
        f = d.norm * pa_term * gamma_term / (gamma * gamma * beta);
        dfdg = -f * ((p + 1.) / gamma + gamma / (gamma * gamma - 1.) + d.inv_gamma_cutoff);
        dfdcx = -f * k * cos_xi / (sin_xi * sin_xi);
    } else {
        const double kappa = d.par[0], width = d.par[1], k = d.par[2];
        const double sin_xi = rim_sqrt(1. - cos_xi * cos_xi);
        const double pa_term = RimMath<0>::pow(sin_xi, k);
        const double gamma_term = kappa_gamma_term<0>(d, gamma);
        f = d.norm * pa_term * gamma_term;
        dfdg = -f * ((kappa + 1.) / (kappa * width + gamma - 1.) + d.inv_gamma_cutoff);
        dfdcx = -f * k * cos_xi / (sin_xi * sin_xi);
    }
}

// the emission and the absorption f_term of one sample (symphony.rs:455-463) from calc_f_both
template <int KIND>
RIM_DEV void gamma_integrand_f_terms(const DistParams &d, double cos_th, const GiShared &sh, double &f_em, double &f_ab)
{
    const double gamma = sh.gamma, beta = sh.beta, cos_xi = sh.cos_xi;
    double dfdg, dfdcx;
    RIM_HIT(24); RIM_HIT(25);
    calc_f_both<KIND>(d, gamma, cos_xi, f_em, dfdg, dfdcx);
    if (KIND == DIST_POWER_LAW || KIND == DIST_THERMAL_JUETTNER || (dist_is_tab(KIND) && !tab_kind_has_pitch<KIND>(d))) {
        f_ab = dfdg + ((beta * cos_th - cos_xi) * dfdcx) * (gamma - 1.);       // (gamma_integrand_f_term says why)
    } else {
        const double dfdcx_factor = (beta * cos_th - cos_xi) / (gamma - 1. / gamma);
        f_ab = dfdg + dfdcx_factor * dfdcx;
    }
}

template <int KIND, int PREC = 0, class ORDER = SymOrder>
RIM_DEV double gamma_integrand(const SymPoint &pt, const DistParams &d, const ORDER &so, double gamma)
{
    const GiShared sh = gamma_integrand_shared<PREC, ORDER>(pt.s, pt.cos_th, pt.sin_th, so, gamma);
    RIM_PROF_T(t_f);
    const double pol_term = gamma_integrand_pol_term(pt.stokes, sh.mj, sh.njp);
    const double f_term = gamma_integrand_f_term<KIND, PREC>(pt.coeff, d, pt.cos_th, sh);
    RIM_PROF_ADD(6, t_f);
    return gamma * gamma * pol_term * f_term;
}

}  // namespace rim
#endif
