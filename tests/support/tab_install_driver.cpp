// CPU driver of tab_install.h (tests only): the host build of the per-line work of a 2-D set installed from device memory,
// looped over the line indices the way the kernels' grid-stride loop visits them, next to the host builders of tab_spline.h
// on the same numbers; and the geometry-only checks next to the full ones.
#include <cstring>
#include <vector>
#include "../../rimphony_amd/csrc/tab_spline.h"
#include "../../rimphony_amd/csrc/tab_install.h"

// what rimphony_ctx_set_tables_2d_device makes of its arguments: gamma null, nodes uniform in ln gamma; mu null, uniform in mu
static int check_full(size_t nt, size_t nn, const double *gamma, double glo, double ghi, size_t nmu, const double *mu,
                      const double *log_n, const double *sin_k)
{
    if (mu) return rim_tab_check_2d_nodes(nt, nn, gamma, nmu, mu, log_n, sin_k);
    if (gamma) return sin_k ? rim_tab_check_2d_grid_pitchy(nt, nn, gamma, nmu, log_n, sin_k) : rim_tab_check_2d_grid(nt, nn, gamma, nmu, log_n);
    return sin_k ? rim_tab_check_2d_pitchy(nt, nn, glo, ghi, nmu, log_n, sin_k) : rim_tab_check_2d(nt, nn, glo, ghi, nmu, log_n);
}

static int check_geometry(size_t nt, size_t nn, const double *gamma, double glo, double ghi, size_t nmu, const double *mu,
                          const double *sin_k)
{
    if (mu) return rim_tab_check_2d_nodes_geometry(nt, nn, gamma, nmu, mu, sin_k);
    if (gamma ? rim_tab_check_2d_grid_geometry(nt, nn, gamma, nmu) : rim_tab_check_2d_geometry(nt, nn, glo, ghi, nmu)) return -1;
    return sin_k ? rim_tab_check_sin_k(nt, sin_k) : 0;
}

extern "C" {

// the verdicts of the full check (*full) and of the geometry-only check (*geometry) on one call; with_mu: the nodes form, whose
// mu may itself be the null pointer under test
int tabi_check(size_t nt, size_t nn, const double *gamma, double glo, double ghi, size_t nmu, const double *mu, int with_mu,
               const double *log_n, const double *sin_k, int *full, int *geometry)
{
    if (with_mu) {
        *full = rim_tab_check_2d_nodes(nt, nn, gamma, nmu, mu, log_n, sin_k);
        *geometry = rim_tab_check_2d_nodes_geometry(nt, nn, gamma, nmu, mu, sin_k);
        return 0;
    }
    *full = check_full(nt, nn, gamma, glo, ghi, nmu, nullptr, log_n, sin_k);
    *geometry = check_geometry(nt, nn, gamma, glo, ghi, nmu, nullptr, sin_k);
    return 0;
}

// The set of the form the arguments select, twice: host_out as the host builder lays it out, dev_out as the device path does --
// the front from rim_tab_front_2d*, the axis blocks from rim_tab_install_axis, then the three families of lines, each family
// visited as `lanes` lanes of a grid-stride loop would visit it.  Returns the size of the set in doubles (both outputs need
// that many; nothing is written where cap is smaller), or -1 where the full check refuses.
long long tabi_run(size_t nt, size_t nn, const double *gamma, double glo, double ghi, size_t nmu, const double *mu,
                   const double *log_n, const double *sin_k, size_t lanes, double *host_out, double *dev_out, size_t cap)
{
    if (check_full(nt, nn, gamma, glo, ghi, nmu, mu, log_n, sin_k)) return -1;
    if (check_geometry(nt, nn, gamma, glo, ghi, nmu, mu, sin_k)) return -2;
    std::vector<double> host, front, h, ih, hm, ihm;
    double hu = 0., hmu = 0.;
    if (mu) {
        rim_tab_build_2d_nodes(nt, nn, gamma, nmu, mu, log_n, sin_k, host);
        rim_tab_front_2d_nodes(nt, nn, gamma, nmu, mu, sin_k, front, h, ih, hm, ihm);
    } else if (gamma) {
        if (sin_k) rim_tab_build_2d_grid_pitchy(nt, nn, gamma, nmu, log_n, sin_k, host);
        else rim_tab_build_2d_grid(nt, nn, gamma, nmu, log_n, host);
        rim_tab_front_2d_grid(nt, nn, gamma, nmu, front, h, ih, hmu);
    } else {
        if (sin_k) rim_tab_build_2d_pitchy(nt, nn, glo, ghi, nmu, log_n, sin_k, host);
        else rim_tab_build_2d(nt, nn, glo, ghi, nmu, log_n, host);
        rim_tab_front_2d(nt, nn, glo, ghi, nmu, front, hu, hmu);
    }
    if (sin_k && !mu) rim_tab_put_2d_sin_k(nt, sin_k, front);
    const size_t total = front.size() + nt * nn * nmu * 4;
    if (total != host.size()) return -3;
    if (cap < total) return (long long) total;
    std::vector<double> axes(rim_tab_axis_doubles(nn) + rim_tab_axis_doubles(nmu), 0.);
    rim_tab_install_axis(nn, hu, gamma ? h.data() : nullptr, gamma ? ih.data() : nullptr, axes.data());
    rim_tab_install_axis(nmu, hmu, mu ? hm.data() : nullptr, mu ? ihm.data() : nullptr, axes.data() + rim_tab_axis_doubles(nn));
    // NaN-filled: a word the lines leave out cannot pass for a 0 of the host's
    memset(dev_out, 0xff, total * sizeof(double));
    memcpy(dev_out, front.data(), front.size() * sizeof(double));
    RimTabInstall s;
    s.log_n = log_n;
    s.nodes = dev_out + front.size();
    s.n_tables = nt; s.n_nodes = nn; s.n_mu = nmu;
    s.au = rim_tab_axis_of(axes.data(), nn, hu, gamma != nullptr);
    s.amu = rim_tab_axis_of(axes.data() + rim_tab_axis_doubles(nn), nmu, hmu, mu != nullptr);
    if (!lanes) lanes = 1;
    for (int family = 0; family < 3; family++) {
        const size_t lines = rim_tab_install_lines(s, family);
        for (size_t lane = 0; lane < lanes; lane++)
            for (size_t line = lane; line < lines; line += lanes) rim_tab_install_family_line(s, family, line);
    }
    memcpy(host_out, host.data(), total * sizeof(double));
    return (long long) total;
}

}
