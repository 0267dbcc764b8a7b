// tab_blobs.cpp -- every builder of tab_spline.h on small sets, the blobs written to one file: build it against two versions
// of the header and `cmp` the files (profiles/tab_forms_isa_identity.txt).  Host only:
//   g++ -O2 -std=c++17 -ffp-contract=off -mfma -I rimphony_amd/csrc tools/tab_blobs.cpp -o tab_blobs && ./tab_blobs out.bin
// 1 and 3 tables of 8 and 9 nodes, n_mu = 8 and 9 where the form has one (and none where it may have none), one jittered
// node vector for the given-nodes form, sin_k = 0, 0.5 and 100.  Every check must pass; the program says how many blobs.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "tab_spline.h"

static FILE *g_out;
static int g_count;

static void put(const std::vector<double> &blob)
{
    const double n = (double) blob.size();
    fwrite(&n, sizeof n, 1, g_out);
    fwrite(blob.data(), sizeof(double), blob.size(), g_out);
    g_count++;
}

static void must(int rc) { if (rc) { fprintf(stderr, "a check refused a good set\n"); exit(1); } }

int main(int argc, char **argv)
{
    if (argc != 2 || !(g_out = fopen(argv[1], "wb"))) return 2;
    const double glo = 1.5, ghi = 3e4, sin_k[3] = { 0., 0.5, 100. };
    std::vector<double> blob;
    for (size_t n_tables : { 1, 3 })
        for (size_t n_nodes : { 8, 9 }) {
            std::vector<double> log_n(n_tables * n_nodes), gamma(n_nodes);
            for (size_t i = 0; i < log_n.size(); i++) log_n[i] = -2.5 * (double) (i % n_nodes) + 0.37 * (double) ((i * 7) % 5) - (double) (i / n_nodes);
            for (size_t j = 0; j < n_nodes; j++) gamma[j] = glo * (1. + 3.1 * (double) j * (double) j + 0.013 * (double) ((j * 5) % 3));
            must(rim_tab_check(n_tables, n_nodes, glo, ghi, log_n.data()));
            rim_tab_build(n_tables, n_nodes, glo, ghi, log_n.data(), blob);
            put(blob);
            for (size_t n_mu : { 0, 8, 9 }) {
                std::vector<double> log_g(n_tables * n_mu), log_n2(n_tables * n_nodes * n_mu);
                for (size_t i = 0; i < log_g.size(); i++) log_g[i] = 0.8 * (double) (i % n_mu) - 0.21 * (double) ((i * 3) % 7);
                for (size_t i = 0; i < log_n2.size(); i++) log_n2[i] = -0.3 * (double) (i / n_mu % n_nodes) + 0.11 * (double) ((i * 11) % 13);
                const double *g = n_mu ? log_g.data() : nullptr;
                must(rim_tab_check_pitch(n_tables, n_nodes, glo, ghi, log_n.data(), n_mu, g));
                rim_tab_build_pitch(n_tables, n_nodes, glo, ghi, log_n.data(), n_mu, g, blob);
                put(blob);
                must(rim_tab_check_pitchy(n_tables, n_nodes, glo, ghi, log_n.data(), n_mu, g, sin_k));
                rim_tab_build_pitchy(n_tables, n_nodes, glo, ghi, log_n.data(), n_mu, g, sin_k, blob);
                put(blob);
                for (const double *k : { sin_k, (const double *) nullptr }) {
                    must(rim_tab_check_grid(n_tables, n_nodes, gamma.data(), log_n.data(), n_mu, g, k));
                    rim_tab_build_grid(n_tables, n_nodes, gamma.data(), log_n.data(), n_mu, g, k, blob);
                    put(blob);
                }
                if (!n_mu) continue;
                must(rim_tab_check_2d(n_tables, n_nodes, glo, ghi, n_mu, log_n2.data()));
                rim_tab_build_2d(n_tables, n_nodes, glo, ghi, n_mu, log_n2.data(), blob);
                put(blob);
            }
        }
    // what the shared checks refuse: ranges and sin_k values, good and bad, through every check that looks at them
    std::vector<double> y(3 * 8 * 8, -1.), nodes = { 1., 2., 3., 4., 5., 6., 7., 8. }, verdicts;
    const double ranges[][2] = { { 1., 2. }, { 0.5, 2. }, { 2., 2. }, { 3., 2. }, { 1., HUGE_VAL }, { NAN, 2. }, { 1., NAN } };
    for (const auto &r : ranges) {
        verdicts.push_back(rim_tab_check(3, 8, r[0], r[1], y.data()));
        verdicts.push_back(rim_tab_check_2d(3, 8, r[0], r[1], 8, y.data()));
    }
    const double ks[][3] = { { 0., 0.5, 100. }, { 0., 0.5, 100.5 }, { -0.5, 0., 0. }, { 0., NAN, 0. }, { 0., 0., HUGE_VAL } };
    for (const auto &k : ks) {
        verdicts.push_back(rim_tab_check_pitchy(3, 8, 1., 2., y.data(), 0, nullptr, k));
        verdicts.push_back(rim_tab_check_grid(3, 8, nodes.data(), y.data(), 0, nullptr, k));
    }
    verdicts.push_back(rim_tab_check_pitchy(3, 8, 1., 2., y.data(), 0, nullptr, nullptr));
    verdicts.push_back(rim_tab_check_grid(3, 8, nodes.data(), y.data(), 0, nullptr, nullptr));
    put(verdicts);
    fclose(g_out);
    printf("%d blobs\n", g_count);
    return 0;
}
