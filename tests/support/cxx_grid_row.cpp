// The C++ mirror on a table set on given gamma nodes, for tests/test_gpu_tabulated_grid.py: reads a text file of
// hexadecimal floats -- n_nodes, the nodes, ln n at the nodes, then sin_k, s and theta --, computes the row through
// Context::set_tables_grid + BatchCalculator and through TabulatedDistributionGrid, and prints both as hexadecimal floats.
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <vector>
#include "../../rimphony_amd/cxx/rimphony.hpp"

using namespace rimphony;

static double next(FILE *f)
{
    char word[64];
    if (fscanf(f, "%63s", word) != 1) { fprintf(stderr, "short input\n"); exit(2); }
    return strtod(word, nullptr);
}

int main(int argc, char **argv)
{
    if (argc != 2) return 2;
    FILE *f = fopen(argv[1], "r");
    if (!f) return 2;
    const size_t n = (size_t) next(f);
    std::vector<double> gamma(n), log_n(n);
    for (auto &x : gamma) x = next(f);
    for (auto &x : log_n) x = next(f);
    const double k = next(f), s = next(f), theta = next(f);
    fclose(f);
    try {
        auto ctx = std::make_shared<Context>(0);
        ctx->set_tables_grid(1, gamma, log_n, 0, {}, {k});
        const auto row = BatchCalculator(ctx, RIMPHONY_TABULATED).compute({s}, {theta}, {{0.}});
        for (int i = 0; i < 8; i++) printf("%a ", row[i]);
        printf("\n");
        ctx->set_tables_grid(0, {}, {});
        const auto all = TabulatedDistributionGrid(gamma, log_n, {}, k).full_calculation(ctx).compute_all_dimensionless(s, theta);
        for (int i = 0; i < 8; i++) printf("%a ", all[i]);
        printf("\n");
    } catch (const std::exception &e) {
        fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    return 0;
}
