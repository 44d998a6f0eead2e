// Host driver of csrc/knn_search.h for tests/test_nn_host.py: the order of pmi_knn_order_dev and the query of
// pmi_knn_query_dev, one query after the other on the CPU, through the very header the kernels are compiled from.
#include <math.h>
#include <stdint.h>

#include <vector>

#include "knn_search.h"

using namespace pmi::knn;

template <int D>
static void run(const Grid &g, const double *x1, int64_t n, const double *x2, int32_t m, int k, double *out,
                int32_t *cell_x, int32_t *cell_y)
{
    const int64_t cells = (int64_t)g.n[0] * g.n[1];
    std::vector<int32_t> start(cells + 1, 0);
    std::vector<int64_t> key(m);
    for (int32_t i = 0; i < m; ++i) {
        cell_x[i] = cell_of(g, 0, x2[(int64_t)i * D]);
        cell_y[i] = cell_of(g, 1, x2[(int64_t)i * D + 1]);
        key[i] = (int64_t)cell_y[i] * g.n[0] + cell_x[i];
        start[key[i] + 1]++;
    }
    for (int64_t c = 0; c < cells; ++c) start[c + 1] += start[c];
    std::vector<int32_t> at(start.begin(), start.end() - 1);
    std::vector<double> sorted((size_t)m * D);
    for (int32_t i = 0; i < m; ++i) {                                   // stable, like the radix sort
        const int32_t p = at[key[i]]++;
        for (int a = 0; a < D; ++a) sorted[(size_t)p * D + a] = x2[(int64_t)i * D + a];
    }
    std::vector<double> best(k);
    for (int64_t i = 0; i < n; ++i) {
        search<D>(g, start.data(), sorted.data(), m, x1 + i * D, k, Best{best.data(), 1});
        for (int j = 0; j < k; ++j) out[i * k + j] = sqrt(best[j]);
    }
}

extern "C" int nn_host_limit(void) { return K_MAX; }

// grid_n[2], grid_lo_w[4] receive the grid; cell_x / cell_y (m each) the cells of the rows of x2
extern "C" int nn_host(const double *x1, int64_t n, const double *x2, int64_t m, int dims, int k, double *out,
                       int32_t *grid_n, double *grid_lo_w, int32_t *cell_x, int32_t *cell_y)
{
    if ((dims != 2 && dims != 3) || k < 1 || k > K_MAX || m < 0 || n < 0) return -1;
    double lo[2] = {0, 0}, hi[2] = {0, 0};
    for (int64_t i = 0; i < m; ++i)
        for (int a = 0; a < 2; ++a) {
            const double v = x2[i * dims + a];
            if (i == 0 || v < lo[a]) lo[a] = v;
            if (i == 0 || v > hi[a]) hi[a] = v;
        }
    const Grid g = plan_grid(lo, hi, m, k);
    for (int a = 0; a < 2; ++a) grid_n[a] = g.n[a], grid_lo_w[a] = g.lo[a], grid_lo_w[2 + a] = g.w[a];
    if (dims == 2) run<2>(g, x1, n, x2, (int32_t)m, k, out, cell_x, cell_y);
    else run<3>(g, x1, n, x2, (int32_t)m, k, out, cell_x, cell_y);
    return 0;
}
