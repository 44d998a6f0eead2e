// knn.hip — the distances from every row of one point set to its k nearest rows of another (picasso/postprocess.py:3704-3739
// nn_analysis, picasso/spinna.py:696-747 get_NN_dist: scipy.spatial.KDTree(X2).query(X1, k)), equal in every bit.
//
// What is computed.  Both sets are float64 (the host converts, as scipy does).  A distance is sqrt(dx * dx + dy * dy
// (+ dz * dz)) with float64 differences, squares, the sum in column order, no contraction and a correctly rounded root.
// A query's row holds its k smallest distances in ascending order, +inf where the set has fewer than k rows.  The k
// smallest VALUES do not depend on how ties between rows are broken, and no index is returned.
//
// Order (pmi_knn_order_dev).  The set is sorted by the cell of its x / y coordinates in a uniform grid over its
// bounding box (knn_search.h: plan_grid, cell_of), key = iy * nx + ix, with the stable radix sort on the bits the
// largest key needs; the rows are gathered into that order and start[c] = the first sorted row of cell c (one bisection
// per cell).  There are at most max(m, 1) cells, so the table of starts is O(rows) like everything else.
//
// Query (pmi_knn_query_dev).  One lane per query: its cell, clamped into the grid, then Chebyshev rings of cells
// outwards until the k-th best sum of squares is <= the bound of knn_search.h on every unvisited row.  The k best sums
// of a lane live in LDS, entry j of lane t at best[j * QUERY_BLOCK + t] (consecutive lanes, consecutive 8-byte words).
// Every loop is bounded by the rows of the set and the cells of the grid.  No atomics.
#include "knn_search.h"
#include "rows_common.h"

#pragma clang fp contract(off)

namespace pmi {
namespace knn {

using namespace rows;

constexpr int QUERY_BLOCK = 128;         // K_MAX * QUERY_BLOCK * 8 B = 32 KB of LDS

static_assert(sizeof(Grid) == sizeof(pmi_knn_grid), "pmi_knn_grid is knn::Grid");

__device__ __forceinline__ double sqrt_rn(double a) { return __builtin_sqrt(a); }

template <int D>
__global__ void key_kernel(Grid g, const double *__restrict__ x, int32_t m, uint32_t *__restrict__ keys,
                           int32_t *__restrict__ rows)
{
    const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= m) return;
    const int64_t cx = cell_of(g, 0, x[i * D]), cy = cell_of(g, 1, x[i * D + 1]);
    keys[i] = (uint32_t)(cy * g.n[0] + cx);
    rows[i] = (int32_t)i;
}

template <int D>
__global__ void gather_kernel(const double *__restrict__ x, const int32_t *__restrict__ rows, int32_t m,
                              double *__restrict__ sorted)
{
    const int64_t p = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (p >= m) return;
    const int32_t i = rows[p];
    const bool ok = i >= 0 && i < m;                                  // not a permutation: nothing is read out of bounds
    for (int a = 0; a < D; ++a) sorted[p * D + a] = ok ? x[(int64_t)i * D + a] : 0.0;
}

// start[c] for c = 0 .. cells
__global__ void start_kernel(const uint32_t *__restrict__ keys, int32_t m, int64_t cells, int32_t *__restrict__ start)
{
    const int64_t c = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (c > cells) return;
    start[c] = lower_bound(keys, 0, m, (uint32_t)c);
}

template <int D>
__global__ void __launch_bounds__(QUERY_BLOCK)
query_kernel(Grid g, const int32_t *__restrict__ start, const double *__restrict__ sorted, int32_t m,
             const double *__restrict__ x1, int32_t n, int k, double *__restrict__ out)
{
    extern __shared__ double best_lds[];
    const int64_t i = (int64_t)blockIdx.x * QUERY_BLOCK + threadIdx.x;
    if (i >= n) return;
    double q[D];
    for (int a = 0; a < D; ++a) q[a] = x1[i * D + a];
    const Best best{best_lds + threadIdx.x, QUERY_BLOCK};
    search<D>(g, start, sorted, m, q, k, best);
    for (int j = 0; j < k; ++j) out[i * k + j] = sqrt_rn(best.get(j));
}

// ---- host ------------------------------------------------------------------------------------------------------
static int check_sizes(const char *what, int dims, int64_t rows_, int64_t k)
{
    if ((dims != 2 && dims != 3) || rows_ < 0 || rows_ > INT32_MAX - 1 || k < 1 || k > K_MAX) {
        set_error("%s: %d columns (2 or 3), %lld rows (indexed with int32), k = %lld (1 .. %d)", what, dims,
                  (long long)rows_, (long long)k, K_MAX);
        return PMI_ERR_ARG;
    }
    return PMI_OK;
}

static int check_grid(const char *what, const Grid &g, int64_t m)
{
    const int64_t cells = (int64_t)g.n[0] * g.n[1];
    bool ok = g.n[0] >= 1 && g.n[1] >= 1 && cells <= std::max<int64_t>(m, 1);
    for (int a = 0; a < 2; ++a) ok = ok && g.w[a] > 0.0 && g.w[a] < infinity() && g.lo[a] - g.lo[a] == 0.0;
    if (!ok) {
        set_error("%s: a grid of %d x %d cells of %g x %g for %lld rows", what, g.n[0], g.n[1], g.w[0], g.w[1], (long long)m);
        return PMI_ERR_ARG;
    }
    return PMI_OK;
}

template <int D>
static int order(const double *x2, int32_t m, const Grid &g, double *sorted, int32_t *start, hipStream_t s)
{
    const size_t M = (size_t)m;
    const int64_t cells = (int64_t)g.n[0] * g.n[1];
    uint32_t *keys, *keys_out;
    int32_t *rows, *rows_out;
    int rc = carve(SCR_STAGE_A, [&](Arena &ar) {
        keys = ar.take<uint32_t>(M), keys_out = ar.take<uint32_t>(M);
        rows = ar.take<int32_t>(M), rows_out = ar.take<int32_t>(M);
    });
    if (rc != PMI_OK) return rc;
    PMI_LAUNCH(key_kernel<D>, m, s, g, x2, m, keys, rows);
    if ((rc = sort_pairs(keys, keys_out, rows, rows_out, M, bits_of((uint64_t)(cells - 1)), s)) != PMI_OK) return rc;
    PMI_LAUNCH(gather_kernel<D>, m, s, x2, rows_out, m, sorted);
    PMI_LAUNCH(start_kernel, cells + 1, s, keys_out, m, cells, start);
    PMI_HIP(hipStreamSynchronize(s));
    return PMI_OK;
}

template <int D>
static int query(const double *x1, int32_t n, const Grid &g, const int32_t *start, const double *sorted, int32_t m,
                 int k, double *out, hipStream_t s)
{
    const unsigned grid = (unsigned)(((int64_t)n + QUERY_BLOCK - 1) / QUERY_BLOCK);
    query_kernel<D><<<grid, QUERY_BLOCK, sizeof(double) * QUERY_BLOCK * (size_t)k, s>>>(g, start, sorted, m, x1, n, k, out);
    PMI_HIP(hipGetLastError());
    PMI_HIP(hipStreamSynchronize(s));
    return PMI_OK;
}

}  // namespace knn
}  // namespace pmi

using namespace pmi;

extern "C" {

int pmi_knn_limit(void) { return knn::K_MAX; }

int pmi_knn_order_dev(const double *d_x2, int dims, int64_t m, const double *lo, const double *hi, int64_t k,
                      double *d_sorted, int32_t *d_start, pmi_knn_grid *grid, void *stream)
{
    int rc = knn::check_sizes("pmi_knn_order_dev", dims, m, k);
    if (rc) return rc;
    if (!lo || !hi || !grid || !d_start || (m > 0 && (!d_x2 || !d_sorted))) {
        set_error("pmi_knn_order_dev: NULL argument");
        return PMI_ERR_ARG;
    }
    const knn::Grid g = knn::plan_grid(lo, hi, m, k);
    if ((rc = knn::check_grid("pmi_knn_order_dev", g, m))) return rc;
    memcpy(grid, &g, sizeof g);
    if (m == 0) {                                                   // one empty cell
        PMI_HIP(hipMemsetAsync(d_start, 0, 2 * sizeof(int32_t), (hipStream_t)stream));
        PMI_HIP(hipStreamSynchronize((hipStream_t)stream));
        return PMI_OK;
    }
    return dims == 2 ? knn::order<2>(d_x2, (int32_t)m, g, d_sorted, d_start, (hipStream_t)stream)
                     : knn::order<3>(d_x2, (int32_t)m, g, d_sorted, d_start, (hipStream_t)stream);
}

int pmi_knn_query_dev(const double *d_x1, int dims, int64_t n, const double *d_sorted, const int32_t *d_start, int64_t m,
                      const pmi_knn_grid *grid, int64_t k, double *d_out, void *stream)
{
    int rc = knn::check_sizes("pmi_knn_query_dev", dims, n, k);
    if (rc || (rc = knn::check_sizes("pmi_knn_query_dev", dims, m, k))) return rc;
    if (!grid || !d_start || (m > 0 && !d_sorted) || (n > 0 && (!d_x1 || !d_out))) {
        set_error("pmi_knn_query_dev: NULL argument");
        return PMI_ERR_ARG;
    }
    knn::Grid g;
    memcpy(&g, grid, sizeof g);
    if ((rc = knn::check_grid("pmi_knn_query_dev", g, m))) return rc;
    if (n == 0) return PMI_OK;
    return dims == 2 ? knn::query<2>(d_x1, (int32_t)n, g, d_start, d_sorted, (int32_t)m, (int)k, d_out, (hipStream_t)stream)
                     : knn::query<3>(d_x1, (int32_t)n, g, d_start, d_sorted, (int32_t)m, (int)k, d_out, (hipStream_t)stream);
}

}  // extern "C"
