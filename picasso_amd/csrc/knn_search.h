// knn_search.h — the search of one query for its k nearest rows of a cell-sorted set (knn.hip), written so that the
// host compiler takes it too (tests/test_nn_host.py builds it into a small shared object): the grid of a set, the cell
// of a coordinate, the walk over Chebyshev rings of cells, the stopping bound, the insertion and the inf padding.
//
// Grid.  nx x ny cells over the x / y bounding box of the set (z, when there is one, enters the distance only).  The
// edges of axis a are the float64 values edge(a, i) = lo[a] + i * w[a], i = 1 .. n[a] - 1, non-decreasing in i (a
// product and a sum, each rounded once, are monotone).  cell_of(a, c) is the one i with edge(a, i) <= c < edge(a, i + 1),
// where edge(a, 0) counts as -inf and edge(a, n[a]) as +inf: it is found by COMPARING c with these values (the rounded
// division is only the first guess), so that a row of cell i satisfies both inequalities in float64, exactly.
//
// Bound.  After the rings 0 .. r around the query's cell (cx, cy) every unvisited row lies in a cell column >= cx + r + 1
// or <= cx - r - 1, or in such a cell row.  For a row p in a column >= cx + r + 1 =: j (it exists only when j <= nx - 1):
// p.x >= edge(j) and, because cx < nx - 1, q.x < edge(cx + 1) <= edge(j); so p.x - q.x >= edge(j) - q.x > 0 in the
// reals, rounding is monotone, |fl(q.x - p.x)| >= fl(edge(j) - q.x) =: b >= 0, fl(dx * dx) >= fl(b * b), and adding
// the non-negative dy * dy (and dz * dz) and rounding cannot go below fl(dx * dx), which is representable.  The other
// three sides are the same with edge(cx - r) <= q.x.  The bound of the ring is the smallest fl(b * b) over the sides
// that still have cells, +inf when none has.  The search stops when the k-th best sum of squares is <= that bound: an
// unvisited row then has a sum >= the k-th best, it could at most tie with it, and a tie leaves the k values as they are.
//
// Arithmetic.  float64 differences, squares, the sum in column order, no contraction; the caller takes the root.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define KNN_HD __host__ __device__ __forceinline__
#else
#define KNN_HD inline
#endif

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace pmi {
namespace knn {

constexpr int K_MAX = 32;                 // neighbours per query, the dropped self column included

struct Grid {
    double lo[2], w[2];
    int32_t n[2];                         // >= 1 each, n[0] * n[1] <= max(rows of the set, 1)
};

// the k best sums of one query, ascending: entry j at p[j * stride]
struct Best {
    double *p;
    int32_t stride;
    KNN_HD double get(int j) const { return p[(int64_t)j * stride]; }
    KNN_HD void set(int j, double v) const { p[(int64_t)j * stride] = v; }
};

KNN_HD double infinity() { return __builtin_huge_val(); }

// Cells of about max(2, (k + 1) / 2) rows: the nine cells around a query then hold a few times k rows.  At most
// max(m, 1) cells in all, split between the axes by the box's aspect; an axis without a usable extent is one cell.
KNN_HD Grid plan_grid(const double lo[2], const double hi[2], int64_t m, int64_t k)
{
    const int64_t per_cell = (k + 1) / 2 > 2 ? (k + 1) / 2 : 2;
    const int64_t cells = m / per_cell > 1 ? m / per_cell : 1;
    double ext[2];
    bool flat[2];
    for (int a = 0; a < 2; ++a) {
        ext[a] = hi[a] - lo[a];
        flat[a] = !(ext[a] > 0.0 && ext[a] < infinity());
    }
    int64_t n[2] = {1, 1};
    if (!flat[0] && flat[1]) n[0] = cells;
    if (flat[0] && !flat[1]) n[1] = cells;
    if (!flat[0] && !flat[1]) {
        const double t = __builtin_sqrt((double)cells * (ext[0] / ext[1]));
        n[0] = t >= (double)cells ? cells : (t >= 1.0 ? (int64_t)t : 1);
        n[1] = cells / n[0] > 1 ? cells / n[0] : 1;
    }
    Grid g;
    for (int a = 0; a < 2; ++a) {
        double w = flat[a] ? 1.0 : ext[a] / (double)n[a];
        if (!(w > 0.0)) { w = 1.0; n[a] = 1; }         // the width underflowed
        g.lo[a] = lo[a];
        g.w[a] = w;
        g.n[a] = (int32_t)n[a];
    }
    return g;
}

KNN_HD double edge(const Grid &g, int a, int64_t i)
{
    const double step = (double)i * g.w[a];
    return g.lo[a] + step;
}

// at most n[a] steps behind the first guess; one at the most unless the cells are narrower than the coordinates' spacing
KNN_HD int32_t cell_of(const Grid &g, int a, double c)
{
    const int32_t last = g.n[a] - 1;
    const double t = (c - g.lo[a]) / g.w[a];
    int32_t i = t >= (double)last ? last : (t > 0.0 ? (int32_t)t : 0);
    for (int32_t it = 0; it < last && i > 0 && c < edge(g, a, i); ++it) --i;
    for (int32_t it = 0; it < last && i < last && c >= edge(g, a, (int64_t)i + 1); ++it) ++i;
    return i;
}

// min(bound, d * d) for the distance d >= 0 to a side of the visited square (a d below 0 cannot be: it bounds nothing)
KNN_HD double lower(double bound, double d)
{
    const double d2 = d > 0.0 ? d * d : 0.0;
    return d2 < bound ? d2 : bound;
}

template <int D>
KNN_HD double sum_of_squares(const double *q, const double *p)
{
    const double dx = q[0] - p[0];
    const double dy = q[1] - p[1];
    double s = dx * dx;
    s = s + dy * dy;
    if (D == 3) {
        const double dz = q[2] - p[2];
        s = s + dz * dz;
    }
    return s;
}

// rows [a, b) of the sorted set against the query; *kth is best.get(k - 1)
template <int D>
KNN_HD void scan_rows(const double *pts, int32_t a, int32_t b, const double *q, int k, const Best &best, double *kth)
{
    for (int32_t j = a; j < b; ++j) {
        const double s = sum_of_squares<D>(q, pts + (int64_t)j * D);
        if (!(s < *kth)) continue;
        int at = k - 1;
        while (at > 0 && best.get(at - 1) > s) {
            best.set(at, best.get(at - 1));
            --at;
        }
        best.set(at, s);
        *kth = best.get(k - 1);
    }
}

// The k smallest sums of squares between q and the m rows `pts` (row-major, D columns, sorted by cell iy * nx + ix),
// ascending, +inf where the set has fewer than k rows.  start[c] is the first sorted row of cell c, start[nx * ny] = m.
template <int D>
KNN_HD void search(const Grid &g, const int32_t *start, const double *pts, int32_t m, const double *q, int k,
                   const Best &best)
{
    for (int j = 0; j < k; ++j) best.set(j, infinity());
    double kth = infinity();
    const int64_t nx = g.n[0], ny = g.n[1];
    const int64_t cx = cell_of(g, 0, q[0]), cy = cell_of(g, 1, q[1]);
    int64_t r_max = cx > nx - 1 - cx ? cx : nx - 1 - cx;
    if (cy > r_max) r_max = cy;
    if (ny - 1 - cy > r_max) r_max = ny - 1 - cy;
    for (int64_t r = 0; r <= r_max; ++r) {
        const int64_t x0 = cx - r > 0 ? cx - r : 0, x1 = cx + r < nx - 1 ? cx + r : nx - 1;
        const int64_t y0 = cy - r > 0 ? cy - r : 0, y1 = cy + r < ny - 1 ? cy + r : ny - 1;
        for (int64_t iy = y0; iy <= y1; ++iy) {
            const int64_t row = iy * nx;
            // the ring's top and bottom rows are one run of cells each, the rows between them its two end cells
            const bool whole = iy == cy - r || iy == cy + r;
            for (int side = 0; side < 2; ++side) {
                int64_t c0, c1;
                if (whole) {
                    if (side) break;
                    c0 = x0, c1 = x1;
                } else {
                    c0 = c1 = side ? cx + r : cx - r;
                    if (c0 < 0 || c0 > nx - 1) continue;
                }
                int32_t a = start[row + c0], b = start[row + c1 + 1];
                if (a < 0) a = 0;
                if (b > m) b = m;
                scan_rows<D>(pts, a, b, q, k, best, &kth);
            }
        }
        double bound = infinity();
        if (cx + r + 1 <= nx - 1) bound = lower(bound, edge(g, 0, cx + r + 1) - q[0]);
        if (cx - r - 1 >= 0) bound = lower(bound, q[0] - edge(g, 0, cx - r));
        if (cy + r + 1 <= ny - 1) bound = lower(bound, edge(g, 1, cy + r + 1) - q[1]);
        if (cy - r - 1 >= 0) bound = lower(bound, q[1] - edge(g, 1, cy - r));
        if (kth <= bound) break;
    }
}

}  // namespace knn
}  // namespace pmi
