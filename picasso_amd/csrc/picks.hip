// picks.hip — the member rows of every pick of one call (picasso/postprocess.py:207-372 _picked_circular_locs,
// _picked_rectangular_locs, _picked_polygonal_locs, _picked_square_locs; :849-928 _get_block_locs_at_numba,
// _locs_at_numba; picasso/lib.py:1884-2004 check_if_in_polygon, check_if_in_rectangle), row for row and in the order
// the reference holds them in before its sort by frame.
//
// One workgroup per pick, all picks in one launch.  A pick walks a few runs of rows in a block order (the sorted keys of
// pmi_pairs_order_dev, read through rows_blocks.h: a run is two bisections, there is no K x L table; a circle's blocks
// are that header's clamped 3 x 3 window), tests 256 rows at a time and compacts the
// members in run order: a ballot per wave, the four wave counts through LDS.  The same kernel counts (members == NULL)
// and writes; between the two the host scans the counts into offsets[P + 1] and reads the total, which sizes `members`.
//
// Circle.  The table is the sanity-filtered one in the order of get_index_blocks.  A pick at block (y_, x_) walks the
// blocks k = y_ - 1 .. y_ + 1, l = x_ - 1 .. x_ + 1 inside the grid, k outside l; the rows of (k, l0 .. l1) are one
// run.  Only the positions < p are visible (the reference's table stops filling at the first row outside the grid).  A
// member has dx ** 2 + dy ** 2 < r2, strict.  The host decides the types from the scalars it was given (numba's typing
// for picked_locs, NumPy's for lib.is_loc_at): flags bit 0 / bit 1 keep the x / y difference and its square in float32
// when that column is float32 (an integer or float32 pick coordinate; the host clears both bits when the reference
// stacks a float32 and a float64 column into one float64 array), else they are float64; the sum of two float32 squares
// is float32 and is compared with float32(r2) when bit 2 is set (an integer or float32 radius), else in float64.
//
// Square, Rectangle, Polygon.  The reference masks the whole table per pick; here the rows are binned once on a grid
// that covers every pick's bounding box (pmi_picks_cells_dev; a row outside it, NaN included, is in no pick, gets the
// block (CY, 0) and so lies behind p), and a pick walks the cell rows under its box.  First the strict box
// x_min < x < x_max, y_min < y < y_max: bit b of the pick's flags says that bound b (x_min, x_max, y_min, y_max) is a
// weak Python scalar, compared in the column's own type (a float32 column against float32(bound)); otherwise in
// float64.  Then, in float64 and in the reference's order of operations: nothing (Square), the ray count over the four
// sides (Rectangle), the ray casting over the corners (Polygon).  Members come out in cell order and a segmented radix
// sort of the row ids restores the ascending table order per pick.
//
// A division by zero follows IEEE here (numba raises; the Python layer does): a rectangle side with equal corner
// heights is only divided by for a row at exactly that height, which the strict box excludes (such a side lies on the
// box).  No contraction.  Every loop is bounded by the row, corner or cell count.
#include <algorithm>
#include <rocprim/device/device_segmented_radix_sort.hpp>

#include "rows_blocks.h"

#pragma clang fp contract(off)

namespace pmi {
namespace picks {

using namespace rows;

constexpr int WAVES = BLOCK / 64;

struct Grid {
    double x0, y0, x1, y1, cell;
    int64_t CX, CY;
};

// the cell of a coordinate inside [lo, hi]: monotone in v, so a row between two bounds lies between their cells
__device__ __forceinline__ int64_t cell_of(double v, double lo, double cell, int64_t cells)
{
    const double q = (v - lo) / cell;
    if (!(q > 0.0)) return 0;
    return q >= (double)cells ? cells - 1 : (int64_t)q;
}

// position of a member among the members of the workgroup's 256 lanes, and their number; every lane calls it
__device__ __forceinline__ uint32_t block_prefix(bool in, uint32_t *wave_count, uint32_t *total)
{
    const uint64_t mask = __ballot(in);
    const unsigned lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    if (lane == 0) wave_count[wave] = (uint32_t)__popcll(mask);
    __syncthreads();
    uint32_t before = 0, all = 0;
    for (unsigned w = 0; w < WAVES; ++w) {
        const uint32_t c = wave_count[w];
        if (w < wave) before += c;
        all += c;
    }
    __syncthreads();
    *total = all;
    return before + (uint32_t)__popcll(mask & ((1ull << lane) - 1ull));
}

// one run of sorted positions [a, b): count its members, or write their rows behind the `done` earlier ones
template <typename Test>
__device__ __forceinline__ void walk_run(const int32_t *__restrict__ rows, int32_t n, int32_t a, int32_t b, Test test,
                                         uint32_t *wave_count, int64_t base, int64_t capacity, int32_t *members,
                                         int64_t *done)
{
    for (int64_t j0 = a; j0 < b; j0 += BLOCK) {
        const int64_t j = j0 + threadIdx.x;
        int32_t row = -1;
        if (j < b) row = rows[j];
        const bool in = row >= 0 && row < n && test(row);
        uint32_t total;
        const uint32_t at = block_prefix(in, wave_count, &total);
        if (members && in) {
            const int64_t w = base + *done + at;
            if (w >= 0 && w < capacity) members[w] = row;
        }
        *done += total;
    }
}

template <typename TX, typename TY>
__global__ void circle_kernel(Blocks g, const TX *__restrict__ x, const TY *__restrict__ y,
                              const int32_t *__restrict__ rows, const double *__restrict__ px,
                              const double *__restrict__ py, const int64_t *__restrict__ bx,
                              const int64_t *__restrict__ by, const uint8_t *__restrict__ flags, double r2,
                              uint32_t *__restrict__ counts, const int64_t *__restrict__ offsets, int64_t capacity,
                              int32_t *__restrict__ members)
{
    __shared__ uint32_t wave_count[WAVES];
    const int64_t pick = blockIdx.x;
    const double cx = px[pick], cy = py[pick];
    const int64_t ki = by[pick], li = bx[pick];
    const unsigned f = flags[pick];
    const float cxf = (float)cx, cyf = (float)cy, r2f = (float)r2;
    // a float32 column keeps its difference and square in float32 when its flag bit says so
    const bool x32 = sizeof(TX) == 4 && (f & 1u), y32 = sizeof(TY) == 4 && (f & 2u);
    auto test = [&](int32_t row) -> bool {
        const TX xr = x[row];
        const TY yr = y[row];
        if (x32 && y32) {
            const float dx = (float)xr - cxf, dy = (float)yr - cyf;
            const float sum = dx * dx + dy * dy;
            return (f & 4u) ? sum < r2f : (double)sum < r2;
        }
        double dx2, dy2;
        if (x32) { const float d = (float)xr - cxf; dx2 = (double)(d * d); } else { const double d = (double)xr - cx; dx2 = d * d; }
        if (y32) { const float d = (float)yr - cyf; dy2 = (double)(d * d); } else { const double d = (double)yr - cy; dy2 = d * d; }
        return dx2 + dy2 < r2;
    };
    const int64_t base = members ? offsets[pick] : 0;
    int64_t done = 0;
    const Window w = window(g, ki, li);
    for (int t = 0; t < 3; ++t) {
        if (!w.row[t]) continue;
        int32_t a, b;
        block_run(g, ki - 1 + t, w.l0, w.l1, &a, &b);
        walk_run(rows, g.n, a, b, test, wave_count, base, capacity, members, &done);
    }
    if (!members && threadIdx.x == 0) counts[pick] = (uint32_t)std::min<int64_t>(done, 0xffffffffLL);
}

template <typename TX, typename TY>
__global__ void cells_kernel(const TX *__restrict__ x, const TY *__restrict__ y, int32_t n, Grid g,
                             uint32_t *__restrict__ x_index, uint32_t *__restrict__ y_index)
{
    const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    const double xv = (double)x[i], yv = (double)y[i];
    if (xv >= g.x0 && xv <= g.x1 && yv >= g.y0 && yv <= g.y1) {
        x_index[i] = (uint32_t)cell_of(xv, g.x0, g.cell, g.CX);
        y_index[i] = (uint32_t)cell_of(yv, g.y0, g.cell, g.CY);
    } else {                                                        // NaN too: behind every cell, outside the grid
        x_index[i] = 0;
        y_index[i] = (uint32_t)g.CY;
    }
}

enum { SQUARE = 0, RECTANGLE = 1, POLYGON = 2 };

// v > bound (UPPER false) or v < bound (UPPER true): in T when the bound is a weak scalar, else in float64
template <typename T, bool UPPER>
__device__ __forceinline__ bool beyond(T v, double bound, bool weak)
{
    if (weak) {
        const T b = (T)bound;
        return UPPER ? v < b : v > b;
    }
    return UPPER ? (double)v < bound : (double)v > bound;
}

// the bound a row is really held against, as a float64
template <typename T>
__device__ __forceinline__ double effective(double bound, bool weak) { return weak ? (double)(T)bound : bound; }

template <typename TX, typename TY>
__global__ void shape_kernel(Blocks g, Grid grid, const TX *__restrict__ x, const TY *__restrict__ y,
                             const int32_t *__restrict__ rows, int shape, const double *__restrict__ bounds,
                             const uint8_t *__restrict__ flags, const int32_t *__restrict__ corner_offsets,
                             const double *__restrict__ X, const double *__restrict__ Y, int32_t n_corners,
                             uint32_t *__restrict__ counts, const int64_t *__restrict__ offsets, int64_t capacity,
                             int32_t *__restrict__ members)
{
    __shared__ uint32_t wave_count[WAVES];
    const int64_t pick = blockIdx.x;
    const double x_min = bounds[4 * pick], x_max = bounds[4 * pick + 1], y_min = bounds[4 * pick + 2],
                 y_max = bounds[4 * pick + 3];
    const unsigned f = flags[pick];
    int32_t c0 = 0, c1 = 0;
    if (shape != SQUARE) {
        c0 = std::min(std::max(corner_offsets[pick], 0), n_corners);
        c1 = std::min(std::max(corner_offsets[pick + 1], c0), n_corners);
    }
    const int32_t m = c1 - c0;
    const double *__restrict__ PX = X + c0, *__restrict__ PY = Y + c0;
    auto test = [&](int32_t row) -> bool {
        const TX xr = x[row];
        const TY yr = y[row];
        if (!(beyond<TX, false>(xr, x_min, f & 1u) && beyond<TX, true>(xr, x_max, f & 2u) &&
              beyond<TY, false>(yr, y_min, f & 4u) && beyond<TY, true>(yr, y_max, f & 8u)))
            return false;
        if (shape == SQUARE) return true;
        const double xv = (double)xr, yv = (double)yr;
        int hits = 0;
        if (shape == RECTANGLE) {
            if (m != 4) return false;
            for (int i = 0; i < 4; ++i) {
                const int i2 = i == 3 ? 0 : i + 1;
                const double y1 = PY[i], y2 = PY[i2];
                const double lo = y2 < y1 ? y2 : y1, hi = y2 > y1 ? y2 : y1;
                if (lo <= yv && yv <= hi) {
                    const double m_inv = (PX[i2] - PX[i]) / (y2 - y1);
                    const double x_intersect = m_inv * (yv - y1) + PX[i];
                    if (x_intersect >= xv) ++hits;
                }
            }
        } else {
            for (int32_t j = 0; j < m; ++j) {
                const int32_t j2 = j + 1 == m ? 0 : j + 1;
                const double y1 = PY[j], y2 = PY[j2];
                if ((y1 > yv) != (y2 > yv)) {
                    const double reach = PX[j] + (PX[j2] - PX[j]) * (yv - y1) / (y2 - y1);
                    if (xv < reach) ++hits;
                }
            }
        }
        return (hits & 1) != 0;
    };
    const int64_t base = members ? offsets[pick] : 0;
    int64_t done = 0;
    const double ex0 = effective<TX>(x_min, f & 1u), ex1 = effective<TX>(x_max, f & 2u),
                 ey0 = effective<TY>(y_min, f & 4u), ey1 = effective<TY>(y_max, f & 8u);
    // a box with a NaN bound, or an empty one, holds no row
    if (ex0 < ex1 && ey0 < ey1 && ex1 >= grid.x0 && ex0 <= grid.x1 && ey1 >= grid.y0 && ey0 <= grid.y1 && g.K > 0 && g.L > 0) {
        const int64_t l0 = cell_of(ex0, grid.x0, grid.cell, g.L), l1 = cell_of(ex1, grid.x0, grid.cell, g.L);
        const int64_t k0 = cell_of(ey0, grid.y0, grid.cell, g.K), k1 = cell_of(ey1, grid.y0, grid.cell, g.K);
        for (int64_t k = k0; k <= k1; ++k) {
            int32_t a, b;
            block_run(g, k, l0, l1, &a, &b);
            walk_run(rows, g.n, a, b, test, wave_count, base, capacity, members, &done);
        }
    }
    if (!members && threadIdx.x == 0) counts[pick] = (uint32_t)std::min<int64_t>(done, 0xffffffffLL);
}

// ---- host ------------------------------------------------------------------------------------------------------
static int check_call(const char *what, int64_t n, int64_t p, int64_t K, int64_t L, int64_t n_picks, int64_t capacity)
{
    if (n < 0 || n > INT32_MAX - 1 || p < 0 || p > n || K < 0 || L < 0 || K > INDEX_MAX || L > INDEX_MAX || n_picks < 0 ||
        n_picks > INT32_MAX - 1 || capacity < 0 || capacity > INT32_MAX - 1) {
        set_error("%s: %lld rows, %lld visible, grid %lld x %lld, %lld picks, room for %lld members (rows, picks and "
                  "members are indexed with int32)", what, (long long)n, (long long)p, (long long)K, (long long)L,
                  (long long)n_picks, (long long)capacity);
        return PMI_ERR_ARG;
    }
    return PMI_OK;
}

// The count pass of a call: launch(counts) fills counts[0 .. P), one workgroup per pick; offsets[0 .. P] is their
// exclusive scan (counts[P] is a zero the scan runs over), and the total comes to the host.
template <typename Launch>
static int count_pass(int64_t P, Launch &&launch, int64_t *offsets, int64_t *total, hipStream_t s)
{
    uint32_t *counts;
    int rc = carve(SCR_STAGE_A, [&](Arena &ar) { counts = ar.take<uint32_t>((size_t)P + 1); });
    if (rc != PMI_OK) return rc;
    PMI_HIP(hipMemsetAsync(counts, 0, sizeof(uint32_t) * ((size_t)P + 1), s));
    launch(counts);
    PMI_HIP(hipGetLastError());
    rc = two_pass([&](void *tmp, size_t &bytes) {
        return rocprim::exclusive_scan(tmp, bytes, counts, offsets, (int64_t)0, (size_t)P + 1, rocprim::plus<int64_t>(), s);
    });
    if (rc != PMI_OK) return rc;
    int64_t h_total = 0;
    PMI_HIP(hipMemcpyAsync(&h_total, offsets + P, sizeof(int64_t), hipMemcpyDeviceToHost, s));
    PMI_HIP(hipStreamSynchronize(s));
    if (h_total < 0 || h_total > INT32_MAX - 1) {
        set_error("picks: %lld member rows in one call (members are indexed with int32)", (long long)h_total);
        return PMI_ERR_ARG;
    }
    *total = h_total;
    return PMI_OK;
}

struct CircleArgs {
    const int32_t *rows;
    const double *px, *py;
    const int64_t *bx, *by;
    const uint8_t *flags;
    double r2;
    int64_t n_picks, *offsets, capacity, *total;
    int32_t *members;
};

template <typename TX, typename TY>
static int circle_typed(const TX *x, const TY *y, Blocks g, const CircleArgs &c, hipStream_t s)
{
    const unsigned P = (unsigned)c.n_picks;
    if (c.members) {
        circle_kernel<TX, TY><<<P, BLOCK, 0, s>>>(g, x, y, c.rows, c.px, c.py, c.bx, c.by, c.flags, c.r2, nullptr,
                                                 c.offsets, c.capacity, c.members);
        PMI_HIP(hipGetLastError());
        PMI_HIP(hipStreamSynchronize(s));
        return PMI_OK;
    }
    return count_pass(c.n_picks, [&](uint32_t *counts) {
        circle_kernel<TX, TY><<<P, BLOCK, 0, s>>>(g, x, y, c.rows, c.px, c.py, c.bx, c.by, c.flags, c.r2, counts, nullptr,
                                                 0, nullptr);
    }, c.offsets, c.total, s);
}

struct ShapeArgs {
    const int32_t *rows;
    Grid grid;
    int shape;
    const double *bounds;
    const uint8_t *flags;
    const int32_t *corner_offsets;
    const double *X, *Y;
    int32_t n_corners;
    int64_t n_picks, *offsets, capacity, *total;
    int32_t *members;
};

template <typename TX, typename TY>
static int shape_typed(const TX *x, const TY *y, Blocks g, const ShapeArgs &c, hipStream_t s)
{
    const unsigned P = (unsigned)c.n_picks;
    if (!c.members)
        return count_pass(c.n_picks, [&](uint32_t *counts) {
            shape_kernel<TX, TY><<<P, BLOCK, 0, s>>>(g, c.grid, x, y, c.rows, c.shape, c.bounds, c.flags, c.corner_offsets,
                                                    c.X, c.Y, c.n_corners, counts, nullptr, 0, nullptr);
        }, c.offsets, c.total, s);
    if (c.capacity == 0) return PMI_OK;
    // members in cell order, then each pick's segment sorted by row id into the caller's array
    int32_t *unsorted;
    int rc = carve(SCR_STAGE_A, [&](Arena &ar) { unsorted = ar.take<int32_t>((size_t)c.capacity); });
    if (rc != PMI_OK) return rc;
    PMI_HIP(hipMemsetAsync(unsorted, 0, sizeof(int32_t) * (size_t)c.capacity, s));
    shape_kernel<TX, TY><<<P, BLOCK, 0, s>>>(g, c.grid, x, y, c.rows, c.shape, c.bounds, c.flags, c.corner_offsets, c.X,
                                            c.Y, c.n_corners, nullptr, c.offsets, c.capacity, unsorted);
    PMI_HIP(hipGetLastError());
    const int bits = bits_of((uint64_t)std::max(g.n - 1, 1));
    rc = two_pass([&](void *tmp, size_t &bytes) {
        return rocprim::segmented_radix_sort_keys(tmp, bytes, (const uint32_t *)unsorted, (uint32_t *)c.members,
                                                  (unsigned)c.capacity, P, c.offsets, c.offsets + 1, 0u, (unsigned)bits, s);
    });
    if (rc != PMI_OK) return rc;
    PMI_HIP(hipStreamSynchronize(s));
    return PMI_OK;
}

template <typename TX, typename TY>
static int cells_typed(const TX *x, const TY *y, int32_t n, Grid g, uint32_t *x_index, uint32_t *y_index, hipStream_t s)
{
    PMI_LAUNCH((cells_kernel<TX, TY>), n, s, x, y, n, g, x_index, y_index);
    PMI_HIP(hipStreamSynchronize(s));
    return PMI_OK;
}

// a call without picks: the count pass answers offsets[0] = 0 and no members, the write pass has nothing to do
static int no_picks(int64_t *offsets, int32_t *members, int64_t *total, hipStream_t s)
{
    if (members) return PMI_OK;
    *total = 0;
    PMI_HIP(hipMemsetAsync(offsets, 0, sizeof(int64_t), s));
    PMI_HIP(hipStreamSynchronize(s));
    return PMI_OK;
}

static int check_grid(const char *what, const Grid &g)
{
    if (!(g.cell > 0.0) || !(g.x0 <= g.x1) || !(g.y0 <= g.y1) || !std::isfinite(g.cell) || !std::isfinite(g.x0) ||
        !std::isfinite(g.x1) || !std::isfinite(g.y0) || !std::isfinite(g.y1) || g.CX < 1 || g.CY < 1 ||
        g.CX >= INDEX_MAX || g.CY >= INDEX_MAX) {
        set_error("%s: grid [%g, %g] x [%g, %g], cells of %g, %lld x %lld of them", what, g.x0, g.x1, g.y0, g.y1, g.cell,
                  (long long)g.CX, (long long)g.CY);
        return PMI_ERR_ARG;
    }
    return PMI_OK;
}

}  // namespace picks
}  // namespace pmi

using namespace pmi;

extern "C" {

int pmi_picks_circle_dev(const void *d_x, int x_type, const void *d_y, int y_type, const int32_t *d_rows,
                         const uint64_t *d_keys, int64_t n, int64_t p, int64_t K, int64_t L, const double *d_pick_x,
                         const double *d_pick_y, const int64_t *d_block_x, const int64_t *d_block_y,
                         const uint8_t *d_flags, int64_t n_picks, double r2, int64_t *d_offsets, int32_t *d_members,
                         int64_t capacity, int64_t *total, void *stream)
{
    const char *what = "pmi_picks_circle_dev";
    int rc = picks::check_call(what, n, p, K, L, n_picks, capacity);
    if (rc || (rc = rows::check_xy(what, x_type, y_type))) return rc;
    if (!d_offsets || (!d_members && !total) || (n_picks > 0 && (!d_pick_x || !d_pick_y || !d_block_x || !d_block_y || !d_flags)) ||
        (n > 0 && (!d_x || !d_y || !d_rows || !d_keys))) {
        set_error("%s: NULL argument", what);
        return PMI_ERR_ARG;
    }
    hipStream_t s = (hipStream_t)stream;
    if (n_picks == 0) return picks::no_picks(d_offsets, d_members, total, s);
    const rows::Blocks g{d_keys, (int32_t)n, (int32_t)p, K, L};
    const picks::CircleArgs c{d_rows, d_pick_x, d_pick_y, d_block_x, d_block_y, d_flags, r2, n_picks, d_offsets,
                              capacity, total, d_members};
    return PMI_XY_DISPATCH(picks::circle_typed, g, c, s);
}

int pmi_picks_cells_dev(const void *d_x, int x_type, const void *d_y, int y_type, int64_t n, double x0, double y0,
                        double x1, double y1, double cell, int64_t CX, int64_t CY, uint32_t *d_x_index,
                        uint32_t *d_y_index, void *stream)
{
    const char *what = "pmi_picks_cells_dev";
    const picks::Grid grid{x0, y0, x1, y1, cell, CX, CY};
    int rc = rows::check_rows(what, n);
    if (rc || (rc = rows::check_xy(what, x_type, y_type)) || (rc = picks::check_grid(what, grid))) return rc;
    if (n > 0 && (!d_x || !d_y || !d_x_index || !d_y_index)) {
        set_error("%s: NULL column", what);
        return PMI_ERR_ARG;
    }
    if (n == 0) return PMI_OK;
    return PMI_XY_DISPATCH(picks::cells_typed, (int32_t)n, grid, d_x_index, d_y_index, (hipStream_t)stream);
}

int pmi_picks_shape_dev(const void *d_x, int x_type, const void *d_y, int y_type, const int32_t *d_rows,
                        const uint64_t *d_keys, int64_t n, int64_t p, double x0, double y0, double x1, double y1,
                        double cell, int64_t CX, int64_t CY, int shape, const double *d_bounds, const uint8_t *d_flags,
                        const int32_t *d_corner_offsets, const double *d_corner_x, const double *d_corner_y,
                        int64_t n_corners, int64_t n_picks, int64_t *d_offsets, int32_t *d_members, int64_t capacity,
                        int64_t *total, void *stream)
{
    const char *what = "pmi_picks_shape_dev";
    const picks::Grid grid{x0, y0, x1, y1, cell, CX, CY};
    int rc = picks::check_call(what, n, p, CY, CX, n_picks, capacity);
    if (rc || (rc = rows::check_xy(what, x_type, y_type)) || (rc = picks::check_grid(what, grid))) return rc;
    const bool corners = shape == picks::RECTANGLE || shape == picks::POLYGON;
    if ((shape != picks::SQUARE && !corners) || n_corners < 0 || n_corners > INT32_MAX - 1 || !d_offsets ||
        (!d_members && !total) || (n_picks > 0 && (!d_bounds || !d_flags)) ||
        (n_picks > 0 && corners && (!d_corner_offsets || (n_corners > 0 && (!d_corner_x || !d_corner_y)))) ||
        (n > 0 && (!d_x || !d_y || !d_rows || !d_keys))) {
        set_error("%s: shape %d, %lld corners, or a NULL argument", what, shape, (long long)n_corners);
        return PMI_ERR_ARG;
    }
    hipStream_t s = (hipStream_t)stream;
    if (n_picks == 0) return picks::no_picks(d_offsets, d_members, total, s);
    const rows::Blocks g{d_keys, (int32_t)n, (int32_t)p, CY, CX};
    const picks::ShapeArgs c{d_rows, grid, shape, d_bounds, d_flags, d_corner_offsets, d_corner_x, d_corner_y,
                             (int32_t)n_corners, n_picks, d_offsets, capacity, total, d_members};
    return PMI_XY_DISPATCH(picks::shape_typed, g, c, s);
}

}  // extern "C"
