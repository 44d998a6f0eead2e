// similar.hip — the grid search of pick_similar (picasso/postprocess.py:597-736 _pick_similar, :820-845 _n_block_locs_at,
// :848-957 get_block_locs_at_numba, locs_at_numba, rmsd_at_com): every point of the hexagonal grid mean-shifted to the
// centre of mass of its circle, in the bits numba gives the reference, and the greedy pass over the candidates on the host.
//
// One lane per grid point, the points in the reference's loop order (column outside, y inside), so consecutive lanes
// take consecutive y values of one column: a wave shares its block column and reads neighbouring block rows.  The sum
// of a circle's members is one ordered chain per point (numba's np.mean is `c = 0; for v in a: c += v`), which cannot be
// split among lanes and keep its bits; the chip is filled by the number of points.
//
// Before the search the two columns are gathered once into block order in their common type S (float32 only when both
// are: the reference stacks x and y into one array), positions < p only (the reference's table stops filling at the
// first row outside the K x L grid).  A point in block (ki, li) then owns three runs of positions, one per block row
// k = ki - 1 .. ki + 1 with 0 <= k < K, blocks l = li - 1 .. li + 1 with 0 <= l < L (two bisections of the sorted keys
// per run: the clamped window of rows_blocks.h, shared with picks.hip); they are found once and never again as the
// centre moves.  The gate, which is this source's own, counts the rows of the
// narrower runs 0 < k < K, 0 < l < L (block row 0 and block column 0 never count; when no block qualifies the
// reference's variable is never assigned and numba leaves it 0) and the point goes on when that count is >= gate.
//
// Per point, with the centre c a float64 throughout: the members are the rows with (S - c.x) ** 2 + (S - c.y) ** 2 < r2
// in float64; with at most one member the point is skipped (n = 0).  The centre moves to their mean, float64(sum in S in
// run order from S(0)) / n, and while |dx| > 1e-3 or |dy| > 1e-3, at most max_shifts times, the members are taken again
// around the new centre; a set of at most one member ends the loop.  What comes out is the last set's count, that set's
// mean as (cx, cy) (the mean before it when it has at most one member), and sqrt(sum of ((S - cx) ** 2 + (S - cy) ** 2)
// in order / n) of it (0 for a set of at most one member, which no range accepts).  Divisions and the square root are
// the correctly rounded float64 ones of the compiler; nothing is contracted.  Every loop is bounded by a row count or by
// max_shifts.
//
// pmi_similar_filter is plain host C++: the candidates in grid order, kept when no given pick and no earlier kept
// candidate has (qx - cx) ** 2 + (qy - cy) ** 2 > d2 false.  A uniform grid of cells a little wider than `cell` (= d)
// holds the picks; a candidate looks at the 3 x 3 cells around its own.  Kept candidates lie more than d apart, the
// given picks may lie anywhere: a cell's list is walked whole.
#include <algorithm>
#include <cmath>
#include <unordered_map>
#include <vector>

#include "rows_blocks.h"

#pragma clang fp contract(off)

namespace pmi {
namespace similar {

using namespace rows;

constexpr int64_t MAX_SHIFTS = 1 << 16;

struct Grid {
    const double *x, *y_base, *y_shift;
    const int64_t *bx, *by_base, *by_shift;
    int64_t n_x, n_y;
};

template <typename TX, typename TY, typename S>
__global__ void gather_kernel(const TX *__restrict__ x, const TY *__restrict__ y, const int32_t *__restrict__ rows,
                              int32_t n, int32_t p, S *__restrict__ xs, S *__restrict__ ys)
{
    const int64_t j = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (j >= p) return;
    const int32_t row = rows[j];
    const bool ok = row >= 0 && row < n;                           // a row that is none is a member of no circle
    xs[j] = ok ? (S)x[row] : (S)__builtin_nan("");
    ys[j] = ok ? (S)y[row] : (S)__builtin_nan("");
}

// the members of the circle around (cx, cy) among three runs: their number, and their sums in S in run order
template <typename S>
__device__ __forceinline__ int32_t select(const S *__restrict__ xs, const S *__restrict__ ys, const int32_t (&a)[3],
                                          const int32_t (&b)[3], double cx, double cy, double r2, S *sum_x, S *sum_y)
{
    S sx = (S)0, sy = (S)0;
    int32_t m = 0;
#pragma unroll
    for (int t = 0; t < 3; ++t) {
        for (int32_t j = a[t]; j < b[t]; ++j) {
            const S xv = xs[j], yv = ys[j];
            const double dx = (double)xv - cx, dy = (double)yv - cy;
            if (dx * dx + dy * dy < r2) {
                sx += xv;
                sy += yv;
                ++m;
            }
        }
    }
    *sum_x = sx;
    *sum_y = sy;
    return m;
}

// the sum over the same members of their squared distance from (mx, my), in run order
template <typename S>
__device__ __forceinline__ double spread(const S *__restrict__ xs, const S *__restrict__ ys, const int32_t (&a)[3],
                                         const int32_t (&b)[3], double cx, double cy, double r2, double mx, double my)
{
    double acc = 0.0;
#pragma unroll
    for (int t = 0; t < 3; ++t) {
        for (int32_t j = a[t]; j < b[t]; ++j) {
            const double xv = (double)xs[j], yv = (double)ys[j];
            const double dx = xv - cx, dy = yv - cy;
            if (dx * dx + dy * dy < r2) {
                const double ex = xv - mx, ey = yv - my;
                acc += ex * ex + ey * ey;
            }
        }
    }
    return acc;
}

template <typename S>
__global__ void shift_kernel(Blocks g, Grid grid, const S *__restrict__ xs, const S *__restrict__ ys, double r2,
                             double gate, int32_t max_shifts, double *__restrict__ out_x, double *__restrict__ out_y,
                             int32_t *__restrict__ out_n, double *__restrict__ out_rmsd)
{
    const int64_t point = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (point >= grid.n_x * grid.n_y) return;
    const int64_t i = point / grid.n_y, j = point - i * grid.n_y;
    const bool odd = (i & 1) != 0;                                  // odd columns take the shifted y values
    const double gx = grid.x[i], gy = odd ? grid.y_shift[j] : grid.y_base[j];
    const int64_t li = grid.bx[i], ki = odd ? grid.by_shift[j] : grid.by_base[j];

    int32_t a[3] = {0, 0, 0}, b[3] = {0, 0, 0};
    int64_t gated = 0;
    const Window w = window(g, ki, li);
#pragma unroll
    for (int t = 0; t < 3; ++t) {
        if (!w.row[t]) continue;
        const int64_t k = ki - 1 + t;
        block_run(g, k, w.l0, w.l1, &a[t], &b[t]);
        if (k >= 1 && w.l1 >= 1)                                    // the gate's blocks: 0 < k, 0 < l
            gated += b[t] - (w.l0 >= 1 ? a[t] : lower_bound(g.keys, a[t], b[t], block_key(k, 1)));
    }

    double cx = gx, cy = gy, rmsd = 0.0;
    int32_t m = 0;
    if ((double)gated >= gate) {
        S sx, sy;
        m = select(xs, ys, a, b, gx, gy, r2, &sx, &sy);
        if (m > 1) {
            double ox = gx, oy = gy;                                // the centre the current set was taken around
            cx = (double)sx / (double)m;
            cy = (double)sy / (double)m;
            for (int32_t count = 1; count <= max_shifts; ++count) {
                if (!(__builtin_fabs(cx - ox) > 1e-3 || __builtin_fabs(cy - oy) > 1e-3)) break;
                ox = cx;
                oy = cy;
                m = select(xs, ys, a, b, ox, oy, r2, &sx, &sy);
                if (m <= 1) break;
                cx = (double)sx / (double)m;
                cy = (double)sy / (double)m;
            }
            if (m > 1) rmsd = __builtin_sqrt(spread(xs, ys, a, b, ox, oy, r2, cx, cy) / (double)m);
        } else {
            m = 0;
        }
    }
    out_x[point] = cx;
    out_y[point] = cy;
    out_n[point] = m;
    out_rmsd[point] = rmsd;
}

struct ShiftArgs {
    const int32_t *rows;
    double r2, gate;
    int32_t max_shifts;
    double *out_x, *out_y;
    int32_t *out_n;
    double *out_rmsd;
};

template <typename TX, typename TY, typename S>
static int shift_in(const TX *x, const TY *y, Blocks g, const Grid &grid, const ShiftArgs &c, hipStream_t s)
{
    S *xs, *ys;
    const size_t room = (size_t)std::max<int32_t>(g.p, 1);
    int rc = carve(SCR_STAGE_A, [&](Arena &ar) { xs = ar.take<S>(room); ys = ar.take<S>(room); });
    if (rc != PMI_OK) return rc;
    if (g.p > 0) PMI_LAUNCH((gather_kernel<TX, TY, S>), g.p, s, x, y, c.rows, g.n, g.p, xs, ys);
    PMI_LAUNCH((shift_kernel<S>), grid.n_x * grid.n_y, s, g, grid, xs, ys, c.r2, c.gate, c.max_shifts, c.out_x, c.out_y,
               c.out_n, c.out_rmsd);
    PMI_HIP(hipStreamSynchronize(s));
    return PMI_OK;
}

template <typename TX, typename TY>
static int shift_typed(const TX *x, const TY *y, Blocks g, const Grid &grid, const ShiftArgs &c, hipStream_t s)
{
    if (sizeof(TX) == 4 && sizeof(TY) == 4) return shift_in<TX, TY, float>(x, y, g, grid, c, s);
    return shift_in<TX, TY, double>(x, y, g, grid, c, s);
}

// ---- the greedy pass (host) ---------------------------------------------------------------------------------------
struct Cells {
    double lo_x, lo_y, cell;
    std::unordered_map<uint64_t, std::vector<int64_t>> held;

    // monotone in v, so two coordinates at most `cell` apart lie in one cell or in neighbouring ones
    int64_t index(double v, double lo) const
    {
        if (!(cell > 0.0) || !std::isfinite(cell)) return 0;
        const double q = (v - lo) / cell;
        if (!(q > 0.0)) return 0;
        return q >= 2147483647.0 ? 2147483647LL : (int64_t)q;
    }
    static uint64_t key(int64_t iy, int64_t ix) { return ((uint64_t)iy << 32) | (uint64_t)ix; }
};

}  // namespace similar
}  // namespace pmi

using namespace pmi;

extern "C" {

int pmi_similar_shift_dev(const void *d_x, int x_type, const void *d_y, int y_type, const int32_t *d_rows,
                          const uint64_t *d_keys, int64_t n, int64_t p, int64_t K, int64_t L, const double *d_grid_x,
                          const int64_t *d_block_x, int64_t n_x, const double *d_grid_y_base,
                          const double *d_grid_y_shift, const int64_t *d_block_y_base, const int64_t *d_block_y_shift,
                          int64_t n_y, double r2, double gate, int64_t max_shifts, double *d_out_x, double *d_out_y,
                          int32_t *d_out_n, double *d_out_rmsd, void *stream)
{
    const char *what = "pmi_similar_shift_dev";
    int rc = rows::check_rows(what, n);
    if (rc || (rc = rows::check_xy(what, x_type, y_type))) return rc;
    if (p < 0 || p > n || K < 0 || L < 0 || K > rows::INDEX_MAX || L > rows::INDEX_MAX || n_x < 0 || n_y < 0 ||
        n_x > INT32_MAX - 1 || n_y > INT32_MAX - 1 || n_x * n_y > INT32_MAX - 1 || max_shifts < 0 ||
        max_shifts > similar::MAX_SHIFTS) {
        set_error("%s: %lld visible of %lld rows, grid %lld x %lld, %lld x %lld points (indexed with int32), %lld shifts "
                  "(at most %lld)", what, (long long)p, (long long)n, (long long)K, (long long)L, (long long)n_x,
                  (long long)n_y, (long long)max_shifts, (long long)similar::MAX_SHIFTS);
        return PMI_ERR_ARG;
    }
    if (n_x == 0 || n_y == 0) return PMI_OK;
    if (!d_grid_x || !d_block_x || !d_grid_y_base || !d_grid_y_shift || !d_block_y_base || !d_block_y_shift || !d_out_x ||
        !d_out_y || !d_out_n || !d_out_rmsd || (n > 0 && (!d_x || !d_y || !d_rows || !d_keys))) {
        set_error("%s: NULL argument", what);
        return PMI_ERR_ARG;
    }
    const rows::Blocks g{d_keys, (int32_t)n, (int32_t)p, K, L};
    const similar::Grid grid{d_grid_x, d_grid_y_base, d_grid_y_shift, d_block_x, d_block_y_base, d_block_y_shift, n_x, n_y};
    const similar::ShiftArgs c{d_rows, r2, gate, (int32_t)max_shifts, d_out_x, d_out_y, d_out_n, d_out_rmsd};
    return PMI_XY_DISPATCH(similar::shift_typed, g, grid, c, (hipStream_t)stream);
}

int pmi_similar_filter(const double *cand_x, const double *cand_y, int64_t n_candidates, const double *pick_x,
                       const double *pick_y, int64_t n_picks, double d2, double cell, uint8_t *keep)
{
    const char *what = "pmi_similar_filter";
    if (n_candidates < 0 || n_picks < 0 || (n_candidates > 0 && (!cand_x || !cand_y || !keep)) ||
        (n_picks > 0 && (!pick_x || !pick_y))) {
        set_error("%s: %lld candidates, %lld picks, or a NULL argument", what, (long long)n_candidates, (long long)n_picks);
        return PMI_ERR_ARG;
    }
    double lo_x = INFINITY, lo_y = INFINITY;
    bool finite = true;
    for (int64_t i = 0; i < n_picks; ++i) {
        finite = finite && std::isfinite(pick_x[i]) && std::isfinite(pick_y[i]);
        lo_x = std::min(lo_x, pick_x[i]);
        lo_y = std::min(lo_y, pick_y[i]);
    }
    for (int64_t i = 0; i < n_candidates; ++i) {
        finite = finite && std::isfinite(cand_x[i]) && std::isfinite(cand_y[i]);
        lo_x = std::min(lo_x, cand_x[i]);
        lo_y = std::min(lo_y, cand_y[i]);
    }
    if (!finite) {
        set_error("%s: a pick or a candidate is not finite", what);
        return PMI_ERR_ARG;
    }
    // a little wider than d: what the rounding of (v - lo) / cell can move stays inside the neighbouring cell
    similar::Cells cells{lo_x, lo_y, cell * (1.0 + 0x1p-10), {}};
    std::vector<double> qx(pick_x, pick_x + n_picks), qy(pick_y, pick_y + n_picks);
    qx.reserve((size_t)(n_picks + n_candidates));
    qy.reserve((size_t)(n_picks + n_candidates));
    for (int64_t i = 0; i < n_picks; ++i)
        cells.held[similar::Cells::key(cells.index(qy[i], lo_y), cells.index(qx[i], lo_x))].push_back(i);
    for (int64_t i = 0; i < n_candidates; ++i) {
        const double cx = cand_x[i], cy = cand_y[i];
        const int64_t iy = cells.index(cy, lo_y), ix = cells.index(cx, lo_x);
        bool apart = true;
        for (int64_t ky = std::max<int64_t>(iy - 1, 0); apart && ky <= iy + 1; ++ky) {
            for (int64_t kx = std::max<int64_t>(ix - 1, 0); apart && kx <= ix + 1; ++kx) {
                const auto at = cells.held.find(similar::Cells::key(ky, kx));
                if (at == cells.held.end()) continue;
                for (const int64_t q : at->second) {
                    const double dx = qx[q] - cx, dy = qy[q] - cy;
                    if (!(dx * dx + dy * dy > d2)) {
                        apart = false;
                        break;
                    }
                }
            }
        }
        keep[i] = apart ? 1 : 0;
        if (apart) {
            cells.held[similar::Cells::key(iy, ix)].push_back((int64_t)qx.size());
            qx.push_back(cx);
            qy.push_back(cy);
        }
    }
    return PMI_OK;
}

}  // extern "C"
