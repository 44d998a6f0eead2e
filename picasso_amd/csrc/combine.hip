// combine.hip — one row per (group, cluster) of a clustered table (picasso/postprocess.py:2174-2288 cluster_combine) and,
// on that table, the distance from every row to the nearest other row of its group (:2291-2419 cluster_combine_dist),
// in the reference's values.
//
// Order (pmi_combine_order_dev).  Rows are ordered by (group key, cluster key) with two stable radix sorts, first by
// cluster - c_min, then by group - g_min (uint64 keys on the bits the largest needs, so negative labels come first): a
// segment is a run of one (group, cluster) pair and keeps its rows in table order, segments ascend by cluster within a
// group and groups ascend, which is np.unique of each as the reference loops over them.  Flags of the pair changes and
// one exclusive scan give start[s], the first sorted position of segment s, closed by n; flags of the group changes and
// a second scan give group_start[g], the first SEGMENT of group g, closed by the number of segments.
//
// Statistics (pmi_combine_stats_dev).  One lane per segment walks its run of the gathered, segment-ordered column:
// pandas' Series.mean() / Series.std() and np.average(x, weights=w), all of them NumPy add.reduce chains
// (segment_stats.h, shared with kinetics.hip) that cannot be split across lanes and keep their bits.  The weighted
// average gathers x and w in one floating type (the host promotes as np.average does) and returns the sum of the weights
// beside it: the host raises np.average's ZeroDivisionError where one is exactly zero.
//
// Nearest other row (pmi_combine_mindist_dev).  The points, float64, are gathered into the order above (every segment
// is one row there: the host has refused a repeated pair).  A workgroup takes a tile of BLOCK rows of one group as
// queries, one per lane, streams the group's rows through LDS in tiles of BLOCK and keeps the running minimum of
// ((dx * dx) + (dy * dy)) (+ (dz * dz)) per lane: knn_search.h's sum, which is scipy's cdist before the root.  The
// lane's own row is skipped by its position, never by its distance: two rows at one place are 0 apart.  A NaN stays
// (np.amin).  The root is taken once, of the minimum: sqrt is monotone and correctly rounded.  Workgroups are assigned
// over (group, tile) from the exclusive scan of the groups' tile counts, one bisection per workgroup, so one group of
// many rows and many groups of two rows both spread over the device.  The cost is quadratic in a group's rows, as the
// reference's is.  With 3 columns the lane also keeps the minimum over x and y alone.
//
// Every loop is bounded by the row count; no float atomics; an inconsistent table gives an empty run.
#include "knn_search.h"
#include "rows_groups.h"
#include "segment_stats.h"

#pragma clang fp contract(off)

namespace pmi {
namespace combine {

using namespace rows;

constexpr int MAX_COLS = 32;

// ---- order -----------------------------------------------------------------------------------------------------
// seg_flag[p]: a new (group, cluster) pair starts at sorted position p; grp_flag[p]: a new group does
__global__ void flag_kernel(const uint64_t *__restrict__ group_keys, const int64_t *__restrict__ cluster,
                            const int32_t *__restrict__ rows, int32_t n, uint32_t *__restrict__ seg_flag,
                            uint32_t *__restrict__ grp_flag)
{
    const int64_t p = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (p >= n) return;
    bool grp = p == 0, seg = p == 0;
    if (p > 0) {
        const int32_t i = rows[p], j = rows[p - 1];
        const int64_t ci = row_ok(i, n) ? cluster[i] : 0, cj = row_ok(j, n) ? cluster[j] : 0;
        grp = group_keys[p] != group_keys[p - 1];
        seg = grp || ci != cj;
    }
    seg_flag[p] = seg ? 1u : 0u;
    grp_flag[p] = grp ? 1u : 0u;
}

// seg_pos / grp_pos = exclusive scans of the flags
__global__ void start_kernel(const uint64_t *__restrict__ group_keys, const int64_t *__restrict__ cluster,
                             const int32_t *__restrict__ rows, const uint32_t *__restrict__ seg_flag,
                             const uint32_t *__restrict__ seg_pos, const uint32_t *__restrict__ grp_flag,
                             const uint32_t *__restrict__ grp_pos, int32_t n, uint64_t g_min, int32_t *__restrict__ start,
                             int64_t *__restrict__ seg_group, int64_t *__restrict__ seg_cluster,
                             int32_t *__restrict__ group_start, uint32_t *__restrict__ totals)
{
    const int64_t p = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (p >= n) return;
    const uint32_t s = seg_pos[p];
    const uint32_t S = close_runs(p, n, seg_flag[p], s, (int32_t)p, n, start);
    // a group starts at a segment and the groups are closed by the number of segments
    const uint32_t G = close_runs(p, n, grp_flag[p], grp_pos[p], (int32_t)s, (int32_t)(S <= (uint32_t)n ? S : 0), group_start);
    if (seg_flag[p] && s < (uint32_t)n) {
        const int32_t i = rows[p];
        seg_group[s] = (int64_t)(group_keys[p] + g_min);
        seg_cluster[s] = row_ok(i, n) ? cluster[i] : 0;
    }
    if (p == n - 1) {
        totals[0] = S;
        totals[1] = G;
    }
}

static int order(const int64_t *group, const int64_t *cluster, int32_t n, int64_t g_min, int64_t g_max, int64_t c_min,
                 int64_t c_max, int32_t *rows_out, int32_t *start, int64_t *seg_group, int64_t *seg_cluster,
                 int32_t *group_start, int64_t *n_segments, int64_t *n_groups, hipStream_t s)
{
    const size_t N = (size_t)n;
    uint64_t *keys, *keys_sorted;
    int32_t *rows, *rows_mid;
    uint32_t *seg_flag, *seg_pos, *grp_flag, *grp_pos, *totals;
    int rc = carve(SCR_STAGE_A, [&](Arena &ar) {
        keys = ar.take<uint64_t>(N), keys_sorted = ar.take<uint64_t>(N);
        rows = ar.take<int32_t>(N), rows_mid = ar.take<int32_t>(N);
        seg_flag = ar.take<uint32_t>(N), seg_pos = ar.take<uint32_t>(N);
        grp_flag = ar.take<uint32_t>(N), grp_pos = ar.take<uint32_t>(N), totals = ar.take<uint32_t>(2);
    });
    if (rc != PMI_OK) return rc;
    // tables that the kernels below do not fill (they fill all of them on a consistent input) hold empty runs
    PMI_HIP(hipMemsetAsync(start, 0, (N + 1) * sizeof(int32_t), s));
    PMI_HIP(hipMemsetAsync(group_start, 0, (N + 1) * sizeof(int32_t), s));
    if ((rc = sort_by_column(cluster, c_min, c_max, true, keys, keys_sorted, rows, rows_mid, n, s)) != PMI_OK) return rc;
    if ((rc = sort_by_column(group, g_min, g_max, false, keys, keys_sorted, rows_mid, rows_out, n, s)) != PMI_OK) return rc;
    PMI_LAUNCH(flag_kernel, n, s, keys_sorted, cluster, rows_out, n, seg_flag, grp_flag);
    if ((rc = exclusive_scan_u32(seg_flag, seg_pos, N, s)) != PMI_OK) return rc;
    if ((rc = exclusive_scan_u32(grp_flag, grp_pos, N, s)) != PMI_OK) return rc;
    PMI_LAUNCH(start_kernel, n, s, keys_sorted, cluster, rows_out, seg_flag, seg_pos, grp_flag, grp_pos, n, (uint64_t)g_min,
               start, seg_group, seg_cluster, group_start, totals);
    uint32_t h_totals[2] = {0, 0};
    PMI_HIP(hipMemcpyAsync(h_totals, totals, sizeof(h_totals), hipMemcpyDeviceToHost, s));
    PMI_HIP(hipStreamSynchronize(s));
    if (h_totals[0] < 1 || h_totals[0] > (uint32_t)n || h_totals[1] < 1 || h_totals[1] > h_totals[0]) {
        set_error("pmi_combine_order_dev: %u segments in %u groups in %d rows", h_totals[0], h_totals[1], n);
        return PMI_ERR_HIP;
    }
    *n_segments = h_totals[0];
    *n_groups = h_totals[1];
    return PMI_OK;
}

// ---- statistics ------------------------------------------------------------------------------------------------
template <typename A>
__global__ void moments_kernel(const A *__restrict__ vs, const int32_t *__restrict__ start, int32_t n, int32_t n_segments,
                               double *__restrict__ mean, double *__restrict__ sd)
{
    const int64_t g = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (g >= n_segments) return;
    int32_t a, b;
    run_of(start, (int32_t)g, n, &a, &b);
    if (mean) mean[g] = segstats::series_mean<A>(vs, a, b);
    if (sd) sd[g] = segstats::series_std<A>(vs, a, b);
}

template <typename T>
__global__ void average_kernel(const T *__restrict__ xs, const T *__restrict__ ws, const int32_t *__restrict__ start,
                               int32_t n, int32_t n_segments, double *__restrict__ average, double *__restrict__ weight_sum)
{
    const int64_t g = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (g >= n_segments) return;
    int32_t a, b;
    run_of(start, (int32_t)g, n, &a, &b);
    double scl = 0.0;
    const double avg = segstats::weighted_average<T>(xs, ws, a, b, &scl);
    if (average) average[g] = avg;
    if (weight_sum) weight_sum[g] = scl;
}

template <typename T>
static int moments_typed(const pmi_combine_column &c, const int32_t *rows, const int32_t *start, int32_t n, int32_t S,
                         void *buf, hipStream_t s)
{
    using A = typename Column<T>::sum_type;
    PMI_LAUNCH((gather_kernel<T, A>), n, s, (const T *)c.data, rows, n, (A *)buf);
    PMI_LAUNCH(moments_kernel<A>, S, s, (const A *)buf, start, n, S, c.mean, c.std);
    return PMI_OK;
}

template <typename T>
static int average_typed(const pmi_combine_column &c, const int32_t *rows, const int32_t *start, int32_t n, int32_t S,
                         void *buf, void *wbuf, hipStream_t s)
{
    PMI_LAUNCH((gather_kernel<T, T>), n, s, (const T *)c.data, rows, n, (T *)buf);
    PMI_LAUNCH((gather_kernel<T, T>), n, s, (const T *)c.weight, rows, n, (T *)wbuf);
    PMI_LAUNCH(average_kernel<T>, S, s, (const T *)buf, (const T *)wbuf, start, n, S, c.average, c.weight_sum);
    return PMI_OK;
}

static int column(const pmi_combine_column &c, const int32_t *rows, const int32_t *start, int32_t n, int32_t S, void *buf,
                  void *wbuf, hipStream_t s)
{
    int rc = PMI_OK;
    if (c.mean || c.std)
        rc = with_column_type(c.type, [&](auto col) {
            return moments_typed<typename decltype(col)::type>(c, rows, start, n, S, buf, s);
        });
    if (rc == PMI_OK && (c.average || c.weight_sum))
        rc = c.type == PMI_CENTERS_F32 ? average_typed<float>(c, rows, start, n, S, buf, wbuf, s)
                                       : average_typed<double>(c, rows, start, n, S, buf, wbuf, s);
    return rc;
}

// ---- nearest other row of the group ----------------------------------------------------------------------------
// sorted[p * D + a] = coordinate a of the row at sorted position p
template <int D>
__global__ void gather_points_kernel(const double *__restrict__ x, const int32_t *__restrict__ rows, int32_t n,
                                     double *__restrict__ sorted)
{
    const int64_t p = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (p >= n) return;
    const int32_t i = rows[p];
    for (int a = 0; a < D; ++a) sorted[p * D + a] = row_ok(i, n) ? x[(int64_t)i * D + a] : 0.0;
}

// [a, b) of group g in sorted positions: group_start names segments, start their first positions
__device__ __forceinline__ void group_run(const int32_t *__restrict__ start, const int32_t *__restrict__ group_start,
                                          int32_t g, int32_t n, int32_t n_segments, int32_t *a, int32_t *b)
{
    const int32_t s0 = group_start[g], s1 = group_start[g + 1];
    *a = *b = 0;
    if (s0 < 0 || s1 > n_segments || s0 > s1) return;
    *a = start[s0];
    *b = start[s1];
    if (*a < 0 || *b > n || *a > *b) *a = *b = 0;
}

__global__ void tiles_kernel(const int32_t *__restrict__ start, const int32_t *__restrict__ group_start, int32_t n,
                             int32_t n_segments, int32_t n_groups, uint32_t *__restrict__ tiles)
{
    const int64_t g = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (g > n_groups) return;
    uint32_t t = 0;                                   // entry n_groups is 0: its scan is the total
    if (g < n_groups) {
        int32_t a, b;
        group_run(start, group_start, (int32_t)g, n, n_segments, &a, &b);
        t = (uint32_t)((b - a + BLOCK - 1) / BLOCK);
    }
    tiles[g] = t;
}

// tile_off: exclusive scan of tiles, n_groups + 1 entries; one workgroup per tile
template <int D>
__global__ void __launch_bounds__(BLOCK)
mindist_kernel(const double *__restrict__ pts, const int32_t *__restrict__ start, const int32_t *__restrict__ group_start,
               const uint32_t *__restrict__ tile_off, int32_t n, int32_t n_segments, int32_t n_groups,
               double *__restrict__ min_dist, double *__restrict__ min_dist_xy)
{
    __shared__ double tile[BLOCK * D];
    const uint32_t w = blockIdx.x;
    // the last group whose first tile is <= w: at most 32 halvings
    int32_t lo = 0, hi = n_groups;
    for (int it = 0; it < 32 && hi - lo > 1; ++it) {
        const int32_t mid = lo + ((hi - lo) >> 1);
        if (tile_off[mid] <= w) lo = mid; else hi = mid;
    }
    const int32_t g = lo;
    int32_t a, b;
    group_run(start, group_start, g, n, n_segments, &a, &b);      // uniform over the workgroup
    const int64_t first = (int64_t)a + (int64_t)(w - tile_off[g]) * BLOCK;
    if (w < tile_off[g] || first >= b) return;                    // an inconsistent table; uniform as well
    const int32_t q = (int32_t)first + (int32_t)threadIdx.x;
    const bool active = q < b;
    double mine[D];
    for (int c = 0; c < D; ++c) mine[c] = active ? pts[(int64_t)q * D + c] : 0.0;
    double best = knn::infinity(), best_xy = knn::infinity();
    for (int32_t base = a; base < b; base += BLOCK) {
        const int32_t count = b - base < BLOCK ? b - base : BLOCK;
        __syncthreads();
        if ((int32_t)threadIdx.x < count)
            for (int c = 0; c < D; ++c) tile[threadIdx.x * D + c] = pts[(int64_t)(base + (int32_t)threadIdx.x) * D + c];
        __syncthreads();
        if (active) {
            for (int32_t j = 0; j < count; ++j) {
                if (base + j == q) continue;
                best = segstats::nearest_update(best, knn::sum_of_squares<D>(mine, tile + j * D));
                if (D == 3) best_xy = segstats::nearest_update(best_xy, knn::sum_of_squares<2>(mine, tile + j * D));
            }
        }
    }
    if (active) {
        min_dist[q] = __builtin_sqrt(best);
        if (D == 3 && min_dist_xy) min_dist_xy[q] = __builtin_sqrt(best_xy);
    }
}

template <int D>
static int mindist(const double *x, const int32_t *rows, const int32_t *start, const int32_t *group_start, int32_t n,
                   int32_t S, int32_t G, double *min_dist, double *min_dist_xy, hipStream_t s)
{
    double *sorted;
    uint32_t *tiles, *tile_off;
    int rc = carve(SCR_STAGE_A, [&](Arena &ar) {
        sorted = ar.take<double>((size_t)n * D);
        tiles = ar.take<uint32_t>((size_t)G + 1), tile_off = ar.take<uint32_t>((size_t)G + 1);
    });
    if (rc != PMI_OK) return rc;
    PMI_LAUNCH(gather_points_kernel<D>, n, s, x, rows, n, sorted);
    PMI_LAUNCH(tiles_kernel, (int64_t)G + 1, s, start, group_start, n, S, G, tiles);
    if ((rc = exclusive_scan_u32(tiles, tile_off, (size_t)G + 1, s)) != PMI_OK) return rc;
    uint32_t total = 0;
    PMI_HIP(hipMemcpyAsync(&total, tile_off + G, 4, hipMemcpyDeviceToHost, s));
    PMI_HIP(hipStreamSynchronize(s));
    // every group has at least one row and at most n: between G and n / BLOCK + G tiles
    if (total < 1 || (int64_t)total > (int64_t)n / BLOCK + G) {
        set_error("pmi_combine_mindist_dev: %u tiles for %d rows in %d groups", total, n, G);
        return PMI_ERR_HIP;
    }
    mindist_kernel<D><<<total, BLOCK, 0, s>>>(sorted, start, group_start, tile_off, n, S, G, min_dist, min_dist_xy);
    PMI_HIP(hipGetLastError());
    PMI_HIP(hipStreamSynchronize(s));
    return PMI_OK;
}

// rows in segments in groups: one level more than rows::check_rows, and its own message
static int check_table(const char *what, int64_t n, int64_t n_segments, int64_t n_groups)
{
    if (n < 0 || n > INT32_MAX - 1 || n_segments < 0 || n_segments > n || n_groups < 0 || n_groups > n_segments) {
        set_error("%s: %lld rows, %lld segments, %lld groups (rows are indexed with int32)", what, (long long)n,
                  (long long)n_segments, (long long)n_groups);
        return PMI_ERR_ARG;
    }
    return PMI_OK;
}

static bool floating(int type) { return type == PMI_CENTERS_F32 || type == PMI_CENTERS_F64; }

}  // namespace combine
}  // namespace pmi

using namespace pmi;

extern "C" {

int pmi_combine_order_dev(const int64_t *d_group, const int64_t *d_cluster, int64_t n, int64_t g_min, int64_t g_max,
                          int64_t c_min, int64_t c_max, int32_t *d_rows, int32_t *d_start, int64_t *d_seg_group,
                          int64_t *d_seg_cluster, int32_t *d_group_start, int64_t *n_segments, int64_t *n_groups,
                          void *stream)
{
    int rc = combine::check_table("pmi_combine_order_dev", n, 0, 0);
    if (rc) return rc;
    if (!n_segments || !n_groups || g_max < g_min || c_max < c_min ||
        (n > 0 && (!d_group || !d_cluster || !d_rows || !d_start || !d_seg_group || !d_seg_cluster || !d_group_start))) {
        set_error("pmi_combine_order_dev: groups %lld .. %lld, clusters %lld .. %lld, or a NULL column", (long long)g_min,
                  (long long)g_max, (long long)c_min, (long long)c_max);
        return PMI_ERR_ARG;
    }
    *n_segments = *n_groups = 0;
    if (n == 0) return PMI_OK;
    return combine::order(d_group, d_cluster, (int32_t)n, g_min, g_max, c_min, c_max, d_rows, d_start, d_seg_group,
                          d_seg_cluster, d_group_start, n_segments, n_groups, (hipStream_t)stream);
}

int pmi_combine_stats_dev(const int32_t *d_rows, const int32_t *d_start, int64_t n, int64_t n_segments,
                          const pmi_combine_column *columns, int n_columns, void *stream)
{
    int rc = combine::check_table("pmi_combine_stats_dev", n, n_segments, 0);
    if (rc) return rc;
    if (n_columns < 0 || n_columns > combine::MAX_COLS || (n_columns > 0 && !columns) ||
        (n > 0 && (!d_rows || !d_start))) {
        set_error("pmi_combine_stats_dev: %d columns (at most %d), or a NULL table", n_columns, combine::MAX_COLS);
        return PMI_ERR_ARG;
    }
    for (int i = 0; i < n_columns; ++i) {
        const pmi_combine_column &c = columns[i];
        const bool averaged = c.average || c.weight_sum;
        if (!c.data || c.type < PMI_CENTERS_F32 || c.type > PMI_CENTERS_I64 || (!c.mean && !c.std && !averaged) ||
            (averaged && (!c.weight || !combine::floating(c.type)))) {
            set_error("pmi_combine_stats_dev: column %d: type %d, nothing to compute, or an average without float weights", i,
                      c.type);
            return PMI_ERR_ARG;
        }
    }
    if (n == 0 || n_segments == 0) return PMI_OK;
    hipStream_t s = (hipStream_t)stream;
    double *buf, *wbuf;      // one gathered column and its weights, of either width
    rc = rows::carve(SCR_STAGE_A, [&](rows::Arena &ar) { buf = ar.take<double>((size_t)n), wbuf = ar.take<double>((size_t)n); });
    if (rc != PMI_OK) return rc;
    for (int i = 0; i < n_columns; ++i)
        if ((rc = combine::column(columns[i], d_rows, d_start, (int32_t)n, (int32_t)n_segments, buf, wbuf, s)) != PMI_OK) return rc;
    PMI_HIP(hipStreamSynchronize(s));
    return PMI_OK;
}

int pmi_combine_mindist_dev(const double *d_points, int dims, const int32_t *d_rows, const int32_t *d_start,
                            const int32_t *d_group_start, int64_t n, int64_t n_segments, int64_t n_groups,
                            double *d_min_dist, double *d_min_dist_xy, void *stream)
{
    int rc = combine::check_table("pmi_combine_mindist_dev", n, n_segments, n_groups);
    if (rc) return rc;
    if ((dims != 2 && dims != 3) || (n > 0 && (!d_points || !d_rows || !d_start || !d_group_start || !d_min_dist)) ||
        (n > 0 && dims == 3 && !d_min_dist_xy)) {
        set_error("pmi_combine_mindist_dev: %d columns (2 or 3), or a NULL table", dims);
        return PMI_ERR_ARG;
    }
    if (n == 0 || n_segments == 0 || n_groups == 0) return PMI_OK;
    hipStream_t s = (hipStream_t)stream;
    // a sorted position that no workgroup reaches (an inconsistent table) keeps NaN
    PMI_HIP(hipMemsetAsync(d_min_dist, 0xff, (size_t)n * sizeof(double), s));
    if (dims == 3) PMI_HIP(hipMemsetAsync(d_min_dist_xy, 0xff, (size_t)n * sizeof(double), s));
    const int32_t N = (int32_t)n, S = (int32_t)n_segments, G = (int32_t)n_groups;
    return dims == 2 ? combine::mindist<2>(d_points, d_rows, d_start, d_group_start, N, S, G, d_min_dist, d_min_dist_xy, s)
                     : combine::mindist<3>(d_points, d_rows, d_start, d_group_start, N, S, G, d_min_dist, d_min_dist_xy, s);
}

}  // extern "C"
