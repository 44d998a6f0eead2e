// centers.hip — the per-cluster statistics of picasso.clusterer.find_cluster_centers (picasso/clusterer.py:694-897:
// _aggregate_cluster_stats, _count_binding_events, _cluster_convex_hulls, _weighted_z_means), in pandas' arithmetic.
//
// Order.  A row's key is group - g_min (uint64, so negative labels come first); (key, row) is sorted with the stable
// radix sort on the bits g_max - g_min needs: the permutation is np.argsort(group, kind="stable"), the distinct keys
// ascending are what groupby(sort=True) returns, and within a label the rows keep their table order.  start[g] is the
// first sorted position of label g (flags of the key changes, one exclusive scan), start[n_groups] = n.
//
// Chains.  pandas sums a group sequentially: group_mean / group_sum are a Kahan-compensated sum in the column's own
// floating type (float32 stays float32; integers are converted to float64 first), NaN values skipped and counted out,
// the compensation reset to 0 when it becomes NaN (an infinite value); group_var is Welford's update in float64 for
// every type, ddof 1.  Neither chain can be split and keep its bits, so one lane walks one label's run of the gathered,
// group-ordered column: a table of many small clusters fills the device, a single label of m rows costs m dependent
// steps on one lane.  C++ float and double, no contraction.
//
// Events.  A sorted position counts when it is its label's first or when frame - previous frame > 3 in the frame
// column's own integer type: an unsigned column that decreases inside a label wraps and counts.
//
// Hull.  Rows are ordered by (label, x, y): a stable sort by y, then by x, then by the label key, on float64 keys made
// monotone (-0.0 counted as 0.0).  One lane per label runs Andrew's monotone chain over its run (lower chain, then upper
// chain, the vertex stack in the label's own slice of an n-entry scratch array) and sums the shoelace terms relative to
// the first hull vertex in float64.  Fewer than three vertices, duplicates, exactly collinear rows and a coordinate that
// is not finite give 0.0.
//
// Every loop is bounded by the row count; no float atomics.
#include <algorithm>

#include "rows_groups.h"
#include "segment_stats.h"

#pragma clang fp contract(off)

namespace pmi {
namespace centers {

using namespace rows;
using segstats::quiet_nan;

constexpr int MAX_COLS = 32;

// ---- order -----------------------------------------------------------------------------------------------------
__global__ void flag_kernel(const uint64_t *__restrict__ keys, int32_t n, uint32_t *__restrict__ flag)
{
    const int64_t p = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (p >= n) return;
    flag[p] = (p == 0 || keys[p] != keys[p - 1]) ? 1u : 0u;
}

// pos = exclusive scan of flag: label pos[p] starts at p; the last position also closes the table
__global__ void start_kernel(const uint64_t *__restrict__ keys, const uint32_t *__restrict__ flag,
                             const uint32_t *__restrict__ pos, int32_t n, uint64_t g_min, int32_t *__restrict__ start,
                             int64_t *__restrict__ unique, uint32_t *__restrict__ total)
{
    const int64_t p = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (p >= n) return;
    const uint32_t g = pos[p];
    const uint32_t G = close_runs(p, n, flag[p], g, (int32_t)p, n, start);
    if (flag[p] && g < (uint32_t)n) unique[g] = (int64_t)(keys[p] + g_min);
    if (p == n - 1) total[0] = G;
}

static int order(const int64_t *group, int32_t n, int64_t g_min, int64_t g_max, int32_t *rows_out, int32_t *start,
                 int64_t *unique, int64_t *n_groups, hipStream_t s)
{
    const size_t N = (size_t)n;
    uint64_t *keys, *keys_sorted;
    int32_t *rows;
    uint32_t *flag, *pos, *total;
    int rc = carve(SCR_STAGE_A, [&](Arena &ar) {
        keys = ar.take<uint64_t>(N), keys_sorted = ar.take<uint64_t>(N);
        rows = ar.take<int32_t>(N);
        flag = ar.take<uint32_t>(N), pos = ar.take<uint32_t>(N), total = ar.take<uint32_t>(1);
    });
    if (rc != PMI_OK) return rc;
    if ((rc = sort_by_column(group, g_min, g_max, true, keys, keys_sorted, rows, rows_out, n, s)) != PMI_OK) return rc;
    PMI_LAUNCH(flag_kernel, n, s, keys_sorted, n, flag);
    if ((rc = exclusive_scan_u32(flag, pos, N, s)) != PMI_OK) return rc;
    PMI_LAUNCH(start_kernel, n, s, keys_sorted, flag, pos, n, (uint64_t)g_min, start, unique, total);
    uint32_t h_total = 0;
    PMI_HIP(hipMemcpyAsync(&h_total, total, 4, hipMemcpyDeviceToHost, s));
    PMI_HIP(hipStreamSynchronize(s));
    if (h_total < 1 || h_total > (uint32_t)n) {
        set_error("pmi_centers_order_dev: %u labels in %d rows", h_total, n);
        return PMI_ERR_HIP;
    }
    *n_groups = h_total;
    return PMI_OK;
}

// ---- the chains ------------------------------------------------------------------------------------------------
template <typename T>
__global__ void weights_kernel(const T *__restrict__ lpx, const T *__restrict__ lpy, int32_t n, T *__restrict__ w)
{
    const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    const T sum = lpx[i] + lpy[i];
    w[i] = (T)1 / (sum * sum);
}

template <typename T, typename W, typename A>
__global__ void gather_product_kernel(const T *__restrict__ data, const W *__restrict__ weight,
                                      const int32_t *__restrict__ rows, int32_t n, A *__restrict__ vs)
{
    const int64_t p = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (p >= n) return;
    const int32_t i = rows[p];
    vs[p] = row_ok(i, n) ? (A)data[i] * (A)weight[i] : (A)0;
}

template <typename A>
__global__ void chain_kernel(const A *__restrict__ vs, const int32_t *__restrict__ start, int32_t n, int32_t n_groups,
                             A *__restrict__ sum, A *__restrict__ mean, double *__restrict__ sd)
{
    const int64_t g = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (g >= n_groups) return;
    int32_t a, b;
    run_of(start, (int32_t)g, n, &a, &b);
    A sumx = 0, comp = 0;
    int64_t nobs = 0;
    double wmean = 0.0, acc = 0.0;
    for (int32_t p = a; p < b; ++p) {
        const A v = vs[p];
        if (v != v) continue;
        ++nobs;
        const A y = v - comp;
        const A t = sumx + y;
        comp = t - sumx - y;
        if (comp != comp) comp = 0;
        sumx = t;
        if (sd) {
            const double dv = (double)v, old = wmean;
            wmean += (dv - old) / (double)nobs;
            acc += (dv - wmean) * (dv - old);
        }
    }
    if (sum) sum[g] = sumx;
    if (mean) mean[g] = nobs ? sumx / (A)nobs : quiet_nan<A>();
    if (sd) sd[g] = nobs > 1 ? __builtin_sqrt(acc / (double)(nobs - 1)) : quiet_nan<double>();
}

template <typename T, bool FLOATING>
__global__ void first_kernel(const T *__restrict__ data, const int32_t *__restrict__ rows,
                             const int32_t *__restrict__ start, int32_t n, int32_t n_groups, T *__restrict__ out)
{
    const int64_t g = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (g >= n_groups) return;
    int32_t a, b;
    run_of(start, (int32_t)g, n, &a, &b);
    T first = 0;
    if constexpr (FLOATING) first = quiet_nan<T>();
    for (int32_t p = a; p < b; ++p) {
        const int32_t i = rows[p];
        if (!row_ok(i, n)) continue;
        const T v = data[i];
        if constexpr (FLOATING)
            if (v != v) continue;
        first = v;
        break;
    }
    out[g] = first;
}

// U: the frame column as unsigned bits, S: the type the difference is compared in
template <typename U, typename S>
__global__ void events_kernel(const U *__restrict__ frame, const int32_t *__restrict__ rows,
                              const int32_t *__restrict__ start, int32_t n, int32_t n_groups, int32_t *__restrict__ out)
{
    const int64_t g = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (g >= n_groups) return;
    int32_t a, b;
    run_of(start, (int32_t)g, n, &a, &b);
    int32_t events = 0;
    U prev = 0;
    for (int32_t p = a; p < b; ++p) {
        const int32_t i = rows[p];
        const U f = row_ok(i, n) ? frame[i] : (U)0;
        if (p == a || (S)(U)(f - prev) > (S)3) ++events;
        prev = f;
    }
    out[g] = events;
}

template <typename A>
static int chain(const A *vs, const int32_t *start, int32_t n, int32_t G, const pmi_centers_column &c, hipStream_t s)
{
    PMI_LAUNCH(chain_kernel<A>, G, s, vs, start, n, G, (A *)c.sum, (A *)c.mean, (double *)c.std);
    return PMI_OK;
}

template <typename T>
static int mean_typed(const pmi_centers_column &c, const int32_t *rows, const int32_t *start, int32_t n, int32_t G,
                      void *buf, hipStream_t s)
{
    using A = typename Column<T>::sum_type;
    PMI_LAUNCH((gather_kernel<T, A>), n, s, (const T *)c.data, rows, n, (A *)buf);
    return chain<A>((const A *)buf, start, n, G, c, s);
}

template <typename T, typename W, typename A>
static int xsum_typed(const pmi_centers_column &c, const int32_t *rows, const int32_t *start, int32_t n, int32_t G,
                      void *buf, hipStream_t s)
{
    PMI_LAUNCH((gather_product_kernel<T, W, A>), n, s, (const T *)c.data, (const W *)c.weight, rows, n, (A *)buf);
    return chain<A>((const A *)buf, start, n, G, c, s);
}

static int column(const pmi_centers_column &c, const int32_t *rows, const int32_t *start, int32_t n, int32_t G, void *buf,
                  hipStream_t s)
{
    const bool f32 = c.type == PMI_CENTERS_F32, w32 = c.w_type == PMI_CENTERS_F32;
    switch (c.op) {
    case PMI_CENTERS_MEAN:
        return with_column_type(c.type, [&](auto col) {
            return mean_typed<typename decltype(col)::type>(c, rows, start, n, G, buf, s);
        });
    case PMI_CENTERS_XSUM:
        if (f32 && w32) return xsum_typed<float, float, float>(c, rows, start, n, G, buf, s);
        if (f32) return xsum_typed<float, double, double>(c, rows, start, n, G, buf, s);
        if (w32) return xsum_typed<double, float, double>(c, rows, start, n, G, buf, s);
        return xsum_typed<double, double, double>(c, rows, start, n, G, buf, s);
    case PMI_CENTERS_FIRST:
        switch (c.type) {
        case PMI_CENTERS_F32:
            PMI_LAUNCH((first_kernel<float, true>), G, s, (const float *)c.data, rows, start, n, G, (float *)c.sum);
            return PMI_OK;
        case PMI_CENTERS_F64:
            PMI_LAUNCH((first_kernel<double, true>), G, s, (const double *)c.data, rows, start, n, G, (double *)c.sum);
            return PMI_OK;
        case PMI_CENTERS_U32:
        case PMI_CENTERS_I32:
            PMI_LAUNCH((first_kernel<uint32_t, false>), G, s, (const uint32_t *)c.data, rows, start, n, G, (uint32_t *)c.sum);
            return PMI_OK;
        default:
            PMI_LAUNCH((first_kernel<uint64_t, false>), G, s, (const uint64_t *)c.data, rows, start, n, G, (uint64_t *)c.sum);
            return PMI_OK;
        }
    default:      // PMI_CENTERS_EVENTS
        switch (c.type) {
        case PMI_CENTERS_U32:
            PMI_LAUNCH((events_kernel<uint32_t, uint32_t>), G, s, (const uint32_t *)c.data, rows, start, n, G, (int32_t *)c.sum);
            return PMI_OK;
        case PMI_CENTERS_I32:
            PMI_LAUNCH((events_kernel<uint32_t, int32_t>), G, s, (const uint32_t *)c.data, rows, start, n, G, (int32_t *)c.sum);
            return PMI_OK;
        case PMI_CENTERS_U64:
            PMI_LAUNCH((events_kernel<uint64_t, uint64_t>), G, s, (const uint64_t *)c.data, rows, start, n, G, (int32_t *)c.sum);
            return PMI_OK;
        default:
            PMI_LAUNCH((events_kernel<uint64_t, int64_t>), G, s, (const uint64_t *)c.data, rows, start, n, G, (int32_t *)c.sum);
            return PMI_OK;
        }
    }
}

// ---- hull ------------------------------------------------------------------------------------------------------
// a key that orders as the float64 value does; -0.0 is 0.0
__device__ __forceinline__ uint64_t ordered_key(double v)
{
    const uint64_t u = (uint64_t)__double_as_longlong(v + 0.0);
    return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}

template <typename T>
__global__ void coord_key_kernel(const T *__restrict__ v, const int32_t *__restrict__ rows /* null: the identity */,
                                 int32_t n, uint64_t *__restrict__ keys, int32_t *__restrict__ rows_out)
{
    const int64_t p = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (p >= n) return;
    const int32_t i = rows ? rows[p] : (int32_t)p;
    keys[p] = row_ok(i, n) ? ordered_key((double)v[i]) : 0;
    if (rows_out) rows_out[p] = (int32_t)p;
}

template <typename TX, typename TY>
__global__ void gather_xy_kernel(const TX *__restrict__ x, const TY *__restrict__ y, const int32_t *__restrict__ rows,
                                 int32_t n, double *__restrict__ xs, double *__restrict__ ys)
{
    const int64_t p = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (p >= n) return;
    const int32_t i = rows[p];
    xs[p] = row_ok(i, n) ? (double)x[i] : 0.0;
    ys[p] = row_ok(i, n) ? (double)y[i] : 0.0;
}

// (a - o) x (b - o)
__device__ __forceinline__ double cross(const double *__restrict__ xs, const double *__restrict__ ys, int32_t o, int32_t a,
                                        int32_t b)
{
    return (xs[a] - xs[o]) * (ys[b] - ys[o]) - (ys[a] - ys[o]) * (xs[b] - xs[o]);
}

__global__ void hull_kernel(const double *__restrict__ xs, const double *__restrict__ ys, const int32_t *__restrict__ start,
                            int32_t n, int32_t n_groups, int32_t *__restrict__ stack, double *__restrict__ area)
{
    const int64_t g = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (g >= n_groups) return;
    int32_t a, b;
    run_of(start, (int32_t)g, n, &a, &b);
    const int32_t m = b - a;
    double twice = 0.0;
    bool finite = true;                              // Qhull refuses an infinite coordinate: the reference's 0.0
    for (int32_t p = a; p < b; ++p) finite = finite && __builtin_isfinite(xs[p]) && __builtin_isfinite(ys[p]);
    if (m >= 3 && finite) {
        int32_t *st = stack + a;                     // at most m entries: every position is pushed once per chain
        for (int side = 0; side < 2; ++side) {       // lower, left to right; upper, right to left
            int32_t k = 0;
            for (int32_t q = 0; q < m; ++q) {
                const int32_t p = side == 0 ? a + q : b - 1 - q;
                while (k >= 2 && !(cross(xs, ys, st[k - 2], st[k - 1], p) > 0.0)) --k;      // pops at most what was pushed
                st[k++] = p;
            }
            for (int32_t j = 1; j < k; ++j) twice += cross(xs, ys, a, st[j - 1], st[j]);
        }
    }
    const double half = 0.5 * twice;
    area[g] = half > 0.0 ? half : (half < 0.0 ? -half : 0.0);
}

template <typename TX, typename TY>
static int hull_typed(const TX *x, const TY *y, const int64_t *group, int64_t g_min, int64_t g_max, const int32_t *start,
                      int32_t n, int32_t G, double *area, hipStream_t s)
{
    const size_t N = (size_t)n;
    uint64_t *keys, *keys_sorted;
    int32_t *rows, *rows_sorted, *stack;
    double *xs, *ys;
    int rc = carve(SCR_STAGE_A, [&](Arena &ar) {
        keys = ar.take<uint64_t>(N), keys_sorted = ar.take<uint64_t>(N);
        rows = ar.take<int32_t>(N), rows_sorted = ar.take<int32_t>(N), stack = ar.take<int32_t>(N);
        xs = ar.take<double>(N), ys = ar.take<double>(N);
    });
    if (rc != PMI_OK) return rc;
    PMI_LAUNCH(coord_key_kernel<TY>, n, s, y, nullptr, n, keys, rows);
    if ((rc = sort_pairs(keys, keys_sorted, rows, rows_sorted, N, 64, s)) != PMI_OK) return rc;
    PMI_LAUNCH(coord_key_kernel<TX>, n, s, x, rows_sorted, n, keys, nullptr);
    if ((rc = sort_pairs(keys, keys_sorted, rows_sorted, rows, N, 64, s)) != PMI_OK) return rc;
    if ((rc = sort_by_column(group, g_min, g_max, false, keys, keys_sorted, rows, rows_sorted, n, s)) != PMI_OK) return rc;
    PMI_LAUNCH((gather_xy_kernel<TX, TY>), n, s, x, y, rows_sorted, n, xs, ys);
    PMI_LAUNCH(hull_kernel, G, s, xs, ys, start, n, G, stack, area);
    PMI_HIP(hipStreamSynchronize(s));
    return PMI_OK;
}

static bool floating(int type) { return type == PMI_CENTERS_F32 || type == PMI_CENTERS_F64; }

}  // namespace centers
}  // namespace pmi

using namespace pmi;

extern "C" {

int pmi_centers_order_dev(const int64_t *d_group, int64_t n, int64_t g_min, int64_t g_max, int32_t *d_rows,
                          int32_t *d_start, int64_t *d_unique, int64_t *n_groups, void *stream)
{
    int rc = rows::check_rows("pmi_centers_order_dev", n, 0, "labels");
    if (rc) return rc;
    if (!n_groups || g_max < g_min || (n > 0 && (!d_group || !d_rows || !d_start || !d_unique))) {
        set_error("pmi_centers_order_dev: labels %lld .. %lld, or a NULL column", (long long)g_min, (long long)g_max);
        return PMI_ERR_ARG;
    }
    *n_groups = 0;
    if (n == 0) return PMI_OK;
    return centers::order(d_group, (int32_t)n, g_min, g_max, d_rows, d_start, d_unique, n_groups, (hipStream_t)stream);
}

int pmi_centers_weights_dev(const void *d_lpx, const void *d_lpy, int type, int64_t n, void *d_w, void *stream)
{
    int rc = rows::check_rows("pmi_centers_weights_dev", n, 0, "labels");
    if (rc) return rc;
    if (!centers::floating(type) || (n > 0 && (!d_lpx || !d_lpy || !d_w))) {
        set_error("pmi_centers_weights_dev: type %d, or a NULL column", type);
        return PMI_ERR_ARG;
    }
    if (n == 0) return PMI_OK;
    hipStream_t s = (hipStream_t)stream;
    if (type == PMI_CENTERS_F32)
        PMI_LAUNCH(centers::weights_kernel<float>, n, s, (const float *)d_lpx, (const float *)d_lpy, (int32_t)n, (float *)d_w);
    else
        PMI_LAUNCH(centers::weights_kernel<double>, n, s, (const double *)d_lpx, (const double *)d_lpy, (int32_t)n, (double *)d_w);
    PMI_HIP(hipStreamSynchronize(s));
    return PMI_OK;
}

int pmi_centers_stats_dev(const int32_t *d_rows, const int32_t *d_start, int64_t n, int64_t n_groups,
                          const pmi_centers_column *columns, int n_columns, void *stream)
{
    int rc = rows::check_rows("pmi_centers_stats_dev", n, n_groups, "labels");
    if (rc) return rc;
    if (n_columns < 0 || n_columns > centers::MAX_COLS || (n_columns > 0 && !columns) ||
        (n > 0 && (!d_rows || !d_start))) {
        set_error("pmi_centers_stats_dev: %d columns (at most %d), or a NULL table", n_columns, centers::MAX_COLS);
        return PMI_ERR_ARG;
    }
    for (int i = 0; i < n_columns; ++i) {
        const pmi_centers_column &c = columns[i];
        const bool known = c.type >= PMI_CENTERS_F32 && c.type <= PMI_CENTERS_I64;
        const bool ok = !c.data || !known ? false
                        : c.op == PMI_CENTERS_MEAN ? (c.sum || c.mean || c.std)
                        : c.op == PMI_CENTERS_XSUM ? (c.sum && c.weight && centers::floating(c.type) && centers::floating(c.w_type))
                        : c.op == PMI_CENTERS_FIRST ? c.sum != nullptr
                        : c.op == PMI_CENTERS_EVENTS ? (c.sum && !centers::floating(c.type)) : false;
        if (!ok) {
            set_error("pmi_centers_stats_dev: column %d: op %d, types %d / %d", i, c.op, c.type, c.w_type);
            return PMI_ERR_ARG;
        }
    }
    if (n == 0 || n_groups == 0) return PMI_OK;
    hipStream_t s = (hipStream_t)stream;
    double *buf;      // one gathered column, of either width
    rc = rows::carve(SCR_STAGE_A, [&](rows::Arena &ar) { buf = ar.take<double>((size_t)n); });
    if (rc != PMI_OK) return rc;
    for (int i = 0; i < n_columns; ++i)
        if ((rc = centers::column(columns[i], d_rows, d_start, (int32_t)n, (int32_t)n_groups, buf, s)) != PMI_OK) return rc;
    PMI_HIP(hipStreamSynchronize(s));
    return PMI_OK;
}

int pmi_centers_hull_dev(const void *d_x, int x_type, const void *d_y, int y_type, const int64_t *d_group,
                         int64_t g_min, int64_t g_max, const int32_t *d_start, int64_t n, int64_t n_groups,
                         double *d_area, void *stream)
{
    int rc = rows::check_rows("pmi_centers_hull_dev", n, n_groups, "labels");
    if (rc) return rc;
    if (!centers::floating(x_type) || !centers::floating(y_type) || g_max < g_min ||
        (n > 0 && (!d_x || !d_y || !d_group || !d_start)) || (n_groups > 0 && !d_area)) {
        set_error("pmi_centers_hull_dev: x / y must be float32 or float64 (codes %d, %d), labels %lld .. %lld", x_type,
                  y_type, (long long)g_min, (long long)g_max);
        return PMI_ERR_ARG;
    }
    if (n == 0 || n_groups == 0) return PMI_OK;
    hipStream_t s = (hipStream_t)stream;
    const int32_t N = (int32_t)n, G = (int32_t)n_groups;
    if (x_type == PMI_CENTERS_F32)
        return y_type == PMI_CENTERS_F32
                   ? centers::hull_typed((const float *)d_x, (const float *)d_y, d_group, g_min, g_max, d_start, N, G, d_area, s)
                   : centers::hull_typed((const float *)d_x, (const double *)d_y, d_group, g_min, g_max, d_start, N, G, d_area, s);
    return y_type == PMI_CENTERS_F32
               ? centers::hull_typed((const double *)d_x, (const float *)d_y, d_group, g_min, g_max, d_start, N, G, d_area, s)
               : centers::hull_typed((const double *)d_x, (const double *)d_y, d_group, g_min, g_max, d_start, N, G, d_area, s);
}

}  // extern "C"
