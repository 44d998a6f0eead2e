// kinetics.hip — the dark time of every binding event (picasso/postprocess.py:1985-2004 _dark_times) and the per-group
// mean and standard deviation of every column (picasso/postprocess.py:3580-3649 groupprops), in the reference's values.
//
// Dark times.  The reference takes, for row i, the smallest frame[i] - last_frame[j] > 0 over the other rows j of its
// group, and keeps it when it is below max_frame = frame.max(): per group that is the largest last_frame below
// frame[i], so no pair loop is needed.  Rows are ordered by (group key, last_frame) with two stable radix sorts (the
// group key is group - g_min as in centers.hip, the last frame is last_frame - l_min), the runs of equal group keys come
// from flags and one exclusive scan, and one lane per sorted position bisects its own run for its own frame.  The
// candidate below the frame may be the row itself (len <= 0 in a hand-made table): the lane then steps to the one
// before it, which may hold the same value.  Differences are signed 64-bit.
//
// Group properties.  pandas' Series.mean() / Series.std() of a group are NumPy sums (nanops.nanmean / nanvar): NaN
// counts as 0 and is counted out; the mean is the sum in the column's own floating type (integers as float64) over the
// count in that type; std (ddof 1) takes avg = the float64 sum over the count, sums (avg - v)^2 in float64, divides by
// count - 1, and takes the root in float32 for a float32 column and in float64 otherwise.  Every sum is NumPy's
// add.reduce of a contiguous array: an accumulator that starts at 0 and takes the pairwise sum of each 8192-element
// chunk in order; pairwise is a serial loop below 8 elements, eight strided accumulators up to 128, and a split at
// n / 2 rounded down to a multiple of 8 above.  One lane walks one group's run of the gathered, group-ordered column
// (the order is pmi_centers_order_dev's).  C++ float and double, no contraction.  The sums and the two pandas statistics
// are segment_stats.h's, which combine.hip shares.
//
// Every loop is bounded by the row count; no float atomics; an inconsistent table gives an empty run.
#include "rows_groups.h"
#include "segment_stats.h"

#pragma clang fp contract(off)

namespace pmi {
namespace kinetics {

using namespace rows;

constexpr int MAX_COLS = 64;

// ---- dark times: order -----------------------------------------------------------------------------------------
__global__ void flag_kernel(const uint64_t *__restrict__ keys, const int64_t *__restrict__ last,
                            const int32_t *__restrict__ rows, int32_t n, uint32_t *__restrict__ flag,
                            int64_t *__restrict__ last_sorted)
{
    const int64_t p = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (p >= n) return;
    flag[p] = (p == 0 || keys[p] != keys[p - 1]) ? 1u : 0u;
    const int32_t i = rows[p];
    last_sorted[p] = row_ok(i, n) ? last[i] : 0;
}

// pos = exclusive scan of flag: run pos[p] starts at the flagged p; the last position also closes the table
__global__ void start_kernel(const uint32_t *__restrict__ flag, const uint32_t *__restrict__ pos, int32_t n,
                             int32_t *__restrict__ start, int32_t *__restrict__ run)
{
    const int64_t p = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (p >= n) return;
    // the runs up to and including this position, >= 1: a position that is not flagged lies in the run before pos[p]
    run[p] = (int32_t)close_runs(p, n, flag[p], pos[p], (int32_t)p, n, start) - 1;
}

static int dark_order(const int64_t *last, const int64_t *group, int32_t n, int64_t l_min, int64_t l_max, int64_t g_min,
                      int64_t g_max, int32_t *rows_out, int64_t *last_sorted, int32_t *run, int32_t *start, hipStream_t s)
{
    const size_t N = (size_t)n;
    uint64_t *keys, *keys_sorted;
    int32_t *rows, *rows_mid;
    uint32_t *flag, *pos;
    int rc = carve(SCR_STAGE_A, [&](Arena &ar) {
        keys = ar.take<uint64_t>(N), keys_sorted = ar.take<uint64_t>(N);
        rows = ar.take<int32_t>(N), rows_mid = ar.take<int32_t>(N);
        flag = ar.take<uint32_t>(N), pos = ar.take<uint32_t>(N);
    });
    if (rc != PMI_OK) return rc;
    // a start table that the kernels below do not fill (they fill all of it on a consistent input) holds empty runs
    PMI_HIP(hipMemsetAsync(start, 0, (N + 1) * sizeof(int32_t), s));
    if ((rc = sort_by_column(last, l_min, l_max, true, keys, keys_sorted, rows, rows_mid, n, s)) != PMI_OK) return rc;
    if ((rc = sort_by_column(group, g_min, g_max, false, keys, keys_sorted, rows_mid, rows_out, n, s)) != PMI_OK) return rc;
    PMI_LAUNCH(flag_kernel, n, s, keys_sorted, last, rows_out, n, flag, last_sorted);
    if ((rc = exclusive_scan_u32(flag, pos, N, s)) != PMI_OK) return rc;
    PMI_LAUNCH(start_kernel, n, s, flag, pos, n, start, run);
    PMI_HIP(hipStreamSynchronize(s));
    return PMI_OK;
}

// ---- dark times: search ----------------------------------------------------------------------------------------
__global__ void dark_kernel(const int64_t *__restrict__ frame, const int32_t *__restrict__ rows,
                            const int64_t *__restrict__ last_sorted, const int32_t *__restrict__ run,
                            const int32_t *__restrict__ start, int32_t n, int64_t max_frame, int64_t *__restrict__ dark)
{
    const int64_t q = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (q >= n) return;
    const int32_t i = rows[q];
    if (!row_ok(i, n)) return;
    int64_t out = -1;
    const int32_t g = run[q];
    if (row_ok(g, n)) {
        int32_t a, b;
        run_of(start, g, n, &a, &b);
        if (a <= q && q < b) {
            const int64_t f = frame[i];
            int32_t p = lower_bound(last_sorted, a, b, f) - 1;      // the last position of the run that ends before f
            if (p == (int32_t)q) --p;                               // the row itself is no candidate
            if (p >= a) {
                const int64_t d = f - last_sorted[p];
                if (d > 0 && d < max_frame) out = d;
            }
        }
    }
    dark[i] = out;
}

// ---- group properties ------------------------------------------------------------------------------------------
template <typename A>
__global__ void stats_kernel(const A *__restrict__ vs, const int32_t *__restrict__ start, int32_t n, int32_t n_groups,
                             double *__restrict__ mean, double *__restrict__ sd)
{
    const int64_t g = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (g >= n_groups) return;
    int32_t a, b;
    run_of(start, (int32_t)g, n, &a, &b);
    if (mean) mean[g] = segstats::series_mean<A>(vs, a, b);
    if (sd) sd[g] = segstats::series_std<A>(vs, a, b);
}

template <typename T>
static int column_typed(const pmi_kinetics_column &c, const int32_t *rows, const int32_t *start, int32_t n, int32_t G,
                        void *buf, hipStream_t s)
{
    using A = typename Column<T>::sum_type;
    PMI_LAUNCH((gather_kernel<T, A>), n, s, (const T *)c.data, rows, n, (A *)buf);
    PMI_LAUNCH(stats_kernel<A>, G, s, (const A *)buf, start, n, G, c.mean, c.std);
    return PMI_OK;
}

static int column(const pmi_kinetics_column &c, const int32_t *rows, const int32_t *start, int32_t n, int32_t G, void *buf,
                  hipStream_t s)
{
    return with_column_type(c.type, [&](auto col) {
        return column_typed<typename decltype(col)::type>(c, rows, start, n, G, buf, s);
    });
}

}  // namespace kinetics
}  // namespace pmi

using namespace pmi;

extern "C" {

int pmi_kinetics_dark_order_dev(const int64_t *d_last, const int64_t *d_group, int64_t n, int64_t l_min, int64_t l_max,
                                int64_t g_min, int64_t g_max, int32_t *d_rows, int64_t *d_last_sorted, int32_t *d_run,
                                int32_t *d_start, void *stream)
{
    int rc = rows::check_rows("pmi_kinetics_dark_order_dev", n, 0, "groups");
    if (rc) return rc;
    if (l_max < l_min || g_max < g_min ||
        (n > 0 && (!d_last || !d_group || !d_rows || !d_last_sorted || !d_run || !d_start))) {
        set_error("pmi_kinetics_dark_order_dev: last frames %lld .. %lld, groups %lld .. %lld, or a NULL column",
                  (long long)l_min, (long long)l_max, (long long)g_min, (long long)g_max);
        return PMI_ERR_ARG;
    }
    if (n == 0) return PMI_OK;
    return kinetics::dark_order(d_last, d_group, (int32_t)n, l_min, l_max, g_min, g_max, d_rows, d_last_sorted, d_run,
                                d_start, (hipStream_t)stream);
}

int pmi_kinetics_dark_search_dev(const int64_t *d_frame, const int32_t *d_rows, const int64_t *d_last_sorted,
                                 const int32_t *d_run, const int32_t *d_start, int64_t n, int64_t max_frame,
                                 int64_t *d_dark, void *stream)
{
    int rc = rows::check_rows("pmi_kinetics_dark_search_dev", n, 0, "groups");
    if (rc) return rc;
    if (n > 0 && (!d_frame || !d_rows || !d_last_sorted || !d_run || !d_start || !d_dark)) {
        set_error("pmi_kinetics_dark_search_dev: a NULL column");
        return PMI_ERR_ARG;
    }
    if (n == 0) return PMI_OK;
    hipStream_t s = (hipStream_t)stream;
    // a row that no sorted position names keeps -1
    PMI_HIP(hipMemsetAsync(d_dark, 0xff, (size_t)n * sizeof(int64_t), s));
    PMI_LAUNCH(kinetics::dark_kernel, n, s, d_frame, d_rows, d_last_sorted, d_run, d_start, (int32_t)n, max_frame, d_dark);
    PMI_HIP(hipStreamSynchronize(s));
    return PMI_OK;
}

int pmi_kinetics_stats_dev(const int32_t *d_rows, const int32_t *d_start, int64_t n, int64_t n_groups,
                           const pmi_kinetics_column *columns, int n_columns, void *stream)
{
    int rc = rows::check_rows("pmi_kinetics_stats_dev", n, n_groups, "groups");
    if (rc) return rc;
    if (n_columns < 0 || n_columns > kinetics::MAX_COLS || (n_columns > 0 && !columns) ||
        (n > 0 && (!d_rows || !d_start))) {
        set_error("pmi_kinetics_stats_dev: %d columns (at most %d), or a NULL table", n_columns, kinetics::MAX_COLS);
        return PMI_ERR_ARG;
    }
    for (int i = 0; i < n_columns; ++i) {
        const pmi_kinetics_column &c = columns[i];
        if (!c.data || c.type < PMI_CENTERS_F32 || c.type > PMI_CENTERS_I64 || (!c.mean && !c.std)) {
            set_error("pmi_kinetics_stats_dev: column %d: type %d, or nothing to compute", i, c.type);
            return PMI_ERR_ARG;
        }
    }
    if (n == 0 || n_groups == 0) return PMI_OK;
    hipStream_t s = (hipStream_t)stream;
    double *buf;      // one gathered column, of either width
    rc = rows::carve(SCR_STAGE_A, [&](rows::Arena &ar) { buf = ar.take<double>((size_t)n); });
    if (rc != PMI_OK) return rc;
    for (int i = 0; i < n_columns; ++i)
        if ((rc = kinetics::column(columns[i], d_rows, d_start, (int32_t)n, (int32_t)n_groups, buf, s)) != PMI_OK) return rc;
    PMI_HIP(hipStreamSynchronize(s));
    return PMI_OK;
}

}  // extern "C"
