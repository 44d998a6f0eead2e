// link.hip — linking of localizations into binding events and the NeNA histogram
// (picasso/postprocess.py:2441-2552 _get_link_groups, :2555-2661 _link_group_*, :1212-1272 _nfndh / _fill_dnfl).
//
// All kernels take the columns of a table SORTED BY FRAME, as the reference's loops do.
//
// Frame index.  Per row i, by bisection of the rows behind it:
//     lo[i] = first row j > i with frame[j] >= frame[i] + 1,     hi[i] = first row j > i with frame[j] > frame[i] + k,
// n where there is none.  The reference finds both with linear loops whose variable keeps its last value when no row
// qualifies; window() restates what its third loop then scans:
//     link   lo found: [lo, hi);  not found: row n - 1 alone, unless frame[n - 1] > frame[i] + k
//     NeNA   [lo or n - 1, hi or n - 1): the last row of the table is never a neighbour
// The last row of the table has no window (the reference leaves its loop variable unassigned there): it ends its
// chain and adds nothing to the histogram.
//
// Link groups.  The reference walks the rows in order; an unassigned row starts a group, and the chain then takes the
// FIRST unassigned row of the window that is in the same `group` and passes dx2 <= r2, dy2 <= r2, dx2 + dy2 <= r2.
// A row is only ever taken by a row it passes that test with, so the connected components of that relation do not
// see each other:
//     1. union_kernel     every row scans its window and unions itself with each candidate (parent[] with
//                         atomicCAS, a parent is always a lower row, the root is the lowest row of the component)
//     2. root_kernel      root of every row; stable radix sort of the rows by root (rocPRIM)
//     3. replay_kernel    one lane per component runs the reference's loop on the component's rows
//     4. exclusive scan of the chain-start flags: link_group[i] = rank of the row that started i's chain
// One huge component is correct but serial on one lane.
//
// Arithmetic is the reference's under numba: with float32 columns the difference, its square and dx2 + dy2 are
// float32 and are compared with the float64 r2; np.sqrt of a float32 is float32, d / bin_size is float64; float64
// columns make everything float64; a float32 with a float64 column gives a float64 sum.  No contraction.
//
// Combine.  Rows are sorted by link_group (stable: row order survives) and one lane walks each group: count,
// min / max frame, last row, and per column descriptor a sum in the column's own dtype IN ROW ORDER — of the column,
// of w = 1 / lp^2, or of column * w.  Nothing is accumulated with atomics.
//
// Every loop is bounded by the row count; a union that does not settle within its bound reports a status.
#include <algorithm>
#include <type_traits>

#include "rows_common.h"

#pragma clang fp contract(off)

namespace pmi {
namespace link {

using namespace rows;

constexpr int MAX_BINS = 8192;       // NeNA histogram in LDS: 32 KB
constexpr int MAX_COLS = 24;

// One rounding per operation: plain operators, which the pragma above keeps from being contracted into an FMA (the
// __f*_rn intrinsics are inline functions of a header compiled with contraction allowed, and __fsqrt_rn is the
// native approximation).  Division and square root of float32 are correctly rounded, hipcc's default.
template <typename T> __device__ __forceinline__ T sub_rn(T a, T b) { return a - b; }
template <typename T> __device__ __forceinline__ T mul_rn(T a, T b) { return a * b; }
template <typename T> __device__ __forceinline__ T add_rn(T a, T b) { return a + b; }
template <typename T> __device__ __forceinline__ T div_rn(T a, T b) { return a / b; }
__device__ __forceinline__ float sqrt_rn(float a) { return __builtin_sqrtf(a); }
__device__ __forceinline__ double sqrt_rn(double a) { return __builtin_sqrt(a); }

__global__ void frame_index_kernel(const int64_t *__restrict__ frame, int32_t n, int64_t k, int32_t *__restrict__ lo,
                                   int32_t *__restrict__ hi)
{
    const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    const int64_t f = frame[i];
    lo[i] = lower_bound(frame, (int32_t)i + 1, n, f + 1);
    hi[i] = lower_bound(frame, (int32_t)i + 1, n, f + k + 1);
}

// rows the reference's candidate loop scans for current row i (i < n - 1)
__device__ __forceinline__ void link_window(const int64_t *__restrict__ frame, const int32_t *__restrict__ lo,
                                            const int32_t *__restrict__ hi, int32_t n, int64_t k, int32_t i, int32_t *a,
                                            int32_t *b)
{
    const int32_t l = lo[i];
    if (l < n) { *a = l; *b = hi[i]; return; }
    *a = n - 1;
    *b = (frame[n - 1] > frame[i] + k) ? n - 1 : n;
}

template <typename TX, typename TY>
struct Pair {
    using S = decltype(TX() + TY());
    // dx2 <= r2, dy2 <= r2, dx2 + dy2 <= r2 with the squares in the columns' types and the comparisons in float64
    __device__ static __forceinline__ bool within(TX cx, TY cy, TX xj, TY yj, double r2, S *sum)
    {
        const TX dx = sub_rn(cx, xj);
        const TX dx2 = mul_rn(dx, dx);
        if (!((double)dx2 <= r2)) return false;
        const TY dy = sub_rn(cy, yj);
        const TY dy2 = mul_rn(dy, dy);
        if (!((double)dy2 <= r2)) return false;
        *sum = add_rn((S)dx2, (S)dy2);
        return true;
    }
};

template <typename TX, typename TY>
__global__ void union_kernel(const int64_t *__restrict__ frame, const TX *__restrict__ x, const TY *__restrict__ y,
                             const int64_t *__restrict__ group, const int32_t *__restrict__ lo,
                             const int32_t *__restrict__ hi, int32_t n, int64_t k, double r2, int32_t *parent,
                             int32_t *status)
{
    const int64_t i64 = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i64 >= n - 1) return;
    const int32_t i = (int32_t)i64;
    int32_t a, b;
    link_window(frame, lo, hi, n, k, i, &a, &b);
    const TX cx = x[i];
    const TY cy = y[i];
    const int64_t cg = group[i];
    for (int32_t j = a; j < b; ++j) {
        if (group[j] != cg) continue;
        typename Pair<TX, TY>::S sum;
        if (!Pair<TX, TY>::within(cx, cy, x[j], y[j], r2, &sum)) continue;
        if ((double)sum <= r2) unite(parent, i, j, n, status);
    }
}

__global__ void root_kernel(const int32_t *__restrict__ parent, int32_t n, uint32_t *__restrict__ root,
                            int32_t *__restrict__ start_of)
{
    const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    root[i] = (uint32_t)find_root(parent, (int32_t)i, n);
    start_of[i] = -1;
}

// One lane per component (the lane of its root row): the reference's loop over the component's rows `rows[p0 .. p1)`,
// ascending.  start_of[i] = the row that started i's chain; only this lane reads or writes the component's entries.
template <typename TX, typename TY>
__global__ void replay_kernel(const int64_t *__restrict__ frame, const TX *__restrict__ x, const TY *__restrict__ y,
                              const int64_t *__restrict__ group, const int32_t *__restrict__ lo,
                              const int32_t *__restrict__ hi, int32_t n, int64_t k, double r2,
                              const uint32_t *__restrict__ sorted_root, const int32_t *__restrict__ rows,
                              int32_t *start_of)
{
    const int64_t r64 = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (r64 >= n) return;
    const int32_t r = (int32_t)r64;
    const int32_t p0 = lower_bound(sorted_root, 0, n, (uint32_t)r);
    if (p0 >= n || sorted_root[p0] != (uint32_t)r) return;          // r is not a root
    int32_t p1 = p0 + 1;
    if (p1 < n && sorted_root[p1] == (uint32_t)r) p1 = lower_bound(sorted_root, 0, n, (uint32_t)r + 1u);
    for (int32_t s = p0; s < p1; ++s) {
        const int32_t first = rows[s];
        if (start_of[first] != -1) continue;
        start_of[first] = first;
        int32_t cur = first, p = s + 1;
        while (cur < n - 1 && p < p1) {                             // each pass moves p forward or ends the chain
            int32_t a, b;
            link_window(frame, lo, hi, n, k, cur, &a, &b);
            while (p < p1 && rows[p] < a) ++p;
            const TX cx = x[cur];
            const TY cy = y[cur];
            const int64_t cg = group[cur];
            int32_t next = -1, q = p;
            for (; q < p1; ++q) {
                const int32_t j = rows[q];
                if (j >= b) break;
                if (group[j] != cg || start_of[j] != -1) continue;
                typename Pair<TX, TY>::S sum;
                if (!Pair<TX, TY>::within(cx, cy, x[j], y[j], r2, &sum)) continue;
                if ((double)sum <= r2) { next = j; break; }
            }
            if (next < 0) break;
            start_of[next] = first;
            cur = next;
            p = q + 1;
        }
    }
}

__global__ void start_flag_kernel(const int32_t *__restrict__ start_of, int32_t n, uint32_t *__restrict__ flag)
{
    const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    flag[i] = start_of[i] == (int32_t)i ? 1u : 0u;
}

__global__ void label_kernel(const int32_t *__restrict__ start_of, const uint32_t *__restrict__ rank, int32_t n,
                             int32_t *__restrict__ link_group, int32_t *status)
{
    const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    const int32_t s = start_of[i];
    if (s < 0 || s >= n) { link_group[i] = -1; atomicExch(status, 2); return; }
    link_group[i] = (int32_t)rank[s];
}

// ---- NeNA ------------------------------------------------------------------------------------------------------
template <typename TX, typename TY>
__global__ void nena_kernel(const int64_t *__restrict__ frame, const TX *__restrict__ x, const TY *__restrict__ y,
                            const int64_t *__restrict__ group, const int32_t *__restrict__ lo,
                            const int32_t *__restrict__ hi, int32_t n, int32_t n_visit, double d_max, double bin_size,
                            int32_t n_bins, unsigned long long *__restrict__ hist)
{
    extern __shared__ uint32_t bins[];
    for (int32_t b = threadIdx.x; b < n_bins; b += BLOCK) bins[b] = 0;
    __syncthreads();
    const double r2 = d_max * d_max;
    const int64_t stride = (int64_t)gridDim.x * BLOCK;
    for (int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x; i < n_visit; i += stride) {
        if (i >= n - 1) continue;                                   // the table's last row has no next row
        const int32_t l = lo[i], h = hi[i];
        const int32_t a = l < n ? l : n - 1, b = h < n ? h : n - 1;
        const TX cx = x[i];
        const TY cy = y[i];
        const int64_t cg = group[i];
        for (int32_t j = a; j < b; ++j) {
            if (group[j] != cg) continue;
            typename Pair<TX, TY>::S sum;
            if (!Pair<TX, TY>::within(cx, cy, x[j], y[j], r2, &sum)) continue;
            const auto d = sqrt_rn(sum);
            if (!((double)d <= d_max)) continue;
            const double q = div_rn((double)d, bin_size);
            if (!(q >= 0.0 && q < (double)n_bins)) continue;        // d == d_max: one past the last bin, dropped
            atomicAdd(&bins[(int32_t)q], 1u);
        }
    }
    __syncthreads();
    for (int32_t b = threadIdx.x; b < n_bins; b += BLOCK)
        if (bins[b]) atomicAdd(&hist[b], (unsigned long long)bins[b]);
}

// ---- combine -----------------------------------------------------------------------------------------------------
struct Col {
    const void *a, *w;      // column, and the precision column of PMI_LINK_WSUM / PMI_LINK_XWSUM
    void *out;
    int32_t op, ta, tw;
};
struct Cols {
    Col c[MAX_COLS];
    int32_t n;
};

template <typename T>
__device__ __forceinline__ T weight(const void *w, int32_t r)
{
    const T lp = ((const T *)w)[r];
    return div_rn((T)1, mul_rn(lp, lp));
}

template <typename T>
__device__ void sum_plain(const Col &c, const int32_t *__restrict__ rows, int32_t p0, int32_t p1, int32_t g)
{
    T acc = 0;
    for (int32_t p = p0; p < p1; ++p) {
        const T v = ((const T *)c.a)[rows[p]];
        if constexpr (std::is_floating_point<T>::value) acc = add_rn(acc, v); else acc += v;
    }
    ((T *)c.out)[g] = acc;
}

template <typename T>
__device__ void sum_weight(const Col &c, const int32_t *__restrict__ rows, int32_t p0, int32_t p1, int32_t g)
{
    T acc = 0;
    for (int32_t p = p0; p < p1; ++p) acc = add_rn(acc, weight<T>(c.w, rows[p]));
    ((T *)c.out)[g] = acc;
}

template <typename TA, typename TW>
__device__ void sum_weighted(const Col &c, const int32_t *__restrict__ rows, int32_t p0, int32_t p1, int32_t g)
{
    using S = decltype(TA() + TW());
    S acc = 0;
    for (int32_t p = p0; p < p1; ++p) {
        const int32_t r = rows[p];
        acc = add_rn(acc, mul_rn((S)((const TA *)c.a)[r], (S)weight<TW>(c.w, r)));
    }
    ((S *)c.out)[g] = acc;
}

__global__ void group_key_kernel(const int32_t *__restrict__ link_group, int32_t n, int32_t n_groups,
                                 uint32_t *__restrict__ key)
{
    const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    const int32_t g = link_group[i];
    key[i] = (g >= 0 && g < n_groups) ? (uint32_t)g : (uint32_t)n_groups;
}

__global__ void combine_kernel(const uint32_t *__restrict__ sorted_group, const int32_t *__restrict__ rows, int32_t n,
                               int32_t n_groups, const int64_t *__restrict__ frame, Cols cols,
                               uint32_t *__restrict__ count, int64_t *__restrict__ first, int64_t *__restrict__ last,
                               int32_t *__restrict__ last_row)
{
    const int64_t g64 = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (g64 >= n_groups) return;
    const int32_t g = (int32_t)g64;
    const int32_t p0 = lower_bound(sorted_group, 0, n, (uint32_t)g);
    const int32_t p1 = lower_bound(sorted_group, 0, n, (uint32_t)g + 1u);
    count[g] = (uint32_t)(p1 - p0);
    int64_t fmin = INT64_MAX, fmax = INT64_MIN;
    if (frame)
        for (int32_t p = p0; p < p1; ++p) {
            const int64_t f = frame[rows[p]];
            fmin = f < fmin ? f : fmin;
            fmax = f > fmax ? f : fmax;
        }
    if (first) first[g] = fmin;
    if (last) last[g] = fmax;
    last_row[g] = p1 > p0 ? rows[p1 - 1] : -1;
    for (int32_t k = 0; k < cols.n; ++k) {
        const Col &c = cols.c[k];
        if (c.op == PMI_LINK_SUM) {
            switch (c.ta) {
            case PMI_LINK_F32: sum_plain<float>(c, rows, p0, p1, g); break;
            case PMI_LINK_F64: sum_plain<double>(c, rows, p0, p1, g); break;
            case PMI_LINK_U32: sum_plain<uint32_t>(c, rows, p0, p1, g); break;
            default: sum_plain<uint64_t>(c, rows, p0, p1, g); break;
            }
        } else if (c.op == PMI_LINK_WSUM) {
            if (c.tw == PMI_LINK_F32) sum_weight<float>(c, rows, p0, p1, g); else sum_weight<double>(c, rows, p0, p1, g);
        } else {
            if (c.ta == PMI_LINK_F32 && c.tw == PMI_LINK_F32) sum_weighted<float, float>(c, rows, p0, p1, g);
            else if (c.ta == PMI_LINK_F32) sum_weighted<float, double>(c, rows, p0, p1, g);
            else if (c.tw == PMI_LINK_F32) sum_weighted<double, float>(c, rows, p0, p1, g);
            else sum_weighted<double, double>(c, rows, p0, p1, g);
        }
    }
}

// ---- host ------------------------------------------------------------------------------------------------------
static int frame_index(const int64_t *d_frame, int32_t n, int64_t k, int32_t *lo, int32_t *hi, hipStream_t s)
{
    if (n == 0) return PMI_OK;
    PMI_LAUNCH(frame_index_kernel, n, s, d_frame, n, k, lo, hi);
    return PMI_OK;
}

// rows sorted by key (stable) -> keys_out, rows_out; keys < 2^bits
static int sort_rows(uint32_t *keys, uint32_t *keys_out, int32_t *rows, int32_t *rows_out, int32_t n, int64_t key_end,
                     hipStream_t s)
{
    return sort_pairs(keys, keys_out, rows, rows_out, (size_t)n, bits_of((uint64_t)(key_end - 1)), s);
}

template <typename TX, typename TY>
static int groups_typed(const TX *x, const TY *y, const int64_t *frame, const int64_t *group, int32_t n, double r2,
                        int64_t k, int32_t *link_group, int64_t *n_groups, hipStream_t s)
{
    const size_t N = (size_t)n;
    int32_t *lo, *hi, *parent, *rows, *rows_sorted, *start_of, *status;
    uint32_t *root, *root_sorted, *rank;
    int rc = carve(SCR_STAGE_A, [&](Arena &ar) {
        lo = ar.take<int32_t>(N), hi = ar.take<int32_t>(N), parent = ar.take<int32_t>(N);
        root = ar.take<uint32_t>(N), root_sorted = ar.take<uint32_t>(N);
        rows = ar.take<int32_t>(N), rows_sorted = ar.take<int32_t>(N), start_of = ar.take<int32_t>(N);
        rank = ar.take<uint32_t>(N);
        status = ar.take<int32_t>(4);
    });
    if (rc != PMI_OK) return rc;
    uint32_t *flag = root;                                          // the roots are dead once they are sorted

    PMI_HIP(hipMemsetAsync(status, 0, 16, s));
    if ((rc = frame_index(frame, n, k, lo, hi, s)) != PMI_OK) return rc;
    PMI_LAUNCH(iota_kernel, n, s, parent, rows, n);
    PMI_LAUNCH((union_kernel<TX, TY>), n, s, frame, x, y, group, lo, hi, n, k, r2, parent, status);
    PMI_LAUNCH(root_kernel, n, s, parent, n, root, start_of);
    if ((rc = sort_rows(root, root_sorted, rows, rows_sorted, n, n, s)) != PMI_OK) return rc;
    PMI_LAUNCH((replay_kernel<TX, TY>), n, s, frame, x, y, group, lo, hi, n, k, r2, root_sorted, rows_sorted, start_of);
    PMI_LAUNCH(start_flag_kernel, n, s, start_of, n, flag);
    if ((rc = exclusive_scan_u32(flag, rank, N, s)) != PMI_OK) return rc;
    PMI_LAUNCH(label_kernel, n, s, start_of, rank, n, link_group, status);
    int32_t h_status = 0;
    uint32_t h_rank = 0, h_flag = 0;
    PMI_HIP(hipMemcpyAsync(&h_status, status, 4, hipMemcpyDeviceToHost, s));
    PMI_HIP(hipMemcpyAsync(&h_rank, rank + (N - 1), 4, hipMemcpyDeviceToHost, s));
    PMI_HIP(hipMemcpyAsync(&h_flag, flag + (N - 1), 4, hipMemcpyDeviceToHost, s));
    PMI_HIP(hipStreamSynchronize(s));
    if (h_status) {
        set_error("pmi_link_groups_dev: %s", h_status == 1 ? "a union did not settle within its bound"
                                                           : "a row was left without a chain");
        return PMI_ERR_HIP;
    }
    *n_groups = (int64_t)h_rank + h_flag;
    return PMI_OK;
}

template <typename TX, typename TY>
static int nena_typed(const TX *x, const TY *y, const int64_t *frame, const int64_t *group, int32_t n, double d_max,
                      double bin_size, int32_t n_bins, unsigned long long *hist, hipStream_t s)
{
    PMI_HIP(hipMemsetAsync(hist, 0, sizeof(unsigned long long) * n_bins, s));
    const int32_t n_visit = 100 * (int32_t)((double)n / 100.0);     // the reference's 100 * int(N / 100)
    if (n_visit == 0) return PMI_OK;
    int32_t *lo, *hi;
    int rc = carve(SCR_STAGE_A, [&](Arena &ar) { lo = ar.take<int32_t>(n), hi = ar.take<int32_t>(n); });
    if (rc != PMI_OK) return rc;
    if ((rc = frame_index(frame, n, 1, lo, hi, s)) != PMI_OK) return rc;
    const unsigned grid = (unsigned)std::min<int64_t>(blocks(n_visit), 8 * (int64_t)device_cu_count());
    nena_kernel<TX, TY><<<grid, BLOCK, sizeof(uint32_t) * n_bins, s>>>(frame, x, y, group, lo, hi, n, n_visit, d_max,
                                                                      bin_size, n_bins, hist);
    PMI_HIP(hipGetLastError());
    return PMI_OK;
}

}  // namespace link
}  // namespace pmi

using namespace pmi;

extern "C" {

int pmi_link_frame_index_dev(const int64_t *d_frame, int64_t n, int64_t k, int32_t *d_lo, int32_t *d_hi, void *stream)
{
    int rc = rows::check_rows("pmi_link_frame_index_dev", n);
    if (rc) return rc;
    if (n > 0 && (!d_frame || !d_lo || !d_hi)) {
        set_error("pmi_link_frame_index_dev: NULL column");
        return PMI_ERR_ARG;
    }
    return link::frame_index(d_frame, (int32_t)n, k, d_lo, d_hi, (hipStream_t)stream);
}

int pmi_link_groups_dev(const int64_t *d_frame, const void *d_x, int x_type, const void *d_y, int y_type,
                        const int64_t *d_group, int64_t n, double r2, int64_t k, int32_t *d_link_group,
                        int64_t *n_groups, void *stream)
{
    int rc = rows::check_rows("pmi_link_groups_dev", n);
    if (rc || (rc = rows::check_xy("pmi_link_groups_dev", x_type, y_type))) return rc;
    if (!n_groups || (n > 0 && (!d_frame || !d_x || !d_y || !d_group || !d_link_group))) {
        set_error("pmi_link_groups_dev: NULL column");
        return PMI_ERR_ARG;
    }
    *n_groups = 0;
    if (n == 0) return PMI_OK;
    return PMI_XY_DISPATCH(link::groups_typed, d_frame, d_group, (int32_t)n, r2, k, d_link_group, n_groups,
                             (hipStream_t)stream);
}

int pmi_link_combine_dev(const int32_t *d_link_group, int64_t n, int64_t n_groups, const int64_t *d_frame,
                         const pmi_link_column *columns, int n_columns, uint32_t *d_count, int64_t *d_first,
                         int64_t *d_last, int32_t *d_last_row, void *stream)
{
    int rc = rows::check_rows("pmi_link_combine_dev", n);
    if (rc) return rc;
    if (n_groups < 0 || n_groups > INT32_MAX - 1 || n_columns < 0 || n_columns > link::MAX_COLS ||
        (n_columns > 0 && !columns) || (n > 0 && !d_link_group) || (n_groups > 0 && (!d_count || !d_last_row))) {
        set_error("pmi_link_combine_dev: n = %lld, groups = %lld, %d columns", (long long)n, (long long)n_groups, n_columns);
        return PMI_ERR_ARG;
    }
    link::Cols cols;
    cols.n = n_columns;
    for (int i = 0; i < n_columns; ++i) {
        const pmi_link_column &c = columns[i];
        const bool fa = c.type == PMI_LINK_F32 || c.type == PMI_LINK_F64, fw = c.w_type == PMI_LINK_F32 || c.w_type == PMI_LINK_F64;
        const bool ok = !c.out ? false
                        : c.op == PMI_LINK_SUM ? (c.data && c.type >= PMI_LINK_F32 && c.type <= PMI_LINK_U64)
                        : c.op == PMI_LINK_WSUM ? (c.weight && fw)
                        : c.op == PMI_LINK_XWSUM ? (c.data && c.weight && fa && fw) : false;
        if (!ok) {
            set_error("pmi_link_combine_dev: column %d: op %d, types %d / %d", i, c.op, c.type, c.w_type);
            return PMI_ERR_ARG;
        }
        cols.c[i] = link::Col{c.data, c.weight, c.out, c.op, c.type, c.w_type};
    }
    if (n_groups == 0) return PMI_OK;
    hipStream_t s = (hipStream_t)stream;
    const size_t N = std::max<size_t>((size_t)n, 1);
    uint32_t *keys, *keys_sorted;
    int32_t *rows, *rows_sorted;
    rc = rows::carve(SCR_STAGE_A, [&](rows::Arena &ar) {
        keys = ar.take<uint32_t>(N), keys_sorted = ar.take<uint32_t>(N);
        rows = ar.take<int32_t>(N), rows_sorted = ar.take<int32_t>(N);
    });
    if (rc != PMI_OK) return rc;
    if (n > 0) {
        // a link group is an index below n_groups: a negative or larger value becomes n_groups, sorts behind every group
        // and is not summed; the sort then needs only the bits of n_groups
        PMI_LAUNCH(link::group_key_kernel, n, s, d_link_group, (int32_t)n, (int32_t)n_groups, keys);
        PMI_LAUNCH(rows::iota_kernel, n, s, rows, nullptr, (int32_t)n);
        if ((rc = link::sort_rows(keys, keys_sorted, rows, rows_sorted, (int32_t)n, n_groups + 1, s)) != PMI_OK) return rc;
    }
    PMI_LAUNCH(link::combine_kernel, n_groups, s, keys_sorted, rows_sorted, (int32_t)n, (int32_t)n_groups, d_frame, cols,
               d_count, d_first, d_last, d_last_row);
    return PMI_OK;
}

int pmi_nena_hist_dev(const int64_t *d_frame, const void *d_x, int x_type, const void *d_y, int y_type,
                      const int64_t *d_group, int64_t n, double d_max, double bin_size, int n_bins, uint64_t *d_hist,
                      void *stream)
{
    int rc = rows::check_rows("pmi_nena_hist_dev", n);
    if (rc || (rc = rows::check_xy("pmi_nena_hist_dev", x_type, y_type))) return rc;
    if (n_bins < 1 || n_bins > link::MAX_BINS || !(bin_size > 0.0) || !d_hist ||
        (n > 0 && (!d_frame || !d_x || !d_y || !d_group))) {
        set_error("pmi_nena_hist_dev: %d bins of %g (at most %d), or a NULL column", n_bins, bin_size, link::MAX_BINS);
        return PMI_ERR_ARG;
    }
    return PMI_XY_DISPATCH(link::nena_typed, d_frame, d_group, (int32_t)n, d_max, bin_size, (int32_t)n_bins,
                             (unsigned long long *)d_hist, (hipStream_t)stream);
}

}  // extern "C"
