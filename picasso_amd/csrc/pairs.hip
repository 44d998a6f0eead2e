// pairs.hip — local density and the distance histogram over a table binned into square blocks
// (picasso/postprocess.py:37-204 get_index_blocks / _fill_index_blocks, :1543-1579 _local_density,
// :960-999 _distance_histogram), count for count.
//
// Block order.  The host computes x_index / y_index (uint32) as the reference does; a row's key is
// y_index << 32 | x_index, and (key, row) is sorted with the stable radix sort on the bits the largest indices need (the
// x bits, then the y bits): the permutation is np.lexsort([x_index, y_index]).  There is no K x L table of block starts
// and ends: the rows of a block are two bisections of the sorted keys, so memory is O(rows) for any frame and radius.
// This source makes the order; reading it (the key, a run of blocks, the clamped 3 x 3 window) is rows_blocks.h, shared
// with picks.hip and similar.hip.
//
// The fill stall.  The reference fills its table by walking the sorted rows block by block, and stops for good at the
// first sorted row whose index lies outside the K x L grid: every later block starts and ends there.  p = that position
// (n when there is none, one integer min).  Rows at positions >= p are never neighbours (every bisection runs over
// [0, p)), but they do look for neighbours themselves in the density.
//
// Density.  Sorted row i counts the rows j < p (itself included when i < p) of the nine blocks (ki - 1 .. ki + 1,
// li - 1 .. li + 1) with dx2 < r2, dy2 < r2 and dx2 + dy2 < r2.  A block index of -1 is the last block row / column,
// as a negative index is in the reference (it only finds rows when K or L <= 2, and then counts a block twice); an
// index >= K or L is an empty block (the reference reads outside its table there).
//
// Histogram.  Pairs of sorted positions a < b < p with block(b) - block(a) one of (0, 0), (0, 1), (1, 0), (1, 1); the
// offset (1, -1) is never visited by the reference and is missing here too.  dx2 < r2, dy2 < r2,
// d = sqrt(dx2 + dy2) < r_max, bin = floor(d / bin_size) < n_bins.  Up to 8192 bins the counts are kept in LDS and every
// block adds its non-empty bins to the uint64 counters with one integer atomic each; above that every pair is one
// integer atomic on the counters.
//
// Arithmetic is the reference's under numba (as in link.hip): float32 columns give a float32 difference, square, sum
// and square root, compared in float64; d / bin_size is float64; a float32 with a float64 column gives a float64 sum.
// No contraction.  One lane per row: a patch of m rows inside one block costs m^2 tests.  Every loop is bounded by the
// row count.
#include <algorithm>

#include "rows_blocks.h"

#pragma clang fp contract(off)

namespace pmi {
namespace pairs {

using namespace rows;

constexpr int MAX_LDS_BINS = 8192;       // 32 KB of LDS

__device__ __forceinline__ float sqrt_rn(float a) { return __builtin_sqrtf(a); }
__device__ __forceinline__ double sqrt_rn(double a) { return __builtin_sqrt(a); }

// keys, the identity permutation and the largest x / y index (one atomic per block and axis)
__global__ void key_kernel(const uint32_t *__restrict__ x_index, const uint32_t *__restrict__ y_index, int32_t n,
                           uint64_t *__restrict__ keys, int32_t *__restrict__ rows, uint32_t *__restrict__ top)
{
    __shared__ uint32_t m[2];
    if (threadIdx.x < 2) m[threadIdx.x] = 0;
    __syncthreads();
    const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i < n) {
        const uint32_t xi = x_index[i], yi = y_index[i];
        keys[i] = block_key(yi, xi);
        rows[i] = (int32_t)i;
        atomicMax(&m[0], xi);
        atomicMax(&m[1], yi);
    }
    __syncthreads();
    if (threadIdx.x < 2 && m[threadIdx.x]) atomicMax(&top[threadIdx.x], m[threadIdx.x]);
}

// stall[0] = min position whose block lies outside the grid (starts as n)
__global__ void stall_kernel(const uint64_t *__restrict__ keys, int32_t n, int64_t K, int64_t L, int32_t *__restrict__ stall)
{
    __shared__ int32_t m;
    if (threadIdx.x == 0) m = n;
    __syncthreads();
    const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i < n) {
        const uint64_t key = keys[i];
        if ((int64_t)(key >> 32) >= K || (int64_t)(key & 0xffffffffu) >= L) atomicMin(&m, (int32_t)i);
    }
    __syncthreads();
    if (threadIdx.x == 0 && m < n) atomicMin(stall, m);
}

template <typename TX, typename TY>
__global__ void gather_kernel(const TX *__restrict__ x, const TY *__restrict__ y, const int32_t *__restrict__ rows,
                              int32_t n, TX *__restrict__ xs, TY *__restrict__ ys)
{
    const int64_t p = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (p >= n) return;
    const int32_t i = rows[p];
    if (i < 0 || i >= n) { xs[p] = 0; ys[p] = 0; return; }          // not a permutation: nothing is read out of bounds
    xs[p] = x[i];
    ys[p] = y[i];
}

template <typename TX, typename TY>
struct Pair {
    using S = decltype(TX() + TY());
    // dx2 < r2 and dy2 < r2 with the squares in the columns' types and the comparisons in float64
    __device__ static __forceinline__ bool within(TX cx, TY cy, TX xj, TY yj, double r2, S *sum)
    {
        const TX dx = cx - xj;
        const TX dx2 = dx * dx;
        if (!((double)dx2 < r2)) return false;
        const TY dy = cy - yj;
        const TY dy2 = dy * dy;
        if (!((double)dy2 < r2)) return false;
        *sum = (S)dx2 + (S)dy2;
        return true;
    }
};

template <typename TX, typename TY>
__device__ __forceinline__ uint32_t count_run(const TX *__restrict__ xs, const TY *__restrict__ ys, int32_t a, int32_t b,
                                              TX cx, TY cy, double r2)
{
    uint32_t c = 0;
    for (int32_t j = a; j < b; ++j) {
        typename Pair<TX, TY>::S sum;
        if (Pair<TX, TY>::within(cx, cy, xs[j], ys[j], r2, &sum) && (double)sum < r2) ++c;
    }
    return c;
}

template <typename TX, typename TY>
__global__ void density_kernel(Blocks g, const TX *__restrict__ xs, const TY *__restrict__ ys, double r2,
                               uint32_t *__restrict__ density)
{
    const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= g.n) return;
    const uint64_t key = g.keys[i];
    const int64_t ki = (int64_t)(key >> 32), li = (int64_t)(key & 0xffffffffu);
    const TX cx = xs[i];
    const TY cy = ys[i];
    const Window w = window(g, ki, li);                             // its column span; the block rows wrap here
    uint32_t c = 0;
    for (int64_t k = ki - 1; k <= ki + 1; ++k) {
        const int64_t kk = k < 0 ? k + g.K : k;                     // -1 is the last block row
        if (kk < 0 || kk >= g.K || kk > INDEX_MAX) continue;        // past the grid: empty; no index reaches past 2^32
        int32_t a, b;
        if (li == 0 && g.L >= 1 && g.L - 1 <= INDEX_MAX) {          // -1 is the last block column
            block_run(g, kk, g.L - 1, g.L - 1, &a, &b);
            c += count_run(xs, ys, a, b, cx, cy, r2);
        }
        if (w.l0 > w.l1) continue;
        block_run(g, kk, w.l0, w.l1, &a, &b);
        c += count_run(xs, ys, a, b, cx, cy, r2);
    }
    density[i] = c;
}

// LDS = true: bins[] in shared memory, flushed per block; false: straight into hist
template <typename TX, typename TY, bool LDS>
__global__ void hist_kernel(Blocks g, const TX *__restrict__ xs, const TY *__restrict__ ys, double r_max, double r2,
                            double bin_size, int32_t n_bins, unsigned long long *__restrict__ hist)
{
    extern __shared__ uint32_t bins[];
    if (LDS) {
        for (int32_t b = threadIdx.x; b < n_bins; b += BLOCK) bins[b] = 0;
        __syncthreads();
    }
    const int64_t stride = (int64_t)gridDim.x * BLOCK;
    for (int64_t i64 = (int64_t)blockIdx.x * BLOCK + threadIdx.x; i64 < g.p; i64 += stride) {
        const int32_t i = (int32_t)i64;
        const uint64_t key = g.keys[i];
        const int64_t ki = (int64_t)(key >> 32), li = (int64_t)(key & 0xffffffffu);      // inside the grid: i < p
        const int64_t l1 = std::min(li + 1, g.L - 1);
        const TX cx = xs[i];
        const TY cy = ys[i];
        for (int dk = 0; dk < 2; ++dk) {
            int32_t a, b;
            if (dk == 0) {                                          // the rest of the row's own block and the next one
                a = i + 1;
                b = lower_bound(g.keys, a, g.p, block_key(ki, l1) + 1u);
            } else {
                if (ki + 1 >= g.K) break;
                block_run(g, ki + 1, li, l1, &a, &b);
            }
            for (int32_t j = a; j < b; ++j) {
                typename Pair<TX, TY>::S sum;
                if (!Pair<TX, TY>::within(cx, cy, xs[j], ys[j], r2, &sum)) continue;
                const auto d = sqrt_rn(sum);
                if (!((double)d < r_max)) continue;
                const double q = (double)d / bin_size;
                if (!(q >= 0.0 && q < (double)n_bins)) continue;
                if (LDS) atomicAdd(&bins[(int32_t)q], 1u); else atomicAdd(&hist[(int32_t)q], 1ull);
            }
        }
    }
    if (LDS) {
        __syncthreads();
        for (int32_t b = threadIdx.x; b < n_bins; b += BLOCK)
            if (bins[b]) atomicAdd(&hist[b], (unsigned long long)bins[b]);
    }
}

// ---- host ------------------------------------------------------------------------------------------------------
static int check_table(const char *what, int64_t n, int64_t p, int64_t K, int64_t L)
{
    if (n < 0 || n > INT32_MAX - 1 || p < 0 || p > n || K < 0 || L < 0) {
        set_error("%s: %lld rows, %lld visible, grid %lld x %lld (rows are indexed with int32)", what, (long long)n,
                  (long long)p, (long long)K, (long long)L);
        return PMI_ERR_ARG;
    }
    return PMI_OK;
}

static int order(const uint32_t *x_index, const uint32_t *y_index, int32_t n, int64_t K, int64_t L, int32_t *rows_out,
                 uint64_t *keys_out, int64_t *p, hipStream_t s)
{
    const size_t N = (size_t)n;
    uint64_t *keys, *keys_mid;
    int32_t *rows, *rows_mid, *stall;
    uint32_t *top;
    int rc = carve(SCR_STAGE_A, [&](Arena &ar) {
        keys = ar.take<uint64_t>(N), keys_mid = ar.take<uint64_t>(N);
        rows = ar.take<int32_t>(N), rows_mid = ar.take<int32_t>(N);
        top = ar.take<uint32_t>(2), stall = ar.take<int32_t>(1);
    });
    if (rc != PMI_OK) return rc;
    PMI_HIP(hipMemsetAsync(top, 0, 8, s));
    PMI_LAUNCH(key_kernel, n, s, x_index, y_index, n, keys, rows, top);
    uint32_t h_top[2] = {0, 0};
    PMI_HIP(hipMemcpyAsync(h_top, top, 8, hipMemcpyDeviceToHost, s));
    PMI_HIP(hipMemcpyAsync(stall, &n, 4, hipMemcpyHostToDevice, s));
    PMI_HIP(hipStreamSynchronize(s));
    // the x bits, then the y bits
    if ((rc = sort_pairs(keys, keys_mid, rows, rows_mid, N, bits_of(h_top[0]), s)) != PMI_OK) return rc;
    if ((rc = sort_pairs(keys_mid, keys_out, rows_mid, rows_out, N, bits_of(h_top[1]), s, 32)) != PMI_OK) return rc;
    PMI_LAUNCH(stall_kernel, n, s, keys_out, n, K, L, stall);
    int32_t h_stall = n;
    PMI_HIP(hipMemcpyAsync(&h_stall, stall, 4, hipMemcpyDeviceToHost, s));
    PMI_HIP(hipStreamSynchronize(s));
    if (h_stall < 0 || h_stall > n) {
        set_error("pmi_pairs_order_dev: stall position %d of %d rows", h_stall, n);
        return PMI_ERR_HIP;
    }
    *p = h_stall;
    return PMI_OK;
}

template <typename TX, typename TY>
static int sorted_columns(const TX *x, const TY *y, const int32_t *rows, int32_t n, TX **xs, TY **ys, hipStream_t s)
{
    int rc = carve(SCR_STAGE_A, [&](Arena &ar) { *xs = ar.take<TX>(n), *ys = ar.take<TY>(n); });
    if (rc != PMI_OK) return rc;
    PMI_LAUNCH((gather_kernel<TX, TY>), n, s, x, y, rows, n, *xs, *ys);
    return PMI_OK;
}

template <typename TX, typename TY>
static int density_typed(const TX *x, const TY *y, const int32_t *rows, Blocks g, double r2, uint32_t *density,
                         hipStream_t s)
{
    TX *xs;
    TY *ys;
    int rc = sorted_columns(x, y, rows, g.n, &xs, &ys, s);
    if (rc != PMI_OK) return rc;
    PMI_LAUNCH((density_kernel<TX, TY>), g.n, s, g, xs, ys, r2, density);
    PMI_HIP(hipStreamSynchronize(s));
    return PMI_OK;
}

template <typename TX, typename TY>
static int hist_typed(const TX *x, const TY *y, const int32_t *rows, Blocks g, double r_max, double r2, double bin_size,
                      int32_t n_bins, unsigned long long *hist, hipStream_t s)
{
    PMI_HIP(hipMemsetAsync(hist, 0, sizeof(unsigned long long) * (size_t)n_bins, s));
    if (g.p > 0) {
        TX *xs;
        TY *ys;
        int rc = sorted_columns(x, y, rows, g.n, &xs, &ys, s);
        if (rc != PMI_OK) return rc;
        const unsigned grid = (unsigned)std::min<int64_t>(blocks(g.p), 8 * (int64_t)device_cu_count());
        if (n_bins <= MAX_LDS_BINS)
            hist_kernel<TX, TY, true><<<grid, BLOCK, sizeof(uint32_t) * n_bins, s>>>(g, xs, ys, r_max, r2, bin_size,
                                                                                    n_bins, hist);
        else
            hist_kernel<TX, TY, false><<<grid, BLOCK, 0, s>>>(g, xs, ys, r_max, r2, bin_size, n_bins, hist);
        PMI_HIP(hipGetLastError());
    }
    PMI_HIP(hipStreamSynchronize(s));
    return PMI_OK;
}

}  // namespace pairs
}  // namespace pmi

using namespace pmi;

extern "C" {

int pmi_pairs_order_dev(const uint32_t *d_x_index, const uint32_t *d_y_index, int64_t n, int64_t K, int64_t L,
                        int32_t *d_rows, uint64_t *d_keys, int64_t *p, void *stream)
{
    int rc = pairs::check_table("pmi_pairs_order_dev", n, 0, K, L);
    if (rc) return rc;
    if (!p || (n > 0 && (!d_x_index || !d_y_index || !d_rows || !d_keys))) {
        set_error("pmi_pairs_order_dev: NULL column");
        return PMI_ERR_ARG;
    }
    *p = 0;
    if (n == 0) return PMI_OK;
    return pairs::order(d_x_index, d_y_index, (int32_t)n, K, L, d_rows, d_keys, p, (hipStream_t)stream);
}

int pmi_pairs_density_dev(const void *d_x, int x_type, const void *d_y, int y_type, const int32_t *d_rows,
                          const uint64_t *d_keys, int64_t n, int64_t p, int64_t K, int64_t L, double r2,
                          uint32_t *d_density, void *stream)
{
    int rc = pairs::check_table("pmi_pairs_density_dev", n, p, K, L);
    if (rc || (rc = rows::check_xy("pmi_pairs_density_dev", x_type, y_type))) return rc;
    if (n > 0 && (!d_x || !d_y || !d_rows || !d_keys || !d_density)) {
        set_error("pmi_pairs_density_dev: NULL column");
        return PMI_ERR_ARG;
    }
    if (n == 0) return PMI_OK;
    const rows::Blocks g{d_keys, (int32_t)n, (int32_t)p, K, L};
    return PMI_XY_DISPATCH(pairs::density_typed, d_rows, g, r2, d_density, (hipStream_t)stream);
}

int pmi_pairs_distance_hist_dev(const void *d_x, int x_type, const void *d_y, int y_type, const int32_t *d_rows,
                                const uint64_t *d_keys, int64_t n, int64_t p, int64_t K, int64_t L, double r_max,
                                double r2, double bin_size, int64_t n_bins, uint64_t *d_hist, void *stream)
{
    int rc = pairs::check_table("pmi_pairs_distance_hist_dev", n, p, K, L);
    if (rc || (rc = rows::check_xy("pmi_pairs_distance_hist_dev", x_type, y_type))) return rc;
    if (n_bins < 0 || n_bins > INT32_MAX - 1 || !(bin_size > 0.0) || (n_bins > 0 && !d_hist) ||
        (n > 0 && (!d_x || !d_y || !d_rows || !d_keys))) {
        set_error("pmi_pairs_distance_hist_dev: %lld bins of %g, or a NULL column", (long long)n_bins, bin_size);
        return PMI_ERR_ARG;
    }
    if (n_bins == 0) return PMI_OK;
    const rows::Blocks g{d_keys, (int32_t)n, (int32_t)p, K, L};
    return PMI_XY_DISPATCH(pairs::hist_typed, d_rows, g, r_max, r2, bin_size, (int32_t)n_bins,
                           (unsigned long long *)d_hist, (hipStream_t)stream);
}

}  // extern "C"
