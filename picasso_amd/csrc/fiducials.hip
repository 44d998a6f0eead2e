// fiducials.hip — the drift of picked fiducials (picasso/postprocess.py:3062-3156 undrift_from_picked,
// _undrift_from_picked_coordinate), in the bits NumPy 2 gives the reference.
//
// The call gets the member rows of P picks as a CSR (offsets, and frame and up to three coordinate columns gathered
// into pick order) and returns (Frames, columns) float64.  Per coordinate, of type T (float32 or float64), on one stream:
//
//   mean_kernel      one workgroup per pick: np.mean = add.reduce(c) / T(n) in T, the sum by group_reduce.h
//   (winner table)   once per call: atomicMax of the row position into win[P x Frames], so that on a repeated frame the
//                    row latest in the given order is the one written (NumPy's fancy assignment), whatever the launch
//                    order; a frame f < 0 is f + Frames, one outside [0, Frames) sets status bit 0
//   scatter_kernel   D[p, frame] = float64(c - mean_p), subtracted in T, by the winning rows; D starts as NaN
//   first_kernel     one lane per frame, loads coalesced along f: np.nanmean(D, 0) = the sum of (D or 0) over p in pick
//                    order, starting from row 0, over the count of values that are not NaN; 0 / 0 is NaN
//   msd_kernel       one workgroup per pick: np.nanmean((D - m0) ** 2, 1), the add.reduce over the Frames-long row by
//                    group_reduce.h with NaN as 0, over the count; w = 1 / msd
//   average_kernel   one lane per frame: np.ma.average(masked D, 0, weights=w): num = sum of (D * w or 0), den = sum of
//                    (w * 1.0 or 0), both over p in pick order from row 0 with 0 for a NaN of D; masked (NaN) where no
//                    pick has the frame or where |num| * DBL_MIN >= |den| (the masked division's domain), else num / den
//   interp_kernel    a NaN frame takes np.interp over the frames that are not NaN: their nearest on either side come
//                    from a max-scan and a reversed min-scan; the value of the first / last one outside them,
//                    slope * (f - f_lo) + y_lo with slope = (y_hi - y_lo) / (f_hi - f_lo) between.  No frame with a
//                    value sets status bit 1 (np.interp raises ValueError).
//
// The presence of a value is D == D throughout, so a NaN coordinate is a hole like an uncovered frame, as np.isnan
// makes it in the reference.  np.interp's second formula for a non-finite product is not taken: with infinite
// coordinates the interpolated frames are not pinned.  P * Frames <= pmi_fiducials_max_cells(): D and the winner table
// are the call's memory, 12 bytes per cell, and D is reused by the coordinates.  No contraction.
#include <float.h>

#include <algorithm>

#include "rows_common.h"
#include "group_reduce.h"

#pragma clang fp contract(off)

namespace pmi {
namespace fiducials {

using namespace rows;

constexpr int64_t MAX_CELLS = 1LL << 28;
constexpr int MAX_COLUMNS = 3;
static_assert(BLOCK == groupreduce::WAVES * 64, "group_reduce.h is written for the row kernels' workgroup");

enum { BAD_FRAME = 1, NO_FRAME = 2 };

struct Picks {
    const int64_t *offsets;
    int32_t P, M, F;
};

// the run of pick p, inside [0, M] whatever the offsets hold
__device__ __forceinline__ void run_of(const Picks &g, int32_t p, int32_t *a, int32_t *b)
{
    const int64_t lo = g.offsets[p], hi = g.offsets[p + 1];
    *a = (int32_t)std::min<int64_t>(std::max<int64_t>(lo, 0), g.M);
    *b = (int32_t)std::min<int64_t>(std::max<int64_t>(hi, *a), g.M);
}

// the pick of row j: the last p with offsets[p] <= j (empty picks share an offset with the next one)
__device__ __forceinline__ int32_t pick_of(const Picks &g, int32_t j)
{
    int32_t lo = 0, hi = g.P;                 // offsets[lo] <= j < offsets[hi] when the offsets are a CSR's
    for (int it = 0; it < 40 && hi - lo > 1; ++it) {
        const int32_t mid = lo + ((hi - lo) >> 1);
        if (g.offsets[mid] <= (int64_t)j) lo = mid; else hi = mid;
    }
    return lo;
}

// the cell of row j in the P x Frames matrix, or -1 for a frame outside it
__device__ __forceinline__ int64_t cell_of_row(const Picks &g, const int64_t *__restrict__ frame, int32_t j)
{
    int64_t f = frame[j];
    if (f < 0) f += g.F;
    if (f < 0 || f >= g.F) return -1;
    return (int64_t)pick_of(g, j) * g.F + f;
}

__global__ void winner_kernel(Picks g, const int64_t *__restrict__ frame, int32_t *__restrict__ win, int32_t *status)
{
    const int64_t j = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (j >= g.M) return;
    const int64_t cell = cell_of_row(g, frame, (int32_t)j);
    if (cell < 0) atomicOr(status, (int32_t)BAD_FRAME);
    else atomicMax(win + cell, (int32_t)j);
}

template <typename T>
__global__ void mean_kernel(Picks g, const T *__restrict__ c, T *__restrict__ mean)
{
    __shared__ groupreduce::Shared<T> sh;
    const int32_t p = blockIdx.x;
    int32_t a, b;
    run_of(g, p, &a, &b);
    const T sum = groupreduce::reduce_sum<T>([&](int32_t i) { return c[i]; }, a, b, sh);
    if (threadIdx.x == 0) mean[p] = sum / (T)(b - a);
}

template <typename T>
__global__ void scatter_kernel(Picks g, const int64_t *__restrict__ frame, const T *__restrict__ c,
                               const T *__restrict__ mean, const int32_t *__restrict__ win, double *__restrict__ D)
{
    const int64_t j = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (j >= g.M) return;
    const int64_t cell = cell_of_row(g, frame, (int32_t)j);
    if (cell < 0 || win[cell] != (int32_t)j) return;
    const T d = c[j] - mean[cell / g.F];
    D[cell] = (double)d;
}

__global__ void first_kernel(Picks g, const double *__restrict__ D, double *__restrict__ m0)
{
    const int64_t f = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (f >= g.F) return;
    double s = 0.0;
    int64_t count = 0;
    for (int32_t p = 0; p < g.P; ++p) {
        const double d = D[(int64_t)p * g.F + f];
        const bool has = d == d;
        const double v = has ? d : 0.0;
        s = p == 0 ? v : s + v;
        count += has ? 1 : 0;
    }
    m0[f] = s / (double)count;
}

__global__ void msd_kernel(Picks g, const double *__restrict__ D, const double *__restrict__ m0, double *__restrict__ w)
{
    __shared__ groupreduce::Shared<double> sh;
    __shared__ unsigned int n_values;
    const int32_t p = blockIdx.x;
    const double *__restrict__ row = D + (int64_t)p * g.F;
    if (threadIdx.x == 0) n_values = 0;
    __syncthreads();
    unsigned int mine = 0;
    const double sum = groupreduce::reduce_sum<double>([&](int32_t f) {
        const double d = row[f] - m0[f];
        const double sq = d * d;
        const bool has = sq == sq;
        mine += has ? 1u : 0u;
        return has ? sq : 0.0;
    }, 0, g.F, sh);
    atomicAdd(&n_values, mine);
    __syncthreads();
    if (threadIdx.x == 0) {
        const double msd = sum / (double)n_values;
        w[p] = 1.0 / msd;
    }
}

__global__ void average_kernel(Picks g, const double *__restrict__ D, const double *__restrict__ w,
                               double *__restrict__ y, int32_t *__restrict__ before, int32_t *__restrict__ after)
{
    const int64_t f = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (f >= g.F) return;
    double num = 0.0, den = 0.0;
    bool any = false;
    for (int32_t p = 0; p < g.P; ++p) {
        const double d = D[(int64_t)p * g.F + f], wp = w[p];
        const bool has = d == d;
        const double a = has ? d * wp : 0.0, b = has ? wp * 1.0 : 0.0;
        num = p == 0 ? a : num + a;
        den = p == 0 ? b : den + b;
        any |= has;
    }
    double v = num / den;
    if (!any || fabs(num) * DBL_MIN >= fabs(den)) v = segstats::quiet_nan<double>();
    const bool has = v == v;
    y[f] = v;
    before[f] = has ? (int32_t)f : -1;                       // a max-scan gives the last frame with a value at or before f
    after[g.F - 1 - f] = has ? (int32_t)f : INT32_MAX;       // a min-scan of the reversed frames, the first at or after f
}

__global__ void interp_kernel(int32_t F, const double *__restrict__ y, const int32_t *__restrict__ before,
                              const int32_t *__restrict__ after, double *__restrict__ out, int n_columns, int column,
                              int32_t *status)
{
    const int64_t f = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (f >= F) return;
    const int32_t lo = before[f], hi = after[F - 1 - f];
    double v = y[f];
    if (lo < 0 && hi >= F) {                                  // no frame has a value
        if (f == 0) atomicOr(status, (int32_t)NO_FRAME);
    } else if (lo < 0) {
        v = y[hi];
    } else if (hi >= F) {
        v = y[lo];
    } else if (lo != (int32_t)f) {
        const double slope = (y[hi] - y[lo]) / ((double)hi - (double)lo);
        v = slope * ((double)f - (double)lo) + y[lo];
    }
    out[f * n_columns + column] = v;
}

// one run per workgroup: the sum alone, for the tests of group_reduce.h
template <typename T>
__global__ void reduce_kernel(Picks g, const T *__restrict__ c, T *__restrict__ out)
{
    __shared__ groupreduce::Shared<T> sh;
    int32_t a, b;
    run_of(g, blockIdx.x, &a, &b);
    const T sum = groupreduce::reduce_sum<T>([&](int32_t i) { return c[i]; }, a, b, sh);
    if (threadIdx.x == 0) out[blockIdx.x] = sum;
}

// ---- host ------------------------------------------------------------------------------------------------------
struct Work {
    int32_t *win, *before, *after, *before_scan, *after_scan, *status;
    double *D, *m0, *w, *y;
    void *mean;
};

template <typename Op>
static int scan_i32(const int32_t *in, int32_t *out, size_t n, Op op, hipStream_t s)
{
    return two_pass([&](void *tmp, size_t &bytes) { return rocprim::inclusive_scan(tmp, bytes, in, out, n, op, s); });
}

template <typename T>
static int column_typed(const Picks &g, const int64_t *frame, const T *c, const Work &k, double *out, int n_columns,
                        int column, hipStream_t s)
{
    const size_t cells = (size_t)g.P * (size_t)g.F;
    T *mean = (T *)k.mean;
    mean_kernel<T><<<(unsigned)g.P, BLOCK, 0, s>>>(g, c, mean);
    PMI_HIP(hipGetLastError());
    PMI_HIP(hipMemsetAsync(k.D, 0xff, sizeof(double) * cells, s));                 // all bits set is a NaN
    if (g.M > 0) PMI_LAUNCH((scatter_kernel<T>), g.M, s, g, frame, c, mean, k.win, k.D);
    PMI_LAUNCH(first_kernel, g.F, s, g, k.D, k.m0);
    msd_kernel<<<(unsigned)g.P, BLOCK, 0, s>>>(g, k.D, k.m0, k.w);
    PMI_HIP(hipGetLastError());
    PMI_LAUNCH(average_kernel, g.F, s, g, k.D, k.w, k.y, k.before, k.after);
    int rc = scan_i32(k.before, k.before_scan, (size_t)g.F, rocprim::maximum<int32_t>(), s);
    if (rc != PMI_OK || (rc = scan_i32(k.after, k.after_scan, (size_t)g.F, rocprim::minimum<int32_t>(), s)) != PMI_OK) return rc;
    PMI_LAUNCH(interp_kernel, g.F, s, g.F, k.y, k.before_scan, k.after_scan, out, n_columns, column, k.status);
    return PMI_OK;
}

static int check_call(const char *what, int64_t P, int64_t M, const void *d_offsets)
{
    if (P < 0 || P > INT32_MAX - 1 || M < 0 || M > INT32_MAX - 1 || !d_offsets) {
        set_error("%s: %lld picks, %lld rows (both are indexed with int32), or no offsets", what, (long long)P, (long long)M);
        return PMI_ERR_ARG;
    }
    return PMI_OK;
}

}  // namespace fiducials
}  // namespace pmi

using namespace pmi;

extern "C" {

int64_t pmi_fiducials_max_cells(void) { return fiducials::MAX_CELLS; }

int pmi_fiducials_drift_dev(const int64_t *d_offsets, int64_t n_picks, const int64_t *d_frame, int64_t n_rows,
                            const void *const *d_columns, const int *types, int n_columns, int64_t n_frames,
                            double *d_out, int *status, void *stream)
{
    using namespace fiducials;
    const char *what = "pmi_fiducials_drift_dev";
    int rc = check_call(what, n_picks, n_rows, d_offsets);
    if (rc) return rc;
    if (n_picks < 1 || n_frames < 1 || n_frames > INT32_MAX - 1 || n_picks * n_frames > MAX_CELLS) {
        set_error("%s: %lld picks x %lld frames (at least one of each, at most %lld cells)", what, (long long)n_picks,
                  (long long)n_frames, (long long)MAX_CELLS);
        return PMI_ERR_ARG;
    }
    if (n_columns < 1 || n_columns > MAX_COLUMNS || !d_columns || !types || !d_out || !status || (n_rows > 0 && !d_frame)) {
        set_error("%s: %d columns (1 .. %d), or a NULL argument", what, n_columns, MAX_COLUMNS);
        return PMI_ERR_ARG;
    }
    for (int c = 0; c < n_columns; ++c)
        if ((types[c] != PMI_LINK_F32 && types[c] != PMI_LINK_F64) || (n_rows > 0 && !d_columns[c])) {
            set_error("%s: column %d must be float32 or float64 (code %d) and not NULL", what, c, types[c]);
            return PMI_ERR_ARG;
        }
    hipStream_t s = (hipStream_t)stream;
    const Picks g{d_offsets, (int32_t)n_picks, (int32_t)n_rows, (int32_t)n_frames};
    const size_t cells = (size_t)n_picks * (size_t)n_frames, F = (size_t)n_frames, P = (size_t)n_picks;
    Work k;
    rc = carve(SCR_STAGE_A, [&](Arena &ar) {
        k.D = ar.take<double>(cells);
        k.win = ar.take<int32_t>(cells);
        k.m0 = ar.take<double>(F);
        k.y = ar.take<double>(F);
        k.w = ar.take<double>(P);
        k.mean = ar.take<double>(P);
        k.before = ar.take<int32_t>(F);
        k.after = ar.take<int32_t>(F);
        k.before_scan = ar.take<int32_t>(F);
        k.after_scan = ar.take<int32_t>(F);
        k.status = ar.take<int32_t>(1);
    });
    if (rc != PMI_OK) return rc;
    PMI_HIP(hipMemsetAsync(k.status, 0, sizeof(int32_t), s));
    PMI_HIP(hipMemsetAsync(k.win, 0xff, sizeof(int32_t) * cells, s));              // -1: no row
    if (n_rows > 0) PMI_LAUNCH(winner_kernel, n_rows, s, g, d_frame, k.win, k.status);
    for (int c = 0; c < n_columns; ++c) {
        if (types[c] == PMI_LINK_F32) rc = column_typed<float>(g, d_frame, (const float *)d_columns[c], k, d_out, n_columns, c, s);
        else rc = column_typed<double>(g, d_frame, (const double *)d_columns[c], k, d_out, n_columns, c, s);
        if (rc != PMI_OK) return rc;
    }
    int32_t h_status = 0;
    PMI_HIP(hipMemcpyAsync(&h_status, k.status, sizeof(int32_t), hipMemcpyDeviceToHost, s));
    PMI_HIP(hipStreamSynchronize(s));
    *status = h_status;
    return PMI_OK;
}

int pmi_fiducials_reduce_dev(const void *d_values, int type, int64_t n_values, const int64_t *d_offsets, int64_t n_runs,
                             void *d_out, void *stream)
{
    using namespace fiducials;
    const char *what = "pmi_fiducials_reduce_dev";
    int rc = check_call(what, n_runs, n_values, d_offsets);
    if (rc) return rc;
    if ((type != PMI_LINK_F32 && type != PMI_LINK_F64) || (n_values > 0 && !d_values) || (n_runs > 0 && !d_out)) {
        set_error("%s: values must be float32 or float64 (code %d) and not NULL", what, type);
        return PMI_ERR_ARG;
    }
    if (n_runs == 0) return PMI_OK;
    hipStream_t s = (hipStream_t)stream;
    const Picks g{d_offsets, (int32_t)n_runs, (int32_t)n_values, 0};
    if (type == PMI_LINK_F32) reduce_kernel<float><<<(unsigned)n_runs, BLOCK, 0, s>>>(g, (const float *)d_values, (float *)d_out);
    else reduce_kernel<double><<<(unsigned)n_runs, BLOCK, 0, s>>>(g, (const double *)d_values, (double *)d_out);
    PMI_HIP(hipGetLastError());
    PMI_HIP(hipStreamSynchronize(s));
    return PMI_OK;
}

}  // extern "C"
