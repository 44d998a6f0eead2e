// cumexp.hip — the kinetic rate of every pick in one call: picasso/lib.py:1305-1327 estimate_kinetic_rate over a CSR of
// samples (the `len` or the `dark` column of the binding events, gathered per pick).
//
// Per segment, as the reference decides it:
//     n <= 2, or n > 2 with max - min == 0     np.nanmean(data)      (n == 0: NaN)
//     otherwise                                 the `t` of fit_cum_exp: the bounded least-squares fit of
//                                               a (1 - exp(-x / t)) + c to (sorted data, 1 .. n) from p0 = (n, mean, min)
// The values arrive as float64 with the kind of the column they came from.  An integer column (`len` and `dark` are
// int32) is exact in float64 and so is every partial sum below 2^53: the order of the summation does not matter, and the
// lanes of a wavefront add their strides and reduce across lanes.  A float32 or float64 column takes NumPy's own sum
// (segment_stats.h, one lane walks the run, mean_kernel) in the column's type.  Where scipy refuses the input (a NaN or an infinity
// in a segment that would be fitted, or a negative minimum: p0 is then outside the bounds) the status says so and the
// outputs are NaN.
//
// Order.  One segmented radix sort (rocPRIM) of the float64 values puts every segment in ascending order.
// Fit.  One wavefront per segment, WAVES wavefronts per workgroup, the grid a function of n_seg alone.  Each pass the
// lanes stride over the samples for the twelve sums of cumexp_core.h, reduce them with a butterfly of cross-lane
// shuffles (every lane ends with the same bits), and run the 3x3 step of cumexp_core.h uniformly.  No LDS, no barrier,
// no atomics, no host round trip inside a fit; the loops are bounded by n and by cumexp::MAX_ITER.
#include <rocprim/device/device_segmented_radix_sort.hpp>

#include "rows_common.h"
#include "segment_stats.h"
#include "cumexp_core.h"

#pragma clang fp contract(off)

namespace pmi {
namespace cumexp {

constexpr int WAVE = 64;
constexpr int WAVES = 4;             // wavefronts, and so segments, per workgroup
enum { KIND_INT = 0, KIND_F32 = 1, KIND_F64 = 2 };

__device__ __forceinline__ double wave_sum(double v)
{
    for (int m = WAVE / 2; m >= 1; m >>= 1) v += __shfl_xor(v, m, WAVE);
    return v;
}
__device__ __forceinline__ double wave_min(double v)
{
    for (int m = WAVE / 2; m >= 1; m >>= 1) { const double o = __shfl_xor(v, m, WAVE); v = o < v ? o : v; }
    return v;
}
__device__ __forceinline__ double wave_max(double v)
{
    for (int m = WAVE / 2; m >= 1; m >>= 1) { const double o = __shfl_xor(v, m, WAVE); v = o > v ? o : v; }
    return v;
}

// the twelve sums at (a, t, c), alike in every lane
__device__ __forceinline__ void sums_at(const double *__restrict__ x, int32_t n, int lane, double a, double t, double c, double *s)
{
#pragma unroll
    for (int k = 0; k < N_SUMS; ++k) s[k] = 0.0;
    for (int32_t i = lane; i < n; i += WAVE) add_sample(s, x[i], (double)(i + 1), a, t, c);
#pragma unroll
    for (int k = 0; k < N_SUMS; ++k) s[k] = wave_sum(s[k]);
}

// 1 when the offsets are not 0 <= offsets[i] <= offsets[i + 1] <= n_values
__global__ void check_offsets_kernel(const int64_t *__restrict__ offsets, int64_t n_seg, int64_t n_values, int32_t *bad)
{
    const int64_t i = (int64_t)blockIdx.x * rows::BLOCK + threadIdx.x;
    if (i >= n_seg) return;
    const int64_t lo = offsets[i], hi = offsets[i + 1];
    if (lo < 0 || hi < lo || hi > n_values) *bad = 1;      // every writer writes the same value
}

__global__ __launch_bounds__(WAVE * WAVES) void fit_kernel(const double *__restrict__ xs, int64_t n_values,
                                                           const int64_t *__restrict__ offsets, int64_t n_seg, int kind,
                                                           double *__restrict__ fit, int32_t *__restrict__ info)
{
    const int lane = threadIdx.x & (WAVE - 1);
    const int64_t seg = (int64_t)blockIdx.x * WAVES + (threadIdx.x / WAVE);
    if (seg >= n_seg) return;                               // whole wavefronts leave: nothing below waits for them
    const double nan = __builtin_nan("");
    double out_a = nan, out_t = nan, out_c = nan, out_cost = nan;
    int32_t out_iters = 0, out_status = CONVERGED;
    const int64_t lo = offsets[seg], hi = offsets[seg + 1];
    if (lo < 0 || hi < lo || hi > n_values || hi - lo > INT32_MAX) {
        out_status = BAD_INPUT;
    } else if (hi > lo) {
        const int32_t n = (int32_t)(hi - lo);
        const double *x = xs + lo;
        // one pass: the sum with NaN as 0, how many values are not NaN, whether all are finite, the extremes
        double sum = 0.0, seen = 0.0, wild = 0.0, mn = __builtin_inf(), mx = -__builtin_inf();
        for (int32_t i = lane; i < n; i += WAVE) {
            const double v = x[i];
            const bool is_nan = v != v;
            sum += is_nan ? 0.0 : v;
            seen += is_nan ? 0.0 : 1.0;
            wild += (is_nan || __builtin_fabs(v) == __builtin_inf()) ? 1.0 : 0.0;
            mn = v < mn ? v : mn;
            mx = v > mx ? v : mx;
        }
        sum = wave_sum(sum), seen = wave_sum(seen), wild = wave_sum(wild), mn = wave_min(mn), mx = wave_max(mx);
        if (n <= 2 || (wild == 0.0 && mx - mn == 0.0)) {
            // np.nanmean.  Integers: exact sums below 2^53, any order.  Floats: NumPy's add.reduce, walked by one lane.
            // (the float kinds are left to mean_kernel: out_iters marks the segment)
            double mean = nan;
            if (kind == KIND_INT) mean = sum / (double)n;
            else if (seen > 0.0) out_iters = -1;
            out_t = mean;
        } else if (wild != 0.0 || mn < 0.0) {
            out_status = BAD_INPUT;
        } else {
            Fit f;
            double s[N_SUMS];
            start(f, (double)n, sum / (double)n, mn, mx);
            sums_at(x, n, lane, f.trial[0], f.trial[1], f.trial[2], s);
            take(f, s);
            f.iters = 1;
            for (int it = 1; it < MAX_ITER; ++it) {
                if (!propose(f)) break;
                sums_at(x, n, lane, f.trial[0], f.trial[1], f.trial[2], s);
                f.iters++;
                judge(f, s);
                if (f.done) break;
            }
            out_a = f.p[0], out_t = f.p[1], out_c = f.p[2], out_cost = f.cost;
            out_iters = f.iters, out_status = f.status;
        }
    }
    if (lane == 0) {
        fit[seg] = out_a, fit[n_seg + seg] = out_t, fit[2 * n_seg + seg] = out_c, fit[3 * n_seg + seg] = out_cost;
        info[seg] = out_iters, info[n_seg + seg] = out_status;
    }
}

// np.nanmean of the marked segments of a float32 / float64 column: NumPy's add.reduce with NaN as 0 in the column's own
// type (segment_stats.h), over the count of the values that are not NaN.  One lane walks one run: a pairwise chain cannot
// be split across lanes and keep its bits.  (Its explicit recursion stack is why this is a kernel of its own.)
__global__ void mean_kernel(const double *__restrict__ xs, const int64_t *__restrict__ offsets, int64_t n_seg, int kind,
                            double *__restrict__ fit, int32_t *__restrict__ info)
{
    const int64_t seg = (int64_t)blockIdx.x * rows::BLOCK + threadIdx.x;
    if (seg >= n_seg || info[seg] != -1) return;
    const int32_t n = (int32_t)(offsets[seg + 1] - offsets[seg]);      // checked by fit_kernel, which marked the segment
    const double *x = xs + offsets[seg];
    double seen = 0.0;
    for (int32_t i = 0; i < n; ++i) seen += x[i] == x[i] ? 1.0 : 0.0;
    double mean;
    if (kind == KIND_F32) {
        const float tot = segstats::reduce_sum<float>([&](int32_t p) { const float v = (float)x[p]; return v == v ? v : 0.0f; }, 0, n);
        mean = (double)(float)((double)tot / seen);
    } else {
        const double tot = segstats::reduce_sum<double>([&](int32_t p) { const double v = x[p]; return v == v ? v : 0.0; }, 0, n);
        mean = tot / seen;
    }
    fit[n_seg + seg] = mean;
    info[seg] = 0;
}

}  // namespace cumexp
}  // namespace pmi

using namespace pmi;

extern "C" {

int pmi_cumexp_fit_dev(const double *d_values, int64_t n_values, const int64_t *d_offsets, int64_t n_seg, int kind,
                       double *d_fit, int32_t *d_info, void *stream)
{
    if (n_values < 0 || n_values > INT32_MAX - 1 || n_seg < 0 || n_seg > INT32_MAX - 1 || kind < cumexp::KIND_INT ||
        kind > cumexp::KIND_F64) {
        set_error("pmi_cumexp_fit_dev: %lld values in %lld segments (both below 2^31 - 1), kind %d (0 .. 2)",
                  (long long)n_values, (long long)n_seg, kind);
        return PMI_ERR_ARG;
    }
    if (n_seg == 0) return PMI_OK;
    if (!d_offsets || !d_fit || !d_info || (n_values > 0 && !d_values)) {
        set_error("pmi_cumexp_fit_dev: a NULL array");
        return PMI_ERR_ARG;
    }
    hipStream_t s = (hipStream_t)stream;
    double *sorted;
    int32_t *bad;
    int rc = rows::carve(SCR_STAGE_A, [&](rows::Arena &ar) {
        sorted = ar.take<double>((size_t)(n_values > 0 ? n_values : 1));
        bad = ar.take<int32_t>(1);
    });
    if (rc != PMI_OK) return rc;
    // the sort reads the segments the offsets name: they are checked before it runs
    PMI_HIP(hipMemsetAsync(bad, 0, sizeof(int32_t), s));
    PMI_LAUNCH(cumexp::check_offsets_kernel, n_seg, s, d_offsets, n_seg, n_values, bad);
    int32_t h_bad = 0;
    PMI_HIP(hipMemcpyAsync(&h_bad, bad, sizeof(int32_t), hipMemcpyDeviceToHost, s));
    PMI_HIP(hipStreamSynchronize(s));
    if (h_bad) {
        set_error("pmi_cumexp_fit_dev: the offsets must ascend from 0 to at most %lld", (long long)n_values);
        return PMI_ERR_ARG;
    }
    if (n_values > 0) {
        rc = rows::two_pass([&](void *tmp, size_t &bytes) {
            return rocprim::segmented_radix_sort_keys(tmp, bytes, d_values, sorted, (unsigned)n_values, (unsigned)n_seg, d_offsets,
                                                      d_offsets + 1, 0, 64, s);
        });
        if (rc != PMI_OK) return rc;
    }
    const unsigned grid = (unsigned)((n_seg + cumexp::WAVES - 1) / cumexp::WAVES);
    cumexp::fit_kernel<<<grid, cumexp::WAVE * cumexp::WAVES, 0, s>>>(sorted, n_values, d_offsets, n_seg, kind, d_fit, d_info);
    PMI_HIP(hipGetLastError());
    if (kind != cumexp::KIND_INT) PMI_LAUNCH(cumexp::mean_kernel, n_seg, s, sorted, d_offsets, n_seg, kind, d_fit, d_info);
    PMI_HIP(hipStreamSynchronize(s));
    return PMI_OK;
}

int pmi_cumexp_fit(const double *values, int64_t n_values, const int64_t *offsets, int64_t n_seg, int kind, double *fit,
                   int32_t *info)
{
    if (pmi_device_count() < 1) { set_error("no HIP device"); return PMI_ERR_NODEVICE; }
    if (n_values < 0 || n_seg < 0 || n_values > INT32_MAX - 1 || n_seg > INT32_MAX - 1) {
        set_error("pmi_cumexp_fit: %lld values in %lld segments (both below 2^31 - 1)", (long long)n_values, (long long)n_seg);
        return PMI_ERR_ARG;
    }
    if (n_seg == 0) return PMI_OK;
    if (!offsets || !fit || !info || (n_values > 0 && !values)) { set_error("pmi_cumexp_fit: a NULL array"); return PMI_ERR_ARG; }
    double *d_values = nullptr, *d_fit = nullptr;
    int64_t *d_offsets = nullptr;
    int32_t *d_info = nullptr;
    Staged st(SCR_STAGE_C);          // the _dev form carves SCR_STAGE_A and sorts through SCR_STAGE_B
    st.add(d_values, n_values, values), st.add(d_offsets, (size_t)n_seg + 1, offsets);
    st.add(d_fit, (size_t)n_seg * 4, nullptr, fit), st.add(d_info, (size_t)n_seg * 2, nullptr, info);
    int rc;
    if ((rc = st.place()) != PMI_OK) return rc;
    if ((rc = pmi_cumexp_fit_dev(d_values, n_values, d_offsets, n_seg, kind, d_fit, d_info, nullptr)) != PMI_OK) return rc;
    return st.fetch();
}

}  // extern "C"
