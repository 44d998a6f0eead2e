// segment_stats.h — the statistics of one run [a, b) of a gathered, segment-ordered column, in NumPy's and pandas'
// arithmetic (kinetics.hip, combine.hip), written so that the host compiler takes it too (tests/test_combine_host.py
// builds it into a small shared object, tests/combine_host_driver.cpp).
//
// Sums.  Every sum is NumPy's add.reduce of a contiguous array: an accumulator that starts at 0 and takes the pairwise
// sum of each 8192-element chunk in order; pairwise is a serial loop below 8 elements, eight strided accumulators up to
// 128, and a split at n / 2 rounded down to a multiple of 8 above.  The recursion runs on an explicit stack.
//
// pandas' Series.mean() / Series.std() (nanops.nanmean / nanvar): NaN counts as 0 and is counted out; the mean is the
// sum in the column's own floating type (integers as float64) over the count in that type; std (ddof 1) takes avg = the
// float64 sum over the count, sums (avg - v)^2 in float64, divides by count - 1, and takes the root in float32 for a
// float32 column and in float64 otherwise.
//
// np.average(x, weights=w) of two columns of one floating type T: np.multiply(x, w) rounded to T, the add.reduce of
// the products in T, the add.reduce of the weights in T, one division in T.  Nothing is skipped: a NaN gives NaN.
//
// One caller walks one run: neither a pairwise nor a chunked chain can be split across lanes and keep its bits.
// C++ float and double, no contraction.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define SEG_HD __host__ __device__ inline
#define SEG_HD_FORCE __host__ __device__ __forceinline__
#else
#define SEG_HD inline
#define SEG_HD_FORCE inline
#endif

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace pmi {
namespace segstats {

constexpr int32_t CHUNK = 8192;      // NumPy's buffer size, in elements
constexpr int DEPTH = 16;            // a chunk halves at most 7 times before it is a 128-element block

template <typename T> SEG_HD_FORCE T quiet_nan();
template <> SEG_HD_FORCE float quiet_nan<float>() { return __builtin_nanf(""); }
template <> SEG_HD_FORCE double quiet_nan<double>() { return __builtin_nan(""); }

// NumPy's pairwise sum of at most 128 terms: term(p) for p in [lo, lo + m)
template <typename S, typename F>
SEG_HD_FORCE S block_sum(F term, int32_t lo, int32_t m)
{
    if (m < 8) {
        S res = 0;
        for (int32_t i = 0; i < m; ++i) res += term(lo + i);
        return res;
    }
    S r[8];
    for (int k = 0; k < 8; ++k) r[k] = term(lo + k);
    int32_t i = 8;
    for (; i < m - (m % 8); i += 8)
        for (int k = 0; k < 8; ++k) r[k] += term(lo + i + k);
    S res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
    for (; i < m; ++i) res += term(lo + i);
    return res;
}

// ... of one chunk: the recursion on an explicit stack.  A frame waits for its left half, then for its right half.
template <typename S, typename F>
SEG_HD S pairwise_sum(F term, int32_t lo, int32_t m)
{
    int32_t f_lo[DEPTH], f_m[DEPTH];
    S f_left[DEPTH];
    int f_state[DEPTH];
    int sp = 0;
    f_lo[0] = lo, f_m[0] = m, f_state[0] = 0, f_left[0] = 0;
    sp = 1;
    S ret = 0;
    // every frame is visited three times and there are fewer than m / 32 + 2 of them
    for (int32_t it = 0; it < 3 * (m / 32 + 2) && sp > 0; ++it) {
        const int t = sp - 1;
        const int32_t cm = f_m[t], clo = f_lo[t];
        int32_t half = cm / 2;
        half -= half % 8;
        if (f_state[t] == 0) {
            if (cm <= 128) {
                ret = block_sum<S>(term, clo, cm);
                --sp;
            } else if (sp == DEPTH) {            // cannot happen within a chunk; it would sum serially, inside the run
                ret = 0;
                for (int32_t i = 0; i < cm; ++i) ret += term(clo + i);
                --sp;
            } else {
                f_state[t] = 1;
                f_lo[sp] = clo, f_m[sp] = half, f_state[sp] = 0, f_left[sp] = 0;
                ++sp;
            }
        } else if (f_state[t] == 1) {
            f_left[t] = ret;
            f_state[t] = 2;
            f_lo[sp] = clo + half, f_m[sp] = cm - half, f_state[sp] = 0, f_left[sp] = 0;      // sp < DEPTH: checked in state 0
            ++sp;
        } else {
            ret = f_left[t] + ret;
            --sp;
        }
    }
    return ret;
}

// NumPy's add.reduce over [a, b)
template <typename S, typename F>
SEG_HD S reduce_sum(F term, int32_t a, int32_t b)
{
    S acc = 0;
    for (int32_t lo = a; lo < b; lo += CHUNK) acc += pairwise_sum<S>(term, lo, b - lo < CHUNK ? b - lo : CHUNK);
    return acc;
}

// the values of the run that are not NaN
template <typename A>
SEG_HD_FORCE int64_t count_values(const A *vs, int32_t a, int32_t b)
{
    int64_t nobs = 0;
    for (int32_t p = a; p < b; ++p) nobs += vs[p] == vs[p] ? 1 : 0;
    return nobs;
}

// pandas' Series.mean() of vs[a .. b), as float64; A is the summing type (float for a float32 column, double otherwise)
template <typename A>
SEG_HD double series_mean(const A *vs, int32_t a, int32_t b)
{
    const int64_t nobs = count_values(vs, a, b);
    const A count = (A)nobs;
    const A sum = reduce_sum<A>([&](int32_t p) { const A v = vs[p]; return v == v ? v : (A)0; }, a, b);
    return nobs > 0 ? (double)(sum / count) : quiet_nan<double>();
}

// pandas' Series.std() (ddof 1) of vs[a .. b), as float64
template <typename A>
SEG_HD double series_std(const A *vs, int32_t a, int32_t b)
{
    const A count = (A)count_values(vs, a, b);
    double out = quiet_nan<double>();
    if (count > (A)1) {
        const double total = reduce_sum<double>([&](int32_t p) { const A v = vs[p]; return v == v ? (double)v : 0.0; }, a, b);
        const double avg = total / (double)count;
        const double sq = reduce_sum<double>([&](int32_t p) {
            const A v = vs[p];
            const double d = avg - (double)v;
            return v == v ? d * d : 0.0;
        }, a, b);
        const double var = sq / (double)(count - (A)1);
        if (sizeof(A) == 4) out = (double)__builtin_sqrtf((float)var);
        else out = __builtin_sqrt(var);
    }
    return out;
}

// np.average(xs[a .. b), weights=ws[a .. b)) in T, as float64; *scl receives the sum of the weights (0 for an empty run)
template <typename T>
SEG_HD double weighted_average(const T *xs, const T *ws, int32_t a, int32_t b, double *scl)
{
    const T weights = reduce_sum<T>([&](int32_t p) { return ws[p]; }, a, b);
    const T products = reduce_sum<T>([&](int32_t p) { const T v = xs[p] * ws[p]; return v; }, a, b);
    *scl = (double)weights;
    return (double)(products / weights);
}

// np.amin over the squares seen so far: a NaN stays, whatever comes after it
SEG_HD_FORCE double nearest_update(double best, double s)
{
    return (s < best || s != s) ? s : best;
}

}  // namespace segstats
}  // namespace pmi
