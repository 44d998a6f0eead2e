// Host driver of csrc/segment_stats.h (and the distance of csrc/knn_search.h) for tests/test_combine_host.py: what the
// kernels of csrc/combine.hip compute per segment and per group, one after the other on the CPU, through the very
// headers the kernels are compiled from.  Columns arrive gathered into segment order, as the kernels read them.
#include <math.h>
#include <stdint.h>

#include "knn_search.h"
#include "segment_stats.h"

using namespace pmi;

template <typename A>
static void moments(const A *vs, const int32_t *start, int32_t segments, double *mean, double *sd)
{
    for (int32_t s = 0; s < segments; ++s) {
        mean[s] = segstats::series_mean<A>(vs, start[s], start[s + 1]);
        sd[s] = segstats::series_std<A>(vs, start[s], start[s + 1]);
    }
}

template <typename T>
static void averages(const T *xs, const T *ws, const int32_t *start, int32_t segments, double *avg, double *scl)
{
    for (int32_t s = 0; s < segments; ++s) avg[s] = segstats::weighted_average<T>(xs, ws, start[s], start[s + 1], scl + s);
}

template <int D>
static void nearest(const double *pts, const int32_t *first, int32_t groups, double *out, double *out_xy)
{
    for (int32_t g = 0; g < groups; ++g)
        for (int32_t q = first[g]; q < first[g + 1]; ++q) {
            double best = knn::infinity(), best_xy = knn::infinity();
            for (int32_t j = first[g]; j < first[g + 1]; ++j) {
                if (j == q) continue;
                best = segstats::nearest_update(best, knn::sum_of_squares<D>(pts + (int64_t)q * D, pts + (int64_t)j * D));
                if (D == 3)
                    best_xy = segstats::nearest_update(best_xy, knn::sum_of_squares<2>(pts + (int64_t)q * D, pts + (int64_t)j * D));
            }
            out[q] = sqrt(best);
            if (D == 3) out_xy[q] = sqrt(best_xy);
        }
}

// wide: 0 for float32 columns, 1 for float64
extern "C" int combine_host_moments(const void *vs, int wide, const int32_t *start, int32_t segments, double *mean, double *sd)
{
    if (wide) moments((const double *)vs, start, segments, mean, sd);
    else moments((const float *)vs, start, segments, mean, sd);
    return 0;
}

extern "C" int combine_host_averages(const void *xs, const void *ws, int wide, const int32_t *start, int32_t segments,
                                     double *avg, double *scl)
{
    if (wide) averages((const double *)xs, (const double *)ws, start, segments, avg, scl);
    else averages((const float *)xs, (const float *)ws, start, segments, avg, scl);
    return 0;
}

// first[g]: the first sorted row of group g, closed by the number of rows
extern "C" int combine_host_nearest(const double *pts, int dims, const int32_t *first, int32_t groups, double *out,
                                    double *out_xy)
{
    if (dims == 2) nearest<2>(pts, first, groups, out, out_xy);
    else if (dims == 3) nearest<3>(pts, first, groups, out, out_xy);
    else return -1;
    return 0;
}

extern "C" float combine_host_sum32(const float *a, int32_t n)
{
    return segstats::reduce_sum<float>([&](int32_t p) { return a[p]; }, 0, n);
}
