// Host build of csrc/average_core.h for tests/test_average_host.py: the same rotate / bin / gather / ordered best the
// kernels of csrc/average.hip are compiled from, looped the plain way.  Built with -ffp-contract=off.
#include <vector>

#include "average_core.h"

using namespace pmi::average;

extern "C" {

// int32 image (n x n, zeroed by the caller) of the float32 table; returns the rows whose pixel fell outside
int average_host_image(const float *x, const float *y, int rows, double t_min, double t_max, double ov, int n, int sub_f32,
                       int mul_f32, int32_t *image)
{
    const Geom g{t_min, t_max, ov, n, sub_f32, mul_f32};
    int dropped = 0;
    for (int i = 0; i < rows; ++i) {
        if (!in_view((double)x[i], (double)y[i], g)) continue;
        const int32_t px = pixel32(x[i], g), py = pixel32(y[i], g);
        if ((uint32_t)px >= (uint32_t)n || (uint32_t)py >= (uint32_t)n) ++dropped;
        else ++image[py * n + px];
    }
    return dropped;
}

// one group: choice[3] = (value, angle, flat) over all angles and shifts, x1 / y1 its aligned rows
void average_host_align(const float *x, const float *y, int rows, double t_min, double t_max, double ov, int n,
                        const double *cosv, const double *sinv, int n_angles, const int32_t *image, int32_t *choice,
                        float *x1, float *y1)
{
    const Geom g{t_min, t_max, ov, n, 0, 0};
    std::vector<uint32_t> list(rows > 0 ? rows : 1);
    Best best = none();
    for (int a = 0; a < n_angles; ++a) {
        int count = 0;
        for (int i = 0; i < rows; ++i) {
            uint32_t packed;
            if (rotate_bin(x[i], y[i], cosv[a], sinv[a], g, &packed) == 1) list[count++] = packed;
        }
        for (int f = 0; f < n * n; ++f) {
            const int32_t v = gather(image, list.data(), count, n, unshift(f / n, n), unshift(f % n, n));
            if (better(v, a, f, best)) best = Best{v, a, f};
        }
    }
    choice[0] = best.value, choice[1] = best.angle, choice[2] = best.flat;
    double cs = 1.0, sn = 0.0, dx = 0.0, dy = 0.0;
    if (best.angle >= 0) {
        cs = cosv[best.angle], sn = sinv[best.angle];
        dy = shift_of(best.flat / n, g), dx = shift_of(best.flat % n, g);
    }
    for (int i = 0; i < rows; ++i) transform(x[i], y[i], cs, sn, dx, dy, x1 + i, y1 + i);
}

}  // extern "C"
