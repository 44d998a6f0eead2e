// average_core.h — what one candidate angle of picasso.average costs for one group (picasso/average.py:49-118
// align_group_core, picasso/render.py:739-773 render_hist_numba), shared by average.hip and the host-side check of it
// (tests/average_host_driver.cpp): rotate, bin, gather, ordered best.  Plain C++: it compiles for the host.
//
// The identity.  Both images are histograms, so their circular cross-correlation is an integer:
//     ifft2(fft2(image) * conj(fft2(avg)))[s] = sum_q image[q] * avg[(q - s) mod n]
//                                             = sum over the group's locs in view of avg[(pixel(loc) - s) mod n],
// per axis.  The reference takes argmax of np.fft.fftshift of it.  fftshift rolls by n / 2 (integer division), so
// entry i of the shifted array is entry (i - n / 2) mod n of the unshifted one, for odd and even n alike
// (n = 4: [2 3 0 1], n = 5: [3 4 0 1 2]); `unshift` is that map.
//
// The order.  np.argmax takes the first flat index (row-major) of the shifted array; the loop over the angles keeps a
// candidate only when it is strictly larger than what it has, starting from 0.  So the choice is the largest value,
// then the lowest angle, then the lowest flat index, and nothing is chosen while every value is 0 (angle -1, flat -1).
//
// The types.  cos(a) and sin(a) are float64, x0 and y0 float32: the products are float64, each rounded on its own
// (no contraction), as are the difference and the sum; the view test is strict; the pixel is oversampling * (v - t_min)
// in float64, truncated.  The average image takes its pixels from float32 coordinates, where NumPy subtracts and
// multiplies in float32 or float64 as the types of t_min and the oversampling decide: two flags say which.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define PMI_AVG_FN __host__ __device__ __forceinline__
#else
#define PMI_AVG_FN static inline
#endif
#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace pmi {
namespace average {

struct Geom {
    double t_min, t_max, ov;      // the view and the oversampling, as float64
    int32_t n;                    // pixels per axis
    int32_t sub_f32, mul_f32;     // average image only: v - t_min, and the product with ov, are float32 operations
};

struct Best {
    int32_t value, angle, flat;   // flat: row * n + column of the fftshifted correlation
};

PMI_AVG_FN Best none() { return Best{0, -1, -1}; }

// (value, angle, flat) comes before b in the order above; never true for a value of 0 against `none()`
PMI_AVG_FN bool better(int32_t value, int32_t angle, int32_t flat, const Best &b)
{
    if (value != b.value) return value > b.value;
    if (angle != b.angle) return angle < b.angle;
    return flat < b.flat;
}

PMI_AVG_FN int32_t unshift(int32_t i, int32_t n)
{
    const int32_t s = i - n / 2;
    return s < 0 ? s + n : s;
}

PMI_AVG_FN bool in_view(double x, double y, const Geom &g) { return x > g.t_min && y > g.t_min && x < g.t_max && y < g.t_max; }

// the pixel of a rotated (float64) coordinate in view; outside [0, n) only when rounding carries it there
PMI_AVG_FN int32_t pixel64(double v, const Geom &g)
{
    const double p = g.ov * (v - g.t_min);
    return p >= 0.0 && p < 2147483647.0 ? (int32_t)p : -1;
}

// the pixel of a float32 coordinate of the table (the average image)
PMI_AVG_FN int32_t pixel32(float v, const Geom &g)
{
    const double d = g.sub_f32 ? (double)(v - (float)g.t_min) : (double)v - g.t_min;
    const double p = g.mul_f32 ? (double)((float)g.ov * (float)d) : g.ov * d;
    return p >= 0.0 && p < 2147483647.0 ? (int32_t)p : -1;
}

// 0: not in view, 1: *packed = row << 16 | column, 2: in view and yet no pixel of the image
PMI_AVG_FN int rotate_bin(float x0, float y0, double c, double s, const Geom &g, uint32_t *packed)
{
    const double cx = c * (double)x0, sy = s * (double)y0;
    const double sx = s * (double)x0, cy = c * (double)y0;
    const double xr = cx - sy, yr = sx + cy;
    if (!in_view(xr, yr, g)) return 0;
    const int32_t px = pixel64(xr, g), py = pixel64(yr, g);
    if ((uint32_t)px >= (uint32_t)g.n || (uint32_t)py >= (uint32_t)g.n) return 2;
    *packed = (uint32_t)py << 16 | (uint32_t)px;
    return 1;
}

// the correlation at the unshifted shift (sy, sx) over `count` packed pixels; every index is below n * n
PMI_AVG_FN int32_t gather(const int32_t *img, const uint32_t *list, int32_t count, int32_t n, int32_t sy, int32_t sx)
{
    int32_t acc = 0;
    for (int32_t k = 0; k < count; ++k) {
        const uint32_t p = list[k];
        int32_t r = (int32_t)(p >> 16) - sy, c = (int32_t)(p & 0xffffu) - sx;
        r += r < 0 ? n : 0;
        c += c < 0 ? n : 0;
        acc += img[r * n + c];
    }
    return acc;
}

// what the reference shifts by: ceil(index - n / 2) / oversampling, in float64
PMI_AVG_FN double shift_of(int32_t index, const Geom &g)
{
    return __builtin_ceil((double)index - (double)g.n / 2.0) / g.ov;
}

// the aligned coordinates of one row, rounded to float32 as the assignment into the shared float32 array does
PMI_AVG_FN void transform(float x0, float y0, double c, double s, double dx, double dy, float *x1, float *y1)
{
    const double cx = c * (double)x0, sy = s * (double)y0;
    const double sx = s * (double)x0, cy = c * (double)y0;
    *x1 = (float)((cx - sy) - dx);
    *y1 = (float)((sx + cy) - dy);
}

}  // namespace average
}  // namespace pmi
