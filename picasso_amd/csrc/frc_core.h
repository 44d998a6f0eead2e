// frc_core.h — the arithmetic of the Fourier ring correlation (picasso/postprocess.py:1398-1502 _frc,
// picasso/imageprocess.py:283-321 radial_sum, picasso/masking.py:649-671 threshold_tukey), shared by frc.hip and the
// host-side check of it (tests/frc_host_driver.cpp): the windowed pixel, the integer square root and the row segments of
// a ring.  Plain C++: it compiles for the host.
//
// The rings.  The image side n is odd, c = n / 2 is the centre (frequency 0 after fftshift).  A bin at the signed
// offset (kx, ky) from the centre has d = kx * kx + ky * ky and belongs to ring r iff r * r <= d < (r + 1) * (r + 1);
// only the rings 0 ... c exist, the corners beyond them belong to none.  In row ky (|ky| <= r) the ring is
//     lo <= |kx| <= hi,   lo = ceil(sqrt(r * r - ky * ky)),   hi = min(c, floor(sqrt((r + 1) * (r + 1) - ky * ky - 1))),
// both from an integer square root, never from a rounded float.  lo <= r <= c and lo <= hi, so no row of a ring is empty.
//
// The two layouts.
//   HALF  the unshifted half spectrum of a real-to-complex transform, n rows of c + 1 bins: row ky is stored at
//         ky mod n, only kx in [0, c] exists.  Ring r is 2 r + 1 segments (one per ky = -r ... r), bins [lo, hi].  A ring
//         is symmetric under k -> -k and F(-k) = conj F(k), so a sum over the whole plane is the sum over this half
//         with weight 1 on the column kx = 0 (where ky and -ky are both stored) and 2 elsewhere; n is odd, there is
//         no Nyquist column.
//   FULL  a centred n x n image (what radial_sum takes): row ky at c + ky, column kx at c + kx.  Ring r is
//         2 (2 r + 1) segments, two per ky: side 0 is [c + lo, c + hi], side 1 is [c - hi, c - max(lo, 1)] (empty when
//         lo = hi = 0, i.e. the centre bin, which side 0 holds).
//
// The window.  mask[i, j] = w[j] * w[n - 1 - i] is ONE float64 product (np.tile times np.rot90 of it), and
// `im *= mask` on a float32 array multiplies in float64 and rounds once: float32(float64(im) * mask).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define PMI_FRC_FN __host__ __device__ __forceinline__
#else
#define PMI_FRC_FN static inline
#endif
#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace pmi {
namespace frc {

// largest s with s * s <= v (v >= 0, below 2^52: the float64 root is then off by at most one)
PMI_FRC_FN int32_t isqrt(int64_t v)
{
    if (v <= 0) return 0;
    int64_t s = (int64_t)__builtin_sqrt((double)v);
    if (s * s > v) --s;
    if ((s + 1) * (s + 1) <= v) ++s;
    return (int32_t)s;
}

struct Segment {
    int64_t first;      // flat index of the first bin (row * width + column)
    int32_t count;      // bins, contiguous from `first`
    int32_t kx;         // signed column offset of the first bin from frequency 0
};

PMI_FRC_FN int32_t segments_of(int32_t r, bool full) { return full ? 2 * (2 * r + 1) : 2 * r + 1; }

// segment s of ring r (0 <= r <= n / 2, 0 <= s < segments_of(r, full)) of an image of odd side n
PMI_FRC_FN Segment segment(int32_t n, int32_t r, int32_t s, bool full)
{
    const int32_t c = n / 2;
    const int32_t ky = (full ? (s >> 1) : s) - r;
    const int64_t a = (int64_t)r * r - (int64_t)ky * ky, b = (int64_t)(r + 1) * (r + 1) - (int64_t)ky * ky;
    int32_t lo = isqrt(a);
    if ((int64_t)lo * lo < a) ++lo;
    int32_t hi = isqrt(b - 1);
    if (hi > c) hi = c;
    Segment g;
    if (!full) {
        const int32_t row = ky < 0 ? ky + n : ky;
        g.first = (int64_t)row * (c + 1) + lo;
        g.count = hi - lo + 1;
        g.kx = lo;
    } else if (!(s & 1)) {
        g.first = (int64_t)(c + ky) * n + c + lo;
        g.count = hi - lo + 1;
        g.kx = lo;
    } else {
        const int32_t inner = lo > 1 ? lo : 1;
        g.first = (int64_t)(c + ky) * n + c - hi;
        g.count = hi - inner + 1;
        g.kx = -hi;
    }
    if (g.count < 0) g.count = 0;
    return g;
}

// a histogram pixel under the Tukey window: w_j = w[column], w_i = w[n - 1 - row]
PMI_FRC_FN float windowed(float pixel, double w_j, double w_i)
{
    const double mask = w_j * w_i;
    return (float)((double)pixel * mask);
}

}  // namespace frc
}  // namespace pmi
