// Host build of csrc/frc_core.h for tests/test_frc_host.py: the same ring segments and windowed pixel the kernels of
// csrc/frc.hip are compiled from, looped the plain way.  Built with -ffp-contract=off.
#include "frc_core.h"

using namespace pmi::frc;

extern "C" {

// Walks every segment of every ring of an image of odd side n (full: the centred n x n image, else the unshifted half
// spectrum of n rows by n / 2 + 1 bins).  visits[bin] counts how often a bin was reached, ring_of[bin] is the ring that
// reached it last, weight[bin] the Hermitian weight (half plane: 1 on the column kx = 0, else 2; full plane: 1).
// Returns the number of bins a segment named outside the array (must be 0), or -1 for a segment count beyond the bound.
int frc_host_cover(int n, int full, int32_t *visits, int32_t *ring_of, int32_t *weight)
{
    const int c = n / 2;
    const int64_t bins = full ? (int64_t)n * n : (int64_t)n * (c + 1);
    int outside = 0;
    for (int r = 0; r <= c; ++r) {
        const int n_seg = segments_of(r, full != 0);
        if (n_seg > (full ? 2 : 1) * (2 * r + 3)) return -1;
        for (int s = 0; s < n_seg; ++s) {
            const Segment g = segment(n, r, s, full != 0);
            for (int i = 0; i < g.count; ++i) {
                const int64_t bin = g.first + i;
                if (bin < 0 || bin >= bins) { ++outside; continue; }
                ++visits[bin];
                ring_of[bin] = r;
                weight[bin] = full ? 1 : (g.kx + i == 0 ? 1 : 2);
            }
        }
    }
    return outside;
}

int frc_host_isqrt(long long v) { return isqrt(v); }

// the crop of an m x m float32 image to the odd side n and the window, as window_kernel does them
void frc_host_window(const float *im, int m, int n, const double *w, float *out)
{
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < n; ++j) out[(int64_t)i * n + j] = windowed(im[(int64_t)i * m + j], w[j], w[n - 1 - i]);
}

}  // extern "C"
