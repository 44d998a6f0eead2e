// Host build of csrc/blur_core.h for tests/test_blur_host.py: the same per-term functions the kernels of csrc/blur.hip
// are compiled from, looped the plain way over a zero-extended line (no chunks, no tiles).  A stand-alone program:
//     blur_host_driver IN OUT
// IN:  int64 ny, nx, ry, rx, has_y, has_x, round_between; float64 scale; float64 wy[2 ry + 1] if has_y;
//      float64 wx[2 rx + 1] if has_x; float32 image[ny * nx].       OUT: float32 image[ny * nx].
// Built with -ffp-contract=off.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "blur_core.h"

using namespace pmi::blur;

// one axis: `count` lines of `len` samples `stride` apart, the lines `step` apart
template <typename TIn, typename TOut>
static void pass(const TIn *in, TOut *out, int64_t count, int64_t step, int64_t len, int64_t stride, const double *w, int64_t r,
                 bool last, int scale_out, double scale)
{
    std::vector<double> line((size_t)(len + 2 * r), 0.0);
    for (int64_t c = 0; c < count; c++) {
        for (int64_t l = 0; l < len; l++) line[(size_t)(r + l)] = (double)in[c * step + l * stride];
        for (int64_t l = 0; l < len; l++) {
            const double *p = line.data() + r + l;
            double tmp = centre_term(p[0], w[r]);
            for (int64_t j = r; j >= 1; j--) tmp = add_pair(tmp, p[-j], p[j], w[r - j]);
            if (last) out[c * step + l * stride] = (TOut)round_out(tmp, scale_out, scale);
            else out[c * step + l * stride] = (TOut)tmp;          // float32 rounds here, float64 keeps tmp
        }
    }
}

int main(int argc, char **argv)
{
    if (argc != 3) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 3;
    int64_t h[7];
    double scale;
    if (fread(h, 8, 7, f) != 7 || fread(&scale, 8, 1, f) != 1) return 4;
    const int64_t ny = h[0], nx = h[1], ry = h[2], rx = h[3];
    const bool has_y = h[4] != 0, has_x = h[5] != 0, round_between = h[6] != 0;
    std::vector<double> wy(has_y ? (size_t)(2 * ry + 1) : 0), wx(has_x ? (size_t)(2 * rx + 1) : 0);
    if (has_y && fread(wy.data(), 8, wy.size(), f) != wy.size()) return 4;
    if (has_x && fread(wx.data(), 8, wx.size(), f) != wx.size()) return 4;
    const size_t n = (size_t)(ny * nx);
    std::vector<float> image(n), out(n);
    if (fread(image.data(), 4, n, f) != n) return 4;
    fclose(f);
    const int scale_out = round_between ? 0 : 1;
    if (has_y && has_x) {
        if (round_between) {
            std::vector<float> mid(n);
            pass(image.data(), mid.data(), nx, 1, ny, nx, wy.data(), ry, false, 0, 1.0);
            pass(mid.data(), out.data(), ny, nx, nx, 1, wx.data(), rx, true, 0, 1.0);
        } else {
            std::vector<double> mid(n);
            pass(image.data(), mid.data(), nx, 1, ny, nx, wy.data(), ry, false, 0, 1.0);
            pass(mid.data(), out.data(), ny, nx, nx, 1, wx.data(), rx, true, 1, scale);
        }
    } else if (has_y) {
        pass(image.data(), out.data(), nx, 1, ny, nx, wy.data(), ry, true, scale_out, scale);
    } else if (has_x) {
        pass(image.data(), out.data(), ny, nx, nx, 1, wx.data(), rx, true, scale_out, scale);
    } else {
        for (size_t i = 0; i < n; i++) out[i] = round_out((double)image[i], scale_out, scale);
    }
    f = fopen(argv[2], "wb");
    if (!f) return 5;
    if (fwrite(out.data(), 4, n, f) != n) return 6;
    fclose(f);
    return 0;
}
