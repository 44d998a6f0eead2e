// Host build of csrc/cumexp_core.h for tests/test_pickkin_host.py: the same sample terms and the same step logic the kernel
// of csrc/cumexp.hip is compiled from, with the sums of a pass added in sample order instead of across a wavefront, and
// segment_stats.h for the NumPy means.  A stand-alone program:
//     cumexp_host_driver IN OUT
// IN:  int64 n_seg, n_values, kind (0 integer column, 1 float32, 2 float64); int64 offsets[n_seg + 1];
//      float64 values[n_values].      OUT: float64 a, t, c, cost [n_seg each]; int32 iterations, status [n_seg each].
// Built with -ffp-contract=off.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "cumexp_core.h"
#include "segment_stats.h"

using namespace pmi::cumexp;

static void sums_at(const double *x, int32_t n, double a, double t, double c, double *s)
{
    for (int k = 0; k < N_SUMS; ++k) s[k] = 0.0;
    for (int32_t i = 0; i < n; ++i) add_sample(s, x[i], (double)(i + 1), a, t, c);
}

int main(int argc, char **argv)
{
    if (argc != 3) return 2;
    FILE *fp = fopen(argv[1], "rb");
    if (!fp) return 3;
    int64_t h[3];
    if (fread(h, 8, 3, fp) != 3) return 4;
    const int64_t n_seg = h[0], n_values = h[1];
    const int kind = (int)h[2];
    std::vector<int64_t> offsets((size_t)n_seg + 1);
    std::vector<double> values((size_t)n_values);
    if (fread(offsets.data(), 8, offsets.size(), fp) != offsets.size()) return 4;
    if (n_values && fread(values.data(), 8, values.size(), fp) != values.size()) return 4;
    fclose(fp);
    const double nan = std::nan("");
    std::vector<double> fit((size_t)n_seg * 4, nan);
    std::vector<int32_t> info((size_t)n_seg * 2, 0);
    for (int64_t seg = 0; seg < n_seg; ++seg) {
        const int64_t lo = offsets[seg], hi = offsets[seg + 1];
        if (lo < 0 || hi < lo || hi > n_values) { info[n_seg + seg] = BAD_INPUT; continue; }
        const int32_t n = (int32_t)(hi - lo);
        if (n == 0) continue;
        double *x = values.data() + lo;
        // the segmented radix sort orders bit patterns: NaN with the sign bit first, any other NaN last
        std::sort(x, x + n, [](double p, double q) {
            const int rp = p != p ? (std::signbit(p) ? 0 : 2) : 1, rq = q != q ? (std::signbit(q) ? 0 : 2) : 1;
            return rp != rq ? rp < rq : (rp == 1 && p < q);
        });
        double sum = 0.0, seen = 0.0, wild = 0.0, mn = INFINITY, mx = -INFINITY;
        for (int32_t i = 0; i < n; ++i) {
            const double v = x[i];
            const bool is_nan = v != v;
            sum += is_nan ? 0.0 : v;
            seen += is_nan ? 0.0 : 1.0;
            wild += (is_nan || std::fabs(v) == INFINITY) ? 1.0 : 0.0;
            mn = v < mn ? v : mn;
            mx = v > mx ? v : mx;
        }
        if (n <= 2 || (wild == 0.0 && mx - mn == 0.0)) {
            double mean = nan;
            if (kind == 0) {
                mean = sum / (double)n;
            } else if (seen > 0.0 && kind == 1) {
                const float tot = pmi::segstats::reduce_sum<float>([&](int32_t p) { const float v = (float)x[p]; return v == v ? v : 0.0f; }, 0, n);
                mean = (double)(float)((double)tot / seen);
            } else if (seen > 0.0) {
                const double tot = pmi::segstats::reduce_sum<double>([&](int32_t p) { const double v = x[p]; return v == v ? v : 0.0; }, 0, n);
                mean = tot / seen;
            }
            fit[n_seg + seg] = mean;
        } else if (wild != 0.0 || mn < 0.0) {
            info[n_seg + seg] = BAD_INPUT;
        } else {
            Fit f;
            double s[N_SUMS];
            start(f, (double)n, sum / (double)n, mn, mx);
            sums_at(x, n, f.trial[0], f.trial[1], f.trial[2], s);
            take(f, s);
            f.iters = 1;
            for (int it = 1; it < MAX_ITER; ++it) {
                if (!propose(f)) break;
                sums_at(x, n, f.trial[0], f.trial[1], f.trial[2], s);
                f.iters++;
                judge(f, s);
                if (f.done) break;
            }
            fit[seg] = f.p[0], fit[n_seg + seg] = f.p[1], fit[2 * n_seg + seg] = f.p[2], fit[3 * n_seg + seg] = f.cost;
            info[seg] = f.iters, info[n_seg + seg] = f.status;
        }
    }
    fp = fopen(argv[2], "wb");
    if (!fp) return 5;
    if (fwrite(fit.data(), 8, fit.size(), fp) != fit.size()) return 6;
    if (fwrite(info.data(), 4, info.size(), fp) != info.size()) return 6;
    fclose(fp);
    return 0;
}
