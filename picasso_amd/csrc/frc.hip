// frc.hip — Fourier ring correlation and radial sums (picasso/postprocess.py:1398-1502 _frc from the two rendered
// histograms to the curve, picasso/imageprocess.py:283-321 radial_sum, picasso/masking.py:649-671 threshold_tukey).
//
//   window_kernel   crop to the odd side n, multiply by mask[i, j] = w[j] * w[n - 1 - i] as NumPy does for a float32
//                   image and a float64 mask (frc_core.h `windowed`): the float32 masked images the reference returns,
//                   and float64 copies of them for the transform.
//   hipFFT D2Z      two real-to-complex float64 transforms, half spectrum (n rows of n / 2 + 1 bins).  The reference
//                   transforms in single precision (np.fft.fft2 of float32 under NumPy 2); that noise is a property of
//                   one FFT library and is not imitated.
//   ring_kernel     one workgroup per ring, the three ring sums (numerator, power 1, power 2) in one pass over both
//                   spectra.  A ring is 2 r + 1 row segments (frc_core.h); lane t takes the segments t, t + 256, ... in
//                   that order, adds their bins left to right in float64, and the 256 partial sums meet in one tree
//                   reduction in LDS.  Every bin is read once, the order is fixed, there is no atomic: two calls give
//                   the same bits.  A half-plane ring of radius r has about pi * r bins in 2 r + 1 segments, 1.6 bins a
//                   segment on average and at most sqrt(2 r + 1) (the rows |ky| near r), so a list of segment offsets in
//                   LDS for lanes to stride over the concatenated bins would cost more than the few long rows gain; the
//                   long rows are neighbours in ky and so go to neighbouring lanes.
//   radial_kernel   the same walk over a centred full image (two segments per row), one quantity of one to two
//                   components at a time: the public radial_sum for float32 / float64 / complex64 / complex128.
//   curve_kernel    num / sqrt(|p1 * p2|), NaN -> 0.
//
// The only seam of the ring walk is BLOCK: a ring with at most BLOCK segments gives every lane at most one.  That is
// r <= 127 in the half plane (n <= 255) and r <= 63 in the full plane (n <= 127); tests/test_gpu_frc.py sits on both sides.
#include <hipfft/hipfft.h>

#include "frc_core.h"
#include "rows_common.h"

#pragma clang fp contract(off)

namespace pmi {
int fft_forward_plan(int64_t Y, int64_t X, hipfftHandle *fwd);      // xcorr.hip: shares its plan cache
namespace frc {

using rows::BLOCK;

__global__ __launch_bounds__(BLOCK) void window_kernel(const float *__restrict__ im1, const float *__restrict__ im2, int32_t m,
                                                       int32_t n, const double *__restrict__ w, float *__restrict__ out1,
                                                       float *__restrict__ out2, double *__restrict__ d1,
                                                       double *__restrict__ d2)
{
    const int64_t p = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (p >= (int64_t)n * n) return;
    const int32_t i = (int32_t)(p / n), j = (int32_t)(p - (int64_t)i * n);
    const double wj = w[j], wi = w[n - 1 - i];
    const int64_t src = (int64_t)i * m + j;
    const float a = windowed(im1[src], wj, wi), b = windowed(im2[src], wj, wi);
    out1[p] = a, out2[p] = b;
    d1[p] = (double)a, d2[p] = (double)b;
}

// side 1: the transform of one pixel is the pixel
__global__ void dc_kernel(const double *__restrict__ d1, const double *__restrict__ d2, double2 *__restrict__ f1,
                          double2 *__restrict__ f2)
{
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        f1[0] = make_double2(d1[0], 0.0);
        f2[0] = make_double2(d2[0], 0.0);
    }
}

template <int K>
__device__ __forceinline__ void reduce(double (&acc)[K], double (*s)[BLOCK])
{
    const int t = threadIdx.x;
    for (int k = 0; k < K; ++k) s[k][t] = acc[k];
    __syncthreads();
    for (int o = BLOCK / 2; o > 0; o >>= 1) {
        if (t < o)
            for (int k = 0; k < K; ++k) s[k][t] += s[k][t + o];
        __syncthreads();
    }
    for (int k = 0; k < K; ++k) acc[k] = s[k][0];
}

// grid = rings (n / 2 + 1); sums = [numerator | power 1 | power 2], `rings` values each
__global__ __launch_bounds__(BLOCK) void ring_kernel(const double2 *__restrict__ f1, const double2 *__restrict__ f2, int32_t n,
                                                     double *__restrict__ sums)
{
    __shared__ double s[3][BLOCK];
    const int32_t r = blockIdx.x, rings = n / 2 + 1;
    if (r >= rings) return;
    double acc[3] = {0.0, 0.0, 0.0};
    const int32_t n_seg = segments_of(r, false);
    for (int32_t q = threadIdx.x; q < n_seg; q += BLOCK) {
        const Segment g = segment(n, r, q, false);
        for (int32_t i = 0; i < g.count; ++i) {
            const double2 a = f1[g.first + i], b = f2[g.first + i];
            const double weight = g.kx + i == 0 ? 1.0 : 2.0;
            acc[0] += weight * (a.x * b.x + a.y * b.y);          // real(f1 * conj(f2)); the imaginary parts cancel over k, -k
            acc[1] += weight * (a.x * a.x + a.y * a.y);
            acc[2] += weight * (b.x * b.x + b.y * b.y);
        }
    }
    reduce<3>(acc, s);
    if (threadIdx.x == 0) sums[r] = acc[0], sums[rings + r] = acc[1], sums[2 * rings + r] = acc[2];
}

// T: float or double, K components per pixel (2: complex).  out[r * K + k] = T(sum in float64)
template <typename T, int K>
__global__ __launch_bounds__(BLOCK) void radial_kernel(const T *__restrict__ image, int32_t n, T *__restrict__ out)
{
    __shared__ double s[K][BLOCK];
    const int32_t r = blockIdx.x;
    if (r >= n / 2 + 1) return;
    double acc[K];
    for (int k = 0; k < K; ++k) acc[k] = 0.0;
    const int32_t n_seg = segments_of(r, true);
    for (int32_t q = threadIdx.x; q < n_seg; q += BLOCK) {
        const Segment g = segment(n, r, q, true);
        for (int32_t i = 0; i < g.count; ++i)
            for (int k = 0; k < K; ++k) acc[k] += (double)image[(g.first + i) * K + k];
    }
    reduce<K>(acc, s);
    if ((int)threadIdx.x < K) out[(int64_t)r * K + threadIdx.x] = (T)acc[threadIdx.x];
}

__global__ void curve_kernel(const double *__restrict__ sums, int32_t rings, double *__restrict__ curve)
{
    const int32_t r = blockIdx.x * BLOCK + threadIdx.x;
    if (r >= rings) return;
    const double v = sums[r] / sqrt(fabs(sums[rings + r] * sums[2 * rings + r]));
    curve[r] = v != v ? 0.0 : v;
}

static int side_of(const char *what, int64_t m, int32_t *n)
{
    const int64_t odd = (m & 1) ? m : m - 1;          // an even side loses its last row and column
    if (m < 1 || odd < 1 || odd > PMI_FRC_MAX_SIDE) {
        set_error("%s: an image side of %lld (1 ... %d after the crop to an odd side)", what, (long long)m, PMI_FRC_MAX_SIDE);
        return PMI_ERR_ARG;
    }
    *n = (int32_t)odd;
    return PMI_OK;
}

struct Stamps {       // device events around the four stages, only when the caller asks for milliseconds
    hipEvent_t e[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    bool on = false;
    int begin(bool want)
    {
        on = want;
        if (on)
            for (auto &x : e) PMI_HIP(hipEventCreate(&x));
        return PMI_OK;
    }
    int mark(int i, hipStream_t s)
    {
        if (on) PMI_HIP(hipEventRecord(e[i], s));
        return PMI_OK;
    }
    int read(float *ms)
    {
        if (on)
            for (int i = 0; i < 4; ++i) PMI_HIP(hipEventElapsedTime(ms + i, e[i], e[i + 1]));
        return PMI_OK;
    }
    ~Stamps()
    {
        for (auto x : e)
            if (x) (void)hipEventDestroy(x);
    }
};

}  // namespace frc
}  // namespace pmi

using namespace pmi;

extern "C" {

int pmi_frc_max_side(void) { return PMI_FRC_MAX_SIDE; }

int pmi_frc_curve_dev(const float *d_im1, const float *d_im2, int64_t m, const double *d_w, double *d_sums, double *d_curve,
                      float *d_masked1, float *d_masked2, float *ms4, void *stream)
{
    int32_t n = 0;
    int rc = frc::side_of("pmi_frc_curve_dev", m, &n);
    if (rc) return rc;
    if (!d_im1 || !d_im2 || !d_w || !d_sums || !d_curve || !d_masked1 || !d_masked2) {
        set_error("pmi_frc_curve_dev: NULL array");
        return PMI_ERR_ARG;
    }
    hipStream_t s = (hipStream_t)stream;
    const int32_t rings = n / 2 + 1;
    const int64_t npix = (int64_t)n * n, nspec = (int64_t)n * rings;
    double *d1 = nullptr, *d2 = nullptr;
    double2 *f1 = nullptr, *f2 = nullptr;
    if ((rc = rows::carve(SCR_STAGE_A, [&](rows::Arena &a) { d1 = a.take<double>(npix), d2 = a.take<double>(npix); }))) return rc;
    if ((rc = rows::carve(SCR_STAGE_B, [&](rows::Arena &a) { f1 = a.take<double2>(nspec), f2 = a.take<double2>(nspec); }))) return rc;
    hipfftHandle plan = nullptr;
    if (n > 1 && (rc = fft_forward_plan(n, n, &plan))) return rc;
    frc::Stamps stamps;
    if ((rc = stamps.begin(ms4 != nullptr))) return rc;
    if ((rc = stamps.mark(0, s))) return rc;
    PMI_LAUNCH(frc::window_kernel, npix, s, d_im1, d_im2, (int32_t)m, n, d_w, d_masked1, d_masked2, d1, d2);
    if ((rc = stamps.mark(1, s))) return rc;
    if (n == 1) {
        frc::dc_kernel<<<1, 1, 0, s>>>(d1, d2, f1, f2);
        PMI_HIP(hipGetLastError());
    } else {
        if (hipfftSetStream(plan, s) != HIPFFT_SUCCESS) { set_error("hipfftSetStream failed"); return PMI_ERR_HIP; }
        const bool ok = hipfftExecD2Z(plan, d1, (hipfftDoubleComplex *)f1) == HIPFFT_SUCCESS &&
                        hipfftExecD2Z(plan, d2, (hipfftDoubleComplex *)f2) == HIPFFT_SUCCESS;
        (void)hipfftSetStream(plan, nullptr);          // the plan is shared with the cross-correlation, which runs on the null stream
        if (!ok) { set_error("hipfftExecD2Z failed"); return PMI_ERR_HIP; }
    }
    if ((rc = stamps.mark(2, s))) return rc;
    frc::ring_kernel<<<(unsigned)rings, frc::BLOCK, 0, s>>>(f1, f2, n, d_sums);
    PMI_HIP(hipGetLastError());
    if ((rc = stamps.mark(3, s))) return rc;
    PMI_LAUNCH(frc::curve_kernel, rings, s, d_sums, rings, d_curve);
    if ((rc = stamps.mark(4, s))) return rc;
    PMI_HIP(hipStreamSynchronize(s));
    return stamps.read(ms4);
}

int pmi_frc_curve(const float *im1, const float *im2, int64_t m, const double *w, double *sums, double *curve, float *masked1,
                  float *masked2)
{
    if (pmi_device_count() < 1) { set_error("no HIP device"); return PMI_ERR_NODEVICE; }
    int32_t n = 0;
    int rc = frc::side_of("pmi_frc_curve", m, &n);
    if (rc) return rc;
    if (!im1 || !im2 || !w || !sums || !curve || !masked1 || !masked2) {
        set_error("pmi_frc_curve: NULL array");
        return PMI_ERR_ARG;
    }
    const int32_t rings = n / 2 + 1;
    const int64_t mpix = m * m, npix = (int64_t)n * n;
    float *d_a = nullptr, *d_b = nullptr, *d_m1 = nullptr, *d_m2 = nullptr;
    double *d_w = nullptr, *d_sums = nullptr, *d_curve = nullptr;
    Staged st(SCR_STAGE_C);          // the _dev form carves SCR_STAGE_A and SCR_STAGE_B
    st.add(d_a, mpix, im1), st.add(d_b, mpix, im2), st.add(d_w, n, w);
    st.add(d_m1, npix, nullptr, masked1), st.add(d_m2, npix, nullptr, masked2);
    st.add(d_sums, 3 * rings, nullptr, sums), st.add(d_curve, rings, nullptr, curve);
    if ((rc = st.place())) return rc;
    if ((rc = pmi_frc_curve_dev(d_a, d_b, m, d_w, d_sums, d_curve, d_m1, d_m2, nullptr, nullptr))) return rc;
    return st.fetch();
}

int pmi_radial_sum(const void *image, int dtype, int64_t n, void *out)
{
    if (pmi_device_count() < 1) { set_error("no HIP device"); return PMI_ERR_NODEVICE; }
    if (!image || !out || n < 1 || n > PMI_FRC_MAX_SIDE || !(n & 1) || dtype < PMI_RADIAL_F32 || dtype > PMI_RADIAL_C128) {
        set_error("pmi_radial_sum: a square image of odd side 1 ... %d and a type 0 ... 3, got side %lld, type %d", PMI_FRC_MAX_SIDE,
                  (long long)n, dtype);
        return PMI_ERR_ARG;
    }
    const size_t item = dtype == PMI_RADIAL_F32 ? 4 : dtype == PMI_RADIAL_C128 ? 16 : 8;
    const int64_t npix = n * n, rings = n / 2 + 1;
    char *d_image = nullptr, *d_out = nullptr;
    Staged st(SCR_STAGE_A);
    st.add(d_image, item * npix, image), st.add(d_out, item * rings, nullptr, out);
    const int rc = st.place();
    if (rc) return rc;
    const unsigned grid = (unsigned)rings;
    const int32_t side = (int32_t)n;
    switch (dtype) {
    case PMI_RADIAL_F32: frc::radial_kernel<float, 1><<<grid, frc::BLOCK>>>((const float *)d_image, side, (float *)d_out); break;
    case PMI_RADIAL_F64: frc::radial_kernel<double, 1><<<grid, frc::BLOCK>>>((const double *)d_image, side, (double *)d_out); break;
    case PMI_RADIAL_C64: frc::radial_kernel<float, 2><<<grid, frc::BLOCK>>>((const float *)d_image, side, (float *)d_out); break;
    default: frc::radial_kernel<double, 2><<<grid, frc::BLOCK>>>((const double *)d_image, side, (double *)d_out); break;
    }
    PMI_HIP(hipGetLastError());
    return st.fetch();
}

}  // extern "C"
