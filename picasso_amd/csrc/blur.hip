// blur.hip — separable blur of a float32 image that is resident on the device: the image blur behind the "smooth" and
// "convolve" renders (picasso/render.py:1413-1460 _fftconvolve).
//
// Spatial route (round_between = 1): scipy.ndimage.gaussian_filter(mode="constant", cval=0) restated bit for bit.  scipy
// runs one correlate1d per axis, axis 0 (y) first, writes float32 after the first axis and reads that float32 back for the
// second.  Per output sample l of a line extended by zeros, with the symmetric float64 weights w[0 .. 2 r]:
//     tmp = line[l] * w[r];   for j = r .. 1:   tmp += (line[l - j] + line[l + j]) * w[r - j];     (float64)
// and tmp is rounded to float32.  The kernels below perform exactly these operations in exactly this order, including the
// terms whose two samples lie outside the image (they add +0.0, which scipy's zero-extended line adds too).
//
// Direct route (round_between = 0): the same two sums with the reference's unnormalised window weights, a float64
// intermediate between the axes, then tmp * scale (scale = 1 / kernel.sum(), from the host) and ONE rounding to float32.
// It stands in for the reference's single-precision FFT convolution, whose noise is not imitated.
//
// Layout.  One output sample per lane in the row pass, eight per lane (one column strip) in the column pass; both passes
// load along x, so every global access is coalesced, and the column pass walks rows in LDS instead of transposing.  The
// radius has no upper bound, so the walk j = r .. 1 is cut in chunks of CHUNK steps: per chunk a workgroup stages the two
// windows of samples the chunk reads (the far side l - j and the near side l + j of every output of its tile) and the
// chunk's weights in LDS.  Every weight and every sample is staged once per workgroup and tile; the accumulators stay in
// registers across chunks.  No atomics, no float32 accumulation, contraction off.
//
// The image limits (rend::check_image) are render_common.h's, the staging of the host forms (Staged) and the table of
// scratch slots pmi_common.h's: pmi_blur_dev keeps the image between the passes in SCR_STAGE_D, the host forms everything in SCR_STAGE_A.
#include "render_common.h"

#include "blur_core.h"

#pragma clang fp contract(off)

namespace pmi {
namespace blur {

constexpr int ROW_T = 256;          // row pass: outputs of a tile = lanes of a workgroup, along x
constexpr int ROW_C = 64;           // ... steps of j per chunk
constexpr int COL_X = 64;           // column pass: columns of a tile (one wave reads 64 consecutive pixels of a row)
constexpr int COL_Y = 32;           // ... rows of a tile, COL_PER of them per lane
constexpr int COL_PER = 8;
constexpr int COL_C = 32;           // ... steps of j per chunk
constexpr unsigned MAX_GRID = 1u << 20;      // workgroups of a launch; a workgroup walks tiles in strides of the grid

template <typename T>
__device__ __forceinline__ T finish(double tmp, int scale_out, double scale);
template <>
__device__ __forceinline__ float finish<float>(double tmp, int scale_out, double scale)
{
    return round_out(tmp, scale_out, scale);
}
template <>
__device__ __forceinline__ double finish<double>(double tmp, int, double) { return tmp; }

// axis 1: out[y][x] from in[y][x - r .. x + r]
template <typename TIn>
__global__ __launch_bounds__(ROW_T) void row_pass_kernel(const TIn *__restrict__ in, float *__restrict__ out, int64_t ny, int64_t nx,
                                                         const double *__restrict__ w, int64_t r, int scale_out, double scale,
                                                         int64_t tiles_x, int64_t ntiles)
{
    __shared__ double s_far[ROW_T + ROW_C], s_near[ROW_T + ROW_C], s_w[ROW_C];
    const int t = threadIdx.x;
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int64_t y = tile / tiles_x, x0 = (tile - y * tiles_x) * ROW_T;
        const TIn *line = in + y * nx;
        const int64_t x = x0 + t;
        double tmp = 0.0;
        if (x < nx) tmp = centre_term((double)line[x], w[r]);
        for (int64_t j_hi = r; j_hi >= 1; j_hi -= ROW_C) {
            const int64_t j_lo = j_hi - ROW_C + 1 > 1 ? j_hi - ROW_C + 1 : 1;
            const int steps = (int)(j_hi - j_lo + 1);              // 1 .. ROW_C
            const int span = ROW_T + steps - 1;                    // samples of a window, < ROW_T + ROW_C
            __syncthreads();                                       // the chunk before (or the tile before) is read
            for (int k = t; k < span; k += ROW_T) {
                const int64_t a = x0 - j_hi + k, b = x0 + j_lo + k;
                s_far[k] = (a >= 0 && a < nx) ? (double)line[a] : 0.0;
                s_near[k] = (b >= 0 && b < nx) ? (double)line[b] : 0.0;
            }
            if (t < steps) s_w[t] = w[r - j_hi + t];               // the weight of j = j_hi - t
            __syncthreads();
            for (int k = 0; k < steps; k++)                        // j = j_hi - k: sample x - j at t + k, x + j at t + steps - 1 - k
                tmp = add_pair(tmp, s_far[t + k], s_near[t + steps - 1 - k], s_w[k]);
        }
        if (x < nx) out[y * nx + x] = finish<float>(tmp, scale_out, scale);
    }
}

// axis 0: out[y][x] from in[y - r .. y + r][x]
template <typename TOut>
__global__ __launch_bounds__(COL_X * COL_Y / COL_PER) void col_pass_kernel(const float *__restrict__ in, TOut *__restrict__ out, int64_t ny,
                                                                           int64_t nx, const double *__restrict__ w, int64_t r,
                                                                           int scale_out, double scale, int64_t tiles_x, int64_t ntiles)
{
    constexpr int LANES = COL_X * COL_Y / COL_PER;
    __shared__ float s_far[COL_Y + COL_C][COL_X], s_near[COL_Y + COL_C][COL_X];
    __shared__ double s_w[COL_C];
    const int t = threadIdx.x, tx = t % COL_X, ty = (t / COL_X) * COL_PER;
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int64_t tile_y = tile / tiles_x, y0 = tile_y * COL_Y, x0 = (tile - tile_y * tiles_x) * COL_X;
        const int64_t x = x0 + tx;
        double tmp[COL_PER];
#pragma unroll
        for (int i = 0; i < COL_PER; i++) {
            const int64_t y = y0 + ty + i;
            tmp[i] = (x < nx && y < ny) ? centre_term((double)in[y * nx + x], w[r]) : 0.0;
        }
        for (int64_t j_hi = r; j_hi >= 1; j_hi -= COL_C) {
            const int64_t j_lo = j_hi - COL_C + 1 > 1 ? j_hi - COL_C + 1 : 1;
            const int steps = (int)(j_hi - j_lo + 1);              // 1 .. COL_C
            const int span = COL_Y + steps - 1;                    // rows of a window, < COL_Y + COL_C
            __syncthreads();
            for (int q = t; q < span * COL_X; q += LANES) {
                const int k = q / COL_X, c = q - k * COL_X;
                const int64_t a = y0 - j_hi + k, b = y0 + j_lo + k, xc = x0 + c;
                s_far[k][c] = (xc < nx && a >= 0 && a < ny) ? in[a * nx + xc] : 0.0f;
                s_near[k][c] = (xc < nx && b >= 0 && b < ny) ? in[b * nx + xc] : 0.0f;
            }
            if (t < steps) s_w[t] = w[r - j_hi + t];
            __syncthreads();
            for (int k = 0; k < steps; k++) {                      // j = j_hi - k
                const double wk = s_w[k];
#pragma unroll
                for (int i = 0; i < COL_PER; i++)
                    tmp[i] = add_pair(tmp[i], (double)s_far[ty + i + k][tx], (double)s_near[ty + i + steps - 1 - k][tx], wk);
            }
        }
#pragma unroll
        for (int i = 0; i < COL_PER; i++) {
            const int64_t y = y0 + ty + i;
            if (x < nx && y < ny) out[y * nx + x] = finish<TOut>(tmp[i], scale_out, scale);
        }
    }
}

__global__ void scale_copy_kernel(const float *__restrict__ in, float *__restrict__ out, int64_t n, int scale_out, double scale)
{
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        out[i] = finish<float>((double)in[i], scale_out, scale);
}

static unsigned grid_of(int64_t ntiles) { return (unsigned)(ntiles < (int64_t)MAX_GRID ? ntiles : (int64_t)MAX_GRID); }

}  // namespace blur
}  // namespace pmi

extern "C" {

int pmi_blur_dev(const float *d_in, float *d_out, int64_t ny, int64_t nx, const double *d_wy, int64_t ry,
                 const double *d_wx, int64_t rx, int round_between, double scale, void *stream)
{
    using namespace pmi;
    int rc = rend::check_image("blur", ny, nx);
    if (rc != PMI_OK) return rc;
    if (!d_in || !d_out || d_in == d_out) { set_error("blur: input and output must be two device images"); return PMI_ERR_ARG; }
    if ((d_wy && ry < 0) || (d_wx && rx < 0) || ry > 0x3fffffff || rx > 0x3fffffff) { set_error("blur: bad radius"); return PMI_ERR_ARG; }
    hipStream_t s = (hipStream_t)stream;
    const int scale_out = round_between ? 0 : 1;
    const int64_t col_tx = (nx + blur::COL_X - 1) / blur::COL_X, col_n = col_tx * ((ny + blur::COL_Y - 1) / blur::COL_Y);
    const int64_t row_tx = (nx + blur::ROW_T - 1) / blur::ROW_T, row_n = row_tx * ny;
    constexpr int COL_LANES = blur::COL_X * blur::COL_Y / blur::COL_PER;
    if (d_wy && d_wx) {
        char *mid = nullptr;               // the image between the passes, float32 or float64
        if ((rc = rows::carve(SCR_STAGE_D, [&](rows::Arena &a) { mid = a.take<char>((size_t)ny * nx * (round_between ? 4 : 8)); })) != PMI_OK) return rc;
        if (round_between) {
            hipLaunchKernelGGL(blur::col_pass_kernel<float>, dim3(blur::grid_of(col_n)), dim3(COL_LANES), 0, s, d_in, (float *)mid, ny, nx,
                               d_wy, ry, 0, 1.0, col_tx, col_n);
            PMI_HIP(hipGetLastError());
            hipLaunchKernelGGL(blur::row_pass_kernel<float>, dim3(blur::grid_of(row_n)), dim3(blur::ROW_T), 0, s, (const float *)mid, d_out,
                               ny, nx, d_wx, rx, 0, 1.0, row_tx, row_n);
        } else {
            hipLaunchKernelGGL(blur::col_pass_kernel<double>, dim3(blur::grid_of(col_n)), dim3(COL_LANES), 0, s, d_in, (double *)mid, ny, nx,
                               d_wy, ry, 0, 1.0, col_tx, col_n);
            PMI_HIP(hipGetLastError());
            hipLaunchKernelGGL(blur::row_pass_kernel<double>, dim3(blur::grid_of(row_n)), dim3(blur::ROW_T), 0, s, (const double *)mid, d_out,
                               ny, nx, d_wx, rx, 1, scale, row_tx, row_n);
        }
    } else if (d_wy) {
        hipLaunchKernelGGL(blur::col_pass_kernel<float>, dim3(blur::grid_of(col_n)), dim3(COL_LANES), 0, s, d_in, d_out, ny, nx, d_wy, ry,
                           scale_out, scale, col_tx, col_n);
    } else if (d_wx) {
        hipLaunchKernelGGL(blur::row_pass_kernel<float>, dim3(blur::grid_of(row_n)), dim3(blur::ROW_T), 0, s, d_in, d_out, ny, nx, d_wx, rx,
                           scale_out, scale, row_tx, row_n);
    } else if (round_between) {
        PMI_HIP(hipMemcpyAsync(d_out, d_in, (size_t)ny * nx * sizeof(float), hipMemcpyDeviceToDevice, s));
    } else {
        const int64_t n = ny * nx;
        hipLaunchKernelGGL(blur::scale_copy_kernel, dim3(blur::grid_of((n + 255) / 256)), dim3(256), 0, s, d_in, d_out, n, 1, scale);
    }
    PMI_HIP(hipGetLastError());
    return PMI_OK;
}

// the weights of both axes named to `st`; a skipped axis has no piece and keeps its nullptr
static int stage_weights(pmi::Staged &st, const double *wy, int64_t ry, const double *wx, int64_t rx, double *&d_wy, double *&d_wx)
{
    using namespace pmi;
    if ((wy && ry < 0) || (wx && rx < 0) || ry > 0x3fffffff || rx > 0x3fffffff) { set_error("blur: bad radius"); return PMI_ERR_ARG; }
    if (wy) st.add(d_wy, (size_t)(2 * ry + 1), wy);
    if (wx) st.add(d_wx, (size_t)(2 * rx + 1), wx);
    return PMI_OK;
}

int pmi_blur(const float *in, float *out, int64_t ny, int64_t nx, const double *wy, int64_t ry, const double *wx,
             int64_t rx, int round_between, double scale)
{
    using namespace pmi;
    if (pmi_device_count() < 1) { set_error("no HIP device"); return PMI_ERR_NODEVICE; }
    if (!in || !out) { set_error("null pointer"); return PMI_ERR_ARG; }
    int rc = rend::check_image("blur", ny, nx);
    if (rc != PMI_OK) return rc;
    float *d_in = nullptr, *d_out = nullptr;
    double *d_wy = nullptr, *d_wx = nullptr;
    Staged st(SCR_STAGE_A);
    st.add(d_in, (size_t)ny * nx, in), st.add(d_out, (size_t)ny * nx, nullptr, out);
    if ((rc = stage_weights(st, wy, ry, wx, rx, d_wy, d_wx)) != PMI_OK || (rc = st.place()) != PMI_OK) return rc;
    rc = pmi_blur_dev(d_in, d_out, ny, nx, d_wy, ry, d_wx, rx, round_between, scale, nullptr);
    return rc != PMI_OK ? rc : st.fetch();
}

int pmi_render_blurred(const float *x, const float *y, int64_t N, double oversampling, double y_min, double x_min,
                       double y_max, double x_max, const double *wy, int64_t ry, const double *wx, int64_t rx,
                       int round_between, double scale, float *image, int64_t ny, int64_t nx, int64_t *n_rendered)
{
    using namespace pmi;
    if (pmi_device_count() < 1) { set_error("no HIP device"); return PMI_ERR_NODEVICE; }
    if (!image || !n_rendered || (N > 0 && (!x || !y))) { set_error("null pointer"); return PMI_ERR_ARG; }
    int rc = rend::check_image("blur", ny, nx);
    if (rc != PMI_OK) return rc;
    float *dx = nullptr, *dy = nullptr, *d_hist = nullptr, *d_out = nullptr;
    double *d_wy = nullptr, *d_wx = nullptr;
    int64_t *dn = nullptr;
    const size_t n = (size_t)(N > 0 ? N : 0);
    Staged st(SCR_STAGE_A);
    st.add(dx, n, x), st.add(dy, n, y), st.add(d_hist, (size_t)ny * nx), st.add(dn, 1, nullptr, n_rendered);
    st.add(d_out, (size_t)ny * nx, nullptr, image);
    if ((rc = stage_weights(st, wy, ry, wx, rx, d_wy, d_wx)) != PMI_OK || (rc = st.place()) != PMI_OK) return rc;
    // the histogram stays on the device: fill, then blur, on one stream
    if ((rc = pmi_render_hist_dev(dx, dy, N, oversampling, y_min, x_min, y_max, x_max, d_hist, ny, nx, dn, nullptr)) != PMI_OK) return rc;
    rc = pmi_blur_dev(d_hist, d_out, ny, nx, d_wy, ry, d_wx, rx, round_between, scale, nullptr);
    return rc != PMI_OK ? rc : st.fetch();
}

}  // extern "C"
