// render.hip — super-resolution rendering of a localization table
// (picasso/render.py:177-232 _render_setup, :451-467 _fill, :494-575 _draw_gaussian_loc /
//  _fill_gaussian, :798-853 _render_hist, :1020-1070 _render_gaussian without rotation).
//
// Histogram: one atomic float add of 1.0 per localization — exact, counts stay below 2^24.
//
// Gaussian: the reference adds every localization's separable footprint into the float32 image
// one after the other, so each pixel's value depends on the ORDER of the additions.  A scatter
// with float atomics would be correct only up to rounding; this kernel reproduces the order
// instead:
//   1. prep: per localization, image coordinates (float64, numba's promotion of the float32
//      columns), blur widths (float32), the clipped +-3 sigma footprint, the number of 32x32
//      image tiles it touches;
//   2. exclusive scan of those counts, emit (tile, localization) pairs in localization order,
//      stable radix sort by tile  ->  every tile gets its localizations in table order
//      (render_common.h, shared with the rotated view of render_rot.hip);
//   3. one workgroup per tile: 256 threads x 4 pixels in registers; the tile's list is walked
//      in chunks of 32 localizations whose 1-D profiles (float64 exp, rounded to float32 like
//      the reference's gx / gy arrays) are built cooperatively in LDS, then every pixel adds
//      gy*gx of each localization in order.  The profiles are 0 outside the footprint and
//      x + 0 == x, so a localization with finite profiles is added to the whole tile unmasked; one
//      with an inf or NaN profile value (inf * 0 = NaN) is added inside its footprint only.
// The result is the reference's image bit for bit, up to a 1-ulp difference between the
// device's and glibc's float64 exp surviving the rounding to float32.
// This file keeps its three kernels and its argument checks; the driver around them (scratch,
// empty table, empty view, tile lists), the staging of the host forms and the table of scratch
// slots are render_common.h's.
#include "render_common.h"

#pragma clang fp contract(off)

namespace pmi {
namespace rend {

struct Loc {              // one localization in view, image coordinates
    double x, y;
    float sx, sy;
    int i_min, i_max, j_min, j_max;      // clipped footprint [min, max); empty when max <= min
};

__device__ __forceinline__ bool in_view(const View &v, float xf, float yf)
{
    const double xd = (double)xf, yd = (double)yf;
    return xd > v.x_min && yd > v.y_min && xd < v.x_max && yd < v.y_max;
}

__global__ void hist_kernel(const float *__restrict__ x, const float *__restrict__ y, int64_t N, View v,
                            float *__restrict__ image, unsigned long long *__restrict__ n_rendered)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    bool ok = false;
    if (i < N && in_view(v, x[i], y[i])) {
        ok = true;
        const int32_t xi = to_int32(v.oversampling * ((double)x[i] - v.x_min));      // astype(int32): truncation
        const int32_t yi = to_int32(v.oversampling * ((double)y[i] - v.y_min));
        atomicAdd(&image[(int64_t)yi * v.nx + xi], 1.0f);
    }
    count_in_view(ok, n_rendered);
}

// footprint of picasso/render.py:505-524, including its asymmetric "+ 1"
__global__ void prep_kernel(const float *__restrict__ x, const float *__restrict__ y, const float *__restrict__ lpx,
                            const float *__restrict__ lpy, int64_t N, View v, Loc *__restrict__ locs,
                            unsigned *__restrict__ ntiles, unsigned long long *__restrict__ n_rendered)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    bool ok = false;
    if (i < N) {
        unsigned cnt = 0;
        Loc L = {};
        if (in_view(v, x[i], y[i])) {
            ok = true;
            L.x = v.oversampling * ((double)x[i] - v.x_min);
            L.y = v.oversampling * ((double)y[i] - v.y_min);
            L.sx = v.os_f * np_maxf(lpx[i], v.min_blur_f);
            L.sy = v.os_f * np_maxf(lpy[i], v.min_blur_f);
            if (v.iso) { L.sy = (L.sy + L.sx) / 2.0f; L.sx = L.sy; }
            const double max_y_off = 3.0 * (double)L.sy, max_x_off = 3.0 * (double)L.sx;
            int64_t i_min = to_int32(L.y - max_y_off), i_max = to_int32(L.y + max_y_off + 1);
            int64_t j_min = to_int32(L.x - max_x_off), j_max = (int64_t)to_int32(L.x + max_x_off) + 1;
            cnt = clamp_footprint(v, i_min, i_max, j_min, j_max);
            L.i_min = (int)i_min; L.i_max = (int)i_max; L.j_min = (int)j_min; L.j_max = (int)j_max;      // also when it is empty
        }
        locs[i] = L;
        ntiles[i] = cnt;
    }
    count_in_view(ok, n_rendered);
}

__global__ __launch_bounds__(256) void tile_kernel(const Loc *__restrict__ locs, const unsigned *__restrict__ vals,
                                                   const unsigned *__restrict__ start, const unsigned *__restrict__ end,
                                                   View v, float *__restrict__ image)
{
    __shared__ float s_gx[CHUNK][TILE], s_gy[CHUNK][TILE];
    __shared__ unsigned s_fp[CHUNK];     // footprint in tile coordinates, one byte each: col min, col max, row min, row max
    __shared__ unsigned s_bad[2];        // bit l: localization l of the chunk has a non-finite profile value (even / odd chunks)
    const int tile = blockIdx.x;
    const unsigned e0 = start[tile], e1 = end[tile];
    const int ty = tile / v.tiles_x, tx = tile - ty * v.tiles_x;
    const int row0 = ty * TILE, col0 = tx * TILE;
    const int tid = threadIdx.x;
    const int pj = tid & (TILE - 1), pi = tid >> 5;           // pixel (pi + 8 k, pj), k = 0..3
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    if (tid < 2) s_bad[tid] = 0;
    __syncthreads();
    int par = 0;
    for (unsigned c0 = e0; c0 < e1; c0 += CHUNK, par ^= 1) {
        const int nloc = (int)min((unsigned)CHUNK, e1 - c0);
        // profiles: 2 * TILE values per localization, CHUNK localizations -> 8 values per thread
        for (int q = tid; q < CHUNK * 2 * TILE; q += 256) {
            const int l = q / (2 * TILE), r = q - l * (2 * TILE);
            float val = 0.f;
            if (l < nloc) {
                const Loc L = locs[vals[c0 + l]];
                if (r < TILE) {                                  // gx at image column col0 + r
                    const int j = col0 + r;
                    if (j >= L.j_min && j < L.j_max) {
                        const double inv_2sx2 = 1.0 / (2.0 * (double)L.sx * (double)L.sx);
                        const double dx = (double)j + 0.5 - L.x;
                        val = (float)exp(-dx * dx * inv_2sx2);
                    }
                } else {                                         // gy at image row row0 + r - TILE
                    const int i = row0 + r - TILE;
                    if (i >= L.i_min && i < L.i_max) {
                        const double inv_2sy2 = 1.0 / (2.0 * (double)L.sy * (double)L.sy);
                        const double norm = 1.0 / (6.283185307179586 * (double)L.sx * (double)L.sy);
                        const double dy = (double)i + 0.5 - L.y;
                        val = (float)(norm * exp(-dy * dy * inv_2sy2));
                    }
                }
                if (!isfinite(val)) atomicOr(&s_bad[par], 1u << l);
                if (r == 0)
                    s_fp[l] = (unsigned)min(max(L.j_min - col0, 0), TILE) | (unsigned)min(max(L.j_max - col0, 0), TILE) << 8 |
                              (unsigned)min(max(L.i_min - row0, 0), TILE) << 16 | (unsigned)min(max(L.i_max - row0, 0), TILE) << 24;
            }
            if (r < TILE) s_gx[l][r] = val; else s_gy[l][r - TILE] = val;
        }
        __syncthreads();
        const unsigned bad = __builtin_amdgcn_readfirstlane(s_bad[par]);      // the same in every wave of the tile
        if (tid == 0) s_bad[par ^ 1] = 0;                                     // the next chunk's, last read before the barrier above
        if (bad == 0) {
            for (int l = 0; l < nloc; l++) {
                const float gx = s_gx[l][pj];
#pragma unroll
                for (int k = 0; k < 4; k++) acc[k] = acc[k] + s_gy[l][pi + 8 * k] * gx;
            }
        } else {
            for (int l = 0; l < nloc; l++) {
                const float gx = s_gx[l][pj];
                if (!((bad >> l) & 1u)) {
#pragma unroll
                    for (int k = 0; k < 4; k++) acc[k] = acc[k] + s_gy[l][pi + 8 * k] * gx;
                } else {                                         // inf * 0 would be NaN: leave every pixel outside the footprint alone
                    const unsigned fp = s_fp[l];
                    const bool in_col = pj >= (int)(fp & 255u) && pj < (int)((fp >> 8) & 255u);
                    const int r_min = (int)((fp >> 16) & 255u), r_max = (int)(fp >> 24);
#pragma unroll
                    for (int k = 0; k < 4; k++) {
                        const int row = pi + 8 * k;
                        if (in_col && row >= r_min && row < r_max) acc[k] = acc[k] + s_gy[l][row] * gx;
                    }
                }
            }
        }
        __syncthreads();
    }
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int i = row0 + pi + 8 * k, j = col0 + pj;
        if (i < v.ny && j < v.nx) image[(int64_t)i * v.nx + j] = acc[k];
    }
}

}  // namespace rend
}  // namespace pmi

extern "C" {

int pmi_render_dims(double oversampling, double y_min, double x_min, double y_max, double x_max, int64_t *ny, int64_t *nx)
{
    if (!ny || !nx) { pmi::set_error("null pointer"); return PMI_ERR_ARG; }
    pmi::rend::view_dims(oversampling, y_min, x_min, y_max, x_max, ny, nx);
    return PMI_OK;
}

int pmi_render_hist_dev(const float *d_x, const float *d_y, int64_t N, double oversampling, double y_min, double x_min,
                        double y_max, double x_max, float *d_image, int64_t ny, int64_t nx, int64_t *d_n_rendered,
                        void *stream)
{
    using namespace pmi;
    rend::View v;
    int rc = rend::make_view(oversampling, y_min, x_min, y_max, x_max, 0.0, ny, nx, &v);
    if (rc != PMI_OK) return rc;
    hipStream_t s = (hipStream_t)stream;
    PMI_HIP(hipMemsetAsync(d_image, 0, (size_t)ny * nx * sizeof(float), s));
    PMI_HIP(hipMemsetAsync(d_n_rendered, 0, 8, s));
    if (N > 0) PMI_LAUNCH(rend::hist_kernel, N, s, d_x, d_y, N, v, d_image, (unsigned long long *)d_n_rendered);
    return PMI_OK;
}

int pmi_render_gaussian_dev(const float *d_x, const float *d_y, const float *d_lpx, const float *d_lpy, int64_t N,
                            double oversampling, double y_min, double x_min, double y_max, double x_max,
                            double min_blur_width, int iso, float *d_image, int64_t ny, int64_t nx,
                            int64_t *d_n_rendered, void *stream)
{
    using namespace pmi;
    rend::View v;
    int rc = rend::make_view(oversampling, y_min, x_min, y_max, x_max, min_blur_width, ny, nx, &v);
    if (rc != PMI_OK) return rc;
    v.iso = iso ? 1 : 0;
    if (N > 0x7fffffffLL) { set_error("render: too many localizations"); return PMI_ERR_ARG; }
    hipStream_t s = (hipStream_t)stream;
    return rend::gaussian<rend::Loc>(N, v, d_image, d_n_rendered, s, [&](rend::Loc *locs, unsigned *ntiles, unsigned long long *n_rendered) {
        PMI_LAUNCH(rend::prep_kernel, N, s, d_x, d_y, d_lpx, d_lpy, N, v, locs, ntiles, n_rendered);
        return (int)PMI_OK;
    }, rend::tile_kernel);
}

// Host forms: columns, image and count are staged in the library's scratch (Staged, pmi_common.h), the results copied back.
static int render_host(const float *x, const float *y, const float *lpx, const float *lpy, int64_t N, double oversampling,
                       double y_min, double x_min, double y_max, double x_max, double min_blur_width, int iso, bool gaussian,
                       float *image, int64_t ny, int64_t nx, int64_t *n_rendered)
{
    using namespace pmi;
    if (pmi_device_count() < 1) { set_error("no HIP device"); return PMI_ERR_NODEVICE; }
    if (!image || !n_rendered || (N > 0 && (!x || !y || (gaussian && (!lpx || !lpy))))) { set_error("null pointer"); return PMI_ERR_ARG; }
    float *dx = nullptr, *dy = nullptr, *dlx = nullptr, *dly = nullptr, *d_img = nullptr;
    int64_t *dn = nullptr;
    const size_t n = (size_t)std::max<int64_t>(N, 0);
    Staged st(SCR_STAGE_A);
    st.add(dx, n, x), st.add(dy, n, y), st.add(dlx, n, lpx), st.add(dly, n, lpy);
    st.add(d_img, (size_t)ny * nx, nullptr, image), st.add(dn, 1, nullptr, n_rendered);
    int rc = st.place();
    if (rc != PMI_OK) return rc;
    rc = gaussian ? pmi_render_gaussian_dev(dx, dy, dlx, dly, N, oversampling, y_min, x_min, y_max, x_max, min_blur_width, iso,
                                            d_img, ny, nx, dn, nullptr)
                  : pmi_render_hist_dev(dx, dy, N, oversampling, y_min, x_min, y_max, x_max, d_img, ny, nx, dn, nullptr);
    return rc != PMI_OK ? rc : st.fetch();
}

int pmi_render_hist(const float *x, const float *y, int64_t N, double oversampling, double y_min, double x_min,
                    double y_max, double x_max, float *image, int64_t ny, int64_t nx, int64_t *n_rendered)
{
    return render_host(x, y, nullptr, nullptr, N, oversampling, y_min, x_min, y_max, x_max, 0.0, 0, false, image, ny, nx, n_rendered);
}

int pmi_render_gaussian(const float *x, const float *y, const float *lpx, const float *lpy, int64_t N,
                        double oversampling, double y_min, double x_min, double y_max, double x_max,
                        double min_blur_width, int iso, float *image, int64_t ny, int64_t nx, int64_t *n_rendered)
{
    return render_host(x, y, lpx, lpy, N, oversampling, y_min, x_min, y_max, x_max, min_blur_width, iso, true, image, ny, nx, n_rendered);
}

}  // extern "C"
