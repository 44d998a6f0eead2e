// render_rot.hip — the rotated 3-D views of a localization table
// (picasso/render.py:1571-1637 locs_rotation, :798-853 _render_hist and :1020-1216 _render_gaussian /
//  _render_gaussian_iso with ang, :578-679 _draw_gaussian_rot_loc / _fill_gaussian_rot).
//
// Rotation, per row, about the centre of the viewport (cx = x_min + (x_max - x_min) / 2, cy likewise, float64 from the
// host).  The coordinate columns come as three float32 columns (the centre is then subtracted in float32, as NumPy does
// on the float32 array the reference takes from the table) or as three float64 columns.  With the row v widened to
// float64,   r_i = (M[i][0] * v0 + M[i][1] * v1) + M[i][2] * v2,   unfused: the order scipy's Rotation.apply
// (einsum 'ijk,ik->ij') evaluates on the column-major (N, 3) array pandas makes of the three columns.  A table of one row
// is row-major as well, and einsum then evaluates (M[i][0] * v0 + M[i][2] * v2) + M[i][1] * v1: N == 1 takes that order
// (DESIGN 8 N21).  M is always scipy's own float64 matrix, handed in by the host.  The centre is added
// back in float64, "in view" is strict on all four sides, then x' = os * (x - x_min), y' = os * (y - y_min), z' = os * z.
//
// Histogram: int32 truncation of x', y' and one atomic float add of 1.0, as render.hip's.  (A row whose x' or y' rounds
// up to the image side is counted and not drawn: the reference writes out of bounds there.)
//
// Gaussian: the projection of the rotated 3-D Gaussian is not separable, so every pixel of a footprint costs one float64
// exp.  The order of the additions into a pixel is the table's, by render.hip's tile schedule (render_common.h):
//   1. prep: rotate; float32 widths sx, sy (render.hip's, with the iso mean) and sz = os * max(lpz, min_blur), lpz =
//      2 * ((lpx + lpy) / 2) where the table has none; the float32 projected covariance
//          P[i][k] = R[i][k] * s_k^2,   S[i][j] = fma(P[i][2], R[j][2], fma(P[i][1], R[j][1], P[i][0] * R[j][0]))
//      (the fused chain in k order is what the reference's float32 3x3 products give through BLAS), det = S00 S11 -
//      S01 S10; a row with (double)det < 1e-10 is counted and draws nothing; the float32 inverse, the float64 norm, the
//      +-3 sqrt(S00) / 3 sqrt(S11) footprint by int64 truncation (NaN and out of range -> INT64_MIN: a NaN or infinite
//      width gives an empty footprint);
//   2. the tile lists;
//   3. one workgroup per 32x32 tile, 256 threads x 4 pixels in registers; the list is walked in chunks of 32 records
//      staged in LDS (every lane reads the same record: broadcast reads), and inside the footprint only
//          a = (float)(j + 0.5 - x'),  b = (float)(i + 0.5 - y'),
//          e = ((a a) inv00 + ((a b) m)) + (b b) inv11                                (float32)
//          pix = (float)((double)pix + norm * exp(-0.5 * (double)e))
//      with glibc's exp (libm_glibc.h), the reference's under numba: the image is the reference's in every bit.
//      A wave owns 8 whole rows of the tile and skips a record whose footprint misses them.
// Contraction is off; the only fused operations are the ones written out above and those inside libm_glibc.h.
// The driver around prep and tile kernel (rend::gaussian), the footprint clamp, the count of rows in view, the staging of
// the host forms and the table of scratch slots are render_common.h's, shared with render.hip.
#include "render_common.h"

#include "libm_glibc.h"

#pragma clang fp contract(off)

namespace pmi {
namespace rend {

namespace {

// 2^(k/128) for pmi_glibc::exp; the tile kernel copies it to LDS
__constant__ uint64_t k_rot_exp_tab[PMI_GLIBC_EXP_TABLE_WORDS] = {
#include "libm_glibc_exp_table.inc"
};

struct Rot {
    double m[9];             // scipy's matrix, row major
    float r[9];              // the same rounded to float32 (the covariance)
    double cx, cy;           // centre of the viewport
    int one_row;             // the table has one row: the other order of the sum (file header)
};

struct RLoc {             // one localization of the rotated view, image coordinates
    double x, y, norm;
    float inv00, m, inv11;
    int i_min, i_max, j_min, j_max;      // clipped footprint [min, max); empty when max <= min
};

struct Rotated { double x, y, z; bool ok; };      // image units; ok: strictly inside the viewport

template <class T>
__device__ __forceinline__ Rotated rotate_row(const T *__restrict__ x, const T *__restrict__ y, const T *__restrict__ z,
                                              int64_t i, const View &v, const Rot &R)
{
    double v0, v1;
    if (sizeof(T) == 4) {
        v0 = (double)((float)x[i] - (float)R.cx);
        v1 = (double)((float)y[i] - (float)R.cy);
    } else {
        v0 = (double)x[i] - R.cx;
        v1 = (double)y[i] - R.cy;
    }
    const double v2 = (double)z[i];
    double r0, r1, r2;
    if (R.one_row) {
        r0 = (R.m[0] * v0 + R.m[2] * v2) + R.m[1] * v1;
        r1 = (R.m[3] * v0 + R.m[5] * v2) + R.m[4] * v1;
        r2 = (R.m[6] * v0 + R.m[8] * v2) + R.m[7] * v1;
    } else {
        r0 = (R.m[0] * v0 + R.m[1] * v1) + R.m[2] * v2;
        r1 = (R.m[3] * v0 + R.m[4] * v1) + R.m[5] * v2;
        r2 = (R.m[6] * v0 + R.m[7] * v1) + R.m[8] * v2;
    }
    const double xr = r0 + R.cx, yr = r1 + R.cy;
    Rotated o;
    o.ok = xr > v.x_min && yr > v.y_min && xr < v.x_max && yr < v.y_max;
    o.x = v.oversampling * (xr - v.x_min);
    o.y = v.oversampling * (yr - v.y_min);
    o.z = v.oversampling * r2;
    return o;
}

template <class T>
__global__ void rotate_kernel(const T *__restrict__ x, const T *__restrict__ y, const T *__restrict__ z, int64_t N, View v,
                              Rot R, double *__restrict__ xo, double *__restrict__ yo, double *__restrict__ zo,
                              uint8_t *__restrict__ in_view)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    const Rotated o = rotate_row(x, y, z, i, v, R);
    xo[i] = o.x; yo[i] = o.y; zo[i] = o.z;
    in_view[i] = o.ok ? 1 : 0;
}

template <class T>
__global__ void hist_rot_kernel(const T *__restrict__ x, const T *__restrict__ y, const T *__restrict__ z, int64_t N, View v,
                                Rot R, float *__restrict__ image, unsigned long long *__restrict__ n_rendered)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    bool ok = false;
    if (i < N) {
        const Rotated o = rotate_row(x, y, z, i, v, R);
        ok = o.ok;
        if (ok) {
            const int32_t xi = to_int32(o.x), yi = to_int32(o.y);               // astype(int32): truncation
            if (xi >= 0 && yi >= 0 && xi < v.nx && yi < v.ny) atomicAdd(&image[(int64_t)yi * v.nx + xi], 1.0f);
        }
    }
    count_in_view(ok, n_rendered);
}

template <class T>
__global__ void prep_rot_kernel(const T *__restrict__ x, const T *__restrict__ y, const T *__restrict__ z,
                                const float *__restrict__ lpx, const float *__restrict__ lpy, const float *__restrict__ lpz,
                                int64_t N, View v, Rot R, RLoc *__restrict__ locs, unsigned *__restrict__ ntiles,
                                unsigned long long *__restrict__ n_rendered)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    bool ok = false;
    if (i < N) {
        unsigned cnt = 0;
        RLoc L = {};
        const Rotated o = rotate_row(x, y, z, i, v, R);
        if (o.ok) {
            ok = true;
            float sx = v.os_f * np_maxf(lpx[i], v.min_blur_f);
            float sy = v.os_f * np_maxf(lpy[i], v.min_blur_f);
            if (v.iso) { sy = (sy + sx) / 2.0f; sx = sy; }
            const float pz = lpz ? lpz[i] : 2.0f * ((lpx[i] + lpy[i]) / 2.0f);
            const float sz = v.os_f * np_maxf(pz, v.min_blur_f);
            const float c0 = sx * sx, c1 = sy * sy, c2 = sz * sz;
            const float p00 = R.r[0] * c0, p01 = R.r[1] * c1, p02 = R.r[2] * c2;
            const float p10 = R.r[3] * c0, p11 = R.r[4] * c1, p12 = R.r[5] * c2;
            const float s00 = __builtin_fmaf(p02, R.r[2], __builtin_fmaf(p01, R.r[1], p00 * R.r[0]));
            const float s01 = __builtin_fmaf(p02, R.r[5], __builtin_fmaf(p01, R.r[4], p00 * R.r[3]));
            const float s10 = __builtin_fmaf(p12, R.r[2], __builtin_fmaf(p11, R.r[1], p10 * R.r[0]));
            const float s11 = __builtin_fmaf(p12, R.r[5], __builtin_fmaf(p11, R.r[4], p10 * R.r[3]));
            const float det = s00 * s11 - s01 * s10;
            if (!((double)det < 1e-10)) {
                L.x = o.x; L.y = o.y;
                L.inv00 = s11 / det;
                const float inv01 = -s01 / det, inv10 = -s10 / det;
                L.inv11 = s00 / det;
                L.m = inv01 + inv10;
                L.norm = 1.0 / (6.283185307179586 * (double)sqrtf(det));
                const double max_x_off = 3.0 * (double)sqrtf(s00), max_y_off = 3.0 * (double)sqrtf(s11);
                int64_t j_min = to_int64(o.x - max_x_off), j_max = to_int64(o.x + max_x_off + 1);
                int64_t i_min = to_int64(o.y - max_y_off), i_max = to_int64(o.y + max_y_off + 1);
                cnt = clamp_footprint(v, i_min, i_max, j_min, j_max);
                if (cnt) {                                   // then 0 <= min < max <= the image side: all four fit an int
                    L.i_min = (int)i_min; L.i_max = (int)i_max; L.j_min = (int)j_min; L.j_max = (int)j_max;
                }
            }
        }
        locs[i] = L;
        ntiles[i] = cnt;
    }
    count_in_view(ok, n_rendered);
}

__global__ __launch_bounds__(256) void tile_rot_kernel(const RLoc *__restrict__ locs, const unsigned *__restrict__ vals,
                                                       const unsigned *__restrict__ start, const unsigned *__restrict__ end,
                                                       View v, float *__restrict__ image)
{
    __shared__ uint64_t s_tab[PMI_GLIBC_EXP_TABLE_WORDS];
    __shared__ double s_x[CHUNK], s_y[CHUNK], s_norm[CHUNK];
    __shared__ float s_inv00[CHUNK], s_m[CHUNK], s_inv11[CHUNK];
    __shared__ int s_fp[CHUNK][4];       // footprint in image coordinates: i_min, i_max, j_min, j_max
    const int tile = blockIdx.x;
    const unsigned e0 = start[tile], e1 = end[tile];
    const int ty = tile / v.tiles_x, tx = tile - ty * v.tiles_x;
    const int tid = threadIdx.x;
    const int j = tx * TILE + (tid & (TILE - 1));
    const int wave_row0 = ty * TILE + 8 * (tid >> 6);                      // the 8 rows of this wave
    const int row0 = wave_row0 + 4 * ((tid >> 5) & 1);                     // pixels (row0 + k, j), k = 0..3
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    s_tab[tid] = k_rot_exp_tab[tid];                                       // 256 threads, 256 words
    for (unsigned c0 = e0; c0 < e1; c0 += CHUNK) {
        const int nloc = (int)min((unsigned)CHUNK, e1 - c0);
        __syncthreads();                                                   // the chunk before is read; the first time: s_tab
        if (tid < nloc) {
            const RLoc L = locs[vals[c0 + tid]];
            s_x[tid] = L.x; s_y[tid] = L.y; s_norm[tid] = L.norm;
            s_inv00[tid] = L.inv00; s_m[tid] = L.m; s_inv11[tid] = L.inv11;
            s_fp[tid][0] = L.i_min; s_fp[tid][1] = L.i_max; s_fp[tid][2] = L.j_min; s_fp[tid][3] = L.j_max;
        }
        __syncthreads();
        for (int l = 0; l < nloc; l++) {
            const int i_min = s_fp[l][0], i_max = s_fp[l][1];
            if (i_max <= wave_row0 || i_min >= wave_row0 + 8) continue;    // the same in every lane of the wave
            if (j < s_fp[l][2] || j >= s_fp[l][3]) continue;
            const double x = s_x[l], y = s_y[l], norm = s_norm[l];
            const float inv00 = s_inv00[l], m = s_m[l], inv11 = s_inv11[l];
            const float a = (float)((double)j + 0.5 - x);
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const int i = row0 + k;
                if (i >= i_min && i < i_max) {
                    const float b = (float)((double)i + 0.5 - y);
                    const float e = ((a * a) * inv00 + ((a * b) * m)) + (b * b) * inv11;
                    acc[k] = (float)((double)acc[k] + norm * pmi_glibc::exp(-0.5 * (double)e, s_tab));
                }
            }
        }
    }
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int i = row0 + k;
        if (i < v.ny && j < v.nx) image[(int64_t)i * v.nx + j] = acc[k];
    }
}

int make_rot(const double *matrix, const float *matrix_f32, const View &v, int64_t N, Rot *R)
{
    if (!matrix) { set_error("null pointer"); return PMI_ERR_ARG; }
    for (int k = 0; k < 9; k++) { R->m[k] = matrix[k]; R->r[k] = matrix_f32 ? matrix_f32[k] : (float)matrix[k]; }
    R->cx = v.x_min + (v.x_max - v.x_min) / 2;
    R->cy = v.y_min + (v.y_max - v.y_min) / 2;
    R->one_row = N == 1;
    return PMI_OK;
}

}  // namespace

}  // namespace rend
}  // namespace pmi

extern "C" {

int pmi_rotate_locs_dev(const void *d_x, const void *d_y, const void *d_z, int coords_f64, int64_t N, const double *matrix,
                        double oversampling, double y_min, double x_min, double y_max, double x_max, double *d_xr,
                        double *d_yr, double *d_zr, uint8_t *d_in_view, void *stream)
{
    using namespace pmi;
    rend::View v = {};
    v.oversampling = oversampling; v.y_min = y_min; v.x_min = x_min; v.y_max = y_max; v.x_max = x_max;
    rend::Rot R;
    int rc = rend::make_rot(matrix, nullptr, v, N, &R);
    if (rc != PMI_OK) return rc;
    if (N < 0) { set_error("render: negative row count"); return PMI_ERR_ARG; }
    if (N == 0) return PMI_OK;
    if (!d_x || !d_y || !d_z || !d_xr || !d_yr || !d_zr || !d_in_view) { set_error("null pointer"); return PMI_ERR_ARG; }
    hipStream_t s = (hipStream_t)stream;
    if (coords_f64)
        PMI_LAUNCH(rend::rotate_kernel<double>, N, s, (const double *)d_x, (const double *)d_y, (const double *)d_z, N, v, R, d_xr,
                   d_yr, d_zr, d_in_view);
    else
        PMI_LAUNCH(rend::rotate_kernel<float>, N, s, (const float *)d_x, (const float *)d_y, (const float *)d_z, N, v, R, d_xr,
                   d_yr, d_zr, d_in_view);
    return PMI_OK;
}

int pmi_render_hist_rot_dev(const void *d_x, const void *d_y, const void *d_z, int coords_f64, int64_t N,
                            const double *matrix, double oversampling, double y_min, double x_min, double y_max,
                            double x_max, float *d_image, int64_t ny, int64_t nx, int64_t *d_n_rendered, void *stream)
{
    using namespace pmi;
    rend::View v;
    int rc = rend::make_view(oversampling, y_min, x_min, y_max, x_max, 0.0, ny, nx, &v);
    if (rc != PMI_OK) return rc;
    rend::Rot R;
    if ((rc = rend::make_rot(matrix, nullptr, v, N, &R)) != PMI_OK) return rc;
    if (N < 0) { set_error("render: negative row count"); return PMI_ERR_ARG; }
    if (!d_image || !d_n_rendered || (N > 0 && (!d_x || !d_y || !d_z))) { set_error("null pointer"); return PMI_ERR_ARG; }
    hipStream_t s = (hipStream_t)stream;
    PMI_HIP(hipMemsetAsync(d_image, 0, (size_t)ny * nx * sizeof(float), s));
    PMI_HIP(hipMemsetAsync(d_n_rendered, 0, 8, s));
    if (N == 0) return PMI_OK;
    if (coords_f64)
        PMI_LAUNCH(rend::hist_rot_kernel<double>, N, s, (const double *)d_x, (const double *)d_y, (const double *)d_z, N, v, R,
                   d_image, (unsigned long long *)d_n_rendered);
    else
        PMI_LAUNCH(rend::hist_rot_kernel<float>, N, s, (const float *)d_x, (const float *)d_y, (const float *)d_z, N, v, R,
                   d_image, (unsigned long long *)d_n_rendered);
    return PMI_OK;
}

int pmi_render_gaussian_rot_dev(const void *d_x, const void *d_y, const void *d_z, int coords_f64, const float *d_lpx,
                                const float *d_lpy, const float *d_lpz, int64_t N, const double *matrix,
                                const float *matrix_f32, double oversampling, double y_min, double x_min, double y_max,
                                double x_max, double min_blur_width, int iso, float *d_image, int64_t ny, int64_t nx,
                                int64_t *d_n_rendered, void *stream)
{
    using namespace pmi;
    rend::View v;
    int rc = rend::make_view(oversampling, y_min, x_min, y_max, x_max, min_blur_width, ny, nx, &v);
    if (rc != PMI_OK) return rc;
    v.iso = iso ? 1 : 0;
    rend::Rot R;
    if (!matrix_f32) { set_error("null pointer"); return PMI_ERR_ARG; }
    if ((rc = rend::make_rot(matrix, matrix_f32, v, N, &R)) != PMI_OK) return rc;
    if (N < 0 || N > 0x7fffffffLL) { set_error("render: too many localizations"); return PMI_ERR_ARG; }
    if (!d_image || !d_n_rendered || (N > 0 && (!d_x || !d_y || !d_z || !d_lpx || !d_lpy))) { set_error("null pointer"); return PMI_ERR_ARG; }
    hipStream_t s = (hipStream_t)stream;
    return rend::gaussian<rend::RLoc>(N, v, d_image, d_n_rendered, s, [&](rend::RLoc *locs, unsigned *ntiles, unsigned long long *n_rendered) {
        if (coords_f64)
            PMI_LAUNCH(rend::prep_rot_kernel<double>, N, s, (const double *)d_x, (const double *)d_y, (const double *)d_z, d_lpx,
                       d_lpy, d_lpz, N, v, R, locs, ntiles, n_rendered);
        else
            PMI_LAUNCH(rend::prep_rot_kernel<float>, N, s, (const float *)d_x, (const float *)d_y, (const float *)d_z, d_lpx,
                       d_lpy, d_lpz, N, v, R, locs, ntiles, n_rendered);
        return (int)PMI_OK;
    }, rend::tile_rot_kernel);
}

// Host forms: columns and results are staged in the library's scratch (render_common.h), the results copied back.
// The coordinate columns of a rotated host form, of 4 or 8 bytes per value, named to `st`.
static int rot_stage(pmi::Staged &st, const void *x, const void *y, const void *z, int coords_f64, int64_t N, char *(&d)[3])
{
    using namespace pmi;
    if (pmi_device_count() < 1) { set_error("no HIP device"); return PMI_ERR_NODEVICE; }
    if (N < 0 || (N > 0 && (!x || !y || !z))) { set_error("null pointer"); return PMI_ERR_ARG; }
    const size_t bytes = (size_t)N * (coords_f64 ? 8 : 4);
    st.add(d[0], bytes, x), st.add(d[1], bytes, y), st.add(d[2], bytes, z);
    return PMI_OK;
}

int pmi_rotate_locs(const void *x, const void *y, const void *z, int coords_f64, int64_t N, const double *matrix,
                    double oversampling, double y_min, double x_min, double y_max, double x_max, double *xr, double *yr,
                    double *zr, uint8_t *in_view)
{
    using namespace pmi;
    Staged st(SCR_STAGE_A);
    char *d[3] = {nullptr, nullptr, nullptr};
    int rc = rot_stage(st, x, y, z, coords_f64, N, d);
    if (rc != PMI_OK) return rc;
    if (N > 0 && (!xr || !yr || !zr || !in_view)) { set_error("null pointer"); return PMI_ERR_ARG; }
    double *dxr = nullptr, *dyr = nullptr, *dzr = nullptr;
    uint8_t *dv = nullptr;
    st.add(dxr, N, nullptr, xr), st.add(dyr, N, nullptr, yr), st.add(dzr, N, nullptr, zr), st.add(dv, N, nullptr, in_view);
    if ((rc = st.place()) != PMI_OK) return rc;
    rc = pmi_rotate_locs_dev(d[0], d[1], d[2], coords_f64, N, matrix, oversampling, y_min, x_min, y_max, x_max, dxr, dyr, dzr, dv,
                             nullptr);
    return rc != PMI_OK ? rc : st.fetch();
}

static int render_rot_host(const void *x, const void *y, const void *z, int coords_f64, const float *lpx, const float *lpy,
                           const float *lpz, int64_t N, const double *matrix, const float *matrix_f32, double oversampling,
                           double y_min, double x_min, double y_max, double x_max, double min_blur_width, int iso,
                           bool gaussian, float *image, int64_t ny, int64_t nx, int64_t *n_rendered)
{
    using namespace pmi;
    if (!image || !n_rendered || (gaussian && N > 0 && (!lpx || !lpy))) { set_error("null pointer"); return PMI_ERR_ARG; }
    int rc = rend::check_image("render", ny, nx);
    if (rc != PMI_OK) return rc;
    Staged st(SCR_STAGE_A);
    char *d[3] = {nullptr, nullptr, nullptr};
    if ((rc = rot_stage(st, x, y, z, coords_f64, N, d)) != PMI_OK) return rc;
    float *dlx = nullptr, *dly = nullptr, *dlz = nullptr, *d_img = nullptr;
    int64_t *dn = nullptr;
    st.add(dlx, N, lpx), st.add(dly, N, lpy);
    if (lpz) st.add(dlz, N, lpz);
    st.add(d_img, (size_t)ny * nx, nullptr, image), st.add(dn, 1, nullptr, n_rendered);
    if ((rc = st.place()) != PMI_OK) return rc;
    rc = gaussian ? pmi_render_gaussian_rot_dev(d[0], d[1], d[2], coords_f64, dlx, dly, dlz, N, matrix, matrix_f32, oversampling,
                                                y_min, x_min, y_max, x_max, min_blur_width, iso, d_img, ny, nx, dn, nullptr)
                  : pmi_render_hist_rot_dev(d[0], d[1], d[2], coords_f64, N, matrix, oversampling, y_min, x_min, y_max, x_max,
                                            d_img, ny, nx, dn, nullptr);
    return rc != PMI_OK ? rc : st.fetch();
}

int pmi_render_hist_rot(const void *x, const void *y, const void *z, int coords_f64, int64_t N, const double *matrix,
                        double oversampling, double y_min, double x_min, double y_max, double x_max, float *image,
                        int64_t ny, int64_t nx, int64_t *n_rendered)
{
    return render_rot_host(x, y, z, coords_f64, nullptr, nullptr, nullptr, N, matrix, nullptr, oversampling, y_min, x_min,
                           y_max, x_max, 0.0, 0, false, image, ny, nx, n_rendered);
}

int pmi_render_gaussian_rot(const void *x, const void *y, const void *z, int coords_f64, const float *lpx, const float *lpy,
                            const float *lpz, int64_t N, const double *matrix, const float *matrix_f32, double oversampling,
                            double y_min, double x_min, double y_max, double x_max, double min_blur_width, int iso,
                            float *image, int64_t ny, int64_t nx, int64_t *n_rendered)
{
    return render_rot_host(x, y, z, coords_f64, lpx, lpy, lpz, N, matrix, matrix_f32, oversampling, y_min, x_min, y_max,
                           x_max, min_blur_width, iso, true, image, ny, nx, n_rendered);
}

}  // extern "C"
