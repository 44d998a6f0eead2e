// average.hip — the alignment step of picasso.average (picasso/average.py:49-118 align_group_core, :459-468 the
// average image), choice for choice.  The arithmetic, the index map of fftshift and the order of the candidates are
// in average_core.h, which also compiles for the host.
//
// image_kernel   render_hist_numba of the whole table: one lane per row, int32 counts by integer atomics.
// align_kernel   one workgroup per (group, chunk of the angle list).  Per angle the lanes rotate the group's rows with
//                the host's cos / sin tables and write the packed pixels of the rows in view into LDS; then every lane
//                takes shifts f = t, t + BLOCK, ... of the fftshifted correlation in flat order and sums
//                avg[(pixel - shift) mod n] over the list: consecutive lanes read consecutive LDS words (one wrap per
//                row), the list entry is a broadcast.  A group of more than PMI_AVERAGE_LIST rows is taken in tiles of
//                the list, rebuilt for each batch of BLOCK shifts (8 rotations a lane against 2048 gathers).  Each lane
//                keeps its best candidate; one tree reduction at the end writes (value, angle, flat) per workgroup.
//                The average image is copied to LDS when it has at most PMI_AVERAGE_LDS_BINS pixels (64 KiB + 8 KiB of
//                list + 3 KiB: two workgroups per CU; 16 KiB when it has at most 4096 pixels: five workgroups per CU),
//                else read from global memory; the integers are the same.
// apply_kernel   one workgroup per group: the chunks reduced in the same order, the shifts and the rotation of the
//                choice applied in float64 and stored as float32.
//
// Every loop is bounded by the rows of the group, the pixels of the image or the angles of the chunk; every index into
// the image is below n * n (average_core.h), every index into the list below PMI_AVERAGE_LIST.  No contraction.
#include "rows_groups.h"
#include "average_core.h"

#pragma clang fp contract(off)

namespace pmi {
namespace average {

using namespace rows;

constexpr int LDS_BINS = PMI_AVERAGE_LDS_BINS;
constexpr int SMALL_BINS = 4096;      // the usual image (28 x 28 at the defaults): 16 KiB, five workgroups per CU
constexpr int LIST = PMI_AVERAGE_LIST;
static_assert(PMI_AVERAGE_MAX_PIXELS <= 32768, "a pixel index must fit 16 bits, n * n an int32");
static_assert(2 * (4 * LDS_BINS + 4 * LIST + 4 * 1024) <= 160 * 1024, "two workgroups of the LDS path per CU");

__global__ __launch_bounds__(BLOCK) void image_kernel(const float *__restrict__ x, const float *__restrict__ y,
                                                      int32_t n_rows, Geom geom, int32_t *__restrict__ image,
                                                      int32_t *__restrict__ dropped)
{
    const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n_rows) return;
    const float xv = x[i], yv = y[i];
    if (!in_view((double)xv, (double)yv, geom)) return;
    const int32_t px = pixel32(xv, geom), py = pixel32(yv, geom);
    if ((uint32_t)px >= (uint32_t)geom.n || (uint32_t)py >= (uint32_t)geom.n) {
        atomicAdd(dropped, 1);
        return;
    }
    atomicAdd(image + py * geom.n + px, 1);
}

template <int BINS>      // of the LDS copy of the image; 0: the image is read from global memory
__global__ __launch_bounds__(BLOCK) void align_kernel(const float *__restrict__ x, const float *__restrict__ y,
                                                      const int32_t *__restrict__ rows, const int32_t *__restrict__ start,
                                                      int32_t n_rows, int32_t n_groups, Geom geom,
                                                      const double *__restrict__ cosv, const double *__restrict__ sinv,
                                                      int32_t n_angles, int32_t chunks, int32_t per_chunk,
                                                      const int32_t *__restrict__ image, int32_t *__restrict__ parts,
                                                      int32_t *__restrict__ dropped)
{
    constexpr bool LDS = BINS > 0;
    __shared__ int32_t s_img[LDS ? BINS : 1];
    __shared__ uint32_t s_list[LIST];
    __shared__ int32_t s_val[BLOCK], s_ang[BLOCK], s_flat[BLOCK];
    __shared__ int32_t s_cnt;
    const int32_t t = threadIdx.x;
    const int32_t g = blockIdx.x / chunks, c = blockIdx.x - g * chunks;
    if (g >= n_groups) return;
    const int32_t n = geom.n, nn = n * n;
    if (LDS && nn > BINS) return;         // uniform: the host sends such an image down the other path
    int32_t a, b;
    run_of(start, g, n_rows, &a, &b);
    const int32_t *img = image;
    if (LDS) {
        for (int32_t i = t; i < nn; i += BLOCK) s_img[i] = image[i];
        img = s_img;
    }
    const int32_t tiles = (b - a + LIST - 1) / LIST;
    const int32_t a0 = c * per_chunk, a1 = min(n_angles, a0 + per_chunk);

    // the packed pixels of the rows [lo, hi) in view, hi - lo <= LIST, in any order: the sums are integer
    auto build = [&](int32_t lo, int32_t hi, double cs, double sn) {
        __syncthreads();      // nobody still reads the list (nor, the first time, writes the image)
        if (t == 0) s_cnt = 0;
        __syncthreads();
        for (int32_t p = lo + t; p < hi; p += BLOCK) {
            const int32_t i = rows[p];
            if (!row_ok(i, n_rows)) continue;
            uint32_t packed;
            const int what = rotate_bin(x[i], y[i], cs, sn, geom, &packed);
            if (what == 1) {
                const int32_t k = atomicAdd(&s_cnt, 1);
                if (k < LIST) s_list[k] = packed;
            } else if (what == 2) {
                atomicAdd(dropped, 1);
            }
        }
        __syncthreads();
    };

    Best best = none();
    for (int32_t ai = a0; ai < a1; ++ai) {
        const double cs = cosv[ai], sn = sinv[ai];
        if (tiles <= 1) build(a, b, cs, sn);
        for (int32_t f0 = 0; f0 < nn; f0 += BLOCK) {
            const int32_t f = f0 + t;
            const int32_t iy = f / n, ix = f - iy * n;
            const int32_t sy = unshift(iy, n), sx = unshift(ix, n);
            int32_t acc = 0;
            if (tiles <= 1) {
                if (f < nn) acc = gather(img, s_list, min(s_cnt, LIST), n, sy, sx);
            } else {
                for (int32_t lo = a; lo < b; lo += LIST) {
                    build(lo, min(b, lo + LIST), cs, sn);
                    if (f < nn) acc += gather(img, s_list, min(s_cnt, LIST), n, sy, sx);
                }
            }
            if (f < nn && better(acc, ai, f, best)) best = Best{acc, ai, f};
        }
    }

    __syncthreads();
    s_val[t] = best.value, s_ang[t] = best.angle, s_flat[t] = best.flat;
    __syncthreads();
    for (int w = BLOCK / 2; w > 0; w >>= 1) {
        if (t < w && better(s_val[t + w], s_ang[t + w], s_flat[t + w], Best{s_val[t], s_ang[t], s_flat[t]}))
            s_val[t] = s_val[t + w], s_ang[t] = s_ang[t + w], s_flat[t] = s_flat[t + w];
        __syncthreads();
    }
    if (t == 0) {
        int32_t *out = parts + 3 * (int64_t)blockIdx.x;
        out[0] = s_val[0], out[1] = s_ang[0], out[2] = s_flat[0];
    }
}

__global__ __launch_bounds__(BLOCK) void apply_kernel(const float *__restrict__ x, const float *__restrict__ y,
                                                      const int32_t *__restrict__ rows, const int32_t *__restrict__ start,
                                                      int32_t n_rows, int32_t n_groups, Geom geom,
                                                      const double *__restrict__ cosv, const double *__restrict__ sinv,
                                                      int32_t n_angles, const int32_t *__restrict__ parts, int32_t chunks,
                                                      int32_t *__restrict__ choice, float *__restrict__ x_out,
                                                      float *__restrict__ y_out)
{
    __shared__ Best s_best;
    const int32_t g = blockIdx.x, t = threadIdx.x;
    if (g >= n_groups) return;
    if (t == 0) {
        Best best = none();
        for (int32_t c = 0; c < chunks; ++c) {
            const int32_t *p = parts + 3 * ((int64_t)g * chunks + c);
            if (better(p[0], p[1], p[2], best)) best = Best{p[0], p[1], p[2]};
        }
        // a choice is an angle of the list and a pixel of the image, or none
        if (best.value <= 0 || best.angle < 0 || best.angle >= n_angles || best.flat < 0 || best.flat >= geom.n * geom.n)
            best = none();
        s_best = best;
        choice[3 * g] = best.value, choice[3 * g + 1] = best.angle, choice[3 * g + 2] = best.flat;
    }
    __syncthreads();
    const Best best = s_best;
    double cs = 1.0, sn = 0.0, dx = 0.0, dy = 0.0;      // rot = 0.0: np.cos gives 1.0, np.sin 0.0
    if (best.angle >= 0) {
        cs = cosv[best.angle], sn = sinv[best.angle];
        dy = shift_of(best.flat / geom.n, geom);
        dx = shift_of(best.flat % geom.n, geom);
    }
    int32_t a, b;
    run_of(start, g, n_rows, &a, &b);
    for (int32_t p = a + t; p < b; p += BLOCK) {
        const int32_t i = rows[p];
        if (!row_ok(i, n_rows)) continue;
        transform(x[i], y[i], cs, sn, dx, dy, x_out + i, y_out + i);
    }
}

static int check(const char *what, const void *d_x, const void *d_y, int64_t n, int64_t n_pixel, double t_min, double t_max,
                 double ov)
{
    if (n < 0 || n > INT32_MAX - 1 || (n > 0 && (!d_x || !d_y))) {
        set_error("%s: %lld rows (rows are indexed with int32), or a NULL column", what, (long long)n);
        return PMI_ERR_ARG;
    }
    if (n_pixel < 1 || n_pixel > PMI_AVERAGE_MAX_PIXELS || !(t_min < t_max) || !(ov > 0.0) || ov - ov != 0.0) {
        set_error("%s: an image of %lld pixels per axis (1 .. %d), a view (%g, %g), an oversampling of %g", what,
                  (long long)n_pixel, PMI_AVERAGE_MAX_PIXELS, t_min, t_max, ov);
        return PMI_ERR_ARG;
    }
    return PMI_OK;
}

static int check_groups(const char *what, const int32_t *d_rows, const int32_t *d_start, int64_t n, int64_t n_groups,
                        const double *d_cos, const double *d_sin, int64_t n_angles, int64_t chunks)
{
    if (n_groups < 0 || n_groups > n || (n > 0 && (!d_rows || !d_start)) || n_angles < 0 || n_angles > INT32_MAX / 2 ||
        (n_angles > 0 && (!d_cos || !d_sin)) || chunks < 1 || chunks > 65536 || n_groups * chunks > INT32_MAX / 4) {
        set_error("%s: %lld groups of %lld rows, %lld angles in %lld chunks, or a NULL table", what, (long long)n_groups,
                  (long long)n, (long long)n_angles, (long long)chunks);
        return PMI_ERR_ARG;
    }
    return PMI_OK;
}

}  // namespace average
}  // namespace pmi

using namespace pmi;

extern "C" {

int pmi_average_limits(int *lds_bins, int *list, int *max_pixels)
{
    if (lds_bins) *lds_bins = PMI_AVERAGE_LDS_BINS;
    if (list) *list = PMI_AVERAGE_LIST;
    if (max_pixels) *max_pixels = PMI_AVERAGE_MAX_PIXELS;
    return PMI_OK;
}

int pmi_average_image_dev(const float *d_x, const float *d_y, int64_t n, int64_t n_pixel, double t_min, double t_max,
                          double oversampling, int sub_f32, int mul_f32, int32_t *d_image, int32_t *d_dropped, void *stream)
{
    int rc = average::check("pmi_average_image_dev", d_x, d_y, n, n_pixel, t_min, t_max, oversampling);
    if (rc) return rc;
    if (!d_image || !d_dropped) {
        set_error("pmi_average_image_dev: NULL output");
        return PMI_ERR_ARG;
    }
    hipStream_t s = (hipStream_t)stream;
    const average::Geom geom{t_min, t_max, oversampling, (int32_t)n_pixel, sub_f32 != 0, mul_f32 != 0};
    PMI_HIP(hipMemsetAsync(d_image, 0, sizeof(int32_t) * (size_t)(n_pixel * n_pixel), s));
    PMI_HIP(hipMemsetAsync(d_dropped, 0, sizeof(int32_t), s));
    if (n > 0) PMI_LAUNCH(average::image_kernel, n, s, d_x, d_y, (int32_t)n, geom, d_image, d_dropped);
    PMI_HIP(hipStreamSynchronize(s));
    return PMI_OK;
}

int pmi_average_align_dev(const float *d_x, const float *d_y, const int32_t *d_rows, const int32_t *d_start, int64_t n,
                          int64_t n_groups, int64_t n_pixel, double t_min, double t_max, double oversampling,
                          const double *d_cos, const double *d_sin, int64_t n_angles, int64_t chunks,
                          const int32_t *d_image, int use_lds, int32_t *d_parts, int32_t *d_dropped, void *stream)
{
    int rc = average::check("pmi_average_align_dev", d_x, d_y, n, n_pixel, t_min, t_max, oversampling);
    if (!rc) rc = average::check_groups("pmi_average_align_dev", d_rows, d_start, n, n_groups, d_cos, d_sin, n_angles, chunks);
    if (rc) return rc;
    if (!d_image || !d_dropped || (n_groups > 0 && !d_parts) || (use_lds && n_pixel * n_pixel > PMI_AVERAGE_LDS_BINS)) {
        set_error("pmi_average_align_dev: a NULL table, or an image of %lld pixels on the LDS path", (long long)(n_pixel * n_pixel));
        return PMI_ERR_ARG;
    }
    hipStream_t s = (hipStream_t)stream;
    PMI_HIP(hipMemsetAsync(d_dropped, 0, sizeof(int32_t), s));
    if (n_groups > 0) {
        const average::Geom geom{t_min, t_max, oversampling, (int32_t)n_pixel, 0, 0};
        const int32_t per_chunk = (int32_t)((n_angles + chunks - 1) / chunks);
        const unsigned grid = (unsigned)(n_groups * chunks);
        if (use_lds && n_pixel * n_pixel <= average::SMALL_BINS)
            average::align_kernel<average::SMALL_BINS><<<grid, rows::BLOCK, 0, s>>>(
                d_x, d_y, d_rows, d_start, (int32_t)n, (int32_t)n_groups, geom, d_cos, d_sin, (int32_t)n_angles,
                (int32_t)chunks, per_chunk, d_image, d_parts, d_dropped);
        else if (use_lds)
            average::align_kernel<average::LDS_BINS><<<grid, rows::BLOCK, 0, s>>>(
                d_x, d_y, d_rows, d_start, (int32_t)n, (int32_t)n_groups, geom, d_cos, d_sin, (int32_t)n_angles,
                (int32_t)chunks, per_chunk, d_image, d_parts, d_dropped);
        else
            average::align_kernel<0><<<grid, rows::BLOCK, 0, s>>>(
                d_x, d_y, d_rows, d_start, (int32_t)n, (int32_t)n_groups, geom, d_cos, d_sin, (int32_t)n_angles,
                (int32_t)chunks, per_chunk, d_image, d_parts, d_dropped);
        PMI_HIP(hipGetLastError());
    }
    PMI_HIP(hipStreamSynchronize(s));
    return PMI_OK;
}

int pmi_average_apply_dev(const float *d_x, const float *d_y, const int32_t *d_rows, const int32_t *d_start, int64_t n,
                          int64_t n_groups, int64_t n_pixel, double oversampling, const double *d_cos, const double *d_sin,
                          int64_t n_angles, const int32_t *d_parts, int64_t chunks, int32_t *d_choice, float *d_x_out,
                          float *d_y_out, void *stream)
{
    int rc = average::check("pmi_average_apply_dev", d_x, d_y, n, n_pixel, 0.0, 1.0, oversampling);
    if (!rc) rc = average::check_groups("pmi_average_apply_dev", d_rows, d_start, n, n_groups, d_cos, d_sin, n_angles, chunks);
    if (rc) return rc;
    if (n_groups > 0 && (!d_parts || !d_choice || !d_x_out || !d_y_out)) {
        set_error("pmi_average_apply_dev: NULL table");
        return PMI_ERR_ARG;
    }
    hipStream_t s = (hipStream_t)stream;
    if (n_groups > 0) {
        const average::Geom geom{0.0, 0.0, oversampling, (int32_t)n_pixel, 0, 0};
        average::apply_kernel<<<(unsigned)n_groups, rows::BLOCK, 0, s>>>(
            d_x, d_y, d_rows, d_start, (int32_t)n, (int32_t)n_groups, geom, d_cos, d_sin, (int32_t)n_angles, d_parts,
            (int32_t)chunks, d_choice, d_x_out, d_y_out);
        PMI_HIP(hipGetLastError());
    }
    PMI_HIP(hipStreamSynchronize(s));
    return PMI_OK;
}

}  // extern "C"
