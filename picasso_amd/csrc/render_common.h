// render_common.h — what the image kernels share (render.hip: flat view, render_rot.hip: rotated view, blur.hip: the
// image blur): the viewport and the image-size limits, the reference's float -> integer conversions, the clamp and the
// count every prep kernel ends on, and the Gaussian driver with its tile schedule:
//   prep (each view's own kernel), exclusive scan of the per-localization tile counts, emit (tile, localization) pairs in
//   localization order, stable radix sort by tile -> every 32x32 tile gets its localizations in table order, then each
//   tile's [start, end), then the view's own tile kernel.
// A localization record is any struct with the clipped footprint i_min, i_max, j_min, j_max ([min, max), ints).
//
// Scratch slots of the image layer, its lines of the library's table (pmi_common.h, where the rule stands):
//   SCR_STAGE_A   host forms (Staged): pmi_render_hist / _gaussian, pmi_rotate_locs, pmi_render_hist_rot / _gaussian_rot,
//                 pmi_blur, pmi_render_blurred
//   SCR_STAGE_B   rocPRIM temporaries (rows::two_pass) — so no arena of this layer
//   SCR_STAGE_C   gaussian(): records, tile counts, offsets, tile bounds
//   SCR_STAGE_D   pmi_blur_dev: the image between the two passes
//   SCR_RECORDS   tile_lists: the (tile, localization) pairs, unsorted and sorted
// The histogram _dev forms and pmi_rotate_locs_dev take no scratch.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstring>

#include "rows_common.h"

#pragma clang fp contract(off)

namespace pmi {
namespace rend {

constexpr int TILE = 32;
constexpr int CHUNK = 32;          // localizations per LDS batch in the tile kernels

struct View {
    double oversampling, y_min, x_min, y_max, x_max;
    float os_f, min_blur_f;
    int iso;                 // gaussian_iso: both widths = their mean (render.py:1148-1216)
    int64_t ny, nx;
    int tiles_x, tiles_y;
};

__device__ __forceinline__ float np_maxf(float a, float b) { return (a != a) ? a : ((b != b) ? b : (a > b ? a : b)); }

// float64 -> int32 as the reference's compiled code does it on x86-64 (cvttsd2si): truncation, and
// INT_MIN for NaN or out-of-range values — a NaN precision then yields an empty footprint.
__device__ __forceinline__ int32_t to_int32(double v)
{
    return (v != v || v >= 2147483648.0 || v < -2147483648.0) ? (int32_t)0x80000000 : (int32_t)v;
}

// ... and float64 -> int64 (numba's int() of a float64, the 64-bit cvttsd2si): INT64_MIN for NaN or out of range
__device__ __forceinline__ int64_t to_int64(double v)
{
    return (v != v || v >= 9223372036854775808.0 || v < -9223372036854775808.0) ? (int64_t)0x8000000000000000LL : (int64_t)v;
}

// the four bounds as a view converts them, clamped to the image -> the tiles the footprint touches, 0 when it is empty
__device__ __forceinline__ unsigned clamp_footprint(const View &v, int64_t &i_min, int64_t &i_max, int64_t &j_min, int64_t &j_max)
{
    if (i_min < 0) i_min = 0;
    if (i_max > v.ny) i_max = v.ny;
    if (j_min < 0) j_min = 0;
    if (j_max > v.nx) j_max = v.nx;
    if (i_max <= i_min || j_max <= j_min) return 0;
    return (unsigned)(((i_max - 1) / TILE - i_min / TILE + 1) * ((j_max - 1) / TILE - j_min / TILE + 1));
}

// n_rendered += the lanes of the wave whose row is in view; every lane of the workgroup calls it
__device__ __forceinline__ void count_in_view(bool ok, unsigned long long *n_rendered)
{
    const unsigned long long bal = __ballot(ok);
    if ((threadIdx.x & 63) == 0 && bal) atomicAdd(n_rendered, (unsigned long long)__popcll(bal));
}

template <class L>
__global__ void emit_kernel(const L *__restrict__ locs, const unsigned *__restrict__ ntiles,
                            const unsigned *__restrict__ offset, int64_t N, int tiles_x,
                            unsigned *__restrict__ keys, unsigned *__restrict__ vals)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N || ntiles[i] == 0) return;
    const L loc = locs[i];
    unsigned o = offset[i];
    for (int ty = loc.i_min / TILE; ty <= (loc.i_max - 1) / TILE; ty++)
        for (int tx = loc.j_min / TILE; tx <= (loc.j_max - 1) / TILE; tx++) {
            keys[o] = (unsigned)(ty * tiles_x + tx);
            vals[o] = (unsigned)i;
            o++;
        }
}

static __global__ void tile_bounds_kernel(const unsigned *__restrict__ keys, unsigned E, unsigned *__restrict__ start,
                                          unsigned *__restrict__ end)
{
    const unsigned e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= E) return;
    const unsigned k = keys[e];
    if (e == 0 || keys[e - 1] != k) start[k] = e;
    if (e + 1 == E || keys[e + 1] != k) end[k] = e + 1;
}

// (n_y, n_x) of a render (render.py:224-225)
static void view_dims(double oversampling, double y_min, double x_min, double y_max, double x_max, int64_t *ny, int64_t *nx)
{
    *ny = (int64_t)std::ceil(oversampling * (y_max - y_min));
    *nx = (int64_t)std::ceil(oversampling * (x_max - x_min));
}

// sides of 1 ... 2^31 - 1 and at most 2^31 - 1 tiles of 32 x 32 pixels; `what` heads the message
static int check_image(const char *what, int64_t ny, int64_t nx)
{
    if (ny <= 0 || nx <= 0 || ny > 0x7fffffff || nx > 0x7fffffff) { set_error("%s: bad image size %lld x %lld", what, (long long)ny, (long long)nx); return PMI_ERR_ARG; }
    if (((ny + TILE - 1) / TILE) * ((nx + TILE - 1) / TILE) > 0x7fffffffLL) { set_error("%s: image too large", what); return PMI_ERR_ARG; }
    return PMI_OK;
}

static int make_view(double oversampling, double y_min, double x_min, double y_max, double x_max, double min_blur,
                     int64_t ny, int64_t nx, View *v)
{
    int64_t ey, ex;
    view_dims(oversampling, y_min, x_min, y_max, x_max, &ey, &ex);
    if (ny != ey || nx != ex) { set_error("render: image is %lld x %lld but the viewport needs %lld x %lld", (long long)ny, (long long)nx, (long long)ey, (long long)ex); return PMI_ERR_ARG; }
    const int rc = check_image("render", ny, nx);
    if (rc != PMI_OK) return rc;
    v->oversampling = oversampling; v->y_min = y_min; v->x_min = x_min; v->y_max = y_max; v->x_max = x_max;
    v->os_f = (float)oversampling; v->min_blur_f = (float)min_blur; v->iso = 0;
    v->ny = ny; v->nx = nx;
    v->tiles_x = (int)((nx + TILE - 1) / TILE); v->tiles_y = (int)((ny + TILE - 1) / TILE);
    return PMI_OK;
}

// Behind a prep kernel that left locs[N] and ntiles[N] (offset: N entries; start: 2 * ntile entries, the second half
// receives each tile's end): the tile lists.  Synchronises the stream once, the number of pairs *E sizes the sort buffers; with *E == 0 nothing is
// listed and *vals is not set.  start / end of a tile without localizations are both 0.
template <class L>
static int tile_lists(const L *locs, const unsigned *ntiles, unsigned *offset, int64_t N, const View &v,
                      unsigned *start, uint64_t *E_out, unsigned **vals_out, hipStream_t s)
{
    int rc;
    const int64_t ntile = (int64_t)v.tiles_x * v.tiles_y;
    // exclusive scan -> offsets; the total decides the size of the pair buffers (one small D2H)
    if ((rc = rows::exclusive_scan_u32(ntiles, offset, (size_t)N, s)) != PMI_OK) return rc;
    unsigned last_off = 0, last_cnt = 0;
    PMI_HIP(hipMemcpyAsync(&last_off, offset + (N - 1), 4, hipMemcpyDeviceToHost, s));
    PMI_HIP(hipMemcpyAsync(&last_cnt, ntiles + (N - 1), 4, hipMemcpyDeviceToHost, s));
    PMI_HIP(hipStreamSynchronize(s));
    const uint64_t E = (uint64_t)last_off + last_cnt;
    if (E > 0x7fffffffULL) { set_error("render: footprints cover %llu tiles in total, more than this kernel handles", (unsigned long long)E); return PMI_ERR_ARG; }
    *E_out = E;

    PMI_HIP(hipMemsetAsync(start, 0, (size_t)ntile * 8, s));
    if (E == 0) return PMI_OK;
    unsigned *keys = nullptr, *vals = nullptr, *keys2 = nullptr, *vals2 = nullptr;
    if ((rc = rows::carve(SCR_RECORDS, [&](rows::Arena &a) {
             keys = a.take<unsigned>(E), vals = a.take<unsigned>(E), keys2 = a.take<unsigned>(E), vals2 = a.take<unsigned>(E);
         })) != PMI_OK)
        return rc;
    PMI_LAUNCH(emit_kernel<L>, N, s, locs, ntiles, offset, N, v.tiles_x, keys, vals);
    if ((rc = rows::sort_pairs(keys, keys2, vals, vals2, (size_t)E, rows::bits_of((uint64_t)ntile - 1), s)) != PMI_OK) return rc;   // stable
    PMI_LAUNCH(tile_bounds_kernel, (int64_t)E, s, keys2, (unsigned)E, start, start + ntile);
    *vals_out = vals2;
    return PMI_OK;
}

// The Gaussian render of either view behind its argument checks.  prep(locs, ntiles, n_rendered) launches the view's prep
// kernel over the N rows; tile_kernel draws one tile from its list.  Synchronises the stream once (tile_lists).
template <class L, class Prep, class TileKernel>
static int gaussian(int64_t N, const View &v, float *d_image, int64_t *d_n_rendered, hipStream_t s, Prep &&prep, TileKernel tile_kernel)
{
    PMI_HIP(hipMemsetAsync(d_n_rendered, 0, 8, s));
    const int64_t ntile = (int64_t)v.tiles_x * v.tiles_y;
    const size_t image_bytes = (size_t)v.ny * v.nx * sizeof(float);
    if (N == 0) { PMI_HIP(hipMemsetAsync(d_image, 0, image_bytes, s)); return PMI_OK; }
    L *locs = nullptr;
    unsigned *ntiles = nullptr, *offset = nullptr, *start = nullptr;
    int rc = rows::carve(SCR_STAGE_C, [&](rows::Arena &a) {
        locs = a.take<L>(N), ntiles = a.take<unsigned>(N), offset = a.take<unsigned>(N), start = a.take<unsigned>(2 * ntile);
    });
    if (rc != PMI_OK) return rc;
    if ((rc = prep(locs, ntiles, (unsigned long long *)d_n_rendered)) != PMI_OK) return rc;
    uint64_t E = 0;
    unsigned *vals = nullptr;
    if ((rc = tile_lists(locs, ntiles, offset, N, v, start, &E, &vals, s)) != PMI_OK) return rc;
    if (E > 0) {
        tile_kernel<<<(unsigned)ntile, 256, 0, s>>>(locs, vals, start, start + ntile, v, d_image);
        PMI_HIP(hipGetLastError());
    } else {
        PMI_HIP(hipMemsetAsync(d_image, 0, image_bytes, s));
    }
    return PMI_OK;
}

}  // namespace rend
}  // namespace pmi
