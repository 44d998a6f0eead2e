// render_common.h — what the Gaussian renders share (render.hip: flat view, render_rot.hip: rotated view): the viewport,
// the reference's float -> integer conversions, and the tile schedule behind each one's own prep kernel:
//   exclusive scan of the per-localization tile counts, emit (tile, localization) pairs in localization order, stable
//   radix sort by tile -> every 32x32 tile gets its localizations in table order, then each tile's [start, end).
// A localization record is any struct with the clipped footprint i_min, i_max, j_min, j_max ([min, max), ints).
#pragma once
#include <algorithm>
#include <cmath>
#include <cstring>

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#include "pmi_common.h"

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

static int make_view(double oversampling, double y_min, double x_min, double y_max, double x_max, double min_blur,
                     int64_t ny, int64_t nx, View *v)
{
    const int64_t ey = (int64_t)std::ceil(oversampling * (y_max - y_min));
    const int64_t ex = (int64_t)std::ceil(oversampling * (x_max - x_min));
    if (ny != ey || nx != ex) { set_error("render: image is %lld x %lld but the viewport needs %lld x %lld", (long long)ny, (long long)nx, (long long)ey, (long long)ex); return PMI_ERR_ARG; }
    if (ny <= 0 || nx <= 0 || ny > 0x7fffffff || nx > 0x7fffffff) { set_error("render: bad image size"); return PMI_ERR_ARG; }
    v->oversampling = oversampling; v->y_min = y_min; v->x_min = x_min; v->y_max = y_max; v->x_max = x_max;
    v->os_f = (float)oversampling; v->min_blur_f = (float)min_blur; v->iso = 0;
    v->ny = ny; v->nx = nx;
    v->tiles_x = (int)((nx + TILE - 1) / TILE); v->tiles_y = (int)((ny + TILE - 1) / TILE);
    if ((int64_t)v->tiles_x * v->tiles_y > 0x7fffffffLL) { set_error("render: image too large"); return PMI_ERR_ARG; }
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
    unsigned *end = start + ntile;
    const unsigned nb = (unsigned)((N + 255) / 256);
    // exclusive scan -> offsets; the total decides the size of the pair buffers (one small D2H)
    size_t tmp_bytes = 0;
    PMI_HIP(rocprim::exclusive_scan(nullptr, tmp_bytes, ntiles, offset, 0u, (size_t)N, rocprim::plus<unsigned>(), s));
    void *p_tmp = nullptr;
    if ((rc = scratch(SCR_STAGE_D, tmp_bytes + 64, &p_tmp)) != PMI_OK) return rc;
    PMI_HIP(rocprim::exclusive_scan(p_tmp, tmp_bytes, ntiles, offset, 0u, (size_t)N, rocprim::plus<unsigned>(), s));
    unsigned last_off = 0, last_cnt = 0;
    PMI_HIP(hipMemcpyAsync(&last_off, offset + (N - 1), 4, hipMemcpyDeviceToHost, s));
    PMI_HIP(hipMemcpyAsync(&last_cnt, ntiles + (N - 1), 4, hipMemcpyDeviceToHost, s));
    PMI_HIP(hipStreamSynchronize(s));
    const uint64_t E = (uint64_t)last_off + last_cnt;
    if (E > 0x7fffffffULL) { set_error("render: footprints cover %llu tiles in total, more than this kernel handles", (unsigned long long)E); return PMI_ERR_ARG; }
    *E_out = E;

    PMI_HIP(hipMemsetAsync(start, 0, (size_t)ntile * 8, s));
    if (E == 0) return PMI_OK;
    void *p_pairs = nullptr;
    if ((rc = scratch(SCR_RECORDS, (size_t)E * 16 + 64, &p_pairs)) != PMI_OK) return rc;
    unsigned *keys = (unsigned *)p_pairs, *vals = keys + E, *keys2 = vals + E, *vals2 = keys2 + E;
    hipLaunchKernelGGL(emit_kernel<L>, dim3(nb), dim3(256), 0, s, locs, ntiles, offset, N, v.tiles_x, keys, vals);
    PMI_HIP(hipGetLastError());
    int bits = 1;
    while ((1LL << bits) < ntile) bits++;
    size_t sort_bytes = 0;
    PMI_HIP(rocprim::radix_sort_pairs(nullptr, sort_bytes, keys, keys2, vals, vals2, (size_t)E, 0, bits, s));
    void *p_sort = nullptr;
    if ((rc = scratch(SCR_RECORDS2, sort_bytes + 64, &p_sort)) != PMI_OK) return rc;
    PMI_HIP(rocprim::radix_sort_pairs(p_sort, sort_bytes, keys, keys2, vals, vals2, (size_t)E, 0, bits, s));   // stable
    hipLaunchKernelGGL(tile_bounds_kernel, dim3((unsigned)((E + 255) / 256)), dim3(256), 0, s, keys2, (unsigned)E, start, end);
    PMI_HIP(hipGetLastError());
    *vals_out = vals2;
    return PMI_OK;
}

}  // namespace rend
}  // namespace pmi
