// rows_common.h — what the kernels over a resident localization table share: launch shape, bisection, union-find, the
// rocPRIM sorts and scan (and the two passes of any rocPRIM call), the argument checks of a row table
// and the dispatch over the x / y element types.  Included by aim, link, cluster, knn, frc and fiducials directly; centers, kinetics, combine, areas and average through rows_groups.h, the
// layer for tables ordered by a label column; pairs, picks and similar through rows_blocks.h, the layer for tables in
// block order; render, render_rot and blur through render_common.h, the layer of the image kernels, which takes the
// sort and the scan from here.  It pulls in rocPRIM: the fit kernels do not pay for it, so the scratch arena and the
// staging of the host forms, which they use too, live in pmi_common.h.
#pragma once
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#include "pmi_common.h"

namespace pmi {
namespace rows {

constexpr int BLOCK = 256;

static inline unsigned blocks(int64_t n) { return (unsigned)((n + BLOCK - 1) / BLOCK); }

// one lane per row of `count`, on `stream`; a kernel name with a comma goes in parentheses
#define PMI_LAUNCH(kernel, count, stream, ...)                                                    \
    do {                                                                                          \
        kernel<<<pmi::rows::blocks(count), pmi::rows::BLOCK, 0, stream>>>(__VA_ARGS__);           \
        PMI_HIP(hipGetLastError());                                                               \
    } while (0)

// first position in [from, n) of the sorted array that is >= v: at most 40 halvings for n < 2^31
template <typename T>
__device__ __forceinline__ int32_t lower_bound(const T *__restrict__ a, int32_t from, int32_t n, T v)
{
    int32_t lo = from, hi = n;
    for (int it = 0; it < 40 && lo < hi; ++it) {
        const int32_t mid = lo + ((hi - lo) >> 1);
        if (a[mid] < v) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// Union-find over rows.  parent[] starts as the identity (iota_kernel); unions may run concurrently from any lane of
// the device, reads of roots come in a later kernel.
__device__ __forceinline__ int32_t find_root(const int32_t *parent, int32_t v, int32_t n)
{
    // a parent is always a lower row: at most n steps
    for (int32_t it = 0; it < n; ++it) {
        const int32_t p = __hip_atomic_load(parent + v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (p == v) return v;
        v = p;
    }
    return v;
}

// status[0] is set when a union did not settle
__device__ __forceinline__ void unite(int32_t *parent, int32_t a, int32_t b, int32_t n, int32_t *status)
{
    for (int32_t it = 0; it < n; ++it) {
        a = find_root(parent, a, n);
        b = find_root(parent, b, n);
        if (a == b) return;
        const int32_t low = min(a, b), high = max(a, b);
        if (atomicCAS(parent + high, high, low) == high) return;
    }
    atomicExch(status, 1);
}

// static: each of the including sources registers its own copy
static __global__ void iota_kernel(int32_t *a, int32_t *b /* may be null */, int32_t n)
{
    const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    a[i] = (int32_t)i;
    if (b) b[i] = (int32_t)i;
}

// ---- host ------------------------------------------------------------------------------------------------------
// the scratch arena of pmi_common.h, under the names the row layers use
using pmi::Arena;
using pmi::carve;

// the bits a radix sort needs for keys 0 .. top: at least one
static int bits_of(uint64_t top)
{
    int bits = 1;
    while (bits < 64 && (top >> bits)) bits++;
    return bits;
}

// The two passes of a rocPRIM call, call(void *tmp, size_t &bytes) -> hipError_t: without a temporary it only says how
// many bytes it wants; they come from SCR_STAGE_B, which no arena of these modules is carved from.
template <typename Call>
static int two_pass(Call &&call)
{
    size_t bytes = 0;
    PMI_HIP(call(nullptr, bytes));
    void *tmp = nullptr;
    const int rc = scratch(SCR_STAGE_B, bytes + 64, &tmp);
    if (rc != PMI_OK) return rc;
    PMI_HIP(call(tmp, bytes));
    return PMI_OK;
}

// Stable radix sorts on the key bits [begin, begin + bits).
template <typename K, typename V>
static int sort_pairs(K *keys, K *keys_out, V *vals, V *vals_out, size_t n, int bits, hipStream_t stream, int begin = 0)
{
    return two_pass([&](void *tmp, size_t &bytes) {
        return rocprim::radix_sort_pairs(tmp, bytes, keys, keys_out, vals, vals_out, n, begin, begin + bits, stream);
    });
}

template <typename K>
static int sort_keys(K *keys, K *keys_out, size_t n, int bits, hipStream_t stream)
{
    return two_pass([&](void *tmp, size_t &bytes) {
        return rocprim::radix_sort_keys(tmp, bytes, keys, keys_out, n, 0, bits, stream);
    });
}

// out[i] = flag[0] + ... + flag[i - 1].  F is uint32_t or const uint32_t; a template, like the sorts, so that a source
// that does not scan carries no scan kernels.
template <typename F>
static int exclusive_scan_u32(F *flag, uint32_t *out, size_t n, hipStream_t stream)
{
    return two_pass([&](void *tmp, size_t &bytes) {
        return rocprim::exclusive_scan(tmp, bytes, flag, out, 0u, n, rocprim::plus<uint32_t>(), stream);
    });
}

// n rows, indexed with int32, in n_groups runs that `unit` names in the message (no unit: a call without runs)
static int check_rows(const char *what, int64_t n, int64_t n_groups = 0, const char *unit = nullptr)
{
    if (n < 0 || n > INT32_MAX - 1 || n_groups < 0 || n_groups > n) {
        if (unit)
            set_error("%s: %lld rows, %lld %s (rows are indexed with int32)", what, (long long)n, (long long)n_groups, unit);
        else
            set_error("%s: %lld rows (this kernel indexes rows with int32)", what, (long long)n);
        return PMI_ERR_ARG;
    }
    return PMI_OK;
}

// x / y type codes of pmi_link_type
static int check_xy(const char *what, int x_type, int y_type)
{
    if ((x_type != PMI_LINK_F32 && x_type != PMI_LINK_F64) || (y_type != PMI_LINK_F32 && y_type != PMI_LINK_F64)) {
        set_error("%s: x / y must be float32 or float64 (codes %d, %d)", what, x_type, y_type);
        return PMI_ERR_ARG;
    }
    return PMI_OK;
}

// fn<TX, TY>((const TX *)d_x, (const TY *)d_y, ...) for the checked codes x_type / y_type of the exported function it
// stands in
#define PMI_XY_DISPATCH(fn, ...)                                                                             \
    (x_type == PMI_LINK_F32                                                                                  \
         ? (y_type == PMI_LINK_F32 ? fn<float, float>((const float *)d_x, (const float *)d_y, __VA_ARGS__)   \
                                   : fn<float, double>((const float *)d_x, (const double *)d_y, __VA_ARGS__)) \
         : (y_type == PMI_LINK_F32 ? fn<double, float>((const double *)d_x, (const float *)d_y, __VA_ARGS__) \
                                   : fn<double, double>((const double *)d_x, (const double *)d_y, __VA_ARGS__)))

}  // namespace rows
}  // namespace pmi
