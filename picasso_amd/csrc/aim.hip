// aim.hip — intersection counting of AIM undrift (Adaptive Intersection Maximization,
// picasso/aim.py:517-659 intersection_max, :662-773 intersection_max_z, :89-126 _count_intersections).
//
// For one segment of target localizations and box^2 (x / y) or box (z) key shifts, the reference counts
//     roi_cc[s] = sum over common keys k of min(c_ref(k), c_target(k - shift_s))
// with np.unique + a stable argsort per shift.  Here the reference keys are counted once per round
// (table_create), and a segment costs one kernel over its rows:
//     occ = atomicAdd(&target_count[key], 1)          (the target's rank among the rows of its key)
//     the row adds 1 to shift s  iff  occ < c_ref(key + shift_s),
// which sums to exactly min(c_target, c_ref) per key whatever the arrival order.  Sums go into LDS,
// then one integer atomicAdd per block and shift: the result is deterministic.  A cleanup kernel
// zeroes the target counters the segment touched.
//
// Keys are made in the arithmetic of the round (the reference's pandas / numpy dtypes):
//   PMI_AIM_XY_F32  x, y float32:  x + float32(rel), / float32(d), rintf, xu + yu * float32(W), each rounded
//   PMI_AIM_XY_F64  the same in float64
//   PMI_AIM_Z_F32   x, y float64 (no rel), z float32 (already / pixelsize): (xu + yu * W) + float64((zu * W_f) * H_f)
//   PMI_AIM_Z_F64   everything float64, (xu + yu * W) + (zu * W) * H
// and cast to int32 the way x86's cvtt* does (NaN / out of range -> INT_MIN; v_cvt_i32_* would saturate).
// x / y shifts are int32 and add with wrap-around (int32 + int32 in numpy); z shifts are float64 and the
// shifted key is float64 (int32 + float64 in numpy), so it matches only where it is an integer in range.
//
// Reference tables: a dense int32 count array over [key_min, key_max] when the span (plus the largest
// shift on either side for the target counters) fits the dense limit (x / y only), else the reference keys
// sorted (rocPRIM radix sort) with counts by two bounded binary searches, and the target counters in an
// open-addressing hash of 2x the segment's rows (bounded probe; no key value can be a sentinel, so a slot
// holds 1 << 32 | key).  Every search and probe loop has a fixed bound and reports a status, never spins.
#include <algorithm>
#include <cmath>
#include <vector>

#include "rows_common.h"

#pragma clang fp contract(off)

namespace pmi {
namespace aim {

using rows::BLOCK;
using rows::blocks;

constexpr int MAX_SHIFTS = 8192;                   // roi_cc in LDS: 32 KB
static int64_t g_dense_limit = int64_t(1) << 28;  // target-counter entries of the dense form (1 GiB)

struct Cols {
    const void *x, *y, *z;
    const int32_t *rows;
    int64_t n;
};

__device__ __forceinline__ int32_t cvt_i32(double v)
{
    return (v >= -2147483648.0 && v < 2147483648.0) ? (int32_t)v : INT32_MIN;
}

// key of row r: the reference's np.int32(x_units + y_units * W [+ z_units * W * H])
template <int MODE>
__device__ __forceinline__ int32_t make_key(const Cols &c, int64_t r, double rx, double ry, double rz, double d, double W, double H)
{
    if (MODE == PMI_AIM_XY_F32) {
        const float df = (float)d, Wf = (float)W;
        const float xs = __fadd_rn(((const float *)c.x)[r], (float)rx);
        const float ys = __fadd_rn(((const float *)c.y)[r], (float)ry);
        const float xu = rintf(__fdiv_rn(xs, df)), yu = rintf(__fdiv_rn(ys, df));
        return cvt_i32((double)__fadd_rn(xu, __fmul_rn(yu, Wf)));
    } else if (MODE == PMI_AIM_XY_F64) {
        const double xs = __dadd_rn(((const double *)c.x)[r], rx);
        const double ys = __dadd_rn(((const double *)c.y)[r], ry);
        const double xu = rint(__ddiv_rn(xs, d)), yu = rint(__ddiv_rn(ys, d));
        return cvt_i32(__dadd_rn(xu, __dmul_rn(yu, W)));
    } else {
        const double xu = rint(__ddiv_rn(((const double *)c.x)[r], d));
        const double yu = rint(__ddiv_rn(((const double *)c.y)[r], d));
        const double xy = __dadd_rn(xu, __dmul_rn(yu, W));
        double zwh;
        if (MODE == PMI_AIM_Z_F32) {
            const float zs = __fadd_rn(((const float *)c.z)[r], (float)rz);
            const float zu = rintf(__fdiv_rn(zs, (float)d));
            zwh = (double)__fmul_rn(__fmul_rn(zu, (float)W), (float)H);
        } else {
            const double zs = __dadd_rn(((const double *)c.z)[r], rz);
            const double zu = rint(__ddiv_rn(zs, d));
            zwh = __dmul_rn(__dmul_rn(zu, W), H);
        }
        return cvt_i32(__dadd_rn(xy, zwh));
    }
}

// key + shift i as the reference compares it; false where no int32 reference key can equal it
template <int MODE>
__device__ __forceinline__ bool shifted(int32_t key, int i, const int32_t *__restrict__ si, const double *__restrict__ sd, int32_t *q)
{
    if (MODE < PMI_AIM_Z_F32) {
        *q = (int32_t)((uint32_t)key + (uint32_t)si[i]);
        return true;
    }
    const double v = __dadd_rn((double)key, sd[i]);
    if (!(v >= -2147483648.0 && v <= 2147483647.0) || v != trunc(v)) return false;
    *q = (int32_t)v;
    return true;
}

// rows of `sorted` equal to q: two binary searches of at most 64 steps each
__device__ __forceinline__ int32_t sorted_count(const int32_t *__restrict__ a, int64_t n, int32_t q)
{
    int64_t lo = 0, hi = n;
    for (int it = 0; it < 64 && lo < hi; ++it) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (a[mid] < q) lo = mid + 1; else hi = mid;
    }
    int64_t lo2 = lo, hi2 = n;
    for (int it = 0; it < 64 && lo2 < hi2; ++it) {
        const int64_t mid = lo2 + ((hi2 - lo2) >> 1);
        if (a[mid] <= q) lo2 = mid + 1; else hi2 = mid;
    }
    return (int32_t)(lo2 - lo);
}

__device__ __forceinline__ uint32_t hash32(uint32_t k)
{
    k ^= k >> 16; k *= 0x7feb352du; k ^= k >> 15; k *= 0x846ca68bu; k ^= k >> 16;
    return k;
}

// what the kernels read of a table, passed by value; the arrays stay the table's from create to destroy
struct Dev {
    int nshift = 0, dense = 0;
    double d = 0, W = 0, H = 0;
    int32_t kmin = 0;
    uint32_t span = 0, tbase = 0, tsize = 0;      // dense: c_ref over [kmin, kmax], target counters over [kmin - S, kmax + S]
    int32_t *cref = nullptr, *tcount = nullptr;
    int32_t *sorted = nullptr;                     // sorted form: the n_ref keys, sorted
    int64_t n_ref = 0;
    unsigned long long *htab = nullptr;            // sorted form: target hash (1 << 32 | key, 0 = free)
    int32_t *hcnt = nullptr;
    uint64_t hsize = 0;
    int32_t *shift_i = nullptr;                    // x / y shifts
    double *shift_d = nullptr;                     // z shifts
    int64_t *slots = nullptr;                      // per target row: its counter slot, -1 = none
};

struct Table {
    Dev v;
    int mode = 0, device = 0;
    int32_t kmax = 0;
    int64_t slots_cap = 0;
};

__device__ __forceinline__ int32_t ref_count(const Dev &t, int32_t q)
{
    if (t.dense) {
        const uint32_t v = (uint32_t)q - (uint32_t)t.kmin;
        return v < t.span ? t.cref[v] : 0;
    }
    return sorted_count(t.sorted, t.n_ref, q);
}

template <int MODE>
__global__ __launch_bounds__(BLOCK) void count_kernel(Dev t, Cols c, double rx, double ry, double rz, int32_t *__restrict__ out)
{
    extern __shared__ int32_t cc[];
    for (int i = threadIdx.x; i < t.nshift; i += BLOCK) cc[i] = 0;
    __syncthreads();
    for (int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x; i < c.n; i += (int64_t)gridDim.x * BLOCK) {
        const int64_t r = c.rows ? (int64_t)c.rows[i] : i;
        const int32_t key = make_key<MODE>(c, r, rx, ry, rz, t.d, t.W, t.H);
        int64_t slot = -1;
        int32_t occ = 0;
        if (t.dense) {
            const uint32_t u = (uint32_t)key - t.tbase;
            if (u < t.tsize) { slot = u; occ = atomicAdd(&t.tcount[u], 1); }
        } else {
            bool any = false;
            for (int s = 0; s < t.nshift && !any; ++s) {
                int32_t q;
                any = shifted<MODE>(key, s, t.shift_i, t.shift_d, &q) && ref_count(t, q) > 0;
            }
            if (any) {
                const unsigned long long e = (1ull << 32) | (uint32_t)key;
                uint64_t h = hash32((uint32_t)key) & (t.hsize - 1);
                for (uint64_t p = 0; p < t.hsize; ++p) {
                    const unsigned long long old = atomicCAS(&t.htab[h], 0ull, e);
                    if (old == 0ull || old == e) { slot = (int64_t)h; break; }
                    h = (h + 1) & (t.hsize - 1);
                }
                if (slot < 0) atomicOr(&out[t.nshift], 1);      // table full: cannot happen at load <= 1/2
                else occ = atomicAdd(&t.hcnt[slot], 1);
            }
        }
        t.slots[i] = slot;
        if (slot < 0) continue;
        for (int s = 0; s < t.nshift; ++s) {
            int32_t q;
            if (shifted<MODE>(key, s, t.shift_i, t.shift_d, &q) && occ < ref_count(t, q)) atomicAdd(&cc[s], 1);
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < t.nshift; i += BLOCK)
        if (cc[i]) atomicAdd(&out[i], cc[i]);
}

__global__ void cleanup_kernel(Dev t, int64_t n)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int64_t slot = t.slots[i];
    if (slot < 0) return;
    if (t.dense) {
        t.tcount[slot] = 0;
    } else {
        t.htab[slot] = 0ull;
        t.hcnt[slot] = 0;
    }
}

template <int MODE>
__global__ void ref_keys_kernel(Cols c, double d, double W, double H, int32_t *__restrict__ keys, int32_t *__restrict__ minmax)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= c.n) return;
    const int64_t r = c.rows ? (int64_t)c.rows[i] : i;
    const int32_t k = make_key<MODE>(c, r, 0.0, 0.0, 0.0, d, W, H);
    keys[i] = k;
    atomicMin(&minmax[0], k);
    atomicMax(&minmax[1], k);
}

__global__ void dense_add_kernel(const int32_t *__restrict__ keys, int64_t n, int32_t kmin, int32_t *__restrict__ cref)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) atomicAdd(&cref[(uint32_t)keys[i] - (uint32_t)kmin], 1);
}

__global__ void seg_hist_kernel(const int64_t *__restrict__ frame, int64_t n, int64_t seg_len, int64_t n_frames,
                                int32_t *__restrict__ counts)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int64_t f = frame[i];
    if (f >= 1 && f <= n_frames) atomicAdd(&counts[(f - 1) / seg_len], 1);
}

__global__ void seg_scatter_kernel(const int64_t *__restrict__ frame, int64_t n, int64_t seg_len, int64_t n_frames,
                                   int64_t *__restrict__ cursor, int32_t *__restrict__ rows)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int64_t f = frame[i];
    if (f >= 1 && f <= n_frames) rows[atomicAdd((unsigned long long *)&cursor[(f - 1) / seg_len], 1ull)] = (int32_t)i;
}

// kernel<MODE> of the table's key arithmetic
#define PMI_AIM_DISPATCH(mode, kernel, grid, lds, stream, ...)                                               \
    do {                                                                                                     \
        switch (mode) {                                                                                      \
        case PMI_AIM_XY_F32: kernel<PMI_AIM_XY_F32><<<grid, BLOCK, lds, stream>>>(__VA_ARGS__); break;       \
        case PMI_AIM_XY_F64: kernel<PMI_AIM_XY_F64><<<grid, BLOCK, lds, stream>>>(__VA_ARGS__); break;       \
        case PMI_AIM_Z_F32: kernel<PMI_AIM_Z_F32><<<grid, BLOCK, lds, stream>>>(__VA_ARGS__); break;         \
        default: kernel<PMI_AIM_Z_F64><<<grid, BLOCK, lds, stream>>>(__VA_ARGS__); break;                    \
        }                                                                                                    \
        PMI_HIP(hipGetLastError());                                                                          \
    } while (0)

static void release(Table *t)
{
    if (!t) return;
    int cur = 0;
    (void)hipGetDevice(&cur);
    (void)hipSetDevice(t->device);
    const Dev &v = t->v;
    for (void *p : {(void *)v.cref, (void *)v.tcount, (void *)v.sorted, (void *)v.htab, (void *)v.hcnt,
                    (void *)v.shift_i, (void *)v.shift_d, (void *)v.slots})
        if (p) (void)hipFree(p);
    (void)hipSetDevice(cur);
    delete t;
}

static int check_mode(int mode)
{
    if (mode < PMI_AIM_XY_F32 || mode > PMI_AIM_Z_F64) {
        set_error("pmi_aim: unknown key mode %d", mode);
        return PMI_ERR_ARG;
    }
    return PMI_OK;
}

static int table_create(int mode, Cols ref, double d, double W, double H, const void *shifts, int nshift, Table **out,
                        hipStream_t s)
{
    *out = nullptr;
    int rc = check_mode(mode);
    if (rc) return rc;
    if (nshift < 1 || nshift > MAX_SHIFTS || !shifts || ref.n < 0 || ref.n > INT32_MAX || !(d > 0)) {
        set_error("pmi_aim_table_create: %d shifts (1..%d), %lld reference rows, d = %g", nshift, MAX_SHIFTS,
                  (long long)ref.n, d);
        return PMI_ERR_ARG;
    }
    Table *t = new Table;
    Dev &v = t->v;
    t->mode = mode; v.nshift = nshift; v.d = d; v.W = W; v.H = H; v.n_ref = ref.n;
    (void)hipGetDevice(&t->device);
    struct Guard { Table *&t; ~Guard() { release(t); } } guard{t};
    const bool xy = mode < PMI_AIM_Z_F32;
    int64_t max_shift = 0;
    if (xy) {
        PMI_HIP(hipMalloc(&v.shift_i, sizeof(int32_t) * nshift));
        PMI_HIP(hipMemcpyAsync(v.shift_i, shifts, sizeof(int32_t) * nshift, hipMemcpyHostToDevice, s));
        for (int i = 0; i < nshift; ++i) max_shift = std::max<int64_t>(max_shift, std::llabs((long long)((const int32_t *)shifts)[i]));
    } else {
        PMI_HIP(hipMalloc(&v.shift_d, sizeof(double) * nshift));
        PMI_HIP(hipMemcpyAsync(v.shift_d, shifts, sizeof(double) * nshift, hipMemcpyHostToDevice, s));
    }
    // the reference keys and their min / max die with this call (the stream is synchronised before it returns)
    int32_t *keys, *mm;
    rc = rows::carve(SCR_STAGE_A, [&](rows::Arena &ar) {
        keys = ar.take<int32_t>(std::max<int64_t>(ref.n, 1));
        mm = ar.take<int32_t>(2);
    });
    if (rc != PMI_OK) return rc;
    const int32_t init[2] = {INT32_MAX, INT32_MIN};
    PMI_HIP(hipMemcpyAsync(mm, init, sizeof(init), hipMemcpyHostToDevice, s));
    if (ref.n > 0) PMI_AIM_DISPATCH(mode, ref_keys_kernel, blocks(ref.n), 0, s, ref, d, W, H, keys, mm);
    int32_t hmm[2];
    PMI_HIP(hipMemcpyAsync(hmm, mm, sizeof(hmm), hipMemcpyDeviceToHost, s));
    PMI_HIP(hipStreamSynchronize(s));
    if (ref.n == 0) { hmm[0] = 0; hmm[1] = -1; }
    v.kmin = hmm[0]; t->kmax = hmm[1];
    const int64_t span = (int64_t)hmm[1] - hmm[0] + 1;          // 0 for an empty reference
    const int64_t tsize = span + 2 * max_shift;
    if (xy && tsize <= g_dense_limit) {
        v.dense = 1;
        v.span = (uint32_t)span;
        v.tsize = (uint32_t)tsize;
        v.tbase = (uint32_t)((int64_t)v.kmin - max_shift);
        PMI_HIP(hipMalloc(&v.cref, sizeof(int32_t) * std::max<int64_t>(span, 1)));
        PMI_HIP(hipMalloc(&v.tcount, sizeof(int32_t) * std::max<int64_t>(tsize, 1)));
        PMI_HIP(hipMemsetAsync(v.cref, 0, sizeof(int32_t) * std::max<int64_t>(span, 1), s));
        PMI_HIP(hipMemsetAsync(v.tcount, 0, sizeof(int32_t) * std::max<int64_t>(tsize, 1), s));
        if (ref.n > 0) PMI_LAUNCH(dense_add_kernel, ref.n, s, keys, ref.n, v.kmin, v.cref);
    } else {
        PMI_HIP(hipMalloc(&v.sorted, sizeof(int32_t) * std::max<int64_t>(ref.n, 1)));
        if (ref.n > 0 && (rc = rows::sort_keys(keys, v.sorted, (size_t)ref.n, 32, s)) != PMI_OK) return rc;
    }
    PMI_HIP(hipStreamSynchronize(s));
    *out = t;
    t = nullptr;          // the guard lets go
    return PMI_OK;
}

static int count(Table *t, Cols c, double rx, double ry, double rz, int32_t *d_out, hipStream_t s)
{
    if (!t || !d_out || c.n < 0 || c.n > INT32_MAX) {
        set_error("pmi_aim_count_dev: no table, no output or %lld rows", (long long)c.n);
        return PMI_ERR_ARG;
    }
    Dev &v = t->v;
    if (c.n > t->slots_cap) {
        PMI_HIP(hipStreamSynchronize(s));
        if (v.slots) { (void)hipFree(v.slots); v.slots = nullptr; t->slots_cap = 0; }
        PMI_HIP(hipMalloc(&v.slots, sizeof(int64_t) * c.n));
        t->slots_cap = c.n;
    }
    if (!v.dense && 2 * (uint64_t)c.n > v.hsize) {
        uint64_t h = 1024;
        while (h < 2 * (uint64_t)c.n) h <<= 1;
        PMI_HIP(hipStreamSynchronize(s));
        if (v.htab) { (void)hipFree(v.htab); v.htab = nullptr; }
        if (v.hcnt) { (void)hipFree(v.hcnt); v.hcnt = nullptr; }
        v.hsize = 0;
        PMI_HIP(hipMalloc(&v.htab, sizeof(unsigned long long) * h));
        PMI_HIP(hipMalloc(&v.hcnt, sizeof(int32_t) * h));
        PMI_HIP(hipMemsetAsync(v.htab, 0, sizeof(unsigned long long) * h, s));
        PMI_HIP(hipMemsetAsync(v.hcnt, 0, sizeof(int32_t) * h, s));
        v.hsize = h;
    }
    PMI_HIP(hipMemsetAsync(d_out, 0, sizeof(int32_t) * (v.nshift + 1), s));
    if (c.n == 0) return PMI_OK;
    const unsigned grid = (unsigned)std::min<int64_t>(blocks(c.n), 8 * (int64_t)device_cu_count());
    PMI_AIM_DISPATCH(t->mode, count_kernel, grid, sizeof(int32_t) * v.nshift, s, v, c, rx, ry, rz, d_out);
    PMI_LAUNCH(cleanup_kernel, c.n, s, v, c.n);
    return PMI_OK;
}

}  // namespace aim
}  // namespace pmi

using namespace pmi;

extern "C" {

int pmi_aim_set_dense_limit(int64_t entries)
{
    if (entries < 0) {
        set_error("pmi_aim_set_dense_limit: %lld < 0", (long long)entries);
        return PMI_ERR_ARG;
    }
    aim::g_dense_limit = entries;
    return PMI_OK;
}

int pmi_aim_partition_dev(const int64_t *d_frame, int64_t n, int64_t seg_len, int64_t n_frames, int32_t *d_rows,
                          int64_t *seg_offsets, void *stream)
{
    if (n < 0 || n > INT32_MAX || seg_len < 1 || n_frames < 0 || (n > 0 && (!d_frame || !d_rows)) || !seg_offsets) {
        set_error("pmi_aim_partition_dev: n = %lld, segmentation = %lld, frames = %lld", (long long)n,
                  (long long)seg_len, (long long)n_frames);
        return PMI_ERR_ARG;
    }
    hipStream_t s = (hipStream_t)stream;
    const int64_t n_seg = (n_frames + seg_len - 1) / seg_len;
    seg_offsets[0] = 0;
    if (n_seg == 0) return PMI_OK;
    // counts and cursor die with this call (the stream is synchronised before it returns)
    int32_t *counts;
    int64_t *cursor;
    const int rc = rows::carve(SCR_STAGE_A, [&](rows::Arena &ar) {
        counts = ar.take<int32_t>(n_seg);
        cursor = ar.take<int64_t>(n_seg);
    });
    if (rc != PMI_OK) return rc;
    PMI_HIP(hipMemsetAsync(counts, 0, sizeof(int32_t) * n_seg, s));
    if (n > 0) PMI_LAUNCH(aim::seg_hist_kernel, n, s, d_frame, n, seg_len, n_frames, counts);
    std::vector<int32_t> h(n_seg);
    PMI_HIP(hipMemcpyAsync(h.data(), counts, sizeof(int32_t) * n_seg, hipMemcpyDeviceToHost, s));
    PMI_HIP(hipStreamSynchronize(s));
    for (int64_t i = 0; i < n_seg; ++i) seg_offsets[i + 1] = seg_offsets[i] + h[i];
    PMI_HIP(hipMemcpyAsync(cursor, seg_offsets, sizeof(int64_t) * n_seg, hipMemcpyHostToDevice, s));
    if (n > 0) PMI_LAUNCH(aim::seg_scatter_kernel, n, s, d_frame, n, seg_len, n_frames, cursor, d_rows);
    PMI_HIP(hipStreamSynchronize(s));
    return PMI_OK;
}

int pmi_aim_table_create_dev(int mode, const void *d_x, const void *d_y, const void *d_z, const int32_t *d_rows,
                             int64_t n_ref, double intersect_d, double width_units, double height_units,
                             const void *shifts, int n_shifts, void **table, void *stream)
{
    if (!table) {
        set_error("pmi_aim_table_create_dev: table == NULL");
        return PMI_ERR_ARG;
    }
    aim::Table *t = nullptr;
    const int rc = aim::table_create(mode, aim::Cols{d_x, d_y, d_z, d_rows, n_ref}, intersect_d, width_units,
                                     height_units, shifts, n_shifts, &t, (hipStream_t)stream);
    *table = t;
    return rc;
}

int pmi_aim_table_info(void *table, int *dense, int64_t *entries)
{
    aim::Table *t = (aim::Table *)table;
    if (!t) {
        set_error("pmi_aim_table_info: table == NULL");
        return PMI_ERR_ARG;
    }
    if (dense) *dense = t->v.dense;
    if (entries) *entries = t->v.dense ? (int64_t)t->v.span : t->v.n_ref;
    return PMI_OK;
}

int pmi_aim_count_dev(void *table, const void *d_x, const void *d_y, const void *d_z, const int32_t *d_rows,
                      int64_t n_rows, double rel_x, double rel_y, double rel_z, int32_t *d_out, void *stream)
{
    return aim::count((aim::Table *)table, aim::Cols{d_x, d_y, d_z, d_rows, n_rows}, rel_x, rel_y, rel_z, d_out,
                      (hipStream_t)stream);
}

int pmi_aim_table_destroy(void *table)
{
    aim::release((aim::Table *)table);
    return PMI_OK;
}

int pmi_aim_roi_cc(int mode, const void *ref_x, const void *ref_y, const void *ref_z, int64_t n_ref, const void *x,
                   const void *y, const void *z, int64_t n, double rel_x, double rel_y, double rel_z,
                   double intersect_d, double width_units, double height_units, const void *shifts, int n_shifts,
                   int64_t *roi_cc)
{
    int rc = aim::check_mode(mode);
    if (rc) return rc;
    if (n_ref < 0 || n < 0 || n_shifts < 1 || n_shifts > aim::MAX_SHIFTS || !roi_cc) {
        set_error("pmi_aim_roi_cc: n_ref = %lld, n = %lld, %d shifts", (long long)n_ref, (long long)n, n_shifts);
        return PMI_ERR_ARG;
    }
    const bool zm = mode >= PMI_AIM_Z_F32;
    const size_t xy_b = (mode == PMI_AIM_XY_F32) ? 4 : 8, z_b = (mode == PMI_AIM_Z_F32) ? 4 : 8;
    // the six columns and the counts; a mode without z leaves drz and dz null
    char *drx = nullptr, *dry = nullptr, *drz = nullptr, *dx = nullptr, *dy = nullptr, *dz = nullptr;
    int32_t *dout = nullptr;
    std::vector<int32_t> h(n_shifts + 1);
    Staged st(SCR_STAGE_C);          // table_create carves SCR_STAGE_A and sorts through SCR_STAGE_B
    st.add(drx, xy_b * n_ref, ref_x), st.add(dry, xy_b * n_ref, ref_y), st.add(dx, xy_b * n, x), st.add(dy, xy_b * n, y);
    if (zm) st.add(drz, z_b * n_ref, ref_z), st.add(dz, z_b * n, z);
    st.add(dout, h.size(), nullptr, h.data());
    if ((rc = st.place())) return rc;
    aim::Table *t = nullptr;
    rc = aim::table_create(mode, aim::Cols{drx, dry, drz, nullptr, n_ref}, intersect_d, width_units, height_units,
                           shifts, n_shifts, &t, nullptr);
    if (rc) return rc;
    rc = aim::count(t, aim::Cols{dx, dy, dz, nullptr, n}, rel_x, rel_y, rel_z, dout, nullptr);
    if (!rc) rc = st.fetch();
    aim::release(t);
    if (rc) return rc;
    if (h[n_shifts]) {
        set_error("pmi_aim_roi_cc: target hash full (status %d)", h[n_shifts]);
        return PMI_ERR_HIP;
    }
    for (int i = 0; i < n_shifts; ++i) roi_cc[i] = h[i];
    return PMI_OK;
}

}  // extern "C"
