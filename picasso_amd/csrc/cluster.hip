// cluster.hip — DBSCAN and the SMLM clusterer (picasso/clusterer.py:114-201 _cluster, :34-111 frame analysis,
// :410-445 _dbscan), label for label.
//
// Both take the points as float64 columns (the reference's KDTree and sklearn widen float32 first) and share one
// neighbour predicate: row j is a neighbour of row i, itself included, iff dx*dx + dy*dy (+ dz*dz) <= r2 in float64,
// summed in dimension order, one rounding per operation (no contraction).
//
// Cell sort.  Rows are binned into cells of side r * (1 + 2^-16) counted from the table's lower corner and radix-sorted
// by cell key (rocPRIM); the coordinates are gathered into that order.  The hair on the side makes the candidate set
// a superset under the rounding of (x - lo) / side: two rows that pass the predicate differ by less than one cell
// coordinate, so the 3 (x 3) x 3 cells around a row hold all its neighbours.  Cell coordinates are clamped to what the
// key has bits for (monotone, so the superset holds; a clamped border cell is only slower).  The key's last dimension
// is lowest, so the three cells along it are one run of the sorted keys: 3 (2-D) or 9 (3-D) row ranges per row, found
// once by bisection and kept.  Memory is O(rows), whatever extent / r is.
//
// SMLM clusterer, as a function of the data (n_i = neighbour count, rows numbered as the caller's):
//     local maximum   n_i > min_locs and n_i = max n over the neighbours; the k-th in row order has the number k
//     fresh           a local maximum without a lower-indexed local maximum among its neighbours
//     label of a row  the number of its highest-indexed fresh neighbour; without one, the label of its lowest-indexed
//                     neighbour maximum (a chain towards lower rows that ends at a maximum with a fresh neighbour:
//                     pointer jumping, a bounded number of rounds); without any, -1
// A fresh maximum's only fresh neighbour is itself, so the rule holds for every row.
//
// DBSCAN: core iff n_i >= min_samples; union-find over core rows (the parent is always the lower row, so a root is the
// lowest core row of its cluster); a cluster's number is the rank of its root; a border row takes the lowest number
// among its core neighbours.
//
// Then labels with fewer than min_locs rows become -1 (integer atomics: the order does not matter), and with a frame
// column every label is checked by its mean frame and its fullest of 20 time bins.  No float atomics or reductions.
// Every loop is bounded by the row count; a union or a chain that does not settle reports a status.
#include <algorithm>

#include "rows_common.h"

#pragma clang fp contract(off)

namespace pmi {
namespace cluster {

using namespace rows;

constexpr int FA_BINS = 20;
constexpr int MAX_ROUNDS = 40;       // pointer jumping doubles the distance covered: 31 rounds for 2^31 rows

struct Grid {
    double lo[3];
    double side;
    int64_t maxc[3];     // highest cell coordinate per dimension (coordinates are clamped into [0, maxc])
    int shift[3];        // key = sum c[k] << shift[k]; the last dimension is lowest
    int bits;            // of the key
};

// the table in cell order
struct Tab {
    const double *x, *y, *z;      // coordinates by sorted position
    const int32_t *rows;          // the caller's row of a sorted position
    const int32_t *rlo, *rhi;     // [k * n + p]: the k-th candidate range of position p
    int32_t n;
    double r2;
};

__device__ __forceinline__ int64_t cell_coord(double v, double lo, double side, int64_t maxc)
{
    const double u = (v - lo) / side;
    if (!(u >= 0.0)) return 0;                   // below the corner, or not a number
    if (u >= (double)maxc) return maxc;
    return (int64_t)u;
}

template <int D>
__global__ void key_kernel(const double *__restrict__ X, int32_t n, Grid g, uint64_t *__restrict__ keys,
                           int32_t *__restrict__ rows)
{
    const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    uint64_t key = 0;
#pragma unroll
    for (int k = 0; k < D; ++k)
        key |= (uint64_t)cell_coord(X[(size_t)k * n + i], g.lo[k], g.side, g.maxc[k]) << g.shift[k];
    keys[i] = key;
    rows[i] = (int32_t)i;
}

template <int D>
__global__ void gather_kernel(const double *__restrict__ X, const uint64_t *__restrict__ keys,
                              const int32_t *__restrict__ rows, int32_t n, Grid g, double *__restrict__ xs,
                              double *__restrict__ ys, double *__restrict__ zs, int32_t *__restrict__ rlo,
                              int32_t *__restrict__ rhi)
{
    const int64_t p = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (p >= n) return;
    const int32_t i = rows[p];
    xs[p] = X[i];
    ys[p] = X[(size_t)n + i];
    if (D == 3) zs[p] = X[2 * (size_t)n + i];
    const uint64_t key = keys[p];
    int64_t c[3] = {0, 0, 0};
#pragma unroll
    for (int k = 0; k < D; ++k) {
        const int top = k == 0 ? g.bits : g.shift[k - 1];
        c[k] = (int64_t)((key >> g.shift[k]) & ((uint64_t(1) << (top - g.shift[k])) - 1));
    }
    const int64_t l0 = c[D - 1] > 0 ? c[D - 1] - 1 : 0;
    const int64_t l1 = c[D - 1] < g.maxc[D - 1] ? c[D - 1] + 1 : g.maxc[D - 1];
    int k = 0;
    for (int ox = -1; ox <= 1; ++ox)
        for (int oy = (D == 3 ? -1 : 0); oy <= (D == 3 ? 1 : 0); ++oy, ++k) {
            const int64_t cx = c[0] + ox, cy = c[1] + oy;
            int32_t a = 0, b = 0;
            if (cx >= 0 && cx <= g.maxc[0] && (D == 2 || (cy >= 0 && cy <= g.maxc[1]))) {
                uint64_t base = (uint64_t)cx << g.shift[0];
                if (D == 3) base |= (uint64_t)cy << g.shift[1];
                a = lower_bound(keys, 0, n, base | (uint64_t)l0);
                b = lower_bound(keys, 0, n, (base | (uint64_t)l1) + 1u);
            }
            rlo[(size_t)k * n + p] = a;
            rhi[(size_t)k * n + p] = b;
        }
}

// f(q) for every neighbour q of position p (p itself included)
template <int D, typename F>
__device__ __forceinline__ void for_neighbours(const Tab &t, int32_t p, F &&f)
{
    constexpr int K = D == 2 ? 3 : 9;
    const double x = t.x[p], y = t.y[p], z = D == 3 ? t.z[p] : 0.0;
    for (int k = 0; k < K; ++k) {
        const int32_t a = t.rlo[(size_t)k * t.n + p], b = t.rhi[(size_t)k * t.n + p];
        for (int32_t q = a; q < b; ++q) {
            const double dx = t.x[q] - x, dy = t.y[q] - y;
            double s = dx * dx + dy * dy;
            if (D == 3) {
                const double dz = t.z[q] - z;
                s = s + dz * dz;
            }
            if (s <= t.r2) f(q);
        }
    }
}

template <int D>
__global__ void count_kernel(Tab t, int32_t *__restrict__ cnt)
{
    const int64_t p64 = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (p64 >= t.n) return;
    int32_t c = 0;
    for_neighbours<D>(t, (int32_t)p64, [&](int32_t) { ++c; });
    cnt[p64] = c;
}

// ---- SMLM clusterer --------------------------------------------------------------------------------------------
// lm[p] = 1 for a local maximum; flag[row] the same by the caller's rows, for the numbering
template <int D>
__global__ void localmax_kernel(Tab t, const int32_t *__restrict__ cnt, int64_t min_locs, int32_t *__restrict__ lm,
                                uint32_t *__restrict__ flag)
{
    const int64_t p64 = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (p64 >= t.n) return;
    const int32_t p = (int32_t)p64, c = cnt[p];
    int32_t is = 0;
    if ((int64_t)c > min_locs) {
        int32_t m = 0;
        for_neighbours<D>(t, p, [&](int32_t q) { m = max(m, cnt[q]); });
        is = c == m;
    }
    lm[p] = is;
    flag[t.rows[p]] = (uint32_t)is;
}

// state[p]: 0 no maximum, 1 a maximum with a lower-indexed maximum among its neighbours, 2 a fresh maximum
template <int D>
__global__ void fresh_kernel(Tab t, const int32_t *__restrict__ lm, int32_t *__restrict__ state)
{
    const int64_t p64 = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (p64 >= t.n) return;
    const int32_t p = (int32_t)p64;
    int32_t s = 0;
    if (lm[p]) {
        const int32_t me = t.rows[p];
        bool lower = false;
        for_neighbours<D>(t, p, [&](int32_t q) { lower |= lm[q] && t.rows[q] < me; });
        s = lower ? 1 : 2;
    }
    state[p] = s;
}

// lab[p] >= -1: the label; lab[p] <= -2: the label of position -(lab[p] + 2), a maximum of a lower row
template <int D>
__global__ void assign_kernel(Tab t, const int32_t *__restrict__ state, const uint32_t *__restrict__ number,
                              int32_t *__restrict__ lab)
{
    const int64_t p64 = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (p64 >= t.n) return;
    const int32_t p = (int32_t)p64;
    int32_t fresh_row = -1, low_row = INT32_MAX, low_pos = -1;
    for_neighbours<D>(t, p, [&](int32_t q) {
        const int32_t s = state[q];
        if (!s) return;
        const int32_t row = t.rows[q];
        if (s == 2) fresh_row = max(fresh_row, row);
        if (row < low_row) { low_row = row; low_pos = q; }
    });
    lab[p] = fresh_row >= 0 ? (int32_t)number[fresh_row] : (low_pos >= 0 && low_pos != p ? -(low_pos + 2) : -1);
}

// One round: a pending row takes what the row it points at holds — that row's label, or its pointer further down.
__global__ void jump_kernel(int32_t *lab, int32_t n, int32_t *pending)
{
    const int64_t p = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (p >= n) return;
    const int32_t v = __hip_atomic_load(lab + p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (v >= -1) return;
    const int32_t target = -(v + 2);
    int32_t w = -1;
    if (target >= 0 && target < n) w = __hip_atomic_load(lab + target, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(lab + p, w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (w < -1) atomicOr(pending, 1);
}

// ---- DBSCAN ------------------------------------------------------------------------------------------------------
// parent[] is indexed by the caller's rows
template <int D>
__global__ void union_kernel(Tab t, const int32_t *__restrict__ cnt, int64_t min_samples, int32_t *parent,
                             int32_t *status)
{
    const int64_t p64 = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (p64 >= t.n) return;
    const int32_t p = (int32_t)p64;
    if ((int64_t)cnt[p] < min_samples) return;
    const int32_t me = t.rows[p];
    for_neighbours<D>(t, p, [&](int32_t q) {
        const int32_t other = t.rows[q];
        if (other < me && (int64_t)cnt[q] >= min_samples) unite(parent, me, other, t.n, status);
    });
}

// root[p] = the lowest core row of a core row's cluster, -1 for a row that is not core; flag[row] = 1 at the roots
__global__ void root_kernel(const int32_t *__restrict__ rows, const int32_t *__restrict__ cnt, int64_t min_samples,
                            const int32_t *__restrict__ parent, int32_t n, int32_t *__restrict__ root,
                            uint32_t *__restrict__ flag)
{
    const int64_t p = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (p >= n) return;
    const int32_t me = rows[p];
    int32_t r = -1;
    if ((int64_t)cnt[p] >= min_samples) r = find_root(parent, me, n);
    root[p] = r;
    flag[me] = r == me ? 1u : 0u;
}

template <int D>
__global__ void dbscan_label_kernel(Tab t, const int32_t *__restrict__ root, const uint32_t *__restrict__ number,
                                    int32_t *__restrict__ lab)
{
    const int64_t p64 = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (p64 >= t.n) return;
    const int32_t p = (int32_t)p64;
    const int32_t r = root[p];
    if (r >= 0) { lab[p] = (int32_t)number[r]; return; }
    int32_t best = INT32_MAX;
    for_neighbours<D>(t, p, [&](int32_t q) {
        const int32_t rq = root[q];
        if (rq >= 0) best = min(best, (int32_t)number[rq]);
    });
    lab[p] = best == INT32_MAX ? -1 : best;
}

// ---- label sizes, frame analysis -----------------------------------------------------------------------------------
__global__ void size_kernel(const int32_t *__restrict__ lab, int32_t n, int32_t *size)
{
    const int64_t p = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (p >= n) return;
    const int32_t l = lab[p];
    if (l >= 0 && l < n) atomicAdd(size + l, 1);
}

__global__ void size_filter_kernel(int32_t *__restrict__ lab, int32_t n, const int32_t *__restrict__ size,
                                   int64_t min_locs)
{
    const int64_t p = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (p >= n) return;
    const int32_t l = lab[p];
    if (l >= 0 && l < n && (int64_t)size[l] < min_locs) lab[p] = -1;
}

struct Edges { double e[FA_BINS + 1]; };

// id = label + shift; the frame of position p is frame[rows[p]] (rows == nullptr: frame[p])
__global__ void fa_count_kernel(const int32_t *__restrict__ lab, int32_t shift, const int32_t *__restrict__ rows,
                                const int64_t *__restrict__ frame, int32_t n, int32_t n_ids, Edges ed,
                                int32_t *count, unsigned long long *sum, int32_t *hist)
{
    const int64_t p = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (p >= n) return;
    const int64_t id = (int64_t)lab[p] + shift;
    if (id < 0 || id >= n_ids) return;
    const int64_t f = frame[rows ? rows[p] : p];
    atomicAdd(count + id, 1);
    atomicAdd(sum + id, (unsigned long long)f);
    const double v = (double)f;
    if (!(v >= ed.e[0] && v <= ed.e[FA_BINS])) return;
    int b = 0;
#pragma unroll
    for (int k = 1; k < FA_BINS; ++k) b += v >= ed.e[k] ? 1 : 0;
    atomicAdd(hist + id * FA_BINS + b, 1);
}

__global__ void fa_decide_kernel(const int32_t *__restrict__ count, const unsigned long long *__restrict__ sum,
                                 const int32_t *__restrict__ hist, int32_t n_ids, double lo, double hi,
                                 int32_t *__restrict__ pass)
{
    const int64_t g = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (g >= n_ids) return;
    const int32_t c = count[g];
    if (c == 0) { pass[g] = 1; return; }
    const double mean = (double)(int64_t)sum[g] / (double)c;
    int32_t m = 0;
    for (int k = 0; k < FA_BINS; ++k) m = max(m, hist[g * FA_BINS + k]);
    pass[g] = (mean < lo || mean > hi || (double)m > 0.8 * (double)c) ? 0 : 1;
}

__global__ void fa_apply_kernel(int32_t *__restrict__ lab, int32_t shift, int32_t n, int32_t n_ids,
                                const int32_t *__restrict__ pass)
{
    const int64_t p = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (p >= n) return;
    const int64_t id = (int64_t)lab[p] + shift;
    if (id >= 0 && id < n_ids && !pass[id]) lab[p] = -1;
}

__global__ void scatter_kernel(const int32_t *__restrict__ lab, const int32_t *__restrict__ rows, int32_t n,
                               int32_t *__restrict__ out)
{
    const int64_t p = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (p < n) out[rows[p]] = lab[p];
}

// ---- host ------------------------------------------------------------------------------------------------------
static int check_args(const char *what, const double *d_X, int dims, int64_t n, const double *lo, const double *hi,
                      double r, double r2)
{
    if (n < 0 || n > INT32_MAX - 1) {
        set_error("%s: %lld rows (this kernel indexes rows with int32)", what, (long long)n);
        return PMI_ERR_ARG;
    }
    if (dims != 2 && dims != 3) {
        set_error("%s: %d dimensions (2 or 3)", what, dims);
        return PMI_ERR_ARG;
    }
    if (!(r > 0.0) || !(r2 >= 0.0) || !(r < 1e300)) {
        set_error("%s: radius %g", what, r);
        return PMI_ERR_ARG;
    }
    if (n > 0 && (!d_X || !lo || !hi)) {
        set_error("%s: NULL column or corner", what);
        return PMI_ERR_ARG;
    }
    for (int k = 0; n > 0 && k < dims; ++k)
        if (!(lo[k] <= hi[k]) || !(hi[k] - lo[k] < 1e300)) {
            set_error("%s: corner %g .. %g of dimension %d", what, lo[k], hi[k], k);
            return PMI_ERR_ARG;
        }
    return PMI_OK;
}

static Grid make_grid(int dims, const double *lo, const double *hi, double r)
{
    Grid g{};
    g.side = r * (1.0 + 1.0 / 65536.0);
    const int cap_bits = dims == 2 ? 31 : 21;
    int bits[3] = {0, 0, 0};
    for (int k = 0; k < dims; ++k) {
        g.lo[k] = lo[k];
        const double cells = (hi[k] - lo[k]) / g.side + 2.0;
        const int64_t cap = (int64_t(1) << cap_bits) - 2;
        g.maxc[k] = cells >= (double)cap ? cap : std::max<int64_t>((int64_t)cells, 1);
        while ((int64_t(1) << bits[k]) <= g.maxc[k] + 1) bits[k]++;      // maxc + 1 fits
    }
    g.shift[dims - 1] = 0;
    for (int k = dims - 2; k >= 0; --k) g.shift[k] = g.shift[k + 1] + bits[k + 1];
    g.bits = g.shift[0] + bits[0];
    return g;
}

struct Work {
    uint64_t *keys, *keys_sorted;
    int32_t *rows0, *rows, *rlo, *rhi, *cnt, *a, *b, *lab, *status;
    uint32_t *flag, *number;
    double *xs, *ys, *zs;
};

static void layout(Arena &ar, Work &w, int dims, size_t N)
{
    const size_t K = dims == 2 ? 3 : 9;
    w.keys = ar.take<uint64_t>(N);
    w.keys_sorted = ar.take<uint64_t>(N);
    w.rows0 = ar.take<int32_t>(N);
    w.rows = ar.take<int32_t>(N);
    w.xs = ar.take<double>(N);
    w.ys = ar.take<double>(N);
    w.zs = ar.take<double>(dims == 3 ? N : 1);
    w.rlo = ar.take<int32_t>(K * N);
    w.rhi = ar.take<int32_t>(K * N);
    w.cnt = ar.take<int32_t>(N);
    w.a = ar.take<int32_t>(N);
    w.b = ar.take<int32_t>(N);
    w.lab = ar.take<int32_t>(N);
    w.flag = ar.take<uint32_t>(N);
    w.number = ar.take<uint32_t>(N);
    w.status = ar.take<int32_t>(4);
}

// cell sort, candidate ranges and neighbour counts: everything both algorithms start from
template <int D>
static int prepare(const double *d_X, int32_t n, const double *lo, const double *hi, double r, double r2, Work &w,
                   Tab &t, hipStream_t s)
{
    const size_t N = (size_t)n;
    int rc = carve(SCR_STAGE_A, [&](Arena &ar) { layout(ar, w, D, N); });
    if (rc != PMI_OK) return rc;
    const Grid g = make_grid(D, lo, hi, r);
    PMI_HIP(hipMemsetAsync(w.status, 0, 16, s));
    PMI_LAUNCH(key_kernel<D>, n, s, d_X, n, g, w.keys, w.rows0);
    if ((rc = sort_pairs(w.keys, w.keys_sorted, w.rows0, w.rows, N, g.bits, s)) != PMI_OK) return rc;
    PMI_LAUNCH(gather_kernel<D>, n, s, d_X, w.keys_sorted, w.rows, n, g, w.xs, w.ys, w.zs, w.rlo, w.rhi);
    t = Tab{w.xs, w.ys, w.zs, w.rows, w.rlo, w.rhi, n, r2};
    PMI_LAUNCH(count_kernel<D>, n, s, t, w.cnt);
    return PMI_OK;
}

// labels below min_locs rows -> -1; `size` is a dead n-entry array
static int drop_small(int32_t *lab, int32_t n, int32_t *size, int64_t min_locs, hipStream_t s)
{
    PMI_HIP(hipMemsetAsync(size, 0, sizeof(int32_t) * (size_t)n, s));
    PMI_LAUNCH(size_kernel, n, s, lab, n, size);
    PMI_LAUNCH(size_filter_kernel, n, s, lab, n, size, min_locs);
    return PMI_OK;
}

// pass[id] of every id = label + shift in [0, n_ids); with `apply` the labels that fail become -1
static int frame_analysis(int32_t *lab, int32_t shift, const int32_t *rows, const int64_t *d_frame, int32_t n,
                          int64_t n_ids, double lo, double hi, const double *edges, int32_t *d_pass, bool apply,
                          hipStream_t s)
{
    const size_t G = (size_t)n_ids;
    unsigned long long *sum;
    int32_t *count, *hist, *pass;
    size_t used = 0;
    const int rc = carve(SCR_STAGE_C, [&](Arena &ar) {
        sum = ar.take<unsigned long long>(G);
        count = ar.take<int32_t>(G), hist = ar.take<int32_t>(G * FA_BINS), pass = ar.take<int32_t>(G);
    }, &used);
    if (rc != PMI_OK) return rc;
    if (d_pass) pass = d_pass;
    PMI_HIP(hipMemsetAsync(sum, 0, used, s));
    Edges ed;
    for (int k = 0; k <= FA_BINS; ++k) ed.e[k] = edges[k];
    PMI_LAUNCH(fa_count_kernel, n, s, lab, shift, rows, d_frame, n, (int32_t)n_ids, ed, count, sum, hist);
    PMI_LAUNCH(fa_decide_kernel, n_ids, s, count, sum, hist, (int32_t)n_ids, lo, hi, pass);
    if (apply) PMI_LAUNCH(fa_apply_kernel, n, s, lab, shift, n, (int32_t)n_ids, pass);
    return PMI_OK;
}

template <int D>
static int counts_typed(const double *d_X, int32_t n, const double *lo, const double *hi, double r, double r2,
                        int32_t *d_counts, hipStream_t s)
{
    Work w;
    Tab t;
    int rc = prepare<D>(d_X, n, lo, hi, r, r2, w, t, s);
    if (rc != PMI_OK) return rc;
    PMI_LAUNCH(scatter_kernel, n, s, w.cnt, w.rows, n, d_counts);
    return PMI_OK;
}

template <int D>
static int smlm_typed(const double *d_X, int32_t n, const double *lo, const double *hi, double r, double r2,
                      int64_t min_locs, const int64_t *d_frame, double fa_lo, double fa_hi, const double *fa_edges,
                      int32_t *d_labels, hipStream_t s)
{
    Work w;
    Tab t;
    int rc = prepare<D>(d_X, n, lo, hi, r, r2, w, t, s);
    if (rc != PMI_OK) return rc;
    int32_t *lm = w.a, *state = w.b;
    PMI_LAUNCH(localmax_kernel<D>, n, s, t, w.cnt, min_locs, lm, w.flag);
    if ((rc = exclusive_scan_u32<const uint32_t>(w.flag, w.number, (size_t)n, s)) != PMI_OK) return rc;
    PMI_LAUNCH(fresh_kernel<D>, n, s, t, lm, state);
    PMI_LAUNCH(assign_kernel<D>, n, s, t, state, w.number, w.lab);
    int32_t pending = 1;
    for (int round = 0; round < MAX_ROUNDS && pending; ++round) {
        PMI_HIP(hipMemsetAsync(w.status + 1, 0, 4, s));
        PMI_LAUNCH(jump_kernel, n, s, w.lab, n, w.status + 1);
        PMI_HIP(hipMemcpyAsync(&pending, w.status + 1, 4, hipMemcpyDeviceToHost, s));
        PMI_HIP(hipStreamSynchronize(s));
    }
    if (pending) {
        set_error("pmi_cluster_smlm_dev: a chain of local maxima did not settle within %d rounds", MAX_ROUNDS);
        return PMI_ERR_HIP;
    }
    if ((rc = drop_small(w.lab, n, lm, min_locs, s)) != PMI_OK) return rc;
    if (d_frame) {
        uint32_t h_number = 0, h_flag = 0;
        PMI_HIP(hipMemcpyAsync(&h_number, w.number + (n - 1), 4, hipMemcpyDeviceToHost, s));
        PMI_HIP(hipMemcpyAsync(&h_flag, w.flag + (n - 1), 4, hipMemcpyDeviceToHost, s));
        PMI_HIP(hipStreamSynchronize(s));
        // id = label + 1: the rows without a label are checked like a label, as the reference does (to no effect)
        const int64_t n_ids = (int64_t)h_number + h_flag + 1;
        if ((rc = frame_analysis(w.lab, 1, w.rows, d_frame, n, n_ids, fa_lo, fa_hi, fa_edges, nullptr, true, s)) != PMI_OK)
            return rc;
    }
    PMI_LAUNCH(scatter_kernel, n, s, w.lab, w.rows, n, d_labels);
    return PMI_OK;
}

template <int D>
static int dbscan_typed(const double *d_X, int32_t n, const double *lo, const double *hi, double r, double r2,
                        int64_t min_samples, int64_t min_locs, int32_t *d_labels, hipStream_t s)
{
    Work w;
    Tab t;
    int rc = prepare<D>(d_X, n, lo, hi, r, r2, w, t, s);
    if (rc != PMI_OK) return rc;
    int32_t *parent = w.a, *root = w.b;
    PMI_LAUNCH(iota_kernel, n, s, parent, nullptr, n);
    PMI_LAUNCH(union_kernel<D>, n, s, t, w.cnt, min_samples, parent, w.status);
    PMI_LAUNCH(root_kernel, n, s, w.rows, w.cnt, min_samples, parent, n, root, w.flag);
    if ((rc = exclusive_scan_u32<const uint32_t>(w.flag, w.number, (size_t)n, s)) != PMI_OK) return rc;
    PMI_LAUNCH(dbscan_label_kernel<D>, n, s, t, root, w.number, w.lab);
    if ((rc = drop_small(w.lab, n, parent, min_locs, s)) != PMI_OK) return rc;
    PMI_LAUNCH(scatter_kernel, n, s, w.lab, w.rows, n, d_labels);
    int32_t h_status = 0;
    PMI_HIP(hipMemcpyAsync(&h_status, w.status, 4, hipMemcpyDeviceToHost, s));
    PMI_HIP(hipStreamSynchronize(s));
    if (h_status) {
        set_error("pmi_cluster_dbscan_dev: a union did not settle within its bound");
        return PMI_ERR_HIP;
    }
    return PMI_OK;
}

}  // namespace cluster
}  // namespace pmi

using namespace pmi;

extern "C" {

int pmi_cluster_counts_dev(const double *d_X, int dims, int64_t n, const double *lo, const double *hi, double r,
                           double r2, int32_t *d_counts, void *stream)
{
    int rc = cluster::check_args("pmi_cluster_counts_dev", d_X, dims, n, lo, hi, r, r2);
    if (rc) return rc;
    if (n == 0) return PMI_OK;
    if (!d_counts) { set_error("pmi_cluster_counts_dev: NULL output"); return PMI_ERR_ARG; }
    return dims == 2 ? cluster::counts_typed<2>(d_X, (int32_t)n, lo, hi, r, r2, d_counts, (hipStream_t)stream)
                     : cluster::counts_typed<3>(d_X, (int32_t)n, lo, hi, r, r2, d_counts, (hipStream_t)stream);
}

int pmi_cluster_smlm_dev(const double *d_X, int dims, int64_t n, const double *lo, const double *hi, double r,
                         double r2, int64_t min_locs, const int64_t *d_frame, double fa_lo, double fa_hi,
                         const double *fa_edges, int32_t *d_labels, void *stream)
{
    int rc = cluster::check_args("pmi_cluster_smlm_dev", d_X, dims, n, lo, hi, r, r2);
    if (rc) return rc;
    if (n == 0) return PMI_OK;
    if (!d_labels || (d_frame && !fa_edges)) { set_error("pmi_cluster_smlm_dev: NULL output or bin edges"); return PMI_ERR_ARG; }
    return dims == 2 ? cluster::smlm_typed<2>(d_X, (int32_t)n, lo, hi, r, r2, min_locs, d_frame, fa_lo, fa_hi, fa_edges,
                                              d_labels, (hipStream_t)stream)
                     : cluster::smlm_typed<3>(d_X, (int32_t)n, lo, hi, r, r2, min_locs, d_frame, fa_lo, fa_hi, fa_edges,
                                              d_labels, (hipStream_t)stream);
}

int pmi_cluster_dbscan_dev(const double *d_X, int dims, int64_t n, const double *lo, const double *hi, double r,
                           double r2, int64_t min_samples, int64_t min_locs, int32_t *d_labels, void *stream)
{
    int rc = cluster::check_args("pmi_cluster_dbscan_dev", d_X, dims, n, lo, hi, r, r2);
    if (rc) return rc;
    if (n == 0) return PMI_OK;
    if (!d_labels) { set_error("pmi_cluster_dbscan_dev: NULL output"); return PMI_ERR_ARG; }
    return dims == 2 ? cluster::dbscan_typed<2>(d_X, (int32_t)n, lo, hi, r, r2, min_samples, min_locs, d_labels,
                                                (hipStream_t)stream)
                     : cluster::dbscan_typed<3>(d_X, (int32_t)n, lo, hi, r, r2, min_samples, min_locs, d_labels,
                                                (hipStream_t)stream);
}

int pmi_cluster_frame_analysis_dev(const int32_t *d_ids, const int64_t *d_frame, int64_t n, int64_t n_ids, double fa_lo,
                                   double fa_hi, const double *fa_edges, int32_t *d_pass, void *stream)
{
    if (n < 0 || n > INT32_MAX - 1 || n_ids < 0 || n_ids > INT32_MAX - 1 || !fa_edges ||
        (n > 0 && (!d_ids || !d_frame)) || (n_ids > 0 && !d_pass)) {
        set_error("pmi_cluster_frame_analysis_dev: n = %lld, ids = %lld, or a NULL argument", (long long)n, (long long)n_ids);
        return PMI_ERR_ARG;
    }
    if (n_ids == 0) return PMI_OK;
    return cluster::frame_analysis(const_cast<int32_t *>(d_ids), 0, nullptr, d_frame, (int32_t)n, n_ids, fa_lo, fa_hi,
                                   fa_edges, d_pass, false, (hipStream_t)stream);
}

}  // extern "C"
