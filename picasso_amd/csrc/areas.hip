// areas.hip — the area (2-D) or volume (3-D) of every cluster of picasso.clusterer.cluster_areas
// (picasso/clusterer.py:1068-1169 _cluster_area, picasso/masking.py:408-446 threshold_otsu), count for count.
//
// One workgroup per group of the order of pmi_centers_order_dev (centers.hip); the points of a group are its rows of
// the x, y (and z / pixelsize) columns in their common type, held as float64 (exact for either type).
//
// Shape.  The smallest and largest coordinate per dimension (a block reduction) give np.arange(min, max + bin, bin) as
// NumPy builds it from scalars: the length ceil(((max + bin) - min) / bin) and next = min + bin in float32 when the
// points and the bin are both float32, else in float64; the edges are float64, edge 1 is next and edge i is
// start + i * (next - start).  They are never stored: a lane computes the edge it compares with.
//
// Image.  histogramdd: per dimension the number of edges <= v by bisection (searchsorted from the right), one less
// for a value on the last edge, the row dropped unless 1 <= index <= edges - 1; counts are 64-bit integer atomics,
// converted to float64 once (exact and free of any order).  The blur is scipy's correlate1d with the 17 symmetric
// weights at sigma 2, axis after axis from one copy of the image into the other: tmp = line[l] * w[8], then for
// j = 8 .. 1 tmp += (line[l - j] + line[l + j]) * w[8 - j], the line extended by half-sample-symmetric reflection.
// An image of at most PMI_AREAS_LDS_BINS bins has both copies in LDS (64 KiB: two workgroups per CU), a larger one
// in its slice of a global scratch; the arithmetic and its order are the same, so are the bits.
//
// Otsu.  np.histogram(image, 256): the range of the image (widened by 0.5 when it is constant), the index
// ((v - first) / (last - first)) * 256 truncated and corrected against the linspace edges i * step + first by one step
// down or up; one lane then runs the 256 sequential float32 and float64 sums of threshold_otsu, divisions by zero as
// IEEE gives them, and takes the first NaN or else the first maximum.  The count of image >= threshold over 4 or over
// 16 / 5 is evaluated in float64 and stored as float32.
//
// Every loop is bounded by the rows of the group, the bins of the image or a constant; every index into the image is
// below its bins, which the kernel checks against LDS or against the scratch it was given.  No contraction.
#include "rows_groups.h"

#pragma clang fp contract(off)

namespace pmi {
namespace areas {

using namespace rows;

constexpr int LDS_BINS = PMI_AREAS_LDS_BINS;
constexpr int RADIUS = 8;
constexpr int OTSU_BINS = 256;
static_assert(BLOCK == OTSU_BINS, "lane t clears bin t of the Otsu histogram");

// coordinate d of row i in the points' common type, as float64
__device__ __forceinline__ double coord(const pmi_areas_columns &c, int d, int32_t i)
{
    double v = c.type[d] == PMI_CENTERS_F32 ? (double)((const float *)c.data[d])[i] : ((const double *)c.data[d])[i];
    if (d == 2) {
        v = v / c.z_div;      // float32 / float32 rounded once is this quotient rounded to float32
        if (c.f32) v = (double)(float)v;
    }
    return v;
}

template <typename PT>
__device__ void arange_of(double mn, double mx, double bin, pmi_areas_geom *geom, int d)
{
    const PT start = (PT)mn, step = (PT)bin;
    const PT stop = (PT)mx + step;
    const PT q = (stop - start) / step;
    const PT next = start + step;
    const double v = __builtin_ceil((double)q);
    geom->start[d] = (double)start;
    geom->next[d] = (double)next;
    geom->len[d] = v != v ? -1 : (v >= 9.0e18 || v <= -9.0e18) ? -2 : v <= 0.0 ? 0 : (int64_t)v;
}

__global__ __launch_bounds__(BLOCK) void shape_kernel(pmi_areas_columns c, const int32_t *__restrict__ rows,
                                                      const int32_t *__restrict__ start, int32_t n, int32_t n_groups,
                                                      double bin_xy, double bin_z, int bin_f32,
                                                      pmi_areas_geom *__restrict__ geom)
{
    __shared__ double lo[BLOCK], hi[BLOCK];
    const int32_t g = blockIdx.x, t = threadIdx.x;
    if (g >= n_groups) return;
    int32_t a, b;
    run_of(start, g, n, &a, &b);
    for (int d = 0; d < c.dims; ++d) {
        double mn = __builtin_inf(), mx = -__builtin_inf();
        int nan = 0;
        for (int32_t p = a + t; p < b; p += BLOCK) {
            const int32_t i = rows[p];
            if (!row_ok(i, n)) continue;
            const double v = coord(c, d, i);
            nan |= v != v;
            mn = v < mn ? v : mn;
            mx = v > mx ? v : mx;
        }
        nan = __syncthreads_or(nan);
        lo[t] = mn, hi[t] = mx;
        __syncthreads();
        for (int w = BLOCK / 2; w > 0; w >>= 1) {
            if (t < w) {
                lo[t] = lo[t + w] < lo[t] ? lo[t + w] : lo[t];
                hi[t] = hi[t + w] > hi[t] ? hi[t + w] : hi[t];
            }
            __syncthreads();
        }
        if (t == 0) {
            const double nn = __builtin_nan("");
            mn = nan ? nn : lo[0], mx = nan ? nn : hi[0];      // np.min / np.max hand a NaN on
            const double bin = d == 2 ? bin_z : bin_xy;
            if (c.f32 && bin_f32) arange_of<float>(mn, mx, bin, geom + g, d);
            else arange_of<double>(mn, mx, bin, geom + g, d);
        }
        __syncthreads();
    }
    if (t == 0)
        for (int d = c.dims; d < 3; ++d) geom[g].start[d] = geom[g].next[d] = 0.0, geom[g].len[d] = 2;      // one bin
}

struct Axis {
    double start, next, delta;
    int32_t len;      // edges
};

__device__ __forceinline__ double edge_of(const Axis &ax, int32_t i)
{
    return i == 0 ? ax.start : i == 1 ? ax.next : ax.start + (double)i * ax.delta;
}

// position p of a line of n samples extended by reflection about its ends (d c b a | a b c d | d c b a)
__device__ __forceinline__ int32_t reflect(int32_t p, int32_t n)
{
    if ((uint32_t)p < (uint32_t)n) return p;
    int32_t m = p % (2 * n);
    if (m < 0) m += 2 * n;
    return m < n ? m : 2 * n - 1 - m;
}

template <bool LDS>
__global__ __launch_bounds__(BLOCK) void image_kernel(pmi_areas_columns c, const int32_t *__restrict__ rows,
                                                      const int32_t *__restrict__ start, int32_t n, int32_t n_groups,
                                                      const pmi_areas_geom *__restrict__ geom,
                                                      const int32_t *__restrict__ list, const int64_t *__restrict__ offset,
                                                      int32_t n_list, double *__restrict__ scratch, int64_t scratch_len,
                                                      const double *__restrict__ weights, float *__restrict__ area,
                                                      int32_t want_group, double *__restrict__ want_image)
{
    __shared__ double lds[LDS ? 2 * LDS_BINS : 1];
    __shared__ double lo[BLOCK], hi[BLOCK], mean2[OTSU_BINS], w[RADIUS + 1], s_first, s_last, s_thresh;
    __shared__ float weight2[OTSU_BINS];
    __shared__ uint32_t hist[OTSU_BINS], s_count;
    const int32_t k = blockIdx.x, t = threadIdx.x;
    if (k >= n_list) return;
    const int32_t g = list[k];
    if (g < 0 || g >= n_groups) return;
    int32_t a, b;
    run_of(start, g, n, &a, &b);

    Axis ax[3];
    int32_t nb[3];
    int64_t bins = 1;
    bool ok = true;
    for (int d = 0; d < 3; ++d) {
        const int64_t len = geom[g].len[d];
        ok = ok && len >= 2 && len <= (int64_t)PMI_AREAS_MAX_BINS + 1;
        ax[d].start = geom[g].start[d], ax[d].next = geom[g].next[d];
        ax[d].delta = ax[d].next - ax[d].start;
        ax[d].len = ok ? (int32_t)len : 2;
        nb[d] = ax[d].len - 1;
        bins *= nb[d];
        ok = ok && bins <= PMI_AREAS_MAX_BINS;
    }
    double *src, *dst;
    if (LDS) {
        ok = ok && bins <= LDS_BINS;
        src = lds, dst = lds + LDS_BINS;
    } else {
        const int64_t at = offset[k];
        ok = ok && at >= 0 && at + 2 * bins <= scratch_len;
        src = scratch + (ok ? at : 0), dst = src + (ok ? bins : 0);
    }
    if (!ok) return;      // uniform over the workgroup: the host never lists such a group
    const int32_t size = (int32_t)bins;

    // ---- histogram
    unsigned long long *count = (unsigned long long *)src;
    for (int32_t i = t; i < size; i += BLOCK) count[i] = 0ull;
    if (t <= RADIUS) w[t] = weights[t];
    __syncthreads();
    for (int32_t p = a + t; p < b; p += BLOCK) {
        const int32_t i = rows[p];
        if (!row_ok(i, n)) continue;
        int32_t at = 0;
        bool inside = true;
        for (int d = 0; d < c.dims; ++d) {
            const double v = coord(c, d, i);
            int32_t left = 0, right = ax[d].len;      // the number of edges <= v
            for (int it = 0; it < 32 && left < right; ++it) {
                const int32_t mid = left + ((right - left) >> 1);
                if (edge_of(ax[d], mid) <= v) left = mid + 1; else right = mid;
            }
            if (v == edge_of(ax[d], ax[d].len - 1)) --left;
            inside = inside && left >= 1 && left <= ax[d].len - 1;
            at = at * nb[d] + (left - 1);
        }
        if (inside && (uint32_t)at < (uint32_t)size) atomicAdd(count + at, 1ull);
    }
    __syncthreads();
    for (int32_t i = t; i < size; i += BLOCK) {
        const unsigned long long u = count[i];
        src[i] = (double)u;
    }
    __syncthreads();

    // ---- blur
    for (int d = 0; d < c.dims; ++d) {
        const int32_t len = nb[d];
        int32_t stride = 1;
        for (int e = d + 1; e < c.dims; ++e) stride *= nb[e];
        for (int32_t i = t; i < size; i += BLOCK) {
            const int32_t l = (i / stride) % len;
            const int32_t base = i - l * stride;
            double tmp = src[i] * w[RADIUS];
#pragma unroll
            for (int j = RADIUS; j >= 1; --j)
                tmp += (src[base + reflect(l - j, len) * stride] + src[base + reflect(l + j, len) * stride]) * w[RADIUS - j];
            dst[i] = tmp;
        }
        __syncthreads();
        double *swap = src;
        src = dst, dst = swap;
    }
    if (g == want_group && want_image)
        for (int32_t i = t; i < size; i += BLOCK) want_image[i] = src[i];

    // ---- np.histogram(image, 256)
    double mn = __builtin_inf(), mx = -__builtin_inf();
    for (int32_t i = t; i < size; i += BLOCK) {
        const double v = src[i];
        mn = v < mn ? v : mn;
        mx = v > mx ? v : mx;
    }
    lo[t] = mn, hi[t] = mx;
    hist[t] = 0;
    __syncthreads();
    for (int s = BLOCK / 2; s > 0; s >>= 1) {
        if (t < s) {
            lo[t] = lo[t + s] < lo[t] ? lo[t + s] : lo[t];
            hi[t] = hi[t + s] > hi[t] ? hi[t + s] : hi[t];
        }
        __syncthreads();
    }
    if (t == 0) {
        double first = lo[0], last = hi[0];
        if (first == last) first = first - 0.5, last = last + 0.5;
        s_first = first, s_last = last, s_count = 0;
    }
    __syncthreads();
    const double first = s_first, last = s_last;
    const double norm = last - first, step = (last - first) / (double)OTSU_BINS;
    auto bin_edge = [&](int32_t i) { return i >= OTSU_BINS ? last : (double)i * step + first; };
    for (int32_t i = t; i < size; i += BLOCK) {
        const double v = src[i];
        const double f = ((v - first) / norm) * (double)OTSU_BINS;
        int32_t q = f >= 0.0 && f <= (double)OTSU_BINS ? (int32_t)f : 0;
        if (q == OTSU_BINS) --q;
        if (v < bin_edge(q)) --q;
        q = q < 0 ? 0 : q;
        if (v >= bin_edge(q + 1) && q != OTSU_BINS - 1) ++q;
        atomicAdd(hist + q, 1u);
    }
    __syncthreads();

    // ---- threshold_otsu: sequential sums, one lane
    if (t == 0) {
        float wsum = 0.0f;
        double msum = 0.0;
        for (int i = OTSU_BINS - 1; i >= 0; --i) {
            const float cnt = (float)hist[i];
            const double center = (bin_edge(i) + bin_edge(i + 1)) / 2.0;
            wsum = wsum + cnt;
            msum = msum + (double)cnt * center;
            weight2[i] = wsum;
            mean2[i] = msum / (double)wsum;
        }
        wsum = 0.0f, msum = 0.0;
        int best = 0;
        double top = 0.0;
        bool done = false;
        for (int i = 0; i < OTSU_BINS - 1 && !done; ++i) {
            const float cnt = (float)hist[i];
            const double center = (bin_edge(i) + bin_edge(i + 1)) / 2.0;
            wsum = wsum + cnt;
            msum = msum + (double)cnt * center;
            const double mean1 = msum / (double)wsum;
            const double diff = mean1 - mean2[i + 1];
            const double var = (double)(wsum * weight2[i + 1]) * (diff * diff);
            if (i == 0 || !(var <= top)) {      // np.argmax: the first NaN, else the first maximum
                top = var, best = i;
                done = var != var;
            }
        }
        s_thresh = (bin_edge(best) + bin_edge(best + 1)) / 2.0;
    }
    __syncthreads();

    // ---- count
    const double thresh = s_thresh;
    uint32_t mine = 0;
    for (int32_t i = t; i < size; i += BLOCK) mine += src[i] >= thresh ? 1u : 0u;
    if (mine) atomicAdd(&s_count, mine);
    __syncthreads();
    if (t == 0) area[g] = (float)(c.dims == 3 ? (double)s_count / (16.0 / 5.0) : (double)s_count / 4.0);
}

static int check(const char *what, const pmi_areas_columns *cols, const int32_t *d_rows, const int32_t *d_start, int64_t n,
                 int64_t n_groups)
{
    const int rc = check_rows(what, n, n_groups, "groups");
    if (rc) return rc;
    if (!cols || (cols->dims != 2 && cols->dims != 3) || (n > 0 && (!d_rows || !d_start))) {
        set_error("%s: 2 or 3 dimensions, and no NULL table", what);
        return PMI_ERR_ARG;
    }
    for (int d = 0; d < cols->dims; ++d)
        if ((n > 0 && !cols->data[d]) || (cols->type[d] != PMI_CENTERS_F32 && cols->type[d] != PMI_CENTERS_F64)) {
            set_error("%s: column %d must be a float32 or float64 device column (code %d)", what, d, cols->type[d]);
            return PMI_ERR_ARG;
        }
    if (cols->dims == 3 && !(cols->z_div == cols->z_div)) {
        set_error("%s: the pixel size is not a number", what);
        return PMI_ERR_ARG;
    }
    return PMI_OK;
}

}  // namespace areas
}  // namespace pmi

using namespace pmi;

extern "C" {

int pmi_areas_lds_bins(void) { return PMI_AREAS_LDS_BINS; }
int pmi_areas_max_bins(void) { return PMI_AREAS_MAX_BINS; }

int pmi_areas_shape_dev(const pmi_areas_columns *cols, const int32_t *d_rows, const int32_t *d_start, int64_t n,
                        int64_t n_groups, double bin_xy, double bin_z, int bin_f32, pmi_areas_geom *d_geom, void *stream)
{
    int rc = areas::check("pmi_areas_shape_dev", cols, d_rows, d_start, n, n_groups);
    if (rc) return rc;
    if (n_groups > 0 && !d_geom) {
        set_error("pmi_areas_shape_dev: NULL output");
        return PMI_ERR_ARG;
    }
    if (n == 0 || n_groups == 0) return PMI_OK;
    hipStream_t s = (hipStream_t)stream;
    areas::shape_kernel<<<(unsigned)n_groups, rows::BLOCK, 0, s>>>(*cols, d_rows, d_start, (int32_t)n, (int32_t)n_groups,
                                                                  bin_xy, bin_z, bin_f32, d_geom);
    PMI_HIP(hipGetLastError());
    PMI_HIP(hipStreamSynchronize(s));
    return PMI_OK;
}

int pmi_areas_image_dev(const pmi_areas_columns *cols, const int32_t *d_rows, const int32_t *d_start, int64_t n,
                        int64_t n_groups, const pmi_areas_geom *d_geom, const int32_t *d_list, const int64_t *d_offset,
                        int64_t n_list, double *d_scratch, int64_t scratch_len, const double *d_weights, float *d_area,
                        int64_t want_group, double *d_want_image, void *stream)
{
    int rc = areas::check("pmi_areas_image_dev", cols, d_rows, d_start, n, n_groups);
    if (rc) return rc;
    if (n_list < 0 || n_list > n_groups || want_group >= n_groups ||
        (n_list > 0 && (!d_geom || !d_list || !d_weights || !d_area)) || (d_offset && (!d_scratch || scratch_len < 0))) {
        set_error("pmi_areas_image_dev: %lld listed groups of %lld, or a NULL table", (long long)n_list, (long long)n_groups);
        return PMI_ERR_ARG;
    }
    if (n == 0 || n_list == 0) return PMI_OK;
    hipStream_t s = (hipStream_t)stream;
    const int32_t want = want_group < 0 ? -1 : (int32_t)want_group;
    if (d_offset)
        areas::image_kernel<false><<<(unsigned)n_list, rows::BLOCK, 0, s>>>(
            *cols, d_rows, d_start, (int32_t)n, (int32_t)n_groups, d_geom, d_list, d_offset, (int32_t)n_list, d_scratch,
            scratch_len, d_weights, d_area, want, d_want_image);
    else
        areas::image_kernel<true><<<(unsigned)n_list, rows::BLOCK, 0, s>>>(
            *cols, d_rows, d_start, (int32_t)n, (int32_t)n_groups, d_geom, d_list, nullptr, (int32_t)n_list, nullptr, 0,
            d_weights, d_area, want, d_want_image);
    PMI_HIP(hipGetLastError());
    PMI_HIP(hipStreamSynchronize(s));
    return PMI_OK;
}

}  // extern "C"
