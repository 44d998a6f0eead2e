// g5m.hip — G5M molecular mapping in 2-D (picasso/g5m.py:820-902 _find_optimal_G5M_2D over every cluster at once,
// :482-567 G5M.fit for one K, :1829-2064 _convert_G5M_results).  All arithmetic is g5m_core.h's, which the host check
// (tests/g5m_host_driver.cpp) compiles too.
//
// Schedule.  The search over K is serial per cluster; clusters and initialisations are independent.  Round r fits K = r
// for every cluster still searching:
//   fit_kernel     one workgroup per (cluster, initialisation): kmeans++ from the host's draws, the EM loop, the valid
//                  components, the Sparrow check -> one record per initialisation.  Rows are strided over the lanes, the
//                  parameters live in LDS, and so do the responsibilities while n K <= PMI_G5M_LDS_RESP; beyond that (or
//                  with PMI_G5M_FORCE_SCRATCH) they live in a slice of the scratch arena.  The arithmetic does not know
//                  where they live: both paths give the same bits.
//   select_kernel  one workgroup per cluster: the best initialisation, set_parameters' weights, the Sparrow check of the
//                  model, its BIC, and the search state (best BIC, rounds without a better one, whether to go on).
// The host reads back four bytes per searching cluster per round and builds the next round's list.
//   assign_kernel  one workgroup per cluster: what _convert_G5M_results computes from the chosen model.
// A workgroup is 256 lanes: 4 wavefronts share the columns of the M step, and 32 KiB of responsibilities plus 8 KiB of
// parameters let three workgroups share the 160 KiB of a CU.  The kernels are bound by float64 exp (exp_cr: some 300
// float64 operations per value, 2 K of them per row and EM iteration), not by memory: a cluster's rows are read from cache.
#include <vector>

#include "pmi_common.h"
#include "g5m_core.h"

#pragma clang fp contract(off)

namespace pmi {
namespace g5m {

namespace {
__constant__ uint64_t k_exp_tab[PMI_GLIBC_EXP_TABLE_WORDS] = {
#include "libm_glibc_exp_table.inc"
};
}

constexpr int THREADS = 256;
constexpr int WAVES = THREADS / PMI_WAVE;
constexpr int LDS_RESP = PMI_G5M_LDS_RESP;
static_assert(MAX_K == PMI_G5M_MAX_K, "the header's limit");
static_assert(sizeof(Shared) + LDS_RESP * sizeof(double) + WAVES * sizeof(double) <= 48 * 1024, "three workgroups per CU");

struct BlockTeam {
    double *red;
    __device__ __forceinline__ int rank() const { return threadIdx.x; }
    __device__ __forceinline__ int size() const { return THREADS; }
    __device__ __forceinline__ int group() const { return threadIdx.x / PMI_WAVE; }
    __device__ __forceinline__ int groups() const { return WAVES; }
    __device__ __forceinline__ int glane() const { return threadIdx.x & (PMI_WAVE - 1); }
    __device__ __forceinline__ int gsize() const { return PMI_WAVE; }
    __device__ __forceinline__ void sync() const { __syncthreads(); }
    __device__ __forceinline__ double gsum(double v) const
    {
        for (int m = PMI_WAVE / 2; m >= 1; m >>= 1) v += __shfl_xor(v, m, PMI_WAVE);
        return v;
    }
    __device__ __forceinline__ double sum(double v) const
    {
        v = gsum(v);
        __syncthreads();
        if (glane() == 0) red[group()] = v;
        __syncthreads();
        double r = 0.0;
        for (int w = 0; w < WAVES; ++w) r += red[w];
        return r;
    }
    __device__ __forceinline__ void count(int32_t *p) const { atomicAdd(p, 1); }
};

// per cluster, four words of the caller's table
enum { TAB_MODEL = 0, TAB_FIRST = 1, TAB_UNIFORM = 2, TAB_STRIDE = 3, TAB_WORDS = 4 };

__global__ __launch_bounds__(THREADS) void fit_kernel(const double *__restrict__ x, const double *__restrict__ y,
                                                      const double *__restrict__ lp, const int64_t *__restrict__ offsets,
                                                      const int32_t *__restrict__ active, int n_init, int K,
                                                      const int64_t *__restrict__ table, const int32_t *__restrict__ first,
                                                      const double *__restrict__ uniform, const double *__restrict__ means_init,
                                                      Bounds b, const int64_t *__restrict__ resp_off, double *resp_scratch,
                                                      double *__restrict__ trials)
{
    __shared__ Shared s;
    __shared__ double lds_resp[LDS_RESP];
    __shared__ double red[WAVES];
    BlockTeam t{red};
    const int64_t a = blockIdx.x / n_init;
    const int ii = blockIdx.x % n_init;
    const int64_t c = active[a], lo = offsets[c];
    const Data d{x + lo, y + lo, lp + lo, (int)(offsets[c + 1] - lo)};
    double *resp = resp_off[a] >= 0 ? resp_scratch + resp_off[a] + (size_t)ii * d.n * K : lds_resp;
    const int64_t *tab = table + c * TAB_WORDS;
    int32_t f = first[tab[TAB_FIRST] + ii];
    f = f < 0 ? 0 : f >= d.n ? d.n - 1 : f;                               // a draw outside the cluster reads no other row
    kmeanspp(t, d, K, f, uniform + tab[TAB_UNIFORM] + (int64_t)ii * tab[TAB_STRIDE], resp, s);
    init_params(t, d, K, resp, s);
    if (means_init) {
        for (int k = t.rank(); k < K; k += t.size()) s.mx[k] = means_init[(c * K + k) * 2], s.my[k] = means_init[(c * K + k) * 2 + 1];
        t.sync();
    }
    fit_init(t, d, K, b, resp, s, trials + (size_t)blockIdx.x * trial_doubles(K));
}

struct Search { double best_bic; int32_t rounds, pad; };

__global__ __launch_bounds__(THREADS) void select_kernel(const double *__restrict__ x, const double *__restrict__ y,
                                                         const double *__restrict__ lp, const int64_t *__restrict__ offsets,
                                                         const int32_t *__restrict__ active, int n_init, int K,
                                                         const int64_t *__restrict__ table, const double *__restrict__ trials,
                                                         Search *search, int fixed, int max_rounds, int min_locs, double *model,
                                                         int32_t *imodel, int64_t total, int32_t *info, double *bic_out, int32_t *still)
{
    __shared__ Shared s;
    __shared__ double red[WAVES];
    BlockTeam t{red};
    const int64_t a = blockIdx.x, c = active[a], lo = offsets[c];
    const Data d{x + lo, y + lo, lp + lo, (int)(offsets[c + 1] - lo)};
    double bic;
    bool converged;
    const bool found = judge(t, d, K, trials + (size_t)a * n_init * trial_doubles(K), n_init, s, &bic, &converged);
    const int64_t m0 = table[c * TAB_WORDS + TAB_MODEL];
    const Model m{model + m0, model + total + m0, model + 2 * total + m0, model + 3 * total + m0, model + 4 * total + m0,
                  imodel + m0, imodel + total + m0};
    Search se = search[c];
    t.sync();                              // every lane has read the state before lane 0 writes it: all lanes decide `take` alike
    const bool take = found && (fixed || bic < se.best_bic);
    if (take) store(t, K, s, m);
    if (t.rank() == 0) {
        if (take) {
            info[c * 4] = K, info[c * 4 + 1] = s.n_valid, info[c * 4 + 2] = converged ? 1 : 0;
            bic_out[c] = bic;
            se.best_bic = bic, se.rounds = 0;
        } else {
            se.rounds++;
        }
        info[c * 4 + 3] = K;                                               // the last K tried
        search[c] = se;
        const int k_max = min(MAX_K, d.n / min_locs);
        still[a] = !fixed && K + 1 <= k_max && se.rounds < max_rounds;
    }
}

__global__ __launch_bounds__(THREADS) void assign_kernel(const double *__restrict__ x, const double *__restrict__ y,
                                                         const double *__restrict__ lp, const double *__restrict__ frame,
                                                         const int64_t *__restrict__ offsets, const int64_t *__restrict__ table,
                                                         const double *__restrict__ model, const int32_t *__restrict__ imodel,
                                                         int64_t total, const int32_t *__restrict__ info, const double *__restrict__ cols,
                                                         int n_cols, int64_t n_rows, int flags, const int64_t *__restrict__ work_off,
                                                         double *work, int32_t *label, double *loglik, double *stats, int32_t *events,
                                                         double *group_ll, double *col_means, double *out_lp, double *out_wlp)
{
    __shared__ Shared s;
    __shared__ double red[WAVES];
    BlockTeam t{red};
    const int64_t c = blockIdx.x, lo = offsets[c];
    const int K = info[c * 4], nv = info[c * 4 + 1];
    const int n = (int)(offsets[c + 1] - lo);
    if (K < 1 || nv < 1 || n < 1) return;                                   // no model: the caller's rows stay as they are
    const int64_t m0 = table[c * 2], p0 = table[c * 2 + 1];
    for (int k = t.rank(); k < K; k += t.size()) {
        s.w[k] = model[m0 + k], s.mx[k] = model[total + m0 + k], s.my[k] = model[2 * total + m0 + k];
        s.cov[k] = model[3 * total + m0 + k], s.pc[k] = model[4 * total + m0 + k];
        s.idx[k] = imodel[total + m0 + k];
    }
    if (t.rank() == 0) s.n_valid = nv;
    t.sync();
    constants(t, K, s);
    const Rows d{x + lo, y + lo, lp + lo, frame + lo, n, (flags & FLAG_QUAD_F32) != 0, (flags & FLAG_FRAME_U32) != 0};
    assign(t, d, K, s, work + work_off[c], k_exp_tab, label + lo, loglik + lo, out_lp ? out_lp + p0 : nullptr,
           out_wlp ? out_wlp + p0 : nullptr, stats + m0 * ASSIGN_STATS, events + m0, group_ll + c, cols ? cols + lo : nullptr, n_cols,
           (size_t)n_rows, col_means ? col_means + m0 : nullptr, (size_t)total);
}

// the rounds of a search (k_fixed == 0) or the one fit of k_fixed components; n_first / n_uniform: the lengths of the draw
// arrays where the caller knows them (the host forms), else -1
static int fit_impl(const char *who, const double *d_x, const double *d_y, const double *d_lp, const int64_t *d_offsets,
                    int64_t n_clusters, int64_t n_rows, const int64_t *d_table, const int32_t *d_first, int64_t n_first,
                    const double *d_uniform, int64_t n_uniform,
                    const double *d_means_init, int k_fixed, int min_locs, double sigma_lo, double sigma_hi, int max_rounds, int flags,
                    double *d_model, int32_t *d_imodel, int64_t total, int32_t *d_info, double *d_bic, pmi_g5m_progress progress,
                    void *user, hipStream_t s)
{
    if (n_clusters < 0 || n_clusters > INT32_MAX - 1 || n_rows < 0 || total < 0 || min_locs < 1 || max_rounds < 0 || k_fixed < 0 ||
        k_fixed > MAX_K || !(sigma_lo >= 0.0) || !(sigma_hi >= sigma_lo)) {
        set_error("%s: %lld clusters (below 2^31 - 1) of %lld rows, min_locs %d (>= 1), max_rounds %d (>= 0), K %d (0 .. %d), "
                  "sigma bounds %g <= %g (from 0)", who, (long long)n_clusters, (long long)n_rows, min_locs, max_rounds, k_fixed, MAX_K,
                  sigma_lo, sigma_hi);
        return PMI_ERR_ARG;
    }
    if (n_clusters == 0) return PMI_OK;
    if (!d_x || !d_y || !d_lp || !d_offsets || !d_table || !d_first || !d_uniform || !d_model || !d_imodel || !d_info || !d_bic) {
        set_error("%s: a NULL array", who);
        return PMI_ERR_ARG;
    }
    // the offsets and the table come down once: the host sizes the rounds from them
    std::vector<int64_t> off((size_t)n_clusters + 1), tab((size_t)n_clusters * TAB_WORDS);
    PMI_HIP(hipMemcpyAsync(off.data(), d_offsets, off.size() * sizeof(int64_t), hipMemcpyDeviceToHost, s));
    PMI_HIP(hipMemcpyAsync(tab.data(), d_table, tab.size() * sizeof(int64_t), hipMemcpyDeviceToHost, s));
    PMI_HIP(hipStreamSynchronize(s));
    std::vector<int32_t> k_max((size_t)n_clusters), act;
    int rounds_cap = 0;
    for (int64_t c = 0; c < n_clusters; ++c) {
        const int64_t lo = off[c], n = off[c + 1] - lo;
        if (off[0] != 0 || n < 0 || off[c + 1] > n_rows || n > INT32_MAX) {
            set_error("%s: the offsets must ascend from 0 to at most %lld, at most 2^31 - 1 rows apart", who, (long long)n_rows);
            return PMI_ERR_ARG;
        }
        int km = (int)std::min<int64_t>(MAX_K, n / min_locs);
        if (k_fixed) km = (n >= 1 && k_fixed <= n) ? k_fixed : 0;
        const int64_t m0 = tab[c * TAB_WORDS + TAB_MODEL];
        if (km > 0 && (m0 < 0 || m0 + km > total || tab[c * TAB_WORDS + TAB_FIRST] < 0 || tab[c * TAB_WORDS + TAB_UNIFORM] < 0 ||
                       tab[c * TAB_WORDS + TAB_STRIDE] < draws_needed(km))) {
            set_error("%s: cluster %lld needs %d components of the model arrays and %d uniforms per seed", who, (long long)c, km,
                      draws_needed(km));
            return PMI_ERR_ARG;
        }
        // a fit of km components reads max(km, 3) first draws and that many strides of uniforms
        const int64_t seeds = std::max(km, 3), stride = tab[c * TAB_WORDS + TAB_STRIDE];
        if (km > 0 && ((n_first >= 0 && tab[c * TAB_WORDS + TAB_FIRST] + seeds > n_first) ||
                       (n_uniform >= 0 && tab[c * TAB_WORDS + TAB_UNIFORM] + seeds * stride > n_uniform))) {
            set_error("%s: the draws of cluster %lld (%lld seeds of %lld uniforms) end outside the %lld first draws or the %lld uniforms",
                      who, (long long)c, (long long)seeds, (long long)stride, (long long)n_first, (long long)n_uniform);
            return PMI_ERR_ARG;
        }
        k_max[c] = km;
        rounds_cap = std::max(rounds_cap, km);
        if (km > 0 && (k_fixed || max_rounds > 0)) act.push_back((int32_t)c);
    }
    // the records of a round (a few hundred bytes per fit): the most a round can need, every eligible cluster still searching
    const bool force = (flags & FLAG_FORCE_SCRATCH) != 0;
    size_t trial_cap = 1;
    for (int K = k_fixed ? k_fixed : 1; K <= rounds_cap; ++K) {
        const size_t n_init = (size_t)std::max(K, 3);
        size_t count = 0;
        for (int32_t c : act) count += k_max[c] >= K ? 1 : 0;
        trial_cap = std::max(trial_cap, count * n_init * trial_doubles(K));
        if ((count * n_init) >> 31) { set_error("%s: more than 2^31 fits in one round", who); return PMI_ERR_ARG; }
    }
    Search *search;
    int32_t *d_active, *d_still;
    int64_t *d_resp_off;
    double *d_trials, *d_resp = nullptr;
    int rc = carve(SCR_STAGE_A, [&](Arena &ar) {
        search = ar.take<Search>((size_t)n_clusters);
        d_active = ar.take<int32_t>((size_t)n_clusters);
        d_still = ar.take<int32_t>((size_t)n_clusters);
        d_resp_off = ar.take<int64_t>((size_t)n_clusters);
        d_trials = ar.take<double>(trial_cap);
    });
    if (rc != PMI_OK) return rc;
    {
        std::vector<Search> init((size_t)n_clusters, Search{INFINITY, 0, 0});
        PMI_HIP(hipMemcpyAsync(search, init.data(), init.size() * sizeof(Search), hipMemcpyHostToDevice, s));
        PMI_HIP(hipMemsetAsync(d_info, 0, (size_t)n_clusters * 4 * sizeof(int32_t), s));
        std::vector<double> inf((size_t)n_clusters, INFINITY);
        PMI_HIP(hipMemcpyAsync(d_bic, inf.data(), inf.size() * sizeof(double), hipMemcpyHostToDevice, s));
        PMI_HIP(hipStreamSynchronize(s));                                   // the vectors go out of scope
    }
    const Bounds b{min_locs, sigma_lo * sigma_lo, sigma_hi * sigma_hi, (flags & FLAG_LP_ABS) ? 1 : 0};
    std::vector<int64_t> resp_off;
    std::vector<int32_t> still;
    struct Events {                      // destroyed on every way out
        hipEvent_t e0 = nullptr, e1 = nullptr;
        ~Events() { if (e0) (void)hipEventDestroy(e0); if (e1) (void)hipEventDestroy(e1); }
    } ev;
    hipEvent_t &e0 = ev.e0, &e1 = ev.e1;
    if (progress) { PMI_HIP(hipEventCreate(&e0)); PMI_HIP(hipEventCreate(&e1)); }
    for (int K = k_fixed ? k_fixed : 1; !act.empty(); ++K) {
        const int n_init = std::max(K, 3);
        resp_off.assign(act.size(), -1);
        size_t used = 0;
        for (size_t a = 0; a < act.size(); ++a) {
            const size_t n = (size_t)(off[act[a] + 1] - off[act[a]]);
            if (force || n * K > (size_t)LDS_RESP) { resp_off[a] = (int64_t)used; used += (size_t)n_init * n * K; }
        }
        // The responsibilities beyond LDS are sized for the clusters this round really fits, not for the worst round.
        // SCR_STAGE_B holds nothing else of this call and the last round has been synchronised, so the pointer of an
        // earlier round is simply dropped when the slot grows.
        if (used && (rc = carve(SCR_STAGE_B, [&](Arena &ar) { d_resp = ar.take<double>(used); })) != PMI_OK) return rc;
        PMI_HIP(hipMemcpyAsync(d_active, act.data(), act.size() * sizeof(int32_t), hipMemcpyHostToDevice, s));
        PMI_HIP(hipMemcpyAsync(d_resp_off, resp_off.data(), act.size() * sizeof(int64_t), hipMemcpyHostToDevice, s));
        if (progress) PMI_HIP(hipEventRecord(e0, s));
        fit_kernel<<<(unsigned)(act.size() * n_init), THREADS, 0, s>>>(d_x, d_y, d_lp, d_offsets, d_active, n_init, K, d_table, d_first,
                                                                       d_uniform, d_means_init, b, d_resp_off, d_resp, d_trials);
        PMI_HIP(hipGetLastError());
        select_kernel<<<(unsigned)act.size(), THREADS, 0, s>>>(d_x, d_y, d_lp, d_offsets, d_active, n_init, K, d_table, d_trials, search,
                                                               k_fixed ? 1 : 0, max_rounds, min_locs, d_model, d_imodel, total, d_info,
                                                               d_bic, d_still);
        PMI_HIP(hipGetLastError());
        if (progress) PMI_HIP(hipEventRecord(e1, s));
        still.resize(act.size());
        PMI_HIP(hipMemcpyAsync(still.data(), d_still, act.size() * sizeof(int32_t), hipMemcpyDeviceToHost, s));
        PMI_HIP(hipStreamSynchronize(s));
        if (progress) {
            float ms = 0.f;
            PMI_HIP(hipEventElapsedTime(&ms, e0, e1));
            progress(K, (int64_t)act.size(), (double)ms, user);
        }
        size_t kept = 0;
        for (size_t a = 0; a < act.size(); ++a)
            if (still[a] && k_max[act[a]] > K) act[kept++] = act[a];
        act.resize(kept);
    }
    return PMI_OK;
}

// the rows of a table, for the host forms: where the last cluster ends
static int64_t rows_of(const int64_t *offsets, int64_t n_clusters) { return n_clusters > 0 ? offsets[n_clusters] : 0; }

}  // namespace g5m
}  // namespace pmi

using namespace pmi;

extern "C" {

int pmi_g5m_limits(int *lds_resp, int *max_k, int *threads)
{
    if (lds_resp) *lds_resp = PMI_G5M_LDS_RESP;
    if (max_k) *max_k = PMI_G5M_MAX_K;
    if (threads) *threads = g5m::THREADS;
    return PMI_OK;
}

int pmi_g5m_fit_dev(const double *d_x, const double *d_y, const double *d_lp, const int64_t *d_offsets, int64_t n_clusters,
                    int64_t n_rows, const int64_t *d_table, const int32_t *d_first, const double *d_uniform, int min_locs,
                    double sigma_lo, double sigma_hi, int max_rounds, int flags, double *d_model, int32_t *d_imodel, int64_t total,
                    int32_t *d_info, double *d_bic, pmi_g5m_progress progress, void *user, void *stream)
{
    return g5m::fit_impl("pmi_g5m_fit_dev", d_x, d_y, d_lp, d_offsets, n_clusters, n_rows, d_table, d_first, -1, d_uniform, -1, nullptr, 0,
                         min_locs, sigma_lo, sigma_hi, max_rounds, flags, d_model, d_imodel, total, d_info, d_bic, progress, user,
                         (hipStream_t)stream);
}

int pmi_g5m_fit_fixed_dev(const double *d_x, const double *d_y, const double *d_lp, const int64_t *d_offsets, int64_t n_clusters,
                          int64_t n_rows, const int64_t *d_table, const int32_t *d_first, const double *d_uniform,
                          const double *d_means_init, int n_components, int min_locs, double sigma_lo, double sigma_hi, int flags,
                          double *d_model, int32_t *d_imodel, int64_t total, int32_t *d_info, double *d_bic, void *stream)
{
    if (n_components < 1) { set_error("pmi_g5m_fit_fixed_dev: %d components (1 .. %d)", n_components, PMI_G5M_MAX_K); return PMI_ERR_ARG; }
    return g5m::fit_impl("pmi_g5m_fit_fixed_dev", d_x, d_y, d_lp, d_offsets, n_clusters, n_rows, d_table, d_first, -1, d_uniform, -1,
                         d_means_init, n_components, min_locs, sigma_lo, sigma_hi, 0, flags, d_model, d_imodel, total, d_info, d_bic,
                         nullptr, nullptr, (hipStream_t)stream);
}

static int g5m_fit_host(bool fixed, const double *x, const double *y, const double *lp, const int64_t *offsets, int64_t n_clusters,
                        const int64_t *table, const int32_t *first, int64_t n_first, const double *uniform, int64_t n_uniform,
                        const double *means_init, int n_components, int min_locs, double sigma_lo, double sigma_hi, int max_rounds,
                        int flags, double *model, int32_t *imodel, int64_t total, int32_t *info, double *bic, pmi_g5m_progress progress,
                        void *user)
{
    const char *who = fixed ? "pmi_g5m_fit_fixed" : "pmi_g5m_fit";
    if (pmi_device_count() < 1) { set_error("no HIP device"); return PMI_ERR_NODEVICE; }
    if (n_clusters < 0 || n_first < 0 || n_uniform < 0 || total < 0 || (fixed && (n_components < 1 || n_components > PMI_G5M_MAX_K))) {
        set_error("%s: %lld clusters, %lld first draws, %lld uniforms, %lld components, K %d", who, (long long)n_clusters,
                  (long long)n_first, (long long)n_uniform, (long long)total, n_components);
        return PMI_ERR_ARG;
    }
    if (n_clusters == 0) return PMI_OK;
    if (!offsets || !x || !y || !lp || !table || !first || !uniform || !model || !imodel || !info || !bic) {
        set_error("%s: a NULL array", who);
        return PMI_ERR_ARG;
    }
    const int64_t n_rows = g5m::rows_of(offsets, n_clusters);
    if (n_rows < 0) { set_error("%s: the offsets must ascend from 0", who); return PMI_ERR_ARG; }
    double *d_x, *d_y, *d_lp, *d_uniform, *d_means = nullptr, *d_model, *d_bic;
    int64_t *d_offsets, *d_table;
    int32_t *d_first, *d_imodel, *d_info;
    Staged st(SCR_STAGE_C);             // the _dev form carves SCR_STAGE_A and SCR_STAGE_B
    st.add(d_x, (size_t)n_rows, x), st.add(d_y, (size_t)n_rows, y), st.add(d_lp, (size_t)n_rows, lp);
    st.add(d_offsets, (size_t)n_clusters + 1, offsets), st.add(d_table, (size_t)n_clusters * g5m::TAB_WORDS, table);
    st.add(d_first, (size_t)n_first, first), st.add(d_uniform, (size_t)n_uniform, uniform);
    if (means_init) st.add(d_means, (size_t)n_clusters * n_components * 2, means_init);
    st.add(d_model, (size_t)total * 5, nullptr, model), st.add(d_imodel, (size_t)total * 2, nullptr, imodel);
    st.add(d_info, (size_t)n_clusters * 4, nullptr, info), st.add(d_bic, (size_t)n_clusters, nullptr, bic);
    int rc;
    if ((rc = st.place()) != PMI_OK) return rc;
    // components no model fills read as zeros, alike in both forms
    PMI_HIP(hipMemset(d_model, 0, (size_t)total * 5 * sizeof(double)));
    PMI_HIP(hipMemset(d_imodel, 0, (size_t)total * 2 * sizeof(int32_t)));
    rc = g5m::fit_impl(who, d_x, d_y, d_lp, d_offsets, n_clusters, n_rows, d_table, d_first, n_first, d_uniform, n_uniform,
                       means_init ? d_means : nullptr,
                       fixed ? n_components : 0, min_locs, sigma_lo, sigma_hi, max_rounds, flags, d_model, d_imodel, total, d_info,
                       d_bic, progress, user, nullptr);
    if (rc != PMI_OK) return rc;
    return st.fetch();
}

int pmi_g5m_fit(const double *x, const double *y, const double *lp, const int64_t *offsets, int64_t n_clusters, const int64_t *table,
                const int32_t *first, int64_t n_first, const double *uniform, int64_t n_uniform, int min_locs, double sigma_lo,
                double sigma_hi, int max_rounds, int flags, double *model, int32_t *imodel, int64_t total, int32_t *info, double *bic,
                pmi_g5m_progress progress, void *user)
{
    return g5m_fit_host(false, x, y, lp, offsets, n_clusters, table, first, n_first, uniform, n_uniform, nullptr, 0, min_locs, sigma_lo,
                        sigma_hi, max_rounds, flags, model, imodel, total, info, bic, progress, user);
}

int pmi_g5m_fit_fixed(const double *x, const double *y, const double *lp, const int64_t *offsets, int64_t n_clusters,
                      const int64_t *table, const int32_t *first, int64_t n_first, const double *uniform, int64_t n_uniform,
                      const double *means_init, int n_components, int min_locs, double sigma_lo, double sigma_hi, int flags,
                      double *model, int32_t *imodel, int64_t total, int32_t *info, double *bic)
{
    return g5m_fit_host(true, x, y, lp, offsets, n_clusters, table, first, n_first, uniform, n_uniform, means_init, n_components,
                        min_locs, sigma_lo, sigma_hi, 0, flags, model, imodel, total, info, bic, nullptr, nullptr);
}

int pmi_g5m_assign_dev(const double *d_x, const double *d_y, const double *d_lp, const double *d_frame, const int64_t *d_offsets,
                       int64_t n_clusters, int64_t n_rows, const int64_t *d_table, const double *d_model, const int32_t *d_imodel,
                       int64_t total, const int32_t *d_info, const double *d_cols, int n_cols, int flags, int32_t *d_label,
                       double *d_loglik, double *d_stats, int32_t *d_events, double *d_group_ll, double *d_col_means, double *d_lp_out,
                       double *d_wlp_out, int64_t n_prob, void *stream)
{
    if (n_clusters < 0 || n_clusters > INT32_MAX - 1 || n_rows < 0 || total < 0 || n_cols < 0 || n_prob < 0) {
        set_error("pmi_g5m_assign_dev: %lld clusters (below 2^31 - 1) of %lld rows, %lld components, %d columns", (long long)n_clusters,
                  (long long)n_rows, (long long)total, n_cols);
        return PMI_ERR_ARG;
    }
    if (n_clusters == 0) return PMI_OK;
    if (!d_x || !d_y || !d_lp || !d_frame || !d_offsets || !d_table || !d_model || !d_imodel || !d_info || !d_label || !d_loglik ||
        !d_stats || !d_events || !d_group_ll || (n_cols > 0 && (!d_cols || !d_col_means))) {
        set_error("pmi_g5m_assign_dev: a NULL array");
        return PMI_ERR_ARG;
    }
    hipStream_t s = (hipStream_t)stream;
    std::vector<int64_t> off((size_t)n_clusters + 1), tab((size_t)n_clusters * 2), work_off((size_t)n_clusters);
    std::vector<int32_t> info((size_t)n_clusters * 4);
    PMI_HIP(hipMemcpyAsync(off.data(), d_offsets, off.size() * sizeof(int64_t), hipMemcpyDeviceToHost, s));
    PMI_HIP(hipMemcpyAsync(tab.data(), d_table, tab.size() * sizeof(int64_t), hipMemcpyDeviceToHost, s));
    PMI_HIP(hipMemcpyAsync(info.data(), d_info, info.size() * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    PMI_HIP(hipStreamSynchronize(s));
    size_t work = 0;
    for (int64_t c = 0; c < n_clusters; ++c) {
        const int64_t lo = off[c], n = off[c + 1] - lo;
        const int K = info[c * 4], nv = info[c * 4 + 1];
        if (off[0] != 0 || n < 0 || off[c + 1] > n_rows || n > INT32_MAX) {
            set_error("pmi_g5m_assign_dev: the offsets must ascend from 0 to at most %lld", (long long)n_rows);
            return PMI_ERR_ARG;
        }
        work_off[c] = (int64_t)work;
        if (K < 1 || nv < 1 || n < 1) continue;
        if (K > PMI_G5M_MAX_K || nv > K || tab[c * 2] < 0 || tab[c * 2] + K > total ||
            ((d_lp_out || d_wlp_out) && (tab[c * 2 + 1] < 0 || tab[c * 2 + 1] + n * nv > n_prob))) {
            set_error("pmi_g5m_assign_dev: cluster %lld: %d components, %d valid, outside the model or probability arrays", (long long)c, K, nv);
            return PMI_ERR_ARG;
        }
        work += 2 * (size_t)n * nv;
    }
    int64_t *d_work_off;
    double *d_work;
    int rc = carve(SCR_STAGE_A, [&](Arena &ar) { d_work_off = ar.take<int64_t>((size_t)n_clusters); d_work = ar.take<double>(work ? work : 1); });
    if (rc != PMI_OK) return rc;
    PMI_HIP(hipMemcpyAsync(d_work_off, work_off.data(), work_off.size() * sizeof(int64_t), hipMemcpyHostToDevice, s));
    g5m::assign_kernel<<<(unsigned)n_clusters, g5m::THREADS, 0, s>>>(d_x, d_y, d_lp, d_frame, d_offsets, d_table, d_model, d_imodel, total,
                                                                     d_info, d_cols, n_cols, n_rows, flags, d_work_off, d_work, d_label,
                                                                     d_loglik, d_stats, d_events, d_group_ll, d_col_means, d_lp_out,
                                                                     d_wlp_out);
    PMI_HIP(hipGetLastError());
    PMI_HIP(hipStreamSynchronize(s));
    return PMI_OK;
}

int pmi_g5m_assign(const double *x, const double *y, const double *lp, const double *frame, const int64_t *offsets, int64_t n_clusters,
                   const int64_t *table, const double *model, const int32_t *imodel, int64_t total, const int32_t *info,
                   const double *cols, int n_cols, int flags, int32_t *label, double *loglik, double *stats, int32_t *events,
                   double *group_ll, double *col_means, double *lp_out, double *wlp_out, int64_t n_prob)
{
    if (pmi_device_count() < 1) { set_error("no HIP device"); return PMI_ERR_NODEVICE; }
    if (n_clusters < 0 || total < 0 || n_cols < 0 || n_prob < 0) { set_error("pmi_g5m_assign: a negative count"); return PMI_ERR_ARG; }
    if (n_clusters == 0) return PMI_OK;
    if (!offsets || !x || !y || !lp || !frame || !table || !model || !imodel || !info || !label || !loglik || !stats || !events ||
        !group_ll || (n_cols > 0 && (!cols || !col_means))) {
        set_error("pmi_g5m_assign: a NULL array");
        return PMI_ERR_ARG;
    }
    const int64_t n_rows = g5m::rows_of(offsets, n_clusters);
    if (n_rows < 0) { set_error("pmi_g5m_assign: the offsets must ascend from 0"); return PMI_ERR_ARG; }
    double *d_x, *d_y, *d_lp, *d_frame, *d_model, *d_cols, *d_loglik, *d_stats, *d_group_ll, *d_col_means, *d_lp_out = nullptr, *d_wlp_out = nullptr;
    int64_t *d_offsets, *d_table;
    int32_t *d_imodel, *d_info, *d_label, *d_events;
    Staged in(SCR_STAGE_C), out(SCR_STAGE_D);      // the _dev form carves SCR_STAGE_A
    in.add(d_x, (size_t)n_rows, x), in.add(d_y, (size_t)n_rows, y), in.add(d_lp, (size_t)n_rows, lp), in.add(d_frame, (size_t)n_rows, frame);
    in.add(d_offsets, (size_t)n_clusters + 1, offsets), in.add(d_table, (size_t)n_clusters * 2, table);
    in.add(d_model, (size_t)total * 5, model), in.add(d_imodel, (size_t)total * 2, imodel), in.add(d_info, (size_t)n_clusters * 4, info);
    in.add(d_cols, (size_t)n_cols * n_rows, cols);
    // rows and components without a model keep what the caller's arrays hold: they go up and come back
    out.add(d_label, (size_t)n_rows, label, label), out.add(d_loglik, (size_t)n_rows, loglik, loglik);
    out.add(d_stats, (size_t)total * g5m::ASSIGN_STATS, stats, stats), out.add(d_events, (size_t)total, events, events);
    out.add(d_group_ll, (size_t)n_clusters, group_ll, group_ll), out.add(d_col_means, (size_t)n_cols * total, col_means, col_means);
    if (lp_out) out.add(d_lp_out, (size_t)n_prob, lp_out, lp_out);
    if (wlp_out) out.add(d_wlp_out, (size_t)n_prob, wlp_out, wlp_out);
    int rc;
    if ((rc = in.place()) != PMI_OK || (rc = out.place()) != PMI_OK) return rc;
    rc = pmi_g5m_assign_dev(d_x, d_y, d_lp, d_frame, d_offsets, n_clusters, n_rows, d_table, d_model, d_imodel, total, d_info,
                            n_cols ? d_cols : nullptr, n_cols, flags, d_label, d_loglik, d_stats, d_events, d_group_ll,
                            n_cols ? d_col_means : nullptr, d_lp_out, d_wlp_out, n_prob, nullptr);
    if (rc != PMI_OK) return rc;
    return out.fetch();
}

}  // extern "C"
