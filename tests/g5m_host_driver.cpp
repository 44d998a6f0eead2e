// Host build of csrc/g5m_core.h for tests/test_g5m_host.py and tools/time_g5m.py: the same kmeans++ / EM / Sparrow / BIC /
// assignment the kernels of csrc/g5m.hip are compiled from, with a team of one lane, so every sum runs in row order.
// Built with -ffp-contract=off; with -DG5M_HOST_MAIN it is a stand-alone program that reads one case file (for the
// sanitizer run).  The argument lists follow pmi_g5m_fit / pmi_g5m_fit_fixed / pmi_g5m_assign.
#include <algorithm>
#include <atomic>
#include <cstdio>
#include <thread>
#include <vector>

#include "g5m_core.h"

using namespace pmi::g5m;

static const uint64_t k_exp_tab[PMI_GLIBC_EXP_TABLE_WORDS] = {
#include "libm_glibc_exp_table.inc"
};

struct OneLane {
    int rank() const { return 0; }
    int size() const { return 1; }
    int group() const { return 0; }
    int groups() const { return 1; }
    int glane() const { return 0; }
    int gsize() const { return 1; }
    void sync() const {}
    double gsum(double v) const { return v; }
    double sum(double v) const { return v; }
    void count(int32_t *p) const { ++*p; }
};

// one cluster: the search (k_fixed == 0) or the one fit
static void fit_cluster(const Data &d, const int64_t *tab, const int32_t *first, const double *uniform, const double *means_init,
                        int k_fixed, const Bounds &b, int max_rounds, const Model &m, int32_t *info, double *bic_out)
{
    OneLane t;
    std::vector<Shared> sh(1);
    Shared &s = sh[0];
    int k_max = std::min(MAX_K, d.n / b.min_locs);
    if (k_fixed) k_max = d.n >= 1 && k_fixed <= d.n ? k_fixed : 0;
    double best_bic = INFINITY;
    int rounds = 0;
    info[0] = info[1] = info[2] = info[3] = 0;
    *bic_out = INFINITY;
    std::vector<double> resp, trials;
    for (int K = k_fixed ? k_fixed : 1; K <= k_max && (k_fixed || rounds < max_rounds); ++K) {
        const int n_init = std::max(K, 3);
        resp.assign((size_t)d.n * K, 0.0);
        trials.assign((size_t)n_init * trial_doubles(K), 0.0);
        for (int ii = 0; ii < n_init; ++ii) {
            int32_t f = first[tab[1] + ii];
            f = f < 0 ? 0 : f >= d.n ? d.n - 1 : f;
            kmeanspp(t, d, K, f, uniform + tab[2] + (int64_t)ii * tab[3], resp.data(), s);
            init_params(t, d, K, resp.data(), s);
            if (means_init)
                for (int k = 0; k < K; ++k) s.mx[k] = means_init[2 * k], s.my[k] = means_init[2 * k + 1];
            fit_init(t, d, K, b, resp.data(), s, trials.data() + (size_t)ii * trial_doubles(K));
        }
        double bic;
        bool converged;
        const bool found = judge(t, d, K, trials.data(), n_init, s, &bic, &converged);
        if (found && (k_fixed || bic < best_bic)) {
            store(t, K, s, m);
            info[0] = K, info[1] = s.n_valid, info[2] = converged ? 1 : 0;
            *bic_out = bic;
            best_bic = bic, rounds = 0;
        } else {
            ++rounds;
        }
        info[3] = K;
        if (k_fixed) break;
    }
}

template <class F>
static void over_clusters(int64_t n, int threads, F &&f)
{
    if (threads <= 1) { for (int64_t c = 0; c < n; ++c) f(c); return; }
    std::atomic<int64_t> next{0};
    std::vector<std::thread> pool;
    for (int w = 0; w < threads; ++w)
        pool.emplace_back([&] { for (int64_t c; (c = next.fetch_add(1)) < n;) f(c); });
    for (auto &th : pool) th.join();
}

extern "C" {

// the header's log of n arguments
void g5m_host_log(const double *x, int64_t n, double *out)
{
    for (int64_t i = 0; i < n; ++i) out[i] = log_(x[i]);
}

void g5m_host_fit(const double *x, const double *y, const double *lp, const int64_t *offsets, int64_t n_clusters, const int64_t *table,
                  const int32_t *first, const double *uniform, const double *means_init, int k_fixed, int min_locs, double sigma_lo,
                  double sigma_hi, int max_rounds, int flags, double *model, int32_t *imodel, int64_t total, int32_t *info, double *bic,
                  int threads)
{
    const Bounds b{min_locs, sigma_lo * sigma_lo, sigma_hi * sigma_hi, (flags & FLAG_LP_ABS) ? 1 : 0};
    over_clusters(n_clusters, threads, [&](int64_t c) {
        const int64_t lo = offsets[c], m0 = table[c * 4];
        const Data d{x + lo, y + lo, lp + lo, (int)(offsets[c + 1] - lo)};
        const Model m{model + m0, model + total + m0, model + 2 * total + m0, model + 3 * total + m0, model + 4 * total + m0,
                      imodel + m0, imodel + total + m0};
        fit_cluster(d, table + c * 4, first, uniform, means_init ? means_init + c * k_fixed * 2 : nullptr, k_fixed, b, max_rounds, m,
                    info + c * 4, bic + c);
    });
}

void g5m_host_assign(const double *x, const double *y, const double *lp, const double *frame, const int64_t *offsets, int64_t n_clusters,
                     const int64_t *table, const double *model, const int32_t *imodel, int64_t total, const int32_t *info,
                     const double *cols, int n_cols, int flags, int32_t *label, double *loglik, double *stats, int32_t *events,
                     double *group_ll, double *col_means, double *lp_out, double *wlp_out, int threads)
{
    const int64_t n_rows = offsets[n_clusters];
    over_clusters(n_clusters, threads, [&](int64_t c) {
        OneLane t;
        const int64_t lo = offsets[c], m0 = table[c * 2], p0 = table[c * 2 + 1];
        const int K = info[c * 4], nv = info[c * 4 + 1], n = (int)(offsets[c + 1] - lo);
        if (K < 1 || nv < 1 || n < 1) return;
        std::vector<Shared> sh(1);
        Shared &s = sh[0];
        for (int k = 0; k < K; ++k) {
            s.w[k] = model[m0 + k], s.mx[k] = model[total + m0 + k], s.my[k] = model[2 * total + m0 + k];
            s.cov[k] = model[3 * total + m0 + k], s.pc[k] = model[4 * total + m0 + k], s.idx[k] = imodel[total + m0 + k];
        }
        s.n_valid = nv;
        constants(t, K, s);
        std::vector<double> work(2 * (size_t)n * nv);
        const Rows d{x + lo, y + lo, lp + lo, frame + lo, n, (flags & FLAG_QUAD_F32) != 0, (flags & FLAG_FRAME_U32) != 0};
        assign(t, d, K, s, work.data(), k_exp_tab, label + lo, loglik + lo, lp_out ? lp_out + p0 : nullptr, wlp_out ? wlp_out + p0 : nullptr,
               stats + m0 * ASSIGN_STATS, events + m0, group_ll + c, cols ? cols + lo : nullptr, n_cols, (size_t)n_rows,
               col_means ? col_means + m0 : nullptr, (size_t)total);
    });
}

}  // extern "C"

#ifdef G5M_HOST_MAIN
// g5m_host_driver FILE: a flat binary of one table (written by tests/test_g5m_host.py): a header of int64
// (n_clusters, n_rows, total, n_first, n_uniform, n_cols, min_locs, max_rounds, flags, k_fixed), two float64 (sigma bounds), then
// offsets, table (4 per cluster), first (int32, padded to 8 bytes), uniform, x, y, lp, frame, cols.  Runs the search (or
// the fixed fit) and the assignment, prints a checksum.
template <typename T>
static std::vector<T> take(FILE *f, size_t n)
{
    std::vector<T> v(n ? n : 1);
    if (n && fread(v.data(), sizeof(T), n, f) != n) { fprintf(stderr, "short file\n"); exit(2); }
    return v;
}

int main(int argc, char **argv)
{
    if (argc != 2) { fprintf(stderr, "usage: %s FILE\n", argv[0]); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    const auto h = take<int64_t>(f, 10);
    const auto sig = take<double>(f, 2);
    const int64_t C = h[0], N = h[1], total = h[2], n_first = h[3], n_uniform = h[4], n_cols = h[5];
    const auto offsets = take<int64_t>(f, C + 1), table = take<int64_t>(f, C * 4);
    const auto first = take<int32_t>(f, (n_first + 1) / 2 * 2);
    const auto uniform = take<double>(f, n_uniform), x = take<double>(f, N), y = take<double>(f, N), lp = take<double>(f, N),
               frame = take<double>(f, N), cols = take<double>(f, n_cols * N);
    fclose(f);
    std::vector<double> model(5 * total + 1), bic(C + 1), loglik(N + 1), stats(ASSIGN_STATS * total + 1), group_ll(C + 1), col_means(n_cols * total + 1);
    std::vector<int32_t> imodel(2 * total + 1), info(4 * C + 1), label(N + 1), events(total + 1);
    g5m_host_fit(x.data(), y.data(), lp.data(), offsets.data(), C, table.data(), first.data(), uniform.data(), nullptr, (int)h[9], (int)h[6],
                 sig[0], sig[1], (int)h[7], (int)h[8], model.data(), imodel.data(), total, info.data(), bic.data(), 1);
    std::vector<int64_t> tab2(2 * C + 1);
    for (int64_t c = 0; c < C; ++c) tab2[2 * c] = table[4 * c], tab2[2 * c + 1] = 0;
    g5m_host_assign(x.data(), y.data(), lp.data(), frame.data(), offsets.data(), C, tab2.data(), model.data(), imodel.data(), total,
                    info.data(), n_cols ? cols.data() : nullptr, (int)n_cols, (int)h[8], label.data(), loglik.data(), stats.data(),
                    events.data(), group_ll.data(), n_cols ? col_means.data() : nullptr, nullptr, nullptr, 1);
    long long ks = 0;
    for (int64_t c = 0; c < C; ++c) ks += info[4 * c] * 100 + info[4 * c + 1];
    printf("clusters %lld chosen %lld\n", (long long)C, ks);
    return 0;
}
#endif
