// g5m_core.h — the arithmetic of G5M in 2-D (picasso/g5m.py, v0.10.3), shared by the kernels of csrc/g5m.hip and the
// host-side check of them (tests/g5m_host_driver.cpp).  float64 throughout, exp from exp_cr.h, one log (log_ below) on the
// host and on the device; the including file switches contraction off.
//
// Restated here, with the lines of picasso/g5m.py:
//   kmeanspp        :212-318   _euclidean_distances, _kmeans_plusplus (the draws come from the host: first index, uniforms)
//   init_params     :695-727   _initialize_G5M_2D
//   estimate        :1699-1740 _estimate_gaussian_parameters_diag_cov (reg_covar 1e-6, nk + 10 eps), :730-741
//   e_step          :744-768   _estimate_log_gaussian_prob_2D, _e_step_2D, :105-118 _logsumexp_axis1
//   m_step_tail     :771-817   _m_step_2D ("local" and "abs" bounds)
//   fit_init        :2126-2298 the EM loop of _fit_G5M for one initialisation (max_iter 100, |change| < 1e-3, n = round(w N))
//   pick_init       :2289-2296 the best initialisation (strict >: the first of equal ones wins)
//   resolved        :630-692   _check_G5M_resolution_2D (picasso/lib.py:1243-1260 find_local_minima)
//   judge           :455-462, :1037-1043 bic, n_parameters, and one round of :820-902 _find_optimal_G5M_2D
//   assign          :1829-2064 _convert_G5M_results, per cluster
//
// Every function is written once over a Team: the lanes that share one (cluster, initialisation).  A Team gives
//   rank(), size()            this lane among the lanes that stride over rows
//   group(), groups()         this lane's column group (a wavefront) and their number; glane(), gsize() inside it
//   gsum(v)                   the sum of v over the lanes of the group, the same bits in every lane
//   sum(v)                    the sum of v over the whole team, the same bits in every lane (a barrier on both sides)
//   sync()                    a barrier
//   count(p)                  ++*p by one lane (integers: the order does not matter)
// On the device a Team is a workgroup (g5m.hip); in the host driver it is one lane, so every sum runs in row order.
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "exp_cr.h"
#include "libm_glibc.h"
#include "segment_stats.h"

#if defined(__HIPCC__)
#define PMI_G5M_FN __host__ __device__ __forceinline__
#define PMI_G5M_T __device__ __forceinline__
#else
#define PMI_G5M_FN static inline
#define PMI_G5M_T static inline
#endif

namespace pmi {
namespace g5m {

constexpr int MAX_K = 100;              // N_COMPONENTS_MAX
constexpr int MAX_ITER = 100;
constexpr int LINE = 40;                // points between two components in the Sparrow check
constexpr int MAX_TRIALS = 6;           // 2 + int(log 100)
constexpr double REG_COVAR = 1e-6, TOL = 1e-3;
constexpr double EPS10 = 10.0 * 2.220446049250313e-16;
constexpr double LOG_2PI = 1.8378770664093453;      // np.log(2 * np.pi)
constexpr double TWO_PI = 6.283185307179586;
constexpr double SQRT_2 = 1.4142135623730951;
enum { FLAG_LP_ABS = 1, FLAG_FORCE_SCRATCH = 2, FLAG_QUAD_F32 = 4, FLAG_FRAME_U32 = 8 };

// log(x): x = 2^k m with m in [sqrt(1/2), sqrt 2), log m = 2 atanh(s), s = (m - 1) / (m + 1), |s| < 0.1716
PMI_G5M_FN double log_(double x)
{
    if (!(x > 0.0)) return x == 0.0 ? -INFINITY : NAN;
    if (x == INFINITY) return x;
    uint64_t u;
    int k = 0;
    memcpy(&u, &x, 8);
    if ((u >> 52) == 0) { x *= 0x1p54; memcpy(&u, &x, 8); k = -54; }
    k += (int)(u >> 52) - 1023;
    u = (u & 0x000fffffffffffffull) | 0x3ff0000000000000ull;
    double m;
    memcpy(&m, &u, 8);
    if (m > SQRT_2) { m *= 0.5; k += 1; }
    const double f = m - 1.0, s = f / (m + 1.0), z = s * s;
    double p = 1.0 / 25.0;
    p = p * z + 1.0 / 23.0, p = p * z + 1.0 / 21.0, p = p * z + 1.0 / 19.0, p = p * z + 1.0 / 17.0, p = p * z + 1.0 / 15.0;
    p = p * z + 1.0 / 13.0, p = p * z + 1.0 / 11.0, p = p * z + 1.0 / 9.0, p = p * z + 1.0 / 7.0, p = p * z + 1.0 / 5.0;
    p = p * z + 1.0 / 3.0;
    // log m = 2 s + 2 s z p = f - s (f - 2 z p)   (f - s f = 2 s: fdlibm's arrangement, the large part f is exact)
    const double lm = f - s * (f - 2.0 * z * p);
    const double kd = (double)k;
    return kd * 0x1.62e42fee00000p-1 + (lm + kd * 0x1.a39ef35793c76p-33);
}

// int(np.log(K)) for K in 1 .. 100 (e, e^2, e^3, e^4 = 2.7, 7.4, 20.1, 54.6: no integer near a boundary)
PMI_G5M_FN int local_trials(int K) { return 2 + (K >= 55 ? 4 : K >= 21 ? 3 : K >= 8 ? 2 : K >= 3 ? 1 : 0); }
// uniforms one seed needs for K components
PMI_G5M_FN int draws_needed(int K) { return (K - 1) * local_trials(K); }

struct Data { const double *x, *y, *lp; int n; };
struct Bounds { int min_locs; double min_cov, max_cov; int lp_abs; };

// what a team shares (LDS on the device): MAX_K of each
struct Shared {
    double w[MAX_K], mx[MAX_K], my[MAX_K], cov[MAX_K], pc[MAX_K];      // the parameters
    double mlp[MAX_K];                                                  // resp-weighted lp per component
    double logw[MAX_K], logdet[MAX_K], prec[MAX_K];                     // per-component constants of the e step
    int32_t idx[MAX_K];                                                 // kmeans++ indices, later the valid components
    int32_t nloc[MAX_K];                                                // round(w N)
    int32_t cand[MAX_TRIALS];
    int32_t n_valid, fails;
};

// _estimate_log_gaussian_prob_2D + log(weight) of one row and one component; f32: the quadratic form is accumulated in a
// float32 array (X is float32 in _convert_G5M_results)
PMI_G5M_FN double wlog_prob(double x, double y, double mx, double my, double prec, double logdet, double logw, bool f32, bool weighted)
{
    const double dx = x - mx, dy = y - my;
    double q;
    if (f32) { float a = (float)(0.0 + dx * dx * prec); a = (float)((double)a + dy * dy * prec); q = (double)a; }
    else { q = 0.0 + dx * dx * prec; q += dy * dy * prec; }
    const double v = -0.5 * (2.0 * LOG_2PI + q) + logdet;
    return weighted ? v + logw : v;
}

// the per-component constants of the e step of components [0, K)
template <class T>
PMI_G5M_T void constants(T &t, int K, Shared &s)
{
    for (int k = t.rank(); k < K; k += t.size()) {
        s.logdet[k] = 2.0 * log_(s.pc[k]);
        s.prec[k] = s.pc[k] * s.pc[k];
        s.logw[k] = log_(s.w[k]);
    }
    t.sync();
}

// _e_step_2D: resp (n x K, row-major) becomes exp(log_resp); -> mean(log_prob_norm)
template <class T>
PMI_G5M_T double e_step(T &t, const Data &d, int K, double *resp, Shared &s)
{
    constants(t, K, s);
    double acc = 0.0;
    for (int i = t.rank(); i < d.n; i += t.size()) {
        double *r = resp + (size_t)i * K;
        double mxv = -INFINITY;
        for (int k = 0; k < K; ++k) {
            const double v = wlog_prob(d.x[i], d.y[i], s.mx[k], s.my[k], s.prec[k], s.logdet[k], s.logw[k], false, true);
            r[k] = v;
            mxv = v > mxv ? v : mxv;
        }
        double es = 0.0;
        for (int k = 0; k < K; ++k) es += exp_cr(r[k] - mxv);
        const double lpn = log_(es) + mxv;
        for (int k = 0; k < K; ++k) r[k] = exp_cr(r[k] - lpn);
        acc += lpn;
    }
    return t.sum(acc) / (double)d.n;
}

// _estimate_gaussian_parameters_2D of resp: s.w = nk, s.mx, s.my, s.cov, and s.mlp = sum(resp lp) / sum(resp)
template <class T>
PMI_G5M_T void estimate(T &t, const Data &d, int K, const double *resp, Shared &s)
{
    for (int k = t.group(); k < K; k += t.groups()) {
        double s0 = 0.0, sx = 0.0, sy = 0.0, sl = 0.0;
        for (int i = t.glane(); i < d.n; i += t.gsize()) {
            const double r = resp[(size_t)i * K + k];
            s0 += r, sx += r * d.x[i], sy += r * d.y[i], sl += r * d.lp[i];
        }
        s0 = t.gsum(s0), sx = t.gsum(sx), sy = t.gsum(sy), sl = t.gsum(sl);
        const double nk = s0 + EPS10, mx = sx / nk, my = sy / nk;
        double cx = 0.0, cy = 0.0;
        for (int i = t.glane(); i < d.n; i += t.gsize()) {
            const double r = resp[(size_t)i * K + k], dx = d.x[i] - mx, dy = d.y[i] - my;
            cx += r * (dx * dx), cy += r * (dy * dy);
        }
        cx = t.gsum(cx), cy = t.gsum(cy);
        if (t.glane() == 0) {
            s.w[k] = nk, s.mx[k] = mx, s.my[k] = my;
            s.cov[k] = ((0.0 + (cx / nk + REG_COVAR)) + (cy / nk + REG_COVAR)) / 2.0;
            s.mlp[k] = sl / s0;
        }
    }
    t.sync();
}

// the rest of _m_step_2D: the clip, the weights, the precisions
template <class T>
PMI_G5M_T void m_step_tail(T &t, int K, const Bounds &b, Shared &s)
{
    double total = 0.0;
    for (int k = 0; k < K; ++k) total += s.w[k];                     // every lane, in order
    t.sync();
    for (int k = t.rank(); k < K; k += t.size()) {
        double lo = b.min_cov, hi = b.max_cov;
        if (!b.lp_abs) { const double m2 = s.mlp[k] * s.mlp[k]; lo = b.min_cov * m2, hi = b.max_cov * m2; }
        double c = s.cov[k];
        if (c < lo) c = lo;
        else if (c > hi) c = hi;
        s.cov[k] = c;
        s.w[k] = s.w[k] / total;
        s.pc[k] = 1.0 / sqrt(c);
    }
    t.sync();
}

// squared distance of _euclidean_distances between the candidate (cx, cy) and the row (x, y)
PMI_G5M_FN double sq_dist(double cx, double cy, double x, double y)
{
    const double XX = (0.0 + cx * cx) + cy * cy, YY = (0.0 + x * x) + y * y;
    double dd = -2.0 * ((0.0 + cx * x) + cy * y);
    dd += XX;
    dd += YY;
    return dd > 0.0 ? dd : 0.0;
}

// _kmeans_plusplus: s.idx[0 .. K) from the first index and the uniforms of one seed; closest is n doubles of work space
template <class T>
PMI_G5M_T void kmeanspp(T &t, const Data &d, int K, int32_t first, const double *u, double *closest, Shared &s)
{
    const int trials = local_trials(K);
    double cx = d.x[first], cy = d.y[first], acc = 0.0;
    for (int i = t.rank(); i < d.n; i += t.size()) { const double dd = sq_dist(cx, cy, d.x[i], d.y[i]); closest[i] = dd; acc += dd; }
    if (t.rank() == 0) s.idx[0] = first;
    double pot = t.sum(acc);
    for (int c = 1; c < K; ++c) {
        if (t.rank() == 0) {
            // np.searchsorted(np.cumsum(closest), rand_vals) from the left, clamped to n - 1
            double val[MAX_TRIALS], run = 0.0;
            bool found[MAX_TRIALS];
            for (int q = 0; q < trials; ++q) { val[q] = u[(c - 1) * trials + q] * pot; s.cand[q] = d.n - 1; found[q] = false; }
            for (int i = 0; i < d.n; ++i) {
                run += closest[i];
                for (int q = 0; q < trials; ++q)
                    if (!found[q] && run >= val[q]) { s.cand[q] = i; found[q] = true; }
            }
        }
        t.sync();
        int best = 0;
        double best_pot = 0.0;
        for (int q = 0; q < trials; ++q) {
            cx = d.x[s.cand[q]], cy = d.y[s.cand[q]];
            acc = 0.0;
            for (int i = t.rank(); i < d.n; i += t.size()) {
                const double dd = sq_dist(cx, cy, d.x[i], d.y[i]);
                acc += dd < closest[i] ? dd : closest[i];
            }
            const double p = t.sum(acc);
            if (q == 0 || p < best_pot) best = q, best_pot = p;
        }
        const int32_t chosen = s.cand[best];
        cx = d.x[chosen], cy = d.y[chosen];
        for (int i = t.rank(); i < d.n; i += t.size()) {
            const double dd = sq_dist(cx, cy, d.x[i], d.y[i]);
            closest[i] = dd < closest[i] ? dd : closest[i];
        }
        pot = best_pot;
        t.sync();                                                     // every lane has read s.cand
        if (t.rank() == 0) s.idx[c] = chosen;
    }
    t.sync();
}

// _initialize_G5M_2D for one seed: the parameters of the one-hot responsibilities of s.idx
template <class T>
PMI_G5M_T void init_params(T &t, const Data &d, int K, double *resp, Shared &s)
{
    for (size_t e = t.rank(); e < (size_t)d.n * K; e += t.size()) resp[e] = 0.0;
    t.sync();
    for (int k = t.rank(); k < K; k += t.size()) resp[(size_t)s.idx[k] * K + k] = 1.0;
    t.sync();
    estimate(t, d, K, resp, s);
    for (int k = t.rank(); k < K; k += t.size()) { s.w[k] = s.w[k] / (double)d.n; s.pc[k] = 1.0 / sqrt(s.cov[k]); }
    t.sync();
}

// find_local_minima(pdf) is not empty, for the line between components a and b (indices into the shared parameters),
// with weights w
PMI_G5M_FN bool pair_resolved(const Shared &s, int a, int b, double wa, double wb)
{
    const double lwa = log_(wa), lwb = log_(wb), lda = 2.0 * log_(s.pc[a]), ldb = 2.0 * log_(s.pc[b]);
    const double pa = s.pc[a] * s.pc[a], pb = s.pc[b] * s.pc[b];
    const double dirx = s.mx[b] - s.mx[a], diry = s.my[b] - s.my[a], step = 1.0 / 39.0;
    double prev2 = 0.0, prev1 = 0.0;
    for (int q = 0; q < LINE; ++q) {
        const double tq = q == LINE - 1 ? 1.0 : (double)q * step;      // np.linspace(0, 1, 40)
        const double x = s.mx[a] + dirx * tq, y = s.my[a] + diry * tq;
        const double la = wlog_prob(x, y, s.mx[a], s.my[a], pa, lda, lwa, false, true);
        const double lb = wlog_prob(x, y, s.mx[b], s.my[b], pb, ldb, lwb, false, true);
        const double pdf = (0.0 + exp_cr(la)) + exp_cr(lb);
        if (q >= 2 && prev1 < prev2 && prev1 < pdf) return true;
        prev2 = prev1, prev1 = pdf;
    }
    return false;
}

// _check_G5M_resolution_2D of the valid components s.idx[0 .. s.n_valid) with the weights w (K of them)
template <class T>
PMI_G5M_T bool resolved(T &t, const double *w, Shared &s)
{
    const int nv = s.n_valid;
    if (nv == 0) return false;
    if (nv == 1) return true;
    if (t.rank() == 0) s.fails = 0;
    t.sync();
    const int pairs = nv * (nv - 1) / 2;
    for (int p = t.rank(); p < pairs; p += t.size()) {
        int i = 0, rest = p;
        while (rest >= nv - 1 - i) { rest -= nv - 1 - i; ++i; }
        const int j = i + 1 + rest, a = s.idx[i], b = s.idx[j];
        if (!pair_resolved(s, a, b, w[a], w[b])) t.count(&s.fails);
    }
    t.sync();
    const bool ok = s.fails == 0;
    t.sync();
    return ok;
}

// n = round(w N) (half to even) and the components with n >= min_locs
template <class T>
PMI_G5M_T void validate(T &t, int K, int n, int min_locs, Shared &s)
{
    for (int k = t.rank(); k < K; k += t.size()) s.nloc[k] = (int32_t)rint(s.w[k] * (double)n);
    t.sync();
    if (t.rank() == 0) {
        int nv = 0;
        for (int k = 0; k < K; ++k)
            if (s.nloc[k] >= min_locs) s.idx[nv++] = k;
        s.n_valid = nv;
    }
    t.sync();
}

// one initialisation's record: what pick_init and judge read.  A Trial of K components is TRIAL_HEAD + 7 K doubles.
constexpr int TRIAL_HEAD = 4;          // lower bound, resolution pass, converged, n_valid
PMI_G5M_FN size_t trial_doubles(int K) { return TRIAL_HEAD + (size_t)7 * K; }

// one initialisation of _fit_G5M: from the parameters in s (weights, means, precisions) through the EM loop to the record
template <class T>
PMI_G5M_T void fit_init(T &t, const Data &d, int K, const Bounds &b, double *resp, Shared &s, double *trial)
{
    double lower = -INFINITY;
    bool converged = false;
    for (int it = 0; it < MAX_ITER; ++it) {
        const double prev = lower;
        lower = e_step(t, d, K, resp, s);
        estimate(t, d, K, resp, s);
        m_step_tail(t, K, b, s);
        const double change = lower - prev;
        if (fabs(change) < TOL) { converged = true; break; }
    }
    validate(t, K, d.n, b.min_locs, s);
    const bool pass = resolved(t, s.w, s);
    if (t.rank() == 0) { trial[0] = lower, trial[1] = pass ? 1.0 : 0.0, trial[2] = converged ? 1.0 : 0.0, trial[3] = (double)s.n_valid; }
    double *p = trial + TRIAL_HEAD;
    for (int k = t.rank(); k < K; k += t.size()) {
        p[k] = s.w[k], p[K + k] = s.mx[k], p[2 * K + k] = s.my[k], p[3 * K + k] = s.cov[k], p[4 * K + k] = s.pc[k];
        p[5 * K + k] = (double)s.nloc[k], p[6 * K + k] = k < s.n_valid ? (double)s.idx[k] : -1.0;
    }
    t.sync();
}

// the initialisation _fit_G5M keeps (-1: none passed the resolution check); trials are n_init records of K components
PMI_G5M_FN int pick_init(const double *trials, int n_init, int K)
{
    double max_lower = -INFINITY;
    int best = -1;
    for (int ii = 0; ii < n_init; ++ii) {
        const double *tr = trials + (size_t)ii * trial_doubles(K);
        if (tr[1] != 0.0 && (tr[0] > max_lower || max_lower == -INFINITY)) max_lower = tr[0], best = ii;
    }
    return best;
}

// a model as the callers keep it, `cap` components apart: weights_ (normalised), means_, covariances_,
// precisions_cholesky_, n_locs and valid_idx (the first n_valid entries)
struct Model { double *w, *mx, *my, *cov, *pc; int32_t *nloc, *valid; };

// score_samples(X).mean() of the valid components of the model in s (weights s.w)
template <class T>
PMI_G5M_T double mean_score(T &t, const Data &d, Shared &s)
{
    const int nv = s.n_valid;
    double acc = 0.0;
    for (int i = t.rank(); i < d.n; i += t.size()) {
        double mxv = -INFINITY;
        for (int j = 0; j < nv; ++j) {
            const int k = s.idx[j];
            const double v = wlog_prob(d.x[i], d.y[i], s.mx[k], s.my[k], s.prec[k], s.logdet[k], s.logw[k], false, true);
            mxv = v > mxv ? v : mxv;
        }
        double es = 0.0;
        for (int j = 0; j < nv; ++j) {
            const int k = s.idx[j];
            es += exp_cr(wlog_prob(d.x[i], d.y[i], s.mx[k], s.my[k], s.prec[k], s.logdet[k], s.logw[k], false, true) - mxv);
        }
        acc += log_(es) + mxv;
    }
    return t.sum(acc) / (double)d.n;
}

// What G5M_2D(K).fit(X) leaves and what _find_optimal_G5M_2D makes of it: the kept initialisation goes to s with
// set_parameters' weights, then the Sparrow check and the BIC.  -> found (fit did not return None); *bic is inf when the
// model is not resolved.
template <class T>
PMI_G5M_T bool judge(T &t, const Data &d, int K, const double *trials, int n_init, Shared &s, double *bic, bool *converged)
{
    const int best = pick_init(trials, n_init, K);
    *bic = INFINITY;
    *converged = false;
    if (best < 0) return false;
    const double *tr = trials + (size_t)best * trial_doubles(K), *p = tr + TRIAL_HEAD;
    double total = 0.0;
    for (int k = 0; k < K; ++k) total += p[k];
    t.sync();
    for (int k = t.rank(); k < K; k += t.size()) {
        s.w[k] = p[k] / total, s.mx[k] = p[K + k], s.my[k] = p[2 * K + k], s.cov[k] = p[3 * K + k], s.pc[k] = p[4 * K + k];
        s.nloc[k] = (int32_t)p[5 * K + k], s.idx[k] = (int32_t)p[6 * K + k];
    }
    if (t.rank() == 0) s.n_valid = (int32_t)tr[3];
    t.sync();
    *converged = tr[2] != 0.0;
    if (resolved(t, s.w, s)) {
        constants(t, K, s);
        const double mean = mean_score(t, d, s);
        const int n_par = 4 * s.n_valid - 1;
        *bic = (double)n_par * log_((double)d.n) - 2.0 * mean * (double)d.n;
    }
    return true;
}

// the model in s -> the caller's arrays
template <class T>
PMI_G5M_T void store(T &t, int K, const Shared &s, const Model &m)
{
    for (int k = t.rank(); k < K; k += t.size()) {
        m.w[k] = s.w[k], m.mx[k] = s.mx[k], m.my[k] = s.my[k], m.cov[k] = s.cov[k], m.pc[k] = s.pc[k];
        m.valid[k] = k < s.n_valid ? s.idx[k] : -1;
        m.nloc[k] = k < s.n_valid ? s.nloc[s.idx[k]] : 0;
    }
}

// ---- _convert_G5M_results, per cluster ---------------------------------------------------------------------------------
constexpr int ASSIGN_STATS = 7;         // per valid component: frame, std_frame, mol_ll, p_val, weighted lp, rsum, weighted log_likelihood
struct Rows { const double *x, *y, *lp, *frame; int n; bool f32, frame_u32; };

// the label of one point: argmax over the valid components of the weighted log probability (the first of equal ones)
PMI_G5M_FN int predict(double x, double y, const Shared &s, bool f32)
{
    int best = 0;
    double bv = 0.0;
    for (int j = 0; j < s.n_valid; ++j) {
        const int k = s.idx[j];
        const double v = wlog_prob(x, y, s.mx[k], s.my[k], s.prec[k], s.logdet[k], s.logw[k], f32, true);
        if (j == 0 || v > bv) best = j, bv = v;
    }
    return best;
}

// The model (K components, s.idx / s.n_valid valid) is in s with its constants.  work: 2 n nv doubles (resp, log_prob).
// Per row: label, log_likelihood; optionally the log probabilities (n x nv) without and with the weights.  Per valid
// component: stats[ASSIGN_STATS], n_events, col_means[c * col_stride].  Per cluster: group_ll.
template <class T>
PMI_G5M_T void assign(T &t, const Rows &d, int K, Shared &s, double *work, const uint64_t *exp_tab, int32_t *label, double *loglik,
                      double *out_lp, double *out_wlp, double *stats, int32_t *n_events, double *group_ll,
                      const double *cols, int n_cols, size_t rows_stride, double *col_means, size_t col_stride)
{
    const int nv = s.n_valid;
    double *resp = work, *lprob = work + (size_t)d.n * nv;
    double acc = 0.0;
    for (int i = t.rank(); i < d.n; i += t.size()) {
        // the e step over all K components (log_prob_norm), then the valid ones
        double mxv = -INFINITY;
        for (int k = 0; k < K; ++k) {
            const double v = wlog_prob(d.x[i], d.y[i], s.mx[k], s.my[k], s.prec[k], s.logdet[k], s.logw[k], d.f32, true);
            mxv = v > mxv ? v : mxv;
        }
        double es = 0.0;
        for (int k = 0; k < K; ++k)
            es += exp_cr(wlog_prob(d.x[i], d.y[i], s.mx[k], s.my[k], s.prec[k], s.logdet[k], s.logw[k], d.f32, true) - mxv);
        const double lpn = log_(es) + mxv;
        double vmx = -INFINITY;
        int best = 0;
        for (int j = 0; j < nv; ++j) {
            const int k = s.idx[j];
            const double v = wlog_prob(d.x[i], d.y[i], s.mx[k], s.my[k], s.prec[k], s.logdet[k], s.logw[k], d.f32, true);
            lprob[(size_t)i * nv + j] = v;
            resp[(size_t)i * nv + j] = exp_cr(v - lpn);
            if (out_wlp) out_wlp[(size_t)i * nv + j] = v;
            if (out_lp) out_lp[(size_t)i * nv + j] = wlog_prob(d.x[i], d.y[i], s.mx[k], s.my[k], s.prec[k], s.logdet[k], s.logw[k], d.f32, false);
            if (v > vmx) best = j, vmx = v;
        }
        double vs = 0.0;
        for (int j = 0; j < nv; ++j) vs += exp_cr(lprob[(size_t)i * nv + j] - vmx);
        const double score = log_(vs) + vmx;
        label[i] = best, loglik[i] = score;
        acc += score;
    }
    const double gll = t.sum(acc) / (double)d.n;
    if (t.rank() == 0) *group_ll = gll;
    for (int j = t.rank(); j < nv; j += t.size()) n_events[j] = 0;
    t.sync();
    for (int j = t.group(); j < nv; j += t.groups()) {
        const int k = s.idx[j];
        double rs = 0.0, ml = 0.0, fr = 0.0, wl = 0.0, sl = 0.0;
        for (int i = t.glane(); i < d.n; i += t.gsize()) {
            const double r = resp[(size_t)i * nv + j];
            rs += r, ml += r * lprob[(size_t)i * nv + j], fr += r * d.frame[i], wl += r * d.lp[i], sl += r * loglik[i];
        }
        rs = t.gsum(rs), ml = t.gsum(ml), fr = t.gsum(fr), wl = t.gsum(wl), sl = t.gsum(sl);
        const double frame = fr / rs, mol = ml / rs;
        double var = 0.0;
        for (int i = t.glane(); i < d.n; i += t.gsize()) { const double df = d.frame[i] - frame; var += resp[(size_t)i * nv + j] * (df * df); }
        var = t.gsum(var);
        for (int c = 0; c < n_cols; ++c) {
            double cs = 0.0;
            for (int i = t.glane(); i < d.n; i += t.gsize()) cs += resp[(size_t)i * nv + j] * cols[(size_t)c * rows_stride + i];
            cs = t.gsum(cs);
            if (t.glane() == 0) col_means[(size_t)c * col_stride + j] = cs / rs;
        }
        if (t.glane() == 0) {
            const double expected = log_(s.w[k] / (TWO_PI * s.cov[k])) - 1.0;
            const double stdev = sqrt(2.0 * 0.5 / ((double)d.n * s.w[k]));
            double *o = stats + (size_t)j * ASSIGN_STATS;
            o[0] = frame;
            o[1] = sqrt(var / ((double)(d.n - 1) * rs / (double)d.n));
            o[2] = mol;
            o[3] = 0.5 * (1.0 + pmi_glibc::erf((mol - expected) / (stdev * SQRT_2), exp_tab));
            o[4] = wl / rs;
            o[5] = rs;
            o[6] = sl / rs;                                          // the log_likelihood column, added before the means are taken
        }
    }
    // binding events: runs of rows whose frames are at most 3 apart; the float32 mean of each, predicted
    for (int i = t.rank(); i < d.n; i += t.size()) {
        auto gap = [&](int a) {
            return d.frame_u32 ? (uint32_t)(int64_t)d.frame[a] - (uint32_t)(int64_t)d.frame[a - 1] > 3u : d.frame[a] - d.frame[a - 1] > 3.0;
        };
        if (i > 0 && !gap(i)) continue;
        int e = i + 1;
        while (e < d.n && !gap(e)) ++e;
        double ex, ey;                                                 // np.mean in the column's own type
        if (d.f32) {
            ex = (double)(segstats::reduce_sum<float>([&](int32_t p) { return (float)d.x[p]; }, i, e) / (float)(e - i));
            ey = (double)(segstats::reduce_sum<float>([&](int32_t p) { return (float)d.y[p]; }, i, e) / (float)(e - i));
        } else {
            ex = segstats::reduce_sum<double>([&](int32_t p) { return d.x[p]; }, i, e) / (double)(e - i);
            ey = segstats::reduce_sum<double>([&](int32_t p) { return d.y[p]; }, i, e) / (double)(e - i);
        }
        t.count(&n_events[predict(ex, ey, s, d.f32)]);
    }
    t.sync();
}

}  // namespace g5m
}  // namespace pmi
