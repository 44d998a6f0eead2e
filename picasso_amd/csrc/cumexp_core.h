// cumexp_core.h — the arithmetic of one cumulative-exponential fit (picasso/lib.py:1263-1327 estimate_kinetic_rate,
// fit_cum_exp), shared by the kernel of csrc/cumexp.hip and the host-side check of it (tests/cumexp_host_driver.cpp).
//
// The model is f(x) = a (1 - exp(-x / t)) + c over the ascending samples x[0 .. n) with y[i] = i + 1; the start is the
// reference's p0 = (n, mean, min) and the bounds are its a in [0, inf), t in [min, max], c in [0, inf).  The minimiser is a
// damped Newton method on the bounded problem, in float64:
//   sums      one pass over the samples gives r = f - y, cost = 0.5 sum r^2, the gradient g = J^T r and the full Hessian
//             H = J^T J + sum r f'' (the model has two second derivatives that are not zero: f_at and f_tt);
//   active    a parameter on a bound whose gradient points out of the box is held for this step;
//   step      (H + lambda diag(J^T J)) d = -g on the free parameters by an LDL^T factorisation; a pivot that is not positive
//             raises lambda (x 10) and factors again; the trial point is p + d clipped to the box;
//   linear    after every accepted step, and first of all, a and c are set to the exact minimiser of the cost at the
//             current t (the model is linear in them; their two bounds are handled by enumeration): the fit walks the
//             ridge of the projected problem and never the plateau a = 0, where t means nothing;
//   judge     a trial whose cost is finite and below the current one (or equal to it while lambda <= 1e-5) is accepted
//             (lambda / 10), any other is refused (lambda x 10): every accepted point is a descent from p0.
// It ends "converged" when an accepted step with lambda <= 1e-5 moved no parameter by more than 1e-10 of its size, when
// the trial point equals the current one, or when lambda has passed 1e10 without an acceptable step (no descent left above
// rounding); "iteration cap" after MAX_ITER passes.  These are its own tolerances, not scipy's.  The caller sums: the
// kernel strides the samples over a wavefront and reduces across lanes, the host adds them in order; everything else here
// runs uniformly, on values every lane holds alike.
//
// exp is exp_cr.h's correctly rounded one, the same function on the device and on the host.  Build with contraction off.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define PMI_CUMEXP_FN __device__ __forceinline__
#else
#define PMI_CUMEXP_FN static inline
#endif
#if defined(__clang__)
#pragma clang fp contract(off)
#endif

#include "exp_cr.h"

namespace pmi {
namespace cumexp {

enum { S_RR, S_GA, S_GT, S_GC, S_AA, S_AT, S_AC, S_TT, S_TC, S_CC, S_RAT, S_RTT, N_SUMS };
enum { CONVERGED = 0, ITER_CAP = 1, BAD_INPUT = 2 };       // pmi_cumexp_fit's status codes
constexpr int MAX_ITER = 300;                              // passes over the samples, the first one included
constexpr int MAX_RAISE = 40;                              // lambda x 10 at most this often inside one step

// what sample (x, y) adds to the twelve sums at the point (a, t, c)
PMI_CUMEXP_FN void add_sample(double *s, double x, double y, double a, double t, double c)
{
    const double u = x / t;
    const double E = exp_cr(-u);
    const double fa = 1.0 - E;
    const double q = E * u / t;                            // E x / t^2:  f_t = -a q,  f_at = -q,  f_tt = a q (2 - u) / t
    const double ft = -(a * q);
    const double r = (a * fa + c) - y;
    s[S_RR] += r * r;
    s[S_GA] += r * fa;
    s[S_GT] += r * ft;
    s[S_GC] += r;
    s[S_AA] += fa * fa;
    s[S_AT] += fa * ft;
    s[S_AC] += fa;
    s[S_TT] += ft * ft;
    s[S_TC] += ft;
    s[S_CC] += 1.0;
    s[S_RAT] += r * -q;
    s[S_RTT] += r * (a * q * (2.0 - u) / t);
}

struct Fit {
    double p[3], lo[3], hi[3];       // a, t, c and their box
    double cost, g[3];
    double H[6];                     // aa, at, ac, tt, tc, cc
    double D[3];                     // diag(J^T J)
    double trial[3];
    double lambda;
    int iters, status, done;
    int linear, was_linear;          // the next step is the linear one; the trial point came from it
};

PMI_CUMEXP_FN void start(Fit &f, double n, double mean, double mn, double mx)
{
    const double inf = __builtin_inf();
    f.p[0] = n, f.p[1] = mean, f.p[2] = mn;
    f.lo[0] = 0.0, f.lo[1] = mn, f.lo[2] = 0.0;
    f.hi[0] = inf, f.hi[1] = mx, f.hi[2] = inf;
    for (int i = 0; i < 3; ++i) f.trial[i] = f.p[i];
    f.lambda = 1e-3;
    f.iters = 0, f.status = ITER_CAP, f.done = 0;
    f.linear = 1, f.was_linear = 0;
    f.cost = inf;
}

// the sums at f.trial become the current point
PMI_CUMEXP_FN void take(Fit &f, const double *s)
{
    for (int i = 0; i < 3; ++i) f.p[i] = f.trial[i];
    f.cost = 0.5 * s[S_RR];
    f.g[0] = s[S_GA], f.g[1] = s[S_GT], f.g[2] = s[S_GC];
    f.H[0] = s[S_AA], f.H[1] = s[S_AT] + s[S_RAT], f.H[2] = s[S_AC];
    f.H[3] = s[S_TT] + s[S_RTT], f.H[4] = s[S_TC], f.H[5] = s[S_CC];
    f.D[0] = s[S_AA], f.D[1] = s[S_TT], f.D[2] = s[S_CC];
}

// The linear step: with t held the model is linear in (a, c), so the Newton step of those two is the exact minimiser of
// the cost over them; with a >= 0 and c >= 0 it is the best of the free solution and the solutions on one or both
// bounds, by the value of the quadratic q(d) = g.d + d.M d / 2 (M = the a, c block of J^T J).  Returns 0 when it moves
// nothing.
PMI_CUMEXP_FN int propose_linear(Fit &f)
{
    const double aa = f.H[0], ac = f.H[2], cc = f.H[5], ga = f.g[0], gc = f.g[2];
    const double a = f.p[0], c = f.p[2];
    if (!(aa > 0.0) || !(cc > 0.0)) return 0;
    const double inf = __builtin_inf();
    double best = inf, best_a = a, best_c = c;
    const double det = aa * cc - ac * ac;
    for (int k = 0; k < 4; ++k) {
        // 0: both free; 1: c' = 0; 2: a' = 0; 3: both on their bounds
        double da, dc;
        if (k == 0) {
            if (!(det > 1e-14 * aa * cc)) continue;
            da = (-ga * cc + gc * ac) / det, dc = (-gc * aa + ga * ac) / det;
        } else if (k == 1) {
            dc = -c, da = (-ga - ac * dc) / aa;
        } else if (k == 2) {
            da = -a, dc = (-gc - ac * da) / cc;
        } else {
            da = -a, dc = -c;
        }
        const double na = k >= 2 ? 0.0 : a + da, nc = (k == 1 || k == 3) ? 0.0 : c + dc;
        if (!(na >= 0.0) || !(nc >= 0.0)) continue;      // also refuses NaN
        const double q = ga * da + gc * dc + 0.5 * (aa * da * da + 2.0 * ac * da * dc + cc * dc * dc);
        if (q < best) best = q, best_a = na, best_c = nc;
    }
    if (best_a == a && best_c == c) return 0;
    f.trial[0] = best_a, f.trial[1] = f.p[1], f.trial[2] = best_c;
    return 1;
}

// the next trial point; returns 0 when the fit has ended instead
PMI_CUMEXP_FN int propose(Fit &f)
{
    if (f.linear) {
        f.linear = 0;
        if (propose_linear(f)) { f.was_linear = 1; return 1; }
    }
    f.was_linear = 0;
    int held[3];
    for (int i = 0; i < 3; ++i)
        held[i] = (f.p[i] <= f.lo[i] && f.g[i] > 0.0) || (f.p[i] >= f.hi[i] && f.g[i] < 0.0);
    if (held[0] && held[1] && held[2]) { f.status = CONVERGED, f.done = 1; return 0; }
    for (int raise = 0; raise < MAX_RAISE; ++raise) {
        // M = H + lambda D on the free parameters, the identity on the held ones
        double m[6], b[3];
        const double tiny = 1e-300;
        m[0] = held[0] ? 1.0 : f.H[0] + f.lambda * (f.D[0] > tiny ? f.D[0] : tiny);
        m[3] = held[1] ? 1.0 : f.H[3] + f.lambda * (f.D[1] > tiny ? f.D[1] : tiny);
        m[5] = held[2] ? 1.0 : f.H[5] + f.lambda * (f.D[2] > tiny ? f.D[2] : tiny);
        m[1] = (held[0] || held[1]) ? 0.0 : f.H[1];
        m[2] = (held[0] || held[2]) ? 0.0 : f.H[2];
        m[4] = (held[1] || held[2]) ? 0.0 : f.H[4];
        for (int i = 0; i < 3; ++i) b[i] = held[i] ? 0.0 : -f.g[i];
        // LDL^T: d0, l10, l20, d1, l21, d2
        const double d0 = m[0];
        const double l10 = m[1] / d0, l20 = m[2] / d0;
        const double d1 = m[3] - l10 * m[1];
        const double l21 = (m[4] - l20 * m[1]) / d1;
        const double d2 = m[5] - l20 * m[2] - l21 * (m[4] - l20 * m[1]);
        if (d0 > 0.0 && d1 > 0.0 && d2 > 0.0) {
            const double z0 = b[0];
            const double z1 = b[1] - l10 * z0;
            const double z2 = b[2] - l20 * z0 - l21 * z1;
            const double w2 = z2 / d2;
            const double w1 = z1 / d1 - l21 * w2;
            const double w0 = z0 / d0 - l10 * w1 - l20 * w2;
            const double d[3] = {w0, w1, w2};
            int moved = 0, finite = 1;
            for (int i = 0; i < 3; ++i) {
                double v = f.p[i] + d[i];
                finite &= (v == v) ? 1 : 0;
                v = v < f.lo[i] ? f.lo[i] : (v > f.hi[i] ? f.hi[i] : v);
                f.trial[i] = v;
                moved |= (v != f.p[i]) ? 1 : 0;
            }
            if (finite) {
                if (!moved) { f.status = CONVERGED, f.done = 1; return 0; }
                return 1;
            }
        }
        f.lambda *= 10.0;
        if (f.lambda > 1e10) break;
    }
    f.status = CONVERGED, f.done = 1;      // no factorisation gives a step: nothing is left to descend
    return 0;
}

// the sums at f.trial decide the step
PMI_CUMEXP_FN void judge(Fit &f, const double *s)
{
    const double cost = 0.5 * s[S_RR];
    if (f.was_linear) {                    // a linear step changes neither lambda nor the state of the fit
        if (cost <= f.cost) take(f, s);
        return;
    }
    // false for a NaN cost; an equal cost counts as a step only while lambda is small, so that rounding cannot keep it from rising
    if (cost < f.cost || (cost == f.cost && f.lambda <= 1e-5)) {
        double rel = 0.0;
        for (int i = 0; i < 3; ++i) {
            const double size = __builtin_fabs(f.trial[i]) > 1e-300 ? __builtin_fabs(f.trial[i]) : 1e-300;
            const double r = __builtin_fabs(f.trial[i] - f.p[i]) / size;
            rel = r > rel ? r : rel;
        }
        const double used = f.lambda;
        take(f, s);
        f.linear = 1;
        f.lambda = used > 1e-14 ? used / 10.0 : used;
        if (rel <= 1e-10 && used <= 1e-5) f.status = CONVERGED, f.done = 1;
    } else {
        f.lambda *= 10.0;
        if (f.lambda > 1e10) f.status = CONVERGED, f.done = 1;
    }
}

}  // namespace cumexp
}  // namespace pmi
