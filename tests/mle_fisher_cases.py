"""Shared by tests/test_mle_fisher_host.py (CPU) and tests/test_gpu_mle_fisher.py (GPU): the spot generators, the
units u and v, the yardstick (what the oracle's float32-rounded arithmetic achieves against tests/mle_fisher_ref.py) and
the device tolerance built on it.  DESIGN.md section 2 ("CRLB and log-likelihood against float64") has the numbers.
"""
import functools
from math import erf, sqrt

import numpy as np

import mle_fisher_ref as ref

MARGIN = 32          # CRLB: device error allowed, in multiples of the oracle's measured worst (K_ref)
MARGIN_LL = 8        # log-likelihood likewise (L_ref)
EPS, MAX_IT = 1e-3, 100
YARDSTICK_SETS = [(box, method) for box in (3, 7, 13, 17) for method in ("sigmaxy", "sigma")]
YARDSTICK_N = 1500


def _poisson_spots(rng, box, x0, y0, sx, sy, photons, bg):
    idx = np.arange(box)
    spots = np.empty((len(x0), box, box), np.float32)
    for i in range(len(x0)):
        ex = np.array([0.5 * (erf((k - x0[i] + .5) / (sqrt(2) * sx[i])) - erf((k - x0[i] - .5) / (sqrt(2) * sx[i]))) for k in idx])
        ey = np.array([0.5 * (erf((k - y0[i] + .5) / (sqrt(2) * sy[i])) - erf((k - y0[i] - .5) / (sqrt(2) * sy[i]))) for k in idx])
        spots[i] = rng.poisson(photons[i] * np.outer(ey, ex) + bg[i])
    return spots


def adversarial_spots(box, n, seed, sigma_lo=0.6):
    """20...9000 photons on backgrounds 0.5...30, centres up to 1.5 px off, sigma 0.6 px...0.25 box + 0.3 (the
    family of tests/test_gpu_parity.py): many of these fits run into max_it, leave the box or collapse to a floor."""
    rng = np.random.default_rng(seed)
    c = box // 2
    u = lambda lo, hi: rng.uniform(lo, hi, n)      # noqa: E731
    return _poisson_spots(rng, box, c + u(-1.5, 1.5), c + u(-1.5, 1.5), u(sigma_lo, 0.25 * box + 0.3), u(sigma_lo, 0.25 * box + 0.3),
                          u(20, 9000), u(0.5, 30))


def offcorner_spots(box, n, seed):
    """The x-y coupling M[0,1] vanishes on a centred spot; it is large where the spot sits off towards a corner of the box,
    is elliptical and stands on little background: centres 1...1.5 px off in BOTH axes (all four corners), sx != sy,
    background below 2."""
    rng = np.random.default_rng(seed)
    c = box // 2
    u = lambda lo, hi: rng.uniform(lo, hi, n)      # noqa: E731
    sgn = lambda: rng.choice([-1.0, 1.0], n)      # noqa: E731
    sx = u(1.1, max(1.6, 0.16 * box))
    ratio = u(0.7, 0.85)
    sy = sx * np.where(rng.random(n) < 0.5, ratio, 1.0 / ratio)
    return _poisson_spots(rng, box, c + sgn() * u(1.0, 1.5), c + sgn() * u(1.0, 1.5), sx, sy, u(1000, 9000), u(1.0, 2.0))


def mixed_spots(box, n_adversarial, n_offcorner, seed, sigma_lo=0.6):
    return np.concatenate([adversarial_spots(box, n_adversarial, seed, sigma_lo), offcorner_spots(box, n_offcorner, seed + 1)])


def yardstick_spots(box):
    """1200 adversarial spots and 300 off-corner ones.  The sigma range starts at 0.75 px here, not 0.6: with 0.6 the
    REFERENCE's Newton loop leaves 11 % of the 7 x 7 "sigmaxy" set outside the well-conditioned class (diverged fits),
    above the 10 % cap; with 0.75 it is 5 %."""
    return mixed_spots(box, YARDSTICK_N - 300, 300, 77 + box, sigma_lo=0.75)


def crlb_unit(lmin, NP):
    """u = NP 2^-24 / lambda_min(C): a float32 rounding of every Fisher entry, amplified by the conditioning."""
    return NP * 2.0 ** -24 / lmin


def crlb_errors(crlb, theta, box, method):
    """-> err (N, NP) relative to crlb64 at theta, u (N,), well (N,), lmin, lmax."""
    NP = ref.n_params(method)
    M = ref.fisher64(theta, box, method)
    c64, well = ref.crlb64(M)
    lmin, lmax = ref.conditioning(M)
    with np.errstate(all="ignore"):
        err = np.abs(np.asarray(crlb, np.float64)[:, :NP] - c64) / c64
    return err, crlb_unit(lmin, NP), well, lmin, lmax


def loglik_errors(ll, spots, theta, method):
    """-> |ll - ll64| (N,), v (N,)."""
    ll64 = ref.loglik64(spots, theta, method)
    return np.abs(np.asarray(ll, np.float64) - ll64), ref.loglik_unit(spots, ll64)


def measure(crlb, ll, spots, theta, method):
    """K = max err / u over the well-conditioned rows and L = max |dll| / v over the same rows, with the share of rows
    outside the well-conditioned class."""
    box = spots.shape[1]
    err, u, well, _, _ = crlb_errors(crlb, theta, box, method)
    dll, v = loglik_errors(ll, spots, theta, method)
    K = float((err[well] / u[well, None]).max()) if well.any() else 0.0
    L = float((dll[well] / v[well]).max()) if well.any() else 0.0
    return K, L, float(1.0 - well.mean())


@functools.lru_cache(maxsize=None)
def yardstick():
    """The oracle against float64 on the eight yardstick sets -> {(box, method): (K_ref, L_ref, share outside)}.
    Computed from the oracle every time it is needed (once per process), never recorded from a device run."""
    from oracle import oracle as orc
    out = {}
    for box, method in YARDSTICK_SETS:
        spots = yardstick_spots(box)
        th, cr, ll, _ = orc.gaussmle(spots, EPS, MAX_IT, method, threads=min(8, orc.max_threads()))
        out[(box, method)] = measure(cr, ll, spots, th, method)
    return out


def k_ref():
    return max(k for k, _, _ in yardstick().values())


def l_ref():
    return max(l for _, l, _ in yardstick().values())


def crlb_tolerance(u, extra_ulps=0):
    """Per-row relative bound on every CRLB entry of a well-conditioned row: MARGIN K_ref u + 2^-23 (the float32 store)."""
    return MARGIN * k_ref() * u + (1 + extra_ulps) * 2.0 ** -23


def loglik_tolerance(v):
    return MARGIN_LL * l_ref() * v


def pinv_rows_check(crlb, theta, box, method):
    """The rows OUTSIDE the well-conditioned class against the reference's pinv semantics at the same theta
    (mle_fisher_ref.pinv_diag_jacobi): |d| <= 4e-3 |ref| + 1e-5 max_row |ref| (the bound tests/test_oracle_golden.py uses
    for this third-party arithmetic), equal NaN patterns, no inf, and 0 exactly where the reference drops a direction.
    Rows where either branch is legitimate (mle_fisher_ref.pinv_ambiguous) are skipped.
    -> outside (N,) bool, skipped (N,) bool, list of (row, what) failures."""
    NP = ref.n_params(method)
    M = ref.fisher64(theta, box, method)
    outside = ~ref.well_conditioned(M)
    skipped = np.zeros(len(M), bool)
    failures = []
    for i in np.flatnonzero(outside):
        if ref.pinv_ambiguous(M[i]):
            skipped[i] = True
            continue
        want = ref.pinv_diag_jacobi(M[i])
        got = np.asarray(crlb[i, :NP], np.float64)
        if not np.array_equal(np.isnan(got), np.isnan(want)):
            failures.append((int(i), "nan pattern", got, want))
            continue
        if np.isnan(want).all():
            continue
        with np.errstate(invalid="ignore"):
            tol = 4e-3 * np.abs(want) + 1e-5 * np.nanmax(np.abs(want))
            if np.isinf(got).any() or np.any(np.abs(got - want) > tol) or np.any(got[want == 0.0] != 0.0):
                failures.append((int(i), "value", got, want))
    return outside, skipped, failures


def pinv_case_spots():
    """Case f, 7 x 7: all-zero and constant spots, single hot pixels, a spot on the box edge whose width hits the cap, a
    spot wider than the box, photon counts collapsing to the floor, a NaN pixel, the degenerate7 golden spots — with
    ordinary spots between them."""
    import os
    rng = np.random.default_rng(11)
    one = lambda *a: _poisson_spots(rng, 7, *[np.array([float(v)]) for v in a])[0]      # noqa: E731
    z = np.zeros((7, 7), np.float32)
    hot = z.copy(); hot[3, 3] = 5000.0
    hot_bg = np.full((7, 7), 3.0, np.float32); hot_bg[2, 4] = 800.0
    hot_corner = np.full((7, 7), 1.0, np.float32); hot_corner[0, 6] = 300.0
    nan = adversarial_spots(7, 1, 3)[0].copy(); nan[1, 5] = np.nan
    rows = [z, np.full((7, 7), 10.0, np.float32), np.full((7, 7), 1000.0, np.float32), hot, hot_bg, hot_corner,
            one(-0.4, 3.0, 3.5, 1.0, 20000, 2), one(3.0, 6.6, 1.0, 4.0, 20000, 2), one(3.0, 3.0, 9.0, 9.0, 50000, 1),
            rng.poisson(0.05, (7, 7)).astype(np.float32),
            rng.poisson(12.0, (7, 7)).astype(np.float32), nan]
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gaussmle_degenerate7.npz"))
    return np.concatenate([np.stack(rows), g["spots"].astype(np.float32), adversarial_spots(7, 40, 4, sigma_lo=0.9)])
