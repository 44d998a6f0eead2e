"""Test-side reference of the astigmatic z fit (picasso_amd/csrc/zfit.hip, oracle/picasso_oracle.c:fminbound): the
target function of picasso/zfit.py:254-291 restated in NumPy float64, minimised by scipy itself, and the table math of
picasso/zfit.py:_fit_z (:364-382), filter_z_fits (:698-703) and lib.ensure_sanity restated in NumPy.  Also the hostile
input sets that tests/test_zfit_host.py (oracle against scipy) and tests/test_gpu_zfit.py (kernel against scipy) share.

Operand order of the reference's target (_fit_z_target): z2 = z*z, z3 = z*z2, z4 = z*z3, z5 = z*z4, z6 = z*z5;
wx = cx[0]*z6 + cx[1]*z5 + cx[2]*z4 + cx[3]*z3 + cx[4]*z2 + cx[5]*z + cx[6], summed left to right (Python's `+` is
left-associative and numba neither reassociates nor contracts without fastmath), wy alike; the result is
(sx**0.5 - wx**0.5)**2 + (sy**0.5 - wy**0.5)**2 with sx, sy float32 scalars that `** 0.5` widens to float64.  The
kernel and the oracle use the same order.  `x ** 0.5` is pow(x, 0.5): the square root, NaN for a negative x, except
that pow(-inf, 0.5) is +inf (see _root).  pow is not correctly rounded in every libm, sqrt is, and the kernel and the
oracle take sqrt, so this restatement takes np.sqrt too.

The minimiser call is the reference's (picasso/zfit.py:359-363): minimize_scalar(target, bounds=[-1000, 1000],
args=...) with no method and no options, which scipy routes to the "bounded" method with xatol 1e-5, maxiter 500.
"""
import contextlib
import io
import math
import os
import warnings

import numpy as np
from scipy.optimize import minimize_scalar

BOUNDS = [-1000, 1000]
GOLDEN_MEAN = 0.5 * (3.0 - math.sqrt(5.0))
FIRST_POINT = -1000 + GOLDEN_MEAN * 2000          # -236.07: where every fit evaluates the target first
ON_BOUND = 1e-4                                   # a fit "ends on a bound" when 1000 - |z| is below this (10 xatol)
MAXFUN = 500
_HERE = os.path.dirname(os.path.abspath(__file__))


# ---- the target --------------------------------------------------------------------------------------------------
def _f64s(c):
    c = np.asarray(c, np.float64)
    assert c.shape == (7,)
    return tuple(np.float64(v) for v in c)


def _width(z, c):
    z2 = z * z
    z3 = z * z2
    z4 = z * z3
    z5 = z * z4
    z6 = z * z5
    return c[0] * z6 + c[1] * z5 + c[2] * z4 + c[3] * z3 + c[4] * z2 + c[5] * z + c[6]


_INF = np.float64(np.inf)


def _root(v):
    """v ** 0.5 as IEEE 754 pow defines it, with the correctly rounded root: sqrt(v), NaN for a negative or NaN v, but
    +inf for v = -inf (pow(-inf, y) is +inf for every y > 0 that is no odd integer; numba's LLVM turns pow(v, 0.5) into
    exactly this select).  pow(-0.0, 0.5) is +0.0 where sqrt gives -0.0; the target squares the difference, so the
    sign of a zero never reaches its value."""
    return _INF if v == -_INF else np.sqrt(v)


def _target(z, sx, sy, cx, cy):
    """z, sx, sy np.float64, cx, cy tuples of np.float64; the caller holds np.errstate(all="ignore")."""
    ax = _root(sx) - _root(_width(z, cx))
    ay = _root(sy) - _root(_width(z, cy))
    return ax * ax + ay * ay


def widths(z, cx, cy):
    """(wx(z), wy(z)) as np.float64, in the target's operand order."""
    with np.errstate(all="ignore"):
        z = np.float64(z)
        return _width(z, _f64s(cx)), _width(z, _f64s(cy))


def target(z, sx, sy, cx, cy):
    """picasso/zfit.py:254-291 in float64; sx, sy are widened (from float32) first; NaN, never an exception, for the
    square root of a negative (finite) or NaN width."""
    with np.errstate(all="ignore"):
        return _target(np.float64(z), np.float64(sx), np.float64(sy), _f64s(cx), _f64s(cy))


# ---- scipy ---------------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def _quiet():
    with warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore")
        yield


def fit(sx, sy, cx, cy, full=False):
    """(z, sq) float64 arrays: scipy's result.x and result.fun row by row; with `full` also nfev (int64)."""
    sx, sy = np.asarray(sx, np.float32), np.asarray(sy, np.float32)
    cx, cy = _f64s(cx), _f64s(cy)
    n = len(sx)
    z, sq, nfev = np.zeros(n), np.zeros(n), np.zeros(n, np.int64)
    with _quiet():
        for i in range(n):
            r = minimize_scalar(_target, bounds=BOUNDS, args=(np.float64(sx[i]), np.float64(sy[i]), cx, cy))
            z[i], sq[i], nfev[i] = r.x, r.fun, r.nfev
    return (z, sq, nfev) if full else (z, sq)


def evaluated(sx, sy, cx, cy):
    """The z values at which scipy called the target for one row, in order."""
    seen = []
    cx, cy = _f64s(cx), _f64s(cy)

    def recorder(z, *args):
        seen.append(float(z))
        return _target(z, *args)
    with _quiet():
        minimize_scalar(recorder, bounds=BOUNDS, args=(np.float64(np.float32(sx)), np.float64(np.float32(sy)), cx, cy))
    return seen


def last_step(sx, sy, cx, cy):
    """'parabolic' or 'golden': what scipy's own trace (disp=3) calls the step of the last iteration of one row, or
    'initial' when the loop never ran."""
    out = io.StringIO()
    with _quiet(), contextlib.redirect_stdout(out):
        minimize_scalar(_target, bounds=BOUNDS, options={"disp": 3},
                        args=(np.float64(np.float32(sx)), np.float64(np.float32(sy)), _f64s(cx), _f64s(cy)))
    steps = [w for line in out.getvalue().splitlines() for w in line.split()[-1:] if w in ("initial", "parabolic", "golden")]
    return steps[-1]


def pow_sqrt_witness(sx, sy, cx, cy):
    """True when, at some z scipy evaluated for this row, pow(v, 0.5) != sqrt(v) in this machine's libm for one of
    v = sx, sy, wx(z), wy(z) (v >= 0 and finite): the only reason an implementation that takes pow may leave
    scipy's path."""
    def differs(v):
        v = float(v)
        return v >= 0 and math.isfinite(v) and math.pow(v, 0.5) != math.sqrt(v)
    if differs(np.float32(sx)) or differs(np.float32(sy)):
        return True
    return any(differs(w) for z in evaluated(sx, sy, cx, cy) for w in widths(z, cx, cy))


def bits_equal(a, b):
    """Row mask: the same float64 bit pattern, any NaN equal to any NaN."""
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return (np.isnan(a) & np.isnan(b)) | (a.view(np.uint64) == b.view(np.uint64))


# ---- the table math of _fit_z --------------------------------------------------------------------------------------
def _get_calib_size(c, z):
    return c[0] * z**6 + c[1] * z**5 + c[2] * z**4 + c[3] * z**3 + c[4] * z**2 + c[5] * z + c[6]


def _get_prime_calib_size(c, z):
    return 6 * c[0] * z**5 + 5 * c[1] * z**4 + 4 * c[2] * z**3 + 3 * c[3] * z**2 + 2 * c[4] * z + c[5]


def _lq_sigma_uncertainty(sigma, sigma_orth, photons, bg):
    """picasso/gausslq.py:621-633."""
    sa2 = sigma**2 + 1 / 12
    sa4 = sa2**2
    sa = sa2**0.5
    sa2_orth = sigma_orth**2 + 1 / 12
    sa_orth = sa2_orth**0.5
    var_sa2 = sa4 / photons * (512 / 81 + (64 * np.pi * sa * sa_orth * bg) / (3 * photons))
    return np.sqrt(var_sa2 / (4 * sigma**2))


def table(locs, info, cx, cy, magnification, pixelsize, fitting_method, filter, z, sq):
    """What _fit_z makes of the minimiser's (z, sq): the DataFrame with z, d_zcalib and lpz after lib.ensure_sanity and
    filter_z_fits.  z and sq are stored into arrays of the dtype of locs["x"] (np.zeros_like), scaled and rooted
    there.  fitting_method "gaussmle" needs the sx_unc / sy_unc columns (picasso/zfit.py:866-868)."""
    cx, cy = np.asarray(cx, np.float64), np.asarray(cy, np.float64)
    locs = locs.copy()
    with _quiet():
        zc = np.zeros_like(locs["x"])
        sc = np.zeros_like(zc)
        zc[:] = z
        sc[:] = sq
        locs["z"] = zc * magnification
        locs["d_zcalib"] = np.sqrt(sc)
        if fitting_method == "gausslq":
            se_sx = _lq_sigma_uncertainty(locs["sx"], locs["sy"], locs["photons"], locs["bg"]) * pixelsize
            se_sy = _lq_sigma_uncertainty(locs["sy"], locs["sx"], locs["photons"], locs["bg"]) * pixelsize
        else:
            se_sx, se_sy = locs["sx_unc"] * pixelsize, locs["sy_unc"] * pixelsize
        zz = locs["z"] / magnification
        swx = np.sqrt(_get_calib_size(cx, zz) * pixelsize)
        swy = np.sqrt(_get_calib_size(cy, zz) * pixelsize)
        swxc2 = (_get_prime_calib_size(cx, zz) * pixelsize / (2 * swx)) ** 2
        swyc2 = (_get_prime_calib_size(cy, zz) * pixelsize / (2 * swy)) ** 2
        swx2 = ((1 / (2 * np.sqrt(locs["sx"] * pixelsize))) * se_sx) ** 2
        swy2 = ((1 / (2 * np.sqrt(locs["sy"] * pixelsize))) * se_sy) ** 2
        locs["lpz"] = np.sqrt((swxc2 * swx2 + swyc2 * swy2) / (swxc2 + swyc2) ** 2) * magnification
        # lib.ensure_sanity: no inf, no NaN, inside the image, non-negative columns
        locs = locs.replace([np.inf, -np.inf], np.nan).dropna(axis=0, how="any")
        locs = locs[locs["x"] < info[0]["Width"]]
        locs = locs[locs["y"] < info[0]["Height"]]
        for attr in ("x", "y", "lpx", "lpy", "lpz", "photons", "ellipticity", "sx", "sy"):
            if attr in locs.columns:
                locs = locs[locs[attr] >= 0]
        if filter > 0:
            rmsd = np.sqrt(np.nanmean(locs["d_zcalib"] ** 2))
            locs = locs[locs["d_zcalib"] <= filter * rmsd]
    return locs


# ---- input sets ----------------------------------------------------------------------------------------------------
def calibration():
    g = np.load(os.path.join(_HERE, "zfit_calib3d.npz"))
    return np.array(g["cx"], np.float64), np.array(g["cy"], np.float64)


def _poly(**k):
    """7 coefficients, highest power first: _poly(c4=..., c6=...) is c4 z^2 + c6."""
    c = np.zeros(7)
    for name, v in k.items():
        c[int(name[1:])] = v
    return c


def _case(label, sx, sy, cx, cy):
    return (label, np.ascontiguousarray(sx, np.float32), np.ascontiguousarray(sy, np.float32),
            np.ascontiguousarray(cx, np.float64), np.ascontiguousarray(cy, np.float64))


def _uniform(rng, n, lo=0.6, hi=3.2):
    return rng.uniform(lo, hi, n).astype(np.float32), rng.uniform(lo, hi, n).astype(np.float32)


def _on_curve(cx, cy, z0):
    with np.errstate(all="ignore"):
        w = [widths(z, cx, cy) for z in z0]
        return np.array([a for a, _ in w]).astype(np.float32), np.array([b for _, b in w]).astype(np.float32)


def ordinary(n=1500):
    """The committed calibration, sx, sy ~ U(0.6, 3.2): every width positive, every fit in the open interval or on a
    bound."""
    cx, cy = calibration()
    return [_case("ordinary", *_uniform(np.random.default_rng(20250101), n), cx, cy)]


SPECIAL_WIDTHS = np.array([0.0, 1e-45, 1e-30, 0.25, 1.0, 4.0, 1e4, 3e38, np.inf, np.nan, -0.0, -1.0, -np.inf], np.float32)


def widths_set():
    """The committed calibration; every pair of SPECIAL_WIDTHS, and pairs (wx(z0), wy(z0)) that put a zero (to float32
    rounding of the widths) of the target at a known z0, the bounds and their neighbourhood included."""
    cx, cy = calibration()
    a, b = np.meshgrid(SPECIAL_WIDTHS, SPECIAL_WIDTHS, indexing="ij")
    z0 = np.concatenate([np.linspace(-1000, 1000, 81), [-1000 + 1e-5, 1000 - 1e-5, -999.99, 999.99, FIRST_POINT, 1e-7, -1e-7]])
    px, py = _on_curve(cx, cy, z0)
    return [_case("widths", np.concatenate([a.ravel(), px]), np.concatenate([b.ravel(), py]), cx, cy)]


def negative_width(n=250, n_nan=40):
    """Parabolic widths that go negative on part of [-1000, 1000], so the target is NaN on an interval: for x only beyond
    |z| = 300 (the first point is valid), for both beyond |z| = 200 (the first point is NaN), and for x inside |z| < 300
    (the first point is NaN, the outer parts are valid).  Where the first point is NaN every comparison with fx is false
    and every row takes the same path whatever its widths, so those two variants have few rows."""
    _, cy = calibration()
    rng = np.random.default_rng(20250102)
    outer300 = _poly(c4=-2.0 / 300.0**2, c6=2.0)
    outer200 = _poly(c4=-1.5 / 200.0**2, c6=1.5)
    inner300 = _poly(c4=2.0 / 300.0**2, c6=-2.0)
    return [_case("x_negative_beyond_300", *_uniform(rng, n, 0.05, 3.2), outer300, cy),
            _case("both_negative_beyond_200", *_uniform(rng, n_nan, 0.05, 3.2), outer200, outer200 * 0.75),
            _case("x_negative_inside_300", *_uniform(rng, n_nan, 0.05, 3.2), inner300, cy)]


def flat_and_twin(n=200):
    """A constant calibration (every comparison of two target values is a tie), an even one with sx = sy (two equal
    minima at +-z), and a linear one with the widths taken on the curve at z0 = +-(1000 + d), |d| from 1e-6 to 100 on
    either side of the bounds, so the minimum sits on, just inside or outside a bound."""
    rng = np.random.default_rng(20250103)
    flat = _case("flat", *_uniform(rng, n), _poly(c6=1.5), _poly(c6=1.25))
    s = rng.uniform(1.0, 6.0, n).astype(np.float32)
    even = _poly(c4=4e-6, c6=1.0)
    twin = _case("twin", s, s, even, even)
    lx, ly = _poly(c5=1e-3, c6=2.0), _poly(c5=-1e-3, c6=2.0)
    d = np.concatenate([[0.0], 10.0 ** rng.uniform(-6, 2, n // 2 - 1)]) * rng.choice([-1.0, 1.0], n // 2)
    z0 = np.concatenate([1000 + d, -1000 - d])
    return [flat, twin, _case("bound", *_on_curve(lx, ly, z0), lx, ly)]


def steep(n=60):
    """z^6 widths that reach 1e300 and beyond at the bounds: the target is huge or inf at the first points, inf - inf
    and inf / inf appear in the parabola.  Then coefficients that are themselves inf or NaN."""
    rng = np.random.default_rng(20250104)
    out = []
    for k, c0 in enumerate((1e282, 1e290, 1e293, 1e294, 1e296, 1e300)):
        cx, cy = _poly(c0=c0, c6=1.0), _poly(c0=c0 / (1 + k), c4=1e-6, c6=1.5)
        out.append(_case(f"c0_{c0:g}", *_uniform(rng, n), cx, cy))
    cx, cy = calibration()
    for label, idx, v in (("c2_inf", 2, np.inf), ("c3_inf", 3, np.inf), ("c5_minus_inf", 5, -np.inf), ("c6_nan", 6, np.nan),
                          ("c0_nan", 0, np.nan)):
        bad = cx.copy()
        bad[idx] = v
        out.append(_case(label, *_uniform(rng, n // 2), bad, cy))
    return out


SETS = {"ordinary": ordinary, "widths": widths_set, "negative_width": negative_width, "flat_and_twin": flat_and_twin,
        "steep": steep}

# what each set is for: the least number of rows of each class that scipy's own results must show
# (tests/test_zfit_host.py::test_sets_hold_what_they_are_for).  A reading of "per set": a class a set cannot produce is
# absent from it (positive widths never give NaN, a target that is NaN outside |z| < 300 never ends on a bound), and
# test_every_class_is_held_by_some_set sees that no class is left out altogether
HOLDS = {"ordinary": dict(parabolic=5, golden=5),
         "widths": dict(lower=5, upper=5, nan=5, parabolic=5, golden=5),
         "negative_width": dict(nan=5, parabolic=5, golden=5),
         "flat_and_twin": dict(lower=5, upper=5, parabolic=5, golden=5),
         "steep": dict(upper=5, nan=5, parabolic=5, golden=5)}


def census(name):
    """Per set, from scipy alone: rows, rows ending on the lower / upper bound, rows with NaN sq, the largest nfev, rows
    at the evaluation cap, rows whose last step was parabolic / golden."""
    c = dict(rows=0, lower=0, upper=0, nan=0, max_nfev=0, capped=0, parabolic=0, golden=0)
    for _, sx, sy, cx, cy in SETS[name]():
        z, sq, nfev = fit(sx, sy, cx, cy, full=True)
        c["rows"] += len(z)
        c["lower"] += int(np.sum(z + 1000 < ON_BOUND))
        c["upper"] += int(np.sum(1000 - z < ON_BOUND))
        c["nan"] += int(np.isnan(sq).sum())
        c["max_nfev"] = max(c["max_nfev"], int(nfev.max()))
        c["capped"] += int(np.sum(nfev >= MAXFUN))
        for i in range(len(z)):
            step = last_step(sx[i], sy[i], cx, cy)
            if step in ("parabolic", "golden"):
                c[step] += 1
    return c
