"""CPU tier of the z fit: the oracle's bounded Brent (oracle/picasso_oracle.c:fminbound) against scipy itself
(tests/golden/_zfit_restate.py) in the bits of z and sq, on the hostile input sets the GPU tier runs through the kernel
(tests/test_gpu_zfit.py), and the proof that those sets hold what they are for."""
import math
import os
import sys

import numpy as np
import pytest
import scipy

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import _zfit_restate as zr  # noqa: E402
from oracle import oracle as orc  # noqa: E402

print(f"scipy {scipy.__version__}")


@pytest.fixture(scope="module")
def census():
    return {name: zr.census(name) for name in zr.SETS}


@pytest.mark.parametrize("name", list(zr.SETS))
def test_oracle_equals_scipy_in_bits(name):
    """Every row of every call of the set: z and sq of the oracle have scipy's bits (NaN masks equal).  A row may
    differ only if pow(v, 0.5) != sqrt(v) for an argument v the target saw on scipy's path (zr.pow_sqrt_witness), and
    such rows are at most 1 % of the set.  The oracle takes sqrt since glibc's pow put 21 of the 1500 `ordinary` rows
    (1.4 %) and 2 of the 250 `x_negative_beyond_300` rows on another path, so the count printed here is 0 in every set."""
    rows = differing = 0
    for label, sx, sy, cx, cy in zr.SETS[name]():
        z, sq = zr.fit(sx, sy, cx, cy)
        zo, sqo = orc.zfit(sx, sy, cx, cy, threads=2)
        rows += len(z)
        for i in np.flatnonzero(~(zr.bits_equal(z, zo) & zr.bits_equal(sq, sqo))):
            differing += 1
            assert zr.pow_sqrt_witness(sx[i], sy[i], cx, cy), (
                f"{name}/{label} row {i} (sx {sx[i]!r}, sy {sy[i]!r}): scipy z {z[i]!r} sq {sq[i]!r}, oracle z {zo[i]!r} "
                f"sq {sqo[i]!r}, and no pow/sqrt difference on scipy's path")
    print(f"{name}: {differing} of {rows} rows differ with a pow/sqrt witness")
    assert differing <= rows // 100


@pytest.mark.parametrize("name", list(zr.SETS))
def test_sets_hold_what_they_are_for(name, census):
    """From scipy's results alone: each set has at least zr.HOLDS[name] rows ending on the lower / upper bound, with a
    NaN sq, and with a parabolic / golden last step.  No set can reach the 500-evaluation cap, so that class is dropped:
    a golden step shrinks the bracket by 0.62, an accepted parabolic step is shorter than half the step before the
    last and every step is at least tol1 > 3.3e-6, so [-1000, 1000] is down to 2 tol2 within a few dozen evaluations
    whatever the target returns: a NaN fu fails `fu <= fx`, so the else branch moves a or b to the (finite) x and the
    bracket shrinks all the same.  That no row is capped is asserted instead; the largest count scipy reports is
    printed."""
    c = census[name]
    print(name, c)
    for what, least in zr.HOLDS[name].items():
        assert c[what] >= least, (name, what, c)
    assert c["capped"] == 0 and c["max_nfev"] < zr.MAXFUN, c


def test_every_class_is_held_by_some_set():
    for what in ("lower", "upper", "nan", "parabolic", "golden"):
        assert any(what in h for h in zr.HOLDS.values()), what


def test_reference_call_shape_is_the_bounded_method():
    """The reference names no method; scipy picks "bounded" when bounds are given, with xatol 1e-5 and maxiter 500."""
    from scipy.optimize import minimize_scalar
    cx, cy = zr.calibration()
    args = (np.float64(1.25), np.float64(2.5), zr._f64s(cx), zr._f64s(cy))
    a = minimize_scalar(zr._target, bounds=[-1000, 1000], args=args)
    b = minimize_scalar(zr._target, bounds=(-1000, 1000), method="bounded", args=args, options={"xatol": 1e-5, "maxiter": 500})
    assert (a.x, a.fun, a.nfev) == (b.x, b.fun, b.nfev)
    z, sq = zr.fit([1.25], [2.5], cx, cy)
    assert z[0] == a.x and sq[0] == a.fun
    assert zr.evaluated(1.25, 2.5, cx, cy)[0] == zr.FIRST_POINT and len(zr.evaluated(1.25, 2.5, cx, cy)) == a.nfev


def test_target_edges():
    """The restated target: float32 widths are widened, a negative finite width is NaN, -inf is +inf like pow."""
    cx, cy = zr.calibration()
    wx, wy = zr.widths(100.0, cx, cy)
    want = (np.sqrt(np.float64(np.float32(1.3))) - np.sqrt(wx)) ** 2 + (np.sqrt(np.float64(np.float32(0.7))) - np.sqrt(wy)) ** 2
    assert zr.target(100.0, np.float32(1.3), np.float32(0.7), cx, cy) == want
    neg = zr._poly(c6=-1.0)
    assert np.isnan(zr.target(0.0, 1.0, 1.0, neg, cy)) and np.isnan(zr.target(0.0, -1.0, 1.0, cx, cy))
    assert zr.target(0.0, 1.0, 1.0, zr._poly(c6=-np.inf), cy) == np.inf
    assert np.isnan(zr.target(np.nan, 1.0, 1.0, cx, cy))


def test_root_is_pow_half_at_the_special_values():
    """_root against the `** 0.5` the reference writes (NumPy's float64 power, C pow) and math.pow, where the two can
    differ from sqrt in more than rounding: -inf gives +inf, a finite negative and NaN give NaN, -0.0 gives a zero."""
    with np.errstate(all="ignore"):
        for v in (-np.inf, -1.0, -1e-300, -0.0, 0.0, 0.25, 4.0, np.inf, np.nan):
            got, want = zr._root(np.float64(v)), np.float64(v) ** 0.5
            assert (np.isnan(got) and np.isnan(want)) or got == want, (v, got, want)
            if v == v and not v < 0:
                assert got == math.pow(v, 0.5)
        assert math.pow(-math.inf, 0.5) == math.inf and np.isnan(np.sqrt(np.float64(-np.inf)))
