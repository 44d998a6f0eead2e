#!/usr/bin/env python3
"""Mint tests/golden/frc_cases.npz: the reference's own ``frc`` / ``_frc`` on small tables.

TEST INFRASTRUCTURE, build container only (needs the reference tree and pandas).  ``frc`` and ``_frc`` are compiled
from where they lie in the reference's ``postprocess.py``, ``threshold_tukey`` and ``loess_smooth`` from its
``masking.py`` (the function-picking loader of make_goldens_areas.py); ``render`` and ``radial_sum`` are the reference's
modules behind the import shim (_refshim.py).  ``statsmodels`` is not installed here: ``lowess`` is a stand-in that
returns its input, so NOTHING of the smoothed curve or the resolution is recorded.  ``nena`` is a stand-in that returns
the case's ``lp``.  Nothing of the reference is stored here.

Per case: ``x`` / ``y`` (float32), ``idx1`` / ``idx2`` (the rows of the two halves: the reference's own split for the
``frc`` cases), ``viewport_in`` and ``viewport`` (after ``frc``'s squaring), ``pixelsize``, ``lp``, ``m`` (render side),
``n`` (odd side), ``masked1`` / ``masked2``, ``R`` (the reference's curve, float32) and ``frequencies``.  ``kinds`` says
which entry point ran, ``nondegenerate`` which cases have power in both images.  The script asserts that the restatement
(_frc_restate.py) reproduces masked images and frequencies in bits and that NumPy's float64 transform (T) is nearer to
the longdouble truth (L) than the reference's single-precision curve (R) on every non-degenerate case.

Run:  python tests/golden/make_goldens_frc.py
"""
import json
import os
import sys
import types
import warnings

import numpy as np
import pandas as pd

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _frc_restate as rs  # noqa: E402
import _refshim  # noqa: E402
from make_goldens_areas import _compile, _get_from_metadata  # noqa: E402

REF = _refshim.REF
PIXELSIZE = 130
LP = 0.25                      # oversampling 2 / lp = 8: a viewport of m / 8 camera pixels renders to m pixels exactly
OV = 2 / LP


def load_reference(captured):
    ref = _refshim.load_reference()
    masking = _compile(os.path.join(REF, "picasso", "masking.py"), ("threshold_tukey", "loess_smooth"),
                       {"np": np, "loess": lambda arr, x, frac, return_sorted=False: arr})
    lib = types.SimpleNamespace(get_from_metadata=_get_from_metadata)
    ns = {"np": np, "pd": pd, "lib": lib, "render": ref["render"], "imageprocess": ref["imageprocess"],
          "masking": types.SimpleNamespace(**{k: masking[k] for k in ("threshold_tukey", "loess_smooth")}),
          "nena": lambda locs, info: (None, captured["lp"])}
    _compile(os.path.join(REF, "picasso", "postprocess.py"), ("frc", "_frc"), ns)
    inner = ns["_frc"]

    def spy(locs1, locs2, pixelsize, lp, viewport):       # the reference's own halves and squared viewport
        captured["idx1"], captured["idx2"] = locs1.index.to_numpy(), locs2.index.to_numpy()
        captured["viewport"] = viewport
        return inner(locs1, locs2, pixelsize, lp, viewport)

    ns["_frc"] = spy
    return ns, inner


def sites(rng, m, per_site=12, sigma=0.15, lo=0.0, hi=1.0):
    """Blinking sites in [lo, hi] of the field of m / OV camera pixels, rows shuffled."""
    size = m / OV
    n_sites = max(2, m * m // 40)
    centres = rng.uniform(lo * size, hi * size, (n_sites, 2))
    pts = np.repeat(centres, per_site, axis=0) + rng.normal(0, sigma, (n_sites * per_site, 2))
    pts = pts[rng.permutation(len(pts))]
    return pts[:, 0].astype(np.float32), pts[:, 1].astype(np.float32)


def cases():
    """name -> (kind, x, y, viewport, render side m)."""
    rng = np.random.default_rng(20261019)
    out = {}
    sq = lambda m: ((0.0, 0.0), (m / OV, m / OV))  # noqa: E731
    for m in (5, 31, 33, 37, 63, 65, 129):
        out[f"dense_{m}"] = ("_frc",) + sites(rng, m) + (sq(m), m)
    for m in (4, 34, 64):                                  # even renders: the last row and column are dropped
        out[f"crop_{m}"] = ("_frc",) + sites(rng, m) + (sq(m), m)
    out["empty_5"] = ("_frc", np.zeros(0, np.float32), np.zeros(0, np.float32), sq(5), 5)
    out["side_1"] = ("_frc",) + sites(rng, 1, sigma=0.01, lo=0.4, hi=0.6) + (sq(1), 1)
    out["single_3"] = ("frc", np.array([0.2], np.float32), np.array([0.21], np.float32), sq(3), 3)
    out["quadrant_65"] = ("_frc",) + sites(rng, 65, lo=0.08, hi=0.5) + (sq(65), 65)       # everything in one quadrant
    x, y = sites(rng, 33)
    out["nonsquare_tall"] = ("frc", x, y + np.float32(1.5), ((0.0, 0.0), (33 / OV + 3.0, 33 / OV)), 33)
    x, y = sites(rng, 37)
    out["nonsquare_wide"] = ("frc", x + np.float32(2.0), y, ((0.0, 0.0), (37 / OV, 37 / OV + 4.0)), 37)
    return out


def main():
    captured = {}
    ns, inner = load_reference(captured)
    store = {}
    names, kinds, good = [], [], []
    report = []
    for name, (kind, x, y, viewport, m) in cases().items():
        locs = pd.DataFrame({"x": x, "y": y, "lpx": np.full(len(x), LP, np.float32), "lpy": np.full(len(x), LP, np.float32)})
        captured["lp"] = LP
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            if kind == "frc":
                res = ns["frc"](locs, [{"Pixelsize": PIXELSIZE}], viewport)
                curve, freq, images = res["frc_curve"], res["frequencies"], res["images"]
                idx1, idx2, squared = captured["idx1"], captured["idx2"], captured["viewport"]
                mine = rs.split(x, y, viewport)
                assert np.array_equal(mine[0], idx1) and np.array_equal(mine[1], idx2) and mine[2] == squared, name
            else:
                perm = np.random.default_rng(len(x)).permutation(len(x))
                idx1, idx2, squared = perm[: len(perm) // 2], perm[len(perm) // 2:], viewport
                curve, _, freq, _, images = inner(locs.iloc[idx1], locs.iloc[idx2], PIXELSIZE, LP, viewport)
        m1, m2 = images
        n = m1.shape[0]
        assert m1.dtype == np.float32 and n == (m if m % 2 else m - 1) and curve.dtype == np.float32, (name, n, curve.dtype)
        # the restatement gives the reference's bits
        ov = PIXELSIZE / (PIXELSIZE / (1 / (LP / 2)))
        mine1 = rs.masked(rs.render_hist(x[idx1], y[idx1], ov, squared))
        mine2 = rs.masked(rs.render_hist(x[idx2], y[idx2], ov, squared))
        assert mine1.tobytes() == m1.tobytes() and mine2.tobytes() == m2.tobytes(), name
        assert rs.frequencies(len(curve), n, PIXELSIZE, LP).tobytes() == freq.tobytes(), name
        live = bool(m1.any() and m2.any())
        if live:
            truth = rs.curve_L(m1, m2)
            e_t, e_r = rs.err_L(rs.curve_T(m1, m2), truth), rs.err_L(curve, truth)
            assert e_t < e_r, (name, e_t, e_r)
            report.append(f"{name}: n = {n}, err_L(T) = {e_t:.3g}, err_L(R) = {e_r:.3g}")
        else:
            assert not curve.any(), name
            report.append(f"{name}: n = {n}, degenerate (an image without power), curve all zero")
        names.append(name), kinds.append(kind), good.append(live)
        for key, val in (("x", x), ("y", y), ("idx1", idx1.astype(np.int64)), ("idx2", idx2.astype(np.int64)),
                         ("viewport_in", np.array(viewport, np.float64)), ("viewport", np.array(squared, np.float64)),
                         ("pixelsize", np.float64(PIXELSIZE)), ("lp", np.float64(LP)), ("m", np.int64(m)), ("n", np.int64(n)),
                         ("masked1", m1), ("masked2", m2), ("R", curve), ("frequencies", freq)):
            store[f"{name}/{key}"] = val
    store["case_names"] = np.array(names)
    store["kinds"] = np.array(kinds)
    store["nondegenerate"] = np.array(good)
    store["versions"] = np.array(json.dumps({"numpy": np.__version__, "pandas": pd.__version__}))
    path = os.path.join(HERE, "frc_cases.npz")
    np.savez_compressed(path, **store)
    print("\n".join(report))
    print(f"wrote {path}: {len(names)} cases, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
