#!/usr/bin/env python3
"""Mint tests/golden/centers_cases.npz: the tables of the reference's own ``find_cluster_centers`` on small
clustered tables.

TEST INFRASTRUCTURE, build container only (needs the reference tree, pandas and scipy; no numba).  The functions of
the reference's ``clusterer.py`` named in NAMES are compiled from where they lie, as make_goldens_cluster.py does;
nothing of the reference is stored here.

Every case stores its input columns (``in_*``), its ``pixelsize`` and the returned table: ``columns``, ``dtypes``,
``index`` and one ``out_*`` array per column.  The versions of pandas, NumPy and SciPy the file was minted under are
stored in ``versions``.  What the reference does with an empty table, with a NaN coordinate and with a 3-D table
without a pixel size is recorded in ``edges``.  The script asserts that each situation the cases are there for occurs.

Run:  python tests/golden/make_goldens_centers.py
"""
import ast
import json
import os
import sys
import warnings

import numpy as np
import pandas as pd
import scipy
from scipy.spatial import ConvexHull, QhullError

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _centers_restate as rs  # noqa: E402

REF = os.environ.get("PICASSO_REFERENCE", "/root/reference")
CLUSTERER_PY = os.path.join(REF, "picasso", "clusterer.py")
NAMES = ("_aggregate_cluster_stats", "_count_binding_events", "_cluster_convex_hulls", "_weighted_z_means",
         "find_cluster_centers")
warnings.simplefilter("ignore")


class _Lib:
    IntArray1D = FloatArray1D = object


def load_reference():
    ns = {"np": np, "pd": pd, "ConvexHull": ConvexHull, "QhullError": QhullError, "lib": _Lib}
    tree = ast.parse(open(CLUSTERER_PY).read())
    keep = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in NAMES]
    assert len(keep) == len(NAMES), [n.name for n in keep]
    mod = ast.Module(body=[ast.ImportFrom("__future__", [ast.alias("annotations")], 0)] + keep, type_ignores=[])
    exec(compile(ast.fix_missing_locations(mod), CLUSTERER_PY, "exec"), ns)
    return ns


# ---- tables -------------------------------------------------------------------------------------------------
def table(rng, frame, x, y, group, dtype=np.float32, z=None, frame_dtype=np.uint32):
    n = len(x)
    cols = {"frame": np.asarray(frame).astype(frame_dtype), "x": np.asarray(x, dtype), "y": np.asarray(y, dtype)}
    if z is not None:
        cols["z"] = np.asarray(z, np.float32)
    for c, (lo, hi) in {"photons": (500, 9000), "sx": (0.8, 1.5), "sy": (0.8, 1.5), "bg": (5, 40)}.items():
        cols[c] = rng.uniform(lo, hi, n).astype(np.float32)
    if z is not None:
        cols["lpx"] = rng.uniform(0.005, 0.06, n).astype(np.float32)
        cols["lpy"] = rng.uniform(0.005, 0.06, n).astype(np.float32)
    cols["net_gradient"] = rng.uniform(3000, 20000, n).astype(np.float32)
    cols["group"] = np.asarray(group, np.int32)
    return cols


def sites(rng, n_sites, per_site, n_frames, dims=2, size=64.0):
    """Blinking sites, rows shuffled: the rows of a group lie between those of the others in table order."""
    centres = rng.uniform(2, size - 2, (n_sites, dims))
    if dims == 3:
        centres[:, 2] = rng.uniform(-300, 300, n_sites)
    sizes = rng.integers(max(3, per_site // 2), per_site * 2, n_sites)
    which = np.repeat(np.arange(n_sites), sizes)
    pts = centres[which] + rng.normal(0, 0.02, (len(which), dims))
    if dims == 3:
        pts[:, 2] = centres[which, 2] + rng.normal(0, 12.0, len(which))
    frame = rng.integers(0, n_frames, len(which))
    order = rng.permutation(len(which))
    return frame[order], pts[order], which[order]


def edge_table(rng):
    """Hand-made groups; labels with gaps and a negative one, rows interleaved."""
    rows = []      # (group, frame, x, y)

    def add(group, frames, xs, ys):
        rows.extend(zip([group] * len(frames), frames, xs, ys))

    add(-3, [5, 6, 7, 40, 41, 90], rng.normal(10, 0.05, 6), rng.normal(10, 0.05, 6))            # a negative label
    add(0, [17], [3.25], [4.5])                                                                  # one row
    add(2, [30, 10], [5.0, 5.5], [6.0, 6.25])                                                    # two rows, decreasing frame
    add(7, [1, 2, 3, 4, 5], [8.125] * 5, [9.375] * 5)                                            # exact duplicates
    add(9, [0, 3, 6, 10, 14, 17], [1.0, 2.5, 1.75, 4.0, 3.0, 2.0], [7.5] * 6)                    # collinear, equal y; gaps of 3 and 4
    add(100, [50, 20, 21, 19, 60, 64, 67, 3], rng.normal(20, 0.05, 8), rng.normal(5, 0.05, 8))   # uint32 frames that decrease
    add(101, list(range(0, 40, 2)), rng.normal(30, 0.05, 20), rng.normal(30, 0.05, 20))          # NaN photons, inf bg go here
    add(4000, [7, 7, 8, 300, 304, 307], rng.normal(40, 0.05, 6), rng.normal(41, 0.05, 6))
    # interleave without changing the order inside a group
    keys = np.concatenate([np.sort(rng.uniform(0, 1, sum(1 for r in rows if r[0] == g))) for g in dict.fromkeys(r[0] for r in rows)])
    rows = [rows[i] for i in np.argsort(keys, kind="stable")]
    group, frame, x, y = (np.array(v) for v in zip(*rows))
    cols = table(rng, frame, x, y, group)
    at = np.flatnonzero(group == 101)
    cols["photons"][at[3]] = np.nan
    cols["photons"][at[11]] = np.nan
    cols["bg"][at[5]] = np.inf
    cols["sx"][np.flatnonzero(group == 0)[0]] = np.nan             # a group whose only value is NaN
    cols["group_input"] = (group % 5).astype(np.int32)
    return cols


def make_cases():
    rng = np.random.default_rng(20261018)
    cases = {}
    fr, pts, which = sites(rng, 60, 40, 5000)
    cases["sites2d_f32"] = (table(rng, fr, pts[:, 0], pts[:, 1], which), None)
    cases["sites2d_f64"] = (table(rng, fr, pts[:, 0], pts[:, 1], which, np.float64), None)
    fr, pts, which = sites(rng, 25, 30, 5000, dims=3)
    cases["sites3d"] = (table(rng, fr, pts[:, 0], pts[:, 1], which, z=pts[:, 2]), 130)
    cases["edges2d"] = (edge_table(rng), None)
    # one group of 5000 rows at large coordinates between small ones: a float32 Kahan sum and a float64 sum part
    fr, pts, which = sites(rng, 6, 10, 5000)
    big = np.stack([rng.normal(2000.3, 0.4, 5000), rng.normal(1777.7, 0.4, 5000)], axis=1)
    order = rng.permutation(len(which) + 5000)
    cases["large_coordinates"] = (table(rng, np.r_[fr, rng.integers(0, 5000, 5000)][order], np.r_[pts[:, 0], big[:, 0]][order],
                                        np.r_[pts[:, 1], big[:, 1]][order], np.r_[which, np.full(5000, 6)][order]), None)
    fr, pts, which = sites(rng, 300, 5, 5000)
    cols = table(rng, fr, pts[:, 0], pts[:, 1], which * 3 - 20, frame_dtype=np.int64)
    cases["groups300"] = (cols, None)
    return cases


def outcome(fn):
    try:
        res = fn()
        return {"returns": list(res.columns), "rows": len(res)}
    except Exception as e:  # noqa: BLE001
        return {"raises": type(e).__name__, "message": str(e)}


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def main():
    ref = load_reference()
    fcc = ref["find_cluster_centers"]
    out = {"versions": np.array(json.dumps({"pandas": pd.__version__, "numpy": np.__version__, "scipy": scipy.__version__}))}
    cases = make_cases()
    out["case_names"] = np.array(list(cases))
    for name, (cols, pixelsize) in cases.items():
        p = name + "/"
        out[p + "pixelsize"] = np.array(-1 if pixelsize is None else pixelsize)
        out[p + "in_columns"] = np.array(list(cols))
        for c, v in cols.items():
            out[p + "in_" + c] = v
        res = fcc(pd.DataFrame(cols), pixelsize)
        assert isinstance(res.index, pd.RangeIndex) and res.index.start == 0 and res.index.step == 1
        out[p + "columns"] = np.array(list(res.columns))
        out[p + "dtypes"] = np.array([str(res[c].dtype) for c in res.columns])
        out[p + "n_rows"] = np.array(len(res))
        for c in res.columns:
            out[p + "out_" + c] = res[c].to_numpy()
        # the restatement, here as well as in the tests
        again, order = rs.centers(cols, pixelsize, res["convexhull"].to_numpy())
        assert list(again) == list(res.columns), name
        off = {c: int((again[c].view(np.uint32) != res[c].to_numpy().view(np.uint32)).sum()) for c in again
               if not same(again[c], res[c].to_numpy())}
        print(f"{name:20s} rows={len(cols['x']):6d} groups={len(res):4d} restatement differs in", off)
        assert set(off) <= {"convexhull"}, (name, off)

    # each situation occurs
    e = {c: out["edges2d/out_" + c] for c in [str(c) for c in out["edges2d/columns"]]}
    g = list(e["group"])
    assert g == sorted(g) and g[0] < 0 and np.any(np.diff(g) > 1)
    i = g.index(0)
    assert e["n_locs"][i] == 1 and np.isnan(e["std_x"][i]) and e["convexhull"][i] == 0 and np.isnan(e["sx"][i])
    assert e["n_locs"][g.index(2)] == 2 and e["convexhull"][g.index(2)] == 0 and e["n_events"][g.index(2)] == 2
    assert e["convexhull"][g.index(7)] == 0 and e["std_x"][g.index(7)] == 0
    assert e["convexhull"][g.index(9)] == 0 and e["std_y"][g.index(9)] == 0 and e["n_events"][g.index(9)] == 3
    assert e["n_events"][g.index(100)] == 6                 # 50 | 20 21 19 (wrap) | 60 | 64 67 | 3 (wrap): 50, 19, 60, 64, 3 + first
    assert np.isfinite(e["photons"][g.index(101)]) and np.isinf(e["bg"][g.index(101)])
    assert "group_input" in e and (e["convexhull"][[g.index(k) for k in (-3, 100, 101, 4000)]] > 0).all()
    cols = cases["large_coordinates"][0]
    big = cols["group"] == 6
    assert np.float32(cols["x"][big].astype(np.float64).sum() / big.sum()) != out["large_coordinates/out_x"][6] or \
        np.float32(cols["y"][big].astype(np.float64).sum() / big.sum()) != out["large_coordinates/out_y"][6]
    assert out["groups300/n_rows"] == 300 and out["groups300/out_group"].min() < 0
    assert out["sites2d_f64/in_x"].dtype == np.float64 and "z" in [str(c) for c in out["sites3d/columns"]]
    which = cases["sites2d_f32"][0]["group"]
    assert (np.diff(which) != 0).mean() > 0.9               # interleaved

    cols = {c: v.copy() for c, v in cases["edges2d"][0].items()}
    cols["x"][np.flatnonzero(cols["group"] == 101)[2]] = np.nan
    for c, v in cols.items():
        out["nan_x/in_" + c] = v
    out["nan_x/in_columns"] = np.array(list(cols))
    empty = {c: v[:0] for c, v in cases["sites2d_f32"][0].items()}
    edges = {"nan_x": outcome(lambda: fcc(pd.DataFrame(cols))),
             "empty": outcome(lambda: fcc(pd.DataFrame(empty))),
             "3d without pixelsize": outcome(lambda: fcc(pd.DataFrame(cases["sites3d"][0])))}
    print("edges", json.dumps(edges))
    out["edges"] = np.array(json.dumps(edges))
    path = os.path.join(HERE, "centers_cases.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) <= os.path.getsize(os.path.join(HERE, "pairs_cases.npz"))


if __name__ == "__main__":
    main()
