#!/usr/bin/env python3
"""Mint tests/golden/areas_cases.npz: the reference's own ``cluster_areas`` and ``test_subclustering`` on small tables.

TEST INFRASTRUCTURE, build container only (needs the reference tree, pandas and SciPy; no numba, no sklearn).
``_cluster_area``, ``cluster_areas`` and ``test_subclustering`` are compiled from where they lie in the reference's
``clusterer.py`` and ``threshold_otsu`` from its ``masking.py``, and run as they are (``tqdm`` and the metadata lookup
are stubbed); nothing of the reference is stored here.

Area cases store ``in_columns`` / ``in_<column>``, ``pixelsize`` and the returned table (``columns``, ``dtypes``,
``index``, ``out_<column>``).  Subclustering cases store the same inputs, the two distances and ``out_clustered`` /
``out_sparse``.  ``edges`` records what the reference returns or raises (type and text) and where, ``signatures`` the
two public signatures, ``versions`` the pandas, NumPy and SciPy versions, ``lds_bins`` the bound of the device's LDS
path the three boundary images of ``lds2d`` / ``lds3d`` were made for (``--lds-bins``, by default the library's),
``one_row_shapes`` the edges, image shape and value of the one-row groups of ``one_rows2d`` / ``one_rows3d``.
The script asserts that each situation the cases are there for occurs and that the restatement
(tests/golden/_areas_restate.py) reproduces every table in bits.

Run:  python tests/golden/make_goldens_areas.py [--lds-bins N]
"""
import argparse
import ast
import inspect
import json
import os
import sys
import types
import warnings

import numpy as np
import pandas as pd
import scipy
from scipy.ndimage import gaussian_filter
from scipy.spatial import KDTree

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _areas_restate as rs  # noqa: E402

REF = os.environ.get("PICASSO_REFERENCE", "/root/reference")
CLUSTERER_PY = os.path.join(REF, "picasso", "clusterer.py")
MASKING_PY = os.path.join(REF, "picasso", "masking.py")
NAMES = ("_cluster_area", "cluster_areas", "test_subclustering")
PUBLIC = ("cluster_areas", "test_subclustering")
LDS_BINS = 4096                 # AREAS_LDS_BINS of the library (tests/test_areas_host.py holds the two together)
PIXELSIZE = 130
MOL_PIXELSIZE = 160             # 25 / 160 and 80 / 160 are exact in binary
LP_EXACT = 0.015625             # bins of 2 ** -7: the hand-made groups have exact edges
LP_GENERIC = 0.013              # a float32 bin that is no power of two: min + bin is rounded
# edges per axis of the groups of ONE row in one_rows2d / one_rows3d, by label: float32 rounding of (min + bin) - min
# decides between 1 and 2 edges per axis, so between an empty image, shape (1, 0) and a single bin
ONE_ROWS = {2: {1: (2, 1), 2: (1, 2), 3: (2, 2), 4: (1, 1)}, 3: {1: (2, 2, 2), 2: (2, 1, 2), 3: (2, 2, 1), 4: (1, 1, 1)}}


def _get_from_metadata(info, key, default=None, *, raise_error=False):
    for d in reversed([info] if isinstance(info, dict) else list(info)):
        if d.get(key):
            return d[key]
    if raise_error:
        raise KeyError(f"Key '{key}' not found in metadata.")
    return default


def _compile(path, names, ns):
    tree = ast.parse(open(path).read())
    keep = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in names]
    assert [n.name for n in keep] == list(names), [n.name for n in keep]
    mod = ast.Module(body=[ast.ImportFrom("__future__", [ast.alias("annotations")], 0)] + keep, type_ignores=[])
    exec(compile(ast.fix_missing_locations(mod), path, "exec"), ns)
    return ns


def load_reference():
    masking = _compile(MASKING_PY, ("threshold_otsu",), {"np": np})
    lib = types.SimpleNamespace(get_from_metadata=_get_from_metadata)
    ns = {"np": np, "pd": pd, "gaussian_filter": gaussian_filter, "KDTree": KDTree, "lib": lib,
          "masking": types.SimpleNamespace(threshold_otsu=masking["threshold_otsu"]),
          "tqdm": lambda it, **k: it}
    return _compile(CLUSTERER_PY, NAMES, ns)


# ---- tables -------------------------------------------------------------------------------------------------
def table(rng, x, y, group, dtype=np.float32, z=None, lp=(0.005, 0.02), x_dtype=None):
    n = len(x)
    cols = {"x": np.asarray(x).astype(x_dtype or dtype), "y": np.asarray(y).astype(dtype)}
    if z is not None:
        cols["z"] = np.asarray(z).astype(dtype)
    if np.isscalar(lp):
        cols["lpx"], cols["lpy"] = np.full(n, lp, np.float32), np.full(n, lp, np.float32)
    else:
        cols["lpx"], cols["lpy"] = rng.uniform(*lp, n).astype(np.float32), rng.uniform(*lp, n).astype(np.float32)
    cols["group"] = np.asarray(group).astype(np.int32)
    return cols


def sites(rng, n_sites, per_site, dims=2, size=64.0, centre=0.0, sigma=(0.008, 0.03)):
    """Blinking sites, rows shuffled; labels 3 * site - 1: -1 is one of them, the labels have gaps and lie in no order."""
    centres = rng.uniform(2, size - 2, (n_sites, dims)) + centre
    sizes = rng.integers(max(3, per_site // 2), per_site * 2, n_sites)
    which = np.repeat(np.arange(n_sites), sizes)
    s = rng.uniform(*sigma, n_sites)
    pts = centres[which] + rng.normal(0, 1, (len(which), dims)) * s[which, None]
    if dims == 3:
        sz = rng.choice([2.0, 12.0], n_sites)                     # nm: a few z bins, or a few dozen
        pts[:, 2] = rng.uniform(-300, 300, n_sites)[which] + rng.normal(0, 1, len(which)) * sz[which]
    order = rng.permutation(len(which))
    return pts[order], (which * 3 - 1)[order]


def interleave(rng, rows):
    """Rows of hand-made groups mixed without changing the order inside a group."""
    labels = list(dict.fromkeys(r[0] for r in rows))
    keys = np.concatenate([np.sort(rng.uniform(0, 1, sum(1 for r in rows if r[0] == g))) for g in labels])
    by_group = [r for g in labels for r in rows if r[0] == g]
    return [by_group[i] for i in np.argsort(keys, kind="stable")]


B = LP_EXACT / 2                # the bin of the hand-made tables
HAND = {"one_row": 0, "two_identical": 2, "line": 5, "one_bin": 7, "narrow": 9, "max_on_edge": 40, "edge_beyond": 41,
        "cloud": 100, "noise": -1}


def edge_table(rng, dtype, three=False):
    rows = []      # (group, x, y, z in nm)

    def add(name, xs, ys, zs=None):
        zs = np.zeros(len(xs)) if zs is None else zs
        rows.extend(zip([HAND[name]] * len(xs), xs, ys, zs))

    add("noise", rng.uniform(20, 21, 30), rng.uniform(20, 20.2, 30), rng.uniform(-40, 40, 30))
    add("one_row", [3.25], [4.5], [10.0])
    add("two_identical", [5.5, 5.5], [6.25, 6.25], [-20.0, -20.0])
    add("line", 8 + B * np.array([0, 3.3, 7.9, 12.5, 20.2, 31.7]), [9.375] * 6, [0.0] * 6)                  # no extent in y (nor z)
    add("one_bin", [2.0, 2.0 + 0.25 * B, 2.0 + 0.125 * B], [3.0, 3.0 + 0.25 * B, 3.0], [0.0, 0.1, 0.05])      # a 1 x 1 (x 1) image
    # 3 bins in x, 30 in y; in 3-D one z bin (2.5 * B * PIXELSIZE nm wide)
    add("narrow", 12 + B * rng.uniform(0, 2.4, 40), 13 + B * np.r_[0, 29.4, rng.uniform(0, 29.4, 38)], rng.uniform(0, 0.5, 40))
    add("max_on_edge", 1.0 + B * np.array([0, 5, 1.5, 2.5, 3.25]), 2.0 + B * np.array([0, 11, 3.5, 6.5, 9.75]),
        B * 2.5 * PIXELSIZE * np.array([0, 0.75, 0.5, 0.25, 1.5]))                                        # 3-D: two z bins
    add("edge_beyond", 1.0 + B * np.array([0, 5.5, 1.5, 2.5, 3.25]), 4.0 + B * np.array([0, 11.5, 3.5, 6.5, 9.75]),
        B * 2.5 * PIXELSIZE * np.array([0, 1.5, 0.5, 0.25, 1.25]))
    add("cloud", rng.normal(30, 0.05, 200), rng.normal(31, 0.08, 200), rng.normal(100, 6, 200))
    group, x, y, z = (np.array(v) for v in zip(*interleave(rng, rows)))
    return table(rng, x, y, group, dtype, z=z if three else None, lp=LP_EXACT)


def factors(n, dims):
    """n as a product of `dims` factors, as equal as they come."""
    best = None
    for a in range(1, int(n ** 0.5) + 1 if dims == 2 else int(round(n ** (1 / 3))) + 2):
        if n % a:
            continue
        rest = [(n // a,)] if dims == 2 else [(b, n // a // b) for b in range(a, int((n // a) ** 0.5) + 1) if (n // a) % b == 0]
        for r in rest:
            f = (a,) + r
            if best is None or max(f) < max(best):
                best = f
    return best


def lds_table(rng, dims, bound):
    """Three groups whose images hold bound - 1, bound and bound + 1 bins: two corner rows set the shape, the others
    fill it."""
    rows = []
    for k, n in enumerate((bound - 1, bound, bound + 1)):
        shape = factors(n, dims)
        size = np.array([B, B, B * 2.5][:dims])
        lo = np.array([4.0 + 8 * k, 16.0, 0.0][:dims])
        pts = np.vstack([lo, lo + (np.array(shape) - 0.5) * size, lo + rng.uniform(0, 1, (150, dims)) * (np.array(shape) - 0.5) * size])
        if dims == 3:
            pts[:, 2] *= PIXELSIZE
        rows.extend((k + 1, *p) for p in pts)
    rows = interleave(rng, [r if dims == 3 else (*r, 0.0) for r in rows])
    group, x, y, z = (np.array(v) for v in zip(*rows))
    return table(rng, x, y, group, np.float64, z=z if dims == 3 else None, lp=LP_EXACT)


def one_row_table(dims):
    """Groups of one row at generic float32 coordinates, found by search: one per pattern of ONE_ROWS, beside a cloud."""
    rng = np.random.default_rng(5 + dims)
    lp = np.float32(LP_GENERIC)
    found = {}
    for _ in range(100000):
        if len(found) == len(ONE_ROWS[dims]):
            break
        p = np.r_[rng.uniform(1, 60, 2), rng.uniform(-300, 300)].astype(np.float32)
        cols = {"x": p[:1], "y": p[1:2], **({"z": p[2:]} if dims == 3 else {})}
        lens = tuple(len(e) for e in rs.edges_of(rs.points(cols, np.arange(1), PIXELSIZE), lp))
        for label, want in ONE_ROWS[dims].items():
            if lens == want and label not in found:
                found[label] = p
    assert len(found) == len(ONE_ROWS[dims]), sorted(found)
    rows = [(label, *p) for label, p in sorted(found.items())]
    rows += [(50, *p) for p in np.c_[rng.normal(30, 0.05, 200), rng.normal(31, 0.08, 200), rng.normal(100, 6, 200)]]
    group, x, y, z = (np.array(v) for v in zip(*interleave(rng, rows)))
    return table(rng, x, y, group, np.float32, z=z if dims == 3 else None, lp=LP_GENERIC)


def area_cases(bound=LDS_BINS):
    rng = np.random.default_rng(20261019)
    cases = {}
    pts, which = sites(rng, 60, 40)
    cases["sites2d_f32"] = table(rng, pts[:, 0], pts[:, 1], which)
    cases["sites2d_f64"] = table(rng, pts[:, 0], pts[:, 1], which, np.float64)
    cases["x_only_f64"] = table(rng, pts[:, 0], pts[:, 1], which, x_dtype=np.float64)
    pts, which = sites(rng, 30, 30, dims=3)
    cases["sites3d"] = table(rng, pts[:, 0], pts[:, 1], which, z=pts[:, 2])
    cases["edges2d_f32"] = edge_table(rng, np.float32)
    cases["edges2d_f64"] = edge_table(rng, np.float64)
    cases["edges3d_f32"] = edge_table(rng, np.float32, True)
    cases["edges3d_f64"] = edge_table(rng, np.float64, True)
    pts, which = sites(rng, 40, 30, centre=2000.0, sigma=(0.004, 0.01))
    cases["large_coordinates"] = table(rng, pts[:, 0], pts[:, 1], which, lp=(0.003, 0.005))
    pts, which = sites(rng, 300, 8)
    cases["groups300"] = table(rng, pts[:, 0], pts[:, 1], which)
    cases["lds2d"] = lds_table(rng, 2, bound)
    cases["lds3d"] = lds_table(rng, 3, bound)
    cases["one_rows2d"] = one_row_table(2)
    cases["one_rows3d"] = one_row_table(3)
    return cases


def mol_cases():
    rng = np.random.default_rng(7)
    cases = {}
    for name, three, dtype in (("mols2d", False, np.float32), ("mols3d", True, np.float32), ("mols2d_f64", False, np.float64)):
        n = 400
        x, y = rng.uniform(0, 40, n), rng.uniform(0, 40, n)
        z = rng.uniform(-200, 200, n)
        # isolated pairs at exactly clustering_dist / pixelsize and at exactly sparse_dist / pixelsize
        x[:4], y[:4] = [100.0, 100.0 + 25 / MOL_PIXELSIZE, 200.0, 200.0], [100.0, 100.0, 300.0, 300.0 + 80 / MOL_PIXELSIZE]
        z[:4] = 0.0
        if three:
            x[4:6], y[4:6], z[4:6] = 400.0, 400.0, [0.0, 25.0]           # the same, along z in nm
        cols = {"x": x.astype(dtype), "y": y.astype(dtype)}
        if three:
            cols["z"] = z.astype(dtype)
        cols["n_events"] = rng.integers(1, 40, n).astype(np.int32)
        cases[name] = cols
    return cases


def outcome(fn):
    try:
        res = fn()
    except Exception as e:  # noqa: BLE001
        return {"raises": type(e).__name__, "message": str(e)}
    if isinstance(res, pd.DataFrame):
        return {"returns": list(res.columns), "dtypes": [str(d) for d in res.dtypes], "rows": len(res),
                "values": [float(v) for v in res.iloc[:, 1].to_numpy()[:8]]}
    return {"returns": [str(a.dtype) for a in res], "rows": [len(a) for a in res]}


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def edge_inputs(cases):
    """name -> (columns, info) of the situations whose outcome is recorded, not decided here."""
    info = [{"Pixelsize": PIXELSIZE}]
    base = cases["sites2d_f32"]
    first = int(np.flatnonzero(base["group"] == 5)[2])

    def changed(**kw):
        cols = {c: v.copy() for c, v in base.items()}
        for c, v in kw.items():
            if callable(v):
                v(cols[c])
            else:
                cols[c] = v
        return cols

    def put(value, at=first):
        return lambda a: a.__setitem__(at, value)

    n = len(base["x"])
    one_first = changed(group=np.where(np.arange(n) == 0, -7, base["group"]).astype(np.int32), lpx=np.zeros(n, np.float32),
                        lpy=np.zeros(n, np.float32))
    return {
        "empty": ({c: v[:0] for c, v in base.items()}, info),
        "no group": ({c: v for c, v in base.items() if c != "group"}, info),
        "no Pixelsize": (base, [{"Width": 64}]),
        "lp 0": (changed(lpx=np.zeros(n, np.float32), lpy=np.zeros(n, np.float32)), info),
        "lp 0, first group of one row": (one_first, info),
        "lp nan": (changed(lpx=np.full(n, np.nan, np.float32), lpy=np.full(n, np.nan, np.float32)), info),
        "nan x": (changed(x=put(np.nan)), info),
        "nan y": (changed(y=put(np.nan)), info),
        "inf x": (changed(x=put(np.inf)), info),
        "-inf y": (changed(y=put(-np.inf)), info),
        "nan z": ({**{c: v.copy() for c, v in cases["sites3d"].items()},
                   "z": np.where(np.arange(len(cases["sites3d"]["z"])) == 11, np.nan, cases["sites3d"]["z"]).astype(np.float32)}, info),
    }


def main():
    warnings.simplefilter("ignore")
    ap = argparse.ArgumentParser()
    ap.add_argument("--lds-bins", type=int, default=LDS_BINS)
    bound = ap.parse_args().lds_bins
    ref = load_reference()
    info = [{"Pixelsize": PIXELSIZE}]
    out = {"versions": np.array(json.dumps({"pandas": pd.__version__, "numpy": np.__version__, "scipy": scipy.__version__})),
           "signatures": np.array(json.dumps({n: str(inspect.signature(ref[n])) for n in PUBLIC})),
           "lds_bins": np.array(bound), "pixelsize": np.array(PIXELSIZE), "mol_pixelsize": np.array(MOL_PIXELSIZE)}
    cases = area_cases(bound)
    out["case_names"] = np.array(list(cases))
    shapes = {}
    for name, cols in cases.items():
        p = name + "/"
        assert len(cols["x"]) <= 5000 and len(np.unique(cols["group"])) <= 300, name
        out[p + "in_columns"] = np.array(list(cols))
        for c, v in cols.items():
            out[p + "in_" + c] = v
        seen = []
        res = ref["cluster_areas"](pd.DataFrame(cols), info, seen.append)
        assert isinstance(res.index, pd.RangeIndex) and res.index.start == 0 and res.index.step == 1
        assert seen == list(range(1, len(res) + 1))
        out[p + "columns"] = np.array(list(res.columns))
        out[p + "dtypes"] = np.array([str(res[c].dtype) for c in res.columns])
        out[p + "n_rows"] = np.array(len(res))
        for c in res.columns:
            out[p + "out_" + c] = res[c].to_numpy()
        key, groups, values = rs.areas(cols, info)
        assert [key] == list(res.columns[1:]) and same(groups, res["group"].to_numpy()), name
        assert same(values, res[key].to_numpy()), (name, np.flatnonzero(values != res[key].to_numpy()))
        lp = rs.median_lp(cols)
        shapes[name] = {int(g): tuple(len(e) - 1 for e in rs.edges_of(rs.points(cols, np.flatnonzero(cols["group"] == g), PIXELSIZE), lp))
                        for g in groups}
        sizes = [int(np.prod(np.maximum(s, 0))) for s in shapes[name].values()]
        print(f"{name:20s} rows={len(cols['x']):5d} groups={len(res):4d} bins {min(sizes)} .. {max(sizes)}, "
              f"{sum(s > bound for s in sizes)} above the bound; {key} {res[key].min()} .. {res[key].max()}")

    # each situation occurs
    for name in ("sites2d_f32", "sites3d", "groups300"):
        g = cases[name]["group"]
        assert -1 in g and (np.diff(np.unique(g)) > 1).any() and (np.diff(g) < 0).any(), name
    assert cases["sites2d_f64"]["x"].dtype == np.float64 and "z" in cases["sites3d"]
    assert cases["x_only_f64"]["x"].dtype == np.float64 and cases["x_only_f64"]["y"].dtype == np.float32
    assert str(out["sites3d/columns"][1]) == "Volume (LP^3)" and str(out["sites2d_f32/columns"][1]) == "Area (LP^2)"
    assert any(np.prod(s) > bound for s in shapes["sites3d"].values()) and any(0 < np.prod(s) <= bound for s in shapes["sites3d"].values())
    for name in ("edges2d_f32", "edges2d_f64", "edges3d_f32", "edges3d_f64"):
        s, cols = shapes[name], cases[name]
        area = dict(zip(out[name + "/out_group"].tolist(), out[name + "/out_" + str(out[name + "/columns"][1])].tolist()))
        print(name, "one row:", s[HAND["one_row"]], "->", area[HAND["one_row"]], " two identical:", s[HAND["two_identical"]],
              "->", area[HAND["two_identical"]], " line:", s[HAND["line"]], " one bin:", s[HAND["one_bin"]], "->", area[HAND["one_bin"]])
        assert (cols["group"] == HAND["one_row"]).sum() == 1 and (cols["group"] == HAND["two_identical"]).sum() == 2
        assert set(s[HAND["one_bin"]]) == {1} and area[HAND["one_bin"]] == (1 / 4 if len(s[0]) == 2 else 1 / (16 / 5))
        assert s[HAND["narrow"]][0] < rs.RADIUS < s[HAND["narrow"]][1]
        assert s[HAND["line"]][0] > rs.RADIUS and s[HAND["line"]][1] <= 1
        if len(s[0]) == 3:
            assert s[HAND["narrow"]][2] == 1 and s[HAND["max_on_edge"]][2] == 2
        if name.endswith("f64"):
            rows = np.flatnonzero(cols["group"] == HAND["max_on_edge"])
            e = rs.edges_of(rs.points(cols, rows, PIXELSIZE), rs.median_lp(cols))
            assert e[0][-1] == cols["x"][rows].max() and e[1][-1] == cols["y"][rows].max()
            rows = np.flatnonzero(cols["group"] == HAND["edge_beyond"])
            e = rs.edges_of(rs.points(cols, rows, PIXELSIZE), rs.median_lp(cols))
            assert e[0][-1] > cols["x"][rows].max() and e[1][-1] > cols["y"][rows].max()
    out["one_row_shape_f32"] = np.array(shapes["edges2d_f32"][HAND["one_row"]])
    # one row at generic float32 coordinates: 1 or 2 edges per axis, as the rounding of min + bin falls
    one_rows = {}
    for name, dims in (("one_rows2d", 2), ("one_rows3d", 3)):
        s, cols = shapes[name], cases[name]
        area = dict(zip(out[name + "/out_group"].tolist(), out[name + "/out_" + str(out[name + "/columns"][1])].tolist()))
        for label, lens in ONE_ROWS[dims].items():
            assert (cols["group"] == label).sum() == 1 and s[label] == tuple(n - 1 for n in lens), (name, label, s[label])
            one_bin = all(n == 2 for n in lens)
            assert area[label] == ((1 / 4 if dims == 2 else 1 / (16 / 5)) if one_bin else 0.0), (name, label, area[label])
        one_rows[name] = {str(label): {"edges": list(lens), "shape": list(s[label]), "value": area[label]}
                          for label, lens in ONE_ROWS[dims].items()}
        print(name, json.dumps(one_rows[name]))
    assert one_rows["one_rows2d"]["1"]["shape"] == [1, 0] and one_rows["one_rows2d"]["3"] == {"edges": [2, 2], "shape": [1, 1], "value": 0.25}
    out["one_row_shapes"] = np.array(json.dumps(one_rows))
    spacing = np.spacing(np.float32(2000.0)) / (rs.median_lp(cases["large_coordinates"]) / 2)
    assert cases["large_coordinates"]["x"].min() > 2000 and spacing > 0.03, spacing
    for name, dims in (("lds2d", 2), ("lds3d", 3)):
        sizes = sorted(int(np.prod(s)) for s in shapes[name].values())
        assert sizes == [bound - 1, bound, bound + 1] and all(len(s) == dims and min(s) > 0 for s in shapes[name].values()), sizes

    edges = {}
    for name, (cols, inf) in edge_inputs(cases).items():
        edges[name] = outcome(lambda: ref["cluster_areas"](pd.DataFrame(cols), inf, lambda i: None))
        print(f"edge {name!r}: {json.dumps(edges[name])}")

    mols = mol_cases()
    mol_info = [{"Pixelsize": MOL_PIXELSIZE}]
    out["mol_names"] = np.array(list(mols))
    for name, cols in mols.items():
        p = "mols/" + name + "/"
        out[p + "in_columns"] = np.array(list(cols))
        for c, v in cols.items():
            out[p + "in_" + c] = v
        close, far = ref["test_subclustering"](pd.DataFrame(cols), mol_info)
        out[p + "out_clustered"], out[p + "out_sparse"] = close, far
        again = rs.subclustering(cols, mol_info)
        assert same(again[0], close) and same(again[1], far), name
        # the pair at exactly clustering_dist is not clustered, the pair at exactly sparse_dist is sparse
        pts = rs.points(cols, np.arange(len(cols["x"])), MOL_PIXELSIZE).astype(np.float64)
        nnd = KDTree(pts).query(pts, k=2)[0][:, 1]
        assert (nnd[:2] == 25 / MOL_PIXELSIZE).all() and (nnd[2:4] == 80 / MOL_PIXELSIZE).all(), (name, nnd[:4])
        if "z" in cols:
            assert (nnd[4:6] == 25 / MOL_PIXELSIZE).all()
        close_d, far_d = ref["test_subclustering"](pd.DataFrame(cols), mol_info, 25.000001, 80.000001)
        assert len(close_d) == len(close) + (4 if "z" in cols else 2) and len(far_d) == len(far) - 2, name
        print(f"mols {name}: {len(close)} clustered, {len(far)} sparse of {len(cols['x'])}")
    m2 = mols["mols2d"]
    edges["mols: no n_events"] = outcome(lambda: ref["test_subclustering"](pd.DataFrame({c: v for c, v in m2.items() if c != "n_events"}), mol_info))
    edges["mols: sparse_dist <= clustering_dist"] = outcome(lambda: ref["test_subclustering"](pd.DataFrame(m2), mol_info, 80, 80))
    edges["mols: no Pixelsize"] = outcome(lambda: ref["test_subclustering"](pd.DataFrame(m2), [{}]))
    for k in list(edges)[-3:]:
        print(f"edge {k!r}: {json.dumps(edges[k])}")
    out["edges"] = np.array(json.dumps(edges))

    path = os.path.join(HERE, "areas_cases.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 1 << 20


if __name__ == "__main__":
    main()
