#!/usr/bin/env python3
"""Mint tests/golden/combine_cases.npz: the reference's own ``cluster_combine`` and ``cluster_combine_dist`` on small
tables.

TEST INFRASTRUCTURE, build container only (needs the reference tree, pandas and SciPy; no numba).  The two functions
are compiled from where they lie in the reference's ``postprocess.py`` and run as they are (plain pandas / NumPy /
SciPy; ``tqdm`` is stubbed); nothing of the reference is stored here.

Combine cases store ``in_columns`` / ``in_<column>`` and the returned table (``columns``, ``dtypes``, ``out_<column>``).
Distance cases store the same plus ``pixelsize`` (JSON: which kind of number, and its value).  ``edges`` records the
exceptions the reference raises (type and text), ``signatures`` the two signatures, ``versions`` the pandas, NumPy and
SciPy versions.  The script asserts that each situation the cases are there for occurs and that the restatement
(tests/golden/_combine_restate.py) reproduces every table in bits.

Run:  python tests/golden/make_goldens_combine.py
"""
import ast
import inspect
import json
import os
import sys
import warnings

import numpy as np
import pandas as pd
import scipy
from scipy.spatial import distance

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _combine_restate as rs  # noqa: E402

REF = os.environ.get("PICASSO_REFERENCE", "/root/reference")
POSTPROCESS_PY = os.path.join(REF, "picasso", "postprocess.py")
NAMES = ("cluster_combine", "cluster_combine_dist")
LENGTHS = (1, 2, 7, 8, 9, 127, 128, 129, 1000)
DIST_GROUPS = (2, 3, 63, 64, 65, 300)
warnings.simplefilter("ignore")


def load_reference():
    ns = {"np": np, "pd": pd, "distance": distance, "tqdm": lambda it, **k: it}
    tree = ast.parse(open(POSTPROCESS_PY).read())
    keep = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in NAMES]
    assert [n.name for n in keep] == list(NAMES)
    mod = ast.Module(body=[ast.ImportFrom("__future__", [ast.alias("annotations")], 0)] + keep, type_ignores=[])
    exec(compile(ast.fix_missing_locations(mod), POSTPROCESS_PY, "exec"), ns)
    return ns


# ---- clustered tables ---------------------------------------------------------------------------------------
def clustered(rng, pairs, lengths, three, coord=np.float32, photons=np.float32, frame=np.uint32, label=np.int32,
              shuffle=True):
    """``pairs``: the (group, cluster) label of every segment, ``lengths`` their sizes; rows interleaved."""
    which = np.repeat(np.arange(len(pairs)), lengths)
    if shuffle:
        which = rng.permutation(which)
    n = len(which)
    pairs = np.asarray(pairs)
    centre = rng.uniform(5, 250, (len(pairs), 3))
    cols = {"frame": rng.integers(0, 60000, n).astype(frame),
            "x": (centre[which, 0] + rng.normal(0, 0.05, n)).astype(coord),
            "y": (centre[which, 1] + rng.normal(0, 0.05, n)).astype(coord)}
    if three:
        cols["z"] = (centre[which, 2] * 4 - 500 + rng.normal(0, 20, n)).astype(coord)
    cols["photons"] = (rng.uniform(200, 90000, n) * 10.0 ** rng.integers(-1, 2, n)).astype(photons)
    cols["group"] = pairs[which, 0].astype(label)
    cols["cluster"] = pairs[which, 1].astype(label)
    return cols


def sweep_table():
    """4 096 segments of one row and one of 20 000, interleaved (not stored: the tests compare with the restatement)."""
    rng = np.random.default_rng(13)
    pairs = [(i % 7 - 3, i) for i in range(4096)] + [(2, 5000)]
    return clustered(rng, pairs, [1] * 4096 + [20000], True)


NINE = [(-3, 5), (-3, -2), (-3, 40), (0, 7), (0, 1), (0, -9), (12, 1), (12, 0), (12, 5)]      # out of order on purpose


def combine_cases():
    rng = np.random.default_rng(20261101)
    cases = {}
    cases["a_2d_f32_u32_i32"] = clustered(rng, NINE, LENGTHS, False)
    cases["b_3d_f64_i64_i64"] = clustered(rng, NINE, LENGTHS[::-1], True, np.float64, np.float64, np.int64, np.int64)
    cases["c_3d_f32_labels_f64"] = clustered(rng, NINE, LENGTHS, True, label=np.float64)
    mixed = clustered(rng, NINE, (3, 130, 9, 1, 40, 2, 260, 8, 17), True)
    mixed["y"] = mixed["y"].astype(np.float64)
    mixed["z"] = mixed["z"].astype(np.float64)
    mixed["photons_other"] = mixed["photons"].astype(np.float64)           # not read
    cases["d_3d_mixed_types"] = mixed
    wide = clustered(rng, NINE, (5, 9, 33, 1, 2, 140, 64, 16, 8), False, photons=np.float64)   # float32 x, float64 weights
    cases["d_2d_f64_weights"] = wide
    nan = clustered(rng, NINE, (6, 20, 150, 1, 9, 8, 2, 300, 12), False)
    at = lambda g, c: np.flatnonzero((nan["group"] == g) & (nan["cluster"] == c))  # noqa: E731
    nan["photons"][at(-3, -2)[3]] = np.nan
    nan["x"][at(12, 0)[100]] = np.nan
    nan["y"][at(0, 1)[0]] = np.nan
    nan["y"][at(12, 1)[1]] = np.nan                                        # a two-row cluster with one value left
    cases["e_2d_nan"] = nan
    pairs = [(g, c) for g in (-40, -1, 0, 3, 1000) for c in range(-2, 58)]
    cases["f_300_small"] = clustered(rng, pairs, rng.integers(1, 6, len(pairs)), True, label=np.int64)
    cases["g_sorted_table"] = clustered(rng, sorted(NINE), (4, 9, 1, 30, 2, 8, 129, 3, 5), False, shuffle=False)
    return cases


# ---- combined tables for the distances ----------------------------------------------------------------------
def combined(rng, sizes, three, group_dtype=np.float64, shuffle=False, first_group=-2):
    group = np.repeat(np.arange(len(sizes)) * 3 + first_group, sizes)
    cluster = np.concatenate([rng.permutation(m) * 2 - 5 for m in sizes])
    n = len(group)
    if not shuffle:
        at = np.lexsort((cluster, group))
        group, cluster = group[at], cluster[at]
    else:
        at = rng.permutation(n)
        group, cluster = group[at], cluster[at]
    cols = {"group": group.astype(group_dtype), "cluster": cluster.astype(np.int32),
            "mean_frame": rng.uniform(0, 60000, n).astype(np.float32),
            "x": rng.uniform(10, 14, n).astype(np.float32), "y": rng.uniform(20, 24, n).astype(np.float32)}
    if three:
        cols["z"] = rng.uniform(-400, 400, n).astype(np.float32)
    cols["std_frame"] = rng.uniform(0, 9000, n).astype(np.float32)
    cols["lpx"] = rng.uniform(0.001, 0.05, n).astype(np.float32)
    cols["lpy"] = rng.uniform(0.001, 0.05, n).astype(np.float32)
    if three:
        cols["lpz"] = rng.uniform(1, 30, n).astype(np.float32)
    cols["n"] = rng.integers(1, 400, n).astype(np.int32)
    return cols


def dist_cases(ref, combine):
    rng = np.random.default_rng(20261102)
    cases = {}
    flat = combined(rng, DIST_GROUPS, False)
    twins = np.flatnonzero(flat["group"] == flat["group"][10])[:2]
    flat["x"][twins[1]], flat["y"][twins[1]] = flat["x"][twins[0]], flat["y"][twins[0]]       # two rows at one place
    cases["h_2d"] = (flat, None)
    deep = combined(rng, DIST_GROUPS, True)
    g0 = np.flatnonzero(deep["group"] == deep["group"][0])                 # the group of two is rows 0, 1
    assert len(g0) == 2
    g1 = np.flatnonzero(deep["group"] == deep["group"][2])                 # the group of three: near in xy, far in z
    assert len(g1) == 3
    deep["x"][g1], deep["y"][g1] = np.float32([11.0, 11.01, 11.5]), np.float32([21.0, 21.0, 21.0])
    deep["z"][g1] = np.float32([0.0, 390.0, 5.0])
    tw = np.flatnonzero(deep["group"] == deep["group"][-1])[:2]
    for c in ("x", "y", "z"):
        deep[c][tw[1]] = deep[c][tw[0]]
    cases["i_3d_none"] = (deep, None)
    cases["i_3d_int"] = (deep, 130)
    cases["i_3d_int_108"] = (deep, 108)
    cases["i_3d_float"] = (deep, 107.5)
    cases["i_3d_np_float64"] = (deep, np.float64(107.5))
    cases["j_3d_int_groups_shuffled"] = (combined(rng, (5, 2, 70, 9), True, np.int32, shuffle=True), None)
    cases["j_2d_shuffled"] = (combined(rng, (4, 2, 66), False, np.int64, shuffle=True), None)
    chain = ref["cluster_combine"](pd.DataFrame(combine["c_3d_f32_labels_f64"]))
    cases["k_after_combine_3d"] = ({c: chain[c].to_numpy() for c in chain.columns}, None)
    chain = ref["cluster_combine"](pd.DataFrame(combine["e_2d_nan"]))
    cases["k_after_combine_2d_nan"] = ({c: chain[c].to_numpy() for c in chain.columns}, None)
    return cases


def pixelsize_json(p):
    kind = "none" if p is None else ("np.float64" if isinstance(p, np.float64) else type(p).__name__)
    return json.dumps({"kind": kind, "value": None if p is None else float(p)})


def pixelsize_from(text):
    d = json.loads(str(text))
    return {"none": lambda v: None, "int": int, "float": float, "np.float64": np.float64}[d["kind"]](d["value"])


def record(fn):
    try:
        return {"returns": fn()}
    except Exception as e:  # noqa: BLE001
        return {"raises": type(e).__name__, "text": str(e)}


def edge_calls(combine, dist):
    """(label, function, columns, pixelsize)"""
    zero = {c: v.copy() for c, v in combine["a_2d_f32_u32_i32"].items()}
    zero["photons"][(zero["group"] == 0) & (zero["cluster"] == 1)] = 0
    flat = dist["h_2d"][0]
    single = {c: v[:3].copy() for c, v in flat.items()}                    # the group of two, and one row of the next
    repeated = {c: v.copy() for c, v in flat.items()}
    three = np.flatnonzero(repeated["group"] == repeated["group"][2])
    repeated["cluster"][three[1]] = repeated["cluster"][three[0]]
    both = {c: v.copy() for c, v in flat.items()}                          # a pair of equal labels: amin comes first
    both["cluster"][1] = both["cluster"][0]
    return [("zero weight sum", "cluster_combine", zero, None),
            ("empty table", "cluster_combine", {c: v[:0] for c, v in zero.items()}, None),
            ("single-cluster group", "cluster_combine_dist", single, None),
            ("repeated label", "cluster_combine_dist", repeated, None),
            ("two rows, one label", "cluster_combine_dist", both, None),
            ("empty table", "cluster_combine_dist", {c: v[:0] for c, v in flat.items()}, None)]


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    if a.dtype.kind == "f":
        nan = np.isnan(a)
        return np.array_equal(nan, np.isnan(b)) and np.array_equal(a[~nan].view(np.uint8), b[~nan].view(np.uint8))
    return np.array_equal(a, b)


def store(out, p, cols, res):
    out[p + "in_columns"] = np.array(list(cols))
    for c, v in cols.items():
        out[p + "in_" + c] = v
    assert isinstance(res.index, pd.RangeIndex) and res.index.start == 0 and res.index.step == 1
    out[p + "columns"] = np.array(list(res.columns))
    out[p + "dtypes"] = np.array([str(res[c].dtype) for c in res.columns])
    for c in res.columns:
        out[p + "out_" + c] = res[c].to_numpy()


def differing(again, res):
    assert list(again) == list(res.columns), (list(again), list(res.columns))
    return [c for c in again if not same(again[c], res[c].to_numpy())]


def main():
    ref = load_reference()
    out = {"versions": np.array(json.dumps({"pandas": pd.__version__, "numpy": np.__version__, "scipy": scipy.__version__})),
           "signatures": np.array(json.dumps({n: str(inspect.signature(ref[n])) for n in NAMES}))}

    combine = combine_cases()
    out["combine_case_names"] = np.array(list(combine))
    for name, cols in combine.items():
        p = "combine/" + name + "/"
        res = ref["cluster_combine"](pd.DataFrame(cols))
        store(out, p, cols, res)
        off = differing(rs.cluster_combine(cols), res)
        print(f"combine {name:26s} rows={len(cols['frame']):5d} clusters={len(res):4d} restatement differs in", off)
        assert not off, (name, off)

    dist = dist_cases(ref, combine)
    out["dist_case_names"] = np.array(list(dist))
    for name, (cols, pixelsize) in dist.items():
        p = "dist/" + name + "/"
        res = ref["cluster_combine_dist"](pd.DataFrame(cols), pixelsize)
        store(out, p, cols, res)
        out[p + "pixelsize"] = np.array(pixelsize_json(pixelsize))
        assert same(pixelsize_from(out[p + "pixelsize"]), pixelsize) and type(pixelsize_from(out[p + "pixelsize"])) is type(pixelsize)
        off = differing(rs.cluster_combine_dist(cols, pixelsize), res)
        print(f"dist    {name:26s} rows={len(cols['x']):5d} restatement differs in", off)
        assert not off, (name, off)

    # ---- each situation occurs --------------------------------------------------------------------------------
    a = {c: out["combine/a_2d_f32_u32_i32/out_" + c] for c in out["combine/a_2d_f32_u32_i32/columns"]}
    assert sorted(a["n"]) == sorted(LENGTHS) and list(a["group"]) == sorted(a["group"]) and a["group"][0] < 0
    assert list(a) == ["group", "cluster", "mean_frame", "x", "y", "std_frame", "lpx", "lpy", "n"]
    assert a["group"].dtype == np.float64 and a["cluster"].dtype == np.int32 and a["n"].dtype == np.int32
    one = int(np.flatnonzero(a["n"] == 1)[0])
    assert np.isnan(a["std_frame"][one]) and np.isnan(a["lpx"][one]) and np.isfinite(a["x"][one])
    assert (np.diff(combine["a_2d_f32_u32_i32"]["group"].astype(np.int64)) < 0).any()
    b = "combine/b_3d_f64_i64_i64/"
    assert list(out[b + "columns"]) == ["group", "cluster", "mean_frame", "x", "y", "z", "std_frame", "lpx", "lpy", "lpz", "n"]
    assert out[b + "out_cluster"].dtype == np.int64 and out[b + "in_frame"].dtype == np.int64 and out[b + "in_x"].dtype == np.float64
    assert out["combine/c_3d_f32_labels_f64/out_cluster"].dtype == np.float64
    d = combine["d_3d_mixed_types"]
    assert (d["x"].dtype, d["y"].dtype, d["photons"].dtype) == (np.float32, np.float64, np.float32)
    assert combine["d_2d_f64_weights"]["photons"].dtype == np.float64 and combine["d_2d_f64_weights"]["x"].dtype == np.float32
    e = {c: out["combine/e_2d_nan/out_" + c] for c in out["combine/e_2d_nan/columns"]}
    pick = lambda g, c: int(np.flatnonzero((e["group"] == g) & (e["cluster"] == c))[0])  # noqa: E731
    assert np.isnan(e["x"][pick(-3, -2)]) and np.isnan(e["y"][pick(-3, -2)]) and np.isfinite(e["lpx"][pick(-3, -2)])
    assert np.isnan(e["x"][pick(12, 0)]) and np.isfinite(e["y"][pick(12, 0)]) and np.isfinite(e["lpx"][pick(12, 0)])
    assert np.isnan(e["lpy"][pick(12, 1)]) and e["n"][pick(12, 1)] == 2
    assert len(out["combine/f_300_small/out_n"]) == 300
    h = {c: out["dist/h_2d/out_" + c] for c in out["dist/h_2d/columns"]}
    assert list(h)[-1] == "min_dist" and "mind_dist_xy" not in h and (h["min_dist"] == 0).sum() == 2
    assert sorted(np.unique(h["group"], return_counts=True)[1]) == sorted(DIST_GROUPS)
    i = {c: out["dist/i_3d_none/out_" + c] for c in out["dist/i_3d_none/columns"]}
    assert list(i)[-2:] == ["min_dist", "mind_dist_xy"] and (i["min_dist"] == 0).sum() == 2
    three = np.flatnonzero(i["group"] == i["group"][2])
    assert np.isclose(i["mind_dist_xy"][three[0]], 0.01, atol=1e-4) and i["min_dist"][three[0]] < 0.6 and i["min_dist"][three[0]] > 0.4
    assert not same(out["dist/i_3d_int_108/out_min_dist"], out["dist/i_3d_none/out_min_dist"])
    assert same(out["dist/i_3d_int/out_min_dist"], out["dist/i_3d_none/out_min_dist"])
    assert not same(out["dist/i_3d_float/out_min_dist"], out["dist/i_3d_np_float64/out_min_dist"])      # float32 against float64 z
    j = dist["j_3d_int_groups_shuffled"][0]
    assert j["group"].dtype == np.int32 and out["dist/j_3d_int_groups_shuffled/out_group"].dtype == np.int32
    assert not np.array_equal(out["dist/j_3d_int_groups_shuffled/out_cluster"],
                              j["cluster"][np.argsort(j["group"], kind="stable")])                      # misaligned, as recorded
    assert np.isnan(out["dist/k_after_combine_2d_nan/out_min_dist"]).sum() >= 2

    edges = []
    for i_edge, (label, fn, cols, pixelsize) in enumerate(edge_calls(combine, dist)):
        got = record(lambda: ref[fn](pd.DataFrame(cols)) if fn == "cluster_combine" else ref[fn](pd.DataFrame(cols), pixelsize))
        assert "raises" in got, label
        again = record(lambda: (rs.cluster_combine if fn == "cluster_combine" else rs.cluster_combine_dist)(cols))
        if len(cols["group"]):
            assert again.get("raises") == got["raises"], (label, again, got)
        edges.append({"label": label, "function": fn, "raises": got["raises"], "text": got["text"]})
        out[f"edge{i_edge}_columns"] = np.array(list(cols))
        for c, v in cols.items():
            out[f"edge{i_edge}_in_{c}"] = v
        print("edge   ", label, fn, got["raises"], repr(got["text"]))
    assert edges[0]["raises"] == "ZeroDivisionError" and edges[0]["text"] == rs.ZERO_WEIGHTS
    assert all(e["raises"] == "ValueError" for e in edges[1:])
    out["edges"] = np.array(json.dumps(edges))

    # beyond one NumPy buffer: the restatement against the reference on a segment of 20 000 rows (not stored)
    rng = np.random.default_rng(5)
    big = clustered(rng, [(0, 0), (0, 1), (1, 0)], (20000, 3, 9000), True)
    assert not differing(rs.cluster_combine(big), ref["cluster_combine"](pd.DataFrame(big)))
    big = clustered(rng, [(0, 0), (0, 1)], (20000, 8193), False, np.float64, np.float64, np.int64)
    assert not differing(rs.cluster_combine(big), ref["cluster_combine"](pd.DataFrame(big)))

    path = os.path.join(HERE, "combine_cases.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 512 * 1024


if __name__ == "__main__":
    main()
