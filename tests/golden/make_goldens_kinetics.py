#!/usr/bin/env python3
"""Mint tests/golden/kinetics_cases.npz: the reference's own ``_dark_times`` / ``dark_times`` / ``compute_dark_times``
and ``groupprops`` on small tables.

TEST INFRASTRUCTURE, build container only (needs the reference tree and pandas; no numba).  The four functions are
compiled from where they lie in the reference's ``postprocess.py``; nothing of the reference is stored here.
``groupprops`` is pure pandas and runs as it is.  ``_dark_times`` is a ``@numba.jit`` function and runs as a Python
loop with its scalar arithmetic typed as numba types it: the binary operations are routed through ``nb_binop`` below
(two unsigned integers meet in uint64 and wrap, every other pair of integers meets in int64; arrays follow the dtypes
alone, as ``_nbemu.binop`` has it), and NumPy 2 compares a uint64 with an int64 by value, as numba does.  Every case
has at most 2000 rows.

Dark cases store ``in_*`` columns, the ``group`` argument (``arg_group``, absent for None), the returned array
(``dark``) and the table ``compute_dark_times`` returns (``cdt_columns``, ``cdt_index``, ``cdt_<column>``).  Group
property cases store ``in_*`` and the returned table (``columns``, ``dtypes``, ``out_*``).  ``edges`` records what the
reference does before any arithmetic: without ``len``, without ``dark``, on empty tables.  ``versions`` holds the
pandas, NumPy and SciPy versions.  The script asserts that each situation the cases are there for occurs.

Run:  python tests/golden/make_goldens_kinetics.py
"""
import ast
import itertools
import json
import os
import sys
import types
import warnings
from typing import Callable, Literal

import numpy as np
import pandas as pd
import scipy

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _kinetics_restate as rs  # noqa: E402
import _nbemu  # noqa: E402

REF = os.environ.get("PICASSO_REFERENCE", "/root/reference")
POSTPROCESS_PY = os.path.join(REF, "picasso", "postprocess.py")
NAMES = ("compute_dark_times", "dark_times", "_dark_times", "groupprops")
warnings.simplefilter("ignore")


def nb_binop(name, a, b):
    """numba's integer scalars: int (op) int is at least 64 bits wide, unsigned only when both are."""
    a, b = _nbemu._lift(a), _nbemu._lift(b)
    if isinstance(a, np.integer) and isinstance(b, np.integer) and name in ("Add", "Sub", "Mult"):
        unsigned = a.dtype.kind == "u" and b.dtype.kind == "u"
        if not unsigned and np.uint64 in (type(a), type(b)):
            raise TypeError("numba computes uint64 (op) int64 in float64: not a table this project takes")
        v = _nbemu._OPS[name](int(a), int(b)) % 2 ** 64
        return np.uint64(v) if unsigned else np.int64(v - 2 ** 64 if v >= 2 ** 63 else v)
    return _nbemu.binop(name, a, b)


class _Lib:
    IntArray1D = FloatArray1D = object


def load_reference():
    numba = types.SimpleNamespace(jit=lambda *a, **k: (lambda fn: fn))
    tqdm = lambda **k: range(k["total"])  # noqa: E731   (never reached: no case passes "console")
    ns = {"np": np, "pd": pd, "itertools": itertools, "numba": numba, "tqdm": tqdm, "lib": _Lib, "Callable": Callable,
          "Literal": Literal, "__nb_binop__": nb_binop}
    tree = ast.parse(open(POSTPROCESS_PY).read())
    keep = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in NAMES]
    assert len(keep) == len(NAMES), [n.name for n in keep]
    tr = _nbemu._Retype()
    keep = [tr.visit(n) for n in keep]
    assert tr.rewritten == ["_dark_times"], tr.rewritten
    mod = ast.Module(body=[ast.ImportFrom("__future__", [ast.alias("annotations")], 0)] + keep, type_ignores=[])
    exec(compile(ast.fix_missing_locations(mod), POSTPROCESS_PY, "exec"), ns)
    return ns


# ---- dark-time tables ---------------------------------------------------------------------------------------
def events(rng, n, n_groups, n_frames, frame_dtype=np.uint32, len_dtype=np.uint32, sort=True, group=True):
    frame = rng.integers(0, n_frames, n)
    if sort:
        frame = np.sort(frame)
    cols = {"frame": frame.astype(frame_dtype), "x": rng.uniform(0, 64, n).astype(np.float32),
            "y": rng.uniform(0, 64, n).astype(np.float32), "photons": rng.uniform(500, 9000, n).astype(np.float32)}
    if group:
        cols["group"] = rng.integers(0, n_groups, n).astype(np.int32)
    cols["len"] = rng.integers(1, 25, n).astype(len_dtype)
    cols["n"] = np.maximum(cols["len"].astype(np.int64) - rng.integers(0, 3, n), 1).astype(len_dtype)
    return cols


def edge_events(frame_dtype, len_dtype, top):
    """Hand-made groups, rows not sorted by frame; ``top`` is the table's largest frame."""
    rows = [      # (group, frame, len)
        (-4, 100, 0), (-4, 95, 5), (-4, 40, 3), (-4, 120, 2),       # len 0: own last frame 99 < 100, and another row ends at 99
        (0, 100, 0), (0, 80, 11), (0, 130, 1),                      # len 0, the next candidate ends at 90
        (3, 10, 50), (3, 20, 10), (3, 30, 5), (3, 61, 2),           # overlap: differences <= 0
        (7, 5, 6), (7, 8, 3), (7, 2, 9), (7, 30, 1), (7, 11, 1),    # three rows end at frame 10; one starts at 11
        (12, 0, 1), (12, top, 2),                                   # the dark time equals max_frame: -1
        (500, 0, 0), (500, top, 1),                                 # 0 + 0 - 1; a signed dark time would exceed max_frame
        (501, 0, 0), (501, 7, 0),                                   # 0 + 0 - 1 again: 8 frames signed, none where it wraps
        (9, 77, 4),                                                 # a group of one
        (2000, 300, 5), (2000, 200, 5), (2000, 250, 5), (2000, 100, 5), (2000, 204, 1),
    ]
    order = np.random.default_rng(3).permutation(len(rows))
    group, frame, length = (np.array(v) for v in zip(*[rows[i] for i in order]))
    n = len(rows)
    return {"frame": frame.astype(frame_dtype), "x": np.linspace(1, 2, n).astype(np.float32),
            "group": group.astype(np.int32), "len": length.astype(len_dtype), "n": np.ones(n, len_dtype)}


def dark_cases():
    rng = np.random.default_rng(20261018)
    cases = {}
    cases["one_row"] = ({"frame": np.array([5], np.uint32), "x": np.array([1.5], np.float32),
                         "len": np.array([3], np.uint32)}, None)
    cases["one_group_300"] = (events(rng, 300, 1, 20000, sort=False, group=False), None)
    singles = events(rng, 300, 1, 20000)
    singles["group"] = rng.permutation(300).astype(np.int32)
    cases["singles_300"] = (singles, None)
    sites = events(rng, 1500, 60, 30000)
    cases["sites_column"] = (sites, None)
    split = sites["group"].astype(np.int64) * 2 + (sites["x"] > 32)
    cases["sites_split_i64"] = (sites, split)
    cases["sites_split_f64"] = (sites, split.astype(np.float64))
    cases["sites_i32_arg_no_column"] = ({c: v for c, v in sites.items() if c != "group"}, (sites["group"] * 7 - 90).astype(np.int32))
    cases["edges_u32"] = (edge_events(np.uint32, np.uint32, 5000), None)
    cases["edges_i64"] = (edge_events(np.int64, np.int32, 5000), None)
    cases["edges_i32_unsorted"] = (events(rng, 400, 9, 3000, np.int32, np.int32, sort=False), None)
    return cases


# ---- group-property tables ----------------------------------------------------------------------------------
def props_table(rng, n_groups, per_group, labels=None):
    sizes = rng.integers(1, per_group * 2, n_groups)
    which = rng.permutation(np.repeat(np.arange(n_groups), sizes))
    n = len(which)
    labels = np.arange(n_groups) if labels is None else labels
    cols = {"frame": rng.integers(0, 40000, n).astype(np.uint32),
            "x": (rng.uniform(0, 256, n_groups)[which] + rng.normal(0, 0.02, n)).astype(np.float32),
            "y": (rng.uniform(0, 256, n_groups)[which] + rng.normal(0, 0.02, n)).astype(np.float32),
            "photons": (rng.uniform(200, 90000, n) * 10.0 ** rng.integers(-2, 3, n)).astype(np.float32),
            "lpx": rng.uniform(0.002, 0.08, n),                         # float64
            "group": labels[which].astype(np.int32),
            "len": rng.integers(1, 40, n).astype(np.int32), "n": rng.integers(1, 40, n).astype(np.int32),
            "dark": np.where(rng.uniform(0, 1, n) < 0.15, -1, rng.integers(1, 9000, n)).astype(np.int32),
            "ok": rng.uniform(0, 1, n) < 0.4}
    first = np.unique(which, return_index=True)[1]
    cols["dark"][first] = np.abs(cols["dark"][first]) + 1               # every group keeps a row
    return cols


def props_cases():
    rng = np.random.default_rng(20261019)
    cases = {}
    cases["groups300"] = props_table(rng, 300, 6, np.arange(300) * 3 - 20)
    cols = props_table(rng, 12, 40, np.array([-7, 0, 1, 2, 5, 9, 40, 41, 300, 301, 9000, 70000]))
    g = cols["group"]
    lone = np.flatnonzero((g == 5) & (cols["dark"] != -1))
    cols["dark"][lone[1:]] = -1                                         # one row of group 5 survives the filter
    at = np.flatnonzero((g == 9) & (cols["dark"] != -1))
    cols["photons"][at[:2]] = np.nan
    cols["photons"][g == 40] = np.nan                                   # all NaN in one group
    cols["x"][np.flatnonzero(g == 41)[0]] = np.inf
    cols["y"][np.flatnonzero(g == 41)[:2]] = [np.inf, -np.inf]
    cols["lpx"][np.flatnonzero(g == 300)[0]] = -np.inf
    cols["lpx"][np.flatnonzero(g == 301)[0]] = np.nan
    cases["edges"] = cols
    cases["one_large_group"] = {c: v for c, v in props_table(rng, 1, 900).items()}
    return cases


def outcome(fn):
    try:
        res = fn()
        if isinstance(res, pd.DataFrame):
            return {"returns": list(res.columns), "rows": len(res), "dtypes": [str(res[c].dtype) for c in res.columns]}
        return {"returns": str(res.dtype), "rows": len(res)}
    except Exception as e:  # noqa: BLE001
        return {"raises": type(e).__name__, "message": str(e)}


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def main():
    assert not (np.uint64(2 ** 64 - 5) < np.int64(7)) and np.uint64(2 ** 64 - 5) > 0
    ref = load_reference()
    out = {"versions": np.array(json.dumps({"pandas": pd.__version__, "numpy": np.__version__, "scipy": scipy.__version__}))}

    dark = dark_cases()
    out["dark_case_names"] = np.array(list(dark))
    for name, (cols, group) in dark.items():
        assert len(cols["frame"]) <= 2000
        p = "dark/" + name + "/"
        out[p + "in_columns"] = np.array(list(cols))
        for c, v in cols.items():
            out[p + "in_" + c] = v
        if group is not None:
            out[p + "arg_group"] = group
        locs = pd.DataFrame(cols)
        res = ref["dark_times"](locs, group)
        out[p + "dark"] = res
        direct = ref["_dark_times"](cols["frame"], np.zeros(len(res)) if group is None and "group" not in cols else
                                    (cols["group"] if group is None else group), rs.last_frames(cols["frame"], cols["len"]))
        assert same(direct, res)
        table = ref["compute_dark_times"](locs, group)
        assert same(locs["dark"].to_numpy(), np.int32(res)) and len(locs) == len(res)      # written into the caller's frame
        out[p + "cdt_columns"] = np.array(list(table.columns))
        out[p + "cdt_index"] = table.index.to_numpy()
        for c in table.columns:
            out[p + "cdt_" + c] = table[c].to_numpy()
        again = rs.dark_times(cols, group)
        print(f"dark  {name:26s} rows={len(res):5d} dtype={res.dtype} -1: {int((res == -1).sum()):4d} kept={len(table)}")
        assert same(again, res), (name, np.flatnonzero(again != res)[:10])

    props = props_cases()
    out["props_case_names"] = np.array(list(props))
    for name, cols in props.items():
        assert len(cols["frame"]) <= 2000
        p = "props/" + name + "/"
        out[p + "in_columns"] = np.array(list(cols))
        for c, v in cols.items():
            out[p + "in_" + c] = v
        seen = []
        res = ref["groupprops"](pd.DataFrame(cols), callback=seen.append)
        assert seen == list(range(len(res) + 1))
        assert isinstance(res.index, pd.RangeIndex) and res.index.start == 0 and res.index.step == 1
        out[p + "columns"] = np.array(list(res.columns))
        out[p + "dtypes"] = np.array([str(res[c].dtype) for c in res.columns])
        for c in res.columns:
            out[p + "out_" + c] = res[c].to_numpy()
        again = rs.groupprops(cols)
        assert list(again) == list(res.columns), name
        off = {c: int((again[c].view(np.uint32) != res[c].to_numpy().view(np.uint32)).sum()) for c in again
               if not same(again[c], res[c].to_numpy())}
        print(f"props {name:26s} rows={len(cols['frame']):5d} groups={len(res):4d} restatement differs in", off)
        assert not off, (name, off)

    # ---- each situation occurs --------------------------------------------------------------------------------
    d = {k: out["dark/" + k + "/dark"] for k in dark}
    assert len(d["one_row"]) == 1 and d["one_row"][0] == -1
    assert (d["singles_300"] == -1).all() and len(d["singles_300"]) == 300
    assert "group" not in dark["one_group_300"][0] and (d["one_group_300"] == -1).sum() >= 1 and (d["one_group_300"] > 0).sum() > 250
    assert not same(d["sites_column"], d["sites_split_i64"]) and same(d["sites_split_i64"], d["sites_split_f64"])
    assert dark["sites_split_f64"][1].dtype == np.float64 and dark["sites_split_i64"][1].dtype == np.int64
    assert dark["sites_i32_arg_no_column"][1].dtype == np.int32 and dark["sites_i32_arg_no_column"][1].min() < 0
    assert same(d["sites_i32_arg_no_column"], d["sites_column"])
    assert d["edges_u32"].dtype == np.int64 and d["edges_i64"].dtype == np.int64 and d["edges_i32_unsorted"].dtype == np.int32
    assert (np.diff(dark["edges_i32_unsorted"][0]["frame"].astype(np.int64)) < 0).any()
    for k in ("edges_u32", "edges_i64"):
        cols = dark[k][0]
        g, f, ln = cols["group"], cols["frame"].astype(np.int64), cols["len"].astype(np.int64)
        at = lambda grp, fr: int(np.flatnonzero((g == grp) & (f == fr))[0])  # noqa: E731
        assert g.min() < 0 and (np.diff(np.unique(g)) > 1).any()
        assert d[k][at(-4, 100)] == 1 and d[k][at(0, 100)] == 10                       # the row itself is stepped over
        assert d[k][at(3, 20)] == -1 and d[k][at(3, 10)] == -1 and d[k][at(3, 30)] == 1 and d[k][at(3, 61)] == 2  # overlap
        assert d[k][at(7, 11)] == 1 and d[k][at(7, 30)] == 19                           # equal last frames
        assert d[k][at(12, 5000)] == -1 and d[k][at(500, 5000)] == -1                   # max_frame, twice
        assert d[k][at(9, 77)] == -1 and (ln == 0).sum() == 5
    assert rs.last_frames(dark["edges_u32"][0]["frame"], dark["edges_u32"][0]["len"]).max() == 2 ** 32 - 1      # 0 + 0 - 1 wraps
    assert d["edges_u32"][int(np.flatnonzero((dark["edges_u32"][0]["group"] == 501) & (dark["edges_u32"][0]["frame"] == 7))[0])] == -1
    assert d["edges_i64"][int(np.flatnonzero((dark["edges_i64"][0]["group"] == 501) & (dark["edges_i64"][0]["frame"] == 7))[0])] == 8

    e = {c: out["props/edges/out_" + c] for c in [str(c) for c in out["props/edges/columns"]]}
    g = list(e["group"])
    assert g == sorted(g) and g[0] < 0 and (np.diff(g) > 1).any()
    one = g.index(5)
    assert e["n_events"][one] == 1 and np.isnan(e["x_std"][one]) and np.isfinite(e["x_mean"][one])
    assert np.isfinite(e["photons_mean"][g.index(9)]) and np.isnan(props["edges"]["photons"]).sum() > 2
    assert np.isnan(e["photons_mean"][g.index(40)]) and np.isnan(e["photons_std"][g.index(40)])
    assert np.isinf(e["x_mean"][g.index(41)]) and np.isnan(e["y_mean"][g.index(41)]) and np.isnan(e["x_std"][g.index(41)])
    assert np.isinf(e["lpx_mean"][g.index(300)]) and np.isfinite(e["lpx_mean"][g.index(301)])
    cols = props["edges"]
    assert cols["lpx"].dtype == np.float64 and cols["frame"].dtype == np.uint32 and cols["ok"].dtype == bool
    assert all(cols[c].dtype == np.int32 for c in ("len", "n", "dark", "group"))
    assert (cols["dark"] == -1).sum() > 10 and (np.diff(cols["group"]) != 0).mean() > 0.8
    assert e["dark_mean"].min() > 0 and "qpaint_idx" in e and "ok_mean" in e and "group_std" in e
    assert len(out["props/groups300/out_group"]) == 300 and out["props/groups300/out_group"].min() < 0
    assert list(out["props/edges/columns"][:4]) == ["group", "n_events", "frame_mean", "frame_std"]

    # ---- what happens before any arithmetic -------------------------------------------------------------------
    sites = dark["sites_column"][0]
    no_dark = {c: v for c, v in props["edges"].items() if c != "dark"}
    edges = {
        "cdt without len": outcome(lambda: ref["compute_dark_times"](pd.DataFrame({c: v for c, v in sites.items() if c != "len"}))),
        "dark_times empty": outcome(lambda: ref["dark_times"](pd.DataFrame({c: v[:0] for c, v in sites.items()}))),
        "cdt empty": outcome(lambda: ref["compute_dark_times"](pd.DataFrame({c: v[:0] for c, v in sites.items()}))),
        "groupprops without dark": outcome(lambda: ref["groupprops"](pd.DataFrame(no_dark))),
        "groupprops empty": outcome(lambda: ref["groupprops"](pd.DataFrame({c: v[:0] for c, v in props["edges"].items()}))),
        "groupprops all filtered": outcome(lambda: ref["groupprops"](pd.DataFrame({**props["edges"], "dark": np.full(len(cols["dark"]), -1, np.int32)}))),
    }
    print("edges", json.dumps({k: {a: b for a, b in v.items() if a != "dtypes"} for k, v in edges.items()}))
    out["edges"] = np.array(json.dumps(edges))
    path = os.path.join(HERE, "kinetics_cases.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 512 * 1024


if __name__ == "__main__":
    main()
