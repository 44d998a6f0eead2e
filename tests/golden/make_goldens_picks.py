#!/usr/bin/env python3
"""Mint tests/golden/picks_cases.npz: the reference's own ``picked_locs``, ``remove_locs_in_picks`` and point-in-shape
helpers on small tables.

TEST INFRASTRUCTURE, build container only (needs the reference tree and pandas; no numba).  The functions are compiled
from where they lie in the reference's ``postprocess.py`` and ``lib.py`` (the function-picking loader of
make_goldens_areas.py); the jitted ones get numba's typing from tests/golden/_nbemu.py (``_Retype`` / ``binop``), their
comparisons the same array rule (``nb_compare``: _nbemu leaves comparisons to NumPy, which differs for float32[:] < int64), and
``_get_block_locs_at_numba`` gets its ``indices`` seeded with an empty array, which is what numba makes of a variable
that no path assigned (pure Python raises UnboundLocalError there).  Nothing of the reference is stored but inputs and
results.

Per case: ``in_columns`` / ``in_<column>`` / ``in_index`` (the table), ``call`` (JSON: shape, pick_size, add_group, info
and the picks, each number tagged with its type: "i" int, "f" Python float, "d" np.float64), and either ``raises`` or,
per returned frame k, ``out<k>_columns`` / ``out<k>_dtypes`` / ``out<k>_index`` and ``out<k>_<column>`` for the columns
the call added (the others are asserted to be the table's rows of that index, and are rebuilt from it); ``removed_index``
is the index of the table after ``remove_locs_in_picks`` (``removed_raises`` when it raises).  ``lib`` holds the helper
results, ``signatures`` the recorded signatures.  The script asserts that the restatement (_picks_restate.py) reproduces
the members, their order and their index for every case, that no division by zero happened, and that each situation the
cases are there for occurs.

Run:  python tests/golden/make_goldens_picks.py
"""
import ast
import inspect
import json
import os
import sys
import types
import warnings
from threading import Thread

import numpy as np
import pandas as pd

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _nbemu  # noqa: E402
import _picks_restate as rs  # noqa: E402

REF = os.environ.get("PICASSO_REFERENCE", "/root/reference")
POSTPROCESS_PY = os.path.join(REF, "picasso", "postprocess.py")
LIB_PY = os.path.join(REF, "picasso", "lib.py")
LIB_NAMES = ("get_from_metadata", "ensure_sanity", "is_loc_at", "locs_at", "check_if_in_polygon", "locs_in_polygon",
             "check_if_in_rectangle", "locs_in_rectangle", "get_pick_polygon_corners", "get_pick_rectangle_corners")
PP_NAMES = ("get_index_blocks", "_index_blocks_shape", "_fill_index_blocks", "_fill_index_block", "_picked_circular_locs",
            "_picked_rectangular_locs", "_picked_polygonal_locs", "_picked_square_locs", "picked_locs",
            "remove_locs_in_picks", "_get_block_locs_at_numba", "_locs_at_numba")
PUBLIC_PP = ("picked_locs", "_picked_circular_locs", "_picked_rectangular_locs", "_picked_polygonal_locs",
             "_picked_square_locs", "remove_locs_in_picks")
PUBLIC_LIB = ("is_loc_at", "locs_at", "check_if_in_polygon", "check_if_in_rectangle", "locs_in_polygon",
              "locs_in_rectangle", "get_pick_polygon_corners", "get_pick_rectangle_corners")
W = H = 32
INFO = [{"Width": W, "Height": H, "Frames": 50, "Pixelsize": 130}]


_COMPARE = {"Lt": np.less, "LtE": np.less_equal, "Gt": np.greater, "GtE": np.greater_equal, "Eq": np.equal, "NotEq": np.not_equal}


def nb_compare(name, a, b):
    """``array (cmp) scalar`` under numba: the comparison ufunc's loop is matched like an arithmetic one (_nbemu's
    array rule: an integer meeting a float array is cast to the array's float type), so ``float32[:] < int64`` compares
    in float32 where NumPy 2 compares in float64.  Scalars compare natively."""
    a, b = _nbemu._lift(a), _nbemu._lift(b)
    if any(isinstance(v, np.ndarray) and v.ndim > 0 for v in (a, b)):
        dt = _nbemu._array_dtype(a, b)
        return _COMPARE[name](np.asarray(a, dtype=dt), np.asarray(b, dtype=dt))
    return _COMPARE[name](a, b)


class _RetypeCompares(_nbemu._Retype):
    """_nbemu's retyping of arithmetic, and the single comparisons of the jitted functions as well."""

    def visit_Compare(self, node):
        self.generic_visit(node)
        if not self.depth or len(node.ops) != 1 or type(node.ops[0]).__name__ not in _COMPARE:
            return node
        call = ast.Call(func=ast.Name(id="__nb_compare__", ctx=ast.Load()),
                        args=[ast.Constant(value=type(node.ops[0]).__name__), node.left, node.comparators[0]], keywords=[])
        return ast.copy_location(call, node)


def _compile(path, names, ns, seed=()):
    tree = ast.parse(open(path).read())
    keep = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in names]
    assert sorted(n.name for n in keep) == sorted(names), [n.name for n in keep]
    retype = _RetypeCompares()
    keep = [retype.visit(n) for n in keep]
    for n in keep:
        if n.name in seed:
            n.body.insert(0, ast.parse("indices = np.zeros(0, np.uint32)").body[0])
    mod = ast.Module(body=[ast.ImportFrom("__future__", [ast.alias("annotations")], 0)] + keep, type_ignores=[])
    ns["__nb_binop__"], ns["__nb_compare__"] = _nbemu.binop, nb_compare
    exec(compile(ast.fix_missing_locations(mod), path, "exec"), ns)
    return ns, retype.rewritten


def load_reference():
    numba = types.SimpleNamespace(jit=lambda *a, **k: (a[0] if len(a) == 1 and callable(a[0]) and not k else (lambda fn: fn)))
    lib_ns, jitted_lib = _compile(LIB_PY, LIB_NAMES, {"np": np, "pd": pd, "numba": numba})
    assert sorted(jitted_lib) == ["check_if_in_polygon", "check_if_in_rectangle"], jitted_lib
    lib = types.SimpleNamespace(**{n: lib_ns[n] for n in LIB_NAMES})
    ns = {"np": np, "pd": pd, "numba": numba, "lib": lib, "Thread": Thread, "tqdm": lambda it, **k: it}
    pp, jitted = _compile(POSTPROCESS_PY, PP_NAMES, ns, seed=("_get_block_locs_at_numba",))
    assert sorted(jitted) == ["_fill_index_block", "_fill_index_blocks", "_get_block_locs_at_numba", "_locs_at_numba"], jitted
    return pp, lib_ns


# ---- picks with typed numbers -----------------------------------------------------------------------------------
def tag(v):
    if isinstance(v, (list, tuple)):
        return [tag(u) for u in v]
    if isinstance(v, np.float64):
        return ["d", float(v).hex()]
    if isinstance(v, float):
        return ["f", v.hex()]
    assert type(v) is int, type(v)
    return ["i", v]


def untag(t):
    if t and isinstance(t[0], str):
        return {"d": lambda s: np.float64(float.fromhex(s)), "f": float.fromhex, "i": int}[t[0]](t[1])
    return tuple(untag(u) for u in t)


def unpack_call(text):
    call = json.loads(text)
    picks = [list(untag(p)) if call["shape"] == "Polygon" else untag(p) for p in call["picks"]]
    size = None if call["size"] is None else untag(call["size"])
    return call["shape"], picks, size, call["add_group"], call["info"]


# ---- tables -------------------------------------------------------------------------------------------------------
def table(rng, x, y, dtype=np.float32, y_dtype=None, frames=50):
    n = len(x)
    return {"frame": np.sort(rng.integers(0, frames, n)).astype(np.uint32), "x": np.asarray(x).astype(dtype),
            "y": np.asarray(y).astype(y_dtype or dtype), "photons": rng.uniform(100, 5000, n).astype(np.float32),
            "lpx": rng.uniform(0.005, 0.05, n).astype(np.float32), "lpy": rng.uniform(0.005, 0.05, n).astype(np.float32)}


def cloud(rng, n, lo=0.0, hi=W):
    return rng.uniform(lo, hi, n), rng.uniform(lo, hi, n)


def ulps(v, k, dtype):
    v = dtype(v)
    for _ in range(abs(k)):
        v = np.nextafter(v, dtype(np.inf if k > 0 else -np.inf))
    return v


def cases():
    """name -> (columns, index or None, shape, picks, pick_size, add_group, info)"""
    rng = np.random.default_rng(20261020)
    c = {}
    x, y = cloud(rng, 3000)
    x[:2], y[:2] = [31.7, 0.2], [31.8, 0.1]          # a row in the last block row and column, one beside the origin
    base = table(rng, x, y)
    shuffled = rng.permutation(len(x)) * 3 + 7
    # circles: empty pick, overlap, truncation toward zero, last block, outside the grid, scalar types, shuffled index
    c["circle_basic"] = (base, shuffled, "Circle", [(5.0, 5.0), (5.3, 5.2), (-0.4, -0.3), (31.9, 31.9), (40.0, 3.0), (3.0, -7.0),
                                                   (16, 16), (np.float64(16.0), np.float64(16.0)), (16, 16.0), (100.5, 100.5)], 0.8, True, INFO)
    c["circle_int_radius"] = (base, None, "Circle", [(5, 5), (5.0, 5), (np.float64(9.5), 9)], 2, True, INFO)
    c["circle_no_group"] = (base, None, "Circle", [(7.0, 9.0), (7.5, 9.0)], 1.0, False, INFO)
    c["circle_f64"] = (table(rng, x, y, np.float64), None, "Circle", [(5.0, 5.0), (16, 16), (np.float64(20.0), 3)], 0.8, True, INFO)
    c["circle_mixed_columns"] = (table(rng, x, y, np.float32, np.float64), None, "Circle", [(5.0, 5.0), (16, 16)], 0.8, True, INFO)
    # an empty pick among rows: the nine blocks hold rows, none within the radius
    xs, ys = np.r_[x[:200], 10.9, 9.1], np.r_[y[:200], 10.9, 9.1]
    far = (np.abs(xs - 10) > 0.5) | (np.abs(ys - 10) > 0.5)
    c["circle_no_rows"] = (table(rng, xs[far], ys[far]), None, "Circle", [(10.0, 10.0), (200.0, 200.0)], 0.3, True, INFO)
    # a row at x == Width - eps whose block index falls outside the grid: it and everything sorted behind it is in no block
    edge = np.nextafter(np.float32(W), np.float32(0))
    r = next(v for v in (0.16, 0.32, 0.64, 1.28) if np.uint32(np.array([edge]) / v)[0] >= int(np.ceil(W / v)))
    xs, ys = np.r_[x[:400] % 4, edge, 2.0, 2.05, 3.0, 3.02], np.r_[y[:400] % 4, 2.0, 2.0, 2.02, 3.5, 3.52]
    c["circle_stall"] = (table(rng, xs, ys), None, "Circle", [(2.0, 2.0), (3.0, 3.5), (31.95, 2.0), (1.0, 1.0)], r, True, INFO)
    # wave and workgroup seams: the nine blocks of a pick hold exactly 63 .. 257 rows
    picks, xs, ys = [], [], []
    for k, m in enumerate((63, 64, 65, 255, 256, 257)):
        cx, cy = 4.0 + 4 * k, 4.0 + 3 * k
        picks.append((cx + 0.5, cy + 0.5))
        xs.append(rng.uniform(cx - 0.99, cx + 1.99, m))
        ys.append(rng.uniform(cy - 0.99, cy + 1.99, m))
    order = rng.permutation(sum(len(v) for v in xs))
    c["circle_seams"] = (table(rng, np.concatenate(xs)[order], np.concatenate(ys)[order]), None, "Circle", picks, 1.0, True, INFO)
    # d == r exactly, one ulp inside and outside, float32 and float64 columns, Python float / np.float64 / int picks
    for name, dt in (("f32", np.float32), ("f64", np.float64)):
        xs = [dt(8.0) + dt(0.5), ulps(8.5, -1, dt), ulps(8.5, 1, dt), dt(8.0), dt(8.3), dt(8.4), ulps(8.3, 1, dt), ulps(8.4, -1, dt)]
        ys = [dt(8.0), dt(8.0), dt(8.0), ulps(7.5, 1, dt), dt(8.4), dt(8.3), dt(8.4), dt(8.3)]
        bx, by = cloud(rng, 300, 7, 9)
        t = table(rng, np.r_[np.array(xs, dt), bx.astype(dt)], np.r_[np.array(ys, dt), by.astype(dt)], dt, frames=4)
        c["circle_edge_" + name] = (t, None, "Circle", [(8.0, 8.0), (np.float64(8.0), np.float64(8.0)), (8, 8), (8, 8.0)], 0.5, True, INFO)
    # NaN / inf rows: ensure_sanity drops them for circles only; many rows share a frame (tie order after the quicksort)
    t = table(rng, x[:600] % 8, y[:600] % 8, frames=3)
    t["x"][[5, 50]] = [np.nan, np.inf]
    t["lpx"][[7, 70]] = [np.nan, np.inf]
    t["y"][90] = -np.inf
    t["photons"][11] = -1.0
    for shape, picks, size in (("Circle", [(4.0, 4.0), (4.5, 4.2), (1, 1)], 1.5), ("Square", [(4.0, 4.0), (4.5, 4.2), (1, 1)], 3.0),
                               ("Rectangle", [((1.0, 1.0), (6.0, 5.0)), ((2.0, 6.0), (6.0, 2.0))], 2.0),
                               ("Polygon", [[(1.0, 1.0), (7.0, 1.5), (4.0, 7.0), (1.0, 1.0)]], None)):
        c["nonfinite_ties_" + shape.lower()] = (t, shuffled[:600], shape, picks, size, True, INFO)
    # squares: types of the bounds, rows exactly on the box, overlap, empty
    t = table(rng, np.r_[x[:800] % 10, 3.0, 5.0, 4.0, 4.0, np.float32(3.2), np.float32(4.8)], np.r_[y[:800] % 10, 4.0, 4.0, 3.0, 5.0, 4.0, 4.0])
    c["square_basic"] = (t, None, "Square", [(4.0, 4.0), (np.float64(4.0), np.float64(4.0)), (4, 4), (4.0, np.float64(4.0)), (4.6, 4.4),
                                           (50.0, 50.0), (4.1, 4.1)], 2.0, True, INFO)
    c["square_bounds_f32"] = (t, None, "Square", [(4.0, 4.0), (np.float64(4.0), np.float64(4.0))], 1.6, True, INFO)      # float32(3.2) > 3.2: the row at float32(3.2) is inside only for a float64 bound
    c["square_f64_no_group"] = (table(rng, t["x"], t["y"], np.float64), None, "Square", [(4.0, 4.0), (4, 4), (4.6, 4.4)], 2, False, INFO)
    # rectangles: vertical, horizontal, tilted, rows on a side and on the box, zero width
    t = table(rng, np.r_[x[:1500] % 12, 2.0, 3.0, 2.5, 2.5, 4.0, 6.0], np.r_[y[:1500] % 12, 5.0, 5.0, 2.0, 8.0, 4.0, 6.0])
    rects = [((2.5, 2.0), (2.5, 8.0)), ((2.0, 5.0), (9.0, 5.0)), ((2.0, 2.0), (8.0, 8.0)), ((8.0, 3.0), (3.0, 9.5)),
             ((np.float64(3.0), np.float64(3.0)), (np.float64(7.0), np.float64(4.0))), ((2, 2), (9, 3)), ((20.0, 20.0), (25.0, 21.0))]
    c["rectangle_basic"] = (t, shuffled[:len(t["x"])], "Rectangle", rects, 1.0, True, INFO)
    c["rectangle_f64_no_group"] = (table(rng, t["x"], t["y"], np.float64), None, "Rectangle", rects[:4], 2, False, INFO)
    c["rectangle_zero_width"] = (t, None, "Rectangle", rects[:3], 0.0, True, INFO)
    # polygons: triangle, concave, horizontal edge at a row's y, unclosed between closed ones, 200 corners, int corners
    ang = np.linspace(0, 2 * np.pi, 200)[:-1]
    big = [(float(6 + 4 * np.cos(a) * (1 + 0.3 * np.sin(7 * a))), float(6 + 4 * np.sin(a) * (1 + 0.3 * np.sin(7 * a)))) for a in ang]
    big.append(big[0])
    assert len(big) == 200
    t = table(rng, np.r_[x[:2000] % 12, 3.0, 5.0, 7.0], np.r_[y[:2000] % 12, 4.0, 4.0, 4.0])
    polys = [[(1.0, 1.0), (5.0, 1.5), (3.0, 6.0), (1.0, 1.0)],
             [(1.0, 1.0), (9.0, 1.0), (9.0, 9.0), (5.0, 3.0), (1.0, 9.0), (1.0, 1.0)],
             [(2.0, 2.0), (5.0, 5.0), (8.0, 2.0)],
             [(2.0, 4.0), (8.0, 4.0), (8.0, 8.0), (2.0, 8.0), (2.0, 4.0)],
             big,
             [(2, 2), (10, 3), (6, 11), (2, 2)],
             [(np.float64(2.5), np.float64(2.5)), (np.float64(9.5), np.float64(3.5)), (np.float64(5.5), np.float64(10.5)), (np.float64(2.5), np.float64(2.5))],
             [(1.0, 1.0), (2.0, 2.0)],
             [(20.0, 20.0), (22.0, 20.0), (21.0, 23.0), (20.0, 20.0)]]
    c["polygon_basic"] = (t, shuffled[:len(t["x"])], "Polygon", polys, None, True, INFO)
    c["polygon_f64_no_group"] = (table(rng, t["x"], t["y"], np.float64), None, "Polygon", polys[:4], None, False, INFO)
    # empty tables: the golden records whatever the reference does
    empty = {k: v[:0] for k, v in base.items()}
    c["empty_circle"] = (empty, None, "Circle", [(5.0, 5.0)], 1.0, True, INFO)
    c["empty_square"] = (empty, None, "Square", [(5.0, 5.0)], 1.0, True, INFO)
    c["empty_rectangle"] = (empty, None, "Rectangle", [((1.0, 1.0), (6.0, 5.0))], 1.0, True, INFO)
    c["empty_polygon"] = (empty, None, "Polygon", [polys[0]], None, True, INFO)
    # the arithmetic types: float32 rows on the rim of a circle, found by search, on which the typings disagree
    rng = np.random.default_rng(20261021)
    xs, ys, _ = rim_rows(rng, 8.0, 0.8, rs.radius_squared(0.8), TYPING_FLAGS)
    bx, by = cloud(rng, 200, 7, 9)
    c["circle_typing"] = (table(rng, np.r_[xs, bx.astype(np.float32)], np.r_[ys, by.astype(np.float32)], frames=5), None, "Circle",
                          [(8, 8), (8.0, 8.0), (np.float64(8.0), np.float64(8.0)), (8, 8.0), (8.0, 8)], 0.8, True, INFO)
    # ... and an integer radius whose square is no float32: float32[:] < int64 compares with float32(r ** 2)
    xs, ys, _ = rim_rows(rng, 5000.0, 4097.0, rs.radius_squared(4097), (7, 3, 0))
    bx, by = cloud(rng, 100, 900, 9100)
    c["circle_typing_int_radius"] = (table(rng, np.r_[xs, bx.astype(np.float32)], np.r_[ys, by.astype(np.float32)], frames=5), None,
                                     "Circle", [(5000, 5000), (5000.0, 5000.0), (5000, 5000.0)], 4097, True, WIDE_INFO)
    return c


TYPING_FLAGS = (0, 1, 2, 3, 7)         # the typings a call can ask for at float32 columns (bit 2 acts with bits 0 and 1 set)
WIDE_INFO = [{"Width": 16384, "Height": 16384, "Frames": 50, "Pixelsize": 130}]


def rim_rows(rng, centre, r, r2, flag_values, per_pattern=6):
    """float32 points within a few ulps of the circle of radius r around (centre, centre) on which the evaluations of
    dx ** 2 + dy ** 2 < r2 under `flag_values` do not all agree: up to `per_pattern` per pattern of answers, such that
    every two of the typings are told apart by some row."""
    theta = rng.uniform(0, 2 * np.pi, 400000)
    rho = r * (1 + rng.uniform(-3e-7, 3e-7, len(theta)))
    x, y = (centre + rho * np.cos(theta)).astype(np.float32), (centre + rho * np.sin(theta)).astype(np.float32)
    answers = np.array([rs.circle_mask(x, y, centre, centre, r2, f) for f in flag_values])
    pattern = (answers * (1 << np.arange(len(flag_values)))[:, None]).sum(axis=0)
    mixed = np.flatnonzero((pattern != 0) & (pattern != (1 << len(flag_values)) - 1))
    keep = np.concatenate([mixed[pattern[mixed] == v][:per_pattern] for v in np.unique(pattern[mixed])])
    for i in range(len(flag_values)):
        for j in range(i):
            assert (answers[i, keep] != answers[j, keep]).any(), (flag_values[i], flag_values[j])
    return x[keep], y[keep], answers[:, keep]


def frame(cols, index):
    df = pd.DataFrame({k: v.copy() for k, v in cols.items()})
    if index is not None:
        df.index = pd.Index(np.asarray(index, np.int64))
    return df


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def expected_frames(df, cols, shape, picks, size, add_group, info):
    """The frames the restatement gives: its members in pre-sort order, then pandas' own quicksort by frame."""
    kept, offsets, rows = rs.members(cols, info, picks, shape, size)
    out = []
    for k, i in enumerate(kept):
        sub = df.iloc[rows[offsets[k]:offsets[k + 1]]]
        order = sub["frame"].to_numpy().argsort(kind="quicksort")
        out.append((i, sub.index.to_numpy()[order]))
    return out


def mint(ref, name, case, out):
    cols, index, shape, picks, size, add_group, info = case
    p = name + "/"
    out[p + "in_columns"] = np.array(list(cols))
    for k, v in cols.items():
        out[p + "in_" + k] = v
    out[p + "in_index"] = np.zeros(0, np.int64) if index is None else np.asarray(index, np.int64)
    out[p + "has_index"] = np.array(index is not None)
    out[p + "call"] = np.array(json.dumps({"shape": shape, "size": None if size is None else tag(size), "add_group": add_group,
                                          "info": info, "picks": tag(picks)}))
    df = frame(cols, index)
    before = df.copy()
    seen = []
    _nbemu.ZERO_DIVISIONS[0] = 0
    try:
        res = ref["picked_locs"](df, info, picks, shape, size, add_group, None, seen.append)
    except Exception as e:  # noqa: BLE001
        out[p + "raises"] = np.array(type(e).__name__)
        print(f"{name:28s} raises {type(e).__name__}: {e}")
        res = None
    assert _nbemu.ZERO_DIVISIONS[0] == 0, name
    assert df.equals(before) and df.index.equals(before.index)
    if res is not None:
        assert seen == list(range(1, len(picks) + 1)), (name, seen)
        want = expected_frames(df, cols, shape, picks, size, add_group, info)
        assert len(want) == len(res), name
        out[p + "n_out"] = np.array(len(res))
        for k, (got, (i, idx)) in enumerate(zip(res, want)):
            assert same(got.index.to_numpy(), idx), (name, k, got.index.to_numpy()[:10], idx[:10])
            assert ("group" in got.columns) == add_group and (not add_group or (got["group"] == i).all()), (name, k)
            q = f"{p}out{k}_"
            out[q + "columns"] = np.array(list(got.columns))
            out[q + "dtypes"] = np.array([str(got[col].dtype) for col in got.columns])
            out[q + "index"] = got.index.to_numpy()
            assert got[list(cols)].equals(df.loc[got.index]), (name, k)          # copies of the member rows
            for col in got.columns:
                if col not in cols:
                    out[q + col] = got[col].to_numpy()
        print(f"{name:28s} rows={len(df):5d} picks={len(picks):3d} members {[len(r) for r in res]}")
    # remove_locs_in_picks: the size is a diameter for circles
    df = frame(cols, index)
    rsize = size * 2 if shape == "Circle" else size
    try:
        got = ref["remove_locs_in_picks"](df, info, picks=picks, pick_shape=shape, pick_size=rsize)
        assert got is df
        out[p + "removed_index"] = got.index.to_numpy()
    except Exception as e:  # noqa: BLE001
        out[p + "removed_raises"] = np.array(type(e).__name__)
        print(f"{name:28s} remove raises {type(e).__name__}: {e}")
    if "removed_index" in "".join(k[len(p):] for k in out if k.startswith(p)):
        # the reference halves the diameter itself: an integer diameter becomes a float radius
        kept, offsets, rows = rs.members(cols, info, picks, shape, rsize / 2 if shape == "Circle" else size)
        assert same(np.delete(before.index.to_numpy(), np.unique(rows)), out[p + "removed_index"]), name
    out[p + "remove_size"] = np.array(json.dumps(None if rsize is None else tag(rsize)))


def lib_cases(ref_lib, all_cases, out):
    """The helpers on one table: is_loc_at / locs_at with each scalar type, the two shape tests with their own corners."""
    cols, index = all_cases["circle_typing"][0], None
    df = frame(cols, index)
    # pandas' typing: arithmetic unwraps a NumPy scalar into a Python one, so the differences, squares and the sum of
    # float32 columns stay float32 whatever x and y are; the comparison does not unwrap, so a Python r ** 2 is compared
    # as float32(r ** 2) and an np.float64 one in float64
    calls = {"py": (8.0, 8.0, 0.8), "np": (np.float64(8.0), np.float64(8.0), np.float64(0.8)), "int": (8, 8, np.float64(0.8))}
    used = {}
    for k, (x, y, r) in calls.items():
        out[f"lib/is_loc_at_{k}"] = ref_lib["is_loc_at"](x, y, df, r)
        assert same(ref_lib["locs_at"](x, y, df, r).index.to_numpy(), np.flatnonzero(out[f"lib/is_loc_at_{k}"]))
        flags = 3 | 4 * int(np.result_type(np.float32, r ** 2) == np.float32)
        assert same(rs.circle_mask(cols["x"], cols["y"], float(x), float(y), float(r ** 2), flags), out[f"lib/is_loc_at_{k}"]), k
        for other in range(8):
            if other & 3 != 3 or other == (flags ^ 4):
                assert not same(rs.circle_mask(cols["x"], cols["y"], float(x), float(y), float(r ** 2), other), out[f"lib/is_loc_at_{k}"]), (k, other)
        used[k] = flags
    assert used == {"py": 7, "np": 3, "int": 3}, used
    assert (out["lib/is_loc_at_py"] != out["lib/is_loc_at_np"]).any(), "the is_loc_at typings give one answer"
    out["lib/is_loc_at_calls"] = np.array(json.dumps({k: tag(v) for k, v in calls.items()}))
    cols = all_cases["polygon_basic"][0]
    df = frame(cols, None)
    poly = all_cases["polygon_basic"][3][1]
    X, Y = ref_lib["get_pick_polygon_corners"](poly)
    out["lib/polygon_X"], out["lib/polygon_Y"] = np.array(X), np.array(Y)
    out["lib/in_polygon"] = ref_lib["check_if_in_polygon"](cols["x"], cols["y"], np.array(X), np.array(Y))
    assert same(ref_lib["locs_in_polygon"](df, X, Y).index.to_numpy(), np.flatnonzero(out["lib/in_polygon"]))
    assert same(rs.in_polygon(cols["x"], cols["y"], X, Y), out["lib/in_polygon"])
    assert ref_lib["get_pick_polygon_corners"](all_cases["polygon_basic"][3][2]) == (None, None)
    rect = (8.0, 3.0, 3.0, 9.5, 1.5)
    X, Y = ref_lib["get_pick_rectangle_corners"](*rect)
    assert (X, Y) == rs.rectangle_corners(*rect)
    out["lib/rectangle_args"], out["lib/rectangle_X"], out["lib/rectangle_Y"] = np.array(rect), np.array(X), np.array(Y)
    _nbemu.ZERO_DIVISIONS[0] = 0
    out["lib/in_rectangle"] = ref_lib["check_if_in_rectangle"](cols["x"], cols["y"], np.array(X), np.array(Y))
    assert _nbemu.ZERO_DIVISIONS[0] == 0 and not rs.rectangle_zero_division(cols["y"], Y)
    assert same(ref_lib["locs_in_rectangle"](df, X, Y).index.to_numpy(), np.flatnonzero(out["lib/in_rectangle"]))
    assert same(rs.in_rectangle(cols["x"], cols["y"], X, Y), out["lib/in_rectangle"])
    # free corners with a flat side at a row's height: the reference divides by zero there (numba raises)
    X, Y = [2.0, 8.0, 8.0, 2.0], [4.0, 4.0, 8.0, 8.0]
    ref_lib["check_if_in_rectangle"](cols["x"], cols["y"], np.array(X), np.array(Y))
    assert _nbemu.ZERO_DIVISIONS[0] > 0 and rs.rectangle_zero_division(cols["y"], Y)
    out["lib/flat_X"], out["lib/flat_Y"] = np.array(X), np.array(Y)


def main():
    warnings.simplefilter("ignore")
    ref, ref_lib = load_reference()
    all_cases = cases()
    out = {"versions": np.array(json.dumps({"pandas": pd.__version__, "numpy": np.__version__})),
           "signatures": np.array(json.dumps({**{n: str(inspect.signature(ref[n])) for n in PUBLIC_PP},
                                              **{"lib." + n: str(inspect.signature(ref_lib[n])) for n in PUBLIC_LIB}})),
           "case_names": np.array(list(all_cases))}
    for name, case in all_cases.items():
        assert len(case[0]["x"]) <= 5000
        mint(ref, name, case, out)
    lib_cases(ref_lib, all_cases, out)
    check_situations(all_cases, out)
    path = os.path.join(HERE, "picks_cases.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 1 << 20


def check_situations(all_cases, out):
    def sizes(name):
        return [len(out[f"{name}/out{k}_index"]) for k in range(int(out[name + "/n_out"]))]

    s = sizes("circle_basic")
    assert s[0] > 0 and s[1] > 0 and s[2] > 0 and s[3] > 0 and s[4] == s[5] == s[9] == 0, s          # truncation, last block, outside
    assert len(np.intersect1d(out["circle_basic/out0_index"], out["circle_basic/out1_index"])) > 0   # shared rows
    assert sizes("circle_no_rows") == [0, 0]
    cols, _, _, picks, r, _, info = all_cases["circle_stall"]
    K, L = rs.grid_shape(info, r)
    _, _, p = rs.block_order(cols["x"], cols["y"], r, K, L)
    assert p < len(cols["x"]) and sizes("circle_stall")[2] == 0, (p, sizes("circle_stall"))
    cols, _, _, picks, r, _, info = all_cases["circle_seams"]
    order, keys, p = rs.block_order(cols["x"], cols["y"], r, *rs.grid_shape(info, r))
    held = []
    for px, py in picks:
        x_, y_ = int(px / r), int(py / r)
        held.append(sum(int(((keys >> 32 == k) & (keys & 0xffffffff == ll)).sum()) for k in range(y_ - 1, y_ + 2) for ll in range(x_ - 1, x_ + 2)))
    assert held == [63, 64, 65, 255, 256, 257], held
    # the typings: int, Python float, np.float64, (int, float), (float, int) picks at float32 columns
    m = [set(out[f"circle_typing/out{k}_index"].tolist()) for k in range(5)]
    assert m[1] == m[2] and len({frozenset(v) for v in (m[0], m[1], m[3], m[4])}) == 4, [len(v) for v in m]
    m = [set(out[f"circle_typing_int_radius/out{k}_index"].tolist()) for k in range(3)]
    assert len({frozenset(v) for v in m}) == 3, [len(v) for v in m]
    for name in ("circle_typing", "circle_typing_int_radius"):
        assert forced_flags_change_the_answer(all_cases[name]), name
    assert sizes("square_bounds_f32")[0] != sizes("square_bounds_f32")[1], sizes("square_bounds_f32")     # weak vs float64 bounds differ
    g = [int(out[f"polygon_basic/out{k}_group"][0]) for k in range(int(out["polygon_basic/n_out"])) if len(out[f"polygon_basic/out{k}_group"])]
    assert int(out["polygon_basic/n_out"]) == 7 and 3 in g and 2 not in g and 7 not in g, g
    t = all_cases["nonfinite_ties_circle"][0]
    assert max(np.bincount(t["frame"])) > 100


def forced_flags_change_the_answer(case) -> bool:
    """Does the restatement give another member set for some pick under every typing but the pick's own?  (Bit 2 only
    acts when bits 0 and 1 are set.)"""
    cols, _, _, picks, r, _, info = case

    def effective(f):
        return f if f & 3 == 3 else f & 3

    own = [effective(rs.circle_flags(px, py, r)) for px, py in picks]
    offsets, rows = rs.circle(cols, info, picks, r)
    keep = rs.circle_flags
    try:
        for forced in range(8):
            rs.circle_flags = lambda x, y, r, forced=forced: forced
            o2, r2 = rs.circle(cols, info, picks, r)
            for k in range(len(picks)):
                equal = np.array_equal(rows[offsets[k]:offsets[k + 1]], r2[o2[k]:o2[k + 1]])
                if equal != (effective(forced) == own[k]):
                    return False
    finally:
        rs.circle_flags = keep
    return True


if __name__ == "__main__":
    main()
