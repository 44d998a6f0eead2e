#!/usr/bin/env python3
"""Mint tests/golden/similar_cases.npz: the reference's own ``pick_similar`` on small tables.

TEST INFRASTRUCTURE, build container only (needs the reference tree and pandas; no numba).  ``pick_similar``,
``_pick_similar``, ``_n_block_locs_at``, ``get_block_locs_at_numba``, ``_get_block_locs_at_numba``, ``_locs_at_numba``,
``locs_at_numba``, ``rmsd_at_com``, ``get_index_blocks`` and its helpers are compiled in memory from where they lie in the
reference's ``postprocess.py`` (the loader of make_goldens_picks.py: numba's typing of arithmetic and comparisons from
tests/golden/_nbemu.py).  On top of that, inside the jitted functions:

  np.mean          is routed to numba's sequential rule (``nb_mean`` below; _similar_restate.py says what was read and
                   what was not run);
  uint64 (op) int  ``x_r[i] - 1`` with a uint64 block index is int64 under numba's integer rule (choose_result_int:
                   signed when either is, at least intp wide); _nbemu.binop uses the native operator, which gives a
                   float64 that ``range`` refuses, so mixed-sign integer scalars are cast to int64 here first;
  unassigned       ``indices`` of _get_block_locs_at_numba and ``n_block_locs`` of _n_block_locs_at are seeded with an
                   empty array and a zero, which is what numba makes of a variable that no path assigned;
  500              the shift cap of _pick_similar reads the global ``__max_shifts__`` (500 unless a case says otherwise:
                   a flat-kernel mean shift stops after finitely many moves, so 500 itself is not reachable on tables
                   this small; the cases ``max_shifts_1`` / ``max_shifts_2`` replace the constant and are named so).

Nothing of the reference is stored but inputs and results.  Per case: ``in_columns`` / ``in_<column>`` (the table),
``call`` (JSON: info, d and the picks with each number tagged "i" int, "f" Python float, "d" np.float64; std_range,
max_shifts, kind "generic" or "dyadic"), and ``out_x`` / ``out_y`` (float64, the returned pairs) or ``raises``.  A float32
table is "dyadic" when its coordinates are multiples of 1/64 (every partial sum of a circle is then exact in float32
and float64, so the case holds whatever numba's accumulator is) and "generic" otherwise (pinned under the accumulator
rule).  The script asserts that the restatement (_similar_restate.py) reproduces every result in bits, and that each
situation the cases are there for occurs.

Run:  python tests/golden/make_goldens_similar.py
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
import _picks_restate as prs  # noqa: E402
import _similar_restate as rs  # noqa: E402
import make_goldens_picks as mkp  # noqa: E402

POSTPROCESS_PY, LIB_PY = mkp.POSTPROCESS_PY, mkp.LIB_PY
LIB_NAMES = ("get_from_metadata", "ensure_sanity")
PP_NAMES = ("get_index_blocks", "_index_blocks_shape", "_fill_index_blocks", "_fill_index_block", "pick_similar",
            "_pick_similar", "_n_block_locs_at", "get_block_locs_at_numba", "_get_block_locs_at_numba", "_locs_at_numba",
            "locs_at_numba", "rmsd_at_com")
JITTED = sorted(n for n in PP_NAMES if n not in ("get_index_blocks", "_index_blocks_shape", "pick_similar"))
SEEDS = {"_get_block_locs_at_numba": "indices = np.zeros(0, np.uint32)", "_n_block_locs_at": "n_block_locs = np.uint32(0)"}
W = H = 32
INFO = [{"Width": W, "Height": H, "Frames": 50, "Pixelsize": 130}]


def nb_mean(a):
    """numba/np/arraymath.py array_mean: ``c = zero; for v in np.nditer(arr): c += v.item(); return c / arr.size`` with
    the accumulator in the array's own float type and a float64 division (a division by zero raises)."""
    a = np.asarray(a)
    assert a.ndim == 1 and a.dtype.kind == "f", (a.ndim, a.dtype)
    c = a.dtype.type(0)
    for v in a:
        c = a.dtype.type(c + v)
    if a.size == 0:
        raise ZeroDivisionError("division by zero")
    return np.float64(c) / np.float64(a.size)


def nb_binop(name, a, b):
    a2, b2 = _nbemu._lift(a), _nbemu._lift(b)
    if isinstance(a2, np.integer) and isinstance(b2, np.integer) and a2.dtype.kind != b2.dtype.kind:
        return _nbemu.binop(name, np.int64(a2), np.int64(b2))
    return _nbemu.binop(name, a, b)


class _Retype(mkp._RetypeCompares):
    """make_goldens_picks' retyping, and np.mean of the jitted functions routed to ``nb_mean``."""

    means = 0

    def visit_Call(self, node):
        self.generic_visit(node)
        f = node.func
        if self.depth and isinstance(f, ast.Attribute) and f.attr == "mean" and isinstance(f.value, ast.Name) and f.value.id == "np":
            assert len(node.args) == 1 and not node.keywords
            self.means += 1
            return ast.copy_location(ast.Call(func=ast.Name(id="__nb_mean__", ctx=ast.Load()), args=node.args, keywords=[]), node)
        return node


def _compile(path, names, ns, seeds=None, cap_in=None):
    tree = ast.parse(open(path).read())
    keep = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in names]
    assert sorted(n.name for n in keep) == sorted(names), [n.name for n in keep]
    retype = _Retype()
    keep = [retype.visit(n) for n in keep]
    for n in keep:
        if seeds and n.name in seeds:
            n.body.insert(0, ast.parse(seeds[n.name]).body[0])
        if n.name == cap_in:
            caps = [c for c in ast.walk(n) if isinstance(c, ast.Constant) and type(c.value) is int and c.value == 500]
            assert len(caps) == 1, len(caps)

            class Cap(ast.NodeTransformer):
                def visit_Constant(self, c):
                    return ast.copy_location(ast.Name(id="__max_shifts__", ctx=ast.Load()), c) if c is caps[0] else c

            Cap().visit(n)
    mod = ast.Module(body=[ast.ImportFrom("__future__", [ast.alias("annotations")], 0)] + keep, type_ignores=[])
    ns.update(__nb_binop__=nb_binop, __nb_compare__=mkp.nb_compare, __nb_mean__=nb_mean, __max_shifts__=500)
    exec(compile(ast.fix_missing_locations(mod), path, "exec"), ns)
    return ns, retype


def load_reference():
    numba = types.SimpleNamespace(jit=lambda *a, **k: (a[0] if len(a) == 1 and callable(a[0]) and not k else (lambda fn: fn)))
    lib_ns, _ = _compile(LIB_PY, LIB_NAMES, {"np": np, "pd": pd, "numba": numba})
    lib = types.SimpleNamespace(**{n: lib_ns[n] for n in LIB_NAMES})
    ns = {"np": np, "pd": pd, "numba": numba, "lib": lib, "Thread": Thread}
    pp, retype = _compile(POSTPROCESS_PY, PP_NAMES, ns, SEEDS, "_pick_similar")
    assert sorted(retype.rewritten) == JITTED, retype.rewritten
    assert retype.means == 7, retype.means          # _pick_similar: the first move and the loop, two each; rmsd_at_com: three
    return pp


# ---- tables -------------------------------------------------------------------------------------------------------
GX = np.arange(1.0, W, np.sqrt(3))                 # the grid columns at d = 2
STARVED_AT = (float(GX[4]), 21.0)                  # an even column: y_range_base holds 21
CLUSTERS = [                                       # (x, y, rows, sigma)
    (20.3, 19.6, 24, 0.25), (25.2, 8.3, 28, 0.30), (6.4, 25.3, 22, 0.22), (16.0, 26.0, 30, 0.45),      # the given picks
    (10.0, 10.2, 24, 0.20), (11.5, 10.2, 25, 0.20), (13.0, 10.2, 26, 0.20),                              # the chain A, B, C
    (27.0, 24.5, 30, 0.45), (4.6, 6.2, 25, 0.25), (17.3, 3.4, 23, 0.28), (28.5, 15.5, 26, 0.25), (12.8, 18.7, 24, 0.25),
    (22.6, 28.2, 27, 0.30), (23.4, 14.2, 60, 0.25), (3.3, 11.2, 6, 0.2)]                                  # too many, too few
PICKS = [(20.3, 19.6), (25.2, 8.3), (6.4, 25.3), (16.0, 26.0)]


def basic_xy(rng):
    xs, ys = [], []
    for cx, cy, n, s in CLUSTERS:
        xs.append(rng.normal(cx, s, n))
        ys.append(rng.normal(cy, s, n))
    # a cluster in block column 0: the circle of the grid point (1, 15) holds it, the gate does not count it
    xs.append(np.clip(rng.normal(0.5, 0.12, 30), 0.05, 0.95))
    ys.append(np.clip(rng.normal(15.0, 0.12, 30), 14.6, 15.4))
    # three rows on the rim of one grid point's circle: their mean loses two of them; and rows in a corner of its nine
    # blocks, outside every circle it takes, that let it pass the gate
    gx, gy = STARVED_AT
    xs.append(np.array([gx - 0.99, gx + 0.99, gx]))
    ys.append(np.array([gy, gy, gy - 0.99]))
    xs.append(rng.uniform(6.05, 6.5, 24))
    ys.append(rng.uniform(22.4, 22.95, 24))
    bx, by = rng.uniform(0, W, 400), rng.uniform(0, H, 400)
    far = (np.hypot(bx - gx, by - gy) > 2.6) & ~((bx < 3.2) & (np.abs(by - 15) < 2.2))
    xs.append(bx[far][:60])
    ys.append(by[far][:60])
    x, y = np.concatenate(xs), np.concatenate(ys)
    order = rng.permutation(len(x))
    return np.clip(x[order], 0.01, W - 0.01), np.clip(y[order], 0.01, H - 0.01)


PATTERN = np.array([[-20, -9], [-14, 12], [-9, -17], [-6, 3], [-3, 21], [-1, -6], [0, 9], [2, -22], [4, 1], [6, 15], [9, -11],
                    [11, 6], [14, -3], [17, 19], [20, -14], [-10, 5]]) / 64.0          # 16 rows: every mean is exact
COPIES = [(8.25, 8.5), (20.25, 8.5), (13.25, 22.5), (23.25, 25.5)]


def copies_xy(rng):
    """Translated copies of one 16-row pattern on the 1/64 lattice: equal counts and RMSDs in every bit."""
    xs, ys = [c[0] + PATTERN[:, 0] for c in COPIES], [c[1] + PATTERN[:, 1] for c in COPIES]
    for cx, cy, n in ((5.5, 18.0, 16), (27.0, 12.0, 20), (16.0, 15.0, 12)):          # same size but another shape, other sizes
        xs.append(cx + rng.integers(-24, 25, n) / 64.0)
        ys.append(cy + rng.integers(-24, 25, n) / 64.0)
    bx, by = rng.integers(64, 31 * 64, 300) / 64.0, rng.integers(64, 31 * 64, 300) / 64.0
    far = np.ones(len(bx), bool)
    for cx, cy in COPIES:
        far &= np.hypot(bx - cx, by - cy) > 2.7
    x, y = np.concatenate(xs + [bx[far][:50]]), np.concatenate(ys + [by[far][:50]])
    order = rng.permutation(len(x))
    return x[order], y[order]


def cases():
    """name -> (columns, info, picks, d, std_range, max_shifts, kind)"""
    rng = np.random.default_rng(20261020)
    x, y = basic_xy(rng)
    c = {}
    f32 = mkp.table(rng, x, y)
    c["basic_f32"] = (f32, INFO, PICKS, 2.0, 2.0, 500, "generic")
    c["basic_f64"] = (mkp.table(rng, x, y, np.float64), INFO, PICKS, 2.0, 2.0, 500, "generic")
    c["basic_mixed"] = (mkp.table(rng, x, y, np.float32, np.float64), INFO, PICKS, 2.0, 2.0, 500, "generic")
    # an integer diameter (d2 is an int, r still a float) and integer / np.float64 pick scalars beside floats
    c["basic_int_d"] = (f32, INFO, [(20, 19.6), (25.2, 8), (np.float64(6.4), 25.3), (16.0, np.float64(26.0))], 2, 2.0, 500, "generic")
    c["basic_d_1p7"] = (f32, INFO, PICKS, 1.7, 2.5, 500, "generic")
    c["max_shifts_1"] = (f32, INFO, PICKS, 2.0, 2.0, 1, "generic")
    c["max_shifts_2"] = (f32, INFO, PICKS, 2.0, 2.0, 2, "generic")
    xq, yq = np.round(x * 64) / 64, np.round(y * 64) / 64
    c["dyadic_f32"] = (mkp.table(rng, xq, yq), INFO, PICKS, 2.0, 2.0, 500, "dyadic")
    cx, cy = copies_xy(rng)
    copies = mkp.table(rng, cx, cy)
    c["single_pick"] = (copies, INFO, [(8.3, 8.4)], 2.0, 2.0, 500, "dyadic")
    c["std_range_0"] = (copies, INFO, [(8.3, 8.4), (20.2, 8.6)], 2.0, 0, 500, "dyadic")
    c["empty_picks"] = (f32, INFO, [], 2.0, 2.0, 500, "generic")
    c["pick_without_members"] = (f32, INFO, [(20.3, 19.6), (30.9, 1.1)], 2.0, 2.0, 500, "generic")
    c["one_block_column"] = (mkp.table(rng, x % 1, y), [{"Width": 1, "Height": H, "Frames": 50, "Pixelsize": 130}], [(0.5, 15.0)],
                             2.0, 2.0, 500, "generic")
    c["empty_table"] = ({k: v[:0] for k, v in f32.items()}, INFO, [], 2.0, 2.0, 500, "generic")
    return c


def unpack_call(text):
    call = json.loads(text)
    return call["info"], [mkp.untag(p) for p in call["picks"]], mkp.untag(call["d"]), mkp.untag(call["std_range"]), \
        call["max_shifts"], call["kind"]


def mint(ref, name, case, out):
    cols, info, picks, d, std_range, max_shifts, kind = case
    p = name + "/"
    out[p + "in_columns"] = np.array(list(cols))
    for k, v in cols.items():
        out[p + "in_" + k] = v
    out[p + "call"] = np.array(json.dumps({"info": info, "picks": mkp.tag(picks), "d": mkp.tag(d), "std_range": mkp.tag(std_range),
                                          "max_shifts": max_shifts, "kind": kind}))
    if kind == "dyadic":
        assert all((v * 64 == np.round(v * 64)).all() for v in (cols["x"], cols["y"])), name
    df = mkp.frame(cols, None)
    before = df.copy()
    ref["__max_shifts__"] = max_shifts
    try:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            res = ref["pick_similar"](df, info, picks, d, std_range)
    except Exception as e:  # noqa: BLE001
        out[p + "raises"] = np.array(type(e).__name__)
        print(f"{name:24s} raises {type(e).__name__}: {e}")
        res = None
    finally:
        ref["__max_shifts__"] = 500
    assert df.equals(before)
    try:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            want = rs.pick_similar(cols, info, picks, d, std_range, max_shifts)
    except Exception as e:  # noqa: BLE001
        want = type(e).__name__
    if res is None:
        assert want == str(out[p + "raises"]), (name, want)
        return
    assert isinstance(res, list) and all(isinstance(t, tuple) and len(t) == 2 for t in res), name
    gx, gy = np.array([t[0] for t in res], np.float64), np.array([t[1] for t in res], np.float64)
    assert all(type(v) is np.float64 for t in res for v in t), name
    assert not isinstance(want, str) and mkp.same(gx, want[0]) and mkp.same(gy, want[1]), (name, len(gx), len(want[0]))
    out[p + "out_x"], out[p + "out_y"] = gx, gy
    print(f"{name:24s} rows={len(df):4d} picks={len(picks)} -> {len(res)} pairs")


def check_situations(ref, all_cases, out):
    def details(name):
        cols, info, picks, d, std_range, max_shifts, _ = all_cases[name]
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            return rs.pick_similar(cols, info, picks, d, std_range, max_shifts, details=True)

    xs, ys, D = details("basic_f32")
    cols, info, picks, d = all_cases["basic_f32"][:4]
    cx, cy, n, rmsd, shifts, ended = D["shift"]
    cand, keep, who, P = D["cand"], D["keep"], D["who"], len(picks)
    accepted = cand[keep]
    assert (shifts[accepted] == 1).any() and (shifts[accepted] >= 3).any(), np.bincount(shifts[accepted])
    gx, gy = rs.grid(info, d)[:2]
    starved = int(np.flatnonzero(np.isclose(gx, STARVED_AT[0]))[0]) * len(gy) + int(np.flatnonzero(gy == STARVED_AT[1])[0])
    assert ended[starved] == rs.STARVED and n[starved] == 1, (ended[starved], n[starved])
    assert (ended == rs.STARVED).sum() >= 1
    # the gate: a point it rejects although its first circle holds >= min_n_locs rows (the cluster in block column 0)
    sane = prs.sane_rows(cols, info)
    K, L = prs.grid_shape(info, d / 2)
    open_gate = rs.shift(cols["x"][sane], cols["y"][sane], d / 2, K, L, rs.grid(info, d), (d / 2) ** 2, 0, 0)
    first = open_gate[2]                                          # max_shifts 0: the first member set
    at = 0 * len(gy) + int(np.flatnonzero(gy == 15.0)[0])       # the grid point (1, 15)
    assert ended[at] == rs.SKIPPED and first[at] >= D["bounds"][0] and n[at] == 0, (first[at], D["bounds"])
    # two grid points on one cluster: a candidate refused by an earlier kept candidate less than d / 10 away (their
    # member sets differ by a row or two, so the two centres are close, not equal)
    kept_x, kept_y = np.r_[[p[0] for p in picks], cx[accepted]], np.r_[[p[1] for p in picks], cy[accepted]]
    refused = np.flatnonzero(~keep)
    close = [i for i in refused if who[i] >= P and np.hypot(kept_x[who[i]] - cx[cand[i]], kept_y[who[i]] - cy[cand[i]]) < d / 10]
    assert close, "no two grid points converged on one centre"
    # a chain: B refused by a kept A, C kept although within d of B (and so not within d of A)
    chain = [(i, j) for i in refused if who[i] >= P for j in np.flatnonzero(keep)
             if j > i and (cx[cand[i]] - cx[cand[j]]) ** 2 + (cy[cand[i]] - cy[cand[j]]) ** 2 <= d ** 2]
    assert chain, "no chain"
    assert any(who[i] < P for i in refused), "no candidate within d of a given pick"
    # the never-assigned gate variable: K == 1 or L == 1 leaves pick_similar no grid point at all (Width <= r gives an
    # empty x_range, Height <= d an empty y_range), so it is reached in the function itself
    z = np.zeros((1, 5), np.uint32)
    assert ref["_n_block_locs_at"](np.uint64(0), np.uint64(2), 1, 5, z, z + 7) == 0
    assert rs.block_rows(np.array([2, 2, 3], np.int64), 1, 5, 2, 0)[1] == 0
    assert len(out["one_block_column/out_x"]) == 1 and len(rs.grid(all_cases["one_block_column"][1], 2.0)[0]) == 0
    # the caps are hit and change the result; single pick and std_range 0 accept the exact copies only
    for name in ("max_shifts_1", "max_shifts_2"):
        capped = details(name)[2]["shift"]
        assert (capped[5] == rs.CAPPED).any() and not mkp.same(capped[0], cx), name          # the cap moves some centre
    assert not mkp.same(out["max_shifts_1/out_x"], out["basic_f32/out_x"])                   # ... and at 1 a returned pair
    assert not (ended == rs.CAPPED).any()
    for name, P in (("single_pick", 1), ("std_range_0", 2)):
        got = np.c_[out[name + "/out_x"], out[name + "/out_y"]][P:]
        want = np.array(COPIES[P:])
        assert len(got) == len(want) and all(np.abs(got - w).max(axis=1).min() < 0.5 for w in want), (name, got)
        b = details(name)[2]["bounds"]
        assert b[0] == b[1] == 16 and b[2] == b[3], (name, b)
    assert len(out["empty_picks/out_x"]) == 0 and len(out["empty_table/out_x"]) == 0
    assert str(out["pick_without_members/raises"]) == "ZeroDivisionError"
    assert not mkp.same(out["dyadic_f32/out_x"], out["basic_f32/out_x"])


def main():
    warnings.simplefilter("ignore")
    ref = load_reference()
    all_cases = cases()
    out = {"versions": np.array(json.dumps({"pandas": pd.__version__, "numpy": np.__version__})),
           "signature": np.array(str(inspect.signature(ref["pick_similar"]))),
           "case_names": np.array(list(all_cases))}
    for name, case in all_cases.items():
        assert len(case[0]["x"]) <= 1000
        mint(ref, name, case, out)
    check_situations(ref, all_cases, out)
    path = os.path.join(HERE, "similar_cases.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 1 << 20


if __name__ == "__main__":
    main()
