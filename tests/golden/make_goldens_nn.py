#!/usr/bin/env python3
"""Mint tests/golden/nn_cases.npz: nearest-neighbour distances between small point sets.

TEST INFRASTRUCTURE, build container only (needs the reference tree).  ``nn_analysis`` of the reference's
``postprocess.py`` and ``get_NN_dist`` of its ``spinna.py`` are compiled from where they lie and run on scipy's KDTree;
nothing of the reference is stored here.

Every case stores X1, X2 (``same`` instead of X2 where the two are one array), nn_count, what ``nn_analysis`` returns and the shape of what
``get_NN_dist`` returns (asserted here to hold the same values).  ``edges`` is a JSON list of the calls the reference refuses or answers without a search (non-finite
coordinates, an empty set, nn_count <= 0, differing column counts), each with its inputs under ``edge<i>_*`` and the
exception's type and text, or the returned array.  The script asserts that every special situation a case was written
for does occur in it.

Run:  python tests/golden/make_goldens_nn.py
"""
import ast
import json
import os
import sys
import types
import warnings
from collections import OrderedDict

import numpy as np
from scipy.spatial import KDTree

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _nn_restate as rs  # noqa: E402

REF = os.environ.get("PICASSO_REFERENCE", "/root/reference")
SOURCES = {"nn_analysis": os.path.join(REF, "picasso", "postprocess.py"),
           "get_NN_dist": os.path.join(REF, "picasso", "spinna.py")}
QUERY_BLOCK = 128          # lanes of a block of the query kernel
warnings.simplefilter("ignore")


def load_reference():
    out = {}
    for name, path in SOURCES.items():
        tree = ast.parse(open(path).read())
        keep = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == name]
        assert len(keep) == 1, name
        mod = ast.Module(body=[ast.ImportFrom("__future__", [ast.alias("annotations")], 0)] + keep, type_ignores=[])
        ns = {"np": np, "KDTree": KDTree, "lib": types.SimpleNamespace()}
        exec(compile(ast.fix_missing_locations(mod), path, "exec"), ns)
        out[name] = ns[name]
    return out


def sites(rng, n_sites, per_site, size, noise, dims):
    centres = rng.uniform(0, size, (n_sites, dims))
    if dims == 3:
        centres[:, 2] = rng.uniform(-0.5, 0.5, n_sites)
    which = rng.permutation(np.repeat(np.arange(n_sites), per_site))
    return centres[which] + rng.normal(0, noise, (len(which), dims))


def cases():
    """name -> (X1, X2 or None for the self case, nn_count)."""
    out = OrderedDict()
    rng = np.random.default_rng(111)
    a2 = sites(rng, 45, 11, 32, 0.05, 2)                 # 495 rows: not a multiple of the block
    b2 = sites(rng, 40, 9, 32, 0.05, 2)
    a3 = sites(rng, 30, 13, 16, 0.04, 3)
    b3 = rng.uniform(0, 16, (700, 3)) * [1, 1, 0.05]
    out["a_self_2d_f32_k4"] = (a2.astype(np.float32), None, 4)
    out["a_self_2d_f64_k1"] = (a2, None, 1)              # (N, 1)
    out["a_self_3d_f64_k5"] = (a3, None, 5)
    out["a_self_3d_f32_k2"] = (a3.astype(np.float32), None, 2)
    out["a_self_2d_limit"] = (a2[:300], None, rs.K_MAX - 1)    # the self column included: the device limit
    out["b_two_2d_f64_k1"] = (a2, b2, 1)                 # (N,)
    out["b_two_2d_f32_k2"] = (a2.astype(np.float32), b2.astype(np.float32), 2)
    out["b_two_2d_mixed_k5"] = (a2.astype(np.float32), b2, 5)
    out["b_two_3d_f64_k5"] = (a3, b3, 5)
    out["b_two_3d_limit"] = (a3[:200], b3, rs.K_MAX)
    out["b_two_2d_int_k2"] = (rng.integers(-40, 40, (450, 2)), rng.integers(-40, 40, (300, 2)).astype(np.int32), 2)
    out["b_self_2d_int_k2"] = (rng.integers(0, 25, (400, 2)), None, 2)
    out["b_equal_copy_k2"] = (a2[:300], a2[:300].copy(), 2)          # two arrays with equal values: the self case

    # fewer rows than neighbours, and exactly as many
    few = rng.uniform(0, 4, (3, 2))
    out["c_few_two_k5"] = (a2[:300], few, 5)             # M = 3 < k = 5
    out["c_few_two_k3"] = (a2[:300], few, 3)             # M = k
    out["c_few_self_k3"] = (few, None, 3)                # k + 1 = 4 > M = 3
    out["c_few_self_k2"] = (few, None, 2)                # k + 1 = M
    out["c_one_row_k1"] = (a2[:130], few[:1], 1)

    # duplicates: zero distances beyond the self column
    dup = np.concatenate([a2[:300], a2[:120], a2[:40]])
    out["d_duplicates_self_k4"] = (dup, None, 4)
    out["d_duplicates_two_k3"] = (a2[:200], dup, 3)

    # all of X2 in one cell: one point many times (no box at all), and fewer rows than one cell holds
    out["e_one_cell_point"] = (a2[:260], np.repeat(a2[5:6], 300, axis=0), 3)
    out["e_one_cell_few"] = (a3[:260], a3[:3] + 0.25, 2)
    # X2 on a line: a box without height, and one without width
    line = rng.uniform(0, 32, 400)
    out["e_line_x"] = (a2[:250], np.stack([line, np.full(400, 7.5)], axis=1), 4)
    out["e_line_y_3d"] = (a3[:250], np.stack([np.full(400, 3.25), line / 2, rng.normal(0, 0.1, 400)], axis=1), 4)

    # queries far outside the box of X2 on every side and corner
    far = np.array([[sx * 500.0 + 16, sy * 500.0 + 16] for sx in (-1, 0, 1) for sy in (-1, 0, 1)])
    far = np.concatenate([far + rng.normal(0, 5, far.shape) for _ in range(30)])
    out["f_far_queries"] = (far, b2, 5)
    # two tight clusters in opposite corners, queries in the empty middle: a long walk over empty rings
    corners = np.concatenate([rng.normal(0, 0.02, (300, 2)), 32 + rng.normal(0, 0.02, (300, 2))])
    middle = rng.uniform(10, 22, (150, 2))
    out["f_corners_middle"] = (middle, corners, 5)
    out["f_corners_middle_3d"] = (np.concatenate([middle, rng.normal(0, 1, (150, 1))], axis=1),
                                  np.concatenate([corners, rng.normal(0, 1, (600, 1))], axis=1), 2)

    # rows and queries within a few ulps of cell edges (the grid is a function of the box, the row count and k)
    base = rng.uniform(0, 8, (700, 2))
    base[0], base[1] = (0.0, 0.0), (8.0, 8.0)
    grid = rs.Grid(base, 2)
    x2, x1 = base.copy(), rng.uniform(0, 8, (500, 2))
    for j in range(2, 420):
        a, i, steps = j % 2, 1 + (j * 7) % (grid.n[j % 2] - 1), (j % 7) - 3
        x2[j, a] = rs.ulps(grid.edge(a, i), steps)
    for j in range(360):
        a, i, steps = j % 2, 1 + (j * 5) % (grid.n[j % 2] - 1), (j % 5) - 2
        x1[j, a] = rs.ulps(grid.edge(a, i), steps)
    out["g_edges_two_k2"] = (x1, x2, 2)
    out["g_edges_self_k1"] = (x2, None, 1)               # k + 1 = 2: the same grid

    # coordinates near 1e6: a cell is a few hundred ulps wide
    big = 1.0e6 + rng.uniform(0, 1e-6, (700, 2))
    out["h_big_self_k4"] = (big, None, 4)
    out["h_big_two_3d_k2"] = (np.concatenate([1.0e6 + rng.uniform(-2.5e-7, 1.25e-6, (300, 2)), rng.uniform(0, 1e-6, (300, 1))], axis=1),
                              np.concatenate([big, rng.uniform(0, 1e-6, (700, 1))], axis=1), 2)
    return out


def edge_calls():
    """What is refused, or answered without a search: (label, function, X1, X2, nn_count)."""
    rng = np.random.default_rng(112)
    a, b = rng.uniform(0, 4, (6, 2)), rng.uniform(0, 4, (9, 2))
    nan1, inf1, nan2, inf2 = a.copy(), a.copy(), b.copy(), b.copy()
    nan1[2, 0], inf1[3, 1], nan2[4, 1], inf2[0, 0] = np.nan, np.inf, np.nan, -np.inf
    empty = np.zeros((0, 2))
    calls = []
    for fn in ("nn_analysis", "get_NN_dist"):
        calls += [("nan in X1", fn, nan1, b, 2), ("inf in X1", fn, inf1, b, 2), ("nan in X2", fn, a, nan2, 2),
                  ("inf in X2", fn, a, inf2, 2), ("nan in both, self", fn, nan1, nan1, 2),
                  ("nan in X1, k 0", fn, nan1, b, 0), ("nan in X2, k 0", fn, a, nan2, 0),
                  ("nan in X2, columns differ", fn, rng.uniform(0, 4, (5, 3)), nan2, 2),
                  ("empty X2, k 2", fn, a, empty, 2), ("empty X2, k 1", fn, a, empty, 1),
                  ("empty X1, k 2", fn, empty, b, 2), ("empty X1, k 1", fn, empty, b, 1),
                  ("both empty, k 2", fn, empty, empty, 2), ("empty X2, k 0", fn, a, empty, 0),
                  ("empty X1, nan in X2", fn, empty, nan2, 2),
                  ("k 0", fn, a, b, 0), ("k -1", fn, a, b, -1), ("k 0, self", fn, a, a, 0), ("k -1, self", fn, a, a, -1),
                  ("k -2, self", fn, a, a, -2),
                  ("columns differ", fn, rng.uniform(0, 4, (5, 3)), b, 2),
                  ("columns differ, empty X2", fn, rng.uniform(0, 4, (5, 3)), empty, 2)]
    return calls


def record(call):
    try:
        return {"returns": np.asarray(call())}
    except Exception as e:      # noqa: BLE001
        return {"raises": type(e).__name__, "text": str(e)}


def check_situations(name, X1, X2, k, nn, dist):
    same = X2 is None
    Y = X1 if same else X2
    n, m, total = len(X1), len(Y), k + (1 if same else 0)
    grid = rs.Grid(Y, total)
    cx, cy = grid.cells(Y)
    want = rs.nn_analysis(X1, Y, k)
    assert want.shape == nn.shape and np.array_equal(want.view(np.uint8), np.ascontiguousarray(nn).view(np.uint8)), name
    assert dist.shape == (n, k) and np.array_equal(dist.reshape(nn.shape), nn), name
    if name.startswith("a_") or name.startswith("b_"):
        assert n % QUERY_BLOCK != 0 and grid.n[0] > 2 and grid.n[1] > 2
    if name in ("a_self_2d_f64_k1", "g_edges_self_k1"):
        assert nn.shape == (n, 1)
    if name in ("b_two_2d_f64_k1", "c_one_row_k1"):
        assert nn.shape == (n,)
    if name.endswith("limit"):
        assert total == rs.K_MAX
    if name == "b_equal_copy_k2":
        assert X1 is not X2 and np.array_equal(X1, X2)
    if "_int_" in name:
        assert X1.dtype.kind == "i" and Y.dtype.kind == "i"
    if name.startswith("c_"):
        assert total >= m
        inf_columns = np.isinf(nn.reshape(n, -1)).all(axis=0).sum()
        assert inf_columns == total - m and np.isfinite(nn.reshape(n, -1)[:, :k - inf_columns]).all()
    if name.startswith("d_"):
        assert (nn.reshape(n, -1)[:, 0] == 0).sum() >= 100 and (nn.reshape(n, -1)[:, 1] == 0).sum() >= 40 and total < m
    if name.startswith("e_one_cell"):
        assert grid.n == [1, 1]
    if name == "e_line_x":
        assert grid.n[1] == 1 and grid.n[0] > 50
    if name == "e_line_y_3d":
        assert grid.n[0] == 1 and grid.n[1] > 50
    if name == "f_far_queries":
        qx, qy = grid.cells(X1)
        for want_x in (0, grid.n[0] - 1):
            for want_y in (0, grid.n[1] - 1):
                assert ((qx == want_x) & (qy == want_y)).sum() >= 20
        lo, hi = Y.min(axis=0), Y.max(axis=0)
        for a in range(2):
            assert (X1[:, a] < lo[a] - 100).sum() >= 60 and (X1[:, a] > hi[a] + 100).sum() >= 60
    if name.startswith("f_corners_middle"):
        assert min(grid.n) >= 8 and rs.rings_needed(grid, X1, Y, total).min() >= min(grid.n) // 4
    if name.startswith("g_edges"):
        for Z, least in ((Y, 350), (X1, 300)):
            hits = 0
            for a in range(2):
                i = grid.cell_of(a, Z[:, a])
                for e in (grid.edge(a, i), grid.edge(a, i + 1)):
                    hits += (np.abs(Z[:, a] - e) <= 4 * np.spacing(e)).sum()
            assert hits >= least, (name, hits)
        on_edge = sum((Y[:, a] == grid.edge(a, grid.cell_of(a, Y[:, a]))).sum() for a in range(2))
        assert on_edge >= 50
    if name.startswith("h_big"):
        for a in range(2):
            assert grid.n[a] > 8 and 50 < grid.w[a] / np.spacing(1.0e6) < 2000
    return grid


def main():
    ref = load_reference()
    data = {"case_names": np.array(list(cases()))}
    for name, (X1, X2, k) in cases().items():
        assert len(X1) <= 1000 and (X2 is None or len(X2) <= 1000)
        Y = X1 if X2 is None else X2
        before = (X1.copy(), Y.copy())
        nn = ref["nn_analysis"](X1, Y, k)
        dist = ref["get_NN_dist"](X1, Y, k)
        assert np.array_equal(before[0], X1) and np.array_equal(before[1], Y) and nn.dtype == dist.dtype == np.float64
        grid = check_situations(name, X1, X2, k, nn, dist)
        p = name + "/"
        data[p + "X1"], data[p + "nn_count"] = X1, np.array(k)
        if X2 is None:
            data[p + "same"] = np.array(True)
        else:
            data[p + "X2"] = X2
        data[p + "nn_analysis"], data[p + "get_NN_dist_shape"] = nn, np.array(dist.shape)      # dist is nn in that shape
        print(f"{name}: {X1.shape} {X1.dtype} against {'itself' if X2 is None else str(X2.shape) + ' ' + str(X2.dtype)}, "
              f"k = {k}, grid {grid.n[0]} x {grid.n[1]}, returns {nn.shape} / {dist.shape}", flush=True)
    edges = []
    for i, (label, fn, X1, X2, k) in enumerate(edge_calls()):
        got = record(lambda: ref[fn](X1, X2, k))
        entry = {"label": label, "function": fn, "nn_count": k, "self": X1 is X2}
        data[f"edge{i}_X1"] = X1
        if X1 is not X2:
            data[f"edge{i}_X2"] = X2
        if "raises" in got:
            entry.update(raises=got["raises"], text=got["text"])
        else:
            entry["returns"] = True
            data[f"edge{i}_out"] = got["returns"]
        edges.append(entry)
        print(fn, label, "->", got.get("raises", None) or ("array", got["returns"].shape), got.get("text", ""), flush=True)
    data["edges"] = np.array(json.dumps(edges))
    path = os.path.join(HERE, "nn_cases.npz")
    np.savez_compressed(path, **data)
    print(path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 768 * 1024          # a committed file may have 1 MiB


if __name__ == "__main__":
    main()
