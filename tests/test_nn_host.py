"""CPU tier of the nearest-neighbour distances (picasso_amd/postprocess.py nn_analysis, picasso_amd/spinna.py
get_NN_dist, csrc/knn.hip): the brute-force float64 restatement (tests/golden/_nn_restate.py) reproduces every array
the reference recorded (tests/golden/nn_cases.npz); so does the search header the kernels are compiled from
(csrc/knn_search.h), built here with the host compiler (tests/nn_host_driver.cpp), whose stopping rule is thereby
checked without a GPU; the goldens regenerate from the reference tree where it is present; and the Python surface
(signatures, NN_NAMES, install(), the errors and answers that come before any device work) and the ABI are checked."""
import ctypes
import inspect
import json
import os
import subprocess
import sys
import types

import numpy as np
import pytest

from conftest import GOLDEN, ROOT, golden

sys.path.insert(0, GOLDEN)
import _nn_restate as rs  # noqa: E402

from picasso_amd import _lib, backend, localize, postprocess, spinna  # noqa: E402

CASES = [str(c) for c in golden("nn_cases")["case_names"]]
EDGES = json.loads(str(golden("nn_cases")["edges"]))
_NO = "<no default>"
SIGNATURES = {      # picasso/postprocess.py:3704, picasso/spinna.py:696
    "nn_analysis": (postprocess, "postprocess.py", [("X1", _NO), ("X2", _NO), ("nn_count", _NO)]),
    "get_NN_dist": (spinna, "spinna.py", [("data1", _NO), ("data2", _NO), ("n_neighbors", _NO)]),
}
FUNCTIONS = {"nn_analysis": postprocess.nn_analysis, "get_NN_dist": spinna.get_NN_dist}


@pytest.fixture(scope="module")
def g():
    return golden("nn_cases")


def case(g, name):
    p = name + "/"
    X1 = g[p + "X1"]
    X2 = X1 if p + "same" in g.files else g[p + "X2"]
    return p, X1, X2, int(g[p + "nn_count"])


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    """csrc/knn_search.h behind a C entry, compiled with the host compiler."""
    out = str(tmp_path_factory.mktemp("nn_host") / "nn_host.so")
    subprocess.run([os.environ.get("CXX", "c++"), "-O2", "-std=c++17", "-shared", "-fPIC", "-ffp-contract=off",
                    "-I", os.path.join(ROOT, "picasso_amd", "csrc"), os.path.join(ROOT, "tests", "nn_host_driver.cpp"),
                    "-o", out], check=True)
    lib = ctypes.CDLL(out)
    p, i64, i32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int
    lib.nn_host.argtypes, lib.nn_host.restype = [p, i64, p, i64, i32, i32, p, p, p, p, p], i32

    def run(X1, X2, k):
        X1, X2 = np.ascontiguousarray(X1, np.float64), np.ascontiguousarray(X2, np.float64)
        out = np.zeros((len(X1), k))
        n, lo_w = np.zeros(2, np.int32), np.zeros(4)
        cx, cy = np.zeros(len(X2), np.int32), np.zeros(len(X2), np.int32)
        assert lib.nn_host(_lib.ptr(X1), len(X1), _lib.ptr(X2), len(X2), X1.shape[1], k, _lib.ptr(out), _lib.ptr(n),
                           _lib.ptr(lo_w), _lib.ptr(cx), _lib.ptr(cy)) == 0
        return out, n, lo_w, cx, cy

    run.limit = lib.nn_host_limit()
    return run


@pytest.mark.parametrize("name", CASES)
def test_restatement_reproduces_the_reference(g, name):
    p, X1, X2, k = case(g, name)
    nn = rs.nn_analysis(X1, X2, k)
    assert same(nn, g[p + "nn_analysis"])
    dist = rs.get_NN_dist(X1, X2, k)
    assert dist.shape == tuple(g[p + "get_NN_dist_shape"]) == (len(X1), k) and same(dist.reshape(nn.shape), nn)


@pytest.mark.parametrize("name", CASES)
def test_search_header_reproduces_the_reference(g, host, name):
    """The ring walk and its stopping bound, as the kernels have them, on every golden case; the grid and the cells are
    those of the restatement the goldens' situations were asserted with."""
    p, X1, X2, k = case(g, name)
    total = k + (1 if np.array_equal(X1, X2) else 0)
    out, n, lo_w, cx, cy = host(X1, X2, total)
    got = out[:, 1:] if total > k else (out[:, 0] if k == 1 else out)
    assert same(got, g[p + "nn_analysis"])
    grid = rs.Grid(X2, total)
    assert list(n) == grid.n and list(lo_w) == grid.lo + grid.w
    rx, ry = grid.cells(X2)
    assert np.array_equal(cx, rx) and np.array_equal(cy, ry)


def test_search_header_on_many_small_sets(host):
    """Every k up to the limit, 2-D and 3-D, sets of 1 to a few hundred rows in boxes of every aspect, queries inside
    and far outside: the header's answer is the sorted brute-force matrix, in every bit."""
    assert host.limit == rs.K_MAX
    rng = np.random.default_rng(7)
    for trial in range(150):
        dims, m, n = 2 + trial % 2, int(rng.integers(1, 400)), 60
        k = int(rng.integers(1, rs.K_MAX + 1))
        scale = 10.0 ** rng.integers(-3, 4, dims)
        X2 = rng.uniform(0, 1, (m, dims)) * scale + rng.uniform(-5, 5, dims) * scale
        if trial % 5 == 0:
            X2 = np.round(X2 / scale, 1) * scale                              # many ties and duplicates
        X1 = np.concatenate([X2[rng.integers(0, m, 20)] + rng.normal(0, 0.01, (20, dims)) * scale,
                             rng.uniform(-3, 4, (40, dims)) * scale + X2.mean(axis=0)])
        assert same(host(X1, X2, k)[0], rs.distances(X1, X2, k)), (trial, dims, m, k)


def test_goldens_hold_what_they_are_for(g):
    assert g["a_self_2d_f64_k1/nn_analysis"].shape == (495, 1) and g["b_two_2d_f64_k1/nn_analysis"].shape == (495,)
    assert g["a_self_2d_limit/nn_analysis"].shape[1] == rs.K_MAX - 1 and g["b_two_3d_limit/nn_analysis"].shape[1] == rs.K_MAX
    assert g["a_self_2d_f32_k4/X1"].dtype == np.float32 and g["b_two_2d_int_k2/X1"].dtype == np.int64
    assert g["b_two_2d_int_k2/X2"].dtype == np.int32 and g["b_two_2d_mixed_k5/X2"].dtype == np.float64
    assert np.isinf(g["c_few_two_k5/nn_analysis"][:, 3:]).all() and np.isfinite(g["c_few_two_k5/nn_analysis"][:, :3]).all()
    assert np.isfinite(g["c_few_two_k3/nn_analysis"]).all() and np.isinf(g["c_few_self_k3/nn_analysis"][:, 2]).all()
    assert np.isfinite(g["c_few_self_k2/nn_analysis"]).all()
    assert (g["d_duplicates_self_k4/nn_analysis"][:, 1] == 0).sum() >= 40
    assert "b_equal_copy_k2/X2" in g.files and np.array_equal(g["b_equal_copy_k2/X1"], g["b_equal_copy_k2/X2"])
    p, X1, X2, k = case(g, "f_corners_middle")
    grid = rs.Grid(X2, k)
    assert rs.rings_needed(grid, X1, X2, k).min() >= 3
    assert any(e["label"] == "k 0, self" and e.get("raises") == "IndexError" for e in EDGES)
    assert {e["label"] for e in EDGES} >= {"nan in X1", "inf in X2", "empty X2, k 1", "k -1", "columns differ"}


@pytest.mark.parametrize("name", sorted(SIGNATURES))
def test_signatures_equal_the_reference(name):
    module, _, want = SIGNATURES[name]
    got = [(n, _NO if q.default is inspect.Parameter.empty else q.default)
           for n, q in inspect.signature(getattr(module, name)).parameters.items()]
    assert got == want


def test_signatures_are_the_reference_trees():
    import ast
    ref = os.environ.get("PICASSO_REFERENCE", "/root/reference")
    if not os.path.isfile(os.path.join(ref, "picasso", "spinna.py")):
        pytest.skip("reference tree not present")
    for name, (_, source, want) in SIGNATURES.items():
        tree = ast.parse(open(os.path.join(ref, "picasso", source)).read())
        a = {n.name: n for n in tree.body if isinstance(n, ast.FunctionDef)}[name].args
        assert [x.arg for x in a.args] == [w[0] for w in want] and not a.defaults and not a.kwonlyargs, name


def test_nn_names_and_install():
    assert postprocess.NN_NAMES == ("nn_analysis",) and spinna.SPINNA_NAMES == ("get_NN_dist",)
    mods = {n: types.ModuleType("picasso." + n) for n in
            ("localize", "gaussmle", "gausslq", "zfit", "render", "imageprocess", "postprocess", "aim", "clusterer",
             "spinna")}
    mods["postprocess"].resi = "theirs"
    mods["spinna"].get_NN_dist_simulated = mods["spinna"].NND_score = "theirs"
    args = [mods[n] for n in ("localize", "gaussmle", "gausslq", "zfit", "render", "imageprocess", "postprocess")]
    localize.install(*args, picasso_aim=mods["aim"], picasso_clusterer=mods["clusterer"])
    assert mods["postprocess"].nn_analysis is postprocess.nn_analysis and not hasattr(mods["spinna"], "get_NN_dist")
    localize.install(*args, picasso_aim=mods["aim"], picasso_clusterer=mods["clusterer"], picasso_spinna=mods["spinna"])
    assert mods["spinna"].get_NN_dist is spinna.get_NN_dist
    assert mods["postprocess"].resi == "theirs"
    assert {k: v for k, v in vars(mods["spinna"]).items() if not k.startswith("__")} == {
        "get_NN_dist": spinna.get_NN_dist, "get_NN_dist_simulated": "theirs", "NND_score": "theirs"}
    for name in postprocess.PAIR_NAMES + postprocess.LINK_NENA_NAMES + postprocess.KINETICS_NAMES + ("segment", "undrift"):
        assert getattr(mods["postprocess"], name) is getattr(postprocess, name)
    assert inspect.signature(localize.install).parameters["picasso_spinna"].default is None


def test_abi_version_and_symbols():
    lib = _lib.load()
    assert lib.pmi_version() >= 114
    for name in ("pmi_knn_limit", "pmi_knn_order_dev", "pmi_knn_query_dev"):
        assert name in _lib.SYMBOLS and hasattr(lib, name)
    assert backend.knn_limit() == rs.K_MAX >= 32


@pytest.mark.parametrize("i", range(len(EDGES)), ids=[e["function"] + ": " + e["label"] for e in EDGES])
def test_edges_as_the_reference_recorded(g, i, monkeypatch):
    """Non-finite coordinates, empty sets, nn_count <= 0 and differing column counts: the reference's exception (type
    and text) or array, and no device is asked for."""
    monkeypatch.setattr(_lib, "require_gpu", lambda: pytest.fail("device work"))
    e = EDGES[i]
    X1 = g[f"edge{i}_X1"]
    X2 = X1 if e["self"] else g[f"edge{i}_X2"]
    fn = FUNCTIONS[e["function"]]
    if "raises" in e:
        with pytest.raises(getattr(__import__("builtins"), e["raises"])) as err:
            fn(X1, X2, e["nn_count"])
        assert type(err.value).__name__ == e["raises"] and str(err.value) == e["text"]
    else:
        assert same(fn(X1, X2, e["nn_count"]), g[f"edge{i}_out"])


def test_limits_come_before_device_work(monkeypatch):
    monkeypatch.setattr(_lib, "require_gpu", lambda: pytest.fail("device work"))
    rng = np.random.default_rng(5)
    a, b = rng.uniform(0, 1, (40, 2)), rng.uniform(0, 1, (50, 2))
    limit = backend.knn_limit()
    for fn in FUNCTIONS.values():
        for dims in (1, 4):
            with pytest.raises(NotImplementedError, match="2 or 3 dimensions"):
                fn(rng.uniform(0, 1, (40, dims)), rng.uniform(0, 1, (50, dims)), 2)
        with pytest.raises(ValueError, match=f"device limit of {limit}"):
            fn(a, b, limit + 1)
        with pytest.raises(ValueError, match=f"device limit of {limit}"):
            fn(a, a, limit)                      # the self column counts


def test_device_points_are_checked_before_device_work(monkeypatch):
    """``KnnIndex(points, k, box)`` hands raw pointers on: anything but a float64 device tensor is refused, and so is a
    box that is not two pairs."""
    import torch
    monkeypatch.setattr(_lib, "require_gpu", lambda: pytest.fail("device work"))
    box = ([0.0, 0.0], [1.0, 1.0])
    for points in (np.zeros((5, 2)), torch.zeros((5, 2), dtype=torch.float64), torch.zeros((5, 2)), [[0.0, 0.0]]):
        with pytest.raises(ValueError, match="contiguous float64 device tensor"):
            backend.KnnIndex(points, 2, box)


def test_no_device_raises(monkeypatch):
    monkeypatch.setattr(_lib, "device_count", lambda: 0)
    rng = np.random.default_rng(6)
    a, b = rng.uniform(0, 1, (40, 2)), rng.uniform(0, 1, (50, 2))
    for fn in FUNCTIONS.values():
        with pytest.raises(_lib.HipBackendError):
            fn(a, b, 2)


def test_goldens_regenerate(g):
    """The committed nn_cases.npz is what make_goldens_nn.py mints from the reference tree today."""
    ref = os.environ.get("PICASSO_REFERENCE", "/root/reference")
    if not os.path.isfile(os.path.join(ref, "picasso", "spinna.py")):
        pytest.skip("reference tree not present")
    import make_goldens_nn as mk
    fns = mk.load_reference()
    cases = mk.cases()
    assert list(cases) == CASES
    for name, (X1, X2, k) in cases.items():
        p = name + "/"
        assert same(X1, g[p + "X1"]) and k == int(g[p + "nn_count"]) and ((X2 is None) == (p + "same" in g.files))
        Y = X1 if X2 is None else X2
        if X2 is not None:
            assert same(X2, g[p + "X2"])
        assert same(fns["nn_analysis"](X1, Y, k), g[p + "nn_analysis"])
        assert fns["get_NN_dist"](X1, Y, k).shape == tuple(g[p + "get_NN_dist_shape"])
    calls = mk.edge_calls()
    assert [(c[0], c[1], c[4]) for c in calls] == [(e["label"], e["function"], e["nn_count"]) for e in EDGES]
    for i, (label, fn, X1, X2, k) in enumerate(calls):
        got = mk.record(lambda: fns[fn](X1, X2, k))
        if "raises" in got:
            assert (got["raises"], got["text"]) == (EDGES[i]["raises"], EDGES[i]["text"])
        else:
            assert same(got["returns"], g[f"edge{i}_out"])
