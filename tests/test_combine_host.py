"""CPU tier of the cluster combine (picasso_amd/postprocess.py cluster_combine / cluster_combine_dist, csrc/combine.hip):
the NumPy restatement (tests/golden/_combine_restate.py) reproduces every table the reference recorded
(tests/golden/combine_cases.npz) in bits; its float32 sum is ``ndarray.sum()``; the header the kernels are compiled from
(csrc/segment_stats.h, with the distance of csrc/knn_search.h), built here with the host compiler
(tests/combine_host_driver.cpp), gives the same tables through the public functions themselves, the device entry points
of ``backend`` replaced by the host build; and the Python surface (signatures, COMBINE_NAMES, install(), the errors that
come before any device work) and the ABI are checked.

The zero weight sum is the one error that needs the statistics: the device returns the sums and the host raises, so
that test feeds the public function sums from the host build and requires the reference's type and text."""
import builtins
import ctypes
import inspect
import json
import os
import subprocess
import sys
import types

import numpy as np
import pandas as pd
import pytest

from conftest import GOLDEN, ROOT, golden

sys.path.insert(0, GOLDEN)
import _combine_restate as rs  # noqa: E402
import make_goldens_combine as mk  # noqa: E402

from picasso_amd import _lib, backend, localize, postprocess  # noqa: E402

G = golden("combine_cases")
COMBINE = [str(c) for c in G["combine_case_names"]]
DIST = [str(c) for c in G["dist_case_names"]]
EDGES = json.loads(str(G["edges"]))
FUNCTIONS = {"cluster_combine": postprocess.cluster_combine, "cluster_combine_dist": postprocess.cluster_combine_dist}


def inputs(p):
    return {str(c): G[p + "in_" + str(c)] for c in G[p + "in_columns"]}


def assert_table(got, p):
    """``got``: a DataFrame or a dict of arrays; names, order, dtypes and every bit (any NaN equals any NaN)."""
    names = [str(c) for c in G[p + "columns"]]
    assert list(got) == names
    if isinstance(got, pd.DataFrame):
        assert isinstance(got.index, pd.RangeIndex) and got.index.start == 0 and got.index.step == 1
        assert len(got) == len(G[p + "out_" + names[0]])
        got = {c: got[c].to_numpy() for c in names}
    for c, dt in zip(names, G[p + "dtypes"]):
        assert str(got[c].dtype) == str(dt), c
        assert mk.same(got[c], G[p + "out_" + c]), (c, np.flatnonzero(~(got[c] == G[p + "out_" + c]))[:8])


# ---- the restatement ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", COMBINE)
def test_restatement_reproduces_cluster_combine(name):
    p = "combine/" + name + "/"
    assert_table(rs.cluster_combine(inputs(p)), p)


@pytest.mark.parametrize("name", DIST)
def test_restatement_reproduces_cluster_combine_dist(name):
    p = "dist/" + name + "/"
    assert_table(rs.cluster_combine_dist(inputs(p), mk.pixelsize_from(G[p + "pixelsize"])), p)


def test_float32_sum_is_numpys():
    rng = np.random.default_rng(11)
    for n in list(range(0, 301)) + [8191, 8192, 8193]:
        a = (rng.uniform(-1, 1, n) * 10.0 ** rng.integers(-3, 6, n)).astype(np.float32)
        assert rs.sum32(a).tobytes() == a.sum().tobytes(), n
        assert rs.sum32(a).dtype == np.float32


def test_goldens_hold_what_they_are_for():
    lengths = sorted(G["combine/a_2d_f32_u32_i32/out_n"])
    assert lengths == [1, 2, 7, 8, 9, 127, 128, 129, 1000]
    assert G["combine/a_2d_f32_u32_i32/in_frame"].dtype == np.uint32 and G["combine/b_3d_f64_i64_i64/in_frame"].dtype == np.int64
    assert G["combine/c_3d_f32_labels_f64/in_group"].dtype == np.float64 and G["combine/f_300_small/in_cluster"].dtype == np.int64
    assert G["combine/a_2d_f32_u32_i32/in_group"].min() < 0 and G["combine/a_2d_f32_u32_i32/in_cluster"].min() < 0
    assert np.isnan(G["combine/e_2d_nan/in_photons"]).sum() == 1 and np.isnan(G["combine/e_2d_nan/in_x"]).sum() == 1
    sizes = sorted(np.unique(G["dist/i_3d_none/in_group"], return_counts=True)[1])
    assert sizes == [2, 3, 63, 64, 65, 300]
    kinds = {json.loads(str(G["dist/" + n + "/pixelsize"]))["kind"] for n in DIST}
    assert kinds == {"none", "int", "float", "np.float64"}
    assert {e["label"] for e in EDGES} >= {"zero weight sum", "empty table", "single-cluster group", "repeated label"}


# ---- the header, built for the host, under the public functions --------------------------------------------
@pytest.fixture(scope="module")
def host(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("combine_host") / "combine_host.so")
    subprocess.run([os.environ.get("CXX", "c++"), "-O2", "-std=c++17", "-shared", "-fPIC", "-ffp-contract=off",
                    "-I", os.path.join(ROOT, "picasso_amd", "csrc"), os.path.join(ROOT, "tests", "combine_host_driver.cpp"),
                    "-o", out], check=True)
    lib = ctypes.CDLL(out)
    p, i32 = ctypes.c_void_p, ctypes.c_int32
    lib.combine_host_moments.argtypes = [p, i32, p, i32, p, p]
    lib.combine_host_averages.argtypes = [p, p, i32, p, i32, p, p]
    lib.combine_host_nearest.argtypes = [p, i32, p, i32, p, p]
    lib.combine_host_sum32.argtypes, lib.combine_host_sum32.restype = [p, i32], ctypes.c_float
    return lib


class HostGroups:
    """What ``backend.CombineGroups`` holds, from the restatement's ``np.lexsort``."""

    def __init__(self, group, cluster):
        assert group.dtype == np.int64 and cluster.dtype == np.int64
        order, start, self.unique, self.clusters, group_start = rs.segments(group, cluster)
        self.n, self.n_groups, self.n_outer = len(group), len(start) - 1, len(group_start) - 1
        self.rows, self.offsets = order, start.astype(np.int32)
        self.group_offsets = group_start.astype(np.int32)
        self.n_locs = np.diff(start).astype(np.int64)


def host_backend(monkeypatch, lib):
    def stats(groups, moments=(), averages=()):
        S, start = groups.n_groups, np.ascontiguousarray(groups.offsets)
        first, second = [], []
        for c in moments:
            c = np.asarray(c)
            vs = np.ascontiguousarray(c[groups.rows].astype(c.dtype if c.dtype == np.float32 else np.float64))
            mean, sd = np.zeros(S), np.zeros(S)
            lib.combine_host_moments(_lib.ptr(vs), int(vs.dtype == np.float64), _lib.ptr(start), S, _lib.ptr(mean), _lib.ptr(sd))
            first.append((mean, sd))
        for x, w in averages:
            assert x.dtype == w.dtype and x.dtype in (np.float32, np.float64)
            xs, ws = np.ascontiguousarray(x[groups.rows]), np.ascontiguousarray(w[groups.rows])
            avg, scl = np.zeros(S), np.zeros(S)
            lib.combine_host_averages(_lib.ptr(xs), _lib.ptr(ws), int(xs.dtype == np.float64), _lib.ptr(start), S,
                                      _lib.ptr(avg), _lib.ptr(scl))
            second.append((avg, scl))
        return first, second

    def nearest(groups, points):
        assert points.dtype == np.float64 and points.flags.c_contiguous and groups.n_groups == groups.n
        pts = np.ascontiguousarray(points[groups.rows])
        first = np.ascontiguousarray(groups.offsets[groups.group_offsets])
        out, out_xy = np.zeros(groups.n), np.zeros(groups.n)
        assert lib.combine_host_nearest(_lib.ptr(pts), points.shape[1], _lib.ptr(first), groups.n_outer, _lib.ptr(out),
                                        _lib.ptr(out_xy)) == 0
        return out, (out_xy if points.shape[1] == 3 else None)

    monkeypatch.setattr(_lib, "require_gpu", lambda: pytest.fail("device work"))
    monkeypatch.setattr(backend, "CombineGroups", HostGroups)
    monkeypatch.setattr(backend, "combine_stats", stats)
    monkeypatch.setattr(backend, "combine_min_distances", nearest)


@pytest.mark.parametrize("name", COMBINE)
def test_header_reproduces_cluster_combine(host, monkeypatch, name):
    host_backend(monkeypatch, host)
    p = "combine/" + name + "/"
    assert_table(postprocess.cluster_combine(pd.DataFrame(inputs(p))), p)


@pytest.mark.parametrize("name", DIST)
def test_header_reproduces_cluster_combine_dist(host, monkeypatch, name):
    host_backend(monkeypatch, host)
    p = "dist/" + name + "/"
    assert_table(postprocess.cluster_combine_dist(pd.DataFrame(inputs(p)), mk.pixelsize_from(G[p + "pixelsize"])), p)


def test_header_float32_sum_is_numpys(host):
    rng = np.random.default_rng(12)
    for n in list(range(0, 301)) + [8191, 8192, 8193, 20000]:
        a = (rng.uniform(-1, 1, n) * 10.0 ** rng.integers(-3, 6, n)).astype(np.float32)
        assert np.float32(host.combine_host_sum32(_lib.ptr(a), n)).tobytes() == a.sum().tobytes(), n


def test_header_on_long_and_unequal_segments(host, monkeypatch):
    """4 096 segments of one row beside one of 20 000: beyond one 8192-element buffer of NumPy's reduction."""
    host_backend(monkeypatch, host)
    cols = mk.sweep_table()
    want = rs.cluster_combine(cols)
    got = postprocess.cluster_combine(pd.DataFrame(cols))
    assert list(got.columns) == list(want)
    for c in want:
        assert mk.same(got[c].to_numpy(), want[c]), c


# ---- the errors that come before any device work -------------------------------------------------------------
def no_device(monkeypatch):
    monkeypatch.setattr(_lib, "require_gpu", lambda: pytest.fail("device work"))
    monkeypatch.setattr(_lib, "load", lambda: pytest.fail("a library call"))


def edge_inputs(i):
    return {str(c): G[f"edge{i}_in_{c}"] for c in G[f"edge{i}_columns"]}


@pytest.mark.parametrize("i", [i for i, e in enumerate(EDGES) if e["label"] != "zero weight sum"],
                         ids=[e["function"] + ": " + e["label"] for e in EDGES if e["label"] != "zero weight sum"])
def test_edges_raise_as_the_reference_recorded(i, monkeypatch):
    no_device(monkeypatch)
    e = EDGES[i]
    with pytest.raises(getattr(builtins, e["raises"])) as err:
        FUNCTIONS[e["function"]](pd.DataFrame(edge_inputs(i)))
    assert type(err.value).__name__ == e["raises"] and str(err.value) == e["text"]


def test_zero_weight_sum_raises_numpys_error(host, monkeypatch):
    host_backend(monkeypatch, host)
    monkeypatch.setattr(_lib, "load", lambda: pytest.fail("a library call"))
    i = [e["label"] for e in EDGES].index("zero weight sum")
    assert EDGES[i]["raises"] == "ZeroDivisionError"
    with pytest.raises(ZeroDivisionError) as err:
        postprocess.cluster_combine(pd.DataFrame(edge_inputs(i)))
    assert str(err.value) == EDGES[i]["text"] == "Weights sum to zero, can't be normalized"
    cols = inputs("combine/e_2d_nan/")                      # a NaN weight raises nothing
    assert np.isnan(postprocess.cluster_combine(pd.DataFrame(cols))["x"]).sum() >= 1


@pytest.mark.parametrize("fn", sorted(FUNCTIONS))
def test_bad_labels_raise_before_device_work(fn, monkeypatch):
    no_device(monkeypatch)
    p = "combine/g_sorted_table/" if fn == "cluster_combine" else "dist/h_2d/"
    for column in ("group", "cluster"):
        for bad in (0.5, np.nan, np.inf):
            cols = inputs(p)
            cols[column] = cols[column].astype(np.float64)
            cols[column][3] = bad
            with pytest.raises(ValueError):
                FUNCTIONS[fn](pd.DataFrame(cols))
        cols = inputs(p)
        cols[column] = np.array([str(v) for v in cols[column]], dtype=object)
        with pytest.raises(ValueError):
            FUNCTIONS[fn](pd.DataFrame(cols))


def test_array_entry_points_check_what_they_are_given(monkeypatch):
    no_device(monkeypatch)
    with pytest.raises(TypeError):
        backend.combine_stats(object())
    with pytest.raises(TypeError):
        backend.combine_min_distances(object(), np.zeros((3, 2)))
    fake = backend.CombineGroups.__new__(backend.CombineGroups)
    fake.n, fake.n_groups, fake.n_outer = 4, 4, 2
    for points in (np.zeros((4, 2), np.float32), np.zeros((4, 4)), np.zeros((3, 2)), np.zeros((2, 4)).T, [[0.0, 0.0]] * 4):
        with pytest.raises(ValueError, match="C-contiguous float64"):
            backend.combine_min_distances(fake, points)
    fake.n_groups = 3
    with pytest.raises(ValueError, match="one row"):
        backend.combine_min_distances(fake, np.zeros((4, 2)))
    with pytest.raises(TypeError, match="float32 or float64"):
        backend.combine_stats(fake, averages=[(np.zeros(4, np.int32), np.zeros(4, np.int32))])
    with pytest.raises(ValueError, match="one floating type"):
        backend.combine_stats(fake, averages=[(np.zeros(4, np.float32), np.zeros(4, np.float64))])
    with pytest.raises(ValueError, match="one entry per row"):
        backend.combine_stats(fake, moments=[np.zeros(5)])


def test_no_device_raises(monkeypatch):
    monkeypatch.setattr(_lib, "device_count", lambda: 0)
    with pytest.raises(_lib.HipBackendError):
        postprocess.cluster_combine(pd.DataFrame(inputs("combine/g_sorted_table/")))
    with pytest.raises(_lib.HipBackendError):
        postprocess.cluster_combine_dist(pd.DataFrame(inputs("dist/j_2d_shuffled/")))


# ---- names, signatures, install, ABI ---------------------------------------------------------------------------
def test_combine_names_and_signatures():
    assert postprocess.COMBINE_NAMES == ("cluster_combine", "cluster_combine_dist")
    recorded = json.loads(str(G["signatures"]))
    assert sorted(recorded) == sorted(postprocess.COMBINE_NAMES)
    for name in postprocess.COMBINE_NAMES:
        assert str(inspect.signature(getattr(postprocess, name))) == recorded[name], name


def test_install_rebinds_the_two_names():
    mods = {n: types.ModuleType("picasso." + n) for n in
            ("localize", "gaussmle", "gausslq", "zfit", "render", "imageprocess", "postprocess", "aim", "clusterer")}
    mods["postprocess"].cluster_combine = mods["postprocess"].calculate_fret = "theirs"
    args = [mods[n] for n in ("localize", "gaussmle", "gausslq", "zfit", "render", "imageprocess", "postprocess")]
    localize.install(*args, picasso_aim=mods["aim"], picasso_clusterer=mods["clusterer"])
    for name in postprocess.COMBINE_NAMES:
        assert getattr(mods["postprocess"], name) is getattr(postprocess, name)
    assert mods["postprocess"].calculate_fret == "theirs"


def test_abi_version_and_symbols():
    lib = _lib.load()
    assert lib.pmi_version() >= 115
    for name in ("pmi_combine_order_dev", "pmi_combine_stats_dev", "pmi_combine_mindist_dev"):
        assert name in _lib.SYMBOLS and hasattr(lib, name)
    header = open(os.path.join(ROOT, "include", "picasso_hip.h")).read()
    assert ctypes.sizeof(backend._CombineColumn) == 56 and "pmi_combine_column" in header


def test_goldens_regenerate():
    """The committed combine_cases.npz is what make_goldens_combine.py mints from the reference tree today."""
    if not os.path.isfile(mk.POSTPROCESS_PY):
        pytest.skip("reference tree not present")
    ref = mk.load_reference()
    combine = mk.combine_cases()
    assert list(combine) == COMBINE
    for name, cols in combine.items():
        p = "combine/" + name + "/"
        assert all(mk.same(v, G[p + "in_" + c]) for c, v in cols.items())
        assert_table(ref["cluster_combine"](pd.DataFrame(cols)), p)
    dist = mk.dist_cases(ref, combine)
    assert list(dist) == DIST
    for name, (cols, pixelsize) in dist.items():
        p = "dist/" + name + "/"
        assert all(mk.same(v, G[p + "in_" + c]) for c, v in cols.items())
        assert_table(ref["cluster_combine_dist"](pd.DataFrame(cols), pixelsize), p)
    assert json.loads(str(G["signatures"])) == {n: str(inspect.signature(ref[n])) for n in mk.NAMES}
