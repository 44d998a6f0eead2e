"""CPU tier of the clusterer (picasso_amd/clusterer.py, csrc/cluster.hip): the test-side restatement
(tests/golden/_cluster_restate.py) reproduces every label array the reference recorded
(tests/golden/cluster_cases.npz), the library exports the new entries, and the argument checks and warnings of
``cluster()`` / ``dbscan()`` that come before any device work behave as the reference's."""
import json
import sys
import warnings

import numpy as np
import pandas as pd
import pytest

from conftest import GOLDEN, golden

sys.path.insert(0, GOLDEN)
import _cluster_restate as rs  # noqa: E402

from picasso_amd import _lib, clusterer  # noqa: E402

CASES = [str(c) for c in golden("cluster_cases")["case_names"]]


@pytest.fixture(scope="module")
def g():
    return golden("cluster_cases")


def case(g, name):
    p = name + "/"
    kw = json.loads(str(g[p + "kwargs"]))
    cols = {str(c): g[p + "in_" + str(c)] for c in g[p + "in_columns"]}
    return p, kw, cols


@pytest.mark.parametrize("name", CASES)
def test_restatement_reproduces_the_reference_labels(g, name):
    p, kw, cols = case(g, name)
    for_cluster, for_dbscan = rs.points(cols, kw)
    if kw.get("cluster", True):
        got = rs.cluster(for_cluster, kw["radius"], kw["min_locs"])
        assert got.dtype == np.int32 and np.array_equal(got, g[p + "labels_cluster"])
        got = rs.cluster(for_cluster, kw["radius"], kw["min_locs"], cols["frame"])
        assert np.array_equal(got, g[p + "labels_cluster_fa"])
    got = rs.dbscan(for_dbscan, kw["radius"], kw["min_samples"], kw["db_min_locs"])
    assert got.dtype == np.int32 and np.array_equal(got, g[p + "labels_dbscan"])
    assert np.array_equal(rs.dbscan(for_dbscan, kw["radius"], kw["min_samples"]), g[p + "labels_dbscan_all"])


def test_cases_hold_the_hard_parts(g):
    """Counted with the restatement: chains of maxima, rows between fresh maxima, border rows, pairs at the radius."""
    chained = two_fresh = stale = border = 0
    for name in CASES:
        p, kw, cols = case(g, name)
        for_cluster, for_dbscan = rs.points(cols, kw)
        s = rs.smlm_parts(for_cluster, kw["radius"], kw["min_locs"])
        chained += int(s["chained"].sum())
        stale += int((s["lm"] & ~s["fresh"]).sum())
        two_fresh += int((s["n_fresh_neighbours"] >= 2).sum())
        border += int(rs.dbscan_parts(for_dbscan, kw["radius"], kw["min_samples"])["border"].sum())
    assert chained >= 100 and stale >= 50 and two_fresh >= 15 and border >= 100, (chained, stale, two_fresh, border)


def test_frame_analysis_of_one_cluster_on_the_host():
    early, spread = pd.Series(np.arange(10, 50)), pd.Series(np.arange(0, 1000, 25))
    burst = pd.Series(np.r_[np.full(36, 510), 5, 300, 700, 990])
    assert clusterer._frame_analysis(spread, 1000) == 1
    assert clusterer._frame_analysis(early, 1000) == 0 and clusterer._frame_analysis(burst, 1000) == 0


def test_abi_has_the_cluster_entries():
    lib = _lib.load()
    assert lib.pmi_version() >= 110
    for name in ("pmi_cluster_counts_dev", "pmi_cluster_smlm_dev", "pmi_cluster_dbscan_dev",
                 "pmi_cluster_frame_analysis_dev"):
        assert name in _lib.SYMBOLS and hasattr(lib, name)


def _locs3d():
    return pd.DataFrame({"frame": np.arange(4, dtype=np.uint32), "x": np.ones(4, np.float32),
                         "y": np.ones(4, np.float32), "z": np.zeros(4, np.float32)})


def test_cluster_argument_checks_and_warnings():
    with pytest.warns(DeprecationWarning, match="cluster will return both"):
        with pytest.raises(ValueError, match="pixel size and clustering radius in z"):
            clusterer.cluster(_locs3d(), 0.1, 2, False)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        with pytest.raises(ValueError, match="pixel size and clustering radius in z"):
            clusterer.cluster(_locs3d(), 0.1, 2, False, pixelsize=130, return_info=True)
        with pytest.raises(ValueError, match="pixel size and clustering radius in z"):
            clusterer.cluster(_locs3d(), 0.1, 2, False, radius_z=0.2, return_info=False)
        empty = pd.DataFrame({"frame": np.zeros(0, np.uint32), "x": np.zeros(0, np.float32), "y": np.zeros(0, np.float32)})
        with pytest.raises(ZeroDivisionError):
            clusterer.cluster(empty, 0.1, 2, False, return_info=True)


def test_dbscan_argument_checks_and_warnings():
    with pytest.warns(DeprecationWarning, match="dbscan will return both"):
        with pytest.raises(ValueError, match="pixel size must be specified"):
            clusterer.dbscan(_locs3d(), 0.1, 2)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        with pytest.raises(ValueError, match="pixel size must be specified"):
            clusterer.dbscan(_locs3d(), 0.1, 2, radius_z=0.2, return_info=True)


def test_edges_as_the_reference_recorded_them(g):
    """An empty table and coordinates that are not finite: what raises in the reference raises the same here, before
    any device work."""
    edges = json.loads(str(g["edges"]))
    empty2 = np.zeros((0, 2))
    bad = {"nan": np.array([[0.0, np.nan], [1.0, 1.0]]), "inf": np.array([[0.0, np.inf], [1.0, 1.0]])}
    assert edges["_cluster empty"] == {"returns": [], "dtype": "int32"}
    got = clusterer._cluster(empty2, 0.1, 3)
    assert got.dtype == np.int32 and got.shape == (0,)
    calls = {"_cluster empty frame": lambda: clusterer._cluster(empty2, 0.1, 3, pd.Series(np.zeros(0, np.uint32))),
             "_dbscan empty": lambda: clusterer._dbscan(empty2, 0.1, 3)}
    for k, X in bad.items():
        calls["_cluster " + k] = lambda X=X: clusterer._cluster(X, 0.1, 3)
        calls["_dbscan " + k] = lambda X=X: clusterer._dbscan(X, 0.1, 3)
    for what, call in calls.items():
        assert edges[what] == {"raises": "ValueError"}, what
        with pytest.raises(ValueError):
            call()


def test_extract_valid_labels_adds_group_and_drops_noise():
    locs = pd.DataFrame({"x": np.arange(5, dtype=np.float32)})
    out = clusterer.extract_valid_labels(locs, np.array([0, -1, 2, -1, 2], np.int32))
    assert list(out.index) == [0, 2, 4] and out["group"].dtype == np.int32 and list(locs["group"]) == [0, -1, 2, -1, 2]


def test_install_rebinds_the_clusterer_names():
    import types
    from picasso_amd import localize
    stub = types.SimpleNamespace(hdbscan="theirs")
    mods = {k: types.SimpleNamespace() for k in ("picasso_localize", "picasso_gaussmle", "picasso_gausslq", "picasso_zfit",
                                                 "picasso_imageprocess", "picasso_postprocess", "picasso_aim")}
    localize.install(picasso_render=types.SimpleNamespace(), picasso_clusterer=stub, **mods)
    for name in clusterer.CLUSTERER_NAMES:
        assert getattr(stub, name) is getattr(clusterer, name)
    assert stub.hdbscan == "theirs" and {"_cluster", "cluster", "_dbscan", "dbscan", "frame_analysis"} <= set(clusterer.CLUSTERER_NAMES)
