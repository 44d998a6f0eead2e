"""GPU tier: DBSCAN and the SMLM clusterer on the device (picasso_amd/clusterer.py, csrc/cluster.hip) against the
reference's recorded results (tests/golden/cluster_cases.npz) and the test-side restatement
(tests/golden/_cluster_restate.py).  Every comparison is on every row and is an equality."""
import json
import sys

import numpy as np
import pandas as pd
import pytest

from conftest import GOLDEN, golden

sys.path.insert(0, GOLDEN)
import _cluster_restate as rs  # noqa: E402

import picasso_amd  # noqa: E402
from picasso_amd import backend, clusterer  # noqa: E402

pytestmark = pytest.mark.gpu
CASES = [str(c) for c in golden("cluster_cases")["case_names"]]


@pytest.fixture(scope="module")
def g():
    return golden("cluster_cases")


def case(g, name):
    p = name + "/"
    kw = json.loads(str(g[p + "kwargs"]))
    cols = {str(c): g[p + "in_" + str(c)] for c in g[p + "in_columns"]}
    return p, kw, cols


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def assert_labels(got, want, label):
    assert got.dtype == np.int32 and got.shape == want.shape, label
    differ = np.flatnonzero(got != want)
    assert len(differ) == 0, f"{label}: {len(differ)} of {len(want)} labels differ, first rows {differ[:5]}: " \
                             f"{got[differ[:5]]} for {want[differ[:5]]}"


def assert_table(g, prefix, got: pd.DataFrame, info, cols, label):
    """Column for column, in dtype and bits: the kept rows of the input, group, and z after its two conversions."""
    assert list(got.columns) == [str(c) for c in g[prefix + "columns"]], label
    assert [str(got[c].dtype) for c in got.columns] == [str(d) for d in g[prefix + "dtypes"]], label
    index = g[prefix + "index"]
    assert np.array_equal(got.index.to_numpy(), index), label
    for c in got.columns:
        want = g[prefix + "col_" + c] if c in ("group", "z") else cols[c][index]
        assert same(got[c].to_numpy(), want), (label, c)
    want_info = json.loads(str(g[prefix + "info"]).replace("{version}", picasso_amd.__version__))
    assert info == want_info and list(info) == list(want_info), label
    assert all(type(info[k]) is type(want_info[k]) for k in info), label


@pytest.mark.parametrize("name", CASES)
def test_neighbour_counts_equal_the_restatement(g, name):
    p, kw, cols = case(g, name)
    for X in rs.points(cols, kw):
        got = backend.ClusterPoints(X).counts(kw["radius"])
        assert got.dtype == np.int32 and np.array_equal(got, rs.neighbour_counts(X, kw["radius"])), name


@pytest.mark.parametrize("name", CASES)
def test_cluster_labels_equal_the_reference(g, name):
    p, kw, cols = case(g, name)
    if not kw.get("cluster", True):
        assert p + "labels_cluster" not in g.files      # a DBSCAN-only case: the isotropic 3-D search
        return
    X = rs.points(cols, kw)[0]
    assert_labels(clusterer._cluster(X.copy(), kw["radius"], kw["min_locs"]), g[p + "labels_cluster"], name)
    with_fa = clusterer._cluster(X.copy(), kw["radius"], kw["min_locs"], pd.Series(cols["frame"]))
    assert_labels(with_fa, g[p + "labels_cluster_fa"], name + " with frame analysis")
    labels = g[p + "labels_cluster"].copy()
    again = clusterer.frame_analysis(labels, cols["frame"])
    assert again is labels
    assert_labels(again, g[p + "labels_cluster_fa"], name + " frame_analysis()")


@pytest.mark.parametrize("name", CASES)
def test_dbscan_labels_equal_the_reference(g, name):
    p, kw, cols = case(g, name)
    X = rs.points(cols, kw)[1]
    assert_labels(clusterer._dbscan(X.copy(), kw["radius"], kw["min_samples"], kw["db_min_locs"]), g[p + "labels_dbscan"], name)
    assert_labels(clusterer._dbscan(X.copy(), kw["radius"], kw["min_samples"]), g[p + "labels_dbscan_all"], name + " all")


@pytest.mark.parametrize("name", CASES)
def test_cluster_and_dbscan_tables_equal_the_reference(g, name):
    p, kw, cols = case(g, name)
    z_kw = {k: kw[k] for k in ("radius_z", "pixelsize") if k in kw}
    locs = pd.DataFrame(cols)
    before = locs.copy()
    if kw.get("cluster", True):
        for fa in (False, True):
            got, info = clusterer.cluster(locs, kw["radius"], kw["min_locs"], fa, return_info=True, **z_kw)
            assert_table(g, p + f"cluster_fa{int(fa)}_", got, info, cols, f"{name} cluster fa={fa}")
        with pytest.warns(DeprecationWarning):
            only = clusterer.cluster(locs, kw["radius"], kw["min_locs"], False, **z_kw)
        assert isinstance(only, pd.DataFrame) and np.array_equal(only.index.to_numpy(), g[p + "cluster_fa0_index"])
    got, info = clusterer.dbscan(locs, kw["radius"], kw["min_samples"], kw["db_min_locs"], return_info=True, **z_kw)
    assert_table(g, p + "dbscan_", got, info, cols, f"{name} dbscan")
    assert locs.equals(before)


def _check_against_restatement(X, frame, radius, min_locs, min_samples, label):
    got = clusterer._cluster(X, radius, min_locs)
    assert_labels(got, rs.cluster(X, radius, min_locs), label + " _cluster")
    got_fa = clusterer._cluster(X, radius, min_locs, pd.Series(frame))
    assert_labels(got_fa, rs.frame_analysis(got, frame), label + " _cluster, frame analysis")
    db = clusterer._dbscan(X, radius, min_samples, min_locs)
    assert_labels(db, rs.dbscan(X, radius, min_samples, min_locs), label + " _dbscan")
    return got, got_fa, db


def test_bench_scale_table_equals_the_restatement():
    """The table of bench.py's movie (10 000 frames of 512 x 512, 116 emitters per frame, about 1e6 rows), localized here."""
    import torch
    from picasso_amd import synth
    cam = {"Baseline": 100.0, "Sensitivity": 1.0, "Gain": 1.0}
    movie = synth.simulate_movie(10000, 512, 512, emitters_per_frame=116, device="cuda:0")
    torch.cuda.synchronize()
    table = backend.localize_mle_device(movie.data_ptr(), np.uint16, tuple(movie.shape), 7, 5000, cam)
    del movie
    torch.cuda.empty_cache()
    n = len(table["frame"])
    assert n > 900_000
    X = np.stack([np.asarray(table["x"]), np.asarray(table["y"])], axis=1)
    assert X.dtype == np.float32
    got, _, db = _check_against_restatement(X, np.asarray(table["frame"]), 1.0, 5, 5, "bench scale")
    assert got.max() > 100 and db.max() > 100


def blinking_sites(n_sites=25000, per_site=40, n_frames=20000, seed=11):
    rng = np.random.default_rng(seed)
    centres = rng.uniform(2, 1022, (n_sites, 2))
    which = rng.permutation(np.repeat(np.arange(n_sites), per_site))
    X = centres[which] + rng.normal(0, 0.012, (len(which), 2))
    start = rng.integers(0, n_frames, n_sites)
    frame = (start[which] + rng.integers(0, np.where(which % 3 == 0, 300, n_frames), len(which))) % n_frames
    return X, frame.astype(np.uint32)


def test_blinking_sites_equal_the_restatement():
    """1e6 rows of sites that blink, a third of them only within 300 frames: float64, then float32."""
    X, frame = blinking_sites()
    assert len(X) == 1_000_000
    got, got_fa, _ = _check_against_restatement(X, frame, 0.04, 10, 8, "blinking sites")
    assert len(np.unique(got)) > 20000 and 1000 < len(np.unique(got_fa)) < len(np.unique(got))
    _check_against_restatement(X.astype(np.float32), frame, 0.04, 10, 8, "blinking sites, float32")


def test_dense_component_equals_the_restatement():
    """A fiducial: 6000 rows within one radius, between ordinary sites and a 3-D copy of the same."""
    rng = np.random.default_rng(12)
    X, frame = blinking_sites(2000, 40, 5000, seed=13)
    fid = np.array([300.0, 300.0]) + rng.normal(0, 0.004, (6000, 2))
    X = np.concatenate([X, fid])
    frame = np.concatenate([frame, rng.integers(0, 5000, 6000).astype(np.uint32)])
    order = rng.permutation(len(X))
    X, frame = X[order], frame[order]
    got, _, db = _check_against_restatement(X, frame, 0.04, 10, 8, "dense component")
    assert np.bincount(got[got >= 0]).max() >= 6000 and np.bincount(db[db >= 0]).max() >= 6000
    X3 = np.concatenate([X, rng.normal(0, 0.01, (len(X), 1))], axis=1)
    _check_against_restatement(X3, frame, 0.04, 10, 8, "dense component, 3-D")
