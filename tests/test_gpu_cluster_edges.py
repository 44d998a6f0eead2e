"""GPU tier of the clusterer's edge cases: DBSCAN and the SMLM clusterer on the device (picasso_amd/clusterer.py,
csrc/cluster.hip) against the reference's recorded labels (tests/golden/cluster_edge_cases.npz) and the test-side
restatement (tests/golden/_cluster_restate.py), on tables of at most 3000 rows that sit where the kernels' cell sort,
candidate ranges, pointer jumping, block guards and frame thresholds can go wrong.  Every comparison is on every row
and is an equality."""
import builtins
import json
import sys

import numpy as np
import pandas as pd
import pytest

from conftest import GOLDEN, golden

sys.path.insert(0, GOLDEN)
import _cluster_restate as rs  # noqa: E402

from picasso_amd import backend, clusterer  # noqa: E402

pytestmark = pytest.mark.gpu
CASES = [str(c) for c in golden("cluster_edge_cases")["case_names"]]
HAIR = 1.0 + 1.0 / 65536.0                  # the cells of csrc/cluster.hip have the side radius * HAIR
CAP = {2: 2**31 - 2, 3: 2**21 - 2}          # and this highest coordinate


@pytest.fixture(scope="module")
def g():
    return golden("cluster_edge_cases")


def case(g, name):
    """(prefix, kwargs, columns): a case reads its own table, or the first ``rows`` rows of the one it names."""
    p = name + "/"
    kw = json.loads(str(g[p + "kwargs"]))
    t = kw.get("table", name) + "/"
    cols = {str(c): g[t + "in_" + str(c)][:kw.get("rows")] for c in g[t + "in_columns"]}
    return p, kw, cols


def assert_labels(got, want, label):
    assert got.dtype == np.int32 and got.shape == want.shape, label
    differ = np.flatnonzero(got != want)
    assert len(differ) == 0, f"{label}: {len(differ)} of {len(want)} labels differ, first rows {differ[:5]}: " \
                             f"{got[differ[:5]]} for {want[differ[:5]]}"


def assert_as_recorded(g, key, name, call):
    """The recorded labels, row for row; where the reference raised, the same exception type."""
    if key in g.files:
        assert_labels(call(), g[key], name)
        return
    raised = json.loads(str(g["edges"]))[f"{name} {key.split('/')[1]}"]["raises"]
    with pytest.raises(getattr(builtins, raised)):
        call()


@pytest.mark.parametrize("name", CASES)
def test_neighbour_counts_equal_the_restatement(g, name):
    p, kw, cols = case(g, name)
    X = rs.points(cols, kw)[0]
    got = backend.ClusterPoints(X).counts(kw["radius"])
    want = rs.neighbour_counts(X, kw["radius"])
    assert got.dtype == np.int32 and got.shape == want.shape
    differ = np.flatnonzero(got != want)
    assert len(differ) == 0, f"{name}: {len(differ)} of {len(want)} counts differ, first rows {differ[:5]}: " \
                             f"{got[differ[:5]]} for {want[differ[:5]]}"


@pytest.mark.parametrize("name", CASES)
def test_cluster_labels_equal_the_reference(g, name):
    p, kw, cols = case(g, name)
    X, r, min_locs = rs.points(cols, kw)[0], kw["radius"], kw["min_locs"]
    assert_as_recorded(g, p + "labels_cluster", name, lambda: clusterer._cluster(X.copy(), r, min_locs))
    assert_as_recorded(g, p + "labels_cluster_fa", name + " with frame analysis",
                       lambda: clusterer._cluster(X.copy(), r, min_locs, pd.Series(cols["frame"])))
    if p + "labels_cluster" in g.files and p + "labels_cluster_fa" in g.files:
        labels = g[p + "labels_cluster"].copy()
        again = clusterer.frame_analysis(labels, cols["frame"])
        assert again is labels
        assert_labels(again, g[p + "labels_cluster_fa"], name + " frame_analysis()")


@pytest.mark.parametrize("name", CASES)
def test_dbscan_labels_equal_the_reference(g, name):
    p, kw, cols = case(g, name)
    X, r = rs.points(cols, kw)[1], kw["radius"]
    assert_as_recorded(g, p + "labels_dbscan", name,
                       lambda: clusterer._dbscan(X.copy(), r, kw["min_samples"], kw["db_min_locs"]))
    assert_as_recorded(g, p + "labels_dbscan_all", name + " all", lambda: clusterer._dbscan(X.copy(), r, kw["min_samples"]))


@pytest.mark.parametrize("n_frames", [1000, 1013])
def test_frame_analysis_kernel_equals_the_rule(g, n_frames):
    """pmi_cluster_frame_analysis_dev on its own, on ids that come from labels with gaps (3, 7, 19, ... and -1),
    against the rule written out: per id the count, the exact integer sum over the count, the fullest of the 20 bins
    of np.histogram, and the three comparisons."""
    p, kw, cols = case(g, f"fa_thresholds_{n_frames}")
    frame, recorded = cols["frame"], g[p + "labels_cluster"].astype(np.int64)
    labels = np.where(recorded < 0, -1, 4 * recorded * recorded + 3).astype(np.int32)
    values, ids = np.unique(labels, return_inverse=True)
    ids = ids.reshape(-1)
    assert values[0] == -1 and {3, 7} <= set(values) and values.max() > 7000 and (np.diff(values) > 1).sum() > 15
    lowest, highest, edges = 0.2 * n_frames, 0.8 * n_frames, np.linspace(0, n_frames, 21)
    want = np.ones(len(values), np.int32)
    for k in range(len(values)):
        f = frame[ids == k]
        mean = int(f.astype(np.int64).sum()) / len(f)
        fullest = np.histogram(f, bins=edges)[0].max()
        want[k] = not (mean < lowest or mean > highest or fullest > 0.8 * len(f))
    assert 8 <= want.sum() <= len(want) - 8
    got = backend.cluster_frame_analysis(ids.astype(np.int32), frame, len(values), lowest, highest, edges)
    assert got.dtype == np.int32 and got.shape == want.shape
    assert np.array_equal(got, want), f"ids {np.flatnonzero(got != want)} (labels {values[got != want]}): {got[got != want]}"
    through = clusterer.frame_analysis(labels.copy(), frame)
    assert_labels(through, np.where(want[ids] == 1, labels, -1).astype(np.int32), "frame_analysis() on labels with gaps")


def _check_against_restatement(X, frame, radius, min_locs, min_samples, label):
    counts = backend.ClusterPoints(X).counts(radius)
    assert counts.dtype == np.int32 and np.array_equal(counts, rs.neighbour_counts(X, radius)), label + " counts"
    got = clusterer._cluster(X, radius, min_locs)
    assert_labels(got, rs.cluster(X, radius, min_locs), label + " _cluster")
    got_fa = clusterer._cluster(X, radius, min_locs, pd.Series(frame))
    assert_labels(got_fa, rs.frame_analysis(got, frame), label + " _cluster, frame analysis")
    db = clusterer._dbscan(X, radius, min_samples, min_locs)
    assert_labels(db, rs.dbscan(X, radius, min_samples, min_locs), label + " _dbscan")
    return got, db


@pytest.mark.parametrize("name", ["clamp_3d", "clamp_2d"])
def test_mirrored_clamp_tables_equal_the_restatement(g, name):
    """The clamp tables mirrored through their centre: the site of the far corner now defines the lower corner, the
    site of the lower corner is clamped on every axis, and most of the table lies in clamped cells."""
    p, kw, cols = case(g, name)
    X = rs.points(cols, kw)[0]
    X = X.min(axis=0) + X.max(axis=0) - X
    dims, side = X.shape[1], kw["radius"] * HAIR
    u = (X - X.min(axis=0)) / side
    assert ((X.max(axis=0) - X.min(axis=0)) / side + 2 > CAP[dims]).all()
    assert (u >= CAP[dims]).any(axis=1).sum() > len(X) // 2 and (u >= CAP[dims]).all(axis=1).sum() >= 30
    got, db = _check_against_restatement(X, cols["frame"], kw["radius"], kw["min_locs"], kw["min_samples"], name + " mirrored")
    assert got.max() >= 20 and db.max() >= 20


def test_line_in_alternating_row_order_equals_the_restatement(g):
    """The line's rows taken from both ends in turn (0, n - 1, 1, n - 2, ...): neighbours in space lie up to n rows apart,
    and the chains of maxima run inwards from both ends."""
    p, kw, cols = case(g, "line_asc")
    n = len(cols["x"])
    order = np.empty(n, np.int64)
    order[0::2], order[1::2] = np.arange((n + 1) // 2), n - 1 - np.arange(n // 2)
    X = rs.points(cols, kw)[0][order]
    assert int(rs.smlm_parts(X, kw["radius"], kw["min_locs"])["chained"].sum()) >= 2900
    got, db = _check_against_restatement(X, cols["frame"][order], kw["radius"], kw["min_locs"], kw["min_samples"], "line, alternating")
    assert (got >= 0).all() and (db == 0).all()
