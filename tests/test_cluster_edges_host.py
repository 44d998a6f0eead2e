"""CPU tier of the clusterer's edge cases (tests/golden/cluster_edge_cases.npz, minted by
tests/golden/make_goldens_cluster_edges.py): the test-side restatement (tests/golden/_cluster_restate.py) reproduces
every label array the reference recorded, and the cases hold what they were built for: clamped cell coordinates with
clusters across the clamp, chains of maxima as long as the table, border rows at exactly the radius from two clusters,
and sites on either side of every threshold of the frame analysis."""
import json
import sys

import numpy as np
import pytest

from conftest import GOLDEN, golden

sys.path.insert(0, GOLDEN)
import _cluster_restate as rs  # noqa: E402

CASES = [str(c) for c in golden("cluster_edge_cases")["case_names"]]
LABELS = ("labels_cluster", "labels_cluster_fa", "labels_dbscan", "labels_dbscan_all")
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


def points(g, name):
    _, kw, cols = case(g, name)
    return rs.points(cols, kw)[0]


def test_the_fixture_holds_every_family(g):
    families = ["line_asc", "line_desc", "lattice_rowmajor_2d", "lattice_rowmajor_3d", "offset_1e6", "offset_2p40",
                "offset_negative", "clamp_3d", "clamp_2d", "flat_x", "coincident", "one_cell", "tiny_radius", "border_exact",
                "fa_thresholds_1000", "fa_thresholds_1013", "extremes_0_1", "extremes_1_2", "extremes_401_401", "extremes_5_5"]
    assert CASES == families[:13] + [f"sizes_{n}" for n in (1, 2, 255, 256, 257, 511, 512, 513)] + families[16:] + families[13:16]
    assert json.loads(str(g["edges"])) == {}          # the reference raised on none of them
    for name in CASES:
        p, kw, cols = case(g, name)
        n = len(cols["x"])
        assert 1 <= n <= 3000 and cols["x"].dtype == np.float64 and all(len(v) == n for v in cols.values()), name
        assert all(g[p + k].dtype == np.int32 and g[p + k].shape == (n,) for k in LABELS), name
        if name in ("tiny_radius", "extremes_401_401"):
            assert all((g[p + k] == -1).all() for k in LABELS), name
        else:
            assert all((g[p + k] >= 0).any() for k in ("labels_cluster", "labels_dbscan", "labels_dbscan_all")), name
    assert [len(case(g, f"sizes_{n}")[2]["x"]) for n in (1, 2, 255, 256, 257, 511, 512, 513)] == [1, 2, 255, 256, 257, 511, 512, 513]
    assert case(g, "extremes_5_5")[1]["db_min_locs"] == 0 and len(case(g, "extremes_0_1")[2]["x"]) == 400
    assert g["fa_thresholds_1000/in_frame"].dtype == np.uint32 and g["fa_thresholds_1013/in_frame"].dtype == np.int64


@pytest.mark.parametrize("name", CASES)
def test_restatement_reproduces_the_reference_labels(g, name):
    p, kw, cols = case(g, name)
    for_cluster, for_dbscan = rs.points(cols, kw)
    got = rs.cluster(for_cluster, kw["radius"], kw["min_locs"])
    assert got.dtype == np.int32 and np.array_equal(got, g[p + "labels_cluster"])
    got = rs.cluster(for_cluster, kw["radius"], kw["min_locs"], cols["frame"])
    assert np.array_equal(got, g[p + "labels_cluster_fa"])
    got = rs.dbscan(for_dbscan, kw["radius"], kw["min_samples"], kw["db_min_locs"])
    assert got.dtype == np.int32 and np.array_equal(got, g[p + "labels_dbscan"])
    assert np.array_equal(rs.dbscan(for_dbscan, kw["radius"], kw["min_samples"]), g[p + "labels_dbscan_all"])


def test_lines_and_lattice_hold_long_chains(g):
    """A maximum without a fresh neighbour takes its label through a chain of lower maxima: nearly every row here."""
    for name, least in (("line_asc", 2900), ("line_desc", 2900), ("lattice_rowmajor_2d", 1000)):
        p, kw, cols = case(g, name)
        chained = int(rs.smlm_parts(rs.points(cols, kw)[0], kw["radius"], kw["min_locs"])["chained"].sum())
        assert chained >= least, (name, chained)
    a, d = case(g, "line_asc")[2], case(g, "line_desc")[2]
    assert np.array_equal(a["x"], d["x"][::-1]) and np.array_equal(np.diff(a["x"]), np.full(2999, 0.125))
    for name, shape in (("lattice_rowmajor_2d", (40, 40)), ("lattice_rowmajor_3d", (30, 30, 2))):
        X = points(g, name)
        want = np.stack([v.ravel() for v in np.meshgrid(*[np.arange(m) * 0.125 + 1 for m in shape], indexing="ij")], axis=1)
        assert np.array_equal(X, want), name


def test_offsets_are_exact(g):
    lat = points(g, "lattice_rowmajor_2d")
    for name, shift in (("offset_1e6", 1e6), ("offset_2p40", 2.0**40), ("offset_negative", -2.0**40 - 3)):
        X = points(g, name)
        assert len(X) == 1800 and np.array_equal(X[:1600] - shift, lat) and (X[:1600] * 8 % 1 == 0).all(), name
        assert (np.sign(X) == np.sign(shift)).all(), name


@pytest.mark.parametrize("name", ["clamp_3d", "clamp_2d"])
def test_clamp_cases_reach_past_the_highest_cell(g, name):
    p, kw, cols = case(g, name)
    X = rs.points(cols, kw)[0]
    dims, side = X.shape[1], kw["radius"] * HAIR
    lo, hi = X.min(axis=0), X.max(axis=0)
    assert ((hi - lo) / side + 2 > CAP[dims]).all()
    u = (X - lo) / side
    assert (u >= CAP[dims]).all(axis=1).sum() >= 30                  # a site clamped on every axis
    for key in ("labels_cluster", "labels_dbscan_all"):
        labels = g[p + key]
        for k in range(dims):
            clamped = u[:, k] >= CAP[dims]
            across = set(labels[clamped & (labels >= 0)]) & set(labels[~clamped & (labels >= 0)])
            assert across, (name, key, k)


def test_border_rows_lie_at_the_radius_from_two_clusters(g):
    p, kw, cols = case(g, "border_exact")
    X, r = rs.points(cols, kw)[1], kw["radius"]
    parts = rs.dbscan_parts(X, r, kw["min_samples"])
    border, labels = g[p + "border_rows"], g[p + "labels_dbscan_all"]
    assert len(border) == 6 and parts["border"][border].all() and parts["border"].sum() == 6
    where = []
    for b in border:
        d = X - X[b]
        at_r = np.flatnonzero((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] == r * r) & parts["core"])
        found = sorted(set(labels[at_r]))
        assert len(found) == 2 and labels[b] == found[0], (b, found, labels[b])
        first_core = sorted(int(np.flatnonzero(parts["core"] & (labels == c))[0]) for c in found)
        where.append(int(np.searchsorted(first_core, b)))
    assert where == [0, 1, 2, 0, 1, 2]                # before, between and after the clusters' lowest core rows
    left_first = [X[np.flatnonzero(parts["core"] & (labels == 2 * k))[0], 0] < X[border[k], 0] for k in range(6)]
    assert left_first.count(True) == 3                # and either side comes first


@pytest.mark.parametrize("n_frames", [1000, 1013])
def test_frame_thresholds_fall_on_both_sides(g, n_frames):
    """Every behaviour is one cluster before the frame analysis; the sites at a limit stay and their twins one frame
    or one row past it go.  0.2 * 1013 rounds above 1013 / 5 in float64, so there the site at the lower limit goes
    too and the one a frame inside stays; with 1000 frames both numbers are 200."""
    p, kw, cols = case(g, f"fa_thresholds_{n_frames}")
    frame, site, names = cols["frame"], g[p + "site"], [str(s) for s in g[p + "site_names"]]
    assert frame[-1] == frame.max() == n_frames - 1
    kept, size = {}, {}
    for k, s in enumerate(names):
        rows = site == k
        before, after = g[p + "labels_cluster"][rows], g[p + "labels_cluster_fa"][rows]
        assert rows.any() and before[0] >= 0 and (before == before[0]).all() and (after == after[0]).all(), s
        kept[s], size[s] = bool(after[0] >= 0), int(rows.sum())
    lo, hi = 0.2 * n_frames, 0.8 * n_frames
    mean = {s: int(frame[site == k].astype(np.int64).sum()) / size[s] for k, s in enumerate(names)}
    fullest = {s: int(np.histogram(frame[site == k], bins=np.linspace(0, n_frames, 21))[0].max()) for k, s in enumerate(names)}
    total = {s: int(frame[site == k].astype(np.int64).sum()) for k, s in enumerate(names)}
    assert size["mean_lo_at"] == size["mean_hi_at"] == 10
    assert total["mean_lo_at"] == 2 * n_frames and total["mean_hi_at"] == 8 * n_frames       # 0.2 and 0.8 n_frames, exactly
    assert total["mean_lo_past"] == 2 * n_frames - 1 and total["mean_lo_inside"] == 2 * n_frames + 1
    assert total["mean_hi_past"] == 8 * n_frames + 1
    assert (mean["mean_lo_at"] < lo) == (n_frames == 1013) and kept["mean_lo_at"] == (n_frames == 1000)
    assert kept["mean_lo_inside"] and kept["mean_hi_at"] and not kept["mean_lo_past"] and not kept["mean_hi_past"]
    for c in (5, 10, 15, 20, 25):
        at, past = f"bin80_at_{c}", f"bin80_past_{c}"
        assert size[at] == size[past] == c and fullest[at] * 5 == 4 * c and fullest[past] == fullest[at] + 1
        assert lo < mean[at] < hi and lo < mean[past] < hi and kept[at] and not kept[past], c
    assert fullest["on_edges"] == fullest["below_edge"] == 5 and kept["on_edges"] and kept["below_edge"]
    assert fullest["on_edges_full"] == 9 and not kept["on_edges_full"] and kept["plain"]
    assert (frame[site == names.index("last_frame")] == n_frames - 1).all() and not kept["last_frame"]
    if n_frames == 1000:
        on = frame[site == names.index("on_edges")]
        assert (on % 50 == 0).all()
