"""GPU tier: the cluster centers on the device (picasso_amd/clusterer.py find_cluster_centers, csrc/centers.hip)
against the reference's recorded tables (tests/golden/centers_cases.npz) and the test-side restatement
(tests/golden/_centers_restate.py).  Every column is compared in bits on every row; ``convexhull`` alone, which the
reference gets from Qhull's sum in another order, may differ by one float32 unit in the last place."""
import json
import sys

import numpy as np
import pandas as pd
import pytest

from conftest import GOLDEN, golden

sys.path.insert(0, GOLDEN)
import _centers_restate as rs  # noqa: E402

from picasso_amd import backend, clusterer  # noqa: E402
from test_centers_host import case, same, within_one_ulp  # noqa: E402

pytestmark = pytest.mark.gpu
CASES = [str(c) for c in golden("centers_cases")["case_names"]]


@pytest.fixture(scope="module")
def g():
    return golden("centers_cases")


def assert_centers(got: pd.DataFrame, want: dict, label):
    """``want``: column -> array, in the reference's order."""
    assert list(got.columns) == list(want), label
    assert [str(got[c].dtype) for c in got.columns] == [str(v.dtype) for v in want.values()], label
    assert isinstance(got.index, pd.RangeIndex) and got.index.start == 0 and got.index.step == 1, label
    assert len(got) == len(want["group"]), label
    for c, v in want.items():
        if c == "convexhull":
            differ = int((got[c].to_numpy().view(np.uint32) != v.view(np.uint32)).sum())
            print(f"{label}: convexhull differs in bits on {differ} of {len(v)} clusters")
            assert within_one_ulp(got[c].to_numpy(), v), (label, c)
        else:
            assert same(got[c].to_numpy(), v), (label, c)


@pytest.mark.parametrize("name", CASES)
def test_centers_equal_the_reference(g, name):
    p, cols, pixelsize = case(g, name)
    locs = pd.DataFrame(cols)
    before = locs.copy()
    got = clusterer.find_cluster_centers(locs, pixelsize)
    assert_centers(got, {str(c): g[p + "out_" + str(c)] for c in g[p + "columns"]}, name)
    assert locs.equals(before)


@pytest.mark.parametrize("name", CASES)
def test_group_order_is_the_stable_argsort(g, name):
    p, cols, pixelsize = case(g, name)
    groups = backend.CenterGroups(cols["group"])
    order = np.argsort(cols["group"], kind="stable")
    assert np.array_equal(groups.order(), order)
    assert np.array_equal(groups.unique, np.unique(cols["group"]))
    assert np.array_equal(groups.n_locs, np.unique(cols["group"], return_counts=True)[1])
    n_events, got_order, group_s = clusterer._count_binding_events(cols["group"], cols["frame"])
    assert np.array_equal(got_order, order) and np.array_equal(group_s, cols["group"][order])
    assert np.array_equal(n_events, g[p + "out_n_events"])


def test_nan_coordinate_raises_as_the_reference(g):
    edges = json.loads(str(g["edges"]))
    assert edges["nan_x"] == {"raises": "ValueError", "message": "Points cannot contain NaN"}
    cols = {str(c): g["nan_x/in_" + str(c)] for c in g["nan_x/in_columns"]}
    with pytest.raises(ValueError, match="Points cannot contain NaN"):
        clusterer.find_cluster_centers(pd.DataFrame(cols))


def test_clustered_blinking_sites_equal_the_restatement():
    """cluster() on about 2e4 rows of about 500 blinking sites, then the centers, against the restatement on the
    same labels."""
    rng = np.random.default_rng(5)
    n_sites, per_site = 500, 40
    centres = rng.uniform(2, 126, (n_sites, 2))
    which = rng.permutation(np.repeat(np.arange(n_sites), per_site))
    n = len(which)
    cols = {"frame": rng.integers(0, 20000, n).astype(np.uint32),
            "x": (centres[which, 0] + rng.normal(0, 0.012, n)).astype(np.float32),
            "y": (centres[which, 1] + rng.normal(0, 0.012, n)).astype(np.float32)}
    for c, (lo, hi) in {"photons": (500, 9000), "sx": (0.8, 1.5), "sy": (0.8, 1.5), "bg": (5, 40),
                        "net_gradient": (3000, 20000)}.items():
        cols[c] = rng.uniform(lo, hi, n).astype(np.float32)
    clustered = clusterer.cluster(pd.DataFrame(cols), 0.04, 10, False, return_info=True)[0]
    assert len(clustered) > 15000 and clustered["group"].nunique() > 400
    got = clusterer.find_cluster_centers(clustered)
    want, order = rs.centers({c: clustered[c].to_numpy() for c in clustered.columns})
    assert_centers(got, want, "blinking sites")
