"""CPU tier of the cluster centers (picasso_amd/clusterer.py find_cluster_centers, csrc/centers.hip): the test-side
restatement (tests/golden/_centers_restate.py) reproduces every array the reference recorded
(tests/golden/centers_cases.npz), the library exports the new entries, ``install()`` rebinds the function, and the
checks that come before any device work behave as the reference's."""
import json
import sys

import numpy as np
import pandas as pd
import pytest

from conftest import GOLDEN, golden

sys.path.insert(0, GOLDEN)
import _centers_restate as rs  # noqa: E402

from picasso_amd import _lib, clusterer  # noqa: E402

CASES = [str(c) for c in golden("centers_cases")["case_names"]]
ULP = 2.0 ** -23      # of a float32 relative to its own magnitude, at most


@pytest.fixture(scope="module")
def g():
    return golden("centers_cases")


def case(g, name):
    p = name + "/"
    cols = {str(c): g[p + "in_" + str(c)] for c in g[p + "in_columns"]}
    pixelsize = int(g[p + "pixelsize"])
    return p, cols, (None if pixelsize < 0 else pixelsize)


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def within_one_ulp(got, want):
    """float32 arrays that differ by at most one unit in the last place, and not at all where ``want`` is 0.0."""
    got, want = np.asarray(got), np.asarray(want)
    if got.dtype != np.float32 or want.dtype != np.float32 or got.shape != want.shape:
        return False
    up, down = np.nextafter(want, np.float32(np.inf)), np.nextafter(want, np.float32(-np.inf))
    near = (got == want) | (got == up) | (got == down)
    return bool(near.all() and (got[want == 0] == 0).all())


@pytest.mark.parametrize("name", CASES)
def test_restatement_reproduces_the_reference(g, name):
    p, cols, pixelsize = case(g, name)
    got, order = rs.centers(cols, pixelsize, g[p + "out_convexhull"])
    assert list(got) == [str(c) for c in g[p + "columns"]]
    assert [str(v.dtype) for v in got.values()] == [str(d) for d in g[p + "dtypes"]]
    assert np.array_equal(order, np.argsort(cols["group"], kind="stable"))
    for c, v in got.items():
        if c == "convexhull":
            assert within_one_ulp(v, g[p + "out_" + c]), (name, c)
        else:
            assert same(v, g[p + "out_" + c]), (name, c)


def test_cases_hold_the_hard_parts(g):
    e = {c: g["edges2d/out_" + c] for c in [str(c) for c in g["edges2d/columns"]]}
    groups = list(e["group"])
    assert groups[0] < 0 and (np.diff(groups) > 1).any()
    one, two, dup, line = (groups.index(k) for k in (0, 2, 7, 9))
    assert e["n_locs"][one] == 1 and np.isnan(e["std_x"][one]) and e["convexhull"][one] == 0
    assert e["n_locs"][two] == 2 and e["convexhull"][two] == 0
    assert e["convexhull"][dup] == 0 and e["convexhull"][line] == 0 and e["n_events"][line] == 3
    assert e["n_events"][groups.index(100)] == 6 and g["edges2d/in_frame"].dtype == np.uint32
    assert np.isnan(g["edges2d/in_photons"]).sum() == 2 and np.isinf(g["edges2d/in_bg"]).sum() == 1
    assert "group_input" in e and g["groups300/n_rows"] == 300 and g["sites2d_f64/in_x"].dtype == np.float64
    cols = case(g, "large_coordinates")[1]
    big = cols["group"] == 6
    assert big.sum() == 5000
    plain = [np.float32(cols[c][big].astype(np.float64).sum() / 5000) for c in ("x", "y")]
    assert plain[0] != g["large_coordinates/out_x"][6] or plain[1] != g["large_coordinates/out_y"][6]
    assert set(json.loads(str(g["versions"]))) == {"pandas", "numpy", "scipy"}


def test_abi_has_the_centers_entries():
    lib = _lib.load()
    assert lib.pmi_version() >= 112
    for name in ("pmi_centers_order_dev", "pmi_centers_weights_dev", "pmi_centers_stats_dev", "pmi_centers_hull_dev"):
        assert name in _lib.SYMBOLS and hasattr(lib, name)


def test_install_rebinds_find_cluster_centers():
    import types
    from picasso_amd import localize
    stub = types.SimpleNamespace(hdbscan="theirs", find_cluster_centers="theirs")
    mods = {k: types.SimpleNamespace() for k in ("picasso_localize", "picasso_gaussmle", "picasso_gausslq", "picasso_zfit",
                                                 "picasso_imageprocess", "picasso_postprocess", "picasso_aim")}
    localize.install(picasso_render=types.SimpleNamespace(), picasso_clusterer=stub, **mods)
    assert stub.find_cluster_centers is clusterer.find_cluster_centers and stub.hdbscan == "theirs"
    assert {"find_cluster_centers", "_count_binding_events", "_cluster_convex_hulls", "_weighted_z_means"} \
        <= set(clusterer.CLUSTERER_NAMES)


def test_edges_as_the_reference_recorded_them(g):
    """What raises in the reference before any per-cluster work raises the same here, before any device work."""
    edges = json.loads(str(g["edges"]))
    assert edges["3d without pixelsize"]["raises"] == "ValueError"
    with pytest.raises(ValueError, match="pixel size must be specified"):
        clusterer.find_cluster_centers(pd.DataFrame(case(g, "sites3d")[1]))
    assert edges["empty"]["raises"] == "IndexError"
    empty = pd.DataFrame({c: v[:0] for c, v in case(g, "sites2d_f32")[1].items()})
    with pytest.raises(IndexError) as err:
        clusterer.find_cluster_centers(empty)
    assert str(err.value) == edges["empty"]["message"]
