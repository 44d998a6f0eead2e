"""GPU tier of the cluster areas (picasso_amd/clusterer.py cluster_areas / test_subclustering, csrc/areas.hip): equal to
the reference's recorded tables (tests/golden/areas_cases.npz) and to the restatement (tests/golden/_areas_restate.py)
in every value; the blurred image equal in every float64 bit on the LDS path and on the scratch path."""
import builtins
import json
import sys

import numpy as np
import pandas as pd
import pytest

from conftest import GOLDEN, golden

sys.path.insert(0, GOLDEN)
import _areas_restate as rs  # noqa: E402
import make_goldens_areas as mk  # noqa: E402

from picasso_amd import backend, clusterer  # noqa: E402

pytestmark = pytest.mark.gpu

G = golden("areas_cases")
CASES = [str(c) for c in G["case_names"]]
MOLS = [str(c) for c in G["mol_names"]]
EDGES = json.loads(str(G["edges"]))
INFO = [{"Pixelsize": int(G["pixelsize"])}]
MOL_INFO = [{"Pixelsize": int(G["mol_pixelsize"])}]


def case(name, prefix=""):
    p = prefix + name + "/"
    return p, {str(c): G[p + "in_" + str(c)] for c in G[p + "in_columns"]}


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def images_of(cols):
    """The package's own steps up to the images: (AreaImages, the median precision)."""
    lp = rs.median_lp(cols)
    names = ["x", "y"] + (["z"] if "z" in cols else [])
    groups = backend.CenterGroups(cols["group"])
    return backend.AreaImages(groups, [cols[c] for c in names], INFO[0]["Pixelsize"], lp / 2, lp / 2 * 2.5), lp


@pytest.mark.parametrize("name", CASES)
def test_cluster_areas_equals_the_reference(name):
    p, cols = case(name)
    seen = []
    res = clusterer.cluster_areas(pd.DataFrame(cols), INFO, seen.append)
    assert list(res.columns) == [str(c) for c in G[p + "columns"]]
    assert [str(d) for d in res.dtypes] == [str(d) for d in G[p + "dtypes"]]
    assert isinstance(res.index, pd.RangeIndex) and len(res) == int(G[p + "n_rows"])
    for c in res.columns:
        differ = np.flatnonzero(res[c].to_numpy() != G[p + "out_" + c])
        assert same(res[c].to_numpy(), G[p + "out_" + c]), (name, c, differ[:5], res[c].to_numpy()[differ[:5]],
                                                            G[p + "out_" + c][differ[:5]])
    assert seen == list(range(1, len(res) + 1))


def test_edges_as_the_reference_recorded_them():
    inputs = mk.edge_inputs({n: case(n)[1] for n in ("sites2d_f32", "sites3d")})
    for name, (cols, info) in inputs.items():
        want = EDGES[name]
        if "raises" in want:
            with pytest.raises(getattr(builtins, want["raises"])) as err:
                clusterer.cluster_areas(pd.DataFrame(cols), info, lambda i: None)
            assert str(err.value) == want["message"], name
        else:
            res = clusterer.cluster_areas(pd.DataFrame(cols), info, lambda i: None)
            assert [list(res.columns), [str(d) for d in res.dtypes], len(res)] == [want["returns"], want["dtypes"], want["rows"]]
            assert [float(v) for v in res.iloc[:, 1].to_numpy()[:8]] == want["values"]


@pytest.mark.parametrize("name", ["lds2d", "lds3d", "sites3d", "edges2d_f32", "edges3d_f64", "one_rows2d", "one_rows3d"])
def test_blurred_image_bits_on_both_paths(name):
    """The blurred image of every group that has bins equals the restatement's in every bit pattern, on the path its size
    gives it and with every image forced through the global scratch; the three boundary images and the single-bin images
    of one-row groups are among them."""
    _, cols = case(name)
    images, lp = images_of(cols)
    bound = backend.AREAS_LDS_BINS
    sizes = set()
    for g in range(images.groups.n_groups):
        X = rs.points(cols, np.flatnonzero(cols["group"] == images.groups.unique[g]), INFO[0]["Pixelsize"])
        want = rs.cluster_image(X, lp)
        assert want.shape == images.shape(g), (name, g)
        if want.size == 0:
            assert images.bins[g] == 0
            continue
        own_area, own = images.areas(image_of=g)
        forced_area, forced = images.areas(image_of=g, force_scratch=True)
        assert same(own, want), (name, g, want.shape, int((own.view(np.uint64) != want.view(np.uint64)).sum()))
        assert same(forced, want), (name, g, want.shape)
        assert same(own_area, forced_area)
        sizes.add(int(images.bins[g]))
    if name.startswith("lds"):
        assert sizes == {bound - 1, bound, bound + 1}
    elif name.startswith("one_rows"):
        assert 1 in sizes
    else:
        assert min(sizes) <= bound


def random_table(seed, dims, dtype):
    """300 groups of 1 to 60 rows and 3 groups of 2 000 rows, rows shuffled."""
    rng = np.random.default_rng(seed)
    sizes = np.r_[rng.integers(1, 61, 300), [2000] * 3]
    which = rng.permutation(np.repeat(np.arange(len(sizes)), sizes))
    centre = rng.uniform(5, 250, (len(sizes), 3))
    sigma = rng.uniform(0.01, 0.06, len(sizes))
    n = len(which)
    cols = {"x": (centre[which, 0] + rng.normal(0, 1, n) * sigma[which]).astype(dtype),
            "y": (centre[which, 1] + rng.normal(0, 1, n) * sigma[which]).astype(dtype)}
    if dims == 3:
        cols["z"] = (centre[which, 2] * 4 - 500 + rng.normal(0, 1, n) * sigma[which] * 200).astype(dtype)
    cols["lpx"] = rng.uniform(0.01, 0.05, n).astype(np.float32)
    cols["lpy"] = rng.uniform(0.01, 0.05, n).astype(np.float32)
    cols["group"] = (which * 2 - 1).astype(np.int32)
    return cols


@pytest.mark.parametrize("dims, dtype", [(2, np.float32), (2, np.float64), (3, np.float32), (3, np.float64)])
def test_random_tables_equal_the_restatement(dims, dtype):
    cols = random_table(100 * dims + np.dtype(dtype).itemsize, dims, dtype)
    key, groups, want = rs.areas(cols, INFO)
    res = clusterer.cluster_areas(pd.DataFrame(cols), INFO, lambda i: None)
    assert list(res.columns) == ["group", key] and len(res) == 303
    assert same(res["group"].to_numpy(), groups)
    differ = np.flatnonzero(res[key].to_numpy() != want)
    assert same(res[key].to_numpy(), want), (len(differ), differ[:5], res[key].to_numpy()[differ[:5]], want[differ[:5]])


def test_progress_sees_every_group_in_order(capsys):
    _, cols = case("groups300")
    seen = []
    res = clusterer.cluster_areas(pd.DataFrame(cols), INFO, seen.append)
    assert seen == list(range(1, 301)) and len(res) == 300
    quiet = clusterer.cluster_areas(pd.DataFrame(cols), INFO)      # None: the console bar
    assert same(quiet.iloc[:, 1].to_numpy(), res.iloc[:, 1].to_numpy())


@pytest.mark.parametrize("name", MOLS)
def test_subclustering_equals_the_reference(name):
    p, cols = case(name, "mols/")
    close, far = clusterer.test_subclustering(pd.DataFrame(cols), MOL_INFO)
    assert same(close, G[p + "out_clustered"]) and same(far, G[p + "out_sparse"])
    again = clusterer.test_subclustering(pd.DataFrame(cols), MOL_INFO, clustering_dist=25.000001, sparse_dist=80.000001)
    assert len(again[0]) == len(close) + (4 if "z" in cols else 2) and len(again[1]) == len(far) - 2


def test_memory_error_names_the_group():
    """The cap, from the host check alone: the edge counts of a two-row group at a tiny precision, as NumPy's arange
    counts them."""
    x, y = np.float64([10.0, 10.5]), np.float64([20.0, 20.25])
    lp = np.float32(1e-5)
    lens = [[len(rs.arange(np.float64(1.0), np.float64(1.0) + lp / 2, lp / 2))] * 2,
            [int(np.ceil((v.max() + lp / 2 - v.min()) / (lp / 2))) for v in (x, y)]]
    with pytest.raises(MemoryError, match="group 7: .* exceeds the limit"):
        backend.areas_bins(np.array([3, 7]), lens)
