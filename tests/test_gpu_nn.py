"""GPU tier of the nearest-neighbour distances (csrc/knn.hip): every golden case of tests/golden/nn_cases.npz through
``postprocess.nn_analysis`` and ``spinna.get_NN_dist`` in every bit, one table of 1e5 blinking-site rows against scipy's
KDTree computed here, and one ordered set answering two query sets."""
import numpy as np
import pytest
from scipy.spatial import KDTree

from conftest import golden

from picasso_amd import backend, postprocess, spinna

pytestmark = pytest.mark.gpu

CASES = [str(c) for c in golden("nn_cases")["case_names"]]


@pytest.fixture(scope="module")
def g():
    return golden("nn_cases")


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


@pytest.mark.parametrize("name", CASES)
def test_golden_case(g, name):
    p = name + "/"
    X1, k = g[p + "X1"], int(g[p + "nn_count"])
    X2 = X1 if p + "same" in g.files else g[p + "X2"]
    before = (X1.copy(), X2.copy())
    want = g[p + "nn_analysis"]
    nn = postprocess.nn_analysis(X1, X2, k)
    assert np.array_equal(nn, want) and same(nn, want)
    dist = spinna.get_NN_dist(X1, X2, k)
    assert dist.shape == tuple(g[p + "get_NN_dist_shape"]) and same(dist.reshape(want.shape), want)
    assert np.array_equal(before[0], X1) and np.array_equal(before[1], X2)


@pytest.fixture(scope="module")
def blinking_sites():
    """1e5 rows: 5000 sites in a 256 x 256 frame that blink 20 times each, 0.04 px apart; z within half a pixel."""
    rng = np.random.default_rng(2024)
    centres = np.concatenate([rng.uniform(0, 256, (5000, 2)), rng.uniform(-0.5, 0.5, (5000, 1))], axis=1)
    which = rng.permutation(np.repeat(np.arange(5000), 20))
    return centres[which] + rng.normal(0, 0.04, (100000, 3))


@pytest.mark.parametrize("dims,dtype", [(2, np.float32), (3, np.float64)])
def test_blinking_sites_against_scipy(blinking_sites, dims, dtype):
    X = np.ascontiguousarray(blinking_sites[:, :dims].astype(dtype))
    want = KDTree(X).query(X, k=5)[0][:, 1:]
    got = postprocess.nn_analysis(X, X, 4)
    assert got.shape == (100000, 4) and np.array_equal(got, want) and same(got, want)


def test_one_order_serves_two_query_sets(blinking_sites):
    rng = np.random.default_rng(9)
    X2 = blinking_sites[:30000, :2]
    first = blinking_sites[30000:50000, :2]
    second = rng.uniform(-50, 300, (7001, 2))
    index = backend.KnnIndex(X2, 3)
    a, b = index.query(first, 3), index.query(second, 3)
    assert same(a, postprocess.nn_analysis(first, X2, 3)) and same(b, postprocess.nn_analysis(second, X2, 3))
    assert same(index.query(first, 3), a)                                   # and again, after the other set
    assert same(index.query(second, 1)[:, 0], postprocess.nn_analysis(second, X2, 1))       # another k on the same order
    assert same(b, KDTree(X2).query(second, k=3)[0])


def test_device_tensor_path_and_its_checks(blinking_sites):
    """Points already on the device, with their host box: the bits of the host path; a tensor the library would misread
    (float32, strided, four columns, on the host) and a malformed box are refused."""
    import torch
    X2 = np.ascontiguousarray(blinking_sites[:5001])
    queries = np.ascontiguousarray(blinking_sites[60000:62001])
    box = (X2[:, :2].min(axis=0), X2[:, :2].max(axis=0))
    d_x2, d_q = torch.from_numpy(X2).cuda(), torch.from_numpy(queries).cuda()
    index = backend.KnnIndex(d_x2, 4, box)
    assert same(index.query_device(d_q, 4).cpu().numpy(), backend.KnnIndex(X2, 4).query(queries, 4))
    wide = torch.zeros((10, 6), dtype=torch.float64, device="cuda")
    for bad in (d_x2.float(), wide[:, :3], wide[:, :4].contiguous(), torch.from_numpy(X2), d_x2[:, 0]):
        with pytest.raises(ValueError, match="contiguous float64 device tensor"):
            backend.KnnIndex(bad, 4, box)
    with pytest.raises(ValueError, match="the box is"):
        backend.KnnIndex(d_x2, 4, (box[0], np.zeros(3)))
    for bad in (d_q.float(), d_q[:, :2], d_q[:, :2].contiguous(), torch.from_numpy(queries)):
        with pytest.raises(ValueError, match="queries must be"):
            index.query_device(bad, 4)
