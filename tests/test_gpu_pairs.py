"""GPU tier: local density, distance histogram and pair correlation on the device (picasso_amd/postprocess.py,
csrc/pairs.hip) against the reference's recorded results (tests/golden/pairs_cases.npz) and the test-side restatement
(tests/golden/_pairs_restate.py).  Every comparison is on every count and is an equality."""
import json
import sys

import numpy as np
import pandas as pd
import pytest

from conftest import GOLDEN, golden

sys.path.insert(0, GOLDEN)
import _pairs_restate as rs  # noqa: E402

from picasso_amd import backend, postprocess  # noqa: E402

pytestmark = pytest.mark.gpu
CASES = [str(c) for c in golden("pairs_cases")["case_names"]]


@pytest.fixture(scope="module")
def g():
    return golden("pairs_cases")


def case(g, name):
    p = name + "/"
    kw = json.loads(str(g[p + "kwargs"]))
    cols = {str(c): g[p + "in_" + str(c)] for c in g[p + "in_columns"]}
    info = [{k: kw[k] for k in ("Width", "Height", "Frames")}]
    return p, kw, cols, info


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def assert_counts(got, want, label):
    assert got.dtype == want.dtype and got.shape == want.shape, (label, got.dtype, got.shape, want.dtype, want.shape)
    differ = np.flatnonzero(got != want)
    assert len(differ) == 0, f"{label}: {len(differ)} of {len(want)} counts differ, first at {differ[:5]}: " \
                             f"{got[differ[:5]]} for {want[differ[:5]]}"


@pytest.mark.parametrize("name", CASES)
def test_block_order_equals_the_reference(g, name):
    p, kw, cols, info = case(g, name)
    b = rs.Blocks(cols, info[0], kw["radius"])
    x, y = cols["x"][b.kept], cols["y"][b.kept]
    table = backend.BlockTable(np.uint32(x / kw["radius"]), np.uint32(y / kw["radius"]), *g[p + "KL"])
    order = table.order()
    assert np.array_equal(order, g[p + "perm"]), name                       # np.lexsort([x_index, y_index]): stable
    keys = table.keys[:table.n].cpu().numpy()
    assert np.array_equal(keys >> 32, g[p + "y_index"]) and np.array_equal(keys & 0xffffffff, g[p + "x_index"])
    assert table.p == b.p


@pytest.mark.parametrize("name", CASES)
def test_local_density_equals_the_reference(g, name):
    p, kw, cols, info = case(g, name)
    locs = pd.DataFrame(cols)
    before = locs.copy()
    got = postprocess.compute_local_density(locs, info, kw["radius"])
    assert locs.equals(before)
    assert list(got.columns) == [str(c) for c in g[p + "out_columns"]] == list(cols) + ["density"]
    assert same(got.index.to_numpy(), g[p + "index"]), name
    assert_counts(got["density"].to_numpy(), g[p + "density"], name)
    for c in cols:
        assert same(got[c].to_numpy(), cols[c][g[p + "index"]]), (name, c)


@pytest.mark.parametrize("name", CASES)
def test_distance_histogram_and_pair_correlation_equal_the_reference(g, name):
    p, kw, cols, info = case(g, name)
    locs = pd.DataFrame(cols)
    before = locs.copy()
    assert_counts(postprocess.distance_histogram(locs, info, kw["bin_size"], kw["r_max"]), g[p + "dh"], name)
    if p + "pc_raises" in g.files:
        with pytest.raises(ValueError, match="broadcast"):
            postprocess.pair_correlation(locs, info, kw["bin_size"], kw["r_max"])
    else:
        lower, pc = postprocess.pair_correlation(locs, info, kw["bin_size"], kw["r_max"])
        assert same(lower, g[p + "bins_lower"]) and same(pc, g[p + "pc"]), name
    assert locs.equals(before)


def _check_against_restatement(cols, info, radius, bin_size, label, big_bins=None):
    locs = pd.DataFrame(cols)
    b, density = rs.local_density(cols, info, radius)
    got = postprocess.compute_local_density(locs, [info], radius)
    assert np.array_equal(got.index.to_numpy(), b.index), label
    assert_counts(got["density"].to_numpy(), density, label + " density")
    assert same(got["x"].to_numpy(), b.x) and same(got["photons"].to_numpy(), cols["photons"][b.index]), label
    dh = postprocess.distance_histogram(locs, [info], bin_size, radius)
    assert_counts(dh, rs.distance_histogram(cols, info, bin_size, radius), label + " histogram")
    if big_bins is not None:                                               # the path without LDS counters
        dh = postprocess.distance_histogram(locs, [info], big_bins, radius)
        assert len(dh) > 8192
        assert_counts(dh, rs.distance_histogram(cols, info, big_bins, radius), label + " histogram, many bins")
    return density, dh


def blinking_sites(n_sites, per_site, size, seed, dtype, on_border=False):
    rng = np.random.default_rng(seed)
    cx, cy = rng.uniform(0, size, n_sites), rng.uniform(0, size, n_sites)
    if on_border:                                                          # one site centred on each edge of the frame
        cx[0], cx[1], cy[2], cy[3] = 0, size, 0, size
    which = rng.permutation(np.repeat(np.arange(n_sites), per_site))
    n = len(which)
    x, y = cx[which] + rng.normal(0, 0.012, n), cy[which] + rng.normal(0, 0.012, n)
    return {"frame": rng.integers(0, 20000, n).astype(np.uint32), "x": x.astype(dtype), "y": y.astype(dtype),
            "photons": rng.uniform(500, 9000, n).astype(np.float32), "lpx": rng.uniform(0.005, 0.06, n).astype(np.float32)}


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_blinking_sites_equal_the_restatement(dtype):
    """1e5 rows of 2500 sites on 324 x 324 px (8100 x 8100 blocks); a site on each edge loses rows to the sanity filter."""
    cols = blinking_sites(2500, 40, 324, 21, dtype, on_border=True)
    assert len(cols["x"]) == 100_000
    info = {"Width": 324, "Height": 324, "Frames": 20000}
    density, dh = _check_against_restatement(cols, info, 0.04, 0.001, f"blinking sites {np.dtype(dtype).name}",
                                             big_bins=0.04 / 9000)
    assert 99_000 < len(density) < 100_000 and np.median(density) > 20 and dh.sum() > 1_000_000


def test_dense_patch_equals_the_restatement():
    """3000 rows inside one block, between ordinary sites."""
    rng = np.random.default_rng(22)
    cols = blinking_sites(400, 25, 32, 23, np.float32)
    patch = {"frame": rng.integers(0, 20000, 3000).astype(np.uint32),
             "x": (7.55 + rng.normal(0, 0.008, 3000)).astype(np.float32),
             "y": (9.55 + rng.normal(0, 0.008, 3000)).astype(np.float32),
             "photons": rng.uniform(500, 9000, 3000).astype(np.float32),
             "lpx": rng.uniform(0.005, 0.06, 3000).astype(np.float32)}
    order = rng.permutation(13000)
    cols = {c: np.concatenate([cols[c], patch[c]])[order] for c in cols}
    info = {"Width": 32, "Height": 32, "Frames": 20000}
    b = rs.Blocks(cols, info, 0.1)
    assert np.bincount(b.ki * b.L + b.li).max() >= 2900
    density, dh = _check_against_restatement(cols, info, 0.1, 0.002, "dense patch")
    assert density.max() >= 2900 and dh.sum() > 4_000_000
