"""GPU tier: the block layer of csrc/rows_blocks.h (the key, the run of a block row by two bisections over the visible
prefix, the clamped 3 x 3 window) at the shapes where it alone can go wrong: one row, two rows, one workgroup and one
row to either side of it, on grids of one to three blocks a side; a fill that stalls before the last row (p < n); block
indices from two outside the grid on one side to one outside on the other.  The order equals NumPy's on the host, the
density, the histogram, the circular picks and the mean shift equal the restatements of tests/golden, and in one
process, from empty scratch slots, the modules run after one another in both directions without changing each other's
results.  Every comparison is an equality."""
import numpy as np
import pytest

from picasso_amd import _lib, backend

from _similar_cases import assert_shift, prs, rs as srs          # _picks_restate, _similar_restate
from test_gpu_picks import device_members

import _fiducials_restate as frs  # noqa: E402  (tests/golden is on the path once _similar_cases is imported)
import _pairs_restate as qrs  # noqa: E402

pytestmark = pytest.mark.gpu

SIZES = (1, 2, 255, 256, 257)
GRIDS = ((1, 1), (1, 3), (3, 1), (2, 2), (3, 3))
R = 1.0          # block size, pick radius and density radius of the tables made here


def points(n, K, L, seed, x_dtype=np.float32, y_dtype=np.float32):
    """n rows inside a frame of K x L blocks of size R."""
    rng = np.random.default_rng([seed, n, K, L])
    return rng.uniform(0, L * R - 0.01, n).astype(x_dtype), rng.uniform(0, K * R - 0.01, n).astype(y_dtype)


def frame(K, L):
    return {"Width": L * R, "Height": K * R}


def around(count):
    """The block indices -2, -1, 0, count - 1, count, count + 1."""
    return sorted({-2, -1, 0, count - 1, count, count + 1})


def centre(b):
    """A coordinate whose block (truncation toward zero) is b."""
    v = (b + 0.5) * R if b >= 0 else (b - 0.5) * R
    assert prs.block_of(v, R) == b
    return v


def block_table(x, y, size, K, L):
    return backend.BlockTable(np.uint32(x / size), np.uint32(y / size), K, L)


def assert_order(t, x, y, size, K, L):
    """order() is np.lexsort([x_index, y_index]), the keys decode to the indices, p is where the fill stops."""
    xi, yi = np.uint32(x / size), np.uint32(y / size)
    order = t.order()
    assert np.array_equal(order, np.lexsort([xi, yi]))
    keys = t.keys[:t.n].cpu().numpy()
    assert np.array_equal(keys >> 32, yi[order].astype(np.int64)) and np.array_equal(keys & 0xffffffff, xi[order].astype(np.int64))
    want_order, want_keys, p = prs.block_order(x, y, size, K, L)
    assert np.array_equal(order, want_order) and np.array_equal(keys, want_keys) and t.p == p
    return p


def assert_pairs(t, cols, info, radius, bin_size=0.05):
    b, density = qrs.local_density(cols, info, radius)
    assert (t.n, t.p, t.K, t.L) == (b.n, b.p, b.K, b.L)
    got = t.density(cols["x"], cols["y"], qrs.squared(radius))
    assert got.dtype == np.uint32 and np.array_equal(got.astype(np.uint64), density)
    n_bins = int(np.uint32(radius / bin_size))
    dh = t.distance_hist(cols["x"], cols["y"], radius, qrs.squared(radius), bin_size, n_bins)
    assert dh.dtype == np.uint64 and np.array_equal(dh, qrs.distance_histogram(cols, info, bin_size, radius))
    return b, density, dh


def assert_circles(cols, info, picks, radius):
    offsets, rows = prs.circle(cols, info, picks, radius)
    got_offsets, got_rows = device_members(cols, [info], picks, "Circle", radius)
    assert got_offsets.dtype == np.int64 and np.array_equal(got_offsets, offsets) and np.array_equal(got_rows, rows)
    return offsets, rows


def shift_grid(K, L, blocks_y, blocks_x):
    """A grid whose points name the blocks given, whatever their coordinates: the points themselves stay inside the
    frame, so that a window clamped wrongly changes the members."""
    inside = lambda blocks, count: np.clip([centre(b) for b in blocks], 0.25 * R, (count - 0.25) * R)      # noqa: E731
    y_base = inside(blocks_y, K)
    return (inside(blocks_x, L), y_base, np.clip(y_base + 0.3 * R, 0, K * R), np.array(blocks_x, np.int64),
            np.array(blocks_y, np.int64), np.roll(np.array(blocks_y, np.int64), 1))


def assert_shifts(t, x, y, K, L, grid, gate):
    got = backend.similar_shift(t, x, y, *grid, R * R, gate)
    want = srs.shift(x, y, R, K, L, grid, R * R, gate)
    assert_shift(got, want, (t.n, K, L, gate))
    return want


@pytest.mark.parametrize("K,L", GRIDS)
@pytest.mark.parametrize("n", SIZES)
def test_every_size_on_every_grid(n, K, L):
    x, y = points(n, K, L, 1)
    t = block_table(x, y, R, K, L)
    assert assert_order(t, x, y, R, K, L) == n
    cols = {"x": x, "y": y}
    assert_pairs(t, cols, frame(K, L), R)
    assert_circles(cols, frame(K, L), [(centre(l), centre(k)) for k in range(K) for l in range(L)], R)
    assert_shifts(t, x, y, K, L, shift_grid(K, L, range(K), range(L)), 0)


def test_mixed_column_types():
    n, K, L = 257, 3, 3
    x, y = points(n, K, L, 2, np.float32, np.float64)
    t = block_table(x, y, R, K, L)
    assert assert_order(t, x, y, R, K, L) == n
    cols = {"x": x, "y": y}
    _, density, dh = assert_pairs(t, cols, frame(K, L), R)
    offsets, _ = assert_circles(cols, frame(K, L), [(centre(l), centre(k)) for k in range(K) for l in range(L)], R)
    want = assert_shifts(t, x, y, K, L, shift_grid(K, L, range(K), range(L)), 1)
    assert density.min() > 1 and dh.sum() > n and offsets[-1] > n and (want[2] > 1).any()


@pytest.mark.parametrize("n", [255, 257])
def test_stalled_fill_on_a_smaller_grid(n):
    """Rows on 8 x 8 blocks, a grid of 5 x 8: the fill stops at the first row of block row 5."""
    x, y = points(n, 8, 8, 3)
    K, L = 5, 8
    t = block_table(x, y, R, K, L)
    p = assert_order(t, x, y, R, K, L)
    assert 0 < p < n and p == (np.uint32(y / R) < K).sum()
    grid = srs.grid([frame(8, 8)], 2 * R)
    want = assert_shifts(t, x, y, K, L, grid, 2)
    assert (want[2] > 1).any()                                             # member rows before p
    everywhere = srs.shift(x, y, R, 8, 8, grid, R * R, 2)
    assert (everywhere[2] != want[2]).any()                                # and rows behind p that would have been members


@pytest.mark.parametrize("n", [255, 257])
def test_stalled_fill_at_the_frame_edge(n):
    """The stall as a user meets it: a float32 x one ulp below Width whose block index is L.  That row and every row
    sorted behind it is in no block; density, histogram and circular picks see the rows before it only."""
    rng = np.random.default_rng([4, n])
    size, info = 0.32, {"Width": 32, "Height": 32}
    x, y = rng.uniform(0, 4, n).astype(np.float32), rng.uniform(0, 4, n).astype(np.float32)
    x[0], y[0] = np.nextafter(np.float32(32), np.float32(0)), 2.0
    x[1:9], y[1:9] = 2.0 + rng.normal(0, 0.05, 8), 1.0 + rng.normal(0, 0.05, 8)          # before the stall
    x[9:17], y[9:17] = 3.0 + rng.normal(0, 0.05, 8), 3.5 + rng.normal(0, 0.05, 8)        # behind it
    cols = {"x": x, "y": y}
    t = block_table(x, y, size, 100, 100)
    p = assert_order(t, x, y, size, 100, 100)
    b, density, dh = assert_pairs(t, cols, info, size, 0.02)
    assert 0 < p < n and b.p == p and b.x_index[p] == b.L
    assert density[:p].max() > 1 and dh.sum() > 0
    offsets, rows = assert_circles(cols, info, [(2.0, 1.0), (3.0, 3.5), (31.95, 2.0)], size)
    position = np.argsort(t.order())
    assert offsets[1] >= 8 and (position[rows[:offsets[1]]] < p).all()     # member rows before p
    assert offsets[2] == offsets[1] and ((x - 3.0) ** 2 + (y - 3.5) ** 2 < size * size).sum() >= 8


@pytest.mark.parametrize("K,L", [(1, 1), (2, 2), (3, 3)])
def test_window_at_and_beyond_the_grid(K, L):
    n = 257
    x, y = points(n, K, L, 5)
    t = block_table(x, y, R, K, L)
    assert assert_order(t, x, y, R, K, L) == n
    cols = {"x": x, "y": y}
    _, density, _ = assert_pairs(t, cols, frame(K, L), R)                    # -1 wraps to the last block here
    picks = [(centre(l), centre(k)) for k in around(K) for l in around(L)]
    offsets, _ = assert_circles(cols, frame(K, L), picks, R)
    counts = np.diff(offsets).reshape(len(around(K)), len(around(L)))
    assert counts[around(K).index(K), around(L).index(0)] > 0              # one block outside: the last block row is in reach
    assert counts[0].sum() == 0 and counts[-1].sum() == 0                  # two outside: nothing is
    grid = shift_grid(K, L, around(K), around(L))
    free, gated = assert_shifts(t, x, y, K, L, grid, 0), assert_shifts(t, x, y, K, L, grid, 1)
    assert (free[2] > 1).any() and (free[2] == 0).any()
    assert (gated[2] > 1).any() == (K > 1) and (gated[2] != free[2]).any()
    assert density.max() > n / (K * L)                                     # a block counted twice through the wrap, K, L <= 2


def test_modules_leave_nothing_behind():
    n, K, L = 257, 3, 3
    rng = np.random.default_rng(6)
    x, y = points(n, K, L, 6)
    cols, info = {"x": x, "y": y}, frame(K, L)
    circles = [(centre(l), centre(k)) for k in around(K) for l in around(L)]
    polygons = [[(0.2, 0.3), (2.6, 0.4), (1.4, 2.8), (0.2, 0.3)], [(1.0, 1.0), (2.0, 1.0), (2.0, 2.0), (1.0, 2.0), (1.0, 1.0)]]
    grid = shift_grid(K, L, around(K), around(L))
    values = rng.normal(5, 2, 9000).astype(np.float32)
    runs = np.array([0, 3, 3, 300, 9000], np.int64)

    def density():
        t = block_table(x, y, R, K, L)
        return [t.order(), t.density(x, y, R * R)]

    def histogram():
        return [block_table(x, y, R, K, L).distance_hist(x, y, R, R * R, 0.05, 20)]

    def circle():
        return list(device_members(cols, [info], circles, "Circle", R))

    def polygon():
        return list(device_members(cols, [info], polygons, "Polygon", None))

    def similar():
        return list(backend.similar_shift(block_table(x, y, R, K, L), x, y, *grid, R * R, 1))

    def reduce():
        return [backend.fiducials_reduce(values, runs)]

    _lib.check(_lib.load().pmi_release_scratch(), "pmi_release_scratch")     # every slot starts empty
    calls = (density, histogram, circle, polygon, similar, reduce)
    first = [call() for call in calls]
    again = [call() for call in reversed(calls)][::-1]
    for a, b in zip(first, again):
        assert len(a) == len(b)
        for u, v in zip(a, b):
            assert u.dtype == v.dtype and u.tobytes() == v.tobytes()
    b, want_density = qrs.local_density(cols, info, R)
    assert np.array_equal(first[0][0], b.perm) and np.array_equal(first[0][1].astype(np.uint64), want_density)
    assert np.array_equal(first[1][0], qrs.distance_histogram(cols, info, 0.05, R))
    for got, (_, offsets, rows) in ((first[2], prs.members(cols, [info], circles, "Circle", R)),
                                    (first[3], prs.members(cols, [info], polygons, "Polygon"))):
        assert np.array_equal(got[0], offsets) and np.array_equal(got[1], rows) and len(rows) > n // 4
    assert_shift(first[4], srs.shift(x, y, R, K, L, grid, R * R, 1), "first")
    want = np.array([frs.pairwise_reduce(values[a:b]) for a, b in zip(runs[:-1], runs[1:])], np.float32)
    assert first[5][0].dtype == want.dtype and first[5][0].tobytes() == want.tobytes()
