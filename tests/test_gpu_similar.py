"""GPU tier of pick_similar: every golden case through ``postprocess.pick_similar`` on the device (the pairs equal to the
reference's in every bit, in length and order, or the recorded exception), and ``backend.similar_shift`` against the
restatement on fixed-seed tables, all four outputs equal in bits per grid point.  No tolerance anywhere."""
import functools
import warnings

import numpy as np
import pytest

from picasso_amd import backend, postprocess

from _similar_cases import CASES, G, assert_pairs, assert_shift, call, clustered, rs, table

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", CASES)
def test_golden_case_on_the_device(name, monkeypatch):
    info, picks, d, std_range, max_shifts, _ = call(name)
    if max_shifts != 500:          # the case replaced the reference's constant; so does the call here
        monkeypatch.setattr(backend, "similar_shift", functools.partial(backend.similar_shift, max_shifts=max_shifts))
    df = table(name)
    before = df.copy()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")          # np.mean of an empty pick list warns, in the reference too
        if f"{name}/raises" in G.files:
            with pytest.raises(ZeroDivisionError):
                postprocess.pick_similar(df, info, picks, d, std_range)
        else:
            assert_pairs(postprocess.pick_similar(df, info, picks, d, std_range), name)
    assert df.equals(before)


def both(x, y, width, height, d, gate, max_shifts=500, K=None, L=None):
    """-> (the device's four outputs, the restatement's) for one table and grid."""
    info = [{"Width": width, "Height": height}]
    r = d / 2
    K = int(np.ceil(height / r)) if K is None else K
    L = int(np.ceil(width / r)) if L is None else L
    grid = rs.grid(info, d)
    t = backend.BlockTable(np.uint32(x / r), np.uint32(y / r), K, L)
    got = backend.similar_shift(t, x, y, *grid[:3], np.uint64(grid[3]), np.uint64(grid[4]), np.uint64(grid[5]), r * r, gate, max_shifts)
    return got, rs.shift(x, y, r, K, L, grid, r * r, gate, max_shifts), grid


@functools.lru_cache(maxsize=None)
def small_table():
    return clustered(11, 24, 24, 30)


@pytest.mark.parametrize("max_shifts", [1, 2, 500])
def test_shift_caps(max_shifts):
    x, y = small_table()
    got, want, _ = both(x, y, 24, 24, 2.0, 4, max_shifts)
    assert_shift(got, want, max_shifts)
    if max_shifts < 500:
        assert (want[5] == rs.CAPPED).any()
    else:
        assert (want[5] == rs.CONVERGED).sum() > 20 and (want[2] == 0).any() and want[4].max() >= 3


@pytest.mark.parametrize("n_y, dtypes", [(63, (np.float32, np.float32)), (64, (np.float64, np.float64)),
                                         (65, (np.float32, np.float64)), (257, (np.float32, np.float32))])
def test_wave_and_workgroup_edges(n_y, dtypes):
    height = 2 * n_y + 2
    x, y = clustered(n_y, 9, height, 3 * n_y // 4, dtypes[0], dtypes[1], background=n_y)
    got, want, grid = both(x, y, 9, height, 2.0, 3)
    assert len(grid[1]) == n_y and len(got[0]) == len(grid[0]) * n_y
    assert_shift(got, want, n_y)
    assert (want[2] > 1).sum() > n_y // 8


def test_one_block_of_300_rows():
    rng = np.random.default_rng(5)
    x, y = clustered(5, 12, 12, 6)
    x = np.r_[x, rng.uniform(5.0, 5.999, 300).astype(np.float32)]
    y = np.r_[y, rng.uniform(7.0, 7.999, 300).astype(np.float32)]
    assert ((np.uint32(x) == 5) & (np.uint32(y) == 7)).sum() >= 300
    got, want, _ = both(x, y, 12, 12, 2.0, 2)
    assert_shift(got, want, "300")
    assert want[2].max() >= 200


def test_all_rows_in_one_block_and_narrow_grids():
    rng = np.random.default_rng(6)
    x, y = rng.uniform(3.0, 3.999, 40).astype(np.float32), rng.uniform(4.0, 4.999, 40).astype(np.float32)
    got, want, _ = both(x, y, 10, 10, 2.0, 2)
    assert_shift(got, want, "one block")
    assert (want[2] > 1).any()
    # the rows in block row 0 / block column 0: the gate never counts them
    got, want, _ = both(x - 3, y - 4, 10, 10, 2.0, 2)
    assert_shift(got, want, "block (0, 0)")
    assert (want[2] == 0).all() and (rs.shift(x - 3, y - 4, 1.0, 10, 10, rs.grid([{"Width": 10, "Height": 10}], 2.0), 1.0, 0)[2] > 1).any()
    # K == 1 / L == 1: no block passes 0 < k < K, the reference's count is never assigned (0)
    for K, L in ((1, 10), (10, 1)):
        xs, ys = (x - 3, y % 1) if K == 1 else (x % 1, y - 4)
        got, want, _ = both(xs, ys, 10, 10, 2.0, 0.5, K=K, L=L)
        assert_shift(got, want, (K, L))
        assert (want[2] == 0).all()


def test_empty_table_and_empty_grid():
    none = np.zeros(0, np.float32)
    got, want, grid = both(none, none, 8, 8, 2.0, 0)
    assert_shift(got, want, "empty")
    assert len(got[0]) == len(grid[0]) * len(grid[1]) > 0 and (got[2] == 0).all()
    x, y = small_table()
    got, want, grid = both(x, y, 24, 2, 2.0, 0)          # Height <= d: no y value
    assert len(grid[1]) == 0 and all(len(a) == 0 for a in got)
