"""GPU tier: the group layer of csrc/rows_groups.h (the sort by "column - minimum", the key width, run closing, the
gather and the type dispatch) at the shapes where it alone can go wrong: one row, two rows, one block and one row to
either side of it; label columns whose span needs one bit, and all 64 with a key subtraction that wraps.  The three
orders built on it (CenterGroups, CombineGroups, DarkTable) equal NumPy's on the host, and in one process, from empty
scratch slots, the modules run after one another in both directions without changing each other's results."""
import numpy as np
import pytest

from picasso_amd import _lib, backend

pytestmark = pytest.mark.gpu

I64 = np.iinfo(np.int64)
SIZES = (1, 2, 255, 256, 257)
KINDS = ("one", "pair", "extremes", "random")
CASES = [(n, kind) for n in SIZES for kind in KINDS if kind != "random" or n >= 255]


def labels(n, kind, seed):
    """An int64 label column: `one` has span 0 (a key of one bit), `pair` is {-1, 0}, `extremes` spans all 64 bits
    (INT64_MAX - INT64_MIN wraps in the key), `random` has about n / 3 distinct labels around zero."""
    rng = np.random.default_rng([seed, n])
    if kind == "one":
        return np.full(n, 7, np.int64)
    if kind == "pair":
        return rng.integers(-1, 1, n).astype(np.int64)
    if kind == "extremes":
        a = rng.choice(np.array([I64.min, -1, 0, I64.max], np.int64), n)
        if n >= 2:
            a[rng.integers(0, n // 2)], a[rng.integers(n // 2, n)] = I64.max, I64.min      # the whole span, out of order
        return a
    return rng.integers(-(n // 6), n // 3 - n // 6, n).astype(np.int64)


def runs_of(*sorted_columns):
    """first[p]: a new run of equal tuples starts at sorted position p."""
    same = np.ones(len(sorted_columns[0]) - 1, bool)
    for c in sorted_columns:
        same &= c[1:] == c[:-1]
    return np.concatenate([[True], ~same])


@pytest.mark.parametrize("n,kind", CASES)
def test_center_groups_order(n, kind):
    group = labels(n, kind, 1)
    g = backend.CenterGroups(group)
    want_unique, want_counts = np.unique(group, return_counts=True)
    assert np.array_equal(g.order(), np.argsort(group, kind="stable"))
    assert g.n_groups == len(want_unique)
    assert g.unique.dtype == np.int64 and np.array_equal(g.unique, want_unique)
    assert np.array_equal(g.n_locs, want_counts)
    assert np.array_equal(g.offsets, np.concatenate([[0], np.cumsum(want_counts)]))


@pytest.mark.parametrize("n,kind", CASES)
def test_combine_groups_order(n, kind):
    group, cluster = labels(n, kind, 1), labels(n, kind, 2)
    g = backend.CombineGroups(group, cluster)
    order = np.lexsort((cluster, group))
    gs, cs = group[order], cluster[order]
    seg, grp = runs_of(gs, cs), runs_of(gs)
    assert np.array_equal(g.order(), order)
    assert g.n_groups == seg.sum() and g.n_outer == grp.sum()
    assert np.array_equal(g.unique, gs[seg]) and np.array_equal(g.clusters, cs[seg])
    assert np.array_equal(g.offsets, np.concatenate([np.flatnonzero(seg), [n]]))
    assert np.array_equal(g.group_offsets, np.concatenate([(np.cumsum(seg) - 1)[grp], [seg.sum()]]))


@pytest.mark.parametrize("n,kind", CASES)
def test_dark_table_order(n, kind):
    rng = np.random.default_rng([3, n])
    group = labels(n, kind, 1)
    top = backend.KINETICS_FRAME_LIMIT - 1
    last = rng.choice(np.array([-top, -1, 0, 1, 5, top], np.int64), n)      # ties, and a span of 63 bits
    frame = rng.integers(0, 100, n).astype(np.int64)
    t = backend.DarkTable(frame, group, last)
    by_last = np.argsort(last, kind="stable")
    order = by_last[np.argsort(group[by_last], kind="stable")]
    assert np.array_equal(order, np.lexsort((last, group)))
    assert np.array_equal(t.rows.cpu().numpy(), order)
    assert np.array_equal(t.last_sorted.cpu().numpy(), last[order])
    first = runs_of(group[order])
    n_runs = int(first.sum())
    assert np.array_equal(t.run.cpu().numpy(), np.cumsum(first) - 1)
    assert np.array_equal(t.start.cpu().numpy()[:n_runs + 1], np.concatenate([np.flatnonzero(first), [n]]))


def test_modules_leave_nothing_behind():
    n = 257
    rng = np.random.default_rng(4)
    group, cluster = labels(n, "random", 1), labels(n, "random", 2)
    f32 = rng.normal(0, 50, n).astype(np.float32)
    i64 = rng.integers(-10 ** 12, 10 ** 12, n).astype(np.int64)
    last = rng.integers(0, 50, n).astype(np.int64)
    frame = last + rng.integers(0, 20, n)

    def centers():
        g = backend.CenterGroups(group)
        return [g.order()] + [a for pair in backend.group_mean_std(g, [f32, i64]) for a in pair]

    def combine():
        g = backend.CombineGroups(group, cluster)
        return [g.order()] + [a for pair in backend.combine_stats(g, moments=[f32, i64])[0] for a in pair]

    def dark():
        t = backend.DarkTable(frame, group, last)
        return [t.rows.cpu().numpy(), t.start.cpu().numpy(), t.search()]

    _lib.check(_lib.load().pmi_release_scratch(), "pmi_release_scratch")     # every slot starts empty
    calls = (centers, combine, dark)
    first = [call() for call in calls]
    again = [call() for call in reversed(calls)][::-1]
    for a, b in zip(first, again):
        assert len(a) == len(b)
        for x, y in zip(a, b):
            assert x.dtype == y.dtype and x.tobytes() == y.tobytes()
    assert np.array_equal(first[0][0], np.argsort(group, kind="stable"))
    assert np.array_equal(first[1][0], np.lexsort((cluster, group)))
    assert len(np.unique(group)) > 1 and np.isfinite(first[0][1]).all()      # the statistics ran over real runs
