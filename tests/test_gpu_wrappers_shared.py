"""GPU tier: the layer the row-table wrappers of picasso_amd/backend.py share (columns, type codes, descriptor tables,
residence) at the shapes where it alone can go wrong: descriptor tables at their limit and one past it, built from
columns nobody but the wrapper references; one column reached as itself, as a view and as a copy; tables of no row and
of one row; a side stream; and the four descriptor calls in both orders from empty scratch.

Every value is a small integer (weights are powers of two) and every group size a power of two, so each sum, each mean
and each squared deviation is exact in float32 and float64 alike: no summation order can show, and every comparison with
NumPy and pandas on the host is an equality."""
import gc

import numpy as np
import pandas as pd
import pytest

from picasso_amd import _lib, backend

pytestmark = pytest.mark.gpu

N = 257
SIZES = (128, 64, 64, 1)                     # 257 rows in 4 groups
DTYPES = ("float32", "float64", "int32", "uint32", "int64", "uint64")


def labels():
    return np.random.default_rng(1).permutation(np.repeat(np.arange(4, dtype=np.int64), SIZES))


def col(j, dtype=None):
    """Column j: integers 0 .. 7 in the dtype the column number selects (or `dtype`)."""
    return np.random.default_rng([2, j]).integers(0, 8, N).astype(dtype or DTYPES[j % len(DTYPES)])


def pow2(j, dtype):
    """Column j of powers of two 0.25 .. 1: its reciprocal square is exact."""
    return np.random.default_rng([3, j]).choice(np.array([0.25, 0.5, 1.0]), N).astype(dtype)


def per_group(group, fn):
    return [fn(np.flatnonzero(group == g)) for g in np.unique(group)]


def mean_std(group, c):
    """pandas' Series.mean() / Series.std() per group, as float64."""
    mean = np.array(per_group(group, lambda rows: pd.Series(c[rows]).mean()), np.float64)
    std = np.array(per_group(group, lambda rows: pd.Series(c[rows]).std()), np.float64)
    return mean, std


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b, equal_nan=a.dtype.kind == "f")


# ---- what NumPy and pandas give for these inputs, stated on its own ------------------------------------------------
def link_jobs(k):
    """k (op, data, weight) requests over fresh columns, every op and every dtype among them."""
    jobs = []
    for j in range(k):
        op = (backend.LINK_SUM, backend.LINK_WSUM, backend.LINK_XWSUM)[j % 3]
        f = ("float32", "float64")[(j // 3) % 2]
        if op == backend.LINK_SUM:
            jobs.append((op, col(j, DTYPES[(j // 3) % len(DTYPES)]), None))
        elif op == backend.LINK_WSUM:
            jobs.append((op, None, pow2(j, f)))
        else:
            jobs.append((op, col(j, ("float64", "float32")[(j // 6) % 2]), pow2(j, f)))
    return jobs


def link_expected(group, frame, jobs):
    sums = []
    for op, data, weight in jobs:
        if op == backend.LINK_SUM:
            terms, dt = data.astype(np.float64), data.dtype
        elif op == backend.LINK_WSUM:
            terms, dt = 1.0 / weight.astype(np.float64) ** 2, weight.dtype
        else:
            terms, dt = data.astype(np.float64) / weight.astype(np.float64) ** 2, np.promote_types(data.dtype, weight.dtype)
        sums.append(np.array(per_group(group, lambda rows: terms[rows].sum())).astype(dt))
    return (np.array(per_group(group, len), np.uint32), np.array(per_group(group, lambda r: frame[r].min()), np.int64),
            np.array(per_group(group, lambda r: frame[r].max()), np.int64),
            np.array(per_group(group, lambda r: r[-1]), np.int32), sums)


def stats_requests(groups, k):
    """k requests for CenterGroups.stats, every op among them; ``groups`` None gives the host side only."""
    requests, expected, group = [], [], labels()
    for j in range(k):
        op = (backend.CENTERS_MEAN, backend.CENTERS_FIRST, backend.CENTERS_EVENTS, backend.CENTERS_XSUM)[j % 4]
        if op == backend.CENTERS_MEAN:
            c = col(j)
            acc = np.float32 if c.dtype == np.float32 else np.float64
            total = np.array(per_group(group, lambda r: c[r].astype(np.float64).sum()))
            std = pd.Series(c.astype(np.float64)).groupby(group).std().to_numpy()      # Welford in float64 for every type
            requests.append((op, c, None, ("sum", "mean", "std")))
            expected.append({"sum": total.astype(acc), "mean": (total / np.array(SIZES)).astype(acc), "std": std})
        elif op == backend.CENTERS_FIRST:
            c = col(j)
            requests.append((op, c, None, ()))
            expected.append({"sum": np.array(per_group(group, lambda r: c[r[0]]), c.dtype)})
        elif op == backend.CENTERS_EVENTS:
            c = col(j, ("int32", "uint32", "int64", "uint64")[(j // 4) % 4]) * np.array(2, "uint8")
            with np.errstate(over="ignore"):
                events = per_group(group, lambda r: 1 + int((c[r][1:] - c[r][:-1] > 3).sum()))      # unsigned differences wrap
            requests.append((op, c, None, ()))
            expected.append({"sum": np.array(events, np.int32)})
        else:
            f = ("float32", "float64")[(j // 4) % 2]
            c, lp = col(j, ("float32", "float64")[(j // 8) % 2]), pow2(j, f)
            w = 1.0 / (2.0 * lp.astype(np.float64)) ** 2
            requests.append((op, c, None if groups is None else groups.weights(pow2(j, f), pow2(j, f)), ()))
            expected.append({"sum": np.array(per_group(group, lambda r: (c[r] * w[r]).sum()))
                             .astype(np.promote_types(c.dtype, lp.dtype))})
    return requests, expected


def combine_jobs(k):
    """k columns for combine_stats: two moments, then an average, and so on -> (moments, averages) as column numbers."""
    return [j for j in range(k) if j % 3 != 2], [j for j in range(k) if j % 3 == 2]


def average_pair(j):
    f = ("float32", "float64")[j % 2]
    return col(j, f), (4.0 * pow2(j, f)).astype(f)


def average_expected(group, x, w):
    avg = per_group(group, lambda r: np.average(x[r], weights=w[r]))
    return np.array(avg, np.float64), np.array(per_group(group, lambda r: w[r].sum()), np.float64)


def check_host_references():
    """The expectations above are what plain arithmetic on exact float64 sums gives, and what pandas' groupby gives by
    its own route: no summation order is in them.  Needs no device: tests/test_abi_structs.py runs it in the CPU tier."""
    group = labels()
    by = lambda c: pd.Series(c).groupby(group)                                # noqa: E731
    frame = col(100, "uint32")
    count, first, last, last_row, sums = link_expected(group, frame, link_jobs(24))
    assert count.tolist() == by(frame).size().tolist() and first.tolist() == by(frame).min().tolist()
    assert last.tolist() == by(frame).max().tolist() and last_row.tolist() == by(np.arange(N)).max().tolist()
    for (op, data, weight), total in zip(link_jobs(24), sums):
        terms = (1.0 if data is None else data.astype(np.float64)) * (1.0 if weight is None else weight.astype(np.float64) ** -2)
        assert total.tolist() == by(terms * np.ones(N)).sum().tolist()
    for (op, c, _, _), want in zip(*stats_requests(None, 32)):
        if op == backend.CENTERS_MEAN:
            assert want["sum"].tolist() == by(c.astype(np.float64)).sum().tolist()
            assert want["mean"].tolist() == by(c.astype(np.float64)).mean().tolist()
        elif op == backend.CENTERS_FIRST:
            assert want["sum"].tolist() == by(c).first().tolist()
        elif op == backend.CENTERS_EVENTS:
            wide = c.astype(np.int64)                                        # values 0 .. 14: an unsigned column that decreases wraps and counts
            gaps = [np.diff(wide[r]) for r in per_group(group, lambda r: r)]
            wraps = c.dtype.kind == "u"
            assert want["sum"].tolist() == [1 + int(((d > 3) | (wraps & (d < 0))).sum()) for d in gaps]
    assert sorted(np.bincount(group)) == sorted(SIZES)
    for j in range(len(DTYPES)):
        c = col(j)
        mean, std = mean_std(group, c)
        exact = np.array(per_group(group, lambda r: c[r].astype(np.float64).sum())) / np.array(SIZES)
        assert np.array_equal(mean, exact)
        for g, rows in enumerate(per_group(group, lambda r: r)):
            v = c[rows].astype(np.float64)
            var = ((v - exact[g]) ** 2).sum() / (len(v) - 1) if len(v) > 1 else np.nan
            want = np.float64(np.sqrt(np.float32(var))) if c.dtype == np.float32 else np.sqrt(var)
            assert std[g] == want or (np.isnan(want) and np.isnan(std[g])), (j, g)
    for j in (2, 5):
        x, w = average_pair(j)
        avg, total = average_expected(group, x, w)
        products = np.array(per_group(group, lambda r: (x[r].astype(np.float64) * w[r]).sum()))
        assert np.array_equal(avg, (products.astype(x.dtype) / total.astype(x.dtype)).astype(np.float64))


# ---- descriptor lifetime and chunking ----------------------------------------------------------------------------
def test_link_combine_at_its_limit():
    group, frame = labels(), col(100, "uint32")
    got = backend.link_combine(group.astype(np.int32), 4, frame.copy(), link_jobs(24))
    gc.collect()
    want = link_expected(group, frame, link_jobs(24))
    assert all(same(a, b) for a, b in zip(got[:4], want[:4]))
    assert len(got[4]) == 24 and all(same(a, b) for a, b in zip(got[4], want[4]))
    with pytest.raises(_lib.HipBackendError, match="pmi_link_combine_dev"):
        backend.link_combine(group.astype(np.int32), 4, frame, link_jobs(25))


def test_center_stats_at_its_limit():
    groups = backend.CenterGroups(labels())
    got = groups.stats(stats_requests(groups, 32)[0])
    gc.collect()
    want = stats_requests(None, 32)[1]
    assert len(got) == 32
    for j, (a, b) in enumerate(zip(got, want)):
        assert sorted(a) == sorted(b), j
        assert all(same(a[k], b[k]) for k in b), (j, a, b)
    with pytest.raises(_lib.HipBackendError, match="pmi_centers_stats_dev"):
        groups.stats(stats_requests(groups, 33)[0])


@pytest.mark.parametrize("k", (64, 65))
def test_group_mean_std_chunks(k):
    group = labels()
    got = backend.group_mean_std(backend.CenterGroups(group), [col(j) for j in range(k)])
    gc.collect()
    assert len(got) == k
    for j, (mean, std) in enumerate(got):
        want = mean_std(group, col(j))
        assert same(mean, want[0]) and same(std, want[1]), j


@pytest.mark.parametrize("k", (32, 33))
def test_combine_stats_chunks(k):
    group = labels()
    moments, averages = combine_jobs(k)
    got_m, got_a = backend.combine_stats(backend.CombineGroups(group, np.zeros(N, np.int32)),
                                         [col(j) for j in moments], [average_pair(j) for j in averages])
    gc.collect()
    assert len(got_m) == len(moments) and len(got_a) == len(averages)
    for j, (mean, std) in zip(moments, got_m):
        want = mean_std(group, col(j))
        assert same(mean, want[0]) and same(std, want[1]), j
    for j, (avg, total) in zip(averages, got_a):
        want = average_expected(group, *average_pair(j))
        assert same(avg, want[0]) and same(total, want[1]), j


# ---- the upload cache ----------------------------------------------------------------------------------------------
def test_one_column_reached_three_ways():
    group, c = labels(), col(0)
    groups = backend.CenterGroups(group)
    first = backend.group_mean_std(groups, [c])
    uploads = len(groups._cache)
    assert backend.group_mean_std(groups, [c[:]])[0][0].tobytes() == first[0][0].tobytes()
    assert len(groups._cache) == uploads                                     # a view of the column is the column
    for other in (c.copy(), np.repeat(c, 2)[::2]):
        again = backend.group_mean_std(groups, [other])
        assert same(again[0][0], first[0][0]) and same(again[0][1], first[0][1])
    assert len(groups._cache) == uploads + 2
    for call in (lambda: backend.group_mean_std(groups, [c[:-1]]),
                 lambda: groups.stats([(backend.CENTERS_MEAN, c[:-1], None, ("mean",))]),
                 lambda: groups.hull_areas(c[:-1], c)):
        with pytest.raises(ValueError, match="one entry per row"):
            call()


# ---- no row, one row ---------------------------------------------------------------------------------------------
def empty(dtype):
    return np.zeros(0, dtype)


def test_tables_of_no_row():
    t = backend.LinkTable(empty("uint32"), empty("float32"), empty("float64"), empty("int32"))
    lo, hi = t.frame_index(3)
    assert same(lo.cpu().numpy(), empty("int32")) and same(hi.cpu().numpy(), empty("int32"))
    link_group, n_groups = t.link_groups(1.0, 2)
    assert same(link_group.cpu().numpy(), empty("int32")) and n_groups == 0
    assert same(t.nena_hist(1.0, 0.1, 10), np.zeros(10, np.int64))

    points = backend.ClusterPoints(np.zeros((0, 2), np.float32))
    assert same(points.counts(1.0), empty("int32")) and same(points.dbscan(1.0, 2, 2), empty("int32"))
    assert same(points.smlm(1.0, 2), empty("int32"))

    table = backend.BlockTable(empty("uint32"), empty("uint32"), 4, 4)
    assert table.p == 0 and same(table.order(), empty("int64"))
    assert same(table.density(empty("float32"), empty("float32"), 1.0), empty("uint32"))
    assert same(table.distance_hist(empty("float32"), empty("float32"), 1.0, 1.0, 0.1, 10), np.zeros(10, np.uint64))


def test_no_pick_and_no_grid_point():
    x = y = np.array([0.5], np.float32)
    table = backend.BlockTable(np.zeros(1, np.uint32), np.zeros(1, np.uint32), 1, 1)
    none = (np.zeros(1, np.int64), empty("int64"))
    for got in (backend.picks_circle(table, x, y, empty("float64"), empty("float64"), empty("int64"), empty("int64"),
                                     empty("uint8"), 1.0),
                backend.picks_square(x, y, np.zeros((0, 4)), empty("uint8")),
                backend.picks_rectangle(x, y, np.zeros((0, 4)), empty("uint8"), np.zeros((0, 4)), np.zeros((0, 4))),
                backend.picks_polygon(x, y, np.zeros((0, 4)), empty("uint8"), np.zeros(1, np.int32), empty("float64"),
                                      empty("float64"))):
        assert same(got[0], none[0]) and same(got[1], none[1])
    got = backend.similar_shift(table, x, y, empty("float64"), empty("float64"), empty("float64"), empty("int64"),
                                empty("int64"), empty("int64"), 1.0, 1.0)
    assert [a.dtype for a in got] == [np.float64, np.float64, np.int32, np.float64] and all(a.shape == (0,) for a in got)


def test_tables_that_refuse_no_row():
    for build in (lambda: backend.CenterGroups(empty("int64")), lambda: backend.CombineGroups(empty("int64"), empty("int64")),
                  lambda: backend.DarkTable(empty("int64"), empty("int64"), empty("int64"))):
        with pytest.raises(ValueError, match="at least one row"):
            build()


def test_tables_of_one_row():
    one_f, one_i = np.array([3.0], np.float32), np.array([5], np.int64)
    t = backend.LinkTable(one_i, one_f, one_f, np.zeros(1, np.int32))
    lo, hi = t.frame_index(3)
    assert lo.cpu().numpy().tolist() == [1] and hi.cpu().numpy().tolist() == [1]
    link_group, n_groups = t.link_groups(1.0, 2)
    assert same(link_group.cpu().numpy(), np.zeros(1, np.int32)) and n_groups == 1
    count, first, last, last_row, sums = backend.link_combine(np.zeros(1, np.int32), 1, one_i, [(backend.LINK_SUM, one_f, None)])
    assert (count.tolist(), first.tolist(), last.tolist(), last_row.tolist()) == ([1], [5], [5], [0]) and same(sums[0], one_f)

    points = backend.ClusterPoints(np.zeros((1, 3)))
    assert same(points.counts(1.0), np.ones(1, np.int32))
    assert points.dbscan(1.0, 2, 2).tolist() == [-1] and points.smlm(1.0, 2).tolist() == [-1]

    table = backend.BlockTable(np.zeros(1, np.uint32), np.zeros(1, np.uint32), 1, 1)
    assert table.p == 1 and table.order().tolist() == [0]
    density = table.density(one_f, one_f, 1.0)
    assert density.dtype == np.uint32 and density.shape == (1,)
    hist = table.distance_hist(one_f, one_f, 1.0, 1.0, 0.1, 10)
    assert hist.dtype == np.uint64 and hist.shape == (10,)
    offsets, rows = backend.picks_circle(table, one_f, one_f, [3.0], [3.0], [0], [0], [0], 1.0)
    assert offsets.tolist() == [0, 1] and rows.tolist() == [0] and rows.dtype == np.int64
    offsets, rows = backend.picks_square(one_f, one_f, [[2.0, 4.0, 2.0, 4.0]], [0])
    assert offsets.tolist() == [0, 1] and rows.tolist() == [0]

    for groups in (backend.CenterGroups(one_i), backend.CombineGroups(one_i, one_i)):
        assert groups.unique.tolist() == [5] and groups.n_locs.tolist() == [1] and groups.order().tolist() == [0]
        (mean, std), = backend.group_mean_std(groups, [one_f])
        assert mean.tolist() == [3.0] and np.isnan(std).all() and mean.dtype == std.dtype == np.float64
        (stats,) = groups.stats([(backend.CENTERS_MEAN, one_f, None, ("sum", "mean", "std"))])
        assert stats["sum"].tolist() == stats["mean"].tolist() == [3.0] and stats["sum"].dtype == np.float32
        assert np.isnan(stats["std"]).all() and stats["std"].dtype == np.float64
    (moments,), (average,) = backend.combine_stats(groups, [one_f], [(one_f, np.array([2.0], np.float32))])
    assert moments[0].tolist() == [3.0] and np.isnan(moments[1]).all()
    assert (average[0].tolist(), average[1].tolist()) == ([3.0], [2.0]) and average[0].dtype == np.float64
    assert same(backend.DarkTable(one_i, one_i, one_i).search(), np.array([-1], np.int64))


# ---- residence -----------------------------------------------------------------------------------------------------
def every_descriptor_call(order):
    """The four descriptor calls over fresh tables, run in ``order`` -> their results as flat lists of arrays, by name."""
    group = labels()

    def link():
        got = backend.link_combine(group.astype(np.int32), 4, col(100, "uint32"), link_jobs(6))
        return list(got[:4]) + got[4]

    def stats():
        groups = backend.CenterGroups(group)
        return [a for out in groups.stats(stats_requests(groups, 8)[0]) for _, a in sorted(out.items())]

    def kinetics():
        return [a for pair in backend.group_mean_std(backend.CenterGroups(group), [col(j) for j in range(6)]) for a in pair]

    def combine():
        groups = backend.CombineGroups(group, np.zeros(N, np.int32))
        got = backend.combine_stats(groups, [col(0), col(2)], [average_pair(1)])
        return [a for pair in got[0] + got[1] for a in pair]

    calls = {"link": link, "stats": stats, "kinetics": kinetics, "combine": combine}
    return {name: calls[name]() for name in order}


def assert_same_results(a, b):
    assert sorted(a) == sorted(b)
    for name in a:
        assert len(a[name]) == len(b[name])
        assert all(x.dtype == y.dtype and x.tobytes() == y.tobytes() for x, y in zip(a[name], b[name])), name


def test_side_stream():
    import torch
    names = ("link", "stats", "kinetics", "combine")
    default = every_descriptor_call(names)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        table = backend.CenterGroups(labels())
        assert table.stream == side.cuda_stream
        on_side = every_descriptor_call(names)
    side.synchronize()
    assert_same_results(default, on_side)


def test_both_orders_from_empty_scratch():
    names = ("link", "stats", "kinetics", "combine")
    _lib.call("pmi_release_scratch")                                         # every slot starts empty
    forward = every_descriptor_call(names)
    backward = every_descriptor_call(names[::-1])
    assert_same_results(forward, backward)
    assert same(forward["kinetics"][0], mean_std(labels(), col(0))[0])
