"""Test-side restatement of the reference's ``cluster_combine`` / ``cluster_combine_dist``
(picasso/postprocess.py:2174-2419) in the structure csrc/combine.hip has: one ``np.lexsort`` by (group, cluster),
segment loops over the sorted table, NumPy's sums written out.

TEST INFRASTRUCTURE, NumPy only.

``sum32`` / ``sum64`` restate ``ndarray.sum()`` of a contiguous 1-D array as ``add.reduce`` runs it: an accumulator
from 0 over the pairwise sums (serial below 8, eight accumulators up to 128, split at n // 2 rounded down to a multiple
of 8 above) of 8192-element chunks.  ``series_mean`` / ``series_std`` are pandas' ``Series.mean()`` / ``Series.std()``
(tests/golden/_kinetics_restate.py).  ``average`` is ``np.average(x, weights=w)``.  The distances are brute force,
one row against the others of its group.
"""
import numpy as np

from _kinetics_restate import chunked_sum, series_mean, series_std  # noqa: F401

ZERO_WEIGHTS = "Weights sum to zero, can't be normalized"


def sum32(a):
    return chunked_sum(a, np.float32)


def sum64(a):
    return chunked_sum(a, np.float64)


def labels(a):
    a = np.asarray(a)
    if a.dtype.kind == "f":
        assert np.isfinite(a).all() and (a == np.trunc(a)).all()
    return a.astype(np.int64)


def segments(group, cluster):
    """-> (order, start, seg_group, seg_cluster, group_start): the table of pmi_combine_order_dev."""
    g, c = labels(group), labels(cluster)
    order = np.lexsort((c, g))                       # stable: table order within a pair
    gs, cs = g[order], c[order]
    new_group = np.r_[True, gs[1:] != gs[:-1]]
    new_seg = new_group | np.r_[True, cs[1:] != cs[:-1]]
    start = np.r_[np.flatnonzero(new_seg), len(g)]
    seg_of = np.cumsum(new_seg) - 1
    group_start = np.r_[seg_of[np.flatnonzero(new_group)], len(start) - 1]
    return order, start, gs[start[:-1]], cs[start[:-1]], group_start


def average(x, w):
    """``np.average(x, weights=w)`` -> (value in the result type, the sum of the weights)."""
    x, w = np.asarray(x), np.asarray(w)
    T = (np.result_type(x.dtype, w.dtype, "f8") if x.dtype.kind in "iub" else np.result_type(x.dtype, w.dtype)).type
    with np.errstate(all="ignore"):
        xs, ws = x.astype(T), w.astype(T)
        scl = chunked_sum(ws, T)
        total = chunked_sum(np.multiply(xs, ws), T)
        if scl == 0.0:
            raise ZeroDivisionError(ZERO_WEIGHTS)
        return T(total / scl), scl


def cluster_combine(cols):
    """``cols``: column name -> array -> dict of the result's columns, in the reference's order and dtypes."""
    axes = ("x", "y", "z") if "z" in cols else ("x", "y")
    order, start, seg_group, seg_cluster, _ = segments(cols["group"], cols["cluster"])
    S = len(start) - 1
    held = {k: np.zeros(S) for k in ("mean_frame", "std_frame") + axes + tuple("lp" + a for a in axes)}
    n = np.zeros(S, np.int32)
    sorted_cols = {c: np.asarray(cols[c])[order] for c in ("frame", "photons") + axes}
    with np.errstate(all="ignore"):
        for s in range(S):
            a, b = start[s], start[s + 1]
            run = {c: v[a:b] for c, v in sorted_cols.items()}
            held["mean_frame"][s] = series_mean(run["frame"])
            held["std_frame"][s] = series_std(run["frame"])
            for ax in axes:
                held[ax][s] = average(run[ax], run["photons"])[0]
                held["lp" + ax][s] = series_std(run[ax]) / np.sqrt(b - a)
            n[s] = b - a
    out = {"group": seg_group.astype(np.float64), "cluster": seg_cluster.astype(np.asarray(cols["cluster"]).dtype),
           "mean_frame": held["mean_frame"].astype(np.float32)}
    for ax in axes:
        out[ax] = held[ax].astype(np.float32)
    out["std_frame"] = held["std_frame"].astype(np.float32)
    for ax in axes:
        out["lp" + ax] = held["lp" + ax].astype(np.float32)
    out["n"] = n
    return out


def nearest_other(points, a, b):
    """float64 distance from every row of points[a:b] to the nearest other row of that run (np.amin: a NaN stays)."""
    out = np.full(b - a, np.inf)
    P = points[a:b]
    with np.errstate(all="ignore"):
        for i in range(b - a):
            d = P[i] - np.delete(P, i, axis=0)
            s = d[:, 0] * d[:, 0]
            for k in range(1, P.shape[1]):
                s = s + d[:, k] * d[:, k]
            if len(s):
                out[i] = np.sqrt(np.amin(s))
    return out


def cluster_combine_dist(cols, pixelsize=None):
    """``cols``: the columns of a combined table -> dict of the result's columns.  Raises what the reference raises for
    a group of one cluster or a repeated cluster label."""
    three = "z" in cols
    order, start, _, seg_cluster, group_start = segments(cols["group"], cols["cluster"])
    for g in range(len(group_start) - 1):
        distinct = group_start[g + 1] - group_start[g]
        rows = start[group_start[g + 1]] - start[group_start[g]]
        if distinct == 1:
            raise ValueError("zero-size array to reduction operation minimum which has no identity")
        if distinct < rows:
            raise ValueError("All arrays must be of the same length")
    x, y = np.asarray(cols["x"]), np.asarray(cols["y"])
    if three:
        pixelsize = 130 if pixelsize is None else pixelsize
        with np.errstate(all="ignore"):
            points = np.stack((x, y, np.asarray(cols["z"]) / pixelsize), axis=1)
    else:
        points = np.stack((x, y), axis=1)
    points = points.astype(np.float64)[order]
    min_dist, min_xy = np.zeros(len(order)), np.zeros(len(order))
    for g in range(len(group_start) - 1):
        a, b = start[group_start[g]], start[group_start[g + 1]]
        min_dist[a:b] = nearest_other(points, a, b)
        if three:
            min_xy[a:b] = nearest_other(points[:, :2], a, b)
    by_group = np.argsort(labels(cols["group"]), kind="stable")
    names = ("mean_frame", "x", "y") + (("z",) if three else ()) + ("std_frame", "lpx", "lpy") + (("lpz",) if three else ())
    out = {"group": np.asarray(cols["group"])[by_group], "cluster": seg_cluster.astype(np.asarray(cols["cluster"]).dtype)}
    with np.errstate(all="ignore"):
        for c in names:
            out[c] = np.asarray(cols[c])[by_group].astype(np.float32)
        out["n"] = np.asarray(cols["n"])[by_group].astype(np.int32)
        out["min_dist"] = min_dist.astype(np.float32)
        if three:
            out["mind_dist_xy"] = min_xy.astype(np.float32)
    return out
