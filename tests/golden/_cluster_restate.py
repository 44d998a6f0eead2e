"""Test-side restatement of the SMLM clusterer, DBSCAN and the frame analysis of picasso.clusterer as functions of
the data, in NumPy / scipy array operations: candidate pairs from a KD-tree with a hair more than the radius, the
exact float64 predicate on them, then scatter-maxima / minima over the pair list and scipy's connected components.
Neither the reference's loops nor the kernels' cell sort, union-find or pointer jumping appear here.

    neighbours      j is a neighbour of i (i included) iff dx*dx + dy*dy (+ dz*dz) <= r*r in float64
    _cluster        local maximum: n_i > min_locs and n_i = max n over the neighbours, numbered in row order;
                    fresh: no lower-indexed maximum among its neighbours; a row takes the number of its
                    highest-indexed fresh neighbour, else the label of its lowest-indexed neighbour maximum, else -1
    _dbscan         core: n_i >= min_samples; clusters = components of the core rows, numbered by their lowest row;
                    a border row takes the lowest number among its core neighbours
    both            labels with fewer than min_locs rows -> -1
"""
import numpy as np
from scipy.sparse import coo_matrix
from scipy.sparse.csgraph import connected_components
from scipy.spatial import cKDTree


def neighbour_edges(X, radius):
    """(src, dst) of every ordered neighbour pair, every row with itself included."""
    X = np.asarray(X, np.float64)
    n = len(X)
    r = float(radius)
    pairs = cKDTree(X).query_pairs(r * (1 + 1e-9) + 1e-300, output_type="ndarray")
    d = X[pairs[:, 0]] - X[pairs[:, 1]]
    s = d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]
    if X.shape[1] == 3:
        s = s + d[:, 2] * d[:, 2]
    pairs = pairs[s <= r * r]
    me = np.arange(n)
    return np.concatenate([pairs[:, 0], pairs[:, 1], me]), np.concatenate([pairs[:, 1], pairs[:, 0], me])


def neighbour_counts(X, radius):
    src, _ = neighbour_edges(X, radius)
    return np.bincount(src, minlength=len(X)).astype(np.int32)


def drop_small(labels, min_locs):
    values, counts = np.unique(labels, return_counts=True)
    labels[np.isin(labels, values[counts < min_locs])] = -1
    return labels


def frame_analysis(labels, frame):
    labels = labels.copy()
    frame = np.asarray(frame)
    n_frames = frame.max() + 1
    edges = np.linspace(0, n_frames, 21)
    values, ids = np.unique(labels, return_inverse=True)
    ids = ids.reshape(-1)
    count = np.bincount(ids, minlength=len(values))
    mean = np.bincount(ids, weights=frame.astype(np.float64), minlength=len(values)) / count
    which = np.clip(np.searchsorted(edges, frame.astype(np.float64), side="right") - 1, 0, 19)
    hist = np.bincount(ids * 20 + which, minlength=20 * len(values)).reshape(len(values), 20)
    failed = (mean < 0.2 * n_frames) | (mean > 0.8 * n_frames) | (hist.max(axis=1) > 0.8 * count)
    labels[np.isin(labels, values[failed])] = -1
    return labels


def smlm_parts(X, radius, min_locs):
    """counts, local maxima, fresh maxima and the labels before the size filter."""
    n = len(X)
    src, dst = neighbour_edges(X, radius)
    counts = np.bincount(src, minlength=n)
    top = np.zeros(n, np.int64)
    np.maximum.at(top, src, counts[dst])
    lm = (counts > min_locs) & (counts == top)
    number = np.cumsum(lm) - 1
    to_lm = lm[dst]
    lower = np.zeros(n, bool)
    lower[src[to_lm & (dst < src)]] = True
    fresh = lm & ~lower
    to_fresh = fresh[dst]
    high_fresh = np.full(n, -1, np.int64)
    np.maximum.at(high_fresh, src[to_fresh], dst[to_fresh])
    low_lm = np.full(n, n, np.int64)
    np.minimum.at(low_lm, src[to_lm], dst[to_lm])
    labels = np.full(n, -1, np.int32)
    direct = high_fresh >= 0
    labels[direct] = number[high_fresh[direct]]
    chained = ~direct & (low_lm < n)
    for i in np.flatnonzero(chained & lm):          # ascending: the maximum it points at is a lower row, already set
        labels[i] = labels[low_lm[i]]
    rest = chained & ~lm
    labels[rest] = labels[low_lm[rest]]
    return {"counts": counts.astype(np.int32), "lm": lm, "fresh": fresh, "chained": chained & lm, "labels": labels,
            "n_fresh_neighbours": np.bincount(src[to_fresh], minlength=n)}


def cluster(X, radius, min_locs, frame=None):
    labels = drop_small(smlm_parts(X, radius, min_locs)["labels"], min_locs)
    if frame is not None:
        labels = frame_analysis(labels, frame)
    return labels


def dbscan_parts(X, radius, min_samples):
    n = len(X)
    src, dst = neighbour_edges(X, radius)
    counts = np.bincount(src, minlength=n)
    core = counts >= min_samples
    both = core[src] & core[dst]
    graph = coo_matrix((np.ones(both.sum(), np.int8), (src[both], dst[both])), shape=(n, n)).tocsr()
    _, comp = connected_components(graph, directed=False)
    root = np.full(comp.max() + 1 if n else 0, n, np.int64)
    np.minimum.at(root, comp[core], np.flatnonzero(core))
    roots = np.sort(root[root < n])
    labels = np.full(n, -1, np.int64)
    labels[core] = np.searchsorted(roots, root[comp[core]])
    to_core = core[dst] & ~core[src]
    best = np.full(n, np.iinfo(np.int64).max)
    np.minimum.at(best, src[to_core], labels[dst[to_core]])
    border = ~core & (best < np.iinfo(np.int64).max)
    labels[border] = best[border]
    return {"core": core, "border": border, "labels": labels.astype(np.int32), "src": src, "dst": dst}


def dbscan(X, radius, min_samples, min_locs=0):
    return drop_small(dbscan_parts(X, radius, min_samples)["labels"], min_locs)


def points(cols, kw):
    """The points cluster() hands to _cluster and dbscan() hands to _dbscan for a table given as a dict of columns:
    z goes from nm to pixels and is scaled by radius / radius_z, in the columns' own dtype."""
    import pandas as pd
    locs = pd.DataFrame(cols)
    if "z" not in cols:
        X = locs[["x", "y"]].to_numpy()
        return X, X
    scaled = locs.copy()
    scaled["z"] /= kw["pixelsize"]
    for_cluster = scaled[["x", "y", "z"]].to_numpy()
    for_dbscan = locs[["x", "y", "z"]].to_numpy()
    for_dbscan[:, 2] /= kw["pixelsize"]
    if kw.get("radius_z") is not None:
        for_cluster[:, 2] *= kw["radius"] / kw["radius_z"]
        for_dbscan[:, 2] *= kw["radius"] / kw["radius_z"]
    return for_cluster, for_dbscan
