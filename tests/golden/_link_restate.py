"""A NumPy restatement of link and NeNA (picasso/postprocess.py:2441-2661, :1212-1272), written for the tests.

It follows the rules of DESIGN 8 N6 with another method than the reference's window scan: the candidate pairs come
from one k-d tree over (x / r, y / r, frame / k) in the maximum norm (a superset, then the exact test in the
columns' own arithmetic and the reference's row windows), the chains are replayed on the adjacency lists, the group
sums add the m-th member of every group in one vector step (so each group is summed in row order, in the column's
dtype), and the histogram is a bincount.  The tests check it against every array of tests/golden/link_cases.npz,
and the device against it on tables too large to store."""
import numpy as np
from scipy.spatial import cKDTree


def squared(d_max):
    """d_max ** 2 in the type numba gives d_max, as float64."""
    if isinstance(d_max, np.floating):
        return float(d_max * d_max)
    return float(d_max) * float(d_max)


def windows(frame, k, nena=False):
    """Rows [a, b) the reference's third loop scans for every current row (the last row has none: a = b = n)."""
    f = np.asarray(frame).astype(np.int64)
    n = len(f)
    lo = np.searchsorted(f, f + 1, side="left")
    hi = np.searchsorted(f, f + k, side="right")
    if nena:
        a, b = np.minimum(lo, n - 1), np.minimum(hi, n - 1)
    else:
        none = lo >= n
        a = np.where(none, n - 1, lo)
        b = np.where(none, np.where(f[n - 1] > f + k, n - 1, n), hi)
    a[n - 1] = b[n - 1] = n
    return a, b


def _pairs(frame, x, y, r, k):
    """i < j with |dx| <= r, |dy| <= r, |dframe| <= k, a little generously (float64)."""
    pts = np.stack([np.asarray(x, np.float64) / r, np.asarray(y, np.float64) / r,
                    np.asarray(frame).astype(np.float64) / max(k, 1)], axis=1)
    ok = np.isfinite(pts).all(axis=1)
    idx = np.flatnonzero(ok)
    p = cKDTree(pts[idx]).query_pairs(1.0 + 1e-5, p=np.inf, output_type="ndarray")
    p = idx[p]
    return np.minimum(p[:, 0], p[:, 1]), np.maximum(p[:, 0], p[:, 1])


def _within(x, y, i, j, r2):
    """(passes dx2 <= r2 and dy2 <= r2, dx2 + dy2) in the columns' types, compared in float64."""
    dx, dy = x[i] - x[j], y[i] - y[j]
    dx2, dy2 = dx * dx, dy * dy
    ok = (dx2.astype(np.float64) <= r2) & (dy2.astype(np.float64) <= r2)
    return ok, dx2 + dy2


def candidates(frame, x, y, group, d_max, k, nena=False):
    """The pairs (i, j), sorted by (i, j), that the reference's test accepts -> (i, j, dx2 + dy2)."""
    x, y, group = np.asarray(x), np.asarray(y), np.asarray(group)
    n = len(x)
    if n < 2:
        return np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0, np.result_type(x, y))
    a, b = windows(frame, k, nena)
    i, j = _pairs(frame, x, y, float(d_max), k)
    keep = (j >= a[i]) & (j < b[i]) & (group[i] == group[j])
    i, j = i[keep], j[keep]
    r2 = squared(d_max)
    ok, s = _within(x, y, i, j, r2)
    ok &= s.astype(np.float64) <= r2
    i, j, s = i[ok], j[ok], s[ok]
    order = np.lexsort((j, i))
    return i[order], j[order], s[order]


def link_groups(frame, x, y, d_max, max_dark_time, group):
    n = len(x)
    i, j, _ = candidates(frame, x, y, group, d_max, int(np.floor(max_dark_time + 1)))
    start = np.searchsorted(i, np.arange(n + 1))
    jl, sl = j.tolist(), start.tolist()
    out = [-1] * n
    current = -1
    for row in range(n):
        if out[row] != -1:
            continue
        current += 1
        out[row] = current
        cur = row
        while True:
            nxt = -1
            for q in range(sl[cur], sl[cur + 1]):
                if out[jl[q]] == -1:
                    nxt = jl[q]
                    break
            if nxt < 0:
                break
            out[nxt] = current
            cur = nxt
    return np.array(out, np.int32)


def nfndh(frame, x, y, group, d_max=1.0, bin_size=0.001):
    n = len(x)
    bins = np.arange(0, d_max, bin_size)
    i, j, s = candidates(frame, x, y, group, d_max, 1, nena=True)
    keep = i < 100 * int(n / 100)
    d = np.sqrt(s[keep])
    d = d[d.astype(np.float64) <= d_max]
    b = (d.astype(np.float64) / bin_size).astype(np.int64)
    b = b[b < len(bins)]
    return bins + bin_size / 2, np.bincount(b, minlength=len(bins)).astype(np.float64)


def ordered_sum(column, link_group, n_groups):
    """Per group the sum of `column` in row order, accumulated in the column's dtype."""
    column = np.asarray(column)
    order = np.argsort(link_group, kind="stable")
    count = np.bincount(link_group, minlength=n_groups)
    first = np.concatenate(([0], np.cumsum(count)[:-1]))
    acc = np.zeros(n_groups, column.dtype)
    with np.errstate(all="ignore"):
        for m in range(int(count.max()) if n_groups else 0):
            g = np.flatnonzero(count > m)
            acc[g] = acc[g] + column[order[first[g] + m]]
    return acc


def _mean(total, divisor):
    a, b = total.dtype, divisor.dtype
    if a.kind in "iu" and b.kind in "iu":
        dt = np.dtype(np.float64)
    else:
        dt = b if a.kind in "iu" else a if b.kind in "iu" else np.promote_types(a, b)
    with np.errstate(all="ignore"):
        return (total.astype(dt) / divisor.astype(dt)).astype(np.float32)


def link_loc_groups(cols, n_frames, link_group, remove_ambiguous_lengths=True):
    """cols: name -> sorted column, in the table's column order -> ordered dict of the combined columns."""
    n_groups = int(link_group.max()) + 1
    n_ = np.bincount(link_group, minlength=n_groups).astype(np.uint32)
    order = np.argsort(link_group, kind="stable")
    ends = np.cumsum(n_.astype(np.int64))
    starts = ends - n_
    out = {}

    def total(c):
        return ordered_sum(c, link_group, n_groups)

    def weighted(c, lp):
        w = 1 / cols[lp] ** 2
        sw = total(w)
        return _mean(total(cols[c] * w), sw), sw

    frame = cols["frame"]
    by_group = frame[order]
    first = np.minimum.reduceat(by_group, starts)
    last = np.maximum.reduceat(by_group, starts)
    out["frame"] = first
    out["x"], swx = weighted("x", "lpx")
    out["y"], swy = weighted("y", "lpy")
    if "photons" in cols:
        out["photons"] = total(cols["photons"])
    for c in ("sx", "sy"):
        if c in cols:
            out[c] = _mean(total(cols[c]), n_)
    if "bg" in cols:
        out["bg"] = total(cols["bg"])
    out["lpx"], out["lpy"] = np.sqrt(1 / swx), np.sqrt(1 / swy)
    for c in ("ellipticity", "net_gradient", "likelihood", "iterations"):
        if c in cols:
            out[c] = _mean(total(cols[c]), n_)
    if "z" in cols:
        if "lpz" in cols:
            out["z"], swz = weighted("z", "lpz")
            out["lpz"] = np.sqrt(1 / swz)
        else:
            out["z"] = _mean(total(cols["z"]), n_)
    if "d_zcalib" in cols:
        out["d_zcalib"] = _mean(total(cols["d_zcalib"]), n_)
    if "group" in cols:
        out["group"] = cols["group"][order[ends - 1]]
    out["len"] = last - first + 1
    out["n"] = n_
    if "photons" in cols:
        out["photon_rate"] = np.float32(out["photons"] / n_)
    if remove_ambiguous_lengths:
        valid = (first > 0) & (last < n_frames)
        out = {k: v[valid] for k, v in out.items()}
    return out
