"""A plain NumPy restatement of the reference's ``_undrift_from_picked_coordinate`` / ``undrift_from_picked``
(picasso/postprocess.py:3062-3156) over a CSR of pick members, operation for operation as csrc/fiducials.hip does it.
make_goldens_fiducials.py asserts that it equals the reference in every bit before it writes the goldens; the tests
hold the device against it where no golden is stored.

The sums: down the picks sequentially from row 0; along a row and over a pick's column NumPy's own ``add.reduce`` of a
contiguous 1-D array (``pairwise_reduce`` restates that one in Python: the pairwise sum of each 8192-element chunk,
added in order).
"""
import numpy as np

CHUNK = 8192


def _pairwise(v, T):
    n = len(v)
    if n < 8:
        res = T(0)
        for u in v:
            res = T(res + u)
        return res
    if n <= 128:
        r = [T(u) for u in v[:8]]
        i = 8
        while i < n - n % 8:
            for k in range(8):
                r[k] = T(r[k] + v[i + k])
            i += 8
        res = T(T(T(r[0] + r[1]) + T(r[2] + r[3])) + T(T(r[4] + r[5]) + T(r[6] + r[7])))
        for u in v[i:]:
            res = T(res + u)
        return res
    half = n // 2
    half -= half % 8
    return T(_pairwise(v[:half], T) + _pairwise(v[half:], T))


def pairwise_reduce(v):
    """np.add.reduce of a contiguous 1-D float array, restated."""
    v = np.ascontiguousarray(v)
    T = v.dtype.type
    acc = T(0)
    with np.errstate(all="ignore"):
        for lo in range(0, len(v), CHUNK):
            acc = T(acc + _pairwise(v[lo:lo + CHUNK], T))
    return acc


def csr(picked, names):
    """A list of per-pick column dicts / frames -> (offsets, frame, [columns])."""
    offsets = np.zeros(len(picked) + 1, np.int64)
    offsets[1:] = np.cumsum([len(p["frame"]) for p in picked])

    def cat(name):
        parts = [np.asarray(p[name]) for p in picked]
        return np.concatenate(parts) if parts else np.zeros(0)

    return offsets, cat("frame"), [cat(n) for n in names]


def drift_coordinate(offsets, frame, c, n_frames):
    """-> float64[n_frames]; raises IndexError / ValueError where NumPy does in the reference."""
    offsets, frame, c = np.asarray(offsets, np.int64), np.asarray(frame).astype(np.int64), np.asarray(c)
    P, F, T = len(offsets) - 1, int(n_frames), c.dtype.type
    D = np.full((P, F), np.nan)
    with np.errstate(all="ignore"):
        for p in range(P):
            a, b = offsets[p], offsets[p + 1]
            cp = np.ascontiguousarray(c[a:b])
            mean = T(np.add.reduce(cp) / T(b - a))
            f = frame[a:b].copy()
            f[f < 0] += F
            if ((f < 0) | (f >= F)).any():
                raise IndexError("frame out of bounds")
            d = (cp - mean).astype(np.float64)
            for k in range(len(f)):               # the row latest in the given order wins
                D[p, f[k]] = d[k]
        has = ~np.isnan(D)
        if P == 0:
            raise ValueError("array of sample points is empty")
        s = np.where(has[0], D[0], 0.0)
        for p in range(1, P):
            s = s + np.where(has[p], D[p], 0.0)
        m0 = s / has.sum(0)
        sd = (D - m0) * (D - m0)
        ok = ~np.isnan(sd)
        w = np.empty(P)
        for p in range(P):
            w[p] = 1.0 / (np.add.reduce(np.ascontiguousarray(np.where(ok[p], sd[p], 0.0))) / np.float64(ok[p].sum()))
        num = np.where(has[0], D[0] * w[0], 0.0)
        den = np.where(has[0], w[0] * 1.0, 0.0)
        for p in range(1, P):
            num = num + np.where(has[p], D[p] * w[p], 0.0)
            den = den + np.where(has[p], w[p] * 1.0, 0.0)
        y = num / den
        y[~has.any(0) | (np.abs(num) * np.finfo(np.float64).tiny >= np.abs(den))] = np.nan
        known = np.flatnonzero(~np.isnan(y))
        if len(known) == 0:
            raise ValueError("array of sample points is empty")
        out = y.copy()
        for f in np.flatnonzero(np.isnan(y)):
            j = np.searchsorted(known, f)
            if j == 0:
                out[f] = y[known[0]]
            elif j == len(known):
                out[f] = y[known[-1]]
            else:
                lo, hi = known[j - 1], known[j]
                slope = (y[hi] - y[lo]) / (np.float64(hi) - np.float64(lo))
                out[f] = slope * (np.float64(f) - np.float64(lo)) + y[lo]
    return out


def drift(offsets, frame, columns, n_frames):
    """-> float64 (n_frames, len(columns))"""
    return np.stack([drift_coordinate(offsets, frame, c, n_frames) for c in columns], axis=1)


def sort_members(frame, offsets, rows):
    """Each pick's rows in the order of the reference's sort_values(by="frame", kind="quicksort") on the pick's subset:
    the same NumPy sort on the subset's frame values alone."""
    rows = np.asarray(rows, np.int64).copy()
    for p in range(len(offsets) - 1):
        a, b = offsets[p], offsets[p + 1]
        rows[a:b] = rows[a:b][np.argsort(frame[rows[a:b]], kind="quicksort")]
    return rows
