"""Test-side restatement of the reference's ``_dark_times`` / ``dark_times`` / ``compute_dark_times``
(picasso/postprocess.py:1920-2004) and ``groupprops`` (:3580-3649), by another method than csrc/kinetics.hip.

TEST INFRASTRUCTURE, NumPy only.

Dark times: ``np.lexsort`` by (group, last_frame), then per group one ``np.searchsorted`` of the frames in the group's
sorted last frames; the row itself is stepped over where it is the best candidate.  Differences are signed int64.

Group properties: what pandas 2.3 ``Series.mean()`` / ``Series.std()`` compute (pandas/core/nanops.py nanmean, nanvar,
nanstd without bottleneck), with ``ndarray.sum()`` restated as NumPy's ``add.reduce`` of a contiguous 1-D array runs it:
the accumulator starts at 0 and takes the pairwise sum of every 8192-element chunk in order.  The pairwise sum is
written with 8-wide array additions, which round as eight scalar accumulators do.
"""
import numpy as np

CHUNK = 8192          # np.getbufsize()


def _leaf(a, T):
    n = len(a)
    if n < 8:
        res = T(0)
        for v in a:
            res = T(res + v)
        return res
    r = a[:8].copy()
    full = n - n % 8
    for i in range(8, full, 8):
        r += a[i:i + 8]
    res = T(T(T(r[0] + r[1]) + T(r[2] + r[3])) + T(T(r[4] + r[5]) + T(r[6] + r[7])))
    for v in a[full:]:
        res = T(res + v)
    return res


def _pairwise(a, T):
    n = len(a)
    if n <= 128:
        return _leaf(a, T)
    half = n // 2
    half -= half % 8
    return T(_pairwise(a[:half], T) + _pairwise(a[half:], T))


def chunked_sum(a, dtype):
    """``np.asarray(a).sum(dtype=dtype)`` of a contiguous 1-D array, in bits."""
    T = np.dtype(dtype).type
    a = np.ascontiguousarray(a).astype(T)
    acc = T(0)
    with np.errstate(all="ignore"):
        for lo in range(0, len(a), CHUNK):
            acc = T(acc + _pairwise(a[lo:lo + CHUNK], T))
    return acc


def series_mean(v):
    """pandas ``Series(v).mean()`` -> a NumPy scalar of the summing type."""
    v = np.asarray(v)
    T = v.dtype.type if v.dtype.kind == "f" else np.float64
    if v.dtype.kind == "f":
        nan = np.isnan(v)
        count = T(len(v) - int(nan.sum()))
        total = chunked_sum(np.where(nan, T(0), v), T)
    else:
        count, total = T(len(v)), chunked_sum(v, T)
    with np.errstate(all="ignore"):
        return T(total / count) if count > 0 else T(np.nan)


def series_std(v):
    """pandas ``Series(v).std()`` (ddof 1) -> float32 for a float32 column, float64 otherwise."""
    v = np.asarray(v)
    T = v.dtype.type if v.dtype.kind == "f" else np.float64
    vals = v.astype(T)
    nan = np.isnan(vals)
    count = T(len(v) - int(nan.sum()))
    if not count > 1:
        return T(np.nan)
    with np.errstate(all="ignore"):
        vals = np.where(nan, T(0), vals)
        avg = np.float64(chunked_sum(vals, np.float64)) / count            # float64 / float32 -> float64
        terms = (np.float64(avg) - vals.astype(np.float64)) ** 2
        terms[nan] = 0.0
        var = chunked_sum(terms, np.float64) / (count - T(1))
        return np.sqrt(T(var))


def groupprops(cols):
    """``cols``: column name -> array, with ``group`` and ``dark`` among them -> (OrderedDict-like dict of the result's
    columns, in the reference's order and dtypes)."""
    keep = cols["dark"] != -1
    cols = {c: np.asarray(v)[keep] for c, v in cols.items()}
    ids = np.unique(cols["group"])
    order = np.argsort(cols["group"], kind="stable")
    bounds = np.searchsorted(cols["group"][order], ids, side="left").tolist() + [len(order)]
    out = {"group": ids.astype(np.float64).astype(np.int32),
           "n_events": np.diff(bounds).astype(np.float64).astype(np.int32)}
    with np.errstate(all="ignore"):
        for c, v in cols.items():
            vs = v[order]
            runs = [vs[a:b] for a, b in zip(bounds[:-1], bounds[1:])]
            for stat, fn in (("_mean", series_mean), ("_std", series_std)):
                held = np.array([np.float64(fn(r)) for r in runs], np.float64)
                held[np.isnan(held)] = np.nan          # DataFrame.loc stores any NaN as pandas' own, sign and payload dropped
                out[c + stat] = held.astype(np.float32)
        out["qpaint_idx"] = np.float32(1) / out["dark_mean"]
    return out


def last_frames(frame, length):
    with np.errstate(all="ignore"):
        return frame + length - 1


def dark_array(frame, group, last_frame):
    """``_dark_times(frame, group, last_frame)``: the dtype numba gives ``max_frame * np.ones(N, np.int32)``."""
    frame, group, last_frame = np.asarray(frame), np.asarray(group), np.asarray(last_frame)
    n = len(frame)
    f, lf = frame.astype(np.int64), last_frame.astype(np.int64)
    max_frame = int(f.max())
    dark = np.full(n, -1, np.result_type(frame.dtype, np.int32))
    order = np.lexsort((lf, group))
    gs, lfs = group[order], lf[order]
    cuts = np.flatnonzero(np.r_[True, gs[1:] != gs[:-1], True])
    where = np.empty(n, np.int64)
    where[order] = np.arange(n)
    for a, b in zip(cuts[:-1], cuts[1:]):
        rows = order[a:b]
        p = a + np.searchsorted(lfs[a:b], f[rows], side="left") - 1      # the last sorted position below the frame
        p = np.where(p == where[rows], p - 1, p)
        ok = p >= a
        d = f[rows] - lfs[np.maximum(p, a)]
        ok &= d < max_frame
        dark[rows[ok]] = d[ok]
    return dark


def dark_times(cols, group=None):
    frame, length = np.asarray(cols["frame"]), np.asarray(cols["len"])
    if group is None:
        group = cols["group"] if "group" in cols else np.zeros(len(frame))
    return dark_array(frame, group, last_frames(frame, length))
