"""The cluster areas of picasso.clusterer (picasso/clusterer.py:1068-1237: _cluster_area, cluster_areas,
test_subclustering; picasso/masking.py:408-446 threshold_otsu) restated in plain NumPy, operation for operation as
csrc/areas.hip runs them: NumPy's ``arange`` of scalars, ``histogramdd``'s binning, SciPy's ``gaussian_filter`` at
sigma 2 and ``np.histogram(., 256)`` with the Otsu sums.  TEST INFRASTRUCTURE: the tests compare the device with it,
and it with the arrays the reference recorded (areas_cases.npz) and with NumPy / SciPy themselves.

Nothing here calls SciPy.  Every function works on one group; ``areas()`` is the loop over a table.
"""
import math
import warnings

import numpy as np
import pandas as pd

RADIUS = 8                      # int(4.0 * 2 + 0.5): gaussian_filter's truncate 4 at sigma 2
OTSU_BINS = 256
MAX_BINS = 1 << 24              # bins of one image; PMI_AREAS_MAX_BINS of the header


def weights(sigma=2.0, radius=RADIUS) -> np.ndarray:
    """scipy.ndimage._filters._gaussian_kernel1d(sigma, 0, radius): the 17 float64 weights."""
    sigma2 = sigma * sigma
    x = np.arange(-radius, radius + 1)
    phi = np.exp(-0.5 / sigma2 * x ** 2)
    return phi / phi.sum()


# ---- edges --------------------------------------------------------------------------------------------------
def arange(start, stop, step) -> np.ndarray:
    """``np.arange(start, stop, step)`` of NumPy scalars: the length is ceil((stop - start) / step) with the
    subtraction and the division in the scalars' own type, the result float64 with the values
    ``start + i * delta``, ``delta = float64(start + step) - float64(start)`` (and entry 1 is ``start + step``)."""
    with np.errstate(all="ignore"):
        q = (stop - start) / step
        nxt = start + step
    v = math.ceil(float(q)) if math.isfinite(float(q)) else float(q)
    if math.isnan(v):
        raise ValueError("arange: cannot compute length")
    if math.isinf(v):
        raise ValueError("Maximum allowed size exceeded")
    n = max(int(v), 0) if math.isfinite(v) else 0
    if n > MAX_BINS + 1:
        raise MemoryError(f"{n} edges")
    s = np.float64(start)
    delta = np.float64(nxt) - s
    out = s + np.arange(n, dtype=np.float64) * delta
    if n > 0:
        out[0] = s
    if n > 1:
        out[1] = np.float64(nxt)
    return out


def edges_of(X: np.ndarray, lp) -> list:
    """The edge arrays of _cluster_area (clusterer.py:1086-1098) for the points X in their own dtype."""
    bin_size = lp / 2
    sizes = [bin_size, bin_size] + ([bin_size * 2.5] if X.shape[1] == 3 else [])
    return [arange(X[:, d].min(), X[:, d].max() + sizes[d], sizes[d]) for d in range(X.shape[1])]


# ---- histogram ----------------------------------------------------------------------------------------------
def histogram(X: np.ndarray, edges: list) -> np.ndarray:
    """``np.histogramdd(X, bins=edges)[0]``: float64 counts; searchsorted from the right, a value on the last edge in
    the last bin, rows outside dropped.  An axis of e edges has max(e - 1, 0) bins."""
    shape = tuple(max(len(e) - 1, 0) for e in edges)
    image = np.zeros(shape, np.float64)
    if image.size == 0:
        return image
    inside = np.ones(len(X), bool)
    index = []
    for d, e in enumerate(edges):
        v = X[:, d].astype(np.float64)
        k = np.searchsorted(e, v, side="right")
        k[v == e[-1]] -= 1
        inside &= (k >= 1) & (k <= len(e) - 1)
        index.append(k - 1)
    np.add.at(image, tuple(i[inside] for i in index), 1.0)
    return image


# ---- blur ---------------------------------------------------------------------------------------------------
def reflect(p: np.ndarray, n: int) -> np.ndarray:
    """Positions of a line of n samples extended by half-sample-symmetric reflection (d c b a | a b c d | d c b a)."""
    m = np.mod(p, 2 * n)
    return np.where(m < n, m, 2 * n - 1 - m)


def blur(image: np.ndarray, w: np.ndarray = None) -> np.ndarray:
    """``scipy.ndimage.gaussian_filter(image, sigma=2)`` of a float64 image: axis after axis, per sample
    ``tmp = line[l] * w[8]`` and then, for j = 8 .. 1, ``tmp += (line[l - j] + line[l + j]) * w[8 - j]``."""
    w = weights() if w is None else w
    r = (len(w) - 1) // 2
    out = np.array(image, np.float64)
    if out.size == 0:
        return out
    for axis in range(out.ndim):
        src = np.moveaxis(out, axis, 0)
        n = src.shape[0]
        at = np.arange(n)
        tmp = src * w[r]
        for j in range(r, 0, -1):
            tmp = tmp + (src[reflect(at - j, n)] + src[reflect(at + j, n)]) * w[r - j]
        out = np.ascontiguousarray(np.moveaxis(tmp, 0, axis))
    return out


# ---- Otsu ---------------------------------------------------------------------------------------------------
def otsu_edges(values: np.ndarray):
    """(first, last, the 257 edges) of ``np.histogram(values, 256)``: np.linspace over the range of the values,
    widened by 0.5 when they are constant, (0, 1) when there are none."""
    if values.size == 0:
        first, last = 0.0, 1.0
    else:
        first, last = float(values.min()), float(values.max())
    if first == last:
        first, last = first - 0.5, last + 0.5
    step = (last - first) / OTSU_BINS
    e = np.arange(OTSU_BINS + 1, dtype=np.float64) * step + first
    e[-1] = last
    return first, last, e


def otsu_counts(values: np.ndarray):
    """(counts, edges) of ``np.histogram(values, 256)`` on NumPy's path for uniform bins: the index
    ``((v - first) / (last - first)) * 256`` truncated, 256 put into 255, then one step down where the value lies
    below its bin's edge and one step up where it reaches the next one."""
    values = np.asarray(values, np.float64).reshape(-1)
    first, last, e = otsu_edges(values)
    k = (((values - first) / (last - first)) * OTSU_BINS).astype(np.intp)
    k[k == OTSU_BINS] -= 1
    k[values < e[k]] -= 1
    k[(values >= e[k + 1]) & (k != OTSU_BINS - 1)] += 1
    return np.bincount(k, minlength=OTSU_BINS).astype(np.int64), e


def otsu(values: np.ndarray) -> float:
    """masking.threshold_otsu: float32 counts, the two float32 and the two float64 running sums added one by one,
    0 / 0 left as NaN, the first NaN or else the first maximum."""
    counts, e = otsu_counts(values)
    c = counts.astype(np.float32)
    centers = (e[:-1] + e[1:]) / 2.0
    n = OTSU_BINS
    w1, w2 = np.zeros(n, np.float32), np.zeros(n, np.float32)
    s1, s2 = np.zeros(n, np.float64), np.zeros(n, np.float64)
    prod = c * centers
    a, b = np.float32(0), np.float64(0)
    for i in range(n):
        a, b = np.float32(a + c[i]), b + prod[i]
        w1[i], s1[i] = a, b
    a, b = np.float32(0), np.float64(0)
    for i in range(n - 1, -1, -1):
        a, b = np.float32(a + c[i]), b + prod[i]
        w2[i], s2[i] = a, b
    with np.errstate(all="ignore"):
        m1, m2 = s1 / w1, s2 / w2
        d = m1[:-1] - m2[1:]
        var = (w1[:-1] * w2[1:]) * (d * d)
    nan = np.flatnonzero(np.isnan(var))
    best = 0
    if len(nan):
        best = int(nan[0])
    else:
        for i in range(1, n - 1):
            if var[i] > var[best]:
                best = i
    return centers[best]


# ---- one group, one table -----------------------------------------------------------------------------------
def cluster_image(X: np.ndarray, lp) -> np.ndarray:
    """The blurred image of one group."""
    return blur(histogram(X, edges_of(X, lp)))


def cluster_area(X: np.ndarray, lp) -> float:
    image = cluster_image(X, lp)
    count = int(np.sum(image >= otsu(image.reshape(-1))))
    return count / (16 / 5) if X.shape[1] == 3 else count / 4


def pixelsize_of(info):
    for d in reversed([info] if isinstance(info, dict) else info):
        if "Pixelsize" in d:
            return d["Pixelsize"]
    raise KeyError("Key 'Pixelsize' not found in metadata.")


def median_lp(cols):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return np.median(pd.DataFrame({"lpx": cols["lpx"], "lpy": cols["lpy"]}).mean(axis=1))


def points(cols, rows, pixelsize) -> np.ndarray:
    """``grouplocs[["x", "y"(, "z")]].to_numpy()`` with z in pixels: the common dtype of the columns."""
    names = ["x", "y"] + (["z"] if "z" in cols else [])
    dtype = np.result_type(*(cols[c].dtype for c in names))
    X = np.stack([cols[c][rows].astype(dtype) for c in names], axis=1)
    if "z" in cols:
        X[:, 2] /= pixelsize
    return X


def areas(cols: dict, info):
    """cluster_areas (clusterer.py:1112-1169) on a table given as a dict of columns ->
    (the name of the value column, int32 groups, float32 values)."""
    assert "group" in cols, "Localizations must contain 'group' column."
    pixelsize = pixelsize_of(info)
    groups = np.unique(cols["group"])
    key = "Area (LP^2)" if "z" not in cols else "Volume (LP^3)"
    out = np.zeros(len(groups), np.float32)
    lp = median_lp(cols)
    for i, g in enumerate(groups):
        out[i] = cluster_area(points(cols, np.flatnonzero(cols["group"] == g), pixelsize), lp)
    return key, groups.astype(np.int32), out


def subclustering(cols: dict, info, clustering_dist=25, sparse_dist=80):
    """test_subclustering (clusterer.py:1172-1237) with a brute-force nearest neighbour: dx * dx + dy * dy (+ dz * dz)
    summed in that order in float64, the square root of the smallest sum over the other rows."""
    assert "n_events" in cols, "The input molecules must have n_events attribute."
    assert sparse_dist > clustering_dist, "The sparse distance must be larger than the clustering distance."
    pixelsize = pixelsize_of(info)
    X = points(cols, np.arange(len(cols["x"])), pixelsize).astype(np.float64)
    d2 = np.zeros((len(X), len(X)))
    for a in range(X.shape[1]):
        diff = X[:, None, a] - X[None, :, a]
        d2 = d2 + diff * diff
    np.fill_diagonal(d2, np.inf)
    nnd = np.sqrt(d2.min(axis=1)) if len(X) > 1 else np.full(len(X), np.inf)
    close = np.flatnonzero(nnd < clustering_dist / pixelsize)
    far = np.flatnonzero(nnd >= sparse_dist / pixelsize)
    return cols["n_events"][close], cols["n_events"][far]
