"""Test-side restatement of the local density, the distance histogram and the pair correlation of
picasso.postprocess, by another method than the reference's loops and the device's bisections: candidate pairs from a
SciPy k-d tree, then the block-offset, visibility and wrap rules as array operations, then ``bincount``.

TEST INFRASTRUCTURE (CPU only).  The rules, as tests/golden/pairs_cases.npz records the reference:

  blocks       x_index = uint32(x / size) in the column's own dtype, K x L = ceil(Height / size) x ceil(Width / size),
               rows in np.lexsort([x_index, y_index]) order
  visibility   p = the first sorted position whose block lies outside the grid; only positions < p are ever neighbours
  density      position i counts position j < p once for every (dk, dl) in {-1, 0, 1}^2 with
               wrap(ki + dk) == kj and wrap(li + dl) == lj, where wrap(-1) is the last block and an index >= K / L
               matches nothing; the pair must pass dx2 < r2, dy2 < r2, dx2 + dy2 < r2
  histogram    positions a < b < p with block(b) - block(a) in {(0, 0), (0, 1), (1, 0), (1, 1)}, dx2 < r2, dy2 < r2,
               d = sqrt(dx2 + dy2) < r_max, bin = floor(d / bin_size) < uint32(r_max / bin_size)
  arithmetic   differences, squares, their sum and the root in the columns' common dtype, comparisons in float64
"""
import numpy as np
from scipy.spatial import cKDTree

SANITY_COLUMNS = ("x", "y", "lpx", "lpy", "lpz", "photons", "ellipticity", "sx", "sy")


def squared(r) -> float:
    if isinstance(r, np.floating):
        return float(r * r)
    if isinstance(r, (int, np.integer)):
        return float(int(r) * int(r))
    return float(r) * float(r)


def sane_rows(cols, info) -> np.ndarray:
    """Rows the sanity filter keeps: every column finite, x < Width, y < Height, the listed columns >= 0."""
    n = len(cols["x"])
    ok = np.ones(n, bool)
    for v in cols.values():
        if np.asarray(v).dtype.kind == "f":
            ok &= np.isfinite(v)
    with np.errstate(invalid="ignore"):
        ok &= (cols["x"] < info["Width"]) & (cols["y"] < info["Height"])
        for c in SANITY_COLUMNS:
            if c in cols:
                ok &= cols[c] >= 0
    return np.flatnonzero(ok)


class Blocks:
    """The sane rows of a table in block order."""

    def __init__(self, cols, info, size):
        self.kept = sane_rows(cols, info)
        x, y = np.asarray(cols["x"])[self.kept], np.asarray(cols["y"])[self.kept]
        xi, yi = np.uint32(x / size), np.uint32(y / size)
        self.K, self.L = int(np.ceil(info["Height"] / size)), int(np.ceil(info["Width"] / size))
        self.perm = np.lexsort([xi, yi])
        self.index = self.kept[self.perm]                     # the caller's row of every sorted position
        self.x, self.y = x[self.perm], y[self.perm]
        self.li, self.ki = xi[self.perm].astype(np.int64), yi[self.perm].astype(np.int64)
        self.x_index, self.y_index = xi[self.perm], yi[self.perm]
        outside = (self.li >= self.L) | (self.ki >= self.K)
        self.n = len(x)
        self.p = int(np.argmax(outside)) if outside.any() else self.n
        self.S = np.result_type(self.x.dtype, self.y.dtype)

    def close_pairs(self, r):
        """Every unordered pair of sorted positions (a < b) closer than a hair more than r, as two arrays."""
        if self.n < 2:
            return np.zeros(0, np.int64), np.zeros(0, np.int64)
        pts = np.stack([self.x.astype(np.float64), self.y.astype(np.float64)], axis=1)
        pairs = cKDTree(pts).query_pairs(float(r) * (1 + 1e-5) + 1e-12, output_type="ndarray")
        a, b = pairs.min(axis=1), pairs.max(axis=1)
        return a.astype(np.int64), b.astype(np.int64)

    def squares(self, a, b):
        dx = self.x[a] - self.x[b]
        dy = self.y[a] - self.y[b]
        return dx * dx, dy * dy


def _matches(ci, cj, count):
    """How many of ci - 1, ci, ci + 1 name block cj: -1 wraps to count - 1, an index >= count names nothing."""
    m = np.zeros(len(ci), np.int64)
    for d in (-1, 0, 1):
        c = ci + d
        c = np.where(c < 0, c + count, c)
        m += (c >= 0) & (c < count) & (c == cj)
    return m


def local_density(cols, info, radius, true_counts=False):
    """-> (Blocks, uint64 density by sorted position).  true_counts: every row within the radius, no block rules."""
    b = Blocks(cols, info, radius)
    r2 = squared(radius)
    lo, hi = b.close_pairs(radius)
    i = np.concatenate([lo, hi, np.arange(b.n)])
    j = np.concatenate([hi, lo, np.arange(b.n)])
    dx2, dy2 = b.squares(i, j)
    ok = (dx2.astype(np.float64) < r2) & (dy2.astype(np.float64) < r2)
    ok &= (dx2.astype(b.S) + dy2.astype(b.S)).astype(np.float64) < r2
    if true_counts:
        weight = ok.astype(np.int64)
    else:
        weight = ok * (j < b.p) * _matches(b.ki[i], b.ki[j], b.K) * _matches(b.li[i], b.li[j], b.L)
    density = np.zeros(b.n, np.int64)
    np.add.at(density, i, weight)
    return b, density.astype(np.uint64)


def histogram_pairs(b, r_max):
    """(a, b, d) of the pairs that pass the distance tests, whatever their blocks."""
    r2 = squared(r_max)
    lo, hi = b.close_pairs(r_max)
    dx2, dy2 = b.squares(lo, hi)
    d = np.sqrt(dx2.astype(b.S) + dy2.astype(b.S))
    ok = (dx2.astype(np.float64) < r2) & (dy2.astype(np.float64) < r2) & (d.astype(np.float64) < r_max)
    return lo[ok], hi[ok], d[ok]


def distance_histogram(cols, info, bin_size, r_max, with_pairs=False):
    b = Blocks(cols, info, r_max)
    n_bins = int(np.uint32(r_max / bin_size))
    lo, hi, d = histogram_pairs(b, r_max)
    dk, dl = b.ki[hi] - b.ki[lo], b.li[hi] - b.li[lo]
    counted = (hi < b.p) & (dk >= 0) & (dk <= 1) & (dl >= 0) & (dl <= 1)
    q = np.floor(d[counted].astype(np.float64) / bin_size)
    q = q[q < n_bins].astype(np.int64)
    dh = np.bincount(q, minlength=n_bins).astype(np.uint64)[:n_bins]
    if with_pairs:
        return dh, b, (lo, hi, d, dk, dl, counted)
    return dh


def pair_correlation(cols, info, bin_size, r_max):
    dh = distance_histogram(cols, info, bin_size, r_max)
    lower = np.arange(bin_size, r_max + bin_size, bin_size)
    if len(lower) > len(dh):
        lower = lower[:-1]
    return lower, dh / (np.pi * bin_size * (2 * lower + bin_size))
