"""Test-side restatement of the nearest-neighbour distances (picasso_amd/postprocess.py nn_analysis, picasso_amd/spinna.py
get_NN_dist): the brute-force float64 distance matrix, sorted, and the grid of csrc/knn_search.h (plan_grid, edge,
cell_of) in NumPy float64, which is the same IEEE arithmetic.  Used by make_goldens_nn.py to assert that a case holds
the situation it was written for, and by tests/test_nn_host.py as the second opinion."""
import math

import numpy as np

K_MAX = 32


def distances(X1, X2, k):
    """(N, k) float64: the k smallest sqrt(dx*dx + dy*dy (+ dz*dz)) of every row of X1 over X2, ascending, inf padded."""
    X1, X2 = np.asarray(X1, np.float64), np.asarray(X2, np.float64)
    n, m = len(X1), len(X2)
    out = np.full((n, k), np.inf)
    if m == 0 or n == 0:
        return out
    step = max(1, 2_000_000 // m)
    with np.errstate(over="ignore"):
        for a in range(0, n, step):
            q = X1[a:a + step]
            d = q[:, None, 0] - X2[None, :, 0]
            s = d * d
            for c in range(1, X1.shape[1]):
                d = q[:, None, c] - X2[None, :, c]
                s = s + d * d
            s = np.sqrt(s)
            s.sort(axis=1)
            out[a:a + step, :min(k, m)] = s[:, :k]
    return out


def nn_analysis(X1, X2, nn_count):
    """The self case asks for one neighbour more and leaves the first column out; one queried neighbour is a 1-D array."""
    own = int(np.array_equal(X1, X2))
    d = distances(X1, X2, nn_count + own)
    return d[:, 0] if d.shape[1] == 1 else d[:, own:]


def get_NN_dist(data1, data2, n_neighbors):
    """Always (N, n_neighbors), but a 1-D empty array when either set is empty."""
    if 0 in (len(data1), len(data2)):
        return np.zeros(0)
    own = int(np.array_equal(data1, data2))
    return distances(data1, data2, n_neighbors + own)[:, own:]


# ---- the grid of csrc/knn_search.h ----------------------------------------------------------------------------
class Grid:
    def __init__(self, X2, k):
        X2 = np.asarray(X2, np.float64)
        m = len(X2)
        lo, hi = (X2[:, :2].min(axis=0), X2[:, :2].max(axis=0)) if m else (np.zeros(2), np.zeros(2))
        per_cell = max((k + 1) // 2, 2)
        cells = max(m // per_cell, 1)
        with np.errstate(over="ignore"):
            ext = hi - lo
        flat = [not (e > 0.0 and e < np.inf) for e in ext]
        n = [1, 1]
        if not flat[0] and flat[1]:
            n[0] = cells
        if flat[0] and not flat[1]:
            n[1] = cells
        if not flat[0] and not flat[1]:
            with np.errstate(over="ignore"):
                t = np.sqrt(np.float64(cells) * (ext[0] / ext[1]))
            n[0] = cells if t >= cells else (int(t) if t >= 1.0 else 1)
            n[1] = max(cells // n[0], 1)
        w = [1.0, 1.0]
        for a in range(2):
            if not flat[a]:
                w[a] = ext[a] / np.float64(n[a])
            if not w[a] > 0.0:
                w[a], n[a] = 1.0, 1
        self.lo, self.w, self.n = [np.float64(v) for v in lo], [np.float64(v) for v in w], n

    def edge(self, a, i):
        return self.lo[a] + np.float64(i) * self.w[a]

    def cell_of(self, a, c):
        """Vectorised: the i with edge(i) <= c < edge(i + 1), the outer cells open-ended."""
        c = np.asarray(c, np.float64)
        if self.n[a] == 1:
            return np.zeros(c.shape, np.int64)
        edges = self.lo[a] + np.arange(1, self.n[a], dtype=np.float64) * self.w[a]
        return np.searchsorted(edges, c, side="right").astype(np.int64)

    def cells(self, X):
        X = np.asarray(X, np.float64)
        return self.cell_of(0, X[:, 0]), self.cell_of(1, X[:, 1])


def rings_needed(grid, X1, X2, k):
    """A lower bound on the rings the search of every query walks: the Chebyshev cell distance to its k-th nearest row."""
    qx, qy = grid.cells(X1)
    px, py = grid.cells(X2)
    out = np.zeros(len(X1), np.int64)
    kk = min(k, len(X2))
    for i in range(len(X1)):
        ring = np.maximum(np.abs(px - qx[i]), np.abs(py - qy[i]))
        out[i] = np.sort(ring)[kk - 1]
    return out


def ulps(v, steps):
    v = np.float64(v)
    for _ in range(abs(steps)):
        v = np.nextafter(v, np.float64(math.inf if steps > 0 else -math.inf))
    return v
