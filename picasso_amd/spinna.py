"""The nearest-neighbour distances of SPINNA (picasso/spinna.py:696-747 ``get_NN_dist``) on top of csrc/knn.hip.
Nothing else of picasso.spinna is here: the mixer, the simulations and the fit stay the reference's own and call this
function once it is installed (``localize.install(picasso_spinna=...)``)."""
from __future__ import annotations

import numpy as np

from .postprocess import _kdtree_points, _knn_table

SPINNA_NAMES = ("get_NN_dist",)


def get_NN_dist(data1, data2, n_neighbors: int) -> np.ndarray:
    """Distances from every point of ``data1`` to its ``n_neighbors`` nearest points of ``data2``, shape
    (N, n_neighbors), float64, in every bit what the reference's KDTree query returns; when the two sets hold the same
    values the point itself is not counted.  An empty set returns ``np.array([])``."""
    if min(len(data1), len(data2)) == 0:
        return np.array([])
    if data1.shape[1] != data2.shape[1]:
        raise ValueError("data1 and data2 must have the same number of dimensions.")
    own = int(np.array_equal(data1, data2))      # 1: every point finds itself first, at distance 0
    points = _kdtree_points(data2)
    total = int(n_neighbors) + own
    if own and total == 1:                       # nothing but the point itself: no search, no column
        return np.empty((len(points), 0))
    return _knn_table(points, data1, total)[:, own:]
