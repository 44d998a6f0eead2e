"""DBSCAN and the SMLM clusterer of picasso.clusterer (picasso/clusterer.py:34-544, :665-691) on top of
csrc/cluster.hip: the same signatures, defaults, warnings, errors, dtypes, ``info`` entries and column handling,
and the same int32 label for every row.

The table handling stays the reference's own NumPy / pandas calls on the same dtypes (``z /= pixelsize`` on the
float32 column, the float32 ``X[:, 2] *= radius_xy / radius_z``, the widening to float64 that its KDTree and
sklearn do); the neighbour search, the local maxima, the union of core rows, the label sizes and the frame
analysis run on the device.  ``hdbscan``, ``find_cluster_centers``, ``cluster_areas`` and ``test_subclustering``
are not here: they stay the reference's and work on the tables these functions return.

Edges, as the reference has them: an empty table gives empty labels from ``_cluster`` (and a ``ValueError`` from
the frame analysis, which takes the maximum of no frames), a ``ValueError`` from ``_dbscan`` (sklearn wants one
sample) and a ``ZeroDivisionError`` from ``cluster`` / ``dbscan``; coordinates that are not finite raise
``ValueError`` (scipy's KDTree and sklearn both refuse them).
"""
from __future__ import annotations

import numpy as np
import pandas as pd

from . import __version__, backend, lib

# what localize.install() rebinds on picasso.clusterer
CLUSTERER_NAMES = ("_frame_analysis", "frame_analysis", "_cluster", "cluster_2D", "cluster_3D", "cluster", "_dbscan",
                   "dbscan", "extract_valid_labels")
_FA_BINS = 20


def _fa_limits(n_frames):
    """(lowest mean, highest mean, bin edges) of the frame analysis of a measurement of n_frames frames."""
    return 0.2 * n_frames, 0.8 * n_frames, np.linspace(0, n_frames, _FA_BINS + 1)


def _frame_analysis(frame, n_frames: int) -> int:
    """1 if the frames of one cluster pass the frame analysis, else 0: the mean frame lies within [20, 80] % of
    the measurement and no 1/20th of it holds more than 80 % of the localizations (clusterer.py:34-73).  One
    cluster on the host; ``frame_analysis`` checks all clusters of a table on the device."""
    lowest, highest, edges = _fa_limits(n_frames)
    mean_frame = frame.mean()
    fullest = np.histogram(frame, bins=edges)[0].max()
    return int(not (mean_frame < lowest or mean_frame > highest or fullest > 0.8 * len(frame)))


def frame_analysis(labels: np.ndarray, frame: np.ndarray) -> np.ndarray:
    """Set the labels of the clusters that fail the frame analysis to -1, IN PLACE, and return them
    (clusterer.py:76-111).  Every distinct label is checked, -1 included, as in the reference."""
    n_frames = frame.max() + 1
    lowest, highest, edges = _fa_limits(n_frames)
    values, ids = np.unique(labels, return_inverse=True)
    passed = backend.cluster_frame_analysis(ids.reshape(-1).astype(np.int32), frame, len(values), lowest, highest,
                                            edges)
    labels[np.isin(labels, values[passed == 0])] = -1
    return labels


def _finite_points(X) -> np.ndarray:
    X = np.asarray(X)
    if X.ndim != 2:
        raise ValueError(f"points must be an array of shape (n_points, n_dim), not {X.shape}")
    if not np.isfinite(X).all():
        raise ValueError("data must be finite, check for nan or inf values")
    return X


def _cluster(X, radius: float, min_locs: int, frame: pd.Series | None = None) -> np.ndarray:
    """int32 labels of the SMLM clusterer for the points X of shape (n, 2 | 3); -1 means no cluster
    (clusterer.py:114-201).  ``frame`` (a pandas Series) adds the frame analysis."""
    X = _finite_points(X)
    if not float(radius) > 0:
        raise ValueError(f"the clustering radius must be positive, not {radius}")
    if X.shape[0] == 0:
        labels = np.zeros(0, np.int32)
        return labels if frame is None else frame_analysis(labels, frame.to_numpy())
    points = backend.ClusterPoints(X)
    if frame is None:
        return points.smlm(radius, min_locs)
    frame = frame.to_numpy()
    return points.smlm(radius, min_locs, frame, *_fa_limits(frame.max() + 1))


def cluster_2D(locs: pd.DataFrame, radius: float, min_locs: int, fa: bool) -> np.ndarray:
    """Labels of a 2-D table (clusterer.py:204-238)."""
    X = locs[["x", "y"]].to_numpy()
    return _cluster(X, radius, min_locs, locs["frame"] if fa else None)


def cluster_3D(locs: pd.DataFrame, radius_xy: float, radius_z: float, min_locs: int, fa: bool) -> np.ndarray:
    """Labels of a 3-D table (clusterer.py:241-288): z is scaled by radius_xy / radius_z, in the columns' own
    dtype, so that the search is a sphere of radius_xy."""
    X = locs[["x", "y", "z"]].to_numpy()
    X[:, 2] *= radius_xy / radius_z
    return _cluster(X, radius_xy, min_locs, locs["frame"] if fa else None)


def cluster(locs: pd.DataFrame, radius_xy: float, min_locs: int, frame_analysis: bool, radius_z: float | None = None,
            pixelsize: float | None = None, return_info: bool = None):
    """SMLM clusterer (clusterer.py:291-407) -> the clustered rows with their ``group``, noise removed
    (and the ``info`` dictionary with ``return_info=True``).  z is in nm, the radii in camera pixels."""
    if return_info is None:
        return_info = False
        lib.deprecation_warning(
            "Deprecation warning: In v0.11.0, cluster will return both "
            "locs and cluster info by default. You can change the "
            "output already by setting return_info=True. In v0.12.0, "
            "this will not be optional anymore and cluster will always "
            "return both locs and cluster info."
        )
    locs = locs.copy()
    n_raw = len(locs)
    three_d = "z" in locs.columns
    if three_d:
        if pixelsize is None or radius_z is None:
            raise ValueError("Camera pixel size and clustering radius in z must be"
                             " specified for 3D clustering.")
        locs["z"] /= pixelsize
        labels = cluster_3D(locs, radius_xy, radius_z, min_locs, frame_analysis)
    else:
        labels = cluster_2D(locs, radius_xy, min_locs, frame_analysis)
    locs = extract_valid_labels(locs, labels)
    if three_d:
        locs["z"] *= pixelsize
    info = {
        "Generated by": f"Picasso v{__version__} SMLM clusterer",
        "Number of clusters": len(np.unique(locs["group"])),
        "Min. cluster size": min_locs,
        "Performed basic frame analysis": frame_analysis,
        "Fraction of rejected locs (%)": 100 * (n_raw - len(locs)) / n_raw,
    }
    unit = "nm" if pixelsize is not None else "px"
    scale = pixelsize if pixelsize is not None else 1
    if three_d:
        info[f"Clustering radius xy ({unit})"] = radius_xy * scale
        info[f"Clustering radius z ({unit})"] = radius_z * scale
    else:
        info[f"Clustering radius ({unit})"] = radius_xy * scale
    return (locs, info) if return_info else locs


def _dbscan(X, radius: float, min_density: int, min_locs: int = 0) -> np.ndarray:
    """int32 DBSCAN labels of the points X of shape (n, 2 | 3), clusters of fewer than ``min_locs`` rows set to
    -1 without renumbering (clusterer.py:410-445)."""
    X = _finite_points(X)
    if X.shape[0] == 0:
        raise ValueError(f"Found array with 0 sample(s) (shape={X.shape}) while a minimum of 1 is required by DBSCAN.")
    if not float(radius) > 0:
        raise ValueError(f"the DBSCAN radius must be positive, not {radius}")
    if int(min_density) < 1:
        raise ValueError(f"min_density must be at least 1, not {min_density}")
    return backend.ClusterPoints(X).dbscan(radius, min_density, min_locs)


def dbscan(locs: pd.DataFrame, radius: float, min_samples: int, min_locs: int = 10, pixelsize: float | None = None,
           radius_z: float | None = None, return_info: bool = None):
    """DBSCAN on a table (clusterer.py:448-544) -> the clustered rows with their ``group``, noise removed (and
    the ``info`` dictionary with ``return_info=True``).  With ``radius_z`` the search is an ellipsoid."""
    if return_info is None:
        return_info = False
        lib.deprecation_warning(
            "Deprecation warning: In v0.11.0, dbscan will return both "
            "locs and cluster info by default. You can change the "
            "output already by setting return_info=True. In v0.12.0, "
            "this will not be optional anymore and dbscan will always "
            "return both locs and cluster info."
        )
    locs = locs.copy()
    n_raw = len(locs)
    three_d = "z" in locs.columns
    if three_d:
        if pixelsize is None:
            raise ValueError("Camera pixel size must be specified as an integer for 3D"
                             " clustering.")
        X = locs[["x", "y", "z"]].to_numpy()
        X[:, 2] /= pixelsize
        if radius_z is not None:
            X[:, 2] *= radius / radius_z
    else:
        X = locs[["x", "y"]].to_numpy()
    labels = _dbscan(X, radius, min_samples, min_locs)
    locs = extract_valid_labels(locs, labels)
    unit = "nm" if pixelsize is not None else "px"
    scale = pixelsize if pixelsize is not None else 1
    info = {
        "Generated by": f"Picasso v{__version__} DBSCAN",
        "Number of clusters": len(np.unique(locs["group"])),
        f"Radius ({unit})": radius * scale,
        "Minimum local density": min_samples,
        "Min. localizations per cluster": min_locs,
        "Fraction of rejected locs (%)": 100 * (n_raw - len(locs)) / n_raw,
    }
    if three_d and radius_z is not None:
        info[f"Radius z ({unit})"] = radius_z * scale
    return (locs, info) if return_info else locs


def extract_valid_labels(locs: pd.DataFrame, labels: np.ndarray) -> pd.DataFrame:
    """``locs`` gets the column ``group`` (in place); the rows with a label other than -1 are returned
    (clusterer.py:665-691)."""
    locs["group"] = labels
    return locs[locs["group"] != -1]
