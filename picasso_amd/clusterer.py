"""DBSCAN, the SMLM clusterer, the cluster centers and the cluster areas of picasso.clusterer
(picasso/clusterer.py:34-544, :665-897, :1068-1237) on top of csrc/cluster.hip, csrc/centers.hip and csrc/areas.hip:
the same signatures, defaults, warnings, errors, dtypes, ``info`` entries and column handling, the same int32 label
for every row, the same table of centers and the same area or volume of every cluster.

The table handling stays the reference's own NumPy / pandas calls on the same dtypes (``z /= pixelsize`` on the
float32 column, the float32 ``X[:, 2] *= radius_xy / radius_z``, the widening to float64 that its KDTree and
sklearn do); the neighbour search, the local maxima, the union of core rows, the label sizes and the frame
analysis run on the device.  ``find_cluster_centers`` computes every per-cluster quantity on the device in pandas'
own arithmetic (the group order, the Kahan means and sums, the Welford standard deviations, the binding events,
``first()`` and the 2-D hull area); the derived columns are the reference's NumPy lines on those arrays, and the
volume of a 3-D hull stays its per-cluster scipy call on the host.  ``cluster_areas`` builds, blurs and thresholds
every cluster's image on the device, one workgroup per cluster, in NumPy's and SciPy's own arithmetic (the edges of
``np.arange``, the counts of ``np.histogramdd``, ``gaussian_filter(sigma=2)``, the Otsu threshold on
``np.histogram(image, 256)``): the result is a count over 4 or over 16 / 5 and equals the reference's.  Only the median
localization precision, one scalar, is the reference's pandas / NumPy call on the host.  ``test_subclustering`` is a
host composition over the device's nearest-neighbour table.  ``hdbscan`` is not here: it stays the reference's and works
on the tables these functions take and return.

Edges, as the reference has them: an empty table gives empty labels from ``_cluster`` (and a ``ValueError`` from
the frame analysis, which takes the maximum of no frames), a ``ValueError`` from ``_dbscan`` (sklearn wants one
sample) and a ``ZeroDivisionError`` from ``cluster`` / ``dbscan``; coordinates that are not finite raise
``ValueError`` (scipy's KDTree and sklearn both refuse them).  ``find_cluster_centers`` raises the reference's
``IndexError`` on an empty table and scipy's ``ValueError`` on a NaN coordinate.  ``cluster_areas`` returns an empty
table for an empty one, raises NumPy's ``ValueError`` where ``np.arange`` refuses a cluster's extent (a coordinate
that is not finite, a median precision of 0 or NaN) and ``MemoryError``, naming the group, where a cluster's image
would exceed ``backend.AREAS_MAX_BINS`` bins (the reference runs out of memory in NumPy there).
"""
from __future__ import annotations

from typing import Callable

import numpy as np
import pandas as pd

from . import __version__, backend, lib

# what localize.install() rebinds on picasso.clusterer
CLUSTERER_NAMES = ("_frame_analysis", "frame_analysis", "_cluster", "cluster_2D", "cluster_3D", "cluster", "_dbscan",
                   "dbscan", "extract_valid_labels", "_count_binding_events", "_cluster_convex_hulls",
                   "_weighted_z_means", "find_cluster_centers", "cluster_areas", "test_subclustering")
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


# ---- cluster centers (clusterer.py:694-897) ----
_MEAN_COLS = ("frame", "x", "y", "photons", "sx", "sy", "bg", "net_gradient")
_STD_COLS = ("frame", "x", "y")


def _groups(group_arr) -> "backend.CenterGroups":
    if len(group_arr) == 0:
        # new_event[0] = True of _count_binding_events (clusterer.py:750)
        raise IndexError("index 0 is out of bounds for axis 0 with size 0")
    return backend.CenterGroups(group_arr)


def _events_column(frame_arr) -> np.ndarray:
    frame_arr = np.asarray(frame_arr)
    if frame_arr.dtype.kind not in "iu" or frame_arr.dtype.itemsize < 4:
        raise TypeError(f"frame must be a 32- or 64-bit integer column, not {frame_arr.dtype}")
    return frame_arr


def _count_binding_events(group_arr, frame_arr, groups=None):
    """Binding events per cluster (clusterer.py:728-757): a new event starts where consecutive frames of a cluster,
    in table order, are more than 3 apart in the frame column's own type.
    -> (n_events per sorted unique group, the stable argsort by group, ``group_arr`` in that order)."""
    groups = groups or _groups(group_arr)
    n_events = groups.stats([(backend.CENTERS_EVENTS, _events_column(frame_arr), None, ())])[0]["sum"]
    order = groups.order()
    return n_events.astype(np.int64), order, np.asarray(group_arr)[order]


def _hull_volumes(locs, order, group_s, unique_groups, pixelsize) -> np.ndarray:
    """The volume of every cluster's 3-D hull: the reference's scipy call per cluster on slices of the device's group
    order (clusterer.py:773-788)."""
    from scipy.spatial import ConvexHull, QhullError
    coords_sorted = locs[["x", "y", "z"]].to_numpy()[order].astype(np.float64, copy=True)
    coords_sorted[:, 2] /= pixelsize
    group_offsets = np.searchsorted(group_s, unique_groups, side="left")
    group_offsets = np.append(group_offsets, len(group_s))
    convexhull = np.zeros(len(unique_groups), dtype=np.float64)
    for i in range(len(unique_groups)):
        X = coords_sorted[group_offsets[i]: group_offsets[i + 1]]
        try:
            convexhull[i] = ConvexHull(X).volume
        except QhullError:
            convexhull[i] = 0.0
    return convexhull


def _cluster_convex_hulls(locs: pd.DataFrame, order, group_s, unique_groups, has_z: bool, pixelsize, groups=None):
    """Convex-hull area (2-D, on the device) or volume (3-D, scipy per cluster) of every cluster
    (clusterer.py:760-788).  0.0 where the rows span no area: one or two rows, duplicates, collinear rows."""
    if has_z:
        return _hull_volumes(locs, order, group_s, unique_groups, pixelsize)
    x, y = locs["x"].to_numpy(), locs["y"].to_numpy()
    if np.isnan(x).any() or np.isnan(y).any():
        raise ValueError("Points cannot contain NaN")           # scipy's, from the first cluster that holds one
    groups = groups or _groups(locs["group"].to_numpy())
    return groups.hull_areas(x, y)


def _weighted_z_means(locs: pd.DataFrame, group_arr, groups=None) -> np.ndarray:
    """Per-cluster z mean weighted by 1 / (lpx + lpy)^2 (clusterer.py:791-800)."""
    groups = groups or _groups(group_arr)
    w = groups.weights(locs["lpx"].to_numpy(), locs["lpy"].to_numpy())
    ws, wz = groups.stats([(backend.CENTERS_MEAN, w, None, ("sum",)),
                           (backend.CENTERS_XSUM, locs["z"].to_numpy(), w, ())])
    return (pd.Series(wz["sum"]) / pd.Series(ws["sum"])).to_numpy()


def find_cluster_centers(locs: pd.DataFrame, pixelsize: float | None = None) -> pd.DataFrame:
    """Cluster centers of a table with a ``group`` column (clusterer.py:803-897): one row per cluster in the format
    of localizations, the same columns, dtypes and values as the reference's.  ``pixelsize`` is needed for 3-D."""
    has_z = "z" in locs.columns
    if has_z and pixelsize is None:
        raise ValueError(
            "Camera pixel size must be specified as an integer for 3D"
            " cluster centers calculation."
        )
    group_arr = locs["group"].to_numpy()
    frame_arr = locs["frame"].to_numpy()
    mean_cols = list(_MEAN_COLS) + (["z"] if has_z else [])
    std_cols = list(_STD_COLS) + (["z"] if has_z else [])
    columns = {c: locs[c].to_numpy() for c in mean_cols}
    groups = _groups(group_arr)

    requests = [(backend.CENTERS_MEAN, columns[c], None, ("mean", "std") if c in std_cols else ("mean",))
                for c in mean_cols]
    requests.append((backend.CENTERS_EVENTS, _events_column(frame_arr), None, ()))
    if "group_input" in locs.columns:
        requests.append((backend.CENTERS_FIRST, locs["group_input"].to_numpy(), None, ()))
    res = groups.stats(requests)
    s = {f"{c}_mean": r["mean"] for c, r in zip(mean_cols, res)}
    # pandas returns the standard deviation of a float32 column as float32
    s.update({f"{c}_std": r["std"].astype(np.float32) if columns[c].dtype == np.float32 else r["std"]
              for c, r in zip(mean_cols, res) if c in std_cols})
    s["n_locs"] = groups.n_locs
    s["unique_groups"] = groups.unique
    n_events = res[len(mean_cols)]["sum"]

    lpx = s["x_std"] / np.sqrt(s["n_locs"])
    lpy = s["y_std"] / np.sqrt(s["n_locs"])
    ellipticity = s["sx_mean"] / s["sy_mean"]
    if has_z:
        order = groups.order()
        convexhull = _cluster_convex_hulls(locs, order, group_arr[order], s["unique_groups"], has_z, pixelsize)
    else:
        convexhull = _cluster_convex_hulls(locs, None, None, s["unique_groups"], has_z, pixelsize, groups)

    columns = {
        "frame": s["frame_mean"].astype(np.float32),
        "std_frame": s["frame_std"].astype(np.float32),
        "x": s["x_mean"].astype(np.float32),
        "y": s["y_mean"].astype(np.float32),
        "std_x": s["x_std"].astype(np.float32),
        "std_y": s["y_std"].astype(np.float32),
    }
    if has_z:
        columns["z"] = _weighted_z_means(locs, group_arr, groups).astype(np.float32)
    columns.update(
        {
            "photons": s["photons_mean"].astype(np.float32),
            "sx": s["sx_mean"].astype(np.float32),
            "sy": s["sy_mean"].astype(np.float32),
            "bg": s["bg_mean"].astype(np.float32),
            "lpx": lpx.astype(np.float32),
            "lpy": lpy.astype(np.float32),
        }
    )
    if has_z:
        columns["lpz"] = (s["z_std"] / np.sqrt(s["n_locs"])).astype(np.float32)
        columns["std_z"] = s["z_std"].astype(np.float32)
    columns.update(
        {
            "ellipticity": ellipticity.astype(np.float32),
            "net_gradient": s["net_gradient_mean"].astype(np.float32),
            "n_locs": s["n_locs"].astype(np.uint32),
            "n_events": n_events.astype(np.int32),
        }
    )
    if has_z:
        volume = (
            np.power((s["x_std"] + s["y_std"] + s["z_std"] / pixelsize) / 3 * 2, 3)
            * 4.18879
        )  # assume radius = 2 * std_xyz
        columns["volume"] = volume.astype(np.float32)
    else:
        # assume radius = 2 * std_xy
        area = np.power(s["x_std"] + s["y_std"], 2) * np.pi
        columns["area"] = area.astype(np.float32)
    columns["convexhull"] = convexhull.astype(np.float32)
    columns["group"] = s["unique_groups"].astype(np.int32)
    if "group_input" in locs.columns:
        columns["group_input"] = res[len(mean_cols) + 1]["sum"].astype(np.int32)
    return pd.DataFrame(columns)


# ---- cluster areas (clusterer.py:1068-1237) ----
def cluster_areas(
    locs: pd.DataFrame,
    info: list[dict],
    progress: Callable[[int], None] | None = None,
) -> pd.DataFrame:
    """Area (2-D, ``"Area (LP^2)"``) or volume (3-D, ``"Volume (LP^3)"``) of every cluster of a table with a
    ``group`` column, in units of the median localization precision (clusterer.py:1112-1169): the number of bins of
    the cluster's blurred image (bins of LP / 2, 1.25 LP in z) at or above its Otsu threshold.  One row per distinct
    label, -1 included, int32 ``group`` and float32 values equal to the reference's.  All clusters are computed on the
    device; a callable ``progress`` then sees 1 .. the number of clusters, ``None`` shows a tqdm bar."""
    assert (
        "group" in locs.columns
    ), "Localizations must contain 'group' column."
    pixelsize = lib.get_from_metadata(info, "Pixelsize", raise_error=True)
    has_z = "z" in locs.columns
    area_key = "Area (LP^2)" if not has_z else "Volume (LP^3)"
    lp = np.median(locs[["lpx", "lpy"]].mean(axis=1))
    group_arr = locs["group"].to_numpy()
    if len(group_arr) == 0:
        return pd.DataFrame({"group": np.unique(group_arr).astype(np.int32), area_key: np.zeros(0, dtype=np.float32)})
    columns = [locs[c].to_numpy() for c in (("x", "y", "z") if has_z else ("x", "y"))]
    bin_size = lp / 2  # pixel size for rendering
    bin_size_z = bin_size * 2.5
    groups = backend.CenterGroups(group_arr)
    images = backend.AreaImages(groups, columns, pixelsize, bin_size, bin_size_z)
    areas = {"group": groups.unique.astype(np.int32), area_key: images.areas()}
    n = groups.n_groups
    if progress is None:
        from tqdm import tqdm
        for _ in tqdm(range(n), desc="Calculating cluster areas"):
            pass
    else:
        for idx in range(n):
            progress(idx + 1)
    return pd.DataFrame(areas)


def test_subclustering(
    mols: pd.DataFrame,
    info: list[dict],
    clustering_dist: float = 25,
    sparse_dist: float = 80,
) -> tuple[lib.IntArray1D, lib.IntArray1D]:
    """``n_events`` of the molecules whose nearest neighbour is closer than ``clustering_dist`` (nm) and of those whose
    nearest neighbour is at least ``sparse_dist`` (nm) away (clusterer.py:1172-1237).  The distances are the device's
    nearest-neighbour table of the molecules to themselves (two neighbours: the first is the molecule itself)."""
    from . import postprocess
    assert (
        "n_events" in mols.columns
    ), "The input molecules must have n_events attribute."
    assert sparse_dist > clustering_dist, (
        "The sparse distance must be larger than the clustering " "distance."
    )
    pixelsize = lib.get_from_metadata(info, "Pixelsize", raise_error=True)
    if "z" in mols.columns:
        coords = mols[["x", "y", "z"]].to_numpy()
        coords[:, 2] /= pixelsize
    else:
        coords = mols[["x", "y"]].to_numpy()
    distances = postprocess._knn_table(postprocess._kdtree_points(coords), coords, 2)
    nnd1 = distances[:, 1]
    close_nnd_idx = np.where(nnd1 < clustering_dist / pixelsize)[0]
    far_nnd_idx = np.where(nnd1 >= sparse_dist / pixelsize)[0]
    clustered_nevents = mols.iloc[close_nnd_idx]["n_events"].to_numpy()
    sparse_nevents = mols.iloc[far_nnd_idx]["n_events"].to_numpy()
    return clustered_nevents, sparse_nevents


test_subclustering.__test__ = False      # a function of the package, not a test of it
