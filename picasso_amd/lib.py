"""The picasso.lib helpers the localization / undrift path depends on
(picasso/lib.py:878-920 get_from_metadata, :1786-1832 ensure_sanity, :2034-2078 minimize_shifts)."""
from __future__ import annotations

from typing import Any

import warnings

import numpy as np
import pandas as pd


def get_from_metadata(info, key: Any, default=None, *, raise_error: bool = False) -> Any:
    """Search the metadata (dict or list of dicts) from the last element to the first."""
    if isinstance(info, dict):
        info = [info]
    for d in reversed(info):
        if key in d:
            return d[key]
    if raise_error:
        raise KeyError(f"Key '{key}' not found in metadata.")
    return default


def ensure_sanity(locs: pd.DataFrame, info) -> pd.DataFrame:
    """Drop rows with inf/NaN, positions outside the image and negative
    x, y, lpx, lpy, lpz, photons, ellipticity, sx, sy (picasso/lib.py:1786-1832)."""
    locs = locs.copy()
    locs.replace([np.inf, -np.inf], np.nan, inplace=True)
    locs.dropna(axis=0, how="any", inplace=True)
    for key in ("Width", "Height", "Frames"):
        if get_from_metadata(info, key) is None:
            raise KeyError(f"Metadata is missing required key: '{key}'")
    locs = locs[locs["x"] < get_from_metadata(info, "Width")]
    locs = locs[locs["y"] < get_from_metadata(info, "Height")]
    for attr in ("x", "y", "lpx", "lpy", "lpz", "photons", "ellipticity", "sx", "sy"):
        if attr in locs.columns:
            locs = locs[locs[attr] >= 0]
    return locs


def deprecation_warning(message: str) -> None:
    warnings.warn(message, DeprecationWarning, stacklevel=3)


def minimize_shifts(shifts_x, shifts_y, shifts_z=None):
    """Least-squares consistent shifts from all pairwise shifts (picasso/lib.py:2034-2078).
    The shift between segments i < j is the sum of the step displacements D_i .. D_{j-1}, so with one
    row per pair (in the order i < j of the upper triangle) r = A D, A[row, i:j] = 1, and D = pinv(A) r.
    -> (shift_y, shift_x[, shift_z]), cumulative from segment 0."""
    n = shifts_x.shape[0]
    pairs = [(i, j) for i in range(n - 1) for j in range(i + 1, n)]
    stacked = [shifts_y, shifts_x] + ([] if shifts_z is None else [shifts_z])
    design = np.zeros((len(pairs), n - 1))
    observed = np.zeros((len(pairs), len(stacked)))
    for row, (i, j) in enumerate(pairs):
        design[row, i:j] = 1
        observed[row] = [m[i, j] for m in stacked]
    steps = np.dot(np.linalg.pinv(design), observed)
    return tuple(np.insert(np.cumsum(steps[:, d]), 0, 0) for d in range(len(stacked)))


# ---- point-in-shape helpers (picasso/lib.py:1835-2031, :2158-2225) on top of csrc/picks.hip -----------------------
PICK_NAMES = ("is_loc_at", "locs_at", "check_if_in_polygon", "check_if_in_rectangle", "locs_in_polygon",
              "locs_in_rectangle", "get_pick_polygon_corners", "get_pick_rectangle_corners")


def is_loc_at(x: float, y: float, locs: pd.DataFrame, r: float) -> BoolArray1D:
    """Boolean array: which localizations lie within ``r`` of (x, y) (picasso/lib.py:1835-1858), strict, one circular
    pick over the whole table on the device.  The reference computes this with pandas, whose arithmetic unwraps a NumPy
    scalar into a Python one: the differences, their squares and the sum of float32 columns stay float32 whatever ``x``
    and ``y`` are.  Its comparison does not unwrap: a Python ``r ** 2`` is compared as float32, a NumPy float64 one in
    float64.  All rows go through one workgroup (one pick): correct at any size, but no use of the whole chip."""
    from . import backend
    xc, yc = locs["x"].to_numpy(), locs["y"].to_numpy()
    r2 = r**2
    flags = 3 | (4 if np.result_type(np.float32, r2) == np.float32 else 0)
    zeros = np.zeros(len(locs), np.uint32)
    table = backend.BlockTable(zeros, zeros, 1, 1)           # one block: every row, in table order
    _, rows = backend.picks_circle(table, xc, yc, [float(x)], [float(y)], [0], [0], [flags], float(r2))
    is_picked = np.zeros(len(locs), bool)
    is_picked[rows] = True
    return is_picked


def locs_at(x: float, y: float, locs: pd.DataFrame, r: float) -> pd.DataFrame:
    """Localizations within ``r`` of (x, y) (picasso/lib.py:1861-1881)."""
    return locs[is_loc_at(x, y, locs, r)]


def _shape_mask(shape: int, x, y, X, Y) -> np.ndarray:
    """One shape over the points (x, y) without a bounding box.  The corners are taken as numba takes an array of
    Python numbers (float64 or int64).  Narrower than the reference in two ways: a point at -inf or beyond 8e307 is
    outside (the reference counts the sides such a ray hits), and all points go through one workgroup (one pick with an
    unbounded box): correct at any size, but no use of the whole chip, so a large table is better picked through
    ``postprocess.picked_locs``."""
    from . import backend
    x, y, X, Y = np.asarray(x), np.asarray(y), np.asarray(X), np.asarray(Y)
    for a in (X, Y):
        if a.dtype.kind not in "iu" and a.dtype != np.float64:
            raise TypeError(f"corners must be float64 or integers (np.array of Python numbers), not {a.dtype}")
    if x.dtype.kind != "f" or y.dtype.kind != "f":
        x, y = x.astype(np.float64), y.astype(np.float64)
    bounds = [[-np.inf, np.inf, -np.inf, np.inf]]
    if shape == backend.PICK_RECTANGLE:
        _, rows = backend.picks_rectangle(x, y, bounds, [0], [X[:4]], [Y[:4]])
    else:
        _, rows = backend.picks_polygon(x, y, bounds, [0], [0, len(X)], X, Y)
    mask = np.zeros(len(x), bool)
    mask[rows] = True
    return mask


def check_if_in_polygon(x: FloatArray1D, y: FloatArray1D, X: FloatArray1D, Y: FloatArray1D) -> BoolArray1D:
    """Which points (x, y) lie within the polygon with corners (X, Y): ray casting (picasso/lib.py:1884-1926), in
    float64 and the reference's order of operations."""
    return _shape_mask(2, x, y, X, Y)


def locs_in_polygon(locs: pd.DataFrame, X: FloatArray1D, Y: FloatArray1D) -> pd.DataFrame:
    """Localizations within the polygon (picasso/lib.py:1929-1952)."""
    return locs[check_if_in_polygon(locs["x"].to_numpy(), locs["y"].to_numpy(), np.array(X), np.array(Y))]


def check_if_in_rectangle(x: FloatArray1D, y: FloatArray1D, X: FloatArray1D, Y: FloatArray1D) -> BoolArray1D:
    """Which points (x, y) lie within the rectangle with corners (X, Y): the rays to the right that hit an odd number of
    the four sides (picasso/lib.py:1955-2004).  A point at exactly the height of a side whose two corners share that
    height makes the reference divide by zero, and numba raises: so does this, before any device work."""
    y_host, Y_host = np.asarray(y), np.asarray(Y)
    for i in range(4):
        if Y_host[i] == Y_host[(i + 1) % 4] and (y_host == Y_host[i]).any():
            raise ZeroDivisionError("division by zero")
    return _shape_mask(1, x, y, X, Y)


def locs_in_rectangle(locs: pd.DataFrame, X: FloatArray1D, Y: FloatArray1D) -> pd.DataFrame:
    """Localizations within the rectangle (picasso/lib.py:2007-2031)."""
    return locs[check_if_in_rectangle(locs["x"].to_numpy(), locs["y"].to_numpy(), np.array(X), np.array(Y))]


def get_pick_polygon_corners(pick: list[tuple[float, float]]) -> tuple[list[float], list[float]]:
    """The x and the y coordinates of a pick polygon's corners as two lists; (None, None) for a polygon that is not
    closed: fewer than three points, or a last point that is not the first (picasso/lib.py:2158-2181)."""
    closed = len(pick) >= 3 and pick[0] == pick[-1]
    if not closed:
        return None, None
    xs, ys = zip(*((corner[0], corner[1]) for corner in pick))
    return list(xs), list(ys)


def get_pick_rectangle_corners(start_x: float, start_y: float, end_x: float, end_y: float,
                               width: float) -> tuple[list[float], list[float]]:
    """The corners of the rectangular pick drawn from (start_x, start_y) to (end_x, end_y) with the given width
    (picasso/lib.py:2184-2225), as two lists of Python floats: left and right of the start, then right and left of the
    end.  The half width is laid across the axis by the axis angle's sine and cosine, computed with NumPy as the
    reference does; a vertical axis has the angle pi / 2 and no division."""
    angle = np.pi / 2 if end_x == start_x else np.arctan((end_y - start_y) / (end_x - start_x))
    across_x, across_y = width * np.sin(angle) / 2, width * np.cos(angle) / 2
    xs = [start_x - across_x, start_x + across_x, end_x + across_x, end_x - across_x]
    ys = [start_y + across_y, start_y - across_y, end_y - across_y, end_y + across_y]
    return [float(v) for v in xs], [float(v) for v in ys]


# ---- kinetic rates (picasso/lib.py:1263-1327) on top of csrc/cumexp.hip --------------------------------------------
KINETICS_NAMES = ("cumulative_exponential", "fit_cum_exp", "estimate_kinetic_rate")


def cumulative_exponential(x: FloatArray1D, a: float, t: float, c: float) -> FloatArray1D:
    """Used for binding kinetics estimation (picasso/lib.py:1263-1270)."""
    return a * (1 - np.exp(-(x / t))) + c


def _one_segment(data):
    """One segment through the kernel -> the backend's KineticRates with one entry each.  A fit that ends on the
    iteration cap raises RuntimeError, as scipy's does; an input scipy refuses raises ValueError."""
    from . import backend
    data = np.asarray(data)
    rates = backend.kinetic_rates(data, [0, len(data)])
    if rates.status[0] == backend.CUMEXP_REFUSED:
        raise ValueError("the samples of a fit must be finite and must not be negative")
    if rates.status[0] == backend.CUMEXP_ITER_CAP:
        raise RuntimeError("Optimal parameters not found: the fit reached its iteration cap")
    return rates


def fit_cum_exp(data: FloatArray1D) -> dict:
    """Fit a cumulative exponential function to data (picasso/lib.py:1273-1302): sorts ``data`` IN PLACE, as the
    reference does, and returns ``best_values`` (a, t, c), ``data`` and ``best_fit``.  The fit is the device's
    (csrc/cumexp.hip): a bounded descent from the reference's p0 to a cost that is not above scipy's; not scipy's bits."""
    rates = _one_segment(data)
    data.sort()
    if rates.a[0] != rates.a[0]:
        raise ValueError("fit_cum_exp needs more than two samples that are not all equal")
    popt = (float(rates.a[0]), float(rates.t[0]), float(rates.c[0]))
    return {"best_values": {"a": popt[0], "t": popt[1], "c": popt[2]}, "data": data,
            "best_fit": cumulative_exponential(data, *popt)}


def estimate_kinetic_rate(data: FloatArray1D) -> float:
    """Mean dark / bright time from the cumulative-exponential fit (picasso/lib.py:1305-1327): the mean of at most two or
    of equal samples, the fitted ``t`` otherwise; one segment through the kernel that ``postprocess.pick_kinetics`` runs
    over all picks.  A fitted ``data`` is sorted IN PLACE, as the reference's is."""
    rates = _one_segment(data)
    if rates.a[0] == rates.a[0]:
        data.sort()
    rate = rates.t[0]
    return np.float32(rate) if np.asarray(data).dtype == np.float32 and rates.a[0] != rates.a[0] else np.float64(rate)
