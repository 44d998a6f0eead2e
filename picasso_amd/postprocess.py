"""The RCC drift-correction entry points of picasso.postprocess (picasso/postprocess.py:2824-2961
``n_segments``, ``segment``, ``undrift``; :3157-3218 ``_apply_drift`` / ``apply_drift``) on top of
the GPU render (csrc/render.hip) and cross-correlation (csrc/xcorr.hip), and linking and NeNA
(:2007-2071 ``link``, :2422-2821 the link groups and their combination, :1058-1119 ``nena``, :1165-1239 the
next-frame neighbour distance histogram) on top of csrc/link.hip, and the local density, the distance histogram and the
pair correlation (:37-204 the index blocks, :1582-1631 ``compute_local_density``, :1002-1055 ``distance_histogram``,
:1505-1540 ``pair_correlation``) on top of csrc/pairs.hip, and the dark times and group properties of qPAINT
(:1920-2004 ``compute_dark_times`` / ``dark_times`` / ``_dark_times``, :3580-3649 ``groupprops``) on top of
csrc/kinetics.hip, and the nearest-neighbour distances (:3704-3739 ``nn_analysis``) on top of csrc/knn.hip, and the
cluster combine and its nearest-cluster distances (:2174-2288 ``cluster_combine``, :2291-2419 ``cluster_combine_dist``)
on top of csrc/combine.hip, and the picked localizations (:207-473) on top of csrc/picks.hip and the fiducial undrift
from them (:2964-3156 ``undrift_from_fiducials``, ``undrift_from_picked``) on top of csrc/fiducials.hip, and
``pick_similar`` (:476-736) on top of csrc/similar.hip.
"""
from __future__ import annotations

import math
from copy import deepcopy
import warnings
from collections import OrderedDict
from typing import Callable, Literal

import numpy as np
import pandas as pd
from scipy.interpolate import InterpolatedUnivariateSpline
from scipy.optimize import curve_fit

from . import backend, imageprocess, lib, render

# what localize.install() rebinds on picasso.postprocess besides segment / undrift
LINK_NENA_NAMES = ("link", "_get_link_groups", "get_link_groups", "_link_loc_groups", "link_loc_groups", "nena",
                   "_next_frame_neighbor_distance_histogram", "next_frame_neighbor_distance_histogram")
# ... and for the analyses over the index blocks
PAIR_NAMES = ("_index_blocks_shape", "compute_local_density", "distance_histogram", "pair_correlation")
# ... and for the dark times and the group properties
KINETICS_NAMES = ("_dark_times", "dark_times", "compute_dark_times", "groupprops")
# ... and for the nearest-neighbour distances
NN_NAMES = ("nn_analysis",)
# ... and for the cluster combine
COMBINE_NAMES = ("cluster_combine", "cluster_combine_dist")
_SEGMENT_RENDER = {"blur_method": "gaussian", "min_blur_width": 1}      # what undrift renders its segments with


def n_segments(info, segmentation: int) -> int:
    """Number of temporal segments: round(Frames / segmentation)."""
    return int(np.round(lib.get_from_metadata(info, "Frames") / segmentation))


def _segment_bounds(info, segmentation: int) -> np.ndarray:
    count = n_segments(info, segmentation)
    return np.linspace(0, info[0]["Frames"] - 1, count + 1, dtype=np.uint32)


def segment(locs: pd.DataFrame, info, segmentation: int, kwargs: dict = {}, callback=None):
    """Render the localizations of every temporal segment (postprocess.py:2846-2897).
    -> (uint32 frame bounds, float64 stack of shape (n_segments, Height, Width)); segment i holds the
    frames bounds[i] <= frame < bounds[i + 1]; the callback sees 0, 1, ..., n_segments."""
    bounds = _segment_bounds(info, segmentation)
    stack = np.zeros((len(bounds) - 1, info[0]["Height"], info[0]["Width"]))
    frame = locs["frame"]
    if callback is not None:
        callback(0)
    # A localization table is ordered by frame (picasso/gaussmle.py:1036): a segment is then a row range, found by
    # bisection, and only the columns a render reads are taken — instead of a boolean mask over every row and a copy
    # of all 17 columns per segment (4e7 rows x 25 segments on one rank of config 4: seconds).
    cols = [c for c in ("x", "y", "lpx", "lpy") if c in locs.columns]
    fr = frame.to_numpy()
    ordered = len(fr) == 0 or bool(np.all(fr[1:] >= fr[:-1]))
    views = {c: locs[c].to_numpy() for c in cols} if ordered else None
    for i, (lo, hi) in enumerate(zip(bounds[:-1], bounds[1:])):
        if ordered:
            a, b = np.searchsorted(fr, lo, side="left"), np.searchsorted(fr, hi, side="left")
            part = pd.DataFrame({c: views[c][a:b] for c in cols}, copy=False)
        else:
            part = locs[(frame >= lo) & (frame < hi)]
        stack[i] = render.render(part, info, **kwargs)[1]
        if callback is not None:
            callback(i + 1)
    return bounds, stack


def _apply_drift(locs: pd.DataFrame, drift: pd.DataFrame) -> pd.DataFrame:
    """coordinate -= drift[frame]; the float64 drift turns the float32 columns into float64, as in
    the reference (postprocess.py:3157-3168)."""
    row = locs["frame"].to_numpy()
    for axis in ("x", "y", "z"):
        if axis in drift.columns and axis in locs.columns:
            locs[axis] = locs[axis] - drift[axis].to_numpy()[row]
    return locs


def apply_drift(locs: pd.DataFrame, info, *, drift):
    """Checked form (postprocess.py:3171-3218): drift is a DataFrame with x, y (, z) per frame or an
    array of shape (Frames, 2 | 3)."""
    assert isinstance(drift, (pd.DataFrame, np.ndarray)), "Drift must be a DataFrame or numpy array"
    n_frames = lib.get_from_metadata(info, "Frames", raise_error=True)
    if isinstance(drift, np.ndarray):
        if drift.shape[0] != n_frames or drift.shape[1] not in (2, 3):
            raise ValueError("Drift array must have shape (n_frames, 2) for x and y drift, "
                             "or (n_frames, 3) for x, y, and z drift.")
        drift = pd.DataFrame(drift, columns=["x", "y", "z"][:drift.shape[1]])
    elif not {"x", "y"} <= set(drift.columns):
        raise ValueError(f"Drift DataFrame must contain columns {{'x', 'y'}}")
    return _apply_drift(locs, drift)


def _spline_over_frames(bounds, shift, n_frames):
    centres = (bounds[1:] + bounds[:-1]) / 2
    return InterpolatedUnivariateSpline(centres, shift, k=3)(np.arange(n_frames))


def undrift(locs: pd.DataFrame, info, segmentation: int, display: bool = True, segmentation_callback=None,
            rcc_callback=None):
    """RCC drift correction (postprocess.py:2900-2961) -> (drift DataFrame, undrifted copy of locs).
    ``display`` (a matplotlib plot in the reference) is ignored."""
    locs = locs.copy(deep=False)          # the drift replaces the x / y columns of the copy; the others are shared
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", DeprecationWarning)       # render()'s oversampling notice, as in the reference call
        bounds, stack = segment(locs, info, segmentation, dict(_SEGMENT_RENDER), segmentation_callback)
    backend.join_fft_prewarm()            # plans started by localize_file on a side thread: ready (or made) before they are used
    shift_y, shift_x = imageprocess.rcc(stack, 32, rcc_callback)
    n_frames = info[0]["Frames"]
    drift = pd.DataFrame({"x": _spline_over_frames(bounds, shift_x, n_frames),
                          "y": _spline_over_frames(bounds, shift_y, n_frames)})
    return drift, apply_drift(locs, info, drift=drift)


# ---- link (postprocess.py:2007-2071, 2422-2821) -----------------------------------------------------------
def _squared_like_numba(d_max) -> float:
    """d_max ** 2 in the type numba gives d_max (a float32 stays float32, an integer stays an integer), as float64:
    the jitted loops compare with it in float64."""
    if isinstance(d_max, np.floating):
        return float(d_max * d_max)
    if isinstance(d_max, (int, np.integer)) and not isinstance(d_max, bool):
        return float(int(d_max) * int(d_max))
    return float(d_max) * float(d_max)


def _device_link_groups(frame, x, y, d_max, max_dark_time, group):
    table = backend.LinkTable(frame, x, y, group)
    # frame > current + max_dark_time + 1 for integer frames: a fractional dark time counts as its floor
    return table.link_groups(_squared_like_numba(d_max), math.floor(max_dark_time + 1))


def _get_link_groups(frame, x, y, d_max: float, max_dark_time: int, group) -> np.ndarray:
    """The int32 link group of every row of a table sorted by frame (postprocess.py:2441-2552): the reference's
    greedy chains, group numbers in the order of their first row.  The last row of the table has no next row
    (the reference is undefined there): its chain ends."""
    if len(x) == 0:
        return np.zeros(0, np.int32)
    d_link_group, _ = _device_link_groups(frame, x, y, d_max, max_dark_time, group)
    return d_link_group.cpu().numpy()


def get_link_groups(frame, x, y, d_max: float, max_dark_time: int, group) -> np.ndarray:
    """Alias to _get_link_groups, deprecated."""
    lib.deprecation_warning("Deprecation warning: This function will become private in "
                            "v0.11.0. Use _get_link_groups instead.")
    return _get_link_groups(frame, x, y, d_max, max_dark_time, group)


def _numba_mean(group_sum: np.ndarray, divisor: np.ndarray) -> np.ndarray:
    """float32(group_sum / divisor) as the jitted _link_group_mean types it: integers join a float operand's
    type (float32 / uint32 is a float32 division), two integer arrays divide in float64."""
    a, b = group_sum.dtype, divisor.dtype
    if a.kind in "iub" and b.kind in "iub":
        dt = np.dtype(np.float64)
    elif a.kind in "iub":
        dt = b
    elif b.kind in "iub":
        dt = a
    else:
        dt = np.promote_types(a, b)
    with np.errstate(all="ignore"):
        return (group_sum.astype(dt) / divisor.astype(dt)).astype(np.float32)


_LINK_MEANS = ("sx", "sy", "ellipticity", "net_gradient", "likelihood", "iterations", "d_zcalib")


def _combine(locs: pd.DataFrame, info, link_group, n_groups: int, remove_ambiguous_lengths: bool) -> pd.DataFrame:
    """_link_loc_groups with the group sums of every column in one pass on the device; `link_group` is a host array
    or the device tensor the link groups were made in."""
    has = locs.columns.__contains__
    col = {c: locs[c].to_numpy() for c in locs.columns}
    jobs, where = [], {}

    def job(key, op, data, weight):
        where[key] = len(jobs)
        jobs.append((op, data, weight))

    for axis, lp in (("x", "lpx"), ("y", "lpy")):
        if has(axis):
            job("w" + axis, backend.LINK_WSUM, None, col[lp])
            job(axis, backend.LINK_XWSUM, col[axis], col[lp])
    if has("z") and has("lpz"):
        job("wz", backend.LINK_WSUM, None, col["lpz"])
        job("z", backend.LINK_XWSUM, col["z"], col["lpz"])
    elif has("z"):
        job("z", backend.LINK_SUM, col["z"], None)
    for c in ("photons", "bg") + _LINK_MEANS:
        if has(c):
            job(c, backend.LINK_SUM, col[c], None)
    frame = col["frame"] if has("frame") else None
    n_, first, last, last_row, sums = backend.link_combine(link_group, n_groups, frame, jobs)
    empty = n_ == 0

    def total(key):
        return sums[where[key]]

    columns = OrderedDict()
    if has("frame"):
        if empty.any():                      # the reference's start values of an empty group
            first[empty], last[empty] = frame.max(), frame.min()
        first_frame_, last_frame_ = first.astype(frame.dtype), last.astype(frame.dtype)
        columns["frame"] = first_frame_
    for axis in ("x", "y"):
        if has(axis):
            columns[axis] = _numba_mean(total(axis), total("w" + axis))
    if has("photons"):
        columns["photons"] = total("photons")
    for c in ("sx", "sy"):
        if has(c):
            columns[c] = _numba_mean(total(c), n_)
    if has("bg"):
        columns["bg"] = total("bg")
    with np.errstate(all="ignore"):
        for axis in ("x", "y"):
            if has(axis):
                columns["lp" + axis] = np.sqrt(1 / total("w" + axis))
        for c in ("ellipticity", "net_gradient", "likelihood", "iterations"):
            if has(c):
                columns[c] = _numba_mean(total(c), n_)
        if has("z"):
            if has("lpz"):
                columns["z"] = _numba_mean(total("z"), total("wz"))
                columns["lpz"] = np.sqrt(1 / total("wz"))
            else:
                columns["z"] = _numba_mean(total("z"), n_)
        if has("d_zcalib"):
            columns["d_zcalib"] = _numba_mean(total("d_zcalib"), n_)
        if has("group"):
            last_group = col["group"][np.where(empty, 0, last_row)]
            if empty.any():
                last_group[empty] = 0
            columns["group"] = last_group
        if has("frame"):
            columns["len"] = last_frame_ - first_frame_ + 1
        columns["n"] = n_
        if has("photons"):
            columns["photon_rate"] = np.float32(columns["photons"] / n_)
    linked_locs = pd.DataFrame(columns)
    if remove_ambiguous_lengths:
        valid = np.logical_and(first_frame_ > 0, last_frame_ < info[0]["Frames"])
        linked_locs = linked_locs[valid]
    return linked_locs


def _link_loc_groups(locs: pd.DataFrame, info, link_group, remove_ambiguous_lengths: bool = True) -> pd.DataFrame:
    """Combine localizations into binding events (postprocess.py:2680-2821): per link group the first frame,
    precision-weighted position, summed photons / background, mean shape columns, length and count."""
    link_group = np.asarray(link_group)
    if len(link_group) != len(locs):
        raise ValueError("link_group must have one entry per localization")
    if link_group.min() < 0:
        raise ValueError("link_group must not be negative")
    return _combine(locs, info, link_group.astype(np.int32, copy=False), int(link_group.max()) + 1,
                    remove_ambiguous_lengths)


def link_loc_groups(locs: pd.DataFrame, info, link_group, remove_ambiguous_lengths: bool = True) -> pd.DataFrame:
    """Alias to _link_loc_groups, deprecated."""
    lib.deprecation_warning("Deprecation warning: This function will become private in "
                            "v0.11.0. Use _link_loc_groups instead.")
    return _link_loc_groups(locs, info, link_group, remove_ambiguous_lengths)


def link(locs: pd.DataFrame, info, r_max: float = 0.05, max_dark_time: int = 3,
         combine_mode: Literal["average", "refit"] = "average", remove_ambiguous_lengths: bool = True) -> pd.DataFrame:
    """Link localizations into binding events by their spatiotemporal proximity (postprocess.py:2007-2071).
    The sort by frame is the reference's own pandas call on the host; everything behind it runs on the device."""
    if len(locs) == 0:
        linked_locs = locs.copy()
        if "frame" in locs.columns:
            linked_locs["len"] = np.array([], dtype=np.int32)
            linked_locs["n"] = np.array([], dtype=np.int32)
        if "photons" in locs.columns:
            linked_locs["photon_rate"] = np.array([], dtype=np.float32)
    else:
        locs = locs.sort_values(kind="quicksort", by="frame")
        if "group" in locs.columns:
            group = locs["group"].to_numpy()
        else:
            group = np.zeros(len(locs), dtype=np.int32)
        d_link_group, n_groups = _device_link_groups(locs["frame"].to_numpy(), locs["x"].to_numpy(),
                                                     locs["y"].to_numpy(), r_max, max_dark_time, group)
        if combine_mode == "average":
            linked_locs = _combine(locs, info, d_link_group, n_groups, remove_ambiguous_lengths)
        elif combine_mode == "refit":
            raise NotImplementedError("Refit mode is not implemented yet. Please use 'average' mode.")
    return linked_locs


# ---- NeNA (postprocess.py:1058-1272) ------------------------------------------------------------------------
def _nfndh(frame, x, y, group, d_max: float, bin_size: float, callback: Callable[[int], None] | None = None):
    """Next-frame neighbour distance histogram of a table sorted by frame (postprocess.py:1212-1272), with the
    reference's three quirks: the last len % 100 rows never look forward, the last row of the table is never a
    neighbour, and a pair at exactly d_max (one past the last bin) is dropped.  The histogram is one kernel; the
    callback then sees 1 .. 100."""
    bins = np.arange(0, d_max, bin_size)
    counts = backend.LinkTable(frame, x, y, group).nena_hist(d_max, bin_size, len(bins))
    dnfl = counts.astype(np.float64)
    if callback is not None:
        for k in range(100):
            callback(k + 1)
    return bins + bin_size / 2, dnfl


def _next_frame_neighbor_distance_histogram(locs: pd.DataFrame, callback: Callable[[int], None] | None = None):
    """-> (bin_centers, dnfl).  Sorts ``locs`` by frame IN PLACE, as the reference does."""
    locs.sort_values(kind="quicksort", by="frame", inplace=True)
    frame = locs["frame"].to_numpy()
    x = locs["x"].to_numpy()
    y = locs["y"].to_numpy()
    if "group" in locs.columns:
        group = locs["group"].to_numpy()
    else:
        group = np.zeros(len(locs), dtype=np.int32)
    return _nfndh(frame, x, y, group, 1.0, 0.001, callback)


def next_frame_neighbor_distance_histogram(locs: pd.DataFrame, callback: Callable[[int], None] | None = None):
    """Alias to _next_frame_neighbor_distance_histogram, deprecated."""
    lib.deprecation_warning("Deprecation warning: This function will become private in "
                            "v0.11.0. Use _next_frame_neighbor_distance_histogram instead.")
    return _next_frame_neighbor_distance_histogram(locs, callback)


def _nena_model(d, delta_a, s, ac, dc, sc):
    a = ac + delta_a  # make sure a >= ac
    p_single = a * (d / (2 * s**2)) * np.exp(-(d**2) / (4 * s**2))
    p_short = ac / (sc * np.sqrt(2 * np.pi)) * np.exp(-0.5 * ((d - dc) / sc) ** 2)
    return p_single + p_short


def _nena_fit(bin_centers, dnfl, median_lp):
    """The reference's curve_fit call on the histogram (postprocess.py:1097-1101), on the host."""
    area = np.trapezoid(dnfl, bin_centers)
    p0 = [0.8 * area, median_lp, 0.1 * area, 2 * median_lp, median_lp]
    bounds = ([0, 0, 0, 0, 0], [np.inf, np.inf, np.inf, np.inf, np.inf])
    popt, _ = curve_fit(_nena_model, bin_centers, dnfl, p0=p0, bounds=bounds)
    return popt


def nena(locs: pd.DataFrame, info=None, callback: Callable[[int], None] | None = None):
    """NeNA, the experimental localization precision (postprocess.py:1058-1119) -> (result dict, s in pixels)."""
    bin_centers, dnfl = _next_frame_neighbor_distance_histogram(locs, callback)
    median_lp = np.mean([np.median(locs["lpx"]), np.median(locs["lpy"])])
    popt = _nena_fit(bin_centers, dnfl, median_lp)
    s = popt[1]
    result = {
        "d": bin_centers,
        "data": dnfl,
        "best_fit": _nena_model(bin_centers, *popt),
        "best_values": {"delta_a": popt[0], "s": popt[1], "ac": popt[2], "dc": popt[3], "sc": popt[4]},
        "pixelsize": lib.get_from_metadata(info, "Pixelsize", default="N/A"),
    }
    return result, s


# ---- local density, distance histogram, pair correlation (postprocess.py:37-204, :960-1055, :1505-1631) ----------
def _index_blocks_shape(info, size: float) -> tuple[int, int]:
    """(blocks in y, blocks in x) of the index grid (postprocess.py:108-129)."""
    width = lib.get_from_metadata(info, "Width", raise_error=True)
    height = lib.get_from_metadata(info, "Height", raise_error=True)
    return int(np.ceil(height / size)), int(np.ceil(width / size))


def _block_table(locs: pd.DataFrame, info, size: float, refuse_empty: bool = False):
    """The host part of get_index_blocks (postprocess.py:74-83), as the reference's own NumPy calls, and the sort on
    the device instead of the K x L block table -> (sanity-filtered locs, backend.BlockTable)."""
    locs = lib.ensure_sanity(locs, info)
    x_index = np.uint32(locs["x"].to_numpy() / size)
    y_index = np.uint32(locs["y"].to_numpy() / size)
    n_blocks_y, n_blocks_x = _index_blocks_shape(info, size)
    if refuse_empty and len(locs) == 0:
        raise ValueError("range() arg 3 must not be zero")
    return locs, backend.BlockTable(x_index, y_index, n_blocks_y, n_blocks_x)


def _index_blocks(locs: pd.DataFrame, info, size: float):
    """_block_table as get_index_blocks itself answers: the reference splits the rows into int(N / n_threads)-row
    chunks and so raises on an empty table (range() with step 0) on every machine; here that is the only table not
    computed."""
    return _block_table(locs, info, size, refuse_empty=True)


def compute_local_density(locs: pd.DataFrame, info, radius: float) -> pd.DataFrame:
    """The localizations in block order with the column ``density``: the number of localizations within ``radius``,
    the row itself included (postprocess.py:1582-1631).  Counted as the reference counts: a row whose block index
    falls outside the grid (x / radius rounds up to Width / radius) and every row sorted behind it is never a
    neighbour, and a block index of -1 is the last block row / column."""
    locs, table = _index_blocks(locs, info, radius)
    density = table.density(locs["x"].to_numpy(), locs["y"].to_numpy(), _squared_like_numba(radius))
    locs = locs.iloc[table.order()]
    locs["density"] = density.astype(np.uint64)        # np.sum over the reference's per-thread uint32 arrays
    return locs


def distance_histogram(locs: pd.DataFrame, info, bin_size: float, r_max: float) -> np.ndarray:
    """uint64 histogram of the pairwise distances below ``r_max`` (postprocess.py:1002-1055), uint32(r_max / bin_size)
    bins.  As in the reference, a pair is counted when the later row (in block order) lies in the same block or in
    the block to the right, below or below right of the earlier one: pairs across the lower-left diagonal are not."""
    locs, table = _index_blocks(locs, info, r_max)
    n_bins = int(np.uint32(r_max / bin_size))
    return table.distance_hist(locs["x"].to_numpy(), locs["y"].to_numpy(), r_max, _squared_like_numba(r_max), bin_size,
                               n_bins)


def pair_correlation(locs: pd.DataFrame, info, bin_size: float, r_max: float):
    """-> (bins_lower, pc): the distance histogram divided by the area of each ring (postprocess.py:1505-1540)."""
    dh = distance_histogram(locs, info, bin_size, r_max)
    bins_lower = np.arange(bin_size, r_max + bin_size, bin_size)
    if bins_lower.shape[0] > dh.shape[0]:
        bins_lower = bins_lower[:-1]
    area = np.pi * bin_size * (2 * bins_lower + bin_size)
    return bins_lower, dh / area


# ---- dark times (postprocess.py:1920-2004) --------------------------------------------------------------------
def _group_labels(group) -> np.ndarray:
    """The ``group`` argument as int64 labels.  Narrower than the reference: a floating array is taken when every value
    is finite and integral (the reference's own ``np.zeros(len(locs))`` is), anything else is refused."""
    group = np.asarray(group)
    if group.ndim != 1:
        raise ValueError(f"group must be a 1-D array, not an array of shape {group.shape}")
    if group.dtype.kind in "iub":
        if group.dtype == np.uint64 and len(group) and int(group.max()) >= 2 ** 63:
            raise ValueError("group labels must fit a signed 64-bit integer")
        return group.astype(np.int64, copy=False)
    if group.dtype.kind != "f":
        raise TypeError(f"group must be an array of integer labels (or of integral floating values), not {group.dtype}")
    if not (np.isfinite(group).all() and (group == np.trunc(group)).all() and (np.abs(group) <= 2.0 ** 53).all()):
        raise ValueError("a floating group array must hold finite, integral labels of at most 2**53")
    return group.astype(np.int64)


def _frame_numbers(a, what: str) -> np.ndarray:
    """An integer column whose values the device may subtract as signed 64-bit integers, as numba subtracts them: two
    unsigned 32-bit columns meet in uint64 and wrap there, and a wrapped difference is never below max_frame, as a
    negative one is never above 0; every other pair of integer columns meets in int64.  uint64 (which numba subtracts
    from a signed column in float64) and magnitudes from 2**62 on are outside that domain."""
    a = np.asarray(a)
    if a.dtype.kind not in "iu":
        raise TypeError(f"{what} must be an integer column, not {a.dtype}")
    if a.dtype == np.uint64:
        raise ValueError(f"{what} must not be a uint64 column: numba subtracts it from a signed column in float64")
    a = a.astype(np.int64, copy=False)
    if len(a) and max(int(a.max()), -int(a.min())) >= backend.KINETICS_FRAME_LIMIT:
        raise ValueError(f"{what} must stay below 2**62 in magnitude")
    return a


def _dark_times(frame, group, last_frame) -> np.ndarray:
    """The dark time before every binding event (postprocess.py:1985-2004): the smallest ``frame[i] - last_frame[j]``
    that is positive and below ``frame.max()`` over the other events j of the group, -1 where there is none.  The
    array has the dtype numba gives ``max_frame * np.ones(N, dtype=np.int32)``: int64 for a uint32 or int64 ``frame``,
    int32 for an int32 one.  An empty table raises NumPy's ValueError for ``frame.max()``, as the reference does."""
    frame, last_frame = np.asarray(frame), np.asarray(last_frame)
    labels = _group_labels(group)
    f, lf = _frame_numbers(frame, "frame"), _frame_numbers(last_frame, "last_frame")
    if not (len(f) == len(lf) == len(labels)):
        raise ValueError("frame, group and last_frame must have one length")
    frame.max()                              # the reference's first line: an empty table raises here
    dark = backend.DarkTable(f, labels, lf).search()
    return dark.astype(np.result_type(frame.dtype, np.int32), copy=False)


def dark_times(locs: pd.DataFrame, group=None) -> np.ndarray:
    """Dark times of the binding events ``locs`` (postprocess.py:1952-1982); ``group`` defaults to the ``group``
    column and, without one, to one group of all events."""
    frame = locs["frame"].to_numpy()
    lens = locs["len"].to_numpy()
    with np.errstate(over="ignore"):
        last_frame = frame + lens - 1        # in the columns' own dtypes, as in the reference
    if group is None:
        if "group" in locs.columns:
            group = locs["group"].to_numpy()
        else:
            group = np.zeros(len(locs))
    dark = _dark_times(frame, group, last_frame)
    return dark


def compute_dark_times(locs: pd.DataFrame, group=None) -> pd.DataFrame:
    """Adds the int32 column ``dark`` to ``locs`` IN PLACE, as the reference does, and returns the events that have a
    dark time (postprocess.py:1920-1949)."""
    if "len" not in locs.columns:
        raise AttributeError("Length not found. Please link localizations first.")
    dark = dark_times(locs, group)
    locs["dark"] = np.int32(dark)
    locs = locs[locs.dark != -1]
    return locs


# ---- group properties (postprocess.py:3580-3649) --------------------------------------------------------------
def groupprops(locs: pd.DataFrame, callback: Callable[[int], None] | Literal["console"] | None = None) -> pd.DataFrame:
    """Mean and standard deviation of every column per group (postprocess.py:3580-3649): ``group``, ``n_events``,
    then ``<c>_mean``, ``<c>_std`` for every column in table order, and ``qpaint_idx = 1 / dark_mean``; events
    without a dark time (``dark == -1``) are left out first.  A table without a ``dark`` column raises KeyError, as
    in the reference (whose ``try`` expects an AttributeError that pandas does not raise).  All groups are computed in
    one pass on the device; a callable ``callback`` then sees 0 .. n - 1 and n, ``"console"`` shows a tqdm bar."""
    try:
        locs = locs[locs["dark"] != -1]
    except AttributeError:
        pass
    names = list(locs.columns)
    out = OrderedDict()
    if len(locs) == 0:
        n = 0
        group_ids = np.unique(locs["group"])
        stats = [(np.zeros(0), np.zeros(0))] * len(names)
        n_events = np.zeros(0, np.int64)
    else:
        groups = backend.CenterGroups(_group_labels(locs["group"].to_numpy()))
        group_ids, n_events, n = groups.unique, groups.n_locs, groups.n_groups
        stats = backend.group_mean_std(groups, [locs[c].to_numpy() for c in names])
    with np.errstate(all="ignore"):
        # the reference stores every scalar into a float64 frame and casts at the end
        out["group"] = np.asarray(group_ids).astype(np.float64).astype(np.int32)
        out["n_events"] = np.asarray(n_events).astype(np.float64).astype(np.int32)
        for c, (mean, std) in zip(names, stats):
            for key, held in ((c + "_mean", mean), (c + "_std", std)):
                held = np.array(held, np.float64)
                held[np.isnan(held)] = np.nan        # DataFrame.loc stores any NaN as pandas' own
                out[key] = held.astype(np.float32)
    if callback == "console":
        from tqdm import tqdm
        for _ in tqdm(range(n), desc="Calculating group statistics", unit="Groups"):
            pass
    elif callable(callback):
        for i in range(n):
            callback(i)
        callback(n)
    groups_df = pd.DataFrame(out)
    if "dark_mean" in groups_df.columns:
        groups_df["qpaint_idx"] = 1 / groups_df["dark_mean"]
    return groups_df


# ---- nearest-neighbour distances (postprocess.py:3704-3739, spinna.py:696-747) ------------------------------------
def _kdtree_points(X2) -> np.ndarray:
    """``KDTree(X2)`` as far as it decides anything: the float64 points, refused where scipy refuses them."""
    X2 = np.asarray(X2)
    if X2.ndim != 2:
        raise ValueError(f"data must be of shape (n, m), where there are n points of dimension m, not {X2.shape}")
    X2 = np.ascontiguousarray(X2, np.float64)
    if not np.isfinite(X2).all():
        raise ValueError("data must be finite, check for nan or inf values")
    return X2


def _knn_table(points: np.ndarray, X1, k: int, index=None) -> np.ndarray:
    """The distances of ``KDTree(points).query(X1, k)`` for a 2-D ``X1`` as a table: float64, always (N, k), inf where
    the tree has fewer than k points.  scipy's own refusals come first and before any device work, then this package's
    limits: 2 or 3 columns, and k at most ``backend.knn_limit()``.  ``index`` is a ``backend.KnnIndex`` of ``points``
    made earlier."""
    X1 = np.ascontiguousarray(X1, np.float64)
    if not np.isfinite(X1).all():
        raise ValueError("'x' must be finite, check for nan or inf values")
    k = int(k)
    if k < 1:
        raise ValueError("zero-size array to reduction operation maximum which has no identity")
    if points.shape[1] not in (2, 3):
        raise NotImplementedError(f"nearest neighbours on the device take 2 or 3 dimensions, not {points.shape[1]}")
    if X1.ndim != 2 or X1.shape[1] != points.shape[1]:
        raise ValueError(f"x must consist of vectors of length {points.shape[1]} but has shape {X1.shape}")
    limit = backend.knn_limit()
    if k > limit:
        raise ValueError(f"{k} neighbours per point (a dropped self column counts) exceed the device limit of {limit}")
    if len(X1) == 0 or len(points) == 0:
        distances = np.full((len(X1), k), np.inf)
    else:
        if index is None:
            index = backend.KnnIndex(points, k)
        distances = index.query(X1, k)
    return distances


def _kdtree_query(points: np.ndarray, X1, k: int, index=None) -> np.ndarray:
    """``_knn_table`` in the shape scipy gives it: (N,) when one neighbour is asked for."""
    table = _knn_table(points, X1, k, index)
    return table[:, 0] if table.shape[1] == 1 else table


def nn_analysis(X1, X2, nn_count: int) -> np.ndarray:
    """Distances from every row of ``X1`` to its ``nn_count`` nearest rows of ``X2`` (postprocess.py:3704-3739),
    float64 and ascending, in every bit what the reference's KDTree query returns.  When the two sets hold the same
    values one more neighbour is found and the first column (the point itself) is dropped.  The reference's final
    reshape does nothing, so ``nn_count == 1`` on two different sets returns a 1-D (N,) array; rows past the number
    of points of ``X2`` are inf.  Non-finite coordinates and ``nn_count <= 0`` raise what scipy raises."""
    if X1.shape[1] != X2.shape[1]:
        raise ValueError("X1 and X2 must have the same number of dimensions.")
    points = _kdtree_points(X2)
    if np.array_equal(X1, X2):
        if int(nn_count) + 1 == 1:               # the query of one neighbour is 1-D and has no column to drop
            raise IndexError("too many indices for array: array is 1-dimensional, but 2 were indexed")
        nn = _kdtree_query(points, X1, nn_count + 1)[:, 1:]
    else:
        nn = _kdtree_query(points, X1, nn_count)
    return nn


# ---- cluster combine (postprocess.py:2174-2419) ------------------------------------------------------------------
def _combine_labels(locs: pd.DataFrame):
    """The ``group`` and ``cluster`` columns as int64 labels, by the rule of ``_group_labels``.  Narrower than the
    reference, which compares any values: non-integral or non-finite labels are refused (ValueError) before device
    work."""
    labels = []
    for name in ("group", "cluster"):
        try:
            labels.append(_group_labels(locs[name].to_numpy()))
        except TypeError as e:
            raise ValueError(str(e).replace("group", name)) from None
        except ValueError as e:
            raise ValueError(str(e).replace("group", name)) from None
    return labels


def _average_pair(col: np.ndarray, weights: np.ndarray):
    """``col`` and ``weights`` in the type ``np.average`` multiplies and sums them in."""
    if col.dtype.kind in "iub":
        dtype = np.result_type(col.dtype, weights.dtype, "f8")
    else:
        dtype = np.result_type(col.dtype, weights.dtype)
    if dtype not in (np.dtype(np.float32), np.dtype(np.float64)):
        raise TypeError(f"the weighted average on the device takes float32 or float64, not {dtype}")
    return col.astype(dtype, copy=False), weights.astype(dtype, copy=False)


def cluster_combine(locs: pd.DataFrame) -> pd.DataFrame:
    """One row per (``group``, ``cluster``) pair (postprocess.py:2174-2288), groups ascending and clusters ascending
    within a group: ``group`` (float64), ``cluster`` (the column's dtype), ``mean_frame``, ``x``, ``y`` (``z``),
    ``std_frame``, ``lpx``, ``lpy`` (``lpz``) as float32 and ``n`` as int32, with a RangeIndex, in the reference's
    values: ``mean_frame`` / ``std_frame`` are pandas' ``Series.mean()`` / ``Series.std()`` of ``frame``, ``x`` .. are
    ``np.average(column, weights=photons)`` in ``np.result_type`` of the two, ``lpx`` .. are ``Series.std()`` of the
    column over ``np.sqrt(n)``; a cluster of one row has NaN ``std_frame`` and ``lp*``.  A cluster whose weights sum
    to exactly zero raises ``np.average``'s ZeroDivisionError; an empty table raises ``pd.concat``'s ValueError.
    Narrower than the reference: ``group`` and ``cluster`` must hold integers (or finite, integral floats), anything
    else raises ValueError before device work.  All pairs are computed in one pass on the device."""
    axes = ("x", "y", "z") if "z" in locs.columns else ("x", "y")
    group, cluster = locs["group"], locs["cluster"]
    columns = {c: locs[c].to_numpy() for c in ("frame", "photons") + axes}
    if len(locs) == 0:
        return pd.concat([], ignore_index=True)           # what the reference's loop over no group ends in
    g_labels, c_labels = _combine_labels(locs)
    pairs = [_average_pair(columns[a], columns["photons"]) for a in axes]
    groups = backend.CombineGroups(g_labels, c_labels)
    moments, averages = backend.combine_stats(groups, [columns["frame"]] + [columns[a] for a in axes], pairs)
    if any((scl == 0.0).any() for _, scl in averages):
        raise ZeroDivisionError("Weights sum to zero, can't be normalized")
    n = groups.n_locs
    out = OrderedDict()
    with np.errstate(all="ignore"):
        out["group"] = groups.unique.astype(np.float64)
        out["cluster"] = groups.clusters.astype(cluster.to_numpy().dtype)
        out["mean_frame"] = moments[0][0].astype(np.float32)
        for a, (avg, _) in zip(axes, averages):
            out[a] = avg.astype(np.float32)
        out["std_frame"] = moments[0][1].astype(np.float32)
        for a, (_, std) in zip(axes, moments[1:]):
            out["lp" + a] = (std / np.sqrt(n)).astype(np.float32)
        out["n"] = n.astype(np.int32)
    return pd.DataFrame(out)


def _check_combined(g_labels: np.ndarray, c_labels: np.ndarray) -> None:
    """What the reference's loop runs into, group after group, before any device work: a group of one distinct cluster
    takes ``np.amin`` of no distance, a group with a repeated cluster label builds a frame from arrays of two
    lengths."""
    order = np.lexsort((c_labels, g_labels))
    gs, cs = g_labels[order], c_labels[order]
    first = np.flatnonzero(np.r_[True, gs[1:] != gs[:-1]])
    rows = np.diff(np.r_[first, len(gs)])
    distinct = np.add.reduceat(np.r_[True, (gs[1:] != gs[:-1]) | (cs[1:] != cs[:-1])].astype(np.int64), first)
    bad = np.flatnonzero((distinct == 1) | (distinct < rows))
    if len(bad):
        if distinct[bad[0]] == 1:
            raise ValueError("zero-size array to reduction operation minimum which has no identity")
        raise ValueError("All arrays must be of the same length")


def cluster_combine_dist(locs: pd.DataFrame, pixelsize: float | None = None) -> pd.DataFrame:
    """The table of ``cluster_combine`` with the distance from every cluster to the nearest other cluster of its group
    (postprocess.py:2291-2419): ``min_dist`` over x, y and ``z / pixelsize`` when the table has ``z`` (``pixelsize`` 130
    when None) plus ``mind_dist_xy`` (the reference's spelling) over x and y; a table without ``z`` gets ``min_dist``
    over x and y only.  In the reference's values:

    * Distance arithmetic: ``scipy.spatial.distance.cdist`` on the columns promoted to float64,
      ``sqrt(((dx*dx) + (dy*dy)) + (dz*dz))`` without contraction; the minimum of the squares followed by one root
      equals ``np.amin`` of the distances, because the root is monotone and correctly rounded.  The row itself is left
      out by position: two clusters at one place are 0 apart.  The result is cast to float32.
    * z scaling: ``z / pixelsize`` is the reference's own NumPy expression, computed on the host, so a float32 ``z``
      stays float32 under a Python number and becomes float64 under an ``np.float64``.
    * Column alignment: groups ascend; within a group ``cluster`` is ``np.unique``-sorted and ``min_dist[i]`` belongs
      to the i-th SORTED cluster, while the copied columns (cast as the reference casts them: float32, ``n`` int32,
      ``group`` as it is) stay in table order.  For a table that came from ``cluster_combine`` the two coincide; for
      one that did not, the rows are misaligned the way the reference's are.
    * A group of a single cluster raises ValueError (the reference's ``np.amin`` of an empty array), a cluster label
      repeated within a group raises ValueError (pandas' length mismatch), an empty table raises ``pd.concat``'s
      ValueError, and labels that are not integral raise ValueError: all before device work."""
    three = "z" in locs.columns
    names = ("mean_frame", "x", "y") + (("z",) if three else ()) + ("std_frame", "lpx", "lpy") + (("lpz",) if three else ())
    group, cluster = locs["group"].to_numpy(), locs["cluster"].to_numpy()
    held = {c: locs[c].to_numpy() for c in names + ("n",)}
    if len(locs) == 0:
        return pd.concat([], ignore_index=True)
    g_labels, c_labels = _combine_labels(locs)
    _check_combined(g_labels, c_labels)
    if three:
        pixelsize = 130 if pixelsize is None else pixelsize
        points = np.stack((held["x"], held["y"], held["z"] / pixelsize), axis=1)
    else:
        points = np.array(locs[["x", "y"]])
    points = np.ascontiguousarray(points, np.float64)                 # what cdist converts to
    groups = backend.CombineGroups(g_labels, c_labels)
    min_dist, min_dist_xy = backend.combine_min_distances(groups, points)
    by_group = np.argsort(g_labels, kind="stable")                    # the reference's boolean mask per ascending group
    out = OrderedDict()
    with np.errstate(all="ignore"):
        out["group"] = group[by_group]
        out["cluster"] = groups.clusters.astype(cluster.dtype)
        for c in names:
            out[c] = held[c][by_group].astype(np.float32)
        out["n"] = held["n"][by_group].astype(np.int32)
        out["min_dist"] = min_dist.astype(np.float32)
        if three:
            out["mind_dist_xy"] = min_dist_xy.astype(np.float32)
    return pd.DataFrame(out)


# ---- Fourier ring correlation (postprocess.py:1320-1502) ----------------------------------------------------------
FRC_NAMES = ("frc", "_frc")


def frc(locs: pd.DataFrame, info, viewport, *, random_seed: int = 42) -> dict:
    """Fourier ring correlation resolution (postprocess.py:1320-1395; Nieuwenhuizen et al., Nat. Methods 10, 557-562).
    -> dict with "frc_curve", "frc_curve_smooth", "frequencies" (nm^-1), "resolution" (nm, or None) and "images" (the
    two rendered and masked half-data images).  The split uses NumPy's legacy global generator, as the reference does:
    it is part of the result."""
    pixelsize = lib.get_from_metadata(info, "Pixelsize", raise_error=True)
    lp = nena(locs, info)[1]
    # correct for the viewport to be square
    viewport_width = viewport[1][1] - viewport[0][1]
    viewport_height = viewport[1][0] - viewport[0][0]
    if viewport_width < viewport_height:
        y_center = 0.5 * (viewport[0][0] + viewport[1][0])
        y_min = y_center - viewport_width / 2
        y_max = y_center + viewport_width / 2
        viewport = ((y_min, viewport[0][1]), (y_max, viewport[1][1]))
    elif viewport_height < viewport_width:
        x_center = 0.5 * (viewport[0][1] + viewport[1][1])
        x_min = x_center - viewport_height / 2
        x_max = x_center + viewport_height / 2
        viewport = ((viewport[0][0], x_min), (viewport[1][0], x_max))

    # select the locs within the viewport
    (y_min, x_min), (y_max, x_max) = viewport
    in_view = (locs["x"] > x_min) & (locs["y"] > y_min) & (locs["x"] < x_max) & (locs["y"] < y_max)
    locs = locs.loc[in_view]

    np.random.seed(random_seed)
    # split locs randomly into two halves
    r_idx = np.random.permutation(len(locs))
    locs1 = locs.iloc[r_idx[: len(r_idx) // 2]]
    locs2 = locs.iloc[r_idx[len(r_idx) // 2:]]
    frc_curve, frc_curve_smooth, frequencies, resolution, images = _frc(locs1, locs2, pixelsize, lp, viewport)
    return {"frc_curve": frc_curve, "frc_curve_smooth": frc_curve_smooth, "frequencies": frequencies,
            "resolution": resolution, "images": images}


def _frc_render(locs, info, oversampling, viewport):
    """``render.render(locs, info, oversampling, viewport, None)[1]`` with the image left on the device: the head of
    ``render.render`` expression for expression (the deprecated positional oversampling goes through the display pixel
    size and back), then the histogram kernel."""
    pixelsize = lib.get_from_metadata(info, "Pixelsize", raise_error=True)
    lib.deprecation_warning("Deprecation warning: the 'oversampling' parameter is deprecated and will be removed "
                            "in v0.11.0. Use 'disp_px_size' instead.")
    disp_px_size = pixelsize / oversampling
    oversampling = pixelsize / disp_px_size
    (y_min, x_min), (y_max, x_max) = viewport
    return backend.render_hist_device(locs["x"].to_numpy(), locs["y"].to_numpy(), oversampling, y_min, x_min, y_max, x_max)[1]


def _frc_curve(im1, im2):
    """Two square float32 renders of one side (host or device) -> (curve, (masked image 1, masked image 2), details):
    the crop to an odd side, the Tukey window, the two transforms and the ring sums on the device (csrc/frc.hip).  The
    curve is float64: the device transforms in double precision where the reference's ``np.fft.fft2`` of a float32
    image works in single."""
    from . import masking
    m = int(im1.shape[0])
    w = masking.tukey_profile(m if m % 2 else m - 1)
    out = backend.frc_arrays(im1, im2, w)
    return out["curve"], out["images"], out


def _fire_resolution(frequencies, smooth, threshold: float = 1 / 7):
    """The first crossing of the smoothed curve below the threshold, linearly interpolated -> resolution in nm, or None
    (postprocess.py:1487-1501)."""
    resolution = None
    for i in range(1, len(smooth)):
        if smooth[i - 1] >= threshold and smooth[i] < threshold:
            # linear interpolation
            f1 = frequencies[i - 1]
            f2 = frequencies[i]
            r1 = smooth[i - 1]
            r2 = smooth[i]
            f_res = f1 + (threshold - r1) * (f2 - f1) / (r2 - r1)
            resolution = 1 / f_res  # in nm
            break
    return resolution


def _frc(locs1: pd.DataFrame, locs2: pd.DataFrame, pixelsize: float, lp: float, viewport):
    """One FRC curve and its resolution at the 1/7 threshold (postprocess.py:1398-1502) -> (frc_curve,
    frc_curve_smooth, frequencies, resolution, (image 1, image 2)).  The renders, the window, the transforms and the
    ring sums stay on the device; the masked images and the curve come back.  The smoothing is statsmodels' LOESS on
    the host (``masking.loess_smooth``)."""
    from . import masking
    # render images
    binsize = lp / 2
    oversampling = 1 / binsize
    dummy_info = {"Pixelsize": pixelsize}
    im1 = _frc_render(locs1, dummy_info, oversampling, viewport)
    im2 = _frc_render(locs2, dummy_info, oversampling, viewport)
    if im1.shape[0] != im1.shape[1]:
        raise AssertionError("Image must be square")          # threshold_tukey's assertion (masking.py:662)
    frc_curve, images, _ = _frc_curve(im1, im2)
    side = images[0].shape[0]

    # smooth the frc curve
    sspan = max(int(np.ceil(int(side / 2) / 20)), 5)
    frc_curve_smooth = masking.loess_smooth(frc_curve, sspan)

    # find the frequencies (q) and resolution
    frequencies = np.arange(len(frc_curve)) / side / (pixelsize * binsize)
    resolution = _fire_resolution(frequencies, frc_curve_smooth)
    return frc_curve, frc_curve_smooth, frequencies, resolution, images


# ---- picked localizations (postprocess.py:207-473, :739-799) --------------------------------------------------
# Not rebound by localize.install(): the reference's picks family (pick_similar, the pick kinetics) hands picked_locs
# a K x L ``index_blocks`` tuple, which this module does not build.
PICK_NAMES = ("picked_locs", "_picked_circular_locs", "_picked_rectangular_locs", "_picked_polygonal_locs",
              "_picked_square_locs", "remove_locs_in_picks")


def _pick_done(i: int, callback, progress) -> None:
    if callback == "console":
        progress.update(1)
    elif callback is not None:
        callback(i + 1)


def _pick_frames(locs: pd.DataFrame, offsets, rows, positions, add_group: bool, callback, progress, n_picks: int,
                 finish=None) -> list[pd.DataFrame]:
    """One frame per pick from the device's CSR pair: the member rows in the reference's order before its sort, then
    the reference's own pandas calls (copy, ``group``, the quicksort by frame, which is not stable)."""
    picked, at = [], dict(zip(positions, range(len(positions))))
    for i in range(n_picks):
        if i in at:
            group_locs = locs.iloc[rows[offsets[at[i]]:offsets[at[i] + 1]]].copy()
            if finish is not None:
                finish(i, group_locs)
            if add_group:
                group_locs["group"] = i
            group_locs.sort_values(by="frame", kind="quicksort", inplace=True)
            picked.append(group_locs)
        _pick_done(i, callback, progress)
    return picked


def _refuse_index_blocks(index_blocks) -> None:
    if index_blocks is not None:
        raise NotImplementedError("index_blocks: the K x L block table of get_index_blocks is not built here; "
                                  "pass None and the blocks are ordered on the device")


def _pick_bounds(boxes):
    """(P, 4) float64 bounds and the weak-scalar bits of each: a Python int or float is compared in the column's dtype,
    a NumPy scalar in the common type (NumPy 2 promotion, which the reference's pandas masks follow)."""
    bounds = np.array([[float(v) for v in b] for b in boxes], np.float64).reshape(-1, 4)
    flags = np.array([sum(1 << k for k, v in enumerate(b) if not isinstance(v, np.generic)) for b in boxes], np.uint8)
    return bounds, flags


def _keeps_float32(v) -> bool:
    """numba: ``float32[:] (op) v`` stays float32 for an integer or float32 scalar, a float64 one widens it."""
    return isinstance(v, (bool, int, np.integer, np.bool_, np.float32, np.float16))


def _circle_members(locs: pd.DataFrame, info: list[dict], picks: list[tuple], pick_size: float, with_table: bool = False):
    """-> (the sanity-filtered table, offsets, rows): the members of circular picks as positions in that table, in the
    reference's order before its sort by frame; all picks in one device call.  ``with_table`` appends the
    backend.BlockTable the call ordered the rows with."""
    locs, table = _block_table(locs, info, pick_size)
    block_x = [int(x / pick_size) for x, _ in picks]
    block_y = [int(y / pick_size) for _, y in picks]
    # the reference stacks x and y into one array: a float32 beside a float64 column is float64 before any arithmetic
    both32 = locs["x"].dtype == np.float32 and locs["y"].dtype == np.float32
    flags = [((1 if _keeps_float32(x) else 0) | (2 if _keeps_float32(y) else 0) | (4 if _keeps_float32(pick_size) else 0))
             if both32 else 0 for x, y in picks]
    if isinstance(pick_size, np.float32):
        r2 = float(pick_size * pick_size)
    elif isinstance(pick_size, (int, np.integer)):
        r2 = float(int(pick_size) ** 2)
    else:
        r2 = float(np.float64(pick_size) * np.float64(pick_size))
    offsets, rows = backend.picks_circle(table, locs["x"].to_numpy(), locs["y"].to_numpy(), [float(x) for x, _ in picks],
                                         [float(y) for _, y in picks], block_x, block_y, flags, r2)
    return (locs, offsets, rows, table) if with_table else (locs, offsets, rows)


def _picked_circular_locs(locs: pd.DataFrame, info: list[dict], picks: list[tuple], pick_size: float,
                          index_blocks: tuple | None, add_group: bool,
                          callback: Callable[[int], None] | Literal["console"] | None, progress: tqdm | None) -> list[pd.DataFrame]:
    """Circular picks (postprocess.py:207-253): the sanity-filtered table in block order, the nine blocks around each
    pick, ``dx**2 + dy**2 < r**2`` as numba types it; all picks in one device call."""
    _refuse_index_blocks(index_blocks)
    locs, offsets, rows = _circle_members(locs, info, picks, pick_size)
    return _pick_frames(locs, offsets, rows, range(len(picks)), add_group, callback, progress, len(picks))


def _picked_rectangular_locs(locs: pd.DataFrame, picks: list[tuple], pick_size: float, add_group: bool,
                             callback: Callable[[int], None] | Literal["console"] | None, progress: tqdm | None) -> list[pd.DataFrame]:
    """Rectangular picks (postprocess.py:256-298): the strict bounding box, the four-sided ray count, and the rotated
    coordinates from the subset with the reference's own pandas expressions."""
    corners = [lib.get_pick_rectangle_corners(xs, ys, xe, ye, pick_size) for (xs, ys), (xe, ye) in picks]
    bounds, flags = _pick_bounds([(min(X), max(X), min(Y), max(Y)) for X, Y in corners])
    offsets, rows = backend.picks_rectangle(locs["x"].to_numpy(), locs["y"].to_numpy(), bounds, flags,
                                            [X for X, _ in corners], [Y for _, Y in corners])

    def rotated(i, group_locs):
        (xs, ys), (xe, ye) = picks[i]
        angle = 0.5 * np.pi - np.arctan2((ye - ys), (xe - xs))
        x_shifted = group_locs["x"] - xs
        y_shifted = group_locs["y"] - ys
        group_locs["x_pick_rot"] = x_shifted * np.cos(angle) - y_shifted * np.sin(angle)
        group_locs["y_pick_rot"] = x_shifted * np.sin(angle) + y_shifted * np.cos(angle)

    return _pick_frames(locs, offsets, rows, range(len(picks)), add_group, callback, progress, len(picks), rotated)


def _picked_polygonal_locs(locs: pd.DataFrame, picks: list[tuple], add_group: bool,
                           callback: Callable[[int], None] | Literal["console"] | None, progress: tqdm | None):
    """Polygonal picks (postprocess.py:301-335): unclosed polygons are skipped (``group`` keeps the pick's position);
    the strict bounding box, then the ray casting over the corners."""
    kept, corners = [], []
    for i, pick in enumerate(picks):
        X, Y = lib.get_pick_polygon_corners(pick)
        if X is not None:
            kept.append(i)
            corners.append((X, Y))
    bounds, flags = _pick_bounds([(min(X), max(X), min(Y), max(Y)) for X, Y in corners])
    corner_offsets = np.zeros(len(corners) + 1, np.int32)
    corner_offsets[1:] = np.cumsum([len(X) for X, _ in corners])
    corner_x = np.array([v for X, _ in corners for v in X], np.float64)
    corner_y = np.array([v for _, Y in corners for v in Y], np.float64)
    offsets, rows = backend.picks_polygon(locs["x"].to_numpy(), locs["y"].to_numpy(), bounds, flags, corner_offsets,
                                          corner_x, corner_y)
    return _pick_frames(locs, offsets, rows, kept, add_group, callback, progress, len(picks))


def _picked_square_locs(locs: pd.DataFrame, picks: list[tuple], pick_size: float, add_group: bool,
                        callback: Callable[[int], None] | Literal["console"] | None, progress: tqdm | None) -> list[pd.DataFrame]:
    """Square picks (postprocess.py:338-372): the strict box of side ``pick_size`` around each pick."""
    half_a = pick_size / 2
    bounds, flags = _pick_bounds([(x - half_a, x + half_a, y - half_a, y + half_a) for x, y in picks])
    offsets, rows = backend.picks_square(locs["x"].to_numpy(), locs["y"].to_numpy(), bounds, flags)
    return _pick_frames(locs, offsets, rows, range(len(picks)), add_group, callback, progress, len(picks))


PICK_SHAPES = ("Circle", "Rectangle", "Polygon", "Square")


def picked_locs(locs: pd.DataFrame, info: list[dict], picks: list[tuple],
                pick_shape: Literal["Circle", "Rectangle", "Polygon", "Square"], pick_size: float = None,
                add_group: bool = True, index_blocks: tuple = None,
                callback: Callable[[int], None] | Literal["console"] | None = None) -> list[pd.DataFrame]:
    """The localizations within each pick (postprocess.py:375-473): a list of frames, one per pick, each a copy of the
    member rows with their index labels, ``group`` = the pick's position when ``add_group``, sorted by frame.
    ``pick_size`` is the radius of a circle, the width of a rectangle, the side of a square.  The members of all picks
    are found in one device call; a non-None ``index_blocks`` is refused.  ``callback`` sees 1 .. len(picks), or is
    ``"console"`` for a tqdm bar."""
    assert pick_shape in PICK_SHAPES, f"Invalid pick shape: {pick_shape}. Choose one of {PICK_SHAPES}."
    if len(picks) == 0:
        return []
    progress = None
    if callback == "console":
        from tqdm import tqdm
        progress = tqdm(range(len(picks)), desc="Picking locs", unit="pick")
    common = dict(locs=locs, picks=picks, add_group=add_group, callback=callback, progress=progress)
    if pick_shape == "Circle":
        return _picked_circular_locs(info=info, pick_size=pick_size, index_blocks=index_blocks, **common)
    if pick_shape == "Polygon":
        return _picked_polygonal_locs(**common)
    by_size = _picked_rectangular_locs if pick_shape == "Rectangle" else _picked_square_locs
    return by_size(pick_size=pick_size, **common)


def remove_locs_in_picks(locs: pd.DataFrame, info: list[dict], *, picks: list[tuple],
                         pick_shape: Literal["Circle", "Rectangle", "Polygon", "Square"],
                         pick_size: float | None = None, index_blocks: tuple = None) -> pd.DataFrame:
    """Drop the localizations inside the picks from ``locs`` itself and return it (postprocess.py:739-799).  For
    circles ``pick_size`` is the DIAMETER here and is halved (an integer diameter gives a float radius); for the other
    shapes ``index_blocks`` is ignored.  Overlapping picks name a row twice, which ``drop`` takes."""
    assert pick_shape in PICK_SHAPES, "pick_shape must be one of 'Circle', 'Rectangle', 'Polygon', or 'Square'."
    assert pick_shape == "Polygon" or isinstance(pick_size, (int, float)), "pick_size must be a number."
    circle = pick_shape == "Circle"
    inside = picked_locs(locs=locs, info=info, picks=picks, pick_shape=pick_shape,
                         pick_size=pick_size / 2 if circle else pick_size, add_group=False,
                         index_blocks=index_blocks if circle else None)
    locs.drop(index=np.concatenate([frame.index for frame in inside]), inplace=True)
    return locs


# ---- fiducial undrift (postprocess.py:2964-3156) ----------------------------------------------------------------
# Not rebound by localize.install(), like the picks they are built on.
FIDUCIAL_NAMES = ("undrift_from_fiducials", "undrift_from_picked", "_undrift_from_picked_coordinate")


def _picked_csr(picked_locs: list[pd.DataFrame], names):
    """The frames of ``picked_locs`` as one CSR: offsets, the frame column and the coordinate columns in pick order.  A
    coordinate must have one dtype in all picks (as the columns of one table have): the mean of a pick is taken in it."""
    offsets = np.zeros(len(picked_locs) + 1, np.int64)
    offsets[1:] = np.cumsum([len(locs) for locs in picked_locs])

    def column(name):
        parts = [locs[name].to_numpy() for locs in picked_locs]
        if len({p.dtype for p in parts}) > 1:
            raise TypeError(f"column {name!r} has the dtypes {sorted({str(p.dtype) for p in parts})} among the picks; "
                            "the drift takes one float32 or float64 column")
        return np.concatenate(parts) if parts else np.zeros(0, np.float64)

    return offsets, column("frame"), [column(name) for name in names]


def _drift_from_picked(picked_locs: list[pd.DataFrame], info, names) -> np.ndarray:
    offsets, frame, columns = _picked_csr(picked_locs, names)
    return backend.fiducials_drift(offsets, frame, columns, info[0]["Frames"])


def _undrift_from_picked_coordinate(picked_locs: list[pd.DataFrame], info: list[dict],
                                    coordinate: Literal["x", "y", "z"]) -> lib.FloatArray1D:
    """The drift of one coordinate over all frames (postprocess.py:3098-3156): every pick minus its own mean, the mean
    over the picks weighted by the inverse of each pick's mean square deviation, frames without a localization
    interpolated; one device call, equal to the reference under NumPy 2 in every bit."""
    return np.ascontiguousarray(_drift_from_picked(picked_locs, info, [coordinate])[:, 0])


def undrift_from_picked(picked_locs: list[pd.DataFrame], info: list[dict]) -> pd.DataFrame:
    """The drift (not the undrifted localizations) from picked localizations (postprocess.py:3062-3095): a frame with
    ``x``, ``y`` and, if every pick has it, ``z``; all coordinates in one device call."""
    names = ["x", "y"] + (["z"] if all("z" in locs.columns for locs in picked_locs) else [])
    drift = _drift_from_picked(picked_locs, info, names)
    return pd.DataFrame({name: drift[:, k] for k, name in enumerate(names)})


def undrift_from_fiducials(locs: pd.DataFrame, info: list[dict], picks: list[tuple] | None = None,
                           pick_size: float | None = None, undrift_z: bool = True,
                           index_blocks: tuple | None = None) -> tuple[pd.DataFrame, list[dict], pd.DataFrame]:
    """Undrift by picked fiducial markers (postprocess.py:2964-3059) -> (undrifted copy, info with one more entry,
    drift).  ``picks`` are (x, y) centres and ``pick_size`` the pick radius in camera pixels.  The members of the
    circular picks come from the device as row numbers; no per-pick frame is built: the host orders each pick's rows
    as the reference's quicksort by frame does (the order decides the bits of a pick's mean, and which of two rows of
    one frame counts), gathers frame, x, y (, z) and makes one device call.  ``picks=None`` (``find_fiducials``) and a
    non-None ``index_blocks`` are refused."""
    from . import __version__
    locs = locs.copy()
    pixelsize = lib.get_from_metadata(info, "Pixelsize", raise_error=True)
    if picks is None:
        raise NotImplementedError("picks=None is not routed here: call imageprocess.find_fiducials and pass its picks and box / 2")
    if pick_size is None:
        raise ValueError("pick_size (radius in camera pixels) must be provided when picks are given as a list of "
                         "coordinates.")
    pick_radius = pick_size
    if len(picks) == 0:
        raise ValueError("No picks found for drift correction.")
    _refuse_index_blocks(index_blocks)
    sane, offsets, rows = _circle_members(locs, info, picks, pick_radius)
    frame = sane["frame"].to_numpy()
    for a, b in zip(offsets[:-1], offsets[1:]):          # sort_values(by="frame", kind="quicksort") of the pick's subset
        rows[a:b] = rows[a:b][np.argsort(frame[rows[a:b]], kind="quicksort")]
    names = ["x", "y"] + (["z"] if "z" in sane.columns else [])
    values = backend.fiducials_drift(offsets, frame[rows], [sane[name].to_numpy()[rows] for name in names], info[0]["Frames"])
    drift = pd.DataFrame({name: values[:, k] for k, name in enumerate(names)})
    if not undrift_z:
        drift = drift.drop(columns="z", errors="ignore")
    locs = apply_drift(locs, info, drift=drift)
    new_info = info + [{"Generated by": f"Picasso v{__version__} Undrift from picked", "Number of picks": len(picks),
                        "Pick radius (nm)": pick_radius * pixelsize}]
    return locs, new_info, drift


# ---- channel alignment (postprocess.py:3296-3443) ------------------------------------------------------------------
# Not rebound by localize.install().  Host compositions over the one-pixel-blur render (csrc/blur.hip) and the RCC.
ALIGN_NAMES = ("align", "align_rcc")


def align(locs: list[pd.DataFrame], infos: list[dict], display: bool = False, *, apply_shifts: bool = True,
          return_shifts: bool = False) -> pd.DataFrame:
    """Align the channels in ``locs`` by the RCC shifts between their rendered images (postprocess.py:3296-3349): one
    ``"smooth"`` render per channel at oversampling 1 over the whole frame, ``imageprocess.rcc`` over the images, and,
    when ``apply_shifts``, ``x`` and ``y`` of each of the caller's tables shifted in place.  ``return_shifts`` adds
    ``(shift_x, shift_y)``.  ``display`` is not used.  A channel without ``Pixelsize`` raises KeyError as in the
    reference's ``render.render``."""
    images = []
    for locs_, info_ in zip(locs, infos):
        lib.get_from_metadata(info_, "Pixelsize", raise_error=True)
        (y_min, x_min), (y_max, x_max) = render._viewport(info_, None)
        _, image = render._render_smooth(locs_, 1.0, y_min, x_min, y_max, x_max)
        images.append(image)
    shift_y, shift_x = imageprocess.rcc(images, callback=lambda _: None)
    if apply_shifts:
        for i, (locs_, dx, dy) in enumerate(zip(locs, shift_x, shift_y)):
            locs_["y"] -= dy
            locs_["x"] -= dx
    if return_shifts:
        shifts = (shift_x, shift_y)
        return locs, shifts
    else:
        return locs


def align_rcc(locs: list[pd.DataFrame], infos: list[list[dict]], display: bool = False,
              return_shifts: bool = False) -> pd.DataFrame:
    """``align`` repeated on a deep copy until every channel's ``|dx| + |dy|`` is at most 0.001 px, five times at the
    most (postprocess.py:3352-3443).  ``return_shifts`` adds one ``(mean dx, mean dy)`` pair per iteration.  ``align``
    returns two shift arrays, so the reference's ``z`` branch is never taken and ``z`` stays as it is.  ``display`` is
    ignored."""
    locs = deepcopy(locs)
    max_iterations = 5
    convergence = 0.001  # (camera pixels), around 0.1 nm
    shift_x = []
    shift_y = []
    for iteration in range(max_iterations):
        completed = True
        shift = align(locs, infos, display=False, apply_shifts=False, return_shifts=True)[1]
        temp_shift_x = []
        temp_shift_y = []
        for i, locs_ in enumerate(locs):
            if np.absolute(shift[0][i]) + np.absolute(shift[1][i]) > convergence:
                completed = False
            locs_["x"] -= shift[0][i]
            locs_["y"] -= shift[1][i]
            temp_shift_x.append(shift[0][i])
            temp_shift_y.append(shift[1][i])
        shift_x.append(np.mean(temp_shift_x))
        shift_y.append(np.mean(temp_shift_y))
        if completed:
            break
    if return_shifts:
        shifts = list(zip(shift_x, shift_y))
        return locs, shifts
    else:
        return locs


# ---- pick similar (postprocess.py:476-736, :820-957) -------------------------------------------------------------
# Not rebound by localize.install(), like the picks it is built on.
SIMILAR_NAMES = ("pick_similar",)


def _sequential_mean(values: np.ndarray) -> np.float64:
    """numba's ``np.mean`` of a 1-D float array: ``c = dtype(0); for v in a: c += v`` in the array's own type (one
    sequential chain, which np.add.accumulate walks too), then a float64 division; an empty array divides by zero."""
    if values.size == 0:
        raise ZeroDivisionError("division by zero")
    total = np.add.accumulate(np.concatenate([np.zeros(1, values.dtype), values]))[-1]
    return np.float64(total) / np.float64(values.size)


def _rmsd_at_com(xs: np.ndarray, ys: np.ndarray) -> np.float64:
    """``rmsd_at_com`` (postprocess.py:947-957) as numba types it: float64 deviations from the two means, plain
    products, the sequential mean of their sum, a correctly rounded square root."""
    ex, ey = xs.astype(np.float64) - _sequential_mean(xs), ys.astype(np.float64) - _sequential_mean(ys)
    return np.sqrt(_sequential_mean(ex * ex + ey * ey))


def pick_similar(locs: pd.DataFrame, info: list[dict], picks: list[tuple], d: float, std_range: float = 2.0,
                 index_blocks: tuple = None) -> list[tuple]:
    """Circular picks that resemble the given ones (postprocess.py:476-594): a hexagonal grid of circles of diameter
    ``d`` over the field of view, each shifted to the centre of mass of its members until it rests, kept when its
    member count and RMSD lie within ``std_range`` standard deviations of the given picks' and no pick kept so far,
    the given ones included, lies within ``d`` -> the given picks, then the found ones in grid order, as (x, y) pairs
    equal to the reference's in every bit.  The grid search is one device call (one lane per grid point), the greedy
    pass runs on the host.  A given pick without members raises ZeroDivisionError as numba's mean does; picks whose x or
    y values are all integers raise TypeError (numba cannot retype the integer array the found picks are appended to
    and refuses to compile); a non-None ``index_blocks`` is refused."""
    _refuse_index_blocks(index_blocks)
    r = d / 2
    d2 = d**2
    # n_locs and rmsd of the given picks
    sane, offsets, rows, table = _circle_members(locs, info, picks, r, with_table=True)
    x, y = sane["x"].to_numpy(), sane["y"].to_numpy()
    stacked = np.result_type(x.dtype, y.dtype)          # the reference stacks x and y into one array
    n_locs, rmsd = [], []
    for a, b in zip(offsets[:-1], offsets[1:]):
        n_locs.append(int(b - a))
        rmsd.append(_rmsd_at_com(x[rows[a:b]].astype(stacked), y[rows[a:b]].astype(stacked)))
    mean_n_locs = np.mean(n_locs)
    mean_rmsd = np.mean(rmsd)
    std_n_locs = np.std(n_locs)
    std_rmsd = np.std(rmsd)
    min_n_locs = max(2, mean_n_locs - std_range * std_n_locs)
    max_n_locs = mean_n_locs + std_range * std_n_locs
    min_rmsd = mean_rmsd - std_range * std_rmsd
    max_rmsd = mean_rmsd + std_range * std_rmsd
    x_similar = np.array([_[0] for _ in picks])
    y_similar = np.array([_[1] for _ in picks])
    if x_similar.dtype.kind != "f" or y_similar.dtype.kind != "f":
        raise TypeError("the x (or y) values of the picks are all integers: the reference appends floats to that "
                        "integer array inside a jitted loop, which numba refuses to type; pass floats")
    # the grid, as the reference builds it
    x_range = np.arange(d / 2, info[0]["Width"], np.sqrt(3) * d / 2)
    y_range_base = np.arange(d / 2, info[0]["Height"] - d / 2, d)
    y_range_shift = y_range_base + d / 2
    x_r = np.uint64(x_range / r)
    y_r1 = np.uint64(y_range_shift / r)
    y_r2 = np.uint64(y_range_base / r)
    cx, cy, n, spread = backend.similar_shift(table, x, y, x_range, y_range_base, y_range_shift, x_r, y_r2, y_r1,
                                              float(np.float64(r) * np.float64(r)), float(min_n_locs))
    # a candidate that fails a range is never appended and never influences another: the ranges first, then the
    # greedy pass in grid order over the rest
    with np.errstate(invalid="ignore"):
        candidates = np.flatnonzero((n >= min_n_locs) & (n <= max_n_locs) & (spread >= min_rmsd) & (spread <= max_rmsd))
    keep = backend.similar_filter(cx[candidates], cy[candidates], x_similar, y_similar, d2, d)
    x_similar = np.concatenate([x_similar.astype(np.float64), cx[candidates][keep]])
    y_similar = np.concatenate([y_similar.astype(np.float64), cy[candidates][keep]])
    return list(zip(x_similar, y_similar))


# ---- pick kinetics (postprocess.py:1634-1917) on top of csrc/cumexp.hip ---------------------------------------------
# Not rebound by localize.install(), like the picks they are built on.
KINETIC_PICK_NAMES = ("evaluate_picks", "_pick_kinetics_single", "pick_kinetics", "pick_properties")
_LINK_ALL = 999999                  # the reference's r_max inside a pick: every localization of the pick may link


def _pick_columns(picked_locs: list[pd.DataFrame]) -> list:
    """The columns all picks share.  The reference decides per pick whether it links; here the picks are one table."""
    columns = list(picked_locs[0].columns)
    if any(list(locs.columns) != columns for locs in picked_locs):
        raise ValueError("all picks must have the same columns")
    return columns


def _link_picks(picks: list[pd.DataFrame], ids: np.ndarray, info, max_dark_time):
    """``link(pick, info, r_max=999999, max_dark_time=max_dark_time)`` of every non-empty pick in one device pass ->
    (binding events, pick-major and in the reference's order inside a pick; the pick of every event).

    Each pick is sorted by frame with the reference's own pandas call.  The picks then become one table sorted by frame:
    pick k's frames are moved by k strides, a stride being wider than the span of all frames plus the dark time, so no
    window of the link reaches another pick, the link groups come out numbered pick by pick, and the ``group`` column
    (zeros without one) keeps separating rows inside a pick, as it does in the reference.  The combination reads the
    frames as they are.  One reference quirk needs the end of a table: a row that shares the pick's last frame with a
    later row scans the LAST row of the table (csrc/link.hip).  Picks whose last frame holds several localizations are
    therefore linked in a call of their own."""
    ordered = [locs.sort_values(kind="quicksort", by="frame") for locs in picks]
    frames = [locs["frame"].to_numpy() for locs in ordered]
    alone = np.array([len(f) > 1 and f[-2] == f[-1] for f in frames], bool)
    tables, table_ids = [], []
    batch = [k for k in range(len(picks)) if not alone[k]]
    if batch:
        cat = pd.concat([ordered[k] for k in batch])
        sizes = np.array([len(frames[k]) for k in batch])
        rank = np.repeat(np.arange(len(batch), dtype=np.int64), sizes)
        frame = _frame_numbers(cat["frame"].to_numpy(), "frame")
        step = math.floor(max_dark_time + 1)
        stride = int(frame.max()) - int(frame.min()) + max(int(step), 0) + 2
        if stride * len(batch) >= backend.KINETICS_FRAME_LIMIT:
            raise ValueError("the frames of the picks span too much to be linked in one pass")
        moved = frame - int(frame.min()) + rank * stride
        group = cat["group"].to_numpy() if "group" in cat.columns else np.zeros(len(cat), dtype=np.int32)
        d_link_group, n_groups = _device_link_groups(moved, cat["x"].to_numpy(), cat["y"].to_numpy(), _LINK_ALL,
                                                     max_dark_time, group)
        pick_of_group = np.zeros(max(n_groups, 1), np.int64)
        pick_of_group[d_link_group.cpu().numpy()] = np.asarray(ids)[batch][rank]
        linked = _combine(cat, info, d_link_group, n_groups, True)
        tables.append(linked), table_ids.append(pick_of_group[linked.index.to_numpy()])
    for k in np.flatnonzero(alone):
        linked = link(picks[k], info, r_max=_LINK_ALL, max_dark_time=max_dark_time)
        tables.append(linked), table_ids.append(np.full(len(linked), ids[k], np.int64))
    events, event_ids = pd.concat(tables, ignore_index=True), np.concatenate(table_ids)
    order = np.argsort(event_ids, kind="stable")
    return events.iloc[order].reset_index(drop=True), event_ids[order]


def _pick_events(picked_locs: list[pd.DataFrame], info, max_dark_time):
    """What the reference's loop has after ``compute_dark_times`` for every pick, as one pick-major table -> (events,
    the pick of every event, events per pick before the dark-time filter)."""
    n_picks = len(picked_locs)
    sizes = np.array([len(locs) for locs in picked_locs], np.int64)
    filled = np.flatnonzero(sizes)
    columns = _pick_columns(picked_locs)
    picks = [picked_locs[k] for k in filled]
    if not picks:
        return None, np.zeros(0, np.int64), np.zeros(n_picks, np.int64)
    if "len" not in columns:
        events, ids = _link_picks(picks, filled, info, max_dark_time)
    else:
        events, ids = pd.concat(picks, ignore_index=True), np.repeat(filled, sizes[filled])
    linked_sizes = np.bincount(ids, minlength=n_picks)
    if len(events) == 0:
        return events, ids, linked_sizes
    # dark times: one search over all picks, a (pick, group) pair as the label
    frame, lens = events["frame"].to_numpy(), events["len"].to_numpy()
    with np.errstate(over="ignore"):
        last_frame = frame + lens - 1
    labels = ids
    if "group" in events.columns:
        group = _group_labels(events["group"].to_numpy())
        span = int(group.max()) - int(group.min()) + 1
        if span * n_picks >= 2 ** 62:
            raise ValueError("the group labels span too much to be paired with the picks")
        labels = ids * span + (group - int(group.min()))
    f = _frame_numbers(frame, "frame")
    dark = backend.DarkTable(f, labels, _frame_numbers(last_frame, "last_frame")).search()
    # the reference keeps a dark time below ITS table's largest frame: the pick's, not that of all picks
    starts = np.flatnonzero(np.r_[True, ids[1:] != ids[:-1]])
    pick_max = np.repeat(np.maximum.reduceat(f, starts), np.diff(np.r_[starts, len(ids)]))
    dark[dark >= pick_max] = -1
    events["dark"] = np.int32(dark)
    keep = (events["dark"] != -1).to_numpy()
    return events[keep].reset_index(drop=True), ids[keep], linked_sizes


def _pick_rates(events: pd.DataFrame, ids: np.ndarray, n_picks: int):
    """The two ``kinetic_rates`` calls over all picks, and the reference's in-place sort: ``fit_cum_exp`` sorts the array
    it is handed, ``Series.to_numpy()`` hands it a view of the table (pandas 2.3.3 without copy-on-write, recorded in
    tests/golden/pickkin_cases.npz as ``sort_quirk``), so the ``len`` and the ``dark`` column of a pick whose rate is
    fitted each come out ascending on their own.  -> (counts per pick, rates of len, rates of dark)."""
    counts = np.bincount(ids, minlength=n_picks)
    offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    out = []
    for name in ("len", "dark"):
        values = events[name].to_numpy()
        rates = backend.kinetic_rates(values, offsets)
        if (rates.status == backend.CUMEXP_REFUSED).any():
            raise ValueError(f"column {name!r}: the samples of a fit must be finite and must not be negative")
        fitted = ~np.isnan(rates.a)
        if fitted.any():
            ascending = values[np.lexsort((values, ids))]
            events[name] = np.where(fitted[ids], ascending, values)
        out.append(rates)
    return counts, out[0], out[1]


def _progress(callback, n: int) -> None:
    """The reference's calls: ``i`` before every pick, then the count.  ``"console"`` is accepted and shows nothing."""
    if callable(callback):
        for i in range(n):
            callback(i)
        callback(n)


def evaluate_picks(picked_locs: list[pd.DataFrame], info: list[dict], *, max_dark_time: int = 3,
                   progress_callback: Callable[[int], None] | Literal["console"] | None = None):
    """Pick statistics (postprocess.py:1634-1746) -> (N, n_events, rmsd, rmsd_z, length, dark, new_locs), all picks in
    one device pass: one link, one dark-time search, two ``backend.kinetic_rates`` calls, and the pandas float32 means of
    the RMSD by the group statistics kernel (csrc/segment_stats.h's sums), in the reference's bits.  The reference leaves
    the entries of empty picks uninitialised (``np.empty``); here they are NaN, as is all of ``rmsd_z`` without a ``z``
    column.  A fit that ends on its iteration cap raises RuntimeError, where scipy's would.  ``progress_callback`` is
    called as the reference calls it; ``"console"`` is accepted and ignored."""
    pixelsize = lib.get_from_metadata(info, "Pixelsize", default=1.0)
    n_picks = len(picked_locs)
    N, n_events, rmsd, rmsd_z, length, dark = (np.full(n_picks, np.nan) for _ in range(6))
    sizes = np.array([len(locs) for locs in picked_locs], np.int64)
    filled = np.flatnonzero(sizes)
    has_z = "z" in picked_locs[0].columns
    _progress(progress_callback, n_picks)
    N[filled] = sizes[filled]
    if len(filled):
        ids = np.repeat(filled, sizes[filled])
        groups = backend.CenterGroups(ids)

        def spread(names):
            cols = [np.concatenate([picked_locs[k][c].to_numpy() for k in filled]) for c in names]
            means = backend.group_mean_std(groups, cols)
            rows = np.repeat(np.arange(len(filled)), sizes[filled])
            with np.errstate(all="ignore"):
                total = sum((col - mean.astype(col.dtype)[rows]) ** 2 for col, (mean, _) in zip(cols, means))
                (mean_sq, _), = backend.group_mean_std(groups, [total])
                return np.sqrt(mean_sq.astype(total.dtype))

        rmsd[filled] = spread(("x", "y")) * pixelsize
        if has_z:
            rmsd_z[filled] = spread(("z",))
    events, ids, linked_sizes = _pick_events(picked_locs, info, max_dark_time)
    if (linked_sizes[filled] == 0).any():
        raise ValueError("zero-size array to reduction operation maximum which has no identity")   # frame.max() of no event
    if events is None:
        raise ValueError("No objects to concatenate")
    counts, len_rates, dark_rates = _pick_rates(events, ids, n_picks)
    if ((len_rates.status | dark_rates.status)[filled] == backend.CUMEXP_ITER_CAP).any():
        raise RuntimeError("Optimal parameters not found: a fit reached its iteration cap")
    n_events[filled], length[filled], dark[filled] = counts[filled], len_rates.t[filled], dark_rates.t[filled]
    return N, n_events, rmsd, rmsd_z, length, dark, events


def _kept_picks(picked_locs: list[pd.DataFrame], info, max_dark_time):
    """-> (the picks ``pick_kinetics`` keeps, their lengths, darks, event counts, their events), or None for none."""
    n_picks = len(picked_locs)
    events, ids, _ = _pick_events(picked_locs, info, max_dark_time)
    if events is None or len(events) == 0:
        return None
    counts, len_rates, dark_rates = _pick_rates(events, ids, n_picks)
    # the reference drops a pick whose curve_fit raises RuntimeError: here, one whose fit did not converge
    kept = (counts > 0) & (len_rates.status == backend.CUMEXP_CONVERGED) & (dark_rates.status == backend.CUMEXP_CONVERGED)
    if not kept.any():
        return None
    out_locs = events[kept[ids]].reset_index(drop=True)
    return np.flatnonzero(kept), len_rates.t[kept], dark_rates.t[kept], counts[kept], out_locs


def _pick_kinetics_single(pick_locs: pd.DataFrame, info: list[dict], max_dark_time: int):
    """Kinetics of one picked region (postprocess.py:1749-1775) -> (events, length, dark), or None when the region has no
    usable data or a fit does not converge."""
    if not len(pick_locs):
        return None
    kept = _kept_picks([pick_locs], info, max_dark_time)
    if kept is None:
        return None
    return kept[4], kept[1][0], kept[2][0]


def pick_kinetics(picked_locs: list[pd.DataFrame], info: list[dict], *, max_dark_time: int = 3,
                  progress_callback: Callable[[int], None] | Literal["console"] | None = None):
    """Kinetics per picked region (postprocess.py:1778-1852) -> (length, dark, no_locs, out_locs), all picks in one
    device pass (``_link_picks``, one dark-time search, two ``backend.kinetic_rates`` calls).  Picks without a binding
    event that has a dark time are dropped, as in the reference, and so is a pick whose fit does not converge (the
    reference drops it on scipy's RuntimeError).  ``out_locs`` has the reference's rows, columns and order, its in-place
    sort of fitted ``len`` / ``dark`` columns included (``_pick_rates``).  Unlike the reference this does not write a
    ``dark`` column into picks that came with ``len``.  ``progress_callback`` is called as the reference calls it;
    ``"console"`` is accepted and ignored."""
    _progress(progress_callback, len(picked_locs))
    kept = _kept_picks(picked_locs, info, max_dark_time)
    if kept is None:
        raise ValueError("No objects to concatenate")
    _, length, dark, no_locs, out_locs = kept
    return length, dark, no_locs, out_locs


def pick_properties(picked_locs: list[pd.DataFrame], info: list[dict], *, max_dark_time: int = 3,
                    influx_rate: float = 0.03, pick_areas=None,
                    kinetics_progress: Callable[[int], None] | Literal["console"] | None = None,
                    groupprops_progress: Callable[[int], None] | Literal["console"] | None = None) -> pd.DataFrame:
    """Pick properties (postprocess.py:1855-1917): ``pick_kinetics``, then ``groupprops`` of its events, then
    ``n_units = 1 / (influx_rate * dark)``, ``locs``, ``length_cdf``, ``dark_cdf``, ``qpaint_idx_cdf = dark ** -1`` and the
    optional ``pick_area_um2``."""
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", category=RuntimeWarning)
        length, dark, no_locs, out_locs = pick_kinetics(picked_locs=picked_locs, info=info, max_dark_time=max_dark_time,
                                                        progress_callback=kinetics_progress)
        pick_props = groupprops(out_locs, callback=groupprops_progress)
        if pick_areas is not None:
            pick_props["pick_area_um2"] = pick_areas
    with np.errstate(all="ignore"):
        pick_props["n_units"] = 1 / (influx_rate * dark)
        pick_props["locs"] = no_locs
        pick_props["length_cdf"] = length
        pick_props["dark_cdf"] = dark
        pick_props["qpaint_idx_cdf"] = dark**-1
    return pick_props
