"""AIM undrift (Adaptive Intersection Maximization, Ma et al. 2024): picasso/aim.py:776-950 aim,
:517-659 intersection_max, :662-773 intersection_max_z, with the intersection counts on the GPU.

What runs where:
  - device (csrc/aim.hip): the segment partition of the rows, the reference key table of each round and,
    per segment, the box x box (x / y) or box (z) intersection counts ``roi_cc``, in the key arithmetic of
    the reference's column dtypes (float32 in the first x / y round, float64 after);
  - host: the sequential drift update.  Each segment reads back its ``roi_cc`` (box^2 int32), the peak is
    the same ``numpy.fft`` phase estimate the reference takes of it, and only the new relative drift goes
    back in.  The cubic spline over the segment centres and the correction of the columns are the
    reference's own numpy / scipy operations on the same dtypes, so drift and coordinates agree bit for bit
    once the counts do.

There is no CPU fallback: without a device every call raises ``HipBackendError``.
"""
from __future__ import annotations

from typing import Literal

import numpy as np
import pandas as pd

from . import __version__, _lib, backend, lib

# tests: a list here receives (round, segment, roi_cc, peak) of every segment counted, round in
# {"xy1", "xy2", "z1", "z2"}
_trace = None
# the columns an aim() call uploaded, by id() of the host object (so the z rounds reuse the x / y ones)
_resident = None


class _MockProgress:
    """No progress display (the reference's lib.MockProgress)."""

    def get_iterator(self, start=0, end=100):
        return range(start, end)

    def set_value(self, *args, **kwargs):
        pass

    def zero_progress(self, *args, **kwargs):
        pass

    def close(self, *args, **kwargs):
        pass


class _ConsoleProgress(_MockProgress):
    """progress="console": a tqdm bar per round (the reference's lib.TqdmProgress)."""

    def __init__(self, description=""):
        self.description = description
        self.bar = None

    def get_iterator(self, start=0, end=100, unit="segment"):
        from tqdm import tqdm
        self.bar = tqdm(range(start, end), desc=self.description, unit=unit)
        return self.bar

    def set_value(self, value, *args, **kwargs):
        if self.bar is not None:
            self.bar.update(value - self.bar.n)

    def zero_progress(self, description, *args, **kwargs):
        self.description = description


def _progress_dialog_types():
    """The reference's lib.ProgressDialog (a Qt dialog) when the reference and Qt import."""
    try:
        from picasso import lib as ref_lib
        return (ref_lib.ProgressDialog,)
    except Exception:
        return ()


def _is_dialog(progress) -> bool:
    types = _progress_dialog_types()
    return bool(types) and isinstance(progress, types)


def _get_fft_peak(roi_cc, roi_size):
    """Sub-pixel peak of a box x box count array from the phase of the first Fourier coefficients
    along x and y (picasso/aim.py:444-477), in units of intersect_d."""
    f = np.fft.fft2(roi_cc.T)
    peaks = []
    for coeff, n in ((f[0, 1], roi_cc.shape[0]), (f[1, 0], roi_cc.shape[1])):
        ang = np.angle(coeff)
        ang = ang - 2 * np.pi * (ang > 0)
        p = np.abs(ang) / (2 * np.pi / n) - (n - 1) / 2
        p *= roi_size / n
        peaks.append(p)
    return peaks[0], peaks[1]


def _get_fft_peak_z(roi_cc, roi_size):
    """The same along z for a 1-D count array (picasso/aim.py:490-514)."""
    f = np.fft.fft(roi_cc)
    ang = np.angle(f[1])
    ang = ang - 2 * np.pi * (ang > 0)
    p = np.abs(ang) / (2 * np.pi / roi_cc.size) - (roi_cc.size - 1) / 2
    p *= roi_size / roi_cc.size
    return p


def _device():
    import torch
    return torch.device("cuda", torch.cuda.current_device())


def _upload(values, dtype):
    """A resident copy of a host column (reused within one aim() call)."""
    import torch
    key = (id(values), np.dtype(dtype).str)
    if _resident is not None and key in _resident:
        return _resident[key][1]
    a = np.ascontiguousarray(np.asarray(values), dtype)
    t = torch.from_numpy(a).to(_device())
    if _resident is not None:
        _resident[key] = (values, t)
    return t


def _segments(frame, seg_bounds):
    """(rows grouped by segment as an int32 device tensor, host offsets) for seg_bounds."""
    import torch
    seg_bounds = np.asarray(seg_bounds)
    n_seg = len(seg_bounds) - 1
    key = ("segments", id(frame), seg_bounds.tobytes())
    if _resident is not None and key in _resident:
        return _resident[key][1]
    f = np.asarray(frame).astype(np.int64)
    n_frames = int(seg_bounds[-1]) if n_seg >= 0 else 0
    step = int(seg_bounds[1] - seg_bounds[0]) if n_seg >= 1 else 1
    uniform = (n_seg >= 1 and seg_bounds[0] == 0 and step > 0
               and np.array_equal(seg_bounds, np.concatenate((np.arange(0, n_frames, step), [n_frames]))))
    if uniform:
        rows, offsets = backend.aim_partition(_upload(f, np.int64), step, n_frames)
    else:
        # any other bounds: segment s holds seg_bounds[s] < frame <= seg_bounds[s + 1]
        seg = np.searchsorted(seg_bounds, f, side="left") - 1
        ok = (f > seg_bounds[0]) & (f <= seg_bounds[-1]) if n_seg >= 1 else np.zeros(len(f), bool)
        idx = np.flatnonzero(ok)
        order = idx[np.argsort(seg[idx], kind="stable")]
        offsets = np.concatenate(([0], np.cumsum(np.bincount(seg[idx], minlength=max(n_seg, 0))))).astype(np.int64)
        rows = torch.from_numpy(np.ascontiguousarray(order, np.int32)).to(_device())
    if _resident is not None:
        _resident[key] = (frame, (rows, offsets))
    return rows, offsets


def _round_tag(kind, aim_round):
    return f"{kind}{aim_round}"


def _record(tag, s, roi_cc, peak):
    if _trace is not None:
        _trace.append((tag, int(s), np.array(roi_cc), peak))


def _spline(seg_bounds, drift):
    from scipy.interpolate import InterpolatedUnivariateSpline
    t = (seg_bounds[1:] + seg_bounds[:-1]) / 2
    pol = InterpolatedUnivariateSpline(t, drift, k=3)
    return pol(np.arange(seg_bounds[-1]) + 1)


def intersection_max(x, y, ref_x, ref_y, frame, seg_bounds, intersect_d: float, roi_r: float, width: int,
                     aim_round: int = 1, progress=None):
    """Undrift x / y by intersection maximization against ref_x / ref_y (picasso/aim.py:517-659).
    -> x_pdc, y_pdc, drift_x, drift_y per frame."""
    assert aim_round in [1, 2], "aim_round must be 1 or 2."
    if progress is None:
        progress = _MockProgress()
    _lib.require_gpu()
    seg_bounds = np.asarray(seg_bounds)
    n_segments = len(seg_bounds) - 1
    drift_x = np.zeros(n_segments)
    drift_y = np.zeros(n_segments)
    rel_x = 0
    rel_y = 0

    # the box x box search region: shifts of steps_x + steps_y * W cells, truncated to int32 (x-major)
    roi_units = int(np.ceil(roi_r / intersect_d))
    steps = np.arange(-roi_units, roi_units + 1, 1)
    box = len(steps)
    width_units = width / intersect_d
    shifts = np.zeros((box, box), dtype=np.int32)
    for i, sx in enumerate(steps):
        for j, sy in enumerate(steps):
            shifts[i, j] = sx + sy * width_units

    single = np.dtype(getattr(x, "dtype", np.float64)) == np.float32 and \
        np.dtype(getattr(y, "dtype", np.float64)) == np.float32
    mode, col_t = (backend.AIM_XY_F32, np.float32) if single else (backend.AIM_XY_F64, np.float64)
    dx, dy = _upload(x, col_t), _upload(y, col_t)
    if ref_x is x and ref_y is y:
        table = backend.AimTable(mode, dx, dy, None, None, dx.numel(), intersect_d, width_units, 0.0, shifts.ravel())
    else:
        rx, ry = _upload(ref_x, col_t), _upload(ref_y, col_t)
        table = backend.AimTable(mode, rx, ry, None, None, rx.numel(), intersect_d, width_units, 0.0, shifts.ravel())
        table.x, table.y = dx, dy
    rows, offsets = _segments(frame, seg_bounds)
    tag = _round_tag("xy", aim_round)
    try:
        for s in progress.get_iterator(1 if aim_round == 1 else 0, n_segments):
            lo, hi = int(offsets[s]), int(offsets[s + 1])
            if hi == lo:                      # an empty segment keeps the previous drift (drift[-1] at s = 0)
                drift_x[s] = drift_x[s - 1]
                drift_y[s] = drift_y[s - 1]
                continue
            roi_cc = table.count(rows[lo:hi], rel_x, rel_y).reshape(box, box)
            px, py = _get_fft_peak(roi_cc, 2 * roi_r)
            _record(tag, s, roi_cc, (px, py))
            rel_x += px
            rel_y += py
            drift_x[s] = -rel_x
            drift_y[s] = -rel_y
            progress.set_value(s)
    finally:
        table.close()

    drift_x = _spline(seg_bounds, drift_x)
    drift_y = _spline(seg_bounds, drift_y)
    x_pdc = x - drift_x[frame - 1]
    y_pdc = y - drift_y[frame - 1]
    return x_pdc, y_pdc, drift_x, drift_y


def intersection_max_z(x, y, z, ref_x, ref_y, ref_z, frame, seg_bounds, intersect_d: float, roi_r: float,
                       width: int, height: int, pixelsize: float, aim_round: int = 1, progress=None):
    """Undrift z (nm) of x / y-undrifted localizations (picasso/aim.py:662-773): keys x + y W + z W H,
    shifts along z only.  -> z_pdc, drift_z per frame (nm)."""
    if progress is None:
        progress = _MockProgress()
    _lib.require_gpu()
    z = z.copy() / pixelsize
    ref_z = ref_z.copy() / pixelsize
    seg_bounds = np.asarray(seg_bounds)
    n_segments = len(seg_bounds) - 1
    drift_z = np.zeros(n_segments)
    rel_z = 0

    roi_units = int(np.ceil(roi_r / intersect_d))
    steps = np.arange(-roi_units, roi_units + 1, 1)
    width_units = width / intersect_d
    height_units = height / intersect_d
    shifts = steps.astype(np.int32) * width_units * height_units         # float64: keys are matched in float64

    single = np.dtype(getattr(z, "dtype", np.float64)) == np.float32
    mode, z_t = (backend.AIM_Z_F32, np.float32) if single else (backend.AIM_Z_F64, np.float64)
    dx, dy, dz = _upload(x, np.float64), _upload(y, np.float64), _upload(z, z_t)
    rx, ry, rz = _upload(ref_x, np.float64), _upload(ref_y, np.float64), _upload(ref_z, z_t)
    table = backend.AimTable(mode, rx, ry, rz, None, rx.numel(), intersect_d, width_units, height_units, shifts)
    table.x, table.y, table.z = dx, dy, dz
    rows, offsets = _segments(frame, seg_bounds)
    tag = _round_tag("z", aim_round)
    try:
        for s in progress.get_iterator(1 if aim_round == 1 else 0, n_segments):
            lo, hi = int(offsets[s]), int(offsets[s + 1])
            if hi == lo:
                drift_z[s] = drift_z[s - 1]
                continue
            roi_cc = table.count(rows[lo:hi], 0.0, 0.0, rel_z)
            pz = _get_fft_peak_z(roi_cc, 2 * roi_r)
            _record(tag, s, roi_cc, (pz,))
            rel_z += pz
            drift_z[s] = -rel_z
            progress.set_value(s)
    finally:
        table.close()

    drift_z = _spline(seg_bounds, drift_z)
    z_pdc = z - drift_z[frame - 1]
    z_pdc *= pixelsize
    drift_z *= pixelsize
    return z_pdc, drift_z


def aim(locs: pd.DataFrame, info: list[dict], segmentation: int = 100, intersect_d: float = 20 / 130,
        roi_r: float = 60 / 130, progress=None) -> tuple[pd.DataFrame, list[dict], pd.DataFrame]:
    """AIM undrift of a localization table (picasso/aim.py:776-950): two x / y rounds (first segment, then the
    whole corrected table as reference), and two z rounds when the table has z.
    -> undrifted locs (x / y / z float64), info + the AIM entry, float32 drift per frame."""
    assert progress is None or (isinstance(progress, str) and progress == "console") or _is_dialog(progress), \
        "progress must be None, 'console', or a ProgressDialog instance."
    if progress is None:
        progress = _MockProgress()
    elif isinstance(progress, str):
        progress = _ConsoleProgress(description="Undrifting by AIM (1/2)")

    locs = locs.copy()
    width = lib.get_from_metadata(info, "Width", raise_error=True)
    height = lib.get_from_metadata(info, "Height", raise_error=True)
    pixelsize = lib.get_from_metadata(info, "Pixelsize", raise_error=True)
    n_frames = lib.get_from_metadata(info, "Frames", raise_error=True)

    global _resident
    _resident = {}
    try:
        frame = locs["frame"] + 1 - locs["frame"].min()
        seg_bounds = np.concatenate((np.arange(0, n_frames, segmentation), [n_frames]))
        first = frame <= segmentation
        x_pdc, y_pdc, drift_x1, drift_y1 = intersection_max(
            locs["x"], locs["y"], locs["x"][first], locs["y"][first], frame, seg_bounds, intersect_d, roi_r, width,
            aim_round=1, progress=progress)
        progress.zero_progress(description="Undrifting by AIM (2/2)")
        x_pdc, y_pdc, drift_x2, drift_y2 = intersection_max(
            x_pdc, y_pdc, x_pdc, y_pdc, frame, seg_bounds, intersect_d, roi_r, width, aim_round=2, progress=progress)
        drift_x = drift_x1 + drift_x2
        drift_y = drift_y1 + drift_y2
        shift_x = np.mean(drift_x)
        shift_y = np.mean(drift_y)
        drift_x -= shift_x
        drift_y -= shift_y
        x_pdc += shift_x
        y_pdc += shift_y

        if "z" in locs.columns:
            progress.zero_progress(description="Undrifting z (1/2)")
            z_pdc, drift_z1 = intersection_max_z(
                x_pdc, y_pdc, locs["z"], x_pdc[first], y_pdc[first], locs["z"][first], frame, seg_bounds,
                intersect_d, roi_r, width, height, pixelsize, aim_round=1, progress=progress)
            progress.zero_progress(description="Undrifting z (2/2)")
            z_pdc, drift_z2 = intersection_max_z(
                x_pdc, y_pdc, z_pdc, x_pdc, y_pdc, z_pdc, frame, seg_bounds, intersect_d, roi_r, width, height,
                pixelsize, aim_round=2, progress=progress)
            drift_z = drift_z1 + drift_z2
            shift_z = np.mean(drift_z)
            drift_z -= shift_z
            z_pdc += shift_z
            drift = pd.DataFrame({"x": drift_x, "y": drift_y, "z": drift_z}, dtype="float32")
        else:
            drift = pd.DataFrame({"x": drift_x, "y": drift_y}, dtype="float32")
    finally:
        _resident = None

    locs["x"] = x_pdc
    locs["y"] = y_pdc
    if "z" in locs.columns:
        locs["z"] = z_pdc
    new_info = info + [{
        "Generated by": f"Picasso v{__version__} AIM",
        "Intersect distance (nm)": intersect_d * pixelsize,
        "Segmentation": segmentation,
        "Search regions radius (nm)": roi_r * pixelsize,
    }]
    progress.close()
    return locs, new_info, drift
