"""picasso.render surface for the render modes on the drift-correction / display path:
``blur_method=None`` (2-D histogram), ``"gaussian"`` (one separable Gaussian per localization,
widths = localization precisions) and ``"gaussian_iso"`` (one width, their mean).  picasso/render.py:37-175 ``render``,
:798-853 ``_render_hist``, :1020-1070 ``_render_gaussian``; the pixels are computed by
csrc/render.hip.  The two blurred histograms, ``_render_smooth`` (:1349-1410) and ``_render_convolve`` (:1249-1319)
with ``_fftconvolve`` (:1413-1460) under them, are computed by csrc/blur.hip and called by name: ``render()`` still
refuses ``blur_method="smooth"`` / ``"convolve"``.

Rotated views (``ang``: a scipy ``Rotation`` or the legacy Euler tuple).  ``_render_hist``,
``_render_gaussian`` and ``_render_gaussian_iso`` (and their older public names) draw them on the device
(csrc/render_rot.hip), in the reference's bits; ``rotation_matrix``, ``to_rotation``, ``closest_rotvec`` and
``locs_rotation`` (picasso/render.py:1463-1637) are here as well, the last one rotating on the device.  The 3x3 matrix
is always scipy's own (``to_rotation(ang).as_matrix()``): the Euler tuple goes through ``Rotation.from_matrix``, which
re-orthogonalises, so the device never rebuilds it from angles.  The widths are taken as float32 columns, as in the flat
view.  The one follow-up, pinned by tests that predate the kernels: ``render(..., ang=...)`` and ``_render_smooth`` /
``_render_convolve`` (and their older names) with ``ang`` still raise ``NotImplementedError``, and
``localize.install()`` still hands rotated ``_render_gaussian`` / ``_render_hist`` calls to the reference's functions.
``backend.render_rot_arrays`` already returns the in-view mask a rotated ``_render_convolve`` needs for its medians.

Zero blur width.  The reference draws each localization in ``_draw_gaussian_loc``, compiled by numba
with Python's error model, so ``1.0 / (2.0 * sx_ * sx_)`` raises ``ZeroDivisionError`` when a
localization that is drawn has a width of exactly 0.  The two layers split that as follows:

* this module (``render``, ``_render_gaussian``, ``_render_gaussian_iso`` and the three older names)
  raises ``ZeroDivisionError`` like the reference.  The widths are evaluated on the host columns as
  the kernel evaluates them: in float32, after ``np.maximum`` with ``min_blur_width``, after the
  multiplication by the oversampling and, for ``gaussian_iso``, after the mean.  Only rows in view
  count, and only rows whose footprint is not empty: a NaN width has an empty footprint, the
  reference returns before the division, nothing raises.
* ``backend.render_arrays`` and the C ABI (``pmi_render_gaussian*``) keep IEEE semantics, like
  ``oracle.render``: a zero width gives a NaN at the one pixel of its footprint and leaves every
  other pixel as it was.
"""
from __future__ import annotations

import numpy as np
import pandas as pd
from scipy.spatial.transform import Rotation

from . import backend, lib

_NOT_BUILT = ("smooth", "convolve")


def _viewport(info, viewport):
    if viewport is None:
        try:
            viewport = [(0, 0), (info[0]["Height"], info[0]["Width"])]
        except TypeError:
            raise ValueError("Need info if no viewport is provided.")
    return viewport


def render(locs: pd.DataFrame, info, oversampling: float = 1.0, viewport=None, blur_method=None,
           min_blur_width: float = 0.0, ang=None, disp_px_size: float | None = None):
    """-> (n, image): number of localizations rendered and the float32 image."""
    pixelsize = lib.get_from_metadata(info, "Pixelsize", raise_error=True)
    if disp_px_size is None:
        lib.deprecation_warning("Deprecation warning: the 'oversampling' parameter is deprecated and will be removed "
                                "in v0.11.0. Use 'disp_px_size' instead.")
        disp_px_size = pixelsize / oversampling
    oversampling = pixelsize / disp_px_size
    (y_min, x_min), (y_max, x_max) = _viewport(info, viewport)
    if ang is not None:
        raise NotImplementedError("rotated rendering (ang) is not routed through render() yet: call _render_hist, "
                                  "_render_gaussian or _render_gaussian_iso with ang (csrc/render_rot.hip)")
    if blur_method is None:
        return _render_hist(locs, oversampling, y_min, x_min, y_max, x_max)
    if blur_method == "gaussian":
        return _render_gaussian(locs, oversampling, y_min, x_min, y_max, x_max, min_blur_width)
    if blur_method == "gaussian_iso":
        return _render_gaussian_iso(locs, oversampling, y_min, x_min, y_max, x_max, min_blur_width)
    if blur_method in _NOT_BUILT:
        raise NotImplementedError(f"blur_method={blur_method!r} is not routed through render(): call "
                                  f"render._render_{blur_method} (csrc/blur.hip); there is no CPU fallback")
    raise Exception("blur_method not understood.")


def _int32(v):
    """float64 -> int32 as the compiled reference does it (cvttsd2si): truncation, INT_MIN for NaN / out of range."""
    ok = (v == v) & (v < 2147483648.0) & (v >= -2147483648.0)
    return np.where(ok, np.trunc(np.where(ok, v, 0.0)), -2147483648.0).astype(np.int64)


def _raise_on_zero_width(x, y, lpx, lpy, oversampling, y_min, x_min, y_max, x_max, min_blur_width, iso):
    """ZeroDivisionError where the reference's ``_draw_gaussian_loc`` divides by a zero width (module docstring)."""
    x = np.asarray(x, np.float32).astype(np.float64)
    y = np.asarray(y, np.float32).astype(np.float64)
    osf, mbw = np.float32(oversampling), np.float32(min_blur_width)
    with np.errstate(all="ignore"):
        sx = osf * np.maximum(np.asarray(lpx, np.float32), mbw)
        sy = osf * np.maximum(np.asarray(lpy, np.float32), mbw)
        if iso:
            sy = (sy + sx) / np.float32(2.0)
            sx = sy
        rows = np.flatnonzero(((sx == 0) | (sy == 0)) & (x > x_min) & (y > y_min) & (x < x_max) & (y < y_max))
        if len(rows) == 0:
            return
        # the division is reached only behind the reference's "nx <= 0 or ny <= 0: return" (render.py:505-524)
        n_y = int(np.ceil(oversampling * (y_max - y_min)))
        n_x = int(np.ceil(oversampling * (x_max - x_min)))
        x_ = oversampling * (x[rows] - x_min)
        y_ = oversampling * (y[rows] - y_min)
        oy = 3.0 * sy[rows].astype(np.float64)
        ox = 3.0 * sx[rows].astype(np.float64)
        cy = np.minimum(_int32(y_ + oy + 1), n_y) - np.maximum(_int32(y_ - oy), 0)
        cx = np.minimum(_int32(x_ + ox) + 1, n_x) - np.maximum(_int32(x_ - ox), 0)
    if np.any((cx > 0) & (cy > 0)):
        raise ZeroDivisionError("division by zero")


def _render_hist(locs, oversampling, y_min, x_min, y_max, x_max, ang=None):
    if ang is not None:
        return _render_rotated(locs, oversampling, y_min, x_min, y_max, x_max, ang)
    return backend.render_arrays(locs["x"].to_numpy(), locs["y"].to_numpy(), oversampling, y_min, x_min, y_max, x_max)


def _render_gaussian(locs, oversampling, y_min, x_min, y_max, x_max, min_blur_width, ang=None):
    if ang is not None:
        return _render_rotated(locs, oversampling, y_min, x_min, y_max, x_max, ang, min_blur_width, iso=False)
    x, y, lpx, lpy = (locs[c].to_numpy() for c in ("x", "y", "lpx", "lpy"))
    _raise_on_zero_width(x, y, lpx, lpy, oversampling, y_min, x_min, y_max, x_max, min_blur_width, False)
    return backend.render_arrays(x, y, oversampling, y_min, x_min, y_max, x_max, lpx=lpx, lpy=lpy,
                                 min_blur_width=min_blur_width)


def _render_gaussian_iso(locs, oversampling, y_min, x_min, y_max, x_max, min_blur_width, ang=None):
    """picasso/render.py:1148-1216: one isotropic width per localization, the mean of the two."""
    if ang is not None:
        return _render_rotated(locs, oversampling, y_min, x_min, y_max, x_max, ang, min_blur_width, iso=True)
    x, y, lpx, lpy = (locs[c].to_numpy() for c in ("x", "y", "lpx", "lpy"))
    _raise_on_zero_width(x, y, lpx, lpy, oversampling, y_min, x_min, y_max, x_max, min_blur_width, True)
    return backend.render_arrays(x, y, oversampling, y_min, x_min, y_max, x_max, lpx=lpx, lpy=lpy,
                                 min_blur_width=min_blur_width, iso=True)


def _refuse_ang(ang) -> None:
    if ang is not None:
        raise NotImplementedError("rotated rendering (ang) of the blurred histograms is not routed to the device yet "
                                  "(module docstring); _render_hist, _render_gaussian and _render_gaussian_iso take ang")


# ---- rotated views (picasso/render.py:1463-1637) -------------------------------------------------------------------------
def rotation_matrix(angx: float, angy: float, angz: float) -> Rotation:
    """The legacy Euler convention: the product of the rotations about x, y and z (radians), in that order, handed to
    ``Rotation.from_matrix`` (which re-orthogonalises it)."""
    cx, sx, cy, sy, cz, sz = np.cos(angx), np.sin(angx), np.cos(angy), np.sin(angy), np.cos(angz), np.sin(angz)
    about_x = np.array([[1.0, 0.0, 0.0], [0.0, cx, sx], [0.0, -sx, cx]])
    about_y = np.array([[cy, 0.0, sy], [0.0, 1.0, 0.0], [-sy, 0.0, cy]])
    about_z = np.array([[cz, -sz, 0.0], [sz, cz, 0.0], [0.0, 0.0, 1.0]])
    return Rotation.from_matrix(about_x @ about_y @ about_z)


def to_rotation(ang: tuple[float, float, float] | Rotation | None) -> Rotation | None:
    """None stays None, a scipy ``Rotation`` is used as it is, a tuple of three angles goes through ``rotation_matrix``."""
    if ang is None or isinstance(ang, Rotation):
        return ang
    return rotation_matrix(*ang)


def closest_rotvec(rotation: Rotation, reference: lib.FloatArray1D) -> lib.FloatArray1D:
    """The rotation vector of ``rotation`` with the number of full turns about its axis that brings it closest to the
    rotation vector ``reference`` (its magnitude may exceed pi).  The identity keeps the reference's axis and whole turns."""
    reference = np.asarray(reference, dtype=float)
    full_turn = 2 * np.pi
    rotvec = rotation.as_rotvec()
    angle = np.linalg.norm(rotvec)
    if angle < 1e-9:
        length = np.linalg.norm(reference)
        if length < 1e-9:
            return np.zeros(3)
        return reference * (full_turn * np.round(length / full_turn) / length)
    axis = rotvec / angle
    turns = np.round((axis @ reference - angle) / full_turn)
    return axis * (angle + full_turn * turns)


def locs_rotation(locs: pd.DataFrame, oversampling: float, x_min: float, x_max: float, y_min: float, y_max: float,
                  ang: tuple[float, float, float] | Rotation) -> tuple[lib.FloatArray1D, lib.FloatArray1D, lib.BoolArray1D, lib.FloatArray1D]:
    """-> (x, y, in_view, z): the rows rotated about the centre of the field of view (csrc/render_rot.hip), those left
    strictly inside it, in display pixels; ``in_view`` marks them in the table.  Note the argument order."""
    x, y, z, in_view = backend.rotate_locs_arrays(locs["x"].to_numpy(), locs["y"].to_numpy(), locs["z"].to_numpy(),
                                                  to_rotation(ang).as_matrix(), oversampling, y_min, x_min, y_max, x_max)
    return x[in_view], y[in_view], in_view, z[in_view]


def _render_rotated(locs, oversampling, y_min, x_min, y_max, x_max, ang, min_blur_width=None, iso=False):
    """The rotated histogram (``min_blur_width`` None) or projected Gaussian in one device call -> (n, image)."""
    widths = {}
    if min_blur_width is not None:
        widths = dict(lpx=locs["lpx"].to_numpy(), lpy=locs["lpy"].to_numpy(),
                      lpz=locs["lpz"].to_numpy() if "lpz" in locs else None, min_blur_width=min_blur_width, iso=iso)
    n, image, _ = backend.render_rot_arrays(locs["x"].to_numpy(), locs["y"].to_numpy(), locs["z"].to_numpy(),
                                            to_rotation(ang).as_matrix(), oversampling, y_min, x_min, y_max, x_max,
                                            with_in_view=False, **widths)
    return n, image


def _fftconvolve(image: lib.FloatArray2D, blur_width: float, blur_height: float) -> lib.FloatArray2D:
    """picasso/render.py:1413-1460 on the device (csrc/blur.hip): scipy's ``gaussian_filter`` in every bit where the
    reference takes it, a float64 direct sum where the reference takes the single-precision FFT."""
    return backend.blur_array(image, blur_width, blur_height)


def _render_smooth(locs: pd.DataFrame, oversampling: float, y_min: float, x_min: float, y_max: float, x_max: float,
                   ang: tuple[float, float, float] | Rotation | None = None) -> tuple[int, lib.FloatArray2D]:
    """picasso/render.py:1349-1410: the histogram blurred by one display pixel; fill and blur in one device call."""
    _refuse_ang(ang)
    return backend.render_blurred_arrays(locs["x"].to_numpy(), locs["y"].to_numpy(), oversampling, y_min, x_min, y_max,
                                         x_max, 1, 1)


def _render_convolve(locs: pd.DataFrame, oversampling: float, y_min: float, x_min: float, y_max: float, x_max: float,
                     min_blur_width: float, ang: tuple[float, float, float] | Rotation | None = None) -> tuple[int, lib.FloatArray2D]:
    """picasso/render.py:1249-1319: the histogram blurred by the median localization precision of the rows in view
    (the host takes the two medians); fill and blur in one device call."""
    _refuse_ang(ang)
    x, y = locs["x"].to_numpy(), locs["y"].to_numpy()
    with np.errstate(invalid="ignore"):          # strict on all four sides, float32 columns compared as float64 (_render_setup)
        xd, yd = np.asarray(x, np.float32).astype(np.float64), np.asarray(y, np.float32).astype(np.float64)
        in_view = (xd > x_min) & (yd > y_min) & (xd < x_max) & (yd < y_max)
    n = int(in_view.sum())
    if n == 0:
        return 0, np.zeros(backend.render_dims(oversampling, y_min, x_min, y_max, x_max), dtype=np.float32)
    blur_width = oversampling * max(
        np.median(locs["lpx"].to_numpy()[in_view]), min_blur_width
    )
    blur_height = oversampling * max(
        np.median(locs["lpy"].to_numpy()[in_view]), min_blur_width
    )
    return backend.render_blurred_arrays(x, y, oversampling, y_min, x_min, y_max, x_max, blur_width, blur_height)


def _older_name(name: str) -> None:
    lib.deprecation_warning(f"Deprecation warning: the '{name}' function is deprecated and will be removed in "
                            f"v0.11.0. Use _{name} instead if necessary.")


def render_hist(locs, oversampling, y_min, x_min, y_max, x_max, ang=None):
    """Older public name of ``_render_hist`` (picasso/render.py:776-795)."""
    _older_name("render_hist")
    return _render_hist(locs, oversampling, y_min, x_min, y_max, x_max, ang=ang)


def render_gaussian(locs, oversampling, y_min, x_min, y_max, x_max, min_blur_width, ang=None):
    """Older public name of ``_render_gaussian`` (picasso/render.py:990-1017) — the call BASELINE.json's
    config 3 is quoted on."""
    _older_name("render_gaussian")
    return _render_gaussian(locs, oversampling, y_min, x_min, y_max, x_max, min_blur_width, ang=ang)


def render_gaussian_iso(locs, oversampling, y_min, x_min, y_max, x_max, min_blur_width, ang=None):
    """Older public name of ``_render_gaussian_iso`` (picasso/render.py:1118-1145)."""
    _older_name("render_gaussian_iso")
    return _render_gaussian_iso(locs, oversampling, y_min, x_min, y_max, x_max, min_blur_width, ang=ang)


def render_convolve(locs: pd.DataFrame, oversampling: float, y_min: float, x_min: float, y_max: float, x_max: float,
                    min_blur_width: float, ang: tuple[float, float, float] | Rotation | None = None) -> tuple[int, lib.FloatArray2D]:
    """Older public name of ``_render_convolve`` (picasso/render.py:1219-1246)."""
    _older_name("render_convolve")
    return _render_convolve(locs, oversampling, y_min, x_min, y_max, x_max, min_blur_width, ang=ang)


def render_smooth(locs: pd.DataFrame, oversampling: float, y_min: float, x_min: float, y_max: float, x_max: float,
                  ang: tuple[float, float, float] | Rotation | None = None) -> tuple[int, lib.FloatArray2D]:
    """Older public name of ``_render_smooth`` (picasso/render.py:1322-1346)."""
    _older_name("render_smooth")
    return _render_smooth(locs, oversampling, y_min, x_min, y_max, x_max, ang=ang)
