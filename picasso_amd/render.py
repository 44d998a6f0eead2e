"""picasso.render surface for the render modes on the drift-correction / display path:
``blur_method=None`` (2-D histogram), ``"gaussian"`` (one separable Gaussian per localization,
widths = localization precisions) and ``"gaussian_iso"`` (one width, their mean).  picasso/render.py:37-175 ``render``,
:798-853 ``_render_hist``, :1020-1070 ``_render_gaussian``; the pixels are computed by
csrc/render.hip.  The two blurred histograms, ``_render_smooth`` (:1349-1410) and ``_render_convolve`` (:1249-1319)
with ``_fftconvolve`` (:1413-1460) under them, are computed by csrc/blur.hip and called by name: ``render()`` still
refuses ``blur_method="smooth"`` / ``"convolve"``.  Rotated views (``ang``) are not built; they
raise instead of falling back to a CPU path.

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
        raise NotImplementedError("rotated rendering (ang) has no HIP kernel in picasso_amd")
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
        raise NotImplementedError("rotated rendering (ang) has no HIP kernel in picasso_amd")
    return backend.render_arrays(locs["x"].to_numpy(), locs["y"].to_numpy(), oversampling, y_min, x_min, y_max, x_max)


def _render_gaussian(locs, oversampling, y_min, x_min, y_max, x_max, min_blur_width, ang=None):
    if ang is not None:
        raise NotImplementedError("rotated rendering (ang) has no HIP kernel in picasso_amd")
    x, y, lpx, lpy = (locs[c].to_numpy() for c in ("x", "y", "lpx", "lpy"))
    _raise_on_zero_width(x, y, lpx, lpy, oversampling, y_min, x_min, y_max, x_max, min_blur_width, False)
    return backend.render_arrays(x, y, oversampling, y_min, x_min, y_max, x_max, lpx=lpx, lpy=lpy,
                                 min_blur_width=min_blur_width)


def _render_gaussian_iso(locs, oversampling, y_min, x_min, y_max, x_max, min_blur_width, ang=None):
    """picasso/render.py:1148-1216: one isotropic width per localization, the mean of the two."""
    if ang is not None:
        raise NotImplementedError("rotated rendering (ang) has no HIP kernel in picasso_amd")
    x, y, lpx, lpy = (locs[c].to_numpy() for c in ("x", "y", "lpx", "lpy"))
    _raise_on_zero_width(x, y, lpx, lpy, oversampling, y_min, x_min, y_max, x_max, min_blur_width, True)
    return backend.render_arrays(x, y, oversampling, y_min, x_min, y_max, x_max, lpx=lpx, lpy=lpy,
                                 min_blur_width=min_blur_width, iso=True)


def _refuse_ang(ang) -> None:
    if ang is not None:
        raise NotImplementedError("rotated rendering (ang) has no HIP kernel in picasso_amd")


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
