"""A NumPy restatement of the rotated views (picasso/render.py:1571-1637 ``locs_rotation``; ``_render_hist``,
``_render_gaussian`` and ``_render_gaussian_iso`` with ``ang``; :578-679 ``_draw_gaussian_rot_loc`` as numba types
it), written for the tests, and the tables the tests and tests/golden/make_goldens_rotrender.py share.

Rotation (float64): the centre of the viewport is subtracted from x and y (in float32 when all three coordinate
columns are float32, as NumPy does on the float32 array the reference takes from the table), then
``r_i = (M[i][0] v0 + M[i][1] v1) + M[i][2] v2`` unfused, which is what scipy's ``Rotation.apply`` evaluates
(scipy 1.15.3 on NumPy 2.2.6: ``einsum('ijk,ik->ij')``) on the array ``locs[["x", "y", "z"]].to_numpy()`` hands it:
pandas (2.3.3) lays that (N, 3) array out column by column (Fortran order) whatever the table was built from.  The same
einsum on a row-major array evaluates ``(M[i][0] v0 + M[i][2] v2) + M[i][1] v1`` instead, and a table of ONE row is
both column- and row-major and takes that second order.  The centre is added back, "in view" is strict on all four sides.

Gaussian, scalar per localization: float32 widths, the float32 projected covariance with
``S[i][j] = fma(P[i][2], R[j][2], fma(P[i][1], R[j][1], P[i][0] R[j][0]))`` (what the float32 3x3 products give through
the OpenBLAS 0.3.29 of NumPy 2.2.6's wheels), a skip on ``float64(det) < 1e-10``, the float32 inverse, the float64 norm,
the +-3 sigma footprint by int64 truncation (NaN / out of range -> INT64_MIN, as cvttsd2si), and per pixel
``pix = float32(float64(pix) + norm * exp(-0.5 * float64(e)))`` with the C library's exp (``math.exp``).  The pixels of
one footprint are evaluated as arrays: each pixel sees the operations of the plain double loop.

make_goldens_rotrender.py asserts that all of this equals the reference in every bit on the finite cases; the rows with
non-finite widths are stated here alone (the emulation of numba's typing cannot do numba's ``int(NaN)``)."""
import math
import struct

import numpy as np

F32 = np.float32
INT64_MIN = -2 ** 63


# ---- scalar helpers ---------------------------------------------------------------------------------------------------
def fmaf(a, b, c):
    """float32 fused multiply-add: the float64 product of two float32 is exact, the sum is rounded to odd in float64
    (TwoSum), and float64 -> float32 then rounds once."""
    p, c = float(a) * float(b), float(c)
    t = p + c
    if math.isfinite(t):
        bb = t - p
        err = (p - (t - bb)) + (c - bb)
        if err != 0.0:
            (bits,) = struct.unpack("<q", struct.pack("<d", abs(t)))
            bits = (bits | 1) if (err > 0) == (t > 0) else ((bits - 1) | 1)
            (mag,) = struct.unpack("<d", struct.pack("<q", bits))
            t = math.copysign(mag, t)
    return F32(t)


def to_int64(v):
    v = float(v)
    return INT64_MIN if (v != v or v >= 9223372036854775808.0 or v < -9223372036854775808.0) else int(v)


def to_int32(v):
    v = float(v)
    return -2 ** 31 if (v != v or v >= 2147483648.0 or v < -2147483648.0) else int(v)


def libm_exp(v):
    try:
        return math.exp(v)
    except OverflowError:
        return math.inf


# ---- the columns --------------------------------------------------------------------------------------------------------
def coords(x, y, z):
    """Three float32 columns stay float32; anything else becomes float64 (``locs[["x", "y", "z"]].to_numpy()``)."""
    cols = [np.asarray(c) for c in (x, y, z)]
    dt = np.float32 if all(c.dtype == np.float32 for c in cols) else np.float64
    return [c.astype(dt) for c in cols]


def rotate(x, y, z, M, oversampling, y_min, x_min, y_max, x_max):
    """-> (x', y', z' float64 in image units, in_view) for every row of the table."""
    x, y, z = coords(x, y, z)
    M = np.asarray(M, np.float64)
    cx, cy = x_min + (x_max - x_min) / 2, y_min + (y_max - y_min) / 2
    with np.errstate(all="ignore"):
        if x.dtype == np.float32:
            v0, v1 = (x - F32(cx)).astype(np.float64), (y - F32(cy)).astype(np.float64)
        else:
            v0, v1 = x - cx, y - cy
        v2 = z.astype(np.float64)
        if len(v0) == 1:
            r = [(M[i, 0] * v0 + M[i, 2] * v2) + M[i, 1] * v1 for i in range(3)]
        else:
            r = [(M[i, 0] * v0 + M[i, 1] * v1) + M[i, 2] * v2 for i in range(3)]
        xr, yr = r[0] + cx, r[1] + cy
        in_view = (xr > x_min) & (yr > y_min) & (xr < x_max) & (yr < y_max)
        return oversampling * (xr - x_min), oversampling * (yr - y_min), oversampling * r[2], in_view


def widths(lpx, lpy, lpz, oversampling, min_blur_width, iso):
    """float32 sx, sy, sz of every row."""
    lpx, lpy = np.asarray(lpx, F32), np.asarray(lpy, F32)
    os_f, mb = F32(oversampling), F32(min_blur_width)
    with np.errstate(all="ignore"):
        sx, sy = os_f * np.maximum(lpx, mb), os_f * np.maximum(lpy, mb)
        if iso:
            sy = (sy + sx) / F32(2.0)
            sx = sy
        lpz = F32(2.0) * ((lpx + lpy) / F32(2.0)) if lpz is None else np.asarray(lpz, F32)
        return sx, sy, os_f * np.maximum(lpz, mb)


def image_shape(oversampling, y_min, x_min, y_max, x_max):
    return int(np.ceil(oversampling * (y_max - y_min))), int(np.ceil(oversampling * (x_max - x_min)))


# ---- one localization -----------------------------------------------------------------------------------------------------
def record(x_, y_, sx, sy, sz, R, n_y, n_x):
    """None where nothing is drawn (det < 1e-10, empty footprint), else
    (inv00, m, inv11 float32, norm float64, i_min, i_max, j_min, j_max).  R: the float32 matrix."""
    with np.errstate(all="ignore"):
        c = (F32(sx) * F32(sx), F32(sy) * F32(sy), F32(sz) * F32(sz))
        P = [[F32(R[i, k]) * c[k] for k in range(3)] for i in range(2)]
        S = [[fmaf(P[i][2], R[j, 2], fmaf(P[i][1], R[j, 1], P[i][0] * F32(R[j, 0]))) for j in range(2)] for i in range(2)]
        det = S[0][0] * S[1][1] - S[0][1] * S[1][0]
        if float(det) < 1e-10:
            return None
        inv00, inv01, inv10, inv11 = S[1][1] / det, -S[0][1] / det, -S[1][0] / det, S[0][0] / det
        m = inv01 + inv10
        norm = 1.0 / (6.283185307179586 * float(np.sqrt(det)))
        x_off, y_off = 3.0 * float(np.sqrt(S[0][0])), 3.0 * float(np.sqrt(S[1][1]))
    j_min, j_max = max(to_int64(x_ - x_off), 0), min(to_int64(x_ + x_off + 1), n_x)
    i_min, i_max = max(to_int64(y_ - y_off), 0), min(to_int64(y_ + y_off + 1), n_y)
    if j_max <= j_min or i_max <= i_min:
        return None
    return inv00, m, inv11, norm, i_min, i_max, j_min, j_max


def draw(image, x_, y_, rec):
    inv00, m, inv11, norm, i_min, i_max, j_min, j_max = rec
    with np.errstate(all="ignore"):
        a = (np.arange(j_min, j_max) + 0.5 - x_).astype(F32)[None, :]
        b = (np.arange(i_min, i_max) + 0.5 - y_).astype(F32)[:, None]
        e = ((a * a) * inv00 + ((a * b) * m)) + (b * b) * inv11
        assert e.dtype == F32
        arg = -0.5 * e.astype(np.float64)
        ex = np.array([libm_exp(v) for v in arg.ravel()], np.float64).reshape(arg.shape)
        part = image[i_min:i_max, j_min:j_max]
        part[...] = (part.astype(np.float64) + norm * ex).astype(F32)


# ---- the renders ------------------------------------------------------------------------------------------------------------
def render_gaussian(x, y, z, lpx, lpy, lpz, M, oversampling, y_min, x_min, y_max, x_max, min_blur_width, iso=False):
    """-> (n, image float32); M: the float64 (3, 3) matrix, rounded to float32 here for the covariance."""
    n_y, n_x = image_shape(oversampling, y_min, x_min, y_max, x_max)
    image = np.zeros((n_y, n_x), F32)
    xr, yr, _, in_view = rotate(x, y, z, M, oversampling, y_min, x_min, y_max, x_max)
    sx, sy, sz = widths(lpx, lpy, lpz, oversampling, min_blur_width, iso)
    R = np.ascontiguousarray(M, dtype=F32)
    for k in np.flatnonzero(in_view):
        rec = record(xr[k], yr[k], sx[k], sy[k], sz[k], R, n_y, n_x)
        if rec is not None:
            draw(image, xr[k], yr[k], rec)
    return int(in_view.sum()), image


def render_hist(x, y, z, M, oversampling, y_min, x_min, y_max, x_max):
    """-> (n, image float32).  A row whose x' or y' rounds up to the image side is counted and not drawn."""
    n_y, n_x = image_shape(oversampling, y_min, x_min, y_max, x_max)
    image = np.zeros((n_y, n_x), F32)
    xr, yr, _, in_view = rotate(x, y, z, M, oversampling, y_min, x_min, y_max, x_max)
    for k in np.flatnonzero(in_view):
        xi, yi = to_int32(xr[k]), to_int32(yr[k])
        if 0 <= xi < n_x and 0 <= yi < n_y:
            image[yi, xi] += F32(1.0)
    return int(in_view.sum()), image


# ---- rotations and tables the tests and the minting script share ----------------------------------------------------------
EULER = {"identity": (0.0, 0.0, 0.0), "quarter_x": (np.pi / 2, 0.0, 0.0), "generic": (0.7, -0.4, 1.1)}
QUAT = (0.18257418583505536, 0.3651483716701107, 0.5477225575051661, 0.7302967433402214)      # (1, 2, 3, 4) / sqrt(30)


def table(rng, n, n_y, n_x, oversampling, with_lpz=True, spread=1.3, z_scale=1.0):
    """n rows around a viewport of n_y x n_x display pixels at (0, 0): more than the view holds in x and y, so that a
    rotation moves rows out of it and others into it; widths of 0.3 .. 1.5 display pixels."""
    h, w = n_y / oversampling, n_x / oversampling
    cols = {"x": rng.uniform(w * (1 - spread) / 2, w * (1 + spread) / 2, n).astype(F32),
            "y": rng.uniform(h * (1 - spread) / 2, h * (1 + spread) / 2, n).astype(F32),
            "z": (rng.normal(0, 0.25 * min(h, w) * z_scale, n)).astype(F32),
            "lpx": (rng.uniform(0.3, 1.5, n) / oversampling).astype(F32),
            "lpy": (rng.uniform(0.3, 1.5, n) / oversampling).astype(F32)}
    if with_lpz:
        cols["lpz"] = (rng.uniform(0.5, 3.0, n) / oversampling).astype(F32)
    return cols
