"""NumPy restatement of the Fourier ring correlation (picasso/postprocess.py:1320-1502, picasso/masking.py:649-671,
picasso/imageprocess.py:283-321) for the tests: the host code of ``frc`` (viewport squaring, split), the window, exact
integer ring masks, and two evaluators of the ring sums from the masked float32 images:

* ``T``: ``np.fft.fft2`` on float64 input -- what NumPy's own double-precision transform gives;
* ``L``: a separable DFT in ``np.longdouble`` (two matrix products) -- the truth the others are measured against.

TEST INFRASTRUCTURE: nothing here is used by the package."""
import math

import numpy as np


def tukey_profile(width):
    nfac = 8
    x = np.arange(width)
    x_im = (x - (width / 2)) / width
    mask = 0.5 - 0.5 * np.cos(np.pi * nfac * x_im)
    mask[np.abs(x_im) < ((nfac - 2) / (nfac * 2))] = 1
    return mask


def crop(im):
    return im[:-1, :-1] if im.shape[0] % 2 == 0 else im


def masked(im):
    """float32 image -> float32(float64(im) * (w[j] * w[n - 1 - i])) on the odd side."""
    im = crop(np.asarray(im, np.float32))
    w = tukey_profile(im.shape[0])
    mask = w[None, :] * w[::-1][:, None]
    return (im.astype(np.float64) * mask).astype(np.float32)


def ring_index(n):
    """(n, n) int: the ring of every bin of a centred image of odd side n, -1 beyond ring n // 2.  Integer arithmetic."""
    c = n // 2
    k = np.arange(n) - c
    d = k[:, None] ** 2 + k[None, :] ** 2
    r = np.array([[math.isqrt(int(v)) for v in row] for row in d])
    assert np.all(r * r <= d) and np.all(d < (r + 1) ** 2)
    return np.where(r <= c, r, -1)


def ring_counts(n):
    ring = ring_index(n)
    return np.bincount(ring[ring >= 0], minlength=n // 2 + 1)


def ring_sum(values, ring):
    """Sum of ``values`` per ring in the type of ``values`` (float64, longdouble or their complex kinds)."""
    rings = int(ring.max()) + 1
    out = np.zeros(rings, values.dtype)
    for r in range(rings):
        out[r] = values[ring == r].sum()
    return out


def spectrum_T(image):
    return np.fft.fftshift(np.fft.fft2(np.asarray(image, np.float64)))


_LPI = 4 * np.arctan(np.longdouble(1))


def dft_matrix_L(n):
    """W[k + c, x] = exp(-2 pi i k x / n) in longdouble, the angle reduced in integers first."""
    k = np.arange(n) - n // 2
    j = (k[:, None] * np.arange(n)[None, :]) % n
    angle = (2 * _LPI) * j.astype(np.longdouble) / np.longdouble(n)
    return (np.cos(angle) - 1j * np.sin(angle)).astype(np.clongdouble)


def spectrum_L(image):
    """The centred spectrum by two longdouble matrix products."""
    w = dft_matrix_L(image.shape[0])
    return w @ np.asarray(image, np.longdouble).astype(np.clongdouble) @ w.T


def sums_of(f1, f2, ring):
    """(numerator, power 1, power 2) per ring, in the real type of the spectra."""
    return (ring_sum((f1 * np.conj(f2)).real, ring), ring_sum(f1.real ** 2 + f1.imag ** 2, ring),
            ring_sum(f2.real ** 2 + f2.imag ** 2, ring))


def curve_of(num, p1, p2):
    with np.errstate(divide="ignore", invalid="ignore"):
        curve = num / np.sqrt(np.abs(p1 * p2))
    curve[np.isnan(curve)] = 0
    return curve


def curve_T(m1, m2):
    ring = ring_index(m1.shape[0])
    return curve_of(*sums_of(spectrum_T(m1), spectrum_T(m2), ring))


def curve_L(m1, m2):
    ring = ring_index(m1.shape[0])
    return curve_of(*sums_of(spectrum_L(m1), spectrum_L(m2), ring))


def err_L(curve, truth):
    """max |curve - L| over the curve, in longdouble."""
    return float(np.max(np.abs(np.asarray(curve).astype(np.longdouble) - truth)))


def radial_sum_exact(image):
    """Ring sums of a centred image in longdouble (per component), not yet cast."""
    image = np.asarray(image)
    ring = ring_index(image.shape[0])
    kind = np.clongdouble if np.iscomplexobj(image) else np.longdouble
    return ring_sum(image.astype(kind), ring)


def frequencies(rings, n, pixelsize, lp):
    binsize = lp / 2
    return np.arange(rings) / n / (pixelsize * binsize)


def square_viewport(viewport):
    """``frc``'s squaring of the viewport around its centre (postprocess.py:1354-1366), in Python floats."""
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
    return viewport


def split(x, y, viewport, random_seed=42):
    """-> (rows of half 1, rows of half 2, squared viewport): the rows strictly in view, permuted by the legacy global
    generator, the first len // 2 to half 1."""
    viewport = square_viewport(viewport)
    (y_min, x_min), (y_max, x_max) = viewport
    in_view = np.flatnonzero((x > x_min) & (y > y_min) & (x < x_max) & (y < y_max))
    np.random.seed(random_seed)
    r_idx = np.random.permutation(len(in_view))
    return in_view[r_idx[: len(r_idx) // 2]], in_view[r_idx[len(r_idx) // 2:]], viewport


def render_hist(x, y, oversampling, viewport):
    """The histogram render of float32 columns (picasso/render.py:451-467, :177-232): float32 counts."""
    (y_min, x_min), (y_max, x_max) = viewport
    n_y = int(np.ceil(oversampling * (y_max - y_min)))
    n_x = int(np.ceil(oversampling * (x_max - x_min)))
    x, y = np.asarray(x, np.float32), np.asarray(y, np.float32)
    keep = (x > x_min) & (y > y_min) & (x < x_max) & (y < y_max)
    px = (oversampling * (x[keep] - x_min)).astype(np.int32)
    py = (oversampling * (y[keep] - y_min)).astype(np.int32)
    image = np.zeros((n_y, n_x), np.float32)
    np.add.at(image, (py, px), 1)
    return image
