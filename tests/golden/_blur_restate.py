"""A NumPy restatement of the image blur behind the "smooth" and "convolve" renders (picasso/render.py:1413-1460
``_fftconvolve``), written for the tests, and the cases the tests and tests/golden/make_goldens_blur.py share.

Spatial route: scipy.ndimage.gaussian_filter(mode="constant", cval=0, truncate=5.0, output=float32) as scipy 1.15 runs
it: axis 0 first, float32 between the axes, and per output sample of a zero-extended line, in float64,
``tmp = line[l] * w[r]``, then for ``j = r .. 1``: ``tmp += (line[l - j] + line[l + j]) * w[r - j]``.  Direct route:
the same two sums with the reference's window functions as weights, float64 between the axes, ``tmp * (1 / S)`` and one
rounding to float32.  ``separable`` vectorises over the samples and keeps the order over j, so each sample sees the
operations of the plain loop.  The tests check it against scipy in bits and the device against it."""
import numpy as np
from scipy import signal


def gaussian_kernel1d(sigma, radius):
    sigma2 = sigma * sigma
    x = np.arange(-radius, radius + 1)
    phi_x = np.exp(-0.5 / sigma2 * x ** 2)
    return phi_x / phi_x.sum()


def one_axis(a, w, r, axis):
    """float64 array -> float64 array: the symmetric correlate1d of every line along ``axis``, extended by zeros."""
    a = np.moveaxis(np.asarray(a, np.float64), axis, 0)
    n = a.shape[0]
    pad = np.zeros((n + 2 * r,) + a.shape[1:], np.float64)
    pad[r:r + n] = a
    tmp = pad[r:r + n] * w[r]
    for j in range(r, 0, -1):
        tmp = tmp + (pad[r - j:r - j + n] + pad[r + j:r + j + n]) * w[r - j]
    return np.moveaxis(tmp, 0, axis)


def separable(image, wy, wx, round_between, scale=1.0):
    """``wy`` / ``wx``: float64 weights of 2 r + 1 values, or None for a skipped axis."""
    a = np.asarray(image, np.float32)
    for axis, w in ((0, wy), (1, wx)):
        if w is None:
            continue
        a = one_axis(a, w, len(w) // 2, axis)
        if round_between:
            a = a.astype(np.float32)
    if round_between:
        return np.array(a, np.float32)
    return (np.asarray(a, np.float64) * scale).astype(np.float32)


def spatial(image, sigma_y, sigma_x):
    weights = [gaussian_kernel1d(float(s), int(5.0 * float(s) + 0.5)) if s > 1e-15 else None for s in (sigma_y, sigma_x)]
    return separable(image, weights[0], weights[1], True)


def direct_weights(kernel_width, kernel_height, blur_width, blur_height):
    ky = signal.windows.gaussian(kernel_height, blur_height)
    kx = signal.windows.gaussian(kernel_width, blur_width)
    return ky, kx, float(np.outer(ky, kx).sum())


def direct(image, kernel_width, kernel_height, blur_width, blur_height):
    ky, kx, S = direct_weights(kernel_width, kernel_height, blur_width, blur_height)
    return separable(image, ky, kx, False, float(np.float64(1.0) / np.float64(S)))


def direct_float64(image, kernel_width, kernel_height, blur_width, blur_height):
    """The float64 direct convolution the reference's FFT result is measured against (not rounded to float32)."""
    ky, kx, S = direct_weights(kernel_width, kernel_height, blur_width, blur_height)
    a = one_axis(one_axis(np.asarray(image, np.float32), ky, len(ky) // 2, 0), kx, len(kx) // 2, 1)
    return a / S


def fft_reference(image, kernel_width, kernel_height, blur_width, blur_height):
    """The reference's FFT route, line for line (picasso/render.py:1455-1460), on scipy alone."""
    kernel_y = signal.windows.gaussian(kernel_height, blur_height)
    kernel_x = signal.windows.gaussian(kernel_width, blur_width)
    kernel = np.outer(kernel_y, kernel_x)
    kernel /= kernel.sum()
    return signal.fftconvolve(np.asarray(image, np.float32), kernel, mode="same").astype(np.float32)


def poisson_image(n_y, n_x, seed):
    """Poisson-filled float32 with one pixel of 60000 near a corner and one at the far edge."""
    rng = np.random.default_rng(seed)
    image = rng.poisson(0.7, (n_y, n_x)).astype(np.float32)
    image[min(1, n_y - 1), min(2, n_x - 1)] = 60000.0
    image[n_y - 1, n_x // 2] = 60000.0
    return image


# (n_y, n_x, sigma_y, sigma_x): the device against scipy.ndimage.gaussian_filter, in bits
SPATIAL_CASES = [
    (221, 221, 1, 1),
    (221, 300, 1.37, 2.9),
    (300, 221, 2.9, 1.37),
    (257, 263, 0.3, 1),
    (257, 263, 0, 1),
    (257, 263, 0, 0),
    (2021, 2021, 10.49, 10.49),
    (2021, 230, 10.49, 1),
]
# the host restatement against scipy (the 2021-pixel sides are left to the device test: minutes in NumPy on some hosts)
SPATIAL_HOST_CASES = SPATIAL_CASES[:6] + [(300, 260, 1, 1), (257, 301, 1.37, 2.9), (700, 650, 3.3, 0.61), (130, 90, 10.49, 1)]
# (n_y, n_x, blur_width, blur_height): the reference's FFT cases; kernel = 10 * int(round(width)) + 1
DIRECT_CASES = [
    (1, 1, 1, 1),
    (1, 64, 1, 1),
    (64, 64, 1, 1),
    (220, 220, 1, 1),
    (33, 47, 2.6, 1.2),
    (40, 40, 11, 12),
]


def kernel_of(width):
    return 10 * int(np.round(width)) + 1
