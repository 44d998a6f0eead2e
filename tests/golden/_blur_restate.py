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


# ---- the edge cases of tests/test_blur_edges_host.py and tests/test_gpu_blur_edges.py -------------------------------------
# Chosen for the control flow of csrc/blur.hip that only a device run takes: the chunked walk over j (64 steps per chunk
# in the row pass, 32 in the column pass), the tiles (256 outputs per row tile, 64 x 32 per column tile, 8 rows per
# lane), the grid-stride loop behind 2 ** 20 workgroups, and the single-axis and no-axis launches.  The host tier reads
# those constants out of blur.hip and checks that the lists below still sit on them.
from collections import namedtuple  # noqa: E402

from scipy import ndimage  # noqa: E402

# sigma 0 skips the axis (radius 0); ``r_y`` / ``r_x`` are the radii the case is there for, asserted against the plan by
# both tiers.  ``gain`` multiplies the weights of both axes: 1 is ``gaussian_filter`` itself, any other value a hand-made
# plan (normalised weights cannot overflow, so the "huge" kind needs one to reach inf).
EdgeSpatial = namedtuple("EdgeSpatial", "n_y n_x sigma_y sigma_x r_y r_x kind gain", defaults=("poisson", 1.0))
# ``entry``: "fft" goes through render._fftconvolve (radius 5 * round(width)), "plan" through backend.direct_plan with
# kernel 2 r + 1 (radii no width gives), "wy" / "wx" / "none" through a hand-made BlurPlan with one axis or none
# (launches no entry point reaches).  ``s_gain`` multiplies S (1 except on the hand-made "huge" plan).
EdgeDirect = namedtuple("EdgeDirect", "n_y n_x entry width height r_y r_x kind s_gain", defaults=("poisson", 1.0))

EDGE_SPATIAL_CASES = [
    # row pass: radii 63, 64, 65, 127, 128, 129, 193 on widths 255, 256, 257, 512, 513
    EdgeSpatial(7, 255, 0, 12.55, 0, 63),
    EdgeSpatial(6, 256, 0.6, 12.7, 3, 64),
    EdgeSpatial(5, 257, 0, 12.9, 0, 65),
    EdgeSpatial(4, 512, 0.6, 25.35, 3, 127),
    EdgeSpatial(3, 513, 0.3, 25.55, 2, 128),
    EdgeSpatial(3, 513, 0, 25.7, 0, 129),
    EdgeSpatial(9, 257, 0.6, 38.5, 3, 193),
    EdgeSpatial(2, 255, 0, 51.4, 0, 257),             # r_x > n_x
    EdgeSpatial(3, 100, 0, 25.7, 0, 129),             # r_x > n_x
    EdgeSpatial(3, 64, 0.6, 25.7, 3, 129),            # r_x >= 2 n_x
    EdgeSpatial(4, 1, 0.6, 12.9, 3, 65),              # n_x = 1
    # column pass: radii 31, 32, 33, 64, 65, 97 on heights 1, 31, 32, 33, 64, 65 and 36, 41 (a lane's strip of eight
    # rows ends part-way), widths 1, 63, 64, 65, 129
    EdgeSpatial(31, 63, 6.15, 0, 31, 0),
    EdgeSpatial(32, 64, 6.3, 0.6, 32, 3),
    EdgeSpatial(33, 65, 6.5, 0, 33, 0),
    EdgeSpatial(64, 129, 12.7, 0.6, 64, 3),
    EdgeSpatial(65, 1, 12.9, 0, 65, 0),
    EdgeSpatial(65, 129, 19.35, 0, 97, 0),            # r_y > n_y
    EdgeSpatial(41, 64, 12.9, 0, 65, 0),              # r_y > n_y
    EdgeSpatial(36, 65, 19.35, 0.3, 97, 2),           # r_y >= 2 n_y
    EdgeSpatial(1, 63, 6.5, 0.6, 33, 3),              # n_y = 1
    # both passes on their chunk edges at once
    EdgeSpatial(65, 257, 6.5, 12.9, 33, 65),
    EdgeSpatial(64, 256, 12.7, 25.55, 64, 128),
    # content: two chunks in at least one pass
    EdgeSpatial(40, 70, 6.5, 12.9, 33, 65, "subnormal"),
    EdgeSpatial(40, 70, 6.5, 12.9, 33, 65, "huge"),
    EdgeSpatial(40, 70, 6.5, 12.9, 33, 65, "huge", 32.0),
    EdgeSpatial(6, 140, 0.05, 12.9, 0, 65, "signed"),
    EdgeSpatial(40, 70, 6.5, 0.6, 33, 3, "nonfinite"),
]

EDGE_DIRECT_CASES = [
    # row pass
    EdgeDirect(7, 255, "wx", 12.6, None, 0, 63),
    EdgeDirect(6, 256, "plan", 12.8, 0.6, 3, 64),
    EdgeDirect(5, 257, "fft", 13, 1, 5, 65),
    EdgeDirect(4, 512, "wx", 25.4, None, 0, 127),
    EdgeDirect(3, 513, "plan", 25.6, 0.4, 2, 128),
    EdgeDirect(3, 513, "plan", 25.8, 1, 0, 129),
    EdgeDirect(9, 257, "plan", 38.6, 0.6, 3, 193),
    EdgeDirect(2, 255, "wx", 51.4, None, 0, 257),     # r_x > n_x
    EdgeDirect(3, 100, "plan", 25.8, 1, 0, 129),      # r_x > n_x
    EdgeDirect(3, 64, "plan", 25.8, 0.6, 3, 129),     # r_x >= 2 n_x
    EdgeDirect(4, 1, "fft", 13, 1, 5, 65),            # n_x = 1
    # column pass
    EdgeDirect(31, 63, "wy", None, 6.2, 31, 0),
    EdgeDirect(32, 64, "plan", 0.6, 6.4, 32, 3),
    EdgeDirect(33, 65, "wy", None, 6.6, 33, 0),
    EdgeDirect(64, 129, "plan", 0.6, 12.8, 64, 3),
    EdgeDirect(65, 1, "fft", 1, 13, 65, 5),
    EdgeDirect(65, 129, "plan", 1, 19.4, 97, 0),      # r_y > n_y
    EdgeDirect(41, 64, "wy", None, 13, 65, 0),        # r_y > n_y
    EdgeDirect(36, 65, "plan", 0.4, 19.4, 97, 2),     # r_y >= 2 n_y
    EdgeDirect(1, 63, "plan", 0.6, 6.6, 33, 3),       # n_y = 1
    # both passes
    EdgeDirect(65, 257, "plan", 13, 6.6, 33, 65),
    EdgeDirect(65, 257, "fft", 13, 26, 130, 65),
    EdgeDirect(64, 256, "plan", 25.6, 12.8, 64, 128),
    # no axis: scale_copy_kernel
    EdgeDirect(33, 65, "none", None, None, 0, 0),
    # content
    EdgeDirect(40, 70, "fft", 13, 1, 5, 65, "subnormal"),
    EdgeDirect(40, 70, "fft", 13, 1, 5, 65, "huge"),
    EdgeDirect(40, 70, "plan", 13, 1, 5, 65, "huge", 2.0 ** -6),
    EdgeDirect(6, 140, "fft", 13, 0.3, 0, 65, "signed"),
    EdgeDirect(40, 70, "fft", 13, 1, 5, 65, "nonfinite"),
]

# the grid-stride loop: more than 2 ** 20 tiles in the row pass (five workgroups take a second tile, with r_x = 3 staged
# again) and in the column pass (128 MiB per buffer: the one large case, left out of the host tier)
EDGE_GRID_ROW_CASE = EdgeSpatial(2 ** 20 + 5, 3, 0.6, 0.5, 3, 3)
EDGE_GRID_COL_CASE = EdgeSpatial(2 ** 25 + 40, 1, 0.6, 0, 3, 0)


def edge_id(case):
    return "-".join(str(v) for v in case)


def edge_image(n_y, n_x, seed, kind="poisson"):
    """float32 image of one content kind.  "subnormal": the counts times 2 ** -140, so that every blurred pixel is a float32 subnormal.  "huge":
    neighbouring pixels of 3e38, and one of the largest float32, among ordinary ones.  "signed": -1 for an empty pixel,
    -0.0 for a count of one, and a last row of -0.0 alone.  "nonfinite": +inf and -inf three columns and two rows apart,
    and one NaN."""
    image = poisson_image(n_y, n_x, seed)
    if kind == "subnormal":
        image = image * np.float32(2.0 ** -140)
    elif kind == "huge":
        image[3, 5] = image[3, 6] = image[n_y // 2, n_x // 2] = image[n_y // 2 + 1, n_x // 2] = 3e38
        image[n_y - 2, 2] = np.finfo(np.float32).max
    elif kind == "signed":
        image = image - np.float32(1.0)
        image[image == 0] = -0.0
        image[n_y - 1] = -0.0
    elif kind == "nonfinite":
        image[5, 10], image[7, 13], image[n_y - 10, n_x - 10] = np.inf, -np.inf, np.nan
    elif kind != "poisson":
        raise ValueError(kind)
    return image


def edge_spatial_weights(case):
    """(w_y, w_x) of a spatial edge case: scipy's Gaussian weights times the case's gain, None for a skipped axis."""
    return tuple(gaussian_kernel1d(float(s), int(5.0 * float(s) + 0.5)) * case.gain if s > 1e-15 else None
                 for s in (case.sigma_y, case.sigma_x))


def edge_spatial_reference(case, image):
    """scipy's result: ``gaussian_filter`` itself, or for a hand-made plan (gain != 1) the correlate1d per axis that
    ``gaussian_filter`` is made of, axis 0 first and float32 after each."""
    with np.errstate(all="ignore"):
        if case.gain == 1.0:
            out = np.empty_like(image)
            ndimage.gaussian_filter(image, sigma=(case.sigma_y, case.sigma_x), output=out, mode="constant", cval=0.0, truncate=5.0)
            return out
        out = image
        for axis, w in enumerate(edge_spatial_weights(case)):
            if w is not None:
                out = ndimage.correlate1d(out, w, axis=axis, output=np.float32, mode="constant", cval=0.0)
        return out


def edge_direct_parts(case):
    """(w_y, w_x, S) of a direct edge case, as the reference's FFT route makes them (``direct_weights``); an axis a
    hand-made plan leaves out is None, and S is then the sum of the other axis alone (3 with no axis at all)."""
    kh, kw = 2 * case.r_y + 1, 2 * case.r_x + 1
    if case.entry == "none":
        return None, None, 3.0 * case.s_gain
    if case.entry == "wy":
        w = signal.windows.gaussian(kh, case.height)
        return w, None, float(w.sum()) * case.s_gain
    if case.entry == "wx":
        w = signal.windows.gaussian(kw, case.width)
        return None, w, float(w.sum()) * case.s_gain
    if case.entry == "fft":
        assert (kh, kw) == (kernel_of(case.height), kernel_of(case.width)), case
    ky, kx, S = direct_weights(kw, kh, case.width, case.height)
    return ky, kx, S * case.s_gain


def edge_direct_reference(case, image):
    """Two scipy.ndimage.correlate1d passes over the float64 image, axis 0 then axis 1, times 1 / S, one rounding."""
    wy, wx, S = edge_direct_parts(case)
    a = np.asarray(image, np.float64)
    with np.errstate(all="ignore"):
        for axis, w in ((0, wy), (1, wx)):
            if w is not None:
                a = ndimage.correlate1d(a, w, axis=axis, mode="constant", cval=0.0)
        return (a * (1.0 / S)).astype(np.float32)


def differing_but_nan(got, want):
    """Pixels whose float32 bit patterns differ.  Where the reference is NaN the other must be NaN, of any sign and
    payload: inf - inf is the negative default NaN on x86 and the positive one on the device."""
    assert got.dtype == want.dtype == np.float32 and got.shape == want.shape, (got.dtype, want.dtype, got.shape, want.shape)
    bits = np.ascontiguousarray(got).view(np.uint32) != np.ascontiguousarray(want).view(np.uint32)
    return int((bits & ~(np.isnan(want) & np.isnan(got))).sum())
