"""Shared by test_rcc_edges_host.py and test_gpu_rcc_edges.py: the edge cases of the RCC correlation stage
(csrc/xcorr.hip: correlation, fftshift, centre crop, maximum, fit window) and the reference they are held to.

The images are sparse renders of small non-negative integers (0 ... 50), so the circular cross-correlation

    c[dy, dx] = sum over (y, x) of A[y, x] * B[(y - dy) mod Y, (x - dx) mod X]

is an integer, evaluated here in int64 without any rounding; the reference image fftshift(c) / sqrt(Y * X) rounds in the
square root and in the division only.  The few float-valued cases (a NaN pixel, the smooth blobs of the end-to-end case)
go to oracle.xcorr / oracle.peak_window, which test_rcc_edges_host.py holds to the exact correlation on every integer
case.  Peak, crop offsets and ``valid`` are compared by equality, which means something only where rounding cannot move
the maximum: every reference asserts that the largest value of the cropped image exceeds every other one by MARGIN * max
|reference| (exact ties cannot be pinned through an FFT and are not part of this tier)."""
from collections import namedtuple

import numpy as np

BOUND = 1e-12              # |got - reference| <= BOUND * max |reference|, images and windows (test_gpu_parity.py's bound)
MARGIN = 1e-9              # the maximum of a cropped image leads by this much of max |reference|: 500 x the 2e-12 that BOUND needs
SHIFT_TOL = 1e-6           # px, end to end (the bound of test_rcc_shifts_on_device_match_reference_goldens)
LANES = 256                # threads of peak_kernel: lanes < box * box cut the window, every lane owns elements lane, lane + 256, ...
SUM_TRIP = 64 * 256        # pixels one trip of sum_kernel's grid-stride loop covers (at most 64 blocks of 256)

# segments (n, Y, X) float64, roi (None = no crop), box, pairs [(i, j), ...] or None, what the case is for, and the facts
# of the situation it was built to hold (test_rcc_edges_host.py checks them against the exact reference)
Case = namedtuple("Case", "segments roi box pairs what expect")
# of one pair: maximum in cropped coordinates, crop offsets, the box x box window (None when the border truncates it),
# max |reference image| and the full reference image
Ref = namedtuple("Ref", "y_max x_max Y_ X_ window scale image")

KNOWN_SIZES = [(32, 32), (33, 32), (32, 33), (33, 33), (31, 37), (24, 64)]
CROP_SIZES = [(24, 64), (31, 37)]                       # one even, one odd; neither square, so Y_ != X_
BORDER_SIZE, BORDER_ROI = (33, 32), 20                  # crop 21 x 20 at offsets (6, 6)
STRIDE_SIZE = (160, 120)


# ---- the exact reference ------------------------------------------------------------------------------------------------
def exact_correlation(a, b):
    """c[dy, dx] of the definition above, int64.  One np.roll per non-zero pixel of A: with F[k] = B[-k mod n],
    roll(F, (y, x))[dy, dx] = F[dy - y, dx - x] = B[y - dy, x - dx]."""
    a, b = as_int(a), as_int(b)
    f = np.roll(b[::-1, ::-1], (1, 1), (0, 1))
    c = np.zeros(a.shape, np.int64)
    for y, x in zip(*np.nonzero(a)):
        c += a[y, x] * np.roll(f, (y, x), (0, 1))
    return c


def exact_correlation_by_definition(a, b):
    """The same, literally: one np.roll of B per lag (for the host tier, on small images)."""
    a, b = as_int(a), as_int(b)
    Y, X = a.shape
    c = np.zeros((Y, X), np.int64)
    for dy in range(Y):
        for dx in range(X):
            c[dy, dx] = np.sum(a * np.roll(b, (dy, dx), (0, 1)))
    return c


def exact_xcorr(a, b):
    Y, X = np.shape(a)
    return np.fft.fftshift(exact_correlation(a, b)) / np.sqrt(Y * X)       # fftshift of integers only moves them


def is_integer_image(a):
    a = np.asarray(a, np.float64)
    return bool(np.all(np.isfinite(a)) and np.all(a == np.rint(a)) and np.all(np.abs(a) <= 50))


def as_int(a):
    assert is_integer_image(a)
    return np.asarray(a, np.float64).astype(np.int64)


def crop_rule(Y, X, roi):
    """(Y_, X_) of picasso/imageprocess.py:89-101."""
    if roi is None:
        return 0, 0
    return max(int((Y - roi) / 2), 0), max(int((X - roi) / 2), 0)


def assert_margin(crop, scale, what=""):
    flat = np.ravel(crop)
    k = int(np.argmax(flat))
    rest = np.delete(flat, k)
    assert rest.size == 0 or flat[k] - rest.max() >= MARGIN * scale, f"builder bug, no margin at the maximum: {what}"


def _cut(image, box, roi, what):
    """Crop, maximum and window of a reference image; the window by numpy's own slicing, as the reference cuts it."""
    Y, X = image.shape
    Y_, X_ = crop_rule(Y, X, roi)
    crop = image[Y_:Y - Y_, X_:X - X_]
    scale = float(np.abs(image).max())
    assert_margin(crop, scale, what)
    ym, xm = (int(v) for v in np.unravel_index(np.argmax(crop), crop.shape))
    h = int(box / 2)
    win = crop[ym - h:ym + h + 1, xm - h:xm + h + 1] if ym - h >= 0 and xm - h >= 0 else np.zeros((0, 0))
    return Ref(ym, xm, Y_, X_, win.copy() if win.shape == (box, box) else None, scale, image)


def exact_reference(a, b, box, roi, what=""):
    """-> None where get_image_shift returns (0, 0) for an empty image, else the Ref of the exact integer correlation."""
    if np.sum(a) == 0 or np.sum(b) == 0:
        return None
    return _cut(exact_xcorr(a, b), box, roi, what)


def oracle_reference(a, b, box, roi, what=""):
    """The same from oracle.xcorr (numpy's FFT): the reference of the float-valued cases."""
    from oracle import oracle
    if np.sum(a) == 0 or np.sum(b) == 0:
        return None
    return _cut(oracle.xcorr(a, b), box, roi, what)


def reference(case, i, j):
    a, b = case.segments[i], case.segments[j]
    exact = is_integer_image(a) and is_integer_image(b)
    return (exact_reference if exact else oracle_reference)(a, b, case.box, case.roi, f"{case.what}, pair ({i}, {j})")


# ---- images -----------------------------------------------------------------------------------------------------------------
def render(rng, Y, X, n=None):
    """A sparse integer render: n pixels of 1 ... 49 and a single brightest pixel of 50."""
    n = n or min(40, max(4, Y * X // 8))
    img = np.zeros((Y, X), np.int64)
    pos = rng.choice(Y * X, n, replace=False)
    img.flat[pos] = rng.integers(1, 50, n)
    img.flat[pos[0]] = 50
    return img


def shifted(rng, img, dy, dx, changed=3):
    """B[y, x] = A[y - dy, x - dx] with a few pixels drawn again, so the two are not identical."""
    out = np.roll(img, (dy, dx), (0, 1)).copy()
    pos = rng.choice(img.size, changed, replace=False)
    out.flat[pos] = rng.integers(0, 50, changed)
    return out


def peak_of_shift(Y, X, dy, dx):
    """Where the maximum of xcorr(A, shifted(A, dy, dx)) lies in the full fftshifted image."""
    return (Y // 2 - dy) % Y, (X // 2 - dx) % X


def shift_for_peak(Y, X, py, px):
    return (Y // 2 - py) % Y, (X // 2 - px) % X


def _one_to_many(rng, Y, X, peaks_full):
    """[A, B_1, ..., B_k] with the maximum of pair (0, k) at peaks_full[k - 1] of the full image."""
    a = render(rng, Y, X)
    segs = [a] + [shifted(rng, a, *shift_for_peak(Y, X, py, px)) for py, px in peaks_full]
    return np.asarray(segs, np.float64), [(0, k + 1) for k in range(len(peaks_full))]


# ---- builders ----------------------------------------------------------------------------------------------------------------
def known_shifts(Y, X):
    """Both signs, zero, one beyond half the side (the roll wraps) and minus half the side (row / column 0 or the last)."""
    return [(0, 0), (3, -5), (-4, 2), (Y // 2 + 1, -(X // 2 + 1)), (-(Y // 2), X // 2)]


def known_shift_case(Y, X):
    rng = np.random.default_rng(1000 * Y + X)
    a = render(rng, Y, X)
    shifts = known_shifts(Y, X)
    segs = np.asarray([a] + [shifted(rng, a, dy, dx) for dy, dx in shifts], np.float64)
    return Case(segs, None, 5, [(0, k + 1) for k in range(len(shifts))], f"known shifts {Y}x{X}",
                {"peaks": [peak_of_shift(Y, X, dy, dx) for dy, dx in shifts]})


def crop_rois(Y, X):
    return [Y - 3, Y - 2, Y - 1, Y, Y + 1, 1, 2, 8, 100]


def crop_case(Y, X, roi, box):
    """One pair whose maximum lies off the centre of the crop (at its last element when the crop is tiny)."""
    rng = np.random.default_rng(7000 + 100 * Y + X)                      # one image pair per size, whatever the roi
    Y_, X_ = crop_rule(Y, X, roi)
    cy, cx = Y - 2 * Y_, X - 2 * X_
    ty, tx = min(cy - 1, cy // 2 + 1), max(0, cx // 2 - 2)
    segs, pairs = _one_to_many(rng, Y, X, [(Y_ + ty, X_ + tx)])
    return Case(segs, roi, box, pairs, f"crop {Y}x{X} roi {roi} box {box}", {"peaks": [(ty, tx)], "crop": (cy, cx)})


def lanes_257_case(box):
    """A 1 x 257 image, whole: lane 0 of the reduction owns two elements, every other lane one."""
    rng = np.random.default_rng(257)
    segs, pairs = _one_to_many(rng, 1, 257, [(0, 256), (0, 3)])            # the maximum at lane 0's second element, and early
    return Case(segs, 300, box, pairs, f"crop of 257 elements box {box}", {"peaks": [(0, 256), (0, 3)], "crop": (1, 257)})


def box_sweep_case(box):
    rng = np.random.default_rng(64)
    segs, pairs = _one_to_many(rng, 64, 64, [(31, 34)])
    return Case(segs, None, box, pairs, f"box {box} on 64x64", {"peaks": [(31, 34)], "valid": [1]})


def box15_crop16_case():
    """Box 15 in a 16 x 16 crop: the window fits at rows / columns 7 and 8 only."""
    rng = np.random.default_rng(1516)
    peaks = [(8, 8), (7, 7), (9, 8), (8, 9)]
    segs, pairs = _one_to_many(rng, 64, 64, [(24 + y, 24 + x) for y, x in peaks])
    return Case(segs, 16, 15, pairs, "box 15 in a 16x16 crop", {"peaks": peaks, "valid": [1, 1, 0, 0], "crop": (16, 16)})


def crop_smaller_than_box_case():
    rng = np.random.default_rng(89)
    segs, pairs = _one_to_many(rng, 64, 64, [(32, 32)])
    return Case(segs, 8, 9, pairs, "an 8x8 crop under box 9", {"peaks": [(4, 4)], "valid": [0], "crop": (8, 8)})


def border_case(box):
    """The maximum h - 1, h and h + 1 pixels from each border of the crop, and in its corners (h = box / 2)."""
    (Y, X), roi = BORDER_SIZE, BORDER_ROI
    Y_, X_ = crop_rule(Y, X, roi)
    cy, cx = Y - 2 * Y_, X - 2 * X_
    h = box // 2
    peaks, valid, distance = [], [], []
    for d in (h - 1, h, h + 1):
        for y, x in ((d, cx // 2), (cy - 1 - d, cx // 2), (cy // 2, d), (cy // 2, cx - 1 - d)):       # top, bottom, left, right
            peaks.append((y, x)); valid.append(int(d >= h)); distance.append(d)
    for y, x, v in ((h - 1, h - 1, 0), (h, h, 1), (h - 1, h, 0), (cy - h, cx - h, 0), (cy - 1 - h, cx - 1 - h, 1), (0, 0, 0),
                    (cy - 1, cx - 1, 0)):
        peaks.append((y, x)); valid.append(v); distance.append(None)
    rng = np.random.default_rng(500 + box)
    segs, pairs = _one_to_many(rng, Y, X, [(Y_ + y, X_ + x) for y, x in peaks])
    return Case(segs, roi, box, pairs, f"crop border box {box}",
                {"peaks": peaks, "valid": valid, "distance": distance, "crop": (cy, cx), "h": h})


def stride_case():
    """Segments 1 and 2 hold one pixel each, past what one trip of sum_kernel's loop covers; segment 0 is empty."""
    Y, X = STRIDE_SIZE
    rng = np.random.default_rng(160120)
    segs = np.zeros((4, Y, X), np.float64)
    segs[1].flat[Y * X - 1] = 7
    segs[2].flat[SUM_TRIP] = 3
    segs[3] = render(rng, Y, X)
    return Case(segs, None, 5, None, "sum past the grid stride", {"empty": [0], "single": {1: Y * X - 1, 2: SUM_TRIP}})


def all_pairs(n):
    return [(i, j) for i in range(n - 1) for j in range(i + 1, n)]


def pairs_of(case):
    return all_pairs(len(case.segments)) if case.pairs is None else list(case.pairs)


def pair_list_segments(seed):
    """Four 32 x 32 segments: shifted copies of one render."""
    rng = np.random.default_rng(seed)
    a = render(rng, 32, 32)
    return np.asarray([a] + [shifted(rng, a, dy, dx) for dy, dx in ((2, -3), (-5, 1), (4, 6))], np.float64)


def pair_list_cases():
    """-> calls in the order they run.  P with every pair (segment 2's spectrum slot is written), then Q, of the same
    size, without segment 2 (its slot still holds P's), then Q with it; before that, (i, i), (j, i) and a repeated pair."""
    P, Q = pair_list_segments(31), pair_list_segments(32)
    return [Case(P, 20, 5, [(0, 0), (1, 1), (0, 1), (1, 0), (0, 1), (3, 0), (3, 3)], "(i, i), (j, i), a repeated pair", {}),
            Case(P, 20, 5, None, "P, every pair", {}),
            Case(Q, 20, 5, [(0, 1), (3, 1), (0, 3)], "Q without segment 2", {"unused": 2}),
            Case(Q, 20, 5, [(0, 2), (2, 1), (2, 3), (0, 1)], "Q with segment 2", {})]


def reuse_cases():
    """-> (large, small): 6 segments of 64 x 64 with every pair, 2 segments of 32 x 33."""
    rng = np.random.default_rng(66)
    a = render(rng, 64, 64)
    big = np.asarray([a] + [shifted(rng, a, dy, dx) for dy, dx in ((1, -2), (-3, 4), (5, 5), (-6, -1), (2, 7))], np.float64)
    small = known_shift_case(32, 33)
    return (Case(big, 32, 5, None, "6 segments of 64x64", {}),
            Case(small.segments[:2], None, 5, None, "2 segments of 32x33 after the large call", {}))


def nan_case():
    """Segment 2 is segment 0 with one NaN pixel."""
    rng = np.random.default_rng(99)
    a = render(rng, 32, 32)
    segs = np.asarray([a, shifted(rng, a, 2, -1), a], np.float64)
    segs[2, 11, 17] = np.nan
    return Case(segs, None, 5, [(0, 1), (0, 2), (2, 1), (2, 2)], "one NaN pixel", {"nan_pairs": [1, 2, 3]})


def blob_case(Y, X, dy, dx):
    """Float-valued and benign: a smooth symmetric blob on a pedestal and its circular translate, so that the window
    is a clean Gaussian above a positive background, symmetric about the maximum."""
    yy, xx = np.mgrid[0:Y, 0:X]
    a = 0.05 + 7.5 * np.exp(-0.5 * ((yy - (Y // 2 - 1)) ** 2 + (xx - (X // 2 + 2)) ** 2) / 1.5 ** 2)
    segs = np.asarray([a, np.roll(a, (dy, dx), (0, 1))], np.float64)
    return Case(segs, None, 5, [(0, 1)], f"blob {Y}x{X} shifted by ({dy}, {dx})",
                {"shift": (dy, dx), "peaks": [peak_of_shift(Y, X, dy, dx)]})


BLOBS = [(33, 32, 3, -2), (32, 33, -4, 5)]


def integer_cases():
    """Every integer case of the tier, for the host tier's sweep."""
    out = [known_shift_case(Y, X) for Y, X in KNOWN_SIZES]
    out += [crop_case(Y, X, roi, box) for Y, X in CROP_SIZES for roi in crop_rois(Y, X) for box in (5, 1)]
    out += [lanes_257_case(1), lanes_257_case(5)]
    out += [box_sweep_case(box) for box in range(1, 16, 2)]
    out += [box15_crop16_case(), crop_smaller_than_box_case(), border_case(5), border_case(9), stride_case()]
    out += pair_list_cases() + list(reuse_cases())
    return out
