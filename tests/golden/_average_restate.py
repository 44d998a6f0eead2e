"""The exact oracle of the particle averaging (picasso/average.py align_group_core over render_hist_numba), in NumPy.

TEST INFRASTRUCTURE.  Same binning as the reference (its expressions, so NumPy's types), the cross-correlation as the
INTEGER it is, and the tie rule the reference's code states: ``argmax`` takes the first flat index of the fftshifted
correlation, the angle loop keeps a candidate only when strictly larger (so the lowest angle wins, and nothing is
chosen while every value is 0).

The correlation is computed two ways, which must agree:
  gather   shifted[iy, ix] = sum over the group's pixels (py, px) of avg[(py - sy) % n, (px - sx) % n],
           (sy, sx) = ((iy - n // 2) % n, (ix - n // 2) % n)   -- the index map of np.fft.fftshift, odd and even n
  fft      rint(fftshift(real(ifft2(fft2(image) * conj(fft2(avg)))))) in float64, exact at these magnitudes
"""
import numpy as np

NONE = (0, -1, -1)


def n_pixel_of(oversampling, t_min, t_max):
    return int(np.ceil(oversampling * (t_max - t_min)))


def pixels(x, y, oversampling, t_min, t_max):
    """(py, px) int32 of the rows in view, in the reference's types."""
    in_view = (x > t_min) & (y > t_min) & (x < t_max) & (y < t_max)
    px = (oversampling * (x[in_view] - t_min)).astype(np.int32)
    py = (oversampling * (y[in_view] - t_min)).astype(np.int32)
    return py, px


def image_of(x, y, oversampling, t_min, t_max):
    """int32 histogram image (render_hist_numba with integer counts)."""
    n = n_pixel_of(oversampling, t_min, t_max)
    py, px = pixels(x, y, oversampling, t_min, t_max)
    image = np.zeros((n, n), np.int32)
    np.add.at(image, (py, px), 1)
    return image


def rotated(xo, yo, angle):
    return np.cos(angle) * xo - np.sin(angle) * yo, np.sin(angle) * xo + np.cos(angle) * yo


def correlation_fft(py, px, avg):
    n = avg.shape[0]
    image = np.zeros((n, n), np.float64)
    np.add.at(image, (py, px), 1)
    raw = np.real(np.fft.ifft2(np.fft.fft2(image) * np.conj(np.fft.fft2(avg.astype(np.float64)))))
    whole = np.rint(raw)
    assert np.abs(raw - whole).max() < 1e-3, np.abs(raw - whole).max()
    return np.fft.fftshift(whole.astype(np.int64))


def correlation_gather(py, px, avg):
    n = avg.shape[0]
    s = (np.arange(n) - n // 2) % n                       # the unshifted shift of every shifted index
    rows = (py.astype(np.int64)[:, None] - s[None, :]) % n
    cols = (px.astype(np.int64)[:, None] - s[None, :]) % n
    out = np.zeros((n, n), np.int64)
    for k in range(0, len(py), 64):
        out += avg.astype(np.int64)[rows[k:k + 64, :, None], cols[k:k + 64, None, :]].sum(axis=0)
    return out


def correlation(xo, yo, angle, avg, oversampling, t_min, t_max, both=True):
    """int64 fftshifted correlation of one group at one angle."""
    x_rot, y_rot = rotated(xo, yo, angle)
    py, px = pixels(x_rot, y_rot, oversampling, t_min, t_max)
    corr = correlation_fft(py, px, avg)
    if both:
        assert np.array_equal(corr, correlation_gather(py, px, avg))
    return corr


def align_group(xo, yo, angles, avg, oversampling, t_min, t_max, check_every=1):
    """-> ((value, angle index, flat index), x_aligned float64, y_aligned float64) of one group."""
    n = avg.shape[0]
    best = NONE
    for ai, angle in enumerate(angles):
        corr = correlation(xo, yo, angle, avg, oversampling, t_min, t_max, both=ai % check_every == 0)
        k = int(corr.argmax())
        if corr.flat[k] > best[0]:
            best = (int(corr.flat[k]), ai, k)
    rot, dy, dx = 0.0, 0.0, 0.0
    if best[1] >= 0:
        rot = angles[best[1]]
        y_max, x_max = np.unravel_index(best[2], (n, n))
        dy = np.ceil(y_max - n / 2) / oversampling
        dx = np.ceil(x_max - n / 2) / oversampling
    x_al = np.cos(rot) * xo - np.sin(rot) * yo - dx
    y_al = np.sin(rot) * xo + np.cos(rot) * yo - dy
    return best, x_al, y_al


def iteration(x, y, order, offsets, angles, oversampling, t_min, t_max, check_every=1):
    """One alignment step from the float32 state (x, y) -> (int32 image, int64 choices (groups, 3), float32 x, y)."""
    assert x.dtype == np.float32 and y.dtype == np.float32
    avg = image_of(x, y, oversampling, t_min, t_max)
    x_new, y_new = x.copy(), y.copy()
    choices = np.zeros((len(offsets) - 1, 3), np.int64)
    for g in range(len(offsets) - 1):
        index = order[offsets[g]:offsets[g + 1]]
        best, x_al, y_al = align_group(x[index], y[index], angles, avg, oversampling, t_min, t_max, check_every)
        choices[g] = best
        x_new[index] = x_al
        y_new[index] = y_al
    return avg, choices, x_new, y_new


def group_order(group):
    groups, inverse = np.unique(np.asarray(group), return_inverse=True)
    order = np.argsort(inverse, kind="stable")
    offsets = np.concatenate([[0], np.cumsum(np.bincount(inverse, minlength=len(groups)))]).astype(np.int64)
    return groups, order, offsets
