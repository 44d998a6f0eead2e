"""Array-level calls into libpicasso_hip.so (numpy in, numpy out).

This is the thin layer the Picasso-shaped modules (localize.py, gaussmle.py)
sit on.  Nothing here computes on the CPU: every function ends in a C-ABI call
and raises if the library or the GPU is missing.
"""
from __future__ import annotations

import ctypes
from typing import NamedTuple

import numpy as np

from . import _lib

LQ_COLUMNS = [
    ("frame", np.uint32), ("x", np.float32), ("y", np.float32), ("photons", np.float32),
    ("sx", np.float32), ("sy", np.float32), ("bg", np.float32), ("lpx", np.float32),
    ("lpy", np.float32), ("ellipticity", np.float32), ("net_gradient", np.float32),
]
LOC_COLUMNS = [
    ("frame", np.uint32), ("x", np.float32), ("y", np.float32), ("photons", np.float32),
    ("sx", np.float32), ("sy", np.float32), ("bg", np.float32), ("lpx", np.float32),
    ("lpy", np.float32), ("ellipticity", np.float32), ("net_gradient", np.float32),
    ("log_likelihood", np.float32), ("iterations", np.uint32), ("photons_unc", np.float32),
    ("bg_unc", np.float32), ("sx_unc", np.float32), ("sy_unc", np.float32),
]


def dtype_code(dtype) -> int:
    dt = np.dtype(dtype)
    if dt not in _lib.DTYPE_CODES:
        raise TypeError(f"unsupported movie dtype {dt}; supported: "
                        + ", ".join(str(d) for d in _lib.DTYPE_CODES))
    return _lib.DTYPE_CODES[dt]


def as_movie_array(movie) -> np.ndarray:
    """C-contiguous native-endian (F, Y, X) view/copy of an ndarray or memmap."""
    a = np.asarray(movie)
    if a.ndim != 3:
        raise ValueError("movie must have shape (frames, height, width)")
    if not a.dtype.isnative:
        a = a.astype(a.dtype.newbyteorder("="))
    dtype_code(a.dtype)
    return np.ascontiguousarray(a)


def normalise_roi(roi, Y, X):
    """numpy slice semantics of frame[y0:y1, x0:x1] (picasso/localize.py:331)."""
    if roi is None:
        return None
    (y0, x0), (y1, x1) = roi
    ys, ye, _ = slice(y0, y1).indices(Y)
    xs, xe, _ = slice(x0, x1).indices(X)
    return np.array([ys, xs, max(ye, ys), max(xe, xs)], np.int64)


def frame_range(frame_bounds, F):
    """Inclusive range of picasso/localize.py:395-401 -> (lo, hi)."""
    lo, hi = 0, F
    if frame_bounds is not None:
        if frame_bounds[0] is not None:
            lo = max(frame_bounds[0], lo)
        if frame_bounds[1] is not None:
            hi = min(frame_bounds[1], hi)
    return int(lo), int(hi)


def identify_arrays(movie: np.ndarray, min_ng: float, box: int, roi=None, frame_bounds=None,
                    f_lo=None, f_hi=None):
    """-> frame, y, x (int32), net_gradient (float32), ordered by (frame, y, x)."""
    _lib.require_gpu()
    movie = as_movie_array(movie)
    F, Y, X = movie.shape
    r = normalise_roi(roi, Y, X)
    lo, hi = frame_range(frame_bounds, F)
    if f_lo is not None:
        lo = max(lo, f_lo)
    if f_hi is not None:
        hi = min(hi, f_hi)
    L = _lib.load()
    cap = max(4096, 256 * F)
    while True:
        fr = np.empty(cap, np.int32); yy = np.empty(cap, np.int32)
        xx = np.empty(cap, np.int32); ng = np.empty(cap, np.float32)
        n = ctypes.c_int64(0)
        with _lib.lock():
            rc = L.pmi_identify(_lib.ptr(movie), dtype_code(movie.dtype), F, Y, X, int(box), float(min_ng),
                                _lib.ptr(r), lo, hi, _lib.ptr(fr), _lib.ptr(yy), _lib.ptr(xx), _lib.ptr(ng),
                                cap, ctypes.byref(n))
        if rc == _lib.PMI_ERR_CAPACITY:
            cap = int(n.value)
            continue
        _lib.check(rc, "pmi_identify")
        k = int(n.value)
        return fr[:k].copy(), yy[:k].copy(), xx[:k].copy(), ng[:k].copy()


def net_gradient_array(image, y, x, box: int, uy, ux) -> np.ndarray:
    """float32 net gradient at the given pixels of one image (pmi_net_gradient)."""
    _lib.require_gpu()
    img = np.ascontiguousarray(image, np.float32)
    if img.ndim != 2:
        raise ValueError("image must be 2-D")
    y = np.ascontiguousarray(y, np.int32)
    x = np.ascontiguousarray(x, np.int32)
    uy = np.ascontiguousarray(uy, np.float32)
    ux = np.ascontiguousarray(ux, np.float32)
    if uy.shape != (box, box) or ux.shape != (box, box) or len(y) != len(x):
        raise ValueError("uy, ux must have shape (box, box) and y, x the same length")
    out = np.zeros(len(y), np.float32)
    with _lib.lock():
        rc = _lib.load().pmi_net_gradient(_lib.ptr(img), img.shape[0], img.shape[1], _lib.ptr(y), _lib.ptr(x), len(y),
                                          int(box), _lib.ptr(uy), _lib.ptr(ux), _lib.ptr(out))
    _lib.check(rc, "pmi_net_gradient")
    return out


def get_spots_array(movie: np.ndarray, frame, y, x, box: int, baseline, sensitivity, gain) -> np.ndarray:
    _lib.require_gpu()
    movie = as_movie_array(movie)
    F, Y, X = movie.shape
    frame = np.ascontiguousarray(frame, np.int32)
    y = np.ascontiguousarray(y, np.int32)
    x = np.ascontiguousarray(x, np.int32)
    N = len(frame)
    spots = np.empty((N, box, box), np.float32)
    with _lib.lock():
        rc = _lib.load().pmi_get_spots(_lib.ptr(movie), dtype_code(movie.dtype), F, Y, X, _lib.ptr(frame),
                                       _lib.ptr(y), _lib.ptr(x), N, int(box), float(baseline),
                                       float(sensitivity), float(gain), _lib.ptr(spots))
    _lib.check(rc, "pmi_get_spots")
    return spots


MLE_MODES = {"fast": 0, "refit": 1, "strict": 2}


def set_mle_mode(mode: str = "refit", margin: float = 0.001):
    """How the Newton loop of the MLE fit runs (pmi_mle_set_mode): "fast" = float32 loop only; "refit" (default) =
    float32 loop, then spots whose convergence decision (picasso/gaussmle.py:844-852) came within `margin` of eps
    are fitted again in the reference's float64-intermediate arithmetic; "strict" = every spot that way."""
    if mode not in MLE_MODES:
        raise ValueError(f"unknown MLE mode {mode!r}")
    _lib.check(_lib.load().pmi_mle_set_mode(MLE_MODES[mode], float(margin)), "pmi_mle_set_mode")


def get_mle_mode():
    m, g = ctypes.c_int(0), ctypes.c_double(0)
    _lib.check(_lib.load().pmi_mle_get_mode(ctypes.byref(m), ctypes.byref(g)), "pmi_mle_get_mode")
    return {v: k for k, v in MLE_MODES.items()}[m.value], g.value


MLE_LIBMS = {"device": 0, "glibc": 1, "auto": 2}


def set_mle_libm(which: str = "auto"):
    """Whose erf / exp the reference-arithmetic MLE kernel evaluates (pmi_mle_set_libm): "glibc" = the bits of the C library
    the reference's math.erf / math.exp resolve to under numba (picasso/gaussmle.py:279, 295), 12 - 18 % slower; "device" = the
    device library's functions; "auto" (default) = glibc's for every spot of the strict mode and for the re-fit of boxes up
    to 5x5, the device library's in the re-fit of larger boxes."""
    if which not in MLE_LIBMS:
        raise ValueError(f"unknown libm {which!r}")
    _lib.check(_lib.load().pmi_mle_set_libm(MLE_LIBMS[which]), "pmi_mle_set_libm")


def get_mle_libm() -> str:
    w = ctypes.c_int(0)
    _lib.check(_lib.load().pmi_mle_get_libm(ctypes.byref(w)), "pmi_mle_get_libm")
    return {v: k for k, v in MLE_LIBMS.items()}[w.value]


def last_refit_count(stream=None) -> int:
    """Spots the last MLE call OF THE CALLING THREAD fitted a second time (synchronises `stream`).  The library keeps these
    statistics — like the scratch bank, `last_flag_reasons`, `last_lq_refit_count`, `last_lq_tie_reasons` — per thread: read
    from another thread than the one that ran the fit they are 0, not an error."""
    n = ctypes.c_int64(0)
    _lib.check(_lib.load().pmi_mle_last_refit_count(ctypes.byref(n), stream), "pmi_mle_last_refit_count")
    return int(n.value)


_prewarm_threads = {}      # (device, Y, X) -> the thread making that size's FFT plans


def prewarm_fft(Y: int, X: int) -> None:
    """Start making the FFT plans of RCC undrift for Y x X frames on a side thread (once per device and size): rocFFT
    compiles a plan's kernels when the plan is made — 2.5 s at 2048 x 2048 — and a caller that localizes first has that
    time.  Call it only when an undrift will follow (`localize_file(drift=...)` does).  The worker sets the CALLER's
    device before it makes the plans (plans belong to a device, and a new thread starts on device 0), is not a daemon,
    and is joined by `join_fft_prewarm` — before the correlations run, and at interpreter exit — so it never outlives
    the library it is calling into."""
    import threading
    L = _lib.load()
    dev = ctypes.c_int(0)
    _lib.check(L.pmi_get_device(ctypes.byref(dev)), "pmi_get_device")
    key = (int(dev.value), int(Y), int(X))
    if key in _prewarm_threads or min(key[1:]) < 64:
        return

    def work():
        try:
            if L.pmi_set_device(key[0]) == 0:
                L.pmi_fft_prewarm(key[1], key[2])       # ctypes releases the GIL
        except Exception:      # noqa: BLE001 - a convenience: the correlation makes its plans itself if this did not
            pass
    t = threading.Thread(target=work, name="pmi-fft-prewarm", daemon=False)
    _prewarm_threads[key] = t
    t.start()


def join_fft_prewarm() -> None:
    """Wait for the plan-making threads (a finished thread stays in the table: its size is not made again)."""
    for t in list(_prewarm_threads.values()):
        if t.is_alive():
            t.join()


import atexit as _atexit      # noqa: E402
_atexit.register(join_fft_prewarm)


def last_lq_refit_count() -> int:
    """Spots the last least-squares call fitted a second time with MINPACK's summation order."""
    n = ctypes.c_int64(0)
    _lib.check(_lib.load().pmi_gausslq_last_refit_count(ctypes.byref(n)), "pmi_gausslq_last_refit_count")
    return int(n.value)


LQ_MODES = {"fast": 0, "refit": 1, "strict": 2}


def set_lq_mode(mode: str = "strict"):
    """How the sums over the residual rows of the least-squares fit run (pmi_gausslq_set_mode): "fast" = tree sums
    only; "refit" = tree sums, spots with a decision of lmdif near its threshold fitted again in MINPACK's order;
    "strict" (the library's default, and this function's) = every spot in MINPACK's order (scipy.optimize.leastsq at
    picasso/gausslq.py:240-242: the oracle's bits)."""
    if mode not in LQ_MODES:
        raise ValueError(f"unknown gausslq mode {mode!r}")
    _lib.check(_lib.load().pmi_gausslq_set_mode(LQ_MODES[mode]), "pmi_gausslq_set_mode")


def get_lq_mode() -> str:
    m = ctypes.c_int(0)
    _lib.check(_lib.load().pmi_gausslq_get_mode(ctypes.byref(m)), "pmi_gausslq_get_mode")
    return {v: k for k, v in LQ_MODES.items()}[m.value]


LQ_TIE_REASONS = ("pivot", "lmpar", "fnorm", "ratio", "ftol", "noise", "xtol", "fragile", "rounds_first_pass", "rounds_second_pass")


def last_lq_tie_reasons() -> dict:
    c = (ctypes.c_int64 * len(LQ_TIE_REASONS))()
    _lib.check(_lib.load().pmi_gausslq_last_tie_reasons(c, len(LQ_TIE_REASONS)), "pmi_gausslq_last_tie_reasons")
    return {k: int(v) for k, v in zip(LQ_TIE_REASONS, c)}


FLAG_REASONS = ("margin", "curvature", "narrow", "swing", "wild", "slow", "unstable")


def last_flag_reasons(stream=None) -> dict:
    """Of the spots the last MLE call fitted a second time, how many each criterion flagged (a spot can carry several)."""
    c = (ctypes.c_int64 * len(FLAG_REASONS))()
    _lib.check(_lib.load().pmi_mle_last_flag_reasons(c, len(FLAG_REASONS), stream), "pmi_mle_last_flag_reasons")
    return {k: int(v) for k, v in zip(FLAG_REASONS, c)}


def gaussmle_arrays(spots: np.ndarray, eps: float, max_it: int, method: str = "sigmaxy"):
    """The allocation contract of picasso/gaussmle.py:455-459."""
    if method not in _lib.MLE_METHODS:
        raise ValueError("Method not available.")
    _lib.require_gpu()
    spots = np.ascontiguousarray(spots, np.float32)
    if spots.ndim != 3 or spots.shape[1] != spots.shape[2]:
        raise ValueError("spots must have shape (N, box, box)")
    N, box, _ = spots.shape
    thetas = np.zeros((N, 6), np.float32)
    crlbs = np.full((N, 6), np.inf, np.float32)
    loglik = np.zeros(N, np.float32)
    iterations = np.zeros(N, np.int32)
    with _lib.lock():
        rc = _lib.load().pmi_gaussmle(_lib.ptr(spots), N, int(box), float(eps), int(max_it),
                                      _lib.MLE_METHODS[method], _lib.ptr(thetas), _lib.ptr(crlbs),
                                      _lib.ptr(loglik), _lib.ptr(iterations))
    _lib.check(rc, "pmi_gaussmle")
    return thetas, crlbs, loglik, iterations


def gausslq_arrays(spots: np.ndarray, full_output: bool = False):
    """theta (N,6) float32 as picasso/gausslq.py:247-268 fit_spots returns it; with
    full_output also MINPACK's info code and nfev per spot."""
    _lib.require_gpu()
    spots = np.ascontiguousarray(spots, np.float32)
    if spots.ndim != 3 or spots.shape[1] != spots.shape[2]:
        raise ValueError("spots must have shape (N, box, box)")
    N, box, _ = spots.shape
    theta = np.empty((N, 6), np.float32)
    info = np.zeros(N, np.int32)
    nfev = np.zeros(N, np.int32)
    with _lib.lock():
        rc = _lib.load().pmi_gausslq(_lib.ptr(spots), N, int(box), _lib.ptr(theta), _lib.ptr(info), _lib.ptr(nfev))
    _lib.check(rc, "pmi_gausslq")
    if full_output:
        return theta, info, nfev
    return theta


def avgroi_array(spots: np.ndarray) -> np.ndarray:
    _lib.require_gpu()
    spots = np.ascontiguousarray(spots, np.float32)
    N, box, _ = spots.shape
    theta = np.empty((N, 6), np.float32)
    theta.fill(np.nan)
    with _lib.lock():
        rc = _lib.load().pmi_avgroi(_lib.ptr(spots), N, int(box), _lib.ptr(theta))
    _lib.check(rc, "pmi_avgroi")
    return theta


def zfit_arrays(sx, sy, cx, cy):
    """-> z (before magnification) and squared calibration residual, float64."""
    _lib.require_gpu()
    sx = np.ascontiguousarray(sx, np.float32)
    sy = np.ascontiguousarray(sy, np.float32)
    cx = np.ascontiguousarray(cx, np.float64)
    cy = np.ascontiguousarray(cy, np.float64)
    if cx.shape != (7,) or cy.shape != (7,):
        raise ValueError("calibration needs 7 coefficients per axis")
    N = len(sx)
    z = np.zeros(N, np.float64)
    sq = np.zeros(N, np.float64)
    with _lib.lock():
        rc = _lib.load().pmi_zfit(_lib.ptr(sx), _lib.ptr(sy), N, _lib.ptr(cx), _lib.ptr(cy), _lib.ptr(z), _lib.ptr(sq))
    _lib.check(rc, "pmi_zfit")
    return z, sq


def _viewport(oversampling, y_min, x_min, y_max, x_max, image=True):
    """-> (the five floats as the C calls take them, (n_y, n_x) of the image by pmi_render_dims, render.py:224-225);
    a viewport without pixels raises ValueError.  ``image=False``: a call that draws nothing (``rotate_locs_arrays``)
    takes the floats alone, whatever the viewport holds.  Needs no GPU."""
    view = (float(oversampling), float(y_min), float(x_min), float(y_max), float(x_max))
    if not image:
        return view, None
    ny, nx = ctypes.c_int64(), ctypes.c_int64()
    _lib.call("pmi_render_dims", *view, ctypes.byref(ny), ctypes.byref(nx))
    if ny.value <= 0 or nx.value <= 0:
        raise ValueError("empty viewport")
    return view, (int(ny.value), int(nx.value))


def render_dims(oversampling, y_min, x_min, y_max, x_max):
    """(n_y, n_x) of a render (render.py:224-225); needs no GPU."""
    return _viewport(oversampling, y_min, x_min, y_max, x_max)[1]


def render_arrays(x, y, oversampling, y_min, x_min, y_max, x_max, lpx=None, lpy=None, min_blur_width=0.0, iso=False):
    """-> (n, image float32).  lpx/lpy None = histogram, else the Gaussian render."""
    _lib.require_gpu()
    x = np.ascontiguousarray(x, np.float32)
    y = np.ascontiguousarray(y, np.float32)
    view, (n_y, n_x) = _viewport(oversampling, y_min, x_min, y_max, x_max)
    image = np.empty((n_y, n_x), np.float32)
    n = ctypes.c_int64(0)
    with _lib.lock():
        if lpx is None:
            _lib.call("pmi_render_hist", _lib.ptr(x), _lib.ptr(y), len(x), *view, _lib.ptr(image), n_y, n_x, ctypes.byref(n))
        else:
            lpx = np.ascontiguousarray(lpx, np.float32)
            lpy = np.ascontiguousarray(lpy, np.float32)
            _lib.call("pmi_render_gaussian", _lib.ptr(x), _lib.ptr(y), _lib.ptr(lpx), _lib.ptr(lpy), len(x), *view,
                      float(min_blur_width), int(bool(iso)), _lib.ptr(image), n_y, n_x, ctypes.byref(n))
    return int(n.value), image


def xcorr_array(image_a, image_b) -> np.ndarray:
    _lib.require_gpu()
    a = np.ascontiguousarray(image_a, np.float64)
    b = np.ascontiguousarray(image_b, np.float64)
    if a.ndim != 2 or a.shape != b.shape:
        raise ValueError("images must be 2-D and of the same shape")
    out = np.empty_like(a)
    with _lib.lock():
        rc = _lib.load().pmi_xcorr(_lib.ptr(a), _lib.ptr(b), a.shape[0], a.shape[1], _lib.ptr(out))
    _lib.check(rc, "pmi_xcorr")
    return out


def _roi_arg(roi) -> int:
    """`roi` as the C calls take it: 0 for None (no crop), else the side of the centre crop.  The library reads 0 as
    "no crop", while get_image_shift with roi=0 crops to nothing or to one row (picasso/imageprocess.py:89-101), so a
    roi below 1 is refused here and never reaches the library as "no crop"."""
    if roi is None:
        return 0
    if int(roi) < 1:
        raise ValueError(f"roi must be None (no crop) or at least 1, got {roi!r}")
    return int(roi)


def rcc_pairs_arrays(segments, roi, box: int, pairs=None):
    """Pairs (i, j) of the segment images (all i < j when `pairs` is None) -> peak (n_pairs, 2),
    valid (n_pairs), fit windows (n_pairs, box, box) float64 and the crop offsets (Y_, X_)."""
    roi = _roi_arg(roi)
    _lib.require_gpu()
    seg = np.ascontiguousarray(segments, np.float64)
    if seg.ndim != 3:
        raise ValueError("segments must have shape (n, Y, X)")
    n, Y, X = seg.shape
    if pairs is None:
        pairs = [(i, j) for i in range(n - 1) for j in range(i + 1, n)]
    pairs = np.ascontiguousarray(np.asarray(pairs, np.int32).reshape(-1, 2))
    n_pairs = len(pairs)
    peak = np.zeros((n_pairs, 2), np.int32)
    valid = np.zeros(n_pairs, np.int32)
    rois = np.zeros((n_pairs, box, box), np.float64)
    crop = np.zeros(2, np.int32)
    with _lib.lock():
        rc = _lib.load().pmi_rcc_pair_list(_lib.ptr(seg), n, Y, X, roi, int(box),
                                           _lib.ptr(pairs), n_pairs, _lib.ptr(peak), _lib.ptr(valid), _lib.ptr(rois),
                                           _lib.ptr(crop))
    _lib.check(rc, "pmi_rcc_pair_list")
    return peak, valid, rois, (int(crop[0]), int(crop[1]))


def peak_fit_arrays(rois):
    """(n, box, box) float64 correlation windows -> popt (n, 5) = a, xc, yc, s, b and the termination status of the
    bounded Gaussian fit (pmi_peak_fit; scipy's curve_fit in the reference, picasso/imageprocess.py:121-141)."""
    _lib.require_gpu()
    rois = np.ascontiguousarray(rois, np.float64)
    if rois.ndim != 3 or rois.shape[1] != rois.shape[2]:
        raise ValueError("rois must have shape (n, box, box)")
    n, box, _ = rois.shape
    popt = np.zeros((n, 5), np.float64)
    status = np.zeros(n, np.int32)
    with _lib.lock():
        rc = _lib.load().pmi_peak_fit(_lib.ptr(rois), n, int(box), _lib.ptr(popt), _lib.ptr(status))
    _lib.check(rc, "pmi_peak_fit")
    return popt, status


def rcc_shifts_arrays(segments, roi, box: int, pairs=None):
    """get_image_shift (picasso/imageprocess.py:53-161) for pairs (i, j) of the segment images (all i < j when
    `pairs` is None), entirely on the device -> shifts (n_pairs, 2) = (-yc, -xc), fit status (n_pairs)."""
    roi = _roi_arg(roi)
    _lib.require_gpu()
    seg = np.ascontiguousarray(segments, np.float64)
    if seg.ndim != 3:
        raise ValueError("segments must have shape (n, Y, X)")
    n, Y, X = seg.shape
    if pairs is None:
        pairs = [(i, j) for i in range(n - 1) for j in range(i + 1, n)]
    pairs = np.ascontiguousarray(np.asarray(pairs, np.int32).reshape(-1, 2))
    n_pairs = len(pairs)
    shifts = np.zeros((n_pairs, 2), np.float64)
    status = np.zeros(n_pairs, np.int32)
    with _lib.lock():
        rc = _lib.load().pmi_rcc_shifts(_lib.ptr(seg), n, Y, X, roi, int(box), _lib.ptr(pairs),
                                        n_pairs, _lib.ptr(shifts), _lib.ptr(status))
    _lib.check(rc, "pmi_rcc_shifts")
    return shifts, status


class DeviceMovie:
    """A movie resident in HBM (pmi_malloc), for repeated calls without H2D."""

    def __init__(self, movie: np.ndarray):
        _lib.require_gpu()
        movie = as_movie_array(movie)
        self.capacity = max(movie.nbytes, 1)
        self._ptr = ctypes.c_void_p()
        _lib.check(_lib.load().pmi_malloc(ctypes.byref(self._ptr), self.capacity), "pmi_malloc")
        self.load(movie)

    def load(self, movie: np.ndarray):
        """Upload another stack of frames into the same allocation (it must fit)."""
        movie = as_movie_array(movie)
        if movie.nbytes > self.capacity:
            raise ValueError("DeviceMovie.load: stack larger than the allocation")
        self.shape = movie.shape
        self.dtype = movie.dtype
        self.nbytes = movie.nbytes
        _lib.check(_lib.load().pmi_memcpy_h2d(self._ptr, _lib.ptr(movie), self.nbytes), "pmi_memcpy_h2d")

    @property
    def ptr(self):
        return self._ptr

    def free(self):
        if self._ptr:
            _lib.load().pmi_free(self._ptr)
            self._ptr = ctypes.c_void_p()

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class DeviceWorkspace:
    """Grow-only device buffers of the fused pipelines (table + row count), kept across submissions so that a
    chunked run does not allocate and free per chunk (hipFree waits for the whole device, uploads included)."""

    def __init__(self):
        self._table = ctypes.c_void_p()
        self._bytes = 0
        self._dn = ctypes.c_void_p()

    def table(self, nbytes: int):
        L = _lib.load()
        if nbytes > self._bytes:
            if self._table:
                L.pmi_free(self._table)
                self._table, self._bytes = ctypes.c_void_p(), 0
            want = nbytes + nbytes // 4
            _lib.check(L.pmi_malloc(ctypes.byref(self._table), want), "pmi_malloc")
            self._bytes = want
        return self._table

    def count(self):
        if not self._dn:
            _lib.check(_lib.load().pmi_malloc(ctypes.byref(self._dn), 8), "pmi_malloc")
        return self._dn

    def free(self):
        L = _lib.load()
        if self._table:
            L.pmi_free(self._table)
        if self._dn:
            L.pmi_free(self._dn)
        self._table, self._bytes, self._dn = ctypes.c_void_p(), 0, ctypes.c_void_p()


class DeviceStream:
    """A non-blocking HIP stream of the library (pmi_stream_create)."""

    def __init__(self):
        self.handle = ctypes.c_void_p()
        _lib.check(_lib.load().pmi_stream_create(ctypes.byref(self.handle)), "pmi_stream_create")

    def destroy(self):
        if self.handle:
            _lib.load().pmi_stream_destroy(self.handle)
            self.handle = ctypes.c_void_p()


def _localize_device(call, columns, d_movie_ptr, dtype, shape, roi, frame_bounds, cap, stream, f_lo, f_hi, work=None):
    """Shared driver of the fused pipelines: allocate the table (or take it from `work`), submit, grow on
    overflow, copy the columns back (on `stream` when one is given, so that nothing orders against the
    default stream)."""
    _lib.require_gpu()
    L = _lib.load()
    F, Y, X = shape
    r = normalise_roi(roi, Y, X)
    lo, hi = frame_range(frame_bounds, F)
    if f_lo is not None:
        lo = max(lo, f_lo)
    if f_hi is not None:
        hi = min(hi, f_hi)
    cap = int(cap or max(4096, 256 * F))
    ncol = len(columns)
    own = work is None
    ws = DeviceWorkspace() if own else work

    def fetch(dst, src, nbytes):
        if stream is None:
            _lib.check(L.pmi_memcpy_d2h(_lib.ptr(dst), src, nbytes), "d2h")
        else:
            _lib.check(L.pmi_memcpy_d2h_async(_lib.ptr(dst), src, nbytes, stream), "d2h")

    try:
        while True:
            table = ws.table(ncol * cap * 4)
            dn = ws.count()
            n = np.zeros(1, np.int64)
            with _lib.lock():
                call(L, d_movie_ptr, dtype_code(dtype), F, Y, X, r, lo, hi, table, cap, dn, stream)
                fetch(n, dn, 8)
                _lib.check(L.pmi_stream_synchronize(stream), "sync")
            n = int(n[0])
            if n > cap:
                cap = n
                continue
            out = {}
            for c, (name, dt) in enumerate(columns):
                out[name] = np.empty(n, dt)
                if n:
                    fetch(out[name], ctypes.c_void_p(table.value + c * cap * 4), n * 4)
            if stream is not None and n:
                _lib.check(L.pmi_stream_synchronize(stream), "sync")
            return out
    finally:
        if own:
            ws.free()


def localize_mle_device(d_movie_ptr, dtype, shape, box, min_ng, camera, eps=1e-3, max_it=100,
                        method="sigmaxy", roi=None, frame_bounds=None, cap=None, stream=None,
                        f_lo=None, f_hi=None, work=None):
    """identify -> fused cut+fit -> table on a resident movie.  Returns a dict of
    numpy columns (LOC_COLUMNS).  d_movie_ptr: int / c_void_p device address."""
    def call(L, d_movie, code, F, Y, X, r, lo, hi, table, cap_, dn, stream_):
        rc = L.pmi_localize_mle_dev(d_movie, code, F, Y, X, int(box), float(min_ng), _lib.ptr(r), lo, hi,
                                    float(camera["Baseline"]), float(camera["Sensitivity"]), float(camera["Gain"]),
                                    float(eps), int(max_it), _lib.MLE_METHODS[method], table, cap_, dn, stream_)
        _lib.check(rc, "pmi_localize_mle_dev")
    return _localize_device(call, LOC_COLUMNS, d_movie_ptr, dtype, shape, roi, frame_bounds, cap, stream, f_lo, f_hi, work)


def localize_lq_device(d_movie_ptr, dtype, shape, box, min_ng, camera, roi=None, frame_bounds=None, cap=None,
                       stream=None, f_lo=None, f_hi=None, work=None):
    """identify -> fused cut + least-squares fit -> 11-column table (LQ_COLUMNS)."""
    em = int(camera["Gain"] > 1)

    def call(L, d_movie, code, F, Y, X, r, lo, hi, table, cap_, dn, stream_):
        rc = L.pmi_localize_lq_dev(d_movie, code, F, Y, X, int(box), float(min_ng), _lib.ptr(r), lo, hi,
                                   float(camera["Baseline"]), float(camera["Sensitivity"]), float(camera["Gain"]),
                                   em, table, cap_, dn, stream_)
        _lib.check(rc, "pmi_localize_lq_dev")
    return _localize_device(call, LQ_COLUMNS, d_movie_ptr, dtype, shape, roi, frame_bounds, cap, stream, f_lo, f_hi, work)


# ---- what the row-table wrappers below share: residence, type codes, columns, descriptor tables ----
def _stream(device) -> int:
    """The stream of `device` current in the calling thread, as the library takes it."""
    import torch
    return torch.cuda.current_stream(device).cuda_stream


def _out(device, dtype, n, *tail, zero: bool = False):
    """A device output of n entries (each of shape `tail`): the allocation is never empty, what comes back is its first
    n entries.  `_dptr` hands the library the allocation even where n is 0."""
    import torch
    return (torch.zeros if zero else torch.empty)((max(int(n), 1),) + tail, dtype=dtype, device=device)[:int(n)]


def _dptr(t):
    """void* of a device tensor (None stays None).  torch gives an empty tensor the address 0; an empty slice gets the
    start of its allocation instead, which is its own address only at offset 0: that is what `_out` returns, and an
    empty slice further into a buffer must not come here."""
    return None if t is None else ctypes.c_void_p(t.data_ptr() or t.untyped_storage().data_ptr())


# The two code tables are data: (what the TypeError names, dtype -> code).  The C enums differ and stay.
LINK_F32, LINK_F64, LINK_U32, LINK_U64 = 0, 1, 2, 3
CENTERS_F32, CENTERS_F64, CENTERS_U32, CENTERS_I32, CENTERS_U64, CENTERS_I64 = 0, 1, 2, 3, 4, 5
_LINK_TYPES = ("link / NeNA", {
    np.dtype("float32"): LINK_F32, np.dtype("float64"): LINK_F64, np.dtype("uint32"): LINK_U32,
    np.dtype("int32"): LINK_U32, np.dtype("uint64"): LINK_U64, np.dtype("int64"): LINK_U64})
_CENTERS_TYPES = ("the cluster centers", {
    np.dtype("float32"): CENTERS_F32, np.dtype("float64"): CENTERS_F64, np.dtype("uint32"): CENTERS_U32,
    np.dtype("int32"): CENTERS_I32, np.dtype("uint64"): CENTERS_U64, np.dtype("int64"): CENTERS_I64})


def _type_code(types, dtype, floating: bool = False) -> int:
    """The code of a NumPy or torch dtype in one of the two tables; `floating` refuses the integers."""
    what, codes = types
    if isinstance(dtype, np.dtype):
        dt = dtype
    else:
        dt = np.dtype(str(dtype)[6:] if type(dtype).__module__ == "torch" else dtype)
    if dt not in codes or (floating and dt.kind != "f"):
        raise TypeError(f"unsupported column dtype {dt} for {what} on the device")
    return codes[dt]


def link_type(dtype, floating: bool = False) -> int:
    return _type_code(_LINK_TYPES, dtype, floating)


def centers_type(dtype, floating: bool = False) -> int:
    return _type_code(_CENTERS_TYPES, dtype, floating)


def _to_device(a, dtype=None):
    """One host column -> a device tensor (integer columns widened on the host)."""
    import torch
    a = np.ascontiguousarray(a if dtype is None else np.asarray(a).astype(dtype, copy=False))
    if a.dtype == np.uint32:
        return torch.from_numpy(a.view(np.int32)).cuda()
    if a.dtype == np.uint64:
        return torch.from_numpy(a.view(np.int64)).cuda()
    return torch.from_numpy(a).cuda()


def _index_column(a, what: str):
    """A label, frame or offset column as the device takes it: any integer or bool column, widened to int64."""
    a = np.asarray(a)
    if a.dtype.kind not in "iub":
        raise TypeError(f"{what} must be an integer column, not {a.dtype}")
    return a.astype(np.int64, copy=False)


def _centers_column(a, what: str) -> np.ndarray:
    """A table column as the device takes it: bool and the narrow integers widened (to a type pandas would convert
    to float64 all the same), float16 refused."""
    a = np.asarray(a)
    if a.dtype.kind == "b" or (a.dtype.kind in "iu" and a.dtype.itemsize < 4):
        a = a.astype(np.int32 if a.dtype.kind != "u" else np.uint32)
    if a.ndim != 1:
        raise ValueError(f"{what} must be a column, not an array of shape {a.shape}")
    centers_type(a.dtype)
    return a


def _float_column(a):
    """A float32 / float64 column, host or device -> (device tensor, LINK type code)."""
    import torch
    if isinstance(a, torch.Tensor):
        if a.dtype not in (torch.float32, torch.float64) or a.dim() != 1 or not a.is_cuda:
            raise TypeError("a device column must be a 1-D float32 or float64 tensor on the GPU")
        return a.contiguous(), link_type(a.dtype)
    a = np.asarray(a)
    return _to_device(a), link_type(a.dtype, True)


def _check_points(X: np.ndarray) -> np.ndarray:
    if X.ndim != 2 or X.shape[1] not in (2, 3):
        raise ValueError(f"points must have shape (n, 2) or (n, 3), not {X.shape}")
    return X


def _check_rows(n: int, message: str, *columns) -> None:
    """The one length check: every column has n entries."""
    if any(len(c) != n for c in columns):
        raise ValueError(message)


_PER_ROW = "every column must have one entry per row of the table"


class _Uploads(dict):
    """One upload per host column of a table of n rows, however many calls read it."""

    def __init__(self, n: int):
        super().__init__()
        self.n = int(n)

    def column(self, a):
        # two views of one column are one upload; a shorter view of it is another column, and is refused below
        key = (a.__array_interface__["data"][0], a.shape, a.strides, a.dtype.str)
        if key not in self:
            _check_rows(self.n, _PER_ROW, a)
            self[key] = (a, _to_device(a))
        return self[key][1]


class _Table:
    """The descriptor table of one statistics call.  `rows` holds one tuple per descriptor in the field order of the
    ctypes structure `struct`: a device tensor (or None) for a pointer field, a code for an integer one.  The table
    references every tensor it points to, so the caller keeps the table until the call has returned and reads the
    outputs from `rows`."""

    def __init__(self, struct, rows):
        self.rows = rows
        self.array = (struct * max(len(rows), 1))(*[
            struct(*[f if f is None or type(f) is int else f.data_ptr() for f in row]) for row in rows])
        self.ptr, self.count = ctypes.cast(self.array, ctypes.c_void_p), len(rows)

    @classmethod
    def chunks(cls, struct, rows, limit: int):
        """One table per `limit` rows, for a call that takes no more descriptors at a time."""
        return [cls(struct, rows[lo:lo + limit]) for lo in range(0, len(rows), limit)]


# ---- AIM undrift: intersection counts (csrc/aim.hip, picasso/aim.py:517-773) ----
AIM_XY_F32, AIM_XY_F64, AIM_Z_F32, AIM_Z_F64 = 0, 1, 2, 3


def aim_partition(d_frame, seg_len: int, n_frames: int):
    """Rows of a resident int64 frame column (numbered from 1) grouped by AIM segment on the device ->
    (d_rows int32 tensor, host offsets of ceil(n_frames / seg_len) + 1 entries)."""
    import torch
    n = int(d_frame.numel())
    n_seg = -(-int(n_frames) // int(seg_len)) if n_frames > 0 else 0
    rows = torch.empty(max(n, 1), dtype=torch.int32, device=d_frame.device)
    offsets = np.zeros(n_seg + 1, np.int64)
    with _lib.lock():
        _lib.call("pmi_aim_partition_dev", ctypes.c_void_p(d_frame.data_ptr()), n, int(seg_len), int(n_frames),
                  ctypes.c_void_p(rows.data_ptr()), _lib.ptr(offsets), ctypes.c_void_p(_stream(d_frame.device)))
    return rows, offsets


class AimTable:
    """The reference keys of one AIM round, counted once on the device (pmi_aim_table_create_dev); `count` gives the
    roi_cc of one segment of target rows of the same resident columns."""

    def __init__(self, mode, x, y, z, ref_rows, n_ref, intersect_d, width_units, height_units, shifts):
        import torch
        self.mode, self.x, self.y, self.z = int(mode), x, y, z
        self.shifts = np.ascontiguousarray(shifts, np.int32 if mode in (AIM_XY_F32, AIM_XY_F64) else np.float64)
        self.n_shifts = int(self.shifts.size)
        self.device, self.stream = x.device, _stream(x.device)
        self.out = torch.zeros(self.n_shifts + 1, dtype=torch.int32, device=self.device)
        self._h = ctypes.c_void_p()
        with _lib.lock():
            _lib.call("pmi_aim_table_create_dev", self.mode, _dptr(x), _dptr(y), _dptr(z), _dptr(ref_rows), int(n_ref),
                      float(intersect_d), float(width_units), float(height_units), _lib.ptr(self.shifts), self.n_shifts,
                      ctypes.byref(self._h), ctypes.c_void_p(self.stream))

    def info(self):
        dense, entries = ctypes.c_int(0), ctypes.c_int64(0)
        _lib.call("pmi_aim_table_info", self._h, ctypes.byref(dense), ctypes.byref(entries))
        return ("dense" if dense.value else "sorted"), int(entries.value)

    def count(self, rows, rel_x=0.0, rel_y=0.0, rel_z=0.0) -> np.ndarray:
        """int64 roi_cc of the target rows `rows` (an int32 device tensor) shifted by rel; one D2H of n_shifts + 1 ints."""
        with _lib.lock():
            _lib.call("pmi_aim_count_dev", self._h, _dptr(self.x), _dptr(self.y), _dptr(self.z), _dptr(rows),
                      int(rows.numel()), float(rel_x), float(rel_y), float(rel_z), _dptr(self.out),
                      ctypes.c_void_p(self.stream))
            h = self.out.cpu().numpy()
        if h[-1]:
            raise _lib.HipBackendError(f"pmi_aim_count_dev: status {int(h[-1])} (target hash overflow)")
        return h[:-1].astype(np.int64)

    def close(self):
        if self._h:
            _lib.load().pmi_aim_table_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def aim_set_dense_limit(entries: int) -> None:
    """Spans of more target-counter entries than this take the sorted table form (default 2**28)."""
    _lib.call("pmi_aim_set_dense_limit", int(entries))


def aim_roi_cc_arrays(mode, ref, target, rel, intersect_d, width_units, height_units, shifts) -> np.ndarray:
    """roi_cc of one segment from host columns (pmi_aim_roi_cc): ref / target = (x, y[, z]) in the dtypes of `mode`."""
    _lib.require_gpu()
    xy_t = np.float32 if mode == AIM_XY_F32 else np.float64
    z_t = np.float32 if mode == AIM_Z_F32 else np.float64
    zmode = mode in (AIM_Z_F32, AIM_Z_F64)

    def cols(c):
        out = [np.ascontiguousarray(c[0], xy_t), np.ascontiguousarray(c[1], xy_t)]
        out.append(np.ascontiguousarray(c[2], z_t) if zmode else None)
        return out
    r, t = cols(ref), cols(target)
    sh = np.ascontiguousarray(shifts, np.float64 if zmode else np.int32)
    out = np.zeros(sh.size, np.int64)
    rel = tuple(rel) + (0.0,) * (3 - len(rel))
    with _lib.lock():
        _lib.call("pmi_aim_roi_cc", int(mode), _lib.ptr(r[0]), _lib.ptr(r[1]), _lib.ptr(r[2]), len(r[0]), _lib.ptr(t[0]),
                  _lib.ptr(t[1]), _lib.ptr(t[2]), len(t[0]), float(rel[0]), float(rel[1]), float(rel[2]),
                  float(intersect_d), float(width_units), float(height_units), _lib.ptr(sh), int(sh.size), _lib.ptr(out))
    return out


# ---- link and NeNA (csrc/link.hip, picasso/postprocess.py:2441-2661, :1212-1272) ----
LINK_SUM, LINK_WSUM, LINK_XWSUM = 0, 1, 2


class _LinkColumn(ctypes.Structure):
    _fields_ = [("data", ctypes.c_void_p), ("weight", ctypes.c_void_p), ("out", ctypes.c_void_p),
                ("op", ctypes.c_int32), ("type", ctypes.c_int32), ("w_type", ctypes.c_int32)]


class LinkTable:
    """frame, x, y, group of a table sorted by frame, sent to the device once (frame / group widened to int64 on
    the host; x / y stay float32 or float64, each on its own)."""

    def __init__(self, frame, x, y, group):
        _lib.require_gpu()
        x, y = np.asarray(x), np.asarray(y)
        self.n = int(len(x))
        _check_rows(self.n, "frame, x, y and group must have one length", frame, y, group)
        self.x_type, self.y_type = link_type(x.dtype, True), link_type(y.dtype, True)
        self.frame = _to_device(_index_column(frame, "frame"))
        self.group = _to_device(_index_column(group, "group"))
        self.x, self.y = _to_device(x), _to_device(y)
        self.device, self.stream = self.x.device, _stream(self.x.device)

    def frame_index(self, k: int):
        """(lo, hi) int32 device tensors of pmi_link_frame_index_dev."""
        import torch
        lo, hi = _out(self.device, torch.int32, self.n), _out(self.device, torch.int32, self.n)
        with _lib.lock():
            _lib.call("pmi_link_frame_index_dev", _dptr(self.frame), self.n, int(k), _dptr(lo), _dptr(hi),
                      ctypes.c_void_p(self.stream))
        return lo, hi

    def link_groups(self, r2: float, k: int):
        """-> (int32 device tensor link_group, number of groups)."""
        import torch
        out = _out(self.device, torch.int32, self.n)
        n_groups = ctypes.c_int64(0)
        with _lib.lock():
            _lib.call("pmi_link_groups_dev", _dptr(self.frame), _dptr(self.x), self.x_type, _dptr(self.y), self.y_type,
                      _dptr(self.group), self.n, float(r2), int(k), _dptr(out), ctypes.byref(n_groups),
                      ctypes.c_void_p(self.stream))
        return out, int(n_groups.value)

    def nena_hist(self, d_max: float, bin_size: float, n_bins: int) -> np.ndarray:
        """int64 counts of the next-frame neighbour distance histogram."""
        import torch
        hist = torch.zeros(int(n_bins), dtype=torch.int64, device=self.device)
        with _lib.lock():
            _lib.call("pmi_nena_hist_dev", _dptr(self.frame), _dptr(self.x), self.x_type, _dptr(self.y), self.y_type,
                      _dptr(self.group), self.n, float(d_max), float(bin_size), int(n_bins), _dptr(hist),
                      ctypes.c_void_p(self.stream))
            return hist.cpu().numpy()


def link_combine(link_group, n_groups: int, frame, columns):
    """Per link group: count, min / max frame, last row and the ordered sums of `columns`, a list of
    (op, data, weight) with host columns (None where the op does not read one).
    -> (uint32 count, int64 first, int64 last, int32 last_row, [sum arrays])."""
    import torch
    _lib.require_gpu()
    n, G = int(len(link_group)), int(n_groups)
    d_lg = link_group if isinstance(link_group, torch.Tensor) else _to_device(np.asarray(link_group, np.int32))
    dev = d_lg.device
    d_frame = None if frame is None else _to_device(_index_column(frame, "frame"))
    uploads, rows, out_dts = _Uploads(n), [], []
    for op, data, weight in columns:
        ta = link_type(data.dtype, op == LINK_XWSUM) if data is not None else 0
        tw = link_type(weight.dtype, True) if weight is not None else 0
        if op == LINK_SUM:
            out_dt = data.dtype
        elif op == LINK_WSUM:
            out_dt = weight.dtype
        else:
            out_dt = np.promote_types(data.dtype, weight.dtype)
        out_dts.append(np.dtype(out_dt))
        rows.append((None if data is None else uploads.column(data), None if weight is None else uploads.column(weight),
                     _to_device(np.zeros(max(G, 1), out_dt)), int(op), ta, tw))
    table = _Table(_LinkColumn, rows)
    count = _out(dev, torch.int32, G, zero=True)
    first, last = _out(dev, torch.int64, G, zero=True), _out(dev, torch.int64, G, zero=True)
    last_row = _out(dev, torch.int32, G, zero=True)
    with _lib.lock():
        _lib.call("pmi_link_combine_dev", _dptr(d_lg), n, G, _dptr(d_frame), table.ptr, table.count, _dptr(count),
                  _dptr(first) if d_frame is not None else None, _dptr(last) if d_frame is not None else None,
                  _dptr(last_row), ctypes.c_void_p(_stream(dev)))
        sums = [row[2].cpu().numpy().view(dt)[:G] for row, dt in zip(table.rows, out_dts)]
        res = (count.cpu().numpy().view(np.uint32), first.cpu().numpy(), last.cpu().numpy(), last_row.cpu().numpy())
    return res + (sums,)


# ---- DBSCAN and the SMLM clusterer (csrc/cluster.hip, picasso/clusterer.py:34-201, :410-445) ----
class ClusterPoints:
    """The points of a clustering call, sent to the device once: an (n, 2 | 3) array, widened to float64 as the
    reference's KDTree and sklearn do, one column per dimension, with the corners the cells are counted from."""

    def __init__(self, X):
        import torch
        _lib.require_gpu()
        X = _check_points(np.asarray(X))
        self.n, self.dims = int(X.shape[0]), int(X.shape[1])
        cols = np.ascontiguousarray(X.T, np.float64)
        if self.n:
            self.lo, self.hi = np.ascontiguousarray(cols.min(axis=1)), np.ascontiguousarray(cols.max(axis=1))
        else:
            self.lo = self.hi = np.zeros(self.dims)
        self.X = torch.from_numpy(cols).cuda()
        self.device, self.stream = self.X.device, _stream(self.X.device)

    def _row_out(self):
        import torch
        return _out(self.device, torch.int32, self.n)

    def _head(self, radius):
        r = float(radius)
        return (_dptr(self.X), self.dims, self.n, _lib.ptr(self.lo), _lib.ptr(self.hi), r, r * r)

    def counts(self, radius) -> np.ndarray:
        """int32 neighbour count of every row (itself included)."""
        out = self._row_out()
        with _lib.lock():
            _lib.call("pmi_cluster_counts_dev", *self._head(radius), _dptr(out), ctypes.c_void_p(self.stream))
            return out.cpu().numpy()

    def smlm(self, radius, min_locs: int, frame=None, fa_lo=0.0, fa_hi=0.0, fa_edges=None) -> np.ndarray:
        """int32 labels of the SMLM clusterer; `frame` (any integer column) adds the frame analysis."""
        out = self._row_out()
        d_frame = None if frame is None else _to_device(_index_column(frame, "frame"))
        edges = None if fa_edges is None else np.ascontiguousarray(fa_edges, np.float64)
        if d_frame is not None and (edges is None or edges.size != 21 or len(frame) != self.n):
            raise ValueError("frame analysis needs one frame per row and 21 bin edges")
        with _lib.lock():
            _lib.call("pmi_cluster_smlm_dev", *self._head(radius), int(min_locs), _dptr(d_frame), float(fa_lo),
                      float(fa_hi), _lib.ptr(edges), _dptr(out), ctypes.c_void_p(self.stream))
            return out.cpu().numpy()

    def dbscan(self, radius, min_samples: int, min_locs: int) -> np.ndarray:
        """int32 DBSCAN labels, clusters of fewer than `min_locs` rows already -1."""
        out = self._row_out()
        with _lib.lock():
            _lib.call("pmi_cluster_dbscan_dev", *self._head(radius), int(min_samples), int(min_locs), _dptr(out),
                      ctypes.c_void_p(self.stream))
            return out.cpu().numpy()


def cluster_frame_analysis(ids, frame, n_ids: int, fa_lo: float, fa_hi: float, fa_edges) -> np.ndarray:
    """int32 pass flag of every id < n_ids (pmi_cluster_frame_analysis_dev); `ids` int32 per row, `frame` integers."""
    import torch
    _lib.require_gpu()
    d_ids = _to_device(np.asarray(ids, np.int32))
    d_frame = _to_device(_index_column(frame, "frame"))
    edges = np.ascontiguousarray(fa_edges, np.float64)
    if edges.size != 21 or len(ids) != len(frame):
        raise ValueError("frame analysis needs one frame per row and 21 bin edges")
    passed = _out(d_ids.device, torch.int32, n_ids).fill_(1)
    with _lib.lock():
        _lib.call("pmi_cluster_frame_analysis_dev", _dptr(d_ids), _dptr(d_frame), len(ids), int(n_ids), float(fa_lo),
                  float(fa_hi), _lib.ptr(edges), _dptr(passed), ctypes.c_void_p(_stream(d_ids.device)))
        return passed.cpu().numpy()


# ---- local density and the distance histogram (csrc/pairs.hip, picasso/postprocess.py:37-204, :960-999, :1543-1579) ----
class BlockTable:
    """A table in the block order of the reference's get_index_blocks: the uint32 block indices go to the device once
    and are sorted there (pmi_pairs_order_dev); `rows` is then np.lexsort([x_index, y_index]) and `p` the sorted
    position at which the reference's block table stops filling (n when every row lies inside the K x L grid)."""

    def __init__(self, x_index, y_index, K: int, L: int):
        _lib.require_gpu()
        x_index, y_index = np.asarray(x_index), np.asarray(y_index)
        if x_index.dtype != np.uint32 or y_index.dtype != np.uint32 or x_index.shape != y_index.shape or x_index.ndim != 1:
            raise TypeError("x_index and y_index must be uint32 arrays of one length")
        self.n, self.K, self.L = int(len(x_index)), int(K), int(L)
        self._order(_to_device(x_index), _to_device(y_index))

    @classmethod
    def from_device(cls, d_x_index, d_y_index, K: int, L: int):
        """The same over uint32 indices already on the device (int32 tensors holding their bits)."""
        self = cls.__new__(cls)
        self.n, self.K, self.L = int(len(d_x_index)), int(K), int(L)
        self._order(d_x_index, d_y_index)
        return self

    def _order(self, d_xi, d_yi):
        import torch
        self.device, self.stream = d_xi.device, _stream(d_xi.device)
        self.rows = _out(self.device, torch.int32, self.n)
        self.keys = _out(self.device, torch.int64, self.n)
        p = ctypes.c_int64(0)
        with _lib.lock():
            _lib.call("pmi_pairs_order_dev", _dptr(d_xi), _dptr(d_yi), self.n, self.K, self.L, _dptr(self.rows),
                      _dptr(self.keys), ctypes.byref(p), ctypes.c_void_p(self.stream))
        self.p = int(p.value)

    def order(self) -> np.ndarray:
        """The int64 permutation into block order."""
        return self.rows.cpu().numpy().astype(np.int64)

    def _columns(self, x, y):
        """x / y of the table's rows, host arrays or device tensors -> (d_x, x type code, d_y, y type code)."""
        d_x, tx = _float_column(x)
        d_y, ty = _float_column(y)
        _check_rows(self.n, "x and y must have one entry per row of the table", d_x, d_y)
        return d_x, tx, d_y, ty

    def density(self, x, y, r2: float) -> np.ndarray:
        """uint32 neighbour count of every row, in block order; x / y in the caller's row order."""
        import torch
        d_x, tx, d_y, ty = self._columns(x, y)
        out = _out(self.device, torch.int32, self.n, zero=True)
        with _lib.lock():
            _lib.call("pmi_pairs_density_dev", _dptr(d_x), tx, _dptr(d_y), ty, _dptr(self.rows), _dptr(self.keys), self.n,
                      self.p, self.K, self.L, float(r2), _dptr(out), ctypes.c_void_p(self.stream))
            return out.cpu().numpy().view(np.uint32)

    def distance_hist(self, x, y, r_max: float, r2: float, bin_size: float, n_bins: int) -> np.ndarray:
        """uint64 counts of the distance histogram."""
        import torch
        d_x, tx, d_y, ty = self._columns(x, y)
        hist = _out(self.device, torch.int64, n_bins, zero=True)
        with _lib.lock():
            _lib.call("pmi_pairs_distance_hist_dev", _dptr(d_x), tx, _dptr(d_y), ty, _dptr(self.rows), _dptr(self.keys),
                      self.n, self.p, self.K, self.L, float(r_max), float(r2), float(bin_size), int(n_bins), _dptr(hist),
                      ctypes.c_void_p(self.stream))
            return hist.cpu().numpy().view(np.uint64)


# ---- picked localizations (csrc/picks.hip, picasso/postprocess.py:207-473, picasso/lib.py:1884-2004) ----
PICK_SQUARE, PICK_RECTANGLE, PICK_POLYGON = 0, 1, 2
PICK_MAX_CELLS = 1 << 14          # cells per axis of the grid the box shapes are binned on
_PICK_FAR = 8e307                 # bounds are clipped here so that the grid's extent stays finite


def _grid_blocks(a):
    """Block indices of picks or grid points as the kernel takes them: int64, clipped so that index + 1 cannot overflow
    (any index beyond [-1, 2^32] names no block of the grid; a Python integer too large for int64 is one of them)."""
    a = np.asarray(a)
    if a.dtype == object:
        a = np.array([min(max(int(b), -2), 1 << 33) for b in a], np.int64)
    return np.clip(_index_column(a, "block indices"), -2, 1 << 33)


def _picks_csr(name: str, head, n_picks: int, device, stream):
    """The two passes of the pick call `name`, whose arguments begin with `head` and end with the CSR outputs and the
    stream: count (offsets and the total, the one copy to the host), then write."""
    import torch
    offsets = torch.zeros(n_picks + 1, dtype=torch.int64, device=device)
    total = ctypes.c_int64(0)
    _lib.call(name, *head, _dptr(offsets), None, 0, ctypes.byref(total), stream)
    rows = _out(device, torch.int32, total.value)
    if total.value:
        _lib.call(name, *head, _dptr(offsets), _dptr(rows), int(total.value), None, stream)
    return offsets.cpu().numpy(), rows.cpu().numpy().astype(np.int64)


def picks_circle(table: "BlockTable", x, y, pick_x, pick_y, block_x, block_y, flags, r2: float):
    """Members of circular picks over a table in block order (``table`` built from uint32(x / r), uint32(y / r) of the
    same rows) -> (int64 offsets[P + 1], int64 rows): per pick the rows with dx ** 2 + dy ** 2 < r2 of the blocks around
    (block_y, block_x), in block order.  ``flags``: numba's typing of each pick, see pmi_picks_circle_dev."""
    _lib.require_gpu()
    d_x, tx, d_y, ty = table._columns(x, y)
    P = len(pick_x)
    if not (len(pick_y) == len(block_x) == len(block_y) == len(flags) == P):
        raise ValueError("one coordinate pair, block pair and flag per pick")
    if P == 0:
        return np.zeros(1, np.int64), np.zeros(0, np.int64)
    d_px, d_py = _to_device(pick_x, np.float64), _to_device(pick_y, np.float64)
    d_bx, d_by = _to_device(_grid_blocks(block_x)), _to_device(_grid_blocks(block_y))
    d_f = _to_device(flags, np.uint8)
    head = (_dptr(d_x), tx, _dptr(d_y), ty, _dptr(table.rows), _dptr(table.keys), table.n, table.p, table.K, table.L,
            _dptr(d_px), _dptr(d_py), _dptr(d_bx), _dptr(d_by), _dptr(d_f), P, float(r2))
    with _lib.lock():
        return _picks_csr("pmi_picks_circle_dev", head, P, table.device, ctypes.c_void_p(table.stream))


def _pick_grid(bounds, flags, tx: int, ty: int):
    """The grid the rows are binned on: it covers every pick's box as the rows are held against it (a weak bound of a
    float32 column is rounded to float32), with cells of half the mean box side, at most PICK_MAX_CELLS per axis."""
    eff = np.array(bounds, np.float64).reshape(-1, 4)
    flags = np.asarray(flags, np.uint8)
    for b in range(4):
        if (tx if b < 2 else ty) == LINK_F32:
            weak = (flags >> b) & 1 == 1
            with np.errstate(over="ignore"):
                eff[weak, b] = eff[weak, b].astype(np.float32).astype(np.float64)
    eff = np.clip(eff, -_PICK_FAR, _PICK_FAR)           # NaN stays NaN
    ok = (eff[:, 0] < eff[:, 1]) & (eff[:, 2] < eff[:, 3])
    if not ok.any():
        return 0.0, 0.0, 1.0, 1.0, 1.0, 1, 1
    e = eff[ok]
    x0, x1, y0, y1 = float(e[:, 0].min()), float(e[:, 1].max()), float(e[:, 2].min()), float(e[:, 3].max())
    extent = max(x1 - x0, y1 - y0)
    with np.errstate(over="ignore"):
        cell = 0.5 * float(np.mean(np.r_[e[:, 1] - e[:, 0], e[:, 3] - e[:, 2]]))
    cell = max(cell, extent / PICK_MAX_CELLS)
    if not (np.isfinite(cell) and cell > 0):
        cell = extent
    CX = min(int((x1 - x0) / cell) + 1, PICK_MAX_CELLS + 1)
    CY = min(int((y1 - y0) / cell) + 1, PICK_MAX_CELLS + 1)
    return x0, y0, x1, y1, cell, CX, CY


def _picks_shape(shape: int, x, y, bounds, flags, corner_offsets=None, corner_x=None, corner_y=None):
    import torch
    _lib.require_gpu()
    d_x, tx = _float_column(x)
    d_y, ty = _float_column(y)
    n = len(d_x)
    _check_rows(n, "x and y must have one length", d_y)
    bounds = np.ascontiguousarray(bounds, np.float64).reshape(-1, 4)
    flags = np.ascontiguousarray(flags, np.uint8)
    P = len(bounds)
    _check_rows(P, "one flag byte per pick", flags)
    if P == 0:
        return np.zeros(1, np.int64), np.zeros(0, np.int64)
    n_corners = 0
    d_co = d_cx = d_cy = None
    if shape != PICK_SQUARE:
        corner_offsets = np.ascontiguousarray(corner_offsets, np.int32)
        corner_x, corner_y = np.ascontiguousarray(corner_x, np.float64), np.ascontiguousarray(corner_y, np.float64)
        n_corners = len(corner_x)
        if len(corner_offsets) != P + 1 or len(corner_y) != n_corners or corner_offsets[0] != 0 or \
                corner_offsets[-1] != n_corners or (np.diff(corner_offsets) < 0).any():
            raise ValueError("corner_offsets must be the P + 1 ascending offsets of the corner arrays")
        if shape == PICK_RECTANGLE and (np.diff(corner_offsets) != 4).any():
            raise ValueError("a rectangle has four corners")
        d_co = _to_device(corner_offsets)
        d_cx, d_cy = _to_device(np.r_[corner_x, 0.0]), _to_device(np.r_[corner_y, 0.0])
    x0, y0, x1, y1, cell, CX, CY = _pick_grid(bounds, flags, tx, ty)
    d_b, d_f = _to_device(bounds.reshape(-1)), _to_device(flags)
    device = d_x.device
    stream = ctypes.c_void_p(_stream(device))
    d_xi, d_yi = _out(device, torch.int32, n), _out(device, torch.int32, n)
    with _lib.lock():
        _lib.call("pmi_picks_cells_dev", _dptr(d_x), tx, _dptr(d_y), ty, n, x0, y0, x1, y1, cell, CX, CY, _dptr(d_xi),
                  _dptr(d_yi), stream)
    table = BlockTable.from_device(d_xi, d_yi, CY, CX)
    head = (_dptr(d_x), tx, _dptr(d_y), ty, _dptr(table.rows), _dptr(table.keys), n, table.p, x0, y0, x1, y1, cell, CX,
            CY, shape, _dptr(d_b), _dptr(d_f), _dptr(d_co), _dptr(d_cx), _dptr(d_cy), n_corners, P)
    with _lib.lock():
        return _picks_csr("pmi_picks_shape_dev", head, P, device, stream)


def picks_square(x, y, bounds, flags):
    """Members of square picks over the whole table -> (int64 offsets[P + 1], int64 rows ascending per pick):
    x_min < x < x_max and y_min < y < y_max with bounds[i] = (x_min, x_max, y_min, y_max); bit b of flags[i] marks bound
    b as a weak Python scalar, compared in the column's dtype (else in float64)."""
    return _picks_shape(PICK_SQUARE, x, y, bounds, flags)


def picks_rectangle(x, y, bounds, flags, corner_x, corner_y):
    """The same box, then check_if_in_rectangle against the (P, 4) corners, in float64."""
    cx, cy = np.asarray(corner_x, np.float64).reshape(-1, 4), np.asarray(corner_y, np.float64).reshape(-1, 4)
    return _picks_shape(PICK_RECTANGLE, x, y, bounds, flags, np.arange(len(cx) + 1, dtype=np.int32) * 4, cx.reshape(-1),
                        cy.reshape(-1))


def picks_polygon(x, y, bounds, flags, corner_offsets, corner_x, corner_y):
    """The same box, then check_if_in_polygon against the corners
    corner_x / corner_y [corner_offsets[i] : corner_offsets[i + 1]] of pick i, in float64."""
    return _picks_shape(PICK_POLYGON, x, y, bounds, flags, corner_offsets, corner_x, corner_y)


# ---- pick similar (csrc/similar.hip, picasso/postprocess.py:476-736, :820-957) ----
SIMILAR_MAX_SHIFTS = 500          # the reference's cap on the moves of one grid point


def similar_shift(table: "BlockTable", x, y, x_range, y_range_base, y_range_shift, x_block, y_block_base, y_block_shift,
                  r2: float, gate: float, max_shifts: int = SIMILAR_MAX_SHIFTS):
    """The mean shift of every point of pick_similar's grid over a table in block order (``table`` built from
    uint32(x / r), uint32(y / r) of the same rows; host arrays or device tensors) -> (cx, cy float64, n int32, rmsd
    float64) per grid point, columns outside and y inside, odd columns on ``y_range_shift`` (pmi_similar_shift_dev).
    ``gate`` is the reference's ``min_n_locs``; ``n == 0`` marks a point the gate or the first circle skipped."""
    import torch
    _lib.require_gpu()
    d_x, tx, d_y, ty = table._columns(x, y)
    gx, gb, gs = (np.ascontiguousarray(a, np.float64) for a in (x_range, y_range_base, y_range_shift))
    bx, bb, bs = (np.ascontiguousarray(_grid_blocks(a)) for a in (x_block, y_block_base, y_block_shift))
    n_x, n_y = len(gx), len(gb)
    if len(bx) != n_x or not (len(gs) == len(bb) == len(bs) == n_y) or any(a.ndim != 1 for a in (gx, gb, gs, bx, bb, bs)):
        raise ValueError("one block index per grid value, and as many shifted y values as base ones")
    if not 0 <= int(max_shifts) <= 1 << 16:
        raise ValueError("max_shifts must lie in 0 .. 65536")
    G = n_x * n_y
    if G == 0:
        return np.zeros(0), np.zeros(0), np.zeros(0, np.int32), np.zeros(0)
    d_grid = [_to_device(a) for a in (gx, bx, gb, gs, bb, bs)]
    out = torch.zeros(3 * G, dtype=torch.float64, device=table.device)
    out_n = torch.zeros(G, dtype=torch.int32, device=table.device)
    with _lib.lock():
        _lib.call("pmi_similar_shift_dev", _dptr(d_x), tx, _dptr(d_y), ty, _dptr(table.rows), _dptr(table.keys), table.n,
                  table.p, table.K, table.L, _dptr(d_grid[0]), _dptr(d_grid[1]), n_x, _dptr(d_grid[2]), _dptr(d_grid[3]),
                  _dptr(d_grid[4]), _dptr(d_grid[5]), n_y, float(r2), float(gate), int(max_shifts), _dptr(out[:G]),
                  _dptr(out[G:2 * G]), _dptr(out_n), _dptr(out[2 * G:]), ctypes.c_void_p(table.stream))
        host = out.cpu().numpy()
        return host[:G].copy(), host[G:2 * G].copy(), out_n.cpu().numpy(), host[2 * G:].copy()


def similar_filter(cand_x, cand_y, pick_x, pick_y, d2: float, d: float) -> np.ndarray:
    """The greedy pass of pick_similar over candidates in grid order, on the host (pmi_similar_filter) -> bool mask: a
    candidate is kept when every given pick and every earlier kept candidate has dx * dx + dy * dy > d2."""
    cx, cy = np.ascontiguousarray(cand_x, np.float64), np.ascontiguousarray(cand_y, np.float64)
    px, py = np.ascontiguousarray(pick_x, np.float64), np.ascontiguousarray(pick_y, np.float64)
    if cx.shape != cy.shape or px.shape != py.shape or cx.ndim != 1 or px.ndim != 1:
        raise ValueError("one x and one y per candidate and per pick")
    keep = np.zeros(len(cx), np.uint8)
    _lib.call("pmi_similar_filter", _lib.ptr(cx), _lib.ptr(cy), len(cx), _lib.ptr(px), _lib.ptr(py), len(px), float(d2),
              float(d), _lib.ptr(keep))
    return keep.astype(bool)


# ---- fiducial undrift (csrc/fiducials.hip, picasso/postprocess.py:3062-3156) ----
def fiducials_max_cells() -> int:
    """The largest picks x Frames matrix one call holds (12 bytes of device scratch per cell)."""
    return int(_lib.load().pmi_fiducials_max_cells())


def _fiducial_offsets(offsets):
    import torch
    if isinstance(offsets, torch.Tensor):
        offsets = offsets.cpu().numpy()
    offsets = np.ascontiguousarray(_index_column(offsets, "offsets"))
    if offsets.ndim != 1 or len(offsets) < 1 or offsets[0] != 0 or (np.diff(offsets) < 0).any():
        raise ValueError("offsets must be the P + 1 ascending offsets of the member rows, from 0")
    return offsets


def fiducials_drift(offsets, frame, columns, n_frames: int) -> np.ndarray:
    """The drift of the picked fiducials, as the reference's ``undrift_from_picked`` computes it under NumPy 2, bit for
    bit (pmi_fiducials_drift_dev) -> float64 (n_frames, len(columns)).  The members of the P picks come as a CSR: int64
    ``offsets[P + 1]``, and ``frame`` and one to three float32 / float64 coordinate ``columns`` gathered into pick
    order (host arrays or device tensors; the order inside a pick decides the bits of its mean and which row of a
    repeated frame counts: the last).  IndexError for a frame outside [-n_frames, n_frames), ValueError when a column
    leaves no frame with a value (np.interp), MemoryError beyond ``fiducials_max_cells()`` cells."""
    import torch
    _lib.require_gpu()
    offsets = _fiducial_offsets(offsets)
    P, F = len(offsets) - 1, int(n_frames)
    if not 1 <= len(columns) <= 3:
        raise ValueError("one to three coordinate columns")
    if P == 0 or F < 1:
        raise ValueError("array of sample points is empty")          # np.interp over no frame at all
    if P * F > fiducials_max_cells():
        raise MemoryError(f"{P} picks x {F} frames: more than {fiducials_max_cells()} cells in one call")
    if isinstance(frame, torch.Tensor):
        if frame.dtype != torch.int64 or frame.dim() != 1 or not frame.is_cuda:
            raise TypeError("a device frame column must be a 1-D int64 tensor on the GPU")
        d_frame = frame.contiguous()
    else:
        d_frame = _to_device(_index_column(frame, "frame"))
    cols = [_float_column(c) for c in columns]
    M = int(offsets[-1])
    _check_rows(M, "frame and the columns must have offsets[-1] rows", d_frame, *[d for d, _ in cols])
    device = d_frame.device
    d_off = _to_device(offsets)
    out = torch.empty((F, len(cols)), dtype=torch.float64, device=device)
    ptrs = (ctypes.c_void_p * len(cols))(*[d.data_ptr() if M else None for d, _ in cols])
    types = (ctypes.c_int * len(cols))(*[t for _, t in cols])
    status = ctypes.c_int(0)
    with _lib.lock():
        _lib.call("pmi_fiducials_drift_dev", _dptr(d_off), P, _dptr(d_frame) if M else None, M, ptrs, types, len(cols), F,
                  _dptr(out), ctypes.byref(status), ctypes.c_void_p(_stream(device)))
        if status.value & 1:
            raise IndexError(f"a frame is out of bounds for {F} frames")
        if status.value & 2:
            raise ValueError("array of sample points is empty")
        return out.cpu().numpy()


def fiducials_reduce(values, offsets) -> np.ndarray:
    """np.add.reduce of each run values[offsets[r] : offsets[r + 1]] in the values' own float type, by the workgroup
    sum of csrc/group_reduce.h (pmi_fiducials_reduce_dev); for the tests of that sum."""
    _lib.require_gpu()
    offsets = _fiducial_offsets(offsets)
    d_v, t = _float_column(values)
    if offsets[-1] > len(d_v):
        raise ValueError("offsets run past the values")
    R = len(offsets) - 1
    out = _out(d_v.device, d_v.dtype, R, zero=True)
    d_off = _to_device(offsets)
    with _lib.lock():
        _lib.call("pmi_fiducials_reduce_dev", _dptr(d_v) if len(d_v) else None, t, len(d_v), _dptr(d_off), R, _dptr(out),
                  ctypes.c_void_p(_stream(d_v.device)))
        return out.cpu().numpy()


# ---- nearest-neighbour distances (csrc/knn.hip, picasso/postprocess.py:3704-3739, picasso/spinna.py:696-747) ----
class _KnnGrid(ctypes.Structure):
    _fields_ = [("lo", ctypes.c_double * 2), ("w", ctypes.c_double * 2), ("n", ctypes.c_int32 * 2)]


def knn_limit() -> int:
    """The largest number of neighbours of one query (a dropped self column counts)."""
    return int(_lib.load().pmi_knn_limit())


def knn_points(X) -> np.ndarray:
    """A point set as the device takes it: float64, C-contiguous, (rows, 2 | 3)."""
    return _check_points(np.ascontiguousarray(X, np.float64))


class KnnIndex:
    """A finite point set X2 ordered on the device by the cells of a uniform grid over its x / y box
    (pmi_knn_order_dev), planned for queries of `k` neighbours; it then answers any number of query sets, with any k
    up to knn_limit().  `X2` is a host array, or a float64 device tensor of the same shape with its host box `box` =
    (lo, hi), the smallest and largest x and y."""

    def __init__(self, X2, k: int, box=None):
        import torch
        if box is None:
            X2 = knn_points(X2)
        else:                                          # raw pointers go to the library: nothing is converted here
            if (not isinstance(X2, torch.Tensor) or not X2.is_cuda or X2.dtype != torch.float64 or X2.dim() != 2
                    or int(X2.shape[1]) not in (2, 3) or not X2.is_contiguous()):
                raise ValueError("with a box the points must be a contiguous float64 device tensor of shape (n, 2) or (n, 3)")
            lo, hi = box
            if np.shape(lo) != (2,) or np.shape(hi) != (2,):
                raise ValueError("the box is (lo, hi): the smallest x and y, and the largest")
        _lib.require_gpu()
        if box is None:
            self.points = torch.from_numpy(X2).cuda()
            lo, hi = np.zeros(2), np.zeros(2)
            for a in range(2 if len(X2) else 0):       # column by column: a reduction along axis 0 is ten times slower
                lo[a], hi[a] = X2[:, a].min(), X2[:, a].max()
        else:
            self.points = X2
        self.m, self.dims = int(self.points.shape[0]), int(self.points.shape[1])
        lo, hi = np.ascontiguousarray(lo, np.float64), np.ascontiguousarray(hi, np.float64)
        self.device, self.stream = self.points.device, _stream(self.points.device)
        self.sorted = _out(self.device, torch.float64, self.m, self.dims)
        self.start = torch.empty(max(self.m, 1) + 1, dtype=torch.int32, device=self.device)
        self.grid = _KnnGrid()
        with _lib.lock():
            _lib.call("pmi_knn_order_dev", _dptr(self.points), self.dims, self.m, _lib.ptr(lo), _lib.ptr(hi), int(k),
                      _dptr(self.sorted), _dptr(self.start), ctypes.byref(self.grid), ctypes.c_void_p(self.stream))

    def query_device(self, d_x1, k: int):
        """(n, k) float64 device tensor of the distances from the rows of the float64 device tensor `d_x1`."""
        import torch
        if (not isinstance(d_x1, torch.Tensor) or d_x1.device != self.device or d_x1.dtype != torch.float64
                or d_x1.dim() != 2 or int(d_x1.shape[1]) != self.dims or not d_x1.is_contiguous()):
            raise ValueError(f"queries must be a contiguous float64 tensor of shape (n, {self.dims}) on {self.device}")
        n = int(d_x1.shape[0])
        out = _out(self.device, torch.float64, n, int(k))
        with _lib.lock():
            _lib.call("pmi_knn_query_dev", _dptr(d_x1), self.dims, n, _dptr(self.sorted), _dptr(self.start), self.m,
                      ctypes.byref(self.grid), int(k), _dptr(out), ctypes.c_void_p(self.stream))
        return out

    def query(self, X1, k: int) -> np.ndarray:
        """(n, k) float64 distances from the rows of the host array `X1`, ascending, inf where the set has fewer rows."""
        import torch
        X1 = knn_points(X1)
        if X1.shape[1] != self.dims:
            raise ValueError(f"queries must have {self.dims} columns, not {X1.shape[1]}")
        return self.query_device(torch.from_numpy(X1).to(self.device), k).cpu().numpy()


# ---- cluster centers (csrc/centers.hip, picasso/clusterer.py:694-897) ----
CENTERS_MEAN, CENTERS_XSUM, CENTERS_FIRST, CENTERS_EVENTS = 0, 1, 2, 3


class _CentersColumn(ctypes.Structure):
    _fields_ = [("data", ctypes.c_void_p), ("weight", ctypes.c_void_p), ("sum", ctypes.c_void_p),
                ("mean", ctypes.c_void_p), ("std", ctypes.c_void_p),
                ("op", ctypes.c_int32), ("type", ctypes.c_int32), ("w_type", ctypes.c_int32)]


class CenterGroups:
    """The rows of a table in the order of their ``group`` column, sent to the device once (pmi_centers_order_dev):
    ``unique`` are the distinct labels ascending (what ``groupby(sort=True)`` returns), ``n_locs`` their sizes,
    ``order()`` is ``np.argsort(group, kind="stable")``.  Every statistic is one array per distinct label."""

    def __init__(self, group):
        import torch
        _lib.require_gpu()
        group = _index_column(group, "group")
        if group.ndim != 1 or len(group) == 0:
            raise ValueError("group must be a column of at least one row")
        self._reside(group)
        unique = torch.empty(self.n, dtype=torch.int64, device=self.device)
        G = ctypes.c_int64(0)
        with _lib.lock():
            _lib.call("pmi_centers_order_dev", _dptr(self.group), self.n, self.g_min, self.g_max, _dptr(self.rows),
                      _dptr(self.start), _dptr(unique), ctypes.byref(G), ctypes.c_void_p(self.stream))
            self.n_groups = int(G.value)
            self.unique = unique[:self.n_groups].cpu().numpy()
            self.offsets = self.start[:self.n_groups + 1].cpu().numpy()
        self.n_locs = np.diff(self.offsets).astype(np.int64)

    def _reside(self, group):
        """What every order by labels keeps: the checked int64 ``group`` column on the device with its range, where the
        table lives, room for the order, and the uploads of its columns."""
        import torch
        self.n = int(len(group))
        self.g_min, self.g_max = int(group.min()), int(group.max())
        self.group = _to_device(group)
        self.device, self.stream = self.group.device, _stream(self.group.device)
        self.rows = torch.empty(self.n, dtype=torch.int32, device=self.device)
        self.start = torch.empty(self.n + 1, dtype=torch.int32, device=self.device)
        self._cache = _Uploads(self.n)

    def order(self) -> np.ndarray:
        """The int64 stable permutation into group order."""
        return self.rows.cpu().numpy().astype(np.int64)

    def _dev(self, a):
        """One upload per host column, however many statistics read it."""
        return self._cache.column(a)

    def weights(self, lpx, lpy):
        """Device column ``1.0 / (lpx + lpy) ** 2`` in NumPy's result type of the two -> (tensor, dtype)."""
        import torch
        lpx, lpy = np.asarray(lpx), np.asarray(lpy)
        dt = np.result_type(lpx.dtype, lpy.dtype)
        code = centers_type(dt, True)
        d_x, d_y = _to_device(lpx, dt), _to_device(lpy, dt)
        _check_rows(self.n, _PER_ROW, lpx, lpy)
        w = torch.empty(self.n, dtype=d_x.dtype, device=self.device)
        with _lib.lock():
            _lib.call("pmi_centers_weights_dev", _dptr(d_x), _dptr(d_y), code, self.n, _dptr(w),
                      ctypes.c_void_p(self.stream))
        return w, np.dtype(dt)

    def stats(self, requests):
        """``requests``: a list of (op, column, weight, wants) with ``wants`` a subset of ("sum", "mean", "std") for
        CENTERS_MEAN and ignored otherwise; ``column`` a host column or the (tensor, dtype) of ``weights()``, which
        is also what ``weight`` takes.
        -> one dict of arrays per request ("sum" holds the result of the other ops)."""
        G = self.n_groups
        rows, outs = [], []
        for op, column, weight, wants in requests:
            if isinstance(column, tuple):                   # already on the device: what weights() returned
                d, dtype = column
            else:
                column = _centers_column(column, "a statistics column")
                d, dtype = self._dev(column), column.dtype
            code = centers_type(dtype, op == CENTERS_XSUM)
            w_code, w_t = 0, None
            if op == CENTERS_MEAN:
                acc = np.dtype(np.float32) if dtype == np.float32 else np.dtype(np.float64)
                types = {"sum": acc, "mean": acc, "std": np.dtype(np.float64)}
                wants = tuple(wants)
            elif op == CENTERS_XSUM:
                w_t, w_dt = weight
                w_code = centers_type(w_dt, True)
                types, wants = {"sum": np.promote_types(dtype, w_dt)}, ("sum",)
            elif op == CENTERS_FIRST:
                types, wants = {"sum": np.dtype(dtype)}, ("sum",)
            elif op == CENTERS_EVENTS:
                types, wants = {"sum": np.dtype(np.int32)}, ("sum",)
            else:
                raise ValueError(f"unknown statistics op {op}")
            out = {k: _to_device(np.zeros(G, types[k])) for k in wants}
            outs.append((out, types))
            rows.append((d, w_t, out.get("sum"), out.get("mean"), out.get("std"), int(op), code, w_code))
        table = _Table(_CentersColumn, rows)
        with _lib.lock():
            _lib.call("pmi_centers_stats_dev", _dptr(self.rows), _dptr(self.start), self.n, G, table.ptr, table.count,
                      ctypes.c_void_p(self.stream))
            return [{k: t.cpu().numpy().view(types[k]) for k, t in out.items()} for out, types in outs]

    def hull_areas(self, x, y) -> np.ndarray:
        """float64 area of the convex hull of every label's (x, y)."""
        import torch
        x, y = np.asarray(x), np.asarray(y)
        tx, ty = centers_type(x.dtype, True), centers_type(y.dtype, True)
        d_x, d_y = self._dev(x), self._dev(y)
        area = torch.zeros(self.n_groups, dtype=torch.float64, device=self.device)
        with _lib.lock():
            _lib.call("pmi_centers_hull_dev", _dptr(d_x), tx, _dptr(d_y), ty, _dptr(self.group), self.g_min, self.g_max,
                      _dptr(self.start), self.n, self.n_groups, _dptr(area), ctypes.c_void_p(self.stream))
            return area.cpu().numpy()


# ---- cluster areas and volumes (csrc/areas.hip, picasso/clusterer.py:1068-1169) ----
AREAS_SCRATCH_BINS = 1 << 25       # bins of the images one launch of the scratch path holds, two float64 copies of each
_AREAS_GEOM = np.dtype([("start", np.float64, 3), ("next", np.float64, 3), ("len", np.int64, 3)])
AREAS_LDS_BINS = 4096              # PMI_AREAS_LDS_BINS: the most bins of an image that stays in LDS
AREAS_MAX_BINS = 1 << 24           # PMI_AREAS_MAX_BINS: the most bins of any image, and of any one axis


def areas_limits():
    """(AREAS_LDS_BINS, AREAS_MAX_BINS) as the loaded library has them; a library built with other bounds is refused."""
    L = _lib.load()
    limits = int(L.pmi_areas_lds_bins()), int(L.pmi_areas_max_bins())
    if limits != (AREAS_LDS_BINS, AREAS_MAX_BINS):
        raise _lib.HipBackendError(f"libpicasso_hip was built with the area bounds {limits}, this package with "
                                   f"{(AREAS_LDS_BINS, AREAS_MAX_BINS)}")
    return limits


class _AreasColumns(ctypes.Structure):
    _fields_ = [("data", ctypes.c_void_p * 3), ("type", ctypes.c_int32 * 3), ("dims", ctypes.c_int32),
                ("f32", ctypes.c_int32), ("z_div", ctypes.c_double)]


def areas_weights() -> np.ndarray:
    """The 17 float64 weights of ``scipy.ndimage.gaussian_filter(sigma=2)`` (truncate 4: radius 8), as scipy's
    ``_gaussian_kernel1d`` computes them with NumPy."""
    x = np.arange(-8, 9)
    phi = np.exp(-0.5 / (2.0 * 2.0) * x ** 2)
    return phi / phi.sum()


def areas_bins(unique, lens) -> np.ndarray:
    """Host check of the edge counts ``lens`` (groups x dimensions, int64; -1 / -2 where NumPy's ``arange`` refuses the
    length) of the groups labelled ``unique`` -> int64 bins of every group's image.  Raises what ``np.arange`` raises
    for the first group it refuses, and ``MemoryError`` for the first group with more than ``AREAS_MAX_BINS`` bins in its
    image or along one axis (NumPy builds every edge array, so the reference fails on a huge axis even beside an empty
    one).  No device work."""
    limit = AREAS_MAX_BINS
    lens = np.asarray(lens, np.int64).reshape(len(unique), -1)
    bins = np.prod(np.clip(lens - 1, 0, None).astype(np.float64), axis=1)
    for g in np.flatnonzero((lens < 0).any(axis=1) | (lens > limit + 1).any(axis=1) | (bins > limit)):
        for n in lens[g]:
            if n == -1:
                raise ValueError("arange: cannot compute length")
            if n == -2:
                raise ValueError("Maximum allowed size exceeded")
        shape = " x ".join(str(max(int(n) - 1, 0)) for n in lens[g])
        raise MemoryError(f"group {unique[g]}: its image of {shape} bins exceeds the limit of {limit} bins "
                          "(the localization precision is too small for the extent of the group)")
    return bins.astype(np.int64)


class AreaImages:
    """The images of ``_cluster_area`` for every group of a ``CenterGroups``: ``columns`` are the host columns x, y
    (and z), each float32 or float64, ``z_div`` what z is divided by in their common type, ``bin_xy`` / ``bin_z`` the
    bin sizes as NumPy scalars (their type decides the arithmetic of ``np.arange``).  The constructor computes the
    extents and edge counts on the device (pmi_areas_shape_dev) and checks them on the host (``areas_bins``);
    ``areas()`` builds, blurs and thresholds the images (pmi_areas_image_dev)."""

    def __init__(self, groups: "CenterGroups", columns, z_div, bin_xy, bin_z):
        import torch
        self.groups, self.dims = groups, len(columns)
        self.lds_bins, self.max_bins = areas_limits()
        if self.dims not in (2, 3):
            raise ValueError("the points have 2 or 3 columns")
        columns = [np.asarray(c) for c in columns]
        self.dtype = np.result_type(*columns)
        for c in columns:
            centers_type(c.dtype, True)
        self._keep = [groups._dev(c) for c in columns]
        self.cols = _AreasColumns()
        for d, (c, t) in enumerate(zip(columns, self._keep)):
            self.cols.data[d], self.cols.type[d] = t.data_ptr(), centers_type(c.dtype)
        self.cols.dims, self.cols.f32 = self.dims, int(self.dtype == np.float32)
        if self.dims == 3:
            # ``X[:, 2] /= pixelsize``: a Python number takes the array's type, a NumPy float64 scalar keeps its own
            weak = np.result_type(np.empty(0, self.dtype), z_div) == self.dtype
            self.cols.z_div = float(self.dtype.type(z_div)) if weak else float(z_div)
        else:
            self.cols.z_div = 1.0
        G = groups.n_groups
        self.geom = torch.zeros(G * _AREAS_GEOM.itemsize, dtype=torch.uint8, device=groups.device)
        bin_f32 = int(np.asarray(bin_xy).dtype == np.float32)
        with _lib.lock():
            _lib.call("pmi_areas_shape_dev", ctypes.byref(self.cols), _dptr(groups.rows), _dptr(groups.start), groups.n, G,
                      float(bin_xy), float(bin_z), bin_f32, _dptr(self.geom), ctypes.c_void_p(groups.stream))
            self.host_geom = self.geom.cpu().numpy().view(_AREAS_GEOM)
        self.lens = self.host_geom["len"][:, :self.dims]
        self.bins = areas_bins(groups.unique, self.lens)

    def shape(self, g: int) -> tuple:
        return tuple(int(max(n - 1, 0)) for n in self.lens[g])

    def _launch(self, listed, offsets, scratch, area, weights, want, want_image):
        import torch
        groups = self.groups
        d_list = torch.from_numpy(np.ascontiguousarray(listed, np.int32)).to(groups.device)
        d_off = None if offsets is None else torch.from_numpy(np.ascontiguousarray(offsets, np.int64)).to(groups.device)
        with _lib.lock():
            _lib.call("pmi_areas_image_dev", ctypes.byref(self.cols), _dptr(groups.rows), _dptr(groups.start), groups.n,
                      groups.n_groups, _dptr(self.geom), _dptr(d_list), _dptr(d_off), len(listed), _dptr(scratch),
                      0 if scratch is None else int(scratch.numel()), _dptr(weights), _dptr(area), int(want),
                      _dptr(want_image), ctypes.c_void_p(groups.stream))

    def areas(self, image_of=None, force_scratch: bool = False):
        """float32 area (count / 4) or volume (count / (16 / 5)) of every group; 0 for a group without bins.  With
        ``image_of`` (an index into the groups) -> (areas, that group's blurred float64 image).  ``force_scratch``
        sends every image through the global scratch, whatever its size."""
        import torch
        device = self.groups.device
        lds_bins = 0 if force_scratch else self.lds_bins
        area = torch.zeros(self.groups.n_groups, dtype=torch.float32, device=device)
        weights = torch.from_numpy(areas_weights()).to(device)
        want = -1 if image_of is None else int(image_of)
        want_image = None
        if want >= 0:
            want_image = _out(device, torch.float64, self.bins[want], zero=True)
        small = np.flatnonzero((self.bins > 0) & (self.bins <= lds_bins))
        large = np.flatnonzero(self.bins > lds_bins)
        if len(small):
            self._launch(small, None, None, area, weights, want, want_image)
        # the images of one launch share one allocation, each at the prefix sum of the sizes before it
        ends = np.cumsum(self.bins[large])
        before = ends - self.bins[large]
        scratch, lo = None, 0
        while lo < len(large):
            hi = max(int(np.searchsorted(ends, before[lo] + AREAS_SCRATCH_BINS, side="right")), lo + 1)
            need = 2 * int(ends[hi - 1] - before[lo])
            if scratch is None or scratch.numel() < need:
                scratch = torch.empty(need, dtype=torch.float64, device=device)
            self._launch(large[lo:hi], 2 * (before[lo:hi] - before[lo]), scratch, area, weights, want, want_image)
            lo = hi
        out = area.cpu().numpy()
        if want < 0:
            return out
        return out, want_image.cpu().numpy().reshape(self.shape(want))


# ---- dark times and group properties (csrc/kinetics.hip, picasso/postprocess.py:1985-2004, :3580-3649) ----
KINETICS_MAX_COLUMNS = 64          # descriptors per pmi_kinetics_stats_dev call
KINETICS_FRAME_LIMIT = 2 ** 62     # |frame|, |last_frame| below it: the signed 64-bit difference cannot overflow


class _KineticsColumn(ctypes.Structure):
    _fields_ = [("data", ctypes.c_void_p), ("mean", ctypes.c_void_p), ("std", ctypes.c_void_p), ("type", ctypes.c_int32)]


class DarkTable:
    """frame, last_frame and group of a table of binding events as int64 device columns, ordered once by
    (group, last_frame) (pmi_kinetics_dark_order_dev); ``search()`` is one bisection per row."""

    def __init__(self, frame, group, last_frame):
        import torch
        _lib.require_gpu()
        frame, group, last_frame = (_index_column(a, what) for a, what in
                                    ((frame, "frame"), (group, "group"), (last_frame, "last_frame")))
        self.n = int(len(frame))
        if self.n == 0 or not (len(group) == len(last_frame) == self.n):
            raise ValueError("frame, group and last_frame must have one length, of at least one row")
        self.max_frame = int(frame.max())
        self.frame, self.group, self.last = _to_device(frame), _to_device(group), _to_device(last_frame)
        self.device, self.stream = self.frame.device, _stream(self.frame.device)
        self.rows = torch.empty(self.n, dtype=torch.int32, device=self.device)
        self.last_sorted = torch.empty(self.n, dtype=torch.int64, device=self.device)
        self.run = torch.empty(self.n, dtype=torch.int32, device=self.device)
        self.start = torch.empty(self.n + 1, dtype=torch.int32, device=self.device)
        with _lib.lock():
            _lib.call("pmi_kinetics_dark_order_dev", _dptr(self.last), _dptr(self.group), self.n, int(last_frame.min()),
                      int(last_frame.max()), int(group.min()), int(group.max()), _dptr(self.rows),
                      _dptr(self.last_sorted), _dptr(self.run), _dptr(self.start), ctypes.c_void_p(self.stream))

    def search(self) -> np.ndarray:
        """int64 dark time of every row, -1 where there is none."""
        import torch
        dark = torch.empty(self.n, dtype=torch.int64, device=self.device)
        with _lib.lock():
            _lib.call("pmi_kinetics_dark_search_dev", _dptr(self.frame), _dptr(self.rows), _dptr(self.last_sorted),
                      _dptr(self.run), _dptr(self.start), self.n, self.max_frame, _dptr(dark),
                      ctypes.c_void_p(self.stream))
            return dark.cpu().numpy()


def _float64_pair(groups: "CenterGroups"):
    """Two float64 device outputs of one entry per group of ``groups``."""
    import torch
    return tuple(torch.empty(groups.n_groups, dtype=torch.float64, device=groups.device) for _ in range(2))


def group_mean_std(groups: "CenterGroups", columns):
    """pandas' ``Series.mean()`` and ``Series.std()`` of every host column in ``columns`` per group of ``groups``
    (pmi_kinetics_stats_dev) -> a list of (float64 mean, float64 std), one pair of arrays per column."""
    out = []
    columns = [_centers_column(c, "a statistics column") for c in columns]
    rows = [(groups._dev(c), *_float64_pair(groups), centers_type(c.dtype)) for c in columns]
    for table in _Table.chunks(_KineticsColumn, rows, KINETICS_MAX_COLUMNS):
        with _lib.lock():
            _lib.call("pmi_kinetics_stats_dev", _dptr(groups.rows), _dptr(groups.start), groups.n, groups.n_groups,
                      table.ptr, table.count, ctypes.c_void_p(groups.stream))
            out += [(mean.cpu().numpy(), std.cpu().numpy()) for _, mean, std, _ in table.rows]
    return out


# ---- cluster combine (csrc/combine.hip, picasso/postprocess.py:2174-2419) ----
COMBINE_MAX_COLUMNS = 32           # descriptors per pmi_combine_stats_dev call


class _CombineColumn(ctypes.Structure):
    _fields_ = [("data", ctypes.c_void_p), ("weight", ctypes.c_void_p), ("mean", ctypes.c_void_p),
                ("std", ctypes.c_void_p), ("average", ctypes.c_void_p), ("weight_sum", ctypes.c_void_p),
                ("type", ctypes.c_int32)]


class CombineGroups(CenterGroups):
    """The rows of a table in the order of their (``group``, ``cluster``) pair, sent to the device once
    (pmi_combine_order_dev).  It is a ``CenterGroups`` whose labels are the pairs: ``n_groups`` counts the segments,
    ``unique`` holds each segment's group label and ``clusters`` its cluster label (groups ascending, clusters
    ascending within a group), ``n_locs`` the sizes, ``order()`` is ``np.lexsort((cluster, group))``; rows keep their
    table order within a segment, so ``group_mean_std`` and the statistics below take it as it is.
    ``group_offsets[g]`` is the first segment of the g-th distinct group, closed by the number of segments."""

    def __init__(self, group, cluster):
        import torch
        _lib.require_gpu()
        group, cluster = _index_column(group, "group"), _index_column(cluster, "cluster")
        if group.ndim != 1 or cluster.ndim != 1 or len(group) == 0 or len(cluster) != len(group):
            raise ValueError("group and cluster must be columns of one length, of at least one row")
        self._reside(group)
        self.c_min, self.c_max = int(cluster.min()), int(cluster.max())
        self.cluster = _to_device(cluster)
        self.group_start = torch.empty(self.n + 1, dtype=torch.int32, device=self.device)
        seg_group = torch.empty(self.n, dtype=torch.int64, device=self.device)
        seg_cluster = torch.empty(self.n, dtype=torch.int64, device=self.device)
        S, G = ctypes.c_int64(0), ctypes.c_int64(0)
        with _lib.lock():
            _lib.call("pmi_combine_order_dev", _dptr(self.group), _dptr(self.cluster), self.n, self.g_min, self.g_max,
                      self.c_min, self.c_max, _dptr(self.rows), _dptr(self.start), _dptr(seg_group), _dptr(seg_cluster),
                      _dptr(self.group_start), ctypes.byref(S), ctypes.byref(G), ctypes.c_void_p(self.stream))
            self.n_groups = int(S.value)
            self.n_outer = int(G.value)
            self.unique = seg_group[:self.n_groups].cpu().numpy()
            self.clusters = seg_cluster[:self.n_groups].cpu().numpy()
            self.offsets = self.start[:self.n_groups + 1].cpu().numpy()
            self.group_offsets = self.group_start[:self.n_outer + 1].cpu().numpy()
        self.n_locs = np.diff(self.offsets).astype(np.int64)

    def hull_areas(self, x, y):
        raise NotImplementedError("convex hulls are per label of one column: use CenterGroups")


def _combine_floats(a, what: str) -> np.ndarray:
    """A host column for the weighted average: 1-D, float32 or float64, contiguous."""
    a = np.ascontiguousarray(a)
    if a.ndim != 1 or a.dtype not in (np.dtype(np.float32), np.dtype(np.float64)):
        raise TypeError(f"{what} must be a float32 or float64 column, not {a.dtype} of shape {a.shape}")
    return a


def combine_stats(groups: "CombineGroups", moments=(), averages=()):
    """Per segment of ``groups`` (pmi_combine_stats_dev): for every host column in ``moments`` pandas'
    ``Series.mean()`` and ``Series.std()``; for every (column, weights) pair in ``averages``, both float32 or both
    float64 (promote as ``np.average`` does before the call), ``np.average(column, weights=weights)`` and the sum of
    the weights.  -> (list of (float64 mean, float64 std), list of (float64 average, float64 weight sum))."""
    if not isinstance(groups, CombineGroups):
        raise TypeError("groups must be a CombineGroups")
    jobs = []
    for c in moments:
        c = _centers_column(c, "a statistics column")
        _check_rows(groups.n, _PER_ROW, c)
        jobs.append((np.ascontiguousarray(c), None))
    for x, w in averages:
        x, w = _combine_floats(x, "an averaged column"), _combine_floats(w, "the weights")
        if x.dtype != w.dtype or len(x) != groups.n or len(w) != groups.n:
            raise ValueError("an averaged column and its weights must have one floating type and one entry per row")
        jobs.append((x, w))
    rows, pairs, out = [], [], []
    for c, w in jobs:
        a, b = _float64_pair(groups)
        pairs.append((a, b))
        if w is None:                                       # the moments: mean and std
            rows.append((groups._dev(c), None, a, b, None, None, centers_type(c.dtype)))
        else:                                               # the average and the weight sum
            rows.append((groups._dev(c), groups._dev(w), None, None, a, b, centers_type(c.dtype, True)))
    for lo, table in enumerate(_Table.chunks(_CombineColumn, rows, COMBINE_MAX_COLUMNS)):
        with _lib.lock():
            _lib.call("pmi_combine_stats_dev", _dptr(groups.rows), _dptr(groups.start), groups.n, groups.n_groups,
                      table.ptr, table.count, ctypes.c_void_p(groups.stream))
            done = pairs[lo * COMBINE_MAX_COLUMNS:(lo + 1) * COMBINE_MAX_COLUMNS]
            out += [(a.cpu().numpy(), b.cpu().numpy()) for a, b in done]
    return out[:len(moments)], out[len(moments):]


def combine_min_distances(groups: "CombineGroups", points):
    """``points``: float64, C-contiguous, (rows, 2 | 3), in table order; every segment of ``groups`` must be one row.
    -> (min_dist, min_dist_xy | None): float64, one entry per SORTED position (``groups.order()``), the distance to the
    nearest other row of the group over all columns and, with 3 columns, over x and y (pmi_combine_mindist_dev)."""
    import torch
    if not isinstance(groups, CombineGroups):
        raise TypeError("groups must be a CombineGroups")
    if (not isinstance(points, np.ndarray) or points.dtype != np.float64 or points.ndim != 2
            or points.shape[1] not in (2, 3) or not points.flags.c_contiguous or len(points) != groups.n):
        raise ValueError("points must be a C-contiguous float64 array of shape (rows of the table, 2 or 3)")
    if groups.n_groups != groups.n:
        raise ValueError("every (group, cluster) pair must be one row")
    dims = int(points.shape[1])
    d_points = torch.from_numpy(points).to(groups.device)
    best = torch.empty(groups.n, dtype=torch.float64, device=groups.device)
    best_xy = torch.empty(groups.n, dtype=torch.float64, device=groups.device) if dims == 3 else None
    with _lib.lock():
        _lib.call("pmi_combine_mindist_dev", _dptr(d_points), dims, _dptr(groups.rows), _dptr(groups.start),
                  _dptr(groups.group_start), groups.n, groups.n_groups, groups.n_outer, _dptr(best), _dptr(best_xy),
                  ctypes.c_void_p(groups.stream))
        return best.cpu().numpy(), (best_xy.cpu().numpy() if best_xy is not None else None)


# ---- particle averaging (csrc/average.hip, picasso/average.py:49-118, :354-530) ----
AVERAGE_LDS_BINS = 16384           # PMI_AVERAGE_LDS_BINS: the most pixels of an average image held in LDS
AVERAGE_LIST = 2048                # PMI_AVERAGE_LIST: the rows of a group rotated at a time
AVERAGE_MAX_PIXELS = 4096          # PMI_AVERAGE_MAX_PIXELS: the most pixels per axis
AVERAGE_TARGET_BLOCKS = 4096       # workgroups the angle list is cut for when the groups are few
AVERAGE_MIN_CHUNK = 8              # angles per chunk, at least


def average_limits():
    """(AVERAGE_LDS_BINS, AVERAGE_LIST, AVERAGE_MAX_PIXELS) as the loaded library has them; a library built with other
    bounds is refused."""
    vals = [ctypes.c_int(0) for _ in range(3)]
    _lib.call("pmi_average_limits", *(ctypes.byref(v) for v in vals))
    limits = tuple(int(v.value) for v in vals)
    if limits != (AVERAGE_LDS_BINS, AVERAGE_LIST, AVERAGE_MAX_PIXELS):
        raise _lib.HipBackendError(f"libpicasso_hip was built with the averaging bounds {limits}, this package with "
                                   f"{(AVERAGE_LDS_BINS, AVERAGE_LIST, AVERAGE_MAX_PIXELS)}")
    return limits


def average_geometry(oversampling, t_min, t_max):
    """The reference's expressions for the image of ``render_hist_numba`` (picasso/render.py:765-770), evaluated by
    NumPy in the types they come in: (n_pixel, sub_f32, mul_f32), the last two saying whether ``x - t_min`` and the
    product with the oversampling are float32 operations for a float32 ``x``.  No device work."""
    n_pixel = int(np.ceil(oversampling * (t_max - t_min)))
    probe = np.zeros(1, np.float32) - t_min
    scaled = oversampling * probe
    for a in (probe, scaled):
        if a.dtype not in (np.float32, np.float64):
            raise TypeError(f"the view and the oversampling give {a.dtype} pixels; float32 or float64 expected")
    return n_pixel, int(probe.dtype == np.float32), int(scaled.dtype == np.float32)


def average_chunks(n_groups: int, n_angles: int) -> int:
    """Chunks the angle list is cut into, so that a few groups still fill the device."""
    want = -(-AVERAGE_TARGET_BLOCKS // max(int(n_groups), 1))
    return int(max(1, min(want, n_angles // AVERAGE_MIN_CHUNK, 65536)))


class AverageAligner:
    """One alignment step of ``picasso.average`` for the groups of a table: the group order goes to the device once
    (``CenterGroups``), the angle list once (``cos`` / ``sin`` taken per scalar angle on the host, as the reference
    takes them); ``iteration()`` is one pass from a given state of the float32 coordinates."""

    def __init__(self, group, angles):
        self.groups = CenterGroups(group)
        self.limits = average_limits()
        angles = np.asarray(angles, np.float64)
        self.n_angles = int(len(angles))
        self.cos = np.array([np.cos(a) for a in angles], np.float64)
        self.sin = np.array([np.sin(a) for a in angles], np.float64)
        self.d_cos, self.d_sin = _to_device(self.cos), _to_device(self.sin)
        self.max_group = int(self.groups.n_locs.max())

    def iteration(self, x, y, oversampling, t_min, t_max, force_global: bool = False, chunks=None):
        """``x``, ``y``: the float32 coordinates before the step.  -> dict with ``image`` (int32, n_pixel x n_pixel: the
        average image), ``choice`` (int32, groups x 3: correlation value, angle index, flat index of the fftshifted
        correlation; (0, -1, -1) where nothing was chosen), ``x`` / ``y`` (float32, aligned), ``chunks`` and ``ms``
        (the three kernels' milliseconds by device events).  Raises ``ValueError`` before the align launch when a
        correlation sum could reach 2**31, ``IndexError`` where the reference's histogram would index past its image."""
        import torch
        groups, L = self.groups, _lib.load()
        x, y = np.ascontiguousarray(x), np.ascontiguousarray(y)
        if x.dtype != np.float32 or y.dtype != np.float32 or len(x) != groups.n or len(y) != groups.n:
            raise ValueError("x and y must be float32 columns with one entry per row of the table")
        n_pixel, sub_f32, mul_f32 = average_geometry(oversampling, t_min, t_max)
        if not 1 <= n_pixel <= self.limits[2]:
            raise ValueError(f"an average image of {n_pixel} pixels per axis (1 .. {self.limits[2]} are supported)")
        ov, lo, hi = float(oversampling), float(t_min), float(t_max)
        use_lds = int(not force_global and n_pixel * n_pixel <= self.limits[0])
        chunks = average_chunks(groups.n_groups, self.n_angles) if chunks is None else int(chunks)
        dev, G, n = groups.device, groups.n_groups, groups.n
        d_x, d_y = _to_device(x), _to_device(y)
        image = torch.empty(n_pixel * n_pixel, dtype=torch.int32, device=dev)
        dropped = torch.zeros(1, dtype=torch.int32, device=dev)
        parts = torch.empty(3 * G * chunks, dtype=torch.int32, device=dev)
        choice = torch.empty(3 * G, dtype=torch.int32, device=dev)
        x_out, y_out = torch.empty_like(d_x), torch.empty_like(d_y)
        stream = ctypes.c_void_p(groups.stream)
        ms = {}

        def timed(name, call, *args):
            t0, t1 = ctypes.c_void_p(), ctypes.c_void_p()
            _lib.call("pmi_event_create", ctypes.byref(t0))
            _lib.call("pmi_event_create", ctypes.byref(t1))
            try:
                _lib.call("pmi_event_record", t0, stream)
                _lib.call(call, *args, stream)
                _lib.call("pmi_event_record", t1, stream)
                took = ctypes.c_float(0)
                _lib.call("pmi_event_elapsed_ms", t0, t1, ctypes.byref(took))
                ms[name] = float(took.value)
            finally:
                L.pmi_event_destroy(t0)
                L.pmi_event_destroy(t1)

        with _lib.lock():
            timed("image", "pmi_average_image_dev", _dptr(d_x), _dptr(d_y), n, n_pixel, lo, hi, ov, sub_f32, mul_f32,
                  _dptr(image), _dptr(dropped))
            host_image = image.cpu().numpy().reshape(n_pixel, n_pixel)
            if int(dropped.cpu()[0]):
                raise IndexError(f"index {n_pixel} is out of bounds for axis 0 with size {n_pixel}")
            top = int(host_image.max())
            if self.max_group * top >= 2 ** 31:
                raise ValueError(f"a group of {self.max_group} rows against an average image that peaks at {top}: the "
                                 "correlation could exceed 32 bits")
            timed("align", "pmi_average_align_dev", _dptr(d_x), _dptr(d_y), _dptr(groups.rows), _dptr(groups.start), n, G,
                  n_pixel, lo, hi, ov, _dptr(self.d_cos), _dptr(self.d_sin), self.n_angles, chunks, _dptr(image), use_lds,
                  _dptr(parts), _dptr(dropped))
            if int(dropped.cpu()[0]):
                raise IndexError(f"index {n_pixel} is out of bounds for axis 0 with size {n_pixel}")
            timed("apply", "pmi_average_apply_dev", _dptr(d_x), _dptr(d_y), _dptr(groups.rows), _dptr(groups.start), n, G,
                  n_pixel, ov, _dptr(self.d_cos), _dptr(self.d_sin), self.n_angles, _dptr(parts), chunks, _dptr(choice),
                  _dptr(x_out), _dptr(y_out))
            return {"image": host_image, "choice": choice.cpu().numpy().reshape(G, 3), "x": x_out.cpu().numpy(),
                    "y": y_out.cpu().numpy(), "chunks": chunks, "ms": ms}


# ---- Fourier ring correlation and radial sums (csrc/frc.hip, picasso/postprocess.py:1398-1502, imageprocess.py:283-321) ----
FRC_MAX_SIDE = 16385               # PMI_FRC_MAX_SIDE: the largest odd image side
FRC_BLOCK = 256                    # lanes of a ring's workgroup: a ring of at most that many row segments gives each lane one
RADIAL_TYPES = {np.dtype("float32"): 0, np.dtype("float64"): 1, np.dtype("complex64"): 2, np.dtype("complex128"): 3}


def frc_max_side() -> int:
    """FRC_MAX_SIDE as the loaded library has it; a library built with another bound is refused."""
    side = int(_lib.load().pmi_frc_max_side())
    if side != FRC_MAX_SIDE:
        raise _lib.HipBackendError(f"libpicasso_hip was built with an FRC side of {side}, this package with {FRC_MAX_SIDE}")
    return side


def _frc_side(m: int) -> int:
    n = m if m % 2 else m - 1
    if n < 1:
        raise ValueError(f"an image of side {m} leaves nothing after the crop to an odd side")
    if n > frc_max_side():
        raise MemoryError(f"an FRC image of side {n} exceeds the limit of {FRC_MAX_SIDE}: two float64 images and two "
                          f"half spectra of that side would take {32 * n * n / 2 ** 30:.0f} GiB of device memory")
    return n


def render_hist_device(x, y, oversampling, y_min, x_min, y_max, x_max):
    """The histogram render (``render_arrays`` without widths) that stays on the device -> (n, float32 device tensor)."""
    import torch
    _lib.require_gpu()
    view, (n_y, n_x) = _viewport(oversampling, y_min, x_min, y_max, x_max)
    if max(n_y, n_x) > FRC_MAX_SIDE + 1:
        raise MemoryError(f"a render of {n_y} x {n_x} pixels exceeds the FRC limit of {FRC_MAX_SIDE} per side")
    d_x, d_y = _to_device(x, np.float32), _to_device(y, np.float32)
    image = torch.empty((n_y, n_x), dtype=torch.float32, device=d_x.device)
    count = torch.zeros(1, dtype=torch.int64, device=d_x.device)
    with _lib.lock():
        _lib.call("pmi_render_hist_dev", _dptr(d_x), _dptr(d_y), len(d_x), *view, _dptr(image), n_y, n_x, _dptr(count), None)
        n = int(count.cpu()[0])
    return n, image


def frc_arrays(im1, im2, w):
    """The device part of ``_frc``: two square float32 images of one side m (NumPy arrays, or device tensors as
    ``render_hist_device`` returns them) and the float64 Tukey profile ``w`` of the odd side n (m, or m - 1 for an even
    m) -> dict with ``images`` (the two masked float32 images, n x n, NumPy's bits for ``im *= mask``), ``sums``
    (3 x rings float64: numerator, power 1, power 2), ``curve`` (rings float64, NaN -> 0) and ``ms`` (window, fft, rings,
    curve: milliseconds by device events)."""
    import torch
    _lib.require_gpu()
    if tuple(im1.shape) != tuple(im2.shape) or len(im1.shape) != 2 or im1.shape[0] != im1.shape[1]:
        raise ValueError(f"two square images of one side are needed, not {tuple(im1.shape)} and {tuple(im2.shape)}")
    m = int(im1.shape[0])
    n = _frc_side(m)
    w = np.ascontiguousarray(w, np.float64)
    if w.shape != (n,):
        raise ValueError(f"the window profile must have the {n} values of the odd side, not {w.shape}")

    def dev(im):
        if isinstance(im, torch.Tensor):
            if im.dtype != torch.float32 or not im.is_cuda:
                raise TypeError("a device image must be a float32 tensor on the GPU")
            return im.contiguous()
        im = np.asarray(im)
        if im.dtype != np.float32:
            raise TypeError(f"the images must be float32, not {im.dtype}")
        return _to_device(im)

    d1, d2, d_w = dev(im1), dev(im2), _to_device(w)
    rings = n // 2 + 1
    sums = torch.empty(3 * rings, dtype=torch.float64, device=d1.device)
    curve = torch.empty(rings, dtype=torch.float64, device=d1.device)
    m1 = torch.empty((n, n), dtype=torch.float32, device=d1.device)
    m2 = torch.empty_like(m1)
    ms = (ctypes.c_float * 4)()
    torch.cuda.current_stream().synchronize()
    with _lib.lock():
        _lib.call("pmi_frc_curve_dev", _dptr(d1), _dptr(d2), m, _dptr(d_w), _dptr(sums), _dptr(curve), _dptr(m1), _dptr(m2),
                  ctypes.cast(ms, ctypes.c_void_p), None)
    return {"images": (m1.cpu().numpy(), m2.cpu().numpy()), "sums": sums.cpu().numpy().reshape(3, rings),
            "curve": curve.cpu().numpy(), "ms": dict(zip(("window", "fft", "rings", "curve"), (float(v) for v in ms)))}


def radial_sum_array(image) -> np.ndarray:
    """Ring sums of a centred square image of odd side: float32 / float64 / complex64 / complex128, summed in float64
    per component and cast to the image's type."""
    image = np.ascontiguousarray(image)
    if image.ndim != 2 or image.shape[0] != image.shape[1] or image.shape[0] % 2 != 1:
        raise ValueError(f"a square image of odd side is needed, not {image.shape}")
    if image.dtype not in RADIAL_TYPES:
        raise TypeError(f"radial sums of {image.dtype} images are not built (float32, float64, complex64, complex128)")
    n = _frc_side(int(image.shape[0]))
    _lib.require_gpu()
    out = np.empty(n // 2 + 1, image.dtype)
    with _lib.lock():
        _lib.call("pmi_radial_sum", _lib.ptr(image), RADIAL_TYPES[image.dtype], n, _lib.ptr(out))
    return out


# ---- image blur (csrc/blur.hip): the "smooth" and "convolve" renders ---------------------------------------------------------
class BlurPlan(NamedTuple):
    """What ``render._fftconvolve`` does to an image of one shape, decided on the host (``blur_plan``)."""
    route: str                  # "spatial": scipy.ndimage.gaussian_filter in bits; "direct": the sum in place of the FFT
    kernel: tuple               # (kernel_height, kernel_width) of the reference
    radius: tuple               # (r_y, r_x)
    weights: tuple              # (w_y, w_x): float64 vectors of 2 r + 1 values, None for a skipped axis
    skip: tuple                 # (skip_y, skip_x)
    S: float                    # the reference's kernel.sum() on the direct route (1.0 on the spatial one)


def gaussian_kernel1d(sigma: float, radius: int) -> np.ndarray:
    """scipy.ndimage's ``_gaussian_kernel1d(sigma, 0, radius)``: normalised float64 weights, symmetric.  The expressions
    are scipy's, so a NumPy scalar sigma is promoted as scipy promotes it."""
    sigma2 = sigma * sigma
    x = np.arange(-radius, radius + 1)
    phi_x = np.exp(-0.5 / sigma2 * x ** 2)
    return phi_x / phi_x.sum()


def spatial_plan(blur_width, blur_height, kernel=(0, 0)) -> BlurPlan:
    """``gaussian_filter(sigma=(blur_height, blur_width), mode="constant", truncate=5.0)`` as scipy runs it: an axis with
    a sigma ``<= 1e-15`` is skipped, the radius is ``int(5.0 * float(sigma) + 0.5)``, the weights ``gaussian_kernel1d`` of
    the sigma as it was given: scipy squares a float32 sigma (``_render_convolve`` makes one from the float32 median)
    in float32."""
    radius, weights, skip = [], [], []
    for sigma in (blur_height, blur_width):
        if sigma > 1e-15:
            sd = float(sigma)
            lw = int(5.0 * sd + 0.5)
            radius.append(lw), weights.append(gaussian_kernel1d(sigma, lw)), skip.append(False)
        else:
            radius.append(0), weights.append(None), skip.append(True)
    return BlurPlan("spatial", tuple(kernel), tuple(radius), tuple(weights), tuple(skip), 1.0)


def direct_plan(kernel_width: int, kernel_height: int, blur_width, blur_height) -> BlurPlan:
    """The reference's kernel of its FFT route: ``signal.windows.gaussian(kernel, width)`` per axis (not normalised) and
    ``S = np.outer(kernel_y, kernel_x).sum()``; no axis is skipped."""
    from scipy import signal
    with np.errstate(all="ignore"):
        kernel_y = np.asarray(signal.windows.gaussian(kernel_height, blur_height), np.float64)
        kernel_x = np.asarray(signal.windows.gaussian(kernel_width, blur_width), np.float64)
        S = float(np.outer(kernel_y, kernel_x).sum())
    return BlurPlan("direct", (kernel_height, kernel_width), (kernel_height // 2, kernel_width // 2), (kernel_y, kernel_x),
                    (False, False), S)


def blur_plan(n_y: int, n_x: int, blur_width, blur_height) -> BlurPlan:
    """The route of picasso/render.py:1433-1460 for an ``n_y`` x ``n_x`` image and what each axis is blurred with
    (``spatial_plan`` or ``direct_plan``).  A NaN width raises ValueError and an infinite one OverflowError from
    ``int(np.round(...))``, as in the reference."""
    kernel_width = 10 * int(np.round(blur_width)) + 1
    kernel_height = 10 * int(np.round(blur_height)) + 1
    spatial = (
        kernel_height < 0.05 * n_y
        and kernel_width < 0.05 * n_x
        and max(kernel_height, kernel_width) <= 101
    )
    if spatial:
        return spatial_plan(blur_width, blur_height, (kernel_height, kernel_width))
    return direct_plan(kernel_width, kernel_height, blur_width, blur_height)


def _blur_args(plan: BlurPlan):
    """The tail of the C calls: weights, radii, mode, scale; and the arrays to keep alive."""
    w_y, w_x = (None if w is None else np.ascontiguousarray(w, np.float64) for w in plan.weights)
    with np.errstate(all="ignore"):
        scale = float(np.float64(1.0) / np.float64(plan.S))
    return (_lib.ptr(w_y), int(plan.radius[0]), _lib.ptr(w_x), int(plan.radius[1]), 1 if plan.route == "spatial" else 0, scale), (w_y, w_x)


def blur_with_plan(image, plan: BlurPlan) -> np.ndarray:
    """The separable blur of csrc/blur.hip on a float32 image with the weights of ``plan`` -> float32 image."""
    image = np.asarray(image)
    if image.ndim != 2 or image.dtype != np.float32:
        raise TypeError(f"a 2-D float32 image is needed, not {image.dtype} with {image.ndim} dimensions")
    image = np.ascontiguousarray(image)
    _lib.require_gpu()
    out = np.empty_like(image)
    tail, keep = _blur_args(plan)
    with _lib.lock():
        _lib.call("pmi_blur", _lib.ptr(image), _lib.ptr(out), image.shape[0], image.shape[1], *tail)
    return out


def blur_array(image, blur_width, blur_height) -> np.ndarray:
    """``render._fftconvolve`` of a float32 image on the device -> float32 image (``blur_plan`` says how)."""
    shape = np.shape(image)
    if len(shape) != 2:
        raise TypeError(f"a 2-D float32 image is needed, not {len(shape)} dimensions")
    return blur_with_plan(image, blur_plan(shape[0], shape[1], blur_width, blur_height))


def render_blurred_arrays(x, y, oversampling, y_min, x_min, y_max, x_max, blur_width, blur_height):
    """-> (n, image float32): the histogram render followed by ``_fftconvolve(image, blur_width, blur_height)`` in one
    call; the histogram never leaves the device."""
    view, (n_y, n_x) = _viewport(oversampling, y_min, x_min, y_max, x_max)
    plan = blur_plan(n_y, n_x, blur_width, blur_height)
    _lib.require_gpu()
    x = np.ascontiguousarray(x, np.float32)
    y = np.ascontiguousarray(y, np.float32)
    image = np.empty((n_y, n_x), np.float32)
    n = ctypes.c_int64(0)
    tail, keep = _blur_args(plan)
    with _lib.lock():
        _lib.call("pmi_render_blurred", _lib.ptr(x), _lib.ptr(y), len(x), *view, *tail, _lib.ptr(image), n_y, n_x, ctypes.byref(n))
    return int(n.value), image


# ---- rotated views (csrc/render_rot.hip, picasso/render.py:1571-1637 locs_rotation and the renders with ang) -----------------
def rotation_coords(x, y, z):
    """The three coordinate columns as the rotated kernels take them -> (x, y, z, LINK type code): three float32 columns
    stay float32, any other mix becomes float64, which is what ``locs[["x", "y", "z"]].to_numpy()`` makes of it."""
    cols = [np.asarray(c) for c in (x, y, z)]
    _check_rows(len(cols[0]), _PER_ROW, *cols)
    dt = np.dtype(np.float32) if all(c.dtype == np.float32 for c in cols) else np.dtype(np.float64)
    return tuple(np.ascontiguousarray(c, dt) for c in cols) + (link_type(dt, True),)


def _rotation_matrices(matrix):
    m = np.ascontiguousarray(matrix, np.float64)
    if m.shape != (3, 3):
        raise ValueError(f"a rotation matrix has shape (3, 3), not {m.shape}")
    return m, np.ascontiguousarray(m, dtype=np.float32)


def _rotate_locs_device(d_x, d_y, d_z, code, m64, view):
    """pmi_rotate_locs_dev on resident columns -> (x', y', z' float64, in_view uint8) device tensors."""
    import torch
    n, dev = len(d_x), d_x.device
    out = [_out(dev, torch.float64, n) for _ in range(3)] + [_out(dev, torch.uint8, n)]
    _lib.call("pmi_rotate_locs_dev", _dptr(d_x), _dptr(d_y), _dptr(d_z), code, n, _lib.ptr(m64), *view,
              *[_dptr(t) for t in out], _stream(dev))
    return out


def rotate_locs_arrays(x, y, z, matrix, oversampling, y_min, x_min, y_max, x_max):
    """Every row rotated about the centre of the viewport -> (x', y', z' float64 in image units, in_view bool): what
    ``locs_rotation`` returns before it drops the rows out of view."""
    _lib.require_gpu()
    x, y, z, code = rotation_coords(x, y, z)
    m64, _ = _rotation_matrices(matrix)
    view, _ = _viewport(oversampling, y_min, x_min, y_max, x_max, image=False)
    with _lib.lock():
        d_x, d_y, d_z = (_to_device(c) for c in (x, y, z))
        xr, yr, zr, in_view = (t.cpu().numpy() for t in _rotate_locs_device(d_x, d_y, d_z, code, m64, view))
    return xr, yr, zr, in_view.astype(bool)


def render_rot_arrays(x, y, z, matrix, oversampling, y_min, x_min, y_max, x_max, lpx=None, lpy=None, lpz=None,
                      min_blur_width=0.0, iso=False, with_in_view=True):
    """-> (n, image float32, in_view bool or None): the rotated view.  lpx / lpy None = histogram, else the projected
    Gaussian (lpz None: twice the mean of lpx and lpy).  ``matrix`` is scipy's (3, 3) float64 rotation matrix; the
    float32 copy the covariance takes is rounded here.  ``in_view`` marks the rows counted in n."""
    import torch
    _lib.require_gpu()
    x, y, z, code = rotation_coords(x, y, z)
    m64, m32 = _rotation_matrices(matrix)
    view, (n_y, n_x) = _viewport(oversampling, y_min, x_min, y_max, x_max)
    widths = None
    if lpx is not None:
        widths = [np.ascontiguousarray(c, np.float32) for c in ((lpx, lpy) if lpz is None else (lpx, lpy, lpz))]
        _check_rows(len(x), _PER_ROW, *widths)
    with _lib.lock():
        d_x, d_y, d_z = (_to_device(c) for c in (x, y, z))
        dev = d_x.device
        image, count = _out(dev, torch.float32, n_y, n_x), _out(dev, torch.int64, 1, zero=True)
        if widths is None:
            _lib.call("pmi_render_hist_rot_dev", _dptr(d_x), _dptr(d_y), _dptr(d_z), code, len(x), _lib.ptr(m64), *view,
                      _dptr(image), n_y, n_x, _dptr(count), _stream(dev))
        else:
            d_w = [_to_device(c) for c in widths] + [None]
            _lib.call("pmi_render_gaussian_rot_dev", _dptr(d_x), _dptr(d_y), _dptr(d_z), code, _dptr(d_w[0]), _dptr(d_w[1]),
                      _dptr(d_w[2]), len(x), _lib.ptr(m64), _lib.ptr(m32), *view, float(min_blur_width), int(bool(iso)),
                      _dptr(image), n_y, n_x, _dptr(count), _stream(dev))
        in_view = _rotate_locs_device(d_x, d_y, d_z, code, m64, view)[3].cpu().numpy().astype(bool) if with_in_view else None
        n = int(count.cpu()[0])
        image = image.cpu().numpy()
    return n, image, in_view


# ---- kinetic rates of picks (csrc/cumexp.hip, picasso/lib.py:1263-1327) -----------------------------------------------------
CUMEXP_CONVERGED, CUMEXP_ITER_CAP, CUMEXP_REFUSED = 0, 1, 2      # the status codes of pmi_cumexp_fit


class KineticRates(NamedTuple):
    """Per segment: the fit's ``a``, ``t``, ``c`` and final cost ``0.5 * sum(r ** 2)`` (float64; ``t`` is the kinetic rate,
    and the mean of a segment the reference does not fit, whose ``a``, ``c`` and ``cost`` are NaN), the passes over the
    samples and the status (int32: CUMEXP_CONVERGED, CUMEXP_ITER_CAP, CUMEXP_REFUSED)."""
    a: np.ndarray
    t: np.ndarray
    c: np.ndarray
    cost: np.ndarray
    iterations: np.ndarray
    status: np.ndarray


def cumexp_kind(dtype) -> int:
    """The column kind pmi_cumexp_fit takes: 0 an integer (or bool) column, 1 float32, 2 float64."""
    dtype = np.dtype(dtype)
    if dtype.kind in "iub":
        return 0
    if dtype == np.float32:
        return 1
    if dtype == np.float64:
        return 2
    raise TypeError(f"no kinetic rate of a {dtype} column")


def kinetic_rates(values, offsets) -> KineticRates:
    """``lib.estimate_kinetic_rate`` of every segment ``values[offsets[s]:offsets[s + 1]]`` in one device call
    (pmi_cumexp_fit): the mean of a segment of at most two samples or of equal samples, the ``t`` of the bounded
    cumulative-exponential fit otherwise.  ``values`` is one column (integer, float32 or float64; integers must stay
    below 2**53), ``offsets`` the S + 1 ascending offsets from 0.  The values are not changed."""
    _lib.require_gpu()
    values = np.asarray(values)
    if values.ndim != 1:
        raise ValueError(f"values must be one column, not an array of shape {values.shape}")
    kind = cumexp_kind(values.dtype)
    offsets = np.ascontiguousarray(_index_column(offsets, "offsets"))
    if offsets.ndim != 1 or len(offsets) < 1 or offsets[0] != 0 or (np.diff(offsets) < 0).any() or offsets[-1] > len(values):
        raise ValueError("offsets must be the S + 1 ascending offsets of the segments, from 0 to at most len(values)")
    if kind == 0 and len(values) and max(int(values.max()), -int(values.min())) >= 2 ** 53:
        raise ValueError("integer samples must stay below 2**53")
    S = len(offsets) - 1
    as_f64 = np.ascontiguousarray(values, np.float64)
    fit = np.full((4, S), np.nan, np.float64)
    info = np.zeros((2, S), np.int32)
    if S:
        with _lib.lock():
            _lib.call("pmi_cumexp_fit", _lib.ptr(as_f64), len(as_f64), _lib.ptr(offsets), S, kind, _lib.ptr(fit), _lib.ptr(info))
    return KineticRates(fit[0], fit[1], fit[2], fit[3], info[0], info[1])


# ---- G5M molecular mapping in 2-D (csrc/g5m.hip, picasso/g5m.py) ---------------------------------------------------------------
G5M_LDS_RESP = 4096                # PMI_G5M_LDS_RESP: the most responsibilities (n K) a workgroup of the fit holds in LDS
G5M_MAX_K = 100                    # PMI_G5M_MAX_K: N_COMPONENTS_MAX of picasso/g5m.py
G5M_LP_ABS, G5M_FORCE_SCRATCH, G5M_QUAD_F32, G5M_FRAME_U32 = 1, 2, 4, 8
G5M_SEED = 42                      # G5M.random_state
G5M_STATS = ("frame", "std_frame", "mol_ll", "p_val", "lp", "rsum", "log_likelihood")
G5M_PROGRESS = ctypes.CFUNCTYPE(None, ctypes.c_int, ctypes.c_int64, ctypes.c_double, ctypes.c_void_p)


def g5m_limits():
    """(G5M_LDS_RESP, G5M_MAX_K, lanes of a workgroup) as the loaded library has them; a library built with other limits
    than this module's is refused."""
    vals = [ctypes.c_int(0) for _ in range(3)]
    _lib.call("pmi_g5m_limits", *(ctypes.byref(v) for v in vals))
    limits = tuple(int(v.value) for v in vals)
    if limits[:2] != (G5M_LDS_RESP, G5M_MAX_K):
        raise _lib.HipBackendError(f"libpicasso_hip.so has the G5M limits {limits[:2]}, this package {(G5M_LDS_RESP, G5M_MAX_K)}")
    return limits


def g5m_local_trials(n_components: int) -> int:
    """``n_local_trials`` of ``_kmeans_plusplus`` (picasso/g5m.py:264)."""
    return 2 + int(np.log(n_components))


def g5m_draws_needed(n_components: int) -> int:
    """Uniforms one seed of ``_kmeans_plusplus`` draws for that many components."""
    return (n_components - 1) * g5m_local_trials(n_components)


def g5m_draws(n_samples: int, n_seeds: int, n_uniform: int):
    """What ``_kmeans_plusplus`` draws for a cluster of ``n_samples`` rows under the seeds 42 .. 42 + n_seeds - 1, with
    NumPy's legacy generator: per seed ``RandomState(seed)``, one ``choice(n_samples)`` (int32) and the next ``n_uniform``
    ``uniform()`` values in order (float64).  The draws depend on the seed, ``n_samples`` and the position in the stream
    only, so one table serves every K."""
    first = np.zeros(n_seeds, np.int32)
    uniform = np.zeros((n_seeds, n_uniform), np.float64)
    for ii in range(n_seeds):
        rs = np.random.RandomState(G5M_SEED + ii)
        first[ii] = rs.choice(n_samples)
        uniform[ii] = rs.uniform(size=n_uniform)
    return first, uniform


class G5MModels(NamedTuple):
    """The models of a table of clusters, ``cap[c]`` components from ``start[c]`` on in every plane: ``model`` (5 x total
    float64: weights_, means_ x, means_ y, covariances_, precisions_cholesky_), ``imodel`` (2 x total int32: n_locs of the
    valid components in valid order, valid_idx padded with -1), ``info`` (n x 4 int32: K or 0, valid components,
    converged, last K tried) and ``bic``."""
    start: np.ndarray
    cap: np.ndarray
    model: np.ndarray
    imodel: np.ndarray
    info: np.ndarray
    bic: np.ndarray

    def of(self, c: int):
        """(weights_, means_, covariances_, precisions_cholesky_, valid_idx, n_locs, converged) of cluster c, or None."""
        K, nv = int(self.info[c, 0]), int(self.info[c, 1])
        if K == 0:
            return None
        s = slice(int(self.start[c]), int(self.start[c]) + K)
        return (self.model[0, s].copy(), np.stack([self.model[1, s], self.model[2, s]], axis=1), self.model[3, s].copy(),
                self.model[4, s].copy(), self.imodel[1, s][:nv].copy(), self.imodel[0, s][:nv].copy(), bool(self.info[c, 2]))


def _g5m_rows(x, y, lp, offsets):
    x, y, lp = (np.ascontiguousarray(a, np.float64) for a in (x, y, lp))
    offsets = np.ascontiguousarray(_index_column(offsets, "offsets"))
    if offsets.ndim != 1 or len(offsets) < 1 or offsets[0] != 0 or (np.diff(offsets) < 0).any() or offsets[-1] != len(x):
        raise ValueError("offsets must be the C + 1 ascending offsets of the clusters, from 0 to len(x)")
    if not (x.ndim == 1 and x.shape == y.shape == lp.shape):
        raise ValueError("x, y and lp must be columns of one length")
    return x, y, lp, offsets


def g5m_table(sizes, caps):
    """The draws of a table of clusters of ``sizes`` rows that fit up to ``caps`` components each: (table, first, uniform)
    as pmi_g5m_fit takes them, drawn once per distinct (size, cap)."""
    sizes, caps = np.asarray(sizes, np.int64), np.asarray(caps, np.int64)
    table = np.zeros((len(sizes), 4), np.int64)
    table[:, 0] = np.cumsum(caps) - caps
    firsts, uniforms, seen, n_first, n_uniform = [], [], {}, 0, 0
    for c, (n, cap) in enumerate(zip(sizes.tolist(), caps.tolist())):
        if cap < 1:
            continue
        if (n, cap) not in seen:
            seeds, stride = max(cap, 3), g5m_draws_needed(cap)
            f, u = g5m_draws(n, seeds, stride)
            seen[n, cap] = (n_first, n_uniform, stride)
            firsts.append(f), uniforms.append(u.ravel())
            n_first, n_uniform = n_first + seeds, n_uniform + seeds * stride
        table[c, 1:] = seen[n, cap]
    first = np.concatenate(firsts + [np.zeros(1, np.int32)])
    uniform = np.concatenate(uniforms + [np.zeros(1, np.float64)])
    return table, first, uniform


def _g5m_empty(caps):
    total = int(caps.sum())
    start = np.cumsum(caps) - caps
    return G5MModels(start, caps, np.zeros((5, total), np.float64), np.zeros((2, total), np.int32),
                     np.zeros((len(caps), 4), np.int32), np.full(len(caps), np.inf))


def g5m_search(x, y, lp, offsets, *, min_locs, sigma_bounds, lp_abs=False, max_rounds=3, force_scratch=False,
               progress=None) -> G5MModels:
    """``_find_optimal_G5M_2D`` of every cluster ``[offsets[c], offsets[c + 1])`` of the float64 rows in one device call
    (pmi_g5m_fit).  ``progress(round, clusters, device_ms)`` is called after every round."""
    _lib.require_gpu()
    x, y, lp, offsets = _g5m_rows(x, y, lp, offsets)
    sizes = np.diff(offsets)
    caps = np.minimum(G5M_MAX_K, sizes // int(min_locs))
    out = _g5m_empty(caps)
    if not len(sizes):
        return out
    table, first, uniform = g5m_table(sizes, caps)
    cb = G5M_PROGRESS((lambda r, n, ms, _u: progress(int(r), int(n), float(ms))) if progress else 0)
    flags = (G5M_LP_ABS if lp_abs else 0) | (G5M_FORCE_SCRATCH if force_scratch else 0)
    with _lib.lock():
        _lib.call("pmi_g5m_fit", _lib.ptr(x), _lib.ptr(y), _lib.ptr(lp), _lib.ptr(offsets), len(sizes), _lib.ptr(table), _lib.ptr(first),
                  len(first), _lib.ptr(uniform), len(uniform), int(min_locs), float(sigma_bounds[0]), float(sigma_bounds[1]),
                  int(max_rounds), flags, _lib.ptr(out.model), _lib.ptr(out.imodel), int(caps.sum()), _lib.ptr(out.info),
                  _lib.ptr(out.bic), cb, None)
    return out


def g5m_fit_fixed(x, y, lp, offsets, n_components, *, min_locs, sigma_bounds, lp_abs=False, means_init=None,
                  force_scratch=False) -> G5MModels:
    """``G5M_2D(n_components, ...).fit`` of every cluster in one device call (pmi_g5m_fit_fixed); ``means_init`` is
    (clusters, n_components, 2) or None."""
    _lib.require_gpu()
    x, y, lp, offsets = _g5m_rows(x, y, lp, offsets)
    K = int(n_components)
    if not 1 <= K <= G5M_MAX_K:
        raise ValueError(f"n_components must be 1 .. {G5M_MAX_K}")
    sizes = np.diff(offsets)
    caps = np.where(sizes >= K, K, 0).astype(np.int64)
    out = _g5m_empty(np.full(len(sizes), K, np.int64))
    if not len(sizes):
        return out
    table, first, uniform = g5m_table(sizes, caps)
    table[:, 0] = out.start
    if means_init is not None:
        means_init = np.ascontiguousarray(means_init, np.float64)
        if means_init.shape != (len(sizes), K, 2):
            raise ValueError(f"means_init must have the shape {(len(sizes), K, 2)}")
    flags = (G5M_LP_ABS if lp_abs else 0) | (G5M_FORCE_SCRATCH if force_scratch else 0)
    with _lib.lock():
        _lib.call("pmi_g5m_fit_fixed", _lib.ptr(x), _lib.ptr(y), _lib.ptr(lp), _lib.ptr(offsets), len(sizes), _lib.ptr(table),
                  _lib.ptr(first), len(first), _lib.ptr(uniform), len(uniform), _lib.ptr(means_init), K, int(min_locs),
                  float(sigma_bounds[0]), float(sigma_bounds[1]), flags, _lib.ptr(out.model), _lib.ptr(out.imodel), len(sizes) * K,
                  _lib.ptr(out.info), _lib.ptr(out.bic))
    return out


class G5MAssigned(NamedTuple):
    """Per row ``label`` (int32) and ``log_likelihood``; per component slot of the models ``stats`` (total x 7: G5M_STATS),
    ``n_events`` and ``col_means`` (columns x total); per cluster ``group_ll``; optionally per cluster the (n, n_valid) log
    probabilities without and with the weights."""
    label: np.ndarray
    log_likelihood: np.ndarray
    stats: np.ndarray
    n_events: np.ndarray
    group_ll: np.ndarray
    col_means: np.ndarray
    log_prob: list
    weighted_log_prob: list


def g5m_assign(x, y, lp, frame, offsets, models: G5MModels, cols=None, *, f32=True, frame_u32=False, probs=False) -> G5MAssigned:
    """What ``_convert_G5M_results`` computes per cluster from its model, in one device call (pmi_g5m_assign).  ``f32``:
    x and y came from a float32 table (the reference then accumulates the quadratic form in float32)."""
    _lib.require_gpu()
    x, y, lp, offsets = _g5m_rows(x, y, lp, offsets)
    frame = np.ascontiguousarray(frame, np.float64)
    n_rows, C, total = len(x), len(offsets) - 1, models.model.shape[1]
    cols = np.zeros((0, n_rows), np.float64) if cols is None else np.ascontiguousarray(cols, np.float64).reshape(-1, n_rows)
    sizes = np.diff(offsets)
    blocks = sizes * models.info[:, 1]
    table = np.ascontiguousarray(np.stack([models.start, np.cumsum(blocks) - blocks], axis=1), np.int64)
    n_prob = int(blocks.sum()) if probs else 0
    out = G5MAssigned(np.zeros(n_rows, np.int32), np.zeros(n_rows, np.float64), np.zeros((total, len(G5M_STATS)), np.float64), np.zeros(total, np.int32),
                      np.zeros(C, np.float64), np.zeros((len(cols), total), np.float64), [], [])
    lp_out = np.zeros(max(n_prob, 1), np.float64) if probs else None
    wlp_out = np.zeros(max(n_prob, 1), np.float64) if probs else None
    flags = (G5M_QUAD_F32 if f32 else 0) | (G5M_FRAME_U32 if frame_u32 else 0)
    if C:
        with _lib.lock():
            _lib.call("pmi_g5m_assign", _lib.ptr(x), _lib.ptr(y), _lib.ptr(lp), _lib.ptr(frame), _lib.ptr(offsets), C, _lib.ptr(table),
                      _lib.ptr(np.ascontiguousarray(models.model)), _lib.ptr(np.ascontiguousarray(models.imodel)), total,
                      _lib.ptr(np.ascontiguousarray(models.info)), _lib.ptr(cols) if len(cols) else None, len(cols), flags,
                      _lib.ptr(out.label), _lib.ptr(out.log_likelihood), _lib.ptr(out.stats), _lib.ptr(out.n_events),
                      _lib.ptr(out.group_ll), _lib.ptr(out.col_means) if len(cols) else None, _lib.ptr(lp_out), _lib.ptr(wlp_out), n_prob)
    if probs:
        for c in range(C):
            s, shape = slice(int(table[c, 1]), int(table[c, 1] + blocks[c])), (int(sizes[c]), int(models.info[c, 1]))
            out.log_prob.append(lp_out[s].reshape(shape)), out.weighted_log_prob.append(wlp_out[s].reshape(shape))
    return out
