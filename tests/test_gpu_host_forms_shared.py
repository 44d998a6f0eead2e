"""The host-pointer entry points stage through one layer (``pmi::Staged`` and the slot table of csrc/pmi_common.h) without
treading on each other or on the ``_dev`` forms they call.

GPU tier.  Slots across modules: one small call of every host form runs interleaved, forwards and backwards, straight
after ``pmi_release_scratch`` and again after one larger call of each kind has made every slot grow; every small result
equals its expectation by the rule of the test that owns that golden or input (tests/test_gpu_parity.py, test_gpu_zfit.py,
test_gpu_rcc_edges.py, test_gpu_aim_edges.py, test_gpu_frc.py, test_gpu_pickkin.py, test_oracle_golden.py).  Layout edges:
N = 0, 1, 3 and 257 rows, where every piece of the aligned layout is shorter than, or one row past, what the packed
layout held; the same spot gives the same bits wherever it lies in the buffer.  Host form against ``_dev`` form on torch
tensors: the same kernel on the same bytes, so every output bit is equal.  ``pmi_cumexp_fit`` without values and with an
empty first segment returns what it returned before the staging moved (recorded once, below).  ``pmi_aim_roi_cc``
twice in a row, the smaller table first, in each key mode."""
import ctypes
import sys

import numpy as np
import pytest

from conftest import GOLDEN, golden

sys.path.insert(0, GOLDEN)
import _aim_restate as aim_rs  # noqa: E402
import _frc_restate as frc_rs  # noqa: E402
import _pickkin_restate as kin_rs  # noqa: E402
import _zfit_restate as zr  # noqa: E402

import _rcc_cases as rc  # noqa: E402
from test_gpu_parity import _check_fit, _check_lq  # noqa: E402
from test_gpu_rcc_edges import check_image, check_pairs  # noqa: E402
from test_gpu_zfit import _assert_theta, _sequential_sum, _spots, assert_bits  # noqa: E402

from picasso_amd import _lib, backend, masking  # noqa: E402

pytestmark = pytest.mark.gpu


def same_bits(a, b):
    """Equal dtype, shape and bytes; a NaN equals a NaN."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    nan = (a != a) & (b != b) if a.dtype.kind == "f" else np.zeros(a.shape, bool)
    word = {4: np.uint32, 8: np.uint64}[a.dtype.itemsize]
    return bool(((a.view(word) == b.view(word)) | nan).all())


# ---- inputs -------------------------------------------------------------------------------------------------------------------
def blobs(n, box, seed):
    """(n, box, box) float32 spots: one Gaussian emitter near the centre on a flat background, Poisson noise."""
    rng = np.random.default_rng(seed)
    h = box // 2
    y, x = np.mgrid[-h:h + 1, -h:h + 1]
    a, bg, s = rng.uniform(500, 4000, n), rng.uniform(2, 30, n), rng.uniform(0.8, 1.4, n)
    cy, cx = rng.uniform(-0.7, 0.7, (2, n))
    mean = [a[i] / (2 * np.pi * s[i] ** 2) * np.exp(-0.5 * ((x - cx[i]) ** 2 + (y - cy[i]) ** 2) / s[i] ** 2) + bg[i] for i in range(n)]
    return rng.poisson(np.array(mean)).astype(np.float32)


def widths(n, seed):
    return np.random.default_rng(seed).uniform(0.6, 3.2, (2, n)).astype(np.float32)


def windows(n, box, seed):
    """(n, box, box) float64 correlation windows as tests/test_gpu_parity.py::test_peak_fit_device_vs_oracle draws them."""
    rng = np.random.default_rng(seed)
    h = box // 2
    y, x = np.mgrid[-h:h + 1, -h:h + 1]
    out = []
    for t in range(n):
        a = rng.uniform(5, 500); xc, yc = rng.uniform(-0.7, 0.7, 2); s = rng.uniform(0.6, 2.5)
        b = rng.uniform(0, 50) if t % 3 else 0.0
        roi = a * np.exp(-0.5 * ((x - xc) ** 2 + (y - yc) ** 2) / s ** 2) + b + rng.normal(0, 0.02 * a, (box, box))
        out.append(np.abs(roi) if t % 2 else np.maximum(roi, 0.0))
    return np.array(out)


def gradient_case(n, side, seed):
    """A float32 image of `side` pixels, n positions whose box-5 window and its ring stay inside, and the golden's tables."""
    g = golden("surface_cases")
    rng = np.random.default_rng(seed)
    image = rng.uniform(0, 4000, (side, side)).astype(np.float32)
    y, x = rng.integers(3, side - 3, (2, n)).astype(np.int32)
    return image, y, x, g["ng5_uy"], g["ng5_ux"]


def dark_times(n_seg, seed):
    """n_seg segments of 4 .. 40 exponential samples (float64), the third one empty -> (values, offsets)."""
    rng = np.random.default_rng(seed)
    lens = rng.integers(4, 41, n_seg)
    lens[2] = 0
    offsets = np.concatenate(([0], np.cumsum(lens))).astype(np.int64)
    return rng.exponential(30.0, int(offsets[-1])).round(3), offsets


def calibration():
    g = golden("zfit_calib3d")
    return np.ascontiguousarray(g["cx"], np.float64), np.ascontiguousarray(g["cy"], np.float64)


# ---- slots across modules -----------------------------------------------------------------------------------------------------
def small_cases():
    """name -> a small call of one host form that asserts its result by the rule of the test owning the golden.  Every
    reference is computed here, once."""
    from oracle import oracle as orc
    mle, lq = golden("gaussmle_poisson5"), golden("gausslq_testdata_real")
    lq_ref = orc.gausslq(lq["spots"], full=True, threads=4)
    adv, cut, movie = golden("identify_adversarial"), golden("get_spots_testdata"), golden("testdata_movie")["movie"]
    order = np.lexsort((adv["d_x"], adv["d_y"], adv["d_frame"]))
    surf, rcc_g, frc_g, kin_g = golden("surface_cases"), golden("undrift_rcc"), golden("frc_cases"), golden("pickkin_cases")
    (_, wsx, wsy, cx, cy), = zr.widths_set()
    z_ref, sq_ref = zr.fit(wsx, wsy, cx, cy)
    roi_spots = _spots(40, 7, 740)
    known = rc.known_shift_case(33, 32)
    wins = windows(12, 5, 3)
    peak_ref = [orc.peak_fit(w) for w in wins]
    radial = np.random.default_rng(33).integers(-1000, 1000, (33, 33)).astype(np.float64)
    tag, s, roi_cc, peak, mode, ref, tgt, rel, d, W, H, sh = next(aim_rs.golden_rounds(golden("aim_edge_cases"), "ties_signs_f32"))
    frc_ims = [frc_rs.render_hist(frc_g["dense_33/x"][frc_g[f"dense_33/idx{h}"]], frc_g["dense_33/y"][frc_g[f"dense_33/idx{h}"]], 8.0,
                                  tuple(tuple(float(v) for v in row) for row in frc_g["dense_33/viewport"])) for h in "12"]

    def zfit():
        assert_bits(*backend.zfit_arrays(wsx, wsy, cx, cy), z_ref, sq_ref, "widths")

    def avgroi():
        _assert_theta(backend.avgroi_array(roi_spots), _sequential_sum(roi_spots), "box 7 n 40")

    def gaussmle():
        th, cr, ll, it = backend.gaussmle_arrays(mle["spots"], 1e-3, 100, "sigmaxy")
        _check_fit(th, cr, ll, it, mle["sigmaxy_theta"], mle["sigmaxy_crlb"], mle["sigmaxy_loglik"], mle["sigmaxy_iterations"])

    def get_spots():
        b, se, g = cut["cam_emccd"]
        assert np.array_equal(backend.get_spots_array(movie, cut["frame"], cut["y"], cut["x"], 7, b, se, g), cut["spots_emccd"])

    def gausslq():
        th, info, nfev = backend.gausslq_arrays(lq["spots"], full_output=True)
        _check_lq(th, info, nfev, *lq_ref)
        assert np.max(np.abs(th[:, :2] - lq["theta"][:, :2])) < 5e-3 and np.max(np.abs(th[:, 4:] - lq["theta"][:, 4:])) < 5e-3
        assert np.max(np.abs(th[:, 2] - lq["theta"][:, 2]) / lq["theta"][:, 2]) < 5e-3

    def identify():
        got = backend.identify_arrays(adv["movie"], float(adv["d_min_ng"]), int(adv["d_box"]),
                                      ((int(adv["d_roi"][0]), int(adv["d_roi"][1])), (int(adv["d_roi"][2]), int(adv["d_roi"][3]))), None)
        for a, k in zip(got, ("d_frame", "d_y", "d_x", "d_ng")):
            assert np.array_equal(a, adv[k][order]), k

    def net_gradient():
        got = backend.net_gradient_array(surf["ng5_frame"], surf["ng5_y"], surf["ng5_x"], 5, surf["ng5_uy"], surf["ng5_ux"])
        assert np.array_equal(got, surf["ng5_ng"])

    def xcorr():
        check_image(known.segments[0], known.segments[1], "known shift 33 x 32")

    def rcc_pairs():
        check_pairs(known)

    def rcc_shifts():
        seg = rcc_g["segments"]
        shifts, status = backend.rcc_shifts_arrays(seg, 32, 5)
        pairs = [(i, j) for i in range(len(seg) - 1) for j in range(i + 1, len(seg))]
        for p, (i, j) in enumerate(pairs):
            assert status[p] > 0
            assert abs(shifts[p, 0] - rcc_g["raw_shift_y"][i, j]) < 1e-6 and abs(shifts[p, 1] - rcc_g["raw_shift_x"][i, j]) < 1e-6

    def peak_fit():
        popt, status = backend.peak_fit_arrays(wins)
        for k, (o, ost, _) in enumerate(peak_ref):
            assert status[k] == ost, (k, status[k], ost)
            assert np.max(np.abs(popt[k, 1:3] - o[1:3])) < 1e-7 and abs(popt[k, 3] - o[3]) < 1e-6 * max(1.0, o[3])

    def cumexp():
        rates = backend.kinetic_rates(kin_g["edges_f64_values"], kin_g["edges_f64_offsets"])
        kin_rs.check_batch(kin_g, "edges_f64", np.stack([rates.a, rates.t, rates.c, rates.cost]), np.stack([rates.iterations, rates.status]))

    def frc_curve():
        sums, curve, m1, m2 = frc_host(frc_ims[0], frc_ims[1], masking.tukey_profile(33))
        assert same_bits(curve, frc_rs.curve_of(*sums)) and same_bits(m1, frc_g["dense_33/masked1"]) and same_bits(m2, frc_g["dense_33/masked2"])

    def radial_sum():
        assert np.array_equal(backend.radial_sum_array(radial), frc_rs.radial_sum_exact(radial).astype(np.float64))

    def aim_roi_cc():
        assert np.array_equal(backend.aim_roi_cc_arrays(mode, ref[:2], tgt[:2], rel, d, W, H, sh), roi_cc)

    return {f.__name__: f for f in (zfit, avgroi, gaussmle, get_spots, gausslq, identify, net_gradient, xcorr, rcc_pairs, rcc_shifts,
                                    peak_fit, cumexp, frc_curve, radial_sum, aim_roi_cc)}


def frc_host(im1, im2, w):
    """pmi_frc_curve on host arrays -> sums (3, rings), curve, the two masked images."""
    m = im1.shape[0]
    n = m if m % 2 else m - 1
    rings = n // 2 + 1
    im1, im2, w = (np.ascontiguousarray(a, t) for a, t in ((im1, np.float32), (im2, np.float32), (w, np.float64)))
    sums, curve = np.empty((3, rings), np.float64), np.empty(rings, np.float64)
    m1, m2 = np.empty((n, n), np.float32), np.empty((n, n), np.float32)
    with _lib.lock():
        _lib.call("pmi_frc_curve", _lib.ptr(im1), _lib.ptr(im2), m, _lib.ptr(w), _lib.ptr(sums), _lib.ptr(curve), _lib.ptr(m1), _lib.ptr(m2))
    return sums, curve, m1, m2


def larger_calls():
    """One call of each kind on about sixteen times the rows or pixels of its small case: every slot it uses grows.
    Status (the wrappers raise on any other than PMI_OK) and shapes only."""
    cx, cy = calibration()
    rng = np.random.default_rng(16)
    sx, sy = widths(4200, 1)
    assert backend.zfit_arrays(sx, sy, cx, cy)[0].shape == (4200,)
    assert backend.avgroi_array(blobs(640, 7, 2)).shape == (640, 6)
    assert backend.gaussmle_arrays(blobs(512, 5, 3), 1e-3, 100)[0].shape == (512, 6)
    assert backend.gausslq_arrays(blobs(480, 7, 4)).shape == (480, 6)
    movie = rng.poisson(20.0, (24, 128, 128)).astype(np.uint16)
    fr, y, x, ng = backend.identify_arrays(movie, 30.0, 7)
    assert len(fr) == len(y) == len(x) == len(ng) > 500
    assert backend.get_spots_array(movie, fr, y, x, 7, 0, 1, 1).shape == (len(fr), 7, 7)
    image, py, px, uy, ux = gradient_case(560, 128, 5)
    assert backend.net_gradient_array(image, py, px, 5, uy, ux).shape == (560,)
    # an FFT plan takes about a second to make: the images keep the 64 x 64 of the small cases, there are 24 of them
    seg = rng.poisson(3.0, (24, 64, 64)).astype(np.float64)
    chain = [(i, i + 1) for i in range(23)]
    assert backend.xcorr_array(seg[0], seg[1]).shape == (64, 64)
    assert backend.rcc_pairs_arrays(seg, None, 5, chain)[2].shape == (23, 5, 5)
    assert backend.rcc_shifts_arrays(seg, 32, 5, chain)[0].shape == (23, 2)
    assert backend.peak_fit_arrays(windows(192, 5, 6))[0].shape == (192, 5)
    assert len(backend.kinetic_rates(*dark_times(200, 7)).t) == 200
    ims = rng.poisson(2.0, (2, 129, 129)).astype(np.float32)
    assert frc_host(ims[0], ims[1], masking.tukey_profile(129))[1].shape == (65,)
    assert backend.radial_sum_array(rng.uniform(0, 1, (131, 131))).shape == (66,)
    cols = rng.uniform(0, 32, (2, 20000)).astype(np.float32)
    sh = aim_rs.shifts_xy(0.5, 0.25, 32)[0]
    assert backend.aim_roi_cc_arrays(aim_rs.XY_F32, cols[:, :4000], cols, (0, 0, 0), 0.25, 128.0, 0.0, sh).shape == (len(sh),)


def test_host_forms_share_scratch():
    cases = small_cases()
    order = list(cases) + list(cases)[::-1]
    _lib.call("pmi_release_scratch")                       # every slot starts empty
    for name in order:
        cases[name]()
    larger_calls()
    for name in order:
        cases[name]()


# ---- layout edges ---------------------------------------------------------------------------------------------------------------
SENTINEL = 0x5A


def untouched(*arrays):
    return all((a.view(np.uint8) == SENTINEL).all() for a in arrays)


def sentinels(*specs):
    """Four rows of SENTINEL bytes per (dtype, *tail): what an N = 0 call must leave alone."""
    out = []
    for dtype, *tail in specs:
        a = np.empty((4, *tail), dtype)
        a.view(np.uint8)[...] = SENTINEL
        out.append(a)
    return out


def fit_mle(box):
    spots = blobs(257, box, 50 + box)
    return lambda n: backend.gaussmle_arrays(spots[:n], 1e-3, 100, "sigmaxy")


def fit_lq():
    spots = blobs(257, 7, 77)
    return lambda n: backend.gausslq_arrays(spots[:n], full_output=True)


def fit_z():
    (sx, sy), (cx, cy) = widths(257, 8), calibration()
    return lambda n: backend.zfit_arrays(sx[:n], sy[:n], cx, cy)


def sum_roi():
    spots = blobs(257, 7, 9)
    return lambda n: (backend.avgroi_array(spots[:n]),)


def fit_peak():
    wins = windows(257, 5, 10)
    return lambda n: backend.peak_fit_arrays(wins[:n])


def gradient():
    image, y, x, uy, ux = gradient_case(257, 64, 11)
    return lambda n: (backend.net_gradient_array(image, y[:n], x[:n], 5, uy, ux),)


EDGE_FORMS = {"gaussmle5": lambda: fit_mle(5), "gaussmle7": lambda: fit_mle(7), "gausslq7": fit_lq, "zfit": fit_z, "avgroi": sum_roi,
              "peak_fit5": fit_peak, "net_gradient": gradient}


@pytest.mark.parametrize("form", list(EDGE_FORMS))
def test_rows_give_the_same_bits_wherever_they_lie(form):
    call = EDGE_FORMS[form]()
    whole = call(257)
    assert all(len(a) == 257 for a in whole)
    for n in (1, 3):
        part = call(n)
        for col, (a, b) in enumerate(zip(part, whole)):
            assert len(a) == n and same_bits(a, b[:n]), (form, n, col)
    assert all(len(a) == 0 for a in call(0))


def test_no_rows_is_ok_and_writes_nothing():
    p = _lib.ptr
    spots, th, cr, ll, sq64, z64 = sentinels((np.float32, 7, 7), (np.float32, 6), (np.float32, 6), (np.float32,), (np.float64,), (np.float64,))
    it, info, popt, rois = sentinels((np.int32,), (np.int32,), (np.float64, 5), (np.float64, 5, 5))
    cx, cy = calibration()
    image, y, x, uy, ux = gradient_case(4, 32, 12)
    with _lib.lock():
        for box in (5, 7):
            _lib.call("pmi_gaussmle", p(spots), 0, box, 1e-3, 100, _lib.MLE_METHODS["sigmaxy"], p(th), p(cr), p(ll), p(it))
        _lib.call("pmi_gausslq", p(spots), 0, 7, p(th), p(it), p(info))
        _lib.call("pmi_zfit", p(ll), p(ll), 0, p(cx), p(cy), p(z64), p(sq64))
        _lib.call("pmi_avgroi", p(spots), 0, 7, p(th))
        _lib.call("pmi_peak_fit", p(rois), 0, 5, p(popt), p(it))
        _lib.call("pmi_net_gradient", p(image), 32, 32, p(y), p(x), 0, 5, p(uy), p(ux), p(ll))
    assert untouched(spots, th, cr, ll, sq64, z64, it, info, popt, rois)


# ---- host form equals _dev form -------------------------------------------------------------------------------------------------
def on_device(call, inputs, outputs):
    """call(device pointers of inputs, then of outputs, stream) with torch tensors -> the outputs as NumPy arrays."""
    import torch
    d_in = [backend._to_device(a) for a in inputs]
    dev = d_in[0].device
    d_out = [backend._out(dev, getattr(torch, np.dtype(dtype).name), n, *tail) for dtype, n, *tail in outputs]
    with _lib.lock():
        call(*[backend._dptr(t) for t in d_in], *[backend._dptr(t) for t in d_out], backend._stream(dev))
        return [t.cpu().numpy() for t in d_out]


@pytest.mark.parametrize("n", [3, 257])
def test_dev_forms_equal_the_host_forms(n):
    c = _lib.call
    (sx, sy), (cx, cy) = widths(n, 20), calibration()
    dev = on_device(lambda a, b, z, sq, s: c("pmi_zfit_dev", a, b, n, None, _lib.ptr(cx), _lib.ptr(cy), z, sq, s), (sx, sy),
                    [(np.float64, n), (np.float64, n)])
    assert all(same_bits(a, b) for a, b in zip(backend.zfit_arrays(sx, sy, cx, cy), dev)), "zfit"

    spots = blobs(n, 7, 21)
    dev, = on_device(lambda a, th, s: c("pmi_avgroi_dev", a, n, None, 7, th, s), (spots,), [(np.float32, n, 6)])
    assert same_bits(backend.avgroi_array(spots), dev), "avgroi"

    for box in (5, 7):
        spots = blobs(n, box, 22 + box)
        dev = on_device(lambda a, th, cr, ll, it, s: c("pmi_gaussmle_dev", a, n, None, box, 1e-3, 100, _lib.MLE_METHODS["sigmaxy"], th, cr, ll, it, s),
                        (spots,), [(np.float32, n, 6), (np.float32, n, 6), (np.float32, n), (np.int32, n)])
        assert all(same_bits(a, b) for a, b in zip(backend.gaussmle_arrays(spots, 1e-3, 100, "sigmaxy"), dev)), ("gaussmle", box)

    spots = blobs(n, 7, 23)
    dev = on_device(lambda a, th, info, nfev, s: c("pmi_gausslq_dev", a, n, None, 7, th, info, nfev, s), (spots,),
                    [(np.float32, n, 6), (np.int32, n), (np.int32, n)])
    assert all(same_bits(a, b) for a, b in zip(backend.gausslq_arrays(spots, full_output=True), dev)), "gausslq"

    values, offsets = dark_times(n, 24)
    fit, info = on_device(lambda v, o, fit, info, s: c("pmi_cumexp_fit_dev", v, len(values), o, n, backend.cumexp_kind(values.dtype), fit, info, s),
                          (values, offsets), [(np.float64, 4, n), (np.int32, 2, n)])
    rates = backend.kinetic_rates(values, offsets)
    assert same_bits(np.stack([rates.a, rates.t, rates.c, rates.cost]), fit) and same_bits(np.stack([rates.iterations, rates.status]), info), "cumexp"

    ims = np.random.default_rng(25).poisson(2.0, (2, n, n)).astype(np.float32)
    w = masking.tukey_profile(n)
    sums, curve, m1, m2 = frc_host(ims[0], ims[1], w)
    dev = backend.frc_arrays(ims[0], ims[1], w)
    assert same_bits(sums, dev["sums"]) and same_bits(curve, dev["curve"]), "frc"
    assert same_bits(m1, dev["images"][0]) and same_bits(m2, dev["images"][1]), "frc images"


# ---- pmi_cumexp_fit without values, and with an empty first segment --------------------------------------------------------------
NAN = 0x7FF8000000000000
SAMPLES = [3, 1, 4, 1, 5, 9, 2, 6, 5, 3, 5, 8, 9, 7, 9, 3]
# name -> (dtype, offsets, the bits of fit (a, t, c, cost per segment), info (iterations, status per segment)) as the
# library returned them before the host form staged through pmi::Staged
_NONE = ([0, 0, 0], [[NAN, NAN]] * 4, [[0, 0], [0, 0]])
_FIRST_EMPTY = ([0, 0, 6, 16], [[NAN, 0x401CAEBE3BE4FE28, 0x4029CC6C581ABC66], [NAN, 0x4014CDD40A50EE6E, 0x4022000000000000],
                                [NAN, 0x3FC90217A1EC305E, 0x0], [NAN, 0x3FD8B23F2E98444C, 0x4018FF38FBDE5A94]], [[0, 29, 9], [0, 0, 0]])
CUMEXP_RECORD = {"no_values_i32": (np.int32, *_NONE), "no_values_f32": (np.float32, *_NONE), "first_empty_i32": (np.int32, *_FIRST_EMPTY),
                 "first_empty_f32": (np.float32, *_FIRST_EMPTY), "first_empty_f64": (np.float64, *_FIRST_EMPTY)}


@pytest.mark.parametrize("name", list(CUMEXP_RECORD))
def test_cumexp_without_values_or_with_an_empty_first_segment(name):
    dtype, offsets, fit_bits, info = CUMEXP_RECORD[name]
    values = np.array(SAMPLES[:offsets[-1]], dtype)
    rates = backend.kinetic_rates(values, offsets)
    fit = np.stack([rates.a, rates.t, rates.c, rates.cost])
    assert fit.view(np.uint64).tolist() == fit_bits, [[hex(int(b)) for b in row] for row in fit.view(np.uint64)]
    assert np.stack([rates.iterations, rates.status]).tolist() == info


# ---- pmi_aim_roi_cc twice in a row ------------------------------------------------------------------------------------------------
AIM_PAIRS = {aim_rs.XY_F32: ("ties_signs_f32", "xy1"), aim_rs.XY_F64: ("ties_signs_f64", "xy2"),
             aim_rs.Z_F32: ("z_int_min_and_range_f32", "z1"), aim_rs.Z_F64: ("z_int_min_and_range_f64", "z2")}


@pytest.mark.parametrize("mode", list(AIM_PAIRS))
def test_aim_roi_cc_twice_with_a_growing_table(mode):
    """The smaller call first, so the second finds every staged column too short: the edge fixture's case of the mode,
    then the first segment of the 3-D golden in that mode; count for count (tests/test_gpu_aim_edges.py)."""
    edge, tag = AIM_PAIRS[mode]
    first = next(aim_rs.golden_rounds(golden("aim_edge_cases"), edge))
    second = next(r for r in aim_rs.golden_rounds(golden("aim_cases"), "c_3d_default") if r[0] == tag)
    assert first[4] == second[4] == mode and len(first[6][0]) < len(second[6][0]) and len(first[5][0]) < len(second[5][0])
    n_col = 3 if mode in (aim_rs.Z_F32, aim_rs.Z_F64) else 2
    for tag, s, roi_cc, peak, m, ref, tgt, rel, d, W, H, sh in (first, second):
        got = backend.aim_roi_cc_arrays(m, ref[:n_col], tgt[:n_col], rel, d, W, H, sh)
        assert np.array_equal(got, roi_cc), (edge, tag, s, np.flatnonzero(got != roi_cc)[:8].tolist())
