"""GPU tier of the RCC correlation stage's edge cases: csrc/xcorr.hip (correlation, fftshift, centre crop, maximum, fit
window) against the exact integer correlation of tests/_rcc_cases.py.  Images and windows within 1e-12 of max |reference|;
maximum, crop offsets and ``valid`` by equality (every reference asserts the margin that makes equality meaningful).
tests/test_rcc_edges_host.py holds the cases to what they are named for."""
import numpy as np
import pytest

import _rcc_cases as rc
from picasso_amd import backend

pytestmark = pytest.mark.gpu


def check_pairs(case, got=None):
    """One rcc_pairs_arrays call against the reference of every pair -> what the call returned."""
    got = got or backend.rcc_pairs_arrays(case.segments, case.roi, case.box, case.pairs)
    peak, valid, rois, crop = got
    pairs = rc.pairs_of(case)
    Y, X = case.segments.shape[1:]
    assert peak.shape == (len(pairs), 2) and valid.shape == (len(pairs),) and rois.shape == (len(pairs), case.box, case.box)
    assert crop == rc.crop_rule(Y, X, case.roi)
    worst = 0.0
    for p, (i, j) in enumerate(pairs):
        ref = rc.reference(case, i, j)
        where = (case.what, p, (i, j))
        if ref is None:                                                  # an empty image: shift (0, 0) by definition
            assert valid[p] == -1 and tuple(peak[p]) == (0, 0) and not rois[p].any(), where
            continue
        assert crop == (ref.Y_, ref.X_), where
        assert tuple(peak[p]) == (ref.y_max, ref.x_max), where
        if "peaks" in case.expect:
            assert tuple(peak[p]) == tuple(case.expect["peaks"][p]), where
        assert valid[p] == (1 if ref.window is not None else 0), where
        if ref.window is None:
            assert not rois[p].any(), where
        else:
            dev = float(np.abs(rois[p] - ref.window).max()) / ref.scale
            worst = max(worst, dev)
            assert dev <= rc.BOUND, (where, dev)
    print(f"{case.what}: windows deviate by at most {worst:.2e} of max |reference|")
    return got


def check_image(a, b, what):
    ref = rc.exact_xcorr(a, b)
    got = backend.xcorr_array(a, b)
    dev = float(np.abs(got - ref).max() / np.abs(ref).max())
    print(f"{what}: image deviates by at most {dev:.2e} of max |reference|")
    assert got.shape == ref.shape and got.dtype == np.float64 and dev <= rc.BOUND, (what, dev)
    return got


@pytest.mark.parametrize("Y,X", rc.KNOWN_SIZES)
def test_known_shifts_at_every_parity(Y, X):
    """B is A moved by a known (dy, dx): the maximum lies at (Y/2 - dy, X/2 - dx) modulo the sides, whatever their parity."""
    case = rc.known_shift_case(Y, X)
    for k, (dy, dx) in enumerate(rc.known_shifts(Y, X)):
        got = check_image(case.segments[0], case.segments[k + 1], f"{case.what} ({dy}, {dx})")
        assert np.unravel_index(np.argmax(got), got.shape) == rc.peak_of_shift(Y, X, dy, dx)
    peak, valid, _, _ = check_pairs(case)
    assert sorted(valid.tolist()) == [0, 0, 1, 1, 1]                    # the two wrapped maxima lie on the image border


@pytest.mark.parametrize("Y,X,roi", [(Y, X, roi) for Y, X in rc.CROP_SIZES for roi in rc.crop_rois(Y, X)])
def test_crop_arithmetic(Y, X, roi):
    for box in (5, 1):
        check_pairs(rc.crop_case(Y, X, roi, box))


@pytest.mark.parametrize("box", [1, 5])
def test_crop_of_257_elements(box):
    peak, valid, _, _ = check_pairs(rc.lanes_257_case(box))
    assert valid.tolist() == ([1, 1] if box == 1 else [0, 0])           # one row is lower than box 5


@pytest.mark.parametrize("box", range(1, 16, 2))
def test_every_window_size(box):
    peak, valid, rois, _ = check_pairs(rc.box_sweep_case(box))
    assert valid.tolist() == [1] and rois[0, box // 2, box // 2] == rois[0].max()


def test_box_15_in_a_16x16_crop_and_a_crop_smaller_than_the_box():
    case = rc.box15_crop16_case()
    peak, valid, _, crop = check_pairs(case)
    assert crop == (24, 24) and valid.tolist() == case.expect["valid"] == [1, 1, 0, 0]
    peak, valid, rois, crop = check_pairs(rc.crop_smaller_than_box_case())
    assert crop == (28, 28) and valid.tolist() == [0] and not rois.any()


@pytest.mark.parametrize("box", [5, 9])
def test_maximum_at_the_crop_border(box):
    case = rc.border_case(box)
    peak, valid, rois, _ = check_pairs(case)
    assert valid.tolist() == case.expect["valid"]
    assert not rois[valid == 0].any() and all(r.any() for r in rois[valid == 1])


def test_single_pixels_past_the_stride_of_the_sum_are_not_empty():
    """160 x 120: one trip of sum_kernel's loop covers 16 384 of the 19 200 pixels."""
    case = rc.stride_case()
    peak, valid, rois, _ = check_pairs(case)
    pairs = rc.pairs_of(case)
    assert [v == -1 for v in valid] == [0 in p for p in pairs]
    assert all(v in (0, 1) for v, p in zip(valid, pairs) if 0 not in p)
    # the other order and (i, i) of the single-pixel segments
    check_pairs(case._replace(pairs=[(2, 1), (1, 1), (2, 2), (1, 0), (3, 2), (0, 0)], what=case.what + ", reversed"))


def test_pair_lists():
    first, full, without, with_ = rc.pair_list_cases()
    peak, valid, rois, crop = check_pairs(first)
    Y, X = first.segments.shape[1:]
    for p, (i, j) in enumerate(first.pairs):
        if i == j:
            assert tuple(peak[p]) == (Y // 2 - crop[0], X // 2 - crop[1]) and valid[p] == 1
    assert np.array_equal(peak[2], peak[4]) and np.array_equal(rois[2], rois[4])          # the repeated pair
    assert not np.array_equal(peak[2], peak[3])                                            # (j, i) is not (i, j)
    for roi in (None, 20, 100):
        peak, valid, rois, crop = backend.rcc_pairs_arrays(first.segments, roi, 5, [])
        assert crop == rc.crop_rule(Y, X, roi) and peak.shape == (0, 2) and valid.shape == (0,) and rois.shape == (0, 5, 5)
    shifts, status = backend.rcc_shifts_arrays(first.segments, 20, 5, [])
    assert shifts.shape == (0, 2) and status.shape == (0,)
    # a segment no pair uses is not transformed; its spectrum slot keeps the last call's
    check_pairs(full)
    check_pairs(without)
    check_pairs(with_)


def test_scratch_and_plans_survive_a_smaller_call():
    large, small = rc.reuse_cases()
    one = check_pairs(large)
    check_pairs(small)
    two = check_pairs(large)
    assert one[3] == two[3] and all(np.array_equal(a, b) for a, b in zip(one[:3], two[:3]))   # windows: equal in every bit
    assert one[2].tobytes() == two[2].tobytes()
    assert len(one[0]) == 15 and (one[1] == 1).all()


def test_nan_pixel_is_correlated_not_skipped():
    """np.sum of the image is NaN, not 0, so the reference correlates the pair: the image is NaN everywhere, argmax is
    element 0 and the window there is truncated (tests/test_rcc_edges_host.py asserts this on oracle.peak_window)."""
    case = rc.nan_case()
    peak, valid, rois, crop = backend.rcc_pairs_arrays(case.segments, case.roi, case.box, case.pairs)
    for p in case.expect["nan_pairs"]:
        assert tuple(peak[p]) == (0, 0) and valid[p] == 0 and not rois[p].any(), p
    ok = case._replace(pairs=[(0, 1)])
    check_pairs(ok, (peak[:1], valid[:1], rois[:1], crop))
    assert np.isnan(backend.xcorr_array(case.segments[0], case.segments[2])).all()


@pytest.mark.parametrize("Y,X,dy,dx", rc.BLOBS)
def test_shift_of_a_benign_pair_end_to_end(Y, X, dy, dx):
    """rcc_shifts_arrays returns the shift from A to B: (dy, dx) for a B that is A moved by (dy, dx)."""
    from oracle import oracle
    case = rc.blob_case(Y, X, dy, dx)
    ref = rc.reference(case, 0, 1)
    check_pairs(case)
    want = oracle.image_shift_from_window(ref.window, case.box, ref.y_max, ref.x_max, ref.Y_, ref.X_, Y, X)
    shifts, status = backend.rcc_shifts_arrays(case.segments, case.roi, case.box, case.pairs)
    print(f"{case.what}: shift {shifts[0]} against {want}, status {status[0]}")
    assert status[0] > 0
    assert abs(shifts[0, 0] - want[0]) <= rc.SHIFT_TOL and abs(shifts[0, 1] - want[1]) <= rc.SHIFT_TOL
