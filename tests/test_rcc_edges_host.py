"""CPU tier of the RCC correlation stage's edge cases (tests/_rcc_cases.py): every builder holds the situation it is
named for and meets the margin condition of its reference, the project's float64 restatement (oracle.xcorr,
oracle.peak_window) agrees with the exact integer correlation on every integer case, the crop rule is the reference's
formula, and the wrappers refuse a roi below 1 before any device work.  tests/test_gpu_rcc_edges.py runs the same cases
through csrc/xcorr.hip."""
import numpy as np
import pytest

import _rcc_cases as rc
from oracle import oracle
from picasso_amd import _lib, backend

INTEGER_CASES = rc.integer_cases()


@pytest.fixture(scope="module")
def refs():
    """The exact reference of every pair of every integer case, computed once (it asserts the margin condition)."""
    return [[rc.exact_reference(c.segments[i], c.segments[j], c.box, c.roi, c.what) for i, j in rc.pairs_of(c)]
            for c in INTEGER_CASES]


def test_fast_exact_correlation_is_the_definition():
    """One roll per non-zero pixel equals one roll of B per lag, on odd, even and one-row images."""
    for Y, X in ((6, 8), (7, 5), (1, 9), (5, 1)):
        rng = np.random.default_rng(Y * 10 + X)
        a, b = rng.integers(0, 51, (Y, X)), rng.integers(0, 51, (Y, X))
        assert np.array_equal(rc.exact_correlation(a, b), rc.exact_correlation_by_definition(a, b))
    a = np.zeros((5, 6), np.int64); a[1, 2] = 3
    b = np.roll(a, (2, -1), (0, 1))
    c = rc.exact_correlation(a, b)
    assert c[-2 % 5, 1] == 9 and c.sum() == 9                          # B = A moved by s: the only overlap is at lag -s
    assert rc.peak_of_shift(5, 6, 2, -1) == tuple(int(v) for v in np.argwhere(np.fft.fftshift(c) == 9)[0])


def test_images_are_small_non_negative_integers():
    for c in INTEGER_CASES:
        assert c.segments.dtype == np.float64 and c.segments.ndim == 3
        assert rc.is_integer_image(c.segments) and c.segments.min() >= 0 and c.segments.max() <= 50, c.what
        n = len(c.segments)
        assert all(0 <= i < n and 0 <= j < n for i, j in rc.pairs_of(c))
        assert c.box % 2 == 1 and 1 <= c.box <= 15
    sizes = {c.segments.shape[1:] for c in INTEGER_CASES} | {(Y, X) for Y, X, _, _ in rc.BLOBS} | {rc.nan_case().segments.shape[1:]}
    assert len(sizes) <= 12, sizes                                  # every size is a pair of hipFFT plans


def test_every_builder_holds_its_situation(refs):
    for c, rr in zip(INTEGER_CASES, refs):
        e = c.expect
        for k, r in enumerate(rr):
            if r is None:
                continue
            Y, X = c.segments.shape[1:]
            assert (Y - 2 * r.Y_, X - 2 * r.X_) == e.get("crop", (Y - 2 * r.Y_, X - 2 * r.X_)), c.what
            if "peaks" in e:
                assert (r.y_max, r.x_max) == tuple(e["peaks"][k]), (c.what, k)
            if "valid" in e:
                assert (r.window is not None) == bool(e["valid"][k]), (c.what, k)


def test_known_shifts_cover_signs_zero_and_the_wrap():
    for Y, X in rc.KNOWN_SIZES:
        s = rc.known_shifts(Y, X)
        assert (0, 0) in s and any(dy > 0 > dx for dy, dx in s) and any(dy < 0 < dx for dy, dx in s)
        assert any(dy == Y // 2 + 1 and dx == -(X // 2 + 1) for dy, dx in s)
        peaks = rc.known_shift_case(Y, X).expect["peaks"]
        assert peaks[0] == (Y // 2, X // 2)
        assert peaks[3] == (Y - 1, 1 - X % 2)                          # one beyond half the side wraps past the far / near edge
        assert peaks[4] == ((2 * (Y // 2)) % Y, 0)
    assert {(Y % 2, X % 2) for Y, X in rc.KNOWN_SIZES} == {(0, 0), (1, 0), (0, 1), (1, 1)}


def test_crop_rule_is_the_formula_for_every_roi_used():
    rois = {(c.segments.shape[1], c.segments.shape[2], c.roi) for c in INTEGER_CASES}
    assert {(Y, X) for Y, X, roi in rois if roi is not None} >= set(rc.CROP_SIZES)
    for Y, X, roi in rois:
        Y_, X_ = rc.crop_rule(Y, X, roi)
        if roi is None:
            assert (Y_, X_) == (0, 0)
            continue
        want = [int((n - roi) / 2) if int((n - roi) / 2) > 0 else 0 for n in (Y, X)]      # imageprocess.py:90-99
        assert [Y_, X_] == want
        a = np.arange(Y * X, dtype=np.float64).reshape(Y, X)
        cut = a[Y_:-Y_, :] if Y_ > 0 else a
        cut = cut[:, X_:-X_] if X_ > 0 else cut
        assert cut.shape == (Y - 2 * Y_, X - 2 * X_) and cut.size >= 1 and cut[0, 0] == a[Y_, X_]
    for Y, X in rc.CROP_SIZES:
        assert set(rc.crop_rois(Y, X)) >= set(range(Y - 3, Y + 2)) | {1, 2, 8} and max(rc.crop_rois(Y, X)) > max(Y, X)


def test_tiny_and_ragged_crops_are_what_they_claim():
    sizes = {}
    for Y, X in rc.CROP_SIZES:
        for roi in rc.crop_rois(Y, X):
            cy, cx = rc.crop_case(Y, X, roi, 5).expect["crop"]
            sizes[(Y, X, roi)] = cy * cx
    tiny = [n for (Y, X, roi), n in sizes.items() if roi in (1, 2, 8)]
    assert min(tiny) == 1 and all(n < rc.LANES for n in tiny) and len(set(tiny)) >= 4        # most lanes of the reduction stay empty
    assert any(n > rc.LANES and n % rc.LANES for n in sizes.values())                        # not a multiple of the lane count
    c = rc.lanes_257_case(1)
    assert c.expect["crop"] == (1, 257) and 257 == rc.LANES + 1 and c.expect["peaks"][0] == (0, rc.LANES)
    assert rc.crop_rule(1, 257, c.roi) == (0, 0)
    for Y, X in rc.CROP_SIZES:                                                               # tiny crop: the maximum is not element 0
        cy, cx = rc.crop_case(Y, X, 2, 5).expect["crop"]
        ty, tx = rc.crop_case(Y, X, 2, 5).expect["peaks"][0]
        assert ty * cx + tx > 0


def test_box_cases_are_what_they_claim(refs):
    assert [c.box for c in INTEGER_CASES if c.what.startswith("box ") and "on 64x64" in c.what] == list(range(1, 16, 2))
    assert 15 * 15 == 225 < rc.LANES
    c = rc.box15_crop16_case()
    assert rc.crop_rule(64, 64, c.roi) == (24, 24) and c.box == 15
    assert c.expect["peaks"][0] == (8, 8) == (64 // 2 - 24, 64 // 2 - 24)                    # the centre, then one pixel off it
    assert all(max(abs(y - 8), abs(x - 8)) == 1 for y, x in c.expect["peaks"][1:])
    c = rc.crop_smaller_than_box_case()
    assert max(c.expect["crop"]) < c.box


def test_border_cases_are_h_minus_1_h_and_h_plus_1_from_each_border():
    for box in (5, 9):
        c = rc.border_case(box)
        e = c.expect
        h, (cy, cx) = e["h"], e["crop"]
        assert h == box // 2
        seen = set()
        for (y, x), v, d in zip(e["peaks"], e["valid"], e["distance"]):
            dist = min(y, cy - 1 - y, x, cx - 1 - x)                    # to the nearest border
            if d is not None:
                assert dist == d and d in (h - 1, h, h + 1)
                seen.add((d, ("top", "bottom", "left", "right")[[y, cy - 1 - y, x, cx - 1 - x].index(d)]))
            assert v == int(dist >= h)
        assert len(seen) == 12                                          # three distances x four borders
        corners = [(y, x) for (y, x), d in zip(e["peaks"], e["distance"]) if d is None]
        assert (0, 0) in corners and (cy - 1, cx - 1) in corners and (h - 1, h - 1) in corners and (h, h) in corners
        assert len(set(e["peaks"])) == len(e["peaks"])


def test_stride_case_has_its_pixels_past_one_trip_of_the_sum():
    c = rc.stride_case()
    Y, X = c.segments.shape[1:]
    assert Y * X == 19200 and rc.SUM_TRIP == 16384 < Y * X <= 2 * rc.SUM_TRIP
    assert not c.segments[0].any()
    for s, at in c.expect["single"].items():
        assert np.flatnonzero(c.segments[s]).tolist() == [at] and at >= rc.SUM_TRIP
    assert c.expect["single"] == {1: 19199, 2: 16384}
    assert np.count_nonzero(c.segments[3]) > 10 and np.count_nonzero(c.segments[3][: rc.SUM_TRIP // X]) > 0
    for i, j in rc.pairs_of(c):
        r = rc.reference(c, i, j)
        assert (r is None) == (0 in (i, j))
    r = rc.reference(c, 1, 2)                                           # two single pixels correlate to a single pixel
    assert np.count_nonzero(r.image) == 1 and r.image.max() == 21 / np.sqrt(Y * X)


def test_pair_list_cases_are_what_they_claim():
    first, full, without, with_ = rc.pair_list_cases()
    assert (0, 0) in first.pairs and (0, 1) in first.pairs and (1, 0) in first.pairs and first.pairs.count((0, 1)) == 2
    assert full.pairs is None and any(2 in p for p in rc.pairs_of(full))
    assert not any(2 in p for p in without.pairs) and any(2 in p for p in with_.pairs)
    assert full.segments.shape == without.segments.shape and not np.array_equal(full.segments[2], without.segments[2])
    assert without.segments is with_.segments
    for i in range(len(first.segments)):                                # (i, i): the maximum is exactly the centre
        r = rc.reference(first, i, i)
        assert (r.y_max, r.x_max) == (32 // 2 - r.Y_, 32 // 2 - r.X_)
    a, b = rc.reference(first, 0, 1), rc.reference(first, 1, 0)         # (j, i) mirrors (i, j) about the centre
    assert (a.y_max + a.Y_ - 16, a.x_max + a.X_ - 16) == (-(b.y_max + b.Y_ - 16), -(b.x_max + b.X_ - 16)) != (0, 0)


def test_oracle_xcorr_is_the_exact_correlation(refs):
    """numpy's FFT against the integers, within the bound the device is held to."""
    worst = 0.0
    for c, rr in zip(INTEGER_CASES, refs):
        for (i, j), r in zip(rc.pairs_of(c), rr):
            if r is None:
                continue
            got = oracle.xcorr(c.segments[i], c.segments[j])
            dev = np.abs(got - r.image).max() / r.scale
            worst = max(worst, dev)
            assert got.shape == r.image.shape and dev <= rc.BOUND, (c.what, i, j, dev)
    print(f"oracle.xcorr against the exact correlation: largest deviation {worst:.2e} of max |reference|")


def test_oracle_peak_window_is_the_exact_reference(refs):
    for c, rr in zip(INTEGER_CASES, refs):
        for (i, j), r in zip(rc.pairs_of(c), rr):
            got = oracle.peak_window(c.segments[i], c.segments[j], c.box, c.roi)
            if r is None:
                assert got is None, (c.what, i, j)
                continue
            ym, xm, Y_, X_, win = got
            assert (ym, xm, Y_, X_) == (r.y_max, r.x_max, r.Y_, r.X_), (c.what, i, j)
            assert (win is None) == (r.window is None), (c.what, i, j)
            if win is not None:
                assert win.shape == (c.box, c.box) and np.abs(win - r.window).max() <= rc.BOUND * r.scale


def test_nan_pixel_is_not_an_empty_image_in_the_reference():
    """np.sum is NaN, not 0: the pair is correlated, the image is NaN everywhere, argmax is element 0 and the box-5
    window is truncated."""
    c = rc.nan_case()
    assert np.count_nonzero(np.isnan(c.segments)) == 1
    for p, (i, j) in enumerate(c.pairs):
        got = oracle.peak_window(c.segments[i], c.segments[j], c.box, c.roi)
        if p in c.expect["nan_pairs"]:
            assert np.isnan(oracle.xcorr(c.segments[i], c.segments[j])).all()
            assert got == (0, 0, 0, 0, None)
        else:
            assert got[4] is not None


def test_blob_cases_are_benign_and_their_shift_is_known():
    """The oracle's own fit of its own window returns the shift the images were built with: image_shift is the shift
    from A to B, so a B that is A moved by (dy, dx) gives (dy, dx)."""
    for Y, X, dy, dx in rc.BLOBS:
        c = rc.blob_case(Y, X, dy, dx)
        assert not rc.is_integer_image(c.segments) and c.segments.min() > 0
        r = rc.reference(c, 0, 1)
        assert (r.y_max, r.x_max) == c.expect["peaks"][0] and r.window is not None and r.window.min() > 0
        assert np.abs(r.window - r.window[::-1, ::-1]).max() <= 1e-12 * r.scale                  # symmetric about the maximum
        sy, sx = oracle.image_shift_from_window(r.window, c.box, r.y_max, r.x_max, r.Y_, r.X_, Y, X)
        assert abs(sy - dy) < rc.SHIFT_TOL and abs(sx - dx) < rc.SHIFT_TOL, (sy, sx)
    assert {(Y % 2, X % 2) for Y, X, _, _ in rc.BLOBS} == {(1, 0), (0, 1)}


@pytest.mark.parametrize("fn", [backend.rcc_pairs_arrays, backend.rcc_shifts_arrays], ids=["rcc_pairs_arrays", "rcc_shifts_arrays"])
def test_roi_below_one_is_refused_before_device_work(fn, monkeypatch):
    """The library reads roi 0 as "no crop"; the reference with roi=0 crops to nothing (even side) or one row (odd)."""
    monkeypatch.setattr(_lib, "require_gpu", lambda: pytest.fail("device work"))
    segs = np.ones((2, 8, 9))
    for roi in (0, -1, -32, np.int64(0)):
        with pytest.raises(ValueError, match="roi must be None"):
            fn(segs, roi, 5)
    a = np.ones((8, 9))
    assert a[int((8 - 0) / 2):-int((8 - 0) / 2), :].shape[0] == 0 and np.ones((9, 8))[4:-4].shape[0] == 1


@pytest.mark.parametrize("fn", [backend.rcc_pairs_arrays, backend.rcc_shifts_arrays], ids=["rcc_pairs_arrays", "rcc_shifts_arrays"])
def test_roi_none_and_roi_one_reach_the_library(fn, monkeypatch):
    """None stays "no crop" (0 on the C side), an integer of at least 1 passes as it is."""

    class Reached(Exception):
        pass

    def stop():
        raise Reached

    monkeypatch.setattr(_lib, "require_gpu", stop)
    for roi in (None, 1, 32, np.int64(7)):
        with pytest.raises(Reached):
            fn(np.ones((2, 8, 9)), roi, 5)
    assert backend._roi_arg(None) == 0 and backend._roi_arg(1) == 1 and backend._roi_arg(np.int64(7)) == 7
