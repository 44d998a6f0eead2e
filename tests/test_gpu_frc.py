"""GPU tier of the Fourier ring correlation (csrc/frc.hip under picasso_amd/postprocess.py and imageprocess.py).  For
every case of tests/golden/frc_cases.npz the masked images, ``n`` and ``frequencies`` equal the reference's record in
bits; the curve is exactly 0 where the record's is 0 because a ring has no power; and on the non-degenerate cases the
device's curve D is no farther from the longdouble truth L than the reference's single-precision curve R, or within 8
times the error of NumPy's own float64 transform T:  err_L(D) <= max(err_L(R), 8 * err_L(T)).

Seams.  The ring walk has one constant, the 256 lanes of a workgroup (backend.FRC_BLOCK): a ring of at most 256 row
segments gives every lane at most one.  Half plane (FRC): 2 r + 1 <= 256, so ring 127 is the last below the seam and
ring 128 the first above: sides 255 (rings up to 127) and 257 (ring 128 exists).  Full plane (radial_sum):
2 (2 r + 1) <= 256, ring 63 below and ring 64 above: sides 127 and 129.

Bound of the seam cases against T (no longdouble truth at side 257: its two matrix products take too long for a test).
With a flat window and one pixel of value 3 the power of every bin is 9, so a ring sum is 9 times the ring's integer
bin count.  A float64 transform of N = n * n points carries a relative error of a few eps * log2(N) (17 doublings at
n = 257, three transforms on the chirp-z route of a prime side: below 3 * 17 * 4 * 1.1e-16 = 2.3e-14 per bin), and a
sum of c terms of one sign adds at most c * eps = 3e-14: 1e-12 leaves more than an order above both and is seven
orders below one bin of the smallest ring, so a bin counted twice, dropped, or weighted wrongly cannot hide in it."""
import sys

import numpy as np
import pandas as pd
import pytest

from conftest import GOLDEN, golden

sys.path.insert(0, GOLDEN)
import _frc_restate as rs  # noqa: E402

from picasso_amd import backend, imageprocess, masking, postprocess  # noqa: E402

pytestmark = pytest.mark.gpu

G = golden("frc_cases")
CASES = [str(c) for c in G["case_names"]]
KIND = dict(zip(CASES, (str(k) for k in G["kinds"])))
LIVE = {c for c, ok in zip(CASES, G["nondegenerate"]) if ok}
_TRUTH = {}


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def viewport_of(a):
    return ((float(a[0][0]), float(a[0][1])), (float(a[1][0]), float(a[1][1])))


def truth(name):
    """(L, err_L(T), err_L(R)) of a case, computed once and shared."""
    if name not in _TRUTH:
        m1, m2 = G[name + "/masked1"], G[name + "/masked2"]
        L = rs.curve_L(m1, m2)
        _TRUTH[name] = (L, rs.err_L(rs.curve_T(m1, m2), L), rs.err_L(G[name + "/R"], L))
    return _TRUTH[name]


def run(name, monkeypatch):
    """The package's own entry point for the case, the smoothing replaced by the identity (statsmodels is not needed
    to check the curve; nothing of the smoothed curve is recorded)."""
    monkeypatch.setattr(masking, "loess_smooth", lambda arr, span=5: arr)
    x, y = G[name + "/x"], G[name + "/y"]
    lp, pixelsize = float(G[name + "/lp"]), float(G[name + "/pixelsize"])
    locs = pd.DataFrame({"x": x, "y": y, "lpx": np.full(len(x), lp, np.float32), "lpy": np.full(len(x), lp, np.float32)})
    with pytest.warns(DeprecationWarning):
        if KIND[name] == "frc":
            monkeypatch.setattr(postprocess, "nena", lambda locs, info: (None, lp))
            out = postprocess.frc(locs, [{"Pixelsize": pixelsize}], viewport_of(G[name + "/viewport_in"]))
            assert list(out) == ["frc_curve", "frc_curve_smooth", "frequencies", "resolution", "images"]
            return out["frc_curve"], out["frc_curve_smooth"], out["frequencies"], out["resolution"], out["images"]
        return postprocess._frc(locs.iloc[G[name + "/idx1"]], locs.iloc[G[name + "/idx2"]], pixelsize, lp,
                                viewport_of(G[name + "/viewport"]))


@pytest.mark.parametrize("name", CASES)
def test_device_equals_the_record(name, monkeypatch):
    curve, smooth, freq, resolution, images = run(name, monkeypatch)
    n = int(G[name + "/n"])
    assert images[0].shape == (n, n) and same(images[0], G[name + "/masked1"]) and same(images[1], G[name + "/masked2"])
    assert same(freq, G[name + "/frequencies"]) and curve.shape == (n // 2 + 1,) and curve.dtype == np.float64
    assert smooth is curve or same(smooth, curve)
    if name not in LIVE:
        assert not curve.any() and not G[name + "/R"].any() and resolution is None
        return
    # a ring without power: both the record and the device give exactly 0 there
    L, e_t, e_r = truth(name)
    m1, m2 = G[name + "/masked1"], G[name + "/masked2"]
    ring = rs.ring_index(n)
    p1, p2 = (rs.ring_sum(np.abs(rs.spectrum_L(m)) ** 2, ring) for m in (m1, m2))
    dead = (np.asarray(p1 * p2, np.float64) == 0) & (G[name + "/R"] == 0)
    assert not curve[dead].any()
    e_d = rs.err_L(curve, L)
    print(f"{name}: n = {n}, err_L(D) = {e_d:.3g}, err_L(T) = {e_t:.3g}, err_L(R) = {e_r:.3g}")
    assert e_d <= max(e_r, 8 * e_t), (name, e_d, e_t, e_r)


def test_sums_and_curve_belong_together():
    name = "dense_33"
    w = masking.tukey_profile(33)
    im1, im2 = (rs.render_hist(G[name + "/x"][G[f"{name}/idx{h}"]], G[name + "/y"][G[f"{name}/idx{h}"]], 8.0,
                               viewport_of(G[name + "/viewport"])) for h in "12")
    out = backend.frc_arrays(im1, im2, w)
    num, p1, p2 = out["sums"]
    assert same(out["curve"], rs.curve_of(num, p1, p2)) and same(out["images"][0], G[name + "/masked1"])
    L = [np.asarray(v, np.float64) for v in rs.sums_of(rs.spectrum_L(G[name + "/masked1"]), rs.spectrum_L(G[name + "/masked2"]),
                                                        rs.ring_index(33))]
    for mine, theirs in zip(out["sums"], L):
        assert np.allclose(mine, theirs, rtol=1e-12, atol=1e-12 * np.abs(theirs).max())
    assert set(out["ms"]) == {"window", "fft", "rings", "curve"} and all(v >= 0 for v in out["ms"].values())


def flat_power(n):
    """One pixel of value 3 under a flat window: every bin has power 9 (module docstring)."""
    im = np.zeros((n, n), np.float32)
    im[n // 3, n // 2 + 1] = 3.0
    return backend.frc_arrays(im, im, np.ones(n))


@pytest.mark.parametrize("n", [255, 257, 259])
def test_ring_seam_of_the_half_plane(n):
    assert (2 * 127 + 1 <= backend.FRC_BLOCK < 2 * 128 + 1) and (n // 2 >= 128) == (n >= 257)
    out = flat_power(n)
    want = 9.0 * rs.ring_counts(n)
    for k in range(3):
        assert np.max(np.abs(out["sums"][k] / want - 1)) < 1e-12, (n, k)
    assert np.max(np.abs(out["curve"] - 1)) < 1e-12
    # an even render of the next side is cropped to this one
    im = np.zeros((n + 1, n + 1), np.float32)
    im[n // 3, n // 2 + 1] = 3.0
    im[n, :] = 7.0
    im[:, n] = 7.0
    again = backend.frc_arrays(im, im, np.ones(n))
    assert same(again["sums"], out["sums"]) and same(again["curve"], out["curve"])


RADIAL_SIDES = [1, 3, 33, 127, 129, 131]


@pytest.mark.parametrize("dtype", [np.float32, np.float64, np.complex64, np.complex128])
@pytest.mark.parametrize("n", RADIAL_SIDES)
def test_radial_sum_is_exact_on_integral_images(n, dtype):
    """Integers below 2^10 in n * n <= 17161 bins: every partial sum is an integer below 2^24, exact in every type."""
    assert 2 * (2 * 63 + 1) <= backend.FRC_BLOCK < 2 * (2 * 64 + 1)
    rng = np.random.default_rng(n)
    image = rng.integers(-1000, 1000, (n, n)).astype(dtype)
    if np.iscomplexobj(image):
        image = image + 1j * rng.integers(-1000, 1000, (n, n)).astype(dtype)
        image = image.astype(dtype)
    out = imageprocess.radial_sum(image)
    want = rs.radial_sum_exact(image)
    assert out.dtype == np.dtype(dtype) and out.shape == (n // 2 + 1,)
    assert np.array_equal(out, want.astype(dtype))
    ones = imageprocess.radial_sum(np.ones((n, n), dtype))
    assert np.array_equal(ones, rs.ring_counts(n).astype(dtype))


def test_radial_sum_adds_in_float64():
    """Float32 values whose float32 running sum would lose the small terms: the sum is taken in float64, cast once."""
    n = 33
    image = np.full((n, n), 2.0 ** -20, np.float32)
    image[n // 2, :] = 4096.0
    out = imageprocess.radial_sum(image)
    want = np.asarray(rs.radial_sum_exact(image)).astype(np.float32)
    assert same(out, want)


def test_two_calls_and_scratch_reuse_give_the_same_bits():
    rng = np.random.default_rng(5)
    big1, big2 = (rng.poisson(2.0, (257, 257)).astype(np.float32) for _ in range(2))
    small1, small2 = (rng.poisson(2.0, (5, 5)).astype(np.float32) for _ in range(2))
    first = backend.frc_arrays(big1, big2, masking.tukey_profile(257))
    second = backend.frc_arrays(big1, big2, masking.tukey_profile(257))
    small = backend.frc_arrays(small1, small2, masking.tukey_profile(5))
    third = backend.frc_arrays(big1, big2, masking.tukey_profile(257))
    for other in (second, third):
        assert same(first["sums"], other["sums"]) and same(first["curve"], other["curve"])
        assert same(first["images"][0], other["images"][0]) and same(first["images"][1], other["images"][1])
    assert same(small["curve"], backend.frc_arrays(small1, small2, masking.tukey_profile(5))["curve"])
    assert same(first["images"][0], rs.masked(big1)) and same(small["images"][1], rs.masked(small2))
    assert np.max(np.abs(first["curve"] - rs.curve_T(first["images"][0], first["images"][1]))) < 1e-12
    image = rng.integers(0, 9, (129, 129)).astype(np.float64)
    assert same(imageprocess.radial_sum(image), imageprocess.radial_sum(image))
