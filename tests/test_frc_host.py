"""CPU tier of the Fourier ring correlation (picasso_amd/postprocess.py frc / _frc, picasso_amd/imageprocess.py
radial_sum, csrc/frc.hip): the NumPy restatement (tests/golden/_frc_restate.py) gives the bits the reference recorded
(tests/golden/frc_cases.npz) for the masked images, the frequencies and the split; NumPy's float64 transform is nearer
to the longdouble truth than the reference's single-precision curve on every non-degenerate case (what makes the GPU
criterion meaningful); the header the kernels are compiled from (csrc/frc_core.h), built here with the host compiler
(tests/frc_host_driver.cpp), covers every ring bin exactly once; the host code around the device call (threshold walk,
smoothing, argument checks, ABI) is checked without a device."""
import ctypes
import inspect
import os
import subprocess
import sys
import types

import numpy as np
import pandas as pd
import pytest

from conftest import GOLDEN, ROOT, golden

sys.path.insert(0, GOLDEN)
import _frc_restate as rs  # noqa: E402

from picasso_amd import _lib, backend, imageprocess, masking, postprocess  # noqa: E402

G = golden("frc_cases")
CASES = [str(c) for c in G["case_names"]]
KIND = dict(zip(CASES, (str(k) for k in G["kinds"])))
LIVE = [c for c, ok in zip(CASES, G["nondegenerate"]) if ok]
ODD = list(range(1, 130, 2))


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def viewport_of(a):
    return ((float(a[0][0]), float(a[0][1])), (float(a[1][0]), float(a[1][1])))


def test_the_cases_are_the_ones_asked_for():
    assert {int(G[c + "/n"]) for c in CASES} == {1, 3, 5, 31, 33, 37, 63, 65, 129}
    assert {int(G[c + "/m"]) for c in CASES if int(G[c + "/m"]) % 2 == 0} == {4, 34, 64}
    assert set(CASES) - set(LIVE) == {"empty_5", "side_1", "single_3"}
    for c in set(CASES) - set(LIVE):
        assert not G[c + "/R"].any()
    q = G["quadrant_65/masked1"]
    assert q[:32, :32].any() and not q[40:, :].any() and not q[:, 40:].any()       # one quadrant, and the blur around its sites
    assert "frc" in KIND.values() and "_frc" in KIND.values()


@pytest.mark.parametrize("name", CASES)
def test_restatement_gives_the_recorded_bits(name):
    x, y, lp, pixelsize = G[name + "/x"], G[name + "/y"], float(G[name + "/lp"]), float(G[name + "/pixelsize"])
    viewport = viewport_of(G[name + "/viewport"])
    ov = pixelsize / (pixelsize / (1 / (lp / 2)))
    for half in ("1", "2"):
        idx = G[f"{name}/idx{half}"]
        image = rs.render_hist(x[idx], y[idx], ov, viewport)
        assert image.shape == (int(G[name + "/m"]),) * 2
        assert same(rs.masked(image), G[f"{name}/masked{half}"]), (name, half)
    n = int(G[name + "/n"])
    assert same(rs.frequencies(n // 2 + 1, n, pixelsize, lp), G[name + "/frequencies"])
    assert len(G[name + "/R"]) == n // 2 + 1 and G[name + "/R"].dtype == np.float32


@pytest.mark.parametrize("name", [c for c in CASES if KIND[c] == "frc"])
def test_split_and_squaring_equal_the_reference(name):
    idx1, idx2, squared = rs.split(G[name + "/x"], G[name + "/y"], viewport_of(G[name + "/viewport_in"]))
    assert same(idx1.astype(np.int64), G[name + "/idx1"]) and same(idx2.astype(np.int64), G[name + "/idx2"])
    assert same(np.array(squared, np.float64), G[name + "/viewport"])


@pytest.mark.parametrize("name", [c for c in CASES if KIND[c] == "frc"])
def test_frc_hands_the_recorded_halves_to__frc(name, monkeypatch):
    """``postprocess.frc`` up to its call of ``_frc``: squaring, view test, legacy generator, halves, NeNA's s."""
    seen = {}

    def spy(locs1, locs2, pixelsize, lp, viewport):
        seen.update(idx1=locs1.index.to_numpy(), idx2=locs2.index.to_numpy(), pixelsize=pixelsize, lp=lp, viewport=viewport)
        return "curve", "smooth", "freq", "res", "images"

    monkeypatch.setattr(postprocess, "_frc", spy)
    monkeypatch.setattr(postprocess, "nena", lambda locs, info: (None, 0.25))
    locs = pd.DataFrame({"x": G[name + "/x"], "y": G[name + "/y"]})
    out = postprocess.frc(locs, [{"Pixelsize": 130}], viewport_of(G[name + "/viewport_in"]))
    assert out == {"frc_curve": "curve", "frc_curve_smooth": "smooth", "frequencies": "freq", "resolution": "res",
                   "images": "images"}
    assert np.array_equal(seen["idx1"], G[name + "/idx1"]) and np.array_equal(seen["idx2"], G[name + "/idx2"])
    assert same(np.array(seen["viewport"], np.float64), G[name + "/viewport"]) and seen["lp"] == 0.25 and seen["pixelsize"] == 130


@pytest.fixture(scope="module")
def truth():
    return {name: rs.curve_L(G[name + "/masked1"], G[name + "/masked2"]) for name in LIVE}


@pytest.mark.parametrize("name", LIVE)
def test_float64_transform_is_nearer_the_truth_than_the_record(name, truth):
    e_t = rs.err_L(rs.curve_T(G[name + "/masked1"], G[name + "/masked2"]), truth[name])
    e_r = rs.err_L(G[name + "/R"], truth[name])
    print(f"{name}: err_L(T) = {e_t:.3g}, err_L(R) = {e_r:.3g}")
    assert e_t < e_r


def test_the_two_evaluators_agree_on_a_hand_made_spectrum():
    """A single pixel at the centre has a flat spectrum: every ring sum is the ring's bin count."""
    n = 9
    im = np.zeros((n, n), np.float32)
    im[0, 0] = 3.0
    for spectrum in (rs.spectrum_T, rs.spectrum_L):
        num, p1, p2 = rs.sums_of(spectrum(im), spectrum(im), rs.ring_index(n))
        assert np.allclose(np.asarray(num, np.float64), 9.0 * rs.ring_counts(n), rtol=1e-13, atol=0)


@pytest.mark.parametrize("n", ODD)
def test_radial_sum_of_ones_counts_the_ring(n):
    """The restatement's exact sums of an all-ones image are the integer ring counts, and the counts are those of the
    reference's own masks (dist_sq >= r ** 2) & (dist_sq < (r + 1) ** 2)."""
    counts = rs.ring_counts(n)
    assert np.array_equal(np.asarray(rs.radial_sum_exact(np.ones((n, n), np.float32)), np.float64), counts)
    c = n // 2
    yy, xx = np.ogrid[:n, :n]
    d = (xx - c) ** 2 + (yy - c) ** 2
    assert np.array_equal(counts, [np.count_nonzero((d >= r ** 2) & (d < (r + 1) ** 2)) for r in range(c + 1)])


# ---- the header, built for the host -------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("frc_host") / "frc_host.so")
    subprocess.run([os.environ.get("CXX", "c++"), "-O2", "-std=c++17", "-shared", "-fPIC", "-ffp-contract=off",
                    "-I", os.path.join(ROOT, "picasso_amd", "csrc"), os.path.join(ROOT, "tests", "frc_host_driver.cpp"),
                    "-o", out], check=True)
    lib = ctypes.CDLL(out)
    p, i32 = ctypes.c_void_p, ctypes.c_int
    lib.frc_host_cover.argtypes = [i32, i32, p, p, p]
    lib.frc_host_isqrt.argtypes = [ctypes.c_longlong]
    lib.frc_host_window.argtypes = [p, i32, i32, p, p]
    return lib


@pytest.mark.parametrize("n", ODD)
def test_ring_segments_cover_every_bin_once(n, host):
    c = n // 2
    ring = rs.ring_index(n)                                  # centred: [ky + c, kx + c]
    # half plane, unshifted: row ky mod n, column kx in [0, c]
    visits, ring_of, weight = (np.zeros((n, c + 1), np.int32) for _ in range(3))
    assert host.frc_host_cover(n, 0, _lib.ptr(visits), _lib.ptr(ring_of), _lib.ptr(weight)) == 0
    want = np.roll(ring[:, c:], -c, axis=0)                  # ifftshift of the rows
    assert np.array_equal(visits, (want >= 0).astype(np.int32))
    assert np.array_equal(ring_of[want >= 0], want[want >= 0])
    expect_w = np.where(np.arange(c + 1)[None, :] == 0, 1, 2) * (want >= 0)
    assert np.array_equal(weight, expect_w)
    # weighted, the half plane counts the whole ring
    assert np.array_equal(np.bincount(want[want >= 0], weights=weight[want >= 0], minlength=c + 1), rs.ring_counts(n))
    # full plane, centred
    visits, ring_of, weight = (np.zeros((n, n), np.int32) for _ in range(3))
    assert host.frc_host_cover(n, 1, _lib.ptr(visits), _lib.ptr(ring_of), _lib.ptr(weight)) == 0
    assert np.array_equal(visits, (ring >= 0).astype(np.int32))
    assert np.array_equal(ring_of[ring >= 0], ring[ring >= 0])


def test_integer_square_root(host):
    import math
    for v in list(range(0, 70000)) + [k * k + d for k in (4097, 8193, 16385, 23171, 1 << 20) for d in (-1, 0, 1)]:
        assert host.frc_host_isqrt(v) == math.isqrt(v), v


@pytest.mark.parametrize("name", CASES)
def test_host_window_gives_the_recorded_bits(name, host):
    x, y = G[name + "/x"], G[name + "/y"]
    m, n = int(G[name + "/m"]), int(G[name + "/n"])
    w = masking.tukey_profile(n)
    assert same(w, rs.tukey_profile(n)) and same(masking.threshold_tukey(np.zeros((n, n))), w[None, :] * w[::-1][:, None])
    for half in ("1", "2"):
        idx = G[f"{name}/idx{half}"]
        image = np.ascontiguousarray(rs.render_hist(x[idx], y[idx], 8.0, viewport_of(G[name + "/viewport"])))
        out = np.empty((n, n), np.float32)
        host.frc_host_window(_lib.ptr(image), m, n, _lib.ptr(w), _lib.ptr(out))
        assert same(out, G[f"{name}/masked{half}"])


# ---- host code of the package ---------------------------------------------------------------------------------
def test_fire_resolution_on_hand_made_curves():
    f = np.arange(6) / 100.0
    t = 1 / 7
    # a crossing between samples 2 and 3: linear interpolation
    smooth = np.array([1.0, 0.8, 0.5, 0.0, 0.3, 0.0])
    f_res = f[2] + (t - 0.5) * (f[3] - f[2]) / (0.0 - 0.5)
    assert postprocess._fire_resolution(f, smooth) == 1 / f_res
    # no crossing
    assert postprocess._fire_resolution(f, np.full(6, 0.9)) is None
    assert postprocess._fire_resolution(f, np.full(6, 0.01)) is None          # never at or above the threshold first
    assert postprocess._fire_resolution(f[:1], np.array([1.0])) is None
    # a crossing at index 1: the first one counts, the later ones do not
    smooth = np.array([1.0, 0.0, 0.9, 0.0, 0.0, 0.0])
    assert postprocess._fire_resolution(f, smooth) == 1 / (f[0] + (t - 1.0) * (f[1] - f[0]) / (0.0 - 1.0))


def test_loess_smooth_needs_statsmodels(monkeypatch):
    monkeypatch.setitem(sys.modules, "statsmodels", None)
    monkeypatch.setitem(sys.modules, "statsmodels.nonparametric", None)
    monkeypatch.setitem(sys.modules, "statsmodels.nonparametric.smoothers_lowess", None)
    with pytest.raises(ImportError, match="statsmodels"):
        masking.loess_smooth(np.arange(10.0), 5)


def test_loess_smooth_is_statsmodels_lowess():
    sm = pytest.importorskip("statsmodels.nonparametric.smoothers_lowess")
    arr = np.cos(np.arange(40) / 5.0)
    assert same(masking.loess_smooth(arr, 6), sm.lowess(arr, np.arange(40), 7 / 40, return_sorted=False))


def test_abi_has_the_frc_entries():
    lib = _lib.load()
    assert lib.pmi_version() >= 119
    header = open(os.path.join(ROOT, "include", "picasso_hip.h")).read()
    for name in ("pmi_frc_max_side", "pmi_frc_curve", "pmi_frc_curve_dev", "pmi_radial_sum"):
        assert name in _lib.SYMBOLS and hasattr(lib, name) and f"int {name}(" in header
    assert backend.frc_max_side() == backend.FRC_MAX_SIDE and f"#define PMI_FRC_MAX_SIDE {backend.FRC_MAX_SIDE}\n" in header
    assert backend.FRC_MAX_SIDE % 2 == 1 and 2 * (backend.FRC_MAX_SIDE // 2) ** 2 < 1 << 28
    source = open(os.path.join(ROOT, "picasso_amd", "csrc", "rows_common.h")).read()
    assert f"constexpr int BLOCK = {backend.FRC_BLOCK};" in source
    for k, v in {"F32": np.float32, "F64": np.float64, "C64": np.complex64, "C128": np.complex128}.items():
        assert f"#define PMI_RADIAL_{k} {backend.RADIAL_TYPES[np.dtype(v)]}\n" in header


def test_signatures_and_names():
    assert str(inspect.signature(postprocess.frc)).startswith("(locs: 'pd.DataFrame', info, viewport, *, random_seed: 'int' = 42)")
    assert list(inspect.signature(postprocess._frc).parameters) == ["locs1", "locs2", "pixelsize", "lp", "viewport"]
    assert list(inspect.signature(imageprocess.radial_sum).parameters) == ["image"]
    assert postprocess.FRC_NAMES == ("frc", "_frc") and not hasattr(postprocess, "plot_frc")
    assert [n for n in dir(masking) if not n.startswith("_") and callable(getattr(masking, n))] == [
        "loess_smooth", "threshold_tukey", "tukey_profile"]


def test_install_rebinds_frc_and_radial_sum():
    from picasso_amd import localize
    pp, ip = types.SimpleNamespace(frc="theirs", _frc="theirs", plot_frc="theirs"), types.SimpleNamespace(radial_sum="theirs")
    mods = {k: types.SimpleNamespace() for k in ("picasso_localize", "picasso_gaussmle", "picasso_gausslq", "picasso_zfit",
                                                 "picasso_render", "picasso_aim", "picasso_clusterer")}
    localize.install(picasso_postprocess=pp, picasso_imageprocess=ip, **mods)
    assert pp.frc is postprocess.frc and pp._frc is postprocess._frc and pp.plot_frc == "theirs"
    assert ip.radial_sum is imageprocess.radial_sum


def test_argument_checks_that_need_no_device(monkeypatch):
    with pytest.raises(AssertionError, match="square"):
        imageprocess.radial_sum(np.zeros((3, 5), np.float32))
    with pytest.raises(AssertionError, match="odd"):
        imageprocess.radial_sum(np.zeros((4, 4), np.float32))
    with pytest.raises(AssertionError, match="2D"):
        imageprocess.radial_sum(np.zeros(5, np.float32))
    with pytest.raises(TypeError, match="int32"):
        imageprocess.radial_sum(np.zeros((5, 5), np.int32))
    with pytest.raises(AssertionError, match="square"):
        masking.threshold_tukey(np.zeros((3, 5)))
    locs = pd.DataFrame({"x": np.zeros(3, np.float32), "y": np.zeros(3, np.float32)})
    with pytest.raises(KeyError, match="Pixelsize"):
        postprocess.frc(locs, [{"Width": 32}], ((0, 0), (1, 1)))
    monkeypatch.setattr(backend._lib, "require_gpu", lambda: None)
    with pytest.raises(ValueError, match="square"):
        backend.frc_arrays(np.zeros((3, 5), np.float32), np.zeros((3, 5), np.float32), np.ones(3))
    with pytest.raises(ValueError, match="square"):
        backend.frc_arrays(np.zeros((5, 5), np.float32), np.zeros((3, 3), np.float32), np.ones(5))
    with pytest.raises(ValueError, match="profile"):
        backend.frc_arrays(np.zeros((6, 6), np.float32), np.zeros((6, 6), np.float32), np.ones(6))
    with pytest.raises(TypeError, match="float32"):
        backend.frc_arrays(np.zeros((5, 5)), np.zeros((5, 5)), np.ones(5))
    big = np.lib.stride_tricks.as_strided(np.zeros(1, np.float32), (backend.FRC_MAX_SIDE + 2,) * 2, (0, 0))
    with pytest.raises(MemoryError, match=str(backend.FRC_MAX_SIDE)):
        backend.frc_arrays(big, big, np.ones(backend.FRC_MAX_SIDE + 2))
    with pytest.raises(MemoryError, match=str(backend.FRC_MAX_SIDE)):
        backend._frc_side(backend.FRC_MAX_SIDE + 2)
    assert backend._frc_side(backend.FRC_MAX_SIDE + 1) == backend.FRC_MAX_SIDE and backend._frc_side(2) == 1
