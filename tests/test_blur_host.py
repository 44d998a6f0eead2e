"""CPU tier of the image blur (csrc/blur.hip) and what is built on it: ``backend.blur_plan`` against the routes the
reference took (tests/golden/blur_cases.npz), ``gaussian_kernel1d`` against scipy's, the header the kernels are compiled
from (csrc/blur_core.h) built as a stand-alone host program (tests/blur_host_driver.cpp) against
scipy.ndimage.gaussian_filter in bits, and the Python layers (``_render_smooth``, ``_render_convolve``,
``find_fiducials``, ``align``, ``align_rcc``) over fakes of the backend calls."""
import inspect
import json
import os
import subprocess
import sys
import types
import warnings

import numpy as np
import pandas as pd
import pytest
from scipy import ndimage

from conftest import GOLDEN, ROOT, golden

sys.path.insert(0, GOLDEN)
import _blur_restate as rs  # noqa: E402

from picasso_amd import _lib, backend, imageprocess, localize, postprocess, render  # noqa: E402

G = golden("blur_cases")


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def untag(t):
    return np.float32(t[1]) if t[0] == "f32" else t[1]


# ---- blur_plan against the reference's routes ---------------------------------------------------------------------
PLANS = list(range(int(G["plan/count"])))


def plan_call(k):
    call = json.loads(str(G[f"plan/{k}/call"]))
    return call["n_y"], call["n_x"], untag(call["blur_width"]), untag(call["blur_height"])


@pytest.mark.parametrize("k", PLANS)
def test_blur_plan_takes_the_reference_route(k):
    n_y, n_x, bw, bh = plan_call(k)
    p = f"plan/{k}/"
    if p + "raises" in G:
        with pytest.raises(Exception) as e:
            backend.blur_plan(n_y, n_x, bw, bh)
        assert type(e.value).__name__ == str(G[p + "raises"])
        return
    plan = backend.blur_plan(n_y, n_x, bw, bh)
    assert plan.route == str(G[p + "route"])
    if plan.route == "spatial":
        sigma = G[p + "sigma"]                                  # (blur_height, blur_width) as gaussian_filter got them
        for axis in (0, 1):
            if p + f"weights_{axis}" in G:                     # what scipy handed to correlate1d for this axis
                assert sigma[axis] > 1e-15 and not plan.skip[axis] and plan.radius[axis] == int(5.0 * float(sigma[axis]) + 0.5)
                assert same(plan.weights[axis], G[p + f"weights_{axis}"])
            else:
                assert sigma[axis] <= 1e-15 and plan.skip[axis] and plan.weights[axis] is None
        assert plan.S == 1.0
    else:
        assert same(plan.weights[0], G[p + "kernel_y"]) and same(plan.weights[1], G[p + "kernel_x"])
        assert plan.radius == (len(plan.weights[0]) // 2, len(plan.weights[1]) // 2) and plan.skip == (False, False)
        assert plan.S == float(G[p + "S"])


def test_the_plan_cases_are_the_ones_asked_for():
    routes = {plan_call(k): (str(G[f"plan/{k}/route"]) if f"plan/{k}/route" in G else str(G[f"plan/{k}/raises"])) for k in PLANS}
    # the flip between 220 and 221 at sigma 1 and between 2020 and 2021 at kernel 101, each axis on its own
    assert routes[(220, 1000, 1, 1)] == routes[(1000, 220, 1, 1)] == routes[(2020, 3000, 10, 10)] == routes[(3000, 2020, 10, 10)] == "direct"
    assert routes[(221, 1000, 1, 1)] == routes[(1000, 221, 1, 1)] == routes[(2021, 3000, 10, 10)] == routes[(3000, 2021, 10, 10)] == "spatial"
    # a kernel above 101 (the next one is 111) takes the FFT route whatever the image
    assert routes[(5000, 5000, 11, 1)] == routes[(5000, 5000, 1, 11)] == "direct"
    # half to even: 10.5 -> 10 (kernel 101, spatial), 0.5 -> 0, 1.5 -> 2, 2.5 -> 2
    assert routes[(100000, 100000, 10.5, 1)] == "spatial"
    assert [backend.blur_plan(500, 500, w, w).kernel for w in (0.5, 1.5, 2.5, 0.4)] == [(1, 1), (21, 21), (21, 21), (1, 1)]
    assert backend.blur_plan(30, 30, 0.5, 2.5).kernel == (21, 1)
    assert backend.blur_plan(300, 300, 1e-16, 0).skip == (True, True) and backend.blur_plan(300, 300, 1, 2e-15).skip == (False, False)
    assert sorted(v for k, v in routes.items() if k[2] != k[2] or k[3] != k[3]) == ["ValueError", "ValueError"]


@pytest.mark.parametrize("sigma", [1.0, 0.3, 1.37, 2.9, 10.49, 0.05, float(np.float32(0.9137))])
def test_gaussian_kernel1d_is_scipys(sigma):
    r = int(5.0 * sigma + 0.5)
    assert same(backend.gaussian_kernel1d(sigma, r), ndimage._filters._gaussian_kernel1d(sigma, 0, r))
    assert same(rs.gaussian_kernel1d(sigma, r), ndimage._filters._gaussian_kernel1d(sigma, 0, r))


# ---- the header, built for the host as a stand-alone program ---------------------------------------------------------
@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    d = tmp_path_factory.mktemp("blur_host")
    exe = str(d / "blur_host_driver")
    subprocess.run([os.environ.get("CXX", "c++"), "-O2", "-std=c++17", "-ffp-contract=off",
                    "-I", os.path.join(ROOT, "picasso_amd", "csrc"), os.path.join(ROOT, "tests", "blur_host_driver.cpp"),
                    "-o", exe], check=True)

    def run(image, wy, wx, round_between, scale=1.0):
        image = np.ascontiguousarray(image, np.float32)
        src, dst = str(d / "in.bin"), str(d / "out.bin")
        with open(src, "wb") as f:
            head = [image.shape[0], image.shape[1], 0 if wy is None else len(wy) // 2, 0 if wx is None else len(wx) // 2,
                    wy is not None, wx is not None, round_between]
            f.write(np.array(head, np.int64).tobytes() + np.float64(scale).tobytes())
            for w in (wy, wx):
                if w is not None:
                    f.write(np.ascontiguousarray(w, np.float64).tobytes())
            f.write(image.tobytes())
        subprocess.run([exe, src, dst], check=True)
        return np.fromfile(dst, np.float32).reshape(image.shape)

    return run


def scipy_blur(image, sigma_y, sigma_x):
    out = np.empty_like(image, dtype=np.float32)
    ndimage.gaussian_filter(image, sigma=(sigma_y, sigma_x), output=out, mode="constant", cval=0.0, truncate=5.0)
    return out


@pytest.mark.parametrize("case", rs.SPATIAL_HOST_CASES, ids=lambda c: "x".join(str(v) for v in c))
def test_host_build_of_the_kernel_terms_equals_scipy_in_bits(case, driver):
    n_y, n_x, sy, sx = case
    image = rs.poisson_image(n_y, n_x, n_y * 7 + n_x)
    plan = backend.spatial_plan(sx, sy)
    want = scipy_blur(image, sy, sx)
    assert same(driver(image, plan.weights[0], plan.weights[1], 1), want)
    assert same(rs.spatial(image, sy, sx), want)                 # and the NumPy restatement the GPU tier leans on


def test_host_build_on_the_direct_route_equals_the_restatement(driver):
    n_y, n_x, bw, bh = rs.DIRECT_CASES[4]
    image = rs.poisson_image(n_y, n_x, 5)
    plan = backend.blur_plan(n_y, n_x, bw, bh)
    assert plan.route == "direct"
    got = driver(image, plan.weights[0], plan.weights[1], 0, 1.0 / plan.S)
    assert same(got, rs.direct(image, rs.kernel_of(bw), rs.kernel_of(bh), bw, bh))
    ref = rs.fft_reference(image, rs.kernel_of(bw), rs.kernel_of(bh), bw, bh)
    assert np.abs(got.astype(np.float64) - ref).max() <= float(G["fft/c"]) * np.abs(ref).max()


def test_the_recorded_fft_noise_and_c():
    dev = G["fft/deviation"]
    assert len(dev) == len(rs.DIRECT_CASES) and float(G["fft/c"]) == 4.0 * dev.max() and 1e-8 < dev.max() < 1e-6
    for k, (n_y, n_x, bw, bh) in enumerate(rs.DIRECT_CASES):     # this machine's scipy against the float64 sum, within c
        image = rs.poisson_image(n_y, n_x, 100 + k)
        kw, kh = rs.kernel_of(bw), rs.kernel_of(bh)
        ref = rs.fft_reference(image, kw, kh, bw, bh)
        assert np.abs(ref - rs.direct_float64(image, kw, kh, bw, bh)).max() <= float(G["fft/c"]) * np.abs(ref).max()


# ---- names, signatures, ABI, refusals ------------------------------------------------------------------------------
def test_signatures_are_the_references():
    recorded = json.loads(str(G["signatures"]))
    where = {"find_fiducials": imageprocess, "align": postprocess, "align_rcc": postprocess}
    assert set(recorded) == {"_render_smooth", "_render_convolve", "_fftconvolve", "render_smooth", "render_convolve",
                             "find_fiducials", "align", "align_rcc"}
    for name, text in recorded.items():
        assert str(inspect.signature(getattr(where.get(name, render), name))) == text, name
    assert postprocess.ALIGN_NAMES == ("align", "align_rcc")


def test_abi_version_and_symbols():
    L = _lib.load()
    assert L.pmi_version() >= 123
    header = open(os.path.join(ROOT, "include", "picasso_hip.h")).read()
    for name in ("pmi_blur_dev", "pmi_blur", "pmi_render_blurred"):
        assert name in _lib.SYMBOLS and hasattr(L, name) and name in header
    assert len(_lib.SYMBOLS["pmi_blur_dev"][1]) == 11 and len(_lib.SYMBOLS["pmi_render_blurred"][1]) == 18


def test_install_leaves_the_new_names_alone():
    mods = {n: types.ModuleType("picasso." + n) for n in
            ("localize", "gaussmle", "gausslq", "zfit", "render", "imageprocess", "postprocess", "aim")}
    new = {"render": ("_render_smooth", "_render_convolve", "_fftconvolve", "render_smooth", "render_convolve"),
           "imageprocess": ("find_fiducials",), "postprocess": postprocess.ALIGN_NAMES}
    for mod, names in new.items():
        for name in names:
            setattr(mods[mod], name, "theirs")
    localize.install(*[mods[n] for n in ("localize", "gaussmle", "gausslq", "zfit", "render", "imageprocess", "postprocess")],
                     picasso_aim=mods["aim"])
    assert all(getattr(mods[mod], name) == "theirs" for mod, names in new.items() for name in names)


def test_the_two_kept_refusals_name_the_way_through():
    locs = pd.DataFrame({"frame": np.zeros(2, np.uint32), "x": np.ones(2, np.float32), "y": np.ones(2, np.float32)})
    info = [{"Height": 32, "Width": 32, "Frames": 1, "Pixelsize": 130.0}]
    for m in ("smooth", "convolve"):
        with pytest.raises(NotImplementedError, match=f"_render_{m}"):
            render.render(locs, info, disp_px_size=26.0, blur_method=m)
    with pytest.raises(NotImplementedError, match=r"imageprocess\.find_fiducials.*box / 2"):
        postprocess.undrift_from_fiducials(locs, info, picks=None)


# ---- the Python layers over fakes of the backend calls ----------------------------------------------------------------
def table(x, y, lpx=None, lpy=None):
    n = len(x)
    return pd.DataFrame({"frame": np.arange(n, dtype=np.uint32), "x": np.asarray(x, np.float32), "y": np.asarray(y, np.float32),
                         "lpx": np.asarray(lpx if lpx is not None else np.full(n, 0.1), np.float32),
                         "lpy": np.asarray(lpy if lpy is not None else np.full(n, 0.2), np.float32)})


@pytest.fixture
def calls(monkeypatch):
    seen = []

    def render_blurred_arrays(x, y, oversampling, y_min, x_min, y_max, x_max, blur_width, blur_height):
        seen.append(dict(x=x, y=y, oversampling=oversampling, view=(y_min, x_min, y_max, x_max), blur=(blur_width, blur_height)))
        return 7, np.zeros((2, 3), np.float32)

    monkeypatch.setattr(backend, "render_blurred_arrays", render_blurred_arrays)
    return seen


def test_render_smooth_passes_one_pixel_of_blur(calls):
    locs = table([1, 2], [3, 4])
    n, image = render._render_smooth(locs, 2.5, 1.0, 2.0, 30.0, 40.0)
    assert n == 7 and image.shape == (2, 3) and len(calls) == 1
    assert calls[0]["blur"] == (1, 1) and calls[0]["oversampling"] == 2.5 and calls[0]["view"] == (1.0, 2.0, 30.0, 40.0)
    assert np.array_equal(calls[0]["x"], locs["x"]) and np.array_equal(calls[0]["y"], locs["y"])
    with pytest.warns(DeprecationWarning, match="'render_smooth' function is deprecated.*_render_smooth instead"):
        render.render_smooth(locs, 1.0, 0, 0, 32, 32)
    for fn, args in ((render._render_smooth, ()), (render.render_smooth, ()), (render._render_convolve, (0.1,)), (render.render_convolve, (0.1,))):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            with pytest.raises(NotImplementedError, match="rotated"):
                fn(locs, 1.0, 0, 0, 32, 32, *args, ang=(0.1, 0, 0))
    assert len(calls) == 2


def test_render_convolve_takes_the_medians_of_the_rows_in_view(calls):
    # view (y 0..10, x 0..10), strict on all four sides: rows 0..3 are on a border or outside, rows 4..8 inside
    x = [0.0, 10.0, 5.0, 5.0, 1.0, 2.0, 3.0, 4.0, 9.5]
    y = [5.0, 5.0, 0.0, 10.0, 1.0, 2.0, 3.0, 4.0, 9.5]
    lpx = [9, 9, 9, 9, 0.1, 0.5, 0.3, 0.2, 0.4]
    lpy = [9, 9, 9, 9, 0.6, 0.8, 0.7, 1.0, 0.9]
    locs = table(x, y, lpx, lpy)
    render._render_convolve(locs, 2.0, 0.0, 0.0, 10.0, 10.0, 0.5)
    bw, bh = calls[0]["blur"]
    # the reference's own expressions: oversampling * max(np.median(float32 column), min_blur_width)
    assert bw == 2.0 * max(np.median(np.asarray(lpx[4:], np.float32)), 0.5) == 1.0
    assert bh == 2.0 * max(np.median(np.asarray(lpy[4:], np.float32)), 0.5) and type(bh) is np.float32 and bh == np.float32(0.8) * 2
    with pytest.warns(DeprecationWarning, match="'render_convolve' function is deprecated.*_render_convolve instead"):
        render.render_convolve(locs, 2.0, 0.0, 0.0, 10.0, 10.0, 0.0)
    assert calls[1]["blur"][0] == 2.0 * np.float32(0.3)
    # no row in view: the zero image, before any median (an empty median would warn and give NaN) and without a device call
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        n, image = render._render_convolve(locs.iloc[:4], 2.5, 0.0, 0.0, 10.0, 10.0, 0.5)
    assert n == 0 and image.shape == (25, 25) and image.dtype == np.float32 and not image.any() and len(calls) == 2


def test_fftconvolve_goes_to_the_plan(monkeypatch):
    seen = []
    monkeypatch.setattr(backend, "blur_with_plan", lambda image, plan: seen.append(plan) or image)
    render._fftconvolve(np.zeros((300, 300), np.float32), 1, 2.9)
    render._fftconvolve(np.zeros((30, 300), np.float32), 1, 1)
    assert [p.route for p in seen] == ["direct", "direct"] and seen[0].kernel == (31, 11)
    render._fftconvolve(np.zeros((700, 300), np.float32), 1, 2.9)
    assert seen[2].route == "spatial" and seen[2].radius == (15, 5)


def test_find_fiducials_over_fakes(monkeypatch):
    seen = {}

    def smooth(locs, oversampling, y_min, x_min, y_max, x_max, ang=None):
        seen["render"] = (oversampling, y_min, x_min, y_max, x_max)
        image = np.zeros((64, 48), np.float32)
        image[10, 20] = 5.0
        return len(locs), image

    def identify(image, threshold, box):
        seen["identify"] = (threshold, box)
        return np.array([10, 30, 50]), np.array([20, 21, 22]), np.zeros(3, np.float32)

    def members(locs, info, picks, pick_size, with_table=False):
        seen["members"] = (list(picks), pick_size)
        return locs, np.array([0, 81, 161, 161 + 80]), np.zeros(241, np.int64)

    monkeypatch.setattr(render, "_render_smooth", smooth)
    monkeypatch.setattr(localize, "identify_in_image", identify)
    monkeypatch.setattr(postprocess, "_circle_members", members)
    locs = table([1.0], [1.0])
    info = [{"Height": 64, "Width": 48, "Frames": 100, "Pixelsize": 100}]
    picks, box = imageprocess.find_fiducials(locs, info)
    assert seen["render"] == (1.0, 0, 0, 64, 48)
    image = smooth(locs, 1, 0, 0, 0, 0)[1]
    assert seen["identify"] == (np.percentile(image.flatten(), 99), 9) and box == 9          # 900 / 100 = 9, odd
    assert seen["members"] == ([(20, 10), (21, 30), (22, 50)], 4.5)
    assert picks == [(20, 10)]                              # 81 > 80 kept, exactly 80 dropped twice
    assert imageprocess.find_fiducials(locs, [{"Height": 64, "Width": 48, "Frames": 100, "Pixelsize": 130}])[1] == 7
    assert imageprocess.find_fiducials(locs, [{"Height": 64, "Width": 48, "Frames": 100, "Pixelsize": 150}])[1] == 7      # 6 -> 7
    with pytest.raises(KeyError):                           # as the reference's render.render (golden: pixelsize_missing)
        imageprocess.find_fiducials(locs, [{"Height": 64, "Width": 48, "Frames": 100}])
    assert str(G["fiducials/pixelsize_missing/raises"]) == "KeyError"


@pytest.fixture
def fake_rcc(monkeypatch):
    """Each channel's shift is read off its first row: x[0] - 10, y[0] - 20 (relative to channel 0 it is what rcc returns)."""
    state = {"renders": 0, "rcc": 0}

    def smooth(locs, oversampling, y_min, x_min, y_max, x_max, ang=None):
        state["renders"] += 1
        assert (oversampling, y_min, x_min, y_max, x_max) == (1.0, 0, 0, 32, 32)
        return len(locs), np.array([[locs["x"].iloc[0], locs["y"].iloc[0]]], np.float64)

    def rcc(images, max_shift=None, callback=None):
        state["rcc"] += 1
        assert max_shift is None
        first = np.array([im[0] for im in images])
        shift_x, shift_y = first[:, 0] - first[0, 0], first[:, 1] - first[0, 1]
        return shift_y * state.get("gain", 1.0), shift_x * state.get("gain", 1.0)

    monkeypatch.setattr(render, "_render_smooth", smooth)
    monkeypatch.setattr(imageprocess, "rcc", rcc)
    return state


def three_channels(z=False):
    out = []
    for dx, dy in ((0.0, 0.0), (0.5, -0.25), (2.0, 1.0)):
        t = pd.DataFrame({"x": np.array([10 + dx, 11 + dx], np.float32), "y": np.array([20 + dy, 21 + dy], np.float32)})
        if z:
            t["z"] = np.array([5.0, 6.0], np.float32)
        out.append(t)
    return out, [[{"Height": 32, "Width": 32, "Frames": 1, "Pixelsize": 130}]] * 3


def test_align_shifts_in_place_and_returns_both_shapes(fake_rcc):
    locs, infos = three_channels()
    got = postprocess.align(locs, infos)
    assert got is locs and fake_rcc == {"renders": 3, "rcc": 1}
    for t in locs:
        assert np.array_equal(t["x"], [10, 11]) and np.array_equal(t["y"], [20, 21]) and t["x"].dtype == np.float32
    locs, infos = three_channels()
    got, (shift_x, shift_y) = postprocess.align(locs, infos, apply_shifts=False, return_shifts=True)
    assert got is locs and np.array_equal(shift_x, [0, 0.5, 2.0]) and np.array_equal(shift_y, [0, -0.25, 1.0])
    assert np.array_equal(locs[2]["x"], [12, 13])          # not applied
    with pytest.raises(TypeError):
        postprocess.align(locs, infos, False, False)       # apply_shifts is keyword-only
    with pytest.raises(KeyError):
        postprocess.align(locs, [[{"Height": 32, "Width": 32}]] * 3)


@pytest.mark.parametrize("z", [False, True])
def test_align_rcc_works_on_a_copy_and_stops_at_convergence(fake_rcc, z):
    locs, infos = three_channels(z)
    before = [t.copy() for t in locs]
    aligned, shifts = postprocess.align_rcc(locs, infos, return_shifts=True)
    assert all(a.equals(b) for a, b in zip(locs, before)) and aligned is not locs
    # the first pass removes the shifts, the second finds none: two iterations, one (mean dx, mean dy) pair each
    assert fake_rcc["rcc"] == 2 and len(shifts) == 2 and all(len(s) == 2 for s in shifts)
    assert shifts[0] == (np.mean([0, 0.5, 2.0]), np.mean([0, -0.25, 1.0])) and shifts[1] == (0.0, 0.0)
    for t in aligned:
        assert np.array_equal(t["x"], [10, 11]) and np.array_equal(t["y"], [20, 21])
        if z:
            assert np.array_equal(t["z"], [5.0, 6.0])
    only = postprocess.align_rcc(locs, infos)
    assert isinstance(only, list) and len(only) == 3


def test_align_rcc_stops_at_five(fake_rcc):
    fake_rcc["gain"] = 0.5                                  # every pass removes half of what is left: 2 * 0.5 ** 5 > 0.001
    locs, infos = three_channels()
    aligned, shifts = postprocess.align_rcc(locs, infos, return_shifts=True)
    assert fake_rcc["rcc"] == 5 and len(shifts) == 5
    assert aligned[2]["x"].iloc[0] == pytest.approx(10 + 2.0 * 0.5 ** 5)
