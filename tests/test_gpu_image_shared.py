"""The image kernels (csrc/render.hip, render_rot.hip, blur.hip) share the scratch slots, the staging of the host forms
and the Gaussian driver of csrc/render_common.h without treading on each other.

GPU tier: in one process the flat Gaussian, the rotated Gaussian, the blurred render, the plain blur, the flat and the
rotated histogram run interleaved, forwards and backwards, on one small case each of the committed goldens, straight
after ``pmi_release_scratch`` and again after one larger call of each kind has made every slot grow; every result
equals its golden expectation by the rule of the test that owns that golden (tests/test_gpu_parity.py,
test_gpu_rotrender.py, test_gpu_blur.py).  The flat ``_dev`` forms on torch tensors equal the host forms in every bit of
image and count.  Host tier: the wrappers' viewport helper."""
import ctypes
import json
import sys

import numpy as np
import pytest

from conftest import GOLDEN, golden

sys.path.insert(0, GOLDEN)
import _rotrender_restate as rot_rs  # noqa: E402

from picasso_amd import _lib, backend, render  # noqa: E402


def same_bits(a, b):
    assert a.shape == b.shape and a.dtype == b.dtype == np.float32, (a.shape, b.shape, a.dtype, b.dtype)
    return not ((a.view(np.uint32) != b.view(np.uint32)) & ~(np.isnan(a) & np.isnan(b))).any()


# ---- slots across modules -----------------------------------------------------------------------------------------------------
def small_cases():
    """name -> a call of one small golden case that asserts its result, by the equality rule of the golden's own test."""
    flat, rot, blur = golden("render_cases"), golden("rotrender_cases"), golden("blur_cases")
    (y_min, x_min), (y_max, x_max) = flat["b_viewport"]                              # 32 x 32 pixels, 3000 rows
    flat_view = (float(flat["b_oversampling"]), y_min, x_min, y_max, x_max)
    p = "render/generic/"                                                            # 33 x 65 pixels, 90 rows
    call = json.loads(str(rot[p + "call"]))
    (y_min, x_min), (y_max, x_max) = call["viewport"]
    rot_view = (call["oversampling"], y_min, x_min, y_max, x_max)
    rot_cols = [rot[p + "in_" + c] for c in ("x", "y", "z")] + [rot[p + "matrix"]]
    crop = json.loads(str(blur["render/smooth_crop/call"]))                           # 64 x 80 pixels, the direct route
    (y_min, x_min), (y_max, x_max) = crop["viewport"]
    crop_view = (crop["oversampling"], y_min, x_min, y_max, x_max)
    c = float(blur["fft/c"])

    def flat_gaussian():
        n, img = backend.render_arrays(flat["x"], flat["y"], *flat_view, flat["lpx"], flat["lpy"], float(flat["b_min_blur"]))
        ref = flat["b_gauss_numba"]
        assert n == int(flat["b_n"]) and img.shape == ref.shape and img.dtype == np.float32
        assert (img != ref).mean() < 1e-3 and np.max(np.abs(img - ref)) <= 4e-7 * float(ref.max())

    def flat_hist():
        n, img = backend.render_arrays(flat["x"], flat["y"], *flat_view)
        assert n == int(flat["b_n"]) and np.array_equal(img, flat["b_hist"])

    def rotated_gaussian():
        n, img, _ = backend.render_rot_arrays(*rot_cols, *rot_view, lpx=rot[p + "in_lpx"], lpy=rot[p + "in_lpy"],
                                              lpz=rot[p + "in_lpz"], min_blur_width=call["min_blur_width"])
        assert n == int(rot[p + "_render_gaussian/n"]) and same_bits(img, rot[p + "_render_gaussian/image"])

    def rotated_hist():
        n, img, in_view = backend.render_rot_arrays(*rot_cols, *rot_view)
        assert n == int(rot[p + "_render_hist/n"]) and np.array_equal(in_view, rot[p + "in_view"])
        assert same_bits(img, rot[p + "_render_hist/image"])

    def blurred_render():
        n, img = backend.render_blurred_arrays(blur["render/in_x"], blur["render/in_y"], *crop_view, 1, 1)
        want = blur["render/smooth_crop/image"]
        assert str(blur["render/smooth_crop/route"]) == "direct" and n == int(blur["render/smooth_crop/n"])
        assert img.dtype == np.float32 and img.shape == want.shape
        assert float(np.abs(img.astype(np.float64) - want).max() / np.abs(want).max()) <= c

    def plain_blur():                                        # _render_smooth is the histogram blurred by (1, 1): the spatial route
        img = backend.blur_array(blur["render/hist_os1/image"], 1, 1)
        assert str(blur["render/smooth_os1/route"]) == "spatial" and same_bits(img, blur["render/smooth_os1/image"])

    return {"flat gaussian": flat_gaussian, "rotated gaussian": rotated_gaussian, "blurred render": blurred_render,
            "plain blur": plain_blur, "flat histogram": flat_hist, "rotated histogram": rotated_hist}


def larger_calls():
    """One call of each kind on a 130 x 97 image with 300 rows and a blur radius of 20: every slot the small cases left grows."""
    cols = rot_rs.table(np.random.default_rng(130), 300, 130, 97, 1.0, spread=1.0)
    view, M = (1.0, 0.0, 0.0, 130.0, 97.0), render.to_rotation(rot_rs.EULER["generic"]).as_matrix()
    n, img = backend.render_arrays(cols["x"], cols["y"], *view, cols["lpx"], cols["lpy"])
    assert img.shape == (130, 97) and n == 300
    backend.render_rot_arrays(cols["x"], cols["y"], cols["z"], M, *view, lpx=cols["lpx"], lpy=cols["lpy"], lpz=cols["lpz"])
    plan = backend.blur_plan(130, 97, 4, 4)
    assert plan.route == "direct" and plan.radius == (20, 20)
    n_h, hist = backend.render_arrays(cols["x"], cols["y"], *view)
    n_b, blurred = backend.render_blurred_arrays(cols["x"], cols["y"], *view, 4, 4)
    assert n_h == n_b == hist.sum() == 300 and same_bits(blurred, backend.blur_with_plan(hist, plan))
    backend.render_rot_arrays(cols["x"], cols["y"], cols["z"], M, *view)


@pytest.mark.gpu
def test_image_modules_share_scratch():
    cases = small_cases()
    order = list(cases) + list(cases)[::-1]
    _lib.call("pmi_release_scratch")                       # every slot starts empty
    for name in order:
        cases[name]()
    larger_calls()
    for name in order:
        cases[name]()


# ---- the flat _dev forms against the host forms ------------------------------------------------------------------------------
def seam_rows():
    """33 rows at the corner (32, 32) that four tiles of a 65 x 41 image share: the footprint of every one reaches into the
    first tile, whose list is then one longer than a chunk of the tile kernel."""
    rng = np.random.default_rng(33)
    x, y, lpx, lpy = (rng.uniform(lo, hi, 33).astype(np.float32) for lo, hi in ((29, 33), (29, 33), (0.5, 1.5), (0.5, 1.5)))
    assert ((x - 3 * lpx < 32) & (y - 3 * lpy < 32)).all() and (x + 3 * lpx > 32).any() and (y + 3 * lpy > 32).any()
    return x, y, lpx, lpy


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["seams", "no_rows", "none_in_view"])
def test_flat_dev_forms_equal_the_host_forms(case):
    import torch
    x, y, lpx, lpy = seam_rows()
    if case == "no_rows":
        x, y, lpx, lpy = (a[:0] for a in (x, y, lpx, lpy))
    elif case == "none_in_view":                            # no footprint, no pair: the E == 0 path
        x = x + np.float32(500.0)
    n_rows, n_y, n_x = len(x), 65, 41                       # three by two tiles
    view = (1.0, 0.0, 0.0, float(n_y), float(n_x))
    host_img, host_n = np.empty((n_y, n_x), np.float32), ctypes.c_int64(-1)
    d_cols = [backend._to_device(a) for a in (x, y, lpx, lpy)]
    dev = d_cols[0].device
    for gaussian in (False, True):
        image, count = backend._out(dev, torch.float32, n_y, n_x), backend._out(dev, torch.int64, 1)
        image.fill_(-1.0)
        with _lib.lock():
            if gaussian:
                _lib.call("pmi_render_gaussian", _lib.ptr(x), _lib.ptr(y), _lib.ptr(lpx), _lib.ptr(lpy), n_rows, *view, 0.0, 0,
                          _lib.ptr(host_img), n_y, n_x, ctypes.byref(host_n))
                _lib.call("pmi_render_gaussian_dev", *[backend._dptr(t) for t in d_cols], n_rows, *view, 0.0, 0,
                          backend._dptr(image), n_y, n_x, backend._dptr(count), backend._stream(dev))
            else:
                _lib.call("pmi_render_hist", _lib.ptr(x), _lib.ptr(y), n_rows, *view, _lib.ptr(host_img), n_y, n_x, ctypes.byref(host_n))
                _lib.call("pmi_render_hist_dev", *[backend._dptr(t) for t in d_cols[:2]], n_rows, *view, backend._dptr(image), n_y, n_x,
                          backend._dptr(count), backend._stream(dev))
            dev_img, dev_n = image.cpu().numpy(), int(count.cpu()[0])
        assert dev_n == host_n.value == (33 if case == "seams" else 0)
        assert np.array_equal(dev_img.view(np.uint32), host_img.view(np.uint32))
        assert dev_img.any() == (case == "seams")


# ---- the viewport helper (host tier) --------------------------------------------------------------------------------------------
VIEWS = [(1.0, 0.0, 0.0, 32.0, 32.0), (5.0, 0.0, 0.0, 32.0, 32.0), (7.3, 3.5, 2.25, 20.0, 30.5), (2.5, 1.5, 3.25, 14.7, 29.25),
         (0.37, -4.0, -9.5, 11.0, 2.0), (10.0, 0.0, 0.0, 512.0, 512.0), (1.0, 0.0, 0.0, 1e-9, 1e-9)]


@pytest.mark.parametrize("view", VIEWS)
def test_viewport_helper_gives_the_floats_and_the_dims(view):
    oversampling, y_min, x_min, y_max, x_max = view
    want = (int(np.ceil(oversampling * (y_max - y_min))), int(np.ceil(oversampling * (x_max - x_min))))      # render.py:224-225
    floats, _ = backend._viewport(np.float32(oversampling), *(np.float64(v) for v in view[1:]))      # NumPy scalars come out as floats
    assert all(type(v) is float for v in floats) and floats[1:] == view[1:] and floats[0] == float(np.float32(oversampling))
    assert backend._viewport(*view) == (view, want) and backend.render_dims(*view) == want and min(want) >= 1
    assert backend._viewport(*view, image=False) == (view, None)


@pytest.mark.parametrize("view", [(1.0, 5.0, 0.0, 5.0, 10.0), (1.0, 5.0, 0.0, 4.0, 10.0), (2.0, 0.0, 3.0, 10.0, 3.0), (0.0, 0.0, 0.0, 8.0, 8.0)])
def test_viewport_helper_refuses_an_empty_viewport(view):
    with pytest.raises(ValueError, match="empty viewport"):
        backend._viewport(*view)
    with pytest.raises(ValueError, match="empty viewport"):
        backend.render_dims(*view)
    assert backend._viewport(*view, image=False) == (view, None)
