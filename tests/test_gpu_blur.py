"""GPU tier of the image blur (csrc/blur.hip): the spatial route against scipy.ndimage.gaussian_filter in every bit, the
direct route against a float64 separable sum in NumPy (in bits) and against scipy.signal.fftconvolve (within ``c`` of its
maximum: four times the reference's own deviation from the float64 sum, measured on the CPU and recorded in
tests/golden/blur_cases.npz), ``pmi_render_blurred`` against the two-step route, and ``_render_smooth``,
``_render_convolve``, ``find_fiducials``, ``align`` and ``align_rcc`` against the reference's recorded results."""
import json
import sys

import numpy as np
import pandas as pd
import pytest
from scipy import ndimage

from conftest import GOLDEN, golden

sys.path.insert(0, GOLDEN)
import _blur_restate as rs  # noqa: E402

from picasso_amd import backend, imageprocess, postprocess, render  # noqa: E402

pytestmark = pytest.mark.gpu
G = golden("blur_cases")
C = float(G["fft/c"])


def differing(a, b):
    assert a.dtype == b.dtype == np.float32 and a.shape == b.shape, (a.dtype, b.dtype, a.shape, b.shape)
    return int((np.ascontiguousarray(a).view(np.uint32) != np.ascontiguousarray(b).view(np.uint32)).sum())


def case_id(c):
    return "x".join(str(v) for v in c)


# ---- the spatial route ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", rs.SPATIAL_CASES, ids=case_id)
def test_spatial_route_equals_scipy_in_every_bit(case):
    n_y, n_x, sy, sx = case
    image = rs.poisson_image(n_y, n_x, n_y * 7 + n_x)
    want = np.empty_like(image)
    ndimage.gaussian_filter(image, sigma=(sy, sx), output=want, mode="constant", cval=0.0, truncate=5.0)
    plan = backend.spatial_plan(sx, sy)
    assert plan.radius == (int(5.0 * sy + 0.5), int(5.0 * sx + 0.5)) and plan.skip == (sy == 0, sx == 0)
    got = backend.blur_with_plan(image, plan)
    print(case, "differing pixels:", differing(got, want))
    assert differing(got, want) == 0
    if backend.blur_plan(n_y, n_x, sx, sy).route == "spatial":          # ... and through the reference's own entry
        assert differing(render._fftconvolve(image, sx, sy), want) == 0


# ---- the direct route --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", range(len(rs.DIRECT_CASES)), ids=lambda k: case_id(rs.DIRECT_CASES[k]))
def test_direct_route_equals_the_float64_sum_in_bits_and_the_fft_within_c(k):
    n_y, n_x, bw, bh = rs.DIRECT_CASES[k]
    image = rs.poisson_image(n_y, n_x, 100 + k)
    kw, kh = rs.kernel_of(bw), rs.kernel_of(bh)
    plan = backend.blur_plan(n_y, n_x, bw, bh)
    assert plan.route == "direct" and plan.kernel == (kh, kw) and plan.radius == (kh // 2, kw // 2)
    got = render._fftconvolve(image, bw, bh)
    want = rs.direct(image, kw, kh, bw, bh)
    ref = rs.fft_reference(image, kw, kh, bw, bh)
    err = float(np.abs(got.astype(np.float64) - ref.astype(np.float64)).max() / np.abs(ref).max())
    print(rs.DIRECT_CASES[k], "differing pixels:", differing(got, want), "| distance to the FFT result:", err, "of its maximum, c =", C)
    assert differing(got, want) == 0
    assert err <= C


# ---- pmi_render_blurred against pmi_render_hist followed by pmi_blur -------------------------------------------------
def render_table():
    return {c: G["render/in_" + c] for c in ("x", "y", "lpx", "lpy")}


@pytest.mark.parametrize("name", ["hist_os1", "hist_empty"])
def test_render_blurred_equals_the_two_steps_in_bits(name):
    call = json.loads(str(G[f"render/{name}/call"]))
    cols = render_table()
    x, y = (cols[c][:0] if call["empty_table"] else cols[c] for c in ("x", "y"))      # the table holds rows on every border
    (y_min, x_min), (y_max, x_max) = call["viewport"]
    n_h, hist = backend.render_arrays(x, y, 1.0, y_min, x_min, y_max, x_max)
    assert n_h == int(G[f"render/{name}/n"]) and differing(hist, G[f"render/{name}/image"]) == 0
    for bw, bh in ((1, 1), (np.float32(0.3), 1.2), (0, 1), (2.2, 2.2)):
        plan = backend.blur_plan(256, 256, bw, bh)
        n, image = backend.render_blurred_arrays(x, y, 1.0, y_min, x_min, y_max, x_max, bw, bh)
        assert n == n_h and differing(image, backend.blur_with_plan(hist, plan)) == 0
    assert backend.blur_plan(256, 256, 2.2, 2.2).route == "direct" and backend.blur_plan(256, 256, 1, 1).route == "spatial"
    if call["empty_table"]:
        assert n_h == 0 and not image.any()


# ---- _render_smooth and _render_convolve against the reference's images ---------------------------------------------
RENDERS = [str(n) for n in G["render/case_names"] if not str(n).startswith("hist")]


@pytest.mark.parametrize("name", RENDERS)
def test_renders_equal_the_reference(name):
    call = json.loads(str(G[f"render/{name}/call"]))
    locs = pd.DataFrame(render_table()).iloc[::call["stride"]]
    (y_min, x_min), (y_max, x_max) = call["viewport"]
    args = (locs, call["oversampling"], y_min, x_min, y_max, x_max) + (() if call["min_blur_width"] is None else (call["min_blur_width"],))
    n, image = getattr(render, call["function"])(*args)
    want, route = G[f"render/{name}/image"], str(G[f"render/{name}/route"])
    assert n == int(G[f"render/{name}/n"]) and image.dtype == np.float32 and image.shape == want.shape
    if route == "direct":
        err = float(np.abs(image.astype(np.float64) - want).max() / np.abs(want).max())
        print(name, "distance to the reference:", err, "of its maximum, c =", C)
        assert err <= C
    else:
        print(name, route, "differing pixels:", differing(image, want))
        assert differing(image, want) == 0


def test_the_render_cases_are_the_ones_asked_for():
    routes = {n: str(G[f"render/{n}/route"]) for n in RENDERS}
    assert routes["smooth_os1"] == routes["smooth_os2p5"] == routes["convolve_below"] == routes["convolve_above"] == "spatial"
    assert routes["smooth_crop"] == routes["convolve_crop"] == "direct"
    assert int(G["render/smooth_out_of_view/n"]) == int(G["render/convolve_out_of_view/n"]) == 0
    lpx = G["render/in_lpx"]
    assert json.loads(str(G["render/convolve_below/call"]))["min_blur_width"] < np.median(lpx) < json.loads(str(G["render/convolve_above/call"]))["min_blur_width"]


# ---- find_fiducials ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [str(n) for n in G["fiducials/case_names"]])
def test_find_fiducials_equals_the_reference(name):
    locs = pd.DataFrame({c: G["fiducials/in_" + c] for c in ("frame", "x", "y", "photons", "lpx", "lpy")})
    info = json.loads(str(G[f"fiducials/{name}/info"]))
    if f"fiducials/{name}/raises" in G:                    # the reference's render.render refuses a missing Pixelsize before
        with pytest.raises(Exception) as e:                 # the 130 nm default can be reached
            imageprocess.find_fiducials(locs, info)
        assert type(e.value).__name__ == str(G[f"fiducials/{name}/raises"])
        return
    picks, box = imageprocess.find_fiducials(locs, info)
    assert type(box) is int and box == int(G[f"fiducials/{name}/box"])
    assert [(int(x), int(y)) for x, y in picks] == [tuple(p) for p in G[f"fiducials/{name}/picks"].tolist()]
    assert len(picks) == 2                                 # 180 and 161 rows kept; exactly 160 rows and the one at the border dropped


# ---- align, align_rcc -------------------------------------------------------------------------------------------------
def channels(name):
    columns = [str(c) for c in G[f"align/{name}/columns"]]
    return [pd.DataFrame({c: G[f"align/{name}/in{k}_{c}"] for c in columns}) for k in range(3)]


@pytest.mark.parametrize("name", ["xy", "xyz"])
def test_align_and_align_rcc_equal_the_reference(name):
    info = json.loads(str(G["align/info"]))
    infos = [info] * 3
    p = f"align/{name}/"
    locs = channels(name)
    got, (shift_x, shift_y) = postprocess.align(locs, infos, return_shifts=True)
    print(name, "align: max |shift - reference| =", max(np.abs(shift_x - G[p + "align_shift_x"]).max(), np.abs(shift_y - G[p + "align_shift_y"]).max()))
    assert got is locs
    assert np.abs(shift_x - G[p + "align_shift_x"]).max() <= 1e-6 and np.abs(shift_y - G[p + "align_shift_y"]).max() <= 1e-6
    fresh = channels(name)
    # a float32 coordinate below 256 moved by a shift that is off by at most 1e-6 lands within that plus one float32
    # spacing (2 ** -16) of the reference's, per subtraction
    step = 1e-6 + 2.0 ** -16
    for k in range(3):                                     # in place: the caller's tables moved, by the shifts returned
        assert locs[k]["x"].dtype == G[f"{p}align_out{k}_x"].dtype == np.float32 and locs[k]["x"].max() < 256
        assert np.abs(locs[k]["x"].to_numpy() - G[f"{p}align_out{k}_x"]).max() <= step
        assert np.abs(locs[k]["y"].to_numpy() - G[f"{p}align_out{k}_y"]).max() <= step
        if k:
            assert not np.array_equal(locs[k]["x"].to_numpy(), fresh[k]["x"].to_numpy())
    before = [t.copy() for t in fresh]
    aligned, shifts = postprocess.align_rcc(fresh, infos, return_shifts=True)
    assert all(a.equals(b) for a, b in zip(fresh, before))
    want = G[p + "rcc_shifts"]
    assert len(shifts) == int(G[p + "iterations"]) and np.shape(shifts) == want.shape
    print(name, "align_rcc:", len(shifts), "iterations, max |shift - reference| =", np.abs(np.array(shifts) - want).max())
    assert np.abs(np.array(shifts) - want).max() <= 1e-6
    for k in range(3):
        assert np.abs(aligned[k]["x"].to_numpy() - G[f"{p}rcc_out{k}_x"]).max() <= len(shifts) * step
        assert np.abs(aligned[k]["y"].to_numpy() - G[f"{p}rcc_out{k}_y"]).max() <= len(shifts) * step
        if name == "xyz":
            assert np.array_equal(aligned[k]["z"].to_numpy(), fresh[k]["z"].to_numpy())
