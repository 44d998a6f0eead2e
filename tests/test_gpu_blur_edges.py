"""GPU tier of the blur's edge cases (csrc/blur.hip; the lists are tests/golden/_blur_restate.py ``EDGE_*``): radii at,
one above and at multiples of the chunk of either pass, sides at and one beside the tile sizes, radii beyond the image,
the grid-stride loop of both kernels, the single-axis and no-axis launches of the direct route, subnormal, huge, signed
and non-finite pixels, ``pmi_render_blurred`` and the reuse of the library's scratch.  Every comparison is equality of the
float32 bit patterns with a plain float64 reference on the CPU (scipy's ``gaussian_filter``, or two ``correlate1d``
passes); where the reference is NaN the device must be NaN, of any sign and payload.  tests/test_blur_edges_host.py
checks on the CPU that the cases sit on the kernel's constants and that the references agree with one another."""
import json
import sys
import time

import numpy as np
import pytest

from conftest import GOLDEN, golden

sys.path.insert(0, GOLDEN)
import _blur_restate as rs  # noqa: E402

from picasso_amd import _lib, backend, render  # noqa: E402

pytestmark = pytest.mark.gpu
differing = rs.differing_but_nan


def seed_of(case):
    return case.n_y * 7 + case.n_x


def spatial_plan_of(case):
    plan = backend.spatial_plan(case.sigma_x, case.sigma_y)
    assert plan.radius == (case.r_y, case.r_x) and plan.skip == (case.sigma_y == 0, case.sigma_x == 0)
    if case.gain != 1.0:                                           # hand-made: the same weights, times the gain
        plan = plan._replace(weights=rs.edge_spatial_weights(case))
    return plan


# ---- the spatial route ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", rs.EDGE_SPATIAL_CASES, ids=rs.edge_id)
def test_spatial_edge_cases_equal_scipy_in_every_bit(case):
    image = rs.edge_image(case.n_y, case.n_x, seed_of(case), case.kind)
    want = rs.edge_spatial_reference(case, image)
    got = backend.blur_with_plan(image, spatial_plan_of(case))
    print(rs.edge_id(case), "differing pixels:", differing(got, want), "of", want.size)
    assert differing(got, want) == 0
    if case.gain == 1.0 and backend.blur_plan(case.n_y, case.n_x, case.sigma_x, case.sigma_y).route == "spatial":
        assert differing(render._fftconvolve(image, case.sigma_x, case.sigma_y), want) == 0


# ---- the direct route ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", rs.EDGE_DIRECT_CASES, ids=rs.edge_id)
def test_direct_edge_cases_equal_two_correlate1d_passes_in_every_bit(case):
    image = rs.edge_image(case.n_y, case.n_x, seed_of(case), case.kind)
    want = rs.edge_direct_reference(case, image)
    wy, wx, S = rs.edge_direct_parts(case)
    if case.entry == "fft":                                        # the reference's own entry: radius 5 * round(width)
        plan = backend.blur_plan(case.n_y, case.n_x, case.width, case.height)
        assert plan.route == "direct" and plan.radius == (case.r_y, case.r_x)
        got = render._fftconvolve(image, case.width, case.height)
    else:
        if case.entry == "plan" and case.s_gain == 1.0:
            plan = backend.direct_plan(2 * case.r_x + 1, 2 * case.r_y + 1, case.width, case.height)
            assert np.array_equal(plan.weights[0], wy) and np.array_equal(plan.weights[1], wx) and plan.S == S
        else:                                                      # hand-made: one axis, no axis, or an S of its own
            plan = backend.BlurPlan("direct", (2 * case.r_y + 1, 2 * case.r_x + 1), (case.r_y, case.r_x), (wy, wx),
                                    (wy is None, wx is None), S)
            with np.errstate(all="ignore"):
                assert differing(rs.separable(image, wy, wx, False, 1.0 / S), want) == 0
        assert plan.radius == (case.r_y, case.r_x)
        got = backend.blur_with_plan(image, plan)
    print(rs.edge_id(case), "differing pixels:", differing(got, want), "of", want.size)
    assert differing(got, want) == 0


# ---- the grid-stride loop of either kernel ----------------------------------------------------------------------------------
def test_row_pass_takes_a_second_tile_behind_the_grid_limit():
    case = rs.EDGE_GRID_ROW_CASE
    image = rs.edge_image(case.n_y, case.n_x, seed_of(case))
    want = rs.edge_spatial_reference(case, image)
    plan = spatial_plan_of(case)
    backend.blur_with_plan(image[:64], plan)                       # the first call of a process loads the code object
    t0 = time.perf_counter()
    got = backend.blur_with_plan(image, plan)
    seconds = time.perf_counter() - t0
    print(rs.edge_id(case), "differing pixels:", differing(got, want), "of", want.size, "| device call with its copies:", round(seconds, 4), "s")
    assert differing(got, want) == 0
    # three columns are too few for the reference's own entry to take the spatial route
    assert backend.blur_plan(case.n_y, case.n_x, case.sigma_x, case.sigma_y).route == "direct"


def test_column_pass_takes_a_second_tile_behind_the_grid_limit():
    case = rs.EDGE_GRID_COL_CASE
    t_all = time.perf_counter()
    rng = np.random.default_rng(seed_of(case))
    image = rng.poisson(0.7, (case.n_y, case.n_x)).astype(np.float32)
    image[1, 0] = image[-1, 0] = 60000.0
    want = rs.edge_spatial_reference(case, image)
    plan = spatial_plan_of(case)
    backend.blur_with_plan(image[:64], plan)
    try:
        t0 = time.perf_counter()
        got = backend.blur_with_plan(image, plan)
        seconds = time.perf_counter() - t0
        count = differing(got, want)
        print(rs.edge_id(case), "differing pixels:", count, "of", want.size, "| device call with its copies:", round(seconds, 4),
              "s | whole test:", round(time.perf_counter() - t_all, 2), "s")
        assert count == 0
    finally:
        del image, want
        got = None
        _lib.call("pmi_release_scratch")                           # two slots of 128 MiB on the device


# ---- pmi_render_blurred on a direct plan of several chunks in both passes -----------------------------------------------------
def test_render_blurred_equals_the_two_steps_and_the_reference_at_radii_65_and_130():
    G = golden("blur_cases")
    call = json.loads(str(G["render/hist_os1/call"]))
    x, y = G["render/in_x"], G["render/in_y"]
    (y_min, x_min), (y_max, x_max) = call["viewport"]
    n_h, hist = backend.render_arrays(x, y, 1.0, y_min, x_min, y_max, x_max)
    assert n_h == int(G["render/hist_os1/n"]) and n_h > 0
    bw, bh = 26, 13
    plan = backend.blur_plan(hist.shape[0], hist.shape[1], bw, bh)
    assert plan.route == "direct" and plan.radius == (65, 130)
    n, image = backend.render_blurred_arrays(x, y, 1.0, y_min, x_min, y_max, x_max, bw, bh)
    two_steps = backend.blur_with_plan(hist, plan)
    case = rs.EdgeDirect(hist.shape[0], hist.shape[1], "fft", bw, bh, 65, 130)
    want = rs.edge_direct_reference(case, hist)
    print("render_blurred: differing pixels:", differing(image, two_steps), "from the two steps,", differing(two_steps, want), "from the reference")
    assert n == n_h and differing(image, two_steps) == 0 and differing(two_steps, want) == 0


# ---- the scratch slots grow, and are reused while larger than needed ----------------------------------------------------------
def test_scratch_slots_are_reused_while_larger_than_needed():
    _lib.call("pmi_release_scratch")                               # every slot starts empty
    big = rs.EdgeDirect(300, 300, "plan", 38.6, 38.6, 193, 193)
    small = rs.EdgeDirect(40, 40, "fft", 1, 1, 5, 5)
    results = []
    for case in (big, small, big):
        image = rs.edge_image(case.n_y, case.n_x, seed_of(case))
        plan = backend.direct_plan(2 * case.r_x + 1, 2 * case.r_y + 1, case.width, case.height)
        assert plan.radius == (case.r_y, case.r_x)
        got = backend.blur_with_plan(image, plan)
        count = differing(got, rs.edge_direct_reference(case, image))
        print(rs.edge_id(case), "differing pixels:", count)
        assert count == 0
        results.append(got)
    assert backend.blur_plan(40, 40, 1, 1).route == "direct"
    assert differing(results[2], results[0]) == 0 and np.array_equal(results[2].view(np.uint32), results[0].view(np.uint32))
