"""CPU tier of the blur's edge cases (tests/golden/_blur_restate.py ``EDGE_*``): the NumPy restatement against scipy in
bits on every case (``gaussian_filter`` on the spatial route, two float64 ``correlate1d`` passes on the direct one), the
cases against the constants of csrc/blur.hip they are there for, the content kinds against what they claim, and the host
build of csrc/blur_core.h on the spatial cases of more than one row-pass chunk.  The device runs the same cases in
tests/test_gpu_blur_edges.py."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

sys.path.insert(0, GOLDEN)
import _blur_restate as rs  # noqa: E402

from picasso_amd import backend  # noqa: E402

SPATIAL = rs.EDGE_SPATIAL_CASES + [rs.EDGE_GRID_ROW_CASE]          # the 2 ** 25 rows of the other one are left to the device
TINY = float(np.finfo(np.float32).tiny)


def seed_of(case):
    return case.n_y * 7 + case.n_x


def direct_plan_of(case):
    """The plan an entry point makes for a direct case, or None where the plan is hand-made."""
    if case.entry == "fft":
        return backend.blur_plan(case.n_y, case.n_x, case.width, case.height)
    if case.entry == "plan":
        return backend.direct_plan(2 * case.r_x + 1, 2 * case.r_y + 1, case.width, case.height)
    return None


# ---- the references agree ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", SPATIAL, ids=rs.edge_id)
def test_restatement_equals_scipy_on_the_spatial_cases(case):
    image = rs.edge_image(case.n_y, case.n_x, seed_of(case), case.kind)
    want = rs.edge_spatial_reference(case, image)
    wy, wx = rs.edge_spatial_weights(case)
    with np.errstate(all="ignore"):
        got = rs.separable(image, wy, wx, True)
        assert rs.differing_but_nan(got, want) == 0
        if case.gain == 1.0:
            assert rs.differing_but_nan(rs.spatial(image, case.sigma_y, case.sigma_x), want) == 0


@pytest.mark.parametrize("case", rs.EDGE_DIRECT_CASES, ids=rs.edge_id)
def test_restatement_equals_two_correlate1d_passes_on_the_direct_cases(case):
    image = rs.edge_image(case.n_y, case.n_x, seed_of(case), case.kind)
    want = rs.edge_direct_reference(case, image)
    wy, wx, S = rs.edge_direct_parts(case)
    with np.errstate(all="ignore"):
        assert rs.differing_but_nan(rs.separable(image, wy, wx, False, 1.0 / S), want) == 0
        if case.entry == "fft":
            kw, kh = rs.kernel_of(case.width), rs.kernel_of(case.height)
            assert rs.differing_but_nan(rs.direct(image, kw, kh, case.width, case.height), want) == 0


def test_the_nan_rule_compares_position_only():
    want = np.array([np.nan, 1.0, -0.0, np.inf], np.float32)
    flipped = want.copy()
    flipped.view(np.uint32)[0] ^= 0x80000001                      # another sign and payload: still a NaN
    assert np.isnan(flipped[0]) and rs.differing_but_nan(flipped, want) == 0
    for k, v in ((0, 1.0), (1, np.nan), (2, 0.0), (3, -np.inf)):
        got = want.copy()
        got[k] = v
        assert rs.differing_but_nan(got, want) == 1


# ---- the cases hold what they are for -----------------------------------------------------------------------------------
def kernel_constants():
    text = open(os.path.join(ROOT, "picasso_amd", "csrc", "blur.hip")).read()
    found = {m.group(1): m.group(2) for m in re.finditer(r"^constexpr\s+(?:int|unsigned)\s+(\w+)\s*=\s*([^;]+);", text, re.M)}
    out = {}
    for name in ("ROW_T", "ROW_C", "COL_X", "COL_Y", "COL_PER", "COL_C", "MAX_GRID"):
        m = re.fullmatch(r"(\d+)u?(?:\s*<<\s*(\d+))?", found[name].strip())
        out[name] = int(m.group(1)) << int(m.group(2) or 0)
    return out


def test_the_cases_sit_on_the_kernels_edges():
    K = kernel_constants()
    ROW_T, ROW_C, COL_X, COL_Y, COL_PER, COL_C, MAX_GRID = (K[n] for n in ("ROW_T", "ROW_C", "COL_X", "COL_Y", "COL_PER", "COL_C", "MAX_GRID"))
    for cases in (rs.EDGE_SPATIAL_CASES, rs.EDGE_DIRECT_CASES):
        rows = [c for c in cases if c.r_x > 0]                     # cases whose row pass walks at least one chunk
        cols = [c for c in cases if c.r_y > 0]
        r_x, r_y = {c.r_x for c in rows}, {c.r_y for c in cols}
        assert {ROW_C - 1, ROW_C, ROW_C + 1, 2 * ROW_C, 2 * ROW_C + 1} <= r_x and max(r_x) > 3 * ROW_C
        assert {COL_C - 1, COL_C, COL_C + 1, 2 * COL_C, 2 * COL_C + 1} <= r_y and max(r_y) > 3 * COL_C
        assert {ROW_T - 1, ROW_T, ROW_T + 1, 2 * ROW_T, 2 * ROW_T + 1, 1} <= {c.n_x for c in rows if c.r_x >= ROW_C - 1}
        assert {COL_X - 1, COL_X, COL_X + 1, 2 * COL_X + 1, 1} <= {c.n_x for c in cols if c.r_y >= COL_C - 1}
        assert {COL_Y - 1, COL_Y, COL_Y + 1, 2 * COL_Y, 2 * COL_Y + 1, 1} <= {c.n_y for c in cols if c.r_y >= COL_C - 1}
        # a lane's strip of COL_PER rows ends half-way in one case, one row into the next lane's strip in another
        assert {COL_PER // 2, COL_PER + 1} <= {c.n_y % COL_Y for c in cols if c.r_y >= COL_C - 1}
        # a radius beyond the side, and beyond twice the side, on each axis
        assert any(c.n_x > 1 and c.n_x < c.r_x < 2 * c.n_x for c in rows) and any(c.n_x > 1 and c.r_x >= 2 * c.n_x for c in rows)
        assert any(c.n_y > 1 and c.n_y < c.r_y < 2 * c.n_y for c in cols) and any(c.n_y > 1 and c.r_y >= 2 * c.n_y for c in cols)
        # both passes past one chunk at once
        assert sum(c.r_x > ROW_C and c.r_y > COL_C for c in cases) >= 2
        # every content kind, on a case of two chunks or more in one pass
        for kind in ("subnormal", "huge", "signed", "nonfinite"):
            assert any(c.kind == kind and (c.r_x > ROW_C or c.r_y > COL_C) for c in cases), kind
        assert all(c.n_y <= 300 and c.n_x <= 513 for c in cases)
    # a skipped second axis and a short one beside a row pass of two chunks or more, on both routes
    assert sum(c.sigma_y == 0 and c.r_x >= ROW_C for c in rs.EDGE_SPATIAL_CASES) >= 2
    assert sum(0 < c.r_y < COL_C and c.r_x >= ROW_C for c in rs.EDGE_SPATIAL_CASES) >= 2
    assert sum(c.entry == "wx" for c in rs.EDGE_DIRECT_CASES) >= 2 and sum(c.entry == "wy" for c in rs.EDGE_DIRECT_CASES) >= 2
    assert sum(c.entry != "wx" and 0 < c.r_y < COL_C and c.r_x >= ROW_C for c in rs.EDGE_DIRECT_CASES) >= 2
    assert sum(c.entry == "none" for c in rs.EDGE_DIRECT_CASES) == 1
    # the grid-stride cases: a few workgroups take a second tile, the others stop after their first
    g = rs.EDGE_GRID_ROW_CASE
    assert MAX_GRID < -(-g.n_x // ROW_T) * g.n_y <= MAX_GRID + 8 and g.r_x > 0
    g = rs.EDGE_GRID_COL_CASE
    assert MAX_GRID < -(-g.n_x // COL_X) * -(-g.n_y // COL_Y) <= MAX_GRID + 8 and g.r_y > 0 and g.sigma_x == 0


@pytest.mark.parametrize("case", SPATIAL + [rs.EDGE_GRID_COL_CASE], ids=rs.edge_id)
def test_spatial_cases_plan_the_radii_they_name(case):
    plan = backend.spatial_plan(case.sigma_x, case.sigma_y)
    assert plan.radius == (case.r_y, case.r_x) and plan.skip == (case.sigma_y == 0, case.sigma_x == 0)
    for w, mine in zip(plan.weights, rs.edge_spatial_weights(case)):
        assert (w is None and mine is None) or np.array_equal(w * case.gain, mine)


@pytest.mark.parametrize("case", rs.EDGE_DIRECT_CASES, ids=rs.edge_id)
def test_direct_cases_plan_the_radii_they_name(case):
    wy, wx, S = rs.edge_direct_parts(case)
    assert tuple(0 if w is None else len(w) // 2 for w in (wy, wx)) == (case.r_y, case.r_x)
    plan = direct_plan_of(case)
    if plan is None:
        assert case.entry in ("wy", "wx", "none") and S != 1.0
        return
    assert plan.route == "direct" and plan.radius == (case.r_y, case.r_x) and plan.skip == (False, False)
    assert np.array_equal(plan.weights[0], wy) and np.array_equal(plan.weights[1], wx) and plan.S * case.s_gain == S
    if case.entry == "fft":
        assert (case.r_y, case.r_x) == (5 * int(np.round(case.height)), 5 * int(np.round(case.width)))


# ---- the content kinds ---------------------------------------------------------------------------------------------------
def references_of(kind):
    for case in rs.EDGE_SPATIAL_CASES:
        if case.kind == kind:
            image = rs.edge_image(case.n_y, case.n_x, seed_of(case), kind)
            yield case, image, rs.edge_spatial_reference(case, image)
    for case in rs.EDGE_DIRECT_CASES:
        if case.kind == kind:
            image = rs.edge_image(case.n_y, case.n_x, seed_of(case), kind)
            yield case, image, rs.edge_direct_reference(case, image)


def test_subnormal_images_blur_to_subnormals_alone():
    seen = 0
    for case, image, want in references_of("subnormal"):
        assert ((image > 0) & (image < TINY)).sum() > image.size // 4          # the two pixels of 60000 alone stay normal
        assert ((want > 0) & (want < TINY)).all(), case          # a kernel that flushes them differs in every pixel
        seen += 1
    assert seen == 2


def test_huge_images_overflow_where_the_weights_are_hand_made():
    seen = []
    for case, image, want in references_of("huge"):
        assert np.isfinite(image).all() and (image == np.float32(3e38)).sum() == 4 and image.max() == np.finfo(np.float32).max
        hand_made = (case.gain if isinstance(case, rs.EdgeSpatial) else case.s_gain) != 1.0
        # normalised weights average: no sum can pass the largest pixel, so only a hand-made plan rounds to inf
        assert bool(np.isinf(want).any()) == hand_made, case
        assert not np.isnan(want).any() and (np.isfinite(want) & (want > 1e30)).any()
        seen.append(hand_made)
    assert sorted(seen) == [False, False, True, True]


def test_signed_images_keep_a_negative_zero_through_the_axis_of_radius_zero():
    seen = 0
    for case, image, want in references_of("signed"):
        w_y = rs.edge_spatial_weights(case)[0] if isinstance(case, rs.EdgeSpatial) else rs.edge_direct_parts(case)[0]
        assert case.r_y == 0 and w_y.tolist() == [1.0]             # the axis is not skipped: one weight of 1
        assert (image < 0).any() and (image > 0).any() and np.signbit(image[image == 0]).all()
        minus_zero = (want == 0) & np.signbit(want)
        # the last row is -0.0 alone: it stays so where the whole window lies inside the image, and nowhere else
        inside = np.arange(case.n_x)
        inside = (inside >= case.r_x) & (inside < case.n_x - case.r_x)
        assert inside.any() and np.array_equal(minus_zero[-1], inside) and (want[-1] == 0).all() and not minus_zero[:-1].any()
        assert (want < 0).any()
        seen += 1
    assert seen == 2


def test_nonfinite_images_give_nan_and_both_infinities():
    seen = 0
    for case, image, want in references_of("nonfinite"):
        assert np.isnan(image).sum() == 1 and (image == np.inf).sum() == 1 and (image == -np.inf).sum() == 1
        (ya,), (xa,) = np.nonzero(image == np.inf)
        (yb,), (xb,) = np.nonzero(image == -np.inf)
        assert abs(ya - yb) <= case.r_y and abs(xa - xb) <= case.r_x
        assert np.isnan(want).sum() > 1 and (want == np.inf).any() and (want == -np.inf).any() and np.isfinite(want).any()
        seen += 1
    assert seen == 2


# ---- the header, built for the host: the plain loop over j on radii the device cuts in chunks ------------------------------
@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    d = tmp_path_factory.mktemp("blur_edges_host")
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


@pytest.mark.parametrize("case", [c for c in rs.EDGE_SPATIAL_CASES if max(c.r_y, c.r_x) > 64], ids=rs.edge_id)
def test_host_build_equals_scipy_on_the_spatial_cases_above_radius_64(case, driver):
    image = rs.edge_image(case.n_y, case.n_x, seed_of(case), case.kind)
    wy, wx = rs.edge_spatial_weights(case)
    assert rs.differing_but_nan(driver(image, wy, wx, 1), rs.edge_spatial_reference(case, image)) == 0


@pytest.mark.parametrize("case", [c for c in rs.EDGE_DIRECT_CASES if c.entry in ("wy", "wx", "none") or c.kind != "poisson"], ids=rs.edge_id)
def test_host_build_equals_correlate1d_on_the_hand_made_and_content_direct_cases(case, driver):
    image = rs.edge_image(case.n_y, case.n_x, seed_of(case), case.kind)
    wy, wx, S = rs.edge_direct_parts(case)
    assert rs.differing_but_nan(driver(image, wy, wx, 0, 1.0 / S), rs.edge_direct_reference(case, image)) == 0
