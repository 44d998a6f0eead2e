"""GPU tier: csrc/render.hip against oracle.render, bit for bit, at the seams the tile scheme has and
the reference's sequential loop has not: the 32x32 tile borders, the 32-localization LDS chunk border
inside a tile's list, the launch borders of the per-localization kernels, and profiles that are not
finite (inf * 0 = NaN must never reach a pixel outside the footprint).

The comparison is equality of the float32 bit patterns (any NaN equals any NaN) and of n.  The one
exception render.hip's header allows, a 1-ulp float64 exp difference that survives the rounding to
float32, has a chance of about 2^-29 per profile value; every case here builds fewer than 1e5 of
them.  The tables are shared with the CPU tier (render_edge_tables.py), which pins the oracle on them.
"""
import numpy as np
import pytest

import render_edge_tables as T

pytestmark = pytest.mark.gpu
METHODS = ["gaussian", "gaussian_iso"]


@pytest.fixture(scope="module")
def be():
    from picasso_amd import backend
    return backend


@pytest.fixture(scope="module")
def orc():
    from oracle import oracle
    return oracle


def assert_same_bits(img, ref):
    assert img.shape == ref.shape and img.dtype == ref.dtype == np.float32
    diff = (img.view(np.uint32) != ref.view(np.uint32)) & ~(np.isnan(img) & np.isnan(ref))
    assert not diff.any(), f"{int(diff.sum())} pixels differ from the oracle, the first at (row, column) {np.argwhere(diff)[:8].tolist()}"


def check(be, orc, case, method):
    """render_arrays == oracle.render in n and in every bit; method None is the histogram."""
    (y_min, x_min), (y_max, x_max) = case.viewport
    if method is None:
        n, img = be.render_arrays(case.x, case.y, case.oversampling, y_min, x_min, y_max, x_max)
        on, ref = orc.render(case.x, case.y, case.oversampling, case.viewport)
        assert img.sum() == n
    else:
        n, img = be.render_arrays(case.x, case.y, case.oversampling, y_min, x_min, y_max, x_max, case.lpx, case.lpy,
                                  case.min_blur, iso=(method == "gaussian_iso"))
        on, ref = orc.render(case.x, case.y, case.oversampling, case.viewport, case.lpx, case.lpy, method, case.min_blur)
    assert n == on
    assert_same_bits(img, ref)
    return img


# ---------------------------------------------------------------------------
# profiles that are not finite
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("name", sorted(T.NONFINITE))
def test_nonfinite_profiles_stay_inside_the_footprint(be, orc, name, method):
    case = T.NONFINITE[name]()
    img = check(be, orc, case, method)
    if name == "inf_rows" and method == "gaussian":
        assert sorted(map(tuple, np.argwhere(~np.isfinite(img)).tolist())) == [(12, 50), (20, 20)]


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("min_blur", [0.0, 0.5, -1.0])
def test_widths_nan_inf_negative_subnormal(be, orc, min_blur, method):
    check(be, orc, T.odd_widths(min_blur), method)


# ---------------------------------------------------------------------------
# tile seams
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("method", METHODS + [None])
@pytest.mark.parametrize("ny,nx", T.SEAM_SIZES)
def test_tile_seams(be, orc, ny, nx, method):
    case = T.tile_seam(ny, nx)
    img = check(be, orc, case, method)
    assert img.shape == (ny, nx)


# ---------------------------------------------------------------------------
# chunk seams
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("interleaved", [False, True])
@pytest.mark.parametrize("m", T.CHUNK_SIZES)
def test_chunk_seams(be, orc, m, interleaved, method):
    case = T.chunk_seam(m, interleaved)
    # a case where the order of the additions does not matter tests nothing
    fwd = orc.render(case.x, case.y, case.oversampling, case.viewport, case.lpx, case.lpy, method, case.min_blur)[1]
    rev = orc.render(case.x[::-1], case.y[::-1], case.oversampling, case.viewport, case.lpx[::-1], case.lpy[::-1], method,
                     case.min_blur)[1]
    assert T.order_matters(fwd, rev)
    check(be, orc, case, method)


# ---------------------------------------------------------------------------
# launch seams
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("method", METHODS + [None])
@pytest.mark.parametrize("n_rows", T.LAUNCH_SIZES)
def test_launch_seams(be, orc, n_rows, method):
    case = T.launch_seam(n_rows)
    check(be, orc, case, method)


# ---------------------------------------------------------------------------
# histogram
# ---------------------------------------------------------------------------
def test_hist_many_rows_in_one_pixel(be, orc):
    case = T.hist_one_pixel()
    img = check(be, orc, case, None)
    assert img[10, 10] == 70_000 and img[9:12, 9:12].sum() == 70_000 and img.sum() == 70_000


def test_hist_rows_next_to_the_borders(be, orc):
    case = T.hist_borders()
    img = check(be, orc, case, None)
    assert img[0, 0] >= 1 and img[-1, -1] >= 1 and img[0, -1] >= 1 and img[-1, 0] >= 1


# ---------------------------------------------------------------------------
# scratch reuse
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("method", METHODS)
def test_scratch_reuse_large_small_large(be, orc, method):
    large, small, sparse = T.scratch_cases()
    first = check(be, orc, large, method)
    check(be, orc, small, method)
    second = check(be, orc, large, method)
    assert np.array_equal(first.view(np.uint32), second.view(np.uint32))
    # most tiles of the same image now without localizations: their start / end must have been cleared
    check(be, orc, sparse, method)
