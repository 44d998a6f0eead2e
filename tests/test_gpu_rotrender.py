"""GPU tier: csrc/render_rot.hip against the NumPy restatement of the rotated views (tests/golden/_rotrender_restate.py,
which the minting script and the CPU tier pin to the reference in bits), in float32 bit equality (any NaN equals any
NaN) and in n; the rotated coordinates in float64 bit equality.  The cases sit where the tile scheme has seams the
reference's sequential loop has not: the 32x32 tile borders, the 32-record LDS chunk border inside a tile's list, the
launch borders of the per-row kernels; and where the arithmetic has corners: nearly degenerate projected covariances,
rows skipped on det < 1e-10, widths that are NaN, infinite, zero or negative.

The kernel evaluates glibc's exp operation for operation (csrc/libm_glibc.h, pinned by tests/test_libm_glibc.py), the
restatement calls the C library's: there is no 1-ulp allowance here and no chance of a miss to bound.
Images are at most 97 x 65 pixels, tables at most a few thousand rows."""
import ctypes
import functools
import json
import sys

import numpy as np
import pandas as pd
import pytest
from scipy.spatial.transform import Rotation

from conftest import GOLDEN, golden

sys.path.insert(0, GOLDEN)
import _rotrender_restate as rs  # noqa: E402

pytestmark = pytest.mark.gpu
NAN, INF = float("nan"), float("inf")


@pytest.fixture(scope="module")
def be():
    from picasso_amd import backend
    return backend


def matrix(name):
    from picasso_amd import render
    return render.to_rotation(Rotation.from_quat(rs.QUAT) if name == "quat" else rs.EULER[name]).as_matrix()


def assert_same_bits(img, ref):
    assert img.shape == ref.shape and img.dtype == ref.dtype == np.float32
    diff = (img.view(np.uint32) != ref.view(np.uint32)) & ~(np.isnan(img) & np.isnan(ref))
    assert not diff.any(), f"{int(diff.sum())} pixels differ from the restatement, the first at (row, column) {np.argwhere(diff)[:8].tolist()}"


def view_of(n_y, n_x, oversampling=1.0, y_min=0.0, x_min=0.0):
    return (oversampling, y_min, x_min, y_min + n_y / oversampling, x_min + n_x / oversampling)


def check(be, cols, M, view, min_blur=0.0, iso=False, hist=False):
    """The device == the restatement in n and in every bit -> (n, image, in_view)."""
    x, y, z = cols["x"], cols["y"], cols["z"]
    if hist:
        n, img, in_view = be.render_rot_arrays(x, y, z, M, *view)
        rn, ref = rs.render_hist(x, y, z, M, *view)
        assert img.sum() == n
    else:
        n, img, in_view = be.render_rot_arrays(x, y, z, M, *view, lpx=cols["lpx"], lpy=cols["lpy"], lpz=cols.get("lpz"),
                                               min_blur_width=min_blur, iso=iso)
        rn, ref = rs.render_gaussian(x, y, z, cols["lpx"], cols["lpy"], cols.get("lpz"), M, *view, min_blur, iso=iso)
    assert n == rn == int(in_view.sum())
    assert np.array_equal(in_view, rs.rotate(x, y, z, M, *view)[3])
    assert_same_bits(img, ref)
    return n, img, in_view


# ---- the reference's own images ---------------------------------------------------------------------------------------
def test_device_matches_the_reference_goldens(be):
    g = golden("rotrender_cases")
    for name in (str(n) for n in g["render/case_names"]):
        p = f"render/{name}/"
        call = json.loads(str(g[p + "call"]))
        cols = {k[len(p) + 3:]: g[k] for k in g.files if k.startswith(p + "in_") and k != p + "in_view"}
        (y_min, x_min), (y_max, x_max) = call["viewport"]
        view = (call["oversampling"], y_min, x_min, y_max, x_max)
        for fn in ("_render_gaussian", "_render_gaussian_iso"):
            n, img, _ = be.render_rot_arrays(cols["x"], cols["y"], cols["z"], g[p + "matrix"], *view, lpx=cols["lpx"],
                                             lpy=cols["lpy"], lpz=cols.get("lpz"), min_blur_width=call["min_blur_width"],
                                             iso=fn.endswith("iso"))
            assert n == int(g[p + fn + "/n"]), (name, fn)
            assert_same_bits(img, g[p + fn + "/image"])
        n, img, in_view = be.render_rot_arrays(cols["x"], cols["y"], cols["z"], g[p + "matrix"], *view)
        assert n == int(g[p + "_render_hist/n"]) and np.array_equal(in_view, g[p + "in_view"])
        assert_same_bits(img, g[p + "_render_hist/image"])


# ---- tile seams -------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def seam_table(n_y, n_x):
    rng = np.random.default_rng(100 * n_y + n_x)
    cols = rs.table(rng, 60, n_y, n_x, 1.0, spread=1.1, z_scale=0.3)
    # rows next to every tile border of the image, wide enough to straddle it (z = 0: the rotation keeps them close)
    edge_x = [31.4, 32.0, 32.6, 63.5, 64.0, 64.4, 31.9, 0.6, n_x - 0.6]
    edge_y = [15.5, 31.7, 32.3, 30.9, 32.0, 16.2, 31.2, 0.7, n_y - 0.7]
    m = len(edge_x)
    cols["x"], cols["y"] = np.concatenate([cols["x"], np.float32(edge_x)]), np.concatenate([cols["y"], np.float32(edge_y)])
    cols["z"] = np.concatenate([cols["z"], np.zeros(m, np.float32)])
    for c in ("lpx", "lpy", "lpz"):
        cols[c] = np.concatenate([cols[c], rng.uniform(1.0, 2.5, m).astype(np.float32)])
    return cols


@pytest.mark.parametrize("mode", ["gaussian", "gaussian_iso", "hist"])
@pytest.mark.parametrize("n_y,n_x", [(a, b) for a in (31, 32, 33) for b in (63, 64, 65)])
def test_tile_seams(be, n_y, n_x, mode):
    n, img, _ = check(be, seam_table(n_y, n_x), matrix("generic"), view_of(n_y, n_x), iso=mode == "gaussian_iso", hist=mode == "hist")
    assert img.shape == (n_y, n_x) and n > 20


# ---- chunk seams ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [31, 32, 33, 65])
def test_chunk_seams(be, m):
    rng = np.random.default_rng(m)
    one = np.ones(m, np.float32)
    cols = {"x": 20.3 * one, "y": 17.6 * one, "z": 0.0 * one, "lpx": rng.uniform(0.4, 3.0, m).astype(np.float32),
            "lpy": rng.uniform(0.4, 3.0, m).astype(np.float32), "lpz": rng.uniform(0.4, 3.0, m).astype(np.float32)}
    M, view = matrix("generic"), view_of(40, 40)
    # a case where the order of the additions does not matter tests nothing
    fwd = rs.render_gaussian(cols["x"], cols["y"], cols["z"], cols["lpx"], cols["lpy"], cols["lpz"], M, *view, 0.0)[1]
    rev = rs.render_gaussian(cols["x"], cols["y"], cols["z"], cols["lpx"][::-1], cols["lpy"][::-1], cols["lpz"][::-1], M, *view, 0.0)[1]
    assert (fwd.view(np.uint32) != rev.view(np.uint32)).any()
    n, img, _ = check(be, cols, M, view)
    assert n == m


# ---- launch seams -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["gaussian", "hist"])
@pytest.mark.parametrize("n_rows", [255, 256, 257, 513])
def test_launch_seams(be, n_rows, mode):
    cols = rs.table(np.random.default_rng(n_rows), n_rows, 40, 48, 2.0)
    # the last rows of the table are in view: a launch that drops the tail shows
    cols["x"][-3:], cols["y"][-3:], cols["z"][-3:] = 12.0, 10.0, 0.0
    n, _, in_view = check(be, cols, matrix("generic"), view_of(40, 48, 2.0), hist=mode == "hist")
    assert in_view[-3:].all()


# ---- rows that are counted and draw nothing -----------------------------------------------------------------------------------
def test_degenerate_covariance_rows_are_counted_and_draw_nothing(be):
    cols = rs.table(np.random.default_rng(5), 40, 33, 33, 1.0, spread=0.6, z_scale=0.2)
    tiny = np.arange(40) % 4 == 0
    for c in ("lpx", "lpy", "lpz"):
        cols[c][tiny] = 1e-4                              # det of the projection ~ 1e-16 < 1e-10
    M, view = matrix("generic"), view_of(33, 33)
    n, img, in_view = check(be, cols, M, view)
    assert (in_view & tiny).sum() >= 5 and n == in_view.sum()
    kept = {k: v[~tiny] for k, v in cols.items()}
    _, without, _ = check(be, kept, M, view)
    assert_same_bits(img, without)


def test_quarter_turn_is_nearly_degenerate(be):
    """(pi / 2, 0, 0): the matrix holds cos(pi / 2) = 6e-17 entries, the projection mixes a width with almost nothing."""
    cols = rs.table(np.random.default_rng(6), 80, 40, 40, 2.0)
    cols["lpy"][::3] = 1e-5                               # becomes the depth: the projected covariance stays regular
    cols["lpz"][1::3] = 2e-6                              # becomes the height: det < 1e-10
    n, img, _ = check(be, cols, matrix("quarter_x"), view_of(40, 40, 2.0))
    assert n > 10 and img.max() > 0


@pytest.mark.parametrize("iso", [False, True])
@pytest.mark.parametrize("min_blur", [0.0, 0.5, -1.0])
def test_widths_nan_inf_zero_negative(be, min_blur, iso):
    odd = [NAN, INF, 0.0, -0.7, -INF, 1e-30, 3e38]
    rows = [(a, 0.8, 1.1) for a in odd] + [(0.8, a, 1.1) for a in odd] + [(0.8, 1.1, a) for a in odd] + [(NAN, NAN, NAN), (0.0, 0.0, 0.0)]
    m = len(rows)
    rng = np.random.default_rng(7)
    cols = {"x": rng.uniform(8, 25, m).astype(np.float32), "y": rng.uniform(8, 25, m).astype(np.float32),
            "z": rng.uniform(-3, 3, m).astype(np.float32)}
    for k, c in enumerate(("lpx", "lpy", "lpz")):
        cols[c] = np.float32([r[k] for r in rows])
    # ordinary rows before, between and after
    normal = rs.table(np.random.default_rng(8), 12, 33, 33, 1.0, spread=0.6)
    cols = {c: np.concatenate([normal[c][:6], cols[c], normal[c][6:]]) for c in cols}
    for name in ("generic", "identity"):
        n, img, _ = check(be, cols, matrix(name), view_of(33, 33), min_blur, iso)
        assert n >= m


# ---- column forms, lpz, rotations -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mixed", [False, True])
@pytest.mark.parametrize("with_lpz", [False, True])
@pytest.mark.parametrize("rotation", ["identity", "quarter_x", "generic", "quat"])
def test_rotations_columns_and_lpz(be, rotation, with_lpz, mixed):
    cols = rs.table(np.random.default_rng(11), 300, 65, 97, 2.5, with_lpz)
    if mixed:
        cols["x"] = cols["x"].astype(np.float64) + 1e-9            # not float32 values any more
    M, view = matrix(rotation), view_of(65, 97, 2.5)
    n, _, in_view = check(be, cols, M, view, 0.01)
    check(be, cols, M, view, hist=True)
    unrotated = (cols["x"] > 0) & (cols["y"] > 0) & (cols["x"] < view[4]) & (cols["y"] < view[3])
    if rotation in ("generic", "quat", "quarter_x"):
        assert (in_view & ~unrotated).any() and (~in_view & unrotated).any()      # rows moved into the view and out of it
    else:
        assert np.array_equal(in_view, unrotated)


@pytest.mark.parametrize("ang", [(0.7, -0.4, 1.1), Rotation.from_quat(rs.QUAT)], ids=["euler", "quat"])
def test_the_render_functions_take_ang(be, ang):
    from picasso_amd import render
    cols = rs.table(np.random.default_rng(12), 200, 48, 40, 2.0, with_lpz=False)
    cols["x"] += np.float32(3.5)
    cols["y"] += np.float32(1.25)
    locs = pd.DataFrame({"frame": np.arange(200, dtype=np.uint32), **cols})
    view = view_of(48, 40, 2.0, 1.25, 3.5)
    M = render.to_rotation(ang).as_matrix()
    args = (locs, 2.0, view[1], view[2], view[3], view[4])
    for fn, iso in ((render._render_gaussian, False), (render._render_gaussian_iso, True)):
        n, img = fn(*args, 0.03, ang=ang)
        rn, ref = rs.render_gaussian(cols["x"], cols["y"], cols["z"], cols["lpx"], cols["lpy"], None, M, *view, 0.03, iso=iso)
        assert n == rn
        assert_same_bits(img, ref)
    n, img = render._render_hist(*args, ang=ang)
    rn, ref = rs.render_hist(cols["x"], cols["y"], cols["z"], M, *view)
    assert n == rn == img.sum()
    assert_same_bits(img, ref)
    # locs_rotation: the reference's argument order (x before y), compacted
    x, y, in_view, z = render.locs_rotation(locs, 2.0, view[2], view[4], view[1], view[3], ang)
    rx, ry, rz, rv = rs.rotate(cols["x"], cols["y"], cols["z"], M, *view)
    assert np.array_equal(in_view, rv) and in_view.dtype == bool
    assert x.tobytes() == rx[rv].tobytes() and y.tobytes() == ry[rv].tobytes() and z.tobytes() == rz[rv].tobytes()


# ---- empty table, empty view ------------------------------------------------------------------------------------------------------
def test_empty_table_and_empty_view(be):
    empty = {c: np.zeros(0, np.float32) for c in ("x", "y", "z", "lpx", "lpy", "lpz")}
    for hist in (False, True):
        n, img, in_view = check(be, empty, matrix("generic"), view_of(33, 40), hist=hist)
        assert n == 0 and not img.any() and img.shape == (33, 40) and in_view.shape == (0,)
    away = rs.table(np.random.default_rng(13), 50, 33, 40, 1.0)
    away["x"] += np.float32(500.0)
    for hist in (False, True):
        n, img, _ = check(be, away, matrix("generic"), view_of(33, 40), hist=hist)
        assert n == 0 and not img.any()
    with pytest.raises(ValueError, match="empty viewport"):
        be.render_rot_arrays(away["x"], away["y"], away["z"], matrix("generic"), 1.0, 0.0, 0.0, 0.0, 10.0)


def test_one_row_and_two_rows(be):
    """A one-row table takes the other order of the rotation's sum (the header of render_rot.hip)."""
    for n_rows in (1, 2):
        cols = rs.table(np.random.default_rng(14), n_rows, 33, 33, 1.0, spread=0.4, z_scale=0.3)
        n, _, _ = check(be, cols, matrix("generic"), view_of(33, 33))
        assert n == n_rows


# ---- the rotated coordinates --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mixed", [False, True])
@pytest.mark.parametrize("n_rows", [1, 2, 257, 3000])
def test_rotate_locs_in_float64_bits(be, n_rows, mixed):
    cols = rs.table(np.random.default_rng(n_rows), n_rows, 65, 97, 2.5)
    if mixed:
        cols["z"] = cols["z"].astype(np.float64) * 1.0000001
    cols["x"][:1] = NAN                                     # a NaN coordinate is out of view
    M, view = matrix("generic"), view_of(65, 97, 2.5, 1.5, 3.25)
    got = be.rotate_locs_arrays(cols["x"], cols["y"], cols["z"], M, *view)
    want = rs.rotate(cols["x"], cols["y"], cols["z"], M, *view)
    assert np.array_equal(got[3], want[3]) and not got[3][0]
    for a, b in zip(got[:3], want[:3]):
        assert a.dtype == np.float64
        differ = (a.view(np.uint64) != b.view(np.uint64)) & ~(np.isnan(a) & np.isnan(b))
        assert not differ.any(), int(differ.sum())


def test_host_forms_of_the_c_abi(be):
    """pmi_rotate_locs, pmi_render_hist_rot and pmi_render_gaussian_rot on host pointers == the device forms the wrappers call."""
    from picasso_amd import _lib
    cols = rs.table(np.random.default_rng(15), 500, 40, 65, 2.0, with_lpz=False)
    M = np.ascontiguousarray(matrix("generic"))
    M32 = M.astype(np.float32)
    view = view_of(40, 65, 2.0)
    x, y, z = (np.ascontiguousarray(cols[c]) for c in "xyz")
    n_rows = len(x)
    xr, yr, zr, inv = np.empty(n_rows), np.empty(n_rows), np.empty(n_rows), np.empty(n_rows, np.uint8)
    image, n = np.empty((40, 65), np.float32), ctypes.c_int64(0)
    with _lib.lock():
        _lib.call("pmi_rotate_locs", _lib.ptr(x), _lib.ptr(y), _lib.ptr(z), 0, n_rows, _lib.ptr(M), *view, _lib.ptr(xr), _lib.ptr(yr),
                  _lib.ptr(zr), _lib.ptr(inv))
    want = rs.rotate(x, y, z, M, *view)
    assert xr.tobytes() == want[0].tobytes() and yr.tobytes() == want[1].tobytes() and zr.tobytes() == want[2].tobytes()
    assert np.array_equal(inv.astype(bool), want[3])
    with _lib.lock():
        _lib.call("pmi_render_gaussian_rot", _lib.ptr(x), _lib.ptr(y), _lib.ptr(z), 0, _lib.ptr(cols["lpx"]), _lib.ptr(cols["lpy"]),
                  None, n_rows, _lib.ptr(M), _lib.ptr(M32), *view, 0.0, 0, _lib.ptr(image), 40, 65, ctypes.byref(n))
    rn, ref = rs.render_gaussian(x, y, z, cols["lpx"], cols["lpy"], None, M, *view, 0.0)
    assert n.value == rn
    assert_same_bits(image, ref)
    x64, y64, z64 = (a.astype(np.float64) for a in (x, y, z))
    with _lib.lock():
        _lib.call("pmi_render_hist_rot", _lib.ptr(x64), _lib.ptr(y64), _lib.ptr(z64), 1, n_rows, _lib.ptr(M), *view, _lib.ptr(image),
                  40, 65, ctypes.byref(n))
    rn, ref = rs.render_hist(x64, y64, z64, M, *view)
    assert n.value == rn == image.sum()
    assert_same_bits(image, ref)
    with pytest.raises(_lib.HipBackendError, match="viewport needs"):
        _lib.call("pmi_render_hist_rot", _lib.ptr(x), _lib.ptr(y), _lib.ptr(z), 0, n_rows, _lib.ptr(M), *view, _lib.ptr(image), 41, 65,
                  ctypes.byref(n))


# ---- scratch reuse ----------------------------------------------------------------------------------------------------------------
def test_scratch_reuse_large_small_large(be):
    large = rs.table(np.random.default_rng(16), 2000, 65, 97, 2.5)
    small = rs.table(np.random.default_rng(17), 3, 65, 97, 2.5, spread=0.3, z_scale=0.1)
    M, view = matrix("generic"), view_of(65, 97, 2.5)
    first = check(be, large, M, view)[1]
    check(be, small, M, view)                  # most tiles now without rows: their start / end must have been cleared
    second = check(be, large, M, view)[1]
    assert np.array_equal(first.view(np.uint32), second.view(np.uint32))
