"""CPU tier of the rotated views (picasso_amd/render.py, csrc/render_rot.hip): the rotation helpers and the NumPy
restatement against the reference's own results (tests/golden/rotrender_cases.npz, minted by
tests/golden/make_goldens_rotrender.py), in bits, and the routing of the Python layer over fakes of the two backend calls.
Needs no GPU."""
import json
import sys
import types
import warnings

import numpy as np
import pandas as pd
import pytest
from scipy.spatial.transform import Rotation

from conftest import GOLDEN, golden

sys.path.insert(0, GOLDEN)
import _rotrender_restate as rs  # noqa: E402

from picasso_amd import backend, localize, render  # noqa: E402


@pytest.fixture(scope="module")
def g():
    return golden("rotrender_cases")


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def case(g, name):
    p = f"render/{name}/"
    call = json.loads(str(g[p + "call"]))
    cols = {k[len(p) + 3:]: g[k] for k in g.files if k.startswith(p + "in_") and k != p + "in_view"}
    (y_min, x_min), (y_max, x_max) = call["viewport"]
    return p, call, cols, (call["oversampling"], y_min, x_min, y_max, x_max)


def test_the_library_exports_the_rotated_calls():
    from picasso_amd import _lib
    L = _lib.load()
    assert L.pmi_version() >= 125
    for name in ("pmi_rotate_locs", "pmi_render_hist_rot", "pmi_render_gaussian_rot"):
        assert name in _lib.SYMBOLS and name + "_dev" in _lib.SYMBOLS and hasattr(L, name) and hasattr(L, name + "_dev")


# ---- the helpers ------------------------------------------------------------------------------------------------------
def test_rotation_matrix_and_to_rotation_match_the_reference_in_bits(g):
    for e, m, q in zip(g["helpers/euler"], g["helpers/euler_matrix"], g["helpers/euler_quat"]):
        r = render.rotation_matrix(*e)
        assert isinstance(r, Rotation) and same_bits(r.as_matrix(), m) and same_bits(r.as_quat(), q)
        assert same_bits(render.to_rotation(tuple(e)).as_matrix(), m)
    q = Rotation.from_quat(g["helpers/quat"])
    assert render.to_rotation(q) is q and same_bits(q.as_matrix(), g["helpers/quat_matrix"])
    assert render.to_rotation(None) is None


def test_closest_rotvec_matches_the_reference_in_bits(g):
    out = g["helpers/rotvec_out"]
    for v, ref, want in zip(g["helpers/rotvec_in"], g["helpers/rotvec_reference"], out):
        assert same_bits(render.closest_rotvec(Rotation.from_rotvec(v), ref), want)
    norms = np.linalg.norm(out, axis=1)
    # the identity branch (with and without turns) and a multi-turn branch are among the cases
    assert not out[0].any() and not out[1].any() and norms[2] == pytest.approx(2 * np.pi) and norms.max() > 4 * np.pi
    assert same_bits(render.closest_rotvec(Rotation.identity(), [0.0, 0.0, 0.0]), np.zeros(3))


def test_signatures_are_the_references(g):
    import inspect
    for name, sig in json.loads(str(g["signatures"])).items():
        assert list(inspect.signature(getattr(render, name)).parameters) == _names(sig), name


def _names(sig):
    """Parameter names of a signature string whose annotations may hold commas."""
    depth, token, out = 0, "", []
    for ch in sig[1:sig.rindex(")")] + ",":
        if ch in "[(":
            depth += 1
        if ch in "])":
            depth -= 1
        if ch == "," and depth == 0:
            out.append(token.split(":")[0].split("=")[0].strip())
            token = ""
        else:
            token += ch
    return [n for n in out if n]


# ---- the restatement ----------------------------------------------------------------------------------------------------
def test_restatement_matches_the_reference_in_bits(g):
    names = [str(n) for n in g["render/case_names"]]
    assert {"identity", "quarter_x", "generic", "generic_no_lpz", "generic_mixed", "quat", "one_row", "two_rows"} <= set(names)
    for name in names:
        p, call, cols, view = case(g, name)
        M = g[p + "matrix"]
        x, y, z, in_view = rs.rotate(cols["x"], cols["y"], cols["z"], M, *view)
        assert same_bits(in_view, g[p + "in_view"])
        assert same_bits(x[in_view], g[p + "rot_x"]) and same_bits(y[in_view], g[p + "rot_y"]) and same_bits(z[in_view], g[p + "rot_z"])
        assert (cols["z"].dtype == np.float64) == call["mixed"]
        for fn in ("_render_gaussian", "_render_gaussian_iso"):
            n, image = rs.render_gaussian(cols["x"], cols["y"], cols["z"], cols["lpx"], cols["lpy"], cols.get("lpz"), M, *view,
                                          call["min_blur_width"], iso=fn.endswith("iso"))
            assert n == int(g[p + fn + "/n"]) and same_bits(image, g[p + fn + "/image"]), (name, fn)
        n, image = rs.render_hist(cols["x"], cols["y"], cols["z"], M, *view)
        assert n == int(g[p + "_render_hist/n"]) == image.sum() and same_bits(image, g[p + "_render_hist/image"])


def test_restated_fmaf_rounds_once():
    # (1 + 2^-23)(1 - 2^-24) + (2^-47 + 2^-70) = 1 + 2^-24 + 2^-70: float64 rounds the sum to the float32 midpoint
    # 1 + 2^-24, which then rounds to even (1.0); the fused operation rounds once, up
    a, b, c = np.float32(1 + 2.0 ** -23), np.float32(1 - 2.0 ** -24), np.float32(2.0 ** -47 + 2.0 ** -70)
    assert float(a) == 1 + 2.0 ** -23 and float(b) == 1 - 2.0 ** -24 and float(c) == 2.0 ** -47 + 2.0 ** -70
    assert np.float32(float(a) * float(b) + float(c)) == np.float32(1.0)
    assert rs.fmaf(a, b, c) == np.float32(1 + 2.0 ** -23)
    assert rs.fmaf(-a, b, -c) == -np.float32(1 + 2.0 ** -23)
    assert rs.fmaf(np.float32(3.0), np.float32(0.5), np.float32(0.25)) == np.float32(1.75)
    assert np.isnan(rs.fmaf(np.float32(np.inf), np.float32(0.0), np.float32(1.0)))


# ---- routing over fakes of the backend calls -----------------------------------------------------------------------------
@pytest.fixture
def calls(monkeypatch):
    seen = []

    def render_rot_arrays(x, y, z, matrix, oversampling, y_min, x_min, y_max, x_max, lpx=None, lpy=None, lpz=None,
                          min_blur_width=0.0, iso=False, with_in_view=True):
        seen.append(dict(x=x, y=y, z=z, matrix=matrix, oversampling=oversampling, view=(y_min, x_min, y_max, x_max), lpx=lpx,
                         lpy=lpy, lpz=lpz, min_blur_width=min_blur_width, iso=iso, coords=backend.rotation_coords(x, y, z)))
        return 5, np.zeros((2, 3), np.float32), None

    def rotate_locs_arrays(x, y, z, matrix, oversampling, y_min, x_min, y_max, x_max):
        seen.append(dict(rotate=True, matrix=matrix, view=(y_min, x_min, y_max, x_max), coords=backend.rotation_coords(x, y, z)))
        n = len(x)
        return np.arange(n) + 0.5, np.arange(n) + 1.5, np.arange(n) + 2.5, np.arange(n) % 2 == 0

    monkeypatch.setattr(backend, "render_rot_arrays", render_rot_arrays)
    monkeypatch.setattr(backend, "rotate_locs_arrays", rotate_locs_arrays)
    return seen


def table(n=4, lpz=False, z_dtype=np.float32):
    cols = {"frame": np.arange(n, dtype=np.uint32), "x": np.linspace(1, 2, n).astype(np.float32),
            "y": np.linspace(2, 3, n).astype(np.float32), "z": np.linspace(-1, 1, n).astype(z_dtype),
            "lpx": np.full(n, 0.1, np.float32), "lpy": np.full(n, 0.2, np.float32)}
    if lpz:
        cols["lpz"] = np.full(n, 0.3, np.float32)
    return pd.DataFrame(cols)


def test_render_gaussian_with_ang_reaches_the_rotated_call(calls):
    ang = (0.7, -0.4, 1.1)
    locs = table(lpz=True)
    n, image = render._render_gaussian(locs, 2.5, 1.0, 2.0, 30.0, 40.0, 0.05, ang=ang)
    assert n == 5 and image.shape == (2, 3) and len(calls) == 1
    c = calls[0]
    assert same_bits(c["matrix"], render.to_rotation(ang).as_matrix()) and c["view"] == (1.0, 2.0, 30.0, 40.0)
    assert c["oversampling"] == 2.5 and c["min_blur_width"] == 0.05 and c["iso"] is False
    assert np.array_equal(c["lpz"], locs["lpz"]) and np.array_equal(c["lpx"], locs["lpx"]) and np.array_equal(c["z"], locs["z"])
    assert c["coords"][3] == backend.LINK_F32
    # no lpz column: NULL, the kernel takes twice the mean of lpx and lpy
    render._render_gaussian_iso(table(), 2.5, 1.0, 2.0, 30.0, 40.0, 0.05, ang=Rotation.from_quat(rs.QUAT))
    assert calls[1]["lpz"] is None and calls[1]["iso"] is True
    assert same_bits(calls[1]["matrix"], Rotation.from_quat(rs.QUAT).as_matrix())
    # the histogram: no widths at all
    render._render_hist(table(), 2.5, 1.0, 2.0, 30.0, 40.0, ang=ang)
    assert calls[2]["lpx"] is None and calls[2]["lpy"] is None
    # the older names pass ang on
    with pytest.warns(DeprecationWarning, match="'render_gaussian' function is deprecated"):
        render.render_gaussian(table(), 1.0, 0, 0, 32, 32, 0.0, ang=ang)
    with pytest.warns(DeprecationWarning):
        render.render_gaussian_iso(table(), 1.0, 0, 0, 32, 32, 0.0, ang=ang)
    with pytest.warns(DeprecationWarning):
        render.render_hist(table(), 1.0, 0, 0, 32, 32, ang=ang)
    assert len(calls) == 6 and calls[4]["iso"] is True and calls[5]["lpx"] is None


def test_mixed_column_types_select_the_float64_form(calls):
    render._render_gaussian(table(z_dtype=np.float64), 1.0, 0, 0, 32, 32, 0.0, ang=(0.1, 0, 0))
    x, y, z, code = calls[0]["coords"]
    assert code == backend.LINK_F64 and x.dtype == y.dtype == z.dtype == np.float64
    assert np.array_equal(x, table()["x"].to_numpy().astype(np.float64))
    x, y, z, code = backend.rotation_coords(*(table()[c].to_numpy() for c in "xyz"))
    assert code == backend.LINK_F32 and x.dtype == y.dtype == z.dtype == np.float32
    with pytest.raises(ValueError, match="one entry per row"):
        backend.rotation_coords(np.zeros(3, np.float32), np.zeros(3, np.float32), np.zeros(2, np.float32))
    with pytest.raises(ValueError, match=r"\(3, 3\)"):
        backend._rotation_matrices(np.zeros(9))
    m64, m32 = backend._rotation_matrices(Rotation.from_quat(rs.QUAT).as_matrix())
    assert m32.dtype == np.float32 and same_bits(m32, m64.astype(np.float32)) and m32.flags.c_contiguous


def test_locs_rotation_compacts_what_the_device_returns(calls):
    locs = table(5)
    x, y, in_view, z = render.locs_rotation(locs, 2.0, 3.0, 40.0, 1.0, 30.0, (0.1, 0.2, 0.3))      # x_min, x_max, y_min, y_max
    assert calls[0]["view"] == (1.0, 3.0, 30.0, 40.0)                                               # y_min, x_min, y_max, x_max
    assert in_view.tolist() == [True, False, True, False, True]
    assert x.tolist() == [0.5, 2.5, 4.5] and y.tolist() == [1.5, 3.5, 5.5] and z.tolist() == [2.5, 4.5, 6.5]


def test_the_pinned_refusals_stay(calls):
    locs = table()
    info = [{"Height": 32, "Width": 32, "Pixelsize": 130.0}]
    for method in (None, "gaussian", "gaussian_iso", "smooth", "convolve"):
        with pytest.raises(NotImplementedError):
            render.render(locs, info, disp_px_size=26.0, blur_method=method, ang=(0.1, 0, 0))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for fn, args in ((render._render_smooth, ()), (render.render_smooth, ()), (render._render_convolve, (0.1,)),
                         (render.render_convolve, (0.1,))):
            with pytest.raises(NotImplementedError, match="rotated"):
                fn(locs, 1.0, 0, 0, 32, 32, *args, ang=(0.1, 0, 0))
    assert calls == []


def test_install_still_hands_rotated_calls_to_the_reference(calls):
    theirs = []
    pl, pm, pq, pz, pi, pp = (types.SimpleNamespace() for _ in range(6))
    pr = types.SimpleNamespace(_render_gaussian=lambda *a, **k: theirs.append("gaussian") or (0, None),
                               _render_gaussian_iso=lambda *a, **k: theirs.append("iso") or (0, None),
                               _render_hist=lambda *a, **k: theirs.append("hist") or (0, None))
    localize.install(pl, pm, pq, pz, pr, pi, pp)
    locs = table()
    pr._render_gaussian(locs, 1, 0, 0, 8, 8, 0.0, ang=(0.1, 0, 0))
    pr._render_gaussian_iso(locs, 1, 0, 0, 8, 8, 0.0, (0.1, 0, 0))
    pr._render_hist(locs, 1, 0, 0, 8, 8, ang=Rotation.from_quat(rs.QUAT))
    assert theirs == ["gaussian", "iso", "hist"] and calls == []
    assert not hasattr(pr, "locs_rotation")
