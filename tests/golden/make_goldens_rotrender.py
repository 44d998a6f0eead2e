#!/usr/bin/env python3
"""Mint tests/golden/rotrender_cases.npz: the reference's own rotated views on small tables, and its rotation helpers.

TEST INFRASTRUCTURE, build container only (needs the reference tree, scipy and pandas; no numba).  ``render.py`` is
executed from where it lies behind the stand-ins of _refshim.py: ``rotation_matrix``, ``to_rotation``,
``closest_rotvec``, ``locs_rotation`` and the bodies of ``_render_hist`` / ``_render_gaussian`` / ``_render_gaussian_iso``
are plain NumPy / scipy there as in production.  The two jitted functions under them, ``_draw_gaussian_rot_loc`` and
``_fill_gaussian_rot``, are compiled in memory from the same file with numba's typing of their arithmetic
(_nbemu: ``_Retype`` / ``binop``, the C library's exp) and put in the place of the plain ones.  Nothing of the
reference is stored but inputs and results.

Every input is finite: the emulation cannot do numba's ``int(NaN)``, so rows with non-finite widths are covered by the
restatement (_rotrender_restate.py) alone.  (One more difference is out of reach of finite random tables: NumPy 2
compares ``float32 < 1e-10`` in float32, numba in float64; the two differ only for det == float32(1e-10).)

The script ASSERTS that the restatement equals the reference IN EVERY BIT on every case: the rotated coordinates
(float64), n and the images (float32).  That assertion is the measurement behind the two orders of operations the kernels
build in: ``r_i = (M[i][0] v0 + M[i][1] v1) + M[i][2] v2`` for ``Rotation.apply`` (scipy 1.15.3, NumPy 2.2.6, einsum) on
the column-major array pandas 2.3.3 makes of the three columns, ``(M[i][0] v0 + M[i][2] v2) + M[i][1] v1`` for a table of
one row (``one_row`` below), and the fused chain in k order for the float32 3x3 products (NumPy 2.2.6's wheel: scipy-openblas 0.3.29, Haswell kernels,
sgemm on a CPU with FMA).  On a host whose NumPy or BLAS evaluates either in another order (another einsum, an sgemm
kernel without FMA or with another blocking of k) the assertion fails: the goldens then are not to be re-minted there.

Contents.
  versions, signatures   JSON;
  helpers/*     Euler triples -> the matrix and quaternion of ``rotation_matrix``; ``to_rotation`` of a tuple / a Rotation /
                None; ``closest_rotvec`` cases (identity with and without turns, multi-turn references);
  rotate/*      tables (float32, and mixed column types) -> the reference's ``locs_rotation`` (x, y, in_view, z);
  render/*      tables and calls -> the reference's (n, image).

Run:  python tests/golden/make_goldens_rotrender.py
"""
import ast
import inspect
import json
import os
import sys
import warnings

import numpy as np
import pandas as pd

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _nbemu  # noqa: E402
import _refshim  # noqa: E402
import _rotrender_restate as rs  # noqa: E402

REF = _refshim.REF
JITTED = ("_draw_gaussian_rot_loc", "_fill_gaussian_rot")
HELPER_EULER = [(0.0, 0.0, 0.0), (np.pi / 2, 0.0, 0.0), (0.7, -0.4, 1.1), (3.0, 2.5, -2.0), (1e-12, 0.0, 0.0), (0.0, np.pi, 0.0)]
ROTVEC_CASES = [            # (rotation vector the Rotation is built from, reference)
    ((0.0, 0.0, 0.0), (0.0, 0.0, 0.0)), ((0.0, 0.0, 0.0), (0.0, 0.0, 1e-12)), ((0.0, 0.0, 0.0), (0.0, 0.0, 6.5)),
    ((0.0, 0.0, 0.0), (3.0, 4.0, 12.0)), ((0.0, 0.0, 0.0), (0.1, 0.2, 0.3)),
    ((0.3, -0.2, 0.5), (0.3, -0.2, 0.5)), ((0.3, -0.2, 0.5), (3.4, -2.3, 5.6)), ((0.3, -0.2, 0.5), (-6.0, 4.0, -10.0)),
    ((0.0, 3.1, 0.0), (0.0, -3.2, 0.0)), ((1.0, 1.0, 1.0), (20.0, 20.0, 20.0)), ((2e-10, 0.0, 0.0), (7.0, 0.0, 0.0)),
]


class _Numba:
    @staticmethod
    def njit(*a, **k):
        return lambda fn: fn

    jit = njit


def retyped_fill(render):
    """The two jitted functions of the rotated Gaussian with numba's typing; -> the retyped ``_fill_gaussian_rot``."""
    path = os.path.join(REF, "picasso", "render.py")
    tree = ast.parse(open(path).read())
    keep = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in JITTED]
    assert [n.name for n in keep] == list(JITTED)
    mod = ast.Module(body=[ast.ImportFrom("__future__", [ast.alias("annotations")], 0)] + keep, type_ignores=[])
    tr = _nbemu._Retype()
    ns = {"np": _nbemu._NumpyProxy(), "numba": _Numba, "lib": None, "__nb_binop__": _nbemu.binop,
          "_DRAW_MAX_SIGMA": render._DRAW_MAX_SIGMA}
    exec(compile(ast.fix_missing_locations(tr.visit(mod)), path, "exec"), ns)
    assert sorted(tr.rewritten) == sorted(JITTED)
    return ns["_fill_gaussian_rot"]


def bits_equal(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def helper_cases(render, out):
    from scipy.spatial.transform import Rotation
    out["helpers/euler"] = np.array(HELPER_EULER, np.float64)
    rots = [render.rotation_matrix(*e) for e in HELPER_EULER]
    out["helpers/euler_matrix"] = np.array([r.as_matrix() for r in rots])
    out["helpers/euler_quat"] = np.array([r.as_quat() for r in rots])
    assert all(bits_equal(render.to_rotation(e).as_matrix(), r.as_matrix()) for e, r in zip(HELPER_EULER, rots))
    q = Rotation.from_quat(rs.QUAT)
    assert render.to_rotation(q) is q and render.to_rotation(None) is None
    out["helpers/quat"], out["helpers/quat_matrix"] = np.array(rs.QUAT, np.float64), q.as_matrix()
    out["helpers/rotvec_in"] = np.array([c[0] for c in ROTVEC_CASES], np.float64)
    out["helpers/rotvec_reference"] = np.array([c[1] for c in ROTVEC_CASES], np.float64)
    got = np.array([render.closest_rotvec(Rotation.from_rotvec(v), np.array(r)) for v, r in ROTVEC_CASES])
    out["helpers/rotvec_out"] = got
    assert np.abs(np.linalg.norm(got, axis=1)).max() > 2 * np.pi          # a multi-turn branch is taken
    print("helpers:", len(HELPER_EULER), "Euler triples,", len(ROTVEC_CASES), "closest_rotvec cases")


# name -> (rotation, rows, n_y, n_x, oversampling, (y_min, x_min), lpz column, mixed column types, min_blur_width)
RENDER_CASES = {
    "identity": ("identity", 70, 33, 40, 2.0, (0.0, 0.0), True, False, 0.0),
    "quarter_x": ("quarter_x", 70, 33, 40, 2.0, (0.0, 0.0), True, False, 0.0),
    "generic": ("generic", 90, 33, 65, 2.5, (1.5, 3.25), True, False, 0.0),
    "generic_no_lpz": ("generic", 90, 33, 65, 2.5, (1.5, 3.25), False, False, 0.02),
    "generic_mixed": ("generic", 90, 40, 33, 2.0, (0.3, 0.7), True, True, 0.0),
    "quat": ("quat", 90, 40, 33, 2.0, (0.3, 0.7), False, False, 0.5),
    # one row takes the other order of the rotation's sum (a (1, 3) array is row-major too), two rows do not
    "one_row": ("generic", 1, 33, 33, 2.0, (0.0, 0.0), True, False, 0.0),
    "two_rows": ("generic", 2, 33, 33, 2.0, (0.0, 0.0), True, False, 0.0),
}
METHODS = ("_render_gaussian", "_render_gaussian_iso", "_render_hist")


def rotation_of(name):
    from scipy.spatial.transform import Rotation
    return Rotation.from_quat(rs.QUAT) if name == "quat" else rs.EULER[name]


def case_table(name):
    rot, n, n_y, n_x, osamp, (y_min, x_min), with_lpz, mixed, _ = RENDER_CASES[name]
    cols = rs.table(np.random.default_rng(sum(map(ord, name))), n, n_y, n_x, osamp, with_lpz, *((0.4, 0.3) if n <= 2 else ()))
    cols["x"], cols["y"] = (cols["x"] + np.float32(x_min)).astype(np.float32), (cols["y"] + np.float32(y_min)).astype(np.float32)
    if mixed:
        cols["z"] = cols["z"].astype(np.float64) * 1.0000001
    return cols, (y_min, x_min, y_min + n_y / osamp, x_min + n_x / osamp)


def render_cases(render, out):
    out["render/case_names"] = np.array(list(RENDER_CASES))
    for name, (rot, n, n_y, n_x, osamp, _, with_lpz, mixed, mbw) in RENDER_CASES.items():
        cols, (y_min, x_min, y_max, x_max) = case_table(name)
        locs = pd.DataFrame({"frame": np.arange(n, dtype=np.uint32), **cols})
        ang = rotation_of(rot)
        M = render.to_rotation(ang).as_matrix()
        p = f"render/{name}/"
        out[p + "call"] = np.array(json.dumps({"rotation": rot, "oversampling": osamp, "viewport": [[y_min, x_min], [y_max, x_max]],
                                              "min_blur_width": mbw, "mixed": mixed}))
        out[p + "matrix"] = M
        for c, v in cols.items():
            out[p + "in_" + c] = v
        # locs_rotation
        x, y, in_view, z = render.locs_rotation(locs, osamp, x_min, x_max, y_min, y_max, ang)
        rx, ry, rz, rv = rs.rotate(cols["x"], cols["y"], cols["z"], M, osamp, y_min, x_min, y_max, x_max)
        assert bits_equal(in_view, rv) and bits_equal(x, rx[rv]) and bits_equal(y, ry[rv]) and bits_equal(z, rz[rv]), name
        assert 0 < in_view.sum() < n or (n <= 2 and in_view.all())
        out[p + "rot_x"], out[p + "rot_y"], out[p + "rot_z"], out[p + "in_view"] = x, y, z, in_view
        unrotated = (cols["x"] > x_min) & (cols["y"] > y_min) & (cols["x"] < x_max) & (cols["y"] < y_max)
        moved = f"{int((in_view & ~unrotated).sum())} rows moved in, {int((~in_view & unrotated).sum())} out"
        for fn in METHODS:
            args = (locs, osamp, y_min, x_min, y_max, x_max) + (() if fn == "_render_hist" else (mbw,))
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                n_ref, image = getattr(render, fn)(*args, ang=ang)
            lpz = cols.get("lpz")
            if fn == "_render_hist":
                n_rs, mine = rs.render_hist(cols["x"], cols["y"], cols["z"], M, osamp, y_min, x_min, y_max, x_max)
                assert image.sum() == n_ref
            else:
                n_rs, mine = rs.render_gaussian(cols["x"], cols["y"], cols["z"], cols["lpx"], cols["lpy"], lpz, M, osamp,
                                                y_min, x_min, y_max, x_max, mbw, iso=fn.endswith("iso"))
                assert image.max() > 0
            assert n_rs == n_ref == int(in_view.sum()), (name, fn)
            assert image.dtype == np.float32 and image.shape == (n_y, n_x)
            same = image.view(np.uint32) == mine.view(np.uint32)
            assert same.all(), f"{name} {fn}: the restatement differs from the reference in {int((~same).sum())} of {same.size} pixels"
            out[p + fn + "/n"], out[p + fn + "/image"] = np.int64(n_ref), image
        print(f"render {name:15s} {n_y} x {n_x}, n = {int(in_view.sum())} of {n} ({moved}): restatement == reference in every bit")


def signatures(render, out):
    names = ("rotation_matrix", "to_rotation", "closest_rotvec", "locs_rotation") + METHODS + tuple(m[1:] for m in METHODS)
    out["signatures"] = np.array(json.dumps({n: str(inspect.signature(getattr(render, n))) for n in names}))


def main():
    import scipy
    render = _refshim.load_reference()["render"]
    render._fill_gaussian_rot = retyped_fill(render)
    out = {"versions": np.array(json.dumps({"numpy": np.__version__, "scipy": scipy.__version__, "pandas": pd.__version__}))}
    signatures(render, out)
    helper_cases(render, out)
    render_cases(render, out)
    path = os.path.join(HERE, "rotrender_cases.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 1 << 20


if __name__ == "__main__":
    main()
