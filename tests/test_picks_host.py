"""CPU tier of the picked localizations: the restatement (tests/golden/_picks_restate.py) against the goldens minted from
the reference, the goldens against the reference tree when it is present, the ABI, the recorded signatures, and the
Python layer of ``postprocess.picked_locs`` / ``remove_locs_in_picks`` with the four ``backend.picks_*`` calls replaced
by the restatement."""
import inspect
import json
import os

import numpy as np
import pandas as pd
import pytest

from picasso_amd import _lib, backend, lib, postprocess

from _picks_cases import CASES, G, assert_frames, call, columns, expected, mk, remove_size, rs, table

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RETURNING = [n for n in CASES if f"{n}/n_out" in G.files]


def test_every_case_returns_and_the_situations_are_there():
    assert RETURNING == CASES and len(CASES) >= 25
    shapes = {call(n)[0] for n in CASES}
    assert shapes == {"Circle", "Square", "Rectangle", "Polygon"}
    assert any(not call(n)[3] for n in CASES) and any(bool(G[n + "/has_index"]) for n in CASES)


@pytest.mark.parametrize("name", CASES)
def test_restatement_reproduces_the_golden(name):
    shape, picks, size, add_group, info = call(name)
    df, cols = table(name), columns(name)
    kept, offsets, rows = rs.members(cols, info, picks, shape, size)
    want = expected(name)
    assert len(kept) == len(want)
    for k, (w, _) in enumerate(want):
        sub = df.iloc[rows[offsets[k]:offsets[k + 1]]]
        # the reference's order before its sort, then its sort: ties between equal frames come out as recorded
        order = sub["frame"].to_numpy().argsort(kind="quicksort")
        assert np.array_equal(sub.index.to_numpy()[order], w.index.to_numpy()), (name, k)
        if add_group:
            assert (w["group"] == kept[k]).all()
    if f"{name}/removed_index" in G.files:
        # remove_locs_in_picks halves a circle's diameter itself: an integer diameter becomes a float radius
        radius = remove_size(name) / 2 if shape == "Circle" else size
        _, _, rows = rs.members(cols, info, picks, shape, radius)
        assert np.array_equal(np.delete(df.index.to_numpy(), np.unique(rows)), G[name + "/removed_index"])


@pytest.mark.parametrize("name", ["circle_typing", "circle_typing_int_radius"])
def test_the_circle_typings_are_told_apart(name):
    """Rim rows found by search: every typing but a pick's own gives that pick another member set, so a kernel or a
    host that ignores the flags fails these goldens."""
    shape, picks, size, add_group, info = call(name)
    assert mk.forced_flags_change_the_answer((columns(name), None, shape, picks, size, add_group, info))
    members = [frozenset(w.index.tolist()) for w, _ in expected(name)]
    if name == "circle_typing":          # int, Python float, np.float64, (int, float), (float, int)
        assert members[1] == members[2] and len({members[0], members[1], members[3], members[4]}) == 4
    else:                                # an integer radius: int, float and (int, float) picks
        assert len(set(members)) == 3
    masks = [G["lib/is_loc_at_py"], G["lib/is_loc_at_np"]]
    assert (masks[0] != masks[1]).any()


def test_zero_division_is_unreachable_behind_the_strict_box():
    for name in CASES:
        shape, picks, size, _, info = call(name)
        if shape != "Rectangle":
            continue
        cols = columns(name)
        bounds, flags, corners = rs.rectangle_plan(picks, size)
        for b, f, (X, Y) in zip(bounds, flags, corners):
            inside = rs.box_mask(cols["x"], cols["y"], b, int(f))
            assert not rs.rectangle_zero_division(cols["y"][inside], Y), name
    assert rs.rectangle_zero_division(G["polygon_basic/in_y"], G["lib/flat_Y"])


def test_goldens_regenerate():
    """The committed picks_cases.npz is what make_goldens_picks.py mints from the reference tree today."""
    if not os.path.isfile(mk.POSTPROCESS_PY):
        pytest.skip("reference tree not present")
    ref, ref_lib = mk.load_reference()
    cases = mk.cases()
    assert list(cases) == CASES
    out = {}
    for name, case in cases.items():
        mk.mint(ref, name, case, out)
    mk.lib_cases(ref_lib, cases, out)
    for key, value in out.items():
        assert mk.same(value, G[key]), key
    recorded = json.loads(str(G["signatures"]))
    assert recorded == {**{n: str(inspect.signature(ref[n])) for n in mk.PUBLIC_PP},
                        **{"lib." + n: str(inspect.signature(ref_lib[n])) for n in mk.PUBLIC_LIB}}


# ---- names, signatures, ABI -------------------------------------------------------------------------------------
def test_names_and_signatures():
    recorded = json.loads(str(G["signatures"]))
    assert sorted(recorded) == sorted(postprocess.PICK_NAMES + tuple("lib." + n for n in lib.PICK_NAMES))
    for name in postprocess.PICK_NAMES:
        assert str(inspect.signature(getattr(postprocess, name))) == recorded[name], name
    for name in lib.PICK_NAMES:
        assert str(inspect.signature(getattr(lib, name))) == recorded["lib." + name], name


def test_abi_version_and_symbols():
    L = _lib.load()
    assert L.pmi_version() >= 120
    header = open(os.path.join(ROOT, "include", "picasso_hip.h")).read()
    for name in ("pmi_picks_circle_dev", "pmi_picks_cells_dev", "pmi_picks_shape_dev"):
        assert name in _lib.SYMBOLS and hasattr(L, name) and name in header
    assert (backend.PICK_SQUARE, backend.PICK_RECTANGLE, backend.PICK_POLYGON) == (rs.SQUARE, rs.RECTANGLE, rs.POLYGON)


# ---- the Python layer over the restatement ------------------------------------------------------------------------
class FakeTable:
    def __init__(self, x_index, y_index, K, L):
        self.x_index, self.y_index, self.K, self.L, self.n = x_index, y_index, K, L, len(x_index)


def fake_circle(table, x, y, pick_x, pick_y, block_x, block_y, flags, r2):
    order = np.lexsort([table.x_index, table.y_index])
    xi, yi = table.x_index[order].astype(np.int64), table.y_index[order].astype(np.int64)
    outside = np.flatnonzero((yi >= table.K) | (xi >= table.L))
    p = int(outside[0]) if len(outside) else len(order)
    keys = ((yi << 32) | xi)[:p]
    S = np.result_type(x.dtype, y.dtype)
    xs, ys = x.astype(S)[order], y.astype(S)[order]
    out = []
    for px, py, bx, by, f in zip(pick_x, pick_y, block_x, block_y, flags):
        idx = [np.arange(*np.searchsorted(keys, [(k << 32) | ll, ((k << 32) | ll) + 1]))
               for k in range(by - 1, by + 2) if 0 <= k < table.K for ll in range(bx - 1, bx + 2) if 0 <= ll < table.L]
        idx = np.concatenate(idx) if idx else np.zeros(0, np.int64)
        out.append(order[idx[rs.circle_mask(xs[idx], ys[idx], px, py, r2, f)]])
    return rs.csr(out)


def corners_of(offsets, X, Y):
    return [(X[a:b], Y[a:b]) for a, b in zip(offsets[:-1], offsets[1:])]


@pytest.fixture
def restated(monkeypatch):
    monkeypatch.setattr(backend, "BlockTable", FakeTable)
    monkeypatch.setattr(backend, "picks_circle", fake_circle)
    monkeypatch.setattr(backend, "picks_square", lambda x, y, b, f: rs.shapes({"x": x, "y": y}, rs.SQUARE, b, f))
    monkeypatch.setattr(backend, "picks_rectangle",
                        lambda x, y, b, f, X, Y: rs.shapes({"x": x, "y": y}, rs.RECTANGLE, b, f, list(zip(X, Y))))
    monkeypatch.setattr(backend, "picks_polygon",
                        lambda x, y, b, f, o, X, Y: rs.shapes({"x": x, "y": y}, rs.POLYGON, b, f, corners_of(o, X, Y)))


@pytest.mark.parametrize("name", CASES)
def test_python_layer_gives_the_golden_frames(restated, name):
    shape, picks, size, add_group, info = call(name)
    df = table(name)
    before = df.copy()
    seen = []
    got = postprocess.picked_locs(df, info, picks, shape, size, add_group, None, seen.append)
    assert_frames(got, name)
    assert seen == list(range(1, len(picks) + 1))
    assert df.equals(before) and df.index.equals(before.index)
    if shape == "Rectangle" and got:
        assert list(got[0].columns)[len(before.columns):len(before.columns) + 2] == ["x_pick_rot", "y_pick_rot"]
    if f"{name}/removed_index" in G.files:
        out = postprocess.remove_locs_in_picks(df, info, picks=picks, pick_shape=shape, pick_size=remove_size(name))
        assert out is df and np.array_equal(df.index.to_numpy(), G[name + "/removed_index"])


def test_edges_before_the_device(restated):
    df, (shape, picks, size, _, info) = table("circle_basic"), call("circle_basic")
    assert postprocess.picked_locs(df, info, [], "Circle", size) == []
    with pytest.raises(AssertionError, match="Invalid pick shape"):
        postprocess.picked_locs(df, info, picks, "Ellipse", size)
    with pytest.raises(NotImplementedError, match="index_blocks"):
        postprocess.picked_locs(df, info, picks, "Circle", size, index_blocks=(df, size))
    with pytest.raises(NotImplementedError):
        postprocess.remove_locs_in_picks(df, info, picks=picks, pick_shape="Circle", pick_size=1.0, index_blocks=(df,))
    with pytest.raises(AssertionError, match="pick_size must be a number"):
        postprocess.remove_locs_in_picks(df, info, picks=picks, pick_shape="Square", pick_size=None)
    with pytest.raises(ZeroDivisionError):
        lib.check_if_in_rectangle(G["polygon_basic/in_x"], G["polygon_basic/in_y"], G["lib/flat_X"], G["lib/flat_Y"])
    assert lib.get_pick_polygon_corners([(1.0, 1.0), (2.0, 2.0)]) == (None, None)
    args = [float(v) for v in G["lib/rectangle_args"]]
    X, Y = lib.get_pick_rectangle_corners(*args)
    assert np.array_equal(X, G["lib/rectangle_X"]) and np.array_equal(Y, G["lib/rectangle_Y"]) and type(X[0]) is float


def test_install_leaves_the_picks_family_alone():
    """An existing test pins ``picked_locs`` as the reference's own after install(): the new names are not rebound."""
    import types
    from picasso_amd import localize
    mods = {n: types.ModuleType("picasso." + n) for n in
            ("localize", "gaussmle", "gausslq", "zfit", "render", "imageprocess", "postprocess", "aim")}
    for name in postprocess.PICK_NAMES:
        setattr(mods["postprocess"], name, "theirs")
    localize.install(*[mods[n] for n in ("localize", "gaussmle", "gausslq", "zfit", "render", "imageprocess", "postprocess")],
                     picasso_aim=mods["aim"])
    assert all(getattr(mods["postprocess"], n) == "theirs" for n in postprocess.PICK_NAMES)
