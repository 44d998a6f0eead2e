"""GPU tier of the picked localizations: every golden case through ``postprocess.picked_locs`` /
``remove_locs_in_picks`` on the device (frames equal to the reference's, index and dtypes included), the
``backend.picks_*`` CSR pairs against the restatement, the ``lib`` helpers against the recorded results, and one
generated case per shape (2 x 10^4 rows, 300 picks) against the restatement."""
import json

import numpy as np
import pytest

from picasso_amd import backend, lib, postprocess

from _picks_cases import CASES, G, assert_frames, call, columns, generated, mk, remove_size, rs, table

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", CASES)
def test_golden_case_on_the_device(name):
    shape, picks, size, add_group, info = call(name)
    df = table(name)
    before = df.copy()
    seen = []
    got = postprocess.picked_locs(df, info, picks, shape, size, add_group, None, seen.append)
    assert_frames(got, name)
    assert seen == list(range(1, len(picks) + 1)) and df.equals(before) and df.index.equals(before.index)
    out = postprocess.remove_locs_in_picks(df, info, picks=picks, pick_shape=shape, pick_size=remove_size(name))
    assert out is df and np.array_equal(df.index.to_numpy(), G[name + "/removed_index"])


def device_members(cols, info, picks, shape, size):
    """The (offsets, rows) of the backend call picked_locs makes, rows as positions in the caller's table."""
    x, y = cols["x"], cols["y"]
    if shape == "Circle":
        sane = rs.sane_rows(cols, info)
        xs, ys = x[sane], y[sane]
        K, L = rs.grid_shape(info, size)
        t = backend.BlockTable(np.uint32(xs / size), np.uint32(ys / size), K, L)
        both32 = xs.dtype == np.float32 and ys.dtype == np.float32
        flags = [rs.circle_flags(px, py, size) if both32 else 0 for px, py in picks]
        off, rows = backend.picks_circle(t, xs, ys, [float(p[0]) for p in picks], [float(p[1]) for p in picks],
                                         [rs.block_of(p[0], size) for p in picks], [rs.block_of(p[1], size) for p in picks],
                                         flags, rs.radius_squared(size))
        return off, sane[rows]
    if shape == "Square":
        b, f, _ = rs.square_plan(picks, size)
        return backend.picks_square(x, y, b, f)
    if shape == "Rectangle":
        b, f, c = rs.rectangle_plan(picks, size)
        return backend.picks_rectangle(x, y, b, f, [X for X, _ in c], [Y for _, Y in c])
    _, b, f, c = rs.polygon_plan(picks)
    offsets = np.r_[0, np.cumsum([len(X) for X, _ in c])].astype(np.int32)
    return backend.picks_polygon(x, y, b, f, offsets, np.array([v for X, _ in c for v in X], np.float64),
                                 np.array([v for _, Y in c for v in Y], np.float64))


@pytest.mark.parametrize("name", CASES)
def test_backend_csr_equals_the_restatement(name):
    shape, picks, size, _, info = call(name)
    cols = columns(name)
    _, offsets, rows = rs.members(cols, info, picks, shape, size)
    got_offsets, got_rows = device_members(cols, info, picks, shape, size)
    assert got_offsets.dtype == np.int64 and np.array_equal(got_offsets, offsets)
    assert np.array_equal(got_rows, rows)


@pytest.mark.parametrize("shape", ["Circle", "Square", "Rectangle", "Polygon"])
def test_generated_case_against_the_restatement(shape):
    cols, info, picks, size = generated(shape)
    kept, offsets, rows = rs.members(cols, info, picks, shape, size)
    assert len(rows) > 1000 and (np.diff(offsets) == 0).any()          # many members, and empty picks between them
    got_offsets, got_rows = device_members(cols, info, picks, shape, size)
    assert np.array_equal(got_offsets, offsets) and np.array_equal(got_rows, rows)
    df = mk.frame(cols, None)
    frames = postprocess.picked_locs(df, info, picks, shape, size)
    assert len(frames) == len(kept)
    for k, (i, fr) in enumerate(zip(kept, frames)):
        sub = df.iloc[rows[offsets[k]:offsets[k + 1]]]
        assert np.array_equal(fr.index.to_numpy(), sub.index.to_numpy()[sub["frame"].to_numpy().argsort(kind="quicksort")])
        assert (fr["group"] == i).all()


def test_lib_helpers_on_the_device():
    cols = columns("circle_typing")          # rim rows on which pandas' float32 and float64 comparisons of r ** 2 disagree
    df = mk.frame(cols, None)
    assert (G["lib/is_loc_at_py"] != G["lib/is_loc_at_np"]).any()
    for k, (x, y, r) in {k: mk.untag(v) for k, v in json.loads(str(G["lib/is_loc_at_calls"])).items()}.items():
        mask = lib.is_loc_at(x, y, df, r)
        assert mask.dtype == bool and np.array_equal(mask, G[f"lib/is_loc_at_{k}"]), k
        assert lib.locs_at(x, y, df, r).equals(df[G[f"lib/is_loc_at_{k}"]])
    cols = columns("polygon_basic")
    df = mk.frame(cols, None)
    X, Y = G["lib/polygon_X"], G["lib/polygon_Y"]
    assert np.array_equal(lib.check_if_in_polygon(cols["x"], cols["y"], X, Y), G["lib/in_polygon"])
    assert lib.locs_in_polygon(df, list(X), list(Y)).equals(df[G["lib/in_polygon"]])
    X, Y = G["lib/rectangle_X"], G["lib/rectangle_Y"]
    assert np.array_equal(lib.check_if_in_rectangle(cols["x"], cols["y"], X, Y), G["lib/in_rectangle"])
    assert lib.locs_in_rectangle(df, list(X), list(Y)).equals(df[G["lib/in_rectangle"]])
