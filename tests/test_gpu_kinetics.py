"""GPU tier: the dark times and the group properties on the device (picasso_amd/postprocess.py, csrc/kinetics.hip)
against the reference's recorded arrays (tests/golden/kinetics_cases.npz) and the test-side restatement
(tests/golden/_kinetics_restate.py).  Everything is compared in bits, with dtype, column order and index."""
import sys

import numpy as np
import pandas as pd
import pytest

from conftest import GOLDEN, golden

sys.path.insert(0, GOLDEN)
import _kinetics_restate as rs  # noqa: E402

from picasso_amd import postprocess  # noqa: E402
from test_kinetics_host import DARK_CASES, PROPS_CASES, dark_case, props_case, props_want, same  # noqa: E402

pytestmark = pytest.mark.gpu
BOUNDARY_SIZES = (1, 2, 7, 8, 9, 127, 128, 129, 136, 257, 8192, 8193, 16385)


@pytest.fixture(scope="module")
def g():
    return golden("kinetics_cases")


def assert_props(got: pd.DataFrame, want: dict, label):
    """``want``: column -> array, in the reference's order."""
    assert list(got.columns) == list(want), label
    assert [str(got[c].dtype) for c in got.columns] == [str(v.dtype) for v in want.values()], label
    assert isinstance(got.index, pd.RangeIndex) and got.index.start == 0 and got.index.step == 1, label
    assert len(got) == len(want["group"]), label
    for c, v in want.items():
        a = got[c].to_numpy()
        if not same(a, v):
            bad = np.flatnonzero(a.view(np.uint32) != v.view(np.uint32))
            print(f"{label}: {c} differs on {len(bad)} of {len(v)} groups, first {bad[:5]}: {a[bad[:5]]} != {v[bad[:5]]}")
        assert same(a, v), (label, c)


@pytest.mark.parametrize("name", DARK_CASES)
def test_dark_times_equal_the_reference(g, name):
    p, cols, group = dark_case(g, name)
    locs = pd.DataFrame(cols)
    before = locs.copy()
    want = g[p + "dark"]
    got = postprocess.dark_times(locs, group)
    assert same(got, want), (name, np.flatnonzero(got != want)[:10])
    assert locs.equals(before)
    if group is None and "group" not in cols:
        labels = np.zeros(len(locs))
    else:
        labels = cols["group"] if group is None else group
    assert same(postprocess._dark_times(cols["frame"], labels, rs.last_frames(cols["frame"], cols["len"])), want)

    table = postprocess.compute_dark_times(locs, group)
    assert list(locs.columns) == list(before.columns) + ["dark"] and len(locs) == len(before)      # written in place
    assert same(locs["dark"].to_numpy(), np.int32(want))
    assert list(table.columns) == [str(c) for c in g[p + "cdt_columns"]]
    assert same(table.index.to_numpy(), g[p + "cdt_index"])
    for c in table.columns:
        assert same(table[c].to_numpy(), g[p + "cdt_" + c]), (name, c)


@pytest.mark.parametrize("name", PROPS_CASES)
def test_group_properties_equal_the_reference(g, name):
    p, cols = props_case(g, name)
    locs = pd.DataFrame(cols)
    before = locs.copy()
    seen = []
    got = postprocess.groupprops(locs, callback=seen.append)
    assert_props(got, props_want(g, p), name)
    assert seen == list(range(len(got) + 1)) and locs.equals(before)


def test_linked_blinking_sites_equal_the_restatement():
    """link() of about 4e5 localizations of 400 blinking sites -> about 2e4 binding events, then both functions."""
    rng = np.random.default_rng(7)
    n_sites, n_events, n_frames = 400, 50, 40000
    start = rng.integers(1, n_frames - 60, n_sites * n_events)
    length = rng.integers(1, 40, len(start))
    site = np.repeat(np.arange(n_sites), n_events)
    frame = np.concatenate([np.arange(s, s + k) for s, k in zip(start, length)])
    which = np.repeat(site, length)
    centres = np.stack([(np.arange(n_sites) % 20) * 6.0 + 4, (np.arange(n_sites) // 20) * 6.0 + 4], axis=1)
    n = len(frame)
    order = np.argsort(frame, kind="stable")
    cols = {"frame": frame.astype(np.uint32), "x": (centres[which, 0] + rng.normal(0, 0.01, n)).astype(np.float32),
            "y": (centres[which, 1] + rng.normal(0, 0.01, n)).astype(np.float32),
            "photons": rng.uniform(500, 9000, n).astype(np.float32), "sx": rng.uniform(0.8, 1.5, n).astype(np.float32),
            "sy": rng.uniform(0.8, 1.5, n).astype(np.float32), "bg": rng.uniform(5, 40, n).astype(np.float32),
            "lpx": rng.uniform(0.005, 0.02, n).astype(np.float32), "lpy": rng.uniform(0.005, 0.02, n).astype(np.float32),
            "group": which.astype(np.int32)}
    locs = pd.DataFrame({c: v[order] for c, v in cols.items()})
    info = [{"Frames": n_frames, "Width": 128, "Height": 128}]
    events = postprocess.link(locs, info, r_max=0.2, max_dark_time=1)
    assert 15000 < len(events) <= 20000 and events["group"].nunique() == n_sites
    host = {c: events[c].to_numpy() for c in events.columns}
    want_dark = rs.dark_times(host)
    got_dark = postprocess.dark_times(events)
    assert same(got_dark, want_dark) and (want_dark > 0).sum() > 10000
    kept = postprocess.compute_dark_times(events)
    assert same(events["dark"].to_numpy(), np.int32(want_dark)) and len(kept) == int((want_dark != -1).sum())
    got = postprocess.groupprops(kept)
    assert len(got) == n_sites
    assert_props(got, rs.groupprops({c: events[c].to_numpy() for c in events.columns}), "linked sites")


def test_group_sizes_at_the_block_split_and_chunk_boundaries():
    """Groups of exactly 1 .. 16385 rows, interleaved in table order, NaN in one float32 column."""
    rng = np.random.default_rng(13)
    which = rng.permutation(np.repeat(np.arange(len(BOUNDARY_SIZES)), BOUNDARY_SIZES))
    n = len(which)
    cols = {"frame": rng.integers(0, 2 ** 31, n).astype(np.uint32),
            "x": (1000.25 + rng.normal(0, 0.01, n)).astype(np.float32),
            "photons": (rng.standard_normal(n) * 10.0 ** rng.uniform(-6, 6, n)).astype(np.float32),
            "lpx": rng.standard_normal(n) * 10.0 ** rng.uniform(-3, 3, n),
            "group": (which * 5 - 11).astype(np.int32),
            "dark": rng.integers(1, 9000, n).astype(np.int32)}
    cols["photons"][rng.integers(0, n, 300)] = np.nan
    got = postprocess.groupprops(pd.DataFrame(cols))
    assert tuple(got["n_events"]) == BOUNDARY_SIZES
    assert_props(got, rs.groupprops(cols), "boundaries")
