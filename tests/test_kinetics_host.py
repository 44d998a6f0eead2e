"""CPU tier of the dark times and the group properties (picasso_amd/postprocess.py compute_dark_times / dark_times /
_dark_times / groupprops, csrc/kinetics.hip): the test-side restatement (tests/golden/_kinetics_restate.py) reproduces
every array the reference recorded (tests/golden/kinetics_cases.npz), its sum is NumPy's ``ndarray.sum()`` in bits and
its mean / std are pandas' at the chunk boundaries, the library exports the new entries, ``install()`` rebinds the
functions, and the checks that come before any device work behave as the reference's."""
import inspect
import json
import sys
import types

import numpy as np
import pandas as pd
import pytest

from conftest import GOLDEN, golden

sys.path.insert(0, GOLDEN)
import _kinetics_restate as rs  # noqa: E402

from picasso_amd import _lib, localize, postprocess  # noqa: E402

G = golden("kinetics_cases")
DARK_CASES = [str(c) for c in G["dark_case_names"]]
PROPS_CASES = [str(c) for c in G["props_case_names"]]
SUM_SIZES = list(range(1, 301)) + [1000, 5000, 8191, 8192, 8193, 8200, 16384, 16385, 16386, 20000, 50000]


@pytest.fixture(scope="module")
def g():
    return G


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def dark_case(g, name):
    p = "dark/" + name + "/"
    cols = {str(c): g[p + "in_" + str(c)] for c in g[p + "in_columns"]}
    return p, cols, (g[p + "arg_group"] if p + "arg_group" in g.files else None)


def props_case(g, name):
    p = "props/" + name + "/"
    return p, {str(c): g[p + "in_" + str(c)] for c in g[p + "in_columns"]}


def props_want(g, p):
    return {str(c): g[p + "out_" + str(c)] for c in g[p + "columns"]}


@pytest.mark.parametrize("name", DARK_CASES)
def test_restated_dark_times_reproduce_the_reference(g, name):
    p, cols, group = dark_case(g, name)
    assert same(rs.dark_times(cols, group), g[p + "dark"]), name


@pytest.mark.parametrize("name", PROPS_CASES)
def test_restated_group_properties_reproduce_the_reference(g, name):
    p, cols = props_case(g, name)
    got, want = rs.groupprops(cols), props_want(g, p)
    assert list(got) == list(want)
    assert [str(v.dtype) for v in got.values()] == [str(d) for d in g[p + "dtypes"]]
    for c in want:
        assert same(got[c], want[c]), (name, c)


def test_cases_hold_the_hard_parts(g):
    d = {k: g["dark/" + k + "/dark"] for k in DARK_CASES}
    assert len(d["one_row"]) == 1 and (d["singles_300"] == -1).all() and len(d["one_group_300"]) == 300
    assert "group" not in dark_case(g, "one_group_300")[1] and "group" in dark_case(g, "sites_column")[1]
    assert not same(d["sites_column"], d["sites_split_i64"]) and same(d["sites_split_i64"], d["sites_split_f64"])
    assert [dark_case(g, k)[2].dtype for k in ("sites_split_i64", "sites_split_f64", "sites_i32_arg_no_column")] == \
        [np.int64, np.float64, np.int32]
    assert d["edges_u32"].dtype == np.int64 and d["edges_i64"].dtype == np.int64 and d["edges_i32_unsorted"].dtype == np.int32
    for k in ("edges_u32", "edges_i64"):
        cols = dark_case(g, k)[1]
        grp, f = cols["group"], cols["frame"].astype(np.int64)
        at = lambda a, b: int(np.flatnonzero((grp == a) & (f == b))[0])  # noqa: E731
        assert grp.min() < 0 and (cols["len"] == 0).sum() == 5 and (np.diff(f) < 0).any()
        assert d[k][at(-4, 100)] == 1 and d[k][at(0, 100)] == 10                  # the row itself is stepped over
        assert d[k][at(3, 20)] == -1 and d[k][at(3, 30)] == 1                      # overlap in time
        assert d[k][at(7, 11)] == 1                                                # three equal last frames
        assert f.max() == 5000 and d[k][at(12, 5000)] == -1 and d[k][at(500, 5000)] == -1
        assert d[k][at(501, 7)] == (8 if k == "edges_i64" else -1)                 # 0 + 0 - 1, signed and wrapped
    cols = dark_case(g, "edges_u32")[1]
    assert rs.last_frames(cols["frame"], cols["len"]).dtype == np.uint32
    assert rs.last_frames(cols["frame"], cols["len"]).max() == 2 ** 32 - 1

    p, cols = props_case(g, "edges")
    e = props_want(g, p)
    ids = list(e["group"])
    assert ids[0] < 0 and (np.diff(ids) > 1).any() and len(g["props/groups300/out_group"]) == 300
    assert e["n_events"][ids.index(5)] == 1 and np.isnan(e["x_std"][ids.index(5)])
    assert np.isnan(cols["photons"][cols["group"] == 40]).all() and np.isnan(e["photons_mean"][ids.index(40)])
    assert np.isfinite(e["photons_mean"][ids.index(9)]) and np.isnan(cols["photons"][cols["group"] == 9]).any()
    assert np.isinf(e["x_mean"][ids.index(41)]) and np.isnan(e["y_mean"][ids.index(41)])
    assert cols["lpx"].dtype == np.float64 and cols["frame"].dtype == np.uint32 and cols["ok"].dtype == bool
    assert all(cols[c].dtype == np.int32 for c in ("len", "n", "dark")) and (cols["dark"] == -1).sum() > 10
    assert (np.diff(cols["group"]) != 0).mean() > 0.8
    assert list(e)[:4] == ["group", "n_events", "frame_mean", "frame_std"] and list(e)[-1] == "qpaint_idx"
    assert set(json.loads(str(g["versions"]))) == {"pandas", "numpy", "scipy"}


def _sweep_arrays(n, rng):
    return {"float32": (rng.standard_normal(n) * 10.0 ** rng.uniform(-6, 6, n)).astype(np.float32),
            "float64": rng.standard_normal(n) * 10.0 ** rng.uniform(-3, 3, n),
            "uint32": rng.integers(0, 2 ** 32, n, dtype=np.uint32),
            "int32": rng.integers(-2 ** 31, 2 ** 31, n).astype(np.int32)}


def test_restated_sum_is_numpys_in_bits():
    """float32 and float64 in their own type, float32 / uint32 / int32 cast to float64, at every size up to 300 and
    around the 8192-element chunks."""
    rng = np.random.default_rng(11)
    for n in SUM_SIZES:
        a = _sweep_arrays(n, rng)
        for name, dtype in (("float32", np.float32), ("float64", np.float64), ("float32", np.float64),
                            ("uint32", np.float64), ("int32", np.float64)):
            want = a[name].sum(dtype=dtype)
            assert same(np.asarray(rs.chunked_sum(a[name], dtype)), np.asarray(want)), (n, name, dtype)


def test_float64_additions_of_the_sweep_round():
    """The sweep's float32 values cast to float64 do not add exactly: the order of the additions shows in the bits."""
    a = _sweep_arrays(5000, np.random.default_rng(11))["float32"]
    assert a.sum(dtype=np.float64) != a[::-1].sum(dtype=np.float64)


@pytest.mark.parametrize("n", [1, 2, 7, 8, 9, 127, 128, 129, 136, 257, 8192, 8193, 16385])
def test_restated_mean_and_std_are_pandas_at_the_boundaries(n):
    """The 8192-row and larger groups are checked against real pandas here, not stored."""
    rng = np.random.default_rng(n)
    a = _sweep_arrays(n, rng)
    a["float32_nan"] = a["float32"].copy()
    a["float32_nan"][rng.integers(0, n, max(n // 50, 1))] = np.nan
    a["bool"] = a["int32"] > 0
    a["near"] = (1000.25 + rng.normal(0, 0.01, n)).astype(np.float32)
    for name, v in a.items():
        s = pd.Series(v)
        want_mean, want_std = s.mean(), s.std()
        got_mean, got_std = rs.series_mean(v.astype(np.int32) if v.dtype == bool else v), rs.series_std(v)
        for got, want in ((got_mean, want_mean), (got_std, want_std)):
            if np.isnan(want):
                assert np.isnan(got), (n, name)
            else:
                assert same(np.asarray(got), np.asarray(want)), (n, name, got, want)


def test_abi_has_the_kinetics_entries():
    lib = _lib.load()
    assert lib.pmi_version() >= 113
    for name in ("pmi_kinetics_dark_order_dev", "pmi_kinetics_dark_search_dev", "pmi_kinetics_stats_dev"):
        assert name in _lib.SYMBOLS and hasattr(lib, name)


def test_kinetics_names_signatures_and_install():
    assert postprocess.KINETICS_NAMES == ("_dark_times", "dark_times", "compute_dark_times", "groupprops")
    assert list(inspect.signature(postprocess._dark_times).parameters) == ["frame", "group", "last_frame"]
    for name in ("dark_times", "compute_dark_times"):
        sig = inspect.signature(getattr(postprocess, name))
        assert list(sig.parameters) == ["locs", "group"] and sig.parameters["group"].default is None
    sig = inspect.signature(postprocess.groupprops)
    assert list(sig.parameters) == ["locs", "callback"] and sig.parameters["callback"].default is None
    mods = {n: types.ModuleType("picasso." + n) for n in
            ("localize", "gaussmle", "gausslq", "zfit", "render", "imageprocess", "postprocess", "aim")}
    theirs = ("get_index_blocks", "picked_locs", "pick_similar", "pick_kinetics", "evaluate_picks", "pick_properties")
    for name in theirs:
        setattr(mods["postprocess"], name, "theirs")
    localize.install(mods["localize"], mods["gaussmle"], mods["gausslq"], mods["zfit"], mods["render"],
                     mods["imageprocess"], mods["postprocess"], picasso_aim=mods["aim"])
    for name in postprocess.KINETICS_NAMES:
        assert getattr(mods["postprocess"], name) is getattr(postprocess, name)
    for name in theirs:
        assert getattr(mods["postprocess"], name) == "theirs"


def test_checks_before_the_device_as_the_reference_recorded(g):
    edges = json.loads(str(g["edges"]))
    _, sites, _ = dark_case(g, "sites_column")
    assert edges["cdt without len"] == {"raises": "AttributeError", "message": "Length not found. Please link localizations first."}
    with pytest.raises(AttributeError) as err:
        postprocess.compute_dark_times(pd.DataFrame({c: v for c, v in sites.items() if c != "len"}))
    assert str(err.value) == edges["cdt without len"]["message"]
    empty = pd.DataFrame({c: v[:0] for c, v in sites.items()})
    for what, fn in (("dark_times empty", postprocess.dark_times), ("cdt empty", postprocess.compute_dark_times)):
        assert edges[what]["raises"] == "ValueError"
        with pytest.raises(ValueError) as err:
            fn(empty)
        assert str(err.value) == edges[what]["message"]
    assert "dark" not in empty.columns

    _, cols = props_case(g, "edges")
    assert edges["groupprops without dark"] == {"raises": "KeyError", "message": "'dark'"}
    with pytest.raises(KeyError) as err:
        postprocess.groupprops(pd.DataFrame({c: v for c, v in cols.items() if c != "dark"}))
    assert str(err.value) == "'dark'"
    tables = {"groupprops empty": pd.DataFrame({c: v[:0] for c, v in cols.items()}),
              "groupprops all filtered": pd.DataFrame({**cols, "dark": np.full(len(cols["dark"]), -1, np.int32)})}
    for what, table in tables.items():
        seen = []
        got = postprocess.groupprops(table, callback=seen.append)
        assert edges[what]["rows"] == 0 and len(got) == 0 and seen == [0]
        assert list(got.columns) == edges[what]["returns"]
        assert [str(got[c].dtype) for c in got.columns] == edges[what]["dtypes"]


def test_group_argument_is_narrowed_by_name():
    _, sites, _ = dark_case(G, "sites_column")
    locs = pd.DataFrame(sites)
    half = sites["group"].astype(np.float64)
    half[3] = 0.5
    with pytest.raises(ValueError, match="group"):
        postprocess.dark_times(locs, half)
    half[3] = np.nan
    with pytest.raises(ValueError, match="group"):
        postprocess.dark_times(locs, half)
    with pytest.raises(TypeError, match="group"):
        postprocess.dark_times(locs, np.array(["a"] * len(locs)))
    with pytest.raises(ValueError, match="frame"):
        postprocess._dark_times(sites["frame"].astype(np.uint64), sites["group"], sites["frame"].astype(np.int64))
    with pytest.raises(ValueError, match="last_frame"):
        postprocess._dark_times(sites["frame"], sites["group"], np.full(len(locs), 2 ** 62, np.int64))
