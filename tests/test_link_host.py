"""CPU tier: link and NeNA (picasso_amd/postprocess.py, csrc/link.hip) without a device.

The test-side restatement (tests/golden/_link_restate.py: a k-d tree for the candidate pairs, a replay on adjacency
lists, member-by-member group sums, a bincount) reproduces every array of tests/golden/link_cases.npz, which pins
the window quirks, the float32-square / float64-compare rule and the summation order without a GPU; the surface
(signatures, deprecation warnings, the refit error, the empty table, install()) and the ABI are checked as well."""
import inspect
import json
import os
import sys
import types
import warnings

import numpy as np
import pandas as pd
import pytest

from conftest import GOLDEN, golden

sys.path.insert(0, GOLDEN)
import _link_restate as rs  # noqa: E402

from picasso_amd import _lib, localize, postprocess  # noqa: E402

CASES = [str(c) for c in golden("link_cases")["case_names"]]

# parameter lists of the reference (picasso/postprocess.py, picasso/localize.py): (name, default)
_NO = "<required>"
SIGNATURES = {
    "link": [("locs", _NO), ("info", _NO), ("r_max", 0.05), ("max_dark_time", 3), ("combine_mode", "average"),
             ("remove_ambiguous_lengths", True)],
    "_get_link_groups": [(p, _NO) for p in ("frame", "x", "y", "d_max", "max_dark_time", "group")],
    "get_link_groups": [(p, _NO) for p in ("frame", "x", "y", "d_max", "max_dark_time", "group")],
    "_link_loc_groups": [("locs", _NO), ("info", _NO), ("link_group", _NO), ("remove_ambiguous_lengths", True)],
    "link_loc_groups": [("locs", _NO), ("info", _NO), ("link_group", _NO), ("remove_ambiguous_lengths", True)],
    "nena": [("locs", _NO), ("info", None), ("callback", None)],
    "_next_frame_neighbor_distance_histogram": [("locs", _NO), ("callback", None)],
    "next_frame_neighbor_distance_histogram": [("locs", _NO), ("callback", None)],
}
CHECK_SIGNATURES = {
    "check_nena": [("locs", _NO), ("info", _NO), ("callback", None)],
    "check_kinetics": [("locs", _NO), ("info", _NO)],
}


@pytest.fixture(scope="module")
def g():
    return golden("link_cases")


def case(g, name):
    p = name + "/"
    kw = json.loads(str(g[p + "kwargs"]))
    cols = {str(c): g[p + "in_" + str(c)] for c in g[p + "in_columns"]}
    group = cols["group"] if "group" in cols else np.zeros(len(cols["x"]), np.int32)
    return p, kw, cols, group


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


@pytest.mark.parametrize("name", CASES)
def test_restatement_reproduces_link_groups(g, name):
    p, kw, cols, group = case(g, name)
    got = rs.link_groups(cols["frame"], cols["x"], cols["y"], kw["r_max"], kw["max_dark_time"], group)
    assert got.dtype == np.int32 and np.array_equal(got, g[p + "link_group"])


@pytest.mark.parametrize("name", CASES)
def test_restatement_reproduces_every_combined_column(g, name):
    p, kw, cols, group = case(g, name)
    lg = g[p + "link_group"]
    out = rs.link_loc_groups(cols, kw["Frames"], lg, remove_ambiguous_lengths=False)
    assert list(out) == [str(c) for c in g[p + "all_columns"]]
    for c, v in out.items():
        assert same(np.ascontiguousarray(v), g[p + "all_" + c]), (name, c)
    kept = rs.link_loc_groups(cols, kw["Frames"], lg, remove_ambiguous_lengths=True)
    assert same(kept["n"], g[p + "all_n"][g[p + "kept"]])


@pytest.mark.parametrize("name", CASES)
def test_restatement_reproduces_the_histogram(g, name):
    p, kw, cols, group = case(g, name)
    centers, dnfl = rs.nfndh(cols["frame"], cols["x"], cols["y"], group)
    assert same(dnfl, g[p + "dnfl"]) and same(centers, g[p + "bin_centers"])


def test_goldens_hold_what_they_are_for(g):
    """The cases the float32 rule, the contested rows and the NeNA quirks were written for do decide something."""
    p, kw, cols, group = case(g, "h_ulps")
    n = np.bincount(g[p + "link_group"])
    assert (n == 2).sum() >= 6 and (n == 1).sum() >= 12             # pairs on either side of r_max
    x64, y64 = cols["x"].astype(np.float64), cols["y"].astype(np.float64)
    in64 = rs.link_groups(cols["frame"], x64, y64, kw["r_max"], kw["max_dark_time"], group)
    assert not np.array_equal(in64, g[p + "link_group"])              # float64 arithmetic decides some otherwise
    p, kw, cols, group = case(g, "m_nena_tail")
    dnfl = g[p + "dnfl"]
    assert dnfl.sum() == 3 and len(cols["x"]) % 100 == 20
    assert dnfl[90:110].sum() == 1 and dnfl[240:255].sum() == 1 and dnfl[490:510].sum() == 1
    everyone, _, d2 = rs.candidates(cols["frame"], cols["x"], cols["y"], group, 1.0, 1)      # link's windows: no quirk
    far = np.sqrt(d2.astype(np.float64))
    assert ((far > 0.59) & (far < 0.61)).sum() == 1 and dnfl[585:615].sum() == 0   # a pair inside the skipped tail: absent
    assert ((far > 0.79) & (far < 0.81)).sum() == 1 and dnfl[785:815].sum() == 0   # the last row as a neighbour: absent
    assert everyone[(far > 0.59) & (far < 0.61)][0] >= 100
    for name in ("n_order_free_f32", "n_order_free_f64"):                          # what makes them order-free
        f = case(g, name)[2]["frame"]
        assert len(f) % 100 == 0 and (f == f.max()).sum() == 1
    assert len(case(g, "b_blink_f32_n100")[2]["x"]) % 100 == 0
    p, kw, cols, group = case(g, "g_contested")
    lg = g[p + "link_group"]

    def row(frame, x):
        return int(np.flatnonzero((cols["frame"] == frame) & (cols["x"] == np.float32(x)))[0])
    assert lg[row(2, 5.03)] == lg[row(0, 5.00)] != lg[row(0, 5.06)]     # the lower start wins the contested row
    assert lg[row(1, 9.04)] == lg[row(0, 9.00)] != lg[row(1, 9.005)]    # the first candidate, not the nearest
    assert lg[-1] == lg[-3]                                           # the last row taken by a row of its own frame
    assert g["a_testdata/link_group"].max() + 1 == 229 and g["a_testdata_r05/link_group"].max() + 1 == 181
    assert g["a_testdata/dnfl"].sum() == 310


@pytest.mark.parametrize("name", sorted(SIGNATURES))
def test_signatures_equal_the_reference(name):
    got = [(n, _NO if q.default is inspect.Parameter.empty else q.default)
           for n, q in inspect.signature(getattr(postprocess, name)).parameters.items()]
    assert got == SIGNATURES[name]


@pytest.mark.parametrize("name", sorted(CHECK_SIGNATURES))
def test_check_signatures_equal_the_reference(name):
    got = [(n, _NO if q.default is inspect.Parameter.empty else q.default)
           for n, q in inspect.signature(getattr(localize, name)).parameters.items()]
    assert got == CHECK_SIGNATURES[name]
    assert localize.MAX_LOCS == 1_000_000


def _stub(monkeypatch, name, value):
    calls = []

    def fn(*a, **k):
        calls.append((a, k))
        return value
    monkeypatch.setattr(postprocess, name, fn)
    return calls


@pytest.mark.parametrize("alias, target, args", [
    ("get_link_groups", "_get_link_groups", (1, 2, 3, 4, 5, 6)),
    ("link_loc_groups", "_link_loc_groups", (1, 2, 3, False)),
    ("next_frame_neighbor_distance_histogram", "_next_frame_neighbor_distance_histogram", (1, None)),
])
def test_deprecated_aliases_warn_and_forward(monkeypatch, alias, target, args):
    calls = _stub(monkeypatch, target, "result")
    with pytest.warns(DeprecationWarning, match=f"v0.11.0. Use {target} instead"):
        assert getattr(postprocess, alias)(*args) == "result"
    assert calls == [(args, {})]


def _locs(n=0):
    return pd.DataFrame({"frame": np.arange(n, dtype=np.uint32), "x": np.ones(n, np.float32),
                         "y": np.ones(n, np.float32), "photons": np.ones(n, np.float32),
                         "lpx": np.ones(n, np.float32), "lpy": np.ones(n, np.float32)})


def test_empty_table():
    out = postprocess.link(_locs(0), [{"Frames": 10}])
    assert list(out.columns) == ["frame", "x", "y", "photons", "lpx", "lpy", "len", "n", "photon_rate"]
    assert len(out) == 0
    assert out["len"].dtype == np.int32 and out["n"].dtype == np.int32 and out["photon_rate"].dtype == np.float32
    assert out["frame"].dtype == np.uint32
    bare = postprocess.link(pd.DataFrame({"x": np.zeros(0, np.float32)}), [{"Frames": 10}])
    assert list(bare.columns) == ["x"]


def test_refit_is_not_implemented(monkeypatch):
    monkeypatch.setattr(postprocess, "_device_link_groups", lambda *a: (np.zeros(3, np.int32), 1))
    with pytest.raises(NotImplementedError, match="Refit mode is not implemented yet. Please use 'average' mode."):
        postprocess.link(_locs(3), [{"Frames": 10}], combine_mode="refit")


def test_no_device_raises(monkeypatch):
    monkeypatch.setattr(_lib, "device_count", lambda: 0)
    with pytest.raises(_lib.HipBackendError):
        postprocess.link(_locs(5), [{"Frames": 10}])
    with pytest.raises(_lib.HipBackendError):
        postprocess.nena(_locs(5), [{"Frames": 10}])


def test_check_nena_turns_errors_into_nan(monkeypatch, capsys):
    monkeypatch.setattr(_lib, "device_count", lambda: 0)
    assert np.isnan(localize.check_nena(_locs(5), None))
    assert "Calculating NeNA.. " in capsys.readouterr().out


def test_checks_slice_and_forward(monkeypatch, capsys):
    seen = {}

    def nena(locs, info, callback=None):
        seen["nena"] = (len(locs), info, callback)
        return {}, 0.125

    def link(locs, info):
        seen["link"] = (len(locs), info)
        return pd.DataFrame({"len": np.array([2, 4], np.uint32)})
    monkeypatch.setattr(postprocess, "nena", nena)
    monkeypatch.setattr(postprocess, "link", link)
    monkeypatch.setattr(localize, "MAX_LOCS", 4)
    cb = object()
    assert localize.check_nena(_locs(9), "info", cb) == 0.125 and seen["nena"] == (4, "info", cb)
    assert localize.check_kinetics(_locs(9), ["i"]) == 3.0 and seen["link"] == (4, ["i"])
    assert "0.12 px." in capsys.readouterr().out


def test_numba_mean_typing():
    f32, u32 = np.array([16777217.0, 3.0], np.float32), np.array([3, 3], np.uint32)
    got = postprocess._numba_mean(f32, u32)
    assert got.dtype == np.float32 and same(got, f32 / u32.astype(np.float32))
    ints = postprocess._numba_mean(np.array([7, 4000000000], np.uint32), u32)
    assert same(ints, (np.array([7, 4000000000], np.float64) / 3).astype(np.float32))
    mixed = postprocess._numba_mean(np.array([1.0, 2.0]), np.array([3.0, 7.0], np.float32))
    assert same(mixed, (np.array([1.0, 2.0]) / np.array([3.0, 7.0])).astype(np.float32))


def test_squared_like_numba():
    assert postprocess._squared_like_numba(0.05) == 0.05 * 0.05
    assert postprocess._squared_like_numba(np.float32(0.05)) == float(np.float32(0.05) * np.float32(0.05))
    assert postprocess._squared_like_numba(2) == 4.0


def test_install_rebinds_link_and_nena():
    mods = {n: types.ModuleType("picasso." + n) for n in
            ("localize", "gaussmle", "gausslq", "zfit", "render", "imageprocess", "postprocess", "aim")}
    localize.install(mods["localize"], mods["gaussmle"], mods["gausslq"], mods["zfit"], mods["render"],
                     mods["imageprocess"], mods["postprocess"], picasso_aim=mods["aim"])
    for name in SIGNATURES:
        assert getattr(mods["postprocess"], name) is getattr(postprocess, name)
    assert set(SIGNATURES) == set(postprocess.LINK_NENA_NAMES)
    for name in CHECK_SIGNATURES:
        assert getattr(mods["localize"], name) is getattr(localize, name)
    for name in ("segment", "undrift"):
        assert getattr(mods["postprocess"], name) is getattr(postprocess, name)


def test_abi_version_and_symbols():
    assert _lib.load().pmi_version() >= 109
    for name in ("pmi_link_frame_index_dev", "pmi_link_groups_dev", "pmi_link_combine_dev", "pmi_nena_hist_dev"):
        assert name in _lib.SYMBOLS and hasattr(_lib.load(), name)


def test_goldens_regenerate(g):
    """The committed link_cases.npz is what make_goldens_link.py mints from the reference tree today."""
    ref = os.environ.get("PICASSO_REFERENCE", "/root/reference")
    if not os.path.isfile(os.path.join(ref, "picasso", "postprocess.py")):
        pytest.skip("reference tree not present")
    import make_goldens_link as mk
    ns = mk.load_reference()
    cases = mk.cases()
    assert list(cases) == CASES
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for name in ("a_testdata", "g_contested", "h_ulps", "j_edges_z_lpz", "m_nena_tail"):
            cols, n_frames, kw, _ = cases[name]
            lg, every, kept, centers, dnfl = mk.run_case(ns, cols, n_frames, kw)
            p = name + "/"
            assert np.array_equal(lg, g[p + "link_group"]) and np.array_equal(kept, g[p + "kept"])
            for c in every.columns:
                assert same(every[c].to_numpy(), g[p + "all_" + c]), (name, c)
            assert same(dnfl, g[p + "dnfl"])
            for c, v in cols.items():
                assert same(np.ascontiguousarray(v), g[p + "in_" + c]), (name, c)
