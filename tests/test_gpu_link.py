"""GPU tier: link and NeNA on the device (picasso_amd/postprocess.py, csrc/link.hip) against the reference's recorded
results (tests/golden/link_cases.npz) and the test-side restatement (tests/golden/_link_restate.py).  Every
comparison is on every row and is an equality of bits."""
import json
import sys

import numpy as np
import pandas as pd
import pytest

from conftest import GOLDEN, golden

sys.path.insert(0, GOLDEN)
import _link_restate as rs  # noqa: E402

from picasso_amd import backend, postprocess  # noqa: E402

pytestmark = pytest.mark.gpu
CASES = [str(c) for c in golden("link_cases")["case_names"]]


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
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def assert_frames_equal(got: pd.DataFrame, want: dict, label):
    assert list(got.columns) == list(want), label
    for c in want:
        assert same(got[c].to_numpy(), want[c]), (label, c)


@pytest.mark.parametrize("name", CASES)
def test_link_groups_equal_the_reference(g, name):
    p, kw, cols, group = case(g, name)
    got = postprocess._get_link_groups(cols["frame"], cols["x"], cols["y"], kw["r_max"], kw["max_dark_time"], group)
    assert got.dtype == np.int32 and np.array_equal(got, g[p + "link_group"])


@pytest.mark.parametrize("name", CASES)
def test_combined_columns_equal_the_reference(g, name):
    p, kw, cols, group = case(g, name)
    locs, info = pd.DataFrame(cols), [{"Frames": kw["Frames"]}]
    every = postprocess._link_loc_groups(locs, info, g[p + "link_group"], remove_ambiguous_lengths=False)
    want = {str(c): g[p + "all_" + str(c)] for c in g[p + "all_columns"]}
    assert_frames_equal(every, want, name)
    kept = postprocess._link_loc_groups(locs, info, g[p + "link_group"])
    assert np.array_equal(kept.index.to_numpy(), g[p + "kept"])
    assert_frames_equal(kept, {c: v[g[p + "kept"]] for c, v in want.items()}, name)


@pytest.mark.parametrize("name", CASES)
def test_histogram_equals_the_reference(g, name):
    p, kw, cols, group = case(g, name)
    seen = []
    centers, dnfl = postprocess._nfndh(cols["frame"], cols["x"], cols["y"], group, 1.0, 0.001, seen.append)
    assert same(dnfl, g[p + "dnfl"]) and same(centers, g[p + "bin_centers"])
    assert seen == list(range(1, 101))


def test_frame_index(g):
    p, kw, cols, group = case(g, "e_gaps_offset")
    f = cols["frame"].astype(np.int64)
    t = backend.LinkTable(cols["frame"], cols["x"], cols["y"], group)
    for k in (1, 4, 11):
        lo, hi = (v.cpu().numpy() for v in t.frame_index(k))
        assert np.array_equal(lo, np.searchsorted(f, f + 1, side="left"))
        assert np.array_equal(hi, np.searchsorted(f, f + k, side="right"))


def shuffled(cols, seed):
    order = np.random.default_rng(seed).permutation(len(cols["x"]))
    return pd.DataFrame({c: v[order] for c, v in cols.items()})


@pytest.mark.parametrize("name", CASES)
def test_link_top_level(g, name):
    p, kw, cols, group = case(g, name)
    info = [{"Frames": kw["Frames"]}]
    locs = shuffled(cols, 11)
    before = locs.copy()
    got = postprocess.link(locs, info, r_max=kw["r_max"], max_dark_time=kw["max_dark_time"])
    assert locs.equals(before)                                        # link works on a sorted copy
    s = locs.sort_values(kind="quicksort", by="frame")
    grp = s["group"].to_numpy() if "group" in s.columns else np.zeros(len(s), np.int32)
    lg = postprocess._get_link_groups(s["frame"].to_numpy(), s["x"].to_numpy(), s["y"].to_numpy(), kw["r_max"],
                                      kw["max_dark_time"], grp)
    want = postprocess._link_loc_groups(s, info, lg)
    assert got.index.equals(want.index)
    assert_frames_equal(got, {c: want[c].to_numpy() for c in want.columns}, name)
    if kw["uncontested"]:          # the order inside a frame cannot change a group: the golden, up to the row order
        order = np.lexsort((got["x"].to_numpy(), got["frame"].to_numpy()))
        kept = g[p + "kept"]
        ref = {str(c): g[p + "all_" + str(c)][kept] for c in g[p + "all_columns"]}
        ref_order = np.lexsort((ref["x"], ref["frame"]))
        assert_frames_equal(got.iloc[order], {c: v[ref_order] for c, v in ref.items()}, name)


def _model(d, delta_a, s, ac, dc, sc):
    a = ac + delta_a
    p_single = a * (d / (2 * s**2)) * np.exp(-(d**2) / (4 * s**2))
    p_short = ac / (sc * np.sqrt(2 * np.pi)) * np.exp(-0.5 * ((d - dc) / sc) ** 2)
    return p_single + p_short


def _fit(bin_centers, dnfl, locs):
    """The reference's curve_fit call (postprocess.py:1097-1101), made here."""
    from scipy.optimize import curve_fit
    area = np.trapezoid(dnfl, bin_centers)
    median_lp = np.mean([np.median(locs["lpx"]), np.median(locs["lpy"])])
    p0 = [0.8 * area, median_lp, 0.1 * area, 2 * median_lp, median_lp]
    bounds = ([0, 0, 0, 0, 0], [np.inf, np.inf, np.inf, np.inf, np.inf])
    return curve_fit(_model, bin_centers, dnfl, p0=p0, bounds=bounds)[0]


def _check_result(result, s, locs, centers, dnfl):
    assert same(result["data"], dnfl) and same(result["d"], centers)
    popt = _fit(centers, dnfl, locs)
    assert s == popt[1]
    assert list(result["best_values"]) == ["delta_a", "s", "ac", "dc", "sc"]
    assert list(result["best_values"].values()) == list(popt)
    assert same(result["best_fit"], _model(centers, *popt)) and result["pixelsize"] == 130


@pytest.mark.parametrize("name", ["n_order_free_f32", "n_order_free_f64"])
@pytest.mark.parametrize("shuffle", [False, True])
def test_nena_top_level_equals_the_reference(g, name, shuffle):
    """nena() sorts the table itself (unstable, in place), and which rows fall into the skipped tail and which row is
    the table's last depends on the order inside a frame.  These cases hold a multiple of 100 rows and one row alone
    in the last frame, so their histogram does not: it is the golden's, however the rows arrive."""
    p, kw, cols, group = case(g, name)
    locs = shuffled(cols, 5) if shuffle else pd.DataFrame(cols)
    seen = []
    result, s = postprocess.nena(locs, [{"Frames": kw["Frames"], "Pixelsize": 130}], callback=seen.append)
    assert seen == list(range(1, 101))
    _check_result(result, s, locs, g[p + "bin_centers"], g[p + "dnfl"])


@pytest.mark.parametrize("name", ["a_testdata", "b_blink_f32", "c_blink_f64", "f_groups", "i_long"])
def test_nena_top_level_equals_the_restatement(g, name):
    """Any table: the histogram of nena() against the test-side restatement (which reproduces every golden on the CPU
    tier) on the table as nena() sorted it."""
    p, kw, cols, group = case(g, name)
    locs = shuffled(cols, 9)
    result, s = postprocess.nena(locs, [{"Frames": kw["Frames"], "Pixelsize": 130}])
    grp = locs["group"].to_numpy() if "group" in locs.columns else np.zeros(len(locs), np.int32)
    centers, dnfl = rs.nfndh(locs["frame"].to_numpy(), locs["x"].to_numpy(), locs["y"].to_numpy(), grp)
    assert same(centers, g[p + "bin_centers"])
    _check_result(result, s, locs, centers, dnfl)


def test_nena_sorts_in_place(g):
    p, kw, cols, group = case(g, "b_blink_f32")
    locs = shuffled(cols, 3)
    want = locs.sort_values(kind="quicksort", by="frame")
    centers, dnfl = postprocess._next_frame_neighbor_distance_histogram(locs)
    assert locs.equals(want)
    grp = want["group"].to_numpy() if "group" in want.columns else np.zeros(len(want), np.int32)
    assert same(dnfl, rs.nfndh(want["frame"].to_numpy(), want["x"].to_numpy(), want["y"].to_numpy(), grp)[1])


def test_empty_groups_and_negative_labels(g):
    """_link_loc_groups takes any labelling: a group without rows gets the reference's start values."""
    p, kw, cols, group = case(g, "a_testdata")
    lg = g[p + "link_group"].copy()
    lg[lg == 5] = 6
    locs, info = pd.DataFrame(cols), [{"Frames": kw["Frames"]}]
    got = postprocess._link_loc_groups(locs, info, lg, remove_ambiguous_lengths=False)
    assert got["n"][5] == 0 and got["frame"][5] == cols["frame"].max() and np.isnan(got["x"][5])
    assert got["photons"][5] == 0
    with pytest.raises(ValueError):
        postprocess._link_loc_groups(locs, info, -np.ones(len(lg), np.int32))


def _compare_with_restatement(cols, n_frames, label):
    group = np.zeros(len(cols["x"]), np.int32)
    lg = postprocess._get_link_groups(cols["frame"], cols["x"], cols["y"], 0.05, 3, group)
    assert np.array_equal(lg, rs.link_groups(cols["frame"], cols["x"], cols["y"], 0.05, 3, group)), label
    got = postprocess._link_loc_groups(pd.DataFrame(cols), [{"Frames": n_frames}], lg)
    assert_frames_equal(got, rs.link_loc_groups(cols, n_frames, lg), label)
    centers, dnfl = postprocess._nfndh(cols["frame"], cols["x"], cols["y"], group, 1.0, 0.001)
    want = rs.nfndh(cols["frame"], cols["x"], cols["y"], group)
    assert same(dnfl, want[1]) and same(centers, want[0]), label
    return lg, dnfl


def test_bench_scale_table_equals_the_restatement():
    """The table of bench.py's movie (10 000 frames of 512 x 512, 116 emitters per frame, about 1e6 rows), localized here."""
    import torch
    from picasso_amd import synth
    cam = {"Baseline": 100.0, "Sensitivity": 1.0, "Gain": 1.0}
    movie = synth.simulate_movie(10000, 512, 512, emitters_per_frame=116, device="cuda:0")
    torch.cuda.synchronize()
    table = backend.localize_mle_device(movie.data_ptr(), np.uint16, tuple(movie.shape), 7, 5000, cam)
    del movie
    torch.cuda.empty_cache()
    assert len(table["frame"]) > 900_000
    order = np.argsort(table["frame"], kind="stable")
    cols = {c: np.ascontiguousarray(np.asarray(table[c])[order]) for c in table}
    cols = {("likelihood" if c == "log_likelihood" else c): v for c, v in cols.items() if not c.endswith("_unc")}
    lg, dnfl = _compare_with_restatement(cols, 10000, "bench scale")
    assert lg.max() + 1 > 0.5 * len(lg) and dnfl.sum() > 0


def test_blinking_in_place_equals_the_restatement():
    """Every emitter blinks in place for hundreds of frames: long chains, long groups, a float64 x / y."""
    rng = np.random.default_rng(5)
    n_emitters, n_frames = 1500, 2000
    ex, ey = rng.uniform(2, 254, n_emitters), rng.uniform(2, 254, n_emitters)
    on = rng.random((n_emitters, n_frames)) < 0.3
    em, fr = np.nonzero(on)
    order = np.argsort(fr, kind="stable")
    em, fr = em[order], fr[order]
    n = len(fr)
    cols = {"frame": fr.astype(np.uint32), "x": ex[em] + rng.normal(0, 0.015, n), "y": ey[em] + rng.normal(0, 0.015, n)}
    for c in ("photons", "sx", "bg", "lpx", "lpy"):
        cols[c] = rng.uniform(0.01, 0.05 if c.startswith("lp") else 900.0, n).astype(np.float32)
    lg, dnfl = _compare_with_restatement(cols, n_frames, "blinking in place")
    assert np.bincount(lg).max() > 20 and n > 800_000
    f32 = dict(cols, x=cols["x"].astype(np.float32), y=cols["y"].astype(np.float32))
    _compare_with_restatement(f32, n_frames, "blinking in place, float32")
