"""Pick kinetics on the device (csrc/cumexp.hip and the wrappers of picasso_amd.postprocess / picasso_amd.lib) against the
reference's results recorded in tests/golden/pickkin_cases.npz.

Per fitted segment (tests/golden/_pickkin_restate.check_batch):
    cost(a, t, c) <= cost_reference * (1 + 1e-12)      the cost recomputed on the host in float64 from the returned parameters
    |t - t_reference| <= tol * t_reference             tol = 4 g = 8.34e-5, g = 2.09e-5 the reference's own largest relative
                                                       gap to the tightly converged optimum, measured at mint time
Segments the reference does not fit are equal in every bit; the wrappers' rows, columns, dtypes, counts and RMSDs are equal
to the goldens, their rates within ``tol``.
"""
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import _pickkin_restate as rs  # noqa: E402

pytestmark = pytest.mark.gpu

G = np.load(os.path.join(ROOT, "tests", "golden", "pickkin_cases.npz"))
BATCHES = json.loads(str(G["batches"]))
WRAPPERS = json.loads(str(G["wrappers"]))
INFO = json.loads(str(G["info"]))
TOL = float(G["tol"])
RATES = ("n_units", "length_cdf", "dark_cdf", "qpaint_idx_cdf")


def close(got, want):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape
    assert np.array_equal(np.isnan(got), np.isnan(want))
    ok = ~np.isnan(want)
    assert (np.abs(got[ok] - want[ok]) <= TOL * np.abs(want[ok])).all(), (got, want)


@pytest.mark.parametrize("name", BATCHES)
def test_fit_batches(name):
    from picasso_amd import backend
    values = G[name + "_values"]
    before = values.copy()
    rates = backend.kinetic_rates(values, G[name + "_offsets"])
    assert np.array_equal(values, before, equal_nan=True)
    fit, info = np.stack([rates.a, rates.t, rates.c, rates.cost]), np.stack([rates.iterations, rates.status])
    print(name, "iterations: max", int(info[0].max()), "statuses", np.bincount(info[1], minlength=3).tolist())
    rs.check_batch(G, name, fit, info)


def test_segments_do_not_depend_on_their_neighbours():
    """The mixed batch again, cut at another place: every segment gives the bits it gave inside the whole batch."""
    from picasso_amd import backend
    values, offsets = G["mixed_i32_values"], G["mixed_i32_offsets"]
    whole = backend.kinetic_rates(values, offsets)
    lo, hi = 101, 230
    part = backend.kinetic_rates(values[offsets[lo]:offsets[hi]], offsets[lo:hi + 1] - offsets[lo])
    for a, b in zip(whole, part):
        assert rs.same_bits(a[lo:hi], b)


def test_bad_offsets_and_types():
    from picasso_amd import backend
    with pytest.raises(ValueError):
        backend.kinetic_rates(np.arange(5), [0, 3, 2, 5])
    with pytest.raises(ValueError):
        backend.kinetic_rates(np.arange(5), [0, 6])
    with pytest.raises(TypeError):
        backend.kinetic_rates(np.zeros(3, np.complex64), [0, 3])
    empty = backend.kinetic_rates(np.zeros(0, np.int32), [0])
    assert len(empty.t) == 0


def test_lib_functions():
    from picasso_amd import lib
    name = "edges_i32"
    values, offsets, mode = G[name + "_values"], G[name + "_offsets"], G[name + "_mode"]
    for s in range(len(mode)):
        data = values[offsets[s]:offsets[s + 1]].copy()
        rate = lib.estimate_kinetic_rate(data)
        if mode[s] == 1:
            assert abs(rate - G[name + "_rate"][s]) <= TOL * G[name + "_rate"][s]
            assert (np.diff(data) >= 0).all()                       # sorted in place, as the reference's is
        else:
            assert rate == G[name + "_rate"][s] or (rate != rate and len(data) == 0)
    s = int(np.flatnonzero(mode == 1)[3])
    data = values[offsets[s]:offsets[s + 1]].copy()
    result = lib.fit_cum_exp(data)
    assert set(result) == {"best_values", "data", "best_fit"} and result["data"] is data
    best = result["best_values"]
    assert rs.cost(data, (best["a"], best["t"], best["c"])) <= G[name + "_ref_cost"][s] * (1 + rs.COST_MARGIN)
    assert np.array_equal(result["best_fit"], lib.cumulative_exponential(data, best["a"], best["t"], best["c"]))
    with pytest.raises(ValueError):
        lib.estimate_kinetic_rate(np.array([1.0, 2.0, np.nan, 4.0]))


@pytest.mark.parametrize("name", WRAPPERS)
def test_pick_kinetics(name):
    from picasso_amd import postprocess
    picks, seen = rs.picks_of(G, name), []
    length, dark, no_locs, out_locs = postprocess.pick_kinetics(picks, INFO, max_dark_time=3, progress_callback=seen.append)
    assert seen == G[name + "_pk_callbacks"].tolist()
    assert rs.same_bits(no_locs, G[name + "_pk_no_locs"])
    rs.assert_table(out_locs, G, name + "_pk_out")
    close(length, G[name + "_pk_length"])
    close(dark, G[name + "_pk_dark"])


@pytest.mark.parametrize("name", WRAPPERS)
def test_evaluate_picks(name):
    from picasso_amd import postprocess
    picks, seen = rs.picks_of(G, name), []
    N, n_events, rmsd, rmsd_z, length, dark, new_locs = postprocess.evaluate_picks(picks, INFO, max_dark_time=3,
                                                                                   progress_callback=seen.append)
    assert seen == G[name + "_ev_callbacks"].tolist()
    filled = G[name + "_ev_filled"]
    assert np.isnan(N[~filled]).all() and np.isnan(rmsd[~filled]).all() and np.isnan(length[~filled]).all()
    assert rs.same_bits(N[filled], G[name + "_ev_N"][filled]) and rs.same_bits(n_events[filled], G[name + "_ev_n_events"][filled])
    assert rs.same_bits(rmsd[filled], G[name + "_ev_rmsd"][filled])
    if bool(G[name + "_ev_has_z"]):
        assert rs.same_bits(rmsd_z[filled], G[name + "_ev_rmsd_z"][filled])
    else:
        assert np.isnan(rmsd_z).all()
    rs.assert_table(new_locs, G, name + "_ev_new")
    close(length[filled], G[name + "_ev_length"][filled])
    close(dark[filled], G[name + "_ev_dark"][filled])


@pytest.mark.parametrize("name", [w for w in WRAPPERS if w + "_pp_columns" in G.files])
def test_pick_properties(name):
    from picasso_amd import postprocess
    seen_k, seen_g = [], []
    props = postprocess.pick_properties(rs.picks_of(G, name), INFO, max_dark_time=3, influx_rate=0.04,
                                        pick_areas=G[name + "_pp_areas"], kinetics_progress=seen_k.append,
                                        groupprops_progress=seen_g.append)
    assert seen_k == G[name + "_pp_callbacks_k"].tolist() and seen_g == G[name + "_pp_callbacks_g"].tolist()
    rs.assert_table(props, G, name + "_pp", close=RATES, tol=TOL)


def test_single_pick_and_last_frame_quirk():
    """One pick through ``_pick_kinetics_single``; and a pick whose last frame holds two localizations, which the batch
    links in a call of its own, gives what ``link`` + ``compute_dark_times`` give for it alone."""
    from picasso_amd import postprocess
    picks = rs.picks_of(G, "plain")
    single = postprocess._pick_kinetics_single(picks[0], INFO, 3)
    n0 = int(G["plain_pk_no_locs"][0])
    assert single is not None and len(single[0]) == n0
    close(np.float64(single[1]), np.float64(G["plain_pk_length"][0]))
    assert postprocess._pick_kinetics_single(picks[1], INFO, 3) is None
    odd = picks[3].copy()
    extra = odd.iloc[[-1]].copy()
    extra["x"] += np.float32(0.01)
    odd = postprocess.pd.concat([odd, extra], ignore_index=True)
    both = postprocess.pick_kinetics([picks[0], odd, picks[5]], INFO, max_dark_time=3)
    alone = postprocess.compute_dark_times(postprocess.link(odd, INFO, r_max=999999, max_dark_time=3))
    n1 = int(both[2][1])
    block = both[3].iloc[n0:n0 + n1]
    assert n1 == len(alone)
    for c in alone.columns:
        if c not in ("len", "dark"):
            assert np.array_equal(block[c].to_numpy(), alone[c].to_numpy()), c
        else:
            assert np.array_equal(np.sort(block[c].to_numpy()), np.sort(alone[c].to_numpy())), c
