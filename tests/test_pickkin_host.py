"""Pick kinetics without a GPU: csrc/cumexp_core.h built for the host (tests/cumexp_host_driver.cpp) against the
reference's fits recorded in tests/golden/pickkin_cases.npz, the restatement of what the reference decides before it fits,
the recorded signatures, and the wrapper logic of picasso_amd.postprocess that needs no device (the device calls replaced
by the host driver and a plain dark-time loop).

Acceptance per fitted segment, as on the device (tests/test_gpu_pickkin.py):
    cost(a, t, c) <= cost_reference * (1 + 1e-12)      the cost recomputed here in float64 from the returned parameters
    |t - t_reference| <= tol * t_reference             tol = 4 g, g the reference's own largest relative gap to the tightly
                                                       converged optimum, measured when the goldens were minted
"""
import inspect
import json
import os
import subprocess
import sys

import numpy as np
import pandas as pd
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import _pickkin_restate as rs  # noqa: E402

G = np.load(os.path.join(ROOT, "tests", "golden", "pickkin_cases.npz"))
BATCHES = json.loads(str(G["batches"]))
WRAPPERS = json.loads(str(G["wrappers"]))
INFO = json.loads(str(G["info"]))
TOL = float(G["tol"])


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    d = tmp_path_factory.mktemp("cumexp_host")
    exe = str(d / "cumexp_host_driver")
    subprocess.run([os.environ.get("CXX", "c++"), "-O2", "-std=c++17", "-ffp-contract=off",
                    "-I", os.path.join(ROOT, "picasso_amd", "csrc"), os.path.join(ROOT, "tests", "cumexp_host_driver.cpp"),
                    "-o", exe], check=True)

    def run(values, offsets):
        values, offsets = np.asarray(values), np.ascontiguousarray(offsets, np.int64)
        n = len(offsets) - 1
        src, dst = str(d / "in.bin"), str(d / "out.bin")
        with open(src, "wb") as f:
            np.array([n, len(values), rs.kind_of(values.dtype)], np.int64).tofile(f)
            offsets.tofile(f)
            values.astype(np.float64).tofile(f)
        subprocess.run([exe, src, dst], check=True)
        raw = open(dst, "rb").read()
        fit = np.frombuffer(raw[:n * 32], np.float64).reshape(4, n)
        info = np.frombuffer(raw[n * 32:], np.int32).reshape(2, n)
        return fit, info

    return run


@pytest.mark.parametrize("name", BATCHES)
def test_fit_batches_on_the_host(driver, name):
    fit, info = driver(G[name + "_values"], G[name + "_offsets"])
    rs.check_batch(G, name, fit, info)


def test_fixture_conditions_and_tolerance():
    g = 0.0
    for name in BATCHES:
        fitted = G[name + "_mode"] == 1
        assert (G[name + "_opt_cost"][fitted] <= G[name + "_ref_cost"][fitted]).all()
        ref, opt = G[name + "_ref"][fitted], G[name + "_opt"][fitted]
        g = max(g, float(np.max(np.abs(ref[:, 1] - opt[:, 1]) / ref[:, 1], initial=0.0)))
    assert g == float(G["g"]) and TOL == 4 * g
    sizes = np.concatenate([np.diff(G[name + "_offsets"])[G[name + "_mode"] == 1] for name in BATCHES])
    assert {3, 63, 64, 65, 257, 4096} <= set(sizes.tolist())


@pytest.mark.parametrize("name", BATCHES)
def test_restatement_of_what_the_reference_decides(name):
    values, offsets, mode = G[name + "_values"], G[name + "_offsets"], G[name + "_mode"]
    for s in range(len(mode)):
        data = values[offsets[s]:offsets[s + 1]]
        prep = rs.prepare(data)
        assert prep[0] == ("mean", "fit", "refused")[mode[s]]
        if mode[s] == 0:
            want = G[name + "_rate"][s]
            assert prep[1] == want or (want != want and prep[1] != prep[1])
        elif mode[s] == 1:
            _, x, p0, lower, upper = prep
            assert (np.diff(x) >= 0).all() and np.array_equal(np.sort(data.astype(np.float64)), x)
            ref_p0 = G[name + "_p0"][s]
            assert p0[0] == ref_p0[0] == len(data) and p0[2] == ref_p0[2] == x[0]
            assert abs(p0[1] - ref_p0[1]) <= 1e-6 * ref_p0[1]           # the reference takes the mean in the column's dtype
            assert np.array_equal(lower, G[name + "_lower"][s]) and np.array_equal(upper, G[name + "_upper"][s])
            assert lower == (0.0, x[0], 0.0) and upper == (np.inf, x[-1], np.inf)
            assert abs(rs.cost(x, G[name + "_ref"][s]) - G[name + "_ref_cost"][s]) <= 1e-12 * G[name + "_ref_cost"][s]


def test_signatures():
    from picasso_amd import lib, postprocess
    recorded = json.loads(str(G["signatures"]))
    assert set(recorded) == set(postprocess.KINETIC_PICK_NAMES) | set(lib.KINETICS_NAMES)
    for name, sig in recorded.items():
        ours = inspect.signature(getattr(postprocess if name in postprocess.KINETIC_PICK_NAMES else lib, name))
        theirs = sig[1:sig.rindex(")")]
        want = [(p.split(":")[0].strip(), "=" in p) for p in _split_params(theirs)]
        got = [("*" if p.kind == p.KEYWORD_ONLY and False else n, p.default is not p.empty) for n, p in ours.parameters.items()]
        assert [w for w in want if w[0] != "*"] == got, name
        keyword_only = [n for n, p in ours.parameters.items() if p.kind == p.KEYWORD_ONLY]
        star = [w[0] for w in want].index("*") if ("*", False) in want else None
        assert keyword_only == ([w[0] for w in want[star + 1:]] if star is not None else []), name


def _split_params(text):
    parts, depth, cur = [], 0, ""
    for ch in text:
        depth += ch in "[("
        depth -= ch in "])"
        if ch == "," and depth == 0:
            parts.append(cur)
            cur = ""
        else:
            cur += ch
    return [p for p in (q.strip() for q in parts + [cur]) if p]


def test_install_rebinds_nothing_new():
    from picasso_amd import localize
    src = inspect.getsource(localize.install)
    for name in ("pick_kinetics", "evaluate_picks", "pick_properties", "estimate_kinetic_rate", "fit_cum_exp"):
        assert name not in src


def test_lib_cumulative_exponential():
    from picasso_amd import lib
    x = np.array([0.5, 2.0, 9.0])
    assert np.array_equal(lib.cumulative_exponential(x, 3.0, 2.5, 0.25), rs.model(x, 3.0, 2.5, 0.25))


# ---- wrapper logic that needs no device: picks that come linked, the device calls replaced ----------------------------
@pytest.fixture
def host_backend(monkeypatch, driver):
    from picasso_amd import backend

    class DarkTable:
        def __init__(self, frame, group, last_frame):
            self.args = (frame, group, last_frame)

        def search(self):
            return rs.host_dark_search(*self.args)

    def kinetic_rates(values, offsets):
        fit, info = driver(values, offsets)
        return backend.KineticRates(fit[0], fit[1], fit[2], fit[3], info[0], info[1])

    monkeypatch.setattr(backend, "DarkTable", DarkTable)
    monkeypatch.setattr(backend, "kinetic_rates", kinetic_rates)
    return backend


LINKED = [w for w in WRAPPERS if w.startswith("linked")]


@pytest.mark.parametrize("name", LINKED)
def test_pick_kinetics_regroups_and_drops(host_backend, name):
    from picasso_amd import postprocess
    picks, seen = rs.picks_of(G, name), []
    before = [p.copy() for p in picks]
    length, dark, no_locs, out_locs = postprocess.pick_kinetics(picks, INFO, max_dark_time=3, progress_callback=seen.append)
    assert seen == G[name + "_pk_callbacks"].tolist() == list(range(len(picks))) + [len(picks)]
    assert np.array_equal(no_locs, G[name + "_pk_no_locs"]) and len(no_locs) < len(picks)        # picks were dropped
    rs.assert_table(out_locs, G, name + "_pk_out")
    for got, want in ((length, G[name + "_pk_length"]), (dark, G[name + "_pk_dark"])):
        assert got.dtype == want.dtype and (np.abs(got - want) <= TOL * np.abs(want)).all()
    assert all(a.equals(b) for a, b in zip(picks, before))                  # documented: the caller's tables are not written
    assert bool(G["sort_quirk"])          # observed with the minting pandas: the fitted columns come out ascending per pick
    at = 0
    for n in no_locs:
        v = out_locs["len"].to_numpy()[at:at + n]
        if n > 2 and v.max() != v.min():
            assert (np.diff(v) >= 0).all()
        at += n


@pytest.mark.parametrize("name", LINKED)
def test_single_pick(host_backend, name):
    from picasso_amd import postprocess
    picks = rs.picks_of(G, name)
    kept = 0
    for pick in picks:
        single = postprocess._pick_kinetics_single(pick, INFO, 3)
        if single is None:
            continue
        events, l_, d_ = single
        assert abs(l_ - G[name + "_pk_length"][kept]) <= TOL * G[name + "_pk_length"][kept]
        assert abs(d_ - G[name + "_pk_dark"][kept]) <= TOL * G[name + "_pk_dark"][kept]
        assert len(events) == G[name + "_pk_no_locs"][kept]
        kept += 1
    assert kept == len(G[name + "_pk_no_locs"])


def test_pick_properties_columns(host_backend, monkeypatch):
    from picasso_amd import postprocess
    name = "linked"
    columns, dtypes, values = rs.table_of(G, name + "_pp")
    fake = pd.DataFrame({c: values[c] for c in columns[:columns.index("n_units")] if c != "pick_area_um2"})
    monkeypatch.setattr(postprocess, "groupprops", lambda locs, callback=None: fake.copy())
    props = postprocess.pick_properties(rs.picks_of(G, name), INFO, max_dark_time=3, influx_rate=0.04,
                                        pick_areas=G[name + "_pp_areas"])
    rs.assert_table(props, G, name + "_pp", close=("n_units", "length_cdf", "dark_cdf", "qpaint_idx_cdf"), tol=TOL)


def test_mixed_columns_are_refused(host_backend):
    from picasso_amd import postprocess
    picks = rs.picks_of(G, "linked")
    picks[0] = picks[0].drop(columns=["len"])
    with pytest.raises(ValueError):
        postprocess.pick_kinetics(picks, INFO)
