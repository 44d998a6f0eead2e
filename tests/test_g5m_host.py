"""CPU tier of G5M (picasso_amd/g5m.py, csrc/g5m.hip): the NumPy oracle (tests/golden/_g5m_restate.py) agrees with what the
reference's own functions recorded (tests/golden/g5m_cases.npz) — every choice equal, every float within the tolerance the
record measured on the reference itself; the header the kernels are compiled from (csrc/g5m_core.h), built here with the
host compiler (tests/g5m_host_driver.cpp, sums added in order), agrees the same way, and runs once over all cases under
the address and undefined-behaviour sanitizers as a stand-alone program; the host side of ``g5m()`` is checked with the
oracle's models in place of the device's."""
import ctypes
import inspect
import json
import os
import subprocess
import sys
import types

import numpy as np
import pandas as pd
import pytest

from conftest import GOLDEN, ROOT
from _g5m_cases import CASES, FIXED, G, INFO, check_model, check_tables, close, columns, frame_of, kwargs

sys.path.insert(0, GOLDEN)
import _g5m_restate as rs  # noqa: E402
import make_goldens_g5m as mk  # noqa: E402

from picasso_amd import __version__, _lib, backend, g5m, localize  # noqa: E402

CSRC = os.path.join(ROOT, "picasso_amd", "csrc")
DRIVER = os.path.join(ROOT, "tests", "g5m_host_driver.cpp")


def settings(name):
    kw = kwargs(name)
    return dict(min_locs=10, handle=kw.get("loc_prec_handle", "local"), bounds=kw.get("sigma_bounds", (0.8, 1.5)),
                max_rounds=kw.get("max_rounds_without_best_bic", 3), max_locs=kw.get("max_locs_per_cluster", np.inf))


def as_fitted(m):
    return None if m is None else (m["weights_"], m["means_"], m["covariances_"], m["precisions_cholesky_"], m["valid_idx"],
                                   m["n_locs"], m["converged"])


@pytest.fixture(scope="module")
def oracle():
    """case -> the oracle's model per fitted cluster (np.unique order), computed once."""
    out = {}
    for name in CASES:
        s = settings(name)
        out[name] = list(rs.models_of(frame_of(name), s["min_locs"], s["bounds"], s["handle"], s["max_rounds"], s["max_locs"]).values())
    return out


@pytest.mark.parametrize("name", CASES)
def test_oracle_agrees_with_the_record(name, oracle):
    assert len(oracle[name]) == int(G[name + "/n_models"])
    for i, m in enumerate(oracle[name]):
        check_model(as_fitted(m), name, i)
        if m is not None:
            close(m["bic"], G[f"{name}/model{i}/bic"], "bic")


@pytest.mark.parametrize("name", FIXED)
def test_oracle_fixed_fit_agrees_with_the_record(name):
    cols = columns(name)
    lp = frame_of(name)[["lpx", "lpy"]].mean(axis=1).to_numpy()
    check_model(as_fitted(rs.fit_fixed(np.stack([cols["x"], cols["y"]], axis=1), lp, int(G[name + "/K"]), 10, (0.8, 1.5))), name, 0)


# ---- the header, built for the host -------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("g5m_host") / "g5m_host.so")
    subprocess.run([os.environ.get("CXX", "c++"), "-O2", "-std=c++17", "-shared", "-fPIC", "-ffp-contract=off", "-pthread", "-I", CSRC,
                    DRIVER, "-o", out], check=True)
    return ctypes.CDLL(out)


def host_run(host, locs, s, k_fixed=0):
    """(models, assigned, rows, offsets, ids) of a table through the host build of the core."""
    ids, rows, offsets = g5m.cluster_rows(locs, s["min_locs"], s["max_locs"])
    part = locs.iloc[rows]
    sizes = np.diff(offsets)
    caps = np.minimum(backend.G5M_MAX_K, sizes // s["min_locs"]) if not k_fixed else np.full(len(sizes), k_fixed, np.int64)
    models = backend._g5m_empty(caps)
    table, first, uniform = backend.g5m_table(sizes, caps)
    lp_mean = part[["lpx", "lpy"]].mean(axis=1).to_numpy().astype(np.float64)
    lp = lp_mean if s["handle"] == "local" else np.ones(len(part))
    x, y = (np.ascontiguousarray(part[c].to_numpy(), np.float64) for c in ("x", "y"))
    p, i64, f64 = _lib.ptr, ctypes.c_int64, ctypes.c_double
    total = int(caps.sum())
    host.g5m_host_fit(p(x), p(y), p(lp), p(offsets), i64(len(sizes)), p(table), p(first), p(uniform), None, k_fixed, s["min_locs"],
                      f64(s["bounds"][0]), f64(s["bounds"][1]), s["max_rounds"], backend.G5M_LP_ABS if s["handle"] == "abs" else 0,
                      p(models.model), p(models.imodel), i64(total), p(models.info), p(models.bic), 2)
    frame = part["frame"].to_numpy().astype(np.float64)
    extra = [c for c in part.columns if c not in g5m.IGNORE_COLUMNS]
    cols = np.ascontiguousarray(np.stack([part[c].to_numpy().astype(np.float64) for c in extra])) if extra else None
    out = backend.G5MAssigned(np.zeros(len(x), np.int32), np.zeros(len(x)), np.zeros((total, 7)), np.zeros(total, np.int32),
                              np.zeros(len(sizes)), np.zeros((len(extra), total)), [], [])
    tab2 = np.ascontiguousarray(np.stack([models.start, np.zeros(len(sizes), np.int64)], axis=1))
    host.g5m_host_assign(p(x), p(y), p(lp_mean), p(frame), p(offsets), i64(len(sizes)), p(tab2), p(models.model), p(models.imodel), i64(total),
                         p(models.info), p(cols), len(extra), backend.G5M_QUAD_F32 | backend.G5M_FRAME_U32, p(out.label),
                         p(out.log_likelihood), p(out.stats), p(out.n_events), p(out.group_ll), p(out.col_means) if extra else None,
                         None, None, 2)
    return models, out, rows, offsets, ids


@pytest.mark.parametrize("name", CASES)
def test_host_build_of_the_core_agrees_with_the_record_and_the_oracle(name, host, oracle, monkeypatch):
    locs, s = frame_of(name), settings(name)
    models, assigned, rows, offsets, ids = host_run(host, locs, s)
    assert len(ids) == len(oracle[name])
    for i, m in enumerate(oracle[name]):
        check_model(models.of(i), name, i)
        if m is not None:
            close(models.bic[i], G[f"{name}/model{i}/bic"], "bic")
            assert list(models.of(i)[4]) == list(m["valid_idx"]) and len(models.of(i)[0]) == m["K"]
    # ... and the tables g5m() builds from what the core computed
    monkeypatch.setattr(g5m, "_fit", lambda *a, **k: (models, assigned))
    check_tables(name, *g5m.g5m(locs, INFO, callback_parent=None, **kwargs(name)), __version__)


@pytest.mark.parametrize("name", FIXED)
def test_host_build_fixed_fit(name, host):
    models = host_run(host, frame_of(name), dict(min_locs=10, handle="local", bounds=(0.8, 1.5), max_rounds=0, max_locs=np.inf),
                      k_fixed=int(G[name + "/K"]))[0]
    check_model(models.of(0), name, 0)


def means_init_inputs():
    """Two clusters of the ``two_apart`` table fitted with two components from given means, another pair per cluster."""
    cols = columns("two_apart")
    offsets = np.concatenate([[0], np.cumsum(np.bincount(cols["group"]))]).astype(np.int64)
    x, y = cols["x"].astype(np.float64), cols["y"].astype(np.float64)
    lp = frame_of("two_apart")[["lpx", "lpy"]].mean(axis=1).to_numpy().astype(np.float64)
    means_init = np.array([[[5.02, 5.01], [5.28, 4.99]], [[8.9, 9.0], [9.1, 9.05]]])
    return x, y, lp, offsets, means_init


def check_means_init(models):
    """Against the oracle started from the same means: choices equal, floats within the record's tolerance."""
    x, y, lp, offsets, means_init = means_init_inputs()
    for c in range(2):
        s = slice(offsets[c], offsets[c + 1])
        want = rs.fit_fixed(np.stack([x[s], y[s]], axis=1), lp[s], 2, 10, (0.8, 1.5), means_init=means_init[c])
        got = models.of(c)
        assert (want is None) == (got is None), c
        if want is None:
            continue
        w, m, cov, pc, valid, n_locs, converged = got
        assert list(valid) == list(want["valid_idx"]) and list(n_locs) == list(want["n_locs"]) and converged == want["converged"], c
        close(w, want["weights_"], "weights"), close(m, want["means_"], "means")
        close(cov, want["covariances_"], "covariances"), close(pc, want["precisions_cholesky_"], "precisions_cholesky")
    assert models.of(0) is not None


def test_host_build_fixed_fit_from_given_means(host):
    x, y, lp, offsets, means_init = means_init_inputs()
    caps = np.full(2, 2, np.int64)
    models = backend._g5m_empty(caps)
    table, first, uniform = backend.g5m_table(np.diff(offsets), caps)
    p, i64, f64 = _lib.ptr, ctypes.c_int64, ctypes.c_double
    host.g5m_host_fit(p(x), p(y), p(lp), p(offsets), i64(2), p(table), p(first), p(uniform), p(means_init), 2, 10, f64(0.8), f64(1.5), 0, 0,
                      p(models.model), p(models.imodel), i64(4), p(models.info), p(models.bic), 1)
    check_means_init(models)


def test_the_headers_log_is_within_one_ulp_of_numpys(host):
    xs = np.concatenate([np.random.default_rng(0).uniform(1e-300, 1e300, 1000), np.random.default_rng(1).uniform(0.5, 2, 100000),
                         10.0 ** np.random.default_rng(2).uniform(-30, 30, 100000), [1.0, 5e-324, 2.2250738585072014e-308, 0.1, 59.0]])
    out = np.zeros_like(xs)
    host.g5m_host_log(_lib.ptr(xs), ctypes.c_int64(len(xs)), _lib.ptr(out))
    ref = np.log(xs)
    assert out[len(xs) - 5] == 0.0 and np.all(np.abs(out - ref) <= np.spacing(np.abs(ref)))


def test_host_build_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "g5m_host_driver")
    subprocess.run([os.environ.get("CXX", "c++"), "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-pthread", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-DG5M_HOST_MAIN", "-I", CSRC, DRIVER, "-o", exe], check=True)
    for name in CASES + FIXED:
        locs = frame_of(name)
        fixed = int(G[name + "/K"]) if name in FIXED else 0
        s = settings(name) if name in CASES else dict(min_locs=10, handle="local", bounds=(0.8, 1.5), max_rounds=0, max_locs=np.inf)
        ids, rows, offsets = g5m.cluster_rows(locs, 10, s["max_locs"])
        part = locs.iloc[rows]
        sizes = np.diff(offsets)
        caps = np.full(len(sizes), fixed, np.int64) if fixed else np.minimum(100, sizes // 10)
        table, first, uniform = backend.g5m_table(sizes, caps)
        first = np.concatenate([first, np.zeros(len(first) % 2, np.int32)])
        extra = [c for c in part.columns if c not in g5m.IGNORE_COLUMNS]
        flags = (backend.G5M_LP_ABS if s["handle"] == "abs" else 0) | backend.G5M_QUAD_F32 | backend.G5M_FRAME_U32
        lp = part[["lpx", "lpy"]].mean(axis=1).to_numpy().astype(np.float64)
        path = tmp_path / (name + ".bin")
        with open(path, "wb") as f:
            f.write(np.array([len(sizes), len(part), caps.sum(), len(first), len(uniform), len(extra), 10, s["max_rounds"], flags, fixed], np.int64).tobytes())
            f.write(np.array(s["bounds"], np.float64).tobytes())
            for a in (offsets, table, first, uniform, *(part[c].to_numpy().astype(np.float64) for c in ("x", "y")), lp,
                      part["frame"].to_numpy().astype(np.float64), *(part[c].to_numpy().astype(np.float64) for c in extra)):
                f.write(np.ascontiguousarray(a).tobytes())
        done = subprocess.run([exe, str(path)], capture_output=True, text=True)
        assert done.returncode == 0 and done.stderr == "" and done.stdout.startswith(f"clusters {len(sizes)} "), (name, done.stderr[-2000:])


# ---- the host side ------------------------------------------------------------------------------------------------------------
def oracle_fit(name, oracle):
    """What fit_clusters returns, from the oracle's models and the oracle's own conversion."""
    def fit(locs, rows, offsets, **kw):
        part = locs.iloc[rows]
        sizes = np.diff(offsets)
        caps = np.minimum(100, sizes // 10)
        models = backend._g5m_empty(caps)
        total = int(caps.sum())
        extra = [c for c in part.columns if c not in g5m.IGNORE_COLUMNS]
        out = backend.G5MAssigned(np.zeros(len(part), np.int32), np.zeros(len(part)), np.zeros((total, 7)), np.zeros(total, np.int32),
                                  np.zeros(len(sizes)), np.zeros((len(extra), total)), [], [])
        for c, m in enumerate(oracle[name]):
            if m is None:
                continue
            K, nv, s0 = m["K"], len(m["valid_idx"]), int(models.start[c])
            models.model[:, s0:s0 + K] = [m["weights_"], m["means_"][:, 0], m["means_"][:, 1], m["covariances_"], m["precisions_cholesky_"]]
            models.imodel[1, s0:s0 + K] = -1
            models.imodel[1, s0:s0 + nv], models.imodel[0, s0:s0 + nv] = m["valid_idx"], m["n_locs"]
            models.info[c] = [K, nv, m["converged"], K]
            if nv == 0:
                continue
            rows_c = slice(int(offsets[c]), int(offsets[c + 1]))
            centers, cl = rs.convert(m, part.iloc[rows_c], 130)
            # the float64 values behind the float32 columns are the oracle's own: recompute what the kernel hands over
            v = m["valid_idx"]
            X = cl[["x", "y"]].to_numpy()
            lprob = rs.log_prob(X, m["means_"][v], m["precisions_cholesky_"][v], True) + np.log(m["weights_"][v])
            wlp = rs.log_prob(X, m["means_"], m["precisions_cholesky_"], True) + np.log(m["weights_"])
            resp = np.exp((wlp - rs.logsumexp(wlp)[:, None])[:, v])
            rsum = resp.sum(0)
            fr = cl["frame"].to_numpy().reshape(-1, 1)
            frame = (resp * fr).sum(0) / rsum
            lpm = cl[["lpx", "lpy"]].mean(axis=1).to_numpy()
            mol = (resp * lprob).sum(0) / rsum
            w, cov = m["weights_"][v], m["covariances_"][v]
            from scipy.special import erf
            pv = 0.5 * (1 + erf((mol - (np.log(w / (2 * np.pi * cov)) - 1)) / (np.sqrt(2 * 0.5 / (len(X) * w)) * np.sqrt(2))))
            out.stats[s0:s0 + nv] = np.stack([frame, np.sqrt((resp * (fr - frame) ** 2).sum(0) / ((len(X) - 1) * rsum / len(X))), mol, pv,
                                              (resp * lpm.reshape(-1, 1)).sum(0) / rsum, rsum,
                                              centers["log_likelihood_mean"]], axis=1)
            out.n_events[s0:s0 + nv] = centers["n_events"]
            out.group_ll[c] = np.mean(rs.logsumexp(lprob))
            for i, col in enumerate(extra):
                out.col_means[i, s0:s0 + nv] = centers[f"{col}_mean"]
            out.label[rows_c], out.log_likelihood[rows_c] = cl["group"], cl["log_likelihood"]
        return models, out
    return fit


@pytest.mark.parametrize("name", CASES)
def test_host_side_of_g5m_with_the_oracles_models(name, oracle, monkeypatch):
    def no_gpu():
        raise AssertionError("the device was asked for")
    monkeypatch.setattr(_lib, "require_gpu", no_gpu)
    monkeypatch.setattr(g5m, "_fit", oracle_fit(name, oracle))
    check_tables(name, *g5m.g5m(frame_of(name), INFO, callback_parent=None, **kwargs(name)), __version__)


def test_error_texts_and_what_is_not_built():
    locs = frame_of("two_apart")
    with pytest.raises(AssertionError, match="loc_prec_handle must be 'local' or 'abs'."):
        g5m.g5m(locs, INFO, loc_prec_handle="global")
    with pytest.raises(AssertionError, match="sigma_bounds must be a tuple of two values."):
        g5m.g5m(locs, INFO, sigma_bounds=(1, 2, 3))
    with pytest.raises(AssertionError, match="must not be larger than"):
        g5m.g5m(locs, INFO, sigma_bounds=(2, 1))
    with pytest.raises(AssertionError, match="Localizations must be grouped. Use DBSCAN or similar."):
        g5m.g5m(locs.drop(columns="group"), INFO)
    with pytest.raises(ValueError, match="Camera pixel size must be provided in info."):
        g5m.g5m(locs, [{"Frames": 10}])
    with pytest.raises(ValueError, match="Calibration dictionary must be provided for 3D data."):
        g5m.g5m(locs.assign(z=0.0), INFO)
    with pytest.raises(NotImplementedError, match="3-D path"):
        g5m.g5m(locs.assign(z=0.0), INFO, calibration={"X Coefficients": [], "Y Coefficients": [], "Magnification factor": 0.79})
    with pytest.raises(NotImplementedError, match="bootstrap_check=True"):
        g5m.g5m(locs, INFO, bootstrap_check=True)
    with pytest.raises(NotImplementedError, match="G5M_2D.sample"):
        g5m.G5M_2D(2, 10, (0.8, 1.5)).sample()
    want = json.loads(str(G["signatures"]))
    assert mk.signature(g5m.g5m) == want["g5m"] and mk.signature(g5m.G5M_2D.__init__) == want["G5M_2D"]
    assert mk.signature(g5m.G5M_2D.fit) == want["fit"]
    for k in ("MIN_LOCS", "MAX_ROUNDS_WITHOUT_BEST_BIC", "MIN_SIGMA_FACTOR", "MAX_SIGMA_FACTOR", "N_TASKS", "N_COMPONENTS_MAX"):
        assert getattr(g5m, k) == {"MIN_LOCS": 10, "MAX_ROUNDS_WITHOUT_BEST_BIC": 3, "MIN_SIGMA_FACTOR": 0.8, "MAX_SIGMA_FACTOR": 1.5,
                                   "N_TASKS": 500, "N_COMPONENTS_MAX": 100}[k]
    for member in ("fit", "bic", "predict", "score_samples", "estimate_log_prob", "estimate_weighted_log_prob", "n_parameters", "means",
                   "weights", "covariances", "precisions_cholesky"):
        assert hasattr(g5m.G5M_2D, member)
    model = g5m.G5M_2D(3, 10, (0.8, 1.5))
    assert list(model.valid_idx) == [0, 1, 2] and list(model.n_locs) == [0, 0, 0] and model.converged is False and model.n_init == 3


@pytest.mark.parametrize("n,seeds,K", [(20, 3, 2), (57, 9, 9), (300, 5, 30)])
def test_draw_table_is_randomstate_call_by_call(n, seeds, K):
    first, uniform = backend.g5m_draws(n, seeds, backend.g5m_draws_needed(K))
    for ii in range(seeds):
        np.random.seed(42 + ii)
        assert first[ii] == np.random.choice(n)
        assert all(uniform[ii, j] == np.random.uniform() for j in range(uniform.shape[1]))
    # every K reads a prefix: the oracle's own kmeans++ sees the same stream
    log = []
    rs.kmeanspp(np.random.default_rng(n).normal(size=(n, 2)), K, 42, log)
    assert log[0][0] == first[0] and np.array_equal(log[0][1], uniform[0, :backend.g5m_draws_needed(K)])
    assert [backend.g5m_local_trials(k) for k in (1, 2, 3, 7, 8, 20, 21, 54, 55, 100)] == [2, 2, 3, 3, 4, 4, 5, 5, 6, 6]


def test_abi_has_the_g5m_entries():
    lib = _lib.load()
    assert lib.pmi_version() >= 126
    header = open(os.path.join(ROOT, "include", "picasso_hip.h")).read()
    for name in ("pmi_g5m_limits", "pmi_g5m_fit", "pmi_g5m_fit_dev", "pmi_g5m_fit_fixed", "pmi_g5m_fit_fixed_dev", "pmi_g5m_assign",
                 "pmi_g5m_assign_dev"):
        assert name in _lib.SYMBOLS and hasattr(lib, name) and f"int {name}(" in header
    assert backend.g5m_limits()[:2] == (backend.G5M_LDS_RESP, backend.G5M_MAX_K) and backend.G5M_LDS_RESP == int(G["lds_resp"]) == mk.LDS_RESP
    assert f"#define PMI_G5M_LDS_RESP {backend.G5M_LDS_RESP}\n" in header and f"#define PMI_G5M_MAX_K {backend.G5M_MAX_K}\n" in header
    # three workgroups of the fit (responsibilities, 8 KiB of parameters) fit the 160 KiB of a CU
    assert 3 * (8 * backend.G5M_LDS_RESP + 8 * 1024) <= 160 * 1024


def test_install_rebinds_the_names():
    stub = types.SimpleNamespace(g5m="theirs", G5M_2D="theirs", G5M_3D="theirs")
    mods = {k: types.SimpleNamespace() for k in ("picasso_localize", "picasso_gaussmle", "picasso_gausslq", "picasso_zfit",
                                                 "picasso_imageprocess", "picasso_postprocess", "picasso_aim", "picasso_clusterer")}
    localize.install(picasso_render=types.SimpleNamespace(), picasso_g5m=stub, **mods)
    assert stub.g5m is g5m.g5m and stub.G5M_2D is g5m.G5M_2D and stub.G5M_3D == "theirs"
    p = inspect.signature(localize.install).parameters["picasso_g5m"]
    assert p.default is None and p.kind is inspect.Parameter.KEYWORD_ONLY


def test_cases_hold_the_hard_parts():
    sizes = np.bincount(columns("sizes_9_10_19_20")["group"])
    assert list(sizes) == [9, 10, 19, 20] and int(G["sizes_9_10_19_20/n_models"]) == 3
    assert [int(G[f"two_apart/model{i}/K"]) for i in range(2)] == [2, 1] and int(G["two_within_sigma/model0/K"]) == 1
    assert len(columns("rows_300")["x"]) == 300 > backend.g5m_limits()[2]
    assert int(G["cov_low_local/model1/K"]) > 1 and json_kwargs("cov_bounds_abs")["loc_prec_handle"] == "abs"
    assert int(G["max_locs/n_models"]) == 2 and list(np.unique(G["max_locs/locs/group_input"])) == [0, 2]
    assert "photons_mean" in [str(c) for c in G["photons/centers_columns"]]
    assert bool(G["filtered/found"]) and len(G["filtered/centers/x"]) == 0 and not bool(G["none_valid/found"])
    assert float(G["tolerance/weights"]) > 0 and float(G["tolerance/x"]) == 0
    # the satellite's chosen model drops a component below min_locs that is not its last: valid_idx is no prefix
    K, valid = int(G["satellite/model0/K"]), list(G["satellite/model0/valid_idx"])
    assert len(valid) < K and valid != list(range(len(valid))) and len(G["satellite/centers/x"]) == len(valid)
    assert list(G["satellite/model0/n_locs"]) == list(G["satellite/centers/n_locs"]) and min(G["satellite/model0/n_locs"]) >= 10


def json_kwargs(name):
    return kwargs(name)


def test_goldens_regenerate():
    """The committed g5m_cases.npz is what make_goldens_g5m.py mints from the reference tree today (two quick cases)."""
    if not os.path.isfile(mk.G5M_PY):
        pytest.skip("reference tree not present")
    cases, fixed = mk.make_cases()
    assert list(cases) == CASES and list(fixed) == FIXED
    ref = mk.load_reference()
    for name in ("two_apart", "none_valid"):
        cols, kw = cases[name]
        assert all(np.array_equal(v, G[f"{name}/in_{c}"]) for c, v in cols.items())
        run = mk.run_table(ref, cols, dict(kw))
        for k, v in run.items():
            assert np.array_equal(np.asarray(v), G[f"{name}/{k}"]), (name, k)
