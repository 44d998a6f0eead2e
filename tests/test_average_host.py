"""CPU tier of the particle averaging (picasso_amd/average.py, csrc/average.hip): the exact NumPy oracle
(tests/golden/_average_restate.py) agrees with what the reference recorded (tests/golden/average_cases.npz) wherever
the reference's choice is not a tie, and every departure is one; the header the kernels are compiled from
(csrc/average_core.h), built here with the host compiler (tests/average_host_driver.cpp), gives the oracle's choices and
bits; the host code around the alignment gives the reference's bits and types; the ABI, ``install()`` and the edges that
need no device are checked."""
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

from conftest import GOLDEN, ROOT, golden

sys.path.insert(0, GOLDEN)
import _average_restate as rs  # noqa: E402
import make_goldens_average as mk  # noqa: E402

from picasso_amd import _lib, average, backend  # noqa: E402

G = golden("average_cases")
CASES = [str(c) for c in G["case_names"]]
ORDINARY = [c for c in CASES if c != "ties"]
EDGES = json.loads(str(G["edges"]))
INFO = json.loads(str(G["info"]))
QUICK = ["sites", "odd_n", "even_n", "edges", "single_group", "ties"]      # the cases a CPU walks through in seconds


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def columns(name):
    return {str(c): G[f"{name}/in_{c}"] for c in G[name + "/in_columns"]}


def setup(name):
    cols = columns(name)
    r = G[name + "/r"][()]
    return cols, rs.group_order(cols["group"]), r, 130 / float(G[name + "/dps"]), G[name + "/angles"]


def theirs(name, it, n):
    c = G[f"{name}/it{it}/choice"]
    return np.where(c[:, :1] < 0, -1, np.c_[c[:, 0], c[:, 1] * n + c[:, 2]])


def check_against_record(name, it, choices, x1, y1, order, offsets, value_at):
    """The 10 % rule: every group has the reference's choice, or the reference's choice attains the integer maximum (a
    tie); outside ``ties`` at most 10 % of the groups are excused, and x, y of the others equal the record in bits."""
    n = int(G[f"{name}/it{it}/n_pixel"])
    ref = theirs(name, it, n)
    departs = np.flatnonzero((ref != choices[:, 1:]).any(axis=1))
    for g in departs:
        assert ref[g, 0] >= 0 and value_at(g, ref[g, 0], ref[g, 1]) == choices[g, 0], (name, it, g)
    if name != "ties":
        assert len(departs) <= 0.1 * len(choices), (name, it, departs)
    keep = np.ones(len(x1), bool)
    for g in departs:
        keep[order[offsets[g]:offsets[g + 1]]] = False
    assert same(x1[keep], G[f"{name}/it{it}/x1"][keep]) and same(y1[keep], G[f"{name}/it{it}/y1"][keep]), (name, it)
    return departs


@pytest.fixture(scope="module")
def oracle():
    """name -> per iteration (image, choices, x1, y1) from the recorded state, computed once."""
    out = {}
    for name in QUICK:
        cols, (groups, order, offsets), r, ov, angles = setup(name)
        out[name] = [rs.iteration(G[f"{name}/it{it}/x0"], G[f"{name}/it{it}/y0"], order, offsets, angles, ov, -r, r, check_every=8)
                     for it in range(int(G[name + "/iterations"]))]
    return out


@pytest.mark.parametrize("name", QUICK)
def test_restatement_agrees_with_the_reference(name, oracle):
    cols, (groups, order, offsets), r, ov, angles = setup(name)
    for it, (avg, choices, x1, y1) in enumerate(oracle[name]):
        x0, y0 = G[f"{name}/it{it}/x0"], G[f"{name}/it{it}/y0"]

        def value_at(g, ai, flat):
            index = order[offsets[g]:offsets[g + 1]]
            return rs.correlation(x0[index], y0[index], angles[ai], avg, ov, -r, r).flat[flat]

        departs = check_against_record(name, it, choices, x1, y1, order, offsets, value_at)
        assert same(departs, G[f"{name}/it{it}/departs"])


@pytest.mark.parametrize("n", [1, 2, 5, 28, 33])
def test_fftshift_index_map(n):
    s = (np.arange(n) - n // 2) % n
    assert np.array_equal(np.fft.fftshift(np.arange(n)), s)
    rng = np.random.default_rng(n)
    avg = rng.integers(0, 9, (n, n)).astype(np.int32)
    py, px = rng.integers(0, n, 7).astype(np.int32), rng.integers(0, n, 7).astype(np.int32)
    assert np.array_equal(rs.correlation_gather(py, px, avg), rs.correlation_fft(py, px, avg))


# ---- the header, built for the host -------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("average_host") / "average_host.so")
    subprocess.run([os.environ.get("CXX", "c++"), "-O2", "-std=c++17", "-shared", "-fPIC", "-ffp-contract=off",
                    "-I", os.path.join(ROOT, "picasso_amd", "csrc"), os.path.join(ROOT, "tests", "average_host_driver.cpp"),
                    "-o", out], check=True)
    lib = ctypes.CDLL(out)
    p, i32, f64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_double
    lib.average_host_image.argtypes = [p, p, i32, f64, f64, f64, i32, i32, i32, p]
    lib.average_host_align.argtypes = [p, p, i32, f64, f64, f64, i32, p, p, i32, p, p, p, p]
    return lib


@pytest.mark.parametrize("name", QUICK)
def test_host_build_of_the_core_equals_the_oracle(name, host, oracle):
    cols, (groups, order, offsets), r, ov, angles = setup(name)
    cos = np.array([np.cos(a) for a in angles])
    sin = np.array([np.sin(a) for a in angles])
    for it, (avg, choices, x1, y1) in enumerate(oracle[name]):
        x0, y0 = G[f"{name}/it{it}/x0"], G[f"{name}/it{it}/y0"]
        n, sub_f32, mul_f32 = backend.average_geometry(ov, -r, r)
        assert n == avg.shape[0] and (sub_f32, mul_f32) == ((1, 1) if r.dtype == np.float32 else (0, 0))
        image = np.zeros((n, n), np.int32)
        assert host.average_host_image(_lib.ptr(x0), _lib.ptr(y0), len(x0), float(-r), float(r), ov, n, sub_f32, mul_f32,
                                       _lib.ptr(image)) == 0
        assert same(image, avg)
        for g in range(len(groups)):
            index = order[offsets[g]:offsets[g + 1]]
            xg, yg = np.ascontiguousarray(x0[index]), np.ascontiguousarray(y0[index])
            choice, xo, yo = np.zeros(3, np.int32), np.zeros(len(index), np.float32), np.zeros(len(index), np.float32)
            host.average_host_align(_lib.ptr(xg), _lib.ptr(yg), len(index), float(-r), float(r), ov, n, _lib.ptr(cos),
                                    _lib.ptr(sin), len(angles), _lib.ptr(image), _lib.ptr(choice), _lib.ptr(xo), _lib.ptr(yo))
            assert list(choice) == list(choices[g]), (name, it, g)
            assert same(xo, x1[index]) and same(yo, y1[index]), (name, it, g)


# ---- the host code around the alignment -----------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_com_align_and_the_search_grid_in_bits(name):
    cols = columns(name)
    locs = pd.DataFrame(cols)
    index = average.build_group_index(locs)
    groups = np.unique(cols["group"])
    assert index.shape == (len(groups), len(locs)) and index.dtype == bool
    for i in (0, len(groups) - 1):
        assert np.array_equal(index[i].nonzero()[1], np.flatnonzero(cols["group"] == groups[i]))
    aligned = average.com_align(locs, index)
    assert same(aligned["x"].to_numpy(), G[name + "/com_x"]) and same(aligned["y"].to_numpy(), G[name + "/com_y"])
    assert same(locs["x"].to_numpy(), cols["x"])                      # a copy, as the reference's
    r = 2 * np.sqrt((aligned["x"] ** 2 + aligned["y"] ** 2).mean())
    a_step = np.arcsin(1 / (130 / float(G[name + "/dps"]) * r))
    angles = np.arange(0, 2 * np.pi, a_step)
    assert type(r).__name__ + "/" + type(a_step).__name__ == str(G[name + "/r_type"])
    assert same(np.asarray(r), G[name + "/r"]) and same(np.asarray(a_step), G[name + "/a_step"]) and same(angles, G[name + "/angles"])


def test_prepare_locs_for_save_in_bits():
    name = "sites"
    locs = pd.DataFrame({str(c): G[f"{name}/out_{c}"] for c in G[name + "/columns"]})
    shifted, info = average.prepare_locs_for_save(locs, INFO, {"disp_px_size": float(G[name + "/dps"]), "it": int(G[name + "/iterations"])})
    assert same(shifted["x"].to_numpy(), G[name + "/shifted_x"]) and same(shifted["y"].to_numpy(), G[name + "/shifted_y"])
    want = json.loads(str(G[name + "/shifted_info"]))
    version = json.loads(str(G["versions"]))["picasso"]
    assert want[-1]["Generated by"] == f"Picasso {version} Average"
    want[-1]["Generated by"] = f"Picasso {average.__version__} Average"
    assert info == want and info[:-1] == INFO


def test_compute_xcorr_is_numpy_s():
    rng = np.random.default_rng(3)
    a, b = rng.poisson(1.0, (9, 9)).astype(np.float32), rng.poisson(1.0, (9, 9)).astype(np.float32)
    want = np.fft.fftshift(np.real(np.fft.ifft2(np.fft.fft2(b) * np.conj(np.fft.fft2(a)))))
    assert same(average.compute_xcorr(np.conj(np.fft.fft2(a)), b), want)


def test_signatures_are_the_reference_s():
    want = json.loads(str(G["signatures"]))
    assert set(want) == set(average.AVERAGE_NAMES)
    for name, sig in want.items():
        assert mk.signature(getattr(average, name)) == sig, name


def test_abi_has_the_average_entries():
    lib = _lib.load()
    assert lib.pmi_version() >= 118
    header = open(os.path.join(ROOT, "include", "picasso_hip.h")).read()
    for name in ("pmi_average_limits", "pmi_average_image_dev", "pmi_average_align_dev", "pmi_average_apply_dev"):
        assert name in _lib.SYMBOLS and hasattr(lib, name) and f"int {name}(" in header
    assert backend.average_limits() == (backend.AVERAGE_LDS_BINS, backend.AVERAGE_LIST, backend.AVERAGE_MAX_PIXELS)
    assert backend.AVERAGE_LDS_BINS == int(G["lds_bins"]) == mk.LDS_BINS and backend.AVERAGE_LIST == int(G["list"]) == mk.LIST
    for k in ("LDS_BINS", "LIST", "MAX_PIXELS"):
        assert f"#define PMI_AVERAGE_{k} {getattr(backend, 'AVERAGE_' + k)}\n" in header
    # two workgroups of the LDS path (image, list, reduction) fit the 160 KiB of a CU
    assert 2 * (4 * backend.AVERAGE_LDS_BINS + 4 * backend.AVERAGE_LIST + 4 * 1024) <= 160 * 1024
    assert backend.AVERAGE_MAX_PIXELS < 1 << 15


def test_geometry_and_chunks_are_host_code():
    r32, r64 = np.float32(0.53), np.float64(0.53)
    assert backend.average_geometry(26.0, -r32, r32) == (int(np.ceil(26.0 * (r32 - -r32))), 1, 1)
    assert backend.average_geometry(26.0, -r64, r64) == (int(np.ceil(26.0 * (r64 + r64))), 0, 0)
    assert backend.average_geometry(np.float64(26.0), -r32, r32)[1:] == (1, 0)
    assert backend.average_chunks(5000, 86) == 1 and backend.average_chunks(6, 424) == 53 and backend.average_chunks(1, 5) == 1


def test_install_rebinds_the_names():
    from picasso_amd import localize
    stub = types.SimpleNamespace(average="theirs", average3="theirs", com_align="theirs")
    mods = {k: types.SimpleNamespace() for k in ("picasso_localize", "picasso_gaussmle", "picasso_gausslq", "picasso_zfit",
                                                 "picasso_imageprocess", "picasso_postprocess", "picasso_aim", "picasso_clusterer")}
    localize.install(picasso_render=types.SimpleNamespace(), picasso_average=stub, **mods)
    for name in average.AVERAGE_NAMES:
        assert getattr(stub, name) is getattr(average, name)
    assert stub.average3 == "theirs"
    assert list(inspect.signature(localize.install).parameters)[-1] == "picasso_average"


def test_edges_that_need_no_device(monkeypatch):
    def no_gpu():
        raise AssertionError("the device was asked for")
    monkeypatch.setattr(_lib, "require_gpu", no_gpu)
    base = columns("sites")
    calls = {"empty": lambda: average.average(pd.DataFrame({c: v[:0] for c, v in base.items()}), INFO),
             "no group": lambda: average.average(pd.DataFrame({c: v for c, v in base.items() if c != "group"}), INFO),
             "no Pixelsize": lambda: average.average(pd.DataFrame(base), [{"Width": 64}])}
    for name, call in calls.items():
        want = EDGES[name]
        with pytest.raises((AssertionError, KeyError, ValueError)) as err, np.errstate(all="ignore"):
            call()
        assert [type(err.value).__name__, str(err.value)] == [want["raises"], want["message"]], name
    want = EDGES["iterations=0"]
    cols = columns("edges")
    res = average.average(pd.DataFrame(cols), INFO, iterations=0)
    assert [list(res.columns), [str(d) for d in res.dtypes], len(res)] == [want["returns"], want["dtypes"], want["rows"]]
    assert same(res["x"].to_numpy(), G["zero_x"]) and same(res["y"].to_numpy(), G["zero_y"])
    seen = []
    assert average.average(pd.DataFrame(cols), INFO, abort_callback=lambda: seen.append(1) or True) is None and seen == [1]


def test_cases_hold_the_hard_parts():
    n = {c: int(G[f"{c}/it0/n_pixel"]) for c in CASES}
    assert n["sites"] == 28 and len(G["sites/angles"]) == 86 and int(G["sites/iterations"]) == 3
    assert n["odd_n"] % 2 == 1 and n["even_n"] % 2 == 0
    assert n["global_path"] ** 2 > backend.AVERAGE_LDS_BINS >= max(v for k, v in n.items() if k != "global_path") ** 2
    assert np.bincount(columns("big_group")["group"]).max() > backend.AVERAGE_LIST
    e, r = columns("edges"), float(G["edges/r"])
    assert e["x"].dtype == np.float64 and G["edges/r"].dtype == np.float64 and G["sites/r"].dtype == np.float32
    assert e["group"].min() < 0 and (np.diff(e["group"]) < 0).any() and (np.bincount(e["group"] - e["group"].min()) == 1).any()
    assert G["edges/it0/x0"][int(G["on_t_max"])] == r and G["edges/it0/x0"][int(G["outlier"])] > r
    assert G["edges/it0/x1"][int(G["outlier"])] != G["edges/it0/x0"][int(G["outlier"])]
    assert len(np.unique(columns("single_group")["group"])) == 1
    assert sum(int(G[f"ties/it{it}/multi"].sum()) for it in range(int(G["ties/iterations"]))) >= 10
    assert bool(G["sites/exact"]) and set(json.loads(str(G["versions"]))) == {"pandas", "numpy", "scipy", "picasso"}
    for name in ORDINARY:
        for it in range(int(G[name + "/iterations"])):
            assert len(G[f"{name}/it{it}/departs"]) <= 0.1 * len(G[f"{name}/it{it}/choice"]), (name, it)


def test_goldens_regenerate():
    """The committed average_cases.npz is what make_goldens_average.py mints from the reference tree today (the two
    quickest cases are walked through again)."""
    if not os.path.isfile(mk.AVERAGE_PY):
        pytest.skip("reference tree not present")
    ref = mk.load_reference()
    cases = mk.make_cases(ref, int(G["lds_bins"]))
    assert list(cases) == CASES
    for name, case in cases.items():
        assert all(same(v, G[f"{name}/in_{c}"]) for c, v in case["cols"].items()), name
    for name in ("odd_n", "single_group"):
        case, log = cases[name], {}
        final = mk.ref_average(ref, pd.DataFrame(case["cols"]), INFO, display_pixel_size=case["dps"],
                               iterations=case["iterations"], log=log)
        assert all(same(final[c].to_numpy(), G[f"{name}/out_{c}"]) for c in final.columns), name
        for it, rec in enumerate(log["its"]):
            assert same(rec["choice"], G[f"{name}/it{it}/choice"]) and same(rec["x1"], G[f"{name}/it{it}/x1"])
    assert ref["seen"].max_err < 0.5
