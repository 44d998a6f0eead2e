"""GPU tier of the particle averaging (csrc/average.hip under picasso_amd/average.py).  For every case and iteration of
tests/golden/average_cases.npz, started from the state the reference recorded, the device's average image, choices and
float32 coordinates equal the exact oracle's (tests/golden/_average_restate.py) in every bit, on the LDS path, on the
global path and with the angle list cut into chunks; against the reference's record every group has the same choice or
the reference's choice attains the integer maximum (a tie), the excused groups staying within 10 % outside ``ties``.
Where the reference never departed, the whole ``average()`` call equals its final table in bits."""
import json
import sys

import numpy as np
import pandas as pd
import pytest

from conftest import GOLDEN, golden

sys.path.insert(0, GOLDEN)
import _average_restate as rs  # noqa: E402

from picasso_amd import average, backend  # noqa: E402

pytestmark = pytest.mark.gpu

G = golden("average_cases")
CASES = [str(c) for c in G["case_names"]]
INFO = json.loads(str(G["info"]))
_ORACLE = {}


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def columns(name):
    return {str(c): G[f"{name}/in_{c}"] for c in G[name + "/in_columns"]}


def setup(name):
    cols = columns(name)
    return cols, rs.group_order(cols["group"]), G[name + "/r"][()], 130 / float(G[name + "/dps"]), G[name + "/angles"]


def oracle(name):
    """Per iteration (image, choices, x1, y1) from the recorded state; computed once and shared."""
    if name not in _ORACLE:
        cols, (groups, order, offsets), r, ov, angles = setup(name)
        _ORACLE[name] = [rs.iteration(G[f"{name}/it{it}/x0"], G[f"{name}/it{it}/y0"], order, offsets, angles, ov, -r, r,
                                      check_every=64) for it in range(int(G[name + "/iterations"]))]
    return _ORACLE[name]


def run(name, it, **how):
    cols, (groups, order, offsets), r, ov, angles = setup(name)
    aligner = backend.AverageAligner(cols["group"], angles)
    assert same(aligner.groups.unique, groups.astype(np.int64)) and same(aligner.groups.offsets.astype(np.int64), offsets)
    return aligner.iteration(G[f"{name}/it{it}/x0"], G[f"{name}/it{it}/y0"], ov, -r, r, **how)


@pytest.mark.parametrize("name", CASES)
def test_device_equals_the_oracle_and_the_record(name):
    cols, (groups, order, offsets), r, ov, angles = setup(name)
    for it, (avg, choices, x1, y1) in enumerate(oracle(name)):
        step = run(name, it)
        n = avg.shape[0]
        assert (n * n > backend.AVERAGE_LDS_BINS) == (name == "global_path")
        assert same(step["image"], avg)
        assert same(step["choice"].astype(np.int64), choices), (name, it, np.flatnonzero((step["choice"] != choices).any(axis=1)))
        assert same(step["x"], x1) and same(step["y"], y1), (name, it)
        # the reference's record: the same choice, or a tie
        c = G[f"{name}/it{it}/choice"]
        ref = np.where(c[:, :1] < 0, -1, np.c_[c[:, 0], c[:, 1] * n + c[:, 2]])
        departs = np.flatnonzero((ref != step["choice"][:, 1:]).any(axis=1))
        x0, y0 = G[f"{name}/it{it}/x0"], G[f"{name}/it{it}/y0"]
        keep = np.ones(len(x0), bool)
        for g in departs:
            index = order[offsets[g]:offsets[g + 1]]
            value = rs.correlation(x0[index], y0[index], angles[ref[g, 0]], avg, ov, -r, r, both=False).flat[ref[g, 1]]
            assert ref[g, 0] >= 0 and value == step["choice"][g, 0], (name, it, g)
            keep[index] = False
        if name != "ties":
            assert len(departs) <= 0.1 * len(groups), (name, it, departs)
        assert same(step["x"][keep], G[f"{name}/it{it}/x1"][keep]) and same(step["y"][keep], G[f"{name}/it{it}/y1"][keep])


@pytest.mark.parametrize("name", ["sites", "odd_n", "even_n", "big_group", "edges", "ties"])
def test_global_path_and_chunks_give_the_same_integers(name):
    avg, choices, x1, y1 = oracle(name)[0]
    for how in ({"force_global": True}, {"chunks": 5}, {"force_global": True, "chunks": len(G[name + "/angles"]) // 8}):
        step = run(name, 0, **how)
        assert same(step["image"], avg) and same(step["choice"].astype(np.int64), choices), (name, how)
        assert same(step["x"], x1) and same(step["y"], y1), (name, how)


def test_global_path_case_in_chunks_of_its_own():
    step = run("global_path", 0)
    avg, choices, x1, y1 = oracle("global_path")[0]
    assert step["chunks"] > 1 and same(step["choice"].astype(np.int64), choices)
    step = run("global_path", 0, chunks=1)
    assert same(step["choice"].astype(np.int64), choices) and same(step["x"], x1) and same(step["y"], y1)


@pytest.mark.parametrize("name", [c for c in CASES if bool(G[c + "/exact"])])
def test_average_equals_the_reference_s_final_table(name):
    cols = columns(name)
    dps, iterations = float(G[name + "/dps"]), int(G[name + "/iterations"])
    seen = []
    res = average.average(pd.DataFrame(cols), INFO, display_pixel_size=dps, iterations=iterations,
                          progress_callback=lambda *a: seen.append((a[0], a[1], a[2]["x"].to_numpy().copy(),
                                                                    a[2]["y"].to_numpy().copy(), a[3], a[4])))
    assert list(res.columns) == [str(c) for c in G[name + "/columns"]]
    for c in res.columns:
        assert same(res[c].to_numpy(), G[f"{name}/out_{c}"]), (name, c)
    n_groups = len(np.unique(cols["group"]))
    assert len(seen) == iterations
    for it, (i, total, x, y, done, of) in enumerate(seen):
        assert (i, total, done, of) == (it + 1, iterations, n_groups, n_groups)
        assert same(x, G[f"{name}/it{it}/cb_x"]) and same(y, G[f"{name}/it{it}/cb_y"])
    shifted, info = average.average(pd.DataFrame(cols), INFO, display_pixel_size=dps, iterations=iterations,
                                    return_shifted_locs=True)
    assert same(shifted["x"].to_numpy(), G[name + "/shifted_x"]) and same(shifted["y"].to_numpy(), G[name + "/shifted_y"])
    want = json.loads(str(G[name + "/shifted_info"]))
    want[-1]["Generated by"] = f"Picasso {average.__version__} Average"
    assert info == want


def test_abort_returns_none_and_console_is_quiet():
    cols = columns("single_group")
    calls = []
    assert average.average(pd.DataFrame(cols), INFO, iterations=2,
                           abort_callback=lambda: calls.append(1) or len(calls) > 1) is None
    assert len(calls) == 2
    res = average.average(pd.DataFrame(cols), INFO, iterations=1, progress_callback="console")
    assert same(res["x"].to_numpy(), G["single_group/out_x"])


def test_overflow_is_refused_before_the_align_launch():
    cols, (groups, order, offsets), r, ov, angles = setup("single_group")
    aligner = backend.AverageAligner(cols["group"], angles)
    aligner.max_group = 2 ** 31
    with pytest.raises(ValueError, match="32 bits"):
        aligner.iteration(G["single_group/it0/x0"], G["single_group/it0/y0"], ov, -r, r)
