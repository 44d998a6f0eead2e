"""CPU tier of the fiducial undrift: the restatement (tests/golden/_fiducials_restate.py) against the goldens minted
from the reference, the restated add.reduce against NumPy's, the recorded signatures, the ABI, the refusals, and the
Python layer of ``postprocess.undrift_from_picked`` / ``undrift_from_fiducials`` with ``backend.fiducials_drift`` and
``backend.picks_circle`` replaced by the restatements."""
import inspect
import json
import os
import sys
import warnings

import numpy as np
import pandas as pd
import pytest

from picasso_amd import __version__, _lib, backend, postprocess

import _fiducials_cases as fc

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import _fiducials_restate as fr  # noqa: E402
import _picks_restate as rs  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = fc.goldens()
PICKED, TABLES = fc.picked_cases(), fc.table_cases()
ERRORS = {"IndexError": IndexError, "ValueError": ValueError}


def test_the_cases_are_the_minted_ones():
    assert list(PICKED) == [str(n) for n in G["picked_names"]] and list(TABLES) == [str(n) for n in G["table_names"]]
    assert {str(G[n + "/raises"]) for n in list(PICKED) + list(TABLES) if n + "/raises" in G.files} == set(ERRORS)
    assert sum(n + "/drift" in G.files for n in PICKED) >= 16 and sum(n + "/drift" in G.files for n in TABLES) >= 7


def restated(name):
    info, picks, coordinate = PICKED[name]
    names = [coordinate] if coordinate else ["x", "y"] + (["z"] if all("z" in p for p in picks) else [])
    offsets, frame, cols = fr.csr(picks, names)
    return names, fr.drift(offsets, frame, cols, info[0]["Frames"])


@pytest.mark.parametrize("name", list(PICKED))
def test_restatement_reproduces_the_golden(name):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        if name + "/raises" in G.files:
            with pytest.raises(ERRORS[str(G[name + "/raises"])]):
                restated(name)
            return
        names, got = restated(name)
    assert names == [str(c) for c in G[name + "/columns"]]
    assert fc.same_bits(got, G[name + "/drift"]), name


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_restated_sum_is_numpys(dtype):
    rng = np.random.default_rng(7)
    for n in fc.PICK_LENGTHS + (0, 3 * 8192 + 130):
        v = rng.normal(5, 2, n).astype(dtype)
        got, want = fr.pairwise_reduce(v), np.add.reduce(v)
        assert got.dtype == want.dtype and got.tobytes() == want.tobytes(), n


def test_names_signatures_and_abi():
    recorded = json.loads(str(G["signatures"]))
    assert sorted(recorded) == sorted(postprocess.FIDUCIAL_NAMES)
    for name in postprocess.FIDUCIAL_NAMES:
        assert str(inspect.signature(getattr(postprocess, name))) == recorded[name], name
    L = _lib.load()
    assert L.pmi_version() >= 121
    header = open(os.path.join(ROOT, "include", "picasso_hip.h")).read()
    for name in ("pmi_fiducials_drift_dev", "pmi_fiducials_reduce_dev", "pmi_fiducials_max_cells"):
        assert name in _lib.SYMBOLS and hasattr(L, name) and name in header
    assert backend.fiducials_max_cells() == 1 << 28 and "2^28" in header


# ---- the Python layer over the restatements ---------------------------------------------------------------------
class FakeTable:
    def __init__(self, x_index, y_index, K, L):
        self.n = len(x_index)


@pytest.fixture
def fakes(monkeypatch):
    calls = []

    def drift(offsets, frame, columns, n_frames):
        calls.append((len(offsets) - 1, len(columns)))
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            return fr.drift(offsets, frame, columns, n_frames)

    monkeypatch.setattr(backend, "fiducials_drift", drift)
    monkeypatch.setattr(backend, "BlockTable", FakeTable)
    return calls


@pytest.mark.parametrize("name", list(PICKED))
def test_undrift_from_picked_over_the_restatement(name, fakes):
    info, picks, coordinate = PICKED[name]
    frames = fc.frames_of(picks)

    def run():
        if coordinate:
            return [coordinate], postprocess._undrift_from_picked_coordinate(frames, info, coordinate).reshape(-1, 1)
        df = postprocess.undrift_from_picked(frames, info)
        assert isinstance(df, pd.DataFrame) and isinstance(df.index, pd.RangeIndex)
        return list(df.columns), df.to_numpy()

    if name + "/raises" in G.files:
        with pytest.raises(ERRORS[str(G[name + "/raises"])]):
            run()
        return
    names, got = run()
    assert names == [str(c) for c in G[name + "/columns"]] and fc.same_bits(got, G[name + "/drift"])
    assert fakes == [(len(picks), len(names))]                   # one call for all coordinates


def run_table(name, monkeypatch):
    cols, index, info, picks, pick_size, undrift_z = TABLES[name]

    def circle(table, x, y, *a):          # the restatement's rows are positions in the caller's table: here in the sane one
        offsets, rows = rs.circle(cols, info, picks, pick_size)
        return offsets, np.searchsorted(rs.sane_rows(cols, info), rows)

    monkeypatch.setattr(backend, "picks_circle", circle)
    df = fc.table_frame(cols, index)
    before = df.copy()
    try:
        return df, postprocess.undrift_from_fiducials(df, info, picks, pick_size, undrift_z)
    finally:
        assert df.equals(before)


def assert_table(name, df, result):
    locs, new_info, drift = result
    info = TABLES[name][2]
    assert [str(c) for c in G[name + "/drift_columns"]] == list(drift.columns) and fc.same_bits(drift.to_numpy(), G[name + "/drift"])
    assert list(locs.columns) == [str(c) for c in G[name + "/out_columns"]] and locs is not df
    assert [str(d) for d in locs.dtypes] == [str(d) for d in G[name + "/out_dtypes"]]
    assert locs.index.equals(df.index)
    for c in locs.columns:
        if f"{name}/out_{c}" in G.files:
            assert fc.same_bits(locs[c].to_numpy(), G[f"{name}/out_{c}"]), (name, c)
        else:
            assert locs[c].equals(df[c]), (name, c)
    want = json.loads(str(G[name + "/new_info"]))
    want["Generated by"] = want["Generated by"].format(version=__version__)
    assert new_info[:-1] == info and new_info[-1] == want and len(info) == 1


@pytest.mark.parametrize("name", list(TABLES))
def test_undrift_from_fiducials_over_the_restatements(name, fakes, monkeypatch):
    if name + "/raises" in G.files:
        with pytest.raises(ERRORS[str(G[name + "/raises"])]):
            run_table(name, monkeypatch)
        return
    df, result = run_table(name, monkeypatch)
    assert_table(name, df, result)
    assert len(fakes) == 1


def test_refusals(fakes):
    cols, index, info, picks, pick_size, _ = TABLES["fid_f32"]
    df = fc.table_frame(cols, index)
    with pytest.raises(NotImplementedError, match="find_fiducials"):
        postprocess.undrift_from_fiducials(df, info)
    with pytest.raises(NotImplementedError, match="index_blocks"):
        postprocess.undrift_from_fiducials(df, info, picks, pick_size, index_blocks=(1, 2))
    with pytest.raises(ValueError, match="pick_size"):
        postprocess.undrift_from_fiducials(df, info, picks)
    with pytest.raises(ValueError, match="No picks"):
        postprocess.undrift_from_fiducials(df, info, [], pick_size)
    with pytest.raises(KeyError):
        postprocess.undrift_from_fiducials(df, [{"Frames": 300, "Width": 32, "Height": 32}], picks, pick_size)
    # a coordinate with two dtypes among the picks has no single type to take the means in
    mixed = fc.frames_of(PICKED["z_all"][1][:1] + PICKED["z_all_f64"][1][:1])
    with pytest.raises(TypeError, match="dtypes"):
        postprocess.undrift_from_picked(mixed, PICKED["z_all"][0])
    assert fakes == []


def test_backend_refuses_before_the_device(monkeypatch):
    monkeypatch.setattr(_lib, "require_gpu", lambda: None)
    x = np.zeros(4, np.float32)
    with pytest.raises(ValueError, match="offsets"):
        backend.fiducials_drift([0, 3, 2, 4], np.zeros(4, np.int64), [x], 10)
    with pytest.raises(MemoryError):
        backend.fiducials_drift(np.arange(70001) * 0, np.zeros(0, np.int64), [x[:0]], 1 << 12)
    with pytest.raises(ValueError, match="columns"):
        backend.fiducials_drift([0, 4], np.zeros(4, np.int64), [x] * 4, 10)
