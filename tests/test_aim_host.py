"""CPU tier: AIM undrift (picasso_amd/aim.py) without a device.

The test-side restatement (tests/golden/_aim_restate.py) reproduces every recorded roi_cc of the golden cases, which
pins the key arithmetic (float32 round 1, float64 round 2, the mixed z pass, int32 wrap, the x86 cast) without a GPU;
the host peak helper, install(), the argument checks and the no-device error are checked here as well."""
import json
import os
import sys
import types

import numpy as np
import pandas as pd
import pytest

from conftest import GOLDEN, golden

sys.path.insert(0, GOLDEN)
import _aim_restate as rs  # noqa: E402

from picasso_amd import _lib, aim, localize  # noqa: E402

CASES = [str(c) for c in golden("aim_cases")["case_names"]]


@pytest.fixture(scope="module")
def g():
    return golden("aim_cases")


@pytest.mark.parametrize("name", CASES)
def test_restatement_reproduces_every_golden_roi_cc(g, name):
    n = 0
    for tag, s, roi, peak, mode, ref, tgt, rel, d, W, H, sh in rs.golden_rounds(g, name):
        ref_k = rs.keys(mode, *ref, (0, 0, 0), d, W, H)
        tgt_k = rs.keys(mode, *tgt, rel, d, W, H)
        got = rs.roi_cc(ref_k, tgt_k, sh)
        assert np.array_equal(got, roi), (name, tag, s)
        n += 1
    assert n == len(g[name + "/rec_seg"]) and n > 0


@pytest.mark.parametrize("name", CASES)
def test_host_peak_bit_equal(g, name):
    p = name + "/"
    starts = np.concatenate(([0], np.cumsum(g[p + "rec_len"])))
    kw = json.loads(str(g[p + "kwargs"]))
    roi_r = kw.get("roi_r", 60 / 130)
    for i, tag in enumerate(g[p + "rec_round"]):
        roi = g[p + "rec_roi"][starts[i]:starts[i + 1]]
        if str(tag).startswith("z"):
            got = (aim._get_fft_peak_z(roi, 2 * roi_r), np.nan)
        else:
            box = int(round(np.sqrt(roi.size)))
            got = aim._get_fft_peak(roi.reshape(box, box), 2 * roi_r)
        assert np.array_equal(np.array(got, np.float64), g[p + "rec_peak"][i], equal_nan=True), (name, i)


def test_golden_pins_float32_key_collisions(g):
    """Case e: on a 2048 px frame most round-1 keys differ from their float64 value (cells merge)."""
    x, y = g["e_wide_2048/in_x"], g["e_wide_2048/in_y"]
    d, W = 20 / 130, 2048 / (20 / 130)
    k32 = rs.keys(rs.XY_F32, x, y, None, (0, 0), d, W)
    k64 = rs.keys(rs.XY_F64, x, y, None, (0, 0), d, W)
    assert (k32 != k64).mean() > 0.5


def test_golden_pins_int_min_key(g):
    k = rs.keys(rs.XY_F32, g["f_outside_nan/in_x"], g["f_outside_nan/in_y"], None, (0, 0), 20 / 130, 16 / (20 / 130))
    assert (k == np.iinfo(np.int32).min).sum() >= 2


def _locs():
    return pd.DataFrame({"frame": np.arange(10, dtype=np.uint32), "x": np.ones(10, np.float32),
                         "y": np.ones(10, np.float32)})


def test_progress_type_checked():
    with pytest.raises(AssertionError, match="progress must be None"):
        aim.aim(_locs(), [{"Width": 8, "Height": 8, "Pixelsize": 130, "Frames": 10}], progress="tqdm")
    with pytest.raises(AssertionError, match="progress must be None"):
        aim.aim(_locs(), [{"Width": 8, "Height": 8, "Pixelsize": 130, "Frames": 10}], progress=object())


@pytest.mark.parametrize("missing", ["Width", "Height", "Pixelsize", "Frames"])
def test_missing_metadata_raises(missing):
    info = {"Width": 8, "Height": 8, "Pixelsize": 130, "Frames": 10}
    del info[missing]
    with pytest.raises(KeyError, match=missing):
        aim.aim(_locs(), [info])


def test_intersection_max_round_checked():
    with pytest.raises(AssertionError, match="aim_round must be 1 or 2"):
        aim.intersection_max(None, None, None, None, None, [0, 1], 0.1, 0.3, 8, aim_round=3)


def test_no_device_raises(monkeypatch):
    monkeypatch.setattr(_lib, "device_count", lambda: 0)
    with pytest.raises(_lib.HipBackendError):
        aim.aim(_locs(), [{"Width": 8, "Height": 8, "Pixelsize": 130, "Frames": 10}], segmentation=2)


def test_install_rebinds_aim():
    mods = {n: types.ModuleType("picasso." + n) for n in
            ("localize", "gaussmle", "gausslq", "zfit", "render", "imageprocess", "postprocess", "aim")}
    localize.install(mods["localize"], mods["gaussmle"], mods["gausslq"], mods["zfit"], mods["render"],
                     mods["imageprocess"], mods["postprocess"], picasso_aim=mods["aim"])
    for name in ("aim", "intersection_max", "intersection_max_z"):
        assert getattr(mods["aim"], name) is getattr(aim, name)


def test_abi_version_and_symbols():
    assert _lib.load().pmi_version() >= 107
    for name in ("pmi_aim_partition_dev", "pmi_aim_table_create_dev", "pmi_aim_count_dev", "pmi_aim_roi_cc"):
        assert name in _lib.SYMBOLS


def test_goldens_regenerate(g):
    """The committed aim_cases.npz is what make_goldens_aim.py mints from the reference tree today."""
    ref = os.environ.get("PICASSO_REFERENCE", "/root/reference")
    if not os.path.isfile(os.path.join(ref, "picasso", "aim.py")):
        pytest.skip("reference tree not present")
    import make_goldens_aim as mk
    ns = mk.load_reference()
    cases = mk.cases()
    for name in ("a_testdata", "d_gaps_unsorted", "f_outside_nan"):
        locs, info, kw = cases[name]
        mk.STATE.update(rec=[], inputs={}, round=None, seg=None)
        new_locs, _, drift = ns["aim"](locs, info, **kw)
        assert np.array_equal(new_locs["x"].to_numpy(), g[name + "/out_x"], equal_nan=True)
        assert np.array_equal(drift["y"].to_numpy(), g[name + "/drift_y"])
        assert np.array_equal(np.concatenate([r[2].ravel() for r in mk.STATE["rec"]]), g[name + "/rec_roi"])
