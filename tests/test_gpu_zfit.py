"""GPU tier of the z fit and the ROI sum (picasso_amd/csrc/zfit.hip): zfit_kernel against scipy itself
(tests/golden/_zfit_restate.py) in the bits of float64 z and sq on every row of the hostile input sets, at the block
and device-count edges, across scratch regrowth and through picasso_amd.zfit.zfit; avgroi_kernel against the
sequential float64 sum.  Every input set went through the oracle on the CPU first (tests/test_zfit_host.py)."""
import ctypes
import os
import sys
import warnings

import numpy as np
import pandas as pd
import pytest
import scipy

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import _zfit_restate as zr  # noqa: E402

pytestmark = pytest.mark.gpu
print(f"scipy {scipy.__version__}")

SENTINEL64 = 0x5A5A5A5A5A5A5A5A
SENTINEL32 = 0x5A5A5A5A
N_EDGE = 513


@pytest.fixture(scope="module")
def refs():
    """name -> [(label, sx, sy, cx, cy, z, sq)]: scipy once per set, never modified."""
    out = {}
    for name, make in zr.SETS.items():
        out[name] = [(label, sx, sy, cx, cy, *zr.fit(sx, sy, cx, cy)) for label, sx, sy, cx, cy in make()]
        for case in out[name]:
            for a in case[1:]:
                a.setflags(write=False)
    return out


@pytest.fixture(scope="module")
def mixed(refs):
    """513 rows on the committed calibration: the whole `widths` set (special values, zeros of the target, bounds) and
    the first rows of `ordinary`.  -> (sx, sy, cx, cy, z, sq)."""
    (_, wsx, wsy, cx, cy, wz, wsq), = refs["widths"]
    (_, osx, osy, _, _, oz, osq), = refs["ordinary"]
    k = N_EDGE - len(wsx)
    assert 0 < k <= len(osx)
    cat = lambda a, b: np.concatenate([a, b[:k]])      # noqa: E731
    return cat(wsx, osx), cat(wsy, osy), cx, cy, cat(wz, oz), cat(wsq, osq)


def assert_bits(z, sq, z_ref, sq_ref, label):
    bad = np.flatnonzero(~(zr.bits_equal(z, z_ref) & zr.bits_equal(sq, sq_ref)))
    assert len(bad) == 0, (f"{label}: {len(bad)} of {len(z)} rows differ from scipy, first row {bad[0]}: "
                           f"z {z[bad[0]]!r} vs {z_ref[bad[0]]!r}, sq {sq[bad[0]]!r} vs {sq_ref[bad[0]]!r}")


@pytest.mark.parametrize("name", list(zr.SETS))
def test_hostile_sets_equal_scipy_in_bits(name, refs):
    from picasso_amd import backend
    for label, sx, sy, cx, cy, z_ref, sq_ref in refs[name]:
        z, sq = backend.zfit_arrays(sx, sy, cx, cy)
        assert z.dtype == np.float64 and sq.dtype == np.float64 and z.shape == sq.shape == sx.shape
        assert_bits(z, sq, z_ref, sq_ref, f"{name}/{label}")


@pytest.mark.parametrize("n", [1, 255, 256, 257, 513])
def test_block_edges(n, mixed):
    """N around the 256-lane block through pmi_zfit; the rows are the last n, so the special widths sit in every size."""
    from picasso_amd import backend
    sx, sy, cx, cy, z_ref, sq_ref = mixed
    z, sq = backend.zfit_arrays(sx[-n:], sy[-n:], cx, cy)
    assert_bits(z, sq, z_ref[-n:], sq_ref[-n:], f"last {n}")
    z, sq = backend.zfit_arrays(sx[:n], sy[:n], cx, cy)
    assert_bits(z, sq, z_ref[:n], sq_ref[:n], f"first {n}")


def _zfit_dev(sx, sy, cx, cy, n, d_n):
    """pmi_zfit_dev on device arrays pre-filled with the sentinel -> (z, sq) as uint64 bit patterns."""
    import torch
    from picasso_amd import _lib
    d_sx, d_sy = torch.from_numpy(np.array(sx)).cuda(), torch.from_numpy(np.array(sy)).cuda()
    sentinel = np.array(SENTINEL64, np.uint64).view(np.int64).item()
    d_z = torch.full((len(sx),), sentinel, dtype=torch.int64, device="cuda")
    d_sq = torch.full((len(sx),), sentinel, dtype=torch.int64, device="cuda")
    d_cnt = torch.tensor([d_n], dtype=torch.int64, device="cuda") if d_n is not None else None
    torch.cuda.synchronize()
    p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None      # noqa: E731
    cx, cy = np.ascontiguousarray(cx, np.float64), np.ascontiguousarray(cy, np.float64)
    with _lib.lock():
        rc = _lib.load().pmi_zfit_dev(p(d_sx), p(d_sy), n, p(d_cnt), _lib.ptr(cx), _lib.ptr(cy), p(d_z), p(d_sq), None)
        _lib.check(rc, "pmi_zfit_dev")
        torch.cuda.synchronize()
    return d_z.cpu().numpy().view(np.uint64), d_sq.cpu().numpy().view(np.uint64)


@pytest.mark.parametrize("d_n", [None, 0, 1, 256, N_EDGE - 1, N_EDGE, N_EDGE + 7])
def test_device_count_clamp(d_n, mixed):
    """pmi_zfit_dev with a count on the device: rows below min(d_n, N) equal scipy, rows at or above it keep the
    sentinel, bit for bit."""
    sx, sy, cx, cy, z_ref, sq_ref = mixed
    z, sq = _zfit_dev(sx, sy, cx, cy, N_EDGE, d_n)
    n = N_EDGE if d_n is None else min(d_n, N_EDGE)
    assert_bits(z[:n].view(np.float64), sq[:n].view(np.float64), z_ref[:n], sq_ref[:n], f"d_n {d_n}")
    assert np.all(z[n:] == SENTINEL64) and np.all(sq[n:] == SENTINEL64)


def test_zero_rows_touch_nothing(mixed):
    from picasso_amd import _lib, backend
    sx, sy, cx, cy, _, _ = mixed
    z, sq = _zfit_dev(sx[:8], sy[:8], cx, cy, 0, 8)
    assert np.all(z == SENTINEL64) and np.all(sq == SENTINEL64)
    z, sq = _zfit_dev(sx[:8], sy[:8], cx, cy, 0, None)
    assert np.all(z == SENTINEL64) and np.all(sq == SENTINEL64)
    with _lib.lock():
        _lib.check(_lib.load().pmi_zfit(None, None, 0, _lib.ptr(cx), _lib.ptr(cy), None, None), "pmi_zfit")
    z, sq = backend.zfit_arrays(sx[:0], sy[:0], cx, cy)
    assert z.shape == (0,) and sq.shape == (0,)


def test_two_calls_one_answer(mixed):
    """The same inputs before and after a larger call that regrows the staging scratch: the same bits, scipy's."""
    from picasso_amd import _lib, backend
    sx, sy, cx, cy, z_ref, sq_ref = mixed
    with _lib.lock():
        _lib.check(_lib.load().pmi_release_scratch(), "pmi_release_scratch")
    z1, sq1 = backend.zfit_arrays(sx, sy, cx, cy)
    rng = np.random.default_rng(5)
    big = rng.uniform(0.6, 3.2, (2, 40 * N_EDGE)).astype(np.float32)
    zb, _ = backend.zfit_arrays(big[0], big[1], cx, cy)
    assert np.all(np.abs(zb) < 1000)
    z2, sq2 = backend.zfit_arrays(sx, sy, cx, cy)
    assert np.array_equal(z1.view(np.uint64), z2.view(np.uint64)) and np.array_equal(sq1.view(np.uint64), sq2.view(np.uint64))
    assert_bits(z2, sq2, z_ref, sq_ref, "second call")


# ---- avgroi_kernel -------------------------------------------------------------------------------------------------
def _spots(n, box, seed):
    """Signed pixels over twelve decades, and in every fifth spot a NaN, a +inf or a -inf pixel (some spots get two)."""
    rng = np.random.default_rng(seed)
    s = (10.0 ** rng.uniform(-6, 6, (n, box, box)) * rng.choice([-1.0, 1.0], (n, box, box))).astype(np.float32)
    for i in range(0, n, 5):
        for v in ((np.nan, np.inf, -np.inf)[(i // 5) % 3], (np.inf, -np.inf)[(i // 15) % 2])[:1 + (i // 5) % 2]:
            s[i, rng.integers(box), rng.integers(box)] = v
    return s


def _sequential_sum(spots):
    """float64 left-to-right sum in row-major pixel order, cast to float32 (np.add.accumulate cannot reorder)."""
    with np.errstate(all="ignore"):
        return np.add.accumulate(spots.reshape(len(spots), -1).astype(np.float64), axis=1)[:, -1].astype(np.float32)


def _assert_theta(theta, want, label):
    assert theta.dtype == np.float32 and theta.shape == (len(want), 6)
    bits = theta.view(np.uint32)
    assert np.all(bits[:, [0, 1]] == 0) and np.all(bits[:, [4, 5]] == np.float32(1).view(np.uint32)), label
    for col in (2, 3):
        got = theta[:, col]
        assert np.array_equal(np.isnan(got), np.isnan(want)), label
        ok = np.isnan(want) | (got.view(np.uint32) == want.view(np.uint32))
        assert ok.all(), f"{label}: column {col} row {np.flatnonzero(~ok)[0]}: {got[~ok][0]!r} vs {want[~ok][0]!r}"


@pytest.mark.parametrize("box", [1, 3, 7, 21])
@pytest.mark.parametrize("n", [1, 255, 257])
def test_avgroi_equals_sequential_float64_sum(box, n):
    from picasso_amd import backend
    spots = _spots(n, box, 100 * box + n)
    want = _sequential_sum(spots)
    if n > 1:
        assert np.isnan(want).any() and np.isinf(want).any() and np.isfinite(want).any()
    _assert_theta(backend.avgroi_array(spots), want, f"box {box} n {n}")


@pytest.mark.parametrize("d_n", [None, 0, 1, 255, 256, 257, 257 + 7])
def test_avgroi_device_count_clamp(d_n):
    import torch
    from picasso_amd import _lib
    n_rows, box = 257, 7
    spots = _spots(n_rows, box, 77)
    want = _sequential_sum(spots)
    d_spots = torch.from_numpy(spots).cuda()
    sentinel = np.array(SENTINEL32, np.uint32).view(np.int32).item()
    d_theta = torch.full((n_rows, 6), sentinel, dtype=torch.int32, device="cuda")
    d_cnt = torch.tensor([d_n], dtype=torch.int64, device="cuda") if d_n is not None else None
    torch.cuda.synchronize()
    with _lib.lock():
        rc = _lib.load().pmi_avgroi_dev(ctypes.c_void_p(d_spots.data_ptr()), n_rows,
                                        ctypes.c_void_p(d_cnt.data_ptr()) if d_cnt is not None else None, box,
                                        ctypes.c_void_p(d_theta.data_ptr()), None)
        _lib.check(rc, "pmi_avgroi_dev")
        torch.cuda.synchronize()
    theta = d_theta.cpu().numpy().view(np.uint32)
    n = n_rows if d_n is None else min(d_n, n_rows)
    _assert_theta(np.ascontiguousarray(theta[:n]).view(np.float32), want[:n], f"d_n {d_n}")
    assert np.all(theta[n:] == SENTINEL32)


# ---- the pipeline --------------------------------------------------------------------------------------------------
def _locs(sx, sy, seed):
    rng = np.random.default_rng(seed)
    n = len(sx)
    f32 = lambda lo, hi: rng.uniform(lo, hi, n).astype(np.float32)      # noqa: E731
    return pd.DataFrame({"frame": np.sort(rng.integers(0, 50, n)).astype(np.uint32), "x": f32(0, 32), "y": f32(0, 32),
                         "photons": f32(1e3, 1e4), "sx": np.array(sx), "sy": np.array(sy), "bg": f32(5, 50),
                         "lpx": f32(0.01, 0.05), "lpy": f32(0.01, 0.05), "sx_unc": f32(0.005, 0.05),
                         "sy_unc": f32(0.005, 0.05)})


# table -> (set, label of the calibration, whether the reference keeps any row)
PIPELINE_TABLES = {
    "mixed": None,                                                   # special widths: dropped for their sx / sy
    "x_negative_beyond_300": ("negative_width", True),               # sane fits beside a NaN region
    "both_negative_beyond_200": ("negative_width", False),           # first point NaN: sq NaN on every row
    "c0_1e+282": ("steep", False),                                   # sq finite in float64, inf once stored as float32
    "c0_1e+294": ("steep", False),                                   # sq inf
    "flat": ("flat_and_twin", False),                                # z and sq sane, lpz 0 / 0
    "bound": ("flat_and_twin", True),                                # fits on both bounds
}


@pytest.mark.parametrize("which", list(PIPELINE_TABLES))
@pytest.mark.parametrize("method", ["gausslq", "gaussmle"])
@pytest.mark.parametrize("filter", [0, 2])
def test_pipeline_equals_table_math_on_scipy_z(which, method, filter, mixed, refs):
    """picasso_amd.zfit.zfit on hostile tables: the rows kept (lib.ensure_sanity drops NaN / inf z, d_zcalib and lpz
    like the reference, filter_z_fits cuts on the RMS residual of what is left) and the float32 bits of z and
    d_zcalib are what the reference's table math makes of scipy's z and sq.  With sane widths a fit result is NaN or
    inf for a whole calibration, never for single rows (sq is NaN exactly when the first point is), so the tables
    whose sx, sy and other columns are all sane and whose sq or lpz is not must come back empty, as they do from the
    reference; in `mixed` every NaN row already has a NaN, inf or negative width."""
    from picasso_amd import zfit
    if which == "mixed":
        sx, sy, cx, cy, z_ref, sq_ref = mixed
        keeps = True
    else:
        name, keeps = PIPELINE_TABLES[which]
        (sx, sy, cx, cy, z_ref, sq_ref), = [c[1:] for c in refs[name] if c[0] == which]
    locs = _locs(sx, sy, 31)
    info = [{"Width": 32, "Height": 32, "Frames": 50, "Pixelsize": 130}]
    calib = {"X Coefficients": list(cx), "Y Coefficients": list(cy), "Magnification factor": 0.79}
    want = zr.table(locs, info, cx, cy, 0.79, 130, method, filter, z_ref, sq_ref)
    if keeps:
        assert len(want) > 20 and (which != "mixed" or len(want) < len(locs))
    else:
        assert len(want) == 0 and np.all(locs[["sx", "sy", "photons", "lpx"]].to_numpy() > 0)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)          # float32 overflow of sq, nanmean of no rows
        out, _ = zfit.zfit(locs, [dict(info[0])], calibration=dict(calib), fitting_method=method, filter=filter)
    assert list(out.index) == list(want.index)
    for col in ("z", "d_zcalib"):
        assert out[col].dtype == np.float32
        assert np.array_equal(out[col].to_numpy().view(np.uint32), want[col].to_numpy().view(np.uint32)), col
