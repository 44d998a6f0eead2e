"""GPU tier of AIM's edge cases: csrc/aim.hip on the seams of its control flow, count for count against the reference's
recorded roi_cc (tests/golden/aim_edge_cases.npz) or the test-side restatement (tests/golden/_aim_restate.py).  Every
comparison is integer equality.  The cases and the constant each one straddles are in tests/golden/_aim_edges.py;
tests/test_aim_edges_host.py holds them to the sources."""
import json
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN, golden

sys.path.insert(0, GOLDEN)
import _aim_edges as ae  # noqa: E402
import _aim_restate as rs  # noqa: E402

from picasso_amd import _lib, aim, backend  # noqa: E402

pytestmark = pytest.mark.gpu
CASES = [str(c) for c in golden("aim_edge_cases")["case_names"]]
DEV = "cuda"


@pytest.fixture(scope="module")
def g():
    return golden("aim_edge_cases")


@pytest.fixture
def dense_limit():
    """Set the dense limit for one test; the default comes back whatever happens."""
    try:
        yield backend.aim_set_dense_limit
    finally:
        backend.aim_set_dense_limit(ae.DENSE_LIMIT)


def dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).to(DEV)


def rows_of(lo, hi):
    return torch.arange(lo, hi, dtype=torch.int32, device=DEV)


def dense_admissible(mode, ref_keys, shifts, limit=ae.DENSE_LIMIT):
    """What table_create decides: x / y keys whose span plus the largest shift on either side fits the limit."""
    if mode in (rs.Z_F32, rs.Z_F64):
        return False
    span = int(ref_keys.max()) - int(ref_keys.min()) + 1 if len(ref_keys) else 0
    return span + 2 * int(np.abs(np.asarray(shifts, np.int64)).max()) <= limit


# ---- the fixture, through intersection_max / intersection_max_z ---------------------------------------------------------
@pytest.mark.parametrize("form", ["default", "sorted"])
@pytest.mark.parametrize("name", CASES)
def test_fixture_case_equals_reference(g, name, form, dense_limit, monkeypatch):
    p = name + "/"
    info = json.loads(str(g[p + "info_in"]))[0]
    kw = json.loads(str(g[p + "kwargs"]))
    rounds = list(rs.golden_rounds(g, name))
    mode, ref, sh, d, W, H = rounds[0][4], rounds[0][5], rounds[0][11], rounds[0][8], rounds[0][9], rounds[0][10]
    want_dense = form == "default" and dense_admissible(mode, rs.keys(mode, *ref, (0, 0, 0), d, W, H), sh)
    assert want_dense == (form == "default" and name in ("wrap_hi_f64", "wrap_lo_f64", "multiplicity", "shifts_289"))
    seen = []

    class Spy(backend.AimTable):
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            seen.append(self.info())

    monkeypatch.setattr(backend, "AimTable", Spy)
    if form == "sorted":
        dense_limit(0)
    frame = g[p + "in_frame"].astype(np.int64) + 1
    first = frame <= kw["segmentation"]
    bounds = np.concatenate((np.arange(0, info["Frames"], kw["segmentation"]), [info["Frames"]]))
    x, y = g[p + "in_x"], g[p + "in_y"]
    aim._trace = []
    try:
        if p + "in_z" in g:
            z = g[p + "in_z"]
            aim.intersection_max_z(x, y, z, x[first], y[first], z[first], frame, bounds, kw["intersect_d"], kw["roi_r"],
                                   info["Width"], info["Height"], info["Pixelsize"], aim_round=1)
        else:
            aim.intersection_max(x, y, x[first], y[first], frame, bounds, kw["intersect_d"], kw["roi_r"], info["Width"],
                                 aim_round=1)
        trace = aim._trace
    finally:
        aim._trace = None
    assert seen == [("dense" if want_dense else "sorted", seen[0][1])]
    starts = np.concatenate(([0], np.cumsum(g[p + "rec_len"])))
    assert len(trace) == len(g[p + "rec_seg"]) == 2
    for i, (tag, s, roi, peak) in enumerate(trace):
        assert tag == str(g[p + "rec_round"][i]) and s == g[p + "rec_seg"][i]
        want = g[p + "rec_roi"][starts[i]:starts[i + 1]]
        assert np.array_equal(roi.ravel(), want), (name, form, s, int((roi.ravel() != want).sum()))
        assert np.array_equal(np.array((tuple(peak) + (np.nan,))[:2], np.float64), g[p + "rec_peak"][i], equal_nan=True)


# ---- the second trip of the grid-stride loop (GRID_FACTOR * CUs * BLOCK rows, then GRID_TAIL more) ------------------------
@pytest.fixture(scope="module")
def grid_table():
    """Cells of a 32 px frame at d = 0.25; the last GRID_TAIL targets share a cell no other target has, which the
    reference set holds 300 times.  Built once, with the restatement's counts of the whole table and of the table
    without its tail."""
    cu = torch.cuda.get_device_properties(0).multi_processor_count
    n = ae.grid_stride_rows(cu)
    assert n == ae.GRID_FACTOR * cu * ae.BLOCK + ae.GRID_TAIL
    rng = np.random.default_rng(8)
    d = 0.25
    cell = lambda m: rng.integers(8, 100, m) * d  # noqa: E731
    ref = [np.concatenate((cell(3000), np.full(300, 120 * d))) for _ in range(2)] + [np.concatenate((np.rint(rng.normal(0, 1, 3000)), np.full(300, 5.0))) * d]
    tgt = [np.concatenate((cell(n - ae.GRID_TAIL), np.full(ae.GRID_TAIL, 120 * d))) for _ in range(2)]
    tgt.append(np.concatenate((np.rint(rng.normal(0, 1, n - ae.GRID_TAIL)).clip(-4, 4), np.full(ae.GRID_TAIL, 5.0))) * d)
    return n, d, ref, tgt


@pytest.mark.parametrize("mode,form", [(rs.XY_F32, "dense"), (rs.XY_F32, "sorted"), (rs.Z_F64, "sorted")])
def test_grid_stride_second_trip(grid_table, mode, form, dense_limit):
    n, d, ref, tgt = grid_table
    W = H = 32 / d
    zmode = mode == rs.Z_F64
    sh = rs.shifts_z(1.0, d, 32, 32) if zmode else rs.shifts_xy(0.25, d, 32)[0]
    assert len(sh) == 9
    r = tuple(ref) if zmode else (ref[0].astype(np.float32), ref[1].astype(np.float32), None)
    t = tuple(tgt) if zmode else (tgt[0].astype(np.float32), tgt[1].astype(np.float32), None)
    rk, tk = rs.keys(mode, *r, (0, 0, 0), d, W, H), rs.keys(mode, *t, (0, 0, 0), d, W, H)
    tail = tk[-ae.GRID_TAIL:]
    assert len(tk) == n and (tail == tail[0]).all() and not (tk[:-ae.GRID_TAIL] == tail[0]).any()
    assert (rk == tail[0]).sum() == 300 > ae.GRID_TAIL
    want, short = rs.roi_cc(rk, tk, sh), rs.roi_cc(rk, tk[:-ae.GRID_TAIL], sh)
    assert want[4] - short[4] == ae.GRID_TAIL and want.min() > 0
    if form == "sorted":
        dense_limit(0)
    got = backend.aim_roi_cc_arrays(mode, r[:3 if zmode else 2], t[:3 if zmode else 2], (0, 0, 0), d, W, H if zmode else 0.0, sh)
    assert not np.array_equal(got, short), "the rows of the second grid-stride trip were dropped"
    assert np.array_equal(got, want), (got - want).tolist()


# ---- shift counts on the BLOCK seam of the LDS loops and on MAX_SHIFTS -----------------------------------------------------
def shift_case(n_shifts, zmode):
    """Distinct shifts 7 i; 300 targets on five keys; reference keys at target + shift for the first, the last and the
    shifts next to the BLOCK seam, so each of those has a count (the last one in particular)."""
    step = np.arange(n_shifts, dtype=np.int64) * 7 - 7 * (n_shifts // 3)
    marked = sorted({i for i in (0, 254, 255, 256, 257, n_shifts // 2, n_shifts - 2, n_shifts - 1) if 0 <= i < n_shifts})
    tk = 1000 + np.arange(300) % 5
    rk = np.concatenate([np.repeat(1000 + j + step[i], 1 + (i + j) % 3) for i in marked for j in range(5)])
    if zmode:
        sh = step.astype(np.float64)
        sh[1:-1:2] += 0.5                                   # every other shift can match nothing
        return rs.Z_F64, ae.xyz_of_keys(rk), ae.xyz_of_keys(tk), sh, (ae.Z_D, ae.Z_W, ae.Z_H)
    return rs.XY_F64, ae.xy_of_keys(rk) + (None,), ae.xy_of_keys(tk) + (None,), step.astype(np.int32), (ae.XY_D, ae.XY_W, 0.0)


@pytest.mark.parametrize("zmode", [False, True], ids=["xy", "z"])
@pytest.mark.parametrize("n_shifts", ae.SHIFT_COUNTS)
def test_shift_counts_on_the_block_seam_and_the_bound(n_shifts, zmode, dense_limit):
    mode, r, t, sh, (d, W, H) = shift_case(n_shifts, zmode)
    assert len(sh) == n_shifts == len(np.unique(sh))
    want = rs.roi_cc(rs.keys(mode, *r, (0, 0, 0), d, W, H), rs.keys(mode, *t, (0, 0, 0), d, W, H), sh)
    assert want[-1] > 0 and want[0] > 0 and (n_shifts < 3 or (want == 0).any())
    n_col = 3 if zmode else 2
    for limit in (ae.DENSE_LIMIT, 0):
        dense_limit(limit)
        got = backend.aim_roi_cc_arrays(mode, r[:n_col], t[:n_col], (0, 0, 0), d, W, H, sh)
        assert np.array_equal(got, want), (n_shifts, limit, np.flatnonzero(got != want)[:8].tolist())


@pytest.mark.parametrize("zmode", [False, True], ids=["xy", "z"])
def test_one_shift_past_the_bound_raises(zmode):
    mode, r, t, sh, (d, W, H) = shift_case(ae.MAX_SHIFTS + 1, zmode)
    n_col = 3 if zmode else 2
    with pytest.raises(_lib.HipBackendError):
        backend.aim_roi_cc_arrays(mode, r[:n_col], t[:n_col], (0, 0, 0), d, W, H, sh)
    x = dev(r[0], np.float64)
    with pytest.raises(_lib.HipBackendError):
        backend.AimTable(mode, x, dev(r[1], np.float64), dev(r[2], np.float64) if zmode else None, None, x.numel(), d, W, H, sh)


# ---- the target hash of the sorted form: wrap-around chains, growth, reuse after cleanup ------------------------------------
@pytest.mark.parametrize("zmode", [False, True], ids=["xy", "z"])
def test_hash_wraps_grows_and_is_reused(zmode, dense_limit):
    ref, tgt, segs, step = ae.hash_case(zmode)
    if zmode:
        mode, (d, W, H), of = rs.Z_F64, (ae.Z_D, ae.Z_W, ae.Z_H), ae.xyz_of_keys
        sh = np.array([-step, 0, step], np.float64)
    else:
        mode, (d, W, H), of = rs.XY_F64, (ae.XY_D, ae.XY_W, 0.0), lambda k: ae.xy_of_keys(k) + (None,)
        sh = np.array([-step, 0, step], np.int32)
    r, t = of(ref), of(tgt)
    rk, tk = rs.keys(mode, *r, (0, 0, 0), d, W, H), rs.keys(mode, *t, (0, 0, 0), d, W, H)
    assert np.array_equal(rk, ref) and np.array_equal(tk, tgt)
    dense_limit(0)
    cols = [dev(c, np.float64) for c in r[:3 if zmode else 2]] + [None] * (0 if zmode else 1)
    table = backend.AimTable(mode, *cols, None, len(ref), d, W, H, sh)
    try:
        assert table.info() == ("sorted", len(ref))
        table.x, table.y, table.z = [dev(c, np.float64) for c in t[:3 if zmode else 2]] + [None] * (0 if zmode else 1)
        got = [table.count(rows_of(lo, hi)) for lo, hi in segs]
    finally:
        table.close()
    for (lo, hi), have in zip(segs, got):
        want = rs.roi_cc(rk, tk[lo:hi], sh)
        assert np.array_equal(have, want), ((lo, hi), have.tolist(), want.tolist())
        assert want.min() > 0
    assert np.array_equal(got[1], got[3])


# ---- the switch between the two table forms ----------------------------------------------------------------------------------
def test_dense_limit_boundary(dense_limit):
    rng = np.random.default_rng(28)
    ref, tgt = rng.integers(5000, 9000, 700), rng.integers(4900, 9100, 900)
    sh = np.array([-70, 0, 3, 70], np.int32)
    r, t = ae.xy_of_keys(ref), ae.xy_of_keys(tgt)
    rk = rs.keys(rs.XY_F64, *r, None, (0, 0), ae.XY_D, ae.XY_W)
    tk = rs.keys(rs.XY_F64, *t, None, (0, 0), ae.XY_D, ae.XY_W)
    span = int(rk.max()) - int(rk.min()) + 1
    tsize = span + 2 * int(np.abs(sh.astype(np.int64)).max())
    want = rs.roi_cc(rk, tk, sh)
    assert want.min() > 0
    rx, ry, tx, ty = (dev(c, np.float64) for c in r + t)
    got = {}
    for limit, form, entries in ((tsize, "dense", span), (tsize - 1, "sorted", len(ref)), (tsize + 1, "dense", span)):
        dense_limit(limit)
        table = backend.AimTable(rs.XY_F64, rx, ry, None, None, len(ref), ae.XY_D, ae.XY_W, 0.0, sh)
        try:
            assert table.info() == (form, entries), (limit, tsize)
            table.x, table.y = tx, ty
            got[limit] = table.count(rows_of(0, len(tgt)))
        finally:
            table.close()
        assert np.array_equal(got[limit], want), (limit, form)
    assert np.array_equal(got[tsize], got[tsize - 1])


def test_dense_form_wraps_modulo_2_32(dense_limit):
    """Reference keys up to INT32_MAX: the target counters run past it, and targets at INT32_MIN sit in them modulo 2^32."""
    top = 2 ** 31 - 1
    ref = np.concatenate((top - np.arange(40), top - np.arange(5), [top] * 3))
    tgt = np.concatenate((top - np.arange(60), -2 ** 31 + np.arange(50), -2 ** 31 + np.arange(7), [top - 90] * 3))
    sh = np.array([-45, -3, 0, 2, 45], np.int32)
    r, t = ae.xy_of_keys(ref), ae.xy_of_keys(tgt)
    rk = rs.keys(rs.XY_F64, *r, None, (0, 0), ae.XY_D, ae.XY_W)
    tk = rs.keys(rs.XY_F64, *t, None, (0, 0), ae.XY_D, ae.XY_W)
    assert np.array_equal(rk, ref) and np.array_equal(tk, tgt)
    want = rs.roi_cc(rk, tk, sh)
    no_wrap = rs.roi_cc(rk, tk[tk > 0], sh)
    assert want[0] > no_wrap[0] and want[1] > no_wrap[1]             # counts that are there because key + shift wrapped
    rx, ry, tx, ty = (dev(c, np.float64) for c in r + t)
    for limit, form in ((ae.DENSE_LIMIT, "dense"), (0, "sorted")):
        dense_limit(limit)
        table = backend.AimTable(rs.XY_F64, rx, ry, None, None, len(ref), ae.XY_D, ae.XY_W, 0.0, sh)
        try:
            assert table.info()[0] == form
            table.x, table.y = tx, ty
            got = table.count(rows_of(0, len(tgt)))
        finally:
            table.close()
        assert np.array_equal(got, want), (form, got.tolist(), want.tolist())


# ---- empty sides -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["dense", "sorted"])
@pytest.mark.parametrize("mode", [rs.XY_F32, rs.Z_F64], ids=["xy_f32", "z_f64"])
def test_empty_sides(mode, form, dense_limit):
    zmode = mode == rs.Z_F64
    if zmode and form == "dense":
        form = "sorted"                                  # a z table has the sorted form at any limit: run it at the default
    else:
        dense_limit(ae.DENSE_LIMIT if form == "dense" else 0)
    rng = np.random.default_rng(40)
    d, W, H = 0.25, 128.0, 128.0 if zmode else 0.0
    xy_t = np.float64 if zmode else np.float32
    cols = [rng.integers(8, 40, 500) * d, rng.integers(8, 40, 500) * d] + ([rng.integers(-2, 3, 500) * d] if zmode else [])
    sh = rs.shifts_z(0.5, d, 32, 32) if zmode else rs.shifts_xy(0.25, d, 32)[0]
    host = tuple(np.ascontiguousarray(c, xy_t) for c in cols) + (() if zmode else (None,))
    k = rs.keys(mode, *host, (0, 0, 0), d, W, H)
    tensors = [dev(c, xy_t) for c in cols] + ([] if zmode else [None])
    none = torch.empty(0, dtype=torch.int32, device=DEV)
    zeros = np.zeros(len(sh), np.int64)

    # no reference rows: every count is zero, for no targets and for 300 of them
    table = backend.AimTable(mode, *tensors, none, 0, d, W, H, sh)
    try:
        assert table.info() == (form, 0)
        assert np.array_equal(table.count(none), zeros)
        assert np.array_equal(table.count(rows_of(200, 500)), zeros)
        assert np.array_equal(table.count(none), zeros)
    finally:
        table.close()
    # no target rows, then a populated count on the same table
    table = backend.AimTable(mode, *tensors, rows_of(0, 200), 200, d, W, H, sh)
    try:
        assert table.info()[0] == form
        assert np.array_equal(table.count(none), zeros)
        want = rs.roi_cc(k[:200], k[200:], sh)
        assert want.max() > 0
        assert np.array_equal(table.count(rows_of(200, 500)), want)
        assert np.array_equal(table.count(none), zeros)
        assert np.array_equal(table.count(rows_of(200, 500)), want)
    finally:
        table.close()
    # the same from host columns
    n_col = 3 if zmode else 2
    empty = tuple(c[:0] for c in host[:n_col])
    for r, t in ((empty, host[:n_col]), (host[:n_col], empty), (empty, empty)):
        assert np.array_equal(backend.aim_roi_cc_arrays(mode, r, t, (0, 0, 0), d, W, H, sh), zeros)


# ---- the partition on its own ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seg_len,n_frames", ae.PARTITION_SHAPES)
@pytest.mark.parametrize("n", ae.PARTITION_ROWS)
def test_partition(n, seg_len, n_frames):
    frame = ae.partition_frames(n, seg_len, n_frames, n)
    offsets, sets = ae.partition_restated(frame, seg_len, n_frames)
    rows, got = backend.aim_partition(torch.from_numpy(frame).to(DEV), seg_len, n_frames)
    assert got.dtype == np.int64 and np.array_equal(got, offsets), (got.tolist(), offsets.tolist())
    rows = rows.cpu().numpy()[:offsets[-1]]
    for s, want in enumerate(sets):
        assert np.array_equal(np.sort(rows[offsets[s]:offsets[s + 1]]), want), s


# ---- a table outlives what other calls do to the scratch ----------------------------------------------------------------------
@pytest.mark.parametrize("form", ["dense", "sorted"])
def test_a_second_table_leaves_the_first_alone(form, dense_limit):
    dense_limit(ae.DENSE_LIMIT if form == "dense" else 0)
    rng = np.random.default_rng(2)
    sh = np.array([-700, -1, 0, 1, 700], np.int32)
    ka, kb = rng.integers(100_000, 103_000, 2000), rng.integers(-2 ** 31, 2 ** 31, 50_000)
    ta = rng.integers(100_000, 103_000, 1500)
    want = rs.roi_cc(ka.astype(np.int32), ta.astype(np.int32), sh)
    assert want.min() > 0
    cols = lambda k: [dev(c, np.float64) for c in ae.xy_of_keys(k)]  # noqa: E731
    a = backend.AimTable(rs.XY_F64, *cols(ka), None, None, len(ka), ae.XY_D, ae.XY_W, 0.0, sh)
    b = None
    try:
        a.x, a.y = cols(ta)
        first = a.count(rows_of(0, len(ta)))
        b = backend.AimTable(rs.XY_F64, *cols(kb), None, None, len(kb), ae.XY_D, ae.XY_W, 0.0, sh)    # sorted at any limit
        assert a.info()[0] == form and b.info() == ("sorted", len(kb))
        b.x, b.y = cols(kb[::-1].copy())
        assert np.array_equal(b.count(rows_of(0, len(kb))), rs.roi_cc(kb.astype(np.int32), kb.astype(np.int32), sh))
        second = a.count(rows_of(0, len(ta)))
    finally:
        a.close()
        if b is not None:
            b.close()
    assert np.array_equal(first, want) and np.array_equal(second, want)
