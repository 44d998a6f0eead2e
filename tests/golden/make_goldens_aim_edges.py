#!/usr/bin/env python3
"""Mint tests/golden/aim_edge_cases.npz: the reference's intersection counts on small tables that sit on the edges of
csrc/aim.hip (int32 wrap of key + shift, float32 keys that round up to 2^31, rint ties and non-finite coordinates, z
keys that leave the int32 range, key multiplicities across wave and block borders, more shifts than a block has
threads).

TEST INFRASTRUCTURE, build container only (needs the reference tree).  ``load_reference()`` of make_goldens_aim.py
executes the reference's functions from where they lie; nothing of the reference is stored here.  Every case is one
call of the reference's ``intersection_max`` / ``intersection_max_z`` in round 1 on a table of five segments of ten
frames: segment 0 is the reference set, segment 1 is counted at rel = 0, segment 2 at the peak the reference found
for segment 1, segments 3 and 4 are empty (the cubic spline needs four knots).  The columns go in as pandas Series,
as ``aim()`` passes them, and the key mode follows their dtype.  The arrays are stored in the layout of aim_cases.npz
so that ``_aim_restate.golden_rounds`` reads them.

Every case is asserted to hold what it exists for (``check``); tests/test_aim_edges_host.py repeats that on the
committed file.  The file is written with fixed zip time stamps: two runs give the same bytes.

Run:  python tests/golden/make_goldens_aim_edges.py
"""
import io
import json
import os
import sys
import zipfile

import numpy as np
import pandas as pd

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _aim_restate as rs  # noqa: E402
import make_goldens_aim as mk  # noqa: E402

PATH = os.path.join(HERE, "aim_edge_cases.npz")
I_MIN, I_MAX = -2 ** 31, 2 ** 31 - 1
SEG_LEN, N_FRAMES = 10, 50
COUNTS = (1, 2, 63, 64, 65, 257)          # multiplicity: one below / on / above a wave of 64 and a block of 256


# ---- the tables ---------------------------------------------------------------------------------------------------------
def _table(segments, dtype, z_dtype=None):
    """segments: per segment a list of (x, y[, z]) rows -> columns; row i of segment s lies in frame 10 s + 1 + i % 10,
    so the first row of the table is in frame 1."""
    cols = [np.concatenate([np.asarray(s, np.float64).reshape(len(s), -1)[:, c] for s in segments])
            for c in range(len(segments[0][0]))]
    frame = np.concatenate([SEG_LEN * s + np.arange(len(rows)) % SEG_LEN for s, rows in enumerate(segments)])
    out = {"frame": frame.astype(np.uint32), "x": cols[0].astype(dtype), "y": cols[1].astype(dtype)}
    if len(cols) == 3:
        out["z"] = cols[2].astype(z_dtype)
    return out


def _info(width, height=None, pixelsize=130):
    return [{"Frames": N_FRAMES, "Width": width, "Height": height or width, "Pixelsize": pixelsize}]


WRAP_SITES = (10, 200, 3000, 65300, 65400, 65471, 65472, 65500, 65530, 65535)


def wrap_table(side, dtype):
    """Width 65536 at d = 1: key = x + 65536 y, so y = 32767 ends at INT32_MAX and y = -32768 starts at INT32_MIN.  The
    reference set lies on one side; the targets on both, so that one row shift (+-65536) wraps a target of the far side
    onto a reference key.  In float32 the sums of the sites from 65472 on round up to 2^31."""
    near, far = (32767, -32768) if side == "hi" else (-32768, 32767)
    ref = [(x, near) for x in WRAP_SITES for _ in range(2)] + [(WRAP_SITES[1], near)] * 3
    seg1 = [(x, near) for x in WRAP_SITES for _ in range(3)] + [(x, far) for x in WRAP_SITES] + [(WRAP_SITES[3], far)] * 4
    seg2 = [(x, far) for x in WRAP_SITES] + [(x, near) for x in WRAP_SITES[2:]] * 2 + [(WRAP_SITES[1], far)] * 5
    return _table([ref, seg1, seg2], dtype), _info(65536), {"segmentation": SEG_LEN, "intersect_d": 1.0, "roi_r": 1.0}


def ties_table(dtype):
    """d = 0.25: x / d on k + 0.5 for even and odd k of both signs, -0.0, negative coordinates, and +-inf / NaN in x, in y
    and in both (every such row gets the key INT_MIN)."""
    d = 0.25
    ties = [(k + 0.5) * d for k in (0, 1, 2, 3, 4, 5, -1, -2, -3, -4)]
    inf, nan = np.inf, np.nan
    bad = [(inf, 1.0), (-inf, 1.0), (nan, 1.0), (1.0, inf), (1.0, -inf), (1.0, nan), (inf, inf), (inf, -inf), (nan, nan),
           (-inf, inf)]
    plain = [(-0.0, -0.0), (-0.0, 1.0), (-1.3, 2.1), (-0.2, -0.7), (3.0, -1.1), (2.0, 2.0)]

    def seg(k):
        rows = [(t, ties[(i + k) % len(ties)]) for i, t in enumerate(ties)] + [(1.0, t) for t in ties[k::2]]
        return rows + bad[k:] + bad[:k + 2] + plain + plain[:k + 1]
    return _table([seg(0), seg(1), seg(2)], dtype), _info(16), {"segmentation": SEG_LEN, "intersect_d": d, "roi_r": 0.25}


def z_table(z_dtype, d):
    """Pixelsize 2 on a 64 x 64 frame.  `top` is the highest z cell whose key still fits int32 (32767 at d = 0.25, where
    W H = 65536): keys next to both ends of the int32 range, which a z shift of +-W H takes out of it; z cells beyond the
    range and NaN z (key INT_MIN) in every segment; a plain cluster."""
    unit = d * 2                                         # nm per z cell
    top = int(np.ceil(2 ** 31 / (64 / d) ** 2)) - 1
    nan = np.nan

    def seg(k):
        rows = [(0.25 * (3 + i), 0.25 * (5 + 2 * i), unit * zu) for i in range(6) for zu in (-2, -1, 0, 1, 2)[k % 2:]]
        rows += [(0.25 * (1 + i), 0.25 * 7, unit * zu) for i in range(3) for zu in (top, top - 1, -top - 1, -top, 1 - top)]
        rows += [(0.25 * 9, 0.25 * 2, unit * (top + 1)), (0.25 * 9, 0.25 * 2, -unit * (top + 2))]       # beyond the range
        rows += [(0.25 * (2 + i), 0.25 * 4, nan) for i in range(2 + k)]
        return rows
    return (_table([seg(0), seg(1), seg(2)], np.float64, z_dtype), _info(64, 64, 2),
            {"segmentation": SEG_LEN, "intersect_d": d, "roi_r": 0.5 if d == 0.25 else 0.6})


def multiplicity_table():
    """18 keys, four cells apart: c_target above, below and on c_ref, each at a minimum of 1, 2, 63, 64, 65 and 257.  The
    targets lie one cell to the right (the counts are then on shift x = -1 alone), and the rows are shuffled, so the
    rows of one key are spread over the waves and blocks of the count kernel."""
    d = 0.25
    plan = [(c + a, c + b) for c in COUNTS for a, b in ((0, 2), (2, 0), (0, 0))]            # (c_ref, c_target) per site
    site = lambda i: (d * (4 * (i % 6) + 2), d * (4 * (i // 6) + 2))  # noqa: E731
    rng = np.random.default_rng(17)
    ref = [site(i) for i, (cr, _) in enumerate(plan) for _ in range(cr)]
    segs = [ref]
    for _ in (1, 2):
        t = [(site(i)[0] + d, site(i)[1]) for i, (_, ct) in enumerate(plan) for _ in range(ct)]
        segs.append([t[j] for j in rng.permutation(len(t))])
    segs[0] = [ref[j] for j in rng.permutation(len(ref))]
    # frame 1 has to hold a row: _table puts row 0 of segment 0 there
    return _table(segs, np.float32), _info(32), {"segmentation": SEG_LEN, "intersect_d": d, "roi_r": 0.25}


def shifts_289_table():
    """roi_r / d = 8: box = 17, 289 shifts.  The targets lie 8 cells to the left and 3 up, so the counts are on the shifts
    of the last x step, numbers 272 to 288: past the first pass of the LDS init and flush loops."""
    d = 0.25
    rng = np.random.default_rng(289)
    sites = np.stack([rng.integers(12, 100, 40), rng.integers(12, 100, 40)], 1) * d
    pick = lambda n: sites[rng.integers(0, len(sites), n)]  # noqa: E731
    segs = [list(map(tuple, pick(120))), list(map(tuple, pick(150) + (-8 * d, 3 * d))),
            list(map(tuple, pick(130) + (-8 * d, 3 * d)))]
    return _table(segs, np.float32), _info(32), {"segmentation": SEG_LEN, "intersect_d": d, "roi_r": 2.0}


def cases():
    out = {}
    out["wrap_hi_f64"] = wrap_table("hi", np.float64)
    out["wrap_lo_f64"] = wrap_table("lo", np.float64)
    out["wrap_f32_round_to_2p31"] = wrap_table("hi", np.float32)
    out["ties_signs_f32"] = ties_table(np.float32)
    out["ties_signs_f64"] = ties_table(np.float64)
    out["z_int_min_and_range_f32"] = z_table(np.float32, 0.25)
    out["z_int_min_and_range_f64"] = z_table(np.float64, 0.25)
    out["z_int_min_and_range_nonintegral_f32"] = z_table(np.float32, 0.3)
    out["z_int_min_and_range_nonintegral_f64"] = z_table(np.float64, 0.3)
    out["multiplicity"] = multiplicity_table()
    out["shifts_289"] = shifts_289_table()
    return out


# ---- what every case is there for ------------------------------------------------------------------------------------------
def _rounds(g, name):
    """The recorded segments of a case with the restatement's keys: dicts of roi, ref / target columns and keys, shifts."""
    for tag, s, roi, peak, mode, ref, tgt, rel, d, W, H, sh in rs.golden_rounds(g, name):
        yield dict(tag=tag, s=s, roi=roi, mode=mode, ref=ref, tgt=tgt, rel=rel, d=d, W=W, H=H, sh=sh,
                   rk=rs.keys(mode, *ref, (0, 0, 0), d, W, H), tk=rs.keys(mode, *tgt, rel, d, W, H))


def _wrap_stats(r):
    """(pairs (target key, shift) whose exact sum leaves int32, per shift the matches by wrapped pairs, by the others)."""
    T, CT = np.unique(r["tk"], return_counts=True)
    U, C = np.unique(r["rk"], return_counts=True)
    exact = T.astype(np.int64)[:, None] + r["sh"].astype(np.int64)[None, :]
    wrapped = (exact > I_MAX) | (exact < I_MIN)
    q = (exact - I_MIN) % 2 ** 32 + I_MIN
    idx = np.minimum(np.searchsorted(U, q), len(U) - 1)
    m = np.where(U[idx] == q, np.minimum(CT[:, None], C[idx]), 0)
    return int(wrapped.sum()), (m * wrapped).sum(0), (m * ~wrapped).sum(0)


def _f32_sum(cols, rel, d, W):
    f = np.float32
    with np.errstate(invalid="ignore"):
        return np.rint((np.asarray(cols[0], f) + f(rel[0])) / f(d)) + np.rint((np.asarray(cols[1], f) + f(rel[1])) / f(d)) * f(W)


def check_wrap(g, name):
    side = "lo" if "_lo_" in name else "hi"
    rounds = list(_rounds(g, name))
    assert [r["s"] for r in rounds] == [1, 2] and all(r["mode"] == rs.XY_F64 for r in rounds)
    for r in rounds:
        S = int(np.abs(r["sh"].astype(np.int64)).max())
        assert len(r["sh"]) == 9 and S == 65537
        for k in (r["rk"], r["tk"]):
            assert (k.max() > I_MAX - S) if side == "hi" else (k.min() < I_MIN + S)
        n_wrap, by_wrap, by_rest = _wrap_stats(r)
        assert n_wrap >= 5
        only = (by_wrap > 0) & (by_rest == 0)                  # shifts whose count is there because of the wrap alone
        assert only.any() and np.array_equal(r["roi"][only], by_wrap[only]) and (r["roi"][only] > 0).all()
    # the reference keys span far less than the dense limit: both table forms are admissible
    assert all(int(r["rk"].max()) - int(r["rk"].min()) < 2 ** 17 for r in rounds)
    assert rounds[1]["rel"][:2] != (0, 0)


def check_wrap_f32(g, name):
    rounds = list(_rounds(g, name))
    assert [r["s"] for r in rounds] == [1, 2] and all(r["mode"] == rs.XY_F32 for r in rounds)
    assert np.array_equal(g[name + "/in_x"], g["wrap_hi_f64/in_x"].astype(np.float32))          # the same table
    assert np.array_equal(g[name + "/in_y"], g["wrap_hi_f64/in_y"].astype(np.float32))
    for r in rounds:
        for cols, rel, k in ((r["ref"], (0, 0), r["rk"]), (r["tgt"], r["rel"], r["tk"])):
            v = _f32_sum(cols, rel, r["d"], r["W"])
            up, below = v == np.float32(2 ** 31), (v < np.float32(2 ** 31)) & (v >= np.float32(2 ** 31 - 512))
            assert up.sum() >= 2 and below.sum() >= 2
            assert (k[up] == I_MIN).all() and (k[below] > I_MAX - 512).all()
            # the coordinates themselves are in range: only the float32 sum is not
            exact = np.rint(np.asarray(cols[0], np.float64)) + np.rint(np.asarray(cols[1], np.float64)) * 65536.0
            if tuple(rel[:2]) == (0, 0):
                assert (exact[up] <= I_MAX).all()
        n_wrap, by_wrap, by_rest = _wrap_stats(r)
        assert n_wrap >= 5 and (by_wrap > 0).any()              # wrapped pairs count here too
        assert int(r["rk"].max()) - int(r["rk"].min()) > 2 ** 31              # INT_MIN beside INT_MAX: sorted form only


def check_ties(g, name):
    rounds = list(_rounds(g, name))
    assert [r["s"] for r in rounds] == [1, 2]
    assert all(r["mode"] == (rs.XY_F32 if name.endswith("f32") else rs.XY_F64) for r in rounds)
    for r in rounds:
        for x, y, _ in (r["ref"], r["tgt"]):
            assert x.dtype == (np.float32 if name.endswith("f32") else np.float64)
            for v in (x, y):
                with np.errstate(invalid="ignore"):
                    u = v[np.isfinite(v)].astype(np.float64) / r["d"]
                    tie = u - np.floor(u) == 0.5
                    assert (tie & (np.floor(u) % 2 == 0)).any() and (tie & (np.floor(u) % 2 == 1)).any()
                    assert (tie & (u < 0)).any() and (tie & (u > 0)).any()
                    assert ((v == 0) & np.signbit(v)).any() and (v < 0).any()
                    assert (v == np.inf).any() and (v == -np.inf).any() and np.isnan(v).any()
            bad_x, bad_y = ~np.isfinite(x), ~np.isfinite(y)
            assert (bad_x & ~bad_y).any() and (~bad_x & bad_y).any() and (bad_x & bad_y).any()
            assert ((x == np.inf) & (y == -np.inf)).any()          # inf - inf: a NaN made by the key sum itself
        c = len(r["sh"]) // 2
        assert r["sh"][c] == 0
        both = min(int((r["rk"] == I_MIN).sum()), int((r["tk"] == I_MIN).sum()))
        others = rs.roi_cc(r["rk"][r["rk"] != I_MIN], r["tk"][r["tk"] != I_MIN], r["sh"])
        assert both >= 5 and r["roi"][c] == others[c] + both
    assert rounds[1]["rel"][:2] != (0, 0)


def check_z(g, name):
    rounds = list(_rounds(g, name))
    assert [r["s"] for r in rounds] == [1, 2]
    assert all(r["mode"] == (rs.Z_F32 if name.endswith("f32") else rs.Z_F64) for r in rounds)
    integral = "nonintegral" not in name
    for r in rounds:
        wh = r["W"] * r["H"]
        assert (wh == np.trunc(wh)) == integral and len(r["sh"]) == 5
        c = len(r["sh"]) // 2
        assert r["sh"][c] == 0.0 and r["sh"].dtype == np.float64
        assert np.isnan(r["ref"][2]).sum() >= 2 and np.isnan(r["tgt"][2]).sum() >= 2
        both = min(int((r["rk"] == I_MIN).sum()), int((r["tk"] == I_MIN).sum()))
        assert both >= 2 and r["roi"][c] >= both
        others = rs.roi_cc(r["rk"][r["rk"] != I_MIN], r["tk"][r["tk"] != I_MIN], r["sh"])
        assert r["roi"][c] == others[c] + both              # the INT_MIN keys match at shift 0.0
        v = r["tk"].astype(np.float64)[:, None] + r["sh"][None, :]
        assert (v > I_MAX).any() and (v < I_MIN).any()        # a shifted key leaves int32 on either side
        if integral:
            assert (np.delete(r["roi"], c) > 0).any()
        else:
            assert r["roi"][c] > 0 and not np.delete(r["roi"], c).any() and len(r["tk"]) < 100
    # a count array with its centre alone has its peak at 0: only the integral runs reach segment 2 with rel != 0
    assert (rounds[1]["rel"][2] != 0) == integral


def check_multiplicity(g, name):
    rounds = list(_rounds(g, name))
    assert [r["s"] for r in rounds] == [1, 2] and all(r["mode"] == rs.XY_F32 for r in rounds)
    for r in rounds:
        U, C = np.unique(r["rk"], return_counts=True)
        T, CT = np.unique(r["tk"], return_counts=True)
        j = int(np.argmax(r["roi"]))
        q = T.astype(np.int64) + int(r["sh"][j])
        hit = np.isin(q, U)
        cr, ct = C[np.searchsorted(U, q[hit])], CT[hit]
        seen = {(int(min(a, b)), int(np.sign(b - a))) for a, b in zip(cr, ct)}
        assert seen == {(c, sgn) for c in COUNTS for sgn in (-1, 0, 1)}
        assert r["roi"][j] == 3 * sum(COUNTS) and r["roi"].sum() == r["roi"][j]
        # the rows of the key with 257 are not contiguous: they meet the counter from several waves and blocks
        big = np.flatnonzero(r["tk"] == T[np.argmax(CT)])
        assert len(big) >= 257 and big.max() - big.min() > 768
    assert rounds[1]["rel"][:2] != (0, 0)


def check_shifts_289(g, name):
    rounds = list(_rounds(g, name))
    assert [r["s"] for r in rounds] == [1, 2] and all(r["mode"] == rs.XY_F32 for r in rounds)
    for r in rounds:
        assert len(r["sh"]) == 289 and len(np.unique(r["sh"])) == 289
    assert rounds[0]["roi"][256:].sum() > 0 and np.argmax(rounds[0]["roi"]) >= 272
    assert abs(rounds[1]["rel"][0]) > 1.0 and rounds[1]["roi"].max() > 0


def check(g, name):
    """Assert that the case `name` of the fixture `g` holds what it was built for."""
    n = sum(len(g[name + "/in_" + c]) for c in ("frame",))
    assert n <= 4200 and g[name + "/in_frame"].min() == 0
    if name.startswith("wrap_f32"):
        check_wrap_f32(g, name)
    elif name.startswith("wrap_"):
        check_wrap(g, name)
    elif name.startswith("ties_"):
        check_ties(g, name)
    elif name.startswith("z_"):
        check_z(g, name)
    elif name == "multiplicity":
        check_multiplicity(g, name)
    elif name == "shifts_289":
        check_shifts_289(g, name)
    else:
        raise AssertionError(f"no check for {name}")


# ---- minting -----------------------------------------------------------------------------------------------------------------
def mint_case(ns, cols, info, kw):
    """One round-1 call of the reference on the table -> the arrays of the case."""
    mk.STATE.update(rec=[], inputs={}, round=None, seg=None)
    frame = pd.Series(cols["frame"].astype(np.int64)) + 1
    first = frame <= SEG_LEN
    bounds = np.concatenate((np.arange(0, N_FRAMES, SEG_LEN), [N_FRAMES]))
    x, y = pd.Series(cols["x"]), pd.Series(cols["y"])
    d, roi_r, width, height, pixelsize = kw["intersect_d"], kw["roi_r"], info[0]["Width"], info[0]["Height"], info[0]["Pixelsize"]
    progress = mk._Lib.MockProgress()
    if "z" in cols:
        z = pd.Series(cols["z"])
        ns["intersection_max_z"](x, y, z, x[first], y[first], z[first], frame, bounds, d, roi_r, width, height, pixelsize,
                                 aim_round=1, progress=progress)
    else:
        ns["intersection_max"](x, y, x[first], y[first], frame, bounds, d, roi_r, width, aim_round=1, progress=progress)
    out = {"in_" + c: v for c, v in cols.items()}
    if "z" in cols:
        out.update(round_z1_x=cols["x"], round_z1_y=cols["y"], round_z1_z=cols["z"])
    out["info_in"] = np.array(json.dumps(info))
    out["kwargs"] = np.array(json.dumps(kw))
    rec = mk.STATE["rec"]
    out["rec_round"] = np.array([r[0] for r in rec])
    out["rec_seg"] = np.array([r[1] for r in rec], np.int64)
    out["rec_len"] = np.array([r[2].size for r in rec], np.int64)
    out["rec_roi"] = np.concatenate([r[2].ravel() for r in rec]).astype(np.int64)
    out["rec_peak"] = np.array([(tuple(r[3]) + (np.nan,))[:2] for r in rec], np.float64)
    return out


def mint():
    ns = mk.load_reference()
    arrays = {"case_names": np.array(list(cases().keys()))}
    for name, (cols, info, kw) in cases().items():
        for k, v in mint_case(ns, cols, info, kw).items():
            arrays[name + "/" + k] = v
    return arrays


def write(path, arrays):
    """An .npz with fixed time stamps, so that the same arrays give the same bytes."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED, compresslevel=9) as zf:
        for k, v in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(v), allow_pickle=False)
            zi = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            zi.compress_type = zipfile.ZIP_DEFLATED
            zi.external_attr = 0o644 << 16
            zf.writestr(zi, buf.getvalue(), compresslevel=9)


def main():
    arrays = mint()
    write(PATH, arrays)
    g = np.load(PATH)
    for name in g["case_names"]:
        name = str(name)
        check(g, name)
        print(f"{name}: {len(g[name + '/in_frame'])} rows, {len(g[name + '/rec_seg'])} segments counted, "
              f"{int(g[name + '/rec_len'][0])} shifts")
    print(f"{PATH}: {os.path.getsize(PATH)} bytes")


if __name__ == "__main__":
    main()
