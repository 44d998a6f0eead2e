"""A NumPy restatement of AIM's intersection counts (picasso/aim.py:89-126, :275-397), written for the tests.

It follows the rules of DESIGN 8 N5 with another method than the reference: keys in the dtype arithmetic of the
round, the x86 float -> int32 cast, and per shift a searchsorted of the shifted unique target keys in the unique
reference keys (the reference concatenates and stable-argsorts per shift).  The tests check it against every
recorded roi_cc of tests/golden/aim_cases.npz, and the device against it on tables too large to store."""
import numpy as np

XY_F32, XY_F64, Z_F32, Z_F64 = 0, 1, 2, 3


def cvt_i32(v):
    """float -> int32 as x86 cvtt*: NaN and out-of-range values give INT_MIN."""
    v = np.asarray(v, np.float64)
    ok = (v >= -2147483648.0) & (v < 2147483648.0)
    out = np.full(v.shape, np.iinfo(np.int32).min, np.int64)
    out[ok] = np.trunc(v[ok]).astype(np.int64)
    return out.astype(np.int32)


def keys(mode, x, y, z, rel, d, W, H=0.0):
    rx, ry, rz = (tuple(rel) + (0.0, 0.0, 0.0))[:3]
    with np.errstate(invalid="ignore"):
        if mode == XY_F32:
            f = np.float32
            xu = np.rint((np.asarray(x, f) + f(rx)) / f(d))
            yu = np.rint((np.asarray(y, f) + f(ry)) / f(d))
            return cvt_i32(xu + yu * f(W))
        if mode == XY_F64:
            xu = np.rint((np.asarray(x, np.float64) + rx) / d)
            yu = np.rint((np.asarray(y, np.float64) + ry) / d)
            return cvt_i32(xu + yu * W)
        xy = np.rint(np.asarray(x, np.float64) / d) + np.rint(np.asarray(y, np.float64) / d) * W
        if mode == Z_F32:
            f = np.float32
            zu = np.rint((np.asarray(z, f) + f(rz)) / f(d))
            return cvt_i32(xy + ((zu * f(W)) * f(H)).astype(np.float64))
        zu = np.rint((np.asarray(z, np.float64) + rz) / d)
        return cvt_i32(xy + (zu * W) * H)


def shifts_xy(roi_r, d, width):
    u = int(np.ceil(roi_r / d))
    steps = np.arange(-u, u + 1)
    W = width / d
    return np.trunc(steps[:, None] + steps[None, :] * W).astype(np.int32).ravel(), len(steps)


def shifts_z(roi_r, d, width, height):
    u = int(np.ceil(roi_r / d))
    return np.arange(-u, u + 1).astype(np.int32) * (width / d) * (height / d)


def roi_cc(ref_keys, target_keys, shifts):
    """sum over keys of min(c_ref, c_target) per shift; int32 shifts add with wrap-around, float64 ones in float64."""
    U, C = np.unique(ref_keys, return_counts=True)
    T, CT = np.unique(target_keys, return_counts=True)
    out = np.zeros(len(shifts), np.int64)
    if len(U) == 0:
        return out
    for i, s in enumerate(shifts):
        if np.asarray(shifts).dtype == np.int32:
            q = ((T.astype(np.int64) + int(s) + 2 ** 31) % 2 ** 32 - 2 ** 31)
            ok = np.ones(len(q), bool)
        else:
            qd = T.astype(np.float64) + s
            ok = (qd == np.trunc(qd)) & (qd >= -2 ** 31) & (qd <= 2 ** 31 - 1)
            q = np.where(ok, qd, 0).astype(np.int64)
        idx = np.minimum(np.searchsorted(U, q), len(U) - 1)
        hit = ok & (U[idx] == q)
        out[i] = np.minimum(CT[hit], C[idx[hit]]).sum()
    return out


def golden_rounds(g, name):
    """Yield (tag, segment, roi_cc, peak, mode, ref cols, target cols, rel, d, W, H, shifts) for every recorded
    segment of one golden case, rebuilt from the columns each round started from."""
    import json
    p = name + "/"
    info = json.loads(str(g[p + "info_in"]))
    kw = json.loads(str(g[p + "kwargs"]))
    get = lambda k: next(d[k] for d in reversed(info) if k in d)  # noqa: E731
    width, height, pixelsize, n_frames = get("Width"), get("Height"), get("Pixelsize"), get("Frames")
    seg_len = kw.get("segmentation", 100)
    d = kw.get("intersect_d", 20 / 130)
    roi_r = kw.get("roi_r", 60 / 130)
    fr = g[p + "in_frame"]
    frame = fr + 1 - fr.min()
    bounds = np.concatenate((np.arange(0, n_frames, seg_len), [n_frames]))
    first = frame <= seg_len
    # the key mode follows the dtype of the columns, as in picasso_amd/aim.py (aim() itself: float32 in round 1, float64
    # after); a fixture of single rounds (aim_edge_cases.npz) stores only the rounds it ran
    single = lambda a: a.dtype == np.float32  # noqa: E731
    cols = {"xy1": (XY_F32 if single(g[p + "in_x"]) and single(g[p + "in_y"]) else XY_F64, g[p + "in_x"], g[p + "in_y"], None)}
    if p + "round_xy2_x" in g:
        cols["xy2"] = (XY_F64, g[p + "round_xy2_x"], g[p + "round_xy2_y"], None)
    if p + "round_z1_z" in g:
        zx, zy = g[p + "round_z1_x"], g[p + "round_z1_y"]
        z1 = g[p + "round_z1_z"] / pixelsize
        cols["z1"] = (Z_F32 if single(z1) else Z_F64, zx, zy, z1)
        if p + "round_z2_z" in g:
            cols["z2"] = (Z_F64, zx, zy, g[p + "round_z2_z"] / pixelsize)
    rounds, segs = g[p + "rec_round"], g[p + "rec_seg"]
    lens, peaks = g[p + "rec_len"], g[p + "rec_peak"]
    starts = np.concatenate(([0], np.cumsum(lens)))
    rel = {}
    for i, (tag, s) in enumerate(zip(rounds, segs)):
        tag = str(tag)
        mode, x, y, z = cols[tag]
        zmode = mode in (Z_F32, Z_F64)
        ref = first if tag.endswith("1") else np.ones(len(x), bool)
        tgt = (frame > bounds[s]) & (frame <= bounds[s + 1])
        sh = shifts_z(roi_r, d, width, height) if zmode else shifts_xy(roi_r, d, width)[0]
        r = rel.setdefault(tag, [0, 0, 0])
        pick = lambda m: (x[m], y[m], None if z is None else z[m])  # noqa: E731
        yield (tag, int(s), g[p + "rec_roi"][starts[i]:starts[i + 1]], peaks[i], mode, pick(ref), pick(tgt),
               ((0, 0, r[0]) if zmode else (r[0], r[1], 0)), d, width / d, height / d, sh)
        if zmode:
            r[0] += peaks[i][0]
        else:
            r[0] += peaks[i][0]
            r[1] += peaks[i][1]
