"""The cluster centers of picasso.clusterer.find_cluster_centers (picasso/clusterer.py:694-897) restated by another
method than the device's and than pandas': plain NumPy scalar loops for the Kahan and Welford chains, ``reduceat`` /
``diff`` for the events, a cross-product hull in Python.  TEST INFRASTRUCTURE; nothing of the reference is stored here.

pandas' arithmetic, as the loops below have it: ``group_mean`` / ``group_sum`` are a Kahan-compensated sum in the
column's floating type (integers as float64), NaN skipped, the compensation reset to 0 when it becomes NaN;
``group_var`` is Welford's update in float64 whatever the column, ddof 1, and a float32 column gets a float32 result.
"""
import numpy as np
import pandas as pd

MEAN_COLS = ("frame", "x", "y", "photons", "sx", "sy", "bg", "net_gradient")
STD_COLS = ("frame", "x", "y")


def runs(group):
    """(stable order, unique labels ascending, offsets of their runs in that order)."""
    group = np.asarray(group)
    order = np.argsort(group, kind="stable")
    gs = group[order]
    first = np.flatnonzero(np.r_[True, gs[1:] != gs[:-1]]) if len(gs) else np.zeros(0, np.int64)
    return order, gs[first], np.r_[first, len(gs)]


def kahan(values, mean=True):
    """Kahan sum (or mean) of one group's values in their own floating type, NaN skipped."""
    t = values.dtype.type
    s, c, n = t(0), t(0), 0
    with np.errstate(all="ignore"):
        for v in values:
            if v != v:
                continue
            n += 1
            y = v - c
            tt = s + y
            c = tt - s - y
            if c != c:
                c = t(0)
            s = tt
        if not mean:
            return s
        return s / t(n) if n else t(np.nan)


def welford_std(values):
    """float64 standard deviation (ddof 1) of one group's values by Welford's update, NaN skipped."""
    n, m, acc = 0, 0.0, 0.0
    with np.errstate(all="ignore"):
        for v in values.astype(np.float64):
            v = float(v)
            if v != v:
                continue
            n += 1
            old = m
            m = np.float64(m) + (np.float64(v) - old) / np.float64(n)
            acc = np.float64(acc) + (np.float64(v) - m) * (np.float64(v) - old)
        return np.sqrt(np.float64(acc) / np.float64(n - 1)) if n > 1 else np.float64(np.nan)


def floating(col):
    col = np.asarray(col)
    return col if col.dtype.kind == "f" else col.astype(np.float64)


def per_group(col, order, offsets, fn, dtype):
    vs = col[order]
    return np.array([fn(vs[a:b]) for a, b in zip(offsets[:-1], offsets[1:])], dtype=dtype)


def events(frame, group):
    """Binding events per group: run starts and frame differences above 3 in the column's own type, summed per run."""
    order, unique, offsets = runs(group)
    fs, gs = np.asarray(frame)[order], np.asarray(group)[order]
    new = np.ones(len(fs), np.int64)
    with np.errstate(over="ignore"):
        new[1:] = (gs[1:] != gs[:-1]) | (np.diff(fs) > 3)
    return np.add.reduceat(new, offsets[:-1])


def hull_area(x, y):
    """Area of the convex hull of float64 points: monotone chain on np.lexsort, shoelace about the first vertex; 0.0 for
    fewer than three vertices or collinear points."""
    pts = np.stack([np.asarray(x, np.float64), np.asarray(y, np.float64)], axis=1) + 0.0
    pts = pts[np.lexsort([pts[:, 1], pts[:, 0]])]
    if len(pts) < 3:
        return 0.0

    def cross(o, a, b):
        return (a[0] - o[0]) * (b[1] - o[1]) - (a[1] - o[1]) * (b[0] - o[0])

    twice = 0.0
    for side in (pts, pts[::-1]):
        st = []
        for p in side:
            while len(st) >= 2 and not cross(st[-2], st[-1], p) > 0.0:
                st.pop()
            st.append(p)
        for a, b in zip(st[:-1], st[1:]):
            twice += cross(pts[0], a, b)
    return abs(0.5 * twice) + 0.0


def centers(cols, pixelsize=None, hull3d=None):
    """The table of centers as a dict of arrays in the reference's column order.  ``cols``: the table's columns.
    ``hull3d``: the convexhull column of a 3-D table (a scipy call per cluster in the product and in the reference;
    not restated)."""
    has_z = "z" in cols
    group = np.asarray(cols["group"])
    order, unique, offsets = runs(group)
    n_locs = np.diff(offsets)
    mean_cols = list(MEAN_COLS) + (["z"] if has_z else [])
    std_cols = list(STD_COLS) + (["z"] if has_z else [])
    s = {}
    for c in mean_cols:
        col = floating(cols[c])
        s[c + "_mean"] = per_group(col, order, offsets, kahan, col.dtype)
    for c in std_cols:
        sd = per_group(np.asarray(cols[c]), order, offsets, welford_std, np.float64)
        s[c + "_std"] = sd.astype(np.float32) if np.asarray(cols[c]).dtype == np.float32 else sd
    with np.errstate(all="ignore"):
        lpx = s["x_std"] / np.sqrt(n_locs)
        lpy = s["y_std"] / np.sqrt(n_locs)
        ellipticity = s["sx_mean"] / s["sy_mean"]
        f32 = np.float32
        out = {"frame": s["frame_mean"].astype(f32), "std_frame": s["frame_std"].astype(f32), "x": s["x_mean"].astype(f32),
               "y": s["y_mean"].astype(f32), "std_x": s["x_std"].astype(f32), "std_y": s["y_std"].astype(f32)}
        if has_z:
            w = 1.0 / (np.asarray(cols["lpx"]) + np.asarray(cols["lpy"])) ** 2
            zw = np.asarray(cols["z"]) * w
            wz = per_group(zw, order, offsets, lambda v: kahan(v, False), zw.dtype)
            ws = per_group(w, order, offsets, lambda v: kahan(v, False), w.dtype)
            out["z"] = (wz / ws).astype(f32)
        out.update({"photons": s["photons_mean"].astype(f32), "sx": s["sx_mean"].astype(f32), "sy": s["sy_mean"].astype(f32),
                    "bg": s["bg_mean"].astype(f32), "lpx": lpx.astype(f32), "lpy": lpy.astype(f32)})
        if has_z:
            out["lpz"] = (s["z_std"] / np.sqrt(n_locs)).astype(f32)
            out["std_z"] = s["z_std"].astype(f32)
        out.update({"ellipticity": ellipticity.astype(f32), "net_gradient": s["net_gradient_mean"].astype(f32),
                    "n_locs": n_locs.astype(np.uint32), "n_events": events(cols["frame"], group).astype(np.int32)})
        if has_z:
            out["volume"] = (np.power((s["x_std"] + s["y_std"] + s["z_std"] / pixelsize) / 3 * 2, 3) * 4.18879).astype(f32)
            out["convexhull"] = np.asarray(hull3d, f32)
        else:
            out["area"] = (np.power(s["x_std"] + s["y_std"], 2) * np.pi).astype(f32)
            xs, ys = np.asarray(cols["x"])[order], np.asarray(cols["y"])[order]
            out["convexhull"] = np.array([hull_area(xs[a:b], ys[a:b]) for a, b in zip(offsets[:-1], offsets[1:])]).astype(f32)
    out["group"] = unique.astype(np.int32)
    if "group_input" in cols:
        gi = np.asarray(cols["group_input"])[order]
        out["group_input"] = gi[offsets[:-1]].astype(np.int32)
    return out, order


def table(cols):
    return pd.DataFrame(cols)
