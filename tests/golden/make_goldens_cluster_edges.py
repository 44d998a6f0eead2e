#!/usr/bin/env python3
"""Mint tests/golden/cluster_edge_cases.npz: the labels of the SMLM clusterer and DBSCAN on small tables that sit on
the edges of the device code: clamped cell coordinates, chains of maxima as long as the table, row counts around the
block size, large and negative corners, a flat dimension, one cell, a radius far below the spacing, the extreme
parameters, border rows at exactly the radius from two clusters, and frames on the thresholds of the frame analysis.

TEST INFRASTRUCTURE, build container only (needs the reference tree, scipy and sklearn).  The reference is loaded as
make_goldens_cluster.py loads it; nothing of it is stored here.

Every case stores ``kwargs`` and ``labels_cluster``, ``labels_cluster_fa`` (with the frame column), ``labels_dbscan``
(with ``db_min_locs``) and ``labels_dbscan_all``.  A case that owns its table stores ``in_columns`` and ``in_<column>``;
a case whose ``kwargs`` name a ``table`` (and ``rows``) takes the first ``rows`` rows of the columns stored under that
name.  All coordinates are float64.  3-D tables carry ``pixelsize = 1`` and ``radius_z = radius``, so z is used as it
stands.  A call that raises in the reference is recorded in ``edges``, as make_goldens_cluster.py does.

The script asserts what makes each case hard and prints the counts.  One condition differs between the two frame
counts of ``fa_thresholds``: with 1000 frames a mean frame of exactly 200 is not below 0.2 * 1000 and the site stays;
with 1013 frames the float64 product 0.2 * 1013 is 202.60000000000002, above the mean 2026 / 10 = 202.6, so the
reference discards the site whose mean is 1013 / 5 and keeps the one a single frame further in.  Both are recorded
and asserted as the reference has them.

Run:  python tests/golden/make_goldens_cluster_edges.py
"""
import json
import os
import sys

import numpy as np
import pandas as pd
from scipy.spatial import KDTree
from sklearn.cluster import DBSCAN

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _cluster_restate as rs  # noqa: E402  (only its table-to-points helper)
from make_goldens_cluster import load_reference, site_centres, sites  # noqa: E402

HAIR = 1.0 + 1.0 / 65536.0
CAP = {2: 2**31 - 2, 3: 2**21 - 2}
SIZES = (1, 2, 255, 256, 257, 511, 512, 513)
FA_FRAMES = {1000: np.uint32, 1013: np.int64}


def table(frame, pts, frame_dtype=np.uint32):
    pts = np.asarray(pts, np.float64)
    cols = {"frame": np.asarray(frame).astype(frame_dtype), "x": pts[:, 0].copy(), "y": pts[:, 1].copy()}
    if pts.shape[1] == 3:
        cols["z"] = pts[:, 2].copy()
    return cols


def kwargs(radius, min_locs, min_samples, db_min_locs, dims=2, **more):
    kw = dict(radius=radius, min_locs=min_locs, min_samples=min_samples, db_min_locs=db_min_locs, **more)
    if dims == 3:
        kw.update(radius_z=radius, pixelsize=1)
    return kw


def lattice(shape, r):
    """Row-major lattice of spacing r: the first axis is the slowest."""
    grid = np.meshgrid(*[np.arange(m) * r + 1.0 for m in shape], indexing="ij")
    return np.stack([g.ravel() for g in grid], axis=1)


def site_rows(rng, n_sites, per_site, sigma, r, n_frames=300):
    fr, pts, _ = sites(rng, site_centres(rng, n_sites, r), per_site, sigma, n_frames)
    return fr, pts


def clamp_table(rng, dims, r, extent):
    """20 sites over the extent, one in the far corner (clamped on every axis), one centred on the first clamped
    cell's lower edge on every axis at once and one per axis that straddles it on that axis alone."""
    edge = CAP[dims] * r * HAIR
    centres = rng.uniform(0, extent, (20, dims))
    centres[0] = 0.0                                  # the lower corner is a site too
    centres[1] = extent
    bulk = centres[np.repeat(np.arange(20), 30)] + rng.normal(0, 3e-4, (600, dims))
    lo = bulk.min(axis=0)
    straddle = [lo + edge]
    for k in range(dims):
        c = rng.uniform(0, extent, dims)
        c[k] = lo[k] + edge
        straddle.append(c)
    straddle = np.asarray(straddle)
    extra = straddle[np.repeat(np.arange(len(straddle)), 30)] + rng.normal(0, 3e-4, (30 * len(straddle), dims))
    pts = np.concatenate([bulk, extra])
    assert np.array_equal(pts.min(axis=0), lo)
    order = rng.permutation(len(pts))
    return rng.integers(0, 300, len(pts)), pts[order]


def border_groups(r):
    """Six groups: two 5-row cores, left and right of a border row that lies at exactly r from one row of each.
    The border row comes before, between or after the cores, and either core comes first.  All coordinates are
    multiples of 2^-6."""
    s = 2.0**-6
    core = np.array([[0, 0], [s, 0], [s, s], [s, -s], [2 * s, 0]])
    pts, border = [], []
    for g in range(6):
        origin = np.array([4.0 * g + 2.0, 3.0])
        left, right = origin + np.array([-r, 0]) - core, origin + np.array([r, 0]) + core
        first, second = (left, right) if g < 3 else (right, left)
        parts = [first, second]
        parts.insert(g % 3, origin[None])
        border.append(sum(len(p) for p in pts) + sum(len(p) for p in parts[:g % 3]))
        pts.extend(parts)
    return np.concatenate(pts), np.array(border)


def fa_table(rng, n_frames, frame_dtype):
    """One tight site per behaviour of the frame analysis, well apart, and six lone rows in the first frames (site -1:
    the rows without a label fail the analysis, to no effect); rows shuffled, the last row at n_frames - 1."""
    r = 0.05
    edges = np.linspace(0, n_frames, 21)
    first = np.ceil(edges).astype(np.int64)            # the first frame of every bin (the edge where it is a frame)
    spread = np.arange(-90, 100, 20)                   # 10 frames over several bins
    behaviours = {}

    def mean_site(total, move):
        f = total // 10 + spread
        f[-1] += total - f.sum()
        f[0] += move
        return f

    behaviours["mean_lo_at"] = mean_site(2 * n_frames, 0)
    behaviours["mean_lo_past"] = mean_site(2 * n_frames, -1)
    behaviours["mean_lo_inside"] = mean_site(2 * n_frames, 1)
    behaviours["mean_hi_at"] = mean_site(8 * n_frames, 0)
    behaviours["mean_hi_past"] = mean_site(8 * n_frames, 1)
    others = first[[4, 16, 6, 14, 8]] + 3
    for c in (5, 10, 15, 20, 25):
        for name, k in ((f"bin80_at_{c}", 4 * c // 5), (f"bin80_past_{c}", 4 * c // 5 + 1)):
            inside = np.linspace(first[10], first[11] - 1, k).astype(np.int64)
            behaviours[name] = np.concatenate([inside, others[:c - k]])
    behaviours["on_edges"] = np.r_[np.full(5, first[10]), np.full(4, first[11]), first[8]]
    behaviours["below_edge"] = np.r_[np.full(5, first[11] - 1), np.full(4, first[11]), first[8]]
    behaviours["on_edges_full"] = np.r_[np.full(9, first[10]), first[11]]
    behaviours["plain"] = np.linspace(50, n_frames - 50, 12).astype(np.int64)
    behaviours["last_frame"] = np.full(10, n_frames - 1)
    names = list(behaviours)
    frame = np.concatenate([behaviours[k] for k in names])
    site = np.repeat(np.arange(len(names)), [len(behaviours[k]) for k in names])
    centres = np.stack([3.0 * np.arange(len(names)) + 2, np.full(len(names), 5.0)], axis=1)
    pts = centres[site] + rng.normal(0, 0.1 * r, (len(site), 2))
    pts = np.concatenate([pts, np.stack([3.0 * np.arange(6) + 2, np.full(6, 9.0)], axis=1)])
    frame, site = np.r_[frame, np.arange(6)], np.r_[site, np.full(6, -1)]
    order = rng.permutation(len(site))
    last = np.flatnonzero(site[order] == names.index("last_frame"))[0]
    order[[last, -1]] = order[[-1, last]]
    assert 10 <= min(len(v) for k, v in behaviours.items() if "_5" not in k) and len(behaviours["bin80_at_5"]) == 5
    assert max(len(v) for v in behaviours.values()) <= 25 and frame.min() >= 0 and frame.max() == n_frames - 1
    return table(frame[order], pts[order], frame_dtype), site[order].astype(np.int32), names


def make_cases():
    rng = np.random.default_rng(20261021)
    tables, cases, extra = {}, {}, {}
    r = 0.125
    line = np.stack([np.arange(3000) * r + 1.0, np.full(3000, 2.0)], axis=1)
    fr = rng.integers(0, 300, 3000)
    tables["line_asc"], cases["line_asc"] = table(fr, line), kwargs(r, 2, 3, 2)
    tables["line_desc"], cases["line_desc"] = table(fr, line[::-1]), kwargs(r, 2, 3, 2)
    lat = lattice((40, 40), r)
    tables["lattice_rowmajor_2d"], cases["lattice_rowmajor_2d"] = table(rng.integers(0, 300, 1600), lat), kwargs(r, 4, 5, 0)
    lat3 = lattice((30, 30, 2), r)
    tables["lattice_rowmajor_3d"] = table(rng.integers(0, 300, 1800), lat3)
    cases["lattice_rowmajor_3d"] = kwargs(r, 4, 5, 0, dims=3)
    fr_s, pts_s = site_rows(rng, 12, 16, 0.3 * r, r)
    pts_s = pts_s[:200]
    for name, shift in (("offset_1e6", 1e6), ("offset_2p40", 2.0**40), ("offset_negative", -2.0**40 - 3)):
        pts = np.concatenate([lat + shift, pts_s + shift])
        assert np.array_equal((pts[:1600] - shift), lat) and np.array_equal(pts[:1600] * 8, np.round(pts[:1600] * 8))
        tables[name], cases[name] = table(np.r_[rng.integers(0, 300, 1600), fr_s[:200]], pts), kwargs(r, 4, 5, 0)
    fr, pts = clamp_table(rng, 3, 1e-3, 3000.0)
    tables["clamp_3d"], cases["clamp_3d"] = table(fr, pts), kwargs(1e-3, 8, 6, 10, dims=3)
    fr, pts = clamp_table(rng, 2, 1e-3, 1e7)
    tables["clamp_2d"], cases["clamp_2d"] = table(fr, pts), kwargs(1e-3, 8, 6, 10)
    r = 0.05
    fr, pts = site_rows(rng, 6, 30, 0.3 * r, r)
    pts = pts[:300]
    pts[:, 0] = 7.25
    tables["flat_x"], cases["flat_x"] = table(fr[:300], pts), kwargs(r, 8, 6, 10)
    tables["coincident"] = table(rng.integers(0, 300, 700), np.tile([[3.3, 4.7]], (700, 1)))
    cases["coincident"] = kwargs(r, 8, 6, 10)
    fr, pts = site_rows(rng, 6, 30, 0.3 * r, r)
    tables["one_cell"], cases["one_cell"] = table(fr[:300], pts[:300]), kwargs(1e6, 8, 6, 10)
    cases["tiny_radius"] = kwargs(1e-12, 8, 6, 10, table="one_cell", rows=300)
    fr, pts = site_rows(rng, 40, 8, 0.3 * r, r)
    pts[1] = pts[0] + np.array([0.25 * r, 0.0])          # the first two rows are neighbours
    tables["sizes"] = table(fr[:513], pts[:513])
    for n in SIZES:
        # one row is labelled only where a row alone is a maximum and a core: min_locs = 0, min_samples = 1
        cases[f"sizes_{n}"] = kwargs(r, 1, 2, 0, table="sizes", rows=n) if n > 1 else kwargs(r, 0, 1, 0, table="sizes", rows=n)
    fr, pts = site_rows(rng, 15, 20, 0.3 * r, r)
    tables["extremes"] = table(fr[:400], pts[:400])
    for min_locs, min_samples, db_min_locs in ((0, 1, 0), (1, 2, 1), (401, 401, 401), (5, 5, 0)):
        cases[f"extremes_{min_locs}_{min_samples}"] = kwargs(r, min_locs, min_samples, db_min_locs, table="extremes", rows=400)
    pts, border = border_groups(0.125)
    tables["border_exact"], cases["border_exact"] = table(rng.integers(0, 300, len(pts)), pts), kwargs(0.125, 4, 5, 0)
    extra["border_exact/border_rows"] = border.astype(np.int32)
    for n_frames, dt in FA_FRAMES.items():
        name = f"fa_thresholds_{n_frames}"
        tables[name], site, names = fa_table(rng, n_frames, dt)
        cases[name] = kwargs(0.05, 4, 3, 4)
        extra[name + "/site"], extra[name + "/site_names"] = site, np.array(names)
    return tables, cases, extra


# ---- what the cases hold, counted with the reference's own neighbour lists ----------------------------------------
def chained_maxima(X, r, min_locs):
    tree = KDTree(X)
    nb = tree.query_ball_tree(tree, r)
    cnt = np.array([len(v) for v in nb])
    lm = np.array([cnt[i] > min_locs and cnt[i] == max(cnt[nb[i]]) for i in range(len(X))])
    fresh = np.array([lm[i] and not any(lm[j] and j < i for j in nb[i]) for i in range(len(X))])
    return int(sum(lm[i] and not fresh[i] and not any(fresh[j] for j in nb[i]) for i in range(len(X))))


def clamp_counts(X, r, labels):
    """Per axis: the cell count the grid would need, and the labels with rows on both sides of the clamp coordinate."""
    dims = X.shape[1]
    lo, hi = X.min(axis=0), X.max(axis=0)
    cells = (hi - lo) / (r * HAIR) + 2
    u = (X - lo) / (r * HAIR)
    both = []
    for k in range(dims):
        clamped = u[:, k] >= CAP[dims]
        both.append(len(set(labels[clamped & (labels >= 0)]) & set(labels[~clamped & (labels >= 0)])))
    return cells, both, int((u >= CAP[dims]).all(axis=1).sum())


def check_border(X, r, min_samples, labels, border):
    db = DBSCAN(eps=r, min_samples=min_samples).fit(X)
    core = np.zeros(len(X), bool)
    core[db.core_sample_indices_] = True
    for b in border:
        d = X - X[b]
        at_r = np.flatnonzero((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] == r * r) & core)
        found = set(db.labels_[at_r])
        assert not core[b] and len(found) == 2 and labels[b] == min(found), (b, found, labels[b])
    first_core = [np.flatnonzero(core & (db.labels_ == c))[0] for c in range(db.labels_.max() + 1)]
    where = [int(np.searchsorted(np.sort([first_core[2 * g], first_core[2 * g + 1]]), b)) for g, b in enumerate(border)]
    assert where == [0, 1, 2, 0, 1, 2], where


def check_fa(out, name, n_frames):
    p = name + "/"
    site, names = out[p + "site"], [str(s) for s in out[p + "site_names"]]
    before, after = out[p + "labels_cluster"], out[p + "labels_cluster_fa"]
    assert (site == -1).sum() == 6 and (before[site == -1] == -1).all() and (before[site >= 0] >= 0).all()
    kept = {}
    for k, s in enumerate(names):
        rows = site == k
        assert rows.any() and len(set(before[rows])) == 1 and before[rows][0] >= 0, s
        assert len(set(after[rows])) == 1
        kept[s] = bool(after[rows][0] >= 0)
    stay = ["mean_lo_inside", "mean_hi_at", "on_edges", "below_edge", "plain"] + [f"bin80_at_{c}" for c in (5, 10, 15, 20, 25)]
    go = ["mean_lo_past", "mean_hi_past", "on_edges_full", "last_frame"] + [f"bin80_past_{c}" for c in (5, 10, 15, 20, 25)]
    # 0.2 * n_frames in float64 against the exact mean n_frames / 5
    (stay if 2 * n_frames / 10 >= 0.2 * n_frames else go).append("mean_lo_at")
    assert sorted(stay + go) == sorted(names)
    assert all(kept[s] for s in stay) and not any(kept[s] for s in go), kept
    return {"kept": sum(kept.values()), "discarded": len(kept) - sum(kept.values()), "mean_lo_at kept": kept["mean_lo_at"]}


def main():
    ref = load_reference()
    tables, cases, extra = make_cases()
    out, edges = dict(extra), {}
    out["case_names"] = np.array(list(cases))
    for name, cols in tables.items():
        out[name + "/in_columns"] = np.array(list(cols))
        for c, v in cols.items():
            out[f"{name}/in_{c}"] = v
    for name, kw in cases.items():
        p = name + "/"
        out[p + "kwargs"] = np.array(json.dumps(kw))
        n = kw.get("rows", len(tables[kw.get("table", name)]["x"]))
        assert n <= 3000
        cols = {c: v[:n] for c, v in tables[kw.get("table", name)].items()}
        Xc, Xd = rs.points(cols, kw)
        assert Xc.dtype == np.float64 and np.array_equal(Xc, Xd)
        r = kw["radius"]
        calls = {"labels_cluster": lambda: ref["_cluster"](Xc.copy(), r, kw["min_locs"]),
                 "labels_cluster_fa": lambda: ref["_cluster"](Xc.copy(), r, kw["min_locs"], pd.Series(cols["frame"])),
                 "labels_dbscan": lambda: ref["_dbscan"](Xd.copy(), r, kw["min_samples"], kw["db_min_locs"]),
                 "labels_dbscan_all": lambda: ref["_dbscan"](Xd.copy(), r, kw["min_samples"])}
        for key, call in calls.items():
            try:
                out[p + key] = call()
                assert out[p + key].dtype == np.int32 and out[p + key].shape == (n,)
            except Exception as e:  # noqa: BLE001
                edges[f"{name} {key}"] = {"raises": type(e).__name__}
        counts = {"clusters": int(out[p + "labels_cluster"].max() + 1), "kept by fa": len(np.unique(out[p + "labels_cluster_fa"])) - 1,
                  "dbscan": int(out[p + "labels_dbscan_all"].max() + 1)}
        if name not in ("tiny_radius", "extremes_401_401"):
            assert all((out[p + k] >= 0).any() for k in ("labels_cluster", "labels_dbscan", "labels_dbscan_all")), name
        else:
            assert all((out[p + k] == -1).all() for k in calls), name
        if name in ("line_asc", "line_desc", "lattice_rowmajor_2d"):
            counts["chained_maxima"] = chained_maxima(Xc, r, kw["min_locs"])
            assert counts["chained_maxima"] >= (1000 if name.startswith("lattice") else 2900)
        if name.startswith("clamp"):
            cells, both, corner = clamp_counts(Xc, r, out[p + "labels_cluster"])
            counts.update(cells=[float(c) for c in cells], clusters_across_clamp=both, rows_clamped_on_all_axes=corner)
            assert (cells > CAP[Xc.shape[1]]).all() and min(both) >= 1 and corner >= 30
            _, both_db, _ = clamp_counts(Xd, r, out[p + "labels_dbscan_all"])
            assert min(both_db) >= 1
        if name == "border_exact":
            check_border(Xd, r, kw["min_samples"], out[p + "labels_dbscan_all"], extra["border_exact/border_rows"])
        if name.startswith("fa_thresholds"):
            assert cols["frame"][-1] == cols["frame"].max() == int(name.split("_")[-1]) - 1
            counts.update(check_fa(out, name, int(name.split("_")[-1])))
        print(f"{name:22s} n={n:5d}", json.dumps(counts))
    print("edges", json.dumps(edges))
    out["edges"] = np.array(json.dumps(edges))
    path = os.path.join(HERE, "cluster_edge_cases.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes; cluster_cases.npz", os.path.getsize(os.path.join(HERE, "cluster_cases.npz")))
    assert os.path.getsize(path) < os.path.getsize(os.path.join(HERE, "cluster_cases.npz"))


if __name__ == "__main__":
    main()
