#!/usr/bin/env python3
"""Time picasso_amd.clusterer.find_cluster_centers() on a seeded clustered table (warm, median of 5, table in host
memory as a user passes it), with the stages of the call timed on their own.

  python tools/time_centers.py [--sizes small,single] [--repeats 5] [--out FILE]
  python tools/time_centers.py --reference FILE.py [--sizes small]      the reference's own function on the CPU, one run

small:   1.0e6 rows, 25 000 sites of 40 rows, 20 000 frames, 1024 x 1024 px (the table of tools/time_cluster.py), with
         the site of every row as its group
single:  1.0e5 rows in ONE group: what a sequential chain costs on one lane
Prints one JSON line per size (and appends it to --out).  --reference needs no GPU: it takes ``find_cluster_centers``
and its helpers from the given clusterer.py (pandas and scipy must import)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import pandas as pd

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SIZES = {"small": (25_000, 40, 20_000, 1024), "single": (1, 100_000, 20_000, 1024)}
REFERENCE_NAMES = ("_aggregate_cluster_stats", "_count_binding_events", "_cluster_convex_hulls", "_weighted_z_means",
                   "find_cluster_centers")


def table(n_sites, per_site, frames, size, seed=1):
    rng = np.random.default_rng(seed)
    cx, cy = rng.uniform(2, size - 2, n_sites), rng.uniform(2, size - 2, n_sites)
    which = rng.permutation(np.repeat(np.arange(n_sites), per_site))
    n = len(which)
    cols = {"frame": rng.integers(0, frames, n).astype(np.uint32),
            "x": (cx[which] + rng.normal(0, 0.012, n)).astype(np.float32),
            "y": (cy[which] + rng.normal(0, 0.012, n)).astype(np.float32)}
    for c, (lo, hi) in {"photons": (500, 9000), "sx": (0.8, 1.5), "sy": (0.8, 1.5), "bg": (5, 40), "lpx": (0.005, 0.06),
                        "lpy": (0.005, 0.06), "net_gradient": (3000, 20000)}.items():
        cols[c] = rng.uniform(lo, hi, n).astype(np.float32)
    cols["group"] = which.astype(np.int32)
    return pd.DataFrame(cols)


def median_ms(fn, repeats, sync, what=""):
    out = None
    print(f"  timing {what or 'call'} ...", file=sys.stderr, flush=True)
    ms = []
    for _ in range(repeats):
        sync()
        t0 = time.perf_counter()
        out = fn()
        sync()
        ms.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ms)), out


def reference_function(path):
    import ast
    from scipy.spatial import ConvexHull, QhullError
    ns = {"np": np, "pd": pd, "ConvexHull": ConvexHull, "QhullError": QhullError}
    keep = [n for n in ast.parse(open(path).read()).body if isinstance(n, ast.FunctionDef) and n.name in REFERENCE_NAMES]
    mod = ast.Module(body=[ast.ImportFrom("__future__", [ast.alias("annotations")], 0)] + keep, type_ignores=[])
    exec(compile(ast.fix_missing_locations(mod), path, "exec"), ns)
    return ns["find_cluster_centers"]


def emit(rec, out):
    rec = {k: (round(v, 3) if isinstance(v, float) else v) for k, v in rec.items()}
    line = json.dumps(rec)
    print(line, flush=True)
    if out:
        with open(out, "a") as fh:
            fh.write(line + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default=None)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--reference", default=None, help="path of the reference's clusterer.py: time its function on the CPU")
    a = ap.parse_args()
    sizes = (a.sizes or ("small" if a.reference else "small,single")).split(",")
    if a.reference:
        fcc = reference_function(a.reference)
        for name in sizes:
            locs = table(*SIZES[name])
            rec = {"size": name, "rows": len(locs), "what": "the reference's own find_cluster_centers on this machine's CPU, one run"}
            rec["ref_centers_ms"], res = median_ms(lambda: fcc(locs), 1, lambda: None, "find_cluster_centers")
            rec["clusters"] = int(len(res))
            emit(rec, a.out)
        return
    import torch
    from picasso_amd import backend, clusterer as cl
    torch.cuda.set_device(0)
    sync = torch.cuda.synchronize
    for name in sizes:
        print(f"{name}: making the table ...", file=sys.stderr, flush=True)
        locs = table(*SIZES[name])
        centers = cl.find_cluster_centers(locs)                                   # warm: library, allocator, scratch
        rec = {"size": name, "rows": len(locs), "clusters": int(len(centers))}
        rec["centers_ms"], _ = median_ms(lambda: cl.find_cluster_centers(locs), a.repeats, sync, "centers_ms")
        # the stages, each on its own
        cols = {c: locs[c].to_numpy() for c in locs.columns}
        rec["host_columns_ms"], _ = median_ms(lambda: [locs[c].to_numpy() for c in locs.columns], a.repeats, sync, "host_columns_ms")
        rec["upload_ms"], _ = median_ms(lambda: [backend._to_device(v) for v in cols.values()], a.repeats, sync, "upload_ms")
        rec["device_order_ms"], groups = median_ms(lambda: backend.CenterGroups(cols["group"]), a.repeats, sync, "device_order_ms (upload of group included)")
        for c in cols:
            groups._dev(cols[c])                                                   # resident: the chains below are timed without their uploads
        rec["device_mean_f32_ms"], _ = median_ms(lambda: groups.stats([(backend.CENTERS_MEAN, cols["photons"], None, ("mean",))]), a.repeats, sync, "device_mean_f32_ms")
        rec["device_mean_std_f32_ms"], _ = median_ms(lambda: groups.stats([(backend.CENTERS_MEAN, cols["x"], None, ("mean", "std"))]), a.repeats, sync, "device_mean_std_f32_ms")
        rec["device_mean_std_u32_ms"], _ = median_ms(lambda: groups.stats([(backend.CENTERS_MEAN, cols["frame"], None, ("mean", "std"))]), a.repeats, sync, "device_mean_std_u32_ms")
        rec["device_events_ms"], _ = median_ms(lambda: groups.stats([(backend.CENTERS_EVENTS, cols["frame"], None, ())]), a.repeats, sync, "device_events_ms")
        every = [(backend.CENTERS_MEAN, cols[c], None, ("mean", "std") if c in cl._STD_COLS else ("mean",)) for c in cl._MEAN_COLS]
        every.append((backend.CENTERS_EVENTS, cols["frame"], None, ()))
        rec["device_all_stats_ms"], _ = median_ms(lambda: groups.stats(every), a.repeats, sync, "device_all_stats_ms")
        rec["device_hull_ms"], _ = median_ms(lambda: groups.hull_areas(cols["x"], cols["y"]), a.repeats, sync, "device_hull_ms")
        emit(rec, a.out)


if __name__ == "__main__":
    main()
