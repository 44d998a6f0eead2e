#!/usr/bin/env python3
"""Time picasso_amd.clusterer.cluster() and dbscan() on seeded tables (warm, median of 5, table in host memory as a
user passes it), with the stages of each call timed on their own.

  python tools/time_cluster.py [--sizes small,config4] [--repeats 5] [--out FILE]
  python tools/time_cluster.py --reference FILE.py [--sizes ref]      the reference's own _cluster / _dbscan on the CPU

small:   1.0e6 rows, 25 000 sites of 40 rows, 20 000 frames, 1024 x 1024 px
config4: 4.0e7 rows, 1 000 000 sites, 25 000 frames, 2048 x 2048 px (one config-4 rank's table)
ref:     1.0e5 rows of the same sites, for --reference (its Python loops take seconds at this size)
Prints one JSON line per size (and appends it to --out).  --reference needs no GPU: it takes ``_cluster``,
``_frame_analysis``, ``frame_analysis`` and ``_dbscan`` from the given clusterer.py (scipy and sklearn must import)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import pandas as pd

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SIZES = {"small": (25_000, 20_000, 1024), "config4": (1_000_000, 25_000, 2048), "ref": (2_500, 20_000, 324)}
RADIUS, MIN_LOCS, MIN_SAMPLES = 0.04, 10, 8


def table(n_sites, frames, size, per_site=40, seed=1):
    rng = np.random.default_rng(seed)
    cx, cy = rng.uniform(2, size - 2, n_sites), rng.uniform(2, size - 2, n_sites)
    which = rng.permutation(np.repeat(np.arange(n_sites), per_site))
    n = len(which)
    cols = {"frame": rng.integers(0, frames, n).astype(np.uint32),
            "x": (cx[which] + rng.normal(0, 0.012, n)).astype(np.float32),
            "y": (cy[which] + rng.normal(0, 0.012, n)).astype(np.float32)}
    for c, (lo, hi) in {"photons": (500, 9000), "sx": (0.8, 1.5), "sy": (0.8, 1.5), "bg": (5, 40), "lpx": (0.005, 0.06),
                        "lpy": (0.005, 0.06)}.items():
        cols[c] = rng.uniform(lo, hi, n).astype(np.float32)
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


def reference_functions(path):
    import ast
    from scipy.spatial import KDTree
    from sklearn.cluster import DBSCAN
    names = ("_frame_analysis", "frame_analysis", "_cluster", "_dbscan")
    ns = {"np": np, "pd": pd, "KDTree": KDTree, "DBSCAN": DBSCAN}
    keep = [n for n in ast.parse(open(path).read()).body if isinstance(n, ast.FunctionDef) and n.name in names]
    mod = ast.Module(body=[ast.ImportFrom("__future__", [ast.alias("annotations")], 0)] + keep, type_ignores=[])
    exec(compile(ast.fix_missing_locations(mod), path, "exec"), ns)
    return ns


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
    ap.add_argument("--reference", default=None, help="path of the reference's clusterer.py: time its functions on the CPU")
    a = ap.parse_args()
    sizes = (a.sizes or ("ref" if a.reference else "small,config4")).split(",")
    if a.reference:
        ref = reference_functions(a.reference)
        for name in sizes:
            locs = table(*SIZES[name])
            X = locs[["x", "y"]].to_numpy()
            rec = {"size": name, "rows": len(locs), "what": "the reference's own functions on this machine's CPU"}
            rec["ref_cluster_ms"], lab = median_ms(lambda: ref["_cluster"](X, RADIUS, MIN_LOCS), a.repeats, lambda: None, "_cluster")
            rec["ref_cluster_fa_ms"], _ = median_ms(lambda: ref["_cluster"](X, RADIUS, MIN_LOCS, locs["frame"]), a.repeats, lambda: None, "_cluster + frame analysis")
            rec["ref_dbscan_ms"], _ = median_ms(lambda: ref["_dbscan"](X, RADIUS, MIN_SAMPLES, MIN_LOCS), a.repeats, lambda: None, "_dbscan")
            rec["clusters"] = int(len(np.unique(lab[lab >= 0])))
            emit(rec, a.out)
        return
    import torch
    from picasso_amd import backend, clusterer as cl
    torch.cuda.set_device(0)
    sync = torch.cuda.synchronize
    for name in sizes:
        n_sites, frames, size = SIZES[name]
        print(f"{name}: making the table ...", file=sys.stderr, flush=True)
        locs = table(n_sites, frames, size)
        clustered = cl.cluster(locs, RADIUS, MIN_LOCS, True, return_info=True)[0]           # warm: library, allocator, scratch
        cl.dbscan(locs, RADIUS, MIN_SAMPLES, MIN_LOCS, return_info=True)
        rec = {"size": name, "rows": len(locs), "frames": frames, "width": size, "clustered_rows": int(len(clustered))}
        rec["cluster_ms"], _ = median_ms(lambda: cl.cluster(locs, RADIUS, MIN_LOCS, False, return_info=True), a.repeats, sync, "cluster_ms")
        rec["cluster_fa_ms"], _ = median_ms(lambda: cl.cluster(locs, RADIUS, MIN_LOCS, True, return_info=True), a.repeats, sync, "cluster_fa_ms")
        rec["dbscan_ms"], _ = median_ms(lambda: cl.dbscan(locs, RADIUS, MIN_SAMPLES, MIN_LOCS, return_info=True), a.repeats, sync, "dbscan_ms")
        # the stages, each on its own
        rec["host_copy_ms"], work = median_ms(lambda: locs.copy(), a.repeats, sync, "host_copy_ms")
        rec["host_points_ms"], X = median_ms(lambda: work[["x", "y"]].to_numpy(), a.repeats, sync, "host_points_ms")
        rec["host_finite_ms"], _ = median_ms(lambda: np.isfinite(X).all(), a.repeats, sync, "host_finite_ms")
        rec["upload_ms"], pts = median_ms(lambda: backend.ClusterPoints(X), a.repeats, sync, "upload_ms")
        rec["device_counts_ms"], _ = median_ms(lambda: pts.counts(RADIUS), a.repeats, sync, "device_counts_ms")
        rec["device_smlm_ms"], lab = median_ms(lambda: pts.smlm(RADIUS, MIN_LOCS), a.repeats, sync, "device_smlm_ms")
        fr = locs["frame"].to_numpy()
        rec["device_smlm_fa_ms"], _ = median_ms(lambda: pts.smlm(RADIUS, MIN_LOCS, fr, *cl._fa_limits(fr.max() + 1)), a.repeats, sync, "device_smlm_fa_ms")
        rec["device_dbscan_ms"], _ = median_ms(lambda: pts.dbscan(RADIUS, MIN_SAMPLES, MIN_LOCS), a.repeats, sync, "device_dbscan_ms")
        rec["host_extract_ms"], _ = median_ms(lambda: cl.extract_valid_labels(work, lab), a.repeats, sync, "host_extract_ms")
        rec["clusters"] = int(len(np.unique(lab[lab >= 0])))
        emit(rec, a.out)


if __name__ == "__main__":
    main()
