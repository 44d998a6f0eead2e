#!/usr/bin/env python3
"""Time the cluster combine (picasso_amd.postprocess.cluster_combine / cluster_combine_dist) stage by stage.

Device rows (default): the order (upload of the labels, two radix sorts, segment table), the statistics (upload of the
columns, one lane per segment), the distances (upload of the points, one workgroup per tile of a group), and the two
public calls as a whole; what a public call takes beyond its stages is download and frame assembly.  Shapes: a table
of ``--locs`` localizations in ``--clusters`` clusters in ``--groups`` groups, and the adversarial one for the
distances, a single group of ``--single`` clusters.  Each figure is the median of ``--repeats`` runs after one
warm-up.

Reference rows (``--reference DIR``, the tree that holds ``picasso/postprocess.py``; needs no device): the reference's
own two functions on the host, on tables of the same make, doubling the size until a call takes longer than
``--budget`` seconds; the largest size that finished within the budget is what the row records, nothing is
extrapolated.

One JSON line per row is appended to ``--out``.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import pandas as pd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def table(rng, n_locs, n_clusters, n_groups):
    """Localizations of ``n_clusters`` clusters spread over ``n_groups`` groups, rows interleaved."""
    which = rng.integers(0, n_clusters, n_locs)
    which[:n_clusters] = np.arange(n_clusters)                    # every cluster has a row
    centre = rng.uniform(0, 512, (n_clusters, 3))
    return pd.DataFrame({
        "frame": rng.integers(0, 60000, n_locs).astype(np.uint32),
        "x": (centre[which, 0] + rng.normal(0, 0.05, n_locs)).astype(np.float32),
        "y": (centre[which, 1] + rng.normal(0, 0.05, n_locs)).astype(np.float32),
        "z": (centre[which, 2] + rng.normal(0, 20, n_locs)).astype(np.float32),
        "photons": rng.uniform(200, 90000, n_locs).astype(np.float32),
        "group": (which % n_groups).astype(np.int32),
        "cluster": (which // n_groups).astype(np.int32)})


def median_ms(fn, repeats):
    fn()
    times = []
    for _ in range(repeats):
        t = time.perf_counter()
        fn()
        times.append((time.perf_counter() - t) * 1e3)
    return round(statistics.median(times), 3)


def device_rows(args):
    from picasso_amd import backend, postprocess
    rng = np.random.default_rng(1)
    rows = []
    for label, n_locs, n_clusters, n_groups in (("table", args.locs, args.clusters, args.groups),
                                                ("single group", args.single * 10, args.single, 1)):
        locs = table(rng, n_locs, n_clusters, n_groups)
        g, c = (postprocess._group_labels(locs[k].to_numpy()) for k in ("group", "cluster"))
        cols = {k: locs[k].to_numpy() for k in ("frame", "x", "y", "z", "photons")}
        pairs = [postprocess._average_pair(cols[a], cols["photons"]) for a in "xyz"]
        row = {"kind": "device", "shape": label, "locs": n_locs, "clusters": n_clusters, "groups": n_groups}
        row["order_ms"] = median_ms(lambda: backend.CombineGroups(g, c), args.repeats)
        groups = backend.CombineGroups(g, c)

        def stats():
            groups._cache.clear()
            backend.combine_stats(groups, [cols["frame"], cols["x"], cols["y"], cols["z"]], pairs)
        row["statistics_ms"] = median_ms(stats, args.repeats)
        row["cluster_combine_ms"] = median_ms(lambda: postprocess.cluster_combine(locs), args.repeats)
        combined = postprocess.cluster_combine(locs)
        cg, cc = (postprocess._group_labels(combined[k].to_numpy()) for k in ("group", "cluster"))
        points = np.ascontiguousarray(np.stack((combined["x"], combined["y"], combined["z"] / 130), axis=1), np.float64)
        row["dist_order_ms"] = median_ms(lambda: backend.CombineGroups(cg, cc), args.repeats)
        small = backend.CombineGroups(cg, cc)
        row["distances_ms"] = median_ms(lambda: backend.combine_min_distances(small, points), args.repeats)
        row["cluster_combine_dist_ms"] = median_ms(lambda: postprocess.cluster_combine_dist(combined), args.repeats)
        row["combine_assembly_ms"] = round(row["cluster_combine_ms"] - row["order_ms"] - row["statistics_ms"], 3)
        row["dist_assembly_ms"] = round(row["cluster_combine_dist_ms"] - row["dist_order_ms"] - row["distances_ms"], 3)
        rows.append(row)
    return rows


def reference_rows(args):
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    os.environ["PICASSO_REFERENCE"] = args.reference
    import make_goldens_combine as mk
    mk.POSTPROCESS_PY = os.path.join(args.reference, "picasso", "postprocess.py")
    ref = mk.load_reference()
    rng = np.random.default_rng(1)
    best = None
    n_locs = 10000
    while True:
        n_clusters, n_groups = max(n_locs // 10, 2), max(n_locs // 1000, 1)
        locs = table(rng, n_locs, n_clusters, n_groups)
        t = time.perf_counter()
        combined = ref["cluster_combine"](locs)
        t_combine = time.perf_counter() - t
        t = time.perf_counter()
        ref["cluster_combine_dist"](combined)
        t_dist = time.perf_counter() - t
        row = {"kind": "reference on the host", "locs": n_locs, "clusters": n_clusters, "groups": n_groups,
               "cluster_combine_s": round(t_combine, 3), "cluster_combine_dist_s": round(t_dist, 3)}
        print(row, flush=True)
        if max(t_combine, t_dist) > args.budget:
            break
        best = row
        n_locs *= 2
    return [dict(best, note=f"the largest size of the doubling at which both calls stay within {args.budget:g} s")] if best else []


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--locs", type=int, default=1000000)
    ap.add_argument("--clusters", type=int, default=100000)
    ap.add_argument("--groups", type=int, default=1000)
    ap.add_argument("--single", type=int, default=20000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--reference", default=None)
    ap.add_argument("--budget", type=float, default=60.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "combine_time.jsonl"))
    args = ap.parse_args()
    rows = reference_rows(args) if args.reference else device_rows(args)
    with open(args.out, "a") as f:
        for row in rows:
            print(json.dumps(row))
            f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
