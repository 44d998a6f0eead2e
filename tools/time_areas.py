#!/usr/bin/env python3
"""Time picasso_amd.clusterer.cluster_areas() on seeded clustered tables (warm, median of 5, table in host memory as a
user passes it), with the stages of the call timed on their own, beside the NumPy restatement of the reference's loop
(tests/golden/_areas_restate.py) on the host.

  python tools/time_areas.py [--sizes many,large] [--repeats 5] [--restate-groups N] [--out FILE]

many:   1.0e6 rows in 1.0e5 groups of 10 rows (images of a few dozen bins, at most a few hundred: the LDS path)
large:  3 000 groups of 300 rows, 3-D, images of some 45 x 45 x 20 bins (the scratch path)
The restatement is timed once on the same table, every group of it (or the first --restate-groups), on group-ordered
slices, i.e. without the reference's ``locs[locs["group"] == g]``, which alone is O(groups x rows); its time is printed
beside the device's.  Prints one JSON line per size (and appends it to --out)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import pandas as pd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))

SIZES = {"many": (100_000, 10, 2, 0.012), "large": (3_000, 300, 3, 0.05)}
INFO = [{"Pixelsize": 130}]


def table(n_groups, per_group, dims, sigma, seed=1):
    rng = np.random.default_rng(seed)
    side = max(64.0, (n_groups * 4.0) ** 0.5)
    centre = rng.uniform(2, side - 2, (n_groups, 2))
    which = rng.permutation(np.repeat(np.arange(n_groups), per_group))
    n = len(which)
    cols = {"x": (centre[which, 0] + rng.normal(0, sigma, n)).astype(np.float32),
            "y": (centre[which, 1] + rng.normal(0, sigma, n)).astype(np.float32)}
    if dims == 3:
        cols["z"] = (rng.uniform(-300, 300, n_groups)[which] + rng.normal(0, sigma * 130, n)).astype(np.float32)
    cols["lpx"] = rng.uniform(0.005, 0.02, n).astype(np.float32)
    cols["lpy"] = rng.uniform(0.005, 0.02, n).astype(np.float32)
    cols["group"] = which.astype(np.int32)
    return cols


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


def emit(rec, out):
    rec = {k: (round(v, 4) if isinstance(v, float) else v) for k, v in rec.items()}
    line = json.dumps(rec)
    print(line, flush=True)
    if out:
        with open(out, "a") as fh:
            fh.write(line + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="many,large")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--restate-groups", type=int, default=0, help="0: every group")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import _areas_restate as rs
    from picasso_amd import backend, clusterer as cl
    torch.cuda.set_device(0)
    sync = torch.cuda.synchronize
    for name in a.sizes.split(","):
        n_groups, per_group, dims, sigma = SIZES[name]
        print(f"{name}: making the table ...", file=sys.stderr, flush=True)
        cols = table(n_groups, per_group, dims, sigma)
        locs = pd.DataFrame(cols)
        quiet = lambda i: None  # noqa: E731
        got = cl.cluster_areas(locs, INFO, quiet)                       # warm: library, allocator
        rec = {"size": name, "rows": len(locs), "groups": n_groups, "dims": dims}
        rec["cluster_areas_ms"], _ = median_ms(lambda: cl.cluster_areas(locs, INFO, quiet), a.repeats, sync, "cluster_areas")
        # the stages, each on its own
        lp = rs.median_lp(cols)
        rec["host_median_lp_ms"], _ = median_ms(lambda: np.median(locs[["lpx", "lpy"]].mean(axis=1)), a.repeats, sync, "median lp")
        rec["device_order_ms"], groups = median_ms(lambda: backend.CenterGroups(cols["group"]), a.repeats, sync, "order")
        points = [cols[c] for c in (("x", "y", "z") if dims == 3 else ("x", "y"))]
        make = lambda: backend.AreaImages(backend.CenterGroups(cols["group"]), points, 130, lp / 2, lp / 2 * 2.5)  # noqa: E731
        rec["device_order_shape_ms"], images = median_ms(make, a.repeats, sync, "order + uploads + shapes")
        rec["device_images_ms"], _ = median_ms(images.areas, a.repeats, sync, "images")
        lds = int(backend.AREAS_LDS_BINS)
        rec["images_in_lds"] = int(((images.bins > 0) & (images.bins <= lds)).sum())
        rec["images_in_scratch"] = int((images.bins > lds).sum())
        rec["median_bins"], rec["max_bins"] = int(np.median(images.bins)), int(images.bins.max())
        # the restatement on the same table
        k = min(a.restate_groups or n_groups, n_groups)
        order = np.argsort(cols["group"], kind="stable")
        bounds = np.searchsorted(cols["group"][order], np.arange(k + 1))
        t0 = time.perf_counter()
        want = np.array([rs.cluster_area(rs.points(cols, order[bounds[i]:bounds[i + 1]], 130), lp) for i in range(k)], np.float32)
        rec["restate_groups"], rec["restate_ms"] = k, (time.perf_counter() - t0) * 1e3
        rec["restate_ms_per_group"] = rec["restate_ms"] / k
        rec["device_ms_per_group"] = rec["cluster_areas_ms"] / n_groups
        rec["equal_on_restated_groups"] = bool(np.array_equal(got.iloc[:k, 1].to_numpy(), want))
        emit(rec, a.out)


if __name__ == "__main__":
    main()
