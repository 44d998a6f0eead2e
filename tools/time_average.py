#!/usr/bin/env python3
"""Time one iteration of the particle averaging at a realistic size (5 000 groups x 100 localizations,
display_pixel_size 5): the image, align and apply kernels by device events, the host share as the rest of the wall
clock of ``AverageAligner.iteration`` (uploads, downloads, the checks between the launches).

``--reference`` instead times the reference's own algorithm on this host, through the functions
tests/golden/make_goldens_average.py compiles from the reference tree, on ``--subset`` of the groups against the
average image of all of them, and scales the time to all groups (one process; the reference spreads the groups over
a pool, so divide by the workers it would have).  A statement of what the row buys, not a threshold.

Each run appends one JSON line to ``--out`` (default profiles/average_time.jsonl).
"""
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


def table(n_groups, per_group, seed=5):
    rng = np.random.default_rng(seed)
    pattern = np.array([[0.3 * np.cos(t), 0.3 * np.sin(t)] for t in (0, 2.1, 4.0)] + [[0.0, 0.0]])
    th = rng.uniform(0, 2 * np.pi, n_groups)
    which = rng.integers(0, len(pattern), (n_groups, per_group))
    p = pattern[which] + rng.normal(0, 0.04, (n_groups, per_group, 2))
    c, s = np.cos(th)[:, None], np.sin(th)[:, None]
    x = c * p[..., 0] - s * p[..., 1] + rng.uniform(5, 30, (n_groups, 1))
    y = s * p[..., 0] + c * p[..., 1] + rng.uniform(5, 30, (n_groups, 1))
    group = np.repeat(np.arange(n_groups), per_group)
    return pd.DataFrame({"x": x.reshape(-1).astype(np.float32), "y": y.reshape(-1).astype(np.float32),
                         "group": group.astype(np.int32)})


def state(locs, dps):
    from picasso_amd import average
    groups, order, offsets = average._group_order(locs["group"])
    locs = average._com_align(locs, order, offsets)
    r = 2 * np.sqrt((locs["x"] ** 2 + locs["y"] ** 2).mean())
    oversampling = 130 / dps
    angles = np.arange(0, 2 * np.pi, np.arcsin(1 / (oversampling * r)))
    return locs, (groups, order, offsets), r, oversampling, angles


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--groups", type=int, default=5000)
    ap.add_argument("--per-group", type=int, default=100)
    ap.add_argument("--dps", type=float, default=5.0)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--reference", action="store_true")
    ap.add_argument("--subset", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "average_time.jsonl"))
    a = ap.parse_args()
    locs, (groups, order, offsets), r, ov, angles = state(table(a.groups, a.per_group), a.dps)
    x, y = locs["x"].to_numpy().astype(np.float32), locs["y"].to_numpy().astype(np.float32)
    rec = {"groups": a.groups, "per_group": a.per_group, "display_pixel_size": a.dps, "angles": len(angles),
           "n_pixel": int(np.ceil(ov * (r + r)))}
    if a.reference:
        import make_goldens_average as mk
        ref = mk.load_reference()
        ref["compute_xcorr"] = ref["compute_xcorr_unwatched"]
        t0 = time.perf_counter()
        _, image = ref["render"].render_hist_numba(x, y, ov, -r, r)
        CF = np.conj(np.fft.fft2(image))
        t1 = time.perf_counter()
        for g in range(a.subset):
            ref["align_group_core"](order[offsets[g]:offsets[g + 1]], x, y, angles, ov, -r, r, CF, image.shape[0] / 2)
        t2 = time.perf_counter()
        rec.update(what="reference, one process", subset=a.subset, image_s=t1 - t0, per_group_s=(t2 - t1) / a.subset,
                   iteration_s_scaled=(t1 - t0) + (t2 - t1) / a.subset * a.groups, cpus=os.cpu_count())
    else:
        import torch
        from picasso_amd import backend
        aligner = backend.AverageAligner(locs["group"].to_numpy(), angles)
        aligner.iteration(x, y, ov, -r, r)                       # warm-up: code objects, allocations
        runs = []
        for _ in range(a.repeats):
            t0 = time.perf_counter()
            step = aligner.iteration(x, y, ov, -r, r)
            wall = (time.perf_counter() - t0) * 1e3
            runs.append({**step["ms"], "wall": wall, "host": wall - sum(step["ms"].values())})
        rec.update(what="device, one iteration", device=torch.cuda.get_device_name(0), chunks=step["chunks"], repeats=a.repeats,
                   chosen=int((step["choice"][:, 1] >= 0).sum()),
                   ms_median={k: float(np.median([q[k] for q in runs])) for k in runs[0]},
                   ms_min={k: float(np.min([q[k] for q in runs])) for k in runs[0]},
                   ms_max={k: float(np.max([q[k] for q in runs])) for k in runs[0]})
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "a") as f:
        f.write(json.dumps(rec) + "\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
