#!/usr/bin/env python3
"""Time pick_similar (picasso_amd.postprocess.pick_similar, csrc/similar.hip) and write profiles/similar_timing.txt.

    python tools/time_similar.py [--rows 1000000] [--picks 100] [--out profiles/similar_timing.txt]

The table is float32 rows on a 512 x 512 px field: 80 % of them in clusters of 40 rows (sigma 0.12 px) at uniform
positions, the rest a uniform background; the given picks are the centres of the first clusters, the pick diameter is 1 px
(a grid of 591 x 511 points).  Three figures, 3 warm-up and 15 timed calls each, milliseconds:

  device       backend.similar_shift over columns ALREADY ON THE DEVICE, between two device events on the call's stream:
               the gather into block order, the grid search, the copy of the four outputs to the host (the block order is
               built once, outside).  The events bracket the upload of the grid arrays too.
  filter       backend.similar_filter alone on the candidates of that call that passed the two ranges, host-timed.
  pick_similar the whole call, host-timed around a device synchronise: ensure_sanity, the block indices and their
               upload and order, the members and statistics of the given picks, the grid search, the ranges, the filter.
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
WARMUP, TIMED = 3, 15


def summary(t):
    q = statistics.quantiles(t, n=4)
    return f"median {statistics.median(t):8.2f}  IQR {q[0]:8.2f} .. {q[2]:8.2f}  min {min(t):8.2f}  max {max(t):8.2f}  n={len(t)}"


def host_timed(fn, sync):
    for _ in range(WARMUP):
        fn()
    t = []
    for _ in range(TIMED):
        sync()
        t0 = time.perf_counter()
        fn()
        sync()
        t.append((time.perf_counter() - t0) * 1e3)
    return t


def event_timed(fn):
    import torch
    for _ in range(WARMUP):
        fn()
    t = []
    for _ in range(TIMED):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        start.record()
        fn()
        stop.record()
        stop.synchronize()
        t.append(start.elapsed_time(stop))
    return t


def workload(rows, n_picks, side=512, seed=11):
    rng = np.random.default_rng(seed)
    per = 40
    n_clusters = int(rows * 0.8) // per
    centres = rng.uniform(1, side - 1, (n_clusters, 2))
    pts = np.repeat(centres, per, axis=0) + rng.normal(0, 0.12, (n_clusters * per, 2))
    pts = np.concatenate([pts, rng.uniform(0, side, (rows - len(pts), 2))])
    pts = np.clip(pts[rng.permutation(len(pts))], 0.0, side - 0.01).astype(np.float32)
    picks = [(float(x), float(y)) for x, y in centres[:n_picks]]
    return pts[:, 0].copy(), pts[:, 1].copy(), picks, [{"Width": side, "Height": side, "Frames": 100, "Pixelsize": 130}]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--picks", type=int, default=100)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "similar_timing.txt"))
    a = ap.parse_args()
    import pandas as pd
    import torch
    from picasso_amd import backend, postprocess
    from _similar_cases import rs
    x, y, picks, info = workload(a.rows, a.picks)
    d, r = 1.0, 0.5
    rng = np.random.default_rng(1)
    df = pd.DataFrame({"frame": np.sort(rng.integers(0, 100, a.rows)).astype(np.uint32), "x": x, "y": y,
                       "photons": rng.uniform(100, 5000, a.rows).astype(np.float32),
                       "lpx": rng.uniform(0.005, 0.05, a.rows).astype(np.float32),
                       "lpy": rng.uniform(0.005, 0.05, a.rows).astype(np.float32)})
    found = postprocess.pick_similar(df, info, picks, d)
    # the device call alone, with the bounds the whole call forms
    sane, offsets, rows, table = postprocess._circle_members(df, info, picks, r, with_table=True)
    n_locs = np.diff(offsets)
    gate = max(2, n_locs.mean() - 2.0 * n_locs.std())
    grid = rs.grid(info, d)
    d_x, d_y = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
    args = (*grid[:3], np.uint64(grid[3]), np.uint64(grid[4]), np.uint64(grid[5]), r * r, float(gate))
    cx, cy, n, spread = backend.similar_shift(table, d_x, d_y, *args)
    cand = np.flatnonzero((n >= gate) & (n <= n_locs.mean() + 2.0 * n_locs.std()))          # the count range alone: a superset
    px, py = [p[0] for p in picks], [p[1] for p in picks]
    lines = [f"pick_similar on one MI355X: {a.rows} float32 rows on a 512 x 512 px field (80 % in clusters of 40 rows), "
             f"{a.picks} given picks, d = 1 (tools/time_similar.py).",
             f"{len(cx)} grid points, {int((n > 0).sum())} of them past the gate and the first circle, {len(cand)} candidates in "
             f"the count range, {len(found) - len(picks)} picks found.",
             f"{WARMUP} warm-up and {TIMED} timed calls per figure, milliseconds.",
             "device = backend.similar_shift over columns already on the device, between two device events (gather, grid",
             "search, the copy of the four outputs; the block order is built outside); filter = backend.similar_filter",
             "alone on the candidates, host-timed; pick_similar = the whole call, host-timed around a synchronise.",
             "No reference time stands beside these: numba, and so the reference's production path, was not available,",
             "and the parent commit has no such call.  No per-kernel figure and no counters were collected.", "",
             f"device        {summary(event_timed(lambda: backend.similar_shift(table, d_x, d_y, *args)))}",
             f"filter        {summary(host_timed(lambda: backend.similar_filter(cx[cand], cy[cand], px, py, d * d, d), lambda: None))}",
             f"pick_similar  {summary(host_timed(lambda: postprocess.pick_similar(df, info, picks, d), torch.cuda.synchronize))}"]
    text = "\n".join(lines) + "\n"
    with open(a.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
