#!/usr/bin/env python3
"""Time the picked localizations (picasso_amd.postprocess.picked_locs, csrc/picks.hip) and write
profiles/picks_timing.txt.

    python tools/time_picks.py [--rows 1000000] [--picks 1000] [--out profiles/picks_timing.txt]

The table is uniform float32 rows on a 64 x 64 px field with the picks of tests/_picks_cases.generated (circles of
radius 1.5 px, squares of side 1.5 px, rectangles up to 8.5 px long and 1.2 px wide, polygons of 3 to 11 corners up to
4 px from their centre with every 11th left open; pick coordinates as Python float, np.float64 and int in turn).  Three
figures per shape, 3 warm-up and 15 timed calls each, milliseconds:

  device       the backend.picks_* call over columns ALREADY ON THE DEVICE, between two device events on the call's
               stream: for a circle the count pass, the scan, the copy of the total, the write pass and the copy of the
               result (the block order is built once, outside); for the box shapes also the cell kernel, the block order
               and the segmented sort.  The events bracket host work between the launches too.
  from host    the same call from host columns, host-timed around a device synchronise: plus the upload of x and y and,
               for a circle, the block order.
  picked_locs  the whole call, with the host's per-pick pandas copy, ``group`` and sort by frame.
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


def host_timed(fn):
    import torch
    for _ in range(WARMUP):
        fn()
    t = []
    for _ in range(TIMED):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
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


def resident_call(backend, rs, cols, info, picks, shape, size):
    """The backend call of this shape over device tensors, as a closure."""
    import torch
    if shape == "Circle":
        sane = rs.sane_rows(cols, info)
        xs, ys = cols["x"][sane], cols["y"][sane]
        table = backend.BlockTable(np.uint32(xs / size), np.uint32(ys / size), *rs.grid_shape(info, size))
        d_x, d_y = torch.from_numpy(xs).cuda(), torch.from_numpy(ys).cuda()
        args = ([float(p[0]) for p in picks], [float(p[1]) for p in picks], [rs.block_of(p[0], size) for p in picks],
                [rs.block_of(p[1], size) for p in picks], [rs.circle_flags(px, py, size) for px, py in picks],
                rs.radius_squared(size))
        return lambda: backend.picks_circle(table, d_x, d_y, *args)
    d_x, d_y = torch.from_numpy(cols["x"]).cuda(), torch.from_numpy(cols["y"]).cuda()
    if shape == "Square":
        b, f, _ = rs.square_plan(picks, size)
        return lambda: backend.picks_square(d_x, d_y, b, f)
    if shape == "Rectangle":
        b, f, c = rs.rectangle_plan(picks, size)
        X, Y = [X for X, _ in c], [Y for _, Y in c]
        return lambda: backend.picks_rectangle(d_x, d_y, b, f, X, Y)
    _, b, f, c = rs.polygon_plan(picks)
    offsets = np.r_[0, np.cumsum([len(X) for X, _ in c])].astype(np.int32)
    X, Y = np.array([v for X, _ in c for v in X], np.float64), np.array([v for _, Y in c for v in Y], np.float64)
    return lambda: backend.picks_polygon(d_x, d_y, b, f, offsets, X, Y)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--picks", type=int, default=1000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "picks_timing.txt"))
    a = ap.parse_args()
    from picasso_amd import backend, postprocess
    from _picks_cases import generated, mk, rs
    from test_gpu_picks import device_members
    lines = [f"picked_locs on one MI355X: {a.rows} float32 rows on a 64 x 64 px field, {a.picks} picks per shape "
             f"(tools/time_picks.py).", f"{WARMUP} warm-up and {TIMED} timed calls per figure, milliseconds.",
             "device = the backend.picks_* call over columns already on the device, between two device events;",
             "from host = the same call from host columns, host-timed around a synchronise (adds the uploads and, for a",
             "circle, the block order); picked_locs = the whole call with its per-pick pandas work.",
             "No reference time stands beside these: numba, and so the reference's production path, was not available.", ""]
    for shape in ("Circle", "Square", "Rectangle", "Polygon"):
        cols, info, picks, size = generated(shape, n=a.rows, n_picks=a.picks, seed=11)
        df = mk.frame(cols, None)
        offsets, rows = device_members(cols, info, picks, shape, size)
        lines.append(f"{shape:10s} {len(rows)} member rows in {len(offsets) - 1} picks")
        lines.append(f"{shape:10s} device       {summary(event_timed(resident_call(backend, rs, cols, info, picks, shape, size)))}")
        lines.append(f"{shape:10s} from host    {summary(host_timed(lambda: device_members(cols, info, picks, shape, size)))}")
        lines.append(f"{shape:10s} picked_locs  {summary(host_timed(lambda: postprocess.picked_locs(df, info, picks, shape, size)))}")
    text = "\n".join(lines) + "\n"
    with open(a.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
