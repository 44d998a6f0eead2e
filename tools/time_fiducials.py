#!/usr/bin/env python3
"""Time the fiducial undrift (picasso_amd.postprocess.undrift_from_fiducials, csrc/fiducials.hip) and write
profiles/fiducials_timing.txt.

    python tools/time_fiducials.py [--picks 100] [--frames 100000] [--rows 1000000] [--out profiles/fiducials_timing.txt]

Milliseconds; 3 warm-up and 15 timed calls for the device figures, 1 and 5 for the host routes beside them.

  device        backend.fiducials_drift over x and y ALREADY ON THE DEVICE (float32, 95 % of the frames of every pick),
                between two device events on the call's stream; the events bracket the host work between the launches
                and the copy of the (Frames, 2) result.
  from host     the same call from host columns, host-timed around a synchronise: plus the uploads.
  numpy         the same drift by NumPy on the host, call for call what the reference's function does (nanmean,
                ma.average, interp); the reference tree itself is not needed for it.
  fused         the whole undrift_from_fiducials on a table of --rows float32 rows, 100 fiducials of radius 0.8 px.
  composed      picked_locs -> undrift_from_picked -> apply_drift on the same table: one pandas frame per pick.
  picked_locs   the first step of the composed route alone.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import time_picks as tp  # noqa: E402


def numpy_route(offsets, frame, columns, n_frames):
    out = []
    with np.errstate(all="ignore"):
        for c in columns:
            drift = np.full((len(offsets) - 1, n_frames), np.nan)
            for i, (a, b) in enumerate(zip(offsets[:-1], offsets[1:])):
                drift[i, frame[a:b]] = c[a:b] - np.mean(c[a:b])
            msd = np.nanmean((drift - np.nanmean(drift, 0)) ** 2, 1)
            mean = np.ma.average(np.ma.MaskedArray(drift, mask=np.isnan(drift)), axis=0, weights=1 / msd).filled(np.nan)
            nans = np.isnan(mean)
            mean[nans] = np.interp(nans.nonzero()[0], (~nans).nonzero()[0], mean[~nans])
            out.append(mean)
    return np.stack(out, axis=1)


def fiducial_table(rows, n_picks, n_frames, seed=3):
    """n_picks fiducials on a 10 x 10 lattice of a 64 x 64 px field, each in 90 % of the frames, over a background."""
    rng = np.random.default_rng(seed)
    picks = [(3.2 + 6.4 * (k % 10), 3.2 + 6.4 * (k // 10 % 10)) for k in range(n_picks)]
    frames, xs, ys = [], [], []
    for cx, cy in picks:
        f = np.flatnonzero(rng.random(n_frames) < 0.9)
        frames.append(f)
        xs.append(cx + 0.4 * f / n_frames + rng.normal(0, 0.1, len(f)))
        ys.append(cy - 0.3 * f / n_frames + rng.normal(0, 0.1, len(f)))
    n = max(rows - sum(len(f) for f in frames), 0)
    frames.append(rng.integers(0, n_frames, n))
    xs.append(rng.uniform(0, 64, n))
    ys.append(rng.uniform(0, 64, n))
    frame = np.concatenate(frames)
    order = np.argsort(frame, kind="stable")
    m = len(frame)
    cols = {"frame": frame[order].astype(np.uint32), "x": np.concatenate(xs)[order].astype(np.float32),
            "y": np.concatenate(ys)[order].astype(np.float32), "photons": rng.uniform(100, 5000, m).astype(np.float32),
            "lpx": rng.uniform(0.005, 0.05, m).astype(np.float32), "lpy": rng.uniform(0.005, 0.05, m).astype(np.float32)}
    return cols, [{"Width": 64, "Height": 64, "Frames": n_frames, "Pixelsize": 130}], picks


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--picks", type=int, default=100)
    ap.add_argument("--frames", type=int, default=100_000)
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fiducials_timing.txt"))
    a = ap.parse_args()
    import pandas as pd
    import torch
    from picasso_amd import backend, postprocess
    from _fiducials_cases import generated, same_bits
    lines = [f"Fiducial undrift on one MI355X (tools/time_fiducials.py).  Milliseconds; {tp.WARMUP} warm-up and {tp.TIMED} "
             "timed calls", "for the device figures, 1 and 5 for the host routes.", ""]
    offsets, frame, columns, F = generated(a.picks, a.frames, 0.95, seed=9)
    lines.append(f"fiducials_drift: {a.picks} picks x {F} frames, {offsets[-1]} member rows, x and y float32")
    d_off, d_frame = torch.from_numpy(offsets).cuda(), torch.from_numpy(frame).cuda()
    d_cols = [torch.from_numpy(c).cuda() for c in columns]
    lines.append(f"  device      {tp.summary(tp.event_timed(lambda: backend.fiducials_drift(d_off, d_frame, d_cols, F)))}")
    lines.append(f"  from host   {tp.summary(tp.host_timed(lambda: backend.fiducials_drift(offsets, frame, columns, F)))}")
    tp.WARMUP, tp.TIMED = 1, 5
    lines.append(f"  numpy       {tp.summary(tp.host_timed(lambda: numpy_route(offsets, frame, columns, F)))}")
    assert same_bits(numpy_route(offsets, frame, columns, F), backend.fiducials_drift(offsets, frame, columns, F))
    n_frames = 10_000
    cols, info, picks = fiducial_table(a.rows, 100, n_frames)
    df = pd.DataFrame(cols)

    def composed():
        picked = postprocess.picked_locs(df, info, picks, "Circle", pick_size=0.8, add_group=False)
        return postprocess.apply_drift(df.copy(), info, drift=postprocess.undrift_from_picked(picked, info))

    lines += ["", f"undrift_from_fiducials: {len(df)} float32 rows, {n_frames} frames, {len(picks)} picks of radius 0.8 px"]
    tp.WARMUP, tp.TIMED = 3, 15
    lines.append(f"  fused       {tp.summary(tp.host_timed(lambda: postprocess.undrift_from_fiducials(df, info, picks, 0.8)))}")
    tp.WARMUP, tp.TIMED = 1, 5
    lines.append(f"  composed    {tp.summary(tp.host_timed(composed))}")
    lines.append(f"  picked_locs {tp.summary(tp.host_timed(lambda: postprocess.picked_locs(df, info, picks, 'Circle', pick_size=0.8, add_group=False)))}")
    assert composed().equals(postprocess.undrift_from_fiducials(df, info, picks, 0.8)[0])
    text = "\n".join(lines) + "\n"
    with open(a.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
