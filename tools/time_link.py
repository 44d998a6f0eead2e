#!/usr/bin/env python3
"""Time picasso_amd.postprocess.link() and nena() on seeded tables (warm, median of 5, table in host memory as a
user passes it), with the stages of each call timed on their own.

  python tools/time_link.py [--sizes small,long,config4] [--repeats 5] [--out FILE]

small:   1.0e6 rows, 10 000 frames, 512 x 512 px, blinking sites
long:    the small table plus one emitter present in every frame (one component of 10 000 rows, replayed by one lane)
config4: 4.0e7 rows, 25 000 frames, 2048 x 2048 px (one config-4 rank's table)
Prints one JSON line per size (and appends it to --out)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import pandas as pd

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SIZES = {"small": (1_000_000, 10_000, 512), "long": (1_000_000, 10_000, 512), "config4": (40_000_000, 25_000, 2048)}


def table(n, frames, size, seed=1, long_component=False):
    """Sites that stay on for a few frames at a time: a row's site is on in runs of about five frames."""
    rng = np.random.default_rng(seed)
    events = max(n // 5, 1)
    ex = rng.uniform(1, size - 1, events).astype(np.float32)
    ey = rng.uniform(1, size - 1, events).astype(np.float32)
    start = rng.integers(0, frames - 8, events)
    e = rng.integers(0, events, n)
    fr = start[e] + rng.integers(0, 8, n)
    cols = {"frame": fr.astype(np.uint32),
            "x": ex[e] + rng.normal(0, 0.012, n).astype(np.float32),
            "y": ey[e] + rng.normal(0, 0.012, n).astype(np.float32)}
    for c, (lo, hi) in {"photons": (500, 9000), "sx": (0.8, 1.5), "sy": (0.8, 1.5), "bg": (5, 40), "lpx": (0.005, 0.06),
                        "lpy": (0.005, 0.06), "ellipticity": (0, 0.3), "net_gradient": (3000, 30000)}.items():
        cols[c] = rng.uniform(lo, hi, n).astype(np.float32)
    if long_component:
        every = rng.permutation(n)[:frames]
        cols["frame"][every] = np.arange(frames, dtype=np.uint32)
        cols["x"][every] = np.float32(size / 2) + rng.normal(0, 0.005, frames).astype(np.float32)
        cols["y"][every] = np.float32(size / 2) + rng.normal(0, 0.005, frames).astype(np.float32)
    locs = pd.DataFrame(cols)
    return locs.iloc[rng.permutation(n)].reset_index(drop=True)          # a user's table need not be sorted


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="small,long,config4")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from picasso_amd import backend, postprocess as pp
    torch.cuda.set_device(0)
    sync = torch.cuda.synchronize
    for name in a.sizes.split(","):
        n, frames, size = SIZES[name]
        print(f"{name}: making the table ...", file=sys.stderr, flush=True)
        locs = table(n, frames, size, long_component=(name == "long"))
        info = [{"Frames": frames, "Width": size, "Height": size, "Pixelsize": 130}]
        linked = pp.link(locs, info)                  # warm: library, allocator, scratch
        pp.nena(locs.copy(), info)
        rec = {"size": name, "rows": n, "frames": frames, "width": size, "events": int(len(linked))}
        rec["link_ms"], _ = median_ms(lambda: pp.link(locs, info), a.repeats, sync, "link_ms")
        rec["nena_ms"], _ = median_ms(lambda: pp.nena(locs.copy(), info), a.repeats, sync, "nena_ms")     # nena sorts in place
        # the stages, each on its own
        rec["host_sort_ms"], s = median_ms(lambda: locs.sort_values(kind="quicksort", by="frame"), a.repeats, sync, "host_sort_ms")
        group = np.zeros(n, np.int32)
        fr, x, y = s["frame"].to_numpy(), s["x"].to_numpy(), s["y"].to_numpy()
        rec["upload_ms"], t = median_ms(lambda: backend.LinkTable(fr, x, y, group), a.repeats, sync, "upload_ms")
        rec["link_groups_ms"], (d_lg, n_groups) = median_ms(lambda: t.link_groups(0.05 * 0.05, 4), a.repeats, sync, "link_groups_ms")
        rec["groups"] = int(n_groups)
        rec["combine_ms"], _ = median_ms(lambda: pp._combine(s, info, d_lg, n_groups, True), a.repeats, sync, "combine_ms")
        rec["histogram_ms"], h = median_ms(lambda: t.nena_hist(1.0, 0.001, 1000), a.repeats, sync, "histogram_ms")
        rec["nena_pairs"] = int(h.sum())
        centers = np.arange(0, 1.0, 0.001) + 0.0005
        lp = np.mean([np.median(s["lpx"]), np.median(s["lpy"])])
        rec["nena_fit_host_ms"], _ = median_ms(lambda: pp._nena_fit(centers, h.astype(np.float64), lp), a.repeats, sync, "nena_fit_host_ms")
        rec = {k: (round(v, 3) if isinstance(v, float) else v) for k, v in rec.items()}
        line = json.dumps(rec)
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as fh:
                fh.write(line + "\n")


if __name__ == "__main__":
    main()
