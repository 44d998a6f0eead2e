#!/usr/bin/env python3
"""Time picasso_amd.aim.aim() on seeded tables (warm, median of 5, table in host memory as a user passes it).

  python tools/time_aim.py [--sizes small,config4] [--repeats 5]

small:   1.0e6 rows, 10 000 frames, 512 x 512 px
config4: 4.0e7 rows, 25 000 frames, 2048 x 2048 px (one config-4 rank's table)
Prints one JSON line per size."""
import argparse
import json
import os
import sys
import time

import numpy as np
import pandas as pd

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SIZES = {"small": (1_000_000, 10_000, 512), "config4": (40_000_000, 25_000, 2048)}


def table(n, frames, size, seed=1):
    rng = np.random.default_rng(seed)
    sites = max(n // 50, 1000)
    sx = rng.uniform(1, size - 1, sites).astype(np.float32)
    sy = rng.uniform(1, size - 1, sites).astype(np.float32)
    fr = np.sort(rng.integers(0, frames, n)).astype(np.uint32)
    t = fr.astype(np.float32) / frames
    s = rng.integers(0, sites, n)
    x = sx[s] + np.float32(0.8) * np.sin(np.float32(3) * t) + rng.normal(0, 0.03, n).astype(np.float32)
    y = sy[s] - np.float32(0.6) * t + rng.normal(0, 0.03, n).astype(np.float32)
    return pd.DataFrame({"frame": fr, "x": x.astype(np.float32), "y": y.astype(np.float32)})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="small,config4")
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    import torch
    from picasso_amd import aim
    torch.cuda.set_device(0)
    for name in a.sizes.split(","):
        n, frames, size = SIZES[name]
        locs = table(n, frames, size)
        info = [{"Frames": frames, "Width": size, "Height": size, "Pixelsize": 130}]
        aim.aim(locs, info)                       # warm: library, plans, allocator
        ms = []
        for _ in range(a.repeats):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            aim.aim(locs, info)
            ms.append((time.perf_counter() - t0) * 1e3)
        print(json.dumps({"size": name, "rows": n, "frames": frames, "width": size, "segments": -(-frames // 100),
                          "ms_median": float(np.median(ms)), "ms_all": [round(v, 2) for v in ms]}), flush=True)


if __name__ == "__main__":
    main()
