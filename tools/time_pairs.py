#!/usr/bin/env python3
"""Time picasso_amd.postprocess.compute_local_density(), distance_histogram() and pair_correlation() on the seeded
tables of tools/time_cluster.py (warm, median of 5, table in host memory as a user passes it), with the stages of a
call timed on their own: the sanity filter, the block indices, the upload and sort (order), the kernels, the pandas
``iloc`` into block order.

  python tools/time_pairs.py [--sizes small] [--repeats 5] [--out FILE]
  python tools/time_pairs.py --restatement [--sizes small]      tests/golden/_pairs_restate.py on the CPU (no GPU)

Prints one JSON line per size (and appends it to --out).  The CPU figure is the test-side restatement (a SciPy k-d
tree and array operations), named as such: the reference's own loops need numba."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from time_cluster import SIZES, emit, median_ms, table  # noqa: E402

RADIUS, BIN_SIZE = 0.04, 0.001


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="small")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--restatement", action="store_true", help="time the test-side restatement on the CPU")
    a = ap.parse_args()
    for name in a.sizes.split(","):
        n_sites, frames, size = SIZES[name]
        print(f"{name}: making the table ...", file=sys.stderr, flush=True)
        locs = table(n_sites, frames, size)
        info = [{"Width": size, "Height": size, "Frames": frames}]
        rec = {"size": name, "rows": len(locs), "frames": frames, "width": size, "radius": RADIUS, "bin_size": BIN_SIZE}
        if a.restatement:
            sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
            import _pairs_restate as rs
            cols = {c: locs[c].to_numpy() for c in locs.columns}
            rec["what"] = "the test-side restatement (SciPy k-d tree, NumPy) on this machine's CPU"
            none = lambda: None      # noqa: E731
            rec["restate_density_ms"], (_, d) = median_ms(lambda: rs.local_density(cols, info[0], RADIUS), a.repeats, none, "density")
            rec["restate_hist_ms"], dh = median_ms(lambda: rs.distance_histogram(cols, info[0], BIN_SIZE, RADIUS), a.repeats, none, "histogram")
            rec["density_sum"], rec["pairs"] = int(d.sum()), int(dh.sum())
            emit(rec, a.out)
            continue
        import torch
        from picasso_amd import backend, lib, postprocess as pp
        torch.cuda.set_device(0)
        sync = torch.cuda.synchronize
        dens = pp.compute_local_density(locs, info, RADIUS)                     # warm: library, allocator, scratch
        dh = pp.distance_histogram(locs, info, BIN_SIZE, RADIUS)
        rec["density_sum"], rec["pairs"] = int(dens["density"].sum()), int(dh.sum())
        rec["density_ms"], _ = median_ms(lambda: pp.compute_local_density(locs, info, RADIUS), a.repeats, sync, "density_ms")
        rec["hist_ms"], _ = median_ms(lambda: pp.distance_histogram(locs, info, BIN_SIZE, RADIUS), a.repeats, sync, "hist_ms")
        rec["pair_correlation_ms"], _ = median_ms(lambda: pp.pair_correlation(locs, info, BIN_SIZE, RADIUS), a.repeats, sync, "pair_correlation_ms")
        # the stages, each on its own
        rec["host_sanity_ms"], sane = median_ms(lambda: lib.ensure_sanity(locs, info), a.repeats, sync, "host_sanity_ms")
        x, y = sane["x"].to_numpy(), sane["y"].to_numpy()
        rec["host_indices_ms"], (xi, yi) = median_ms(lambda: (np.uint32(x / RADIUS), np.uint32(y / RADIUS)), a.repeats, sync, "host_indices_ms")
        K, L = pp._index_blocks_shape(info, RADIUS)
        rec["upload_order_ms"], tab = median_ms(lambda: backend.BlockTable(xi, yi, K, L), a.repeats, sync, "upload_order_ms")
        rec["device_density_ms"], _ = median_ms(lambda: tab.density(x, y, RADIUS * RADIUS), a.repeats, sync, "device_density_ms")
        rec["device_hist_ms"], _ = median_ms(lambda: tab.distance_hist(x, y, RADIUS, RADIUS * RADIUS, BIN_SIZE, 40), a.repeats, sync, "device_hist_ms")
        order = tab.order()
        rec["host_iloc_ms"], _ = median_ms(lambda: sane.iloc[order], a.repeats, sync, "host_iloc_ms")
        rec["blocks"], rec["visible"] = [K, L], tab.p
        emit(rec, a.out)


if __name__ == "__main__":
    main()
