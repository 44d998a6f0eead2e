#!/usr/bin/env python3
"""Time picasso_amd.postprocess.nn_analysis() on the seeded table of tools/time_cluster.py (x / y of every row against
the table itself, warm, median of 5, coordinates in host memory as a user passes them) with k = 1 and k = 10, the
stages of a call timed on their own (upload, order, query, download), and the SPINNA shape: 1 000 calls of
picasso_amd.spinna.get_NN_dist() on 2 000 x 2 000 points, fresh every call and with one ordered set reused.  Beside each
stands the reference's own computation on this machine's CPU: scipy.spatial.KDTree(X2).query(X1, k), one thread; beside
the reused order, the queries of one KDTree built once.

  python tools/time_nn.py [--sizes small] [--repeats 5] [--calls 1000] [--out FILE] [--no-scipy]

Prints one JSON line per measurement (and appends it to --out)."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from time_cluster import SIZES, emit, median_ms, table  # noqa: E402


def scipy_query(X1, X2, k):
    from scipy.spatial import KDTree
    return KDTree(X2).query(X1, k=k)[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="small")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--calls", type=int, default=1000)
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-scipy", action="store_true")
    a = ap.parse_args()
    import torch
    from picasso_amd import backend, postprocess as pp, spinna
    torch.cuda.set_device(0)
    sync = torch.cuda.synchronize
    none = lambda: None      # noqa: E731
    for name in a.sizes.split(","):
        n_sites, frames, size = SIZES[name]
        print(f"{name}: making the table ...", file=sys.stderr, flush=True)
        locs = table(n_sites, frames, size)
        X = np.ascontiguousarray(np.stack([locs["x"].to_numpy(), locs["y"].to_numpy()], axis=1))
        for k in (1, 10):
            rec = {"what": "nn_analysis(X, X, k)", "size": name, "rows": len(X), "dtype": str(X.dtype), "k": k}
            got = pp.nn_analysis(X, X, k)                                       # warm: library, allocator, scratch
            rec["nn_analysis_ms"], _ = median_ms(lambda: pp.nn_analysis(X, X, k), a.repeats, sync, "nn_analysis_ms")
            # the stages, each on its own (k + 1 neighbours: the self column)
            rec["host_checks_ms"], P = median_ms(lambda: (pp._kdtree_points(X), np.array_equal(X, X), np.isfinite(X).all())[0],
                                                 a.repeats, sync, "host_checks_ms")
            rec["upload_ms"], d_x = median_ms(lambda: torch.from_numpy(P).cuda(), a.repeats, sync, "upload_ms")

            def upload_and_read_back():             # the copy is complete when its last row is back on the host
                d = torch.from_numpy(P).cuda()
                return d, d[-1].cpu().numpy()
            rec["upload_read_back_ms"], (_, last) = median_ms(upload_and_read_back, a.repeats, sync, "upload_read_back_ms")
            assert np.array_equal(last, P[-1]) and np.array_equal(d_x[::9973].cpu().numpy(), P[::9973])
            rec["box_ms"], ext = median_ms(lambda: [(P[:, c].min(), P[:, c].max()) for c in range(2)], a.repeats, sync, "box_ms")
            box = ([ext[0][0], ext[1][0]], [ext[0][1], ext[1][1]])
            rec["order_ms"], index = median_ms(lambda: backend.KnnIndex(d_x, k + 1, box), a.repeats, sync, "order_ms")
            rec["query_ms"], d_out = median_ms(lambda: index.query_device(d_x, k + 1), a.repeats, sync, "query_ms")
            rec["download_ms"], out = median_ms(lambda: d_out.cpu().numpy(), a.repeats, sync, "download_ms")
            rec["grid"] = [int(index.grid.n[0]), int(index.grid.n[1])]
            assert np.array_equal(out[:, 1:], got)
            if not a.no_scipy:
                rec["scipy_ms"], want = median_ms(lambda: scipy_query(X, X, k + 1)[:, 1:], 1, none, "scipy_ms")
                rec["equal_bits"] = bool(np.array_equal(want, got))
                rec["scipy_over_device"] = rec["scipy_ms"] / rec["nn_analysis_ms"]
            emit(rec, a.out)
    # SPINNA: many small calls
    rng = np.random.default_rng(4)
    sets = [(rng.uniform(0, 5000, (2000, 2)), rng.uniform(0, 5000, (2000, 2))) for _ in range(8)]
    for k in (1, 4):
        rec = {"what": "get_NN_dist(2000 x 2, 2000 x 2, k)", "calls": a.calls, "k": k}
        spinna.get_NN_dist(*sets[0], k)
        sync()
        t0 = time.perf_counter()
        for c in range(a.calls):
            spinna.get_NN_dist(*sets[c % 8], k)
        sync()
        rec["fresh_ms"] = (time.perf_counter() - t0) * 1e3
        index = backend.KnnIndex(sets[0][1], k)
        t0 = time.perf_counter()
        for c in range(a.calls):
            index.query(sets[c % 8][0], k)
        sync()
        rec["reused_order_ms"] = (time.perf_counter() - t0) * 1e3
        if not a.no_scipy:
            t0 = time.perf_counter()
            for c in range(a.calls):
                scipy_query(*sets[c % 8], k)
            rec["scipy_ms"] = (time.perf_counter() - t0) * 1e3
            from scipy.spatial import KDTree
            tree = KDTree(sets[0][1])               # like for like with the reused order: one tree, queries only
            t0 = time.perf_counter()
            for c in range(a.calls):
                tree.query(sets[c % 8][0], k=k)
            rec["scipy_reused_tree_ms"] = (time.perf_counter() - t0) * 1e3
            rec["scipy_over_fresh"] = rec["scipy_ms"] / rec["fresh_ms"]
            rec["scipy_reused_over_reused"] = rec["scipy_reused_tree_ms"] / rec["reused_order_ms"]
        emit(rec, a.out)


if __name__ == "__main__":
    main()
