"""Time g5m() on a seeded synthetic table: 10^4 clusters of 20-200 rows, one to four molecules each.

Prints the device time of every round of the search (HIP events around the round's two kernels, as pmi_g5m_fit reports
them) and the wall time of the whole call, as one JSON line.  ``--host THREADS`` times the host-compiled core
(tests/g5m_host_driver.cpp) on that many threads for the same table instead: the only CPU figure there is.  No comparison
with numba's G5M has been measured.

    python tools/time_g5m.py [--clusters 10000] [--seed 1] [--host 16]
"""
import argparse
import ctypes
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np
import pandas as pd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from picasso_amd import _lib, backend, g5m  # noqa: E402


def table(n_clusters, seed):
    rng = np.random.default_rng(seed)
    sizes = rng.integers(20, 201, n_clusters)
    group = np.repeat(np.arange(n_clusters), sizes)
    n = len(group)
    mol = rng.integers(0, 4, n) % np.repeat(rng.integers(1, 5, n_clusters), sizes)
    cx = np.repeat(rng.uniform(5, 250, n_clusters), sizes) + 0.25 * mol
    cy = np.repeat(rng.uniform(5, 250, n_clusters), sizes)
    frame = np.concatenate([np.sort(rng.integers(0, 20000, s)) for s in sizes])
    return pd.DataFrame({"frame": frame.astype(np.uint32), "x": rng.normal(cx, 0.05).astype(np.float32),
                         "y": rng.normal(cy, 0.05).astype(np.float32), "lpx": np.full(n, 0.05, np.float32),
                         "lpy": np.full(n, 0.05, np.float32), "group": group.astype(np.int32)})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clusters", type=int, default=10000)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--host", type=int, default=0)
    args = ap.parse_args()
    locs = table(args.clusters, args.seed)
    info = [{"Frames": 20000, "Pixelsize": 130}]
    out = {"clusters": args.clusters, "rows": len(locs)}
    if args.host:
        so = os.path.join(tempfile.mkdtemp(), "g5m_host.so")
        subprocess.run([os.environ.get("CXX", "c++"), "-O2", "-std=c++17", "-shared", "-fPIC", "-ffp-contract=off", "-pthread", "-I",
                        os.path.join(ROOT, "picasso_amd", "csrc"), os.path.join(ROOT, "tests", "g5m_host_driver.cpp"), "-o", so], check=True)
        host = ctypes.CDLL(so)
        ids, rows, offsets = g5m.cluster_rows(locs, 10, np.inf)
        part = locs.iloc[rows]
        sizes = np.diff(offsets)
        caps = np.minimum(backend.G5M_MAX_K, sizes // 10)
        models = backend._g5m_empty(caps)
        tab, first, uniform = backend.g5m_table(sizes, caps)
        x, y = (np.ascontiguousarray(part[c].to_numpy(), np.float64) for c in ("x", "y"))
        lp = part[["lpx", "lpy"]].mean(axis=1).to_numpy().astype(np.float64)
        p = _lib.ptr
        t0 = time.perf_counter()
        host.g5m_host_fit(p(x), p(y), p(lp), p(offsets), ctypes.c_int64(len(sizes)), p(tab), p(first), p(uniform), None, 0, 10,
                          ctypes.c_double(0.8), ctypes.c_double(1.5), 3, 0, p(models.model), p(models.imodel), ctypes.c_int64(int(caps.sum())),
                          p(models.info), p(models.bic), args.host)
        out.update(host_threads=args.host, host_search_s=time.perf_counter() - t0, molecules=int(models.info[:, 1].sum()))
    else:
        rounds = []
        real = g5m.fit_clusters
        g5m._fit = lambda *a, **k: real(*a, **{**k, "progress": lambda r, n, ms: rounds.append({"round": r, "clusters": n, "device_ms": ms})})
        g5m.g5m(locs.iloc[:2000], info, callback_parent=None)      # warm-up: library load, scratch
        rounds.clear()
        t0 = time.perf_counter()
        centers, clustered, _ = g5m.g5m(locs, info, callback_parent=None, postprocess=False)
        out.update(call_s=time.perf_counter() - t0, device_ms=sum(r["device_ms"] for r in rounds), rounds=rounds, molecules=len(centers))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
