"""Mint tests/golden/g5m_edge_cases.npz: what the reference's own ``G5M_2D(K).fit`` gives on the seam clusters of
tests/_g5m_edge_cases.py (one cluster per size at which a wavefront or the workgroup of the device fit gets its first
idle lane or its first lane with two rows), for K = 1, 2 and 3.

The reference is loaded and perturbed as make_goldens_g5m.py does it, and the deviation is measured the same way: every
fit runs as it is, with every ``exp`` / ``log`` result moved by one ulp, and with every accumulation reversed; every
integer and every choice must be the same in all three runs, and 8 x the largest relative deviation of every float
quantity at these sizes is stored as ``tolerance/*``.  The tests compare within the tolerances of g5m_cases.npz; the ones
stored here say what the reference's own spread is at the seam sizes.  Only inputs and results are stored.

    python tests/golden/make_goldens_g5m_edges.py      # writes g5m_edge_cases.npz next to this file
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [HERE, os.path.dirname(HERE)]
import make_goldens_g5m as mk  # noqa: E402
import _g5m_edge_cases as ec  # noqa: E402

OUT = os.path.join(HERE, "g5m_edge_cases.npz")
MAX_BYTES = 1 << 20


def run_seam(ref, n, K):
    """The record of the reference's fit of K components on the seam cluster of n rows."""
    c = ec.seam(n)
    X = c.X
    m = ref["G5M_2D"](K, ec.MIN_LOCS, ec.BOUNDS).fit(X, lp=c.lp)
    return {ec.key(n, K) + k: v for k, v in mk.model_record(m, np.inf if m is None else m.bic(X)).items()}


def inputs(n):
    c = ec.seam(n)
    return {f"n{n}/in_{k}": getattr(c, k) for k in ("x", "y", "lp", "frame")}


def record(log=lambda *a: None):
    """Everything the file holds, by name."""
    refs = {mode: mk.load_reference(mode) for mode in ("plain", "ulp", "reversed")}
    out = {"seam_sizes": np.array(ec.SEAM_SIZES, np.int64), "seam_ks": np.array(ec.SEAM_KS, np.int64), "version": refs["plain"]["version"]}
    tol = {}
    for n in ec.SEAM_SIZES:
        out.update(inputs(n))
        for K in ec.SEAM_KS:
            runs = {mode: run_seam(ref, n, K) for mode, ref in refs.items()}
            for mode in ("ulp", "reversed"):
                mk.deviation(tol, runs["plain"], runs[mode], (n, K))
            out.update(runs["plain"])
            log(n, K, "valid", [int(v) for v in runs["plain"].get(ec.key(n, K) + "valid_idx", [])])
    for q, v in sorted(tol.items()):
        out["tolerance/" + q] = np.float64(8 * v)
        log(f"tolerance/{q} = 8 x {v:.3e}")
    return out


def main():
    np.savez_compressed(OUT, **record(print))
    assert os.path.getsize(OUT) <= MAX_BYTES, os.path.getsize(OUT)


if __name__ == "__main__":
    sys.exit(main())
