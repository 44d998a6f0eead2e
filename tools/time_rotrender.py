"""Times the rotated views (csrc/render_rot.hip) on one GPU: 1e6 rows on a 512 x 512 camera-pixel field at oversampling 10
(a 5120 x 5120 image), generic angle, for the histogram and the projected Gaussian, next to the unrotated
``_render_gaussian`` on the same table.  "device": the ``_dev`` call on resident columns by device events (the Gaussian
forms synchronise once inside, so the figure holds that wait); "whole call": ``render._render_*`` on the DataFrame by the
host clock, uploads and the image's copy back included.  Warm-up and sample counts: time_picks.py's.

usage: python tools/time_rotrender.py [--rows N] [--field PX] [--oversampling F] [--out FILE]"""
import argparse
import os
import sys

import numpy as np
import pandas as pd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import time_picks as tp  # noqa: E402

ANG = (0.7, -0.4, 1.1)


def table(n, field, seed=0):
    """Clustered rows as tools/time_render.py's, with a depth of a tenth of the field and an axial precision."""
    rng = np.random.default_rng(seed)
    sites = rng.uniform(8, field - 8, (max(n // 100, 1), 3))
    pick = rng.integers(0, len(sites), n)
    f32 = lambda a: a.astype(np.float32)      # noqa: E731
    return pd.DataFrame({"frame": np.sort(rng.integers(0, 10000, n)).astype(np.uint32),
                         "x": f32(sites[pick, 0] + rng.normal(0, 0.05, n)), "y": f32(sites[pick, 1] + rng.normal(0, 0.05, n)),
                         "z": f32((sites[pick, 2] - field / 2) * 0.1 + rng.normal(0, 0.1, n)),
                         "lpx": f32(rng.uniform(0.02, 0.08, n)), "lpy": f32(rng.uniform(0.02, 0.08, n)),
                         "lpz": f32(rng.uniform(0.04, 0.16, n))})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--field", type=int, default=512)
    ap.add_argument("--oversampling", type=float, default=10.0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from picasso_amd import _lib, backend, render
    locs = table(a.rows, a.field)
    osamp, view = a.oversampling, (0.0, 0.0, float(a.field), float(a.field))
    n_y, n_x = backend.render_dims(osamp, *view)
    m64, m32 = backend._rotation_matrices(render.to_rotation(ANG).as_matrix())
    d = {c: backend._to_device(locs[c].to_numpy()) for c in ("x", "y", "z", "lpx", "lpy", "lpz")}
    image = torch.empty((n_y, n_x), dtype=torch.float32, device="cuda")
    count = torch.zeros(1, dtype=torch.int64, device="cuda")
    p = backend._dptr
    stream = lambda: backend._stream(image.device)      # noqa: E731
    coords = (p(d["x"]), p(d["y"]), p(d["z"]), backend.LINK_F32)
    tail = (p(image), n_y, n_x, p(count))
    device = {
        "hist rotated": lambda: _lib.call("pmi_render_hist_rot_dev", *coords, a.rows, _lib.ptr(m64), osamp, *view, *tail, stream()),
        "gaussian rotated": lambda: _lib.call("pmi_render_gaussian_rot_dev", *coords, p(d["lpx"]), p(d["lpy"]), p(d["lpz"]), a.rows,
                                              _lib.ptr(m64), _lib.ptr(m32), osamp, *view, 0.0, 0, *tail, stream()),
        "gaussian unrotated": lambda: _lib.call("pmi_render_gaussian_dev", p(d["x"]), p(d["y"]), p(d["lpx"]), p(d["lpy"]), a.rows,
                                                osamp, *view, 0.0, 0, *tail, stream()),
    }
    whole = {
        "hist rotated": lambda: render._render_hist(locs, osamp, *view, ang=ANG),
        "gaussian rotated": lambda: render._render_gaussian(locs, osamp, *view, 0.0, ang=ANG),
        "gaussian unrotated": lambda: render._render_gaussian(locs, osamp, *view, 0.0),
    }
    lines = [f"Rotated views on one MI355X (tools/time_rotrender.py).  Milliseconds; {tp.WARMUP} warm-up and {tp.TIMED} timed calls.",
             f"{a.rows} float32 rows, {a.field} x {a.field} camera pixels, oversampling {osamp:g} ({n_y} x {n_x} image), ang = {ANG}", ""]
    with _lib.lock():
        for name, fn in device.items():
            lines.append(f"  device      {name:19s} {tp.summary(tp.event_timed(fn))}")
            if name == "gaussian rotated":
                lines.append(f"              (rows in view: {int(count.cpu()[0])})")
    for name, fn in whole.items():
        lines.append(f"  whole call  {name:19s} {tp.summary(tp.host_timed(fn))}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
