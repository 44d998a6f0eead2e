#!/usr/bin/env python3
"""Time the Fourier ring correlation (picasso_amd.postprocess._frc, csrc/frc.hip) and record its parity.

    python tools/time_frc.py             # GPU: whole _frc call and its kernels at image sides 1001 and 4001
    python tools/time_frc.py --cpu       # CPU: NumPy's single-precision fft2 and the per-radius mask loop of radial_sum
    python tools/time_frc.py --parity    # GPU: err_L(D), err_L(T), err_L(R) per golden case -> profiles/frc_parity.md

Rows are appended to profiles/frc_time.jsonl; profiles/frc_time.md is rewritten from every row of that file.  The table
is 1.0e6 rows of blinking sites (seed 7) on a 64 x 64 pixel field; the localization precision is chosen so that the
render has the wanted side.  The smoothing is replaced by the identity when statsmodels is absent, and the row says so.
The CPU mode times the mask loop on 16 radii spread over the range and scales to all of them: the loop's cost per radius
does not depend on the radius (one full-image mask each)."""
import argparse
import json
import os
import sys
import time
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
PROFILES = os.path.join(ROOT, "profiles")
JSONL = os.path.join(PROFILES, "frc_time.jsonl")
FIELD = 64.0
SIDES = (1001, 4001)


def table(rows=1_000_000, seed=7):
    import pandas as pd
    rng = np.random.default_rng(seed)
    sites = rng.uniform(1, FIELD - 1, (rows // 50, 2))
    pts = np.repeat(sites, 50, axis=0) + rng.normal(0, 0.05, (rows, 2))
    return pd.DataFrame({"x": pts[:, 0].astype(np.float32), "y": pts[:, 1].astype(np.float32)})


def gpu_rows():
    from picasso_amd import masking, postprocess
    try:
        import statsmodels  # noqa: F401
        smoothing = "statsmodels"
    except ImportError:
        masking.loess_smooth = lambda arr, span=5: arr
        smoothing = "identity (statsmodels absent)"
    locs = table()
    half = len(locs) // 2
    out = []
    for side in SIDES:
        lp = 2 * FIELD / (side - 0.5)                  # ceil(oversampling * FIELD) = side
        viewport = ((0.0, 0.0), (FIELD, FIELD))
        seen = {}
        inner = postprocess._frc_curve

        def spy(im1, im2):
            res = inner(im1, im2)
            seen.update(res[2]["ms"])
            return res

        postprocess._frc_curve = spy
        whole = []
        for rep in range(4):                           # the first call makes the hipFFT plan
            t0 = time.perf_counter()
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                res = postprocess._frc(locs.iloc[:half], locs.iloc[half:], 130, lp, viewport)
            whole.append((time.perf_counter() - t0) * 1e3)
        postprocess._frc_curve = inner
        assert res[4][0].shape[0] == side, (res[4][0].shape, side)
        out.append({"what": "gpu", "side": side, "rows": len(locs), "first_call_ms": whole[0], "call_ms": min(whole[1:]),
                    "kernels_ms": dict(seen), "smoothing": smoothing})
    return out


def cpu_rows(radii=16):
    out = []
    rng = np.random.default_rng(7)
    for side in SIDES:
        image = rng.poisson(0.06, (side, side)).astype(np.float32)
        t0 = time.perf_counter()
        spectrum = np.fft.fftshift(np.fft.fft2(image))
        fft_ms = (time.perf_counter() - t0) * 1e3
        centre = side // 2
        y, x = np.ogrid[:side, :side]
        dist_sq = (x - centre) ** 2 + (y - centre) ** 2
        picked = np.linspace(0, centre, radii).astype(int)
        t0 = time.perf_counter()
        for radius in picked:
            np.sum(spectrum[(dist_sq >= radius ** 2) & (dist_sq < (radius + 1) ** 2)])
        loop_ms = (time.perf_counter() - t0) * 1e3
        out.append({"what": "cpu", "side": side, "fft2_complex64_ms": fft_ms, "radial_sum_radii_timed": radii,
                    "radial_sum_scaled_ms": loop_ms / radii * (centre + 1), "note": "radial_sum scaled from the radii timed; "
                    "_frc transforms twice and calls radial_sum three times"})
    return out


def parity():
    import _frc_restate as rs
    from picasso_amd import backend, masking
    G = np.load(os.path.join(ROOT, "tests", "golden", "frc_cases.npz"))
    lines = ["# FRC parity: distance of each curve from the longdouble truth L", "",
             "D: the device (float64 hipFFT), T: NumPy's float64 fft2, R: the reference's recorded curve (complex64).", "",
             "| case | n | err_L(D) | err_L(T) | err_L(R) |", "|---|---|---|---|---|"]
    for name, live in zip(G["case_names"], G["nondegenerate"]):
        name = str(name)
        m1, m2, n = G[name + "/masked1"], G[name + "/masked2"], int(G[name + "/n"])
        vp = G[name + "/viewport"]
        ims = [rs.render_hist(G[name + "/x"][G[f"{name}/idx{h}"]], G[name + "/y"][G[f"{name}/idx{h}"]], 8.0,
                              ((vp[0][0], vp[0][1]), (vp[1][0], vp[1][1]))) for h in "12"]
        out = backend.frc_arrays(ims[0], ims[1], masking.tukey_profile(n))
        assert out["images"][0].tobytes() == m1.tobytes() and out["images"][1].tobytes() == m2.tobytes(), name
        if not live:
            assert not out["curve"].any()
            lines.append(f"| {name} | {n} | curve all zero | (an image without power) | |")
            continue
        L = rs.curve_L(m1, m2)
        lines.append(f"| {name} | {n} | {rs.err_L(out['curve'], L):.3g} | {rs.err_L(rs.curve_T(m1, m2), L):.3g} | "
                     f"{rs.err_L(G[name + '/R'], L):.3g} |")
    with open(os.path.join(PROFILES, "frc_parity.md"), "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


def write_md():
    rows = [json.loads(line) for line in open(JSONL)]
    lines = ["# FRC timing", "", "Written by tools/time_frc.py from profiles/frc_time.jsonl.  Milliseconds.", "",
             "## Device: `_frc` on 1.0e6 rows (two histogram renders, window, two float64 transforms, ring sums, curve)", "",
             "| side | first call (plan made) | call | window | transforms | ring sums | curve | smoothing |", "|---|---|---|---|---|---|---|---|"]
    for r in rows:
        if r["what"] == "gpu":
            k = r["kernels_ms"]
            lines.append(f"| {r['side']} | {r['first_call_ms']:.1f} | {r['call_ms']:.1f} | {k['window']:.3f} | {k['fft']:.3f} | "
                         f"{k['rings']:.3f} | {k['curve']:.3f} | {r['smoothing']} |")
    lines += ["", "## CPU: NumPy on one image (np.fft.fft2 of float32, and radial_sum's per-radius mask loop)", "",
              "| side | fft2 (complex64), one image | radial_sum, one call (scaled) | radii timed |", "|---|---|---|---|"]
    for r in rows:
        if r["what"] == "cpu":
            lines.append(f"| {r['side']} | {r['fft2_complex64_ms']:.1f} | {r['radial_sum_scaled_ms']:.0f} | {r['radial_sum_radii_timed']} |")
    lines += ["", "`_frc` on the CPU transforms two images and calls radial_sum three times.  The radial_sum column is the time of "
              "the radii timed, scaled to all n // 2 + 1 radii; the whole reference `_frc` was not run at these sides, and "
              "its renders were not timed.  The CPU rows are one process of a shared multi-core host, not the host of the MI355X; "
              "no speed-up is claimed beyond these rows."]
    with open(os.path.join(PROFILES, "frc_time.md"), "w") as f:
        f.write("\n".join(lines) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cpu", action="store_true")
    ap.add_argument("--parity", action="store_true")
    args = ap.parse_args()
    os.makedirs(PROFILES, exist_ok=True)
    if args.parity:
        return parity()
    rows = cpu_rows() if args.cpu else gpu_rows()
    with open(JSONL, "a") as f:
        for r in rows:
            f.write(json.dumps(r) + "\n")
            print(json.dumps(r))
    write_md()


if __name__ == "__main__":
    main()
