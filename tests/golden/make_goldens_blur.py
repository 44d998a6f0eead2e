#!/usr/bin/env python3
"""Mint tests/golden/blur_cases.npz: the reference's own ``_fftconvolve`` routes, ``_render_smooth``,
``_render_convolve``, ``find_fiducials``, ``align`` and ``align_rcc`` on small tables.

TEST INFRASTRUCTURE, build container only (needs the reference tree, scipy and pandas; no numba).  ``render.py``,
``imageprocess.py`` and ``localize.py`` are executed from where they lie behind the stand-ins of _refshim.py; ``align``,
``align_rcc`` and ``minimize_shifts`` are compiled in memory from ``postprocess.py`` / ``lib.py`` (the loader of
make_goldens_postprocess.py), ``picked_locs`` by the loader of make_goldens_picks.py.  Nothing of the reference is
stored but inputs and results.

Every coordinate of a table lies on the 1/64 lattice and every viewport bound is a dyadic number, so the float32
arithmetic of the shim's NumPy run and the float64 arithmetic of numba's compiled run place every row in the same pixel.

Contents.
  plan/*        (n_y, n_x, blur_width, blur_height) -> the route ``_fftconvolve`` took (which of scipy's two functions it
                called, recorded by wrapping them), the sigmas it passed and the weights scipy made of them, or the window
                functions, or what it raised;
  fft/*         per direct-route case of _blur_restate.DIRECT_CASES: max |reference - float64 direct sum| / max |reference|,
                and ``c`` = four times the largest of them;
  signatures    JSON, ``str(inspect.signature(...))`` of the reference's functions;
  render/*      tables, calls and the reference's (n, image);
  fiducials/*   table, info and the reference's (picks, box), or what it raised;
  align/*       three channels and the reference's shifts, iteration count and shifted columns.

Run:  python tests/golden/make_goldens_blur.py
"""
import inspect
import json
import os
import sys
import warnings
from copy import deepcopy

import numpy as np
import pandas as pd

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _blur_restate as rs  # noqa: E402
import _refshim  # noqa: E402
import make_goldens_picks as mkp  # noqa: E402
from make_goldens_postprocess import functions_from  # noqa: E402

REF = _refshim.REF
NAN = float("nan")
PLAN_CASES = [
    # the route flips between sides 220 and 221 at sigma 1, each axis on its own
    (220, 1000, 1, 1), (221, 1000, 1, 1), (1000, 220, 1, 1), (1000, 221, 1, 1), (221, 221, 1, 1), (220, 220, 1, 1),
    # ... and between 2020 and 2021 at kernel 101
    (2020, 3000, 10, 10), (2021, 3000, 10, 10), (3000, 2020, 10, 10), (3000, 2021, 10, 10), (2021, 2021, 10.49, 10.49),
    # kernels are 10 k + 1: the first one above 101 is 111, which no image size brings back to the spatial route
    (5000, 5000, 11, 1), (5000, 5000, 1, 11), (100000, 100000, 10.5, 1),
    # np.round is half to even: 0.5 -> 0, 1.5 -> 2, 2.5 -> 2; round == 0 gives kernel 1
    (500, 500, 0.5, 0.5), (500, 500, 1.5, 1.5), (500, 500, 2.5, 2.5), (500, 500, 0.4, 0.3), (4, 4, 0.4, 0.4), (30, 30, 0.5, 2.5),
    # sigmas of exactly 0 and of 1e-16 are skipped; 1e-15 is skipped too (<=), 2e-15 is not
    (300, 300, 0, 1), (300, 300, 1, 0), (300, 300, 0, 0), (300, 300, 1e-16, 1), (300, 300, 1e-15, 1e-16), (300, 300, 2e-15, 1),
    # float32 widths, as _render_convolve makes them
    (256, 256, np.float32(0.3), np.float32(1.2)), (64, 80, np.float32(0.3), np.float32(1.2)),
    # what cannot be rounded
    (300, 300, NAN, 1), (300, 300, 1, NAN), (300, 300, float("inf"), 1),
]


def tagged(v):
    return ["f32", float(v)] if isinstance(v, np.float32) else ["py", float(v) if isinstance(v, float) else int(v)]


def plan_cases(render, out):
    from scipy import ndimage, signal
    seen = {}

    def gaussian_filter(image, sigma, output, mode, cval, truncate):
        assert mode == "constant" and cval == 0.0 and truncate == 5.0 and output.dtype == np.float32
        seen.update(route="spatial", sigma=[float(s) for s in sigma], weights={})
        # the weights scipy itself hands to correlate1d for these sigmas (they do not depend on the image): its own
        # gaussian_filter on a 3 x 3 image, with correlate1d wrapped
        real_correlate = ndimage._filters.correlate1d

        def correlate1d(input, weights, axis, *rest):
            seen["weights"][int(axis)] = np.array(weights, np.float64)
            return real_correlate(input, weights, axis, *rest)

        ndimage._filters.correlate1d = correlate1d
        try:
            real_filter(np.zeros((3, 3), np.float32), sigma=sigma, output=np.zeros((3, 3), np.float32), mode=mode, cval=cval,
                        truncate=truncate)
        finally:
            ndimage._filters.correlate1d = real_correlate

    def window(M, std):
        w = real_window(M, std)
        seen.setdefault("windows", []).append(np.asarray(w, np.float64))
        return w

    def fftconvolve(image, kernel, mode):
        assert mode == "same"
        seen.update(route="direct")
        return image

    real_filter, real_window, real_fft = ndimage.gaussian_filter, signal.windows.gaussian, signal.fftconvolve
    ndimage.gaussian_filter, signal.windows.gaussian, signal.fftconvolve = gaussian_filter, window, fftconvolve
    try:
        for k, (n_y, n_x, bw, bh) in enumerate(PLAN_CASES):
            seen.clear()
            p = f"plan/{k}/"
            out[p + "call"] = np.array(json.dumps({"n_y": n_y, "n_x": n_x, "blur_width": tagged(bw), "blur_height": tagged(bh)}))
            image = np.lib.stride_tricks.as_strided(np.zeros(1, np.float32), (n_y, n_x), (0, 0))
            try:
                with warnings.catch_warnings():
                    warnings.simplefilter("ignore")
                    render._fftconvolve(image, bw, bh)
            except Exception as e:  # noqa: BLE001
                out[p + "raises"] = np.array(type(e).__name__)
                print(f"plan {k}: {n_y} x {n_x}, {bw!r}, {bh!r}: raises {type(e).__name__}")
                continue
            out[p + "route"] = np.array(seen["route"])
            if seen["route"] == "spatial":
                out[p + "sigma"] = np.array(seen["sigma"], np.float64)
                for axis, w in seen["weights"].items():
                    out[p + f"weights_{axis}"] = w
            else:
                ky, kx = seen["windows"]
                out[p + "kernel_y"], out[p + "kernel_x"] = ky, kx
                out[p + "S"] = np.float64(np.outer(ky, kx).sum())
            print(f"plan {k}: {n_y} x {n_x}, {bw!r}, {bh!r}: {seen['route']}")
    finally:
        ndimage.gaussian_filter, signal.windows.gaussian, signal.fftconvolve = real_filter, real_window, real_fft
    out["plan/count"] = np.int64(len(PLAN_CASES))


def fft_noise(render, out):
    """The reference's FFT route against the float64 direct sum, and the restatement of the route against the reference's
    own function in bits."""
    worst = []
    for k, (n_y, n_x, bw, bh) in enumerate(rs.DIRECT_CASES):
        image = rs.poisson_image(n_y, n_x, 100 + k)
        ref = render._fftconvolve(image, bw, bh)
        kw, kh = rs.kernel_of(bw), rs.kernel_of(bh)
        assert np.array_equal(ref.view(np.uint32), rs.fft_reference(image, kw, kh, bw, bh).view(np.uint32))
        exact = rs.direct_float64(image, kw, kh, bw, bh)
        dev = float(np.abs(ref.astype(np.float64) - exact).max() / np.abs(ref).max())
        ours = rs.direct(image, kw, kh, bw, bh)
        same = float((ours.view(np.uint32) == ref.view(np.uint32)).mean())
        print(f"fft {n_y} x {n_x}, kernel {kw} x {kh}: reference - float64 sum = {dev:.3e} of the maximum, {same:.0%} of pixels equal as float32")
        worst.append(dev)
    out["fft/deviation"] = np.array(worst, np.float64)
    out["fft/c"] = np.float64(4.0 * max(worst))
    print("c =", float(out["fft/c"]))


# ---- tables on the 1/64 lattice -----------------------------------------------------------------------------------
def lattice(v):
    return (np.round(np.asarray(v, np.float64) * 64) / 64).astype(np.float32)


def render_table(rng):
    cx, cy = rng.uniform(5, 250, 60), rng.uniform(5, 250, 60)
    x = np.concatenate([rng.normal(c, 0.4, 40) for c in cx] + [rng.uniform(-2, 258, 500)])
    y = np.concatenate([rng.normal(c, 0.4, 40) for c in cy] + [rng.uniform(-2, 258, 500)])
    # rows exactly on the viewport borders (strictly inside is drawn: none of these is) and just inside them
    edge_x = [0.0, 256.0, 100.0, 100.0, 0.0, 256.0, 1 / 64, 256 - 1 / 64, 20.25, 100.25, 50.0, 50.0]
    edge_y = [100.0, 100.0, 0.0, 256.0, 0.0, 256.0, 1 / 64, 256 - 1 / 64, 30.0, 30.0, 10.5, 74.5]
    x, y = lattice(np.concatenate([x, edge_x])), lattice(np.concatenate([y, edge_y]))
    n = len(x)
    return pd.DataFrame({"frame": np.sort(rng.integers(0, 200, n)).astype(np.uint32), "x": x, "y": y,
                         "lpx": rng.uniform(0.1, 0.5, n).astype(np.float32), "lpy": rng.uniform(0.12, 0.56, n).astype(np.float32)})


FULL = ((0.0, 0.0), (256.0, 256.0))
CROP = ((10.5, 20.25), (74.5, 100.25))
AWAY = ((300.0, 300.0), (364.0, 364.0))
RENDER_CASES = {           # name -> (function, oversampling, viewport, min_blur_width or None)
    "smooth_os1": ("_render_smooth", 1.0, FULL, None),
    "smooth_os2p5": ("_render_smooth", 2.5, FULL, None),
    "smooth_crop": ("_render_smooth", 1.0, CROP, None),
    "smooth_out_of_view": ("_render_smooth", 1.0, AWAY, None),
    "convolve_below": ("_render_convolve", 1.0, FULL, 0.05),
    "convolve_above": ("_render_convolve", 1.0, FULL, 1.2),
    "convolve_above_os2p5": ("_render_convolve", 2.5, FULL, 1.2),
    "convolve_crop": ("_render_convolve", 1.0, CROP, 1.2),
    "convolve_out_of_view": ("_render_convolve", 1.0, AWAY, 0.05),
    "hist_os1": ("_render_hist", 1.0, FULL, None),
    "hist_empty": ("_render_hist", 1.0, FULL, None),
}


def render_cases(render, out):
    locs = render_table(np.random.default_rng(20261021))
    for c in locs.columns:
        out["render/in_" + c] = locs[c].to_numpy()
    out["render/case_names"] = np.array(list(RENDER_CASES))
    for name, (fn, osamp, ((y_min, x_min), (y_max, x_max)), mbw) in RENDER_CASES.items():
        stride = 5 if osamp != 1.0 else 1                  # the 640 x 640 images: every fifth row, most pixels stay 0
        table = locs.iloc[:0] if name == "hist_empty" else locs.iloc[::stride]
        args = (table, osamp, y_min, x_min, y_max, x_max) + (() if mbw is None else (mbw,))
        # the float64-widened columns are numba's promotion of the float32 ones (make_goldens_postprocess.py)
        wide = table.assign(x=table["x"].astype(np.float64), y=table["y"].astype(np.float64))
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            n, image = getattr(render, fn)(*args)
            n2, image2 = getattr(render, fn)(*((wide,) + args[1:]))
        assert n == n2 and np.array_equal(image.view(np.uint32), image2.view(np.uint32)), name
        p = f"render/{name}/"
        out[p + "call"] = np.array(json.dumps({"function": fn, "oversampling": osamp, "viewport": [[y_min, x_min], [y_max, x_max]],
                                              "min_blur_width": mbw, "empty_table": name == "hist_empty", "stride": stride}))
        out[p + "n"], out[p + "image"] = np.int64(n), image
        route = "none"
        if fn != "_render_hist" and n:
            in_view = ((table["x"] > x_min) & (table["y"] > y_min) & (table["x"] < x_max) & (table["y"] < y_max)).to_numpy()
            if mbw is None:
                bw = bh = 1
            else:
                bw = osamp * max(np.median(table["lpx"].to_numpy()[in_view]), mbw)
                bh = osamp * max(np.median(table["lpy"].to_numpy()[in_view]), mbw)
            kw, kh = rs.kernel_of(bw), rs.kernel_of(bh)
            route = "spatial" if kh < 0.05 * image.shape[0] and kw < 0.05 * image.shape[1] and max(kh, kw) <= 101 else "direct"
            out[p + "blur"] = np.array([bw, bh], np.float64)
        out[p + "route"] = np.array(route)
        print(f"render {name:22s} n={n:5d} image {image.shape} route {route} max {image.max():.4g}")
    routes = {n: str(out[f"render/{n}/route"]) for n in RENDER_CASES}
    assert routes["smooth_os1"] == routes["smooth_os2p5"] == routes["convolve_below"] == routes["convolve_above"] == "spatial"
    assert routes["convolve_above_os2p5"] == "spatial" and routes["smooth_crop"] == routes["convolve_crop"] == "direct"
    assert int(out["render/smooth_out_of_view/n"]) == 0 and not out["render/convolve_out_of_view/image"].any()


# ---- find_fiducials ---------------------------------------------------------------------------------------------------
FIDUCIALS = [(60.5, 70.5, 180), (150.5, 90.5, 160), (100.5, 200.5, 161), (2.5, 120.5, 190)]      # (x, y, rows); the last: half a box from the border


def fiducial_table(rng):
    xs, ys, fr = [], [], []
    for cx, cy, rows in FIDUCIALS:
        xs.append(cx + rng.normal(0, 0.06, rows))
        ys.append(cy + rng.normal(0, 0.06, rows))
        fr.append(rng.permutation(200)[:rows])
    bx, by = rng.uniform(1, 255, 900), rng.uniform(1, 255, 900)
    far = np.ones(len(bx), bool)
    for cx, cy, _ in FIDUCIALS:
        far &= np.hypot(bx - cx, by - cy) > 8
    xs.append(bx[far][:300]), ys.append(by[far][:300]), fr.append(rng.integers(0, 200, 300))
    x, y, frame = lattice(np.concatenate(xs)), lattice(np.concatenate(ys)), np.concatenate(fr)
    order = np.argsort(frame, kind="stable")
    n = len(x)
    return pd.DataFrame({"frame": frame[order].astype(np.uint32), "x": x[order], "y": y[order],
                         "photons": rng.uniform(500, 5000, n).astype(np.float32),
                         "lpx": rng.uniform(0.01, 0.05, n).astype(np.float32), "lpy": rng.uniform(0.01, 0.05, n).astype(np.float32)})


def fiducial_cases(ref, out):
    imageprocess = ref["imageprocess"]
    pp, _ = mkp.load_reference()
    sys.modules["picasso.postprocess"].picked_locs = pp["picked_locs"]
    locs = fiducial_table(np.random.default_rng(20261022))
    for c in locs.columns:
        out["fiducials/in_" + c] = locs[c].to_numpy()
    infos = {"pixelsize_130": [{"Width": 256, "Height": 256, "Frames": 200, "Pixelsize": 130}],
             "pixelsize_missing": [{"Width": 256, "Height": 256, "Frames": 200}]}
    out["fiducials/case_names"] = np.array(list(infos))
    for name, info in infos.items():
        p = f"fiducials/{name}/"
        out[p + "info"] = np.array(json.dumps(info))
        try:
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                picks, box = imageprocess.find_fiducials(locs.copy(), info)
        except Exception as e:  # noqa: BLE001
            out[p + "raises"] = np.array(type(e).__name__)
            print(f"fiducials {name}: raises {type(e).__name__}: {e}")
            continue
        out[p + "picks"] = np.array([[int(px), int(py)] for px, py in picks], np.int64).reshape(-1, 2)
        out[p + "box"] = np.int64(box)
        print(f"fiducials {name}: box {box}, picks {picks}")
        assert type(box) is int and box == 7
        kept = {(int(px), int(py)) for px, py in picks}
        assert kept == {(60, 70), (100, 200)}, kept              # 180 and 161 rows kept; 160 rows and the one at the border dropped
        x, y = locs["x"].to_numpy().astype(np.float64), locs["y"].to_numpy().astype(np.float64)
        assert int((np.hypot(x - 150, y - 90) < 3.5).sum()) == 160 and int((np.hypot(x - 100, y - 200) < 3.5).sum()) == 161


# ---- align, align_rcc ---------------------------------------------------------------------------------------------------
CHANNEL_SHIFTS = [(0.0, 0.0), (0.375, -0.203125), (2.609375, 1.296875)]          # (dx, dy) of each channel, on the lattice


def channels(rng, with_z):
    cx, cy = rng.uniform(20, 236, 45), rng.uniform(20, 236, 45)
    out = []
    for dx, dy in CHANNEL_SHIFTS:
        x = np.concatenate([rng.normal(c, 0.3, 45) for c in cx]) + dx
        y = np.concatenate([rng.normal(c, 0.3, 45) for c in cy]) + dy
        n = len(x)
        cols = {"frame": np.sort(rng.integers(0, 100, n)).astype(np.uint32), "x": lattice(x), "y": lattice(y),
                "lpx": rng.uniform(0.01, 0.05, n).astype(np.float32), "lpy": rng.uniform(0.01, 0.05, n).astype(np.float32)}
        if with_z:
            cols["z"] = rng.normal(0, 50, n).astype(np.float32)
        out.append(pd.DataFrame(cols))
    return out


def align_cases(ref, out):
    render, imageprocess = ref["render"], ref["imageprocess"]
    lib = sys.modules["picasso.lib"]

    class MockProgress:
        def set_value(self, value):
            pass

    lib.MockProgress = MockProgress
    ns = {"np": np, "pd": pd, "render": render, "imageprocess": imageprocess, "lib": lib, "plt": None, "deepcopy": deepcopy}
    functions_from(os.path.join(REF, "picasso", "lib.py"), {"minimize_shifts"}, ns)
    lib.minimize_shifts = ns["minimize_shifts"]
    functions_from(os.path.join(REF, "picasso", "postprocess.py"), {"align", "align_rcc"}, ns)
    info = [{"Width": 256, "Height": 256, "Frames": 100, "Pixelsize": 130}]
    out["align/info"] = np.array(json.dumps(info))
    out["align/case_names"] = np.array(["xy", "xyz"])
    for name, with_z in (("xy", False), ("xyz", True)):
        tables = channels(np.random.default_rng(20261023), with_z)
        infos = [info] * len(tables)
        p = f"align/{name}/"
        out[p + "columns"] = np.array(list(tables[0].columns))
        for k, t in enumerate(tables):
            for c in t.columns:
                out[f"{p}in{k}_{c}"] = t[c].to_numpy()
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            # align: in place, (shift_x, shift_y)
            mine = deepcopy(tables)
            got, (shift_x, shift_y) = ns["align"](mine, infos, return_shifts=True)
            assert got is mine
            # align_rcc: on a copy, one (mean dx, mean dy) per iteration
            before = deepcopy(tables)
            aligned, shifts = ns["align_rcc"](tables, infos, return_shifts=True)
        assert all(a.equals(b) for a, b in zip(tables, before))
        out[p + "align_shift_x"], out[p + "align_shift_y"] = np.asarray(shift_x, np.float64), np.asarray(shift_y, np.float64)
        out[p + "rcc_shifts"] = np.array(shifts, np.float64).reshape(len(shifts), -1)
        out[p + "iterations"] = np.int64(len(shifts))
        for k, (t, a) in enumerate(zip(mine, aligned)):
            out[f"{p}align_out{k}_x"], out[f"{p}align_out{k}_y"] = t["x"].to_numpy(), t["y"].to_numpy()
            out[f"{p}rcc_out{k}_x"], out[f"{p}rcc_out{k}_y"] = a["x"].to_numpy(), a["y"].to_numpy()
            if with_z:
                assert np.array_equal(a["z"].to_numpy(), tables[k]["z"].to_numpy())
        print(f"align {name}: shifts x {np.round(shift_x, 4)}, y {np.round(shift_y, 4)}; align_rcc: {len(shifts)} iterations, "
              f"shape {out[p + 'rcc_shifts'].shape}, dtypes {[str(a['x'].dtype) for a in aligned]}")
        assert np.abs(np.asarray(shift_x) - [s[0] for s in CHANNEL_SHIFTS] - (shift_x[0] - 0)).max() < 0.05


def signatures(ref, out):
    ns = {}
    functions_from(os.path.join(REF, "picasso", "postprocess.py"), {"align", "align_rcc"}, ns)
    render, imageprocess = ref["render"], ref["imageprocess"]
    sig = {n: str(inspect.signature(getattr(render, n))) for n in ("_render_smooth", "_render_convolve", "_fftconvolve",
                                                                   "render_smooth", "render_convolve")}
    sig["find_fiducials"] = str(inspect.signature(imageprocess.find_fiducials))
    sig["align"], sig["align_rcc"] = str(inspect.signature(ns["align"])), str(inspect.signature(ns["align_rcc"]))
    out["signatures"] = np.array(json.dumps(sig))


def main():
    import scipy
    ref = _refshim.load_reference()
    out = {"versions": np.array(json.dumps({"numpy": np.__version__, "scipy": scipy.__version__, "pandas": pd.__version__}))}
    plan_cases(ref["render"], out)
    fft_noise(ref["render"], out)
    signatures(ref, out)
    render_cases(ref["render"], out)
    fiducial_cases(ref, out)
    align_cases(ref, out)
    path = os.path.join(HERE, "blur_cases.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 1 << 20


if __name__ == "__main__":
    main()
