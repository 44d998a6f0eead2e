#!/usr/bin/env python3
"""Mint tests/golden/average_cases.npz: the reference's own particle averaging on small tables.

TEST INFRASTRUCTURE, build container only (needs the reference tree, pandas and SciPy; no numba).
``_fill`` and ``render_hist_numba`` are compiled from where they lie in the reference's ``render.py`` (the ``numba.njit``
decorator dropped), ``compute_xcorr``, ``align_group_core``, ``build_group_index``, ``com_align`` and
``prepare_locs_for_save`` from its ``average.py``, and run as they are; nothing of the reference is stored here.
``ref_average`` below drives them in a serial loop that repeats the body of the reference's ``average()`` line for
line: its process pool cannot pickle functions made by ``exec``, and a group only touches its own rows, so the order
of the groups does not matter.  ``compute_xcorr`` is wrapped to see every correlation the reference computes: that
gives the reference's choice per group (angle index, y_max, x_max, as ``align_group_core`` decides it) and the
distance of its float32 correlation from the integer one.

Per case the file holds the input table, the metadata, ``r`` / ``a_step`` / ``angles`` / the centre-of-mass aligned
x, y, and per iteration the float32 state before (``x0``, ``y0``), the reference's choices (``choice``: groups x 3,
-1 where nothing was chosen), the state after (``x1``, ``y1``), the callback's table columns (``cb_x``, ``cb_y``),
``multi`` (groups whose integer maximum is attained more than once) and ``departs`` (groups where the reference's
choice is not the oracle's); then the final table (``out_*``) and the shifted one with its metadata.  ``edges``
records what the reference returns or raises (type and text), ``signatures`` the public signatures, ``versions`` the
library versions, ``lds_bins`` the LDS bound ``global_path`` was made for.

The script asserts (a) the reference's float32 correlation is within 0.5 of the integer everywhere, (b) in every
ordinary case the reference departs from the oracle (tests/golden/_average_restate.py) in at most 10 % of the groups
per iteration and every departure is a tie, (c) every edge the cases are there for occurs.

Run:  python tests/golden/make_goldens_average.py [--lds-bins N]
"""
import argparse
import ast
import inspect
import json
import os
import re
import sys
import types
import warnings
from multiprocessing import sharedctypes

import numpy as np
import pandas as pd
import scipy
import scipy.sparse

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _average_restate as rs  # noqa: E402

REF = os.environ.get("PICASSO_REFERENCE", "/root/reference")
AVERAGE_PY = os.path.join(REF, "picasso", "average.py")
RENDER_PY = os.path.join(REF, "picasso", "render.py")
VERSION_PY = os.path.join(REF, "picasso", "version.py")
RENDER_NAMES = ("_fill", "render_hist_numba")
NAMES = ("compute_xcorr", "align_group_core", "build_group_index", "com_align", "prepare_locs_for_save")
PUBLIC = ("compute_xcorr", "build_group_index", "com_align", "prepare_locs_for_save")
LDS_BINS = 16384                # AVERAGE_LDS_BINS of the library (tests/test_average_host.py holds the two together)
LIST = 2048                     # AVERAGE_LIST of the library
INFO = [{"Pixelsize": 130, "Width": 64, "Height": 32}]
ORDINARY = ("sites", "odd_n", "even_n", "global_path", "big_group", "edges", "single_group")


def _get_from_metadata(info, key, default=None, *, raise_error=False):
    for d in reversed([info] if isinstance(info, dict) else list(info)):
        if key in d:
            return d[key]
    if raise_error:
        raise KeyError(f"Key '{key}' not found in metadata.")
    return default


def _compile(path, names, ns):
    tree = ast.parse(open(path).read())
    keep = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in names]
    assert [n.name for n in keep] == list(names), [n.name for n in keep]
    for n in keep:
        n.decorator_list = []
    mod = ast.Module(body=[ast.ImportFrom("__future__", [ast.alias("annotations")], 0)] + keep, type_ignores=[])
    exec(compile(ast.fix_missing_locations(mod), path, "exec"), ns)
    return ns


class Seen:
    """What ``align_group_core`` decides, followed through the correlations it asks for."""

    def __init__(self):
        self.max_err = 0.0
        self.begin(None)

    def begin(self, avg):
        self.avg, self.ai, self.best, self.choice = avg, 0, 0.0, (-1, -1, -1)

    def see(self, xcorr, image):
        exact = np.fft.fftshift(np.rint(np.real(np.fft.ifft2(
            np.fft.fft2(image.astype(np.float64)) * np.conj(np.fft.fft2(self.avg.astype(np.float64)))))))
        self.max_err = max(self.max_err, float(np.abs(xcorr - exact).max()))
        y_max, x_max = np.unravel_index(xcorr.argmax(), xcorr.shape)
        if xcorr[y_max, x_max] > self.best:
            self.best, self.choice = xcorr[y_max, x_max], (self.ai, int(y_max), int(x_max))
        self.ai += 1


def load_reference():
    version = re.search(r'__version__\s*=\s*"([^"]+)"', open(VERSION_PY).read()).group(1)
    r = _compile(RENDER_PY, RENDER_NAMES, {"np": np})
    ns = {"np": np, "pd": pd, "scipy": scipy, "render": types.SimpleNamespace(render_hist_numba=r["render_hist_numba"]),
          "lib": types.SimpleNamespace(get_from_metadata=_get_from_metadata), "__version__": version}
    _compile(AVERAGE_PY, NAMES, ns)
    seen, real = Seen(), ns["compute_xcorr"]

    def watched(CF_image_avg, image):
        xcorr = real(CF_image_avg, image)
        seen.see(xcorr, image)
        return xcorr

    ns["compute_xcorr_unwatched"], ns["compute_xcorr"], ns["seen"], ns["version"] = real, watched, seen, version
    ns["average"] = _compile(AVERAGE_PY, ("average",), {})["average"]      # for its signature only: it is never called
    return ns


def signature(fn):
    """[name, kind, default] of every parameter: what a caller can rely on (the annotations name the reference's types)."""
    return [[p.name, p.kind.name, repr(p.default) if p.default is not p.empty else None]
            for p in inspect.signature(fn).parameters.values()]


def ref_average(ref, locs, info, *, display_pixel_size=5.0, iterations=3, return_shifted_locs=False, tamper=None, log=None):
    """The body of the reference's ``average()`` with the pool replaced by a loop over the groups.  ``tamper`` may
    change the shared arrays before the first iteration (a state the tests start from); ``log`` collects the record."""
    render, seen = ref["render"], ref["seen"]
    log = {} if log is None else log
    assert (
        "group" in locs.columns
    ), "Localizations DataFrame must have a 'group' column."
    group_index = ref["build_group_index"](locs)
    locs = ref["com_align"](locs, group_index)
    n_groups = group_index.shape[0]
    r = 2 * np.sqrt((locs["x"] ** 2 + locs["y"] ** 2).mean())
    t_min = -r
    t_max = r
    camera_pixelsize = _get_from_metadata(info, "Pixelsize", raise_error=True)
    oversampling = camera_pixelsize / display_pixel_size
    a_step = np.arcsin(1 / (oversampling * r))
    angles = np.arange(0, 2 * np.pi, a_step)
    x_ = sharedctypes.RawArray("f", locs["x"].to_numpy())
    y_ = sharedctypes.RawArray("f", locs["y"].to_numpy())
    x, y = np.ctypeslib.as_array(x_), np.ctypeslib.as_array(y_)
    log.update(r=r, a_step=a_step, angles=angles, oversampling=oversampling, com_x=locs["x"].to_numpy().copy(),
               com_y=locs["y"].to_numpy().copy(), n_groups=n_groups, its=[])
    if tamper is not None:
        tamper(x, y, t_max)
    for it in range(iterations):
        rec = {"x0": x.copy(), "y0": y.copy(), "choice": []}
        N_avg, image_avg = render.render_hist_numba(x, y, oversampling, t_min, t_max)
        n_pixel, _ = image_avg.shape
        image_half = n_pixel / 2
        CF_image_avg = np.conj(np.fft.fft2(image_avg))
        for group in range(n_groups):
            index = group_index[group].nonzero()[1]
            seen.begin(image_avg)
            x_aligned, y_aligned = ref["align_group_core"](index, x, y, angles, oversampling, t_min, t_max, CF_image_avg,
                                                           image_half)
            assert seen.ai == len(angles)
            rec["choice"].append(seen.choice)
            x[index] = x_aligned
            y[index] = y_aligned
        locs["x"] = np.ctypeslib.as_array(x)
        locs["y"] = np.ctypeslib.as_array(y)
        locs["x"] -= np.mean(locs["x"])
        locs["y"] -= np.mean(locs["y"])
        rec.update(x1=x.copy(), y1=y.copy(), cb_x=locs["x"].to_numpy().copy(), cb_y=locs["y"].to_numpy().copy(),
                   n_pixel=n_pixel, image=image_avg.copy(), choice=np.array(rec["choice"], np.int64).reshape(n_groups, 3))
        log["its"].append(rec)
    if return_shifted_locs:
        params = {"disp_px_size": display_pixel_size, "it": iterations}
        locs, info = ref["prepare_locs_for_save"](locs, info, params)
        return locs, info
    return locs


# ---- tables -------------------------------------------------------------------------------------------------
PATTERN = np.array([[0.3 * np.cos(t), 0.3 * np.sin(t)] for t in (0, 2.1, 4.0)] + [[0.0, 0.0]])


def particles(rng, sizes, labels=None, sigma=0.04):
    """Groups on the 3-site pattern + centre, each rotated and moved at random; rows shuffled."""
    rows = []
    for g, n in enumerate(sizes):
        th = rng.uniform(0, 2 * np.pi)
        p = PATTERN[rng.integers(0, len(PATTERN), n)] + rng.normal(0, sigma, (n, 2))
        R = np.array([[np.cos(th), -np.sin(th)], [np.sin(th), np.cos(th)]])
        p = p @ R.T + rng.uniform(5, 30, 2)
        rows.extend((q[0], q[1], g if labels is None else labels[g]) for q in p)
    rows = [rows[i] for i in rng.permutation(len(rows))]
    return table(rows)


def table(rows, x_dtype=np.float32):
    x, y, g = (np.array(v) for v in zip(*rows))
    return {"x": x.astype(x_dtype), "y": y.astype(np.float32), "group": g.astype(np.int32),
            "photons": (np.arange(len(x)) * 7 % 1000).astype(np.float32)}


def n_pixel_for(ref, cols, dps):
    log = {}
    ref_average(ref, pd.DataFrame(cols), INFO, display_pixel_size=dps, iterations=0, log=log)
    return rs.n_pixel_of(log["oversampling"], -log["r"], log["r"])


def make_cases(ref, bound):
    rng = np.random.default_rng(20261019)
    cases = {}
    # 12 groups of 20 to 60 rows, drawn group after group from seed 1 and left in that order
    one, rows = np.random.default_rng(1), []
    for g in range(12):
        th, n = one.uniform(0, 2 * np.pi), one.integers(20, 60)
        p = PATTERN[one.integers(0, len(PATTERN), n)] + one.normal(0, 0.04, (n, 2))
        p = p @ np.array([[np.cos(th), -np.sin(th)], [np.sin(th), np.cos(th)]]).T + one.uniform(5, 30, 2)
        rows.extend((q[0], q[1], g) for q in p)
    base = table(rows)
    cases["sites"] = dict(cols=base, dps=5.0, iterations=3)
    small = {c: v[np.isin(base["group"], [0, 1, 2, 3, 4])] for c, v in base.items()}
    found = {}
    for dps in np.arange(40, 61) / 10:
        n = n_pixel_for(ref, small, float(dps))
        found.setdefault("odd_n" if n % 2 else "even_n", float(dps))
    for name in ("odd_n", "even_n"):
        cases[name] = dict(cols=small, dps=found[name], iterations=2)
    cases["global_path"] = dict(cols=particles(rng, rng.integers(15, 25, 6)), dps=1.0, iterations=1, check_every=16)
    cases["big_group"] = dict(cols=particles(rng, [30, LIST + 250, 25, 40]), dps=5.0, iterations=1)
    # edges: unsorted, negative and gapped labels; a group of one row; an outlier beyond r; a float64 x column;
    # and, put into the state before the first iteration, a row exactly on t_max
    # The group of one row is a tie by construction once it has left the origin (every angle gives one pixel, and the
    # average image has plateaus), so the case holds 20 groups: the 10 % share of (b) then admits it.
    e = particles(rng, [30, 1, 40, 25, 35, 30] + [28] * 14, labels=[7, -3, 2000, 2, 100, -40] + list(range(300, 342, 3)))
    k = int(np.flatnonzero(e["group"] == 100)[0])
    e["x"][k] += 1.5
    e["x"] = e["x"].astype(np.float64)
    cases["edges"] = dict(cols=e, dps=5.0, iterations=2, on_t_max=int(np.flatnonzero(e["group"] == 2)[3]), outlier=k)
    cases["single_group"] = dict(cols=particles(rng, [45]), dps=5.0, iterations=1)
    # ties: two rows (a turn by pi gives the same two pixels back, or nearly), four-fold symmetric crosses
    rows = []
    for g in range(6):
        c, d = rng.uniform(5, 30, 2), rng.uniform(0.1, 0.3) * np.array([np.cos(g), np.sin(g)])
        rows += [(c[0] + d[0], c[1] + d[1], g), (c[0] - d[0], c[1] - d[1], g)]
    for g in range(6, 10):
        c, a = rng.uniform(5, 30, 2), 0.125 * (g - 4)
        rows += [(c[0] + a, c[1], g), (c[0] - a, c[1], g), (c[0], c[1] + a, g), (c[0], c[1] - a, g)]
    cases["ties"] = dict(cols=table(rows), dps=5.0, iterations=2)
    assert rs.n_pixel_of(130 / 1.0, -1, 1) ** 2 > bound
    return cases


def outcome(fn):
    try:
        res = fn()
    except Exception as e:  # noqa: BLE001
        return {"raises": type(e).__name__, "message": str(e)}
    if res is None:
        return {"returns": None}
    return {"returns": list(res.columns), "dtypes": [str(d) for d in res.dtypes], "rows": len(res)}


def edge_inputs(base):
    return {"empty": {c: v[:0] for c, v in base.items()},
            "no group": {c: v for c, v in base.items() if c != "group"}}


def analyse(name, case, log, ordinary):
    """Per iteration: the oracle from the recorded state, the groups that depart, the groups with several maxima."""
    groups, order, offsets = rs.group_order(case["cols"]["group"])
    ov, r, angles = log["oversampling"], log["r"], log["angles"]
    for it, rec in enumerate(log["its"]):
        avg, choices, x1, y1 = rs.iteration(rec["x0"], rec["y0"], order, offsets, angles, ov, -r, r, case.get("check_every", 1))
        assert np.array_equal(avg, rec["image"]) and rec["image"].dtype == np.float32
        n = avg.shape[0]
        theirs = np.where(rec["choice"][:, :1] < 0, -1, np.c_[rec["choice"][:, 0], rec["choice"][:, 1] * n + rec["choice"][:, 2]])
        departs = np.flatnonzero((theirs != choices[:, 1:]).any(axis=1))
        multi = np.zeros(len(groups), bool)
        for g in range(len(groups)):
            index = order[offsets[g]:offsets[g + 1]]
            corrs = [rs.correlation(rec["x0"][index], rec["y0"][index], a, avg, ov, -r, r, both=False) for a in angles] \
                if n * n <= LDS_BINS else None
            if corrs is not None:
                multi[g] = sum(int((c == choices[g, 0]).sum()) for c in corrs) > 1 and choices[g, 0] > 0
            if g in departs:          # a departure must be a tie: the reference's choice attains the integer maximum
                assert theirs[g, 0] >= 0, (name, it, g)
                c = rs.correlation(rec["x0"][index], rec["y0"][index], angles[theirs[g, 0]], avg, ov, -r, r)
                assert c.flat[theirs[g, 1]] == choices[g, 0], (name, it, g, c.flat[theirs[g, 1]], choices[g])
        if ordinary:
            assert len(departs) <= 0.1 * len(groups), (name, it, departs)
            keep = np.ones(len(rec["x0"]), bool)
            for g in departs:
                keep[order[offsets[g]:offsets[g + 1]]] = False
            assert np.array_equal(x1[keep], rec["x1"][keep]) and np.array_equal(y1[keep], rec["y1"][keep]), (name, it)
        rec.update(multi=multi, departs=departs, oracle=choices)
        print(f"{name:13s} it {it}: n_pixel {n:3d}, {len(angles):3d} angles, {len(groups):2d} groups, "
              f"{len(departs)} depart, {int(multi.sum())} with several maxima")


def main():
    warnings.simplefilter("ignore")
    ap = argparse.ArgumentParser()
    ap.add_argument("--lds-bins", type=int, default=LDS_BINS)
    bound = ap.parse_args().lds_bins
    ref = load_reference()
    out = {"versions": np.array(json.dumps({"pandas": pd.__version__, "numpy": np.__version__, "scipy": scipy.__version__,
                                            "picasso": ref["version"]})),
           "signatures": np.array(json.dumps({**{n: signature(ref[n if n != "compute_xcorr" else "compute_xcorr_unwatched"])
                                                 for n in PUBLIC}, "average": signature(ref["average"])})),
           "lds_bins": np.array(bound), "list": np.array(LIST), "info": np.array(json.dumps(INFO))}
    cases = make_cases(ref, bound)
    out["case_names"] = np.array(list(cases))
    for name, case in cases.items():
        p, cols, log = name + "/", case["cols"], {}
        tamper = None
        if "on_t_max" in case:
            def tamper(x, y, t_max, k=case["on_t_max"]):
                x[k] = t_max
        final = ref_average(ref, pd.DataFrame(cols), INFO, display_pixel_size=case["dps"], iterations=case["iterations"],
                            tamper=tamper, log=log)
        analyse(name, case, log, name in ORDINARY)
        out[p + "in_columns"] = np.array(list(cols))
        for c, v in cols.items():
            out[p + "in_" + c] = v
        out[p + "dps"], out[p + "iterations"] = np.array(case["dps"]), np.array(case["iterations"])
        for k in ("r", "a_step", "angles", "com_x", "com_y"):
            out[p + k] = np.asarray(log[k])
        out[p + "r_type"] = np.array(type(log["r"]).__name__ + "/" + type(log["a_step"]).__name__)
        for it, rec in enumerate(log["its"]):
            for k in ("x0", "y0", "choice", "x1", "y1", "cb_x", "cb_y", "multi", "departs", "n_pixel"):
                out[f"{p}it{it}/{k}"] = np.asarray(rec[k])
        out[p + "exact"] = np.array(all(len(rec["departs"]) == 0 for rec in log["its"]) and tamper is None)
        out[p + "columns"] = np.array(list(final.columns))
        for c in final.columns:
            out[p + "out_" + c] = final[c].to_numpy()
        shifted, info = ref_average(ref, pd.DataFrame(cols), INFO, display_pixel_size=case["dps"],
                                    iterations=case["iterations"], return_shifted_locs=True, tamper=tamper)
        out[p + "shifted_x"], out[p + "shifted_y"] = shifted["x"].to_numpy(), shifted["y"].to_numpy()
        out[p + "shifted_info"] = np.array(json.dumps(info))
    seen = ref["seen"]
    print("largest distance of the reference's float32 correlation from the integer:", seen.max_err)
    assert seen.max_err < 0.5                                                                     # (a)

    # (c) each edge occurs
    n_of = {name: int(out[f"{name}/it0/n_pixel"]) for name in cases}
    assert n_of["odd_n"] % 2 == 1 and n_of["even_n"] % 2 == 0 and n_of["sites"] == 28 and len(out["sites/angles"]) == 86, n_of
    assert n_of["global_path"] ** 2 > bound >= max(n_of[k] for k in cases if k != "global_path") ** 2
    assert np.bincount(cases["big_group"]["cols"]["group"]).max() > LIST
    e, cols = cases["edges"], cases["edges"]["cols"]
    r = float(out["edges/r"])
    assert out["edges/r"].dtype == np.float64 and out["sites/r"].dtype == np.float32 and cols["x"].dtype == np.float64
    assert (np.bincount(cols["group"] - cols["group"].min()) == 1).any() and (np.diff(cols["group"]) < 0).any() and cols["group"].min() < 0
    assert out["edges/it0/x0"][e["on_t_max"]] == np.float32(r) == r and out["edges/it0/x1"][e["on_t_max"]] != np.float32(r)
    assert out["edges/it0/x0"][e["outlier"]] > r and out["edges/it0/x1"][e["outlier"]] != out["edges/it0/x0"][e["outlier"]]
    assert len(np.unique(cases["single_group"]["cols"]["group"])) == 1
    ties = sum(int(out[f"ties/it{it}/multi"].sum()) for it in range(cases["ties"]["iterations"]))
    assert ties >= 10, ties
    assert bool(out["sites/exact"])
    out["on_t_max"], out["outlier"] = np.array(e["on_t_max"]), np.array(e["outlier"])

    edges = {}
    base = cases["sites"]["cols"]
    for name, cols in edge_inputs(base).items():
        edges[name] = outcome(lambda: ref_average(ref, pd.DataFrame(cols), INFO))
    edges["no Pixelsize"] = outcome(lambda: ref_average(ref, pd.DataFrame(base), [{"Width": 64}]))
    zero = ref_average(ref, pd.DataFrame(cases["edges"]["cols"]), INFO, iterations=0)
    edges["iterations=0"] = outcome(lambda: zero)
    out["zero_x"], out["zero_y"] = zero["x"].to_numpy(), zero["y"].to_numpy()
    for k, v in edges.items():
        print(f"edge {k!r}: {json.dumps(v)}")
    out["edges"] = np.array(json.dumps(edges))

    path = os.path.join(HERE, "average_cases.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 1 << 20


if __name__ == "__main__":
    main()
