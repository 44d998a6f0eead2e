#!/usr/bin/env python3
"""Mint tests/golden/pickkin_cases.npz: the reference's own ``estimate_kinetic_rate`` / ``fit_cum_exp`` on small samples and
its ``pick_kinetics`` / ``evaluate_picks`` / ``pick_properties`` on small lists of picks.

TEST INFRASTRUCTURE, build container only (needs the reference tree, pandas and scipy; no numba).  The functions are
compiled in memory from where they lie in the reference's ``lib.py`` and ``postprocess.py``: the link functions through
make_goldens_link.load_reference (numba's typing from _nbemu), the dark times and ``groupprops`` through
make_goldens_kinetics.load_reference, the rest with the function-picking loader of make_goldens_postprocess.  Nothing of
the reference is stored but inputs and results.

Fit batches.  ``batches`` (JSON) names them; per batch B: ``B_values`` (the column, in its dtype), ``B_offsets``, and per
segment ``B_mode`` (0 not fitted, 1 fitted, 2 scipy raised ValueError), ``B_rate`` (what ``estimate_kinetic_rate``
returned, as float64), ``B_ref`` (a, t, c of ``fit_cum_exp``), ``B_ref_cost``, ``B_opt`` / ``B_opt_cost`` (the tightly
converged optimum: ``scipy.optimize.least_squares`` on the same model and bounds, started at the reference's result, with
ftol = xtol = gtol = 1e-15), ``B_p0`` / ``B_lower`` / ``B_upper`` (what the reference handed to ``curve_fit``).  Costs are
``_pickkin_restate.cost``.  ``g`` is the largest relative gap between the reference's ``t`` and the optimum's over all
fitted segments and ``tol = 4 * g``.  The script asserts for every fitted segment that the reference did not raise and
that the optimum's cost is not above the reference's; a candidate that fails is replaced by the next seed.

Wrapper cases.  ``wrappers`` (JSON) names them; per case W the picks as one CSR (``W_in_columns``, ``W_in_<column>``,
``W_in_offsets``; the column set is uniform per case) and the results of the three functions (``W_pk_*``, ``W_ev_*``, ``W_pp_*``; tables as ``*_columns``,
``*_dtypes``, ``*_<column>``), the callback sequences, and ``W_ev_filled`` (the picks ``evaluate_picks`` writes: it leaves
the others uninitialised).  ``sort_quirk`` records what this pandas does with ``fit_cum_exp``'s in-place sort.

Run:  python tests/golden/make_goldens_pickkin.py
"""
import inspect
import json
import os
import sys
import types
import warnings
from typing import Callable, Literal

import numpy as np
import pandas as pd
import scipy
from scipy import optimize

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _pickkin_restate as rs  # noqa: E402
import make_goldens_kinetics as mgk  # noqa: E402
import make_goldens_link as mgl  # noqa: E402
from make_goldens_postprocess import functions_from  # noqa: E402

REF = os.environ.get("PICASSO_REFERENCE", "/root/reference")
LIB_PY = os.path.join(REF, "picasso", "lib.py")
POST_PY = os.path.join(REF, "picasso", "postprocess.py")
LIB_NAMES = {"cumulative_exponential", "fit_cum_exp", "estimate_kinetic_rate", "get_from_metadata"}
PP_NAMES = {"link", "evaluate_picks", "_pick_kinetics_single", "pick_kinetics", "pick_properties"}
PUBLIC = ("evaluate_picks", "_pick_kinetics_single", "pick_kinetics", "pick_properties")
PUBLIC_LIB = ("cumulative_exponential", "fit_cum_exp", "estimate_kinetic_rate")
warnings.simplefilter("ignore")


class _Recorder:
    """scipy.optimize with a curve_fit that remembers what it was handed."""

    def __init__(self):
        self.last = None

    def curve_fit(self, f, xdata, ydata, p0=None, bounds=None, **kw):
        self.last = (np.array(xdata, np.float64), [float(v) for v in p0], [float(v) for v in bounds[0]],
                     [float(v) for v in bounds[1]])
        return optimize.curve_fit(f, xdata, ydata, p0=p0, bounds=bounds, **kw)


def load_reference():
    rec = _Recorder()
    lib_ns = {"np": np, "optimize": rec, "Any": object}
    functions_from(LIB_PY, LIB_NAMES, lib_ns)
    lib = types.SimpleNamespace(**{k: lib_ns[k] for k in LIB_NAMES}, FloatArray1D=object, IntArray1D=object)
    lns, kns = mgl.load_reference(), mgk.load_reference()
    ns = {"np": np, "pd": pd, "warnings": warnings, "lib": lib, "Callable": Callable, "Literal": Literal,
          "OptimizeWarning": optimize.OptimizeWarning, "tqdm": None,
          "_get_link_groups": lns["_get_link_groups"], "_link_loc_groups": lns["_link_loc_groups"],
          "compute_dark_times": kns["compute_dark_times"], "groupprops": kns["groupprops"]}
    functions_from(POST_PY, PP_NAMES, ns)
    return ns, lib, rec


# ---- fit batches ---------------------------------------------------------------------------------------------------
def tight(x, p_ref, lower, upper):
    y = np.arange(1, len(x) + 1, dtype=np.float64)
    res = optimize.least_squares(lambda p: rs.model(x, *p) - y, np.clip(p_ref, lower, upper), bounds=(lower, upper),
                                 ftol=1e-15, xtol=1e-15, gtol=1e-15, max_nfev=20000)
    return res.x


def run_segment(lib, rec, data):
    """-> dict of what the reference does with one segment, or None when it fails the fixture conditions."""
    out = {"mode": 0, "rate": np.nan, "ref": [np.nan] * 3, "ref_cost": np.nan, "opt": [np.nan] * 3, "opt_cost": np.nan,
           "p0": [np.nan] * 3, "lower": [np.nan] * 3, "upper": [np.nan] * 3}
    rec.last = None
    try:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            out["rate"] = float(lib.estimate_kinetic_rate(data.copy()))
    except ValueError:
        out["mode"] = 2
        assert rs.prepare(data)[0] == "refused", data
        return out
    if rec.last is None:
        kind, value = rs.prepare(data)
        assert kind == "mean" and (value == out["rate"] or (value != value and out["rate"] != out["rate"])), (data, value)
        return out
    x, p0, lower, upper = rec.last
    prep = rs.prepare(data)
    assert prep[0] == "fit" and np.array_equal(prep[1], x) and list(prep[3]) == lower and list(prep[4]) == upper, data
    assert prep[2][0] == p0[0] and prep[2][2] == p0[2] and abs(prep[2][1] - p0[1]) <= 1e-6 * abs(p0[1]), (prep[2], p0)
    ref = lib.fit_cum_exp(data.copy())["best_values"]
    p_ref = np.array([ref["a"], ref["t"], ref["c"]], np.float64)
    assert p_ref[1] == out["rate"]
    p_opt = tight(x, p_ref, lower, upper)
    c_ref, c_opt = rs.cost(x, p_ref), rs.cost(x, p_opt)
    if not c_opt <= c_ref:
        return None
    out.update(mode=1, ref=list(p_ref), ref_cost=c_ref, opt=list(p_opt), opt_cost=c_opt, p0=p0, lower=lower, upper=upper)
    return out


def geometric(rng, n, mean=3.0):
    return rng.geometric(1.0 / mean, n)


def candidates(name, n, seed):
    """The sample of a named kind; another seed gives another sample of the same kind."""
    rng = np.random.default_rng(seed)
    if name == "geometric":
        return geometric(rng, n)
    if name == "exponential":
        return np.ceil(rng.exponential(12.0, n))
    if name == "linear":                    # a near-linear CDF: t runs to its upper bound
        return rng.permutation(np.arange(5, 5 + n)) + (rng.integers(0, 2, n) if seed % 2 else 0)
    if name == "steep":                     # a steep CDF on a high floor: t runs to its lower bound
        return 400 + geometric(rng, n, 2.0)
    if name == "early":                     # many values at the smallest one: c is active at 0
        return np.concatenate([np.ones(max(n // 20, 0)), 1 + np.ceil(rng.exponential(30.0, n - max(n // 20, 0)))])
    if name == "continuous":
        return rng.exponential(7.5, n) + 0.25
    raise KeyError(name)


def build_batch(lib, rec, dtype, plan):
    """plan: a list of literal arrays or (kind, n) -> the batch's arrays."""
    values, offsets, rows, seed = [], [0], [], 1000
    for item in plan:
        if isinstance(item, tuple):
            for attempt in range(50):
                seed += 1
                data = np.asarray(candidates(item[0], item[1], seed)).astype(dtype)
                row = run_segment(lib, rec, data)
                if row is not None and (row["mode"] == 1 or item[1] <= 2):
                    break
            else:
                raise AssertionError(f"no sample of {item} meets the fixture conditions")
        else:
            data = np.asarray(item).astype(dtype)
            row = run_segment(lib, rec, data)
            assert row is not None, item
        values.append(data), offsets.append(offsets[-1] + len(data)), rows.append(row)
    out = {"values": np.concatenate(values).astype(dtype) if values else np.zeros(0, dtype),
           "offsets": np.asarray(offsets, np.int64), "mode": np.array([r["mode"] for r in rows], np.int32)}
    for key in ("rate", "ref_cost", "opt_cost"):
        out[key] = np.array([r[key] for r in rows], np.float64)
    for key in ("ref", "opt", "p0", "lower", "upper"):
        out[key] = np.array([r[key] for r in rows], np.float64).reshape(len(rows), 3)
    return out


def fit_batches(lib, rec):
    nan = np.nan
    edges_int = [[], [7], [3, 9], [1, 2, 3], [1, 5, 6], [4, 4, 4, 4, 4], [6, 6, 6],
                 ("geometric", 63), ("geometric", 64), ("geometric", 65), ("geometric", 257), ("exponential", 64),
                 ("linear", 40), ("linear", 129), ("steep", 50), ("steep", 200), ("early", 100), ("early", 300),
                 ("exponential", 1000)]
    edges_float = [[], [2.5], [1.25, 7.5], [nan], [nan, 4.5], [nan, nan], [0.1, 0.2, 0.7], [3.3, 3.3, 3.3, 3.3],
                   ("continuous", 63), ("continuous", 64), ("continuous", 65), ("continuous", 257), ("linear", 40),
                   ("steep", 50), ("early", 100), [1.0, 2.0, nan, 4.0, 5.0], [1.0, 2.0, np.inf, 4.0]]
    rng = np.random.default_rng(5)
    mixed = [("geometric", int(n)) for n in rng.integers(0, 200, 300)]
    mixed[7], mixed[130], mixed[299] = ("geometric", 0), ("geometric", 1), ("geometric", 2)
    plans = {"edges_i32": (np.int32, edges_int), "edges_i64": (np.int64, edges_int[:11]),
             "edges_f32": (np.float32, edges_float), "edges_f64": (np.float64, edges_float[:12]),
             "mixed_i32": (np.int32, mixed), "big_i32": (np.int32, [("geometric", 4096)]),
             "big_f32": (np.float32, [("continuous", 4096), [5.5] * 300])}
    return {name: build_batch(lib, rec, dtype, plan) for name, (dtype, plan) in plans.items()}


# ---- wrapper cases -------------------------------------------------------------------------------------------------
FRAMES = 3000
INFO = [{"Frames": FRAMES, "Width": 64, "Height": 64, "Pixelsize": 130}]


def blinking_pick(rng, pick, n_events, z=False, group=True, xy=np.float32):
    """One pick: a site that binds n_events times; a list of localizations in frame order, a few frames skipped."""
    frames, t = [], int(rng.integers(5, 40))
    for _ in range(n_events):
        length = int(rng.geometric(1 / 3.0))
        frames += [t + k for k in range(length) if k == 0 or k == length - 1 or rng.random() > 0.15]
        t += length + int(rng.geometric(1 / 25.0)) + 4
    frames = np.array([f for f in frames if f < FRAMES - 1], np.int64)
    n = len(frames)
    cx, cy = rng.uniform(5, 59, 2)
    cols = {"frame": frames.astype(np.uint32), "x": (cx + rng.normal(0, 0.05, n)).astype(xy),
            "y": (cy + rng.normal(0, 0.05, n)).astype(xy), "photons": rng.uniform(500, 9000, n).astype(np.float32),
            "sx": rng.uniform(0.8, 1.5, n).astype(np.float32), "sy": rng.uniform(0.8, 1.5, n).astype(np.float32),
            "bg": rng.uniform(5, 40, n).astype(np.float32), "lpx": rng.uniform(0.005, 0.06, n).astype(np.float32),
            "lpy": rng.uniform(0.005, 0.06, n).astype(np.float32)}
    if z:
        cols["z"] = rng.normal(0, 80, n).astype(np.float32)
    if group:
        cols["group"] = np.full(n, pick, np.int32)
    return pd.DataFrame(cols)


def wrapper_inputs(ns):
    cases = {}
    for name, seed, n_picks, z, group, linked, shuffle in (
            ("plain", 1, 12, False, True, False, False), ("z_nogroup", 2, 5, True, False, False, False),
            ("z_group", 3, 40, True, True, False, True), ("linked", 4, 9, False, True, True, False),
            ("linked_nogroup_z", 5, 6, True, False, True, False), ("f64", 6, 7, False, True, False, True)):
        rng = np.random.default_rng(seed)
        picks = []
        for p in range(n_picks):
            n_events = [0, 1][p - 1] if p in (1, 2) else int(rng.integers(2, 45))
            if p == 4:
                n_events = 3
            pick = blinking_pick(rng, p, n_events, z=z, group=group, xy=np.float64 if name == "f64" else np.float32)
            if shuffle and len(pick):
                pick = pick.iloc[rng.permutation(len(pick))].reset_index(drop=True)
            if linked and len(pick):
                pick = ns["link"](pick, INFO, r_max=999999, max_dark_time=3).reset_index(drop=True)
            picks.append(pick)
        if linked:                                  # an empty pick of a linked list has the linked columns
            template = next(p for p in picks if len(p))
            picks = [p if len(p) else template.iloc[:0].copy() for p in picks]
        cases[name] = picks
    return cases


def table_arrays(prefix, table):
    out = {prefix + "_columns": np.array(list(table.columns)), prefix + "_dtypes": np.array([str(t) for t in table.dtypes]),
           prefix + "_index": np.asarray(table.index)}
    for c in table.columns:
        out[f"{prefix}_{c}"] = table[c].to_numpy()
    return out


def run_wrappers(ns, name, picks, lib):
    out = {}
    columns = list(picks[0].columns)
    assert all(list(p.columns) == columns for p in picks)
    out["in_columns"] = np.array(columns)
    out["in_offsets"] = np.concatenate([[0], np.cumsum([len(p) for p in picks])]).astype(np.int64)
    for c in columns:
        out["in_" + c] = np.concatenate([p[c].to_numpy() for p in picks])
    fresh = lambda: [p.copy() for p in picks]      # noqa: E731   (the reference writes into the tables it is handed)
    seen = []
    length, dark, no_locs, out_locs = ns["pick_kinetics"](fresh(), INFO, max_dark_time=3, progress_callback=seen.append)
    out.update(pk_length=length, pk_dark=dark, pk_no_locs=no_locs, pk_callbacks=np.array(seen, np.int64))
    out.update(table_arrays("pk_out", out_locs))
    seen = []
    N, n_events, rmsd, rmsd_z, ev_length, ev_dark, new_locs = ns["evaluate_picks"](fresh(), INFO, max_dark_time=3,
                                                                                    progress_callback=seen.append)
    filled = np.array([len(p) > 0 for p in picks])
    out.update(ev_N=N, ev_n_events=n_events, ev_rmsd=rmsd, ev_rmsd_z=rmsd_z, ev_length=ev_length, ev_dark=ev_dark,
               ev_filled=filled, ev_has_z=np.bool_("z" in columns), ev_callbacks=np.array(seen, np.int64))
    out.update(table_arrays("ev_new", new_locs))
    if "group" in columns:
        seen_k, seen_g = [], []
        areas = np.linspace(0.01, 0.02, len(length))
        props = ns["pick_properties"](fresh(), INFO, max_dark_time=3, influx_rate=0.04, pick_areas=areas,
                                      kinetics_progress=seen_k.append, groupprops_progress=seen_g.append)
        out.update(table_arrays("pp", props))
        out.update(pp_areas=areas, pp_callbacks_k=np.array(seen_k, np.int64), pp_callbacks_g=np.array(seen_g, np.int64))
    # what the in-place sort of fit_cum_exp did: the same call with a library that fits a copy
    plain = types.SimpleNamespace(**vars(lib))
    plain.estimate_kinetic_rate = lambda data: lib.estimate_kinetic_rate(np.array(data))
    ns["lib"] = plain
    try:
        _, _, _, unsorted = ns["pick_kinetics"](fresh(), INFO, max_dark_time=3)
    finally:
        ns["lib"] = lib
    sorted_rows = not (np.array_equal(unsorted["len"].to_numpy(), out_locs["len"].to_numpy())
                       and np.array_equal(unsorted["dark"].to_numpy(), out_locs["dark"].to_numpy()))
    restated = pd.concat([rs.sort_fitted_columns(t.copy()) if sorted_rows else t for _, t in _split(unsorted, no_locs)],
                         ignore_index=True)
    matches = all(np.array_equal(restated[c].to_numpy(), out_locs[c].to_numpy()) for c in out_locs.columns)
    return {f"{name}_{k}": v for k, v in out.items()}, sorted_rows, matches


def _split(table, counts):
    at = 0
    for k, n in enumerate(counts):
        yield k, table.iloc[at:at + n]
        at += n


def main():
    ns, lib, rec = load_reference()
    out = {}
    batches = fit_batches(lib, rec)
    gaps = []
    for name, b in batches.items():
        fitted = b["mode"] == 1
        assert (b["opt_cost"][fitted] <= b["ref_cost"][fitted]).all()
        gaps += list(np.abs(b["ref"][fitted, 1] - b["opt"][fitted, 1]) / b["ref"][fitted, 1])
        out.update({f"{name}_{k}": v for k, v in b.items()})
    everything = np.concatenate([np.c_[b["opt"], b["lower"], b["upper"]][b["mode"] == 1] for b in batches.values()])
    t, t_lo, t_hi, c = everything[:, 1], everything[:, 4], everything[:, 7], everything[:, 2]
    assert (t >= t_hi * (1 - 1e-9)).any(), "no case with t at its upper bound"
    # No sample is known that ends with t on its LOWER bound: the "steep" samples (a steep CDF on a high floor) have a local
    # minimum there, which the reference's descent from p0 does not reach (it ends on the upper bound), and a search over
    # 6000 random small samples found none either.  The count is printed, not asserted.
    assert (c <= 1e-8).any(), "no case with c active at 0"
    assert any((b["mode"] == 2).any() for b in batches.values())
    g = float(max(gaps))
    out.update(batches=json.dumps(list(batches)), g=np.float64(g), tol=np.float64(4 * g))
    print(f"{sum(int((b['mode'] == 1).sum()) for b in batches.values())} fitted segments, g = {g:.3e}, tol = {4 * g:.3e}; "
          f"t at upper bound {int((t >= t_hi * (1 - 1e-9)).sum())}, at lower {int((t <= t_lo * (1 + 1e-9)).sum())}, "
          f"c = 0 {int((c <= 1e-8).sum())}")

    quirk, restated_ok = [], []
    inputs = wrapper_inputs(ns)
    for name, picks in inputs.items():
        arrays, sorted_rows, matches = run_wrappers(ns, name, picks, lib)
        out.update(arrays)
        quirk.append(sorted_rows), restated_ok.append(matches)
        print(f"{name}: {len(picks)} picks, {len(arrays[name + '_pk_length'])} kept, in-place sort seen: {sorted_rows}, "
              f"restated: {matches}")
    assert all(restated_ok), "the restatement of the in-place sort does not reproduce out_locs"
    assert len(set(quirk)) == 1 or not any(quirk), quirk
    sigs = {n: str(inspect.signature(ns[n])) for n in PUBLIC}
    sigs.update({n: str(inspect.signature(getattr(lib, n))) for n in PUBLIC_LIB})
    out.update(wrappers=json.dumps(list(inputs)), sort_quirk=np.bool_(any(quirk)), signatures=json.dumps(sigs),
               info=json.dumps(INFO), versions=json.dumps({"pandas": pd.__version__, "numpy": np.__version__,
                                                           "scipy": scipy.__version__}))
    path = os.path.join(HERE, "pickkin_cases.npz")
    np.savez_compressed(path, **out)
    print(f"pickkin_cases.npz: {os.path.getsize(path)} bytes, sort_quirk = {any(quirk)}")


if __name__ == "__main__":
    main()
