#!/usr/bin/env python3
"""Time picasso_amd.postprocess.compute_dark_times() and groupprops() on a seeded table of binding events (warm, median
of 5, table in host memory as a user passes it), with the stages of the calls timed on their own.

  python tools/time_kinetics.py [--sizes small,single] [--repeats 5] [--out FILE]
  python tools/time_kinetics.py --reference FILE.py [--groups 250]      the reference's own groupprops on the CPU, one run
                                                                        on the first --groups groups, and the repository's
                                                                        vectorised restatement of the dark times

small:   the 1.0e6-row, 25 000-site table of tools/time_centers.py (the site of every row as its group) after link()
single:  1.0e5 binding events in ONE group: what the per-group sums cost on one lane
Prints one JSON line per size (and appends it to --out).  --reference needs no GPU for its own timings, but the table
it times is link()'s: it reads the events from --events FILE.npz when given (written by a GPU run with --save-events),
and otherwise makes unlinked events of one row each from the same seeded table."""
import argparse
import json
import os
import sys
import time

import numpy as np
import pandas as pd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from time_centers import SIZES, emit, median_ms, table  # noqa: E402

INFO = [{"Frames": 20_000, "Width": 1024, "Height": 1024}]


def single_events(n=100_000, seed=2):
    rng = np.random.default_rng(seed)
    frame = np.sort(rng.integers(0, 4_000_000, n)).astype(np.uint32)
    cols = {"frame": frame, "x": (512 + rng.normal(0, 0.012, n)).astype(np.float32),
            "y": (512 + rng.normal(0, 0.012, n)).astype(np.float32)}
    for c, (lo, hi) in {"photons": (500, 9000), "sx": (0.8, 1.5), "sy": (0.8, 1.5), "bg": (5, 40), "lpx": (0.005, 0.06),
                        "lpy": (0.005, 0.06), "net_gradient": (3000, 20000)}.items():
        cols[c] = rng.uniform(lo, hi, n).astype(np.float32)
    cols["group"] = np.zeros(n, np.int32)
    cols["len"] = rng.integers(1, 20, n).astype(np.uint32)
    cols["n"] = cols["len"].copy()
    return pd.DataFrame(cols)


def unlinked_events(locs):
    """Every localization as an event of one frame: the shape of the linked table without a GPU."""
    ev = locs.sort_values(kind="quicksort", by="frame").reset_index(drop=True)
    ev["len"] = np.ones(len(ev), np.uint32)
    ev["n"] = np.ones(len(ev), np.uint32)
    return ev


def reference_groupprops(path):
    import ast
    import itertools
    from typing import Callable, Literal
    ns = {"np": np, "pd": pd, "itertools": itertools, "Callable": Callable, "Literal": Literal}
    keep = [n for n in ast.parse(open(path).read()).body if isinstance(n, ast.FunctionDef) and n.name == "groupprops"]
    mod = ast.Module(body=[ast.ImportFrom("__future__", [ast.alias("annotations")], 0)] + keep, type_ignores=[])
    exec(compile(ast.fix_missing_locations(mod), path, "exec"), ns)
    return ns["groupprops"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default=None)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--reference", default=None, help="path of the reference's postprocess.py: time its groupprops on the CPU")
    ap.add_argument("--groups", type=int, default=250, help="with --reference: the number of groups it runs on")
    ap.add_argument("--events", default=None, help="with --reference: an .npz of the linked events")
    ap.add_argument("--save-events", default=None, help="write the linked events of the small table to this .npz")
    a = ap.parse_args()
    if a.reference:
        sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
        import _kinetics_restate as rs
        if a.events:
            z = np.load(a.events)
            events, origin = pd.DataFrame({c: z[c] for c in z.files}), "the linked events of a GPU run"
        else:
            events, origin = unlinked_events(table(*SIZES["small"])), "one event per row of the seeded table (no link)"
        rec = {"size": "small", "events": len(events), "table": origin,
               "what": "this machine's CPU, one run each: the repository's vectorised restatement of the dark times (the "
                       "reference's numba loop is not run), and the reference's own groupprops on the first groups"}
        cols = {c: events[c].to_numpy() for c in events.columns}
        rec["restated_dark_ms"], dark = median_ms(lambda: rs.dark_times(cols), 1, lambda: None, "restated dark times")
        events["dark"] = np.int32(dark)
        ids = np.unique(events["group"])
        part = events[events["group"] < ids[min(a.groups, len(ids)) - 1] + 1]
        gp = reference_groupprops(a.reference)
        rec["ref_groupprops_part_ms"], res = median_ms(lambda: gp(part), 1, lambda: None, "the reference's groupprops")
        rec["part_groups"], rec["part_rows"], rec["all_groups"] = int(len(res)), int(len(part)), int(len(ids))
        # per group the reference masks the whole table, so the cost of a group grows with the rows: a lower bound
        rec["ref_groupprops_lower_bound_ms"] = rec["ref_groupprops_part_ms"] * len(ids) / len(res)
        rec["extrapolation"] = "part_ms * all_groups / part_groups, a lower bound: every group also masks the whole table"
        emit(rec, a.out)
        return
    import torch
    from picasso_amd import backend, postprocess as pp
    torch.cuda.set_device(0)
    sync = torch.cuda.synchronize
    for name in (a.sizes or "small,single").split(","):
        print(f"{name}: making the table ...", file=sys.stderr, flush=True)
        if name == "single":
            events = single_events()
        else:
            events = pp.link(table(*SIZES[name]), INFO, r_max=0.05, max_dark_time=3).reset_index(drop=True)
            if a.save_events:
                np.savez(a.save_events, **{c: events[c].to_numpy() for c in events.columns})
        fresh = lambda: events.copy(deep=False)  # noqa: E731      compute_dark_times adds a column to its argument
        kept = pp.compute_dark_times(fresh())                                       # warm: library, allocator, scratch
        props = pp.groupprops(kept)
        rec = {"size": name, "events": len(events), "with_dark_time": len(kept), "groups": len(props), "columns": len(kept.columns)}
        rec["compute_dark_times_ms"], _ = median_ms(lambda: pp.compute_dark_times(fresh()), a.repeats, sync, "compute_dark_times_ms")
        rec["groupprops_ms"], _ = median_ms(lambda: pp.groupprops(kept), a.repeats, sync, "groupprops_ms")
        # the stages, each on its own
        frame, group = events["frame"].to_numpy(), events["group"].to_numpy()
        last = frame + events["len"].to_numpy() - 1
        f64, g64, l64 = (v.astype(np.int64) for v in (frame, group, last))
        rec["dark_upload_ms"], _ = median_ms(lambda: [backend._to_device(v) for v in (f64, g64, l64)], a.repeats, sync, "dark_upload_ms")
        rec["dark_order_ms"], dt = median_ms(lambda: backend.DarkTable(f64, g64, l64), a.repeats, sync, "dark_order_ms (upload included)")
        rec["dark_search_ms"], _ = median_ms(dt.search, a.repeats, sync, "dark_search_ms (download included)")
        rec["host_filter_ms"], _ = median_ms(lambda: kept[kept["dark"] != -1], a.repeats, sync, "host_filter_ms")
        cols = {c: kept[c].to_numpy() for c in kept.columns}
        rec["props_upload_ms"], _ = median_ms(lambda: [backend._to_device(v) for v in cols.values()], a.repeats, sync, "props_upload_ms")
        rec["props_order_ms"], groups = median_ms(lambda: backend.CenterGroups(cols["group"]), a.repeats, sync, "props_order_ms (upload of group included)")
        for c in cols:
            groups._dev(backend._centers_column(cols[c], c))                         # resident: the statistics are timed without uploads
        rec["props_one_f32_column_ms"], _ = median_ms(lambda: backend.group_mean_std(groups, [cols["x"]]), a.repeats, sync, "props_one_f32_column_ms")
        rec["props_one_u32_column_ms"], _ = median_ms(lambda: backend.group_mean_std(groups, [cols["frame"]]), a.repeats, sync, "props_one_u32_column_ms")
        rec["props_all_columns_ms"], _ = median_ms(lambda: backend.group_mean_std(groups, list(cols.values())), a.repeats, sync, "props_all_columns_ms")
        emit(rec, a.out)


if __name__ == "__main__":
    main()
