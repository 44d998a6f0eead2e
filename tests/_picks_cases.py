"""Shared by test_picks_host.py and test_gpu_picks.py: the golden cases of tests/golden/picks_cases.npz as tables, calls
and expected frames."""
import json
import os
import sys

import numpy as np
import pandas as pd

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import _picks_restate as rs  # noqa: E402
import make_goldens_picks as mk  # noqa: E402

G = np.load(os.path.join(HERE, "golden", "picks_cases.npz"))
CASES = [str(n) for n in G["case_names"]]


def columns(name):
    return {str(c): G[f"{name}/in_{c}"] for c in G[name + "/in_columns"]}


def table(name):
    return mk.frame(columns(name), G[name + "/in_index"] if bool(G[name + "/has_index"]) else None)


def call(name):
    return mk.unpack_call(str(G[name + "/call"]))


def expected(name):
    """The golden frames: the table's rows of the recorded index plus the columns the call added."""
    df = table(name)
    frames = []
    for k in range(int(G[name + "/n_out"])):
        q = f"{name}/out{k}_"
        sub = df.loc[G[q + "index"]].copy()
        for c in G[q + "columns"]:
            if str(c) not in sub.columns:
                sub[str(c)] = G[q + str(c)]
        assert list(sub.columns) == [str(c) for c in G[q + "columns"]]
        frames.append((sub, [str(d) for d in G[q + "dtypes"]]))
    return frames


def assert_frames(got, name):
    want = expected(name)
    assert isinstance(got, list) and len(got) == len(want), (name, len(got), len(want))
    for k, (g, (w, dtypes)) in enumerate(zip(got, want)):
        assert list(g.columns) == list(w.columns), (name, k)
        assert [str(d) for d in g.dtypes] == dtypes, (name, k, list(g.dtypes), dtypes)
        assert g.index.dtype == w.index.dtype and np.array_equal(g.index.to_numpy(), w.index.to_numpy()), (name, k)
        assert g.equals(w), (name, k)


def remove_size(name):
    t = json.loads(str(G[name + "/remove_size"]))
    return None if t is None else mk.untag(t)


def generated(shape, n=20000, n_picks=300, seed=3):
    """A table of n rows and n_picks picks of one shape, scalar types mixed, for the CSR offsets across many picks."""
    rng = np.random.default_rng(seed)
    cols = mk.table(rng, rng.uniform(0, 64, n), rng.uniform(0, 64, n), frames=200)
    info = [{"Width": 64, "Height": 64, "Frames": 200, "Pixelsize": 130}]
    c = rng.uniform(-2, 66, (n_picks, 2))

    def typed(v, k):
        return (float(v), np.float64(v), int(v))[k % 3]

    if shape in ("Circle", "Square"):
        picks = [(typed(x, k), typed(y, k + 1)) for k, (x, y) in enumerate(c)]
        size = 1.5
    elif shape == "Rectangle":
        d = rng.uniform(-6, 6, (n_picks, 2))
        d[::7, 0], d[3::7, 1] = 0.0, 0.0
        picks = [((typed(x, k), typed(y, k)), (float(x + dx), float(y + dy))) for k, ((x, y), (dx, dy)) in enumerate(zip(c, d))]
        size = 1.2
    else:
        picks = []
        for k, (x, y) in enumerate(c):
            m = int(rng.integers(3, 12))
            ang = np.sort(rng.uniform(0, 2 * np.pi, m))
            rad = rng.uniform(0.5, 4, m)
            pts = [(typed(x + r * np.cos(a), k), typed(y + r * np.sin(a), k)) for a, r in zip(ang, rad)]
            picks.append(pts + ([pts[0]] if k % 11 else []))          # every 11th stays open
        size = None
    return cols, info, picks, size
