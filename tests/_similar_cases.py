"""Shared by test_similar_host.py and test_gpu_similar.py: the golden cases of tests/golden/similar_cases.npz as tables
and calls, and fixed-seed tables for the grid search."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import _picks_restate as prs  # noqa: E402
import _similar_restate as rs  # noqa: E402
import make_goldens_similar as mk  # noqa: E402

G = np.load(os.path.join(HERE, "golden", "similar_cases.npz"))
CASES = [str(n) for n in G["case_names"]]


def columns(name):
    return {str(c): G[f"{name}/in_{c}"] for c in G[name + "/in_columns"]}


def table(name):
    return mk.mkp.frame(columns(name), None)


def call(name):
    """-> (info, picks, d, std_range, max_shifts, kind)"""
    return mk.unpack_call(str(G[name + "/call"]))


def same_bits(a, b) -> bool:
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def assert_pairs(got, name):
    """The returned list against the golden: length, order and every bit of every pair."""
    assert isinstance(got, list) and all(isinstance(t, tuple) and len(t) == 2 for t in got), name
    want_x, want_y = G[name + "/out_x"], G[name + "/out_y"]
    assert len(got) == len(want_x), (name, len(got), len(want_x))
    assert all(type(v) is np.float64 for t in got for v in t), name
    assert same_bits(np.array([t[0] for t in got], np.float64), want_x), name
    assert same_bits(np.array([t[1] for t in got], np.float64), want_y), name


def clustered(seed, width, height, n_clusters, dtype=np.float32, y_dtype=None, background=60):
    """A fixed-seed table of a few hundred rows: clusters of 5 .. 40 rows and a sparse background."""
    rng = np.random.default_rng(seed)
    xs, ys = [rng.uniform(0, width, background)], [rng.uniform(0, height, background)]
    for _ in range(n_clusters):
        m, s = int(rng.integers(5, 41)), rng.uniform(0.1, 0.5)
        xs.append(rng.normal(rng.uniform(0, width), s, m))
        ys.append(rng.normal(rng.uniform(0, height), s, m))
    x = np.clip(np.concatenate(xs), 0.0, width - 0.01).astype(dtype)
    y = np.clip(np.concatenate(ys), 0.0, height - 0.01).astype(y_dtype or dtype)
    order = rng.permutation(len(x))
    return x[order], y[order]


def assert_shift(got, want, what):
    """The four per-point outputs of the grid search against the restatement's, in bits."""
    assert got[2].dtype == np.int32 and np.array_equal(got[2], want[2]), what
    for k in (0, 1, 3):
        assert same_bits(got[k], want[k]), (what, k, int((got[k] != want[k]).sum()))
