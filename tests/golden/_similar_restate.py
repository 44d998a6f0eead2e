"""NumPy restatement of the pick-similar contract (picasso/postprocess.py:476-736 pick_similar / _pick_similar, :820-845
_n_block_locs_at, :848-957 get_block_locs_at_numba, locs_at_numba, rmsd_at_com).  TEST INFRASTRUCTURE: both tiers compare
against it, and make_goldens_similar.py asserts that it reproduces the reference's own results in bits before it writes a
golden.  ``max_shifts`` (the reference's constant 500) is a parameter so that the cap can be tested.

The table.  ``get_index_blocks(locs, info, r)`` with ``r = d / 2``: ``ensure_sanity``, then the stable order by
(y_index, x_index) = uint32(y / r), uint32(x / r); the block table stops filling at the first sorted row outside the
K x L grid (_picks_restate.block_order).  x and y meet in one array of their common type S (float32 only when both are).

The given picks.  Their members are N16's circle (_picks_restate.circle, numba's typing of the pick's scalars
included; r is always a Python float here).  ``n_locs`` is their number and ``rmsd`` is ``rmsd_at_com`` of them; a pick
without members divides 0.0 by 0 in numba's ``np.mean`` (ZeroDivisionError).  The four bounds are the reference's own
NumPy calls on the two lists.

numba's ``np.mean`` of a 1-D array (numba/np/arraymath.py array_mean) is ``c = zero; for v in np.nditer(arr):
c += v.item(); return c / arr.size``: one sequential chain, not NumPy's pairwise sum.  For float32 the accumulator is
float32 (``get_accumulator(dtype, 0)`` is ``np.float32(0)`` and ``float32 + float32`` stays float32) and the division
``float32 / int64`` is a float64 one.  The loop was read in a copy of numba's source; the accumulator and return type
are those of numba >= 0.57's overload as remembered (the copy at hand was 0.54.1, whose lowering returns the array's
own dtype and which the reference's ``numba>=0.62.1`` excludes); nothing of it was run.  Tables whose coordinates are
multiples of 1/64 with fewer than 2^10 members per circle have exact partial sums in float32 and float64 alike: their
goldens hold whatever the accumulator is ("dyadic" cases).

The grid search.  The centre is a float64 throughout, so ``S[:] - centre`` and everything after it is float64; squares
are plain products (``dd->d`` power with exponent 2).  Per grid point, columns outside and y inside, odd columns on the
shifted y values:
  gate     the rows of the blocks k = y_r - 1 .. y_r + 1, l = x_r - 1 .. x_r + 1 with 0 < k < K and 0 < l < L (block row 0
           and block column 0 never count; no such block: numba's zero-initialised variable, 0) must number
           >= min_n_locs; ``uint64 - 1`` is int64 under numba (NumPy: float64);
  rows     those of the same blocks with 0 <= k < K, 0 <= l < L in block order, fetched once;
  shift    members around the grid point; at most one: skipped.  The centre moves to their mean; while |dx| > 1e-3 or
           |dy| > 1e-3: count += 1, break if count > max_shifts, members around the new centre, break if at most one,
           else the centre moves to their mean;
  judged   the last member set (taken around the previous centre), its mean and its ``rmsd_at_com``;
  accept   every pick so far, the given ones included, has (xs - x) ** 2 + (ys - y) ** 2 > d2; min_n <= n <= max_n;
           min_rmsd <= rmsd <= max_rmsd.  A candidate that fails a range never influences another, so the ranges are
           applied first and ``greedy`` runs over the rest.
"""
from __future__ import annotations

import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _picks_restate as picks  # noqa: E402

SKIPPED, CONVERGED, CAPPED, STARVED = 0, 1, 2, 3          # how a grid point's loop ended


def seq_sum(a):
    """``c = dtype(0); for v in a: c += v`` in a's own type (np.add.accumulate is that chain)."""
    a = np.asarray(a)
    return np.add.accumulate(np.concatenate([np.zeros(1, a.dtype), a]))[-1]


def nb_mean(a) -> np.float64:
    a = np.asarray(a)
    if a.size == 0:
        raise ZeroDivisionError("division by zero")
    return np.float64(seq_sum(a)) / np.float64(a.size)


def rmsd_at_com(xs, ys) -> np.float64:
    com_x, com_y = nb_mean(xs), nb_mean(ys)
    ex, ey = xs.astype(np.float64) - com_x, ys.astype(np.float64) - com_y
    return np.sqrt(nb_mean(ex * ex + ey * ey))


def common(x, y):
    S = np.result_type(np.asarray(x).dtype, np.asarray(y).dtype)
    return np.asarray(x).astype(S), np.asarray(y).astype(S)


def pick_stats(cols, info, picks_, r):
    """-> (n_locs list of int, rmsd list of float64) of the given picks."""
    offsets, rows = picks.circle(cols, info, picks_, r)
    x, y = common(cols["x"], cols["y"])
    n_locs, rmsd = [], []
    for a, b in zip(offsets[:-1], offsets[1:]):
        n_locs.append(int(b - a))
        rmsd.append(rmsd_at_com(x[rows[a:b]], y[rows[a:b]]))
    return n_locs, rmsd


def bounds(n_locs, rmsd, std_range):
    mean_n_locs, mean_rmsd = np.mean(n_locs), np.mean(rmsd)
    std_n_locs, std_rmsd = np.std(n_locs), np.std(rmsd)
    return (max(2, mean_n_locs - std_range * std_n_locs), mean_n_locs + std_range * std_n_locs,
            mean_rmsd - std_range * std_rmsd, mean_rmsd + std_range * std_rmsd)


def grid(info, d):
    """-> (x_range, y_range_base, y_range_shift, x_r, y_r_base, y_r_shift), the block indices as int64."""
    r = d / 2
    x_range = np.arange(d / 2, info[0]["Width"], np.sqrt(3) * d / 2)
    y_range_base = np.arange(d / 2, info[0]["Height"] - d / 2, d)
    y_range_shift = y_range_base + d / 2
    as_int = lambda v: np.uint64(v / r).astype(np.int64)          # noqa: E731
    return x_range, y_range_base, y_range_shift, as_int(x_range), as_int(y_range_base), as_int(y_range_shift)


def _run(keys, k, l0, l1):
    return np.searchsorted(keys, [(k << 32) | l0, ((k << 32) | l1) + 1])


def block_rows(keys, K, L, x_r, y_r):
    """-> (positions of the nine blocks' rows in block order, the gate's count)."""
    idx, gated = [], 0
    for k in range(y_r - 1, y_r + 2):
        if 0 <= k < K:
            l0, l1 = max(x_r - 1, 0), min(x_r + 1, L - 1)
            if l0 <= l1:
                a, b = _run(keys, k, l0, l1)
                idx.append(np.arange(a, b))
                if k >= 1 and l1 >= 1:
                    a, b = _run(keys, k, max(l0, 1), l1)
                    gated += int(b - a)
    return (np.concatenate(idx) if idx else np.zeros(0, np.int64)), gated


def members(xs, ys, cx, cy, r2):
    dx, dy = xs.astype(np.float64) - np.float64(cx), ys.astype(np.float64) - np.float64(cy)
    return dx * dx + dy * dy < np.float64(r2)


def shift(x, y, size, K, L, grid_, r2, gate, max_shifts=500):
    """The mean shift of every grid point over the (sanity-filtered) columns x, y -> cx, cy (float64), n (int32), rmsd
    (float64) per grid point in grid order, and two diagnostics: the number of shifts and how the loop ended."""
    x_range, y_base, y_shift, x_r, y_r_base, y_r_shift = grid_
    xs, ys = common(x, y)
    order, keys, p = picks.block_order(xs, ys, size, K, L)
    xs, ys, keys = xs[order], ys[order], keys[:p]
    G = len(x_range) * len(y_base)
    cx, cy, rmsd = np.zeros(G), np.zeros(G), np.zeros(G)
    n, shifts, ended = np.zeros(G, np.int32), np.zeros(G, np.int64), np.zeros(G, np.int64)
    g = -1
    for i, x_grid in enumerate(x_range):
        ygrid, y_r = (y_shift, y_r_shift) if i % 2 else (y_base, y_r_base)
        for j, y_grid in enumerate(ygrid):
            g += 1
            cx[g], cy[g] = x_grid, y_grid
            idx, gated = block_rows(keys, K, L, int(x_r[i]), int(y_r[j]))
            if not gated >= gate:
                continue
            bx, by = xs[idx], ys[idx]
            m = members(bx, by, x_grid, y_grid, r2)
            if m.sum() <= 1:
                continue
            old_x, old_y = np.float64(x_grid), np.float64(y_grid)
            tx, ty = nb_mean(bx[m]), nb_mean(by[m])
            count, ended[g] = 0, CONVERGED
            while abs(tx - old_x) > 1e-3 or abs(ty - old_y) > 1e-3:
                count += 1
                if count > max_shifts:
                    ended[g] = CAPPED
                    break
                old_x, old_y = tx, ty
                m = members(bx, by, tx, ty, r2)
                if m.sum() > 1:
                    tx, ty = nb_mean(bx[m]), nb_mean(by[m])
                else:
                    ended[g] = STARVED
                    break
            cx[g], cy[g], n[g], shifts[g] = tx, ty, m.sum(), min(count, max_shifts)
            if n[g] > 1:
                rmsd[g] = rmsd_at_com(bx[m], by[m])
    return cx, cy, n, rmsd, shifts, ended


def in_ranges(n, rmsd, b):
    min_n, max_n, min_rmsd, max_rmsd = b
    with np.errstate(invalid="ignore"):
        return (n >= min_n) & (n <= max_n) & (rmsd >= min_rmsd) & (rmsd <= max_rmsd)


def greedy(cand_x, cand_y, pick_x, pick_y, d2):
    """The accept test's first clause over candidates in grid order -> (bool keep, int64 who: the position in
    picks + kept candidates of the first pick that refused a candidate, -1 for a kept one)."""
    xs, ys = list(np.asarray(pick_x, np.float64)), list(np.asarray(pick_y, np.float64))
    keep, who = np.zeros(len(cand_x), bool), np.full(len(cand_x), -1, np.int64)
    for i, (x, y) in enumerate(zip(cand_x, cand_y)):
        ax, ay = np.array(xs, np.float64) - x, np.array(ys, np.float64) - y
        apart = ax * ax + ay * ay > d2
        if apart.all():
            keep[i] = True
            xs.append(x)
            ys.append(y)
        else:
            who[i] = int(np.flatnonzero(~apart)[0])
    return keep, who


def pick_similar(cols, info, picks_, d, std_range=2.0, max_shifts=500, details=False):
    """-> (x_similar, y_similar) float64: the given picks, then the accepted grid points in grid order."""
    r, d2 = d / 2, d ** 2
    n_locs, rmsd = pick_stats(cols, info, picks_, r)
    b = bounds(n_locs, rmsd, std_range)
    sane = picks.sane_rows(cols, info)
    x, y = np.asarray(cols["x"])[sane], np.asarray(cols["y"])[sane]
    K, L = picks.grid_shape(info, r)
    out = shift(x, y, r, K, L, grid(info, d), np.float64(r) * np.float64(r), b[0], max_shifts)
    cx, cy, n, spread = out[:4]
    px = np.array([p[0] for p in picks_], np.float64)
    py = np.array([p[1] for p in picks_], np.float64)
    cand = np.flatnonzero(in_ranges(n, spread, b))
    keep, who = greedy(cx[cand], cy[cand], px, py, d2)
    xs, ys = np.concatenate([px, cx[cand][keep]]), np.concatenate([py, cy[cand][keep]])
    if details:
        return xs, ys, dict(bounds=b, shift=out, cand=cand, keep=keep, who=who, n_locs=n_locs, rmsd=rmsd)
    return xs, ys
