"""NumPy restatement of the picked-localizations contract (picasso/postprocess.py:207-473 picked_locs and its four
helpers, :739-799 remove_locs_in_picks, :849-928 _get_block_locs_at_numba / _locs_at_numba; picasso/lib.py:1884-2031 the
point-in-shape helpers).  TEST INFRASTRUCTURE: both tiers compare against it, and make_goldens_picks.py asserts that it
reproduces the reference's own results (members, order, index) before it writes a golden.

What it pins, per pick, is the member rows as positions in the caller's table IN THE ORDER THE REFERENCE HOLDS THEM IN
BEFORE ITS ``sort_values(by="frame", kind="quicksort")``: quicksort is not stable, so ties between equal frames come
out as the reference's only when the sort is applied to the same sequence.

Circle.  ``ensure_sanity`` first (rows with a NaN / inf in ANY column, x >= Width, y >= Height or a negative x, y, lpx,
lpy, lpz, photons, ellipticity, sx, sy leave).  The rest is sorted by (y_index, x_index) = uint32(y / r), uint32(x / r),
stable.  The reference's block table stops filling at the first sorted row whose index lies outside the K x L grid
(K, L = ceil(Height / r), ceil(Width / r)): that row and every row behind it are in no block.  A pick at
x_, y_ = int(x / r), int(y / r) (truncation toward zero: -0.5 -> 0) takes the blocks k = y_ - 1 .. y_ + 1,
l = x_ - 1 .. x_ + 1 with 0 <= k < K and 0 <= l < L, k outside l, rows in sorted order, and keeps
dx ** 2 + dy ** 2 < r ** 2, strict.  When none of the blocks holds a row the reference's ``indices`` is never
assigned: numba zero-initialises such a variable (an empty array; ssa.py inserts ``Expr.undef``, lowered as a null
constant), pure Python raises UnboundLocalError; the empty result is restated, and minted by seeding the variable.

numba's typing of ``_locs_at_numba`` (tests/golden/_nbemu.py; the squares are plain products): x and y meet in one
array, so in their common type S.  S float64: all float64.  S float32: ``float32[:] - int64`` and
``float32[:] - float32`` stay float32, ``float32[:] - float64`` (a Python float or np.float64 pick coordinate) is
float64; the square keeps the type, the sum of a float32 and a float64 square is float64; r ** 2 is int64 for an
integer radius, float32 for a float32 one, else float64; ``float32[:] < int64`` and ``< float32`` compare in float32,
everything else in float64.

``lib.is_loc_at`` is the same test computed by pandas, not numba: pandas' arithmetic unwraps a NumPy scalar into a
Python one, so float32 columns keep their differences, squares and sum in float32 whatever x and y are (bits 0 and 1
set), while its comparison does not unwrap: a Python ``r ** 2`` compares as float32 (bit 2), an np.float64 one in
float64.  The goldens ``circle_typing`` / ``circle_typing_int_radius`` hold rim rows on which these typings disagree.

Square, Rectangle, Polygon.  No ``ensure_sanity``; boolean masks, so members ascend by table position and a NaN row
fails every comparison.  The strict box ``x_min < x < x_max and y_min < y < y_max`` is a pandas / NumPy-2 comparison: a
Python int or float bound is weak and the compare runs in the column's dtype (a float32 column against
float32(bound)), a NumPy scalar bound compares in the common type, float64 here.  Then nothing (Square),
``check_if_in_rectangle`` or ``check_if_in_polygon``: under numba every operation in them has a float64 operand
(the corners are float64, or int64 meeting a float), so they run in float64 whatever the columns are.

ZeroDivisionError.  ``check_if_in_rectangle`` divides by y_corner_2 - y_corner_1 for a row with
min <= y <= max of the two, so by zero only for a row at exactly the height c of a side with equal corner heights.  The
corners are y1, y2 = sy + dy, sy - dy and y4, y3 = ey + dy, ey - dy (get_pick_rectangle_corners; addition and
subtraction round monotonically).  For dy >= 0: y2 <= y1 and y3 <= y4, so min(Y) = min(y2, y3) and max(Y) =
max(y1, y4).  Side 2-3 flat means c = y2 = y3 = min(Y); side 4-1 flat means c = y4 = y1 = max(Y); side 1-2 flat means
y1 = y2 = sy, then Y = [sy, sy, y3, y4] with y3 <= ey <= y4 and sy strictly inside would need |ey - sy| < dy while dy
vanishes against sy, i.e. ey = sy up to half an ulp, so ey = sy and c is again an extreme (side 3-4 alike); dy < 0
swaps the roles.  A row that passes the strict box has min(Y) < y < max(Y): the division by zero is unreachable from
``picked_locs``.  It IS reachable through ``lib.check_if_in_rectangle`` / ``locs_in_rectangle`` with free corners:
``rectangle_zero_division`` says when, and the Python layer raises there as numba does.  ``check_if_in_polygon`` only
divides behind ``(Y[j] > y) != (Y[j_next] > y)``, which two equal heights never satisfy.
"""
from __future__ import annotations

import numpy as np

SANITY = ("x", "y", "lpx", "lpy", "lpz", "photons", "ellipticity", "sx", "sy")
SQUARE, RECTANGLE, POLYGON = 0, 1, 2


def get_from_metadata(info, key):
    for d in reversed([info] if isinstance(info, dict) else list(info)):
        if key in d:
            return d[key]
    return None


def sane_rows(cols, info):
    """Positions of the rows ``ensure_sanity`` keeps."""
    n = len(cols["x"])
    keep = np.ones(n, bool)
    for v in cols.values():
        v = np.asarray(v)
        if v.dtype.kind == "f":
            keep &= np.isfinite(v)
    keep &= np.asarray(cols["x"]) < get_from_metadata(info, "Width")
    keep &= np.asarray(cols["y"]) < get_from_metadata(info, "Height")
    for c in SANITY:
        if c in cols:
            keep &= np.asarray(cols[c]) >= 0
    return np.flatnonzero(keep)


def grid_shape(info, size):
    return int(np.ceil(get_from_metadata(info, "Height") / size)), int(np.ceil(get_from_metadata(info, "Width") / size))


def block_order(x, y, size, K, L):
    """-> (order, keys in that order, p): np.lexsort([x_index, y_index]) and the position the fill stops at."""
    x_index, y_index = np.uint32(x / size), np.uint32(y / size)
    order = np.lexsort([x_index, y_index])
    xi, yi = x_index[order].astype(np.int64), y_index[order].astype(np.int64)
    outside = np.flatnonzero((yi >= K) | (xi >= L))
    p = int(outside[0]) if len(outside) else len(order)
    return order, (yi << 32) | xi, p


# ---- what the host decides from the scalars it was given ----------------------------------------------------------
def is_weak(v) -> bool:
    """A Python scalar (NEP 50): the comparison runs in the array's dtype."""
    return isinstance(v, (bool, int, float)) and not isinstance(v, np.generic)


def keeps_float32(v) -> bool:
    """numba: float32[:] (op) v stays float32 for an integer or a float32 scalar."""
    return isinstance(v, (bool, int, np.integer, np.bool_, np.float32, np.float16))


def circle_flags(x, y, r) -> int:
    return (1 if keeps_float32(x) else 0) | (2 if keeps_float32(y) else 0) | (4 if keeps_float32(r) else 0)


def radius_squared(r) -> float:
    """r ** 2 under numba, as a float64 value: int64 for an integer, float32 for a float32, else float64."""
    if isinstance(r, np.float32):
        return float(r * r)
    if isinstance(r, (int, np.integer)) and not isinstance(r, bool):
        return float(int(r) * int(r))
    return float(np.float64(r) * np.float64(r))


def block_of(v, size) -> int:
    return int(v / size)


def bound_flags(x_min, x_max, y_min, y_max) -> int:
    return sum(1 << b for b, v in enumerate((x_min, x_max, y_min, y_max)) if is_weak(v))


# ---- membership ---------------------------------------------------------------------------------------------------
def circle_mask(xs, ys, px, py, r2, flags):
    """dx ** 2 + dy ** 2 < r2 for the rows (xs, ys), already in their common type."""
    f32 = xs.dtype == np.float32

    def square(col, c, keep):
        if f32 and keep:
            d = col - np.float32(c)
        else:
            d = col.astype(np.float64) - np.float64(c)
        return d * d

    total = square(xs, px, flags & 1) + square(ys, py, flags & 2)
    if total.dtype == np.float32 and flags & 4:
        return total < np.float32(r2)
    return total.astype(np.float64) < np.float64(r2)


def circle(cols, info, picks, r):
    """-> (offsets int64[P + 1], rows int64: positions in the caller's table, pre-sort order)."""
    sane = sane_rows(cols, info)
    x, y = np.asarray(cols["x"])[sane], np.asarray(cols["y"])[sane]
    S = np.result_type(x.dtype, y.dtype)
    K, L = grid_shape(info, r)
    order, keys, p = block_order(x, y, r, K, L)
    xs, ys, keys = x.astype(S)[order], y.astype(S)[order], keys[:p]
    r2 = radius_squared(r)
    out = []
    for px, py in picks:
        x_, y_ = block_of(px, r), block_of(py, r)
        idx = []
        for k in range(y_ - 1, y_ + 2):
            if 0 <= k < K:
                for ll in range(x_ - 1, x_ + 2):
                    if 0 <= ll < L:
                        a, b = np.searchsorted(keys, [(k << 32) | ll, ((k << 32) | ll) + 1])
                        idx.append(np.arange(a, b))
        idx = np.concatenate(idx) if idx else np.zeros(0, np.int64)
        inside = circle_mask(xs[idx], ys[idx], float(px), float(py), r2, circle_flags(px, py, r))
        out.append(sane[order[idx[inside]]])
    return csr(out)


def csr(per_pick):
    offsets = np.zeros(len(per_pick) + 1, np.int64)
    offsets[1:] = np.cumsum([len(m) for m in per_pick])
    rows = np.concatenate(per_pick).astype(np.int64) if per_pick else np.zeros(0, np.int64)
    return offsets, rows


def box_mask(x, y, bounds, flags):
    def cmp(col, bound, weak, upper):
        if weak:
            b = col.dtype.type(bound)
            return col < b if upper else col > b
        c, b = col.astype(np.float64), np.float64(bound)
        return c < b if upper else c > b

    return (cmp(x, bounds[0], flags & 1, False) & cmp(x, bounds[1], flags & 2, True)
            & cmp(y, bounds[2], flags & 4, False) & cmp(y, bounds[3], flags & 8, True))


def in_rectangle(x, y, X, Y):
    """check_if_in_rectangle in float64; a 0 / 0 or v / 0 follows IEEE (see rectangle_zero_division)."""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    X, Y = np.asarray(X, np.float64), np.asarray(Y, np.float64)
    hits = np.zeros(len(x), np.int64)
    with np.errstate(all="ignore"):
        for i in range(4):
            i2 = 0 if i == 3 else i + 1
            y1, y2, x1, x2 = Y[i], Y[i2], X[i], X[i2]
            level = (min(y1, y2) <= y) & (y <= max(y1, y2))
            m_inv = (x2 - x1) / (y2 - y1)
            x_intersect = m_inv * (y - y1) + x1
            hits += level & (x_intersect >= x)
    return hits % 2 == 1


def rectangle_zero_division(y, Y) -> bool:
    """Would check_if_in_rectangle divide by zero (numba: ZeroDivisionError) for these rows?"""
    y, Y = np.asarray(y, np.float64), np.asarray(Y, np.float64)
    return any(Y[i] == Y[(i + 1) % 4] and bool((y == Y[i]).any()) for i in range(4))


def in_polygon(x, y, X, Y):
    """check_if_in_polygon in float64, operation for operation."""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    X, Y = np.asarray(X, np.float64), np.asarray(Y, np.float64)
    hits = np.zeros(len(x), np.int64)
    m = len(X)
    with np.errstate(all="ignore"):
        for j in range(m):
            j2 = (j + 1) % m
            crosses = (Y[j] > y) != (Y[j2] > y)
            reach = X[j] + (X[j2] - X[j]) * (y - Y[j]) / (Y[j2] - Y[j])
            hits += crosses & (x < reach)
    return hits % 2 == 1


def shapes(cols, shape, bounds, flags, corners=None):
    """-> (offsets, rows): per pick the rows inside the strict box and the shape, ascending.  bounds (P, 4) float64,
    flags P weak-bound bits, corners a list of (X, Y) per pick (None for squares)."""
    x, y = np.asarray(cols["x"]), np.asarray(cols["y"])
    out = []
    for i in range(len(bounds)):
        rows = np.flatnonzero(box_mask(x, y, bounds[i], int(flags[i])))
        if shape == RECTANGLE:
            rows = rows[in_rectangle(x[rows], y[rows], *corners[i])]
        elif shape == POLYGON:
            rows = rows[in_polygon(x[rows], y[rows], *corners[i])]
        out.append(rows)
    return csr(out)


# ---- the picks of a call as the device takes them --------------------------------------------------------------
def rectangle_corners(start_x, start_y, end_x, end_y, width):
    if end_x == start_x:
        alpha = np.pi / 2
    else:
        alpha = np.arctan((end_y - start_y) / (end_x - start_x))
    dx = width * np.sin(alpha) / 2
    dy = width * np.cos(alpha) / 2
    return ([float(start_x - dx), float(start_x + dx), float(end_x + dx), float(end_x - dx)],
            [float(start_y + dy), float(start_y - dy), float(end_y - dy), float(end_y + dy)])


def square_plan(picks, pick_size):
    half_a = pick_size / 2
    b = [(x - half_a, x + half_a, y - half_a, y + half_a) for x, y in picks]
    return np.array([[float(v) for v in q] for q in b], np.float64).reshape(-1, 4), np.array([bound_flags(*q) for q in b], np.uint8), None


def rectangle_plan(picks, pick_size):
    corners = [rectangle_corners(xs, ys, xe, ye, pick_size) for (xs, ys), (xe, ye) in picks]
    b = [(min(X), max(X), min(Y), max(Y)) for X, Y in corners]
    return np.array(b, np.float64).reshape(-1, 4), np.array([bound_flags(*q) for q in b], np.uint8), corners


def polygon_plan(picks):
    """Closed polygons only -> (positions of the kept picks, bounds, flags, corners)."""
    kept = [i for i, pick in enumerate(picks) if len(pick) >= 3 and pick[0] == pick[-1]]
    corners = [([c[0] for c in picks[i]], [c[1] for c in picks[i]]) for i in kept]
    b = [(min(X), max(X), min(Y), max(Y)) for X, Y in corners]
    return kept, np.array([[float(v) for v in q] for q in b], np.float64).reshape(-1, 4), \
        np.array([bound_flags(*q) for q in b], np.uint8), corners


def members(cols, info, picks, pick_shape, pick_size=None):
    """-> (positions of the picks that give a frame, offsets, rows) for one picked_locs call."""
    if pick_shape == "Circle":
        return list(range(len(picks))), *circle(cols, info, picks, pick_size)
    if pick_shape == "Square":
        b, f, _ = square_plan(picks, pick_size)
        return list(range(len(picks))), *shapes(cols, SQUARE, b, f)
    if pick_shape == "Rectangle":
        b, f, c = rectangle_plan(picks, pick_size)
        return list(range(len(picks))), *shapes(cols, RECTANGLE, b, f, c)
    kept, b, f, c = polygon_plan(picks)
    return kept, *shapes(cols, POLYGON, b, f, c)
