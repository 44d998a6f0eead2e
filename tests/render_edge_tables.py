"""Localization tables for the render edge tests (test_gpu_render_edges.py on the GPU,
test_oracle_golden.py on the CPU).  Everything is generated from fixed seeds; no image is larger than
160 x 160 and every table builds fewer than 1e5 profile values.
"""
from collections import namedtuple

import numpy as np

Case = namedtuple("Case", "x y lpx lpy oversampling viewport min_blur")
VIEW64 = [(0.0, 0.0), (64.0, 64.0)]
# float32 widths whose normalisation 1 / (2 pi sx sy) overflows float32: the profile holds inf or NaN
TINY = 1e-20            # with itself: norm = 1.6e39
SUBNORMAL = 1e-40       # a float32 subnormal; with an ordinary width: norm = 5e39


def f32(*v):
    return np.array(v, np.float32)


def case(rows, oversampling=1.0, viewport=VIEW64, min_blur=0.0):
    """rows: (x, y, lpx, lpy) each."""
    a = np.asarray(rows, np.float64).reshape(-1, 4)
    with np.errstate(all="ignore"):
        a = a.astype(np.float32)
    return Case(a[:, 0].copy(), a[:, 1].copy(), a[:, 2].copy(), a[:, 3].copy(), float(oversampling), viewport, float(min_blur))


def ordinary_rows(rng, n, x_lo, x_hi, y_lo, y_hi, lp_lo=0.05, lp_hi=5.0):
    """n rows in the box, both widths log-uniform over two decades."""
    return np.stack([rng.uniform(x_lo, x_hi, n), rng.uniform(y_lo, y_hi, n),
                     np.exp(rng.uniform(np.log(lp_lo), np.log(lp_hi), n)),
                     np.exp(rng.uniform(np.log(lp_lo), np.log(lp_hi), n))], axis=1)


# ---------------------------------------------------------------------------
# profiles that are not finite (oversampling 1, viewport (0,0)-(64,64), min_blur_width 0)
# ---------------------------------------------------------------------------
INF_ROWS = [(20.5, 20.5, TINY, TINY),          # on a pixel centre: dy = 0, norm overflows -> inf at (20, 20) only
            (40.5, 40.5, 0.2, 0.2),            # ordinary
            (50.5, 12.5, TINY, TINY)]          # inf at (12, 50) only
ZERO_ROW = (10.3, 10.7, 0.0, 0.0)              # 0 * inf: NaN at (10, 10) only (the Python surface raises instead)
MIXED_ROWS = [(20.5, 20.5, SUBNORMAL, 0.3),    # one column, three rows, inf in the middle one
              (44.5, 20.5, 0.3, SUBNORMAL),    # one row, three columns, all inf
              (30.25, 50.5, TINY, TINY),       # off the pixel centre in x: gy = inf, gx = exp(-huge) = 0, NaN at (50, 30) only
              (10.5, 40.5, SUBNORMAL, SUBNORMAL),
              (40.5, 40.5, 0.2, 0.2)]


def _inf_rows():
    return case(INF_ROWS)


def _with_zero_width():
    return case(INF_ROWS + [ZERO_ROW])


def _mixed():
    return case(MIXED_ROWS)


def _among_ordinary():
    """The same rows in one tile between ordinary localizations: 76 rows of tile (0, 0) in three LDS chunks, the first
    two with rows that are not finite, the third without; plus rows of the other three tiles."""
    rng = np.random.default_rng(11)
    rows = list(ordinary_rows(rng, 70, 2, 30, 2, 30, 0.05, 2.0))
    bad = [(20.5, 20.5, TINY, TINY), (10.5, 5.5, TINY, TINY), (25.5, 9.5, SUBNORMAL, 0.3), (7.5, 27.5, 0.3, SUBNORMAL),
           (10.3, 10.7, 0.0, 0.0), (15.25, 3.75, TINY, TINY)]
    for at, row in zip((3, 10, 17, 33, 40, 52), bad):
        rows.insert(at, row)
    rows += list(ordinary_rows(rng, 30, 2, 62, 2, 62, 0.05, 2.0))
    rows.insert(90, (50.5, 44.5, TINY, TINY))
    return case(rows)


NONFINITE = {"inf_rows": _inf_rows, "with_zero_width": _with_zero_width, "mixed": _mixed, "among_ordinary": _among_ordinary}


def odd_widths(min_blur):
    """Widths NaN, +-inf, negative, huge and float32-subnormal, alone and paired with an ordinary one: empty or
    one-pixel footprints, between ordinary rows.  np.maximum turns a negative width into 0 unless min_blur is
    negative too."""
    odd = [np.nan, np.inf, -np.inf, -0.3, -0.1, -1e-3, 1e9, SUBNORMAL, 1.4e-45, TINY]
    rng = np.random.default_rng(12)
    rows = list(ordinary_rows(rng, 6, 2, 62, 2, 62, 0.1, 1.5))
    k = 0
    for w in odd:
        for lpx, lpy in ((w, w), (w, 0.3), (0.3, w)):
            cx, cy = 4.5 + 6 * (k % 10), 4.5 + 6 * (k // 10)        # on a pixel centre, and a little off it
            rows.append((cx, cy, lpx, lpy))
            rows.append((cx + 2.8, cy + 3.3, lpx, lpy))
            k += 1
    rows += list(ordinary_rows(rng, 6, 2, 62, 2, 62, 0.1, 1.5))
    return case(rows, min_blur=min_blur)


# ---------------------------------------------------------------------------
# tile seams
# ---------------------------------------------------------------------------
SEAM_SIZES = [(31, 32), (32, 33), (33, 64), (63, 31), (64, 65), (65, 63), (32, 32), (64, 64), (65, 31), (31, 65)]


def tile_seam(ny, nx):
    """An ny x nx image whose size ceil() decides: oversampling 1.3, viewport origin (-1.21, -0.37)."""
    osamp, y_min, x_min = 1.3, -1.21, -0.37
    y_max, x_max = y_min + (ny - 0.4) / osamp, x_min + (nx - 0.4) / osamp
    rng = np.random.default_rng(1000 * ny + nx)
    px = []                                                         # rows in image coordinates, widths in image pixels
    for cy in (32, 64):
        for cx in (32, 64):
            if cy < ny and cx < nx:                                 # on a tile corner: the footprint spans 4 tiles
                px += [(cx, cy, 0.7, 1.1), (cx + 0.01, cy - 0.01, 2.5, 0.4), (cx - 0.3, cy + 0.2, 1e-3, 1e-3)]
    for cx, cy in ((0.01, 0.01), (nx - 0.02, 0.02), (0.02, ny - 0.02), (nx - 0.01, ny - 0.01)):
        px.append((cx, cy, 1.2, 0.9))                               # on an image corner: clipped on two sides
    px += [(nx / 2, ny / 2, 100.0, 100.0), (nx / 3, ny / 1.5, 40.0, 0.6), (nx / 1.5, ny / 3, 0.5, 30.0)]   # wider than the image
    for _ in range(12):                                             # 1 x 1 footprints
        px.append((rng.uniform(0.2, nx - 0.2), rng.uniform(0.2, ny - 0.2), 1e-3, 1e-3))
    px += list(ordinary_rows(rng, 60, 0.05, nx - 0.05, 0.05, ny - 0.05, 0.05, 5.0))
    px = np.asarray(px)
    order = rng.permutation(len(px))
    px = px[order]
    rows = np.stack([x_min + px[:, 0] / osamp, y_min + px[:, 1] / osamp, px[:, 2] / osamp, px[:, 3] / osamp], axis=1)
    rows = np.concatenate([rows, [(x_min - 0.5, y_min + 3, 0.5, 0.5), (x_max + 0.5, y_min + 3, 0.5, 0.5),
                                  (x_min + 3, y_max + 0.5, 0.5, 0.5)]])            # out of view, next to the image
    return case(rows, osamp, [(y_min, x_min), (y_max, x_max)])


# ---------------------------------------------------------------------------
# chunk seams
# ---------------------------------------------------------------------------
CHUNK_SIZES = [31, 32, 33, 64, 65, 97]
OVERLAP = (slice(12, 16), slice(40, 44))        # every footprint of chunk_seam() covers part of these pixels


def chunk_seam(m, interleaved):
    """m localizations in tile (0, 1) of a 64 x 64 image, centres within 4 x 4 pixels, widths over two decades, so that
    the order of the additions decides the float32 sum.  Interleaved: the same rows in the same order between rows of
    other tiles and rows out of view."""
    rng = np.random.default_rng(100 + m)
    rows = ordinary_rows(rng, m, 40, 44, 12, 16, 0.05, 5.0)
    if interleaved:
        out = []
        for row in rows:
            for _ in range(rng.integers(0, 3)):
                if rng.random() < 0.5:
                    out.append(ordinary_rows(rng, 1, 2, 30, 34, 62, 0.05, 1.0)[0])          # tile (1, 0)
                else:
                    out.append(ordinary_rows(rng, 1, 65, 90, -20, 80, 0.05, 5.0)[0])        # out of view
            out.append(row)
        rows = np.asarray(out)
    return case(rows)


def order_matters(fwd, rev):
    """The image of the reversed table differs in bits where the footprints overlap."""
    return bool((fwd[OVERLAP].view(np.uint32) != rev[OVERLAP].view(np.uint32)).any())


# ---------------------------------------------------------------------------
# launch seams
# ---------------------------------------------------------------------------
LAUNCH_SIZES = [1, 63, 64, 65, 255, 256, 257, 513]
LAUNCH_VIEW = [(-0.5, 0.25), (63.5, 64.25)]          # exact in float32, so that a row can lie on a border


def launch_seam(n):
    """n rows, about half of them out of view, one exactly on each border of the viewport (from 8 rows on; the last row
    of the table among them)."""
    rng = np.random.default_rng(200 + n)
    (y_min, x_min), (y_max, x_max) = LAUNCH_VIEW
    rows = ordinary_rows(rng, n, x_min - 13, x_max + 13, y_min - 13, y_max + 13, 0.05, 2.0)
    if n == 1:
        rows[0, :2] = (31.7, 12.2)
    if n >= 8:
        rows[0, :2] = (x_min, 20.0)
        rows[n // 3, :2] = (x_max, 30.0)
        rows[2 * n // 3, :2] = (40.0, y_min)
        rows[n - 1, :2] = (50.0, y_max)
    return case(rows, 1.0, LAUNCH_VIEW)


# ---------------------------------------------------------------------------
# histogram
# ---------------------------------------------------------------------------
def hist_one_pixel():
    rng = np.random.default_rng(13)
    n = 70_000
    x = rng.uniform(10.001, 10.999, n)
    y = rng.uniform(10.001, 10.999, n)
    lp = np.full(n, 0.1)
    return case(np.stack([x, y, lp, lp], axis=1), 1.0, [(0.0, 0.0), (33.0, 31.0)])


def hist_borders():
    """Rows one float32 step inside each border, at a non-integer oversampling (84 x 84 pixels)."""
    (y_min, x_min), (y_max, x_max) = LAUNCH_VIEW
    lo_x, hi_x = np.nextafter(np.float32(x_min), np.float32(np.inf)), np.nextafter(np.float32(x_max), np.float32(-np.inf))
    lo_y, hi_y = np.nextafter(np.float32(y_min), np.float32(np.inf)), np.nextafter(np.float32(y_max), np.float32(-np.inf))
    rows = [(x, y, 0.1, 0.1) for x in (lo_x, hi_x, 30.0) for y in (lo_y, hi_y, 30.0)]
    rows += [(x_min, 30.0, 0.1, 0.1), (x_max, 30.0, 0.1, 0.1), (30.0, y_min, 0.1, 0.1), (30.0, y_max, 0.1, 0.1)]
    return case(rows, 1.3, LAUNCH_VIEW)


# ---------------------------------------------------------------------------
# scratch reuse
# ---------------------------------------------------------------------------
def scratch_cases():
    """A 160 x 160 render with every tile in use, a one-tile render, and the 160 x 160 viewport with 3 tiles in use."""
    rng = np.random.default_rng(14)
    large = case(ordinary_rows(rng, 1500, 0.1, 63.9, 0.1, 63.9, 0.02, 0.8), 2.5, VIEW64)
    small = case(ordinary_rows(rng, 5, 1, 30, 1, 30, 0.1, 1.0), 1.0, [(0.0, 0.0), (31.0, 31.0)])
    sparse = case(np.concatenate([ordinary_rows(rng, 40, 1, 11, 1, 11, 0.02, 0.3), ordinary_rows(rng, 40, 53, 63, 53, 63, 0.02, 0.3),
                                  ordinary_rows(rng, 3, 30, 32, 20, 22, 0.02, 0.1)]), 2.5, VIEW64)
    return large, small, sparse
