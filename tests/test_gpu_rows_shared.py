"""GPU tier: AIM, link and the clusterers share the scratch slots of csrc/rows_common.h without treading on each
other.  In one process an AimTable in each form is made, link and cluster calls run over the same slots, the tables
are counted, a larger table makes every slot grow, and the tables are counted again.  Every result equals what the
same call gave before the others ran, and the test-side restatements (tests/golden/_*_restate.py)."""
import sys

import numpy as np
import pytest

from conftest import GOLDEN

sys.path.insert(0, GOLDEN)
import _aim_restate as aim_rs  # noqa: E402
import _cluster_restate as cluster_rs  # noqa: E402
import _link_restate as link_rs  # noqa: E402

from picasso_amd import _lib, backend  # noqa: E402

pytestmark = pytest.mark.gpu

FIELD, RADIUS, N_FRAMES = 4.0, 0.3, 21
DARK, MIN_SAMPLES, MIN_LOCS = 3, 3, 2
D = 20 / 130
REL = (0.05, -0.02)


def table(n, seed):
    """n rows sorted by frame: float32 x / y in a 4 x 4 px field, frames 0..20, one float32 column to sum."""
    rng = np.random.default_rng(seed)
    frame = np.sort(rng.integers(0, N_FRAMES, n)).astype(np.uint32)
    x = rng.uniform(0, FIELD, n).astype(np.float32)
    y = rng.uniform(0, FIELD, n).astype(np.float32)
    photons = rng.uniform(100, 900, n).astype(np.float32)
    return frame, x, y, photons


def link_groups(frame, x, y):
    t = backend.LinkTable(frame, x, y, np.zeros(len(x), np.int32))
    lg, n_groups = t.link_groups(link_rs.squared(RADIUS), DARK + 1)
    return lg.cpu().numpy(), n_groups


@pytest.mark.parametrize("n", [1, 255, 257])
def test_modules_share_scratch(n):
    import torch
    frame, x, y, photons = table(n, n)
    group = np.zeros(n, np.int32)
    X = np.stack([x, y], axis=1).astype(np.float64)
    shifts, _ = aim_rs.shifts_xy(60 / 130, D, FIELD)
    W = FIELD / D
    n_frames = int(frame.max()) + 1                    # as cluster() takes it from the table
    fa = (0.2 * n_frames, 0.8 * n_frames, np.linspace(0, n_frames, 21))
    d_x, d_y = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
    d_rows = torch.arange(n, dtype=torch.int32, device="cuda")
    n_ref = (n + 1) // 2

    want_cc = aim_rs.roi_cc(aim_rs.keys(aim_rs.XY_F32, x[:n_ref], y[:n_ref], None, (0, 0), D, W),
                            aim_rs.keys(aim_rs.XY_F32, x, y, None, REL, D, W), shifts)
    want_lg = link_rs.link_groups(frame, x, y, RADIUS, DARK, group)
    want_sum = link_rs.ordered_sum(photons, want_lg, int(want_lg.max()) + 1)
    want_last = np.zeros(int(want_lg.max()) + 1, np.int32)
    want_last[want_lg] = np.arange(n)                 # rows ascend: the last row of a group is written last
    want_counts = cluster_rs.neighbour_counts(X, RADIUS)
    want_db = cluster_rs.dbscan(X, RADIUS, MIN_SAMPLES, MIN_LOCS)
    want_smlm = cluster_rs.cluster(X, RADIUS, MIN_LOCS, frame)

    def aim_table():
        return backend.AimTable(aim_rs.XY_F32, d_x, d_y, None, None, n_ref, D, W, W, shifts)

    def combine(lg, n_groups):
        count, _, _, last_row, sums = backend.link_combine(lg, n_groups, frame, [(backend.LINK_SUM, photons, None)])
        return count, last_row, sums[0]

    _lib.check(_lib.load().pmi_release_scratch(), "pmi_release_scratch")     # every slot starts empty
    try:
        # each call once, before any other module has used the slots
        backend.aim_set_dense_limit(0)
        first = aim_table()
        assert first.info()[0] == "sorted"
        first_cc = first.count(d_rows, *REL)
        first.close()
        first_lg, first_groups = link_groups(frame, x, y)
        first_combined = combine(first_lg, first_groups)
        points = backend.ClusterPoints(X)
        first_counts = points.counts(RADIUS)
        first_db = points.dbscan(RADIUS, MIN_SAMPLES, MIN_LOCS)
        first_smlm = points.smlm(RADIUS, MIN_LOCS, frame, *fa)

        # 1. a table in each form
        sorted_table = aim_table()
        backend.aim_set_dense_limit(1 << 28)
        dense_table = aim_table()
        assert sorted_table.info()[0] == "sorted" and dense_table.info()[0] == "dense"
        # 2. link
        lg, n_groups = link_groups(frame, x, y)
        combined = combine(lg, n_groups)
        # 3. cluster
        counts = points.counts(RADIUS)
        db = points.dbscan(RADIUS, MIN_SAMPLES, MIN_LOCS)
        smlm = points.smlm(RADIUS, MIN_LOCS, frame, *fa)
        # 4. the tables of step 1
        cc = [sorted_table.count(d_rows, *REL), dense_table.count(d_rows, *REL)]
        # 5. a 4x larger table: every slot of the link call grows
        big = table(4 * n, n + 1000)
        big_lg, _ = link_groups(*big[:3])
        cc += [sorted_table.count(d_rows, *REL), dense_table.count(d_rows, *REL)]
    finally:
        backend.aim_set_dense_limit(1 << 28)

    for got in [first_cc] + cc:
        assert got.dtype == np.int64 and np.array_equal(got, want_cc)
    assert want_cc.max() > 0
    for got, groups in ((first_lg, first_groups), (lg, n_groups)):
        assert got.dtype == np.int32 and np.array_equal(got, want_lg) and groups == want_lg.max() + 1
    for count, last_row, total in (first_combined, combined):
        assert np.array_equal(count, np.bincount(want_lg).astype(np.uint32))
        assert np.array_equal(last_row, want_last)
        assert total.dtype == np.float32 and np.array_equal(total.view(np.uint32), want_sum.view(np.uint32))
    assert np.array_equal(big_lg, link_rs.link_groups(*big[:3], RADIUS, DARK, np.zeros(4 * n, np.int32)))
    for got in (first_counts, counts):
        assert got.dtype == np.int32 and np.array_equal(got, want_counts)
    for got, want in ((first_db, want_db), (db, want_db), (first_smlm, want_smlm), (smlm, want_smlm)):
        assert got.dtype == np.int32 and np.array_equal(got, want)
