"""GPU tier of the cluster combine (csrc/combine.hip): every table the reference recorded
(tests/golden/combine_cases.npz) through the public functions, equal in column names, order, dtypes, index and every
bit (any NaN equals any NaN); the two functions chained; the work assignment of the distance kernel on very unequal
groups; the statistics kernel on very unequal segments, one of them longer than one buffer of NumPy's reduction; and a
smaller table after a larger one.  No tolerance anywhere."""
import json
import sys

import numpy as np
import pandas as pd
import pytest

from conftest import GOLDEN, golden

sys.path.insert(0, GOLDEN)
import _combine_restate as rs  # noqa: E402
import make_goldens_combine as mk  # noqa: E402

from picasso_amd import backend, postprocess  # noqa: E402

pytestmark = pytest.mark.gpu

G = golden("combine_cases")
COMBINE = [str(c) for c in G["combine_case_names"]]
DIST = [str(c) for c in G["dist_case_names"]]
EDGES = json.loads(str(G["edges"]))


def inputs(p):
    return {str(c): G[p + "in_" + str(c)] for c in G[p + "in_columns"]}


def assert_frame(got, want, dtypes=None):
    """``want``: column -> array, in order."""
    assert list(got.columns) == list(want)
    assert isinstance(got.index, pd.RangeIndex) and got.index.start == 0 and got.index.step == 1
    assert len(got) == len(next(iter(want.values())))
    for i, c in enumerate(want):
        a = got[c].to_numpy()
        if dtypes is not None:
            assert str(a.dtype) == str(dtypes[i]), c
        assert mk.same(a, want[c]), (c, np.flatnonzero(~(a == want[c]))[:8])


def golden_table(p):
    return {str(c): G[p + "out_" + str(c)] for c in G[p + "columns"]}, [str(d) for d in G[p + "dtypes"]]


@pytest.mark.parametrize("name", COMBINE)
def test_cluster_combine_equals_the_reference(name):
    p = "combine/" + name + "/"
    assert_frame(postprocess.cluster_combine(pd.DataFrame(inputs(p))), *golden_table(p))


@pytest.mark.parametrize("name", DIST)
def test_cluster_combine_dist_equals_the_reference(name):
    p = "dist/" + name + "/"
    got = postprocess.cluster_combine_dist(pd.DataFrame(inputs(p)), mk.pixelsize_from(G[p + "pixelsize"]))
    assert_frame(got, *golden_table(p))


def test_combine_then_distances():
    locs = pd.DataFrame(inputs("combine/c_3d_f32_labels_f64/"))
    combined = postprocess.cluster_combine(locs)
    assert_frame(combined, *golden_table("combine/c_3d_f32_labels_f64/"))
    assert_frame(postprocess.cluster_combine_dist(combined), *golden_table("dist/k_after_combine_3d/"))


def test_zero_weight_sum_raises_numpys_error():
    i = [e["label"] for e in EDGES].index("zero weight sum")
    cols = {str(c): G[f"edge{i}_in_{c}"] for c in G[f"edge{i}_columns"]}
    with pytest.raises(ZeroDivisionError) as err:
        postprocess.cluster_combine(pd.DataFrame(cols))
    assert str(err.value) == EDGES[i]["text"]


def test_many_small_groups_beside_a_large_one():
    """3 000 groups of 2 rows and one of 700 in one call: tiles of one lane pair next to a group of three tiles."""
    rng = np.random.default_rng(21)
    cols = mk.combined(rng, [2] * 1500 + [700] + [2] * 1500, True, shuffle=False)
    want = rs.cluster_combine_dist(cols, 130)
    assert_frame(postprocess.cluster_combine_dist(pd.DataFrame(cols), 130), want)
    flat = {c: v for c, v in cols.items() if c not in ("z", "lpz")}
    assert_frame(postprocess.cluster_combine_dist(pd.DataFrame(flat)), rs.cluster_combine_dist(flat))


def test_unequal_segments_share_a_wave():
    """4 096 segments of one row beside one of 20 000 rows: lanes with very unequal chains in one wave, and a chain
    longer than one 8192-element buffer of NumPy's reduction."""
    cols = mk.sweep_table()
    assert_frame(postprocess.cluster_combine(pd.DataFrame(cols)), rs.cluster_combine(cols))


def test_a_smaller_table_after_a_larger_one():
    """The arena is reused: what the larger call left behind must not reach the smaller one."""
    large, small = "combine/a_2d_f32_u32_i32/", "combine/g_sorted_table/"
    assert_frame(postprocess.cluster_combine(pd.DataFrame(inputs(large))), *golden_table(large))
    assert_frame(postprocess.cluster_combine(pd.DataFrame(inputs(small))), *golden_table(small))
    assert_frame(postprocess.cluster_combine_dist(pd.DataFrame(inputs("dist/i_3d_none/"))), *golden_table("dist/i_3d_none/"))
    assert_frame(postprocess.cluster_combine_dist(pd.DataFrame(inputs("dist/j_2d_shuffled/"))), *golden_table("dist/j_2d_shuffled/"))


def test_order_is_the_lexsort():
    cols = inputs("combine/f_300_small/")
    groups = backend.CombineGroups(cols["group"], cols["cluster"])
    order, start, seg_group, seg_cluster, group_start = rs.segments(cols["group"], cols["cluster"])
    assert np.array_equal(groups.order(), order) and np.array_equal(groups.offsets, start)
    assert np.array_equal(groups.unique, seg_group) and np.array_equal(groups.clusters, seg_cluster)
    assert np.array_equal(groups.group_offsets, group_start) and groups.n_outer == 5 and groups.n_groups == 300
    # the table is one the group statistics take as it is
    (mean, std), = backend.group_mean_std(groups, [cols["frame"]])
    (mean2, std2), = backend.combine_stats(groups, [cols["frame"]])[0]
    assert mk.same(mean, mean2) and mk.same(std, std2)
