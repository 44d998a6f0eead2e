"""CPU tier of AIM's edge cases (tests/golden/aim_edge_cases.npz, minted by tests/golden/make_goldens_aim_edges.py from the
reference's intersection_max / intersection_max_z): the test-side restatement (tests/golden/_aim_restate.py) reproduces
every recorded roi_cc, every case holds what it was built for, and the device-tier cases of tests/test_gpu_aim_edges.py
sit on the constants of csrc/aim.hip as the sources state them today."""
import os
import sys

import numpy as np
import pytest

from conftest import GOLDEN, golden

sys.path.insert(0, GOLDEN)
import _aim_edges as ae  # noqa: E402
import _aim_restate as rs  # noqa: E402
import make_goldens_aim_edges as mke  # noqa: E402

CASES = [str(c) for c in golden("aim_edge_cases")["case_names"]]
I_MIN = -2 ** 31


@pytest.fixture(scope="module")
def g():
    return golden("aim_edge_cases")


def test_the_fixture_holds_every_case():
    assert CASES == ["wrap_hi_f64", "wrap_lo_f64", "wrap_f32_round_to_2p31", "ties_signs_f32", "ties_signs_f64",
                     "z_int_min_and_range_f32", "z_int_min_and_range_f64", "z_int_min_and_range_nonintegral_f32",
                     "z_int_min_and_range_nonintegral_f64", "multiplicity", "shifts_289"]
    assert os.path.getsize(os.path.join(GOLDEN, "aim_edge_cases.npz")) <= 200_000


@pytest.mark.parametrize("name", CASES)
def test_restatement_reproduces_every_recorded_roi_cc(g, name):
    n = 0
    for tag, s, roi, peak, mode, ref, tgt, rel, d, W, H, sh in rs.golden_rounds(g, name):
        got = rs.roi_cc(rs.keys(mode, *ref, (0, 0, 0), d, W, H), rs.keys(mode, *tgt, rel, d, W, H), sh)
        assert np.array_equal(got, roi), (name, tag, s)
        assert roi.sum() > 0
        n += 1
    assert n == len(g[name + "/rec_seg"]) == 2


@pytest.mark.parametrize("name", CASES)
def test_the_case_holds_what_it_is_for(g, name):
    mke.check(g, name)


def test_rel_is_added_in_the_precision_of_the_round(g):
    """float32(rel) added in float32 leaves a tie a tie where the float64 sum has left it: the two key modes put the row
    in different cells.  Segment 2 of the float32 cases runs at a rel that is no float32 value."""
    for name in ("shifts_289", "multiplicity"):
        tag, s, roi, peak, mode, ref, tgt, rel, d, W, H, sh = list(rs.golden_rounds(g, name))[1]
        assert mode == rs.XY_F32 and rel[0] != 0 and np.float64(np.float32(rel[0])) != rel[0]
    x = np.array([0.625], np.float32)                   # 2.5 cells: the tie goes to 2, anything above it to 3
    k32 = rs.keys(rs.XY_F32, x, x, None, (1e-9, 0.0), 0.25, 64.0)[0]
    k64 = rs.keys(rs.XY_F64, x, x, None, (1e-9, 0.0), 0.25, 64.0)[0]
    assert (k32, k64) == (2 + 2 * 64, 3 + 2 * 64)


def test_key_arithmetic_corners():
    """rint ties go to even, -0.0 is cell 0, and every non-finite coordinate or sum gives INT_MIN, in both precisions."""
    inf, nan = np.inf, np.nan
    for mode, t in ((rs.XY_F32, np.float32), (rs.XY_F64, np.float64)):
        x = np.array([0.125, 0.375, 0.625, -0.125, -0.375, -0.0, inf, -inf, nan, 1.0, inf], t)
        y = np.array([0.0, 0.0, 0.0, 0.0, 0.0, -0.0, 0.0, 0.0, 0.0, nan, -inf], t)
        k = rs.keys(mode, x, y, None, (0, 0), 0.25, 64.0)
        assert k.tolist() == [0, 2, 2, 0, -2, 0] + [I_MIN] * 5
    # float32 sums that round up to 2^31 leave the range; one float32 step below they stay
    k = rs.keys(rs.XY_F32, np.array([65472.0, 65471.0], np.float32), np.array([32767.0, 32767.0], np.float32), None, (0, 0),
                1.0, 65536.0)
    assert k.tolist() == [I_MIN, 2 ** 31 - 128]


def test_the_device_cases_sit_on_the_kernels_constants():
    K = ae.kernel_constants()
    assert K == {"BLOCK": ae.BLOCK, "MAX_SHIFTS": ae.MAX_SHIFTS, "GRID_FACTOR": ae.GRID_FACTOR, "MIN_HSIZE": ae.MIN_HSIZE,
                 "LOAD_FACTOR": ae.LOAD_FACTOR, "DENSE_LIMIT": ae.DENSE_LIMIT, "HASH_OPS": ae.HASH_OPS}
    B = K["BLOCK"]
    assert ae.SHIFT_COUNTS == (1, B - 1, B, B + 1, K["MAX_SHIFTS"])
    assert ae.PARTITION_ROWS == (0, 1, B - 1, B, B + 1, 2 * B + 1)
    assert ae.GRID_TAIL == B + 1 and ae.grid_stride_rows(256) == K["GRID_FACTOR"] * 256 * B + B + 1
    small, big = ae.HASH_SEGMENTS[0], ae.HASH_SEGMENTS[1]
    assert K["LOAD_FACTOR"] * small <= K["MIN_HSIZE"] < K["LOAD_FACTOR"] * big and ae.HASH_SEGMENTS == (small, big, small, big)
    # the fixture: 289 shifts are more than a block, and 257 rows of one key more than a block of rows
    assert 17 * 17 > B and max(mke.COUNTS) == B + 1 and {63, 64, 65} <= set(mke.COUNTS)
    # the default dense limit is the one the device tests restore
    assert K["DENSE_LIMIT"] == 1 << 28


def test_python_hash32_and_the_colliding_keys():
    def scalar(k):                  # the kernel's line, statement by statement, on Python ints
        k &= 0xFFFFFFFF
        k ^= k >> 16; k = k * 0x7feb352d & 0xFFFFFFFF; k ^= k >> 15; k = k * 0x846ca68b & 0xFFFFFFFF; k ^= k >> 16  # noqa: E702
        return k
    probe = [0, 1, 2, 1023, 1024, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFF, 123456789]
    assert [int(v) for v in ae.hash32(probe)] == [scalar(k) for k in probe]
    assert int(ae.hash32(-1)) == scalar(0xFFFFFFFF) and int(ae.hash32(I_MIN)) == scalar(0x80000000)
    assert ae.hash32(0) == 0 and len(set(ae.hash32(np.arange(1 << 16)).tolist())) == 1 << 16          # a bijection so far
    for hsize in (1024, 2048):
        end = ae.keys_hashing_to((hsize - 2, hsize - 1), hsize, 4)
        front = ae.keys_hashing_to((0, 1), hsize, 4, start=1)
        assert len(set(end.tolist()) | set(front.tolist())) == 8
        assert set((ae.hash32(end) & (hsize - 1)).tolist()) <= {hsize - 2, hsize - 1}
        assert set((ae.hash32(front) & (hsize - 1)).tolist()) <= {0, 1}
    # keys come back from the coordinates they were turned into
    k = np.array([I_MIN, -1, 0, 1, 2 ** 31 - 1, 123456789, -987654321])
    assert rs.keys(rs.XY_F64, *ae.xy_of_keys(k), None, (0, 0), ae.XY_D, ae.XY_W).tolist() == k.tolist()
    assert rs.keys(rs.Z_F64, *ae.xyz_of_keys(k), (0, 0, 0), ae.Z_D, ae.Z_W, ae.Z_H).tolist() == k.tolist()


@pytest.mark.parametrize("zmode", [False, True], ids=["xy", "z"])
def test_hash_case_probes_across_the_end_of_the_table(zmode):
    """Linear probing of the small segments' keys, in any order, at both table sizes they meet: more keys start in the
    last two slots than there are slots left, so a probe goes from slot hsize - 1 to slot 0, finds it taken and goes on.
    An increment without the `& (hsize - 1)` would index slot hsize there: one past the allocation."""
    ref, tgt, segs, step = ae.hash_case(zmode)
    assert [hi - lo for lo, hi in segs] == list(ae.HASH_SEGMENTS) and segs[1] == segs[3]
    assert set(tgt[610:620].tolist()) <= set(ref.tolist()) and set(tgt[:10].tolist()) <= set(ref.tolist())      # all inserted
    rng = np.random.default_rng(1)
    for (lo, hi), hsize in (((0, 10), ae.MIN_HSIZE), ((610, 620), 2 * ae.MIN_HSIZE)):
        keys = np.unique(tgt[lo:hi])
        home = ae.hash32(keys) & (hsize - 1)
        assert (home >= hsize - 2).sum() >= 4 and (home == 0).sum() >= 1 and (home == 1).sum() >= 1
        for _ in range(20):
            slots, past_end = {}, 0
            for i in rng.permutation(len(keys)):
                h, unmasked = int(home[i]), int(home[i])
                while h in slots:
                    unmasked += 1
                    h = (h + 1) & (hsize - 1)
                past_end += unmasked >= hsize
                slots[h] = keys[i]
            assert past_end >= 2 and len(slots) == len(keys)


@pytest.mark.parametrize("seg_len,n_frames", ae.PARTITION_SHAPES)
def test_partition_cases_hold_their_frames(seg_len, n_frames):
    for n in ae.PARTITION_ROWS:
        f = ae.partition_frames(n, seg_len, n_frames, n)
        assert len(f) == n
        if n >= 5:
            assert {0, -3, n_frames, n_frames + 1} <= set(f.tolist()) and (np.diff(f) < 0).any()
        offsets, sets = ae.partition_restated(f, seg_len, n_frames)
        assert len(offsets) == len(sets) + 1 and offsets[-1] == ((f >= 1) & (f <= n_frames)).sum()
        if n >= 255 and len(sets) > 4:
            assert len(sets[1]) == 0 and len(sets[3]) == 0 and len(sets[0]) > 0 and len(sets[-1]) > 0


def test_fixture_regenerates(g):
    """The committed aim_edge_cases.npz is what make_goldens_aim_edges.py mints from the reference tree today."""
    ref = os.environ.get("PICASSO_REFERENCE", "/root/reference")
    if not os.path.isfile(os.path.join(ref, "picasso", "aim.py")):
        pytest.skip("reference tree not present")
    arrays = mke.mint()
    assert sorted(arrays) == sorted(g.files)
    for k, v in arrays.items():
        assert np.array_equal(np.asarray(v), g[k], equal_nan=np.asarray(v).dtype.kind == "f"), k
        assert np.asarray(v).dtype == g[k].dtype, k
