"""CPU tier of pick_similar: the restatement (tests/golden/_similar_restate.py) against the goldens minted from the
reference, the goldens against the reference tree when it is present, the host filter ``pmi_similar_filter`` against the
restatement's greedy pass, the recorded signature, the ABI, and the Python layer of ``postprocess.pick_similar`` with the
two device calls replaced by the restatement."""
import inspect
import os
import warnings

import numpy as np
import pytest

from picasso_amd import _lib, backend, postprocess

from _similar_cases import CASES, G, assert_pairs, call, columns, mk, prs, rs, same_bits, table

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RAISING = [n for n in CASES if f"{n}/raises" in G.files]


def restated(name, details=False):
    info, picks, d, std_range, max_shifts, _ = call(name)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")          # the reference's own np.mean of an empty pick list warns
        return rs.pick_similar(columns(name), info, picks, d, std_range, max_shifts, details=details)


def test_the_cases_are_there():
    assert len(CASES) >= 14 and RAISING == ["pick_without_members"]
    kinds = {n: call(n)[5] for n in CASES}
    assert set(kinds.values()) == {"generic", "dyadic"}
    for n, kind in kinds.items():
        if kind == "dyadic":
            c = columns(n)
            assert c["x"].dtype == np.float32 and (c["x"] * 64 == np.round(c["x"] * 64)).all() and (c["y"] * 64 == np.round(c["y"] * 64)).all()
    dtypes = {(str(columns(n)["x"].dtype), str(columns(n)["y"].dtype)) for n in CASES}
    assert {("float32", "float32"), ("float64", "float64"), ("float32", "float64")} <= dtypes
    assert {type(call(n)[2]) for n in CASES} == {int, float}
    assert {call(n)[4] for n in CASES} == {1, 2, 500}


@pytest.mark.parametrize("name", CASES)
def test_restatement_reproduces_the_golden(name):
    if name in RAISING:
        with pytest.raises(ZeroDivisionError):
            restated(name)
        assert str(G[name + "/raises"]) == "ZeroDivisionError"
        return
    xs, ys = restated(name)
    assert same_bits(xs, G[name + "/out_x"]) and same_bits(ys, G[name + "/out_y"])


def test_goldens_regenerate():
    """The committed similar_cases.npz is what make_goldens_similar.py mints from the reference tree today."""
    if not os.path.isfile(mk.POSTPROCESS_PY):
        pytest.skip("reference tree not present")
    ref = mk.load_reference()
    cases = mk.cases()
    assert list(cases) == CASES
    out = {}
    for name, case in cases.items():
        mk.mint(ref, name, case, out)
    mk.check_situations(ref, cases, out)
    for key, value in out.items():
        assert same_bits(value, G[key]), key
    assert str(G["signature"]) == str(inspect.signature(ref["pick_similar"]))


# ---- the host filter ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [n for n in CASES if n not in RAISING])
def test_filter_on_the_golden_candidates(name):
    _, picks, d, _, _, _ = call(name)
    D = restated(name, details=True)[2]
    cx, cy = D["shift"][0][D["cand"]], D["shift"][1][D["cand"]]
    px, py = [p[0] for p in picks], [p[1] for p in picks]
    got = backend.similar_filter(cx, cy, px, py, d ** 2, d)
    assert got.dtype == bool and np.array_equal(got, D["keep"])
    if name == "basic_f32":
        assert got.any() and not got.all()


@pytest.mark.parametrize("d", [1.0, 2, 0.375])          # dyadic: 30 + d - 30 == d
def test_filter_on_random_candidates(d):
    rng = np.random.default_rng(20261020)
    # given picks: a scatter, ten of them within a third of d of one point, two on one spot
    px = np.r_[rng.uniform(-5, 45, 40), 12.0 + rng.uniform(-0.15, 0.15, 10) * d, 30.0, 30.0]
    py = np.r_[rng.uniform(-5, 45, 40), 17.0 + rng.uniform(-0.15, 0.15, 10) * d, 8.0, 8.0]
    assert (np.hypot(px[40:50, None] - px[None, 40:50], py[40:50, None] - py[None, 40:50]) < d).all()
    # candidates: a scatter, a lattice of pitch d / 2 (distances of exactly d from one another: refused, the test is
    # strict), points around the crowded picks, and one at exactly d from a given pick
    lattice = np.stack(np.meshgrid(np.arange(20) * (d / 2), 20.0 + np.arange(20) * (d / 2)), -1).reshape(-1, 2)
    near = np.c_[12.0 + rng.uniform(-2, 2, 300) * d, 17.0 + rng.uniform(-2, 2, 300) * d]
    cand = np.concatenate([rng.uniform(-6, 46, (3000, 2)), lattice, near, [[30.0 + d, 8.0]]])
    cand = cand[rng.permutation(len(cand))]
    keep, who = rs.greedy(cand[:, 0], cand[:, 1], px, py, d ** 2)
    got = backend.similar_filter(cand[:, 0], cand[:, 1], px, py, d ** 2, d)
    assert np.array_equal(got, keep)
    assert 100 < keep.sum() < len(keep) and (who[~keep] < len(px)).any() and (who[~keep] >= len(px)).any()
    at = int(np.flatnonzero((cand[:, 0] == 30.0 + d) & (cand[:, 1] == 8.0))[0])
    assert not got[at] and (30.0 + d - 30.0) ** 2 == d ** 2          # exactly d away: not > d2


def test_filter_edges():
    none = np.zeros(0)
    assert backend.similar_filter(none, none, none, none, 4.0, 2.0).shape == (0,)
    assert backend.similar_filter([1.0, 1.0, 5.0], [1.0, 1.0, 5.0], none, none, 4.0, 2.0).tolist() == [True, False, True]
    # d == 0: only a point on the very spot is refused; every pick lands in one cell and is still checked
    assert backend.similar_filter([1.0, 1.0, 2.0], [1.0, 1.0, 2.0], [2.0], [2.0], 0, 0).tolist() == [True, False, False]
    with pytest.raises(_lib.HipBackendError, match="not finite"):
        backend.similar_filter([np.nan], [1.0], none, none, 4.0, 2.0)
    with pytest.raises(ValueError):
        backend.similar_filter([1.0], [1.0, 2.0], none, none, 4.0, 2.0)


# ---- names, signature, ABI -----------------------------------------------------------------------------------------
def test_name_and_signature():
    assert postprocess.SIMILAR_NAMES == ("pick_similar",)
    assert str(inspect.signature(postprocess.pick_similar)) == str(G["signature"])
    assert "pick_similar" not in postprocess.PICK_NAMES


def test_abi_version_and_symbols():
    L = _lib.load()
    assert L.pmi_version() >= 122
    header = open(os.path.join(ROOT, "include", "picasso_hip.h")).read()
    for name in ("pmi_similar_shift_dev", "pmi_similar_filter"):
        assert name in _lib.SYMBOLS and hasattr(L, name) and name in header
    assert backend.SIMILAR_MAX_SHIFTS == 500


def test_install_leaves_pick_similar_alone():
    import types
    from picasso_amd import localize
    mods = {n: types.ModuleType("picasso." + n) for n in
            ("localize", "gaussmle", "gausslq", "zfit", "render", "imageprocess", "postprocess", "aim")}
    for name in postprocess.SIMILAR_NAMES:
        setattr(mods["postprocess"], name, "theirs")
    localize.install(*[mods[n] for n in ("localize", "gaussmle", "gausslq", "zfit", "render", "imageprocess", "postprocess")],
                     picasso_aim=mods["aim"])
    assert all(getattr(mods["postprocess"], n) == "theirs" for n in postprocess.SIMILAR_NAMES)


# ---- the Python layer over the restatement -----------------------------------------------------------------------------
class FakeTable:
    def __init__(self, x_index, y_index, K, L):
        self.x_index, self.y_index, self.K, self.L, self.n = x_index, y_index, K, L, len(x_index)


def fake_circle(table, x, y, pick_x, pick_y, block_x, block_y, flags, r2):
    order = np.lexsort([table.x_index, table.y_index])
    xi, yi = table.x_index[order].astype(np.int64), table.y_index[order].astype(np.int64)
    outside = np.flatnonzero((yi >= table.K) | (xi >= table.L))
    p = int(outside[0]) if len(outside) else len(order)
    keys = ((yi << 32) | xi)[:p]
    S = np.result_type(x.dtype, y.dtype)
    xs, ys = x.astype(S)[order], y.astype(S)[order]
    out = []
    for px, py, bx, by, f in zip(pick_x, pick_y, block_x, block_y, flags):
        idx = [np.arange(*np.searchsorted(keys, [(k << 32) | ll, ((k << 32) | ll) + 1]))
               for k in range(by - 1, by + 2) if 0 <= k < table.K for ll in range(bx - 1, bx + 2) if 0 <= ll < table.L]
        idx = np.concatenate(idx) if idx else np.zeros(0, np.int64)
        out.append(order[idx[prs.circle_mask(xs[idx], ys[idx], px, py, r2, f)]])
    return prs.csr(out)


@pytest.fixture
def on_the_restatement(monkeypatch):
    """backend.BlockTable, picks_circle and similar_shift by the restatement; similar_filter stays the library's."""
    cap = {"max_shifts": 500, "size": None}

    def fake_shift(table, x, y, x_range, y_base, y_shift, x_r, y_r_base, y_r_shift, r2, gate, max_shifts=500):
        assert max_shifts == 500 and x_r.dtype == np.uint64
        grid = (x_range, y_base, y_shift, x_r.astype(np.int64), y_r_base.astype(np.int64), y_r_shift.astype(np.int64))
        return rs.shift(x, y, cap["size"], table.K, table.L, grid, r2, gate, cap["max_shifts"])[:4]

    monkeypatch.setattr(backend, "BlockTable", FakeTable)
    monkeypatch.setattr(backend, "picks_circle", fake_circle)
    monkeypatch.setattr(backend, "similar_shift", fake_shift)
    return cap


@pytest.mark.parametrize("name", CASES)
def test_python_layer_gives_the_golden_pairs(on_the_restatement, name):
    info, picks, d, std_range, max_shifts, _ = call(name)
    on_the_restatement.update(max_shifts=max_shifts, size=d / 2)
    df = table(name)
    before = df.copy()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        if name in RAISING:
            with pytest.raises(ZeroDivisionError):
                postprocess.pick_similar(df, info, picks, d, std_range)
        else:
            assert_pairs(postprocess.pick_similar(df, info, picks, d, std_range), name)
    assert df.equals(before)


def test_edges_before_the_device(on_the_restatement):
    info, picks, d, std_range, _, _ = call("basic_f32")
    on_the_restatement.update(size=d / 2)
    df = table("basic_f32")
    with pytest.raises(NotImplementedError, match="index_blocks"):
        postprocess.pick_similar(df, info, picks, d, index_blocks=(df, d / 2))
    # (an all-integer x or y list is decided from numba's typing in DESIGN N18 and not pinned here)
    # an integer beside a float in each coordinate is a float array: the integer types only that pick's own circle
    assert len(postprocess.pick_similar(df, info, [(20, 19.6), (25.2, 8)], d)) >= 2
