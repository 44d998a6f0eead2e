"""CPU tier of the G5M edge cases (tests/_g5m_edge_cases.py): the inputs decide what they claim to decide.

Every seam cluster is fitted with K = 1, 2 and 3 by the host build of csrc/g5m_core.h (tests/g5m_host_driver.cpp, a team
of one lane) and by the NumPy oracle (tests/golden/_g5m_restate.py): the two agree on every choice and, within the
tolerances tests/golden/g5m_cases.npz records, on every float, and both agree the same way with what the reference's own
functions recorded (tests/golden/g5m_edge_cases.npz).  The mixed table holds the rounds the device tier is after, as the
host build's ``info`` shows."""
import os
import sys

import numpy as np
import pytest

from conftest import GOLDEN, golden
from _g5m_cases import close, same
from _g5m_edge_cases import (BOUNDS, MIN_LOCS, MIXED, NO_MODEL, RESIDENCE, SEAM_KS, SEAM_SIZES, Table, build_host, check_fixed, host_fit, key,
                             mixed, residence, seam)

sys.path.insert(0, GOLDEN)
import _g5m_restate as rs  # noqa: E402
import make_goldens_g5m as mk  # noqa: E402
import make_goldens_g5m_edges as mke  # noqa: E402

from picasso_amd import backend  # noqa: E402

E = golden("g5m_edge_cases")


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return build_host(tmp_path_factory.mktemp("g5m_edges_host"))


def as_fitted(m):
    return None if m is None else (m["weights_"], m["means_"], m["covariances_"], m["precisions_cholesky_"], m["valid_idx"],
                                   m["n_locs"], m["converged"])


def test_the_seam_sizes_are_the_ones_the_workgroup_has():
    assert SEAM_SIZES == (10, 19, 20, 63, 64, 65, 127, 129, 255, 256, 257, 511, 513, 1366) and SEAM_KS == (1, 2, 3)
    assert list(E["seam_sizes"]) == list(SEAM_SIZES) and list(E["seam_ks"]) == list(SEAM_KS)
    lds, _, lanes = backend.g5m_limits()
    assert lanes == 256 and all(s in SEAM_SIZES for w in (64, lanes) for s in (w - 1, w, w + 1))
    assert 1366 * 2 <= lds < 1366 * 3
    for n in SEAM_SIZES:
        c = seam(n)
        assert c.n == n and all(same(getattr(c, k), E[f"n{n}/in_{k}"]) for k in ("x", "y", "lp", "frame")), n
        assert same(np.float64(np.float32(c.x)), c.x) and same(np.float64(np.float32(c.y)), c.y) and np.all(np.diff(c.frame) >= 0)
    # the fits without a model are the listed ones: at every seam of a wavefront and of the workgroup K = 1, 2 and 3 all
    # (K = 1 and 2 at the least) put numbers against the record
    assert tuple((n, K) for n in SEAM_SIZES for K in SEAM_KS if int(E[key(n, K) + "K"]) == 0) == NO_MODEL
    assert all(n in (10, 127, 255, 256, 511) and K > 1 for n, K in NO_MODEL)


def test_the_residence_cases_straddle_the_bound_and_give_a_model(host):
    lds, max_k, _ = backend.g5m_limits()
    assert len(RESIDENCE) >= 4 and any(K >= 64 and n <= 64 for n, K, _, _ in RESIDENCE)      # ... one with many components and few rows
    for n, K, min_locs, grid in RESIDENCE:
        assert n * K == lds < (n + 1) * K and K <= max_k
        for rows in (n, n + 1):
            models = host_fit(host, residence(rows, K, grid), k_fixed=K, min_locs=min_locs)
            assert models.info[0].tolist() == [K, K, 1, K] and np.isfinite(models.bic[0]), (rows, K)


@pytest.mark.parametrize("n", SEAM_SIZES)
def test_host_build_and_oracle_agree_on_the_seam_fits(n, host):
    c = seam(n)
    for K in SEAM_KS:
        want = rs.fit_fixed(c.X, c.lp, K, MIN_LOCS, BOUNDS)
        got = host_fit(host, Table([c]), k_fixed=K).of(0)
        check_fixed(as_fitted(want), E, n, K), check_fixed(got, E, n, K)
        assert (want is None) == (got is None), (n, K)
        if want is None:
            continue
        w, m, cov, pc, valid, n_locs, converged = got
        assert list(valid) == list(want["valid_idx"]) and list(n_locs) == list(want["n_locs"]) and converged == want["converged"], (n, K)
        close(w, want["weights_"], "weights"), close(m, want["means_"], "means")
        close(cov, want["covariances_"], "covariances"), close(pc, want["precisions_cholesky_"], "precisions_cholesky")


def rounds_of(models, sizes):
    """From ``info``: per round K the clusters fitted in it (those whose last K tried is at least K)."""
    last = models.info[:, 3]
    return {K: [c for c in range(len(sizes)) if last[c] >= K] for K in range(1, int(last.max()) + 1)}


def test_the_mixed_table_holds_the_rounds_it_is_for(host):
    t = mixed()
    assert len(t.sizes) == len(MIXED) >= 12 and t.offsets[-1] < 4000
    assert 1366 in MIXED and 9 in MIXED[1:-1] and "satellite" in MIXED and all(n in SEAM_SIZES for n in MIXED if n not in (9, "satellite"))
    models = host_fit(host, t)
    sizes, info, lds = t.sizes, models.info, backend.G5M_LDS_RESP
    chosen, last = info[:, 0], info[:, 3]
    rounds = rounds_of(models, sizes)
    # a round with clusters on both sides of the bound
    assert any(any(sizes[c] * K <= lds for c in act) and any(sizes[c] * K > lds for c in act) for K, act in rounds.items())
    # a cluster that crosses it during its own search
    assert any(sizes[c] <= lds < sizes[c] * last[c] for c in range(len(sizes)))
    # the active list shrinks, and stays non-empty, after at least three rounds: position and cluster drift apart
    shrinks = [K for K in rounds if K + 1 in rounds and len(rounds[K + 1]) < len(rounds[K])]
    assert len(shrinks) >= 3, shrinks
    # the order of the survivors is not the order of the table's head: some cluster is fitted after a neighbour before it stopped
    assert any(act != list(range(len(act))) for act in rounds.values())
    # never searched: 9 rows with min_locs 10
    never = [c for c in range(len(sizes)) if sizes[c] // MIN_LOCS == 0]
    assert [int(sizes[c]) for c in never] == [9] and all(last[c] == 0 and chosen[c] == 0 for c in never)
    assert 0 < never[0] < len(sizes) - 1 and last[never[0] - 1] > 0 and last[never[0] + 1] > 0
    # stopped by k_max, not by the rounds counter: the rounds since the best model are fewer than max_rounds
    k_max = np.minimum(backend.G5M_MAX_K, sizes // MIN_LOCS)
    by_k_max = [c for c in range(len(sizes)) if 0 < k_max[c] == last[c] and last[c] - chosen[c] < 3]
    assert {19, 20} <= {int(sizes[c]) for c in by_k_max}
    assert [int(k_max[list(sizes).index(n)]) for n in (19, 20)] == [1, 2]
    # ... and the others by the counter
    assert any(chosen[c] > 0 and last[c] - chosen[c] == 3 and last[c] < k_max[c] for c in range(len(sizes)))
    # the satellite's chosen model keeps a valid_idx that is no prefix
    s = MIXED.index("satellite")
    valid = list(models.of(s)[4])
    assert valid != list(range(len(valid))) and len(valid) < chosen[s]


def test_the_edge_record_regenerates():
    """The committed g5m_edge_cases.npz is what make_goldens_g5m_edges.py mints from the reference tree today."""
    if not os.path.isfile(mk.G5M_PY):
        pytest.skip("reference tree not present")
    out = mke.record()
    assert sorted(out) == sorted(E.files)
    for k, v in out.items():
        assert same(np.asarray(v), E[k]), k
    assert os.path.getsize(mke.OUT) <= mke.MAX_BYTES
    assert all(key(n, K) + "K" in E.files for n in SEAM_SIZES for K in SEAM_KS)
