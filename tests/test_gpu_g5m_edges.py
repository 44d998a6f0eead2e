"""The G5M kernels (csrc/g5m.hip) where only the device can go wrong (cases: tests/_g5m_edge_cases.py; their CPU tier:
tests/test_g5m_edges_host.py).

Seams: a fixed fit at every size at which a wavefront or the workgroup gets its first idle lane or its first lane with
two rows, against what the reference recorded (tests/golden/g5m_edge_cases.npz), and in scratch equal to LDS in bits.
The residence bound as a product n K.  A mixed table whose clusters live on both sides of the bound in one round and
stop in different rounds: every cluster's result is, in bits, what the cluster gives alone, wherever it stands.  The
search state machine at max_rounds 0 and 1, at k_max, and as the progress callback sees it.  The clamp of a first draw
outside the cluster.  Nothing is left behind in the scratch slots."""
import math

import numpy as np
import pytest
import torch

from conftest import golden
from _g5m_cases import same
from _g5m_edge_cases import (BOUNDS, MIN_LOCS, MIXED, NO_MODEL, RESIDENCE, SEAM_KS, SEAM_SIZES, Table, build_host, check_fixed, cluster,
                             host_fit, mixed, orders, parts, residence, seam)

from picasso_amd import _lib, backend

pytestmark = pytest.mark.gpu

E = golden("g5m_edge_cases")
KW = dict(min_locs=MIN_LOCS, sigma_bounds=BOUNDS)


def same_models(a, b):
    return all(same(p, q) for p, q in zip(a[2:], b[2:]))


def search(t, **kw):
    return backend.g5m_search(t.x, t.y, t.lp, t.offsets, **KW, **kw)


def fixed(t, K, min_locs=MIN_LOCS, **kw):
    return backend.g5m_fit_fixed(t.x, t.y, t.lp, t.offsets, K, min_locs=min_locs, sigma_bounds=BOUNDS, **kw)


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return build_host(tmp_path_factory.mktemp("g5m_edges_host"))


# ---- seams ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SEAM_SIZES)
def test_fixed_fit_at_the_seams_of_the_workgroup(n):
    t = Table([seam(n)])
    for K in SEAM_KS:
        lds = fixed(t, K)
        check_fixed(lds.of(0), E, n, K)
        assert (lds.of(0) is None) == ((n, K) in NO_MODEL)
        assert same_models(lds, fixed(t, K, force_scratch=True)), (n, K)


# n K = 4096 and the first product above it, on K sites: a model of K components comes out on both sides
@pytest.mark.parametrize("n,K,min_locs,grid", RESIDENCE)
def test_the_residence_bound_is_a_product(n, K, min_locs, grid):
    lds, max_k, _ = backend.g5m_limits()
    assert n * K == lds < (n + 1) * K and K <= max_k
    for rows in (n, n + 1):
        t = residence(rows, K, grid)
        a, b = fixed(t, K, min_locs), fixed(t, K, min_locs, force_scratch=True)
        assert a.info[0, 0] == K == a.info[0, 3] and a.info[0, 1] >= 1 and np.isfinite(a.bic[0]) and a.model[0].all(), (rows, K)
        assert same_models(a, b), (rows, K)


# ---- batch invariance -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def alone():
    """name of MIXED -> the search of that cluster alone."""
    return {n: search(Table([seam(n)])) for n in MIXED}


@pytest.fixture(scope="module")
def batches():
    """order -> (positions, the table in that order, its search)."""
    out = {}
    for name, perm in orders().items():
        t = Table(seam(MIXED[i]) for i in perm)
        out[name] = (perm, t, search(t))
    return out


def test_the_draws_of_a_cluster_do_not_depend_on_its_place():
    """What lets the comparisons below be direct: backend.g5m_table draws per (size, cap), so a cluster alone and the same
    cluster in a table read the same first draws and uniforms."""
    t = mixed()
    caps = np.minimum(backend.G5M_MAX_K, t.sizes // MIN_LOCS)
    table, first, uniform = backend.g5m_table(t.sizes, caps)
    for c in range(len(t.sizes)):
        if caps[c] < 1:
            continue
        t1, f1, u1 = backend.g5m_table(t.sizes[c:c + 1], caps[c:c + 1])
        seeds, stride = max(int(caps[c]), 3), int(table[c, 3])
        assert stride == t1[0, 3] and same(first[table[c, 1]:table[c, 1] + seeds], f1[:seeds])
        assert same(uniform[table[c, 2]:table[c, 2] + seeds * stride], u1[:seeds * stride])


@pytest.mark.parametrize("order", list(orders()))
def test_a_cluster_searched_in_a_table_gives_the_bits_it_gives_alone(order, alone, batches):
    perm, t, batch = batches[order]
    assert sorted(perm) == list(range(len(MIXED))) and (order == "built") == (list(perm) == list(range(len(MIXED))))
    for p, i in enumerate(perm):
        for got, want in zip(parts(batch, p), parts(alone[MIXED[i]], 0)):
            assert same(got, want), (order, p, MIXED[i])
    # the table is the one the CPU tier describes: rounds on both sides of the bound, clusters that stop in different rounds
    last, lds = batch.info[:, 3], backend.g5m_limits()[0]
    assert len(set(last.tolist())) >= 4 and last.min() == 0
    assert any((t.sizes[last >= K] * K > lds).any() and (t.sizes[last >= K] * K <= lds).any() for K in range(1, int(last.max()) + 1))


def test_a_cluster_fitted_from_given_means_in_a_table_gives_the_bits_it_gives_alone():
    # one row cannot be fitted with two components: the clusters behind it stand one place further in the table than in
    # the list of the fitted ones
    sizes, K = (63, 1, 257, 129), 2
    clusters = [seam(n) if n in SEAM_SIZES else cluster(n) for n in sizes]
    t = Table(clusters)
    means_init = np.array([[[5.0, 5.0], [5.4, 5.2]], [[5.0, 5.0], [5.0, 5.0]], [[5.1, 5.05], [5.7, 5.0]], [[5.8, 5.0], [5.2, 5.1]]])
    batch = fixed(t, K, means_init=means_init)
    assert not same_models(batch, fixed(t, K))                 # the given means are used
    for c, n in enumerate(sizes):
        one = fixed(Table([clusters[c]]), K, means_init=means_init[c:c + 1])
        assert (one.of(0) is not None) == (n >= K)
        for got, want in zip(parts(batch, c), parts(one, 0)):
            assert same(got, want), n


def assigned_parts(out, t, models, c):
    s = slice(int(models.start[c]), int(models.start[c] + models.cap[c]))
    return (out.label[t.rows(c)], out.log_likelihood[t.rows(c)], out.stats[s], out.n_events[s], out.group_ll[c:c + 1], out.col_means[:, s])


@pytest.mark.parametrize("order", list(orders()))
def test_a_cluster_assigned_in_a_table_gives_the_bits_it_gives_alone(order, batches):
    perm, t, models = batches[order]
    extra = np.random.default_rng(11).uniform(500, 5000, (1, len(t.x)))
    out = backend.g5m_assign(t.x, t.y, t.lp, t.frame, t.offsets, models, extra, f32=True, frame_u32=True)
    seen = set()
    for p, i in enumerate(perm):
        cap = int(models.cap[p])
        s = slice(int(models.start[p]), int(models.start[p]) + cap)
        one_t = Table([t.clusters[p]])
        one_m = backend.G5MModels(np.zeros(1, np.int64), models.cap[p:p + 1], np.ascontiguousarray(models.model[:, s]),
                                  np.ascontiguousarray(models.imodel[:, s]), models.info[p:p + 1].copy(), models.bic[p:p + 1].copy())
        one = backend.g5m_assign(one_t.x, one_t.y, one_t.lp, one_t.frame, one_t.offsets, one_m, extra[:, t.rows(p)], f32=True, frame_u32=True)
        for got, want in zip(assigned_parts(out, t, models, p), assigned_parts(one, one_t, one_m, 0)):
            assert same(got, want), (order, p, MIXED[i])
        if models.info[p, 0] == 0:                               # no model: rows and slots stay what the caller's arrays held
            assert not out.label[t.rows(p)].any() and not out.log_likelihood[t.rows(p)].any() and out.group_ll[p] == 0
            seen.add("none")
        else:
            valid = models.imodel[1, s][:models.info[p, 1]].tolist()
            assert out.label[t.rows(p)].max() < len(valid)
            seen.add("prefix" if valid == list(range(len(valid))) else "no prefix")
    assert seen == {"none", "prefix", "no prefix"}


# ---- the search state machine ---------------------------------------------------------------------------------------------
def test_one_round_without_a_better_bic_ends_the_search_where_the_host_build_ends_it(host):
    t = mixed()
    got, want = search(t, max_rounds=1), host_fit(host, t, max_rounds=1)
    assert same(got.info[:, 3], want.info[:, 3]) and len(set(got.info[:, 3].tolist())) >= 3
    assert same(got.info[:, :2], want.info[:, :2])
    assert same(search(t).info[:, 3], host_fit(host, t).info[:, 3])


class Dev:
    """A table and its draws on the device, for the ``_dev`` entry points."""

    def __init__(self, t, caps, first=None):
        self.t, self.caps, self.total = t, np.asarray(caps, np.int64), int(np.sum(caps))
        self.table, drawn, uniform = backend.g5m_table(t.sizes, self.caps)
        self.first = drawn if first is None else first
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()      # noqa: E731
        self.d = [up(a) for a in (t.x, t.y, t.lp, t.offsets, self.table, self.first, uniform)]
        C = len(t.sizes)
        self.model, self.imodel = torch.zeros((5, self.total), dtype=torch.float64, device="cuda"), torch.zeros((2, self.total), dtype=torch.int32, device="cuda")
        self.info, self.bic = torch.zeros((C, 4), dtype=torch.int32, device="cuda"), torch.zeros(C, dtype=torch.float64, device="cuda")

    def results(self):
        start = np.cumsum(self.caps) - self.caps
        return backend.G5MModels(start, self.caps, *(a.cpu().numpy() for a in (self.model, self.imodel, self.info, self.bic)))

    def search(self, max_rounds):
        torch.cuda.synchronize()
        with _lib.lock():
            _lib.call("pmi_g5m_fit_dev", *(a.data_ptr() for a in self.d[:4]), len(self.t.sizes), len(self.t.x), *(a.data_ptr() for a in self.d[4:]),
                      MIN_LOCS, BOUNDS[0], BOUNDS[1], max_rounds, 0, self.model.data_ptr(), self.imodel.data_ptr(), self.total,
                      self.info.data_ptr(), self.bic.data_ptr(), None, None, None)
        return self.results()

    def fixed(self, K):
        torch.cuda.synchronize()
        with _lib.lock():
            _lib.call("pmi_g5m_fit_fixed_dev", *(a.data_ptr() for a in self.d[:4]), len(self.t.sizes), len(self.t.x), *(a.data_ptr() for a in self.d[4:]),
                      None, K, MIN_LOCS, BOUNDS[0], BOUNDS[1], 0, self.model.data_ptr(), self.imodel.data_ptr(), self.total,
                      self.info.data_ptr(), self.bic.data_ptr(), None)
        return self.results()


def test_no_round_at_all_writes_what_the_search_starts_from_and_nothing_else():
    t = mixed()
    dev = Dev(t, np.minimum(backend.G5M_MAX_K, t.sizes // MIN_LOCS))
    dev.model.fill_(-7.25), dev.imodel.fill_(-77), dev.info.fill_(5), dev.bic.fill_(1.0)
    got = dev.search(0)
    assert (got.model == -7.25).all() and (got.imodel == -77).all() and got.model.size == 5 * dev.total > 0
    assert not got.info.any() and np.isposinf(got.bic).all()
    host_form = search(t, max_rounds=0)
    assert not host_form.model.any() and not host_form.imodel.any() and not host_form.info.any() and np.isposinf(host_form.bic).all()
    # the same arrays, searched: a cluster's chosen K components are written and no slot beyond them
    got, full = dev.search(3), search(t)
    assert same(got.info, full.info) and same(got.bic, full.bic)
    for c in range(len(t.sizes)):
        s0, K, end = int(full.start[c]), int(full.info[c, 0]), int(full.start[c] + full.cap[c])
        assert same(got.model[:, s0:s0 + K], full.model[:, s0:s0 + K]) and same(got.imodel[:, s0:s0 + K], full.imodel[:, s0:s0 + K])
        assert (got.model[:, s0 + K:end] == -7.25).all() and (got.imodel[:, s0 + K:end] == -77).all()


def test_k_max_ends_the_search_of_19_and_20_rows():
    t = Table([seam(19), seam(20)])
    info = search(t).info
    # k_max 1 and 2; after K = 1 at most one round has gone by without a better BIC, so 20 rows are fitted with K = 2 as well
    assert info[:, 3].tolist() == [1, 2] and info[0, 0] == 1 and 1 <= info[1, 0] <= 2


def test_the_progress_callback_sees_every_round_once():
    t, calls = mixed(), []
    got = search(t, progress=lambda r, n, ms: calls.append((r, n, ms)))
    last = got.info[:, 3]
    assert [c[0] for c in calls] == list(range(1, int(last.max()) + 1)) and len(calls) >= 4
    assert [c[1] for c in calls] == [int((last >= K).sum()) for K in range(1, int(last.max()) + 1)]
    assert all(math.isfinite(c[2]) and c[2] >= 0 for c in calls)
    assert same_models(got, search(t))


# ---- the clamp of a first draw outside the cluster ------------------------------------------------------------------------
def test_a_first_draw_outside_the_cluster_is_the_nearest_row_inside():
    sizes, K = (63, 129, 65), 2
    t = Table(seam(n) for n in sizes)
    caps = np.full(3, K, np.int64)
    table, drawn, _ = backend.g5m_table(t.sizes, caps)
    mid = slice(int(table[1, 1]), int(table[1, 1]) + 3)
    assert len({int(table[c, 1]) for c in range(3)}) == 3 and drawn.dtype == np.int32

    def run(value):
        first = drawn.copy()
        if value is not None:
            first[mid] = value
        return Dev(t, caps, first).fixed(K)
    plain = run(None)
    assert same_models(plain, fixed(t, K))
    n = sizes[1]
    for inside, outside in ((0, (-1, -2 ** 31)), (n - 1, (n, n + 1000, 2 ** 31 - 1))):
        want = run(inside)
        assert want.of(1) is not None
        for value in outside:
            got = run(value)
            assert same_models(got, want), value
            for c in (0, 2):
                for p, q in zip(parts(got, c), parts(plain, c)):
                    assert same(p, q), (value, c)


# ---- nothing is left behind -------------------------------------------------------------------------------------------------
def test_the_scratch_slots_carry_nothing_from_call_to_call():
    t, small = mixed(), Table([seam(min(SEAM_SIZES))])
    _lib.call("pmi_release_scratch")                           # every slot starts empty
    a = search(t)                                              # the responsibilities' slot grows in the third round
    s1, s2 = fixed(small, 1), fixed(small, 1, force_scratch=True)     # ... is not needed, then needed for 3 x 10 values
    b = search(t)
    assert same_models(a, b) and same_models(s1, s2) and a.info[:, 3].max() >= 3
    _lib.call("pmi_release_scratch")
    assert same_models(fixed(small, 1, force_scratch=True), s1) and same_models(search(t), a)
