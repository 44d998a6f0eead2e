"""G5M on the device (csrc/g5m.hip, picasso_amd/g5m.py) against what the reference's own functions recorded
(tests/golden/g5m_cases.npz): every choice equal, every float within the tolerance the record measured on the reference
itself; the LDS and the scratch path in bits; the device-array forms against the host-array forms in bits."""
import numpy as np
import pytest

from _g5m_cases import CASES, FIXED, G, INFO, check_model, check_tables, columns, frame_of, kwargs, same

from picasso_amd import __version__, _lib, backend, g5m

pytestmark = pytest.mark.gpu


def fixed_inputs(name):
    cols = columns(name)
    lp = frame_of(name)[["lpx", "lpy"]].mean(axis=1).to_numpy()
    return cols["x"].astype(np.float64), cols["y"].astype(np.float64), lp.astype(np.float64), np.array([0, len(lp)], np.int64)


@pytest.mark.parametrize("name", CASES)
def test_g5m_end_to_end(name):
    kw = kwargs(name)
    locs = frame_of(name)
    ids, rows, offsets = g5m.cluster_rows(locs, 10, kw.get("max_locs_per_cluster", np.inf))
    assert len(ids) == int(G[name + "/n_models"])
    if len(ids):
        models, _ = g5m.fit_clusters(locs, rows, offsets, min_locs=10, loc_prec_handle=kw.get("loc_prec_handle", "local"),
                                     sigma_bounds=kw.get("sigma_bounds", (0.8, 1.5)),
                                     max_rounds_without_best_bic=kw.get("max_rounds_without_best_bic", 3))
        for i in range(len(ids)):
            check_model(models.of(i), name, i)
            if models.of(i) is not None:
                from _g5m_cases import close
                close(models.bic[i], G[f"{name}/model{i}/bic"], "bic")
    check_tables(name, *g5m.g5m(locs, INFO, callback_parent=None, **kw), __version__)


@pytest.mark.parametrize("name", FIXED)
def test_fixed_fit_on_both_sides_of_the_lds_bound(name):
    x, y, lp, offsets = fixed_inputs(name)
    K = int(G[name + "/K"])
    assert (len(x) * K > backend.G5M_LDS_RESP) == (name == "fixed_above") and abs(len(x) * K - backend.G5M_LDS_RESP) <= K
    check_model(backend.g5m_fit_fixed(x, y, lp, offsets, K, min_locs=10, sigma_bounds=(0.8, 1.5)).of(0), name, 0)
    model = g5m.G5M_2D(K, 10, (0.8, 1.5)).fit(np.stack([x, y], axis=1), lp)
    check_model((model.weights_, model.means_, model.covariances_, model.precisions_cholesky_, model.valid_idx, model.n_locs,
                 model.converged), name, 0)
    X = np.stack([x, y], axis=1)
    assert model.predict(X).shape == (len(x),) and model.estimate_log_prob(X).shape == (len(x), len(model.valid_idx))
    assert np.isfinite(model.bic(X))
    assert np.array_equal(model.estimate_weighted_log_prob(X).argmax(axis=1), model.predict(X))


def test_fixed_fit_from_given_means():
    """means_init through the host form (its twelfth staged piece) for two clusters, and through G5M_2D.fit."""
    from test_g5m_host import check_means_init, means_init_inputs
    x, y, lp, offsets, means_init = means_init_inputs()
    models = backend.g5m_fit_fixed(x, y, lp, offsets, 2, min_locs=10, sigma_bounds=(0.8, 1.5), means_init=means_init)
    check_means_init(models)
    free = backend.g5m_fit_fixed(x, y, lp, offsets, 2, min_locs=10, sigma_bounds=(0.8, 1.5))
    assert not same(free.model, models.model)                # the given means are used
    s = slice(offsets[1], offsets[2])
    one = g5m.G5M_2D(2, 10, (0.8, 1.5), means_init=means_init[1]).fit(np.stack([x[s], y[s]], axis=1), lp[s])
    second = models.of(1)
    assert (one is None) == (second is None)
    if one is not None:
        assert same(one.weights_, second[0]) and same(one.means_, second[1]) and same(one.covariances_, second[2])


def test_lds_and_scratch_paths_give_the_same_bits():
    x, y, lp, offsets = fixed_inputs("fixed_below")
    K = int(G["fixed_below/K"])
    a = backend.g5m_fit_fixed(x, y, lp, offsets, K, min_locs=10, sigma_bounds=(0.8, 1.5))
    b = backend.g5m_fit_fixed(x, y, lp, offsets, K, min_locs=10, sigma_bounds=(0.8, 1.5), force_scratch=True)
    assert all(same(p, q) for p, q in zip(a[2:], b[2:])) and a.info[0, 0] == K
    cols = columns("two_apart")
    lp2 = frame_of("two_apart")[["lpx", "lpy"]].mean(axis=1).to_numpy()
    off2 = np.concatenate([[0], np.cumsum(np.bincount(cols["group"]))])
    a = backend.g5m_search(cols["x"], cols["y"], lp2, off2, min_locs=10, sigma_bounds=(0.8, 1.5))
    b = backend.g5m_search(cols["x"], cols["y"], lp2, off2, min_locs=10, sigma_bounds=(0.8, 1.5), force_scratch=True)
    assert all(same(p, q) for p, q in zip(a[2:], b[2:]))


def test_dev_forms_equal_the_host_forms_in_bits():
    import torch
    cols = columns("photons")
    locs = frame_of("photons")
    lp = locs[["lpx", "lpy"]].mean(axis=1).to_numpy().astype(np.float64)
    x, y = cols["x"].astype(np.float64), cols["y"].astype(np.float64)
    offsets = np.array([0, len(x)], np.int64)
    host = backend.g5m_search(x, y, lp, offsets, min_locs=10, sigma_bounds=(0.8, 1.5))
    caps = host.cap
    table, first, uniform = backend.g5m_table(np.diff(offsets), caps)
    total = int(caps.sum())
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()      # noqa: E731
    d = {k: dev(v) for k, v in dict(x=x, y=y, lp=lp, off=offsets, table=table, first=first, uniform=uniform).items()}
    model, imodel = torch.zeros((5, total), dtype=torch.float64, device="cuda"), torch.zeros((2, total), dtype=torch.int32, device="cuda")
    info, bic = torch.zeros((1, 4), dtype=torch.int32, device="cuda"), torch.zeros(1, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    with _lib.lock():
        _lib.call("pmi_g5m_fit_dev", d["x"].data_ptr(), d["y"].data_ptr(), d["lp"].data_ptr(), d["off"].data_ptr(), 1, len(x),
                  d["table"].data_ptr(), d["first"].data_ptr(), d["uniform"].data_ptr(), 10, 0.8, 1.5, 3, 0, model.data_ptr(),
                  imodel.data_ptr(), total, info.data_ptr(), bic.data_ptr(), None, None, None)
    assert same(model.cpu().numpy(), host.model) and same(imodel.cpu().numpy(), host.imodel)
    assert same(info.cpu().numpy(), host.info) and same(bic.cpu().numpy(), host.bic)
    # the fixed fit and the assignment
    K = int(host.info[0, 0])
    fixed = backend.g5m_fit_fixed(x, y, lp, offsets, K, min_locs=10, sigma_bounds=(0.8, 1.5))
    t2, f2, u2 = backend.g5m_table(np.diff(offsets), np.array([K]))
    m2, i2 = torch.zeros((5, K), dtype=torch.float64, device="cuda"), torch.zeros((2, K), dtype=torch.int32, device="cuda")
    n2, b2 = torch.zeros((1, 4), dtype=torch.int32, device="cuda"), torch.zeros(1, dtype=torch.float64, device="cuda")
    dt2, df2, du2 = dev(t2), dev(f2), dev(u2)
    torch.cuda.synchronize()
    with _lib.lock():
        _lib.call("pmi_g5m_fit_fixed_dev", d["x"].data_ptr(), d["y"].data_ptr(), d["lp"].data_ptr(), d["off"].data_ptr(), 1, len(x),
                  dt2.data_ptr(), df2.data_ptr(), du2.data_ptr(), None, K, 10, 0.8, 1.5, 0, m2.data_ptr(), i2.data_ptr(), K,
                  n2.data_ptr(), b2.data_ptr(), None)
    assert same(m2.cpu().numpy(), fixed.model) and same(i2.cpu().numpy(), fixed.imodel) and same(n2.cpu().numpy(), fixed.info)
    frame = cols["frame"].astype(np.float64)
    extra = cols["photons"].astype(np.float64)[None]
    want = backend.g5m_assign(x, y, lp, frame, offsets, host, extra, f32=True, frame_u32=True)
    dframe, dcols, dtab = dev(frame), dev(extra), dev(np.array([[0, 0]], np.int64))
    label, ll = torch.zeros(len(x), dtype=torch.int32, device="cuda"), torch.zeros(len(x), dtype=torch.float64, device="cuda")
    stats, ev = torch.zeros((total, 7), dtype=torch.float64, device="cuda"), torch.zeros(total, dtype=torch.int32, device="cuda")
    gll, cm = torch.zeros(1, dtype=torch.float64, device="cuda"), torch.zeros((1, total), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    with _lib.lock():
        _lib.call("pmi_g5m_assign_dev", d["x"].data_ptr(), d["y"].data_ptr(), d["lp"].data_ptr(), dframe.data_ptr(), d["off"].data_ptr(), 1,
                  len(x), dtab.data_ptr(), model.data_ptr(), imodel.data_ptr(), total, info.data_ptr(), dcols.data_ptr(), 1,
                  backend.G5M_QUAD_F32 | backend.G5M_FRAME_U32, label.data_ptr(), ll.data_ptr(), stats.data_ptr(), ev.data_ptr(),
                  gll.data_ptr(), cm.data_ptr(), None, None, 0, None)
    for got, exp in ((label, want.label), (ll, want.log_likelihood), (stats, want.stats), (ev, want.n_events), (gll, want.group_ll), (cm, want.col_means)):
        assert same(got.cpu().numpy(), exp)
