"""GPU tier: the accept-rate prior of the deferring scan (csrc/identify_fast.hip FastParams::prior_in / stats_out, csrc/runtime.hip
defer_prior_begin and fit_rows_kernel, ABI 117).

A wave of the fused MLE call's scan may emit its candidates undecided once its own exact rounds kept three in four of them.
What a scan's waves measured is handed to the scan of the call's second frame range and to the next call with the same key
(dtype, Y, X, roi, box, min_ng) on the same device and bank, whose waves start from it and verify it on their first eight
candidates.  Who decides a candidate changes — pmi_localize_last_scan_decisions counts it — the table never does: every table
here equals the one of pmi_localize_set_defer(0), where the scan decides everything, bit for bit.

Shapes: 1000 x 512 x 512 (2.6e8 pixels, the two-range schedule applies) and 200 x 256 x 256 (one range), the shapes and the
threshold of test_fused_call_with_the_exact_stage_of_identify_in_the_fit.  At either a wave holds about ten candidates, so a
cold wave never reaches the 32 it needs to defer and a seeded one defers what follows its probe of eight: the counts below
differ between cold and warm calls for that reason alone.
"""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

F_BIG, F_SMALL = 1000, 200


def _lib_():
    from picasso_amd import _lib
    return _lib, _lib.load()


def _run(movie, box=7, min_ng=5000.0, roi=None, baseline=100.0, cap=None, ranges=2):
    """One pmi_localize_mle_dev over the whole movie -> (table, rows, (decided A, undecided A, decided B, undecided B))."""
    import torch
    from picasso_amd import backend
    _lib, L = _lib_()
    F, Y, X = movie.shape
    cap = cap or 160 * F
    code = backend.dtype_code({torch.uint16: np.uint16, torch.uint8: np.uint8, torch.int16: np.int16}[movie.dtype])
    _lib.check(L.pmi_localize_set_ranges(ranges), "pmi_localize_set_ranges")
    table = torch.zeros((_lib.PMI_LOC_COLUMNS, cap), dtype=torch.int32, device="cuda")
    d_n = torch.zeros(1, dtype=torch.int64, device="cuda")
    r = (ctypes.c_int64 * 4)(*roi) if roi else None
    rc = L.pmi_localize_mle_dev(ctypes.c_void_p(movie.data_ptr()), code, F, Y, X, box, min_ng, r, 0, F - 1, baseline, 1.0, 1.0,
                                1e-3, 100, _lib.MLE_METHODS["sigmaxy"], ctypes.c_void_p(table.data_ptr()), cap,
                                ctypes.c_void_p(d_n.data_ptr()), None)
    _lib.check(rc, "pmi_localize_mle_dev")
    out = (ctypes.c_int64 * 4)()
    _lib.check(L.pmi_localize_last_scan_decisions(out, None), "pmi_localize_last_scan_decisions")
    torch.cuda.synchronize()
    return table, int(d_n.item()), tuple(int(v) for v in out)


def _reference(movie, **kw):
    """The table with the exact stage in the scan (set_defer(0)); leaves deferral on and the prior reset."""
    _lib, L = _lib_()
    _lib.check(L.pmi_localize_set_defer(0), "pmi_localize_set_defer")
    try:
        table, n, dec = _run(movie, ranges=1, **kw)
    finally:
        _lib.check(L.pmi_localize_set_defer(1), "pmi_localize_set_defer")
    assert n > 5000, n
    assert dec == (0, 0, 0, 0), dec                     # a call that does not defer reports nothing
    return table[:, :n].clone(), n


def _reset():
    _lib, L = _lib_()
    _lib.check(L.pmi_localize_reset_defer_prior(), "pmi_localize_reset_defer_prior")


def _same(got, n_got, ref):
    import torch
    table, n = ref
    return n_got == n and bool(torch.equal(got[:, :n_got], table))


def decided(dec): return dec[0] + dec[2]
def undecided(dec): return dec[1] + dec[3]


@pytest.fixture(scope="module")
def bright():
    import torch
    from picasso_amd import synth
    movie = synth.simulate_movie(F_BIG, 512, 512, emitters_per_frame=70, seed=31, device="cuda")
    torch.cuda.synchronize()
    return movie


@pytest.fixture(scope="module")
def bright_ref(bright):
    return _reference(bright)


@pytest.fixture(scope="module")
def dim():
    """Emitters around the threshold: a net gradient of 5000 takes 2300 ... 3500 photons at these widths, the floor filter lets
    a spot through from about 1500."""
    import torch
    from picasso_amd import synth
    movie = synth.simulate_movie(F_BIG, 512, 512, emitters_per_frame=70, seed=37, photons=(1500.0, 3200.0), device="cuda")
    torch.cuda.synchronize()
    return movie


@pytest.fixture(scope="module")
def small():
    import torch
    from picasso_amd import synth
    movie = synth.simulate_movie(F_SMALL, 256, 256, emitters_per_frame=200, seed=41, device="cuda")
    torch.cuda.synchronize()
    return movie


@pytest.fixture(autouse=True)
def _settings_back():
    yield
    _lib, L = _lib_()
    _lib.check(L.pmi_localize_set_ranges(2), "pmi_localize_set_ranges")
    _lib.check(L.pmi_localize_set_defer(1), "pmi_localize_set_defer")


def test_cold_then_warm(bright, bright_ref):
    """The first call after a reset proves the accept rate wave by wave in range A and hands it to range B; the second call
    starts from it in both ranges.  Same table each time, also with a capacity of exactly the rows."""
    _reset()
    t1, n1, d1 = _run(bright)
    t2, n2, d2 = _run(bright)
    print("cold", d1, "warm", d2, "rows", n1)
    assert _same(t1, n1, bright_ref) and _same(t2, n2, bright_ref)
    # (the candidates' number is not the same from call to call: the floor a chunk of rows filters with comes from the chunk
    # before it, and where a chunk ends depends on when the wave takes its rounds; every row is among them either way)
    assert decided(d1) + undecided(d1) >= n1 and decided(d2) + undecided(d2) >= n1
    assert d1[0] > 0 and d1[2] > 0 and d2[0] > 0 and d2[2] > 0                   # two ranges, and every seeded wave still probes
    assert decided(d2) < decided(d1), (d1, d2)
    assert d1[2] < d1[0], d1                                                     # within the cold call: B started from A's rate
    t3, n3, d3 = _run(bright, cap=bright_ref[1])
    assert _same(t3, n3, bright_ref), (n3, bright_ref[1])


def test_decisions_are_reproducible(bright):
    """A scan's waves read a prior that was settled before the launch and never what a sibling wrote: the same history gives
    the same counts."""
    runs = []
    for _ in range(2):
        _reset()
        runs.append([_run(bright)[2] for _ in range(3)])
    print(runs)
    assert runs[0] == runs[1], runs
    assert runs[0][0] != runs[0][1]                                              # (cold and warm are different things)


def test_wrong_prior_costs_no_row(bright, dim):
    """A prior from a movie that keeps nine candidates in ten, then a movie of the same shape and parameters that keeps under
    half: the seeded waves' probes send them back to deciding for themselves, the fit decides the rest, no row is lost."""
    ref = _reference(dim)
    _reset()
    t0, n0, d0 = _run(dim)
    cand = decided(d0) + undecided(d0)
    print("dim cold", d0, "rows", n0, "candidates", cand)
    assert _same(t0, n0, ref)
    assert 0 < 2 * n0 < cand, (n0, cand)                                         # the precondition: under half are kept
    assert 10 * n0 < 3 * cand, (n0, cand)                                        # (this movie: under 30 %, what the bound below rests on)
    _reset()
    _run(bright)
    wb = _run(bright)[2]
    t1, n1, d1 = _run(dim)
    print("bright warm", wb, "dim after bright", d1)
    assert _same(t1, n1, ref), (n1, ref[1])                                      # *d_out_n is the row count: no overflow
    assert undecided(d1) > undecided(d0)                                         # the prior was in play
    # ... and waves left deferral.  A seeded wave decides its probe of eight whatever happens next, so "decided > 0" shows
    # nothing.  Were the fall-back broken, every seeded wave would go on deferring what follows its probe, as in the warm bright
    # call: the dim movie has the same waves and no fewer candidates per wave, so it would leave at least about undecided(wb)
    # undecided.  Working, only the waves whose probe kept enough go on: with the bright prior (over 75 %: a seeded history of
    # at least 36 of 48) a wave needs at least 3 of its 8 kept at the most lenient, and at an accept rate under 30 % fewer than
    # 45 % of the probes reach that (binomial tail P(k >= 3 | 8, 0.3) = 0.448) — at this movie's 22 % and its prior's 82 %
    # (5 of 8) about 1 %.  Range B starts cold: A's rejects pull the prior under the rule.
    assert 2 * undecided(d1) < undecided(wb), (d1, wb)
    assert decided(d1) > decided(wb), (d1, wb)


def test_another_key_starts_cold(small, bright):
    """box and min_ng are part of the key: a call that differs in either reports the counts of a call after a reset.  uint8
    pixels and an ROI that starts off an 8-pixel boundary, warm, against their set_defer(0) tables."""
    import torch
    kw = dict(ranges=1)
    _reset()
    cold5 = _run(small, box=5, **kw)[2]
    _reset()
    cold_ng = _run(small, min_ng=4000.0, **kw)[2]
    _reset()
    cold7 = _run(small, **kw)[2]
    warm7 = _run(small, **kw)[2]
    print("box 7 cold", cold7, "warm", warm7, "box 5 cold", cold5, "min_ng 4000 cold", cold_ng)
    assert decided(warm7) < decided(cold7)                                       # the prior of this key is in play ...
    assert _run(small, box=5, **kw)[2] == cold5                                  # ... and not used for another box
    assert _run(small, min_ng=4000.0, **kw)[2] == cold_ng                        # nor for another threshold
    counts = bright.view(torch.int16).to(torch.int32) & 0xffff
    u8 = (counts // 8).clamp(max=255).to(torch.uint8)
    del counts
    # (the uint8 movie keeps under half of its candidates — the shot-noise maxima of its coarse counts pass the floor — so its
    # prior stays below the rule and the second call is the first again; the ROI call must come out warm)
    for movie, args, warm in ((u8, dict(min_ng=600.0, baseline=12.0), False), (bright, dict(roi=(10, 10, 499, 503)), True)):
        ref = _reference(movie, **args)
        c = _run(movie, **args)
        w = _run(movie, **args)
        print(args, "cold", c[2], "second call", w[2])
        assert _same(c[0], c[1], ref) and _same(w[0], w[1], ref), args
        assert decided(w[2]) < decided(c[2]) if warm else w[2] == c[2], (args, c[2], w[2])


def test_release_and_set_defer_drop_the_prior(small):
    _lib, L = _lib_()
    kw = dict(ranges=1)
    _reset()
    cold = _run(small, **kw)[2]
    warm = _run(small, **kw)[2]
    assert decided(warm) < decided(cold), (cold, warm)
    _lib.check(L.pmi_release_scratch(), "pmi_release_scratch")
    assert _run(small, **kw)[2] == cold
    assert _run(small, **kw)[2] == warm
    _lib.check(L.pmi_localize_set_defer(1), "pmi_localize_set_defer")
    assert _run(small, **kw)[2] == cold
