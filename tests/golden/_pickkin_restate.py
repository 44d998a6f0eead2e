"""What picasso/lib.py:1263-1327 (``estimate_kinetic_rate``, ``fit_cum_exp``) decides before it calls scipy, and the cost
its fit minimises, restated in NumPy for the tests of csrc/cumexp.hip.  No solver here: the minimiser under test is the
kernel's (csrc/cumexp_core.h), and scipy's results are recorded in tests/golden/pickkin_cases.npz.

Also the row bookkeeping of the pick wrappers that needs no device: which columns ``fit_cum_exp``'s in-place sort reorders
(``SORT_QUIRK`` in the golden says whether it does, as observed with the pandas the goldens were minted with).
"""
import numpy as np

KIND = {"i": 0, "u": 0, "b": 0}          # integer columns; float32 is 1, float64 is 2


def kind_of(dtype) -> int:
    dtype = np.dtype(dtype)
    if dtype.kind in KIND:
        return 0
    if dtype == np.float32:
        return 1
    if dtype == np.float64:
        return 2
    raise TypeError(f"no kinetic rate of a {dtype} column")


def model(x, a, t, c):
    with np.errstate(all="ignore"):
        return a * (1 - np.exp(-(x / t))) + c


def cost(x_sorted, p) -> float:
    """0.5 * sum r^2 of the model at p = (a, t, c) over (x_sorted, 1 .. n), in float64."""
    x = np.asarray(x_sorted, np.float64)
    y = np.arange(1, len(x) + 1, dtype=np.float64)
    r = model(x, *[np.float64(v) for v in p]) - y
    return float(0.5 * np.sum(r * r))


def prepare(data):
    """-> ("mean", value) for a segment the reference does not fit, ("refused", None) for one scipy raises ValueError on,
    or ("fit", x_sorted float64, p0, lower, upper)."""
    data = np.asarray(data)
    n = len(data)
    with np.errstate(all="ignore"):
        if n <= 2:
            return ("mean", nanmean(data))
        spread = data.max() - data.min()
        if spread == 0:
            return ("mean", nanmean(data))
        x = np.sort(data.astype(np.float64))
        if not np.isfinite(x).all() or x[0] < 0:
            return ("refused", None)
        p0 = (float(n), float(np.mean(x)), float(x[0]))
        return ("fit", x, p0, (0.0, float(x[0]), 0.0), (np.inf, float(x[-1]), np.inf))


def nanmean(data) -> float:
    """np.nanmean as a float64 value (NaN for no value), without its warning."""
    data = np.asarray(data)
    if len(data) == 0:
        return float("nan")
    import warnings
    with warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore")
        return float(np.nanmean(data))


def sort_fitted_columns(table, names=("len", "dark")):
    """The in-place sort of ``fit_cum_exp`` seen through ``Series.to_numpy()`` when that is a view: each named column of a
    pick's table whose rate is fitted (more than two rows, not all equal) ends up ascending, on its own."""
    for name in names:
        v = table[name].to_numpy()
        if len(v) > 2 and v.max() - v.min() != 0:
            table[name] = np.sort(v)
    return table


# ---- reading tests/golden/pickkin_cases.npz --------------------------------------------------------------------------
def picks_of(g, name):
    """The list of pick tables of wrapper case ``name``."""
    import pandas as pd
    columns = [str(c) for c in g[f"{name}_in_columns"]]
    offsets = g[f"{name}_in_offsets"]
    whole = pd.DataFrame({c: g[f"{name}_in_{c}"] for c in columns})
    return [whole.iloc[offsets[k]:offsets[k + 1]].reset_index(drop=True) for k in range(len(offsets) - 1)]


def table_of(g, prefix):
    """A stored table: (columns, dtypes, {column: values})."""
    columns = [str(c) for c in g[prefix + "_columns"]]
    return columns, [str(t) for t in g[prefix + "_dtypes"]], {c: g[f"{prefix}_{c}"] for c in columns}


def same_bits(a, b) -> bool:
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def assert_table(table, g, prefix, close=(), tol=0.0):
    """``table`` equals the stored one: columns, dtypes and every value (NaN positions included; the columns in
    ``close`` within the relative ``tol``)."""
    columns, dtypes, values = table_of(g, prefix)
    assert list(table.columns) == columns
    assert [str(t) for t in table.dtypes] == dtypes
    assert np.array_equal(np.asarray(table.index), g[prefix + "_index"])
    for c in columns:
        got, want = table[c].to_numpy(), values[c]
        if c in close:
            assert np.array_equal(np.isnan(got), np.isnan(want)), c
            ok = ~np.isnan(want)
            assert (np.abs(got[ok] - want[ok]) <= tol * np.abs(want[ok])).all(), (c, got, want)
        else:
            assert np.array_equal(got, want, equal_nan=got.dtype.kind == "f"), c


def host_dark_search(frame, labels, last_frame):
    """csrc/kinetics.hip's dark times with the table's largest frame as the limit, as a plain loop (for the host tests)."""
    frame, labels, last_frame = (np.asarray(a, np.int64) for a in (frame, labels, last_frame))
    top, out = int(frame.max()), np.full(len(frame), -1, np.int64)
    for i in range(len(frame)):
        d = frame[i] - last_frame[(labels == labels[i]) & (np.arange(len(frame)) != i)]
        d = d[(d > 0) & (d < top)]
        if len(d):
            out[i] = d.min()
    return out


cost_of = cost
COST_MARGIN = 1e-12                  # n <= 4096 samples: n * 2**-52 < 1e-12 covers the rounding of the two cost sums


def check_batch(G, name, fit, info):
    """The acceptance conditions of one fit batch, for the host driver and for the device alike: per fitted segment the
    cost recomputed here from the returned (a, t, c) is at most the reference's times 1 + 1e-12 and t is within ``tol`` of
    the reference's; a segment that is not fitted is the reference's value in every bit; a refused one has status 2."""
    TOL = float(G["tol"])
    values, offsets, mode = G[name + "_values"], G[name + "_offsets"], G[name + "_mode"]
    for s in range(len(mode)):
        x = np.sort(values[offsets[s]:offsets[s + 1]].astype(np.float64))
        if mode[s] == 1:
            t_ref, cost_ref = G[name + "_ref"][s, 1], G[name + "_ref_cost"][s]
            cost = cost_of(x, fit[:3, s])
            assert info[1, s] == 0, (name, s, "status", info[:, s])
            assert cost <= cost_ref * (1 + COST_MARGIN), (name, s, len(x), cost, cost_ref)
            assert abs(fit[1, s] - t_ref) <= TOL * t_ref, (name, s, len(x), fit[1, s], t_ref)
            assert abs(fit[3, s] - cost) <= 1e-9 * cost, (name, s, fit[3, s], cost)
            lower, upper = G[name + "_lower"][s], G[name + "_upper"][s]
            assert (fit[:3, s] >= lower).all() and (fit[:3, s] <= upper).all(), (name, s, fit[:3, s])
        elif mode[s] == 0:
            want = G[name + "_rate"][s]
            assert info[1, s] == 0 and info[0, s] == 0
            assert same_bits(np.float64(fit[1, s]), np.float64(want)) or (want != want and fit[1, s] != fit[1, s]), (name, s)
            assert np.isnan(fit[[0, 2, 3], s]).all()
        else:
            assert info[1, s] == 2 and np.isnan(fit[:, s]).all(), (name, s)
