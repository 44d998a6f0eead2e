"""G5M in 2-D (picasso/g5m.py, v0.10.3) restated in vectorised NumPy: the oracle of csrc/g5m_core.h and csrc/g5m.hip.

Same formulas, same decisions, NumPy's own sums, exp and log; the draws are ``RandomState(seed)``'s, call by call.  The
recorded results of the reference's own functions are in tests/golden/g5m_cases.npz (make_goldens_g5m.py)."""
import numpy as np
import pandas as pd
from scipy.special import erf

EPS10 = 10.0 * np.finfo(np.float64).eps
IGNORE = ("frame", "x", "y", "z", "lpx", "lpy", "lpz", "group", "group_input")


def sq_dist(c, X):
    d = -2.0 * (c[0] * X[:, 0] + c[1] * X[:, 1])
    d += c[0] * c[0] + c[1] * c[1]
    d += X[:, 0] * X[:, 0] + X[:, 1] * X[:, 1]
    return np.maximum(d, 0)


def kmeanspp(X, K, seed, log=None):
    rs = np.random.RandomState(seed)
    n, trials = len(X), 2 + int(np.log(K))
    first = rs.choice(n)
    idx = [int(first)]
    closest = sq_dist(X[first], X)
    pot = closest.sum()
    drawn = []
    for _ in range(1, K):
        u = np.array([rs.uniform() for _ in range(trials)])
        drawn.extend(u)
        cand = np.minimum(np.searchsorted(np.cumsum(closest), u * pot), n - 1)
        dist = np.minimum(closest, np.stack([sq_dist(X[c], X) for c in cand]))
        pots = dist.sum(axis=1)
        best = int(np.argmin(pots))
        pot, closest = pots[best], dist[best]
        idx.append(int(cand[best]))
    if log is not None:
        log.append((int(first), np.array(drawn)))
    return np.array(idx)


def estimate(X, resp):
    s0 = resp.sum(0)
    nk = s0 + EPS10
    means = (resp.T @ X) / nk[:, None]
    cov = np.stack([(resp * (X[:, [j]] - means[:, j]) ** 2).sum(0) / nk + 1e-6 for j in range(2)], axis=1)
    return nk, means, (cov[:, 0] + cov[:, 1]) / 2, s0


def log_prob(X, means, pc, f32=False):
    d0 = (X[:, [0]].astype(np.float64) - means[:, 0]) ** 2 * pc ** 2
    d1 = (X[:, [1]].astype(np.float64) - means[:, 1]) ** 2 * pc ** 2
    q = (d0.astype(np.float32).astype(np.float64) + d1).astype(np.float32).astype(np.float64) if f32 else d0 + d1
    return -0.5 * (2 * np.log(2 * np.pi) + q) + 2 * np.log(pc)


def logsumexp(a):
    m = a.max(axis=1)
    return np.log(np.exp(a - m[:, None]).sum(axis=1)) + m


def resolved(means, weights, pc):
    n = len(means)
    if n == 0:
        return False
    t = np.linspace(0, 1, 40)
    for i in range(n):
        for j in range(i + 1, n):
            m = means[[i, j]]
            line = m[0] + (m[1] - m[0]) * t[:, None]
            pdf = np.exp(log_prob(line, m, pc[[i, j]]) + np.log(weights[[i, j]])).sum(axis=1)
            if not ((pdf[1:-1] < pdf[:-2]) & (pdf[1:-1] < pdf[2:])).any():
                return False
    return True


def fit_fixed(X, lp, K, min_locs, bounds, handle="local", means_init=None):
    """G5M_2D(K).fit(X, lp, handle) -> dict(weights_, means_, covariances_, precisions_cholesky_, valid_idx, n_locs,
    converged) or None."""
    X, lp, n = np.float64(X), np.float64(lp), len(X)
    lo, hi = bounds[0] ** 2, bounds[1] ** 2
    best, max_lower = None, -np.inf
    for ii in range(max(K, 3)):
        resp = np.zeros((n, K))
        resp[kmeanspp(X, K, 42 + ii), np.arange(K)] = 1
        nk, means, cov, _ = estimate(X, resp)
        w, pc = nk / n, 1.0 / np.sqrt(cov)
        if means_init is not None:
            means = np.float64(means_init).copy()
        lower, converged = -np.inf, False
        for _ in range(100):
            prev = lower
            wlp = log_prob(X, means, pc) + np.log(w)
            lpn = logsumexp(wlp)
            resp = np.exp(wlp - lpn[:, None])
            nk, means, cov, s0 = estimate(X, resp)
            if handle == "local":
                m2 = ((resp * lp[:, None]).sum(0) / s0) ** 2
                cov = np.clip(cov, lo * m2, hi * m2)
            else:
                cov = np.clip(cov, lo, hi)
            w, pc = nk / nk.sum(), 1.0 / np.sqrt(cov)
            lower = np.mean(lpn)
            if abs(lower - prev) < 1e-3:
                converged = True
                break
        nloc = np.round(w * np.float64(n)).astype(np.int32)
        valid = np.where(nloc >= min_locs)[0].astype(np.int32)
        if resolved(means[valid], w[valid], pc[valid]) and (lower > max_lower or max_lower == -np.inf):
            max_lower = lower
            best = dict(weights_=w / w.sum(), means_=means, covariances_=cov, precisions_cholesky_=pc, valid_idx=valid,
                        n_locs=nloc[valid].astype(int), converged=converged)
    return best


def bic(model, X):
    v = model["valid_idx"]
    score = logsumexp(log_prob(np.float64(X), model["means_"][v], model["precisions_cholesky_"][v]) + np.log(model["weights_"][v]))
    return (4 * len(v) - 1) * np.log(len(X)) - 2 * score.mean() * len(X)


def search(X, lp, min_locs, bounds, handle="local", max_rounds=3):
    """_find_optimal_G5M_2D -> the model (with "bic" and "K") or None."""
    K, rounds, best_bic, best = 1, 0, np.inf, None
    k_max = min(100, len(X) // min_locs)
    while K <= k_max and rounds < max_rounds:
        m = fit_fixed(X, lp, K, min_locs, bounds, handle)
        v = None if m is None else m["valid_idx"]
        if m is None or not resolved(m["means_"][v], m["weights_"][v], m["precisions_cholesky_"][v]):
            rounds += 1
        else:
            b = bic(m, X)
            if b < best_bic:
                best_bic, rounds, best = b, 0, dict(m, bic=b, K=K)
            else:
                rounds += 1
        K += 1
    return best


def convert(model, locs_group, pixelsize):
    """_convert_G5M_results (2-D, no bootstrap) -> (centers, clustered locs)."""
    g = locs_group.copy()
    v = model["valid_idx"]
    means, cov, w = model["means_"][v], model["covariances_"][v], model["weights_"][v]
    X = g[["x", "y"]].to_numpy()
    f32 = X.dtype == np.float32
    lprob = log_prob(X, means, model["precisions_cholesky_"][v], f32) + np.log(w)
    score = logsumexp(lprob)
    wlp = log_prob(X, model["means_"], model["precisions_cholesky_"], f32) + np.log(model["weights_"])
    resp = np.exp((wlp - logsumexp(wlp)[:, None])[:, v])
    rsum = resp.sum(0)
    mol_ll = (resp * lprob).sum(0) / rsum
    expected = np.log(w / (2 * np.pi * cov)) - 1
    stdev = np.sqrt(2 * 0.5 / (len(X) * w))
    p_val = 0.5 * (1 + erf((mol_ll - expected) / (stdev * np.sqrt(2))))
    sem = np.sqrt(np.repeat(cov, 2).reshape(-1, 2) / (len(g) * w.reshape(len(w), -1)))
    sigma = np.sqrt(cov) * pixelsize
    lp = g[["lpx", "lpy"]].mean(axis=1).to_numpy()
    frames = g["frame"].to_numpy().reshape(-1, 1)
    frame = (resp * frames).sum(0) / rsum
    std_frame = np.sqrt((resp * (frames - frame) ** 2).sum(0) / ((len(X) - 1) * rsum / len(X)))
    split = np.where(np.diff(g["frame"].to_numpy()) > 3)[0] + 1
    ev = np.stack(([np.mean(_) for _ in np.split(g["x"].to_numpy(), split)], [np.mean(_) for _ in np.split(g["y"].to_numpy(), split)])).T
    ev_lab = (log_prob(ev, means, model["precisions_cholesky_"][v], ev.dtype == np.float32) + np.log(w)).argmax(axis=1)
    group0 = g["group"].iloc[0]
    centers = pd.DataFrame({
        "frame": frame.astype(np.float32), "std_frame": std_frame.astype(np.float32), "x": means[:, 0].astype(np.float32),
        "y": means[:, 1].astype(np.float32), "lpx": sem[:, 0].astype(np.float32), "lpy": sem[:, 1].astype(np.float32),
        "fitted_sigma": sigma.astype(np.float32), "rel_sigma": (sigma / ((resp * lp.reshape(-1, 1)).sum(0) / rsum) / pixelsize).astype(np.float32),
        "p_val": p_val.astype(np.float32), "mol_log_likelihood": mol_ll.astype(np.float32),
        "group_log_likelihood": (np.ones(len(v)) * np.mean(score)).astype(np.float32), "n_locs": model["n_locs"].astype(np.int32),
        "n_events": np.bincount(ev_lab, minlength=len(v)).astype(np.int32), "group_input": (group0 * np.ones(len(v), dtype=int)).astype(np.int32)})
    extra = [c for c in g.columns if c not in IGNORE]
    g["group_input"] = group0 * np.ones(len(g), dtype=int)
    g["group"] = lprob.argmax(axis=1)
    g["log_likelihood"] = score
    for col in extra + ["log_likelihood"]:
        centers[f"{col}_mean"] = (resp * g[col].to_numpy().reshape(-1, 1)).sum(0) / rsum
    return centers, g


def models_of(locs, min_locs, bounds, handle, max_rounds, max_locs=np.inf):
    """group id -> the chosen model (or None) of every cluster g5m fits, in np.unique order."""
    out = {}
    for group in np.unique(locs["group"]):
        g = locs[locs["group"] == group]
        if len(g) < min_locs or len(g) > max_locs:
            continue
        lp = g[["lpx", "lpy"]].mean(axis=1).to_numpy() if handle == "local" else np.ones(len(g))
        out[int(group)] = search(g[["x", "y"]].to_numpy().astype(np.float64), lp, min_locs, bounds, handle, max_rounds)
    return out
