"""Mint tests/golden/g5m_cases.npz: what the reference's own G5M functions give on seeded synthetic tables.

The named functions and classes are compiled from where they lie in the reference's ``g5m.py`` and ``lib.py`` (the ``njit``
decorators dropped: numba is not installed, so the record follows NumPy execution of the reference's source, with NumPy's
legacy global generator) and run as they are.  Only inputs and results are stored.

Tolerance.  Every case runs three times through the same functions: as they are; with every ``exp`` / ``log`` result
moved by one ulp at random (fixed seed); and with every accumulation (``_sum_along_*``, ``_matmul``'s inner loop,
``np.sum``) in reversed order.  The largest relative deviation per output quantity is recorded; a test allows 8 x that
value and nothing else (a quantity that did not move, such as the float32 columns of the centers, must be equal in
bits).  Every integer and every choice must be the same in all three runs, or the script fails: such a case gets another
seed.

    python tests/golden/make_goldens_g5m.py            # writes g5m_cases.npz next to this file
"""
import ast
import json
import os
import re
import sys
import types
from abc import ABCMeta, abstractmethod

import numpy as np
import pandas as pd
from scipy.special import erf

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("PICASSO_REFERENCE", "/root/reference")
G5M_PY = os.path.join(REF, "picasso", "g5m.py")
LIB_PY = os.path.join(REF, "picasso", "lib.py")
VERSION_PY = os.path.join(REF, "picasso", "version.py")
LDS_RESP = 4096                 # G5M_LDS_RESP of the library (tests/test_g5m_host.py holds the two together)
NAMES = ("_max_along_axis1", "_sum_along_axis0", "_sum_along_axis1", "_mean_along_axis1", "_logsumexp_axis1", "_matmul",
         "_square_elements_1d", "_square_elements_2d", "_gauss_exponential_term_2D", "_euclidean_distances", "_kmeans_plusplus",
         "G5M", "_check_G5M_resolution_2D", "_initialize_G5M_2D", "_estimate_gaussian_parameters_2D",
         "_estimate_log_gaussian_prob_2D", "_e_step_2D", "_m_step_2D", "_find_optimal_G5M_2D", "_run_g5m_group_2D", "G5M_2D",
         "_estimate_gaussian_parameters_diag_cov", "_approximate_sem", "_convert_G5M_results", "_fit_G5M", "_g5m", "g5m")
CONSTANTS = ("MIN_LOCS", "MAX_ROUNDS_WITHOUT_BEST_BIC", "MIN_SIGMA_FACTOR", "MAX_SIGMA_FACTOR", "N_TASKS", "N_COMPONENTS_MAX", "fastmath",
             "SPOT_SIZE_DEPRECATION_WARNING")
SATELLITE_SEED = 100


def signature(fn):
    """[name, kind, repr(default)] per parameter: what a test compares without the reference tree."""
    import inspect
    return [[p.name, p.kind.name, repr(p.default)] for p in inspect.signature(fn).parameters.values()]


def _compile(path, names, ns, constants=()):
    tree = ast.parse(open(path).read())
    keep = [n for n in tree.body if (isinstance(n, (ast.FunctionDef, ast.ClassDef)) and n.name in names) or
            (isinstance(n, ast.Assign) and getattr(n.targets[0], "id", None) in constants)]
    found = [n.name for n in keep if not isinstance(n, ast.Assign)]
    assert sorted(found) == sorted(names), sorted(set(names) ^ set(found))
    for n in keep:
        if isinstance(n, ast.FunctionDef):
            n.decorator_list = []
    mod = ast.Module(body=[ast.ImportFrom("__future__", [ast.alias("annotations")], 0)] + keep, type_ignores=[])
    exec(compile(ast.fix_missing_locations(mod), path, "exec"), ns)
    return ns


class MockProgress:
    def update(self, *a): pass
    def set_value(self, *a): pass
    def close(self): pass


def _get_from_metadata(info, key, default=None, *, raise_error=False):
    for d in reversed([info] if isinstance(info, dict) else list(info)):
        if key in d:
            return d[key]
    return default


class Numpy:
    """``np`` as the reference sees it in the perturbed runs: everything is NumPy's, except what a mode replaces."""

    def __init__(self, mode):
        self.mode, self.rng = mode, np.random.default_rng(20261021)

    def __getattr__(self, name):
        return getattr(np, name)

    def _ulp(self, v):
        v = np.asarray(v, np.float64)
        step = self.rng.integers(-1, 2, v.shape)
        out = np.where(step > 0, np.nextafter(v, np.inf), np.where(step < 0, np.nextafter(v, -np.inf), v))
        return out if out.ndim else np.float64(out)

    def exp(self, v):
        return self._ulp(np.exp(v)) if self.mode == "ulp" else np.exp(v)

    def log(self, v):
        return self._ulp(np.log(v)) if self.mode == "ulp" else np.log(v)

    def sum(self, a, *args, **kw):
        if self.mode == "reversed" and not args and not kw:
            total = np.float64(0.0)
            for v in np.asarray(a).ravel()[::-1]:
                total = total + v
            return total
        return np.sum(a, *args, **kw)


def load_reference(mode="plain"):
    version = re.search(r'__version__\s*=\s*"([^"]+)"', open(VERSION_PY).read()).group(1)
    lib_ns = _compile(LIB_PY, ("find_local_minima",), {"np": np})
    ns = {"np": np if mode == "plain" else Numpy(mode), "pd": pd, "erf": erf, "ABCMeta": ABCMeta, "abstractmethod": abstractmethod,
          "lib": types.SimpleNamespace(find_local_minima=lib_ns["find_local_minima"], get_from_metadata=_get_from_metadata,
                                       MockProgress=MockProgress),
          "__version__": version, "version": version}
    _compile(G5M_PY, NAMES, ns, CONSTANTS)
    if mode == "reversed":
        def sum0(X, final_shape):
            out = np.zeros(final_shape, dtype=X.dtype)
            for i in range(X.shape[0] - 1, -1, -1):
                out += X[i]
            return out

        def sum1(X, final_shape):
            out = np.zeros(final_shape, dtype=X.dtype)
            for i in range(X.shape[1] - 1, -1, -1):
                out += X[:, i]
            return out

        def matmul(a, b):
            c = np.zeros((a.shape[0], b.shape[1]), dtype=a.dtype)
            for k in range(a.shape[1] - 1, -1, -1):
                c += a[:, k:k + 1] * b[k:k + 1, :]
            return c
        ns["_sum_along_axis0"], ns["_sum_along_axis1"], ns["_matmul"] = sum0, sum1, matmul
    # the models _find_optimal_G5M_2D returns, in the order g5m asks for them
    real, ns["found"] = ns["_find_optimal_G5M_2D"], []

    def watched(X, *a, **kw):
        m = real(X, *a, **kw)
        ns["found"].append((m, None if m is None else m.bic(X)))
        return m
    ns["_find_optimal_G5M_2D"] = watched
    return ns


# ---- the tables ----------------------------------------------------------------------------------------------------------
def blob(rng, n, cx, cy, sigma, frames=20000):
    return rng.normal(cx, sigma, n), rng.normal(cy, sigma, n), np.sort(rng.integers(0, frames, n))


def table(parts, rng, lp=0.05, lp_spread=0.0, extra=False):
    """parts: per cluster a list of (n, cx, cy, sigma); rows of one cluster lie together, frames ascending."""
    cols = {k: [] for k in ("frame", "x", "y", "lpx", "lpy", "group")}
    for g, blobs in enumerate(parts):
        x, y, f = (np.concatenate(v) for v in zip(*[blob(rng, *b) for b in blobs]))
        order = np.argsort(f, kind="stable")
        n = len(x)
        cols["frame"].append(f[order]), cols["x"].append(x[order]), cols["y"].append(y[order]), cols["group"].append(np.full(n, g))
        cols["lpx"].append(lp * (1 + lp_spread * rng.uniform(-1, 1, n))), cols["lpy"].append(lp * (1 + lp_spread * rng.uniform(-1, 1, n)))
    out = {"frame": np.concatenate(cols["frame"]).astype(np.uint32), "x": np.concatenate(cols["x"]).astype(np.float32),
           "y": np.concatenate(cols["y"]).astype(np.float32), "lpx": np.concatenate(cols["lpx"]).astype(np.float32),
           "lpy": np.concatenate(cols["lpy"]).astype(np.float32), "group": np.concatenate(cols["group"]).astype(np.int32)}
    if extra:
        out["photons"] = rng.uniform(500, 5000, len(out["x"])).astype(np.float32)
    return out


def make_cases():
    """name -> (columns, keyword arguments of g5m).  Every case is a table; what it covers is in the name."""
    S = 0.05
    r = lambda s: np.random.default_rng(s)  # noqa: E731
    cases = {
        "sizes_9_10_19_20": (table([[(9, 5, 5, S)], [(10, 8, 5, S)], [(19, 11, 5, S)], [(20, 14, 5, S)]], r(1)), {}),
        "two_apart": (table([[(40, 5, 5, S), (40, 5.3, 5, S)], [(30, 9, 9, S)]], r(2)), {}),
        "two_within_sigma": (table([[(40, 5, 5, S), (40, 5.04, 5, S)]], r(3)), {}),
        # a broad cloud (three times the largest sigma the bounds allow: several components tile it) with a 4-row satellite:
        # the seed is one for which the chosen model drops a component that is not its last (main() asserts it)
        "satellite": (table([[(45, 5, 5, 0.15), (4, 5.6, 5.3, 0.01)]], r(SATELLITE_SEED)), {}),
        "cov_low_local": (table([[(40, 5, 5, 0.01)], [(40, 8, 8, 0.2)]], r(5)), {}),
        "cov_bounds_abs": (table([[(40, 5, 5, 0.01)], [(40, 8, 8, 0.2)]], r(6)), {"loc_prec_handle": "abs", "sigma_bounds": (0.04, 0.08)}),
        "spread_lp": (table([[(40, 5, 5, S), (35, 5.3, 5.1, S)]], r(17), lp_spread=0.5), {}),
        "rows_300": (table([[(150, 5, 5, S), (150, 5.4, 5.2, S)]], r(8)), {"max_rounds_without_best_bic": 2}),
        "max_locs": (table([[(30, 5, 5, S)], [(60, 8, 8, S)], [(25, 11, 11, S)]], r(9)), {"max_locs_per_cluster": 50}),
        "photons": (table([[(40, 5, 5, S), (30, 5.3, 5, S)]], r(10), extra=True), {}),
        "filtered": (table([[(40, 5, 5, S)]], r(11)), {"postprocess": True}),
        "none_valid": (table([[(9, 5, 5, S)], [(7, 8, 8, S)]], r(12)), {}),
    }
    for name, (cols, kw) in cases.items():
        kw.setdefault("postprocess", False)
    cases["filtered"][0]["frame"] = (cases["filtered"][0]["frame"] // 1000).astype(np.uint32)      # std_frame below 0.1 n_frames
    # one fixed-K fit with n K just above the LDS bound and one just below (K = 8: 512 and 513 rows)
    fixed = {"fixed_below": (table([[(LDS_RESP // 8, 5, 5, 0.3)]], r(13)), 8), "fixed_above": (table([[(LDS_RESP // 8 + 1, 5, 5, 0.3)]], r(14)), 8)}
    return cases, fixed


INFO = [{"Frames": 20000, "Pixelsize": 130, "Width": 64, "Height": 64}]
DEFAULTS = dict(min_locs=10, loc_prec_handle="local", sigma_bounds=(0.8, 1.5), max_rounds_without_best_bic=3, max_locs_per_cluster=np.inf)


def model_record(m, b):
    if m is None:
        return {"K": np.int64(0)}
    return {"K": np.int64(len(m.weights_)), "valid_idx": np.asarray(m.valid_idx, np.int32), "converged": np.bool_(m.converged),
            "n_locs": np.asarray(m.n_locs, np.int64), "weights": m.weights_, "means": m.means_, "covariances": m.covariances_,
            "precisions_cholesky": m.precisions_cholesky_, "bic": np.float64(b)}


def run_table(ref, cols, kw):
    ref["found"].clear()
    centers, clustered, info = ref["g5m"](pd.DataFrame(cols), INFO, asynch=False, callback_parent=None, **kw)
    out = {"n_models": np.int64(len(ref["found"])), "info": json.dumps(info)}
    for i, (m, b) in enumerate(ref["found"]):
        out.update({f"model{i}/{k}": v for k, v in model_record(m, b).items()})
    out["found"] = np.bool_(centers is not None)
    if centers is not None:
        out["centers_columns"] = np.array(list(centers.columns))
        out["locs_columns"] = np.array(list(clustered.columns))
        out.update({f"centers/{c}": centers[c].to_numpy() for c in centers.columns})
        out.update({f"locs/{c}": clustered[c].to_numpy() for c in clustered.columns})
    return out


def run_fixed(ref, cols, K):
    X = np.stack([cols["x"], cols["y"]], axis=1)
    lp = pd.DataFrame(cols)[["lpx", "lpy"]].mean(axis=1).to_numpy()
    m = ref["G5M_2D"](K, 10, (0.8, 1.5)).fit(X, lp=lp)
    return {f"model0/{k}": v for k, v in model_record(m, np.inf if m is None else m.bic(np.float64(X))).items()}


def deviation(tol, a, b, name):
    """Integers and choices equal; floats: the largest relative deviation goes to tol[quantity]."""
    assert set(a) == set(b), name
    for key in a:
        va, vb = np.asarray(a[key]), np.asarray(b[key])
        assert va.shape == vb.shape and va.dtype == vb.dtype, (name, key)
        if va.dtype.kind != "f":
            assert np.array_equal(va, vb), (name, key)
            continue
        assert np.array_equal(np.isfinite(va), np.isfinite(vb)), (name, key)
        ok = np.isfinite(va)
        if ok.any():
            rel = np.abs(va[ok].astype(np.float64) - vb[ok]) / np.maximum(np.abs(va[ok]), np.finfo(np.float64).tiny)
            q = key.split("/")[-1]
            tol[q] = max(tol.get(q, 0.0), float(rel.max()))


def main():
    cases, fixed = make_cases()
    refs = {mode: load_reference(mode) for mode in ("plain", "ulp", "reversed")}
    out = {"case_names": np.array(list(cases)), "fixed_names": np.array(list(fixed)), "info": json.dumps(INFO),
           "lds_resp": np.int64(LDS_RESP), "version": refs["plain"]["version"],
           "signatures": json.dumps({"g5m": signature(refs["plain"]["g5m"]), "G5M_2D": signature(refs["plain"]["G5M_2D"].__init__),
                                     "fit": signature(refs["plain"]["G5M"].fit)})}
    tol = {}
    for name, (cols, kw) in cases.items():
        runs = {mode: run_table(ref, cols, dict(kw)) for mode, ref in refs.items()}
        for mode in ("ulp", "reversed"):
            deviation(tol, runs["plain"], runs[mode], name)
        out.update({f"{name}/{k}": v for k, v in runs["plain"].items()})
        out.update({f"{name}/in_{c}": v for c, v in cols.items()})
        out[name + "/in_columns"] = np.array(list(cols))
        out[name + "/kwargs"] = json.dumps({k: (None if v == np.inf else v) for k, v in kw.items()})
        print(name, "models", int(runs["plain"]["n_models"]), [int(runs["plain"][f"model{i}/K"]) for i in range(int(runs["plain"]["n_models"]))], flush=True)
    for name, (cols, K) in fixed.items():
        runs = {mode: run_fixed(ref, cols, K) for mode, ref in refs.items()}
        for mode in ("ulp", "reversed"):
            deviation(tol, runs["plain"], runs[mode], name)
        out.update({f"{name}/{k}": v for k, v in runs["plain"].items()})
        out.update({f"{name}/in_{c}": v for c, v in cols.items()})
        out[name + "/in_columns"], out[name + "/K"] = np.array(list(cols)), np.int64(K)
        print(name, int(runs["plain"]["model0/K"]), flush=True)
    dropped = out["satellite/model0/valid_idx"]
    assert len(dropped) < int(out["satellite/model0/K"]) and list(dropped) != list(range(len(dropped))), ("satellite", dropped)
    for q, v in sorted(tol.items()):
        out["tolerance/" + q] = np.float64(8 * v)
        print(f"tolerance/{q} = 8 x {v:.3e}")
    np.savez_compressed(os.path.join(HERE, "g5m_cases.npz"), **out)


if __name__ == "__main__":
    sys.exit(main())
