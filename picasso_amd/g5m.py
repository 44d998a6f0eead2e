"""picasso.g5m on the GPU, 2-D: Gaussian mixture modelling for molecular mapping (picasso/g5m.py, v0.10.3).

``g5m`` keeps the reference's signature, constants, assertions, error texts and return values; ``G5M_2D`` its fitting and
scoring members.  Every cluster's search over the number of components (``_find_optimal_G5M_2D``) runs in one device
call (csrc/g5m.hip: one workgroup per cluster and initialisation, round r fits K = r for every cluster still searching),
and so does ``_convert_G5M_results``.  The random draws of kmeans++ are NumPy's legacy generator's, drawn on the host
(``backend.g5m_draws``); everything that depends on the data runs on the device.  There is no CPU fallback.

Not built: the 3-D path (``_m_step_3D`` needs the astigmatism calibration), ``bootstrap_check=True``, ``G5M_2D.sample``.
``asynch`` is accepted and ignored: the device call is the parallel form.
"""
from __future__ import annotations

import sys

import numpy as np
import pandas as pd

from . import __version__, _lib, backend, lib

MIN_LOCS = 10
MAX_ROUNDS_WITHOUT_BEST_BIC = 3
MIN_SIGMA_FACTOR = 0.8
MAX_SIGMA_FACTOR = 1.5
N_TASKS = 500
N_COMPONENTS_MAX = 100
G5M_NAMES = ("g5m", "G5M_2D")
IGNORE_COLUMNS = ("frame", "x", "y", "z", "lpx", "lpy", "lpz", "group", "group_input")


def _not_built(what: str):
    raise NotImplementedError(f"picasso_amd.g5m: {what} is not built on the device, and there is no CPU fallback")


class G5M_2D:
    """G5M for 2-D data on the device; see ``picasso.g5m.G5M`` for the parameters."""

    def __init__(self, n_components, min_locs, sigma_bounds, *, means_init=None) -> None:
        assert sigma_bounds[0] >= 0.0 and sigma_bounds[1] >= 0.0
        assert sigma_bounds[1] >= sigma_bounds[0]
        self.n_components = int(n_components)
        self.min_locs = int(min_locs)
        self.sigma_bounds = sigma_bounds
        self.n_init = max(int(n_components), 3)
        self.random_state = 42
        self.converged = False
        self.means_init = means_init
        self.loc_prec_handle = "local"
        self.calibration = None
        self.spot_size = None
        self.z_range = None
        self.mag_factor = None
        self.n_dimensions = 2
        self.valid_idx = np.arange(n_components).astype(int)
        self.n_locs = np.zeros(n_components, dtype=int)

    # -- parameters ----------------------------------------------------------------------------------------------------
    def set_parameters(self, weights, means, covs, precisions_cholesky, converged, valid_idx=None) -> None:
        self.weights_ = weights / weights.sum()
        self.means_ = means
        self.covariances_ = covs
        self.precisions_cholesky_ = precisions_cholesky
        self.converged = converged
        if self.valid_idx is not None:
            self.valid_idx = valid_idx
        else:
            self.valid_idx = np.arange(len(weights))

    def _take(self, fitted) -> "G5M_2D":
        """The parameters as the device left them (weights_ already normalised)."""
        w, m, c, pc, valid, n_locs, converged = fitted
        self.weights_, self.means_, self.covariances_, self.precisions_cholesky_ = w, m, c, pc
        self.converged, self.valid_idx, self.n_locs = converged, valid.astype(np.int32), n_locs.astype(int)
        return self

    covariances = property(lambda self: self.covariances_[self.valid_idx], doc="Valid covariance.")
    means = property(lambda self: self.means_[self.valid_idx], doc="Valid means.")
    precisions_cholesky = property(lambda self: self.precisions_cholesky_[self.valid_idx], doc="Valid precision.")
    weights = property(lambda self: self.weights_[self.valid_idx], doc="Valid weights.")

    def n_parameters(self) -> int:
        n_valid = len(self.valid_idx)
        return int(n_valid + 2 * n_valid + n_valid - 1)

    # -- fitting ---------------------------------------------------------------------------------------------------------
    def fit(self, X, lp, loc_prec_handle="local"):
        """Fit G5M to data X on the device (pmi_g5m_fit_fixed).  Return None if fitting failed."""
        assert X.shape[1] == self.n_dimensions, (
            "The number of dimensions in X must match the number of "
            f"dimensions in the G5M class ({self.n_dimensions})."
        )
        X = np.ascontiguousarray(np.float64(X))
        lp = np.ascontiguousarray(np.float64(lp))
        self.n_samples = X.shape[0]
        self.loc_prec_handle = loc_prec_handle
        means_init = None if self.means_init is None else np.asarray(self.means_init, np.float64)[None]
        models = backend.g5m_fit_fixed(X[:, 0], X[:, 1], lp, [0, len(X)], self.n_components, min_locs=self.min_locs,
                                       sigma_bounds=self.sigma_bounds, lp_abs=loc_prec_handle != "local", means_init=means_init)
        fitted = models.of(0)
        if fitted is None:
            return None
        return self._take(fitted)

    # -- scoring: one device call (pmi_g5m_assign) over the rows of X ------------------------------------------------------
    def _models(self) -> backend.G5MModels:
        K, nv = len(self.weights_), len(self.valid_idx)
        model = np.stack([self.weights_, self.means_[:, 0], self.means_[:, 1], self.covariances_, self.precisions_cholesky_]).astype(np.float64)
        imodel = np.zeros((2, K), np.int32)
        imodel[1] = -1
        imodel[1, :nv] = self.valid_idx
        imodel[0, :nv] = self.n_locs
        return backend.G5MModels(np.zeros(1, np.int64), np.full(1, K, np.int64), model, imodel,
                                 np.array([[K, nv, int(self.converged), K]], np.int32), np.full(1, np.inf))

    def _score(self, X) -> backend.G5MAssigned:
        X = np.asarray(X)
        zero = np.zeros(len(X))
        return backend.g5m_assign(X[:, 0], X[:, 1], zero, zero, [0, len(X)], self._models(), f32=X.dtype == np.float32, probs=True)

    def estimate_log_prob(self, X):
        return self._score(X).log_prob[0]

    def estimate_weighted_log_prob(self, X):
        return self._score(X).weighted_log_prob[0]

    def predict(self, X):
        return self._score(X).label.astype(np.int64)

    def score_samples(self, X):
        return self._score(X).log_likelihood

    def bic(self, X) -> float:
        X = np.asarray(X)
        return self.n_parameters() * np.log(X.shape[0]) - 2 * self.score_samples(X).mean() * X.shape[0]

    def sample(self, n_samples: int = 1):
        _not_built("G5M_2D.sample")


def cluster_rows(locs: pd.DataFrame, min_locs: int, max_locs_per_cluster):
    """The clusters ``_run_g5m_group_2D`` fits, in ``np.unique(locs["group"])`` order: (group ids, rows in cluster order
    keeping the table's row order, offsets).  Clusters of fewer than ``min_locs`` or more than ``max_locs_per_cluster``
    rows are skipped."""
    group = locs["group"].to_numpy()
    order = np.argsort(group, kind="stable")
    ids, start, count = np.unique(group[order], return_index=True, return_counts=True)
    keep = (count >= min_locs) & (count <= max_locs_per_cluster)
    rows = [order[s:s + n] for s, n in zip(start[keep], count[keep])]
    offsets = np.concatenate([[0], np.cumsum(count[keep])]).astype(np.int64)
    return ids[keep], (np.concatenate(rows) if rows else np.zeros(0, np.int64)), offsets


def fit_clusters(locs, rows, offsets, *, min_locs, loc_prec_handle, sigma_bounds, max_rounds_without_best_bic, progress=None):
    """(models, assigned) of the clusters ``rows`` / ``offsets`` name: the two device calls of ``g5m``."""
    part = locs.iloc[rows]
    if loc_prec_handle == "local":
        lp = part[["lpx", "lpy"]].mean(axis=1).to_numpy()
    else:
        lp = np.ones(len(part))  # dummy
    xy = part[["x", "y"]].to_numpy()
    models = backend.g5m_search(xy[:, 0], xy[:, 1], lp, offsets, min_locs=min_locs, sigma_bounds=sigma_bounds,
                                lp_abs=loc_prec_handle != "local", max_rounds=max_rounds_without_best_bic, progress=progress)
    lp_mean = part[["lpx", "lpy"]].mean(axis=1).to_numpy()
    extra = [c for c in part.columns if c not in IGNORE_COLUMNS]
    cols = np.stack([part[c].to_numpy().astype(np.float64) for c in extra]) if extra else None
    frame = part["frame"].to_numpy()
    assigned = backend.g5m_assign(xy[:, 0], xy[:, 1], lp_mean, frame, offsets, models, cols, f32=xy.dtype == np.float32,
                                  frame_u32=frame.dtype == np.uint32)
    return models, assigned


def build_tables(locs, rows, offsets, group_ids, models, assigned, pixelsize):
    """``_convert_G5M_results`` of every cluster with a model and the concatenation and renumbering of ``g5m``: the
    centers and the clustered localizations, or (None, None)."""
    part = locs.iloc[rows]
    extra = [c for c in part.columns if c not in IGNORE_COLUMNS]
    centers, clustered, max_label = [], [], 0
    for c in range(len(group_ids)):
        K, nv = int(models.info[c, 0]), int(models.info[c, 1])
        if K == 0 or nv == 0:
            continue
        s0 = int(models.start[c])
        valid = models.imodel[1, s0:s0 + nv]
        weights, covariances = models.model[0, s0 + valid], models.model[3, s0 + valid]
        n = int(offsets[c + 1] - offsets[c])
        stats = assigned.stats[s0:s0 + nv]
        sem = np.sqrt(np.repeat(covariances, 2).reshape(-1, 2) / (n * weights.reshape(len(weights), -1)))
        sigma = np.sqrt(covariances) * pixelsize
        rel_sigma = sigma / stats[:, 4] / pixelsize
        group_input = part["group"].iloc[int(offsets[c])] * np.ones(nv, dtype=int)
        frame_center = pd.DataFrame({
            "frame": stats[:, 0].astype(np.float32),
            "std_frame": stats[:, 1].astype(np.float32),
            "x": models.model[1, s0 + valid].astype(np.float32),
            "y": models.model[2, s0 + valid].astype(np.float32),
            "lpx": sem[:, 0].astype(np.float32),
            "lpy": sem[:, 1].astype(np.float32),
            "fitted_sigma": sigma.astype(np.float32),
            "rel_sigma": rel_sigma.astype(np.float32),
            "p_val": stats[:, 3].astype(np.float32),
            "mol_log_likelihood": stats[:, 2].astype(np.float32),
            "group_log_likelihood": (np.ones(nv) * assigned.group_ll[c]).astype(np.float32),
            "n_locs": models.imodel[0, s0:s0 + nv].astype(np.int32),
            "n_events": assigned.n_events[s0:s0 + nv].astype(np.int32),
            "group_input": group_input.astype(np.int32),
        })
        for i, col in enumerate(extra):
            frame_center[f"{col}_mean"] = assigned.col_means[i, s0:s0 + nv]
        frame_center["log_likelihood_mean"] = stats[:, 6]      # the reference adds the column before it takes the means
        rows_c = slice(int(offsets[c]), int(offsets[c + 1]))
        locs_group = part.iloc[rows_c].copy()
        locs_group["group_input"] = locs_group["group"].iloc[0] * np.ones(len(locs_group), dtype=int)
        locs_group["group"] = assigned.label[rows_c].astype(np.int64)
        locs_group["log_likelihood"] = assigned.log_likelihood[rows_c]
        locs_group["group"] += max_label
        max_label = locs_group["group"].max() + 1
        centers.append(frame_center), clustered.append(locs_group)
    if not centers:
        return None, None
    return pd.concat(centers, ignore_index=True), pd.concat(clustered, ignore_index=True)


def g5m(locs, info, *, min_locs=MIN_LOCS, loc_prec_handle="local", sigma_bounds=(MIN_SIGMA_FACTOR, MAX_SIGMA_FACTOR),
        max_rounds_without_best_bic=MAX_ROUNDS_WITHOUT_BEST_BIC, bootstrap_check=False, calibration=None, postprocess=True,
        max_locs_per_cluster=np.inf, asynch=True, callback_parent="console"):
    """Run G5M on the device.  Returns the centers of the G5M components, the localizations with their component labels,
    and the updated info; ``(None, None, info)`` when no molecule is found.  See ``picasso.g5m.g5m`` for the parameters."""
    assert loc_prec_handle in [
        "local",
        "abs",
    ], "loc_prec_handle must be 'local' or 'abs'."
    assert (
        len(sigma_bounds) == 2
    ), "sigma_bounds must be a tuple of two values."
    assert (
        sigma_bounds[0] <= sigma_bounds[1]
    ), "sigma_bounds[0] must not be larger than sigma_bounds[1]."
    assert (
        "group" in locs.columns
    ), "Localizations must be grouped. Use DBSCAN or similar."

    pixelsize = lib.get_from_metadata(info, "Pixelsize")
    if pixelsize is None:
        raise ValueError("Camera pixel size must be provided in info.")
    if "z" in locs.columns and calibration is None:
        raise ValueError(
            "Calibration dictionary must be provided for 3D data. "
            "The dictionary must specify 'X Coefficients' and 'Y "
            "Coefficients' and 'Magnification factor'. See "
            "https://picassosr.readthedocs.io/en/latest/localize.html#d-calibration"  # noqa: E501
        )
    if "z" in locs.columns:
        _not_built("the 3-D path (_m_step_3D and the astigmatism calibration)")
    if bootstrap_check:
        _not_built("bootstrap_check=True (_bootstrap_sem)")
    if callback_parent not in ("console", None):
        raise ValueError("callback_parent must be 'console' or None")

    def report(rnd, n_clusters, _ms):
        if callback_parent == "console":
            print(f"Running G5M... round {rnd}: {n_clusters} clusters", file=sys.stderr)

    group_ids, rows, offsets = cluster_rows(locs, min_locs, max_locs_per_cluster)
    centers = clustered_locs = None
    if len(group_ids):
        models, assigned = _fit(locs, rows, offsets, min_locs=min_locs, loc_prec_handle=loc_prec_handle, sigma_bounds=sigma_bounds,
                                max_rounds_without_best_bic=max_rounds_without_best_bic, progress=report)
        centers, clustered_locs = build_tables(locs, rows, offsets, group_ids, models, assigned, pixelsize)
    if centers is None:  # no molecules found, return None
        return None, None, info

    new_info = {
        "Generated by": f"Picasso v{__version__} G5M",
        "Model determination": "BIC",
        "Number of molecules": len(centers),
        "Min. no. locs per molecule": min_locs,
        "Max. rounds w/o BIC improvement": max_rounds_without_best_bic,
        "Bootstrap SEM": bootstrap_check,
        "Initialization method": "KMeans++",
        "Filtered": False,
    }
    if loc_prec_handle == "local":
        new_info["Sigma bounds (factors)"] = list(sigma_bounds)
        new_info["Sigma bounds method"] = "Local"
    else:
        new_info["Sigma bounds (nm)"] = [
            sigma_bounds[0] * pixelsize,
            sigma_bounds[1] * pixelsize,
        ]
        new_info["Sigma bounds method"] = "Abs"
    info = info + [new_info]
    if postprocess:
        n_frames = info[0]["Frames"]
        min_std_frame = 0.1 * n_frames
        min_pval = 0.015
        min_n_events = 3
        idx = (
            (centers["std_frame"] > min_std_frame)
            & (centers["p_val"] > min_pval)
            & (centers["n_events"] > min_n_events)
        )
        centers = centers[idx]
        clustered_locs = clustered_locs[
            np.isin(clustered_locs["group"], np.arange(len(idx))[idx])
        ]
        info[-1]["Filtered"] = True
        info[-1]["Filter; min. std frame"] = min_std_frame
        info[-1]["Filter; min. p value"] = min_pval
        info[-1]["Filter; min. n_events"] = min_n_events
    return centers, clustered_locs, info


# what ``g5m`` calls for the two device calls: the host-side tests put the oracle's models here
_fit = fit_clusters
