"""Float64 restatement of the MLE fit's second output: Fisher matrix, CRLB and log-likelihood of the
integrated-Gaussian model at a given theta (picasso/gaussmle.py:673-742, 887-954).

Plain numpy, used by tests only.  Everything is evaluated in float64 from the formulas:

    E(i; mu, s) = (erf((i - mu + 1/2) / (sqrt2 s)) - erf((i - mu - 1/2) / (sqrt2 s))) / 2
    A = dE/dmu  = (exp(-(i - mu - 1/2)^2 / 2s^2) - exp(-(i - mu + 1/2)^2 / 2s^2)) / (sqrt(2 pi) s)
    S = dE/ds   = ((i - mu - 1/2) exp(-(i - mu - 1/2)^2 / 2s^2) - (i - mu + 1/2) exp(-(i - mu + 1/2)^2 / 2s^2)) / (sqrt(2 pi) s^2)
    model = N Ex Ey + bg        (pixel (row y, column x) of the spot, theta = x, y, N, bg, sx, sy)
    du = (N Ax Ey, N Ex Ay, Ex Ey, 1, N Sx Ey, N Ex Sy)            "sigmaxy", six parameters
    du = (N Ax Ey, N Ex Ay, Ex Ey, 1, N (Sx Ey + Ex Sy))           "sigma", five parameters, sy = sx = theta[4]
    M_kl = sum over ALL pixels of du_k du_l / model                 (no model > 0 guard, as in the reference)
    ll = sum over pixels with model > 0 of  d ln(model) - model - d ln d + d   (d > 0)   or   -model   (otherwise)

theta is the float32 theta the code under test returned, cast to float64: the reference is evaluated where that
code stopped, so the Newton path does not enter a comparison.
"""
import math

import numpy as np

_erf = np.frompyfunc(math.erf, 1, 1)
SQRT2 = math.sqrt(2.0)
SQRT2PI = math.sqrt(2.0 * math.pi)
RAW_RATIO = 1e-13         # ... and lambda_min(M) >= this times lambda_max(M): pinv's 1e-15 cutoff is far away
WELL_LMIN = 1e-4          # a row is well-conditioned when lambda_min(C) >= this (and M is finite, diagonal positive)


def n_params(method):
    return {"sigmaxy": 6, "sigma": 5}[method]


def profiles(mu, s, box):
    """E, A = dE/dmu, S = dE/ds on pixels 0..box-1; mu, s (N,) float64 -> three (N, box) arrays."""
    i = np.arange(box, dtype=np.float64)[None, :]
    mu = np.asarray(mu, np.float64)[:, None]
    s = np.asarray(s, np.float64)[:, None]
    with np.errstate(all="ignore"):
        lo, hi = i - mu - 0.5, i - mu + 0.5
        E = 0.5 * (_erf(hi / (SQRT2 * s)).astype(np.float64) - _erf(lo / (SQRT2 * s)).astype(np.float64))
        el, eh = np.exp(-0.5 * (lo / s) ** 2), np.exp(-0.5 * (hi / s) ** 2)
        A = (el - eh) / (SQRT2PI * s)
        S = (lo * el - hi * eh) / (SQRT2PI * s * s)
    return E, A, S


def derivatives(theta, box, method):
    """-> du (N, NP, box, box), model (N, box, box), and for "sigma" the two separable parts of du_4
    (N Sx Ey, N Ex Sy), else None.  Axis order of a spot: [row y, column x]."""
    th = np.asarray(theta, np.float64)
    N = th[:, 2][:, None, None]
    sx = th[:, 4]
    sy = th[:, 5] if method == "sigmaxy" else th[:, 4]
    Ex, Ax, Sx = (a[:, None, :] for a in profiles(th[:, 0], sx, box))
    Ey, Ay, Sy = (a[:, :, None] for a in profiles(th[:, 1], sy, box))
    with np.errstate(all="ignore"):
        model = N * Ex * Ey + th[:, 3][:, None, None]
        du = [N * Ax * Ey, N * Ex * Ay, Ex * Ey, np.ones_like(model)]
        if method == "sigmaxy":
            du += [N * Sx * Ey, N * Ex * Sy]
            parts = None
        else:
            parts = (N * Sx * Ey, N * Ex * Sy)
            du += [parts[0] + parts[1]]
    return np.stack(du, axis=1), model, parts


def fisher64(theta, box, method):
    """Fisher matrices (N, NP, NP) at theta (N, 6)."""
    du, model, _ = derivatives(theta, box, method)
    with np.errstate(all="ignore"):
        return np.einsum("nkyx,nlyx->nkl", du / model[:, None], du)


def loglik64(spots, theta, method):
    """Log-likelihood (N,) of spots (N, box, box) at theta, with the reference's model > 0 and data > 0 branches."""
    d = np.asarray(spots, np.float64)
    _, model, _ = derivatives(theta, d.shape[1], method)
    with np.errstate(all="ignore"):
        pos = d > 0
        dsafe = np.where(pos, d, 1.0)
        msafe = np.where(model > 0, model, 1.0)
        term = np.where(pos, d * np.log(msafe) - model - d * np.log(dsafe) + d, -model)
        return np.where(model > 0, term, 0.0).sum(axis=(1, 2))


def loglik_unit(spots, ll):
    """v = 2^-24 sum_pixels d |ln d| + ulp32(ll): the rounding of the reference's float32 d log d term and of its
    float32 result."""
    d = np.asarray(spots, np.float64)
    with np.errstate(all="ignore"):
        t = np.where(d > 0, d * np.abs(np.log(np.where(d > 0, d, 1.0))), 0.0).sum(axis=(1, 2))
        ulp = np.spacing(np.abs(np.asarray(ll, np.float64)).astype(np.float32)).astype(np.float64)
    return 2.0 ** -24 * t + ulp


def conditioning(M):
    """lambda_min, lambda_max (N,) of C = D^-1/2 M D^-1/2, D = diag(M); NaN where M is not finite or its diagonal
    not positive."""
    M = np.asarray(M, np.float64)
    n, k = M.shape[0], M.shape[1]
    lmin, lmax = np.full(n, np.nan), np.full(n, np.nan)
    dg = np.einsum("nii->ni", M)
    with np.errstate(all="ignore"):
        ok = np.isfinite(M).all(axis=(1, 2)) & (dg > 0).all(axis=1) & np.isfinite(1.0 / np.sqrt(dg)).all(axis=1)
        r = 1.0 / np.sqrt(np.where(ok[:, None], dg, 1.0))
        C = M * r[:, :, None] * r[:, None, :]
        ok &= np.isfinite(C).all(axis=(1, 2))
    if ok.any():
        w = np.linalg.eigvalsh(C[ok])
        lmin[ok], lmax[ok] = w[:, 0], w[:, k - 1]
    return lmin, lmax


def well_conditioned(M):
    """M finite, diagonal positive, lambda_min(C) >= WELL_LMIN — and every eigenvalue of M itself at least RAW_RATIO of
    its largest, a hundred times pinv's cutoff, so that the reference's pinv(M) IS inv(M).  (The second condition is not
    implied by the first: a 3 x 3 box with sigma 0.03 px has M_00 ~ 1e-50 beside M_22 ~ 1 at lambda_min(C) = 0.07, and the
    reference's pinv then returns 0 for that direction, not 1e50.)"""
    M = np.asarray(M, np.float64)
    lmin, _ = conditioning(M)
    with np.errstate(invalid="ignore"):
        well = lmin >= WELL_LMIN
    if well.any():
        w = np.linalg.eigvalsh(M[well])
        well[np.flatnonzero(well)[w[:, 0] < RAW_RATIO * w[:, -1]]] = False
    return well


def pinv_diag(M):
    """diag(np.linalg.pinv(M, rcond=1e-15, hermitian=True)) of one matrix: the reference's semantics (a direction whose
    eigenvalue is at most 1e-15 of the largest is dropped: 0, not inf).  All NaN where M is not finite."""
    M = np.asarray(M, np.float64)
    if not np.isfinite(M).all():
        return np.full(M.shape[0], np.nan)
    return np.diag(np.linalg.pinv(M, rcond=1e-15, hermitian=True)).copy()


def jacobi_eigh(M):
    """Eigenvalues and eigenvectors of one symmetric matrix by cyclic Jacobi rotations, float64.  On the graded matrices a
    collapsed fit leaves (diagonal from 1e-80 to 1e6) Jacobi finds the small eigenvalues to their own relative accuracy,
    where a tridiagonalising solver (LAPACK behind np.linalg.pinv) only finds them to 1e-16 of the LARGEST — which is the
    size of pinv's cutoff, so that solver's pinv is not defined near it."""
    A = np.array(M, np.float64)
    n = A.shape[0]
    V = np.eye(n)
    for _ in range(60):
        off = sum(A[p, q] ** 2 for p in range(n) for q in range(p + 1, n))
        if off == 0.0:
            break
        for p in range(n):
            for q in range(p + 1, n):
                if A[p, q] == 0.0:
                    continue
                tau = (A[q, q] - A[p, p]) / (2.0 * A[p, q])
                t = (1.0 if tau >= 0 else -1.0) / (abs(tau) + math.sqrt(1.0 + tau * tau))
                c = 1.0 / math.sqrt(1.0 + t * t)
                R = np.eye(n)
                R[p, p] = R[q, q] = c
                R[p, q], R[q, p] = t * c, -t * c
                A = R.T @ A @ R
                V = V @ R
    return np.diag(A).copy(), V


def pinv_diag_jacobi(M):
    """pinv_diag with jacobi_eigh for the eigen-decomposition: the same semantics (eigenvalues of magnitude at most 1e-15 of
    the largest are dropped), defined on graded matrices too."""
    M = np.asarray(M, np.float64)
    if not np.isfinite(M).all():
        return np.full(M.shape[0], np.nan)
    with np.errstate(all="ignore"):
        w, V = jacobi_eigh(M)
        if not (np.isfinite(w).all() and np.isfinite(V).all()):
            return np.full(M.shape[0], np.nan)
        keep = np.abs(w) > 1e-15 * np.abs(w).max()
        return (V[:, keep] ** 2 / w[keep]).sum(axis=1)


def pinv_ambiguous(M):
    """True where either branch of a pinv is legitimate: an eigenvalue of M within a factor 10 of the 1e-15 lambda_max
    cutoff, or trace(M) trace(pinv M) within a factor 10 of 1e12 (where the device changes from LDL^T to Jacobi)."""
    M = np.asarray(M, np.float64)
    if not np.isfinite(M).all():
        return False
    with np.errstate(all="ignore"):
        w = np.abs(jacobi_eigh(M)[0])
        cut = 1e-15 * w.max()
        t = np.trace(M) * pinv_diag_jacobi(M).sum()
    return bool(np.any((w > 0.1 * cut) & (w < 10 * cut)) or (1e11 < t < 1e13))


def crlb64(M, pinv=None):
    """-> crlb (N, NP), well (N,) bool.  Well-conditioned rows: diag(inv(M)), inverted in the scaled form
    inv(M)_ii = inv(C)_ii / M_ii, which keeps float64's error at 2^-53 / lambda_min.  The rest: pinv_diag (np.linalg.pinv), or
    `pinv` when given (pinv_diag_jacobi, for matrices that a fit at a floor or far outside its box leaves)."""
    M = np.asarray(M, np.float64)
    well = well_conditioned(M)
    out = np.empty(M.shape[:2])
    if well.any():
        dg = np.einsum("nii->ni", M[well])
        r = 1.0 / np.sqrt(dg)
        C = M[well] * r[:, :, None] * r[:, None, :]
        out[well] = np.einsum("nii->ni", np.linalg.inv(C)) / dg
    for i in np.flatnonzero(~well):
        out[i] = (pinv or pinv_diag)(M[i])
    return out, well
