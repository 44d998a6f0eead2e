"""The two functions of picasso.masking the Fourier ring correlation needs (picasso/masking.py:649-691):
``threshold_tukey`` and ``loess_smooth``.  Both are host code.  The Tukey mask is O(n^2) NumPy and trivial beside the
transforms; the device never needs the 2-D mask, only its one row (``tukey_profile``), and forms the products itself
(csrc/frc_core.h).  The smoothing is statsmodels' ``lowess``, imported when called: there is no LOESS of our own."""
from __future__ import annotations

import numpy as np


def tukey_profile(width: int) -> np.ndarray:
    """One row of ``threshold_tukey``'s mask before the product with its rotation: float64, ``width`` values."""
    nfac = 8
    x = np.arange(width)
    x_im = (x - (width / 2)) / width
    mask = 0.5 - 0.5 * np.cos(np.pi * nfac * x_im)
    mask[np.abs(x_im) < ((nfac - 2) / (nfac * 2))] = 1
    return mask


def threshold_tukey(image: np.ndarray) -> np.ndarray:
    """Tukey's mask of a square image, used to avoid FFT artifacts (picasso/masking.py:649-671)."""
    assert image.shape[0] == image.shape[1], "Image must be square"
    nfac = 8
    height, width = image.shape
    x = np.arange(width)
    x_im = (x - (width / 2)) / width
    x_im = np.tile(x_im, (height, 1))
    mask = 0.5 - 0.5 * np.cos(np.pi * nfac * x_im)
    mask[np.abs(x_im) < ((nfac - 2) / (nfac * 2))] = 1
    mask = mask * np.rot90(mask)
    return mask


def loess_smooth(arr: np.ndarray, span: int = 5) -> np.ndarray:
    """LOESS smoothing of a 1-D array (picasso/masking.py:674-691), by statsmodels."""
    try:
        from statsmodels.nonparametric.smoothers_lowess import lowess as loess
    except ImportError as exc:
        raise ImportError("loess_smooth needs statsmodels (statsmodels.nonparametric.smoothers_lowess.lowess), which "
                          "is not installed; picasso_amd has no LOESS of its own") from exc
    span += 1 - (span % 2)  # make sure span is odd
    x = np.arange(len(arr))
    smoothed_arr = loess(arr, x, span / len(arr), return_sorted=False)
    return smoothed_arr
