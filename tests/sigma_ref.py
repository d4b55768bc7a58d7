"""The noise-level estimator of nlk_dev_estimate_sigma (include/nlk_hip.h) restated in float64 numpy:
a block-DCT percentile estimator in the spirit of Ponomarenko et al. Imports neither the product nor the oracle.

For every channel of an HWC image on the 0..255 scale:
  1. every 8 x 8 block whose top-left corner (x, y) has x % step == 0, y % step == 0, x <= w - 8, y <= h - 8, in
     raster order; a block holding a non-finite sample is skipped; N blocks are kept
  2. Y = C B C^T with C the orthonormal DCT-II
  3. L = the sum of Y[i][j]^2 over 1 <= i + j <= low_max
  4. K = min(N, max(kmin, ceil(frac N))) with frac rounded to float32 first (the C struct holds a float) and the
     product taken in double; T = the K-th smallest L; the selection is every block with L <= T, n >= K of them
  5. the mean of Y[i][j]^2 over the selection, for each (i, j) with i + j >= high_min
  6. sigma_c^2 = the median of those means (the mean of the two middle values for an even count)
The pooled value is sqrt(mean_c sigma_c^2). A channel without blocks gives NaN and the counts (0, 0)."""
import math

import numpy as np

DEFAULTS = dict(step=4, frac=0.05, kmin=64, low_max=5, high_min=8)


def dct8():
    k, j = np.mgrid[0:8, 0:8].astype(np.float64)
    c = 0.5 * np.cos(np.pi * (2 * j + 1) * k / 16)
    c[0] = math.sqrt(1 / 8)
    return c


def channel(plane, step=4, frac=0.05, kmin=64, low_max=5, high_min=8):
    """-> (sigma_c^2, N, n, relative gap between the K-th and the (K+1)-th smallest L; inf where there is none)"""
    plane = np.asarray(plane, np.float64)
    b = np.lib.stride_tricks.sliding_window_view(plane, (8, 8))[::step, ::step].reshape(-1, 8, 8)
    b = b[np.isfinite(b).all(axis=(1, 2))]
    n_blocks = len(b)
    if n_blocks == 0:
        return float("nan"), 0, 0, float("inf")
    c = dct8()
    y2 = (c @ b @ c.T) ** 2
    i, j = np.mgrid[0:8, 0:8]
    low = ((i + j >= 1) & (i + j <= low_max)).reshape(-1)
    high = (i + j >= high_min).reshape(-1)
    y2 = y2.reshape(n_blocks, 64)
    low_e = y2[:, low].sum(axis=1)
    k = min(n_blocks, max(int(kmin), math.ceil(float(np.float32(frac)) * n_blocks)))
    order = np.sort(low_e)
    t = order[k - 1]
    with np.errstate(divide="ignore", invalid="ignore"):
        gap = float((order[k] - t) / t) if k < n_blocks else float("inf")
    sel = low_e <= t
    n_sel = int(sel.sum())
    means = y2[sel][:, high].sum(axis=0) / n_sel
    return float(np.median(means)), n_blocks, n_sel, gap


def estimate(img, **params):
    """-> dict(sigma, sigma_ch [ch], counts [ch][2] = (N_c, n_c), gap = the smallest selection gap of the channels)"""
    img = np.asarray(img)
    if img.ndim == 2:
        img = img[:, :, None]
    p = dict(DEFAULTS, **params)
    res = [channel(img[:, :, c], **p) for c in range(img.shape[2])]
    var = np.array([r[0] for r in res])
    return dict(sigma=float(np.sqrt(var.mean())), sigma_ch=np.sqrt(var),
                counts=np.array([[r[1], r[2]] for r in res], np.int64), gap=min(r[3] for r in res))
