"""The noise-curve estimator of nlk_dev_estimate_noise_curve and the variance-stabilising transform of
nlk_dev_vst_forward / nlk_dev_vst_inverse (include/nlk_hip.h) restated in float64 numpy. Imports
neither the product nor the oracle.

Estimator, for every channel of an HWC image on the 0..255 scale (the model: var(z | y) = a y + b):
  1. the 8 x 8 blocks on the grid of `step`, in raster order; a block holding a non-finite sample is skipped;
     Y = C B C^T with C the orthonormal DCT-II; L = the sum of Y[i][j]^2 over 1 <= i + j <= low_max
  2. m = the sum of the block's 64 samples in raster order, divided by 64
  3. the bin q = floor((m - lo) / (hi - lo) * nbins) (nbins - 1 at most), lo and hi rounded to float32 first; a block
     with m outside [lo, hi) is skipped; N_q blocks are kept in bin q; a bin with N_q < nmin is dropped
  4. K_q = min(N_q, max(kmin, ceil(frac N_q))) with frac rounded to float32 first; the selection of the bin is its
     blocks with L <= the K_q-th smallest L of the bin, n_q of them
  5. v_q = the median over i + j >= high_min of the mean of Y[i][j]^2 over the selection, m_q = the mean of m over it
  6. v = a m + b by least squares with weights n_q over the bins kept. With fewer than 2 bins kept, or
     sum n (m - mbar)^2 = 0, or a < 0: a = 0, b = sum n v / sum n. Then, if b < 0: a = sum n m v / sum n m^2, b = 0.
     With no bin kept: a = b = NaN.

Transform, per channel with (a >= 0, b >= 0) and one scale s; u0 = 3 a^2 / 8 + b, u = a y + u0:
  forward   g = (2 s / a) (sqrt(max(u, 0)) - sqrt(u0)), evaluated as 2 s y / (sqrt(u) + sqrt(u0)) for u > 0
  inverse   r = max(g / s, -2 sqrt(u0) / a); mode 0: y = r sqrt(u0) + a r^2 / 4; mode 1 adds
            a (1/4 + (1/4) sqrt(3/2) / D - (11/8) / D^2 + (5/8) sqrt(3/2) / D^3),
            D = max(2 (sqrt(u0) + a r / 2) / a, 2 sqrt(u0) / a); nothing for a = 0
  scale     s = 255 / mean_c(span_c), span_c = 2 * 255 / (sqrt(255 a_c + u0_c) + sqrt(u0_c))"""
import math

import numpy as np

DEFAULTS = dict(step=4, frac=0.1, kmin=32, low_max=5, high_min=8, nbins=16, lo=0.0, hi=256.0, nmin=32)


def dct8():
    k, j = np.mgrid[0:8, 0:8].astype(np.float64)
    c = 0.5 * np.cos(np.pi * (2 * j + 1) * k / 16)
    c[0] = math.sqrt(1 / 8)
    return c


def fit(n, m, v):
    """the line of step 6 through the bins (n_q, m_q, v_q) with n_q > 0 -> (a, b)"""
    n, m, v = (np.asarray(x, np.float64) for x in (n, m, v))
    keep = n > 0
    n, m, v = n[keep], m[keep], v[keep]
    if len(n) == 0:
        return float("nan"), float("nan")
    mbar, vbar = (n * m).sum() / n.sum(), (n * v).sum() / n.sum()
    sxx = (n * (m - mbar) ** 2).sum()
    a = (n * (m - mbar) * (v - vbar)).sum() / sxx if len(n) >= 2 and sxx != 0 else -1.0
    b = vbar - a * mbar
    if not a >= 0:
        a, b = 0.0, vbar
    if b < 0:
        a, b = (n * m * v).sum() / (n * m * m).sum(), 0.0
    return float(a), float(b)


def channel(plane, step=4, frac=0.1, kmin=32, low_max=5, high_min=8, nbins=16, lo=0.0, hi=256.0, nmin=32):
    """-> dict(a, b, bins [nbins][4] = (N_q, n_q, m_q, v_q) with n_q = 0 and NaN for a bin dropped or empty,
    gap = the smallest relative gap between the K_q-th and the next L over the kept bins (inf where there is none),
    edge = the smallest distance of a block mean from a bin edge (inf without blocks))"""
    plane = np.asarray(plane, np.float64)
    lo, hi = float(np.float32(lo)), float(np.float32(hi))
    out = np.full((nbins, 4), np.nan)
    out[:, :2] = 0
    b = np.lib.stride_tricks.sliding_window_view(plane, (8, 8))[::step, ::step].reshape(-1, 8, 8)
    b = b[np.isfinite(b).all(axis=(1, 2))]
    mean = np.zeros(len(b))
    for k in range(64):   # raster order
        mean = mean + b[:, k // 8, k % 8]
    mean = mean / 64.0
    inside = (mean >= lo) & (mean < hi)
    b, mean = b[inside], mean[inside]
    if len(b) == 0:
        return dict(a=float("nan"), b=float("nan"), bins=out, gap=float("inf"), edge=float("inf"))
    pos = (mean - lo) / (hi - lo) * nbins
    q = np.minimum(np.floor(pos).astype(np.int64), nbins - 1)
    edge = float(np.min(np.minimum(pos - np.floor(pos), np.floor(pos) + 1 - pos)) * (hi - lo) / nbins)
    c = dct8()
    y2 = ((c @ b @ c.T) ** 2).reshape(len(b), 64)
    i, j = np.mgrid[0:8, 0:8]
    low = ((i + j >= 1) & (i + j <= low_max)).reshape(-1)
    high = (i + j >= high_min).reshape(-1)
    low_e = y2[:, low].sum(axis=1)
    gap = float("inf")
    for bin_ in range(nbins):
        at = q == bin_
        n_q = int(at.sum())
        out[bin_, 0] = n_q
        if n_q < max(nmin, 1):
            continue
        k = min(n_q, max(int(kmin), math.ceil(float(np.float32(frac)) * n_q)))
        order = np.sort(low_e[at])
        t = order[k - 1]
        if k < n_q:
            with np.errstate(divide="ignore", invalid="ignore"):
                gap = min(gap, float((order[k] - t) / t))
        sel = at & (low_e <= t)
        n_sel = int(sel.sum())
        out[bin_, 1] = n_sel
        out[bin_, 2] = mean[sel].sum() / n_sel
        out[bin_, 3] = np.median(y2[sel][:, high].sum(axis=0) / n_sel)
    a, b_ = fit(out[:, 1], out[:, 2], out[:, 3])
    return dict(a=a, b=b_, bins=out, gap=gap, edge=edge)


def estimate(img, **params):
    """-> dict(ab [ch][2], bins [ch][nbins][4], gap, edge: the smallest over the channels)"""
    img = np.asarray(img)
    if img.ndim == 2:
        img = img[:, :, None]
    p = dict(DEFAULTS, **params)
    res = [channel(img[:, :, c], **p) for c in range(img.shape[2])]
    return dict(ab=np.array([[r["a"], r["b"]] for r in res]), bins=np.array([r["bins"] for r in res]),
                gap=min(r["gap"] for r in res), edge=min(r["edge"] for r in res))


# ------------------------------------------------------------ the transform

def _ab(ab, ch):
    ab = np.asarray(ab, np.float64)
    return np.tile(ab, (ch, 1)) if ab.ndim == 1 else ab


def vst_scale(ab, ch=None):
    ab = _ab(ab, ch if ch is not None else len(np.atleast_2d(ab)))
    a, b = ab[:, 0], ab[:, 1]
    u0 = 0.375 * a * a + b
    span = 2 * 255.0 / (np.sqrt(255.0 * a + u0) + np.sqrt(u0))
    return float(255.0 / span.mean())


def vst_forward(img, ab, s):
    """img [h][w][ch] (or [h][w]) -> the transformed image, float64; NaN passes through"""
    x = np.asarray(img, np.float64)
    x3 = x[:, :, None] if x.ndim == 2 else x
    ab = _ab(ab, x3.shape[2])
    a, b = ab[None, None, :, 0], ab[None, None, :, 1]
    u0 = 0.375 * a * a + b
    u = a * x3 + u0
    with np.errstate(invalid="ignore", divide="ignore"):
        g = np.where(u <= 0, -2.0 * s * np.sqrt(u0) / np.where(a > 0, a, 1.0),
                     2.0 * s * x3 / (np.sqrt(np.maximum(u, 0)) + np.sqrt(u0)))
    g = np.where(np.isnan(x3), np.nan, g)
    return g.reshape(x.shape)


def vst_inverse(img, ab, s, mode=1):
    g = np.asarray(img, np.float64)
    g3 = g[:, :, None] if g.ndim == 2 else g
    ab = _ab(ab, g3.shape[2])
    a, b = ab[None, None, :, 0], ab[None, None, :, 1]
    ru0 = np.sqrt(0.375 * a * a + b)
    with np.errstate(invalid="ignore", divide="ignore"):
        floor = np.where(a > 0, -2.0 * ru0 / np.where(a > 0, a, 1.0), -np.inf)
        r = np.maximum(g3 / s, floor)      # (np.maximum keeps a NaN)
        y = r * ru0 + a * r * r / 4
        if mode == 1:
            sa = np.where(a > 0, a, 1.0)
            d = np.maximum(2 * (ru0 + a * r / 2) / sa, 2 * ru0 / sa)
            c32 = math.sqrt(1.5)
            y = y + np.where(a > 0, a * (0.25 + 0.25 * c32 / d - 1.375 / d ** 2 + 0.625 * c32 / d ** 3), 0.0)
    return y.reshape(g.shape)
