"""The SSIM of include/nlk_hip.h (nlk_dev_ssim) restated in float64 numpy: the 11-tap Gaussian window (sigma 1.5),
population moments, the valid region, every channel by itself, separably (rows, then columns)."""
import numpy as np

TAPS, R = 11, 5


def window():
    k = np.arange(TAPS, dtype=np.float64)
    g = np.exp(-((k - R) ** 2) / (2 * 1.5 ** 2))
    return g / g.sum()


def _hwc(a):
    a = np.asarray(a, np.float64)
    return a[:, :, None] if a.ndim == 2 else a


def moments(v):
    """the window mean of v (H, W, C) at every valid position: rows (along x) first, then columns"""
    g = window()
    h, w = v.shape[:2]
    rows = sum(g[j] * v[:, j:j + w - 2 * R] for j in range(TAPS))
    return sum(g[i] * rows[i:i + h - 2 * R] for i in range(TAPS))


def value(ma, mb, eaa, ebb, eab, rng=255.0):
    """S from the five window moments"""
    c1, c2 = (0.01 * rng) ** 2, (0.03 * rng) ** 2
    va, vb, cab = eaa - ma * ma, ebb - mb * mb, eab - ma * mb
    with np.errstate(invalid="ignore", over="ignore"):
        return ((2 * ma * mb + c1) * (2 * cab + c2)) / ((ma * ma + mb * mb + c1) * (va + vb + c2))


def ssim(a, b, rng=255.0):
    """(ssim, ssim_ch [ch], map [h - 10][w - 10][ch]) of the reference a and the image b, all float64"""
    a, b = _hwc(a), _hwc(b)
    assert a.shape == b.shape and a.shape[0] >= TAPS and a.shape[1] >= TAPS
    with np.errstate(invalid="ignore", over="ignore"):
        m = value(moments(a), moments(b), moments(a * a), moments(b * b), moments(a * b), rng)
    per_ch = m.mean(axis=(0, 1))
    return float(per_ch.mean()), per_ch, m
