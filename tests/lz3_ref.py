"""float64 numpy restatement of the Lanczos-3 pyramid of the lz3 multiscale pipeline, written
from the formulas, for the tests only: nothing under the package imports it. Images are (h, w, ch) arrays;
every operation is separable, horizontal first, then vertical."""
import numpy as np


def window(x):
    """sin(pi x) sin(pi x / 3) / (pi^2 x^2 / 3) for |x| < 3, 1 at 0, else 0."""
    x = np.asarray(x, np.float64)
    safe = np.where(x == 0, 1.0, x)
    v = np.sin(np.pi * safe) * np.sin(np.pi * safe / 3) / (np.pi ** 2 * safe ** 2 / 3)
    return np.where(x == 0, 1.0, np.where(np.abs(x) < 3, v, 0.0))


def down_taps():
    k = window((np.arange(12) - 5.5) / 2)
    return k / k.sum()


def up_taps():
    """(ke for s = -3..2, ko for s = -2..3)"""
    ke = window(np.arange(-3, 3) + 0.25)
    ko = window(np.arange(-2, 4) - 0.25)
    return ke / ke.sum(), ko / ko.sum()


def gauss_taps(g):
    """(taps, anchor) of gblur; g = 0: the identity."""
    if g == 0:
        return np.ones(1), 0
    n = max(2 * int(np.floor(g)), 5)
    x = np.arange(n) - (n - 1) / 2
    w = np.exp(-x * x / (2 * g * g))
    w[w < np.finfo(np.float64).eps * w.max()] = 0
    return w / w.sum(), (n + 1) // 2 - 1


def _clamp(i, n):
    return np.clip(i, 0, n - 1)


def _mirror(i, n):
    i = np.mod(i, 2 * n)
    return np.where(i < n, i, 2 * n - 1 - i)


def _axis(a, axis, fn):
    """apply the 1-D map fn (a (n, ...) -> (m, ...) array function) along axis 1 (x) or 0 (y)"""
    a = np.moveaxis(np.asarray(a, np.float64), axis, 0)
    return np.moveaxis(fn(a), 0, axis)


def down1(x):
    n, k = x.shape[0], down_taps()
    m = np.arange((n + 1) // 2)
    return sum(k[t] * x[_clamp(2 * m + t - 5, n)] for t in range(12))


def up1(x, N):
    n = x.shape[0]
    assert 2 * n - 1 <= N <= 2 * n + 1 and N >= 1
    ke, ko = up_taps()
    j = np.arange(n)
    out = np.empty((2 * n,) + x.shape[1:])
    out[0::2] = sum(ke[s + 3] * x[_clamp(j + s, n)] for s in range(-3, 3))
    out[1::2] = sum(ko[s + 2] * x[_clamp(j + s, n)] for s in range(-2, 4))
    return out[np.minimum(np.arange(N), 2 * n - 1)]


def gblur1(x, g):
    taps, a = gauss_taps(g)
    n = x.shape[0]
    q = np.arange(n)
    return sum(taps[t] * x[_mirror(q + t - a, n)] for t in range(len(taps)))


def down(img):
    return _axis(_axis(img, 1, down1), 0, down1)


def up(img, size):
    """size = (h, w) of the result"""
    return _axis(_axis(img, 1, lambda a: up1(a, size[1])), 0, lambda a: up1(a, size[0]))


def gblur(img, g):
    if g == 0:
        return np.asarray(img, np.float64)
    return _axis(_axis(img, 1, lambda a: gblur1(a, g)), 0, lambda a: gblur1(a, g))


def decompose(img, levels):
    out = [np.asarray(img, np.float64)]
    for _ in range(1, levels):
        out.append(down(out[-1]))
    return out


def recompose_step(yh, rl, g):
    return np.asarray(yh, np.float64) + up(gblur(np.asarray(rl, np.float64) - down(yh), g), yh.shape[:2])


def recompose(levels, g=0.0):
    """levels finest first; the coarsest is the last"""
    r = np.asarray(levels[-1], np.float64)
    for y in reversed(levels[:-1]):
        r = recompose_step(y, r, g)
    return r
