"""The noise-level-function transform of nlk_nlf_build and nlk_dev_nlf_forward / nlk_dev_nlf_inverse (include/nlk_hip.h,
DESIGN.md §9) restated in numpy: the table rule in float64, the two transforms in float32 with every operation rounded
by itself, as the kernels do them. Imports neither the product nor the oracle.

Table, per channel, from the bins (N_q, n_q, m_q, v_q) of curve_ref.estimate measured over [lo, hi) in nbins bins:
  a. K = the bins with n_q > 0 and v_q finite and > 0, in increasing q; an empty K in any channel: s = NaN
  b. vs_k = (n_{k-1} v_{k-1} + 2 n_k v_k + n_{k+1} v_{k+1}) / (n_{k-1} + 2 n_k + n_{k+1}) over neighbours IN K, a
     missing neighbour left out of both sums
  c. vs_k = max(vs_k, rho^2 median(vs))
  d. x_j = lo + j (hi - lo) / nbins, j = 0..nbins; v(x_j) = the linear interpolation of (m_k, vs_k), constant outside
     [m_first, m_last]; sigma_j = sqrt(v(x_j))
  e. kappa_j = 2 / (sigma_j + sigma_{j+1}); g(x_0) = 0, g(x_{j+1}) = g(x_j) + kappa_j (x_{j+1} - x_j); end segments extend
  f. span_c = g_c(255) - g_c(0); s = 255 / mean_c span_c
  g. x[j], G[c][j] = float32(s (g_c(x_j) - g_c(0))), slope[c][j] = float32(s kappa_j),
     islope[c][j] = float32(1 / (s kappa_j)), inv_dx = float32(nbins / (hi - lo))
Transforms, the channel of sample i being i mod ch:
  forward   t = fmin(fmax((y - lo) inv_dx, 0), nbins - 1), j = int(floor(t)), g = G[j] + (y - x[j]) slope[j]
  inverse   j = the number of k in 1..nbins-1 with G[k] <= g, y = x[j] + (g - G[j]) islope[j]"""
import numpy as np

RHO = 0.25


def _g_at(y, x, g, kappa, nbins, lo, hi):
    t = min(max((y - lo) / (hi - lo) * nbins, 0.0), nbins - 1)
    j = int(np.floor(t))
    return g[j] + kappa[j] * (y - x[j])


def build(bins, lo=0.0, hi=256.0, rho=RHO):
    """bins [ch][nbins][4] = (N_q, n_q, m_q, v_q) -> dict(ch, nbins, lo, hi (float32 values), s, inv_dx, kept [ch],
    x [nbins+1], G, sigma [ch][nbins+1], slope, islope [ch][nbins]); the arrays float32, NaN where s is NaN"""
    bins = np.asarray(bins, np.float64)
    ch, nbins = bins.shape[:2]
    lo, hi = float(np.float32(lo)), float(np.float32(hi))
    rho = float(np.float32(rho))
    x = lo + np.arange(nbins + 1) * ((hi - lo) / nbins)
    g = np.full((ch, nbins + 1), np.nan)
    kappa = np.full((ch, nbins), np.nan)
    sigma = np.full((ch, nbins + 1), np.nan)
    g0, span, kept = np.full(ch, np.nan), np.full(ch, np.nan), np.zeros(ch, np.int32)
    for c in range(ch):
        n, m, v = bins[c, :, 1], bins[c, :, 2], bins[c, :, 3]
        with np.errstate(invalid="ignore"):
            keep = (n > 0) & np.isfinite(v) & (v > 0)
        n, m, v = n[keep], m[keep], v[keep]
        kept[c] = len(n)
        if len(n) == 0:
            continue
        vs = np.empty(len(n))
        for k in range(len(n)):
            nb = [i for i in (k - 1, k + 1) if 0 <= i < len(n)]
            vs[k] = (2 * n[k] * v[k] + sum(n[i] * v[i] for i in nb)) / (2 * n[k] + sum(n[i] for i in nb))
        vs = np.maximum(vs, rho * rho * np.median(vs))
        for j in range(nbins + 1):
            if x[j] <= m[0]:
                vj = vs[0]
            elif x[j] >= m[-1]:
                vj = vs[-1]
            else:
                k = int(np.searchsorted(m, x[j], side="right")) - 1       # m_k <= x_j < m_{k+1}
                vj = vs[k] + (x[j] - m[k]) / (m[k + 1] - m[k]) * (vs[k + 1] - vs[k])
            sigma[c, j] = np.sqrt(vj)
        kappa[c] = 2.0 / (sigma[c, :-1] + sigma[c, 1:])
        g[c, 0] = 0.0
        for j in range(nbins):
            g[c, j + 1] = g[c, j] + kappa[c, j] * (x[j + 1] - x[j])
        g0[c] = _g_at(0.0, x, g[c], kappa[c], nbins, lo, hi)
        span[c] = _g_at(255.0, x, g[c], kappa[c], nbins, lo, hi) - g0[c]
    s = 255.0 / span.mean() if np.all(kept > 0) else float("nan")
    with np.errstate(invalid="ignore"):
        return dict(ch=ch, nbins=nbins, lo=lo, hi=hi, s=float(np.float32(s)), inv_dx=np.float32(nbins / (hi - lo)),
                    kept=kept, x=x.astype(np.float32), G=(s * (g - g0[:, None])).astype(np.float32),
                    slope=(s * kappa).astype(np.float32), islope=(1.0 / (s * kappa)).astype(np.float32),
                    sigma=sigma.astype(np.float32))


def _channels(n, ch):
    return np.arange(n, dtype=np.int64) % ch


def forward(y, t):
    """y: any shape, float32, the channel of flat sample i being i mod ch -> float32, every operation rounded by itself"""
    y = np.asarray(y, np.float32)
    f, c = y.reshape(-1), _channels(y.size, t["ch"])
    with np.errstate(invalid="ignore", over="ignore"):
        pos = (f - np.float32(t["lo"])) * np.float32(t["inv_dx"])
        pos = np.fmin(np.fmax(pos, np.float32(0)), np.float32(t["nbins"] - 1))    # (fmax of a NaN and 0 is 0)
        j = np.floor(pos).astype(np.int64)
        out = t["G"][c, j] + (f - t["x"][j]) * t["slope"][c, j]
    assert out.dtype == np.float32
    return out.reshape(y.shape)


def inverse(g, t):
    g = np.asarray(g, np.float32)
    f, c = g.reshape(-1), _channels(g.size, t["ch"])
    with np.errstate(invalid="ignore", over="ignore"):
        j = (t["G"][c, 1:t["nbins"]] <= f[:, None]).sum(axis=1)      # (a NaN counts nothing)
        out = t["x"][j] + (f - t["G"][c, j]) * t["islope"][c, j]
    assert out.dtype == np.float32
    return out.reshape(g.shape)
