"""The defective-pixel rule of nlk_dev_despike (include/nlk_hip.h), stated once in float32 numpy.

despike(img, thr, radius) -> (out, counts) for an HWC float32 image, every channel by itself:
  ring of (x, y)   the samples at Chebyshev distance exactly `radius`: 8 values for radius 1, 16 for radius 2
  border indices   along an axis of n samples: j = |i|; j = 2 (n - 1) - j if j >= n; then clamped to [0, n - 1]
                   (a reflection that does not repeat the edge; the clamp keeps frames smaller than the ring total)
  mn, mx           the ring's minimum and maximum; lo, hi its two middle order statistics (4th and 5th of 8, 8th and
                   9th of 16); med = (lo + hi) * 0.5, one float32 rounding each
  hit              v > mx + thr or v < mn - thr, one float32 add / subtract each: writes med. Anything else copies v
                   bit for bit; so does a sample that is non-finite or whose ring holds a non-finite value
  counts[c]        the replaced samples of channel c (uint32)
-0 and +0 compare equal; the sign of a replaced value that equals zero is unspecified (same_bits compares such samples
as numbers and everything else as bits)."""
import numpy as np


def border_index(i, n):
    """the in-frame index of i along an axis of n samples (i: an integer array)"""
    j = np.abs(np.asarray(i, np.int64))
    j = np.where(j >= n, 2 * (n - 1) - j, j)
    return np.clip(j, 0, n - 1)


def ring_offsets(radius):
    """(dx, dy) of the ring, row by row"""
    r = int(radius)
    return [(dx, dy) for dy in range(-r, r + 1) for dx in range(-r, r + 1) if max(abs(dx), abs(dy)) == r]


def ring_stack(img, radius):
    """[N][h][w][ch]: the ring values of every sample"""
    img = np.asarray(img, np.float32)
    h, w = img.shape[:2]
    ys, xs = np.arange(h), np.arange(w)
    return np.stack([img[border_index(ys + dy, h)][:, border_index(xs + dx, w)] for dx, dy in ring_offsets(radius)])


def despike(img, thr, radius=1):
    img = np.ascontiguousarray(img, np.float32)
    if img.ndim != 3:
        raise ValueError("despike: want an HWC image")
    if radius not in (1, 2):
        raise ValueError("despike: radius is 1 or 2")
    thr = np.float32(thr)
    ring = ring_stack(img, radius)
    n = ring.shape[0]
    with np.errstate(invalid="ignore", over="ignore"):
        ok = np.isfinite(img) & np.isfinite(ring).all(axis=0)
        srt = np.sort(np.where(ok[None], ring, np.float32(0)), axis=0)
        mn, mx = srt[0], srt[-1]
        lo, hi = srt[n // 2 - 1], srt[n // 2]
        med = ((lo + hi).astype(np.float32) * np.float32(0.5)).astype(np.float32)
        hit = ok & ((img > (mx + thr).astype(np.float32)) | (img < (mn - thr).astype(np.float32)))
    out = np.where(hit, med, img).astype(np.float32)
    counts = hit.reshape(-1, img.shape[2]).sum(axis=0).astype(np.uint32)
    return out, counts


def same_bits(a, b):
    """a and b agree bit for bit, except where both are zero (of either sign)"""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    if a.shape != b.shape:
        return False
    zero = (a == 0) & (b == 0)
    return bool(np.all(zero | (a.view(np.uint32) == b.view(np.uint32))))


# ---- what the filter is for: the recursion's chain on the CPU oracle with defective sensor sites
# (tests/test_despike.py, tools/despike_table.py). All of it is synthetic.

def defect_sites(w, h, n=21, border=3, seed=2024, blob=1):
    """n fixed sensor positions (x, y, value): `border` of them on the frame's border, 70 % stuck at 255, the rest at
    0; no two closer than 4 pixels, so that every ring holds one defect at most. blob = 2: each is the top-left
    corner of a 2 x 2 blob, kept off the border (a blob there reflects onto itself: a stated limit of the filter)."""
    rng = np.random.default_rng(seed)
    sites = []
    while len(sites) < n:
        if len(sites) < border and blob == 1:
            side = len(sites) % 3
            x, y = ((0, int(rng.integers(1, h - 1))), (int(rng.integers(1, w - 1)), h - 1), (w - 1, 0))[side]
        else:
            x, y = int(rng.integers(2, w - 3)), int(rng.integers(2, h - 3))
        if all(max(abs(x - a), abs(y - b)) >= 4 + blob for a, b, _ in sites):
            sites.append((x, y, 255.0 if len(sites) % 10 < 7 else 0.0))
    return sites


def plant(img, sites, blob=1):
    out = np.array(img, np.float32)
    for x, y, v in sites:
        out[y:y + blob, x:x + blob] = v
    return out


def site_mask(shape, sites, blob=1):
    m = np.zeros(shape[:2], bool)
    for x, y, _ in sites:
        m[y:y + blob, x:x + blob] = True
    return m


def chain(O, synth, sigma, prep=None, nf=4, w=96, h=64, sites=None, blob=1):
    """bmflow_ref.chain_psnr's chain (TV-L1 -> mask 0.75 -> warp -> FLT1 -> FLT2, free running, default parameters) on
    the 2 px/frame pan of synth.clean_frame, noise seeds 300 + t; prep(noisy RGB frame) is what the sensor and a
    pre-filter do to the frame before the chain sees it. Returns (the flt2 PSNR of every frame, the RMSE of every flt2
    frame in RGB at the sites (NaN without sites), the flt2 frames)."""
    from bmflow_ref import lum
    p1, p2 = O.default_params(sigma, O.FLT1), O.default_params(sigma, O.FLT2)
    f1 = f2 = None
    ps, rm, outs = [], [], []
    mask = site_mask((h, w), sites, blob) if sites else None
    for t in range(nf):
        clean = synth.clean_frame(w, h, 3, t)
        rgb = synth.awgn(clean, sigma, 300 + t)
        if prep is not None:
            rgb = np.ascontiguousarray(prep(rgb), np.float32)
        nz = O.rgb2opp(rgb)
        if t == 0:
            f1 = O.filter_frame(nz, None, None, sigma, p1)
            f2 = O.filter_frame(nz, None, f1, sigma, p2)
        else:
            B = np.ascontiguousarray(np.stack(O.tvl1_flow(lum(rgb), lum(O.opp2rgb(f2)), lam=0.25, fscale=1), -1), np.float32)
            occ = O.tvl1_occlusion_mask(B, 0.75)
            n1 = O.filter_frame(nz, O.warp_bicubic(f1, B, occ), None, sigma, p1)
            f2 = O.filter_frame(nz, O.warp_bicubic(f2, B, occ), n1, sigma, p2)
            f1 = n1
        ps.append(synth.psnr(f2, O.rgb2opp(clean)))
        d = (O.opp2rgb(f2).astype(np.float64) - clean)[mask] if sites else np.array([np.nan])
        rm.append(float(np.sqrt(np.mean(d ** 2))))
        outs.append(f2)
    return ps, rm, outs
