"""The defect map learned over time: the rule of nlk_dev_defect_step and the schedule of nlk_defect_schedule
(include/nlk_hip.h), stated once in float32 numpy, every operation rounded by itself.

A sensor defect sits at the same coordinates in every frame; scene and noise do not. The mean of the noisy frames,
taken without motion compensation, carries noise sigma / sqrt(T) while the defect keeps its height: despike's range
test (despike_ref), read on that mean with a threshold that shrinks as 1 / sqrt(T), finds it.

step(v, m, thr, gain, radius) -> (out, m_new, hit, counts); v: the noisy HWC frame, m: the mean of the frames before
it (None on the first frame). Every channel by itself:
  hit      m > mx + thr or m < mn - thr, mn and mx the minimum and maximum of m's ring at Chebyshev distance `radius`
           (despike_ref.ring_stack: the same border reflection). No hit where m or its ring is non-finite, and none at
           all on the first frame
  out      at a hit (lo + hi) * 0.5f, lo and hi the two middle order statistics of v's ring, if v and its ring are all
           finite; everything else is v, bit for bit
  m_new    m + (v - m) * gain for a finite v, else m; on the first frame v, or 0 for a non-finite v. The mean takes the
           raw v at hit sites too: a flagged site that lost its evidence would flicker
  counts   counts[c] = the replaced samples of channel c (uint32): the hits whose v and ring are finite
schedule(t, n_window, k_sigma) -> (thr, gain) for the frame of index t >= 1 (the first frame needs neither):
  gain = 1f / (float)min(t + 1, N), thr = k_sigma * sqrtf(1f / (float)min(t, N))
an exact mean up to N frames, then an exponential window, whose noise is below sigma / sqrt(N): the threshold stays on
the safe side.

The noise of anything here that averages over time comes from np.random.default_rng(seed + t). synth.awgn with
consecutive seeds (what despike_ref.chain uses) is not independent enough across frames for a temporal mean: the same
experiment with it flags up to 207 clean samples per frame where independent noise flags none."""
import numpy as np

from despike_ref import ring_stack

F32 = np.float32


def schedule(t, n_window, k_sigma):
    t, n = int(t), int(n_window)
    if t < 1 or n < 1:
        raise ValueError("schedule: t >= 1 and n_window >= 1")
    gain = F32(F32(1) / F32(min(t + 1, n)))
    thr = F32(F32(k_sigma) * np.sqrt(F32(F32(1) / F32(min(t, n)))))
    return thr, gain


def step(v, m, thr, gain, radius=1):
    v = np.ascontiguousarray(v, F32)
    if v.ndim != 3:
        raise ValueError("step: want an HWC frame")
    if radius not in (1, 2):
        raise ValueError("step: radius is 1 or 2")
    ch = v.shape[2]
    with np.errstate(invalid="ignore", over="ignore"):
        fin = np.isfinite(v)
        if m is None:
            m_new = np.where(fin, v, F32(0)).astype(F32)
            return v.copy(), m_new, np.zeros(v.shape, bool), np.zeros(ch, np.uint32)
        m = np.ascontiguousarray(m, F32)
        thr, gain = F32(thr), F32(gain)
        mr = ring_stack(m, radius)
        mok = np.isfinite(m) & np.isfinite(mr).all(axis=0)
        safe = np.where(mok[None], mr, F32(0))
        mn, mx = safe.min(axis=0), safe.max(axis=0)
        hit = mok & ((m > (mx + thr).astype(F32)) | (m < (mn - thr).astype(F32)))
        vr = ring_stack(v, radius)
        n = vr.shape[0]
        vok = fin & np.isfinite(vr).all(axis=0)
        srt = np.sort(np.where(vok[None], vr, F32(0)), axis=0)
        med = ((srt[n // 2 - 1] + srt[n // 2]).astype(F32) * F32(0.5)).astype(F32)
        rep = hit & vok
        out = np.where(rep, med, v).astype(F32)
        upd = (m + ((v - m).astype(F32) * gain).astype(F32)).astype(F32)
        m_new = np.where(fin, upd, m).astype(F32)
    counts = rep.reshape(-1, ch).sum(axis=0).astype(np.uint32)
    return out, m_new, hit, counts


def run(frames, k_sigma, radius=1, n_window=32):
    """the steps over a list of frames from an empty mean -> [(out, hit, counts)] per frame"""
    m, res = None, []
    for t, v in enumerate(frames):
        thr, gain = schedule(t, n_window, k_sigma) if t else (F32(0), F32(1))
        out, m, hit, counts = step(v, m, thr, gain, radius)
        res.append((out, hit, counts))
    return res


# ---- what the map is for: the recursion's chain on the CPU oracle with defective sensor sites
# (tests/test_defect_map.py, tools/defectmap_table.py). All of it is synthetic.

def noisy_frame(synth, sigma, t, w=96, h=64, static=False):
    """(clean, noisy) frame t of the 2 px/frame pan of synth.clean_frame (static: frame 0 every time), the noise of
    frame t from np.random.default_rng(300 + t): independent across frames (see the head of this file)"""
    clean = synth.clean_frame(w, h, 3, 0 if static else t)
    noise = np.random.default_rng(300 + t).normal(0, sigma, clean.shape)
    return clean, (clean + noise).astype(F32)


class Cleaner:
    """prep for chain(): the sensor (plant), then the defect map's steps (k_map: None = off) and despike (k_despike:
    None = off) in the tools' order, at K sigma. .replaced: the samples the map replaced on every frame."""

    def __init__(self, sigma, sites=None, blob=1, k_map=None, k_despike=None, n_window=32):
        self.sigma, self.sites, self.blob, self.k_map, self.k_despike, self.n = sigma, sites, blob, k_map, k_despike, n_window
        self.t, self.m, self.replaced = 0, None, []

    def __call__(self, a):
        import despike_ref as DR
        if self.sites:
            a = DR.plant(a, self.sites, self.blob)
        if self.k_map is not None:
            thr, gain = schedule(self.t, self.n, F32(self.k_map) * F32(self.sigma)) if self.t else (F32(0), F32(1))
            a, self.m, _, counts = step(a, self.m, thr, gain, self.blob)
            self.replaced.append(int(counts.sum()))
        if self.k_despike is not None:
            a = DR.despike(a, float(F32(self.k_despike) * F32(self.sigma)), self.blob)[0]
        self.t += 1
        return a


def chain(O, synth, sigma, prep=None, nf=24, w=96, h=64, sites=None, blob=1, static=False):
    """despike_ref.chain's chain (TV-L1 -> mask 0.75 -> warp -> FLT1 -> FLT2, free running, default parameters) with
    noisy_frame's frames; prep(noisy RGB frame) is called once per frame, in order. Returns (the flt2 PSNR of every
    frame, the RMSE of every flt2 frame in RGB at the sites (NaN without sites), the flt2 frames)."""
    from bmflow_ref import lum
    from despike_ref import site_mask
    p1, p2 = O.default_params(sigma, O.FLT1), O.default_params(sigma, O.FLT2)
    f1 = f2 = None
    ps, rm, outs = [], [], []
    mask = site_mask((h, w), sites, blob) if sites else None
    for t in range(nf):
        clean, rgb = noisy_frame(synth, sigma, t, w, h, static)
        if prep is not None:
            rgb = np.ascontiguousarray(prep(rgb), F32)
        nz = O.rgb2opp(rgb)
        if t == 0:
            f1 = O.filter_frame(nz, None, None, sigma, p1)
            f2 = O.filter_frame(nz, None, f1, sigma, p2)
        else:
            B = np.ascontiguousarray(np.stack(O.tvl1_flow(lum(rgb), lum(O.opp2rgb(f2)), lam=0.25, fscale=1), -1), F32)
            occ = O.tvl1_occlusion_mask(B, 0.75)
            n1 = O.filter_frame(nz, O.warp_bicubic(f1, B, occ), None, sigma, p1)
            f2 = O.filter_frame(nz, O.warp_bicubic(f2, B, occ), n1, sigma, p2)
            f1 = n1
        ps.append(synth.psnr(f2, O.rgb2opp(clean)))
        d = (O.opp2rgb(f2).astype(np.float64) - clean)[mask] if sites else np.array([np.nan])
        rm.append(float(np.sqrt(np.mean(d ** 2))))
        outs.append(f2)
    return ps, rm, outs
