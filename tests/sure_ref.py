"""Monte-Carlo SURE (Ramani, Blu, Unser 2008) as the project computes it (include/nlk_hip.h: nlk_dev_probe_add,
nlk_dev_sure_terms, nlk_sure_mse; host/seq_step.h: seq_sure_step), restated in numpy: the sign generator
with uint64 arithmetic, the probe in float32, the sums in float64, and the chain of the sequence tools on the CPU oracle.

For a frame y of N samples under white Gaussian noise of deviation sigma, f = the filter's output, b independent signs:

    MSE_hat = R / N - sigma^2 + 2 sigma^2 D / (eps N),   R = sum (y - f)^2,   D = sum b (f(y + eps b) - f(y))

Imports numpy only; the chain takes the oracle and the frame synthesis as arguments."""
import numpy as np

F32 = np.float32
MASK = (1 << 64) - 1
GOLDEN, MIX1, MIX2 = 0x9E3779B97F4A7C15, 0xBF58476D1CE4E5B9, 0x94D049BB133111EB
FRAME_STEP = 0xD1B54A32D192ED03   # seed of frame t = seed + t * FRAME_STEP (mod 2^64)
EPS_REL = 0.05                    # the default probe size, in units of sigma
BLOCK = 16                        # the default tile of the risk map


def sign_py(i, seed):
    """b_i by plain big-integer arithmetic: the five lines of the definition"""
    z = (seed + (i + 1) * GOLDEN) & MASK
    z = ((z ^ (z >> 30)) * MIX1) & MASK
    z = ((z ^ (z >> 27)) * MIX2) & MASK
    z ^= z >> 31
    return -1 if z >> 63 else 1


def signs(n, seed, start=0):
    """b_i for i = start .. start + n - 1 as int8 (+1 | -1)"""
    with np.errstate(over="ignore"):
        z = np.uint64(seed & MASK) + (np.arange(start, start + n, dtype=np.uint64) + np.uint64(1)) * np.uint64(GOLDEN)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(MIX1)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(MIX2)
        z ^= z >> np.uint64(31)
    return np.where(z >> np.uint64(63), -1, 1).astype(np.int8)


def frame_seed(seed, t):
    return (seed + t * FRAME_STEP) & MASK


def probe_add(x, eps, seed):
    """x + (b_i > 0 ? eps : -eps) in float32, i the index of the flattened array"""
    x = np.ascontiguousarray(x, F32)
    e = F32(eps)
    return (x + np.where(signs(x.size, seed).reshape(x.shape) > 0, e, -e).astype(F32)).astype(F32)


def terms(y, f, fp, seed, block=None, order=0):
    """totals [ch][2] = (R_c, D_c) of the HWC images y, f, fp in float64; with `block` also the map [nby][nbx][ch][2] of
    the same sums over block x block tiles (ragged at the right and bottom). order != 0: the same sums added in another
    order (what sets the tests' bar)."""
    y, f, fp = (np.asarray(a, F32).astype(np.float64) for a in (y, f, fp))
    if y.ndim == 2:
        y, f, fp = y[..., None], f[..., None], fp[..., None]
    h, w, ch = y.shape
    b = signs(y.size, seed).reshape(y.shape).astype(np.float64)
    r, d = (y - f) ** 2, b * (fp - f)
    both = np.stack([r, d], -1)                      # [h][w][ch][2]
    if order:
        tot = both[::-1, ::-1].cumsum(0)[-1].cumsum(0)[-1]
    else:
        tot = both.sum((0, 1))
    if block is None:
        return tot
    nby, nbx = -(-h // block), -(-w // block)
    pad = np.zeros((nby * block, nbx * block, ch, 2))
    pad[:h, :w] = both
    tiles = pad.reshape(nby, block, nbx, block, ch, 2)
    if order:
        blocks = tiles[:, ::-1, :, ::-1].cumsum(1)[:, -1].cumsum(2)[:, :, -1]
    else:
        blocks = tiles.sum((1, 3))
    return tot, blocks


def mse(R, D, n, sigma, eps):
    """the estimate from its two sums over n samples"""
    s2 = float(sigma) ** 2
    return R / n - s2 + 2.0 * s2 * D / (eps * n)


def estimate(y, f, fp, seed, sigma, eps):
    """dict(mse, psnr, resid = R / N, div = D / (eps N)) of all samples, and the same per channel (arrays) as mse_ch ..."""
    tot = terms(y, f, fp, seed)
    npix = np.asarray(y).size // tot.shape[0]
    out = {}
    for key, R, D, n in (("", tot[:, 0].sum(), tot[:, 1].sum(), npix * tot.shape[0]), ("_ch", tot[:, 0], tot[:, 1], npix)):
        m = mse(R, D, n, sigma, eps)
        out["mse" + key], out["resid" + key], out["div" + key] = m, R / n, D / (eps * n)
        with np.errstate(invalid="ignore", divide="ignore"):
            out["psnr" + key] = 10.0 * np.log10(255.0 ** 2 / m)
    return out


# ---- the linear filter of the formula's test: the 3 x 3 box mean with replicated edges

def box3(x):
    x = np.asarray(x, np.float64)
    p = np.pad(x, 1, mode="edge")
    h, w = x.shape
    return sum(p[i:i + h, j:j + w] for i in range(3) for j in range(3)) / 9.0


def box3_trace(h, w):
    """trace of box3's matrix: the weight a sample has in its own mean (a replicated edge counts again)"""
    cy = np.full(h, 1.0)
    cx = np.full(w, 1.0)
    cy[[0, -1]] += 1.0
    cx[[0, -1]] += 1.0
    if h == 1:
        cy[:] = 3.0
    if w == 1:
        cx[:] = 3.0
    return float(np.outer(cy, cx).sum() / 9.0)


# ---- the chain of the sequence tools on the CPU oracle, with the probe

def lum(rgb):
    c = np.asarray(rgb, F32).astype(np.float64)
    if c.ndim == 2 or c.shape[-1] == 1:
        return c.reshape(c.shape[:2]).astype(F32)
    return (.299 * c[..., 0] + .587 * c[..., 1] + .114 * c[..., 2]).astype(F32)


def scaled(p, k):
    """the parameter set p with both beta scaled by k"""
    q = type(p).from_buffer_copy(p)
    q.beta_x, q.beta_t = p.beta_x * k, p.beta_t * k
    return q


def chain(O, synth, scene, sigma, flow_of, nf=3, eps_rel=EPS_REL, seeds=(0,), noise_seed=300, beta=1.0,
          sigma_stated=None, probe_before_flow=False):
    """flow -> mask(0.75) -> warp -> FLT1 -> FLT2 free running on the CPU oracle O over the clean frames scene(t) with
    noise of seed noise_seed + t (tests/bmflow_ref.py: chain_psnr), and per frame the probe evaluation of seq_sure_step
    for every probe seed: the probe eps_rel * sigma on the opponent-space noisy frame, the same flow, mask and warps,
    FLT1' then FLT2' with FLT1' as its basic estimate. flow_of(gray of the noisy frame, gray of the previous flt2) is
    the flow. Returns per frame dict(true1, true2 = the errors against the clean frame, est1, est2 = [per seed] the
    dicts of `estimate`). sigma_stated: the sigma given to the formula (default: the true one). probe_before_flow: the
    probe evaluation computes a flow of its own from the perturbed frame."""
    p1 = scaled(O.default_params(sigma, O.FLT1), beta)
    p2 = scaled(O.default_params(sigma, O.FLT2), beta)
    eps = float(F32(eps_rel) * F32(sigma))   # (the product in float32, as seq_sure_step makes it)
    said = sigma if sigma_stated is None else sigma_stated
    f1 = f2 = None
    out = []
    for t in range(nf):
        clean = scene(t).astype(F32)
        rgb = synth.awgn(clean, sigma, noise_seed + t)
        nz = O.rgb2opp(rgb)
        if t == 0:
            w1 = w2 = None
        else:
            B = np.ascontiguousarray(flow_of(lum(rgb), lum(O.opp2rgb(f2))), F32)
            occ = O.tvl1_occlusion_mask(B, 0.75)
            w1, w2 = O.warp_bicubic(f1, B, occ), O.warp_bicubic(f2, B, occ)
        n1 = O.filter_frame(nz, w1, None, sigma, p1)
        n2 = O.filter_frame(nz, w2, n1, sigma, p2)
        ref = O.rgb2opp(clean).astype(np.float64)
        rec = dict(true1=float(np.mean((n1 - ref) ** 2)), true2=float(np.mean((n2 - ref) ** 2)), est1=[], est2=[])
        for seed in seeds:
            st = frame_seed(seed, t)
            pz = probe_add(nz, eps, st)
            v1, v2 = w1, w2
            if probe_before_flow and t > 0:
                Bp = np.ascontiguousarray(flow_of(lum(O.opp2rgb(pz)), lum(O.opp2rgb(f2))), F32)
                occp = O.tvl1_occlusion_mask(Bp, 0.75)
                v1, v2 = O.warp_bicubic(f1, Bp, occp), O.warp_bicubic(f2, Bp, occp)
            q1 = O.filter_frame(pz, v1, None, sigma, p1)
            q2 = O.filter_frame(pz, v2, q1, sigma, p2)
            rec["est1"].append(estimate(nz, n1, q1, st, said, eps))
            rec["est2"].append(estimate(nz, n2, q2, st, said, eps))
        out.append(rec)
        f1, f2 = n1, n2
    return out
