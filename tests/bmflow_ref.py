"""nlk_dev_bm_flow (include/nlk_hip.h, csrc/k_bmflow.h) restated in numpy: the block-matching optical flow, float32,
every operation rounded by itself, sums in the written order. For finite images the kernels give these bits.

flow(I0, I1)[y][x] = (u, v) with I1(q + flow(q)) ~ I0(q): the layout and direction of nlk_dev_tvl1_flow.

  pyramid   level l + 1 = the 2 x 2 box mean ((a00 + a01) + (a10 + a11)) * 0.25 of level l, of floor(w / 2) x floor(h / 2)
            pixels; levels are added while min(w_l, h_l) // 2 >= min_side (a min_side below 8, the side of a block,
            counts as 8). L = the number of levels added.
  finest    the finest level that is matched is min(fscale, L); an image with a side below 8 has the flow 0.
  blocks    8 x 8, stride 4: along n pixels the origins min(4 i, n - 8), i = 0 .. ceil((n - 8) / 4)
  per level, from the coarsest (prediction 0) to the finest:
    prediction  of a block: the coarser level's dense flow, upsampled (up2) at the pixel (ox + 4, oy + 4); per component
                rint, int, clamped to +-(w_l + h_l)
    search      cost(dy, dx) = sum over rows, then columns, of (T - I1[clamp(y)][clamp(x)])^2 for (dy, dx) in
                [-(R + 1), R + 1]^2, the coordinates clamped after every offset is added; the winner is the lowest cost
                of the inner [-R, R]^2, the first in raster order (dy outer) among equals
    sub-pel     per axis, from the winner's two neighbours: den = (cm - 2 c0) + cp; 0 if den <= 0, else
                (0.5 (cm - cp)) / den clamped to +-0.5; the block's vector is (float)(prediction + winner) + that
    median      3 x 3 over the block grid, per component, edges replicated
    dense       bilinear between the block centres (origin + 3.5): k = the last centre <= q, clamped to 0 .. nb - 2,
                t = clamp((q - c_k) / (c_{k+1} - c_k), 0, 1) (one block: t = 0), top + t_y (bot - top) as
                tests/flowinv_ref.py
  up2       from the finest matched level down to level 0: X = clamp((x - 0.5) * 0.5, 0, w_l - 1), the same in y,
            bilinear as above, times 2
"""
import numpy as np

F32 = np.float32
BLOCK, STRIDE = 8, 4


def box_down(a):
    h2, w2 = a.shape[0] // 2, a.shape[1] // 2
    a = a[:2 * h2, :2 * w2]
    return ((a[0::2, 0::2] + a[0::2, 1::2]) + (a[1::2, 0::2] + a[1::2, 1::2])) * F32(0.25)


def pyramid(img, min_side=16):
    levels = [np.ascontiguousarray(img, F32)]
    while min(levels[-1].shape) // 2 >= max(int(min_side), BLOCK):
        levels.append(box_down(levels[-1]))
    return levels


def origins(n):
    nb = -(-(n - BLOCK) // STRIDE) + 1
    return np.minimum(STRIDE * np.arange(nb), n - BLOCK)


def bilinear(A, X, Y):
    """A [h][w][2] at the positions (X, Y), float32 arrays inside the frame (tests/flowinv_ref.py's)"""
    h, w, _ = A.shape
    x0 = np.clip(np.floor(X).astype(np.int64), 0, w - 1)
    y0 = np.clip(np.floor(Y).astype(np.int64), 0, h - 1)
    x1, y1 = np.minimum(x0 + 1, w - 1), np.minimum(y0 + 1, h - 1)
    fx, fy = (X - x0.astype(F32))[..., None], (Y - y0.astype(F32))[..., None]
    a00, a01, a10, a11 = A[y0, x0], A[y0, x1], A[y1, x0], A[y1, x1]
    top = a00 + fx * (a01 - a00)
    bot = a10 + fx * (a11 - a10)
    return top + fy * (bot - top)


def up2_at(A, x, y):
    """twice the flow A [hs][ws][2] of the coarser level at the pixels (x, y) (integer arrays) of the finer one"""
    hs, ws, _ = A.shape
    X = np.minimum(np.maximum((x.astype(F32) - F32(0.5)) * F32(0.5), F32(0)), F32(ws - 1))
    Y = np.minimum(np.maximum((y.astype(F32) - F32(0.5)) * F32(0.5), F32(0)), F32(hs - 1))
    X, Y = np.broadcast_arrays(X, Y)
    return bilinear(A, X, Y) * F32(2)


def up2(A, w, h):
    return up2_at(A, np.arange(w)[None, :], np.arange(h)[:, None])


def _axis(n):
    """per pixel along a side of n: the two block indices and the weight of the second"""
    o = origins(n)
    nb, q = len(o), np.arange(n)
    if nb == 1:
        return np.zeros(n, np.int64), np.zeros(n, np.int64), np.zeros(n, F32)
    c = o.astype(F32) + F32(3.5)
    k = np.clip((q - 4) >> 2, 0, nb - 2)
    t = (q.astype(F32) - c[k]) / (c[k + 1] - c[k])
    return k, k + 1, np.minimum(np.maximum(t, F32(0)), F32(1))


def dense(V, w, h):
    """block vectors V [nby][nbx][2] -> the flow of the w x h level"""
    kx0, kx1, tx = _axis(w)
    ky0, ky1, ty = _axis(h)
    tx, ty = tx[None, :, None], ty[:, None, None]
    v00, v01 = V[ky0[:, None], kx0[None, :]], V[ky0[:, None], kx1[None, :]]
    v10, v11 = V[ky1[:, None], kx0[None, :]], V[ky1[:, None], kx1[None, :]]
    top = v00 + tx * (v01 - v00)
    bot = v10 + tx * (v11 - v10)
    return top + ty * (bot - top)


def median3(V):
    P = np.pad(V, ((1, 1), (1, 1), (0, 0)), mode="edge")
    nby, nbx, _ = V.shape
    nine = np.stack([P[j:j + nby, i:i + nbx] for j in range(3) for i in range(3)])
    return np.sort(nine, axis=0)[4]


def _subpel(cm, c0, cp):
    den = (cm - F32(2) * c0) + cp
    with np.errstate(all="ignore"):
        off = (F32(0.5) * (cm - cp)) / den
    off = np.minimum(np.maximum(off, F32(-0.5)), F32(0.5))
    return np.where(den > 0, off, F32(0)).astype(F32)


def match(T0, I1, pred, R):
    """block vectors [nby][nbx][2] of one level; pred: int [nby][nbx][2] (x, y)"""
    h, w = T0.shape
    oy, ox = origins(h), origins(w)
    S = 2 * R + 3
    off = np.arange(S) - (R + 1)
    px, py = pred[..., 0][:, :, None, None], pred[..., 1][:, :, None, None]
    cost = np.zeros((len(oy), len(ox), S, S), F32)
    for r in range(BLOCK):
        yy = np.clip(oy[:, None, None, None] + r + py + off[None, None, :, None], 0, h - 1)
        for c in range(BLOCK):
            xx = np.clip(ox[None, :, None, None] + c + px + off[None, None, None, :], 0, w - 1)
            d = T0[oy[:, None] + r, ox[None, :] + c][:, :, None, None] - I1[yy, xx]
            cost = cost + d * d
    assert cost.dtype == F32
    inner = cost[:, :, 1:-1, 1:-1].reshape(len(oy), len(ox), -1)
    win = np.argmin(inner, axis=-1)                      # the first of equal minima, raster order
    iy, ix = win // (S - 2) + 1, win % (S - 2) + 1
    by, bx = np.arange(len(oy))[:, None], np.arange(len(ox))[None, :]
    c0 = cost[by, bx, iy, ix]
    sx = _subpel(cost[by, bx, iy, ix - 1], c0, cost[by, bx, iy, ix + 1])
    sy = _subpel(cost[by, bx, iy - 1, ix], c0, cost[by, bx, iy + 1, ix])
    u = (pred[..., 0] + ix - (R + 1)).astype(F32) + sx
    v = (pred[..., 1] + iy - (R + 1)).astype(F32) + sy
    return np.stack([u, v], -1)


def flow(I0, I1, fscale=1, radius=2, min_side=16):
    I0, I1 = np.ascontiguousarray(I0, F32), np.ascontiguousarray(I1, F32)
    assert I0.ndim == 2 and I0.shape == I1.shape and fscale >= 0 and 1 <= radius <= 3
    h, w = I0.shape
    if w < BLOCK or h < BLOCK:
        return np.zeros((h, w, 2), F32)
    P0, P1 = pyramid(I0, min_side), pyramid(I1, min_side)
    L = len(P0) - 1
    f = min(fscale, L)
    D = None
    for l in range(L, f - 1, -1):
        hl, wl = P0[l].shape
        oy, ox = origins(hl), origins(wl)
        if D is None:
            pred = np.zeros((len(oy), len(ox), 2), np.int64)
        else:
            p = up2_at(D, (ox + 4)[None, :], (oy + 4)[:, None])
            pred = np.clip(np.rint(p).astype(np.int64), -(wl + hl), wl + hl)
        D = dense(median3(match(P0[l], P1[l], pred, radius)), wl, hl)
    for l in range(f - 1, -1, -1):
        D = up2(D, P0[l].shape[1], P0[l].shape[0])
    assert D.dtype == F32 and D.shape == (h, w, 2)
    return D


# ---- what the flow is for: the recursion's chain on the CPU oracle (tests/test_bmflow.py, tools/bmflow_table.py)

def lum(rgb):
    c = rgb.astype(np.float64)
    return (.299 * c[..., 0] + .587 * c[..., 1] + .114 * c[..., 2]).astype(F32)


def chain_psnr(O, synth, scene, sigma, flow_of, nf=4):
    """flow -> mask(0.75) -> warp -> FLT1 -> FLT2, free running on the CPU oracle O over the clean frames scene(t),
    t = 0 .. nf - 1, with noise of seed 300 + t; flow_of(gray of the noisy frame, gray of the previous flt2) is the flow.
    The mean flt2 PSNR of frames 1 .. nf - 1."""
    p1, p2 = O.default_params(sigma, O.FLT1), O.default_params(sigma, O.FLT2)
    f1 = f2 = None
    ps = []
    for t in range(nf):
        clean = scene(t).astype(F32)
        rgb = synth.awgn(clean, sigma, 300 + t)
        nz = O.rgb2opp(rgb)
        if t == 0:
            f1 = O.filter_frame(nz, None, None, sigma, p1)
            f2 = O.filter_frame(nz, None, f1, sigma, p2)
            continue
        B = np.ascontiguousarray(flow_of(lum(rgb), lum(O.opp2rgb(f2))), F32)
        occ = O.tvl1_occlusion_mask(B, 0.75)
        n1 = O.filter_frame(nz, O.warp_bicubic(f1, B, occ), None, sigma, p1)
        f2 = O.filter_frame(nz, O.warp_bicubic(f2, B, occ), n1, sigma, p2)
        f1 = n1
        ps.append(synth.psnr(f2, O.rgb2opp(clean)))
    return float(np.mean(ps))
