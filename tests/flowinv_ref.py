"""nlk_dev_flow_invert (include/nlk_hip.h, csrc/k_flowinv.h) restated in numpy: float32, every operation rounded by
itself, in the kernel's order. For finite flows the kernel gives these bits."""
import numpy as np

F32 = np.float32


def bilinear(B, X, Y):
    """B~ at the positions (X, Y) (float32 arrays, already clamped to the frame): [.., 2]"""
    h, w, _ = B.shape
    x0 = np.clip(np.floor(X).astype(np.int64), 0, w - 1)
    y0 = np.clip(np.floor(Y).astype(np.int64), 0, h - 1)
    x1, y1 = np.minimum(x0 + 1, w - 1), np.minimum(y0 + 1, h - 1)
    fx, fy = (X - x0.astype(F32))[..., None], (Y - y0.astype(F32))[..., None]
    b00, b01, b10, b11 = B[y0, x0], B[y0, x1], B[y1, x0], B[y1, x1]
    top = b00 + fx * (b01 - b00)
    bot = b10 + fx * (b11 - b10)
    return top + fy * (bot - top)


def step(B, F):
    """F_{k+1} = -B~(q + F_k)"""
    h, w, _ = B.shape
    x, y = np.arange(w, dtype=F32)[None, :], np.arange(h, dtype=F32)[:, None]
    X = np.minimum(np.maximum(x + F[..., 0], F32(0)), F32(w - 1))
    Y = np.minimum(np.maximum(y + F[..., 1], F32(0)), F32(h - 1))
    return -bilinear(B, X, Y)


def invert(B, iters=4):
    """B: [h][w][2] float32 (u, v) pairs; F_0 = -B, then `iters` steps"""
    B = np.ascontiguousarray(B, F32)
    assert B.ndim == 3 and B.shape[2] == 2 and 0 <= iters <= 16
    F = -B
    for _ in range(iters):
        F = step(B, F)
    assert F.dtype == F32
    return F
