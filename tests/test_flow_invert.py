"""nlk_dev_flow_invert (csrc/k_flowinv.h): the inverse of a flow by fixed-point steps. The numpy restatement
(tests/flowinv_ref.py) is checked for what it must compute; the kernel is checked against the restatement, bit for
bit."""
import numpy as np
import pytest

import flowinv_ref as FR

F32 = np.float32


def _bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


# ------------------------------------------------------------ CPU: the restatement

@pytest.mark.parametrize("iters", [0, 1, 4, 16])
def test_ref_constant_flow_gives_minus_b(iters):
    B = np.empty((12, 16, 2), F32)
    B[..., 0], B[..., 1] = 2.5, -1.25
    assert np.array_equal(_bits(FR.invert(B, iters)), _bits(-B))


def test_ref_smooth_flow_contracts():
    """|F_k + B~(q + F_k)| = |F_{k+1} - F_k| shrinks by the slope L of B per step (B~, the bilinear interpolation, has
    the finite-difference slopes of B), and |F_1 - F_0| = |B(q) - B~(q - B(q))| <= L max|B|: after 4 steps the residual
    is below L^4 max|B|. L bounds |B(p) - B(q)|_inf / |p - q|_inf: per component the sum of its largest slopes along x
    and along y; each component of this flow varies along one axis only, so L is the largest finite-difference slope."""
    w, h = 64, 48
    y, x = np.mgrid[0:h, 0:w]
    B = np.stack([1.5 * np.sin(y / 7.0), 0.8 * np.cos(x / 9.0)], -1).astype(F32)
    L = max(np.abs(np.diff(B[..., c], axis=1)).max() + np.abs(np.diff(B[..., c], axis=0)).max() for c in (0, 1))
    assert L == max(np.abs(np.diff(B, axis=0)).max(), np.abs(np.diff(B, axis=1)).max()) and 0.1 < L < 0.25
    bmax = np.abs(B).max()
    m = 3                                                       # |F| < 2: q + F stays inside, no clamp in the interior
    res = [np.abs(FR.invert(B, k + 1) - FR.invert(B, k))[m:-m, m:-m].max() for k in range(6)]
    print("L %.4f, max|B| %.3f, residuals %s, bound after 4 steps %.3e" % (L, bmax, res, L ** 4 * bmax))
    assert res[4] < L ** 4 * bmax
    for k in range(4):                                          # (until float32 rounding takes over)
        assert res[k + 1] <= L * res[k] + 1e-6, k


# ------------------------------------------------------------ GPU: the kernel against the restatement

SHAPES = [(64, 48), (37, 21), (130, 5), (1, 1), (1, 9), (9, 1)]


def _flows(w, h):
    rng = np.random.default_rng(w * 1000 + h)
    y, x = np.mgrid[0:h, 0:w]
    a = rng.uniform(-3, 3, 4)
    smooth = np.stack([a[0] * np.sin(x / 11.0 + a[1]) * np.cos(y / 8.0), a[2] * np.cos(x / 7.0) * np.sin(y / 13.0 + a[3])], -1)
    out = 200.0 * np.where(rng.random((h, w, 2)) < 0.5, -1.0, 1.0) + rng.uniform(-20, 20, (h, w, 2))
    return {"zeros": np.zeros((h, w, 2), F32), "smooth": smooth.astype(F32), "out": out.astype(F32)}


@pytest.mark.gpu
@pytest.mark.parametrize("w,h", SHAPES)
def test_gpu_kernel_equals_the_restatement_bit_for_bit(ctx, built, w, h):
    d_inv = ctx.alloc(w * h * 8)
    try:
        for name, B in _flows(w, h).items():
            assert np.isfinite(B).all()
            if name == "smooth":
                assert np.abs(B).max() <= 3
            if name == "out":                                    # every pixel points out of the frame, on either axis
                assert np.abs(B).min() > max(w, h)
            d_B = ctx.upload(B)
            for iters in (0, 1, 4, 16):
                ctx.flow_invert(d_inv, d_B, w, h, iters)
                got, want = ctx.download(d_inv, (h, w, 2)), FR.invert(B, iters)
                assert np.array_equal(_bits(got), _bits(want)), (name, iters, float(np.abs(got - want).max()))
            assert np.array_equal(_bits(ctx.download(d_B, (h, w, 2))), _bits(B))    # (the flow is only read)
            ctx.free(d_B)
    finally:
        ctx.free(d_inv)


@pytest.mark.gpu
def test_gpu_refused_calls_leave_the_context_working(ctx, built):
    w, h = 37, 21
    B = _flows(w, h)["smooth"]
    mark = np.full((h, w, 2), 7.0, F32)
    d_B, d_inv = ctx.upload(B), ctx.upload(mark)
    try:
        def refused(*a):
            with pytest.raises(built.NlkError, match="rc=-3"):      # NLK_EINVAL
                ctx.flow_invert(*a)
        for a in ((d_inv, d_B, 0, h, 4), (d_inv, d_B, w, 0, 4), (d_inv, d_B, -1, h, 4), (d_inv, d_B, w, h, -1),
                  (d_inv, d_B, w, h, 17), (None, d_B, w, h, 4), (d_inv, None, w, h, 4), (d_B, d_B, w, h, 4)):
            refused(*a)
        assert built.hip().nlk_dev_flow_invert(None, d_inv, d_B, w, h, 4) == -3
        assert np.array_equal(ctx.download(d_inv, (h, w, 2)), mark)     # (nothing was written)
        ctx.flow_invert(d_inv, d_B, w, h, 4)
        assert np.array_equal(_bits(ctx.download(d_inv, (h, w, 2))), _bits(FR.invert(B, 4)))
    finally:
        ctx.free(d_B)
        ctx.free(d_inv)
