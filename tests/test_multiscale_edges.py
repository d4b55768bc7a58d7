"""The multiscale whole-image DCT (csrc/k_ms.h, csrc/ms_host.h) and its tools (host/main_multiscale.c)
at the edges of the kernels: tile edges (128), K-chunk edges (16), w*ch crossing a tile where w does not,
1..4 channels, w == 1 / h == 1 (the staging predicates' other value), and the tools' float arithmetic.

The reference of every numeric test is float64: the matrices of the header comment of k_ms.h,
    forward  M[k][j] = cos(pi (j + 1/2) k / n) / n
    inverse  M[k][j] = j == 0 ? 1 : 2 cos(pi j (k + 1/2) / n)
built in numpy double, and R[k][l][c] = sum_{y,x} Mh[k][y] X[y][x][c] Mw[l][x]. It is pinned twice on the CPU:
against scipy.fft.dctn and against the oracle (test_reference_matrices_against_scipy_and_oracle).

u = 2^-24 is the unit roundoff of f32 throughout."""
import functools
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from test_cli import rpfm, run, server, sock_dir, wpfm  # noqa: E402,F401  (sock_dir: a fixture)
from test_multiscale import _img  # noqa: E402

U = 2.0 ** -24

# m of the yardstick 2(b) below: twice the largest rms(G - R) / e_ref measured on an MI355X over every shape and
# direction of RANDOM, rounded up, not below 2. The table of measured ratios: DESIGN.md §9, "Multiscale DCT:
# accuracy against an f32 evaluation".
M_YARDSTICK = 5

IMPULSE_SHAPES = [(1, 1, 1), (1, 9, 3), (9, 1, 3), (2, 2, 2), (16, 17, 4), (15, 16, 1), (43, 20, 3),
                  (127, 129, 1), (128, 128, 2), (129, 127, 3), (257, 130, 1)]
RANDOM = [(22, 13, 3), (16, 17, 4), (43, 20, 3), (129, 127, 2), (128, 128, 1), (333, 190, 3), (257, 130, 1),
          (640, 360, 3), (1920, 1080, 3)]


# ------------------------------------------------------------ the float64 reference

def basis(n, inverse):
    """M of k_ms.h in double; the argument of cos in the kernel's order of operations."""
    k = np.arange(n, dtype=np.float64)[:, None]
    j = np.arange(n, dtype=np.float64)[None, :]
    if not inverse:
        return np.cos(np.pi * (j + 0.5) * k / n) / n
    m = 2.0 * np.cos(np.pi * j * (k + 0.5) / n)
    m[:, 0] = 1.0
    return m


def apply2(mh, x, mw):
    """einsum('ky,yxc,lx->klc', mh, x, mw) as two matrix products in the operands' own precision."""
    h, w, ch = x.shape
    t = (mh @ x.reshape(h, w * ch)).reshape(h, w, ch)
    return np.ascontiguousarray(np.tensordot(t, mw, axes=([1], [1])).transpose(0, 2, 1))


def reference(x, inverse):
    h, w, _ = x.shape
    return apply2(basis(h, inverse), x.astype(np.float64), basis(w, inverse))


def bound_a(x, inverse, const=1.0):
    """2(a): |G - R| <= (h + w + 6) u (|Mh| |X| |Mw|^T), in float64: the forward-error bound of a dot product
    (gamma_n |A| |B|) for the two chained products, h and w terms long, plus the casts of the two basis entries,
    of the intermediate and of the result. Nothing that evaluates the two products in f32 can exceed it."""
    h, w, _ = x.shape
    b = apply2(np.abs(basis(h, inverse)), np.abs(x.astype(np.float64)), np.abs(basis(w, inverse)))
    return const * (h + w + 6) * U * b


def f32_evaluation(x, inverse):
    """The same two products in plain numpy float32, per channel: the yardstick of 2(b)."""
    h, w, ch = x.shape
    mh, mw = basis(h, inverse).astype(np.float32), basis(w, inverse).astype(np.float32)
    x = np.asarray(x, np.float32)       # (a contiguous plane per channel: numpy's BLAS path)
    return np.stack([mh @ np.ascontiguousarray(x[..., c]) @ mw.T for c in range(ch)], axis=-1)


def rms(a):
    return float(np.sqrt(np.mean(np.square(a, dtype=np.float64))))


@functools.lru_cache(maxsize=None)
def case(w, h, ch):
    """Inputs, float64 references, bounds and the f32 yardstick of one RANDOM shape, computed once and shared
    (read-only) by the tests: forward on the image, inverse on the f32 cast of the float64 forward result."""
    x = _img(w, h, ch, w)
    r_f = reference(x, False)
    f = r_f.astype(np.float32)
    out = {}
    for inverse, inp, r in ((False, x, r_f), (True, f, reference(f, True))):
        e32 = f32_evaluation(inp, inverse)
        d = dict(inp=inp, r=r, bound=bound_a(inp, inverse), e32=e32, e_ref=rms(e32 - r))
        for a in (d["inp"], d["r"], d["bound"], d["e32"]):
            a.flags.writeable = False
        out[inverse] = d
    return out


def gpu_dct(ctx, x, inverse):
    h, w, ch = x.shape
    d = ctx.upload(np.ascontiguousarray(x, np.float32))
    try:
        ctx.image_dct(d, w, h, ch, inverse)
        return ctx.download(d, (h, w, ch))
    finally:
        ctx.free(d)


# ------------------------------------------------------------ CPU: the reference is pinned, and inside its bound

def test_reference_matrices_against_scipy_and_oracle(O):
    """R from the float64 matrices = scipy's type-2 transform / (4 w h) and its type-3 transform (1e-12 of the
    largest coefficient: both are double), = the literal einsum, and = the oracle within f32 rounding."""
    import scipy.fft as sf
    for (w, h, ch) in [(1, 1, 1), (1, 9, 3), (9, 1, 3), (2, 2, 2), (16, 17, 4), (43, 20, 3), (129, 127, 2)]:
        x = _img(w, h, ch, w + h)
        x64 = x.astype(np.float64)
        for inverse in (False, True):
            r = reference(x, inverse)
            lit = np.einsum("ky,yxc,lx->klc", basis(h, inverse), x64, basis(w, inverse), optimize=True)
            s = sf.dctn(x64, type=3, axes=(0, 1)) if inverse else sf.dctn(x64, type=2, axes=(0, 1)) / (4 * w * h)
            scale = np.abs(s).max()
            assert np.abs(r - lit).max() <= 1e-12 * scale and np.abs(r - s).max() <= 1e-12 * scale, (w, h, ch, inverse)
            assert np.all(np.abs(O.ms_dct(x, inverse) - r) <= bound_a(x, inverse)), (w, h, ch, inverse)
        # inverse(forward(x)) = x: the two sets of matrices are each other's inverses
        assert np.abs(reference(reference(x, False), True) - x64).max() <= 1e-10


@pytest.mark.parametrize("w,h,ch", RANDOM)
def test_reference_evaluations_inside_the_bound(O, w, h, ch):
    """2(a) holds for the reference evaluations themselves at every shape of the GPU test: the numpy f32
    products and the oracle, which rounds to f32 between its passes. The oracle is a plain double loop (2e10
    scalar products per transform at 1080p); its lines are independent, so the channels and the two directions
    run side by side as one-channel images (the library call releases the interpreter lock)."""
    from concurrent.futures import ThreadPoolExecutor
    c = case(w, h, ch)
    for inverse in (False, True):
        d = c[inverse]
        assert d["e_ref"] > 0
        assert np.all(np.abs(d["e32"] - d["r"]) <= d["bound"]), (inverse, "numpy f32")
    jobs = [(inverse, k) for inverse in (False, True) for k in range(ch)]
    with ThreadPoolExecutor(len(jobs)) as pool:
        got = list(pool.map(lambda j: O.ms_dct(np.ascontiguousarray(c[j[0]]["inp"][..., j[1]]), j[0])[..., 0], jobs))
    for (inverse, k), g in zip(jobs, got):
        d = c[inverse]
        assert np.all(np.abs(g - d["r"][..., k]) <= d["bound"][..., k]), (inverse, k, "oracle")


# ------------------------------------------------------------ 1. impulses

def edge_set(n):
    return sorted({min(v, n - 1) for v in (0, 15, 16, 127, 128, n - 1)})


def impulses(w, h, ch):
    """Rows and columns of the edge sets paired in order (the shorter set repeating), then each row with the next
    column; the channels in turn; the first 8 distinct ones."""
    ys, xs = edge_set(h), edge_set(w)
    n = max(len(ys), len(xs), ch)
    pairs = [(ys[i % len(ys)], xs[(i + s) % len(xs)]) for s in (0, 1) for i in range(n)]
    return list(dict.fromkeys((y, x, i % ch) for i, (y, x) in enumerate(pairs)))[:8]


def test_impulse_positions_cover_the_edges():
    for (w, h, ch) in IMPULSE_SHAPES:
        p = impulses(w, h, ch)
        every_pair = {(y, x) for y, x, _ in p} == {(y, x) for y in edge_set(h) for x in edge_set(w)}
        assert len(p) <= 10 and (len(p) >= 6 or every_pair)
        assert {c for _, _, c in p} == set(range(ch))
        assert [sorted({q[i] for q in p}) for i in (0, 1)] == [edge_set(h), edge_set(w)]


@pytest.mark.gpu
@pytest.mark.parametrize("w,h,ch", IMPULSE_SHAPES)
def test_gpu_impulse_is_the_outer_product_of_two_basis_columns(ctx, w, h, ch):
    """An image that is 1.0 at (y0, x0, c0) and zero elsewhere transforms to Mh[k, y0] * Mw[l, x0] in channel c0
    and to exactly 0.0 in the others. Derived tolerance: one term of each sum is non-zero, so the first product
    returns the f32 basis entry unchanged and the roundings are the casts of the two basis entries to f32
    (u each, plus at most one more f32 ulp = 2 u where the device's double cos differs from numpy's in the
    last place) and one f32 product (u): |G - R| <= 6 u |R| + 1e-12 per element, the absolute term for the
    zeros of the cosine, which in double are 1e-16 here and there."""
    for inverse in (False, True):
        mh, mw = basis(h, inverse), basis(w, inverse)
        for (y0, x0, c0) in impulses(w, h, ch):
            x = np.zeros((h, w, ch), np.float32)
            x[y0, x0, c0] = 1.0
            g = gpu_dct(ctx, x, inverse)
            r = np.outer(mh[:, y0], mw[:, x0])
            err = np.abs(g[..., c0] - r)
            tol = 6 * U * np.abs(r) + 1e-12
            worst = np.unravel_index(np.argmax(err - tol), err.shape)
            assert np.all(err <= tol), (inverse, y0, x0, c0, worst, g[..., c0][worst], r[worst])
            others = [c for c in range(ch) if c != c0]
            assert np.all(g[..., others] == 0.0), (inverse, y0, x0, c0)


# ------------------------------------------------------------ 2. random images

@pytest.mark.gpu
@pytest.mark.parametrize("w,h,ch", RANDOM)
def test_gpu_random_image_bound_and_yardstick(ctx, w, h, ch):
    """Forward on pattern + noise, inverse on the f32 cast of the float64 forward coefficients.
    (a) per coefficient, the derived bound (bound_a); it is loose by about sqrt(K): the floor.
    (b) rms(G - R) <= m * e_ref, e_ref the rms error of the numpy f32 evaluation of the same products, whose
        summation order differs from the kernel's (an fma chain over k in MFMA groups of 4 inside chunks of
        16, against BLAS blocking). m = M_YARDSTICK = twice the largest ratio measured over these shapes and
        directions, rounded up, not below 2; the measured table is in DESIGN.md §9."""
    c = case(w, h, ch)
    seen = {}
    for inverse in (False, True):       # (both directions are measured and printed before either is asserted)
        d = c[inverse]
        g = gpu_dct(ctx, d["inp"], inverse)
        err = np.abs(g - d["r"])
        seen[inverse] = (rms(g - d["r"]) / d["e_ref"], float((err / d["bound"]).max()))
        print(f"random {w}x{h}x{ch} inv={int(inverse)}: rms(G-R) {rms(g - d['r']):.3e} e_ref {d['e_ref']:.3e} "
              f"ratio {seen[inverse][0]:.3f} max |G-R|/bound {seen[inverse][1]:.4f}")
    for inverse, (ratio, worst) in seen.items():
        assert worst <= 1.0, (inverse, worst)
        assert ratio <= M_YARDSTICK, (inverse, ratio)


# ------------------------------------------------------------ 3. properties

@pytest.mark.gpu
def test_gpu_dct_run_to_run_bits(ctx):
    x = _img(333, 190, 3, 333)
    for inverse in (False, True):
        assert np.array_equal(gpu_dct(ctx, x, inverse).view(np.uint32), gpu_dct(ctx, x, inverse).view(np.uint32))


@pytest.mark.gpu
def test_gpu_dct_scratch_reuse(ctx, built):
    """c->ms is re-reserved and the basis rebuilt per call: a smaller transform and a filter call in between
    leave nothing behind. 333x190x3, 22x13x3, a filter_frame on a small frame, 333x190x3 again on one context;
    the 22x13 result against a fresh context's."""
    big, small = _img(333, 190, 3, 333), _img(22, 13, 3, 22)
    for inverse in (False, True):
        first = gpu_dct(ctx, big, inverse)
        mid = gpu_dct(ctx, small, inverse)
        frame = _img(48, 40, 1, 3)
        d_in, d_out = ctx.upload(frame), ctx.alloc(frame.nbytes)
        ctx.filter_frame(d_out, d_in, None, None, 48, 40, 1, 20.0, built.default_params(20.0, built.FLT1))
        ctx.sync()
        ctx.free(d_in)
        ctx.free(d_out)
        third = gpu_dct(ctx, big, inverse)
        assert np.array_equal(first.view(np.uint32), third.view(np.uint32)), inverse
        fresh = built.Context(0)
        try:
            alone = gpu_dct(fresh, small, inverse)
        finally:
            fresh.close()
        assert np.array_equal(mid.view(np.uint32), alone.view(np.uint32)), inverse


@pytest.mark.gpu
@pytest.mark.parametrize("w,h", [(43, 20), (129, 127), (333, 190)])
def test_gpu_dct_channels_are_independent(ctx, w, h):
    """An HWC image of 3 channels gives, per channel, the bits of that channel transformed alone: every output
    element is the same ordered sum over k whatever tile column it lands in (w*ch = 129 at 43x20: the channels
    straddle a tile edge of the first product that the single channel does not have)."""
    x = _img(w, h, 3, w)
    for inverse in (False, True):
        g = gpu_dct(ctx, x, inverse)
        for c in range(3):
            one = gpu_dct(ctx, x[..., c:c + 1], inverse)
            assert np.array_equal(g[..., c].view(np.uint32), one[..., 0].view(np.uint32)), (inverse, c)


@pytest.mark.gpu
@pytest.mark.parametrize("w,h", [(129, 127), (43, 20)])
def test_gpu_dct_of_the_transpose(ctx, w, h):
    """dct(X^T) = dct(X)^T for one channel. The two sides sum over y and x in the other order (and through the
    other product: contiguous N against strided N), so they are not bit-equal; each is within 2(a) of R, their
    difference within twice that."""
    x = _img(w, h, 1, w)
    xt = np.ascontiguousarray(x.transpose(1, 0, 2))
    for inverse in (False, True):
        g, gt = gpu_dct(ctx, x, inverse), gpu_dct(ctx, xt, inverse)
        b = bound_a(x, inverse, const=2.0)
        d = np.abs(g[..., 0].astype(np.float64) - gt[..., 0].T)
        print(f"transpose {w}x{h} inv={int(inverse)}: max diff/bound {(d / b[..., 0]).max():.4f}")
        assert np.all(d <= b[..., 0]), inverse


# 6 u * 100 allows for the casts of the two basis entries and one product, that is for sums that are exact. They
# are where w and h are powers of two: 1/n, 100/n and every partial sum k * 100/n are f32 numbers. At any other
# size each sum adds the same addend n times, which rounds the same way at every step inside a binade: the error
# of a correct f32 evaluation grows like n u / 4 (test_constant_image_dc_of_a_sequential_f32_sum shows it for the
# sizes below). So DC is held to 6 u * 100 at the power-of-two shapes and to 2(a) at the others.
CONSTANT_EXACT = [(128, 128, 2), (256, 16, 3), (2, 2, 2)]
CONSTANT_OTHER = [(43, 20, 3), (129, 127, 2)]


def _sequential_f32_dc(w, h):
    """DC of a constant 100 image as the kernel's sums run: an f32 accumulator over k, products exact (fma)."""
    def chain(n, v):
        m = np.float32(1.0 / n)
        s = np.float32(0)
        for _ in range(n):
            s = np.float32(np.float64(s) + np.float64(m) * np.float64(v))
        return s
    return float(chain(w, chain(h, np.float32(100.0))))


def test_constant_image_dc_of_a_sequential_f32_sum():
    """Why CONSTANT_OTHER is not held to 6 u * 100: a correct sequential f32 sum already misses it there, and is
    exact at the powers of two."""
    for (w, h, _) in CONSTANT_EXACT:
        assert _sequential_f32_dc(w, h) == 100.0
    assert any(abs(_sequential_f32_dc(w, h) - 100.0) > 6 * U * 100 for (w, h, _) in CONSTANT_OTHER)


@pytest.mark.gpu
@pytest.mark.parametrize("w,h,ch", CONSTANT_EXACT + CONSTANT_OTHER)
def test_gpu_dct_of_a_constant_image(ctx, w, h, ch):
    """100.0 everywhere: DC = 100 within 6 u * 100 (power-of-two sizes, see above; within 2(a) at the others),
    every other coefficient within 2(a) of the float64 result (which is 0 up to double rounding)."""
    x = np.full((h, w, ch), 100.0, np.float32)
    g = gpu_dct(ctx, x, False)
    r, b = reference(x, False), bound_a(x, False)
    print(f"constant {w}x{h}x{ch}: |DC - 100| / (u * 100) = {np.abs(g[0, 0] - 100.0).max() / (U * 100):.2f}")
    if (w, h, ch) in CONSTANT_EXACT:
        assert np.all(np.abs(g[0, 0].astype(np.float64) - 100.0) <= 6 * U * 100)
    assert np.all(np.abs(g - r) <= b)


# ------------------------------------------------------------ 4. nlk_dev_copy_block, argument checks

@pytest.mark.gpu
@pytest.mark.parametrize("dw,dh,sw,sh,ch,bw,bh", [(100, 40, 60, 30, 3, 60, 30), (86, 9, 86, 9, 3, 86, 9),
                                                  (85, 5, 90, 5, 3, 85, 5), (64, 64, 64, 64, 4, 64, 1),
                                                  (300, 7, 257, 7, 1, 257, 7), (5, 5, 3, 3, 2, 1, 1)])
def test_gpu_copy_block(ctx, dw, dh, sw, sh, ch, bw, bh):
    """The top-left bw x bh block of the source lands in the destination bit for bit; every other element of
    the destination (distinct finite sentinels) stays as it was."""
    src = (np.arange(sh * sw * ch, dtype=np.float32) + 0.25).reshape(sh, sw, ch)
    dst = -(np.arange(dh * dw * ch, dtype=np.float32) + 1.5).reshape(dh, dw, ch)
    want = dst.copy()
    want[:bh, :bw] = src[:bh, :bw]
    d_src, d_dst = ctx.upload(src), ctx.upload(dst)
    try:
        ctx.copy_block(d_dst, dw, d_src, sw, ch, bw, bh)
        got = ctx.download(d_dst, dst.shape)
        assert np.array_equal(ctx.download(d_src, src.shape), src)
    finally:
        ctx.free(d_src)
        ctx.free(d_dst)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


@pytest.mark.gpu
def test_gpu_copy_block_and_image_dct_arguments(ctx, built):
    src = np.arange(6 * 5 * 2, dtype=np.float32).reshape(5, 6, 2)
    dst = -np.arange(8 * 5 * 2, dtype=np.float32).reshape(5, 8, 2) - 1
    d_src, d_dst = ctx.upload(src), ctx.upload(dst)
    try:
        ctx.copy_block(d_dst, 8, d_src, 6, 2, 0, 3)          # an empty block is fine and writes nothing
        ctx.copy_block(d_dst, 8, d_src, 6, 2, 3, 0)
        assert np.array_equal(ctx.download(d_dst, dst.shape), dst)
        for args in ((d_dst, 8, d_src, 6, 2, 9, 1),          # bw > dw
                     (d_dst, 8, d_src, 6, 2, 7, 1),          # bw > sw
                     (d_dst, 8, d_src, 6, 0, 3, 3),          # ch < 1
                     (None, 8, d_src, 6, 2, 3, 3), (d_dst, 8, None, 6, 2, 3, 3)):
            with pytest.raises(built.NlkError):
                ctx.copy_block(*args)
        for args in ((d_dst, 0, 5, 2), (d_dst, 8, 0, 2), (d_dst, 8, 5, 0), (d_dst, -1, 5, 2), (None, 8, 5, 2)):
            with pytest.raises(built.NlkError):
                ctx.image_dct(*args, False)
        assert np.array_equal(ctx.download(d_dst, dst.shape), dst)
        assert np.array_equal(ctx.download(d_src, src.shape), src)
    finally:
        ctx.free(d_src)
        ctx.free(d_dst)


# ------------------------------------------------------------ 5. the tools at the edges of their arithmetic

def _ok(r):
    assert r.returncode == 0, r.stderr
    return r


def _levels(tmp, prefix, n, suffix=".pfm"):
    return [rpfm(tmp / f"{prefix}{i}{suffix}") for i in range(n)]


def _bytes(p):
    with open(p, "rb") as f:
        return f.read()


@pytest.mark.gpu
def test_tools_decompose_ratios(built, O, tmp_path):
    """-r 1.5 and -r 3: the level sizes follow from float division and truncation (decompose.cpp: w /= ratio);
    the option before the positional arguments is the option after them."""
    a = _img(121, 91, 3, 7)
    wpfm(tmp_path / "a.pfm", a)
    _ok(run("decompose", tmp_path / "a.pfm", str(tmp_path / "p"), 3, ".pfm", "-r", 1.5))
    lv, want = _levels(tmp_path, "p", 3), O.ms_decompose(a, 3, 1.5)
    assert [x.shape for x in lv] == [(91, 121, 3), (60, 80, 3), (40, 53, 3)]
    for g, wv in zip(lv, want):
        assert g.shape == wv.shape and np.abs(g - wv).max() < 2e-3
    _ok(run("decompose", "-r", 1.5, tmp_path / "a.pfm", str(tmp_path / "q"), 3, ".pfm"))
    _ok(run("decompose", "-r", 2, tmp_path / "a.pfm", str(tmp_path / "s"), 3, ".pfm"))
    _ok(run("decompose", tmp_path / "a.pfm", str(tmp_path / "t"), 3, ".pfm", "-r", 2))
    for i in range(3):
        assert _bytes(tmp_path / f"q{i}.pfm") == _bytes(tmp_path / f"p{i}.pfm")
        assert _bytes(tmp_path / f"s{i}.pfm") == _bytes(tmp_path / f"t{i}.pfm")
    assert [x.shape for x in _levels(tmp_path, "s", 3)] == [(91, 121, 3), (45, 60, 3), (22, 30, 3)]

    b = _img(100, 75, 1, 8)
    wpfm(tmp_path / "b.pfm", b)
    _ok(run("decompose", tmp_path / "b.pfm", str(tmp_path / "g"), 3, ".pfm", "-r", 3))
    lv, want = _levels(tmp_path, "g", 3), O.ms_decompose(b, 3, 3.0)
    assert [x.shape for x in lv] == [(75, 100, 1), (25, 33, 1), (8, 11, 1)]
    for g, wv in zip(lv, want):
        assert g.shape == wv.shape and np.abs(g - wv).max() < 2e-3


@pytest.mark.gpu
def test_tools_recompose_factors_and_round_trip(built, O, tmp_path):
    """-c 1.0 (the whole coarse spectrum), -c 0.5, and recompose(decompose(x)) = x at ratios 2 and 1.5: the
    coarse levels' spectra are the fine one's own low frequencies. The coarse levels are changed before -c 1.0 /
    0.5 so that the factor shows in the result."""
    a = _img(121, 91, 3, 9)
    wpfm(tmp_path / "a.pfm", a)
    for tag, ratio in (("r2_", 2), ("r15_", 1.5)):
        _ok(run("decompose", tmp_path / "a.pfm", str(tmp_path / tag), 3, ".pfm", "-r", ratio))
        _ok(run("recompose", str(tmp_path / tag), 3, ".pfm", tmp_path / (tag + "back.pfm")))
        assert np.abs(rpfm(tmp_path / (tag + "back.pfm")) - a).max() < 3e-3, ratio
    lv = _levels(tmp_path, "r2_", 3)
    rng = np.random.default_rng(4)
    lv[1] = lv[1] + rng.normal(0, 5, lv[1].shape).astype(np.float32)
    lv[2] = lv[2] + rng.normal(0, 5, lv[2].shape).astype(np.float32)
    for i in range(3):
        wpfm(tmp_path / f"m{i}.pfm", lv[i])
    outs = {}
    for f in (1.0, 0.5):
        _ok(run("recompose", str(tmp_path / "m"), 3, ".pfm", tmp_path / f"out{f}.pfm", "-c", f))
        outs[f] = rpfm(tmp_path / f"out{f}.pfm")
        assert np.abs(outs[f] - O.ms_recompose(lv, f)).max() < 3e-3, f
    assert np.abs(outs[1.0] - outs[0.5]).max() > 1.0          # (the factor is not ignored)


@pytest.mark.gpu
def test_tools_recompose_clamps_the_block(built, O, tmp_path):
    """-c 1.5 where 1.5 times the coarse size exceeds the fine image: the block is clipped to the coefficients
    that both images have (low_frequencies in host/main_multiscale.c; the reference reads and writes out of
    bounds). A coarse level of 80x60 under 100x75 (120x90 -> 80x60: the whole coarse spectrum, as -c 1.0), a
    coarse image of the fine one's size (150x113 -> 100x75: the result is the coarse image) and one that is
    narrower and taller, 90x80 (135x120 -> 90x75). Before the clip to the coarse size the first of these ended
    with "nlk_dev_copy_block: bad argument". Images whose channel counts differ are refused."""
    a = _img(100, 75, 3, 10)
    wpfm(tmp_path / "a.pfm", a)
    _ok(run("decompose", tmp_path / "a.pfm", str(tmp_path / "k"), 2, ".pfm", "-r", 1.25))
    lv = _levels(tmp_path, "k", 2)
    assert [x.shape for x in lv] == [(75, 100, 3), (60, 80, 3)]
    lv[1] = lv[1] + np.random.default_rng(5).normal(0, 5, lv[1].shape).astype(np.float32)
    wpfm(tmp_path / "k1.pfm", lv[1])
    _ok(run("recompose", str(tmp_path / "k"), 2, ".pfm", tmp_path / "out.pfm", "-c", 1.5))
    out = rpfm(tmp_path / "out.pfm")
    assert out.shape == a.shape and np.abs(out - O.ms_recompose(lv, 1.5)).max() < 3e-3
    _ok(run("recompose", str(tmp_path / "k"), 2, ".pfm", tmp_path / "out1.pfm", "-c", 1.0))
    assert _bytes(tmp_path / "out1.pfm") == _bytes(tmp_path / "out.pfm")
    _ok(run("merge_coarse", tmp_path / "k0.pfm", tmp_path / "k1.pfm", tmp_path / "mc.pfm", "-c", 1.5))
    assert _bytes(tmp_path / "mc.pfm") == _bytes(tmp_path / "out.pfm")
    for name, (cw, chh) in (("same", (100, 75)), ("tall", (90, 80))):
        c = _img(cw, chh, 3, 20 + cw)
        wpfm(tmp_path / f"{name}.pfm", c)
        _ok(run("merge_coarse", tmp_path / "a.pfm", tmp_path / f"{name}.pfm", tmp_path / f"{name}_mc.pfm", "-c", 1.5))
        got = rpfm(tmp_path / f"{name}_mc.pfm")
        assert got.shape == a.shape and np.abs(got - O.ms_recompose([a, c], 1.5)).max() < 3e-3, name
        if name == "same":
            assert np.abs(got - c).max() < 3e-3
    wpfm(tmp_path / "gray.pfm", a[..., 0])
    r = run("merge_coarse", tmp_path / "gray.pfm", tmp_path / "k1.pfm", tmp_path / "no.pfm")
    assert r.returncode == 1 and "channels" in r.stderr and not os.path.exists(tmp_path / "no.pfm")


@pytest.mark.gpu
def test_tools_merge_coarse_of_an_odd_pair(built, O, tmp_path):
    """merge_coarse where the coarse image is not half the fine one: 121x91 and 53x40."""
    a = _img(121, 91, 3, 11)
    coarse = _img(53, 40, 3, 12)
    wpfm(tmp_path / "a.pfm", a)
    wpfm(tmp_path / "c.pfm", coarse)
    _ok(run("merge_coarse", tmp_path / "a.pfm", tmp_path / "c.pfm", tmp_path / "m8.pfm", "-c", 0.8))
    _ok(run("merge_coarse", tmp_path / "a.pfm", tmp_path / "c.pfm", tmp_path / "md.pfm"))
    want = O.ms_recompose([a, coarse], 0.8)
    assert np.abs(rpfm(tmp_path / "m8.pfm") - want).max() < 3e-3
    assert _bytes(tmp_path / "m8.pfm") == _bytes(tmp_path / "md.pfm")
    assert np.abs(want - a).max() > 1.0                        # (the coarse image is not ignored)


@pytest.mark.gpu
def test_tools_decompose_level_that_becomes_empty(built, O, tmp_path):
    """9x5 in 5 levels of ratio 2: 9x5, 4x2, 2x1, then 1x0. decompose says so and exits with 1; the earlier
    levels are written, the empty one and what would follow are not."""
    a = _img(9, 5, 1, 13)
    wpfm(tmp_path / "a.pfm", a)
    r = run("decompose", tmp_path / "a.pfm", str(tmp_path / "e"), 5, ".pfm")
    assert r.returncode == 1 and "level 3 is empty" in r.stderr, (r.returncode, r.stderr)
    want = O.ms_decompose(a, 3, 2.0)
    assert [x.shape for x in want] == [(5, 9, 1), (2, 4, 1), (1, 2, 1)]
    for g, wv in zip(_levels(tmp_path, "e", 3), want):
        assert g.shape == wv.shape and np.abs(g - wv).max() < 2e-3
    assert not os.path.exists(tmp_path / "e3.pfm") and not os.path.exists(tmp_path / "e4.pfm")


@pytest.mark.gpu
def test_tools_behind_the_server_write_the_same_bytes(built, tmp_path, sock_dir):  # noqa: F811
    """decompose -> recompose -> merge_coarse with NLK_SERVER set against the direct run: identical files."""
    a = _img(121, 91, 3, 14)
    wpfm(tmp_path / "a.pfm", a)

    def steps(tag, env):
        q = lambda f: str(tmp_path / (tag + f))  # noqa: E731
        for args in (("decompose", tmp_path / "a.pfm", q("l"), 3, ".pfm", "-r", 1.5),
                     ("recompose", q("l"), 3, ".pfm", q("rec.pfm"), "-c", 0.5),
                     ("merge_coarse", tmp_path / "a.pfm", q("l2.pfm"), q("mc.pfm"), "-c", 0.8)):
            r = run(*args, env=env)
            assert r.returncode == 0, (args, r.stderr)

    steps("d_", dict(os.environ))
    with server(sock_dir) as env:
        steps("s_", env)
    for f in ("l0.pfm", "l1.pfm", "l2.pfm", "rec.pfm", "mc.pfm"):
        assert _bytes(tmp_path / ("d_" + f)) == _bytes(tmp_path / ("s_" + f)), f
