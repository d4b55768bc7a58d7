"""The block-matching optical flow (nlk_dev_bm_flow, csrc/k_bmflow.h) and its way through the sequence tools
(--of bm, SequenceFilter(of="bm"), bin/bmflow). The algorithm is stated once, in numpy, by tests/bmflow_ref.py; the
kernels give its bits. The quality evidence is synthetic: the frames of bwd-nlkalman_amd/synth.py."""
import importlib
import os
import subprocess

import numpy as np
import pytest

import bmflow_ref as BR
import cases
import yuv_ref as R
from test_cli import BIN, rpfm, run, wpfm

W, H, CH, SIGMA, NF = 96, 64, 3, 20.0, 3
TOOLS = ("nlkalman-seq", "nlkalman-seq-gt", "nlkalman-lsmo-seq", "nlkalman-y4m")


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ------------------------------------------------------------ CPU: the restatement

def _texture(x, y):
    return (128 + 50 * np.sin(0.31 * x + 0.17 * y) + 40 * np.cos(0.23 * y - 0.11 * x)
            + 25 * np.sin(0.05 * x * y / 8 + 1)).astype(np.float32)


@pytest.mark.parametrize("sx,sy", [(3, -2), (0, 0)])
def test_restatement_finds_a_shift(sx, sy):
    """I0 = g(x, y), I1 = g(x - sx, y - sy), g smooth: I1(q + (sx, sy)) = I0(q)"""
    w, h = 61, 45
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    F = BR.flow(_texture(x, y), _texture(x - sx, y - sy), fscale=0)
    epe = float(np.hypot(F[..., 0] - sx, F[..., 1] - sy)[8:-8, 8:-8].mean())
    print("shift (%d, %d): interior mean endpoint error %.4f px" % (sx, sy, epe))
    assert epe <= 0.05


def test_restatement_small_images():
    rng = np.random.default_rng(5)
    a, b = (rng.uniform(0, 255, (5, 7)).astype(np.float32) for _ in range(2))
    F = BR.flow(a, b)
    assert F.shape == (5, 7, 2) and not F.any()
    a, b = (rng.uniform(0, 255, (8, 8)).astype(np.float32) for _ in range(2))
    F = BR.flow(a, b)
    assert F.shape == (8, 8, 2) and len(np.unique(F.reshape(-1, 2), axis=0)) == 1
    assert len(BR.pyramid(np.zeros((64, 96), np.float32))) == 3 and len(BR.pyramid(np.zeros((45, 61), np.float32))) == 2
    assert list(BR.origins(61)) == list(range(0, 53, 4)) + [53] and list(BR.origins(8)) == [0]


# ------------------------------------------------------------ CPU: what the flow is for

def _chain_psnr(O, synth, sigma, flow_of):
    return BR.chain_psnr(O, synth, lambda t: synth.clean_frame(W, H, CH, t), sigma, flow_of)


@pytest.mark.parametrize("sigma", [20.0, 40.0])
def test_quality_on_the_cpu_oracle(O, synth, sigma):
    """The consumer tolerates the block matcher's error: it keeps at least half of TV-L1's gain over no flow at all."""
    zero = _chain_psnr(O, synth, sigma, lambda a, b: np.zeros(a.shape + (2,), np.float32))
    tvl1 = _chain_psnr(O, synth, sigma, lambda a, b: np.stack(O.tvl1_flow(a, b, lam=0.25, fscale=1), -1))
    bm = _chain_psnr(O, synth, sigma, lambda a, b: BR.flow(a, b, fscale=1, radius=2))
    print("sigma %g: mean flt2 PSNR of frames 1..3: zero flow %.3f, TV-L1 %.3f, block matching %.3f" % (sigma, zero, tvl1, bm))
    assert bm - zero >= 0.5 * (tvl1 - zero)


# ------------------------------------------------------------ CPU: usage

def _tool(tool, *args, data=b"", **kw):
    return subprocess.run([os.path.join(BIN, tool), *map(str, args)], input=data, capture_output=True, **kw)


def test_usage_errors(built, tmp_path):
    if not all(os.path.exists(os.path.join(BIN, t)) for t in TOOLS + ("bmflow",)):
        built.build()
    for tool in TOOLS:
        rest = (20,) if tool == "nlkalman-y4m" else (tmp_path / "%03d.tif", 1, 3, 20, tmp_path / "out")
        r = _tool(tool, "--of", "bogus", *rest, data=R.y4m_bytes(4, 2, None, []))
        assert r.returncode == 1 and r.stdout == b"", tool
        assert r.stderr == b"%s: --of bogus: want tvl1 or bm\n" % tool.encode(), (tool, r.stderr)
    # the old usage lines are still there
    for tool, old in (("nlkalman-seq", "SEQ FFR LFR SIG OUT [STP [FPM [SPM [OPM]]]]"),
                      ("nlkalman-seq-gt", "[--ssim] SEQ FFR LFR SIG OUT [FPM [SPM [OPM]]]"),
                      ("nlkalman-lsmo-seq", "[--flow tvl1|inv] SEQ FFR LFR SIG OUT [FPM [SPM [OPM]]]")):
        for args in ((), ("--of", "bm")):
            r = run(tool, *args)
            assert r.returncode == 1 and r.stdout == "" and r.stderr.startswith("usage: ") and old in r.stderr, (tool, args)
            assert "--of tvl1|bm" in r.stderr
    r = run("nlkalman-lsmo-seq", "--of", "bm", "--flow", "bogus", tmp_path / "%03d.tif", 1, 3, 20, tmp_path / "out")
    assert r.returncode == 1 and "want tvl1 or inv" in r.stderr
    r = _tool("nlkalman-y4m")
    assert r.returncode == 1 and b"[options] SIG [IN [OUT]]" in r.stderr and b"--of tvl1|bm" in r.stderr
    r = run("bmflow")
    assert r.returncode == 1 and r.stdout == "" and "I0 I1 OUT [FSCALE [RADIUS]]" in r.stderr
    r = run("bmflow", "a", "b", tmp_path / "o.flo", 1, 4)
    assert r.returncode == 1 and r.stderr.startswith("bmflow: ") and "RADIUS" in r.stderr


def test_of_parameter_is_checked(built):
    seq = importlib.import_module("bwd-nlkalman_amd.sequence")
    with pytest.raises(ValueError):
        seq.SequenceFilter(None, W, H, CH, SIGMA, of="bogus")


# ------------------------------------------------------------ GPU: the kernels give the restatement's bits

def _pair(synth, w, h):
    n0, n1, _ = synth.noisy_pair(w, h, 1, SIGMA, seed=7)
    return np.ascontiguousarray(n0[..., 0]), np.ascontiguousarray(n1[..., 0])


def _dev_flow(ctx, g0, g1, **kw):
    h, w = g0.shape
    d0, d1, df = ctx.upload(g0), ctx.upload(g1), ctx.alloc(w * h * 8)
    ctx.bm_flow(df, d0, d1, w, h, **kw)
    out = ctx.download(df, (h, w, 2))
    for d in (d0, d1, df):
        ctx.free(d)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("w,h,fscale,radius", [
    (96, 64, 0, 2), (96, 64, 1, 2),   # three levels
    (96, 64, 5, 2),                   # fscale beyond the pyramid: the coarsest level alone, upsampled twice
    (61, 45, 1, 1), (61, 45, 1, 2), (61, 45, 1, 3), (61, 45, 0, 3),   # odd halving, the last origin off the stride; every radius
    (33, 17, 1, 2),                   # one level, the block rows pressed against the border
    (16, 8, 1, 2), (8, 8, 1, 2),      # one block row, one block
    (7, 5, 1, 2),                     # no room for a block: zeros
])
def test_kernels_equal_the_restatement(ctx, synth, w, h, fscale, radius):
    g0, g1 = _pair(synth, w, h)
    want = BR.flow(g0, g1, fscale=fscale, radius=radius)
    got = _dev_flow(ctx, g0, g1, fscale=fscale, radius=radius)
    bad = np.argwhere(_bits(got) != _bits(want))
    print("%d x %d fscale %d radius %d: %d of %d values differ%s" % (
        w, h, fscale, radius, len(bad), want.size, "" if not len(bad) else ", first at %s: %r != %r" % (
            bad[0], got[tuple(bad[0])], want[tuple(bad[0])])))
    assert not len(bad)
    again = _dev_flow(ctx, g0, g1, fscale=fscale, radius=radius)
    assert np.array_equal(_bits(again), _bits(got))
    if min(w, h) >= 8:
        assert got.any()


def _quadrants(w, h, sx=0, sy=0):
    """two levels of gray in four quadrants, the cross at (w // 2 + sx, h // 2 + sy)"""
    y, x = np.mgrid[0:h, 0:w]
    return (64.0 + 128.0 * ((x >= w // 2 + sx) ^ (y >= h // 2 + sy))).astype(np.float32)


@pytest.mark.gpu
@pytest.mark.parametrize("radius", [1, 2, 3])
def test_kernels_on_equal_costs(ctx, radius):
    """Noise-free pairs, where the noisy ones above never go: candidates of equal cost, which the wavefront reduction
    must settle by raster order (at radius 3 also between its two rounds of candidates), and flat or concave parabolas
    (den <= 0: offset 0)."""
    flat = np.full((17, 33), 128.0, np.float32)          # one level: every cost is 0, every den is 0
    want = BR.flow(flat, flat, fscale=0, radius=radius)
    assert (want == np.float32(-radius)).all()           # the first candidate of the inner square, no sub-pel part
    got = _dev_flow(ctx, flat, flat, fscale=0, radius=radius)
    assert np.array_equal(_bits(got), _bits(want)), "flat"
    for fscale in (0, 1):                                # two levels: blocks inside a quadrant tie, blocks on the cross do not
        g0, g1 = _quadrants(61, 45), _quadrants(61, 45, 1, -1)
        want = BR.flow(g0, g1, fscale=fscale, radius=radius)
        got = _dev_flow(ctx, g0, g1, fscale=fscale, radius=radius)
        bad = np.argwhere(_bits(got) != _bits(want))
        print("quadrants, fscale %d radius %d: %d of %d values differ, %d distinct vectors" % (
            fscale, radius, len(bad), want.size, len(np.unique(want.reshape(-1, 2), axis=0))))
        assert not len(bad), (fscale, bad[0])
        assert len(np.unique(want.reshape(-1, 2), axis=0)) > 1


@pytest.mark.gpu
def test_refused_parameters(ctx, built, synth):
    g0, g1 = _pair(synth, 16, 8)
    for kw in (dict(radius=0), dict(radius=4), dict(fscale=-1)):
        with pytest.raises(built.NlkError):
            _dev_flow(ctx, g0, g1, **kw)
    assert np.array_equal(_dev_flow(ctx, g0, g1), BR.flow(g0, g1))    # the context keeps working


# ------------------------------------------------------------ GPU: the driver against the oracle

def _frames(synth, w=W, h=H, nf=NF):
    return [synth.awgn(synth.clean_frame(w, h, CH, t), SIGMA, 100 + t) for t in range(nf)]   # tests/test_sequence.py's


def _dev_gray(ctx, rgb, opp=False):
    """the gray image the driver's flow sees: of an RGB frame, or of an opponent-space one through opp2rgb"""
    h, w, ch = rgb.shape
    d, dg = ctx.upload(np.ascontiguousarray(rgb, np.float32)), ctx.alloc(w * h * 4)
    if opp:
        ctx.opp2rgb(d, w, h, ch)
    ctx.gray(dg, d, w, h, ch)
    g = ctx.download(dg, (h, w))
    ctx.free(d)
    ctx.free(dg)
    return g


@pytest.mark.gpu
@pytest.mark.parametrize("lag1", [None, "inv", "tvl1"])
def test_driver_equals_oracle_recursion(ctx, built, O, synth, lag1):
    """Stage by stage, as tests/test_lag1.py::test_driver_equals_oracle_recursion: the oracle fed with the driver's
    previous outputs and the restatement's flow of the driver's own gray images. Flow and mask exactly, pixels within
    the project's tolerance."""
    import flowinv_ref as FR
    seq = importlib.import_module("bwd-nlkalman_amd.sequence")
    frames = _frames(synth)
    fscale, th = 1, 0.75
    p1, p2, ps = (O.default_params(SIGMA, m) for m in (O.FLT1, O.FLT2, O.SMO1))
    sf = seq.SequenceFilter(ctx, W, H, CH, SIGMA, of_fscale=fscale, occ_th=th, keep_history=False, lag1=lag1, of="bm")
    got1, got2 = [], []
    for t, rgb in enumerate(frames):
        d = ctx.upload(rgb)
        sf.push(d)
        ctx.free(d)
        got1.append(ctx.download(sf.flt1, (H, W, CH)))
        got2.append(ctx.download(sf.flt2, (H, W, CH)))
        nz = O.rgb2opp(rgb)
        if t == 0:
            w1 = w2 = None
        else:
            B = BR.flow(_dev_gray(ctx, rgb), _dev_gray(ctx, got2[t - 1], opp=True), fscale=fscale)
            assert np.array_equal(_bits(ctx.download(sf.d_flow, (H, W, 2))), _bits(B)), t
            occ = O.tvl1_occlusion_mask(B, th)
            assert np.array_equal(ctx.download(sf.d_occ, (H, W)), occ), t
            w1, w2 = O.warp_bicubic(got1[t - 1], B, occ), O.warp_bicubic(got2[t - 1], B, occ)
        for name, got, (r, tr) in (("flt1", got1[t], O.filter_frame(nz, w1, None, SIGMA, p1, trace=True)),
                                   ("flt2", got2[t], O.filter_frame(nz, w2, got1[t], SIGMA, p2, trace=True))):
            g, _ = cases.excuse_threshold_pixels(got, r, tr, f"{name} frame {t}", 16)
            cases.assert_close(g, r, f"{name} frame {t}")
        if not lag1 or t == 0:
            continue
        if lag1 == "inv":
            F = FR.invert(B, seq.SequenceFilter.LAG1_INVERT_STEPS)
        else:   # the smoother's own flow comes from the block matcher too
            F = BR.flow(_dev_gray(ctx, got2[t - 1], opp=True), _dev_gray(ctx, got2[t], opp=True), fscale=fscale)
        assert np.array_equal(_bits(ctx.download(sf.d_fflow, (H, W, 2))), _bits(F)), t
        focc = O.tvl1_occlusion_mask(F, th)
        assert np.array_equal(ctx.download(sf.d_focc, (H, W)), focc), t
        ref, tr = O.smooth_frame(got2[t - 1], O.warp_bicubic(got2[t], F, focc), None, SIGMA, ps, trace=True)
        g, _ = cases.excuse_threshold_pixels(ctx.download(sf.lsm1, (H, W, CH)), ref, tr, f"lsm1 frame {t - 1}", 16)
        cases.assert_close(g, ref, f"lsm1 frame {t - 1}")
    assert sf.flow_iterations == [] and (not lag1 or sf.lag1_flow_iterations == [])
    clean = O.rgb2opp(synth.clean_frame(W, H, CH, NF - 1))
    assert synth.psnr(got2[-1], clean) > synth.psnr(O.rgb2opp(frames[-1]), clean) + 3      # (and it did filter)


# ------------------------------------------------------------ GPU: the tools

DET = dict(os.environ, NLK_DETERMINISTIC="1")


def _rd(tmp_path, path):
    r = run("nlk-imgconv", path, tmp_path / "x.pfm")
    assert r.returncode == 0, r.stderr
    return rpfm(tmp_path / "x.pfm")


def _rflo(path):
    b = open(path, "rb").read()
    assert b[:4] == b"PIEH"
    w, h = np.frombuffer(b[4:12], "<i4")
    return np.frombuffer(b[12:], np.float32).reshape(h, w, 2)


def _write_inputs(tmp_path, frames, first=1):
    src = tmp_path / "in"
    src.mkdir()
    for t, f in enumerate(frames):
        wpfm(src / f"{t + first:03d}.pfm", f)
    return src


def _same(got, want, what):
    """the bounds of tests/test_sequence.py::test_one_process_tool_equals_the_driver: the same C-ABI calls in the same
    order with bit-reproducible aggregation"""
    d = np.abs(np.asarray(got, np.float64) - want)
    assert np.quantile(d, 0.99) < 2e-3 and np.sqrt(np.mean(d ** 2)) < 5e-2, what
    assert d.max() < 1e-3, (what, float(d.max()))


@pytest.mark.gpu
def test_seq_and_y4m_tools_under_bm(ctx, built, synth, tmp_path):
    """nlkalman-seq --of bm: its flt2 and smo1 frames are the Python driver's, its bflo files are Context.bm_flow of
    the gray images it saw; nlkalman-y4m --of bm writes exactly the codes of those flt2 files."""
    seq = importlib.import_module("bwd-nlkalman_amd.sequence")
    f = R.fmt("444", 0, 601)
    pay = [R.to_yuv(a, f).tobytes() for a in _frames(synth)]
    frames = [np.ascontiguousarray(R.to_rgb(p, W, H, f), np.float32) for p in pay]
    src = _write_inputs(tmp_path, frames)
    out = tmp_path / "bm"
    r = run("nlkalman-seq", "--of", "bm", src / "%03d.pfm", 1, NF, 20, out, env=DET)
    assert r.returncode == 0, r.stderr + r.stdout
    names = [f"{k}-{t:03d}.tif" for k in ("flt1", "flt2", "smo1") for t in range(1, NF + 1)] + \
            [f"{k}-{t:03d}.{e}" for k, e in (("bflo1", "flo"), ("bocc1", "png")) for t in range(2, NF + 1)] + \
            [f"{k}-{t:03d}.{e}" for k, e in (("fflo", "flo"), ("focc", "png")) for t in range(1, NF)]
    assert sorted(os.listdir(out)) == sorted(names)
    flt2 = [_rd(tmp_path, out / f"flt2-{t:03d}.tif") for t in range(1, NF + 1)]
    for t in range(1, NF):   # the flow file holds the flow that was used
        want = _dev_flow(ctx, _dev_gray(ctx, frames[t]), _dev_gray(ctx, flt2[t - 1]))
        assert np.array_equal(_bits(_rflo(out / f"bflo1-{t + 1:03d}.flo")), _bits(want)), t + 1
    ctx.set_deterministic(True)
    try:
        sf = seq.SequenceFilter(ctx, W, H, CH, 20.0, of="bm")
        for t, fr in enumerate(frames):
            d = ctx.upload(fr)
            sf.push(d)
            ctx.free(d)
            _same(flt2[t], sf.download_rgb(sf.flt2), f"flt2 of frame {t + 1}")
        smo = sf.smooth()     # (the backward pass: its flows come from the block matcher too)
        _same(_rd(tmp_path, out / "smo1-001.tif"), sf.download_rgb(smo[0]), "smo1 of frame 1")
        assert sf.flow_iterations == []
    finally:
        ctx.set_deterministic(False)
    r = _tool("nlkalman-y4m", "--of", "bm", 20, data=R.y4m_bytes(W, H, "444", pay), env=DET)
    assert r.returncode == 0, r.stderr
    line, _, _, _, got = R.y4m_parse(r.stdout)
    assert line == R.y4m_header(W, H, "444") and len(got) == NF
    for t in range(NF):
        assert got[t] == R.to_yuv(flt2[t], f).tobytes(), t + 1
    plain = _tool("nlkalman-y4m", 20, data=R.y4m_bytes(W, H, "444", pay), env=DET)
    assert plain.returncode == 0 and plain.stdout != r.stdout          # (and the option did something)


@pytest.mark.gpu
def test_bmflow_tool(ctx, built, synth, tmp_path):
    a, b = _frames(synth, 61, 45, 2)
    wpfm(tmp_path / "a.pfm", a)
    wpfm(tmp_path / "b.pfm", b)
    for args, kw in (((), {}), ((0, 3), dict(fscale=0, radius=3))):
        r = run("bmflow", tmp_path / "a.pfm", tmp_path / "b.pfm", tmp_path / "o.flo", *args)
        assert r.returncode == 0, r.stderr
        want = _dev_flow(ctx, _dev_gray(ctx, a), _dev_gray(ctx, b), **kw)
        assert np.array_equal(_bits(_rflo(tmp_path / "o.flo")), _bits(want)), args


def _tree(path):
    return {n: open(os.path.join(path, n), "rb").read() for n in sorted(os.listdir(path))}


@pytest.mark.gpu
@pytest.mark.parametrize("tool", TOOLS)
def test_default_run_is_the_tvl1_run(built, synth, tmp_path, tool):
    """--of tvl1 is the default: the same bytes in every file and on stdout"""
    if tool == "nlkalman-y4m":
        f = R.fmt("444", 0, 601)
        data = R.y4m_bytes(W, H, "444", [R.to_yuv(a, f).tobytes() for a in _frames(synth, nf=2)])
        a, b = (_tool(tool, *of, "--smooth", "tvl1", 20, data=data, env=DET) for of in ((), ("--of", "tvl1")))
        assert a.returncode == 0 and b.returncode == 0, a.stderr + b.stderr
        assert a.stdout == b.stdout and len(R.y4m_parse(a.stdout)[4]) == 2
        return
    frames = [synth.clean_frame(W, H, CH, t) for t in range(2)] if tool == "nlkalman-seq-gt" else _frames(synth, nf=2)
    src = _write_inputs(tmp_path, frames)
    outs = []
    for name, of in (("a", ()), ("b", ("--of", "tvl1"))):
        r = run(tool, *of, src / "%03d.pfm", 1, 2, 20, tmp_path / name, env=DET)
        assert r.returncode == 0, r.stderr + r.stdout
        outs.append((r.stdout, _tree(tmp_path / name)))
    assert outs[0][0] == outs[1][0]
    assert outs[0][1].keys() == outs[1][1].keys() and len(outs[0][1]) >= 6
    for n in outs[0][1]:
        assert outs[0][1][n] == outs[1][1][n], n
