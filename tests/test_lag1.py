"""The lag-1 smoother (scripts/nlkalman-lsmo-seq.sh): seq_lag1_step of host/seq_step.c behind
SequenceFilter(lag1=...), bin/nlkalman-lsmo-seq and nlkalman-y4m --smooth, with the script's own TV-L1 flow ("tvl1")
or the inverted backward flow ("inv", nlk_dev_flow_invert). The oracle chain is composed here from the CPU oracle's
functions and, for "inv", the numpy restatement of the inversion (tests/flowinv_ref.py)."""
import importlib
import os
import subprocess

import numpy as np
import pytest

import cases
import flowinv_ref as FR
import yuv_ref as R
from test_cli import BIN, rpfm, run, wpfm

W, H, CH, SIGMA, NF = 96, 64, 3, 20.0, 3
STEPS = 4            # SEQ_LAG1_INVERT_STEPS of host/seq_step.h


def _lum(rgb):
    c = rgb.astype(np.float64)
    return (.299 * c[..., 0] + .587 * c[..., 1] + .114 * c[..., 2]).astype(np.float32)


def _oracle_lag1(O, prev2, cur2, F, th, sigma, ps, trace=False):
    """lsm1 of the previous frame from a forward flow F (script lines 98-108)"""
    F = np.ascontiguousarray(F, np.float32)
    occ = O.tvl1_occlusion_mask(F, th)
    return O.smooth_frame(prev2, O.warp_bicubic(cur2, F, occ), None, sigma, ps, trace=trace)


def _oracle_fflow(O, prev2, cur2, lam, fscale):
    u, v = O.tvl1_flow(_lum(O.opp2rgb(prev2)), _lum(O.opp2rgb(cur2)), lam=lam, fscale=fscale)
    return np.stack([u, v], -1)


def _oracle_chain(O, frames, sigma, lam, fscale, th):
    """the script's recursion, free running: flt2, lsm1 by its own flow, lsm1 by the inverted backward flow"""
    p1, p2, ps = (O.default_params(sigma, m) for m in (O.FLT1, O.FLT2, O.SMO1))
    f1s, f2s, lt, li = [], [], [], []
    for t, rgb in enumerate(frames):
        nz = O.rgb2opp(rgb)
        if t == 0:
            f1 = O.filter_frame(nz, None, None, sigma, p1)
            f2 = O.filter_frame(nz, None, f1, sigma, p2)
        else:
            u, v = O.tvl1_flow(_lum(rgb), _lum(O.opp2rgb(f2s[-1])), lam=lam, fscale=fscale)
            B = np.stack([u, v], -1)
            occ = O.tvl1_occlusion_mask(B, th)
            f1 = O.filter_frame(nz, O.warp_bicubic(f1s[-1], B, occ), None, sigma, p1)
            f2 = O.filter_frame(nz, O.warp_bicubic(f2s[-1], B, occ), f1, sigma, p2)
            lt.append(_oracle_lag1(O, f2s[-1], f2, _oracle_fflow(O, f2s[-1], f2, lam, fscale), th, sigma, ps))
            li.append(_oracle_lag1(O, f2s[-1], f2, FR.invert(B, STEPS), th, sigma, ps))
        f1s.append(f1)
        f2s.append(f2)
    return f2s, lt + [f2s[-1]], li + [f2s[-1]]


# ------------------------------------------------------------ CPU

def test_lag1_quality_on_the_cpu_oracle(O, synth):
    """What the smoother is for, on frames other than those of DESIGN.md §9's table (seeds 100 + t: +0.47 dB there):
    lag 1 with the script's flow gains at least half of that, and the inverted flow keeps at least half of the gain."""
    nf = 4
    frames = [synth.awgn(synth.clean_frame(W, H, CH, t), SIGMA, 300 + t) for t in range(nf)]
    f2s, lt, li = _oracle_chain(O, frames, SIGMA, 0.25, 1, 0.75)
    clean = [O.rgb2opp(synth.clean_frame(W, H, CH, t)) for t in range(nf)]
    mean = lambda xs: float(np.mean([synth.psnr(x, c) for x, c in zip(xs[:nf - 1], clean)]))
    flt2, tvl1, inv = mean(f2s), mean(lt), mean(li)
    print("mean PSNR of frames 0..2: flt2 %.3f, lag-1 tvl1 %.3f, lag-1 inv %.3f" % (flt2, tvl1, inv))
    assert tvl1 - flt2 >= 0.23
    assert inv - flt2 >= 0.5 * (tvl1 - flt2)


def test_usage_errors(built, tmp_path):
    if not os.path.exists(os.path.join(os.path.dirname(built.__file__), "bin", "nlkalman-lsmo-seq")):
        built.build()
    data = R.y4m_bytes(4, 2, None, [])
    for args in (("--smooth", "bogus", 20), ("--opm", "1 0.25 0.75 1", 20), ("--smooth",)):
        r = subprocess.run([os.path.join(BIN, "nlkalman-y4m"), *map(str, args)], input=data, capture_output=True)
        assert r.returncode == 1 and r.stdout == b"", args
        assert r.stderr.startswith(b"nlkalman-y4m: ") and r.stderr.count(b"\n") == 1, (args, r.stderr)
    r = run("nlkalman-lsmo-seq")
    assert r.returncode == 1 and "[--flow tvl1|inv] SEQ FFR LFR SIG OUT [FPM [SPM [OPM]]]" in r.stderr
    r = run("nlkalman-lsmo-seq", "--flow", "bogus", tmp_path / "%03d.tif", 1, 3, 20, tmp_path / "out")
    assert r.returncode == 1 and "want tvl1 or inv" in r.stderr
    for flow in ((), ("--flow", "inv")):
        r = run("nlkalman-lsmo-seq", *flow, tmp_path / "%03d.tif", 1, 3, 20, tmp_path / "out")
        assert r.returncode == 1 and r.stdout.startswith("ERROR: ") and "001.tif not found" in r.stdout
    r = run("nlkalman-lsmo-seq", tmp_path / "%03d.tif", 1, 3, 20, tmp_path / "out", "", "", "1 2 3")
    assert r.returncode == 1 and "OPM must hold 6 numbers" in r.stderr


# ------------------------------------------------------------ GPU: the driver against the oracle

def _frames(synth, w=W, h=H):
    return [synth.awgn(synth.clean_frame(w, h, CH, t), SIGMA, 100 + t) for t in range(NF)]   # tests/test_sequence.py's


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["tvl1", "inv"])
def test_driver_equals_oracle_recursion(ctx, built, O, synth, mode):
    """Stage by stage, the oracle fed with the driver's own flt2 frames (and, for "inv", the restatement's inverse of
    the driver's own backward flow), as tests/test_sequence.py does for smo1; the free-running chain in PSNR."""
    seq = importlib.import_module("bwd-nlkalman_amd.sequence")
    frames = _frames(synth)
    lam, fscale, th = 0.40, 0, 0.75
    ps = O.default_params(SIGMA, O.SMO1)
    sf = seq.SequenceFilter(ctx, W, H, CH, SIGMA, of_lambda=lam, of_fscale=fscale, occ_th=th, keep_history=False, lag1=mode)
    got2, lsm = [], []
    for t, rgb in enumerate(frames):
        d = ctx.upload(rgb)
        sf.push(d)
        ctx.free(d)
        got2.append(ctx.download(sf.flt2, (H, W, CH)))
        if t == 0:
            assert sf.lsm1 is None
            continue
        lsm.append(ctx.download(sf.lsm1, (H, W, CH)))
        fflow = ctx.download(sf.d_fflow, (H, W, 2))
        if mode == "inv":
            F = FR.invert(ctx.download(sf.d_flow, (H, W, 2)), STEPS)
            assert np.array_equal(fflow.view(np.uint32), F.view(np.uint32)), t
            assert np.array_equal(ctx.download(sf.d_focc, (H, W)), O.tvl1_occlusion_mask(F, th)), t
        else:   # (the driver's flow saw the gray of its own device RGB frames: the oracle's differs in the last bits)
            F = _oracle_fflow(O, got2[t - 1], got2[t], lam, fscale)
            print("frame %d: forward flow, driver against oracle: max-abs %.3e" % (t, np.abs(fflow - F).max()))
        ref, tr = _oracle_lag1(O, got2[t - 1], got2[t], F, th, SIGMA, ps, trace=True)
        g, _ = cases.excuse_threshold_pixels(lsm[-1], ref, tr, f"lsm1 frame {t - 1}", 16)
        cases.assert_close(g, ref, f"lsm1 frame {t - 1}")
    assert sf.finish() == sf.flt2
    assert np.array_equal(ctx.download(sf.finish(), (H, W, CH)), got2[-1])
    lsm.append(got2[-1])
    assert len(sf.flow_iterations) == NF - 1                      # (keeps its meaning: the backward flows)
    assert len(sf.lag1_flow_iterations) == (NF - 1 if mode == "tvl1" else 0)
    r2, rt, ri = _oracle_chain(O, frames, SIGMA, lam, fscale, th)
    rl = rt if mode == "tvl1" else ri
    for t in range(NF):
        clean = O.rgb2opp(synth.clean_frame(W, H, CH, t))
        assert abs(synth.psnr(got2[t], clean) - synth.psnr(r2[t], clean)) < 0.02, f"flt2 frame {t}"
        assert abs(synth.psnr(lsm[t], clean) - synth.psnr(rl[t], clean)) < 0.02, f"lsm1 frame {t}"
    clean = O.rgb2opp(synth.clean_frame(W, H, CH, 0))
    assert synth.psnr(lsm[0], clean) > synth.psnr(got2[0], clean)            # (and it did smooth)


def test_lag1_parameter_is_checked(built):
    seq = importlib.import_module("bwd-nlkalman_amd.sequence")
    with pytest.raises(ValueError):
        seq.SequenceFilter(None, W, H, CH, SIGMA, lag1="bogus")


# ------------------------------------------------------------ GPU: the tools

DET = dict(os.environ, NLK_DETERMINISTIC="1")
OPM = "0 0.40 0.75 0 0.40 0.75"


def _rd(tmp_path, path):
    r = run("nlk-imgconv", path, tmp_path / "x.pfm")
    assert r.returncode == 0, r.stderr
    return rpfm(tmp_path / "x.pfm")


def _rflo(path):
    b = open(path, "rb").read()
    assert b[:4] == b"PIEH"
    w, h = np.frombuffer(b[4:12], "<i4")
    return np.frombuffer(b[12:], np.float32).reshape(h, w, 2)


def _write_inputs(tmp_path, frames, first=3):
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
@pytest.mark.parametrize("mode", ["tvl1", "inv"])
@pytest.mark.parametrize("w,h", [(96, 64), (95, 63)])
def test_lsmo_tool_equals_nlkalman_seq_and_the_driver(ctx, built, synth, tmp_path, w, h, mode):
    """bin/nlkalman-lsmo-seq = scripts/nlkalman-lsmo-seq.sh in one process: the script's files; its forward
    recursion is nlkalman-seq's, byte for byte; its smoothed frames, forward flows and masks are the driver's."""
    seq = importlib.import_module("bwd-nlkalman_amd.sequence")
    frames = _frames(synth, w, h)
    src = _write_inputs(tmp_path, frames)
    last = 3 + NF - 1
    ref, out = tmp_path / "seq", tmp_path / mode
    r = run("nlkalman-seq", src / "%03d.pfm", 3, last, SIGMA, ref, 1, "", "no", OPM, env=DET)
    assert r.returncode == 0, r.stderr + r.stdout
    flag = () if mode == "tvl1" else ("--flow", "inv")         # (tvl1 is the default, the script's)
    r = run("nlkalman-lsmo-seq", *flag, src / "%03d.pfm", 3, last, SIGMA, out, "", "", OPM, env=DET)
    assert r.returncode == 0, r.stderr + r.stdout
    want = [f"{k}-{t:03d}.tif" for k in ("flt1", "flt2", "lsm1") for t in range(3, last + 1)] + \
           [f"{k}-{t:03d}.{e}" for k, e in (("bflo", "flo"), ("bocc", "png"), ("fflo", "flo"), ("focc", "png"))
            for t in range(4, last + 1)]
    assert sorted(os.listdir(out)) == sorted(want)
    for t in range(3, last + 1):
        for k in ("flt1", "flt2"):
            assert (out / f"{k}-{t:03d}.tif").read_bytes() == (ref / f"{k}-{t:03d}.tif").read_bytes(), (k, t)
    for t in range(4, last + 1):
        assert (out / f"bflo-{t:03d}.flo").read_bytes() == (ref / f"bflo1-{t:03d}.flo").read_bytes(), t
        assert (out / f"bocc-{t:03d}.png").read_bytes() == (ref / f"bocc1-{t:03d}.png").read_bytes(), t
    assert np.array_equal(_rd(tmp_path, out / f"lsm1-{last:03d}.tif"), _rd(tmp_path, out / f"flt2-{last:03d}.tif"))
    ctx.set_deterministic(True)
    try:
        sf = seq.SequenceFilter(ctx, w, h, CH, SIGMA, of_lambda=0.40, of_fscale=0, occ_th=0.75, keep_history=False,
                                lag1=mode)
        for t, f in enumerate(frames):
            d = ctx.upload(f)
            sf.push(d)
            ctx.free(d)
            if t == 0:
                continue
            _same(_rd(tmp_path, out / f"lsm1-{t + 2:03d}.tif"), sf.download_rgb(sf.lsm1), f"lsm1 of frame {t + 2}")
            _same(_rflo(out / f"fflo-{t + 3:03d}.flo"), ctx.download(sf.d_fflow, (h, w, 2)), f"fflo {t + 3}")
            _same(_rd(tmp_path, out / f"focc-{t + 3:03d}.png")[..., 0], ctx.download(sf.d_focc, (h, w)), f"focc {t + 3}")
    finally:
        ctx.set_deterministic(False)


@pytest.mark.gpu
def test_lsmo_tool_without_smoothing(ctx, built, synth, tmp_path):
    """SPM = no: the forward recursion alone, no fflo / focc / lsm1"""
    src = _write_inputs(tmp_path, _frames(synth)[:2])
    ref, out = tmp_path / "seq", tmp_path / "nosmo"
    r = run("nlkalman-seq", src / "%03d.pfm", 3, 4, SIGMA, ref, 1, "", "no", OPM, env=DET)
    assert r.returncode == 0, r.stderr + r.stdout
    r = run("nlkalman-lsmo-seq", "--flow", "inv", src / "%03d.pfm", 3, 4, SIGMA, out, "", "no", OPM, env=DET)
    assert r.returncode == 0, r.stderr + r.stdout
    assert sorted(os.listdir(out)) == ["bflo-004.flo", "bocc-004.png", "flt1-003.tif", "flt1-004.tif", "flt2-003.tif",
                                       "flt2-004.tif"]
    assert (out / "flt2-004.tif").read_bytes() == (ref / "flt2-004.tif").read_bytes()


def _y4m(*args, data, env=DET):
    return subprocess.run([os.path.join(BIN, "nlkalman-y4m"), *map(str, args)], input=data, capture_output=True, env=env)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["tvl1", "inv"])
@pytest.mark.parametrize("w,h,tag", [(96, 64, "444"), (95, 63, "420jpeg")])
def test_y4m_smooth_equals_the_lsmo_tool(ctx, built, synth, tmp_path, w, h, tag, mode):
    """Both tools make the same calls on the same bits (NLK_DETERMINISTIC=1): the stream's frames are the codes of
    nlkalman-lsmo-seq's lsm1 files, exactly (the pattern of tests/test_y4m.py for flt2)."""
    f = R.fmt(tag, 0, 601)
    pay = [R.to_yuv(a, f).tobytes() for a in _frames(synth, w, h)]
    src = _write_inputs(tmp_path, [R.to_rgb(p, w, h, f) for p in pay], first=1)
    out = tmp_path / mode
    r = run("nlkalman-lsmo-seq", "--flow", mode, src / "%03d.pfm", 1, NF, 20, out, env=DET)
    assert r.returncode == 0, r.stderr + r.stdout
    want = [R.to_yuv(_rd(tmp_path, out / f"lsm1-{t + 1:03d}.tif"), f).tobytes() for t in range(NF)]
    r = _y4m("--smooth", mode, 20, data=R.y4m_bytes(w, h, tag, pay))
    assert r.returncode == 0, r.stderr
    line, _, _, _, got = R.y4m_parse(r.stdout)
    assert line == R.y4m_header(w, h, tag) and len(got) == NF
    for t in range(NF):
        diff = np.frombuffer(got[t], np.uint8).astype(int) - np.frombuffer(want[t], np.uint8)
        print("frame %d: %d of %d codes differ, max %d" % (t + 1, np.count_nonzero(diff), diff.size, np.abs(diff).max()))
        assert got[t] == want[t], t + 1
    assert got[0] != pay[0]


@pytest.fixture(scope="module")
def stream(synth):
    """(payloads, the stream, its flt2 frames: the tool without --smooth) at 96 x 64, 4:4:4"""
    f = R.fmt("444", 0, 601)
    pay = [R.to_yuv(a, f).tobytes() for a in _frames(synth)]
    data = R.y4m_bytes(W, H, "444", pay)
    r = _y4m(20, data=data)
    assert r.returncode == 0, r.stderr
    return pay, data, R.y4m_parse(r.stdout)[4]


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["tvl1", "inv"])
def test_y4m_smooth_frame_counts_truncation_and_inline_io(ctx, built, stream, mode):
    pay, data, plain = stream
    r = _y4m("--smooth", mode, 20, data=data)
    assert r.returncode == 0, r.stderr
    got = R.y4m_parse(r.stdout)[4]
    # as many frames out as in, in order; the last one is its flt2
    assert len(plain) == NF and len(got) == NF and got[NF - 1] == plain[NF - 1] and got[0] != plain[0]
    for n in (1, 2):
        rn = _y4m("--smooth", mode, 20, data=R.y4m_bytes(W, H, "444", pay[:n]))
        assert rn.returncode == 0, rn.stderr
        short = R.y4m_parse(rn.stdout)[4]
        assert len(short) == n and short[:n - 1] == got[:n - 1] and short[n - 1] == plain[n - 1], n
    # in-line I/O: the same bytes
    inline = dict(DET, NLK_SEQ_IO_THREADS="0")
    r0 = _y4m("--smooth", mode, 20, data=data, env=inline)
    assert r0.returncode == 0 and r0.stdout == r.stdout, r0.stderr
    # a stream cut inside frame 3: the two complete frames, the second as its flt2, status 1 and the message
    cut = data[:len(data) - len(pay[2]) // 2]
    for env in (DET, inline) if mode == "inv" else (DET,):
        r3 = _y4m("--smooth", mode, 20, data=cut, env=env)
        assert r3.returncode == 1
        assert r3.stderr.count(b"\n") == 1 and b"frame 3: the stream ends inside a frame" in r3.stderr, r3.stderr
        assert R.y4m_parse(r3.stdout)[4] == [got[0], plain[1]]
    if mode == "inv":   # 6 numbers with the second triple equal to the first are the 3 numbers; --spm is read
        r6 = _y4m("--smooth", mode, "--opm", "1 0.25 0.75 1 0.25 0.75", "--spm", "--s1_p 8", 20, data=data)
        assert r6.returncode == 0 and r6.stdout == r.stdout, r6.stderr


@pytest.mark.gpu
def test_y4m_smooth_under_vst_transforms_back(ctx, built, synth, tmp_path):
    """SIG = vst:A,B: the smoothed frames leave through the inverse transform, as nlkalman-lsmo-seq's files do"""
    w, h, tag = 96, 64, "444"
    f = R.fmt(tag, 0, 601)
    pay = [R.to_yuv(a, f).tobytes() for a in _frames(synth, w, h)[:2]]
    src = _write_inputs(tmp_path, [R.to_rgb(p, w, h, f) for p in pay], first=1)
    r = run("nlkalman-lsmo-seq", "--flow", "inv", src / "%03d.pfm", 1, 2, "vst:0.5,4", tmp_path / "out", env=DET)
    assert r.returncode == 0, r.stderr + r.stdout
    want = [R.to_yuv(_rd(tmp_path, tmp_path / "out" / f"lsm1-{t + 1:03d}.tif"), f).tobytes() for t in range(2)]
    r = _y4m("--smooth", "inv", "vst:0.5,4", data=R.y4m_bytes(w, h, tag, pay))
    assert r.returncode == 0, r.stderr
    assert R.y4m_parse(r.stdout)[4] == want
