"""The ground-truth loop of scripts/nlkalman-seq-gt.sh on the GPU: the noise (nlk_dev_awgn, Context.awgn,
bin/awgn), the error measure (nlk_dev_sqdiff_sum, Context.sqdiff_sum / mse) and bin/nlkalman-seq-gt.

The noise is pinned bit for bit to synth.awgn (the numpy restatement of the reference's generator, itself pinned
to the reference's own `awgn` by tests/test_reference_tools.py) and, where oracle/_ref/awgn is built, to that
tool. The measures are pinned to what oracle/_ref/plambda -c prints for the script's formula chain."""
import os
import re
import subprocess

import numpy as np
import pytest

from test_cli import rpfm, server, sock_dir, wpfm  # noqa: F401  (sock_dir: a fixture)
from test_reference_tools import iio  # noqa: F401  (a fixture: the reference's image I/O library)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "bwd-nlkalman_amd", "bin")
REF = os.path.join(ROOT, "oracle", "_ref")
GPU_STEP_S = 300   # time limit of one tool run on the GPU


def run(tool, *args, **kw):
    kw.setdefault("timeout", GPU_STEP_S)
    exe = tool if os.sep in tool else os.path.join(BIN, tool)
    return subprocess.run([exe, *map(str, args)], capture_output=True, text=True, **kw)


@pytest.fixture(scope="module")
def gt_tools(built):
    if not all(os.path.exists(os.path.join(BIN, t)) for t in ("awgn", "nlkalman-seq-gt", "nlk-imgconv")):
        built.build()
    return BIN


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32).astype(np.int64)


def _same_noise(got, want, what):
    """Bit for bit; the one accepted departure is a last-bit difference of OCML's and glibc's double log / cos,
    at most 1 float ulp, and it is counted (and printed)."""
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    assert got.shape == want.shape, what
    same = (_bits(got) == _bits(want)) | (np.isnan(got) & np.isnan(want))
    if same.all():
        return 0
    ulp = np.abs(_bits(got) - _bits(want))[~same]
    assert ulp.max() <= 1, f"{what}: {int((~same).sum())} samples differ, by up to {int(ulp.max())} ulp"
    print(f"{what}: {int((~same).sum())} samples differ by 1 ulp (libm last bit)")
    return int((~same).sum())


# ------------------------------------------------------------ CPU: the command lines

def test_awgn_usage_and_stdio(gt_tools, tmp_path):
    exe = os.path.join(BIN, "awgn")
    for args in ((), ("1", "2", "3", "4")):
        r = run("awgn", *args)
        assert r.returncode == 1 and r.stdout == ""
        assert r.stderr == f"usage:\n\t{exe} sigma [in [out]]\n"     # lib/imscript-lite/src/awgn.c:11-15
    wpfm(tmp_path / "in.pfm", np.zeros((4, 5, 3), np.float32))
    for args in (("10",), ("10", tmp_path / "in.pfm"), ("10", "-", tmp_path / "out.pfm")):
        r = run("awgn", *args, cwd=tmp_path)
        assert r.returncode == 1 and '"-"' in r.stderr and "not supported" in r.stderr
    assert not (tmp_path / "out.pfm").exists()


def test_seq_gt_command_line(gt_tools, tmp_path):
    r = run("nlkalman-seq-gt", "a", "1", "2")
    assert r.returncode == 1 and r.stderr.startswith("usage: ") and "SEQ FFR LFR SIG OUT [FPM [SPM [OPM]]]" in r.stderr
    # a missing clean frame: the script's message on stdout, status 1, no noise made
    (tmp_path / "clean").mkdir()
    wpfm(tmp_path / "clean" / "001.pfm", np.zeros((8, 8, 3), np.float32))
    out = tmp_path / "out"
    r = run("nlkalman-seq-gt", tmp_path / "clean" / "%03d.pfm", 1, 2, 20, out)
    assert r.returncode == 1 and r.stdout == f"ERROR: {tmp_path}/clean/002.pfm not found\n"
    assert not (out / "001.tif").exists()
    r = run("nlkalman-seq-gt", tmp_path / "clean" / "%03d.pfm", 1, 1, 20, out, "", "", "1 0.4 x")
    assert r.returncode == 1 and "OPM" in r.stderr
    assert not (out / "001.tif").exists()


# ------------------------------------------------------------ GPU: the kernels

AWGN_SHAPES = [(1, 1, 1), (37, 53, 3), (64, 64, 1), (7, 9, 3)]    # (7, 9, 3): n = 189, odd


@pytest.mark.gpu
@pytest.mark.parametrize("shape", AWGN_SHAPES)
def test_gpu_awgn_equals_synth(ctx, synth, shape):
    h, w, ch = shape
    clean = synth.clean_frame(w, h, ch)
    n = clean.size
    d_in = ctx.upload(clean)
    d_out = ctx.alloc(n * 4)
    try:
        for seed in (0, 1, 12345, 2 ** 32 - 1):
            for sigma in (0.0, 7.5, 20.0, 40.0):
                want = synth.awgn(clean, sigma, seed)
                ctx.awgn(d_out, d_in, n, sigma, seed)
                _same_noise(ctx.download(d_out, clean.shape), want, f"{shape} seed {seed} sigma {sigma}")
    finally:
        ctx.free(d_in)
        ctx.free(d_out)


@pytest.mark.gpu
def test_gpu_awgn_full_size_and_in_place(ctx, synth):
    clean = synth.clean_frame(1920, 1080, 3)
    n = clean.size
    d_in, d_out = ctx.upload(clean), ctx.alloc(n * 4)
    try:
        for seed, sigma in ((12345, 20.0), (2 ** 32 - 1, 7.5)):
            want = synth.awgn(clean, sigma, seed)
            ctx.awgn(d_out, d_in, n, sigma, seed)
            out = ctx.download(d_out, clean.shape)
            _same_noise(out, want, f"1080p seed {seed} sigma {sigma}")
        ctx.awgn(d_in, d_in, n, 7.5, 2 ** 32 - 1)        # in place = out of place
        assert np.array_equal(_bits(ctx.download(d_in, clean.shape)), _bits(out))
    finally:
        ctx.free(d_in)
        ctx.free(d_out)


@pytest.mark.gpu
@pytest.mark.parametrize("shape,sigma,seed", [((37, 53, 3), 20.0, 1), ((64, 64, 1), 40.0, 0),
                                              ((20, 31, 3), 7.5, 12345), ((9, 11, 3), 20.0, 4294967295)])
def test_gpu_awgn_tool_equals_the_reference_awgn(ctx, gt_tools, synth, iio, tmp_path, sock_dir, shape, sigma,  # noqa: F811
                                                 seed):
    ref = os.path.join(REF, "awgn")
    if not os.path.exists(ref):
        pytest.skip("oracle/_ref/awgn not built")
    h, w, ch = shape
    clean = synth.clean_frame(w, h, ch)
    iio.write(tmp_path / "clean.pfm", clean)
    env = dict(os.environ, SRAND=str(seed))
    r = run(ref, repr(sigma), tmp_path / "clean.pfm", tmp_path / "ref.pfm", env=env)
    assert r.returncode == 0, r.stderr
    want = iio.read(tmp_path / "ref.pfm").reshape(clean.shape)
    r = run("awgn", repr(sigma), tmp_path / "clean.pfm", tmp_path / "ours.pfm", env=env)
    assert r.returncode == 0, r.stderr
    _same_noise(iio.read(tmp_path / "ours.pfm").reshape(clean.shape), want, "bin/awgn vs the reference's awgn")
    d = ctx.upload(clean)
    ctx.awgn(d, d, clean.size, sigma, seed)
    _same_noise(ctx.download(d, clean.shape), want, "Context.awgn vs the reference's awgn")
    ctx.free(d)
    # behind nlk-server (whose own SRAND differs): the client's SRAND is the one used, same bytes
    with server(sock_dir, SRAND="777") as senv:
        r = run("awgn", repr(sigma), tmp_path / "clean.pfm", tmp_path / "served.pfm", env=dict(senv, SRAND=str(seed)))
    assert r.returncode == 0, r.stderr
    assert (tmp_path / "served.pfm").read_bytes() == (tmp_path / "ours.pfm").read_bytes()


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 63, 64, 65, 1_000_003, 1920 * 1080 * 3])
def test_gpu_sqdiff_sum(ctx, n):
    rng = np.random.default_rng(n)
    a = (rng.random(n) * 255).astype(np.float32)
    b = (a + rng.normal(0, 20, n)).astype(np.float32)
    want = float(np.sum((a.astype(np.float64) - b.astype(np.float64)) ** 2))
    d_a, d_b, d_s = ctx.upload(a), ctx.upload(b), ctx.alloc(16)
    try:
        ctx.sqdiff_sum(d_s, d_a, d_b, n)
        ctx.sqdiff_sum(d_s + 8, d_a, d_b, n)
        s = ctx.download(d_s, (2,), np.float64)
        assert abs(s[0] - want) <= 1e-12 * want
        assert s[0].tobytes() == s[1].tobytes()          # the same bits on every run
        assert ctx.mse(d_a, d_b, n) == s[0] / n
    finally:
        for d in (d_a, d_b, d_s):
            ctx.free(d)


@pytest.mark.gpu
def test_gpu_sqdiff_sums_of_frames_in_one_buffer(ctx, synth):
    frames = [synth.clean_frame(96, 64, 3, t) for t in range(5)]
    noisy = [synth.awgn(f, 20.0, t) for t, f in enumerate(frames)]
    n = frames[0].size
    d_c = [ctx.upload(f) for f in frames]
    d_n = [ctx.upload(f) for f in noisy]
    d_s = ctx.alloc(8 * len(frames))
    for t in range(len(frames)):          # nothing waits between the frames
        ctx.sqdiff_sum(d_s + 8 * t, d_c[t], d_n[t], n)
    s = ctx.download(d_s, (len(frames),), np.float64)
    for t in range(len(frames)):
        want = np.sum((frames[t].astype(np.float64) - noisy[t]) ** 2)
        assert abs(s[t] - want) <= 1e-12 * want
    for d in d_c + d_n + [d_s]:
        ctx.free(d)


# ------------------------------------------------------------ GPU: bin/nlkalman-seq-gt end to end

SIG, NF, FFR = 20, 4, 1
OPM = "1 0.40 0.75 1 0.40 0.75"


def _read(tmp_path, path):
    """any image file -> HWC float32 (through nlk-imgconv and PFM)"""
    pfm = tmp_path / (os.path.basename(str(path)) + ".conv.pfm")
    r = run("nlk-imgconv", path, pfm)
    assert r.returncode == 0, r.stderr
    a = rpfm(pfm)
    os.unlink(pfm)
    return a


def _write(tmp_path, path, a):
    pfm = tmp_path / (os.path.basename(str(path)) + ".conv.pfm")
    wpfm(pfm, a)
    r = run("nlk-imgconv", pfm, path)
    assert r.returncode == 0, r.stderr
    os.unlink(pfm)


def _plambda(expr):
    """`plambda -c expr` of the reference, or its arithmetic restated (every number read as a float, every
    operation in double rounded to float, printed %.15lf)"""
    tool = os.path.join(REF, "plambda")
    if os.path.exists(tool):
        r = subprocess.run([tool, "-c", expr], capture_output=True, text=True, timeout=60)
        assert r.returncode == 0, r.stderr
        return r.stdout.strip()
    st = []
    for tok in expr.split():
        if tok in ("sqrt", "log10"):
            st.append(np.float32(getattr(np, tok)(np.float64(st.pop()))))
        elif tok in "+*/":
            b, a = np.float64(st.pop()), np.float64(st.pop())
            st.append(np.float32(a + b if tok == "+" else a * b if tok == "*" else a / b))
        else:
            st.append(np.float32(tok))
    return "%.15f" % st[-1]


def _measures(mses):
    """the lines of OUT/measures from the per-frame MSEs [pass][frame] (scripts/nlkalman-seq-gt.sh:44-138), and the
    total MSEs as printed"""
    lines, tot = [], []
    for label, ms in zip(("F1", "F2", "S1"), mses):
        mm, pp, ss = [], [], "0"
        for n, m in enumerate(ms):
            m = "%g" % m
            mm.append(_plambda(f"{m} sqrt"))
            pp.append(_plambda(f"255 {mm[-1]} / log10 20 *"))
            ss = _plambda(f"{m} {n} {ss} * + {n + 1} /")
        rmse = _plambda(f"{ss} sqrt")
        lines += [f"{label} - Frame RMSE  " + " ".join(mm), f"{label} - Frame PSNR  " + " ".join(pp),
                  f"{label} - Total RMSE {rmse}", f"{label} - Total PSNR " + _plambda(f"255 {rmse} / log10 20 *")]
        tot.append(ss)
    return lines, tot


MEASURE_LINE = re.compile(r"([FS][12] - (?:Frame|Total) (?:RMSE|PSNR) ) ?(\S.*)")


def _same_measures(got, want):
    """the same labels in the same order; the numbers equal as text (with the reference's plambda), else to 1e-6
    relative"""
    assert len(got) == len(want), got
    for g, w in zip(got, want):
        gm, wm = MEASURE_LINE.fullmatch(g), MEASURE_LINE.fullmatch(w)
        assert gm and wm and gm.group(1) == wm.group(1), (g, w)
        if os.path.exists(os.path.join(REF, "plambda")):
            assert g == w
        else:
            assert np.allclose(np.array(gm.group(2).split(), float), np.array(wm.group(2).split(), float),
                               rtol=1e-6, atol=0), (g, w)


def _mse(clean, out):
    return float(np.mean((clean.astype(np.float64) - out.astype(np.float64)) ** 2))


def _clean_seq(tmp_path, synth, ch):
    src = tmp_path / "clean"
    src.mkdir()
    frames = {i: synth.clean_frame(96, 64, ch, i) for i in range(FFR, FFR + NF)}
    for i, f in frames.items():
        wpfm(src / ("%03d.pfm" % i), f)
    return src, frames


@pytest.mark.gpu
def test_seq_gt_end_to_end(gt_tools, synth, tmp_path):
    src, frames = _clean_seq(tmp_path, synth, 3)
    out, ref = tmp_path / "out", tmp_path / "ref"
    env = dict(os.environ, NLK_DETERMINISTIC="1", SRAND="4242")
    r = run("nlkalman-seq-gt", src / "%03d.pfm", FFR, FFR + NF - 1, SIG, out, "", "", OPM, env=env)
    assert r.returncode == 0, r.stderr
    # the noisy frames: synth.awgn with seed SRAND + frame number
    for i, c in frames.items():
        _same_noise(_read(tmp_path, out / ("%03d.tif" % i)), synth.awgn(c, SIG, 4242 + i), f"noisy frame {i}")
    # the recursion: nlkalman-seq's on those files, its TIFFs quantised as the PNG writer does
    r2 = run("nlkalman-seq", out / "%03d.tif", FFR, FFR + NF - 1, SIG, ref, 1, "", "", OPM, env=env)
    assert r2.returncode == 0, r2.stderr
    mses = [[], [], []]
    for i, c in frames.items():
        for p, kind in enumerate(("flt1", "flt2", "smo1")):
            tif = _read(tmp_path, ref / ("%s-%03d.tif" % (kind, i)))
            png = _read(tmp_path, out / ("%s-%03d.png" % (kind, i)))
            assert np.array_equal(png, np.clip(tif, 0, 255).astype(np.uint8).astype(np.float32)), (kind, i)
            mses[p].append(_mse(c, tif))
    names = set(os.listdir(out))
    assert not [f for f in names if re.match(r"(flt1|flt2|smo1)-\d+\.tif$", f)]
    assert {"bflo1-%03d.flo" % i for i in range(FFR + 1, FFR + NF)} <= names
    assert {"fflo-%03d.flo" % i for i in range(FFR, FFR + NF - 1)} <= names
    # OUT/measures: the script's 12 lines with plambda's numbers; stdout: one "%f %f %f" line
    lines, tot = _measures(mses)
    got = (out / "measures").read_text()
    assert got.endswith("\n") and len(lines) == 12
    _same_measures(got[:-1].split("\n"), lines)
    assert re.fullmatch(r"\S+ \S+ \S+\n", r.stdout), r.stdout
    assert np.allclose([float(v) for v in r.stdout.split()], [float(t) for t in tot], rtol=0, atol=1e-6)
    if os.path.exists(os.path.join(REF, "plambda")):
        assert r.stdout == "%s %s %s\n" % tuple("%f" % float(t) for t in tot)


@pytest.mark.gpu
def test_seq_gt_gray_no_smoothing_and_an_existing_noisy_frame(gt_tools, synth, tmp_path):
    src, frames = _clean_seq(tmp_path, synth, 1)
    out, ref = tmp_path / "out", tmp_path / "ref"
    out.mkdir()
    mine = synth.awgn(frames[FFR], 30.0, 99)               # made by hand, kept as it is
    _write(tmp_path, out / ("%03d.tif" % FFR), mine)
    before = (out / ("%03d.tif" % FFR)).read_bytes()
    env = dict(os.environ, NLK_DETERMINISTIC="1")
    env.pop("SRAND", None)
    r = run("nlkalman-seq-gt", src / "%03d.pfm", FFR, FFR + NF - 1, SIG, out, "", "no", OPM, env=env)
    assert r.returncode == 0, r.stderr
    assert (out / ("%03d.tif" % FFR)).read_bytes() == before
    for i in range(FFR + 1, FFR + NF):
        _same_noise(_read(tmp_path, out / ("%03d.tif" % i)), synth.awgn(frames[i], SIG, i), f"noisy frame {i}")
    names = set(os.listdir(out))
    assert not [f for f in names if re.match(r"(smo1-|fflo-|focc-)", f) or re.match(r"flt[12]-\d+\.tif$", f)]
    lines = (out / "measures").read_text().splitlines()
    assert len(lines) == 8 and re.fullmatch(r"\S+ \S+\n", r.stdout), r.stdout
    # the MSEs are those of nlkalman-seq run on the noisy files, the hand-made one among them
    r2 = run("nlkalman-seq", out / "%03d.tif", FFR, FFR + NF - 1, SIG, ref, 1, "", "no", OPM, env=env)
    assert r2.returncode == 0, r2.stderr
    for p, kind in enumerate(("flt1", "flt2")):
        rmse = [np.sqrt(_mse(frames[i], _read(tmp_path, ref / ("%s-%03d.tif" % (kind, i)))))
                for i in range(FFR, FFR + NF)]
        got = np.array(lines[4 * p].split("  ", 1)[1].split(), float)
        assert np.allclose(got, rmse, rtol=1e-5, atol=0), (kind, got, rmse)
