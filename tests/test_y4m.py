"""Planar Y'CbCr in and out: struct nlk_yuv_format and its two host functions, the kernels nlk_dev_yuv_to_rgb /
nlk_dev_rgb_to_yuv against their float32 numpy restatement (tests/yuv_ref.py) bit for bit, the container module
host/y4m.c on well-formed and malformed streams, and bin/nlkalman-y4m against nlkalman-seq on the same frames."""
import os
import subprocess

import numpy as np
import pytest

import yuv_ref as R
from test_cli import BIN, ROOT, rpfm, run, wpfm

TOOL = os.path.join(BIN, "nlkalman-y4m")
FIELDS = ("mono", "sx", "sy", "cosited_x", "depth", "full_range", "matrix")
ACCEPTED = [None, "", "420jpeg", "420mpeg2", "420", "422", "444", "mono"] + \
           [fam + str(n) for fam in ("420p", "422p", "444p", "mono") for n in range(9, 17)]
REFUSED = ["420paldv", "411", "444alpha", "420p8", "420p17", "444p", "mono8", "mono17", "420jpeg10", "440", "C420",
           "420 ", "yuv420p", "422p010", "444p1x"]


@pytest.fixture(scope="module")
def tool(built):
    if not os.path.exists(TOOL):
        built.build()
    return TOOL


def y4m(*args, data=None, env=None):
    return subprocess.run([TOOL, *map(str, args)], input=data, capture_output=True, env=env, timeout=120)


def c_fmt(pkg, f):
    return pkg.YuvFormat(*(getattr(f, k) for k in FIELDS))


# ------------------------------------------------------------ CPU: the format

def test_format_from_tag_and_frame_bytes(built):
    for tag in ACCEPTED:
        got, want = built.yuv_format_from_tag(tag), R.fmt(tag)
        assert [getattr(got, k) for k in FIELDS] == [getattr(want, k) for k in FIELDS], tag
        for w, h in ((1, 1), (2, 2), (3, 3), (17, 5), (64, 33), (131, 67), (1920, 1080)):
            assert got.frame_bytes(w, h) == R.frame_bytes(w, h, want), (tag, w, h)
    f = built.yuv_format_from_tag("420jpeg")
    assert f.frame_bytes(17, 5) == 85 + 2 * 9 * 3           # (Cb starts at byte 85)
    assert built.yuv_format_from_tag("420p10").frame_bytes(17, 5) == 2 * (85 + 2 * 9 * 3)
    assert f.frame_bytes(0, 5) == 0 and f.frame_bytes(5, -1) == 0
    L = built.hip()
    for tag in REFUSED:
        g = built.YuvFormat(9, 9, 9, 9, 9, 9, 9)            # a refused tag leaves the struct alone ...
        assert L.nlk_yuv_format_from_tag(g, tag.encode()) == -4, tag    # NLK_EUNSUP
        assert tag.encode() in L.nlk_last_error(None)
        assert g.frame_bytes(17, 5) == 0, tag               # ... and what it holds is no format
        with pytest.raises(built.NlkError):
            built.yuv_format_from_tag(tag)
    for field, bad in (("depth", 7), ("depth", 17), ("sx", 3), ("sy", 0), ("matrix", 2020), ("full_range", 2),
                       ("cosited_x", -1)):
        g = built.yuv_format_from_tag("420jpeg")
        setattr(g, field, bad)
        assert g.frame_bytes(17, 5) == 0, (field, bad)
    big = 2 ** 31 - 1                                       # the largest sizes: no wrap on the way, 0 past SIZE_MAX / 2
    assert built.yuv_format_from_tag("mono").frame_bytes(big, big) == big * big
    assert built.yuv_format_from_tag("444p16").frame_bytes(big, big) == 0


# ------------------------------------------------------------ CPU: the restatement itself

@pytest.mark.parametrize("full_range", [0, 1])
@pytest.mark.parametrize("matrix", [601, 709])
def test_ref_444_identity_all_8bit_triples(full_range, matrix):
    """codes -> RGB -> codes is the identity at 4:4:4 for every one of the 2^24 8-bit triples"""
    n = 4096
    i = np.arange(n * n, dtype=np.uint32)
    f = R.fmt("444", full_range, matrix)
    p = R.join((i >> 16).astype(np.uint8), ((i >> 8) & 255).astype(np.uint8), (i & 255).astype(np.uint8), f)
    assert np.array_equal(R.to_yuv(R.to_rgb(p, n, n, f), f), p)


def _filter_161(c, luma_shape):
    """[1 6 1] / 8 along both axes of a chroma plane, the edge sample replicated, in double: what interpolating to
    the luma grid with (3/4, 1/4) and averaging the pairs again amounts to. Where the luma length is odd the last
    chroma sample covers one luma position only, the interpolated value there: [1 3] / 4."""
    c = c.astype(np.float64)
    for ax in (0, 1):
        p = np.concatenate([np.take(c, [0], ax), c, np.take(c, [-1], ax)], ax)
        n = c.shape[ax]
        out = (np.take(p, range(0, n), ax) + 6.0 * np.take(p, range(1, n + 1), ax) + np.take(p, range(2, n + 2), ax)) / 8.0
        if luma_shape[ax] % 2:
            last = (np.take(p, [n - 1], ax) + 3.0 * np.take(p, [n], ax)) / 4.0
            out = np.concatenate([np.take(out, range(0, n - 1), ax), last], ax)
        c = out
    return c


@pytest.mark.parametrize("w,h", [(64, 48), (37, 21)])
def test_ref_420_centred_there_and_back_is_the_161_filter(w, h):
    rng = np.random.default_rng(5)
    f = R.fmt("420jpeg", 0, 709)
    cw, chh = R.chroma_size(w, h, f)
    # chroma well inside the RGB cube's image (no code is clamped on the way back)
    Y = rng.integers(90, 170, (h, w))
    Cb, Cr = (rng.integers(100, 156, (chh, cw)) for _ in range(2))
    Y2, Cb2, Cr2 = R.split(R.to_yuv(R.to_rgb(R.join(Y, Cb, Cr, f), w, h, f), f), w, h, f)
    assert np.abs(Y2.astype(int) - Y).max() <= 1
    for got, src in ((Cb2, Cb), (Cr2, Cr)):
        assert np.abs(got.astype(np.float64) - np.rint(_filter_161(src, (h, w)))).max() <= 1


# ------------------------------------------------------------ CPU: the container, through --probe and a stand-alone program

def _payloads(w, h, f, n, seed=0):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, R.frame_bytes(w, h, f), dtype=np.uint8).tobytes() for _ in range(n)]


def _good_streams():
    out = []
    for w, h, tag, extra, n in ((17, 5, None, "", 3), (64, 33, "420mpeg2", " XYSCSS=420MPEG2", 2),
                                (1280, 6, "422", "", 1), (96, 64, "444p10", " XCOLORRANGE=FULL", 2),
                                (31, 7, "mono", " XCOLORRANGE=LIMITED XFOO=1", 4), (3, 3, "420p12", "", 0)):
        out.append((w, h, tag, extra, n, R.y4m_bytes(w, h, tag, _payloads(w, h, R.fmt(tag), n), extra)))
    return out


def _malformed():
    """(name, bytes, a word of the message) for every malformed input the module must refuse"""
    f = R.fmt(None)
    p = _payloads(4, 2, f, 2)
    good = R.y4m_bytes(4, 2, None, p)
    head = R.y4m_header(4, 2)
    return [
        ("empty", b"", "empty"),
        ("no magic", b"YUV4MPEG W4 H2\n" + good[16:], "magic"),
        ("magic glued", b"YUV4MPEG2W4 H2\nFRAME\n" + p[0], "magic"),
        ("no W", b"YUV4MPEG2 H2 F25:1\nFRAME\n" + p[0], "W is missing"),
        ("no H", b"YUV4MPEG2 W4 F25:1\nFRAME\n" + p[0], "H is missing"),
        ("W not a number", b"YUV4MPEG2 Wx4 H2\nFRAME\n" + p[0], "size"),
        ("W negative", b"YUV4MPEG2 W-4 H2\nFRAME\n" + p[0], "size"),
        ("H zero", b"YUV4MPEG2 W4 H0\nFRAME\n" + p[0], "size"),
        ("H trailing junk", b"YUV4MPEG2 W4 H2x\nFRAME\n" + p[0], "size"),
        ("W overflows int", b"YUV4MPEG2 W99999999999 H2\nFRAME\n" + p[0], "size"),
        ("bad F", b"YUV4MPEG2 W4 H2 F25\nFRAME\n" + p[0], "frame rate"),
        ("interlaced", b"YUV4MPEG2 W4 H2 It\nFRAME\n" + p[0], "interlaced"),
        ("C unsupported", b"YUV4MPEG2 W4 H2 C420paldv\nFRAME\n" + p[0], "420paldv"),
        ("C 411", b"YUV4MPEG2 W4 H2 C411\nFRAME\n" + p[0], "411"),
        ("C overlong", b"YUV4MPEG2 W4 H2 C" + b"4" * 100 + b"\nFRAME\n" + p[0], "not supported"),
        ("header too long", b"YUV4MPEG2 W4 H2 X" + b"a" * 400 + b"\nFRAME\n" + p[0], "longer"),
        ("header without newline", b"YUV4MPEG2 W4 H2 X" + b"a" * 5000, "longer"),
        ("header cut", b"YUV4MPEG2 W4 H", "ends inside the header"),
        ("NUL in header", b"YUV4MPEG2 W4 H2 X\0\nFRAME\n" + p[0], "NUL"),
        ("FRAME misspelt", head + b"FRAME\n" + p[0] + b"FRAMF\n" + p[1], "FRAME expected"),
        ("FRAME glued", head + b"FRAMEX\n" + p[0], "FRAME expected"),
        ("FRAME line too long", head + b"FRAME " + b"x" * 300 + b"\n" + p[0], "longer"),
        ("FRAME line cut", head + b"FRAME\n" + p[0] + b"FRA", "FRAME line"),
        ("payload cut", good[:-5], "ends inside a frame"),
        ("payload missing", head + b"FRAME\n", "ends inside a frame"),
    ]


def test_probe_reads_what_the_reference_writer_wrote(tool, tmp_path):
    for k, (w, h, tag, extra, n, data) in enumerate(_good_streams()):
        f = R.fmt(tag)
        path = tmp_path / ("s%d.y4m" % k)
        path.write_bytes(data)
        rng = "full" if "RANGE=FULL" in extra else "limited"
        want = "%d %d 25:1 p 1:1 %s %d %s %d %d\n" % (w, h, tag or "420jpeg", f.depth, rng,
                                                     709 if w >= 1280 or h > 576 else 601, n)
        r = y4m("--probe", 0, path)
        assert (r.returncode, r.stdout.decode(), r.stderr) == (0, want, b""), (tag, r)
        # the same bytes through a pipe, 1000 at a time
        p = subprocess.Popen([TOOL, "--probe", "0"], stdin=subprocess.PIPE, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        for at in range(0, len(data), 1000):
            p.stdin.write(data[at:at + 1000])
            p.stdin.flush()
        out, err = p.communicate(timeout=60)
        assert (p.returncode, out.decode(), err) == (0, want, b""), tag
    w, h, tag, extra, n, data = _good_streams()[0]
    r = y4m("--probe", "--frames", 2, "--matrix", 709, "--range", "full", 0, "-", data=data)
    assert r.stdout.decode() == "17 5 25:1 p 1:1 420jpeg 8 full 709 2\n"
    # a FRAME line may carry parameters; a header may be the magic and the two sizes alone, tags in any order
    p = _payloads(4, 2, R.fmt(None), 2)
    r = y4m("--probe", 0, data=b"YUV4MPEG2 H2 W4\nFRAME Ip\n" + p[0] + b"FRAME\n" + p[1])
    assert (r.returncode, r.stdout.decode()) == (0, "4 2 0:0 ? 0:0 420jpeg 8 limited 601 2\n")


def test_probe_refuses_malformed_streams(tool, tmp_path):
    for name, data, word in _malformed():
        for how in ("file", "pipe"):
            if how == "file":
                (tmp_path / "bad.y4m").write_bytes(data)
                r = y4m("--probe", 0, tmp_path / "bad.y4m")
            else:
                r = y4m("--probe", 0, "-", data=data)
            msg = r.stderr.decode(errors="replace")
            assert r.returncode == 1 and r.stdout == b"", (name, how, r)
            assert msg.startswith("nlkalman-y4m: ") and msg.count("\n") == 1 and msg.endswith("\n"), (name, msg)
            assert word in msg, (name, msg)


def test_usage_errors(tool):
    for args in ((), ("--matrix", "2020", 20), ("--range", "tv", 20), ("--opm", "1 2", 20), ("--frames", "x", 20),
                 ("--nonsense", 20), ("vst:1", ), ("--fpm",)):
        r = y4m(*args, data=R.y4m_bytes(4, 2, None, []))
        assert r.returncode == 1 and r.stdout == b"" and r.stderr, args
    r = y4m("--probe", 0, "/nonexistent/x.y4m")
    assert r.returncode == 1 and b"cannot open" in r.stderr


def test_container_module_under_sanitizers(built, tmp_path):
    """host/y4m.c with a small driver as a stand-alone program, under AddressSanitizer and UBSan where the compiler
    links them (else the plain build), over the same streams"""
    src = [os.path.join(ROOT, "tests", "y4m_driver.c"), os.path.join(ROOT, "bwd-nlkalman_amd", "host", "y4m.c")]
    inc = ["-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "bwd-nlkalman_amd", "host")]
    exe, path = str(tmp_path / "y4m_driver"), str(tmp_path / "s.y4m")
    base = ["gcc", "-O1", "-g", "-std=gnu99", "-Wall", "-Werror", *inc, "-o", exe, *src]
    # the sanitizer runtimes linked statically: the program then runs in any environment as it is. Where that build
    # does not link, or does not start here (asked to open no file, before the module is called at all), the plain build
    san = base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"]
    ok = subprocess.run(san, capture_output=True).returncode == 0
    if ok:
        r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
        ok = (r.returncode, r.stdout, r.stderr) == (1, "error: cannot open the files\n", "")
    if not ok:
        subprocess.check_call(base)
    for w, h, tag, extra, n, data in _good_streams():
        open(path, "wb").write(data)
        r = subprocess.run([exe, path], capture_output=True, text=True, timeout=60)
        assert (r.returncode, r.stdout, r.stderr) == (0, "ok %d %d frames %d\n" % (w, h, n), ""), tag
    for name, data, word in _malformed():
        open(path, "wb").write(data)
        r = subprocess.run([exe, path], capture_output=True, text=True, timeout=60, errors="replace")
        assert r.returncode == 1 and r.stderr == "", (name, r)
        assert r.stdout.startswith("error: ") and r.stdout.count("\n") == 1 and word in r.stdout, (name, r.stdout)


# ------------------------------------------------------------ GPU: the kernels against the restatement

SIZES = [(1, 1), (2, 2), (3, 3), (17, 5), (64, 33), (131, 67)]
FAMILY = {"mono": ("mono", "mono%d"), "420jpeg": ("420jpeg", None), "420mpeg2": ("420mpeg2", "420p%d"),
          "422": ("422", "422p%d"), "444": ("444", "444p%d")}


def _format(family, depth, full_range, matrix):
    """the format of one of the five families at any depth (the 420jpeg siting has no tag above 8 bit)"""
    t8, tn = FAMILY[family]
    f = R.fmt(t8 if depth == 8 or tn is None else tn % depth, full_range, matrix)
    f.depth = depth
    return f


def _random_codes(rng, w, h, f):
    cw, chh = R.chroma_size(w, h, f)
    top = 1 << f.depth
    planes = [rng.integers(0, top, (h, w))] + ([] if f.mono else [rng.integers(0, top, (chh, cw)) for _ in range(2)])
    for p in planes:            # both ends of the code range are in every plane that has room for them
        p.flat[0] = top - 1
        p.flat[-1] = 0
    return R.join(planes[0], *(planes[1:] if len(planes) > 1 else (None, None)), f)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.gpu
@pytest.mark.parametrize("depth", [8, 10, 12, 16])
@pytest.mark.parametrize("family", list(FAMILY))
def test_gpu_kernels_equal_the_restatement_bit_for_bit(ctx, built, family, depth):
    rng = np.random.default_rng(1000 * depth + len(family))
    for full_range in (0, 1):
        for matrix in (601, 709):
            f = _format(family, depth, full_range, matrix)
            cf = c_fmt(built, f)
            for w, h in SIZES:
                what = (family, depth, full_range, matrix, w, h)
                codes = _random_codes(rng, w, h, f)
                got = ctx.yuv_to_rgb(codes, w, h, cf)
                want = R.to_rgb(codes, w, h, f)
                assert got.shape == want.shape and np.array_equal(_bits(got), _bits(want)), what
                rgb = rng.uniform(-20.0, 275.0, (h, w, 1 if f.mono else 3)).astype(np.float32)
                got = ctx.rgb_to_yuv(rgb, cf)
                want = R.to_yuv(rgb, f)
                assert got.dtype == np.uint8 and np.array_equal(got, want), what


@pytest.mark.gpu
@pytest.mark.parametrize("depth", [8, 10, 12, 16])
def test_gpu_444_there_and_back_is_the_identity(ctx, built, depth):
    rng = np.random.default_rng(depth)
    w = h = 256
    for full_range, matrix in ((0, 709), (1, 601)):
        f = _format("444", depth, full_range, matrix)
        cf = c_fmt(built, f)
        codes = _random_codes(rng, w, h, f)
        rgb = ctx.yuv_to_rgb(codes, w, h, cf)
        assert np.array_equal(ctx.rgb_to_yuv(rgb, cf), codes)
        # a NaN sample gives code 0 in its own pixel's three planes; no other code changes
        rgb[100, 37, 0] = np.nan
        Y, Cb, Cr = (p.copy() for p in R.split(codes, w, h, f))
        Y[100, 37] = Cb[100, 37] = Cr[100, 37] = 0
        assert np.array_equal(ctx.rgb_to_yuv(rgb, cf), R.join(Y, Cb, Cr, f))


@pytest.mark.gpu
def test_gpu_refused_calls_leave_the_context_working(ctx, built):
    w, h = 17, 5
    f = R.fmt("420jpeg", 0, 709)
    codes = _random_codes(np.random.default_rng(3), w, h, f)
    d_yuv, d_rgb = ctx.upload(codes), ctx.alloc(w * h * 3 * 4)
    try:
        def refused(call, *a):
            with pytest.raises(built.NlkError, match="rc=-3"):      # NLK_EINVAL
                call(*a)
        for field, bad in (("depth", 7), ("sx", 3), ("matrix", 2020)):
            g = c_fmt(built, f)
            setattr(g, field, bad)
            refused(ctx.yuv_to_rgb_dev, d_rgb, d_yuv, w, h, g)
            refused(ctx.rgb_to_yuv_dev, d_yuv, d_rgb, w, h, g)
        g = c_fmt(built, f)
        for a in ((d_rgb, d_yuv, 0, h, g), (d_rgb, d_yuv, w, -1, g), (None, d_yuv, w, h, g), (d_rgb, None, w, h, g)):
            refused(ctx.yuv_to_rgb_dev, *a)
        for a in ((d_yuv, d_rgb, 0, h, g), (None, d_rgb, w, h, g), (d_yuv, None, w, h, g)):
            refused(ctx.rgb_to_yuv_dev, *a)
        assert built.hip().nlk_dev_yuv_to_rgb(ctx.h, d_rgb, d_yuv, w, h, None) == -3
        # more rows than one launch covers (8 * 65535): NLK_EUNSUP before anything is launched
        assert built.hip().nlk_dev_yuv_to_rgb(ctx.h, d_rgb, d_yuv, 1, 8 * 65535 + 1, g) == -4
        assert built.hip().nlk_dev_rgb_to_yuv(ctx.h, d_yuv, d_rgb, 1, 8 * 65535 + 1, g) == -4
        assert np.array_equal(ctx.download(d_yuv, (len(codes),), np.uint8), codes)     # (nothing was written)
        ctx.yuv_to_rgb_dev(d_rgb, d_yuv, w, h, g)
        assert np.array_equal(_bits(ctx.download(d_rgb, (h, w, 3))), _bits(R.to_rgb(codes, w, h, f)))
    finally:
        ctx.free(d_yuv)
        ctx.free(d_rgb)


# ------------------------------------------------------------ GPU: the tool

def _there_and_back(payloads, w, h, f):
    return [R.to_yuv(R.to_rgb(p, w, h, f), f).tobytes() for p in payloads]


@pytest.mark.gpu
@pytest.mark.parametrize("w,h,tag,extra", [(95, 63, "420mpeg2", ""), (96, 64, "444p10", " XCOLORRANGE=FULL XA=b")])
def test_gpu_tool_copy_is_the_conversion_there_and_back(ctx, tool, tmp_path, w, h, tag, extra):
    f = R.fmt(tag, "FULL" in extra, 601)
    rng = np.random.default_rng(w)
    pay = [_random_codes(rng, w, h, f).tobytes() for _ in range(3)]
    data = R.y4m_bytes(w, h, tag, pay, extra)
    (tmp_path / "in.y4m").write_bytes(data)
    want = R.y4m_bytes(w, h, tag, _there_and_back(pay, w, h, f), extra)
    r = y4m("--copy", 0, tmp_path / "in.y4m", tmp_path / "out.y4m")
    assert (r.returncode, r.stdout, r.stderr) == (0, b"", b""), r
    assert (tmp_path / "out.y4m").read_bytes() == want
    r = y4m("--copy", 0, data=data)                            # stdin and stdout as pipes
    assert (r.returncode, r.stderr) == (0, b"") and r.stdout == want
    r = y4m("--copy", 0, "-", "-", data=data, env=dict(os.environ, NLK_SEQ_IO_THREADS="0"))   # in-line I/O
    assert (r.returncode, r.stderr) == (0, b"") and r.stdout == want


@pytest.fixture(scope="module")
def noisy(synth):
    """3 noisy frames (sigma 20) of 96 x 64 and of 95 x 63"""
    return {(w, h): [synth.awgn(synth.clean_frame(w, h, 3, t), 20.0, 100 + t) for t in range(3)]
            for (w, h) in ((96, 64), (95, 63))}


def _seq_reference(tmp_path, rgbs, sig, env):
    """nlkalman-seq on the RGB frames as PFM files, no smoother: (its stdout, the flt2 frames as float RGB)"""
    src, out = tmp_path / "in", tmp_path / "seq"
    src.mkdir(exist_ok=True)
    for t, a in enumerate(rgbs):
        wpfm(src / ("%03d.pfm" % (t + 1)), a)
    r = run("nlkalman-seq", src / "%03d.pfm", 1, len(rgbs), sig, out, 1, "", "no", env=env)
    assert r.returncode == 0, r.stderr
    flt2 = []
    for t in range(len(rgbs)):
        pfm = tmp_path / "conv.pfm"
        c = run("nlk-imgconv", out / ("flt2-%03d.tif" % (t + 1)), pfm)
        assert c.returncode == 0, c.stderr
        flt2.append(rpfm(pfm))
    return r.stdout, flt2


@pytest.mark.gpu
@pytest.mark.parametrize("w,h,tag", [(96, 64, "444"), (95, 63, "420jpeg")])
def test_gpu_tool_equals_nlkalman_seq_on_the_same_frames(ctx, tool, noisy, tmp_path, w, h, tag):
    """Both tools make the same calls on the same bits (NLK_DETERMINISTIC=1): the tool's frames are the codes of
    nlkalman-seq's flt2 files, exactly."""
    f = R.fmt(tag, 0, 601)                                     # (the tool's choice for a frame this small)
    pay = [R.to_yuv(a, f).tobytes() for a in noisy[(w, h)]]
    rgbs = [R.to_rgb(p, w, h, f) for p in pay]                 # what the filter sees (4:2:0: chroma interpolated)
    env = dict(os.environ, NLK_DETERMINISTIC="1")
    _, flt2 = _seq_reference(tmp_path, rgbs, 20, env)
    want = [R.to_yuv(a, f).tobytes() for a in flt2]
    data = R.y4m_bytes(w, h, tag, pay)
    r = y4m(20, data=data, env=env)
    assert r.returncode == 0, r.stderr
    line, w2, h2, tag2, got = R.y4m_parse(r.stdout)
    assert line == R.y4m_header(w, h, tag) and len(got) == 3
    for t in range(3):
        diff = np.frombuffer(got[t], np.uint8).astype(int) - np.frombuffer(want[t], np.uint8)
        print("frame %d: %d of %d codes differ, max %d" % (t + 1, np.count_nonzero(diff), diff.size, np.abs(diff).max()))
        assert got[t] == want[t], "frame %d" % (t + 1)
    assert got[0] != pay[0]                                    # (and it did filter)


@pytest.mark.gpu
def test_gpu_tool_sig_auto_vst_frames_and_truncation(ctx, tool, noisy, tmp_path):
    w, h, tag = 96, 64, "444"
    f = R.fmt(tag, 0, 601)
    pay = [R.to_yuv(a, f).tobytes() for a in noisy[(w, h)]]
    data = R.y4m_bytes(w, h, tag, pay)
    env = dict(os.environ, NLK_DETERMINISTIC="1")
    # SIG = auto: the sigma line (on stderr here) is nlkalman-seq's, and so are the frames
    stdout, flt2 = _seq_reference(tmp_path, [R.to_rgb(p, w, h, f) for p in pay], "auto", env)
    r = y4m("auto", data=data, env=env)
    assert r.returncode == 0, r.stderr
    lines = [l for l in r.stderr.decode().splitlines(True) if l.startswith("sigma ")]
    assert lines == [stdout] and stdout.startswith("sigma "), (lines, stdout)
    assert R.y4m_parse(r.stdout)[4] == [R.to_yuv(a, f).tobytes() for a in flt2]
    # SIG = vst:A,B runs; its line goes to stderr as well
    r = y4m("vst:0.5,4", data=data, env=env)
    assert r.returncode == 0 and r.stderr.startswith(b"vst 0.5 4 0.5 4 0.5 4 sigma "), r.stderr
    assert len(R.y4m_parse(r.stdout)[4]) == 3
    # --frames 2
    r2 = y4m("--frames", 2, 20, data=data, env=env)
    assert r2.returncode == 0, r2.stderr
    two = R.y4m_parse(r2.stdout)[4]
    assert len(two) == 2
    # a stream cut in the middle of frame 3: status 1, the two complete frames filtered and written, the message
    cut = data[:len(data) - len(pay[2]) // 2]
    r3 = y4m(20, data=cut, env=env)
    assert r3.returncode == 1
    assert r3.stderr.decode().count("\n") == 1 and b"frame 3: the stream ends inside a frame" in r3.stderr, r3.stderr
    assert R.y4m_parse(r3.stdout)[4] == two
