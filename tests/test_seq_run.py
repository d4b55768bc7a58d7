"""The run of the sequence tools (host/seq_step.h: struct seq_opts, seq_opts_read, struct seq_run and its steps).

CPU: the one reader of the options all four tools share, host/seq_args.c, as a stand-alone program
(tests/seq_opts_driver.c, plain and under the sanitizers): every accepted and refused value of tests/test_despike.py and
tests/test_defect_map.py, a missing value, names that are no shared option, and the walk in the table's order that
main_seq.c makes: consumed counts, values and the exact stderr lines.
GPU: every shared option at once, 4 frames of 48 x 40 x 3 (8 x 8 patches, ring radius 2, a two-level flow pyramid;
seeded noise and a few stuck sites, as a 4:4:4 stream holds them): nlkalman-seq, nlkalman-lsmo-seq --flow inv,
nlkalman-seq-gt --ssim and nlkalman-y4m --smooth inv against SequenceFilter with the same arguments, bit for bit, and
one run with no option at all."""
import importlib
import os
import subprocess

import numpy as np
import pytest

import despike_ref as DR
import yuv_ref
from test_cli import BIN, rpfm, wpfm
from test_defect_map import ACCEPTED as DEFECT_OK, REFUSED as DEFECT_BAD, WANT as DEFECT_WANT, _drivers, run
from test_despike import ACCEPTED as DESPIKE_OK, REFUSED as DESPIKE_BAD, WANT as DESPIKE_WANT

F32 = np.float32
OF_WANT = "%s: --of %s: want tvl1 or bm\n"


def _bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


# ---------------------------------------------------------------- the option reader, as a program

def _line(reads, stop, of=0, despike=(0.0, 0), defect=(0.0, 0, 0), sure=0):
    return "read %s stop %d of %d despike %.9g %d defect %.9g %d %d sure %d" % (
        " ".join(map(str, reads)), stop, of, despike[0], despike[1], *defect, sure)


def _vectors():
    """(mode, arguments, the driver's stdout line, the stderr line or None)"""
    v = []
    for mode in ("order", "any"):
        tail = [0]   # the call that ends the walk: nothing left (any), or not a row that is left (order)
        for text, of in (("tvl1", 0), ("bm", 1)):
            v.append((mode, ["--of", text], _line([2] + tail, 2, of=of), None))
        for text in ("", "x", "TVL1", "bm ", "tvl1,bm"):
            v.append((mode, ["--of", text], _line([-1], 0), OF_WANT % ("prog", text)))
        for text, (k, r) in DESPIKE_OK.items():
            v.append((mode, ["--despike", text], _line([2] + tail, 2, despike=(k, r)), None))
        for text in DESPIKE_BAD:
            v.append((mode, ["--despike", text], _line([-1], 0), DESPIKE_WANT % ("prog", text)))
        for text, (k, r, n) in DEFECT_OK.items():
            v.append((mode, ["--defect-map", text], _line([2] + tail, 2, defect=(k, r, n)), None))
        for text in DEFECT_BAD:
            v.append((mode, ["--defect-map", text], _line([-1], 0), DEFECT_WANT % ("prog", text)))
        v.append((mode, ["--sure"], _line([1] + tail, 1, sure=1), None))
        # a missing value: the option's line with an empty text
        for name, want in (("--of", OF_WANT), ("--despike", DESPIKE_WANT), ("--defect-map", DEFECT_WANT)):
            v.append((mode, [name], _line([-1], 0), want % ("prog", "")))
        v.append((mode, ["--of", "bm", "--despike"], _line([2, -1], 2, of=1), DESPIKE_WANT % ("prog", "")))
        v.append((mode, [], _line([0], 0), None))
        # everything, in the table's order; what follows is the tool's
        v.append((mode, ["--of", "bm", "--despike", "4,2", "--defect-map", "4,1,8", "--sure"],
                  _line([2, 2, 2, 1, 0], 7, of=1, despike=(4.0, 2), defect=(4.0, 1, 8), sure=1), None))
        # a refused value leaves what the options before it set, and its own fields as they were
        v.append((mode, ["--despike", "3", "--defect-map", "4,1,1", "--sure"], _line([2, -1], 2, despike=(3.0, 1)),
                  DEFECT_WANT % ("prog", "4,1,1")))
    # names that are no shared option: main_seq.c's walk stops there, main_y4m.c's loop steps over them
    for name in ("--flow", "--ssim", "--despik", "--despike=4", "-sure", "--sure ", "--SURE", "20", "in/%03d.tif", ""):
        v.append(("order", [name, "--sure"], _line([0], 0), None))
        v.append(("any", [name, "--sure"], _line([0, 1, 0], 2, sure=1), None))
    # the fixed order of main_seq.c: an option behind its place is left unread ...
    v.append(("order", ["--sure", "--despike", "4"], _line([1, 0], 1, sure=1), None))
    v.append(("order", ["--despike", "4", "--of", "bm"], _line([2, 0], 2, despike=(4.0, 1)), None))
    v.append(("order", ["--defect-map", "4", "--despike", "4", "--sure"], _line([2, 0], 2, defect=(4.0, 1, 32)), None))
    v.append(("order", ["--of", "bm", "--of", "tvl1"], _line([2, 0], 2, of=1), None))
    v.append(("order", ["--sure", "--sure"], _line([1, 0], 1, sure=1), None))
    v.append(("order", ["--despike", "4", "--sure", "SEQ", "--of", "x"], _line([2, 1, 0], 3, despike=(4.0, 1), sure=1), None))
    # ... (its value is not looked at either) and main_y4m.c's loop reads it wherever it stands, the last one winning
    v.append(("order", ["--sure", "--despike", "0"], _line([1, 0], 1, sure=1), None))
    v.append(("any", ["--sure", "--despike", "4"], _line([1, 2, 0], 3, despike=(4.0, 1), sure=1), None))
    v.append(("any", ["--despike", "4", "--copy", "--of", "bm", "20", "--of", "tvl1", "--defect-map", "2.5,2"],
              _line([2, 0, 2, 0, 2, 2, 0], 10, despike=(4.0, 1), defect=(2.5, 2, 32)), None))
    v.append(("any", ["20", "--sure", "--of", "x", "--despike", "4"], _line([0, 1, -1], 2, sure=1), OF_WANT % ("prog", "x")))
    return v


@pytest.fixture(scope="module")
def opts_drivers(tmp_path_factory):
    return _drivers(tmp_path_factory.mktemp("seq_opts_driver"), "seq_opts_driver", ["seq_args.c"])


def test_option_reader_counts_values_and_lines(opts_drivers):
    vectors = _vectors()
    assert len(vectors) > 120
    argv = []
    for mode, args, _, _ in vectors:
        argv += ["//"] * bool(argv) + [mode, *args]
    for exe in opts_drivers:
        r = subprocess.run([exe, *argv], capture_output=True, text=True, timeout=60)
        assert r.returncode == 0, (exe, r)
        lines = r.stdout.splitlines()
        assert len(lines) == len(vectors), (exe, r)
        for (mode, args, want, _), line in zip(vectors, lines):
            assert line == want, (exe, mode, args)
        assert r.stderr == "".join(err for _, _, _, err in vectors if err), exe
        names = ["--of", "--despike", "--defect-map", "--sure", "--flow", "--ssim", "--smooth", "--sur", "", "20", "-v"]
        r = subprocess.run([exe, "arity", *names], capture_output=True, text=True, timeout=60)
        assert (r.returncode, r.stdout, r.stderr) == (0, "2 2 2 1 0 0 0 0 0 0 0\n", ""), (exe, r)


# ---------------------------------------------------------------- every shared option at once

W, H, NF, NOISE = 48, 40, 4, 8.0
VST = (0.5, 4.0)                   # SIG = vst:0.5,4: var = 0.5 y + 4, about NOISE^2 in the middle of the range
OPTS = ["--of", "bm", "--despike", "4,2", "--defect-map", "4,1,8", "--sure"]
SF_OPTS = dict(of="bm", despike=(4, 2), defect_map=(4, 1, 8), sure=True)
SITES = [(0, 0, 255.0), (47, 17, 0.0), (20, 39, 255.0), (13, 11, 255.0), (30, 25, 0.0), (40, 6, 255.0)]
FMT = yuv_ref.fmt("444", 0, 601)


def _decode(path):
    r = run("nlk-imgconv", path, str(path) + ".pfm")
    assert r.returncode == 0, r.stderr
    return rpfm(str(path) + ".pfm")


def _tifs(folder, frames):
    folder.mkdir()
    for t, a in enumerate(frames):
        wpfm(folder / "tmp.pfm", a)
        r = run("nlk-imgconv", folder / "tmp.pfm", folder / ("%03d.tif" % (t + 1)))
        assert r.returncode == 0, r.stderr
    return folder / "%03d.tif"


def _reference(ctx, frames, sigma, **kw):
    """SequenceFilter on the frames: per frame flt1, flt2 (RGB, as the tools write them) and lsm1 of the frame before
    (lag1="inv"), then the backward pass, and the filter itself (its .sure, .sigma)"""
    seq = importlib.import_module("bwd-nlkalman_amd.sequence")
    ctx.set_deterministic(True)
    try:
        sf = seq.SequenceFilter(ctx, W, H, 3, sigma, lag1="inv", **kw)
        flt1, flt2, lsm1 = [], [], []
        for a in frames:
            d = ctx.upload(a)
            sf.push(d)
            ctx.free(d)
            flt1.append(sf.download_rgb(sf.flt1))
            flt2.append(sf.download_rgb(sf.flt2))
            if sf.lsm1 is not None:
                lsm1.append(sf.download_rgb(sf.lsm1))
        lsm1.append(flt2[-1])   # the last frame's lsm1 is its flt2
        smo1 = [sf.download_rgb(d) for d in sf.smooth()]
    finally:
        ctx.set_deterministic(False)
    return dict(flt1=flt1, flt2=flt2, lsm1=lsm1, smo1=smo1, sf=sf)


@pytest.fixture(scope="module")
def scene(ctx, built, synth, tmp_path_factory):
    """the frames (what a 4:4:4 stream of the noisy frames with the stuck sites decodes to), their float TIFF files, the
    clean frames' files, and the three references, each computed once"""
    if not all(os.path.exists(os.path.join(BIN, t)) for t in
               ("nlkalman-seq", "nlkalman-seq-gt", "nlkalman-lsmo-seq", "nlkalman-y4m", "nlk-imgconv")):
        built.build()
    base = tmp_path_factory.mktemp("seq_run")
    clean = [synth.clean_frame(W, H, 3, t) for t in range(NF)]
    pay = [yuv_ref.to_yuv(DR.plant(synth.awgn(c, NOISE, 700 + t), SITES), FMT).tobytes() for t, c in enumerate(clean)]
    frames = [yuv_ref.to_rgb(p, W, H, FMT) for p in pay]
    s = dict(base=base, clean=clean, pay=pay, frames=frames, src=_tifs(base / "in", frames),
             clean_src=_tifs(base / "clean", clean), env=dict(os.environ, NLK_DETERMINISTIC="1"))
    s["all"] = _reference(ctx, frames, ("vst", *VST), **SF_OPTS)
    s["none"] = _reference(ctx, frames, NOISE)
    s["number"] = _reference(ctx, frames, NOISE, **SF_OPTS)
    # the options do something on these frames: each of them alone moves flt2 of the last frame
    for key in ("of", "despike", "defect_map"):
        one = _reference(ctx, frames, NOISE, **{key: SF_OPTS[key]})
        assert not np.array_equal(_bits(one["flt2"][-1]), _bits(s["none"]["flt2"][-1])), key
    return s


def _same_files(out, ref, kinds, what):
    for kind in kinds:
        for t in range(NF):
            got = _decode(out / ("%s-%03d.tif" % (kind, t + 1)))
            assert np.array_equal(_bits(got), _bits(ref[kind][t])), (what, kind, t + 1)


def _sure_lines(sf, label, which):
    return ["%s %d %.9g %.9g %.9g %.9g" % (label, t + 1, *(float(which(s)[k]) for k in ("mse", "psnr", "resid", "div")))
            for t, s in enumerate(sf.sure)]


def _same_measures_sure(path, sf):
    """measures-sure against SequenceFilter.sure, to the printed digits ("%.9g": 5e-9 relative)"""
    rows = [ln.split() for ln in open(path).read().splitlines()]
    assert len(rows) == 2 * (NF + 1) and all(len(r) == 6 for r in rows), rows
    for p, (label, which) in enumerate((("F1", lambda s: s["flt1"]), ("F2", lambda s: s))):
        part = rows[p * (NF + 1):(p + 1) * (NF + 1)]
        assert [r[:2] for r in part] == [[label, str(t + 1)] for t in range(NF)] + [[label, "total"]]
        got = np.array([[float(x) for x in r[2:]] for r in part[:NF]])
        want = np.array([[which(s)[k] for k in ("mse", "psnr", "resid", "div")] for s in sf.sure])
        # (a frame of this size is a coarse instrument: an MSE_hat below 0 has no PSNR, "nan" on both sides)
        assert np.allclose(got, want, rtol=2e-8, atol=0, equal_nan=True), (label, got, want)
        assert np.isfinite(got[:, [0, 2, 3]]).all() and (got[:, 2] > 0).all(), (label, got)
        assert abs(float(part[NF][2]) - want[:, 0].mean()) <= 1e-8 * abs(want[:, 0]).mean(), label


@pytest.mark.gpu
def test_gpu_seq_with_every_option_is_the_sequence_filter(scene):
    out = scene["base"] / "seq_all"
    r = run("nlkalman-seq", *OPTS, scene["src"], 1, NF, "vst:%g,%g" % VST, out, env=scene["env"])
    sf = scene["all"]["sf"]
    assert r.returncode == 0 and r.stderr == "", r
    assert r.stdout == "vst" + " 0.5 4" * 3 + " sigma %.9g\n" % sf.sigma
    assert sorted(os.listdir(out)) == sorted(
        ["%s-%03d.tif" % (k, t) for k in ("flt1", "flt2", "smo1") for t in range(1, NF + 1)] + ["measures-sure"] +
        ["%s-%03d.%s" % (k, t, e) for k, e in (("bflo1", "flo"), ("bocc1", "png")) for t in range(2, NF + 1)] +
        ["%s-%03d.%s" % (k, t, e) for k, e in (("fflo", "flo"), ("focc", "png")) for t in range(1, NF)])
    _same_files(out, scene["all"], ("flt1", "flt2", "smo1"), "nlkalman-seq, every option")
    _same_measures_sure(out / "measures-sure", sf)


@pytest.mark.gpu
def test_gpu_seq_without_any_option_is_the_sequence_filter(scene):
    out = scene["base"] / "seq_none"
    r = run("nlkalman-seq", scene["src"], 1, NF, NOISE, out, env=scene["env"])
    assert (r.returncode, r.stdout, r.stderr) == (0, "", ""), r
    _same_files(out, scene["none"], ("flt1", "flt2", "smo1"), "nlkalman-seq, no option")
    assert "measures-sure" not in os.listdir(out)
    # ... and the options make a difference on these frames
    assert not np.array_equal(_bits(scene["none"]["flt2"][-1]), _bits(scene["number"]["flt2"][-1]))


@pytest.mark.gpu
def test_gpu_lsmo_and_y4m_with_every_option_are_the_sequence_filter(scene):
    out = scene["base"] / "lsmo_all"
    r = run("nlkalman-lsmo-seq", *OPTS, "--flow", "inv", scene["src"], 1, NF, "vst:%g,%g" % VST, out, env=scene["env"])
    sf = scene["all"]["sf"]
    assert r.returncode == 0 and r.stderr == "", r
    assert r.stdout == "vst" + " 0.5 4" * 3 + " sigma %.9g\n" % sf.sigma
    _same_files(out, scene["all"], ("flt1", "flt2", "lsm1"), "nlkalman-lsmo-seq, every option")
    _same_measures_sure(out / "measures-sure", sf)
    # the stream tool, the options in another order: the stream made from those lsm1 frames, and flt2's estimates
    y = run("nlkalman-y4m", "--sure", "--smooth", "inv", "--defect-map", "4,1,8", "--despike", "4,2", "--of", "bm",
            "vst:%g,%g" % VST, input=yuv_ref.y4m_bytes(W, H, "444", scene["pay"]), env=scene["env"], text=False)
    assert y.returncode == 0, y.stderr
    want = [yuv_ref.to_yuv(_decode(out / ("lsm1-%03d.tif" % (t + 1))), FMT).tobytes() for t in range(NF)]
    assert yuv_ref.y4m_parse(y.stdout)[4] == want
    f2 = [ln.replace("F2", "sure", 1) for ln in open(out / "measures-sure").read().splitlines() if ln.startswith("F2 ")]
    err = y.stderr.decode().splitlines()
    assert err[:-1] == [r.stdout.rstrip("\n")] + f2[:-1]
    # (the two tools add the total up in two ways: the same value to the printed digits)
    assert err[-1].split()[:2] == ["sure", "total"] and len(err[-1].split()) == 6
    assert np.allclose([float(x) for x in err[-1].split()[2:]], [float(x) for x in f2[-1].split()[2:]], rtol=2e-8, atol=0,
                       equal_nan=True)


@pytest.mark.gpu
def test_gpu_seq_gt_with_every_option_and_ssim(scene):
    """a numeric SIG; the noisy files exist, so the tool reads them: its measures are those of SequenceFilter's frames
    against the clean ones (the MSE lines go through six-digit text, `%g`: 1e-5 relative)"""
    out = scene["base"] / "gt_all"
    out.mkdir()
    for t in range(1, NF + 1):
        (out / ("%03d.tif" % t)).write_bytes((scene["base"] / "in" / ("%03d.tif" % t)).read_bytes())
    r = run("nlkalman-seq-gt", *OPTS, "--ssim", scene["clean_src"], 1, NF, NOISE, out, "", "no", env=scene["env"])
    assert r.returncode == 0 and r.stderr == "", r
    lines = r.stdout.splitlines()
    assert len(lines) == 3 and lines[1].startswith("ssim ") and lines[2].startswith("sure "), lines
    ref = scene["number"]
    _same_measures_sure(out / "measures-sure", ref["sf"])
    for p, kind in enumerate(("flt1", "flt2")):
        mse = np.mean([np.mean((a.astype(np.float64) - c) ** 2) for a, c in zip(ref[kind], scene["clean"])])
        assert abs(float(lines[0].split()[p]) - mse) <= 1e-5 * mse, (kind, lines[0], mse)
        assert 0.0 < float(lines[1].split()[1 + p]) < 1.0
    assert {"measures", "measures-ssim", "measures-sure", "flt2-%03d.png" % NF} <= set(os.listdir(out))
