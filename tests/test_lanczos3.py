"""Lanczos-3 pyramid of the lz3 multiscale pipeline (scripts/msnlkalman-lz3-seq.sh; the reference's
lib/ms-lanczos3 Octave tools): the C-ABI (nlk_dev_lz3_*), the Python conveniences and the two tools
bin/lanczos3_decompose and bin/lanczos3_recompose.

Parity here is "HIP = our restatement of the spec" (tests/lz3_ref.py, float64, written from the formulas of
DESIGN.md §9), like the DCT multiscale wrapper's: Octave is not available, so nothing is pinned to the
reference's own output. The CPU tests check the restatement's mathematical properties and the tools' command
line; the GPU tests compare the kernels and the tools' files with it."""
import os
import subprocess
import time

import numpy as np
import pytest

import lz3_ref as R
from test_cli import rpfm, server, sock_dir, wpfm  # noqa: F401  (sock_dir: a fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "bwd-nlkalman_amd", "bin")
TOOLS = ("lanczos3_decompose", "lanczos3_recompose")
USAGE = {"lanczos3_decompose": "Usage: lanczos3_decompose.m input prefix levels suffix",
         "lanczos3_recompose": "Usage: lanczos3_recompose.m input prefix levels suffix [factor]"}
GPU_STEP_S = 300   # time limit of one tool run on the GPU


def run(tool, *args, **kw):
    kw.setdefault("timeout", GPU_STEP_S)
    exe = tool if os.sep in tool else os.path.join(BIN, tool)
    return subprocess.run([exe, *map(str, args)], capture_output=True, text=True, **kw)


@pytest.fixture(scope="module")
def lz3_tools(built):
    if not all(os.path.exists(os.path.join(BIN, t)) for t in TOOLS + ("nlk-imgconv",)):
        built.build()
    return BIN


def _img(w, h, ch, seed):
    """0..255 data with structure and noise"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    base = 128 + 80 * np.sin(0.17 * x + 0.05 * y) * np.cos(0.09 * x - 0.21 * y)
    return np.clip(base[..., None] + rng.normal(0, 20, (h, w, ch)), 0, 255).astype(np.float32)


# ------------------------------------------------------------ CPU: the restatement

def test_taps_sum_to_one():
    ke, ko = R.up_taps()
    for t in (R.down_taps(), ke, ko, R.gauss_taps(0.7)[0], R.gauss_taps(2.5)[0], R.gauss_taps(3.5)[0]):
        assert abs(t.sum() - 1) < 1e-14
    k = R.down_taps()
    assert np.allclose(k[:6], [0.003689, 0.015056, -0.033999, -0.066637, 0.135505, 0.446385], atol=1e-6)
    assert np.array_equal(k, k[::-1])
    assert len(R.gauss_taps(0.7)[0]) == 5 and len(R.gauss_taps(3.5)[0]) == 6 and R.gauss_taps(3.5)[1] == 2


@pytest.mark.parametrize("h,w", [(1, 1), (1, 9), (9, 1), (13, 22), (40, 33)])
def test_constant_is_a_fixed_point_and_sizes(h, w):
    c = np.full((h, w, 2), 37.25)
    d = R.down(c)
    assert d.shape == ((h + 1) // 2, (w + 1) // 2, 2) and np.abs(d - 37.25).max() < 1e-12
    for fh in (-1, 0, 1):
        for fw in (-1, 0, 1):
            size = (max(2 * h + fh, 1), max(2 * w + fw, 1))
            u = R.up(c, size)
            assert u.shape == size + (2,) and np.abs(u - 37.25).max() < 1e-12
    for g in (0.7, 2.5, 3.5):
        assert np.abs(R.gblur(c, g) - 37.25).max() < 1e-12


def test_gblur_mirror_on_tiny_axes():
    t, a = R.gauss_taps(0.7)
    assert a == 2
    x = np.array([[[5.0]]])
    assert np.allclose(R.gblur(x, 0.7), 5.0)
    # n = 2: x[-2] = x[1], x[-1] = x[0], x[2] = x[1], x[3] = x[0]
    x2 = np.array([3.0, 11.0]).reshape(1, 2, 1)
    got = R.gblur(x2, 0.7)[0, :, 0]
    want0 = t[0] * 11 + t[1] * 3 + t[2] * 3 + t[3] * 11 + t[4] * 11
    want1 = t[0] * 3 + t[1] * 3 + t[2] * 11 + t[3] * 11 + t[4] * 3
    assert np.allclose(got, [want0, want1], atol=1e-12)
    assert np.allclose(R.gblur(x2.reshape(2, 1, 1), 0.7)[:, 0, 0], [want0, want1], atol=1e-12)


def test_offset_on_the_coarsest_level_moves_the_result():
    a = _img(45, 31, 3, 2).astype(np.float64)
    lv = R.decompose(a, 4)
    assert [x.shape[:2] for x in lv] == [(31, 45), (16, 23), (8, 12), (4, 6)]
    assert np.abs(R.recompose(lv, 0.7) - a).max() < 1e-9
    lv[-1] = lv[-1] + 10
    r = R.recompose(lv, 0.7)
    assert abs((r - a).mean() - 10) < 1e-9 and np.abs(r - a - 10).max() < 1e-9


# ------------------------------------------------------------ CPU: the tools' command line

@pytest.mark.parametrize("tool", TOOLS)
def test_tools_usage_and_errors(lz3_tools, tool, tmp_path):
    for args in ([], ["a"], ["a", "b", "3"]):
        r = run(tool, *args, cwd=tmp_path)
        assert (r.returncode, r.stdout, r.stderr) == (0, USAGE[tool] + "\n", ""), args
    # the name the pipeline calls it by: $DIR/../../lib/ms-lanczos3/<tool>.m
    link = tmp_path / (tool + ".m")
    os.symlink(os.path.join(BIN, tool), link)
    r = run(str(link), cwd=tmp_path)
    assert (r.returncode, r.stdout) == (0, USAGE[tool] + "\n")
    if tool == "lanczos3_decompose":
        r = run(str(link), "missing.tif", "ms", 3, ".tif", cwd=tmp_path)
        assert r.returncode == 1 and "missing.tif" in r.stderr and not os.path.exists(tmp_path / "ms0.tif")
        wpfm(tmp_path / "in.pfm", _img(8, 6, 3, 0))
        r = run(tool, "in.pfm", "ms", "three", ".tif", cwd=tmp_path)
        assert r.returncode == 1 and "three" in r.stderr
    else:
        r = run(str(link), "out.tif", "ms", 3, ".tif", cwd=tmp_path)       # level 0 is missing
        assert r.returncode == 1 and "ms0.tif" in r.stderr and not os.path.exists(tmp_path / "out.tif")
        r = run(tool, "out.tif", "ms", "x", ".tif", cwd=tmp_path)
        assert r.returncode == 1 and "x" in r.stderr
        wpfm(tmp_path / "ms0.pfm", _img(8, 6, 3, 0))
        r = run(tool, "out.pfm", "ms", 3, ".pfm", "0.7abc", cwd=tmp_path)
        assert r.returncode == 1 and "0.7abc" in r.stderr and not os.path.exists(tmp_path / "out.pfm")


# ------------------------------------------------------------ GPU: the C-ABI

SIZES = [(1, 1), (1, 9), (9, 1), (22, 13), (333, 190), (1920, 1080)]


def _assert_close(got, want, tol, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    err = float(np.abs(got.astype(np.float64) - want).max())
    assert np.isfinite(got).all() and err <= tol, (what, err)


@pytest.mark.gpu
@pytest.mark.parametrize("ch", [1, 3, 4])
@pytest.mark.parametrize("w,h", SIZES)
def test_gpu_down_and_up_vs_ref(ctx, w, h, ch):
    a = _img(w, h, ch, w * 7 + h + ch)
    d = ctx.upload(a)
    dw, dh = (w + 1) // 2, (h + 1) // 2
    out = ctx.alloc(dw * dh * ch * 4)
    ctx.lz3_down(out, d, w, h, ch)
    _assert_close(ctx.download(out, (dh, dw, ch)), R.down(a), 2e-3, ("down", w, h, ch))
    ctx.free(out)
    for fit in (-1, 0, 1):            # 2n - 1, 2n, 2n + 1
        uw, uh = 2 * w + fit, 2 * h + fit
        out = ctx.alloc(uw * uh * ch * 4)
        ctx.lz3_up(out, uw, uh, d, w, h, ch)
        _assert_close(ctx.download(out, (uh, uw, ch)), R.up(a, (uh, uw)), 2e-3, ("up", w, h, ch, fit))
        ctx.free(out)
    # mixed fits, and sizes the up refuses
    out = ctx.alloc((2 * w + 1) * (2 * h + 1) * ch * 4)
    ctx.lz3_up(out, 2 * w + 1, 2 * h, d, w, h, ch)
    _assert_close(ctx.download(out, (2 * h, 2 * w + 1, ch)), R.up(a, (2 * h, 2 * w + 1)), 2e-3, ("up mixed", w, h))
    pkg = __import__("importlib").import_module("bwd-nlkalman_amd")
    with pytest.raises(pkg.NlkError):
        ctx.lz3_up(out, 2 * w + 2, 2 * h, d, w, h, ch)
    ctx.free(out)
    ctx.free(d)


@pytest.mark.gpu
@pytest.mark.parametrize("g", [0.0, 0.7, 2.5, 3.5, 12.0])
@pytest.mark.parametrize("w,h,ch", [(1, 1, 3), (9, 1, 1), (22, 13, 3), (333, 190, 4), (1920, 1080, 3)])
def test_gpu_recompose_step_vs_ref(ctx, w, h, ch, g):
    """one level: out = yh + up(gblur(rl - down(yh), g)), with an rl that differs from down(yh); g = 3.5 is an
    even-length Gaussian (the imfilter anchor), g = 12 one that needs fewer channels per workgroup"""
    yh = _img(w, h, ch, 11 * w + h)
    wl, hl = (w + 1) // 2, (h + 1) // 2
    rl = (R.down(yh) + np.random.default_rng(5).normal(0, 6, (hl, wl, ch))).astype(np.float32)
    d_y, d_r = ctx.upload(yh), ctx.upload(rl)
    out = ctx.alloc(w * h * ch * 4)
    ctx.lz3_recompose_step(out, d_y, w, h, d_r, wl, hl, ch, g)
    _assert_close(ctx.download(out, (h, w, ch)), R.recompose_step(yh, rl, g), 2e-3, ("step", w, h, ch, g))
    # in place over yh (what the tool does)
    ctx.lz3_recompose_step(d_y, d_y, w, h, d_r, wl, hl, ch, g)
    assert np.array_equal(ctx.download(d_y, (h, w, ch)), ctx.download(out, (h, w, ch)))
    for d in (d_y, d_r, out):
        ctx.free(d)


@pytest.mark.gpu
@pytest.mark.parametrize("w,h,ch,levels", [(333, 190, 3, 4), (22, 13, 1, 5), (1, 9, 4, 5), (1920, 1080, 3, 3)])
def test_gpu_recompose_of_decompose_is_the_input_bit_for_bit(ctx, w, h, ch, levels):
    a = _img(w, h, ch, levels + w)
    d = ctx.upload(a)
    lv = ctx.lz3_decompose(d, w, h, ch, levels)
    assert [(lw, lh) for _, lw, lh in lv] == [(x.shape[1], x.shape[0]) for x in R.decompose(a, levels)]
    for (p, lw, lh), want in zip(lv, R.decompose(a, levels)):
        _assert_close(ctx.download(p, (lh, lw, ch)), want, 2e-3, ("level", lw, lh))
    for g in (0.0, 0.7, 2.5):
        r = ctx.lz3_recompose(lv, g)
        got = ctx.download(r, (h, w, ch))
        assert np.array_equal(got, a), (g, float(np.abs(got - a).max()))
        ctx.free(r)
    # a changed coarse level shows up as the reference recompose says, and twice the same
    lv2 = type(lv)(lv)
    lv2.ch = ch
    coarse = ctx.download(lv[-1][0], (lv[-1][2], lv[-1][1], ch)) + 10
    lv2[-1] = (ctx.upload(coarse), lv[-1][1], lv[-1][2])
    want = R.recompose([ctx.download(p, (lh, lw, ch)) for p, lw, lh in lv[:-1]] + [coarse], 0.7)
    r1, r2 = ctx.lz3_recompose(lv2, 0.7), ctx.lz3_recompose(lv2, 0.7)
    g1, g2 = ctx.download(r1, (h, w, ch)), ctx.download(r2, (h, w, ch))
    _assert_close(g1, want, 3e-3, "offset recompose")
    assert np.array_equal(g1, g2)
    for p in [r1, r2, lv2[-1][0]] + [p for p, _, _ in lv]:
        ctx.free(p)


@pytest.mark.gpu
def test_gpu_runs_are_bit_identical(ctx):
    w, h, ch = 517, 301, 3
    a = _img(w, h, ch, 9)
    rl = (R.down(a) + 3 * np.sin(np.arange(151 * 259 * 3)).reshape(151, 259, 3)).astype(np.float32)
    d_a, d_r = ctx.upload(a), ctx.upload(rl)
    outs = []
    for _ in range(2):
        o = ctx.alloc(w * h * ch * 4)
        dn = ctx.alloc(259 * 151 * ch * 4)
        up = ctx.alloc(1035 * 603 * ch * 4)
        ctx.lz3_recompose_step(o, d_a, w, h, d_r, 259, 151, ch, 0.7)
        ctx.lz3_down(dn, d_a, w, h, ch)
        ctx.lz3_up(up, 1035, 603, d_a, w, h, ch)
        outs.append([ctx.download(o, (h, w, ch)), ctx.download(dn, (151, 259, ch)), ctx.download(up, (603, 1035, ch))])
        for p in (o, dn, up):
            ctx.free(p)
    for x, y in zip(*outs):
        assert np.array_equal(x, y)
    ctx.free(d_a)
    ctx.free(d_r)


# ------------------------------------------------------------ GPU: the tools

def _to_pfm(tmp_path, f):
    r = run("nlk-imgconv", tmp_path / f, tmp_path / (f + ".pfm"))
    assert r.returncode == 0, r.stderr
    return rpfm(tmp_path / (f + ".pfm"))


def _write_tif(tmp_path, name, a):
    wpfm(tmp_path / (name + ".pfm"), a)
    r = run("nlk-imgconv", tmp_path / (name + ".pfm"), tmp_path / name)
    assert r.returncode == 0, r.stderr


@pytest.mark.gpu
def test_tools_pyramid_files(lz3_tools, tmp_path):
    """decompose / recompose the way scripts/msnlkalman-lz3-seq.sh calls them: prefix `ms`, suffix `-007.tif`,
    3 levels, recompose with 0.7; float TIFF files"""
    a = _img(161, 97, 3, 4)
    _write_tif(tmp_path, "in.tif", a)
    r = run("lanczos3_decompose", tmp_path / "in.tif", tmp_path / "ms", 3, "-007.tif")
    assert r.returncode == 0, r.stderr
    want = R.decompose(a, 3)
    got = [_to_pfm(tmp_path, f"ms{i}-007.tif") for i in range(3)]
    assert not os.path.exists(tmp_path / "ms3-007.tif")
    for i, (gv, wv) in enumerate(zip(got, want)):
        _assert_close(gv, wv, 2e-3, ("level", i))
    assert np.array_equal(got[0], a)
    # recompose(decompose(x)) == x, through the files
    r = run("lanczos3_recompose", tmp_path / "out.tif", tmp_path / "ms", 3, "-007.tif", 0.7, "ignored")
    assert r.returncode == 0, r.stderr
    assert np.array_equal(_to_pfm(tmp_path, "out.tif"), a)
    # with filtered-looking levels: against the restatement, 3e-3
    lv = [np.clip(x + np.random.default_rng(i).normal(0, 4, x.shape), 0, 255).astype(np.float32) for i, x in enumerate(got)]
    for i, x in enumerate(lv):
        _write_tif(tmp_path, f"ms{i}-flt1-007.tif", x)
    r = run("lanczos3_recompose", tmp_path / "flt1-007.tif", tmp_path / "ms", 3, "-flt1-007.tif", 0.7)
    assert r.returncode == 0, r.stderr
    rec = _to_pfm(tmp_path, "flt1-007.tif")
    _assert_close(rec, R.recompose(lv, 0.7), 3e-3, "recompose")
    # the default factor is 0
    r = run("lanczos3_recompose", tmp_path / "g0.tif", tmp_path / "ms", 3, "-flt1-007.tif")
    assert r.returncode == 0, r.stderr
    _assert_close(_to_pfm(tmp_path, "g0.tif"), R.recompose(lv, 0.0), 3e-3, "recompose g = 0")
    # twice the same bytes
    r = run("lanczos3_recompose", tmp_path / "again.tif", tmp_path / "ms", 3, "-flt1-007.tif", 0.7)
    assert r.returncode == 0, r.stderr
    assert open(tmp_path / "again.tif", "rb").read() == open(tmp_path / "flt1-007.tif", "rb").read()
    # the recompose stops at the first missing level: 5 levels asked, 0..2 there = 3 levels
    r = run("lanczos3_recompose", tmp_path / "five.tif", tmp_path / "ms", 5, "-flt1-007.tif", 0.7)
    assert r.returncode == 0, r.stderr
    assert open(tmp_path / "five.tif", "rb").read() == open(tmp_path / "flt1-007.tif", "rb").read()
    os.remove(tmp_path / "ms2-flt1-007.tif")
    r = run("lanczos3_recompose", tmp_path / "two.tif", tmp_path / "ms", 3, "-flt1-007.tif", 0.7)
    assert r.returncode == 0, r.stderr
    _assert_close(_to_pfm(tmp_path, "two.tif"), R.recompose(lv[:2], 0.7), 3e-3, "recompose of 2 levels")
    # one level: the file as it is
    r = run("lanczos3_recompose", tmp_path / "one.pfm", tmp_path / "ms", 1, "-flt1-007.tif", 0.7)
    assert r.returncode == 0, r.stderr
    assert np.array_equal(rpfm(tmp_path / "one.pfm"), lv[0])


@pytest.mark.gpu
def test_tools_through_the_resident_server(lz3_tools, tmp_path, sock_dir):  # noqa: F811
    """each tool's files are the same bytes whether it runs by itself or is served by bin/nlk-server, and a
    served request costs less than half of a standalone one (no HIP start)"""
    a = _img(200, 120, 3, 8)
    _write_tif(tmp_path, "in.tif", a)
    lv = [np.clip(x + 2.5, 0, 255).astype(np.float32) for x in R.decompose(a, 3)]
    for i, x in enumerate(lv):
        _write_tif(tmp_path, f"ms{i}-flt2-003.tif", x)

    def steps(tag, env):
        seq = [("lanczos3_decompose", tmp_path / "in.tif", tmp_path / (tag + "ms"), 3, "-003.tif"),
               ("lanczos3_recompose", tmp_path / (tag + "rec.tif"), tmp_path / "ms", 3, "-flt2-003.tif", 0.7)]
        t0 = time.perf_counter()
        for s in seq:
            r = run(*s, env=env)
            assert r.returncode == 0, (s, r.stderr)
        return (time.perf_counter() - t0) / len(seq)

    alone = steps("a_", dict(os.environ))
    with server(sock_dir) as env:
        steps("w_", env)
        served = min(steps("s_", env) for _ in range(3))
        r = run("lanczos3_decompose", env=env)
        assert (r.returncode, r.stdout) == (0, USAGE["lanczos3_decompose"] + "\n")
    for f in ("ms0-003.tif", "ms1-003.tif", "ms2-003.tif", "rec.tif"):
        x, y = (open(tmp_path / (t + f), "rb").read() for t in ("a_", "s_"))
        assert x == y, f
    assert served < alone / 2, (served, alone)


@pytest.mark.gpu
def test_lz3_pipeline_two_frames(lz3_tools, synth, tmp_path):
    """scripts/msnlkalman-lz3-seq.sh for two frames, entirely through our binaries: decompose, the filter per level
    with sigma / 2^l (frame 1: backward flow per level from tvl1flow, the previous frame's outputs decomposed into
    `ma`), then recompose of flt1 and flt2 with 0.7. (The occlusion masks come from the reference's plambda, which
    is not ours; the filter runs without them.)"""
    w, h, ch, sigma, L = 96, 72, 3, 20.0, 2
    n0, n1, clean1 = synth.noisy_pair(w, h, ch, sigma, seed=3)
    _write_tif(tmp_path, "n-000.tif", n0)
    _write_tif(tmp_path, "n-001.tif", n1)
    o = lambda f: str(tmp_path / "out" / f)  # noqa: E731
    os.makedirs(tmp_path / "out")
    for i in (0, 1):
        r = run("lanczos3_decompose", tmp_path / f"n-{i:03d}.tif", o("ms"), L, f"-{i:03d}.tif")
        assert r.returncode == 0, r.stderr
        if i > 0:
            for k in ("flt1", "flt2"):
                r = run("lanczos3_decompose", o(f"{k}-{i - 1:03d}.tif"), o("ma"), L, f"-{k}-{i - 1:03d}.tif")
                assert r.returncode == 0, r.stderr
        for lvl in range(L - 1, -1, -1):
            nsy, f11, f21 = o(f"ms{lvl}-{i:03d}.tif"), o(f"ms{lvl}-flt1-{i:03d}.tif"), o(f"ms{lvl}-flt2-{i:03d}.tif")
            lsig = "%.2f" % (sigma / 2 ** lvl)
            if i > 0:
                f10, f20 = o(f"ma{lvl}-flt1-{i - 1:03d}.tif"), o(f"ma{lvl}-flt2-{i - 1:03d}.tif")
                flw = o(f"ms{lvl}-bflo-{i:03d}.flo")
                r = run("tvl1flow", nsy, f20, flw, 2, 0, 0.25, 0, 0, 1)
                assert r.returncode == 0, r.stderr
                r = run("nlkalman-flt", "-i", nsy, "-s", lsig, "-o", flw, "--flt10", f10, "--flt11", f11,
                        "--flt20", f20, "--flt21", f21)
            else:
                r = run("nlkalman-flt", "-i", nsy, "-s", lsig, "--flt11", f11, "--flt21", f21)
            assert r.returncode == 0, r.stderr
        for k in ("flt1", "flt2"):
            r = run("lanczos3_recompose", o(f"{k}-{i:03d}.tif"), o("ms"), L, f"-{k}-{i:03d}.tif", 0.7)
            assert r.returncode == 0, r.stderr
    f2 = _to_pfm(tmp_path / "out", "flt2-001.tif")
    assert f2.shape == (h, w, ch) and np.isfinite(f2).all()
    # the filtered pyramid recomposes to a denoised frame
    assert synth.psnr(f2, clean1) > synth.psnr(n1, clean1) + 5
