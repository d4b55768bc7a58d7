"""The defective-pixel filter: nlk_dev_despike (include/nlk_hip.h, csrc/k_despike.h), the sequence tools' --despike
K[,R], bin/nlk-despike and SequenceFilter(despike=...), against the one statement of the rule, tests/despike_ref.py
(float32 numpy).

CPU: the restatement against values worked out by hand; its false positives on frames without defects; what it gives
the recursion back on the CPU oracle with 21 stuck sensor sites (the setup of DESIGN.md §9's table, all synthetic); the
grammar of --despike's value (seq_despike_parse of host/seq_args.c, as a stand-alone program, plain and under the
sanitizers) and the tools that refuse through it. GPU: the kernel bit for bit (signed zeros compared as numbers), its
refusals, and the tools byte for byte against the same tools run on frames the restatement despiked."""
import importlib
import os
import subprocess

import numpy as np
import pytest

import despike_ref as DR
import yuv_ref
from test_cli import BIN, ROOT, rpfm, wpfm

F32 = np.float32
TINY = [(1, 1), (1, 9), (9, 1), (2, 2), (3, 2)]
SHAPES = TINY + [(37, 21), (130, 5), (64, 48), (257, 3)]   # (w, h)


def _bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def run(tool, *args, **kw):
    kw.setdefault("text", True)
    kw.setdefault("timeout", 300)
    return subprocess.run([os.path.join(BIN, tool), *map(str, args)], capture_output=True, **kw)


# ---------------------------------------------------------------- the restatement, by hand

def _ramp():
    y, x = np.mgrid[0:6, 0:7]
    return (10 * y + x).astype(F32)[:, :, None]   # 7 wide, 6 high: v(x, y) = 10 y + x


def test_ref_constant_image_is_unchanged_at_thr_0():
    for r in (1, 2):
        a = np.full((9, 11, 3), 7.25, F32)
        out, counts = DR.despike(a, 0.0, r)
        assert np.array_equal(_bits(out), _bits(a)) and not counts.any()   # v > mx is false


# (x, y, radius) -> the median of the ring of v = 10 y + x on 7 x 6, its indices reflected without repeating the edge:
#  R = 1 corner: (1,1) x 4, (0,1) x 2, (1,0) x 2 = 1 1 10 10 | 11 11 11 11         edge (3,0): 2 4 12 12 | 13 13 14 14
#  R = 1 interior (3,3): 22 23 24 32 | 34 42 43 44
#  R = 2 corner: 2 2 12 12 12 12 20 20 | 21 21 21 21 22 22 22 22       edge (3,0): 1 5 11 11 15 15 21 21 | 22 22 23 23 ...
#  R = 2 interior (3,3): 11 12 13 14 15 21 25 31 | 35 41 45 51 52 53 54 55
BY_HAND = {(0, 0, 1): 10.5, (3, 0, 1): 12.5, (3, 3, 1): 33.0, (0, 0, 2): 20.5, (3, 0, 2): 21.5, (3, 3, 2): 33.0}


@pytest.mark.parametrize("x,y,r", sorted(BY_HAND))
@pytest.mark.parametrize("spike", [1000.0, -1000.0])
def test_ref_one_planted_sample_becomes_the_median_worked_out_by_hand(x, y, r, spike):
    a = _ramp()
    a[y, x, 0] = spike
    out, counts = DR.despike(a, 5.0, r)
    want = a.copy()
    want[y, x, 0] = BY_HAND[(x, y, r)]
    assert np.array_equal(out, want) and list(counts) == [1]


def _reads_itself(w, h, r):
    """[h][w]: the sample's own position is on its (reflected, clamped) ring"""
    ys, xs = np.arange(h)[:, None], np.arange(w)[None, :]
    m = np.zeros((h, w), bool)
    for dx, dy in DR.ring_offsets(r):
        m |= (DR.border_index(ys + dy, h) == ys) & (DR.border_index(xs + dx, w) == xs)
    return m


@pytest.mark.parametrize("w,h", TINY)
def test_ref_tiny_shapes_change_nothing_without_a_ring_in_the_frame(w, h):
    rng = np.random.default_rng(w * 100 + h)
    for r in (1, 2):
        for ch in (1, 3):
            a = rng.normal(128, 60, (h, w, ch)).astype(F32)
            out, counts = DR.despike(a, 0.0, r)
            own = _reads_itself(w, h, r)
            assert np.array_equal(_bits(out)[own], _bits(a)[own])          # v > mx >= v is false
            assert counts.sum() == np.count_nonzero(_bits(out) != _bits(a))
            if w == 1 or h == 1:
                assert own.all() and not counts.any()
    assert _reads_itself(2, 2, 2).all() and not _reads_itself(2, 2, 1).any()


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_ref_a_non_finite_sample_blocks_exactly_the_samples_that_read_it(bad):
    rng = np.random.default_rng(5)
    a = rng.normal(128, 20, (12, 15, 2)).astype(F32)
    base, _ = DR.despike(a, 0.0, 1)
    assert np.count_nonzero(_bits(base) != _bits(a)) > 30                 # at thr = 0 about 2 of 10 samples are hits
    for r in (1, 2):
        base, _ = DR.despike(a, 0.0, r)
        blocked_hits = 0
        for (x, y) in ((0, 0), (7, 5), (14, 11), (1, 6)):
            b = a.copy()
            b[y, x, 1] = bad
            out, counts = DR.despike(b, 0.0, r)
            reads = np.zeros(a.shape, bool)
            ys, xs = np.arange(12)[:, None], np.arange(15)[None, :]
            for dx, dy in DR.ring_offsets(r):
                reads[..., 1] |= (DR.border_index(ys + dy, 12) == y) & (DR.border_index(xs + dx, 15) == x)
            reads[y, x, 1] = True
            assert np.array_equal(_bits(out)[reads], _bits(b)[reads])     # copied, the bad sample included
            assert np.array_equal(_bits(out)[~reads], _bits(base)[~reads])  # nobody else notices
            blocked_hits += np.count_nonzero(_bits(base)[reads] != _bits(a)[reads])
            assert counts.sum() == np.count_nonzero(_bits(out) != _bits(b))
        assert blocked_hits > 0   # (hits were among the blocked)


def test_ref_false_positives(synth):
    """frames without defects: at most 1e-4 of the samples are replaced at thr = 4 sigma (measured: none)"""
    n = total = 0
    for sigma in (5.0, 20.0, 40.0):
        for seed in range(1, 9):
            a = synth.awgn(synth.clean_frame(96, 64, 3), sigma, seed)
            for r in (1, 2):
                out, counts = DR.despike(a, 4.0 * sigma, r)
                assert counts.sum() == np.count_nonzero(_bits(out) != _bits(a))
                n += int(counts.sum())
                total += a.size
    print("replaced %d of %d" % (n, total))
    assert total == 884736 and n <= 1e-4 * total


@pytest.mark.parametrize("sigma", [10.0, 20.0])
def test_oracle_despiking_recovers_what_the_defects_cost(O, synth, sigma):
    """the chain of DESIGN.md §9's table on the CPU oracle, 21 stuck sites: despiking first recovers at least half of
    the PSNR lost, in dB, over frames 1..3 (measured: 8.25 -> 0.02 dB lost at sigma 10, 2.72 -> 0.21 at sigma 20); without
    defects the run is the run without despiking, exactly"""
    sites = DR.defect_sites(96, 64)
    assert len(sites) == 21 and sum(x in (0, 95) or y in (0, 63) for x, y, _ in sites) == 3
    thr = float(F32(4.0) * F32(sigma))
    clean, _, outs = DR.chain(O, synth, sigma)
    bad, rb, _ = DR.chain(O, synth, sigma, lambda a: DR.plant(a, sites), sites=sites)
    fix, rf, _ = DR.chain(O, synth, sigma, lambda a: DR.despike(DR.plant(a, sites), thr, 1)[0], sites=sites)
    same, _, outs2 = DR.chain(O, synth, sigma, lambda a: DR.despike(a, thr, 1)[0])
    lost, left = np.mean(clean[1:]) - np.mean(bad[1:]), np.mean(clean[1:]) - np.mean(fix[1:])
    print("sigma %g: lost %.2f dB, after despiking %.2f dB; RMSE at the sites %.1f -> %.1f" % (
        sigma, lost, left, np.mean(rb), np.mean(rf)))
    assert lost > 2.0 and left <= 0.5 * lost
    assert max(rf) < 0.5 * min(rb)
    assert same == clean and all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(outs, outs2))


# ---------------------------------------------------------------- the grammar

ACCEPTED = {"4": (4.0, 1), "4,1": (4.0, 1), "2.5,2": (2.5, 2)}
REFUSED = ["0", "-1", "4,3", "4,", "nan", "x", "", "inf", "4,1x", "4x", "4,0", ",1", "4,12"]
WANT = "%s: --despike %s: want K or K,R with K > 0 and R = 1 or 2\n"


@pytest.fixture(scope="module")
def drivers(tmp_path_factory):
    """tests/despike_args_driver.c with host/seq_args.c and nothing else, plain and under the sanitizers (their runtimes
    linked statically where the compiler has them: the program runs as it is, nothing is preloaded)"""
    d = tmp_path_factory.mktemp("despike_args")
    src = [os.path.join(ROOT, "tests", "despike_args_driver.c"), os.path.join(ROOT, "bwd-nlkalman_amd", "host", "seq_args.c")]
    inc = ["-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "bwd-nlkalman_amd", "host")]
    base = ["gcc", "-O1", "-g", "-std=gnu99", "-Wall", "-Werror", *inc, *src, "-o"]
    plain, san = str(d / "plain"), str(d / "san")
    subprocess.check_call(base + [plain])
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    for static in (["-static-libasan", "-static-libubsan"], []):
        if subprocess.run(base + [san, *flags, *static], capture_output=True).returncode == 0 and \
                subprocess.run([san], capture_output=True).returncode == 0:
            return [plain, san]
    return [plain]


def test_grammar(drivers):
    for exe in drivers:
        texts = list(ACCEPTED) + REFUSED
        r = subprocess.run([exe, *texts], capture_output=True, text=True, timeout=60)
        assert r.returncode == 0 and r.stderr == "", (exe, r)
        lines = r.stdout.splitlines()
        assert len(lines) == len(texts)
        for text, line in zip(texts, lines):
            f = line.split()
            got = (float(f[1]), int(f[3]), int(f[5]))
            assert got == ((*ACCEPTED[text], 0) if text in ACCEPTED else (-1.0, -1, 1)), (text, line)


@pytest.mark.parametrize("tool", ["nlkalman-seq", "nlkalman-seq-gt", "nlkalman-lsmo-seq", "nlkalman-y4m"])
def test_tools_refuse_under_their_own_name(built, tool, tmp_path):
    exe = os.path.join(BIN, tool)
    if not os.path.exists(exe):
        built.build()
    out, missing = tmp_path / "out", tmp_path / "missing.y4m"
    for text in REFUSED:
        # (the seq tools make OUT, the stream tool opens IN, before either opens a device: neither happens)
        args = ["--despike", text, 20, missing] if tool == "nlkalman-y4m" else \
            ["--of", "tvl1", "--despike", text, "--sure", tmp_path / "%03d.tif", 1, 3, 20, out]
        r = subprocess.run([exe, *map(str, args)], capture_output=True, text=True, timeout=60)
        assert (r.returncode, r.stdout, r.stderr) == (1, "", WANT % (tool, text)), (text, r)
        assert not out.exists()
    # the option's place: after --of, in front of --sure; an accepted value goes on to the missing frames
    r = subprocess.run([exe, "--despike", "4,2", str(tmp_path / "%03d.tif"), "1", "3", "20", str(out)] if tool != "nlkalman-y4m"
                       else [exe, "--despike", "4,2", "20", str(missing)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "--despike" not in r.stderr and not out.exists(), r


def test_nlk_despike_usage(built):
    exe = os.path.join(BIN, "nlk-despike")
    if not os.path.exists(exe):
        built.build()
    for args in ([], ["4"], ["4", "a", "b", "c"], ["-r", "3", "4", "a", "b"], ["-1", "a", "b"], ["nan", "a", "b"],
                 ["x", "a", "b"], ["-r", "2", "4", "a"]):
        r = subprocess.run([exe, *args], capture_output=True, text=True, timeout=60)
        assert r.returncode == 1 and r.stdout == "" and r.stderr.startswith("usage: "), (args, r)


# ---------------------------------------------------------------- the kernel

def _spots(w, h):
    """every corner, the middle of every edge, and interior positions"""
    xs = sorted({0, w // 2, w - 1, w // 3, min(w - 1, 70)})
    ys = sorted({0, h // 2, h - 1, h // 3})
    return [(x, y) for x in xs for y in ys]


def _inputs(w, h, ch, seed):
    """name -> (image, thr)"""
    rng = np.random.default_rng(seed)
    noise = rng.normal(128, 10, (h, w, ch)).astype(F32)
    spikes = noise.copy()
    for n, (x, y) in enumerate(_spots(w, h)):
        for c in range(ch):
            spikes[y, x, c] += 200.0 if (n + c) % 2 else -200.0
    blobs = noise.copy()
    for n, (x, y) in enumerate(_spots(w, h)):
        if n % 3 == 0:
            blobs[y:y + 2, x:x + 2] = 255.0 if n % 2 else 0.0
    ties = rng.integers(-2, 3, (h, w, ch)).astype(F32)
    ties[(ties == 0) & (rng.random((h, w, ch)) < 0.5)] = -0.0
    bad = spikes.copy()
    for n, v in enumerate((np.nan, np.inf, -np.inf, np.nan)):
        bad[(n * 5) % h, (n * 11 + 3) % w, n % ch] = v
    return {"spikes": (spikes, 40.0), "blobs": (blobs, 40.0), "ties": (ties, 0.0), "non-finite": (bad, 40.0)}


@pytest.mark.gpu
@pytest.mark.parametrize("ch", [1, 3, 4])
@pytest.mark.parametrize("radius", [1, 2])
def test_gpu_kernel_gives_the_bits_of_the_restatement(ctx, ch, radius):
    total = 0
    for w, h in SHAPES:
        nb = w * h * ch * 4
        d_in, d_out, d_cnt = ctx.alloc(nb), ctx.alloc(nb), ctx.alloc(4 * ch)
        for name, (a, thr) in _inputs(w, h, ch, 1000 * w + h).items():
            what = (name, w, h, ch, radius)
            want, counts = DR.despike(a, thr, radius)
            ctx._chk(ctx.L.nlk_h2d(ctx.h, d_in, a.ctypes.data, nb))
            ctx._chk(ctx.L.nlk_h2d(ctx.h, d_cnt, np.full(ch, 77, np.uint32).ctypes.data, 4 * ch))   # the call zeroes them
            ctx.despike(d_out, d_in, w, h, ch, thr, radius, d_cnt)
            got = ctx.download(d_out, a.shape)
            assert DR.same_bits(got, want), what
            assert np.array_equal(ctx.download(d_cnt, (ch,), np.uint32), counts), what
            assert np.array_equal(_bits(ctx.download(d_in, a.shape)), _bits(a)), what      # in is only read
            ctx._chk(ctx.L.nlk_h2d(ctx.h, d_out, np.zeros_like(a).ctypes.data, nb))
            ctx.despike(d_out, d_in, w, h, ch, thr, radius)                               # d_count = NULL
            assert np.array_equal(_bits(ctx.download(d_out, a.shape)), _bits(got)), what  # ... and the same bits again
            assert np.array_equal(ctx.despike_counts(d_out, d_in, w, h, ch, thr, radius), counts), what
            total += int(counts.sum())
        for p in (d_in, d_out, d_cnt):
            ctx.free(p)
    assert total > 100   # (the inputs do have hits)


@pytest.mark.gpu
def test_gpu_refused_calls_write_nothing_and_leave_the_context_working(ctx, built):
    w, h, ch = 37, 21, 3
    a, thr = _inputs(w, h, ch, 3)["spikes"]
    mark = np.full_like(a, -5.0)
    d_in, d_out, d_cnt = ctx.upload(a), ctx.upload(mark), ctx.upload(np.full(ch, 77, np.uint32))
    L, EINVAL = ctx.L, -3
    calls = [(ctx.h, d_out, d_in, d_cnt, 0, h, ch, 1, thr), (ctx.h, d_out, d_in, d_cnt, w, 0, ch, 1, thr),
             (ctx.h, d_out, d_in, d_cnt, -1, h, ch, 1, thr), (ctx.h, d_out, d_in, d_cnt, w, h, 0, 1, thr),
             (ctx.h, d_out, d_in, d_cnt, w, h, 17, 1, thr), (ctx.h, d_out, d_in, d_cnt, w, h, ch, 0, thr),
             (ctx.h, d_out, d_in, d_cnt, w, h, ch, 3, thr), (ctx.h, d_out, d_in, d_cnt, w, h, ch, 1, -1.0),
             (ctx.h, d_out, d_in, d_cnt, w, h, ch, 1, float("nan")), (ctx.h, d_out, d_in, d_cnt, w, h, ch, 1, float("inf")),
             (None, d_out, d_in, d_cnt, w, h, ch, 1, thr), (ctx.h, None, d_in, d_cnt, w, h, ch, 1, thr),
             (ctx.h, d_out, None, d_cnt, w, h, ch, 1, thr), (ctx.h, d_in, d_in, d_cnt, w, h, ch, 1, thr)]
    for args in calls:
        assert L.nlk_dev_despike(*args) == EINVAL, args
        if args[0] is not None:
            assert b"nlk_dev_despike" in L.nlk_last_error(ctx.h)
    ctx.sync()
    assert np.array_equal(ctx.download(d_out, a.shape), mark)
    assert np.array_equal(_bits(ctx.download(d_in, a.shape)), _bits(a))
    assert list(ctx.download(d_cnt, (ch,), np.uint32)) == [77] * ch
    want, counts = DR.despike(a, thr, 1)
    assert np.array_equal(ctx.despike_counts(d_out, d_in, w, h, ch, thr), counts) and counts.sum() > 0
    assert DR.same_bits(ctx.download(d_out, a.shape), want)
    for p in (d_in, d_out, d_cnt):
        ctx.free(p)


# ---------------------------------------------------------------- the tools

W, H, SIGMA, K = 96, 64, 20.0, 4.0
FMT = yuv_ref.fmt("444", 0, 601)


def _decode(path):
    r = run("nlk-imgconv", path, str(path) + ".pfm")
    assert r.returncode == 0, r.stderr
    return rpfm(str(path) + ".pfm")


def _tifs(folder, frames):
    """the frames as float TIFF files 001.tif ... through the project's image I/O"""
    folder.mkdir()
    for t, a in enumerate(frames):
        wpfm(folder / "tmp.pfm", a)
        r = run("nlk-imgconv", folder / "tmp.pfm", folder / ("%03d.tif" % (t + 1)))
        assert r.returncode == 0, r.stderr
        assert np.array_equal(_bits(_decode(folder / ("%03d.tif" % (t + 1)))), _bits(a))
    return folder / "%03d.tif"


@pytest.fixture(scope="module")
def seq_runs(built, synth, tmp_path_factory):
    """3 frames of 96 x 64 x 3 at sigma 20 with the 21 stuck sites, as a 4:4:4 stream holds them; `nlkalman-seq
    --despike 4` on them and `nlkalman-seq` on the frames the restatement despiked (float TIFF), no smoother"""
    if not all(os.path.exists(os.path.join(BIN, t)) for t in ("nlkalman-seq", "nlkalman-y4m", "nlk-imgconv", "nlk-despike")):
        built.build()
    base = tmp_path_factory.mktemp("despike")
    sites = DR.defect_sites(W, H)
    pay = [yuv_ref.to_yuv(DR.plant(synth.awgn(synth.clean_frame(W, H, 3, t), SIGMA, 100 + t), sites), FMT).tobytes()
           for t in range(3)]
    frames = [yuv_ref.to_rgb(p, W, H, FMT) for p in pay]
    thr = float(F32(K) * F32(SIGMA))
    fixed = [DR.despike(a, thr, 1) for a in frames]
    print("replaced per frame:", [int(c.sum()) for _, c in fixed])
    assert all(c.sum() >= 30 for _, c in fixed)         # (of 63 samples: a 0 on a dark patch, a 255 on a bright one is no hit)
    env = dict(os.environ, NLK_DETERMINISTIC="1")
    src, ref = _tifs(base / "in", frames), _tifs(base / "fixed", [a for a, _ in fixed])
    got = run("nlkalman-seq", "--despike", 4, src, 1, 3, 20, base / "got", 1, "", "no", env=env)
    assert got.returncode == 0, got.stderr
    want = run("nlkalman-seq", ref, 1, 3, 20, base / "want", 1, "", "no", env=env)
    assert want.returncode == 0, want.stderr
    return base, sites, pay, frames, fixed, env


@pytest.mark.gpu
def test_gpu_seq_despike_is_seq_on_despiked_frames(ctx, seq_runs):
    base = seq_runs[0]
    names = ["%s-%03d.tif" % (kind, i) for kind in ("flt1", "flt2") for i in (1, 2, 3)] + ["bflo1-002.flo", "bocc1-003.png"]
    for name in names:
        assert (base / "got" / name).read_bytes() == (base / "want" / name).read_bytes(), name
    plain = run("nlkalman-seq", base / "in" / "%03d.tif", 1, 3, 20, base / "plain", 1, "", "no", env=seq_runs[5])
    assert plain.returncode == 0, plain.stderr
    assert (base / "plain" / "flt2-002.tif").read_bytes() != (base / "got" / "flt2-002.tif").read_bytes()


@pytest.mark.gpu
def test_gpu_lsmo_and_gt_tools_take_the_option(ctx, seq_runs, tmp_path):
    """the other two tools of the same source: the option in its place (after --of, in front of --sure) gives the
    flt2 files of nlkalman-seq --despike"""
    base, env = seq_runs[0], seq_runs[5]
    r = run("nlkalman-lsmo-seq", "--of", "tvl1", "--despike", "4,1", "--sure", base / "in" / "%03d.tif", 1, 3, 20,
            tmp_path / "lsmo", "", "no", env=env)
    assert r.returncode == 0, r.stderr
    for i in (1, 2, 3):
        name = "flt2-%03d.tif" % i
        assert (tmp_path / "lsmo" / name).read_bytes() == (base / "got" / name).read_bytes(), name
    # gt: the noisy files exist, so they are read and used; the measures are against the clean frames
    synth = importlib.import_module("bwd-nlkalman_amd.synth")
    clean = _tifs(tmp_path / "clean", [synth.clean_frame(W, H, 3, t) for t in range(3)])
    outs = {}
    for tag, opt in (("with", ["--despike", "4"]), ("without", [])):
        d = tmp_path / ("gt_" + tag)
        d.mkdir()
        for i in (1, 2, 3):
            (d / ("%03d.tif" % i)).write_bytes((base / "in" / ("%03d.tif" % i)).read_bytes())
        r = run("nlkalman-seq-gt", *opt, clean, 1, 3, 20, d, "", "no", env=env)
        assert r.returncode == 0, r.stderr
        outs[tag] = [float(v) for v in r.stdout.split()]
    # flt2's MSE: DESIGN.md §9's table has 35.0 against 32.4 dB at this sigma, a factor of 0.55
    assert len(outs["with"]) == 2 and outs["with"][1] < 0.75 * outs["without"][1], outs


@pytest.mark.gpu
def test_gpu_y4m_and_sequence_filter_agree_with_seq(ctx, built, seq_runs):
    base, sites, pay, frames, fixed, env = seq_runs
    flt2 = [_decode(base / "want" / ("flt2-%03d.tif" % (t + 1))) for t in range(3)]
    y = run("nlkalman-y4m", "--despike", 4, 20, input=yuv_ref.y4m_bytes(W, H, "444", pay), env=env, text=False)
    assert y.returncode == 0, y.stderr
    got = yuv_ref.y4m_parse(y.stdout)[4]
    assert got == [yuv_ref.to_yuv(a, FMT).tobytes() for a in flt2]
    off = run("nlkalman-y4m", 20, input=yuv_ref.y4m_bytes(W, H, "444", pay), env=env, text=False)
    assert off.returncode == 0 and yuv_ref.y4m_parse(off.stdout)[4] != got
    seq = importlib.import_module("bwd-nlkalman_amd.sequence")
    ctx.set_deterministic(True)
    try:
        sf = seq.SequenceFilter(ctx, W, H, 3, SIGMA, keep_history=False, despike=4)
        for t in range(3):
            d = ctx.upload(frames[t])
            sf.push(d)
            assert np.array_equal(_bits(ctx.download(d, frames[t].shape)), _bits(frames[t]))   # not modified
            assert np.array_equal(_bits(sf.download_rgb(sf.flt2)), _bits(flt2[t])), t
            ctx.free(d)
        assert seq.SequenceFilter(ctx, W, H, 3, SIGMA, despike=(2.5, 2)).despike == (2.5, 2)
        for bad in (0, -1, (4, 3), float("nan")):
            with pytest.raises(ValueError):
                seq.SequenceFilter(ctx, W, H, 3, SIGMA, despike=bad)
    finally:
        ctx.set_deterministic(False)


@pytest.mark.gpu
def test_gpu_despike_under_vst(ctx, seq_runs):
    """under vst:A,B the filter runs on the transformed frame at the run's sigma: a threshold nothing reaches is the
    run without the option, byte for byte; --despike 4 differs from it at the planted sites"""
    base, sites, _, frames, _, env = seq_runs
    outs = {}
    for tag, opt in (("off", []), ("huge", ["--despike", "1e9"]), ("on", ["--despike", "4"])):
        r = run("nlkalman-seq", *opt, base / "in" / "%03d.tif", 1, 3, "vst:1,300", base / ("vst_" + tag), 1, "", "no", env=env)
        assert r.returncode == 0 and r.stdout.startswith("vst 1 300 "), (r.stdout, r.stderr)
        outs[tag] = r.stdout
    assert outs["off"] == outs["huge"] == outs["on"]
    mask = DR.site_mask((H, W), sites)
    for kind in ("flt1", "flt2"):
        for i in (1, 2, 3):
            name = "%s-%03d.tif" % (kind, i)
            assert (base / "vst_huge" / name).read_bytes() == (base / "vst_off" / name).read_bytes(), name
            d = np.abs(_decode(base / "vst_on" / name).astype(np.float64) - _decode(base / "vst_off" / name)).max(axis=2)
            print("%s: mean difference at the sites %.1f, elsewhere %.2f" % (name, d[mask].mean(), d[~mask].mean()))
            # the input changed at the sites only (by about 100 where the rule replaced one): more than half of them
            # differ in the output, and by more than the rest of the frame, which the sites reach through shared patches
            assert np.count_nonzero(d[mask] > 0) > 10 and d[mask].mean() > d[~mask].mean(), name


@pytest.mark.gpu
def test_gpu_nlk_despike_prints_the_counts_of_the_restatement(ctx, seq_runs, tmp_path):
    base, _, _, frames, fixed, _ = seq_runs
    r = run("nlk-despike", 80, base / "in" / "001.tif", tmp_path / "out.tif")
    assert (r.returncode, r.stderr) == (0, ""), r
    assert r.stdout == " ".join(str(int(c)) for c in fixed[0][1]) + "\n"
    assert DR.same_bits(_decode(tmp_path / "out.tif"), fixed[0][0])
    want, counts = DR.despike(frames[0], 30.0, 2)
    r = run("nlk-despike", "-r", 2, 30, base / "in" / "001.tif", tmp_path / "out2.tif")
    assert (r.returncode, r.stderr) == (0, ""), r
    assert r.stdout == " ".join(str(int(c)) for c in counts) + "\n" and counts.sum() > fixed[0][1].sum()
    assert DR.same_bits(_decode(tmp_path / "out2.tif"), want)
