"""A defect map learned over time: nlk_dev_defect_step and nlk_defect_schedule (include/nlk_hip.h, csrc/k_defect.h,
host/defect_schedule.c), the sequence tools' --defect-map K[,R[,N]], bin/nlk-defects and
SequenceFilter(defect_map=...), against the one statement of the rule, tests/defectmap_ref.py (float32 numpy).

CPU: the restatement against values worked out by hand; what it detects, and when, on the pan with independent noise;
the schedule and the grammar as stand-alone programs (plain and under the sanitizers); the tools that refuse; what the
map gives the recursion back on the CPU oracle where --despike alone cannot (sigma 40: the set-up of DESIGN.md §9's
table, all synthetic). GPU: the kernel bit for bit over six frames with swapped means, its refusals, and the tools byte
for byte against the same tools run on frames the restatement cleaned."""
import importlib
import os
import subprocess

import numpy as np
import pytest

import defectmap_ref as DM
import despike_ref as DR
import yuv_ref
from test_cli import BIN, ROOT, rpfm, wpfm

F32 = np.float32


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


# (x, y, radius) -> the median of the ring of v = 10 y + x on 7 x 6, its indices reflected without repeating the edge:
#  R = 1 corner: (1,1) x 4, (0,1) x 2, (1,0) x 2 = 1 1 10 10 | 11 11 11 11         edge (3,0): 2 4 12 12 | 13 13 14 14
#  R = 1 interior (3,3): 22 23 24 32 | 34 42 43 44
#  R = 2 corner: 2 2 12 12 12 12 20 20 | 21 21 21 21 22 22 22 22       edge (3,0): 1 5 11 11 15 15 21 21 | 22 22 23 23 ...
#  R = 2 interior (3,3): 11 12 13 14 15 21 25 31 | 35 41 45 51 52 53 54 55
BY_HAND = {(0, 0, 1): 10.5, (3, 0, 1): 12.5, (3, 3, 1): 33.0, (0, 0, 2): 20.5, (3, 0, 2): 21.5, (3, 3, 2): 33.0}


def test_ref_first_frame_is_copied_and_starts_the_mean():
    rng = np.random.default_rng(1)
    v = rng.normal(128, 40, (9, 11, 3)).astype(F32)
    v[2, 3, 1], v[0, 0, 0], v[8, 10, 2] = np.nan, np.inf, -0.0
    out, m, hit, counts = DM.step(v, None, 0.0, 1.0, 1)
    assert np.array_equal(_bits(out), _bits(v)) and not hit.any() and list(counts) == [0, 0, 0]
    want = v.copy()
    want[2, 3, 1] = want[0, 0, 0] = 0.0
    assert np.array_equal(_bits(m), _bits(want))


@pytest.mark.parametrize("x,y,r", sorted(BY_HAND))
@pytest.mark.parametrize("site", [1000.0, -1000.0])
def test_ref_a_planted_site_of_the_mean_becomes_the_median_of_the_frames_ring(x, y, r, site):
    """the mean: a constant plus half the ramp, the site a constant; the frame: the ramp, its own sample at the site far
    off. thr = 5, gain = 1/4: every value below is exact in float32"""
    m = (F32(50) + F32(0.5) * _ramp()).astype(F32)
    m[y, x, 0] = site
    v = _ramp()
    v[y, x, 0] = 500.0
    out, m_new, hit, counts = DM.step(v, m, 5.0, 0.25, r)
    want = v.copy()
    want[y, x, 0] = BY_HAND[(x, y, r)]
    assert np.array_equal(out, want) and list(counts) == [1]
    assert hit.sum() == 1 and hit[y, x, 0]
    # the mean takes the raw sample, at the site too: site + (500 - site) / 4, not the median
    by_hand = (m.astype(np.float64) + (v.astype(np.float64) - m) * 0.25).astype(F32)
    assert by_hand[y, x, 0] == site + (500.0 - site) / 4 and np.array_equal(_bits(m_new), _bits(by_hand))


def test_ref_a_hit_sites_mean_keeps_taking_the_raw_value():
    """a stuck site stays flagged on every frame: the mean at the site follows the raw 255, not what replaced it"""
    rng = np.random.default_rng(2)
    frames = []
    for t in range(12):
        a = rng.normal(100, 10, (9, 11, 1)).astype(F32)
        a[4, 5, 0] = 255.0
        frames.append(a)
    m = None
    for t, v in enumerate(frames):
        thr, gain = DM.schedule(t, 32, 40.0) if t else (0.0, 1.0)
        out, m, hit, counts = DM.step(v, m, thr, gain, 1)
        assert m[4, 5, 0] == 255.0                            # (255 + (255 - 255) * gain)
        if t:
            assert hit[4, 5, 0] and hit.sum() == 1 and list(counts) == [1], t
            ring = np.sort(np.delete(v[3:6, 4:7, 0].ravel(), 4))
            assert out[4, 5, 0] == F32(F32(ring[3] + ring[4]) * F32(0.5))


def _reads(shape, x, y, c, r):
    """the samples whose ring (reflected, clamped) holds sample (x, y, c), and that sample"""
    h, w = shape[:2]
    reads = np.zeros(shape, bool)
    ys, xs = np.arange(h)[:, None], np.arange(w)[None, :]
    for dx, dy in DR.ring_offsets(r):
        reads[..., c] |= (DR.border_index(ys + dy, h) == y) & (DR.border_index(xs + dx, w) == x)
    reads[y, x, c] = True
    return reads


@pytest.mark.parametrize("r", [1, 2])
def test_ref_a_nan_blocks_exactly_the_replacements_that_read_it(r):
    rng = np.random.default_rng(5)
    m = rng.normal(128, 20, (12, 15, 2)).astype(F32)
    v = rng.normal(128, 20, (12, 15, 2)).astype(F32)
    base, m_base, hit_base, _ = DM.step(v, m, 0.0, 0.5, r)
    assert np.count_nonzero(_bits(base) != _bits(v)) > 30                 # at thr = 0 about 2 of 10 samples are hits
    blocked = 0
    for (x, y) in ((0, 0), (7, 5), (14, 11), (1, 6)):
        b = v.copy()
        b[y, x, 1] = np.nan
        out, m_new, hit, counts = DM.step(b, m, 0.0, 0.5, r)
        reads = _reads(v.shape, x, y, 1, r)
        assert np.array_equal(hit, hit_base)                                # the hits are read on the mean
        assert np.array_equal(_bits(out)[reads], _bits(b)[reads])           # copied, the NaN included
        assert np.array_equal(_bits(out)[~reads], _bits(base)[~reads])      # nobody else notices
        assert counts.sum() == np.count_nonzero(hit & ~reads)
        blocked += np.count_nonzero((hit & reads)[..., 1])
        assert m_new[y, x, 1] == m[y, x, 1]                                 # the mean stays at the NaN's site ...
        m_new[y, x, 1] = m_base[y, x, 1]
        assert np.array_equal(_bits(m_new), _bits(m_base))                  # ... and only there
    assert blocked > 0   # (hits were among the blocked)
    # a NaN in the mean: no hit where it is read
    mb = m.copy()
    mb[5, 7, 0] = np.nan
    out, m_new, hit, _ = DM.step(v, mb, 0.0, 0.5, r)
    reads = _reads(v.shape, 7, 5, 0, r)
    assert not hit[reads].any() and np.array_equal(hit[~reads], hit_base[~reads])
    assert np.isnan(m_new[5, 7, 0])


@pytest.mark.parametrize("w,h", [(1, 1), (1, 5), (5, 1), (2, 2), (3, 3)])
def test_ref_tiny_frames_run_and_change_nothing_they_should_not(w, h):
    rng = np.random.default_rng(w * 100 + h)
    for r in (1, 2):
        for ch in (1, 3):
            ys, xs = np.arange(h)[:, None], np.arange(w)[None, :]
            own = np.zeros((h, w), bool)   # the sample's own position is on its ring: m > mx >= m is false
            for dx, dy in DR.ring_offsets(r):
                own |= (DR.border_index(ys + dy, h) == ys) & (DR.border_index(xs + dx, w) == xs)
            m = None
            for t in range(4):
                v = rng.normal(128, 60, (h, w, ch)).astype(F32)
                thr, gain = DM.schedule(t, 2, 0.0) if t else (0.0, 1.0)
                out, m_new, hit, counts = DM.step(v, m, thr, gain, r)
                assert out.shape == m_new.shape == hit.shape == v.shape and counts.shape == (ch,)
                assert not hit[own].any() and np.array_equal(_bits(out)[~hit], _bits(v)[~hit])
                assert counts.sum() == hit.sum()
                if w == 1 or h == 1:
                    assert own.all()
                m = m_new
    assert DM.step(np.zeros((1, 1, 1), F32), np.ones((1, 1, 1), F32), 0.0, 0.5, 1)[1][0, 0, 0] == 0.5


# ---------------------------------------------------------------- what it detects, and when

def _pan(synth, sigma, sites, blob, nf=48):
    return [DR.plant(DM.noisy_frame(synth, sigma, t)[1], sites, blob) if sites else DM.noisy_frame(synth, sigma, t)[1]
            for t in range(nf)]


@pytest.mark.parametrize("sigma", [10.0, 20.0, 40.0])
@pytest.mark.parametrize("blob,since", [(1, 16), (2, 32)])
def test_ref_detection_on_the_pan(synth, sigma, blob, since):
    """K = 4, N = 32, 48 frames of the pan: every planted sample is flagged on every frame from 16 on (single sites,
    R = 1; measured: from 4 / 7 / 15 at sigma 10 / 20 / 40) and from 32 on (2 x 2 blobs, R = 2; measured: 6 / 10 / 20);
    on a clean sensor at most 1e-4 of the samples are ever flagged (measured: none)"""
    sites = DR.defect_sites(96, 64, blob=blob)
    mask = DR.site_mask((64, 96), sites, blob)
    assert len(sites) == 21 and mask.sum() == 21 * blob * blob
    k_sigma = F32(4) * F32(sigma)
    res = DM.run(_pan(synth, sigma, sites, blob), k_sigma, blob, 32)
    full = [bool(hit[mask].all()) for _, hit, _ in res]
    print("sigma %g, blob %d: all %d planted samples flagged from frame %d on" % (
        sigma, blob, 3 * mask.sum(), max([t + 1 for t, f in enumerate(full) if not f])))
    assert all(full[since:])
    off = sum(int(hit[~mask].sum()) for _, hit, _ in res)
    clean = sum(int(hit.sum()) for _, hit, _ in DM.run(_pan(synth, sigma, None, blob), k_sigma, blob, 32))
    print("flagged off the sites: %d; on a clean sensor: %d of %d" % (off, clean, 48 * 96 * 64 * 3))
    assert clean <= 1e-4 * 48 * 96 * 64 * 3 and off <= 1e-4 * 48 * 96 * 64 * 3


# ---------------------------------------------------------------- the schedule and the grammar, as programs

def _drivers(d, name, sources, libs=()):
    """tests/<name>.c with the given host sources and nothing else, plain and under the sanitizers (their runtimes
    linked statically where the compiler has them: the program runs as it is, nothing is preloaded)"""
    host = os.path.join(ROOT, "bwd-nlkalman_amd", "host")
    src = [os.path.join(ROOT, "tests", name + ".c")] + [os.path.join(host, s) for s in sources]
    inc = ["-I" + os.path.join(ROOT, "include"), "-I" + host]
    plain, san = str(d / (name + "_plain")), str(d / (name + "_san"))
    base = ["gcc", "-O1", "-g", "-std=gnu99", "-Wall", "-Werror", *inc, *src]
    subprocess.check_call(base + ["-o", plain, *libs])
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    for static in (["-static-libasan", "-static-libubsan"], []):
        if subprocess.run(base + ["-o", san, *flags, *static, *libs], capture_output=True).returncode == 0 and \
                subprocess.run([san], capture_output=True).returncode in (0, 2):
            return [plain, san]
    return [plain]


@pytest.fixture(scope="module")
def drivers(tmp_path_factory):
    d = tmp_path_factory.mktemp("defect_drivers")
    return {"schedule": _drivers(d, "defect_schedule_driver", ["defect_schedule.c"], ["-lm"]),
            "args": _drivers(d, "defect_args_driver", ["seq_args.c"])}


def test_schedule_gives_the_bits_of_the_restatement(drivers):
    k_sigma = F32(4) * F32(12.7)
    for exe in drivers["schedule"]:
        r = subprocess.run([exe, "%.9g" % k_sigma, "100", "2", "32", "4096"], capture_output=True, text=True, timeout=60)
        assert r.returncode == 0 and r.stderr == "", (exe, r)
        lines = r.stdout.splitlines()
        assert len(lines) == 302 and lines[-2:] == ["refused -3 -3 -3 -3", "untouched 1"]
        it = iter(lines)
        for n in (2, 32, 4096):
            for t in range(1, 101):
                thr, gain = DM.schedule(t, n, k_sigma)
                want = "%d %d %08x %08x 0" % (n, t, thr.view(np.uint32), gain.view(np.uint32))
                assert next(it) == want, (exe, n, t)
    # what the schedule is: an exact mean up to N frames, then a fixed gain and threshold
    assert DM.schedule(1, 32, 40.0) == (F32(40), F32(0.5)) and DM.schedule(4, 32, 40.0) == (F32(20), F32(0.2))
    assert DM.schedule(31, 32, 40.0)[1] == DM.schedule(1000, 32, 40.0)[1] == F32(1) / F32(32)
    assert DM.schedule(32, 32, 40.0)[0] == DM.schedule(1000, 32, 40.0)[0] == F32(40) * np.sqrt(F32(1) / F32(32))


ACCEPTED = {"4": (4.0, 1, 32), "4,1": (4.0, 1, 32), "2.5,2": (2.5, 2, 32), "4,2,2": (4.0, 2, 2), "3,1,4096": (3.0, 1, 4096),
            "4,1,32": (4.0, 1, 32)}
REFUSED = ["0", "-1", "4,3", "4,", "nan", "x", "", "inf", "4,1x", "4x", "4,0", ",1", "4,12", "4,1,", "4,1,1", "4,1,4097",
           "4,1,0", "4,1,-5", "4,1,3x", "4,1,32,1", "4,,32", "4,1,032", "4,1,99999999999999999999", "4,1, 8", "4,1,+8"]
WANT = "%s: --defect-map %s: want K, K,R or K,R,N with K > 0, R = 1 or 2 and N = 2 .. 4096\n"


def test_grammar(drivers):
    for exe in drivers["args"]:
        texts = list(ACCEPTED) + REFUSED
        r = subprocess.run([exe, *texts], capture_output=True, text=True, timeout=60)
        assert r.returncode == 0 and r.stderr == "", (exe, r)
        lines = r.stdout.splitlines()
        assert len(lines) == len(texts)
        for text, line in zip(texts, lines):
            f = line.split()
            got = (float(f[1]), int(f[3]), int(f[5]), int(f[7]))
            assert got == ((*ACCEPTED[text], 0) if text in ACCEPTED else (-1.0, -1, -1, 1)), (text, line)


@pytest.mark.parametrize("tool", ["nlkalman-seq", "nlkalman-seq-gt", "nlkalman-lsmo-seq", "nlkalman-y4m"])
def test_tools_refuse_under_their_own_name(built, tool, tmp_path):
    exe = os.path.join(BIN, tool)
    if not os.path.exists(exe):
        built.build()
    out, missing = tmp_path / "out", tmp_path / "missing.y4m"
    for text in REFUSED:
        # (the seq tools make OUT, the stream tool opens IN, before either opens a device: neither happens)
        args = ["--defect-map", text, 20, missing] if tool == "nlkalman-y4m" else \
            ["--of", "tvl1", "--despike", "4", "--defect-map", text, "--sure", tmp_path / "%03d.tif", 1, 3, 20, out]
        r = subprocess.run([exe, *map(str, args)], capture_output=True, text=True, timeout=60)
        assert (r.returncode, r.stdout, r.stderr) == (1, "", WANT % (tool, text)), (text, r)
        assert not out.exists()
    # the option's place: after --despike, in front of --sure; an accepted value goes on to the missing frames
    r = subprocess.run([exe, "--defect-map", "4,2,16", str(tmp_path / "%03d.tif"), "1", "3", "20", str(out)]
                       if tool != "nlkalman-y4m" else [exe, "--defect-map", "4,2,16", "20", str(missing)],
                       capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "--defect-map" not in r.stderr and not out.exists(), r
    # ... and the usage text names it
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "--defect-map K[,R[,N]]" in r.stderr, r


def test_nlk_defects_usage(built):
    exe = os.path.join(BIN, "nlk-defects")
    if not os.path.exists(exe):
        built.build()
    for args in ([], ["4"], ["4", "20", "map"], ["-r", "3", "4", "20", "map", "a"], ["-1", "20", "map", "a"],
                 ["nan", "20", "map", "a"], ["4", "0", "map", "a"], ["4", "x", "map", "a"], ["-n", "1", "4", "20", "map", "a"],
                 ["-n", "4097", "4", "20", "map", "a"], ["-n", "8x", "4", "20", "map", "a"], ["-r", "2", "-n", "8", "4", "20", "map"]):
        r = subprocess.run([exe, *args], capture_output=True, text=True, timeout=60)
        assert r.returncode == 1 and r.stdout == "" and r.stderr.startswith("usage: "), (args, r)
        assert "[-r 1|2] [-n N] K SIGMA OUTMAP FILE..." in r.stderr
    assert not os.path.exists("map")


# ---------------------------------------------------------------- what it buys, on the CPU oracle

def test_oracle_the_map_recovers_what_despike_cannot_at_sigma_40(O, synth):
    """the chain of DESIGN.md §9's table on the CPU oracle, sigma 40, 21 stuck single sites, 24 frames, the flt2 PSNR
    and the RMSE at the sites over frames 16..23: the defect map leaves at most half of the dB that --despike 4 alone
    leaves and at most half of its RMSE at the sites (the table: despike leaves 0.62 of 0.65 dB and an RMSE of 31.5,
    the map -0.04 dB and 9.5); on a clean sensor the run is the run without the option, exactly"""
    sigma, last = 40.0, slice(16, 24)
    sites = DR.defect_sites(96, 64)
    clean, _, outs = DM.chain(O, synth, sigma)
    dsp, rd, _ = DM.chain(O, synth, sigma, DM.Cleaner(sigma, sites, k_despike=4.0), sites=sites)
    dmap, rmap, _ = DM.chain(O, synth, sigma, DM.Cleaner(sigma, sites, k_map=4.0), sites=sites)
    left_d, left_m = np.mean(clean[last]) - np.mean(dsp[last]), np.mean(clean[last]) - np.mean(dmap[last])
    print("sigma 40: despike leaves %.2f dB, the map %.2f dB; RMSE at the sites %.1f and %.1f" % (
        left_d, left_m, np.mean(rd[last]), np.mean(rmap[last])))
    assert left_d > 0.3 and left_m <= 0.5 * left_d
    assert np.mean(rmap[last]) <= 0.5 * np.mean(rd[last])
    prep = DM.Cleaner(sigma, None, k_map=4.0)
    same, _, outs2 = DM.chain(O, synth, sigma, prep)
    assert sum(prep.replaced) == 0
    assert same == clean and all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(outs, outs2))


# ---------------------------------------------------------------- the kernel

SHAPES = [(70, 53), (23, 9), (3, 3)]   # w ch no multiple of 64 and h none of 8; one row of waves on both borders; tiny
NFRAMES = 6


def _kernel_frames(w, h, ch, seed, radius=1):
    """six frames of noise (sigma 10) with stuck sites at a corner, on an edge and inside, and two NaN samples: one in
    the first frame (the mean starts at 0 there) and one in frame 3, on the inner site's ring (it blocks that
    replacement and leaves the mean there)"""
    rng = np.random.default_rng(seed)
    spots = sorted({(0, 0), (w - 1, h // 2), (w // 2, h - 1), (w // 2, h // 2), (w // 3, h // 3), (min(w - 1, 66), 2 * h // 3)})
    frames = []
    for t in range(NFRAMES):
        a = rng.normal(128, 10, (h, w, ch)).astype(F32)
        for n, (x, y) in enumerate(spots):
            a[y, x, :] = 255.0 if n % 2 == 0 else 0.0
        frames.append(a)
    frames[0][h - 1, 0, ch - 1] = np.nan
    frames[3][h // 2, max(w // 2 - radius, 0), 0] = np.nan
    return frames


@pytest.mark.gpu
@pytest.mark.parametrize("ch", [1, 3, 4])
@pytest.mark.parametrize("radius", [1, 2])
def test_gpu_kernel_gives_the_bits_of_the_restatement(ctx, ch, radius):
    total = blocked = 0
    for w, h in SHAPES:
        n = w * h * ch
        frames = _kernel_frames(w, h, ch, 1000 * w + h, radius)
        d_in, d_out, d_mean = ctx.alloc(4 * n), ctx.alloc(4 * n), [ctx.alloc(4 * n), ctx.alloc(4 * n)]
        d_out2, d_mean2 = ctx.alloc(4 * n), ctx.alloc(4 * n)
        d_map, d_cnt = ctx.alloc(n), ctx.alloc(4 * ch)
        m = None
        for t, v in enumerate(frames):
            what = (w, h, ch, radius, t)
            thr, gain = DM.schedule(t, 4, 40.0) if t else (F32(0), F32(1))     # N = 4: both branches of the schedule
            if t:
                assert ctx.defect_schedule(t, 4, 40.0) == (float(thr), float(gain)), what
            out, m_new, hit, counts = DM.step(v, m, thr, gain, radius)
            ctx._chk(ctx.L.nlk_h2d(ctx.h, d_in, v.ctypes.data, 4 * n))
            ctx._chk(ctx.L.nlk_h2d(ctx.h, d_map, np.full(n, 7, np.uint8).ctypes.data, n))          # every byte is written
            ctx._chk(ctx.L.nlk_h2d(ctx.h, d_cnt, np.full(ch, 77, np.uint32).ctypes.data, 4 * ch))   # the call zeroes them
            cur, prv = d_mean[(t + 1) & 1], d_mean[t & 1] if t else None
            ctx.defect_step(d_out, d_in, cur, prv, w, h, ch, thr, gain, radius, d_map, d_cnt)
            got = ctx.download(d_out, v.shape)
            got_m = ctx.download(cur, v.shape)
            assert DR.same_bits(got, out), what
            assert np.array_equal(_bits(got_m), _bits(m_new)), what
            assert np.array_equal(ctx.download(d_map, v.shape, np.uint8), hit.astype(np.uint8)), what
            assert np.array_equal(ctx.download(d_cnt, (ch,), np.uint32), counts), what
            assert np.array_equal(_bits(ctx.download(d_in, v.shape)), _bits(v)), what               # in is only read
            if t:
                assert np.array_equal(_bits(ctx.download(prv, v.shape)), _bits(m)), what            # ... and so is mean_in
            # the same call again, without map and counts: the same bits
            ctx.defect_step(d_out2, d_in, d_mean2, prv, w, h, ch, thr, gain, radius)
            assert np.array_equal(_bits(ctx.download(d_out2, v.shape)), _bits(got)), what
            assert np.array_equal(_bits(ctx.download(d_mean2, v.shape)), _bits(got_m)), what
            total += int(counts.sum())
            blocked += int(hit.sum()) - int(counts.sum())
            m = m_new
        for p in (d_in, d_out, d_out2, d_mean2, d_map, d_cnt, *d_mean):
            ctx.free(p)
    assert total > 20 and blocked > 0   # (the frames do have replaced samples, and hits that a NaN blocked)


@pytest.mark.gpu
def test_gpu_refused_calls_write_nothing_and_leave_the_context_working(ctx, built):
    w, h, ch = 37, 21, 3
    n = w * h * ch
    frames = _kernel_frames(w, h, ch, 3)
    v, m = frames[1], frames[0].copy()
    m[~np.isfinite(m)] = 0.0
    mark = np.full_like(v, -5.0)
    d_in, d_m = ctx.upload(v), ctx.upload(m)
    d_out, d_mo = ctx.upload(mark), ctx.upload(mark)
    d_map, d_cnt = ctx.upload(np.full(n, 7, np.uint8)), ctx.upload(np.full(ch, 77, np.uint32))
    L, EINVAL, thr, gain = ctx.L, -3, 40.0, 0.5

    def call(ctx_h=ctx.h, out=d_out, in_=d_in, mo=d_mo, mi=d_m, w_=w, h_=h, ch_=ch, r=1, thr_=thr, gain_=gain):
        return L.nlk_dev_defect_step(ctx_h, out, in_, mo, mi, d_map, d_cnt, w_, h_, ch_, r, thr_, gain_)

    refused = [dict(w_=0), dict(h_=0), dict(w_=-1), dict(ch_=0), dict(ch_=17), dict(r=0), dict(r=3), dict(thr_=-1.0),
               dict(thr_=float("nan")), dict(thr_=float("inf")), dict(ctx_h=None), dict(out=None), dict(in_=None),
               dict(mo=None), dict(gain_=0.0), dict(gain_=-0.5), dict(gain_=1.5), dict(gain_=float("nan")),
               dict(gain_=float("inf")),
               # no two of the four planes may be one, or overlap (here: by all but one sample)
               dict(out=d_in), dict(out=d_mo), dict(out=d_m), dict(in_=d_mo), dict(in_=d_m), dict(mo=d_m),
               dict(out=d_in + 4), dict(mo=d_m - 4), dict(out=d_mo + 4 * (n - 1)), dict(mi=None, out=d_in), dict(mi=None, mo=d_in)]
    for kw in refused:
        assert call(**kw) == EINVAL, kw
        if kw.get("ctx_h", 1) is not None:
            assert b"nlk_dev_defect_step" in L.nlk_last_error(ctx.h)
    ctx.sync()
    assert np.array_equal(ctx.download(d_out, v.shape), mark) and np.array_equal(ctx.download(d_mo, v.shape), mark)
    assert np.array_equal(_bits(ctx.download(d_in, v.shape)), _bits(v))
    assert np.array_equal(_bits(ctx.download(d_m, v.shape)), _bits(m))
    assert list(ctx.download(d_cnt, (ch,), np.uint32)) == [77] * ch
    assert np.all(ctx.download(d_map, (n,), np.uint8) == 7)
    out, m_new, hit, counts = DM.step(v, m, thr, gain, 1)
    assert call() == 0 and counts.sum() > 0
    assert DR.same_bits(ctx.download(d_out, v.shape), out)
    assert np.array_equal(_bits(ctx.download(d_mo, v.shape)), _bits(m_new))
    assert np.array_equal(ctx.download(d_cnt, (ch,), np.uint32), counts)
    assert np.array_equal(ctx.download(d_map, v.shape, np.uint8), hit.astype(np.uint8))
    for p in (d_in, d_m, d_out, d_mo, d_map, d_cnt):
        ctx.free(p)


# ---------------------------------------------------------------- the tools

W, H, SIGMA, K, NF = 96, 64, 20.0, 4.0, 4
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


def _cleaned(frames, sigma=SIGMA, **kw):
    prep = DM.Cleaner(sigma, None, **kw)
    return [prep(a) for a in frames], prep.replaced


@pytest.fixture(scope="module")
def seq_runs(built, synth, tmp_path_factory):
    """4 frames of 96 x 64 x 3 at sigma 20 with the 21 stuck sites, as a 4:4:4 stream holds them; `nlkalman-seq
    --defect-map 4` on them and `nlkalman-seq` on the frames the restatement cleaned (float TIFF), no smoother"""
    if not all(os.path.exists(os.path.join(BIN, t)) for t in ("nlkalman-seq", "nlkalman-y4m", "nlk-imgconv", "nlk-defects")):
        built.build()
    base = tmp_path_factory.mktemp("defect_map")
    sites = DR.defect_sites(W, H)
    pay = [yuv_ref.to_yuv(DR.plant(DM.noisy_frame(synth, SIGMA, t)[1], sites), FMT).tobytes() for t in range(NF)]
    frames = [yuv_ref.to_rgb(p, W, H, FMT) for p in pay]
    fixed, replaced = _cleaned(frames, k_map=K)
    print("replaced per frame:", replaced)
    assert replaced[0] == 0 and all(n >= 30 for n in replaced[1:])   # (of 63 samples, at thr = 80, 57, 46)
    env = dict(os.environ, NLK_DETERMINISTIC="1")
    src, ref = _tifs(base / "in", frames), _tifs(base / "fixed", fixed)
    got = run("nlkalman-seq", "--defect-map", 4, src, 1, NF, 20, base / "got", 1, "", "no", env=env)
    assert got.returncode == 0, got.stderr
    want = run("nlkalman-seq", ref, 1, NF, 20, base / "want", 1, "", "no", env=env)
    assert want.returncode == 0, want.stderr
    return base, sites, pay, frames, fixed, env


@pytest.mark.gpu
def test_gpu_seq_defect_map_is_seq_on_cleaned_frames(ctx, seq_runs):
    base = seq_runs[0]
    names = ["%s-%03d.tif" % (kind, i) for kind in ("flt1", "flt2") for i in range(1, NF + 1)] + ["bflo1-002.flo", "bocc1-003.png"]
    for name in names:
        assert (base / "got" / name).read_bytes() == (base / "want" / name).read_bytes(), name
    plain = run("nlkalman-seq", base / "in" / "%03d.tif", 1, NF, 20, base / "plain", 1, "", "no", env=seq_runs[5])
    assert plain.returncode == 0, plain.stderr
    # streaming: the first frame passes as it is, the second does not
    assert (base / "plain" / "flt2-001.tif").read_bytes() == (base / "got" / "flt2-001.tif").read_bytes()
    assert (base / "plain" / "flt2-002.tif").read_bytes() != (base / "got" / "flt2-002.tif").read_bytes()
    # a threshold nothing reaches is the run without the option: the step changes nothing else
    huge = run("nlkalman-seq", "--defect-map", "1e9,2,8", base / "in" / "%03d.tif", 1, NF, 20, base / "huge", 1, "", "no",
               env=seq_runs[5])
    assert huge.returncode == 0, huge.stderr
    for i in range(1, NF + 1):
        assert (base / "huge" / ("flt2-%03d.tif" % i)).read_bytes() == (base / "plain" / ("flt2-%03d.tif" % i)).read_bytes()


@pytest.mark.gpu
def test_gpu_defect_map_and_despike_compose_in_that_order(ctx, seq_runs):
    base, _, _, frames, _, env = seq_runs
    both, _ = _cleaned(frames, k_map=K, k_despike=K)
    ref = _tifs(base / "both_in", both)
    got = run("nlkalman-seq", "--despike", 4, "--defect-map", 4, base / "in" / "%03d.tif", 1, NF, 20, base / "both_got", 1, "",
              "no", env=env)
    assert got.returncode == 0, got.stderr
    want = run("nlkalman-seq", ref, 1, NF, 20, base / "both_want", 1, "", "no", env=env)
    assert want.returncode == 0, want.stderr
    for i in range(1, NF + 1):
        name = "flt2-%03d.tif" % i
        assert (base / "both_got" / name).read_bytes() == (base / "both_want" / name).read_bytes(), name
    assert (base / "both_got" / "flt2-001.tif").read_bytes() != (base / "got" / "flt2-001.tif").read_bytes()   # (despike saw frame 1)


@pytest.mark.gpu
def test_gpu_lsmo_and_gt_tools_take_the_option(ctx, seq_runs, tmp_path):
    """the other two tools of the same source: the option in its place (after --despike, in front of --sure) gives the
    flt2 files of nlkalman-seq --defect-map"""
    base, env = seq_runs[0], seq_runs[5]
    r = run("nlkalman-lsmo-seq", "--of", "tvl1", "--defect-map", "4,1,32", "--sure", base / "in" / "%03d.tif", 1, NF, 20,
            tmp_path / "lsmo", "", "no", env=env)
    assert r.returncode == 0, r.stderr
    for i in range(1, NF + 1):
        name = "flt2-%03d.tif" % i
        assert (tmp_path / "lsmo" / name).read_bytes() == (base / "got" / name).read_bytes(), name
    # gt: the noisy files exist, so they are read and used; the measures are against the clean frames
    synth = importlib.import_module("bwd-nlkalman_amd.synth")
    clean = _tifs(tmp_path / "clean", [synth.clean_frame(W, H, 3, t) for t in range(NF)])
    outs = {}
    for tag, opt in (("with", ["--defect-map", "4"]), ("without", [])):
        d = tmp_path / ("gt_" + tag)
        d.mkdir()
        for i in range(1, NF + 1):
            (d / ("%03d.tif" % i)).write_bytes((base / "in" / ("%03d.tif" % i)).read_bytes())
        r = run("nlkalman-seq-gt", *opt, clean, 1, NF, 20, d, "", "no", env=env)
        assert r.returncode == 0, r.stderr
        outs[tag] = [float(v) for v in r.stdout.split()]
    assert len(outs["with"]) == 2 and outs["with"][1] < outs["without"][1], outs   # flt2's MSE over the 4 frames


@pytest.mark.gpu
def test_gpu_y4m_and_sequence_filter_agree_with_seq(ctx, built, seq_runs):
    base, sites, pay, frames, fixed, env = seq_runs
    flt2 = [_decode(base / "want" / ("flt2-%03d.tif" % (t + 1))) for t in range(NF)]
    y = run("nlkalman-y4m", "--defect-map", 4, 20, input=yuv_ref.y4m_bytes(W, H, "444", pay), env=env, text=False)
    assert y.returncode == 0, y.stderr
    got = yuv_ref.y4m_parse(y.stdout)[4]
    assert got == [yuv_ref.to_yuv(a, FMT).tobytes() for a in flt2]
    off = run("nlkalman-y4m", 20, input=yuv_ref.y4m_bytes(W, H, "444", pay), env=env, text=False)
    assert off.returncode == 0 and yuv_ref.y4m_parse(off.stdout)[4] != got
    seq = importlib.import_module("bwd-nlkalman_amd.sequence")
    ctx.set_deterministic(True)
    try:
        sf = seq.SequenceFilter(ctx, W, H, 3, SIGMA, keep_history=False, defect_map=4, defect_counts=True)
        assert sf.defects == (4.0, 1, 32) and sf.defect_map is None
        m = None
        for t in range(NF):
            d = ctx.upload(frames[t])
            sf.push(d)
            assert np.array_equal(_bits(ctx.download(d, frames[t].shape)), _bits(frames[t]))   # not modified
            assert np.array_equal(_bits(sf.download_rgb(sf.flt2)), _bits(flt2[t])), t
            thr, gain = DM.schedule(t, 32, F32(K) * F32(SIGMA)) if t else (0.0, 1.0)
            _, m, hit, counts = DM.step(frames[t], m, thr, gain, 1)
            assert np.array_equal(ctx.download(sf.defect_map, hit.shape, np.uint8), hit.astype(np.uint8)), t
            assert np.array_equal(sf.defect_counts, counts), t
            ctx.free(d)
        assert seq.SequenceFilter(ctx, W, H, 3, SIGMA, defect_map=(2.5, 2)).defects == (2.5, 2, 32)
        assert seq.SequenceFilter(ctx, W, H, 3, SIGMA, defect_map=(2.5, 2, 8)).defects == (2.5, 2, 8)
        for bad in (0, -1, (4, 3), float("nan"), (4, 1, 1), (4, 1, 4097), (4, 1, 2.5), (), (4, 1, 8, 1), (4, 1, "x"),
                    (4, 1, None), "x"):
            with pytest.raises(ValueError):
                seq.SequenceFilter(ctx, W, H, 3, SIGMA, defect_map=bad)
        # the counts are on request only (their atomics cost time, and reading them waits for the device)
        sf = seq.SequenceFilter(ctx, W, H, 3, SIGMA, keep_history=False, defect_map=4)
        d = ctx.upload(frames[0])
        sf.push(d)
        ctx.free(d)
        assert sf.defect_map is not None and sf.d_defect[3] is None
        with pytest.raises(ValueError):
            sf.defect_counts
        # the option off: nothing of it exists
        sf = seq.SequenceFilter(ctx, W, H, 3, SIGMA, keep_history=False)
        d = ctx.upload(frames[0])
        sf.push(d)
        ctx.free(d)
        assert sf.defects is None and sf.defect_map is None and sf.d_defect is None
        with pytest.raises(ValueError):
            sf.defect_counts
    finally:
        ctx.set_deterministic(False)


@pytest.mark.gpu
def test_gpu_defect_map_under_vst(ctx, seq_runs):
    """under vst:A,B the step runs on the transformed frame at the run's sigma: a threshold nothing reaches is the run
    without the option, byte for byte; --defect-map 4 is that run on the first frame and differs from it afterwards at
    the planted sites"""
    base, sites, _, frames, _, env = seq_runs
    outs = {}
    for tag, opt in (("off", []), ("huge", ["--defect-map", "1e9"]), ("on", ["--defect-map", "4"])):
        r = run("nlkalman-seq", *opt, base / "in" / "%03d.tif", 1, NF, "vst:1,300", base / ("vst_" + tag), 1, "", "no", env=env)
        assert r.returncode == 0 and r.stdout.startswith("vst 1 300 "), (r.stdout, r.stderr)
        outs[tag] = r.stdout
    assert outs["off"] == outs["huge"] == outs["on"]
    mask = DR.site_mask((H, W), sites)
    for kind in ("flt1", "flt2"):
        for i in range(1, NF + 1):
            name = "%s-%03d.tif" % (kind, i)
            assert (base / "vst_huge" / name).read_bytes() == (base / "vst_off" / name).read_bytes(), name
            if i == 1:
                assert (base / "vst_on" / name).read_bytes() == (base / "vst_off" / name).read_bytes(), name
                continue
            d = np.abs(_decode(base / "vst_on" / name).astype(np.float64) - _decode(base / "vst_off" / name)).max(axis=2)
            print("%s: mean difference at the sites %.1f, elsewhere %.2f" % (name, d[mask].mean(), d[~mask].mean()))
            assert np.count_nonzero(d[mask] > 0) > 10 and d[mask].mean() > d[~mask].mean(), name


@pytest.mark.gpu
def test_gpu_defect_map_runs_in_the_stabilised_domain(ctx, built, seq_runs):
    """under vst:1,300 the step sees the transformed frames at the run's sigma S (the transform's scale): the run is the
    run at the plain sigma S on the frames that the restatement cleaned after the transform (Context.vst_forward), bit
    for bit in opponent space; and nlkalman-seq's files under vst are that SequenceFilter's frames. A step in front of
    the transform would test the frames as read at K S, another threshold in another domain"""
    base, _, _, frames, _, env = seq_runs
    seq = importlib.import_module("bwd-nlkalman_amd.sequence")
    ab = np.tile(np.asarray([1.0, 300.0], F32), (3, 1))
    S = float(built.vst_scale(ab))
    n = W * H * 3
    moved = []
    for a in frames:
        d_in, d_out = ctx.upload(a), ctx.alloc(4 * n)
        ctx.vst_forward(d_out, d_in, n, 3, ab, S)
        moved.append(ctx.download(d_out, a.shape))
        ctx.free(d_in)
        ctx.free(d_out)
    cleaned, replaced = _cleaned(moved, sigma=S, k_map=K)
    print("sigma of the run %.6g; replaced per frame in the stabilised domain: %s" % (S, replaced))
    assert all(r > 0 for r in replaced[1:])
    as_read, _ = _cleaned(frames, sigma=S, k_map=K)   # (the other order, the step on the frames as read, replaces others)
    here = [_bits(a) != _bits(b) for a, b in zip(cleaned, moved)]
    there = [_bits(a) != _bits(b) for a, b in zip(as_read, frames)]
    assert any(a.any() for a in here) and any(not np.array_equal(a, b) for a, b in zip(here, there))
    r = run("nlkalman-seq", "--defect-map", 4, base / "in" / "%03d.tif", 1, NF, "vst:1,300", base / "vst_dom", 1, "", "no", env=env)
    assert r.returncode == 0 and r.stdout.split()[-1] == "%.9g" % S, (r.stdout, r.stderr)
    ctx.set_deterministic(True)
    try:
        got = seq.SequenceFilter(ctx, W, H, 3, ("vst", 1.0, 300.0), keep_history=False, defect_map=4)
        want = seq.SequenceFilter(ctx, W, H, 3, S, keep_history=False)
        for t in range(NF):
            d, e = ctx.upload(frames[t]), ctx.upload(cleaned[t])
            got.push(d)
            want.push(e)
            ctx.free(d)
            ctx.free(e)
            assert np.array_equal(_bits(ctx.download(got.flt2, frames[t].shape)), _bits(ctx.download(want.flt2, frames[t].shape))), t
            tool = _decode(base / "vst_dom" / ("flt2-%03d.tif" % (t + 1)))
            assert np.array_equal(_bits(got.download_rgb(got.flt2)), _bits(tool)), t
    finally:
        ctx.set_deterministic(False)


@pytest.mark.gpu
def test_gpu_nlk_defects_prints_the_counts_of_the_restatement(ctx, seq_runs, tmp_path):
    base, _, _, frames, _, _ = seq_runs
    files = [base / "in" / ("%03d.tif" % i) for i in range(1, NF + 1)]
    for opt, radius, window in (([], 1, 32), (["-r", 2, "-n", 2], 2, 2)):
        res = DM.run(frames, F32(K) * F32(SIGMA), radius, window)
        out = tmp_path / ("map%d.tif" % radius)
        r = run("nlk-defects", *opt, 4, 20, out, *files)
        assert (r.returncode, r.stderr) == (0, ""), r
        assert r.stdout == "".join(" ".join(str(int(c)) for c in counts) + "\n" for _, _, counts in res)
        assert sum(int(c.sum()) for _, _, c in res) > 60
        assert np.array_equal(_decode(out), np.where(res[-1][1], F32(255), F32(0)))
    r = run("nlk-defects", 4, 20, tmp_path / "no.tif", files[0], tmp_path / "missing.tif")
    assert r.returncode == 1 and "cannot read" in r.stderr and not (tmp_path / "no.tif").exists()
