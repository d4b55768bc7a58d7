"""Signal-dependent noise, var(z | y) = a y + b: the noise-curve estimator (nlk_dev_estimate_noise_curve,
Context.estimate_noise_curve, bin/nlk-sigma --curve), the variance-stabilising transform (nlk_dev_vst_forward /
_inverse, nlk_vst_scale), nlk_dev_noise_affine and SIG = vst of nlkalman-seq / SequenceFilter, against
tests/curve_ref.py, the float64 numpy restatement of the definitions in include/nlk_hip.h.

Unless a test says otherwise its input is synth.noise_affine(synth.clean_frame(w, h, ch), (0.5, 4), seed=w + h).

Bars.
* Estimator parity: the block counts N_q, n_q are exact; m_q, v_q, a and b agree with the restatement within 1e-4
  relative (plus 1e-6 absolute on a): the rounding argument of test_sigma.py's docstring (an f32 coefficient carries
  <= 5e-6 relative on its square, less on a mean), with 10x margin for the line's b = vbar - a mbar, which subtracts
  two numbers ~10x its size (measured: m_q 6e-8, v_q 1.8e-6, a and b 1.2e-5 at worst, and 6.3e-5 on the 12 x 8
  input, whose line goes through two bins of one block each). Exact counts need two preconditions, asserted for every parity input without a GPU: the
  relative gap between the K_q-th and the next low-frequency energy is >= 1e-4 in every kept bin (f32 rounding of
  that energy is ~1e-6), and no block mean lies within 1e-9 of a bin edge (the mean is the same double on both sides:
  64 additions in raster order; the bin expression may differ by an ulp, ~3e-14 at 255).
* Estimator accuracy: on 256 x 192 x 3 frames with (a, b) in {(0.5, 4), (0.2, 25), (0, 400)} and seeds 1, 2, 3 the
  estimated sqrt(a m + b) over the true one reads 0.9788 ... 1.0123 at m = 100 and 160 (worst distance from 1: 0.0212)
  and 0.9498 ... 1.0437 at m = 40 (worst: 0.0502) in the restatement. The bars are those plus a quarter: 0.0265 and
  0.0628. ((a, b) = (1, 1) is left out: its dark end reads 0.917.)
* Transform parity: max-abs <= 1e-3 on the 0..255 scale: f32 eps x 255 x about 10 operations ~ 3e-4, with a margin
  of 3x. The same bar for the round trip inverse(mode 0) of forward.
* nlk_dev_noise_affine: within 1 ulp of synth.noise_affine (double arithmetic on both sides, one rounding to float;
  log / cos of the device library differ from libm in the last bits of the double).
* The filter on stabilised frames (CPU oracle, FLT1 -> FLT2 at zero flow on three noisy copies of one scene): the
  table of DESIGN.md §9, measured with other noise seeds: every flt2 PSNR within 1 dB of the table's, and the gain of
  the transform over one sigma from sigma_ref.estimate at least half the table's gain, frame by frame.
* SIG = vst on the GPU: the mean flt2 PSNR of the vst run is at least that of the auto run on the same files plus
  half the mean gain the oracle measured on those frames (about 1.1 dB of 2.2)."""
import functools
import importlib
import math
import os
import re
import subprocess

import numpy as np
import pytest

import curve_ref
import sigma_ref
from test_cli import rpfm, server, sock_dir, wpfm  # noqa: F401  (sock_dir: a fixture)
from test_sigma import _holed

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "bwd-nlkalman_amd", "bin")
GPU_STEP_S = 300   # time limit of one tool run on the GPU
AB = (0.5, 4.0)


def run(tool, *args, **kw):
    kw.setdefault("timeout", GPU_STEP_S)
    return subprocess.run([os.path.join(BIN, tool), *map(str, args)], capture_output=True, text=True, **kw)


@pytest.fixture(scope="module")
def curve_tools(built):
    if not all(os.path.exists(os.path.join(BIN, t)) for t in ("nlk-sigma", "nlkalman-seq", "nlkalman-seq-gt",
                                                              "nlk-server", "nlk-imgconv")):
        built.build()
    return BIN


def _synth():
    return importlib.import_module("bwd-nlkalman_amd.synth")


# (w, h, ch, holed, parameters); the comments say what a case reaches
PARITY = [
    (8, 8, 1, False, dict(nmin=1)),              # one block, one bin
    (12, 8, 1, False, dict(nmin=1)),             # two blocks
    (12, 8, 1, False, {}),                       # every bin dropped: NaN
    (100, 9, 2, False, dict(nmin=1)),            # K = N, two channels, one block row
    (70, 53, 3, False, {}),                      # ragged: w - 8 and h - 8 are no multiples of 4
    (96, 64, 3, False, {}),
    (96, 64, 3, True, {}),                       # skipped blocks
    (70, 53, 3, False, dict(step=1)),
    (70, 53, 3, False, dict(step=8, nmin=4, kmin=4)),   # (step 8: the blocks come straight from the image)
    (96, 64, 3, False, dict(nbins=1)),
    (96, 64, 3, False, dict(nbins=64, nmin=1)),  # histograms in HBM; bins of one block have K = N
    (96, 64, 3, False, dict(lo=64.0, hi=192.0)),  # blocks skipped by range
    (256, 192, 1, False, dict(step=1, nbins=17)),  # 23 workgroup shares (more than the final kernel's 4 quarters), HBM histograms
    (352, 240, 1, False, dict(step=1, frac=0.01)),  # 40 shares: more than its 32 partials in flight
]
PARITY_IDS = ["%dx%dx%d%s%s" % (w, h, ch, "-holed" if holed else "", "".join(f"-{k}{v}" for k, v in p.items()))
              for w, h, ch, holed, p in PARITY]


@functools.lru_cache(maxsize=None)
def _input(w, h, ch, holed=False):
    synth = _synth()
    im = synth.noise_affine(synth.clean_frame(w, h, ch), AB, seed=w + h)
    im = _holed(im) if holed else im
    im.setflags(write=False)
    return im


@functools.lru_cache(maxsize=None)
def _reference(case):
    w, h, ch, holed, p = PARITY[case]
    return curve_ref.estimate(_input(w, h, ch, holed), **p)


@functools.lru_cache(maxsize=None)
def _accuracy_frame(ab, seed):
    synth = _synth()
    return synth.noise_affine(synth.clean_frame(256, 192, 3), ab, seed)


ACCURACY_BAR = {40: 0.0628, 100: 0.0265, 160: 0.0265}


def _assert_accurate(est, ab, what):
    est = np.asarray(est, np.float64)
    for m, bar in ACCURACY_BAR.items():
        ratio = np.sqrt(est[:, 0] * m + est[:, 1]) / math.sqrt(ab[0] * m + ab[1])
        print(f"{what}: m = {m}: estimated / true deviation per channel {np.round(ratio, 4)}")
        assert np.all(np.abs(ratio - 1) <= bar), (what, m)


# ---- the oracle's filter on stabilised frames: three noisy copies of one scene, FLT1 -> FLT2 at zero flow

SEQ_SEED = 100   # frame t: noise_affine(clean, ab, SEQ_SEED + t)
# flt2 PSNR of frames 1 / 2 / 3: one sigma from sigma_ref.estimate | per-channel transform, curve of frame 1
TABLE = {(0.5, 4.0): ((39.37, 39.77, 39.30), (40.92, 41.93, 42.07)),
         (0.2, 25.0): ((41.09, 41.93, 41.80), (41.67, 42.74, 42.91)),
         (1.0, 1.0): ((36.66, 36.86, 36.30), (38.87, 39.72, 39.73))}


def _seq_frames(ab):
    synth = _synth()
    clean = synth.clean_frame(96, 64, 3)
    return clean, [synth.noise_affine(clean, ab, SEQ_SEED + t) for t in range(3)]


@functools.lru_cache(maxsize=None)
def _oracle_psnr(ab):
    """-> (flt2 PSNR per frame at sigma = sigma_ref.estimate(frame 1), the same on frames stabilised with the curve
    curve_ref.estimate finds on frame 1, transformed back with mode 1)"""
    import oracle as O
    O.build()
    synth = _synth()
    clean, frames = _seq_frames(ab)

    def recursion(fr, sigma, back):
        p1, p2 = O.default_params(sigma, O.FLT1), O.default_params(sigma, O.FLT2)
        f1 = f2 = None
        out = []
        for f in fr:
            o = O.rgb2opp(f)
            f1 = O.filter_frame(o, f1, None, sigma, p1, nthreads=4)
            f2 = O.filter_frame(o, f2, f1, sigma, p2, nthreads=4)
            out.append(synth.psnr(back(O.opp2rgb(f2)), clean))
        return out
    auto = recursion(frames, sigma_ref.estimate(frames[0])["sigma"], lambda x: x)
    est = curve_ref.estimate(frames[0])["ab"].astype(np.float32).astype(np.float64)
    s = curve_ref.vst_scale(est)
    stab = [curve_ref.vst_forward(f, est, s).astype(np.float32) for f in frames]
    gat = recursion(stab, s, lambda x: curve_ref.vst_inverse(x, est, s, 1))
    return auto, gat


# ------------------------------------------------------------ without a GPU

def test_the_feature_is_exported(built, curve_tools):
    L = built.hip()
    names = ("nlk_curve_default_params", "nlk_dev_estimate_noise_curve", "nlk_vst_scale", "nlk_dev_vst_forward",
             "nlk_dev_vst_inverse", "nlk_dev_noise_affine")
    for name in names:
        assert hasattr(L, name) and name in built.HIP_SYMBOLS, name
    for name in ("estimate_noise_curve", "vst_forward", "vst_inverse", "noise_affine"):
        assert hasattr(built.Context, name), name
    p = built.curve_params()
    assert isinstance(p, built.CurveParams)
    assert (p.step, p.frac, p.kmin, p.low_max, p.high_min, p.nbins, p.lo, p.hi, p.nmin) == \
        (4, float(np.float32(0.1)), 32, 5, 8, 16, 0.0, 256.0, 32)
    assert built.curve_params(nbins=8, lo=16.0).nbins == 8
    with pytest.raises(TypeError):
        built.curve_params(bins=8)
    # the scale: a host function; (0.5, 4) gives s ~ 6.75
    assert abs(built.vst_scale(AB, 3) - 6.747) < 1e-3
    assert abs(built.vst_scale([(0.5, 4), (0.2, 25), (0, 400)]) / curve_ref.vst_scale([(0.5, 4), (0.2, 25), (0, 400)]) - 1) < 1e-6
    for bad in ((0, 0), (-1, 4), (0.5, -1), (float("nan"), 1), (float("inf"), 1)):
        with pytest.raises(ValueError):
            built.vst_scale(bad, 3)
    r = run("nlk-sigma")
    assert r.returncode == 1 and r.stdout == ""
    assert r.stderr.startswith("usage: ") and "--curve" in r.stderr and "--nbins" in r.stderr and "--nmin" in r.stderr
    assert r.stderr.count("\n") == 1
    r = run("nlk-sigma", "--nbins", "8", "x.pfm")     # a curve option without --curve
    assert r.returncode == 1 and r.stdout == "" and r.stderr.startswith("usage: ")
    r = run("nlk-sigma", "--curve")                   # no file
    assert r.returncode == 1 and r.stdout == "" and r.stderr.startswith("usage: ")


def test_restatement_definition():
    """The pieces of the definition on inputs whose answer is known."""
    c = curve_ref.dct8()
    i, j = np.mgrid[0:8, 0:8]
    # one block: one bin, a = 0, b = the median of the 28 high squares
    b = _input(8, 8, 1)
    y2 = (c @ b[:, :, 0].astype(np.float64) @ c.T) ** 2
    r = curve_ref.estimate(b, nmin=1)
    q = int(b.astype(np.float64).mean() // 16)
    assert r["bins"][0, :, 0].sum() == 1 and r["bins"][0, q, :2].tolist() == [1, 1]
    assert r["ab"][0, 0] == 0 and math.isclose(r["ab"][0, 1], np.median(y2[i + j >= 8]), rel_tol=1e-12)
    assert math.isclose(r["bins"][0, q, 2], b.astype(np.float64).mean(), rel_tol=1e-14)
    # with the default nmin the bin is dropped: nothing is kept
    r = curve_ref.estimate(b)
    assert np.isnan(r["ab"]).all() and r["bins"][0, q, :2].tolist() == [1, 0]
    # one bin over everything with sigma_ref's selection: its estimator
    for im in (_input(96, 64, 3), _input(96, 64, 3, True), _input(70, 53, 3)):
        want = sigma_ref.estimate(im)
        got = curve_ref.estimate(im, nbins=1, lo=-1e6, hi=1e6, nmin=1, frac=0.05, kmin=64)
        assert got["bins"][:, 0, :2].tolist() == want["counts"].tolist()
        assert np.all(got["ab"][:, 0] == 0) and np.allclose(got["ab"][:, 1], want["sigma_ch"] ** 2, rtol=1e-12)
    # the line: exact on points of a line; a falling line gives the weighted mean; b < 0 refits through the origin
    a, b_ = curve_ref.fit([3, 5, 2], [10, 20, 40], [9, 14, 24])
    assert math.isclose(a, 0.5, rel_tol=1e-12) and math.isclose(b_, 4.0, rel_tol=1e-12)
    assert curve_ref.fit([3, 5], [10, 20], [9, 5]) == (0.0, (3 * 9 + 5 * 5) / 8)
    assert curve_ref.fit([3, 0, 0], [10, 20, 30], [9, 1, 1]) == (0.0, 9.0)          # one bin kept
    assert curve_ref.fit([3, 5], [10, 10], [9, 5]) == (0.0, (3 * 9 + 5 * 5) / 8)    # no spread of the means
    n, m, v = np.array([4.0, 4.0]), np.array([10.0, 20.0]), np.array([2.0, 12.0])   # the free line: v = m - 8
    a, b_ = curve_ref.fit(n, m, v)
    assert b_ == 0.0 and math.isclose(a, (n * m * v).sum() / (n * m * m).sum(), rel_tol=1e-15) and 0.5 < a < 1
    assert all(math.isnan(x) for x in curve_ref.fit([0, 0], [1, 2], [3, 4]))
    # a NaN sample removes the blocks that hold it, an all-NaN channel gives NaN
    im = np.array(_input(96, 64, 3)[:, :, :1])
    im[20, 30] = np.nan
    assert curve_ref.estimate(im)["bins"][0, :, 0].sum() == 23 * 15 - 4
    r = curve_ref.estimate(np.full((16, 16, 1), np.nan), nmin=1)
    assert np.isnan(r["ab"]).all() and r["bins"][0, :, :2].sum() == 0
    # blocks outside [lo, hi) are skipped
    r = curve_ref.estimate(_input(96, 64, 3), lo=64.0, hi=192.0)
    assert 0 < r["bins"][0, :, 0].sum() < 23 * 15
    # K per bin: frac is a float32 before it is multiplied
    assert math.ceil(float(np.float32(0.1)) * 100) == 11 and math.ceil(0.1 * 100) == 10


@pytest.mark.parametrize("ab", [(0.5, 4.0), (0.2, 25.0), (0.0, 400.0)], ids=lambda ab: "a%g-b%g" % ab)
def test_restatement_accuracy(ab):
    for seed in (1, 2, 3):
        _assert_accurate(curve_ref.estimate(_accuracy_frame(ab, seed))["ab"], ab, f"(a, b) = {ab} seed {seed}")


@pytest.mark.parametrize("case", range(len(PARITY)), ids=PARITY_IDS)
def test_preconditions_of_the_exact_counts(case):
    """(no near-tie at a selection threshold, no block mean at a bin edge)"""
    r = _reference(case)
    print(f"{PARITY_IDS[case]}: relative gap {r['gap']:.3e}, distance from a bin edge {r['edge']:.3e}")
    assert r["gap"] >= 1e-4 and r["edge"] >= 1e-9


def test_restatement_of_the_transform():
    rng = np.random.default_rng(5)
    y = rng.uniform(0, 255, (40, 30, 3))
    ab = [(0.5, 4.0), (0.2, 25.0), (0.0, 400.0)]
    s = curve_ref.vst_scale(ab)
    g = curve_ref.vst_forward(y, ab, s)
    assert np.abs(curve_ref.vst_inverse(g, ab, s, 0) - y).max() <= 1e-9
    # the textbook form where it is stable
    a, b = 0.5, 4.0
    u0 = 0.375 * a * a + b
    assert np.allclose(g[:, :, 0], 2 * s / a * (np.sqrt(a * y[:, :, 0] + u0) - math.sqrt(u0)), rtol=1e-12)
    # a -> 0 is continuous with s y / sqrt(b), and a = 0 is that
    assert np.allclose(g[:, :, 2], s * y[:, :, 2] / 20.0, rtol=1e-14, atol=0)
    assert np.abs(curve_ref.vst_forward(y, (1e-9, 400.0), s) - s * y / 20.0).max() <= 1e-6
    # below u = 0 the transform stays at its value there, and the inverse returns -u0 / a; NaN passes through
    low = curve_ref.vst_forward(np.array([[-9.0, -1e3, np.nan]]), (a, b), s)
    assert low[0, 0] == low[0, 1] == -2 * s * math.sqrt(u0) / a and math.isnan(low[0, 2])
    back = curve_ref.vst_inverse(np.array([[low[0, 0], 10 * low[0, 0], np.nan]]), (a, b), s, 0)
    assert np.allclose(back[0, :2], -u0 / a, rtol=1e-12) and math.isnan(back[0, 2])
    # mode 1 adds a positive, decreasing term of at most a (1/4 + ...) at D's floor, nothing for a = 0
    d1 = curve_ref.vst_inverse(g, ab, s, 1) - curve_ref.vst_inverse(g, ab, s, 0)
    assert np.all(d1[:, :, 2] == 0) and np.all(d1[:, :, :2] > 0) and d1[:, :, 0].max() < 0.5 * 0.5
    # the scale: (0.5, 4) gives ~ 6.75, and the transform of 0..255 then spans 255
    s3 = curve_ref.vst_scale(AB, 3)
    assert abs(s3 - 6.747) < 1e-3
    assert math.isclose(curve_ref.vst_forward(np.array([[255.0]]), AB, s3)[0, 0], 255.0, rel_tol=1e-12)
    # the noise of a transformed flat frame has deviation s
    synth = _synth()
    flat = np.full((192, 256, 3), 128.0, np.float32)
    t = curve_ref.vst_forward(synth.noise_affine(flat, AB, 3), AB, s3)
    print("deviation of the transformed flat frame / s:", np.round(t.std(axis=(0, 1)) / s3, 4))
    assert np.all(np.abs(t.std(axis=(0, 1)) / s3 - 1) <= 0.02)


def test_noise_affine_restatement():
    synth = _synth()
    clean = synth.clean_frame(70, 53, 3)
    x, y = synth.noise_affine(clean, (0.0, 400.0), 7), synth.awgn(clean, 20.0, 7)
    assert np.abs(x.view(np.int32).astype(np.int64) - y.view(np.int32)).max() <= 1
    # per channel pairs, and a variance that would be negative gives no noise
    z = synth.noise_affine(clean, [(0.0, 400.0), (0.0, 0.0), (-1.0, 0.0)], 7)
    assert np.array_equal(z[:, :, 0], x[:, :, 0]) and np.array_equal(z[:, :, 1:], clean[:, :, 1:])
    # the deviation follows the signal
    flat = np.stack([np.full((96, 128), v, np.float32) for v in (10.0, 100.0, 200.0)], axis=2)
    sd = (synth.noise_affine(flat, AB, 1) - flat).std(axis=(0, 1))
    assert np.all(np.abs(sd / np.sqrt(0.5 * np.array([10.0, 100.0, 200.0]) + 4) - 1) <= 0.03)


@pytest.mark.parametrize("ab", list(TABLE), ids=lambda ab: "a%g-b%g" % ab)
def test_oracle_filters_stabilised_frames_better(ab):
    auto, gat = _oracle_psnr(ab)
    t_auto, t_gat = TABLE[ab]
    print(f"(a, b) = {ab}: flt2 PSNR at one sigma {np.round(auto, 2)}, stabilised {np.round(gat, 2)}")
    for k in range(3):
        assert abs(auto[k] - t_auto[k]) <= 1.0 and abs(gat[k] - t_gat[k]) <= 1.0, k
        assert gat[k] - auto[k] >= 0.5 * (t_gat[k] - t_auto[k]), k


# ------------------------------------------------------------ on the GPU

def _estimate(ctx, im, **p):
    h, w, ch = im.shape
    d = ctx.upload(im)
    try:
        return ctx.estimate_noise_curve(d, w, h, ch, **p)
    finally:
        ctx.free(d)


def _bits(x):
    return np.asarray(x, np.float32).view(np.uint32).tolist()


def _close(got, want, rel=1e-4, abs_=0.0):
    """NaN where the restatement has NaN, else within the bar"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    nan = np.isnan(want)
    return bool(np.array_equal(np.isnan(got), nan) and np.all(np.abs(got - want)[~nan] <= rel * np.abs(want)[~nan] + abs_))


def _assert_matches(got, want, what):
    ab, bins = got
    wb = want["bins"]
    rel = lambda g, w: float(np.nanmax(np.abs(np.asarray(g, np.float64) / w - 1), initial=0))  # noqa: E731
    with np.errstate(invalid="ignore", divide="ignore"):
        print(f"{what}: kept bins {(wb[:, :, 1] > 0).sum(axis=1).tolist()}, (a, b) {np.asarray(ab).tolist()}, worst "
              f"relative difference m_q {rel(bins['mean'], wb[:, :, 2]):.2e} v_q {rel(bins['var'], wb[:, :, 3]):.2e} "
              f"a, b {rel(ab, want['ab']):.2e}")
    assert bins["nblocks"].tolist() == wb[:, :, 0].astype(int).tolist()
    assert bins["nsel"].tolist() == wb[:, :, 1].astype(int).tolist()
    assert _close(bins["mean"], wb[:, :, 2]) and _close(bins["var"], wb[:, :, 3])
    assert _close(ab[:, 0], want["ab"][:, 0], abs_=1e-6) and _close(ab[:, 1], want["ab"][:, 1])


@pytest.mark.gpu
@pytest.mark.parametrize("case", range(len(PARITY)), ids=PARITY_IDS)
def test_gpu_parity_with_the_restatement(ctx, case):
    w, h, ch, holed, p = PARITY[case]
    _assert_matches(_estimate(ctx, _input(w, h, ch, holed), **p), _reference(case), PARITY_IDS[case])


@pytest.mark.gpu
def test_gpu_same_bits_on_every_call(ctx):
    im = _input(96, 64, 3)
    a = _estimate(ctx, im)
    b = _estimate(ctx, im)
    _estimate(ctx, _accuracy_frame(AB, 1), step=1)        # a larger frame grows the scratch in between
    c = _estimate(ctx, im)
    for other in (b, c):
        assert _bits(a[0]) == _bits(other[0]) and a[1].tobytes() == other[1].tobytes()


@pytest.mark.gpu
def test_gpu_refused_parameters(ctx, built):
    d = ctx.upload(np.zeros((20, 12, 1), np.float32))
    for bad in (dict(nbins=0), dict(nbins=65), dict(lo=10.0, hi=10.0), dict(lo=20.0, hi=10.0), dict(nmin=0),
                dict(step=0), dict(frac=0.0)):
        with pytest.raises(built.NlkError, match="rc=-3"):
            ctx.estimate_noise_curve(d, 12, 20, 1, **bad)
    with pytest.raises(built.NlkError, match="rc=-3"):
        ctx.estimate_noise_curve(d, 7, 20, 1)
    ctx.free(d)
    _assert_matches(_estimate(ctx, _input(8, 8, 1), nmin=1), _reference(0), "8x8x1 after the refusals")
    # an all-NaN channel beside a sound one
    im = np.array(np.broadcast_to(_input(96, 64, 3)[:, :, :1], (64, 96, 2)))
    im[:, :, 1] = np.nan
    ab, bins = _estimate(ctx, im)
    want = curve_ref.estimate(im)
    assert np.isnan(ab[1]).all() and bins["nblocks"][1].sum() == 0 and _close(ab[0], want["ab"][0], abs_=1e-6)


@pytest.mark.gpu
def test_gpu_one_bin_is_the_sigma_estimator(ctx):
    for im in (_input(96, 64, 3), _input(96, 64, 3, True)):
        h, w, ch = im.shape
        d = ctx.upload(im)
        _, sigma_ch, counts = ctx.estimate_sigma(d, w, h, ch)
        ab, bins = ctx.estimate_noise_curve(d, w, h, ch, nbins=1, lo=-1e6, hi=1e6, nmin=1, frac=0.05, kmin=64)
        ctx.free(d)
        assert np.stack([bins["nblocks"][:, 0], bins["nsel"][:, 0]], axis=1).tolist() == counts.tolist()
        assert np.all(ab[:, 0] == 0) and _close(ab[:, 1], sigma_ch.astype(np.float64) ** 2)


@pytest.mark.gpu
def test_gpu_accuracy(ctx):
    """the frame made and measured on the device"""
    synth = _synth()
    clean = synth.clean_frame(256, 192, 3)
    d = ctx.upload(clean)
    ctx.noise_affine(d, d, clean.size, 3, AB, 1)
    ab, _ = ctx.estimate_noise_curve(d, 256, 192, 3)
    ctx.free(d)
    _assert_accurate(ab, AB, "device frame, (0.5, 4) seed 1")


VST_AB = [[(0.5, 4.0)] * 3, [(0.2, 25.0), (1.0, 1.0), (0.05, 0.0)], [(0.0, 400.0), (0.0, 1.0), (0.5, 4.0)]]


def _vst_input():
    """a noisy frame with negative samples, samples below u = 0 for every pair with a > 0, and a NaN"""
    im = np.array(_input(70, 53, 3))
    im[5:15, 10:40] -= 80.0
    im[20:24, 3:50] = np.linspace(-30.0, 2.0, 47, dtype=np.float32)[None, :, None]
    im[30:32, 5:20] = -200.0
    im[40, 7, 1] = np.nan
    return im


@pytest.mark.gpu
@pytest.mark.parametrize("ab", VST_AB, ids=["same", "mixed", "a0"])
def test_gpu_transform_parity(ctx, built, ab):
    im = _vst_input()
    n, s = im.size, built.vst_scale(ab)
    ab32 = np.asarray(ab, np.float32).astype(np.float64)
    u = ab32[:, 0] * im.astype(np.float64) + (0.375 * ab32[:, 0] ** 2 + ab32[:, 1])
    assert all((u[:, :, c] < 0).any() for c in range(3) if ab32[c, 0] > 0) and (im < 0).any()
    want = curve_ref.vst_forward(im, ab32, s)
    d_in, d_out = ctx.upload(im), ctx.alloc(im.nbytes)
    ctx.vst_forward(d_out, d_in, n, 3, ab, s)
    fwd = ctx.download(d_out, im.shape)
    ctx.vst_forward(d_in, d_in, n, 3, ab, s)            # in place
    assert np.array_equal(ctx.download(d_in, im.shape), fwd, equal_nan=True)
    assert np.array_equal(np.isnan(fwd), np.isnan(im))
    print(f"forward: max-abs difference {np.nanmax(np.abs(fwd - want)):.2e}, range {np.nanmin(fwd):.1f} .. {np.nanmax(fwd):.1f}")
    assert np.nanmax(np.abs(fwd - want)) <= 1e-3
    # the inverse of the same float32 image, also of values below the transform's floor
    g = fwd.copy()
    g[0, :8] = np.nanmin(fwd, axis=(0, 1)) * 3 - 1
    ctx.free(d_in)
    d_in = ctx.upload(g)
    for mode in (0, 1):
        want = curve_ref.vst_inverse(g, ab32, s, mode)
        ctx.vst_inverse(d_out, d_in, n, 3, ab, s, mode)
        inv = ctx.download(d_out, im.shape)
        assert np.array_equal(np.isnan(inv), np.isnan(g))
        print(f"inverse mode {mode}: max-abs difference {np.nanmax(np.abs(inv - want)):.2e}")
        assert np.nanmax(np.abs(inv - want)) <= 1e-3
    ctx.vst_inverse(d_in, d_in, n, 3, ab, s, 1)          # in place
    assert np.array_equal(ctx.download(d_in, im.shape), inv, equal_nan=True)
    # the round trip, where the forward transform is not at its floor
    d_f = ctx.upload(fwd)
    ctx.vst_inverse(d_f, d_f, n, 3, ab, s, 0)
    back = ctx.download(d_f, im.shape)
    live = u > 0
    print(f"round trip: max-abs difference {np.abs(back - im)[live].max():.2e}")
    assert live.sum() > 0.9 * n and np.abs(back - im)[live].max() <= 1e-3
    for p in (d_in, d_out, d_f):
        ctx.free(p)


@pytest.mark.gpu
def test_gpu_transform_refusals(ctx, built):
    d = ctx.upload(np.zeros((8, 8, 3), np.float32))
    for ab in ((0.0, 0.0), (-0.1, 4.0), (0.5, -1.0), (float("nan"), 4.0), (0.5, float("inf"))):
        with pytest.raises(built.NlkError, match="rc=-3"):
            ctx.vst_forward(d, d, 192, 3, ab, 1.0)
        with pytest.raises(built.NlkError, match="rc=-3"):
            ctx.vst_inverse(d, d, 192, 3, ab, 1.0)
    with pytest.raises(built.NlkError, match="rc=-3"):
        ctx.vst_forward(d, d, 192, 3, AB, 0.0)
    with pytest.raises(built.NlkError, match="rc=-3"):
        ctx.vst_inverse(d, d, 192, 3, AB, 1.0, mode=2)
    ctx.vst_forward(d, d, 192, 3, AB, 1.0)
    assert np.all(ctx.download(d, (8, 8, 3)) == 0)
    ctx.free(d)


@pytest.mark.gpu
def test_gpu_noise_affine(ctx):
    synth = _synth()
    clean = synth.clean_frame(70, 53, 3)
    ab = [(0.5, 4.0), (0.0, 400.0), (0.2, 25.0)]
    want = synth.noise_affine(clean, ab, 9)
    d = ctx.upload(clean)
    d_out = ctx.alloc(clean.nbytes)
    ctx.noise_affine(d_out, d, clean.size, 3, ab, 9)
    got = ctx.download(d_out, clean.shape)
    ctx.noise_affine(d, d, clean.size, 3, ab, 9)         # in place
    assert np.array_equal(ctx.download(d, clean.shape), got)
    ulp = np.abs(got.view(np.int32).astype(np.int64) - want.view(np.int32))
    print(f"noise_affine: {int((ulp > 0).sum())} of {ulp.size} samples differ, by {int(ulp.max())} ulp at most")
    assert ulp.max() <= 1
    # with a = 0 it is awgn's frame
    h = ctx.upload(clean)
    ctx.awgn(d, h, clean.size, 20.0, 9)
    ctx.noise_affine(d_out, h, clean.size, 3, (0.0, 400.0), 9)
    a, b = ctx.download(d, clean.shape), ctx.download(d_out, clean.shape)
    assert np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32)).max() <= 1
    for p in (d, d_out, h):
        ctx.free(p)


@pytest.mark.gpu
def test_gpu_nlk_sigma_curve(ctx, curve_tools, tmp_path, sock_dir):  # noqa: F811
    im = _input(96, 64, 3)
    wpfm(tmp_path / "noisy.pfm", im)
    ab, _ = _estimate(ctx, im)
    r = run("nlk-sigma", "--curve", tmp_path / "noisy.pfm")
    assert r.returncode == 0, r.stderr
    assert r.stdout == " ".join([str(tmp_path / "noisy.pfm")] + ["%.9g" % v for v in ab.reshape(-1)]) + "\n"
    # parameters reach the estimator
    ab8, _ = _estimate(ctx, im, nbins=8, nmin=4, step=2)
    r2 = run("nlk-sigma", "--step", 2, "--curve", "--nbins", 8, "--nmin", 4, tmp_path / "noisy.pfm")
    assert r2.returncode == 0, r2.stderr
    assert r2.stdout.split()[1:] == ["%.9g" % v for v in ab8.reshape(-1)] and r2.stdout != r.stdout
    with server(sock_dir) as env:
        served = run("nlk-sigma", "--curve", tmp_path / "noisy.pfm", env=env)
    assert served.returncode == 0, served.stderr
    assert served.stdout == r.stdout


def _decode(path):
    r = run("nlk-imgconv", path, str(path) + ".pfm")
    assert r.returncode == 0, r.stderr
    return rpfm(str(path) + ".pfm")


@pytest.fixture(scope="module")
def vst_run(curve_tools, tmp_path_factory):
    """`nlkalman-seq ... vst ...` on three noisy copies of one scene: (folder, clean, frames, coefficients, S, stdout)"""
    base = tmp_path_factory.mktemp("vst")
    (base / "in").mkdir()
    clean, frames = _seq_frames(AB)
    for t, f in enumerate(frames):
        wpfm(base / "in" / ("%03d.pfm" % (t + 1)), f)
    env = dict(os.environ, NLK_DETERMINISTIC="1")
    r = run("nlkalman-seq", base / "in" / "%03d.pfm", 1, 3, "vst", base / "vst", env=env)
    assert r.returncode == 0, r.stderr
    m = re.match(r"vst((?: \S+){6}) sigma (\S+)\n", r.stdout)
    assert m, r.stdout
    ab = np.array([float(v) for v in m.group(1).split()], np.float32).reshape(3, 2)
    return base, clean, frames, ab, m.group(2), env


@pytest.mark.gpu
def test_gpu_seq_with_sig_vst(ctx, built, vst_run):
    """`nlkalman-seq ... vst ...` prints the curve it measured and the scale, and is the run at that sigma on frames
    transformed with them, transformed back; SequenceFilter measures the same."""
    base, _, frames, ab, s, env = vst_run
    assert np.all(ab >= 0) and float(s) > 0
    assert "%.9g" % built.vst_scale(ab) == s
    measured, _ = _estimate(ctx, frames[0])
    assert _bits(measured) == _bits(ab)
    n = frames[0].size
    (base / "tin").mkdir()
    d = ctx.alloc(frames[0].nbytes)
    for t, f in enumerate(frames):
        ctx._chk(ctx.L.nlk_h2d(ctx.h, d, f.ctypes.data, f.nbytes))
        ctx.vst_forward(d, d, n, 3, ab, float(s))
        wpfm(base / "tin" / ("%03d.pfm" % (t + 1)), ctx.download(d, f.shape))
    lit = run("nlkalman-seq", base / "tin" / "%03d.pfm", 1, 3, s, base / "lit", env=env)
    assert lit.returncode == 0, lit.stderr
    for kind in ("flt1", "flt2", "smo1"):
        for i in (1, 2, 3):
            name = "%s-%03d.tif" % (kind, i)
            x = _decode(base / "lit" / name)
            ctx._chk(ctx.L.nlk_h2d(ctx.h, d, x.ctypes.data, x.nbytes))
            ctx.vst_inverse(d, d, n, 3, ab, float(s), 1)
            want = ctx.download(d, x.shape)
            got = _decode(base / "vst" / name)
            assert got.view(np.uint32).tolist() == want.view(np.uint32).tolist(), name
    ctx.free(d)
    for name in ("bflo1-002.flo", "bocc1-003.png", "fflo-001.flo", "focc-002.png"):   # the flows saw the same frames
        assert (base / "vst" / name).read_bytes() == (base / "lit" / name).read_bytes(), name
    # the coefficients given
    g = run("nlkalman-seq", base / "in" / "%03d.pfm", 1, 1, "vst:0.5,4", base / "given", "1", "", "no", env=env)
    assert g.returncode == 0, g.stderr
    assert g.stdout == "vst 0.5 4 0.5 4 0.5 4 sigma %.9g\n" % built.vst_scale(AB, 3)
    for bad in ("vst:0.5", "vst:-1,4", "vst:0,0", "vstx"):
        b = run("nlkalman-seq", base / "in" / "%03d.pfm", 1, 1, bad, base / "bad", env=env)
        assert b.returncode == 1 and b.stdout == "" and "vst" in b.stderr, bad
    # the ground-truth loop refuses
    gt = run("nlkalman-seq-gt", base / "in" / "%03d.pfm", 1, 3, "vst", base / "gt", env=env)
    assert gt.returncode == 1 and gt.stdout == "" and gt.stderr.count("\n") == 1 and "vst" in gt.stderr
    assert not (base / "gt").exists()
    # the Python driver
    seq = importlib.import_module("bwd-nlkalman_amd.sequence")
    sf = seq.SequenceFilter(ctx, 96, 64, 3, "vst", keep_history=False)
    assert sf.sigma is None and sf.noise is None
    d = ctx.upload(frames[0])
    sf.push(d)
    ctx.sync()
    assert _bits(sf.noise) == _bits(ab) and "%.9g" % sf.sigma == s
    lit_sf = seq.SequenceFilter(ctx, 96, 64, 3, float(s))
    assert sf.f1.as_dict() == lit_sf.f1.as_dict() and sf.s1.as_dict() == lit_sf.s1.as_dict()
    assert np.array_equal(ctx.download(d, frames[0].shape), frames[0])      # the pushed frame is not modified
    out = sf.download_rgb(sf.flt2)                  # applies the inverse
    t = ctx.alloc(frames[0].nbytes)
    ctx.d2d(t, sf.flt2, frames[0].nbytes)
    ctx.opp2rgb(t, 96, 64, 3)
    ctx.vst_inverse(t, t, n, 3, ab, sf.sigma, 1)
    assert np.array_equal(out, ctx.download(t, frames[0].shape))
    assert abs(out.mean() - frames[0].mean()) < 1.0   # (on the frame's scale again, not the transform's)
    ctx.free(t)
    given = seq.SequenceFilter(ctx, 96, 64, 3, ("vst", 0.5, 4))
    assert given.noise.tolist() == [[0.5, 4.0]] * 3 and given.sigma == built.vst_scale(AB, 3)
    ctx.free(d)


@pytest.mark.gpu
def test_gpu_quality_of_sig_vst(synth, vst_run):
    base, clean, _, _, _, env = vst_run
    auto = run("nlkalman-seq", base / "in" / "%03d.pfm", 1, 3, "auto", base / "auto", "1", "", "no", env=env)
    assert auto.returncode == 0, auto.stderr
    psnr = {k: np.mean([synth.psnr(_decode(base / k / ("flt2-%03d.tif" % i)), clean) for i in (1, 2, 3)])
            for k in ("vst", "auto")}
    o_auto, o_gat = _oracle_psnr(AB)
    gain = float(np.mean(o_gat) - np.mean(o_auto))
    print(f"mean flt2 PSNR: vst {psnr['vst']:.3f} dB, auto {psnr['auto']:.3f} dB; the oracle's gain {gain:.3f} dB")
    assert psnr["vst"] >= psnr["auto"] + 0.5 * gain
