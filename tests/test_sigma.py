"""The noise-level estimator (nlk_dev_estimate_sigma, Context.estimate_sigma, bin/nlk-sigma) and SIG = auto of the
sequence tools, against tests/sigma_ref.py, the float64 numpy restatement of the definition in include/nlk_hip.h.

Unless a test says otherwise its input is synth.awgn(synth.clean_frame(w, h, ch), 20.0, seed=w + h).

Bars. Block counts (N_c kept, n_c selected) are exact. sigma and sigma_c agree with the restatement within 1e-4
relative: an f32 high-frequency coefficient of size ~20 carries ~5e-5 absolute rounding from 16 products with samples
~200, that is <= 5e-6 relative on its square and less on a mean, so the bar has more than 10x margin. An exact count
needs the selection threshold to be no near-tie: the relative gap between the K-th and the (K+1)-th smallest
low-frequency energy of the restatement is asserted >= 1e-4 for every parity input (f32 rounding of that energy is
~1e-6), without a GPU. Accuracy: on 256 x 192 x 3 frames every sigma_c is within 6 % and the pooled value within 4 %
of the true sigma (the worst channel of the restatement over sigma 5 / 20 / 40 and three seeds reads 0.964)."""
import functools
import math
import os
import re
import subprocess

import numpy as np
import pytest

import sigma_ref
from test_cli import server, sock_dir, wpfm  # noqa: F401  (sock_dir: a fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "bwd-nlkalman_amd", "bin")
GPU_STEP_S = 300   # time limit of one tool run on the GPU


def run(tool, *args, **kw):
    kw.setdefault("timeout", GPU_STEP_S)
    return subprocess.run([os.path.join(BIN, tool), *map(str, args)], capture_output=True, text=True, **kw)


@pytest.fixture(scope="module")
def sigma_tools(built):
    if not all(os.path.exists(os.path.join(BIN, t)) for t in ("nlk-sigma", "nlkalman-seq", "nlk-server")):
        built.build()
    return BIN


def _synth():
    import importlib
    return importlib.import_module("bwd-nlkalman_amd.synth")


def _holed(im):
    """the NaN block and NaN first column of test_long_lists._holed"""
    h, w = im.shape[:2]
    p = im.copy()
    p[h // 3:h // 3 + 6, w // 2:w // 2 + 9] = np.nan
    p[:, :1] = np.nan
    return p


# (w, h, ch, holed, parameters), default parameters first; the comments say what a case reaches
PARITY = [
    (8, 8, 1, False, {}),            # one block
    (12, 8, 1, False, {}),           # two blocks
    (100, 9, 2, False, {}),          # K = N, two channels, one block row
    (64, 48, 1, False, {}),
    (70, 53, 3, False, {}),          # ragged: w - 8 and h - 8 are no multiples of 4
    (96, 64, 3, False, {}),
    (96, 64, 3, True, {}),           # skipped blocks
    (64, 48, 1, False, dict(step=1)),
    (70, 53, 3, False, dict(step=1)),
    (64, 48, 1, False, dict(step=8, frac=0.5, kmin=4)),   # (step 8: the blocks come straight from the image)
    (70, 53, 3, False, dict(step=8, frac=0.5, kmin=4)),
    (96, 64, 3, False, dict(frac=1.0)),                   # no selection
    (256, 192, 1, False, dict(step=1, frac=0.01)),        # 23 workgroup shares: more than the final kernel's 4 quarters
    (352, 240, 1, False, dict(step=1, frac=0.01)),        # 40 shares: more than its 32 partials in flight
]
PARITY_IDS = ["%dx%dx%d%s%s" % (w, h, ch, "-holed" if holed else "", "".join(f"-{k}{v}" for k, v in p.items()))
              for w, h, ch, holed, p in PARITY]


@functools.lru_cache(maxsize=None)
def _input(w, h, ch, holed=False):
    synth = _synth()
    im = synth.awgn(synth.clean_frame(w, h, ch), 20.0, seed=w + h)
    im = _holed(im) if holed else im
    im.setflags(write=False)
    return im


@functools.lru_cache(maxsize=None)
def _reference(case):
    w, h, ch, holed, p = PARITY[case]
    return sigma_ref.estimate(_input(w, h, ch, holed), **p)


@functools.lru_cache(maxsize=None)
def _accuracy_frame(sigma, seed):
    synth = _synth()
    return synth.awgn(synth.clean_frame(256, 192, 3), sigma, seed)


def _assert_accurate(sigma, sigma_ch, true, what):
    print(f"{what}: sigma / true = {sigma / true:.4f}, per channel {np.round(np.asarray(sigma_ch) / true, 4)}")
    assert np.all(np.abs(np.asarray(sigma_ch, np.float64) / true - 1) <= 0.06), what
    assert abs(sigma / true - 1) <= 0.04, what


# ------------------------------------------------------------ without a GPU

def test_the_estimator_is_exported(built, sigma_tools):
    L = built.hip()
    assert hasattr(L, "nlk_sigma_default_params") and hasattr(L, "nlk_dev_estimate_sigma")
    assert hasattr(built.Context, "estimate_sigma")
    assert os.path.exists(os.path.join(BIN, "nlk-sigma"))
    p = built.sigma_params()
    assert (p.step, p.frac, p.kmin, p.low_max, p.high_min) == (4, float(np.float32(0.05)), 64, 5, 8)
    assert built.sigma_params(step=8, frac=0.5).step == 8
    with pytest.raises(TypeError):
        built.sigma_params(stride=2)


def test_nlk_sigma_without_arguments(sigma_tools):
    r = run("nlk-sigma")
    assert r.returncode == 1 and r.stdout == ""
    assert r.stderr.startswith("usage: ") and "FILE" in r.stderr and r.stderr.count("\n") == 1
    r = run("nlk-sigma", "--step", "2")     # options but no file
    assert r.returncode == 1 and r.stdout == "" and r.stderr.startswith("usage: ")


def test_restatement_definition():
    """The pieces of the definition on inputs whose answer is known."""
    c = sigma_ref.dct8()
    assert np.allclose(c @ c.T, np.eye(8), atol=1e-14)
    # one block: N = n = 1, and the median of the 28 squares
    b = _input(8, 8, 1)
    y2 = (c @ b[:, :, 0].astype(np.float64) @ c.T) ** 2
    i, j = np.mgrid[0:8, 0:8]
    r = sigma_ref.estimate(b)
    assert r["counts"].tolist() == [[1, 1]] and (i + j >= 8).sum() == 28 and ((i + j >= 1) & (i + j <= 5)).sum() == 20
    assert math.isclose(r["sigma"] ** 2, np.median(y2[i + j >= 8]), rel_tol=1e-12)
    # K: 5 % of the blocks, at least 64, at most all; frac is a float32 before it is multiplied
    assert sigma_ref.estimate(_input(96, 64, 3))["counts"][0].tolist() == [23 * 15, 64]
    assert sigma_ref.estimate(_accuracy_frame(20.0, 1))["counts"][0].tolist() == [63 * 47, math.ceil(0.05 * 63 * 47)]
    assert sigma_ref.estimate(np.zeros((24, 88)), kmin=1)["counts"].tolist() == [[5 * 21, 105]]   # all tie at L = 0
    assert math.ceil(float(np.float32(0.05)) * 100) == 6 and math.ceil(0.05 * 100) == 5
    # a NaN sample removes the blocks that hold it, an all-NaN channel gives NaN and (0, 0)
    im = np.array(_input(64, 48, 1))
    im[20, 30] = np.nan
    assert sigma_ref.estimate(im)["counts"][0, 0] == 15 * 11 - 4
    r = sigma_ref.estimate(np.full((16, 16, 1), np.nan))
    assert math.isnan(r["sigma"]) and r["counts"].tolist() == [[0, 0]]


@pytest.mark.parametrize("sigma", [5.0, 20.0, 40.0])
def test_restatement_accuracy(sigma):
    for seed in (1, 2, 3):
        r = sigma_ref.estimate(_accuracy_frame(sigma, seed))
        _assert_accurate(r["sigma"], r["sigma_ch"], sigma, f"sigma {sigma} seed {seed}")


@pytest.mark.parametrize("case", range(len(PARITY)), ids=PARITY_IDS)
def test_selection_gap_of_the_parity_inputs(case):
    """(the precondition of the exact counts below: the threshold of the selection is no near-tie)"""
    gap = _reference(case)["gap"]
    print(f"{PARITY_IDS[case]}: relative gap {gap:.3e}")
    assert gap >= 1e-4


# ------------------------------------------------------------ on the GPU

def _estimate(ctx, im, **p):
    h, w, ch = im.shape
    d = ctx.upload(im)
    try:
        return ctx.estimate_sigma(d, w, h, ch, **p)
    finally:
        ctx.free(d)


def _bits(x):
    return np.asarray(x, np.float32).view(np.uint32).tolist()


@pytest.mark.gpu
@pytest.mark.parametrize("case", range(len(PARITY)), ids=PARITY_IDS)
def test_gpu_parity_with_the_restatement(ctx, case):
    w, h, ch, holed, p = PARITY[case]
    want = _reference(case)
    sigma, sigma_ch, counts = _estimate(ctx, _input(w, h, ch, holed), **p)
    got = np.array([sigma, *sigma_ch], np.float64)
    ref = np.array([want["sigma"], *want["sigma_ch"]])
    print(f"{PARITY_IDS[case]}: counts {counts.tolist()}, worst relative difference {np.abs(got / ref - 1).max():.3e}")
    assert counts.tolist() == want["counts"].tolist()
    assert np.all(np.abs(got / ref - 1) <= 1e-4), (got, ref)


@pytest.mark.gpu
def test_gpu_degenerate_inputs(ctx, built):
    sigma, sigma_ch, counts = _estimate(ctx, np.zeros((24, 32, 1), np.float32))
    assert _bits([sigma, *sigma_ch]) == [0, 0] and counts.tolist() == [[5 * 7, 5 * 7]]
    # an all-NaN channel beside a sound one
    im = np.array(np.broadcast_to(_input(64, 48, 1), (48, 64, 2)))
    im[:, :, 1] = np.nan
    sigma, sigma_ch, counts = _estimate(ctx, im)
    want = sigma_ref.estimate(im[:, :, :1])
    assert math.isnan(sigma) and math.isnan(sigma_ch[1]) and counts[1].tolist() == [0, 0]
    assert counts[0].tolist() == want["counts"][0].tolist() and abs(sigma_ch[0] / want["sigma"] - 1) <= 1e-4
    # refused sizes and parameters, and the context goes on working
    d = ctx.upload(np.zeros((20, 7, 1), np.float32))
    with pytest.raises(built.NlkError, match="rc=-3"):
        ctx.estimate_sigma(d, 7, 20, 1)
    for bad in (dict(step=0), dict(frac=0.0), dict(frac=1.5), dict(low_max=0), dict(low_max=15), dict(high_min=0),
                dict(high_min=15)):
        with pytest.raises(built.NlkError, match="rc=-3"):
            ctx.estimate_sigma(d, 10, 14, 1, **bad)
    ctx.free(d)
    sigma, _, counts = _estimate(ctx, _input(8, 8, 1))
    assert counts.tolist() == [[1, 1]] and abs(sigma / _reference(0)["sigma"] - 1) <= 1e-4


@pytest.mark.gpu
def test_gpu_same_bits_on_every_call(ctx):
    im = _input(96, 64, 3)
    a = _estimate(ctx, im)
    b = _estimate(ctx, im)
    _estimate(ctx, _accuracy_frame(20.0, 1), step=1)        # a larger frame grows the scratch in between
    c = _estimate(ctx, im)
    for other in (b, c):
        assert _bits([a[0], *a[1]]) == _bits([other[0], *other[1]]) and a[2].tolist() == other[2].tolist()


@pytest.fixture(scope="module")
def device_frame(ctx):
    """the 256 x 192 x 3, sigma 20, seed 1 frame, made on the device: (host copy, its estimate)"""
    synth = _synth()
    clean = synth.clean_frame(256, 192, 3)
    d = ctx.upload(clean)
    ctx.awgn(d, d, clean.size, 20.0, 1)
    est = ctx.estimate_sigma(d, 256, 192, 3)
    im = ctx.download(d, clean.shape)
    ctx.free(d)
    return im, est


@pytest.mark.gpu
def test_gpu_accuracy(device_frame):
    _, (sigma, sigma_ch, counts) = device_frame
    assert counts[:, 0].tolist() == [63 * 47] * 3
    _assert_accurate(sigma, sigma_ch, 20.0, "device frame, sigma 20 seed 1")


@pytest.mark.gpu
def test_gpu_nlk_sigma_tool(device_frame, sigma_tools, tmp_path, sock_dir):  # noqa: F811
    im, (sigma, sigma_ch, _) = device_frame
    wpfm(tmp_path / "noisy.pfm", im)
    r = run("nlk-sigma", tmp_path / "noisy.pfm")
    assert r.returncode == 0, r.stderr
    assert r.stdout == " ".join([str(tmp_path / "noisy.pfm")] + ["%.9g" % v for v in (sigma, *sigma_ch)]) + "\n"
    # parameters reach the estimator, several files give several lines
    r2 = run("nlk-sigma", "--step", 8, "--frac", 0.5, "--kmin", 4, tmp_path / "noisy.pfm", tmp_path / "noisy.pfm")
    assert r2.returncode == 0, r2.stderr
    lines = r2.stdout.splitlines()
    want = sigma_ref.estimate(im, step=8, frac=0.5, kmin=4)["sigma"]
    assert len(lines) == 2 and lines[0] == lines[1] and abs(float(lines[0].split()[1]) / want - 1) <= 1e-4
    r3 = run("nlk-sigma", tmp_path / "missing.pfm")
    assert r3.returncode == 1 and r3.stdout == "" and "missing.pfm" in r3.stderr
    with server(sock_dir) as env:
        served = run("nlk-sigma", tmp_path / "noisy.pfm", env=env)
    assert served.returncode == 0, served.stderr
    assert served.stdout == r.stdout


@pytest.mark.gpu
def test_gpu_seq_with_sig_auto(ctx, built, sigma_tools, synth, tmp_path):
    """`nlkalman-seq ... auto ...` prints the sigma it measured and is the run that number gives; SequenceFilter
    measures the same value."""
    import importlib
    src = tmp_path / "in"
    src.mkdir()
    frames = [synth.awgn(synth.clean_frame(96, 64, 3, t), 20.0, 100 + t) for t in range(3)]
    for t, f in enumerate(frames):
        wpfm(src / ("%03d.pfm" % (t + 1)), f)
    env = dict(os.environ, NLK_DETERMINISTIC="1")
    a = run("nlkalman-seq", src / "%03d.pfm", 1, 3, "auto", tmp_path / "auto", env=env)
    assert a.returncode == 0, a.stderr
    m = re.match(r"sigma (\S+)\n", a.stdout)
    assert m, a.stdout
    s = m.group(1)
    assert float(s) > 0
    b = run("nlkalman-seq", src / "%03d.pfm", 1, 3, s, tmp_path / "lit", env=env)
    assert b.returncode == 0, b.stderr
    assert not b.stdout.startswith("sigma")
    for kind in ("flt1", "flt2", "smo1"):
        for i in (1, 2, 3):
            name = "%s-%03d.tif" % (kind, i)
            assert (tmp_path / "auto" / name).read_bytes() == (tmp_path / "lit" / name).read_bytes(), name
    seq = importlib.import_module("bwd-nlkalman_amd.sequence")
    sf = seq.SequenceFilter(ctx, 96, 64, 3, "auto", keep_history=False)
    assert sf.sigma is None
    d = ctx.upload(frames[0])
    sf.push(d)
    ctx.sync()
    assert "%.9g" % sf.sigma == s and np.float32(sf.sigma) == np.float32(float(s))
    lit = seq.SequenceFilter(ctx, 96, 64, 3, float(s))
    assert sf.f1.as_dict() == lit.f1.as_dict() and sf.s1.as_dict() == lit.s1.as_dict()
    ctx.free(d)
