"""SIG = nlf: a noise-level function of any shape. nlk_nlf_build (host/nlf_build.c, as a stand-alone program built plain
and under AddressSanitizer and UBSan: tests/nlf_build_driver.c), the kernels nlk_dev_nlf_forward / nlk_dev_nlf_inverse,
the mode through seq_sig_parse / seq_sig_resolve into nlkalman-seq and nlkalman-y4m, bin/nlk-sigma --nlf and the Python
additions, against tests/nlf_ref.py, the numpy restatement of the definitions in include/nlk_hip.h.

The noisy frames: lin = 255 (clean / 255)^gamma of synth.clean_frame, nz = lin + sqrt(a lin + b) N with
N = default_rng(100 + t).standard_normal(shape) for frame t, z = 255 sign(nz) (|nz| / 255)^(1 / gamma) as float32
(gamma = 1: z = nz).

Bars.
* Table: every entry of nlk_nlf_build within 1e-6 relative of the restatement (both do the same double arithmetic and
  round once to float32, 6e-8; the bar leaves room for a differently associated sum), NaN where it has NaN.
* Round trip: inverse(forward(y)) within 2e-3 of y on [-64, 320], the project's pixel bar (measured: 3.1e-5 on every
  table of the test; an ulp of G near 255 is 3e-5, times islope, 0.6 .. 3 here).
* Kernels: the bits of the float32 restatement (no contraction on either side).
* CPU-oracle quality (FLT1 -> FLT2 at zero flow on three noisy copies of one scene, the curve measured on the first):
  the table of DESIGN.md §9: at 256 x 192 every flt2 PSNR within 1 dB of the table's and nlf - auto, nlf - vst each at
  least half the table's gain, per frame; at 96 x 64 on affine and white noise |nlf - vst| <= 0.2 dB per frame.
* SIG = nlf on the GPU: the mean flt2 PSNR of the nlf run is at least that of the auto run on the same files plus half
  the mean gain the oracle measured on those frames (the rule of test_noise_curve.py's test_gpu_quality_of_sig_vst)."""
import functools
import importlib
import os
import re
import subprocess

import numpy as np
import pytest

import curve_ref
import nlf_ref
import sigma_ref
import yuv_ref
from test_cli import BIN, ROOT, rpfm, wpfm
from test_seq_sig import drivers  # noqa: F401  (a fixture: tests/seq_sig_driver.c, plain and under the sanitizers)

GPU_STEP_S = 300   # time limit of one tool run on the GPU
G22 = (0.6, 4.0, 2.2)


def run(tool, *args, **kw):
    kw.setdefault("timeout", GPU_STEP_S)
    kw.setdefault("text", True)
    return subprocess.run([os.path.join(BIN, tool), *map(str, args)], capture_output=True, **kw)


def _synth():
    return importlib.import_module("bwd-nlkalman_amd.synth")


@functools.lru_cache(maxsize=None)
def gamma_frames(w, h, a, b, gamma):
    """-> (clean, the three noisy frames), read-only"""
    clean = _synth().clean_frame(w, h, 3)
    lin = 255.0 * (clean.astype(np.float64) / 255.0) ** gamma
    frames = []
    for t in range(3):
        nz = lin + np.sqrt(a * lin + b) * np.random.default_rng(100 + t).standard_normal(clean.shape)
        z = nz if gamma == 1 else 255.0 * np.sign(nz) * (np.abs(nz) / 255.0) ** (1.0 / gamma)
        frames.append(z.astype(np.float32))
    for x in (clean, *frames):
        x.setflags(write=False)
    return clean, tuple(frames)


def _f32_bins(bins):
    """the restatement's bins with m_q, v_q rounded to float32, as the device returns them"""
    b = np.array(bins, np.float64)
    b[..., 2:] = b[..., 2:].astype(np.float32)
    return b


@functools.lru_cache(maxsize=None)
def _bins(w, h, abg, **params):
    return _f32_bins(curve_ref.estimate(gamma_frames(w, h, *abg)[1][0], **dict(params))["bins"])


def _synthetic(keep, nbins=16, ch=1):
    """bins with the (q -> (n, m, v)) of `keep` kept in every channel, the others dropped (n = 0, NaN)"""
    b = np.full((ch, nbins, 4), np.nan)
    b[:, :, :2] = 0
    for q, (n, m, v) in keep.items():
        b[:, q] = (n + 40, n, m, v)
    return _f32_bins(b)


def _table_cases():
    """name -> (bins [ch][nbins][4], lo, hi, rho)"""
    cases = {
        "gamma": (_bins(256, 192, G22), 0.0, 256.0, 0.25),
        "one-kept-bin": (_synthetic({5: (40, 88.5, 30.0)}), 0.0, 256.0, 0.25),
        "missing-middle": (_synthetic({3: (50, 55.0, 9.0), 4: (70, 72.0, 16.0), 6: (64, 104.0, 30.0), 7: (33, 121.5, 2.0),
                                       9: (90, 150.0, 0.01)}), 0.0, 256.0, 0.25),
        "nbins1": (_bins(96, 64, G22, nbins=1), 0.0, 256.0, 0.25),
        "nbins64": (_bins(96, 64, G22, nbins=64, nmin=1), 0.0, 256.0, 0.5),
        "lo16": (_bins(256, 192, G22, lo=16.0, hi=240.0), 16.0, 240.0, 1.0),
    }
    # bins that are not kept although they have blocks: v = 0, NaN, inf, negative
    odd = _synthetic({2: (40, 40.0, 25.0), 3: (40, 56.0, 0.0), 4: (40, 72.0, np.nan), 5: (40, 88.0, np.inf),
                      6: (40, 104.0, -1.0), 7: (40, 120.0, 36.0)})
    cases["unusable-variances"] = (odd, 0.0, 256.0, 0.25)
    empty = np.concatenate([_synthetic({5: (40, 88.5, 30.0), 8: (50, 130.0, 20.0)}), _synthetic({})])
    cases["empty-channel"] = (empty, 0.0, 256.0, 0.25)
    return cases


REFUSED = [(0, 16, 0, 256, 0.25), (17, 16, 0, 256, 0.25), (1, 0, 0, 256, 0.25), (1, 65, 0, 256, 0.25),
           (1, 16, 10, 10, 0.25), (1, 16, 20, 10, 0.25), (1, 16, 0, "inf", 0.25), (1, 16, "nan", 256, 0.25),
           (1, 16, 0, 256, 0), (1, 16, 0, 256, -0.25), (1, 16, 0, 256, 1.5), (1, 16, 0, 256, "nan")]
FIELDS = ("x", "G", "slope", "islope", "sigma")


def _close(got, want, rel=1e-6):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    nan = np.isnan(want)
    return bool(got.shape == want.shape and np.array_equal(np.isnan(got), nan)
                and np.all(np.abs(got - want)[~nan] <= rel * np.abs(want)[~nan]))


def _assert_table(got, want, what):
    assert (got["kept"].tolist(), got["nbins"], got["ch"]) == (want["kept"].tolist(), want["nbins"], want["ch"]), what
    assert _close([got["s"], got["inv_dx"]], [want["s"], want["inv_dx"]]), (what, got["s"], want["s"])
    for k in FIELDS:
        assert _close(got[k], want[k]), (what, k, got[k], want[k])


# ------------------------------------------------------------ without a GPU

@pytest.fixture(scope="module")
def build_drivers(tmp_path_factory):
    """tests/nlf_build_driver.c with host/nlf_build.c and nothing else, plain and under the sanitizers (their runtimes
    linked statically where the compiler has them: the program runs as it is, nothing is preloaded)"""
    d = tmp_path_factory.mktemp("nlf_build")
    src = [os.path.join(ROOT, "tests", "nlf_build_driver.c"), os.path.join(ROOT, "bwd-nlkalman_amd", "host", "nlf_build.c")]
    base = ["gcc", "-O1", "-g", "-std=gnu99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), *src, "-lm", "-o"]
    plain, san = str(d / "plain"), str(d / "san")
    subprocess.check_call(base + [plain])
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    for static in (["-static-libasan", "-static-libubsan"], []):
        if subprocess.run(base + [san, *flags, *static], capture_output=True).returncode == 0 and \
                subprocess.run([san], capture_output=True).returncode == 1:     # (no file named: its own status)
            return [plain, san]
    return [plain]


def _case_text(bins, lo, hi, rho, ch=None, nbins=None):
    bins = np.asarray(bins, np.float64).reshape(-1, 4)
    head = "%s %s %s %s %s %d\n" % (ch, nbins, lo, hi, rho, len(bins))
    return head + "".join("%d %d %.9g %.9g\n" % (b[0], b[1], b[2], b[3]) for b in bins)


def _parse_tables(text, shapes):
    """the driver's output -> per case None (refused) or the table as nlf_ref.build's dict"""
    lines, out = text.splitlines(), []
    for ch, nbins in shapes:
        rc = int(lines.pop(0).split()[1])
        if rc != 0:
            assert rc == -3, rc
            out.append(None)
            continue
        f = lines.pop(0).split()
        t = dict(ch=ch, nbins=nbins, s=float(f[1]), inv_dx=float(f[3]),
                 kept=np.array(lines.pop(0).split()[1:], np.int32), x=np.array(lines.pop(0).split()[1:], np.float32))
        rows = {k: [] for k in FIELDS[1:]}
        for c in range(ch):
            for k in ("G", "slope", "islope", "sigma"):
                f = lines.pop(0).split()
                assert f[:2] == [k, str(c)]
                rows[k].append(np.array(f[2:], np.float32))
        t.update({k: np.array(v, np.float32).reshape(ch, -1) for k, v in rows.items()})
        out.append(t)
    assert not lines
    return out


def test_grammar(drivers):  # noqa: F811
    """`nlf` is mode 4 and must be the whole word; everything else reads as before"""
    texts = ["nlf", "nlfx", "nl", "NLF", "nlf:1,2", "auto", "vst", "vst:0.5,2", "20"]
    want = [(4, 0, 0), (0, 0, 0), (0, 0, 0), (0, 0, 0), (0, 0, 0), (1, 0, 0), (2, 0, 0), (3, 0, 0), (0, 20, 0)]
    for exe in drivers:
        r = subprocess.run([exe, *texts], capture_output=True, text=True, timeout=60)
        assert r.returncode == 0 and r.stderr == "", (exe, r)
        got = [(int(f[1]), float(f[7]), int(f[9])) for f in (line.split() for line in r.stdout.splitlines())]
        assert got == want, (exe, r.stdout)


def test_table_equals_the_restatement(build_drivers, tmp_path):
    cases = _table_cases()
    text = "".join(_case_text(b, lo, hi, rho, *b.shape[:2]) for b, lo, hi, rho in cases.values())
    one = _synthetic({5: (40, 88.5, 30.0)})
    text += "".join(_case_text(one if (ch, nb) == (1, 16) else [], lo, hi, rho, ch, nb) for ch, nb, lo, hi, rho in REFUSED)
    text += _case_text(one, 0, 256, 1, 1, 16)          # rho = 1 is accepted
    (tmp_path / "cases.txt").write_text(text)
    shapes = [b.shape[:2] for b, *_ in cases.values()] + [(ch, nb) for ch, nb, *_ in REFUSED] + [(1, 16)]
    for exe in build_drivers:
        r = subprocess.run([exe, str(tmp_path / "cases.txt")], capture_output=True, text=True, timeout=60)
        assert r.returncode == 0 and r.stderr == "", (exe, r.returncode, r.stderr)
        tables = _parse_tables(r.stdout, shapes)
        for (name, (b, lo, hi, rho)), got in zip(cases.items(), tables):
            want = nlf_ref.build(b, lo, hi, rho)
            print(f"{os.path.basename(exe)} {name}: kept {want['kept'].tolist()} s {got['s']:.9g} (restatement {want['s']:.9g})")
            _assert_table(got, want, name)
        assert all(t is None for t in tables[len(cases):-1]), "every refused argument returns NLK_EINVAL"
        _assert_table(tables[-1], nlf_ref.build(one, 0, 256, 1.0), "rho = 1")
    # what the cases are meant to reach
    t = nlf_ref.build(*cases["empty-channel"])
    assert np.isnan(t["s"]) and t["kept"].tolist() == [2, 0] and np.isnan(t["G"]).all()
    assert nlf_ref.build(*cases["unusable-variances"])["kept"].tolist() == [2]
    assert nlf_ref.build(*cases["one-kept-bin"])["kept"].tolist() == [1]
    assert nlf_ref.build(*cases["gamma"])["kept"].min() >= 8


def test_restatement_definition():
    """The pieces of the rule on inputs whose answer is known."""
    # one kept bin: a constant noise level, so the map is y * 255 / 255 scaled: g(y) = y exactly, s = sigma
    t = nlf_ref.build(_synthetic({5: (40, 88.5, 36.0)}))
    assert np.allclose(t["sigma"], 6.0) and abs(t["s"] - 6.0) < 1e-6 and np.allclose(t["G"][0], t["x"], rtol=1e-6)
    assert np.allclose(t["slope"], 1.0) and np.allclose(t["islope"], 1.0)
    # smoothing over neighbours in K, not in q: bins 2 and 9 are neighbours; the end bins miss one neighbour
    b = _synthetic({2: (10, 40.0, 4.0), 9: (30, 150.0, 16.0)})
    t = nlf_ref.build(b, rho=1e-3)
    v_lo, v_hi = (2 * 10 * 4 + 30 * 16) / 50.0, (2 * 30 * 16 + 10 * 4) / 70.0
    assert np.isclose(t["sigma"][0, 0] ** 2, v_lo, rtol=1e-6) and np.isclose(t["sigma"][0, -1] ** 2, v_hi, rtol=1e-6)
    # linear interpolation between the means: the knot at 96 lies (96 - 40) / 110 of the way
    assert np.isclose(t["sigma"][0, 6] ** 2, v_lo + (96.0 - 40.0) / 110.0 * (v_hi - v_lo), rtol=1e-6)
    # the floor: where the variance collapses (a clipped end) it is raised to rho^2 times the median. Equal counts,
    # v = 16 16 16 16 e e with e = 1e-6: vs = 16 16 16 12 4 e (+ O(e)), an even count: the median is (12 + 16) / 2
    b = _synthetic({q: (10, 16.0 * q + 8, 16.0 if q < 6 else 1e-6) for q in range(2, 8)})
    for rho in (0.25, 0.5):
        t = nlf_ref.build(b, rho=rho)
        assert np.isclose(t["sigma"][0, -1] ** 2, rho * rho * 14.0, rtol=1e-6)      # the last bin: at the floor
        assert np.isclose(t["sigma"][0, 0] ** 2, 16.0, rtol=1e-6)                   # the first: untouched
    # the scale: the transform of 0..255 spans 255 on average over the channels, black stays 0
    t = nlf_ref.build(_bins(256, 192, G22))
    span = nlf_ref.forward(np.full(3, 255, np.float32), t) - nlf_ref.forward(np.zeros(3, np.float32), t)
    assert abs(span.mean() - 255.0) < 1e-3 and np.all(nlf_ref.forward(np.zeros(3, np.float32), t) == 0)
    # the noise of a transformed flat field has deviation s where the curve was measured
    clean, frames = gamma_frames(256, 192, *G22)
    g = nlf_ref.forward(frames[0], t)
    flat = np.abs(clean[:, :, 0] - 150.0) < 2.0
    dev = (g[:, :, 0] - nlf_ref.forward(clean, t)[:, :, 0])[flat].std()
    print(f"deviation of the transformed frame near 150 over s: {dev / t['s']:.3f} ({int(flat.sum())} samples)")
    assert flat.sum() > 500 and abs(dev / t["s"] - 1) < 0.1


@pytest.mark.parametrize("name", ["gamma", "nbins1", "nbins64", "lo16", "one-kept-bin", "missing-middle"])
def test_restatement_properties(name):
    b, lo, hi, rho = _table_cases()[name]
    t = nlf_ref.build(b, lo, hi, rho)
    assert np.all(np.diff(t["G"].astype(np.float64), axis=1) > 0), "G is strictly increasing"
    zero = nlf_ref.forward(np.zeros(t["ch"], np.float32), t)
    # lo = 0: x[0] = G[0] = 0 and forward(0) is 0 exactly; else G[0] + (0 - x[0]) slope[0], three roundings of
    # numbers of |G[0]|'s size (an ulp of 64 is 8e-6)
    assert np.all(zero == 0) if lo == 0 else np.abs(zero).max() <= 1e-4, zero
    grid = np.repeat(np.arange(-64.0, 320.0 + 1 / 32, 1 / 16, dtype=np.float32), t["ch"])
    rng = np.random.default_rng(3)
    grid = np.concatenate([grid, rng.uniform(-64, 320, 3000 * t["ch"]).astype(np.float32)])
    back = nlf_ref.inverse(nlf_ref.forward(grid, t), t)
    print(f"{name}: round trip max-abs {np.abs(back - grid).max():.3e}; islope {t['islope'].min():.3g} .. {t['islope'].max():.3g}")
    assert np.abs(back - grid).max() <= 2e-3
    # NaN gives NaN, +-inf passes through, on both sides
    odd = np.array([np.nan, np.inf, -np.inf] * t["ch"], np.float32)
    for f in (nlf_ref.forward, nlf_ref.inverse):
        assert np.array_equal(f(odd, t), odd, equal_nan=True)


# ---- the oracle's filter on transformed frames: three noisy copies of one scene, FLT1 -> FLT2 at zero flow

# flt2 PSNR of frames 0 / 1 / 2: auto | vst | nlf
TABLE = {(256, 192, 0.6, 4.0, 2.2): ((37.00, 37.24, 36.97), (37.56, 37.89, 37.66), (39.16, 39.74, 39.53)),
         (256, 192, 0.3, 30.0, 2.2): ((28.36, 28.37, 28.23), (31.56, 31.59, 31.29), (36.47, 37.15, 37.00)),
         (96, 64, 0.5, 4.0, 1): ((39.34, 39.70, 39.47), (40.69, 41.63, 41.96), (40.70, 41.62, 41.89)),
         (96, 64, 0.0, 400.0, 1): ((34.49, 35.34, 35.56), (34.37, 35.20, 35.37), (34.39, 35.22, 35.40))}


@functools.lru_cache(maxsize=None)
def _oracle_psnr(case, modes=("auto", "vst", "nlf")):
    """-> {mode: flt2 PSNR per frame}, the method of test_noise_curve.py's _oracle_psnr: everything a mode needs is
    measured on frame 0"""
    import oracle as O
    O.build()
    synth = _synth()
    w, h, a, b, gamma = case
    clean, frames = gamma_frames(w, h, a, b, gamma)

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
    res = {}
    curve = curve_ref.estimate(frames[0])
    if "auto" in modes:
        res["auto"] = recursion(frames, sigma_ref.estimate(frames[0])["sigma"], lambda x: x)
    if "vst" in modes:
        est = curve["ab"].astype(np.float32).astype(np.float64)
        s = curve_ref.vst_scale(est)
        res["vst"] = recursion([curve_ref.vst_forward(f, est, s).astype(np.float32) for f in frames], s,
                               lambda x: curve_ref.vst_inverse(x, est, s, 1))
    if "nlf" in modes:
        t = nlf_ref.build(_f32_bins(curve["bins"]))
        res["nlf"] = recursion([nlf_ref.forward(f, t) for f in frames], t["s"],
                               lambda x: nlf_ref.inverse(np.ascontiguousarray(x, np.float32), t))
    return res


@pytest.mark.parametrize("case", [k for k in TABLE if k[0] == 256], ids=lambda k: "a%g-b%g-g%g" % k[2:])
def test_oracle_filters_gamma_frames_better(case):
    got = _oracle_psnr(case)
    t_auto, t_vst, t_nlf = TABLE[case]
    for k, v in got.items():
        print(f"{case}: flt2 PSNR {k} {np.round(v, 2)}")
    for k in range(3):
        for mode, want in zip(("auto", "vst", "nlf"), (t_auto, t_vst, t_nlf)):
            assert abs(got[mode][k] - want[k]) <= 1.0, (mode, k)
        assert got["nlf"][k] - got["auto"][k] >= 0.5 * (t_nlf[k] - t_auto[k]), k
        assert got["nlf"][k] - got["vst"][k] >= 0.5 * (t_nlf[k] - t_vst[k]), k


@pytest.mark.parametrize("case", [k for k in TABLE if k[0] == 96], ids=lambda k: "a%g-b%g-g%g" % k[2:])
def test_oracle_nlf_equals_vst_on_affine_and_white_noise(case):
    got = _oracle_psnr(case, modes=("vst", "nlf"))
    diff = np.abs(np.array(got["nlf"]) - np.array(got["vst"]))
    print(f"{case}: flt2 PSNR vst {np.round(got['vst'], 2)}, nlf {np.round(got['nlf'], 2)}, |nlf - vst| {np.round(diff, 3)}")
    assert diff.max() <= 0.2


def test_the_feature_is_exported(built):
    L = built.hip()
    for name in ("nlk_nlf_build", "nlk_dev_nlf_forward", "nlk_dev_nlf_inverse"):
        assert hasattr(L, name) and name in built.HIP_SYMBOLS, name
    for name in ("nlf_table", "nlf_forward", "nlf_inverse"):
        assert hasattr(built.Context, name), name
    # the library's nlk_nlf_build through the Python mirror of the struct
    for name, (b, lo, hi, rho) in _table_cases().items():
        rec = np.zeros(b.shape[:2], built.CURVE_BIN)
        rec["nblocks"], rec["nsel"], rec["mean"], rec["var"] = (b[:, :, k] for k in range(4))
        t = built.nlf_build(rec, lo, hi, rho)
        got = dict(t.arrays(), ch=t.ch, nbins=t.nbins, s=t.s, inv_dx=t.inv_dx)
        _assert_table(got, nlf_ref.build(b, lo, hi, rho), name)
    with pytest.raises(ValueError):
        built.nlf_build(np.zeros((1, 16), built.CURVE_BIN), 10.0, 10.0)
    with pytest.raises(ValueError):
        built.nlf_build(np.zeros((17, 16), built.CURVE_BIN))
    r = run("nlk-sigma")
    assert r.returncode == 1 and r.stdout == "" and r.stderr.startswith("usage: ") and "--nlf" in r.stderr
    r = run("nlk-sigma", "--curve", "--nlf", "x.pfm")     # one report or the other
    assert r.returncode == 1 and r.stdout == "" and r.stderr.startswith("usage: ")


# ------------------------------------------------------------ on the GPU

def _c_table(built, t):
    """the NlfTable holding the restatement's float32 arrays"""
    c = built.NlfTable()
    c.ch, c.nbins, c.lo, c.hi, c.inv_dx, c.s = t["ch"], t["nbins"], t["lo"], t["hi"], float(t["inv_dx"]), t["s"]
    for k in ("G", "slope", "islope", "sigma"):
        a = np.ctypeslib.as_array(getattr(c, k))
        a[:t["ch"], :t[k].shape[1]] = t[k]
    np.ctypeslib.as_array(c.x)[:t["nbins"] + 1] = t["x"]
    np.ctypeslib.as_array(c.kept)[:t["ch"]] = t["kept"]
    return c


@functools.lru_cache(maxsize=None)
def _kernel_table(ch, nbins):
    """a table of `ch` channels (the gamma frame's three, repeated with other gains) and nbins bins"""
    params = dict(nbins=nbins, nmin=1) if nbins == 64 else dict(nbins=nbins)
    b3 = _bins(256, 192, G22, **params)
    b = np.concatenate([b3] * 6)[:ch].copy()
    for c in range(ch):
        b[c, :, 3] *= 1.0 + 0.37 * (c // 3)          # other channels, other levels
    return nlf_ref.build(b)


def _samples(n, t, seed):
    """n samples over the table's range and beyond, with knots, NaN and +-inf among them where there is room"""
    rng = np.random.default_rng(seed)
    y = rng.uniform(-80.0, 340.0, n).astype(np.float32)
    special = np.concatenate([t["x"], [np.nan, np.inf, -np.inf, -1e30, 1e30, t["lo"], t["hi"], 0.0, 255.0]]).astype(np.float32)
    if n >= 255:
        at = rng.permutation(n)[:3 * len(special)]
        y[at] = np.tile(special, 3)                   # (each in more than one channel)
    return y


def _bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


def _same(got, want):
    """the same bits, a NaN where the restatement has a NaN (whatever its payload)"""
    nan = np.isnan(want)
    return bool(np.array_equal(np.isnan(got), nan) and np.array_equal(_bits(got)[~nan], _bits(want)[~nan]))


KERNEL_CASES = [(n, ch, nbins) for ch, nbins in ((1, 1), (3, 16), (4, 64), (16, 16), (16, 64), (3, 1))
                for n in (1, 255, 256, 257, 3000)]


@pytest.mark.gpu
def test_gpu_kernels_give_the_bits_of_the_restatement(ctx, built):
    """n = 1, 255, 256, 257, 3 x 1000; ch = 1, 3, 4, 16; nbins = 1, 16, 64; samples below lo, above hi, on knots, NaN,
    +-inf; in place; the same bits on a second call; tables alternate, so every call but the first of a pair uploads or
    reuses the context's copy"""
    d_in, d_out = ctx.alloc(4 * 3000), ctx.alloc(4 * 3000)
    for n, ch, nbins in KERNEL_CASES:
        t = _kernel_table(ch, nbins)
        ct = _c_table(built, t)
        y = _samples(n, t, seed=n + ch + nbins)
        want_f = nlf_ref.forward(y, t)
        g = want_f.copy()
        fin = np.isfinite(g)
        g[fin] += np.random.default_rng(n).normal(0, 2, int(fin.sum())).astype(np.float32)   # (off the forward's image)
        if n >= 255:
            k = np.arange(t["nbins"] + 1)
            g[k] = t["G"][k % ch, k]                  # sample k sits on knot k of its own channel
        want_i = nlf_ref.inverse(g, t)
        for src, want, call in ((y, want_f, ctx.nlf_forward), (g, want_i, ctx.nlf_inverse)):
            ctx._chk(ctx.L.nlk_h2d(ctx.h, d_in, src.ctypes.data, src.nbytes))
            call(d_out, d_in, n, ch, ct)
            got = ctx.download(d_out, (n,))
            assert _same(got, want), (n, ch, nbins, call.__name__)
            call(d_out, d_in, n, ch, ct)              # again: the context's copy of the table is reused
            assert np.array_equal(_bits(ctx.download(d_out, (n,))), _bits(got))
            call(d_in, d_in, n, ch, ct)               # in place
            assert np.array_equal(_bits(ctx.download(d_in, (n,))), _bits(got))
        assert np.array_equal(np.isnan(want_f), np.isnan(y)) and np.array_equal(want_f[np.isinf(y)], y[np.isinf(y)])
    for p in (d_in, d_out):
        ctx.free(p)


@pytest.mark.gpu
def test_gpu_a_second_table_and_refused_arguments(ctx, built):
    t1, t2 = _kernel_table(3, 16), _kernel_table(3, 64)
    c1, c2 = _c_table(built, t1), _c_table(built, t2)
    y = _samples(3000, t1, seed=11)
    d = ctx.upload(y)
    d_out = ctx.alloc(y.nbytes)
    for t, c in ((t1, c1), (t2, c2), (t1, c1), (t1, c1), (t2, c2)):     # new, new, back, same, new
        ctx.nlf_forward(d_out, d, 3000, 3, c)
        assert _same(ctx.download(d_out, (3000,)), nlf_ref.forward(y, t))
    # a table edited in place is another table
    c1.G[1][3] = c1.G[1][3] + 0.5
    t1e = dict(t1, G=t1["G"].copy())
    t1e["G"][1, 3] += np.float32(0.5)
    ctx.nlf_forward(d_out, d, 3000, 3, c1)
    assert _same(ctx.download(d_out, (3000,)), nlf_ref.forward(y, t1e))
    # refused: the channel count of another table, an invalid table, sizes outside the limits, NULL
    bad = []
    for ch, edit in ((4, {}), (3, dict(s=float("nan"))), (3, dict(s=0.0)), (3, dict(s=float("inf"))), (3, dict(nbins=0)),
                     (3, dict(nbins=65)), (17, dict(ch=17)), (0, dict(ch=0))):
        c = _c_table(built, t2)
        for k, v in edit.items():
            setattr(c, k, v)
        bad.append((ch, c))
    for ch, c in bad:
        for call in (ctx.nlf_forward, ctx.nlf_inverse):
            with pytest.raises(built.NlkError, match="rc=-3"):
                call(d_out, d, 3000, ch, c)
    with pytest.raises(built.NlkError, match="rc=-3"):
        ctx._chk(ctx.L.nlk_dev_nlf_forward(ctx.h, d_out, d, 3000, 3, None))
    with pytest.raises(built.NlkError, match="rc=-3"):
        ctx._chk(ctx.L.nlk_dev_nlf_inverse(ctx.h, None, d, 3000, 3, c2))
    ctx.nlf_forward(d_out, d, 0, 3, c2)               # nothing to do
    ctx.nlf_inverse(d_out, d, 3000, 3, c2)            # the context still works
    assert _same(ctx.download(d_out, (3000,)), nlf_ref.inverse(y, t2))
    for p in (d, d_out):
        ctx.free(p)


@pytest.mark.gpu
def test_gpu_table_of_a_device_frame(ctx, built):
    """Context.nlf_table: the device's bins through nlk_nlf_build, within the estimator's tolerance of the restatement
    (test_noise_curve.py: counts exact, m_q and v_q 1e-4 relative)"""
    _, frames = gamma_frames(256, 192, *G22)
    d = ctx.upload(frames[0])
    t = ctx.nlf_table(d, 256, 192, 3)
    ab, bins = ctx.estimate_noise_curve(d, 256, 192, 3)
    ctx.free(d)
    again = built.nlf_build(bins)
    assert bytes(t) == bytes(again)
    want = nlf_ref.build(_bins(256, 192, G22))
    got = t.arrays()
    assert got["kept"].tolist() == want["kept"].tolist() and abs(t.s / want["s"] - 1) <= 1e-4
    for k in FIELDS:
        assert _close(got[k], want[k], rel=1e-4), k


def _decode(path):
    r = run("nlk-imgconv", path, str(path) + ".pfm")
    assert r.returncode == 0, r.stderr
    return rpfm(str(path) + ".pfm")


@pytest.fixture(scope="module")
def nlf_run(built, tmp_path_factory):
    """`nlkalman-seq ... nlf ...` on the three 256 x 192 gamma frames: (folder, clean, frames, kept counts, S, env)"""
    if not all(os.path.exists(os.path.join(BIN, t)) for t in ("nlk-sigma", "nlkalman-seq", "nlkalman-y4m", "nlk-imgconv")):
        built.build()
    base = tmp_path_factory.mktemp("nlf")
    (base / "in").mkdir()
    clean, frames = gamma_frames(256, 192, *G22)
    for t, f in enumerate(frames):
        wpfm(base / "in" / ("%03d.pfm" % (t + 1)), f)
    env = dict(os.environ, NLK_DETERMINISTIC="1")
    r = run("nlkalman-seq", base / "in" / "%03d.pfm", 1, 3, "nlf", base / "nlf", env=env)
    assert r.returncode == 0, r.stderr
    m = re.fullmatch(r"nlf kept (\d+) (\d+) (\d+) sigma (\S+)\n", r.stdout)
    assert m, r.stdout
    return base, clean, frames, [int(m.group(k)) for k in (1, 2, 3)], m.group(4), env


@pytest.mark.gpu
def test_gpu_seq_with_sig_nlf(ctx, built, nlf_run):
    """`nlkalman-seq ... nlf ...` prints the bins it kept and the scale, and is the run at that sigma on frames
    transformed with the first frame's table, transformed back: the composition of the C-ABI calls, exactly."""
    base, _, frames, kept, s, env = nlf_run
    n = frames[0].size
    d = ctx.upload(frames[0])
    table = ctx.nlf_table(d, 256, 192, 3)
    assert kept == list(table.kept)[:3] and "%.9g" % table.s == s and min(kept) >= 8
    (base / "tin").mkdir()
    for t, f in enumerate(frames):
        ctx._chk(ctx.L.nlk_h2d(ctx.h, d, f.ctypes.data, f.nbytes))
        ctx.nlf_forward(d, d, n, 3, table)
        wpfm(base / "tin" / ("%03d.pfm" % (t + 1)), ctx.download(d, f.shape))
    lit = run("nlkalman-seq", base / "tin" / "%03d.pfm", 1, 3, s, base / "lit", env=env)
    assert lit.returncode == 0, lit.stderr
    for kind in ("flt1", "flt2", "smo1"):
        for i in (1, 2, 3):
            name = "%s-%03d.tif" % (kind, i)
            x = _decode(base / "lit" / name)
            ctx._chk(ctx.L.nlk_h2d(ctx.h, d, x.ctypes.data, x.nbytes))
            ctx.nlf_inverse(d, d, n, 3, table)
            want = ctx.download(d, x.shape)
            got = _decode(base / "nlf" / name)
            assert np.array_equal(_bits(got), _bits(want)), name
    for name in ("bflo1-002.flo", "bocc1-003.png", "fflo-001.flo", "focc-002.png"):   # the flows saw the same frames
        assert (base / "nlf" / name).read_bytes() == (base / "lit" / name).read_bytes(), name
    # the Python driver measures the same and leaves through the inverse
    seq = importlib.import_module("bwd-nlkalman_amd.sequence")
    sf = seq.SequenceFilter(ctx, 256, 192, 3, "nlf", keep_history=False)
    assert sf.sigma is None and sf.nlf is None
    ctx._chk(ctx.L.nlk_h2d(ctx.h, d, frames[0].ctypes.data, frames[0].nbytes))
    sf.push(d)
    ctx.sync()
    assert bytes(sf.nlf) == bytes(table) and "%.9g" % sf.sigma == s
    assert sf.f1.as_dict() == seq.SequenceFilter(ctx, 256, 192, 3, float(s)).f1.as_dict()
    assert np.array_equal(ctx.download(d, frames[0].shape), frames[0])      # the pushed frame is not modified
    out = sf.download_rgb(sf.flt2)
    t = ctx.alloc(frames[0].nbytes)
    ctx.d2d(t, sf.flt2, frames[0].nbytes)
    ctx.opp2rgb(t, 256, 192, 3)
    ctx.nlf_inverse(t, t, n, 3, table)
    assert np.array_equal(out, ctx.download(t, frames[0].shape))
    assert abs(out.mean() - frames[0].mean()) < 1.0   # (on the frame's scale again, not the transform's)
    for p in (t, d):
        ctx.free(p)


@pytest.mark.gpu
def test_gpu_y4m_with_sig_nlf(ctx, nlf_run, tmp_path):
    """nlkalman-y4m nlf at 4:4:4: the codes of nlkalman-seq's flt2 files on the frames the stream holds, and the same
    report line on stderr"""
    _, _, frames, _, _, env = nlf_run
    f = yuv_ref.fmt("444", 0, 601)
    pay = [yuv_ref.to_yuv(a, f).tobytes() for a in frames]
    rgbs = [yuv_ref.to_rgb(p, 256, 192, f) for p in pay]
    (tmp_path / "in").mkdir()
    for t, a in enumerate(rgbs):
        wpfm(tmp_path / "in" / ("%03d.pfm" % (t + 1)), a)
    r = run("nlkalman-seq", tmp_path / "in" / "%03d.pfm", 1, 3, "nlf", tmp_path / "seq", 1, "", "no", env=env)
    assert r.returncode == 0 and r.stdout.startswith("nlf kept "), (r.stdout, r.stderr)
    want = [yuv_ref.to_yuv(_decode(tmp_path / "seq" / ("flt2-%03d.tif" % (t + 1))), f).tobytes() for t in range(3)]
    y = run("nlkalman-y4m", "nlf", input=yuv_ref.y4m_bytes(256, 192, "444", pay), env=env, text=False)
    assert y.returncode == 0, y.stderr
    assert [l for l in y.stderr.decode().splitlines(True) if l.startswith("nlf ")] == [r.stdout]
    got = yuv_ref.y4m_parse(y.stdout)[4]
    assert got == want and got[0] != pay[0]


@pytest.mark.gpu
def test_gpu_quality_of_sig_nlf(synth, nlf_run):
    base, clean, _, _, _, env = nlf_run
    auto = run("nlkalman-seq", base / "in" / "%03d.pfm", 1, 3, "auto", base / "auto", "1", "", "no", env=env)
    assert auto.returncode == 0, auto.stderr
    psnr = {k: np.mean([synth.psnr(_decode(base / k / ("flt2-%03d.tif" % i)), clean) for i in (1, 2, 3)])
            for k in ("nlf", "auto")}
    o = _oracle_psnr((256, 192, *G22))
    gain = float(np.mean(o["nlf"]) - np.mean(o["auto"]))
    print(f"mean flt2 PSNR: nlf {psnr['nlf']:.3f} dB, auto {psnr['auto']:.3f} dB; the oracle's gain {gain:.3f} dB")
    assert psnr["nlf"] >= psnr["auto"] + 0.5 * gain


@pytest.mark.gpu
def test_gpu_tools_refuse_a_frame_without_bins(ctx, built, nlf_run, tmp_path):
    """a frame too small for any bin to reach nmin: a message under the tool's name, status 1, nothing filtered"""
    _, frames = gamma_frames(96, 64, *G22)
    wpfm(tmp_path / "001.pfm", np.ascontiguousarray(frames[0][:24, :24]))
    r = run("nlkalman-seq", tmp_path / "%03d.pfm", 1, 1, "nlf", tmp_path / "out", 1, "", "no")
    assert r.returncode == 1 and r.stdout == "" and r.stderr.startswith("nlkalman-seq: SIG = nlf: ") and r.stderr.count("\n") == 1
    assert not (tmp_path / "out" / "flt2-001.tif").exists()
    seq = importlib.import_module("bwd-nlkalman_amd.sequence")
    d = ctx.upload(np.ascontiguousarray(frames[0][:24, :24]))
    with pytest.raises(ValueError):
        seq.SequenceFilter(ctx, 24, 24, 3, "nlf").push(d)
    ctx.free(d)


@pytest.mark.gpu
def test_gpu_lsmo_and_gt_tools_take_nlf(ctx, built, nlf_run, synth, tmp_path):
    """the lag-1 smoother tool and the ground-truth loop read SIG through the same two functions"""
    clean, frames = gamma_frames(96, 64, *G22)
    env = nlf_run[5]
    (tmp_path / "in").mkdir()
    (tmp_path / "clean").mkdir()
    (tmp_path / "gt").mkdir()
    for t, f in enumerate(frames):
        wpfm(tmp_path / "in" / ("%03d.pfm" % (t + 1)), f)
        wpfm(tmp_path / "clean" / ("%03d.pfm" % (t + 1)), clean)
    seq = run("nlkalman-seq", tmp_path / "in" / "%03d.pfm", 1, 3, "nlf", tmp_path / "seq", 1, "", "no", env=env)
    lsmo = run("nlkalman-lsmo-seq", tmp_path / "in" / "%03d.pfm", 1, 3, "nlf", tmp_path / "lsmo", env=env)
    assert seq.returncode == 0 and lsmo.returncode == 0, (seq.stderr, lsmo.stderr)
    assert lsmo.stdout == seq.stdout and seq.stdout.startswith("nlf kept ")
    for i in (1, 2, 3):
        name = "flt2-%03d.tif" % i
        assert (tmp_path / "lsmo" / name).read_bytes() == (tmp_path / "seq" / name).read_bytes(), name
        lsm1 = _decode(tmp_path / "lsmo" / ("lsm1-%03d.tif" % i))
        assert abs(lsm1.mean() - frames[0].mean()) < 1.0           # (through the inverse: on the frame's scale)
    # the ground-truth loop: as with auto there is no sigma to make noise with, the noisy frames must be there
    gt = run("nlkalman-seq-gt", tmp_path / "clean" / "%03d.pfm", 1, 3, "nlf", tmp_path / "gt", "", "no", env=env)
    assert gt.returncode == 1 and gt.stdout == "" and gt.stderr.count("\n") == 1, gt
    assert gt.stderr.startswith("nlkalman-seq-gt: SIG = nlf needs the noisy frame "), gt.stderr
    for t in range(3):
        r = run("nlk-imgconv", tmp_path / "in" / ("%03d.pfm" % (t + 1)), tmp_path / "gt" / ("%03d.tif" % (t + 1)))
        assert r.returncode == 0, r.stderr
    gt = run("nlkalman-seq-gt", tmp_path / "clean" / "%03d.pfm", 1, 3, "nlf", tmp_path / "gt", "", "no", env=env)
    assert gt.returncode == 0, gt.stderr
    lines = gt.stdout.splitlines(True)
    assert lines[0] == seq.stdout and len(lines) == 2
    mse_f1, mse_f2 = (float(v) for v in lines[1].split()[:2])
    noisy_mse = float(np.mean([(f.astype(np.float64) - clean) ** 2 for f in frames]))
    print(f"nlkalman-seq-gt nlf: MSE flt1 {mse_f1:.3f} flt2 {mse_f2:.3f}, of the noisy frames {noisy_mse:.3f}")
    # measured on the frame's scale, after the inverse: the 96 x 64 gamma row of DESIGN.md §9's table (34.83 34.75 35.08 dB
    # on the CPU oracle at zero flow), within the quality tests' 1 dB
    assert max(mse_f1, mse_f2) < noisy_mse and abs(10 * np.log10(255.0 ** 2 / mse_f2) - 34.89) <= 1.0


@pytest.mark.gpu
def test_gpu_nlk_sigma_nlf(ctx, built, nlf_run):
    """nlk-sigma --nlf prints x_j sigma_j per channel: the table of the restatement within the estimator's tolerance"""
    base = nlf_run[0]
    path = base / "in" / "001.pfm"
    r = run("nlk-sigma", "--nlf", path)
    assert r.returncode == 0, r.stderr
    want = nlf_ref.build(_bins(256, 192, G22))
    lines = r.stdout.splitlines()
    assert len(lines) == 3
    for c, line in enumerate(lines):
        f = line.split()
        assert f[0] == str(path) and (int(f[1]), int(f[2])) == (c, int(want["kept"][c])) and len(f) == 3 + 2 * 17
        v = np.array(f[3:], np.float64).reshape(17, 2)
        assert np.array_equal(v[:, 0], want["x"].astype(np.float64)) and _close(v[:, 1], want["sigma"][c], rel=1e-4)
    # parameters reach the estimator and the table
    r8 = run("nlk-sigma", "--nlf", "--nbins", 8, path)
    want8 = nlf_ref.build(_bins(256, 192, G22, nbins=8))
    f = r8.stdout.splitlines()[0].split()
    assert r8.returncode == 0 and len(f) == 3 + 2 * 9 and _close(np.array(f[4::2], np.float64), want8["sigma"][0], rel=1e-4)
