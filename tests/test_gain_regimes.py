"""The group kernels off the default line beta(sigma) at sigma 10..50 on mid-grey frames: low noise on bright frames,
10-bit and negative levels, a unit range, betas from 0 to 10.

k_group8m and k_groupp form their variances from sums, (T[1] - T[0] * T[0] * in1) * in1, made safe by a pivot (the
target patch's coefficient is subtracted first); k_group_lds runs the oracle's Welford recursion. At sigma
20 / level 128 a float32 variance from sums WITHOUT the pivot is wrong by 3e-4, which no pixel test sees; at sigma 1 /
level 245 by 50 %, at sigma 2 / level 1000 by 200 %. Every regime below runs the four frame calls (FLT1 spatial, FLT1
temporal, FLT2, SMO1) of one noisy pair

    clean = level + amp sin(x / 5) cos(y / 7),   n0, n1 = clean + sigma N(0, 1) from one seeded generator,
    cur = n1, prev = n0 with the NaN rectangle and NaN first column of test_group_tile_shapes._holes (spatial-branch
    targets inside a temporal frame), basic (FLT2) = (n0 + n1) / 2

through two references: the serial oracle (float32, Welford) and tests/ref_numpy.py (float64 statistics and gains,
weight plane summed in float64). The CPU test holds the two against each other, which fixes the yardsticks and shows
the inputs are well conditioned; the GPU tests hold every group kernel variant to the float64 one.

Left out on purpose:
  * beta_x = 0 on a spatial call: every coefficient with V1 < sigma^2 is 0 / 0 in the reference, the frame is NaN;
  * sigma >= 97.75: the default beta_x is <= 0 there and the gain has a pole (oracle and restatement differ by 11.7
    at sigma 100);
  * levels scaled above ~x 4: the reference's absolute `aggr > 1e-6` test passes every pixel through, nothing is
    filtered;
  * sigma 80 / 90: 37 % .. 94 % of the pixels pass through on temporal calls, which would hide the kernel.
"""
import numpy as np
import pytest

import cases
import ref_numpy
from test_group_tile_shapes import _holes

CALLS = ("flt1 spatial", "flt1 temporal", "flt2", "smo1")

# name: level, amp, sigma, and where they differ from 40 x 32 x 1 at 8 x 8 with default betas: scale (of frame and
# sigma), betas, patch size, frame size, channels
REGIMES = {
    "control": dict(level=128, amp=60, sigma=20),
    "bright-s0.5": dict(level=245, amp=8, sigma=0.5),
    "bright-s1": dict(level=245, amp=8, sigma=1),
    "bright-s2": dict(level=245, amp=8, sigma=2),
    "bright-s5": dict(level=245, amp=8, sigma=5),
    "level1000": dict(level=1000, amp=30, sigma=2),
    "negative": dict(level=-500, amp=10, sigma=1),
    "unit": dict(level=245, amp=8, sigma=2, scale=1 / 255),
    "beta0.01": dict(level=128, amp=60, sigma=20, betas=dict(beta_x=0.01, beta_t=0.01)),
    "beta0.3": dict(level=128, amp=60, sigma=20, betas=dict(beta_x=0.3, beta_t=0.3)),
    "beta10": dict(level=128, amp=60, sigma=20, betas=dict(beta_x=10.0, beta_t=10.0)),
    "beta_t0": dict(level=128, amp=60, sigma=20, betas=dict(beta_t=0.0)),
    "bright-s1-rgb": dict(level=245, amp=8, sigma=1, ch=3),
    "bright-s2-rgb": dict(level=245, amp=8, sigma=2, ch=3),
    "level1000-rgb": dict(level=1000, amp=30, sigma=2, ch=3),
    # kernels of their own: k_groupp<12>, k_groupp<8> at 5 x 5, k_group_lds<GroupAny>
    "p12-rgb": dict(level=245, amp=8, sigma=2, psz=12, size=(44, 36), ch=3),
    "p5-gray": dict(level=245, amp=8, sigma=2, psz=5, size=(30, 26)),
    "p17-gray": dict(level=245, amp=8, sigma=2, psz=17, size=(41, 33)),   # (4 x 3 targets: step 8)
}
REGIMES_8X8 = [r for r in REGIMES if "psz" not in REGIMES[r]]
REGIMES_OWN = [r for r in REGIMES if "psz" in REGIMES[r]]

# switches -> (family last_group_shape must report, DCT form or None); family None = another launcher than
# tu_group8.hip's (k_groupp, k_group_lds), which is all the shape record says about those
VARIANTS = {
    "default": ({}, "k_group8m", None),
    "sep0": ({"NLK_GROUP_SEP": "0"}, "k_group8m", 0),
    "sep2": ({"NLK_GROUP_SEP": "2"}, "k_group8m", 2),
    "sep6": ({"NLK_GROUP_SEP": "6"}, "k_group8m", 6),
    "ilp0": ({"NLK_GROUP_ILP": "0"}, "k_group8m", None),
    "packed": ({"NLK_GROUP_PACKED": "1"}, None, None),
    "generic": ({"NLK_GENERIC_GROUP": "1"}, None, None),
}
_SWITCHES = sorted({k for sw, _, _ in VARIANTS.values() for k in sw})

WEIGHT_FACTOR = 16.0   # (order of the 64 ch-term sums, FMA contraction, MFMA accumulation order, 1 ulp of v_rcp_f32)
WEIGHT_CAP = 1e-3      # (a lost pivot moves the weight by >= 2e-3: past this the test would stop seeing it)


def _scale(spec):
    """What "2e-3 on the 0..255 scale" is multiplied by: the frame's own scale factor, or level / 255 above 255."""
    if "scale" in spec:
        return spec["scale"]
    return max(abs(spec["level"]) / 255.0, 1.0)


def _inputs(name):
    spec = REGIMES[name]
    w, h = spec.get("size", (40, 32))
    ch, sc = spec.get("ch", 1), spec.get("scale", 1.0)
    rng = np.random.default_rng(2024)
    y, x, c = np.meshgrid(np.arange(h), np.arange(w), np.arange(ch), indexing="ij")
    clean = spec["level"] + spec["amp"] * np.sin(x / 5.0 + 0.7 * c) * np.cos(y / 7.0 - 0.7 * c)
    n0, n1 = (((clean + spec["sigma"] * rng.standard_normal(clean.shape)) * sc).astype(np.float32) for _ in range(2))
    return n0, n1, np.float32(spec["sigma"] * sc)


_REFS = {}


def _refs(O, name):
    """Both references of one regime's four calls, computed once per module run and never changed: call ->
    dict(smo, args, po (oracle Params), r, tr (oracle), r64, tr64 (restatement), Y, S)."""
    if name not in _REFS:
        spec = REGIMES[name]
        n0, n1, sigma = _inputs(name)
        prev = _holes(n0)
        over = dict(spec.get("betas", {}))
        if "psz" in spec:
            over["patch_sz"] = spec["psz"]
        p1, p2, ps = (O.default_params(sigma, m, **over) for m in (O.FLT1, O.FLT2, O.SMO1))
        basic = ((n0.astype(np.float64) + n1) / 2).astype(np.float32)
        out = {}
        for call, smo, args, po in (("flt1 spatial", False, (n1, None, None), p1),
                                    ("flt1 temporal", False, (n1, prev, None), p1),
                                    ("flt2", False, (n1, prev, basic), p2),
                                    ("smo1", True, (n1, prev, None), ps)):
            r, tr = (O.smooth_frame if smo else O.filter_frame)(*args, sigma, po, trace=True)
            r64, tr64 = ref_numpy.frame(*args, sigma, po.as_dict(), smoother=smo, trace=True)
            a32, a64 = tr["aggr"].astype(np.float64), tr64["aggr"]
            live = a64 > 0
            Y = float((np.abs(a32 - a64)[live] / a64[live]).max())
            for a in (r, r64, *tr.values(), *tr64.values(), *args):
                if isinstance(a, np.ndarray):
                    a.setflags(write=False)
            out[call] = dict(smo=smo, args=args, sigma=float(sigma), po=po, r=r, tr=tr, r64=r64, tr64=tr64, Y=Y,
                             S=_scale(spec))
        _REFS[name] = out
    return _REFS[name]


def _close(got, ref, what, S):
    cases.assert_close(got, ref, what, maxabs=2e-3 * S, rmse=2e-4 * S)


# ---------------------------------------------------------------- the references against each other (CPU)

@pytest.mark.parametrize("name", list(REGIMES))
def test_oracle_and_float64_restatement_agree(O, name):
    """Oracle (float32, Welford) against restatement (float64 statistics and gains) on every call of every regime:
    finite output, no pixel at the reference's `aggr > 1e-6` threshold, at most 25 % of the pixels passed through (a
    call that filters nothing is no coverage), pixels without any weight at the same places, pixels within the standing
    2e-3 / 2e-4 times the regime's scale; and the yardstick Y = max |aggr_oracle - aggr_64| / aggr_64 that the GPU
    tests multiply by 16, which must leave 16 Y <= 1e-3.

    Measured (this file's inputs): pixel differences 6.1e-5 .. 2.9e-4 on the 0..255 regimes (8.3e-7 = 2.1e-4 / 255 on
    the unit range), 5.2e-4 at level -500 (bar 3.9e-3), 1.1e-3 at level 1000 (bar 7.8e-3); Y 4.3e-7 .. 4.2e-5, the
    largest being sigma 0.5 SMO1 (4.2e-5) and level -500 SMO1 (3.4e-5), so 16 Y <= 6.8e-4; passed through at most
    12.5 %."""
    for call, c in _refs(O, name).items():
        what = f"{name}, {call}"
        r, r64, a32, a64, S = c["r"], c["r64"], c["tr"]["aggr"], c["tr64"]["aggr"], c["S"]
        through = float((a32 <= 1e-6).mean())
        d = float(np.abs(r.astype(np.float64) - r64).max())
        print(f"{what}: Y {c['Y']:.2e}, pixels differ by {d:.2e} (bar {2e-3 * S:.2e}), passed through {100 * through:.1f} %")
        assert np.isfinite(r).all() and np.isfinite(r64).all(), what
        assert not (np.abs(a32 - 1e-6) <= 1e-10).any(), f"{what}: pixels at the aggregation threshold"
        assert through <= 0.25, f"{what}: {100 * through:.0f} % of the pixels pass through"
        assert np.array_equal(a32 == 0, a64 == 0), f"{what}: pixels without any weight differ"
        assert np.array_equal(a32 <= 1e-6, a64 <= 1e-6), f"{what}: passed-through pixels differ"
        _close(r, r64, what, S)
        assert WEIGHT_FACTOR * c["Y"] <= WEIGHT_CAP, f"{what}: Y {c['Y']:.2e}"


# ---------------------------------------------------------------- the kernels against the float64 restatement (GPU)

def _to_built(built, po):
    return built.Params(*[getattr(po, k) for k, _ in po._fields_])


def _weight_deviation(ctx, O, c, p):
    """Relative deviation of the weight plane that frame_accumulate leaves from the restatement's float64 `aggr`."""
    cur, prev, basic = c["args"]
    h, w, ch = cur.shape
    d = [ctx.upload(a) if a is not None else None for a in (cur, prev, basic)]
    d_acc = ctx.upload(np.zeros((ch + 1, h, w), np.float32))
    ctx.frame_accumulate(d_acc, d[0], d[1], d[2], w, h, ch, c["sigma"], p, 0, O.grid_shape(w, h, p.patch_sz)[1],
                         smoother=c["smo"])
    wgt = ctx.download(d_acc, (ch + 1, h, w))[ch].astype(np.float64)
    for x in d + [d_acc]:
        if x:
            ctx.free(x)
    ref = c["tr64"]["aggr"]
    assert np.array_equal(wgt == 0, ref == 0), "pixels without any weight differ"
    return float((np.abs(wgt - ref)[ref > 0] / ref[ref > 0]).max())


def _check_regime(ctx, built, O, monkeypatch, name, variant):
    from test_gpu_parity import _check_records, _dev_frame
    switches, family, sep = VARIANTS[variant]
    for k in _SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in switches.items():
        monkeypatch.setenv(k, v)
    if "psz" in REGIMES[name]:
        family = None
    failures = []
    for call, c in _refs(O, name).items():
        what = f"{name}, {variant}, {call}"
        p, S = _to_built(built, c["po"]), c["S"]
        bound = WEIGHT_FACTOR * c["Y"]
        assert bound <= WEIGHT_CAP, f"{what}: the yardstick 16 Y = {bound:.2e} is past {WEIGHT_CAP}"

        def ran():
            s = ctx.last_group_shape()
            assert s["family"] == family, f"{what}: ran {s}"
            if family == "k_group8m":
                assert s["sep"] == sep if sep is not None else s["sep"] in (0, 2, 6), f"{what}: ran {s}"
        g, rec = _dev_frame(ctx, c["smo"], *c["args"], c["sigma"], p)
        ran()
        _check_records(rec, c["tr"], what)                                        # (a)
        dev = _weight_deviation(ctx, O, c, p)                                     # (c), measured before (b) asserts
        ran()
        err = float(np.nanmax(np.abs(g.astype(np.float64) - c["r64"])))
        print(f"{what}: weights {dev:.3e} (allowed {bound:.3e}, ratio to Y {dev / c['Y']:.2f}), "
              f"pixels {err:.3e} (allowed {2e-3 * S:.3e})")
        try:
            g, _ = cases.excuse_threshold_pixels(g, c["r64"], c["tr"], what, most=0)
            _close(g, c["r64"], what, S)                                          # (b)
            assert dev <= bound, f"{what}: weight plane {dev:.3e} from the float64 one, 16 x {c['Y']:.3e} allowed"
            if name == "beta_t0" and call != "flt1 spatial":                      # (d): a = 1
                cur = c["args"][0]
                same = np.abs(c["r"] - cur) <= 2e-3 * S
                assert same.any(), what
                assert (np.abs(g - cur)[same] <= 2e-3 * S).all(), f"{what}: a = 1 does not return the input"
        except AssertionError as e:   # (every call of the regime is measured and printed before the test fails)
            failures.append(str(e))
    assert not failures, "\n".join(failures)


@pytest.mark.gpu
@pytest.mark.parametrize("name", REGIMES_8X8)
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_group_kernel_variants_by_regime(ctx, built, O, monkeypatch, variant, name):
    """Every 8 x 8 group kernel - k_group8m by default, in each DCT form and under the default scheduler,
    k_groupp<8>, k_group_lds - on every 8 x 8 regime: (a) integer records exact against the oracle; (b) pixels within
    the scaled 2e-3 / 2e-4 of the float64 restatement, no pixel excused; (c) the weight plane frame_accumulate leaves
    within 16 Y of the restatement's float64 `aggr`, Y being the oracle's own distance from it; (d) with beta_t = 0
    the temporal calls return the input wherever the oracle does. last_group_shape() must name the kernel family (and
    DCT form) the switch asks for.

    Largest measured weight deviation as a multiple of Y, per kernel (MI355X, one run; 16 allowed): k_group8m 3.22
    by default, in the separable form and under the default scheduler (level -500, FLT2), 2.25 / 2.26 in the Kronecker /
    hybrid form; k_groupp<8> 1.44; k_group_lds 1.95. Largest pixel difference as a share of the scaled
    bar: 0.22 (sigma 5, FLT1 temporal, hybrid form). Nothing grows with the level: no cancellation.

    Sensitivity (not committed): with k_groupp's v1 / v0 formed from the sums as they would be WITHOUT the pivot
    (T0 + n x0, T1 + 2 x0 T0 + n x0^2, same formula), NLK_GROUP_PACKED=1 fails every regime: weights 50 Y on the
    control (pixels still inside 2e-3 there), 250 .. 1550 Y on the bright regimes, up to 46 800 Y at level 1000, and
    pixels past their bar on every bright, unit-range and level-1000 regime."""
    _check_regime(ctx, built, O, monkeypatch, name, variant)


@pytest.mark.gpu
@pytest.mark.parametrize("name", REGIMES_OWN)
def test_other_patch_sizes_bright_low_noise(ctx, built, O, monkeypatch, name):
    """The same four checks at level 245 / sigma 2 on the kernels other patch sizes get: k_groupp<12> (12 x 12 RGB),
    k_groupp<8> (5 x 5 gray), k_group_lds<GroupAny> (17 x 17 gray, the smallest frame with 4 x 3 targets).
    Measured weight deviation (MI355X, one run): 0.56 Y, 0.69 Y, 1.04 Y."""
    _check_regime(ctx, built, O, monkeypatch, name, "default")
