"""Matching and grouping on tie-dense and zero-variance frames.

On noise two candidates essentially never have the same distance and no coefficient has zero variance, so the tie cut
of the selection (nlk_match_select in k_match.h, its copy in k_bm_generic) and the variance clamps of the gains
(k_group8m.h, k_groupp.h, k_group_math.h) stay almost unexercised by the other suites. The frames here are built so
that those lines decide the result:

* tie-dense: seeded random samples 100 + 16 j, j < L. Every squared difference and every partial sum of a patch
  distance is an integer below 2^24 (32 x 32 x 3 x (16 (L-1))^2 <= 7.1e6 for L <= 4), so each float32 distance is exact
  in any summation order; the division by psz^2 ch is correctly rounded and monotone, so ties stay ties. Each test
  asserts in float64 numpy (exact for these values) that at least 25 % of the targets whose window holds more than k
  candidates have d[k-1] == d[k], and at least 10 % a tie class at the cut that spans two rounds of 64 window indices;
* structured ties: a frame tiled from one step x step block (zero distance at every multiple of step), a checkerboard;
* zero variance: flat frames, a flat half at 255 beside noise, the tiled frame under FLT2 with basic = cur (k = 20
  identical candidates). Temporal calls there get prev = cur with a NaN hole and a NaN first column.

(a) CPU: the two restatements (oracle/nlk_oracle.c, tests/ref_numpy.py) agree on every input, including the smoother's
0/0 gain (reference: src/nlkalman.c:1768) that the reference's max() macro (:15-18, :1824) turns into NaN output.
(b) GPU: tie-dense frames against the serial oracle on every selection path; records exact, pixels 2e-3 / 2e-4.
(c) GPU: zero-variance frames on every group kernel, the same assertions.
(d) GPU: the smoother's 0/0 corner: where the oracle gives NaN the product gives NaN or the input."""
import numpy as np
import pytest

import cases
import ref_numpy
from test_gpu_parity import _check_records, _dev_frame, _to_o
from test_long_lists import LARGE_GRID

gpu = pytest.mark.gpu
SIGMA = 20.0


# ---------------------------------------------------------------- inputs

def _levels(w, h, ch, L, seed):
    return (100 + 16 * np.random.default_rng(seed).integers(0, L, (h, w, ch))).astype(np.float32)


def _tiled(w, h, ch, L, step, seed):
    blk = _levels(step, step, ch, L, seed)
    return np.ascontiguousarray(np.tile(blk, (h // step + 1, w // step + 1, 1))[:h, :w])


def _checker(w, h, ch):
    yy, xx = np.mgrid[0:h, 0:w]
    return np.ascontiguousarray(np.repeat((100 + 16 * ((xx + yy) & 1))[..., None], ch, 2).astype(np.float32))


def _flat(w, h, ch, v=128.0):
    return np.full((h, w, ch), v, np.float32)


def _clip(w, h, ch, seed):
    """A clipped highlight beside texture: the left half flat at 255, the right half uniform noise."""
    im = np.random.default_rng(seed).uniform(0, 255, (h, w, ch)).astype(np.float32)
    im[:, :w // 2] = 255.0
    return im


def _holed(im):
    """A previous frame with a NaN block and a NaN first column (spatial-branch targets inside a temporal call)."""
    h, w = im.shape[:2]
    p = im.copy()
    p[h // 3:h // 3 + 6, w // 2:w // 2 + 9] = np.nan
    p[:, :1] = np.nan
    return p


def _make(kind, w, h, ch, L=0, seed=0, step=4):
    if kind == "levels":
        return _levels(w, h, ch, L, seed)
    if kind == "tiled":
        return _tiled(w, h, ch, L, step, seed)
    if kind == "checker":
        return _checker(w, h, ch)
    if kind == "flat":
        return _flat(w, h, ch)
    assert kind == "clip"
    return _clip(w, h, ch, seed)


# ---------------------------------------------------------------- the precondition: how tie-dense an input is

def _tie_density(img, psz, radius, k, sel=None):
    """Over the grid targets (those of the boolean grid `sel` if given) whose clipped window of `radius` holds more
    than k candidates: the fraction with d[k-1] == d[k] in the sorted distances, and the fraction whose tie class at
    that cut also spans two rounds of 64 window indices (raster order of the clipped window, as the kernels count
    them). Float64 sums of integers: exact."""
    im = img.astype(np.float64)
    h, w, _ = im.shape
    step = psz // 2
    nx, ny = w - psz + 1, h - psz + 1
    side = 2 * radius + 1
    D = np.full((side, side, ny, nx), np.inf)
    for dy in range(-radius, radius + 1):
        ya, yb = max(0, -dy), min(h, h - dy)
        for dx in range(-radius, radius + 1):
            xa, xb = max(0, -dx), min(w, w - dx)
            if yb - ya < psz or xb - xa < psz:
                continue
            e = ((im[ya + dy:yb + dy, xa + dx:xb + dx] - im[ya:yb, xa:xb]) ** 2).sum(-1)
            c = np.zeros((e.shape[0] + 1, e.shape[1] + 1))
            c[1:, 1:] = e.cumsum(0).cumsum(1)
            D[dy + radius, dx + radius, ya:yb - psz + 1, xa:xb - psz + 1] = \
                c[psz:, psz:] - c[:-psz, psz:] - c[psz:, :-psz] + c[:-psz, :-psz]
    ntargets = ncut = nspan = 0
    for gy, py in enumerate(range(0, ny, step)):
        for gx, px in enumerate(range(0, nx, step)):
            if sel is not None and not sel[gy, gx]:
                continue
            d = D[:, :, py, px].ravel()
            d = d[np.isfinite(d)]            # (the clipped window in raster order)
            if d.size <= k:
                continue
            ntargets += 1
            s = np.sort(d)
            if s[k - 1] == s[k]:
                ncut += 1
                idx = np.flatnonzero(d == s[k - 1])
                nspan += idx[0] // 64 != idx[-1] // 64
    assert ntargets > 0
    return ncut / ntargets, nspan / ntargets


def _assert_tie_dense(img, psz, radius, k, what, sel=None):
    cut, span = _tie_density(img, psz, radius, k, sel)
    print(f"{what}: tie at the cut {100 * cut:.0f} %, spanning two rounds {100 * span:.0f} %")
    assert cut >= 0.25 and span >= 0.10, f"{what}: not tie-dense ({cut:.2f}, {span:.2f})"


# ---------------------------------------------------------------- the four calls on one input, oracle side (cached)

_REF = {}


def _calls(O, kind, w, h, ch, L=0, seed=0, names=("flt1x", "flt1t", "flt2", "smo1"), **over):
    """name -> (smoother, cur, prev, basic, mode, overrides, oracle output, oracle trace), computed once per input.
    Tie-dense and tiled frames: prev = the oracle's own first-frame output with a hole; zero-variance frames (flat,
    clip, checker, or zerovar=True): prev = cur with the hole. (The checkerboard belongs there: its 61 same-parity
    candidates of a temporal window are identical, and a previous frame that differs from it by the 1e-4 of a filter's
    rounding makes the smoother's gain 0 / 1e-9 - the ill-conditioned neighbour of the 0/0 corner, on which the
    oracle itself returns NaN for some targets.) FLT2 matches on basic = cur."""
    key = (kind, w, h, ch, L, seed, names, tuple(sorted(over.items())))
    if key in _REF:
        return _REF[key]
    over = dict(over)
    zerovar = over.pop("zerovar", kind in ("flat", "clip", "checker"))
    cur = _make(kind, w, h, ch, L, seed, step=over.get("patch_sz", 8) // 2)
    smo_over = {k: v for k, v in over.items() if k not in ("search_sz_x", "npatches_x")}
    out = {}

    def run(name, smoother, prev, basic, mode, ov):
        p = O.default_params(SIGMA, mode, **ov)
        fn = O.smooth_frame if smoother else O.filter_frame
        r, tr = fn(cur, prev, basic, SIGMA, p, trace=True)
        out[name] = (smoother, cur, prev, basic, mode, ov, r, tr)
        return r
    if zerovar:
        prev = _holed(cur)
    else:
        r0 = run("flt1x", False, None, None, O.FLT1, over) if "flt1x" in names else \
            O.filter_frame(cur, None, None, SIGMA, O.default_params(SIGMA, O.FLT1, **over))
        prev = _holed(r0)
    if zerovar and "flt1x" in names:
        run("flt1x", False, None, None, O.FLT1, over)
    if "flt1t" in names:
        run("flt1t", False, prev, None, O.FLT1, over)
    if "flt2" in names:
        run("flt2", False, prev, cur, O.FLT2, over)
    if "flt2x" in names:
        run("flt2x", False, None, cur, O.FLT2, over)
    if "smo1" in names:
        run("smo1", True, prev, None, O.SMO1, smo_over)
    _REF[key] = out
    return out


def _gpu_check(ctx, built, O, call, what, report=None):
    """One call on the GPU against its cached oracle result: records exact, no pixel at the aggregation threshold,
    pixels within the project's tolerance."""
    smoother, cur, prev, basic, mode, ov, r, tr = call
    p = built.default_params(SIGMA, mode, **ov)
    assert _to_o(O, p).as_dict() == O.default_params(SIGMA, mode, **ov).as_dict()
    g, rec = _dev_frame(ctx, smoother, cur, prev, basic, SIGMA, p)
    _check_records(rec, tr, what)
    g, _ = cases.excuse_threshold_pixels(g, r, tr, what, 0)
    with np.errstate(invalid="ignore"):
        d = np.abs(g - r)
    d = d[np.isfinite(d)]
    if d.size:
        print(f"{what}: max-abs {d.max():.3e}, rmse {np.sqrt(np.mean(d ** 2)):.3e}")
    cases.assert_close(g, r, what)
    return g, rec


def _launch(monkeypatch, launch):
    """auto: small tiles, target by target. large-grid: the shapes of a full-size frame (2 x 2 blocks on 8 wavefronts
    where they exist, 4 x 2 blocks otherwise). large-grid-4x2: 4 x 2 blocks everywhere. noblock: NLK_MATCH_NOBLOCK.
    A '+block-order' suffix adds the opt-in NLK_MATCH_ORDER=block (8 x 8 patches)."""
    base, _, order = launch.partition("+")
    if base.startswith("large-grid"):
        for kv in LARGE_GRID:
            monkeypatch.setenv(*kv)
        if base == "large-grid-4x2":
            monkeypatch.setenv("NLK_MATCH_BX2", "0")
    elif base == "noblock":
        monkeypatch.setenv("NLK_MATCH_NOBLOCK", "1")
    elif base == "generic":
        monkeypatch.setenv("NLK_GENERIC_MATCH", "1")
    else:
        assert base == "auto"
    if order:
        monkeypatch.setenv("NLK_MATCH_ORDER", "block")


def _grid(tr, name):
    ngx, ngy = tr["grid"]
    return tr[name].reshape(ngy, ngx)


def _check_four(ctx, built, O, calls, psz, what, precondition=("flt1x", "flt1t", "flt2", "smo1")):
    """The tie-density precondition of each call (on the image it matches on, over the targets the oracle processed,
    with the radius and k of the call's dominant branch), then the GPU comparison."""
    for name, call in calls.items():
        smoother, cur, prev, basic, mode, ov, r, tr = call
        p = O.default_params(SIGMA, mode, **ov)
        act = _grid(tr, "active").astype(bool)
        if prev is None:
            radius, k, sel = p.search_sz_x, p.npatches_x, act
        else:
            radius, k, sel = p.search_sz_t, p.npatches_t, act & (_grid(tr, "np0") > 0)
        if name in precondition:
            _assert_tie_dense(cur, psz, radius, k, f"{what} {name}", sel)
        _gpu_check(ctx, built, O, call, f"{what} {name}")


# ---------------------------------------------------------------- (a) CPU: the two restatements agree

CPU_INPUTS = {
    "levels-gray-L4": ("levels", 48, 40, 1, 4, 11),
    "levels-rgb-L2": ("levels", 48, 40, 3, 2, 12),
    "tiled-gray-L4": ("tiled", 48, 40, 1, 4, 13),
    "checker-gray": ("checker", 48, 40, 1, 0, 0),
    "flat-gray": ("flat", 48, 40, 1, 0, 0),
    "flat-rgb": ("flat", 48, 40, 3, 0, 0),
    "clip-gray": ("clip", 48, 40, 1, 0, 14),
    "tiled-rgb-L2-zerovar": ("tiled", 48, 40, 3, 2, 15),
}


@pytest.mark.parametrize("name", ["flt1x", "flt1t", "flt2", "smo1"])
@pytest.mark.parametrize("inp", list(CPU_INPUTS))
def test_restatements_agree(O, inp, name):
    """oracle/nlk_oracle.c against tests/ref_numpy.py: same NaN pattern, max-abs <= 2e-3, RMSE <= 2e-4. On the flat
    frames the smoother call is the 0/0 corner: more than half of the oracle's samples are NaN, and ref_numpy must
    produce the same ones (its weight clamp in the form of the reference's macro)."""
    kind, w, h, ch, L, seed = CPU_INPUTS[inp]
    over = dict(zerovar=True) if inp.endswith("zerovar") else {}
    smoother, cur, prev, basic, mode, ov, r, tr = _calls(O, kind, w, h, ch, L, seed, **over)[name]
    assert not (np.abs(tr["aggr"] - 1e-6) <= 1e-10).any(), "a pixel sits at the aggregation threshold"
    with np.errstate(invalid="ignore"):   # (the 0/0 itself)
        n = ref_numpy.frame(cur, prev, basic, SIGMA, O.default_params(SIGMA, mode, **ov).as_dict(), smoother=smoother)
    nnan = int(np.isnan(r).sum())
    print(f"{inp} {name}: {nnan} NaN samples of {r.size}")
    if kind == "flat" and name == "smo1":
        assert nnan > r.size // 2, f"{inp}: only {nnan} of {r.size} samples are NaN: not the 0/0 corner"
    if name != "smo1":
        assert nnan == 0
    cases.assert_close(r, n, f"{inp} {name}: oracle vs ref_numpy")


# ---------------------------------------------------------------- (b) GPU: tie-dense frames on every selection path

# 8 x 8 patches, default radii: the first frame searches 441 candidates (7 rounds of 64), the temporal targets 121
# (2 rounds), the targets under the hole of the previous frame go to the wide queue (k_bm_wide: sx 10 > st 5)
TIES_8X8 = {"gray-L4": ("levels", 56, 48, 1, 4, 21), "rgb-L2": ("levels", 56, 48, 3, 2, 22),
            "tiled-L4": ("tiled", 56, 48, 1, 4, 23), "checker": ("checker", 56, 48, 3, 0, 0)}
LAUNCHES = ["auto", "large-grid", "large-grid-4x2", "noblock", "generic", "auto+block-order",
            "large-grid+block-order", "large-grid-4x2+block-order"]


@gpu
@pytest.mark.parametrize("launch", LAUNCHES)
@pytest.mark.parametrize("inp", list(TIES_8X8))
def test_ties_8x8_every_launch_shape(ctx, built, O, monkeypatch, inp, launch):
    """FLT1 spatial (M = 7), FLT1 temporal (M = 2, and k_bm_wide under the hole), FLT2 and SMO1 on the 8 x 8 inputs,
    for each launch shape of the matcher, k_bm_generic, and the opt-in block-summed order (exact sums: it must give
    the oracle's records bit for bit here)."""
    # (the checkerboard's smoother call is the 0/0 corner: test_smoother_zero_over_zero)
    names = ("flt1x", "flt1t", "flt2") if inp == "checker" else ("flt1x", "flt1t", "flt2", "smo1")
    calls = _calls(O, *TIES_8X8[inp], names=names)
    _launch(monkeypatch, launch)
    if inp in ("gray-L4", "rgb-L2"):
        _check_four(ctx, built, O, calls, 8, f"{inp} {launch}")
    else:   # (structured ties: the zero-distance class is the point, the density figures do not apply)
        for name, call in calls.items():
            _gpu_check(ctx, built, O, call, f"{inp} {launch} {name}")
    t = calls["flt1t"][7]
    wide = t["active"].astype(bool) & (t["np0"] == 0)
    assert wide.sum() > 0   # (spatial-branch targets inside the temporal call)


@gpu
@pytest.mark.parametrize("launch", ["auto", "large-grid", "large-grid-4x2", "noblock"])
def test_ties_wide_queue_lists_longer_than_the_temporal_window(ctx, built, O, monkeypatch, launch):
    """k_bm_wide with lists of 125 from its 441-candidate window: more than the 121 candidates of the temporal
    window, so a target that lost its way to the wide queue cannot have such a list."""
    calls = _calls(O, "levels", 64, 56, 1, 4, 31, names=("flt1t",), npatches_x=125, npatches_tagg=125)
    _launch(monkeypatch, launch)
    call = calls["flt1t"]
    p, tr = O.default_params(SIGMA, O.FLT1, **call[5]), call[7]
    assert (p.search_sz_x, p.search_sz_t) == (10, 5)
    spatial = _grid(tr, "active").astype(bool) & (_grid(tr, "np0") == 0)
    assert spatial.sum() > 10 and tr["nsel"][spatial.ravel()].max() == 125
    _assert_tie_dense(call[1], 8, 10, 125, f"wide {launch}", spatial)
    _gpu_check(ctx, built, O, call, f"wide queue {launch}")


@gpu
@pytest.mark.parametrize("launch", ["auto", "large-grid", "noblock"])
def test_ties_sixteen_rounds(ctx, built, O, monkeypatch, launch):
    """Radius 15: 961 candidates, M = 16, spatial and temporal, on a frame where some target has the full window."""
    calls = _calls(O, "levels", 64, 56, 1, 4, 41, names=("flt1x", "flt1t"), search_sz_x=15, search_sz_t=15)
    _launch(monkeypatch, launch)
    tr = calls["flt1x"][7]
    ngx, ngy = tr["grid"]
    px, py = np.meshgrid(np.arange(ngx) * 4, np.arange(ngy) * 4)
    full = (px >= 15) & (px + 15 <= 64 - 8) & (py >= 15) & (py + 15 <= 56 - 8)
    assert (full & _grid(tr, "active").astype(bool)).any()
    _check_four(ctx, built, O, calls, 8, f"radius 15 {launch}")


GENERIC = {"p7-ch2": dict(args=("levels", 47, 41, 2, 2, 51), psz=7, over=dict(patch_sz=7)),
           "radius16": dict(args=("levels", 56, 48, 1, 4, 52), psz=8, over=dict(search_sz_x=16, search_sz_t=16))}


@gpu
@pytest.mark.parametrize("inp", list(GENERIC))
def test_ties_generic_matcher(ctx, built, O, inp):
    """k_bm_generic where the plan itself chooses it: 7 x 7 patches with two channels, and radius 16 (1089
    candidates, more than the 16 rounds of the tiled kernels)."""
    cfg = GENERIC[inp]
    calls = _calls(O, *cfg["args"], names=("flt1x", "flt1t", "smo1"), **cfg["over"])
    _check_four(ctx, built, O, calls, cfg["psz"], f"generic {inp}")


LENGTHS = [(20, "auto"), (32, "auto"), (33, "auto"), (50, "auto"), (64, "auto"), (65, "auto"), (70, "auto"),
           (120, "auto"), (32, "large-grid"), (33, "large-grid"), (65, "large-grid-4x2"), (120, "large-grid"),
           (200, "large-grid"), (33, "generic"), (32, "noblock")]


@gpu
@pytest.mark.parametrize("k,launch", LENGTHS, ids=[f"k{k}-{l}" for k, l in LENGTHS])
def test_ties_list_lengths(ctx, built, O, monkeypatch, k, launch):
    """Both ranking branches of the selection (k <= 32: two lanes per survivor; above: 64 survivors per round) on
    both sides of their boundaries; k = 120 is more than every clipped temporal window holds (and one less than the
    full one), k = 200 more than the temporal window: the lists there are the whole window in distance order."""
    over = dict(npatches_x=k, npatches_t=k, npatches_tagg=k)
    calls = _calls(O, "levels", 52, 44, 1, 4, 60 + k, names=("flt1x", "flt1t"), **over)
    _launch(monkeypatch, launch)
    # (at k = 120 only the two largest distances of a full window are at the cut, at k = 200 no temporal window holds
    # more than k: the density figures are about the first frame's 441 candidates there)
    _check_four(ctx, built, O, calls, 8, f"k {k} {launch}", precondition=("flt1x", "flt1t") if k < 120 else ("flt1x",))
    assert calls["flt1x"][7]["nsel"].max() == k
    tt = calls["flt1t"][7]
    temporal = tt["active"].astype(bool) & (tt["np0"] > 0)
    assert tt["nsel"][temporal].max() == min(k, 121)
    if k >= 120:
        assert tt["nsel"][temporal].min() < 120   # (clipped windows shorter than the list)


PATCHES = [(psz, ch) for psz in (4, 6, 8, 10, 12, 16) for ch in (1, 3)]
SIZES = {4: (40, 40), 6: (44, 40), 8: (48, 40), 10: (56, 50), 12: (60, 52), 16: (64, 56), 20: (64, 56)}


def _patch_case(psz, ch):
    L = 2 if (psz >= 10 or ch == 3) else 4
    over = dict(patch_sz=psz)
    if psz == 4:
        over["search_sz_x"] = 6   # (radius 10 with step 2 reaches 5 grid cells: tests/cases.py's p4 case does the same)
    w, h = SIZES[psz]
    return ("levels", w, h, ch, L, 100 * psz + ch), over


@gpu
@pytest.mark.parametrize("launch", ["auto", "large-grid", "large-grid-4x2"])
@pytest.mark.parametrize("psz,ch", PATCHES, ids=[f"p{p}c{c}" for p, c in PATCHES])
def test_ties_patch_sizes(ctx, built, O, monkeypatch, psz, ch, launch):
    """Every instantiated patch size, gray and RGB, all four calls, auto and full-size launch shapes."""
    args, over = _patch_case(psz, ch)
    calls = _calls(O, *args, **over)
    _launch(monkeypatch, launch)
    _check_four(ctx, built, O, calls, psz, f"p{psz} ch{ch} {launch}")


@gpu
def test_ties_patch_20_on_the_lds_dct_route(ctx, built, O):
    """20 x 20 patches: k_bm_generic and the run-time shape of k_group_lds."""
    calls = _calls(O, "levels", 64, 56, 3, 2, 2003, names=("flt1x", "flt1t", "smo1"), patch_sz=20)
    _check_four(ctx, built, O, calls, 20, "p20 ch3")


# ---------------------------------------------------------------- (c) GPU: zero-variance frames on every group kernel

ZEROVAR = {"flat-gray": ("flat", 48, 40, 1, 0, 0), "flat-rgb": ("flat", 48, 40, 3, 0, 0),
           "clip-gray": ("clip", 48, 40, 1, 0, 71), "clip-rgb": ("clip", 48, 40, 3, 0, 72),
           "tiled-gray": ("tiled", 48, 40, 1, 4, 73), "tiled-rgb": ("tiled", 48, 40, 3, 2, 74)}
# ("dpp": NLK_GROUP_DPP selected the retired k_group8 and is ignored like any unknown variable now: these cases hold the
# default kernel to the same checks with it set)
GROUP_KERNELS = {"default": {}, "sep0": {"NLK_GROUP_SEP": "0"}, "sep2": {"NLK_GROUP_SEP": "2"},
                 "sep6": {"NLK_GROUP_SEP": "6"}, "dpp": {"NLK_GROUP_DPP": "1"}, "lds-dct": {"NLK_GENERIC_GROUP": "1"}}
ZV_NAMES = ("flt1x", "flt1t", "flt2", "flt2x")


def _zv_calls(O, inp, names=ZV_NAMES, **over):
    return _calls(O, *ZEROVAR[inp], names=names, zerovar=True, **over)


def _assert_flat_stays(g, cur, what):
    assert np.isfinite(g).all() and np.abs(g - cur).max() <= 2e-3, f"{what}: a flat frame must come back unchanged"


def _assert_zero_variance_reached(inp, calls):
    """The tiled frame under FLT2 with basic = cur and no previous frame: lists of 20 identical candidates, the
    oracle's vp exactly 0."""
    tr = calls["flt2x"][7]
    act = tr["active"].astype(bool)
    assert (tr["vp"][act & (tr["nsel"] == 20)] == 0).any(), f"{inp}: no target with zero variance"


@gpu
@pytest.mark.parametrize("kernel", list(GROUP_KERNELS))
@pytest.mark.parametrize("inp", list(ZEROVAR))
def test_zero_variance_frames(ctx, built, O, monkeypatch, inp, kernel):
    """FLT1 spatial, FLT1 temporal (prev = cur with a hole), FLT2 temporal and FLT2 spatial on frames whose kept
    candidates are identical: the oracle's Welford variance is exactly 0 there, the kernels' sum-of-squares variance
    a rounding residual of either sign in front of the clamps and the weight's 1e-6 floor."""
    calls = _zv_calls(O, inp)
    if inp.startswith("tiled"):
        _assert_zero_variance_reached(inp, calls)
    for k, v in GROUP_KERNELS[kernel].items():
        monkeypatch.setenv(k, v)
    for name, call in calls.items():
        g, _ = _gpu_check(ctx, built, O, call, f"{inp} {kernel} {name}")
        if inp.startswith("flat"):
            _assert_flat_stays(g, call[1], f"{inp} {kernel} {name}")


@gpu
@pytest.mark.parametrize("psz", [12, 6, 16])
@pytest.mark.parametrize("kind", ["flat", "clip", "tiled"])
def test_zero_variance_frames_packed_lane_kernel(ctx, built, O, kind, psz):
    """k_groupp (its own variance lines): 12 x 12, and 6 x 6 / 16 x 16 for its other two instantiations, RGB."""
    calls = _calls(O, kind, 60, 52, 3, 2, 80 + psz, names=ZV_NAMES, zerovar=True, patch_sz=psz,
                   search_sz_x=min(10, 3 * (psz // 2)))
    for name, call in calls.items():
        g, _ = _gpu_check(ctx, built, O, call, f"{kind} p{psz} {name}")
        if kind == "flat":
            _assert_flat_stays(g, call[1], f"flat p{psz} {name}")


@gpu
@pytest.mark.parametrize("inp", list(ZEROVAR))
def test_zero_variance_frames_deterministic_mode(built, O, monkeypatch, inp):
    """NLK_DETERMINISTIC=1: two runs bit-identical, and within tolerance of the oracle and of the default mode.
    (The switch is re-read by every live context, and an unset switch leaves a context's mode as it is: the test
    ends on NLK_DETERMINISTIC=0, which puts the session's context back into the default mode.)"""
    calls = _zv_calls(O, inp)
    c = built.Context(0)
    try:
        monkeypatch.setenv("NLK_DETERMINISTIC", "1")
        det = {}
        for name, call in calls.items():
            smoother, cur, prev, basic, mode, ov, r, tr = call
            a, _ = _gpu_check(c, built, O, call, f"{inp} deterministic {name}")
            b, _ = _dev_frame(c, smoother, cur, prev, basic, SIGMA, built.default_params(SIGMA, mode, **ov))
            assert np.array_equal(a, b, equal_nan=True), f"{inp} {name}: two deterministic runs differ"
            if inp.startswith("flat"):
                _assert_flat_stays(a, cur, f"{inp} deterministic {name}")
            det[name] = a
        monkeypatch.setenv("NLK_DETERMINISTIC", "0")
        for name, call in calls.items():
            smoother, cur, prev, basic, mode, ov, r, tr = call
            d, _ = _dev_frame(c, smoother, cur, prev, basic, SIGMA, built.default_params(SIGMA, mode, **ov))
            cases.assert_close(det[name], d, f"{inp} {name}: deterministic vs default mode")
    finally:
        monkeypatch.setenv("NLK_DETERMINISTIC", "0")
        c.close()


# ---------------------------------------------------------------- (d) GPU: the smoother's 0/0 corner

SMO_INPUTS = {"flat-gray": ("flat", 48, 40, 1, 0, 0), "flat-rgb": ("flat", 48, 40, 3, 0, 0),
              "tiled-gray": ("tiled", 48, 40, 1, 4, 73), "tiled-rgb": ("tiled", 48, 40, 3, 2, 74),
              "checker-rgb": ("checker", 56, 48, 3, 0, 0)}


@gpu
@pytest.mark.parametrize("kernel", list(GROUP_KERNELS))
@pytest.mark.parametrize("inp", list(SMO_INPUTS))
def test_smoother_zero_over_zero(ctx, built, O, monkeypatch, inp, kernel):
    """SMO1 with prev = cur (and a hole) on flat, step-periodic and checkerboard frames. The reference's gain is 0/0 there
    (src/nlkalman.c:1768) and its max() macro (:15-18, :1824) makes the weight 1e6 of a NaN patch: NaN output, which
    the oracle reproduces. A sum-of-squares variance cannot be required to be exactly 0, so this is the one place
    where the product may differ from the reference: where the oracle's sample is NaN the product's is NaN or within
    2e-3 of cur (with prev == cur every finite gain returns the member itself), and never anything else. Records
    exact; where the oracle is finite, the project's tolerance."""
    call = _calls(O, *SMO_INPUTS[inp], names=("smo1",), zerovar=True)["smo1"]
    smoother, cur, prev, basic, mode, ov, r, tr = call
    nan_r = np.isnan(r)
    if inp.startswith("flat"):
        assert nan_r.sum() > r.size // 2
    assert nan_r.any()
    for k, v in GROUP_KERNELS[kernel].items():
        monkeypatch.setenv(k, v)
    g, rec = _dev_frame(ctx, True, cur, prev, None, SIGMA, built.default_params(SIGMA, built.SMO1, **ov))
    what = f"smo1 0/0 {inp} {kernel}"
    _check_records(rec, tr, what)
    nan_g = np.isnan(g)
    with np.errstate(invalid="ignore"):
        near = np.abs(g - cur) <= 2e-3
    print(f"{what}: oracle NaN {int(nan_r.sum())} of {r.size}: product NaN {int((nan_r & nan_g).sum())}, "
          f"input {int((nan_r & near).sum())}, other {int((nan_r & ~nan_g & ~near).sum())}")
    assert (nan_g | near)[nan_r].all(), f"{what}: a sample is neither NaN nor the input where the reference is NaN"
    assert not nan_g[~nan_r].any(), f"{what}: NaN where the reference is finite"
    g, _ = cases.excuse_threshold_pixels(g, r, tr, what, 0)
    cases.assert_close(np.where(nan_r, 0, g), np.where(nan_r, 0, r), what)
