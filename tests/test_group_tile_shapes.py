"""The tile shapes a full-size frame gives the 8 x 8 group kernels, on frames small enough for the serial oracle.

The launcher (csrc/tu_group8.hip, shape_pass()) picks the targets per tile from the size of the patch grid: 3 x 2 with
one-row "tail" tiles and "single" targets at the end of a 1080p temporal frame, 2 x 2 / 3 x 2 for its first frame,
2 x 1 at 720p - and 1 x 1 for everything a quick test can afford. Here NLK_GTX / NLK_GTY / NLK_G8_TAIL /
NLK_G8_SINGLE force those shapes onto grids of a few hundred targets, and Context.last_group_shape() says what the
launch really ran: every test asserts it, so a switch the launcher ignored or clamped fails the test instead of
quietly running 1 x 1 tiles again.

Against the oracle: integer records exact (`_check_records`), pixels within the standing tolerance of
`cases.assert_close` after `cases.excuse_threshold_pixels`. Product against product: `cases.excuse_flips` and the
5e-4 / 5e-5 of the strip tests. Frames are `synth.noisy_pair` at sigma 20; a previous frame carries a NaN rectangle
and a NaN first column (spatial-branch targets inside a temporal frame)."""
import os

import numpy as np
import pytest

import cases
from test_gpu_parity import _check_records, _dev_frame, _random_config, _to_o

pytestmark = pytest.mark.gpu

SIGMA = 20.0
SHAPES = [(2, 1), (3, 1), (4, 1), (1, 2), (2, 2), (3, 2), (2, 3)]
CALLS = ("flt1 spatial", "flt1 temporal", "flt2", "smo1")
# (a): ngx = 53 is no multiple of 2, 3 or 4 and gives more than 16 tiles per row up to tgx = 3; ngy = 25 is odd and
# gives more than 4 tile rows at every tgy: the chunk order (16 x 4 tiles per chunk) wraps in both directions
FRAME_A = (216, 104)
# (b): ngy >= 17. 88 x 72: 21 x 17 targets - `single` rows of 21 targets are no multiple of 8 (ragged last run of
# the per-XCD decode), 17 - 0 - 0 and 17 - 2 - 4 are odd; 100 x 80: 24 x 19 - whole runs, 19 - 0 - 0 odd
FRAMES_B = {"21x17-rgb": (88, 72, 3), "24x19-gray": (100, 80, 1)}
SPLITS = [(0, 0), (1, 0), (0, 1), (3, 2), (99, 99), (None, None)]   # (NLK_G8_TAIL, NLK_G8_SINGLE); None = unset


def _grid(w, h):
    return (w - 8) // 4 + 1, (h - 8) // 4 + 1


def _holes(im):
    """A previous frame with a NaN rectangle and a NaN first column (test_large_patches_and_other_channel_counts)."""
    h, w = im.shape[:2]
    out = im.copy()
    out[h // 3:h // 3 + 5, w // 2:w // 2 + 9] = np.nan
    out[:, :1] = np.nan
    return out


_SCENES = {}


def _scene(O, built, w, h, ch, seed=5):
    """The four frame calls of one noisy pair and what the serial oracle makes of them, computed once per module run
    and never changed: name -> (smoother, (cur, prev, basic), params, oracle output, oracle trace)."""
    key = (w, h, ch, seed)
    if key not in _SCENES:
        n0, n1, _ = cases.synth.noisy_pair(w, h, ch, SIGMA, seed)
        o0, o1 = (O.rgb2opp(n0), O.rgb2opp(n1)) if ch == 3 else (n0, n1)
        p1, p2, ps = (built.default_params(SIGMA, m) for m in (built.FLT1, built.FLT2, built.SMO1))
        s = {}

        def add(name, smo, args, p):
            r, tr = (O.smooth_frame if smo else O.filter_frame)(*args, SIGMA, _to_o(O, p), trace=True)
            for a in (r, *tr.values()):
                if isinstance(a, np.ndarray):
                    a.setflags(write=False)
            s[name] = (smo, args, p, r, tr)
            return r
        r0 = add("flt1 spatial", False, (o0, None, None), p1)
        prev = _holes(r0)
        r1 = add("flt1 temporal", False, (o1, prev, None), p1)
        add("flt2", False, (o1, prev, r1), p2)
        add("smo1", True, (r0, _holes(r1), None), ps)
        _SCENES[key] = s
    return _SCENES[key]


def _flat_scene(O, built, w, h, ch):
    """FLT1 temporal on a zero-variance frame: every group's variance is 0 and its weight the clamp 1 / 1e-6
    (oracle/nlk_oracle.c, aggregate), so one missed or doubled target moves the summed weight of its pixels by a
    whole term."""
    key = (w, h, ch, "flat")
    if key not in _SCENES:
        cur = np.full((h, w, ch), 128.0, np.float32)
        p1 = built.default_params(SIGMA, built.FLT1)
        args = (cur, _holes(cur), None)
        r, tr = O.filter_frame(*args, SIGMA, _to_o(O, p1), trace=True)
        live = (tr["active"] > 0) & (tr["nagg"] > 0)
        assert live.sum() > 0.5 * live.size and (tr["vp"][live] == 0).all()   # (the weight clamp in every group)
        _SCENES[key] = {"flt1 temporal": (False, args, p1, r, tr)}
    return _SCENES[key]


def _run(ctx, call):
    smo, args, p = call[:3]
    return _dev_frame(ctx, smo, *args, SIGMA, p)


def _against_oracle(g, rec, call, what, flips=0):
    r, tr = call[3:]
    _check_records(rec, tr, what)
    g, _ = cases.excuse_threshold_pixels(g, r, tr, what, 16)
    cases.assert_close(g, r, what, flips=flips)


def _force(monkeypatch, tgx, tgy, tail=None, single=None):
    monkeypatch.setenv("NLK_GTX", str(tgx))
    monkeypatch.setenv("NLK_GTY", str(tgy))
    for name, v in (("NLK_G8_TAIL", tail), ("NLK_G8_SINGLE", single)):
        if v is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, str(v))


def _assert_ran(ctx, ngx, ngy, tgx, tgy, tail=None, single=None, family="k_group8m", uniform=False, what=""):
    """The last group launch ran tgx x tgy tiles over the ngx x ngy grid - and, for k_group8m outside deterministic
    mode, this many one-row tail tiles and single rows. tail / single None: the default formulas, which on a small grid
    come out above their clamps ngy / 4 and ngy / 8 (the code path of a 1080p frame)."""
    s = ctx.last_group_shape()
    what = f"{what}: asked for {tgx} x {tgy} tail {tail} single {single}, ran {s}"
    assert s["family"] == family, what
    assert (s["tgx"], s["tgy"], s["ntx"]) == (tgx, tgy, -(-ngx // tgx)), what
    if family != "k_group8m" or uniform or (tgx == 1 and tgy == 1):
        assert (s["nty"], s["nty_full"], s["single"]) == (-(-ngy // tgy),) * 2 + (0,), what
        return s
    single = ngy // 8 if single is None else min(max(single, 0), ngy // 8)
    tail = 0 if tgy == 1 else ngy // 4 if tail is None else min(max(tail, 0), ngy // 4)
    rows = ngy - single
    full = (rows - tail) // tgy
    assert (s["nty_full"], s["nty"], s["single"]) == (full, full + rows - full * tgy, single), what
    # (every grid row in exactly one kind of tile)
    assert s["nty_full"] * tgy + (s["nty"] - s["nty_full"]) + s["single"] == ngy, what
    return s


# ---------------------------------------------------------------- (a) shape x call x channels x DCT form

@pytest.mark.parametrize("ch", [1, 3])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_every_tile_shape_against_the_oracle(ctx, built, O, monkeypatch, shape, ch):
    """The seven multi-target shapes the launcher can pick, forced onto a 53 x 25 grid: the four frame calls, the three
    DCT forms of k_group8m and its default choice, one and three channels - each against the serial oracle, which runs
    once per (call, channel count). Tiles of two and three grid rows, ragged right and bottom edges, the default tail
    (6 rows) and single (3 rows) of that grid, a chunk order that wraps."""
    w, h = FRAME_A
    ngx, ngy = _grid(w, h)
    scene = _scene(O, built, w, h, ch)
    _force(monkeypatch, *shape)
    for sep in (None, 0, 2, 6):
        if sep is None:
            monkeypatch.delenv("NLK_GROUP_SEP", raising=False)
        else:
            monkeypatch.setenv("NLK_GROUP_SEP", str(sep))
        for name in CALLS:
            what = f"{shape[0]} x {shape[1]} tiles, {ch} ch, NLK_GROUP_SEP {sep}, {name}"
            g, rec = _run(ctx, scene[name])
            s = _assert_ran(ctx, ngx, ngy, *shape, what=what)
            assert s["sep"] == sep if sep is not None else s["sep"] in (0, 2, 6), what
            assert s["passes"] == 1, what
            _against_oracle(g, rec, scene[name], what)


def test_a_tile_of_more_targets_than_lanes_is_refused(ctx, built, monkeypatch):
    """A tile's target records sit one per lane of the tile's wavefront: 65 x 1 or 13 x 5 targets fit the LDS limit but
    not the 64 lanes. The launcher refuses them (and tiles of no targets) instead of launching."""
    w, h = FRAME_A
    cur = np.full((h, w, 1), 100.0, np.float32)
    p = built.default_params(SIGMA, built.FLT1)
    d_cur, d_out = ctx.upload(cur), ctx.alloc(cur.nbytes)
    try:
        for tgx, tgy in ((65, 1), (13, 5), (0, 1), (1, 0), (-2, 1)):
            _force(monkeypatch, tgx, tgy)
            with pytest.raises(built.NlkError, match="targets"):
                ctx.filter_frame(d_out, d_cur, None, None, w, h, 1, SIGMA, p)
            assert ctx.last_group_shape()["family"] is None
        _force(monkeypatch, 16, 4)   # (64 targets: the most a tile holds)
        ctx.filter_frame(d_out, d_cur, None, None, w, h, 1, SIGMA, p)
        _assert_ran(ctx, *_grid(w, h), 16, 4, what="16 x 4")
        assert np.abs(ctx.download(d_out, cur.shape) - cur).max() <= 2e-3   # (a flat frame comes back unchanged)
    finally:
        ctx.free(d_cur)
        ctx.free(d_out)


# ---------------------------------------------------------------- (b) tail and single rows on a small grid

@pytest.mark.parametrize("shape", [(3, 2), (2, 2)], ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("frame", list(FRAMES_B))
def test_tail_and_single_rows_on_a_small_grid(ctx, built, O, monkeypatch, frame, shape):
    """The end of a full-size launch - tile rows of one grid row, then grid rows worked one target per workgroup - for
    every split of the grid rows: none, one of each, both, more than the clamps allow, and the default formulas (which
    clamp, as at 1080p). FLT1 temporal and the smoother against the oracle; an odd number of rows left to the full
    tiles, and single targets that do not fill the last run of eight."""
    w, h, ch = FRAMES_B[frame]
    ngx, ngy = _grid(w, h)
    scene = _scene(O, built, w, h, ch, seed=9)
    for tail, single in SPLITS:
        _force(monkeypatch, *shape, tail, single)
        for name in ("flt1 temporal", "smo1"):
            what = f"{frame} {shape[0]} x {shape[1]} tiles, tail {tail} single {single}, {name}"
            g, rec = _run(ctx, scene[name])
            _assert_ran(ctx, ngx, ngy, *shape, tail, single, what=what)
            _against_oracle(g, rec, scene[name], what)


# ---------------------------------------------------------------- (c) grid geometry sweep

_NGX = [1, 2, 3, 4, 31, 32, 33, 48, 49, 65]
_NGY = [1, 2, 3, 7, 8, 9, 16, 17]


@pytest.mark.parametrize("i", range(len(_NGX)), ids=[f"ngx{n}" for n in _NGX])
def test_grid_geometry_sweep(ctx, built, O, monkeypatch, i):
    """3 x 2 tiles with the default tail and single rows over grids that cross the 32-target decision word, the 16-tile
    chunk width, the steps of the clamps ngy / 8 and ngy / 4 from 0 to 1, and grids smaller than one tile: FLT1
    temporal against the oracle. Every ngx with two ngy, every ngy with at least two ngx."""
    ngx = _NGX[i]
    _force(monkeypatch, 3, 2)
    for ngy in (_NGY[i % 8], _NGY[(i + 4) % 8]):
        w, h, ch = 8 + 4 * (ngx - 1), 8 + 4 * (ngy - 1), (3, 1)[i % 2]
        assert _grid(w, h) == (ngx, ngy)
        _, n1, _ = cases.synth.noisy_pair(w, h, ch, SIGMA, 40 + i)
        prev = cases.synth.awgn(cases.synth.clean_frame(w, h, ch, 0), 5.0, 80 + i).reshape(n1.shape)
        cur, prev = (O.rgb2opp(n1), O.rgb2opp(prev)) if ch == 3 else (n1, prev)
        prev = _holes(prev)
        p = built.default_params(SIGMA, built.FLT1)
        r, tr = O.filter_frame(cur, prev, None, SIGMA, _to_o(O, p), trace=True)
        call = (False, (cur, prev, None), p, r, tr)
        g, rec = _run(ctx, call)
        what = f"grid {ngx} x {ngy}, {ch} ch"
        _assert_ran(ctx, ngx, ngy, 3, 2, what=what)
        _against_oracle(g, rec, call, what)


# ---------------------------------------------------------------- (d) every target exactly once: the weight plane

# max over the pixels of |weight - oracle aggr| / aggr for the default 1 x 1 launch, measured on the inputs of these
# tests (see test_weight_plane_counts_every_target_once_by_shape), and the factor every launch gets: the forced shapes
# differ from the 1 x 1 launch in the order of the float sums only
WEIGHT_YARDSTICK = {"noisy flt1 temporal": 4.756e-6, "noisy smo1": 1.219e-5, "flat flt1 temporal": 1.289e-6}
WEIGHT_FACTOR = 4.0


def _weight_deviation(ctx, call):
    """Relative deviation of the weight plane that frame_accumulate leaves from the oracle trace's `aggr`."""
    smo, (cur, prev, basic), p, _, tr = call
    h, w, ch = cur.shape
    d = [ctx.upload(a) if a is not None else None for a in (cur, prev, basic)]
    d_acc = ctx.upload(np.zeros((ch + 1, h, w), np.float32))
    ctx.frame_accumulate(d_acc, d[0], d[1], d[2], w, h, ch, SIGMA, p, 0, _grid(w, h)[1], smoother=smo)
    wgt = ctx.download(d_acc, (ch + 1, h, w))[ch].astype(np.float64)
    for x in d + [d_acc]:
        if x:
            ctx.free(x)
    ref = tr["aggr"].astype(np.float64)
    assert np.array_equal(wgt == 0, ref == 0), "pixels without any weight differ"
    return float((np.abs(wgt - ref)[ref > 0] / ref[ref > 0]).max())


_VISIBLE = {}


def _least_visible_target(O, call):
    """How far ONE missed (or doubled) target moves the weight plane, at least: the oracle's `aggr` rebuilt in float64
    from its trace - weight 1 / max(vp, 1e-6) times the aggregation window at every member of every group - and, for
    the target that shows least, the largest share it has of any pixel's weight."""
    tr = call[4]
    if id(tr) not in _VISIBLE:
        h, w = tr["aggr"].shape
        win = np.asarray(O.window(8), np.float64).reshape(8, 8)
        ref = tr["aggr"].astype(np.float64)
        total, least = np.zeros((h, w)), np.inf
        for t in np.flatnonzero((tr["active"] > 0) & (tr["nagg"] > 0)):
            one = np.zeros((h, w))
            for m in tr["gcoords"][t, :tr["nagg"][t]]:
                x, y = int(m) & 0xffff, int(m) >> 16
                one[y:y + 8, x:x + 8] += win / max(float(tr["vp"][t]), 1e-6)
            total += one
            least = min(least, float((one[ref > 0] / ref[ref > 0]).max()))
        assert (np.abs(total - ref)[ref > 0] / ref[ref > 0]).max() <= 1e-5   # (this IS how the oracle sums)
        _VISIBLE[id(tr)] = least
    return _VISIBLE[id(tr)]


def _weights_once(ctx, O, monkeypatch, calls, ngx, ngy, shape, tail=None, single=None):
    for (frame, kind), call in calls.items():
        what = f"weight plane, {frame} {kind}, {shape[0]} x {shape[1]} tiles, tail {tail} single {single}"
        # (on these inputs any one target is 6 % or more of some pixel's weight: the bound sees it 1000 times over)
        assert _least_visible_target(O, call) >= 1000 * WEIGHT_FACTOR * WEIGHT_YARDSTICK[kind], what
        if shape == (1, 1):   # (the default of these grids: nothing set)
            for name in ("NLK_GTX", "NLK_GTY", "NLK_G8_TAIL", "NLK_G8_SINGLE"):
                monkeypatch.delenv(name, raising=False)
        else:
            _force(monkeypatch, *shape, tail, single)
        dev = _weight_deviation(ctx, call)
        _assert_ran(ctx, ngx, ngy, *shape, tail, single, what=what)
        bound = WEIGHT_FACTOR * WEIGHT_YARDSTICK[kind]
        print(f"{what}: {dev:.3e} (allowed {bound:.3e})")
        assert dev <= bound, f"{what}: {dev:.3e} from the oracle's weights, {WEIGHT_FACTOR} x {WEIGHT_YARDSTICK[kind]:.3e} allowed"


def test_weight_plane_of_the_default_launch(ctx, built, O, monkeypatch):
    """The yardstick itself: the 1 x 1 tiles these grids get with no switch set, on every input of the two tests
    below - printed, and held to the same bound."""
    for (w, h, ch), seed in [((*FRAME_A, 3), 5), ((*FRAME_A, 1), 5)] + [(f, 9) for f in FRAMES_B.values()]:
        scene, flat = _scene(O, built, w, h, ch, seed), _flat_scene(O, built, w, h, ch)
        calls = {(f"{w}x{h}x{ch}", "noisy flt1 temporal"): scene["flt1 temporal"],
                 (f"{w}x{h}x{ch}", "noisy smo1"): scene["smo1"],
                 (f"{w}x{h}x{ch}", "flat flt1 temporal"): flat["flt1 temporal"]}
        _weights_once(ctx, O, monkeypatch, calls, *_grid(w, h), (1, 1))


@pytest.mark.parametrize("ch", [1, 3])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_weight_plane_counts_every_target_once_by_shape(ctx, built, O, monkeypatch, shape, ch):
    """frame_accumulate returns the unnormalised accumulator: its weight plane is, per pixel, the sum of weight x window
    over every patch of every group - a target filtered twice or never shows there as a whole missing or doubled
    term: on these inputs every single target is at least 6 % of some pixel's weight (`_least_visible_target`, asserted
    against the bound), 16 % on the zero-variance frame, where every weight is the clamp 1e6. Compared with the oracle trace's `aggr` as max |w - aggr| / aggr over the pixels; pixels without
    weight must have none.

    Yardstick: the default 1 x 1 launch on the same inputs, five runs each, MI355X. FLT1 temporal, noisy:
    4.756e-6 (216 x 104 RGB), 3.580e-6 (gray), 4.595e-6 (88 x 72 RGB), 2.737e-6 (100 x 80 gray); smoother, noisy:
    1.219e-5, 9.465e-6, 1.039e-5, 6.959e-6; FLT1 temporal, flat: 1.190e-6, 1.289e-6, 1.131e-6, 1.100e-6 (the oracle sums
    in float32 too, in target order). WEIGHT_YARDSTICK holds the largest of each kind and every launch is allowed
    WEIGHT_FACTOR = 4 times it: a forced shape differs from the 1 x 1 launch in the order of the sums only."""
    w, h = FRAME_A
    calls = {(f"{ch} ch", "noisy flt1 temporal"): _scene(O, built, w, h, ch)["flt1 temporal"],
             (f"{ch} ch", "flat flt1 temporal"): _flat_scene(O, built, w, h, ch)["flt1 temporal"]}
    _weights_once(ctx, O, monkeypatch, calls, *_grid(w, h), shape)


@pytest.mark.parametrize("shape", [(3, 2), (2, 2)], ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("frame", list(FRAMES_B))
def test_weight_plane_counts_every_target_once_by_split(ctx, built, O, monkeypatch, frame, shape):
    """The same measure (see ..._by_shape for the yardstick) for every split of the grid rows into full tiles, one-row
    tiles and single targets: FLT1 temporal on the noisy and on the zero-variance frame, the smoother on the noisy
    one."""
    w, h, ch = FRAMES_B[frame]
    scene, flat = _scene(O, built, w, h, ch, seed=9), _flat_scene(O, built, w, h, ch)
    calls = {(frame, "noisy flt1 temporal"): scene["flt1 temporal"], (frame, "noisy smo1"): scene["smo1"],
             (frame, "flat flt1 temporal"): flat["flt1 temporal"]}
    for tail, single in SPLITS:
        _weights_once(ctx, O, monkeypatch, calls, *_grid(w, h), shape, tail, single)


# ---------------------------------------------------------------- (e) replay inside the launch, multi-row tiles

@pytest.mark.parametrize("shape", [(3, 2), (2, 3)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_mask_replay_in_the_launch_with_tiles_of_several_rows(ctx, built, O, monkeypatch, shape):
    """A tile of two or three grid rows waits for the decision words of all of them, and rescues itself by replaying
    down to its LAST row: the default launch (workgroup 0 replays), NLK_NO_CHASE=1 (the separate kernels) and
    NLK_CHASE_TEST_SKIP0=1 (every workgroup rescues itself; the wait is bounded) on a first frame (reach 2) and a
    temporal frame (reach 1). Same decisions in all three, the oracle's; same frames up to the order of the sums."""
    w, h = FRAME_A
    ngx, ngy = _grid(w, h)
    scene = _scene(O, built, w, h, 3)
    _force(monkeypatch, *shape)
    for name, reach in (("flt1 spatial", 2), ("flt1 temporal", 1)):
        call = scene[name]
        runs = {}
        for mode, switch in (("default", None), ("separate", "NLK_NO_CHASE"), ("self-rescue", "NLK_CHASE_TEST_SKIP0")):
            for sw in ("NLK_NO_CHASE", "NLK_CHASE_TEST_SKIP0"):
                monkeypatch.delenv(sw, raising=False)
            if switch:
                monkeypatch.setenv(switch, "1")
            what = f"{shape[0]} x {shape[1]} tiles, {name}, replay {mode}"
            g, rec = _run(ctx, call)
            s = _assert_ran(ctx, ngx, ngy, *shape, what=what)
            assert s["chase"] == (0 if mode == "separate" else reach), f"{what}: {s}"
            assert np.array_equal(rec["active"].astype(bool), call[4]["active"].astype(bool)), what
            _against_oracle(g, rec, call, what)
            runs[mode] = (g, rec)
        for mode in ("separate", "self-rescue"):
            what = f"{shape[0]} x {shape[1]} tiles, {name}: replay {mode} vs default"
            assert np.array_equal(runs[mode][1]["active"], runs["default"][1]["active"]), what
            a, _ = cases.excuse_flips(runs[mode][0], runs["default"][0], call[1][0], what, most=8)
            cases.assert_close(a, runs["default"][0], what, maxabs=5e-4, rmse=5e-5)


# ---------------------------------------------------------------- (g) deterministic mode

@pytest.fixture(scope="module")
def det_ctx(built):
    c = built.Context(0)
    c.set_deterministic(True)
    yield c
    c.close()


@pytest.mark.parametrize("shape", [(2, 1), (3, 2), (2, 2)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_deterministic_mode_over_multi_target_tiles(det_ctx, built, O, monkeypatch, shape):
    """Deterministic aggregation keeps uniform tiles (no tail, no single rows): slabs per tile, k_gather sums them in a
    fixed order - with ragged tiles at the right and, only in this mode, at the bottom edge (25 grid rows). A temporal
    frame whose spatial radius exceeds the temporal one runs a near and a far pass. Two runs bit for bit the same,
    and the oracle's frame without a single excused sample beyond the threshold pixels."""
    w, h = FRAME_A
    ngx, ngy = _grid(w, h)
    _force(monkeypatch, *shape)
    for ch in (3, 1):
        scene = _scene(O, built, w, h, ch)
        for name in ("flt1 temporal", "flt1 spatial", "smo1"):
            call = scene[name]
            what = f"deterministic, {shape[0]} x {shape[1]} tiles, {ch} ch, {name}"
            p = call[2]
            assert p.search_sz_x > p.search_sz_t or name == "smo1"
            a, rec = _run(det_ctx, call)
            s = _assert_ran(det_ctx, ngx, ngy, *shape, uniform=True, what=what)
            assert s["passes"] == (2 if name == "flt1 temporal" else 1) and s["chase"] == 0, f"{what}: {s}"
            assert s["far"] == (shape if name == "flt1 temporal" else None), f"{what}: {s}"
            b, _ = _run(det_ctx, call)
            assert np.array_equal(a, b, equal_nan=True), f"{what}: two runs differ"
            _against_oracle(a, rec, call, what, flips=0)


def test_deterministic_mode_on_the_packed_lane_kernel(det_ctx, built, O, monkeypatch):
    """Deterministic aggregation under NLK_GROUP_PACKED=1: k_groupp<8>, one target per tile, whose launcher takes its
    slabs, flags and counters from the same plan as k_group8m's (csrc/group_det.h) - a temporal frame's near and far
    pass each sized by its own tiles. Two runs bit for bit the same, and the oracle's frame without a single excused
    sample beyond the threshold pixels, as the matrix-core kernel gives on this scene."""
    w, h = FRAME_A
    monkeypatch.setenv("NLK_GROUP_PACKED", "1")
    for ch in (3, 1):
        scene = _scene(O, built, w, h, ch)
        for name in ("flt1 temporal", "flt1 spatial", "smo1"):
            call = scene[name]
            what = f"deterministic, k_groupp<8>, {ch} ch, {name}"
            p = call[2]
            assert p.search_sz_x > p.search_sz_t or name == "smo1"
            a, rec = _run(det_ctx, call)
            # (this launcher reports no shape, so the two passes of "flt1 temporal" follow from the radii above alone)
            assert det_ctx.last_group_shape()["family"] is None, what
            b, _ = _run(det_ctx, call)
            assert np.array_equal(a, b, equal_nan=True), f"{what}: two runs differ"
            _against_oracle(a, rec, call, what, flips=0)


# ---------------------------------------------------------------- (h) random parameters at 8 x 8

_RANDOM_SHAPES = [(3, 2), (2, 2), (2, 3), (4, 1)]


@pytest.mark.parametrize("part", range(len(_RANDOM_SHAPES)), ids=[f"{s[0]}x{s[1]}" for s in _RANDOM_SHAPES])
def test_randomised_parameters_under_full_size_shapes(ctx, built, O, monkeypatch, part):
    """The generator of test_randomised_parameters_and_shapes at patch size 8 - 60 configurations (NLK_RANDOM_SEED /
    NLK_RANDOM_COUNT as there), the tile shape cycling over 3 x 2, 2 x 2, 2 x 3, 4 x 1 with the default tail and single
    rows; every test id draws the whole sequence and runs the configurations of its shape. Search radii up to 15 (a
    halo wider than the tile), k above the window, groups above k, NaN holes, all three modes: records exact, pixels
    within that test's tolerance. Configurations the kernels refuse loudly (reach, LDS) are skipped as there, and at
    least 80 % must run: at patch size 8 the generator's radii stay within reach 3 (15 / 4) and the widest tile, 3 x 2
    targets with halo 15, takes 46 x 42 floats x 4 planes = 31 KB of the 160 KB - with seed 2024 none is refused."""
    rng = np.random.default_rng(int(os.environ.get("NLK_RANDOM_SEED", 2024)))
    want = int(os.environ.get("NLK_RANDOM_COUNT", 60))
    shape = _RANDOM_SHAPES[part]
    _force(monkeypatch, *shape)
    drawn = ran = 0
    for it in range(want):
        smoother, cur, prev, basic, sigma, p, what = _random_config(rng, built, 8)
        if it % len(_RANDOM_SHAPES) != part:
            continue
        drawn += 1
        what = f"random #{it}, {shape[0]} x {shape[1]} tiles: {what}"
        r, tr = (O.smooth_frame if smoother else O.filter_frame)(cur, prev, basic, sigma, _to_o(O, p), trace=True)
        try:
            g, rec = _dev_frame(ctx, smoother, cur, prev, basic, sigma, p)
        except built.NlkError as e:
            assert "reach" in str(e) or "LDS" in str(e), str(e)
            continue
        _assert_ran(ctx, *_grid(cur.shape[1], cur.shape[0]), *shape, what=what)
        _check_records(rec, tr, what)
        edge = np.abs(tr["aggr"] - 1e-6) <= 1e-10   # (as there: pixels AT the reference's absolute threshold)
        assert edge.sum() <= max(4, 0.02 * edge.size), what
        g = np.where(edge[..., None], r, g)
        cases.assert_close(g, r, what, maxabs=5e-3, rmse=5e-4)
        ran += 1
    assert ran >= 0.8 * drawn, f"only {ran} of {drawn} configurations ran"
