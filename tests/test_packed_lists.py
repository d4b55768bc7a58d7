"""k_group8m's packed-list instantiation against the 32-bit lists, on one build.

The tiled matchers leave every target's candidate and member lists a second time, as one byte per entry
(csrc/nlk_common.h: displacement from the target at the target's own search radius), and flag the targets whose
record is valid; k_group8m<.., PK = true> (csrc/k_group8m.h) reads a whole tile's records with two loads.
NLK_PACKED_LISTS=0 keeps the 32-bit lists in the same build. Every case here runs a call both ways and

  * asserts from Context.last_group_shape() which of the two ran - a silent fallback fails the test - and from
    Context.count_packed() that the matcher flagged exactly the targets whose record is valid: with no flag set every
    target would take the 32-bit lists INSIDE the packed kernel and nothing else would show it;
  * requires the integer records (k-NN lists, members, counts) and the processed-mask decisions to be identical;
  * in deterministic mode requires the accumulator to be BIT-identical: it is the same arithmetic on the same operands
    in the same order;
  * in the default mode (float atomics: the order of the sums changes from run to run) holds the two frames to the
    product-against-product tolerance of the strip tests, 5e-4 / 5e-5 after `cases.excuse_flips`.

One case per scene also goes against the serial oracle with the standing helpers. Frames and forced tile shapes are
those of test_group_tile_shapes.py; a previous frame with `_holes` puts spatial-branch targets - flag clear, 32-bit
lists - inside packed tiles."""
import importlib

import numpy as np
import pytest

import cases
from test_gpu_parity import _check_records, _dev_frame, _to_o
from test_group_tile_shapes import FRAME_A, SIGMA, _against_oracle, _assert_ran, _force, _grid, _holes, _run, _scene

pytestmark = pytest.mark.gpu

SWITCH = "NLK_PACKED_LISTS"


@pytest.fixture(scope="module")
def det_ctx(built):
    c = built.Context(0)
    c.set_deterministic(True)
    yield c
    c.close()


def _set_packed(monkeypatch, on):
    if on:
        monkeypatch.delenv(SWITCH, raising=False)
    else:
        monkeypatch.setenv(SWITCH, "0")


def _accumulate(ctx, call):
    smo, (cur, prev, basic), p = call[:3]
    h, w, ch = cur.shape
    d = [ctx.upload(a) if a is not None else None for a in (cur, prev, basic)]
    d_acc = ctx.upload(np.zeros((ch + 1, h, w), np.float32))
    ctx.frame_accumulate(d_acc, d[0], d[1], d[2], w, h, ch, SIGMA, p, 0, _grid(w, h)[1], smoother=smo)
    acc = ctx.download(d_acc, (ch + 1, h, w))
    for x in d + [d_acc]:
        if x:
            ctx.free(x)
    return acc


def _flagged_expected(call, rec):
    """How many targets the matcher must flag: none unless the call keeps packed lists at all (csrc/nlk_internal.h:
    nlk_packed_geom), else those with at most 32 kept candidates that searched a radius of at most 7. A target searched
    the temporal radius exactly when its own previous patch is valid, and then that patch - distance 0 - is among its
    candidates: np0 > 0. (Targets of a single-patch mode, nsel = 0, have no lists.)"""
    smo, (cur, prev, basic), p = call[:3]
    t = prev is not None
    kdom, rdom = (p.npatches_t, p.search_sz_t) if t else (p.npatches_x, p.search_sz_x)
    if smo or kdom > 32 or max(p.npatches_tagg, 1) > 32 or max(p.npatches_x, p.npatches_t) > 64 or rdom > 7:
        return 0
    r = np.where(rec["np0"] > 0, p.search_sz_t, p.search_sz_x) if t else np.full(rec["nsel"].shape, p.search_sz_x)
    return int(((rec["nsel"] >= 2) & (rec["nsel"] <= 32) & (r <= 7)).sum())


def _both_ways(ctx, det_ctx, monkeypatch, call, packed, what, shape=None, oracle=False, det_packed=None, ran=None):
    """The call with NLK_PACKED_LISTS=0 and with the default, on `ctx` (atomics) and on `det_ctx` (deterministic).
    `packed`: whether the default run must report the packed instantiation (the run with the switch at 0 never may);
    `det_packed`: the same for deterministic mode's near pass where it differs. `ran`: extra check of the shape
    report. Returns the default run's frame and records."""
    cur = call[1][0]
    w, h = cur.shape[1], cur.shape[0]
    out = {}
    for on in (False, True):
        _set_packed(monkeypatch, on)
        g, rec = _run(ctx, call)
        s = ctx.last_group_shape()
        assert s["family"] == "k_group8m", f"{what}: {s}"
        flagged, want_flagged = ctx.count_packed(), _flagged_expected(call, rec) if on else 0
        assert flagged == want_flagged, f"{what}, {SWITCH} {'unset' if on else 0}: {flagged} targets flagged, {want_flagged} expected"
        if packed and on:
            assert flagged > 0, what
        if shape:
            _assert_ran(ctx, *_grid(w, h), *shape[:2], *shape[2:], what=what)
        if ran:
            ran(s)
        assert s["packed_lists"] == (packed and on), f"{what}, {SWITCH} {'unset' if on else 0}: ran {s}"
        acc = _accumulate(det_ctx, call)
        sd = det_ctx.last_group_shape()
        want = packed if det_packed is None else det_packed
        assert sd["family"] == "k_group8m" and sd["packed_lists"] == (want and on), f"{what}, deterministic: ran {sd}"
        out[on] = (g, rec, acc)
    (g0, rec0, acc0), (g1, rec1, acc1) = out[False], out[True]
    assert np.array_equal(rec0["active"], rec1["active"]), f"{what}: processed-mask decisions differ"
    _check_records(rec1, {k: np.asarray(v) for k, v in rec0.items()}, f"{what}: packed against 32-bit lists")
    for f in ("nsel", "np0", "nagg"):
        assert np.array_equal(rec0[f], rec1[f]), f"{what}: {f} differs"
    assert np.array_equal(acc0.view(np.uint32), acc1.view(np.uint32)), \
        f"{what}: deterministic accumulators differ in {(acc0.view(np.uint32) != acc1.view(np.uint32)).sum()} words"
    a, _ = cases.excuse_flips(g1, g0, cur, what, most=8)
    cases.assert_close(a, g0, f"{what}: packed against 32-bit lists", maxabs=5e-4, rmse=5e-5)
    if oracle:
        _against_oracle(g1, rec1, call, what)
    return g1, rec1


def _call(O, built, cur, prev, basic, p, smoother=False):
    r, tr = (O.smooth_frame if smoother else O.filter_frame)(cur, prev, basic, SIGMA, _to_o(O, p), trace=True)
    return (smoother, (cur, prev, basic), p, r, tr)


def _pair(O, w, h, ch, seed):
    """(current frame, previous frame with holes): a noisy frame and the noisier-free neighbour of
    test_grid_geometry_sweep, in the opponent space for RGB."""
    _, n1, _ = cases.synth.noisy_pair(w, h, ch, SIGMA, seed)
    prev = cases.synth.awgn(cases.synth.clean_frame(w, h, ch, 0), 5.0, seed + 40).reshape(n1.shape)
    cur, prev = (O.rgb2opp(n1), O.rgb2opp(prev)) if ch == 3 else (n1, prev)
    return cur, _holes(prev)


# ---------------------------------------------------------------- holes, RGB: tile shapes

@pytest.mark.parametrize("shape", [(1, 1), (2, 2), (3, 2), (4, 2), (3, 3)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_holes_rgb_by_tile_shape(ctx, det_ctx, built, O, monkeypatch, shape):
    """216 x 104 RGB, FLT1 temporal and FLT2, the previous frame with a NaN rectangle and a NaN first column:
    spatial-branch and wide-window targets with the flag clear inside packed tiles. Tiles of 1 to 8 targets run
    packed; 3 x 3 = 9 targets do not fit the two registers and must report the 32-bit lists."""
    scene = _scene(O, built, *FRAME_A, 3)
    if shape == (1, 1):
        for name in ("NLK_GTX", "NLK_GTY", "NLK_G8_TAIL", "NLK_G8_SINGLE"):
            monkeypatch.delenv(name, raising=False)
    else:
        _force(monkeypatch, *shape)
    for name in ("flt1 temporal", "flt2"):
        call = scene[name]
        tr = call[4]
        if name == "flt1 temporal":   # (both kinds of target are there, and both get filtered)
            live = (tr["active"] > 0) & (tr["nagg"] > 0)
            assert (live & (tr["np0"] == 0)).sum() >= 8 and (live & (tr["np0"] > 0)).sum() >= 100
        _both_ways(ctx, det_ctx, monkeypatch, call, shape[0] * shape[1] <= 8,
                   f"holes RGB, {shape[0]} x {shape[1]} tiles, {name}", shape=shape, oracle=shape in ((3, 2), (4, 2)))


# ---------------------------------------------------------------- ragged single runs

@pytest.mark.parametrize("frame", [(88, 72, 3), (100, 80, 1)], ids=["21x17-rgb", "24x19-gray"])
def test_ragged_single_runs_and_edges(ctx, det_ctx, built, O, monkeypatch, frame):
    """3 x 2 tiles with NLK_G8_TAIL = 3 one-row tiles and NLK_G8_SINGLE = 2 rows of one target per workgroup (21
    targets per row: a ragged last run of eight), and ragged tiles - cx * cy below tgx * tgy - at the right and bottom
    edges: the lanes that load a tile's records are 8 per target of the tile as it is, not as it is shaped."""
    w, h, ch = frame
    scene = _scene(O, built, w, h, ch, seed=9)
    _force(monkeypatch, 3, 2, 3, 2)
    _both_ways(ctx, det_ctx, monkeypatch, scene["flt1 temporal"], True, f"{w} x {h} x {ch}, tail 3 single 2",
               shape=(3, 2, 3, 2), oracle=True)


# ---------------------------------------------------------------- clipped windows

def test_clipped_windows(ctx, det_ctx, built, O, monkeypatch):
    """24 x 20 RGB: 5 x 4 targets, every search window clipped on at least one side - the displacement is taken from
    the target, not from the clipped window's origin."""
    cur, prev = _pair(O, 24, 20, 3, 21)
    p = built.default_params(SIGMA, built.FLT1)
    call = _call(O, built, cur, prev, None, p)
    py = 4 * np.arange(4)
    assert ((py - p.search_sz_t < 0) | (py + p.search_sz_t > 20 - 8)).all()   # (every window clipped in y)
    for shape in ((1, 1), (3, 2)):
        _force(monkeypatch, *shape)
        _both_ways(ctx, det_ctx, monkeypatch, call, True, f"24 x 20, {shape[0]} x {shape[1]} tiles",
                   oracle=shape == (3, 2))


# ---------------------------------------------------------------- no valid previous patch

def test_no_valid_previous_patch(ctx, det_ctx, built, O, monkeypatch):
    """The previous frame all NaN except one block: np0 = 0 almost everywhere, the members are the first candidates.
    With the default parameters those targets searched radius 10 with 50 candidates - flag clear, every tile a mix; with
    a spatial radius of 7 and 32 candidates they are packed too, their members taken from the candidate list."""
    w, h = 88, 72
    cur, prev = _pair(O, w, h, 3, 23)
    blk = prev[24:48, 32:64].copy()
    prev[:] = np.nan
    prev[24:48, 32:64] = blk
    _force(monkeypatch, 3, 2)
    for tight in (False, True):
        p = built.default_params(SIGMA, built.FLT1)
        if tight:
            p.search_sz_x, p.npatches_x = 7, 32
        call = _call(O, built, cur, prev, None, p)
        tr = call[4]
        live = (tr["active"] > 0) & (tr["nagg"] > 0)
        assert (live & (tr["np0"] == 0)).sum() > 0.5 * live.sum() and (live & (tr["np0"] > 0)).sum() >= 4
        _both_ways(ctx, det_ctx, monkeypatch, call, True, f"one valid block, spatial radius {p.search_sz_x}",
                   oracle=True)


# ---------------------------------------------------------------- boundaries of eligibility

@pytest.mark.parametrize("field,value,packed", [("npatches_t", 32, True), ("npatches_t", 33, False),
                                                ("npatches_tagg", 32, True), ("npatches_tagg", 33, False),
                                                ("search_sz_t", 7, True), ("search_sz_t", 8, False)],
                         ids=lambda v: str(v))
def test_boundaries_of_eligibility(ctx, det_ctx, built, O, monkeypatch, field, value, packed):
    """A record holds 32 candidates, 32 members and a radius of 7 (225 candidates): one more of each and the launch
    reads the 32-bit lists."""
    w, h = 88, 72
    cur, prev = _pair(O, w, h, 3, 25)
    p = built.default_params(SIGMA, built.FLT1)
    if field == "npatches_tagg":
        p.npatches_t = 32   # (groups that fill the member list)
    setattr(p, field, value)
    call = _call(O, built, cur, prev, None, p)
    if packed and field != "search_sz_t":
        assert call[4]["nsel"].max() >= 32 and call[4]["nagg"].max() == min(32, p.npatches_tagg)
    _force(monkeypatch, 2, 2)
    # (deterministic mode at radius 8: the far pass has the wider halo, the near pass the temporal one)
    _both_ways(ctx, det_ctx, monkeypatch, call, packed, f"{field} = {value}", oracle=True)


# ---------------------------------------------------------------- off-path calls

def test_first_frame_and_smoother_keep_the_32_bit_lists(ctx, det_ctx, built, O, monkeypatch):
    """A first frame (50 candidates at radius 10) and the smoother (its instances are not packed) run as before,
    whatever the switch says."""
    scene = _scene(O, built, *FRAME_A, 3)
    _force(monkeypatch, 2, 2)
    for name in ("flt1 spatial", "smo1"):
        _both_ways(ctx, det_ctx, monkeypatch, scene[name], False, f"off path, {name}", oracle=True)


def test_two_bands_with_separate_commit_kernels(ctx, det_ctx, built, O, monkeypatch):
    """NLK_BANDS=2 and NLK_NO_CHASE=1: the second band's launch works on views offset by the band's first row - the
    packed records with them."""
    w, h = 104, 216
    ngx, ngy = _grid(w, h)
    cur, prev = _pair(O, w, h, 3, 27)
    p = built.default_params(SIGMA, built.FLT1)
    call = _call(O, built, cur, prev, None, p)
    monkeypatch.setenv("NLK_BANDS", "2")
    monkeypatch.setenv("NLK_NO_CHASE", "1")
    _force(monkeypatch, 3, 2)

    def ran(s):   # (the last launch is the second band's: fewer tile rows than the grid has)
        assert s["chase"] == 0 and s["nty_full"] * 2 + (s["nty"] - s["nty_full"]) + s["single"] < ngy, s
    banded, rec = _both_ways(ctx, det_ctx, monkeypatch, call, True, "two bands", ran=ran, oracle=True)
    monkeypatch.delenv("NLK_BANDS", raising=False)
    monkeypatch.delenv("NLK_NO_CHASE", raising=False)
    whole, rec_w = _run(ctx, call)
    assert ctx.last_group_shape()["packed_lists"]
    assert np.array_equal(rec["active"], rec_w["active"])
    a, _ = cases.excuse_flips(banded, whole, cur, "two bands against one", most=8)
    cases.assert_close(a, whole, "two bands against one", maxabs=5e-4, rmse=5e-5)


@pytest.mark.parametrize("fused", [False, True], ids=["separate", "fused"])
def test_strip_entry_points_on_two_strips(ctx, built, O, monkeypatch, fused):
    """The three-phase strip form on a two-strip split of 216 x 104 (test_gpu_exact_strips_equal_whole_frame): every
    strip's group launch must report the packed instantiation, and the frame equal the whole-frame call's - with the
    32-bit lists as well. Every strip's records (its own grid rows: k-NN lists, members, counts) are the same under both
    settings, its flagged targets those whose record is valid, and the packed frame the oracle's."""
    strips = importlib.import_module("bwd-nlkalman_amd.strips")
    w, h = FRAME_A
    ch = 3
    cur, prev = _pair(O, w, h, ch, 29)
    p = built.default_params(SIGMA, built.FLT1)
    call = _call(O, built, cur, prev, None, p)
    step = p.patch_sz // 2
    ngx, ngy = _grid(w, h)
    plan = strips.strip_plan(h, p.patch_sz, max(p.search_sz_x, p.search_sz_t), 2)
    _force(monkeypatch, 3, 2)
    frames, strip_recs = {}, {False: [], True: []}
    for on in (False, True):
        _set_packed(monkeypatch, on)
        whole, rec = _dev_frame(ctx, False, cur, prev, None, SIGMA, p)
        assert ctx.last_group_shape()["packed_lists"] == on
        d_marks = ctx.upload(np.zeros(ngx * ngy, np.uint64))
        d_active = ctx.upload(np.zeros(ngx * ngy, np.uint8))
        bufs = []
        for s in plan:
            cur_s, prev_s = (np.ascontiguousarray(a[s["Y0"]:s["Y1"]]) for a in (cur, prev))
            d_cur, d_prev = ctx.upload(cur_s), ctx.upload(prev_s)
            oy, ngy_l = s["gy0"] * step - s["Y0"], s["gy1"] - s["gy0"]
            reach = ctx.strip_match(d_marks + 8 * s["gy0"] * ngx, d_cur, d_prev, None, w, cur_s.shape[0], ch, SIGMA, p,
                                    oy, ngy_l)
            bufs.append((d_cur, d_prev, cur_s.shape[0], oy, ngy_l))
        ctx.mask_commit(d_marks, ngx, ngy, reach, d_active)
        assert np.array_equal(ctx.download(d_active, (ngx * ngy,), np.uint8), rec["active"])
        acc = np.zeros((ch + 1, h, w), np.float32)
        for s, (d_cur, d_prev, hl, oy, ngy_l) in zip(plan, bufs):
            ctx.strip_match(None, d_cur, d_prev, None, w, hl, ch, SIGMA, p, oy, ngy_l)
            srec = ctx.read_records()
            strip_call = (False, (cur[s["Y0"]:s["Y1"]], prev[s["Y0"]:s["Y1"]], None), p)
            assert ctx.count_packed() == (_flagged_expected(strip_call, srec) if on else 0), f"strip at row {s['gy0']}"
            strip_recs[on].append(srec)
            d_acc = ctx.upload(np.zeros((ch + 1, hl, w), np.float32))
            if fused:
                d_scratch = ctx.upload(np.full(ngx * ngy, 7, np.uint8))
                ctx.strip_commit_group(d_acc, d_marks, ngx, ngy, reach, s["gy0"], d_scratch)
                ctx.free(d_scratch)
            else:
                ctx.strip_group(d_acc, d_active + s["gy0"] * ngx)
            ran = ctx.last_group_shape()
            assert (ran["family"], ran["tgx"], ran["tgy"]) == ("k_group8m", 3, 2) and (ran["chase"] > 0) == fused, ran
            assert ran["packed_lists"] == on, f"strip at row {s['gy0']}, {SWITCH} {'unset' if on else 0}: ran {ran}"
            acc[:, s["Y0"]:s["Y1"]] += ctx.download(d_acc, (ch + 1, hl, w))
            for x in (d_cur, d_prev, d_acc):
                ctx.free(x)
        d_acc, d_cur, d_out = ctx.upload(acc), ctx.upload(cur), ctx.alloc(cur.nbytes)
        ctx.frame_normalize(d_out, d_acc, d_cur, w, h, ch, 0, h)
        got = ctx.download(d_out, cur.shape)
        for x in (d_acc, d_cur, d_out, d_marks, d_active):
            ctx.free(x)
        what = f"two strips against the whole frame (fused {fused}, {SWITCH} {'unset' if on else 0})"
        a, _ = cases.excuse_flips(got, whole, cur, what, most=8)
        cases.assert_close(a, whole, what, maxabs=5e-4, rmse=5e-5)
        frames[on] = (got, rec)
    for r0, r1 in zip(strip_recs[False], strip_recs[True]):
        for f in ("nsel", "np0", "nagg"):
            assert np.array_equal(r0[f], r1[f]), f"strips: {f} differs between the two settings"
        r0 = dict(r0, active=np.ones_like(r0["active"]))   # (a strip's decisions are the whole grid's: every list compared)
        _check_records(dict(r1, active=r0["active"]), r0, "strips: packed against 32-bit lists")
    a, _ = cases.excuse_flips(frames[True][0], frames[False][0], cur, "strips: packed against 32-bit lists", most=8)
    cases.assert_close(a, frames[False][0], "strips: packed against 32-bit lists", maxabs=5e-4, rmse=5e-5)
    _against_oracle(*frames[True], call, f"two strips (fused {fused}) against the oracle")
