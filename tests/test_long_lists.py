"""Candidate lists and groups of more than 128 entries (-m gpu).

Above 128 entries (list capacities: k = max(npatches_x, npatches_t), group = npatches_tagg) the group phase leaves
the tuned kernels: patch sizes 4 / 6 / 8 / 10 / 12 / 16 with 1 or 3 channels go to the fixed shapes of the LDS-DCT
kernel (k_group_lds.h, GroupFixed), every other shape to its run-time shape (GroupAny). The smoother's default
capacity, int(3 sigma - 15), crosses 128 at sigma = 48, so default parameters reach this path. The matcher sizes its
per-wavefront list space by the capacities as well (nlk_hip.hip, plan_frame): 8 wavefronts, then 4, then
k_bm_generic, which refuses above 160 KiB of LDS.

Every case is compared with the serial oracle: integer records (k-NN lists, groups, np0, nagg, mask decisions)
exactly, pixels within the bar of the neighbouring tests (tests/test_gpu_parity.py), excusing only the pixels whose
summed weight sits at the reference's aggregation threshold (cases.excuse_threshold_pixels)."""
import os

import numpy as np
import pytest

import cases
from test_gpu_parity import GOLD, _check_records, _dev_frame, _to_o

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "bwd-nlkalman_amd", "bin")
LDS_MAX = 160 * 1024         # the matcher's LDS budget per workgroup (nlk_hip.hip: plan_frame, tu_match.hip)
BM_THREADS, BM_WAVES = 256, 4  # NLK_BM_THREADS / NLK_BM_WAVES (k_match.h)


def _frames(w, h, ch, sigma, seed):
    """Two noisy frames of a smooth ramp: many near-equal patches, so that long lists are full and ranked by
    small distance differences."""
    rng = np.random.default_rng(seed)
    clean = np.add.outer(np.linspace(30, 200, h), np.linspace(0, 40, w))[..., None] * np.ones(ch)
    clean = clean + 25 * np.sin(np.arange(w) / 5.0)[None, :, None] * np.cos(np.arange(h) / 7.0)[:, None, None]
    n0 = (clean + rng.normal(0, sigma, clean.shape)).astype(np.float32)
    n1 = (clean + rng.normal(0, sigma, clean.shape)).astype(np.float32)
    return n0, n1


def _holed(im):
    """A previous frame with a NaN block and a NaN first column (spatial-branch targets inside a temporal call)."""
    h, w = im.shape[:2]
    p = im.copy()
    p[h // 3:h // 3 + 6, w // 2:w // 2 + 9] = np.nan
    p[:, :1] = np.nan
    return p


def _compare(ctx, O, smoother, cur, prev, basic, sigma, p, what, maxabs=5e-3, rmse=5e-4, most=None):
    fn = O.smooth_frame if smoother else O.filter_frame
    r, tr = fn(cur, prev, basic, sigma, _to_o(O, p), trace=True)
    g, rec = _dev_frame(ctx, smoother, cur, prev, basic, sigma, p)
    _check_records(rec, tr, what)
    h, w = cur.shape[:2]
    g, _ = cases.excuse_threshold_pixels(g, r, tr, what, max(4, int(0.02 * h * w)) if most is None else most)
    cases.assert_close(g, r, what, maxabs=maxabs, rmse=rmse)
    return r, tr


def _four_modes(ctx, built, O, w, h, ch, sigma, seed, what, **over):
    """FLT1 spatial, FLT1 temporal (NaN block + NaN first column in the previous frame), FLT2, SMO1."""
    n0, n1 = _frames(w, h, ch, sigma, seed)
    p1 = built.default_params(sigma, built.FLT1, **over)
    p2 = built.default_params(sigma, built.FLT2, **over)
    ps = built.default_params(sigma, built.SMO1, **{k: v for k, v in over.items() if k != "npatches_x"})
    r0, t0 = _compare(ctx, O, False, n0, None, None, sigma, p1, f"{what}: flt1 spatial")
    prev = _holed(r0)
    r1, t1 = _compare(ctx, O, False, n1, prev, None, sigma, p1, f"{what}: flt1 temporal")
    _compare(ctx, O, False, n1, prev, r1, sigma, p2, f"{what}: flt2")
    _compare(ctx, O, True, r0, _holed(r1), None, sigma, ps, f"{what}: smo1")
    return t0, t1


def _long(n, psz, over=None):
    """List length n on every route: both capacities, and windows that hold more than n candidates (radius at
    least 6, below the reach that needs the coordinate-list mask replay where the patch allows)."""
    r = 6
    while (2 * r + 1) ** 2 <= n:
        r += 1
    d = dict(patch_sz=psz, npatches_x=n, npatches_t=n, npatches_tagg=n, search_sz_x=r + 1, search_sz_t=r)
    d.update(over or {})
    return d


# ---------------------------------------------------------------- 1. the 128 boundary on every route

SHAPES = [(8, 3, (72, 56)), (8, 1, (64, 60)), (12, 3, (84, 66)), (6, 1, (61, 53)), (16, 3, (88, 72)),
          (7, 3, (67, 51)), (5, 1, (53, 50)), (8, 2, (70, 58)), (12, 4, (78, 62)), (20, 3, (90, 70))]
LENGTHS = [(psz, ch, size, n) for psz, ch, size in SHAPES for n in (128, 129)] + \
          [(psz, ch, size, n) for psz, ch, size in SHAPES[:1] + SHAPES[2:3] for n in (64, 65, 127, 200)]


@pytest.mark.parametrize("psz,ch,size,n", LENGTHS, ids=[f"p{p}c{c}-n{n}" for p, c, _, n in LENGTHS])
def test_list_length_boundary(ctx, built, O, psz, ch, size, n):
    """List lengths on both sides of 128 (k_groupp / k_group8m below, k_group_lds above), for the
    patch sizes and channel counts of every group route; lists really that long."""
    w, h = size
    t0, t1 = _four_modes(ctx, built, O, w, h, ch, 20.0, 1000 * psz + 10 * ch + n, f"p{psz} ch{ch} n{n}",
                         **_long(n, psz))
    assert t0["nsel"].max() == n and t1["nsel"].max() == n   # (the lists are full somewhere)
    assert t0["nagg"].max() == n


@pytest.mark.parametrize("over", [dict(npatches_t=30, npatches_tagg=129), dict(npatches_x=129, search_sz_x=4)],
                         ids=["group-capacity-129", "k-capacity-129-short-window"])
def test_capacity_alone_selects_the_long_route(ctx, built, O, over):
    """A capacity above 128 with short lists: the group size alone (nt 30, nt_agg 129), or k alone with a window
    of 81 candidates."""
    t0, t1 = _four_modes(ctx, built, O, 76, 60, 3, 20.0, 77, f"capacity {over}", **over)
    assert max(t0["nagg"].max(), t1["nagg"].max()) < 128   # (short lists in long capacities)


# ---------------------------------------------------------------- 2. k_group_lds on the short lists

@pytest.mark.parametrize("name", list(cases.CASES))
def test_lds_dct_group_kernel_stagewise_vs_oracle_and_golden(built, O, monkeypatch, name):
    """NLK_GENERIC_GROUP=1: the LDS-DCT kernel (k_group_lds<GroupFixed<PSZ, CH>, SMO>) on the seeded cases, with the assertions of
    test_pipeline_stagewise_vs_oracle_and_golden, golden files included."""
    monkeypatch.setenv("NLK_GENERIC_GROUP", "1")
    ref = cases.run_chain(O, name)
    got = cases.run_chain_stagewise(built, ref, name)
    for k in ("f1_0", "f2_0", "w1", "w2", "f1_1", "f2_1", "ws", "s1_0", "rgb_f2_1"):
        cases.assert_close(got[k], ref[k], f"{name}/{k}")
    with np.load(os.path.join(GOLD, name + ".npz")) as g:
        for k in g.files:
            cases.assert_close(got[k], g[k], f"golden {name}/{k}")


# ---------------------------------------------------------------- 3. sigma around the smoother's switch

def _smoother_inputs(O, w, h, ch, sigma, seed):
    n0, n1 = _frames(w, h, ch, sigma, seed)
    p1 = O.default_params(sigma, O.FLT1)
    f0 = O.filter_frame(n0, None, None, sigma, p1)
    return f0, _holed(O.filter_frame(n1, f0, None, sigma, p1))


@pytest.mark.parametrize("sigma,cap", [(47.9, 128), (48.0, 129), (50.0, 135), (60.0, 165)])
@pytest.mark.parametrize("w,h,ch", [(96, 64, 3), (70, 53, 1)])
def test_smoother_defaults_around_the_switch(ctx, built, O, sigma, cap, w, h, ch):
    ps = built.default_params(sigma, built.SMO1)
    assert (ps.npatches_t, ps.npatches_tagg) == (cap, cap)
    f0, prev = _smoother_inputs(O, w, h, ch, sigma, int(sigma * 10) + ch)
    _compare(ctx, O, True, f0, prev, None, sigma, ps, f"smo1 defaults sigma {sigma} {w}x{h}x{ch}", maxabs=2e-3,
             rmse=2e-4)


@pytest.mark.parametrize("psz,ch", [(7, 3), (8, 4), (8, 2)])
def test_smoother_defaults_sigma50_other_shapes(ctx, built, O, psz, ch):
    """The sigma = 50 default smoother (lists of 135) with an odd patch and with 4 and 2 channels: shapes the
    LDS-DCT kernel is not instantiated for."""
    sigma = 50.0
    f0, prev = _smoother_inputs(O, 80, 62, ch, sigma, 50 + psz + ch)
    ps = built.default_params(sigma, built.SMO1, patch_sz=psz)
    assert ps.npatches_t == 135
    _compare(ctx, O, True, f0, prev, None, sigma, ps, f"smo1 sigma 50 psz {psz} ch {ch}", maxabs=2e-3, rmse=2e-4)


def test_chain_sigma50_640x360(ctx, built, O, synth):
    """FLT1 -> FLT2 -> SMO1 at sigma = 50 on 640x360 RGB, stage by stage on the oracle's outputs (two frames; the
    smoother's default lists of 135 entries)."""
    w, h, ch, sigma = 640, 360, 3, 50.0
    n0, n1, _ = synth.noisy_pair(w, h, ch, sigma, 50)
    o0, o1 = built.rgb2opp(n0), built.rgb2opp(n1)
    p1, p2, ps = (built.default_params(sigma, m) for m in (built.FLT1, built.FLT2, built.SMO1))
    kw = dict(maxabs=2e-3, rmse=2e-4, most=64)
    f1_0, _ = _compare(ctx, O, False, o0, None, None, sigma, p1, "640x360 flt1 spatial", **kw)
    f2_0, _ = _compare(ctx, O, False, o0, None, f1_0, sigma, p2, "640x360 flt2 spatial", **kw)
    f1_1, _ = _compare(ctx, O, False, o1, f2_0, None, sigma, p1, "640x360 flt1 temporal", **kw)
    f2_1, _ = _compare(ctx, O, False, o1, f2_0, f1_1, sigma, p2, "640x360 flt2 temporal", **kw)
    _, ts = _compare(ctx, O, True, f2_0, f2_1, None, sigma, ps, "640x360 smo1", **kw)
    assert ts["nagg"].max() > 0 and ps.npatches_tagg == 135


def test_smoother_sigma50_full_size_1080p(ctx, built, O, synth):
    """flt1 -> smo1 at 1080p RGB and sigma = 50 (lists of 135: the LDS-DCT kernel at full size), serial oracle;
    mirrors tests/test_gpu_parity.py::test_smoother_full_size_1080p."""
    w, h, ch, sigma = 1920, 1080, 3, 50.0
    n0, n1, _ = synth.noisy_pair(w, h, ch, sigma, 1)
    o0, o1 = built.rgb2opp(n0), built.rgb2opp(n1)
    p1, ps = built.default_params(sigma, built.FLT1), built.default_params(sigma, built.SMO1)
    f0, _ = _dev_frame(ctx, False, o0, None, None, sigma, p1)
    f1, _ = _dev_frame(ctx, False, o1, f0, None, sigma, p1)
    g, rec = _dev_frame(ctx, True, f0, f1, None, sigma, ps)
    r, tr = O.smooth_frame(f0, f1, None, sigma, _to_o(O, ps), trace=True)
    _check_records(rec, tr, "smo 1080p sigma 50")
    g, _ = cases.excuse_threshold_pixels(g, r, tr, "smo 1080p sigma 50", 64)
    cases.assert_close(g, r, "smo 1080p sigma 50")


# ---------------------------------------------------------------- 4. the matcher's plans under long lists

def _plan(psz, ch, sx, st, k, ntagg, have_prev, smoother, tgx, tgy, block):
    """The matcher's choice for a tiled shape (tu_match.hip: nlk_match_plan and the generic launcher, restated):
    ('tile', wavefronts, bytes), ('generic', None, bytes) or ('refused', None, bytes); and the wide queue's bytes
    (FLT1 temporal with sx > st) or None."""
    step = psz // 2
    halo = st if (smoother or have_prev) else sx
    ga = max(ntagg, 1)
    tiles84 = tgx == 8 and tgy == 4 and block
    rounds0 = ((2 * halo + 1) ** 2 + 63) // 64
    threads = 512 if tiles84 and psz >= 8 and (rounds0 <= 2 or (psz == 8 and rounds0 <= 7)) else BM_THREADS
    need = (tgx - 1) * step + 2 * halo + psz
    rwp = need + (2 * halo + 1 - need) % 32
    rh = (tgy - 1) * step + 2 * halo + psz

    def tile(th):
        return 4 * (ch * rwp * rh + 1 + th // 64 * (3 * k + ga))
    lds = tile(threads)
    if lds > LDS_MAX and threads > BM_THREADS and tgy == 4:
        threads = BM_THREADS
        lds = tile(threads)
    wide = None
    if lds <= LDS_MAX:
        if have_prev and not smoother and sx > st:
            needw = 2 * sx + psz
            rwpw = needw + (2 * sx + 1 - needw) % 32
            per_wave = ((ch * rwpw * needw + 1) & ~1) + ((3 * k + ga + 1) & ~1)
            wide = 4 * BM_WAVES * per_wave
            if wide > LDS_MAX:
                wide = None
                lds = LDS_MAX + 1
        if lds <= LDS_MAX:
            return ("tile", threads // 64, lds), wide
    wfull = 2 * max(sx, st) + 1
    gl = 8 * k + 4 * k + 4 * ga + 4 * wfull * wfull + 16
    return ("refused" if gl > LDS_MAX else "generic", None, gl), None


LARGE_GRID = (("NLK_MATCH_BLOCK", "1"), ("NLK_MTX", "8"), ("NLK_MTY", "4"), ("NLK_GTX", "4"))


@pytest.mark.parametrize("k,branch", [(600, ("tile", 8)), (2000, ("tile", 4)), (4000, ("generic", None))],
                         ids=["8-wavefronts", "4-wavefronts", "k_bm_generic"])
def test_matcher_plans_under_long_lists(ctx, built, O, monkeypatch, k, branch):
    """Capacities of 600 / 2000 / 4000 with the temporal radius 5 (121 candidates) on full-size match tiles
    (8 x 4 targets, blocks of 2 x 2 on 8 wavefronts): the per-wavefront list space moves the plan from 8 wavefronts
    to 4 and then to k_bm_generic. FLT1 temporal with sx = st (no wide queue) and the smoother."""
    for kv in LARGE_GRID:
        monkeypatch.setenv(*kv)
    psz, ch, sx, st = 8, 3, 5, 5
    for smo in (False, True):
        (kind, waves, lds), _ = _plan(psz, ch, sx, st, k, k, True, smo, 8, 4, True)
        assert (kind, waves) == branch, (k, smo, kind, waves, lds)
    w, h, sigma = 84, 60, 20.0
    n0, n1 = _frames(w, h, ch, sigma, k)
    over = dict(npatches_x=k, npatches_t=k, npatches_tagg=k, search_sz_x=sx, search_sz_t=st)
    p1 = built.default_params(sigma, built.FLT1, **over)
    ps = built.default_params(sigma, built.SMO1, **over)
    r0 = O.filter_frame(n0, None, None, sigma, _to_o(O, p1))
    prev = _holed(r0)
    _, t1 = _compare(ctx, O, False, n1, prev, None, sigma, p1, f"k {k}: flt1 temporal")
    _compare(ctx, O, True, r0, prev, None, sigma, ps, f"k {k}: smo1")
    assert t1["nsel"].max() == 121


def test_wide_queue_with_long_lists(ctx, built, O):
    """FLT1 temporal with the default sx = 10 > st = 5 and NaN holes: the targets without a valid previous patch
    are queued for k_bm_wide, with lists of 300 from its 441-candidate window."""
    psz, ch, n = 8, 3, 300
    w, h, sigma = 90, 72, 20.0
    (kind, _, _), wide = _plan(psz, ch, 10, 5, n, n, True, False, 4, 2, False)
    assert kind == "tile" and wide is not None and wide <= LDS_MAX
    n0, n1 = _frames(w, h, ch, sigma, 300)
    p1 = built.default_params(sigma, built.FLT1, npatches_x=n, npatches_t=n, npatches_tagg=n)
    assert (p1.search_sz_x, p1.search_sz_t) == (10, 5)
    r0 = O.filter_frame(n0, None, None, sigma, _to_o(O, p1))
    prev = _holed(r0)
    prev[h // 2:h // 2 + 20, 5:30] = np.nan
    _, t1 = _compare(ctx, O, False, n1, prev, None, sigma, p1, "wide queue n 300")
    spatial = t1["active"].astype(bool) & (t1["np0"] == 0)
    assert spatial.sum() > 10 and t1["nsel"][spatial].max() == n


def test_generic_matcher_refuses_above_its_lds(ctx, built, O):
    """Capacities whose lists do not fit k_bm_generic's LDS: an NlkError that names it, with the byte count of the
    formula (tu_match.hip: launch_match_generic)."""
    psz, ch, sx, st, n = 8, 3, 10, 5, 11000
    w, h, sigma = 24, 24, 20.0
    (kind, _, lds), _ = _plan(psz, ch, sx, st, n, n, False, False, 4, 2, False)
    assert kind == "refused"
    cur = _frames(w, h, ch, sigma, 1)[0]
    p = built.default_params(sigma, built.FLT1, npatches_x=n, npatches_t=n, npatches_tagg=n)
    d_cur, d_out = ctx.upload(cur), ctx.alloc(cur.nbytes)
    try:
        with pytest.raises(built.NlkError, match="LDS") as e:
            ctx.filter_frame(d_out, d_cur, None, None, w, h, ch, sigma, p)
    finally:
        ctx.free(d_cur)
        ctx.free(d_out)
    assert f"needs {lds} bytes of LDS" in str(e.value)
    # (the context stays usable)
    p = built.default_params(sigma, built.FLT1)
    g, _ = _dev_frame(ctx, False, cur, None, None, sigma, p)
    cases.assert_close(g, O.filter_frame(cur, None, None, sigma, _to_o(O, p)), "after the refusal")


# ---------------------------------------------------------------- 5. command line

@pytest.mark.parametrize("extra", [[], ["--s1_p", "7"]], ids=["defaults", "patch7"])
def test_smoother_tool_sigma50(built, O, tmp_path, extra):
    """bin/nlkalman-smo -s 50 (lists of 135) on PFM frames against O.smooth_frame."""
    from test_cli import rpfm, run, wpfm
    if not os.path.exists(os.path.join(BIN, "nlkalman-smo")):
        built.build()
    sigma = 50.0
    f0, f1 = _frames(72, 56, 3, sigma, 5)
    wpfm(tmp_path / "f0.pfm", f0)
    wpfm(tmp_path / "f1.pfm", f1)
    r = run("nlkalman-smo", "--flt1", tmp_path / "f0.pfm", "--smo0", tmp_path / "f1.pfm",
            "--smo1", tmp_path / "s.pfm", "-s", "50", *extra)
    assert r.returncode == 0, r.stderr
    got = rpfm(tmp_path / "s.pfm")
    ps = O.default_params(sigma, O.SMO1, **({"patch_sz": 7} if extra else {}))
    assert ps.npatches_t == 135
    s, tr = O.smooth_frame(O.rgb2opp(f0), O.rgb2opp(f1), None, sigma, ps, trace=True)
    ref = O.opp2rgb(s)
    got, _ = cases.excuse_threshold_pixels(got, ref, tr, "nlkalman-smo -s 50", 16)
    cases.assert_close(got, ref, f"nlkalman-smo -s 50 {' '.join(extra)}")


# ---------------------------------------------------------------- 6. deterministic mode

@pytest.mark.parametrize("psz,over,cause", [
    (8, dict(npatches_t=129, npatches_tagg=129), "more than 128 entries"),
    (7, dict(npatches_t=129, npatches_tagg=129), "more than 128 entries"),
    (20, dict(), "above 16 x 16")])
def test_deterministic_mode_refuses_long_lists_and_large_patches(built, psz, over, cause):
    """Deterministic aggregation exists for the tuned kernels only: a call that needs k_group_lds stops
    with NLK_EUNSUP and a message that names the cause (long lists, or patches above 16), not the patch size."""
    sigma = 20.0
    f0, f1 = _frames(64, 56, 3, sigma, psz)
    ps = built.default_params(sigma, built.SMO1, patch_sz=psz, **over)
    det = built.Context(0)
    det.set_deterministic(True)
    try:
        with pytest.raises(built.NlkError) as e:
            _dev_frame(det, True, f0, f1, None, sigma, ps)
        msg = str(e.value)
        assert "deterministic" in msg and cause in msg and "patch size 7" not in msg, msg
        if psz != 20:
            assert "k = 129, group size = 129" in msg, msg
    finally:
        det.close()
