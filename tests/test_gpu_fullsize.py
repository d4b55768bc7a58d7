"""Full-size parity of the paths that round 2 checked at small sizes only (missing 3):
the spatial first-frame call (441-candidate windows in seven-round 4 x 2 blocks, reach-3 mask replay
over 269 grid rows), the second iteration of a first frame, 12 x 12 patches with a reach-2 replay,
and the deterministic aggregation mode against the serial oracle at 1080p.

Reference: src/nlkalman.c:597-600 (mask skip), :630-639 (spatial window), :930-931 (marking).
Tolerances as in test_gpu_parity.py: integer records exact, pixels max-abs 2e-3 / RMSE 2e-4 on the
0..255 scale. The only excused samples are pixels whose summed weight lies within 1e-4 relative of
the reference's absolute `aggr > 1e-6` threshold (src/nlkalman.c:939-942), where the order of a
float sum decides the side; they are counted and bounded (cases.excuse_threshold_pixels). Two runs of the
product against each other excuse exactly the pixels that flipped at that threshold, recognised by their
signature (cases.excuse_flips). No other flip allowance anywhere in this file."""
import numpy as np
import pytest

import cases
from test_gpu_parity import _check_records, _dev_frame, _to_o

pytestmark = pytest.mark.gpu


_excuse_threshold_pixels = cases.excuse_threshold_pixels


def _same(a, b, cur, what, most=64):
    """Two product runs on the same inputs: equal up to the order of the accumulator's adds; the only samples
    excused are threshold flips, recognised by their signature (cases.excuse_flips)."""
    a, _ = cases.excuse_flips(a, b, cur, what, most)
    cases.assert_close(a, b, what)


def test_spatial_first_frame_full_size_1080p(ctx, built, O, synth):
    """FLT1 spatial (deno0 = NULL) at 1920x1080 RGB sigma 20: every target searches the 21 x 21
    window (k = 50, groups of 20 reach 3 grid cells), then FLT2 spatial on the oracle's basic
    estimate (the first stage pair of BASELINE.json configs[4]). Serial oracle."""
    w, h, ch, sigma = 1920, 1080, 3, 20.0
    n0, _, c0 = synth.noisy_pair(w, h, ch, sigma, 1)
    o0 = built.rgb2opp(n0)
    p1, p2 = built.default_params(sigma, built.FLT1), built.default_params(sigma, built.FLT2)
    r, tr = O.filter_frame(o0, None, None, sigma, _to_o(O, p1), trace=True)
    g, rec = _dev_frame(ctx, False, o0, None, None, sigma, p1)
    assert 0.2 < 1 - tr["active"].mean() < 0.6          # the skip is exercised over the whole grid
    _check_records(rec, tr, "flt1 spatial 1080p")
    g, _ = _excuse_threshold_pixels(g, r, tr, "flt1 spatial 1080p", 64)
    cases.assert_close(g, r, "flt1 spatial 1080p")
    r2, tr2 = O.filter_frame(o0, None, r, sigma, _to_o(O, p2), trace=True)
    g2, rec2 = _dev_frame(ctx, False, o0, None, r, sigma, p2)
    _check_records(rec2, tr2, "flt2 spatial 1080p")
    g2, _ = _excuse_threshold_pixels(g2, r2, tr2, "flt2 spatial 1080p", 64)
    cases.assert_close(g2, r2, "flt2 spatial 1080p")
    clean = synth.clean_frame(w, h, ch, 0)
    assert abs(synth.psnr(built.opp2rgb(g2), clean) - synth.psnr(O.opp2rgb(r2), clean)) <= 0.02


def test_spatial_patch12_reach2_720p(ctx, built, O, synth):
    """FLT1 spatial with 12 x 12 patches (step 6, radius 10: a group reaches 2 grid cells, the
    second-order replay) at 1280x720 RGB sigma 40, serial oracle: `k_bm_topk<12,3,7>` blocks,
    `k_mask_commit_wave<2>`, `k_groupp<12>` with the wide halo."""
    w, h, ch, sigma = 1280, 720, 3, 40.0
    n0, _, _ = synth.noisy_pair(w, h, ch, sigma, 5)
    o0 = built.rgb2opp(n0)
    p = built.default_params(sigma, built.FLT1, patch_sz=12)
    r, tr = O.filter_frame(o0, None, None, sigma, _to_o(O, p), trace=True)
    g, rec = _dev_frame(ctx, False, o0, None, None, sigma, p)
    assert 0.02 < 1 - tr["active"].mean() < 0.6
    _check_records(rec, tr, "psz 12 spatial 720p")
    g, _ = _excuse_threshold_pixels(g, r, tr, "psz 12 spatial 720p", 64)
    cases.assert_close(g, r, "psz 12 spatial 720p")


def test_deterministic_mode_against_serial_oracle_1080p(built, O, synth):
    """nlk_ctx_set_deterministic at BASELINE.json configs[1]: FLT1 temporal at 1080p against the
    serial oracle with NO flip allowance beyond the threshold pixels (fixed summation order), and
    a second run bit-identical."""
    w, h, ch, sigma = 1920, 1080, 3, 20.0
    n0, n1, _ = synth.noisy_pair(w, h, ch, sigma, 1)
    o0, o1 = built.rgb2opp(n0), built.rgb2opp(n1)
    p = built.default_params(sigma, built.FLT1)
    det = built.Context(0)
    det.set_deterministic(True)
    try:
        prev, _ = _dev_frame(det, False, o0, None, None, sigma, p)
        g, rec = _dev_frame(det, False, o1, prev, None, sigma, p)
        g_again, _ = _dev_frame(det, False, o1, prev, None, sigma, p)
    finally:
        det.close()
    assert np.array_equal(g, g_again)
    r, tr = O.filter_frame(o1, prev, None, sigma, _to_o(O, p), trace=True)
    _check_records(rec, tr, "deterministic 1080p")
    g, n_edge = _excuse_threshold_pixels(g, r, tr, "deterministic 1080p", 64)
    cases.assert_close(g, r, "deterministic 1080p", flips=0)


@pytest.mark.parametrize("tail,single", [("0", "0"), ("7", "3"), ("1", "33"), ("60", "0")])
def test_group_tiles_of_mixed_sizes_1080p(ctx, built, O, synth, monkeypatch, tail, single):
    """`k_group8m` ends a 1080p launch on smaller tiles (3 x 1 targets, then single targets: tu_group8.hip).
    Whatever the split of the grid rows between the three kinds - none, odd counts, clamped counts - every target
    is filtered exactly once: FLT1 temporal and SMO1 equal the default split up to the order of the accumulator's
    adds, and the default equals the serial oracle."""
    w, h, ch, sigma = 1920, 1080, 3, 20.0
    n0, n1, _ = synth.noisy_pair(w, h, ch, sigma, 1)
    o0, o1 = built.rgb2opp(n0), built.rgb2opp(n1)
    p1, ps = built.default_params(sigma, built.FLT1), built.default_params(sigma, built.SMO1)
    d0, _ = _dev_frame(ctx, False, o0, None, None, sigma, p1)
    d1, rec = _dev_frame(ctx, False, o1, d0, None, sigma, p1)
    ds, _ = _dev_frame(ctx, True, d0, d1, None, sigma, ps)
    if tail == "0":   # (once: the default split against the oracle)
        r, tr = O.filter_frame(o1, d0, None, sigma, _to_o(O, p1), trace=True)
        _check_records(rec, tr, "flt1 temporal 1080p")
        g, _ = _excuse_threshold_pixels(d1, r, tr, "flt1 temporal 1080p", 64)
        cases.assert_close(g, r, "flt1 temporal 1080p")
    monkeypatch.setenv("NLK_G8_TAIL", tail)
    monkeypatch.setenv("NLK_G8_SINGLE", single)
    e1, _ = _dev_frame(ctx, False, o1, d0, None, sigma, p1)
    es, _ = _dev_frame(ctx, True, d0, d1, None, sigma, ps)
    e1, _ = cases.excuse_flips(e1, d1, o1, f"tail {tail} single {single}: flt1 temporal", 64)
    es, _ = cases.excuse_flips(es, ds, d0, f"tail {tail} single {single}: smo1", 64)
    cases.assert_close(e1, d1, f"tail {tail} single {single}: flt1 temporal")
    cases.assert_close(es, ds, f"tail {tail} single {single}: smo1")


def test_single_target_tail_on_single_row_tiles_720p(ctx, built, O, synth, monkeypatch):
    """Grids that use tiles of one grid row (2 x 1 targets: 720p, and every first frame) end their launch on single
    targets too. FLT1 spatial + temporal at 1280x720 against the serial oracle, and against the same calls with the
    tail switched off / enlarged."""
    w, h, ch, sigma = 1280, 720, 3, 20.0
    n0, n1, _ = synth.noisy_pair(w, h, ch, sigma, 9)
    o0, o1 = built.rgb2opp(n0), built.rgb2opp(n1)
    p1 = built.default_params(sigma, built.FLT1)
    d0, rec0 = _dev_frame(ctx, False, o0, None, None, sigma, p1)
    d1, rec1 = _dev_frame(ctx, False, o1, d0, None, sigma, p1)
    r0, tr0 = O.filter_frame(o0, None, None, sigma, _to_o(O, p1), trace=True)
    _check_records(rec0, tr0, "720p spatial")
    g0, _ = _excuse_threshold_pixels(d0, r0, tr0, "720p spatial", 64)
    cases.assert_close(g0, r0, "720p spatial")
    r1, tr1 = O.filter_frame(o1, d0, None, sigma, _to_o(O, p1), trace=True)
    _check_records(rec1, tr1, "720p temporal")
    g1, _ = _excuse_threshold_pixels(d1, r1, tr1, "720p temporal", 64)
    cases.assert_close(g1, r1, "720p temporal")
    for single in ("0", "5", "40"):
        monkeypatch.setenv("NLK_G8_SINGLE", single)
        e0, _ = _dev_frame(ctx, False, o0, None, None, sigma, p1)
        e1, _ = _dev_frame(ctx, False, o1, d0, None, sigma, p1)
        e0, _ = cases.excuse_flips(e0, d0, o0, f"single {single}: spatial", 64)
        e1, _ = cases.excuse_flips(e1, d1, o1, f"single {single}: temporal", 64)
        cases.assert_close(e0, d0, f"single {single}: spatial")
        cases.assert_close(e1, d1, f"single {single}: temporal")


def test_4k_patch8_temporal_against_serial_oracle(ctx, built, O, synth):
    """3840x2160 RGB sigma 20 with the default 8x8 patches, FLT1 temporal, serial oracle: the patch grid of
    959 x 539 targets (4x the 1080p one) through the 8-wavefront match tiles, the row replay of the mask and
    `k_group8m` with its three kinds of tiles (3x2, the last 8 grid rows 3x1, the last 3 one target each).
    Records exact, pixels within the tolerances of the 1080p tests."""
    w, h, ch, sigma = 3840, 2160, 3, 20.0
    n0, n1, c1 = synth.noisy_pair(w, h, ch, sigma, 3)
    o0, o1 = built.rgb2opp(n0), built.rgb2opp(n1)
    p = built.default_params(sigma, built.FLT1)
    prev, _ = _dev_frame(ctx, False, o0, None, None, sigma, p)
    g, rec = _dev_frame(ctx, False, o1, prev, None, sigma, p)
    r, tr = O.filter_frame(o1, prev, None, sigma, _to_o(O, p), trace=True)
    _check_records(rec, tr, "4K psz 8")
    g, _ = _excuse_threshold_pixels(g, r, tr, "4K psz 8", 256)
    cases.assert_close(g, r, "4K psz 8")
    assert abs(synth.psnr(built.opp2rgb(g), c1) - synth.psnr(O.opp2rgb(r), c1)) <= 0.02


def test_host_pointer_calls_pipeline_the_frame_in_row_bands(ctx, built, synth, monkeypatch):
    """The drop-in API (host pointers, libnlkalman.so -> nlk_filter_frame_host) moves a frame over PCIe in
    row bands while the bands before are matched and filtered, and returns finished rows while the last
    bands are filtered. Same decisions as the whole-frame device call, so: equal up to the order of the
    accumulator's atomic adds, for every kind of call of the flt1 -> flt2 -> smo1 chain at 1080p (incl. a
    previous frame with a NaN ring and an occlusion hole: validity map built band by band), and for 2 and
    8 bands."""
    w, h, ch, sigma = 1920, 1080, 3, 20.0
    n0, n1, _ = synth.noisy_pair(w, h, ch, sigma, 1)
    o0, o1 = built.rgb2opp(n0), built.rgb2opp(n1)
    p1, p2, ps = (built.default_params(sigma, m) for m in (built.FLT1, built.FLT2, built.SMO1))
    d0, _ = _dev_frame(ctx, False, o0, None, None, sigma, p1)
    hole = d0.copy()
    hole[:1], hole[-2:], hole[:, :1], hole[:, -2:] = np.nan, np.nan, np.nan, np.nan   # the warp's NaN ring
    hole[500:540, 900:1000] = np.nan
    d1, _ = _dev_frame(ctx, False, o1, hole, None, sigma, p1)
    d2, _ = _dev_frame(ctx, False, o1, hole, d1, sigma, p2)
    ds, _ = _dev_frame(ctx, True, d0, d2, None, sigma, ps)
    for bands in (None, "2", "8"):
        if bands:
            monkeypatch.setenv("NLK_HOST_BANDS", bands)
        tag = f"host bands {bands or 'default'}"
        _same(built.filter_frame(o0, None, None, sigma, p1), d0, o0, f"{tag}: flt1 spatial")
        _same(built.filter_frame(o1, hole, None, sigma, p1), d1, o1, f"{tag}: flt1 temporal")
        if bands is None:
            _same(built.filter_frame(o1, hole, d1, sigma, p2), d2, o1, f"{tag}: flt2")
            _same(built.smooth_frame(d0, d2, None, sigma, ps), ds, d0, f"{tag}: smo1")


def test_host_pointer_calls_form_two_bands_on_the_smallest_frame(ctx, built, synth, monkeypatch, capfd):
    """The row bands of the host-pointer calls at the smallest size that still forms two: 64 x 168 RGB has 41 grid rows,
    and a band needs 4 * (reach + 1) + 8 of them: 20 for the first frame (reach 2), 16 for the temporal one (reach 1).
    The previous frame has the warp's NaN ring and a hole across the seam between the bands (band 0 reads pixel rows up
    to 84 + the search radius, band 1's targets start at row 80). Each call equals the device call up to the order of
    the accumulator's adds, and its trace says that two bands ran: the single-upload path cannot pass."""
    w, h, ch, sigma = 64, 168, 3, 20.0
    n0, n1, _ = synth.noisy_pair(w, h, ch, sigma, 1)
    o0, o1 = built.rgb2opp(n0), built.rgb2opp(n1)
    p1 = built.default_params(sigma, built.FLT1)
    d0, _ = _dev_frame(ctx, False, o0, None, None, sigma, p1)
    hole = d0.copy()
    hole[:1], hole[-2:], hole[:, :1], hole[:, -2:] = np.nan, np.nan, np.nan, np.nan   # the warp's NaN ring
    hole[76:91, 20:44] = np.nan
    d1, _ = _dev_frame(ctx, False, o1, hole, None, sigma, p1)
    monkeypatch.setenv("NLK_HOST_BANDS", "2")
    monkeypatch.setenv("NLK_HOST_TRACE", "1")
    for what, cur, prev, want in (("flt1 spatial", o0, None, d0), ("flt1 temporal", o1, hole, d1)):
        capfd.readouterr()
        got = built.filter_frame(cur, prev, None, sigma, p1)
        assert "2 bands" in capfd.readouterr().err, f"host bands 2, 64 x 168: {what}: not the banded pipeline"
        _same(got, want, cur, f"host bands 2, 64 x 168: {what}")


@pytest.mark.parametrize("seed", [3, 4, 5])
def test_host_pointer_pipeline_on_odd_sizes(ctx, built, synth, seed):
    """Row bands of the host-pointer calls on frames whose sizes are nothing round: one or three channels,
    8 x 8 and 12 x 12 patches (mask reach 1 and 0), a previous frame with NaN holes on band seams, a basic
    estimate. Equal to the device call up to the order of the accumulator's atomic adds."""
    rng = np.random.default_rng(seed)
    w, h = int(rng.integers(500, 900)), int(rng.integers(420, 700))
    ch = int(rng.choice([1, 3]))
    psz = int(rng.choice([8, 12]))
    sigma = float(rng.choice([20.0, 40.0]))
    n0, n1, _ = synth.noisy_pair(w, h, ch, sigma, seed)
    o0, o1 = built.rgb2opp(n0), built.rgb2opp(n1)
    p1 = built.default_params(sigma, built.FLT1, patch_sz=psz)
    p2 = built.default_params(sigma, built.FLT2, patch_sz=psz)
    d0, _ = _dev_frame(ctx, False, o0, None, None, sigma, p1)
    hole = d0.copy()
    for _ in range(12):   # (holes anywhere: some straddle the seams between two bands)
        y, x = int(rng.integers(0, h - 20)), int(rng.integers(0, w - 30))
        hole[y:y + int(rng.integers(1, 20)), x:x + int(rng.integers(1, 30))] = np.nan
    d1, _ = _dev_frame(ctx, False, o1, hole, None, sigma, p1)
    d2, _ = _dev_frame(ctx, False, o1, hole, d1, sigma, p2)
    what = f"host pipeline {w}x{h}x{ch} psz {psz}"
    _same(built.filter_frame(o0, None, None, sigma, p1), d0, o0, what + ": flt1 spatial")
    _same(built.filter_frame(o1, hole, None, sigma, p1), d1, o1, what + ": flt1 temporal")
    _same(built.filter_frame(o1, hole, d1, sigma, p2), d2, o1, what + ": flt2")


def _warped_previous(O, prev, seed):
    """What every real temporal call receives (src/nlkalman.c:29-88): the previous output through
    warp_bicubic - here with zero flow and a blob-shaped occlusion mask - i.e. a NaN ring (1 px left /
    top, 2 px right / bottom) and NaN holes."""
    h, w, _ = prev.shape
    out = O.warp_bicubic(prev, np.zeros((h, w, 2), np.float32), cases.blob_mask(w, h, seed))
    nan = np.isnan(out[..., 0])
    assert nan[0].all() and nan[:, 0].all() and nan[-2:].all() and nan[:, -2:].all()     # the ring
    assert 0.01 < nan[4:-4, 4:-4].mean() < 0.2                                            # the holes
    return out


def test_nan_ring_and_holes_full_size_1080p_against_serial_oracle(ctx, built, O, synth):
    """SURVEY.md §8(d)'s second variant at full size: FLT1 temporal, FLT2 temporal and SMO1
    at 1920x1080 RGB with a previous frame that went through warp_bicubic (NaN ring + occlusion holes): targets
    without a valid previous patch take the spatial branch with the wide window and do not mark the mask
    (src/nlkalman.c:605-609, 637, 931), candidates without one leave the Kalman statistics (:725-732), the
    smoother passes such targets through (:1795-1804). Serial oracle: records exact, pixels 2e-3, threshold
    pixels excused and counted, nothing else."""
    w, h, ch, sigma = 1920, 1080, 3, 20.0
    n0, n1, c1 = synth.noisy_pair(w, h, ch, sigma, 1)
    o0, o1 = built.rgb2opp(n0), built.rgb2opp(n1)
    p1, p2, ps = (built.default_params(sigma, m) for m in (built.FLT1, built.FLT2, built.SMO1))
    f0, _ = _dev_frame(ctx, False, o0, None, None, sigma, p1)
    wp = _warped_previous(O, f0, 11)
    # FLT1 temporal
    r1, tr1 = O.filter_frame(o1, wp, None, sigma, _to_o(O, p1), trace=True)
    g1, rec1 = _dev_frame(ctx, False, o1, wp, None, sigma, p1)
    a = tr1["active"].astype(bool)
    assert (tr1["np0"][a] == 0).mean() > 0.005          # spatial-branch targets inside a temporal frame
    _check_records(rec1, tr1, "flt1 temporal, NaN ring + holes, 1080p")
    g1, n1e = _excuse_threshold_pixels(g1, r1, tr1, "flt1 temporal, NaN ring + holes, 1080p", 64)
    cases.assert_close(g1, r1, "flt1 temporal, NaN ring + holes, 1080p")
    # FLT2 temporal on the oracle's basic estimate
    r2, tr2 = O.filter_frame(o1, wp, r1, sigma, _to_o(O, p2), trace=True)
    g2, rec2 = _dev_frame(ctx, False, o1, wp, r1, sigma, p2)
    _check_records(rec2, tr2, "flt2 temporal, NaN ring + holes, 1080p")
    g2, _ = _excuse_threshold_pixels(g2, r2, tr2, "flt2 temporal, NaN ring + holes, 1080p", 64)
    cases.assert_close(g2, r2, "flt2 temporal, NaN ring + holes, 1080p")
    # SMO1 of frame 0 against frame 1's result warped back (another ring, other holes)
    ws = _warped_previous(O, r2, 12)
    rs, trs = O.smooth_frame(f0, ws, None, sigma, _to_o(O, ps), trace=True)
    gs, recs = _dev_frame(ctx, True, f0, ws, None, sigma, ps)
    a = trs["active"].astype(bool)
    assert (trs["np0"][a] == 0).mean() > 0.005          # pass-through targets
    _check_records(recs, trs, "smo1, NaN ring + holes, 1080p")
    gs, _ = _excuse_threshold_pixels(gs, rs, trs, "smo1, NaN ring + holes, 1080p", 64)
    cases.assert_close(gs, rs, "smo1, NaN ring + holes, 1080p")
    assert abs(synth.psnr(built.opp2rgb(g2), c1) - synth.psnr(O.opp2rgb(r2), c1)) <= 0.02


def test_gray_1080p_against_serial_oracle(ctx, built, O, synth):
    """Single-channel frames at the real size (the reference's own published numbers are on
    *_mono sequences, scripts/dev-scripts/best-results.sh:60-61; rounds 1-4 tested gray at 256 x 256 and below):
    FLT1 temporal and SMO1 at 1920x1080x1, sigma 20, the previous frame through warp_bicubic (NaN ring + holes).
    Serial oracle: records exact, pixels 2e-3, threshold pixels excused and counted."""
    w, h, ch, sigma = 1920, 1080, 1, 20.0
    n0, n1, c1 = synth.noisy_pair(w, h, ch, sigma, 9)
    p1, ps = built.default_params(sigma, built.FLT1), built.default_params(sigma, built.SMO1)
    f0, _ = _dev_frame(ctx, False, n0, None, None, sigma, p1)
    wp = _warped_previous(O, f0, 13)
    r1, tr1 = O.filter_frame(n1, wp, None, sigma, _to_o(O, p1), trace=True)
    g1, rec1 = _dev_frame(ctx, False, n1, wp, None, sigma, p1)
    assert 0.05 < 1 - tr1["active"].mean() < 0.6
    _check_records(rec1, tr1, "gray flt1 temporal 1080p")
    g1, _ = _excuse_threshold_pixels(g1, r1, tr1, "gray flt1 temporal 1080p", 64)
    cases.assert_close(g1, r1, "gray flt1 temporal 1080p")
    ws = _warped_previous(O, r1, 14)
    rs, trs = O.smooth_frame(f0, ws, None, sigma, _to_o(O, ps), trace=True)
    gs, recs = _dev_frame(ctx, True, f0, ws, None, sigma, ps)
    _check_records(recs, trs, "gray smo1 1080p")
    gs, _ = _excuse_threshold_pixels(gs, rs, trs, "gray smo1 1080p", 64)
    cases.assert_close(gs, rs, "gray smo1 1080p")
    assert abs(synth.psnr(g1, c1) - synth.psnr(r1, c1)) <= 0.02
    assert synth.psnr(g1, c1) > synth.psnr(n1, c1) + 8


def test_free_running_chain_1080p_psnr(ctx, built, O, synth):
    """BASELINE.json configs[4] end to end, nobody fed by the other: the product runs
    flt1 -> flt2 on frame 0, warps, flt1 -> flt2 on frame 1, warps back, smo1 of frame 0 - every stage on its
    OWN previous outputs - and so does the serial oracle. What BASELINE.json's "PSNR delta vs ref" is about:
    |dPSNR| <= 0.02 dB against the clean frames on the flt2 and smo1 outputs (and the outputs themselves stay
    within a small RMSE of each other: the chains may differ where a near-tied k-NN rank flipped upstream)."""
    w, h, ch, sigma = 1920, 1080, 3, 20.0
    n0, n1, c1 = synth.noisy_pair(w, h, ch, sigma, 1)
    c0 = synth.clean_frame(w, h, ch, 0)
    flow, occ = cases.flow_and_occ(w, h)

    def chain(B, frame):
        p1, p2, ps = (B.default_params(sigma, m) for m in (0, 1, 2))
        o0, o1 = B.rgb2opp(n0), B.rgb2opp(n1)
        f1_0 = frame(False, o0, None, None, p1)
        f2_0 = frame(False, o0, None, f1_0, p2)
        f1_1 = frame(False, o1, B.warp_bicubic(f1_0, flow, occ), None, p1)
        f2_1 = frame(False, o1, B.warp_bicubic(f2_0, flow, occ), f1_1, p2)
        s1_0 = frame(True, f2_0, B.warp_bicubic(f2_1, -flow, occ), None, ps)
        return B.opp2rgb(f2_1), B.opp2rgb(s1_0)
    g21, gs0 = chain(built, lambda smo, cur, prev, basic, p: _dev_frame(ctx, smo, cur, prev, basic, sigma, p)[0])
    r21, rs0 = chain(O, lambda smo, cur, prev, basic, p: (O.smooth_frame if smo else O.filter_frame)(cur, prev, basic, sigma, p))
    for name, g, r, clean in (("flt2 of frame 1", g21, r21, c1), ("smo1 of frame 0", gs0, rs0, c0)):
        dp = synth.psnr(g, clean) - synth.psnr(r, clean)
        rm = float(np.sqrt(np.mean((g - r) ** 2)))
        print(f"free-running 1080p chain, {name}: dPSNR {dp:+.5f} dB, RMSE vs oracle chain {rm:.2e}")
        assert abs(dp) <= 0.02, f"{name}: dPSNR {dp}"
        assert rm <= 0.05, f"{name}: RMSE {rm}"
        assert synth.psnr(g, clean) > synth.psnr(n1 if clean is c1 else n0, clean) + 8


def test_8k_frame_replay_inside_the_launch_equals_the_separate_kernels(ctx, built, synth, monkeypatch):
    """7680 x 4320 RGB: a patch grid of 1919 x 1079 targets - more grid rows than a workgroup has threads, nearly
    as wide as the row replay's 2048-target limit, 2 M targets. FLT1 spatial (reach 2) and temporal (reach 1): the
    mask replay inside the group kernel's launch (default) and as separate kernels (NLK_NO_CHASE=1) must give the
    same decisions for every target and the same frame up to the order of the float sums; k-NN lists identical."""
    w, h, ch, sigma = 7680, 4320, 3, 20.0
    n0, n1, _ = synth.noisy_pair(w, h, ch, sigma, 8)
    o0, o1 = built.rgb2opp(n0), built.rgb2opp(n1)
    del n0, n1
    p = built.default_params(sigma, built.FLT1)
    out = {}
    for tag, env in (("in", None), ("sep", "1")):
        if env:
            monkeypatch.setenv("NLK_NO_CHASE", env)
        else:
            monkeypatch.delenv("NLK_NO_CHASE", raising=False)
        f0, r0 = _dev_frame(ctx, False, o0, None, None, sigma, p)
        f1, r1 = _dev_frame(ctx, False, o1, f0, None, sigma, p)
        out[tag] = (f0, r0, f1, r1)
    monkeypatch.delenv("NLK_NO_CHASE", raising=False)
    for k in (1, 3):
        a, b = out["in"][k], out["sep"][k]
        assert a["active"].size == 1919 * 1079
        for f in ("active", "nsel", "np0", "nagg", "topk", "gcoords"):
            assert np.array_equal(a[f], b[f]), (k, f)
        assert 0.1 < 1 - a["active"].mean() < 0.6
    _same(out["in"][0], out["sep"][0], o0, "8K first frame, replay inside the launch vs separate kernels", most=256)
    # (the temporal frames were fed their own first frames: compare them through the same previous frame)
    monkeypatch.setenv("NLK_NO_CHASE", "1")
    f1_sep, _ = _dev_frame(ctx, False, o1, out["in"][0], None, sigma, p)
    monkeypatch.delenv("NLK_NO_CHASE", raising=False)
    f1_in, _ = _dev_frame(ctx, False, o1, out["in"][0], None, sigma, p)
    _same(f1_in, f1_sep, o1, "8K temporal frame, replay inside the launch vs separate kernels", most=256)


@pytest.mark.parametrize("seed", [101, 102, 103])
def test_random_parameters_full_size_soak(ctx, built, O, seed):
    """tools/soak_fullsize.py as a test: two random configurations per seed at ~1080p -
    random size, 1 or 3 channels, FLT1 / FLT2 / SMO1, random radius, list lengths and group sizes, a previous
    frame with NaN holes - against the serial oracle: records exact, pixels 2e-3, threshold pixels excused."""
    rng = np.random.default_rng(seed)
    for it in range(2):
        w, h = int(rng.integers(1700, 2300)), int(rng.integers(950, 1300))
        ch = int(rng.choice([1, 3]))
        smoother = rng.random() < 0.3
        mode = built.SMO1 if smoother else int(rng.choice([built.FLT1, built.FLT2]))
        sigma = float(rng.choice([10.0, 20.0, 40.0]))
        over = dict(patch_sz=8, search_sz_t=int(rng.integers(2, 7)), npatches_t=int(rng.integers(2, 64)),
                    npatches_tagg=int(rng.integers(1, 45)), npatches_x=int(rng.integers(2, 64)))
        p = built.default_params(sigma, mode, **over)
        base = np.add.outer(np.linspace(20, 220, h), np.linspace(0, 30, w))[..., None] * np.ones(ch)
        cur = (base + rng.normal(0, sigma, base.shape)).astype(np.float32)
        prev = (base + rng.normal(0, sigma / 3, base.shape)).astype(np.float32)
        for _ in range(6):
            y0, x0 = int(rng.integers(0, h - 40)), int(rng.integers(0, w - 60))
            prev[y0:y0 + int(rng.integers(1, 40)), x0:x0 + int(rng.integers(1, 60))] = np.nan
        basic = (base + rng.normal(0, 3, base.shape)).astype(np.float32) if mode == built.FLT2 else None
        fn = O.smooth_frame if smoother else O.filter_frame
        r, tr = fn(cur, prev, basic, sigma, _to_o(O, p), trace=True)
        g, rec = _dev_frame(ctx, smoother, cur, prev, basic, sigma, p)
        what = f"soak seed {seed} #{it}: {w}x{h}x{ch} mode {mode} {over} sigma {sigma}"
        _check_records(rec, tr, what)
        # (a ramp image with identical patches everywhere puts many pixels on the same summed weight: the bound
        # is a sanity guard - 0.05 % of the frame -, what it excuses is still only |aggr - 1e-6| <= 1e-10)
        g, _ = _excuse_threshold_pixels(g, r, tr, what, 1024)
        cases.assert_close(g, r, what)
