"""One table of operations over the C-ABI of include/nlk_hip.h, for the tests that state a property of EVERY entry
point at once: tests/test_context_history.py (a context's results do not depend on the calls made before) and
tests/test_stream_order.py (every launch, memset and copy of a call goes to the stream the caller set).

An operation (Op) has
  make(rng)        seeded host inputs: a dict with "in" (name -> numpy array that goes to the device), "out" (name ->
                   (shape, dtype) of a device buffer the call fills; a name that is also in "in" is worked in place)
                   and whatever parameters its call needs
  call(ctx, d, I)  the library calls, on device pointers d[name] alone (uploads, downloads and frees are run()'s)
  check(ctx, I, det)  host-only: the path that ran is the path the op is in the table for (nlk_host_match_plan,
                   nlk_frame_grid, nlk_ctx_last_group_shape / _packed), so that a later change of thresholds cannot
                   turn an op into a duplicate of another without notice
  same(a, b, what, I)  the comparison of two results
and the flags
  bitexact   two fresh contexts give the same bits (FOUND by running test_fresh_contexts_agree, not read from code)
  syncs      the call waits for the device on a warm context, with the reason (found by tests/test_stream_order.py's
             assertion, then confirmed in the code)
  det_ok     runs in deterministic mode (nlk_ctx_set_deterministic)
  records    a frame op whose nlk_ctx_read_records are part of its result
  env        NLK_* switches the op runs under (set through monkeypatch.setenv, undone right after the call)

Shapes and parameters are those of the operations' own tests (named beside each op), at the smallest frames at which
the path is still selected: the correctness of a fresh context's result is pinned there, here only its independence.

Comparisons. Ops with bitexact: np.array_equal(equal_nan=True) on every output. Frame ops in the default mode add
their accumulator with float atomics: integer records exact over live entries (check_records), pixels through
cases.excuse_flips(.., 150) and cases.assert_close(maxabs=5e-4, rmse=5e-5), the project's figures for two runs of
the product on the same input (tests/test_gpu_parity.py: test_accumulators_of_filter_and_smoother_interleaved,
test_deterministic_aggregation_is_bit_reproducible)."""
import importlib

import numpy as np
import pytest

import cases

synth = importlib.import_module("bwd-nlkalman_amd.synth")
pkg = importlib.import_module("bwd-nlkalman_amd")

FLT1, FLT2, SMO1 = 0, 1, 2


# ---------------------------------------------------------------- the shared record comparison

def check_records(rec, tr, what):
    """Integer records of a frame call, exact over live entries: `tr` is the oracle's trace or a second GPU record
    dict (Context.read_records). Decisions for every target; nsel, np0, nagg of the active ones; their k-NN lists up
    to nsel and their group members up to nagg (what lies beyond is never read by a kernel)."""
    act_o, act_g = tr["active"].astype(bool), rec["active"].astype(bool)
    assert np.array_equal(act_o, act_g), f"{what}: processed-mask decisions differ"
    a = act_o
    for f in ("nsel", "np0", "nagg"):
        assert np.array_equal(tr[f][a], rec[f][a]), f"{what}: {f} differs"
    k = tr["topk"].shape[1]
    col = np.arange(k)[None, :]
    live = a[:, None] & (col < tr["nsel"][:, None])
    assert np.array_equal(tr["topk"][live], rec["topk"][:, :k].astype(np.int64)[live]), f"{what}: k-NN lists differ"
    g = tr["gcoords"].shape[1]
    col = np.arange(g)[None, :]
    live = a[:, None] & (col < tr["nagg"][:, None])
    assert np.array_equal(tr["gcoords"][live], rec["gcoords"][:, :g].astype(np.int64)[live]), f"{what}: group members differ"


# ---------------------------------------------------------------- comparisons

def same_bits(a, b, what, I=None):
    assert a.keys() == b.keys(), what
    for k in a:
        if k == "records":
            check_records(a[k], b[k], f"{what}: records")
            continue
        x, y = np.asarray(a[k]), np.asarray(b[k])
        assert x.shape == y.shape and x.dtype == y.dtype, f"{what}: {k}: {x.shape} {x.dtype} / {y.shape} {y.dtype}"
        if x.dtype.fields:   # (structured: nlk_curve_bin)
            for f in x.dtype.fields:
                assert np.array_equal(x[f], y[f], equal_nan=x[f].dtype.kind == "f"), f"{what}: {k}.{f} differs"
        else:
            assert np.array_equal(x, y, equal_nan=x.dtype.kind == "f"), f"{what}: output {k} differs in {int((x != y).sum())} places"


def same_frame(a, b, what, I):
    """Frame ops in the default mode (float atomics): records exact, pixels to summation-order noise, with the pixels
    that flip at the aggregation threshold excused, counted and bounded."""
    assert a.keys() == b.keys(), what
    for k in a:
        if k == "records":
            check_records(a[k], b[k], f"{what}: records")
            continue
        x, _ = cases.excuse_flips(a[k], b[k], I["passthrough"][k], f"{what}: {k}", 150)
        cases.assert_close(x, b[k], f"{what}: {k}", maxabs=5e-4, rmse=5e-5)


class Op:
    def __init__(self, name, make, call, check=None, same=same_bits, bitexact=True, syncs=None, det_ok=False,
                 records=False, env=None, source="", shares=None):
        self.shares = shares or name   # (an op that runs another op's inputs another way: NLK_NO_CHASE, NLK_BANDS)
        self.name, self.make, self.call, self.check_, self.same_ = name, make, call, check, same
        self.bitexact, self.syncs, self.det_ok, self.records = bitexact, syncs, det_ok, records
        self.env, self.source = dict(env or {}), source

    def __repr__(self):
        return self.name

    def inputs(self, seed=0):
        """The op's inputs: the same for every seed given the same number (the name enters, so no two ops share noise)."""
        return self.make(np.random.default_rng([seed] + [ord(c) for c in self.shares]))

    def check(self, ctx, I, det=False):
        if self.check_ is not None:
            self.check_(ctx, I, det)

    def same(self, a, b, what, I, det=False):
        (same_bits if (det or self.bitexact) else self.same_)(a, b, what, I)

    def run(self, ctx, I, det=False):
        """Uploads, calls, downloads, frees: a dict of host arrays (+ "records" for frame ops)."""
        d, mine = {}, []
        try:
            for k, a in I["in"].items():
                d[k] = ctx.upload(a)
                mine.append(d[k])
            for k, (shape, dtype) in I["out"].items():
                if k not in d:   # (a poisoned buffer: what a call leaves unwritten shows as 0xFF bytes on both sides)
                    d[k] = ctx.upload(np.full(int(np.prod(shape)) * np.dtype(dtype).itemsize, 0xFF, np.uint8))
                    mine.append(d[k])
            extra = self.call(ctx, d, I) or {}
            self.check(ctx, I, det)
            out = {k: ctx.download(d[k], shape, dtype) for k, (shape, dtype) in I["out"].items()}
            out.update({k: np.asarray(v) for k, v in extra.items()})
            if self.records:
                out["records"] = ctx.read_records()
            return out
        finally:
            ctx.sync()
            for p in mine:
                ctx.free(p)


def with_env(op, monkeypatch, fn):
    """fn() under the op's NLK_* switches: set through monkeypatch.setenv, which makes every live context reload
    them (tests/conftest.py), and undone right after the call."""
    for k, v in op.env.items():
        monkeypatch.setenv(k, v)
    try:
        return fn()
    finally:
        for k in op.env:
            monkeypatch.delenv(k, raising=False)


# ---------------------------------------------------------------- contexts and the fresh-context results

FRESH = {}   # (op name, deterministic, seed) -> (inputs, the result on a fresh context): computed once, never changed


def context(built, det=False):
    """A context of the caller's own (to be closed by it)."""
    if built.hip().nlk_device_count() < 1:
        pytest.fail("GPU test selected but no HIP device is visible (no CPU fallback exists)")
    c = built.Context(0)
    if det:
        c.set_deterministic(True)
    return c


def fresh(built, monkeypatch, op, det=False, seed=0):
    """(inputs, result) of the op on a context that has run nothing else. seed: which of the op's inputs (same
    shapes and parameters, other values) - a sequence that runs an op twice runs it on different values, so that
    what the first run left in the context is not the second run's answer."""
    key = (op.name, det, seed)
    if key not in FRESH:
        c = context(built, det)
        try:
            I = op.inputs(seed)
            FRESH[key] = (I, with_env(op, monkeypatch, lambda: op.run(c, I, det)))
        finally:
            c.close()
    return FRESH[key]


# ---------------------------------------------------------------- inputs

def rgb2opp(im):
    """Opponent colours for three channels (the package's own helper, as the rest of the suite prepares its inputs)."""
    return pkg.rgb2opp(im) if im.shape[2] == 3 else im


def holed(im):
    """A previous frame with a NaN rectangle and NaN first columns (tests/test_gpu_parity.py:
    test_mask_replay_inside_the_group_launch_equals_the_separate_kernels): spatial-branch targets inside a temporal
    call, i.e. 32-bit lists among the packed ones and the wide-window queue."""
    h, w = im.shape[:2]
    p = im.copy()
    p[h // 4:h // 3, w // 3:w // 2] = np.nan
    p[:, :2] = np.nan
    return p


def frame_inputs(rng, w, h, ch, sigma=20.0):
    """cur = noisy frame 1, prev = a stand-in for the filtered frame 0 (clean frame 0 + a fifth of the noise), basic =
    the same for frame 1; in opponent colours where ch = 3. (synth.noisy_pair's frames; the ramp of
    tests/test_long_lists.py for channel counts it has no colours for.)"""
    seed = int(rng.integers(1, 1 << 30))
    _, n1, c1 = synth.noisy_pair(w, h, ch, sigma, seed)
    c0 = synth.clean_frame(w, h, ch, 0)
    f0, f1 = synth.awgn(c0, sigma / 5, seed + 7), synth.awgn(c1, sigma / 5, seed + 8)
    return rgb2opp(n1), rgb2opp(f0), rgb2opp(f1)


def texture_pair(rng, w, h):
    """Two smooth textured single-channel frames related by a sub-pixel translation (tests/test_tvl1.py: _pair)."""
    y, x = np.mgrid[0:h, 0:w].astype(np.float32)

    def tex(xx, yy):
        return (96 + 60 * np.sin(0.21 * xx + 0.1 * yy) * np.cos(0.17 * yy - 0.05 * xx)
                + 40 * np.sin(0.045 * xx * yy / 8 + 1.0)).astype(np.float32)
    i0 = tex(x, y) + rng.normal(0, 2, (h, w)).astype(np.float32)
    i1 = tex(x + 1.7, y - 0.8) + rng.normal(0, 2, (h, w)).astype(np.float32)
    return np.ascontiguousarray(i0), np.ascontiguousarray(i1)


def image(rng, w, h, ch, sigma=8.0):
    return (synth.clean_frame(w, h, ch) + rng.normal(0, sigma, (h, w, ch))).astype(np.float32)


F32 = np.float32


# ---------------------------------------------------------------- frame ops

def frame_op(name, w, h, ch, mode=FLT1, temporal=False, basic=False, over=None, env=None, expect=None, records=True,
             det_ok=True, source="", sigma=20.0, shares=None):
    """A whole-frame call (nlk_dev_filter_frame / nlk_dev_smooth_frame). expect: generic, wide (nlk_host_match_plan),
    reach (nlk_frame_grid), family, chase, packed (nlk_ctx_last_group_shape: family is "k_group8m" or None = another
    launcher, which is all that report tells apart; chase and packed in the default mode only: deterministic mode
    replays the mask in its own kernels)."""
    over, expect, smo = dict(over or {}), dict(expect or {}), mode == SMO1

    def make(rng):
        cur, f0, f1 = frame_inputs(rng, w, h, ch, sigma)
        p = pkg.default_params(sigma, mode, **over)
        I = dict(w=w, h=h, ch=ch, sigma=sigma, p=p, smo=smo, out={"out": (cur.shape, F32)})
        if smo:      # (the smoother: frame 0's filtered frame against frame 1's, tests/test_gpu_parity.py:645)
            I["in"] = {"cur": f0, "prev": holed(f1)}
        else:
            I["in"] = {"cur": cur}
            if temporal:
                I["in"]["prev"] = holed(f0)
            if basic:
                I["in"]["basic"] = f1
        I["passthrough"] = {"out": I["in"]["cur"]}
        return I

    def call(ctx, d, I):
        fn = ctx.smooth_frame if I["smo"] else ctx.filter_frame
        fn(d["out"], d["cur"], d.get("prev"), d.get("basic"), I["w"], I["h"], I["ch"], I["sigma"], I["p"])

    def check(ctx, I, det):
        have_prev = "prev" in I["in"]
        if "reach" in expect:
            assert pkg.frame_grid(w, h, I["p"], smo, have_prev).reach == expect["reach"], name
        if "ngy" in expect:
            assert pkg.frame_grid(w, h, I["p"], smo, have_prev).ngy == expect["ngy"], name
        if "generic" in expect or "wide" in expect:
            mp = pkg.host_match_plan(w, h, ch, I["p"], smo, have_prev)
            for k in ("generic", "wide"):
                assert k not in expect or mp[k] == expect[k], (name, k, mp)
        ran = ctx.last_group_shape()
        if "family" in expect:
            assert ran["family"] == expect["family"], (name, ran)
        if not det:
            if "chase" in expect:
                assert (ran["chase"] > 0) == expect["chase"], (name, ran)
            if "packed" in expect:
                assert ran["packed_lists"] == expect["packed"], (name, ran)

    return Op(name, make, call, check, same=same_frame, bitexact=False, syncs=None, det_ok=det_ok and not env,
              records=records, env=env, source=source, shares=shares)


def _long(n, psz):
    """tests/test_long_lists.py: _long - list length n on every route, windows that hold more than n candidates."""
    r = 6
    while (2 * r + 1) ** 2 <= n:
        r += 1
    return dict(patch_sz=psz, npatches_x=n, npatches_t=n, npatches_tagg=n, search_sz_x=r + 1, search_sz_t=r)


G8 = "k_group8m"
FRAME_OPS = [
    frame_op("flt1-spatial-p8c3-120x88", 120, 88, 3, expect=dict(generic=0, reach=2, family=G8, chase=True),
             source="test_gpu_parity.py: test_integer_records_exact (x)"),
    frame_op("flt1-spatial-p8c3-200x172", 200, 172, 3, expect=dict(generic=0, reach=2, family=G8, chase=True),
             source="the same, a larger frame"),
    # NLK_BANDS=2: two bands on stream and aux_stream (clamp_bands wants ngy / 2 >= 4 (R + 1) + 8 = 20 at reach 2:
    # 42 grid rows here, which check() holds through nlk_frame_grid). What pins the banded path is indirect: bands
    # replay the mask in their own kernels, so the last group launch reports no replay inside it, where the same
    # frame in one band (the op above) reports one.
    frame_op("flt1-spatial-p8c3-200x172-bands2", 200, 172, 3, env={"NLK_BANDS": "2"},
             expect=dict(generic=0, reach=2, ngy=42, family=G8, chase=False), shares="flt1-spatial-p8c3-200x172",
             source="test_gpu_parity.py: test_banded_two_stream_pipeline_equals_single_stream"),
    frame_op("flt1-temporal-p8c3-120x88", 120, 88, 3, temporal=True,
             expect=dict(generic=0, wide=1, reach=1, family=G8, chase=True, packed=True),
             source="test_gpu_parity.py: test_mask_replay_inside_the_group_launch_equals_the_separate_kernels"),
    frame_op("flt1-temporal-p8c3-120x88-nochase", 120, 88, 3, temporal=True, env={"NLK_NO_CHASE": "1"},
             expect=dict(generic=0, wide=1, reach=1, family=G8, chase=False), shares="flt1-temporal-p8c3-120x88",
             source="the same: the replay in its own kernels"),
    # search_sz_t = 8: reach 2, and a radius the packed lists have no byte code for (nlk_packed_geom)
    frame_op("flt1-temporal-p8c1-120x88-st8", 120, 88, 1, temporal=True, over=dict(search_sz_t=8),
             expect=dict(generic=0, reach=2, family=G8, chase=True, packed=False),
             source="test_packed_lists.py (radii above the packed range)"),
    frame_op("flt1-temporal-p8c1-120x88", 120, 88, 1, temporal=True,
             expect=dict(generic=0, wide=1, reach=1, family=G8, chase=True, packed=True),
             source="the same, ch 1"),
    frame_op("flt2-temporal-p8c3-120x88", 120, 88, 3, mode=FLT2, temporal=True, basic=True,
             expect=dict(generic=0, family=G8), source="the same, second iteration"),
    frame_op("smo1-p8c3-120x88", 120, 88, 3, mode=SMO1, expect=dict(generic=0, family=G8, packed=False),
             source="the same, smoother (fourth plane prev - cur)"),
    frame_op("flt1-temporal-p6c1-61x53", 61, 53, 1, temporal=True, over=dict(patch_sz=6, search_sz_x=9),
             expect=dict(generic=0, family=None), source="test_gpu_parity.py: test_deterministic_aggregation_is_bit_reproducible (psz 6)"),
    frame_op("flt1-temporal-p12c3-84x60", 84, 60, 3, temporal=True, over=dict(patch_sz=12, search_sz_x=10),
             expect=dict(generic=0, family=None), source="the same (psz 12); cases.CASES rgb84x60_p12_s40"),
    frame_op("flt1-temporal-p16c1-50x40", 50, 40, 1, temporal=True, over=dict(patch_sz=16, search_sz_x=10),
             expect=dict(generic=0, family=None), source="test_gpu_parity.py: test_edge_cases (psz 16, 50x40)"),
    frame_op("flt1-temporal-p20c3-90x70", 90, 70, 3, temporal=True, over=dict(patch_sz=20),
             expect=dict(generic=1, family=None), det_ok=False,   # (deterministic mode: the tuned kernels only)
             source="test_gpu_parity.py: test_large_patches_and_other_channel_counts"),
    frame_op("flt1-temporal-p8c2-60x50", 60, 50, 2, temporal=True, expect=dict(generic=1, family=None),
             source="the same (8, 2, (60, 50))"),
    # (lists of 129 entries go to the LDS-DCT kernel, tu_frame.hip: launch_group; the report of the last group launch
    # only says "not k_group8m", and that is all that is asserted here)
    frame_op("flt1-temporal-p8c3-72x56-n129", 72, 56, 3, temporal=True, over=_long(129, 8),
             expect=dict(family=None), det_ok=False, source="test_long_lists.py: test_list_length_boundary p8c3-n129"),
    frame_op("flt1-spatial-p4c3-40x40-reach5", 40, 40, 3, over=dict(patch_sz=4, search_sz_x=10),
             expect=dict(reach=5, family=None), source="test_gpu_parity.py: test_unsupported_parameters_fail_loudly (reach)"),
    frame_op("flt1-temporal-p8c3-64x48", 64, 48, 3, temporal=True, expect=dict(generic=0, reach=1, family=G8, chase=True),
             source="a small grid after a large one"),
    frame_op("flt1-temporal-p8c3-33x47", 33, 47, 3, temporal=True, expect=dict(generic=0, reach=1, family=G8, chase=True),
             source="test_gpu_parity.py: test_edge_cases (8, (33, 47, 3))"),
]


def _tiny():
    """An image smaller than a patch: the copy path of run_frame (no target, no records)."""
    def make(rng):
        im = rng.uniform(0, 255, (7, 20, 1)).astype(F32)
        prev = rng.uniform(0, 255, (7, 20, 1)).astype(F32)
        return {"in": {"cur": im, "prev": prev}, "out": {"out": (im.shape, F32)}, "p": pkg.default_params(20.0, FLT1)}

    def call(ctx, d, I):
        ctx.filter_frame(d["out"], d["cur"], d["prev"], None, 20, 7, 1, 20.0, I["p"])

    def check(ctx, I, det):
        try:
            pkg.frame_grid(20, 7, I["p"], False, True)
        except ValueError:
            return
        raise AssertionError("20x7 holds a patch of 8?")
    return Op("flt1-20x7-smaller-than-a-patch", make, call, check, det_ok=True,
              source="test_gpu_parity.py: test_image_smaller_than_a_patch_is_returned_unchanged")


def _split_api():
    """nlk_dev_frame_accumulate twice into two accumulators (filter, then smoother), then both normalisations."""
    w, h, ch, sigma = 120, 88, 3, 20.0

    def make(rng):
        cur, f0, f1 = frame_inputs(rng, w, h, ch, sigma)
        z = np.zeros((ch + 1, h, w), F32)
        return {"in": {"cur": cur, "f0": f0, "f1": holed(f1), "acc_f": z, "acc_s": z.copy()},
                "out": {"out_f": (cur.shape, F32), "out_s": (cur.shape, F32)},
                "passthrough": {"out_f": cur, "out_s": f0},
                "p1": pkg.default_params(sigma, FLT1), "ps": pkg.default_params(sigma, SMO1)}

    def call(ctx, d, I):
        ngy = (h - 8) // 4 + 1
        ctx.frame_accumulate(d["acc_f"], d["cur"], d["f0"], None, w, h, ch, sigma, I["p1"], 0, ngy)
        ctx.frame_accumulate(d["acc_s"], d["f0"], d["f1"], None, w, h, ch, sigma, I["ps"], 0, ngy, smoother=True)
        ctx.frame_normalize(d["out_f"], d["acc_f"], d["cur"], w, h, ch, 0, h)
        ctx.frame_normalize(d["out_s"], d["acc_s"], d["f0"], w, h, ch, 0, h)
    return Op("split-accumulate-filter-smoother-normalize", make, call, same=same_frame, bitexact=False, det_ok=True,
              source="test_gpu_parity.py: test_accumulators_of_filter_and_smoother_interleaved")


def _strip(part):
    """The three-phase strip form on the lower half of a 120x88 frame. part False: nlk_dev_strip_match of the strip
    into caller-owned mark words, nlk_dev_strip_commit_group with gy0 > 0, nlk_dev_frame_normalize of its rows. part
    True: the strip matched in two nlk_dev_strip_match_part calls (the first lays the whole strip out, the second
    nothing) with nlk_ctx_set_strip_accumulator clearing the accumulator, then nlk_dev_mask_commit +
    nlk_dev_strip_group. The mark words of the rows above the strip are the caller's: zero (no target marked). The
    accumulator is an input only (part True: full of 3.0 until the layout clears it); what is compared is the strip
    normalised from it, which shows an accumulator that was not cleared or not filled."""
    w, h, ch, sigma = 120, 88, 3, 20.0
    ngx, ngy, gy0 = (w - 8) // 4 + 1, (h - 8) // 4 + 1, 10
    Y0 = gy0 * 4 - 12           # (the strip's pixel rows: its targets' patches and a halo of 12 rows above)
    hl, ngy_l = h - Y0, ngy - gy0

    def make(rng):
        cur, f0, _ = frame_inputs(rng, w, h, ch, sigma)
        cur_s, prev_s = np.ascontiguousarray(cur[Y0:]), np.ascontiguousarray(holed(f0)[Y0:])
        acc = np.zeros((ch + 1, hl, w), F32) if not part else np.full((ch + 1, hl, w), 3.0, F32)
        return {"in": {"cur": cur_s, "prev": prev_s, "marks": np.zeros(ngx * ngy, np.uint64), "acc": acc,
                       "active": np.full(ngx * ngy, 7, np.uint8)},
                "out": {"out": (cur_s.shape, F32)},
                "passthrough": {"out": cur_s}, "p": pkg.default_params(sigma, FLT1)}

    def call(ctx, d, I):
        oy, p = gy0 * 4 - Y0, I["p"]
        d_marks = d["marks"] + 8 * gy0 * ngx
        if not part:
            reach = ctx.strip_match(d_marks, d["cur"], d["prev"], None, w, hl, ch, sigma, p, oy, ngy_l)
            ctx.strip_commit_group(d["acc"], d["marks"], ngx, ngy, reach, gy0, d["active"])
        else:
            ctx._chk(ctx.L.nlk_ctx_set_strip_accumulator(ctx.h, d["acc"]))
            try:
                half = ngy_l // 2
                ctx.strip_match_part(d_marks, d["cur"], d["prev"], None, w, hl, ch, sigma, p, oy, ngy_l, 0, half,
                                     (0, hl, 0, hl))
                reach = ctx.strip_match_part(d_marks, d["cur"], d["prev"], None, w, hl, ch, sigma, p, oy, ngy_l, half,
                                             ngy_l - half, (hl, hl, hl, hl))
            finally:   # (the context must not keep a pointer to a buffer the caller is about to free)
                ctx._chk(ctx.L.nlk_ctx_set_strip_accumulator(ctx.h, None))
            ctx.mask_commit(d["marks"], ngx, ngy, reach, d["active"])
            ctx.strip_group(d["acc"], d["active"] + gy0 * ngx)
        ctx.frame_normalize(d["out"], d["acc"], d["cur"], w, hl, ch, 0, hl)

    def check(ctx, I, det):
        ran = ctx.last_group_shape()
        assert ran["family"] == G8, ran
        if not det:
            assert (ran["chase"] > 0) == (not part), ran

    return Op("strip-match-part-x2-commit-group" if part else "strip-match-commit-group-gy0", make, call, check,
              same=same_frame, bitexact=False, source="test_gpu_parity.py: test_gpu_exact_strips_equal_whole_frame")


# ---------------------------------------------------------------- everything else

def _tvl1(w, h):
    def make(rng):
        i0, i1 = texture_pair(rng, w, h)
        i0 = i0 + rng.normal(0, 6, i0.shape).astype(F32)   # (noise: tens of iterations per warp, test_tvl1.py:188)
        i1 = i1 + rng.normal(0, 6, i1.shape).astype(F32)
        return {"in": {"i0": i0, "i1": i1}, "out": {"flow": ((h, w, 2), F32)}, "p": pkg.tvl1_params(w, h, lam=0.3)}

    def call(ctx, d, I):
        return {"iterations": ctx.tvl1_flow(d["flow"], d["i0"], d["i1"], w, h, I["p"])}
    return Op(f"tvl1-{w}x{h}", make, call, syncs="reads the solver state back between batches and at the end (tu_tvl1.hip)",
              source="test_tvl1.py: test_gpu_flow_every_driver_variant_is_exact / test_gpu_small and odd sizes")


def _bm_flow():
    w, h = 131, 97

    def make(rng):
        i0, i1 = texture_pair(rng, w, h)
        return {"in": {"i0": i0, "i1": i1}, "out": {"flow": ((h, w, 2), F32)}}

    def call(ctx, d, I):
        ctx.bm_flow(d["flow"], d["i0"], d["i1"], w, h)
    return Op("bm-flow-131x97", make, call, source="test_bmflow.py")


def _flow_invert():
    w, h = 67, 41

    def make(rng):
        flow = rng.normal(0, 2.5, (h, w, 2)).astype(F32)
        return {"in": {"flow": flow}, "out": {"inv": ((h, w, 2), F32)}}

    def call(ctx, d, I):
        ctx.flow_invert(d["inv"], d["flow"], w, h, 4)
    return Op("flow-invert-67x41", make, call, source="test_flow_invert.py")


def _gray_occlusion():
    w, h = 83, 57

    def make(rng):
        return {"in": {"im": image(rng, w, h, 3), "flow": rng.normal(0, 1.0, (h, w, 2)).astype(F32)},
                "out": {"gray": ((h, w), F32), "mask": ((h, w), F32)}}

    def call(ctx, d, I):
        ctx.gray(d["gray"], d["im"], w, h, 3)
        ctx.occlusion_mask(d["mask"], d["flow"], w, h, 0.75)
    return Op("gray-occlusion-83x57", make, call, source="test_tvl1.py (gray, occlusion mask)")


def _warp(ch):
    w, h = 83, 57

    def make(rng):
        im = rng.uniform(0, 255, (h, w, ch)).astype(F32)
        im[10:12, 20:23] = np.nan
        flow = rng.normal(0, 3, (h, w, 2)).astype(F32)
        flow[:5] += 9.0
        occ = (rng.random((h, w)) < 0.05).astype(F32)
        return {"in": {"im": im, "flow": flow, "occ": occ}, "out": {"out": (im.shape, F32)}}

    def call(ctx, d, I):
        ctx.warp_bicubic(d["out"], d["im"], d["flow"], d["occ"], w, h, ch)
    return Op(f"warp-bicubic-c{ch}-83x57", make, call, source="test_gpu_parity.py: test_warp_bicubic_any_channel_count")


def _image_dct(w, h):
    def make(rng):
        im = image(rng, w, h, 3)
        return {"in": {"fwd": im, "inv": im.copy()}, "out": {"fwd": (im.shape, F32), "inv": (im.shape, F32)}}

    def call(ctx, d, I):
        ctx.image_dct(d["fwd"], w, h, 3, False)
        ctx.image_dct(d["inv"], w, h, 3, True)
    return Op(f"image-dct-{w}x{h}x3", make, call, source="test_multiscale_edges.py: test_gpu_dct_scratch_reuse")


def _lz3():
    w, h, ch = 45, 31, 3
    w1, h1, w2, h2 = 23, 16, 12, 8

    def make(rng):
        return {"in": {"y0": image(rng, w, h, ch)},
                "out": {"y1": ((h1, w1, ch), F32), "y2": ((h2, w2, ch), F32), "r1": ((h1, w1, ch), F32),
                        "r0": ((h, w, ch), F32), "up": ((h, w, ch), F32)}}

    def call(ctx, d, I):
        ctx.lz3_down(d["y1"], d["y0"], w, h, ch)
        ctx.lz3_down(d["y2"], d["y1"], w1, h1, ch)
        ctx.lz3_recompose_step(d["r1"], d["y1"], w1, h1, d["y2"], w2, h2, ch, 1.5)
        ctx.lz3_recompose_step(d["r0"], d["y0"], w, h, d["r1"], w1, h1, ch, 0.0)
        ctx.lz3_up(d["up"], w, h, d["y1"], w1, h1, ch)
    return Op("lz3-decompose-recompose-45x31x3", make, call, source="test_lanczos3.py")


def _noise():
    w, h, ch = 37, 29, 3
    n = w * h * ch

    def make(rng):
        im = image(rng, w, h, ch, 0.0)
        return {"in": {"im": im}, "out": {k: (im.shape, F32) for k in ("awgn", "affine", "probe")},
                "ab": np.array([[0.4, 2.0], [0.1, 9.0], [0.0, 25.0]], F32)}

    def call(ctx, d, I):
        ctx.awgn(d["awgn"], d["im"], n, 20.0, 12345)
        ctx.noise_affine(d["affine"], d["im"], n, ch, I["ab"], 777)
        ctx.probe_add(d["probe"], d["im"], n, 0.5, 0x1234567890ABCDEF)
    return Op("awgn-noise-affine-probe-add", make, call, source="test_noise_gt.py, test_noise_curve.py, test_sure.py")


def _mse():
    w, h, ch = 37, 29, 3

    def make(rng):
        a = image(rng, w, h, ch)
        return {"in": {"a": a, "b": (a + rng.normal(0, 5, a.shape)).astype(F32)}, "out": {}}

    def call(ctx, d, I):
        return {"mse": np.float64(ctx.mse(d["a"], d["b"], w * h * ch))}
    return Op("mse-37x29x3", make, call, syncs="Context.mse downloads the sum (nlk_d2h)", source="test_noise_gt.py")


def _ssim(want_map):
    w, h, ch = 37, 29, 3

    def make(rng):
        a = image(rng, w, h, ch)
        return {"in": {"a": a, "b": (a + rng.normal(0, 9, a.shape)).astype(F32)}, "out": {}}

    def call(ctx, d, I):
        r = ctx.ssim(d["a"], d["b"], w, h, ch, want_map=want_map)
        out = {"ssim": np.float64(r[0]), "ssim_ch": r[1]}
        if want_map:
            out["map"] = r[2]
        return out
    return Op("ssim-37x29x3" + ("-map" if want_map else ""), make, call, syncs="Context.ssim downloads the result (nlk_d2h)",
              source="test_ssim.py")


def _sure(want_blocks):
    w, h, ch = 37, 29, 3

    def make(rng):
        y = image(rng, w, h, ch, 20.0)
        f = image(rng, w, h, ch, 2.0)
        return {"in": {"y": y, "f": f, "fp": (f + rng.normal(0, 0.1, f.shape)).astype(F32)}, "out": {}}

    def call(ctx, d, I):
        r = ctx.sure_terms(d["y"], d["f"], d["fp"], w, h, ch, block=16, seed=99, want_blocks=want_blocks)
        return {"totals": r[0], "blocks": r[1]} if want_blocks else {"totals": r}
    return Op("sure-terms-37x29x3" + ("-blocks" if want_blocks else ""), make, call,
              syncs="Context.sure_terms downloads the sums (nlk_d2h)", source="test_sure.py")


def _sigma():
    w, h, ch = 97, 71, 3

    def make(rng):
        return {"in": {"im": image(rng, w, h, ch, 12.0)}, "out": {}}

    def call(ctx, d, I):
        s, s_ch, counts = ctx.estimate_sigma(d["im"], w, h, ch)
        ab, bins = ctx.estimate_noise_curve(d["im"], w, h, ch, nmin=8, kmin=4)
        return {"sigma": np.float64(s), "sigma_ch": s_ch, "counts": counts, "ab": ab, "bins": bins}
    return Op("estimate-sigma-noise-curve-97x71x3", make, call, syncs="the wrappers download the estimates (nlk_d2h)",
              source="test_sigma.py, test_noise_curve.py")


def _vst():
    w, h, ch = 37, 29, 3
    n = w * h * ch
    ab = np.array([[0.5, 4.0], [0.0, 16.0], [0.2, 0.0]], F32)   # (an a = 0 channel, a b = 0 channel)

    def make(rng):
        im = image(rng, w, h, ch)
        im[3, 4, 1] = np.nan
        return {"in": {"im": im}, "out": {k: (im.shape, F32) for k in ("fwd", "inv0", "inv1")}, "s": pkg.vst_scale(ab)}

    def call(ctx, d, I):
        ctx.vst_forward(d["fwd"], d["im"], n, ch, ab, I["s"])
        ctx.vst_inverse(d["inv0"], d["fwd"], n, ch, ab, I["s"], 0)
        ctx.vst_inverse(d["inv1"], d["fwd"], n, ch, ab, I["s"], 1)
    return Op("vst-forward-inverse-c3", make, call, source="test_noise_curve.py")


def nlf_host_table(ch, nbins, tilt):
    """A valid table from synthetic bins (host only): variance rising with the mean, one empty bin."""
    bins = np.zeros((ch, nbins), pkg.CURVE_BIN)
    for c in range(ch):
        m = (np.arange(nbins) + 0.5) * 256.0 / nbins
        bins[c]["nblocks"] = 200
        bins[c]["nsel"] = 40
        bins[c]["mean"] = m
        bins[c]["var"] = 9.0 + tilt * (c + 1) * m
    bins["nsel"][0, nbins // 2] = 0
    return pkg.nlf_build(bins)


def _nlf(tag, nbins, tilt):
    n, ch = 3000, 3

    def make(rng):
        y = rng.uniform(-20, 280, n).astype(F32)
        y[7] = np.nan
        return {"in": {"y": y}, "out": {"fwd": ((n,), F32), "back": ((n,), F32)}, "t": nlf_host_table(ch, nbins, tilt)}

    def call(ctx, d, I):
        ctx.nlf_forward(d["fwd"], d["y"], n, ch, I["t"])
        ctx.nlf_inverse(d["back"], d["fwd"], n, ch, I["t"])
    return Op(f"nlf-table-{tag}", make, call, source="test_nlf.py: test_gpu_a_second_table_and_refused_arguments")


def _nlf_measured():
    w, h, ch = 97, 71, 3

    def make(rng):
        clean = synth.clean_frame(w, h, ch)
        im = synth.noise_affine(clean, (0.3, 4.0), int(rng.integers(1, 1 << 30)))
        return {"in": {"im": im}, "out": {"fwd": (im.shape, F32)}}

    def call(ctx, d, I):
        t = ctx.nlf_table(d["im"], w, h, ch, nmin=8, kmin=4)
        assert t.s > 0, "the measured table kept no bin"
        ctx.nlf_forward(d["fwd"], d["im"], w * h * ch, ch, t)
        return {"s": np.float32(t.s), "G": t.arrays()["G"]}
    return Op("nlf-table-measured-97x71x3", make, call, syncs="Context.nlf_table downloads the bins (nlk_d2h)",
              source="test_nlf.py")


def _despike_defect():
    w, h, ch = 37, 29, 3

    def make(rng):
        im = image(rng, w, h, ch, 3.0)
        im[5, 6, 0] += 120
        im[20, 30, 2] -= 110
        mean = image(rng, w, h, ch, 1.0)
        mean[9, 9, 1] += 60
        return {"in": {"im": im, "mean": mean},
                "out": {"clean": (im.shape, F32), "dout": (im.shape, F32), "mean_out": (im.shape, F32),
                        "map": ((h, w, ch), np.uint8), "count": ((ch,), np.uint32)}}

    def call(ctx, d, I):
        counts = ctx.despike_counts(d["clean"], d["im"], w, h, ch, 30.0, 1)
        ctx.defect_step(d["dout"], d["im"], d["mean_out"], d["mean"], w, h, ch, 20.0, 0.25, 1, d["map"], d["count"])
        return {"despike_counts": counts}
    return Op("despike-counts-defect-step-37x29x3", make, call, syncs="Context.despike_counts downloads the counts (nlk_d2h)",
              source="test_despike.py, test_defect_map.py")


def _yuv(tag, w, h):
    def make(rng):
        fmt = pkg.yuv_format_from_tag(tag)
        nbytes = fmt.frame_bytes(w, h)
        if fmt.depth > 8:
            buf = rng.integers(0, 1 << fmt.depth, nbytes // 2).astype("<u2").view(np.uint8)
        else:
            buf = rng.integers(0, 256, nbytes).astype(np.uint8)
        return {"in": {"yuv": buf}, "out": {"rgb": ((h, w, 3), F32), "back": ((nbytes,), np.uint8)}, "fmt": fmt}

    def call(ctx, d, I):
        ctx.yuv_to_rgb_dev(d["rgb"], d["yuv"], w, h, I["fmt"])
        ctx.rgb_to_yuv_dev(d["back"], d["rgb"], w, h, I["fmt"])
    return Op(f"yuv-{tag}-{w}x{h}", make, call, source="test_y4m.py")


def _copy_block():
    def make(rng):
        return {"in": {"src": image(rng, 31, 17, 3), "dst": np.zeros((11, 23, 3), F32)}, "out": {"dst": ((11, 23, 3), F32)}}

    def call(ctx, d, I):
        ctx.copy_block(d["dst"], 23, d["src"], 31, 3, 13, 9)
    return Op("copy-block", make, call, source="test_multiscale_edges.py")


OTHER_OPS = [
    _tvl1(131, 97), _tvl1(16, 16), _bm_flow(), _flow_invert(), _gray_occlusion(), _warp(3), _warp(2),
    _image_dct(333, 190), _image_dct(22, 13), _lz3(), _noise(), _mse(), _ssim(False), _ssim(True), _sure(False),
    _sure(True), _sigma(), _vst(), _nlf("a-16", 16, 0.05), _nlf("b-64", 64, 0.2), _nlf_measured(), _despike_defect(),
    _yuv("420jpeg", 37, 29), _yuv("422p10", 37, 29), _copy_block(),
]

OPS = FRAME_OPS + [_tiny(), _split_api(), _strip(False), _strip(True)] + OTHER_OPS
BY_NAME = {op.name: op for op in OPS}
assert len(BY_NAME) == len(OPS)
