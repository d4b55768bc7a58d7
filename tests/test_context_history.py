"""A context's results do not depend on the calls made before (-m gpu).

An nlk_ctx carries state from call to call (csrc/nlk_internal.h: scratch buffers that only grow and keep their old
bytes, the DCT tables cached by patch size, the device copy of the last NLF table, `last` for the strip calls, the
lazily expanded decision bytes, the in-launch replay's generation and tagged words, the wide-window queue counters,
deterministic mode's slabs and flags, the TV-L1 mailbox, the strip accumulator, the second stream and its events).
The rest of the suite runs on one session-wide context in collection order, so "call B is wrong only after call A"
is caught there only by accident. Here every operation of tests/ctx_ops.py is compared with its own result on a fresh
context: after a seeded shuffle of the whole table, after the transitions a shuffle may miss, and bit for bit in
deterministic mode. The contexts are this file's own, one alive at a time beside the sequence's."""
import os

import numpy as np
import pytest

import ctx_ops
from ctx_ops import BY_NAME, OPS, with_env

pytestmark = pytest.mark.gpu

_context, _fresh = ctx_ops.context, ctx_ops.fresh


def _run_and_compare(built, monkeypatch, c, op, what, det=False, seed=0):
    I, want = _fresh(built, monkeypatch, op, det, seed)
    got = with_env(op, monkeypatch, lambda: op.run(c, I, det))
    op.same(got, want, what, I, det)
    return got


def _sequence(built, monkeypatch, c, names, what, det=False):
    """names: "op" or "op@seed" (which of the op's inputs, default 0)."""
    for i, n in enumerate(names):
        before = ", ".join(names[max(0, i - 5):i]) or "nothing"
        name, _, seed = n.partition("@")
        _run_and_compare(built, monkeypatch, c, BY_NAME[name], f"{what}: {n} at position {i}, after {before}", det,
                         int(seed or 0))


@pytest.mark.parametrize("op", OPS, ids=[op.name for op in OPS])
def test_fresh_contexts_agree(built, monkeypatch, op):
    """Two fresh contexts, one run each: the comparison and its caps hold for the reference side alone. A failure
    here means the op is unsuitable for the table (change its input), not that the product is wrong."""
    I, first = _fresh(built, monkeypatch, op)
    c = _context(built)
    try:
        second = with_env(op, monkeypatch, lambda: op.run(c, I))
    finally:
        c.close()
    op.same(second, first, f"{op.name}: two fresh contexts", I)
    if not op.bitexact:   # (the flag of the table is what the device gives: reported, and asserted where it says "bit-exact")
        try:
            ctx_ops.same_bits(second, first, op.name)
            print(f"{op.name}: bit-identical on this pair of runs (table: not bit-exact)")
        except AssertionError:
            pass


def _shuffles(ops, default_seed):
    """A seeded shuffle of `ops`, three times over with different permutations (NLK_RANDOM_SEED / NLK_RANDOM_COUNT run
    other or longer sequences, e.g. as a soak test). Every round runs an op on the other one of its two inputs: what
    its run of the round before left in the context is not this round's answer."""
    rng = np.random.default_rng(int(os.environ.get("NLK_RANDOM_SEED", default_seed)))
    rounds = int(os.environ.get("NLK_RANDOM_COUNT", 3))
    return [f"{ops[i].name}@{r % 2}" for r in range(rounds) for i in rng.permutation(len(ops))]


def test_results_do_not_depend_on_history(built, monkeypatch):
    """One context, default mode, the whole table shuffled three times over: every result against the op's
    fresh-context result."""
    names = _shuffles(OPS, 2025)
    c = _context(built)
    try:
        _sequence(built, monkeypatch, c, names, "shuffle")
    finally:
        c.close()


# ---------------------------------------------------------------- transitions a shuffle may miss

T120, S120 = "flt1-temporal-p8c3-120x88", "flt1-spatial-p8c3-120x88"
TRANSITIONS = {   # ("op@1": the op on the second of its inputs - same shapes and parameters, other values)
    # the replay words of a taller grid under a shorter one, then buffers that regrow
    "tall-short-tall-grid": [T120, "flt1-temporal-p8c3-33x47", S120, "flt1-temporal-p8c3-64x48", T120 + "@1",
                             "flt1-spatial-p8c3-200x172", "flt1-temporal-p8c3-33x47@1"],
    # the DCT / window tables cached by patch size
    "tables-12-6-12": ["flt1-temporal-p12c3-84x60", "flt1-temporal-p6c1-61x53", "flt1-temporal-p12c3-84x60@1"],
    # last.packed: packed lists, a radius that has no packed form, packed lists again
    "packed-unpacked-packed": [T120, "flt1-temporal-p8c1-120x88-st8", T120 + "@1", "flt1-temporal-p8c1-120x88", T120],
    # the generation of the tagged words moves on across a call that does not use them: the same frame both ways
    # (records read every time), then another frame both ways
    "replay-in-launch-then-separate-kernels": [T120, T120 + "-nochase", T120, T120 + "-nochase@1", T120 + "@1",
                                               T120 + "-nochase"],
    "smaller-than-a-patch-after-a-frame": [T120, "flt1-20x7-smaller-than-a-patch", T120 + "@1",
                                           "flt1-20x7-smaller-than-a-patch@1"],
    "tvl1-large-small-large": ["tvl1-131x97", "tvl1-16x16", "tvl1-131x97@1", "tvl1-16x16@1"],
    "nlf-tables-alternate": ["nlf-table-a-16", "nlf-table-b-64", "nlf-table-a-16@1", "nlf-table-b-64@1", "nlf-table-a-16"],
    # four planes (cur | prev | basic | prev - cur), then one plane of a larger frame
    "smoother-then-larger-spatial": ["smo1-p8c3-120x88", "flt1-spatial-p8c3-200x172", "smo1-p8c3-120x88@1"],
    "strip-calls-around-whole-frames": ["strip-match-commit-group-gy0", T120, "strip-match-part-x2-commit-group", S120,
                                        "split-accumulate-filter-smoother-normalize", "strip-match-commit-group-gy0@1",
                                        "strip-match-part-x2-commit-group@1"],
    "long-lists-between-short": [T120, "flt1-temporal-p8c3-72x56-n129", T120 + "@1", "flt1-temporal-p20c3-90x70",
                                 T120, "flt1-temporal-p8c3-72x56-n129@1"],
}


@pytest.mark.parametrize("name", list(TRANSITIONS))
def test_directed_transitions(built, monkeypatch, name):
    c = _context(built)
    try:
        _sequence(built, monkeypatch, c, TRANSITIONS[name], name)
    finally:
        c.close()


def test_replay_in_launch_and_separate_kernels_give_the_same_records(built, monkeypatch):
    """The two ops of the transition above share their input: whatever replays the mask, the decisions and lists are
    the same (what makes that transition a statement about ONE frame)."""
    a, b = BY_NAME[T120], BY_NAME[T120 + "-nochase"]
    (I, ra), (_, rb) = _fresh(built, monkeypatch, a), _fresh(built, monkeypatch, b)
    ctx_ops.check_records(ra["records"], rb["records"], "replay in the launch vs separate kernels")
    for f in ("active", "nsel", "np0", "nagg"):
        assert np.array_equal(ra["records"][f], rb["records"][f]), f
    assert 0.05 < 1 - ra["records"]["active"].mean() < 0.9   # (the mask really skips targets)


class _Buffers:
    """Device buffers of a test's own, freed when the block ends, however it ends."""

    def __init__(self, c):
        self.c, self.mine = c, []

    def __enter__(self):
        return self

    def upload(self, a):
        self.mine.append(self.c.upload(a))
        return self.mine[-1]

    def alloc(self, n):
        self.mine.append(self.c.alloc(n))
        return self.mine[-1]

    def op_buffers(self, I):
        d = {k: self.upload(v) for k, v in I["in"].items()}
        d["out"] = self.alloc(I["in"]["cur"].nbytes)
        return d

    def __exit__(self, *exc):
        self.c.sync()
        for p in self.mine:
            self.c.free(p)


def _refusals(built, c, B):
    """The refusals by argument checks that include/nlk_hip.h promises to leave the context as it was: (name, call
    that must raise NlkError, pattern of its message)."""
    im = np.zeros((40, 40, 1), np.float32)
    d, o, marks = B.upload(im), B.alloc(im.nbytes), B.upload(np.zeros(19 * 19, np.uint64))
    p34 = built.default_params(20.0, 0, patch_sz=34)
    p4 = built.default_params(20.0, 0, patch_sz=4, search_sz_x=10)   # (reach 5: tests/test_gpu_parity.py:225)
    p8 = built.default_params(20.0, 0)
    return [("patch size 34", lambda: c.filter_frame(o, d, None, None, 40, 40, 1, 20.0, p34), "not supported"),
            ("strip_match with mark words at reach 5",
             lambda: c.strip_match(marks, d, None, None, 40, 40, 1, 20.0, p4, 0, 19), "reach"),
            ("strip_match_rows outside the strip's rows",
             lambda: c.strip_match_rows(marks, d, None, None, 40, 40, 1, 20.0, p8, 0, 9, 5, 5), "outside the strip")]


def test_refused_call_between_two_good_calls(built, monkeypatch):
    """include/nlk_hip.h (nlk_dev_strip_match, "Refused calls"): a call refused by its argument checks - a patch size
    the kernels do not cover, nlk_dev_strip_match with mark words at a reach above 3, target rows outside the strip -
    leaves the context as it was. The calls around it give their fresh results, the records read after it are still
    the last good call's, also where nobody had read them yet (the decisions of a replay inside the group launch are
    tagged words, expanded on demand; the decision bytes in the context are then those of ANOTHER frame of the same
    grid, read before), and a strip_group after it still works on the last good call's state."""
    op = BY_NAME[T120]
    I, want = _fresh(built, monkeypatch, op)
    c = _context(built)
    try:
        with _Buffers(c) as B:
            for what, refused, pattern in _refusals(built, c, B):
                first = _run_and_compare(built, monkeypatch, c, op, f"before: {what}")
                with pytest.raises(built.NlkError, match=pattern):
                    refused()
                ctx_ops.check_records(c.read_records(), first["records"], f"records after a refused call: {what}")
                _run_and_compare(built, monkeypatch, c, BY_NAME[S120], f"a spatial frame of the same grid, after: {what}")
                dd = B.op_buffers(I)
                op.call(c, dd, I)
                with pytest.raises(built.NlkError, match=pattern):
                    refused()
                got = {"out": c.download(dd["out"], I["in"]["cur"].shape), "records": c.read_records()}
                op.same(got, want, f"a good call whose records are first read after a refused call: {what}", I)
                _group_of_last_frame(c, B, I, got, f"strip_group after a refused call: {what}")
    finally:
        c.close()


def test_late_refusal_leaves_no_match_state(built, monkeypatch):
    """include/nlk_hip.h: a call that is refused after it has begun to work on the context (here the generic matcher,
    whose lists of 11000 entries need more LDS than a workgroup has: tests/test_long_lists.py:
    test_generic_matcher_refuses_above_its_lds) has overwritten part of what the call before left. It must not pass
    for that call: the readers of the match state fail cleanly until a call is accepted again, which then gives its
    fresh result."""
    op = BY_NAME[T120]
    c = _context(built)
    try:
        _run_and_compare(built, monkeypatch, c, op, "before the late refusal")
        with _Buffers(c) as B:
            cur = np.full((24, 24, 3), 100.0, np.float32)
            d_cur, d_out = B.upload(cur), B.alloc(cur.nbytes)
            p = built.default_params(20.0, built.FLT1, npatches_x=11000, npatches_t=11000, npatches_tagg=11000)
            with pytest.raises(built.NlkError, match="LDS"):
                c.filter_frame(d_out, d_cur, None, None, 24, 24, 3, 20.0, p)
            with pytest.raises(built.NlkError, match="no frame has been processed"):
                c.read_records()
            with pytest.raises(built.NlkError, match="has not run"):
                c.strip_group(d_out, d_cur)
            with pytest.raises(built.NlkError, match="no frame has been processed"):
                c.count_packed()
        _run_and_compare(built, monkeypatch, c, op, "after the late refusal")
        _run_and_compare(built, monkeypatch, c, BY_NAME[S120], "after the late refusal")
    finally:
        c.close()


def test_frame_smaller_than_a_patch_leaves_the_records(built, monkeypatch):
    """include/nlk_hip.h (nlk_ctx_read_records): a whole-frame call on an image smaller than a patch copies its input,
    runs no match phase and leaves the records, and the strip calls' state, of the call before it."""
    op, tiny = BY_NAME[T120], BY_NAME["flt1-20x7-smaller-than-a-patch"]
    I, want = _fresh(built, monkeypatch, op)
    c = _context(built)
    try:
        with _Buffers(c) as B:
            _run_and_compare(built, monkeypatch, c, BY_NAME[S120], "a spatial frame of the same grid")
            dd = B.op_buffers(I)
            op.call(c, dd, I)
            _run_and_compare(built, monkeypatch, c, tiny, "the copy path")
            got = {"out": c.download(dd["out"], I["in"]["cur"].shape), "records": c.read_records()}
            op.same(got, want, "records first read after a frame smaller than a patch", I)
            _group_of_last_frame(c, B, I, got, "strip_group after a frame smaller than a patch")
    finally:
        c.close()


def _group_of_last_frame(c, B, I, whole, what):
    """nlk_dev_strip_group on the state a whole-frame call of the op T120 left: with the frame's own decisions it
    rebuilds the frame `whole` (and leaves its records alone)."""
    w, h, ch = I["w"], I["h"], I["ch"]
    d_cur = B.upload(I["in"]["cur"])
    d_acc = B.upload(np.zeros((ch + 1, h, w), np.float32))
    d_act = B.upload(whole["records"]["active"])
    d_out = B.alloc(I["in"]["cur"].nbytes)
    c.strip_group(d_acc, d_act)
    c.frame_normalize(d_out, d_acc, d_cur, w, h, ch, 0, h)
    got = c.download(d_out, I["in"]["cur"].shape)
    ctx_ops.same_frame({"out": got}, {"out": whole["out"]}, what, I)
    ctx_ops.check_records(c.read_records(), whole["records"], f"{what}: records afterwards")


def test_strip_group_after_a_whole_frame_call(built, monkeypatch):
    """include/nlk_hip.h: nlk_dev_strip_group works on what the context's LAST match phase left, whichever call ran
    it. After the strip op and then a whole-frame call, a strip_group without a new match is the group phase of that
    whole frame (its grid, its planar images, its lists): with the frame's own decisions it rebuilds the frame."""
    op = BY_NAME[T120]
    c = _context(built)
    try:
        _run_and_compare(built, monkeypatch, c, BY_NAME["strip-match-commit-group-gy0"], "strip op first")
        whole = _run_and_compare(built, monkeypatch, c, op, "whole frame after the strip op")
        I, _ = _fresh(built, monkeypatch, op)
        with _Buffers(c) as B:
            _group_of_last_frame(c, B, I, whole, "strip_group on a whole-frame call's state")
    finally:
        c.close()


def test_two_band_frame_followed_at_once_by_a_one_band_frame(built, monkeypatch):
    """NLK_BANDS=2 puts half of a frame on the context's second stream; the next call, enqueued with no
    synchronisation in between, reuses every scratch buffer of the first. Both against their fresh results."""
    a, b = BY_NAME["flt1-spatial-p8c3-200x172-bands2"], BY_NAME[T120]
    (Ia, wa), (Ib, wb) = _fresh(built, monkeypatch, a), _fresh(built, monkeypatch, b)
    c = _context(built)
    try:
        for rep in range(2):
            with _Buffers(c) as B:
                da, db = B.op_buffers(Ia), B.op_buffers(Ib)
                with_env(a, monkeypatch, lambda: (a.call(c, da, Ia), a.check(c, Ia)))
                b.call(c, db, Ib)   # (nothing waited for the device since the banded call was enqueued)
                b.check(c, Ib)
                ga = {"out": c.download(da["out"], Ia["in"]["cur"].shape)}
                gb = {"out": c.download(db["out"], Ib["in"]["cur"].shape), "records": c.read_records()}
            ctx_ops.same_frame(ga, {"out": wa["out"]}, f"two bands, then one at once (round {rep}): the banded frame", Ia)
            b.same(gb, wb, f"two bands, then one at once (round {rep}): the frame after it", Ib)
    finally:
        c.close()


# ---------------------------------------------------------------- deterministic mode

DET_OPS = [op for op in OPS if op.det_ok]


def test_deterministic_mode_history_is_bit_exact(built, monkeypatch):
    """nlk_ctx_set_deterministic: slabs and an ordered gather instead of float atomics. The frame ops shuffled on one
    deterministic context: every output bit for bit that of a fresh deterministic context - no caps, no tolerance
    (the slabs' "written" flags are not cleared between calls, csrc/group_det.h). Then one context toggled off, on,
    off, on between calls, each call against the fresh result of its mode."""
    c = _context(built, det=True)
    try:
        _sequence(built, monkeypatch, c, _shuffles(DET_OPS, 4711), "deterministic shuffle", det=True)
    finally:
        c.close()
    c = _context(built)
    try:
        for name in (T120, S120, "split-accumulate-filter-smoother-normalize", "flt1-temporal-p12c3-84x60"):
            for seed, det in enumerate((False, True, False, True, True)):
                c.set_deterministic(det)
                _run_and_compare(built, monkeypatch, c, BY_NAME[name], f"{name} with deterministic toggled to {det}", det,
                                 seed % 2)
    finally:
        c.close()
