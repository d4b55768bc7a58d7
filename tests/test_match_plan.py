"""The plan of a frame call's match launches, pinned: nlk_host_match_plan (include/nlk_hip.h) runs the geometry code of
the frame calls (nlk_frame_geom, csrc/tu_frame.hip) and their planner (nlk_match_plan, csrc/tu_match.hip) without a
context or a device. No GPU.

A wrong match shape computes the right result more slowly, so nothing else notices one. PLANS holds, for inputs that
reach every branch of the planner, every output field as the commit BEFORE the planner moved into tu_match.hip computed
it (32bfbe5: its lines of plan_frame and of match_launch.h, lifted verbatim into a scratch program that printed these
rows) - recorded, never produced by the code under test. What profiles/match_plan_refactor.txt says about the sweep of
random geometries is the wide check; this table is the one that stays."""
import pytest

FIELDS = ("generic", "wide", "tgx", "tgy", "bx", "threads", "block", "order", "halo", "rwp", "rh_max", "ksel_max", "ntx",
          "rounds", "lds", "wide_halo", "wide_rwp", "wide_rh_max", "wide_rounds", "wide_lds")
SWITCHES = ("NLK_MTX", "NLK_MTY", "NLK_MATCH_BX2", "NLK_MATCH_BLOCK", "NLK_MATCH_NOBLOCK", "NLK_MATCH_ORDER",
            "NLK_GENERIC_MATCH", "NLK_MATCH_WG8")
EUNSUP, EINVAL = -4, -3

# (id, w, h, ch, (patch_sz, search_sz_x, search_sz_t, npatches_x, npatches_t, npatches_tagg), smoother, have_prev,
#  target rows of the call (0: the whole grid), switches, the FIELDS - or the frame call's error code)
# Parameters: the defaults at sigma 20 of FLT1 (8, 10, 5, 50, 30, 20), FLT2 (.., 20, 20, 1) and SMO1 (.., 0, 45, 45)
# unless the row is about something else. First frame: 441 candidates (7 rounds); temporal: 121 (2 rounds) and the wide
# tile for the spatial radius. 575 / 576 tiles: 23 x 25 / 24 x 24 tiles of 8 x 4 targets.
PLANS = [
    ("1080px1-first", 1920, 1080, 1, (8, 10, 5, 50, 30, 20), 0, 0, 0, {},
     (0, 0, 8, 4, 2, 512, 1, 0, 10, 85, 40, 50, 60, 7, 19044, 0, 0, 0, 0, 0)),
    ("1080px1-temporal", 1920, 1080, 1, (8, 10, 5, 50, 30, 20), 0, 1, 0, {},
     (0, 1, 8, 4, 2, 512, 1, 0, 5, 75, 30, 50, 60, 2, 14444, 10, 53, 28, 7, 26464)),
    ("1080px1-flt2", 1920, 1080, 1, (8, 10, 5, 20, 20, 1), 0, 1, 0, {},
     (0, 1, 8, 4, 2, 512, 1, 0, 5, 75, 30, 20, 60, 2, 10956, 10, 53, 28, 7, 24736)),
    ("1080px1-smoother", 1920, 1080, 1, (8, 10, 5, 0, 45, 45), 1, 1, 0, {},
     (0, 0, 8, 4, 2, 512, 1, 0, 5, 75, 30, 45, 60, 2, 14764, 0, 0, 0, 0, 0)),
    ("1080px3-first", 1920, 1080, 3, (8, 10, 5, 50, 30, 20), 0, 0, 0, {},
     (0, 0, 8, 4, 2, 512, 1, 0, 10, 85, 40, 50, 60, 7, 46244, 0, 0, 0, 0, 0)),
    ("1080px3-temporal", 1920, 1080, 3, (8, 10, 5, 50, 30, 20), 0, 1, 0, {},
     (0, 1, 8, 4, 2, 512, 1, 0, 5, 75, 30, 50, 60, 2, 32444, 10, 53, 28, 7, 73952)),
    ("1080px3-flt2", 1920, 1080, 3, (8, 10, 5, 20, 20, 1), 0, 1, 0, {},
     (0, 1, 8, 4, 2, 512, 1, 0, 5, 75, 30, 20, 60, 2, 28956, 10, 53, 28, 7, 72224)),
    ("1080px3-smoother", 1920, 1080, 3, (8, 10, 5, 0, 45, 45), 1, 1, 0, {},
     (0, 0, 8, 4, 2, 512, 1, 0, 5, 75, 30, 45, 60, 2, 32764, 0, 0, 0, 0, 0)),
    ("256x1-first", 256, 256, 1, (8, 10, 5, 50, 30, 20), 0, 0, 0, {},
     (0, 0, 4, 2, 4, 256, 0, 0, 10, 53, 32, 50, 16, 7, 9508, 0, 0, 0, 0, 0)),
    ("256x1-temporal", 256, 256, 1, (8, 10, 5, 50, 30, 20), 0, 1, 0, {},
     (0, 1, 4, 2, 4, 256, 0, 0, 5, 43, 22, 50, 16, 2, 6508, 10, 53, 28, 7, 26464)),
    ("256x1-flt2", 256, 256, 1, (8, 10, 5, 20, 20, 1), 0, 1, 0, {},
     (0, 1, 4, 2, 4, 256, 0, 0, 5, 43, 22, 20, 16, 2, 4764, 10, 53, 28, 7, 24736)),
    ("256x1-smoother", 256, 256, 1, (8, 10, 5, 0, 45, 45), 1, 1, 0, {},
     (0, 0, 4, 2, 4, 256, 0, 0, 5, 43, 22, 45, 16, 2, 6668, 0, 0, 0, 0, 0)),
    ("256x3-first", 256, 256, 3, (8, 10, 5, 50, 30, 20), 0, 0, 0, {},
     (0, 0, 4, 2, 4, 256, 0, 0, 10, 53, 32, 50, 16, 7, 23076, 0, 0, 0, 0, 0)),
    ("256x3-temporal", 256, 256, 3, (8, 10, 5, 50, 30, 20), 0, 1, 0, {},
     (0, 1, 4, 2, 4, 256, 0, 0, 5, 43, 22, 50, 16, 2, 14076, 10, 53, 28, 7, 73952)),
    ("256x3-flt2", 256, 256, 3, (8, 10, 5, 20, 20, 1), 0, 1, 0, {},
     (0, 1, 4, 2, 4, 256, 0, 0, 5, 43, 22, 20, 16, 2, 12332, 10, 53, 28, 7, 72224)),
    ("256x3-smoother", 256, 256, 3, (8, 10, 5, 0, 45, 45), 1, 1, 0, {},
     (0, 0, 4, 2, 4, 256, 0, 0, 5, 43, 22, 45, 16, 2, 14236, 0, 0, 0, 0, 0)),
    ("575-tiles", 740, 404, 3, (8, 10, 5, 50, 30, 20), 0, 1, 0, {},
     (0, 1, 4, 2, 4, 256, 0, 0, 5, 43, 22, 50, 46, 2, 14076, 10, 53, 28, 7, 73952)),
    ("576-tiles", 772, 388, 3, (8, 10, 5, 50, 30, 20), 0, 1, 0, {},
     (0, 1, 8, 4, 2, 512, 1, 0, 5, 75, 30, 50, 24, 2, 32444, 10, 53, 28, 7, 73952)),
    ("575-tiles-first", 740, 404, 1, (8, 10, 5, 50, 30, 20), 0, 0, 0, {},
     (0, 0, 4, 2, 4, 256, 0, 0, 10, 53, 32, 50, 46, 7, 9508, 0, 0, 0, 0, 0)),
    ("576-tiles-first", 772, 388, 1, (8, 10, 5, 50, 30, 20), 0, 0, 0, {},
     (0, 0, 8, 4, 2, 512, 1, 0, 10, 85, 40, 50, 24, 7, 19044, 0, 0, 0, 0, 0)),
    ("1080p-strip34", 1920, 1080, 3, (8, 10, 5, 50, 30, 20), 0, 1, 34, {},
     (0, 1, 4, 2, 4, 256, 0, 0, 5, 43, 22, 50, 120, 2, 14076, 10, 53, 28, 7, 73952)),
    ("1080p-strip67-first", 1920, 1080, 3, (8, 10, 5, 50, 30, 20), 0, 0, 67, {},
     (0, 0, 8, 4, 2, 512, 1, 0, 10, 85, 40, 50, 60, 7, 46244, 0, 0, 0, 0, 0)),
    ("psz4-temporal", 1920, 1080, 3, (4, 10, 5, 50, 30, 20), 0, 1, 0, {},
     (0, 1, 8, 4, 4, 256, 1, 0, 5, 43, 20, 50, 120, 2, 13044, 10, 53, 24, 7, 63776)),
    ("psz6-temporal", 1920, 1080, 1, (6, 10, 5, 50, 30, 20), 0, 1, 0, {},
     (0, 1, 8, 4, 4, 256, 1, 0, 5, 43, 25, 50, 80, 2, 7024, 10, 53, 26, 7, 24768)),
    ("psz6-first", 1920, 1080, 3, (6, 10, 5, 50, 30, 20), 0, 0, 0, {},
     (0, 0, 8, 4, 4, 256, 1, 0, 10, 53, 35, 50, 80, 7, 24984, 0, 0, 0, 0, 0)),
    ("psz10-temporal", 1920, 1080, 3, (10, 10, 5, 50, 30, 20), 0, 1, 0, {},
     (0, 1, 8, 4, 2, 512, 1, 0, 5, 75, 35, 50, 48, 2, 36944, 10, 53, 30, 7, 79040)),
    ("psz12-temporal", 1920, 1080, 3, (12, 10, 5, 50, 30, 20), 0, 1, 0, {},
     (0, 1, 8, 4, 2, 512, 1, 0, 5, 75, 40, 50, 40, 2, 41444, 10, 53, 32, 7, 84128)),
    ("psz12-first", 1920, 1080, 3, (12, 10, 5, 50, 30, 20), 0, 0, 0, {},
     (0, 0, 8, 4, 4, 256, 1, 0, 10, 85, 50, 50, 40, 7, 53724, 0, 0, 0, 0, 0)),
    ("psz16-temporal", 1920, 1080, 1, (16, 10, 5, 50, 30, 20), 0, 1, 0, {},
     (0, 1, 8, 4, 2, 512, 1, 0, 5, 107, 50, 50, 30, 2, 26844, 10, 53, 36, 7, 33248)),
    ("psz16-smoother", 1920, 1080, 3, (16, 10, 5, 0, 45, 45), 1, 1, 0, {},
     (0, 0, 8, 4, 2, 512, 1, 0, 5, 107, 50, 45, 30, 2, 69964, 0, 0, 0, 0, 0)),
    ("generic-2ch", 1920, 1080, 2, (8, 10, 5, 50, 30, 20), 0, 1, 0, {},
     (1, 0, 8, 4, 2, 512, 1, 0, 5, 75, 30, 50, 60, 2, 23444, 0, 0, 0, 0, 0)),
    ("generic-psz5", 1920, 1080, 3, (5, 10, 5, 50, 30, 20), 0, 1, 0, {},
     (1, 0, 8, 4, 4, 256, 1, 0, 5, 43, 21, 50, 120, 2, 13560, 0, 0, 0, 0, 0)),
    ("generic-radius16", 1920, 1080, 3, (8, 16, 5, 50, 30, 20), 0, 0, 0, {},
     (1, 0, 8, 4, 4, 256, 1, 0, 16, 97, 52, 50, 60, 16, 63252, 0, 0, 0, 0, 0)),
    ("generic-radius16-temporal", 1920, 1080, 3, (8, 16, 5, 50, 30, 20), 0, 1, 0, {},
     (1, 0, 8, 4, 2, 512, 1, 0, 5, 75, 30, 50, 60, 2, 32444, 0, 0, 0, 0, 0)),
    ("lds-4-wavefronts", 1920, 1080, 3, (8, 10, 5, 1200, 1200, 1200), 0, 1, 0, {},
     (0, 1, 8, 4, 4, 256, 1, 0, 5, 75, 30, 1200, 60, 2, 103804, 10, 53, 28, 7, 148032)),
    ("lds-generic", 1920, 1080, 3, (8, 10, 5, 2500, 2500, 2000), 0, 1, 0, {},
     (1, 0, 8, 4, 4, 256, 1, 0, 5, 75, 30, 2500, 60, 2, 179004, 0, 0, 0, 0, 0)),
    ("lds-4-wavefronts-first", 1920, 1080, 3, (8, 10, 5, 1200, 1200, 1200), 0, 0, 0, {},
     (0, 0, 8, 4, 4, 256, 1, 0, 10, 85, 40, 1200, 60, 7, 117604, 0, 0, 0, 0, 0)),
    ("wide-over-limit", 1920, 1080, 3, (8, 15, 5, 800, 800, 700), 0, 1, 0, {},
     (1, 0, 8, 4, 2, 512, 1, 0, 5, 75, 30, 800, 60, 2, 126204, 0, 0, 0, 0, 0)),
    ("wide-over-limit-after-fallback", 1920, 1080, 3, (8, 10, 5, 1500, 1500, 1300), 0, 1, 0, {},
     (1, 0, 8, 4, 4, 256, 1, 0, 5, 75, 30, 1500, 60, 2, 119804, 0, 0, 0, 0, 0)),
    ("mtx8-mty4-small", 256, 256, 1, (8, 10, 5, 50, 30, 20), 0, 1, 0, {'NLK_MTX': '8', 'NLK_MTY': '4'},
     (0, 1, 8, 4, 4, 256, 0, 0, 5, 75, 30, 50, 8, 2, 11724, 10, 53, 28, 7, 26464)),
    ("mtx8-mty4-block-small", 256, 256, 1, (8, 10, 5, 50, 30, 20), 0, 1, 0, {'NLK_MTX': '8', 'NLK_MTY': '4', 'NLK_MATCH_BLOCK': '1'},
     (0, 1, 8, 4, 2, 512, 1, 0, 5, 75, 30, 50, 8, 2, 14444, 10, 53, 28, 7, 26464)),
    ("block-small", 256, 256, 3, (8, 10, 5, 50, 30, 20), 0, 1, 0, {'NLK_MATCH_BLOCK': '1'},
     (0, 1, 4, 2, 4, 256, 1, 0, 5, 43, 22, 50, 16, 2, 14076, 10, 53, 28, 7, 73952)),
    ("noblock", 1920, 1080, 3, (8, 10, 5, 50, 30, 20), 0, 1, 0, {'NLK_MATCH_NOBLOCK': '1'},
     (0, 1, 8, 4, 2, 512, 0, 0, 5, 75, 30, 50, 60, 2, 32444, 10, 53, 28, 7, 73952)),
    ("bx2-off", 1920, 1080, 3, (8, 10, 5, 50, 30, 20), 0, 1, 0, {'NLK_MATCH_BX2': '0'},
     (0, 1, 8, 4, 4, 256, 1, 0, 5, 75, 30, 50, 60, 2, 29724, 10, 53, 28, 7, 73952)),
    ("bx2-off-first", 1920, 1080, 3, (8, 10, 5, 50, 30, 20), 0, 0, 0, {'NLK_MATCH_BX2': '0'},
     (0, 0, 8, 4, 4, 256, 1, 0, 10, 85, 40, 50, 60, 7, 43524, 0, 0, 0, 0, 0)),
    ("order-block-8", 1920, 1080, 3, (8, 10, 5, 50, 30, 20), 0, 1, 0, {'NLK_MATCH_ORDER': 'block'},
     (0, 1, 8, 4, 2, 512, 1, 1, 5, 75, 30, 50, 60, 2, 32444, 10, 53, 28, 7, 73952)),
    ("order-block-12-ignored", 1920, 1080, 3, (12, 10, 5, 50, 30, 20), 0, 1, 0, {'NLK_MATCH_ORDER': 'block'},
     (0, 1, 8, 4, 2, 512, 1, 0, 5, 75, 40, 50, 40, 2, 41444, 10, 53, 32, 7, 84128)),
    ("generic-switch", 1920, 1080, 3, (8, 10, 5, 50, 30, 20), 0, 1, 0, {'NLK_GENERIC_MATCH': '1'},
     (1, 0, 8, 4, 2, 512, 1, 0, 5, 75, 30, 50, 60, 2, 32444, 0, 0, 0, 0, 0)),
    ("retired-wg8", 1920, 1080, 3, (8, 10, 5, 50, 30, 20), 0, 1, 0, {'NLK_MATCH_WG8': '1'},
     (0, 1, 8, 4, 2, 512, 1, 0, 5, 75, 30, 50, 60, 2, 32444, 10, 53, 28, 7, 73952)),
    ("retired-wg8-first-1ch", 1920, 1080, 1, (8, 10, 5, 50, 30, 20), 0, 0, 0, {'NLK_MATCH_WG8': '1'},
     (0, 0, 8, 4, 2, 512, 1, 0, 10, 85, 40, 50, 60, 7, 19044, 0, 0, 0, 0, 0)),
    ("refused-psz1", 256, 256, 1, (1, 10, 5, 50, 30, 20), 0, 0, 0, {},
     -4),
    ("refused-small-image", 6, 6, 1, (8, 10, 5, 50, 30, 20), 0, 0, 0, {},
     -3),
    ("refused-negative-radius", 256, 256, 1, (8, -1, 5, 50, 30, 20), 0, 0, 0, {},
     -3),
    ("refused-rows", 256, 256, 1, (8, 10, 5, 50, 30, 20), 0, 0, 64, {},
     -3),
]
BY_ID = {row[0]: row for row in PLANS}


def _plan(built, monkeypatch, row):
    _, w, h, ch, prm, smoother, have_prev, rows, env, _ = row
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)
    for name, value in env.items():
        monkeypatch.setenv(name, value)
    keys = ("patch_sz", "search_sz_x", "search_sz_t", "npatches_x", "npatches_t", "npatches_tagg")
    p = built.Params(**dict(zip(keys, prm)), dista_lambda=1.0, beta_x=1.0, beta_t=1.0)
    return built.host_match_plan(w, h, ch, p, smoother, have_prev, rows)


def test_table_is_well_formed():
    assert len(PLANS) >= 24 and len(BY_ID) == len(PLANS)
    assert all(isinstance(r[9], int) or len(r[9]) == len(FIELDS) for r in PLANS)


@pytest.mark.parametrize("row", PLANS, ids=[r[0] for r in PLANS])
def test_match_plan_is_the_recorded_one(built, monkeypatch, row):
    want = row[9]
    if isinstance(want, int):  # refused like the frame call refuses it, nothing written
        with pytest.raises(built.NlkError) as e:
            _plan(built, monkeypatch, row)
        assert e.value.args[1] == want
        return
    got = _plan(built, monkeypatch, row)
    assert tuple(got) == FIELDS == built.MATCH_PLAN_FIELDS
    assert got == dict(zip(FIELDS, want)), {k: (got[k], v) for k, v in zip(FIELDS, want) if got[k] != v}


def test_refused_inputs_write_nothing(built):
    import ctypes as C
    out = (C.c_int * 20)(*([-77] * 20))
    for w, h, psz, code in ((256, 256, 1, EUNSUP), (6, 6, 8, EINVAL)):
        p = built.Params(patch_sz=psz, search_sz_x=10, search_sz_t=5, npatches_x=50, npatches_t=30, npatches_tagg=20)
        assert built.hip().nlk_host_match_plan(w, h, 1, C.byref(p), 0, 0, 0, out) == code
        assert list(out) == [-77] * 20


def test_retired_switch_is_ignored(built, monkeypatch):
    """NLK_MATCH_WG8 (tiles of 8 x 8 targets, retired): a set variable changes nothing"""
    for with_it, without in (("retired-wg8", "1080px3-temporal"), ("retired-wg8-first-1ch", "1080px1-first")):
        assert BY_ID[with_it][9] == BY_ID[without][9]
        assert _plan(built, monkeypatch, BY_ID[with_it]) == _plan(built, monkeypatch, BY_ID[without])


def test_branches_the_table_reaches():
    """the rows are the issue's: every branch of the planner has one"""
    f = {r[0]: dict(zip(FIELDS, r[9])) for r in PLANS if not isinstance(r[9], int)}
    assert f["575-tiles"]["tgx"] == 4 and f["576-tiles"]["tgx"] == 8 and f["1080p-strip34"]["tgx"] == 4  # small-grid limit
    assert (f["psz4-temporal"]["bx"], f["psz6-temporal"]["threads"]) == (4, 256)
    assert (f["psz12-temporal"]["bx"], f["psz12-first"]["bx"], f["psz16-temporal"]["bx"]) == (2, 4, 2)
    assert all(f[k]["generic"] for k in ("generic-2ch", "generic-psz5", "generic-radius16", "generic-switch", "lds-generic",
                                         "wide-over-limit"))
    assert (f["lds-4-wavefronts"]["threads"], f["lds-4-wavefronts"]["generic"]) == (256, 0)
    assert f["1080px3-temporal"]["wide"] and not f["1080px3-first"]["wide"] and not f["1080px3-smoother"]["wide"]
    assert f["order-block-8"]["order"] == 1 and f["order-block-12-ignored"]["order"] == 0


def test_default_parameters_are_the_table_s(built):
    for mode, want in ((built.FLT1, (8, 10, 5, 50, 30, 20)), (built.FLT2, (8, 10, 5, 20, 20, 1)), (built.SMO1, (8, 10, 5, 0, 45, 45))):
        p = built.default_params(20.0, mode)
        assert (p.patch_sz, p.search_sz_x, p.search_sz_t, p.npatches_x, p.npatches_t, p.npatches_tagg) == want
