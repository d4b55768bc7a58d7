"""The plan of a TV-L1 flow call's pyramid levels, pinned: nlk_host_tvl1_plan (include/nlk_hip.h) runs the parameter check
and the scratch layout walk of nlk_dev_tvl1_flow and the level planner (nlk_tv_plan, csrc/tu_tvl1.hip) without a context
or a device. No GPU.

A wrong level shape computes the same flow more slowly, and every flow test is bit-exact, so nothing else notices one.
PLANS holds, for inputs that reach every branch of the planner, every field of every level as the commit BEFORE the
planner existed computed it (a993891: its lines of tv_scale and of nlk_dev_tvl1_flow's pyramid loop, lifted verbatim
into a scratch program that printed these rows) - recorded, never produced by the code under test. The rows of the
retired variables are that commit's rows with nothing set (NLK_TV_SHAPE=3: with NLK_TV_SHAPE=0), the one intended
difference. What profiles/tvl1_plan_refactor.txt says about the sweep of random level sizes is the wide check; this
table is the one that stays."""
import ctypes as C

import pytest

FIELDS = ("nx", "ny", "solved", "driver", "threads", "shape", "tw", "th", "gx", "gy", "inline", "look")
WG, BLOCKED, PLAIN = 0, 1, 2
SWITCHES = ("NLK_TV_WG_PIXELS", "NLK_TV_UNBLOCKED", "NLK_TV_SHAPE", "NLK_TV_INLINE", "NLK_TV_LOOK")
RETIRED = ("NLK_TV_DEEP", "NLK_TV_MID", "NLK_TV_WG_FULL", "NLK_TV_LOOK2", "NLK_TV_BATCH")
EINVAL = -3

# (id, w, h, nscales (None: the count nlk_tvl1_scales gives), fscale, zfactor, switches,
#  one tuple of FIELDS per level, finest first - or the flow call's error code)
# Tiles: 99 / 108 and 380 / 400 are tiles of 64 x 16, 496 / 512 tiles of 64 x 32, 600 / 620 workgroups of the chosen shape.
PLANS = [
    ("1080p", 1920, 1080, None, 0, 0.5, {},
     ((1920, 1080, 1, 1, 512, 2, 64, 32, 30, 34, 0, 4),
      (960, 540, 1, 1, 1024, 1, 64, 32, 15, 17, 1, 4),
      (480, 270, 1, 1, 1024, 0, 64, 16, 8, 17, 1, 4),
      (240, 135, 1, 1, 576, 4, 16, 16, 15, 9, 1, 4),
      (120, 68, 1, 1, 576, 4, 16, 16, 8, 5, 1, 4),
      (60, 34, 1, 0, 1024, 0, 0, 0, 0, 0, 0, 0),
      (30, 17, 1, 0, 512, 0, 0, 0, 0, 0, 0, 0),
      (15, 9, 1, 0, 192, 0, 0, 0, 0, 0, 0, 0))),
    ("1080p-fscale1", 1920, 1080, None, 1, 0.5, {},
     ((1920, 1080, 0, 1, 512, 2, 64, 32, 30, 34, 0, 4),
      (960, 540, 1, 1, 1024, 1, 64, 32, 15, 17, 1, 4),
      (480, 270, 1, 1, 1024, 0, 64, 16, 8, 17, 1, 4),
      (240, 135, 1, 1, 576, 4, 16, 16, 15, 9, 1, 4),
      (120, 68, 1, 1, 576, 4, 16, 16, 8, 5, 1, 4),
      (60, 34, 1, 0, 1024, 0, 0, 0, 0, 0, 0, 0),
      (30, 17, 1, 0, 512, 0, 0, 0, 0, 0, 0, 0),
      (15, 9, 1, 0, 192, 0, 0, 0, 0, 0, 0, 0))),
    ("2160p", 3840, 2160, None, 0, 0.5, {},
     ((3840, 2160, 1, 1, 512, 2, 64, 32, 60, 68, 0, 4),
      (1920, 1080, 1, 1, 512, 2, 64, 32, 30, 34, 0, 4),
      (960, 540, 1, 1, 1024, 1, 64, 32, 15, 17, 1, 4),
      (480, 270, 1, 1, 1024, 0, 64, 16, 8, 17, 1, 4),
      (240, 135, 1, 1, 576, 4, 16, 16, 15, 9, 1, 4),
      (120, 68, 1, 1, 576, 4, 16, 16, 8, 5, 1, 4),
      (60, 34, 1, 0, 1024, 0, 0, 0, 0, 0, 0, 0),
      (30, 17, 1, 0, 512, 0, 0, 0, 0, 0, 0, 0),
      (15, 9, 1, 0, 192, 0, 0, 0, 0, 0, 0, 0))),
    ("1000x700", 1000, 700, None, 0, 0.5, {},
     ((1000, 700, 1, 1, 1024, 1, 64, 32, 16, 22, 1, 4),
      (500, 350, 1, 1, 1024, 0, 64, 16, 8, 22, 1, 4),
      (250, 175, 1, 1, 576, 4, 16, 16, 16, 11, 1, 4),
      (125, 88, 1, 1, 576, 4, 16, 16, 8, 6, 1, 4),
      (63, 44, 1, 1, 576, 4, 16, 16, 4, 3, 1, 4),
      (32, 22, 1, 0, 704, 0, 0, 0, 0, 0, 0, 0),
      (16, 11, 1, 0, 192, 0, 0, 0, 0, 0, 0, 0))),
    ("200x150", 200, 150, None, 0, 0.5, {},
     ((200, 150, 1, 1, 576, 4, 16, 16, 13, 10, 1, 4),
      (100, 75, 1, 1, 576, 4, 16, 16, 7, 5, 1, 4),
      (50, 38, 1, 0, 1024, 0, 0, 0, 0, 0, 0, 0),
      (25, 19, 1, 0, 512, 0, 0, 0, 0, 0, 0, 0))),
    ("131x97", 131, 97, None, 0, 0.5, {},
     ((131, 97, 1, 1, 576, 4, 16, 16, 9, 7, 1, 4),
      (66, 49, 1, 1, 576, 4, 16, 16, 5, 4, 1, 4),
      (33, 25, 1, 0, 832, 0, 0, 0, 0, 0, 0, 0),
      (17, 13, 1, 0, 256, 0, 0, 0, 0, 0, 0, 0))),
    ("16x16", 16, 16, None, 0, 0.5, {},
     ((16, 16, 1, 0, 256, 0, 0, 0, 0, 0, 0, 0),)),
    ("level-60x35-2100px", 60, 35, 1, 0, 0.5, {},
     ((60, 35, 1, 0, 1024, 0, 0, 0, 0, 0, 0, 0),)),
    ("level-61x35-2135px", 61, 35, 1, 0, 0.5, {},
     ((61, 35, 1, 1, 576, 4, 16, 16, 4, 3, 1, 4),)),
    ("level-64x15-960px", 64, 15, 1, 0, 0.5, {},
     ((64, 15, 1, 0, 960, 0, 0, 0, 0, 0, 0, 0),)),
    ("level-32x32-1024px", 32, 32, 1, 0, 0.5, {},
     ((32, 32, 1, 0, 1024, 0, 0, 0, 0, 0, 0, 0),)),
    ("level-41x25-1025px", 41, 25, 1, 0, 0.5, {},
     ((41, 25, 1, 0, 1024, 0, 0, 0, 0, 0, 0, 0),)),
    ("level-576x176-99tiles", 576, 176, 1, 0, 0.5, {},
     ((576, 176, 1, 1, 576, 4, 16, 16, 36, 11, 1, 4),)),
    ("level-576x177-108tiles", 576, 177, 1, 0, 0.5, {},
     ((576, 177, 1, 1, 1024, 0, 64, 16, 9, 12, 1, 4),)),
    ("level-1280x304-380tiles", 1280, 304, 1, 0, 0.5, {},
     ((1280, 304, 1, 1, 1024, 0, 64, 16, 20, 19, 1, 4),)),
    ("level-1280x305-400tiles", 1280, 305, 1, 0, 0.5, {},
     ((1280, 305, 1, 1, 1024, 1, 64, 32, 20, 10, 1, 4),)),
    ("level-1024x992-496tall", 1024, 992, 1, 0, 0.5, {},
     ((1024, 992, 1, 1, 1024, 1, 64, 32, 16, 31, 1, 4),)),
    ("level-1024x993-512tall", 1024, 993, 1, 0, 0.5, {},
     ((1024, 993, 1, 1, 512, 2, 64, 32, 16, 32, 1, 4),)),
    ("level-1280x960-600wg", 1280, 960, 1, 0, 0.5, {},
     ((1280, 960, 1, 1, 512, 2, 64, 32, 20, 30, 1, 4),)),
    ("level-1280x961-620wg", 1280, 961, 1, 0, 0.5, {},
     ((1280, 961, 1, 1, 512, 2, 64, 32, 20, 31, 0, 4),)),
    ("shape0", 200, 150, None, 0, 0.5, {'NLK_TV_SHAPE': '0'},
     ((200, 150, 1, 1, 1024, 0, 64, 16, 4, 10, 1, 4),
      (100, 75, 1, 1, 1024, 0, 64, 16, 2, 5, 1, 4),
      (50, 38, 1, 0, 1024, 0, 0, 0, 0, 0, 0, 0),
      (25, 19, 1, 0, 512, 0, 0, 0, 0, 0, 0, 0))),
    ("shape1", 200, 150, None, 0, 0.5, {'NLK_TV_SHAPE': '1'},
     ((200, 150, 1, 1, 1024, 1, 64, 32, 4, 5, 1, 4),
      (100, 75, 1, 1, 1024, 1, 64, 32, 2, 3, 1, 4),
      (50, 38, 1, 0, 1024, 0, 0, 0, 0, 0, 0, 0),
      (25, 19, 1, 0, 512, 0, 0, 0, 0, 0, 0, 0))),
    ("shape2", 200, 150, None, 0, 0.5, {'NLK_TV_SHAPE': '2'},
     ((200, 150, 1, 1, 512, 2, 64, 32, 4, 5, 1, 4),
      (100, 75, 1, 1, 512, 2, 64, 32, 2, 3, 1, 4),
      (50, 38, 1, 0, 1024, 0, 0, 0, 0, 0, 0, 0),
      (25, 19, 1, 0, 512, 0, 0, 0, 0, 0, 0, 0))),
    ("shape4", 200, 150, None, 0, 0.5, {'NLK_TV_SHAPE': '4'},
     ((200, 150, 1, 1, 576, 4, 16, 16, 13, 10, 1, 4),
      (100, 75, 1, 1, 576, 4, 16, 16, 7, 5, 1, 4),
      (50, 38, 1, 0, 1024, 0, 0, 0, 0, 0, 0, 0),
      (25, 19, 1, 0, 512, 0, 0, 0, 0, 0, 0, 0))),
    ("shape7", 200, 150, None, 0, 0.5, {'NLK_TV_SHAPE': '7'},
     ((200, 150, 1, 1, 1024, 0, 64, 16, 4, 10, 1, 4),
      (100, 75, 1, 1, 1024, 0, 64, 16, 2, 5, 1, 4),
      (50, 38, 1, 0, 1024, 0, 0, 0, 0, 0, 0, 0),
      (25, 19, 1, 0, 512, 0, 0, 0, 0, 0, 0, 0))),
    ("inline0", 200, 150, None, 0, 0.5, {'NLK_TV_INLINE': '0'},
     ((200, 150, 1, 1, 576, 4, 16, 16, 13, 10, 0, 4),
      (100, 75, 1, 1, 576, 4, 16, 16, 7, 5, 0, 4),
      (50, 38, 1, 0, 1024, 0, 0, 0, 0, 0, 0, 0),
      (25, 19, 1, 0, 512, 0, 0, 0, 0, 0, 0, 0))),
    ("look1", 200, 150, None, 0, 0.5, {'NLK_TV_LOOK': '1'},
     ((200, 150, 1, 1, 576, 4, 16, 16, 13, 10, 1, 1),
      (100, 75, 1, 1, 576, 4, 16, 16, 7, 5, 1, 1),
      (50, 38, 1, 0, 1024, 0, 0, 0, 0, 0, 0, 0),
      (25, 19, 1, 0, 512, 0, 0, 0, 0, 0, 0, 0))),
    ("wg-pixels0", 200, 150, None, 0, 0.5, {'NLK_TV_WG_PIXELS': '0'},
     ((200, 150, 1, 1, 576, 4, 16, 16, 13, 10, 1, 4),
      (100, 75, 1, 1, 576, 4, 16, 16, 7, 5, 1, 4),
      (50, 38, 1, 1, 576, 4, 16, 16, 4, 3, 1, 4),
      (25, 19, 1, 1, 576, 4, 16, 16, 2, 2, 1, 4))),
    ("wg-pixels5000", 200, 150, None, 0, 0.5, {'NLK_TV_WG_PIXELS': '5000'},
     ((200, 150, 1, 1, 576, 4, 16, 16, 13, 10, 1, 4),
      (100, 75, 1, 1, 576, 4, 16, 16, 7, 5, 1, 4),
      (50, 38, 1, 0, 1024, 0, 0, 0, 0, 0, 0, 0),
      (25, 19, 1, 0, 512, 0, 0, 0, 0, 0, 0, 0))),
    ("unblocked", 200, 150, None, 0, 0.5, {'NLK_TV_UNBLOCKED': '1'},
     ((200, 150, 1, 2, 0, 0, 0, 0, 4, 38, 0, 0),
      (100, 75, 1, 2, 0, 0, 0, 0, 2, 19, 0, 0),
      (50, 38, 1, 0, 1024, 0, 0, 0, 0, 0, 0, 0),
      (25, 19, 1, 0, 512, 0, 0, 0, 0, 0, 0, 0))),
    ("retired-1080p", 1920, 1080, None, 0, 0.5, {'NLK_TV_DEEP': '1', 'NLK_TV_MID': '0', 'NLK_TV_WG_FULL': '1', 'NLK_TV_LOOK2': '1', 'NLK_TV_BATCH': '3'},
     ((1920, 1080, 1, 1, 512, 2, 64, 32, 30, 34, 0, 4),
      (960, 540, 1, 1, 1024, 1, 64, 32, 15, 17, 1, 4),
      (480, 270, 1, 1, 1024, 0, 64, 16, 8, 17, 1, 4),
      (240, 135, 1, 1, 576, 4, 16, 16, 15, 9, 1, 4),
      (120, 68, 1, 1, 576, 4, 16, 16, 8, 5, 1, 4),
      (60, 34, 1, 0, 1024, 0, 0, 0, 0, 0, 0, 0),
      (30, 17, 1, 0, 512, 0, 0, 0, 0, 0, 0, 0),
      (15, 9, 1, 0, 192, 0, 0, 0, 0, 0, 0, 0))),
    ("retired-200x150", 200, 150, None, 0, 0.5, {'NLK_TV_DEEP': '1', 'NLK_TV_MID': '0', 'NLK_TV_WG_FULL': '1', 'NLK_TV_LOOK2': '1', 'NLK_TV_BATCH': '3'},
     ((200, 150, 1, 1, 576, 4, 16, 16, 13, 10, 1, 4),
      (100, 75, 1, 1, 576, 4, 16, 16, 7, 5, 1, 4),
      (50, 38, 1, 0, 1024, 0, 0, 0, 0, 0, 0, 0),
      (25, 19, 1, 0, 512, 0, 0, 0, 0, 0, 0, 0))),
    ("retired-shape3", 200, 150, None, 0, 0.5, {'NLK_TV_SHAPE': '3'},
     ((200, 150, 1, 1, 1024, 0, 64, 16, 4, 10, 1, 4),
      (100, 75, 1, 1, 1024, 0, 64, 16, 2, 5, 1, 4),
      (50, 38, 1, 0, 1024, 0, 0, 0, 0, 0, 0, 0),
      (25, 19, 1, 0, 512, 0, 0, 0, 0, 0, 0, 0))),
    ("refused-nscales0", 200, 150, 0, 0, 0.5, {},
     -3),
    ("refused-nscales65", 200, 150, 65, 0, 0.5, {},
     -3),
    ("refused-zfactor1", 200, 150, 3, 0, 1.0, {},
     -3),
    ("refused-w1", 1, 150, 1, 0, 0.5, {},
     -3),
    ("refused-level-below-2", 16, 16, 5, 0, 0.5, {},
     -3),
]
BY_ID = {row[0]: row for row in PLANS}


def _params(built, row):
    _, w, h, ns, fscale, zfactor, _, _ = row
    p = built.Tvl1Params()
    built.hip().nlk_tvl1_default_params(C.byref(p))
    p.fscale, p.zfactor = fscale, zfactor
    p.nscales = built.hip().nlk_tvl1_scales(w, h, p.nscales, p.zfactor) if ns is None else ns
    return p


def _plan(built, monkeypatch, row):
    for name in SWITCHES + RETIRED:
        monkeypatch.delenv(name, raising=False)
    for name, value in row[6].items():
        monkeypatch.setenv(name, value)
    return built.host_tvl1_plan(row[1], row[2], _params(built, row))


def test_table_is_well_formed():
    assert len(PLANS) >= 38 and len(BY_ID) == len(PLANS)
    assert all(isinstance(r[7], int) or all(len(level) == len(FIELDS) for level in r[7]) for r in PLANS)


@pytest.mark.parametrize("row", PLANS, ids=[r[0] for r in PLANS])
def test_tvl1_plan_is_the_recorded_one(built, monkeypatch, row):
    want = row[7]
    if isinstance(want, int):  # refused like the flow call refuses it
        with pytest.raises(built.NlkError) as e:
            _plan(built, monkeypatch, row)
        assert e.value.args[1] == want and "nlk_dev_tvl1_flow" in e.value.args[0]
        return
    got = _plan(built, monkeypatch, row)
    assert all(tuple(level) == FIELDS == built.TVL1_PLAN_FIELDS for level in got)
    assert [tuple(level.values()) for level in got] == list(want)


def test_refused_inputs_write_nothing(built, monkeypatch):
    """... and room for fewer levels than the pyramid has is refused too"""
    n = len(FIELDS)
    for id_ in ("refused-nscales0", "refused-nscales65", "refused-zfactor1", "refused-w1", "refused-level-below-2"):
        row = BY_ID[id_]
        out, levels = (C.c_int * (64 * n))(*([-77] * (64 * n))), C.c_int(-77)
        assert built.hip().nlk_host_tvl1_plan(row[1], row[2], C.byref(_params(built, row)), 64, out, C.byref(levels)) == EINVAL
        assert set(out) == {-77} and levels.value == -77
    row = BY_ID["1080p"]
    p = _params(built, row)
    assert p.nscales == len(row[7]) == 8
    out, levels = (C.c_int * (8 * n))(*([-77] * (8 * n))), C.c_int(-77)
    assert built.hip().nlk_host_tvl1_plan(1920, 1080, C.byref(p), 7, out, C.byref(levels)) == EINVAL
    assert set(out) == {-77} and levels.value == -77
    assert built.hip().nlk_host_tvl1_plan(1920, 1080, C.byref(p), 8, out, C.byref(levels)) == 0
    assert levels.value == 8 and tuple(out) == sum(row[7], ())
    assert built.hip().nlk_host_tvl1_plan(1920, 1080, None, 8, out, C.byref(levels)) == EINVAL


def test_retired_switches_are_ignored(built, monkeypatch):
    """NLK_TV_DEEP, _MID, _WG_FULL, _LOOK2, _BATCH: set variables change nothing; NLK_TV_SHAPE=3 (64 x 16 tiles at 512
    threads, retired) is out of range like 7"""
    for with_it, without in (("retired-1080p", "1080p"), ("retired-200x150", "200x150"), ("retired-shape3", "shape0"),
                             ("shape7", "shape0")):
        assert BY_ID[with_it][7] == BY_ID[without][7]
        assert _plan(built, monkeypatch, BY_ID[with_it]) == _plan(built, monkeypatch, BY_ID[without])
    assert set(BY_ID["retired-1080p"][6]) == set(RETIRED)


def test_branches_the_table_reaches():
    """the rows are the issue's: every branch of the planner has one, both sides of every threshold"""
    f = {r[0]: [dict(zip(FIELDS, level)) for level in r[7]] for r in PLANS if not isinstance(r[7], int)}
    p = f["1080p"]  # 1080p alone reaches every default path
    assert [(v["nx"], v["ny"]) for v in p] == [(1920, 1080), (960, 540), (480, 270), (240, 135), (120, 68), (60, 34), (30, 17), (15, 9)]
    assert [(v["driver"], v["shape"], v["inline"]) for v in p[:5]] == [(BLOCKED, 2, 0), (BLOCKED, 1, 1), (BLOCKED, 0, 1), (BLOCKED, 4, 1), (BLOCKED, 4, 1)]
    assert [(v["driver"], v["threads"]) for v in p[5:]] == [(WG, 1024), (WG, 512), (WG, 192)]
    assert [v["solved"] for v in f["1080p-fscale1"]] == [0] + [1] * 7 and all(v["solved"] for v in p)
    one = {k: v[0] for k, v in f.items() if k.startswith("level-")}
    assert (one["level-60x35-2100px"]["driver"], one["level-61x35-2135px"]["driver"]) == (WG, BLOCKED)
    assert [one[k]["threads"] for k in ("level-64x15-960px", "level-32x32-1024px", "level-41x25-1025px")] == [960, 1024, 1024]
    assert (one["level-576x176-99tiles"]["shape"], one["level-576x177-108tiles"]["shape"]) == (4, 0)
    assert (one["level-1280x304-380tiles"]["shape"], one["level-1280x305-400tiles"]["shape"]) == (0, 1)
    assert (one["level-1024x992-496tall"]["shape"], one["level-1024x993-512tall"]["shape"]) == (1, 2)
    assert (one["level-1280x960-600wg"]["inline"], one["level-1280x961-620wg"]["inline"]) == (1, 0)
    assert [f[f"shape{s}"][0]["shape"] for s in (0, 1, 2, 4, 7)] == [0, 1, 2, 4, 0]
    assert [(v["tw"], v["th"], v["threads"]) for v in (f[f"shape{s}"][0] for s in (0, 1, 2, 4))] == \
        [(64, 16, 1024), (64, 32, 1024), (64, 32, 512), (16, 16, 576)]
    assert f["inline0"][0]["inline"] == 0 and f["look1"][0]["look"] == 1 and f["200x150"][0]["look"] == 4
    assert all(v["driver"] == BLOCKED for v in f["wg-pixels0"]) and f["wg-pixels5000"] == f["200x150"]  # (clamped to 2100)
    assert [v["driver"] for v in f["unblocked"]] == [PLAIN, PLAIN, WG, WG]
    assert (f["unblocked"][0]["gx"], f["unblocked"][0]["gy"]) == (4, 38)  # 64 x 4 pixels per workgroup
