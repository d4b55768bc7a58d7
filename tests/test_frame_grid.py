"""The one C statement of a frame call's patch grid and of its split into row strips: nlk_frame_grid and nlk_strip_plan
(include/nlk_hip.h, bwd-nlkalman_amd/host/frame_grid.c), which the frame pipeline, csrc/strips.hip and host/multidev.c
share. No GPU.

The strip plan against strips.strip_plan (the Python statement, which imports no backend) field by field, through the
built library and as a stand-alone program (tests/frame_grid_driver.c, plain and under AddressSanitizer and UBSan); the
grid against its formulas written out here."""
import importlib
import itertools
import os
import subprocess

import pytest

from test_cli import ROOT

HS = (8, 13, 33, 64, 96, 135, 168, 400, 1080)
PSZS = (2, 4, 5, 7, 8, 12, 16)
HALOS = (0, 3, 5, 10, 15)
WORLDS = (1, 2, 3, 4, 8)


@pytest.fixture(scope="module")
def strips():
    return importlib.import_module("bwd-nlkalman_amd.strips")


def _grid_with_halo(built, h, psz, halo):
    """a first frame's grid whose halo is the spatial radius (one patch wide: the plan reads no ngx)"""
    g = built.frame_grid(psz, h, built.Params(patch_sz=psz, search_sz_x=halo, search_sz_t=0))
    assert (g.psz, g.step, g.halo) == (psz, psz // 2, halo)
    return g


def _py_outcome(strips, h, psz, halo, world):
    """strips.strip_plan's plan, or which of its two refusals it raised"""
    try:
        return strips.strip_plan(h, psz, halo, world)
    except ValueError as e:
        few, thin = "cannot be split over" in str(e), "thinner than the search halo" in str(e)
        assert few != thin, e
        return "few" if few else "thin"


def test_strip_plan_equals_strips_py_over_the_sweep(built, strips):
    counts = {"plan": 0, "few": 0, "thin": 0}
    for h, psz, halo, world in itertools.product(HS, PSZS, HALOS, WORLDS):
        if h < psz:
            continue
        want = _py_outcome(strips, h, psz, halo, world)
        try:
            got = built.strip_plan(h, _grid_with_halo(built, h, psz, halo), world)
        except ValueError as e:
            got = {built.STRIPS_FEW_ROWS: "few", built.STRIPS_THIN: "thin"}[e.args[1]]
        assert got == want, (h, psz, halo, world)
        counts[want if isinstance(want, str) else "plan"] += 1
    assert counts == {"plan": 1199, "few": 150, "thin": 151}   # (all three outcomes, 1500 cases)


def test_frame_grid_equals_its_formulas(built):
    n = 0
    for w, h, psz in itertools.product(HS, HS, PSZS):
        if w < psz or h < psz:
            continue
        for smoother, have_prev, (rx, rt) in itertools.product((0, 1), (0, 1), ((10, 5), (5, 10), (3, 3))):
            g = built.frame_grid(w, h, built.Params(patch_sz=psz, search_sz_x=rx, search_sz_t=rt), smoother, have_prev)
            step = psz // 2
            want = (psz, step, (w - psz) // step + 1, (h - psz) // step + 1, rt if smoother else max(rx, rt),
                    (rt if (smoother or have_prev) else rx) // step)
            assert (g.psz, g.step, g.ngx, g.ngy, g.halo, g.reach) == want, (w, h, psz, smoother, have_prev, rx, rt)
            n += 1
    assert n > 5000


@pytest.mark.parametrize("w,h,psz", [(64, 64, 1), (64, 64, 0), (7, 64, 8), (64, 7, 8), (3, 3, 4)])
def test_frame_grid_refuses_and_writes_nothing(built, w, h, psz):
    import ctypes as C
    g = built.FrameGrid(-7, -7, -7, -7, -7, -7)
    p = built.Params(patch_sz=psz, search_sz_x=10, search_sz_t=5)
    assert built.hip().nlk_frame_grid(w, h, C.byref(p), 0, 0, C.byref(g)) == -3   # NLK_EINVAL
    assert [getattr(g, k) for k, _ in g._fields_] == [-7] * 6
    with pytest.raises(ValueError):
        built.frame_grid(w, h, p)


# ---------------------------------------------------------------- the stand-alone program

SHAPES = [(8, 8, 0), (13, 5, 3), (33, 4, 10), (64, 8, 10), (135, 7, 5), (168, 8, 5), (400, 12, 15), (1080, 8, 10),
          (1080, 16, 3), (96, 2, 0)]   # (h, psz, halo)


@pytest.fixture(scope="module")
def drivers(tmp_path_factory):
    """tests/frame_grid_driver.c with host/frame_grid.c and nothing else, plain and under the sanitizers (their runtimes
    linked statically where the compiler has them: the program runs as it is, nothing is preloaded)"""
    d = tmp_path_factory.mktemp("frame_grid")
    src = [os.path.join(ROOT, "tests", "frame_grid_driver.c"), os.path.join(ROOT, "bwd-nlkalman_amd", "host", "frame_grid.c")]
    base = ["gcc", "-O1", "-g", "-std=gnu99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), *src, "-o"]
    plain, san = str(d / "plain"), str(d / "san")
    subprocess.check_call(base + [plain])
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    for static in (["-static-libasan", "-static-libubsan"], []):
        if subprocess.run(base + [san, *flags, *static], capture_output=True).returncode == 0 and \
                subprocess.run([san], capture_output=True).returncode == 0:
            return [plain, san]
    return [plain]


def test_driver_plans_worlds_1_to_64_like_strips_py(drivers, strips):
    args = [str(v) for shape in SHAPES for v in shape]
    for exe in drivers:
        r = subprocess.run([exe, *args], capture_output=True, text=True, timeout=60)
        assert r.returncode == 0 and r.stderr == "", (exe, r.returncode, r.stderr)
        lines = iter(r.stdout.splitlines())
        seen = set()
        for (h, psz, halo), world in itertools.product(SHAPES, range(1, 65)):
            head = next(lines).split()
            assert head[:8] == ["h", str(h), "psz", str(psz), "halo", str(halo), "world", str(world)], head
            want = _py_outcome(strips, h, psz, halo, world)
            code = int(head[9])
            if isinstance(want, str):
                assert code == {"few": 1, "thin": 2}[want], (h, psz, halo, world, code)
            else:
                assert code == 0, (h, psz, halo, world, code)
                got = [dict(zip(("gy0", "gy1", "Y0", "Y1", "own0", "own1"), map(int, next(lines).split()))) for _ in range(world)]
                assert got == want, (h, psz, halo, world)
            seen.add(code)
        assert next(lines, None) is None and seen == {0, 1, 2}
