"""The SIG argument of the sequence tools (a number | auto | vst | vst:A,B): seq_sig_parse of host/seq_args.c, the one
statement of the grammar, as a stand-alone program (tests/seq_sig_driver.c) built plain and under AddressSanitizer and
UBSan, and the three tools that read SIG through it on every refused form. No GPU: the grammar makes no device call,
and the tools refuse before they open a device."""
import os
import subprocess

import pytest

from test_cli import BIN, ROOT

NUMBER, AUTO, VST, VST_GIVEN = range(4)
# text -> (mode, a, b, sigma): what nlkalman-seq and nlkalman-y4m each made of it while each had its own copy of the
# grammar ("vst" prefix -> vst, the rest sscanf ":%f,%f"; "auto"; anything else atof)
ACCEPTED = {
    "20": (NUMBER, 0, 0, 20), "0": (NUMBER, 0, 0, 0), "-3": (NUMBER, 0, 0, -3), "auto": (AUTO, 0, 0, 0),
    "vst": (VST, 0, 0, 0), "vst:0.5,2": (VST_GIVEN, 0.5, 2, 0), "vst:0,1": (VST_GIVEN, 0, 1, 0),
    "vst:1,0": (VST_GIVEN, 1, 0, 0),
    # junk: a number is what atof reads (its leading part, 0 when there is none: "auto" must be the whole word),
    # sscanf stops after B
    "20abc": (NUMBER, 0, 0, 20), "abc": (NUMBER, 0, 0, 0), "autox": (NUMBER, 0, 0, 0), "": (NUMBER, 0, 0, 0),
    "vst:1,2junk": (VST_GIVEN, 1, 2, 0),
}
REFUSED = ["vst:", "vst:1", "vst:1,", "vst:-1,2", "vst:0,0", "vst:nan,1", "vst:3e38,3e38", "vstx"]
WANT = "%s: SIG = %s: want vst or vst:A,B with A, B >= 0, not both 0\n"


@pytest.fixture(scope="module")
def drivers(tmp_path_factory):
    """the driver with host/seq_args.c and nothing else, plain and under the sanitizers (their runtimes linked
    statically where the compiler has them: the program runs as it is, nothing is preloaded)"""
    d = tmp_path_factory.mktemp("seq_sig")
    src = [os.path.join(ROOT, "tests", "seq_sig_driver.c"), os.path.join(ROOT, "bwd-nlkalman_amd", "host", "seq_args.c")]
    inc = ["-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "bwd-nlkalman_amd", "host")]
    base = ["gcc", "-O1", "-g", "-std=gnu99", "-Wall", "-Werror", *inc, *src, "-o"]
    plain, san = str(d / "plain"), str(d / "san")
    subprocess.check_call(base + [plain])
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    for static in (["-static-libasan", "-static-libubsan"], []):
        if subprocess.run(base + [san, *flags, *static], capture_output=True).returncode == 0 and \
                subprocess.run([san], capture_output=True).returncode == 0:
            return [plain, san]
    return [plain]


def test_grammar(drivers):
    for exe in drivers:
        texts = list(ACCEPTED) + REFUSED
        r = subprocess.run([exe, *texts], capture_output=True, text=True, timeout=60)
        assert r.returncode == 0 and r.stderr == "", (exe, r)
        lines = r.stdout.splitlines()
        assert len(lines) == len(texts)
        for text, line in zip(texts, lines):
            f = line.split()
            mode, a, b, sigma, code = int(f[1]), float(f[3]), float(f[5]), float(f[7]), int(f[9])
            if text in ACCEPTED:
                assert (mode, a, b, sigma, code) == (*ACCEPTED[text], 0), (text, line)
            else:
                assert code == 1 and mode == VST_GIVEN, (text, line)


@pytest.mark.parametrize("tool", ["nlkalman-seq", "nlkalman-lsmo-seq", "nlkalman-y4m"])
def test_tools_refuse_under_their_own_name(built, tool, tmp_path):
    exe = os.path.join(BIN, tool)
    if not os.path.exists(exe):
        built.build()
    out, missing = tmp_path / "out", tmp_path / "missing.y4m"
    for text in REFUSED:
        # (the seq tools make OUT, the stream tool opens IN, before either opens a device: neither happens)
        args = [text, missing] if tool == "nlkalman-y4m" else [tmp_path / "%03d.tif", 1, 3, text, out]
        r = subprocess.run([exe, *map(str, args)], capture_output=True, text=True, timeout=60)
        assert (r.returncode, r.stdout, r.stderr) == (1, "", WANT % (tool, text)), (text, r)
        assert not out.exists()
