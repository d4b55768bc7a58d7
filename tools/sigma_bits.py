"""Dumps the raw bits of everything nlk_dev_estimate_sigma (sigma[1 + ch], counts) and nlk_dev_estimate_noise_curve
(curve[ch][2], every nlk_curve_bin) write, as JSON, so that two builds of the library can be held to each other bit
for bit (the parity tests allow 1e-4 and would not see a drift):

    python tools/sigma_bits.py --json A.json [--root DIR]     DIR: a tree whose bwd-nlkalman_amd/ holds the other build
    python tools/sigma_bits.py --compare A.json B.json        exit status 1 if an entry differs

Inputs: every PARITY case of tests/test_sigma.py and tests/test_noise_curve.py; the 256 x 192 x 3 accuracy frames at
step 4, 1, 6 (the last staged step) and 7 (the first unstaged one); the curve with 1, 16, 17 and 64 bins; a
1920 x 1080 x 3 frame made on the device with default parameters."""
import argparse
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def bits(x):
    return np.ascontiguousarray(x).view(np.uint32).reshape(-1).tolist()


def dump(root):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    sys.path.insert(0, os.path.abspath(root))
    pkg = importlib.import_module("bwd-nlkalman_amd")
    synth = importlib.import_module("bwd-nlkalman_amd.synth")
    import test_noise_curve as tc
    import test_sigma as ts
    if pkg.hip().nlk_device_count() < 1:
        raise SystemExit("sigma_bits: no HIP device")
    ctx = pkg.Context(0)
    out = {}

    def sigma(name, d, w, h, ch, **p):
        s, s_ch, counts = ctx.estimate_sigma(d, w, h, ch, **p)
        out["sigma " + name] = bits(np.array([s, *s_ch], np.float32)) + bits(counts)

    def curve(name, d, w, h, ch, **p):
        ab, bins = ctx.estimate_noise_curve(d, w, h, ch, **p)
        out["curve " + name] = bits(ab) + bits(bins)

    def both(name, d, w, h, ch, **p):
        sigma(name, d, w, h, ch, **p)
        curve(name, d, w, h, ch, **p)

    for mod, fn in ((ts, sigma), (tc, curve)):
        for case, (w, h, ch, holed, p) in zip(mod.PARITY_IDS, mod.PARITY):
            d = ctx.upload(mod._input(w, h, ch, holed))
            fn("parity " + case, d, w, h, ch, **p)
            ctx.free(d)
    frames = {"awgn 256x192x3": ts._accuracy_frame(20.0, 1), "affine 256x192x3": tc._accuracy_frame(tc.AB, 1),
              "awgn holed 96x64x3": ts._input(96, 64, 3, True), "affine holed 96x64x3": tc._input(96, 64, 3, True)}
    for name, im in frames.items():
        h, w, ch = im.shape
        d = ctx.upload(im)
        for step in (4, 1, 6, 7):
            both(f"{name} step {step}", d, w, h, ch, step=step)
        for nbins in (1, 16, 17, 64):
            curve(f"{name} nbins {nbins}", d, w, h, ch, nbins=nbins)
            curve(f"{name} nbins {nbins} step 1 nmin 1", d, w, h, ch, nbins=nbins, step=1, nmin=1)
        ctx.free(d)
    w, h, ch = 1920, 1080, 3
    clean = synth.clean_frame(w, h, ch)
    d_clean, d = ctx.upload(clean), ctx.alloc(clean.nbytes)
    ctx.awgn(d, d_clean, clean.size, 20.0, 1)
    both("awgn 1920x1080x3", d, w, h, ch)
    ctx.noise_affine(d, d_clean, clean.size, ch, tc.AB, 1)
    both("affine 1920x1080x3", d, w, h, ch)
    for nbins in (1, 17, 64):
        curve(f"affine 1920x1080x3 nbins {nbins}", d, w, h, ch, nbins=nbins)
    ctx.free(d)
    ctx.free(d_clean)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=ROOT)
    ap.add_argument("--json")
    ap.add_argument("--compare", nargs=2, metavar="JSON")
    a = ap.parse_args()
    if a.compare:
        x, y = (json.load(open(f)) for f in a.compare)
        names = sorted(set(x) | set(y))
        bad = [n for n in names if x.get(n) != y.get(n)]
        words = sum(len(v) for v in x.values())
        for n in bad:
            print("differs:", n)
        print(f"{len(names)} entries ({words} 32-bit words), {len(bad)} differ")
        raise SystemExit(1 if bad else 0)
    out = dump(a.root)
    with open(a.json, "w") as f:
        json.dump(out, f)
    print(f"sigma_bits: {len(out)} entries written to {a.json}")


if __name__ == "__main__":
    main()
