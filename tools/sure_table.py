#!/usr/bin/env python3
"""The tables of DESIGN.md §9, "Error estimate without clean frames", measured on the CPU oracle (no GPU): the chain of
tests/sure_ref.py (block-matching flow restatement -> mask 0.75 -> warp -> FLT1 -> FLT2, the probe on the opponent-space
noisy frame, flow and warps reused) on synth.clean_frame(192, 128, 3, t), noise seeds 300 + t.

    python tools/sure_table.py [WxH[xNF]] [accuracy] [beta] [sigma] [bar]     (default: 192x128x3, all four;
                                                                             > profiles/sure_table.txt)

accuracy  MSE_hat / true MSE of flt2 per frame, eps / sigma x sigma
beta      both beta of both iterations scaled: true and estimated mean of 3 frames at sigma = 20
sigma     the x1 run of `beta` with the formula given sigma = 19 / 20 / 21
bar       per-frame |MSE_hat - true| of flt2 over sigma x 3 noise seeds x 3 probe seeds: what sets the bar of
          tests/test_sure.py (twice the worst at sigma = 20, first frames and later frames each)"""
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import bmflow_ref as BR  # noqa: E402
import oracle as O  # noqa: E402
import sure_ref as S  # noqa: E402

W, H, CH, NF = 192, 128, 3, 3
SIGMAS = (10.0, 20.0, 40.0)


def flow(a, b):
    return BR.flow(a, b, fscale=1, radius=2)


def run(synth, sigma, **kw):
    return S.chain(O, synth, lambda t: synth.clean_frame(W, H, CH, t), sigma, flow, nf=NF, **kw)


def accuracy(synth):
    print("accuracy: flt2, MSE_hat / true MSE per frame t = 0, 1, ... (probe seed 0)")
    for er in (0.025, 0.05, 0.1, 0.2):
        row = []
        for sigma in SIGMAS:
            r = run(synth, sigma, eps_rel=er)
            row.append(", ".join("%.1f/%.1f" % (x["est2"][0]["mse"], x["true2"]) for x in r))
        print("  eps/sigma %-5g | %s" % (er, " | ".join("sigma %g: %s" % (s, v) for s, v in zip(SIGMAS, row))))
    n = W * H * CH
    print("  SURE's own s.d. sigma^2 sqrt(2 / N), N = %d: %s" % (n, ", ".join("%.1f" % (s * s * np.sqrt(2.0 / n)) for s in SIGMAS)))


def beta(synth):
    print("beta: both beta of both iterations scaled, sigma = 20, eps/sigma = %g, mean of %d frames (flt2)" % (S.EPS_REL, NF))
    for k in (0.25, 0.5, 1.0, 2.0, 4.0):
        r = run(synth, 20.0, beta=k)
        print("  x%-4g true %.1f  SURE %.1f  div %.4f" % (k, np.mean([x["true2"] for x in r]),
                                                       np.mean([x["est2"][0]["mse"] for x in r]),
                                                       np.mean([x["est2"][0]["div"] for x in r])))


def misstated(synth):
    print("sigma: true sigma = 20, the formula given 19 / 20 / 21 (flt2, mean of %d frames)" % NF)
    for k in (1.0, 4.0):
        vals = []
        for said in (19.0, 20.0, 21.0):
            r = run(synth, 20.0, beta=k, sigma_stated=said)
            vals.append(np.mean([x["est2"][0]["mse"] for x in r]))
        print("  beta x%g: %s" % (k, " / ".join("%.1f" % v for v in vals)))


def bar(synth):
    print("bar: flt2, |MSE_hat - true| per frame, noise seeds 300 / 400 / 500 + t, probe seeds 0 / 1 / 2, eps/sigma = %g" % S.EPS_REL)
    for sigma in SIGMAS:
        first, later, tr0, tr = [], [], [], []
        for ns in (300, 400, 500):
            r = run(synth, sigma, seeds=(0, 1, 2), noise_seed=ns)
            for t, x in enumerate(r):
                (first if t == 0 else later).extend(abs(e["mse"] - x["true2"]) for e in x["est2"])
                (tr0 if t == 0 else tr).append(x["true2"])
        print("  sigma %g: first frames worst %.3f (true %.1f .. %.1f), later frames worst %.3f (true %.1f .. %.1f)"
              % (sigma, max(first), min(tr0), max(tr0), max(later), min(tr), max(tr)))
        print("            twice the worst as a ratio of the smallest true MSE: first %.3f dB, later %.3f dB"
              % (10 * np.log10(1 + 2 * max(first) / min(tr0)), 10 * np.log10(1 + 2 * max(later) / min(tr))))


def main():
    O.build()
    synth = importlib.import_module("bwd-nlkalman_amd.synth")
    parts = dict(accuracy=accuracy, beta=beta, sigma=misstated, bar=bar)
    args = sys.argv[1:]
    if args and args[0][0].isdigit():
        global W, H, NF
        W, H, NF = (list(map(int, args[0].split("x"))) + [NF])[:3]
        args = args[1:]
    print("# %d x %d x %d, %d frames" % (W, H, CH, NF))
    for name in (args or list(parts)):
        parts[name](synth)
        sys.stdout.flush()


if __name__ == "__main__":
    main()
