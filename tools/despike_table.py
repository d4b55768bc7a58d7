"""The table of DESIGN.md §9 "Defective pixels": what stuck sensor sites cost the recursion and what the ring-median
pre-filter of nlk_dev_despike gives back, on the CPU oracle (no GPU) from the numpy statement of the rule
(tests/despike_ref.py). Chain: TV-L1 -> mask 0.75 -> warp -> FLT1 -> FLT2, free running, default parameters, 96 x 64 x 3,
the 2 px/frame pan of synth.clean_frame, 4 frames, noise seeds 300 + t. 21 fixed sensor positions (0.3 %, three of them on
the border; despike_ref.defect_sites) are set to 255 (70 %) or 0 in every noisy frame; "despiked" is the rule at
thr = K sigma, K = 4, R = 1. The last rows plant 2 x 2 blobs instead (off the border) and despike at R = 2. All of it is
synthetic.

    python tools/despike_table.py"""
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import despike_ref as DR  # noqa: E402
import oracle as O        # noqa: E402

W, H, K = 96, 64, 4.0
SYNTH = importlib.import_module("bwd-nlkalman_amd.synth")


def fmt(v):
    return " ".join("%.2f" % x for x in v)


def rows(sigmas, blob, radius):
    sites = DR.defect_sites(W, H, blob=blob)
    for sigma in sigmas:
        thr = float(np.float32(K) * np.float32(sigma))
        clean, _, _ = DR.chain(O, SYNTH, sigma)
        bad, rb, _ = DR.chain(O, SYNTH, sigma, lambda a: DR.plant(a, sites, blob), sites=sites, blob=blob)
        fix, rf, _ = DR.chain(O, SYNTH, sigma, lambda a: DR.despike(DR.plant(a, sites, blob), thr, radius)[0],
                              sites=sites, blob=blob)
        lost, left = np.mean(clean[1:]) - np.mean(bad[1:]), np.mean(clean[1:]) - np.mean(fix[1:])
        what = "%d sites" % len(sites) if blob == 1 else "%d blobs of 2 × 2, R = 2" % len(sites)
        print("| %g | %s | %s | %s | %s | %.0f–%.0f / %.1f–%.1f | %.2f / %.2f |" % (
            sigma, what, fmt(clean), fmt(bad), fmt(fix), min(rb), max(rb), min(rf), max(rf), lost, left), flush=True)


def false_positives():
    """samples replaced on frames without defects: sigma 5 / 20 / 40, seeds 1..8, R = 1 and 2, K = 4"""
    n = total = 0
    for sigma in (5.0, 20.0, 40.0):
        for seed in range(1, 9):
            a = SYNTH.awgn(SYNTH.clean_frame(W, H, 3), sigma, seed)
            for r in (1, 2):
                n += int(DR.despike(a, float(np.float32(K) * np.float32(sigma)), r)[1].sum())
                total += a.size
    return n, total


def main():
    O.build()
    print("| σ | defects | flt2 PSNR of frames 0..3, clean sensor | with defects | with defects, despiked first | "
          "RMSE at the sites: defects / despiked | dB lost (mean of frames 1..3): defects / despiked |")
    print("|---|---|---|---|---|---|---|")
    rows((10.0, 20.0, 40.0), 1, 1)
    rows((10.0, 20.0), 2, 2)
    print("\nwithout defects the pre-filter replaced %d of %d samples (σ = 5 / 20 / 40, seeds 1..8, R = 1 and 2, K = 4)"
          % false_positives())


if __name__ == "__main__":
    main()
