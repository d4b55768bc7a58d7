"""The table of DESIGN.md §9 "A defect map learned over time": what stuck sensor sites cost the recursion over 24 frames
and what --despike alone, the defect map alone and both give back, on the CPU oracle (no GPU) from the numpy statements
of the rules (tests/despike_ref.py, tests/defectmap_ref.py). Chain: TV-L1 -> mask 0.75 -> warp -> FLT1 -> FLT2, free
running, default parameters, 96 x 64 x 3, the 2 px/frame pan of synth.clean_frame (static rows: frame 0 every time), 24
frames, the noise of frame t from np.random.default_rng(300 + t). 21 fixed sensor positions (despike_ref.defect_sites)
are set to 255 (70 %) or 0 in every noisy frame, single sites (R = 1) or 2 x 2 blobs (R = 2); despike at K = 4, the map
at K = 4, N = 32. Every figure: the flt2 PSNR averaged over frames 16..23 / the RMSE at the sites over the same frames.
All of it is synthetic.

    python tools/defectmap_table.py > profiles/defectmap_table.txt"""
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import defectmap_ref as DM  # noqa: E402
import despike_ref as DR    # noqa: E402
import oracle as O          # noqa: E402

W, H, K, NF, LAST = 96, 64, 4.0, 24, slice(16, 24)
SYNTH = importlib.import_module("bwd-nlkalman_amd.synth")


def run(sigma, static, sites=None, blob=1, k_map=None, k_despike=None):
    prep = DM.Cleaner(sigma, sites, blob, k_map, k_despike)
    ps, rm, _ = DM.chain(O, SYNTH, sigma, prep, NF, W, H, sites, blob, static)
    return float(np.mean(ps[LAST])), float(np.mean(rm[LAST])), prep.replaced


def main():
    O.build()
    print("| σ | scene | defects | clean sensor | defects | --despike 4[,2] | --defect-map 4[,2] | both | "
          "dB lost: defects / despike / map / both |")
    print("|---|---|---|---|---|---|---|---|---|")
    clean = {}
    for static in (False, True):
        for sigma in (10.0, 20.0, 40.0):
            clean[sigma, static] = run(sigma, static)
            for blob in ((1, 2) if not static else (1,)):
                sites = DR.defect_sites(W, H, blob=blob)
                bad = run(sigma, static, sites, blob)
                cols = [run(sigma, static, sites, blob, k_despike=K), run(sigma, static, sites, blob, k_map=K),
                        run(sigma, static, sites, blob, k_map=K, k_despike=K)]
                c = clean[sigma, static][0]
                print("| %g | %s | %s | %.2f | %.2f / %.1f | %s | %.2f / %.2f / %.2f / %.2f |" % (
                    sigma, "static" if static else "pan", "21 sites" if blob == 1 else "21 blobs of 2 × 2, R = 2", c,
                    bad[0], bad[1], " | ".join("%.2f / %.1f" % (p, r) for p, r, _ in cols), c - bad[0], c - cols[0][0],
                    c - cols[1][0], c - cols[2][0]), flush=True)
    print("\nclean sensor (no defects), the map alone at K = 4, N = 32: the flt2 PSNR of frames 16..23 without / with the "
          "map, and the samples it replaced on the 24 frames (of %d)" % (NF * W * H * 3))
    print("| σ | scene | R | without | with | replaced |")
    print("|---|---|---|---|---|---|")
    for static in (False, True):
        for sigma in (10.0, 20.0, 40.0):
            for blob in (1, 2):
                p, _, rep = run(sigma, static, None, blob, k_map=K)
                print("| %g | %s | %d | %.2f | %.2f | %d |" % (sigma, "static" if static else "pan", blob,
                                                              clean[sigma, static][0], p, sum(rep)), flush=True)


if __name__ == "__main__":
    main()
