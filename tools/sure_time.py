"""Times the error estimate without clean frames (nlk_dev_probe_add, nlk_dev_sure_terms, SequenceFilter(sure=True)) at
1080p RGB, with HIP events after a clock-settle phase (as tools/bmflow_time.py). The variants alternate inside one
process, round after round, so that the spread of each is seen next to the difference between them:

  - nlk_dev_probe_add (out of place and in place) and nlk_dev_sure_terms (tiles of 4, 16 and 64, with and without the
    map) beside nlk_dev_sqdiff_sum, the one-pass helper that reads two of the three images;
  - one SequenceFilter step (push of a temporal frame) with sure=True beside the step without it, over a cycle of four
    distinct frames of a pan pushed in order (bench.py's S1 does the same). The step with the estimate also downloads
    its terms and its map, so it ends with a wait for the device.

    python tools/sure_time.py [--iters N] [--step-iters N] [--rounds N] [--json FILE]  > profiles/sure_time.txt"""
import argparse
import importlib
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from bmflow_time import CH, H, NFR, SIGMA, W, noisy_frame, timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200, help="kernel calls per timed window")
    ap.add_argument("--step-iters", type=int, default=24, help="steps per timed window (whole cycles of 4 frames)")
    ap.add_argument("--rounds", type=int, default=3, help="alternating rounds of every comparison")
    ap.add_argument("--settle", type=float, default=1.0, help="seconds of back-to-back calls before timing")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    pkg = importlib.import_module("bwd-nlkalman_amd")
    synth = importlib.import_module("bwd-nlkalman_amd.synth")
    seq = importlib.import_module("bwd-nlkalman_amd.sequence")
    if pkg.hip().nlk_device_count() < 1:
        raise SystemExit("sure_time: no HIP device (there is nothing to time without one)")
    ctx = pkg.Context(0)
    stream = torch.cuda.Stream()
    ctx.set_stream(stream.cuda_stream)
    base = synth.clean_frame(W, H, CH)
    n = W * H * CH
    rows = []
    print(f"{torch.cuda.get_device_name(0)}; {W} x {H} x {CH} float32 ({n * 4 / 1e6:.1f} MB an image); HIP events, "
          f"{a.iters} calls / {a.step_iters} steps per window, {a.rounds} alternating rounds", flush=True)

    def report(name, us, note=""):
        rows.append({"call": name, "us": [round(u, 2) for u in us], "median_us": round(float(np.median(us)), 2)})
        print(f"1080p  {name:44s} median {np.median(us):10.2f} us  (rounds: {' '.join('%.1f' % u for u in us)}){note}", flush=True)

    frames = [noisy_frame(ctx, base, t) for t in range(NFR)]
    d_y, d_f, d_fp = frames[0], frames[1], frames[2]
    d_out = ctx.alloc(n * 4)
    d_tot = ctx.alloc(8 * 2 * CH)
    d_map = ctx.alloc(16 * CH * ((H + 3) // 4) * ((W + 3) // 4))
    calls = {"sqdiff_sum (2 images read)": (lambda: ctx.sqdiff_sum(d_tot, d_y, d_f, n), 2),
             "probe_add (1 read, 1 written)": (lambda: ctx.probe_add(d_out, d_y, n, 1.0, 7), 2),
             "probe_add in place": (lambda: ctx.probe_add(d_out, d_out, n, 1.0, 7), 2)}
    for block in (16, 4, 64):
        calls[f"sure_terms block {block} (3 images read)"] = (
            lambda block=block: ctx.sure_terms_dev(d_tot, None, d_y, d_f, d_fp, W, H, CH, block, 7), 3)
        calls[f"sure_terms block {block} with the map"] = (
            lambda block=block: ctx.sure_terms_dev(d_tot, d_map, d_y, d_f, d_fp, W, H, CH, block, 7), 3)
    us = {k: [] for k in calls}
    for _ in range(a.rounds):                       # alternate: a drift of the clocks lands on all
        for k, (call, _) in calls.items():
            us[k].append(timed(ctx, stream, call, a.iters, a.settle))
    for k, (_, images) in calls.items():
        report(k, us[k], "  %.0f GB/s of image traffic" % (images * n * 4 / np.median(us[k]) / 1e3))

    # the step: a cycle of NFR distinct frames pushed in order and round again (tools/bmflow_time.py says why)
    sfs, nxt = {}, {}
    for name, kw in (("SequenceFilter step", {}), ("SequenceFilter step, sure=True", dict(sure=True))):
        sf = seq.SequenceFilter(ctx, W, H, CH, SIGMA, keep_history=False, **kw)
        for t in range(2):
            sf.push(frames[t])
        sfs[name], nxt[name] = sf, 2
    ctx.sync()

    def step(name):
        sfs[name].push(frames[nxt[name] % NFR])
        nxt[name] += 1

    us = {k: [] for k in sfs}
    for _ in range(a.rounds):
        for k in sfs:
            us[k].append(timed(ctx, stream, lambda k=k: step(k), a.step_iters, a.settle))
    for k in sfs:
        report(k, us[k])
    plain, sure = (float(np.median(us[k])) for k in sfs)
    print(f"1080p  the estimate adds {sure - plain:.0f} us to a step of {plain:.0f} us ({100 * (sure - plain) / plain:.0f} %)", flush=True)
    # (the second push, before any frame came round again: in the timed cycle the recursion has seen a frame's noise
    # before, which the estimate's assumption excludes)
    e = sfs["SequenceFilter step, sure=True"].sure[1]
    print("1080p  the estimate of the second frame pushed: MSE_hat %.3f, PSNR_hat %.3f, R/N %.3f, div %.5f"
          % (e["mse"], e["psnr"], e["resid"], e["div"]), flush=True)
    ctx.close()
    if a.json:
        with open(a.json, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "iters": a.iters, "step_iters": a.step_iters,
                       "rounds": a.rounds, "calls": rows}, f, indent=1)


if __name__ == "__main__":
    main()
