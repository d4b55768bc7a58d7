"""Times the defective-pixel filter (nlk_dev_despike: R = 1 and 2, with and without counts) on a 1080p RGB frame
beside two calls that move the same bytes, nlk_dev_opp2rgb (in place) and nlk_dev_nlf_forward (each reads and writes
the image once): the yardstick, since no earlier commit has such a kernel. Then one SequenceFilter step (a temporal
frame, 1080p RGB, sigma 20) with and without despike=4. HIP events in one process, after a clock-settle phase; the
calls are alternated for --rounds rounds and every round is printed, so that the spread is on the page. The frame
holds noise of sigma 20 and 0.3 % stuck pixels (the density of DESIGN.md §9's table); the counts are also timed on a
frame with 0.01 % of them, since their cost is that of the atomics, one per wave and channel with a hit, all on ch
addresses. The rate is that of the algorithmic bytes against the ~6.3 TB/s achievable HBM rate of the MI355X.

    python tools/despike_time.py [--iters N] [--rounds N] [--steps N] [--out FILE]

For the time of each kernel run it under `rocprofv3 --kernel-trace --stats`, in a run of its own."""
import argparse
import importlib
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM = 6.3e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=10, help="SequenceFilter steps per round")
    ap.add_argument("--settle", type=float, default=1.0, help="seconds of back-to-back calls before timing")
    ap.add_argument("--out", default=None, help="also write the lines to this file")
    a = ap.parse_args()
    pkg = importlib.import_module("bwd-nlkalman_amd")
    synth = importlib.import_module("bwd-nlkalman_amd.synth")
    seq = importlib.import_module("bwd-nlkalman_amd.sequence")
    if pkg.hip().nlk_device_count() < 1:
        raise SystemExit("despike_time: no HIP device (there is nothing to time without one)")
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    ctx = pkg.Context(0)
    stream = torch.cuda.Stream()
    ctx.set_stream(stream.cuda_stream)
    w, h, ch, sigma = 1920, 1080, 3, 20.0
    rng = np.random.default_rng(1)
    frames = []
    for t in range(2):
        f = synth.clean_frame(w, h, ch, t) + rng.normal(0, sigma, (h, w, ch)).astype(np.float32)
        stuck = rng.random((h, w)) < 0.003
        f[stuck] = 255.0
        frames.append(np.ascontiguousarray(f, np.float32))
    n, nbytes = frames[0].size, frames[0].nbytes
    d_img, d_work, d_cnt = ctx.upload(frames[0]), ctx.alloc(nbytes), ctx.alloc(4 * ch)
    table = ctx.nlf_table(d_img, w, h, ch)
    thr = 4.0 * sigma
    sparse = synth.clean_frame(w, h, ch) + rng.normal(0, sigma, (h, w, ch)).astype(np.float32)
    sparse[rng.random((h, w)) < 0.0001] = 255.0
    d_sparse = ctx.upload(np.ascontiguousarray(sparse, np.float32))
    say(f"{torch.cuda.get_device_name(0)}; 1080p RGB, sigma {sigma:g}, thr {thr:g}; replaced at R = 1: "
        f"{ctx.despike_counts(d_work, d_img, w, h, ch, thr, 1).tolist()}, at R = 2: "
        f"{ctx.despike_counts(d_work, d_img, w, h, ch, thr, 2).tolist()}; on the frame with 0.01 % stuck pixels: "
        f"{ctx.despike_counts(d_work, d_sparse, w, h, ch, thr, 1).tolist()}")
    calls = {
        "despike R=1": lambda: ctx.despike(d_work, d_img, w, h, ch, thr, 1),
        "despike R=1 +counts": lambda: ctx.despike(d_work, d_img, w, h, ch, thr, 1, d_cnt),
        "despike R=2": lambda: ctx.despike(d_work, d_img, w, h, ch, thr, 2),
        "despike R=2 +counts": lambda: ctx.despike(d_work, d_img, w, h, ch, thr, 2, d_cnt),
        "R=1 +counts, 0.01 %": lambda: ctx.despike(d_work, d_sparse, w, h, ch, thr, 1, d_cnt),
        "opp2rgb": lambda: ctx.opp2rgb(d_work, w, h, ch),
        "nlf_forward": lambda: ctx.nlf_forward(d_work, d_img, n, ch, table),
    }
    t_end = time.perf_counter() + a.settle       # clock settle (code objects loaded, the table uploaded)
    while time.perf_counter() < t_end:
        for call in calls.values():
            for _ in range(10):
                call()
        ctx.sync()
    us = {name: [] for name in calls}
    for _ in range(a.rounds):
        for name, call in calls.items():
            for _ in range(10):
                call()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            for _ in range(a.iters):
                call()
            e1.record(stream)
            e1.synchronize()
            us[name].append(e0.elapsed_time(e1) * 1e3 / a.iters)
    for name, v in us.items():
        best = min(v)
        rate = 2 * nbytes / (best * 1e-6)
        say(f"1080p  {name:20s} " + " ".join(f"{x:8.2f}" for x in v) + f" us   best {rate / 1e9:7.1f} GB/s "
            f"{rate / HBM:6.1%} of 6.3 TB/s")
    for r in ("R=1", "R=2"):
        d = min(us["despike " + r])
        say(f"despike {r} / opp2rgb = {d / min(us['opp2rgb']):.2f}, / nlf_forward = {d / min(us['nlf_forward']):.2f} "
            f"(best of {a.rounds} rounds each)")

    # one SequenceFilter step with and without the option: temporal frames, alternated
    d_fr = [ctx.upload(f) for f in frames]
    filt = {"step": seq.SequenceFilter(ctx, w, h, ch, sigma, keep_history=False),
            "step despike=4": seq.SequenceFilter(ctx, w, h, ch, sigma, keep_history=False, despike=4)}
    for sf in filt.values():
        for k in range(6):
            sf.push(d_fr[k & 1])
    ctx.sync()
    ms = {name: [] for name in filt}
    for _ in range(a.rounds):
        for name, sf in filt.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            for k in range(a.steps):
                sf.push(d_fr[k & 1])
            e1.record(stream)
            e1.synchronize()
            ms[name].append(e0.elapsed_time(e1) / a.steps)
    for name, v in ms.items():
        say(f"1080p  SequenceFilter {name:16s} " + " ".join(f"{x:8.3f}" for x in v) + " ms per temporal frame")
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
