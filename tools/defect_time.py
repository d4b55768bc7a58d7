"""Times one step of the defect map learned over time (nlk_dev_defect_step: R = 1 and 2; without map and counts, with
the map, with both) on a 1080p RGB frame beside nlk_dev_despike R = 1 and nlk_dev_nlf_forward on the same frame. The
step moves four planes (frame and mean read, frame and mean written) where despike moves two: that ratio is the
yardstick. Then one SequenceFilter step (a temporal frame, 1080p RGB, sigma 20) with and without defect_map=4, every
pushed frame with noise of its own.

The method of tools/despike_time.py: HIP events in one process, after a clock-settle phase; the calls are alternated
for --rounds rounds and every round is printed, so that the spread is on the page. The frames hold noise of sigma 20
and 0.3 % stuck pixels (the density of DESIGN.md §9's table); the mean is that of 8 such frames, the threshold the
schedule's for frame 8. The rate is that of the algorithmic bytes (four planes; two for despike and nlf_forward)
against the ~6.3 TB/s achievable HBM rate of the MI355X.

    python tools/defect_time.py [--iters N] [--rounds N] [--steps N] [--out FILE]
    python tools/defect_time.py --step-only [--root TREE]

--step-only: only the SequenceFilter step without the option, from the package under TREE (default: this tree): for
alternated processes against the parent commit's build, whose package has no defect step."""
import argparse
import importlib
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HBM = 6.3e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=10, help="SequenceFilter steps per round")
    ap.add_argument("--settle", type=float, default=1.0, help="seconds of back-to-back calls before timing")
    ap.add_argument("--out", default=None, help="also write the lines to this file")
    ap.add_argument("--step-only", action="store_true")
    ap.add_argument("--root", default=ROOT, help="the tree whose package is timed")
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.root))
    pkg = importlib.import_module("bwd-nlkalman_amd")
    synth = importlib.import_module("bwd-nlkalman_amd.synth")
    seq = importlib.import_module("bwd-nlkalman_amd.sequence")
    if pkg.hip().nlk_device_count() < 1:
        raise SystemExit("defect_time: no HIP device (there is nothing to time without one)")
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    ctx = pkg.Context(0)
    stream = torch.cuda.Stream()
    ctx.set_stream(stream.cuda_stream)
    w, h, ch, sigma = 1920, 1080, 3, 20.0
    rng = np.random.default_rng(1)
    stuck = rng.random((h, w)) < 0.003
    frames = []
    for t in range(9):
        f = synth.clean_frame(w, h, ch, t) + rng.normal(0, sigma, (h, w, ch)).astype(np.float32)
        f[stuck] = 255.0
        frames.append(np.ascontiguousarray(f, np.float32))
    n, nbytes = frames[0].size, frames[0].nbytes

    def steps(filt, label):
        """one SequenceFilter step of each filter: temporal frames, alternated. Every push of a filter is a frame with
        noise of its own (a repeated frame is a static scene with static noise: the map would learn the noise)"""
        clean = [synth.clean_frame(w, h, ch, t) for t in range(9)]
        d_fr = []
        for k in range(6 + a.rounds * a.steps):
            f = clean[k % 9] + sigma * rng.standard_normal((h, w, ch), dtype=np.float32)
            f[stuck] = 255.0
            d_fr.append(ctx.upload(np.ascontiguousarray(f, np.float32)))
        for sf in filt.values():
            for k in range(6):
                sf.push(d_fr[k])
        ctx.sync()
        ms = {name: [] for name in filt}
        for r in range(a.rounds):
            for name, sf in filt.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                for k in range(a.steps):
                    sf.push(d_fr[6 + r * a.steps + k])
                e1.record(stream)
                e1.synchronize()
                ms[name].append(e0.elapsed_time(e1) / a.steps)
        for name, v in ms.items():
            say(f"1080p  SequenceFilter {name:20s} " + " ".join(f"{x:8.3f}" for x in v) + f" ms per temporal frame{label}")

    if a.step_only:
        t_end = time.perf_counter() + a.settle
        d = ctx.upload(frames[0])
        while time.perf_counter() < t_end:
            for _ in range(50):
                ctx.opp2rgb(d, w, h, ch)
            ctx.sync()
        steps({"step": seq.SequenceFilter(ctx, w, h, ch, sigma, keep_history=False)}, "   " + os.path.abspath(a.root))
        return

    # the mean of frames 0..7 by the kernel itself, then frame 8 is the one timed
    d_img, d_work = ctx.upload(frames[8]), ctx.alloc(nbytes)
    d_mean, d_map, d_cnt = [ctx.alloc(nbytes), ctx.alloc(nbytes)], ctx.alloc(n), ctx.alloc(4 * ch)
    for t in range(8):
        d = ctx.upload(frames[t])
        thr, gain = ctx.defect_schedule(t, 32, 4.0 * sigma) if t else (0.0, 1.0)
        ctx.defect_step(d_work, d, d_mean[(t + 1) & 1], d_mean[t & 1] if t else None, w, h, ch, thr, gain, 1)
        ctx.sync()
        ctx.free(d)
    d_m, d_mo = d_mean[0], d_mean[1]          # (8 steps: the last one wrote d_mean[0])
    thr, gain = ctx.defect_schedule(8, 32, 4.0 * sigma)
    table = ctx.nlf_table(d_img, w, h, ch)
    counts = {}
    for r in (1, 2):
        ctx.defect_step(d_work, d_img, d_mo, d_m, w, h, ch, thr, gain, r, None, d_cnt)
        counts[r] = ctx.download(d_cnt, (ch,), np.uint32).tolist()
    say(f"{torch.cuda.get_device_name(0)}; 1080p RGB, sigma {sigma:g}, frame 8: thr {thr:.4g}, gain {gain:.4g}; "
        f"{int(stuck.sum())} stuck pixels; replaced at R = 1: {counts[1]}, at R = 2: {counts[2]}")

    def step(r, with_map=False, with_counts=False):
        return lambda: ctx.defect_step(d_work, d_img, d_mo, d_m, w, h, ch, thr, gain, r, d_map if with_map else None,
                                       d_cnt if with_counts else None)

    calls = {
        "defect_step R=1": (step(1), 4),
        "defect_step R=1 +map": (step(1, True), 4),
        "defect_step R=1 +map +counts": (step(1, True, True), 4),
        "defect_step R=2": (step(2), 4),
        "defect_step R=2 +map": (step(2, True), 4),
        "defect_step first frame": (lambda: ctx.defect_step(d_work, d_img, d_mo, None, w, h, ch, 0.0, 1.0, 1), 3),
        "despike R=1": (lambda: ctx.despike(d_work, d_img, w, h, ch, 4.0 * sigma, 1), 2),
        "nlf_forward": (lambda: ctx.nlf_forward(d_work, d_img, n, ch, table), 2),
    }
    t_end = time.perf_counter() + a.settle       # clock settle (code objects loaded, the table uploaded)
    while time.perf_counter() < t_end:
        for call, _ in calls.values():
            for _ in range(10):
                call()
        ctx.sync()
    us = {name: [] for name in calls}
    for _ in range(a.rounds):
        for name, (call, _) in calls.items():
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
        rate = calls[name][1] * nbytes / (best * 1e-6)
        say(f"1080p  {name:30s} " + " ".join(f"{x:8.2f}" for x in v) + f" us   best {rate / 1e9:7.1f} GB/s "
            f"{rate / HBM:6.1%} of 6.3 TB/s ({calls[name][1]} planes)")
    for r in ("R=1", "R=2"):
        d = min(us["defect_step " + r])
        say(f"defect_step {r} / despike R=1 = {d / min(us['despike R=1']):.2f}, / nlf_forward = "
            f"{d / min(us['nlf_forward']):.2f} (best of {a.rounds} rounds each; four planes against two)")

    steps({"step": seq.SequenceFilter(ctx, w, h, ch, sigma, keep_history=False),
           "step defect_map=4": seq.SequenceFilter(ctx, w, h, ch, sigma, keep_history=False, defect_map=4),
           "defect_map=4 +counts": seq.SequenceFilter(ctx, w, h, ch, sigma, keep_history=False, defect_map=4,
                                                      defect_counts=True)}, "")
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
