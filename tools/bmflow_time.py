"""Times the block-matching flow (nlk_dev_bm_flow, --of bm) beside the TV-L1 path it can stand in for, at 1080p RGB, with
HIP events after a clock-settle phase (as tools/lag1_time.py). The two estimators alternate inside one process, round
after round, so that the spread of each is seen next to the difference between them:

  - nlk_dev_bm_flow beside nlk_dev_tvl1_flow on the same pair of gray images (noisy frame 1 -> flt2 of frame 0, the pair
    that the recursion hands to its flow), with the median vector of each (the frames pan by 2 pixels);
  - one SequenceFilter step (push of a temporal frame) with of="bm" beside of="tvl1", over a cycle of four distinct
    frames of the pan pushed in order (bench.py's S1 does the same), with TV-L1's iteration counts inside those steps;
  - the wall time per frame of `nlkalman-y4m --of bm 20` beside `nlkalman-y4m 20` on the same 60-frame 1080p 4:2:0
    stream in a memory-backed folder.

To be read against the S1 step of bench.py (`bench.py --workload S1`), which keeps timing the default.

    python tools/bmflow_time.py [--iters N] [--rounds N] [--frames N] [--no-tools] [--json FILE]"""
import argparse
import importlib
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
BIN = os.path.join(ROOT, "bwd-nlkalman_amd", "bin")
W, H, CH, SIGMA = 1920, 1080, 3, 20.0
NFR = 4   # distinct frames in the cycle that the timed steps push


def timed(ctx, stream, call, iters, settle):
    t_end = time.perf_counter() + settle             # clock settle (code objects loaded)
    while time.perf_counter() < t_end:
        for _ in range(max(1, min(20, iters))):
            call()
        ctx.sync()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    for _ in range(iters):
        call()
    e1.record(stream)
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters


def noisy_frame(ctx, base, t):
    """frame t of a pan of 2 pixels per frame with noise of sigma 20 made on the GPU: a device RGB image"""
    clean = np.ascontiguousarray(np.roll(base, -2 * t, axis=1))
    d = ctx.upload(clean)
    ctx.awgn(d, d, clean.size, SIGMA, 100 + t)
    return d


def device_calls(pkg, synth, a):
    seq = importlib.import_module("bwd-nlkalman_amd.sequence")
    ctx = pkg.Context(0)
    stream = torch.cuda.Stream()
    ctx.set_stream(stream.cuda_stream)
    base = synth.clean_frame(W, H, CH)
    rows = []

    def report(name, us, note=""):
        rows.append({"call": name, "us": [round(u, 2) for u in us], "median_us": round(float(np.median(us)), 2)})
        print(f"1080p  {name:40s} median {np.median(us):10.2f} us  (rounds: {' '.join('%.1f' % u for u in us)}){note}", flush=True)

    # The two steps run on a cycle of NFR distinct frames of the pan, pushed in order and round again, as the S1 workload
    # of bench.py does: every timed push sees a frame that moved against the filter's previous estimate (2 pixels, and 6
    # back where the cycle closes), so TV-L1's stop test ends where it ends on moving footage. Pushing one frame over and
    # over would hand the flow a pair without motion, which TV-L1 leaves after a few iterations.
    frames = [noisy_frame(ctx, base, t) for t in range(NFR)]
    sfs, nxt = {}, {}
    for of in ("tvl1", "bm"):
        sf = seq.SequenceFilter(ctx, W, H, CH, SIGMA, keep_history=False, of=of)
        for t in range(2):
            sf.push(frames[t])
        sfs[of], nxt[of] = sf, 2
    ctx.sync()

    def step(of):
        sfs[of].push(frames[nxt[of] % NFR])
        nxt[of] += 1

    sf = seq.SequenceFilter(ctx, W, H, CH, SIGMA, keep_history=False)   # its gray images: noisy frame 1 -> flt2 of frame 0
    for t in range(2):
        sf.push(frames[t])
    ctx.sync()
    d_flow = ctx.alloc(W * H * 8)
    flows = {"tvl1_flow (lam 0.25, fscale 1)": lambda: ctx.tvl1_flow(d_flow, sf.d_g0, sf.d_g1, W, H, sf.of),
             "bm_flow (fscale 1, radius 2)": lambda: ctx.bm_flow(d_flow, sf.d_g0, sf.d_g1, W, H),
             "bm_flow (fscale 0, radius 2)": lambda: ctx.bm_flow(d_flow, sf.d_g0, sf.d_g1, W, H, fscale=0),
             "bm_flow (fscale 1, radius 3)": lambda: ctx.bm_flow(d_flow, sf.d_g0, sf.d_g1, W, H, radius=3)}
    steps = {f"SequenceFilter step, of={of}": (lambda of=of: step(of)) for of in ("tvl1", "bm")}
    for group, iters in ((flows, a.iters), (steps, a.step_iters)):
        us = {k: [] for k in group}
        for _ in range(a.rounds):                       # alternate: a drift of the clocks lands on both
            for k, call in group.items():
                us[k].append(timed(ctx, stream, call, iters, a.settle))
        for k, call in group.items():
            note = ""
            if group is flows:
                call()
                f = ctx.download(d_flow, (H, W, 2))
                note = "  median vector (%.3f, %.3f)" % (np.median(f[..., 0]), np.median(f[..., 1]))
            report(k, us[k], note)
    # TV-L1's work depends on its stop test: the iterations of the flow that was timed alone, beside those of the last
    # cycle of timed steps
    alone = ctx.tvl1_flow(d_flow, sf.d_g0, sf.d_g1, W, H, sf.of)
    in_steps = sfs["tvl1"].flow_iterations[-NFR:]
    rows.append({"tvl1_iterations": {"alone": alone, "last_cycle_of_steps": in_steps}})
    print(f"1080p  TV-L1 iterations: {alone} in the flow timed alone, {in_steps} in the last {NFR} timed steps", flush=True)
    ctx.close()
    return rows


def tools(pkg, synth, a):
    import yuv_ref as R
    n = a.frames
    base = "/dev/shm" if os.path.isdir("/dev/shm") and os.access("/dev/shm", os.W_OK) else None
    tmp = tempfile.mkdtemp(prefix="bmflow_time_", dir=base)
    rows = []
    try:
        ctx = pkg.Context(0)
        cf = pkg.yuv_format_from_tag("420jpeg")
        base_frame = synth.clean_frame(W, H, CH)
        with open(os.path.join(tmp, "in.y4m"), "wb") as s:
            s.write(R.y4m_header(W, H, "420jpeg"))
            for t in range(n):
                d = noisy_frame(ctx, base_frame, t)
                s.write(b"FRAME\n" + ctx.rgb_to_yuv(ctx.download(d, base_frame.shape), cf).tobytes())
                ctx.free(d)
        ctx.close()
        tool, src, dst = os.path.join(BIN, "nlkalman-y4m"), os.path.join(tmp, "in.y4m"), os.path.join(tmp, "out.y4m")
        runs = (("nlkalman-y4m 20", []), ("nlkalman-y4m --of bm 20", ["--of", "bm"]))
        wall = {name: [] for name, _ in runs}
        for _ in range(a.rounds):                        # alternate (the first round also pays for a cold page cache)
            for name, flags in runs:
                t0 = time.perf_counter()
                r = subprocess.run([tool, *flags, "20", src, dst], capture_output=True, timeout=900)
                wall[name].append(time.perf_counter() - t0)
                if r.returncode:
                    raise SystemExit(f"bmflow_time: {name} failed: {r.stderr.decode()[-400:]}")
        for name, _ in runs:
            best = min(wall[name])
            rows.append({"run": name, "frames": n, "wall_s": [round(x, 3) for x in wall[name]],
                         "best_ms_per_frame": round(best * 1e3 / n, 2)})
            print(f"1080p x {n}  {name:28s} best {best:7.2f} s  {best * 1e3 / n:8.2f} ms / frame (process start included; "
                  f"rounds: {' '.join('%.2f' % x for x in wall[name])})", flush=True)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200, help="flows per timed window")
    ap.add_argument("--step-iters", type=int, default=48, help="steps per timed window (whole cycles of 4 frames)")
    ap.add_argument("--rounds", type=int, default=3, help="alternating rounds of every comparison")
    ap.add_argument("--settle", type=float, default=1.0, help="seconds of back-to-back calls before timing")
    ap.add_argument("--frames", type=int, default=60)
    ap.add_argument("--no-tools", action="store_true")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    pkg = importlib.import_module("bwd-nlkalman_amd")
    synth = importlib.import_module("bwd-nlkalman_amd.synth")
    if pkg.hip().nlk_device_count() < 1:
        raise SystemExit("bmflow_time: no HIP device (there is nothing to time without one)")
    out = {"device": torch.cuda.get_device_name(0), "iters": a.iters, "step_iters": a.step_iters, "rounds": a.rounds,
           "calls": device_calls(pkg, synth, a)}
    if not a.no_tools:
        out["tools"] = tools(pkg, synth, a)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
