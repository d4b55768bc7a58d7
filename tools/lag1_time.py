"""Times the lag-1 smoother at 1080p RGB, with HIP events after a clock-settle phase (as tools/y4m_time.py):

  - nlk_dev_flow_invert by itself, on the backward flow that the recursion left for a real pair of frames, beside
    nlk_dev_opp2rgb on the same frame (an existing one-pass kernel) and nlk_dev_tvl1_flow flt2_0 -> flt2_1 (the flow
    that the inversion replaces);
  - one lag-1 step (seq_lag1_step: flow, mask, warp, SMO1) with each flow source, through SequenceFilter;
  - the wall time per frame of `nlkalman-y4m 20` on a 60-frame 1080p 4:2:0 stream in a memory-backed folder without
    smoothing, with --smooth tvl1 and with --smooth inv.

To be read against the S1 step of bench.py (`bench.py --workload S1`): the forward recursion that the smoother is
added to.

    python tools/lag1_time.py [--iters N] [--step-iters N] [--frames N] [--no-tools] [--json FILE]"""
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


def noisy_frame(ctx, synth, base, t):
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

    def report(name, us, nbytes=None):
        row = {"call": name, "us": round(us, 2)}
        if nbytes:
            row.update(bytes=nbytes, GBps=round(nbytes / (us * 1e-6) / 1e9, 1))
        rows.append(row)
        rate = f"{nbytes / 1e6:6.1f} MB  {nbytes / (us * 1e-6) / 1e9:8.1f} GB/s" if nbytes else ""
        print(f"1080p  {name:44s} {us:10.2f} us  {rate}", flush=True)

    for mode in ("tvl1", "inv"):
        sf = seq.SequenceFilter(ctx, W, H, CH, SIGMA, keep_history=False, lag1=mode)
        prev = None
        for t in range(2):
            d = noisy_frame(ctx, synth, base, t)
            if t == 1:
                prev = sf.flt2                        # (push returns it to the pool, where nothing takes it: one frame only)
            sf.push(d)
            ctx.free(d)
        ctx.sync()
        cur, sf.flt2 = sf.flt2, prev                 # the state in which push() calls the step: flt2 of frame 0, 1 and its flow
        if mode == "inv":
            d_inv, nb = ctx.alloc(W * H * 8), W * H * 8
            report("flow_invert (4 steps)", timed(ctx, stream, lambda: ctx.flow_invert(d_inv, sf.d_flow, W, H, 4), a.iters, a.settle), 2 * nb)
            report("flow_invert (0 steps: the two passes alone)",
                   timed(ctx, stream, lambda: ctx.flow_invert(d_inv, sf.d_flow, W, H, 0), a.iters, a.settle), 2 * nb)
            ctx.d2d(sf.d_rgb, cur, sf.nbytes)
            report("opp2rgb (in place)", timed(ctx, stream, lambda: ctx.opp2rgb(sf.d_rgb, W, H, CH), a.iters, a.settle), 2 * sf.nbytes)
            ctx.free(d_inv)
        else:
            report("tvl1_flow flt2_0 -> flt2_1 (what inv replaces)",
                   timed(ctx, stream, lambda: ctx.tvl1_flow(sf.d_fflow, sf.d_g0, sf.d_g1, W, H, sf.of2), a.step_iters, a.settle))
        report(f"lag-1 step, flow source {mode}", timed(ctx, stream, lambda: sf._lag1_step(cur), a.step_iters, a.settle))
    ctx.close()
    return rows


def tools(pkg, synth, a):
    import yuv_ref as R
    n = a.frames
    base = "/dev/shm" if os.path.isdir("/dev/shm") and os.access("/dev/shm", os.W_OK) else None
    tmp = tempfile.mkdtemp(prefix="lag1_time_", dir=base)
    rows = []
    try:
        ctx = pkg.Context(0)
        cf = pkg.yuv_format_from_tag("420jpeg")
        base_frame = synth.clean_frame(W, H, CH)
        with open(os.path.join(tmp, "in.y4m"), "wb") as s:
            s.write(R.y4m_header(W, H, "420jpeg"))
            for t in range(n):
                d = noisy_frame(ctx, synth, base_frame, t)
                s.write(b"FRAME\n" + ctx.rgb_to_yuv(ctx.download(d, base_frame.shape), cf).tobytes())
                ctx.free(d)
        ctx.close()
        tool, src, dst = os.path.join(BIN, "nlkalman-y4m"), os.path.join(tmp, "in.y4m"), os.path.join(tmp, "out.y4m")
        for name, flags in (("nlkalman-y4m 20", []), ("nlkalman-y4m --smooth tvl1 20", ["--smooth", "tvl1"]),
                            ("nlkalman-y4m --smooth inv 20", ["--smooth", "inv"])):
            best = None
            for _ in range(2):                        # (the first run also pays for a cold page cache)
                t0 = time.perf_counter()
                r = subprocess.run([tool, *flags, "20", src, dst], capture_output=True, timeout=900)
                dt = time.perf_counter() - t0
                if r.returncode:
                    raise SystemExit(f"lag1_time: {name} failed: {r.stderr.decode()[-400:]}")
                best = dt if best is None else min(best, dt)
            rows.append({"run": name, "frames": n, "wall_s": round(best, 3), "ms_per_frame": round(best * 1e3 / n, 2)})
            print(f"1080p x {n}  {name:34s} {best:7.2f} s  {best * 1e3 / n:8.2f} ms / frame (process start included)", flush=True)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=2000, help="calls per timed window of a one-pass kernel (microseconds each)")
    ap.add_argument("--step-iters", type=int, default=50, help="calls per timed window of a flow or a whole step (milliseconds each)")
    ap.add_argument("--settle", type=float, default=1.0, help="seconds of back-to-back calls before timing")
    ap.add_argument("--frames", type=int, default=60)
    ap.add_argument("--no-tools", action="store_true")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    pkg = importlib.import_module("bwd-nlkalman_amd")
    synth = importlib.import_module("bwd-nlkalman_amd.synth")
    if pkg.hip().nlk_device_count() < 1:
        raise SystemExit("lag1_time: no HIP device (there is nothing to time without one)")
    out = {"device": torch.cuda.get_device_name(0), "iters": a.iters, "step_iters": a.step_iters,
           "calls": device_calls(pkg, synth, a)}
    if not a.no_tools:
        out["tools"] = tools(pkg, synth, a)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
