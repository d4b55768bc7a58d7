"""Times the quality measure (nlk_dev_ssim: the tile kernel and the final sum on the context's stream) on a 1080p and
a 4K RGB frame pair with HIP events, after a clock-settle phase, with and without the map, and prints the rate of its
algorithmic bytes (both images read once) against the ~6.3 TB/s achievable HBM rate of the MI355X - beside
nlk_dev_sqdiff_sum on the same frames, which reads the same bytes, and the step of the resident filter that three
calls per frame have to stay small against (0.91 ms at 1080p, README).

    python tools/ssim_time.py [--iters N] [--json FILE]

For the time of each kernel run it under `rocprofv3 --kernel-trace --stats`, in a run of its own."""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM = 6.3e12
FILTER_STEP_US = {"1080p": 910.0}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--settle", type=float, default=1.0, help="seconds of back-to-back calls before timing")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    pkg = importlib.import_module("bwd-nlkalman_amd")
    synth = importlib.import_module("bwd-nlkalman_amd.synth")
    if pkg.hip().nlk_device_count() < 1:
        raise SystemExit("ssim_time: no HIP device (there is nothing to time without one)")
    ctx = pkg.Context(0)
    stream = torch.cuda.Stream()
    ctx.set_stream(stream.cuda_stream)
    ch, rows = 3, []
    for name, (w, h) in (("1080p", (1920, 1080)), ("4K", (3840, 2160))):
        clean = synth.clean_frame(w, h, ch)
        n = clean.size
        d_a = ctx.upload(clean)
        d_b = ctx.alloc(4 * n)
        ctx.awgn(d_b, d_a, n, 20.0, 1)
        d_out = ctx.alloc(8 * (2 + ch))        # ssim, ssim_c | the squared-error sum
        d_map = ctx.alloc(4 * (w - 10) * (h - 10) * ch)
        calls = {
            "ssim": lambda: ctx.ssim_dev(d_out, None, d_a, d_b, w, h, ch),
            "ssim+map": lambda: ctx.ssim_dev(d_out, d_map, d_a, d_b, w, h, ch),
            "sqdiff_sum": lambda: ctx.sqdiff_sum(d_out + 8 * (1 + ch), d_a, d_b, n),
        }
        nbytes = 2 * n * 4
        for call in calls.values():                      # every slot of d_out holds its value from here on
            call()
        ctx.sync()
        for what, call in calls.items():
            t_end = time.perf_counter() + a.settle       # clock settle (code objects loaded, scratch grown)
            while time.perf_counter() < t_end:
                for _ in range(20):
                    call()
                ctx.sync()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            for _ in range(a.iters):
                call()
            e1.record(stream)
            e1.synchronize()
            us = e0.elapsed_time(e1) * 1e3 / a.iters
            rate = nbytes / (us * 1e-6)
            res = ctx.download(d_out, (2 + ch,), np.float64)
            row = {"size": name, "w": w, "h": h, "ch": ch, "what": what, "us": round(us, 2), "bytes": nbytes,
                   "GBps": round(rate / 1e9, 1), "of_hbm": round(rate / HBM, 4), "ssim": float(res[0]),
                   "mse": float(res[1 + ch]) / n}
            line = f"{name:6s} {what:11s} {us:9.2f} us  {rate / 1e9:8.1f} GB/s  {rate / HBM:6.1%} of 6.3 TB/s"
            if name in FILTER_STEP_US and what != "sqdiff_sum":
                row["of_filter_step"] = round(us / FILTER_STEP_US[name], 4)
                line += f"   {us / FILTER_STEP_US[name]:.1%} of the filter's {FILTER_STEP_US[name] / 1e3:.2f} ms step"
            if what == "ssim":
                line += f"   ssim {res[0]:.6f}"
            rows.append(row)
            print(line, flush=True)
        for d in (d_a, d_b, d_out, d_map):
            ctx.free(d)
    if a.json:
        with open(a.json, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "iters": a.iters, "rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
