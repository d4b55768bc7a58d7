"""Times the Lanczos-3 pyramid kernels (nlk_dev_lz3_down / _up / _recompose_step) at 1080p and 4K RGB with HIP
events, after a clock-settle phase, and prints the rate of algorithmic bytes (each input read once, each output
written once) against the ~6.3 TB/s achievable HBM rate of the MI355X.

    python tools/lz3_time.py [--iters N] [--json FILE]

The up is timed at the named size as its output (from the half-size image, 2n fit); the recompose step has the
named size as its fine level and g = 0.7 (two launches: down(yh), then yh + up(gblur(rl - down(yh))))."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--settle", type=float, default=1.0, help="seconds of back-to-back launches before timing")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    pkg = importlib.import_module("bwd-nlkalman_amd")
    if pkg.hip().nlk_device_count() < 1:
        raise SystemExit("lz3_time: no HIP device (there is nothing to time without one)")
    ctx = pkg.Context(0)
    stream = torch.cuda.Stream()
    ctx.set_stream(stream.cuda_stream)
    ch, rows = 3, []
    for name, (w, h) in (("1080p", (1920, 1080)), ("4K", (3840, 2160))):
        wl, hl = (w + 1) // 2, (h + 1) // 2
        rng = np.random.default_rng(0)
        d_y = ctx.upload(rng.uniform(0, 255, (h, w, ch)).astype(np.float32))
        d_l = ctx.upload(rng.uniform(0, 255, (hl, wl, ch)).astype(np.float32))
        d_o = ctx.alloc(w * h * ch * 4)
        d_d = ctx.alloc(wl * hl * ch * 4)
        fine, coarse = w * h * ch * 4, wl * hl * ch * 4
        ops = {
            "down": (lambda: ctx.lz3_down(d_d, d_y, w, h, ch), fine + coarse),
            "up": (lambda: ctx.lz3_up(d_o, w, h, d_l, wl, hl, ch), coarse + fine),
            "recompose_step": (lambda: ctx.lz3_recompose_step(d_o, d_y, w, h, d_l, wl, hl, ch, 0.7),
                               fine + coarse + fine),
        }
        t_end = time.perf_counter() + a.settle       # clock settle (and code objects loaded)
        while time.perf_counter() < t_end:
            for fn, _ in ops.values():
                for _ in range(20):
                    fn()
            ctx.sync()
        for op, (fn, nbytes) in ops.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            for _ in range(a.iters):
                fn()
            e1.record(stream)
            e1.synchronize()
            us = e0.elapsed_time(e1) * 1e3 / a.iters
            rate = nbytes / (us * 1e-6)
            rows.append({"size": name, "w": w, "h": h, "ch": ch, "op": op, "us": round(us, 2),
                         "bytes": nbytes, "GBps": round(rate / 1e9, 1), "of_hbm": round(rate / HBM, 3)})
            print(f"{name:6s} {op:15s} {us:8.2f} us  {rate / 1e9:8.1f} GB/s  {rate / HBM:6.1%} of 6.3 TB/s", flush=True)
        for d in (d_y, d_l, d_o, d_d):
            ctx.free(d)
    if a.json:
        with open(a.json, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "iters": a.iters, "rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
