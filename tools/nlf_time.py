"""Times the two kernels of the noise-level-function transform (nlk_dev_nlf_forward / nlk_dev_nlf_inverse) beside
the variance-stabilising pair (nlk_dev_vst_forward / nlk_dev_vst_inverse) on a 1080p RGB frame with HIP events, after a
clock-settle phase, and prints the rate of their algorithmic bytes (each reads and writes the image once) against the
~6.3 TB/s achievable HBM rate of the MI355X. The table is the one Context.nlf_table measures on the frame (16 bins);
--nbins 64 times the largest table (the inverse's binary search takes the same 7 steps either way).

    python tools/nlf_time.py [--iters N] [--nbins N] [--json FILE]

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
AB = (0.5, 4.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--settle", type=float, default=1.0, help="seconds of back-to-back calls before timing")
    ap.add_argument("--nbins", type=int, default=16)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    pkg = importlib.import_module("bwd-nlkalman_amd")
    synth = importlib.import_module("bwd-nlkalman_amd.synth")
    if pkg.hip().nlk_device_count() < 1:
        raise SystemExit("nlf_time: no HIP device (there is nothing to time without one)")
    ctx = pkg.Context(0)
    stream = torch.cuda.Stream()
    ctx.set_stream(stream.cuda_stream)
    w, h, ch = 1920, 1080, 3
    clean = synth.clean_frame(w, h, ch)
    n, nbytes = clean.size, clean.nbytes
    d_clean, d_img, d_work, d_back = ctx.upload(clean), ctx.alloc(nbytes), ctx.alloc(nbytes), ctx.alloc(nbytes)
    ctx.noise_affine(d_img, d_clean, n, ch, AB, 1)
    table = ctx.nlf_table(d_img, w, h, ch, nbins=a.nbins)
    if not table.s > 0:
        raise SystemExit(f"nlf_time: the frame keeps {list(table.kept)[:ch]} bins")
    ab = np.ascontiguousarray(np.tile(np.asarray(AB, np.float32), (ch, 1)))
    s = pkg.vst_scale(ab)
    calls = {
        "nlf_forward": lambda: ctx.nlf_forward(d_work, d_img, n, ch, table),
        "nlf_inverse": lambda: ctx.nlf_inverse(d_back, d_work, n, ch, table),
        "vst_forward": lambda: ctx.vst_forward(d_work, d_img, n, ch, ab, s),
        "vst_inverse": lambda: ctx.vst_inverse(d_back, d_work, n, ch, ab, s, 1),
    }
    rows = []
    for name, call in calls.items():
        t_end = time.perf_counter() + a.settle       # clock settle (code objects loaded, the table uploaded)
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
        rate = 2 * nbytes / (us * 1e-6)
        rows.append({"call": name, "w": w, "h": h, "ch": ch, "nbins": a.nbins, "us": round(us, 2), "bytes": 2 * nbytes,
                     "GBps": round(rate / 1e9, 1), "of_hbm": round(rate / HBM, 3)})
        print(f"1080p  {name:14s} {us:8.2f} us  {rate / 1e9:8.1f} GB/s  {rate / HBM:6.1%} of 6.3 TB/s", flush=True)
    print(f"kept bins {list(table.kept)[:ch]}, s = {table.s:.4f}")
    for d in (d_clean, d_img, d_work, d_back):
        ctx.free(d)
    if a.json:
        with open(a.json, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "iters": a.iters, "rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
