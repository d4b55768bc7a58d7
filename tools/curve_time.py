"""Times the noise-curve estimator (nlk_dev_estimate_noise_curve: one memset and ten kernels on the context's
stream), the two variance-stabilising transforms (nlk_dev_vst_forward / _inverse, one kernel each) and
nlk_dev_noise_affine on a 1080p RGB frame with HIP events, after a clock-settle phase, and prints the rate of their
algorithmic bytes (the estimator reads the image once, the others read and write it once) against the ~6.3 TB/s
achievable HBM rate of the MI355X. For comparison it times nlk_dev_estimate_sigma and nlk_dev_awgn the same way.

    python tools/curve_time.py [--iters N] [--json FILE]

For the time of each kernel run it under `rocprofv3 --kernel-trace --stats`, in a run of its own."""
import argparse
import ctypes as C
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
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    pkg = importlib.import_module("bwd-nlkalman_amd")
    synth = importlib.import_module("bwd-nlkalman_amd.synth")
    if pkg.hip().nlk_device_count() < 1:
        raise SystemExit("curve_time: no HIP device (there is nothing to time without one)")
    ctx = pkg.Context(0)
    stream = torch.cuda.Stream()
    ctx.set_stream(stream.cuda_stream)
    w, h, ch = 1920, 1080, 3
    clean = synth.clean_frame(w, h, ch)
    n, nbytes = clean.size, clean.nbytes
    d_clean, d_img, d_work, d_back = ctx.upload(clean), ctx.alloc(nbytes), ctx.alloc(nbytes), ctx.alloc(nbytes)
    ctx.noise_affine(d_img, d_clean, n, ch, AB, 1)
    cprm, sprm = pkg.curve_params(), pkg.sigma_params()
    nb = cprm.nbins
    d_out = ctx.alloc(8 * ch + 16 * ch * nb)
    ab = np.ascontiguousarray(np.tile(np.asarray(AB, np.float32), (ch, 1)))
    s = pkg.vst_scale(ab)
    L, H = ctx.L, ctx.h
    calls = {
        "estimate_noise_curve": (1, lambda: L.nlk_dev_estimate_noise_curve(H, d_out, d_out + 8 * ch, d_img, w, h, ch, C.byref(cprm))),
        "estimate_sigma": (1, lambda: L.nlk_dev_estimate_sigma(H, d_out, d_out + 4 * (1 + ch), d_img, w, h, ch, C.byref(sprm))),
        "vst_forward": (2, lambda: L.nlk_dev_vst_forward(H, d_work, d_img, n, ch, ab.ctypes.data, s)),
        "vst_inverse": (2, lambda: L.nlk_dev_vst_inverse(H, d_back, d_work, n, ch, ab.ctypes.data, s, 1)),
        "noise_affine": (2, lambda: L.nlk_dev_noise_affine(H, d_work, d_clean, n, ch, ab.ctypes.data, 1)),
        "awgn": (2, lambda: L.nlk_dev_awgn(H, d_work, d_clean, n, 20.0, 1)),
    }
    rows = []
    for name, (passes, call) in calls.items():
        t_end = time.perf_counter() + a.settle       # clock settle (code objects loaded, scratch grown)
        while time.perf_counter() < t_end:
            for _ in range(20):
                ctx._chk(call())
            ctx.sync()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(a.iters):
            ctx._chk(call())
        e1.record(stream)
        e1.synchronize()
        us = e0.elapsed_time(e1) * 1e3 / a.iters
        rate = passes * nbytes / (us * 1e-6)
        row = {"call": name, "w": w, "h": h, "ch": ch, "us": round(us, 2), "bytes": passes * nbytes,
               "GBps": round(rate / 1e9, 1), "of_hbm": round(rate / HBM, 3)}
        line = f"1080p  {name:22s} {us:8.2f} us  {rate / 1e9:8.1f} GB/s  {rate / HBM:6.1%} of 6.3 TB/s"
        if name == "estimate_noise_curve":
            est = ctx.download(d_out, (ch, 2))
            row["ab"] = [[float(v) for v in r] for r in est]
            line += "   (a, b) " + " ".join("(%.3f, %.2f)" % tuple(r) for r in est) + "  (true (0.5, 4))"
        rows.append(row)
        print(line, flush=True)
    for d in (d_clean, d_img, d_work, d_back, d_out):
        ctx.free(d)
    if a.json:
        with open(a.json, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "iters": a.iters, "rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
