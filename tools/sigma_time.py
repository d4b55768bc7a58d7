"""Times the noise-level estimator (nlk_dev_estimate_sigma: one memset and ten kernels on the context's stream)
on a 1080p and a 4K RGB frame with HIP events, after a clock-settle phase, and prints the rate of its algorithmic
bytes (the image read once) against the ~6.3 TB/s achievable HBM rate of the MI355X, and the budget it has to stay
under: the first frame of a sequence, which `SIG = auto` precedes (1.67 ms at 1080p).

    python tools/sigma_time.py [--iters N] [--json FILE]

For the time of each kernel run it under `rocprofv3 --kernel-trace --stats`, in a run of its own."""
import argparse
import ctypes as C
import importlib
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM = 6.3e12
FIRST_FRAME_US = {"1080p": 1670.0}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--settle", type=float, default=1.0, help="seconds of back-to-back calls before timing")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    pkg = importlib.import_module("bwd-nlkalman_amd")
    synth = importlib.import_module("bwd-nlkalman_amd.synth")
    if pkg.hip().nlk_device_count() < 1:
        raise SystemExit("sigma_time: no HIP device (there is nothing to time without one)")
    ctx = pkg.Context(0)
    stream = torch.cuda.Stream()
    ctx.set_stream(stream.cuda_stream)
    ch, rows = 3, []
    prm = pkg.sigma_params()
    for name, (w, h) in (("1080p", (1920, 1080)), ("4K", (3840, 2160))):
        clean = synth.clean_frame(w, h, ch)
        d_img = ctx.upload(clean)
        ctx.awgn(d_img, d_img, clean.size, 20.0, 1)
        d_out = ctx.alloc(4 * (1 + 3 * ch))

        def call():
            ctx._chk(ctx.L.nlk_dev_estimate_sigma(ctx.h, d_out, d_out + 4 * (1 + ch), d_img, w, h, ch, C.byref(prm)))

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
        sigma = ctx.download(d_out, (1 + ch,))
        counts = ctx.download(d_out + 4 * (1 + ch), (ch, 2), "int32")
        nbytes = w * h * ch * 4
        rate = nbytes / (us * 1e-6)
        row = {"size": name, "w": w, "h": h, "ch": ch, "us": round(us, 2), "bytes": nbytes,
               "GBps": round(rate / 1e9, 1), "of_hbm": round(rate / HBM, 3), "sigma": [float(v) for v in sigma],
               "blocks": int(counts[0, 0]), "selected": int(counts[0, 1])}
        line = (f"{name:6s} estimate_sigma {us:8.2f} us  {rate / 1e9:8.1f} GB/s  {rate / HBM:6.1%} of 6.3 TB/s"
                f"   sigma {sigma[0]:.4f} (true 20), {row['selected']} of {row['blocks']} blocks per channel")
        if name in FIRST_FRAME_US:
            row["of_first_frame"] = round(us / FIRST_FRAME_US[name], 4)
            line += f"   {us / FIRST_FRAME_US[name]:.1%} of the first frame's {FIRST_FRAME_US[name] / 1e3:.2f} ms"
        rows.append(row)
        print(line, flush=True)
        ctx.free(d_img)
        ctx.free(d_out)
    if a.json:
        with open(a.json, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "iters": a.iters, "rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
