"""Times the two colour-conversion kernels (nlk_dev_yuv_to_rgb / nlk_dev_rgb_to_yuv) at 1080p, 4:2:0 8 bit, 4:2:0
10 bit and 4:4:4 8 bit, with HIP events after a clock-settle phase, and prints the rate of their algorithmic bytes
(the code planes once plus the float image once; the frame stays in the Infinity Cache between calls, so these are
cache-resident rates, to be compared with each other and not with the HBM roof) beside nlk_dev_opp2rgb and nlk_dev_awgn on the same RGB frame: the
existing one-pass kernels over the same 25 MB. Then the wall time per frame of `nlkalman-y4m 20` on a 60-frame 1080p
4:2:0 stream in a memory-backed folder, against `nlkalman-seq ... no` on the same frames as float TIFF files (what
there was for the same job before), and of `nlkalman-y4m --copy` (transport and conversion alone).

    python tools/y4m_time.py [--iters N] [--frames N] [--no-tools] [--json FILE]"""
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


def timed(ctx, stream, call, iters, settle):
    t_end = time.perf_counter() + settle             # clock settle (code objects loaded)
    while time.perf_counter() < t_end:
        for _ in range(20):
            call()
        ctx.sync()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    for _ in range(iters):
        call()
    e1.record(stream)
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters


def kernels(pkg, synth, a):
    ctx = pkg.Context(0)
    stream = torch.cuda.Stream()
    ctx.set_stream(stream.cuda_stream)
    w, h, ch = 1920, 1080, 3
    rgb = synth.clean_frame(w, h, ch)
    d_rgb, d_out = ctx.upload(rgb), ctx.alloc(rgb.nbytes)
    rows = []

    def report(name, us, nbytes):
        rate = nbytes / (us * 1e-6)
        rows.append({"call": name, "us": round(us, 2), "bytes": nbytes, "GBps": round(rate / 1e9, 1)})
        print(f"1080p  {name:28s} {us:8.2f} us  {nbytes / 1e6:6.1f} MB  {rate / 1e9:8.1f} GB/s", flush=True)

    for tag in ("420jpeg", "420p10", "444"):
        f = pkg.yuv_format_from_tag(tag)
        nb = f.frame_bytes(w, h)
        d_yuv = ctx.alloc(nb)
        ctx.rgb_to_yuv_dev(d_yuv, d_rgb, w, h, f)
        report("yuv_to_rgb " + tag, timed(ctx, stream, lambda: ctx.yuv_to_rgb_dev(d_out, d_yuv, w, h, f), a.iters, a.settle),
               nb + rgb.nbytes)
        report("rgb_to_yuv " + tag, timed(ctx, stream, lambda: ctx.rgb_to_yuv_dev(d_yuv, d_rgb, w, h, f), a.iters, a.settle),
               nb + rgb.nbytes)
        ctx.free(d_yuv)
    ctx.d2d(d_out, d_rgb, rgb.nbytes)
    report("opp2rgb (in place)", timed(ctx, stream, lambda: ctx.opp2rgb(d_out, w, h, ch), a.iters, a.settle), 2 * rgb.nbytes)
    report("awgn", timed(ctx, stream, lambda: ctx.awgn(d_out, d_rgb, rgb.size, 20.0, 1), a.iters, a.settle), 2 * rgb.nbytes)
    ctx.free(d_rgb)
    ctx.free(d_out)
    ctx.close()
    return rows


def tools(pkg, synth, a):
    import yuv_ref as R
    from test_cli import wpfm
    w, h, n = 1920, 1080, a.frames
    base = "/dev/shm" if os.path.isdir("/dev/shm") and os.access("/dev/shm", os.W_OK) else None
    tmp = tempfile.mkdtemp(prefix="y4m_time_", dir=base)
    rows = []
    try:
        ctx = pkg.Context(0)
        cf = pkg.yuv_format_from_tag("420jpeg")
        os.mkdir(os.path.join(tmp, "in"))
        base_frame = synth.clean_frame(w, h, 3)
        with open(os.path.join(tmp, "in.y4m"), "wb") as s:
            s.write(R.y4m_header(w, h, "420jpeg"))
            for t in range(n):                        # a pan of 2 pixels per frame, noise of sigma 20 made on the GPU
                clean = np.ascontiguousarray(np.roll(base_frame, -2 * t, axis=1))
                d_clean = ctx.upload(clean)
                ctx.awgn(d_clean, d_clean, clean.size, 20.0, 100 + t)
                pay = ctx.rgb_to_yuv(ctx.download(d_clean, clean.shape), cf)
                ctx.free(d_clean)
                s.write(b"FRAME\n" + pay.tobytes())
                # the same frame as the filter sees it, as a float TIFF for nlkalman-seq
                pfm = os.path.join(tmp, "f.pfm")
                wpfm(pfm, ctx.yuv_to_rgb(pay, w, h, cf))
                subprocess.check_call([os.path.join(BIN, "nlk-imgconv"), pfm, os.path.join(tmp, "in", "%03d.tif" % (t + 1))],
                                      stdout=subprocess.DEVNULL)
        ctx.close()
        runs = (("nlkalman-y4m 20", [os.path.join(BIN, "nlkalman-y4m"), "20", os.path.join(tmp, "in.y4m"), os.path.join(tmp, "out.y4m")]),
                ("nlkalman-y4m --copy", [os.path.join(BIN, "nlkalman-y4m"), "--copy", "0", os.path.join(tmp, "in.y4m"), os.path.join(tmp, "copy.y4m")]),
                ("nlkalman-seq ... no (float TIFF)", [os.path.join(BIN, "nlkalman-seq"), os.path.join(tmp, "in", "%03d.tif"), "1", str(n), "20",
                                                       os.path.join(tmp, "seq"), "1", "", "no"]))
        for name, cmd in runs:
            best = None
            for _ in range(2):                        # (the first run also pays for a cold page cache)
                t0 = time.perf_counter()
                r = subprocess.run(cmd, capture_output=True, timeout=900)
                dt = time.perf_counter() - t0
                if r.returncode:
                    raise SystemExit(f"y4m_time: {name} failed: {r.stderr.decode()[-400:]}")
                best = dt if best is None else min(best, dt)
            rows.append({"run": name, "frames": n, "wall_s": round(best, 3), "ms_per_frame": round(best * 1e3 / n, 2)})
            print(f"1080p x {n}  {name:34s} {best:7.2f} s  {best * 1e3 / n:8.2f} ms / frame (process start included)", flush=True)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=2000, help="calls per timed window (the kernels take microseconds)")
    ap.add_argument("--settle", type=float, default=1.0, help="seconds of back-to-back calls before timing")
    ap.add_argument("--frames", type=int, default=60)
    ap.add_argument("--no-tools", action="store_true")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    pkg = importlib.import_module("bwd-nlkalman_amd")
    synth = importlib.import_module("bwd-nlkalman_amd.synth")
    if pkg.hip().nlk_device_count() < 1:
        raise SystemExit("y4m_time: no HIP device (there is nothing to time without one)")
    out = {"device": torch.cuda.get_device_name(0), "iters": a.iters, "kernels": kernels(pkg, synth, a)}
    if not a.no_tools:
        out["tools"] = tools(pkg, synth, a)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
