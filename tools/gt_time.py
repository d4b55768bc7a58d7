"""Wall time per frame of bin/nlkalman-seq-gt against bin/nlkalman-seq on the same noisy frames: a 1080p RGB
sequence of synth.clean_frame frames, the two tools run alternately in one process tree.

    python tools/gt_time.py [--frames N] [--rounds R] [--json FILE] [--keep DIR]

A first gt run writes the noisy frames (OUT/%03d.tif, SRAND 0); every nlkalman-seq run reads those, every gt run
starts from an empty output folder and so makes the noise itself (nlk_dev_awgn), measures each output
(nlk_dev_sqdiff_sum) and writes PNG where nlkalman-seq writes float TIFF. Both run with their default parameters
(smoothing on). Under `rocprofv3 --kernel-trace --stats -- python tools/gt_time.py --rounds 0` only the first gt
run happens: the kernel statistics of one 10-frame ground-truth loop."""
import argparse
import importlib
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
BIN = os.path.join(ROOT, "bwd-nlkalman_amd", "bin")


def run(args, env):
    t0 = time.perf_counter()
    r = subprocess.run(args, capture_output=True, text=True, env=env, timeout=600)
    dt = time.perf_counter() - t0
    if r.returncode:
        raise SystemExit(f"{args[0]} failed ({r.returncode}): {r.stderr}")
    return dt, r.stdout


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--sigma", type=float, default=20.0)
    ap.add_argument("--json", default=None)
    ap.add_argument("--keep", default=None, help="work in this folder and keep it")
    a = ap.parse_args()
    synth = importlib.import_module("bwd-nlkalman_amd.synth")
    from test_cli import wpfm

    work = a.keep or tempfile.mkdtemp(prefix="gt_time")
    os.makedirs(os.path.join(work, "clean"), exist_ok=True)
    for i in range(1, a.frames + 1):
        wpfm(os.path.join(work, "clean", "%03d.pfm" % i), synth.clean_frame(1920, 1080, 3, i))
    env = dict(os.environ, SRAND="0")
    clean, noisy = os.path.join(work, "clean", "%03d.pfm"), os.path.join(work, "noisy")
    shutil.rmtree(noisy, ignore_errors=True)
    first, line = run([os.path.join(BIN, "nlkalman-seq-gt"), clean, "1", str(a.frames), str(a.sigma), noisy], env)
    print(f"first gt run: {first:.3f} s, stdout {line.strip()}")
    seq_t, gt_t = [], []
    for r in range(a.rounds):
        for tool in ("nlkalman-seq", "nlkalman-seq-gt"):
            out = os.path.join(work, "out")
            shutil.rmtree(out, ignore_errors=True)
            if tool == "nlkalman-seq":
                dt, _ = run([os.path.join(BIN, tool), os.path.join(noisy, "%03d.tif"), "1", str(a.frames),
                             str(a.sigma), out], env)
                seq_t.append(dt)
            else:
                dt, _ = run([os.path.join(BIN, tool), clean, "1", str(a.frames), str(a.sigma), out], env)
                gt_t.append(dt)
            print(f"round {r} {tool:16s} {dt:.3f} s  {1e3 * dt / a.frames:.1f} ms/frame")
    res = {"frames": a.frames, "size": "1920x1080x3", "rounds": a.rounds, "seq_s": seq_t, "gt_s": gt_t}
    if a.rounds:
        ms, mg = statistics.median(seq_t), statistics.median(gt_t)
        res.update(seq_ms_per_frame=1e3 * ms / a.frames, gt_ms_per_frame=1e3 * mg / a.frames, ratio=mg / ms)
        print(f"median per frame: nlkalman-seq {res['seq_ms_per_frame']:.1f} ms, nlkalman-seq-gt "
              f"{res['gt_ms_per_frame']:.1f} ms, ratio {res['ratio']:.3f} (process start included)")
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)
    if not a.keep:
        shutil.rmtree(work, ignore_errors=True)


if __name__ == "__main__":
    main()
