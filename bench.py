#!/usr/bin/env python3
"""bench.py — Mpix/s per frame of the NL-Kalman hot path (nlkalman-flt, FLT1
temporal) on synthetic AWGN frames, BASELINE.json configs[1]: 1920x1080 RGB,
sigma = 20, 8x8 patches.

  python bench.py --gpus N --steps K --warmup W
  python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N ...

A step = one nlkalman_filter_frame() of one frame with every input already in
HBM. With N > 1 the frame is split into N row strips of the patch grid (one
process per GPU, bwd-nlkalman_amd/strips.py): halo rows of the previous
denoised frame and of the accumulators travel between neighbours by RCCL
send/recv over xGMI, and the per-target mark words are all-gathered so that
every rank replays the exact serial processed-mask. Total work is fixed, so
scaling is "strong".
Rank 0 prints ONE JSON line.

A plain run sets up, warms up, times the K steps and prints the line (metric,
value, ms_per_step, ...). --full adds what takes runs of its own: per-kernel
times, the roofline, the CPU baseline and the parity / PSNR comparison with
the CPU oracle, the first-frame and host-API times (--no-cpu / --no-extras
drop parts of it). --dump-outputs DIR writes what the last timed step computed
as DIR/<name>.npy (float32); the inputs are seeded, the same on every run.
"""
import argparse
import importlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
T_PROCESS_START = __import__("time").time()
sys.path.insert(0, ROOT)

WORKLOADS = {
    # name: (w, h, ch, sigma, patch, seed)   — BASELINE.json configs
    "C1": (256, 256, 1, 20.0, 8, 0),
    # C1L: a single-channel frame at the real size (the reference's own published numbers are on *_mono sequences,
    # scripts/dev-scripts/best-results.sh:60-61)
    "C1L": (1920, 1080, 1, 20.0, 8, 9),
    "C2": (1920, 1080, 3, 20.0, 8, 1),
    "C3": (3840, 2160, 3, 40.0, 12, 2),
    # C5: the full per-frame chain flt1 -> flt2 -> smo1 on resident frames (single GPU only)
    "C5": (1920, 1080, 3, 20.0, 8, 1),
    # F1: the optical flow the pipelines compute before every temporal call:
    # tvl1flow with its default parameters between two noisy 1080p frames
    "F1": (1920, 1080, 3, 20.0, 8, 1),
    # S1: one frame of the pipelines' forward recursion, frames resident:
    # flow + occlusion mask + 2 warps + FLT1 + FLT2 (bwd-nlkalman_amd/sequence.py)
    "S1": (1920, 1080, 3, 20.0, 8, 1),
}
_JSON_FD = 1


def emit(res):
    os.write(_JSON_FD, (json.dumps(res) + "\n").encode())


DUMP_BYTES = 60 << 20    # --dump-outputs: at most this many bytes of arrays in all (< 64 MB)


def dump_outputs(path, arrays):
    """--dump-outputs: one <path>/<name>.npy (float32) per array of {name: host array}. If they hold more than
    DUMP_BYTES together, each is replaced by the same fixed, seeded sample of its flattened elements (its share of
    the budget), so that two builds are compared element for element."""
    import numpy as np
    os.makedirs(path, exist_ok=True)
    total = sum(a.size * 4 for a in arrays.values())
    for name, a in arrays.items():
        a = np.ascontiguousarray(a, dtype=np.float32)
        if total > DUMP_BYTES:
            n = a.size * DUMP_BYTES // total
            a = a.reshape(-1)[np.sort(np.random.default_rng(20240).choice(a.size, n, replace=False))]
        np.save(os.path.join(path, name + ".npy"), a)


HBM_PEAK_GBS = 8000.0       # MI355X_MICROARCH.md: HBM3E peak 8 TB/s
MFMA_F32_PEAK_TFLOPS = 157.3    # MI355X_MICROARCH.md: dense f32 MFMA peak (= the f32 vector peak)


def cpu_model():
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown"


def cpu_baseline(O, o1, prev, sigma, p, reps=5):
    """The CPU restatement ("port": oracle/nlk_oracle.c, its DCT a table product - FFTW, which the reference
    uses, is absent from the image) with OpenMP over the host cores on full frames of the same workload, in two
    builds: the strict one the parity legs use and one with the flags the reference is released with
    (CMakeLists.txt:10). One warm-up frame, then the median of `reps` frames each; `value` = the FASTER build."""
    nthr = min(O.max_threads(), os.cpu_count() or 1, 100)  # the reference aborts above 100
    po = O.Params(*[getattr(p, k) for k, _ in p._fields_])
    h, w = o1.shape[:2]
    builds = {}
    out = None
    for name, flags, fn in (("strict", O.STRICT_FLAGS, None), ("release", O.RELEASE_FLAGS, O.release_filter_frame())):
        run = ((lambda: O.filter_frame(o1, prev, None, sigma, po, nthreads=nthr)) if fn is None
               else (lambda: O.filter_frame_with(fn, o1, prev, None, sigma, po, nthreads=nthr)))
        t0 = time.time()
        res = run()  # warm-up (pages, thread pool)
        tw = time.time() - t0
        if fn is None:
            out = res
        nrep = max(1, min(reps, int(8.0 / max(tw, 1e-3))))  # (bounded: ~8 s per build; 5 at 1080p on the GPU box)
        ts = []
        for _ in range(nrep):
            t0 = time.time()
            run()
            ts.append(time.time() - t0)
        ts.sort()
        builds[name] = {"flags": flags, "frames_timed": nrep, "median_s": round(ts[len(ts) // 2], 4), "min_s": round(ts[0], 4),
                        "mpix_s": round(w * h / ts[len(ts) // 2] / 1e6, 4)}
    best = max(builds, key=lambda b: builds[b]["mpix_s"])
    return out, {"value": builds[best]["mpix_s"], "unit": "Mpix/s", "cores": nthr, "kind": "port",
                 "flags": builds[best]["flags"], "build": best, "dct": "table (FFTW absent)",
                 "cpu": cpu_model(), "threads": nthr, "builds": builds,
                 "sample": f"full frames {w}x{h}x{o1.shape[2]} FLT1-temporal, OpenMP over {nthr} threads of "
                           f"{cpu_model()}: 1 warm-up + median of {builds[best]['frames_timed']} per build; oracle/nlk_oracle.c "
                           f"(table DCT, FFTW absent) built strict ({O.STRICT_FLAGS}) and with the reference's "
                           f"release flags ({O.RELEASE_FLAGS}); value = the faster ({best}) build"}


def kernel_sources_sha():
    """sha256 over the HIP sources of the product (csrc/*.h, *.hip) and the lines of the Makefile that hold their
    compiler flags (HIPFLAGS, per-unit scheduling): what a PMC table was measured on."""
    import glob
    import hashlib
    hsh = hashlib.sha256()
    for f in sorted(glob.glob(os.path.join(ROOT, "bwd-nlkalman_amd", "csrc", "*"))):
        if f.endswith((".h", ".hip")):
            hsh.update(os.path.basename(f).encode())
            hsh.update(open(f, "rb").read())
    for line in open(os.path.join(ROOT, "bwd-nlkalman_amd", "Makefile"), "rb"):
        if any(k in line for k in (b"HIPFLAGS", b"SCHED", b"HIPCC")) and not line.lstrip().startswith(b"#"):
            hsh.update(line)
    return hsh.hexdigest()


def measured_traffic(workload, instance, largest_grid=False):
    """HBM-side bytes per launch of kernel `instance` (full template name, e.g. "k_bm_topk<8, 3, 2>": the
    instantiation this run timed) from the committed PMC passes (profiles/<tag>_traffic.json, made by
    tools/profile_round.sh + tools/make_traffic.py; tag = NLK_TRAFFIC_TAG, default r06) - only while the
    kernel sources are still the ones the table was measured on; otherwise (None, why)."""
    tag = os.environ.get("NLK_TRAFFIC_TAG", "r06")
    tpath = os.path.join(ROOT, "profiles", f"{tag}_traffic.json")
    if not os.path.exists(tpath):
        return None, f"no PMC table profiles/{tag}_traffic.json committed"
    tab = json.load(open(tpath))
    if tab.get("kernel_sources_sha256") != kernel_sources_sha():
        return None, (f"the kernel sources differ from the ones profiles/{tag}_traffic.json was measured on "
                      f"(git {tab.get('git_head', '?')[:10]}): re-run tools/profile_round.sh")
    ents = tab.get("workloads", {}).get(workload, {})
    ent = ents.get(instance)
    if ent is None:
        # a kernel family with one instance per launch shape (largest_grid: the full-size one), or an instance named
        # without its trailing template arguments (k_bm_topk<8, 3, 2> for k_bm_topk<8, 3, 2, 2, 0>)
        stem = instance if largest_grid else instance.rstrip(">") + ","
        fam = [e for k_, e in ents.items() if k_.startswith(stem)]
        ent = max(fam, key=lambda e: (e["launches_per_pass"], e["traffic_bytes"]) if not largest_grid else e["traffic_bytes"]) if fam else None
    if not ent:
        return None, f"no entry for {instance} at {workload}"
    return ent["traffic_bytes"], (f"FETCH_SIZE + WRITE_SIZE per launch of {ent['instance']} ({ent['launch_shape']}, "
                                  f"{ent['launches_per_pass']} launches), git {tab['git_head'][:10]} "
                                  f"(fetch x2 bound: {ent['traffic_bytes_fetch_x2']:.4g})")


def c5_roofline(c5, w, h, ch, psz, ngrid, ps):
    """Roofline object of config 5's dominant launch: the smoother's group kernel (`k_group8m<CH, true, ...>`, the
    largest single launch of the chain). Algorithmic flops from the launch's records with the terms of SURVEY.md
    Appendix B: per processed target with previous-frame patches, forward transforms of the kept candidates' image
    patches (M1, V1 over all of them, `src/nlkalman.c:1646-1658`) and of the valid previous-frame patches (M0, V0, V01,
    group slots, `:1659-1676`), inverse transforms of the group members (`:1780`), `2 psz^3` MACs per channel each;
    statistics 16 flop per coefficient and candidate, gains 68 per coefficient, aggregation 2 per member pixel and
    plane. A target without a valid previous patch aggregates its own patch unchanged (`:1795-1804`): no transform."""
    import numpy as np
    rec, tm = c5["smo1"]["rec"], c5["smo1"]["ms"]
    act = rec["active"].astype(bool) & (rec["nagg"] > 0)
    nsel, np0, nagg = (rec[k_][act].astype(np.float64) for k_ in ("nsel", "np0", "nagg"))
    hp = np0 > 0
    ntr = float(((nsel + np0 + nagg) * hp).sum())
    group_flops = ntr * ch * 2 * 2 * psz ** 3
    other = float(((nsel * ch * psz * psz * 16 + ch * psz * psz * 68) * hp + nagg * psz * psz * (ch + 1) * 2).sum())
    dur = tm["group_ms"] * 1e-3
    k = ps.npatches_t
    alg_bytes = 2 * w * h * ch * 4 + (ch + 1) * w * h * 4 + ngrid * k * 4
    sep = os.environ.get("NLK_GROUP_SEP", "6" if ch == 1 else "2")   # (tu_group8.hip: the separable pass B on the difference image)
    inst = f"k_group8m<{ch}, true, {sep}, 0>"
    traffic, traffic_note = measured_traffic("C5", inst)
    tfl = group_flops / dur / 1e12 if dur > 0 else 0.0
    chain = sum(c5[n_]["ms"]["total_ms"] for n_ in c5)
    return {"kernel": inst, "what": "the smoother's group launch: the largest single launch of the chain "
                                    f"({tm['group_ms']:.3f} of {chain:.3f} ms of kernels per step)",
            "bound": "mfma", "achieved": round(tfl, 3), "peak": MFMA_F32_PEAK_TFLOPS, "unit": "TFLOP/s",
            "frac": round(tfl / MFMA_F32_PEAK_TFLOPS, 4), "traffic": traffic, "traffic_note": traffic_note,
            "launch_ms": round(tm["group_ms"], 4),
            "frac_all_survey_terms": round((group_flops + other) / dur / 1e12 / MFMA_F32_PEAK_TFLOPS, 4) if dur > 0 else None,
            "algorithmic_flops_per_launch": int(group_flops), "algorithmic_bytes_per_launch": int(alg_bytes),
            "targets": {"processed": int(act.sum()), "with_previous_patches": int(hp.sum()),
                        "mean_candidates": round(float(nsel[hp].mean()) if hp.any() else 0.0, 2),
                        "mean_members": round(float(nagg[hp].mean()) if hp.any() else 0.0, 2)},
            "hbm": {"achieved": round(alg_bytes / dur / 1e9, 3) if dur > 0 else 0.0, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                    "frac": round(alg_bytes / dur / 1e9 / HBM_PEAK_GBS, 6) if dur > 0 else 0.0},
            "valu": {"achieved": round(other / dur / 1e12, 3) if dur > 0 else 0.0, "peak": MFMA_F32_PEAK_TFLOPS, "unit": "TFLOP/s",
                     "frac": round(other / dur / 1e12 / MFMA_F32_PEAK_TFLOPS, 4) if dur > 0 else 0.0,
                     "what": "statistics 16 flop per coefficient and candidate, gains 68 per coefficient, aggregation 2 per "
                             "member pixel and plane (estimate), over the same launch time"},
            "other_launches": {n_: {"group_ms": round(c5[n_]["ms"]["group_ms"], 4), "match_ms": round(c5[n_]["ms"]["match_ms"], 4)}
                               for n_ in ("flt1", "flt2")},
            "note": "frac = transform flops only (matrix cores) over the launch's mean time from HIP events on the "
                    "context's stream; compute bound like the filter's group launch (DESIGN.md \u00a75)"}


def cpu_baseline_chain(O, o1, prev, sigma, p1, p2, ps, reps=3):
    """Config 5's chain - flt1 temporal, flt2 on its basic estimate, smo1 - on the CPU restatement built with the
    reference's release flags, OpenMP over the host cores: one warm-up chain, then the median of `reps`."""
    nthr = min(O.max_threads(), os.cpu_count() or 1, 100)
    fn = O.release_filter_frame()
    cv = lambda p_: O.Params(*[getattr(p_, k) for k, _ in p_._fields_])
    h, w = o1.shape[:2]

    def chain():
        f1 = O.filter_frame_with(fn, o1, prev, None, sigma, cv(p1), nthreads=nthr)
        f2 = O.filter_frame_with(fn, o1, prev, f1, sigma, cv(p2), nthreads=nthr)
        return O.smooth_frame(prev, f2, None, sigma, cv(ps), nthreads=nthr)
    chain()
    ts = []
    for _ in range(reps):
        t0 = time.time()
        chain()
        ts.append(time.time() - t0)
    ts.sort()
    med = ts[len(ts) // 2]
    return {"value": round(w * h / med / 1e6, 4), "unit": "Mpix/s", "cores": nthr, "kind": "port",
            "flags": O.RELEASE_FLAGS + " (the two filter calls); " + O.STRICT_FLAGS + " (the smoother)",
            "dct": "table (FFTW absent)", "cpu": cpu_model(), "threads": nthr, "median_s": round(med, 4),
            "sample": f"full chains flt1 -> flt2 -> smo1 on {w}x{h}x{o1.shape[2]} frames, OpenMP over {nthr} threads: "
                      f"1 warm-up + median of {reps}; oracle/nlk_oracle.c (table DCT, FFTW absent)"}


def settle_steps(w, h, ch, ms_1080p_rgb=1.0):
    """Untimed steps in front of the warm-up steps: ~80 ms of the step, so that the timed loop runs at settled clocks
    (the GPU takes ~25 ms of sustained load after an idle phase: DESIGN.md §5, profiles/r05_step_trace.txt). A fixed
    number by frame size - every rank runs the same. NLK_BENCH_SETTLE_STEPS overrides (0: none)."""
    return int(os.environ.get("NLK_BENCH_SETTLE_STEPS",
                              min(2000, max(16, round(80.0 / (ms_1080p_rgb * w * h * ch / (1920 * 1080 * 3.0)))))))


def bench_flow(args, pkg, synth, ctx, torch, dist, rank, world, dev):
    """Workload F1: one step = one multiscale TV-L1 flow between two resident gray frames.
    The path does not shard (every iteration couples the whole image): N > 1 runs N independent
    replicas on different frame pairs ("replicas only")."""
    import ctypes as C
    import numpy as np
    w, h, ch, sigma, _, seed = WORKLOADS["F1"]
    n0, n1, _ = synth.noisy_pair(w, h, ch, sigma, seed + rank)
    t0_, t1_ = torch.from_numpy(n0).to(dev), torch.from_numpy(n1).to(dev)
    g0 = torch.empty((h, w), dtype=torch.float32, device=dev)
    g1 = torch.empty_like(g0)
    ctx.gray(g0.data_ptr(), t0_.data_ptr(), w, h, ch)
    ctx.gray(g1.data_ptr(), t1_.data_ptr(), w, h, ch)
    flow = torch.empty((h, w, 2), dtype=torch.float32, device=dev)
    prm = pkg.tvl1_params(w, h)

    def barrier():
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()
    iters = 0
    settle = settle_steps(w, h, 3, 6.0)
    for _ in range(settle + args.warmup):
        iters = ctx.tvl1_flow(flow.data_ptr(), g0.data_ptr(), g1.data_ptr(), w, h, prm)
    barrier()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        ctx.L.nlk_dev_tvl1_flow(ctx.h, flow.data_ptr(), g0.data_ptr(), g1.data_ptr(), w, h,
                                C.byref(prm), None)
    barrier()
    dt = time.perf_counter() - t0
    if world > 1:
        tt = torch.tensor([dt], dtype=torch.float64, device=dev)
        dist.all_reduce(tt, op=dist.ReduceOp.MAX)
        dt = float(tt.item())
    if rank != 0:
        return
    if args.dump_outputs:      # (before the roofline's run below writes `flow` again)
        dump_outputs(args.dump_outputs, {"flow": flow.cpu().numpy()})
    ms = dt / args.steps * 1e3
    res = {"metric": "Mpix/s per flow (tvl1flow, 1080p, default parameters)", "value": round(world * w * h / (dt / args.steps) / 1e6, 3),
           "unit": "Mpix/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "clock_settle_steps": settle,
           "ms_per_step": round(ms, 4), "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
           "dtype": "f32", "data": "synthetic",
           "config": {"workload": f"F1: dual TV-L1 flow between two {w}x{h} noisy frames (sigma {sigma:g}), "
                                  f"tau 0.25 lambda 0.15 theta 0.3, {prm.nscales} scales, 5 warps, epsilon 0.01",
                      "parallelism": "single GPU" if world == 1 else f"{world} independent replicas",
                      "iterations": iters}}
    if not args.full:
        emit(res)
        return
    # roofline of the dominant kernel (k_tv_block at full size): a one-level run is nothing but
    # its iterations (+ 5 warps). Algorithmic bytes: an iteration reads 16 and writes 6 floats per
    # pixel = 88 B; the kernel runs 4 iterations per launch on LDS tiles, so its real
    # traffic is about a quarter of that and it is bound by LDS + VALU instead
    one = pkg.tvl1_params(w, h)
    one.nscales = 1
    it1 = ctx.tvl1_flow(flow.data_ptr(), g0.data_ptr(), g1.data_ptr(), w, h, one)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    reps = 3
    for _ in range(reps):
        ctx.L.nlk_dev_tvl1_flow(ctx.h, flow.data_ptr(), g0.data_ptr(), g1.data_ptr(), w, h, C.byref(one), None)
    torch.cuda.synchronize()
    t_iter = (time.perf_counter() - t1) / reps / max(it1, 1)
    # ALGORITHMIC bytes of the kernel as built: it advances 4 iterations per launch on LDS tiles, so the
    # compulsory traffic of a launch is one read of the 16 and one write of the 6 state floats per pixel = 88 B per
    # 4 iterations = 22 B per pixel and iteration. (The plain recursion - one launch per iteration - would move
    # 88 B per pixel and iteration: reported beside it as the equivalent bandwidth, which may exceed the HBM peak
    # and is NOT an HBM fraction: VERDICT r3, weak 11.)
    gbs = 22.0 * w * h / t_iter / 1e9
    gbs_equiv = 88.0 * w * h / t_iter / 1e9
    # HBM-side bytes per iteration from the committed PMC passes of the same sources (a launch = 4 iterations)
    traffic, traffic_note = (None, "single-GPU runs only") if world > 1 else measured_traffic("F1", "k_tv_block", largest_grid=True)
    traffic = traffic / 4 if traffic else None
    res["roofline"] = {"kernel": "k_tv_block (full-size level, per iteration)", "bound": "hbm",
                       "achieved": round(gbs, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                       "frac": round(gbs / HBM_PEAK_GBS, 4), "traffic": traffic, "traffic_note": traffic_note,
                       "iteration_us": round(t_iter * 1e6, 2), "algorithmic_bytes_per_iteration": 22 * w * h,
                       "traffic_frac": (round(traffic / t_iter / 1e9 / HBM_PEAK_GBS, 4) if traffic else None),
                       "equivalent_unblocked_gbs": round(gbs_equiv, 1),
                       "note": "measured on a one-level run (wall time / iterations; launches, redone "
                               "batches and state read-backs included). achieved = the blocked kernel's "
                               "compulsory bytes (88 B per pixel per 4-iteration launch) / time; traffic_frac = "
                               "PMC-counted bytes / time / peak; equivalent_unblocked_gbs = what a one-launch-"
                               "per-iteration recursion would have to move in the same time (not an HBM fraction)"}
    if not args.no_cpu:
        sys.path.insert(0, os.path.join(ROOT, "oracle"))
        import oracle as O
        a, b = g0.cpu().numpy(), g1.cpu().numpy()
        ref_so = os.path.join(ROOT, "oracle", "_ref", "libtvl1flow_ref.so")
        fl = flow.cpu().numpy()
        if os.path.exists(ref_so):  # the reference's own library (OpenMP), built by `make -C oracle ref`
            L = C.CDLL(ref_so)
            fp, i, f = C.POINTER(C.c_float), C.c_int, C.c_float
            L.Dual_TVL1_optic_flow_multiscale.argtypes = [fp, fp, fp, fp, i, i, f, f, f, i, i, f, i, f, C.c_bool]
            u, v = np.zeros((h, w), np.float32), np.zeros((h, w), np.float32)
            tc = time.time()
            L.Dual_TVL1_optic_flow_multiscale(a.ctypes.data_as(fp), b.ctypes.data_as(fp), u.ctypes.data_as(fp),
                                              v.ctypes.data_as(fp), w, h, prm.tau, prm.lam, prm.theta, prm.nscales,
                                              prm.fscale, prm.zfactor, prm.nwarps, prm.epsilon, False)
            dtc = time.time() - tc
            kind, cores = "reference", min(O.max_threads(), os.cpu_count() or 1)
            sample = f"1 full flow {w}x{h}, lib/tvl1flow built from the reference sources, OpenMP, {dtc:.2f} s wall"
        else:
            sw, sh = 480, 270  # bounded sample for the single-threaded restatement
            a, b = np.ascontiguousarray(a[:sh, :sw]), np.ascontiguousarray(b[:sh, :sw])
            tc = time.time()
            u, v = O.tvl1_flow(a, b)
            dtc = time.time() - tc
            fl = None
            kind, cores = "port", 1
            sample = f"1 flow on a {sw}x{sh} crop, single-threaded restatement, {dtc:.2f} s wall"
            w_, h_ = sw, sh
        npx = (w * h) if kind == "reference" else sw * sh
        res["cpu_baseline"] = {"value": round(npx / dtc / 1e6, 4), "unit": "Mpix/s", "cores": cores,
                               "kind": kind, "sample": sample}
        if fl is not None:
            # (the threaded reference adds its convergence measure in a thread-dependent order, so
            # its own result depends on the thread count; the strict check is the crop below)
            res["max_abs_vs_threaded_reference"] = round(
                float(max(np.abs(fl[..., 0] - u).max(), np.abs(fl[..., 1] - v).max())), 4)
        res["speedup_vs_cpu"] = round(res["value"] / world / res["cpu_baseline"]["value"], 1)
        # parity: the same call on a 480x270 crop against the single-threaded oracle (= the
        # single-threaded reference, bit for bit: tests/test_tvl1.py)
        cw, chh = 480, 270
        ca = np.ascontiguousarray(g0.cpu().numpy()[:chh, :cw])
        cb = np.ascontiguousarray(g1.cpu().numpy()[:chh, :cw])
        cu, cv = O.tvl1_flow(ca, cb)
        ta, tb = torch.from_numpy(ca).to(dev), torch.from_numpy(cb).to(dev)
        tf = torch.empty((chh, cw, 2), dtype=torch.float32, device=dev)
        ctx.tvl1_flow(tf.data_ptr(), ta.data_ptr(), tb.data_ptr(), cw, chh, pkg.tvl1_params(cw, chh))
        cf = tf.cpu().numpy()
        res["parity_crop_480x270"] = {
            "max_abs": round(float(max(np.abs(cf[..., 0] - cu).max(), np.abs(cf[..., 1] - cv).max())), 6),
            "bit_exact": bool(np.array_equal(cf[..., 0], cu) and np.array_equal(cf[..., 1], cv))}
    emit(res)


def bench_sequence(args, pkg, synth, ctx, torch, rank, world, dev):
    """Workload S1: one step = one frame of the forward recursion of scripts/nlkalman-seq.sh on
    resident frames (tvl1flow lambda 0.25 fscale 1 -> mask 0.75 -> warp + FLT1 -> warp + FLT2)."""
    import numpy as np
    seq = importlib.import_module("bwd-nlkalman_amd.sequence")
    if world != 1:
        raise SystemExit("workload S1 is single-GPU (the recursion over frames is sequential)")
    w, h, ch, sigma, _, seed = WORKLOADS["S1"]
    # a short moving sequence with independent noise per frame, cycled (pushing one noisy frame
    # repeatedly would feed the filter its own noise realisation as "previous frame")
    nfr = 4
    cleans = [synth.clean_frame(w, h, ch, t) for t in range(nfr)]
    noisy = [torch.from_numpy(synth.awgn(cleans[t], sigma, seed + t)).to(dev) for t in range(nfr)]
    # one sequence per stream: the flow's coarse levels are latency-bound, so independent sequences
    # overlap well on one GPU (each has its own context = its own HIP stream, and a host thread)
    import threading
    ns = max(1, args.streams)
    ctxs = [ctx] + [pkg.Context(dev.index) for _ in range(ns - 1)]
    if ns > 1:
        ctx.L.nlk_ctx_use_own_stream(ctx.h)
    sfs = [seq.SequenceFilter(c, w, h, ch, sigma, keep_history=False) for c in ctxs]
    torch.cuda.synchronize()

    def run(sf, n, k0):
        for j in range(n):
            sf.push(noisy[(k0 + j) % nfr].data_ptr())
        sf.ctx.sync()
    settle = settle_steps(w, h, ch, 5.0)
    k = 1 + settle + args.warmup
    for sf in sfs:
        run(sf, k, 0)
    t0 = time.perf_counter()
    th = [threading.Thread(target=run, args=(sf, args.steps, k)) for sf in sfs]
    for t in th:
        t.start()
    for t in th:
        t.join()
    dt = (time.perf_counter() - t0) / ns  # time per frame of the aggregate = wall / (steps * ns)
    k += args.steps
    sf = sfs[0]
    ms = dt / args.steps * 1e3
    out = sf.download_rgb(sf.flt2) if args.full or args.dump_outputs else None
    if args.dump_outputs:
        dump_outputs(args.dump_outputs, {"flt2_rgb": out})
    res = {"metric": "Mpix/s per frame (flow + mask + nlkalman-flt x2, 1080p sigma=20, frames resident)",
           "value": round(w * h / (dt / args.steps) / 1e6, 3), "unit": "Mpix/s", "n_gpus": 1,
           "steps": args.steps, "warmup": args.warmup, "clock_settle_steps": settle, "ms_per_step": round(ms, 4), "higher_is_better": True,
           "scaling": "strong", "vs_baseline": None, "dtype": "f32", "data": "synthetic",
           "config": {"workload": f"S1: {w}x{h}x{ch} sigma={sigma:g}, per frame: TV-L1 flow (lambda 0.25, fscale 1: the default of scripts/nlkalman-seq.sh) "
                                  "to the previous FLT2 output, occlusion mask (0.75), warp + FLT1, warp + FLT2 "
                                  "(defaults of nlkalman_default_params), nothing leaves HBM",
                      "parallelism": "single GPU" if ns == 1 else f"single GPU, {ns} concurrent sequences",
                      "flow_iterations_last_frame": sf.flow_iterations[-1]}}
    if args.full:
        c1, n1 = cleans[(k - 1) % nfr], noisy[(k - 1) % nfr].cpu().numpy()
        res["psnr_flt2_db"] = round(float(synth.psnr(out, c1)), 4)
        res["psnr_noisy_db"] = round(float(synth.psnr(n1, c1)), 4)
    if ns == 1 and args.full:
        # where a frame goes: a second, PROFILED pass of the same frames with a device sync after every stage
        # (not part of `value`; the syncs cost the stages their overlap with the host's enqueueing)
        nprof = min(args.steps, 20)
        sf.stage_s = {}
        run(sf, nprof, k)
        res["stages_ms"] = {n_: round(v / nprof * 1e3, 4) for n_, v in sf.stage_s.items()}
        res["stages_ms"]["note"] = ("profiled pass with a device sync after each stage: TV-L1 flow + occlusion mask | bicubic warp + "
                                    "FLT1 | bicubic warp + FLT2 (basic = FLT1)")
        sf.stage_s = None
        # the roofline of the stage's dominant kernel is the F1 line's (`k_tv_block`, the same kernel on the same
        # frame size; this workload starts the pyramid one level lower, fscale 1); the filter launches' are C2's / C5's
        res["roofline"] = None
        res["roofline_note"] = ("the frame is a chain of three stages, each with its own dominant kernel: the flow's k_tv_block "
                                "(bench.py --workload F1 carries its roofline), FLT1's and FLT2's k_group8m (--workload C2 / C5)")
    emit(res)


def descendants(pid):
    """Every live descendant of `pid`, children first, from /proc (no psutil needed: ADVICE r5). The ranks of
    torch.distributed.run sit in sessions of their own, so a killpg of the launcher does not reach them."""
    kids = {}
    for d in os.listdir("/proc"):
        if not d.isdigit():
            continue
        try:
            with open(f"/proc/{d}/stat") as f:
                st = f.read()
            ppid = int(st[st.rindex(")") + 2:].split()[1])    # (the command name may hold spaces and parentheses)
        except (OSError, ValueError, IndexError):
            continue
        kids.setdefault(ppid, []).append(int(d))
    out, todo = [], [pid]
    while todo:
        for k in kids.get(todo.pop(), []):
            out.append(k)
            todo.append(k)
    return out


def kill_tree(proc):
    """SIGKILL for `proc` (a Popen started in its own session), its process group and every descendant; says so
    loudly if somebody survives - fresh ranks must not be started beside ranks that still hold the GPUs."""
    import signal
    victims = descendants(proc.pid)
    try:
        os.killpg(proc.pid, signal.SIGKILL)
    except (ProcessLookupError, PermissionError):
        pass
    for v in victims:
        try:
            os.kill(v, signal.SIGKILL)
        except (ProcessLookupError, PermissionError):
            pass
    deadline = time.time() + 10
    left = victims
    while left and time.time() < deadline:
        left = [v for v in left if os.path.exists(f"/proc/{v}") and "Z" not in _proc_state(v)]
        if left:
            time.sleep(0.1)
    if left:
        print(f"bench.py: could not end the processes {left}: they may still hold the GPUs", file=sys.stderr)
    return not left


def _proc_state(pid):
    try:
        with open(f"/proc/{pid}/stat") as f:
            st = f.read()
        return st[st.rindex(")") + 2:].split()[0]
    except (OSError, ValueError, IndexError):
        return "Z"


def launch_ranks(args):
    """`python bench.py --gpus N` without a launcher: run `python -m torch.distributed.run --nnodes=1
    --nproc-per-node N --master-addr 127.0.0.1 --master-port <free> bench.py <same arguments>` as a
    child process (the ranks are its children). This parent never touches the GPU (no torch import, no
    exec of a process that initialised HIP); it forwards rank 0's single JSON line and returns the
    launcher's exit status, so a failed rank is a non-zero exit.

    The run cannot end without a line because a step HANGS (the C strip driver's neighbour send / recv has never
    met a second device - DESIGN.md §6): the child runs under a time limit (NLK_BENCH_LAUNCH_TIMEOUT seconds;
    default 300 + 120 for the CPU legs of --full + 50 ms per step - a fresh box pages torch in for a minute or two); past
    it, its whole process group is killed and a FRESH child is started with the Python strip driver
    (--strip-driver py; never a process that has touched the GPU re-used or re-exec'ed), and the line says
    which driver produced it and why (`launch`)."""
    import signal
    import socket
    import subprocess
    n = args.gpus
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")   # dmabuf IPC: what RCCL needs on this driver
    limit = float(os.environ.get("NLK_BENCH_LAUNCH_TIMEOUT",
                                 300 + (120 if args.full and not args.no_cpu else 0) + 0.05 * (args.steps + args.warmup)))

    def run_once(extra):
        with socket.socket() as sk:
            sk.bind(("127.0.0.1", 0))
            port = sk.getsockname()[1]
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}",
               "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:] + extra
        proc = subprocess.Popen(cmd, stdout=subprocess.PIPE, text=True, env=env, cwd=ROOT, start_new_session=True)
        try:
            out, _ = proc.communicate(timeout=limit)
            return proc.returncode, out, False
        except subprocess.TimeoutExpired:
            # the launcher AND every rank: the ranks may sit in sessions of their own (a killpg of the launcher's
            # group would leave them running, holding the pipe open), so the descendants are collected first
            if not kill_tree(proc):
                raise SystemExit("bench.py: the hung ranks could not be ended: no fresh ranks are started beside them")
            try:
                out, _ = proc.communicate(timeout=15)
            except subprocess.TimeoutExpired:                                # (somebody still holds the pipe: give it up)
                proc.kill()
                out = ""
            return -9, out or "", True

    launch = {"strip_driver_requested": args.strip_driver, "time_limit_s": round(limit, 1)}
    import tempfile
    mark = os.path.join(tempfile.gettempdir(), f"nlk_bench_stuck_{os.getpid()}")
    if os.path.exists(mark):
        os.remove(mark)
    env["NLK_BENCH_STUCK_FILE"] = mark
    rc, out, timed_out = run_once([])
    # (the ranks' own watchdog over the C driver's first step leaves this file: torch.distributed.run itself only says
    # that a rank failed)
    stuck = rc != 0 and os.path.exists(mark) and not [ln for ln in out.splitlines() if ln.startswith("{")]
    if os.path.exists(mark):
        os.remove(mark)
    if (timed_out or stuck) and args.strip_driver == "c":
        why = (f"the run with the C strip driver did not finish within {limit:.0f} s and was killed" if timed_out else
               "the ranks' watchdog ended the run with the C strip driver: its set-up and first step did not get through")
        print(f"bench.py: {why}; starting fresh ranks with --strip-driver py", file=sys.stderr)
        launch["fallback"] = "py"
        launch["reason"] = why
        rc, out, timed_out = run_once(["--strip-driver", "py"])
    if timed_out:
        print(f"bench.py: the ranks did not finish within {limit:.0f} s: killed, no line", file=sys.stderr)
        return 1
    lines = [ln for ln in out.splitlines() if ln.startswith("{")]
    for ln in out.splitlines():
        if not ln.startswith("{") and ln.strip():
            print(ln, file=sys.stderr)                   # anything else a rank printed is not the line
    if rc == 0 and len(lines) != 1:
        print(f"bench.py: expected one JSON line from rank 0, got {len(lines)}", file=sys.stderr)
        return 1
    for ln in lines:
        try:
            d = json.loads(ln)
            d["launch"] = launch
            ln = json.dumps(d)
        except ValueError:
            pass
        print(ln)
    return rc


def run_preflight(rank):
    """A rank started by somebody else's launcher (the driver's `python -m torch.distributed.run ... bench.py --gpus N`)
    has no parent that could time it out, and a collective that hangs cannot be undone inside the process (the
    watchdog below can only end the rank - and with it the run, without a line). So BEFORE this rank touches its GPU,
    the C strip driver's whole first contact with N devices - communicator, buffers, one step, the self-check against
    the whole-frame call - is tried in a CHILD process per rank (the same command with --steps 1, a rendezvous port of
    its own, its own short watchdog). All children fine: the ranks go on with the C driver. Any child hung, crashed or
    wrong: it is killed with its descendants, and EVERY rank takes the Python driver (agreed by an all-reduce); the
    line says so (`preflight`). Returns {"ok", "seconds", "why"}."""
    import signal
    import subprocess
    import tempfile
    env = dict(os.environ)
    env.pop("TORCHELASTIC_USE_AGENT_STORE", None)     # (the children's rank 0 hosts their store itself)
    env.pop("NLK_BENCH_STUCK_FILE", None)
    # The trial's rendezvous port: rank 0 takes a FREE one from the system (bind to port 0) and hands it to the other
    # ranks through a file named after the launcher they all share (one node: nnodes = 1) - a port computed from
    # MASTER_PORT could be taken, or be the launcher's own store.
    port_file = os.path.join(tempfile.gettempdir(), f"nlk_bench_preflight_{os.getppid()}_{env.get('MASTER_PORT', '0')}.port")
    tport = None
    if rank == 0:
        import socket
        with socket.socket() as sk:
            sk.bind(("127.0.0.1", 0))
            tport = sk.getsockname()[1]
        with open(port_file + ".tmp", "w") as f:
            f.write(str(tport))
        os.replace(port_file + ".tmp", port_file)
    else:
        t_wait = time.time()
        while time.time() - t_wait < 60:
            try:
                if os.path.getmtime(port_file) >= T_PROCESS_START - 5:
                    with open(port_file) as f:
                        tport = int(f.read().strip())
                    break
            except (OSError, ValueError):
                pass
            time.sleep(0.05)
    if tport is None:
        return {"ok": False, "seconds": 0.0, "why": f"rank {rank} did not learn the trial's rendezvous port from rank 0 "
                                                       "(rendezvous, not the C strip driver)"}
    env["MASTER_PORT"] = str(tport)
    env.setdefault("MASTER_ADDR", "127.0.0.1")
    env["NLK_BENCH_C_TRIAL_TIMEOUT"] = os.environ.get("NLK_BENCH_PREFLIGHT_TRIAL", "60")
    limit = float(os.environ.get("NLK_BENCH_PREFLIGHT_TIMEOUT", 240))
    cmd = ([sys.executable, os.path.abspath(__file__)] + sys.argv[1:] +
           ["--preflight-child", "--steps", "1", "--warmup", "0", "--no-cpu", "--no-extras"])
    t0 = time.time()
    with tempfile.TemporaryFile(mode="w+") as errf:
        proc = subprocess.Popen(cmd, stdout=subprocess.DEVNULL, stderr=errf, env=env, cwd=ROOT, start_new_session=True)
        why = None
        try:
            rc = proc.wait(timeout=limit)
            if rc != 0:
                why = f"the trial process of rank {rank} ended with status {rc}"
        except subprocess.TimeoutExpired:
            kill_tree(proc)
            proc.wait()
            why = f"the trial process of rank {rank} did not finish within {limit:.0f} s and was killed"
        if why:
            errf.seek(0)
            tail = errf.read()[-1500:]
            if "ddress already in use" in tail or "EADDRINUSE" in tail:
                why += " (the rendezvous port was taken: a rendezvous failure, not the C strip driver's)"
            sys.stderr.write(f"bench.py: {why}; its last words:\n{tail}\n")
    if rank == 0:
        try:
            os.remove(port_file)
        except OSError:
            pass
    return {"ok": why is None, "seconds": round(time.time() - t0, 1), "why": why}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--workload", default="C2", choices=sorted(WORKLOADS))
    ap.add_argument("--full", action="store_true",
                    help="besides the timed steps: per-kernel times, roofline, CPU baseline, parity / PSNR against the "
                         "CPU oracle, first-frame and host-API times (each in runs of its own; off: the headline only)")
    ap.add_argument("--dump-outputs", metavar="DIR",
                    help="write what the last timed step computed as DIR/<name>.npy (float32, at most 64 MB in all)")
    ap.add_argument("--no-cpu", action="store_true", help="--full: skip the CPU baseline leg")
    ap.add_argument("--streams", type=int, default=1,
                    help="workload S1: independent sequences run concurrently on the GPU (one context, "
                         "HIP stream and host thread each); value = aggregate")
    ap.add_argument("--phase-times", action="store_true",
                    help="row-strip runs (N > 1 or --force-strips): a third, untimed loop that synchronises after "
                         "every phase of a step and reports exchange / match / gather / commit / group / exchange / "
                         "normalise wall times per rank")
    ap.add_argument("--force-strips", action="store_true",
                    help="run the N > 1 strip machinery even at N = 1 (measures its fixed overhead)")
    ap.add_argument("--strip-driver", choices=["c", "py"], default="c",
                    help="row-strip runs: the step enqueued from C (csrc/strips.hip: RCCL called from C, one ctypes call "
                         "per step - the default) or from Python (strips.py over torch.distributed)")
    ap.add_argument("--no-extras", action="store_true",
                    help="--full: skip first_frame_ms / api_wall_ms (profiler passes: only the timed call's kernels run)")
    ap.add_argument("--strip-model", action="store_true",
                    help="N = 1 only: additionally step ONE middle rank of a world of 2 / 4 / 8 alone, every exchange "
                         "skipped (csrc/strips.hip dry run): the kernels + launch gaps one rank pays per frame at that "
                         "world size - an upper bound of the scaling curve a one-GPU box can measure, not a result")
    ap.add_argument("--preflight-child", action="store_true",
                    help="internal: this process is the trial run a rank starts before it uses the C strip driver (run_preflight)")
    ap.add_argument("--strip-graph", action="store_true",
                    help="C strip driver: capture the step into a HIP graph once and replay it")
    args = ap.parse_args()
    if args.preflight_child:
        args.dump_outputs = None    # (the trial step of run_preflight is not the run)

    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # `python bench.py --gpus N` by itself: start the N ranks as CHILD processes before this
        # process makes any GPU call (it never does), forward rank 0's line, exit with their status
        raise SystemExit(launch_ranks(args))

    if os.environ.get("NLK_STRIPS_TEST_HANG") == "early" and args.strip_driver == "c" and "WORLD_SIZE" in os.environ:
        # test hook for boxes without a GPU (tests/test_bench_contract.py): a rank that hangs before it touches anything
        while True:
            time.sleep(3600)

    # The ONE JSON line goes out through a private copy of stdout; whatever else this process writes to file
    # descriptor 1 from here on - librccl prints a five-line version banner there when a communicator is made -
    # goes to stderr instead.
    global _JSON_FD
    sys.stdout.flush()
    _JSON_FD = os.dup(1)
    os.dup2(2, 1)

    import torch
    import torch.distributed as dist

    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}: start it as `python bench.py --gpus {args.gpus}` "
                         f"(launches its own ranks) or with torch.distributed.run --nproc-per-node {args.gpus}")
    one_gpu = os.environ.get("NLK_BENCH_ONE_GPU") == "1"
    if world > 1 and not one_gpu and torch.cuda.device_count() < world:   # device_count() does not initialise HIP
        raise SystemExit(f"--gpus {world} but {torch.cuda.device_count()} HIP device(s) visible "
                         "(NLK_BENCH_ONE_GPU=1 puts every rank on device 0 over gloo: plumbing check, not a measurement)")
    preflight = None
    want_pf = os.environ.get("NLK_BENCH_PREFLIGHT", "1")   # ("0": none; "force": also with every rank on one device)
    if (world > 1 and args.strip_driver == "c" and not args.preflight_child and args.workload not in ("C5", "S1", "F1")
            and want_pf != "0" and (not one_gpu or want_pf == "force")):
        preflight = run_preflight(rank)                    # (child processes: this one has not touched the GPU yet)
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a GPU: the HIP path has no CPU fallback")
    # NLK_BENCH_ONE_GPU=1 (development aid): every rank on device 0 with the gloo backend and host
    # staging, to drive the whole N > 1 code path on a one-GPU box; its numbers mean nothing
    if one_gpu:
        local = 0
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if one_gpu:
            dist.init_process_group("gloo", rank=rank, world_size=world)
        else:
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)

    if preflight is not None:
        okt = torch.tensor([1 if preflight["ok"] else 0], dtype=torch.int32, device="cpu" if one_gpu else dev)
        dist.all_reduce(okt, op=dist.ReduceOp.MIN)
        preflight["ok_on_every_rank"] = int(okt.item()) == 1
        if not preflight["ok_on_every_rank"]:
            if rank == 0:
                print("bench.py: the C strip driver's trial run failed on some rank: every rank takes --strip-driver py",
                      file=sys.stderr)
            args.strip_driver = "py"

    pkg = importlib.import_module("bwd-nlkalman_amd")
    synth = importlib.import_module("bwd-nlkalman_amd.synth")
    strips = importlib.import_module("bwd-nlkalman_amd.strips")
    w, h, ch, sigma, psz, seed = WORKLOADS[args.workload]
    p = pkg.default_params(sigma, pkg.FLT1, patch_sz=psz)
    step = p.patch_sz // 2
    ngx, ngy = (w - psz) // step + 1, (h - psz) // step + 1

    ctx = pkg.Context(local)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    if args.workload == "S1":
        bench_sequence(args, pkg, synth, ctx, torch, rank, world, dev)
        return
    if args.workload == "F1":
        bench_flow(args, pkg, synth, ctx, torch, dist, rank, world, dev)
        if world > 1:
            dist.destroy_process_group()
        return

    # ---- synthetic inputs (every rank builds the same frames; cheap)
    n0, n1, c1 = synth.noisy_pair(w, h, ch, sigma, seed)
    t_n0, t_n1 = torch.from_numpy(n0).to(dev), torch.from_numpy(n1).to(dev)
    ctx.rgb2opp(t_n0.data_ptr(), w, h, ch)
    ctx.rgb2opp(t_n1.data_ptr(), w, h, ch)
    # previous denoised frame = spatial FLT1 of frame 0, unwarped
    t_prev = torch.empty_like(t_n0)
    ctx.filter_frame(t_prev.data_ptr(), t_n0.data_ptr(), None, None, w, h, ch, sigma, p)
    torch.cuda.synchronize()
    t_out = torch.empty_like(t_n1)

    cs, c_driver_note = None, None
    ctx_whole = ctx   # (the strip drivers below may hand `ctx` over to a strip's own context)
    # The C strip driver's first steps run under a watchdog in every rank. Started by a launcher of its own (the
    # driver's `python -m torch.distributed.run ... bench.py --gpus N`) there is no parent to time the ranks out: a
    # step that hangs - the neighbour send / recv between two devices has never run - would hold the job until somebody
    # else's clock ends it. A hung collective cannot be recovered inside the process, so the watchdog ends the rank at
    # once with status 5 and says what to do; `python bench.py --gpus N` (launch_ranks) takes that status, like its own
    # time limit, as the signal to start fresh ranks on the Python driver.
    watchdog = None
    if args.strip_driver == "c" and (world > 1 or args.force_strips) and args.workload != "C5":
        import threading
        trial_s = float(os.environ.get("NLK_BENCH_C_TRIAL_TIMEOUT", 90))

        def _stuck():
            sys.stderr.write(f"bench.py: rank {rank}: the C strip driver did not get through its set-up and first step "
                             f"in {trial_s:.0f} s - a hung collective cannot be undone in this process: exiting with "
                             "status 5 (use --strip-driver py, or `python bench.py --gpus N`, which falls back by itself)\n")
            sys.stderr.flush()
            mark = os.environ.get("NLK_BENCH_STUCK_FILE")   # (launch_ranks: the launcher in between reports only "a rank failed")
            if mark:
                try:
                    open(mark, "w").close()
                except OSError:
                    pass
            os._exit(5)
        watchdog = threading.Timer(trial_s, _stuck)
        watchdog.daemon = True
        watchdog.start()
    if args.strip_driver == "c" and (world > 1 or args.force_strips) and os.environ.get("NLK_STRIPS_TEST_HANG") == "1":
        # test hook: a C strip driver whose first step never returns (tests/test_bench_contract.py: the launcher must
        # kill the ranks and produce the line with the Python driver)
        while True:
            time.sleep(3600)
    if args.workload == "C5":
        if world != 1:
            raise SystemExit("workload C5 is single-GPU")
        p2 = pkg.default_params(sigma, pkg.FLT2, patch_sz=psz)
        ps = pkg.default_params(sigma, pkg.SMO1, patch_sz=psz)
        t_f1, t_f2 = torch.empty_like(t_n1), torch.empty_like(t_n1)

        def one_step():  # temporal flt1, flt2 on its basic estimate, smoother of the previous frame
            ctx.filter_frame(t_f1.data_ptr(), t_n1.data_ptr(), t_prev.data_ptr(), None, w, h, ch, sigma, p)
            ctx.filter_frame(t_f2.data_ptr(), t_n1.data_ptr(), t_prev.data_ptr(), t_f1.data_ptr(),
                             w, h, ch, sigma, p2)
            ctx.smooth_frame(t_out.data_ptr(), t_prev.data_ptr(), t_f2.data_ptr(), None, w, h, ch, sigma, ps)
    elif world == 1 and not args.force_strips:
        def one_step():
            ctx.filter_frame(t_out.data_ptr(), t_n1.data_ptr(), t_prev.data_ptr(), None,
                             w, h, ch, sigma, p)
    else:
        if args.strip_driver == "c" and not one_gpu:
            # the step enqueued from C: rank 0 makes the RCCL id, torch.distributed only carries it to the others.
            # If the C driver cannot be set up on some rank (an error code, e.g. no usable librccl), EVERY rank
            # falls back to the Python driver - agreed on by an all-reduce - and the line says so.
            ident = [None]
            if rank == 0:
                try:
                    ident = [pkg.Strips.unique_id()]
                except Exception as e:                                       # noqa: BLE001
                    c_driver_note = f"C strip driver not usable on rank 0: {e}"
            if world > 1:
                dist.broadcast_object_list(ident, src=0)                     # (every rank takes part, whatever happened)
            def everybody(ok):   # (the communicator's creation is collective: nobody enters it unless everybody can)
                if world == 1:
                    return ok
                okt = torch.tensor([1 if ok else 0], dtype=torch.int32, device=dev)
                dist.all_reduce(okt, op=dist.ReduceOp.MIN)
                return int(okt.item()) == 1
            try:
                if ident[0] is None:
                    raise RuntimeError("no RCCL id from rank 0")
                cs = pkg.Strips([local], rank, world, w, h, ch, sigma, p)        # local: buffers, contexts
            except Exception as e:                                           # noqa: BLE001
                c_driver_note = c_driver_note or f"C strip driver not usable on rank {rank}: {e}"
                cs = None
            if everybody(cs is not None):
                try:
                    cs.rccl_init(ident[0])                                   # collective: ncclCommInitRank
                    cs.set_options(overlap=False, timing=False, graph=args.strip_graph)
                    cs.load(0, t_n1.data_ptr(), t_prev.data_ptr())
                    ok = True
                except Exception as e:                                       # noqa: BLE001
                    c_driver_note, ok = f"C strip driver: RCCL set-up failed on rank {rank}: {e}", False
                if not everybody(ok):
                    c_driver_note = c_driver_note or "C strip driver: RCCL set-up failed on another rank"
                    cs.close()
                    cs = None
            elif cs is not None:
                cs.close()
                cs, c_driver_note = None, "C strip driver not usable on another rank"
        if cs is not None:
            ctx = pkg.Context.from_handle(cs.L.nlk_strips_ctx(cs.h, 0))   # the strip's own context: its timings and records
            one_step = cs.step
    if cs is None and (world > 1 or args.force_strips) and args.workload != "C5":
        def accumulate(acc, cur, prev, oy, ngy_):
            ctx.frame_accumulate(acc.data_ptr(), cur.data_ptr(), prev.data_ptr(), None, w,
                                 cur.shape[0], ch, sigma, p, oy, ngy_)

        def normalize(out, acc, cur, y0, y1):
            ctx.frame_normalize(out.data_ptr(), acc.data_ptr(), cur.data_ptr(), w, cur.shape[0],
                                ch, y0, y1)
        # exact mode: all-gather of the mark words (RCCL) + whole-grid mask replay on every rank
        def match(marks, cur, prev, oy, ngy_):
            return ctx.strip_match(marks.data_ptr(), cur.data_ptr(), prev.data_ptr(), None, w,
                                   cur.shape[0], ch, sigma, p, oy, ngy_)

        def match_rows(marks, cur, prev, oy, ngy_, r0, rows, lay):
            return ctx.strip_match_part(marks.data_ptr(), cur.data_ptr(), prev.data_ptr(), None, w,
                                        cur.shape[0], ch, sigma, p, oy, ngy_, r0, rows, lay)

        def commit(marks_full, ngx_, ngy_, reach, active_full):
            ctx.mask_commit(marks_full.data_ptr(), ngx_, ngy_, reach, active_full.data_ptr())

        def group(acc, active):
            ctx.strip_group(acc.data_ptr(), active.data_ptr())
        sf = strips.StripFrame(rank, world, w, h, ch, psz, max(p.search_sz_x, p.search_sz_t), dev,
                               accumulate, normalize, phases=(match, commit, group, match_rows), stage_host=one_gpu)
        sf.load(t_n1, t_prev)
        one_step = sf.step

    def barrier():
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    # Row-strip runs check themselves before anything is timed: every rank computes the WHOLE frame on its own GPU
    # (one call, ~1 ms) and compares the rows one strip step gave it. Same decisions = same pixels up to the order
    # of the float sums (2e-3 on the 0..255 scale); the pixels excused are exactly those that sit at the reference's
    # `aggr > 1e-6` threshold and fell on the other side - one of the two outputs equals the input bit for bit
    # in every channel (tests/cases.py: excuse_flips). A mismatch on any rank ends the run with a non-zero status.
    selfcheck = None
    if (world > 1 or args.force_strips) and args.workload != "C5":
        t_full = torch.empty_like(t_n1)
        ctx_whole.filter_frame(t_full.data_ptr(), t_n1.data_ptr(), t_prev.data_ptr(), None, w, h, ch, sigma, p)
        one_step()
        barrier()
        if cs is not None:
            y0, y1, rows_ptr, _ = cs.own_rows(0)
            t_rows = torch.empty((y1 - y0, w, ch), dtype=torch.float32, device=dev)
            ctx.d2d(t_rows.data_ptr(), rows_ptr, (y1 - y0) * w * ch * 4)
            ctx.sync()
        else:
            y0, y1, t_rows = sf.own_rows()
        torch.cuda.synchronize()
        a, b, inp = t_rows, t_full[y0:y1], t_n1[y0:y1]
        flipped = ((a == inp).all(dim=2) ^ (b == inp).all(dim=2))
        diff = (a - b).abs().amax(dim=2)
        diff = torch.where(flipped, torch.zeros_like(diff), diff)
        diff = torch.nan_to_num(diff, nan=float("inf"))
        st = torch.tensor([float(diff.max().item()) if diff.numel() else 0.0, float(flipped.sum().item())],
                          dtype=torch.float64, device=dev)
        if world > 1:
            if one_gpu:
                st = st.cpu()                      # (gloo)
            mx = st[:1].clone()
            dist.all_reduce(mx, op=dist.ReduceOp.MAX)
            sm = st[1:].clone()
            dist.all_reduce(sm, op=dist.ReduceOp.SUM)
            st = torch.cat([mx, sm])
        selfcheck = {"max_abs": round(float(st[0].item()), 6), "threshold_pixels_excused": int(st[1].item()),
                     "tolerance": 2e-3, "what": "own rows of one strip step against the whole-frame call on the same GPU, every rank"}
        if watchdog is not None:
            watchdog.cancel()   # (set-up and a whole step went through)
            watchdog = None
        if not st[0].item() <= 2e-3:
            if rank == 0:
                print(f"bench.py: strip self-check FAILED: max |strip step - whole-frame call| = {st[0].item():g} "
                      f"(> 2e-3) on some rank's own rows: no line", file=sys.stderr)
            if world > 1:
                dist.destroy_process_group()
            raise SystemExit(3)

    if watchdog is not None:
        watchdog.cancel()
    # The GPU's clocks take ~25 ms of sustained load to settle (tools/step_trace.py, profiles/r05_step_trace.txt: the
    # 1080p step falls from 1.19 to 1.02 ms over its first 25 repetitions after an idle phase - the CPU legs above are
    # one): a timed loop of a few dozen 1 ms steps right after W warm-up steps would time that ramp, not the filter. So
    # the same step runs untimed for ~80 ms first (a fixed number of steps by frame size: every rank runs the same);
    # then the W warm-up steps and the K timed ones, as always (settle_steps).
    settle = settle_steps(w, h, ch)
    ramp_ms = None   # (what a loop of 20 steps started right here reads: reported beside ms_per_step, never instead)
    torch.cuda.synchronize()
    t_ramp = time.perf_counter()
    for i_ in range(settle):
        one_step()
        if i_ == 19:
            torch.cuda.synchronize()
            ramp_ms = (time.perf_counter() - t_ramp) / 20 * 1e3
    for _ in range(args.warmup):
        one_step()
    barrier()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        one_step()
    barrier()
    dt = time.perf_counter() - t0
    striped = world > 1 or args.force_strips
    dumped = None
    if args.dump_outputs and rank == 0 and (args.workload == "C5" or not striped):
        # (taken now: the loops of --full below run the step again; row strips: the frame assembled further down)
        dumped = {"smoothed": t_out, "flt2": t_f2} if args.workload == "C5" else {"denoised": t_out}
        dumped = {k_: v_.cpu().numpy() for k_, v_ in dumped.items()}
    if cs is not None:
        _, issue_us, replayed = cs.stats()          # (of the timed loop)
    tm, c5, ntr_local, nother_local = None, None, 0.0, 0.0
    if args.full:
        # Per-kernel times: a second, untimed loop of the same steps with HIP events around every kernel
        # on the context's stream (the timed loop above runs the same single-stream order, unprofiled).
        if cs is not None:
            cs.set_options(overlap=False, timing=False, graph=False)   # (a replayed graph carries no profiling events)
        ctx.set_profiling(True)
        for _ in range(args.steps):
            one_step()
        barrier()
        tm = ctx.timings()
        if args.workload == "C5":
            # the chain's three calls one at a time (HIP events around every kernel, as above): which launch dominates and
            # what it did - the smoother's records feed its roofline below (missing 3 / next 2)
            c5 = {}
            for name_, call_ in (("flt1", lambda: ctx.filter_frame(t_f1.data_ptr(), t_n1.data_ptr(), t_prev.data_ptr(), None, w, h, ch, sigma, p)),
                                 ("flt2", lambda: ctx.filter_frame(t_f2.data_ptr(), t_n1.data_ptr(), t_prev.data_ptr(), t_f1.data_ptr(), w, h, ch, sigma, p2)),
                                 ("smo1", lambda: ctx.smooth_frame(t_out.data_ptr(), t_prev.data_ptr(), t_f2.data_ptr(), None, w, h, ch, sigma, ps))):
                call_()
                barrier()
                ctx.set_profiling(False)
                ctx.set_profiling(True)     # (restarts the sums)
                for _ in range(args.steps):
                    call_()
                barrier()
                c5[name_] = {"ms": ctx.timings(), "rec": ctx.read_records()}
        ctx.set_profiling(False)
        # transforms this rank's group kernel really ran (from its records): the roofline's flops
        import numpy as np
        rec = ctx.read_records()
        if striped and args.workload != "C5" and cs is not None:
            geo = cs.geometry(0)
            _, _, _, act_ptr = cs.own_rows(0)
            act = ctx.download(act_ptr, (ngx * ngy,), np.uint8)[geo["gy0"] * ngx:geo["gy1"] * ngx].astype(bool)
        elif striped and args.workload != "C5":
            p_ = sf.p
            act = sf.active_full[p_["gy0"] * sf.ngx:p_["gy1"] * sf.ngx].cpu().numpy().astype(bool)
        else:
            act = rec["active"].astype(bool)
        act = act & (rec["nagg"] > 0)
        # ALGORITHMIC work of the group kernel (SURVEY.md §8(d) terms, per processed target): forward transforms of the
        # kept candidates (image, and previous frame when the target has valid previous patches), inverse transforms of
        # the group members (their forward transforms ARE candidate transforms: the kernels redo them, the algorithm
        # does not), statistics 16 flop per coefficient and candidate, gains 68 per coefficient, aggregation 2 per
        # member pixel and plane. Summed from the last launch's records.
        nsel_a, np0_a, nagg_a = (rec[k_][act].astype(np.float64) for k_ in ("nsel", "np0", "nagg"))
        ntr_local = float((nsel_a * (1 + (np0_a > 0)) + nagg_a).sum())                     # patch transforms per channel
        nother_local = float((nsel_a * ch * psz * psz * 16 + ch * psz * psz * 68 + nagg_a * psz * psz * (ch + 1) * 2).sum())
    phase_ms, strip_info = None, None
    if cs is not None:
        strip_info = {"driver": "C (csrc/strips.hip), one call per step", "transport": cs.transport(),
                      "enqueue_us_per_step": round(issue_us, 1), "hip_graph": replayed}
        if args.phase_times:
            cs.set_options(overlap=False, timing=True, graph=False)
            for _ in range(args.steps):
                one_step()
            barrier()
            phase_ms = cs.stats()[0]
            cs.set_options(overlap=False, timing=False, graph=False)
    elif striped and args.workload != "C5":
        strip_info = {"driver": "Python (strips.py over torch.distributed)"}
        if c_driver_note:
            strip_info["note"] = c_driver_note
    if cs is None and striped and args.phase_times and args.workload != "C5":
        sf.timers, sf.phase_s = True, {}
        for _ in range(args.steps):
            one_step()
        barrier()
        sf.timers = False
        phase_ms = {k_: round(v / args.steps * 1e3, 4) for k_, v in sf.phase_s.items()}
    if world > 1:
        tt = torch.tensor([dt] + ([tm["group_ms"], tm["match_ms"]] if tm is not None else []), dtype=torch.float64, device=dev)
        dist.all_reduce(tt, op=dist.ReduceOp.MAX)
        dt = float(tt[0].item())
        if tm is not None:
            tm["group_ms"], tm["match_ms"] = float(tt[1].item()), float(tt[2].item())   # slowest rank
        ts = torch.tensor([ntr_local, nother_local], dtype=torch.float64, device=dev)
        dist.all_reduce(ts)
        ntr_total, nother_total = float(ts[0].item()), float(ts[1].item())
        if phase_ms is not None:
            allp = [None] * world
            dist.all_gather_object(allp, phase_ms)
            phase_ms = allp
        full = torch.zeros_like(t_n1)
        if cs is not None:
            y0, y1, rows_ptr, _ = cs.own_rows(0)
            ctx.d2d(full[y0:y1].data_ptr(), rows_ptr, (y1 - y0) * w * ch * 4)
            ctx.sync()
        else:
            y0, y1, rows = sf.own_rows()
            full[y0:y1] = rows
        dist.all_reduce(full)
        t_out = full
    else:
        ntr_total, nother_total = ntr_local, nother_local
        if cs is not None:   # (--force-strips at N = 1: the one strip is the frame)
            y0, y1, rows_ptr, _ = cs.own_rows(0)
            ctx.d2d(t_out.data_ptr(), rows_ptr, (y1 - y0) * w * ch * 4)
            ctx.sync()
        elif striped and args.workload != "C5":
            y0, y1, rows = sf.own_rows()
            t_out[y0:y1] = rows

    if rank == 0:
        ms = dt / args.steps * 1e3
        value = w * h / (dt / args.steps) / 1e6
        if args.dump_outputs:
            dump_outputs(args.dump_outputs, dumped if dumped is not None else {"denoised": t_out.cpu().numpy()})
        res = {"metric": "Mpix/s per frame (nlkalman-flt, 1080p sigma=20)"
               if args.workload == "C2" else f"Mpix/s per frame (nlkalman-flt, {args.workload})",
               "value": round(value, 3), "unit": "Mpix/s", "n_gpus": world, "steps": args.steps,
               "warmup": args.warmup, "clock_settle_steps": settle,
               "ms_per_step_first_20_unsettled": round(ramp_ms, 4) if ramp_ms is not None else None,
               "ms_per_step": round(ms, 4), "higher_is_better": True,
               "scaling": "strong", "vs_baseline": None, "dtype": "f32", "data": "synthetic",
               "config": {"workload": f"{args.workload}: {w}x{h}x{ch} synthetic AWGN sigma={sigma:g}, "
                                      f"FLT1 temporal (deno0 = spatial FLT1 of frame 0, bsic1=NULL), "
                                      f"patch {psz}, defaults of nlkalman_default_params",
                          "parallelism": f"row strips x{world}" if world > 1 else "single GPU",
                          "mask_order": "serial-exact" if world == 1 else
                          "serial-exact (mark words all-gathered, mask replayed on every rank)",
                          # (the opt-in block-summed distance order, 8 x 8 patches: k_match.h; `value` of a default run
                          # is always the exact order)
                          "match_order": ("block-summed (NLK_MATCH_ORDER=block: NOT the reference's summation order)"
                                          if os.environ.get("NLK_MATCH_ORDER", "") in ("block", "1") and psz == 8
                                          else "exact (the reference's hy, hx, c order)")}}
    if rank == 0 and args.full:
        out = t_out.cpu().numpy()
        # dominant kernel and its roofline; algorithmic bytes and flops: DESIGN.md §5.
        # The group kernel runs its DCTs on the f32 matrix cores and everything else on the
        # f32 vector ALU, which share one FP32 datapath on gfx950 (tools/ubench/mfma_valu.hip):
        # it is priced against the dense f32 MFMA peak. Algorithmic flops per launch: see above
        # (2 * psz^3 MACs per psz x psz patch transform in the row-column matrix form).
        k, ngrid = p.npatches_t, ngx * ngy
        alg_bytes = {"match": w * h * ch * 4 + ngrid * k * 4,
                     "group": 2 * w * h * ch * 4 + (ch + 1) * w * h * 4 + ngrid * k * 4}
        # (all ranks' transforms; per-GPU figures below divide by the world size and use the slowest
        # rank's kernel time)
        # (the fraction of the f32 MFMA peak counts the TRANSFORMS only - what runs on the matrix cores, and what
        # rounds 1 and 2 counted; the statistics / gains / aggregation estimate is vector-ALU work and has its own
        # line, against the same peak: a wave64 v_fma_f32 issues in 2 cycles on a SIMD-32 = 64 FLOP / clk / SIMD =
        # 157.3 TFLOP/s, MI355X_MICROARCH.md (round 4 priced it against half of that: VERDICT r4, weak 7))
        group_flops = ntr_total * ch * 2 * 2 * psz ** 3
        alg_flops = {"match": ngrid * (121 * 192 * 3), "group": group_flops}
        dom = "group" if tm["group_ms"] >= tm["match_ms"] else "match"
        dur = tm[dom + "_ms"] * 1e-3
        gbs = alg_bytes[dom] / world / dur / 1e9 if dur > 0 else 0.0
        tfl = alg_flops[dom] / world / dur / 1e12 if dur > 0 else 0.0
        kname = ("k_group8m" if psz == 8 and ch in (1, 3) else "k_groupp") if dom == "group" else "k_bm_topk"
        # the instantiation the timed (temporal) frames launch: what the PMC table is looked up by
        # (k_group8m's third template argument: which pass runs the separable DCT form - tu_group8.hip; the filter's
        # temporal frames: 6, separable in both passes)
        # (the fourth: 1 = the copy compiled under the max-ilp scheduler, tu_group8_ilp.hip - the RGB filter's two forms)
        g8sep = os.environ.get("NLK_GROUP_SEP", "6")
        g8unit = 1 if ch == 3 and g8sep in ("2", "6") and os.environ.get("NLK_GROUP_ILP", "1") != "0" else 0
        inst = ((f"k_group8m<{ch}, false, {g8sep}, {g8unit}>" if kname == "k_group8m" else f"k_groupp<{psz}, false>") if dom == "group"
                else f"k_bm_topk<{psz}, {ch}, {((2 * p.search_sz_t + 1) ** 2 + 63) // 64}>")
        # HBM-side bytes per launch: PMC passes of the same sources (see measured_traffic)
        traffic, traffic_note = (None, "single-GPU runs only") if world > 1 else measured_traffic(args.workload, inst)
        roof = {"kernel": inst, "bound": "mfma",
                "achieved": round(tfl, 3), "peak": MFMA_F32_PEAK_TFLOPS, "unit": "TFLOP/s",
                "frac": round(tfl / MFMA_F32_PEAK_TFLOPS, 4), "traffic": traffic, "traffic_note": traffic_note,
                "launch_ms": round(tm[dom + "_ms"], 4),
                # (round 3's figure for comparison: every term of SURVEY.md §8(d) - transforms, statistics, gains,
                # aggregation - over the f32 peak; `frac` above is the transforms alone)
                "frac_all_survey_terms": (round((group_flops + nother_total) / world / dur / 1e12 / MFMA_F32_PEAK_TFLOPS, 4)
                                          if dom == "group" and dur > 0 else None),
                "algorithmic_flops_per_launch": int(alg_flops[dom] / world),
                "algorithmic_bytes_per_launch": alg_bytes[dom] // world,
                "hbm": {"achieved": round(gbs, 3), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                        "frac": round(gbs / HBM_PEAK_GBS, 6)},
                "valu": ({"achieved": round(nother_total / world / dur / 1e12, 3), "peak": MFMA_F32_PEAK_TFLOPS,
                          "unit": "TFLOP/s", "frac": round(nother_total / world / dur / 1e12 / MFMA_F32_PEAK_TFLOPS, 4),
                          "what": "statistics 16 flop per coefficient and candidate, gains 68 per coefficient, "
                                  "aggregation 2 per member pixel and plane (estimate), over the same launch time"}
                         if dom == "group" and dur > 0 else None),
                "note": (f"{psz}x{psz} patches: the transforms run as flow graphs on the f32 vector ALU (same FP32 datapath, "
                         "same peak; algorithmic flops = the row-column matrix form). " if kname == "k_groupp" else "") +
                        ("per GPU: all ranks' transforms / world size over the slowest rank's kernel time. " if world > 1 else "") +
                        "~550 flop per algorithmic byte: compute bound. frac = transform flops only (matrix cores); "
                        "the vector-ALU share of the same launch is roofline.valu; f32 MFMA and f32 VALU share "
                        "the FP32 datapath on gfx950: see DESIGN.md §5"}
        res["kernels_ms"] = {k_: round(v, 4) for k_, v in tm.items()}
        res["kernels_ms_note"] = ("second loop of the same steps with HIP events around every kernel on the "
                                  "context's stream; ms_per_step is the timed (unprofiled) loop. Whole-frame calls "
                                  "of 8x8 patches replay the processed mask inside the group kernel's launch: "
                                  "commit_ms is the bit-plane kernel alone, group_ms includes the replay "
                                  "(NLK_NO_CHASE=1: separate kernels)")
        res["roofline"] = roof
        if world == 1 and not striped and not args.no_extras and args.workload in ("C1", "C1L", "C2", "C3"):
            # beside the resident temporal call: the first frame of a sequence (deno0 = NULL: the spatial branch
            # everywhere, 441-candidate windows) and the drop-in API on host pointers (PCIe
            # included; pageable host memory, frame in row bands). Neither is `value`.
            reps = 5
            for timed in (0, 1):  # (2 untimed calls, then 20 timed ones)
                torch.cuda.synchronize()
                t1 = time.perf_counter()
                for _ in range(20 if timed else 2):
                    ctx.filter_frame(t_out.data_ptr(), t_n0.data_ptr(), None, None, w, h, ch, sigma, p)
                torch.cuda.synchronize()
            res["first_frame_ms"] = round((time.perf_counter() - t1) / 20 * 1e3, 4)
            ctx.filter_frame(t_out.data_ptr(), t_n1.data_ptr(), t_prev.data_ptr(), None, w, h, ch, sigma, p)
            torch.cuda.synchronize()
            h_n1, h_prev = t_n1.cpu().numpy(), t_prev.cpu().numpy()
            pkg.filter_frame(h_n1, h_prev, None, sigma, p)           # (its own context, buffers and streams: once)
            walls = []
            for _ in range(reps):
                t1 = time.perf_counter()
                pkg.filter_frame(h_n1, h_prev, None, sigma, p)
                walls.append(time.perf_counter() - t1)
            res["api_wall_ms"] = round(min(walls) * 1e3, 4)
            res["api_wall_note"] = ("nlkalman_filter_frame on pageable host images (75 MB up, 25 MB down at 1080p RGB), "
                                    f"best of {reps}; PCIe-inclusive, never `value`")
        if args.workload == "C5":
            res["kernels_ms"] = {k_: round(3 * v, 4) for k_, v in tm.items()}  # per step = 3 calls
            res["stages_ms"] = {n_: {k_: round(v, 4) for k_, v in c5[n_]["ms"].items()} for n_ in c5}
            res["roofline"] = c5_roofline(c5, w, h, ch, psz, ngx * ngy, ps)
            if not args.no_cpu:
                sys.path.insert(0, os.path.join(ROOT, "oracle"))
                import oracle as O
                res["cpu_baseline"] = cpu_baseline_chain(O, t_n1.cpu().numpy(), t_prev.cpu().numpy(), sigma, p, p2, ps)
                res["speedup_vs_cpu"] = round(value / res["cpu_baseline"]["value"], 1)
        if not args.no_cpu and args.workload != "C5":
            sys.path.insert(0, os.path.join(ROOT, "oracle"))
            import oracle as O
            o1_h, prev_h = t_n1.cpu().numpy(), t_prev.cpu().numpy()
            if world == 1:   # the CPU baseline is timed at N = 1 only; N > 1 keeps the parity leg below
                ref, cb = cpu_baseline(O, o1_h, prev_h, sigma, p)
                res["cpu_baseline"] = cb
            else:
                cb = None
                if args.workload == "C3":   # (every other workload takes the serial order below)
                    po = O.Params(*[getattr(p, k) for k, _ in p._fields_])
                    ref = O.filter_frame(o1_h, prev_h, None, sigma, po, nthreads=min(os.cpu_count() or 1, 100))
            # quality reference = the serial (OpenMP off) order, which is the order the GPU path
            # reproduces; the threaded run above perturbs the processed-mask like the reference's
            # own OpenMP build does. C3 never skips (step > temporal radius): any order is the same.
            order = "parallel (order-independent for this config)"
            if args.workload != "C3":
                po = O.Params(*[getattr(p, k) for k, _ in p._fields_])
                ref = O.filter_frame(o1_h, prev_h, None, sigma, po, nthreads=1)
                order = "serial"
            res["psnr_gpu_db"] = round(synth.psnr(O.opp2rgb(out), c1), 4)
            res["psnr_cpu_db"] = round(synth.psnr(O.opp2rgb(ref), c1), 4)
            res["psnr_delta_db"] = round(res["psnr_gpu_db"] - res["psnr_cpu_db"], 4)
            res["psnr_reference_order"] = order
            import numpy as np
            res["max_abs_vs_cpu"] = round(float(np.abs(out - ref).max()), 6)
            if cb is not None:
                res["speedup_vs_cpu"] = round(value / cb["value"], 1)
    if rank == 0:
        if args.strip_model and world == 1 and args.workload in ("C2", "C3"):
            model = []
            for nw in (2, 4, 8):
                row = {"world": nw, "rank": nw // 2}
                for graph in (False, True):
                    m = pkg.Strips([local], nw // 2, nw, w, h, ch, sigma, p)
                    m.set_dry_run(True)
                    m.set_options(overlap=False, timing=False, graph=graph)
                    m.load(0, t_n1.data_ptr(), t_prev.data_ptr())
                    for _ in range(5):
                        m.step()
                    m.sync()
                    m.stats()
                    t1 = time.perf_counter()
                    for _ in range(args.steps):
                        m.step()
                    m.sync()
                    dtm = (time.perf_counter() - t1) / args.steps * 1e3
                    _, us, rep = m.stats()
                    row["graph_ms" if graph else "ms"] = round(dtm, 4)
                    row["graph_enqueue_us" if graph else "enqueue_us"] = round(us, 1)
                    if graph:
                        row["graph_replayed"] = rep
                    g_ = m.geometry(0)
                    row["grid_rows"] = g_["gy1"] - g_["gy0"]
                    m.close()
                row["mpix_s_if_every_rank_took_this"] = round(w * h / (min(row["ms"], row["graph_ms"]) * 1e-3) / 1e6, 1)
                model.append(row)
            res["strip_model"] = {"note": "ONE middle rank of a world of N stepped alone on this GPU, exchanges skipped: its "
                                          "kernels and launch gaps per frame; the last column is the frame rate if every rank "
                                          "took that long and the exchanges were free - an upper bound, not a measurement",
                                  "ranks": model}
        if strip_info is not None:
            res["strip_step"] = strip_info
        if preflight is not None:
            # (rank 0's own trial + what the ranks agreed on: run_preflight)
            res["preflight"] = dict(preflight, what="the C strip driver's set-up, one step and the self-check tried in a child "
                                                    "process per rank before the ranks touched their GPUs")
        if selfcheck is not None:
            res["strip_selfcheck_max_abs"] = selfcheck["max_abs"]
            res["strip_selfcheck"] = selfcheck
        if phase_ms is not None:
            res["strip_phase_ms"] = phase_ms
        if one_gpu and world > 1:
            res["not_a_measurement"] = (f"NLK_BENCH_ONE_GPU=1: all {world} ranks share device 0 and exchange through host "
                                        "memory over gloo - a record of the N > 1 code path running end to end, "
                                        "its times mean nothing")
        if args.workload == "C5":
            res["config"]["workload"] = (f"C5: {w}x{h}x{ch} sigma={sigma:g}: flt1 temporal -> flt2 -> smo1 "
                                         f"(3 frame calls per step), frames resident")
            res["metric"] = "Mpix/s per frame (flt1 -> flt2 -> smo1 chain, 1080p sigma=20, frames resident)"
        emit(res)
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
