"""In-process sequence driver: the recursion of
scripts/nlkalman-seq.sh — per frame `tvl1flow` -> occlusion mask -> `nlkalman-flt`
(iteration 1) -> `nlkalman-flt` (iteration 2), then backwards `tvl1flow` -> mask ->
`nlkalman-smo` — with every frame, flow and mask resident in HBM and one device context,
instead of four processes and ~10 float-TIFF round trips per frame.

Forward (reference: scripts/nlkalman-seq.sh:30-115):
    frame 0:  flt1_0 = FLT1(noisy_0),  flt2_0 = FLT2(noisy_0, basic = flt1_0)
    frame t:  flow_t = TVL1(noisy_t -> flt2_{t-1});  occ_t = |div flow_t| > TH
              flt1_t = FLT1(noisy_t, warp(flt1_{t-1}, flow_t, occ_t))
              flt2_t = FLT2(noisy_t, warp(flt2_{t-1}, flow_t, occ_t), basic = flt1_t)
Backward (reference: :117-150):
    smo_T = flt2_T;  smo_t = SMO1(flt2_t, warp(smo_{t+1}, TVL1(flt2_t -> smo_{t+1}), occ))

Lag-1 smoother (reference: scripts/nlkalman-lsmo-seq.sh:87-116), SequenceFilter(lag1="tvl1" | "inv"):
    after frame t:  lsm1_{t-1} = SMO1(flt2_{t-1}, warp(flt2_t, F_t, occ(F_t)))
    F_t = TVL1(flt2_{t-1} -> flt2_t)  ("tvl1", the script's)  or  the inverse of flow_t  ("inv", Context.flow_invert)
    lsm1 of the last frame is its flt2

Frames are kept in the opponent colour space the filters work in (src/main-flt.c:335-343
converts on read and back on write); the flow sees the luminance of the RGB frames like
the tool does. Compared with the chain of processes this skips one opp->rgb->opp rounding
of the previous outputs per frame (~1e-5 on the 0..255 scale); nothing else differs.

Host side only: every array operation is a call of the C-ABI (include/nlk_hip.h).
"""
import importlib

import numpy as np

_pkg = None


def _p():
    global _pkg
    if _pkg is None:
        _pkg = importlib.import_module(__name__.rsplit(".", 1)[0])
    return _pkg


class SequenceFilter:
    """`ctx` = bwd-nlkalman_amd.Context. Flow parameters `of_*` are what the scripts pass to
    tvl1flow (lambda = "DW", finest scale, occlusion threshold: nlkalman-seq.sh:47-52); the defaults
    are the script's own OPM default "1 0.25 0.75 1 0.25 0.75" (nlkalman-seq.sh:12), as in host/main_seq.c
    (nlkalman-seq-gt.sh uses DW = 0.40). sigma="auto": the noise level is measured on the first pushed frame
    (Context.estimate_sigma on the RGB frame as pushed, what `nlkalman-seq ... auto` does); .sigma is None until then,
    and the parameter sets not given are the defaults of the measured value.
    sigma="vst" or ("vst", a, b): signal-dependent noise var = a y + b, as `nlkalman-seq ... vst` / `vst:A,B`: the
    pairs are measured on the first pushed frame (Context.estimate_noise_curve) or given for every channel; .noise
    holds them ([ch][2] float32), .sigma the scale S of the variance-stabilising transform (vst_scale). Every pushed
    frame is transformed first (Context.vst_forward), the recursion runs on transformed frames at sigma = S, and
    download_rgb transforms back (Context.vst_inverse, mode 1).
    sigma="nlf": a noise-level function of any shape (gamma-encoded video), as `nlkalman-seq ... nlf`: .nlf is the
    NlfTable of the first pushed frame (Context.nlf_table), .sigma its scale; Context.nlf_forward / nlf_inverse stand
    where vst's transform stands.
    lag1="tvl1" | "inv": after push() of frame t >= 1, .lsm1 is the smoothed frame t - 1 (device pointer, opponent
    space, valid until the next push; None after the first push), .d_fflow / .d_focc the forward flow
    flt2_{t-1} -> flt2_t and its mask: "tvl1" computes that flow (its iteration counts go to .lag1_flow_iterations),
    "inv" inverts the backward flow of frame t (LAG1_INVERT_STEPS fixed-point steps). lag1_of_* / lag1_occ_th are the
    second triple of OPM (default: the first). finish() gives the last frame's lsm1, its flt2.
    of="tvl1" | "bm": the flow estimator of the run, as the tools' --of. "bm": Context.bm_flow (block matching,
    DESIGN.md §9) wherever a flow is computed - push(), smooth(), lag1="tvl1"'s own flow - at of_fscale / lag1_of_fscale;
    of_lambda is ignored and flow_iterations / lag1_flow_iterations stay empty.
    sure=True | eps_rel: the error of every pushed frame's flt1 and flt2 is estimated without clean frames by
    Monte-Carlo SURE (seq_sure_step of host/seq_step.c), at the cost of one more FLT1 and FLT2 on the
    frame plus a probe of +-eps, eps = eps_rel * sigma (True: SURE_EPS_REL, or NLK_SURE_EPS). After push(), which then
    waits for the device, .sure[-1] is a dict: mse, psnr (at 255), resid = R / N, div = D / (eps N) of flt2 over all
    samples, mse_ch ... div_ch the same per channel (arrays), "flt1" the same dict for flt1, eps and seed as used; and
    .sure_blocks the risk map of flt2, [nby][nbx][ch][2] = (R, D) per sure_block x sure_block tile. sure_seed (default
    0, or NLK_SURE_SEED): frame t uses sure_seed + t * SURE_FRAME_STEP. The estimate is in the domain the filter works
    in: under sigma="vst" | "nlf" the stabilised one, at .sigma. The smoother's outputs are not estimated.
    despike=K | (K, R): as the tools' --despike K[,R]: every pushed frame goes through Context.despike at
    thr = K * sigma and ring radius R (1, the default, or 2) after the vst / nlf transform and before anything else
    sees it (stuck, hot and dead pixels; DESIGN.md §9, whose table was made with K = 4). The pushed frame itself is
    not modified; sure= then treats the despiked frame as the data. None: nothing is allocated or launched for it.
    defect_map=K | (K, R) | (K, R, N): as the tools' --defect-map K[,R[,N]]: a defect map learned over time
    (Context.defect_step at Context.defect_schedule's threshold and gain). Frame t is cleaned with the
    evidence of the frames 0 .. t - 1: where their running mean (window N = 2 .. 4096, default 32; no motion
    compensation) lies more than K sigma / sqrt(min(t, N)) outside its ring's range (radius R = 1, the default, or 2),
    the frame's sample becomes the median of its own ring. After the vst / nlf transform, in front of despike= when both
    are given. .defect_map: the device uint8 map [h][w][ch] of the last step (1 = flagged). defect_counts=True: the
    steps also count, and .defect_counts is the samples of every channel the last step replaced ([ch] uint32), downloaded
    when asked for (it waits for the device; the count's atomics cost what Context.despike_counts' cost, so they are on
    request only). None: nothing is allocated or launched for it."""

    LAG1_INVERT_STEPS = 4   # SEQ_LAG1_INVERT_STEPS of host/seq_step.h
    SURE_EPS_REL, SURE_BLOCK, SURE_FRAME_STEP = 0.05, 16, 0xD1B54A32D192ED03   # SEQ_SURE_* of host/seq_step.h

    def __init__(self, ctx, w, h, ch, sigma, f1=None, f2=None, s1=None, of_lambda=0.25, of_fscale=1,
                 occ_th=0.75, keep_history=True, lag1=None, lag1_of_lambda=None, lag1_of_fscale=None,
                 lag1_occ_th=None, of="tvl1", sure=None, sure_seed=None, sure_block=None, despike=None,
                 defect_map=None, defect_counts=False):
        pkg = _p()
        self.despike, self.d_despiked = None, None
        if despike is not None:
            k, r = despike if isinstance(despike, (tuple, list)) else (despike, 1)
            if not (np.isfinite(float(k)) and float(k) > 0 and r in (1, 2)):
                raise ValueError(f"SequenceFilter(despike={despike!r}): want None, K or (K, R) with K > 0 and R = 1 or 2")
            self.despike = (float(k), int(r))
        self.defects, self.defect_map, self.d_defect = None, None, None
        if defect_map is not None:
            kr = tuple(defect_map) if isinstance(defect_map, (tuple, list)) else (defect_map,)
            kr = kr + (1, 32)[len(kr) - 1:] if 1 <= len(kr) <= 3 else (0, 0, 0)
            try:
                ok = (np.isfinite(float(kr[0])) and float(kr[0]) > 0 and kr[1] in (1, 2)
                      and kr[2] == int(kr[2]) and 2 <= kr[2] <= 4096)
            except (TypeError, ValueError):   # (a value that is no number at all)
                ok = False
            if not ok:
                raise ValueError(f"SequenceFilter(defect_map={defect_map!r}): want None, K, (K, R) or (K, R, N) with "
                                 "K > 0, R = 1 or 2 and N = 2 .. 4096")
            self.defects = (float(kr[0]), int(kr[1]), int(kr[2]))
        self.want_defect_counts = bool(defect_counts) and self.defects is not None
        if of not in ("tvl1", "bm"):
            raise ValueError(f"SequenceFilter(of={of!r}): want 'tvl1' or 'bm'")
        self.flow_estimator = of
        if lag1 not in (None, "tvl1", "inv"):
            raise ValueError(f"SequenceFilter(lag1={lag1!r}): want None, 'tvl1' or 'inv'")
        self.ctx, self.w, self.h, self.ch = ctx, w, h, ch
        self.f1, self.f2, self.s1 = f1, f2, s1
        self.sigma = None
        self.vst, self.noise, self.d_vst = False, None, None
        self.nlf = None
        self._nlf = isinstance(sigma, str) and sigma == "nlf"
        if isinstance(sigma, str) and sigma == "vst":
            self.vst = True
        elif isinstance(sigma, (tuple, list)) and len(sigma) == 3 and sigma[0] == "vst":
            self.vst = True
            self._resolve_vst(np.tile(np.asarray(sigma[1:], np.float32), (ch, 1)))
        elif not (isinstance(sigma, str) and sigma in ("auto", "nlf")):
            self._resolve(float(sigma))
        self.of = pkg.tvl1_params(w, h, lam=of_lambda, fscale=of_fscale)
        self.occ_th = float(occ_th)
        self.nbytes = w * h * ch * 4
        a = ctx.alloc
        self.d_noisy, self.d_rgb, self.d_warp = a(self.nbytes), a(self.nbytes), a(self.nbytes)
        self.d_g0, self.d_g1, self.d_occ = a(w * h * 4), a(w * h * 4), a(w * h * 4)
        self.d_flow = a(w * h * 8)
        self.flt1, self.flt2 = None, None   # previous outputs (opponent space, device)
        self.history = [] if keep_history else None  # flt2 of every frame, for smooth()
        self._pool = []                      # released frame buffers (no hipMalloc / hipFree per frame)
        self.t = 0
        self.flow_iterations = []
        self.lag1, self.lsm1 = lag1, None
        if lag1:
            self.of2 = pkg.tvl1_params(w, h, lam=of_lambda if lag1_of_lambda is None else lag1_of_lambda,
                                       fscale=of_fscale if lag1_of_fscale is None else lag1_of_fscale)
            self.occ_th2 = float(occ_th if lag1_occ_th is None else lag1_occ_th)
            self.d_fflow, self.d_focc = a(w * h * 8), a(w * h * 4)
            self.lag1_flow_iterations = []
        self.sure_eps_rel = None
        if sure is not None and sure is not False:
            import os
            env_eps, env_seed = os.environ.get("NLK_SURE_EPS"), os.environ.get("NLK_SURE_SEED")
            if sure is True:
                sure = float(env_eps) if env_eps and float(env_eps) > 0 else self.SURE_EPS_REL
            if not float(sure) > 0:
                raise ValueError(f"SequenceFilter(sure={sure!r}): want True or eps / sigma > 0")
            self.sure_eps_rel = float(sure)
            self.sure_seed = int(sure_seed) if sure_seed is not None else int(env_seed, 0) if env_seed else 0
            self.sure_block = int(sure_block or self.SURE_BLOCK)
            self.sure, self.sure_blocks = [], None
            self._sure_img = [a(self.nbytes) for _ in range(3)]   # the perturbed frame and its two estimates
            nby, nbx = -(-h // self.sure_block), -(-w // self.sure_block)
            self._sure_map_shape = (nby, nbx, ch, 2)
            self._d_sure = a(8 * (4 * ch + 2 * ch * nby * nbx))   # the terms of flt1 and flt2, then flt2's map
        self.stage_s = None   # set to {} to have push() synchronise after each stage and add up its wall times (bench.py S1)

    def _resolve(self, sigma):
        """sigma is known: the parameter sets the caller left out are its defaults"""
        pkg = _p()
        self.sigma = sigma
        self.f1 = self.f1 or pkg.default_params(sigma, pkg.FLT1)
        self.f2 = self.f2 or pkg.default_params(sigma, pkg.FLT2)
        self.s1 = self.s1 or pkg.default_params(sigma, pkg.SMO1)

    def _resolve_vst(self, ab):
        """the noise coefficients are known: the scale of the transform is the sigma of the run"""
        self.noise = np.ascontiguousarray(ab, np.float32)
        self._resolve(_p().vst_scale(self.noise))

    def _flow_and_mask(self, d_from_rgb, d_to_opp):
        """flow from frame `d_from_rgb` (RGB) to the frame whose opponent image is `d_to_opp`."""
        c, w, h, ch = self.ctx, self.w, self.h, self.ch
        c.gray(self.d_g0, d_from_rgb, w, h, ch)
        c.d2d(self.d_rgb, d_to_opp, self.nbytes)
        c.opp2rgb(self.d_rgb, w, h, ch)
        c.gray(self.d_g1, self.d_rgb, w, h, ch)
        self._flow(self.d_flow, self.of, self.flow_iterations)
        c.occlusion_mask(self.d_occ, self.d_flow, w, h, self.occ_th)

    def _flow(self, d_flow, of, iterations):
        """the flow d_g0 -> d_g1 of the run's estimator (seq_flow of host/seq_step.c)"""
        c, w, h = self.ctx, self.w, self.h
        if self.flow_estimator == "bm":
            c.bm_flow(d_flow, self.d_g0, self.d_g1, w, h, fscale=max(of.fscale, 0))
        else:
            iterations.append(c.tvl1_flow(d_flow, self.d_g0, self.d_g1, w, h, of))

    @property
    def defect_counts(self):
        """the samples of every channel that the last step's defect map replaced ([ch] uint32); waits for the device"""
        if self.d_defect is None or self.d_defect[3] is None:
            raise ValueError("SequenceFilter.defect_counts: want defect_map= with defect_counts=True, and a pushed frame")
        return self.ctx.download(self.d_defect[3], (self.ch,), np.uint32)

    def push(self, d_noisy_rgb):
        """Next noisy frame (device pointer, HWC RGB or gray, not modified). Afterwards
        self.flt1 / self.flt2 hold its two estimates (opponent space)."""
        c, w, h, ch = self.ctx, self.w, self.h, self.ch
        if self.vst:
            if self.noise is None:
                self._resolve_vst(c.estimate_noise_curve(d_noisy_rgb, w, h, ch)[0])
            if self.d_vst is None:
                self.d_vst = c.alloc(self.nbytes)
            c.vst_forward(self.d_vst, d_noisy_rgb, w * h * ch, ch, self.noise, self.sigma)
            d_noisy_rgb = self.d_vst   # the flow sees the transformed frame too
        if self._nlf:
            if self.nlf is None:
                table = c.nlf_table(d_noisy_rgb, w, h, ch)
                if not table.s > 0:
                    raise ValueError(f"SequenceFilter(sigma='nlf'): the first frame keeps {list(table.kept)[:ch]} bins")
                self.nlf = table
                self._resolve(float(table.s))
            if self.d_vst is None:
                self.d_vst = c.alloc(self.nbytes)
            c.nlf_forward(self.d_vst, d_noisy_rgb, w * h * ch, ch, self.nlf)
            d_noisy_rgb = self.d_vst
        if self.sigma is None:
            est = c.estimate_sigma(d_noisy_rgb, w, h, ch)[0]
            if not est > 0:
                raise ValueError(f"SequenceFilter(sigma='auto'): the first frame gives sigma = {est}")
            self._resolve(est)
        sg = self.sigma
        if self.defects:
            k, r, n = self.defects
            if self.d_defect is None:   # the cleaned frame, the two means (swapped every step), the counts
                self.d_defect = [c.alloc(self.nbytes) for _ in range(3)] + [c.alloc(4 * ch) if self.want_defect_counts else None]
                self.defect_map = c.alloc(w * h * ch)
            d_out, d_count = self.d_defect[0], self.d_defect[3]
            thr, gain = c.defect_schedule(self.t, n, float(np.float32(k) * np.float32(sg))) if self.t else (0.0, 1.0)
            c.defect_step(d_out, d_noisy_rgb, self.d_defect[1 + (self.t + 1) % 2],
                          self.d_defect[1 + self.t % 2] if self.t else None, w, h, ch, thr, gain, r, self.defect_map, d_count)
            d_noisy_rgb = d_out   # what despike and the flow see
        if self.despike:
            if self.d_despiked is None:
                self.d_despiked = c.alloc(self.nbytes)
            thr = float(np.float32(self.despike[0]) * np.float32(sg))
            c.despike(self.d_despiked, d_noisy_rgb, w, h, ch, thr, self.despike[1])
            d_noisy_rgb = self.d_despiked   # the flow sees the despiked frame too
        c.d2d(self.d_noisy, d_noisy_rgb, self.nbytes)
        c.rgb2opp(self.d_noisy, w, h, ch)
        n1, n2 = self._frame(), self._frame()
        if self.t == 0:
            c.filter_frame(n1, self.d_noisy, None, None, w, h, ch, sg, self.f1)
            c.filter_frame(n2, self.d_noisy, None, n1, w, h, ch, sg, self.f2)
        else:
            mark = self._stage_mark
            mark(None)
            self._flow_and_mask(d_noisy_rgb, self.flt2)
            mark("flow_and_mask")
            c.warp_bicubic(self.d_warp, self.flt1, self.d_flow, self.d_occ, w, h, ch)
            c.filter_frame(n1, self.d_noisy, self.d_warp, None, w, h, ch, sg, self.f1)
            mark("warp_flt1")
            c.warp_bicubic(self.d_warp, self.flt2, self.d_flow, self.d_occ, w, h, ch)
            c.filter_frame(n2, self.d_noisy, self.d_warp, n1, w, h, ch, sg, self.f2)
            mark("warp_flt2")
        if self.sure_eps_rel is not None:
            self._sure_step(n1, n2)
        if self.lag1 and self.t > 0:
            self._lag1_step(n2)
        if self.flt1:
            self._pool.append(self.flt1)
        if self.flt2 and self.history is None:
            self._pool.append(self.flt2)
        self.flt1, self.flt2 = n1, n2
        if self.history is not None:
            self.history.append(n2)
        self.t += 1

    def _sure_step(self, n1, n2):
        """the estimates of this frame's flt1 (n1) and flt2 (n2) while d_noisy, d_flow and d_occ hold its values:
        seq_sure_step of host/seq_step.c; waits for the device"""
        c, w, h, ch, sg = self.ctx, self.w, self.h, self.ch, self.sigma
        d_probe, q1, q2 = self._sure_img
        eps = float(np.float32(self.sure_eps_rel) * np.float32(sg))
        seed = (self.sure_seed + self.t * self.SURE_FRAME_STEP) & 0xFFFFFFFFFFFFFFFF
        c.probe_add(d_probe, self.d_noisy, w * h * ch, eps, seed)
        prev = self.t > 0
        if prev:
            c.warp_bicubic(self.d_warp, self.flt1, self.d_flow, self.d_occ, w, h, ch)
        c.filter_frame(q1, d_probe, self.d_warp if prev else None, None, w, h, ch, sg, self.f1)
        if prev:
            c.warp_bicubic(self.d_warp, self.flt2, self.d_flow, self.d_occ, w, h, ch)
        c.filter_frame(q2, d_probe, self.d_warp if prev else None, q1, w, h, ch, sg, self.f2)
        d_tot, d_map = self._d_sure, self._d_sure + 8 * 4 * ch
        c.sure_terms_dev(d_tot, None, self.d_noisy, n1, q1, w, h, ch, self.sure_block, seed)
        c.sure_terms_dev(d_tot + 8 * 2 * ch, d_map, self.d_noisy, n2, q2, w, h, ch, self.sure_block, seed)
        tot = c.download(d_tot, (2, ch, 2), np.float64)
        self.sure_blocks = c.download(d_map, self._sure_map_shape, np.float64)
        pkg = _p()

        def est(t2):
            out = {}
            for key, R, D, n in (("", t2[:, 0].sum(), t2[:, 1].sum(), w * h * ch), ("_ch", t2[:, 0], t2[:, 1], w * h)):
                m = R / n - sg * sg + 2.0 * sg * sg * D / (eps * n)
                with np.errstate(invalid="ignore", divide="ignore"):
                    out.update({"mse" + key: m, "psnr" + key: 10.0 * np.log10(255.0 ** 2 / m), "resid" + key: R / n,
                                "div" + key: D / (eps * n)})
            out["mse"] = pkg.sure_mse(t2[:, 0].sum(), t2[:, 1].sum(), w * h * ch, sg, eps)
            return out
        rec = est(tot[1])
        rec.update(flt1=est(tot[0]), eps=eps, seed=seed)
        self.sure.append(rec)

    def _lag1_step(self, d_cur):
        """lsm1 of the previous frame from its flt2 (self.flt2), this frame's flt2 and, for "inv", this frame's
        backward flow (self.d_flow): seq_lag1_step of host/seq_step.c"""
        c, w, h, ch = self.ctx, self.w, self.h, self.ch
        if self.lag1 == "inv":
            c.flow_invert(self.d_fflow, self.d_flow, w, h, self.LAG1_INVERT_STEPS)
        else:
            for d_gray, d_opp in ((self.d_g0, self.flt2), (self.d_g1, d_cur)):
                c.d2d(self.d_rgb, d_opp, self.nbytes)
                c.opp2rgb(self.d_rgb, w, h, ch)
                c.gray(d_gray, self.d_rgb, w, h, ch)
            self._flow(self.d_fflow, self.of2, self.lag1_flow_iterations)
        c.occlusion_mask(self.d_focc, self.d_fflow, w, h, self.occ_th2)
        c.warp_bicubic(self.d_warp, d_cur, self.d_fflow, self.d_focc, w, h, ch)
        if self.lsm1 is None:
            self.lsm1 = self._frame()
        c.smooth_frame(self.lsm1, self.flt2, self.d_warp, None, w, h, ch, self.sigma, self.s1)

    def finish(self):
        """The last frame's lsm1: its flt2 (device pointer, opponent space)."""
        if not self.lag1:
            raise RuntimeError("SequenceFilter(lag1=None) has no lag-1 smoother to finish")
        return self.flt2

    def _frame(self):
        return self._pool.pop() if self._pool else self.ctx.alloc(self.nbytes)

    def _stage_mark(self, name):
        """(profiling only: self.stage_s is a dict) wall time since the last mark, after a device sync, added to `name`"""
        if self.stage_s is None:
            return
        import time
        self.ctx.sync()
        now = time.perf_counter()
        if name is not None:
            self.stage_s[name] = self.stage_s.get(name, 0.0) + now - self._stage_t
        self._stage_t = now

    def smooth(self, of_lambda=None, of_fscale=None, occ_th=None):
        """Backward pass over the kept flt2 frames; returns the list of smoothed frames
        (device pointers, opponent space; the last one is flt2 of the last frame)."""
        if self.history is None:
            raise RuntimeError("SequenceFilter(keep_history=False) kept no frames to smooth")
        pkg = _p()
        c, w, h, ch = self.ctx, self.w, self.h, self.ch
        of_fwd, th_fwd = self.of, self.occ_th
        self.of = pkg.tvl1_params(w, h, lam=of_lambda if of_lambda is not None else self.of.lam,
                                  fscale=of_fscale if of_fscale is not None else self.of.fscale)
        if occ_th is not None:
            self.occ_th = float(occ_th)
        out = [None] * len(self.history)
        out[-1] = self.history[-1]
        for t in range(len(self.history) - 2, -1, -1):
            # the flow tool is given flt2_t as an RGB file: convert a copy
            c.d2d(self.d_noisy, self.history[t], self.nbytes)
            c.opp2rgb(self.d_noisy, w, h, ch)
            self._flow_and_mask(self.d_noisy, out[t + 1])
            c.warp_bicubic(self.d_warp, out[t + 1], self.d_flow, self.d_occ, w, h, ch)
            out[t] = c.alloc(self.nbytes)
            c.smooth_frame(out[t], self.history[t], self.d_warp, None, w, h, ch, self.sigma, self.s1)
        self.of, self.occ_th = of_fwd, th_fwd
        return out

    def download_rgb(self, d_opp):
        """Host RGB copy of a resident opponent-space frame."""
        c = self.ctx
        c.d2d(self.d_rgb, d_opp, self.nbytes)
        c.opp2rgb(self.d_rgb, self.w, self.h, self.ch)
        if self.vst:
            c.vst_inverse(self.d_rgb, self.d_rgb, self.w * self.h * self.ch, self.ch, self.noise, self.sigma, 1)
        if self.nlf is not None:
            c.nlf_inverse(self.d_rgb, self.d_rgb, self.w * self.h * self.ch, self.ch, self.nlf)
        return c.download(self.d_rgb, (self.h, self.w, self.ch))
