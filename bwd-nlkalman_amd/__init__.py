"""bwd-nlkalman_amd — MI355X-native NL-Kalman per-frame hot path.

Python is only a thin ctypes mirror of the two C interfaces of the product:

* ``libnlkalman.so``  — the drop-in C API of include/nlkalman.h (same symbols as
  the reference's src/nlkalman.h:14-53), host pointers in / out;
* ``libnlk_hip.so``   — the C-ABI of include/nlk_hip.h over the HIP kernels,
  device pointers in / out (used by bench.py and the multi-GPU driver).

There is no CPU fallback here: every function that touches pixels needs the
HIP library and a GPU, and raises loudly otherwise.  (The directory name holds
a hyphen: import it with ``importlib.import_module("bwd-nlkalman_amd")``.)
"""
import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
FLT1, FLT2, SMO1 = 0, 1, 2

HIP_SYMBOLS = [
    "nlk_device_count", "nlk_ctx_create", "nlk_ctx_destroy", "nlk_last_error",
    "nlk_ctx_set_profiling", "nlk_ctx_get_timings", "nlk_ctx_set_stream",
    "nlk_ctx_get_stream", "nlk_ctx_use_own_stream", "nlk_dev_alloc", "nlk_dev_free", "nlk_h2d", "nlk_d2h",
    "nlk_d2d", "nlk_sync", "nlk_host_alloc", "nlk_host_free", "nlk_dev_rgb2opp", "nlk_dev_opp2rgb",
    "nlk_dev_warp_bicubic", "nlk_dev_filter_frame", "nlk_dev_smooth_frame",
    "nlk_dev_frame_accumulate", "nlk_dev_frame_normalize", "nlk_ctx_read_records",
    "nlk_dev_strip_match", "nlk_dev_strip_match_rows", "nlk_dev_mask_commit", "nlk_dev_strip_group",
    "nlk_tvl1_default_params", "nlk_tvl1_scales", "nlk_dev_tvl1_flow", "nlk_dev_gray",
    "nlk_dev_occlusion_mask", "nlk_dev_image_dct", "nlk_dev_copy_block", "nlk_host_tables", "nlk_ctx_set_deterministic", "nlk_dev_zero", "nlk_dev_add", "nlk_dev_copy_peer",
    "nlk_filter_frame_host", "nlk_smooth_frame_host", "nlk_dev_strip_match_part", "nlk_ctx_reload_switches", "nlk_ctx_last_group_shape", "nlk_ctx_last_group_packed", "nlk_host_packed_entry", "nlk_host_match_plan", "nlk_host_tvl1_plan", "nlk_ctx_count_packed", "nlk_ctx_set_strip_accumulator",
    "nlk_strips_create", "nlk_strips_destroy", "nlk_strips_last_error", "nlk_rccl_unique_id", "nlk_strips_rccl_init",
    "nlk_strips_transport", "nlk_strips_load", "nlk_strips_set_options", "nlk_strips_step", "nlk_strips_sync",
    "nlk_strips_own_rows", "nlk_strips_ctx", "nlk_strips_geometry", "nlk_strips_stats", "nlk_strips_set_dry_run",
    "nlk_dev_strip_commit_group", "nlk_ctx_flush_active",
    "nlk_dev_lz3_down", "nlk_dev_lz3_up", "nlk_dev_lz3_recompose_step",
    "nlk_dev_awgn", "nlk_dev_sqdiff_sum", "nlk_dev_ssim",
    "nlk_sigma_default_params", "nlk_dev_estimate_sigma",
    "nlk_curve_default_params", "nlk_dev_estimate_noise_curve", "nlk_vst_scale", "nlk_dev_vst_forward",
    "nlk_dev_vst_inverse", "nlk_dev_noise_affine",
    "nlk_nlf_build", "nlk_dev_nlf_forward", "nlk_dev_nlf_inverse", "nlk_dev_despike",
    "nlk_dev_defect_step", "nlk_defect_schedule",
    "nlk_yuv_format_from_tag", "nlk_yuv_frame_bytes", "nlk_dev_yuv_to_rgb", "nlk_dev_rgb_to_yuv",
    "nlk_dev_flow_invert", "nlk_bmflow_default_params", "nlk_dev_bm_flow",
    "nlk_dev_probe_add", "nlk_dev_sure_terms", "nlk_sure_mse",
    "nlk_frame_grid", "nlk_strip_plan",
]
API_SYMBOLS = [
    "rgb2opp", "opp2rgb", "warp_bicubic", "nlkalman_default_params",
    "nlkalman_filter_frame", "nlkalman_smooth_frame",
]
TVL1_SYMBOLS = ["Dual_TVL1_optic_flow_multiscale"]  # include/tvl1flow.h, exported by libnlkalman.so


class Tvl1Params(C.Structure):
    """struct nlk_tvl1_params (include/nlk_hip.h; reference: lib/tvl1flow/main.c:26-35)."""
    _fields_ = [("tau", C.c_float), ("lam", C.c_float), ("theta", C.c_float),
                ("nscales", C.c_int), ("fscale", C.c_int), ("zfactor", C.c_float),
                ("nwarps", C.c_int), ("epsilon", C.c_float)]


class BmflowParams(C.Structure):
    """struct nlk_bmflow_params (include/nlk_hip.h): the finest level that is matched, the search radius (1..3) and the
    smallest side of a pyramid level."""
    _fields_ = [("fscale", C.c_int), ("radius", C.c_int), ("min_side", C.c_int)]


class Params(C.Structure):
    """struct nlkalman_params (reference: src/nlkalman.h:22-37)."""
    _fields_ = [("patch_sz", C.c_int), ("search_sz_x", C.c_int),
                ("search_sz_t", C.c_int), ("npatches_x", C.c_int),
                ("npatches_t", C.c_int), ("npatches_tagg", C.c_int),
                ("dista_lambda", C.c_float), ("beta_x", C.c_float),
                ("beta_t", C.c_float)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class FrameGrid(C.Structure):
    """struct nlk_frame_grid (include/nlk_hip.h): the patch grid of a frame call."""
    _fields_ = [(k, C.c_int) for k in ("psz", "step", "ngx", "ngy", "halo", "reach")]


class StripPlan(C.Structure):
    """struct nlk_strip_plan (include/nlk_hip.h): grid rows, pixel rows held and pixel rows owned of one strip."""
    _fields_ = [(k, C.c_int) for k in ("gy0", "gy1", "Y0", "Y1", "own0", "own1")]


STRIPS_FEW_ROWS, STRIPS_THIN = 1, 2


class SigmaParams(C.Structure):
    """struct nlk_sigma_params (include/nlk_hip.h): the noise-level estimator's block step, selected fraction and its
    floor, and the two frequency bounds."""
    _fields_ = [("step", C.c_int), ("frac", C.c_float), ("kmin", C.c_int), ("low_max", C.c_int),
                ("high_min", C.c_int)]


class CurveParams(C.Structure):
    """struct nlk_curve_params (include/nlk_hip.h): SigmaParams' fields, then the bins of the block mean (their number
    and range) and the fewest blocks a bin needs."""
    _fields_ = [("step", C.c_int), ("frac", C.c_float), ("kmin", C.c_int), ("low_max", C.c_int),
                ("high_min", C.c_int), ("nbins", C.c_int), ("lo", C.c_float), ("hi", C.c_float), ("nmin", C.c_int)]


CURVE_BIN = np.dtype([("nblocks", np.int32), ("nsel", np.int32), ("mean", np.float32), ("var", np.float32)])


NLF_MAX_CH, NLF_MAX_BINS, NLF_RHO = 16, 64, 0.25


class NlfTable(C.Structure):
    """struct nlk_nlf_table (include/nlk_hip.h): the noise-level-function transform nlk_nlf_build makes of a noise
    curve's bins: knots x[0..nbins], per channel G[0..nbins], slope and islope[0..nbins-1], the noise level sigma at the
    knots and the bins kept; s is the scale = the sigma of a run on transformed frames (NaN: a channel kept no bin)."""
    _row = C.c_float * (NLF_MAX_BINS + 1)
    _fields_ = [("ch", C.c_int), ("nbins", C.c_int), ("lo", C.c_float), ("hi", C.c_float), ("inv_dx", C.c_float),
                ("s", C.c_float), ("kept", C.c_int * NLF_MAX_CH), ("x", _row), ("G", _row * NLF_MAX_CH),
                ("slope", _row * NLF_MAX_CH), ("islope", _row * NLF_MAX_CH), ("sigma", _row * NLF_MAX_CH)]

    def arrays(self):
        """dict of numpy copies cut to the table's sizes: x [nbins+1], G and sigma [ch][nbins+1], slope and islope
        [ch][nbins], kept [ch]"""
        ch, nb = self.ch, self.nbins
        a = {k: np.ctypeslib.as_array(getattr(self, k)).copy() for k in ("x", "G", "slope", "islope", "sigma", "kept")}
        return dict(x=a["x"][:nb + 1], G=a["G"][:ch, :nb + 1], sigma=a["sigma"][:ch, :nb + 1],
                    slope=a["slope"][:ch, :nb], islope=a["islope"][:ch, :nb], kept=a["kept"][:ch])


class YuvFormat(C.Structure):
    """struct nlk_yuv_format (include/nlk_hip.h): a planar Y'CbCr frame's subsampling, chroma siting, sample depth,
    range and matrix."""
    _fields_ = [("mono", C.c_int), ("sx", C.c_int), ("sy", C.c_int), ("cosited_x", C.c_int), ("depth", C.c_int),
                ("full_range", C.c_int), ("matrix", C.c_int)]

    def frame_bytes(self, w, h):
        """Bytes of one w x h frame (0 if refused)."""
        return int(hip().nlk_yuv_frame_bytes(int(w), int(h), C.byref(self)))


class Timings(C.Structure):
    _fields_ = [(k, C.c_float) for k in ("layout_ms", "match_ms", "commit_ms",
                                          "group_ms", "normalize_ms", "total_ms")]


def build(force=False):
    """Compile the in-tree libraries with hipcc/gcc (gfx950). No GPU needed."""
    args = ["make", "-j8", "-C", _HERE, "all"]
    if force:
        args.insert(1, "-B")
    subprocess.check_call(args)


def _load(name):
    path = os.path.join(_HERE, name)
    if not os.path.exists(path):
        raise RuntimeError(
            f"{name} is not built: run `python -c 'import __graft_entry__ as g; g.build()'` "
            "(the HIP path is mandatory, there is no CPU fallback)")
    return C.CDLL(path, mode=C.RTLD_GLOBAL)


_hip = None
_api = None


def hip():
    """libnlk_hip.so with argtypes set."""
    global _hip
    if _hip is None:
        L = _load("libnlk_hip.so")
        vp, fp, i, f = C.c_void_p, C.c_void_p, C.c_int, C.c_float
        L.nlk_device_count.restype = i
        L.nlk_ctx_create.argtypes = [C.POINTER(vp), i]
        L.nlk_ctx_destroy.argtypes = [vp]
        L.nlk_ctx_destroy.restype = None
        L.nlk_last_error.argtypes = [vp]
        L.nlk_last_error.restype = C.c_char_p
        L.nlk_ctx_set_profiling.argtypes = [vp, i]
        L.nlk_ctx_get_timings.argtypes = [vp, C.POINTER(Timings)]
        L.nlk_ctx_set_stream.argtypes = [vp, vp]
        L.nlk_ctx_use_own_stream.argtypes = [vp]
        L.nlk_ctx_get_stream.argtypes = [vp]
        L.nlk_ctx_get_stream.restype = vp
        L.nlk_dev_alloc.argtypes = [vp, C.POINTER(vp), C.c_size_t]
        L.nlk_dev_free.argtypes = [vp, vp]
        for fn in (L.nlk_h2d, L.nlk_d2h, L.nlk_d2d):
            fn.argtypes = [vp, vp, vp, C.c_size_t]
        L.nlk_sync.argtypes = [vp]
        for fn in (L.nlk_dev_rgb2opp, L.nlk_dev_opp2rgb):
            fn.argtypes = [vp, fp, i, i, i]
        L.nlk_dev_warp_bicubic.argtypes = [vp, fp, fp, fp, fp, i, i, i]
        for fn in (L.nlk_dev_filter_frame, L.nlk_dev_smooth_frame):
            fn.argtypes = [vp, fp, fp, fp, fp, i, i, i, f, C.POINTER(Params)]
        L.nlk_dev_frame_accumulate.argtypes = [vp, fp, fp, fp, fp, i, i, i, f,
                                               C.POINTER(Params), i, i, i]
        L.nlk_dev_frame_normalize.argtypes = [vp, fp, fp, fp, i, i, i, i, i]
        L.nlk_dev_strip_match.argtypes = [vp, fp, fp, fp, i, i, i, f, C.POINTER(Params), i, i, i,
                                          vp, C.POINTER(i)]
        L.nlk_dev_strip_match_rows.argtypes = [vp, fp, fp, fp, i, i, i, f, C.POINTER(Params), i, i, i, i, i,
                                               vp, C.POINTER(i)]
        L.nlk_dev_strip_match_part.argtypes = [vp, fp, fp, fp, i, i, i, f, C.POINTER(Params), i, i, i, i, i, i, i, i, i,
                                               vp, C.POINTER(i)]
        L.nlk_dev_mask_commit.argtypes = [vp, vp, i, i, i, vp]
        L.nlk_dev_strip_group.argtypes = [vp, fp, vp]
        L.nlk_dev_strip_commit_group.argtypes = [vp, fp, vp, i, i, i, i, vp]
        L.nlk_ctx_read_records.argtypes = [vp, C.POINTER(i), C.POINTER(i), C.POINTER(i),
                                           vp, vp, vp, vp, vp, vp]
        L.nlk_tvl1_default_params.argtypes = [C.POINTER(Tvl1Params)]
        L.nlk_tvl1_default_params.restype = None
        L.nlk_tvl1_scales.argtypes = [i, i, i, f]
        L.nlk_dev_tvl1_flow.argtypes = [vp, fp, fp, fp, i, i, C.POINTER(Tvl1Params), C.POINTER(i)]
        L.nlk_dev_gray.argtypes = [vp, fp, fp, i, i, i]
        L.nlk_dev_occlusion_mask.argtypes = [vp, fp, fp, i, i, f]
        L.nlk_dev_flow_invert.argtypes = [vp, fp, fp, i, i, i]
        L.nlk_bmflow_default_params.argtypes = [C.POINTER(BmflowParams)]
        L.nlk_bmflow_default_params.restype = None
        L.nlk_dev_bm_flow.argtypes = [vp, fp, fp, fp, i, i, C.POINTER(BmflowParams)]
        L.nlk_dev_image_dct.argtypes = [vp, fp, i, i, i, i]
        L.nlk_dev_copy_block.argtypes = [vp, fp, i, fp, i, i, i, i]
        L.nlk_dev_lz3_down.argtypes = [vp, fp, fp, i, i, i]
        L.nlk_dev_lz3_up.argtypes = [vp, fp, i, i, fp, i, i, i]
        L.nlk_dev_lz3_recompose_step.argtypes = [vp, fp, fp, i, i, fp, i, i, i, f]
        L.nlk_dev_awgn.argtypes = [vp, fp, fp, C.c_size_t, f, C.c_uint32]
        L.nlk_dev_sqdiff_sum.argtypes = [vp, vp, fp, fp, C.c_size_t]
        L.nlk_dev_ssim.argtypes = [vp, vp, fp, fp, fp, i, i, i, f]
        L.nlk_dev_probe_add.argtypes = [vp, fp, fp, C.c_size_t, f, C.c_uint64]
        L.nlk_dev_sure_terms.argtypes = [vp, vp, vp, fp, fp, fp, i, i, i, i, C.c_uint64]
        L.nlk_sure_mse.argtypes = [C.c_double] * 5
        L.nlk_sure_mse.restype = C.c_double
        L.nlk_sigma_default_params.argtypes = [C.POINTER(SigmaParams)]
        L.nlk_sigma_default_params.restype = None
        L.nlk_dev_estimate_sigma.argtypes = [vp, fp, vp, fp, i, i, i, C.POINTER(SigmaParams)]
        L.nlk_curve_default_params.argtypes = [C.POINTER(CurveParams)]
        L.nlk_curve_default_params.restype = None
        L.nlk_dev_estimate_noise_curve.argtypes = [vp, fp, vp, fp, i, i, i, C.POINTER(CurveParams)]
        L.nlk_vst_scale.argtypes = [vp, i]
        L.nlk_vst_scale.restype = f
        L.nlk_dev_vst_forward.argtypes = [vp, fp, fp, C.c_size_t, i, vp, f]
        L.nlk_dev_vst_inverse.argtypes = [vp, fp, fp, C.c_size_t, i, vp, f, i]
        L.nlk_dev_noise_affine.argtypes = [vp, fp, fp, C.c_size_t, i, vp, C.c_uint32]
        L.nlk_nlf_build.argtypes = [C.POINTER(NlfTable), vp, i, i, f, f, f]
        for fn in (L.nlk_dev_nlf_forward, L.nlk_dev_nlf_inverse):
            fn.argtypes = [vp, fp, fp, C.c_size_t, i, C.POINTER(NlfTable)]
        L.nlk_dev_despike.argtypes = [vp, fp, fp, vp, i, i, i, i, f]
        L.nlk_dev_defect_step.argtypes = [vp, fp, fp, fp, fp, vp, vp, i, i, i, i, f, f]
        L.nlk_defect_schedule.argtypes = [C.c_long, i, f, C.POINTER(C.c_float), C.POINTER(C.c_float)]
        L.nlk_yuv_format_from_tag.argtypes = [C.POINTER(YuvFormat), C.c_char_p]
        L.nlk_yuv_frame_bytes.argtypes = [i, i, C.POINTER(YuvFormat)]
        L.nlk_yuv_frame_bytes.restype = C.c_size_t
        L.nlk_dev_yuv_to_rgb.argtypes = [vp, fp, vp, i, i, C.POINTER(YuvFormat)]
        L.nlk_dev_rgb_to_yuv.argtypes = [vp, vp, fp, i, i, C.POINTER(YuvFormat)]
        L.nlk_host_tables.argtypes = [i, vp, vp, vp]
        L.nlk_frame_grid.argtypes = [i, i, C.POINTER(Params), i, i, C.POINTER(FrameGrid)]
        L.nlk_strip_plan.argtypes = [i, C.POINTER(FrameGrid), i, C.POINTER(StripPlan)]
        L.nlk_ctx_set_deterministic.argtypes = [vp, i]
        L.nlk_ctx_reload_switches.argtypes = [vp]
        L.nlk_ctx_last_group_shape.argtypes = [vp, C.POINTER(i)]
        L.nlk_ctx_last_group_packed.argtypes = [vp]
        L.nlk_host_packed_entry.argtypes = [i, i, i, i, i, i, i, C.POINTER(C.c_uint), C.POINTER(i)]
        L.nlk_host_match_plan.argtypes = [i, i, i, C.POINTER(Params), i, i, i, C.POINTER(i)]
        L.nlk_host_tvl1_plan.argtypes = [i, i, C.POINTER(Tvl1Params), i, C.POINTER(i), C.POINTER(i)]
        L.nlk_ctx_count_packed.argtypes = [vp, C.POINTER(i)]
        L.nlk_ctx_set_strip_accumulator.argtypes = [vp, vp]
        L.nlk_strips_create.argtypes = [C.POINTER(vp), i, C.POINTER(i), i, i, i, i, i, C.c_float, C.POINTER(Params), i, i]
        L.nlk_strips_destroy.argtypes = [vp]
        L.nlk_strips_destroy.restype = None
        L.nlk_strips_last_error.argtypes = [vp]
        L.nlk_strips_last_error.restype = C.c_char_p
        L.nlk_rccl_unique_id.argtypes = [vp]
        L.nlk_strips_rccl_init.argtypes = [vp, vp]
        L.nlk_strips_transport.argtypes = [vp]
        L.nlk_strips_transport.restype = C.c_char_p
        L.nlk_strips_load.argtypes = [vp, i, vp, vp]
        L.nlk_strips_set_options.argtypes = [vp, i, i, i]
        L.nlk_strips_step.argtypes = [vp]
        L.nlk_strips_set_dry_run.argtypes = [vp, i]
        L.nlk_strips_sync.argtypes = [vp]
        L.nlk_strips_own_rows.argtypes = [vp, i, C.POINTER(i), C.POINTER(i), C.POINTER(vp), C.POINTER(vp), C.POINTER(vp)]
        L.nlk_strips_ctx.argtypes = [vp, i]
        L.nlk_strips_ctx.restype = vp
        L.nlk_strips_geometry.argtypes = [vp, i, C.POINTER(i)]
        L.nlk_strips_stats.argtypes = [vp, C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(i)]
        _hip = L
    return _hip


def api():
    """libnlkalman.so (drop-in C API) with argtypes set."""
    global _api
    if _api is None:
        hip()  # dependency, RTLD_GLOBAL
        L = _load("libnlkalman.so")
        fp, i, f = C.POINTER(C.c_float), C.c_int, C.c_float
        for fn in (L.rgb2opp, L.opp2rgb):
            fn.argtypes = [fp, i, i, i]
            fn.restype = None
        L.warp_bicubic.argtypes = [fp, fp, fp, fp, i, i, i]
        L.warp_bicubic.restype = None
        L.nlkalman_default_params.argtypes = [C.POINTER(Params), f, i]
        L.nlkalman_default_params.restype = None
        for fn in (L.nlkalman_filter_frame, L.nlkalman_smooth_frame):
            fn.argtypes = [fp, fp, fp, fp, i, i, i, f, Params, i]
            fn.restype = None
        _api = L
    return _api


class NlkError(RuntimeError):
    pass


def _fp(a):
    return None if a is None else a.ctypes.data_as(C.POINTER(C.c_float))


def _img(a):
    if a is None:
        return None
    a = np.ascontiguousarray(a, dtype=np.float32)
    return a[:, :, None] if a.ndim == 2 else a


# ---------------------------------------------------------------- drop-in API

def tvl1_params(w, h, **over):
    """nlk_tvl1_default_params + the scale count the reference's command line would use
    for a w x h image (fields may be overridden, e.g. lam=0.4, fscale=1)."""
    p = Tvl1Params()
    hip().nlk_tvl1_default_params(C.byref(p))
    for k, v in over.items():
        setattr(p, k, v)
    p.nscales = hip().nlk_tvl1_scales(w, h, p.nscales, p.zfactor)
    p.fscale = min(p.fscale, p.nscales)
    return p


def bmflow_params(fscale=None, radius=None, min_side=None):
    """nlk_bmflow_default_params, with the fields given overridden."""
    p = BmflowParams()
    hip().nlk_bmflow_default_params(C.byref(p))
    for k, v in (("fscale", fscale), ("radius", radius), ("min_side", min_side)):
        if v is not None:
            setattr(p, k, int(v))
    return p


def yuv_format_from_tag(tag=None, full_range=False, matrix=709):
    """nlk_yuv_format_from_tag: the YuvFormat of a YUV4MPEG2 `C` tag value (None or "" = the tag is absent), with the
    range and matrix the caller chooses. An unsupported tag raises NlkError."""
    f = YuvFormat()
    rc = hip().nlk_yuv_format_from_tag(C.byref(f), None if tag is None else str(tag).encode())
    if rc:
        raise NlkError(f"rc={rc}: " + hip().nlk_last_error(None).decode())
    f.full_range, f.matrix = int(bool(full_range)), int(matrix)
    return f


def sigma_params(**over):
    """nlk_sigma_default_params (step 4, frac 0.05, kmin 64, low_max 5, high_min 8) with fields overridden."""
    p = SigmaParams()
    hip().nlk_sigma_default_params(C.byref(p))
    for k, v in over.items():
        if k not in dict(p._fields_):
            raise TypeError(f"sigma_params: no field {k!r}")
        setattr(p, k, v)
    return p


def curve_params(**over):
    """nlk_curve_default_params (step 4, frac 0.1, kmin 32, low_max 5, high_min 8, nbins 16, lo 0, hi 256, nmin 32)
    with fields overridden."""
    p = CurveParams()
    hip().nlk_curve_default_params(C.byref(p))
    for k, v in over.items():
        if k not in dict(p._fields_):
            raise TypeError(f"curve_params: no field {k!r}")
        setattr(p, k, v)
    return p


def _ab(ab, ch):
    """(a, b) for every channel, or [ch][2] -> a contiguous float32 [ch][2]"""
    a = np.asarray(ab, np.float32)
    a = np.tile(a, (ch, 1)) if a.ndim == 1 else a
    if a.shape != (ch, 2):
        raise ValueError(f"noise coefficients: want (a, b) or [{ch}][2], got shape {a.shape}")
    return np.ascontiguousarray(a)


def vst_scale(ab, ch=None):
    """nlk_vst_scale: the common scale s = 255 / mean_c(span_c) of the variance-stabilising transform for the
    coefficients ab ((a, b) with ch given, or [ch][2]); host-only."""
    a = _ab(ab, ch if ch is not None else len(np.atleast_2d(ab)))
    s = float(hip().nlk_vst_scale(a.ctypes.data, len(a)))
    if not s > 0:
        raise ValueError(f"vst_scale: refused coefficients {a.tolist()}")
    return s


def nlf_build(bins, lo=0.0, hi=256.0, rho=NLF_RHO):
    """nlk_nlf_build: the NlfTable of the bins [ch][nbins] (CURVE_BIN, as Context.estimate_noise_curve returns them)
    measured over [lo, hi); host-only. Refused arguments raise ValueError; a channel that kept no bin gives a table
    with s = NaN."""
    b = np.ascontiguousarray(bins, CURVE_BIN)
    if b.ndim != 2:
        raise ValueError(f"nlf_build: want bins [ch][nbins], got shape {b.shape}")
    t = NlfTable()
    rc = hip().nlk_nlf_build(C.byref(t), b.ctypes.data, b.shape[0], b.shape[1], float(lo), float(hi), float(rho))
    if rc:
        raise ValueError(f"nlf_build: refused (rc={rc}): ch = {b.shape[0]}, nbins = {b.shape[1]}, lo = {lo}, hi = {hi}, rho = {rho}")
    return t


def frame_grid(w, h, params, smoother=False, have_prev=False):
    """nlk_frame_grid: the FrameGrid of a w x h frame call; host-only. ValueError where no patch grid exists."""
    g = FrameGrid()
    if hip().nlk_frame_grid(int(w), int(h), C.byref(params), int(smoother), int(have_prev), C.byref(g)):
        raise ValueError(f"frame_grid: patch size {params.patch_sz} on a {w}x{h} frame")
    return g


def strip_plan(h, grid, world):
    """nlk_strip_plan: the strips of an h-row frame with this FrameGrid, one dict(gy0, gy1, Y0, Y1, own0, own1) per
    rank like strips.strip_plan; host-only. ValueError, whose args[1] is STRIPS_FEW_ROWS or STRIPS_THIN, where the
    frame cannot be split."""
    plan = (StripPlan * world)()
    rc = hip().nlk_strip_plan(int(h), C.byref(grid), int(world), plan)
    if rc:
        raise ValueError(f"strip_plan: {grid.ngy} grid rows, halo {grid.halo}, {world} ranks (rc={rc})", rc)
    return [{k: getattr(q, k) for k, _ in StripPlan._fields_} for q in plan]


def sure_mse(R, D, n, sigma, eps):
    """Monte-Carlo SURE from its two sums over n samples (nlk_sure_mse): R / n - sigma^2 + 2 sigma^2 D / (eps n)."""
    return float(hip().nlk_sure_mse(float(R), float(D), float(n), float(sigma), float(eps)))


def default_params(sigma, mode, **over):
    """nlkalman_default_params (reference: src/nlkalman.c:426-487); host-only."""
    p = Params(-1, -1, -1, -1, -1, -1, -1.0, -1.0, -1.0)
    for k, v in over.items():
        setattr(p, k, v)
    api().nlkalman_default_params(C.byref(p), float(sigma), int(mode))
    return p


def filter_frame(nisy1, deno0, bsic1, sigma, params):
    """nlkalman_filter_frame through the drop-in C API (host arrays)."""
    nisy1, deno0, bsic1 = _img(nisy1), _img(deno0), _img(bsic1)
    h, w, ch = nisy1.shape
    out = np.empty_like(nisy1)
    api().nlkalman_filter_frame(_fp(out), _fp(nisy1), _fp(deno0), _fp(bsic1), w, h, ch,
                                float(sigma), params, 0)
    return out


def smooth_frame(filt1, smoo0, bsic1, sigma, params):
    filt1, smoo0, bsic1 = _img(filt1), _img(smoo0), _img(bsic1)
    h, w, ch = filt1.shape
    out = np.empty_like(filt1)
    api().nlkalman_smooth_frame(_fp(out), _fp(filt1), _fp(smoo0), _fp(bsic1), w, h, ch,
                                float(sigma), params, 0)
    return out


def rgb2opp(im):
    a = _img(im).copy()
    api().rgb2opp(_fp(a), a.shape[1], a.shape[0], a.shape[2])
    return a


def opp2rgb(im):
    a = _img(im).copy()
    api().opp2rgb(_fp(a), a.shape[1], a.shape[0], a.shape[2])
    return a


def warp_bicubic(im, flow, occ=None):
    im = _img(im)
    h, w, ch = im.shape
    flow = np.ascontiguousarray(flow, np.float32)
    occ = None if occ is None else np.ascontiguousarray(occ, np.float32)
    out = np.empty_like(im)
    api().warp_bicubic(_fp(out), _fp(im), _fp(flow), _fp(occ), w, h, ch)
    return out


def host_tables(psz):
    """The DCT basis and aggregation window a frame call uploads for this patch size, and the 12x12
    matrix the 12-point flow graph of k_dct12.h applies (nlk_host_tables; no device needed)."""
    b, w, b12 = (np.zeros((psz, psz), np.float32), np.zeros((psz, psz), np.float32),
                 np.zeros((12, 12), np.float32))
    rc = hip().nlk_host_tables(psz, b.ctypes.data, w.ctypes.data, b12.ctypes.data)
    if rc:
        raise NlkError(hip().nlk_last_error(None).decode())
    return b, w, b12


def host_packed_entry(dx, dy, r, k=1, px=16, py=16, passthrough=False):
    """(byte, (x, y) decoded from it) of one entry of the packed candidate / member lists: displacement (dx, dy) from a
    target at (px, py) that searched radius r and kept k candidates - through the functions the matcher and the group
    kernel call (nlk_host_packed_entry; no device needed); None where a packed record cannot hold it."""
    byte, back = C.c_uint(0), (C.c_int * 2)()
    if hip().nlk_host_packed_entry(px, py, dx, dy, r, k, int(passthrough), C.byref(byte), back):
        return None
    return byte.value, (back[0], back[1])


MATCH_PLAN_FIELDS = ("generic", "wide", "tgx", "tgy", "bx", "threads", "block", "order", "halo", "rwp", "rh_max",
                     "ksel_max", "ntx", "rounds", "lds", "wide_halo", "wide_rwp", "wide_rh_max", "wide_rounds", "wide_lds")


def host_match_plan(w, h, ch, params, smoother=False, have_prev=False, rows=0):
    """The launch plan of a frame call's block matching as a dict of MATCH_PLAN_FIELDS (nlk_host_match_plan: the frame
    call's geometry code and planner, the NLK_* switches from the environment; no device needed). rows: the call's
    target rows, 0 = the whole grid. NlkError, whose args[1] is the frame call's error code, for refused inputs."""
    out = (C.c_int * len(MATCH_PLAN_FIELDS))()
    rc = hip().nlk_host_match_plan(int(w), int(h), int(ch), C.byref(params), int(smoother), int(have_prev), int(rows), out)
    if rc:
        raise NlkError(hip().nlk_last_error(None).decode(), rc)
    return dict(zip(MATCH_PLAN_FIELDS, out))


TVL1_PLAN_FIELDS = ("nx", "ny", "solved", "driver", "threads", "shape", "tw", "th", "gx", "gy", "inline", "look")
TVL1_DRIVER_WG, TVL1_DRIVER_BLOCKED, TVL1_DRIVER_PLAIN = 0, 1, 2


def host_tvl1_plan(w, h, params):
    """The plan of every pyramid level of a TV-L1 flow call, finest first, as a list of dicts of TVL1_PLAN_FIELDS
    (nlk_host_tvl1_plan: the flow call's checks, layout walk and level planner, the NLK_TV_* switches from the
    environment; no device needed). NlkError, whose args[1] is the flow call's error code, for refused inputs."""
    n, levels = len(TVL1_PLAN_FIELDS), C.c_int(0)
    out = (C.c_int * (64 * n))()
    rc = hip().nlk_host_tvl1_plan(int(w), int(h), C.byref(params), 64, out, C.byref(levels))
    if rc:
        raise NlkError(hip().nlk_last_error(None).decode(), rc)
    return [dict(zip(TVL1_PLAN_FIELDS, out[s * n:(s + 1) * n])) for s in range(levels.value)]


def reload_switches():
    """Re-read the NLK_* environment switches for every live context of this process (they are read once,
    at context creation: include/nlk_hip.h). Only the tests need this."""
    if _hip is not None:
        _hip.nlk_ctx_reload_switches(None)


# ------------------------------------------------------- device-resident C-ABI

class Lz3Levels(list):
    """[(dptr, w, h)] of a Lanczos-3 pyramid, finest first; .ch = the channel count (Context.lz3_decompose)."""
    ch = None


class Context:
    """nlk_ctx wrapper: device pointers are plain ints (e.g. tensor.data_ptr())."""

    def __init__(self, device=0):
        self.L = hip()
        self.h = C.c_void_p()
        rc = self.L.nlk_ctx_create(C.byref(self.h), int(device))
        if rc:
            raise NlkError(self.L.nlk_last_error(None).decode())

    @classmethod
    def from_handle(cls, handle):
        """A view of a context somebody else owns (a strip's: nlk_strips_ctx); never destroyed from here."""
        c = cls.__new__(cls)
        c.L, c.h, c._borrowed = hip(), C.c_void_p(handle), True
        return c

    def close(self):
        if self.h and not getattr(self, "_borrowed", False):
            self.L.nlk_ctx_destroy(self.h)
        self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc):
        if rc:
            raise NlkError(f"rc={rc}: " + self.L.nlk_last_error(self.h).decode())

    def set_stream(self, hip_stream):
        self._chk(self.L.nlk_ctx_set_stream(self.h, hip_stream))

    def set_deterministic(self, on):
        """Bit-reproducible aggregation (slabs + ordered gather instead of float atomics)."""
        self._chk(self.L.nlk_ctx_set_deterministic(self.h, int(on)))

    def last_group_shape(self):
        """What the last group launch ran (nlk_ctx_last_group_shape): family "k_group8m" / None (another
        launcher), sep, tgx, tgy, ntx, nty, nty_full, single, passes, chase (reach of the replay inside the launch, 0 =
        not in it), far = (tgx, tgy) of deterministic mode's far pass or None, packed_lists / packed_far = the launch / its far
        pass read the lists packed (nlk_ctx_last_group_packed)."""
        out = (C.c_int * 12)()
        self._chk(self.L.nlk_ctx_last_group_shape(self.h, out))
        v = list(out)
        d = dict(zip(("sep", "tgx", "tgy", "ntx", "nty", "nty_full", "single", "passes", "chase"), v[1:10]))
        d["family"] = {1: "k_group8m"}.get(v[0])
        d["far"] = (v[10], v[11]) if v[8] > 1 else None
        pk = self.L.nlk_ctx_last_group_packed(self.h)
        d["packed_lists"], d["packed_far"] = pk > 0 and bool(pk & 1), pk > 0 and bool(pk & 2)
        return d

    def count_packed(self):
        """Targets of the last match phase with a valid packed record (nlk_ctx_count_packed)."""
        n = C.c_int()
        self._chk(self.L.nlk_ctx_count_packed(self.h, C.byref(n)))
        return n.value

    def set_profiling(self, on):
        self._chk(self.L.nlk_ctx_set_profiling(self.h, int(on)))

    def timings(self):
        t = Timings()
        self._chk(self.L.nlk_ctx_get_timings(self.h, C.byref(t)))
        return {k: getattr(t, k) for k, _ in t._fields_}

    def sync(self):
        self._chk(self.L.nlk_sync(self.h))

    def alloc(self, nbytes):
        p = C.c_void_p()
        self._chk(self.L.nlk_dev_alloc(self.h, C.byref(p), nbytes))
        return p.value

    def free(self, dptr):
        self._chk(self.L.nlk_dev_free(self.h, dptr))

    def d2d(self, d_dst, d_src, nbytes):
        self._chk(self.L.nlk_d2d(self.h, d_dst, d_src, nbytes))

    def upload(self, arr):
        arr = np.ascontiguousarray(arr)
        d = self.alloc(arr.nbytes)
        self._chk(self.L.nlk_h2d(self.h, d, arr.ctypes.data, arr.nbytes))
        return d

    def download(self, dptr, shape, dtype=np.float32):
        out = np.empty(shape, dtype)
        self._chk(self.L.nlk_d2h(self.h, out.ctypes.data, dptr, out.nbytes))
        return out

    def rgb2opp(self, d_im, w, h, ch):
        self._chk(self.L.nlk_dev_rgb2opp(self.h, d_im, w, h, ch))

    def opp2rgb(self, d_im, w, h, ch):
        self._chk(self.L.nlk_dev_opp2rgb(self.h, d_im, w, h, ch))

    def warp_bicubic(self, d_out, d_im, d_flow, d_occ, w, h, ch):
        self._chk(self.L.nlk_dev_warp_bicubic(self.h, d_out, d_im, d_flow, d_occ, w, h, ch))

    def filter_frame(self, d_out, d_nisy, d_prev, d_basic, w, h, ch, sigma, params):
        self._chk(self.L.nlk_dev_filter_frame(self.h, d_out, d_nisy, d_prev, d_basic, w, h,
                                              ch, float(sigma), C.byref(params)))

    def smooth_frame(self, d_out, d_filt, d_prev, d_basic, w, h, ch, sigma, params):
        self._chk(self.L.nlk_dev_smooth_frame(self.h, d_out, d_filt, d_prev, d_basic, w, h,
                                              ch, float(sigma), C.byref(params)))

    def tvl1_flow(self, d_flow, d_i0, d_i1, w, h, params):
        """Flow I0 -> I1 into d_flow (w*h interleaved pairs); returns the iteration count."""
        it = C.c_int()
        self._chk(self.L.nlk_dev_tvl1_flow(self.h, d_flow, d_i0, d_i1, w, h, C.byref(params),
                                           C.byref(it)))
        return it.value

    def gray(self, d_gray, d_im, w, h, ch):
        self._chk(self.L.nlk_dev_gray(self.h, d_gray, d_im, w, h, ch))

    def occlusion_mask(self, d_mask, d_flow, w, h, th):
        self._chk(self.L.nlk_dev_occlusion_mask(self.h, d_mask, d_flow, w, h, float(th)))

    def flow_invert(self, d_inv, d_flow, w, h, iters=4):
        """The inverse of a flow by `iters` fixed-point steps (nlk_dev_flow_invert; tests/flowinv_ref.py restates it)."""
        self._chk(self.L.nlk_dev_flow_invert(self.h, d_inv, d_flow, w, h, int(iters)))

    def bm_flow(self, d_flow, d_i0, d_i1, w, h, fscale=None, radius=None, min_side=None):
        """Block-matching flow I0 -> I1 into d_flow (w*h interleaved pairs, nlk_dev_bm_flow; tests/bmflow_ref.py restates
        it). Parameters left None are nlk_bmflow_default_params' (1, 2, 16)."""
        p = bmflow_params(fscale, radius, min_side)
        self._chk(self.L.nlk_dev_bm_flow(self.h, d_flow, d_i0, d_i1, w, h, C.byref(p)))

    def image_dct(self, d_img, w, h, ch, inverse=False):
        self._chk(self.L.nlk_dev_image_dct(self.h, d_img, w, h, ch, int(inverse)))

    def copy_block(self, d_dst, dw, d_src, sw, ch, bw, bh):
        self._chk(self.L.nlk_dev_copy_block(self.h, d_dst, dw, d_src, sw, ch, bw, bh))

    # ---- Lanczos-3 pyramid (the lz3 multiscale pipeline's decompose / recompose; include/nlk_hip.h)
    def lz3_down(self, d_dst, d_src, w, h, ch):
        """d_dst (ceil(w/2) x ceil(h/2) x ch) = the Lanczos-3 half-band downsampling of d_src."""
        self._chk(self.L.nlk_dev_lz3_down(self.h, d_dst, d_src, w, h, ch))

    def lz3_up(self, d_dst, dw, dh, d_src, w, h, ch):
        """d_dst (dw x dh x ch) = the 2x Lanczos-3 upsampling of d_src, fitted to dw, dh (2n - 1, 2n or 2n + 1)."""
        self._chk(self.L.nlk_dev_lz3_up(self.h, d_dst, dw, dh, d_src, w, h, ch))

    def lz3_recompose_step(self, d_out, d_yh, w, h, d_rl, wl, hl, ch, g=0.0):
        """d_out = yh + up(gblur(rl - down(yh), g)) (w x h); rl is the recomposed coarser level."""
        self._chk(self.L.nlk_dev_lz3_recompose_step(self.h, d_out, d_yh, w, h, d_rl, wl, hl, ch, float(g)))

    def lz3_decompose(self, d_img, w, h, ch, levels):
        """The pyramid of lanczos3_decompose: [(dptr, w, h)] for levels 0 .. levels - 1, level 0 being d_img itself
        (not copied); the other levels are new allocations of the caller's. Nothing is synchronised."""
        out = Lz3Levels([(d_img, w, h)])
        out.ch = ch
        for _ in range(1, levels):
            d = self.alloc(((w + 1) // 2) * ((h + 1) // 2) * ch * 4)
            self.lz3_down(d, out[-1][0], w, h, ch)
            w, h = (w + 1) // 2, (h + 1) // 2
            out.append((d, w, h))
        return out

    def lz3_recompose(self, levels, g=0.0, ch=None):
        """R_0 of lanczos3_recompose from the levels [(dptr, w, h)], finest first (what lz3_decompose returns, or
        the same shape of list with `ch` given): R_l = Y_l + up(gblur(R_{l+1} - down(Y_l), g)). Every level stays
        resident and nothing waits for the device between levels; returns a new allocation (the levels are not
        changed) of levels[0]'s size."""
        ch = getattr(levels, "ch", None) if ch is None else ch
        if ch is None:
            raise ValueError("lz3_recompose: the channel count is unknown (pass ch=)")
        r, rw, rh = levels[-1]
        if len(levels) == 1:
            out = self.alloc(rw * rh * ch * 4)
            self.d2d(out, r, rw * rh * ch * 4)
            return out
        outs = [self.alloc(w * h * ch * 4) for (_, w, h) in levels[:-1]]
        for l in range(len(levels) - 2, -1, -1):
            y, w, h = levels[l]
            self.lz3_recompose_step(outs[l], y, w, h, r, rw, rh, ch, g)
            r, rw, rh = outs[l], w, h
        for d in outs[1:]:   # (a free waits for the device: after the last level only)
            self.free(d)
        return outs[0]

    # ---- the ground-truth loop's noise and error measure (scripts/nlkalman-seq-gt.sh; include/nlk_hip.h)
    def awgn(self, d_out, d_in, n, sigma, seed):
        """d_out[i] = d_in[i] + sigma * N_i for i < n: what `SRAND=seed awgn sigma` writes (d_out may be d_in)."""
        self._chk(self.L.nlk_dev_awgn(self.h, d_out, d_in, n, float(sigma), int(seed) & 0xFFFFFFFF))

    def sqdiff_sum(self, d_sum, d_a, d_b, n):
        """*d_sum (one device double) = sum of (a[i] - b[i])^2 over i < n in double, fixed order; not synchronised."""
        self._chk(self.L.nlk_dev_sqdiff_sum(self.h, d_sum, d_a, d_b, n))

    def mse(self, d_a, d_b, n):
        """The mean of (a[i] - b[i])^2 over i < n (sqdiff_sum / n); waits for the device."""
        d = self.alloc(8)
        try:
            self.sqdiff_sum(d, d_a, d_b, n)
            s = float(self.download(d, (1,), np.float64)[0])
        finally:
            self.free(d)
        return s / n

    # ---- the quality measure (include/nlk_hip.h: nlk_dev_ssim)
    def ssim_dev(self, d_ssim, d_map, d_a, d_b, w, h, ch, range=255.0):
        """d_ssim[0] = the SSIM of the device images a (the reference) and b, d_ssim[1 + c] = that of channel c (device
        doubles); d_map: None, or the (h - 10, w - 10, ch) float32 map. Not synchronised."""
        self._chk(self.L.nlk_dev_ssim(self.h, d_ssim, d_map, d_a, d_b, w, h, ch, float(range)))

    def ssim(self, d_a, d_b, w, h, ch, range=255.0, want_map=False):
        """(ssim, ssim_ch [ch] float64) of the device images d_a (the reference) and d_b (HWC float32, dynamic range
        `range`); with want_map also the (h - 10, w - 10, ch) float32 map of S. Waits for the device."""
        nres, nmap = 1 + max(ch, 0), max(h - 10, 0) * max(w - 10, 0) * max(ch, 0)
        d = self.alloc(8 * nres)
        d_map = self.alloc(4 * max(nmap, 1)) if want_map else None
        try:
            self.ssim_dev(d, d_map, d_a, d_b, w, h, ch, range)
            s = self.download(d, (nres,), np.float64)
            smap = self.download(d_map, (h - 10, w - 10, ch)) if want_map else None
        finally:
            self.free(d)
            if d_map is not None:
                self.free(d_map)
        return (float(s[0]), s[1:].copy(), smap) if want_map else (float(s[0]), s[1:].copy())

    # ---- the error estimate without clean frames (include/nlk_hip.h: nlk_dev_probe_add, nlk_dev_sure_terms)
    def probe_add(self, d_out, d_in, n, eps, seed):
        """d_out[i] = d_in[i] + (b_i > 0 ? eps : -eps) for i < n, b the signs of `seed` (d_out may be d_in)."""
        self._chk(self.L.nlk_dev_probe_add(self.h, d_out, d_in, n, float(eps), int(seed) & 0xFFFFFFFFFFFFFFFF))

    def sure_terms_dev(self, d_total, d_blocks, d_y, d_f, d_fp, w, h, ch, block=16, seed=0):
        """d_total[2 c], d_total[2 c + 1] = R_c, D_c of the device images y, f = filter(y), fp = filter(y + eps b)
        (device doubles); d_blocks: None, or the [nby][nbx][ch][2] map of the same sums per tile. Not synchronised."""
        self._chk(self.L.nlk_dev_sure_terms(self.h, d_total, d_blocks, d_y, d_f, d_fp, w, h, ch, block,
                                            int(seed) & 0xFFFFFFFFFFFFFFFF))

    def sure_terms(self, d_y, d_f, d_fp, w, h, ch, block=16, seed=0, want_blocks=False):
        """totals [ch][2] float64 = (R_c, D_c); with want_blocks also the map [nby][nbx][ch][2]. Waits for the device."""
        nby, nbx = -(-max(h, 1) // max(block, 1)), -(-max(w, 1) // max(block, 1))
        d = self.alloc(16 * max(ch, 1))
        d_map = self.alloc(16 * max(ch, 1) * nby * nbx) if want_blocks else None
        try:
            self.sure_terms_dev(d, d_map, d_y, d_f, d_fp, w, h, ch, block, seed)
            tot = self.download(d, (ch, 2), np.float64)
            blocks = self.download(d_map, (nby, nbx, ch, 2), np.float64) if want_blocks else None
        finally:
            self.free(d)
            if d_map is not None:
                self.free(d_map)
        return (tot, blocks) if want_blocks else tot

    # ---- the noise level of an image (include/nlk_hip.h: nlk_dev_estimate_sigma)
    def estimate_sigma(self, d_img, w, h, ch, **params):
        """(sigma, sigma_ch [ch] float32, counts [ch][2] int32 = blocks kept and blocks selected per channel) of the
        device image d_img (HWC, 0..255 scale); params: the fields of SigmaParams. Waits for the device."""
        p = sigma_params(**params)
        d = self.alloc(4 * (1 + 3 * ch))
        try:
            self._chk(self.L.nlk_dev_estimate_sigma(self.h, d, d + 4 * (1 + ch), d_img, w, h, ch, C.byref(p)))
            s = self.download(d, (1 + ch,))
            counts = self.download(d + 4 * (1 + ch), (ch, 2), np.int32)
        finally:
            self.free(d)
        return float(s[0]), s[1:].copy(), counts

    # ---- signal-dependent noise (include/nlk_hip.h: nlk_dev_estimate_noise_curve, nlk_dev_vst_*, nlk_dev_noise_affine)
    def estimate_noise_curve(self, d_img, w, h, ch, **params):
        """(ab [ch][2] float32 = (a_c, b_c) of var = a mean + b, bins [ch][nbins] of CURVE_BIN = N_q, n_q, m_q, v_q) of
        the device image d_img (HWC, 0..255 scale); params: the fields of CurveParams. Waits for the device."""
        p = curve_params(**params)
        nb = max(int(p.nbins), 0)
        d = self.alloc(8 * ch + 16 * ch * max(nb, 1))
        try:
            self._chk(self.L.nlk_dev_estimate_noise_curve(self.h, d, d + 8 * ch, d_img, w, h, ch, C.byref(p)))
            ab = self.download(d, (ch, 2))
            bins = self.download(d + 8 * ch, (ch, nb), CURVE_BIN)
        finally:
            self.free(d)
        return ab, bins

    def vst_forward(self, d_out, d_in, n, ch, ab, s):
        """d_out[i] = the generalised Anscombe transform of d_in[i] with channel i mod ch's (a, b) and the scale s
        (vst_scale); d_out may be d_in. Not synchronised."""
        a = _ab(ab, ch)
        self._chk(self.L.nlk_dev_vst_forward(self.h, d_out, d_in, n, ch, a.ctypes.data, float(s)))

    def vst_inverse(self, d_out, d_in, n, ch, ab, s, mode=1):
        """The inverse transform: mode 0 algebraic (exact), mode 1 with the closed-form unbiasing terms."""
        a = _ab(ab, ch)
        self._chk(self.L.nlk_dev_vst_inverse(self.h, d_out, d_in, n, ch, a.ctypes.data, float(s), int(mode)))

    # ---- a noise-level function of any shape (include/nlk_hip.h: nlk_nlf_build, nlk_dev_nlf_forward / _inverse)
    def nlf_table(self, d_img, w, h, ch, rho=NLF_RHO, **params):
        """The NlfTable of the device image d_img: the bins of estimate_noise_curve (params: the fields of
        CurveParams) through nlf_build. Waits for the device."""
        p = curve_params(**params)
        return nlf_build(self.estimate_noise_curve(d_img, w, h, ch, **params)[1], p.lo, p.hi, rho)

    def nlf_forward(self, d_out, d_in, n, ch, table):
        """d_out[i] = the table's map of channel i mod ch at d_in[i]; the noise of the result has deviation table.s in
        every channel. d_out may be d_in. Not synchronised (a table the context has not seen is uploaded first)."""
        self._chk(self.L.nlk_dev_nlf_forward(self.h, d_out, d_in, n, ch, C.byref(table)))

    def nlf_inverse(self, d_out, d_in, n, ch, table):
        """The inverse map (algebraic: no unbiasing term)."""
        self._chk(self.L.nlk_dev_nlf_inverse(self.h, d_out, d_in, n, ch, C.byref(table)))

    # ---- defective pixels (include/nlk_hip.h: nlk_dev_despike)
    def despike(self, d_out, d_in, w, h, ch, thr, radius=1, d_count=None):
        """d_out = d_in with every sample that lies more than thr outside the range of its ring (its channel's samples
        at Chebyshev distance `radius`, 1 or 2) replaced by the ring's median, everything else bit for bit (the rule:
        tests/despike_ref.py). d_out must not be d_in. d_count: None, or ch device uint32 that receive the replaced
        samples of every channel. Not synchronised."""
        self._chk(self.L.nlk_dev_despike(self.h, d_out, d_in, d_count, w, h, ch, int(radius), float(thr)))

    def despike_counts(self, d_out, d_in, w, h, ch, thr, radius=1):
        """despike(), and the replaced samples of every channel ([ch] uint32). Waits for the device."""
        d = self.alloc(4 * max(ch, 1))
        try:
            self.despike(d_out, d_in, w, h, ch, thr, radius, d)
            return self.download(d, (ch,), np.uint32)
        finally:
            self.free(d)

    # ---- a defect map learned over time (include/nlk_hip.h: nlk_dev_defect_step, nlk_defect_schedule)
    def defect_step(self, d_out, d_in, d_mean_out, d_mean_in, w, h, ch, thr, gain, radius=1, d_map=None, d_count=None):
        """One frame of the defect map (the rule: tests/defectmap_ref.py): where the mean d_mean_in of the frames before
        lies more than thr outside the range of its ring, d_out = the median of d_in's ring, anything else d_in bit for
        bit; d_mean_out = d_mean_in + (d_in - d_mean_in) * gain. d_mean_in None: the first frame (out = in, the mean
        starts as the frame; thr and gain are not used). d_map: None, or w h ch device bytes, 1 = hit; d_count: None,
        or ch device uint32, the replaced samples of every channel. No two of the four planes may overlap. Not
        synchronised."""
        self._chk(self.L.nlk_dev_defect_step(self.h, d_out, d_in, d_mean_out, d_mean_in, d_map, d_count, w, h, ch,
                                             int(radius), float(thr), float(gain)))

    @staticmethod
    def defect_schedule(t, n_window, k_sigma):
        """nlk_defect_schedule: (thr, gain) of the frame of index t >= 1 (float32 values as Python floats)."""
        thr, gain = C.c_float(), C.c_float()
        if hip().nlk_defect_schedule(int(t), int(n_window), float(k_sigma), C.byref(thr), C.byref(gain)) != 0:
            raise ValueError(f"defect_schedule(t={t}, n_window={n_window}): want t >= 1 and n_window >= 1")
        return thr.value, gain.value

    def noise_affine(self, d_out, d_in, n, ch, ab, seed):
        """d_out[i] = d_in[i] + sqrt(max(a_c d_in[i] + b_c, 0)) N_i with awgn's deviates N_i (d_out may be d_in)."""
        a = _ab(ab, ch)
        self._chk(self.L.nlk_dev_noise_affine(self.h, d_out, d_in, n, ch, a.ctypes.data, int(seed) & 0xFFFFFFFF))

    # ---- planar Y'CbCr frames <-> HWC float RGB (include/nlk_hip.h: nlk_dev_yuv_to_rgb / nlk_dev_rgb_to_yuv)
    def yuv_to_rgb_dev(self, d_rgb, d_yuv, w, h, fmt):
        """d_rgb (h, w, 3 or 1 for mono; float32, 0..255) = the frame d_yuv (device pointers). Not synchronised."""
        self._chk(self.L.nlk_dev_yuv_to_rgb(self.h, d_rgb, d_yuv, w, h, C.byref(fmt)))

    def rgb_to_yuv_dev(self, d_yuv, d_rgb, w, h, fmt):
        """The frame d_yuv (fmt.frame_bytes(w, h) bytes) = the codes of d_rgb (device pointers). Not synchronised."""
        self._chk(self.L.nlk_dev_rgb_to_yuv(self.h, d_yuv, d_rgb, w, h, C.byref(fmt)))

    def yuv_to_rgb(self, buf, w, h, fmt):
        """The (h, w, ch) float32 RGB image (ch = 1 for mono) of one frame's payload. buf: a torch tensor on this
        context's device (any dtype, fmt.frame_bytes(w, h) bytes; a tensor comes back) or a numpy array / bytes
        (uploaded; a numpy array comes back). Waits for the device."""
        ch, nbytes = (1 if fmt.mono else 3), fmt.frame_bytes(w, h)
        if hasattr(buf, "data_ptr"):
            import torch
            if buf.numel() * buf.element_size() != nbytes or not buf.is_contiguous():
                raise ValueError(f"yuv_to_rgb: want a contiguous tensor of {nbytes} bytes")
            out = torch.empty((h, w, ch), dtype=torch.float32, device=buf.device)
            torch.cuda.current_stream(buf.device).synchronize()
            self.yuv_to_rgb_dev(out.data_ptr(), buf.data_ptr(), w, h, fmt)
            self.sync()
            return out
        a = np.frombuffer(buf, np.uint8) if isinstance(buf, (bytes, bytearray)) else np.ascontiguousarray(buf).view(np.uint8).ravel()
        if a.nbytes != nbytes:
            raise ValueError(f"yuv_to_rgb: the payload holds {a.nbytes} bytes, the frame {nbytes}")
        d_yuv, d_rgb = self.upload(a), self.alloc(w * h * ch * 4)
        try:
            self.yuv_to_rgb_dev(d_rgb, d_yuv, w, h, fmt)
            return self.download(d_rgb, (h, w, ch))
        finally:
            self.free(d_yuv)
            self.free(d_rgb)

    def rgb_to_yuv(self, rgb, fmt):
        """One frame's payload (uint8 [fmt.frame_bytes(w, h)]; little-endian uint16 samples above 8 bit) from the
        (h, w, ch) float32 image rgb (ch = 1, or (h, w), for mono): a torch tensor on this context's device gives a
        tensor, a numpy array an array. Waits for the device."""
        ch = 1 if fmt.mono else 3
        if hasattr(rgb, "data_ptr"):
            import torch
            h, w = int(rgb.shape[0]), int(rgb.shape[1])
            if rgb.dtype != torch.float32 or rgb.numel() != w * h * ch or not rgb.is_contiguous():
                raise ValueError(f"rgb_to_yuv: want a contiguous float32 tensor (h, w, {ch})")
            out = torch.empty((fmt.frame_bytes(w, h),), dtype=torch.uint8, device=rgb.device)
            torch.cuda.current_stream(rgb.device).synchronize()
            self.rgb_to_yuv_dev(out.data_ptr(), rgb.data_ptr(), w, h, fmt)
            self.sync()
            return out
        a = _img(rgb)
        h, w = a.shape[:2]
        if a.shape[2] != ch:
            raise ValueError(f"rgb_to_yuv: the image has {a.shape[2]} channels, the format {ch}")
        nbytes = fmt.frame_bytes(w, h)
        d_rgb, d_yuv = self.upload(a), self.alloc(max(nbytes, 1))
        try:
            self.rgb_to_yuv_dev(d_yuv, d_rgb, w, h, fmt)
            return self.download(d_yuv, (nbytes,), np.uint8)
        finally:
            self.free(d_rgb)
            self.free(d_yuv)

    def frame_accumulate(self, d_acc, d_cur, d_prev, d_basic, w, h, ch, sigma, params, oy,
                         ngy, smoother=False):
        self._chk(self.L.nlk_dev_frame_accumulate(self.h, d_acc, d_cur, d_prev, d_basic, w, h,
                                                  ch, float(sigma), C.byref(params), oy, ngy,
                                                  int(smoother)))

    def strip_match(self, d_marks, d_cur, d_prev, d_basic, w, h, ch, sigma, params, oy, ngy,
                    smoother=False):
        """Phase 1 on a strip; returns the marking reach R for mask_commit."""
        r = C.c_int()
        self._chk(self.L.nlk_dev_strip_match(self.h, d_cur, d_prev, d_basic, w, h, ch, float(sigma),
                                             C.byref(params), oy, ngy, int(smoother), d_marks,
                                             C.byref(r)))
        return r.value

    def strip_match_rows(self, d_marks, d_cur, d_prev, d_basic, w, h, ch, sigma, params, oy, ngy, r0, rows,
                         smoother=False):
        """Phase 1 for the strip's target rows [r0, r0 + rows) only (marks / records at their place)."""
        r = C.c_int()
        self._chk(self.L.nlk_dev_strip_match_rows(self.h, d_cur, d_prev, d_basic, w, h, ch, float(sigma),
                                                  C.byref(params), oy, ngy, int(smoother), r0, rows, d_marks,
                                                  C.byref(r)))
        return r.value

    def strip_match_part(self, d_marks, d_cur, d_prev, d_basic, w, h, ch, sigma, params, oy, ngy, r0, rows, lay,
                         smoother=False):
        """strip_match_rows that lays out only the pixel rows lay = (lay0, lay1, v0, v1) (include/nlk_hip.h)."""
        r = C.c_int()
        self._chk(self.L.nlk_dev_strip_match_part(self.h, d_cur, d_prev, d_basic, w, h, ch, float(sigma),
                                                  C.byref(params), oy, ngy, int(smoother), r0, rows,
                                                  int(lay[0]), int(lay[1]), int(lay[2]), int(lay[3]), d_marks, C.byref(r)))
        return r.value

    def mask_commit(self, d_marks, ngx, ngy, reach, d_active):
        self._chk(self.L.nlk_dev_mask_commit(self.h, d_marks, ngx, ngy, reach, d_active))

    def strip_group(self, d_acc, d_active):
        self._chk(self.L.nlk_dev_strip_group(self.h, d_acc, d_active))

    def strip_commit_group(self, d_acc, d_marks, ngx, ngy, reach, gy0, d_active):
        """mask_commit over the whole grid + strip_group of the strip starting at grid row gy0, as one call (the
        replay inside the group kernel's launch where it can: include/nlk_hip.h)."""
        self._chk(self.L.nlk_dev_strip_commit_group(self.h, d_acc, d_marks, ngx, ngy, reach, gy0, d_active))

    def frame_normalize(self, d_out, d_acc, d_cur, w, h, ch, y0, y1):
        self._chk(self.L.nlk_dev_frame_normalize(self.h, d_out, d_acc, d_cur, w, h, ch, y0, y1))

    def read_records(self):
        n, k, g = C.c_int(), C.c_int(), C.c_int()
        self._chk(self.L.nlk_ctx_read_records(self.h, C.byref(n), C.byref(k), C.byref(g),
                                              None, None, None, None, None, None))
        n, k, g = n.value, k.value, g.value
        rec = dict(active=np.zeros(n, np.uint8), nsel=np.zeros(n, np.int32),
                   np0=np.zeros(n, np.int32), nagg=np.zeros(n, np.int32),
                   topk=np.zeros((n, k), np.uint32), gcoords=np.zeros((n, g), np.uint32))
        self._chk(self.L.nlk_ctx_read_records(
            self.h, None, None, None, rec["active"].ctypes.data, rec["nsel"].ctypes.data,
            rec["np0"].ctypes.data, rec["nagg"].ctypes.data, rec["topk"].ctypes.data,
            rec["gcoords"].ctypes.data))
        return rec


class Strips:
    """nlk_strips wrapper (include/nlk_hip.h, csrc/strips.hip): one frame over `world` row strips, driven from C.
    devices = one HIP device index (this process holds rank `rank0` of the world: RCCL between the processes,
    call rccl_init) or `world` of them (every strip in this process, device copies; indices may repeat)."""
    PHASES = ("exchange_prev", "match", "marks", "commit", "group", "exchange_acc", "normalize")

    def __init__(self, devices, rank0, world, w, h, ch, sigma, params, smoother=False, have_prev=True):
        self.L = hip()
        self.h = C.c_void_p()
        self.w, self.hh, self.ch, self.world, self.nlocal = w, h, ch, world, len(devices)
        dev = (C.c_int * len(devices))(*devices)
        rc = self.L.nlk_strips_create(C.byref(self.h), len(devices), dev, rank0, world, w, h, ch, float(sigma),
                                      C.byref(params), int(smoother), int(have_prev))
        if rc:
            raise NlkError(f"rc={rc}: " + self.L.nlk_last_error(None).decode())

    def _chk(self, rc):
        if rc:
            raise NlkError(f"rc={rc}: " + self.L.nlk_strips_last_error(self.h).decode() + " / " + self.L.nlk_last_error(None).decode())

    def close(self):
        if self.h:
            self.L.nlk_strips_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @staticmethod
    def unique_id():
        buf = C.create_string_buffer(128)
        rc = hip().nlk_rccl_unique_id(buf)
        if rc:
            raise NlkError(hip().nlk_last_error(None).decode())
        return bytes(buf.raw)

    def rccl_init(self, id128):
        self._chk(self.L.nlk_strips_rccl_init(self.h, C.c_char_p(id128)))

    def transport(self):
        return self.L.nlk_strips_transport(self.h).decode()

    def load(self, local, d_cur_full, d_prev_full):
        self._chk(self.L.nlk_strips_load(self.h, local, d_cur_full, d_prev_full))

    def set_options(self, overlap=False, timing=False, graph=False):
        self._chk(self.L.nlk_strips_set_options(self.h, int(overlap), int(timing), int(graph)))

    def set_dry_run(self, on=True):
        self._chk(self.L.nlk_strips_set_dry_run(self.h, int(on)))

    def step(self):
        self._chk(self.L.nlk_strips_step(self.h))

    def sync(self):
        self._chk(self.L.nlk_strips_sync(self.h))

    def geometry(self, local=0):
        g = (C.c_int * 6)()
        self._chk(self.L.nlk_strips_geometry(self.h, local, g))
        return dict(zip(("gy0", "gy1", "Y0", "Y1", "own0", "own1"), g))

    def own_rows(self, local=0):
        """(y0, y1, device pointer to the output rows, pointer to the whole-grid decisions)"""
        y0, y1, rows, act = C.c_int(), C.c_int(), C.c_void_p(), C.c_void_p()
        self._chk(self.L.nlk_strips_own_rows(self.h, local, C.byref(y0), C.byref(y1), C.byref(rows), None, C.byref(act)))
        return y0.value, y1.value, rows.value, act.value

    def download_rows(self, local=0):
        y0, y1, rows, _ = self.own_rows(local)
        out = np.empty((y1 - y0, self.w, self.ch), np.float32)
        c = self.L.nlk_strips_ctx(self.h, local)
        rc = self.L.nlk_d2h(c, out.ctypes.data, rows, out.nbytes)
        if rc:
            raise NlkError(self.L.nlk_last_error(c).decode())
        return y0, y1, out

    def stats(self):
        ph, us, g = (C.c_float * 7)(), C.c_float(), C.c_int()
        self._chk(self.L.nlk_strips_stats(self.h, ph, C.byref(us), C.byref(g)))
        return dict(zip(self.PHASES, (round(float(v), 4) for v in ph))), float(us.value), bool(g.value)
