"""ctypes binding of libcaesar_yolo_hip.so (the C-ABI in include/caesar_yolo_hip.h).

There is no CPU fallback: if the shared library is missing, or an entry point fails, an exception is raised.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libcaesar_yolo_hip.so")

CY_MAX_DET = 300
CY_MAX_STAGES = 8
CY_MEAS_FIELDS = 12
MEAS_NAMES = ("npix", "nring", "bkg", "rms", "peak", "x_peak", "y_peak", "sum", "sw", "swx", "swy", "reserved")
CY_ISL_FIELDS = 20
ISL_NAMES = ("status", "nseed", "nislands", "npix", "npix_main", "nborder", "xmin", "xmax", "ymin", "ymax", "S", "Sx", "Sy", "Sxx", "Syy",
             "Sxy", "S_main", "reserved0", "reserved1", "reserved2")
CY_DBL_MAX_COMP, CY_DBL_FIELDS, CY_DBL_COMP_FIELDS = 16, 8, 12
DBL_NAMES = ("status", "nsummits", "npeaks", "ncomp", "npix", "npix_unassigned", "reserved0", "reserved1")
DBL_COMP_NAMES = ("npix", "peak", "x_peak", "y_peak", "S", "Sx", "Sy", "Sxx", "Syy", "Sxy", "main", "nsummits")
CY_FIT_FIELDS = 32
FIT_NAMES = ("status", "niter", "npix", "F", "lambda", "A", "x0", "y0", "a", "b", "c") + tuple(
    "H%d%d" % (i, j) for i in range(6) for j in range(i, 6))
CY_BLEND_FIELDS = 36
CY_BLEND_MAX_MEMBERS = 4
BLEND_NAMES = ("status", "niter", "npix", "F", "lambda", "group", "nmembers", "slot", "A", "x0", "y0", "a", "b", "c", "cov_ok") + tuple(
    "C%d%d" % (i, j) for i in range(6) for j in range(i, 6))
CY_RND_FIELDS, CY_RND_HALF_MAX = 8, 256
RND_NAMES = ("status", "sx0", "sx1", "sy0", "sy1", "ntiles", "reserved0", "reserved1")
CY_RES_FIELDS = 12
RES_NAMES = ("status", "npix_win", "npix_isl", "sum_win", "sumsq_win", "sum_isl", "sumsq_isl", "maxabs_isl", "x_max", "y_max", "model_isl",
             "reserved")
CY_PEAK_FIELDS, CY_PEAK_RADIUS_MAX, CY_PEAK_CAP_MAX = 12, 8, 1 << 20
PEAK_NAMES = ("x", "y", "v", "rms", "snr", "npix", "nabove", "sum", "sw", "swx", "swy", "reserved")
CY_ATROUS_STEP_MAX = 64
CY_APER_RINGS_MAX, CY_APER_RADIUS_MAX, CY_APER_HEAD, CY_APER_RING_FIELDS, CY_APER_JOBS_MAX = 8, 256, 8, 4, 1 << 20
CY_APER_FIELDS = CY_APER_HEAD + CY_APER_RING_FIELDS * CY_APER_RINGS_MAX
APER_NAMES = ("status", "x0", "x1", "y0", "y1", "clipped", "bkg_med", "bkg_mad")
APER_RING_NAMES = ("npix", "sum", "sumsq", "svar")
CY_PFIT_JOB_FIELDS, CY_PFIT_FIELDS, CY_PFIT_RADIUS_MAX, CY_PFIT_NEIGH_MAX, CY_PFIT_JOBS_MAX = 11, 40, 256, 8, 1 << 20
PFIT_JOB_NAMES = ("cx", "cy", "R", "bkg", "sign", "A", "x0", "y0", "a", "b", "c")
PFIT_NAMES = FIT_NAMES + ("wx0", "wx1", "wy0", "wy1", "clipped", "nneigh", "crowded", "nexcluded")
CY_PGRP_FIELDS = 44
PGRP_NAMES = BLEND_NAMES + ("wx0", "wx1", "wy0", "wy1", "clipped", "nexcluded", "nlinked", "reserved")
CY_DRES_FIELDS = 16
DRES_NAMES = ("status", "npix", "nexcluded", "sum", "sumsq", "maxabs", "x_max", "y_max", "model_sum", "reserved", "wx0", "wx1", "wy0", "wy1",
              "clipped", "nneigh")
CY_FORCED_JOB_FIELDS, CY_FORCED_FIELDS, CY_FORCED_NEIGH_MAX, CY_FORCED_JOBS_MAX = 6, 24, 7, 1 << 20
FORCED_JOB_NAMES = ("x0", "y0", "a", "b", "c", "bkg")
FORCED_NAMES = ("status", "npix", "nexcluded", "K", "nneigh", "crowded", "ndup", "amp", "amp_var", "bkg_off", "bkg_var", "cov_amp_bkg", "chi2",
                "syy", "n00", "b0", "corr_max", "wx0", "wx1", "wy0", "wy1", "capped", "reserved0", "reserved1")
CY_BKG_FIELDS = 8
BKG_NAMES = ("n0", "n", "bkg", "rms", "L", "H", "rounds", "reserved")
OP_BKG, OP_SHIFT, OP_CLIP, OP_ZSCALE, OP_HISTEQ, OP_MINMAX = 1, 2, 3, 4, 5, 6
F16, F32, F16X3 = 0, 1, 2
PRECISIONS = {"fp16": F16, "f16": F16, "half": F16, "fp32": F32, "f32": F32, "float": F32, "fp16x3": F16X3, "f16x3": F16X3, "split": F16X3}

EXPORTS = [
    "cy_create", "cy_destroy", "cy_last_error", "cy_load_weights", "cy_load_weights_mem", "cy_num_classes",
    "cy_weight_passes", "cy_class_name", "cy_plan_num_convs", "cy_plan_conv_desc", "cy_letterbox_geometry", "cy_num_anchors",
    "cy_pred_elems", "cy_profile_enable", "cy_profile_summary", "cy_profile_summary_lane", "cy_profile_layers", "cy_profile_layer_variant", "cy_mosaic_prepare", "cy_letterbox_pack", "cy_preproc", "cy_preproc_planes", "cy_preproc_params", "cy_forward", "cy_debug_read_conv",
    "cy_debug_stop_after", "cy_debug_ops_done", "cy_debug_read_tensor", "cy_debug_sparse_box",
    "cy_decode_nms", "cy_debug_stamps", "cy_debug_fastdiv", "cy_debug_reduce", "cy_debug_lds_fill", "cy_debug_cand_counts", "cy_iou_merge", "cy_detect_tiles", "cy_detect_flush", "cy_detect_fence", "cy_compact_records", "cy_compact_records_ctx", "cy_detect_counters", "cy_conv_bn_silu", "cy_conv_slices", "cy_conv_variant_name", "cy_bottleneck64", "cy_dwconv3x3",
    "cy_attention", "cy_maxpool5", "cy_make_tile_records",
    "cy_merge_edge_sources", "cy_augment_geometry", "cy_enable_augment", "cy_letterbox_pack_f32", "cy_augment_pack",
    "cy_decode_nms_augmented", "cy_detect_tiles_augmented", "cy_measure_sources", "cy_measure_kernel_ms",
    "cy_measure_islands", "cy_islands_kernel_ms", "cy_measure_background", "cy_background_kernel_ms", "cy_expand_background",
    "cy_deblend_islands", "cy_deblend_kernel_ms", "cy_fit_components", "cy_fit_kernel_ms", "cy_fit_blends", "cy_blend_kernel_ms",
    "cy_render_gaussians", "cy_render_kernel_ms", "cy_render_signed_gaussians", "cy_measure_residuals", "cy_residual_kernel_ms", "cy_find_peaks", "cy_peaks_kernel_ms",
    "cy_atrous_step", "cy_atrous_kernel_ms", "cy_aperture_sums", "cy_aperture_kernel_ms",
    "cy_fit_peaks", "cy_peakfit_kernel_ms", "cy_fit_peak_groups", "cy_peakgroup_kernel_ms",
    "cy_disc_residuals", "cy_disc_residual_kernel_ms", "cy_forced_fit", "cy_forced_kernel_ms",
]


class CyError(RuntimeError):
    pass


class cy_config(C.Structure):
    _fields_ = [("precision", C.c_int), ("max_batch", C.c_int), ("max_h", C.c_int), ("max_w", C.c_int),
                ("max_cand", C.c_int)]


class cy_pre_stage(C.Structure):
    _fields_ = [("op", C.c_int), ("p0", C.c_double), ("p1", C.c_double), ("p2", C.c_double), ("flag", C.c_int)]


class cy_pre_program(C.Structure):
    _fields_ = [("n", C.c_int), ("st", cy_pre_stage * CY_MAX_STAGES)]


class cy_preproc_cfg(C.Structure):
    _fields_ = [("nprog", C.c_int), ("prog", cy_pre_program * 3)]


class cy_conv_desc(C.Structure):
    _fields_ = [("name", C.c_char * 48), ("cin", C.c_int), ("cout", C.c_int), ("k", C.c_int), ("s", C.c_int),
                ("act", C.c_int)]


class cy_conv_layout(C.Structure):
    _fields_ = [("d_in0", C.c_void_p), ("in0_ct", C.c_int), ("in0_coff", C.c_int), ("c0", C.c_int), ("up0", C.c_int),
                ("d_in1", C.c_void_p), ("in1_ct", C.c_int), ("in1_coff", C.c_int), ("c1", C.c_int),
                ("d_res", C.c_void_p), ("res_ct", C.c_int), ("res_coff", C.c_int),
                ("d_out", C.c_void_p), ("out_ct", C.c_int), ("out_coff", C.c_int),
                ("rows", C.c_int), ("out_bs", C.c_int), ("out_ro", C.c_int),
                ("B", C.c_int), ("Hi", C.c_int), ("Wi", C.c_int), ("Cin", C.c_int), ("Cout", C.c_int), ("k", C.c_int), ("s", C.c_int),
                ("act", C.c_int)]


class cy_prof_entry(C.Structure):
    _fields_ = [("kernel", C.c_char * 64), ("ms", C.c_double), ("flops", C.c_double), ("launches", C.c_long)]


class cy_letterbox(C.Structure):
    _fields_ = [("new_h", C.c_int), ("new_w", C.c_int), ("top", C.c_int), ("left", C.c_int), ("H", C.c_int),
                ("W", C.c_int)]


class cy_augment_view(C.Structure):
    _fields_ = [("scale", C.c_double), ("flip", C.c_int), ("ch", C.c_int), ("cw", C.c_int), ("Hp", C.c_int), ("Wp", C.c_int),
                ("A", C.c_int), ("lo", C.c_int), ("hi", C.c_int), ("off", C.c_int)]


class cy_augment_geom(C.Structure):
    _fields_ = [("v", cy_augment_view * 3), ("total", C.c_int)]


_lib = None


def load():
    """Load the shared library (once).  Raises CyError if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    # PyTorch (device memory / streams for this package) bundles its own HIP runtime.  It must be the one already mapped
    # when libcaesar_yolo_hip.so resolves libamdhip64: two HIP runtimes in one process do not both see the GPU.
    import torch  # noqa: F401
    if not os.path.exists(LIB_PATH):
        raise CyError("%s not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                      "(there is no CPU fallback)" % LIB_PATH)
    lib = C.CDLL(LIB_PATH)
    vp, ip, fp, dp = C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_float), C.POINTER(C.c_double)
    sig = {
        "cy_create": (C.c_int, [C.c_int, C.POINTER(cy_config), C.POINTER(vp)]),
        "cy_destroy": (C.c_int, [vp]),
        "cy_last_error": (C.c_char_p, [vp]),
        "cy_load_weights": (C.c_int, [vp, C.c_char_p]),
        "cy_load_weights_mem": (C.c_int, [vp, vp, C.c_size_t]),
        "cy_num_classes": (C.c_int, [vp]),
        "cy_weight_passes": (C.c_int, [vp, ip]),
        "cy_class_name": (C.c_char_p, [vp, C.c_int]),
        "cy_plan_num_convs": (C.c_int, [C.c_char, C.c_int]),
        "cy_plan_conv_desc": (C.c_int, [C.c_char, C.c_int, C.c_int, C.POINTER(cy_conv_desc)]),
        "cy_letterbox_geometry": (C.c_int, [C.c_int, C.c_int, C.c_int, C.POINTER(cy_letterbox)]),
        "cy_num_anchors": (C.c_int, [C.c_int, C.c_int]),
        "cy_pred_elems": (C.c_size_t, [vp, C.c_int, C.c_int, C.c_int]),
        "cy_mosaic_prepare": (C.c_int, [vp, vp, C.c_size_t, C.c_int, vp]),
        "cy_preproc": (C.c_int, [vp, vp, C.c_int, C.c_int, ip, C.c_int, C.c_int, C.c_int, C.c_int,
                                 C.POINTER(cy_preproc_cfg), vp, vp, vp]),
        "cy_preproc_planes": (C.c_int, [vp, vp, C.c_int, C.c_int, ip, C.c_int, C.c_int, C.c_int, C.POINTER(cy_preproc_cfg), vp, vp, vp]),
        "cy_preproc_params": (C.c_int, [vp, dp, C.c_int]),
        "cy_letterbox_pack": (C.c_int, [vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp]),
        "cy_forward": (C.c_int, [vp, vp, C.c_int, C.c_int, C.c_int, vp, vp]),
        "cy_profile_enable": (C.c_int, [vp, C.c_int]),
        "cy_profile_summary": (C.c_int, [vp, C.POINTER(cy_prof_entry), C.c_int]),
        "cy_profile_summary_lane": (C.c_int, [vp, C.POINTER(cy_prof_entry), C.c_int, C.c_int]),
        "cy_profile_layers": (C.c_int, [vp, C.POINTER(cy_prof_entry), C.c_int]),
        "cy_profile_layer_variant": (C.c_int, [vp, C.c_char_p, C.c_char_p, C.c_int]),
        "cy_debug_read_conv": (C.c_int, [vp, C.c_char_p, fp, C.c_size_t, ip]),
        "cy_debug_stop_after": (C.c_int, [vp, C.c_int]),
        "cy_debug_ops_done": (C.c_int, [vp]),
        "cy_debug_sparse_box": (C.c_int, [vp, vp, C.c_int, C.c_int, C.c_int, vp, C.c_float, ip, vp]),
        "cy_debug_read_tensor": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, fp, C.c_size_t, ip]),
        "cy_decode_nms": (C.c_int, [vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float,
                                    vp, vp, vp, vp]),
        "cy_debug_cand_counts": (C.c_int, [vp, ip, C.c_int]),
        "cy_debug_lds_fill": (C.c_int, [vp, C.c_uint, vp]),
        "cy_debug_stamps": (C.c_int, [C.POINTER(C.c_ulonglong), C.c_int]),
        "cy_debug_fastdiv": (C.c_int, [vp, vp, vp, vp, C.c_int]),
        "cy_debug_reduce": (C.c_int, [vp, vp, C.c_int, C.c_int, vp]),
        "cy_iou_merge": (C.c_int, [vp, vp, vp, C.c_int, C.c_float, C.c_double, C.c_double, vp, vp, vp, vp]),
        "cy_detect_tiles": (C.c_int, [vp, vp, C.c_int, C.c_int, ip, C.c_int, C.c_int, C.c_int, C.c_int,
                                      C.POINTER(cy_preproc_cfg), C.c_float, C.c_float, C.c_double, C.c_double,
                                      vp, vp, vp, vp]),
        "cy_detect_flush": (C.c_int, [vp, vp]),
        "cy_detect_fence": (C.c_int, [vp, vp]),
        "cy_compact_records": (C.c_int, [vp, C.c_longlong, vp, C.c_int, C.c_int, vp, vp, vp]),
        "cy_compact_records_ctx": (C.c_int, [vp, vp, C.c_longlong, vp, C.c_int, C.c_int, vp, vp, vp]),
        "cy_detect_counters": (C.c_int, [vp, C.POINTER(C.c_longlong), C.c_int]),
        "cy_conv_bn_silu": (C.c_int, [vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, fp, fp, C.c_int, C.c_int, C.c_int,
                                      C.c_int, vp, vp, vp]),
        "cy_conv_slices": (C.c_int, [vp, C.POINTER(cy_conv_layout), fp, fp, C.c_char_p, C.c_int, ip, vp]),
        "cy_conv_variant_name": (C.c_char_p, [C.c_int]),
        "cy_bottleneck64": (C.c_int, [vp, vp, C.c_int, C.c_int, C.c_int, fp, fp, fp, fp, C.c_int, vp, vp]),
        "cy_dwconv3x3": (C.c_int, [vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, fp, fp, C.c_int, C.c_int, C.c_int,
                                   C.c_int, vp, C.c_int, C.c_int, vp, C.c_int, C.c_int, vp]),
        "cy_attention": (C.c_int, [vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp, C.c_int, C.c_int, vp]),
        "cy_maxpool5": (C.c_int, [vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp, C.c_int, vp]),
        "cy_make_tile_records": (C.c_int, [fp, ip, C.c_int, ip, C.c_int, dp]),
        "cy_merge_edge_sources": (C.c_int, [dp, C.c_int, ip, C.c_int, dp]),
        "cy_augment_geometry": (C.c_int, [C.c_int, C.c_int, C.POINTER(cy_augment_geom)]),
        "cy_enable_augment": (C.c_int, [vp]),
        "cy_letterbox_pack_f32": (C.c_int, [vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp]),
        "cy_augment_pack": (C.c_int, [vp, vp, C.c_int, C.c_int, C.c_int, vp, vp, vp, vp]),
        "cy_decode_nms_augmented": (C.c_int, [vp, vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float,
                                              vp, vp, vp, vp]),
        "cy_detect_tiles_augmented": (C.c_int, [vp, vp, C.c_int, C.c_int, ip, C.c_int, C.c_int, C.c_int, C.c_int,
                                                C.POINTER(cy_preproc_cfg), C.c_float, C.c_float, C.c_double, C.c_double, C.c_int,
                                                vp, vp, vp, vp]),
        "cy_measure_sources": (C.c_int, [vp, vp, C.c_int, C.c_int, dp, C.c_int, C.c_int, dp, vp]),
        "cy_measure_kernel_ms": (C.c_int, [vp, dp]),
        "cy_measure_islands": (C.c_int, [vp, vp, C.c_int, C.c_int, dp, dp, C.c_int, C.c_int, dp, vp, C.POINTER(C.c_longlong), vp]),
        "cy_islands_kernel_ms": (C.c_int, [vp, dp]),
        "cy_deblend_islands": (C.c_int, [vp, vp, C.c_int, C.c_int, dp, dp, C.c_int, C.c_int, C.c_int, dp, dp, vp, C.POINTER(C.c_longlong), vp]),
        "cy_deblend_kernel_ms": (C.c_int, [vp, dp]),
        "cy_fit_components": (C.c_int, [vp, vp, C.c_int, C.c_int, dp, dp, ip, dp, C.c_int, C.c_int, vp, C.POINTER(C.c_longlong), dp, vp]),
        "cy_fit_kernel_ms": (C.c_int, [vp, dp]),
        "cy_fit_blends": (C.c_int, [vp, vp, C.c_int, C.c_int, dp, dp, ip, dp, C.c_int, C.c_int, vp, C.POINTER(C.c_longlong), dp, vp]),
        "cy_blend_kernel_ms": (C.c_int, [vp, dp]),
        "cy_render_gaussians": (C.c_int, [vp, vp, C.c_int, C.c_int, dp, C.c_int, C.c_double, vp, vp, vp, dp, vp]),
        "cy_render_kernel_ms": (C.c_int, [vp, dp]),
        "cy_render_signed_gaussians": (C.c_int, [vp, vp, C.c_int, C.c_int, dp, C.c_int, C.c_double, vp, vp, vp, dp, vp]),
        "cy_measure_residuals": (C.c_int, [vp, vp, vp, C.c_int, C.c_int, dp, dp, C.c_int, vp, C.POINTER(C.c_longlong), dp, vp]),
        "cy_residual_kernel_ms": (C.c_int, [vp, dp]),
        "cy_find_peaks": (C.c_int, [vp, vp, vp, C.c_int, C.c_int, C.c_double, C.c_int, C.c_int, C.c_int, dp, C.POINTER(C.c_longlong), vp]),
        "cy_peaks_kernel_ms": (C.c_int, [vp, dp]),
        "cy_atrous_step": (C.c_int, [vp, vp, C.c_int, C.c_int, C.c_int, vp, vp, vp]),
        "cy_atrous_kernel_ms": (C.c_int, [vp, dp]),
        "cy_aperture_sums": (C.c_int, [vp, vp, vp, C.c_int, C.c_int, dp, C.c_int, dp, C.c_int, dp, vp]),
        "cy_aperture_kernel_ms": (C.c_int, [vp, dp]),
        "cy_fit_peaks": (C.c_int, [vp, vp, C.c_int, C.c_int, dp, C.c_int, C.c_int, dp, vp]),
        "cy_peakfit_kernel_ms": (C.c_int, [vp, dp]),
        "cy_fit_peak_groups": (C.c_int, [vp, vp, C.c_int, C.c_int, dp, C.c_int, C.c_double, C.c_int, dp, vp]),
        "cy_peakgroup_kernel_ms": (C.c_int, [vp, dp]),
        "cy_disc_residuals": (C.c_int, [vp, vp, vp, C.c_int, C.c_int, dp, C.c_int, dp, vp]),
        "cy_disc_residual_kernel_ms": (C.c_int, [vp, dp]),
        "cy_forced_fit": (C.c_int, [vp, vp, vp, C.c_int, C.c_int, dp, C.c_int, C.c_double, C.c_int, dp, vp]),
        "cy_forced_kernel_ms": (C.c_int, [vp, dp]),
        "cy_measure_background": (C.c_int, [vp, vp, C.c_int, C.c_int, C.c_int, C.c_double, C.c_int, dp, vp]),
        "cy_background_kernel_ms": (C.c_int, [vp, dp]),
        "cy_expand_background": (C.c_int, [vp, dp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, vp]),
    }
    for name, (res, args) in sig.items():
        f = getattr(lib, name)          # AttributeError here = header/library mismatch
        f.restype, f.argtypes = res, args
    _lib = lib
    return lib


def check(rc, ctx=None):
    if rc < 0:
        msg = load().cy_last_error(ctx)
        raise CyError("libcaesar_yolo_hip: %s (status %d)" % (msg.decode() if msg else "error", rc))
    return rc


def letterbox(h0, w0, imgsz):
    lb = cy_letterbox()
    check(load().cy_letterbox_geometry(h0, w0, imgsz, C.byref(lb)))
    return lb


def plan_convs(scale, nc):
    lib = load()
    n = check(lib.cy_plan_num_convs(scale.encode(), nc))
    out = []
    for i in range(n):
        d = cy_conv_desc()
        check(lib.cy_plan_conv_desc(scale.encode(), nc, i, C.byref(d)))
        out.append((d.name.decode(), d.cin, d.cout, d.k, d.s, d.act))
    return out


def augment_geometry(H, W):
    """Test-time augmentation views of an H x W letterboxed input (cy_augment_geometry): list of three dicts
    (scale, flip, ch, cw, Hp, Wp, A, lo, hi, off) and the concatenated anchor count."""
    g = cy_augment_geom()
    check(load().cy_augment_geometry(int(H), int(W), C.byref(g)))
    views = [{k: getattr(g.v[i], k) for k, _ in cy_augment_view._fields_} for i in range(3)]
    return views, int(g.total)
