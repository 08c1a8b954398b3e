"""ctypes binding of libbsx.so and the Python mirror of the reference interface.

Reference interface mirrored here (same names / argument meaning / error behaviour):
  lib/libbackscrub.h:13   bs_tensorflow_version()
  lib/libbackscrub.h:16   bs_maskgen_new(modelname, threads, width, height, ondebug, onprep, oninfer, onmask, caller_ctx)
  lib/libbackscrub.h:36   bs_maskgen_delete(context)
  lib/libbackscrub.h:39   bs_maskgen_process(context, frame, mask) -> bool
  app/deepseg.cc:108      alpha_blend(srca, srcb, mask)

PyTorch is used only as the owner of device memory and streams.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None

_u8p = C.POINTER(C.c_uint8)
DEBUG_FN = C.CFUNCTYPE(None, C.c_void_p, C.c_char_p)
STAGE_FN = C.CFUNCTYPE(None, C.c_void_p)


BSX_STREAM_FILTER_OFF = 32          # bsx.h: bits of bsx_stream_setting.flags next to the flip bits and the blur size
BSX_STREAM_YUYV_IN = 64             # ... in an item of step_geoms / step_vcam_geoms only: that item's frame is YUYV 4:2:2
BSX_MAX_OUT_SIZES = 4               # bsx.h: distinct output sizes of one bsx_step_batch_vcam_geoms_outs call
BSX_MAX_OUTS_PER_ITEM = 4           # ... and output records that may name one item
BSX_GEOMS_EDGE_ROI = 1              # bsx.h: creation flag of bsx_new_geoms_ex (MaskGen.with_geometries(edge_roi=True))


class BsxError(RuntimeError):
    pass


class BsxFrameFormatError(BsxError, ValueError):
    """a frame tensor of step_geoms / step_vcam_geoms whose shape is not that of its item's class and pixel format ([H,W,3] BGR, [H,W,2] with yuyv_in)"""


class _Info(C.Structure):
    _fields_ = [("model_type", C.c_int), ("width", C.c_int), ("height", C.c_int), ("n_streams", C.c_int),
                ("in_w", C.c_int), ("in_h", C.c_int), ("in_c", C.c_int), ("out_w", C.c_int), ("out_h", C.c_int),
                ("out_c", C.c_int), ("roi", C.c_int * 4), ("in_roi", C.c_int * 4), ("n_ops", C.c_int), ("n_steps", C.c_int),
                ("device", C.c_int), ("norm_scale", C.c_float), ("norm_offset", C.c_float), ("nn_flops_per_frame", C.c_double),
                ("act_bytes_per_stream", C.c_size_t)]


class _StreamSetting(C.Structure):          # bsx.h bsx_stream_setting
    _fields_ = [("d_bg", C.c_void_p), ("flags", C.c_uint)]


class _ResizeItem(C.Structure):             # bsx.h bsx_resize_item
    _fields_ = [("d_src", C.c_void_p), ("sw", C.c_int), ("sh", C.c_int), ("d_dst", C.c_void_p)]


class _BlurItem(C.Structure):               # bsx.h bsx_blur_item
    _fields_ = [("d_src", C.c_void_p), ("d_dst", C.c_void_p), ("w", C.c_int), ("h", C.c_int), ("ksize", C.c_int), ("flags", C.c_uint)]


class _BlurSurfaceItem(C.Structure):        # bsx.h bsx_blur_surface_item
    _fields_ = [("d_y", C.c_void_p), ("d_uv", C.c_void_p), ("d_dst", C.c_void_p), ("pitch_y", C.c_int), ("pitch_uv", C.c_int), ("w", C.c_int), ("h", C.c_int),
                ("ksize", C.c_int), ("flags", C.c_uint)]


class _ResizeSurfaceItem(C.Structure):      # bsx.h bsx_resize_surface_item
    _fields_ = [("d_y", C.c_void_p), ("d_uv", C.c_void_p), ("d_dst", C.c_void_p), ("pitch_y", C.c_int), ("pitch_uv", C.c_int), ("sw", C.c_int), ("sh", C.c_int),
                ("dw", C.c_int), ("dh", C.c_int), ("flags", C.c_uint), ("reserved", C.c_int)]


class _Geometry(C.Structure):               # bsx.h bsx_geometry
    _fields_ = [("width", C.c_int), ("height", C.c_int), ("n_streams", C.c_int)]


class _GeomInfo(C.Structure):               # bsx.h bsx_geom_info
    _fields_ = [("width", C.c_int), ("height", C.c_int), ("n_streams", C.c_int), ("first_stream", C.c_int), ("roi", C.c_int * 4), ("in_roi", C.c_int * 4),
                ("mask_offset", C.c_size_t)]


class _GeomItem(C.Structure):               # bsx.h bsx_geom_item
    _fields_ = [("d_frame", C.c_void_p), ("d_out", C.c_void_p), ("setting", _StreamSetting)]


class _VcamOut(C.Structure):                # bsx.h bsx_vcam_out
    _fields_ = [("item", C.c_int), ("out_w", C.c_int), ("out_h", C.c_int), ("d_out", C.c_void_p)]


class _VcamOutNv12(C.Structure):            # bsx.h bsx_vcam_out_nv12
    _fields_ = [("item", C.c_int), ("out_w", C.c_int), ("out_h", C.c_int), ("pitch_y", C.c_int), ("pitch_uv", C.c_int), ("d_y", C.c_void_p), ("d_uv", C.c_void_p)]


class _SurfaceItem(C.Structure):            # bsx.h bsx_surface_item
    _fields_ = [("d_y", C.c_void_p), ("d_uv", C.c_void_p), ("pitch_y", C.c_int), ("pitch_uv", C.c_int), ("setting", _StreamSetting)]


class StreamSetting:
    """one stream's settings for MaskGen.step_mixed — what one reference process takes as -b <image> (bg), -H / -V (flip_h / flip_v), -p bgblur:<k> (bgblur)
    and toggles at run time with the s / h / v keys (filter_off, flip_h, flip_v; app/deepseg.cc:387-437, 624-673, 777-790).  bg: a cuda uint8 [H,W,3] image
    (any number of streams may share one); unused with bgblur or filter_off.  yuyv_in (step_geoms / step_vcam_geoms only, where every item brings its own frame):
    this item's frame is the camera's raw YUYV 4:2:2 [H,W,2] (BSX_STREAM_YUYV_IN); the mixed steps take the format batch-wide and refuse it."""
    __slots__ = ("bg", "flip_h", "flip_v", "bgblur", "filter_off", "yuyv_in")

    def __init__(self, bg=None, flip_h=False, flip_v=False, bgblur=0, filter_off=False, yuyv_in=False):
        self.bg, self.flip_h, self.flip_v, self.bgblur, self.filter_off = bg, bool(flip_h), bool(flip_v), int(bgblur), bool(filter_off)
        self.yuyv_in = bool(yuyv_in)

    def flags(self):
        return ((2 if self.flip_h else 0) | (4 if self.flip_v else 0) | ((self.bgblur & 255) << 8) | (BSX_STREAM_FILTER_OFF if self.filter_off else 0) |
                (BSX_STREAM_YUYV_IN if self.yuyv_in else 0))

    def __repr__(self):
        return "StreamSetting(bg=%s, flip_h=%s, flip_v=%s, bgblur=%d, filter_off=%s%s)" % (
            "None" if self.bg is None else "<image>", self.flip_h, self.flip_v, self.bgblur, self.filter_off, ", yuyv_in=True" if self.yuyv_in else "")


class LaunchStat(C.Structure):
    _fields_ = [("name", C.c_char * 64), ("avg_ms", C.c_double), ("bytes", C.c_double), ("flops", C.c_double)]


# every symbol include/bsx.h declares: (name, restype, argtypes)
SYMBOLS = [
    ("bsx_version", C.c_char_p, []),
    ("bsx_device_count", C.c_int, []),
    ("bsx_new", C.c_void_p, [C.c_char_p, C.c_size_t, C.c_size_t, C.c_size_t, C.c_int, C.c_int, DEBUG_FN, STAGE_FN, STAGE_FN, STAGE_FN, C.c_void_p]),
    ("bsx_delete", None, [C.c_void_p]),
    ("bsx_get_info", C.c_int, [C.c_void_p, C.POINTER(_Info)]),
    ("bsx_last_error", C.c_char_p, [C.c_void_p]),
    ("bsx_reset", C.c_int, [C.c_void_p, C.c_void_p]),
    ("bsx_process_host", C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t]),
    ("bsx_process_batch", C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    ("bsx_masks_device", C.c_void_p, [C.c_void_p]),
    ("bsx_composite_batch", C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    ("bsx_step_batch", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_int, C.c_void_p]),
    ("bsx_step_batch_yuyv", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_int, C.c_void_p]),
    ("bsx_step_batch_ex", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_int, C.c_void_p, C.c_uint]),
    ("bsx_step_batch_pipelined", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_int, C.c_void_p, C.c_uint]),
    ("bsx_step_batch_vcam", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_uint]),
    ("bsx_step_batch_streams", C.c_int, [C.c_void_p, C.POINTER(C.c_int), C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_int, C.c_void_p, C.c_uint]),
    ("bsx_reset_streams", C.c_int, [C.c_void_p, C.POINTER(C.c_int), C.c_int, C.c_void_p]),
    ("bsx_new_geoms", C.c_void_p, [C.c_char_p, C.c_size_t, C.POINTER(_Geometry), C.c_int, C.c_int, DEBUG_FN, STAGE_FN, STAGE_FN, STAGE_FN, C.c_void_p]),
    ("bsx_new_geoms_ex", C.c_void_p, [C.c_char_p, C.c_size_t, C.POINTER(_Geometry), C.c_int, C.c_int, C.c_uint, DEBUG_FN, STAGE_FN, STAGE_FN, STAGE_FN, C.c_void_p]),
    ("bsx_geom_count", C.c_int, [C.c_void_p]),
    ("bsx_get_geom_info", C.c_int, [C.c_void_p, C.c_int, C.POINTER(_GeomInfo)]),
    ("bsx_step_batch_geoms", C.c_int, [C.c_void_p, C.POINTER(C.c_int), C.POINTER(_GeomItem), C.c_int, C.c_void_p, C.c_uint]),
    ("bsx_step_batch_vcam_geoms", C.c_int, [C.c_void_p, C.POINTER(C.c_int), C.POINTER(_GeomItem), C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_uint]),
    ("bsx_step_batch_vcam_geoms_outs", C.c_int, [C.c_void_p, C.POINTER(C.c_int), C.POINTER(_GeomItem), C.c_int, C.POINTER(_VcamOut), C.c_int, C.c_void_p, C.c_uint]),
    ("bsx_step_batch_vcam_geoms_outs_nv12", C.c_int, [C.c_void_p, C.POINTER(C.c_int), C.POINTER(_GeomItem), C.c_int, C.POINTER(_VcamOutNv12), C.c_int, C.c_void_p,
                                                      C.c_uint]),
    ("bsx_step_batch_surfaces", C.c_int, [C.c_void_p, C.POINTER(C.c_int), C.POINTER(_SurfaceItem), C.c_int, C.POINTER(_VcamOutNv12), C.c_int, C.c_void_p, C.c_uint]),
    ("bsx_step_batch_mixed", C.c_int, [C.c_void_p, C.POINTER(C.c_int), C.c_void_p, C.POINTER(_StreamSetting), C.c_void_p, C.c_int, C.c_void_p, C.c_uint]),
    ("bsx_step_batch_vcam_mixed", C.c_int, [C.c_void_p, C.POINTER(C.c_int), C.c_void_p, C.POINTER(_StreamSetting), C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                            C.c_uint]),
    ("bsx_resize_bgr", C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    ("bsx_resize_bgr_batch", C.c_int, [C.c_void_p, C.POINTER(_ResizeItem), C.c_int, C.c_int, C.c_int, C.c_void_p]),
    ("bsx_bgr_to_yuyv", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    ("bsx_bgr_to_nv12", C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p]),
    ("bsx_nv12_to_bgr", C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    ("bsx_yuyv_to_bgr", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    ("bsx_background_load", C.c_void_p, [C.c_void_p, C.c_char_p, C.c_int]),
    ("bsx_background_from_frames", C.c_void_p, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_double, C.c_int]),
    ("bsx_background_free", None, [C.c_void_p]),
    ("bsx_background_info", C.c_int, [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_double), C.POINTER(C.c_int)]),
    ("bsx_background_grab", C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    ("bsx_background_grab_batch", C.c_int, [C.POINTER(C.c_void_p), C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.c_double, C.POINTER(C.c_int), C.c_void_p]),
    ("bsx_media_decode", C.c_int, [C.c_char_p, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_double), C.POINTER(C.POINTER(C.c_uint8)), C.c_char_p, C.c_size_t]),
    ("bsx_media_free", None, [C.POINTER(C.c_uint8)]),
    ("bsx_live_new", C.c_void_p, [C.c_void_p]),
    ("bsx_live_delete", None, [C.c_void_p]),
    ("bsx_live_set_input_frame", C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t]),
    ("bsx_live_get_output_mask", C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t]),
    ("bsx_live_timings", C.c_int, [C.c_void_p, C.POINTER(C.c_long), C.POINTER(C.c_long)]),
    ("bsx_gaussian_blur_bgr", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    ("bsx_gaussian_blur_bgr_batch", C.c_int, [C.c_void_p, C.POINTER(_BlurItem), C.c_int, C.c_void_p]),
    ("bsx_gaussian_blur_surfaces_batch", C.c_int, [C.c_void_p, C.POINTER(_BlurSurfaceItem), C.c_int, C.c_void_p]),
    ("bsx_resize_surfaces_batch", C.c_int, [C.c_void_p, C.POINTER(_ResizeSurfaceItem), C.c_int, C.c_void_p]),
    ("bsx_debug_gauss_coeffs", C.c_int, [C.c_int, C.c_int, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    ("bsx_flip_bgr", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    ("bsx_debug_buffer", C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]),
    ("bsx_debug_run_stage", C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p]),
    ("bsx_plan_describe", C.c_char_p, [C.c_void_p]),
    ("bsx_debug_tensor", C.c_long, [C.c_void_p, C.c_int, C.POINTER(C.c_float), C.c_long]),
    ("bsx_model_precompile", C.c_int, [C.c_char_p, C.c_char_p, C.c_char_p, C.c_size_t]),
    ("bsx_model_kernel_source", C.c_long, [C.c_char_p, C.c_char_p, C.c_size_t]),
    ("bsx_model_seg_source", C.c_long, [C.c_char_p, C.c_char_p, C.c_size_t]),
    ("bsx_debug_tensor_of", C.c_long, [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_float), C.c_long]),
    ("bsx_debug_mask_tile_stats", C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_long)]),
    ("bsx_debug_program_timeline", C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_ulonglong), C.c_int, C.c_void_p]),
    ("bsx_model_describe", C.c_int, [C.c_char_p, C.c_char_p, C.c_size_t]),
    ("bsx_profile_batch", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_int, C.c_int, C.POINTER(LaunchStat), C.c_int, C.c_void_p]),
]


def lib_path() -> str:
    return os.environ.get("BSX_LIBRARY") or os.path.join(_HERE, "libbsx.so")   # BSX_LIBRARY: A/B another build of the same ABI


def lib():
    """Load libbsx.so.  Fails loudly (no fallback) when it has not been built."""
    global _LIB
    if _LIB is None:
        # torch bundles its own HIP runtime under the same SONAME as /opt/rocm's; importing it first makes the
        # whole process (torch allocations + our launches) use ONE runtime instance.
        import torch  # noqa: F401
        p = lib_path()
        if not os.path.exists(p):
            raise BsxError("libbsx.so is missing (%s): run `python -m backscrub_amd.build` — there is no CPU fallback" % p)
        L = C.CDLL(p)
        for name, res, args in SYMBOLS:
            f = getattr(L, name)  # AttributeError if the library does not export it
            f.restype = res
            f.argtypes = args
        _LIB = L
    return _LIB


def _ids(ids):
    """stream ids (any sequence of ints, a numpy array or a CPU tensor) → (ctypes int array, n); the C side validates range and uniqueness"""
    v = [int(i) for i in (ids.tolist() if hasattr(ids, "tolist") else ids)]
    return (C.c_int * max(len(v), 1))(*v), len(v)


def _check(rc, ctx=None, what=""):
    if rc != 0:
        msg = lib().bsx_last_error(ctx) or b""
        raise BsxError("%s failed (%d): %s" % (what, rc, msg.decode(errors="replace").strip()))


def _torch():
    import torch
    return torch


def _ptr(t):
    """a tensor's device address for the C ABI (None: NULL)"""
    return C.c_void_p(t.data_ptr() if t is not None else None)


def _stream_ptr():
    torch = _torch()
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


class MaskGen:
    """Batched mask generator: n_streams independent camera streams on one GPU."""

    def __init__(self, model_path, width, height, n_streams=1, device=0, threads=2, ondebug=None, onprep=None, oninfer=None,
                 onmask=None, caller_ctx=None):
        L = lib()
        self._cbs = (DEBUG_FN(ondebug) if ondebug else DEBUG_FN(), STAGE_FN(onprep) if onprep else STAGE_FN(),
                     STAGE_FN(oninfer) if oninfer else STAGE_FN(), STAGE_FN(onmask) if onmask else STAGE_FN())
        self.h = L.bsx_new(os.fsencode(model_path), threads, width, height, n_streams, device, *self._cbs, caller_ctx)
        if not self.h:
            raise BsxError("bsx_new failed: %s" % (L.bsx_last_error(None) or b"").decode(errors="replace").strip())
        info = _Info()
        _check(L.bsx_get_info(self.h, C.byref(info)), self.h, "bsx_get_info")
        self.info = {k: (list(getattr(info, k)) if k in ("roi", "in_roi") else getattr(info, k)) for k, _ in _Info._fields_}
        self.width, self.height, self.n_streams, self.device = width, height, n_streams, device

    @classmethod
    def with_geometries(cls, model_path, geometries, device=0, threads=2, ondebug=None, onprep=None, oninfer=None, onmask=None, caller_ctx=None, edge_roi=False):
        """a context for cameras of several capture sizes (bsx_new_geoms): geometries = [(width, height, n_streams), ...], at most 8 distinct sizes.  Streams are
        numbered class after class; step_geoms advances any mix of them in one launch sequence.  width / height / info are class 0's, n_streams the total.
        edge_roi=True (bsx_new_geoms_ex with BSX_GEOMS_EDGE_ROI): sizes whose ROI is off the 4-pixel grid are taken too (segm_lite at 1920x1080); every width
        must still be a multiple of 4."""
        geometries = [tuple(int(v) for v in g) for g in geometries]
        if not geometries or any(len(g) != 3 for g in geometries):
            raise BsxError("geometries must be a non-empty list of (width, height, n_streams)")
        if not isinstance(edge_roi, (bool, np.bool_)):
            raise BsxError("edge_roi must be True or False, not %r" % (edge_roi,))
        if edge_roi:
            for g, (w, _h, _n) in enumerate(geometries):
                if w % 4:
                    raise BsxError("geometries[%d]: width %d is not a multiple of 4 (edge_roi frees the ROI's column and width, not the frame's)" % (g, w))
        L = lib()
        self = cls.__new__(cls)
        self._cbs = (DEBUG_FN(ondebug) if ondebug else DEBUG_FN(), STAGE_FN(onprep) if onprep else STAGE_FN(),
                     STAGE_FN(oninfer) if oninfer else STAGE_FN(), STAGE_FN(onmask) if onmask else STAGE_FN())
        arr = (_Geometry * len(geometries))(*[_Geometry(*g) for g in geometries])
        if edge_roi:
            self.h = L.bsx_new_geoms_ex(os.fsencode(model_path), threads, arr, len(geometries), device, BSX_GEOMS_EDGE_ROI, *self._cbs, caller_ctx)
        else:
            self.h = L.bsx_new_geoms(os.fsencode(model_path), threads, arr, len(geometries), device, *self._cbs, caller_ctx)
        if not self.h:
            raise BsxError("%s failed: %s" % ("bsx_new_geoms_ex" if edge_roi else "bsx_new_geoms", (L.bsx_last_error(None) or b"").decode(errors="replace").strip()))
        info = _Info()
        _check(L.bsx_get_info(self.h, C.byref(info)), self.h, "bsx_get_info")
        self.info = {k: (list(getattr(info, k)) if k in ("roi", "in_roi") else getattr(info, k)) for k, _ in _Info._fields_}
        self.width, self.height, self.n_streams, self.device = info.width, info.height, info.n_streams, device
        return self

    def geometries(self):
        """the context's geometry classes: a list of dicts (width, height, n_streams, first_stream, roi, in_roi, mask_offset) — one entry for a one-geometry context"""
        if getattr(self, "_geoms", None) is None:
            out = []
            for g in range(lib().bsx_geom_count(self.h)):
                gi = _GeomInfo()
                _check(lib().bsx_get_geom_info(self.h, g, C.byref(gi)), self.h, "bsx_get_geom_info")
                out.append({k: (list(getattr(gi, k)) if k in ("roi", "in_roi") else getattr(gi, k)) for k, _ in _GeomInfo._fields_})
            self._geoms = out
        return self._geoms

    def _geom_of(self, stream):
        for g in self.geometries():
            if g["first_stream"] <= stream < g["first_stream"] + g["n_streams"]:
                return g
        raise BsxError("stream %d is out of range [0, %d)" % (stream, self.n_streams))

    def _on_device(self, t):
        return t.is_cuda and t.device.index == self.device

    def masks_of(self, stream):
        """torch u8 view [H_g, W_g] of the persistent mask of one stream, at the capture size of its class"""
        stream = int(stream)
        g = self._geom_of(stream)
        px = g["width"] * g["height"]
        p, b = C.c_void_p(), C.c_size_t()
        _check(lib().bsx_debug_buffer(self.h, 3, C.byref(p), C.byref(b)), self.h, "bsx_debug_buffer")
        return _as_torch(p.value + g["mask_offset"] + (stream - g["first_stream"]) * px, px, "uint8", (g["height"], g["width"]), self.device)

    def _u8(self, t, shape):
        """is t a contiguous uint8 tensor of that shape on the context's device?"""
        torch = _torch()
        return isinstance(t, torch.Tensor) and t.dtype == torch.uint8 and self._on_device(t) and tuple(t.shape) == shape and t.is_contiguous()

    def _geom_setting(self, who, i, s, H, W, stream, item, yuyv_in=True):
        """settings[i] of a multi-geometry step, validated against its class's size and written into item.setting"""
        if not isinstance(s, StreamSetting):
            raise BsxError("settings[%d] is not a StreamSetting" % i)
        if s.bgblur:
            raise BsxError("settings[%d]: bgblur is not taken by %s" % (i, who))
        if s.yuyv_in and not yuyv_in:
            raise BsxError("settings[%d]: yuyv_in is not taken by %s (every frame is an NV12 surface)" % (i, who))
        if not s.filter_off and s.bg is None:
            raise BsxError("settings[%d]: bg is required unless filter_off is set" % i)
        if s.bg is not None and not self._u8(s.bg, (H, W, 3)):
            raise BsxError("settings[%d].bg must be a contiguous cuda:%d uint8 tensor [%d,%d,3] (stream %d)" % (i, self.device, H, W, stream))
        item.setting.d_bg = s.bg.data_ptr() if s.bg is not None else None
        item.setting.flags = s.flags()

    def _geom_items(self, who, ids, frames, settings, outs=None, ch=3, common=False):
        """the ids and items of step_geoms / step_vcam_geoms / step_vcam_geoms_outs / _nv12, validated: (ctypes ids, n, ctypes items, out_w, out_h).  outs: one output
        per item, at the size of the item's class, or (common) all at the size of outs[0], which is returned; None: the items carry no output"""
        arr, n = _ids(ids)
        frames, settings = list(frames), list(settings)
        if outs is None:
            if len(frames) != n or len(settings) != n:
                raise BsxError("%d ids for %d frames and %d settings" % (n, len(frames), len(settings)))
        elif len(frames) != n or len(outs) != n or len(settings) != n:
            raise BsxError("%d ids for %d frames, %d outs and %d settings" % (n, len(frames), len(outs), len(settings)))
        items = (_GeomItem * max(n, 1))()
        out_h = out_w = 0
        if common and n:
            if not isinstance(outs[0], _torch().Tensor) or outs[0].dim() != 3 or outs[0].shape[2] != ch:
                raise BsxError("outs[0] must be a cuda:%d uint8 tensor [out_h,out_w,%d]: it gives the output size" % (self.device, ch))
            out_h, out_w = int(outs[0].shape[0]), int(outs[0].shape[1])
            if ch == 2 and (out_w & 1):
                raise BsxError("YUYV output needs an even width (outs[0] is %d wide)" % out_w)
        for i in range(n):
            g = self._geom_of(int(arr[i]))
            H, W = g["height"], g["width"]
            s = settings[i]
            fch = 2 if isinstance(s, StreamSetting) and s.yuyv_in else 3      # the item's own pixel format: YUYV 4:2:2 or BGR
            if not self._u8(frames[i], (H, W, fch)):
                raise BsxFrameFormatError("frames[%d] must be a contiguous cuda:%d uint8 tensor [%d,%d,%d] (stream %d%s)" % (
                    i, self.device, H, W, fch, arr[i], ", a YUYV item" if fch == 2 else ""))
            if common and not self._u8(outs[i], (out_h, out_w, ch)):
                raise BsxError("outs[%d] must be a contiguous cuda:%d uint8 tensor [%d,%d,%d] (the size of outs[0])" % (i, self.device, out_h, out_w, ch))
            if outs is not None and not common and not self._u8(outs[i], (H, W, ch)):
                raise BsxError("outs[%d] must be a contiguous cuda:%d uint8 tensor [%d,%d,%d] (stream %d)" % (i, self.device, H, W, ch, arr[i]))
            self._geom_setting(who, i, s, H, W, arr[i], items[i])
            items[i].d_frame, items[i].d_out = frames[i].data_ptr(), outs[i].data_ptr() if outs is not None else None
        return arr, n, items, out_w, out_h

    def _out_records(self, outs, n, rec_type, form, fill):
        """the output records of a call of n positions, validated: (ctypes records, m).  outs: a list of (item_index, ...) of the given form (its words, its length);
        fill(j, record, ...) checks the rest of outs[j], writes the record's buffers and returns (out_w, out_h)"""
        m = len(outs)
        recs = (rec_type * max(m, 1))()
        named, sizes = {}, []
        for j, rec in enumerate(outs):
            if not isinstance(rec, (tuple, list)) or len(rec) != form[1]:
                raise BsxError("outs[%d] must be a %s" % (j, form[0]))
            item = rec[0]
            if isinstance(item, bool) or not isinstance(item, (int, np.integer)) or not 0 <= int(item) < n:
                raise BsxError("outs[%d]: item %r is not an index into the call's %d positions" % (j, item, n))
            ow, oh = fill(j, recs[j], *rec[1:])
            named[int(item)] = named.get(int(item), 0) + 1
            if named[int(item)] > BSX_MAX_OUTS_PER_ITEM:
                raise BsxError("outs[%d]: record %d of position %d (at most %d name one position)" % (j, named[int(item)], int(item), BSX_MAX_OUTS_PER_ITEM))
            if (ow, oh) not in sizes:
                sizes.append((ow, oh))
                if len(sizes) > BSX_MAX_OUT_SIZES:
                    raise BsxError("outs[%d]: %d x %d is distinct output size %d of the call (at most %d)" % (j, ow, oh, len(sizes), BSX_MAX_OUT_SIZES))
            recs[j].item, recs[j].out_w, recs[j].out_h = int(item), ow, oh
        return recs, m

    def step_geoms(self, ids, frames, outs, settings, yuyv=False, no_mask=False):
        """one main-loop iteration for streams of ANY mix of the context's geometry classes (bsx_step_batch_geoms): ids[i] names the stream of position i, frames[i]
        (cuda uint8 [H_g, W_g, 3] BGR, or the camera's raw YUYV 4:2:2 [H_g, W_g, 2] for an item whose setting has yuyv_in), outs[i] ([H_g, W_g, 3], or [.., 2]
        with yuyv) and settings[i] (a StreamSetting: bg at the class's size, flip_h, flip_v, filter_off, yuyv_in; no bgblur) have the capture size of that
        stream's class.  One prep launch, one network pass, one tile launch whatever the mix of sizes and pixel formats."""
        outs = list(outs)
        arr, n, items, _w, _h = self._geom_items("step_geoms", ids, frames, settings, outs, 2 if yuyv else 3)
        flags = (1 if yuyv else 0) | (8 if no_mask else 0)
        _check(lib().bsx_step_batch_geoms(self.h, arr, items, n, _stream_ptr(), flags), self.h, "bsx_step_batch_geoms")
        return outs

    def step_vcam_geoms(self, ids, frames, outs, settings, yuyv=False):
        """step_geoms with every composite written at ONE common size, the virtual camera's (bsx_step_batch_vcam_geoms): frames[i] and settings[i].bg have the
        capture size of the class of ids[i] (frames[i] is [H_g, W_g, 2] YUYV 4:2:2 where settings[i].yuyv_in); every outs[i] is a cuda uint8 [out_h, out_w, 3]
        (or [.., 2] with yuyv) — the size is taken from outs[0].  Blend ->
        flip -> resize -> [pack] in one pass per position: no capture-size composite is stored."""
        outs = list(outs)
        arr, n, items, out_w, out_h = self._geom_items("step_vcam_geoms", ids, frames, settings, outs, 2 if yuyv else 3, common=True)
        _check(lib().bsx_step_batch_vcam_geoms(self.h, arr, items, n, out_w, out_h, _stream_ptr(), 1 if yuyv else 0), self.h, "bsx_step_batch_vcam_geoms")
        return outs

    def step_vcam_geoms_outs(self, ids, frames, settings, outs, yuyv=False):
        """step_vcam_geoms with several outputs per stream, each of its own size (bsx_step_batch_vcam_geoms_outs): outs is a sequence of (item_index, tensor) —
        write the composite of position item_index at the tensor's size, a cuda uint8 [out_h, out_w, 3] (or [.., 2] with yuyv).  A position may be named by 0 to 4
        records (with none its stream still advances), a call uses at most 4 distinct sizes.  Every stream is filtered once; one resize pass writes every record."""
        torch = _torch()
        outs = list(outs)
        arr, n, items, _w, _h = self._geom_items("step_vcam_geoms_outs", ids, frames, settings)
        ch = 2 if yuyv else 3

        def fill(j, r, t):
            if not isinstance(t, torch.Tensor) or t.dim() != 3 or not self._u8(t, (int(t.shape[0]), int(t.shape[1]), ch)) or t.numel() == 0:
                raise BsxError("outs[%d]: the output must be a contiguous, non-empty cuda:%d uint8 tensor [out_h,out_w,%d]" % (j, self.device, ch))
            if yuyv and (int(t.shape[1]) & 1):
                raise BsxError("outs[%d]: YUYV output needs an even width (the tensor is %d wide)" % (j, int(t.shape[1])))
            r.d_out = t.data_ptr()
            return int(t.shape[1]), int(t.shape[0])
        recs, m = self._out_records(outs, n, _VcamOut, ("pair (item_index, tensor)", 2), fill)
        _check(lib().bsx_step_batch_vcam_geoms_outs(self.h, arr, items, n, recs, m, _stream_ptr(), 1 if yuyv else 0), self.h, "bsx_step_batch_vcam_geoms_outs")
        return [t for _i, t in outs]

    def _nv12_planes(self, who, y, uv, device=True):
        """the two views of an NV12 surface, validated: (out_w, out_h, pitch_y, pitch_uv).  y: uint8 [out_h, out_w] with strides (pitch_y, 1); uv: uint8
        [out_h / 2, out_w] with strides (pitch_uv, 1) — U, V interleaved; sizes even, pitches multiples of 4, both 4-byte aligned.  device=False: where the tensors
        live is the caller's to check."""
        torch = _torch()
        for name, t in (("y", y), ("uv", uv)):
            if not isinstance(t, torch.Tensor) or t.dtype != torch.uint8 or t.dim() != 2 or t.numel() == 0:
                raise BsxError("%s: %s must be a non-empty uint8 tensor of two dimensions (it is %s)" % (who, name, "a %s" % type(t).__name__ if not isinstance(
                    t, torch.Tensor) else "%s %s" % (t.dtype, tuple(t.shape))))
            if device and not self._on_device(t):
                raise BsxError("%s: %s must be on cuda:%d (it is on %s)" % (who, name, self.device, t.device))
        oh, ow = int(y.shape[0]), int(y.shape[1])
        if (ow | oh) & 1:
            raise BsxError("%s: NV12 needs an even width and height (y is %d x %d)" % (who, ow, oh))
        if tuple(uv.shape) != (oh // 2, ow):
            raise BsxError("%s: uv must be [%d, %d] for a y of [%d, %d] (it is %s)" % (who, oh // 2, ow, oh, ow, list(uv.shape)))
        pitch = []
        for name, t in (("y", y), ("uv", uv)):
            if t.stride(1) != 1:
                raise BsxError("%s: %s has an inner stride of %d (the bytes of a row must be adjacent)" % (who, name, t.stride(1)))
            p = int(t.stride(0)) if t.shape[0] > 1 else max(int(t.stride(0)), ow)      # (the stride of a single row means nothing: any pitch that holds the row)
            if p < ow:
                raise BsxError("%s: the pitch of %s, %d, is below out_w = %d" % (who, name, p, ow))
            if p % 4:
                raise BsxError("%s: the pitch of %s, %d, is not a multiple of 4" % (who, name, p))
            if t.data_ptr() % 4:
                raise BsxError("%s: %s at 0x%x is not 4-byte aligned" % (who, name, t.data_ptr()))
            pitch.append(p)
        return ow, oh, pitch[0], pitch[1]

    def _nv12_out_records(self, outs, n):
        """the NV12 output records of a call of n positions, validated: (ctypes records, m).  outs: a list of (item_index, y, uv)"""
        def fill(j, r, y, uv):
            ow, oh, r.pitch_y, r.pitch_uv = self._nv12_planes("outs[%d]" % j, y, uv)
            r.d_y, r.d_uv = y.data_ptr(), uv.data_ptr()
            return ow, oh
        return self._out_records(outs, n, _VcamOutNv12, ("triple (item_index, y, uv)", 3), fill)

    def step_vcam_geoms_outs_nv12(self, ids, frames, settings, outs):
        """step_vcam_geoms_outs with every output an NV12 surface with row pitches, as a video encoder takes it (bsx_step_batch_vcam_geoms_outs_nv12): outs is a
        sequence of (item_index, y, uv) — y a cuda uint8 view [out_h, out_w] with strides (pitch_y, 1), uv [out_h / 2, out_w] with strides (pitch_uv, 1), U and V
        interleaved; sizes and pitches are read from the views.  out_w and out_h even, pitches multiples of 4, both planes 4-byte aligned.  Y and chroma are the
        bytes of the YUYV output of step_vcam_geoms_outs, the chroma averaged (truncating) over each pair of rows; bytes past out_w of a row are not written."""
        outs = list(outs)
        arr, n, items, _w, _h = self._geom_items("step_vcam_geoms_outs_nv12", ids, frames, settings)
        recs, m = self._nv12_out_records(outs, n)
        _check(lib().bsx_step_batch_vcam_geoms_outs_nv12(self.h, arr, items, n, recs, m, _stream_ptr(), 0), self.h, "bsx_step_batch_vcam_geoms_outs_nv12")
        return [(y, uv) for _i, y, uv in outs]

    def step_surfaces(self, ids, surfaces, settings, outs):
        """step_vcam_geoms_outs_nv12 whose frames are NV12 surfaces too, as a video decoder leaves them (bsx_step_batch_surfaces): surfaces is a sequence of (y, uv),
        one per id — y a cuda uint8 view [H, W] with strides (pitch_y, 1), uv [H / 2, W] with strides (pitch_uv, 1), U and V interleaved, at the capture size of the
        stream's class; pitches multiples of 4, both planes 4-byte aligned; bytes past W of a row are never read.  The BGR frame of a surface is nv12_to_bgr of it.
        settings: flip_h / flip_v / filter_off and bg (no bgblur, no yuyv_in); outs: as step_vcam_geoms_outs_nv12."""
        arr, n = _ids(ids)
        surfaces, settings, outs = list(surfaces), list(settings), list(outs)
        if len(surfaces) != n or len(settings) != n:
            raise BsxError("%d ids for %d surfaces and %d settings" % (n, len(surfaces), len(settings)))
        items = (_SurfaceItem * max(n, 1))()
        for i in range(n):
            g = self._geom_of(int(arr[i]))
            H, W = g["height"], g["width"]
            if not isinstance(surfaces[i], (tuple, list)) or len(surfaces[i]) != 2:
                raise BsxError("surfaces[%d] must be a pair (y, uv)" % i)
            y, uv = surfaces[i]
            sw, sh, py, puv = self._nv12_planes("surfaces[%d]" % i, y, uv)
            if (sw, sh) != (W, H):
                raise BsxFrameFormatError("surfaces[%d] is %d x %d, stream %d captures %d x %d" % (i, sw, sh, arr[i], W, H))
            self._geom_setting("step_surfaces", i, settings[i], H, W, arr[i], items[i], yuyv_in=False)
            it = items[i]
            it.d_y, it.d_uv, it.pitch_y, it.pitch_uv = y.data_ptr(), uv.data_ptr(), py, puv
        recs, m = self._nv12_out_records(outs, n)
        _check(lib().bsx_step_batch_surfaces(self.h, arr, items, n, recs, m, _stream_ptr(), 0), self.h, "bsx_step_batch_surfaces")
        return [(y, uv) for _i, y, uv in outs]

    # ---- batched device path -----------------------------------------------------------------
    def process_batch(self, frames, masks_out=None):
        """frames: torch u8 cuda [n,H,W,3] contiguous.  Returns a torch view [n,H,W] of the persistent masks."""
        n = self._n(frames)
        mo = C.c_void_p(masks_out.data_ptr()) if masks_out is not None else None
        _check(lib().bsx_process_batch(self.h, C.c_void_p(frames.data_ptr()), n, mo, _stream_ptr()), self.h, "bsx_process_batch")
        return self.masks()[:n]

    def composite(self, bg, frames, masks=None, out=None):
        torch = _torch()
        n = self._n(frames)
        if out is None:
            out = torch.empty_like(frames)
        stride = self._bg(bg, n)
        mp = C.c_void_p(masks.data_ptr()) if masks is not None else None
        _check(lib().bsx_composite_batch(self.h, C.c_void_p(bg.data_ptr()), stride, C.c_void_p(frames.data_ptr()), mp,
                                         C.c_void_p(out.data_ptr()), n, _stream_ptr()), self.h, "bsx_composite_batch")
        return out

    def _bg(self, bg, n):
        """background operand of a step → bg_frame_stride: ONE image [H,W,3] shared by all streams, or one per stream [>=n,H,W,3] — cuda uint8 on the context's
        device with a contiguous [H,W,3] inside; the stream dimension may be strided or expanded (stride 0 = one image for all), which is what the C ABI's
        bg_frame_stride serves.  (every entry point validates, not only step_pipelined.)"""
        ok = (bg.dtype == _torch().uint8 and bg.is_cuda and bg.dim() in (3, 4) and tuple(bg.shape[-3:]) == (self.height, self.width, 3)
              and tuple(bg.stride()[-3:]) == (self.width * 3, 3, 1) and (bg.dim() == 3 or bg.shape[0] >= n) and bg.device.index == self.device
              and (bg.dim() == 3 or bg.stride(0) >= 0))
        if not ok:
            raise BsxError("bg must be a cuda:%d uint8 tensor [%d,%d,3] or [>=%d,%d,%d,3] with contiguous images" % (self.device, self.height, self.width, n, self.height, self.width))
        return 0 if bg.dim() == 3 else int(bg.stride(0))

    def _step_out(self, out, n, yuyv):
        want = (self.height, self.width, 2 if yuyv else 3)
        if out.dim() != 4 or tuple(out.shape[1:]) != want or out.shape[0] < n or not out.is_contiguous() or not out.is_cuda or out.dtype != _torch().uint8:
            raise BsxError("out must be a contiguous cuda uint8 tensor [>=%d,%d,%d,%d]" % ((n,) + want))

    def _step_flags(self, bg, n, flip_h=False, flip_v=False, yuyv=False, no_mask=False, yuyv_in=False, bgblur=0):
        """the flags word of a step (bsx.h BSX_STEP_*) and bg_frame_stride; bg may be None only with bgblur"""
        if bg is None and not bgblur:
            raise BsxError("bg is required unless bgblur is set")
        flags = (1 if yuyv else 0) | (2 if flip_h else 0) | (4 if flip_v else 0) | (8 if no_mask else 0) | (16 if yuyv_in else 0) | ((int(bgblur) & 255) << 8)
        return flags, (0 if bg is None else self._bg(bg, n))

    def step(self, frames, bg, out):
        n = self._n(frames)
        stride = self._bg(bg, n)
        _check(lib().bsx_step_batch(self.h, C.c_void_p(frames.data_ptr()), C.c_void_p(bg.data_ptr()), stride,
                                    C.c_void_p(out.data_ptr()), n, _stream_ptr()), self.h, "bsx_step_batch")
        return out

    def step_yuyv(self, frames, bg, out_yuyv):
        """one main-loop iteration with the composite written as YUYV 4:2:2 [n,H,W,2] (convert_rgb_to_yuyv fused into the blend)"""
        n = self._n(frames)
        if (out_yuyv.dim() != 4 or tuple(out_yuyv.shape[1:]) != (self.height, self.width, 2) or out_yuyv.shape[0] < n or not out_yuyv.is_contiguous()
                or not out_yuyv.is_cuda or out_yuyv.dtype != _torch().uint8):
            raise BsxError("out_yuyv must be a contiguous cuda uint8 tensor [>=%d,%d,%d,2]" % (n, self.height, self.width))
        stride = self._bg(bg, n)
        _check(lib().bsx_step_batch_yuyv(self.h, C.c_void_p(frames.data_ptr()), C.c_void_p(bg.data_ptr()), stride,
                                         C.c_void_p(out_yuyv.data_ptr()), n, _stream_ptr()), self.h, "bsx_step_batch_yuyv")
        return out_yuyv

    def step_ex(self, frames, bg, out, flip_h=False, flip_v=False, yuyv=False, no_mask=False, bgblur=0, yuyv_in=False):
        """one main-loop iteration with cv::flip of the composite (app/deepseg.cc:667-673) and / or the YUYV pack folded into the blend's store;
        bgblur=<odd ksize>: the background is GaussianBlur(the stream's own frame) (-p bgblur:<n> without -b, deepseg.cc:652-661), `bg` may be None;
        yuyv_in: `frames` is the camera's raw YUYV 4:2:2 [n,H,W,2] (cv::COLOR_YUV2BGR_YUYV folded into the kernels that read it: BSX_STEP_YUYV_IN)"""
        n = self._n(frames, yuyv_in)
        self._step_out(out, n, yuyv)
        flags, stride = self._step_flags(bg, n, flip_h, flip_v, yuyv, no_mask, yuyv_in, bgblur)
        _check(lib().bsx_step_batch_ex(self.h, _ptr(frames), _ptr(bg), stride, _ptr(out), n, _stream_ptr(), flags), self.h, "bsx_step_batch_ex")
        return out

    def step_streams(self, ids, frames, bg, out, flip_h=False, flip_v=False, yuyv=False, no_mask=False, bgblur=0, yuyv_in=False):
        """step_ex for the streams named in `ids` (bsx_step_batch_streams): frames[i], bg[i] (per-stream backgrounds) and out[i] belong to stream ids[i], whose
        temporal state and persistent mask advance in place; every other stream is untouched.  ids: n distinct stream indices (any sequence of ints), n = len(frames)"""
        arr, n_ids = _ids(ids)
        if n_ids == 0:
            _check(lib().bsx_step_batch_streams(self.h, arr, None, None, 0, None, 0, _stream_ptr(), 0), self.h, "bsx_step_batch_streams")
            return out
        n = self._n(frames, yuyv_in)
        if n != n_ids:
            raise BsxError("%d ids for a batch of %d frames" % (n_ids, n))
        self._step_out(out, n, yuyv)
        flags, stride = self._step_flags(bg, n, flip_h, flip_v, yuyv, no_mask, yuyv_in, bgblur)
        _check(lib().bsx_step_batch_streams(self.h, arr, _ptr(frames), _ptr(bg), stride, _ptr(out), n, _stream_ptr(), flags), self.h, "bsx_step_batch_streams")
        return out

    def _setting_bg(self, bg, i):
        """a stream's background image: cuda:<device> uint8 [H,W,3], contiguous (the checks of _bg for one image)"""
        ok = (bg.dtype == _torch().uint8 and bg.is_cuda and bg.dim() == 3 and tuple(bg.shape) == (self.height, self.width, 3)
              and tuple(bg.stride()) == (self.width * 3, 3, 1) and bg.device.index == self.device)
        if not ok:
            raise BsxError("settings[%d].bg must be a contiguous cuda:%d uint8 tensor [%d,%d,3]" % (i, self.device, self.height, self.width))
        return bg.data_ptr()

    def step_mixed(self, frames, out, settings, ids=None, yuyv=False, no_mask=False, yuyv_in=False):
        """one main-loop iteration where every stream has its OWN settings (bsx_step_batch_mixed): settings[i] (a StreamSetting) belongs to frames[i] / out[i] —
        background image, flip, bgblur, filter switch — in one mask pipeline and one tile launch.  ids: None = frame i is stream i, else the stream ids as in
        step_streams.  yuyv / no_mask / yuyv_in are batch-wide (they define the buffer layouts)."""
        settings = list(settings)
        arr, n_ids = _ids(ids) if ids is not None else (None, None)
        n = self._n(frames, yuyv_in) if (ids is None or n_ids) else 0
        if ids is not None and n_ids != n:
            raise BsxError("%d ids for a batch of %d frames" % (n_ids, n))
        if len(settings) != n:
            raise BsxError("%d settings for a batch of %d frames" % (len(settings), n))
        if n == 0:
            _check(lib().bsx_step_batch_mixed(self.h, arr, None, None, None, 0, _stream_ptr(), 0), self.h, "bsx_step_batch_mixed")
            return out
        self._step_out(out, n, yuyv)
        st = self._settings(settings)
        flags = (1 if yuyv else 0) | (8 if no_mask else 0) | (16 if yuyv_in else 0)
        _check(lib().bsx_step_batch_mixed(self.h, arr, _ptr(frames), st, _ptr(out), n, _stream_ptr(), flags), self.h, "bsx_step_batch_mixed")
        return out

    def _settings(self, settings):
        """a list of StreamSetting → the C array of bsx_stream_setting, each one checked"""
        st = (_StreamSetting * len(settings))()
        for i, s in enumerate(settings):
            if not isinstance(s, StreamSetting):
                raise BsxError("settings[%d] is not a StreamSetting" % i)
            reads_bg = not s.filter_off and not s.bgblur
            if reads_bg and s.bg is None:
                raise BsxError("settings[%d]: bg is required unless bgblur or filter_off is set" % i)
            st[i].d_bg = self._setting_bg(s.bg, i) if s.bg is not None else None
            st[i].flags = s.flags()
        return st

    def reset_streams(self, ids):
        """reset the temporal state of the listed streams only (ofinal -> 0, mask -> 255; bsx_reset_streams) — a slot reused for a new camera"""
        arr, n = _ids(ids)
        _check(lib().bsx_reset_streams(self.h, arr, n, _stream_ptr()), self.h, "bsx_reset_streams")

    def step_vcam(self, frames, bg, out, flip_h=False, flip_v=False, yuyv=False, yuyv_in=False, bgblur=0):
        """one main-loop iteration at the virtual camera's geometry (--vg, app/deepseg.cc:634-681): blend, flip, cv::resize to out's size and optionally the
        YUYV pack in one pass (bsx_step_batch_vcam).  out: contiguous cuda uint8 [>=n, out_h, out_w, 3], or [.., 2] with yuyv; out_w, out_h come from its shape."""
        self._vcam_out(out, yuyv)
        n = self._n(frames, yuyv_in)
        if out.shape[0] < n:
            raise BsxError("out holds %d frames, the batch has %d" % (out.shape[0], n))
        flags, stride = self._step_flags(bg, n, flip_h, flip_v, yuyv, False, yuyv_in, bgblur)
        _check(lib().bsx_step_batch_vcam(self.h, _ptr(frames), _ptr(bg), stride, _ptr(out), int(out.shape[2]), int(out.shape[1]), n, _stream_ptr(), flags),
               self.h, "bsx_step_batch_vcam")
        return out

    def _vcam_out(self, out, yuyv):
        """the output of a step at the virtual camera's geometry: out_w, out_h come from its shape"""
        ch = 2 if yuyv else 3
        if (out.dim() != 4 or out.shape[3] != ch or out.shape[1] <= 0 or out.shape[2] <= 0 or not out.is_contiguous() or not out.is_cuda
                or out.dtype != _torch().uint8 or (yuyv and out.shape[2] % 2)):
            raise BsxError("out must be a contiguous cuda uint8 tensor [n,out_h,out_w,%d]%s" % (ch, " with an even out_w" if yuyv else ""))

    def step_vcam_mixed(self, frames, out, settings, ids=None, yuyv=False, yuyv_in=False):
        """step_vcam where every stream has its OWN settings and the batch may be a chosen subset of the streams (bsx_step_batch_vcam_mixed): settings[i] (a
        StreamSetting: background image, flip, bgblur, filter switch) belongs to frames[i] / out[i]; blend, the stream's flip, cv::resize to out's size and
        optionally the YUYV pack in one pass.  ids: None = frame i is stream i, else the stream ids as in step_streams.  out: contiguous cuda uint8
        [>=n, out_h, out_w, 3], or [.., 2] with yuyv; out_w, out_h come from its shape.  yuyv / yuyv_in are batch-wide (they define the buffer layouts)."""
        settings = list(settings)
        arr, n_ids = _ids(ids) if ids is not None else (None, None)
        empty = ids is not None and n_ids == 0
        if not empty:
            self._vcam_out(out, yuyv)
        n = 0 if empty else self._n(frames, yuyv_in)
        if ids is not None and n_ids != n:
            raise BsxError("%d ids for a batch of %d frames" % (n_ids, n))
        if len(settings) != n:
            raise BsxError("%d settings for a batch of %d frames" % (len(settings), n))
        if n == 0:
            _check(lib().bsx_step_batch_vcam_mixed(self.h, arr, None, None, None, 0, 0, 0, _stream_ptr(), 0), self.h, "bsx_step_batch_vcam_mixed")
            return out
        if out.shape[0] < n:
            raise BsxError("out holds %d frames, the batch has %d" % (out.shape[0], n))
        st = self._settings(settings)
        flags = (1 if yuyv else 0) | (16 if yuyv_in else 0)
        _check(lib().bsx_step_batch_vcam_mixed(self.h, arr, _ptr(frames), st, _ptr(out), int(out.shape[2]), int(out.shape[1]), n, _stream_ptr(), flags),
               self.h, "bsx_step_batch_vcam_mixed")
        return out

    def step_pipelined(self, frames, bg, out, flip_h=False, flip_v=False, yuyv=False, no_mask=False, yuyv_in=False):
        """throughput mode (bsx_step_batch_pipelined): enqueue the mask pipeline of THIS batch and, concurrently, the composite of the batch handed over by
        the previous call (the reference's CalcMask worker next to its blend loop, app/deepseg.cc:159-285).  `out` — and masks() — hold THIS batch's results
        once the NEXT call (or flush_pipelined()) has completed; frames / bg / out must stay untouched until then.  Bit-identical to step_ex per batch."""
        n = self._n(frames, yuyv_in)
        self._step_out(out, n, yuyv)
        flags, stride = self._step_flags(bg, n, flip_h, flip_v, yuyv, no_mask, yuyv_in)
        _check(lib().bsx_step_batch_pipelined(self.h, _ptr(frames), _ptr(bg), stride, _ptr(out), n, _stream_ptr(), flags), self.h, "bsx_step_batch_pipelined")
        # the composite of THIS batch is enqueued by the NEXT call, on a stream torch's caching allocator knows nothing about: the three tensors stay referenced
        # here until then (a caller that drops them would otherwise have their memory handed out again under the pending kernel) — and for ONE MORE call: a caller
        # that alternates streams gets composite k joined into the stream of call k + 1, so a block of call k's stream freed right after call k + 1 could be handed
        # out again on that stream while the composite still runs.  Released after call k + 2, a flush or a reset.
        held = getattr(self, "_pending", None)
        self._pending_prev = held
        self._pending = (frames, bg, out)
        return out

    def flush_pipelined(self):
        """composite the batch still pending in the two-deep pipeline (on the current stream)"""
        _check(lib().bsx_step_batch_pipelined(self.h, None, None, 0, None, 0, _stream_ptr(), 0), self.h, "bsx_step_batch_pipelined(flush)")
        self._release_pending()

    def _release_pending(self):
        """drop the references step_pipelined holds: after a flush the composite that used them is ordered on the caller's own stream, after a reset it was dropped
        with the state.  (Between calls k and k + 1 the references move on by themselves: call k + 1 orders the caller's stream behind composite k — the launch that
        advances the temporal state waits for it — so memory freed after that call cannot be reused ahead of the composite.)"""
        self._pending = None
        self._pending_prev = None

    def profile(self, frames, bg, out, iters=5):
        """per-launch hipEvent timings of the whole per-batch sequence → list of dicts"""
        n = self._n(frames)
        cap = self.info["n_steps"] + 8
        arr = (LaunchStat * cap)()
        stride = self._bg(bg, n)
        k = lib().bsx_profile_batch(self.h, C.c_void_p(frames.data_ptr()), C.c_void_p(bg.data_ptr()), stride, C.c_void_p(out.data_ptr()),
                                    n, iters, arr, cap, _stream_ptr())
        if k < 0:
            _check(k, self.h, "bsx_profile_batch")
        return [dict(name=arr[i].name.decode(), avg_ms=arr[i].avg_ms, bytes=arr[i].bytes, flops=arr[i].flops) for i in range(k)]

    def program_timeline(self, n=None):
        """per-micro-op durations (microseconds, workgroup 0) of the per-frame network program"""
        n = n or self.n_streams
        cap = 1024 + 64 * 16 * 4
        arr = (C.c_ulonglong * cap)()
        k = lib().bsx_debug_program_timeline(self.h, n, arr, cap, _stream_ptr())
        if k < 0:
            _check(k, self.h, "bsx_debug_program_timeline")
        self.last_subphase_us = [arr[256 + i] / 100.0 for i in range(12)]   # debug accumulators of instrumented micro-ops
        # fine[op][wave] = (wait+barrier, weight-DMA issue, body) in shader cycles, lane 0 of each wave of workgroup 0
        self.last_fine = [[tuple(arr[1024 + (i * 16 + w) * 4 + j] for j in range(4)) for w in range(16)] for i in range(min(k, 64))]
        return [(arr[i + 1] - arr[i]) / 100.0 for i in range(k)]

    def masks(self):
        """torch u8 view [n_streams,H,W] of the lib-owned persistent masks (cf. `mask = ctx.mask`, libbackscrub.cc:374)."""
        return self._view(3, "uint8", (self.n_streams, self.height, self.width))

    def reset(self):
        _check(lib().bsx_reset(self.h, _stream_ptr()), self.h, "bsx_reset")
        self._release_pending()

    def resize_bgr(self, src, dw, dh):
        torch = _torch()
        n, sh, sw, _ = src.shape
        dst = torch.empty((n, dh, dw, 3), dtype=torch.uint8, device=src.device)
        _check(lib().bsx_resize_bgr(self.h, C.c_void_p(src.data_ptr()), sw, sh, C.c_void_p(dst.data_ptr()), dw, dh, n, _stream_ptr()),
               self.h, "bsx_resize_bgr")
        return dst

    def _batch_out(self, out, n, dw, dh):
        """the output of a batch of n images dw x dh: cuda:<device> uint8 [n,dh,dw,3] whose images are contiguous; the batch dimension may be strided (any stride
        >= one image: the C ABI takes one destination per image, of any alignment).  None: a new contiguous tensor."""
        torch = _torch()
        if out is None:
            return torch.empty((n, dh, dw, 3), dtype=torch.uint8, device="cuda:%d" % self.device)
        ok = (out.dtype == torch.uint8 and out.is_cuda and out.device.index == self.device and out.dim() == 4 and tuple(out.shape) == (n, dh, dw, 3)
              and tuple(out.stride()[1:]) == (dw * 3, 3, 1) and (n <= 1 or out.stride(0) >= dh * dw * 3))
        if not ok:
            raise BsxError("out must be a cuda:%d uint8 tensor [%d,%d,%d,3] with contiguous images that do not overlap" % (self.device, n, dh, dw))
        return out

    def resize_bgr_batch(self, srcs, dw, dh, out=None):
        """cv::resize of n images, each of its OWN size, to dw x dh in one launch (bsx_resize_bgr_batch; the integers of resize_bgr).  srcs: a sequence of
        contiguous cuda uint8 [sh_i, sw_i, 3] tensors on the context's device; out: see _batch_out.  Returns out ([n, dh, dw, 3])."""
        torch = _torch()
        srcs = list(srcs)
        n, dw, dh = len(srcs), int(dw), int(dh)
        if n > self.n_streams:
            raise BsxError("%d images for a context of %d streams" % (n, self.n_streams))
        if dw <= 0 or dh <= 0:
            raise BsxError("output size %d x %d is not positive" % (dw, dh))
        for i, t in enumerate(srcs):
            ok = (isinstance(t, torch.Tensor) and t.dtype == torch.uint8 and t.is_cuda and t.device.index == self.device and t.dim() == 3 and t.shape[2] == 3
                  and t.shape[0] > 0 and t.shape[1] > 0 and t.is_contiguous())
            if not ok:
                raise BsxError("srcs[%d] must be a contiguous cuda:%d uint8 tensor [h,w,3]" % (i, self.device))
        out = self._batch_out(out, n, dw, dh)
        items = (_ResizeItem * max(n, 1))()
        for i, t in enumerate(srcs):
            items[i].d_src, items[i].sw, items[i].sh, items[i].d_dst = t.data_ptr(), int(t.shape[1]), int(t.shape[0]), out.data_ptr() + i * out.stride(0)
        _check(lib().bsx_resize_bgr_batch(self.h, items, n, dw, dh, _stream_ptr()), self.h, "bsx_resize_bgr_batch")
        return out

    def bgr_to_yuyv(self, bgr):
        torch = _torch()
        n, h, w, _ = bgr.shape
        out = torch.empty((n, h, w, 2), dtype=torch.uint8, device=bgr.device)
        _check(lib().bsx_bgr_to_yuyv(self.h, C.c_void_p(bgr.data_ptr()), C.c_void_p(out.data_ptr()), w, h, n, _stream_ptr()),
               self.h, "bsx_bgr_to_yuyv")
        return out

    def bgr_to_nv12(self, bgr, pitch_y=None, pitch_uv=None):
        """[n,h,w,3] u8 device frames → NV12 (bsx_bgr_to_nv12): (y, uv), views [n, h, w] and [n, h / 2, w] (U, V interleaved) of planes with rows of pitch_y and
        pitch_uv bytes (default: w rounded up to a multiple of 4).  w and h even; bytes past w of a row are not written (the planes are allocated zeroed)."""
        torch = _torch()
        if not isinstance(bgr, torch.Tensor) or bgr.dtype != torch.uint8 or bgr.dim() != 4 or bgr.shape[3] != 3 or bgr.numel() == 0 or not bgr.is_contiguous():
            raise BsxFrameFormatError("bgr must be a contiguous, non-empty uint8 tensor [n,h,w,3]")
        if not self._on_device(bgr):
            raise BsxError("bgr must be on cuda:%d (it is on %s)" % (self.device, bgr.device))
        n, h, w, _ = (int(v) for v in bgr.shape)
        if (w | h) & 1:
            raise BsxFrameFormatError("NV12 needs an even width and height (bgr is %d x %d)" % (w, h))
        pitch = []
        for name, p in (("pitch_y", pitch_y), ("pitch_uv", pitch_uv)):
            p = (w + 3) // 4 * 4 if p is None else p
            if isinstance(p, bool) or not isinstance(p, (int, np.integer)) or p < w or p % 4:
                raise BsxError("%s = %r must be a multiple of 4 and at least w = %d" % (name, p, w))
            pitch.append(int(p))
        y = torch.zeros((n, h, pitch[0]), dtype=torch.uint8, device=bgr.device)
        uv = torch.zeros((n, h // 2, pitch[1]), dtype=torch.uint8, device=bgr.device)
        _check(lib().bsx_bgr_to_nv12(self.h, C.c_void_p(bgr.data_ptr()), w, h, n, C.c_void_p(y.data_ptr()), pitch[0], C.c_void_p(uv.data_ptr()), pitch[1],
                                     _stream_ptr()), self.h, "bsx_bgr_to_nv12")
        return y[:, :, :w], uv[:, :, :w]

    def nv12_to_bgr(self, y, uv, w=None, h=None):
        """NV12 surfaces → [n,h,w,3] u8 device frames (bsx_nv12_to_bgr), the counterpart of bgr_to_nv12 and of its layout: y a cuda uint8 view [n, h, w] (or [h, w])
        with strides (h * pitch_y, pitch_y, 1), uv [n, h / 2, w] with strides (h / 2 * pitch_uv, pitch_uv, 1), U and V interleaved — the images' planes one behind
        the other.  w, h: checked against the views where given.  Bytes past w of a row are not read."""
        torch = _torch()
        for name, t in (("y", y), ("uv", uv)):
            if not isinstance(t, torch.Tensor) or t.dtype != torch.uint8 or t.dim() not in (2, 3) or t.numel() == 0:
                raise BsxFrameFormatError("nv12_to_bgr: %s must be a non-empty uint8 tensor [n,rows,w] or [rows,w]" % name)
            if not self._on_device(t):
                raise BsxError("nv12_to_bgr: %s must be on cuda:%d (it is on %s)" % (name, self.device, t.device))
        if y.dim() != uv.dim():
            raise BsxFrameFormatError("nv12_to_bgr: y has %d dimensions and uv %d" % (y.dim(), uv.dim()))
        y3, uv3 = (y, uv) if y.dim() == 3 else (y[None], uv[None])
        n = int(y3.shape[0])
        if int(uv3.shape[0]) != n:
            raise BsxFrameFormatError("nv12_to_bgr: y holds %d images and uv %d" % (n, int(uv3.shape[0])))
        sw, sh, py, puv = self._nv12_planes("nv12_to_bgr", y3[0], uv3[0])
        if (w is not None and int(w) != sw) or (h is not None and int(h) != sh):
            raise BsxFrameFormatError("nv12_to_bgr: the views are %d x %d, not w = %r, h = %r" % (sw, sh, w, h))
        if n > 1 and (y3.stride(0) != sh * py or uv3.stride(0) != sh // 2 * puv):
            raise BsxFrameFormatError("nv12_to_bgr: image i's planes must lie at i * h * pitch_y and i * (h / 2) * pitch_uv (strides %d and %d, pitches %d and %d)" % (
                y3.stride(0), uv3.stride(0), py, puv))
        out = torch.empty((n, sh, sw, 3), dtype=torch.uint8, device=y.device)
        _check(lib().bsx_nv12_to_bgr(self.h, C.c_void_p(y3.data_ptr()), py, C.c_void_p(uv3.data_ptr()), puv, sw, sh, n, C.c_void_p(out.data_ptr()), _stream_ptr()),
               self.h, "bsx_nv12_to_bgr")
        return out if y.dim() == 3 else out[0]

    def flip_bgr(self, bgr, code):
        """cv::flip(bgr, out, code) for [n,h,w,3] u8 device frames (deepseg.cc:667-673): 0 vertical, >0 horizontal, <0 both."""
        torch = _torch()
        n, h, w, _ = bgr.shape
        out = torch.empty_like(bgr)
        _check(lib().bsx_flip_bgr(self.h, C.c_void_p(bgr.data_ptr()), C.c_void_p(out.data_ptr()), w, h, n, int(code), _stream_ptr()), self.h, "bsx_flip_bgr")
        return out

    def gaussian_blur(self, bgr, ksize=25, out=None):
        """cv::GaussianBlur(bgr, out, Size(ksize, ksize), 0) for [n,h,w,3] u8 device frames (deepseg.cc:657-658, -p bgblur:<ksize>)."""
        torch = _torch()
        n, h, w, _ = bgr.shape
        if out is None:
            out = torch.empty_like(bgr)
        elif out.shape != bgr.shape or out.dtype != bgr.dtype or not out.is_contiguous() or out.device != bgr.device:
            raise BsxError("out must be a contiguous tensor shaped like the input")
        _check(lib().bsx_gaussian_blur_bgr(self.h, C.c_void_p(bgr.data_ptr()), C.c_void_p(out.data_ptr()), w, h, n, int(ksize), _stream_ptr()),
               self.h, "bsx_gaussian_blur_bgr")
        return out

    def gaussian_blur_batch(self, srcs, ksizes, out=None):
        """cv::GaussianBlur of n images, each of its OWN size, blur size and pixel format, in one launch (bsx_gaussian_blur_bgr_batch; the integers of
        gaussian_blur, after yuyv_to_bgr for a YUYV image).  srcs: a sequence of contiguous cuda uint8 tensors on the context's device, [h,w,3] (BGR) or [h,w,2]
        (the camera's raw YUYV 4:2:2); ksizes: one odd int of 1..31 for all, or one per image (1 = the image itself, converted); out: None (new tensors) or a
        sequence of contiguous [h_i,w_i,3] tensors.  Returns the list of outputs — what a StreamSetting's bg takes."""
        torch = _torch()
        srcs = list(srcs)
        n = len(srcs)
        if n > self.n_streams:
            raise BsxError("%d images for a context of %d streams" % (n, self.n_streams))
        ks = [int(ksizes)] * n if isinstance(ksizes, (int, np.integer)) else [int(k) for k in ksizes]
        if len(ks) != n:
            raise BsxError("%d ksizes for %d images" % (len(ks), n))
        for i, k in enumerate(ks):
            if k < 1 or k > 31 or not (k & 1):
                raise BsxError("ksizes[%d] = %d is not an odd number of 1..31" % (i, k))
        for i, t in enumerate(srcs):
            ok = (isinstance(t, torch.Tensor) and t.dtype == torch.uint8 and t.dim() == 3 and t.shape[2] in (2, 3) and t.shape[0] > 0 and t.shape[1] > 0
                  and t.is_contiguous())
            if not ok:
                raise BsxError("srcs[%d] must be a contiguous uint8 tensor [h,w,3] (BGR) or [h,w,2] (YUYV)" % i)
        if out is not None:
            out = list(out)
            if len(out) != n:
                raise BsxError("%d outputs for %d images" % (len(out), n))
            for i, (o, t) in enumerate(zip(out, srcs)):
                ok = isinstance(o, torch.Tensor) and o.dtype == torch.uint8 and tuple(o.shape) == (int(t.shape[0]), int(t.shape[1]), 3) and o.is_contiguous()
                if not ok:
                    raise BsxError("out[%d] must be a contiguous uint8 tensor [%d,%d,3]" % (i, int(t.shape[0]), int(t.shape[1])))
        for what, ts in (("srcs", srcs), ("out", out or [])):
            for i, t in enumerate(ts):
                if not t.is_cuda or t.device.index != self.device:
                    raise BsxError("%s[%d] is on %s, not on the context's cuda:%d" % (what, i, t.device, self.device))
        if out is None:
            out = [torch.empty((int(t.shape[0]), int(t.shape[1]), 3), dtype=torch.uint8, device="cuda:%d" % self.device) for t in srcs]
        items = (_BlurItem * max(n, 1))()
        for i, (t, o) in enumerate(zip(srcs, out)):
            items[i].d_src, items[i].d_dst, items[i].w, items[i].h = t.data_ptr(), o.data_ptr(), int(t.shape[1]), int(t.shape[0])
            items[i].ksize, items[i].flags = ks[i], BSX_STREAM_YUYV_IN if t.shape[2] == 2 else 0
        _check(lib().bsx_gaussian_blur_bgr_batch(self.h, items, n, _stream_ptr()), self.h, "bsx_gaussian_blur_bgr_batch")
        return out

    def gaussian_blur_surfaces(self, surfaces, ksizes, out=None):
        """gaussian_blur_batch for NV12 decoder surfaces, in one launch (bsx_gaussian_blur_surfaces_batch; the integers of nv12_to_bgr, then gaussian_blur's — no BGR
        copy of a frame is made).  surfaces: a sequence of (y, uv) as step_surfaces takes them, each of its own size and pitches — y a cuda uint8 view [h, w] with
        strides (pitch_y, 1), uv [h / 2, w] with strides (pitch_uv, 1); the surfaces need not be adjacent; ksizes: one odd int of 1..31 for all, or one per surface
        (1 = the conversion alone); out: None (new tensors) or a sequence of contiguous [h_i,w_i,3] tensors.  Returns the list of outputs — what a StreamSetting's
        bg takes, so a surfaces tick in blur mode is this call followed by step_surfaces."""
        torch = _torch()
        surfaces = list(surfaces)
        n = len(surfaces)
        if n > self.n_streams:
            raise BsxError("%d surfaces for a context of %d streams" % (n, self.n_streams))
        ks = [int(ksizes)] * n if isinstance(ksizes, (int, np.integer)) else [int(k) for k in ksizes]
        if len(ks) != n:
            raise BsxError("%d ksizes for %d surfaces" % (len(ks), n))
        for i, k in enumerate(ks):
            if k < 1 or k > 31 or not (k & 1):
                raise BsxError("ksizes[%d] = %d is not an odd number of 1..31" % (i, k))
        geo = []
        for i, sf in enumerate(surfaces):
            if not isinstance(sf, (tuple, list)) or len(sf) != 2:
                raise BsxError("surfaces[%d] must be a pair (y, uv)" % i)
            geo.append(self._nv12_planes("surfaces[%d]" % i, sf[0], sf[1], device=False))
        if out is not None:
            out = list(out)
            if len(out) != n:
                raise BsxError("%d outputs for %d surfaces" % (len(out), n))
            for i, (o, (w, h, _py, _puv)) in enumerate(zip(out, geo)):
                if not (isinstance(o, torch.Tensor) and o.dtype == torch.uint8 and tuple(o.shape) == (h, w, 3) and o.is_contiguous()):
                    raise BsxError("out[%d] must be a contiguous uint8 tensor [%d,%d,3]" % (i, h, w))
        for i, (y, uv) in enumerate(surfaces):
            for name, t in (("y", y), ("uv", uv)):
                if not self._on_device(t):
                    raise BsxError("surfaces[%d]: %s is on %s, not on the context's cuda:%d" % (i, name, t.device, self.device))
        for i, t in enumerate(out or []):
            if not self._on_device(t):
                raise BsxError("out[%d] is on %s, not on the context's cuda:%d" % (i, t.device, self.device))
        if out is None:
            out = [torch.empty((h, w, 3), dtype=torch.uint8, device="cuda:%d" % self.device) for w, h, _py, _puv in geo]
        items = (_BlurSurfaceItem * max(n, 1))()
        for i, ((y, uv), o, (w, h, py, puv)) in enumerate(zip(surfaces, out, geo)):
            it = items[i]
            it.d_y, it.d_uv, it.d_dst, it.pitch_y, it.pitch_uv = y.data_ptr(), uv.data_ptr(), o.data_ptr(), py, puv
            it.w, it.h, it.ksize, it.flags = w, h, ks[i], 0
        _check(lib().bsx_gaussian_blur_surfaces_batch(self.h, items, n, _stream_ptr()), self.h, "bsx_gaussian_blur_surfaces_batch")
        return out

    def resize_surfaces(self, surfaces, sizes, out=None):
        """grab_background() of video backgrounds whose frames a hardware decoder leaves as NV12 surfaces, in one launch (bsx_resize_surfaces_batch; the integers of
        nv12_to_bgr, then resize_bgr's — no BGR copy of a surface is made).  surfaces: a sequence of (y, uv) as gaussian_blur_surfaces takes them, each of its own
        size and pitches, not necessarily adjacent, the same one any number of times; sizes: one (w, h) for all, or one per surface — at most 8 distinct ones; out:
        None (new tensors) or a sequence of contiguous [h_i,w_i,3] tensors.  Returns the list of outputs — what a StreamSetting's bg takes, so a surfaces tick with
        video backgrounds is this call followed by step_surfaces."""
        torch = _torch()
        surfaces = list(surfaces)
        n = len(surfaces)
        if n > self.n_streams:
            raise BsxError("%d surfaces for a context of %d streams" % (n, self.n_streams))
        sizes = list(sizes)
        if len(sizes) == 2 and all(isinstance(v, (int, np.integer)) for v in sizes):
            sizes = [tuple(sizes)] * n
        if len(sizes) != n:
            raise BsxError("%d sizes for %d surfaces" % (len(sizes), n))
        dst = []
        for i, sz in enumerate(sizes):
            if not isinstance(sz, (tuple, list)) or len(sz) != 2 or not all(isinstance(v, (int, np.integer)) for v in sz):
                raise BsxError("sizes[%d] must be a pair (w, h) of integers" % i)
            if sz[0] <= 0 or sz[1] <= 0:
                raise BsxError("sizes[%d] = %d x %d is not positive" % (i, sz[0], sz[1]))
            dst.append((int(sz[0]), int(sz[1])))
        geo = []
        for i, sf in enumerate(surfaces):
            if not isinstance(sf, (tuple, list)) or len(sf) != 2:
                raise BsxError("surfaces[%d] must be a pair (y, uv)" % i)
            geo.append(self._nv12_planes("surfaces[%d]" % i, sf[0], sf[1], device=False))
        if out is not None:
            out = list(out)
            if len(out) != n:
                raise BsxError("%d outputs for %d surfaces" % (len(out), n))
            for i, (o, (w, h)) in enumerate(zip(out, dst)):
                if not (isinstance(o, torch.Tensor) and o.dtype == torch.uint8 and tuple(o.shape) == (h, w, 3) and o.is_contiguous()):
                    raise BsxError("out[%d] must be a contiguous uint8 tensor [%d,%d,3]" % (i, h, w))
        for i, (y, uv) in enumerate(surfaces):
            for name, t in (("y", y), ("uv", uv)):
                if not self._on_device(t):
                    raise BsxError("surfaces[%d]: %s is on %s, not on the context's cuda:%d" % (i, name, t.device, self.device))
        for i, t in enumerate(out or []):
            if not self._on_device(t):
                raise BsxError("out[%d] is on %s, not on the context's cuda:%d" % (i, t.device, self.device))
        if out is None:
            out = [torch.empty((h, w, 3), dtype=torch.uint8, device="cuda:%d" % self.device) for w, h in dst]
        items = (_ResizeSurfaceItem * max(n, 1))()
        for i, ((y, uv), o, (sw, sh, py, puv), (dw, dh)) in enumerate(zip(surfaces, out, geo, dst)):
            it = items[i]
            it.d_y, it.d_uv, it.d_dst, it.pitch_y, it.pitch_uv = y.data_ptr(), uv.data_ptr(), o.data_ptr(), py, puv
            it.sw, it.sh, it.dw, it.dh, it.flags, it.reserved = sw, sh, dw, dh, 0, 0
        _check(lib().bsx_resize_surfaces_batch(self.h, items, n, _stream_ptr()), self.h, "bsx_resize_surfaces_batch")
        return out

    def yuyv_to_bgr(self, yuyv):
        torch = _torch()
        n, h, w, _ = yuyv.shape
        out = torch.empty((n, h, w, 3), dtype=torch.uint8, device=yuyv.device)
        _check(lib().bsx_yuyv_to_bgr(self.h, C.c_void_p(yuyv.data_ptr()), C.c_void_p(out.data_ptr()), w, h, n, _stream_ptr()),
               self.h, "bsx_yuyv_to_bgr")
        return out

    # ---- drop-in single frame path (host buffers) -----------------------------------------------
    def process_host(self, frame: np.ndarray, stream_idx=0, mask_out: np.ndarray | None = None) -> np.ndarray:
        if frame.dtype != np.uint8 or frame.ndim != 3 or frame.shape[2] != 3 or frame.shape[0] != self.height or frame.shape[1] != self.width:
            raise BsxError("frame must be uint8 [%d,%d,3]" % (self.height, self.width))
        if frame.strides[2] != 1 or frame.strides[1] != 3:
            frame = np.ascontiguousarray(frame)
        if mask_out is None:
            mask_out = np.empty((self.height, self.width), np.uint8)
        elif (not isinstance(mask_out, np.ndarray) or mask_out.dtype != np.uint8 or mask_out.shape != (self.height, self.width)
              or mask_out.strides[1] != 1 or mask_out.strides[0] < self.width or not mask_out.flags.writeable):
            # the C side writes height rows of width bytes: anything else would scribble over the host heap
            raise BsxError("mask_out must be a writable uint8 [%d,%d] array with unit inner stride" % (self.height, self.width))
        _check(lib().bsx_process_host(self.h, stream_idx, frame.ctypes.data, frame.strides[0], mask_out.ctypes.data, mask_out.strides[0]),
               self.h, "bsx_process_host")
        return mask_out

    # ---- introspection (tests) --------------------------------------------------------------------
    def run_stage(self, stage, frames=None, n=None):
        n = n if n is not None else (self._n(frames, yuyv_in=(stage == 4)) if frames is not None else self.n_streams)
        fp = C.c_void_p(frames.data_ptr()) if frames is not None else None
        _check(lib().bsx_debug_run_stage(self.h, stage, fp, n, _stream_ptr()), self.h, "bsx_debug_run_stage")

    def input_tensor(self):
        i = self.info
        return self._view(0, "float32", (self.n_streams, i["in_h"], i["in_w"], i["in_c"]))

    def input_u8(self):
        """torch u8 view [n_streams, in_h, in_w, 4] of the 8-bit network input the steps' prep writes (bytes R, G, B, 0 of each word), by POSITION in the last
        call; BsxError where this context's stem reads the f32 form (input_tensor) instead"""
        i = self.info
        return self._view(4, "uint8", (self.n_streams, i["in_h"], i["in_w"], 4))

    def output_tensor(self):
        i = self.info
        return self._view(1, "float32", (self.n_streams, i["out_h"], i["out_w"], i["out_c"]))

    def ofinal(self):
        i = self.info
        return self._view(2, "uint8", (self.n_streams, i["out_h"], i["out_w"]))

    def plan(self) -> str:
        return lib().bsx_plan_describe(self.h).decode()

    def mask_tile_stats(self, n=None) -> dict:
        """how the fused mask + blend launch classifies its tiles for the current temporal state: a uniform tile (whole source block 0xFF / 0x00) skips the
        mask phases and reads only the operand its composite copies"""
        a = (C.c_long * 4)()
        _check(lib().bsx_debug_mask_tile_stats(self.h, n or self.n_streams, a), self.h, "bsx_debug_mask_tile_stats")
        return {"tiles": a[0], "uniform_255": a[1], "uniform_0": a[2], "general": a[3], "tile": "128x32"}

    def graph_tensor(self, idx, stream=None) -> np.ndarray:
        if stream is not None:
            n = lib().bsx_debug_tensor_of(self.h, idx, stream, None, 0)
            if n < 0:
                raise BsxError("tensor %d not materialised: %s" % (idx, (lib().bsx_last_error(self.h) or b"").decode(errors="replace").strip()))
            a = np.empty(n, np.float32)
            lib().bsx_debug_tensor_of(self.h, idx, stream, a.ctypes.data_as(C.POINTER(C.c_float)), n)
            return a
        n = lib().bsx_debug_tensor(self.h, idx, None, 0)
        if n < 0:
            raise BsxError("tensor %d not materialised" % idx)
        _torch().cuda.synchronize()
        a = np.empty(n, np.float32)
        lib().bsx_debug_tensor(self.h, idx, a.ctypes.data_as(C.POINTER(C.c_float)), n)
        return a

    def _view(self, which, dtype, shape):
        torch = _torch()
        p, b = C.c_void_p(), C.c_size_t()
        _check(lib().bsx_debug_buffer(self.h, which, C.byref(p), C.byref(b)), self.h, "bsx_debug_buffer")
        return _as_torch(p.value, b.value, dtype, shape, self.device)

    def _n(self, frames, yuyv_in=False):
        ch = 2 if yuyv_in else 3                 # BSX_STEP_YUYV_IN: the camera's raw 4:2:2 frames, 2 bytes per pixel
        if frames.dim() != 4 or tuple(frames.shape[1:]) != (self.height, self.width, ch) or not frames.is_contiguous() or not frames.is_cuda or frames.dtype != _torch().uint8:
            raise BsxError("frames must be a contiguous cuda uint8 tensor [n,%d,%d,%d]" % (self.height, self.width, ch))
        if frames.shape[0] > self.n_streams:
            raise BsxError("batch larger than n_streams")
        return int(frames.shape[0])

    def close(self):
        if getattr(self, "h", None):
            lib().bsx_delete(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class _CudaArray:
    """__cuda_array_interface__ holder so torch can alias lib-owned device memory without copying."""

    def __init__(self, ptr, nbytes, typestr, shape):
        self.__cuda_array_interface__ = {"shape": tuple(shape), "typestr": typestr, "data": (ptr, False), "version": 2, "strides": None}
        self._nbytes = nbytes


def _as_torch(ptr, nbytes, dtype, shape, device):
    torch = _torch()
    typestr = {"uint8": "|u1", "float32": "<f4"}[dtype]
    return torch.as_tensor(_CudaArray(ptr, nbytes, typestr, shape), device="cuda:%d" % device)


def media_decode(path: str):
    """Host-only decode of a background file (GIF / PNG / PPM) → (frames [n,h,w,3] u8 BGR, fps).  BsxError with the decoder's reason."""
    w, h, fps, ptr = C.c_int(), C.c_int(), C.c_double(), C.POINTER(C.c_uint8)()
    err = C.create_string_buffer(512)
    n = lib().bsx_media_decode(os.fsencode(path), C.byref(w), C.byref(h), C.byref(fps), C.byref(ptr), err, len(err))
    if n <= 0:
        raise BsxError(err.value.decode(errors="replace") or "media decode failed (%d)" % n)
    try:
        frames = np.ctypeslib.as_array(ptr, (n, h.value, w.value, 3)).copy()
    finally:
        lib().bsx_media_free(ptr)
    return frames, fps.value


class Background:
    """load_background / grab_background of app/background.cc on top of a MaskGen's GPU."""

    def __init__(self, mg: MaskGen, path=None, frames=None, fps=0.0, debug=0):
        self.mg = mg
        if path is not None:
            self.h = lib().bsx_background_load(mg.h, os.fsencode(path), debug)
        else:
            frames = np.ascontiguousarray(frames, np.uint8)
            n, hh, ww, _ = frames.shape
            self.h = lib().bsx_background_from_frames(mg.h, frames.ctypes.data, ww, hh, n, float(fps), debug)
        if not self.h:
            raise BsxError("cannot load background")
        w, h, n, f, v = C.c_int(), C.c_int(), C.c_int(), C.c_double(), C.c_int()
        lib().bsx_background_info(self.h, C.byref(w), C.byref(h), C.byref(n), C.byref(f), C.byref(v))
        self.width, self.height, self.n_frames, self.fps, self.video = w.value, h.value, n.value, f.value, bool(v.value)

    def grab(self, width, height, out=None):
        """→ (frame number, torch u8 cuda [height,width,3])"""
        torch = _torch()
        if out is None:
            out = torch.empty((height, width, 3), dtype=torch.uint8, device="cuda:%d" % self.mg.device)
        frm = lib().bsx_background_grab(self.h, width, height, C.c_void_p(out.data_ptr()), _stream_ptr())
        if frm < 0:
            raise BsxError("bsx_background_grab failed")
        return frm, out

    def close(self):
        if getattr(self, "h", None):
            lib().bsx_background_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def grab_backgrounds(backgrounds, width, height, out=None, at=None):
    """grab_background for a batch of sources in ONE launch (bsx_background_grab_batch): out[i] = the current picture of backgrounds[i] resized to width x height
    — what StreamSetting.bg of stream i points at, grabbed every tick.  backgrounds: Background objects of ONE MaskGen (a source may appear more than once);
    out: cuda uint8 [n,height,width,3] on that MaskGen's device (MaskGen._batch_out; None: a new tensor); at: seconds since the start of playback — every
    animation shows picture floor(at * fps) mod n_frames, the same in every run — or None for the clock, read once for the whole batch.
    → (frame numbers: 1 for a still, picture c of an animation as c + 1; out)"""
    backgrounds = list(backgrounds)
    n, width, height = len(backgrounds), int(width), int(height)
    for i, b in enumerate(backgrounds):
        if not isinstance(b, Background) or not getattr(b, "h", None):
            raise BsxError("backgrounds[%d] is not an open Background" % i)
        if b.mg is not backgrounds[0].mg:
            raise BsxError("backgrounds[%d] belongs to another MaskGen than backgrounds[0]" % i)
    if n == 0:
        if out is None:
            raise BsxError("an empty batch has no MaskGen to allocate `out` on: pass out")
        return [], out
    mg = backgrounds[0].mg
    if n > mg.n_streams:
        raise BsxError("%d backgrounds for a context of %d streams" % (n, mg.n_streams))
    if width <= 0 or height <= 0:
        raise BsxError("output size %d x %d is not positive" % (width, height))
    if at is not None:
        at = float(at)
        if not (0.0 <= at < float("inf")):
            raise BsxError("at = %r must be a time >= 0 (None: the clock)" % at)
    out = mg._batch_out(out, n, width, height)
    arr = (C.c_void_p * n)(*[b.h for b in backgrounds])
    nos = (C.c_int * n)()
    stride = int(out.stride(0)) if n > 1 else width * height * 3
    rc = lib().bsx_background_grab_batch(arr, n, width, height, _ptr(out), stride, -1.0 if at is None else at, nos, _stream_ptr())
    _check(rc, mg.h, "bsx_background_grab_batch")
    return list(nos), out


class Live:
    """CalcMask (app/deepseg.cc:159-286): set_input_frame / get_output_mask around a worker thread."""

    def __init__(self, mg: MaskGen):
        self.mg = mg
        self.h = lib().bsx_live_new(mg.h)
        if not self.h:
            raise BsxError("bsx_live_new failed")

    def set_input_frame(self, frame: np.ndarray):
        if not isinstance(frame, np.ndarray) or frame.dtype != np.uint8 or frame.shape != (self.mg.height, self.mg.width, 3):
            raise BsxError("frame must be uint8 [%d,%d,3]" % (self.mg.height, self.mg.width))
        if frame.strides[2] != 1 or frame.strides[1] != 3:
            frame = np.ascontiguousarray(frame)
        _check(lib().bsx_live_set_input_frame(self.h, frame.ctypes.data, frame.strides[0]), self.mg.h, "bsx_live_set_input_frame")

    def get_output_mask(self, mask: np.ndarray) -> bool:
        if (not isinstance(mask, np.ndarray) or mask.dtype != np.uint8 or mask.shape != (self.mg.height, self.mg.width) or mask.strides[1] != 1
                or mask.strides[0] < self.mg.width or not mask.flags.writeable):
            # the C side writes height rows of width bytes (as process_host does)
            raise BsxError("mask must be a writable uint8 [%d,%d] array with unit inner stride" % (self.mg.height, self.mg.width))
        rc = lib().bsx_live_get_output_mask(self.h, mask.ctypes.data, mask.strides[0])
        if rc < 0:
            _check(rc, self.mg.h, "bsx_live_get_output_mask")
        return rc == 1

    def close(self):
        if getattr(self, "h", None):
            lib().bsx_live_delete(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def model_precompile(path: str, arch: str | None = None) -> str:
    """Host only: emit + compile (hipRTC) the kernel specialised to this model's graph into the code-object cache; returns the note."""
    buf = C.create_string_buffer(1 << 14)
    rc = lib().bsx_model_precompile(os.fsencode(path), arch.encode() if arch else None, buf, len(buf))
    if rc != 0:
        raise BsxError(buf.value.decode(errors="replace"))
    return buf.value.decode()


def model_kernel_source(path: str) -> str:
    """The generated HIP source of the specialised per-frame program ('' when the graph has none)."""
    buf = C.create_string_buffer(1 << 20)
    n = lib().bsx_model_kernel_source(os.fsencode(path), buf, len(buf))
    if n < 0:
        raise BsxError(buf.value.decode(errors="replace"))
    return buf.value.decode() if n > 0 else ""


def model_seg_source(path: str) -> str:
    """The generated HIP source of the graph-specialised segment kernels ('' when the plan has no segment kernels)."""
    buf = C.create_string_buffer(1 << 20)
    n = lib().bsx_model_seg_source(os.fsencode(path), buf, len(buf))
    if n < 0:
        raise BsxError(buf.value.decode(errors="replace"))
    return buf.value.decode() if n > 0 else ""


def gauss_coeff_words(ksize: int, shift: int = 0):
    """(c4 [4][9] u32, c2 [2][17] u32): the coefficient words gauss_blur_k multiplies with (host only, no GPU) — bsx_debug_gauss_coeffs"""
    c4 = np.zeros((4, 9), np.uint32)
    c2 = np.zeros((2, 17), np.uint32)
    _check(lib().bsx_debug_gauss_coeffs(int(ksize), int(shift), c4.ctypes.data_as(C.POINTER(C.c_uint32)), c2.ctypes.data_as(C.POINTER(C.c_uint32))), None,
           "bsx_debug_gauss_coeffs")
    return c4, c2


def model_describe(path: str) -> str:
    """Parse + plan a model on the host only (no GPU needed); raises BsxError with the loader's message."""
    buf = C.create_string_buffer(1 << 16)
    rc = lib().bsx_model_describe(os.fsencode(path), buf, len(buf))
    if rc != 0:
        raise BsxError(buf.value.decode(errors="replace"))
    return buf.value.decode()


# ---- reference-named entry points -----------------------------------------------------------------
def bs_tensorflow_version() -> str:
    return lib().bsx_version().decode()


def bs_maskgen_new(modelname, threads, width, height, ondebug=None, onprep=None, oninfer=None, onmask=None, caller_ctx=None):
    """Returns a context, or None on failure (after a message through ondebug/stderr) — like lib/libbackscrub.cc:161-259."""
    try:
        return MaskGen(modelname, width, height, n_streams=1, threads=threads, ondebug=ondebug, onprep=onprep, oninfer=oninfer,
                       onmask=onmask, caller_ctx=caller_ctx)
    except BsxError:
        return None


def bs_maskgen_delete(context):
    if context is not None:  # NULL-safe like :262
        context.close()


def bs_maskgen_process(context, frame: np.ndarray, mask: np.ndarray) -> bool:
    """frame: BGR uint8 [H,W,3]; mask: uint8 [H,W] written in place.  False on a null context / failure (:280)."""
    if context is None or getattr(context, "h", None) is None:
        return False
    try:
        context.process_host(frame, 0, mask)
        return True
    except BsxError:
        return False


def alpha_blend(srca, srcb, mask, context: MaskGen):
    """GPU alpha_blend (app/deepseg.cc:108-134): srca=background, srcb=frame, mask 255⇒srca. Torch cuda u8 tensors."""
    if srcb.dim() == 3:
        return context.composite(srca, srcb[None], mask[None])[0]
    return context.composite(srca, srcb, mask)
