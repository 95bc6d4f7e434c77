"""ctypes binding of libimagekit_hip.so (the C ABI in include/imagekit_hip.h).

The product path has no CPU fallback: if the HIP library is missing or fails
to load, every call raises.  `load()` builds nothing; run `make -C
rust-image-transform_amd` (or `__graft_entry__.build()`) first.
"""
from __future__ import annotations

import atexit
import ctypes
import os
import threading

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("IK_LIB_PATH") or os.path.join(os.path.dirname(_HERE), "lib", "libimagekit_hip.so")

_lock = threading.Lock()
_lib = None

u8p = ctypes.POINTER(ctypes.c_uint8)
c_img_p = ctypes.c_void_p


class WebpExactItem(ctypes.Structure):
    """ik_webp_exact_item: one image of ik_webp_encode_exact_items."""
    _fields_ = [("dev_yuv", ctypes.c_void_p), ("w", ctypes.c_uint32), ("h", ctypes.c_uint32), ("quality", ctypes.c_int)]


class RequestOpts(ctypes.Structure):
    """ik_request_opts: one request's options for the *_opts entry points (the defaults are
    IK_FIT_CONTAIN, IK_ORIENT_STORED, IK_BG_NONE)."""
    _fields_ = [("fit", ctypes.c_int), ("orient", ctypes.c_int), ("background", ctypes.c_int32)]


class RequestOpts2(ctypes.Structure):
    """ik_request_opts2: RequestOpts' fields, then blur and unsharpen (a sigma of 0 is off)."""
    _fields_ = [("fit", ctypes.c_int), ("orient", ctypes.c_int), ("background", ctypes.c_int32),
                ("blur_sigma", ctypes.c_float), ("sharpen_sigma", ctypes.c_float), ("sharpen_threshold", ctypes.c_int32)]


class RequestOpts3(ctypes.Structure):
    """ik_request_opts3: RequestOpts2's fields, then the watermark (overlay NULL is none)."""
    _fields_ = RequestOpts2._fields_ + [
        ("overlay", ctypes.c_void_p), ("overlay_gravity", ctypes.c_int32), ("overlay_dx", ctypes.c_int32),
        ("overlay_dy", ctypes.c_int32), ("overlay_opacity", ctypes.c_int32), ("overlay_tile", ctypes.c_int32),
        ("reserved", ctypes.c_int32)]


class Adjust(ctypes.Structure):
    """ik_adjust: a colour adjustment (all zero is none)."""
    _fields_ = [("brightness", ctypes.c_int32), ("contrast", ctypes.c_int32), ("saturation", ctypes.c_int32),
                ("hue", ctypes.c_int32), ("gamma", ctypes.c_float), ("invert", ctypes.c_int32)]


class RequestOpts4(ctypes.Structure):
    """ik_request_opts4: RequestOpts3's fields, then the colour adjustment (all zero is none)."""
    _fields_ = RequestOpts3._fields_ + [("adjust", Adjust)]


class Pad(ctypes.Structure):
    """ik_pad: the output extended onto a canvas (mode 0 is none, and then all zero)."""
    _fields_ = [("mode", ctypes.c_int32), ("gravity", ctypes.c_int32), ("width", ctypes.c_int32),
                ("height", ctypes.c_int32), ("color", ctypes.c_int32), ("alpha", ctypes.c_int32)]


class RequestOpts5(ctypes.Structure):
    """ik_request_opts5: RequestOpts4's fields, then the pad (all zero is none)."""
    _fields_ = RequestOpts4._fields_ + [("pad", Pad)]


_opts_p = ctypes.c_void_p  # any declared layout (const void *opts, with its size)
_batch_head = [ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_size_t), ctypes.c_uint32,
               ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int64)]
_batch_opts = (_batch_head + [_opts_p, ctypes.c_size_t] + [ctypes.POINTER(ctypes.c_int)] * 2 + [ctypes.c_int, ctypes.c_int]
               + [ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_size_t), ctypes.POINTER(ctypes.c_int)])

# (name, restype, argtypes) for every entry point declared in include/imagekit_hip.h
SIGNATURES = [
    ("ik_init", ctypes.c_int, [ctypes.c_int]),
    ("ik_shutdown", ctypes.c_int, []),
    ("ik_close", ctypes.c_int, []),
    ("ik_memory_stats", ctypes.c_int, [ctypes.POINTER(ctypes.c_uint64), ctypes.c_int]),
    ("ik_device_count", ctypes.c_int, []),
    ("ik_init_devices", ctypes.c_int, [ctypes.POINTER(ctypes.c_int), ctypes.c_int]),
    ("ik_logical_device_count", ctypes.c_int, []),
    ("ik_logical_device_stats", ctypes.c_int, [ctypes.c_uint32, ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint64)]),
    ("ik_request_cost", ctypes.c_uint64, [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_int64, ctypes.c_int64, ctypes.c_int]),
    ("ik_schedule_plan", None, [ctypes.POINTER(ctypes.c_uint64), ctypes.c_uint32, ctypes.c_uint32, ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint32)]),
    ("ik_schedule_split", ctypes.c_uint32, [ctypes.POINTER(ctypes.c_uint64), ctypes.c_uint32, ctypes.c_uint32, ctypes.POINTER(ctypes.c_uint64), ctypes.c_uint32, ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint32)]),
    ("ik_post_plan", ctypes.c_int,
     [ctypes.c_uint32, ctypes.POINTER(ctypes.c_int)] + [ctypes.POINTER(ctypes.c_uint32)] * 3
     + [ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_uint32)]
     + [ctypes.POINTER(ctypes.c_int64)] * 2 + [ctypes.POINTER(ctypes.c_int)] * 2 + [ctypes.c_int, ctypes.c_int]
     + [ctypes.POINTER(ctypes.c_uint32)] * 2 + [ctypes.POINTER(ctypes.c_int)] * 3 + [ctypes.POINTER(ctypes.c_uint32)]),
    ("ik_last_error", ctypes.c_size_t, [ctypes.c_char_p, ctypes.c_size_t]),
    ("ik_version", ctypes.c_char_p, []),
    ("ik_host_alloc", ctypes.c_int, [ctypes.c_size_t, ctypes.POINTER(ctypes.c_void_p)]),
    ("ik_host_free", ctypes.c_int, [ctypes.c_void_p]),
    ("ik_host_register", ctypes.c_int, [ctypes.c_void_p, ctypes.c_size_t]),
    ("ik_host_unregister", ctypes.c_int, [ctypes.c_void_p]),
    ("ik_image_from_host", ctypes.c_int, [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, ctypes.POINTER(c_img_p)]),
    ("ik_image_wrap_device", ctypes.c_int, [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_size_t, ctypes.POINTER(c_img_p)]),
    ("ik_image_info", ctypes.c_int, [c_img_p, ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint32)]),
    ("ik_image_to_host", ctypes.c_int, [c_img_p, ctypes.c_void_p, ctypes.c_size_t]),
    ("ik_image_depth", ctypes.c_int, [c_img_p]),
    ("ik_image_from_host16", ctypes.c_int, [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, ctypes.POINTER(c_img_p)]),
    ("ik_image_free", None, [c_img_p]),
    ("ik_buf_free", None, [ctypes.c_void_p]),
    ("ik_decode", ctypes.c_int, [ctypes.c_char_p, ctypes.c_size_t, ctypes.POINTER(c_img_p), ctypes.POINTER(ctypes.c_int)]),
    ("ik_resize", ctypes.c_int, [c_img_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_int, ctypes.POINTER(c_img_p)]),
    ("ik_resize_exact", ctypes.c_int, [c_img_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_int, ctypes.POINTER(c_img_p)]),
    ("ik_encode", ctypes.c_int, [c_img_p, ctypes.c_int, ctypes.c_int, ctypes.POINTER(u8p), ctypes.POINTER(ctypes.c_size_t)]),
    ("ik_transform", ctypes.c_int, [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_int64, ctypes.c_int64, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.POINTER(u8p), ctypes.POINTER(ctypes.c_size_t)]),
    ("ik_set_webp_encoder", ctypes.c_int, [ctypes.c_int]),
    ("ik_libwebp_version", ctypes.c_int, []),
    ("ik_codec_library", ctypes.c_size_t, [ctypes.c_int, ctypes.c_char_p, ctypes.c_size_t]),
    ("ik_get_webp_encoder", ctypes.c_int, []),
    ("ik_pipeline_set_webp_encoder", ctypes.c_int, [ctypes.c_void_p, ctypes.c_int]),
    ("ik_webp_encode_exact_device", ctypes.c_int, [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]),
    ("ik_webp_encode_exact_items", ctypes.c_int, [ctypes.POINTER(WebpExactItem), ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p]),
    ("ik_webp_exact_plan", ctypes.c_longlong, [ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint32), ctypes.c_uint32, ctypes.POINTER(ctypes.c_uint64), ctypes.c_size_t, ctypes.POINTER(ctypes.c_uint32)]),
    ("ik_set_webp_mixed", ctypes.c_int, [ctypes.c_int]),
    ("ik_get_webp_mixed", ctypes.c_int, []),
    ("ik_webp_enc_counters", ctypes.c_int, [ctypes.POINTER(ctypes.c_ulonglong)]),
    ("ik_vp8_analyze_device", ctypes.c_int, [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_float, ctypes.c_void_p, ctypes.c_void_p]),
    ("ik_pipeline_create", ctypes.c_int, [ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_uint32, ctypes.c_int, ctypes.POINTER(ctypes.c_void_p)]),
    ("ik_pipeline_run", ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_size_t, ctypes.POINTER(ctypes.c_size_t)]),
    ("ik_decode_batch", ctypes.c_int, [ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_size_t), ctypes.c_uint32, ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int)]),
    ("ik_transform_batch", ctypes.c_int, [ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_size_t), ctypes.c_uint32, ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int), ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_size_t), ctypes.POINTER(ctypes.c_int)]),
    ("ik_transform_batch_submit", ctypes.c_int, [ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_size_t), ctypes.c_uint32, ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int), ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_size_t), ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_uint64)]),
    ("ik_transform_batch_submit_device", ctypes.c_int, [ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_size_t), ctypes.c_uint32, ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int), ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_size_t), ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_uint64)]),
    ("ik_transform_batch_wait", ctypes.c_int, [ctypes.c_uint64]),
    ("ik_set_resize_mode", ctypes.c_int, [ctypes.c_int]),
    ("ik_set_png_gpu_min", ctypes.c_int, [ctypes.c_longlong]),
    ("ik_png_last_timing", ctypes.c_int, [ctypes.POINTER(ctypes.c_double), ctypes.c_int]),
    ("ik_batch_last_timing", ctypes.c_int, [ctypes.POINTER(ctypes.c_double), ctypes.c_int]),
    ("ik_png_counters", ctypes.c_int, [ctypes.POINTER(ctypes.c_ulonglong)]),
    ("ik_png_adam7_plan", ctypes.c_int, [ctypes.c_uint32, ctypes.c_uint32, ctypes.c_int, ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint64)]),
    ("ik_webp_counters", ctypes.c_int, [ctypes.POINTER(ctypes.c_ulonglong)]),
    ("ik_webp_last_timing", ctypes.c_int, [ctypes.POINTER(ctypes.c_double), ctypes.c_int]),
    ("ik_webp_gpu_min_batch_pixels", ctypes.c_ulonglong, []),
    ("ik_set_webp_alpha_decode", ctypes.c_int, [ctypes.c_int]),
    ("ik_get_webp_alpha_decode", ctypes.c_int, []),
    ("ik_webp_alpha_plane", ctypes.c_int, [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t, ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int)]),
    ("ik_webp_batch_plan", ctypes.c_int, [ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint64), ctypes.c_uint32, ctypes.c_uint64, ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint32)]),
    ("ik_jpeg_counters", ctypes.c_int, [ctypes.POINTER(ctypes.c_ulonglong)]),
    ("ik_jpeg_device_counters", ctypes.c_int, [ctypes.POINTER(ctypes.c_ulonglong)]),
    ("ik_jpeg_device_walk_ms", ctypes.c_double, []),
    ("ik_set_jpeg_device", ctypes.c_int, [ctypes.c_int]),
    ("ik_get_jpeg_device", ctypes.c_int, []),
    ("ik_set_jpeg_prog_free", ctypes.c_int, [ctypes.c_int]),
    ("ik_get_jpeg_prog_free", ctypes.c_int, []),
    ("ik_jpeg_prog_free_ms", ctypes.c_int, [ctypes.POINTER(ctypes.c_double)]),
    ("ik_jpeg_walk_host", ctypes.c_int, [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]),
    ("ik_get_resize_mode", ctypes.c_int, []),
    ("ik_resize_kernel_name", ctypes.c_char_p, [ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_int]),
    ("ik_resize_plan_info", ctypes.c_int, [ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_int, ctypes.c_uint32, ctypes.POINTER(ctypes.c_int32), ctypes.c_int]),
    ("ik_set_jpeg_reconstruction", ctypes.c_int, [ctypes.c_int]),
    ("ik_get_jpeg_reconstruction", ctypes.c_int, []),
    ("ik_pipeline_submit", ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_uint32]),
    ("ik_pipeline_collect", ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.POINTER(ctypes.c_size_t), ctypes.POINTER(ctypes.c_uint32)]),
    ("ik_pipeline_run_device", ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_uint32]),
    ("ik_pipeline_kernel_ms", ctypes.c_double, [ctypes.c_void_p, ctypes.c_int]),
    ("ik_pipeline_fetch_resized", ctypes.c_int, [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_size_t]),
    ("ik_pipeline_destroy", None, [ctypes.c_void_p]),
    ("ik_resize_batch_device", ctypes.c_int, [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_void_p]),
    ("ik_webp_yuv420_device", ctypes.c_int, [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p]),
    ("ik_avif_yuv444_device", ctypes.c_int, [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p]),
    ("ik_jpeg_coeffs_device", ctypes.c_int, [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]),
    ("ik_jpeg_enc_capacity", ctypes.c_size_t, [ctypes.c_uint32, ctypes.c_uint32]),
    ("ik_jpeg_huffman_device", ctypes.c_int, [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p]),
    ("ik_jpeg_enc_counters", ctypes.c_int, [ctypes.POINTER(ctypes.c_ulonglong)]),
    ("ik_dev_alloc", ctypes.c_int, [ctypes.c_size_t, ctypes.POINTER(ctypes.c_void_p)]),
    ("ik_dev_free", ctypes.c_int, [ctypes.c_void_p]),
    ("ik_memcpy_h2d", ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t]),
    ("ik_memcpy_d2h", ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t]),
    ("ik_dev_synchronize", ctypes.c_int, []),
    ("ik_fit_target", ctypes.c_int, [ctypes.c_uint32, ctypes.c_uint32, ctypes.c_int64, ctypes.c_int64, ctypes.c_int, ctypes.POINTER(ctypes.c_uint32)]),
    ("ik_resize_fit", ctypes.c_int, [c_img_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_int, ctypes.c_int, ctypes.POINTER(c_img_p)]),
    ("ik_resize_window", ctypes.c_int, [c_img_p] + [ctypes.c_uint32] * 6 + [ctypes.c_int, ctypes.POINTER(c_img_p)]),
    ("ik_resize_window_batch_device", ctypes.c_int, [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_uint32] + [ctypes.c_uint32] * 6 + [ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_void_p]),
    ("ik_resize_plan_info_window", ctypes.c_int, [ctypes.c_uint32] * 9 + [ctypes.c_int, ctypes.c_uint32, ctypes.POINTER(ctypes.c_int32), ctypes.c_int]),
    ("ik_transform_fit", ctypes.c_int, [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_int64, ctypes.c_int64, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.POINTER(u8p), ctypes.POINTER(ctypes.c_size_t)]),
    ("ik_transform_batch_fit", ctypes.c_int, [ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_size_t), ctypes.c_uint32, ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int), ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_size_t), ctypes.POINTER(ctypes.c_int)]),
    ("ik_transform_batch_submit_fit", ctypes.c_int, [ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_size_t), ctypes.c_uint32, ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int), ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_size_t), ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_uint64)]),
    ("ik_post_plan_fit", ctypes.c_int,
     [ctypes.c_uint32, ctypes.POINTER(ctypes.c_int)] + [ctypes.POINTER(ctypes.c_uint32)] * 3
     + [ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_uint32)]
     + [ctypes.POINTER(ctypes.c_int64)] * 2 + [ctypes.POINTER(ctypes.c_int)] * 3 + [ctypes.c_int, ctypes.c_int]
     + [ctypes.POINTER(ctypes.c_uint32)] * 2 + [ctypes.POINTER(ctypes.c_int)] * 3 + [ctypes.POINTER(ctypes.c_uint32)] * 2),
    ("ik_exif_orientation", ctypes.c_int, [ctypes.c_char_p, ctypes.c_size_t]),
    ("ik_orient_tile", ctypes.c_int, []),
    ("ik_orient_strip", ctypes.c_int, []),
    ("ik_image_orient", ctypes.c_int, [c_img_p, ctypes.c_int, ctypes.POINTER(c_img_p)]),
    ("ik_decode_oriented", ctypes.c_int, [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_int, ctypes.POINTER(c_img_p), ctypes.POINTER(ctypes.c_int)]),
    ("ik_orient_batch_device", ctypes.c_int, [ctypes.c_void_p] + [ctypes.c_uint32] * 4 + [ctypes.c_size_t, ctypes.c_size_t, ctypes.c_uint32, ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_void_p]),
    ("ik_transform_oriented", ctypes.c_int, [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_int64, ctypes.c_int64] + [ctypes.c_int] * 5 + [ctypes.POINTER(u8p), ctypes.POINTER(ctypes.c_size_t)]),
    ("ik_transform_batch_oriented", ctypes.c_int, [ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_size_t), ctypes.c_uint32, ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int64)] + [ctypes.POINTER(ctypes.c_int)] * 4 + [ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_size_t), ctypes.POINTER(ctypes.c_int)]),
    ("ik_transform_batch_submit_oriented", ctypes.c_int, [ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_size_t), ctypes.c_uint32, ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int64)] + [ctypes.POINTER(ctypes.c_int)] * 4 + [ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_size_t), ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_uint64)]),
    ("ik_flatten_span", ctypes.c_int, []),
    ("ik_flatten_row_cap", ctypes.c_int, []),
    ("ik_flatten_counters", ctypes.c_int, [ctypes.POINTER(ctypes.c_ulonglong)]),
    ("ik_image_flatten", ctypes.c_int, [c_img_p, ctypes.c_int32, ctypes.POINTER(c_img_p)]),
    ("ik_flatten_batch_device", ctypes.c_int, [ctypes.c_void_p] + [ctypes.c_uint32] * 4 + [ctypes.c_size_t, ctypes.c_size_t, ctypes.c_uint32, ctypes.c_int32, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_void_p]),
    ("ik_blur_axis_plan", ctypes.c_int, [ctypes.c_uint32, ctypes.c_float, ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_float), ctypes.c_uint32, ctypes.POINTER(ctypes.c_uint32)]),
    ("ik_image_blur", ctypes.c_int, [c_img_p, ctypes.c_float, ctypes.POINTER(c_img_p)]),
    ("ik_image_unsharpen", ctypes.c_int, [c_img_p, ctypes.c_float, ctypes.c_int32, ctypes.POINTER(c_img_p)]),
    ("ik_blur_tile", ctypes.c_int, [ctypes.POINTER(ctypes.c_int)]),
    ("ik_blur_counters", ctypes.c_int, [ctypes.POINTER(ctypes.c_ulonglong)]),
    ("ik_blur_batch_device", ctypes.c_int, [ctypes.c_void_p] + [ctypes.c_uint32] * 4 + [ctypes.c_size_t, ctypes.c_size_t, ctypes.c_uint32, ctypes.c_float, ctypes.c_int, ctypes.c_int32, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_void_p]),
    ("ik_overlay_place", ctypes.c_int, [ctypes.c_uint32] * 4 + [ctypes.c_int, ctypes.c_int32, ctypes.c_int32, ctypes.c_int, ctypes.POINTER(ctypes.c_int32)]),
    ("ik_image_overlay", ctypes.c_int, [c_img_p, c_img_p, ctypes.c_int, ctypes.c_int32, ctypes.c_int32, ctypes.c_int, ctypes.c_int, ctypes.POINTER(c_img_p)]),
    ("ik_overlay_span", ctypes.c_int, []),
    ("ik_overlay_counters", ctypes.c_int, [ctypes.POINTER(ctypes.c_ulonglong)]),
    ("ik_overlay_batch_device", ctypes.c_int, [ctypes.c_void_p] + [ctypes.c_uint32] * 4 + [ctypes.c_size_t, ctypes.c_size_t, ctypes.c_uint32, ctypes.c_void_p] + [ctypes.c_uint32] * 4 + [ctypes.c_size_t, ctypes.c_int, ctypes.c_int32, ctypes.c_int32, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]),
    ("ik_adjust_plan", ctypes.c_int, [ctypes.POINTER(Adjust), ctypes.c_int, ctypes.POINTER(ctypes.c_uint16), ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int)]),
    ("ik_image_adjust", ctypes.c_int, [c_img_p, ctypes.POINTER(Adjust), ctypes.POINTER(c_img_p)]),
    ("ik_adjust_span", ctypes.c_int, []),
    ("ik_adjust_counters", ctypes.c_int, [ctypes.POINTER(ctypes.c_ulonglong)]),
    ("ik_adjust_batch_device", ctypes.c_int, [ctypes.c_void_p] + [ctypes.c_uint32] * 4 + [ctypes.c_size_t, ctypes.c_size_t, ctypes.c_uint32, ctypes.POINTER(Adjust), ctypes.c_void_p]),
    ("ik_pad_place", ctypes.c_int, [ctypes.c_uint32] * 4 + [ctypes.c_int, ctypes.POINTER(ctypes.c_int32)]),
    ("ik_image_pad", ctypes.c_int, [c_img_p, ctypes.POINTER(Pad), ctypes.POINTER(c_img_p)]),
    ("ik_pad_span", ctypes.c_int, []),
    ("ik_pad_row_cap", ctypes.c_int, []),
    ("ik_pad_counters", ctypes.c_int, [ctypes.POINTER(ctypes.c_ulonglong)]),
    ("ik_pad_batch_device", ctypes.c_int, [ctypes.c_void_p] + [ctypes.c_uint32] * 4 + [ctypes.c_size_t, ctypes.c_size_t, ctypes.c_uint32, ctypes.POINTER(Pad), ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_void_p]),
    ("ik_transform_opts", ctypes.c_int, [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_int64, ctypes.c_int64] + [ctypes.c_int] * 3 + [_opts_p, ctypes.c_size_t, ctypes.POINTER(u8p), ctypes.POINTER(ctypes.c_size_t)]),
    ("ik_transform_batch_opts", ctypes.c_int, _batch_opts),
    ("ik_transform_batch_submit_opts", ctypes.c_int, _batch_opts + [ctypes.POINTER(ctypes.c_uint64)]),
    ("ik_transform_batch_submit_device_opts", ctypes.c_int, _batch_opts + [ctypes.POINTER(ctypes.c_uint64)]),
]


class LibraryMissing(RuntimeError):
    pass


def load() -> ctypes.CDLL:
    """Load (once) and return the HIP library; raise if it is not built."""
    global _lib
    with _lock:
        if _lib is not None:
            return _lib
        if not os.path.exists(LIB_PATH):
            raise LibraryMissing(
                f"{LIB_PATH} not found: build it with `make -C rust-image-transform_amd` "
                "(there is no CPU fallback)")
        lib = ctypes.CDLL(LIB_PATH)
        for name, res, args in SIGNATURES:
            fn = getattr(lib, name)
            fn.restype = res
            fn.argtypes = args
        _lib = lib
        # orderly teardown while the HIP runtime is alive (ik_close: callers still
        # inside the library return first, the worker and stage threads end,
        # streams and arenas are released, later calls fail instead of bringing
        # the library back up under daemon threads), not in destructors during
        # process exit
        atexit.register(lib.ik_close)
        return lib


def last_error() -> str:
    lib = load()
    buf = ctypes.create_string_buffer(1024)
    lib.ik_last_error(buf, len(buf))
    return buf.value.decode("utf-8", "replace")
