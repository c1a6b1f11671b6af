"""ctypes binding of libmijpeg.so (include/mijpeg.h) for tests and bench.py.

The product is the C ABI; this module only marshals numpy buffers across it.
There is deliberately no CPU fallback: if the HIP library is missing or no
GPU is visible, every call raises.
"""
from __future__ import annotations

import ctypes as C
import math
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
# MIJ_LIB: alternative build of the same library (A/B timing runs, scripts/ab.sh)
LIB_PATH = os.environ.get("MIJ_LIB") or os.path.join(HERE, "libmijpeg.so")

EXPORTS = [
    # drop-in (reference include/encoder.h:10-12)
    "rgb_to_dct", "init_huffman", "write_jpg",
    # extensions
    "mij_set_input_stride", "mij_set_quality", "mij_last_error", "mij_strerror", "mij_last_message",
    "mij_max_jpg_bytes", "mij_encode",
    "mij_batch_create", "mij_batch_destroy", "mij_batch_upload", "mij_batch_set_input",
    "mij_batch_encode", "mij_batch_keep_coefs", "mij_batch_set_split", "mij_batch_set_overlap", "mij_batch_set_option", "mij_batch_get_option", "mij_batch_dct", "mij_batch_pattern_floor", "mij_batch_sync", "mij_batch_output",
    "mij_batch_lengths", "mij_batch_coefs", "mij_batch_tables", "mij_batch_set_timing",
    "mij_batch_stage_ms", "mij_batch_stage_history", "mij_batch_token_count", "mij_batch_geometry", "mij_batch_replays", "mij_batch_stream", "mij_batch_set_stream", "mij_batch_audit", "mij_batch_build_tables",
    "mij_band_analyze", "mij_band_histograms", "mij_band_tables", "mij_band_pack", "mij_band_words",
    "mij_assemble_begin", "mij_assemble_words", "mij_assemble_end",
    "mij_band_words_all", "mij_assemble_pieces", "mij_assembler_create",
    "mij_band_analyze_async", "mij_band_histograms_async", "mij_band_tables_async", "mij_band_pack_async",
    "mij_band_words_async", "mij_assemble_tables_async", "mij_assemble_async",
    "mij_band_stuff_async", "mij_assemble_stuffed_async", "mij_copy_to_host_async",
    "mij_probe_mfma", "mij_colour_lut", "mij_build_target",
    # change detector (reference include/brain.h:7-10 drop-in + extensions)
    "subsample", "store", "compare", "enlargeAdjust", "mij_set_frame_height",
    "mij_decoder_create", "mij_decoder_destroy", "mij_decoder_decode", "mij_decoder_info",
    "mij_decoder_coefs", "mij_decoder_device_coefs", "mij_decoder_passes",
    "mij_decoder_accept", "mij_decoder_scan_info", "mij_loader_accept", "mij_jpeg_size",
    "mij_decoder_reconstruct", "mij_decoder_pixels", "mij_decoder_planes", "mij_decoder_device_pixels",
    "mij_decoder_reconstruct_ms", "mij_decoder_stream", "mij_decode",
    "mij_decoder_layout", "mij_decoder_component", "mij_decoder_plane",
    "mij_detector_create", "mij_detector_destroy", "mij_detector_subsample", "mij_detector_compare",
    "mij_detector_step", "mij_detector_launch", "mij_detector_store", "mij_detector_upload", "mij_detector_get_plane",
    "mij_detector_set_plane", "mij_detector_mask", "mij_detector_stream",
    "mij_batch_set_rgb", "mij_ppm_header", "mij_ppm_read",
    "mij_stream_create", "mij_stream_destroy", "mij_stream_encode_files",
    "mij_stream_encode_frames", "mij_stream_stats",
    "mij_batch_set_frame_dims", "mij_batch_gather_regions", "mij_batch_upload_regions",
    "mij_encode_regions",
    "mij_max_jpg_bytes_any", "mij_batch_pad_input", "mij_batch_upload_any", "mij_batch_encode_interleaved",
    "mij_encode_any",
    "mij_decoder_transcode", "mij_decoder_transcoded", "mij_decoder_device_transcoded", "mij_decoder_transcode_ms",
    "mij_transcode", "mij_decoder_output", "mij_transcode_progressive",
    "mij_decoder_transform", "mij_transform", "mij_exif_orientation", "mij_orientation_op",
    "mij_decoder_reconstruct_scaled", "mij_decoder_scaled_layout", "mij_decode_scaled",
    "mij_max_jpg_bytes_sampled", "mij_batch_encode_sampled", "mij_batch_sampled_component",
    "mij_batch_sampled_layout", "mij_encode_sampled",
    "mij_resizer_create", "mij_resizer_destroy", "mij_resizer_resize", "mij_resizer_device_pixels", "mij_resizer_pixels",
    "mij_resizer_ms", "mij_resizer_stream", "mij_resizer_set_stream", "mij_resize", "mij_thumbnail",
    "mij_thumbnail_denom",
    "mij_libjpeg_tables", "mij_batch_encode_libjpeg", "mij_encode_libjpeg", "mij_thumbnail_libjpeg",
    "mij_tensorizer_create", "mij_tensorizer_destroy", "mij_tensorizer_run", "mij_tensor_bytes", "mij_tensorizer_device",
    "mij_tensorizer_read", "mij_tensorizer_ms", "mij_tensorizer_stream", "mij_tensorizer_set_stream",
    "mij_loader_create", "mij_loader_destroy", "mij_loader_load", "mij_loader_denom", "mij_loader_device",
    "mij_loader_read", "mij_loader_ms", "mij_loader_stream",
]


class Huff(C.Structure):
    """huff_code (reference include/structs.h:5-13)."""
    _fields_ = [
        ("sym_freq", C.c_int * 257),
        ("code_len", C.c_int * 257),
        ("next", C.c_int * 257),
        ("code_len_freq", C.c_int * 32),
        ("sym_sorted", C.c_int * 256),
        ("sym_code_len", C.c_int * 256),
        ("sym_code", C.c_int * 256),
    ]


class Area(C.Structure):
    """area_t (reference include/structs.h:15-18)."""
    _fields_ = [("x", C.c_int), ("y", C.c_int), ("w", C.c_int), ("h", C.c_int)]


class MijError(RuntimeError):
    pass


# mij_batch_set_option (include/mijpeg.h: MIJ_OPT_*)
OPTIONS = {"seam": 0, "ff_pack": 1, "actab": 2, "segdc_fused": 3, "pack_wide": 4, "emit_slots": 5,
           "overlap_prio": 6, "pack_segs": 8}


# mij_test_last_plan (csrc/mij_testing.h: MIJ_PLAN_*), in the library's order
PLAN_FIELDS = ["nframes", "f0", "entropy_calls", "dc_last", "actab", "tables", "segdc", "seam", "ff_pack",
               "seam_in_scan", "emit_slots", "pack_ls_luma", "pack_ls_chroma", "pack_wide",
               "hist_fill_skipped", "k1_mode", "dc_only"]


_lib = None


def load() -> C.CDLL:
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise MijError(f"{LIB_PATH} missing: build it with `make -C {HERE}` "
                       "(there is no CPU fallback)")
    lib = C.CDLL(LIB_PATH)
    p, i, sz = C.c_void_p, C.c_int, C.c_size_t
    lib.rgb_to_dct.argtypes = [p, p, p, p, Area]
    lib.rgb_to_dct.restype = None
    lib.init_huffman.argtypes = [p, p, p, Area, p, p]
    lib.init_huffman.restype = None
    lib.write_jpg.argtypes = [p, p, p, p, p, Area, p, p]
    lib.write_jpg.restype = sz
    lib.mij_set_input_stride.argtypes = [i]
    lib.mij_set_quality.argtypes = [i]
    lib.mij_last_error.restype = i
    lib.mij_strerror.restype = C.c_char_p
    lib.mij_strerror.argtypes = [i]
    lib.mij_last_message.restype = C.c_char_p
    lib.mij_last_message.argtypes = []
    lib.mij_max_jpg_bytes.restype = sz
    lib.mij_max_jpg_bytes.argtypes = [i, i]
    lib.mij_encode.argtypes = [p, i, Area, i, p, sz, C.POINTER(sz)]
    lib.mij_batch_create.restype = p
    lib.mij_batch_create.argtypes = [i, i, i, i, i]
    lib.mij_batch_destroy.argtypes = [p]
    lib.mij_batch_destroy.restype = None
    lib.mij_batch_upload.argtypes = [p, p, i, i]
    lib.mij_batch_set_input.argtypes = [p, p, C.c_longlong, i]
    lib.mij_batch_encode.argtypes = [p, i]
    lib.mij_batch_keep_coefs.argtypes = [p, i]
    lib.mij_batch_set_split.argtypes = [p, i]
    lib.mij_batch_set_overlap.argtypes = [p, i]
    lib.mij_batch_set_option.argtypes = [p, i, i]
    lib.mij_batch_get_option.argtypes = [p, i]
    lib.mij_batch_dct.argtypes = [p, i]
    lib.mij_batch_pattern_floor.argtypes = [p, i]
    lib.mij_batch_audit.argtypes = [p, i, p]
    lib.mij_band_analyze_async.argtypes = [p, i, p]
    lib.mij_band_histograms_async.argtypes = [p, i, p, p]
    lib.mij_band_tables_async.argtypes = [p, i, p, p]
    lib.mij_band_pack_async.argtypes = [p, i, p]
    lib.mij_band_words_async.argtypes = [p, i, p, sz]
    lib.mij_assemble_tables_async.argtypes = [p, i, p]
    lib.mij_assemble_async.argtypes = [p, i, p, i, p, sz]
    lib.mij_band_stuff_async.argtypes = [p, i, p, i, i, p, p, p, sz]
    lib.mij_assemble_stuffed_async.argtypes = [p, i, p, i, p, sz]
    lib.mij_copy_to_host_async.argtypes = [p, p, p, sz]
    lib.mij_batch_build_tables.argtypes = [p, i, p]
    lib.mij_batch_sync.argtypes = [p]
    lib.mij_batch_output.argtypes = [p, i, p, sz, C.POINTER(sz)]
    lib.mij_batch_lengths.argtypes = [p, C.POINTER(sz), i]
    lib.mij_batch_coefs.argtypes = [p, i, p, p, p, i]
    lib.mij_batch_tables.argtypes = [p, i, p]
    lib.mij_batch_set_timing.argtypes = [p, i]
    lib.mij_batch_stage_ms.argtypes = [p, p, i]
    lib.mij_batch_stage_history.argtypes = [p, p, i]
    lib.mij_batch_token_count.restype = C.c_ulonglong
    lib.mij_batch_token_count.argtypes = [p, i]
    lib.mij_batch_geometry.argtypes = [p, p, i]
    lib.mij_batch_replays.restype = C.c_ulonglong
    lib.mij_batch_replays.argtypes = [p]
    lib.mij_batch_stream.restype = p
    lib.mij_batch_stream.argtypes = [p]
    lib.mij_batch_set_stream.argtypes = [p, p]
    u64 = C.c_ulonglong
    lib.mij_band_analyze.argtypes = [p, i, p]
    lib.mij_band_histograms.argtypes = [p, i, p, p]
    lib.mij_band_tables.argtypes = [p, i, p, p]
    lib.mij_band_pack.argtypes = [p, i, p, p]
    lib.mij_band_words.argtypes = [p, i, i, p, C.c_size_t, i]
    lib.mij_assemble_begin.argtypes = [p, i, p]
    lib.mij_assemble_words.argtypes = [p, i, i, u64, p, C.c_size_t, i]
    lib.mij_assemble_end.argtypes = [p, i, p]
    lib.mij_band_words_all.argtypes = [p, i, p, C.c_size_t, i]
    lib.mij_assemble_pieces.argtypes = [p, p, C.c_size_t, i, p, i]
    lib.mij_assembler_create.restype = p
    lib.mij_assembler_create.argtypes = [i, i, i, i, i]
    lib.mij_probe_mfma.argtypes = [p, p, p]
    lib.mij_colour_lut.argtypes = [p]
    lib.mij_build_target.restype = C.c_char_p
    lib.mij_batch_set_rgb.argtypes = [p, i]
    lib.mij_ppm_header.argtypes = [C.c_char_p, C.POINTER(i), C.POINTER(i), C.POINTER(C.c_longlong)]
    lib.mij_ppm_read.argtypes = [C.c_char_p, p, sz, i, i]
    lib.mij_stream_create.restype = p
    lib.mij_stream_create.argtypes = [i, i, i, i, i, i]
    lib.mij_stream_destroy.argtypes = [p]
    lib.mij_stream_destroy.restype = None
    lib.mij_stream_encode_files.argtypes = [p, C.POINTER(C.c_char_p), C.POINTER(C.c_char_p), i,
                                            C.POINTER(i)]
    lib.mij_stream_encode_frames.argtypes = [p, C.POINTER(p), i, C.POINTER(p), C.POINTER(sz),
                                             C.POINTER(sz)]
    lib.mij_stream_stats.argtypes = [p, p, i]
    try:
        lib.mij_detector_create.restype = p
        lib.mij_detector_create.argtypes = [i, i, i]
        lib.mij_detector_destroy.argtypes = [p]
        lib.mij_detector_subsample.argtypes = [p, p, C.c_longlong]
        lib.mij_detector_compare.argtypes = [p, p, C.POINTER(i)]
        lib.mij_detector_step.argtypes = [p, p, C.c_longlong, p, C.POINTER(i)]
        lib.mij_detector_store.argtypes = [p]
        lib.mij_detector_launch.argtypes = [p, p, C.c_longlong]
        lib.mij_detector_upload.argtypes = [p, p, C.c_longlong, C.POINTER(p)]
        lib.mij_detector_get_plane.argtypes = [p, i, p]
        lib.mij_detector_set_plane.argtypes = [p, i, p]
        lib.mij_detector_mask.argtypes = [p, p, sz, C.POINTER(i)]
        lib.mij_detector_stream.restype = p
        lib.mij_detector_stream.argtypes = [p]
        lib.mij_set_frame_height.argtypes = [i]
        lib.mij_decoder_create.restype = p
        lib.mij_decoder_create.argtypes = [i, i, i, i]
        lib.mij_decoder_destroy.argtypes = [p]
        lib.mij_decoder_decode.argtypes = [p, C.POINTER(p), C.POINTER(sz), i]
        lib.mij_decoder_info.argtypes = [p, i, C.POINTER(i), C.POINTER(i), p]
        lib.mij_decoder_coefs.argtypes = [p, i, p, p, p]
        lib.mij_decoder_device_coefs.restype = p
        lib.mij_decoder_device_coefs.argtypes = [p, i]
        lib.mij_decoder_passes.argtypes = [p]
        lib.mij_decoder_reconstruct.argtypes = [p, i]
        lib.mij_decoder_pixels.argtypes = [p, i, p, sz, C.c_longlong]
        lib.mij_decoder_planes.argtypes = [p, i, p, p, p]
        lib.mij_decoder_device_pixels.restype = p
        lib.mij_decoder_device_pixels.argtypes = [p, i, C.POINTER(C.c_longlong)]
        lib.mij_decoder_reconstruct_ms.argtypes = [p, p]
        lib.mij_decoder_stream.restype = p
        lib.mij_decoder_stream.argtypes = [p]
        lib.mij_decode.argtypes = [p, sz, i, p, sz, C.POINTER(i), C.POINTER(i)]
        lib.subsample.restype = None
        lib.subsample.argtypes = [p, p, p]
        lib.store.restype = None
        lib.store.argtypes = [p, p]
        lib.compare.restype = C.c_uint8
        lib.compare.argtypes = [p, p, p, p]
        lib.enlargeAdjust.restype = None
        lib.enlargeAdjust.argtypes = [p]
        lib.mij_batch_set_frame_dims.argtypes = [p, p, i]
        lib.mij_batch_gather_regions.argtypes = [p, p, C.c_longlong, i, i, p, i]
        lib.mij_batch_upload_regions.argtypes = [p, p, i, i, p, i]
        lib.mij_encode_regions.argtypes = [p, i, i, p, i, i, p, sz, p]
        lib.mij_decoder_layout.argtypes = [p, i, p, i]
        lib.mij_decoder_component.argtypes = [p, i, i, p, sz]
        lib.mij_decoder_plane.argtypes = [p, i, i, p, sz]
        lib.mij_max_jpg_bytes_any.restype = sz
        lib.mij_max_jpg_bytes_any.argtypes = [i, i, i]
        lib.mij_batch_pad_input.argtypes = [p, p, C.c_longlong, C.c_longlong, p, i]
        lib.mij_batch_upload_any.argtypes = [p, p, i, i, i, i]
        lib.mij_batch_encode_interleaved.argtypes = [p, i, i]
        lib.mij_encode_any.argtypes = [p, i, i, i, i, i, i, p, sz, C.POINTER(sz)]
        lib.mij_decoder_transcode.argtypes = [p, i]
        lib.mij_decoder_transcoded.argtypes = [p, i, p, sz, C.POINTER(sz)]
        lib.mij_decoder_device_transcoded.restype = p
        lib.mij_decoder_device_transcoded.argtypes = [p, i, C.POINTER(sz)]
        lib.mij_decoder_transcode_ms.argtypes = [p, C.POINTER(C.c_float)]
        lib.mij_transcode.argtypes = [p, sz, i, p, sz, C.POINTER(sz)]
        lib.mij_decoder_transform.argtypes = [p, i, i, C.POINTER(Area), i]
        lib.mij_transform.argtypes = [p, sz, i, i, C.POINTER(Area), i, p, sz, C.POINTER(sz)]
        lib.mij_exif_orientation.argtypes = [p, sz]
        lib.mij_orientation_op.argtypes = [i]
        lib.mij_decoder_reconstruct_scaled.argtypes = [p, i, i]
        lib.mij_decoder_scaled_layout.argtypes = [p, i, i, p, i]
        lib.mij_decode_scaled.argtypes = [p, sz, i, i, p, sz, C.POINTER(i), C.POINTER(i)]
        lib.mij_max_jpg_bytes_sampled.restype = sz
        lib.mij_max_jpg_bytes_sampled.argtypes = [i, i, i, i]
        lib.mij_batch_encode_sampled.argtypes = [p, i, i, i]
        lib.mij_batch_sampled_component.argtypes = [p, i, i, p, sz]
        lib.mij_batch_sampled_layout.argtypes = [p, i, p, i]
        lib.mij_encode_sampled.argtypes = [p, i, i, i, i, i, i, i, p, sz, C.POINTER(sz)]
        lib.mij_resizer_create.restype = p
        lib.mij_resizer_create.argtypes = [i, i]
        lib.mij_resizer_destroy.restype = None
        lib.mij_resizer_destroy.argtypes = [p]
        lib.mij_resizer_resize.argtypes = [p, p, p, i, i]
        lib.mij_resizer_device_pixels.restype = p
        lib.mij_resizer_device_pixels.argtypes = [p, i, C.POINTER(C.c_longlong)]
        lib.mij_resizer_pixels.argtypes = [p, i, p, sz, C.c_longlong]
        lib.mij_resizer_ms.argtypes = [p, p]
        lib.mij_resizer_stream.restype = p
        lib.mij_resizer_stream.argtypes = [p]
        lib.mij_resizer_set_stream.argtypes = [p, p]
        lib.mij_resize.argtypes = [p, i, i, i, i, i, i, p, sz]
        lib.mij_thumbnail.argtypes = [p, sz, i, i, i, i, p, sz, C.POINTER(sz)]
        lib.mij_thumbnail_denom.argtypes = [i, i, i, i]
        lib.mij_libjpeg_tables.argtypes = [i, p]
        lib.mij_batch_encode_libjpeg.argtypes = [p, i, i, i]
        lib.mij_encode_libjpeg.argtypes = [p, i, i, i, i, i, i, i, p, sz, C.POINTER(sz)]
        lib.mij_thumbnail_libjpeg.argtypes = [p, sz, i, i, i, i, i, p, sz, C.POINTER(sz)]
        lib.mij_tensorizer_create.restype = p
        lib.mij_tensorizer_create.argtypes = [i, i]
        lib.mij_tensorizer_destroy.restype = None
        lib.mij_tensorizer_destroy.argtypes = [p]
        lib.mij_tensorizer_run.argtypes = [p, p, p, i, p, p, sz]
        lib.mij_tensor_bytes.restype = sz
        lib.mij_tensor_bytes.argtypes = [i, i, i, i]
        lib.mij_tensorizer_device.restype = p
        lib.mij_tensorizer_device.argtypes = [p, C.POINTER(sz)]
        lib.mij_tensorizer_read.argtypes = [p, p, sz]
        lib.mij_tensorizer_ms.argtypes = [p, C.POINTER(C.c_float)]
        lib.mij_tensorizer_stream.restype = p
        lib.mij_tensorizer_stream.argtypes = [p]
        lib.mij_tensorizer_set_stream.argtypes = [p, p]
        lib.mij_loader_create.restype = p
        lib.mij_loader_create.argtypes = [i, i, i, i]
        lib.mij_loader_destroy.restype = None
        lib.mij_loader_destroy.argtypes = [p]
        lib.mij_loader_load.argtypes = [p, C.POINTER(p), C.POINTER(sz), i, p, p, i, i, i, i, i, p, p, sz]
        lib.mij_loader_denom.argtypes = [p]
        lib.mij_loader_device.restype = p
        lib.mij_loader_device.argtypes = [p, C.POINTER(sz)]
        lib.mij_loader_read.argtypes = [p, p, sz]
        lib.mij_loader_ms.argtypes = [p, p]
        lib.mij_loader_stream.restype = p
        lib.mij_loader_stream.argtypes = [p]
        lib.mij_decoder_accept.argtypes = [p, C.c_uint]
        lib.mij_decoder_scan_info.argtypes = [p, i, C.POINTER(i), C.POINTER(i), C.POINTER(i)]
        lib.mij_loader_accept.argtypes = [p, C.c_uint]
        lib.mij_jpeg_size.argtypes = [p, sz, C.POINTER(i), C.POINTER(i)]
        lib.mij_test_prog_mapping.argtypes = [p, i]
        lib.mij_decoder_output.argtypes = [p, i]
        lib.mij_transcode_progressive.argtypes = [p, sz, i, p, sz, C.POINTER(sz)]
    except AttributeError:
        if not os.environ.get("MIJ_LIB"):  # older builds only in A/B timing runs
            raise
    _lib = lib
    return lib


def _check(rc: int, what: str) -> None:
    if rc != 0:
        lib = load()
        raise MijError(f"{what}: {lib.mij_strerror(rc).decode()} ({rc}): "
                       f"{lib.mij_last_message().decode(errors='replace')}")


def _ptr(a: np.ndarray) -> int:
    return a.ctypes.data


def max_jpg_bytes(w: int, h: int) -> int:
    return int(load().mij_max_jpg_bytes(w, h))


# ---- drop-in three-call path (main.c:144-152 call sequence) -----------------

def set_input_stride(px: int) -> None:
    _check(load().mij_set_input_stride(px), "mij_set_input_stride")


def set_quality(q: int) -> None:
    _check(load().mij_set_quality(q), "mij_set_quality")


def rgb_to_dct(frame_bgr: np.ndarray, region):
    """encoder.h:10 on a BGR frame; returns (Y, Cb, Cr) int16 planes."""
    lib = load()
    frame_bgr = np.ascontiguousarray(frame_bgr, np.uint8)
    x, y, w, h = region
    set_input_stride(frame_bgr.shape[1])
    Y = np.zeros(w * h, np.int16)
    Cb = np.zeros(w * h // 4, np.int16)
    Cr = np.zeros(w * h // 4, np.int16)
    lib.rgb_to_dct(_ptr(frame_bgr), _ptr(Y), _ptr(Cb), _ptr(Cr), Area(x, y, w, h))
    _check(lib.mij_last_error(), "rgb_to_dct")
    return Y, Cb, Cr


def init_huffman(Y, Cb, Cr, region):
    lib = load()
    x, y, w, h = region
    t = (Huff * 4)()
    lib.init_huffman(_ptr(Y), _ptr(Cb), _ptr(Cr), Area(x, y, w, h), C.addressof(t),
                     C.addressof(t) + 2 * C.sizeof(Huff))
    _check(lib.mij_last_error(), "init_huffman")
    return list(t)


def write_jpg(Y, Cb, Cr, region, tables) -> bytes:
    lib = load()
    x, y, w, h = region
    t = (Huff * 4)(*tables)
    out = np.zeros(max_jpg_bytes(w, h), np.uint8)
    n = lib.write_jpg(None, _ptr(out), _ptr(Y), _ptr(Cb), _ptr(Cr), Area(x, y, w, h),
                      C.addressof(t), C.addressof(t) + 2 * C.sizeof(Huff))
    _check(lib.mij_last_error(), "write_jpg")
    return out[:n].tobytes()


def _areas(regions):
    arr = (Area * len(regions))(*[Area(*map(int, r)) for r in regions])
    return arr


def encode_regions(frame_bgr: np.ndarray, regions, quality: int = 50) -> list:
    """mij_encode_regions: every (x, y, w, h) region of a BGR frame to its own
    JPEG in one launch sequence (main.c:142-155)."""
    lib = load()
    frame_bgr = np.ascontiguousarray(frame_bgr, np.uint8)
    H, W = frame_bgr.shape[:2]
    cap = sum(max_jpg_bytes(r[2], r[3]) for r in regions)
    out = np.zeros(max(cap, 1), np.uint8)
    lens = (C.c_size_t * len(regions))()
    _check(lib.mij_encode_regions(_ptr(frame_bgr), W, H, _areas(regions), len(regions), quality,
                                  _ptr(out), out.size, lens), "mij_encode_regions")
    res, off = [], 0
    for n in lens:
        res.append(out[off:off + n].tobytes())
        off += n
    return res


def _last_plan(handle) -> dict:
    """mij_test_last_plan (test-only, csrc/mij_testing.h; bound by name): the
    launch plan the last encode stored, as {field: value}."""
    fn = load().mij_test_last_plan
    fn.argtypes, fn.restype = [C.c_void_p, C.POINTER(C.c_int), C.c_int], C.c_int
    out = (C.c_int * len(PLAN_FIELDS))()
    n = fn(handle, out, len(PLAN_FIELDS))
    if n != len(PLAN_FIELDS):  # -2: bad arguments; anything else: this list is out of date
        raise MijError(f"mij_test_last_plan: {n} fields, expected {len(PLAN_FIELDS)}")
    return dict(zip(PLAN_FIELDS, [int(v) for v in out]))


def regions_last_plan() -> dict:
    """the launch plan of the last encode_regions call"""
    return _last_plan(None)


def encode(frame_bgr: np.ndarray, quality: int = 50, region=None) -> bytes:
    """mij_encode: whole path host->host."""
    lib = load()
    frame_bgr = np.ascontiguousarray(frame_bgr, np.uint8)
    H, W = frame_bgr.shape[:2]
    x, y, w, h = region if region else (0, 0, W, H)
    cap = max_jpg_bytes(w, h)
    out = np.zeros(cap, np.uint8)
    n = C.c_size_t(0)
    _check(lib.mij_encode(_ptr(frame_bgr), W, Area(x, y, w, h), quality, _ptr(out), cap,
                          C.byref(n)), "mij_encode")
    return out[:n.value].tobytes()


def max_jpg_bytes_any(w: int, h: int, restart_rows: int = 0) -> int:
    return int(load().mij_max_jpg_bytes_any(w, h, restart_rows))


SAMPLINGS = {"420": 0, "422": 1, "444": 2, "gray": 3}  # MIJ_SAMP_*


def _sampling(sampling) -> int:
    if sampling not in SAMPLINGS:
        raise ValueError(f"sampling {sampling!r}: one of {sorted(SAMPLINGS)}")
    return SAMPLINGS[sampling]


def max_jpg_bytes_sampled(w: int, h: int, sampling: str = "420", restart_rows: int = 0) -> int:
    return int(load().mij_max_jpg_bytes_sampled(w, h, _sampling(sampling), restart_rows))


ARITHMETICS = ("reference", "libjpeg")


def _arithmetic(arithmetic) -> bool:
    if arithmetic not in ARITHMETICS:
        raise ValueError(f"arithmetic {arithmetic!r}: one of {ARITHMETICS}")
    return arithmetic == "libjpeg"


def libjpeg_tables(quality: int) -> np.ndarray:
    """mij_libjpeg_tables: (2, 64) uint8, the luma and the chroma table libjpeg
    uses at a quality, zigzag order; host only"""
    out = np.zeros((2, 64), np.uint8)
    _check(load().mij_libjpeg_tables(int(quality), _ptr(out)), "mij_libjpeg_tables")
    return out


def encode_any(frame: np.ndarray, order: str = "bgr", quality: int = 50, restart_rows: int = 0,
               sampling: str = "420") -> bytes:
    """mij_encode_any: an (h, w, 3) frame of any size to a standard
    interleaved baseline stream, host to host; with sampling
    "422", "444" or "gray" through mij_encode_sampled.
    encode_libjpeg is the same call with libjpeg's arithmetic."""
    return _encode_host(frame, order, quality, restart_rows, sampling, False)


def encode_libjpeg(frame: np.ndarray, order: str = "bgr", quality: int = 75, restart_rows: int = 0,
                   sampling: str = "420") -> bytes:
    """mij_encode_libjpeg: encode_any with libjpeg's tables and coefficients
    for that quality and sampling, host to host"""
    return _encode_host(frame, order, quality, restart_rows, sampling, True)


def _encode_host(frame, order, quality, restart_rows, sampling, libjpeg) -> bytes:
    lib = load()
    frame = np.ascontiguousarray(frame, np.uint8)
    h, w = frame.shape[:2]
    n = C.c_size_t(0)
    samp = _sampling(sampling)
    if libjpeg:
        def call(px, out, cap):
            return lib.mij_encode_libjpeg(px, w, w, h, PIXEL_ORDERS[order], quality, samp, restart_rows, out, cap,
                                          C.byref(n))
        what = "mij_encode_libjpeg"
    elif samp:
        def call(px, out, cap):
            return lib.mij_encode_sampled(px, w, w, h, PIXEL_ORDERS[order], quality, samp, restart_rows, out, cap,
                                          C.byref(n))
        what = "mij_encode_sampled"
    else:
        def call(px, out, cap):
            return lib.mij_encode_any(px, w, w, h, PIXEL_ORDERS[order], quality, restart_rows, out, cap, C.byref(n))
        what = "mij_encode_any"
    rc = call(None, None, 0)
    if rc != 4:  # MIJ_ENOSPC carries the bound
        _check(rc or 1, what)
    out = np.zeros(n.value, np.uint8)
    _check(call(_ptr(frame), _ptr(out), out.size), what)
    return out[:n.value].tobytes()


# ---- device-resident batch ---------------------------------------------------

class Batch:
    STAGES = ["k1_colour_dct_quant", "fix", "tokenize", "stats", "tables", "pack", "emit", "total"]

    def __init__(self, w: int, h: int, max_frames: int, quality: int = 50, device: int = 0,
                 keep_coefs: bool = False, assembler: bool = False):
        """assembler=True: mij_assembler_create -- a batch that only assembles
        whole frames from band words (no input, coefficient or token buffers)."""
        self.lib = load()
        self.w, self.h, self.max_frames = w, h, max_frames
        create = self.lib.mij_assembler_create if assembler else self.lib.mij_batch_create
        self.h_ = create(device, w, h, max_frames, quality)
        self.fdims = None  # per-frame (w, h) of a region batch
        if not self.h_:
            raise MijError(f"{'mij_assembler_create' if assembler else 'mij_batch_create'} failed: "
                           f"{self.lib.mij_strerror(self.lib.mij_last_error()).decode()}")
        if keep_coefs:
            _check(self.lib.mij_batch_keep_coefs(self.h_, 1), "keep_coefs")

    def close(self) -> None:
        if self.h_:
            self.lib.mij_batch_destroy(self.h_)
            self.h_ = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_split(self, on: bool) -> None:
        _check(self.lib.mij_batch_set_split(self.h_, int(on)), "set_split")

    def set_overlap(self, nsub: int) -> None:
        """fused pipeline in nsub sub-batches, entropy of one beside K1 of the next"""
        _check(self.lib.mij_batch_set_overlap(self.h_, int(nsub)), "set_overlap")

    def set_option(self, name: str, value: int) -> None:
        """entropy-stage variant (include/mijpeg.h MIJ_OPT_*; same bytes)"""
        _check(self.lib.mij_batch_set_option(self.h_, OPTIONS[name], int(value)), f"set_option({name})")

    def get_option(self, name: str) -> int:
        v = int(self.lib.mij_batch_get_option(self.h_, OPTIONS[name]))
        if v == -2:  # mij_batch_get_option's error value (the error is set)
            _check(self.lib.mij_last_error() or 1, "get_option")
        return v

    def set_rgb(self, on: bool) -> None:
        """frames in R, G, B byte order (PPM) instead of the encoder's B, G, R"""
        _check(self.lib.mij_batch_set_rgb(self.h_, int(on)), "set_rgb")

    def set_frame_dims(self, dims) -> None:
        """per-frame (w, h) of a region batch; None restores the batch geometry"""
        if dims is None:
            _check(self.lib.mij_batch_set_frame_dims(self.h_, None, 0), "set_frame_dims")
            self.fdims = None
            return
        wh = np.ascontiguousarray(np.asarray(dims, np.int32).reshape(-1, 2))
        _check(self.lib.mij_batch_set_frame_dims(self.h_, _ptr(wh), wh.shape[0]), "set_frame_dims")
        self.fdims = [tuple(map(int, d)) for d in wh]

    def upload_regions(self, frame_bgr: np.ndarray, regions) -> None:
        frame_bgr = np.ascontiguousarray(frame_bgr, np.uint8)
        H, W = frame_bgr.shape[:2]
        _check(self.lib.mij_batch_upload_regions(self.h_, _ptr(frame_bgr), W, H, _areas(regions),
                                                 len(regions)), "upload_regions")
        self.fdims = [(int(r[2]), int(r[3])) for r in regions]

    def gather_regions(self, dev_ptr: int, pitch: int, frame_w: int, frame_h: int, regions) -> None:
        _check(self.lib.mij_batch_gather_regions(self.h_, dev_ptr, pitch, frame_w, frame_h,
                                                 _areas(regions), len(regions)), "gather_regions")
        self.fdims = [(int(r[2]), int(r[3])) for r in regions]

    def pad_input(self, dev_ptr: int, frame_stride: int, pitch: int, dims) -> None:
        """device frames of any (w, h), alignment and pitch, edge-extended to
        multiples of 16 into slots 0..n-1 (mij_batch_pad_input)"""
        wh = np.ascontiguousarray(np.asarray(dims, np.int32).reshape(-1, 2))
        _check(self.lib.mij_batch_pad_input(self.h_, dev_ptr, frame_stride, pitch, _ptr(wh), wh.shape[0]),
               "pad_input")
        self.fdims = [((int(w) + 15) & ~15, (int(h) + 15) & ~15) for w, h in wh]

    def upload_any(self, frame: np.ndarray, slot: int = 0) -> None:
        """one host (h, w, 3) frame of any size into a slot (mij_batch_upload_any)"""
        frame = np.ascontiguousarray(frame, np.uint8)
        h, w = frame.shape[:2]
        _check(self.lib.mij_batch_upload_any(self.h_, _ptr(frame), w, w, h, slot), "upload_any")
        dims = list(self.fdims) if self.fdims is not None else []
        dims += [(self.w, self.h)] * max(0, self.max_frames - len(dims))
        dims[slot] = ((w + 15) & ~15, (h + 15) & ~15)
        self.fdims = dims

    def encode_interleaved(self, n: int, restart_rows: int = 0) -> None:
        """slots 0..n-1 (padded input) to one-interleaved-scan streams of
        their true sizes; restart_rows MCU rows per restart interval (0: none)"""
        _check(self.lib.mij_batch_encode_interleaved(self.h_, n, restart_rows), "encode_interleaved")

    def encode_sampled(self, n: int, sampling: str = "444", restart_rows: int = 0) -> None:
        """encode_interleaved at a chroma sampling ("420", "422", "444", "gray";
        mij_batch_encode_sampled); restart_rows counts MCU rows of that sampling"""
        _check(self.lib.mij_batch_encode_sampled(self.h_, n, _sampling(sampling), restart_rows), "encode_sampled")

    def encode_libjpeg(self, n: int, sampling: str = "420", restart_rows: int = 0) -> None:
        """encode_sampled with libjpeg's arithmetic and the batch's quality on
        its scale (mij_batch_encode_libjpeg), 4:2:0 included"""
        _check(self.lib.mij_batch_encode_libjpeg(self.h_, n, _sampling(sampling), restart_rows), "encode_libjpeg")

    def sampled_layout(self, frame: int) -> dict:
        """mij_batch_sampled_layout: the geometry the last encode_sampled or encode_libjpeg coded, as
        Decoder.layout gives it"""
        out = np.zeros(24, np.int32)
        _check(self.lib.mij_batch_sampled_layout(self.h_, frame, _ptr(out), out.size), "sampled_layout")
        v = [int(x) for x in out]
        keys = ("w", "h", "ncomp", "hmax", "vmax", "mcus_x", "mcus_y", "ri", "interleaved")
        lay = dict(zip(keys, v[:9]))
        lay["comps"] = [tuple(v[9 + 5 * c:14 + 5 * c]) for c in range(lay["ncomp"])]  # h, v, tq, bw, bh
        lay["raw"] = v[:9 + 5 * lay["ncomp"]]
        return lay

    def sampled_component(self, frame: int, comp: int) -> np.ndarray:
        """(blocks, 64) int16: the plane the last encode_sampled coded, zigzag order, absolute DC"""
        _, _, _, bw, bh = self.sampled_layout(frame)["comps"][comp]
        out = np.zeros((bw * bh, 64), np.int16)
        _check(self.lib.mij_batch_sampled_component(self.h_, frame, comp, _ptr(out), out.size), "sampled_component")
        return out

    def upload(self, frames_bgr: np.ndarray, first: int = 0) -> None:
        frames_bgr = np.ascontiguousarray(frames_bgr, np.uint8)
        n = frames_bgr.shape[0] if frames_bgr.ndim == 4 else 1
        _check(self.lib.mij_batch_upload(self.h_, _ptr(frames_bgr), first, n), "upload")
        # full frames: the uploaded slots are canvas-sized again, the others
        # keep their region sizes (as the library does)
        if self.fdims is not None:
            dims = list(self.fdims) + [(self.w, self.h)] * max(0, self.max_frames - len(self.fdims))
            dims[first:first + n] = [(self.w, self.h)] * n
            self.fdims = None if all(d == (self.w, self.h) for d in dims) else dims

    def set_input(self, dev_ptr: int, frame_stride: int, pitch: int) -> None:
        _check(self.lib.mij_batch_set_input(self.h_, dev_ptr, frame_stride, pitch), "set_input")
        self.fdims = None

    def encode(self, n: int) -> None:
        _check(self.lib.mij_batch_encode(self.h_, n), "encode")

    def last_plan(self) -> dict:
        """what the last encode() launched (PLAN_FIELDS): host state the
        encode stored as it decided, read without touching the device"""
        return _last_plan(self.h_)

    def dct(self, n: int) -> None:
        _check(self.lib.mij_batch_dct(self.h_, n), "dct")

    def pattern_floor(self, n: int) -> None:
        """measurement only: K1's memory traffic without its arithmetic
        (mij_batch_pattern_floor); leaves garbage in the coefficient planes"""
        _check(self.lib.mij_batch_pattern_floor(self.h_, n), "pattern_floor")

    def sync(self) -> None:
        _check(self.lib.mij_batch_sync(self.h_), "sync")

    def output(self, frame: int) -> bytes:
        n = C.c_size_t(0)
        _check(self.lib.mij_batch_output(self.h_, frame, None, 0, C.byref(n)), "output")
        buf = np.zeros(max(n.value, 1), np.uint8)
        _check(self.lib.mij_batch_output(self.h_, frame, _ptr(buf), buf.size, C.byref(n)),
               "output")
        return buf[:n.value].tobytes()

    def lengths(self, n: int) -> np.ndarray:
        arr = (C.c_size_t * n)()
        _check(self.lib.mij_batch_lengths(self.h_, arr, n), "lengths")
        return np.array(arr[:], np.int64)

    def coefs(self, frame: int, diffed: bool = True):
        w, h = self.fdims[frame] if self.fdims and frame < len(self.fdims) else (self.w, self.h)
        Y = np.zeros(w * h, np.int16)
        Cb = np.zeros(w * h // 4, np.int16)
        Cr = np.zeros(w * h // 4, np.int16)
        _check(self.lib.mij_batch_coefs(self.h_, frame, _ptr(Y), _ptr(Cb), _ptr(Cr),
                                        int(diffed)), "coefs")
        return Y, Cb, Cr

    def tables(self, frame: int):
        t = (Huff * 4)()
        _check(self.lib.mij_batch_tables(self.h_, frame, C.addressof(t)), "tables")
        return list(t)

    def set_timing(self, on: bool) -> None:
        _check(self.lib.mij_batch_set_timing(self.h_, int(on)), "set_timing")

    def stage_ms(self) -> dict:
        ms = np.zeros(len(self.STAGES), np.float32)
        _check(self.lib.mij_batch_stage_ms(self.h_, _ptr(ms), len(ms)), "stage_ms")
        return dict(zip(self.STAGES, [float(v) for v in ms]))

    def stage_history(self, steps: int) -> list:
        ms = np.zeros((steps, len(self.STAGES)), np.float32)
        n = self.lib.mij_batch_stage_history(self.h_, _ptr(ms), steps)
        if n < 0:
            _check(self.lib.mij_last_error(), "stage_history")
        return [dict(zip(self.STAGES, [float(v) for v in row])) for row in ms[:n]]

    def token_count(self, n: int) -> int:
        return int(self.lib.mij_batch_token_count(self.h_, n))

    def geometry(self) -> dict:
        keys = ["w", "h", "nblk", "nseg", "tiles_per_frame", "pack_window_words"]
        g = np.zeros(len(keys), np.int64)
        _check(self.lib.mij_batch_geometry(self.h_, _ptr(g), len(keys)), "geometry")
        return dict(zip(keys, [int(v) for v in g]))

    def audit(self, n: int) -> np.ndarray:
        """K1's fast-path keep/replay decisions (mij_batch_audit): uint64 per
        block [n, nblk], bit z = zigzag coefficient z was replayed in FP64."""
        nblk = self.geometry()["nblk"]
        m = np.zeros((n, nblk, 4), np.uint16)
        _check(self.lib.mij_batch_audit(self.h_, n, _ptr(m)), "audit")
        m = m.astype(np.uint64)
        return m[..., 0] | (m[..., 1] << np.uint64(16)) | (m[..., 2] << np.uint64(32)) | (m[..., 3] << np.uint64(48))

    def build_tables(self, n: int, hist: np.ndarray) -> None:
        """the four tables of frames 0..n-1 from given counts [n, 4, 257]
        (mij_batch_build_tables; read them with tables())"""
        h = np.ascontiguousarray(hist, np.uint32).reshape(n, 4, 257)
        _check(self.lib.mij_batch_build_tables(self.h_, n, _ptr(h)), "build_tables")

    def replays(self) -> int:
        return int(self.lib.mij_batch_replays(self.h_))

    # ---- one large frame over several ranks (include/mijpeg.h, sharding.py) ----
    def band_analyze(self, n: int) -> np.ndarray:
        last = np.zeros((n, 3), np.int16)
        _check(self.lib.mij_band_analyze(self.h_, n, _ptr(last)), "band_analyze")
        return last

    def band_histograms(self, n: int, prev_dc: np.ndarray) -> np.ndarray:
        prev = np.ascontiguousarray(prev_dc, np.int16).reshape(n, 3)
        hist = np.zeros((n, 4, 257), np.uint32)
        _check(self.lib.mij_band_histograms(self.h_, n, _ptr(prev), _ptr(hist)), "band_histograms")
        return hist

    def band_tables(self, n: int, hist: np.ndarray) -> np.ndarray:
        h = np.ascontiguousarray(hist, np.uint32).reshape(n, 4, 257)
        bits = np.zeros((n, 3), np.uint64)
        _check(self.lib.mij_band_tables(self.h_, n, _ptr(h), _ptr(bits)), "band_tables")
        return bits

    def band_pack(self, n: int, bit_offset: np.ndarray) -> np.ndarray:
        off = np.ascontiguousarray(bit_offset, np.uint64).reshape(n, 3)
        nw = np.zeros((n, 3), np.uint64)
        _check(self.lib.mij_band_pack(self.h_, n, _ptr(off), _ptr(nw)), "band_pack")
        return nw

    def band_words(self, frame: int, comp: int, nwords: int, dst_dev_ptr: int = 0):
        """Packed words of one band scan: into host memory (returned array), or
        into device memory at dst_dev_ptr (returns None)."""
        if dst_dev_ptr:
            _check(self.lib.mij_band_words(self.h_, frame, comp, dst_dev_ptr, nwords, 1), "band_words")
            return None
        out = np.zeros(max(nwords, 1), np.uint32)
        _check(self.lib.mij_band_words(self.h_, frame, comp, _ptr(out), nwords, 0), "band_words")
        return out[:nwords]

    def band_words_all(self, n: int, dst=None, dst_dev_ptr: int = 0, cap_words: int = 0):
        """Every scan's band words of frames 0..n-1 in (frame, comp) order, one
        call: into device memory at dst_dev_ptr (cap_words words), into the
        host array dst, or into a returned host array."""
        if dst_dev_ptr:
            _check(self.lib.mij_band_words_all(self.h_, n, dst_dev_ptr, cap_words, 1), "band_words_all")
            return None
        if dst is None:
            dst = np.zeros(max(cap_words, 1), np.uint32)
        _check(self.lib.mij_band_words_all(self.h_, n, _ptr(dst), dst.size, 0), "band_words_all")
        return dst

    def assemble_pieces(self, pieces: np.ndarray, src=None, src_dev_ptr: int = 0, src_words: int = 0) -> None:
        """OR pieces {frame*3+comp, first word, first src word, words} of one
        source buffer (device pointer or host array) into the scans."""
        pc = np.ascontiguousarray(pieces, np.uint64).reshape(-1, 4)
        if src_dev_ptr:
            _check(self.lib.mij_assemble_pieces(self.h_, src_dev_ptr, src_words, 1, _ptr(pc), pc.shape[0]),
                   "assemble_pieces")
        else:
            w = np.ascontiguousarray(src).view(np.uint32).reshape(-1)
            _check(self.lib.mij_assemble_pieces(self.h_, _ptr(w), w.size, 0, _ptr(pc), pc.shape[0]),
                   "assemble_pieces")

    # ---- the device-resident band protocol (all pointers device memory) ----
    def stream_ptr(self) -> int:
        """the batch's HIP stream (hipStream_t), for torch.cuda.ExternalStream"""
        return int(self.lib.mij_batch_stream(self.h_) or 0)

    def set_stream(self, stream_ptr: int) -> None:
        """enqueue on another HIP stream from now on (0: the batch's own);
        ordered after the work enqueued before (mij_batch_set_stream)"""
        _check(self.lib.mij_batch_set_stream(self.h_, stream_ptr or None), "set_stream")

    def band_analyze_async(self, n: int, d_last: int) -> None:
        _check(self.lib.mij_band_analyze_async(self.h_, n, d_last), "band_analyze_async")

    def band_histograms_async(self, n: int, d_prev: int, d_hist: int) -> None:
        _check(self.lib.mij_band_histograms_async(self.h_, n, d_prev, d_hist), "band_histograms_async")

    def band_tables_async(self, n: int, d_ghist: int, d_bound: int) -> None:
        """tables from the summed histograms; an upper bound of the band's
        words -> d_bound (uint64 [1] device buffer)"""
        _check(self.lib.mij_band_tables_async(self.h_, n, d_ghist, d_bound), "band_tables_async")

    def band_pack_async(self, n: int, d_bits: int) -> None:
        """the band packed from bit 0; d_bits: uint64 [3n + 1] device buffer
        (bits per scan, then the word count)"""
        _check(self.lib.mij_band_pack_async(self.h_, n, d_bits), "band_pack_async")

    def band_words_async(self, n: int, d_dst: int, cap_words: int) -> None:
        _check(self.lib.mij_band_words_async(self.h_, n, d_dst, cap_words), "band_words_async")

    def assemble_tables_async(self, n: int, d_ghist: int) -> None:
        _check(self.lib.mij_assemble_tables_async(self.h_, n, d_ghist), "assemble_tables_async")

    def assemble_async(self, n: int, d_allbits: int, world: int, d_src: int, stride_words: int) -> None:
        _check(self.lib.mij_assemble_async(self.h_, n, d_allbits, world, d_src, stride_words), "assemble_async")

    def band_stuff_async(self, n: int, d_allbits: int, world: int, rank: int, d_rec: int, d_total: int,
                         d_dst: int, cap: int) -> None:
        """distributed emission: this band's whole bytes of the final scans,
        stuffed, into d_dst; records [n, 3, 4] u64 and the total to d_rec / d_total"""
        _check(self.lib.mij_band_stuff_async(self.h_, n, d_allbits, world, rank, d_rec, d_total, d_dst, cap),
               "band_stuff_async")

    def copy_to_host_async(self, h_dst: int, d_src: int, nbytes: int) -> None:
        """device -> pinned host bytes on the batch's stream"""
        _check(self.lib.mij_copy_to_host_async(self.h_, h_dst, d_src, nbytes), "copy_to_host_async")

    def assemble_stuffed_async(self, n: int, d_allrec: int, world: int, d_src: int, stride: int) -> None:
        _check(self.lib.mij_assemble_stuffed_async(self.h_, n, d_allrec, world, d_src, stride),
               "assemble_stuffed_async")

    def assemble_begin(self, n: int, hist: np.ndarray) -> None:
        h = np.ascontiguousarray(hist, np.uint32).reshape(n, 4, 257)
        _check(self.lib.mij_assemble_begin(self.h_, n, _ptr(h)), "assemble_begin")

    def assemble_words(self, frame: int, comp: int, first_word: int, words=None,
                       src_dev_ptr: int = 0, nwords: int = 0) -> None:
        if src_dev_ptr:
            _check(self.lib.mij_assemble_words(self.h_, frame, comp, first_word, src_dev_ptr,
                                               nwords, 1), "assemble_words")
        else:
            w = np.ascontiguousarray(words, np.uint32)
            _check(self.lib.mij_assemble_words(self.h_, frame, comp, first_word, _ptr(w), w.size, 0),
                   "assemble_words")

    def assemble_end(self, n: int, total_bits: np.ndarray) -> None:
        t = np.ascontiguousarray(total_bits, np.uint64).reshape(n, 3)
        _check(self.lib.mij_assemble_end(self.h_, n, _ptr(t)), "assemble_end")


# ---- PPM ingest (utils/original.c:294-365 rules) and the streaming encoder ----

def ppm_header(path: str):
    """(width, height, pixel data offset) of a P6 file; raises MijError with
    the reference reader's message class (MIJ_EPPM / MIJ_EIO) otherwise."""
    w, h, off = C.c_int(0), C.c_int(0), C.c_longlong(0)
    _check(load().mij_ppm_header(path.encode(), C.byref(w), C.byref(h), C.byref(off)),
           f"ppm_header({path})")
    return w.value, h.value, off.value


def ppm_read(path: str, to_bgr: bool = False) -> np.ndarray:
    w, h, _ = ppm_header(path)
    out = np.zeros((h, w, 3), np.uint8)
    _check(load().mij_ppm_read(path.encode(), _ptr(out), out.nbytes, 3 * w, int(to_bgr)),
           f"ppm_read({path})")
    return out


class Stream:
    """mij_stream: PPM files / RGB frames -> JPEG through two device batches
    in ping-pong (include/mijpeg.h)."""
    STATS = ["wall_s", "read_s", "write_s", "gpu_s", "frames", "bytes_in", "bytes_out"]

    def __init__(self, w: int, h: int, chunk: int, quality: int = 50, device: int = 0,
                 threads: int = 0):
        self.lib = load()
        self.w, self.h = w, h
        self.h_ = self.lib.mij_stream_create(device, w, h, chunk, quality, threads)
        if not self.h_:
            raise MijError(f"mij_stream_create failed: "
                           f"{self.lib.mij_strerror(self.lib.mij_last_error()).decode()}")

    def close(self) -> None:
        if self.h_:
            self.lib.mij_stream_destroy(self.h_)
            self.h_ = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def encode_files(self, ins, outs) -> None:
        n = len(ins)
        a = (C.c_char_p * n)(*[s.encode() for s in ins])
        b = (C.c_char_p * n)(*[s.encode() for s in outs])
        failed = C.c_int(-1)
        rc = self.lib.mij_stream_encode_files(self.h_, a, b, n, C.byref(failed))
        if rc:
            raise MijError(f"stream_encode_files: {self.lib.mij_strerror(rc).decode()} ({rc}), "
                           f"file {failed.value}")

    def encode_frames(self, frames_rgb) -> list:
        n = len(frames_rgb)
        frames = [np.ascontiguousarray(f, np.uint8) for f in frames_rgb]
        cap = max_jpg_bytes(self.w, self.h)
        outs = [np.zeros(cap, np.uint8) for _ in range(n)]
        ins = (C.c_void_p * n)(*[_ptr(f) for f in frames])
        ops = (C.c_void_p * n)(*[_ptr(o) for o in outs])
        caps = (C.c_size_t * n)(*([cap] * n))
        lens = (C.c_size_t * n)()
        _check(self.lib.mij_stream_encode_frames(self.h_, ins, n, ops, caps, lens), "stream_encode_frames")
        return [o[:lens[i]].tobytes() for i, o in enumerate(outs)]

    def stats(self) -> dict:
        v = np.zeros(len(self.STATS), np.float64)
        _check(self.lib.mij_stream_stats(self.h_, _ptr(v), len(v)), "stream_stats")
        return dict(zip(self.STATS, [float(x) for x in v]))


def probe_mfma(A: np.ndarray, B: np.ndarray) -> np.ndarray:
    A = np.ascontiguousarray(A, np.int8).reshape(64, 16)
    B = np.ascontiguousarray(B, np.int8).reshape(64, 16)
    D = np.zeros((64, 4), np.int32)
    _check(load().mij_probe_mfma(_ptr(A), _ptr(B), _ptr(D)), "probe_mfma")
    return D


def colour_lut() -> np.ndarray:
    out = np.zeros(3 * 1024, np.uint32)
    _check(load().mij_colour_lut(_ptr(out)), "colour_lut")
    return out.reshape(3, 1024)


# ---- change detector (reference main/brain.c) ------

class Pair(C.Structure):
    """pair_t, reference include/structs.h:20-22."""
    _fields_ = [("beg", C.c_int), ("end", C.c_int), ("row", C.c_int), ("done", C.c_int)]


def _area_list(outs, n: int) -> list:
    return [(a.x, a.y, a.w, a.h) for a in outs[:max(0, min(n, 100))]]


class Detector:
    """Device-resident change detector over frames of w x h BGR pixels.

    step(frame) = the reference's subsample + compare (main.c:140-143) in one
    kernel launch plus the host-side area joining; store() = main.c:161.
    Returns (count, areas) with the count the reference's compare returns."""

    def __init__(self, w: int, h: int, device: int = 0):
        self.lib = load()
        self.w, self.h = w, h
        self.h_ = self.lib.mij_detector_create(device, w, h)
        if not self.h_:
            raise MijError("mij_detector_create failed: "
                           f"{self.lib.mij_strerror(self.lib.mij_last_error()).decode()}")
        self._outs = (Area * 100)()

    def close(self) -> None:
        if self.h_:
            self.lib.mij_detector_destroy(self.h_)
            self.h_ = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def upload(self, frame_bgr: np.ndarray, pitch: int = 0) -> int:
        """Copies a host frame ((h, w, 3), or (h, pitch) bytes rows) to the
        detector's frame buffer; returns its device address."""
        f = np.ascontiguousarray(frame_bgr, np.uint8)
        if pitch:
            assert f.shape == (self.h, pitch), f.shape
        else:
            assert f.shape == (self.h, self.w, 3), f.shape
        ptr = C.c_void_p()
        _check(self.lib.mij_detector_upload(self.h_, _ptr(f), pitch, C.byref(ptr)), "detector_upload")
        return ptr.value

    def subsample(self, dev_ptr: int, pitch: int | None = None) -> None:
        _check(self.lib.mij_detector_subsample(self.h_, dev_ptr, pitch or 3 * self.w),
               "detector_subsample")

    def compare(self):
        n = C.c_int()
        _check(self.lib.mij_detector_compare(self.h_, self._outs, C.byref(n)), "detector_compare")
        return n.value, _area_list(self._outs, n.value)

    def step(self, dev_ptr: int, pitch: int | None = None):
        n = C.c_int()
        _check(self.lib.mij_detector_step(self.h_, dev_ptr, pitch or 3 * self.w, self._outs,
                                          C.byref(n)), "detector_step")
        return n.value, _area_list(self._outs, n.value)

    def launch(self, dev_ptr: int, pitch: int | None = None) -> None:
        """The step's kernel alone, asynchronous (timing)."""
        _check(self.lib.mij_detector_launch(self.h_, dev_ptr, pitch or 3 * self.w), "detector_launch")

    def stream(self) -> int:
        return int(self.lib.mij_detector_stream(self.h_) or 0)

    def store(self) -> None:
        _check(self.lib.mij_detector_store(self.h_), "detector_store")

    def plane(self, which: int = 0) -> np.ndarray:
        out = np.zeros((self.h // 4, self.w // 4, 3), np.uint8)
        _check(self.lib.mij_detector_get_plane(self.h_, which, _ptr(out)), "detector_get_plane")
        return out

    def set_plane(self, which: int, rgb: np.ndarray) -> None:
        rgb = np.ascontiguousarray(rgb, np.uint8)
        assert rgb.shape == (self.h // 4, self.w // 4, 3), rgb.shape
        _check(self.lib.mij_detector_set_plane(self.h_, which, _ptr(rgb)), "detector_set_plane")

    def mask(self) -> np.ndarray:
        """Bit mask of the last compare as a bool array (h/4, w/4)."""
        words = C.c_int()
        _check(self.lib.mij_detector_mask(self.h_, None, 0, C.byref(words)), "detector_mask")
        m = np.zeros((self.h // 4, words.value), np.uint64)
        _check(self.lib.mij_detector_mask(self.h_, _ptr(m), m.size, C.byref(words)), "detector_mask")
        bits = np.unpackbits(m.view(np.uint8).reshape(self.h // 4, -1), axis=1, bitorder="little")
        return bits[:, :self.w // 4].astype(bool)


def drop_in_subsample(frame_bgr: np.ndarray) -> np.ndarray:
    """brain.h:7 subsample() through the drop-in entry point (f = NULL)."""
    lib = load()
    f = np.ascontiguousarray(frame_bgr, np.uint8)
    H, W = f.shape[:2]
    _check(lib.mij_set_input_stride(W), "set_input_stride")
    _check(lib.mij_set_frame_height(H), "set_frame_height")
    out = np.zeros((H // 4, W // 4, 3), np.uint8)
    lib.subsample(None, _ptr(f), _ptr(out))
    _check(lib.mij_last_error(), "subsample")
    return out


def drop_in_compare(sub: np.ndarray, saved: np.ndarray, W: int, H: int):
    """brain.h:9 compare() through the drop-in entry point."""
    lib = load()
    _check(lib.mij_set_input_stride(W), "set_input_stride")
    _check(lib.mij_set_frame_height(H), "set_frame_height")
    sub = np.ascontiguousarray(sub, np.uint8)
    saved = np.ascontiguousarray(saved, np.uint8)
    outs = (Area * 100)()
    diffs = (Pair * (2 * (W // 8)))()
    n = lib.compare(_ptr(sub), _ptr(saved), outs, diffs)
    _check(lib.mij_last_error(), "compare")
    return int(n), _area_list(outs, int(n))


def drop_in_enlarge_adjust(area, W: int, H: int):
    lib = load()
    _check(lib.mij_set_input_stride(W), "set_input_stride")
    _check(lib.mij_set_frame_height(H), "set_frame_height")
    a = Area(*area)
    lib.enlargeAdjust(C.byref(a))
    return (a.x, a.y, a.w, a.h)


# ---- round-trip verifier ---------------------------

PIXEL_ORDERS = {"bgr": 0, "rgb": 1}  # MIJ_PIX_*


def _order(order: str) -> int:
    if order not in PIXEL_ORDERS:
        raise MijError(f"pixel order {order!r}: 'bgr' or 'rgb'")
    return PIXEL_ORDERS[order]


ACCEPT_PROGRESSIVE = 1  # MIJ_ACCEPT_PROGRESSIVE
ACCEPT_440 = 4  # MIJ_ACCEPT_440: luma 1x2; bit value 2 is unknown


def jpeg_size(jpg: bytes):
    """mij_jpeg_size: (w, h) from the stream's frame header, of any SOFn; (0, 0) where it has none"""
    buf = np.frombuffer(jpg, np.uint8)
    w, h = C.c_int(0), C.c_int(0)
    load().mij_jpeg_size(_ptr(buf), buf.size, C.byref(w), C.byref(h))
    return w.value, h.value


def _progressive_decoder(jpg: bytes, progressive: bool = True, output: str = "baseline",
                         accept440: bool = False) -> "Decoder":
    """a decoder of the stream's size with MIJ_ACCEPT_PROGRESSIVE and MIJ_ACCEPT_440 set (or not), holding the
    decoded stream"""
    w, h = jpeg_size(jpg)  # (0, 0): the decoder then says what is wrong
    d = Decoder(max(16, (w + 15) // 16 * 16), max(16, (h + 15) // 16 * 16), 1, progressive=progressive,
                accept440=accept440)
    try:
        d.output(output)
        d.decode([jpg])
    except Exception:
        d.close()
        raise
    return d


def decode(jpg: bytes, order: str = "bgr", scale: int = 1, progressive: bool = False,
           accept440: bool = False) -> np.ndarray:
    """mij_decode: one baseline JFIF stream -> (h, w, 3) uint8 pixels, host to
    host; scale = 2, 4, 8: mij_decode_scaled, the image at 1/scale as
    libjpeg's reduced IDCTs give it.  progressive=True: through
    a Decoder that also accepts progressive streams;
    accept440=True: through one that also accepts 4:4:0."""
    if progressive or accept440:
        d = _progressive_decoder(jpg, progressive, accept440=accept440)
        try:
            d.reconstruct(order, scale)
            return d.pixels(0)
        finally:
            d.close()
    lib = load()
    buf = np.frombuffer(jpg, np.uint8)
    w, h = C.c_int(0), C.c_int(0)
    probe = np.zeros(1, np.uint8)
    if scale == 1:
        def call(dst, cap):
            return lib.mij_decode(_ptr(buf), buf.size, _order(order), _ptr(dst), cap, C.byref(w), C.byref(h))
        what = "mij_decode"
    else:
        def call(dst, cap):
            return lib.mij_decode_scaled(_ptr(buf), buf.size, _order(order), int(scale), _ptr(dst), cap, C.byref(w),
                                         C.byref(h))
        what = "mij_decode_scaled"
    rc = call(probe, 0)
    if rc != 4:  # MIJ_ENOSPC once the size is known, before any device work
        _check(rc, what)
    out = np.zeros((h.value, w.value, 3), np.uint8)
    _check(call(out, out.nbytes), what)
    return out


# mij_decoder_output (include/mijpeg.h: MIJ_OUT_*)
OUTPUTS = {"baseline": 0, "progressive": 1}


def transcode(jpg: bytes, restart_rows: int = 0, progressive: bool = False, output: str = "baseline",
              accept440: bool = False) -> bytes:
    """mij_transcode: one baseline stream -> the same coefficients in one
    interleaved scan with optimised Huffman tables and restart intervals of
    restart_rows MCU rows (0: none), host to host; lossless.
    progressive=True: through a Decoder that also accepts progressive streams
    ("progressive in, optimised baseline out").  output="progressive": the
    same coefficients as a progressive file instead.
    accept440=True: through a Decoder that also accepts 4:4:0."""
    if progressive or accept440 or output != "baseline":
        d = _progressive_decoder(jpg, progressive, output, accept440)
        try:
            d.transcode(restart_rows)
            return d.transcoded(0)
        finally:
            d.close()
    lib = load()
    buf = np.frombuffer(jpg, np.uint8)
    n = C.c_size_t(0)
    out = np.zeros(len(jpg) + 4096, np.uint8)  # enough for most; the exact size comes back otherwise
    rc = lib.mij_transcode(_ptr(buf), buf.size, restart_rows, _ptr(out), out.nbytes, C.byref(n))
    if rc == 4 and n.value > out.nbytes:  # MIJ_ENOSPC
        out = np.zeros(n.value, np.uint8)
        rc = lib.mij_transcode(_ptr(buf), buf.size, restart_rows, _ptr(out), out.nbytes, C.byref(n))
    _check(rc, "mij_transcode")
    return out[:n.value].tobytes()


# MIJ_XF_*: jpegtran's JXFORM order; rot90 is clockwise
XF_OPS = {"none": 0, "flip_h": 1, "flip_v": 2, "transpose": 3, "transverse": 4, "rot90": 5, "rot180": 6, "rot270": 7}
XF_TRIM = 1


def exif_orientation(jpg: bytes) -> int:
    """mij_exif_orientation: 1..8, 1 where the stream has no (well-formed) EXIF orientation; host only"""
    buf = np.frombuffer(jpg, np.uint8)
    return load().mij_exif_orientation(_ptr(buf), buf.size)


def orientation_op(n: int) -> str:
    """the operation (by name) that makes an image of EXIF orientation n upright"""
    code = load().mij_orientation_op(n)
    return next(k for k, v in XF_OPS.items() if v == code)


def _xf_args(jpg, op, trim, crop):
    """(op code, flags, crop pointer or None) of a transform call"""
    if op == "auto":
        if jpg is None:
            raise MijError("op 'auto' needs the stream: transform(jpg, 'auto'), or "
                           "orientation_op(exif_orientation(jpg))")
        op = orientation_op(exif_orientation(jpg))
    if isinstance(op, str):
        if op not in XF_OPS:
            raise MijError(f"operation {op!r}: one of {', '.join(XF_OPS)} or 'auto'")
        op = XF_OPS[op]
    area = C.byref(Area(*[int(v) for v in crop])) if crop is not None else None
    return int(op), XF_TRIM if trim is True else int(trim), area


def transform(jpg: bytes, op="rot90", trim: bool = False, crop=None, restart_rows: int = 0,
              progressive: bool = False, output: str = "baseline", accept440: bool = False) -> bytes:
    """mij_transform: one baseline stream -> the flipped / transposed / rotated
    (op, by name; "auto": by the stream's EXIF orientation) and / or cropped
    (crop = (x, y, w, h), MCU-aligned offset) image, coded as transcode codes
    it; lossless.  trim: cut a mirrored dimension down to
    whole MCUs instead of refusing it.  progressive=True: through a Decoder
    that also accepts progressive streams.  output="progressive": written
    as a progressive file.  accept440=True: through a Decoder
    that also accepts 4:4:0, with which a transposing operation turns 4:2:2
    into 4:4:0 and back instead of being refused."""
    if progressive or accept440 or output != "baseline":
        code, _, _ = _xf_args(jpg, op, trim, crop)  # resolves "auto" from the stream
        d = _progressive_decoder(jpg, progressive, output, accept440)
        try:
            d.transform(code, trim, crop, restart_rows)
            return d.transcoded(0)
        finally:
            d.close()
    lib = load()
    buf = np.frombuffer(jpg, np.uint8)
    code, flags, area = _xf_args(jpg, op, trim, crop)
    n = C.c_size_t(0)
    out = np.zeros(len(jpg) + 4096, np.uint8)  # enough for most; the exact size comes back otherwise
    rc = lib.mij_transform(_ptr(buf), buf.size, code, flags, area, restart_rows, _ptr(out), out.nbytes, C.byref(n))
    if rc == 4 and n.value > out.nbytes:  # MIJ_ENOSPC
        out = np.zeros(n.value, np.uint8)
        rc = lib.mij_transform(_ptr(buf), buf.size, code, flags, area, restart_rows, _ptr(out), out.nbytes, C.byref(n))
    _check(rc, "mij_transform")
    return out[:n.value].tobytes()


class Decoder:
    """Baseline JPEG streams (the encoder's own three-scan shape, and what
    libjpeg writes: one interleaved scan, greyscale / 4:4:4 / 4:2:2 / 4:2:0,
    any size, restart intervals) -> coefficient planes, entropy-decoded on
    the GPU, and from those (reconstruct) the pixels libjpeg would give.
    progressive=True (mij_decoder_accept): progressive streams too;
    accept440=True: 4:4:0 too, and transposing transforms of 4:2:2."""

    def __init__(self, max_w: int, max_h: int, max_frames: int, device: int = 0, progressive: bool = False,
                 accept440: bool = False):
        self.lib = load()
        self.scale_ = 1  # of the last reconstruct
        self.h_ = self.lib.mij_decoder_create(device, max_w, max_h, max_frames)
        if not self.h_:
            raise MijError("mij_decoder_create failed: "
                           f"{self.lib.mij_strerror(self.lib.mij_last_error()).decode()}")
        if progressive or accept440:
            self.accept((ACCEPT_PROGRESSIVE if progressive else 0) | (ACCEPT_440 if accept440 else 0))

    def accept(self, mask: int) -> None:
        """mij_decoder_accept: what the decoder takes beyond baseline (ACCEPT_PROGRESSIVE | ACCEPT_440), until
        changed"""
        _check(self.lib.mij_decoder_accept(self.h_, mask), "decoder_accept")

    def output(self, fmt: str) -> None:
        """mij_decoder_output: what transcode and transform write, "baseline" (the default) or "progressive",
        until changed"""
        if fmt not in OUTPUTS:
            raise MijError(f"output {fmt!r}: one of {', '.join(OUTPUTS)}")
        _check(self.lib.mij_decoder_output(self.h_, OUTPUTS[fmt]), "decoder_output")

    def scan_info(self, frame: int) -> dict:
        """mij_decoder_scan_info of the last decode: progressive (bool), nscans, levels"""
        a, b, c = C.c_int(), C.c_int(), C.c_int()
        _check(self.lib.mij_decoder_scan_info(self.h_, frame, C.byref(a), C.byref(b), C.byref(c)), "decoder_scan_info")
        return {"progressive": bool(a.value), "nscans": b.value, "levels": c.value}

    def close(self) -> None:
        if self.h_:
            self.lib.mij_decoder_destroy(self.h_)
            self.h_ = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def decode(self, streams) -> None:
        n = len(streams)
        bufs = [np.frombuffer(s, np.uint8) for s in streams]
        ptrs = (C.c_void_p * n)(*[_ptr(b) for b in bufs])
        lens = (C.c_size_t * n)(*[len(s) for s in streams])
        _check(self.lib.mij_decoder_decode(self.h_, ptrs, lens, n), "decoder_decode")

    def passes(self) -> int:
        return int(self.lib.mij_decoder_passes(self.h_))

    def info(self, frame: int):
        w, h = C.c_int(), C.c_int()
        dqt = np.zeros(128, np.uint8)
        _check(self.lib.mij_decoder_info(self.h_, frame, C.byref(w), C.byref(h), _ptr(dqt)), "decoder_info")
        return w.value, h.value, dqt

    def coefs(self, frame: int):
        w, h, _ = self.info(frame)
        Y = np.zeros(w * h, np.int16)
        Cb = np.zeros(w * h // 4, np.int16)
        Cr = np.zeros(w * h // 4, np.int16)
        _check(self.lib.mij_decoder_coefs(self.h_, frame, _ptr(Y), _ptr(Cb), _ptr(Cr)), "decoder_coefs")
        return Y, Cb, Cr

    def layout(self, frame: int) -> dict:
        """mij_decoder_layout: the frame's geometry; "raw" is the int list as the library gives it"""
        out = np.zeros(24, np.int32)
        _check(self.lib.mij_decoder_layout(self.h_, frame, _ptr(out), out.size), "decoder_layout")
        v = [int(x) for x in out]
        keys = ("w", "h", "ncomp", "hmax", "vmax", "mcus_x", "mcus_y", "ri", "interleaved")
        lay = dict(zip(keys, v[:9]))
        lay["comps"] = [tuple(v[9 + 5 * c:14 + 5 * c]) for c in range(lay["ncomp"])]  # h, v, tq, bw, bh
        lay["raw"] = v[:9 + 5 * lay["ncomp"]]
        return lay

    def component(self, frame: int, comp: int) -> np.ndarray:
        """(blocks, 64) int16: the component's padded plane, zigzag order, absolute DC"""
        _, _, _, bw, bh = self.layout(frame)["comps"][comp]
        out = np.zeros((bw * bh, 64), np.int16)
        _check(self.lib.mij_decoder_component(self.h_, frame, comp, _ptr(out), out.size), "decoder_component")
        return out

    def scaled_layout(self, frame: int, scale: int) -> dict:
        """mij_decoder_scaled_layout: the frame's geometry at 1/scale; comps: (S, cw, ch, pitch, rows)"""
        out = np.zeros(18, np.int32)
        _check(self.lib.mij_decoder_scaled_layout(self.h_, frame, int(scale), _ptr(out), out.size),
               "decoder_scaled_layout")
        v = [int(x) for x in out]
        lay = {"w": v[0], "h": v[1], "ncomp": v[2]}
        lay["comps"] = [tuple(v[3 + 5 * c:8 + 5 * c]) for c in range(v[2])]
        lay["raw"] = v[:3 + 5 * v[2]]
        return lay

    def plane(self, frame: int, comp: int) -> np.ndarray:
        """(8 * blocks down, 8 * blocks across) uint8: the padded sample plane
        after the IDCT; after a scaled reconstruct (rows, pitch) of scaled_layout"""
        if self.scale_ > 1:
            _, _, _, pitch, rows = self.scaled_layout(frame, self.scale_)["comps"][comp]
            out = np.zeros((rows, pitch), np.uint8)
            _check(self.lib.mij_decoder_plane(self.h_, frame, comp, _ptr(out), out.nbytes), "decoder_plane")
            return out
        _, _, _, bw, bh = self.layout(frame)["comps"][comp]
        out = np.zeros((8 * bh, 8 * bw), np.uint8)
        _check(self.lib.mij_decoder_plane(self.h_, frame, comp, _ptr(out), out.nbytes), "decoder_plane")
        return out

    def reconstruct(self, order: str = "bgr", scale: int = 1) -> None:
        """every frame of the last decode -> planes and pixels (asynchronous);
        scale = 2, 4, 8: at 1/scale (mij_decoder_reconstruct_scaled), and
        pixels / plane / device_pixels then serve the scaled result"""
        if scale == 1:
            _check(self.lib.mij_decoder_reconstruct(self.h_, _order(order)), "decoder_reconstruct")
        else:
            _check(self.lib.mij_decoder_reconstruct_scaled(self.h_, _order(order), int(scale)),
                   "decoder_reconstruct_scaled")
        self.scale_ = int(scale)

    def pixels(self, frame: int, pitch: int = 0, out: np.ndarray | None = None) -> np.ndarray:
        """(h, w, 3) uint8 pixels of `frame`; with `pitch` (bytes, >= 3*w) the
        rows land pitch bytes apart in `out` (a flat uint8 array, or a new
        one), whose other bytes are left as they are"""
        w, h, _ = self.info(frame)
        if self.scale_ > 1:
            w, h = self.scaled_layout(frame, self.scale_)["raw"][:2]
        if not pitch:
            out = np.zeros((h, w, 3), np.uint8)
        elif out is None:
            out = np.zeros(h * pitch, np.uint8)
        _check(self.lib.mij_decoder_pixels(self.h_, frame, _ptr(out), out.nbytes, pitch), "decoder_pixels")
        return out

    def planes(self, frame: int):
        """the IDCT output before upsampling: Y (h, w), Cb and Cr (h/2, w/2)"""
        w, h, _ = self.info(frame)
        Y = np.zeros((h, w), np.uint8)
        Cb = np.zeros((h // 2, w // 2), np.uint8)
        Cr = np.zeros((h // 2, w // 2), np.uint8)
        _check(self.lib.mij_decoder_planes(self.h_, frame, _ptr(Y), _ptr(Cb), _ptr(Cr)), "decoder_planes")
        return Y, Cb, Cr

    def device_pixels(self, frame: int):
        """(device address, pitch in bytes) of `frame`'s pixels: valid until
        the next decode, complete once the decoder's stream (stream_ptr) has
        run the reconstruct"""
        pitch = C.c_longlong(0)
        ptr = self.lib.mij_decoder_device_pixels(self.h_, frame, C.byref(pitch))
        if not ptr:
            _check(self.lib.mij_last_error() or 1, "decoder_device_pixels")
        return int(ptr), int(pitch.value)

    def reconstruct_ms(self):
        """(dc + idct, colour) HIP-event milliseconds of the last reconstruct; waits for it"""
        ms = (C.c_float * 2)()
        _check(self.lib.mij_decoder_reconstruct_ms(self.h_, ms), "decoder_reconstruct_ms")
        return float(ms[0]), float(ms[1])

    def stream_ptr(self) -> int:
        """the decoder's hipStream_t (Batch.set_stream orders an encode behind a reconstruct)"""
        return int(self.lib.mij_decoder_stream(self.h_) or 0)

    def transcode(self, restart_rows: int = 0) -> None:
        """every frame of the last decode -> a losslessly re-coded interleaved
        stream (mij_decoder_transcode); waits for the device"""
        _check(self.lib.mij_decoder_transcode(self.h_, restart_rows), "decoder_transcode")

    def transform(self, op="rot90", trim: bool = False, crop=None, restart_rows: int = 0) -> None:
        """every frame of the last decode -> its transformed and / or cropped
        image, coded as transcode codes it (mij_decoder_transform; op by
        name); read with transcoded / device_transcoded / transcode_ms"""
        code, flags, area = _xf_args(None, op, trim, crop)
        _check(self.lib.mij_decoder_transform(self.h_, code, flags, area, restart_rows), "decoder_transform")

    def transcoded(self, frame: int) -> bytes:
        """host copy of `frame`'s stream of the last transcode or transform"""
        _, size = self.device_transcoded(frame)
        n = C.c_size_t(0)
        out = np.zeros(size, np.uint8)
        _check(self.lib.mij_decoder_transcoded(self.h_, frame, _ptr(out), out.nbytes, C.byref(n)), "decoder_transcoded")
        return out[:n.value].tobytes()

    def device_transcoded(self, frame: int):
        """(device address, bytes) of `frame`'s stream: valid until the next decode or transcode"""
        n = C.c_size_t(0)
        ptr = self.lib.mij_decoder_device_transcoded(self.h_, frame, C.byref(n))
        if not ptr:
            _check(self.lib.mij_last_error() or 1, "decoder_device_transcoded")
        return int(ptr), int(n.value)

    def transcode_ms(self) -> float:
        """HIP-event milliseconds of the last transcode; waits for it"""
        ms = C.c_float(0)
        _check(self.lib.mij_decoder_transcode_ms(self.h_, C.byref(ms)), "decoder_transcode_ms")
        return float(ms.value)


# ---- resize: thumbnails at any size ---------------------------
RS_FILTERS = {"box": 0, "bilinear": 1, "bicubic": 2}  # MIJ_RS_*


class Image(C.Structure):
    """mij_image: 3-byte pixels in device memory, rows pitch bytes apart"""
    _fields_ = [("px", C.c_void_p), ("pitch", C.c_longlong), ("w", C.c_int), ("h", C.c_int)]


def _filter(name) -> int:
    if isinstance(name, str):
        if name not in RS_FILTERS:
            raise MijError(f"filter {name!r}: one of {', '.join(RS_FILTERS)}")
        return RS_FILTERS[name]
    return int(name)


def thumbnail_denom(w: int, h: int, out_w: int, out_h: int) -> int:
    """mij_thumbnail_denom: the scale 1/denom Pillow's Image.draft picks for a
    w x h file asked for out_w x out_h; host only"""
    return int(load().mij_thumbnail_denom(w, h, out_w, out_h))


def fit_size(w: int, h: int, max_w: int, max_h: int):
    """the size Image.thumbnail((max_w, max_h)) gives a w x h image: inside the
    box, the aspect ratio kept as nearly as whole pixels allow, never larger
    than the image; host only"""
    def round_aspect(number, key):
        return max(min(math.floor(number), math.ceil(number), key=key), 1)
    x, y = int(max_w), int(max_h)
    if x < 1 or y < 1 or w < 1 or h < 1:
        raise MijError(f"fit_size: {w}x{h} into {max_w}x{max_h}")
    if x >= w and y >= h:
        return w, h
    aspect = w / h
    if x / y >= aspect:
        x = round_aspect(y * aspect, key=lambda n: abs(aspect - n / y))
    else:
        y = round_aspect(x / aspect, key=lambda n: 0 if n == 0 else abs(aspect - x / n))
    return x, y


def resize(frame: np.ndarray, size, filter="bicubic") -> np.ndarray:
    """mij_resize: (h, w, 3) uint8 pixels -> (size[1], size[0], 3), byte for
    byte PIL.Image.resize(size, FILTER) for box, bilinear and bicubic; host to
    host through the GPU"""
    lib = load()
    if frame.ndim != 3 or frame.shape[2] != 3 or frame.dtype != np.uint8:
        raise MijError("resize: an (h, w, 3) uint8 array")
    frame = np.ascontiguousarray(frame)
    h, w = frame.shape[:2]
    ow, oh = int(size[0]), int(size[1])
    out = np.zeros((max(oh, 0), max(ow, 0), 3), np.uint8)
    _check(lib.mij_resize(_ptr(frame), w, w, h, ow, oh, _filter(filter), _ptr(out), out.nbytes), "mij_resize")
    return out


def thumbnail(jpg: bytes, size, filter="bicubic", quality: int = 75, arithmetic: str = "reference",
              sampling: str = "420", accept440: bool = False) -> bytes:
    """mij_thumbnail: one baseline stream -> a JPEG of exactly size = (w, h):
    decoded at thumbnail_denom, resized, encoded as encode_any encodes; the
    pixels never leave the device.  arithmetic "libjpeg": through
    mij_thumbnail_libjpeg at `sampling`, the coefficients Pillow's draft ->
    resize -> save(quality, subsampling) gives; with the
    default arithmetic the sampling is 4:2:0 and nothing else.
    accept440=True: the same three stages on one stream through a Decoder
    that also accepts 4:4:0."""
    lib = load()
    buf = np.frombuffer(jpg, np.uint8)
    ow, oh = int(size[0]), int(size[1])
    n = C.c_size_t(0)
    samp = _sampling(sampling)
    if accept440:
        if samp and not _arithmetic(arithmetic):
            raise ValueError(f"thumbnail: sampling {sampling!r} needs arithmetic=\"libjpeg\"")
        if ow < 1 or oh < 1 or ow > 65535 or oh > 65535:
            raise MijError(f"thumbnail: out size {ow}x{oh} (1..65535 each)")
        d = _progressive_decoder(jpg, False, accept440=True)
        r = b = None
        try:
            w, h, _ = d.info(0)
            denom = thumbnail_denom(w, h, ow, oh)
            r = Resizer(1)
            b = Batch((ow + 15) // 16 * 16, (oh + 15) // 16 * 16, 1, int(quality))
            r.set_stream(d.stream_ptr())
            b.set_stream(d.stream_ptr())
            d.reconstruct("bgr", denom)
            ptr, pitch = d.device_pixels(0)
            r.resize([(ptr, pitch, -(-w // denom), -(-h // denom))], [(ow, oh)], filter)
            ptr, pitch = r.device_pixels(0)
            b.pad_input(ptr, 0, pitch, [(ow, oh)])
            if _arithmetic(arithmetic):
                b.encode_libjpeg(1, sampling)
            else:
                b.encode_interleaved(1)
            return b.output(0)
        finally:  # the borrowers of the decoder's stream first
            if b is not None:
                b.close()
            if r is not None:
                r.close()
            d.close()
    if _arithmetic(arithmetic):
        out = np.zeros(max(int(lib.mij_max_jpg_bytes_sampled(ow, oh, samp, 0)), 1), np.uint8)
        _check(lib.mij_thumbnail_libjpeg(_ptr(buf), buf.size, ow, oh, _filter(filter), int(quality), samp, _ptr(out),
                                         out.nbytes, C.byref(n)), "mij_thumbnail_libjpeg")
        return out[:n.value].tobytes()
    if samp:
        raise ValueError(f"thumbnail: sampling {sampling!r} needs arithmetic=\"libjpeg\"")
    out = np.zeros(max(int(lib.mij_max_jpg_bytes_any(ow, oh, 0)), 1), np.uint8)
    _check(lib.mij_thumbnail(_ptr(buf), buf.size, ow, oh, _filter(filter), int(quality), _ptr(out), out.nbytes,
                             C.byref(n)), "mij_thumbnail")
    return out[:n.value].tobytes()


class Resizer:
    """Device images of any size, pointer and pitch -> resampled device images
    (mij_resizer_*): Pillow's Image.resize for box, bilinear and bicubic, byte
    for byte, frames of a call in one launch per pass."""

    def __init__(self, max_frames: int, device: int = 0):
        self.lib = load()
        self.sizes_ = []
        self.h_ = self.lib.mij_resizer_create(device, max_frames)
        if not self.h_:
            raise MijError("mij_resizer_create failed: "
                           f"{self.lib.mij_strerror(self.lib.mij_last_error()).decode()}: "
                           f"{self.lib.mij_last_message().decode(errors='replace')}")

    def close(self) -> None:
        if self.h_:
            self.lib.mij_resizer_destroy(self.h_)
            self.h_ = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def resize(self, images, sizes, filter="bicubic") -> None:
        """images: (device address, pitch, w, h) each; sizes: (out_w, out_h)
        each; asynchronous on the resizer's stream"""
        n = len(images)
        src = (Image * max(n, 1))(*[Image(int(a), int(pitch), int(w), int(h)) for a, pitch, w, h in images])
        wh = (C.c_int * (2 * max(n, 1)))(*[int(v) for s in sizes for v in s])
        _check(self.lib.mij_resizer_resize(self.h_, src, wh, n, _filter(filter)), "resizer_resize")
        self.sizes_ = [(int(s[0]), int(s[1])) for s in sizes]

    def pixels(self, frame: int) -> np.ndarray:
        """(out_h, out_w, 3) uint8 pixels of `frame` of the last resize; waits"""
        w, h = self.sizes_[frame] if 0 <= frame < len(self.sizes_) else (1, 1)
        out = np.zeros((h, w, 3), np.uint8)
        _check(self.lib.mij_resizer_pixels(self.h_, frame, _ptr(out), out.nbytes, 0), "resizer_pixels")
        return out

    def device_pixels(self, frame: int):
        """(device address, pitch in bytes) of `frame`'s pixels: valid until
        the next resize, complete once the resizer's stream has run it;
        Batch.pad_input takes them as they are"""
        pitch = C.c_longlong(0)
        ptr = self.lib.mij_resizer_device_pixels(self.h_, frame, C.byref(pitch))
        if not ptr:
            _check(self.lib.mij_last_error() or 1, "resizer_device_pixels")
        return int(ptr), int(pitch.value)

    def ms(self):
        """(horizontal, vertical) HIP-event milliseconds of the last resize; waits for it"""
        ms = (C.c_float * 2)()
        _check(self.lib.mij_resizer_ms(self.h_, ms), "resizer_ms")
        return float(ms[0]), float(ms[1])

    def stream_ptr(self) -> int:
        return int(self.lib.mij_resizer_stream(self.h_) or 0)

    def set_stream(self, stream) -> None:
        """run on the caller's hipStream_t (0 / None: the resizer's own), as Batch.set_stream"""
        _check(self.lib.mij_resizer_set_stream(self.h_, stream or None), "resizer_set_stream")


# ---- pixels to tensors -----------------------------------------
# MIJ_T_*: name -> (code, numpy dtype of the host copy; bfloat16 comes back as its uint16 bit patterns)
T_DTYPES = {"uint8": (0, np.uint8), "float16": (1, np.float16), "bfloat16": (2, np.uint16), "float32": (3, np.float32)}
T_LAYOUTS = {"nchw": 0, "nhwc": 1}
IMAGENET_MEAN = (0.485, 0.456, 0.406)
IMAGENET_STD = (0.229, 0.224, 0.225)


class TensorSpec(C.Structure):
    """mij_tensor_spec"""
    _fields_ = [("dtype", C.c_int), ("layout", C.c_int), ("swap", C.c_int), ("mean", C.c_float * 3),
                ("std", C.c_float * 3)]


def _dtype(dtype) -> int:
    if isinstance(dtype, str):
        if dtype not in T_DTYPES:
            raise MijError(f"dtype {dtype!r}: one of {', '.join(T_DTYPES)}")
        return T_DTYPES[dtype][0]
    return int(dtype)


def _spec(dtype, layout, swap, mean, std) -> TensorSpec:
    if isinstance(layout, str):
        if layout not in T_LAYOUTS:
            raise MijError(f"layout {layout!r}: one of {', '.join(T_LAYOUTS)}")
        layout = T_LAYOUTS[layout]
    return TensorSpec(_dtype(dtype), int(layout), int(swap), (C.c_float * 3)(*[float(v) for v in mean]),
                      (C.c_float * 3)(*[float(v) for v in std]))


def tensor_bytes(n: int, w: int, h: int, dtype="float16") -> int:
    """mij_tensor_bytes: bytes of an [n, 3, h, w] tensor of `dtype`; 0 for bad arguments; host only"""
    return int(load().mij_tensor_bytes(int(n), int(w), int(h), _dtype(dtype)))


def _shape(n: int, w: int, h: int, layout: int):
    return (n, h, w, 3) if layout == T_LAYOUTS["nhwc"] else (n, 3, h, w)


def _host_tensor(read, spec: TensorSpec, n: int, w: int, h: int) -> np.ndarray:
    """the owned buffer's host copy, through read(address, bytes)"""
    np_dtype = next(v[1] for v in T_DTYPES.values() if v[0] == spec.dtype)
    out = np.zeros(_shape(n, w, h, spec.layout), np_dtype)
    read(_ptr(out), out.nbytes)
    return out


def _out_target(out, spec: TensorSpec, dtype, n: int, w: int, h: int):
    """(address, bytes) of a caller's tensor: anything with data_ptr(),
    element_size(), numel() and is_contiguous(), such as a torch tensor on the
    library's device; refused when it is short, strided or of another dtype"""
    need = tensor_bytes(n, w, h, spec.dtype)
    es = need // max(3 * n * w * h, 1)
    if not out.is_contiguous():
        raise MijError("out: not contiguous")
    name = str(getattr(out, "dtype", ""))
    if out.element_size() != es or (isinstance(dtype, str) and name and name.split(".")[-1] != dtype):
        raise MijError(f"out: dtype {name or out.element_size()} where {dtype} ({es} bytes an element) is asked for")
    if out.numel() * es < need:
        raise MijError(f"out: {out.numel()} elements where {need // es} are needed")
    return int(out.data_ptr()), out.numel() * es


class Tensorizer:
    """Device images of one size -> one dense normalised tensor
    (mij_tensorizer_*): torchvision's to_tensor + normalize, bit for bit, all
    frames of a call in one launch."""

    def __init__(self, max_frames: int, device: int = 0):
        self.lib = load()
        self.last_ = None
        self.h_ = self.lib.mij_tensorizer_create(device, max_frames)
        if not self.h_:
            raise MijError("mij_tensorizer_create failed: "
                           f"{self.lib.mij_strerror(self.lib.mij_last_error()).decode()}: "
                           f"{self.lib.mij_last_message().decode(errors='replace')}")

    def close(self) -> None:
        if self.h_:
            self.lib.mij_tensorizer_destroy(self.h_)
            self.h_ = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def run(self, images, mirror=None, dtype="float16", layout="nchw", mean=IMAGENET_MEAN, std=IMAGENET_STD,
            swap: bool = False, out=None, dst_ptr: int = 0, cap: int = 0):
        """images: (device address, pitch, w, h) each, one size; mirror: a
        flag per image or None.  out (a tensor, see Loader.load) or dst_ptr +
        cap (a raw device address): written there, asynchronously on the
        tensorizer's stream; neither: into the tensorizer's own buffer, read
        with result()"""
        n = len(images)
        src = (Image * max(n, 1))(*[Image(int(a), int(pitch), int(w), int(h)) for a, pitch, w, h in images])
        flags = None if mirror is None else (C.c_uint8 * max(n, 1))(*[1 if m else 0 for m in mirror])
        spec = _spec(dtype, layout, swap, mean, std)
        w, h = (int(images[0][2]), int(images[0][3])) if n else (0, 0)
        if out is not None:
            dst_ptr, cap = _out_target(out, spec, dtype, n, w, h)
        _check(self.lib.mij_tensorizer_run(self.h_, src, flags, n, C.byref(spec), dst_ptr or None, cap), "tensorizer_run")
        if not dst_ptr:
            self.last_ = (spec, n, w, h)
        return out

    def result(self) -> np.ndarray:
        """host copy of the last run into the tensorizer's own buffer; waits"""
        if self.last_ is None:
            _check(self.lib.mij_tensorizer_read(self.h_, None, 0), "tensorizer_read")
        return _host_tensor(lambda a, nb: _check(self.lib.mij_tensorizer_read(self.h_, a, nb), "tensorizer_read"),
                            *self.last_)

    def device(self):
        """(device address, bytes) of the own buffer's tensor"""
        nb = C.c_size_t(0)
        ptr = self.lib.mij_tensorizer_device(self.h_, C.byref(nb))
        if not ptr:
            _check(self.lib.mij_last_error() or 1, "tensorizer_device")
        return int(ptr), int(nb.value)

    def ms(self) -> float:
        """HIP-event milliseconds of the last run; waits for it"""
        ms = C.c_float(0)
        _check(self.lib.mij_tensorizer_ms(self.h_, C.byref(ms)), "tensorizer_ms")
        return float(ms.value)

    def stream_ptr(self) -> int:
        return int(self.lib.mij_tensorizer_stream(self.h_) or 0)

    def set_stream(self, stream) -> None:
        """run on the caller's hipStream_t (0 / None: the tensorizer's own), as Batch.set_stream"""
        _check(self.lib.mij_tensorizer_set_stream(self.h_, stream or None), "tensorizer_set_stream")


class Loader:
    """Stored JPEGs -> one normalised tensor on the device (mij_loader_*):
    decode at a scale, crop, resize, tensorize, on one stream."""

    def __init__(self, max_w: int, max_h: int, max_frames: int, device: int = 0, progressive: bool = False,
                 accept440: bool = False):
        self.lib = load()
        self.last_ = None
        self.h_ = self.lib.mij_loader_create(device, max_w, max_h, max_frames)
        if not self.h_:
            raise MijError("mij_loader_create failed: "
                           f"{self.lib.mij_strerror(self.lib.mij_last_error()).decode()}: "
                           f"{self.lib.mij_last_message().decode(errors='replace')}")
        if progressive or accept440:
            self.accept((ACCEPT_PROGRESSIVE if progressive else 0) | (ACCEPT_440 if accept440 else 0))

    def accept(self, mask: int) -> None:
        """mij_loader_accept: as Decoder.accept, for the loader's decoder"""
        _check(self.lib.mij_loader_accept(self.h_, mask), "loader_accept")

    def close(self) -> None:
        if self.h_:
            self.lib.mij_loader_destroy(self.h_)
            self.h_ = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def load(self, jpgs, size, crops=None, mirror=None, filter="bilinear", scale: int = 0, dtype="float16",
             layout="nchw", mean=IMAGENET_MEAN, std=IMAGENET_STD, order="rgb", out=None):
        """jpgs: the streams; size = (w, h) of every output frame; crops: an
        (x, y, w, h) in full-size pixels per stream, or None; mirror: a flag
        per stream, or None; scale: the decode's denominator 1, 2, 4, 8, or 0:
        the largest that enlarges no frame (denom() tells).  out=None: the
        tensor as a numpy array from the loader's own buffer (bfloat16 as
        uint16 bit patterns).  out: an object with data_ptr(), element_size(),
        numel() and is_contiguous() (a torch tensor on the loader's device):
        written there on the loader's stream, and returned; synchronise
        (sync(), or torch.cuda.synchronize()) before reading it."""
        n = len(jpgs)
        bufs = [np.frombuffer(s, np.uint8) for s in jpgs]
        ptrs = (C.c_void_p * max(n, 1))(*[_ptr(b) for b in bufs])
        lens = (C.c_size_t * max(n, 1))(*[len(s) for s in jpgs])
        areas = None if crops is None else (Area * max(n, 1))(*[Area(*[int(v) for v in c]) for c in crops])
        flags = None if mirror is None else (C.c_uint8 * max(n, 1))(*[1 if m else 0 for m in mirror])
        spec = _spec(dtype, layout, False, mean, std)
        w, h = int(size[0]), int(size[1])
        dst_ptr, cap = _out_target(out, spec, dtype, n, w, h) if out is not None else (0, 0)
        _check(self.lib.mij_loader_load(self.h_, ptrs, lens, n, areas, flags, w, h, _filter(filter), int(scale),
                                        _order(order), C.byref(spec), dst_ptr or None, cap), "loader_load")
        if out is not None:
            return out
        self.last_ = (spec, n, w, h)
        return _host_tensor(lambda a, nb: _check(self.lib.mij_loader_read(self.h_, a, nb), "loader_read"), *self.last_)

    def denom(self) -> int:
        """the denominator the last load decoded at"""
        return int(self.lib.mij_loader_denom(self.h_))

    def device(self):
        """(device address, bytes) of the own buffer's tensor"""
        nb = C.c_size_t(0)
        ptr = self.lib.mij_loader_device(self.h_, C.byref(nb))
        if not ptr:
            _check(self.lib.mij_last_error() or 1, "loader_device")
        return int(ptr), int(nb.value)

    def ms(self):
        """(entropy decode, reconstruct, resize, tensorize) milliseconds of the last load; waits for it"""
        ms = (C.c_float * 4)()
        _check(self.lib.mij_loader_ms(self.h_, ms), "loader_ms")
        return tuple(float(v) for v in ms)

    def sync(self) -> None:
        """waits for the last load (its tensorize stage's end)"""
        self.ms()

    def stream_ptr(self) -> int:
        return int(self.lib.mij_loader_stream(self.h_) or 0)
