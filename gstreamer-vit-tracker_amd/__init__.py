"""MI355X-native ViT tracker hot path — Python bindings over the C ABI (include/vittrack_hip.h).

The classes mirror the reference's `vit_tracker` crate surface as its host uses it
(/root/reference/src/tracker_context.rs:2,21,88,90,94,120; src/selection_state.rs:1,44):
`VitTrack.new / init / update`, `BBox.new / from_array`. They are thin ctypes wrappers: all
computation happens in libvittrack_hip.so (hand-written gfx950 kernels). There is no CPU
fallback — without the built library or without a gfx950 device every call raises.
"""
from __future__ import annotations

import ctypes
import os
from ctypes import (POINTER, Structure, byref, c_char, c_char_p, c_double, c_float, c_int,
                    c_int32, c_int64, c_size_t, c_uint8, c_uint16, c_uint32, c_uint64, c_void_p)

import numpy as np

from . import weights  # noqa: F401  (blob writer / configs)
from . import synth    # noqa: F401
from . import snapshot  # noqa: F401  (the snapshot format in NumPy)

PKG_DIR = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("VITTRACK_HIP_LIB", os.path.join(PKG_DIR, "libvittrack_hip.so"))

PIX_RGB8, PIX_NV12, PIX_YUY2 = 0, 1, 2
# byte permutations / paddings of the three above (include/vittrack_hip.h: vt_pixfmt)
PIX_BGR8, PIX_RGBX, PIX_BGRX, PIX_NV21, PIX_UYVY = 3, 4, 5, 6, 7
# vt_pixfmt2: further values of vt_frame.format (three-plane 4:2:0, 16-bit NV12, 4:2:2 semi-planar, grey, pad-first RGB)
PIX_I420, PIX_YV12, PIX_P010, PIX_NV16, PIX_GRAY8, PIX_XRGB, PIX_XBGR = 16, 17, 18, 19, 20, 21, 22
# colour meaning of a YUV frame (vt_color_matrix, vt_color_range): vt_frame.format = pixel format | matrix << 8 | range << 12
COLOR_BT601, COLOR_BT709, COLOR_BT2020 = 0, 1, 2
RANGE_LIMITED, RANGE_FULL = 0, 1


def frame_format(pix: int, matrix: int = COLOR_BT601, full_range: bool = False) -> int:
    """VT_FRAME_FORMAT: the format word of a frame. The defaults give `pix` itself (BT.601, limited range). The library
    refuses colour bits on a format without chroma, a matrix above 2 and anything above bit 15."""
    return int(pix) | int(matrix) << 8 | (RANGE_FULL if full_range else RANGE_LIMITED) << 12


def colorimetry_from_gst(text: str):
    """(matrix, full_range) of the `colorimetry` field of GStreamer video/x-raw caps: the named forms bt601, bt709, bt2020
    and bt2020-10 (all limited range) or range:matrix:transfer:primaries in numbers (GstVideoColorRange: 1 full (0-255),
    2 limited (16-235); GstVideoColorMatrix: 3 BT.709, 4 BT.601, 6 BT.2020). ValueError for everything else: an unknown
    range or matrix, RGB, FCC, SMPTE240M, sRGB - there is no format word for them."""
    t = str(text).strip().lower()
    named = {"bt601": COLOR_BT601, "bt709": COLOR_BT709, "bt2020": COLOR_BT2020, "bt2020-10": COLOR_BT2020}
    if t in named:
        return named[t], False
    parts = t.split(":")
    if len(parts) == 4 and all(q.isdigit() for q in parts):
        rng, mat = int(parts[0]), int(parts[1])
        matrices = {3: COLOR_BT709, 4: COLOR_BT601, 6: COLOR_BT2020}
        if rng in (1, 2) and mat in matrices:
            return matrices[mat], rng == 1
    raise ValueError(f"colorimetry {text!r}: no BT.601 / BT.709 / BT.2020 YUV frame format")


class VtError(RuntimeError):
    def __init__(self, code, text):
        super().__init__(f"vittrack_hip error {code}: {text}")
        self.code = code


class CBBox(Structure):
    _fields_ = [("x", c_int32), ("y", c_int32), ("width", c_int32), ("height", c_int32)]


class CResult(Structure):
    _fields_ = [("success", c_int32), ("score", c_float), ("bbox", CBBox)]


class CConfig(Structure):
    _fields_ = [("struct_size", c_uint32), ("success_threshold", c_float), ("use_graph", c_int32),
                ("n_streams", c_int32), ("max_frame_width", c_int32),
                ("max_frame_height", c_int32), ("max_device_mib", c_int32),
                ("host_window_margin_pct", c_int32), ("host_zero_copy", c_int32), ("reserved", c_int32 * 5)]


class CModelInfo(Structure):
    _fields_ = [("patch", c_int32), ("template_size", c_int32), ("search_size", c_int32),
                ("dim", c_int32), ("heads", c_int32), ("layers", c_int32), ("mlp_dim", c_int32),
                ("head_channels", c_int32), ("tokens_template", c_int32),
                ("tokens_search", c_int32), ("kpad", c_int32), ("score_grid", c_int32),
                ("flops_per_frame", c_double), ("encoder_flops_per_frame", c_double),
                ("weight_bytes", c_uint64)]


class CFrame(Structure):
    _fields_ = [("plane0", c_void_p), ("plane1", c_void_p), ("width", c_int32),
                ("height", c_int32), ("stride0", c_int32), ("stride1", c_int32),
                ("format", c_int32), ("origin_x", c_int32), ("origin_y", c_int32),
                ("windowed", c_int32), ("window_w", c_int32), ("window_h", c_int32)]


class CCandidate(Structure):
    """one slot of a candidate pass (vt_candidate): the stream it works for and, with has_box, the box its search
    window is cut around instead of the stream's own state box"""
    _fields_ = [("stream", c_int32), ("has_box", c_int32), ("box", c_float * 4)]


class CRefreshStats(Structure):
    """vt_refresh_stats (32 bytes): a stream's refresh policy and what it has done since init"""
    _fields_ = [("period", c_int32), ("min_score", c_float), ("generation", c_int32), ("last_frame", c_int32),
                ("skipped_geometry", c_int32), ("reserved", c_int32 * 3)]


class CSnapshotDesc(Structure):
    """vt_snapshot_desc (128 bytes): what vt_snapshot_info reports of a stream snapshot"""
    _fields_ = [("total_bytes", c_uint32), ("header_bytes", c_uint32), ("state_bytes", c_uint32),
                ("policy_bytes", c_uint32), ("rows_bytes", c_uint32), ("flags", c_uint32),
                ("patch", c_int32), ("template_size", c_int32), ("search_size", c_int32), ("kpad", c_int32),
                ("tokens_template", c_int32), ("norm_a", c_float * 3), ("norm_b", c_float * 3), ("box", c_float * 4),
                ("frame_width", c_int32), ("frame_height", c_int32), ("frames_done", c_int32),
                ("success_count", c_int32), ("last_score", c_float), ("period", c_int32), ("min_score", c_float),
                ("skipped_geometry", c_int32), ("generation", c_int32), ("last_frame", c_int32),
                ("reserved", c_int32 * 1)]


class CChipInfo(Structure):
    """vt_chip_info (48 bytes): what the last pass of a stream did about its chip"""
    _fields_ = [("status", c_int32), ("frames_done", c_int32), ("success", c_int32), ("score", c_float),
                ("box", c_int32 * 4), ("geo", c_float * 3), ("reserved", c_int32 * 1)]


CHIP_NORM_BF16, CHIP_RGB8 = 0, 1     # vt_chip_kind

PEAKS_MAX = 8                        # VT_PEAKS_MAX


class CPeak(Structure):
    """vt_peak (32 bytes): one maximum of a slot's response map with its decoded box"""
    _fields_ = [("score", c_float), ("resp", c_float), ("box", c_float * 4), ("cell", c_int32), ("reserved", c_int32)]


class CPeaks(Structure):
    """vt_peaks (272 bytes): the peaks a pass listed for one of its slots"""
    _fields_ = [("n", c_int32), ("stream", c_int32), ("frames_done", c_int32), ("radius", c_int32), ("peak", CPeak * PEAKS_MAX)]


# vt_peak / vt_peaks (include/vittrack_hip.h) as NumPy records: 32 / 272 bytes
PEAK_DTYPE = np.dtype([("score", "<f4"), ("resp", "<f4"), ("box", "<f4", 4), ("cell", "<i4"), ("reserved", "<i4")])
PEAKS_DTYPE = np.dtype([("n", "<i4"), ("stream", "<i4"), ("frames_done", "<i4"), ("radius", "<i4"), ("peak", PEAK_DTYPE, PEAKS_MAX)])


class CDrawCmd(Structure):
    _fields_ = [("type", c_int32), ("x", c_int32), ("y", c_int32), ("w", c_int32), ("h", c_int32),
                ("p", c_int32), ("value", c_int32), ("text", c_char * 36)]


DRAW_BACKGROUND, DRAW_TEXT, DRAW_RECT, DRAW_CROSSHAIR, DRAW_CURSOR, DRAW_SELECTION = range(6)


class CKernelTime(Structure):
    _fields_ = [("name", c_char * 48), ("launches", c_int32), ("ms_total", c_float),
                ("flops", c_double), ("bytes", c_double)]


_lib = None

# every symbol include/vittrack_hip.h declares (tests check the library exports all of them)
EXPORTS = [
    "vt_config_default", "vt_last_error", "vt_abi_version", "vt_build_info", "vt_device_count", "vt_create",
    "vt_create_from_device_blob", "vt_destroy", "vt_get_model_info", "vt_init_rgb8",
    "vt_update_rgb8", "vt_init_yuy2", "vt_update_yuy2", "vt_init_nv12", "vt_update_nv12", "vt_init_rgb8_device",
    "vt_update_rgb8_device", "vt_init_nv12_device", "vt_update_nv12_device", "vt_group_create",
    "vt_group_create_from_device_blob", "vt_group_destroy", "vt_group_streams",
    "vt_group_get_model_info", "vt_group_init_device", "vt_group_enqueue_device", "vt_group_wait",
    "vt_recommended_streams", "vt_plan_engines", "vt_import_dmabuf", "vt_release_dmabuf", "vt_export_dmabuf", "vt_host_register", "vt_host_unregister", "vt_group_update_device", "vt_group_hip_stream", "vt_group_init_host", "vt_group_update_host", "vt_group_enqueue_host", "vt_group_wait_next",
    "vt_group_host_redos", "vt_group_graph_captures", "vt_nv12_to_rgb8", "vt_nv12_to_rgb8_device", "vt_nv12_to_rgb8_batch_device", "vt_overlay_nv12", "vt_overlay_nv12_device", "vt_overlay_rgb8",
    "vt_overlay_rgb8_device",
    "vt_group_profile_device", "vt_group_enable_taps", "vt_group_set_tuning", "vt_group_set_state_box", "vt_tracker_as_group",
    "vt_group_read_tensor", "vt_group_enqueue_device_streams", "vt_group_update_device_streams", "vt_group_update_host_streams",
    "vt_group_enqueue_host_streams", "vt_group_enqueue_init_host",
    "vt_group_update_device_candidates", "vt_group_update_host_candidates", "vt_scan_windows",
    "vt_rccl_unique_id", "vt_broadcast_weights_rccl", "vt_free_device_blob", "vt_init_frame", "vt_update_frame",
    "vt_set_template_refresh", "vt_template_refresh_stats", "vt_group_set_template_refresh",
    "vt_group_template_refresh_stats",
    "vt_group_enable_chips", "vt_group_set_chips", "vt_group_read_chips", "vt_group_chips_device",
    "vt_enable_chip", "vt_set_chip", "vt_read_chip",
    "vt_group_set_peaks", "vt_group_last_peaks", "vt_set_peaks", "vt_last_peaks",
    "vt_snapshot_bytes", "vt_group_snapshot_bytes", "vt_snapshot_info", "vt_group_export_stream",
    "vt_group_import_stream", "vt_group_copy_stream", "vt_export_state", "vt_import_state",
]


def lib():
    """Load libvittrack_hip.so (built in-tree by build.py). Fails loudly if it is missing."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise VtError(-2, f"{LIB_PATH} not built: run `python __graft_entry__.py` "
                          "(hipcc --offload-arch=gfx950). There is no CPU fallback.")
    # One HIP runtime per process: PyTorch bundles its own libamdhip64.so.7 / libhsa-runtime64 and a
    # second copy loaded later cannot see the GPU ("No HIP GPUs are available"). Importing torch
    # first makes this library's DT_NEEDED libamdhip64.so.7 resolve to the copy already loaded.
    try:
        import torch  # noqa: F401
    except Exception:  # torch absent: the library brings in /opt/rocm's runtime itself
        pass
    L = ctypes.CDLL(LIB_PATH)
    L.vt_last_error.restype = c_char_p
    L.vt_build_info.restype = c_char_p
    L.vt_config_default.argtypes = [POINTER(CConfig)]
    L.vt_create.argtypes = [c_char_p, c_int, POINTER(CConfig), POINTER(c_void_p)]
    L.vt_create_from_device_blob.argtypes = [c_void_p, c_size_t, c_int, POINTER(CConfig),
                                             POINTER(c_void_p)]
    L.vt_destroy.argtypes = [c_void_p]
    L.vt_destroy.restype = None
    L.vt_get_model_info.argtypes = [c_void_p, POINTER(CModelInfo)]
    u8p = POINTER(c_uint8)
    L.vt_init_rgb8.argtypes = [c_void_p, u8p, c_int, c_int, c_int, CBBox]
    L.vt_update_rgb8.argtypes = [c_void_p, u8p, c_int, c_int, c_int, POINTER(CResult)]
    L.vt_init_yuy2.argtypes = [c_void_p, u8p, c_int, c_int, c_int, CBBox]
    L.vt_update_yuy2.argtypes = [c_void_p, u8p, c_int, c_int, c_int, POINTER(CResult)]
    L.vt_init_nv12.argtypes = [c_void_p, u8p, u8p, c_int, c_int, c_int, c_int, CBBox]
    L.vt_update_nv12.argtypes = [c_void_p, u8p, u8p, c_int, c_int, c_int, c_int, POINTER(CResult)]
    L.vt_init_frame.argtypes = [c_void_p, POINTER(CFrame), c_int, CBBox]
    L.vt_update_frame.argtypes = [c_void_p, POINTER(CFrame), c_int, POINTER(CResult)]
    L.vt_init_rgb8_device.argtypes = [c_void_p, c_void_p, c_int, c_int, c_int, CBBox]
    L.vt_update_rgb8_device.argtypes = [c_void_p, c_void_p, c_int, c_int, c_int, POINTER(CResult)]
    L.vt_init_nv12_device.argtypes = [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int,
                                      CBBox]
    L.vt_update_nv12_device.argtypes = [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int,
                                        POINTER(CResult)]
    L.vt_host_register.argtypes = [c_int, c_void_p, c_size_t, POINTER(c_void_p)]
    L.vt_host_unregister.argtypes = [c_int, c_void_p]
    L.vt_group_create.argtypes = [c_char_p, c_int, POINTER(CConfig), POINTER(c_void_p)]
    L.vt_group_create_from_device_blob.argtypes = [c_void_p, c_size_t, c_int, POINTER(CConfig),
                                                   POINTER(c_void_p)]
    L.vt_group_destroy.argtypes = [c_void_p]
    L.vt_group_destroy.restype = None
    L.vt_group_streams.argtypes = [c_void_p]
    L.vt_group_get_model_info.argtypes = [c_void_p, POINTER(CModelInfo)]
    L.vt_group_init_device.argtypes = [c_void_p, c_int, POINTER(CFrame), CBBox]
    L.vt_group_enqueue_device.argtypes = [c_void_p, POINTER(CFrame), c_int]
    L.vt_group_wait.argtypes = [c_void_p, POINTER(CResult), c_int]
    L.vt_group_update_device.argtypes = [c_void_p, POINTER(CFrame), c_int, POINTER(CResult)]
    L.vt_recommended_streams.argtypes = [POINTER(CModelInfo), c_int]
    L.vt_plan_engines.argtypes = [POINTER(CModelInfo), c_int, POINTER(c_int), c_int]
    L.vt_import_dmabuf.argtypes = [c_int, c_int, c_size_t, POINTER(c_void_p), POINTER(c_void_p)]
    L.vt_release_dmabuf.argtypes = [c_void_p]
    L.vt_release_dmabuf.restype = None
    L.vt_export_dmabuf.argtypes = [c_int, c_void_p, c_size_t, POINTER(c_int)]
    L.vt_group_init_host.argtypes = [c_void_p, c_int, POINTER(CFrame), CBBox]
    L.vt_group_update_host.argtypes = [c_void_p, POINTER(CFrame), c_int, POINTER(CResult)]
    L.vt_group_enqueue_host.argtypes = [c_void_p, POINTER(CFrame), c_int]
    L.vt_group_wait_next.argtypes = [c_void_p, POINTER(CResult), c_int]
    L.vt_group_enqueue_device_streams.argtypes = [c_void_p, POINTER(c_int32), POINTER(CFrame), c_int]
    L.vt_group_update_device_streams.argtypes = [c_void_p, POINTER(c_int32), POINTER(CFrame), c_int, POINTER(CResult)]
    L.vt_group_update_host_streams.argtypes = [c_void_p, POINTER(c_int32), POINTER(CFrame), c_int, POINTER(CResult)]
    L.vt_group_enqueue_host_streams.argtypes = [c_void_p, POINTER(c_int32), POINTER(CFrame), c_int]
    L.vt_group_enqueue_init_host.argtypes = [c_void_p, c_int, POINTER(CFrame), CBBox]
    L.vt_group_update_device_candidates.argtypes = [c_void_p, POINTER(CCandidate), POINTER(CFrame), c_int, POINTER(CResult),
                                                    POINTER(c_int32)]
    L.vt_group_update_host_candidates.argtypes = L.vt_group_update_device_candidates.argtypes
    L.vt_scan_windows.argtypes = [c_int, c_int, c_float, c_float, c_int, POINTER(c_float), c_int]
    L.vt_set_template_refresh.argtypes = [c_void_p, c_int, c_float]
    L.vt_template_refresh_stats.argtypes = [c_void_p, POINTER(CRefreshStats)]
    L.vt_group_set_template_refresh.argtypes = [c_void_p, c_int, c_int, c_float]
    L.vt_group_template_refresh_stats.argtypes = [c_void_p, c_int, POINTER(CRefreshStats)]
    L.vt_snapshot_bytes.argtypes = [POINTER(CModelInfo)]
    L.vt_snapshot_bytes.restype = c_size_t
    L.vt_group_snapshot_bytes.argtypes = [c_void_p]
    L.vt_group_snapshot_bytes.restype = c_size_t
    L.vt_snapshot_info.argtypes = [c_void_p, c_size_t, POINTER(CSnapshotDesc)]
    L.vt_group_export_stream.argtypes = [c_void_p, c_int, c_void_p, c_size_t, POINTER(c_size_t)]
    L.vt_group_import_stream.argtypes = [c_void_p, c_int, c_void_p, c_size_t]
    L.vt_group_copy_stream.argtypes = [c_void_p, c_int, c_void_p, c_int]
    L.vt_export_state.argtypes = [c_void_p, c_void_p, c_size_t, POINTER(c_size_t)]
    L.vt_import_state.argtypes = [c_void_p, c_void_p, c_size_t]
    L.vt_group_enable_chips.argtypes = [c_void_p, c_int, c_int, POINTER(c_float), POINTER(c_float)]
    L.vt_group_set_chips.argtypes = [c_void_p, c_int, c_float, c_int, c_int]
    L.vt_group_read_chips.argtypes = [c_void_p, POINTER(c_int), c_int, c_void_p, c_size_t, POINTER(CChipInfo)]
    L.vt_group_chips_device.argtypes = [c_void_p, POINTER(c_void_p), POINTER(c_size_t), POINTER(c_void_p)]
    L.vt_enable_chip.argtypes = [c_void_p, c_int, c_int, POINTER(c_float), POINTER(c_float)]
    L.vt_set_chip.argtypes = [c_void_p, c_float, c_int, c_int]
    L.vt_read_chip.argtypes = [c_void_p, c_void_p, POINTER(CChipInfo)]
    L.vt_group_set_peaks.argtypes = [c_void_p, c_int, c_int, c_int, c_float]
    L.vt_group_last_peaks.argtypes = [c_void_p, c_void_p, c_int]
    L.vt_set_peaks.argtypes = [c_void_p, c_int, c_int, c_float]
    L.vt_last_peaks.argtypes = [c_void_p, c_void_p]
    L.vt_group_host_redos.argtypes = [c_void_p]
    L.vt_group_graph_captures.argtypes = [c_void_p]
    L.vt_group_hip_stream.argtypes = [c_void_p]
    L.vt_group_hip_stream.restype = c_void_p
    L.vt_group_profile_device.argtypes = [c_void_p, POINTER(CFrame), c_int, c_int,
                                          POINTER(CKernelTime), c_int]
    L.vt_group_enable_taps.argtypes = [c_void_p, c_int]
    L.vt_group_set_tuning.argtypes = [c_void_p, c_char_p, c_int]
    L.vt_group_set_state_box.argtypes = [c_void_p, c_int, POINTER(c_float)]
    L.vt_tracker_as_group.argtypes = [c_void_p]
    L.vt_tracker_as_group.restype = c_void_p
    L.vt_group_read_tensor.argtypes = [c_void_p, c_int, c_char_p, POINTER(c_float), c_int64]
    L.vt_group_read_tensor.restype = c_int64
    L.vt_nv12_to_rgb8.argtypes = [c_int, u8p, c_size_t, c_int, c_int, u8p]
    L.vt_nv12_to_rgb8_device.argtypes = [c_int, c_void_p, c_size_t, c_int, c_int, c_void_p,
                                         c_void_p]
    L.vt_nv12_to_rgb8_batch_device.argtypes = [c_int, POINTER(c_void_p), POINTER(c_size_t), c_int, c_int, c_int,
                                               POINTER(c_void_p), c_void_p]
    L.vt_overlay_nv12_device.argtypes = [c_int, c_void_p, c_int, c_int, c_int, POINTER(CDrawCmd), c_int,
                                         c_void_p]
    L.vt_overlay_nv12.argtypes = [c_int, u8p, c_int, c_int, POINTER(CDrawCmd), c_int]
    L.vt_overlay_rgb8_device.argtypes = L.vt_overlay_nv12_device.argtypes
    L.vt_overlay_rgb8.argtypes = L.vt_overlay_nv12.argtypes
    L.vt_rccl_unique_id.argtypes = [u8p]
    L.vt_broadcast_weights_rccl.argtypes = [u8p, c_int, c_int, c_int, c_char_p, POINTER(c_void_p),
                                            POINTER(c_size_t)]
    L.vt_free_device_blob.argtypes = [c_int, c_void_p]
    L.vt_free_device_blob.restype = None
    _lib = L
    return L


def _check(rc):
    if rc < 0:
        raise VtError(rc, lib().vt_last_error().decode(errors="replace"))
    return rc


def build_info() -> dict:
    """vt_build_info(): 'key=value;...' of the loaded library - ABI version and the sha256 build.py stamped into the
    translation unit of the dominant kernels (their sources + compile flags)"""
    txt = lib().vt_build_info().decode()
    return dict(kv.split("=", 1) for kv in txt.split(";") if "=" in kv)


def recommended_streams(info: "CModelInfo", max_streams: int = 128) -> int:
    """vt_recommended_streams: streams per group that fill the 256 CUs in whole GEMM rounds"""
    return lib().vt_recommended_streams(byref(info), max_streams)


def model_info_for(cfg_name: str) -> "CModelInfo":
    """the fields of vt_model_info the planners read, from a named configuration (no engine needed)"""
    cfg = weights.get_config(cfg_name)
    mi = CModelInfo()
    mi.patch, mi.template_size, mi.search_size = cfg.patch, cfg.template, cfg.search
    mi.dim, mi.heads, mi.layers, mi.mlp_dim, mi.head_channels = cfg.dim, cfg.heads, cfg.layers, cfg.mlp_dim, cfg.head_ch
    mi.tokens_template, mi.tokens_search, mi.kpad, mi.score_grid = cfg.n_t, cfg.n_s, cfg.kpad, cfg.grid_s
    return mi


def plan_engines(info: "CModelInfo", n_streams: int) -> list:
    """vt_plan_engines: engine (Group) sizes for n_streams on one GPU that avoid a nearly empty GEMM round"""
    sizes = (c_int * 16)()
    k = lib().vt_plan_engines(byref(info), n_streams, sizes, 16)
    if k <= 0:
        raise ValueError(f"vt_plan_engines({n_streams}) failed")
    return [int(sizes[i]) for i in range(k)]


def snapshot_bytes(info: "CModelInfo") -> int:
    """vt_snapshot_bytes: size of a stream snapshot of a model with info's tokens_template and kpad; needs no GPU"""
    return int(lib().vt_snapshot_bytes(byref(info)))


def snapshot_info(blob) -> dict:
    """vt_snapshot_info: validate a stream snapshot (everything but the comparison with an engine) and describe it:
    sizes, flags, input geometry, box, frame size, counters, last score, the refresh policy, generation and last_frame.
    Needs no GPU. Raises VtError (VT_ERR_FORMAT, -4) with the reason for a snapshot no engine would take."""
    raw = bytes(blob)
    d = CSnapshotDesc()
    _check(lib().vt_snapshot_info(raw, len(raw), byref(d)))
    out = {}
    for name, _ in CSnapshotDesc._fields_:
        if name == "reserved":
            continue
        v = getattr(d, name)
        out[name] = [float(x) for x in v] if hasattr(v, "__len__") else (float(v) if isinstance(v, float) else int(v))
    return out


def _export_snapshot(fn, *head) -> bytes:
    """the two-call form of vt_group_export_stream / vt_export_state: the size, then the bytes"""
    need = c_size_t(0)
    rc = fn(*head, None, 0, byref(need))
    if rc != -7:            # VT_ERR_SHORT_BUFFER carries the size; anything else is the answer
        _check(rc)
    buf = ctypes.create_string_buffer(int(need.value))
    _check(fn(*head, buf, need.value, byref(need)))
    return buf.raw[:int(need.value)]


def scan_windows(w: int, h: int, box_w: float, box_h: float, overlap_pct: int = 50) -> np.ndarray:
    """vt_scan_windows: the candidate state boxes [n, 4] (x, y, w, h) whose search windows tile a w x h frame, row by
    row; needs no GPU. Raises ValueError on arguments the library refuses."""
    n = lib().vt_scan_windows(w, h, box_w, box_h, overlap_pct, None, 0)
    if n <= 0:
        raise ValueError(f"vt_scan_windows({w}, {h}, {box_w}, {box_h}, {overlap_pct}) refused its arguments")
    out = np.empty((n, 4), np.float32)
    lib().vt_scan_windows(w, h, box_w, box_h, overlap_pct, _f32(out), n)
    return out


class DmaBuf:
    """a dma-buf mapped into device memory (vt_import_dmabuf); .ptr is usable as a frame plane"""

    def __init__(self, fd: int, nbytes: int, device: int = 0):
        self._h, p = c_void_p(), c_void_p()
        _check(lib().vt_import_dmabuf(device, fd, nbytes, byref(self._h), byref(p)))
        self.ptr, self.nbytes = p.value, nbytes

    def close(self):
        try:
            if getattr(self, "_h", None) is not None and self._h.value:
                lib().vt_release_dmabuf(self._h)
                self._h = c_void_p()
        except TypeError:      # interpreter shutdown: module globals are already None
            pass

    __del__ = close


def export_dmabuf(d_ptr: int, nbytes: int, device: int = 0) -> int:
    fd = c_int(-1)
    _check(lib().vt_export_dmabuf(device, d_ptr, nbytes, byref(fd)))
    return fd.value


class HostMapping:
    """A host buffer (NumPy array) page-locked and mapped into the device's address space
    (vt_host_register): `.d_ptr` + offset serves as plane pointers of frame_nv12 / frame_rgb8 with the
    *_device entry points - the pixel kernel reads only the pixels it samples over PCIe."""

    def __init__(self, arr: np.ndarray, device: int = 0):
        self.arr, self.device, self.d_ptr = arr, device, None
        dp = c_void_p()
        _check(lib().vt_host_register(device, c_void_p(arr.ctypes.data), arr.nbytes, byref(dp)))
        self.d_ptr = dp.value

    def close(self):
        if self.d_ptr is not None:
            lib().vt_host_unregister(self.device, c_void_p(self.arr.ctypes.data))
            self.d_ptr = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def rccl_unique_id() -> bytes:
    """rank 0: the 128-byte ncclUniqueId the host ships to the other ranks"""
    buf = (c_uint8 * 128)()
    _check(lib().vt_rccl_unique_id(buf))
    return bytes(buf)


def broadcast_weights_rccl(unique_id: bytes, world: int, rank: int, device: int,
                           weights_path: str | None):
    """vt_broadcast_weights_rccl: -> (device pointer, nbytes); release with free_device_blob"""
    idb = (c_uint8 * 128)(*unique_id)
    p, n = c_void_p(), c_size_t()
    _check(lib().vt_broadcast_weights_rccl(idb, world, rank, device,
                                           weights_path.encode() if weights_path else None,
                                           byref(p), byref(n)))
    return p.value, n.value


def free_device_blob(ptr: int, device: int = 0):
    lib().vt_free_device_blob(device, ptr)


def device_count() -> int:
    return lib().vt_device_count()


def _u8(a):
    return a.ctypes.data_as(POINTER(c_uint8))


def _u16(a):
    return a.ctypes.data_as(POINTER(c_uint16))


def _f32(a):
    return a.ctypes.data_as(POINTER(c_float))


def make_config(success_threshold=-1.0, use_graph=True, n_streams=1, max_w=0, max_h=0,
                max_device_mib=0, host_window_margin_pct=0, host_zero_copy=0) -> CConfig:
    c = CConfig()
    lib().vt_config_default(byref(c))
    c.success_threshold = success_threshold
    c.use_graph = 1 if use_graph else 0
    c.n_streams = n_streams
    c.max_frame_width, c.max_frame_height = max_w, max_h
    c.max_device_mib = max_device_mib
    c.host_window_margin_pct = host_window_margin_pct
    c.host_zero_copy = host_zero_copy
    return c


# ---- reference-shaped API ---------------------------------------------------------------------

class BBox:
    """≙ vit_tracker::BBox (src/selection_state.rs:44, src/tracker_context.rs:94)."""
    __slots__ = ("x", "y", "width", "height")

    def __init__(self, x, y, width, height):
        self.x, self.y, self.width, self.height = int(x), int(y), int(width), int(height)

    @staticmethod
    def new(x, y, width, height):
        return BBox(x, y, width, height)

    @staticmethod
    def from_array(a):
        return BBox(int(a[0]), int(a[1]), int(a[2]), int(a[3]))

    def as_tuple(self):
        return (self.x, self.y, self.width, self.height)

    def _c(self):
        return CBBox(self.x, self.y, self.width, self.height)

    def __eq__(self, o):
        return isinstance(o, BBox) and self.as_tuple() == o.as_tuple()

    def __repr__(self):
        return f"BBox(x={self.x}, y={self.y}, width={self.width}, height={self.height})"


class TrackResult:
    """≙ the Ok value of VitTrack::update: .success, .score, .bbox ([x, y, w, h])"""
    __slots__ = ("success", "score", "bbox")

    def __init__(self, c: CResult):
        self.success = bool(c.success)
        self.score = float(c.score)
        self.bbox = [c.bbox.x, c.bbox.y, c.bbox.width, c.bbox.height]

    def __repr__(self):
        return f"TrackResult(success={self.success}, score={self.score:.4f}, bbox={self.bbox})"


class NV12Frame:
    """packed NV12 host buffer: Y plane then interleaved UV, stride == width
    (the layout /root/reference/src/nv12_convert.rs:47-54 assumes)"""

    def __init__(self, buf: np.ndarray, width: int, height: int, matrix: int = COLOR_BT601, full_range: bool = False):
        self.format = frame_format(PIX_NV12, matrix, full_range)
        self.buf = np.ascontiguousarray(buf, np.uint8).reshape(-1)
        self.w, self.h = width, height
        assert self.buf.size >= width * height + ((width + 1) & ~1) * ((height + 1) // 2)

    def cframe(self) -> "CFrame":
        uv = self.buf[self.w * self.h:]
        return CFrame(self.buf.ctypes.data, uv.ctypes.data, self.w, self.h, self.w, (self.w + 1) & ~1, self.format,
                      0, 0, 0, 0, 0)


class YUY2Frame:
    """packed 4:2:2 host frame (Y0 U Y1 V), rows of 2*width bytes (src/pipeline_ir.rs:27-41)"""

    def __init__(self, buf: np.ndarray, width: int, height: int, matrix: int = COLOR_BT601, full_range: bool = False):
        self.format = frame_format(PIX_YUY2, matrix, full_range)
        self.buf = np.ascontiguousarray(buf, np.uint8).reshape(-1)
        self.w, self.h = width, height
        assert self.buf.size >= 2 * width * height and width % 2 == 0

    def cframe(self) -> "CFrame":
        return CFrame(self.buf.ctypes.data, None, self.w, self.h, 2 * self.w, 0, self.format, 0, 0, 0, 0, 0)


class _PackedFrame:
    """(H,W,C) uint8 host array of a packed pixel format. An array whose rows lie a constant number of bytes apart with
    the pixels of a row contiguous (e.g. buf[:, :W] of a wider buffer) is used in place, its row pitch as the stride;
    any other array is copied to C order. `stride` (bytes, >= C*W) asks for rows that far apart: the pixels are copied
    into such a buffer unless the array already has that pitch."""
    C = 3
    FMT = PIX_RGB8

    def __init__(self, a: np.ndarray, stride: int | None = None):
        a = np.asarray(a)
        if a.ndim != 3 or a.shape[2] != self.C:
            raise VtError(-1, f"{type(self).__name__}: need an (H,W,{self.C}) array, got {a.shape}")
        self.h, self.w = a.shape[0], a.shape[1]
        row = self.C * self.w
        if not (a.dtype == np.uint8 and a.strides[1:] == (self.C, 1) and a.strides[0] >= row):
            a = np.ascontiguousarray(a, np.uint8)
        if stride is not None and stride != a.strides[0]:
            if stride < row:
                raise VtError(-1, f"{type(self).__name__}: stride {stride} < {row}")
            buf = np.zeros((self.h, stride), np.uint8)
            buf[:, :row] = a.reshape(self.h, row)
            a = buf[:, :row].reshape(self.h, self.w, self.C)
        self.arr = a
        self.stride = int(a.strides[0])

    def cframe(self) -> "CFrame":
        return CFrame(self.arr.ctypes.data, None, self.w, self.h, self.stride, 0, self.FMT, 0, 0, 0, 0, 0)


class BGR8Frame(_PackedFrame):
    """(H,W,3) host array, channel order B,G,R (OpenCV's cv2.imread / VideoCapture)"""
    C, FMT = 3, PIX_BGR8


class RGBXFrame(_PackedFrame):
    """(H,W,4) host array R,G,B,x (RGBA: alpha ignored)"""
    C, FMT = 4, PIX_RGBX


class BGRXFrame(_PackedFrame):
    """(H,W,4) host array B,G,R,x (BGRA: alpha ignored; GStreamer BGRx / BGRA)"""
    C, FMT = 4, PIX_BGRX


class NV21Frame:
    """packed NV21 host buffer: Y plane then interleaved V,U, stride == width (Android / V4L2 sensors)"""

    def __init__(self, buf: np.ndarray, width: int, height: int, matrix: int = COLOR_BT601, full_range: bool = False):
        self.format = frame_format(PIX_NV21, matrix, full_range)
        self.buf = np.ascontiguousarray(buf, np.uint8).reshape(-1)
        self.w, self.h = width, height
        assert self.buf.size >= width * height + ((width + 1) & ~1) * ((height + 1) // 2)

    def cframe(self) -> "CFrame":
        vu = self.buf[self.w * self.h:]
        return CFrame(self.buf.ctypes.data, vu.ctypes.data, self.w, self.h, self.w, (self.w + 1) & ~1, self.format,
                      0, 0, 0, 0, 0)


class UYVYFrame:
    """packed 4:2:2 host frame (U Y0 V Y1), rows of 2*width bytes (V4L2 / SDI capture)"""

    def __init__(self, buf: np.ndarray, width: int, height: int, matrix: int = COLOR_BT601, full_range: bool = False):
        self.format = frame_format(PIX_UYVY, matrix, full_range)
        self.buf = np.ascontiguousarray(buf, np.uint8).reshape(-1)
        self.w, self.h = width, height
        assert self.buf.size >= 2 * width * height and width % 2 == 0

    def cframe(self) -> "CFrame":
        return CFrame(self.buf.ctypes.data, None, self.w, self.h, 2 * self.w, 0, self.format, 0, 0, 0, 0, 0)


class I420Frame:
    """packed I420 host buffer: Y plane (stride == width), then the U plane, then the V plane, each ceil(w/2) x
    ceil(h/2) bytes with stride ceil(w/2) (libav / GStreamer software decoders, raw .yuv files)"""
    FMT = PIX_I420

    def __init__(self, buf: np.ndarray, width: int, height: int, matrix: int = COLOR_BT601, full_range: bool = False):
        self.format = frame_format(self.FMT, matrix, full_range)
        self.buf = np.ascontiguousarray(buf, np.uint8).reshape(-1)
        self.w, self.h = width, height
        assert self.buf.size >= width * height + 2 * ((width + 1) // 2) * ((height + 1) // 2)

    def cframe(self) -> "CFrame":
        c = self.buf[self.w * self.h:]
        return CFrame(self.buf.ctypes.data, c.ctypes.data, self.w, self.h, self.w, (self.w + 1) // 2, self.format,
                      0, 0, 0, 0, 0)


class YV12Frame(I420Frame):
    """packed YV12 host buffer: I420 with the V plane in front of the U plane"""
    FMT = PIX_YV12


class P010Frame:
    """packed P010 (P012, P016) host buffer: NV12's layout with 16-bit little-endian samples, rows of 2*width bytes; only
    the high byte of a sample is read. `buf`: uint8 bytes or uint16 samples"""

    def __init__(self, buf: np.ndarray, width: int, height: int, matrix: int = COLOR_BT601, full_range: bool = False):
        self.format = frame_format(PIX_P010, matrix, full_range)
        buf = np.ascontiguousarray(buf)
        if buf.dtype == np.uint16:
            buf = buf.astype("<u2", copy=False).view(np.uint8)
        self.buf = np.ascontiguousarray(buf, np.uint8).reshape(-1)
        self.w, self.h = width, height
        assert self.buf.size >= 2 * (width * height + ((width + 1) & ~1) * ((height + 1) // 2))

    def cframe(self) -> "CFrame":
        uv = self.buf[2 * self.w * self.h:]
        return CFrame(self.buf.ctypes.data, uv.ctypes.data, self.w, self.h, 2 * self.w, 2 * ((self.w + 1) & ~1), self.format,
                      0, 0, 0, 0, 0)


class NV16Frame:
    """packed NV16 host buffer: Y plane then interleaved U,V with one chroma row per luma row, stride == width (even)"""

    def __init__(self, buf: np.ndarray, width: int, height: int, matrix: int = COLOR_BT601, full_range: bool = False):
        self.format = frame_format(PIX_NV16, matrix, full_range)
        self.buf = np.ascontiguousarray(buf, np.uint8).reshape(-1)
        self.w, self.h = width, height
        assert self.buf.size >= 2 * width * height and width % 2 == 0

    def cframe(self) -> "CFrame":
        uv = self.buf[self.w * self.h:]
        return CFrame(self.buf.ctypes.data, uv.ctypes.data, self.w, self.h, self.w, self.w, self.format, 0, 0, 0, 0, 0)


class Gray8Frame(_PackedFrame):
    """(H,W) or (H,W,1) host array, one grey byte per pixel (mono and thermal cameras): r = g = b = that byte"""
    C, FMT = 1, PIX_GRAY8

    def __init__(self, a: np.ndarray, stride: int | None = None):
        a = np.asarray(a)
        if a.ndim == 2:     # a trailing axis of stride 1, so that a padded buffer's view stays a view
            a = a[:, :, None]
            if a.dtype == np.uint8 and a.strides[1] == 1:
                a = np.lib.stride_tricks.as_strided(a, a.shape, (a.strides[0], 1, 1), writeable=False)
        super().__init__(a, stride)


class XRGBFrame(_PackedFrame):
    """(H,W,4) host array x,R,G,B (ARGB: alpha ignored; GStreamer xRGB / ARGB)"""
    C, FMT = 4, PIX_XRGB


class XBGRFrame(_PackedFrame):
    """(H,W,4) host array x,B,G,R (ABGR: alpha ignored; GStreamer xBGR / ABGR)"""
    C, FMT = 4, PIX_XBGR


class VitTrack:
    """≙ vit_tracker::VitTrack (src/tracker_context.rs:21,88,90,120)."""

    def __init__(self, weights_path: str, device: int = 0, success_threshold: float = -1.0,
                 use_graph: bool = True, max_w: int = 0, max_h: int = 0):
        self._h = c_void_p()
        cfg = make_config(success_threshold, use_graph, 1, max_w, max_h)
        _check(lib().vt_create(weights_path.encode(), device, byref(cfg), byref(self._h)))

    @staticmethod
    def new(model_path: str, **kw) -> "VitTrack":
        return VitTrack(model_path, **kw)

    def close(self):
        try:
            if getattr(self, "_h", None) and self._h.value:
                lib().vt_destroy(self._h)
                self._h = c_void_p()
        except TypeError:      # interpreter shutdown: module globals are already None
            pass

    __del__ = close

    def model_info(self) -> CModelInfo:
        mi = CModelInfo()
        _check(lib().vt_get_model_info(self._h, byref(mi)))
        return mi

    def as_group(self) -> "Group":
        return Group._view(lib().vt_tracker_as_group(self._h), self)

    def _call(self, op, frame, last):
        """vt_<op>_rgb8 / _nv12 / _yuy2 for a frame of those formats (the reference's call sites), vt_<op>_frame for
        every other format; `last`: the call's last argument (the box / the result)"""
        c, keep = Group._host_frame(frame)
        p0, p1 = ctypes.cast(c.plane0, POINTER(c_uint8)), ctypes.cast(c.plane1, POINTER(c_uint8))
        if c.format == PIX_NV12:
            rc = getattr(lib(), f"vt_{op}_nv12")(self._h, p0, p1, c.width, c.height, c.stride0, c.stride1, last)
        elif c.format in (PIX_RGB8, PIX_YUY2):
            fn = getattr(lib(), f"vt_{op}_{'rgb8' if c.format == PIX_RGB8 else 'yuy2'}")
            rc = fn(self._h, p0, c.width, c.height, c.stride0, last)
        else:
            rc = getattr(lib(), f"vt_{op}_frame")(self._h, byref(c), 0, last)
        _check(rc)

    def init(self, frame, bbox: BBox) -> None:
        """frame: (H,W,3) uint8 RGB array (≙ ArrayView3<u8>), NV12Frame, YUY2Frame, or one of BGR8Frame, RGBXFrame,
        BGRXFrame, NV21Frame, UYVYFrame, I420Frame, YV12Frame, P010Frame, NV16Frame, Gray8Frame, XRGBFrame, XBGRFrame. Like the reference's call site (src/tracker_context.rs:88) the caller gets
        nothing back; errors raise."""
        self._call("init", frame, bbox._c())

    def update(self, frame) -> TrackResult:
        r = CResult()
        self._call("update", frame, byref(r))
        return TrackResult(r)

    def set_template_refresh(self, period: int, min_score: float = 0.5) -> None:
        """vt_set_template_refresh: re-cut the template on the device every `period` updates (0: off, else >= 2) whose
        result succeeds with score >= min_score; see Group.set_template_refresh"""
        _check(lib().vt_set_template_refresh(self._h, int(period), float(min_score)))

    def template_refresh_stats(self) -> dict:
        st = CRefreshStats()
        _check(lib().vt_template_refresh_stats(self._h, byref(st)))
        return _refresh_stats_dict(st)

    def enable_chips(self, size: int, kind: int = CHIP_NORM_BF16, norm_a=(1.0, 1.0, 1.0), norm_b=(0.0, 0.0, 0.0)) -> None:
        """vt_enable_chip: see Group.enable_chips"""
        a, b = _chip_norms(kind, norm_a, norm_b)
        _check(lib().vt_enable_chip(self._h, int(size), int(kind), a, b))

    def set_chips(self, factor: float, period: int = 1, phase: int = 0) -> None:
        _check(lib().vt_set_chip(self._h, float(factor), int(period), int(phase)))

    def read_chips(self):
        """vt_read_chip -> (chip array [1, ...], [info dict])"""
        size, kind, _, _, _ = _chip_shape(lib().vt_tracker_as_group(self._h))
        out, ci = _chip_array(size, kind, 1), CChipInfo()
        _check(lib().vt_read_chip(self._h, out.ctypes.data, byref(ci)))
        return out, [_chip_info_dict(ci)]

    def chips_device(self) -> "DeviceChips":
        size, kind, stride, ptr, infos = _chip_shape(lib().vt_tracker_as_group(self._h))
        return DeviceChips(ptr, stride, infos, 1, size, kind)

    def set_peaks(self, max_peaks: int, radius: int = 2, min_resp: float = 0.0) -> None:
        """vt_set_peaks: see Group.set_peaks"""
        _check(lib().vt_set_peaks(self._h, int(max_peaks), int(radius), float(min_resp)))

    def last_peaks(self):
        """vt_last_peaks -> PEAKS_DTYPE array of one record: the peaks of the last update"""
        out = np.zeros(1, PEAKS_DTYPE)
        _check(lib().vt_last_peaks(self._h, out.ctypes.data))
        return out

    def set_result_overlay(self, **kw) -> None:
        """the result overlay of this tracker's engine: see Group.set_result_overlay"""
        self.as_group().set_result_overlay(**kw)

    def result_overlay_stats(self) -> dict:
        return self.as_group().result_overlay_stats(0)

    def set_motion_prior(self, on: bool = True, gain_pct: int | None = None, coast: int | None = None,
                         max_pct: int | None = None) -> None:
        """the motion prior of this tracker's engine: see Group.set_motion_prior"""
        self.as_group().set_motion_prior(on, gain_pct, coast, max_pct)

    def motion(self) -> dict:
        return self.as_group().motion(0)

    def set_appearance(self, on: bool = True, period: int | None = None, gate: float | None = None) -> None:
        """the appearance check of this tracker's engine: see Group.set_appearance"""
        self.as_group().set_appearance(on, period, gate)

    def appearance(self) -> dict:
        return self.as_group().appearance(0)

    def anchor(self) -> np.ndarray:
        return self.as_group().anchor(0)

    def set_proposals(self, mode: int = 1, **keys) -> None:
        """the reacquire proposals of this tracker's engine: see Group.set_proposals"""
        self.as_group().set_proposals(mode, **keys)

    def proposals(self) -> dict:
        return self.as_group().proposals(0)

    def set_conflicts(self, on: bool = True, iou: float | None = None, gate: bool | None = None) -> None:
        """the stream conflicts of this tracker's engine: see Group.set_conflicts (a group of one has nobody to compare with)"""
        self.as_group().set_conflicts(on, iou, gate)

    def set_scene(self, scene: int) -> None:
        self.as_group().set_scene(0, scene)

    def conflicts(self) -> dict:
        return self.as_group().conflicts(0)

    def export_state(self) -> bytes:
        """vt_export_state: this tracker's stream as a snapshot (state, refresh policy, current template rows) - what a
        later VitTrack of the same input geometry, in any process and on any checkpoint, resumes from with import_state"""
        return _export_snapshot(lib().vt_export_state, self._h)

    def import_state(self, blob) -> None:
        """vt_import_state: become the stream the snapshot was exported from; the next update continues its track"""
        raw = bytes(blob)
        _check(lib().vt_import_state(self._h, raw, len(raw)))

    # device-resident frames (pointers into this GPU's HBM, e.g. torch tensors' data_ptr())
    def init_nv12_device(self, d_y, d_uv, w, h, y_stride, uv_stride, bbox: BBox):
        _check(lib().vt_init_nv12_device(self._h, d_y, d_uv, w, h, y_stride, uv_stride, bbox._c()))

    def update_nv12_device(self, d_y, d_uv, w, h, y_stride, uv_stride) -> TrackResult:
        r = CResult()
        _check(lib().vt_update_nv12_device(self._h, d_y, d_uv, w, h, y_stride, uv_stride,
                                           byref(r)))
        return TrackResult(r)

    def init_device(self, frame: "CFrame", bbox: BBox):
        """any vt_pixfmt resident in this GPU's HBM (frame_nv12, frame_bgrx, ...): vt_init_frame(on_device=1)"""
        _check(lib().vt_init_frame(self._h, byref(frame), 1, bbox._c()))

    def update_device(self, frame: "CFrame") -> TrackResult:
        r = CResult()
        _check(lib().vt_update_frame(self._h, byref(frame), 1, byref(r)))
        return TrackResult(r)

    def init_rgb8_device(self, d_rgb, w, h, stride, bbox: BBox):
        _check(lib().vt_init_rgb8_device(self._h, d_rgb, w, h, stride, bbox._c()))

    def update_rgb8_device(self, d_rgb, w, h, stride) -> TrackResult:
        r = CResult()
        _check(lib().vt_update_rgb8_device(self._h, d_rgb, w, h, stride, byref(r)))
        return TrackResult(r)


def _chip_info_dict(ci: "CChipInfo") -> dict:
    return dict(status=int(ci.status), frames_done=int(ci.frames_done), success=int(ci.success), score=float(ci.score),
                box=tuple(int(v) for v in ci.box), geo=tuple(float(v) for v in ci.geo))


def _chip_norms(kind, norm_a, norm_b):
    if int(kind) == CHIP_RGB8 and norm_a is None and norm_b is None:
        return None, None
    return (c_float * 3)(*[float(v) for v in norm_a]), (c_float * 3)(*[float(v) for v in norm_b])


def _chip_array(size: int, kind: int, n: int):
    """host array for n chips: bf16 chips as their uint16 bit patterns [n, 3, C, C], u8 chips as [n, C, C, 3]"""
    import numpy as np
    if int(kind) == CHIP_NORM_BF16:
        return np.zeros((n, 3, size, size), np.uint16)
    return np.zeros((n, size, size, 3), np.uint8)


def _chip_shape(group_handle):
    """(C, kind, stride, device address of the chips, of the infos) of a chip-capable engine, from vt_group_chips_device:
    the stride is 6 C^2 (bf16) or 3 C^2 (u8), and no 6 C^2 equals a 3 C'^2, so it names both"""
    p, st, inf = c_void_p(), c_size_t(), c_void_p()
    _check(lib().vt_group_chips_device(group_handle, byref(p), byref(st), byref(inf)))
    stride = int(st.value)
    c = int(round((stride / 3) ** 0.5))
    if 3 * c * c == stride and c % 8 == 0:
        size, kind = c, CHIP_RGB8
    else:
        size, kind = int(round((stride / 6) ** 0.5)), CHIP_NORM_BF16
    return size, kind, stride, int(p.value or 0), int(inf.value or 0)


class DeviceChips:
    """The chip store of a group as a device array: `__cuda_array_interface__` over vt_group_chips_device, so that
    torch.as_tensor(g.chips_device(), device="cuda") is a view of the store - [B, 3, C, C] int16 (the bf16 bit patterns:
    .view(torch.bfloat16)) or [B, C, C, 3] uint8 - without a copy. `infos` is the device address of the [B] vt_chip_info
    records. Contents: those of the last pass once wait / wait_next / a synchronous update has returned, until the next
    enqueue."""

    def __init__(self, ptr: int, stride: int, infos: int, n: int, size: int, kind: int):
        self.ptr, self.stride, self.infos, self.n, self.size, self.kind = ptr, stride, infos, n, size, kind
        bf = kind == CHIP_NORM_BF16
        self.__cuda_array_interface__ = dict(
            shape=(n, 3, size, size) if bf else (n, size, size, 3), typestr="<i2" if bf else "|u1",
            data=(ptr, False), version=2, strides=None)


def _refresh_stats_dict(st: "CRefreshStats") -> dict:
    return dict(period=int(st.period), min_score=float(st.min_score), generation=int(st.generation),
                last_frame=int(st.last_frame), skipped_geometry=int(st.skipped_geometry))


def frame_nv12(d_y, d_uv, w, h, y_stride=None, uv_stride=None, matrix=COLOR_BT601, full_range=False) -> CFrame:
    return CFrame(d_y, d_uv, w, h, y_stride or w, uv_stride or ((w + 1) & ~1), frame_format(PIX_NV12, matrix, full_range), 0, 0, 0, 0, 0)


def frame_yuy2(d_yuy2, w, h, stride=None, matrix=COLOR_BT601, full_range=False) -> CFrame:
    return CFrame(d_yuy2, None, w, h, stride or 2 * w, 0, frame_format(PIX_YUY2, matrix, full_range), 0, 0, 0, 0, 0)


def frame_rgb8(d_rgb, w, h, stride=None) -> CFrame:
    return CFrame(d_rgb, None, w, h, stride or 3 * w, 0, PIX_RGB8, 0, 0, 0, 0, 0)


def frame_bgr8(d_bgr, w, h, stride=None) -> CFrame:
    return CFrame(d_bgr, None, w, h, stride or 3 * w, 0, PIX_BGR8, 0, 0, 0, 0, 0)


def frame_rgbx(d_rgbx, w, h, stride=None) -> CFrame:
    return CFrame(d_rgbx, None, w, h, stride or 4 * w, 0, PIX_RGBX, 0, 0, 0, 0, 0)


def frame_bgrx(d_bgrx, w, h, stride=None) -> CFrame:
    return CFrame(d_bgrx, None, w, h, stride or 4 * w, 0, PIX_BGRX, 0, 0, 0, 0, 0)


def frame_nv21(d_y, d_vu, w, h, y_stride=None, vu_stride=None, matrix=COLOR_BT601, full_range=False) -> CFrame:
    return CFrame(d_y, d_vu, w, h, y_stride or w, vu_stride or ((w + 1) & ~1), frame_format(PIX_NV21, matrix, full_range), 0, 0, 0, 0, 0)


def frame_uyvy(d_uyvy, w, h, stride=None, matrix=COLOR_BT601, full_range=False) -> CFrame:
    return CFrame(d_uyvy, None, w, h, stride or 2 * w, 0, frame_format(PIX_UYVY, matrix, full_range), 0, 0, 0, 0, 0)


def frame_i420(d_y, d_u, w, h, y_stride=None, c_stride=None, matrix=COLOR_BT601, full_range=False) -> CFrame:
    """d_u: the U plane; the V plane lies c_stride * ceil(h / 2) bytes behind it"""
    return CFrame(d_y, d_u, w, h, y_stride or w, c_stride or (w + 1) // 2, frame_format(PIX_I420, matrix, full_range), 0, 0, 0, 0, 0)


def frame_yv12(d_y, d_v, w, h, y_stride=None, c_stride=None, matrix=COLOR_BT601, full_range=False) -> CFrame:
    """d_v: the V plane; the U plane lies c_stride * ceil(h / 2) bytes behind it"""
    return CFrame(d_y, d_v, w, h, y_stride or w, c_stride or (w + 1) // 2, frame_format(PIX_YV12, matrix, full_range), 0, 0, 0, 0, 0)


def frame_p010(d_y, d_uv, w, h, y_stride=None, uv_stride=None, matrix=COLOR_BT601, full_range=False) -> CFrame:
    """strides in bytes"""
    return CFrame(d_y, d_uv, w, h, y_stride or 2 * w, uv_stride or 2 * ((w + 1) & ~1), frame_format(PIX_P010, matrix, full_range), 0, 0, 0, 0, 0)


def frame_nv16(d_y, d_uv, w, h, y_stride=None, uv_stride=None, matrix=COLOR_BT601, full_range=False) -> CFrame:
    return CFrame(d_y, d_uv, w, h, y_stride or w, uv_stride or w, frame_format(PIX_NV16, matrix, full_range), 0, 0, 0, 0, 0)


def frame_gray8(d_y, w, h, stride=None) -> CFrame:
    return CFrame(d_y, None, w, h, stride or w, 0, PIX_GRAY8, 0, 0, 0, 0, 0)


def frame_xrgb(d_xrgb, w, h, stride=None) -> CFrame:
    return CFrame(d_xrgb, None, w, h, stride or 4 * w, 0, PIX_XRGB, 0, 0, 0, 0, 0)


def frame_xbgr(d_xbgr, w, h, stride=None) -> CFrame:
    return CFrame(d_xbgr, None, w, h, stride or 4 * w, 0, PIX_XBGR, 0, 0, 0, 0, 0)


class Group:
    """B independent tracked streams batched on one GPU (vt_group_*)."""

    def __init__(self, weights_path: str | None = None, n_streams: int = 1, device: int = 0,
                 success_threshold: float = -1.0, use_graph: bool = True,
                 device_blob: tuple[int, int] | None = None, max_device_mib: int = 0,
                 host_window_margin_pct: int = 0, host_zero_copy: int = 0):
        self._h = c_void_p()
        self._owner = None
        self._keep = {}
        cfg = make_config(success_threshold, use_graph, n_streams, max_device_mib=max_device_mib,
                          host_window_margin_pct=host_window_margin_pct, host_zero_copy=host_zero_copy)
        if device_blob is not None:
            ptr, nbytes = device_blob
            _check(lib().vt_group_create_from_device_blob(ptr, nbytes, device, byref(cfg),
                                                          byref(self._h)))
        else:
            _check(lib().vt_group_create(weights_path.encode(), device, byref(cfg),
                                         byref(self._h)))
        self._own = True

    @classmethod
    def _view(cls, handle, owner):
        g = cls.__new__(cls)
        g._h = c_void_p(handle)
        g._owner = owner
        g._own = False
        return g

    def close(self):
        try:
            if getattr(self, "_own", False) and self._h.value:
                lib().vt_group_destroy(self._h)
            self._h = c_void_p()
        except TypeError:      # interpreter shutdown: module globals are already None
            pass

    __del__ = close

    @property
    def streams(self) -> int:
        return lib().vt_group_streams(self._h)

    def model_info(self) -> CModelInfo:
        mi = CModelInfo()
        _check(lib().vt_group_get_model_info(self._h, byref(mi)))
        return mi

    def hip_stream(self) -> int:
        return lib().vt_group_hip_stream(self._h)

    def init_device(self, stream: int, frame: CFrame, bbox: BBox):
        _check(lib().vt_group_init_device(self._h, stream, byref(frame), bbox._c()))

    @staticmethod
    def _arr(frames):
        arr = (CFrame * len(frames))(*frames)
        return arr

    @staticmethod
    def _streams(streams, n):
        """int32 array of a subset pass's stream indices (the library checks them)"""
        s = [int(i) for i in streams]
        if len(s) != n:
            raise VtError(-1, f"{len(s)} stream indices for {n} frames")
        return (c_int32 * max(n, 1))(*s)

    def enqueue_device(self, frames, streams=None):
        """one pass; streams=None: all streams (frames[i] feeds stream i), else frames[i] feeds streams[i]
        and no other stream is touched (vt_group_enqueue_device_streams)"""
        arr = self._arr(frames)
        if streams is None:
            _check(lib().vt_group_enqueue_device(self._h, arr, len(frames)))
        else:
            _check(lib().vt_group_enqueue_device_streams(self._h, self._streams(streams, len(frames)), arr, len(frames)))
        self._last_n = len(frames)

    def wait(self):
        """results of the last pass, as many as it had streams, in its order"""
        n = getattr(self, "_last_n", None) or self.streams
        out = (CResult * n)()
        _check(lib().vt_group_wait(self._h, out, n))
        return [TrackResult(r) for r in out]

    def update_device(self, frames, streams=None):
        arr = self._arr(frames)
        out = (CResult * len(frames))()
        if streams is None:
            _check(lib().vt_group_update_device(self._h, arr, len(frames), out))
        else:
            _check(lib().vt_group_update_device_streams(self._h, self._streams(streams, len(frames)), arr, len(frames),
                                                        out))
        self._last_n = len(frames)
        return [TrackResult(r) for r in out]

    @staticmethod
    def _host_frame(frame):
        """(CFrame with HOST pointers, keep-alive object): a frame object (NV12Frame, YUY2Frame, BGR8Frame, ...) says
        what it is through cframe(); a bare (H,W,3) array is RGB8"""
        if hasattr(frame, "cframe"):
            return frame.cframe(), frame
        a = np.ascontiguousarray(frame, np.uint8)
        h, w, _ = a.shape
        return CFrame(a.ctypes.data, None, w, h, 3 * w, 0, PIX_RGB8, 0, 0, 0, 0, 0), a

    def init_host(self, stream: int, frame, bbox: BBox):
        f, keep = self._host_frame(frame)
        _check(lib().vt_group_init_host(self._h, stream, byref(f), bbox._c()))

    def update_host(self, frames, streams=None):
        """one pass on HOST frames (RGB arrays / NV12Frame / YUY2Frame, one per stream - or one per
        listed stream with `streams`): only the search windows cross PCIe, in one copy"""
        pairs = [self._host_frame(fr) for fr in frames]
        arr = (CFrame * len(pairs))(*[p[0] for p in pairs])
        out = (CResult * len(pairs))()
        if streams is None:
            _check(lib().vt_group_update_host(self._h, arr, len(pairs), out))
        else:
            _check(lib().vt_group_update_host_streams(self._h, self._streams(streams, len(pairs)), arr, len(pairs), out))
        self._last_n = len(pairs)
        return [TrackResult(r) for r in out]

    @staticmethod
    def _cands(cands):
        """CCandidate array of a candidate pass: items are CCandidate, a stream index, or (stream, box or None)"""
        arr = (CCandidate * max(len(cands), 1))()
        for i, c in enumerate(cands):
            if isinstance(c, CCandidate):
                arr[i] = c
                continue
            s, box = c if isinstance(c, (tuple, list)) else (c, None)
            arr[i].stream = int(s)
            if box is not None:
                arr[i].has_box = 1
                arr[i].box = (c_float * 4)(*[float(v) for v in box])
        return arr

    def update_device_candidates(self, cands, frames):
        """one candidate pass (vt_group_update_device_candidates): slot i is cands[i] - a stream index, or (stream, box) -
        on frames[i]; a stream may fill several slots, each an independent update around its own box, and only the
        stream's best slot is committed. Returns (results by slot, winners: the winning slot of slot i's stream)."""
        n = len(frames)
        if len(cands) != n:
            raise VtError(-1, f"{len(cands)} candidates for {n} frames")
        out, win = (CResult * max(n, 1))(), (c_int32 * max(n, 1))()
        _check(lib().vt_group_update_device_candidates(self._h, self._cands(cands), self._arr(frames), n, out, win))
        self._last_n = n
        return [TrackResult(out[i]) for i in range(n)], [int(win[i]) for i in range(n)]

    def update_host_candidates(self, cands, frames):
        """the same on HOST frames (vt_group_update_host_candidates): slots that are given the same frame object's
        buffer are staged once, as the bounding rectangle of their windows"""
        n = len(frames)
        if len(cands) != n:
            raise VtError(-1, f"{len(cands)} candidates for {n} frames")
        pairs = [self._host_frame(fr) for fr in frames]
        arr = (CFrame * max(n, 1))(*[p[0] for p in pairs])
        out, win = (CResult * max(n, 1))(), (c_int32 * max(n, 1))()
        _check(lib().vt_group_update_host_candidates(self._h, self._cands(cands), arr, n, out, win))
        self._last_n = n
        return [TrackResult(out[i]) for i in range(n)], [int(win[i]) for i in range(n)]

    def reacquire(self, stream: int, frame, box_wh=None, overlap_pct: int = 50, host: bool = False, proposals: bool = False):
        """Look for a lost stream's target over the whole frame: the windows of scan_windows, in grid order, in candidate
        passes of `streams` slots each; stops at the first chunk whose winner succeeds and returns that result, or the
        last chunk's winner if none does. box_wh: the (w, h) of the candidate boxes, default the size of the stream's
        state box. Each chunk is one update of the stream. frame: a CFrame of device memory, or with host=True a host
        frame object. `last_scan` keeps every chunk's (results, winners) for inspection.
        proposals=True (a proposals-capable engine, set_proposals): first ONE candidate pass over the boxes the stream's
        record lists - written by its last device pass, the failed update as a rule - and the scan only if there are none
        or that pass's winner fails too. `last_proposal_pass` keeps its (results, winners), None if none ran."""
        self.last_scan = []
        self.last_proposal_pass = None
        fn = self.update_host_candidates if host else self.update_device_candidates
        if proposals:
            rec = self.proposals(stream)
            listed = [p["box"] for p in rec["proposals"]][:self.streams] if rec["status"] == 1 else []
            if listed:
                res, win = fn([(stream, b) for b in listed], [frame] * len(listed))
                self.last_proposal_pass = (res, win)
                if res[win[0]].success:
                    return res[win[0]]
        if box_wh is None:
            box_wh = self.read_state(stream)["box"][2:4]
        cf = self._host_frame(frame)[0] if host else frame
        boxes = scan_windows(cf.width, cf.height, float(box_wh[0]), float(box_wh[1]), overlap_pct)
        step, best = self.streams, None
        for c0 in range(0, len(boxes), step):
            chunk = boxes[c0:c0 + step]
            cands = [(stream, b) for b in chunk]
            res, win = fn(cands, [frame] * len(chunk))
            self.last_scan.append((res, win))
            best = res[win[0]]
            if best.success:
                break
        return best

    def enqueue_init_host(self, stream: int, frame, bbox: BBox):
        """(re)initialise `stream` behind the outstanding pipelined passes without waiting for them
        (vt_group_enqueue_init_host); the stream must be in none of them. The frame is consumed before this returns."""
        f, keep = self._host_frame(frame)
        _check(lib().vt_group_enqueue_init_host(self._h, stream, byref(f), bbox._c()))

    def enqueue_host(self, frames, streams=None):
        """pipelined host pass: returns once the windows are packed and the upload + pass are
        enqueued; collect with wait_next(). streams=None: all streams (frames[i] feeds stream i), else
        frames[i] feeds streams[i] and no other stream is touched (vt_group_enqueue_host_streams). The frames
        must stay alive and unchanged until then (this wrapper keeps references)."""
        pairs = [self._host_frame(fr) for fr in frames]
        arr = (CFrame * max(len(pairs), 1))(*[p[0] for p in pairs])
        if streams is None:
            _check(lib().vt_group_enqueue_host(self._h, arr, len(pairs)))
        else:
            _check(lib().vt_group_enqueue_host_streams(self._h, self._streams(streams, len(pairs)), arr, len(pairs)))
        self._last_n = None       # the results of a pipelined pass come from wait_next()
        if not hasattr(self, "_keep") or self._keep is None:
            self._keep = {}
        # the frames and the size of every outstanding pass, oldest first
        self._keep[self._keep.get("seq", 0)] = pairs
        self._keep["seq"] = self._keep.get("seq", 0) + 1

    def wait_next(self):
        """results of the oldest uncollected pipelined pass, as many as it had streams, in its order"""
        keep = getattr(self, "_keep", None) or {}
        pairs = keep.get(keep.get("done", 0))
        n = len(pairs) if pairs else self.streams
        out = (CResult * n)()
        _check(lib().vt_group_wait_next(self._h, out, n))
        if keep:
            done = keep.get("done", 0)
            keep.pop(done, None)
            keep["done"] = done + 1
        return [TrackResult(r) for r in out]

    def set_template_refresh(self, period: int, min_score: float = 0.5, stream: int | None = None) -> None:
        """vt_group_set_template_refresh: the refresh policy of `stream` (None: every stream). period 0 switches it off;
        otherwise the device re-cuts the stream's template from the frame of an update, at the box that update returned,
        once at least `period` (>= 2) updates have passed since the last refresh, the update succeeded with score >=
        min_score and the new template crop lies inside the search crop that update sampled - inside the pass, on every
        kind of pass, the pipelined ones included. Exactly init(stream, that frame, that box) as far as the template
        goes. The first enabling makes the engine refresh-capable (a second template buffer per stream, graphs
        recaptured); refused while a pipelined pass is outstanding."""
        _check(lib().vt_group_set_template_refresh(self._h, -1 if stream is None else int(stream), int(period),
                                                   float(min_score)))

    def template_refresh_stats(self, stream: int = 0) -> dict:
        """vt_group_template_refresh_stats: period, min_score, generation (refreshes since init), last_frame (frames_done
        at the last one), skipped_geometry (due refreshes skipped by the geometry rule)"""
        st = CRefreshStats()
        _check(lib().vt_group_template_refresh_stats(self._h, int(stream), byref(st)))
        return _refresh_stats_dict(st)

    def snapshot_bytes(self) -> int:
        return int(lib().vt_group_snapshot_bytes(self._h))

    def export_stream(self, stream: int) -> bytes:
        """vt_group_export_stream: the stream's state record, refresh policy and current template rows as one
        self-contained byte string (layout: include/vittrack_hip.h, snapshot.py). The stream is not changed."""
        return _export_snapshot(lib().vt_group_export_stream, self._h, int(stream))

    def import_stream(self, stream: int, blob) -> None:
        """vt_group_import_stream: make `stream` what the snapshot's stream was when it was exported - any slot of any
        engine of the same input geometry, whatever its weights. With pipelined passes outstanding the import is
        queued behind them (the stream must be in none), like enqueue_init_host."""
        raw = bytes(blob)
        _check(lib().vt_group_import_stream(self._h, int(stream), raw, len(raw)))

    def copy_stream(self, stream: int, dst: "Group", dst_stream: int) -> None:
        """vt_group_copy_stream: export + import without a host buffer - device to device when both engines are on
        one GPU, through pinned staging otherwise; dst may be this group (another slot)"""
        _check(lib().vt_group_copy_stream(self._h, int(stream), dst._h, int(dst_stream)))

    def enable_chips(self, size: int, kind: int = CHIP_NORM_BF16, norm_a=(1.0, 1.0, 1.0), norm_b=(0.0, 0.0, 0.0)) -> None:
        """vt_group_enable_chips: make the engine cut target chips - a resized crop of a stream's frame at the box its
        update committed, on the device, inside the pass. size: the chip side C (a multiple of 8, 32..512); kind:
        CHIP_NORM_BF16 (planar [3][C][C] bf16 = v * norm_a[c] + norm_b[c], the caller's normalisation) or CHIP_RGB8 (packed
        [C][C][3] u8, norms ignored). Fixed for the engine by the first call, which allocates the store (within
        max_device_mib) and recaptures the graphs; refused while a pipelined pass is outstanding. Streams cut nothing
        until set_chips gives them a factor."""
        a, b = _chip_norms(kind, norm_a, norm_b)
        _check(lib().vt_group_enable_chips(self._h, int(size), int(kind), a, b))

    def set_chips(self, factor: float, period: int = 1, phase: int = 0, stream: int | None = None) -> None:
        """vt_group_set_chips: the chip policy of `stream` (None: every stream). factor 0 switches it off; otherwise (0.5..4)
        the crop side is factor * sqrt(w * h) of the new box and a chip is cut after every update whose frames_done %
        period == phase - also after a failed one, at the last good box (info["success"] says so)."""
        _check(lib().vt_group_set_chips(self._h, -1 if stream is None else int(stream), float(factor), int(period), int(phase)))

    def read_chips(self, streams=None):
        """vt_group_read_chips: the chips and infos of `streams` (None: all) as the last pass left them -> (ndarray, [dict]).
        bf16 chips come as their uint16 bit patterns [n, 3, C, C], u8 chips as [n, C, C, 3]. A chip is current only where
        its info has status 1 (0: not due, 2: due but skipped by the geometry rule - the bytes are then those of an earlier
        cut and not to be used). Size and kind come from the engine, so any wrapper of an enabled engine can read."""
        size, kind, _, _, _ = _chip_shape(self._h)
        lst = list(range(self.streams)) if streams is None else [int(v) for v in streams]
        n = len(lst)
        out, infos = _chip_array(size, kind, max(n, 1)), (CChipInfo * max(n, 1))()
        if n:
            _check(lib().vt_group_read_chips(self._h, (c_int * n)(*lst), n, out.ctypes.data, out[0].nbytes, infos))
        return out[:n], [_chip_info_dict(infos[i]) for i in range(n)]

    def chips_device(self) -> "DeviceChips":
        """vt_group_chips_device: the store as a device array for a consumer on the same GPU (DeviceChips)"""
        size, kind, stride, ptr, infos = _chip_shape(self._h)
        return DeviceChips(ptr, stride, infos, self.streams, size, kind)

    def set_peaks(self, max_peaks: int, radius: int = 2, min_resp: float = 0.0, stream: int | None = None) -> None:
        """vt_group_set_peaks: the response-peaks policy of `stream` (None: every stream). max_peaks 0 switches it off, else
        (1..8) every pass lists up to that many maxima of the stream's Hann-weighted score map with their decoded boxes:
        greedy, each peak suppressing the (2 radius + 1)^2 square of cells around it (radius 1..4); a peak behind the first
        needs a response of at least min_resp (0..1). The first call with max_peaks > 0 makes the engine peaks-capable
        (records within max_device_mib, graphs recaptured); refused while a pipelined pass is outstanding."""
        _check(lib().vt_group_set_peaks(self._h, -1 if stream is None else int(stream), int(max_peaks), int(radius), float(min_resp)))

    def last_peaks(self, n: int | None = None):
        """vt_group_last_peaks: the records of the pass whose results the last wait / wait_next / synchronous update
        returned, in that pass's slot order -> PEAKS_DTYPE array [n] (None: one per stream; entries beyond the pass's size stay
        zero). rec["n"] == 0: the slot's stream has the policy off, or the slot lost a candidate pass. A peak's box (x1, y1,
        w, h floats) can be passed to a candidate slot as it is."""
        n = self.streams if n is None else int(n)
        out = np.zeros(max(n, 1), PEAKS_DTYPE)
        _check(lib().vt_group_last_peaks(self._h, out.ctypes.data if n > 0 else None, n))
        return out[:n]

    def set_result_overlay(self, rect: bool = True, crosshair: bool = True, score: bool = True, thickness: int | None = None,
                           size: int | None = None, scale: int | None = None, luma: int | None = None, rgb: int | None = None,
                           min_score_pct: int | None = None) -> None:
        """the "result_overlay*" keys of vt_group_set_tuning: every DEVICE-frame pass of this engine ends by drawing each
        stream's new box into its frame - a rectangle (thickness 1..16), a crosshair at the centre (size 1..64) and the
        text "score: N%" (scale 1..4) - where the result succeeds with score > min_score_pct / 100. luma (0..255): the
        brightness on luma surfaces and of the text everywhere; rgb (0xRRGGBB): rectangle and crosshair on packed RGB.
        None keeps a value (style: the reference's 3 / 15 / 2 unless all three were set before). All three shapes off
        stops the drawing. The first enable makes the engine overlay-capable (graphs recaptured); such an engine WRITES
        the frames its device passes are given. Refused while a pipelined pass is outstanding."""
        for key, v in (("result_overlay_luma", luma), ("result_overlay_rgb", rgb), ("result_overlay_min_score_pct", min_score_pct)):
            if v is not None:
                if int(v) < 0:
                    raise ValueError(f"{key}: {v}")
                self.set_tuning(key, int(v))
        if thickness is not None or size is not None or scale is not None:
            st = getattr(self, "_overlay_style", (3, 15, 2))
            st = tuple(int(n) if n is not None else o for n, o in zip((thickness, size, scale), st))
            if min(st) < 0 or st[0] > 255 or st[1] > 255:
                raise ValueError(f"result_overlay_style: {st}")
            self.set_tuning("result_overlay_style", st[0] | st[1] << 8 | st[2] << 16)
            self._overlay_style = st
        self.set_tuning("result_overlay", (1 if rect else 0) | (2 if crosshair else 0) | (4 if score else 0))

    def result_overlay_stats(self, stream: int = 0) -> dict:
        """vt_group_read_tensor "result_overlay": the engine's flags and the stream's counters since the first enable -
        drawn (by the stream's last pass), n_drawn, n_gated (score gate), n_unsupported (P010), last_n (N of the last
        label drawn)"""
        v = self.read_tensor("result_overlay", stream)
        return dict(zip(("flags", "drawn", "n_drawn", "n_gated", "n_unsupported", "last_n"), (int(x) for x in v)))

    def set_motion_prior(self, on: bool = True, gain_pct: int | None = None, coast: int | None = None,
                         max_pct: int | None = None) -> None:
        """the "motion_*" keys of vt_group_set_tuning: every pass of this engine first moves each of its streams' boxes by
        a per-stream velocity estimate kept on the device, so the search window is cut where the target is heading, and
        keeps the box moving through `coast` (0..60) failed updates. gain_pct (1..100): weight of the newest displacement;
        max_pct (0..200): per-axis limit of the velocity in percent of sqrt(w*h) of the new box. None keeps a value. The
        first enable makes the engine motion-capable (graphs recaptured, two more launches per pass from then on); on=False
        zeroes every stream's record. Refused while a pipelined pass is outstanding."""
        for key, v in (("motion_gain_pct", gain_pct), ("motion_coast", coast), ("motion_max_pct", max_pct)):
            if v is not None:
                if int(v) < 0:
                    raise ValueError(f"{key}: {v}")
                self.set_tuning(key, int(v))
        self.set_tuning("motion_prior", 1 if on else 0)

    def motion(self, stream: int = 0) -> dict:
        """vt_group_read_tensor "motion": the engine flag and the stream's record - on, v (vx, vy), live, shift (of the
        stream's last pass), n_shift (passes with a non-zero shift), n_coast (failed updates that advanced the box)"""
        v = self.read_tensor("motion", stream)
        return dict(on=int(v[0]), v=(float(v[1]), float(v[2])), live=int(v[3]), shift=(float(v[4]), float(v[5])),
                    n_shift=int(v[6]), n_coast=int(v[7]))

    def set_appearance(self, on: bool = True, period: int | None = None, gate: float | None = None) -> None:
        """the "appearance*" keys of vt_group_set_tuning: every pass of this engine cuts a template-sized crop at each
        stream's new box (the probe) and scores it against the rows the stream was started from (the anchor): zero-mean
        normalised correlation, 1 = the same pixels. period (1..1,000,000): evaluated when frames_done % period == 0; gate
        (0..1, stored per mille): a template refresh additionally needs similarity >= gate, 0 = report only. None keeps a
        value. The first enable makes the engine appearance-capable (graphs recaptured, two more launches per pass from then
        on). Refused while a pipelined pass is outstanding."""
        if period is not None:
            if int(period) < 0:
                raise ValueError(f"appearance_period: {period}")
            self.set_tuning("appearance_period", int(period))
        if gate is not None:
            if not 0.0 <= float(gate) <= 1.0:
                raise ValueError(f"appearance gate: {gate}")
            self.set_tuning("appearance_gate_pm", int(round(float(gate) * 1000.0)))
        self.set_tuning("appearance", 1 if on else 0)

    def set_anchor(self, stream: int = -1) -> None:
        """the "appearance_anchor" action: the stream's (-1: every initialised stream's) anchor becomes its CURRENT template"""
        self.set_tuning("appearance_anchor", int(stream))

    def appearance(self, stream: int = 0) -> dict:
        """vt_group_read_tensor "appearance": the engine flag, the stream's record of its last pass - status (0 not due or
        not evaluated, 1 evaluated, 2 the crop left the sampled search crop, 3 a flat anchor or probe), similarity,
        frames_done - and its counters (evaluated; gated: refreshes the gate refused), the period and the gate per mille"""
        v = self.read_tensor("appearance", stream)
        return dict(on=int(v[0]), status=int(v[1]), similarity=float(v[2]), frames_done=int(v[3]), evaluated=int(v[4]),
                    gated=int(v[5]), period=int(v[6]), gate_pm=int(v[7]))

    def anchor(self, stream: int = 0) -> np.ndarray:
        """vt_group_read_tensor "anchor": the [Nt * Kpad] rows the stream's probes are compared with"""
        return self.read_tensor("anchor", stream)

    def probe(self, stream: int = 0) -> np.ndarray:
        """vt_group_read_tensor "probe": the rows of the stream's last cut probe (valid where the record's status is 1 or 3)"""
        return self.read_tensor("probe", stream)

    def set_proposals(self, mode: int = 1, period: int | None = None, max_n: int | None = None, min_sim: float | None = None,
                      max_cells: int | None = None) -> None:
        """the "proposals*" keys of vt_group_set_tuning: behind the decode of every device pass the engine slides each due
        stream's own template, pooled to an M x M pattern, over a coarse thumbnail of the whole frame and lists the best
        places as boxes of the stream's size (proposals()). mode 0 off, 1 streams whose update failed, 2 every update;
        period (1..1,000,000): due when frames_done % period == 0; max_n (1..8) proposals listed; min_sim (0..1, stored
        per mille): the least similarity listed; max_cells (16,384..4,194,304): thumbnail cells per slot, before the first
        enable only. None keeps a value. The first non-zero mode makes the engine proposals-capable (graphs recaptured, four
        more launches per pass from then on). Refused while a pipelined pass is outstanding."""
        if max_cells is not None:
            self.set_tuning("proposals_max_cells", int(max_cells))
        if period is not None:
            if int(period) < 0:
                raise ValueError(f"proposals_period: {period}")
            self.set_tuning("proposals_period", int(period))
        if max_n is not None:
            if int(max_n) < 0:
                raise ValueError(f"proposals_max: {max_n}")
            self.set_tuning("proposals_max", int(max_n))
        if min_sim is not None:
            if not 0.0 <= float(min_sim) <= 1.0:
                raise ValueError(f"proposals min_sim: {min_sim}")
            self.set_tuning("proposals_min_sim_pm", int(round(float(min_sim) * 1000.0)))
        self.set_tuning("proposals", int(mode))

    def proposals(self, stream: int = 0) -> dict:
        """vt_group_read_tensor "proposals": the policy (mode, period, max_n, min_sim_pm, max_cells), the stream's record of
        its last collected pass - status (0 not due, 1 evaluated, 2 the grid is larger than max_cells or smaller than the
        pattern, 3 a flat pattern, 4 no whole device frame), frames_done, c (cell side in pixels), grid (Wg, Hg) and the
        listed proposals, best first: dict(sim, box (x, y, w, h floats), pos) - and the counter `evaluated`"""
        v = self.read_tensor("proposals", stream)
        n = int(v[3])
        props = [dict(sim=float(v[12 + 6 * k]), box=tuple(float(x) for x in v[13 + 6 * k:17 + 6 * k]), pos=int(v[17 + 6 * k]))
                 for k in range(n)]
        return dict(mode=int(v[0]), status=int(v[1]), frames_done=int(v[2]), n=n, c=float(v[4]), grid=(int(v[5]), int(v[6])),
                    evaluated=int(v[7]), period=int(v[8]), max_n=int(v[9]), min_sim_pm=int(v[10]), max_cells=int(v[11]),
                    proposals=props)

    def proposals_pattern(self, stream: int = 0) -> np.ndarray:
        """vt_group_read_tensor "proposals_pattern": the [M, M] pattern (integers in floats) the stream's last pass pooled"""
        v = self.read_tensor("proposals_pattern", stream)
        m = int(round(len(v) ** 0.5))
        return v.reshape(m, m)

    def proposals_map(self, stream: int = 0) -> np.ndarray:
        """vt_group_read_tensor "proposals_map": the [Hg - M + 1, Wg - M + 1] similarity map of the stream's last pass"""
        wg, hg = self.proposals(stream)["grid"]
        v = self.read_tensor("proposals_map", stream)
        m = self.proposals_pattern(stream).shape[0]
        return v.reshape(hg - m + 1, wg - m + 1)

    def set_conflicts(self, on: bool = True, iou: float | None = None, gate: bool | None = None) -> None:
        """the "conflicts*" keys of vt_group_set_tuning: behind the decode of every pass the engine records, per stream, which
        other streams of the same pass and the same scene (set_scene) overlap its new box - IoU at or over `iou` (0.001..1,
        stored per mille) - and lists the up to four largest. gate True: a stream with such a partner does not refresh its
        template in that pass (refresh rule 9). None keeps a value. The first enable makes the engine conflicts-capable
        (graphs recaptured, one more launch per pass from then on). Refused while a pipelined pass is outstanding."""
        if iou is not None:
            if not 0.001 <= float(iou) <= 1.0:
                raise ValueError(f"conflicts iou: {iou}")
            self.set_tuning("conflicts_iou_pm", int(round(float(iou) * 1000.0)))
        if gate is not None:
            self.set_tuning("conflicts_gate", 1 if gate else 0)
        self.set_tuning("conflicts", 1 if on else 0)

    def set_scene(self, stream: int | None, scene: int) -> None:
        """the "conflicts_scene" action: `stream` (None: every stream) shows picture `scene` (0..32767; 0, the default:
        compared with nobody). The records of the streams it names are zeroed. Needs a conflicts-capable engine."""
        st = 0xFFFF if stream is None else int(stream)
        if not (0 <= st <= 0xFFFF and 0 <= int(scene) <= 0x7FFF):
            raise ValueError(f"set_scene: stream {stream}, scene {scene}")
        self.set_tuning("conflicts_scene", st | int(scene) << 16)

    def conflicts(self, stream: int = 0) -> dict:
        """vt_group_read_tensor "conflicts": the engine flag, the stream's record of its last collected pass - status (0 no
        pass wrote it, 1 evaluated and alone, 2 evaluated with partners over the threshold, 3 not eligible), frames_done,
        n_over and the listed partners, largest IoU first: (stream, iou) -, its counters (evaluated, conflicting; gated:
        refreshes rule 9 refused) and its scene"""
        v = self.read_tensor("conflicts", stream)
        partners = [(int(v[4 + k]), float(v[8 + k])) for k in range(4) if int(v[4 + k]) >= 0]
        return dict(on=int(v[0]), status=int(v[1]), frames_done=int(v[2]), n_over=int(v[3]), partners=partners,
                    partner=[int(x) for x in v[4:8]], iou=np.asarray(v[8:12], np.float32).copy(), evaluated=int(v[12]),
                    conflicting=int(v[13]), gated=int(v[14]), scene=int(v[15]))

    def set_health(self, on: bool = True, gate: bool | None = None, **keys) -> None:
        """the "health*" keys of vt_group_set_tuning: behind the decode of every pass the engine takes a thumbnail of each due
        stream's whole frame, measures it and its change since the stream's previous thumbnail, and flags a FROZEN (1), FLAT
        (2) or CUT (4) picture. gate True: a flagged picture is not cut into the template in that pass (refresh rule 10).
        keys: period, cell, still_run, flat_q, cut_pm, max_cells (max_cells before the first enable only). None keeps a
        value. The first enable makes the engine health-capable (graphs recaptured, four more launches per pass from then
        on). Refused while a pipelined pass is outstanding."""
        for k, v in keys.items():
            if k not in ("period", "cell", "still_run", "flat_q", "cut_pm", "max_cells"):
                raise ValueError(f"set_health: {k}")
            self.set_tuning("health_" + k, int(v))
        if gate is not None:
            self.set_tuning("health_gate", 1 if gate else 0)
        self.set_tuning("health", 1 if on else 0)

    def frame_health(self, stream: int = 0) -> dict:
        """the stream's frame-health record of its last collected pass as exact integers (vt_group_read_tensor
        "health_words": the record's 32-bit words in 16-bit halves) - status (0 no pass wrote it, 1 measured and compared, 2
        no geometry, 4 no whole device frame, 5 measured without a comparable previous thumbnail), frames_done, flags, c, Wg,
        Hg, still, S1, S2, G, D, HD, G_ref, has_prev - plus the engine flag and the stream's counters (evaluated, flagged;
        gated: refreshes rule 10 refused) of the tensor "health".
        The thumbnail's bookkeeping follows in the words and is not returned but for has_prev"""
        h = self.read_tensor("health_words", stream).astype(np.uint32)
        w = (h[0::2] | (h[1::2] << 16)).astype(np.uint32)
        i32 = w.view(np.int32)
        i64 = w[8:20].view(np.int64)
        v = self.read_tensor("health", stream)
        return dict(on=int(v[0]), status=int(i32[0]), frames_done=int(i32[1]), flags=int(i32[2]), c=int(i32[3]), Wg=int(i32[4]),
                    Hg=int(i32[5]), still=int(i32[6]), S1=int(i64[0]), S2=int(i64[1]), G=int(i64[2]), D=int(i64[3]), HD=int(i64[4]),
                    G_ref=int(i64[5]), has_prev=int(i32[20]), evaluated=int(v[13]), flagged=int(v[14]), gated=int(v[15]))

    def set_arbitration(self, on: bool = True, **keys) -> None:
        """the "arbitrate*" keys of vt_group_set_tuning: behind the decode of every pass, where the committed box no longer
        looks like the stream's anchor (similarity below low_pm) and a runner-up peak of the response map does (at least
        high_pm), the runner-up is committed instead. keys: max, radius, min_resp_pm, low_pm, high_pm; None keeps a value. The
        first enable needs an appearance-capable engine (set_appearance first) and makes the engine arbitration-capable (graphs
        recaptured, four more launches per pass from then on). Refused while a pipelined pass is outstanding."""
        for k, v in keys.items():
            if k not in ("max", "radius", "min_resp_pm", "low_pm", "high_pm"):
                raise ValueError(f"set_arbitration: {k}")
            if v is not None:
                self.set_tuning("arbitrate_" + k, int(v))
        self.set_tuning("arbitrate", 1 if on else 0)

    def arbitration(self, stream: int = 0) -> dict:
        """the stream's arbitration record of its last collected pass (vt_group_read_tensor "arbitrate"): status (0 not due, 1
        kept, 2 switched, 3 candidate pass, 4 rule 6 failed at peak 0, 5 window miss), frames_done, n, chosen, the counters
        evaluated and switched, and peaks: n dicts of cell, status, score, resp, similarity (np.float32) and box"""
        v = self.read_tensor("arbitrate", stream)
        n = int(v[3])
        peaks = [dict(cell=int(p[0]), status=int(p[1]), score=np.float32(p[2]), resp=np.float32(p[3]), similarity=np.float32(p[4]),
                      box=np.asarray(p[5:9], np.float32).copy()) for p in (v[8 + 10 * k:18 + 10 * k] for k in range(n))]
        return dict(on=int(v[0]), status=int(v[1]), frames_done=int(v[2]), n=n, chosen=int(v[4]), evaluated=int(v[5]),
                    switched=int(v[6]), peaks=peaks)

    def graph_captures(self) -> int:
        """hipGraph captures since creation: all crop tiers are captured when the engine is created (those for formats
        other than RGB8 / NV12 / YUY2 in the first init on such a format), none inside a pass"""
        return lib().vt_group_graph_captures(self._h)

    def host_redos(self) -> int:
        return lib().vt_group_host_redos(self._h)

    def profile_device(self, frames, iters=5):
        arr = self._arr(frames)
        out = (CKernelTime * 64)()
        n = _check(lib().vt_group_profile_device(self._h, arr, len(frames), iters, out, 64))
        return [dict(name=out[i].name.decode(), launches=out[i].launches,
                     ms=float(out[i].ms_total), flops=out[i].flops, bytes=out[i].bytes)
                for i in range(n)]

    def set_state_box(self, stream: int, box):
        b = (c_float * 4)(*[float(v) for v in box])
        _check(lib().vt_group_set_state_box(self._h, stream, b))

    def enable_taps(self, on=True):
        _check(lib().vt_group_enable_taps(self._h, 1 if on else 0))

    def set_tuning(self, key: str, value: int):
        """diagnostics: alternative kernels for A/B runs (vt_group_set_tuning)"""
        _check(lib().vt_group_set_tuning(self._h, key.encode(), int(value)))

    def read_tensor(self, name: str, stream: int = 0) -> np.ndarray:
        n = _check(lib().vt_group_read_tensor(self._h, stream, name.encode(), None, 0))
        out = np.empty(n, np.float32)
        _check(lib().vt_group_read_tensor(self._h, stream, name.encode(), _f32(out), n))
        return out

    def residual_range(self, stream: int = 0) -> list:
        """vt_group_read_tensor "xrange": what the stream's stored residual pair holds, one dict per stage (with taps:
        tokens0, layer0 .. of the last pass; without: the final residual) - lo_shift, max_abs, n_sat (elements on the
        clamp, |lo8| == 127) and n_ge_pow2[k - 1] = n(|x| >= 2^k), k = 1..9. weights.recommend_lo_shift takes the list."""
        rows = self.read_tensor("xrange", stream).reshape(-1, weights.XRANGE_COLS)
        names = ["tokens0"] + [f"layer{i}" for i in range(len(rows) - 1)] if len(rows) > 1 else ["x"]
        return [dict(stage=nm, lo_shift=int(r[0]), max_abs=float(r[1]), n_sat=int(r[2]),
                     n_ge_pow2=[int(v) for v in r[3:]]) for nm, r in zip(names, rows)]

    def read_state(self, stream: int = 0) -> dict:
        raw = self.read_tensor("state", stream)
        i = raw.view(np.int32)
        return dict(box=raw[0:4].copy(), geo=raw[4:8].copy(), frame_w=int(i[8]),
                    frame_h=int(i[9]), initialized=int(i[10]), frames_done=int(i[11]),
                    success_count=int(i[12]), last_idx=int(i[13]), last_fbox=raw[14:18].copy(),
                    last_score=float(raw[18]), window_miss=int(i[19]), tpl_gen=int(i[20]), tpl_frame=int(i[21]))


# ---- reference colour converter -------------------------------------------------------------

def nv12_full_to_rgb(nv12_data: np.ndarray, width: int, height: int, device: int = 0):
    """≙ nv12_full_to_rgb_parallel (src/nv12_convert.rs:46) on the GPU -> (H,W,3) uint8"""
    buf = np.ascontiguousarray(nv12_data, np.uint8).reshape(-1)
    out = np.empty((height, width, 3), np.uint8)
    _check(lib().vt_nv12_to_rgb8(device, _u8(buf), buf.size, width, height, _u8(out)))
    return out


# ---- overlays (the reference's per-frame drawing, on the GPU) -------------------------------------

def nv12_to_rgb8_batch_device(d_nv12_ptrs, lens, w: int, h: int, d_rgb_ptrs, device: int = 0, hip_stream=None):
    """vt_nv12_to_rgb8_batch_device: n device-resident packed NV12 frames -> n RGB8 frames in one launch per 64 frames"""
    n = len(d_nv12_ptrs)
    ins = (c_void_p * n)(*[int(p) for p in d_nv12_ptrs])
    outs = (c_void_p * n)(*[int(p) for p in d_rgb_ptrs])
    ls = (c_size_t * n)(*[int(x) for x in lens])
    _check(lib().vt_nv12_to_rgb8_batch_device(device, ins, ls, n, w, h, outs, hip_stream))


def draw_cmd(kind, x=0, y=0, w=0, h=0, p=0, value=0, text="") -> CDrawCmd:
    return CDrawCmd(kind, x, y, w, h, p, value, text.encode()[:35])


def overlay_nv12(nv12: np.ndarray, width: int, height: int, cmds, device: int = 0) -> np.ndarray:
    """apply draw commands to the luma plane of a packed NV12 host buffer (returns a copy)"""
    buf = np.ascontiguousarray(nv12, np.uint8).reshape(-1).copy()
    arr = (CDrawCmd * len(cmds))(*cmds)
    _check(lib().vt_overlay_nv12(device, _u8(buf), width, height, arr, len(cmds)))
    return buf


def overlay_rgb8(rgb: np.ndarray, cmds, device: int = 0) -> np.ndarray:
    """apply draw commands to an (H,W,3) RGB8 host image (returns a copy)"""
    img = np.ascontiguousarray(rgb, np.uint8).copy()
    h, w, _ = img.shape
    arr = (CDrawCmd * len(cmds))(*cmds)
    _check(lib().vt_overlay_rgb8(device, _u8(img), w, h, arr, len(cmds)))
    return img


# ---- operator-level test hooks (include/vittrack_hip_ops.h, libvittrack_hip_ops.so): ops.py -----------
# vt.op_*, vt.ops_lib, vt.OPS_EXPORTS and the hooks' record dtypes; last, because ops.py imports the names above
from .ops import *  # noqa: E402,F401,F403

