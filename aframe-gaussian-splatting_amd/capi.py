"""ctypes binding of the C ABI (include/gs_splat.h -> csrc/libgs_splat_hip.so).

Plumbing only: every call goes straight into the HIP library.  There is no Python or CPU fallback -- if the
library is missing, or no GPU is usable, this raises.
"""
import ctypes as C
import os
import sys

import numpy as np

from . import build as _build

GS_OK = 0
E_BADARG, E_PLY_HEADER, E_PLY_PROP, E_HIP, E_OOM, E_NODEVICE, E_STATE, E_PLY_DATA, E_RETRY = -1, -2, -3, -4, -5, -6, -7, -8, -9
RENDER_FLIP_Y, RENDER_COUNT_FRAGS, RENDER_NO_EARLY_OUT, RENDER_ASYNC, RENDER_COUNT_EVALUATED = 1, 2, 4, 8, 16
RENDER_PARALLEL = 32               # a parallel-projection camera (gs_splat.h: "Parallel-projection cameras")
OPT_PROFILE, OPT_TERMINATION, OPT_NEAR_PERMILLE, OPT_RECORD_STAGED, OPT_PIPELINE_DEPTH, OPT_WIDE_PAIRS, OPT_ENQUEUE_THREADS = 1, 2, 3, 4, 5, 6, 7
OPT_COMM_SELF_COPY = 8
OPT_BLEND_SPLIT = 9
OPT_FRAME_BATCH = 10
OPT_SORT_NEAR = 11
OPT_COMM_TRANSPORT = 12
OPT_AUTO_RETRY = 13
OPT_SORT_SHARE = 15
OPT_BINNING = 16
OPT_SUBTILE = 17
OPT_ROW_WALK = 18
OPT_SH_DEGREE = 19
OPT_ANTIALIAS = 20
OPT_SEG_COUNT = 21
OPT_SORT_NEAR_FORCE = 22
OPT_HIGHLIGHT = 23
SORT_WHOLE, SORT_HISTOGRAM, SORT_SPEC, SORT_TAIL, SORT_STASH = 0, 1, 2, 3, 4     # gs_sort_info.form
TRANSPORT_RCCL, TRANSPORT_INPROC = 0, 1
COMM_ID_BYTES = 128
BUF_CENTER_SCALE, BUF_COV_COLOR, BUF_SORT_ROWS, BUF_SORTED, BUF_PROJECTED, BUF_TILE_COUNT, BUF_TILE_STATS, BUF_UNSAT_MASK = 0, 1, 2, 3, 4, 5, 6, 7
BUF_SH = 8
BUF_STATE = 9
BUF_CONTRIB = 10
STATE_HIDDEN, STATE_SELECTED = 1, 2
SELECT_INVERT = 1
PROP_X, PROP_Y, PROP_Z, PROP_RED, PROP_GREEN, PROP_BLUE, PROP_ALPHA, PROP_SIZE2 = range(8)
PROP_SEEN = 16                     # the contribution store in pixels (render_contrib); no function of the record: prop_eval refuses it
HIST_MAX_BINS = 4096

EXPORTS = [
    "gs_create", "gs_destroy", "gs_last_error", "gs_version", "gs_device_count", "gs_clear", "gs_push_splat", "gs_push_matrices", "gs_load_ply",
    "gs_ply_to_splat", "gs_ply_to_splat_gpu", "gs_count", "gs_sort", "gs_render", "gs_render_device", "gs_render_stereo", "gs_set_scene", "gs_sync",
    "gs_set_stream", "gs_frame_stream", "gs_frame_status_device", "gs_frame_lane", "gs_lane_stream", "gs_wait_stream", "gs_stream_wait_frame",
    "gs_model_view_matrix", "gs_projection_matrix", "gs_tick_uniforms", "gs_focal", "gs_scaled_size", "gs_set_option",
    "gs_get_stats", "gs_download",
    "gs_comm_unique_id", "gs_comm_init", "gs_comm_destroy", "gs_partition", "gs_render_gathered", "gs_read_gathered",
    "gs_host_alloc", "gs_host_free", "gs_sort_for", "gs_sort_gathered", "gs_gathered_size", "gs_sort_begin", "gs_sort_poll",
    "gs_create_multi", "gs_multi_destroy", "gs_multi_last_error", "gs_multi_devices", "gs_multi_ctx", "gs_multi_clear",
    "gs_multi_push_splat", "gs_multi_load_ply", "gs_multi_count", "gs_multi_set_option", "gs_multi_sort", "gs_multi_render",
    "gs_multi_render_device", "gs_multi_read", "gs_multi_sync",
    "gs_ply_sh", "gs_ply_sh_host", "gs_push_sh", "gs_sh_count", "gs_sh_eval", "gs_sh_eval_unrounded", "gs_camera_in_object", "gs_multi_push_sh",
    "gs_render_surface", "gs_render_surface_device", "gs_pick",
    "gs_antialias_factor",
    "gs_set_state", "gs_set_state_ids", "gs_state_count", "gs_select_box", "gs_select_sphere", "gs_select_rect", "gs_compact",
    "gs_sort_inspect",
    "gs_multi_set_state", "gs_multi_set_state_ids", "gs_multi_select_box", "gs_multi_select_sphere", "gs_multi_select_rect", "gs_multi_compact",
    "gs_select_mask", "gs_multi_select_mask", "gs_mask_polygon", "gs_highlight_info", "gs_highlight_word",
    "gs_prop_eval", "gs_hist_bin", "gs_prop_range", "gs_histogram", "gs_select_range",
    "gs_multi_prop_range", "gs_multi_histogram", "gs_multi_select_range",
    "gs_render_contrib", "gs_render_contrib_device", "gs_contrib_clear", "gs_contrib_info",
    "gs_export_row", "gs_export_splat", "gs_export_sh", "gs_splat_to_ply", "gs_export_ply", "gs_multi_export_splat", "gs_multi_export_ply",
    "gs_adjust_colour", "gs_adjust_word", "gs_adjust_sh_row", "gs_replace_splat", "gs_replace_sh",
    "gs_multi_adjust_colour", "gs_multi_replace_splat", "gs_multi_replace_sh",
    "gs_transform", "gs_multi_transform", "gs_transform_record", "gs_transform_records", "gs_transform_sh_row", "gs_sh_rotation", "gs_similarity_about",
    "gs_project_record", "gs_ortho_matrix", "gs_projection_info",
    "gs_cply_info", "gs_cply_to_splat", "gs_cply_sh_host", "gs_splat_to_cply", "gs_log_fixed", "gs_load_cply", "gs_cply_to_splat_gpu", "gs_export_cply",
    "gs_multi_load_cply", "gs_multi_export_cply",
]
CPLY_MORTON = 1                    # gs_splat_to_cply / gs_export_cply flags: rows in stable Morton order
SURFACE_NONE = 0xFFFFFFFF          # gs_surface.id / gs_hit.id where the transmittance never falls below one half


class Piece(C.Structure):
    _fields_ = [("view", C.c_int32), ("x0", C.c_int32), ("x1", C.c_int32), ("owner", C.c_int32)]


class RenderParams(C.Structure):
    _fields_ = [("model_view", C.c_float * 16), ("projection", C.c_float * 16), ("fb_width", C.c_int32), ("fb_height", C.c_int32),
                ("x0", C.c_int32), ("x1", C.c_int32), ("focal", C.c_float), ("background", C.c_float * 4), ("flags", C.c_uint32)]


class Stats(C.Structure):
    _fields_ = [("n_splats", C.c_uint64), ("n_sorted", C.c_uint64), ("n_visible", C.c_uint64), ("n_pairs", C.c_uint64),
                ("n_frags", C.c_uint64), ("n_tiles", C.c_uint64), ("ms_sort", C.c_float), ("ms_project", C.c_float),
                ("ms_bin", C.c_float), ("ms_blend", C.c_float), ("ms_render", C.c_float), ("blend_launches", C.c_uint32),
                ("prof_frames", C.c_uint32), ("sum_ms_sort", C.c_float), ("sum_ms_project", C.c_float), ("sum_ms_bin", C.c_float),
                ("sum_ms_blend", C.c_float), ("acc_frames", C.c_uint64), ("acc_sorted", C.c_uint64), ("acc_visible", C.c_uint64),
                ("acc_pairs", C.c_uint64), ("unsat_tiles", C.c_uint32), ("near_permille", C.c_uint32),
                ("sort_records", C.c_uint32), ("retried_frames", C.c_uint32), ("spec_sorts", C.c_uint32), ("spec_misses", C.c_uint32), ("need_splats", C.c_uint32),
                ("sort_mode", C.c_uint32), ("subtile", C.c_uint32), ("row_walk", C.c_uint32),
                ("binning", C.c_uint32), ("sh_degree", C.c_uint32), ("n_hidden", C.c_uint32), ("surface", C.c_uint32), ("antialias", C.c_uint32),
                ("seg_count", C.c_uint32), ("n_runs", C.c_uint32)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class SortInfo(C.Structure):
    _fields_ = [("form", C.c_uint32), ("near_req", C.c_uint32), ("n_kept", C.c_uint32), ("n_valid", C.c_uint32), ("n_records", C.c_uint32),
                ("order_incomplete", C.c_uint32), ("near_overflow", C.c_uint32), ("spec_fail", C.c_uint32), ("threshold_bin", C.c_uint32),
                ("reserved", C.c_uint32 * 3)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_ if n != "reserved"}


class Surface(C.Structure):
    _fields_ = [("id", C.c_void_p), ("depth", C.c_void_p), ("alpha", C.c_void_p)]


class Hit(C.Structure):
    _fields_ = [("id", C.c_uint32), ("depth", C.c_float), ("alpha", C.c_float), ("pos", C.c_float * 3)]


class ColourAdjust(C.Structure):
    """gs_colour_adjust: colour' = m (row-major 3x3) colour + offset (byte units), alpha' = alpha_scale * alpha + alpha_offset"""
    _fields_ = [("m", C.c_float * 9), ("offset", C.c_float * 3), ("alpha_scale", C.c_float), ("alpha_offset", C.c_float)]


def colour_adjust(m=None, offset=(0.0, 0.0, 0.0), alpha_scale=1.0, alpha_offset=0.0):
    """A ColourAdjust; the defaults are the identity.  m: 9 values, row-major (out channel c reads m[3c .. 3c+2])"""
    a = ColourAdjust()
    a.m[:] = [float(v) for v in np.asarray(np.eye(3) if m is None else m, np.float32).reshape(9)]
    a.offset[:] = [float(v) for v in np.asarray(offset, np.float32).reshape(3)]
    a.alpha_scale, a.alpha_offset = float(np.float32(alpha_scale)), float(np.float32(alpha_offset))
    return a


HIT_DTYPE = np.dtype([("id", np.uint32), ("depth", np.float32), ("alpha", np.float32), ("pos", np.float32, 3)])


class GsError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("gs_splat error %d: %s" % (code, msg))
        self.code = code
        self.message = msg


_lib = None


def library_path():
    return _build.LIB


def _hip_runtime_mapped():
    try:
        with open("/proc/self/maps") as f:
            return any("libamdhip64" in line for line in f)
    except OSError:
        return False


def hip_runtime():
    """ctypes handle of the HIP runtime THIS process has mapped (the one libgs_splat_hip.so talks to): for helpers that call
    hipMalloc / hipMemcpy next to the library (tests, bench.py).  dlopen("libamdhip64.so") by NAME may pick another copy than
    the one already loaded by path (torch's wheel and /opt/rocm both ship one), and memory from one is no use to the other."""
    load()
    try:
        with open("/proc/self/maps") as f:
            for line in f:
                if "libamdhip64" in line and "/" in line:
                    return C.CDLL(line[line.index("/"):].strip())
    except OSError:
        pass
    return C.CDLL("libamdhip64.so")


def load(build_if_missing=True):
    """dlopen the HIP library (building it first if absent and a compiler is present)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(_build.LIB):
        if not build_if_missing:
            raise FileNotFoundError(_build.LIB + " not built; run __graft_entry__.build()")
        _build.build_lib()
    # A process that also uses torch must have torch's HIP runtime loaded first: the wheel ships its own libamdhip64 /
    # libhsa-runtime64 under the same sonames as /opt/rocm's, the first one loaded serves both, and torch finds no GPU through the
    # other one ("No HIP GPUs are available").  Loading that ONE shared object is enough -- importing torch (1-2 s, hundreds of MB)
    # is not a ctypes loader's business; nothing happens when no torch is installed, when a HIP runtime is already mapped, or with
    # GS_SPLAT_NO_TORCH_PRELOAD set.
    if "torch" not in sys.modules and os.environ.get("GS_SPLAT_NO_TORCH_PRELOAD") is None and not _hip_runtime_mapped():
        try:
            import importlib.util
            spec = importlib.util.find_spec("torch")
            cand = os.path.join(os.path.dirname(spec.origin), "lib", "libamdhip64.so") if spec and spec.origin else None
            if cand and os.path.exists(cand):
                C.CDLL(cand, mode=C.RTLD_GLOBAL)
        except (ImportError, OSError, ValueError):
            pass
    # GS_SPLAT_LIB: load another build of the same library (A/B measurements of kernel variants); never a different backend
    L = C.CDLL(os.environ.get("GS_SPLAT_LIB") or _build.LIB)
    vp, sz, i32, u32p, f32 = C.c_void_p, C.c_size_t, C.c_int, C.POINTER(C.c_uint32), C.c_float
    L.gs_create.argtypes = [i32, C.POINTER(vp)]
    L.gs_destroy.argtypes = [vp]
    L.gs_last_error.argtypes = [vp]; L.gs_last_error.restype = C.c_char_p
    L.gs_version.restype = C.c_uint32
    L.gs_clear.argtypes = [vp]
    L.gs_push_splat.argtypes = [vp, vp, sz]
    L.gs_push_matrices.argtypes = [vp, vp, sz]
    L.gs_load_ply.argtypes = [vp, vp, sz]
    L.gs_ply_to_splat.argtypes = [vp, sz, vp, C.POINTER(sz), C.c_char_p, sz]
    L.gs_ply_to_splat_gpu.argtypes = [vp, vp, sz, vp, C.POINTER(sz)]
    L.gs_count.argtypes = [vp]; L.gs_count.restype = sz
    L.gs_sort.argtypes = [vp, vp, vp, vp, u32p]
    L.gs_sort_begin.argtypes = [vp, vp, vp]
    L.gs_sort_poll.argtypes = [vp, i32, vp, u32p, C.POINTER(C.c_int)]
    L.gs_render.argtypes = [vp, C.POINTER(RenderParams), vp, sz]
    L.gs_render_device.argtypes = [vp, C.POINTER(RenderParams), vp]
    L.gs_render_stereo.argtypes = [vp, C.POINTER(RenderParams), C.POINTER(vp), sz]
    L.gs_set_scene.argtypes = [vp, vp, vp, i32, i32]
    L.gs_sync.argtypes = [vp]
    L.gs_set_stream.argtypes = [vp, vp]
    L.gs_wait_stream.argtypes = [vp, vp]
    L.gs_frame_stream.argtypes = [vp]; L.gs_frame_stream.restype = C.c_void_p
    if hasattr(L, "gs_frame_status_device"):                   # (an older build loaded through GS_SPLAT_LIB for an A/B run has none)
        L.gs_frame_status_device.argtypes = [vp, C.POINTER(C.c_void_p)]; L.gs_frame_status_device.restype = C.c_int
    L.gs_frame_lane.argtypes = [vp]; L.gs_frame_lane.restype = C.c_int
    L.gs_lane_stream.argtypes = [vp, C.c_int]; L.gs_lane_stream.restype = C.c_void_p
    L.gs_stream_wait_frame.argtypes = [vp, vp]
    L.gs_model_view_matrix.argtypes = [vp, vp, vp]; L.gs_model_view_matrix.restype = None
    L.gs_projection_matrix.argtypes = [vp, vp]; L.gs_projection_matrix.restype = None
    L.gs_tick_uniforms.argtypes = [vp, vp, vp, vp, vp]; L.gs_tick_uniforms.restype = None
    L.gs_focal.argtypes = [vp, C.c_double]; L.gs_focal.restype = C.c_double
    L.gs_scaled_size.argtypes = [i32, i32, C.c_double, C.POINTER(i32), C.POINTER(i32)]; L.gs_scaled_size.restype = None
    L.gs_set_option.argtypes = [vp, i32, C.c_int64]
    L.gs_get_stats.argtypes = [vp, C.POINTER(Stats)]
    if hasattr(L, "gs_push_sh"):                               # (an older build loaded through GS_SPLAT_LIB for an A/B run has none)
        L.gs_ply_sh.argtypes = [vp, vp, sz, i32, vp, C.POINTER(sz), C.POINTER(i32)]
        L.gs_ply_sh_host.argtypes = [vp, sz, i32, vp, C.POINTER(sz), C.POINTER(i32), C.c_char_p, sz]
        L.gs_push_sh.argtypes = [vp, vp, sz, i32]
        L.gs_multi_push_sh.argtypes = [vp, vp, sz, i32]
        L.gs_sh_count.argtypes = [vp, C.POINTER(sz), C.POINTER(i32)]
        L.gs_sh_eval.argtypes = [vp, i32, vp, vp, vp]
        L.gs_sh_eval_unrounded.argtypes = [vp, i32, vp, vp, vp]
        L.gs_camera_in_object.argtypes = [vp, vp]
    if hasattr(L, "gs_pick"):
        L.gs_render_surface.argtypes = [vp, C.POINTER(RenderParams), vp, sz, C.POINTER(Surface)]
        L.gs_render_surface_device.argtypes = [vp, C.POINTER(RenderParams), vp, C.POINTER(Surface)]
        L.gs_pick.argtypes = [vp, C.POINTER(RenderParams), vp, sz, vp]
    if hasattr(L, "gs_antialias_factor"):
        L.gs_antialias_factor.argtypes = [vp, vp]
    if hasattr(L, "gs_set_state"):                             # (an older build loaded through GS_SPLAT_LIB for an A/B run has none)
        u8, szp = C.c_uint8, C.POINTER(sz)
        for pre in ("gs_", "gs_multi_"):
            getattr(L, pre + "set_state").argtypes = [vp, sz, vp, sz]
            getattr(L, pre + "set_state_ids").argtypes = [vp, vp, sz, u8, u8]
            getattr(L, pre + "select_box").argtypes = [vp, vp, u8, u8, C.c_uint32, szp]
            getattr(L, pre + "select_sphere").argtypes = [vp, vp, f32, u8, u8, C.c_uint32, szp]
            getattr(L, pre + "select_rect").argtypes = [vp, C.POINTER(RenderParams), vp, u8, u8, C.c_uint32, szp]
            getattr(L, pre + "compact").argtypes = [vp, vp, szp]
        L.gs_state_count.argtypes = [vp, szp, szp]
    if hasattr(L, "gs_select_mask"):                           # (an older build loaded through GS_SPLAT_LIB for an A/B run has none)
        u8, szp = C.c_uint8, C.POINTER(sz)
        for pre in ("gs_", "gs_multi_"):
            getattr(L, pre + "select_mask").argtypes = [vp, C.POINTER(RenderParams), vp, sz, vp, u8, u8, C.c_uint32, szp]
        L.gs_mask_polygon.argtypes = [vp, sz, i32, i32, vp, sz]
        L.gs_highlight_info.argtypes = [vp, u32p, u32p]
        L.gs_highlight_word.argtypes = [C.c_uint32, C.c_uint32, u32p]
    if hasattr(L, "gs_project_record"):                        # (an older build loaded through GS_SPLAT_LIB for an A/B run has none)
        L.gs_project_record.argtypes = [vp, vp, C.POINTER(RenderParams), vp, C.POINTER(C.c_float), C.POINTER(C.c_int)]
        L.gs_ortho_matrix.argtypes = [C.c_double] * 6 + [vp]
        L.gs_projection_info.argtypes = [vp, u32p]
    if hasattr(L, "gs_histogram"):                             # (an older build loaded through GS_SPLAT_LIB for an A/B run has none)
        u8, szp, f64 = C.c_uint8, C.POINTER(sz), C.c_double
        L.gs_prop_eval.argtypes = [vp, vp, i32, vp]
        L.gs_hist_bin.argtypes = [f64, f64, f64, C.c_uint32, C.POINTER(C.c_int32)]
        for pre in ("gs_", "gs_multi_"):
            getattr(L, pre + "prop_range").argtypes = [vp, i32, u8, u8, C.POINTER(f64), C.POINTER(f64), szp]
            getattr(L, pre + "histogram").argtypes = [vp, i32, f64, f64, C.c_uint32, u8, u8, vp, vp]
            getattr(L, pre + "select_range").argtypes = [vp, i32, f64, f64, u8, u8, C.c_uint32, szp]
    if hasattr(L, "gs_render_contrib"):                        # (an older build loaded through GS_SPLAT_LIB for an A/B run has none)
        L.gs_render_contrib.argtypes = [vp, C.POINTER(RenderParams), vp, sz]
        L.gs_render_contrib_device.argtypes = [vp, C.POINTER(RenderParams), vp]
        L.gs_contrib_clear.argtypes = [vp]
        L.gs_contrib_info.argtypes = [vp, C.POINTER(sz), C.POINTER(C.c_uint64)]
    if hasattr(L, "gs_export_splat"):                          # (an older build loaded through GS_SPLAT_LIB for an A/B run has none)
        u8, szp = C.c_uint8, C.POINTER(sz)
        L.gs_export_row.argtypes = [vp, vp, vp, vp]
        L.gs_splat_to_ply.argtypes = [vp, vp, vp, sz, i32, sz, vp, szp]
        L.gs_export_sh.argtypes = [vp, u8, u8, vp, szp, C.POINTER(i32)]
        for pre in ("gs_", "gs_multi_"):
            getattr(L, pre + "export_splat").argtypes = [vp, u8, u8, vp, vp, vp, szp]
            getattr(L, pre + "export_ply").argtypes = [vp, u8, u8, i32, vp, szp]
    if hasattr(L, "gs_load_cply"):                             # (likewise)
        u8, szp = C.c_uint8, C.POINTER(sz)
        L.gs_cply_info.argtypes = [vp, sz, szp, szp, C.POINTER(i32), C.POINTER(i32), C.c_char_p, sz]
        L.gs_cply_to_splat.argtypes = [vp, sz, vp, vp, szp, C.c_char_p, sz]
        L.gs_cply_sh_host.argtypes = [vp, sz, i32, vp, szp, C.POINTER(i32), C.c_char_p, sz]
        L.gs_splat_to_cply.argtypes = [vp, vp, vp, sz, i32, sz, C.c_uint32, vp, vp, szp]
        L.gs_log_fixed.argtypes = [C.c_double, C.POINTER(C.c_double)]
        L.gs_cply_to_splat_gpu.argtypes = [vp, vp, sz, vp, vp, szp]
        for pre in ("gs_", "gs_multi_"):
            getattr(L, pre + "load_cply").argtypes = [vp, vp, sz]
            getattr(L, pre + "export_cply").argtypes = [vp, u8, u8, i32, C.c_uint32, vp, vp, szp]
    if hasattr(L, "gs_adjust_colour"):                         # (likewise)
        L.gs_adjust_word.argtypes = [C.c_uint32, C.POINTER(ColourAdjust), u32p]
        L.gs_adjust_sh_row.argtypes = [vp, i32, C.POINTER(ColourAdjust), vp]
        for pre in ("gs_", "gs_multi_"):
            getattr(L, pre + "adjust_colour").argtypes = [vp, C.POINTER(ColourAdjust), u8, u8, szp]
            getattr(L, pre + "replace_splat").argtypes = [vp, sz, vp, sz]
            getattr(L, pre + "replace_sh").argtypes = [vp, sz, vp, sz, i32]
    if hasattr(L, "gs_transform"):                             # (likewise)
        u8, szp = C.c_uint8, C.POINTER(sz)
        L.gs_transform_record.argtypes = [vp, vp, vp, C.POINTER(Similarity), vp, vp, vp, vp]
        L.gs_transform_records.argtypes = [vp, vp, vp, sz, C.POINTER(Similarity), vp, vp, vp, vp]
        L.gs_transform_sh_row.argtypes = [vp, i32, C.POINTER(Similarity), vp]
        L.gs_sh_rotation.argtypes = [C.POINTER(Similarity), vp]
        L.gs_similarity_about.argtypes = [vp, vp, f32, C.POINTER(Similarity)]
        for pre in ("gs_", "gs_multi_"):
            getattr(L, pre + "transform").argtypes = [vp, C.POINTER(Similarity), u8, u8, szp]
    L.gs_download.argtypes = [vp, i32, vp, sz]
    if hasattr(L, "gs_sort_inspect"):
        L.gs_sort_inspect.argtypes = [vp, C.POINTER(SortInfo), vp, sz]
    L.gs_comm_unique_id.argtypes = [vp, vp]
    L.gs_comm_init.argtypes = [vp, vp, i32, i32]
    L.gs_comm_destroy.argtypes = [vp]
    L.gs_partition.argtypes = [i32, C.POINTER(i32), i32, C.POINTER(Piece), i32]
    L.gs_render_gathered.argtypes = [vp, C.POINTER(RenderParams), i32, i32, C.POINTER(vp), C.c_uint32]
    L.gs_read_gathered.argtypes = [vp, i32, vp, sz]
    L.gs_sort_for.argtypes = [vp, vp, vp, C.POINTER(RenderParams), vp, u32p]
    L.gs_sort_gathered.argtypes = [vp, vp, vp, C.POINTER(RenderParams), i32]
    L.gs_gathered_size.argtypes = [vp, i32, C.POINTER(i32), C.POINTER(i32)]
    L.gs_host_alloc.argtypes = [sz]; L.gs_host_alloc.restype = C.c_void_p
    L.gs_host_free.argtypes = [vp]; L.gs_host_free.restype = None
    L.gs_create_multi.argtypes = [C.POINTER(i32), i32, C.POINTER(vp)]
    L.gs_multi_destroy.argtypes = [vp]
    L.gs_multi_last_error.argtypes = [vp]; L.gs_multi_last_error.restype = C.c_char_p
    L.gs_multi_devices.argtypes = [vp]
    L.gs_multi_ctx.argtypes = [vp, i32]; L.gs_multi_ctx.restype = vp
    L.gs_multi_clear.argtypes = [vp]
    L.gs_multi_push_splat.argtypes = [vp, vp, sz]
    L.gs_multi_load_ply.argtypes = [vp, vp, sz]
    L.gs_multi_count.argtypes = [vp]; L.gs_multi_count.restype = sz
    L.gs_multi_set_option.argtypes = [vp, i32, C.c_int64]
    L.gs_multi_sort.argtypes = [vp, vp, vp, C.POINTER(RenderParams), i32]
    L.gs_multi_render.argtypes = [vp, C.POINTER(RenderParams), i32, C.POINTER(vp), sz, C.c_uint32]
    L.gs_multi_render_device.argtypes = [vp, C.POINTER(RenderParams), i32, C.POINTER(vp), C.c_uint32]
    L.gs_multi_read.argtypes = [vp, i32, vp, sz]
    L.gs_multi_sync.argtypes = [vp]
    _lib = L
    return L


class Similarity(C.Structure):
    """gs_similarity: p' = scale * R p + translation in the rows' object space; rotation = quaternion (w, x, y, z), need not be normalised"""
    _fields_ = [("rotation", C.c_float * 4), ("scale", C.c_float), ("translation", C.c_float * 3)]


def similarity(rotation=(1.0, 0.0, 0.0, 0.0), scale=1.0, translation=(0.0, 0.0, 0.0)):
    """A Similarity; the defaults are the identity"""
    t = Similarity()
    t.rotation[:] = [float(v) for v in np.asarray(rotation, np.float32).reshape(4)]
    t.scale = float(np.float32(scale))
    t.translation[:] = [float(v) for v in np.asarray(translation, np.float32).reshape(3)]
    return t


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


# ---- host helpers (no context needed) ------------------------------------------------------------------

def host_frame(height, width):
    """An H x W x 4 uint8 array over page-locked memory (gs_host_alloc); keep the returned owner alive, free with owner.free()."""
    L = load()
    n = int(height) * int(width) * 4
    p = L.gs_host_alloc(n)
    if not p:
        raise MemoryError("gs_host_alloc(%d)" % n)

    class _Owner:
        def free(self):
            if self.p:
                L.gs_host_free(self.p); self.p = None
    o = _Owner(); o.p = p
    arr = np.ctypeslib.as_array((C.c_uint8 * n).from_address(p)).reshape(int(height), int(width), 4)
    return arr, o


def device_count():
    return int(load().gs_device_count())


def partition(widths, world):
    """gs_partition: [(view, x0, x1, owner rank)] for one view (column strips) or two (XR eyes), in gather order."""
    widths = [int(w) for w in widths]
    arr = (C.c_int * len(widths))(*widths)
    out = (Piece * 128)()
    n = load().gs_partition(len(widths), arr, int(world), out, 128)
    if n < 0:
        raise GsError(n, "gs_partition(%r, world=%d)" % (widths, world))
    return [(out[i].view, out[i].x0, out[i].x1, out[i].owner) for i in range(n)]



def model_view_matrix(cam_world, obj_world):
    a = np.ascontiguousarray(cam_world, np.float64); b = np.ascontiguousarray(obj_world, np.float64); o = np.zeros(16, np.float64)
    load().gs_model_view_matrix(_p(a), _p(b), _p(o))
    return o


def projection_matrix(proj):
    a = np.ascontiguousarray(proj, np.float64); o = np.zeros(16, np.float64)
    load().gs_projection_matrix(_p(a), _p(o))
    return o


def ortho_matrix(left, right, top, bottom, near, far):
    """gs_ortho_matrix: three.js Matrix4.makeOrthographic (WebGL convention), column-major f64; feed it through projection_matrix and draw
    with RENDER_PARALLEL"""
    o = np.zeros(16, np.float64)
    rc = load().gs_ortho_matrix(float(left), float(right), float(top), float(bottom), float(near), float(far), _p(o))
    if rc != GS_OK:
        raise GsError(rc, "gs_ortho_matrix: bad argument")
    return o


def project_record(cs, cc, params):
    """gs_project_record: packed records -- cs = float32[n, 4], cc = uint32[n, 4] -- through the kernels' own projection with `params`
    (RENDER_PARALLEL in its flags or not) -> (records uint32[n, 8] as BUF_PROJECTED holds them, zwin float32[n], visible bool[n])"""
    a = np.ascontiguousarray(cs, np.float32).reshape(-1, 4)
    b = np.ascontiguousarray(cc, np.uint32).reshape(-1, 4)
    if len(a) != len(b):
        raise ValueError("cs and cc: the same number of records")
    n = len(a)
    rec = np.zeros((n, 8), np.float32)
    zwin, vis = np.zeros(n, np.float32), np.zeros(n, bool)
    f, z, v = load().gs_project_record, C.c_float(0), C.c_int(0)
    pa, pb, pr = a.ctypes.data, b.ctypes.data, rec.ctypes.data
    for i in range(n):
        rc = f(pa + 16 * i, pb + 16 * i, C.byref(params), pr + 32 * i, C.byref(z), C.byref(v))
        if rc != GS_OK:
            raise GsError(rc, "gs_project_record: bad argument")
        zwin[i], vis[i] = z.value, bool(v.value)
    return rec.view(np.uint32), zwin, vis


def tick_uniforms(cam_world, obj_world, cutout_world=None):
    a = np.ascontiguousarray(cam_world, np.float64); b = np.ascontiguousarray(obj_world, np.float64)
    c = None if cutout_world is None else np.ascontiguousarray(cutout_world, np.float64)
    view = np.zeros(4, np.float32); cut = np.zeros(16, np.float32)
    load().gs_tick_uniforms(_p(a), _p(b), _p(c), _p(view), _p(cut))
    return view, (cut if c is not None else None)


def focal(gs_proj, viewport_h):
    a = np.ascontiguousarray(gs_proj, np.float64)
    return load().gs_focal(_p(a), float(viewport_h))


def scaled_size(css_w, css_h, ratio):
    w, h = C.c_int(0), C.c_int(0)
    load().gs_scaled_size(int(css_w), int(css_h), float(ratio), C.byref(w), C.byref(h))
    return w.value, h.value


def ply_to_splat(ply_bytes):
    """processPlyBuffer (index.js:600-745): PLY bytes -> uint8 array of 32-byte .splat rows."""
    buf = np.frombuffer(bytes(ply_bytes), np.uint8)
    n = C.c_size_t(0); err = C.create_string_buffer(256)
    rc = load().gs_ply_to_splat(_p(buf), buf.size, None, C.byref(n), err, 256)
    if rc != GS_OK:
        raise GsError(rc, err.value.decode())
    out = np.zeros(n.value * 32, np.uint8)
    rc = load().gs_ply_to_splat(_p(buf), buf.size, _p(out), C.byref(n), err, 256)
    if rc != GS_OK:
        raise GsError(rc, err.value.decode())
    return out


def _sh_rows(sh_rows, degree):
    k = 3 * (int(degree) + 1) ** 2
    rows = np.ascontiguousarray(sh_rows, np.float32).reshape(-1)
    if rows.size % k:
        raise ValueError("SH rows of degree %d are %d floats each" % (degree, k))
    return rows, rows.size // k


def ply_sh(ply_bytes, degree=3, ctx=None):
    """The SH rows of a PLY in the converter's row order -> (float32[n, 3 (D+1)^2], D); D = min(degree, what the file carries),
    (empty, -1) for a file without usable coefficients.  ctx: a Context (gs_ply_sh) or None (gs_ply_sh_host)."""
    buf = np.frombuffer(bytes(ply_bytes), np.uint8)
    n = C.c_size_t(0); d = C.c_int(-1); err = C.create_string_buffer(256)

    def call(out):
        if ctx is not None:
            ctx._ck(load().gs_ply_sh(ctx._h, _p(buf), buf.size, int(degree), out, C.byref(n), C.byref(d)))
            return
        rc = load().gs_ply_sh_host(_p(buf), buf.size, int(degree), out, C.byref(n), C.byref(d), err, 256)
        if rc != GS_OK:
            raise GsError(rc, err.value.decode())

    call(None)
    if d.value < 0:
        return np.zeros((0, 0), np.float32), -1
    out = np.zeros((n.value, 3 * (d.value + 1) ** 2), np.float32)
    if n.value:
        call(_p(out))
    return out, d.value


def sh_eval(sh_row, degree, cam, pos, unrounded=False):
    """gs_sh_eval: one SH row (3 (degree+1)^2 f32, channel-major), camera (f64 x3) and position (f32 x3) in object space -> uint8[3]
    (unrounded=True: the three f64 values before the byte rounding, in units of one colour byte)."""
    row, n = _sh_rows(sh_row, degree)
    if n != 1:
        raise ValueError("one row expected")
    cam = np.ascontiguousarray(cam, np.float64).reshape(3); pos = np.ascontiguousarray(pos, np.float32).reshape(3)
    out = np.zeros(3, np.float64 if unrounded else np.uint8)
    rc = (load().gs_sh_eval_unrounded if unrounded else load().gs_sh_eval)(_p(row), int(degree), _p(cam), _p(pos), _p(out))
    if rc != GS_OK:
        raise GsError(rc, "gs_sh_eval: bad argument")
    return out


def camera_in_object(model_view):
    """gs_camera_in_object: the camera position in object space (f64 x3) a frame with this model_view evaluates SH colours for."""
    mv = np.ascontiguousarray(np.asarray(model_view, np.float32).reshape(16))
    out = np.zeros(3, np.float64)
    rc = load().gs_camera_in_object(_p(mv), _p(out))
    if rc != GS_OK:
        raise GsError(rc, "gs_camera_in_object: singular model_view")
    return out


def antialias_factor(cov):
    """gs_antialias_factor: cov = (cov00, cov01, cov11), a projected covariance in px^2 before the 0.3 px^2 dilation, or an array of
    such rows -> the opacity factor c of GS_OPT_ANTIALIAS as float32 (one value, or one per row)."""
    c = np.ascontiguousarray(cov, np.float32)
    if c.shape[-1:] != (3,):
        raise ValueError("rows of (cov00, cov01, cov11) expected")
    rows = c.reshape(-1, 3)
    out = np.zeros(len(rows), np.float32)
    f, base, obase = load().gs_antialias_factor, rows.ctypes.data, out.ctypes.data
    for i in range(len(rows)):
        rc = f(base + 12 * i, obase + 4 * i)
        if rc != GS_OK:
            raise GsError(rc, "gs_antialias_factor: bad argument")
    return out.reshape(c.shape[:-1]) if c.ndim > 1 else out[0]


def highlight_option(rgb, weight):
    """the value of OPT_HIGHLIGHT for a colour (r, g, b) and a weight, bytes each: R | G << 8 | B << 16 | W << 24"""
    r, g, b = (int(v) & 255 for v in rgb)
    return r | g << 8 | b << 16 | (int(weight) & 255) << 24


def highlight_word(rgba, option_value):
    """gs_highlight_word: the colour word(s) R | G << 8 | B << 16 | A << 24 of selected splats under OPT_HIGHLIGHT = option_value, by the
    kernel's own function (one value, or an array of them)"""
    w = np.ascontiguousarray(rgba, np.uint32)
    flat, out = w.reshape(-1), C.c_uint32(0)
    res = np.zeros(flat.size, np.uint32)
    f = load().gs_highlight_word
    for i in range(flat.size):
        rc = f(int(flat[i]), int(option_value) & 0xFFFFFFFF, C.byref(out))
        if rc != GS_OK:
            raise GsError(rc, "gs_highlight_word: bad argument")
        res[i] = out.value
    return res.reshape(w.shape) if w.ndim else res[0]


def prop_eval(cs, cc, prop):
    """gs_prop_eval: the property `prop` (PROP_*) of packed records -- cs = float32[..., 4] and cc = uint32[..., 4], as BUF_CENTER_SCALE and
    BUF_COV_COLOR hold them -- by the kernels' own function -> float64 (one value, or one per record)"""
    a = np.ascontiguousarray(cs, np.float32)
    b = np.ascontiguousarray(cc, np.uint32)
    if a.shape[-1:] != (4,) or a.shape != b.shape:
        raise ValueError("cs and cc: records of four words each, the same number of them")
    ra, rb = a.reshape(-1, 4), b.reshape(-1, 4)
    out = np.zeros(len(ra), np.float64)
    f, pa, pb, po = load().gs_prop_eval, ra.ctypes.data, rb.ctypes.data, out.ctypes.data
    for i in range(len(ra)):
        rc = f(pa + 16 * i, pb + 16 * i, int(prop), po + 8 * i)
        if rc != GS_OK:
            raise GsError(rc, "gs_prop_eval: bad argument")
    return out.reshape(a.shape[:-1]) if a.ndim > 1 else out[0]


def hist_bin(v, lo, hi, nbins):
    """gs_hist_bin: the bin(s) of the value(s) v in a histogram of nbins bins over [lo, hi] (-1 below, -2 above, -3 NaN) -> int32"""
    vals = np.ascontiguousarray(v, np.float64)
    flat, out = vals.reshape(-1), C.c_int32(0)
    res = np.zeros(flat.size, np.int32)
    f = load().gs_hist_bin
    for i in range(flat.size):
        rc = f(float(flat[i]), float(lo), float(hi), int(nbins), C.byref(out))
        if rc != GS_OK:
            raise GsError(rc, "gs_hist_bin: bad argument")
        res[i] = out.value
    return res.reshape(vals.shape) if vals.ndim else res[0]


def export_row(cs, cc, want_wide=False):
    """gs_export_row: packed records -- cs = float32[..., 4], cc = uint32[..., 4], as BUF_CENTER_SCALE and BUF_COV_COLOR hold them -- back to
    32-byte .splat rows by the export kernel's own function -> uint8[n, 32] (want_wide: and float32[n, 7], the scales and the stored
    quaternion before the byte rounding)"""
    a = np.ascontiguousarray(cs, np.float32)
    b = np.ascontiguousarray(cc, np.uint32)
    if a.shape[-1:] != (4,) or a.shape != b.shape:
        raise ValueError("cs and cc: records of four words each, the same number of them")
    ra, rb = a.reshape(-1, 4), b.reshape(-1, 4)
    rows = np.zeros((len(ra), 32), np.uint8)
    wide = np.zeros((len(ra), 7), np.float32)
    f, pa, pb, pr, pw = load().gs_export_row, ra.ctypes.data, rb.ctypes.data, rows.ctypes.data, wide.ctypes.data
    for i in range(len(ra)):
        rc = f(pa + 16 * i, pb + 16 * i, pr + 32 * i, pw + 28 * i if want_wide else None)
        if rc != GS_OK:
            raise GsError(rc, "gs_export_row: bad argument")
    return (rows, wide) if want_wide else rows


def adjust_word(rgba, adjust):
    """gs_adjust_word: the colour word(s) R | G << 8 | B << 16 | A << 24 under the ColourAdjust, by the kernel's own function (one value,
    or an array of them)"""
    w = np.ascontiguousarray(rgba, np.uint32)
    flat, out = w.reshape(-1), C.c_uint32(0)
    res = np.zeros(flat.size, np.uint32)
    f, pa, po = load().gs_adjust_word, C.byref(adjust), C.byref(out)
    for i, v in enumerate(flat.tolist()):
        rc = f(v, pa, po)
        if rc != GS_OK:
            raise GsError(rc, "gs_adjust_word: bad argument")
        res[i] = out.value
    return res.reshape(w.shape) if w.ndim else res[0]


def adjust_sh_rows(sh_rows, degree, adjust, in_place=False):
    """gs_adjust_sh_row over rows of 3 (degree+1)^2 f32 each -> float32[n, 3 (degree+1)^2] (in_place: sh_rows itself, a C-contiguous
    float32 array, is rewritten and returned)"""
    k = 3 * (int(degree) + 1) ** 2
    src = sh_rows if in_place else np.ascontiguousarray(sh_rows, np.float32).reshape(-1, k)
    if in_place and (src.dtype != np.float32 or not src.flags.c_contiguous or src.size % k):
        raise ValueError("in_place: a C-contiguous float32 array of whole rows expected")
    out = src if in_place else np.zeros_like(src)
    f, pa = load().gs_adjust_sh_row, C.byref(adjust)
    for i in range(src.size // k):
        rc = f(src.ctypes.data + 4 * k * i, int(degree), pa, out.ctypes.data + 4 * k * i)
        if rc != GS_OK:
            raise GsError(rc, "gs_adjust_sh_row: bad argument")
    return out


def similarity_about(pivot, rotation=(1.0, 0.0, 0.0, 0.0), scale=1.0):
    """gs_similarity_about: the Similarity that rotates and scales about `pivot` (rows' object space)"""
    t = Similarity()
    pv, q = np.ascontiguousarray(pivot, np.float32).reshape(3), np.ascontiguousarray(rotation, np.float32).reshape(4)
    rc = load().gs_similarity_about(_p(pv), _p(q), float(np.float32(scale)), C.byref(t))
    if rc != GS_OK:
        raise GsError(rc, "gs_similarity_about: bad argument")
    return t


def transform_records(cs, cc, sort_rows, t, want_bound=False, one_by_one=False):
    """gs_transform_records (one_by_one: gs_transform_record per record) over packed records (cs: [n, 4] f32 or its u32 bits, cc: [n, 4]
    u32, sort_rows: [n, 4] f32 or bits, as gs_download returns them) -> (cs', cc', sort_rows') as uint32[n, 4] each [, bound:
    float32[n]], by the kernel's own function"""
    a = [np.ascontiguousarray(x).view(np.uint32).reshape(-1, 4) for x in (cs, cc, sort_rows)]
    n = len(a[0])
    out = [np.zeros((n, 4), np.uint32) for _ in range(3)]
    bound = np.zeros(n, np.float32)
    L, pt = load(), C.byref(t)
    if not one_by_one:
        rc = L.gs_transform_records(_p(a[0]), _p(a[1]), _p(a[2]), n, pt, _p(out[0]), _p(out[1]), _p(out[2]), _p(bound))
        if rc != GS_OK:
            raise GsError(rc, "gs_transform_records: bad argument")
    else:
        base = [x.ctypes.data for x in a] + [x.ctypes.data for x in out]
        for i in range(n):
            o = 16 * i
            rc = L.gs_transform_record(base[0] + o, base[1] + o, base[2] + o, pt, base[3] + o, base[4] + o, base[5] + o, bound.ctypes.data + 4 * i)
            if rc != GS_OK:
                raise GsError(rc, "gs_transform_record: bad argument")
    return (out[0], out[1], out[2], bound) if want_bound else tuple(out)


def transform_sh_rows(sh_rows, degree, t, in_place=False):
    """gs_transform_sh_row over rows of 3 (degree+1)^2 f32 each -> float32[n, 3 (degree+1)^2] (in_place: sh_rows itself, a C-contiguous
    float32 array, is rewritten and returned)"""
    k = 3 * (int(degree) + 1) ** 2
    src = sh_rows if in_place else np.ascontiguousarray(sh_rows, np.float32).reshape(-1, k)
    if in_place and (src.dtype != np.float32 or not src.flags.c_contiguous or src.size % k):
        raise ValueError("in_place: a C-contiguous float32 array of whole rows expected")
    out = src if in_place else np.zeros_like(src)
    f, pt = load().gs_transform_sh_row, C.byref(t)
    for i in range(src.size // k):
        rc = f(src.ctypes.data + 4 * k * i, int(degree), pt, out.ctypes.data + 4 * k * i)
        if rc != GS_OK:
            raise GsError(rc, "gs_transform_sh_row: bad argument")
    return out


def sh_rotation(t):
    """gs_sh_rotation: the band matrices the SH kernel is handed -> (D1 [3, 3], D2 [5, 5], D3 [7, 7]) float64"""
    d = np.zeros(83, np.float64)
    rc = load().gs_sh_rotation(C.byref(t), _p(d))
    if rc != GS_OK:
        raise GsError(rc, "gs_sh_rotation: bad argument")
    return d[:9].reshape(3, 3).copy(), d[9:34].reshape(5, 5).copy(), d[34:].reshape(7, 7).copy()


def _transform(fn, h, ck, t, of):
    m, v = _of(of)
    hit = C.c_size_t(0)
    ck(fn(h, C.byref(t), m, v, C.byref(hit)))
    return hit.value


def _adjust_colour(fn, h, ck, adjust, of):
    m, v = _of(of)
    hit = C.c_size_t(0)
    ck(fn(h, C.byref(adjust), m, v, C.byref(hit)))
    return hit.value


def _replace_splat(fn, h, ck, first, rows):
    rows = np.ascontiguousarray(np.asarray(rows).view(np.uint8).reshape(-1))
    if rows.size % 32:
        raise ValueError("rows must be a multiple of 32 bytes")
    ck(fn(h, int(first), _p(rows), rows.size // 32))


def splat_to_ply(rows, wide=None, sh=None, degree=0):
    """gs_splat_to_ply: .splat rows (+ the wide parts of export_splat, + SH rows of `degree` for the first len(sh) of them) -> the bytes
    of a binary little-endian INRIA .ply (uint8 array) that ply_to_splat / load_ply / ply_sh read back"""
    r = np.ascontiguousarray(np.asarray(rows).view(np.uint8).reshape(-1))
    if r.size % 32:
        raise ValueError("rows must be a multiple of 32 bytes")
    n = r.size // 32
    w = None
    if wide is not None:
        w = np.ascontiguousarray(wide, np.float32).reshape(-1)
        if w.size != 7 * n:
            raise ValueError("wide: seven floats per row")
    s, ns = None, 0
    if sh is not None:
        s, ns = _sh_rows(sh, degree)
    nb = C.c_size_t(0)
    rc = load().gs_splat_to_ply(_p(r), _p(w), _p(s), ns, int(degree), n, None, C.byref(nb))
    if rc != GS_OK:
        raise GsError(rc, "gs_splat_to_ply: bad argument")
    out = np.zeros(nb.value, np.uint8)
    rc = load().gs_splat_to_ply(_p(r), _p(w), _p(s), ns, int(degree), n, _p(out), C.byref(nb))
    if rc != GS_OK:
        raise GsError(rc, "gs_splat_to_ply: bad argument")
    return out


def cply_info(ply_bytes):
    """gs_cply_info: the header of a compressed .ply -> dict(splats, chunks, sh_degree, chunk_floats); GsError (GS_E_PLY_HEADER) for anything
    else, an INRIA .ply included: that is the sniff"""
    buf = np.frombuffer(bytes(ply_bytes), np.uint8)
    n, c = C.c_size_t(0), C.c_size_t(0); d, cf = C.c_int(0), C.c_int(0); err = C.create_string_buffer(256)
    rc = load().gs_cply_info(_p(buf), buf.size, C.byref(n), C.byref(c), C.byref(d), C.byref(cf), err, 256)
    if rc != GS_OK:
        raise GsError(rc, err.value.decode())
    return {"splats": n.value, "chunks": c.value, "sh_degree": d.value, "chunk_floats": cf.value}


def _cply_rows(call, ck, buf, want_wide):
    n = C.c_size_t(0)
    ck(call(_p(buf), buf.size, None, None, C.byref(n)))
    rows = np.zeros((n.value, 32), np.uint8)
    wide = np.zeros((n.value, 7), np.float32) if want_wide else None
    if n.value:
        ck(call(_p(buf), buf.size, _p(rows), _p(wide), C.byref(n)))
    return (rows, wide) if want_wide else rows


def cply_to_splat(ply_bytes, want_wide=False):
    """gs_cply_to_splat: a compressed .ply -> its rows in file order (uint8[n, 32]) [, their wide parts (float32[n, 7])]"""
    buf = np.frombuffer(bytes(ply_bytes), np.uint8)
    err = C.create_string_buffer(256)

    def ck(rc):
        if rc != GS_OK:
            raise GsError(rc, err.value.decode())
    return _cply_rows(lambda *a: load().gs_cply_to_splat(*a, err, 256), ck, buf, want_wide)


def cply_sh(ply_bytes, degree=3):
    """gs_cply_sh_host: the SH rows of a compressed .ply in file order -> (float32[n, 3 (D+1)^2], D), D = min(degree, the file's)"""
    buf = np.frombuffer(bytes(ply_bytes), np.uint8)
    n = C.c_size_t(0); d = C.c_int(-1); err = C.create_string_buffer(256)
    rc = load().gs_cply_sh_host(_p(buf), buf.size, int(degree), None, C.byref(n), C.byref(d), err, 256)
    if rc != GS_OK:
        raise GsError(rc, err.value.decode())
    out = np.zeros((n.value, 3 * (d.value + 1) ** 2), np.float32)
    if n.value:
        rc = load().gs_cply_sh_host(_p(buf), buf.size, int(degree), _p(out), C.byref(n), C.byref(d), err, 256)
        if rc != GS_OK:
            raise GsError(rc, err.value.decode())
    return out, d.value


def splat_to_cply(rows, wide=None, sh=None, degree=0, morton=False, want_index=False):
    """gs_splat_to_cply: splat_to_ply's inputs -> the bytes of a compressed .ply (uint8 array) [, the input row of every output row]"""
    r = np.ascontiguousarray(np.asarray(rows).view(np.uint8).reshape(-1))
    if r.size % 32:
        raise ValueError("rows must be a multiple of 32 bytes")
    n = r.size // 32
    w = None
    if wide is not None:
        w = np.ascontiguousarray(wide, np.float32).reshape(-1)
        if w.size != 7 * n:
            raise ValueError("wide: seven floats per row")
    s, ns = None, 0
    if sh is not None:
        s, ns = _sh_rows(sh, degree)
    flags = CPLY_MORTON if morton else 0
    nb = C.c_size_t(0)
    rc = load().gs_splat_to_cply(_p(r), _p(w), _p(s), ns, int(degree), n, flags, None, None, C.byref(nb))
    if rc != GS_OK:
        raise GsError(rc, "gs_splat_to_cply: bad argument")
    out = np.zeros(nb.value, np.uint8)
    index = np.zeros(n, np.uint32) if want_index else None
    rc = load().gs_splat_to_cply(_p(r), _p(w), _p(s), ns, int(degree), n, flags, _p(index), _p(out), C.byref(nb))
    if rc != GS_OK:
        raise GsError(rc, "gs_splat_to_cply: bad argument")
    return (out, index) if want_index else out


def log_fixed(x):
    """gs_log_fixed: the encoder's logarithm (the same bits on the host and on the device)"""
    out = C.c_double(0.0)
    load().gs_log_fixed(float(x), C.byref(out))
    return out.value


def _export_cply(fn, count_fn, h, ck, of, sh_degree, morton, want_index):
    m, v = _of(of)
    flags = CPLY_MORTON if morton else 0
    nb, n = C.c_size_t(0), C.c_size_t(0)
    ck(fn(h, m, v, int(sh_degree), flags, None, None, C.byref(nb)))
    out = np.zeros(nb.value, np.uint8)
    index = None
    if want_index:
        ck(count_fn(h, m, v, None, None, None, C.byref(n)))
        index = np.zeros(n.value, np.uint32)
    ck(fn(h, m, v, int(sh_degree), flags, _p(index), _p(out), C.byref(nb)))
    return (out[:nb.value], index) if want_index else out[:nb.value]


OF_FILTERS = {"all": (0, 0), "visible": (STATE_HIDDEN, 0), "selected": (STATE_HIDDEN | STATE_SELECTED, STATE_SELECTED)}


def _of(of):
    """a state filter: 'all' | 'visible' | 'selected', or (state_mask, state_value)"""
    m, v = OF_FILTERS[of] if isinstance(of, str) else of
    return int(m), int(v)


def _export_splat(L, fn, h, ck, of, want_wide, want_index):
    m, v = _of(of)
    n = C.c_size_t(0)
    ck(fn(h, m, v, None, None, None, C.byref(n)))
    rows = np.zeros((n.value, 32), np.uint8)
    wide = np.zeros((n.value, 7), np.float32) if want_wide else None
    index = np.zeros(n.value, np.uint32) if want_index else None
    if n.value:
        ck(fn(h, m, v, _p(rows), _p(wide), _p(index), C.byref(n)))
    out = (rows,) + ((wide,) if want_wide else ()) + ((index,) if want_index else ())
    return out if len(out) > 1 else rows


def _export_ply(fn, h, ck, of, sh_degree):
    m, v = _of(of)
    nb = C.c_size_t(0)
    ck(fn(h, m, v, int(sh_degree), None, C.byref(nb)))
    out = np.zeros(nb.value, np.uint8)
    ck(fn(h, m, v, int(sh_degree), _p(out), C.byref(nb)))
    return out[:nb.value]


def mask_polygon(points, width, height, out=None):
    """gs_mask_polygon: even-odd fill of the closed polygon `points` (n x (x, y), pixels, row 0 = top) -> uint8[height, width] of 0 / 1.
    out: a C-contiguous uint8 array of `height` rows to fill instead (its row length is the stride; bytes beyond `width` stay)."""
    pts = np.ascontiguousarray(points, np.float32).reshape(-1, 2)
    if out is None:
        out = np.zeros((int(height), int(width)), np.uint8)
    if out.dtype != np.uint8 or out.ndim != 2 or not out.flags.c_contiguous or out.shape[0] != int(height):
        raise ValueError("out: a C-contiguous uint8 array of `height` rows expected")
    rc = load().gs_mask_polygon(_p(pts) if len(pts) else None, len(pts), int(width), int(height), _p(out), out.shape[1])
    if rc != GS_OK:
        raise GsError(rc, "gs_mask_polygon: bad argument")
    return out


def _mask_args(params, mask, depth_max):
    """(mask as rows of bytes, its stride, the depth plane or None) for gs_select_mask: a uint8 view with padded rows is passed as it is"""
    m = np.asarray(mask)
    if m.dtype != np.uint8 or m.ndim != 2 or m.strides[1] != 1 or m.strides[0] < m.shape[1]:
        m = np.ascontiguousarray(mask, np.uint8)
    if m.ndim != 2 or m.shape != (params.fb_height, params.fb_width):
        raise ValueError("mask: fb_height x fb_width bytes expected")
    d = None
    if depth_max is not None:
        d = np.ascontiguousarray(depth_max, np.float32)
        if d.shape != (params.fb_height, params.fb_width):
            raise ValueError("depth_max: fb_height x fb_width float32 expected")
    return m, m.strides[0], d


def make_params(mv, proj, width, height, x0=0, x1=None, focal_=0.0, background=(0.0, 0.0, 0.0, 1.0), flags=0):
    p = RenderParams()
    p.model_view[:] = [float(v) for v in np.asarray(mv, np.float32)]
    p.projection[:] = [float(v) for v in np.asarray(proj, np.float32)]
    p.fb_width, p.fb_height = int(width), int(height)
    p.x0, p.x1 = int(x0), int(width if x1 is None else x1)
    p.focal = float(np.float32(focal_))
    p.background[:] = [float(v) for v in background]
    p.flags = int(flags)
    return p


class Context:
    """One gs_ctx: one component instance on one GPU."""

    def __init__(self, device=0):
        self._L = load()
        h = C.c_void_p()
        rc = self._L.gs_create(int(device), C.byref(h))
        if rc != GS_OK:
            raise GsError(rc, self._L.gs_last_error(None).decode())
        self._h = h
        self.device = device

    def close(self):
        if getattr(self, "_h", None):
            self._L.gs_destroy(self._h)
            self._h = None

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def _ck(self, rc):
        if rc != GS_OK:
            raise GsError(rc, self._L.gs_last_error(self._h).decode())

    # ingest
    def clear(self):
        self._ck(self._L.gs_clear(self._h))

    def push_splat(self, rows):
        rows = np.ascontiguousarray(np.asarray(rows).view(np.uint8).reshape(-1))
        if rows.size % 32:
            raise ValueError("rows must be a multiple of 32 bytes")
        self._ck(self._L.gs_push_splat(self._h, _p(rows), rows.size // 32))

    def push_matrices(self, matrices):
        m = np.ascontiguousarray(matrices, np.float32).reshape(-1)
        if m.size % 16:
            raise ValueError("matrices must be a multiple of 16 floats")
        self._ck(self._L.gs_push_matrices(self._h, _p(m), m.size // 16))

    def ply_to_splat(self, ply_bytes):
        """processPlyBuffer on this context's GPU -> uint8[32 * n] (same bytes as the host converter)."""
        buf = np.frombuffer(bytes(ply_bytes), np.uint8)
        n = C.c_size_t(0)
        self._ck(self._L.gs_ply_to_splat_gpu(self._h, _p(buf), buf.size, None, C.byref(n)))
        out = np.zeros(n.value * 32, np.uint8)
        if n.value:
            self._ck(self._L.gs_ply_to_splat_gpu(self._h, _p(buf), buf.size, _p(out), C.byref(n)))
        return out

    def load_ply(self, ply_bytes):
        buf = np.frombuffer(bytes(ply_bytes), np.uint8)
        self._ck(self._L.gs_load_ply(self._h, _p(buf), buf.size))

    # view-dependent colour (GS_OPT_SH_DEGREE)
    def push_sh(self, sh_rows, degree):
        rows, n = _sh_rows(sh_rows, degree)
        self._ck(self._L.gs_push_sh(self._h, _p(rows), n, int(degree)))

    def ply_sh(self, ply_bytes, degree=3):
        return ply_sh(ply_bytes, degree, ctx=self)

    def sh_count(self):
        n = C.c_size_t(0); d = C.c_int(0)
        self._ck(self._L.gs_sh_count(self._h, C.byref(n), C.byref(d)))
        return n.value, d.value

    def download_sh(self):
        """The SH store: float32[rows, 3 (D+1)^2] (0 rows while nothing is stored)."""
        n, d = self.sh_count()
        return self.download(BUF_SH, n, np.float32, 3 * (d + 1) ** 2 if n else 0)

    def count(self):
        return self._L.gs_count(self._h)

    # editing the resident cloud: per-splat state bytes (STATE_HIDDEN leaves every sort), region selection, deletion
    def set_state(self, first, states):
        st = np.ascontiguousarray(states, np.uint8).reshape(-1)
        self._ck(self._L.gs_set_state(self._h, int(first), _p(st), st.size))

    def set_state_ids(self, ids, set_bits=0, clear_bits=0):
        ids = np.ascontiguousarray(ids, np.uint32).reshape(-1)
        self._ck(self._L.gs_set_state_ids(self._h, _p(ids), ids.size, int(set_bits), int(clear_bits)))

    def select_box(self, box16, set_bits=0, clear_bits=0, flags=0):
        """state = (state & ~clear_bits) | set_bits for the splats inside the cutout box (SELECT_INVERT: outside) -> how many"""
        box = np.ascontiguousarray(box16, np.float32).reshape(16)
        hit = C.c_size_t(0)
        self._ck(self._L.gs_select_box(self._h, _p(box), int(set_bits), int(clear_bits), int(flags), C.byref(hit)))
        return hit.value

    def select_sphere(self, centre, radius, set_bits=0, clear_bits=0, flags=0):
        c = np.ascontiguousarray(centre, np.float32).reshape(3)
        hit = C.c_size_t(0)
        self._ck(self._L.gs_select_sphere(self._h, _p(c), float(np.float32(radius)), int(set_bits), int(clear_bits), int(flags), C.byref(hit)))
        return hit.value

    def select_rect(self, params, rect, set_bits=0, clear_bits=0, flags=0):
        """rect = (x0, y0, x1, y1) in pixels of the frame `params` describes, row 0 = top; among the splats of the last whole order"""
        r = np.ascontiguousarray(rect, np.int32).reshape(4)
        hit = C.c_size_t(0)
        self._ck(self._L.gs_select_rect(self._h, C.byref(params), _p(r), int(set_bits), int(clear_bits), int(flags), C.byref(hit)))
        return hit.value

    def select_mask(self, params, mask, depth_max=None, set_bits=0, clear_bits=0, flags=0):
        """mask: uint8[fb_height, fb_width] (a view with padded rows is passed with its stride), non-zero = inside; depth_max: optional
        float32[fb_height, fb_width] of window depths (the depth plane of render_surface: visible splats only) -> positions hit"""
        m, stride, d = _mask_args(params, mask, depth_max)
        hit = C.c_size_t(0)
        self._ck(self._L.gs_select_mask(self._h, C.byref(params), _p(m), stride, _p(d), int(set_bits), int(clear_bits), int(flags), C.byref(hit)))
        return hit.value

    def highlight_info(self):
        """(the value of OPT_HIGHLIGHT, 1 if the last frame was projected by the highlighting kernels)"""
        v, last = C.c_uint32(0), C.c_uint32(0)
        self._ck(self._L.gs_highlight_info(self._h, C.byref(v), C.byref(last)))
        return v.value, last.value

    def projection_info(self):
        """1 if the last frame was projected by the parallel kernels (RENDER_PARALLEL), else 0"""
        last = C.c_uint32(0)
        self._ck(self._L.gs_projection_info(self._h, C.byref(last)))
        return last.value

    # properties of the resident records (PROP_*): their range, a histogram, selection by value.  A splat takes part in the first two iff
    # (state & state_mask) == state_value
    def prop_range(self, prop, state_mask=0, state_value=0):
        """-> (min, max, n): of the non-NaN values among the splats that pass (+inf, -inf: none), and how many pass"""
        mn, mx, n = C.c_double(0), C.c_double(0), C.c_size_t(0)
        self._ck(self._L.gs_prop_range(self._h, int(prop), int(state_mask), int(state_value), C.byref(mn), C.byref(mx), C.byref(n)))
        return mn.value, mx.value, n.value

    def histogram(self, prop, lo, hi, nbins, state_mask=0, state_value=0):
        """-> (counts uint32[nbins], tally uint64[4] = passing, below lo, above hi, NaN)"""
        nb = int(nbins)
        counts = np.zeros(min(max(nb, 1), HIST_MAX_BINS), np.uint32)        # (a bin count out of range is the library's to refuse)
        tally = np.zeros(4, np.uint64)
        self._ck(self._L.gs_histogram(self._h, int(prop), float(lo), float(hi), nb & 0xFFFFFFFF, int(state_mask), int(state_value), _p(counts), _p(tally)))
        return counts, tally

    def select_range(self, prop, lo, hi, set_bits=0, clear_bits=0, flags=0):
        """state = (state & ~clear_bits) | set_bits for the splats with lo <= value <= hi (SELECT_INVERT: the others) -> how many"""
        hit = C.c_size_t(0)
        self._ck(self._L.gs_select_range(self._h, int(prop), float(lo), float(hi), int(set_bits), int(clear_bits), int(flags), C.byref(hit)))
        return hit.value

    def compact(self):
        """gs_compact: delete the hidden splats -> uint32[count afterwards], the old index of every splat that stays"""
        old = np.zeros(max(self.count(), 1), np.uint32)
        n = C.c_size_t(0)
        self._ck(self._L.gs_compact(self._h, _p(old), C.byref(n)))
        return old[:n.value].copy()

    # export: the resident cloud back to the host.  of: 'all' | 'visible' | 'selected' or (state_mask, state_value); reading calls
    def export_splat(self, of="all", want_wide=False, want_index=False):
        """gs_export_splat: the passing splats as .splat rows in ascending old index -> uint8[n, 32] (, float32[n, 7]) (, uint32[n])"""
        return _export_splat(self._L, self._L.gs_export_splat, self._h, self._ck, of, want_wide, want_index)

    def export_sh(self, of="all"):
        """gs_export_sh: the SH rows of the exported splats that have one (the first rows of export_splat) -> (float32[n, 3 (D+1)^2], D)"""
        m, v = _of(of)
        n, d = C.c_size_t(0), C.c_int(0)
        self._ck(self._L.gs_export_sh(self._h, m, v, None, C.byref(n), C.byref(d)))
        out = np.zeros((n.value, 3 * (d.value + 1) ** 2), np.float32)
        if n.value:
            self._ck(self._L.gs_export_sh(self._h, m, v, _p(out), C.byref(n), C.byref(d)))
        return out, d.value

    def export_ply(self, of="all", sh_degree=3):
        """gs_export_ply: the passing splats as the bytes of an INRIA .ply (uint8 array) with min(sh_degree, stored degree) SH bands"""
        return _export_ply(self._L.gs_export_ply, self._h, self._ck, of, sh_degree)

    def load_cply(self, ply_bytes):
        """gs_load_cply: decode a compressed .ply on the GPU and append its rows in file order (and its SH rows under load_ply's rule)"""
        buf = np.frombuffer(bytes(ply_bytes), np.uint8)
        self._ck(self._L.gs_load_cply(self._h, _p(buf), buf.size))

    def cply_to_splat_gpu(self, ply_bytes, want_wide=False):
        """gs_cply_to_splat_gpu: cply_to_splat by the decode kernel"""
        buf = np.frombuffer(bytes(ply_bytes), np.uint8)
        return _cply_rows(lambda *a: self._L.gs_cply_to_splat_gpu(self._h, *a), self._ck, buf, want_wide)

    def export_cply(self, of="all", sh_degree=3, morton=True, want_index=False):
        """gs_export_cply: the passing splats as the bytes of a compressed .ply (uint8 array) [, the resident index of every output row]"""
        return _export_cply(self._L.gs_export_cply, self._L.gs_export_splat, self._h, self._ck, of, sh_degree, morton, want_index)

    # in-place changes: colour and opacity of the splats that pass `of` on the GPU; rows and SH rows written over resident ones
    def adjust_colour(self, adjust, of="all"):
        """gs_adjust_colour: the ColourAdjust on the colour word and SH row of every passing splat -> how many pass"""
        return _adjust_colour(self._L.gs_adjust_colour, self._h, self._ck, adjust, of)

    def transform(self, t, of="all"):
        """gs_transform: the Similarity baked into every passing splat (records, sort rows, strip bounds, SH rows) -> how many pass;
        every order is dropped, as by a push"""
        return _transform(self._L.gs_transform, self._h, self._ck, t, of)

    def replace_splat(self, first, rows):
        """gs_replace_splat: .splat rows over splats [first, first + len(rows)); every order is dropped, as by a push"""
        _replace_splat(self._L.gs_replace_splat, self._h, self._ck, first, rows)

    def replace_sh(self, first, sh_rows, degree):
        rows, n = _sh_rows(sh_rows, degree)
        self._ck(self._L.gs_replace_sh(self._h, int(first), _p(rows), n, int(degree)))

    def state_count(self):
        """(rows in the state store, hidden splats among them)"""
        rows, hidden = C.c_size_t(0), C.c_size_t(0)
        self._ck(self._L.gs_state_count(self._h, C.byref(rows), C.byref(hidden)))
        return rows.value, hidden.value

    def download_state(self):
        return self.download(BUF_STATE, self.state_count()[0], np.uint8, 1).reshape(-1)

    # sort
    def sort(self, view, cutout=None, want_indices=True):
        view = np.ascontiguousarray(view, np.float32)
        cut = None if cutout is None else np.ascontiguousarray(cutout, np.float32)
        if not want_indices:
            self._ck(self._L.gs_sort(self._h, _p(view), _p(cut), None, None))
            return None
        out = np.zeros(max(self.count(), 1), np.uint32)
        n = C.c_uint32(0)
        self._ck(self._L.gs_sort(self._h, _p(view), _p(cut), _p(out), C.byref(n)))
        return out[:n.value].copy()

    def sort_begin(self, view, cutout=None):
        """gs_sort_begin: post the sort and return (the reference's tick, index.js:438-455); draws keep using the last completed order"""
        view = np.ascontiguousarray(view, np.float32)
        cut = None if cutout is None else np.ascontiguousarray(cutout, np.float32)
        self._ck(self._L.gs_sort_begin(self._h, _p(view), _p(cut)))

    def sort_poll(self, wait=False, want_indices=True):
        """gs_sort_poll: None while the sort begun with sort_begin() runs; else the new order (installed for the draws that follow), or
        True with want_indices=False"""
        out = np.zeros(max(self.count(), 1), np.uint32) if want_indices else None
        n, done = C.c_uint32(0), C.c_int(0)
        self._ck(self._L.gs_sort_poll(self._h, 1 if wait else 0, _p(out), C.byref(n), C.byref(done)))
        if not done.value:
            return None
        return out[:n.value].copy() if want_indices else True

    def sort_for(self, view, cutout, strip_params, want_indices=True):
        """gs_sort_for: the order of the splats that can reach strip_params' column strip (a sub-sequence of sort()'s result)."""
        view = np.ascontiguousarray(view, np.float32)
        cut = None if cutout is None else np.ascontiguousarray(cutout, np.float32)
        if not want_indices:
            self._ck(self._L.gs_sort_for(self._h, _p(view), _p(cut), C.byref(strip_params), None, None))
            return None
        out = np.zeros(max(self.count(), 1), np.uint32)
        n = C.c_uint32(0)
        self._ck(self._L.gs_sort_for(self._h, _p(view), _p(cut), C.byref(strip_params), _p(out), C.byref(n)))
        return out[:n.value].copy()

    def sort_gathered(self, view, cutout, views):
        """the sort of a frame drawn with render_gathered(views): only this rank's strip when it owns exactly one"""
        views = list(views) if isinstance(views, (list, tuple)) else [views]
        arr = (RenderParams * len(views))(*views)
        view = np.ascontiguousarray(view, np.float32)
        cut = None if cutout is None else np.ascontiguousarray(cutout, np.float32)
        self._ck(self._L.gs_sort_gathered(self._h, _p(view), _p(cut), arr, len(views)))

    # render
    def render(self, params, flip=False):
        sw = max(params.x1 - params.x0, 0)
        out = np.zeros((max(params.fb_height, 0), sw, 4), np.uint8)
        scratch = out if out.size else np.zeros(4, np.uint8)          # let the library reject bad sizes itself
        self._ck(self._L.gs_render(self._h, C.byref(params), _p(scratch), 0))
        return out

    def render_into(self, params, out):
        """gs_render into a caller-owned H x w x 4 uint8 array (e.g. page-locked memory from host_frame())."""
        self._ck(self._L.gs_render(self._h, C.byref(params), _p(out), out.strides[0]))
        return out

    def render_device(self, params, device_ptr=None):
        self._ck(self._L.gs_render_device(self._h, C.byref(params), C.c_void_p(device_ptr) if device_ptr else None))

    # surface output: what lies under a pixel
    def render_surface(self, params, rgba=True, planes=("id", "depth", "alpha")):
        """gs_render_surface -> (rgba | None, id, depth, alpha): the frame and, per pixel, the splat at which the transmittance falls
        below one half (SURFACE_NONE: never), its window depth (1.0: none) and the accumulated alpha.  A plane not named in `planes`
        is not asked for (None)."""
        h, sw = max(params.fb_height, 0), max(params.x1 - params.x0, 0)
        out = np.zeros((h, sw, 4), np.uint8) if rgba else None
        pid = np.zeros((h, sw), np.uint32) if "id" in planes else None
        dep = np.zeros((h, sw), np.float32) if "depth" in planes else None
        alp = np.zeros((h, sw), np.float32) if "alpha" in planes else None
        s = Surface(*[a.ctypes.data if a is not None and a.size else None for a in (pid, dep, alp)])
        self._ck(self._L.gs_render_surface(self._h, C.byref(params), _p(out) if rgba and out.size else None, 0, C.byref(s)))
        return out, pid, dep, alp

    def render_surface_device(self, params, device_rgba=None, id_ptr=None, depth_ptr=None, alpha_ptr=None):
        s = Surface(id_ptr or None, depth_ptr or None, alpha_ptr or None)
        self._ck(self._L.gs_render_surface_device(self._h, C.byref(params), C.c_void_p(device_rgba) if device_rgba else None, C.byref(s)))

    # per-splat contribution: the blend weights a splat's fragments had in the frames drawn by render_contrib
    def render_contrib(self, params, want_rgba=True):
        """gs_render_contrib -> rgba | None: the frame gs_render draws on the tile lists; every applied fragment adds its weight
        alpha * exp(-q) * T, as 16.16 fixed point, to its splat's word of the contribution store (download_contrib, PROP_SEEN)"""
        h, sw = max(params.fb_height, 0), max(params.x1 - params.x0, 0)
        out = np.zeros((h, sw, 4), np.uint8) if want_rgba else None
        self._ck(self._L.gs_render_contrib(self._h, C.byref(params), _p(out) if want_rgba and out.size else None, 0))
        return out

    def render_contrib_device(self, params, device_rgba=None):
        self._ck(self._L.gs_render_contrib_device(self._h, C.byref(params), C.c_void_p(device_rgba) if device_rgba else None))

    def contrib_clear(self):
        self._ck(self._L.gs_contrib_clear(self._h))

    def contrib_info(self):
        """(rows in the contribution store, contribution frames that drew since it was last emptied)"""
        rows, frames = C.c_size_t(0), C.c_uint64(0)
        self._ck(self._L.gs_contrib_info(self._h, C.byref(rows), C.byref(frames)))
        return rows.value, frames.value

    def download_contrib(self):
        """the contribution store: uint64[rows], each the sum of its splat's weights * 65536"""
        rows = self.contrib_info()[0]
        if not rows:
            return np.zeros(0, np.uint64)
        return self.download(BUF_CONTRIB, rows, np.uint64, 1).reshape(-1)

    def pick(self, params, points):
        """gs_pick: points = (n, 2) int (column, row; row 0 = top) -> structured array (id, depth, alpha, pos[3]) of what the full
        frame's planes hold there; pos = the hit splat's position as its .splat row stores it (NaN where id == SURFACE_NONE)."""
        pts = np.ascontiguousarray(np.asarray(points, np.int32).reshape(-1, 2))
        out = np.zeros(max(len(pts), 1), HIT_DTYPE)
        assert HIT_DTYPE.itemsize == C.sizeof(Hit)
        self._ck(self._L.gs_pick(self._h, C.byref(params), _p(pts) if len(pts) else None, len(pts), _p(out)))
        return out[:len(pts)]

    def render_stereo(self, left, right):
        arr = (RenderParams * 2)(left, right)
        o0 = np.zeros((left.fb_height, left.x1 - left.x0, 4), np.uint8)
        o1 = np.zeros((right.fb_height, right.x1 - right.x0, 4), np.uint8)
        outs = (C.c_void_p * 2)(o0.ctypes.data, o1.ctypes.data)
        self._ck(self._L.gs_render_stereo(self._h, arr, outs, 0))
        return o0, o1

    def set_scene(self, depth=None, rgba=None):
        """Opaque-scene inputs (depthTest LEQUAL against `depth` [H,W] f32 window depth; blend over `rgba` [H,W,4] u8)."""
        if depth is None and rgba is None:
            self._ck(self._L.gs_set_scene(self._h, None, None, 0, 0))
            return
        d = None if depth is None else np.ascontiguousarray(depth, np.float32)
        c = None if rgba is None else np.ascontiguousarray(rgba, np.uint8)
        h, w = (d.shape if d is not None else c.shape[:2])
        self._ck(self._L.gs_set_scene(self._h, _p(d), _p(c), int(w), int(h)))

    def sync(self):
        self._ck(self._L.gs_sync(self._h))

    def set_stream(self, stream_ptr):
        self._ck(self._L.gs_set_stream(self._h, C.c_void_p(stream_ptr) if stream_ptr else None))

    def frame_stream(self):
        """hipStream_t (as an int) of the lane the current frame was enqueued on."""
        return int(self._L.gs_frame_stream(self._h) or 0)

    def frame_status_device(self):
        """device address (int) of the current frame's completion word: one uint32, 0 = complete, else drawn again at sync()"""
        p = C.c_void_p()
        self._ck(self._L.gs_frame_status_device(self._h, C.byref(p)))
        return int(p.value or 0)

    def frame_status(self):
        """the completion word read back once the frame's stream is idle (a test's view of it: a GPU-side consumer reads the word itself)"""
        addr, st = self.frame_status_device(), self.frame_stream()
        hip = hip_runtime()
        hip.hipStreamSynchronize(C.c_void_p(st))
        v = C.c_uint32(0)
        hip.hipMemcpy(C.byref(v), C.c_void_p(addr), C.c_size_t(4), 2)
        return int(v.value)

    def frame_lane(self):
        """Index of the pipeline lane the current frame went to (no waiting)."""
        return int(self._L.gs_frame_lane(self._h))

    def lane_stream(self, lane):
        """hipStream_t of a lane, once its worker thread has enqueued everything handed to it so far."""
        return int(self._L.gs_lane_stream(self._h, int(lane)) or 0)

    def wait_stream(self, stream_ptr):
        """The next frame starts (on the GPU) only after everything queued on the given hipStream_t so far."""
        self._ck(self._L.gs_wait_stream(self._h, C.c_void_p(stream_ptr)))

    def stream_wait_frame(self, stream_ptr):
        """The given hipStream_t waits (on the GPU) for the frame enqueued last."""
        self._ck(self._L.gs_stream_wait_frame(self._h, C.c_void_p(stream_ptr)))

    # ---- several GPUs (one Context per GPU; see gs_splat.h) ----
    def comm_unique_id(self, transport=None):
        """rank 0: the id every rank passes to comm_init.  transport: TRANSPORT_RCCL / TRANSPORT_INPROC (None = as set)."""
        if transport is not None:
            self.set_option(OPT_COMM_TRANSPORT, transport)
        buf = (C.c_uint8 * COMM_ID_BYTES)()
        self._ck(self._L.gs_comm_unique_id(self._h, buf))
        return bytes(buf)

    def comm_init(self, uid, rank, world):
        buf = (C.c_uint8 * COMM_ID_BYTES).from_buffer_copy(bytes(uid))
        self._ck(self._L.gs_comm_init(self._h, buf, int(rank), int(world)))

    def render_gathered(self, views, root=0, device_frames=None, flags=0):
        """views: one RenderParams (column strips over the ranks) or two (XR eyes).  Asynchronous with RENDER_ASYNC."""
        views = list(views) if isinstance(views, (list, tuple)) else [views]
        arr = (RenderParams * len(views))(*views)
        ptrs = None
        if device_frames is not None:
            ptrs = (C.c_void_p * len(views))(*[C.c_void_p(int(p)) if p else None for p in device_frames])
        self._ck(self._L.gs_render_gathered(self._h, arr, len(views), int(root), ptrs, int(flags)))

    def gathered_size(self, view):
        w, h = C.c_int(0), C.c_int(0)
        self._ck(self._L.gs_gathered_size(self._h, int(view), C.byref(w), C.byref(h)))
        return w.value, h.value

    def read_gathered(self, view, width=None, height=None):
        """root: view `view` of the last gathered frame as H x W x 4 uint8 (the size is the library's; width / height, if
        given, are checked against it)."""
        w, h = self.gathered_size(view)
        if (width is not None and int(width) != w) or (height is not None and int(height) != h):
            raise ValueError("gathered frame %d is %dx%d, not %sx%s" % (view, w, h, width, height))
        out = np.empty((h, w, 4), np.uint8)
        self._ck(self._L.gs_read_gathered(self._h, int(view), _p(out), 0))
        return out

    def set_option(self, opt, value):
        self._ck(self._L.gs_set_option(self._h, int(opt), int(value)))

    def stats(self):
        s = Stats()
        self._ck(self._L.gs_get_stats(self._h, C.byref(s)))
        return s.as_dict()

    def sort_inspect(self, want_indices=True):
        """gs_sort_inspect: the current lane's order as it lies -> (info dict, uint32[n_records] or None); also collects that sort for the
        near-only forms' bookkeeping (include/gs_splat.h)"""
        info = SortInfo()
        out = np.zeros(max(self.count(), 1), np.uint32) if want_indices else None
        self._ck(self._L.gs_sort_inspect(self._h, C.byref(info), _p(out), 0 if out is None else out.size))
        return info.as_dict(), (None if out is None else out[:info.n_records].copy())

    def download(self, which, count, dtype, width):
        out = np.zeros((count, width), dtype)
        self._ck(self._L.gs_download(self._h, int(which), _p(out), out.nbytes))
        return out


class Multi:
    """gs_multi: one host process, several GPUs (or several "devices" on one GPU): the single-context calls over all of them."""

    def __init__(self, devices):
        self._L = load()
        devs = [int(d) for d in devices]
        arr = (C.c_int * len(devs))(*devs)
        h = C.c_void_p()
        rc = self._L.gs_create_multi(arr, len(devs), C.byref(h))
        if rc != GS_OK:
            raise GsError(rc, self._L.gs_multi_last_error(None).decode())
        self._h = h
        self.devices = devs

    def close(self):
        if getattr(self, "_h", None):
            self._L.gs_multi_destroy(self._h)
            self._h = None

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def _ck(self, rc):
        if rc != GS_OK:
            raise GsError(rc, self._L.gs_multi_last_error(self._h).decode())

    def ctx_stats(self, i):
        """gs_get_stats of the context on devices[i] (call sync() first)"""
        s = Stats()
        h = self._L.gs_multi_ctx(self._h, int(i))
        rc = self._L.gs_get_stats(h, C.byref(s))
        if rc != GS_OK:
            raise GsError(rc, self._L.gs_last_error(h).decode())
        return s.as_dict()

    def ctx_highlight_info(self, i):
        """gs_highlight_info of the context on devices[i] (call sync() first)"""
        v, last = C.c_uint32(0), C.c_uint32(0)
        h = self._L.gs_multi_ctx(self._h, int(i))
        rc = self._L.gs_highlight_info(h, C.byref(v), C.byref(last))
        if rc != GS_OK:
            raise GsError(rc, self._L.gs_last_error(h).decode())
        return v.value, last.value

    def ctx_projection_info(self, i):
        """gs_projection_info of the context on devices[i] (call sync() first)"""
        last = C.c_uint32(0)
        h = self._L.gs_multi_ctx(self._h, int(i))
        rc = self._L.gs_projection_info(h, C.byref(last))
        if rc != GS_OK:
            raise GsError(rc, self._L.gs_last_error(h).decode())
        return last.value

    def clear(self):
        self._ck(self._L.gs_multi_clear(self._h))

    def push_splat(self, rows):
        rows = np.ascontiguousarray(np.asarray(rows).view(np.uint8).reshape(-1))
        if rows.size % 32:
            raise ValueError("rows must be a multiple of 32 bytes")
        self._ck(self._L.gs_multi_push_splat(self._h, _p(rows), rows.size // 32))

    def load_ply(self, ply_bytes):
        buf = np.frombuffer(bytes(ply_bytes), np.uint8)
        self._ck(self._L.gs_multi_load_ply(self._h, _p(buf), buf.size))

    def push_sh(self, sh_rows, degree):
        rows, n = _sh_rows(sh_rows, degree)
        self._ck(self._L.gs_multi_push_sh(self._h, _p(rows), n, int(degree)))

    def count(self):
        return self._L.gs_multi_count(self._h)

    # editing the resident cloud: per-splat state bytes (STATE_HIDDEN leaves every sort), region selection, deletion
    def set_state(self, first, states):
        st = np.ascontiguousarray(states, np.uint8).reshape(-1)
        self._ck(self._L.gs_multi_set_state(self._h, int(first), _p(st), st.size))

    def set_state_ids(self, ids, set_bits=0, clear_bits=0):
        ids = np.ascontiguousarray(ids, np.uint32).reshape(-1)
        self._ck(self._L.gs_multi_set_state_ids(self._h, _p(ids), ids.size, int(set_bits), int(clear_bits)))

    def select_box(self, box16, set_bits=0, clear_bits=0, flags=0):
        """state = (state & ~clear_bits) | set_bits for the splats inside the cutout box (SELECT_INVERT: outside) -> how many"""
        box = np.ascontiguousarray(box16, np.float32).reshape(16)
        hit = C.c_size_t(0)
        self._ck(self._L.gs_multi_select_box(self._h, _p(box), int(set_bits), int(clear_bits), int(flags), C.byref(hit)))
        return hit.value

    def select_sphere(self, centre, radius, set_bits=0, clear_bits=0, flags=0):
        c = np.ascontiguousarray(centre, np.float32).reshape(3)
        hit = C.c_size_t(0)
        self._ck(self._L.gs_multi_select_sphere(self._h, _p(c), float(np.float32(radius)), int(set_bits), int(clear_bits), int(flags), C.byref(hit)))
        return hit.value

    def select_rect(self, params, rect, set_bits=0, clear_bits=0, flags=0):
        """rect = (x0, y0, x1, y1) in pixels of the frame `params` describes, row 0 = top; among the splats of the last whole order"""
        r = np.ascontiguousarray(rect, np.int32).reshape(4)
        hit = C.c_size_t(0)
        self._ck(self._L.gs_multi_select_rect(self._h, C.byref(params), _p(r), int(set_bits), int(clear_bits), int(flags), C.byref(hit)))
        return hit.value

    def select_mask(self, params, mask, depth_max=None, set_bits=0, clear_bits=0, flags=0):
        """Context.select_mask on every device -> the positions hit on devices[0]"""
        m, stride, d = _mask_args(params, mask, depth_max)
        hit = C.c_size_t(0)
        self._ck(self._L.gs_multi_select_mask(self._h, C.byref(params), _p(m), stride, _p(d), int(set_bits), int(clear_bits), int(flags), C.byref(hit)))
        return hit.value

    # properties of the resident records (PROP_*): their range, a histogram, selection by value.  A splat takes part in the first two iff
    # (state & state_mask) == state_value
    def prop_range(self, prop, state_mask=0, state_value=0):
        """-> (min, max, n): of the non-NaN values among the splats that pass (+inf, -inf: none), and how many pass"""
        mn, mx, n = C.c_double(0), C.c_double(0), C.c_size_t(0)
        self._ck(self._L.gs_multi_prop_range(self._h, int(prop), int(state_mask), int(state_value), C.byref(mn), C.byref(mx), C.byref(n)))
        return mn.value, mx.value, n.value

    def histogram(self, prop, lo, hi, nbins, state_mask=0, state_value=0):
        """-> (counts uint32[nbins], tally uint64[4] = passing, below lo, above hi, NaN)"""
        nb = int(nbins)
        counts = np.zeros(min(max(nb, 1), HIST_MAX_BINS), np.uint32)        # (a bin count out of range is the library's to refuse)
        tally = np.zeros(4, np.uint64)
        self._ck(self._L.gs_multi_histogram(self._h, int(prop), float(lo), float(hi), nb & 0xFFFFFFFF, int(state_mask), int(state_value), _p(counts), _p(tally)))
        return counts, tally

    def select_range(self, prop, lo, hi, set_bits=0, clear_bits=0, flags=0):
        """state = (state & ~clear_bits) | set_bits for the splats with lo <= value <= hi (SELECT_INVERT: the others) -> how many"""
        hit = C.c_size_t(0)
        self._ck(self._L.gs_multi_select_range(self._h, int(prop), float(lo), float(hi), int(set_bits), int(clear_bits), int(flags), C.byref(hit)))
        return hit.value

    def compact(self):
        """gs_compact: delete the hidden splats -> uint32[count afterwards], the old index of every splat that stays"""
        old = np.zeros(max(self.count(), 1), np.uint32)
        n = C.c_size_t(0)
        self._ck(self._L.gs_multi_compact(self._h, _p(old), C.byref(n)))
        return old[:n.value].copy()

    def export_splat(self, of="all", want_wide=False, want_index=False):
        """gs_multi_export_splat: Context.export_splat on devices[0] (every device holds the same splats)"""
        return _export_splat(self._L, self._L.gs_multi_export_splat, self._h, self._ck, of, want_wide, want_index)

    def export_ply(self, of="all", sh_degree=3):
        return _export_ply(self._L.gs_multi_export_ply, self._h, self._ck, of, sh_degree)

    def load_cply(self, ply_bytes):
        buf = np.frombuffer(bytes(ply_bytes), np.uint8)
        self._ck(self._L.gs_multi_load_cply(self._h, _p(buf), buf.size))

    def export_cply(self, of="all", sh_degree=3, morton=True, want_index=False):
        return _export_cply(self._L.gs_multi_export_cply, self._L.gs_multi_export_splat, self._h, self._ck, of, sh_degree, morton, want_index)

    # in-place changes: colour and opacity of the splats that pass `of` on the GPU; rows and SH rows written over resident ones
    def adjust_colour(self, adjust, of="all"):
        """gs_adjust_colour: the ColourAdjust on the colour word and SH row of every passing splat -> how many pass"""
        return _adjust_colour(self._L.gs_multi_adjust_colour, self._h, self._ck, adjust, of)

    def transform(self, t, of="all"):
        """gs_transform on every device -> how many pass on devices[0]"""
        return _transform(self._L.gs_multi_transform, self._h, self._ck, t, of)

    def replace_splat(self, first, rows):
        """gs_replace_splat: .splat rows over splats [first, first + len(rows)); every order is dropped, as by a push"""
        _replace_splat(self._L.gs_multi_replace_splat, self._h, self._ck, first, rows)

    def replace_sh(self, first, sh_rows, degree):
        rows, n = _sh_rows(sh_rows, degree)
        self._ck(self._L.gs_multi_replace_sh(self._h, int(first), _p(rows), n, int(degree)))

    def set_option(self, opt, value):
        self._ck(self._L.gs_multi_set_option(self._h, int(opt), int(value)))

    @staticmethod
    def _views(views):
        views = list(views) if isinstance(views, (list, tuple)) else [views]
        return (RenderParams * len(views))(*views), len(views)

    def sort(self, view, cutout, views):
        arr, n = self._views(views)
        view = np.ascontiguousarray(view, np.float32)
        cut = None if cutout is None else np.ascontiguousarray(cutout, np.float32)
        self._ck(self._L.gs_multi_sort(self._h, _p(view), _p(cut), arr, n))

    def render(self, views, frames, flags=0):
        """host-direct: frames = one H x W x 4 uint8 array per view (page-locked: host_frame()); strips are copied into them"""
        arr, n = self._views(views)
        frames = list(frames) if isinstance(frames, (list, tuple)) else [frames]
        ptrs = (C.c_void_p * n)(*[f.ctypes.data for f in frames])
        self._ck(self._L.gs_multi_render(self._h, arr, n, ptrs, frames[0].strides[0], int(flags)))

    def render_device(self, views, device_frames=None, flags=0):
        arr, n = self._views(views)
        ptrs = None
        if device_frames is not None:
            ptrs = (C.c_void_p * n)(*[C.c_void_p(int(p)) if p else None for p in device_frames])
        self._ck(self._L.gs_multi_render_device(self._h, arr, n, ptrs, int(flags)))

    def read(self, view, width, height):
        out = np.empty((int(height), int(width), 4), np.uint8)
        self._ck(self._L.gs_multi_read(self._h, int(view), _p(out), 0))
        return out

    def sync(self):
        self._ck(self._L.gs_multi_sync(self._h))
