"""4dgaussiansplatrendering_amd — ctypes binding of libgs4d.so (include/gs4d.h).

The product is the HIP library; this module is plumbing for the tests and bench.py.  It has no CPU
fallback: importing it without the built library, or creating a Context without a GPU, raises.

(The directory name starts with a digit, so import it with
``importlib.import_module("4dgaussiansplatrendering_amd")``.)
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libgs4d.so")

MODE_4D_SORTED, MODE_4D_DIRECT, MODE_3D_FULL, MODE_2D = 0, 1, 2, 3
U_TIME, U_MIN_OPACITY = 0, 1
U_VIEW, U_PROJ = 0, 1
# glBlendFunc factors (GL enum values): the reference's blend menu, DebugMenus.h:41-59
ZERO, ONE, SRC_COLOR, ONE_MINUS_SRC_COLOR, SRC_ALPHA, ONE_MINUS_SRC_ALPHA = 0, 1, 0x0300, 0x0301, 0x0302, 0x0303
DST_ALPHA, ONE_MINUS_DST_ALPHA, DST_COLOR, ONE_MINUS_DST_COLOR = 0x0304, 0x0305, 0x0306, 0x0307
CONSTANT_COLOR, ONE_MINUS_CONSTANT_COLOR, CONSTANT_ALPHA, ONE_MINUS_CONSTANT_ALPHA = 0x8001, 0x8002, 0x8003, 0x8004
KEY_REF_INV_EUCLID, KEY_VIEW_Z = 0, 1
KEEP_INVERT = 1                                           # gs4d_keep_rule.flags: keep exactly the records the rule would drop
STAT_PIXELS, STAT_WMAX, STAT_WSUM = 0, 1, 2               # gs4d_stat_cut: the field of gs4d_record_stat
PARAMS_3D, PARAMS_4D_VEL, PARAMS_4D_2Q = 0, 1, 2           # gs4d_splat_params.form
EDIT_SET, EDIT_MUL, EDIT_LERP, EDIT_COPY = 0, 1, 2, 3      # gs4d_colour_edit.op
CQ_BOX, CQ_SPHERE, CQ_SCREEN, CQ_FRAME, CQ_SKIP_HIDDEN, CQ_SKIP_DEAD = 1, 2, 4, 8, 16, 32      # gs4d_centre_query.tests
CQ_ADD, CQ_REMOVE = 0, 1                                   # gs4d_centre_query.op
MS_SKIP_HIDDEN, MS_SKIP_DEAD = 1, 2                        # gs4d_measure_query.flags
POSE_INDEX, POSE_BLEND4 = 0, 1                             # gs4d_pose_records: the form of a bind row
SH_EACH = 2                                                # gs4d_rotate_sh: no bind table, every map to every row
XS_PIVOT, XS_PIVOT_MEASURE = 1, 2                          # gs4d_selection_xf.flags
NB_SKIP_HIDDEN, NB_SKIP_DEAD, NB_COUNT_SELF = 1, 2, 4      # gs4d_neighbour_query.flags
CC_SKIP_HIDDEN, CC_SKIP_DEAD = 1, 2                        # gs4d_component_query.flags
NN_SKIP_HIDDEN, NN_SKIP_DEAD, NN_INCLUDE_SELF = 1, 2, 4    # gs4d_nearest_query.flags
ID_NONE = 0xFFFFFFFF                                       # GS4D_ID_NONE: the label of a record that is no member
TIME_DEAD_ARG = -106.0                                    # GS4D_TIME_DEAD_ARG: no float32 exponential is non-zero below this argument
STAGES = ("keygen", "sort", "preprocess", "binning", "pairsort", "composite")
CLEAR_COLOR = (0.18431373, 0.20784314, 0.25882353, 1.0)   # Application.cpp:125


class Gs4dError(RuntimeError):
    pass


def _load():
    if not os.path.exists(LIB_PATH):
        raise ImportError(f"{LIB_PATH} is missing: build it with `make lib` (or __graft_entry__.build()); there is no CPU fallback")
    lib = C.CDLL(LIB_PATH)
    vp, sz, u32, i32, f32 = C.c_void_p, C.c_size_t, C.c_uint32, C.c_int, C.c_float
    sig = {
        "gs4d_create": (i32, [i32, i32, i32, C.POINTER(vp)]),
        "gs4d_destroy": (None, [vp]),
        "gs4d_resize": (i32, [vp, i32, i32]),
        "gs4d_last_error": (C.c_char_p, [vp]),
        "gs4d_buffer_create": (i32, [vp, vp, sz, C.POINTER(u32)]),
        "gs4d_buffer_subdata": (i32, [vp, u32, sz, vp, sz]),
        "gs4d_buffer_read": (i32, [vp, u32, sz, vp, sz]),
        "gs4d_buffer_destroy": (i32, [vp, u32]),
        "gs4d_buffer_device_ptr": (i32, [vp, u32, C.POINTER(vp), C.POINTER(sz)]),
        "gs4d_buffer_invalidate": (i32, [vp, u32]),
        "gs4d_bind_storage": (i32, [vp, i32, u32]),
        "gs4d_set_mode": (i32, [vp, i32]),
        "gs4d_set_uniform_1f": (i32, [vp, i32, f32]),
        "gs4d_set_uniform_mat4": (i32, [vp, i32, vp]),
        "gs4d_set_clear_color": (i32, [vp, vp]),
        "gs4d_set_blend": (i32, [vp, i32, i32]),
        "gs4d_clear": (i32, [vp]),
        "gs4d_sort_pairs": (i32, [vp, u32, u32, sz]),
        "gs4d_keygen": (i32, [vp, u32, f32, vp, u32, u32, sz, i32]),
        "gs4d_draw_instanced": (i32, [vp, sz]),
        "gs4d_draw_quads": (i32, [vp, u32, sz]),
        "gs4d_draw_lines": (i32, [vp, vp, sz, i32, i32, vp, vp, f32]),
        "gs4d_host_camera_input": (None, [vp, vp, vp, vp]),
        "gs4d_host_camera_rotate": (None, [vp, C.c_double, C.c_double]),
        "gs4d_host_camera_look_at_point": (None, [vp, vp]),
        "gs4d_host_camera_viewport": (None, [i32, i32, vp]),
        "gs4d_host_camera_focal": (None, [f32, i32, i32, vp]),
        "gs4d_host_unproject": (None, [vp, vp, i32, i32, f32, f32, f32, vp]),
        "gs4d_read_pixels": (i32, [vp, vp, sz]),
        "gs4d_read_pixels_device": (i32, [vp, vp, sz]),
        "gs4d_read_pixels_rgba8_device": (i32, [vp, vp, sz]),
        "gs4d_read_frame_rgba8_device": (i32, [vp, i32, vp, sz]),
        "gs4d_read_frame_rgba8_device_after": (i32, [vp, i32, vp, sz, vp]),
        "gs4d_set_tile_shard": (i32, [vp, i32, i32]),
        "gs4d_band_rows": (i32, [vp, vp]),
        "gs4d_read_band_rgba8_device": (i32, [vp, vp, sz]),
        "gs4d_set_stream": (i32, [vp, vp]),
        "gs4d_finish": (i32, [vp]),
        "gs4d_set_aux_outputs": (i32, [vp, i32]),
        "gs4d_read_aux": (i32, [vp, vp, sz]),
        "gs4d_read_aux_device": (i32, [vp, vp, sz]),
        "gs4d_set_id_outputs": (i32, [vp, i32]),
        "gs4d_read_ids": (i32, [vp, i32, i32, i32, i32, vp, vp, vp]),
        "gs4d_read_ids_device": (i32, [vp, vp, vp, vp, sz]),
        "gs4d_set_depth_test": (i32, [vp, u32]),
        "gs4d_set_record_stats": (i32, [vp, u32, sz]),
        "gs4d_compact_records": (i32, [vp, u32, sz, vp, u32, sz, u32, u32, u32]),
        "gs4d_stat_cut": (i32, [vp, u32, sz, i32, sz, u32]),
        "gs4d_count_ids": (i32, [vp, vp, u32, u32, sz]),
        "gs4d_record_time_spans": (i32, [vp, u32, sz, f32, u32]),
        "gs4d_compact_time_window": (i32, [vp, u32, sz, f32, f32, u32, sz, u32, u32, u32]),
        "gs4d_spatial_order": (i32, [vp, u32, sz, sz, sz, u32]),
        "gs4d_gather_records": (i32, [vp, u32, sz, u32, sz, sz, u32]),
        "gs4d_shade_sh": (i32, [vp, u32, sz, u32, sz, i32, f32, vp]),
        "gs4d_shade_sh_t": (i32, [vp, u32, sz, u32, sz, vp]),
        "gs4d_collapse_sh": (i32, [vp, u32, sz, u32, sz, vp, u32, sz]),
        "gs4d_edit_colours": (i32, [vp, u32, sz, vp, u32, vp, u32]),
        "gs4d_count_centres": (i32, [vp, u32, sz, vp, u32, u32]),
        "gs4d_measure_records": (i32, [vp, u32, sz, vp, u32, vp, u32]),
        "gs4d_build_records": (i32, [vp, vp, sz, u32]),
        "gs4d_decompose_records": (i32, [vp, u32, sz, sz, vp]),
        "gs4d_transform_records": (i32, [vp, u32, sz, u32, sz, u32, sz]),
        "gs4d_transform_selected": (i32, [vp, u32, sz, vp, u32, vp, u32]),
        "gs4d_pose_records": (i32, [vp, u32, sz, u32, sz, u32, u32, sz, u32, sz]),
        "gs4d_rotate_sh": (i32, [vp, u32, sz, sz, i32, u32, sz, u32, u32, sz, u32, sz]),
        "gs4d_warp_records": (i32, [vp, u32, sz, u32, vp, u32, sz]),
        "gs4d_slice_records": (i32, [vp, u32, sz, vp, u32, sz]),
        "gs4d_count_neighbours": (i32, [vp, u32, sz, vp, u32, vp, u32]),
        "gs4d_label_components": (i32, [vp, u32, sz, vp, u32, vp, u32, u32]),
        "gs4d_count_labels": (i32, [vp, u32, sz, u32, vp, u32]),
        "gs4d_nearest_neighbours": (i32, [vp, u32, sz, vp, u32, vp, u32, sz, u32]),
        "gs4d_cell_labels": (i32, [vp, u32, sz, vp, u32]),
        "gs4d_merge_records": (i32, [vp, u32, sz, u32, vp, u32, vp, u32, u32, u32, u32]),
        "gs4d_merge_rows": (i32, [vp, u32, sz, u32, u32, vp, u32, sz, u32]),
        "gs4d_copy_rows": (i32, [vp, u32, sz, sz, sz, u32, sz]),
        "gs4d_lod_append": (i32, [vp, u32, sz, u32, sz, sz, u32, u32, sz]),
        "gs4d_lod_cut": (i32, [vp, u32, u32, sz, vp, u32, u32, u32, u32]),
        "gs4d_set_profiling": (i32, [vp, i32]),
        "gs4d_get_timings": (i32, [vp, vp]),
        "gs4d_get_timeline": (i32, [vp, vp, i32, vp]),
        "gs4d_get_stats": (i32, [vp, vp]),
        "gs4d_get_sort_stats": (i32, [vp, vp]),
        "gs4d_debug_read_projected": (i32, [vp, vp, sz]),
        "gs4d_debug_shadow_builds": (i32, [vp, u32, C.POINTER(C.c_uint64)]),
        "gs4d_host_look_at": (None, [vp, vp, vp, vp]),
        "gs4d_host_perspective": (None, [f32, i32, i32, f32, f32, vp]),
        "gs4d_host_key_bounds": (None, [vp, vp, f32, vp, i32, C.POINTER(u32), C.POINTER(u32)]),
        "gs4d_host_quat_look_at": (None, [vp, vp, vp]),
        "gs4d_host_splat3d_cov": (None, [vp, vp, vp]),
        "gs4d_host_splat3d_mesh": (None, [vp, vp, vp, vp, vp]),
        "gs4d_host_splat2d_sigma_inv": (None, [vp, f32, f32, vp]),
        "gs4d_host_gaussians2d_record": (None, [f32, f32, f32, f32, f32, vp, vp]),
        "gs4d_host_splat4d_cov": (None, [vp, vp, f32, f32, vp, vp]),
        "gs4d_host_splat4d_cov2q": (None, [vp, vp, vp, vp]),
        "gs4d_host_build_records_3d": (None, [sz, vp, vp, vp, vp, vp]),
        "gs4d_host_build_records_4d": (None, [sz, vp, vp, vp, vp, vp, vp, vp, vp]),
        "gs4d_host_time_variance": (f32, [f32, f32]),
        "gs4d_host_time_variances": (None, [sz, vp, vp, vp]),
        "gs4d_host_build_records_4d_tvar": (None, [sz, vp, vp, vp, vp, vp, vp, vp]),
        "gs4d_host_build_records_4d_2q": (None, [sz, vp, vp, vp, vp, vp, vp]),
        "gs4d_host_decompose_records": (None, [sz, vp, u32, vp, vp, vp, vp, vp, vp]),
        "gs4d_host_transform_records": (None, [sz, vp, vp, vp]),
        "gs4d_host_pose_records": (None, [sz, vp, vp, sz, vp, u32, sz, vp]),
        "gs4d_host_sh_rotation": (i32, [vp, vp]),
        "gs4d_host_rotate_sh": (None, [sz, vp, sz, i32, vp, sz, vp, u32, sz, vp]),
        "gs4d_host_sh_time_weights": (None, [vp, f32, vp, C.POINTER(i32)]),
        "gs4d_host_collapse_sh": (None, [sz, vp, vp, sz, vp, vp, sz]),
        "gs4d_host_shade_sh_t": (None, [sz, vp, vp, sz, vp]),
        "gs4d_host_warp_records": (None, [sz, vp, vp, vp, vp]),
        "gs4d_host_slice_records": (None, [sz, vp, vp, vp]),
        "gs4d_host_edit_colours": (None, [sz, vp, vp, vp, vp, vp]),
        "gs4d_host_count_centres": (None, [sz, vp, vp, i32, i32, vp, vp]),
        "gs4d_host_measure_records": (None, [sz, vp, vp, vp, vp, vp]),
        "gs4d_host_measure_centre": (i32, [vp, vp]),
        "gs4d_host_transform_selected": (None, [sz, vp, vp, vp, vp, vp]),
        "gs4d_host_count_neighbours": (None, [sz, vp, vp, vp, vp, vp]),
        "gs4d_host_label_components": (None, [sz, vp, vp, vp, vp, vp, vp]),
        "gs4d_host_count_labels": (None, [sz, vp, vp, vp, vp]),
        "gs4d_host_nearest_neighbours": (None, [sz, vp, vp, vp, vp, vp, sz, vp]),
        "gs4d_host_cell_labels": (None, [sz, vp, vp, vp]),
        "gs4d_host_merge_records": (None, [sz, vp, vp, vp, vp, vp, vp, vp, vp, vp]),
        "gs4d_host_merge_rows": (None, [sz, vp, vp, vp, vp, vp, sz, sz, vp]),
        "gs4d_host_lod_cut": (None, [sz, vp, vp, vp, vp, vp, vp, vp, sz]),
        "gs4d_host_frame_box": (None, [vp, vp, vp, f32, i32, i32, vp]),
        "gs4d_host_affine4": (None, [vp, f32, vp, vp, f32, f32, vp]),
        "gs4d_host_scene_linear": (None, [sz, vp, i32, f32, f32, vp, f32, f32, f32, vp]),
        "gs4d_host_scene_nonlinear": (None, [sz, vp, i32, f32, f32, f32, vp, f32, f32, f32, sz, vp]),
        "gs4d_host_scene_rotation": (None, [sz, vp, i32, f32, f32, vp, f32, f32, f32, sz, vp]),
        "gs4d_host_scene_combined": (None, [sz, vp, i32, f32, f32, f32, f32, f32, vp, f32, f32, f32, sz, vp]),
        "gs4d_host_scene_broken": (None, [sz, vp, i32, f32, vp, f32, f32, f32, sz, vp]),
        "gs4d_host_scene_square": (None, [sz, vp, i32, f32, f32, vp, f32, f32, f32, sz, vp]),
        "gs4d_host_parse_vdata": (C.c_long, [C.c_char_p, vp, sz]),
        "gs4d_host_parse_sd": (C.c_long, [C.c_char_p, f32, vp, sz]),
        "gs4d_host_write_png": (i32, [C.c_char_p, vp, i32, i32]),
        "gs4d_version": (C.c_char_p, []),
    }
    for name, (res, args) in sig.items():
        fn = getattr(lib, name)          # AttributeError if the library does not export what gs4d.h declares
        fn.restype, fn.argtypes = res, args
    return lib, tuple(sig)


_lib, EXPORTS = _load()


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


# ---- host-side parameterisation (CPU code in libgs4d.so; Splat.h / Camera.cpp mirror) ---------------
def look_at(eye, orientation, up=(0.0, 1.0, 0.0)):
    out = np.zeros(16, np.float32)
    _lib.gs4d_host_look_at(_ptr(_f32(eye)), _ptr(_f32(orientation)), _ptr(_f32(up)), _ptr(out))
    return out


def perspective(fov_deg, width, height, znear, zfar):
    out = np.zeros(16, np.float32)
    _lib.gs4d_host_perspective(fov_deg, width, height, znear, zfar, _ptr(out))
    return out


def quat_look_at(direction, up=(0.0, 1.0, 0.0)):
    out = np.zeros(4, np.float32)
    _lib.gs4d_host_quat_look_at(_ptr(_f32(direction)), _ptr(_f32(up)), _ptr(out))
    return out


def splat3d_cov(q_wxyz, scale3):
    out = np.zeros(9, np.float32)
    _lib.gs4d_host_splat3d_cov(_ptr(_f32(q_wxyz)), _ptr(_f32(scale3)), _ptr(out))
    return out


def splat4d_cov(q_wxyz, scale3, lifetime, fade, dir3):
    out = np.zeros(16, np.float32)
    _lib.gs4d_host_splat4d_cov(_ptr(_f32(q_wxyz)), _ptr(_f32(scale3)), lifetime, fade, _ptr(_f32(dir3)), _ptr(out))
    return out


def splat4d_cov2q(q0, q1, scale4):
    out = np.zeros(16, np.float32)
    _lib.gs4d_host_splat4d_cov2q(_ptr(_f32(q0)), _ptr(_f32(q1)), _ptr(_f32(scale4)), _ptr(out))
    return out


def build_records_3d(pos3, q_wxyz, scale3, rgba):
    pos3, q, s, col = _f32(pos3).reshape(-1, 3), _f32(q_wxyz).reshape(-1, 4), _f32(scale3).reshape(-1, 3), _f32(rgba).reshape(-1, 4)
    n = pos3.shape[0]
    assert q.shape[0] == n and s.shape[0] == n and col.shape[0] == n
    rec = np.empty((n, 24), np.float32)
    _lib.gs4d_host_build_records_3d(n, _ptr(pos3), _ptr(q), _ptr(s), _ptr(col), _ptr(rec))
    return rec


def build_records_4d(pos4, q_wxyz, scale3, lifetime, fade, dir3, rgba):
    pos4, q, s = _f32(pos4).reshape(-1, 4), _f32(q_wxyz).reshape(-1, 4), _f32(scale3).reshape(-1, 3)
    life, fd, d, col = _f32(lifetime).reshape(-1), _f32(fade).reshape(-1), _f32(dir3).reshape(-1, 3), _f32(rgba).reshape(-1, 4)
    n = pos4.shape[0]
    assert all(x.shape[0] == n for x in (q, s, life, fd, d, col))
    rec = np.empty((n, 24), np.float32)
    _lib.gs4d_host_build_records_4d(n, _ptr(pos4), _ptr(q), _ptr(s), _ptr(life), _ptr(fd), _ptr(d), _ptr(col), _ptr(rec))
    return rec


def time_variance(lifetime, fade):
    """gs4d_host_time_variance: the temporal variance (Sigma44) the reference gives a 4D splat of this lifetime and fade — lifetime^2 /
    (-2 log(fade)), the quotient in double.  Scalars give a float32 scalar, arrays (broadcast against each other) a float32 array."""
    life, fd = np.broadcast_arrays(_f32(lifetime), _f32(fade))
    life, fd = _f32(life).reshape(-1), _f32(fd).reshape(-1)
    out = np.empty(life.shape[0], np.float32)
    _lib.gs4d_host_time_variances(out.shape[0], _ptr(life), _ptr(fd), _ptr(out))
    shape = np.broadcast(np.asarray(lifetime), np.asarray(fade)).shape
    return out.reshape(shape) if shape else out[0]


def build_records_4d_tvar(pos4, q_wxyz, scale3, dir3, tvar, rgba):
    """build_records_4d with the temporal variance given instead of (lifetime, fade): what gs4d_build_records' PARAMS_4D_VEL form computes."""
    pos4, q, s = _f32(pos4).reshape(-1, 4), _f32(q_wxyz).reshape(-1, 4), _f32(scale3).reshape(-1, 3)
    d, tv, col = _f32(dir3).reshape(-1, 3), _f32(tvar).reshape(-1), _f32(rgba).reshape(-1, 4)
    n = pos4.shape[0]
    assert all(x.shape[0] == n for x in (q, s, d, tv, col))
    rec = np.empty((n, 24), np.float32)
    _lib.gs4d_host_build_records_4d_tvar(n, _ptr(pos4), _ptr(q), _ptr(s), _ptr(d), _ptr(tv), _ptr(col), _ptr(rec))
    return rec


def build_records_4d_2q(pos4, q0_wxyz, q1_wxyz, scale4, rgba):
    """Records of 4D splats given by a left and a right quaternion and four scales (splat4d_cov2q per record): PARAMS_4D_2Q."""
    pos4, q0, q1 = _f32(pos4).reshape(-1, 4), _f32(q0_wxyz).reshape(-1, 4), _f32(q1_wxyz).reshape(-1, 4)
    s, col = _f32(scale4).reshape(-1, 4), _f32(rgba).reshape(-1, 4)
    n = pos4.shape[0]
    assert all(x.shape[0] == n for x in (q0, q1, s, col))
    rec = np.empty((n, 24), np.float32)
    _lib.gs4d_host_build_records_4d_2q(n, _ptr(pos4), _ptr(q0), _ptr(q1), _ptr(s), _ptr(col), _ptr(rec))
    return rec


# floats per row of the parameters a record decomposes into, per form, in the order of gs4d_splat_params (PARAMS_4D_2Q is not decomposed)
PARAM_ROWS = {PARAMS_3D: {"pos": 3, "rot": 4, "scale": 3, "rgba": 4}, PARAMS_4D_VEL: {"pos": 4, "rot": 4, "scale": 3, "rgba": 4, "dir": 3, "tvar": 1}}


def _param_names(form, only):
    rows = PARAM_ROWS.get(int(form))
    if rows is None:
        raise ValueError("decompose_records: the form is PARAMS_3D or PARAMS_4D_VEL (a 4D record of any origin can be taken out as PARAMS_4D_VEL)")
    names = tuple(rows) if only is None else tuple(only)
    if not names or set(names) - set(rows):
        raise ValueError(f"decompose_records: `only` names at least one of {tuple(rows)}")
    return rows, names


def decompose_records_host(records, form, only=None):
    """gs4d_host_decompose_records, the definition of Context.decompose_records and the inverse of build_records_3d / build_records_4d_tvar: records
    [n, 24] as a dict {name: float32 [n, k]} of the parameters of the form — PARAMS_3D: pos (3), rot (w x y z), scale (3), rgba; PARAMS_4D_VEL: pos
    (4), rot, scale, rgba, dir (3), tvar (1).  The scales descend, the quaternion is of unit length with w >= 0.  only: the names wanted (all)."""
    rows, names = _param_names(form, only)
    rec = _f32(records).reshape(-1, 24)
    n = rec.shape[0]
    out = {k: np.empty((n, rows[k]), np.float32) for k in names}
    _lib.gs4d_host_decompose_records(n, _ptr(rec), int(form), *(_ptr(out[k]) if k in out else None for k in ("pos", "rot", "scale", "rgba", "dir", "tvar")))
    return out


class Affine4(C.Structure):
    """gs4d_affine4 (include/gs4d.h): one 4D affine map x' = L x + o of gs4d_transform_records — l column-major (L[r, c] = l[4 c + r]), row and
    column 3 = time; 80 bytes."""
    _fields_ = [("l", C.c_float * 16), ("o", C.c_float * 4)]


def affine4(q_wxyz=(1.0, 0.0, 0.0, 0.0), scale=1.0, translate=(0.0, 0.0, 0.0), velocity=(0.0, 0.0, 0.0), time_scale=1.0, time_offset=0.0):
    """gs4d_host_affine4: one row of transform_records' table as 20 float32 (l[16], o[4]) — the upper 3x3 scale * R(q) (the quaternion as given),
    column 3 = velocity, L[3, 3] = time_scale, o = (translate, time_offset).  A source time t shows at time_scale * t + time_offset."""
    out = np.zeros(20, np.float32)
    _lib.gs4d_host_affine4(_ptr(_f32(q_wxyz)), scale, _ptr(_f32(translate)), _ptr(_f32(velocity)), time_scale, time_offset, _ptr(out))
    return out


def _affine_rows(xf):
    """(m, 20) float32 from an Affine4, a sequence of them, or an array of 20 m floats"""
    if isinstance(xf, Affine4):
        xf = [xf]
    if isinstance(xf, (list, tuple)) and xf and isinstance(xf[0], Affine4):
        xf = np.stack([np.frombuffer(bytes(a), np.float32) for a in xf])
    rows = _f32(xf)
    if rows.size % 20:
        raise ValueError("expected rows of 20 float32 (l[16], o[4])")
    return rows.reshape(-1, 20)


def transform_records_host(records, xf):
    """gs4d_host_transform_records, the definition of Context.transform_records: records [n, 24] under xf (20 floats or an Affine4: [n, 24]; m rows:
    [m, n, 24], instance after instance)."""
    rec = _f32(records).reshape(-1, 24)
    single = isinstance(xf, Affine4) or np.ndim(xf) == 1
    rows = _affine_rows(xf)
    out = np.empty((rows.shape[0], rec.shape[0], 24), np.float32)
    for j in range(rows.shape[0]):
        _lib.gs4d_host_transform_records(rec.shape[0], _ptr(rec), _ptr(rows[j]), _ptr(out[j]))
    return out[0] if single else out


def bind_rows(joints, weights):
    """The bind table of pose_records' BLEND4 form as uint32 [n, 8]: per record uint32 j[4], then the bits of float32 w[4].  joints [n, k] and
    weights [n, k] with k <= 4; missing slots are ID_NONE with weight 0 (a slot takes part iff its joint is a row of the table, whatever its weight)."""
    j = np.asarray(joints)
    if j.dtype.kind not in "iu":
        raise TypeError("joints must be integers")
    j, w = np.atleast_2d(j.astype(np.uint32)), np.atleast_2d(_f32(weights))
    if j.shape != w.shape or j.shape[1] > 4:
        raise ValueError("joints and weights must both be [n, k] with k <= 4")
    out = np.empty((j.shape[0], 8), np.uint32)
    out[:, :4], out[:, 4:] = ID_NONE, 0
    out[:, :j.shape[1]] = j
    out[:, 4:4 + j.shape[1]] = w.view(np.uint32)
    return out


def _bind_table(bind, form=None, bind_stride=None):
    """(bytes uint8 [n * stride], form, stride) of a bind array: uint32 [n] is the INDEX form at stride 4, uint32 [n, 8] (bind_rows) the BLEND4 form at
    stride 32; with form / bind_stride given the array is taken as the bytes of rows of that stride"""
    a = np.ascontiguousarray(bind)
    if form is None:
        if a.dtype != np.uint32 or not (a.ndim == 1 or (a.ndim == 2 and a.shape[1] == 8)):
            raise TypeError("expected a uint32 [n] array of row indices or a bind_rows [n, 8] array (or give form and bind_stride)")
        form = POSE_INDEX if a.ndim == 1 else POSE_BLEND4
    if bind_stride is None:
        bind_stride = a.strides[0] if a.ndim == 2 else (4 if form == POSE_INDEX else 32)
    return a.reshape(-1).view(np.uint8), int(form), int(bind_stride)


def pose_records_host(records, xf, bind, form=None, bind_stride=None):
    """gs4d_host_pose_records, the definition of Context.pose_records: records [n, 24] as [n, 24], record i under what row i of `bind` takes from
    the rows of xf ([m, 20] float32; m may be 0) — a uint32 [n] array (INDEX) or a bind_rows array (BLEND4), or with form and bind_stride the bytes
    of rows of that stride.  A form or stride the device call would refuse gives zeros."""
    rec = _f32(records).reshape(-1, 24)
    rows = _f32(xf).reshape(-1, 20)
    table, form, bind_stride = _bind_table(bind, form, bind_stride)
    if table.size < rec.shape[0] * bind_stride:
        raise ValueError("bind holds fewer rows than there are records")
    out = np.zeros_like(rec)
    _lib.gs4d_host_pose_records(rec.shape[0], _ptr(rec), _ptr(rows) if rows.size else None, rows.shape[0], _ptr(table) if table.size else None, form, bind_stride,
                                _ptr(out))
    return out


def sh_rotation(l):
    """gs4d_host_sh_rotation: (ok, d) — the band matrices of gs4d_rotate_sh for the 16 floats of a map's l (a row of 20 floats is taken by its first
    16), float32 [84] with D_1 at 0 (3 x 3), D_2 at 9 (5 x 5), D_3 at 34 (7 x 7), row-major, word 83 = 0; ok is False, d zeros, where the map does
    not rotate."""
    a = _f32(l).reshape(-1)
    if a.size not in (16, 20):
        raise ValueError("expected the 16 floats of l (or a row of 20)")
    a = np.ascontiguousarray(a[:16])
    d = np.zeros(84, np.float32)
    ok = bool(_lib.gs4d_host_sh_rotation(_ptr(a), _ptr(d)))
    return ok, d


def _sh_table(rows, stride=None):
    """(float32 [n, stride / 4], stride) of a table given as float32 [n, words] or uint8 [n, stride] rows, or flat with its stride; a 2-D table
    whose rows are not `stride` bytes wide is refused"""
    a = np.ascontiguousarray(rows)
    if a.dtype == np.uint8:
        if a.shape[-1] % 4:
            raise ValueError("rows of bytes must be a multiple of 4 wide")
        a = a.view(np.float32)
    a = _f32(a)
    if a.ndim != 2:
        if stride is None:
            raise ValueError("a flat table needs its stride")
        a = a.reshape(-1, int(stride) // 4)
    if stride is None:
        stride = a.shape[1] * 4
    if a.shape[1] * 4 != int(stride):
        raise ValueError("the rows are not `stride` bytes wide")
    return a, int(stride)


def rotate_sh_host(rows, xf, degree, bind=None, form=None, bind_stride=None, stride=None):
    """gs4d_host_rotate_sh, the definition of Context.rotate_sh: the table `rows` (float32 [n, stride / 4]) under the maps of xf ([m, 20] float32; m
    may be 0).  bind None: SH_EACH, [m * n, stride / 4] with row j * n + i = row i under map j; else a uint32 [n] array (INDEX) or a bind_rows
    array (BLEND4), or with form and bind_stride the bytes of rows of that stride: [n, stride / 4].  Arguments the device call would refuse give
    zeros."""
    table, stride = _sh_table(rows, stride)
    maps = _f32(xf).reshape(-1, 20)
    n, m = table.shape[0], maps.shape[0]
    if bind is None:
        form = SH_EACH if form is None else form
        bt, bind_stride = None, 0 if bind_stride is None else bind_stride
        out = np.zeros((m * n if form == SH_EACH else n, table.shape[1]), np.float32)
    else:
        bt, form, bind_stride = _bind_table(bind, form, bind_stride)
        if bt.size < n * bind_stride:
            raise ValueError("bind holds fewer rows than the table")
        out = np.zeros_like(table)
    _lib.gs4d_host_rotate_sh(n, _ptr(table) if table.size else None, stride, int(degree), _ptr(maps) if maps.size else None, m,
                             None if bt is None else (_ptr(bt) if bt.size else _ptr(np.zeros(1, np.uint8))), int(form), int(bind_stride), _ptr(out) if out.size else None)
    return out


class Lattice(C.Structure):
    """gs4d_lattice (include/gs4d.h): where node 0 stands, the nodes per unit, the nodes per axis (x, y, z, t) and the clamp bits of a
    gs4d_warp_records call; 64 bytes."""
    _fields_ = [("lo", C.c_float * 4), ("inv", C.c_float * 4), ("dims", C.c_uint32 * 4), ("clamp", C.c_uint32), ("pad", C.c_uint32 * 3)]


def lattice(lo, hi, dims, clamp=""):
    """one gs4d_lattice (Lattice) whose first nodes stand at lo and whose last nodes at hi (4 floats each: x, y, z, t), dims nodes along each axis:
    inv[a] = (dims[a] - 1) / (hi[a] - lo[a]) rounded to float32, 0 for an axis of one node (which takes no part).  clamp: a string over "xyzt",
    the axes along which a centre outside the lattice is moved to its face instead of leaving the record as it is."""
    lo64, hi64 = np.asarray(lo, np.float64).reshape(4), np.asarray(hi, np.float64).reshape(4)
    d = [int(v) for v in dims]
    if len(d) != 4:
        raise ValueError("dims must hold 4 node counts (x, y, z, t)")
    if set(clamp) - set("xyzt"):
        raise ValueError('clamp must be a string over "xyzt"')
    with np.errstate(all="ignore"):                          # (hi == lo gives inf: data like any other, nobody is inside then)
        inv = [(d[a] - 1) / (hi64[a] - lo64[a]) if d[a] >= 2 else 0.0 for a in range(4)]
    bits = sum(1 << "xyzt".index(ch) for ch in set(clamp))
    return Lattice((C.c_float * 4)(*lo64), (C.c_float * 4)(*inv), (C.c_uint32 * 4)(*d), bits, (C.c_uint32 * 3)(0, 0, 0))


def lattice_points(lat):
    """the positions of the nodes of a Lattice as float32 [nt, nz, ny, nx, 4] (the order of the nodes in memory), lo[a] + i / inv[a] along an axis
    of two or more nodes and lo[a] along an axis of one: a displacement field is f(points) - points."""
    axes = []
    for a in range(4):
        i = np.arange(lat.dims[a], dtype=np.float64)
        axes.append(lat.lo[a] + (i / float(lat.inv[a]) if lat.dims[a] >= 2 else 0.0 * i))
    t, z, y, x = np.meshgrid(axes[3], axes[2], axes[1], axes[0], indexing="ij")
    return np.ascontiguousarray(np.stack([x, y, z, t], -1), np.float32)


def _lattice_nodes(nodes, lat):
    """the nodes of a lattice as float32 [count, 4]"""
    count = int(lat.dims[0]) * int(lat.dims[1]) * int(lat.dims[2]) * int(lat.dims[3])
    a = _f32(nodes).reshape(-1, 4)
    if a.shape[0] != count:
        raise ValueError(f"the lattice has {count} nodes, the array {a.shape[0]}")
    return a


def warp_records_host(records, nodes, lat):
    """gs4d_host_warp_records, the definition of Context.warp_records: records [n, 24] as [n, 24], record i through the map of the Lattice `lat`
    whose nodes (dx, dy, dz, dt) are `nodes` ([nt, nz, ny, nx, 4] or anything of that size), linearised at the record's centre; a record whose
    centre is not inside the lattice is copied.  A lattice the device call would refuse gives zeros."""
    rec = _f32(records).reshape(-1, 24)
    a = _f32(nodes).reshape(-1, 4)
    out = np.zeros_like(rec)
    count = int(lat.dims[0]) * int(lat.dims[1]) * int(lat.dims[2]) * int(lat.dims[3])
    if all(1 <= int(d) <= 65535 for d in lat.dims) and count <= 1 << 28 and a.shape[0] != count:      # (a lattice that is refused reads no node)
        raise ValueError(f"the lattice has {count} nodes, the array {a.shape[0]}")
    _lib.gs4d_host_warp_records(rec.shape[0], _ptr(rec), _ptr(a) if a.size else None, C.byref(lat), _ptr(out))
    return out


class ShTime(C.Structure):
    """gs4d_sh_time (include/gs4d.h): the degrees, the time, 1 / period of the cosine series and the camera position of a gs4d_shade_sh_t or
    gs4d_collapse_sh call; 32 bytes."""
    _fields_ = [("degree", C.c_int32), ("degree_t", C.c_int32), ("t", C.c_float), ("inv_period", C.c_float), ("cam_pos", C.c_float * 3),
                ("reserved", C.c_uint32)]


def sh_time_query(degree, degree_t, t, inv_period, cam_pos=(0.0, 0.0, 0.0)):
    """one gs4d_sh_time (ShTime); inv_period is 1 / T of the cosine series (4DGS: 1 / time_duration); cam_pos matters to shade_sh_t only"""
    cam = _f32(cam_pos).reshape(3)
    return ShTime(int(degree), int(degree_t), float(t), float(inv_period), (C.c_float * 3)(*(float(v) for v in cam)), 0)


def _sh_time(q, degree=None, degree_t=None, t=None, inv_period=None, cam_pos=None):
    return q if isinstance(q, ShTime) else sh_time_query(degree, degree_t, t, inv_period, (0.0, 0.0, 0.0) if cam_pos is None else cam_pos)


def sh_time_weights(degree_t, t, inv_period, mu_t):
    """gs4d_host_sh_time_weights: (w float32 [2], mask) for a record whose float 3 is mu_t — w[n - 1] weighs block n = 1 .. degree_t of a 4D SH
    row, bit n - 1 of mask says whether the block takes part (w of one that does not: 0)."""
    q = sh_time_query(0, degree_t, t, inv_period)
    w, mask = np.zeros(2, np.float32), C.c_int(0)
    _lib.gs4d_host_sh_time_weights(C.byref(q), C.c_float(np.float32(mu_t)), _ptr(w), C.byref(mask))
    return w, mask.value


def _sh_table_t(sh, n, sh_stride):
    table = np.ascontiguousarray(sh).view(np.uint8).reshape(-1)
    if table.size < n * sh_stride:
        raise ValueError(f"the table holds fewer than {n} rows of {sh_stride} bytes")
    return table


def collapse_sh_host(records, sh, degree, degree_t, t, inv_period, sh_stride=None, dst_stride=None):
    """gs4d_host_collapse_sh, the definition of Context.collapse_sh: the 4D SH table `sh` (rows of sh_stride bytes, default sh_row_bytes_t(degree,
    degree_t)) of the records [n, 24] collapsed at time t: float32 [n, dst_stride / 4] (default sh_row_bytes(degree)) — the effective row, zeros
    behind it.  Arguments the device call would refuse give zeros."""
    rec = _f32(records).reshape(-1, 24)
    n = rec.shape[0]
    sh_stride = sh_row_bytes_t(degree, degree_t) if sh_stride is None else int(sh_stride)
    dst_stride = sh_row_bytes(degree) if dst_stride is None else int(dst_stride)
    table = _sh_table_t(sh, n, sh_stride)
    out = np.zeros((n, dst_stride // 4), np.float32)
    q = sh_time_query(degree, degree_t, t, inv_period)
    _lib.gs4d_host_collapse_sh(n, _ptr(rec), _ptr(table) if table.size else None, sh_stride, C.byref(q), _ptr(out) if out.size else None, dst_stride)
    return out


def shade_sh_t_host(records, sh, degree, degree_t, t, inv_period, cam_pos, sh_stride=None):
    """gs4d_host_shade_sh_t, the definition of Context.shade_sh_t: a copy of the records [n, 24] with floats 4..6 <- the colour of their rows of the
    4D SH table `sh` at time t, seen from cam_pos.  Arguments the device call would refuse give the records back."""
    rec = _f32(records).reshape(-1, 24).copy()
    n = rec.shape[0]
    sh_stride = sh_row_bytes_t(degree, degree_t) if sh_stride is None else int(sh_stride)
    table = _sh_table_t(sh, n, sh_stride)
    q = sh_time_query(degree, degree_t, t, inv_period, cam_pos)
    _lib.gs4d_host_shade_sh_t(n, _ptr(rec), _ptr(table) if table.size else None, sh_stride, C.byref(q))
    return rec


class Slice(C.Structure):
    """gs4d_slice (include/gs4d.h): the time, the opacity floor and the two time words of a gs4d_slice_records call; 16 bytes."""
    _fields_ = [("t", C.c_float), ("min_opacity", C.c_float), ("mu_t_out", C.c_float), ("s44_out", C.c_float)]


def slice_query(t, min_opacity=0.0, mu_t_out=None, s44_out=1.0):
    """one gs4d_slice (Slice): mu_t_out=None means t — the slice is drawn at the time it was taken at"""
    return Slice(float(t), float(min_opacity), float(t if mu_t_out is None else mu_t_out), float(s44_out))


def slice_records_host(records, t, min_opacity=0.0, mu_t_out=None, s44_out=1.0):
    """gs4d_host_slice_records, the definition of Context.slice_records: records [n, 24] conditioned at time t as [n, 24] — the conditional centre
    and covariance, alpha times the time opacity, mu_t = mu_t_out (None: t), Sigma44 = s44_out and a time row and column of -0.  The query is
    evaluated as it stands, also one the device call would refuse."""
    rec = _f32(records).reshape(-1, 24)
    out = np.empty_like(rec)
    q = slice_query(t, min_opacity, mu_t_out, s44_out)
    _lib.gs4d_host_slice_records(rec.shape[0], _ptr(rec), C.byref(q), _ptr(out))
    return out


# gs4d_colour_edit and gs4d_keep_rule (include/gs4d.h) as numpy records
COLOUR_EDIT = np.dtype([("op", "<u4"), ("channels", "<u4"), ("value", "<f4", (4,)), ("amount", "<f4"), ("reserved", "<u4")])
KEEP_RULE = np.dtype([("min_pixels", "<u4"), ("min_wmax", "<u4"), ("min_wsum", "<u8"), ("flags", "<u4"), ("reserved", "<u4")])
RECORD_STAT = np.dtype([("pixels", "<u4"), ("wmax", "<f4"), ("wsum", "<u8")])
EDIT_OPS = {"set": EDIT_SET, "mul": EDIT_MUL, "lerp": EDIT_LERP, "copy": EDIT_COPY}
_CHANNEL_BITS = {"r": 1, "g": 2, "b": 4, "a": 8}


def _keep_rule(min_pixels=1, min_wmax=0.0, min_wsum=0, invert=False):
    """one gs4d_keep_rule from compact_records' keywords: min_wmax is a weight (float32), min_wsum is in units of 2^-24"""
    rule = np.zeros(1, KEEP_RULE)
    rule["min_pixels"], rule["min_wmax"], rule["min_wsum"] = int(min_pixels), np.array([min_wmax], np.float32).view(np.uint32)[0], int(min_wsum)
    rule["flags"] = KEEP_INVERT if invert else 0
    return rule


def colour_edit(op, value=(0.0, 0.0, 0.0, 0.0), channels="rgb", amount=0.0):
    """one gs4d_colour_edit (COLOUR_EDIT): op "set" / "mul" / "lerp" / "copy" or an EDIT_* constant; channels a string over "rgba" or the mask 1 .. 15
    (1 r, 2 g, 4 b, 8 a); value: up to four operands, r first."""
    e = np.zeros(1, COLOUR_EDIT)
    e["op"] = EDIT_OPS[op] if isinstance(op, str) else int(op)
    if isinstance(channels, str):
        mask = 0
        for ch in channels:
            mask |= _CHANNEL_BITS[ch]
        channels = mask
    e["channels"] = int(channels)
    v = _f32(value).ravel()
    e["value"][0, :v.size] = v[:4]
    e["amount"] = np.float32(amount)
    return e


def edit_colours_host(records, op, value=(0.0, 0.0, 0.0, 0.0), channels="rgb", amount=0.0, stats=None, from_=None, **rule):
    """gs4d_host_edit_colours, the definition of Context.edit_colours: a copy of records [n, 24] with the rgba of the selected records edited.
    stats: a RECORD_STAT array of n rows (the rule keywords of compact_records select by it) or None: every record; from_: [n, 24], for "copy"."""
    rec = np.array(_f32(records).reshape(-1, 24), copy=True)
    n = rec.shape[0]
    e = colour_edit(op, value, channels, amount)
    if stats is None and rule:
        raise TypeError("edit_colours_host: a rule without stats")
    st = None if stats is None else np.ascontiguousarray(stats, RECORD_STAT)
    if st is not None and st.shape[0] < n:
        raise ValueError("edit_colours_host: stats holds fewer than n rows")
    fr = None if from_ is None else _f32(from_).reshape(-1, 24)
    if int(e["op"][0]) == EDIT_COPY and (fr is None or fr.shape[0] < n):
        raise ValueError("edit_colours_host: copy needs n records in from_")
    k = _keep_rule(**rule)
    _lib.gs4d_host_edit_colours(n, _ptr(rec), _ptr(st) if st is not None else None, _ptr(k) if st is not None else None, _ptr(e), _ptr(fr) if fr is not None else None)
    return rec


def scene_linear(verts6, steps=50, time_multiplier=1.0, object_scale=5.0, splat_scale=(4.0, 4.0, 1.0), lifetime=1.0, fade=0.5, speed=1.0):
    """LinearMotion::init records (Scenes.h:258-279) with the class defaults (Scenes.h:186-201)."""
    v = _f32(verts6).reshape(-1, 6)
    rec = np.empty((v.shape[0] * steps, 24), np.float32)
    _lib.gs4d_host_scene_linear(v.shape[0], _ptr(v), steps, time_multiplier, object_scale, _ptr(_f32(splat_scale)), lifetime, fade, speed, _ptr(rec))
    return rec


def scene_nonlinear(verts6, steps=92, angle_multiplier=4.0, radius=20.0, object_scale=5.0, splat_scale=(4.0, 4.0, 1.0), lifetime=1.0, fade=0.5, speed=20.0,
                    max_records=None):
    """NonLinearMotion::init records (Scenes.h:517-545) with the class defaults (Scenes.h:451-467)."""
    v = _f32(verts6).reshape(-1, 6)
    n = v.shape[0] * steps if max_records is None else min(max_records, v.shape[0] * steps)
    rec = np.empty((n, 24), np.float32)
    _lib.gs4d_host_scene_nonlinear(v.shape[0], _ptr(v), steps, angle_multiplier, radius, object_scale, _ptr(_f32(splat_scale)), lifetime, fade, speed, n, _ptr(rec))
    return rec


def _scene_out(verts6, steps, max_records):
    v = _f32(verts6).reshape(-1, 6)
    n = v.shape[0] * steps if max_records is None else min(max_records, v.shape[0] * steps)
    return v, n, np.empty((n, 24), np.float32)


def scene_rotation(verts6, steps=92, angle_multiplier=4.0, object_scale=5.0, splat_scale=(4.0, 4.0, 1.0), lifetime=0.6, fade=0.5, speed=5.0, max_records=None):
    """RotationMotion::init records (Scenes.h:775-803) with the class defaults (Scenes.h:711-727).  Camera (0,60,30) / (0,-1,-0.5)."""
    v, n, rec = _scene_out(verts6, steps, max_records)
    _lib.gs4d_host_scene_rotation(v.shape[0], _ptr(v), steps, angle_multiplier, object_scale, _ptr(_f32(splat_scale)), lifetime, fade, speed, n, _ptr(rec))
    return rec


def scene_combined(verts6, steps=65, angle_multiplier=8.0, lin_multiplier=8.0, amplitude=1.0, frequency=0.15, object_scale=5.0, splat_scale=(4.0, 4.0, 0.0),
                   lifetime=1.0, fade=0.5, speed=1.0, max_records=None):
    """CombinedMotion::init records (Scenes.h:1035-1068) with the class defaults (Scenes.h:959-976).  Camera (50,90,90) / (0,-1,-1)."""
    v, n, rec = _scene_out(verts6, steps, max_records)
    _lib.gs4d_host_scene_combined(v.shape[0], _ptr(v), steps, angle_multiplier, lin_multiplier, amplitude, frequency, object_scale, _ptr(_f32(splat_scale)),
                                  lifetime, fade, speed, n, _ptr(rec))
    return rec


def scene_broken(verts6, steps=92, object_scale=5.0, splat_scale=(4.0, 4.0, 1.0), lifetime=1.0, fade=0.5, speed=1.0, max_records=None):
    """BrokenMotion::init records (Scenes.h:1965-1989) with the class defaults (Scenes.h:1899-1912).  Camera (0,60,60) / (0,-1,-1)."""
    v, n, rec = _scene_out(verts6, steps, max_records)
    _lib.gs4d_host_scene_broken(v.shape[0], _ptr(v), steps, object_scale, _ptr(_f32(splat_scale)), lifetime, fade, speed, n, _ptr(rec))
    return rec


def scene_square(verts6, steps=92, square_size=40.0, object_scale=5.0, splat_scale=(4.0, 4.0, 1.0), lifetime=1.0, fade=0.5, speed=1.0, max_records=None):
    """SquareMotion::init records (Scenes.h:2216-2259) with the class defaults (Scenes.h:2151-2165).  Camera (0,60,60) / (0,-1,-1)."""
    v, n, rec = _scene_out(verts6, steps, max_records)
    _lib.gs4d_host_scene_square(v.shape[0], _ptr(v), steps, square_size, object_scale, _ptr(_f32(splat_scale)), lifetime, fade, speed, n, _ptr(rec))
    return rec


def parse_vdata(path, cap_vertices=1 << 20):
    buf = np.empty((cap_vertices, 6), np.float32)
    n = _lib.gs4d_host_parse_vdata(os.fsencode(path), _ptr(buf), cap_vertices)
    if n < 0:
        raise FileNotFoundError(path)
    return buf[:min(n, cap_vertices)].copy()


def splat3d_mesh(pos3, q_wxyz, scale3, color4):
    """Splat3D::GetSplatMesh (Splat.h:433-447): (4, 18) float32 = four 72-byte vertices {corner, position, colour, Sigma3}."""
    out = np.empty((4, 18), np.float32)
    _lib.gs4d_host_splat3d_mesh(_ptr(_f32(pos3)), _ptr(_f32(q_wxyz)), _ptr(_f32(scale3)), _ptr(_f32(color4)), _ptr(out))
    return out


def splat2d_sigma_inv(v0, l0, l1):
    """Splat2D::CalcAndSetSigma (Splat.h:576-582): inverse 2x2 covariance, column-major."""
    out = np.empty(4, np.float32)
    _lib.gs4d_host_splat2d_sigma_inv(_ptr(_f32(v0)), l0, l1, _ptr(out))
    return out


def gaussians2d_record(angle, s0, s1, px, py, rgb):
    """One 48-byte record of the Gaussians2D scene (Scenes.h:1490-1496) for GS4D_MODE_2D."""
    out = np.empty(12, np.float32)
    _lib.gs4d_host_gaussians2d_record(angle, s0, s1, px, py, _ptr(_f32(rgb)), _ptr(out))
    return out


def parse_sd(path, object_scale=1.0, cap_records=1 << 22):
    """`.sd` splat file -> (n, 24) records (VDataParser.h:60-123 + ObjectDisplay::init, Scenes.h:2483-2491; its object scale defaults to 1)."""
    buf = np.empty((cap_records, 24), np.float32)
    n = _lib.gs4d_host_parse_sd(os.fsencode(path), object_scale, _ptr(buf), cap_records)
    if n < 0:
        raise FileNotFoundError(path)
    return buf[:min(n, cap_records)].copy()


class CameraState(C.Structure):
    """gs4d_camera_state (include/gs4d.h): the Camera of Camera.h:16-85 as plain data."""
    _fields_ = [("position", C.c_float * 3), ("orientation", C.c_float * 3), ("up", C.c_float * 3), ("width", C.c_int), ("height", C.c_int),
                ("sensitivity", C.c_float), ("speed", C.c_float), ("fast_speed", C.c_float),
                ("capture_mouse", C.c_int), ("first_capture", C.c_int), ("fix_view", C.c_int), ("fix_position", C.c_int), ("lock_x", C.c_int), ("lock_y", C.c_int)]

    @classmethod
    def make(cls, width, height, position, orientation, up=(0.0, 1.0, 0.0)):
        st = cls()
        st.position[:], st.orientation[:], st.up[:] = position, orientation, up
        st.width, st.height = width, height
        st.sensitivity, st.speed, st.fast_speed = 100.0, 0.5, 2.0          # Camera.h:78-80
        st.first_capture = 1
        return st


class IdRegion(C.Structure):
    """gs4d_id_region (include/gs4d.h): the rectangle, the draws and the least weight of a gs4d_count_ids call."""
    _fields_ = [("x", C.c_int32), ("y", C.c_int32), ("w", C.c_int32), ("h", C.c_int32), ("draw_first", C.c_uint32), ("draw_last", C.c_uint32),
                ("min_weight", C.c_uint32), ("reserved", C.c_uint32)]


class CentreQuery(C.Structure):
    """gs4d_centre_query (include/gs4d.h): the tests, the op and the operands of a gs4d_count_centres call."""
    _fields_ = [("tests", C.c_uint32), ("op", C.c_uint32), ("t", C.c_float), ("reserved", C.c_uint32), ("frame", C.c_float * 12),
                ("box_lo", C.c_float * 3), ("box_hi", C.c_float * 3), ("sphere", C.c_float * 4), ("view", C.c_float * 16), ("proj", C.c_float * 16),
                ("x", C.c_int32), ("y", C.c_int32), ("w", C.c_int32), ("h", C.c_int32), ("depth_min", C.c_float), ("depth_max", C.c_float)]


def centre_query(box=None, sphere=None, frame=None, screen=None, rect=None, depth=(0.0, float("inf")), t=0.0, skip_hidden=False, skip_dead=False,
                 remove=False):
    """one gs4d_centre_query (CentreQuery).  box=(lo, hi): the centre inside the closed box; sphere=(c, r): inside the closed ball; frame: a 3x4
    world -> volume-frame map, 12 floats column-major (or a [3, 4] array given as rows), applied before box and sphere; screen=(view, proj): the
    centre projects into rect=(x, y, w, h) (y from the bottom row; required with screen) at a view depth inside depth=(min, max); t: the time the
    centre is taken at; skip_hidden / skip_dead: leave out records of alpha <= 0 / dead at t; remove: zero the rows instead of adding to them."""
    q = CentreQuery()
    q.t = float(t)
    q.op = CQ_REMOVE if remove else CQ_ADD
    tests = (CQ_SKIP_HIDDEN if skip_hidden else 0) | (CQ_SKIP_DEAD if skip_dead else 0)
    if box is not None:
        tests |= CQ_BOX
        q.box_lo[:], q.box_hi[:] = [float(v) for v in _f32(box[0]).ravel()[:3]], [float(v) for v in _f32(box[1]).ravel()[:3]]
    if sphere is not None:
        tests |= CQ_SPHERE
        q.sphere[:] = [float(v) for v in _f32(sphere[0]).ravel()[:3]] + [float(np.float32(sphere[1]))]
    if frame is not None:
        tests |= CQ_FRAME
        f = _f32(frame)
        q.frame[:] = [float(v) for v in (f.T.ravel() if f.shape == (3, 4) else f.ravel())]
    if screen is not None:
        if rect is None:
            raise TypeError("centre_query: screen needs rect")
        tests |= CQ_SCREEN
        q.view[:], q.proj[:] = [float(v) for v in _f32(screen[0]).ravel()], [float(v) for v in _f32(screen[1]).ravel()]
        q.x, q.y, q.w, q.h = (int(v) for v in rect)
        q.depth_min, q.depth_max = float(np.float32(depth[0])), float(np.float32(depth[1]))
    elif rect is not None:
        raise TypeError("centre_query: rect without screen")
    q.tests = tests
    return q


def count_centres_host(records, query, width, height, mask=None, stats=None):
    """gs4d_host_count_centres, the definition of Context.count_centres: the RECORD_STAT table (a copy of `stats`, rows of 16 bytes, or n zeroed rows
    if None) after the query (centre_query) on records [n, 24] for a width x height image; mask: an (h, w) bool / uint8 array, rows bottom-up, or None."""
    rec = _f32(records).reshape(-1, 24)
    n = rec.shape[0]
    st = np.zeros(n, RECORD_STAT) if stats is None else np.array(np.ascontiguousarray(stats), copy=True)
    if st.dtype.itemsize != 16 or st.ndim != 1 or st.shape[0] < n:
        raise ValueError("count_centres_host: stats must be at least n rows of 16 bytes")
    st = st.view(RECORD_STAT)                                  # (the bytes as they are: a table whose wmax is kept as its bit pattern is not converted)
    m = None
    if mask is not None:
        m = np.ascontiguousarray(np.asarray(mask) != 0, np.uint8)
        if m.shape != (query.h, query.w):
            raise ValueError(f"count_centres_host: expected a mask of shape {(query.h, query.w)}, got {m.shape}")
    _lib.gs4d_host_count_centres(n, _ptr(rec), C.byref(query), int(width), int(height), _ptr(m) if m is not None else None, _ptr(st))
    return st


class MeasureQuery(C.Structure):
    """gs4d_measure_query (include/gs4d.h): the time and the skips of a gs4d_measure_records call."""
    _fields_ = [("t", C.c_float), ("flags", C.c_uint32), ("reserved", C.c_uint32 * 2)]


class Measure(C.Structure):
    """gs4d_measure (include/gs4d.h): the 96 bytes a gs4d_measure_records call writes."""
    _fields_ = [("count", C.c_uint32), ("unplaced", C.c_uint32), ("skipped", C.c_uint32), ("reserved0", C.c_uint32),
                ("lo", C.c_float * 3), ("hi", C.c_float * 3), ("ext_lo", C.c_float * 3), ("ext_hi", C.c_float * 3),
                ("cell_sum", C.c_uint64 * 3), ("reserved1", C.c_uint64)]

    def as_dict(self):
        """count, unplaced, skipped, lo, hi, ext_lo, ext_hi (float32 [3]), cell_sum (uint64 [3]) and centre (gs4d_host_measure_centre: float32
        [3], or None when nothing was measured)"""
        centre = np.zeros(3, np.float32)
        has = _lib.gs4d_host_measure_centre(C.byref(self), _ptr(centre))
        out = {k: int(getattr(self, k)) for k in ("count", "unplaced", "skipped")}
        out.update({k: np.array(getattr(self, k)[:], np.float32) for k in ("lo", "hi", "ext_lo", "ext_hi")})
        out["cell_sum"] = np.array(self.cell_sum[:], np.uint64)
        out["centre"] = centre if has else None
        return out


def measure_query(t=0.0, skip_hidden=False, skip_dead=False):
    """one gs4d_measure_query (MeasureQuery)"""
    q = MeasureQuery()
    q.t, q.flags = float(t), (MS_SKIP_HIDDEN if skip_hidden else 0) | (MS_SKIP_DEAD if skip_dead else 0)
    return q


def measure_records_host(records, t=0.0, stats=None, skip_hidden=False, skip_dead=False, query=None, **rule):
    """gs4d_host_measure_records, the definition of Context.measure_records: the Measure of records [n, 24] at time t.  stats: a RECORD_STAT array
    of n rows (the rule keywords of compact_records select by it) or None: every record; query: a MeasureQuery instead of t and the skips."""
    rec = _f32(records).reshape(-1, 24)
    n = rec.shape[0]
    if stats is None and rule:
        raise TypeError("measure_records_host: a rule without stats")
    st = None if stats is None else np.ascontiguousarray(stats)
    if st is not None and (st.dtype.itemsize != 16 or st.ndim != 1 or st.shape[0] < n):
        raise ValueError("measure_records_host: stats must be at least n rows of 16 bytes")
    q = measure_query(t, skip_hidden, skip_dead) if query is None else query
    k = _keep_rule(**rule)
    out = Measure()
    _lib.gs4d_host_measure_records(n, _ptr(rec), C.byref(q), _ptr(st) if st is not None else None, _ptr(k) if st is not None else None, C.byref(out))
    return out


class SelectionXf(C.Structure):
    """gs4d_selection_xf (include/gs4d.h): the map, the pivot and the pivot flag of a gs4d_transform_selected call; 96 bytes."""
    _fields_ = [("xf", Affine4), ("pivot", C.c_float * 3), ("flags", C.c_uint32)]


def selection_xf(xf, pivot=None, measure=False):
    """one gs4d_selection_xf (SelectionXf): xf 20 float32 (affine4) or an Affine4; pivot: a 3-tuple, the point the map is applied about
    (XS_PIVOT); measure=True: the pivot is the centre of a Measure the call is given (XS_PIVOT_MEASURE).  Passing both is an error."""
    if pivot is not None and measure:
        raise TypeError("selection_xf: pivot and measure exclude each other")
    rows = _affine_rows(xf)
    if rows.shape[0] != 1:
        raise ValueError("selection_xf: expected one row of 20 float32 (l[16], o[4])")
    x = SelectionXf()
    x.xf = Affine4.from_buffer_copy(rows[0].tobytes())
    if pivot is not None:
        c = _f32(pivot).ravel()
        if c.size != 3:
            raise ValueError("selection_xf: pivot is a 3-tuple")
        # (the bits as they are: a float32 NaN keeps its payload)
        C.memmove(C.addressof(x) + SelectionXf.pivot.offset, _ptr(c), 12)
        x.flags = XS_PIVOT
    elif measure:
        x.flags = XS_PIVOT_MEASURE
    return x


def transform_selected_host(records, xf, stats=None, pivot=None, measure=None, n=None, **rule):
    """gs4d_host_transform_selected, the definition of Context.transform_selected: a copy of records [total, 24] with the selected ones of the
    first n (default: all) moved under xf (20 float32, an Affine4, or a SelectionXf, which then carries pivot and flag itself) about the pivot.
    stats: a RECORD_STAT array of n rows (the rule keywords of compact_records select by it) or None: every record; pivot: a 3-tuple;
    measure: a Measure, whose centre is the pivot.  Passing both is an error."""
    rec = np.array(_f32(records).reshape(-1, 24), copy=True)
    n = rec.shape[0] if n is None else int(n)
    if n > rec.shape[0]:
        raise ValueError("transform_selected_host: fewer than n records")
    if stats is None and rule:
        raise TypeError("transform_selected_host: a rule without stats")
    st = None if stats is None else np.ascontiguousarray(stats)
    if st is not None and (st.dtype.itemsize != 16 or st.ndim != 1 or st.shape[0] < n):
        raise ValueError("transform_selected_host: stats must be at least n rows of 16 bytes")
    if isinstance(xf, SelectionXf):
        if pivot is not None:
            raise TypeError("transform_selected_host: a SelectionXf carries its own pivot")
        x = xf
    else:
        x = selection_xf(xf, pivot, measure is not None)
    if x.flags == XS_PIVOT_MEASURE and measure is None:
        raise TypeError("transform_selected_host: XS_PIVOT_MEASURE needs measure")
    k = _keep_rule(**rule)
    _lib.gs4d_host_transform_selected(n, _ptr(rec), _ptr(st) if st is not None else None, _ptr(k) if st is not None else None, C.byref(x),
                                      C.byref(measure) if measure is not None else None)
    return rec


class NeighbourQuery(C.Structure):
    """gs4d_neighbour_query (include/gs4d.h): the time, the radius, the cap and the flags of a gs4d_count_neighbours call; 32 bytes."""
    _fields_ = [("t", C.c_float), ("radius", C.c_float), ("cap", C.c_uint32), ("flags", C.c_uint32), ("reserved", C.c_uint32 * 4)]


def neighbour_query(radius, t=0.0, cap=0xFFFFFFFF, skip_hidden=False, skip_dead=False, count_self=False):
    """one gs4d_neighbour_query (NeighbourQuery): centres at time t, within `radius` (float32; 2^-63 <= radius < 2^64), the count saturating at
    cap >= 1; skip_hidden / skip_dead: records of alpha <= 0 / dead at t take no part; count_self: a record that is a source counts itself."""
    q = NeighbourQuery()
    q.t, q.radius, q.cap = float(t), float(np.float32(radius)), int(cap)
    q.flags = (NB_SKIP_HIDDEN if skip_hidden else 0) | (NB_SKIP_DEAD if skip_dead else 0) | (NB_COUNT_SELF if count_self else 0)
    return q


def count_neighbours_host(records, radius=None, t=0.0, cap=0xFFFFFFFF, source=None, skip_hidden=False, skip_dead=False, count_self=False, query=None,
                          stats=None, **rule):
    """gs4d_host_count_neighbours, the definition of Context.count_neighbours — the brute-force double loop: the RECORD_STAT table (a copy of
    `stats`, rows of 16 bytes, or n zeroed rows if None) after the call on records [n, 24].  source: a table of n rows of 16 bytes whose row j
    makes record j a source by compact_records' rule keywords, or None: every record (and no rule); query: a NeighbourQuery instead of the
    radius and the other keywords."""
    rec = _f32(records).reshape(-1, 24)
    n = rec.shape[0]
    if source is None and rule:
        raise TypeError("count_neighbours_host: a rule without source")
    if query is None:
        if radius is None:
            raise TypeError("count_neighbours_host: radius or query is needed")
        query = neighbour_query(radius, t, cap, skip_hidden, skip_dead, count_self)
    st = np.zeros(n, RECORD_STAT) if stats is None else np.array(np.ascontiguousarray(stats), copy=True)
    if st.dtype.itemsize != 16 or st.ndim != 1 or st.shape[0] < n:
        raise ValueError("count_neighbours_host: stats must be at least n rows of 16 bytes")
    st = st.view(RECORD_STAT)                                  # (the bytes as they are, as in count_centres_host)
    src = None if source is None else np.ascontiguousarray(source)
    if src is not None and (src.dtype.itemsize != 16 or src.ndim != 1 or src.shape[0] < n):
        raise ValueError("count_neighbours_host: source must be at least n rows of 16 bytes")
    k = _keep_rule(**rule)
    _lib.gs4d_host_count_neighbours(n, _ptr(rec), C.byref(query), _ptr(src) if src is not None else None, _ptr(k) if src is not None else None, _ptr(st))
    return st


class ComponentQuery(C.Structure):
    """gs4d_component_query (include/gs4d.h): the time, the radius, the cap and the flags of a gs4d_label_components call; 32 bytes."""
    _fields_ = [("t", C.c_float), ("radius", C.c_float), ("cap", C.c_uint32), ("flags", C.c_uint32), ("reserved", C.c_uint32 * 4)]


def component_query(radius, t=0.0, cap=0xFFFFFFFF, skip_hidden=False, skip_dead=False):
    """one gs4d_component_query (ComponentQuery): centres at time t, members linked iff within `radius` (float32; 2^-63 <= radius < 2^64), the
    size written to a row saturating at cap >= 1; skip_hidden / skip_dead: records of alpha <= 0 / dead at t are no members."""
    q = ComponentQuery()
    q.t, q.radius, q.cap = float(t), float(np.float32(radius)), int(cap)
    q.flags = (CC_SKIP_HIDDEN if skip_hidden else 0) | (CC_SKIP_DEAD if skip_dead else 0)
    return q


def label_components_host(records, radius=None, t=0.0, cap=0xFFFFFFFF, source=None, skip_hidden=False, skip_dead=False, query=None, stats=None,
                          with_stats=True, **rule):
    """gs4d_host_label_components, the definition of Context.label_components — the brute-force double loop with a sequential union-find: (labels
    [n] uint32, the RECORD_STAT table after the call — a copy of `stats`, or n zeroed rows if None; None with with_stats=False) on records [n, 24].
    source: a table of n rows of 16 bytes whose row i makes record i a candidate member by compact_records' rule keywords, or None: every record
    (and no rule); query: a ComponentQuery instead of the radius and the other keywords.  A query the device would refuse leaves the labels at
    ID_NONE and the table as it was."""
    rec = _f32(records).reshape(-1, 24)
    n = rec.shape[0]
    if source is None and rule:
        raise TypeError("label_components_host: a rule without source")
    if query is None:
        if radius is None:
            raise TypeError("label_components_host: radius or query is needed")
        query = component_query(radius, t, cap, skip_hidden, skip_dead)
    st = None
    if with_stats:
        st = np.zeros(n, RECORD_STAT) if stats is None else np.array(np.ascontiguousarray(stats), copy=True)
        if st.dtype.itemsize != 16 or st.ndim != 1 or st.shape[0] < n:
            raise ValueError("label_components_host: stats must be at least n rows of 16 bytes")
        st = st.view(RECORD_STAT)
    src = None if source is None else np.ascontiguousarray(source)
    if src is not None and (src.dtype.itemsize != 16 or src.ndim != 1 or src.shape[0] < n):
        raise ValueError("label_components_host: source must be at least n rows of 16 bytes")
    k = _keep_rule(**rule)
    labels = np.full(n, ID_NONE, np.uint32)
    _lib.gs4d_host_label_components(n, _ptr(rec), C.byref(query), _ptr(src) if src is not None else None, _ptr(k) if src is not None else None,
                                    _ptr(labels), _ptr(st) if st is not None else None)
    return labels, st


def count_labels_host(labels, seeds, stats=None, n=None, **rule):
    """gs4d_host_count_labels, the definition of Context.count_labels: the RECORD_STAT table (a copy of `stats`, or n zeroed rows if None) after
    the call — one fragment of weight 1 for every record < n whose label is the label of a record whose row of `seeds` (n rows of 16 bytes)
    passes compact_records' rule keywords.  n: default all of `labels`."""
    lab = np.ascontiguousarray(labels, np.uint32).ravel()
    n = lab.shape[0] if n is None else int(n)
    sd = np.ascontiguousarray(seeds)
    if lab.shape[0] < n or sd.dtype.itemsize != 16 or sd.ndim != 1 or sd.shape[0] < n:
        raise ValueError("count_labels_host: labels must be at least n words and seeds at least n rows of 16 bytes")
    st = np.zeros(n, RECORD_STAT) if stats is None else np.array(np.ascontiguousarray(stats), copy=True)
    if st.dtype.itemsize != 16 or st.ndim != 1 or st.shape[0] < n:
        raise ValueError("count_labels_host: stats must be at least n rows of 16 bytes")
    st = st.view(RECORD_STAT)
    k = _keep_rule(**rule)
    _lib.gs4d_host_count_labels(n, _ptr(lab), _ptr(sd), _ptr(k), _ptr(st))
    return st


class NearestQuery(C.Structure):
    """gs4d_nearest_query (include/gs4d.h): the time, the radius, k and the flags of a gs4d_nearest_neighbours call; 32 bytes."""
    _fields_ = [("t", C.c_float), ("radius", C.c_float), ("k", C.c_uint32), ("flags", C.c_uint32), ("reserved", C.c_uint32 * 4)]


HIT = np.dtype([("record", "<u4"), ("dist2", "<f4")])      # gs4d_neighbour_hit; an empty slot is {ID_NONE, +inf}


def nearest_query(radius, k, t=0.0, skip_hidden=False, skip_dead=False, include_self=False):
    """one gs4d_nearest_query (NearestQuery): centres at time t, the k (1 .. 16) nearest sources within `radius` (float32; 2^-63 <= radius <
    2^64); skip_hidden / skip_dead: records of alpha <= 0 / dead at t take no part; include_self: a record that is a source is its own hit."""
    q = NearestQuery()
    q.t, q.radius, q.k = float(t), float(np.float32(radius)), int(k)
    q.flags = (NN_SKIP_HIDDEN if skip_hidden else 0) | (NN_SKIP_DEAD if skip_dead else 0) | (NN_INCLUDE_SELF if include_self else 0)
    return q


def hit_stride_for(k):
    """the smallest hit_stride that holds k hits: 8 k bytes rounded up to a multiple of 16"""
    return 16 * ((8 * int(k) + 15) // 16)


def nearest_neighbours_host(records, radius=None, k=3, t=0.0, source=None, skip_hidden=False, skip_dead=False, include_self=False, hits=None,
                            hit_stride=None, stats=None, with_stats=True, query=None, **rule):
    """gs4d_host_nearest_neighbours, the definition of Context.nearest_neighbours — the brute-force double loop: (the hit table as uint8
    [n, hit_stride] — a copy of `hits`, or zeroed bytes if None; row[:8 k].view(HIT) are the slots — and the RECORD_STAT table after the call — a
    copy of `stats`, or n zeroed rows if None; None with with_stats=False) on records [n, 24].  hit_stride: default hit_stride_for(k).  source: a
    table of n rows of 16 bytes whose row j makes record j a source by compact_records' rule keywords, or None: every record (and no rule); query:
    a NearestQuery instead of the radius, k and the other keywords.  A call the device would refuse leaves both tables as they were."""
    rec = _f32(records).reshape(-1, 24)
    n = rec.shape[0]
    if source is None and rule:
        raise TypeError("nearest_neighbours_host: a rule without source")
    if query is None:
        if radius is None:
            raise TypeError("nearest_neighbours_host: radius or query is needed")
        query = nearest_query(radius, k, t, skip_hidden, skip_dead, include_self)
    if hit_stride is None:
        hit_stride = hit_stride_for(query.k)
    hit_stride = int(hit_stride)
    ht = np.zeros((n, max(hit_stride, 1)), np.uint8) if hits is None else np.array(np.ascontiguousarray(hits).view(np.uint8).reshape(n, -1), copy=True)
    if ht.shape[1] != max(hit_stride, 1):
        raise ValueError("nearest_neighbours_host: hits must be n rows of hit_stride bytes")
    st = None
    if with_stats:
        st = np.zeros(n, RECORD_STAT) if stats is None else np.array(np.ascontiguousarray(stats), copy=True)
        if st.dtype.itemsize != 16 or st.ndim != 1 or st.shape[0] < n:
            raise ValueError("nearest_neighbours_host: stats must be at least n rows of 16 bytes")
        st = st.view(RECORD_STAT)
    src = None if source is None else np.ascontiguousarray(source)
    if src is not None and (src.dtype.itemsize != 16 or src.ndim != 1 or src.shape[0] < n):
        raise ValueError("nearest_neighbours_host: source must be at least n rows of 16 bytes")
    kr = _keep_rule(**rule)
    _lib.gs4d_host_nearest_neighbours(n, _ptr(rec), C.byref(query), _ptr(src) if src is not None else None, _ptr(kr) if src is not None else None,
                                      _ptr(ht), hit_stride, _ptr(st) if st is not None else None)
    return ht, st


class CellGrid(C.Structure):
    """gs4d_cell_grid (include/gs4d.h): the low corner, the cell edges and the cell counts of a gs4d_cell_labels call along x, y, z, t; 64 bytes."""
    _fields_ = [("lo", C.c_float * 4), ("edge", C.c_float * 4), ("dims", C.c_uint32 * 4), ("reserved", C.c_uint32 * 4)]


class MergeQuery(C.Structure):
    """gs4d_merge_query (include/gs4d.h): the alpha clamp of a gs4d_merge_records call; 16 bytes."""
    _fields_ = [("alpha_max", C.c_float), ("flags", C.c_uint32), ("reserved", C.c_uint32 * 2)]


MERGE_GROUP = np.dtype([("label", "<u4"), ("size", "<u4"), ("first", "<u4"), ("reserved", "<u4")])          # gs4d_merge_group
MERGE_COUNT = np.dtype([("groups", "<u4"), ("written", "<u4"), ("members", "<u4"), ("left_out", "<u4")])   # gs4d_merge_count


def cell_grid(lo, edge, dims):
    """one gs4d_cell_grid (CellGrid): lo, edge and dims of up to four entries (x, y, z, t); a missing axis gets lo 0, edge 1 and ONE cell, so three
    entries give the grid of a static or sliced set.  edge may be one number for every axis given."""
    lo = [float(v) for v in np.atleast_1d(lo)]
    dims = [int(v) for v in np.atleast_1d(dims)]
    edge = [float(v) for v in np.atleast_1d(edge)]
    if len(edge) == 1:
        edge = edge * len(dims)
    if not (len(lo) == len(edge) == len(dims) <= 4):
        raise ValueError("cell_grid: lo, edge and dims must have the same number of entries, at most 4")
    g = CellGrid()
    for a in range(4):
        g.lo[a], g.edge[a], g.dims[a] = (lo[a], edge[a], dims[a]) if a < len(dims) else (0.0, 1.0, 1)
    return g


def cell_labels_host(records, grid):
    """gs4d_host_cell_labels, the definition of Context.cell_labels: uint32 [n], the cell of every record of records [n, 24] in `grid` (a CellGrid).
    A grid the device call would refuse gives zeros."""
    rec = _f32(records).reshape(-1, 24)
    labels = np.zeros(rec.shape[0], np.uint32)
    _lib.gs4d_host_cell_labels(rec.shape[0], _ptr(rec), C.byref(grid), _ptr(labels))
    return labels


def merge_query(alpha_max=1.0):
    """one gs4d_merge_query (MergeQuery)"""
    q = MergeQuery()
    q.alpha_max = float(alpha_max)
    return q


def merge_records_host(records, labels, alpha_max=1.0, stats=None, query=None, **rule):
    """gs4d_host_merge_records, the definition of Context.merge_records: (out float32 [n, 24] whose first `groups` rows are the merged records and
    the rest zeros, groups MERGE_GROUP [n] likewise, member_group uint32 [n], count: one MERGE_COUNT row) of records [n, 24] under labels uint32
    [n].  stats: a RECORD_STAT array of n rows (the rule keywords of compact_records let a record be a member by it) or None: every record; query:
    a MergeQuery instead of alpha_max.  A call the device would refuse gives zeros."""
    rec = _f32(records).reshape(-1, 24)
    n = rec.shape[0]
    lab = np.ascontiguousarray(labels, dtype=np.uint32)
    if lab.shape != (n,):
        raise ValueError("merge_records_host: labels must be n uint32 words")
    if stats is None and rule:
        raise TypeError("merge_records_host: a rule without stats")
    st = None if stats is None else np.ascontiguousarray(stats)
    if st is not None and (st.dtype.itemsize != 16 or st.ndim != 1 or st.shape[0] < n):
        raise ValueError("merge_records_host: stats must be at least n rows of 16 bytes")
    q = merge_query(alpha_max) if query is None else query
    k = _keep_rule(**rule)
    out, groups, member_group, count = np.zeros((n, 24), np.float32), np.zeros(n, MERGE_GROUP), np.zeros(n, np.uint32), np.zeros(1, MERGE_COUNT)
    _lib.gs4d_host_merge_records(n, _ptr(rec), _ptr(lab), C.byref(q), _ptr(st) if st is not None else None, _ptr(k) if st is not None else None,
                                 _ptr(out), _ptr(groups), _ptr(member_group), _ptr(count))
    return out, groups, member_group, count[0]


class RowsQuery(C.Structure):
    """gs4d_rows_query (include/gs4d.h): the row stride and the merged width of a gs4d_merge_rows call; 16 bytes."""
    _fields_ = [("stride", C.c_uint32), ("width", C.c_uint32), ("flags", C.c_uint32), ("reserved", C.c_uint32)]


def rows_query(stride, width=None):
    """one gs4d_rows_query (RowsQuery); width: every float32 word of the stride if None"""
    q = RowsQuery()
    q.stride, q.width = int(stride), int(stride) // 4 if width is None else int(width)
    return q


def merge_rows_host(rows, member_group, records=None, stride=None, width=None, dst=None, dst_first=0, query=None):
    """gs4d_host_merge_rows, the definition of Context.merge_rows: (dst, count) — dst, uint8 [capacity, stride], is a copy of `dst` (or, if None,
    zeros of room for dst_first + the largest group value + 1 rows) in which row dst_first + g holds the merged row of group g; count: one
    MERGE_COUNT row.  rows: the table, n rows of `stride` bytes (any dtype; stride: the bytes of a row of a 2-d array if None); member_group:
    uint32 [n]; records: float32 [n, 24], the weights by their mass, or None: unit weights; query: a RowsQuery instead of stride and width.  A
    call the device would refuse changes nothing."""
    table = np.ascontiguousarray(rows)
    mg = np.ascontiguousarray(member_group, dtype=np.uint32)
    n = mg.shape[0]
    if query is None:
        if stride is None:
            stride = table.shape[1] * table.itemsize if table.ndim == 2 else None
        if stride is None:
            raise ValueError("merge_rows_host: stride is needed for a table that is not 2-d")
        query = rows_query(stride, width)
    stride = int(query.stride)
    raw = table.reshape(-1).view(np.uint8)
    if mg.ndim != 1 or raw.size < n * stride:
        raise ValueError("merge_rows_host: member_group must be n uint32 words and rows at least n rows of `stride` bytes")
    rec = None if records is None else _f32(records).reshape(-1, 24)
    if rec is not None and rec.shape[0] < n:
        raise ValueError("merge_rows_host: records must be at least n rows of 24 floats")
    if dst is None:
        named = mg[mg != ID_NONE]
        out = np.zeros((int(dst_first) + (int(named.max()) + 1 if named.size else 0), max(stride, 1)), np.uint8)
    else:
        out = np.array(np.ascontiguousarray(dst).reshape(-1).view(np.uint8), copy=True)
        out = out[:out.size // max(stride, 1) * max(stride, 1)].reshape(-1, max(stride, 1))
    count = np.zeros(1, MERGE_COUNT)
    _lib.gs4d_host_merge_rows(n, _ptr(rec) if rec is not None else None, _ptr(mg), _ptr(raw), C.byref(query), _ptr(out), int(dst_first), out.shape[0], _ptr(count))
    return out, count[0]


class LodQuery(C.Structure):
    """gs4d_lod_query (include/gs4d.h): the eye, the time, the ratio and the level table of a gs4d_lod_cut call; 112 bytes."""
    _fields_ = [("eye", C.c_float * 3), ("t", C.c_float), ("ratio", C.c_float), ("near_dist", C.c_float), ("levels", C.c_uint32), ("flags", C.c_uint32),
                ("level_first", C.c_uint32 * 17), ("reserved", C.c_uint32 * 3)]


LOD_COUNT = np.dtype([("drawn", "<u4"), ("written", "<u4"), ("tested", "<u4"), ("drawn_leaves", "<u4")])   # gs4d_lod_count


class LodForest:
    """A forest of merged levels on the device (Context.build_lod, Context.lod_append): `nodes`, a buffer of n 96-byte records laid out level by level
    with the leaves first, `parent`, a buffer of n uint32, and level_first, the first node of every level with n behind the last.  A forest built
    over a table with a row per record (an SH table) carries `rows`, a buffer of n rows of row_stride bytes laid out like `nodes` whose first
    row_width float32 words are merged (Context.merge_rows); the three are None without a table."""

    def __init__(self, nodes, parent, level_first, rows=None, row_stride=None, row_width=None):
        self.nodes, self.parent = nodes, parent
        self.level_first = [int(v) for v in level_first]
        self.levels, self.n = len(self.level_first) - 1, self.level_first[-1]
        self.rows, self.row_stride, self.row_width = rows, row_stride, row_width


def lod_query(level_first, eye, t, ratio, near=0.0):
    """one gs4d_lod_query (LodQuery): level_first holds levels + 1 entries, the last one the node count"""
    first = [int(v) for v in level_first]
    if not 2 <= len(first) <= 17:
        raise ValueError("lod_query: level_first must hold 2 .. 17 entries (1 .. 16 levels and the node count)")
    q = LodQuery()
    q.eye[0], q.eye[1], q.eye[2] = (float(v) for v in eye)
    q.t, q.ratio, q.near_dist, q.levels = float(t), float(ratio), float(near), len(first) - 1
    for k, v in enumerate(first):
        q.level_first[k] = v
    return q


def lod_ratio(fov_deg, height, pixels, sigmas=3.0):
    """The ratio of lod_cut at which a node stops being refined once `sigmas` standard deviations of its largest rest extent cover at most `pixels`
    pixels of an image `height` pixels high under a vertical field of view of fov_deg: a length s at distance d covers s / d * (height / 2) /
    tan(fov / 2) pixels, and lod_cut compares sqrt(variance) / d with the ratio."""
    return float(pixels) * 2.0 * float(np.tan(np.radians(float(fov_deg)) * 0.5)) / (float(sigmas) * float(height))


def lod_cut_host(records, parent, query, capacity=None, stats=None):
    """gs4d_host_lod_cut, the definition of Context.lod_cut: (dst float32 [capacity, 24] whose first `written` rows are the cut and the rest zeros,
    cut_index uint32 [capacity] likewise, stats — a copy of `stats` (RECORD_STAT rows) or n zeroed rows — with one fragment added to the row of every
    DRAW node, count: one LOD_COUNT row) of the forest records [n, 24] / parent uint32 [n] under `query` (a LodQuery).  capacity: n if None.  A
    query the device call would refuse gives zeros."""
    rec = _f32(records).reshape(-1, 24)
    n = rec.shape[0]
    par = np.ascontiguousarray(parent, dtype=np.uint32)
    if par.shape != (n,):
        raise ValueError("lod_cut_host: parent must be n uint32 words")
    cap = n if capacity is None else int(capacity)
    st = np.zeros(n, RECORD_STAT) if stats is None else np.array(stats, copy=True)
    if st.dtype.itemsize != 16 or st.ndim != 1 or st.shape[0] < n:
        raise ValueError("lod_cut_host: stats must be at least n rows of 16 bytes")
    dst, index, count = np.zeros((max(cap, 1), 24), np.float32), np.zeros(max(cap, 1), np.uint32), np.zeros(1, LOD_COUNT)
    _lib.gs4d_host_lod_cut(n, _ptr(rec), _ptr(par), C.byref(query), _ptr(dst), _ptr(index), _ptr(st), _ptr(count), cap)
    return dst[:cap], index[:cap], st, count[0]


def hits_of(table, k):
    """the (n, k) HIT view of a hit table given as uint8 [n, hit_stride] (nearest_neighbours_host's, or Context.read of the buffer)"""
    t = np.ascontiguousarray(table, np.uint8)
    return np.ascontiguousarray(t[:, :8 * int(k)]).view(HIT).reshape(t.shape[0], int(k))


def knn_mean_dist2(hits_array, radius=None):
    """float32 [n]: the mean of the filled dist2 of each row of an (n, k) HIT array (a slot is filled iff its record is not ID_NONE) — the sum in
    slot order in float32, divided by the count; a row without a filled slot gets radius ** 2 in float32 (radius is needed then).  With k = 3
    over a point cloud this is the quantity 3DGS-style pipelines initialise scales from (distCUDA2 of simple-knn), restricted to a radius: a
    point with fewer than 3 points within the radius averages those it has."""
    h = np.asarray(hits_array)
    filled = h["record"] != ID_NONE
    cnt = filled.sum(1)
    if radius is None and (cnt == 0).any():
        raise ValueError("knn_mean_dist2: a row without hits needs the radius")
    s = np.zeros(h.shape[0], np.float32)
    for p in range(h.shape[1]):
        s = (s + np.where(filled[:, p], h["dist2"][:, p], np.float32(0.0))).astype(np.float32)
    fallback = np.float32(radius if radius is not None else 0.0) * np.float32(radius if radius is not None else 0.0)
    with np.errstate(all="ignore"):
        mean = (s / np.maximum(cnt, 1).astype(np.float32)).astype(np.float32)
    return np.where(cnt > 0, mean, np.float32(fallback)).astype(np.float32)


def frame_box(lo, hi, orientation, fov_deg, width, height):
    """gs4d_host_frame_box: the eye from which look_at(eye, orientation) and perspective(fov_deg, width, height, ..) show the whole box lo .. hi,
    its centre in the middle of the image ("frame selection": lo, hi of a Measure)."""
    out = np.zeros(3, np.float32)
    _lib.gs4d_host_frame_box(_ptr(_f32(lo)), _ptr(_f32(hi)), _ptr(_f32(orientation)), fov_deg, int(width), int(height), _ptr(out))
    return out


class SplatParams(C.Structure):
    """gs4d_splat_params (include/gs4d.h): the form and the parameter buffers of a gs4d_build_records call, or the destinations of a
    gs4d_decompose_records call (Context.decompose_records returns one; Context.build_records takes it in the place of the form)."""
    _fields_ = [("form", C.c_uint32), ("flags", C.c_uint32), ("pos", C.c_uint32), ("rot", C.c_uint32), ("rot_r", C.c_uint32), ("scale", C.c_uint32),
                ("rgba", C.c_uint32), ("dir", C.c_uint32), ("tvar", C.c_uint32), ("reserved", C.c_uint32)]

    def buffers(self):
        """{name: buffer} of the buffers that are given"""
        return {k: getattr(self, k) for k in ("pos", "rot", "rot_r", "scale", "rgba", "dir", "tvar") if getattr(self, k)}


class CameraInput(C.Structure):
    _fields_ = [("keys", C.c_uint), ("mouse_x", C.c_double), ("mouse_y", C.c_double), ("imgui_active", C.c_int)]


CAMKEY = {"W": 1, "S": 2, "A": 4, "D": 8, "E": 16, "Q": 32, "SPACE": 64, "LCTRL": 128, "LSHIFT": 256, "C": 512, "ESC": 1024}


def camera_input(state, keys, mouse_x, mouse_y, imgui_active=False):
    """One Camera::HandleInput call (Camera.cpp:116-183) on a CameraState; returns (recenter_cursor, hide_cursor)."""
    inp = CameraInput(int(keys), float(mouse_x), float(mouse_y), 1 if imgui_active else 0)
    rc, hide = C.c_int(0), C.c_int(0)
    _lib.gs4d_host_camera_input(C.byref(state), C.byref(inp), C.byref(rc), C.byref(hide))
    return bool(rc.value), bool(hide.value)


def camera_look_at_point(state, point):
    _lib.gs4d_host_camera_look_at_point(C.byref(state), _ptr(_f32(point)))


def camera_viewport(width, height):
    out = np.zeros(2, np.float32)
    _lib.gs4d_host_camera_viewport(width, height, _ptr(out))
    return out


def camera_focal(fov, width, height):
    out = np.zeros(2, np.float32)
    _lib.gs4d_host_camera_focal(fov, width, height, _ptr(out))
    return out


def unproject(view, proj, width, height, px, py, depth):
    """World point at view depth `depth` (-z_view, e.g. Context.read_aux(normalized=True)[..., 0]) on the ray through the centre of pixel
    (px, py): column px, row py counted from the bottom, as the images returned by read_pixels / read_aux are indexed ([py, px])."""
    out = np.zeros(3, np.float32)
    _lib.gs4d_host_unproject(_ptr(_f32(view)), _ptr(_f32(proj)), width, height, px, py, depth, _ptr(out))
    return out


def key_bounds(lo7, hi7, t, cam_pos, key_mode=KEY_REF_INV_EUCLID):
    """(bias, span) gs4d_keygen proves for the keys of records inside the box lo7 .. hi7 of (x, y, z, mu_t, vx, vy, vz): every key's bit
    pattern lies in [bias, bias + span]."""
    bias, span = C.c_uint32(0), C.c_uint32(0)
    _lib.gs4d_host_key_bounds(_ptr(_f32(lo7)), _ptr(_f32(hi7)), t, _ptr(_f32(cam_pos)), key_mode, C.byref(bias), C.byref(span))
    return bias.value, span.value


def write_png(path, rgba8):
    """(H, W, 4) uint8 frame, bottom row first (the framebuffer's orientation) -> PNG file."""
    a = np.ascontiguousarray(rgba8, np.uint8)
    if a.ndim != 3 or a.shape[2] != 4:
        raise ValueError("write_png: expected an (H, W, 4) uint8 array")
    if _lib.gs4d_host_write_png(os.fsencode(path), _ptr(a), a.shape[1], a.shape[0]) != 0:
        raise OSError(f"cannot write {path}")


def sh_row_bytes(degree):
    """The minimal row of gs4d_shade_sh's table for an SH degree: 12 (degree + 1)^2 bytes rounded up to 16 — 16 / 48 / 112 / 192."""
    return (12 * (int(degree) + 1) ** 2 + 15) // 16 * 16


def sh_rows(f_dc, f_rest, degree, stride=None):
    """The table of gs4d_shade_sh from a 3DGS export's arrays: f_dc [n, 3] and f_rest [n, 3 ((D + 1)^2 - 1)] for the export's degree D >= degree,
    channel-major as in the PLY (all R, then all G, then all B; None or empty for D = 0).  Returns uint8 [n, stride] (default: the minimal stride
    of `degree`): float32 row[3k + channel], k < (degree + 1)^2, zero padded to the stride."""
    f_dc = _f32(f_dc)
    n = f_dc.shape[0]
    if f_dc.shape != (n, 3):
        raise ValueError("sh_rows: f_dc must be [n, 3]")
    K = (int(degree) + 1) ** 2
    if not 0 <= int(degree) <= 3:
        raise ValueError("sh_rows: degree must be 0 .. 3")
    stride = sh_row_bytes(degree) if stride is None else int(stride)
    if stride % 16 or not 16 <= stride <= 1024 or stride < 12 * K:
        raise ValueError("sh_rows: stride must be a multiple of 16 from 16 to 1024 that holds 12 (degree + 1)^2 bytes")
    coeff = np.zeros((n, K, 3), np.float32)
    coeff[:, 0, :] = f_dc
    if K > 1:
        rest = _f32(f_rest).reshape(n, -1)
        if rest.shape[1] % 3 or rest.shape[1] // 3 < K - 1:
            raise ValueError("sh_rows: f_rest must be [n, 3 ((D + 1)^2 - 1)] with D >= degree")
        coeff[:, 1:, :] = rest.reshape(n, 3, -1)[:, :, :K - 1].transpose(0, 2, 1)
    rows = np.zeros((n, stride), np.uint8)
    rows[:, :12 * K] = coeff.reshape(n, 3 * K).view(np.uint8)
    return rows


def sh_row_bytes_t(degree, degree_t):
    """The minimal row of gs4d_shade_sh_t's table: 12 (degree + 1)^2 (degree_t + 1) bytes rounded up to 16 — 576 at degree 3 / degree_t 2."""
    return (12 * (int(degree) + 1) ** 2 * (int(degree_t) + 1) + 15) // 16 * 16


def sh_rows_t(features, degree, degree_t, src_degree=3, stride=None):
    """The table of gs4d_shade_sh_t from a 4DGS checkpoint: features [n, (src_degree + 1)^2 B, 3], coefficient-major with B >= degree_t + 1 blocks
    of (src_degree + 1)^2 coefficients (cat(features_dc, features_rest)).  Returns uint8 [n, stride] (default: the minimal stride): float32
    row[3 (b K + k) + channel] for the first K = (degree + 1)^2 coefficients k of the first degree_t + 1 blocks b, zero padded to the stride."""
    degree, degree_t, src_degree = int(degree), int(degree_t), int(src_degree)
    if not 0 <= degree <= 3 or not 0 <= degree_t <= 2 or src_degree < degree:
        raise ValueError("sh_rows_t: degree must be 0 .. 3, degree_t 0 .. 2, src_degree >= degree")
    K, KS = (degree + 1) ** 2, (src_degree + 1) ** 2
    f = _f32(features)
    if f.ndim != 3 or f.shape[2] != 3 or f.shape[1] % KS or f.shape[1] // KS < degree_t + 1:
        raise ValueError("sh_rows_t: features must be [n, (src_degree + 1)^2 B, 3] with B >= degree_t + 1")
    n = f.shape[0]
    stride = sh_row_bytes_t(degree, degree_t) if stride is None else int(stride)
    used = 12 * K * (degree_t + 1)
    if stride % 16 or not 16 <= stride <= 1024 or stride < used:
        raise ValueError("sh_rows_t: stride must be a multiple of 16 from 16 to 1024 that holds 12 (degree + 1)^2 (degree_t + 1) bytes")
    coeff = np.ascontiguousarray(f.reshape(n, -1, KS, 3)[:, :degree_t + 1, :K, :])
    rows = np.zeros((n, stride), np.uint8)
    rows[:, :used] = coeff.reshape(n, used // 4).view(np.uint8)
    return rows


_hip_runtime = None


def _hip():
    """the HIP runtime the process has loaded (libgs4d.so links it), for the one call write_tensor makes itself"""
    global _hip_runtime
    if _hip_runtime is None:
        _hip_runtime = C.CDLL("libamdhip64.so")
        _hip_runtime.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
        _hip_runtime.hipMemcpyAsync.restype = C.c_int
    return _hip_runtime


# ---- device context -----------------------------------------------------------------------------
class Context:
    """One GPU context (gs4d_ctx): buffers, pipeline state, a small swap chain of RGBA32F framebuffers (one per frame lane)."""

    def __init__(self, width, height, device=0):
        h = C.c_void_p()
        rc = _lib.gs4d_create(device, width, height, C.byref(h))
        if rc != 0:
            raise Gs4dError(f"gs4d_create failed ({rc}): {_lib.gs4d_last_error(None).decode()}")
        self._h = h
        self.width, self.height = width, height

    def close(self):
        if getattr(self, "_h", None):
            _lib.gs4d_destroy(self._h)
            self._h = None

    def __del__(self):
        self.close()

    def _chk(self, rc):
        if rc != 0:
            raise Gs4dError(f"gs4d error {rc}: {_lib.gs4d_last_error(self._h).decode()}")

    # buffers
    def buffer(self, data=None, nbytes=None):
        name = C.c_uint32()
        if data is not None:
            a = np.ascontiguousarray(data)
            self._chk(_lib.gs4d_buffer_create(self._h, _ptr(a), a.nbytes, C.byref(name)))
        else:
            self._chk(_lib.gs4d_buffer_create(self._h, None, nbytes, C.byref(name)))
        return name.value

    def subdata(self, buf, data, offset=0):
        a = np.ascontiguousarray(data)
        self._chk(_lib.gs4d_buffer_subdata(self._h, buf, offset, _ptr(a), a.nbytes))

    def read(self, buf, dtype, count, offset=0):
        out = np.empty(count, dtype)
        self._chk(_lib.gs4d_buffer_read(self._h, buf, offset, _ptr(out), out.nbytes))
        return out

    def delete(self, buf):
        self._chk(_lib.gs4d_buffer_destroy(self._h, buf))

    def device_ptr(self, buf):
        p, n = C.c_void_p(), C.c_size_t()
        self._chk(_lib.gs4d_buffer_device_ptr(self._h, buf, C.byref(p), C.byref(n)))
        return p.value, n.value

    def invalidate(self, buf):
        """Before overwriting a buffer through its device pointer on the caller's stream (gs4d_buffer_invalidate)."""
        self._chk(_lib.gs4d_buffer_invalidate(self._h, buf))

    def bind(self, slot, buf):
        self._chk(_lib.gs4d_bind_storage(self._h, slot, buf))

    # state
    def set_mode(self, mode):
        self._chk(_lib.gs4d_set_mode(self._h, mode))

    def set_uniforms(self, time=None, min_opacity=None, view=None, proj=None):
        if time is not None:
            self._chk(_lib.gs4d_set_uniform_1f(self._h, U_TIME, time))
        if min_opacity is not None:
            self._chk(_lib.gs4d_set_uniform_1f(self._h, U_MIN_OPACITY, min_opacity))
        if view is not None:
            self._chk(_lib.gs4d_set_uniform_mat4(self._h, U_VIEW, _ptr(_f32(view))))
        if proj is not None:
            self._chk(_lib.gs4d_set_uniform_mat4(self._h, U_PROJ, _ptr(_f32(proj))))

    def set_clear_color(self, rgba):
        self._chk(_lib.gs4d_set_clear_color(self._h, _ptr(_f32(rgba))))

    def set_blend(self, src, dst):
        self._chk(_lib.gs4d_set_blend(self._h, src, dst))

    def clear(self):
        self._chk(_lib.gs4d_clear(self._h))

    def resize(self, width, height):
        self._chk(_lib.gs4d_resize(self._h, width, height))
        self.width, self.height = width, height

    # ordering
    def sort_pairs(self, keys, vals, n):
        self._chk(_lib.gs4d_sort_pairs(self._h, keys, vals, n))

    def keygen(self, data, t, cam_pos, keys, idx, n, key_mode=KEY_REF_INV_EUCLID):
        self._chk(_lib.gs4d_keygen(self._h, data, t, _ptr(_f32(cam_pos)), keys, idx, n, key_mode))

    # draw / read-back
    def draw_instanced(self, instances):
        self._chk(_lib.gs4d_draw_instanced(self._h, instances))

    def draw_quads(self, vertices, nquads):
        self._chk(_lib.gs4d_draw_quads(self._h, vertices, nquads))

    def draw_lines(self, verts, rgba, width=1.0, viewproj=None, strip=False):
        """Renderer::DrawLine/DrawGrid/DrawAxis: verts (n, 3) with viewproj, or (n, 2) NDC positions; GL_LINES pairs or a GL_LINE_STRIP."""
        v = _f32(verts)
        dims = v.shape[-1]
        vp = _f32(viewproj) if viewproj is not None else None
        self._chk(_lib.gs4d_draw_lines(self._h, _ptr(v), v.size // dims, dims, 1 if strip else 0, _ptr(vp) if vp is not None else None, _ptr(_f32(rgba)), width))

    def read_pixels(self):
        out = np.empty((self.height, self.width, 4), np.float32)
        self._chk(_lib.gs4d_read_pixels(self._h, _ptr(out), out.nbytes))
        return out

    def read_pixels_device(self, dptr, nbytes):
        self._chk(_lib.gs4d_read_pixels_device(self._h, C.c_void_p(dptr), nbytes))

    def read_pixels_rgba8_device(self, dptr, nbytes):
        self._chk(_lib.gs4d_read_pixels_rgba8_device(self._h, C.c_void_p(dptr), nbytes))

    def read_frame_rgba8_device(self, frames_back, dptr, nbytes):
        """Pack the current (0) or the previous (1) image of the swap chain to RGBA8 at device pointer `dptr`, asynchronously."""
        self._chk(_lib.gs4d_read_frame_rgba8_device(self._h, frames_back, C.c_void_p(dptr), nbytes))

    def read_frame_rgba8_device_after(self, frames_back, dptr, nbytes, hip_event=None):
        """As read_frame_rgba8_device, but the pack waits only for `hip_event` (a hipEvent_t handle; None: for nothing) instead of for
        everything queued on the caller's stream: for callers that alternate between destination buffers."""
        self._chk(_lib.gs4d_read_frame_rgba8_device_after(self._h, frames_back, C.c_void_p(dptr), nbytes, C.c_void_p(hip_event or 0)))

    # aux outputs: per-pixel depth and opacity
    def set_aux_outputs(self, on):
        """Frames cleared from the next clear() on carry (D, O) per pixel beside the colour (default blend function only)."""
        self._chk(_lib.gs4d_set_aux_outputs(self._h, 1 if on else 0))

    def read_aux(self, normalized=False):
        """(H, W, 2) float32, rows bottom-up like read_pixels: raw (D, O) — they compose across draws — or with normalized=True
        (D / O, O): the expected depth, 0 where O == 0."""
        out = np.empty((self.height, self.width, 2), np.float32)
        self._chk(_lib.gs4d_read_aux(self._h, _ptr(out), out.nbytes))
        if normalized:
            d, o = out[..., 0], out[..., 1]
            out = np.stack([np.divide(d, o, out=np.zeros_like(d), where=o > 0), o], axis=-1)
        return out

    def read_aux_device(self, dptr, nbytes):
        """Raw (D, O) planes to device pointer `dptr` (e.g. a torch tensor's data_ptr()), asynchronously like read_pixels_device."""
        self._chk(_lib.gs4d_read_aux_device(self._h, C.c_void_p(dptr), nbytes))

    # ID outputs: which splat record each pixel shows, for picking and selection
    ID_NONE = 0xFFFFFFFF

    def set_id_outputs(self, on):
        """Frames cleared from the next clear() on carry {record, draw, weight} per pixel beside the colour — and (D, O), as with
        set_aux_outputs(True) (default blend function only)."""
        self._chk(_lib.gs4d_set_id_outputs(self._h, 1 if on else 0))

    def read_ids(self, rect=None):
        """(record uint32, draw uint32, weight float32), each (h, w), rows bottom-up like read_pixels; rect = (x, y, w, h) with y counted
        from the bottom row, None = the whole image.  A pixel no fragment reached holds record = draw = ID_NONE and weight 0."""
        x, y, w, h = rect if rect is not None else (0, 0, self.width, self.height)
        if w <= 0 or h <= 0:
            self._chk(_lib.gs4d_read_ids(self._h, x, y, w, h, None, None, None))       # refused: the error names the rectangle
        rec, drw, wt = np.empty((h, w), np.uint32), np.empty((h, w), np.uint32), np.empty((h, w), np.float32)
        self._chk(_lib.gs4d_read_ids(self._h, x, y, w, h, _ptr(rec), _ptr(drw), _ptr(wt)))
        return rec, drw, wt

    def read_ids_device(self, record_ptr, draw_ptr, weight_ptr, bytes_per_plane):
        """The full planes to device pointers (each W * H * 4 bytes; 0 / None skips a plane), asynchronously like read_aux_device."""
        self._chk(_lib.gs4d_read_ids_device(self._h, C.c_void_p(record_ptr or 0), C.c_void_p(draw_ptr or 0), C.c_void_p(weight_ptr or 0), bytes_per_plane))

    def pick(self, px, py, view, proj):
        """What pixel (px, py) (column, row from the bottom) of the current frame shows: a dict with the record, its draw, its weight,
        the pixel's expected depth D / O and the world point at that depth on the pixel's ray (unproject); None where no fragment reached
        the pixel.  The frame must have been cleared with ID outputs on."""
        rec, drw, wt = self.read_ids((px, py, 1, 1))
        if int(rec[0, 0]) == self.ID_NONE:
            return None
        do = self.read_aux()[py, px]
        depth = float(do[0] / do[1]) if do[1] > 0.0 else 0.0
        return {"record": int(rec[0, 0]), "draw": int(drw[0, 0]), "weight": float(wt[0, 0]), "depth": depth,
                "point": unproject(view, proj, self.width, self.height, px, py, depth)}

    # depth test against the caller's depth plane: splats among opaque geometry
    def depth_plane(self, z):
        """A buffer for set_depth_test from an (H, W) float32 array of view depths (-z_view, rows bottom-up like read_pixels; +inf = no
        geometry)."""
        a = np.ascontiguousarray(z, np.float32)
        if a.shape != (self.height, self.width):
            raise ValueError(f"depth_plane: expected shape {(self.height, self.width)}, got {a.shape}")
        return self.buffer(a)

    def set_depth_test(self, plane):
        """Draws issued from now on blend a fragment of depth d at pixel p only where d < Z[p] (GL_LESS) against the buffer `plane`
        (depth_plane); None or 0 turns the test off.  Draw state: it survives clear(); deleting the buffer turns it off."""
        self._chk(_lib.gs4d_set_depth_test(self._h, int(plane or 0)))

    # record statistics: what each record contributed to the picture
    RECORD_STAT = RECORD_STAT

    def record_stats(self, n):
        """A zeroed buffer of n gs4d_record_stat for set_record_stats."""
        return self.buffer(np.zeros(n, self.RECORD_STAT))

    def set_record_stats(self, buf, n=0):
        """Draws issued from now on add, per record, the fragments that entered the colour with weight w > 0 (pixels), the largest such w
        (wmax) and the sum of rint(w * 2^24) (wsum) into `buf` (record_stats); None or 0 turns it off.  Draw state: it survives clear();
        nothing zeroes the buffer (subdata zeros to start a new count); deleting it turns the statistics off."""
        self._chk(_lib.gs4d_set_record_stats(self._h, int(buf or 0), int(n) if buf else 0))

    def read_record_stats(self, buf, n):
        """Structured array (pixels uint32, wmax float32, wsum uint64) of the first n records, after every draw issued so far."""
        return self.read(buf, self.RECORD_STAT, n)

    # compaction: prune a record set by its record statistics, on the device
    KEEP_RULE = KEEP_RULE
    COMPACT_COUNT = np.dtype([("kept", "<u4"), ("written", "<u4")])

    def compact_records(self, stats, n, src=None, stride=96, dst=None, kept_index=None, count=None, min_pixels=1, min_wmax=0.0, min_wsum=0, invert=False):
        """Stable compaction on the device (gs4d_compact_records): record i of the n is kept iff (pixels >= min_pixels and wmax >= min_wmax
        and wsum >= min_wsum) != invert, with the record_stats row stats[i]; the kept `stride`-byte records of `src` go to `dst` in
        ascending i, their indices (uint32) to `kept_index`, and `count` (a new 8-byte buffer if None) receives COMPACT_COUNT {kept, written}.
        Any of dst / kept_index may be None.  min_wmax is a weight (float32), min_wsum is in units of 2^-24.  Asynchronous; returns `count`."""
        rule = _keep_rule(min_pixels, min_wmax, min_wsum, invert)
        if count is None:
            count = self.buffer(nbytes=self.COMPACT_COUNT.itemsize)
        self._chk(_lib.gs4d_compact_records(self._h, int(stats), int(n), _ptr(rule), int(src or 0), int(stride), int(dst or 0), int(kept_index or 0), int(count)))
        return count

    def read_compact_count(self, count):
        """(kept, written) of a compact_records call; blocks until its kernels have finished."""
        c = self.read(count, self.COMPACT_COUNT, 1)[0]
        return int(c["kept"]), int(c["written"])

    def prune(self, stats, n, src, stride=96, **rule):
        """compact_records into exact-size new buffers: counts first, allocates, compacts.  Returns (dst, kept_index, kept); the buffers hold
        at least 16 bytes, so kept == 0 still gives valid names."""
        count = self.compact_records(stats, n, stride=stride, **rule)
        kept, _ = self.read_compact_count(count)
        dst, kept_index = self.buffer(nbytes=max(16, kept * int(stride))), self.buffer(nbytes=max(16, kept * 4))
        self.compact_records(stats, n, src=src, stride=stride, dst=dst, kept_index=kept_index, count=count, **rule)
        got, written = self.read_compact_count(count)
        self.delete(count)
        if (got, written) != (kept, kept):
            raise Gs4dError(f"prune: the table changed between the two passes ({kept} kept, then {got} kept / {written} written)")
        return dst, kept_index, kept

    # to a budget: the threshold of one statistics field that keeps the records that matter most
    STAT_FIELDS = {"pixels": STAT_PIXELS, "wmax": STAT_WMAX, "wsum": STAT_WSUM}
    CUT = np.dtype([("value", "<u8"), ("above", "<u4"), ("equal", "<u4")])

    def stat_cut(self, stats, n, budget, field="wsum", out=None):
        """gs4d_stat_cut: the k-th largest value, k = min(budget, n), of one field ("pixels", "wmax" as its bit pattern, "wsum"; or a
        STAT_* constant) of the n record_stats rows of `stats`, with the number of rows above it and equal to it, as one CUT {value, above,
        equal} into `out` (a new 16-byte buffer if None).  A selection on the device: no sort, no permutation.  Asynchronous; returns `out`."""
        if out is None:
            out = self.buffer(nbytes=self.CUT.itemsize)
        self._chk(_lib.gs4d_stat_cut(self._h, int(stats), int(n), int(self.STAT_FIELDS.get(field, field)), int(budget), int(out)))
        return out

    def read_stat_cut(self, out):
        """(value, above, equal) of a stat_cut call; blocks until its kernels have finished."""
        c = self.read(out, self.CUT, 1)[0]
        return int(c["value"]), int(c["above"]), int(c["equal"])

    def prune_to_budget(self, stats, n, src, budget, field="wsum", stride=96):
        """At most `budget` of the n records of `src`, those with the largest `field`, in exact-size new buffers and in their original order:
        stat_cut, one 16-byte read-back, compact_records with the field's threshold at `value` if above + equal <= budget, else at value + 1
        (a tie at the cut that does not fit is dropped whole) — no count-only pass, and no second read-back: `kept` follows from the cut.  Returns (dst, kept_index, kept), as prune does; the
        buffers hold at least 16 bytes, so kept == 0 (nothing above a tie that does not fit) still gives valid names."""
        out = self.stat_cut(stats, n, budget, field)
        value, above, equal = self.read_stat_cut(out)
        self.delete(out)
        fits = above + equal <= int(budget)
        kept = above + equal if fits else above
        dst, kept_index = self.buffer(nbytes=max(16, kept * int(stride))), self.buffer(nbytes=max(16, kept * 4))
        if kept == 0:
            return dst, kept_index, 0
        rule = np.zeros(1, self.KEEP_RULE)
        name = {v: k for k, v in self.STAT_FIELDS.items()}.get(field, field)
        rule["min_" + name] = value if fits else value + 1       # (kept > 0: value + 1 does not leave the field)
        count = self.buffer(nbytes=self.COMPACT_COUNT.itemsize)
        self._chk(_lib.gs4d_compact_records(self._h, int(stats), int(n), _ptr(rule), int(src), int(stride), int(dst), int(kept_index), int(count)))
        self.delete(count)                                       # (nothing between the cut and the compaction adds to the table: the count is `kept`)
        return dst, kept_index, kept

    # selection: a statistics table from a region of the ID planes
    def count_ids(self, stats, n, rect=None, mask=None, draws=None, min_weight=0.0):
        """gs4d_count_ids: every pixel of `rect` ((x, y, w, h), y from the bottom row; None: the whole image) of the current frame's ID planes
        whose record is below n, whose draw ordinal lies in `draws` (an int, or a (first, last) pair; None: every draw), whose weight is >=
        min_weight and whose `mask` byte is non-zero (a buffer of w*h bytes, rows bottom-up, or an (h, w) bool / uint8 array that is uploaded
        for the call; None: no mask) adds one fragment to row record of the record_stats buffer `stats`: pixels += 1, wmax = max(wmax,
        weight), wsum += rint(weight * 2^24).  Nothing zeroes `stats`: calls add up.  Asynchronous with a buffer mask or none; an array mask is
        uploaded and deleted again, and deleting a buffer waits for every frame lane: keep the mask in a buffer where that matters."""
        x, y, w, h = rect if rect is not None else (0, 0, self.width, self.height)
        first, last = (0, 0xFFFFFFFF) if draws is None else (int(draws), int(draws)) if np.ndim(draws) == 0 else (int(draws[0]), int(draws[1]))
        region = IdRegion(int(x), int(y), int(w), int(h), first, last, int(np.array([min_weight], np.float32).view(np.uint32)[0]), 0)
        own = mask is not None and not isinstance(mask, (int, np.integer))
        if own:
            a = np.ascontiguousarray(np.asarray(mask) != 0, np.uint8)
            if a.shape != (h, w):
                raise ValueError(f"count_ids: expected a mask of shape {(h, w)}, got {a.shape}")
            mask = self.buffer(a)
        try:
            self._chk(_lib.gs4d_count_ids(self._h, C.byref(region), int(mask or 0), int(stats), int(n)))
        finally:
            if own:
                self.delete(mask)

    def select(self, n, src=None, stride=96, rect=None, mask=None, draws=None, min_weight=0.0):
        """The records of the n that some pixel of the region shows (count_ids into a zeroed table, then compact_records with min_pixels=1), in
        exact-size new buffers and in their original order.  Returns (dst, kept_index, kept, stats): as prune does, and the table, whose rows
        say how much of the region each record holds (stat_cut on it: the k most visible).  src None: no records are copied (dst is None).
        Blocking, as prune is: it reads the count back."""
        stats = self.record_stats(n)
        self.count_ids(stats, n, rect=rect, mask=mask, draws=draws, min_weight=min_weight)
        if src is not None:
            return self.prune(stats, n, src, stride=stride, min_pixels=1) + (stats,)
        count = self.compact_records(stats, n, stride=stride, min_pixels=1)
        kept, _ = self.read_compact_count(count)
        kept_index = self.buffer(nbytes=max(16, kept * 4))
        self.compact_records(stats, n, stride=stride, kept_index=kept_index, count=count, min_pixels=1)
        self.delete(count)
        return None, kept_index, kept, stats

    # selection by where a record is: a statistics table from a volume or a screen region
    def count_centres(self, stats, n, data, mask=None, **query):
        """gs4d_count_centres: row i of the record_stats buffer `stats` gets one fragment of weight 1 (remove=True: becomes zero) iff the centre of
        record i < n of `data` at time t passes every test of the query — centre_query's keywords, or query=a CentreQuery — whether anything shows
        it or not.  mask: a buffer of w*h bytes, rows bottom-up, or an (h, w) bool / uint8 array that is uploaded for the call, as count_ids takes
        it; with screen= only.  Nothing zeroes `stats`: calls add up (rule min_pixels=1: the union; min_pixels=k: the intersection of k calls).
        With the bits of count_centres_host.  Asynchronous with a buffer mask or none."""
        q = query.pop("query", None)
        if q is None:
            q = centre_query(**query)
        elif query:
            raise TypeError("count_centres: query= excludes centre_query's keywords")
        own = mask is not None and not isinstance(mask, (int, np.integer))
        if own:
            a = np.ascontiguousarray(np.asarray(mask) != 0, np.uint8)
            if a.shape != (q.h, q.w):
                raise ValueError(f"count_centres: expected a mask of shape {(q.h, q.w)}, got {a.shape}")
            mask = self.buffer(a)
        try:
            self._chk(_lib.gs4d_count_centres(self._h, int(data), int(n), C.byref(q), int(mask or 0), int(stats)))
        finally:
            if own:
                self.delete(mask)

    def select_volume(self, n, data, src=None, stride=96, **query):
        """The records of the n of `data` whose centre passes the query (count_centres into a zeroed table, then compact_records with
        min_pixels=1), in exact-size new buffers and in their original order: the analogue of select for records that ARE somewhere.  Returns
        (dst, kept_index, kept, stats), as select does.  src: the buffer whose `stride`-byte records are copied (usually `data` itself); None:
        no records are copied (dst is None).  mask= goes to count_centres.  Blocking, as prune is: it reads the count back."""
        stats = self.record_stats(n)
        self.count_centres(stats, n, data, **query)
        if src is not None:
            return self.prune(stats, n, src, stride=stride, min_pixels=1) + (stats,)
        count = self.compact_records(stats, n, stride=stride, min_pixels=1)
        kept, _ = self.read_compact_count(count)
        kept_index = self.buffer(nbytes=max(16, kept * 4))
        self.compact_records(stats, n, stride=stride, kept_index=kept_index, count=count, min_pixels=1)
        self.delete(count)
        return None, kept_index, kept, stats

    # where a selection is: bounds and centroid of selected records
    def measure_records(self, data, n, t=0.0, stats=None, skip_hidden=False, skip_dead=False, out=None, query=None, **rule):
        """gs4d_measure_records: how many of the selected ones of the first n 96-byte records of `data` have a finite centre at time t, the box of
        those centres, the box of centre -/+ reach and the cell sums of the centroid, as one 96-byte Measure into `out` (a new buffer if None).
        stats: a record_stats buffer whose row i selects record i by compact_records' rule keywords (None: every record, and no rule);
        skip_hidden / skip_dead: leave out records of alpha <= 0 / dead at t (they are counted in `skipped`); query: a MeasureQuery instead of
        t and the skips.  With the bits of measure_records_host.  Asynchronous; returns `out`."""
        if stats is None and rule:
            raise TypeError("measure_records: a rule without stats")
        q = measure_query(t, skip_hidden, skip_dead) if query is None else query
        k = _keep_rule(**rule) if stats is not None else None
        if out is None:
            out = self.buffer(nbytes=C.sizeof(Measure))
        self._chk(_lib.gs4d_measure_records(self._h, int(data), int(n), C.byref(q), int(stats or 0), _ptr(k) if k is not None else None, int(out)))
        return out

    def read_measure(self, out):
        """The Measure of a measure_records call as a dict (Measure.as_dict: count, unplaced, skipped, lo, hi, ext_lo, ext_hi, cell_sum,
        centre); blocks until its kernels have finished."""
        raw = self.read(out, np.uint8, C.sizeof(Measure))
        return Measure.from_buffer_copy(raw.tobytes()).as_dict()

    # a coarser level of detail: a label per record from a cell grid, one moment-matched record per labelled group
    def cell_labels(self, data, n, grid, labels=None):
        """gs4d_cell_labels: labels[i] (a buffer of n uint32; a new one if None) = the cell of the rest mean of record i < n of `data` in `grid` (a
        CellGrid: cell_grid), ID_NONE where a coordinate that is looked at is a NaN.  With the bits of cell_labels_host.  Asynchronous; returns
        `labels`."""
        if labels is None:
            labels = self.buffer(nbytes=max(16, 4 * int(n)))
        self._chk(_lib.gs4d_cell_labels(self._h, int(data), int(n), C.byref(grid), int(labels)))
        return labels

    def merge_records(self, data, n, labels, alpha_max=1.0, stats=None, dst=None, groups=None, member_group=None, count=None, query=None, **rule):
        """gs4d_merge_records: one record per group of members of equal label among the first n 96-byte records of `data` — the group's mass-weighted
        mean, covariance and colour, alpha from the preserved mass clamped at alpha_max — into `dst` (a new buffer of n records if None), in
        ascending label.  labels: a buffer of n uint32 (cell_labels, label_components; ID_NONE: no member).  stats: a record_stats buffer whose row i
        lets record i be a member by compact_records' rule keywords (None: every record, and no rule).  groups: a buffer of MERGE_GROUP rows
        {label, size, first} or None; member_group: a buffer of n uint32 (the group of every record, ID_NONE for a non-member) or None; count: a
        buffer of 16 bytes (a new one if None) that receives the MERGE_COUNT.  No slot past what dst and groups hold is written.  With the bits of
        merge_records_host.  A full write of dst: the next draw rebuilds its SoA shadow.  Asynchronous; returns (dst, count)."""
        if stats is None and rule:
            raise TypeError("merge_records: a rule without stats")
        q = merge_query(alpha_max) if query is None else query
        k = _keep_rule(**rule) if stats is not None else None
        if dst is None:
            dst = self.buffer(nbytes=max(16, 96 * int(n)))
        if count is None:
            count = self.buffer(nbytes=MERGE_COUNT.itemsize)
        self._chk(_lib.gs4d_merge_records(self._h, int(data), int(n), int(labels), C.byref(q), int(stats or 0), _ptr(k) if k is not None else None,
                                          int(dst), int(groups or 0), int(member_group or 0), int(count)))
        return dst, count

    def read_merge_count(self, count):
        """The MERGE_COUNT row (groups, written, members, left_out) of a merge_records call; blocks until its kernels have finished."""
        return self.read(count, np.uint32, 4).view(MERGE_COUNT)[0]

    def lod(self, data, n, grid, alpha_max=1.0):
        """A coarser level of detail of the first n records of `data`: cell_labels in `grid`, then merge_records over those labels.  Asynchronous;
        returns (dst, count) — read_merge_count(count).written records of dst are the set to draw."""
        labels = self.cell_labels(data, n, grid)
        try:
            return self.merge_records(data, n, labels, alpha_max=alpha_max)
        finally:
            self.delete(labels)

    # the view's cut through a forest of merged levels
    def lod_append(self, level, m, nodes, parent, first, member_group=None, child_first=0, c=0):
        """gs4d_lod_append: the m 96-byte records of `level` become nodes first .. first + m - 1 of the forest buffers `nodes` / `parent`, with parent
        word ID_NONE; with member_group (merge_records' output over the c nodes from child_first on) those nodes get their parents: first +
        member_group[i], or ID_NONE where that word is not below m.  Asynchronous."""
        self._chk(_lib.gs4d_lod_append(self._h, int(level), int(m), int(member_group or 0), int(child_first), int(c), int(nodes), int(parent), int(first)))

    def merge_rows(self, member_group, n, rows, stride, width=None, data=None, dst=None, dst_first=0, count=None, query=None):
        """gs4d_merge_rows: row dst_first + g of `dst` <- the mean of the rows of the members of group g — the records i < n with member_group[i]
        == g (a buffer of n uint32, merge_records' output; ID_NONE: no member) whose first `width` float32 words of their row of `rows` (n rows of
        `stride` bytes) are finite — weighted by the mass of merge_records of the 96-byte records of `data`, or plainly if data is None: the SH
        row of a merged record.  width: every word of the stride if None.  dst: a new buffer of dst_first + n rows if None; rows of groups without
        members and rows past what dst holds are not written.  count: a buffer of 16 bytes (a new one if None) that receives the MERGE_COUNT.
        query: a RowsQuery instead of stride and width.  With the bits of merge_rows_host.  Asynchronous; returns (dst, count)."""
        q = rows_query(stride, width) if query is None else query
        if dst is None:
            dst = self.buffer(nbytes=max(16, (int(dst_first) + int(n)) * int(q.stride)))
        if count is None:
            count = self.buffer(nbytes=MERGE_COUNT.itemsize)
        self._chk(_lib.gs4d_merge_rows(self._h, int(data or 0), int(n), int(member_group), int(rows), C.byref(q), int(dst), int(dst_first), int(count)))
        return dst, count

    def copy_rows(self, src, m, stride, dst=None, src_first=0, dst_first=0):
        """gs4d_copy_rows: rows dst_first .. of `dst` (a new buffer of dst_first + m rows if None) <- rows src_first .. src_first + m - 1 of `src`,
        `stride` bytes each (a multiple of 16 up to 1024), bits kept; the rest of dst keeps its contents.  Asynchronous; returns `dst`."""
        if dst is None:
            dst = self.buffer(nbytes=max(16, (int(dst_first) + int(m)) * int(stride)))
        self._chk(_lib.gs4d_copy_rows(self._h, int(src), int(src_first), int(m), int(stride), int(dst), int(dst_first)))
        return dst

    def build_lod(self, data, n, grids, alpha_max=1.0, rows=None, row_stride=None, row_width=None):
        """A LodForest over the first n records of `data`: level 0 is the set itself, and for each CellGrid of `grids`, coarser each time, the level
        above is merge_records of the level below under cell_labels in that grid (a counting merge, one count read-back, then the merge into an
        exact-size buffer), linked with lod_append through member_group.  rows: a table of n rows of row_stride bytes (an SH table; row_width:
        the float32 words of a row that are merged, all of them if None) — the forest then carries a table with a row per node: the leaf rows by
        copy_rows, every level above by merge_rows of the level below under the same member_group (into a buffer of the level's own, since a call
        cannot read and write one buffer, then copy_rows).  At most 15 grids.  Blocking: once per upload, not per frame."""
        grids = list(grids)
        if len(grids) > 15:
            raise ValueError("build_lod: at most 15 grids (16 levels)")
        if rows is None:
            if row_stride is not None or row_width is not None:
                raise TypeError("build_lod: row_stride or row_width without rows")
            return self._build_lod(data, n, grids, alpha_max, None, None)
        if row_stride is None:
            raise TypeError("build_lod: rows without row_stride")
        return self._build_lod(data, n, grids, alpha_max, rows, rows_query(row_stride, row_width))

    def _build_lod(self, data, n, grids, alpha_max, rows, rq):
        levels, links, made = [(data, int(n))], [], []
        tables = [rows]
        try:
            for grid in grids:
                prev, pn = levels[-1]
                labels = self.cell_labels(prev, pn, grid)
                made.append(labels)
                none = self.buffer(nbytes=16)                  # (holds no record: the merge counts)
                made.append(none)
                _, count = self.merge_records(prev, pn, labels, alpha_max=alpha_max, dst=none)
                made.append(count)
                groups = int(self.read_merge_count(count)["groups"])
                dst, member_group = self.buffer(nbytes=max(16, 96 * groups)), self.buffer(nbytes=max(16, 4 * pn))
                made += [dst, member_group]
                self.merge_records(prev, pn, labels, alpha_max=alpha_max, dst=dst, member_group=member_group, count=count)
                if rows is not None:
                    # zeros first: a group whose members all have a non-finite row gets no merged row
                    table = self.buffer(np.zeros(max(16, int(rq.stride) * groups), np.uint8))
                    made.append(table)
                    self.merge_rows(member_group, pn, tables[-1], rq.stride, data=prev, dst=table, count=count, query=rq)
                    tables.append(table)
                levels.append((dst, groups))
                links.append(member_group)
            first = [0]
            for _, m in levels:
                first.append(first[-1] + m)
            nodes, parent = self.buffer(nbytes=max(16, 96 * first[-1])), self.buffer(nbytes=max(16, 4 * first[-1]))
            for k, (buf, m) in enumerate(levels):
                if k == 0:
                    self.lod_append(buf, m, nodes, parent, 0)
                else:
                    self.lod_append(buf, m, nodes, parent, first[k], member_group=links[k - 1], child_first=first[k - 1], c=levels[k - 1][1])
            if rows is None:
                return LodForest(nodes, parent, first)
            forest_rows = self.buffer(nbytes=max(16, int(rq.stride) * first[-1]))
            for k, (_, m) in enumerate(levels):
                self.copy_rows(tables[k], m, rq.stride, dst=forest_rows, dst_first=first[k])
            return LodForest(nodes, parent, first, rows=forest_rows, row_stride=int(rq.stride), row_width=int(rq.width))
        finally:
            for b in made:
                self.delete(b)

    def lod_cut(self, forest, eye, t, ratio, near=0.0, dst=None, cut_index=None, stats=None, count=None, query=None):
        """gs4d_lod_cut: the cut of a camera at `eye` and the time t through `forest` (a LodForest) — from the roots down, a node is drawn where its
        largest rest variance is at most (ratio * distance) ** 2 (lod_ratio; distances below `near` count as it) or it is a leaf, and refined
        otherwise.  The drawn nodes go to `dst` (96 bytes each) and their indices to `cut_index` in ascending node index, as far as those hold;
        `stats` (a record_stats buffer of forest.n rows) gets one fragment per drawn node; any of the three may be None.  count: a buffer of 16
        bytes (a new one if None) that receives the LOD_COUNT.  query: a LodQuery instead of eye, t, ratio and near.  With the words of
        lod_cut_host.  A full write of dst.  Asynchronous; returns `count`."""
        q = lod_query(forest.level_first, eye, t, ratio, near) if query is None else query
        if count is None:
            count = self.buffer(nbytes=LOD_COUNT.itemsize)
        self._chk(_lib.gs4d_lod_cut(self._h, int(forest.nodes), int(forest.parent), int(forest.n), C.byref(q), int(dst or 0), int(cut_index or 0),
                                    int(stats or 0), int(count)))
        return count

    def lod_rows(self, forest, cut_index, m, dst=None):
        """The rows of a cut: gather_records of forest.rows (a LodForest built with a table) through the cut_index of lod_cut, m of its entries —
        slot j of `dst` (a new buffer if None) <- the row of node cut_index[j].  Per frame: lod_cut, lod_rows, shade_sh, keygen, sort, draw.
        Asynchronous; returns `dst`."""
        if forest.rows is None:
            raise ValueError("lod_rows: the forest carries no rows (build_lod(..., rows=...))")
        return self.gather_records(cut_index, m, forest.rows, forest.n, stride=forest.row_stride, dst=dst)

    def read_lod_count(self, count):
        """The LOD_COUNT row (drawn, written, tested, drawn_leaves) of a lod_cut call; blocks until its kernels have finished."""
        return self.read(count, np.uint32, 4).view(LOD_COUNT)[0]

    # records relative to each other: the sources within a radius of each record
    def count_neighbours(self, stats, n, data, radius=None, t=0.0, cap=0xFFFFFFFF, source=None, skip_hidden=False, skip_dead=False, count_self=False,
                         query=None, **rule):
        """gs4d_count_neighbours: row i of the record_stats buffer `stats` gets c fragments of weight 1, c = min(cap, the number of source
        records whose centre at time t lies within `radius` of that of record i < n of `data`) — records of a non-finite centre, and with
        skip_hidden / skip_dead those of alpha <= 0 / dead at t, take no part on either side.  source: a record_stats buffer whose row j makes
        record j a source by compact_records' rule keywords (None: every record, and no rule); count_self: a source counts itself; query: a
        NeighbourQuery instead of the radius and the other keywords.  Nothing zeroes `stats`: calls add up.  With the bits of
        count_neighbours_host, from a hashed grid instead of its double loop.  Asynchronous."""
        if source is None and rule:
            raise TypeError("count_neighbours: a rule without source")
        if query is None:
            if radius is None:
                raise TypeError("count_neighbours: radius or query is needed")
            query = neighbour_query(radius, t, cap, skip_hidden, skip_dead, count_self)
        k = _keep_rule(**rule) if source is not None else None
        self._chk(_lib.gs4d_count_neighbours(self._h, int(data), int(n), C.byref(query), int(source or 0), _ptr(k) if k is not None else None, int(stats)))

    def grow_selection(self, n, data, source, radius, t=0.0, cap=1, skip_hidden=False, skip_dead=False, **rule):
        """Grow a selection: a fresh zeroed table filled by one count_neighbours call with count_self, whose rule min_pixels=1 selects every record
        within `radius` of a record that `source` selects by the rule keywords (default min_pixels=1) — a superset of the part of the selection
        that takes part.  cap=1 is all a selection needs; a larger cap leaves the number of selected records nearby in pixels.  Growing again
        takes the result as the source.  Asynchronous; returns the table."""
        stats = self.record_stats(n)
        self.count_neighbours(stats, n, data, radius, t=t, cap=cap, source=source, skip_hidden=skip_hidden, skip_dead=skip_dead, count_self=True, **rule)
        return stats

    def isolated(self, n, data, radius, k, t=0.0, skip_hidden=False, skip_dead=False):
        """Isolated records (floaters): a fresh zeroed table with, per record that takes part, the number of OTHER records within `radius`,
        saturating at k — ready for the rule min_pixels=k, invert=True (compact_records, hide, edit_colours), which selects the records with fewer
        than k neighbours (those that take no part among them: their rows stay zero).  Asynchronous; returns the table."""
        stats = self.record_stats(n)
        self.count_neighbours(stats, n, data, radius, t=t, cap=k, skip_hidden=skip_hidden, skip_dead=skip_dead)
        return stats

    # connected clusters: one label per record, the cluster's size as a table, what a selection touches by label
    def label_components(self, n, data, radius=None, t=0.0, cap=0xFFFFFFFF, source=None, skip_hidden=False, skip_dead=False, labels=None, stats=None,
                         query=None, **rule):
        """gs4d_label_components: labels[i] (a buffer of n uint32; a new one if None) = the smallest record index of the connected component of
        record i < n of `data` — members linked iff their centres at time t lie within `radius` of each other — or ID_NONE for a record that is
        no member (a non-finite centre; with skip_hidden / skip_dead alpha <= 0 / dead at t; not selected by `source`).  stats: a record_stats
        buffer whose row i gets min(cap, size of the component) fragments of weight 1 for a member (None: labels only); nothing zeroes it.
        source: a record_stats buffer whose row i selects record i by compact_records' rule keywords (None: every record, and no rule); query: a
        ComponentQuery instead of the radius and the other keywords.  With the bits of label_components_host.  Asynchronous; returns `labels`."""
        if source is None and rule:
            raise TypeError("label_components: a rule without source")
        if query is None:
            if radius is None:
                raise TypeError("label_components: radius or query is needed")
            query = component_query(radius, t, cap, skip_hidden, skip_dead)
        k = _keep_rule(**rule) if source is not None else None
        if labels is None:
            labels = self.buffer(nbytes=max(16, 4 * int(n)))
        self._chk(_lib.gs4d_label_components(self._h, int(data), int(n), C.byref(query), int(source or 0), _ptr(k) if k is not None else None, int(labels),
                                             int(stats or 0)))
        return labels

    def count_labels(self, stats, n, labels, seeds, **rule):
        """gs4d_count_labels: row i of the record_stats buffer `stats` gets one fragment of weight 1 iff labels[i] (a buffer of n uint32, as
        label_components leaves it) is below n and is the label of some record < n whose row of the record_stats buffer `seeds` passes
        compact_records' rule keywords (default min_pixels=1).  Nothing zeroes `stats`.  With the bits of count_labels_host.  Asynchronous."""
        k = _keep_rule(**rule)
        self._chk(_lib.gs4d_count_labels(self._h, int(labels), int(n), int(seeds), _ptr(k), int(stats)))

    def small_components(self, n, data, radius, k, t=0.0, skip_hidden=False, skip_dead=False):
        """Floater clumps: (labels, a fresh zeroed table with, per member, the size of its connected component saturating at k) — ready for the
        rule min_pixels=k, invert=True (compact_records, edit_colours), which selects the records in clusters of fewer than k records (those that
        are no members among them: their rows stay zero), like isolated.  Asynchronous."""
        stats = self.record_stats(n)
        labels = self.label_components(n, data, radius, t=t, cap=k, skip_hidden=skip_hidden, skip_dead=skip_dead, stats=stats)
        return labels, stats

    def select_connected(self, n, data, seeds, radius, t=0.0, skip_hidden=False, skip_dead=False, labels=None, **rule):
        """Select connected: (labels, a fresh zeroed table whose rule min_pixels=1 selects every record of a connected component that holds a
        record `seeds` selects by the rule keywords (default min_pixels=1)).  labels: a buffer label_components has filled for this edit state
        (then `data`, radius, t and the skips are not used), or None: they are computed over every record.  Asynchronous."""
        if labels is None:
            labels = self.label_components(n, data, radius, t=t, skip_hidden=skip_hidden, skip_dead=skip_dead)
        stats = self.record_stats(n)
        self.count_labels(stats, n, labels, seeds, **rule)
        return labels, stats

    # the k nearest sources of every record: a neighbour list, a density-adaptive distance
    HIT = HIT

    def nearest_neighbours(self, n, data, radius=None, k=3, t=0.0, source=None, skip_hidden=False, skip_dead=False, include_self=False, hits=None,
                           hit_stride=None, stats=None, query=None, **rule):
        """gs4d_nearest_neighbours: the first k HIT slots of row i of `hits` (rows hit_stride bytes apart; a new buffer of n rows if None;
        hit_stride: default hit_stride_for(k), else a multiple of 16 up to 1024 that is at least 8 k) <- the k (1 .. 16) source records nearest to
        record i < n of `data` among those whose centre at time t lies within `radius` of its own, ordered by (dist2, record index); empty slots,
        and all k of a record that takes no part, are {ID_NONE, +inf}; bytes of a row past 8 k keep their contents.  stats: a record_stats buffer
        whose row i gets pixels += hits found, wmax = max(wmax, dist2 of the last of them), wsum += found << 24 (None: hits only); nothing zeroes
        it.  source: a record_stats buffer whose row j makes record j a source by compact_records' rule keywords (None: every record, and no
        rule); include_self: a source is its own hit; query: a NearestQuery instead of the radius, k and the other keywords.  With the bits of
        nearest_neighbours_host, from a hashed grid instead of its double loop.  Asynchronous; returns `hits`, or (hits, stats) with a table."""
        if source is None and rule:
            raise TypeError("nearest_neighbours: a rule without source")
        if query is None:
            if radius is None:
                raise TypeError("nearest_neighbours: radius or query is needed")
            query = nearest_query(radius, k, t, skip_hidden, skip_dead, include_self)
        if hit_stride is None:
            hit_stride = hit_stride_for(query.k)
        kr = _keep_rule(**rule) if source is not None else None
        if hits is None:
            hits = self.buffer(nbytes=max(16, int(n) * int(hit_stride)))
        self._chk(_lib.gs4d_nearest_neighbours(self._h, int(data), int(n), C.byref(query), int(source or 0), _ptr(kr) if kr is not None else None, int(hits),
                                               int(hit_stride), int(stats or 0)))
        return hits if stats is None else (hits, stats)

    def read_hits(self, hits, n, k, hit_stride=None):
        """The (n, k) HIT array {record, dist2} of a nearest_neighbours table of stride hit_stride (default hit_stride_for(k)); blocks until the
        kernels have finished."""
        hit_stride = hit_stride_for(k) if hit_stride is None else int(hit_stride)
        if int(n) == 0:
            return np.zeros((0, int(k)), HIT)
        return hits_of(self.read(hits, np.uint8, int(n) * hit_stride).reshape(int(n), hit_stride), k)

    def sparse_records(self, n, data, radius, k, t=0.0, skip_hidden=False, skip_dead=False):
        """Density-adaptive floaters: (hits, a fresh zeroed table filled by one nearest_neighbours call) — per record that takes part, pixels =
        the number of other records found within `radius` (at most k) and wmax = the dist2 of the last of them.  Three selections follow without
        another kernel:
            compact_records(stats, n, min_pixels=k, invert=True)        fewer than k records within radius
            compact_records(stats, n, min_wmax=x)                       the k-th neighbour (or the last one found) at dist2 >= x
            prune_to_budget(stats, n, data, K, field="wmax")            the K records whose k-th neighbour is farthest (stat_cut over wmax)
        — the last is the floater tool for a set whose density varies, where isolated() needs one radius for all of it.  Asynchronous."""
        stats = self.record_stats(n)
        hits = self.nearest_neighbours(n, data, radius, k, t=t, skip_hidden=skip_hidden, skip_dead=skip_dead, stats=stats)[0]
        return hits, stats

    # time windows: the records of a 4D set that can show anything between two times
    TIME_SPAN =np.dtype([("t_first", "<f4"), ("t_last", "<f4")])

    def record_time_spans(self, data, n, min_opacity=0.0, spans=None):
        """gs4d_record_time_spans: for each of the n 96-byte records of `data`, the closed interval of float32 times outside which it provably
        contributes nothing to a draw with uMinOpacity == min_opacity, as TIME_SPAN rows into `spans` (a new buffer if None): {+inf, -inf}
        never, {-inf, +inf} always.  Once per upload.  Asynchronous; returns `spans`."""
        if spans is None:
            spans = self.buffer(nbytes=max(16, int(n) * self.TIME_SPAN.itemsize))
        self._chk(_lib.gs4d_record_time_spans(self._h, int(data), int(n), float(min_opacity), int(spans)))
        return spans

    def compact_time_window(self, spans, n, t0, t1, src=None, stride=96, dst=None, kept_index=None, count=None):
        """gs4d_compact_time_window: compact_records with the table of record_time_spans and the rule "the span meets [t0, t1]" (t_first <= t1
        and t_last >= t0; infinite ends allowed).  Asynchronous; returns `count` (a new 8-byte buffer if None)."""
        if count is None:
            count = self.buffer(nbytes=self.COMPACT_COUNT.itemsize)
        self._chk(_lib.gs4d_compact_time_window(self._h, int(spans), int(n), float(t0), float(t1), int(src or 0), int(stride), int(dst or 0), int(kept_index or 0), int(count)))
        return count

    def time_window(self, data, n, t0, t1, min_opacity=0.0, spans=None, stride=96):
        """The records of `data` that can show anything at a uTime in [t0, t1], in exact-size new buffers: computes the spans unless the caller
        kept them from an earlier call (`spans`), counts, allocates, compacts.  Returns (dst, kept_index, kept); the buffers hold at least 16
        bytes, so kept == 0 still gives valid names.  A draw of (dst, kept) at such a time gives the bits of a draw of (data, n)."""
        own = spans is None
        if own:
            spans = self.record_time_spans(data, n, min_opacity)
        count = self.compact_time_window(spans, n, t0, t1, stride=stride)
        kept, _ = self.read_compact_count(count)
        dst, kept_index = self.buffer(nbytes=max(16, kept * int(stride))), self.buffer(nbytes=max(16, kept * 4))
        self.compact_time_window(spans, n, t0, t1, src=data, stride=stride, dst=dst, kept_index=kept_index, count=count)
        got, written = self.read_compact_count(count)
        self.delete(count)
        if own:
            self.delete(spans)
        if (got, written) != (kept, kept):
            raise Gs4dError(f"time_window: the spans changed between the two passes ({kept} kept, then {got} kept / {written} written)")
        return dst, kept_index, kept

    # spatial order: a record set reordered so that neighbours in space are neighbours in memory
    def spatial_order(self, src, n, stride=96, pos_offset=0, order_index=None):
        """gs4d_spatial_order: the permutation that puts the n `stride`-byte records of `src` into Morton order of their positions (three
        float32 at pos_offset; 10 bits per axis over the box of the finite positions; records with a non-finite coordinate last; equal codes
        keep their order) as uint32 into `order_index` (a new buffer if None): order_index[j] = the record that comes j-th.  Once per upload.
        Asynchronous; returns `order_index`."""
        if order_index is None:
            order_index = self.buffer(nbytes=max(16, int(n) * 4))
        self._chk(_lib.gs4d_spatial_order(self._h, int(src), int(n), int(stride), int(pos_offset), int(order_index)))
        return order_index

    def gather_records(self, index, m, src, nsrc, stride=96, dst=None):
        """gs4d_gather_records: slot j of `dst` (a new buffer if None) <- the `stride` bytes of record index[j] of the nsrc records of `src`,
        j < m; an entry >= nsrc leaves its slot as it is.  stride: a multiple of 16 up to 1024, or 4 or 8 (index lists, TIME_SPAN rows).  Reorders a set by spatial_order's index, or carries a table with a row per record
        along with a reorder or a compaction (its kept_index).  Asynchronous; returns `dst`."""
        if dst is None:
            dst = self.buffer(nbytes=max(16, int(m) * int(stride)))
        self._chk(_lib.gs4d_gather_records(self._h, int(index), int(m), int(src), int(nsrc), int(stride), int(dst)))
        return dst

    def reorder_spatial(self, data, n, stride=96):
        """The n records of `data` in spatial order, in new buffers: spatial_order, then gather_records.  Returns (dst, order_index); the
        buffers hold at least 16 bytes, so n == 0 still gives valid names.  A GS4D_MODE_4D_SORTED draw of (dst, n) gives the bits of a draw of
        (data, n) when no two records share a depth key (gs4d.h); gather a table with a row per record through the same order_index."""
        order_index = self.spatial_order(data, n, stride=stride)
        return self.gather_records(order_index, n, data, n, stride=stride), order_index

    # view-dependent colour: rgb from spherical harmonics
    def shade_sh(self, data, n, sh, degree, t, cam_pos, sh_stride=None):
        """gs4d_shade_sh: floats 4..6 of the first n 96-byte records of `data` <- the colour of their rows of `sh` (float32 coefficients
        row[3k + channel], see sh_rows) at SH degree 0..3, seen from cam_pos at time t.  sh_stride: bytes per row, a multiple of 16 up to 1024
        (default: the minimal one for the degree, sh_row_bytes(degree)); a table of a higher degree is shaded through a prefix of its rows.
        A colour-only write: a current SoA shadow is patched, not rebuilt.  Per frame: shade, keygen, sort, draw.  Asynchronous."""
        if sh_stride is None:
            sh_stride = sh_row_bytes(degree)
        self._chk(_lib.gs4d_shade_sh(self._h, int(data), int(n), int(sh), int(sh_stride), int(degree), float(t), _ptr(_f32(cam_pos))))

    # time-varying view-dependent colour: SH times a cosine series in time, the colour model of trained 4D sets
    def shade_sh_t(self, data, n, sh, degree, degree_t, t, inv_period, cam_pos, sh_stride=None):
        """gs4d_shade_sh_t: floats 4..6 of the first n 96-byte records of `data` <- the colour of their rows of the 4D table `sh` (degree_t + 1
        blocks of (degree + 1)^2 coefficients, see sh_rows_t; block b weighted by cos(2 pi b (t - mu_t) inv_period)) seen from cam_pos at time t,
        with the bits of shade_sh_t_host — and of shade_sh on collapse_sh's rows.  sh_stride: bytes per row (default sh_row_bytes_t(degree,
        degree_t)).  degree may be a ShTime, which then carries everything but the buffers.  A colour-only write: a current SoA shadow is patched,
        not rebuilt.  Per frame: shade_sh_t, keygen, sort, draw.  Asynchronous."""
        q = _sh_time(degree, degree, degree_t, t, inv_period, cam_pos)
        if sh_stride is None:
            sh_stride = sh_row_bytes_t(q.degree, q.degree_t)
        self._chk(_lib.gs4d_shade_sh_t(self._h, int(data), int(n), int(sh), int(sh_stride), C.byref(q)))

    def collapse_sh(self, data, n, sh, degree, degree_t, t, inv_period, sh_stride=None, dst=None, dst_stride=None):
        """gs4d_collapse_sh: row i < n of `dst` (a new buffer if None; dst_stride bytes a row, default sh_row_bytes(degree)) <- the 3DGS row that
        row i of the 4D table `sh` is at time t for the mu_t of record i of `data`, zeros behind it, with the bits of collapse_sh_host: shade_sh of
        the rows at `degree` gives what shade_sh_t gives.  data and sh are only read.  Asynchronous; returns `dst`."""
        q = _sh_time(degree, degree, degree_t, t, inv_period)
        if sh_stride is None:
            sh_stride = sh_row_bytes_t(q.degree, q.degree_t)
        if dst_stride is None:
            dst_stride = sh_row_bytes(q.degree)
        if dst is None:
            dst = self.buffer(nbytes=max(16, int(n) * int(dst_stride)))
        self._chk(_lib.gs4d_collapse_sh(self._h, int(data), int(n), int(sh), int(sh_stride), C.byref(q), int(dst), int(dst_stride)))
        return dst

    # colour edits by a selection: recolour, hide or restore selected records
    COLOUR_EDIT = COLOUR_EDIT

    def edit_colours(self, data, n, op, value=(0.0, 0.0, 0.0, 0.0), channels="rgb", amount=0.0, stats=None, from_=None, **rule):
        """gs4d_edit_colours: the rgba (floats 4..7) of the selected ones of the first n 96-byte records of `data`, edited in place — op "set"
        (c = value), "mul" (c = c * value), "lerp" (c = c + amount * (value - c)) or "copy" (c = the same float of record i of `from_`), on the
        channels named ("rgba" letters or the mask 1 .. 15).  stats: a record_stats table (count_ids, set_record_stats) whose row i selects
        record i by compact_records' rule keywords (min_pixels, min_wmax, min_wsum, invert); None: every record.  With the bits of
        edit_colours_host.  A colour-only write: a current SoA shadow is patched, not rebuilt.  Per frame: (shade_sh), edit, keygen, sort,
        draw.  Asynchronous."""
        if stats is None and rule:
            raise TypeError("edit_colours: a rule without stats")
        e = colour_edit(op, value, channels, amount)
        k = _keep_rule(**rule) if stats is not None else None
        self._chk(_lib.gs4d_edit_colours(self._h, int(data), int(n), _ptr(e), int(stats or 0), _ptr(k) if k is not None else None, int(from_ or 0)))

    def hide(self, data, n, stats, **rule):
        """The selected records' alpha set to 0 (edit_colours "set" on "a"): with the default blend function they draw nothing, count nothing and
        are never picked — the picture of the compacted complement without moving a record.  restore_colours puts them back."""
        self.edit_colours(data, n, "set", (0.0, 0.0, 0.0, 0.0), "a", stats=stats, **rule)

    def restore_colours(self, data, n, from_, stats=None, **rule):
        """The rgba of the selected records (every record if stats is None) copied back from the pristine records `from_` (edit_colours "copy")."""
        self.edit_colours(data, n, "copy", channels="rgba", stats=stats, from_=from_, **rule)

    # records from parameters: the records of a splat set built on the device
    PARAM_BUFFERS = ("pos", "rot", "rot_r", "scale", "rgba", "dir", "tvar")

    def build_records(self, form, n, dst=None, **buffers):
        """gs4d_build_records: the first n 96-byte records of `dst` (a new buffer if None) from row i of the parameter buffers of the form —
        PARAMS_3D: pos (3 floats), rot (w x y z), scale (3), rgba; PARAMS_4D_VEL: pos (x y z mu_t), rot, scale (3), dir (3), tvar (1: see
        time_variance), rgba; PARAMS_4D_2Q: pos (4), rot, rot_r, scale (4), rgba — with the bits of build_records_3d / build_records_4d_tvar /
        build_records_4d_2q.  A full write of dst: the next draw rebuilds its SoA shadow.  Per frame: build, (shade_sh), keygen, sort, draw.
        Asynchronous; returns `dst`.  form may be the SplatParams that decompose_records returned: its form and its buffers."""
        if isinstance(form, SplatParams):
            form, buffers = form.form, {**form.buffers(), **buffers}
        unknown = set(buffers) - set(self.PARAM_BUFFERS)
        if unknown:
            raise TypeError(f"build_records: unknown parameter buffer(s) {sorted(unknown)}")
        if dst is None:
            dst = self.buffer(nbytes=max(16, int(n) * 96))
        params = SplatParams(int(form), 0, *(int(buffers.get(k) or 0) for k in self.PARAM_BUFFERS), 0)
        self._chk(_lib.gs4d_build_records(self._h, C.byref(params), int(n), int(dst)))
        return dst

    # records back to parameters: a set edited on the device taken out for a trainer or a file
    def decompose_records(self, src, n, form, src_first=0, only=None, **buffers):
        """gs4d_decompose_records: row i < n of every destination from record src_first + i of `src`, with the bits of decompose_records_host —
        PARAMS_3D: pos (3 floats), rot (w x y z), scale (3), rgba; PARAMS_4D_VEL: pos (4), rot, scale, rgba, dir (3), tvar (1).  Destinations are
        given by name (pos=buffer, ...); those of `only` (default: all of the form) that are not given are allocated.  With neither rot nor scale
        the eigen-solve does not run.  src is not written and its shadow not touched.  Asynchronous; returns the SplatParams of the destinations,
        which build_records accepts back and read_params reads."""
        unknown = set(buffers) - set(self.PARAM_BUFFERS)
        if unknown:
            raise TypeError(f"decompose_records: unknown destination(s) {sorted(unknown)}")
        rows, names = _param_names(form, tuple(buffers) if only is None and buffers else only)
        use = {k: int(v) for k, v in buffers.items() if v}
        made = []
        try:
            for k in names:
                if k not in use:
                    use[k] = self.buffer(nbytes=max(16, int(n) * 4 * rows[k]))
                    made.append(use[k])
            params = SplatParams(int(form), 0, *(use.get(k, 0) for k in self.PARAM_BUFFERS), 0)
            self._chk(_lib.gs4d_decompose_records(self._h, int(src), int(n), int(src_first), C.byref(params)))
        except Exception:
            for b in made:
                self.delete(b)
            raise
        return params

    def read_params(self, params, n):
        """The first n rows of every buffer of a SplatParams as {name: float32 [n, k]} (blocking reads)."""
        rows = dict(PARAM_ROWS.get(params.form, {"pos": 4, "rot": 4, "scale": 4, "rgba": 4}), rot_r=4)
        return {k: self.read(b, np.float32, int(n) * rows[k]).reshape(int(n), rows[k]) for k, b in params.buffers().items()}

    # placing a set: the records under 4D affine maps
    def transform_records(self, src, n, xf, m=1, dst=None, dst_first=0):
        """gs4d_transform_records: record dst_first + j * n + i of `dst` (a new buffer of dst_first + m * n records if None) <- record i < n of
        `src` under row j < m of `xf` — a buffer of 80-byte rows (affine4, Affine4), or an (m, 20) float32 array, which is uploaded to a
        temporary buffer (m is then its row count; deleting it waits for the device, so a frame loop keeps a buffer of its own) — with the bits
        of transform_records_host.  A full write of dst: the next draw rebuilds its SoA
        shadow.  Per frame: (shade_sh), transform, keygen, sort, draw.  Asynchronous; returns `dst`."""
        own = not isinstance(xf, (int, np.integer))
        if own:
            rows = _affine_rows(xf)
            m = rows.shape[0]
            xf = self.buffer(rows) if m else self.buffer(nbytes=80)
        try:
            if dst is None:
                dst = self.buffer(nbytes=max(16, (int(dst_first) + int(m) * int(n)) * 96))
            self._chk(_lib.gs4d_transform_records(self._h, int(src), int(n), int(xf), int(m), int(dst), int(dst_first)))
        finally:
            if own:
                self.delete(xf)
        return dst

    # one transform per record: a set posed by a table of maps
    def pose_records(self, src, n, xf, bind, form=None, m=None, bind_stride=None, dst=None, dst_first=0):
        """gs4d_pose_records: record dst_first + i of `dst` (a new buffer of dst_first + n records if None) <- record i < n of `src` under what row i
        of `bind` takes from the m rows of `xf`, with the bits of pose_records_host; a row that names no row of the table copies the record.  xf: a
        buffer of 80-byte rows (m is then required) or an [m, 20] float32 array; bind: a buffer (form is then required; bind_stride defaults to 4 /
        32) or a uint32 [n] array of row indices (POSE_INDEX) or a bind_rows array (POSE_BLEND4).  Arrays are uploaded to temporary buffers
        (deleting them waits for the device, so a frame loop keeps buffers of its own and updates xf with subdata).  A full write of dst: the next
        draw rebuilds its SoA shadow.  Per frame: (shade_sh), pose, keygen, sort, draw.  Asynchronous; returns `dst`."""
        temps = []
        try:
            if not isinstance(xf, (int, np.integer)):
                rows = _f32(xf).reshape(-1, 20)
                m = rows.shape[0]
                xf = self.buffer(rows) if m else self.buffer(nbytes=80)
                temps.append(xf)
            elif m is None:
                raise TypeError("m is required when xf is a buffer")
            if not isinstance(bind, (int, np.integer)):
                table, form, bind_stride = _bind_table(bind, form, bind_stride)
                bind = self.buffer(table) if table.size else self.buffer(nbytes=32)
                temps.append(bind)
            else:
                if form is None:
                    raise TypeError("form is required when bind is a buffer")
                if bind_stride is None:
                    bind_stride = 4 if form == POSE_INDEX else 32
            if dst is None:
                dst = self.buffer(nbytes=max(16, (int(dst_first) + int(n)) * 96))
            self._chk(_lib.gs4d_pose_records(self._h, int(src), int(n), int(xf), int(m), int(bind), int(form), int(bind_stride), int(dst), int(dst_first)))
        finally:
            for b in temps:
                self.delete(b)
        return dst

    # an SH table turned with the maps that move its records
    def rotate_sh(self, src, n, xf, degree, m=1, bind=None, form=None, bind_stride=None, stride=None, dst=None, dst_first=0):
        """gs4d_rotate_sh: a rotated copy of the first n rows of the SH table `src` (stride bytes a row, default the minimal row of the degree) in
        `dst` (a new buffer if None), with the bits of rotate_sh_host.  bind None: SH_EACH — row dst_first + j * n + i <- row i under map j < m of
        `xf`, the layout of transform_records.  Else row dst_first + i <- row i under the map row i of `bind` chooses, as pose_records: pass the
        same xf, bind, form and m again.  xf: a buffer of 80-byte rows (with m) or an [m, 20] float32 array; bind: a buffer (form is then
        required) or a uint32 [n] / bind_rows array.  Arrays are uploaded to temporary buffers.  Per frame: pose, rotate_sh, shade_sh (on the
        posed set with the true camera), keygen, sort, draw.  Asynchronous; returns `dst`."""
        temps = []
        try:
            if stride is None:
                stride = sh_row_bytes(degree)
            if not isinstance(xf, (int, np.integer)):
                rows = _f32(xf).reshape(-1, 20)
                m = rows.shape[0]
                xf = self.buffer(rows) if m else self.buffer(nbytes=80)
                temps.append(xf)
            if bind is None:
                form = SH_EACH if form is None else form
                bind, bind_stride = 0, 0 if bind_stride is None else bind_stride
            elif not isinstance(bind, (int, np.integer)):
                table, form, bind_stride = _bind_table(bind, form, bind_stride)
                bind = self.buffer(table) if table.size else self.buffer(nbytes=32)
                temps.append(bind)
            else:
                if form is None:
                    raise TypeError("form is required when bind is a buffer")
                if bind_stride is None:
                    bind_stride = 4 if form == POSE_INDEX else 32
            if dst is None:
                total = int(m) * int(n) if form == SH_EACH else int(n)
                dst = self.buffer(nbytes=max(16, (int(dst_first) + total) * int(stride)))
            self._chk(_lib.gs4d_rotate_sh(self._h, int(src), int(n), int(stride), int(degree), int(xf), int(m), int(bind), int(form), int(bind_stride), int(dst),
                                          int(dst_first)))
        finally:
            for b in temps:
                self.delete(b)
        return dst

    # a map that varies from point to point: a set deformed through a 4D lattice
    def warp_records(self, src, n, nodes, lat, dst=None, dst_first=0):
        """gs4d_warp_records: record dst_first + i of `dst` (a new buffer of dst_first + n records if None) <- record i < n of `src` through the map
        x' = x + D(x) of the Lattice `lat` (lattice()), linearised at the record's centre, with the bits of warp_records_host; a record whose centre
        is not inside the lattice is copied.  nodes: a buffer of 16-byte nodes (dx, dy, dz, dt), or an array of the lattice's size, which is
        uploaded to a temporary buffer (deleting it waits for the device, so a frame loop keeps a buffer of its own and updates it with subdata).
        A full write of dst: the next draw rebuilds its SoA shadow.  Per frame: (shade_sh), warp, keygen, sort, draw.  Asynchronous; returns `dst`."""
        own = not isinstance(nodes, (int, np.integer))
        if own:
            nodes = self.buffer(_lattice_nodes(nodes, lat))
        try:
            if dst is None:
                dst = self.buffer(nbytes=max(16, (int(dst_first) + int(n)) * 96))
            self._chk(_lib.gs4d_warp_records(self._h, int(src), int(n), int(nodes), C.byref(lat), int(dst), int(dst_first)))
        finally:
            if own:
                self.delete(nodes)
        return dst

    # a frame of a clip as a 3D set: the records baked at one time
    def slice_records(self, src, n, t, min_opacity=0.0, mu_t_out=None, s44_out=1.0, dst=None, dst_first=0):
        """gs4d_slice_records: record dst_first + i of `dst` (a new buffer of dst_first + n records if None) <- record i < n of `src` conditioned at
        time t: the conditional centre and covariance, alpha times the time opacity floored at min_opacity, mu_t = mu_t_out (None: t), Sigma44 =
        s44_out, a time row and column of -0 — with the bits of slice_records_host but for word 7, which is the alpha the device's draw computes.
        A draw of the slice at uTime == mu_t_out with uMinOpacity == min_opacity <= 1 gives the bits of a draw of src at uTime == t.  A full write
        of dst: the next draw rebuilds its SoA shadow, as the 64-byte static layout when dst holds nothing else.  Asynchronous; returns `dst`."""
        q = slice_query(t, min_opacity, mu_t_out, s44_out)
        if dst is None:
            dst = self.buffer(nbytes=max(16, (int(dst_first) + int(n)) * 96))
        self._chk(_lib.gs4d_slice_records(self._h, int(src), int(n), C.byref(q), int(dst), int(dst_first)))
        return dst

    def freeze(self, data, n, t, min_opacity=0.0, mu_t_out=None, s44_out=1.0):
        """The 3D set that the 4D set (data, n) is at time t, without the records that show nothing there: slice_records, then the records of
        the slice with alpha > 0 (count_centres with skip_hidden into a zeroed table, compact_records with min_pixels=1) in their old order, in
        exact-size new buffers.  Returns (dst, kept_index, count): the set, the uint32 index in `data` of each of its records, and the
        COMPACT_COUNT buffer, whose `kept` is their number (read_compact_count; it is settled when the call returns).  A record of alpha 0 changes no pixel under the default blend, so a draw of (dst, kept) at uTime == mu_t_out
        (None: t) is the draw of (data, n) at t, record i of dst being record kept_index[i] of data.  For a long clip the cheaper order is
        compact_time_window(spans, n, t, t) first and slice_records of the survivors: the slice then reads only what can show at t.  A source
        with a 4D SH table keeps its view dependence: collapse_sh of the source's table at t, then gather_records of the collapsed rows through
        kept_index — shade_sh of (dst, kept) at time mu_t_out with those rows gives the colours shade_sh_t gives the source at t."""
        sliced = self.slice_records(data, n, t, min_opacity, mu_t_out, s44_out)
        table = self.buffer(np.zeros(max(1, int(n)), RECORD_STAT))
        try:
            self.count_centres(table, n, sliced, skip_hidden=True)
            count = self.compact_records(table, n)
            kept, _ = self.read_compact_count(count)
            dst, kept_index = self.buffer(nbytes=max(16, kept * 96)), self.buffer(nbytes=max(16, kept * 4))
            self.compact_records(table, n, src=sliced, dst=dst, kept_index=kept_index, count=count)
            got, written = self.read_compact_count(count)
        finally:
            self.delete(table)
            self.delete(sliced)
        if (got, written) != (kept, kept):
            raise Gs4dError(f"freeze: the table changed between the two passes ({kept} kept, then {got} kept / {written} written)")
        return dst, kept_index, count

    # moving a selection: the selected records under a 4D affine map about a pivot, in place
    def transform_selected(self, data, n, xf, stats=None, pivot=None, measure=None, **rule):
        """gs4d_transform_selected: the selected ones of the first n 96-byte records of `data` <- themselves under xf (20 float32 as affine4 gives
        them, an Affine4, or a SelectionXf, which then carries pivot and flag itself), in place.  stats: a record_stats table (count_ids,
        count_centres, set_record_stats) whose row i selects record i by compact_records' rule keywords; None: every record.  pivot: a 3-tuple,
        the point the map is applied about; measure: the buffer a measure_records call wrote, whose centre is the pivot — computed on the device,
        nothing is read back.  Passing both is an error.  With the bits of transform_selected_host.  A full write of data: the next draw rebuilds
        its SoA shadow.  Per frame: (shade_sh), (edit), transform_selected, keygen, sort, draw.  Asynchronous."""
        if stats is None and rule:
            raise TypeError("transform_selected: a rule without stats")
        if pivot is not None and measure is not None:
            raise TypeError("transform_selected: pivot and measure exclude each other")
        if isinstance(xf, SelectionXf):
            if pivot is not None:
                raise TypeError("transform_selected: a SelectionXf carries its own pivot")
            x = xf
        else:
            x = selection_xf(xf, pivot, measure is not None)
        k = _keep_rule(**rule) if stats is not None else None
        self._chk(_lib.gs4d_transform_selected(self._h, int(data), int(n), C.byref(x), int(stats or 0), _ptr(k) if k is not None else None, int(measure or 0)))

    def write_tensor(self, buf, tensor, offset=0):
        """A contiguous device tensor copied into the buffer `buf` at byte `offset`, with no host copy and no host synchronisation: the
        contract of gs4d_buffer_device_ptr — gs4d_buffer_invalidate, then an asynchronous device-to-device copy on the tensor's current
        stream, which the caller has named with set_stream (the legacy default stream cannot be named: run under a stream of your own).  The
        library's next call that uses the buffer is ordered behind the copy."""
        import torch                                             # lazily: the package imports without torch
        if not (isinstance(tensor, torch.Tensor) and tensor.is_cuda and tensor.is_contiguous()):
            raise ValueError("write_tensor: expected a contiguous device tensor")
        stream = torch.cuda.current_stream(tensor.device).cuda_stream
        if not stream or stream != getattr(self, "_stream", None):
            raise Gs4dError("write_tensor: name the tensor's current stream with set_stream first (a stream of your own, not the default stream)")
        nbytes = tensor.numel() * tensor.element_size()
        dptr, size = self.device_ptr(buf)
        if offset < 0 or offset + nbytes > size:
            raise ValueError(f"write_tensor: {nbytes} bytes at offset {offset} do not fit a buffer of {size} bytes")
        if nbytes == 0:
            return
        self.invalidate(buf)
        rc = _hip().hipMemcpyAsync(C.c_void_p(dptr + offset), C.c_void_p(tensor.data_ptr()), nbytes, 3, C.c_void_p(stream))      # 3: hipMemcpyDeviceToDevice
        if rc != 0:
            raise Gs4dError(f"write_tensor: hipMemcpyAsync failed ({rc})")

    def read_tensor(self, buf, tensor, offset=0):
        """The other direction: the bytes of the buffer `buf` from byte `offset` copied into a contiguous device tensor, with no host copy and no
        host synchronisation — gs4d_buffer_invalidate makes the tensor's current stream (named with set_stream, as for write_tensor) wait for the
        kernels the library has queued on the buffer, e.g. a decompose_records that writes it; the copy runs on that stream behind them."""
        import torch
        if not (isinstance(tensor, torch.Tensor) and tensor.is_cuda and tensor.is_contiguous()):
            raise ValueError("read_tensor: expected a contiguous device tensor")
        stream = torch.cuda.current_stream(tensor.device).cuda_stream
        if not stream or stream != getattr(self, "_stream", None):
            raise Gs4dError("read_tensor: name the tensor's current stream with set_stream first (a stream of your own, not the default stream)")
        nbytes = tensor.numel() * tensor.element_size()
        dptr, size = self.device_ptr(buf)
        if offset < 0 or offset + nbytes > size:
            raise ValueError(f"read_tensor: {nbytes} bytes at offset {offset} are not inside a buffer of {size} bytes")
        if nbytes == 0:
            return
        self.invalidate(buf)
        rc = _hip().hipMemcpyAsync(C.c_void_p(tensor.data_ptr()), C.c_void_p(dptr + offset), nbytes, 3, C.c_void_p(stream))      # 3: hipMemcpyDeviceToDevice
        if rc != 0:
            raise Gs4dError(f"read_tensor: hipMemcpyAsync failed ({rc})")

    def shadow_builds(self, buf):
        """gs4d_debug_shadow_builds: how many times the SoA shadow of this record buffer has been (re)built."""
        n = C.c_uint64(0)
        self._chk(_lib.gs4d_debug_shadow_builds(self._h, int(buf), C.byref(n)))
        return n.value

    def set_tile_shard(self, rank, world):
        """Single-frame sharding: this context bins and composites the tile rows ty % world == rank only."""
        self._chk(_lib.gs4d_set_tile_shard(self._h, rank, world))

    def band_rows(self):
        n = C.c_int(0)
        self._chk(_lib.gs4d_band_rows(self._h, C.byref(n)))
        return n.value

    def read_band_rgba8_device(self, dptr, nbytes):
        self._chk(_lib.gs4d_read_band_rgba8_device(self._h, C.c_void_p(dptr), nbytes))

    def set_stream(self, hip_stream):
        self._chk(_lib.gs4d_set_stream(self._h, C.c_void_p(hip_stream) if hip_stream else None))
        self._stream = hip_stream or None

    def finish(self):
        self._chk(_lib.gs4d_finish(self._h))

    # measurement
    def set_profiling(self, on, every=1):
        """False: off; True: every stage; an iterable of stage names: only those.  every=k: time only every k-th frame (each timed stage
        costs two event records in a timed frame)."""
        if isinstance(on, (list, tuple, set)):
            mask = 0
            for name in on:
                mask |= 1 << STAGES.index(name)
        else:
            mask = 0x3F if on else 0
        self._chk(_lib.gs4d_set_profiling(self._h, mask | ((int(every) & 0xFF) << 8 if mask and every > 1 else 0)))

    def timings(self):
        ms = np.zeros(len(STAGES), np.float32)
        self._chk(_lib.gs4d_get_timings(self._h, _ptr(ms)))
        return dict(zip(STAGES, (float(x) for x in ms)))

    def timeline(self, max_frames=128):
        """[frames, stages, 2] start/end (ms since the first timed stage of frame 0) of the frames recorded so far; -1 where not run."""
        ms = np.full((max_frames, len(STAGES), 2), -1.0, np.float32)
        n = C.c_int(0)
        self._chk(_lib.gs4d_get_timeline(self._h, _ptr(ms), max_frames, C.byref(n)))
        return ms[:n.value]

    def stats(self):
        st = np.zeros(8, np.uint64)
        self._chk(_lib.gs4d_get_stats(self._h, _ptr(st)))
        return {"entries": int(st[0]) & 0xFFFFFFFF, "staged_draws": int(st[0]) >> 32, "capacity": int(st[1]) & 0xFFFFFFFFFF, "staged_misses": int(st[1]) >> 40, "reruns": int(st[2]) & 0xFFFFFFFF, "aborted_discarded": int(st[2]) >> 32, "tiles": int(st[3]) & 0xFFFFFFFF, "record_read_bytes": (int(st[3]) >> 32) & 0xFF, "composited_tiles": int(st[3]) >> 40,
                "depth_sort_passes": int(st[4]) & 0xFFFFFFFF, "lane_streams_rejected": int(st[4]) >> 32, "tile_sort_passes": int(st[5]) & 0xFFFFFFFF, "renamed_keygens": int(st[5]) >> 32, "lanes": int(st[6]) & 0xFFFF, "lanes_sharing_a_queue": (int(st[6]) >> 16) & 0xFFFF, "fused_keygen_draws": int(st[6]) >> 32,
                "unordered_draws": int(st[7]) & 0xFFFFFFFF, "longest_list": int(st[7]) >> 32}

    def sort_stats(self):
        """The depth sorts so far (gs4d_get_sort_stats; waits for everything queued): hybrid sorts, sort kernel launches, and the latest
        top-digit report: its largest bucket and its buckets above the tail's capacity."""
        st = np.zeros(4, np.uint64)
        self._chk(_lib.gs4d_get_sort_stats(self._h, _ptr(st)))
        return {"hybrid_sorts": int(st[0]), "sort_launches": int(st[1]), "largest_bucket": int(st[2]), "slow_buckets": int(st[3])}

    def debug_projected(self, n):
        out = np.empty((n, 16), np.float32)
        self._chk(_lib.gs4d_debug_read_projected(self._h, _ptr(out), n))
        return out


def record_weight_sum(stats):
    """wsum of read_record_stats in weight units (float64): the summed weight with which each record entered the colour."""
    return np.asarray(stats["wsum"], np.uint64).astype(np.float64) * 2.0 ** -24


def version():
    return _lib.gs4d_version().decode()
