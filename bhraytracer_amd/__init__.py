"""bhraytracer_amd — ctypes binding of libbhrt.so (include/bhrt.h).

Plumbing only: the product is the C-ABI library (host front-end in C++ + hand-written gfx950
HIP kernels).  This module loads it for the tests, bench.py and tools, and fails loudly when
the library has not been built — there is no Python or CPU fallback for the render path.
"""
import ctypes as C
import os

import numpy as np

from .flat import FlatView

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("BHRT_LIB") or os.path.join(_HERE, "libbhrt.so")  # BHRT_LIB: load another build of the same ABI

SIDE_FRONT, SIDE_BACK, SIDE_BOTH = 1, 2, 3


class BhrtError(RuntimeError):
    pass


class Info(C.Structure):
    _fields_ = [("width", C.c_int32), ("height", C.c_int32)] + [
        (n, C.c_uint32) for n in ("n_nodes", "n_meshes", "n_triangles", "n_bvh_nodes", "n_materials", "n_lights",
                                  "n_textures", "max_node_depth", "max_bvh_depth")] + [
        ("flat_bytes", C.c_uint64), ("n_warnings", C.c_uint32)]


class Opts(C.Structure):
    _fields_ = [("spp", C.c_int32), ("gi_bounces", C.c_int32), ("internal_bounces", C.c_int32), ("seed", C.c_uint32),
                ("jitter", C.c_int32), ("gamma", C.c_int32), ("photon_map", C.c_int32),
                ("rank", C.c_int32), ("world_size", C.c_int32), ("tile_size", C.c_int32),
                ("samples_per_pass", C.c_int32), ("timers", C.c_int32), ("photon_exact", C.c_int32), ("leaf_skip", C.c_int32), ("photon_radius", C.c_float), ("lens", C.c_int32)]


class Stats(C.Structure):
    _fields_ = [("closest_rays", C.c_uint64), ("shadow_rays", C.c_uint64), ("shade_calls", C.c_uint64),
                ("camera_samples", C.c_uint64), ("passes", C.c_uint32), ("wave_iterations", C.c_uint32),
                ("seconds_total", C.c_double), ("seconds_trace_closest", C.c_double),
                ("seconds_trace_shadow", C.c_double), ("seconds_shade", C.c_double), ("seconds_other", C.c_double),
                ("launches_trace_closest", C.c_uint64), ("launches_trace_shadow", C.c_uint64),
                ("seconds_photon_gather", C.c_double), ("seconds_photon_heavy", C.c_double),
                ("photon_queries", C.c_uint64), ("photon_heavy_queries", C.c_uint64), ("photon_wave_queries", C.c_uint64),
                ("photon_exact_queries", C.c_uint64), ("photon_nodes_visited", C.c_uint64), ("deferred_rays", C.c_uint64),
                ("photon_lane_queries", C.c_uint64), ("photon_lane_nodes", C.c_uint64), ("photon_found", C.c_uint64), ("launches_resolve_fused", C.c_uint64),
                ("global_gather_queries", C.c_uint64), ("global_gather_heavy_queries", C.c_uint64), ("seconds_global_gather", C.c_double)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_ if n != "reserved"}


class DenoiseOpts(C.Structure):
    """bhrt_denoise_opts: the a-trous denoiser's levels, guide tolerances and output gamma (csrc/denoise.hip states the filter)."""
    _fields_ = [("iterations", C.c_int32), ("sigma_normal", C.c_float), ("sigma_depth", C.c_float), ("sigma_luminance", C.c_float),
                ("gamma", C.c_int32), ("reserved", C.c_int32 * 3)]


class AdaptiveOpts(C.Structure):
    """bhrt_adaptive_opts: round-0 samples, the retirement threshold and its luminance floor (include/bhrt.h states the rounds and the test)."""
    _fields_ = [("min_spp", C.c_int32), ("threshold", C.c_float), ("floor", C.c_float), ("reserved", C.c_int32 * 5)]


class Progress(C.Structure):
    """bhrt_progress: where a progressive session stands (bhrt_progressive_status)."""
    _fields_ = [("steps", C.c_uint32), ("spp_min", C.c_uint32), ("spp_max", C.c_uint32), ("active_pixels", C.c_uint64),
                ("camera_samples", C.c_uint64), ("finished", C.c_int32), ("reserved", C.c_int32 * 3)]


class ReprojectOpts(C.Structure):
    """bhrt_reproject_opts: when a tap of the previous view counts as the same surface (csrc/temporal.hip states the stage)."""
    _fields_ = [("depth_tolerance", C.c_float), ("normal_threshold", C.c_float), ("reserved", C.c_int32 * 6)]


class TemporalOpts(C.Structure):
    """bhrt_temporal_opts: the history clamp, the longest history and the output gamma of bhrt_temporal_accumulate (csrc/temporal.hip)."""
    _fields_ = [("clamp_k", C.c_float), ("max_length", C.c_float), ("gamma", C.c_int32), ("reserved", C.c_int32 * 5)]


class SpatialVarianceOpts(C.Structure):
    """bhrt_spatial_variance_opts: the window, the edge stops and the pass-through length of bhrt_variance_spatial (csrc/temporal.hip, stage 3S)."""
    _fields_ = [("radius", C.c_int32), ("depth_tolerance", C.c_float), ("normal_threshold", C.c_float), ("min_length", C.c_float), ("demodulate", C.c_int32),
                ("reserved", C.c_int32 * 3)]


class ChangeOpts(C.Structure):
    """bhrt_change_opts: the window, the two thresholds and the edge stops of bhrt_temporal_change (csrc/temporal.hip, stage 2C)."""
    _fields_ = [("radius", C.c_int32), ("sigma_lo", C.c_float), ("sigma_hi", C.c_float), ("depth_tolerance", C.c_float), ("normal_threshold", C.c_float),
                ("reserved", C.c_int32 * 3)]


class UpsampleOpts(C.Structure):
    """bhrt_upsample_opts: the edge stops, the demodulation switch and the output gamma of bhrt_upsample (csrc/upsample.hip, stage 4U).
    `fallback` (UPSAMPLE_FALLBACK_*) is the header's field in the place of reserved[0]; the header's reserved[3] is reserved[1:] here."""
    _fields_ = [("depth_tolerance", C.c_float), ("normal_threshold", C.c_float), ("demodulate", C.c_int32), ("gamma", C.c_int32), ("reserved", C.c_int32 * 4)]

    @property
    def fallback(self) -> int:
        return self.reserved[0]

    @fallback.setter
    def fallback(self, value: int):
        self.reserved[0] = value


class TemporalSessionOpts(C.Structure):
    """bhrt_temporal_session_opts: the four stages' options and the four switches of a temporal session (include/bhrt.h)."""
    _fields_ = [("reproject", ReprojectOpts), ("temporal", TemporalOpts), ("spatial", SpatialVarianceOpts), ("denoise_opts", DenoiseOpts),
                ("carry_variance", C.c_int32), ("spatial_variance", C.c_int32), ("denoise", C.c_int32), ("follow_nodes", C.c_int32),
                ("reserved", C.c_int32 * 4)]


class TemporalProgress(C.Structure):
    """bhrt_temporal_progress: where a temporal session stands (bhrt_temporal_status)."""
    _fields_ = [("frames", C.c_uint32), ("failed", C.c_int32), ("history_pixels", C.c_uint64), ("pixels", C.c_uint64), ("reserved", C.c_int32 * 4)]


# BHRT_TEMPORAL_IMG_* of include/bhrt.h: the images a temporal session keeps, with their element type and channels
(TEMPORAL_IMG_ACCUMULATED, TEMPORAL_IMG_VARIANCE, TEMPORAL_IMG_LENGTH, TEMPORAL_IMG_HISTORY_LENGTH, TEMPORAL_IMG_FILTER_VARIANCE, TEMPORAL_IMG_Z,
 TEMPORAL_IMG_NORMAL, TEMPORAL_IMG_ALBEDO, TEMPORAL_IMG_NODE, TEMPORAL_IMG_CURRENT, TEMPORAL_IMG_CURRENT_VARIANCE, TEMPORAL_IMG_CHANGE,
 TEMPORAL_IMG_USED_LENGTH) = range(13)
_TEMPORAL_IMG_ONE_CHANNEL = (TEMPORAL_IMG_LENGTH, TEMPORAL_IMG_HISTORY_LENGTH, TEMPORAL_IMG_Z, TEMPORAL_IMG_NODE, TEMPORAL_IMG_CHANGE, TEMPORAL_IMG_USED_LENGTH)


class XformOp(C.Structure):
    """bhrt_xform_op: one <scale> / <rotate> / <translate> of bhrt_scene_set_node_transform."""
    _fields_ = [("kind", C.c_int32), ("v", C.c_float * 4)]


XFORM_SCALE, XFORM_ROTATE, XFORM_TRANSLATE = 0, 1, 2
# a node's bhrt_xform as a numpy record: tm (9, column-major), pos (3), itm (9); 84 bytes
XFORM_DTYPE = np.dtype([("tm", np.float32, 9), ("pos", np.float32, 3), ("itm", np.float32, 9)])


def scale(x, y, z):
    return XformOp(XFORM_SCALE, (x, y, z, 0.0))


def rotate(x, y, z, degrees):
    return XformOp(XFORM_ROTATE, (x, y, z, degrees))


def translate(x, y, z):
    return XformOp(XFORM_TRANSLATE, (x, y, z, 0.0))


class LightInfo(C.Structure):
    """bhrt_light_info: one light of a loaded scene as the loader read it, and where it stands in the blob's sorted lights[]."""
    _fields_ = [("type", C.c_int32), ("intensity", C.c_float * 3), ("vec", C.c_float * 3), ("size", C.c_float), ("blob_index", C.c_int32),
                ("reserved", C.c_int32 * 5)]


# BHRT_LIGHT_* of include/bhrt_flat.h
LIGHT_AMBIENT, LIGHT_DIRECT, LIGHT_POINT = 0, 1, 2


class Hits(C.Structure):
    _fields_ = [("t", C.c_void_p), ("node", C.c_void_p), ("prim", C.c_void_p), ("front", C.c_void_p)]


_lib = None

# every symbol include/bhrt.h declares
EXPORTS = [
    "bhrt_last_error", "bhrt_default_opts", "bhrt_scene_load_xml", "bhrt_scene_free", "bhrt_scene_info",
    "bhrt_scene_warning", "bhrt_scene_flat", "bhrt_scene_upload", "bhrt_device_count",
    "bhrt_trace_closest_host", "bhrt_trace_closest_dev", "bhrt_trace_shadow_host", "bhrt_trace_shadow_dev",
    "bhrt_render", "bhrt_render_dev", "bhrt_render_samples", "bhrt_photon_build", "bhrt_photon_gather_host",
    "bhrt_photon_get", "bhrt_photon_export", "bhrt_photon_import", "bhrt_photon_build_global", "bhrt_save_png", "bhrt_math_eval_dev",
    "bhrt_tiles_block_bytes", "bhrt_tiles_pack_dev", "bhrt_tiles_unpack_dev",
    "bhrt_first_hit", "bhrt_first_hit_dev", "bhrt_zbuffer_image_dev", "bhrt_color_image_dev",
    "bhrt_scene_load_xml_ex", "bhrt_bvh_build", "bhrt_photon_emit_range", "bhrt_photon_install", "bhrt_scene_clone", "bhrt_host_alloc", "bhrt_host_free", "bhrt_photon_gather_host_ex", "bhrt_scene_knob",
    "bhrt_default_denoise_opts", "bhrt_render_var", "bhrt_render_var_dev", "bhrt_denoise", "bhrt_denoise_dev",
    "bhrt_default_adaptive_opts", "bhrt_render_adaptive", "bhrt_render_adaptive_dev", "bhrt_sample_count_image", "bhrt_sample_count_image_dev",
    "bhrt_save_png_gray",
    "bhrt_scene_set_lens", "bhrt_camera_rays",
    "bhrt_scene_set_emissive", "bhrt_scene_material_index", "bhrt_scene_set_material_emission", "bhrt_scene_get_material_emission",
    "bhrt_scene_set_face_materials", "bhrt_scene_submaterial_count", "bhrt_scene_get_submaterial",
    "bhrt_scene_set_global_gather", "bhrt_global_map_build", "bhrt_global_map_set", "bhrt_global_map_get", "bhrt_global_gather_host",
    "bhrt_progressive_begin", "bhrt_progressive_step", "bhrt_progressive_frame", "bhrt_progressive_frame_dev", "bhrt_progressive_status",
    "bhrt_progressive_end",
    "bhrt_guides", "bhrt_guides_dev",
    "bhrt_denoise_sampled", "bhrt_denoise_sampled_dev",
    "bhrt_scene_set_camera", "bhrt_scene_set_shutter", "bhrt_scene_get_shutter",
    "bhrt_scene_get_camera_frame", "bhrt_default_reproject_opts", "bhrt_default_temporal_opts",
    "bhrt_reproject", "bhrt_reproject_dev", "bhrt_temporal_accumulate", "bhrt_temporal_accumulate_dev",
    "bhrt_scene_node_index", "bhrt_scene_get_node_transform", "bhrt_scene_get_node_transforms", "bhrt_scene_set_node_transform",
    "bhrt_first_hit_node", "bhrt_first_hit_node_dev", "bhrt_reproject_moving", "bhrt_reproject_moving_dev",
    "bhrt_reproject_var", "bhrt_reproject_var_dev", "bhrt_temporal_accumulate_var", "bhrt_temporal_accumulate_var_dev",
    "bhrt_default_spatial_variance_opts", "bhrt_variance_spatial", "bhrt_variance_spatial_dev",
    "bhrt_first_hit_ex", "bhrt_first_hit_ex_dev",
    "bhrt_default_temporal_session_opts", "bhrt_temporal_begin", "bhrt_temporal_frame", "bhrt_temporal_frame_dev", "bhrt_temporal_reset",
    "bhrt_temporal_status", "bhrt_temporal_image", "bhrt_temporal_image_dev", "bhrt_temporal_end",
    "bhrt_default_change_opts", "bhrt_temporal_change", "bhrt_temporal_change_dev", "bhrt_temporal_set_change",
    "bhrt_scene_set_resolution", "bhrt_default_upsample_opts", "bhrt_upsample", "bhrt_upsample_dev",
    "bhrt_scene_light_count", "bhrt_scene_light_index", "bhrt_scene_get_light", "bhrt_scene_set_light",
]

# BHRT_UPSAMPLE_FALLBACK_* of include/bhrt.h: what a pixel no tap passes takes from its taps
UPSAMPLE_FALLBACK_ALBEDO, UPSAMPLE_FALLBACK_LIGHT = 0, 1
# BHRT_DENOISE_SIGMA_COVERAGE of include/bhrt.h: the default coverage tolerance of the denoiser for sampled guides
DENOISE_SIGMA_COVERAGE = 0.5
# BHRT_REPROJECT_* and BHRT_TEMPORAL_* of include/bhrt.h: the measured defaults of temporal reprojection
REPROJECT_DEPTH_TOLERANCE = 0.01
REPROJECT_NORMAL_THRESHOLD = 0.99
TEMPORAL_CLAMP_K = 1.0
TEMPORAL_MAX_LENGTH = 16.0
# BHRT_CHANGE_SIGMA_* of include/bhrt.h: the measured thresholds of the temporal change test
CHANGE_SIGMA_LO = 3.0
CHANGE_SIGMA_HI = 6.0


def lib():
    """Loads libbhrt.so; raises if it is missing (run `python -m bhraytracer_amd.build` first)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise BhrtError(f"{LIB_PATH} not found: build it with `python -m bhraytracer_amd.build` "
                            "(the render path has no fallback)")
        # torch ships its own libamdhip64 under the SONAME of the system's: whichever copy a process loads first serves
        # both.  Two HIP runtimes in one process do not both see the GPU, so when torch is present (tests, bench.py:
        # device tensors, torch.distributed) it goes first.  The library itself does not depend on torch.
        import sys
        if "torch" not in sys.modules:
            try:
                import torch  # noqa: F401
            except Exception:
                pass
        L = C.CDLL(LIB_PATH)
        L.bhrt_last_error.restype = C.c_char_p
        L.bhrt_scene_free.restype = None
        L.bhrt_default_opts.restype = None
        L.bhrt_default_denoise_opts.restype = None
        L.bhrt_default_adaptive_opts.restype = None
        L.bhrt_default_reproject_opts.restype = None
        L.bhrt_default_temporal_opts.restype = None
        L.bhrt_default_spatial_variance_opts.restype = None
        L.bhrt_default_temporal_session_opts.restype = None
        L.bhrt_default_change_opts.restype = None
        L.bhrt_default_upsample_opts.restype = None
        _lib = L
    return _lib


def _check(rc):
    if rc != 0:
        raise BhrtError(f"bhrt error {rc}: {lib().bhrt_last_error().decode(errors='replace')}")


def default_opts(**kw) -> Opts:
    o = Opts()
    lib().bhrt_default_opts(C.byref(o))
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def default_denoise_opts(**kw) -> DenoiseOpts:
    """bhrt_default_denoise_opts (K = 4, sigma_normal = 32, sigma_depth = 0.01, sigma_luminance = 4, gamma = 1), fields overridden by kw."""
    o = DenoiseOpts()
    lib().bhrt_default_denoise_opts(C.byref(o))
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def default_adaptive_opts(**kw) -> AdaptiveOpts:
    """bhrt_default_adaptive_opts (min_spp = 16, threshold and floor from DESIGN.md 10), fields overridden by kw."""
    o = AdaptiveOpts()
    lib().bhrt_default_adaptive_opts(C.byref(o))
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def default_reproject_opts(**kw) -> ReprojectOpts:
    """bhrt_default_reproject_opts (depth_tolerance, normal_threshold: DESIGN.md 19), fields overridden by kw."""
    o = ReprojectOpts()
    lib().bhrt_default_reproject_opts(C.byref(o))
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def default_temporal_opts(**kw) -> TemporalOpts:
    """bhrt_default_temporal_opts (clamp_k, max_length: DESIGN.md 19; gamma = 1), fields overridden by kw."""
    o = TemporalOpts()
    lib().bhrt_default_temporal_opts(C.byref(o))
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def default_spatial_variance_opts(**kw) -> SpatialVarianceOpts:
    """bhrt_default_spatial_variance_opts (radius 3, depth_tolerance 0.01, normal_threshold 0.99, min_length 4, demodulate 1: DESIGN.md 22), fields overridden by kw."""
    o = SpatialVarianceOpts()
    lib().bhrt_default_spatial_variance_opts(C.byref(o))
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def default_change_opts(**kw) -> ChangeOpts:
    """bhrt_default_change_opts (radius 3, sigma_lo and sigma_hi from DESIGN.md 24, depth_tolerance 0.01, normal_threshold 0.99), fields overridden by kw."""
    o = ChangeOpts()
    lib().bhrt_default_change_opts(C.byref(o))
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def default_upsample_opts(**kw) -> UpsampleOpts:
    """bhrt_default_upsample_opts (depth_tolerance 0.01, normal_threshold 0.99, demodulate 1, gamma 1, fallback UPSAMPLE_FALLBACK_ALBEDO: DESIGN.md 25), fields
    overridden by kw."""
    o = UpsampleOpts()
    lib().bhrt_default_upsample_opts(C.byref(o))
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def default_temporal_session_opts(**kw) -> TemporalSessionOpts:
    """bhrt_default_temporal_session_opts (the four stages' defaults, the four switches 0), fields overridden by kw."""
    o = TemporalSessionOpts()
    lib().bhrt_default_temporal_session_opts(C.byref(o))
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def device_count() -> int:
    n = C.c_int(0)
    rc = lib().bhrt_device_count(C.byref(n))
    return n.value if rc == 0 else 0


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


class Scene:
    """A loaded scene = the reference's LoadScene() globals behind one handle (Main.cpp:17-37,43)."""

    def __init__(self, xml_path: str, bvh_device: int = -1):
        """bvh_device >= 0: mesh BVHs are built on that HIP device (bhrt_scene_load_xml_ex) instead of by the host front-end."""
        self._h = C.c_void_p()
        _check(lib().bhrt_scene_load_xml_ex(os.fsencode(xml_path), int(bvh_device), C.byref(self._h)))
        self.info = Info()
        _check(lib().bhrt_scene_info(self._h, C.byref(self.info)))
        self._flat = None

    def close(self):
        """bhrt_scene_free: the scene, its device state and an open progressive session with it."""
        if self._h:
            lib().bhrt_scene_free(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def width(self):
        return self.info.width

    @property
    def height(self):
        return self.info.height

    def warnings(self):
        out = []
        for i in range(self.info.n_warnings):
            s = C.c_char_p()
            _check(lib().bhrt_scene_warning(self._h, i, C.byref(s)))
            out.append(s.value.decode(errors="replace"))
        return out

    def flat_bytes(self) -> bytes:
        if self._flat is None:
            p, n = C.c_void_p(), C.c_uint64()
            _check(lib().bhrt_scene_flat(self._h, C.byref(p), C.byref(n)))
            self._flat = C.string_at(p, n.value)
        return self._flat

    def flat_view(self) -> FlatView:
        return FlatView(self.flat_bytes())

    def upload(self, device: int = 0):
        _check(lib().bhrt_scene_upload(self._h, device))

    def set_lens(self, focaldist: float = 0.0, dof: float = 0.0):
        """bhrt_scene_set_lens: the camera's <focaldist> (<= 0 keeps the current one) and <dof> of the loaded scene; the camera frame is derived
        again, and an uploaded scene's camera is refreshed.  Opts.lens = 1 then renders through a thin lens of aperture radius dof."""
        _check(lib().bhrt_scene_set_lens(self._h, C.c_float(focaldist), C.c_float(dof)))
        self._flat = None

    def set_resolution(self, width: int, height: int):
        """bhrt_scene_set_resolution: the camera's <width> and <height> of the loaded scene; the camera frame (and pose 1 of an active shutter) is
        derived again, the blob becomes that of the edited scene file, and an uploaded scene's camera is refreshed.  Refused while a progressive
        or temporal session is open."""
        _check(lib().bhrt_scene_set_resolution(self._h, C.c_int32(width), C.c_int32(height)))
        _check(lib().bhrt_scene_info(self._h, C.byref(self.info)))
        self._flat = None

    # ---- the camera and its shutter ---------------------------------------------------------------------------------------
    def set_camera(self, pos, target, up, fov: float = 0.0):
        """bhrt_scene_set_camera: the camera's <position>, <target>, <up> and <fov> (<= 0 keeps the current one) of the loaded scene, through
        the loader's own operations; the blob becomes that of the edited scene file, and an uploaded scene's camera is refreshed."""
        v = [None if a is None else (C.c_float * 3)(*[float(x) for x in a]) for a in (pos, target, up)]
        _check(lib().bhrt_scene_set_camera(self._h, v[0], v[1], v[2], C.c_float(fov)))
        self._flat = None

    def set_shutter(self, on: bool = True, pos1=None, target1=None, up1=None):
        """bhrt_scene_set_shutter: camera motion blur between the scene's camera (pose 0) and (pos1, target1, up1), the camera at the end of the
        exposure; every camera sample draws its own time in [0, 1).  on = False clears the state.  The blob keeps its bytes."""
        v = [None if a is None else (C.c_float * 3)(*[float(x) for x in a]) for a in (pos1, target1, up1)]
        _check(lib().bhrt_scene_set_shutter(self._h, 1 if on else 0, v[0], v[1], v[2]))

    def shutter(self):
        """bhrt_scene_get_shutter: (on, pose1 (3, 3) float32 = pos1, target1, up1 as given, frame1 (4, 3) float32 = pos1, top_left1, dd_x1,
        dd_y1 as derived)."""
        on = C.c_int(0)
        pose, frame = np.zeros((3, 3), np.float32), np.zeros((4, 3), np.float32)
        _check(lib().bhrt_scene_get_shutter(self._h, C.byref(on), _ptr(pose), _ptr(frame)))
        return bool(on.value), pose, frame

    # ---- moving objects: node names and transforms ------------------------------------------------------------------------
    def node_index(self, name: str) -> int:
        """bhrt_scene_node_index: the first node named `name` in the blob's pre-order (BhrtError, BHRT_ERR_ARG, when there is none)."""
        i = C.c_int32(-1)
        _check(lib().bhrt_scene_node_index(self._h, None if name is None else name.encode(), C.byref(i)))
        return i.value

    def node_transform(self, node: int):
        """bhrt_scene_get_node_transform: the blob's record of that node, a numpy record of XFORM_DTYPE (tm, pos, itm)."""
        out = np.zeros(1, XFORM_DTYPE)
        _check(lib().bhrt_scene_get_node_transform(self._h, int(node), _ptr(out)))
        return out[0]

    def node_transforms(self):
        """bhrt_scene_get_node_transforms: all n_nodes records, (n_nodes,) of XFORM_DTYPE: the snapshot reproject_moving reads."""
        out = np.zeros(max(self.info.n_nodes, 1), XFORM_DTYPE)
        n = C.c_uint32(0)
        _check(lib().bhrt_scene_get_node_transforms(self._h, _ptr(out), C.c_uint32(out.shape[0]), C.byref(n)))
        return out[:n.value].copy()

    def set_node_transform(self, node: int, tm=None, pos=None, ops=()):
        """bhrt_scene_set_node_transform: start from (tm, pos) (both None: the identity), apply the ops (scale(), rotate(), translate() of this
        module) in order with the loader's own operations; the blob becomes that of the edited scene file, and an uploaded scene's node and camera
        chain are refreshed.  Restoring a saved record r: set_node_transform(node, r["tm"], r["pos"])."""
        v = [None if a is None else (C.c_float * k)(*[float(x) for x in np.asarray(a).reshape(-1)]) for a, k in ((tm, 9), (pos, 3))]
        arr = None if ops is None else (XformOp * max(len(ops), 1))(*ops)
        _check(lib().bhrt_scene_set_node_transform(self._h, int(node), v[0], v[1], arr, C.c_uint32(0 if ops is None else len(ops))))
        self._flat = None

    # ---- lights: named by their index in document order; the blob holds them sorted by Gray() -----------------------------
    def light_count(self) -> int:
        """bhrt_scene_light_count: the number of lights."""
        n = C.c_int32(-1)
        _check(lib().bhrt_scene_light_count(self._h, C.byref(n)))
        return n.value

    def light_index(self, name: str) -> int:
        """bhrt_scene_light_index: the first light named `name` in document order (BhrtError, BHRT_ERR_ARG, when there is none)."""
        i = C.c_int32(-1)
        _check(lib().bhrt_scene_light_index(self._h, None if name is None else name.encode(), C.byref(i)))
        return i.value

    def light(self, light: int) -> LightInfo:
        """bhrt_scene_get_light: the light as the loader read it (type, intensity, vec, size) and its blob_index."""
        out = LightInfo()
        _check(lib().bhrt_scene_get_light(self._h, int(light), C.byref(out)))
        return out

    def set_light(self, light: int, intensity=None, vec=None, size: float = -1.0):
        """bhrt_scene_set_light: None keeps the intensity / the position or direction, size < 0 the size; the loader's own sort and sum run
        again, the blob becomes that of the edited scene file, and an uploaded scene's lights, pick table and summed intensity are refreshed."""
        v = [None if a is None else (C.c_float * 3)(*[float(x) for x in a]) for a in (intensity, vec)]
        _check(lib().bhrt_scene_set_light(self._h, int(light), v[0], v[1], C.c_float(size)))
        self._flat = None

    # ---- the emission term: scene state beside the flat blob, which keeps its bytes --------------------
    def set_emissive(self, on: bool = True):
        """bhrt_scene_set_emissive: with the term on, every Shade() frame of a Blinn material adds its <emission> (colour x optional texture) last,
        at every bounce, in all later renders of this scene.  Off by default: the reference parses <emission> and never shades it."""
        _check(lib().bhrt_scene_set_emissive(self._h, 1 if on else 0))

    def material_index(self, name: str) -> int:
        """bhrt_scene_material_index: the index of the XML material `name` (BhrtError, BHRT_ERR_ARG, when there is none)."""
        i = C.c_int32(-1)
        _check(lib().bhrt_scene_material_index(self._h, name.encode(), C.byref(i)))
        return i.value

    def set_material_emission(self, material: int, rgb):
        """bhrt_scene_set_material_emission: a plain emission colour for material `material` (any map is dropped); refreshes an uploaded scene."""
        c = (C.c_float * 3)(*[float(x) for x in rgb])
        _check(lib().bhrt_scene_set_material_emission(self._h, int(material), c))

    def material_emission(self, material: int):
        """bhrt_scene_get_material_emission: ((r, g, b), texmap) — the colour and the index into the blob's texmaps[] (-1 = plain colour)."""
        c = (C.c_float * 3)()
        m = C.c_int32(-1)
        _check(lib().bhrt_scene_get_material_emission(self._h, int(material), c, C.byref(m)))
        return (c[0], c[1], c[2]), m.value

    # ---- face materials: scene state beside the flat blob, which keeps its bytes ---------------------------------------------
    def set_face_materials(self, on: bool = True):
        """bhrt_scene_set_face_materials: with the switch on, a hit of a node whose material is a MultiMtl (an OBJ with a .mtl) shades with the
        sub-material of the face that was hit, in all later renders and first-hit images of this scene.  Off by default: the reference shades
        the whole mesh with sub-material 0."""
        _check(lib().bhrt_scene_set_face_materials(self._h, 1 if on else 0))

    def submaterial_count(self, material: int) -> int:
        """bhrt_scene_submaterial_count: the number of sub-materials of material `material`; 0 for one that is not a MultiMtl."""
        n = C.c_int32(0)
        _check(lib().bhrt_scene_submaterial_count(self._h, int(material), C.byref(n)))
        return n.value

    def submaterial(self, material: int, sub: int):
        """bhrt_scene_get_submaterial: (record, face_end) — sub-material `sub` of material `material` as a flat.Material (the layout of the
        blob's materials; bytes(record) are its bytes) and the end of its face range: faces [face_end of sub - 1, face_end) shade with it."""
        from .flat import Material
        m = Material()
        e = C.c_uint32(0)
        _check(lib().bhrt_scene_get_submaterial(self._h, int(material), int(sub), C.byref(m), C.byref(e)))
        return m, e.value

    # ---- the global gather: switch and radius beside the flat blob, the map in a device slot of its own ----------------------
    def set_global_gather(self, on: bool = True, radius: float = 0.0):
        """bhrt_scene_set_global_gather: with the switch on, a Shade() frame whose GI term is cut by gi < 0 gathers it from the installed global
        map instead (diffuse x EstimateIrradiance<1000>), in all later renders of this scene.  radius 0 = the reference's 0.5.  The renders
        raise (BHRT_ERR_ARG) while the switch is on and no global map is installed."""
        _check(lib().bhrt_scene_set_global_gather(self._h, 1 if on else 0, C.c_float(radius)))

    def global_map_build(self, opts: Opts, max_photons: int) -> int:
        """bhrt_global_map_build: BuildPhotonMap on the device, balanced and left installed for the global gather; returns the photons stored."""
        n = C.c_uint32(0)
        _check(lib().bhrt_global_map_build(self._h, C.byref(opts), int(max_photons), C.byref(n)))
        return n.value

    def global_map_set(self, records) -> int:
        """bhrt_global_map_set: installs balanced (n, 24) uint8 records as they are (photon_build_global's or global_map_get's); none removes the map."""
        r = np.ascontiguousarray(records if records is not None else np.zeros((0, 24)), np.uint8).reshape(-1, 24)
        _check(lib().bhrt_global_map_set(self._h, _ptr(r) if len(r) else None, len(r)))
        return len(r)

    def global_map_set_ptr(self, ptr: int, n: int):
        """Same from `ptr` (host or device memory holding n balanced records)."""
        _check(lib().bhrt_global_map_set(self._h, C.c_void_p(ptr), int(n)))

    def global_map_get(self) -> np.ndarray:
        """bhrt_global_map_get: the installed global map, balanced (n, 24) uint8 records."""
        n = C.c_uint32(0)
        _check(lib().bhrt_global_map_get(self._h, None, 0, C.byref(n)))
        out = np.zeros((n.value, 24), np.uint8)
        _check(lib().bhrt_global_map_get(self._h, _ptr(out), n.value, C.byref(n)))
        return out

    def global_gather(self, p, nrm, radius=0.5, exact=False):
        """bhrt_global_gather_host: EstimateIrradiance<1000> on the global map for n points; returns (irradiance, direction), each (n, 3)."""
        p = np.ascontiguousarray(p, np.float32)
        nrm = np.ascontiguousarray(nrm, np.float32)
        irr, d = np.zeros_like(p), np.zeros_like(p)
        _check(lib().bhrt_global_gather_host(self._h, _ptr(p), _ptr(nrm), C.c_size_t(p.shape[0]), C.c_float(radius), 1 if exact else 0, _ptr(irr), _ptr(d)))
        return irr, d

    def clone(self) -> "Scene":
        """bhrt_scene_clone: a second handle on the same loaded scene (host state only: the emission, face-material, global-gather and shutter state, node names and edited node transforms,
        light names and edited lights included; no device state, so no photon map)."""
        other = Scene.__new__(Scene)
        other._h = C.c_void_p()
        other._flat = None
        _check(lib().bhrt_scene_clone(self._h, C.byref(other._h)))
        other.info = Info()
        _check(lib().bhrt_scene_info(other._h, C.byref(other.info)))
        return other

    def camera_rays(self, opts: Opts, region=None):
        """Test hook (bhrt_camera_rays): the camera rays of region (x0, y0, x1, y1) — default the whole frame — as the render's first wave step forms
        them on the device, pinhole (opts.lens = 0) or thin lens.  Returns (origins, dirs), each (region_pixels, spp, 3) float32, in the order
        of render_samples."""
        x0, y0, x1, y1 = region if region is not None else (0, 0, self.width, self.height)
        out = np.zeros(((y1 - y0) * (x1 - x0), opts.spp, 6), np.float32)
        _check(lib().bhrt_camera_rays(self._h, C.byref(opts), int(x0), int(y0), int(x1), int(y1), _ptr(out)))
        return np.ascontiguousarray(out[..., :3]), np.ascontiguousarray(out[..., 3:])

    # ---- hot path, host buffers -------------------------------------------------------------
    def trace_closest(self, origins, dirs, hit_side=SIDE_FRONT):
        """recursive() for n rays; origins/dirs: (n,3) float32. Returns dict of numpy arrays."""
        o = np.ascontiguousarray(origins, np.float32)
        d = np.ascontiguousarray(dirs, np.float32)
        n = o.shape[0]
        soa = np.ascontiguousarray(np.concatenate([o.T, d.T], axis=0), np.float32)  # ox[n] oy[n] oz[n] dx..
        t = np.empty(n, np.float32)
        node = np.empty(n, np.int32)
        prim = np.empty(n, np.int32)
        front = np.empty(n, np.int32)
        h = Hits(_ptr(t), _ptr(node), _ptr(prim), _ptr(front))
        _check(lib().bhrt_trace_closest_host(self._h, _ptr(soa), int(hit_side), C.c_size_t(n), h))
        return {"t": t, "node": node, "prim": prim, "front": front}

    def trace_shadow(self, origins, dirs, tmax):
        o = np.ascontiguousarray(origins, np.float32)
        d = np.ascontiguousarray(dirs, np.float32)
        n = o.shape[0]
        soa = np.ascontiguousarray(np.concatenate([o.T, d.T], axis=0), np.float32)
        tm = np.ascontiguousarray(np.broadcast_to(np.asarray(tmax, np.float32), (n,)), np.float32)
        vis = np.empty(n, np.float32)
        _check(lib().bhrt_trace_shadow_host(self._h, _ptr(soa), _ptr(tm), C.c_size_t(n), _ptr(vis)))
        return vis

    def render(self, opts: Opts, want_radiance=True):
        """BeginRender(): returns (rgb8 HxWx3 uint8, radiance HxWx3 float32 or None, Stats)."""
        W, H = self.width, self.height
        rgb = np.zeros((H, W, 3), np.uint8)
        rad = np.zeros((H, W, 3), np.float32) if want_radiance else None
        st = Stats()
        _check(lib().bhrt_render(self._h, C.byref(opts), _ptr(rgb), _ptr(rad) if want_radiance else None, C.byref(st)))
        return rgb, rad, st

    def render_dev(self, opts: Opts, d_rgb8_ptr: int, d_radiance_ptr: int):
        """Same with outputs left in HBM (raw device pointers, e.g. torch tensor .data_ptr())."""
        st = Stats()
        _check(lib().bhrt_render_dev(self._h, C.byref(opts), C.c_void_p(d_rgb8_ptr or None),
                                     C.c_void_p(d_radiance_ptr or None), C.byref(st), None))
        return st

    def render_var(self, opts: Opts):
        """render() plus the denoiser's noise estimate: returns (rgb8, radiance, variance), variance (H, W, 3) float32 = the per-channel
        variance of every pixel's mean (bhrt_render_var)."""
        W, H = self.width, self.height
        rgb = np.zeros((H, W, 3), np.uint8)
        rad = np.zeros((H, W, 3), np.float32)
        var = np.zeros((H, W, 3), np.float32)
        _check(lib().bhrt_render_var(self._h, C.byref(opts), _ptr(rgb), _ptr(rad), _ptr(var), None))
        return rgb, rad, var

    def render_var_dev(self, opts: Opts, d_rgb8_ptr: int, d_radiance_ptr: int, d_variance_ptr: int):
        """Same with outputs left in HBM (raw device pointers; any may be 0 = not wanted)."""
        st = Stats()
        _check(lib().bhrt_render_var_dev(self._h, C.byref(opts), C.c_void_p(d_rgb8_ptr or None), C.c_void_p(d_radiance_ptr or None),
                                         C.c_void_p(d_variance_ptr or None), C.byref(st), None))
        return st

    def render_adaptive(self, opts: Opts, aopts: AdaptiveOpts):
        """Adaptive sampling (bhrt_render_adaptive): opts.spp is the per-pixel maximum.  Returns (rgb8 (H, W, 3) uint8, radiance (H, W, 3),
        variance (H, W, 3) float32, count (H, W) uint32 samples per pixel, Stats); pixels of other ranks' tiles stay 0."""
        W, H = self.width, self.height
        rgb = np.zeros((H, W, 3), np.uint8)
        rad = np.zeros((H, W, 3), np.float32)
        var = np.zeros((H, W, 3), np.float32)
        cnt = np.zeros((H, W), np.uint32)
        st = Stats()
        _check(lib().bhrt_render_adaptive(self._h, C.byref(opts), C.byref(aopts), _ptr(rgb), _ptr(rad), _ptr(var), _ptr(cnt), C.byref(st)))
        return rgb, rad, var, cnt, st

    def render_adaptive_dev(self, opts: Opts, aopts: AdaptiveOpts, d_rgb8_ptr: int = 0, d_radiance_ptr: int = 0, d_variance_ptr: int = 0,
                            d_count_ptr: int = 0):
        """Same with outputs left in HBM (raw device pointers; any may be 0 = not wanted).  Returns Stats."""
        st = Stats()
        v = lambda x: C.c_void_p(x or None)  # noqa: E731
        _check(lib().bhrt_render_adaptive_dev(self._h, C.byref(opts), C.byref(aopts), v(d_rgb8_ptr), v(d_radiance_ptr), v(d_variance_ptr), v(d_count_ptr),
                                              C.byref(st), None))
        return st

    # ---- progressive rendering: the frame as a session that steps advance and that can be read at any point ----------------
    def progressive_begin(self, opts: Opts, aopts: AdaptiveOpts = None):
        """bhrt_progressive_begin: opens the scene's session; opts.spp is the per-pixel maximum, aopts (None = uniform) the retirement test."""
        _check(lib().bhrt_progressive_begin(self._h, C.byref(opts), C.byref(aopts) if aopts is not None else None))

    def progressive_step(self, n: int) -> Stats:
        """bhrt_progressive_step: n more samples for every active pixel (up to the maximum); returns that step's Stats."""
        st = Stats()
        _check(lib().bhrt_progressive_step(self._h, int(n), C.byref(st)))
        return st

    def progressive_frame(self, variance=True, count=True):
        """bhrt_progressive_frame: the session's frame now, (rgb8 (H, W, 3) uint8, radiance (H, W, 3), variance (H, W, 3) float32 or None,
        count (H, W) uint32 or None); pixels of other ranks' tiles stay 0."""
        W, H = self.width, self.height
        rgb = np.zeros((H, W, 3), np.uint8)
        rad = np.zeros((H, W, 3), np.float32)
        var = np.zeros((H, W, 3), np.float32) if variance else None
        cnt = np.zeros((H, W), np.uint32) if count else None
        _check(lib().bhrt_progressive_frame(self._h, _ptr(rgb), _ptr(rad), _ptr(var) if variance else None, _ptr(cnt) if count else None))
        return rgb, rad, var, cnt

    def progressive_frame_into(self, rgb=None, rad=None, var=None, cnt=None):
        """bhrt_progressive_frame into the caller's host arrays (None = not wanted): pixels of other ranks' tiles keep what the arrays hold."""
        p = lambda x: _ptr(x) if x is not None else None  # noqa: E731
        _check(lib().bhrt_progressive_frame(self._h, p(rgb), p(rad), p(var), p(cnt)))

    def progressive_frame_dev(self, d_rgb8_ptr: int = 0, d_radiance_ptr: int = 0, d_variance_ptr: int = 0, d_count_ptr: int = 0, stream: int = 0):
        """bhrt_progressive_frame_dev on raw device pointers (0 = not wanted); with a stream the call does not synchronise."""
        v = lambda x: C.c_void_p(x or None)  # noqa: E731
        _check(lib().bhrt_progressive_frame_dev(self._h, v(d_rgb8_ptr), v(d_radiance_ptr), v(d_variance_ptr), v(d_count_ptr), v(stream)))

    def progressive_status(self) -> Progress:
        """bhrt_progressive_status: steps, smallest / largest count, active pixels, samples so far, finished."""
        p = Progress()
        _check(lib().bhrt_progressive_status(self._h, C.byref(p)))
        return p

    def progressive_end(self):
        """bhrt_progressive_end (the seam's StopRender): closes the session and frees its state; fine when none is open."""
        _check(lib().bhrt_progressive_end(self._h))

    # ---- temporal session: reproject -> accumulate -> estimate -> denoise as one device-resident call per frame ------------
    def temporal_begin(self, opts: Opts, topts: TemporalSessionOpts):
        """bhrt_temporal_begin: opens the scene's temporal session; frame k renders with opts.seed + k."""
        _check(lib().bhrt_temporal_begin(self._h, C.byref(opts) if opts is not None else None, C.byref(topts) if topts is not None else None))

    def temporal_frame(self, want_radiance=True):
        """bhrt_temporal_frame: the next frame of the session at the scene's camera and node transforms; returns the displayed frame,
        (rgb8 (H, W, 3) uint8, radiance (H, W, 3) float32 or None, Stats)."""
        H, W = self.height, self.width
        rgb = np.zeros((H, W, 3), np.uint8)
        rad = np.zeros((H, W, 3), np.float32) if want_radiance else None
        st = Stats()
        _check(lib().bhrt_temporal_frame(self._h, _ptr(rgb), _ptr(rad) if want_radiance else None, C.byref(st)))
        return rgb, rad, st

    def temporal_frame_dev(self, d_rgb8_ptr: int = 0, d_radiance_ptr: int = 0) -> Stats:
        """bhrt_temporal_frame_dev on raw device pointers (0 = not wanted); synchronises the scene's stream."""
        st = Stats()
        _check(lib().bhrt_temporal_frame_dev(self._h, C.c_void_p(d_rgb8_ptr or None), C.c_void_p(d_radiance_ptr or None), C.byref(st)))
        return st

    def temporal_reset(self):
        """bhrt_temporal_reset: a cut; the next frame is frame 0 again, the images stay allocated."""
        _check(lib().bhrt_temporal_reset(self._h))

    def temporal_status(self) -> TemporalProgress:
        """bhrt_temporal_status: frames, pixels with history in the last frame, W * H, failed."""
        p = TemporalProgress()
        _check(lib().bhrt_temporal_status(self._h, C.byref(p)))
        return p

    def temporal_image(self, which: int) -> np.ndarray:
        """bhrt_temporal_image: a host copy of one kept image (TEMPORAL_IMG_*) of the last frame: (H, W) or (H, W, 3), float32 (int32: the node ids)."""
        shape = (self.height, self.width) if which in _TEMPORAL_IMG_ONE_CHANNEL else (self.height, self.width, 3)
        a = np.zeros(shape, np.int32 if which == TEMPORAL_IMG_NODE else np.float32)
        _check(lib().bhrt_temporal_image(self._h, int(which), _ptr(a)))
        return a

    def temporal_image_dev(self, which: int) -> int:
        """bhrt_temporal_image_dev: the device address of one kept image, borrowed until the next frame, reset or end."""
        p = C.c_void_p()
        _check(lib().bhrt_temporal_image_dev(self._h, int(which), C.byref(p)))
        return p.value or 0

    def temporal_set_change(self, opts: "ChangeOpts | None"):
        """bhrt_temporal_set_change: the session's change test on with these options, None = off; legal until the first frame since
        begin or reset has completed.  With it on, TEMPORAL_IMG_CHANGE and TEMPORAL_IMG_USED_LENGTH are kept."""
        _check(lib().bhrt_temporal_set_change(self._h, C.byref(opts) if opts is not None else None))

    def temporal_end(self):
        """bhrt_temporal_end: closes the session and frees its images; fine when none is open."""
        _check(lib().bhrt_temporal_end(self._h))

    def sample_count_image(self, count):
        """RenderImage::ComputeSampleCountImage (scene.h:603-626, bhrt_sample_count_image) of a count image: returns (img uint8 shaped like
        count, smax)."""
        c = np.ascontiguousarray(count, np.uint32)
        img = np.zeros(c.shape, np.uint8)
        smax = C.c_uint32(0)
        _check(lib().bhrt_sample_count_image(self._h, _ptr(c), C.c_size_t(c.size), _ptr(img), C.byref(smax)))
        return img, smax.value

    def denoise(self, opts: DenoiseOpts, radiance, variance=None, z=None, normal=None, albedo=None):
        """DenoiseImage (bhrt_denoise) on host arrays of the scene's W x H frame: radiance (H, W, 3) linear, variance like it or None;
        guides z (H, W), normal / albedo (H, W, 3), each None = the first hit computed on the device.  Returns (out (H, W, 3) float32 linear,
        rgb8 (H, W, 3) uint8)."""
        W, H = self.width, self.height

        def arr(a, shape):
            if a is None:
                return None
            a = np.ascontiguousarray(a, np.float32)
            if a.size != int(np.prod(shape)):
                raise ValueError(f"expected {shape} floats, got {a.shape}")
            return a
        c = arr(radiance, (H, W, 3))
        v, zz, n, a = arr(variance, (H, W, 3)), arr(z, (H, W)), arr(normal, (H, W, 3)), arr(albedo, (H, W, 3))
        out = np.zeros((H, W, 3), np.float32)
        rgb = np.zeros((H, W, 3), np.uint8)
        p = lambda x: _ptr(x) if x is not None else None  # noqa: E731
        _check(lib().bhrt_denoise(self._h, C.byref(opts), _ptr(c), p(v), p(zz), p(n), p(a), _ptr(out), _ptr(rgb)))
        return out, rgb

    def denoise_dev(self, opts: DenoiseOpts, d_radiance: int, d_variance: int = 0, d_z: int = 0, d_normal: int = 0, d_albedo: int = 0,
                    d_out: int = 0, d_rgb8: int = 0, stream: int = 0):
        """bhrt_denoise_dev on raw device pointers (0 = NULL); with a stream the call does not synchronise."""
        v = lambda x: C.c_void_p(x or None)  # noqa: E731
        _check(lib().bhrt_denoise_dev(self._h, C.byref(opts), v(d_radiance), v(d_variance), v(d_z), v(d_normal), v(d_albedo), v(d_out), v(d_rgb8),
                                      v(stream)))

    def denoise_sampled(self, opts: DenoiseOpts, radiance, variance, z, normal, albedo, coverage, sigma_coverage: float = DENOISE_SIGMA_COVERAGE):
        """The denoiser for sampled guides (bhrt_denoise_sampled) on host arrays: radiance and variance as for denoise(); z, normal,
        albedo and coverage are the four images of guides() with the render's seed, jitter and lens (None is passed as NULL: an error unless
        opts.iterations == 0).  Returns (out (H, W, 3) float32 linear, rgb8 (H, W, 3) uint8)."""
        W, H = self.width, self.height

        def arr(a, shape):
            if a is None:
                return None
            a = np.ascontiguousarray(a, np.float32)
            if a.size != int(np.prod(shape)):
                raise ValueError(f"expected {shape} floats, got {a.shape}")
            return a
        c = arr(radiance, (H, W, 3))
        v, zz, n, a, cov = arr(variance, (H, W, 3)), arr(z, (H, W)), arr(normal, (H, W, 3)), arr(albedo, (H, W, 3)), arr(coverage, (H, W))
        out = np.zeros((H, W, 3), np.float32)
        rgb = np.zeros((H, W, 3), np.uint8)
        p = lambda x: _ptr(x) if x is not None else None  # noqa: E731
        _check(lib().bhrt_denoise_sampled(self._h, C.byref(opts), C.c_float(sigma_coverage), _ptr(c), p(v), p(zz), p(n), p(a), p(cov), _ptr(out), _ptr(rgb)))
        return out, rgb

    def denoise_sampled_dev(self, opts: DenoiseOpts, sigma_coverage: float, d_radiance: int, d_variance: int = 0, d_z: int = 0, d_normal: int = 0,
                            d_albedo: int = 0, d_coverage: int = 0, d_out: int = 0, d_rgb8: int = 0, stream: int = 0):
        """bhrt_denoise_sampled_dev on raw device pointers (0 = NULL); with a stream the call does not synchronise."""
        v = lambda x: C.c_void_p(x or None)  # noqa: E731
        _check(lib().bhrt_denoise_sampled_dev(self._h, C.byref(opts), C.c_float(sigma_coverage), v(d_radiance), v(d_variance), v(d_z), v(d_normal),
                                              v(d_albedo), v(d_coverage), v(d_out), v(d_rgb8), v(stream)))

    # ---- temporal reprojection: carry a frame's light across a camera move ------------------------------------------------
    def camera_frame(self):
        """bhrt_scene_get_camera_frame: (4, 3) float32 = pos, top_left, dd_x, dd_y of the scene's camera now.  A host that reprojects reads it
        before it moves the camera."""
        f = np.zeros((4, 3), np.float32)
        _check(lib().bhrt_scene_get_camera_frame(self._h, _ptr(f)))
        return f

    def _image(self, a, shape, what):
        if a is None:
            return None
        a = np.ascontiguousarray(a, np.float32)
        if a.size != int(np.prod(shape)):
            raise ValueError(f"{what}: expected {shape} floats, got {a.shape}")
        return a

    def reproject(self, opts: ReprojectOpts, prev_frame, prev_z, prev_normal, prev_radiance=None, prev_length=None, prev_albedo=None, z=None, normal=None,
                  albedo=None, want=("history", "length", "motion")):
        """bhrt_reproject on host arrays of the scene's W x H frame: the previous view's camera_frame(), first hit (prev_z, prev_normal, optionally
        prev_albedo), radiance and length image (None = 1 everywhere), and the current view's first hit, each None = computed on the device.
        Returns (history (H, W, 3), length (H, W), motion (H, W, 2)) float32, None for those not named in `want`."""
        W, H = self.width, self.height
        pf = None if prev_frame is None else np.ascontiguousarray(prev_frame, np.float32).reshape(-1)
        if pf is not None and pf.size != 12:
            raise ValueError("prev_frame: expected 12 floats")
        i = [self._image(a, sh, k) for a, sh, k in ((prev_z, (H, W), "prev_z"), (prev_normal, (H, W, 3), "prev_normal"), (prev_radiance, (H, W, 3), "prev_radiance"),
                                                    (prev_length, (H, W), "prev_length"), (prev_albedo, (H, W, 3), "prev_albedo"), (z, (H, W), "z"),
                                                    (normal, (H, W, 3), "normal"), (albedo, (H, W, 3), "albedo"))]
        shapes = {"history": (H, W, 3), "length": (H, W), "motion": (H, W, 2)}
        o = [np.zeros(shapes[k], np.float32) if k in want else None for k in ("history", "length", "motion")]
        p = lambda x: _ptr(x) if x is not None else None  # noqa: E731
        _check(lib().bhrt_reproject(self._h, C.byref(opts) if opts is not None else None, p(pf), *[p(a) for a in i], *[p(a) for a in o]))
        return tuple(o)

    def reproject_dev(self, opts: ReprojectOpts, prev_frame, d_prev_z: int, d_prev_normal: int, d_prev_radiance: int = 0, d_prev_length: int = 0,
                      d_prev_albedo: int = 0, d_z: int = 0, d_normal: int = 0, d_albedo: int = 0, d_history: int = 0, d_length: int = 0, d_motion: int = 0,
                      stream: int = 0):
        """bhrt_reproject_dev on raw device pointers (0 = NULL; prev_frame stays a host array of 12 floats); with a stream the call does not
        synchronise."""
        pf = np.ascontiguousarray(prev_frame, np.float32).reshape(-1)
        if pf.size != 12:
            raise ValueError("prev_frame: expected 12 floats")
        v = lambda x: C.c_void_p(x or None)  # noqa: E731
        _check(lib().bhrt_reproject_dev(self._h, C.byref(opts), _ptr(pf), v(d_prev_z), v(d_prev_normal), v(d_prev_radiance), v(d_prev_length), v(d_prev_albedo),
                                        v(d_z), v(d_normal), v(d_albedo), v(d_history), v(d_length), v(d_motion), v(stream)))

    def _xforms(self, prev_xforms):
        if prev_xforms is None:
            return None
        x = np.ascontiguousarray(prev_xforms, XFORM_DTYPE).reshape(-1)
        if x.shape[0] != self.info.n_nodes:
            raise ValueError(f"prev_xforms: expected {self.info.n_nodes} records, got {x.shape[0]}")
        return x if x.shape[0] else np.zeros(1, XFORM_DTYPE)

    def _ids(self, a, what):
        if a is None:
            return None
        a = np.ascontiguousarray(a, np.int32)
        if a.size != self.width * self.height:
            raise ValueError(f"{what}: expected {(self.height, self.width)} int32, got {a.shape}")
        return a

    def reproject_moving(self, opts: ReprojectOpts, prev_frame, prev_xforms, prev_z, prev_normal, prev_radiance=None, prev_length=None, prev_albedo=None,
                         prev_id=None, z=None, normal=None, albedo=None, id=None, want=("history", "length", "motion")):
        """bhrt_reproject_moving on host arrays: reproject() with the previous frame's node_transforms() snapshot, its first_hit_node() image
        (optional) and the current view's (None = computed on the device).  Pixels of a node that moved, or whose ancestor moved, are carried
        through the node's motion.  Returns (history, length, motion) as reproject()."""
        W, H = self.width, self.height
        pf = None if prev_frame is None else np.ascontiguousarray(prev_frame, np.float32).reshape(-1)
        if pf is not None and pf.size != 12:
            raise ValueError("prev_frame: expected 12 floats")
        px = self._xforms(prev_xforms)
        i = [self._image(a, sh, k) for a, sh, k in ((prev_z, (H, W), "prev_z"), (prev_normal, (H, W, 3), "prev_normal"), (prev_radiance, (H, W, 3), "prev_radiance"),
                                                    (prev_length, (H, W), "prev_length"), (prev_albedo, (H, W, 3), "prev_albedo"))]
        g = [self._image(a, sh, k) for a, sh, k in ((z, (H, W), "z"), (normal, (H, W, 3), "normal"), (albedo, (H, W, 3), "albedo"))]
        pid, cid = self._ids(prev_id, "prev_id"), self._ids(id, "id")
        shapes = {"history": (H, W, 3), "length": (H, W), "motion": (H, W, 2)}
        o = [np.zeros(shapes[k], np.float32) if k in want else None for k in ("history", "length", "motion")]
        p = lambda x: _ptr(x) if x is not None else None  # noqa: E731
        _check(lib().bhrt_reproject_moving(self._h, C.byref(opts) if opts is not None else None, p(pf), p(px), *[p(a) for a in i], p(pid), *[p(a) for a in g], p(cid),
                                           *[p(a) for a in o]))
        return tuple(o)

    def reproject_moving_dev(self, opts: ReprojectOpts, prev_frame, prev_xforms, d_prev_z: int, d_prev_normal: int, d_prev_radiance: int = 0, d_prev_length: int = 0,
                             d_prev_albedo: int = 0, d_prev_id: int = 0, d_z: int = 0, d_normal: int = 0, d_albedo: int = 0, d_id: int = 0, d_history: int = 0,
                             d_length: int = 0, d_motion: int = 0, stream: int = 0):
        """bhrt_reproject_moving_dev on raw device pointers (0 = NULL; prev_frame and prev_xforms stay host arrays); with a stream the call does
        not synchronise."""
        pf = np.ascontiguousarray(prev_frame, np.float32).reshape(-1)
        if pf.size != 12:
            raise ValueError("prev_frame: expected 12 floats")
        px = self._xforms(prev_xforms)
        v = lambda x: C.c_void_p(x or None)  # noqa: E731
        _check(lib().bhrt_reproject_moving_dev(self._h, C.byref(opts), _ptr(pf), _ptr(px), v(d_prev_z), v(d_prev_normal), v(d_prev_radiance), v(d_prev_length),
                                               v(d_prev_albedo), v(d_prev_id), v(d_z), v(d_normal), v(d_albedo), v(d_id), v(d_history), v(d_length), v(d_motion),
                                               v(stream)))

    def temporal_accumulate(self, opts: TemporalOpts, radiance, cur_samples: float, history=None, length=None):
        """bhrt_temporal_accumulate on host arrays: the current frame's radiance (H, W, 3) with cur_samples samples behind it, blended into
        reproject()'s history and length (either None: no pixel has a history).  Returns (out (H, W, 3) float32, out_length (H, W) float32,
        rgb8 (H, W, 3) uint8)."""
        W, H = self.width, self.height
        c, h, l = self._image(radiance, (H, W, 3), "radiance"), self._image(history, (H, W, 3), "history"), self._image(length, (H, W), "length")
        out, ol, rgb = np.zeros((H, W, 3), np.float32), np.zeros((H, W), np.float32), np.zeros((H, W, 3), np.uint8)
        p = lambda x: _ptr(x) if x is not None else None  # noqa: E731
        _check(lib().bhrt_temporal_accumulate(self._h, C.byref(opts) if opts is not None else None, p(c), C.c_float(cur_samples), p(h), p(l), _ptr(out), _ptr(ol),
                                              _ptr(rgb)))
        return out, ol, rgb

    def temporal_accumulate_dev(self, opts: TemporalOpts, d_radiance: int, cur_samples: float, d_history: int = 0, d_length: int = 0, d_out: int = 0,
                                d_out_length: int = 0, d_rgb8: int = 0, stream: int = 0):
        """bhrt_temporal_accumulate_dev on raw device pointers (0 = NULL); with a stream the call does not synchronise."""
        v = lambda x: C.c_void_p(x or None)  # noqa: E731
        _check(lib().bhrt_temporal_accumulate_dev(self._h, C.byref(opts), v(d_radiance), C.c_float(cur_samples), v(d_history), v(d_length), v(d_out), v(d_out_length),
                                                  v(d_rgb8), v(stream)))

    # ---- the variance of a temporally accumulated frame ----------------------------------------------------------------------
    def reproject_var(self, opts: ReprojectOpts, prev_frame, prev_z, prev_normal, prev_radiance=None, prev_variance=None, prev_length=None, prev_albedo=None,
                      z=None, normal=None, albedo=None, prev_xforms=None, prev_id=None, id=None, want=("history", "history_variance", "length", "motion")):
        """bhrt_reproject_var on host arrays: reproject() (reproject_moving() when prev_xforms, the previous frame's node_transforms(), is given)
        that also carries prev_variance, the variance of prev_radiance, into the new view.  Returns (history (H, W, 3), history_variance
        (H, W, 3), length (H, W), motion (H, W, 2)) float32, None for those not named in `want`."""
        W, H = self.width, self.height
        pf = None if prev_frame is None else np.ascontiguousarray(prev_frame, np.float32).reshape(-1)
        if pf is not None and pf.size != 12:
            raise ValueError("prev_frame: expected 12 floats")
        px = self._xforms(prev_xforms)
        i = [self._image(a, sh, k) for a, sh, k in ((prev_z, (H, W), "prev_z"), (prev_normal, (H, W, 3), "prev_normal"), (prev_radiance, (H, W, 3), "prev_radiance"),
                                                    (prev_variance, (H, W, 3), "prev_variance"), (prev_length, (H, W), "prev_length"),
                                                    (prev_albedo, (H, W, 3), "prev_albedo"))]
        g = [self._image(a, sh, k) for a, sh, k in ((z, (H, W), "z"), (normal, (H, W, 3), "normal"), (albedo, (H, W, 3), "albedo"))]
        pid, cid = self._ids(prev_id, "prev_id"), self._ids(id, "id")
        shapes = {"history": (H, W, 3), "history_variance": (H, W, 3), "length": (H, W), "motion": (H, W, 2)}
        o = [np.zeros(shapes[k], np.float32) if k in want else None for k in ("history", "history_variance", "length", "motion")]
        p = lambda x: _ptr(x) if x is not None else None  # noqa: E731
        _check(lib().bhrt_reproject_var(self._h, C.byref(opts) if opts is not None else None, p(pf), p(px), *[p(a) for a in i], p(pid), *[p(a) for a in g], p(cid),
                                        *[p(a) for a in o]))
        return tuple(o)

    def reproject_var_dev(self, opts: ReprojectOpts, prev_frame, d_prev_z: int, d_prev_normal: int, d_prev_radiance: int = 0, d_prev_variance: int = 0,
                          d_prev_length: int = 0, d_prev_albedo: int = 0, d_z: int = 0, d_normal: int = 0, d_albedo: int = 0, d_history: int = 0,
                          d_history_variance: int = 0, d_length: int = 0, d_motion: int = 0, prev_xforms=None, d_prev_id: int = 0, d_id: int = 0, stream: int = 0):
        """bhrt_reproject_var_dev on raw device pointers (0 = NULL; prev_frame and prev_xforms stay host arrays, prev_xforms None = camera only);
        with a stream the call does not synchronise."""
        pf = np.ascontiguousarray(prev_frame, np.float32).reshape(-1)
        if pf.size != 12:
            raise ValueError("prev_frame: expected 12 floats")
        px = self._xforms(prev_xforms)
        v = lambda x: C.c_void_p(x or None)  # noqa: E731
        _check(lib().bhrt_reproject_var_dev(self._h, C.byref(opts), _ptr(pf), _ptr(px) if px is not None else None, v(d_prev_z), v(d_prev_normal), v(d_prev_radiance),
                                            v(d_prev_variance), v(d_prev_length), v(d_prev_albedo), v(d_prev_id), v(d_z), v(d_normal), v(d_albedo), v(d_id), v(d_history),
                                            v(d_history_variance), v(d_length), v(d_motion), v(stream)))

    def temporal_accumulate_var(self, opts: TemporalOpts, radiance, variance, cur_samples: float, history=None, history_variance=None, length=None):
        """bhrt_temporal_accumulate_var on host arrays: temporal_accumulate() with the current frame's variance (render_var's) and
        reproject_var()'s history_variance.  Returns (out (H, W, 3), out_variance (H, W, 3), out_length (H, W)) float32 and rgb8 (H, W, 3) uint8;
        out_variance is denoise()'s variance and the next reproject_var()'s prev_variance."""
        W, H = self.width, self.height
        c, vv = self._image(radiance, (H, W, 3), "radiance"), self._image(variance, (H, W, 3), "variance")
        h, hv, l = self._image(history, (H, W, 3), "history"), self._image(history_variance, (H, W, 3), "history_variance"), self._image(length, (H, W), "length")
        out, ov, ol, rgb = np.zeros((H, W, 3), np.float32), np.zeros((H, W, 3), np.float32), np.zeros((H, W), np.float32), np.zeros((H, W, 3), np.uint8)
        p = lambda x: _ptr(x) if x is not None else None  # noqa: E731
        _check(lib().bhrt_temporal_accumulate_var(self._h, C.byref(opts) if opts is not None else None, p(c), p(vv), C.c_float(cur_samples), p(h), p(hv), p(l), _ptr(out),
                                                  _ptr(ov), _ptr(ol), _ptr(rgb)))
        return out, ov, ol, rgb

    def temporal_accumulate_var_dev(self, opts: TemporalOpts, d_radiance: int, d_variance: int, cur_samples: float, d_history: int = 0, d_history_variance: int = 0,
                                    d_length: int = 0, d_out: int = 0, d_out_variance: int = 0, d_out_length: int = 0, d_rgb8: int = 0, stream: int = 0):
        """bhrt_temporal_accumulate_var_dev on raw device pointers (0 = NULL); with a stream the call does not synchronise."""
        v = lambda x: C.c_void_p(x or None)  # noqa: E731
        _check(lib().bhrt_temporal_accumulate_var_dev(self._h, C.byref(opts), v(d_radiance), v(d_variance), C.c_float(cur_samples), v(d_history), v(d_history_variance),
                                                      v(d_length), v(d_out), v(d_out_variance), v(d_out_length), v(d_rgb8), v(stream)))

    # ---- spatial variance estimate ---------------------------------------------------------------------------------------------
    def variance_spatial(self, opts: SpatialVarianceOpts, radiance, variance=None, length=None, z=None, normal=None, albedo=None):
        """bhrt_variance_spatial on host arrays: the variance of `radiance` estimated from each pixel's neighbourhood on its own surface; where
        length >= opts.min_length the pixel keeps `variance`.  z, normal, albedo None = computed here.  Returns out_variance (H, W, 3) float32,
        what denoise() and temporal_accumulate_var() take as variance."""
        W, H = self.width, self.height
        i = [self._image(a, sh, k) for a, sh, k in ((radiance, (H, W, 3), "radiance"), (variance, (H, W, 3), "variance"), (length, (H, W), "length"), (z, (H, W), "z"),
                                                    (normal, (H, W, 3), "normal"), (albedo, (H, W, 3), "albedo"))]
        out = np.zeros((H, W, 3), np.float32)
        p = lambda x: _ptr(x) if x is not None else None  # noqa: E731
        _check(lib().bhrt_variance_spatial(self._h, C.byref(opts) if opts is not None else None, *[p(a) for a in i], _ptr(out)))
        return out

    def variance_spatial_dev(self, opts: SpatialVarianceOpts, d_radiance: int, d_variance: int = 0, d_length: int = 0, d_z: int = 0, d_normal: int = 0,
                             d_albedo: int = 0, d_out_variance: int = 0, stream: int = 0):
        """bhrt_variance_spatial_dev on raw device pointers (0 = NULL); with a stream the call does not synchronise."""
        v = lambda x: C.c_void_p(x or None)  # noqa: E731
        _check(lib().bhrt_variance_spatial_dev(self._h, C.byref(opts), v(d_radiance), v(d_variance), v(d_length), v(d_z), v(d_normal), v(d_albedo), v(d_out_variance),
                                               v(stream)))

    # ---- temporal change test --------------------------------------------------------------------------------------------------
    def temporal_change(self, opts: ChangeOpts, radiance, variance, history, history_variance, length, z=None, normal=None, want_change=True):
        """bhrt_temporal_change on host arrays: reproject_var()'s length shortened where history and current frame differ by more than the noise
        both variances predict, over each pixel's window on its own surface.  z, normal None = computed here.  Returns (out_length (H, W),
        change (H, W) or None) float32; out_length is temporal_accumulate_var()'s length."""
        W, H = self.width, self.height
        i = [self._image(a, sh, k) for a, sh, k in ((radiance, (H, W, 3), "radiance"), (variance, (H, W, 3), "variance"), (history, (H, W, 3), "history"),
                                                    (history_variance, (H, W, 3), "history_variance"), (length, (H, W), "length"), (z, (H, W), "z"),
                                                    (normal, (H, W, 3), "normal"))]
        out, change = np.zeros((H, W), np.float32), np.zeros((H, W), np.float32) if want_change else None
        p = lambda x: _ptr(x) if x is not None else None  # noqa: E731
        _check(lib().bhrt_temporal_change(self._h, C.byref(opts) if opts is not None else None, *[p(a) for a in i], _ptr(out), p(change)))
        return out, change

    def temporal_change_dev(self, opts: ChangeOpts, d_radiance: int, d_variance: int, d_history: int, d_history_variance: int, d_length: int, d_z: int = 0,
                            d_normal: int = 0, d_out_length: int = 0, d_change: int = 0, stream: int = 0):
        """bhrt_temporal_change_dev on raw device pointers (0 = NULL); with a stream the call does not synchronise."""
        v = lambda x: C.c_void_p(x or None)  # noqa: E731
        _check(lib().bhrt_temporal_change_dev(self._h, C.byref(opts), v(d_radiance), v(d_variance), v(d_history), v(d_history_variance), v(d_length), v(d_z), v(d_normal),
                                              v(d_out_length), v(d_change), v(stream)))

    # ---- guided upsampling ----------------------------------------------------------------------------------------------------
    def upsample(self, opts: UpsampleOpts, low_radiance, low_z, low_normal, low_albedo=None, low_variance=None, z=None, normal=None, albedo=None,
                 want=("out", "variance", "confidence", "rgb8")):
        """bhrt_upsample on host arrays: this (full-size) scene's frame rebuilt from a low frame (h, w, 3) with H = s h, W = s w, along the
        full-size first hit (z, normal, albedo None = computed here).  Returns a dict of the outputs named in `want`: out (H, W, 3) float32,
        variance (H, W, 3) float32 (needs low_variance), confidence (H, W) float32, rgb8 (H, W, 3) uint8."""
        W, H = self.width, self.height
        low_radiance = np.ascontiguousarray(low_radiance, np.float32)
        if low_radiance.ndim != 3 or low_radiance.shape[2] != 3:
            raise ValueError(f"low_radiance: expected (h, w, 3), got {low_radiance.shape}")
        h, w = low_radiance.shape[:2]
        i = [self._image(a, sh, k) for a, sh, k in ((low_variance, (h, w, 3), "low_variance"), (low_z, (h, w), "low_z"), (low_normal, (h, w, 3), "low_normal"),
                                                    (low_albedo, (h, w, 3), "low_albedo"), (z, (H, W), "z"), (normal, (H, W, 3), "normal"),
                                                    (albedo, (H, W, 3), "albedo"))]
        res = {}
        if "out" in want:
            res["out"] = np.zeros((H, W, 3), np.float32)
        if "variance" in want and low_variance is not None:
            res["variance"] = np.zeros((H, W, 3), np.float32)
        if "confidence" in want:
            res["confidence"] = np.zeros((H, W), np.float32)
        if "rgb8" in want:
            res["rgb8"] = np.zeros((H, W, 3), np.uint8)
        p = lambda x: _ptr(x) if x is not None else None  # noqa: E731
        _check(lib().bhrt_upsample(self._h, C.byref(opts) if opts is not None else None, C.c_int32(w), C.c_int32(h), _ptr(low_radiance), *[p(a) for a in i],
                                   p(res.get("out")), p(res.get("variance")), p(res.get("confidence")), p(res.get("rgb8"))))
        return res

    def upsample_dev(self, opts: UpsampleOpts, low_width: int, low_height: int, d_low_radiance: int, d_low_variance: int = 0, d_low_z: int = 0,
                     d_low_normal: int = 0, d_low_albedo: int = 0, d_z: int = 0, d_normal: int = 0, d_albedo: int = 0, d_out: int = 0, d_out_variance: int = 0,
                     d_confidence: int = 0, d_rgb8: int = 0, stream: int = 0):
        """bhrt_upsample_dev on raw device pointers (0 = NULL); with a stream the call does not synchronise."""
        v = lambda x: C.c_void_p(x or None)  # noqa: E731
        _check(lib().bhrt_upsample_dev(self._h, C.byref(opts), C.c_int32(low_width), C.c_int32(low_height), v(d_low_radiance), v(d_low_variance), v(d_low_z),
                                       v(d_low_normal), v(d_low_albedo), v(d_z), v(d_normal), v(d_albedo), v(d_out), v(d_out_variance), v(d_confidence),
                                       v(d_rgb8), v(stream)))

    # ---- images beside the colour image (RenderImage z-buffer, DenoiseImage inputs) ------------
    def first_hit(self):
        """First hit of every pixel's un-jittered camera ray: z (H, W), normal (H, W, 3), albedo (H, W, 3), host arrays."""
        H, W = self.height, self.width
        z, nrm, alb = np.zeros((H, W), np.float32), np.zeros((H, W, 3), np.float32), np.zeros((H, W, 3), np.float32)
        _check(lib().bhrt_first_hit(self._h, _ptr(z), _ptr(nrm), _ptr(alb)))
        return z, nrm, alb

    def first_hit_dev(self, d_z: int = 0, d_normal: int = 0, d_albedo: int = 0, stream: int = 0):
        _check(lib().bhrt_first_hit_dev(self._h, C.c_void_p(d_z or None), C.c_void_p(d_normal or None), C.c_void_p(d_albedo or None),
                                        C.c_void_p(stream or None)))

    def first_hit_node(self):
        """bhrt_first_hit_node: (H, W) int32, the node index of the first hit of every pixel's un-jittered camera ray, -1 on a miss."""
        node = np.zeros((self.height, self.width), np.int32)
        _check(lib().bhrt_first_hit_node(self._h, _ptr(node)))
        return node

    def first_hit_node_dev(self, d_node: int, stream: int = 0):
        _check(lib().bhrt_first_hit_node_dev(self._h, C.c_void_p(d_node or None), C.c_void_p(stream or None)))

    def first_hit_ex(self, want=("z", "normal", "albedo", "node"), into=None):
        """bhrt_first_hit_ex: the images of first_hit and first_hit_node from one trace per pixel.  Returns a dict of the images named in
        `want` (the others are passed as NULL); `into`: a dict of host arrays to write into instead of fresh zeros."""
        H, W = self.height, self.width
        shapes = {"z": ((H, W), np.float32), "normal": ((H, W, 3), np.float32), "albedo": ((H, W, 3), np.float32), "node": ((H, W), np.int32)}
        out = {}
        for k in want:
            out[k] = into[k] if into is not None and k in into else np.zeros(*shapes[k])
            assert out[k].shape == shapes[k][0] and out[k].dtype == shapes[k][1] and out[k].flags["C_CONTIGUOUS"], k
        p = lambda k: _ptr(out[k]) if k in out else None  # noqa: E731
        _check(lib().bhrt_first_hit_ex(self._h, p("z"), p("normal"), p("albedo"), p("node")))
        return out

    def first_hit_ex_dev(self, d_z: int = 0, d_normal: int = 0, d_albedo: int = 0, d_node: int = 0, stream: int = 0):
        v = lambda x: C.c_void_p(x or None)  # noqa: E731
        _check(lib().bhrt_first_hit_ex_dev(self._h, v(d_z), v(d_normal), v(d_albedo), v(d_node), v(stream)))

    def guides(self, opts: Opts, want=("z", "normal", "albedo", "coverage"), into=None):
        """Sampled guide images (bhrt_guides): z (H, W), normal (H, W, 3), albedo (H, W, 3) and coverage (H, W), formed by the
        camera samples of a render with these options (spp, seed, jitter, lens, rank / world_size / tile_size, samples_per_pass) and averaged
        per pixel.  Returns a dict of the images named in `want` (the others are passed as NULL); `into`: a dict of host arrays to write into
        instead of fresh zeros (pixels of other ranks' tiles keep what they hold)."""
        H, W = self.height, self.width
        shapes = {"z": (H, W), "normal": (H, W, 3), "albedo": (H, W, 3), "coverage": (H, W)}
        out = {}
        for k in want:
            a = into[k] if into is not None and k in into else np.zeros(shapes[k], np.float32)
            if a.dtype != np.float32 or a.shape != shapes[k] or not a.flags["C_CONTIGUOUS"]:
                raise ValueError(f"{k}: expected a contiguous float32 array of shape {shapes[k]}")
            out[k] = a
        p = lambda k: _ptr(out[k]) if k in out else None  # noqa: E731
        _check(lib().bhrt_guides(self._h, C.byref(opts), p("z"), p("normal"), p("albedo"), p("coverage")))
        return out

    def guides_dev(self, opts: Opts, d_z: int = 0, d_normal: int = 0, d_albedo: int = 0, d_coverage: int = 0, stream: int = 0):
        """bhrt_guides_dev on raw device pointers (0 = NULL); with a stream the call does not synchronise."""
        v = lambda x: C.c_void_p(x or None)  # noqa: E731
        _check(lib().bhrt_guides_dev(self._h, C.byref(opts), v(d_z), v(d_normal), v(d_albedo), v(d_coverage), v(stream)))

    def zbuffer_image_dev(self, d_z: int, n: int, d_img: int, stream: int = 0):
        """RenderImage::ComputeZBufferImage (scene.h:578-600) on device buffers."""
        _check(lib().bhrt_zbuffer_image_dev(self._h, C.c_void_p(d_z), C.c_size_t(n), C.c_void_p(d_img), C.c_void_p(stream or None)))

    def color_image_dev(self, d_radiance: int, n_pixels: int, gamma: int, d_color: int, stream: int = 0):
        """colorArray of BeginRender (Main.cpp:219-229): the gamma-corrected float image DenoiseImage is given."""
        _check(lib().bhrt_color_image_dev(self._h, C.c_void_p(d_radiance), C.c_size_t(n_pixels), int(gamma), C.c_void_p(d_color),
                                          C.c_void_p(stream or None)))

    # ---- caustic photon map ------------------------------------------------------------------
    def photon_build(self, opts: Opts, max_photons: int) -> int:
        n = C.c_uint32(0)
        _check(lib().bhrt_photon_build(self._h, C.byref(opts), int(max_photons), C.byref(n)))
        return n.value

    def knob(self, name: str, value: int):
        """Knobs ("frame_cap", "gather_lane_budget", "gather_stats", "shadow_overlap", "fused_resolve", "finish_misses"): which internal path a render takes, never its result (bhrt_scene_knob)."""
        _check(lib().bhrt_scene_knob(self._h, name.encode(), int(value)))

    def photon_get(self) -> np.ndarray:
        """Balanced (heap-order) photon array as (n, 24) uint8 records (cyPhotonMap.h:72-90)."""
        n = C.c_uint32(0)
        _check(lib().bhrt_photon_get(self._h, None, 0, C.byref(n)))
        out = np.zeros((n.value, 24), np.uint8)
        _check(lib().bhrt_photon_get(self._h, _ptr(out), n.value, C.byref(n)))
        return out

    def photon_gather(self, p, nrm, radius=0.5, exact=False):
        """EstimateIrradiance<1000> for n points; exact: bhrt_opts.photon_exact (the reference's heap history replayed for heavy queries)."""
        irr, d, _, _, _ = self.photon_gather_ex(p, nrm, radius, exact=exact, want_knn=False)
        return irr, d

    def photon_gather_ex(self, p, nrm, radius=0.5, exact=False, want_knn=True):
        """photon_gather with the choice of bhrt_opts.photon_exact; returns (irr, dir, knn (cnt, 1000) uint32, knn_count (cnt,), d2max (cnt,))."""
        p = np.ascontiguousarray(p, np.float32)
        nrm = np.ascontiguousarray(nrm, np.float32)
        irr, d = np.zeros_like(p), np.zeros_like(p)
        cnt = p.shape[0]
        knn = np.zeros((cnt, 1000), np.uint32) if want_knn else None
        kc, dm = np.zeros(cnt, np.uint32), np.zeros(cnt, np.float32)
        _check(lib().bhrt_photon_gather_host_ex(self._h, _ptr(p), _ptr(nrm), C.c_size_t(cnt), C.c_float(radius), 1 if exact else 0, _ptr(irr), _ptr(d),
                                                _ptr(knn) if want_knn else None, _ptr(kc), _ptr(dm)))
        return irr, d, knn, kc, dm

    def photon_emit_range(self, opts: Opts, e0: int, count: int, global_map: bool = False, capacity: int = 0) -> np.ndarray:
        """Emissions [e0, e0 + count): the photons they store, emission order, unscaled power, (n, 24) uint8 (multi-GPU build)."""
        capacity = capacity or 16 * count
        out = np.zeros((capacity, 24), np.uint8)
        n = C.c_uint32(0)
        _check(lib().bhrt_photon_emit_range(self._h, C.byref(opts), int(bool(global_map)), C.c_uint64(e0), int(count), _ptr(out), int(capacity), C.byref(n)))
        return out[: n.value].copy()

    def photon_emit_range_into(self, opts: Opts, e0: int, count: int, out_ptr: int, capacity: int, global_map: bool = False):
        """Same, records written to `out_ptr` (host or device memory, room for `capacity` records).  Returns (n, ok): ok is False when
        n > capacity (nothing usable was written; call again with room for n)."""
        n = C.c_uint32(0)
        rc = lib().bhrt_photon_emit_range(self._h, C.byref(opts), int(bool(global_map)), C.c_uint64(e0), int(count), C.c_void_p(out_ptr), int(capacity), C.byref(n))
        if rc != 0 and n.value <= capacity:
            _check(rc)
        return n.value, rc == 0

    def photon_install_ptr(self, ptr: int, n: int) -> int:
        """Emission-order records at `ptr` (host or device memory) -> scaled, balanced and installed caustic map."""
        _check(lib().bhrt_photon_install(self._h, C.c_void_p(ptr), int(n)))
        return n

    def photon_install(self, records: np.ndarray) -> int:
        """Emission-order records (n, 24) -> scaled, balanced and installed caustic map."""
        r = np.ascontiguousarray(records, np.uint8).reshape(-1, 24)
        _check(lib().bhrt_photon_install(self._h, _ptr(r), len(r)))
        return len(r)

    def photon_build_global(self, opts: Opts, max_photons: int, dat_path=None) -> np.ndarray:
        """BuildPhotonMap (Main.cpp:251-295): the global photon map, balanced (n, 24) uint8 records."""
        out = np.zeros((max_photons, 24), np.uint8)
        n = C.c_uint32(0)
        _check(lib().bhrt_photon_build_global(self._h, C.byref(opts), int(max_photons), _ptr(out), int(max_photons), C.byref(n),
                                              os.fsencode(dat_path) if dat_path else None))
        return out[: n.value].copy()

    def photon_export(self, path: str):
        _check(lib().bhrt_photon_export(self._h, os.fsencode(path)))

    def photon_import(self, path: str, rebalance: bool = False):
        """Loads a .dat of 24-byte records; rebalance=True mirrors PhotonMap::InitializePhotonMapByFile."""
        _check(lib().bhrt_photon_import(self._h, os.fsencode(path), 1 if rebalance else 0))

    def render_samples(self, opts: Opts, x0, y0, x1, y1):
        out = np.zeros(((y1 - y0) * (x1 - x0), opts.spp, 3), np.float32)
        st = Stats()
        _check(lib().bhrt_render_samples(self._h, C.byref(opts), x0, y0, x1, y1, _ptr(out), C.byref(st)))
        return out, st


def math_eval_dev(fn: int, a, b=None):
    a = np.ascontiguousarray(a, np.float32)
    bb = np.ascontiguousarray(b, np.float32) if b is not None else None
    out = np.empty_like(a)
    _check(lib().bhrt_math_eval_dev(int(fn), _ptr(a), _ptr(bb) if bb is not None else None, C.c_size_t(a.size), _ptr(out)))
    return out


def tiles_block_bytes(width: int, height: int, tile: int, world: int) -> int:
    f = lib().bhrt_tiles_block_bytes
    f.restype = C.c_size_t
    return int(f(width, height, tile, world))


def bvh_build(vertices, faces, max_per_leaf=4, device=0):
    """cyBVH::Build on the device (bhrt_bvh_build): returns (nodes (n+1, 8) uint32 words of bhrt_bvh_node incl. the unused
    slot 0, element order (n_faces,) uint32, depth)."""
    v = np.ascontiguousarray(vertices, np.float32).reshape(-1, 3)
    f = np.ascontiguousarray(faces, np.uint32).reshape(-1, 3)
    nodes = np.zeros((2 * len(f) + 1, 8), np.uint32)
    elems = np.zeros(len(f), np.uint32)
    n, depth = C.c_uint32(0), C.c_uint32(0)
    _check(lib().bhrt_bvh_build(_ptr(v), len(v), _ptr(f), len(f), int(max_per_leaf), int(device), _ptr(nodes), len(nodes), C.byref(n), _ptr(elems),
                                C.byref(depth)))
    return nodes[: n.value + 1].copy(), elems, depth.value


def tiles_pack_dev(rgb8_ptr: int, radiance_ptr: int, width, height, tile, rank, world, block_ptr: int, stream: int = 0):
    _check(lib().bhrt_tiles_pack_dev(C.c_void_p(rgb8_ptr), C.c_void_p(radiance_ptr), width, height, tile, rank, world, C.c_void_p(block_ptr),
                                     C.c_void_p(stream)))


def tiles_unpack_dev(blocks_ptr: int, width, height, tile, world, rgb8_ptr: int, radiance_ptr: int, stream: int = 0):
    _check(lib().bhrt_tiles_unpack_dev(C.c_void_p(blocks_ptr), width, height, tile, world, C.c_void_p(rgb8_ptr), C.c_void_p(radiance_ptr),
                                       C.c_void_p(stream)))


def save_png(path: str, rgb8: np.ndarray):
    a = np.ascontiguousarray(rgb8, np.uint8)
    _check(lib().bhrt_save_png(os.fsencode(path), _ptr(a), a.shape[1], a.shape[0]))
