"""ctypes binding of the C-ABI in include/ptc.h (physically-based-renderer_amd/lib/libptc.so).

`PathTracer` is the drop-in for the reference's render seam: where the reference calls
`PbrRenderSystem::render(cmd, scene, gBuffer, renderTarget, extent)`
(src/pbr_engine/engine/pbr/PbrRenderSystem.hpp:46-47, called at src/gltf_viewer/App.cpp:387-388) after
`gltf::Asset::loadScene` (src/pbr_engine/gltf/pbr/gltf/Asset.hpp:76-78), a caller here does
`PathTracer(device).load_scene(desc).render(w, h, spp, ...)`.

HIP only.  There is no CPU fallback: if libptc.so is missing or no gfx950 device is usable this
module raises — loudly — instead of computing anything on the host.

A new entry point of include/ptc.h is declared here in three places at most: its prototype in `_prototypes()` (the only place that says what a
call passes; tests/test_binding_matches_header.py holds the table, the struct mirrors and the constants to the header), a `_Struct` mirror when it
brings a struct, and the method that calls it.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# PTC_LIB selects another build of the same library (the instrumented builds tools/diag.py and tools/stamp*.py read: profiles/instr_*.patch
# applied, built with EXTRA=-DPT_DIAG / -DPT_STAMP / -DPT_STAMP_SHADE)
LIB_PATH = os.environ.get("PTC_LIB") or os.path.join(os.path.dirname(_HERE), "lib", "libptc.so")

DEVICE_NONE = -1  # PTC_DEVICE_NONE: description-only context (host flatten + BVH build; renders nothing)
INTEGRATOR_PATH = 0
INTEGRATOR_RASTER_COMPAT = 1
INTEGRATOR_RASTER_GBUFFER16 = 2   # raster-compat lit from the reference's G-buffer formats (RGBA16F P/N, UNORM16 albedo)
COMM_ID_BYTES = 128
ABI_VERSION = 4
LIGHT_POINT = 0
LIGHT_SPOT = 1
LIGHT_DIRECTIONAL = 2
MAX_LIGHTS = 256
ALPHA_OPAQUE = 0          # glTF alphaMode (set_material_alpha)
ALPHA_MASK = 1
ALPHA_BLEND = 2
TONEMAP_ACES = 0          # the ACES fit of tonemap()
TONEMAP_PBR_NEUTRAL = 1   # Khronos PBR Neutral
TONEMAP_REINHARD = 2      # extended Reinhard on luminance
TONEMAP_CLAMP = 3
OETF_GAMMA22 = 0
OETF_SRGB = 1
LUMINANCE_BINS = 4096
GUIDE_ALBEDO = 0          # (albedo rgb, class: 0 miss, 1 surface, 2 emitter)
GUIDE_NORMAL_DEPTH = 1    # (unit vertex normal, t along the unit camera ray)
OUTPUT_RADIANCE = 0
OUTPUT_DENOISED = 1
OUTPUT_ACCUMULATED = 2    # the image of the frame's temporal_accumulate()
TEMPORAL_HISTORY = 0      # (D rgb, n)
TEMPORAL_MOMENTS = 1      # (m1, m2, Var_t, a)
TEMPORAL_MOTION = 2       # (x_prev, y_prev, W, reprojected n)
TEMPORAL_NORMAL_DEPTH = 3     # the history's copy of its frame's (N, Z)
TEMPORAL_POSITION_CLASS = 4   # the history's copy of its frame's (P, K)


class PtcError(RuntimeError):
    pass


class _Struct(C.Structure):
    """Base of the mirrors of include/ptc.h's structs.  A parameter struct names its ptc_*_default_params in `_defaults_`, says in `_unknown_` how it
    refuses a key that is no field, and lists in `_names_` the fields that also take a name for a value."""
    _defaults_ = None
    _unknown_ = "unknown field {}"
    _names_ = {}

    def as_dict(self):
        return {k: tuple(getattr(self, k)) if issubclass(t, C.Array) else getattr(self, k) for k, t in self._fields_}

    @classmethod
    def defaults(cls, **fields):
        """A new struct holding the library's defaults, with `fields` set on it."""
        if cls._defaults_ is None:
            raise TypeError(f"{cls.__name__} has no ptc_*_default_params")
        p = cls()
        getattr(load_library(), cls._defaults_)(C.byref(p))
        return p.update(**fields) if fields else p

    def update(self, **fields):
        """Set `fields` on this struct, in place, each converted by its field's ctype; TypeError for a key that is no field.  Returns self."""
        types = dict(self._fields_)
        for k, v in fields.items():
            if k not in types:
                raise TypeError(self._unknown_.format(k))
            if isinstance(v, str):
                if v not in self._names_.get(k, ()):
                    raise ValueError(f"{k}: {v!r} is not one of {sorted(self._names_.get(k, ()))}")
                v = self._names_[k][v]
            t = types[k]
            setattr(self, k, t(*[float(x) for x in v]) if issubclass(t, C.Array) else float(v) if t in (C.c_float, C.c_double) else int(v))
        return self


class PtcStats(_Struct):
    _fields_ = [
        ("paths", C.c_uint64), ("segments", C.c_uint64), ("shadow_rays", C.c_uint64), ("hits", C.c_uint64),
        ("node_visits_closest", C.c_uint64), ("tri_tests_closest", C.c_uint64),
        ("node_visits_any", C.c_uint64), ("tri_tests_any", C.c_uint64), ("algorithmic_bytes", C.c_uint64),
        ("seconds_render", C.c_double), ("seconds_trace_closest", C.c_double), ("seconds_trace_any", C.c_double),
        ("seconds_shade", C.c_double), ("seconds_commit", C.c_double), ("seconds_reduce", C.c_double), ("seconds_refit", C.c_double),
        ("launches_trace_closest", C.c_uint32), ("launches_trace_any", C.c_uint32),
        ("n_triangles", C.c_uint32), ("n_bvh_nodes", C.c_uint32), ("n_emitters", C.c_uint32), ("bvh_max_depth", C.c_uint32),
        ("bvh_sa_cost", C.c_double), ("bvh_sa_cost_built", C.c_double), ("seconds_rebuild", C.c_double),
    ]


class PtcLensParams(_Struct):
    _fields_ = [("aperture_radius", C.c_float), ("focus_distance", C.c_float), ("blades", C.c_int), ("rotation", C.c_float)]
    _defaults_ = "ptc_lens_default_params"


_PROJECTIONS = {"perspective": 0, "orthographic": 1, "equirect": 2}      # PTC_PROJ_* of include/ptc_camera.h


class PtcCameraParams(_Struct):
    _fields_ = [("projection", C.c_int), ("camera_to_world", C.c_float * 16), ("yfov", C.c_float), ("aspect", C.c_float), ("xmag", C.c_float), ("ymag", C.c_float)]
    _defaults_ = "ptc_camera_default_params"
    _unknown_ = "unknown camera field {}"
    _names_ = {"projection": _PROJECTIONS}


_ALPHA_MODES = {"opaque": ALPHA_OPAQUE, "mask": ALPHA_MASK, "blend": ALPHA_BLEND}
_LIGHT_TYPES = {"point": LIGHT_POINT, "spot": LIGHT_SPOT, "directional": LIGHT_DIRECTIONAL, "sun": LIGHT_DIRECTIONAL}


class PtcLightParams(_Struct):
    _fields_ = [("type", C.c_int), ("position", C.c_float * 3), ("direction", C.c_float * 3), ("intensity", C.c_float * 3), ("range", C.c_float),
                ("cos_inner", C.c_float), ("cos_outer", C.c_float), ("sampling_weight", C.c_float)]
    _defaults_ = "ptc_light_default_params"
    _names_ = {"type": _LIGHT_TYPES}


class PtcAlphaStats(_Struct):
    _fields_ = [("closest_passes", C.c_uint64), ("shadow_walked", C.c_uint64), ("shadow_passes", C.c_uint64), ("exhausted", C.c_uint64), ("seconds_alpha", C.c_double)]


class PtcTransmissionParams(_Struct):
    _fields_ = [("transmission", C.c_float), ("ior", C.c_float), ("thin_walled", C.c_int), ("attenuation_color", C.c_float * 3), ("attenuation_distance", C.c_float)]
    _defaults_ = "ptc_transmission_default_params"
    _unknown_ = "unknown transmission field {}"


class PtcGlassStats(_Struct):
    _fields_ = [("reflections", C.c_uint64), ("refractions", C.c_uint64), ("standing", C.c_uint64), ("exhausted", C.c_uint64), ("seconds_glass", C.c_double)]


class PtcGlassInteraction(_Struct):
    _fields_ = [("P", C.c_float * 3), ("ng", C.c_float * 3), ("ns", C.c_float * 3), ("front", C.c_int), ("d", C.c_float * 3), ("T", C.c_float * 3), ("t", C.c_float),
                ("base", C.c_float * 3), ("metallic", C.c_float), ("u_s", C.c_float), ("u_e", C.c_float), ("j", C.c_uint32), ("max_interactions", C.c_uint32),
                ("ray_eps", C.c_float), ("outcome", C.c_int), ("o_out", C.c_float * 3), ("d_out", C.c_float * 3), ("T_out", C.c_float * 3), ("F", C.c_float)]


class PtcEmissiveTexStats(_Struct):
    _fields_ = [("entries", C.c_uint64), ("hit_additions", C.c_uint64), ("shadow_records", C.c_uint64), ("seconds_emissive_tex", C.c_double)]


class PtcEmissiveTexSample(_Struct):
    _fields_ = [("P", C.c_float * 3), ("r1", C.c_float), ("r2", C.c_float), ("hit_u", C.c_float), ("hit_v", C.c_float), ("bounce", C.c_uint32),
                ("prev_pdf", C.c_float), ("hit_t", C.c_float), ("hit_cos", C.c_float), ("ok", C.c_int), ("y", C.c_float * 3), ("wi", C.c_float * 3),
                ("pl", C.c_float), ("Le", C.c_float * 3), ("hit_Le", C.c_float * 3), ("hit_weight", C.c_float)]
    _unknown_ = "unknown emissive-texture sample field {}"


class PtcGlassShadowStats(_Struct):
    _fields_ = [("walked", C.c_uint64), ("passes", C.c_uint64), ("visible", C.c_uint64), ("exhausted", C.c_uint64)]


class PtcGlassShadowHit(_Struct):
    _fields_ = [("ng", C.c_float * 3), ("ns", C.c_float * 3), ("d", C.c_float * 3), ("base", C.c_float * 3), ("metallic", C.c_float), ("W", C.c_float * 3), ("F_t", C.c_float)]


class PtcMediumParams(_Struct):
    _fields_ = [("box_lo", C.c_float * 3), ("box_hi", C.c_float * 3), ("sigma_t", C.c_float), ("albedo", C.c_float * 3), ("g", C.c_float)]
    _unknown_ = "unknown medium field {}"


class PtcMediumStats(_Struct):
    _fields_ = [("crossed", C.c_uint64), ("scattered", C.c_uint64), ("attenuated", C.c_uint64), ("seconds_medium", C.c_double)]


class PtcLightmapDesc(_Struct):
    _fields_ = [("instance", C.c_int), ("width", C.c_int), ("height", C.c_int), ("uv", C.POINTER(C.c_float)), ("texel_index_base", C.c_uint32), ("spp_total", C.c_int),
                ("seed", C.c_uint64), ("max_bounces", C.c_int)]


class PtcMediumSample(_Struct):
    _fields_ = [("o", C.c_float * 3), ("d", C.c_float * 3), ("t_end", C.c_float), ("u0", C.c_float), ("u1", C.c_float), ("u2", C.c_float),
                ("so", C.c_float * 3), ("sd", C.c_float * 3), ("stmax", C.c_float), ("crosses", C.c_int), ("t0", C.c_float), ("t1", C.c_float), ("s", C.c_float),
                ("scatters", C.c_int), ("P", C.c_float * 3), ("cos_theta", C.c_float), ("wi", C.c_float * 3), ("pdf", C.c_float), ("transmittance", C.c_float)]


class PtcDenoiseParams(_Struct):
    _fields_ = [("iterations", C.c_int), ("sigma_l", C.c_float), ("sigma_n", C.c_float), ("sigma_p", C.c_float), ("demodulate", C.c_int)]
    _defaults_ = "ptc_denoise_default_params"
    _unknown_ = "denoise: unknown parameter {}"


class PtcAdaptiveParams(_Struct):
    _fields_ = [("threshold", C.c_float), ("radius", C.c_int), ("min_samples", C.c_int), ("step_samples", C.c_int)]
    _defaults_ = "ptc_adaptive_default_params"
    _unknown_ = "adaptive sampling: unknown parameter {}"


class PtcAdaptiveStats(_Struct):
    _fields_ = [("owned_pixels", C.c_uint64), ("active_pixels", C.c_uint64), ("samples_total", C.c_uint64),
                ("passes", C.c_uint32), ("max_count", C.c_uint32), ("seconds_adapt", C.c_double)]


class PtcTemporalParams(_Struct):
    _fields_ = [("max_history", C.c_int), ("sigma_z", C.c_float), ("demodulate", C.c_int)]
    _defaults_ = "ptc_temporal_default_params"
    _unknown_ = "temporal_accumulate: unknown parameter {}"


_TONEMAPS = {"aces": TONEMAP_ACES, "neutral": TONEMAP_PBR_NEUTRAL, "pbr_neutral": TONEMAP_PBR_NEUTRAL, "reinhard": TONEMAP_REINHARD, "clamp": TONEMAP_CLAMP}
_OETFS = {"gamma22": OETF_GAMMA22, "srgb": OETF_SRGB}


class PtcDisplayParams(_Struct):
    _fields_ = [("gain", C.c_float), ("auto_exposure", C.c_int), ("key", C.c_float), ("percentile_lo", C.c_float), ("percentile_hi", C.c_float),
                ("adapt_rate", C.c_float), ("min_luminance", C.c_float), ("max_luminance", C.c_float), ("tonemap", C.c_int), ("white", C.c_float), ("oetf", C.c_int)]
    _defaults_ = "ptc_display_default_params"
    _unknown_ = "display parameters: unknown field {}"
    _names_ = {"tonemap": _TONEMAPS, "oetf": _OETFS}


def _prototypes():
    """name -> (restype, argtypes) of every function include/ptc.h declares, section by section in the header's order."""
    i, f, u32, u64, s = C.c_int, C.c_float, C.c_uint32, C.c_uint64, C.c_char_p
    vp, ip, fp, dp = C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_float), C.POINTER(C.c_double)
    u8p, u16p, u32p, u64p, i32p = C.POINTER(C.c_uint8), C.POINTER(C.c_uint16), C.POINTER(C.c_uint32), C.POINTER(C.c_uint64), C.POINTER(C.c_int32)
    lens, light, display = C.POINTER(PtcLensParams), C.POINTER(PtcLightParams), C.POINTER(PtcDisplayParams)
    denoise, adaptive, temporal = C.POINTER(PtcDenoiseParams), C.POINTER(PtcAdaptiveParams), C.POINTER(PtcTemporalParams)
    return {
        # context
        "ptc_create": (vp, [i]),
        "ptc_destroy": (None, [vp]),
        "ptc_last_error": (s, [vp]),
        "ptc_abi_version": (i, []),
        "ptc_build_info": (s, []),
        "ptc_launch_policy": (s, [vp]),
        # scene description
        "ptc_scene_begin": (i, [vp]),
        "ptc_add_material": (i, [vp, fp, f, f, fp, i, i, i]),
        "ptc_add_texture_rgba8": (i, [vp, u8p, i, i]),
        "ptc_add_mesh": (i, [vp, vp, u32, u32p, u32, i]),
        "ptc_add_instance": (i, [vp, i, fp, fp, fp]),
        "ptc_add_instance_matrix": (i, [vp, i, fp]),
        "ptc_update_instance": (i, [vp, i, fp, fp, fp]),
        "ptc_update_instance_matrix": (i, [vp, i, fp]),
        "ptc_scene_refit": (i, [vp]),
        "ptc_scene_rebuild": (i, [vp]),
        # deforming meshes
        "ptc_mesh_set_morph_targets": (i, [vp, i, u32, fp, fp, fp]),
        "ptc_mesh_set_skin": (i, [vp, i, u32, u16p, fp]),
        "ptc_update_mesh_pose": (i, [vp, i, fp, u32, fp, u32]),
        "ptc_update_mesh_vertices": (i, [vp, i, vp, u32]),
        # camera and thin lens
        "ptc_set_camera": (i, [vp, fp, fp, f, f]),
        "ptc_lens_default_params": (None, [lens]),
        "ptc_set_camera_lens": (i, [vp, lens]),
        "ptc_get_camera_lens": (i, [vp, lens]),
        "ptc_focus_distance_at_pixel": (i, [vp, i, i, fp]),
        # punctual lights
        "ptc_light_default_params": (None, [light]),
        "ptc_add_light": (i, [vp, light]),
        "ptc_update_light": (i, [vp, i, light]),
        "ptc_get_light": (i, [vp, i, light]),
        "ptc_light_count": (i, [vp]),
        "ptc_clear_lights": (i, [vp]),
        # environment, texture filter, builders, commit
        "ptc_set_env_latlong_rgb32f": (i, [vp, fp, i, i]),
        "ptc_set_texture_filter": (i, [vp, i]),
        "ptc_set_bvh_builder": (i, [vp, i]),
        "ptc_set_device_builder": (i, [vp, i]),
        "ptc_scene_commit": (i, [vp]),
        # rendering
        "ptc_render": (i, [vp, i, i, i, u64, i, i]),
        "ptc_frame_begin": (i, [vp, i, i, i, u64, i, i, i, i]),
        "ptc_frame_add_samples": (i, [vp, i]),
        "ptc_frame_reserve": (i, [vp]),
        "ptc_frame_resolve": (i, [vp]),
        "ptc_sync": (i, [vp]),
        "ptc_read_radiance_rgba32f": (i, [vp, fp]),
        "ptc_radiance_device_ptr": (vp, [vp]),
        "ptc_write_radiance_rgba32f": (i, [vp, fp]),
        "ptc_read_radiance_rgba16f": (i, [vp, u16p]),
        "ptc_radiance_rgba16f_device_ptr": (vp, [vp]),
        "ptc_tonemap_rgba8": (i, [vp, u8p]),
        # checkpoint / resume, sample ranges, counters
        "ptc_frame_checkpoint": (i, [vp, fp, u64p, u32p]),
        "ptc_frame_restore": (i, [vp, fp, u64, u32]),
        "ptc_frame_set_sample_range": (i, [vp, u32, u32]),
        "ptc_get_stats": (i, [vp, C.POINTER(PtcStats)]),
        # guide buffers, denoiser, output selection
        "ptc_frame_guides": (i, [vp]),
        "ptc_read_guide_rgba32f": (i, [vp, i, fp]),
        "ptc_read_guide_hit": (i, [vp, i32p, fp]),
        "ptc_denoise_default_params": (None, [denoise]),
        "ptc_denoise": (i, [vp, denoise]),
        "ptc_select_output": (i, [vp, i]),
        "ptc_get_denoise_seconds": (i, [vp, dp, dp]),
        # adaptive sampling
        "ptc_adaptive_default_params": (None, [adaptive]),
        "ptc_frame_set_adaptive": (i, [vp, adaptive]),
        "ptc_frame_adapt": (i, [vp, u64p]),
        "ptc_read_sample_counts": (i, [vp, u32p]),
        "ptc_render_adaptive": (i, [vp, i, i, i, u64, i, adaptive]),
        "ptc_get_adaptive_stats": (i, [vp, C.POINTER(PtcAdaptiveStats)]),
        # denoising from per-sample statistics
        "ptc_set_sample_covariance": (i, [vp, i]),
        "ptc_read_sample_covariance": (i, [vp, fp]),
        "ptc_denoise_sampled": (i, [vp, denoise]),
        "ptc_read_sampled_variance": (i, [vp, fp]),
        # temporal accumulation
        "ptc_temporal_default_params": (None, [temporal]),
        "ptc_temporal_accumulate": (i, [vp, temporal]),
        "ptc_temporal_reset": (i, [vp]),
        "ptc_read_temporal_rgba32f": (i, [vp, i, fp]),
        "ptc_denoise_accumulated": (i, [vp, denoise]),
        "ptc_get_temporal_seconds": (i, [vp, dp]),
        # display transform
        "ptc_display_default_params": (None, [display]),
        "ptc_set_display": (i, [vp, display]),
        "ptc_get_display": (i, [vp, display]),
        "ptc_meter_exposure": (i, [vp]),
        "ptc_exposure_reset": (i, [vp]),
        "ptc_get_exposure": (i, [vp, fp, fp, fp, u64p, u64p]),
        "ptc_read_luminance_histogram": (i, [vp, u32p]),
        "ptc_display_rgba8": (i, [vp, u8p]),
        "ptc_display_rgba16f": (i, [vp, u16p]),
        "ptc_display_rgba16f_device_ptr": (vp, [vp]),
        "ptc_get_display_seconds": (i, [vp, dp, dp]),
        # light probes
        "ptc_probes_begin": (i, [vp, fp, i, u32, i, u64, i]),
        "ptc_probes_read_sh": (i, [vp, fp]),
        "ptc_render_probes": (i, [vp, fp, i, i, u64, i, fp]),
        "ptc_sh9_eval": (i, [fp, fp, fp]),
        "ptc_sh9_irradiance": (i, [fp, fp, fp]),
        # multi-GPU: one process per GPU
        "ptc_comm_unique_id": (i, [u8p]),
        "ptc_comm_init": (i, [vp, u8p, i, i]),
        "ptc_comm_reduce_radiance": (i, [vp, i]),
        "ptc_comm_destroy": (i, [vp]),
        # multi-GPU: one process driving several GPUs
        "ptc_group_create": (vp, [ip, i]),
        "ptc_group_size": (i, [vp]),
        "ptc_group_scene_commit": (i, [vp]),
        "ptc_group_scene_refit": (i, [vp]),
        "ptc_group_ctx": (vp, [vp, i]),
        "ptc_group_render": (i, [vp, i, i, i, u64, i, i]),
        "ptc_group_last_error": (s, [vp]),
        "ptc_group_destroy": (None, [vp]),
        # test hooks
        "ptc_debug_trace_closest": (i, [vp, fp, fp, u32, fp, i32p, fp]),
        "ptc_debug_trace_any": (i, [vp, fp, fp, fp, u32, u8p]),
        "ptc_debug_lens_sample": (i, [lens, f, f, fp]),
        "ptc_debug_light_sample": (i, [light, fp, fp, fp, fp]),
        "ptc_debug_get_light_table": (i, [vp, u32p, fp, fp]),
        "ptc_debug_punctual_nee": (i, [vp, fp, fp, u32p, u32, u32, u8p, fp, fp, fp, fp]),
        "ptc_debug_display_pixel": (i, [display, f, fp, u8p, u16p]),
        "ptc_debug_meter": (i, [display, fp, u64, u32, u32p, u32p, u64p, u64p, u64p, u32p]),
        "ptc_debug_display_internals": (i, [vp, u64p]),
        "ptc_debug_display_state": (i, [vp, u32p]),
        "ptc_debug_camera_rays": (i, [vp, i, i, u64, u32, u32, u32p, u32, fp, fp]),
        "ptc_debug_probe_rays": (i, [vp, fp, i, u32, u64, u32, u32, fp, u32p]),
        "ptc_debug_probe_project": (i, [vp, i, u32, u64, u32, u32, fp, fp]),
        "ptc_debug_probe_resolve": (i, [fp, i, u32, fp]),
        "ptc_debug_get_flat_scene": (i, [vp, u32p, u32p, vp, u32p, i32p]),
        "ptc_debug_get_mesh_vertices": (i, [vp, i, vp]),
        "ptc_debug_get_description": (i, [vp, ip, ip]),
        "ptc_debug_get_material": (i, [vp, i, fp, ip]),
        "ptc_debug_get_texture": (i, [vp, i, ip, ip, vp]),
        "ptc_debug_get_counters": (i, [vp, u64p, i]),
        "ptc_debug_get_bvh": (i, [vp, u32p, u32p, u32p, fp, fp]),
        "ptc_debug_host_build_id": (u64, [vp]),
        "ptc_debug_get_internals": (i, [vp, u64p]),
        "ptc_debug_commit_host_parts": (i, [vp, u64p]),
        "ptc_debug_get_shading_tables": (i, [vp, u32p, fp, u32p, fp, fp]),
        "ptc_debug_refit_host_parts": (i, [vp, u64p]),
    }


def _alpha_prototypes():
    """name -> (restype, argtypes) of every function include/ptc_alpha.h declares, in the header's order.  The library exports them under the prefix ptcx_ (the
    header maps the names by macros): load_library looks them up there and hangs them on the library object under the names the header gives them."""
    i, f, u32 = C.c_int, C.c_float, C.c_uint32
    vp, ip, fp = C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_float)
    u32p, i32p = C.POINTER(C.c_uint32), C.POINTER(C.c_int32)
    return {
        "ptc_set_material_alpha": (i, [vp, i, i, f]),
        "ptc_get_material_alpha": (i, [vp, i, ip, fp]),
        "ptc_set_alpha_max_layers": (i, [vp, i]),
        "ptc_get_alpha_stats": (i, [vp, C.POINTER(PtcAlphaStats)]),
        "ptc_debug_alpha_closest": (i, [vp, fp, fp, u32p, u32, u32, i, fp, i32p, fp, u32p]),
        "ptc_debug_alpha_any": (i, [vp, fp, fp, fp, u32, fp]),
        "ptc_debug_alpha_decide": (i, [i, f, f, f, ip, fp]),
        "ptc_debug_get_alpha_tables": (i, [vp, u32p, u32p, u32p, fp]),
    }


def _glass_prototypes():
    """name -> (restype, argtypes) of every function include/ptc_glass.h declares, in the header's order; exported under ptcx_ like ptc_alpha.h's."""
    i, u32 = C.c_int, C.c_uint32
    vp, fp = C.c_void_p, C.POINTER(C.c_float)
    u32p, i32p = C.POINTER(C.c_uint32), C.POINTER(C.c_int32)
    tp = C.POINTER(PtcTransmissionParams)
    return {
        "ptc_transmission_default_params": (None, [tp]),
        "ptc_set_material_transmission": (i, [vp, i, tp]),
        "ptc_get_material_transmission": (i, [vp, i, tp]),
        "ptc_set_glass_max_interactions": (i, [vp, i]),
        "ptc_get_glass_stats": (i, [vp, C.POINTER(PtcGlassStats)]),
        "ptc_debug_glass_closest": (i, [vp, fp, fp, u32p, u32, u32, fp, i32p, fp, fp, u32p]),
        "ptc_debug_glass_interact": (i, [tp, C.POINTER(PtcGlassInteraction)]),
        "ptc_debug_get_glass_tables": (i, [vp, u32p, u32p, u32p, fp]),
    }


def _glass_shadow_prototypes():
    """name -> (restype, argtypes) of every function include/ptc_glass_shadows.h declares, in the header's order; exported under ptcx_ like ptc_glass.h's."""
    i, u32 = C.c_int, C.c_uint32
    vp, ip, fp, u32p = C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_float), C.POINTER(C.c_uint32)
    return {
        "ptc_set_glass_shadows": (i, [vp, i]),
        "ptc_get_glass_shadows": (i, [vp, ip]),
        "ptc_get_glass_shadow_stats": (i, [vp, C.POINTER(PtcGlassShadowStats)]),
        "ptc_debug_glass_any": (i, [vp, fp, fp, fp, u32, fp, u32p]),
        "ptc_debug_glass_shadow_transmit": (i, [C.POINTER(PtcTransmissionParams), C.POINTER(PtcGlassShadowHit)]),
    }


def _shade_debug_prototypes():
    """name -> (restype, argtypes) of every function include/ptc_shade_debug.h declares, in the header's order; exported under ptcx_ like ptc_alpha.h's."""
    i, u32 = C.c_int, C.c_uint32
    vp, ip, fp, u8p, u32p = C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_float), C.POINTER(C.c_uint8), C.POINTER(C.c_uint32)
    return {
        "ptc_debug_shade_step": (i, [vp, fp, fp, fp, fp, u32p, u32, u32, u32, i, fp, fp, u8p, fp, u8p, fp]),
        "ptc_debug_get_env_tables": (i, [vp, ip, ip, ip, fp, fp, fp]),
    }


def _exact_debug_prototypes():
    """name -> (restype, argtypes) of the function include/ptc_exact_debug.h declares; exported under ptcx_ like ptc_shade_debug.h's."""
    i, u32, u64 = C.c_int, C.c_uint32, C.c_uint64
    vp, fp, u64p = C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_uint64)
    return {
        "ptc_debug_exact_arith": (i, [vp, i, fp, fp, u64, u32, i, u64p]),
    }


def _medium_prototypes():
    """name -> (restype, argtypes) of every function include/ptc_medium.h declares, in the header's order; exported under ptcx_ like ptc_glass.h's."""
    i, u32 = C.c_int, C.c_uint32
    vp, fp, u8p, u32p = C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_uint8), C.POINTER(C.c_uint32)
    mp = C.POINTER(PtcMediumParams)
    return {
        "ptc_set_medium": (i, [vp, mp]),
        "ptc_get_medium": (i, [vp, mp]),
        "ptc_clear_medium": (i, [vp]),
        "ptc_get_medium_stats": (i, [vp, C.POINTER(PtcMediumStats)]),
        "ptc_debug_medium_sample": (i, [mp, C.POINTER(PtcMediumSample)]),
        "ptc_debug_medium_step": (i, [vp, fp, fp, fp, fp, u32p, u32, u32, u32, fp, u8p, fp, u8p, fp, u8p, fp]),
        "ptc_debug_medium_env": (i, [vp, fp, fp, fp, u32, fp, fp, fp]),
    }


def _lightmap_prototypes():
    """name -> (restype, argtypes) of every function include/ptc_lightmap.h declares, in the header's order; exported under ptcx_ like ptc_medium.h's."""
    i, u32 = C.c_int, C.c_uint32
    vp, fp, u32p = C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_uint32)
    dp = C.POINTER(PtcLightmapDesc)
    return {
        "ptc_lightmap_begin": (i, [vp, dp]),
        "ptc_lightmap_texel_count": (i, [vp, u32p, u32p]),
        "ptc_lightmap_read_texels": (i, [vp, u32p, u32p, fp, fp]),
        "ptc_lightmap_read": (i, [vp, i, C.c_float, fp, fp]),
        "ptc_render_lightmap": (i, [vp, dp, i, C.c_float, fp]),
        "ptc_debug_lightmap_cover": (i, [vp, u32p, u32, fp, u32, i, i, u32p]),
        "ptc_debug_lightmap_rays": (i, [vp, dp, u32, u32, u32p, u32p, u32p, fp, fp, fp, u32p]),
        "ptc_debug_lightmap_dilate": (i, [vp, i, i, i, fp]),
    }


def _emissive_tex_prototypes():
    """name -> (restype, argtypes) of every function include/ptc_emissive_tex.h declares, in the header's order; exported under ptcx_ like ptc_glass.h's."""
    i, u32 = C.c_int, C.c_uint32
    vp, ip, fp, u8p, u32p, i32p = C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_float), C.POINTER(C.c_uint8), C.POINTER(C.c_uint32), C.POINTER(C.c_int32)
    return {
        "ptc_set_material_emission_texture": (i, [vp, i, i, fp]),
        "ptc_get_material_emission_texture": (i, [vp, i, ip, fp]),
        "ptc_get_emissive_tex_stats": (i, [vp, C.POINTER(PtcEmissiveTexStats)]),
        "ptc_debug_get_emissive_tex_table": (i, [vp, u32p, fp, fp, u32p, i32p, fp]),
        "ptc_debug_emissive_tex_sample": (i, [fp, u8p, i, i, i, C.POINTER(PtcEmissiveTexSample)]),
        "ptc_debug_emissive_tex_step": (i, [vp, fp, fp, fp, fp, u32p, u32, u32, u32, fp, u8p, fp]),
    }


def _camera_prototypes():
    """name -> (restype, argtypes) of every function include/ptc_camera.h declares, in the header's order; exported under ptcx_ like ptc_medium.h's."""
    cp = C.POINTER(PtcCameraParams)
    return {
        "ptc_camera_default_params": (None, [cp]),
        "ptc_set_camera_ex": (C.c_int, [C.c_void_p, cp]),
        "ptc_get_camera_ex": (C.c_int, [C.c_void_p, cp]),
        "ptc_debug_read_guide_positions": (C.c_int, [C.c_void_p, C.POINTER(C.c_float)]),
    }


_PROTOTYPES = _prototypes()
_CAMERA_PROTOTYPES = _camera_prototypes()
_EMISSIVE_TEX_PROTOTYPES = _emissive_tex_prototypes()
_LIGHTMAP_PROTOTYPES = _lightmap_prototypes()
_MEDIUM_PROTOTYPES = _medium_prototypes()
_ALPHA_PROTOTYPES = _alpha_prototypes()
_GLASS_PROTOTYPES = _glass_prototypes()
_GLASS_SHADOW_PROTOTYPES = _glass_shadow_prototypes()
_SHADE_DEBUG_PROTOTYPES = _shade_debug_prototypes()
_EXACT_DEBUG_PROTOTYPES = _exact_debug_prototypes()
# every function include/ptc_glass.h declares, by the header's names
GLASS_SYMBOLS = list(_GLASS_PROTOTYPES)
# every function include/ptc_alpha.h declares, by the header's names
ALPHA_SYMBOLS = list(_ALPHA_PROTOTYPES)
# every symbol include/ptc.h declares (tests check the library exports all of them)
ABI_SYMBOLS = list(_PROTOTYPES)

_lib = None


def load_library():
    """Load libptc.so and declare the prototypes.  Raises PtcError when the HIP library is not built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise PtcError(f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                       "(hipcc --offload-arch=gfx950); there is no CPU fallback")
    L = C.CDLL(LIB_PATH)
    for name, (restype, argtypes) in _PROTOTYPES.items():
        fn = getattr(L, name)
        fn.restype, fn.argtypes = restype, argtypes
    for name, (restype, argtypes) in list(_ALPHA_PROTOTYPES.items()) + list(_GLASS_PROTOTYPES.items()) + list(_GLASS_SHADOW_PROTOTYPES.items()) + list(_SHADE_DEBUG_PROTOTYPES.items()) + list(_EXACT_DEBUG_PROTOTYPES.items()) + list(_MEDIUM_PROTOTYPES.items()) + list(_LIGHTMAP_PROTOTYPES.items()) + list(_EMISSIVE_TEX_PROTOTYPES.items()) + list(_CAMERA_PROTOTYPES.items()):
        fn = getattr(L, "ptcx_" + name[len("ptc_"):])
        fn.restype, fn.argtypes = restype, argtypes
        setattr(L, name, fn)
    _lib = L
    return L


# the pointer type of an array's elements; anything else (MESH_VERTEX records) goes as void*
_POINTERS = {np.dtype(t): C.POINTER(c) for t, c in ((np.float32, C.c_float), (np.uint8, C.c_uint8), (np.uint16, C.c_uint16), (np.uint32, C.c_uint32),
                                                    (np.int32, C.c_int32), (np.uint64, C.c_uint64))}


def _ptr(a):
    return a.ctypes.data_as(_POINTERS.get(a.dtype, C.c_void_p))


def _f(a):
    a = np.ascontiguousarray(a, np.float32)
    return a, _ptr(a)


def camera_default_params():
    return PtcCameraParams.defaults().as_dict()


def look_at_matrix(position, target, up=(0.0, 1.0, 0.0)):
    """The camera-to-world matrix (4x4 float64) of a glTF camera at `position` that looks at `target` with `up` upwards in the image."""
    pos, tgt, up = (np.asarray(v, np.float64) for v in (position, target, up))
    z = pos - tgt
    z /= np.linalg.norm(z)
    x = np.cross(up, z)
    x /= np.linalg.norm(x)
    m = np.eye(4)
    m[:3, 0], m[:3, 1], m[:3, 2], m[:3, 3] = x, np.cross(z, x), z, pos
    return m


def _camera_ex_fields(cam):
    """set_camera_ex's arguments for a scene.CameraDesc with a matrix or a projection of its own.  Without a matrix: the panorama is taken at the camera's
    position with the identity rotation, the other projections look from position to target with +Y up."""
    projection = getattr(cam, "projection", "perspective")
    matrix = getattr(cam, "matrix", None)
    if matrix is None:
        matrix = look_at_matrix(cam.position, cam.target)
        if projection == "equirect":
            matrix[:3, :3] = np.eye(3)
    fields = dict(matrix=matrix, projection=projection)
    if projection == "perspective":
        fields.update(yfov=cam.fov_y, aspect=cam.aspect)
    elif projection == "orthographic":
        fields.update(xmag=cam.xmag, ymag=cam.ymag)
    return fields


def lens_default_params():
    return PtcLensParams.defaults().as_dict()


def lens_sample(u1, u2, aperture_radius=1.0, blades=0, rotation=0.0):
    """ptc_debug_lens_sample: the aperture point (lx, ly) of the pair (u1, u2) in [0,1)^2, the host's evaluation of csrc/pt_lens.h.  Scalars give a pair,
    arrays an (n, 2) float32 array."""
    L = load_library()
    p = PtcLensParams(aperture_radius, 1.0, int(blades), rotation)
    a, b = np.atleast_1d(np.asarray(u1, np.float32)), np.atleast_1d(np.asarray(u2, np.float32))
    out = np.zeros((a.size, 2), np.float32)
    xy = (C.c_float * 2)()
    for i in range(a.size):
        if L.ptc_debug_lens_sample(C.byref(p), float(a[i]), float(b[i]), xy) < 0:
            raise PtcError(f"lens_sample: bad lens parameters or u outside [0, 1): {p.as_dict()}, ({a[i]}, {b[i]})")
        out[i] = xy[0], xy[1]
    return out if np.ndim(u1) else (float(out[0, 0]), float(out[0, 1]))


def _sh9_apply(fn, name, sh, vecs):
    sh = np.ascontiguousarray(sh, np.float32)
    v = np.ascontiguousarray(vecs, np.float32)
    if sh.shape[-2:] != (9, 3) or v.shape[-1:] != (3,):
        raise PtcError(f"{name}: sh must end in (9, 3) and the directions in (3,), got {sh.shape} and {v.shape}")
    lead = np.broadcast_shapes(sh.shape[:-2], v.shape[:-1])
    shb = np.ascontiguousarray(np.broadcast_to(sh, lead + (9, 3))).reshape(-1, 27)
    vb = np.ascontiguousarray(np.broadcast_to(v, lead + (3,))).reshape(-1, 3)
    out = np.zeros((shb.shape[0], 3), np.float32)
    for i in range(shb.shape[0]):
        if fn(_ptr(shb[i]), _ptr(vb[i]), _ptr(out[i])) < 0:
            raise PtcError(f"{name}: bad argument")
    return out.reshape(lead + (3,))


def sh9_eval(sh, dirs):
    """ptc_sh9_eval: the radiance sum_k sh_k Y_k(dir) of SH9 coefficients sh (..., 9, 3) from the unit directions dirs (..., 3); leading shapes broadcast;
    (..., 3) float32.  The host's evaluation of csrc/pt_probes.h."""
    return _sh9_apply(load_library().ptc_sh9_eval, "sh9_eval", sh, dirs)


def sh9_irradiance(sh, normals):
    """ptc_sh9_irradiance: the irradiance on a surface with the unit normals (..., 3) under the radiance the SH9 coefficients sh (..., 9, 3) describe
    (Ramamoorthi-Hanrahan: A = pi, 2 pi / 3, pi / 4 per band); (..., 3) float32."""
    return _sh9_apply(load_library().ptc_sh9_irradiance, "sh9_irradiance", sh, normals)


def probe_resolve(acc, n_samples):
    """ptc_debug_probe_resolve: running sums (n, 9, 3) -> coefficients, acc * (4 pi / n_samples) in float32."""
    a = np.ascontiguousarray(acc, np.float32).reshape(-1, 9, 3)
    out = np.zeros_like(a)
    if load_library().ptc_debug_probe_resolve(_ptr(a), a.shape[0], int(n_samples), _ptr(out)) < 0:
        raise PtcError("probe_resolve: bad argument")
    return out


def light_params(type="point", position=(0, 0, 0), direction=(0, 0, -1), intensity=(1, 1, 1), range=0.0, cos_inner=1.0, cos_outer=0.70710678, sampling_weight=1.0):
    """A ptc_light_params: `type` is a name (point, spot, directional) or a LIGHT_* value; an object with these attributes (scene.LightDesc) is taken by light_params_of."""
    return PtcLightParams().update(type=type, position=position, direction=direction, intensity=intensity, range=range, cos_inner=cos_inner,
                                    cos_outer=cos_outer, sampling_weight=sampling_weight)


def light_params_of(l):
    if isinstance(l, PtcLightParams):
        return l
    if isinstance(l, dict):
        return light_params(**l)
    return light_params(l.type, l.position, l.direction, l.intensity, l.range, l.cos_inner, l.cos_outer, l.sampling_weight)


def light_default_params():
    return PtcLightParams.defaults().as_dict()


def light_sample(light, P):
    """ptc_debug_light_sample: the host's evaluation of csrc/pt_lights.h for one light (light_params / LightDesc / dict) and the points P (n, 3):
    (has_sample (n,) bool, wi (n, 3), dist (n,), Li (n, 3)), float32; rows without a sample are 0."""
    L = load_library()
    p = light_params_of(light)
    pts = np.ascontiguousarray(np.atleast_2d(np.asarray(P, np.float32)))
    n = pts.shape[0]
    ok, wi, dist, Li = np.zeros(n, bool), np.zeros((n, 3), np.float32), np.zeros(n, np.float32), np.zeros((n, 3), np.float32)
    w, li, d = (C.c_float * 3)(), (C.c_float * 3)(), C.c_float(0)
    for i in range(n):
        rc = L.ptc_debug_light_sample(C.byref(p), _ptr(pts[i]), w, C.byref(d), li)
        if rc < 0:
            raise PtcError(f"light_sample: bad light parameters: {p.as_dict()}")
        if rc:
            ok[i], wi[i], dist[i], Li[i] = True, tuple(w), d.value, tuple(li)
    return ok, wi, dist, Li


def alpha_decide(mode, cutoff, a, u):
    """ptc_debug_alpha_decide: the host's evaluation of csrc/pt_alpha.h: (accept bool, transmit float32) of one hit of coverage a."""
    acc, tr = C.c_int(0), C.c_float(0)
    rc = load_library().ptc_debug_alpha_decide(_ALPHA_MODES[mode] if isinstance(mode, str) else int(mode), float(cutoff), float(a), float(u), C.byref(acc), C.byref(tr))
    if rc < 0:
        raise PtcError(f"alpha_decide: unknown mode {mode!r}")
    return bool(acc.value), np.float32(tr.value)


def transmission_params(**fields):
    """A ptc_transmission_params: the defaults (transmission 0, ior 1.5, thin-walled, no attenuation) with `fields` replaced."""
    return PtcTransmissionParams.defaults(**fields)


def _material_transmission(m):
    """The ptc_transmission_params of a scene.Material (or anything with its fields)."""
    return transmission_params(transmission=getattr(m, "transmission", 0.0), ior=getattr(m, "ior", 1.5), thin_walled=1 if getattr(m, "thin_walled", True) else 0,
                               attenuation_color=getattr(m, "attenuation_color", (1.0, 1.0, 1.0)), attenuation_distance=getattr(m, "attenuation_distance", 0.0))


def glass_interact(params, **fields):
    """ptc_debug_glass_interact: the host's evaluation of steps 2 to 4 of csrc/pt_glass.h for one hit.  Returns the struct as a dict (outcome, o_out, d_out, T_out, F, ..)."""
    io = PtcGlassInteraction().update(**fields)
    rc = load_library().ptc_debug_glass_interact(C.byref(params), C.byref(io))
    if rc < 0:
        raise PtcError("glass_interact: bad argument")
    return io.as_dict()


def emissive_tex_sample(entry, texture, linear=False, **fields):
    """ptc_debug_emissive_tex_sample: the host's evaluation of csrc/pt_emissive_tex.h for one table entry (28 floats) over one (h, w, 4) uint8 texture.  fields: P, r1,
    r2 of the sample; hit_u, hit_v, bounce, prev_pdf, hit_t, hit_cos of the hit side.  Returns the struct as a dict (ok, y, wi, pl, Le, hit_Le, hit_weight, ..)."""
    e = np.ascontiguousarray(entry, np.float32).reshape(28)
    t = np.ascontiguousarray(texture, np.uint8)
    assert t.ndim == 3 and t.shape[2] == 4, "the texture is (h, w, 4) uint8"
    io = PtcEmissiveTexSample().update(**fields)
    rc = load_library().ptc_debug_emissive_tex_sample(_ptr(e), _ptr(t), t.shape[1], t.shape[0], 1 if linear else 0, C.byref(io))
    if rc < 0:
        raise PtcError("emissive_tex_sample: bad argument")
    return io.as_dict()


def glass_shadow_transmit(params, **fields):
    """ptc_debug_glass_shadow_transmit: the host's evaluation of csrc/pt_glass_shadow.h's pt_glass_shadow_transmit for one hit (ng, ns, d, base, metallic).  Returns
    the struct as a dict (W, F_t, ..)."""
    io = PtcGlassShadowHit().update(**fields)
    rc = load_library().ptc_debug_glass_shadow_transmit(C.byref(params), C.byref(io))
    if rc < 0:
        raise PtcError("glass_shadow_transmit: bad argument")
    return io.as_dict()


def medium_params(box_lo, box_hi, sigma_t, albedo=(1.0, 1.0, 1.0), g=0.0):
    """A ptc_medium_params: the fog box [box_lo, box_hi], its extinction per world unit, single-scattering albedo (a number or rgb) and HG anisotropy."""
    a = (albedo,) * 3 if np.isscalar(albedo) else albedo
    return PtcMediumParams().update(box_lo=box_lo, box_hi=box_hi, sigma_t=sigma_t, albedo=a, g=g)


def medium_sample(params, **fields):
    """ptc_debug_medium_sample: the host's evaluation of csrc/pt_medium.h for one ray (o, d, t_end, u0, u1, u2) and one shadow segment (so, sd, stmax).  Returns
    the struct as a dict (crosses, t0, t1, s, scatters, P, cos_theta, wi, pdf, transmittance, ..)."""
    io = PtcMediumSample().update(**fields)
    rc = load_library().ptc_debug_medium_sample(C.byref(params), C.byref(io))
    if rc < 0:
        raise PtcError("medium_sample: bad argument")
    return io.as_dict()


def display_params(**fields):
    """A ptc_display_params: the defaults with `fields` replaced.  `tonemap` takes a name (aces, neutral, reinhard, clamp) or a TONEMAP_* value, `oetf` a name
    (gamma22, srgb) or an OETF_* value."""
    return PtcDisplayParams.defaults(**fields)


def display_default_params():
    return display_params().as_dict()


def ev_to_gain(ev):
    """The linear exposure multiplier of `ev` stops: 2**ev in float64, rounded to float32."""
    return float(np.float32(2.0 ** float(ev)))


def display_pixels(rgba, E=1.0, **fields):
    """ptc_debug_display_pixel: the host's evaluation of csrc/pt_display.h for the pixels rgba (n, 4) at the exposure scale E with display_params(**fields):
    (RGBA8 (n, 4) uint8, RGBA16F (n, 4) uint16 bit patterns)."""
    L = load_library()
    p = fields.pop("params", None) or display_params(**fields)
    px = np.ascontiguousarray(np.atleast_2d(np.asarray(rgba, np.float32)))
    n = px.shape[0]
    o8, o16 = np.zeros((n, 4), np.uint8), np.zeros((n, 4), np.uint16)
    f, u8, u16 = _POINTERS[px.dtype], _POINTERS[o8.dtype], _POINTERS[o16.dtype]
    base, b8, b16 = px.ctypes.data, o8.ctypes.data, o16.ctypes.data
    fn, pr, e = L.ptc_debug_display_pixel, C.byref(p), C.c_float(float(E))
    for i in range(n):
        if fn(pr, e, C.cast(base + 16 * i, f), C.cast(b8 + 4 * i, u8), C.cast(b16 + 8 * i, u16)) < 0:
            raise PtcError(f"display_pixels: bad display parameters: {p.as_dict()}")
    return o8, o16


def meter(rgba, state=0, **fields):
    """ptc_debug_meter: the host's metering of the pixels rgba (..., 4) from the adaptation state `state` with display_params(**fields): a dict with the new
    state A, Q, N, M, rejected (integers) and hist (4096,) uint32."""
    L = load_library()
    p = fields.pop("params", None) or display_params(**fields)
    px = np.ascontiguousarray(np.asarray(rgba, np.float32).reshape(-1, 4))
    A, Q = C.c_uint32(0), C.c_uint32(0)
    N, M, R = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
    hist = np.zeros(LUMINANCE_BINS, np.uint32)
    rc = L.ptc_debug_meter(C.byref(p), _ptr(px), px.shape[0], int(state), C.byref(A), C.byref(Q), C.byref(N), C.byref(M), C.byref(R), _ptr(hist))
    if rc < 0:
        raise PtcError(f"meter: bad display parameters or too many pixels: {p.as_dict()}")
    return {"A": A.value, "Q": Q.value, "N": N.value, "M": M.value, "rejected": R.value, "hist": hist}


def comm_unique_id() -> bytes:
    """ptc_comm_unique_id: the 128 bytes rank 0 ships to the other ranks before ptc_comm_init."""
    L = load_library()
    buf = (C.c_uint8 * COMM_ID_BYTES)()
    if L.ptc_comm_unique_id(buf) < 0:
        raise PtcError(L.ptc_last_error(None).decode())
    return bytes(buf)


class PathTracer:
    def __init__(self, device: int = 0, _handle=None):
        self._L = load_library()
        self._owned = _handle is None
        self._h = self._L.ptc_create(int(device)) if _handle is None else _handle
        if not self._h:
            raise PtcError(self._L.ptc_last_error(None).decode())
        self.device = int(device)
        self._w = self._h_px = 0

    def close(self):
        if getattr(self, "_h", None):
            if self._owned:
                self._L.ptc_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _ck(self, rc):
        if rc < 0:
            raise PtcError(f"ptc error {rc}: {self._L.ptc_last_error(self._h).decode()}")
        return rc

    def _read(self, fn, shape, dtype, *args, alloc=np.empty):
        """The read-back fn(ctx, *args, out) into a new array; alloc is np.zeros where the library does not write every element."""
        out = alloc(shape, dtype)
        self._ck(fn(self._h, *args, _ptr(out)))
        return out

    def _get(self, fn, struct, *args):
        """fn(ctx, *args, &s) for a new `struct` s, as a dict."""
        s = struct()
        self._ck(fn(self._h, *args, C.byref(s)))
        return s.as_dict()

    # ---- scene ------------------------------------------------------------------------------------
    def load_scene(self, desc):
        """Describe `desc` and commit it (ptc_scene_commit): on the host, or on the device for an LBVH scene — and for a SAH scene when the device builder is
        the SAH (set_device_builder("sah") before this call, or PTC_DEVICE_BVH=sah in the environment)."""
        L, h = self._L, self._h
        self._ck(L.ptc_scene_begin(h))
        for t in getattr(desc, "textures", []):
            t = np.ascontiguousarray(t, np.uint8)
            assert t.ndim == 3 and t.shape[2] == 4, "textures are (h, w, 4) uint8"
            self._ck(L.ptc_add_texture_rgba8(h, _ptr(t), t.shape[1], t.shape[0]))
        self._ck(L.ptc_set_texture_filter(h, 1 if getattr(desc, "texture_filter", "nearest") == "linear" else 0))
        if getattr(desc, "bvh_builder", None) is not None:      # None: the context's default (SAH, or what PTC_BVH says)
            self._ck(L.ptc_set_bvh_builder(h, {"sah": 0, "lbvh": 1}[desc.bvh_builder]))
        env = getattr(desc, "env", None)
        if env is not None:
            e = np.ascontiguousarray(env, np.float32)
            assert e.ndim == 3 and e.shape[2] == 3, "env is (h, w, 3) float32"
            self._ck(L.ptc_set_env_latlong_rgb32f(h, _ptr(e), e.shape[1], e.shape[0]))
        for m in desc.materials:
            mid = self._ck(L.ptc_add_material(h, _f(m.base_color)[1], m.metallic, m.roughness, _f(m.emissive)[1], m.tex_color, m.tex_normal, m.tex_mr))
            if str(getattr(m, "alpha_mode", "opaque")).lower() not in ("opaque", str(ALPHA_OPAQUE)):
                self.set_material_alpha(mid, m.alpha_mode, getattr(m, "alpha_cutoff", 0.5))
            if getattr(m, "transmission", 0.0) > 0.0:
                self.set_material_transmission(mid, _material_transmission(m))
            if getattr(m, "emissive_texture", -1) >= 0:
                self.set_material_emission_texture(mid, m.emissive_texture, getattr(m, "emissive_texture_factor", (1.0, 1.0, 1.0)))
        for me in desc.meshes:
            v = np.ascontiguousarray(me.vertices)
            i = np.ascontiguousarray(me.indices, np.uint32)
            mid = self._ck(L.ptc_add_mesh(h, v.ctypes.data, v.size, _ptr(i), i.size, me.material))
            if getattr(me, "morph_dpos", None) is not None:
                self.mesh_set_morph_targets(mid, me.morph_dpos, getattr(me, "morph_dnormal", None), getattr(me, "morph_dtangent", None))
            if getattr(me, "joints", None) is not None:
                self.mesh_set_skin(mid, me.n_joints, me.joints, me.weights)
            if getattr(me, "morph_weights", None) is not None or getattr(me, "joint_matrices", None) is not None:
                self.update_mesh_pose(mid, getattr(me, "morph_weights", None), getattr(me, "joint_matrices", None))
        for it in desc.instances:
            if getattr(it, "matrix", None) is not None:
                self._ck(L.ptc_add_instance_matrix(h, it.mesh, _f(np.asarray(it.matrix, np.float32).reshape(16))[1]))
            else:
                self._ck(L.ptc_add_instance(h, it.mesh, _f(it.t)[1], _f(it.q_wxyz)[1], _f(it.s)[1]))
        c = desc.camera
        self._ck(L.ptc_set_camera(h, _f(c.position)[1], _f(c.target)[1], c.fov_y, c.aspect))
        if getattr(c, "matrix", None) is not None or getattr(c, "projection", "perspective") != "perspective":      # an extended camera replaces the look-at
            self.set_camera_ex(**_camera_ex_fields(c))
        self.set_camera_lens(getattr(c, "aperture_radius", 0.0), getattr(c, "focus_distance", 1.0), getattr(c, "blades", 0), getattr(c, "aperture_rotation", 0.0))
        for l in getattr(desc, "lights", []):
            self.add_light(l)
        if getattr(desc, "medium", None) is not None:      # a dict of medium_params' arguments
            self.set_medium(**desc.medium)
        self._ck(L.ptc_scene_commit(h))
        return self

    # ---- punctual lights (csrc/pt_lights.h) ---------------------------------------------------------------
    def add_light(self, light=None, **kw):
        """ptc_add_light: a light_params(...) / scene.LightDesc / dict, or the fields as keywords.  Returns the light's id.  Needs no commit; a frame sees the
        lights recorded when it began."""
        return self._ck(self._L.ptc_add_light(self._h, C.byref(light_params_of(light) if light is not None else light_params(**kw))))

    def update_light(self, light_id, light=None, **kw):
        self._ck(self._L.ptc_update_light(self._h, int(light_id), C.byref(light_params_of(light) if light is not None else light_params(**kw))))
        return self

    def get_light(self, light_id):
        return self._get(self._L.ptc_get_light, PtcLightParams, int(light_id))

    def light_count(self):
        return self._ck(self._L.ptc_light_count(self._h))

    def clear_lights(self):
        self._ck(self._L.ptc_clear_lights(self._h))
        return self

    def light_table(self):
        """ptc_debug_get_light_table: (records (n, 16) float32 — word 3 holds the type's int bits —, cdf (n,) float32) as a frame would upload them."""
        n = C.c_uint32()
        self._ck(self._L.ptc_debug_get_light_table(self._h, C.byref(n), None, None))
        rec, cdf = np.zeros((n.value, 16), np.float32), np.zeros(n.value, np.float32)
        if n.value:
            self._ck(self._L.ptc_debug_get_light_table(self._h, None, _ptr(rec), _ptr(cdf)))
        return rec, cdf

    def punctual_nee(self, origins, dirs, keys, bounce=0):
        """ptc_debug_punctual_nee: explicit rays (throughput 1, path id = index, RNG key keys[i]) through k_trace_closest and k_shade_punctual at `bounce`:
        (valid (n,) bool, origin (n, 3), dir (n, 3), tmax (n,), contrib (n, 3)) of the shadow record each ray produced."""
        o, op = _f(origins)
        d, dp = _f(dirs)
        k = np.ascontiguousarray(keys, np.uint32)
        n = o.shape[0]
        assert d.shape[0] == n and k.size == n
        valid = np.zeros(n, np.uint8)
        so, sd, tm, ct = np.zeros((n, 3), np.float32), np.zeros((n, 3), np.float32), np.zeros(n, np.float32), np.zeros((n, 3), np.float32)
        self._ck(self._L.ptc_debug_punctual_nee(self._h, op, dp, _ptr(k), n, int(bounce), _ptr(valid), _ptr(so), _ptr(sd), _ptr(tm), _ptr(ct)))
        return valid.astype(bool), so, sd, tm, ct

    # ---- alpha coverage (csrc/pt_alpha.h) -------------------------------------------------------------------
    def set_material_alpha(self, material, mode, cutoff=0.5):
        """ptc_set_material_alpha, between add_material and the commit: mode "opaque" / "mask" / "blend" (or ALPHA_*), cutoff in [0, 1] (MASK)."""
        self._ck(self._L.ptc_set_material_alpha(self._h, int(material), _ALPHA_MODES[mode.lower()] if isinstance(mode, str) else int(mode), float(cutoff)))
        return self

    def get_material_alpha(self, material):
        """(mode, cutoff) of a material of the description."""
        m, c = C.c_int(0), C.c_float(0)
        self._ck(self._L.ptc_get_material_alpha(self._h, int(material), C.byref(m), C.byref(c)))
        return int(m.value), float(c.value)

    def set_alpha_max_layers(self, n):
        self._ck(self._L.ptc_set_alpha_max_layers(self._h, int(n)))
        return self

    def alpha_stats(self):
        return self._get(self._L.ptc_get_alpha_stats, PtcAlphaStats)

    def alpha_closest(self, origins, dirs, keys, bounce=0, deterministic=False):
        """ptc_debug_alpha_closest: explicit rays through k_trace_closest and the closest-hit alpha resolution: (t, prim, uv, layers)."""
        o, op = _f(origins)
        d, dp = _f(dirs)
        k = np.ascontiguousarray(keys, np.uint32)
        n = o.shape[0]
        assert d.shape[0] == n and k.size == n
        t, prim, uv, layers = np.zeros(n, np.float32), np.zeros(n, np.int32), np.zeros((n, 2), np.float32), np.zeros(n, np.uint32)
        self._ck(self._L.ptc_debug_alpha_closest(self._h, op, dp, _ptr(k), n, int(bounce), 1 if deterministic else 0, _ptr(t), _ptr(prim), _ptr(uv), _ptr(layers)))
        return t, prim, uv, layers

    def alpha_any(self, origins, dirs, tmax):
        """ptc_debug_alpha_any: explicit shadow rays through the shadow resolution: the transmittance per ray (0: occluded)."""
        o, op = _f(origins)
        d, dp = _f(dirs)
        tm, tp = _f(tmax)
        n = o.shape[0]
        assert d.shape[0] == n and tm.size == n
        out = np.zeros(n, np.float32)
        self._ck(self._L.ptc_debug_alpha_any(self._h, op, dp, tp, n, _ptr(out)))
        return out

    def alpha_tables(self):
        """ptc_debug_get_alpha_tables: (bits (ceil(n_prims / 32),) uint32, mode (n_mats,) int32, cutoff (n_mats,) float32, n_prims, whether an alpha queue is allocated)."""
        npr, nm = C.c_uint32(), C.c_uint32()
        self._ck(self._L.ptc_debug_get_alpha_tables(self._h, C.byref(npr), None, C.byref(nm), None))
        bits, mc = np.zeros((npr.value + 31) // 32, np.uint32), np.zeros((nm.value, 2), np.float32)
        rc = self._ck(self._L.ptc_debug_get_alpha_tables(self._h, None, _ptr(bits), None, _ptr(mc)))
        return bits, mc[:, 0].copy().view(np.int32), mc[:, 1].copy(), int(npr.value), bool(rc)

    # ---- dielectric transmission (csrc/pt_glass.h) ----------------------------------------------------------
    def set_material_transmission(self, material, params=None, **fields):
        """ptc_set_material_transmission, between add_material and the commit: a transmission_params(...) or its fields (transmission, ior, thin_walled,
        attenuation_color, attenuation_distance) as keywords."""
        self._ck(self._L.ptc_set_material_transmission(self._h, int(material), C.byref(params if params is not None else transmission_params(**fields))))
        return self

    def get_material_transmission(self, material):
        return self._get(self._L.ptc_get_material_transmission, PtcTransmissionParams, int(material))

    def set_glass_max_interactions(self, n):
        self._ck(self._L.ptc_set_glass_max_interactions(self._h, int(n)))
        return self

    def glass_stats(self):
        return self._get(self._L.ptc_get_glass_stats, PtcGlassStats)

    def glass_closest(self, origins, dirs, keys, bounce=0):
        """ptc_debug_glass_closest: explicit rays of throughput 1 through k_trace_closest, the alpha resolution and the glass resolution:
        (t, prim, uv, o (n, 3), d (n, 3), T (n, 3), pdf word (n,), j)."""
        o, op = _f(origins)
        d, dp = _f(dirs)
        k = np.ascontiguousarray(keys, np.uint32)
        n = o.shape[0]
        assert d.shape[0] == n and k.size == n
        t, prim, uv, ray, j = np.zeros(n, np.float32), np.zeros(n, np.int32), np.zeros((n, 2), np.float32), np.zeros((n, 10), np.float32), np.zeros(n, np.uint32)
        self._ck(self._L.ptc_debug_glass_closest(self._h, op, dp, _ptr(k), n, int(bounce), _ptr(t), _ptr(prim), _ptr(uv), _ptr(ray), _ptr(j)))
        return t, prim, uv, ray[:, 0:3].copy(), ray[:, 3:6].copy(), ray[:, 6:9].copy(), ray[:, 9].copy(), j

    def glass_tables(self):
        """ptc_debug_get_glass_tables: (bits (ceil(n_prims / 32),) uint32, mats (n_mats, 8) float32 — word 2 holds thin's int bits —, n_prims, whether a glass queue is allocated)."""
        npr, nm = C.c_uint32(), C.c_uint32()
        self._ck(self._L.ptc_debug_get_glass_tables(self._h, C.byref(npr), None, C.byref(nm), None))
        bits, mats = np.zeros((npr.value + 31) // 32, np.uint32), np.zeros((nm.value, 8), np.float32)
        rc = self._ck(self._L.ptc_debug_get_glass_tables(self._h, None, _ptr(bits), None, _ptr(mats)))
        return bits, mats, int(npr.value), bool(rc)

    # ---- a homogeneous participating medium (csrc/pt_medium.h) ------------------------------------------------
    def set_medium(self, params=None, **fields):
        """ptc_set_medium: a medium_params(...) or its arguments as keywords (box_lo, box_hi, sigma_t, albedo, g).  Recorded; the next frame uses it."""
        self._ck(self._L.ptc_set_medium(self._h, C.byref(params if params is not None else medium_params(**fields))))
        return self

    def get_medium(self):
        """ptc_get_medium: the parameters as a dict, or None when no medium is set."""
        p = PtcMediumParams()
        return p.as_dict() if self._ck(self._L.ptc_get_medium(self._h, C.byref(p))) else None

    def clear_medium(self):
        self._ck(self._L.ptc_clear_medium(self._h))
        return self

    def medium_stats(self):
        return self._get(self._L.ptc_get_medium_stats, PtcMediumStats)

    def medium_step(self, origins, dirs, throughput, prev_pdf, keys, bounce=0, max_bounces=8):
        """ptc_debug_medium_step: explicit rays (path id = index) through k_trace_closest and the medium pass of one bounce, k_shade between its kernels as in a
        frame.  A dict of arrays per ray: t, word (the hit record as k_shade saw it), uv, alive, o / d / T (n, 3) and pdf of the continuation, shadow, so / sd
        (n, 3), tmax, contrib (n, 3) of the emitter-or-environment shadow record, punctual, po / pd, ptmax, pcontrib of the punctual one; rows without a record
        are zero."""
        o, op = _f(origins)
        d, dp = _f(dirs)
        T, Tp = _f(throughput)
        pp, ppp = _f(prev_pdf)
        k = np.ascontiguousarray(keys, np.uint32)
        n = o.shape[0]
        assert o.shape == d.shape == T.shape == (n, 3) and pp.shape == (n,) and k.shape == (n,)
        hit = np.zeros((n, 4), np.float32)
        alive, sh, pl = np.zeros(n, np.uint8), np.zeros(n, np.uint8), np.zeros(n, np.uint8)
        cont, srec, prec = np.zeros((n, 10), np.float32), np.zeros((n, 10), np.float32), np.zeros((n, 10), np.float32)
        self._ck(self._L.ptc_debug_medium_step(self._h, op, dp, Tp, ppp, _ptr(k), n, int(bounce), int(max_bounces), _ptr(hit), _ptr(alive), _ptr(cont), _ptr(sh),
                                               _ptr(srec), _ptr(pl), _ptr(prec)))
        return dict(t=hit[:, 0].copy(), word=hit[:, 1].copy().view(np.int32), uv=hit[:, 2:4].copy(), alive=alive.astype(bool), o=cont[:, 0:3].copy(),
                    d=cont[:, 3:6].copy(), T=cont[:, 6:9].copy(), pdf=cont[:, 9].copy(), shadow=sh.astype(bool), so=srec[:, 0:3].copy(), sd=srec[:, 3:6].copy(),
                    tmax=srec[:, 6].copy(), contrib=srec[:, 7:10].copy(), punctual=pl.astype(bool), po=prec[:, 0:3].copy(), pd=prec[:, 3:6].copy(),
                    ptmax=prec[:, 6].copy(), pcontrib=prec[:, 7:10].copy())

    def medium_env(self, r1, r2, dir_in):
        """ptc_debug_medium_env: the medium pass's environment sampler and lookup on their own: (direction sampled from (r1, r2) (n, 3), Le (n, 3) and pdf (n,) of dir_in)."""
        a, ap = _f(r1)
        b, bp = _f(r2)
        d, dp = _f(dir_in)
        n = a.shape[0]
        assert a.shape == b.shape == (n,) and d.shape == (n, 3)
        wi, Le, pdf = np.zeros((n, 3), np.float32), np.zeros((n, 3), np.float32), np.zeros(n, np.float32)
        self._ck(self._L.ptc_debug_medium_env(self._h, ap, bp, dp, n, _ptr(wi), _ptr(Le), _ptr(pdf)))
        return wi, Le, pdf

    # ---- textured emission (csrc/pt_emissive_tex.h) -----------------------------------------------------------
    def set_material_emission_texture(self, material, texture, factor=(1.0, 1.0, 1.0)):
        """ptc_set_material_emission_texture, between add_material and the commit: the surfaces of `material` emit factor x texel of `texture` (texture -1 removes it)."""
        self._ck(self._L.ptc_set_material_emission_texture(self._h, int(material), int(texture), _f(np.asarray(factor, np.float32).reshape(3))[1]))
        return self

    def get_material_emission_texture(self, material):
        """(texture id or -1, factor (3,) float32)."""
        tex, f = C.c_int(-1), np.zeros(3, np.float32)
        self._ck(self._L.ptc_get_material_emission_texture(self._h, int(material), C.byref(tex), _ptr(f)))
        return int(tex.value), f

    def emissive_tex_stats(self):
        return self._get(self._L.ptc_get_emissive_tex_stats, PtcEmissiveTexStats)

    def emissive_tex_table(self):
        """ptc_debug_get_emissive_tex_table: (records (n, 28) float32 — word 11 holds the texture id's int bits —, cdf (n,), prim_map (n_prims,) int32, total)."""
        n, npr, total = C.c_uint32(0), C.c_uint32(0), C.c_float(0)
        self._ck(self._L.ptc_debug_get_emissive_tex_table(self._h, C.byref(n), None, None, C.byref(npr), None, C.byref(total)))
        recs, cdf, pm = np.zeros((n.value, 28), np.float32), np.zeros(n.value, np.float32), np.zeros(npr.value, np.int32)
        self._ck(self._L.ptc_debug_get_emissive_tex_table(self._h, None, _ptr(recs), _ptr(cdf), None, _ptr(pm), None))
        return recs, cdf, pm, float(total.value)

    def emissive_tex_step(self, origins, dirs, throughput, prev_pdf, keys, bounce, max_bounces, lpath=None):
        """ptc_debug_emissive_tex_step: explicit rays through k_trace_closest and one launch of k_shade_emissive_tex: (lpath (n, 3) — the paths' radiance `lpath`, zero
        by default, with what the hit side added —, shadow valid (n,) bool, shadow records (n, 10): origin, direction, tmax, contribution), by path id."""
        (o, op), (d, dp), (t, tp), (pp, ppp) = _f(origins), _f(dirs), _f(throughput), _f(prev_pdf)
        k = np.ascontiguousarray(keys, np.uint32)
        n = k.size
        assert o.size == n * 3 and d.size == n * 3 and t.size == n * 3 and pp.size == n
        lp = np.zeros((n, 3), np.float32) if lpath is None else np.array(lpath, np.float32, order="C").reshape(n, 3)
        valid, sh = np.zeros(n, np.uint8), np.zeros((n, 10), np.float32)
        self._ck(self._L.ptc_debug_emissive_tex_step(self._h, op, dp, tp, ppp, _ptr(k), n, int(bounce), int(max_bounces), _ptr(lp), _ptr(valid), _ptr(sh)))
        return lp, valid.astype(bool), sh

    # ---- transparent shadows through thin glass (csrc/pt_glass_shadow.h) --------------------------------------
    def set_glass_shadows(self, on=True):
        """ptc_set_glass_shadows: shadow rays pass thin-walled panes with their expected transmittance (off by default; the next frame uses it)."""
        self._ck(self._L.ptc_set_glass_shadows(self._h, 1 if on else 0))
        return self

    def get_glass_shadows(self):
        on = C.c_int(0)
        self._ck(self._L.ptc_get_glass_shadows(self._h, C.byref(on)))
        return bool(on.value)

    def glass_shadow_stats(self):
        return self._get(self._L.ptc_get_glass_shadow_stats, PtcGlassShadowStats)

    def glass_any(self, origins, dirs, tmax):
        """ptc_debug_glass_any: explicit shadow rays through the shadow resolution: (the RGB transmittance per ray (n, 3) — 0: occluded —, the surfaces passed (n,))."""
        o, op = _f(origins)
        d, dp = _f(dirs)
        tm, tp = _f(tmax)
        n = o.shape[0]
        assert d.shape[0] == n and tm.size == n
        out, layers = np.zeros((n, 3), np.float32), np.zeros(n, np.uint32)
        self._ck(self._L.ptc_debug_glass_any(self._h, op, dp, tp, n, _ptr(out), _ptr(layers)))
        return out, layers

    def set_camera(self, position, target, fov_y, aspect):
        self._ck(self._L.ptc_set_camera(self._h, _f(position)[1], _f(target)[1], fov_y, aspect))

    def set_camera_lens(self, aperture_radius=0.0, focus_distance=1.0, blades=0, rotation=0.0):
        """ptc_set_camera_lens: the thin lens of the path integrator's camera.  aperture_radius 0 is the pinhole; blades 0 a disk, 3..16 a regular polygon with
        a vertex at `rotation` turns; focus_distance the view depth of the plane of focus.  Kept across set_camera, reset by load_scene (which applies the
        scene camera's lens fields)."""
        p = PtcLensParams(aperture_radius, focus_distance, int(blades), rotation)
        self._ck(self._L.ptc_set_camera_lens(self._h, C.byref(p)))
        return self

    def get_camera_lens(self):
        return self._get(self._L.ptc_get_camera_lens, PtcLensParams)

    # ---- camera models (csrc/pt_camera.h, include/ptc_camera.h) ------------------------------------------------
    def set_camera_ex(self, matrix=None, projection="perspective", **fields):
        """ptc_set_camera_ex: the camera given by its camera-to-world `matrix` (4x4, glTF camera space: looks along -Z, +Y up, +X right; None is the
        identity) and a projection: "perspective" (yfov radians, aspect), "orthographic" (xmag, ymag: half extents) or "equirect" (the 360-degree panorama,
        no parameters).  Fields left out keep the library's defaults.  Replaces set_camera's camera, and is replaced by it."""
        p = PtcCameraParams.defaults(projection=projection, **fields)
        if matrix is not None:
            m = np.asarray(matrix, np.float32)
            if m.shape not in ((4, 4), (16,)):
                raise PtcError(f"set_camera_ex: the matrix must be 4x4 (or its 16 entries in column-major order), got {m.shape}")
            p.update(camera_to_world=(m.T if m.ndim == 2 else m).reshape(16))      # a 4x4 array is the mathematical matrix: its columns go out one after the other
        self._ck(self._L.ptc_set_camera_ex(self._h, C.byref(p)))
        return self

    def debug_guide_positions(self):
        """ptc_debug_read_guide_positions: (h, w, 4) = (P, class) of the current frame's guides, P = origin + Z direction of the pixel-centre ray."""
        return self._read(self._L.ptc_debug_read_guide_positions, (self._h_px, self._w, 4), np.float32)

    def get_camera_ex(self):
        """ptc_get_camera_ex: the extended camera as a dict (camera_to_world: the 16 column-major entries; projection: its name), or None when set_camera's
        camera is in force."""
        p = PtcCameraParams()
        if not self._ck(self._L.ptc_get_camera_ex(self._h, C.byref(p))):
            return None
        d = p.as_dict()
        d["projection"] = {v: k for k, v in _PROJECTIONS.items()}[d["projection"]]
        return d

    def focus_distance_at_pixel(self, x, y):
        """ptc_focus_distance_at_pixel: the view depth of what pixel (x, y)'s centre sees (0 on a miss), from the current frame's guides (frame_guides())."""
        out = C.c_float(0)
        self._ck(self._L.ptc_focus_distance_at_pixel(self._h, int(x), int(y), C.byref(out)))
        return float(out.value)

    def update_instance(self, instance, t=None, q_wxyz=None, s=None, matrix=None):
        """New transform for a committed instance (ptc_update_instance / ptc_update_instance_matrix); scene_refit() applies it."""
        if matrix is not None:
            self._ck(self._L.ptc_update_instance_matrix(self._h, instance, _f(np.asarray(matrix, np.float32).reshape(16))[1]))
        else:
            self._ck(self._L.ptc_update_instance(self._h, instance, _f(t)[1], _f(q_wxyz)[1], _f(s)[1]))
        return self

    def scene_refit(self):
        self._ck(self._L.ptc_scene_refit(self._h))
        return self

    # ---- deforming meshes ----------------------------------------------------------------
    def mesh_set_morph_targets(self, mesh, dpos, dnormal=None, dtangent=None):
        """ptc_mesh_set_morph_targets, before the commit: dpos (and dnormal, dtangent, which may be None) are (n_targets, n_verts, 3) float32."""
        dp = np.ascontiguousarray(dpos, np.float32)
        assert dp.ndim == 3 and dp.shape[2] == 3, "morph deltas are (n_targets, n_verts, 3)"
        ptrs = [_ptr(dp)]
        for a in (dnormal, dtangent):
            if a is None:
                ptrs.append(None)
                continue
            a = np.ascontiguousarray(a, np.float32)
            assert a.shape == dp.shape, "every delta array has the shape of dpos"
            ptrs.append(_ptr(a))
        self._ck(self._L.ptc_mesh_set_morph_targets(self._h, int(mesh), dp.shape[0], *ptrs))
        return self

    def mesh_set_skin(self, mesh, n_joints, joints, weights):
        """ptc_mesh_set_skin, before the commit: joints (n_verts, 4) uint16, weights (n_verts, 4) float32."""
        j = np.ascontiguousarray(joints, np.uint16)
        w = np.ascontiguousarray(weights, np.float32)
        assert j.ndim == 2 and j.shape[1] == 4 and w.shape == j.shape, "joints and weights are (n_verts, 4)"
        self._ck(self._L.ptc_mesh_set_skin(self._h, int(mesh), int(n_joints), _ptr(j), _ptr(w)))
        return self

    def update_mesh_pose(self, mesh, morph_weights=None, joint_matrices=None):
        """ptc_update_mesh_pose: morph_weights (n_targets,) and / or joint_matrices (n_joints, 12) — rows 0..2 of a column-major 4x4, column by column; None
        leaves that half of the pose as it is.  scene_refit() / scene_rebuild() / a commit apply it."""
        wp = jp = None
        nw = nj = 0
        if morph_weights is not None:
            w = np.ascontiguousarray(morph_weights, np.float32).reshape(-1)
            wp, nw = _ptr(w), w.size
        if joint_matrices is not None:
            jm = np.ascontiguousarray(joint_matrices, np.float32)
            assert jm.size % 12 == 0, "joint matrices are 12 floats each"
            jp, nj = _ptr(jm), jm.size // 12
        self._ck(self._L.ptc_update_mesh_pose(self._h, int(mesh), wp, nw, jp, nj))
        return self

    def update_mesh_vertices(self, mesh, vertices):
        """ptc_update_mesh_vertices: new BASE vertices (MESH_VERTEX, the mesh's count) for a caller who deforms on their own."""
        v = np.ascontiguousarray(vertices)
        assert v.dtype.itemsize == 48, "vertices are MESH_VERTEX records"
        self._ck(self._L.ptc_update_mesh_vertices(self._h, int(mesh), v.ctypes.data, v.size))
        return self

    def mesh_vertices(self, mesh, n_verts):
        """ptc_debug_get_mesh_vertices: the current posed object-space vertices of a mesh as (n_verts, 12) float32."""
        return self._read(self._L.ptc_debug_get_mesh_vertices, (int(n_verts), 12), np.float32, int(mesh), alloc=np.zeros)

    def host_build_id(self):
        return int(self._L.ptc_debug_host_build_id(self._h))

    def launch_policy(self):
        """ptc_launch_policy of this context (after a commit: with the launch configuration that followed)."""
        return self._L.ptc_launch_policy(self._h).decode()

    def set_device_builder(self, builder):
        """ptc_set_device_builder: the tree a build on the device makes, "lbvh" (the default) or "sah" (the host's binned-SAH tree, byte for byte); kept across
        load_scene.  With "sah" a SAH scene commits on the device and scene_rebuild makes the SAH tree."""
        self._ck(self._L.ptc_set_device_builder(self._h, {"sah": 0, "lbvh": 1}[builder]))
        return self

    def scene_rebuild(self):
        """ptc_scene_rebuild: pending transforms + a new tree for the moved geometry, built on the device: the device builder's (set_device_builder), the LBVH by default."""
        self._ck(self._L.ptc_scene_rebuild(self._h))
        return self

    # ---- rendering --------------------------------------------------------------------------------
    def render(self, w, h, spp, seed=1, max_bounces=8, integrator=INTEGRATOR_PATH):
        self._ck(self._L.ptc_render(self._h, w, h, spp, seed, max_bounces, integrator))
        self._w, self._h_px = w, h
        return self.read_radiance()

    def frame_begin(self, w, h, spp_total, seed=1, max_bounces=8, integrator=INTEGRATOR_PATH, tile_rank=0, tile_count=1):
        self._ck(self._L.ptc_frame_begin(self._h, w, h, spp_total, seed, max_bounces, integrator, tile_rank, tile_count))
        self._w, self._h_px = w, h

    # ---- light probes (csrc/pt_probes.h) ----------------------------------------------------------------
    @staticmethod
    def _probe_positions(positions):
        p = np.ascontiguousarray(positions, np.float32)
        if p.ndim != 2 or p.shape[1] != 3:
            raise PtcError(f"probe positions must be (n, 3), got {p.shape}")
        return p

    def probes_begin(self, positions, spp_total, seed=0, max_bounces=8, index_base=0):
        """ptc_probes_begin: a probe frame of len(positions) probes; frame_add_samples / frame_set_sample_range / sync work as in any frame, and after
        frame_resolve read_radiance returns the (1, n, 4) image of each probe's mean incoming radiance."""
        p = self._probe_positions(positions)
        self._ck(self._L.ptc_probes_begin(self._h, _ptr(p), p.shape[0], index_base, spp_total, seed, max_bounces))
        self._w, self._h_px = p.shape[0], 1
        self._n_probes = p.shape[0]

    def read_probes_sh(self):
        """ptc_probes_read_sh: the SH9 coefficients of the probe frame in progress, (n, 9, 3) float32 laid out [probe][k][rgb]."""
        return self._read(self._L.ptc_probes_read_sh, (getattr(self, "_n_probes", 0) or 1, 9, 3), np.float32, alloc=np.zeros)

    def render_probes(self, positions, spp, seed=0, max_bounces=8, index_base=0):
        """Bake the probes at `positions` (n, 3) with spp samples each: (n, 9, 3) float32 SH9 coefficients of the incoming radiance (sh9_irradiance turns them
        into the irradiance for a normal).  ptc_render_probes when index_base is 0; index_base shards a probe set: the probes [a, b) with index_base = a are
        bit for bit those of the whole set."""
        p = self._probe_positions(positions)
        if index_base == 0:
            out = self._read(self._L.ptc_render_probes, (p.shape[0], 9, 3), np.float32, _ptr(p), p.shape[0], spp, seed, max_bounces, alloc=np.zeros)
            self._w, self._h_px, self._n_probes = p.shape[0], 1, p.shape[0]
            return out
        self.probes_begin(p, spp, seed, max_bounces, index_base)
        self.frame_add_samples(spp)
        return self.read_probes_sh()

    # ---- lightmaps (csrc/pt_lightmap.h, include/ptc_lightmap.h) -------------------------------------------------------------
    def _lightmap_desc(self, instance, width, height, spp_total, uv, seed, max_bounces, index_base):
        """(ptc_lightmap_desc, the array its uv points into): uv is (n_verts, 2) float32 or None = the mesh's texcoord."""
        d = PtcLightmapDesc()
        d.instance, d.width, d.height, d.texel_index_base, d.spp_total, d.seed, d.max_bounces = int(instance), int(width), int(height), int(index_base), int(spp_total), int(seed), int(max_bounces)
        keep = None
        if uv is not None:
            keep = np.ascontiguousarray(uv, np.float32)
            if keep.ndim != 2 or keep.shape[1] != 2:
                raise PtcError(f"lightmap uv must be (n_verts, 2), got {keep.shape}")
            d.uv = _ptr(keep)
        return d, keep

    def lightmap_begin(self, instance, width, height, spp_total, uv=None, seed=0, max_bounces=8, index_base=0):
        """ptc_lightmap_begin: a lightmap frame over the covered texels of `instance`'s width x height atlas; frame_add_samples / frame_set_sample_range / sync work
        as in any frame, and read_lightmap resolves what has been accumulated."""
        d, keep = self._lightmap_desc(instance, width, height, spp_total, uv, seed, max_bounces, index_base)
        self._ck(self._L.ptc_lightmap_begin(self._h, C.byref(d)))
        n = C.c_uint32(0)
        self._ck(self._L.ptc_lightmap_texel_count(self._h, C.byref(n), None))
        self._w, self._h_px = int(n.value), 1
        self._lm_size = (int(height), int(width))

    def lightmap_texel_count(self):
        """ptc_lightmap_texel_count: (entries of the lightmap frame in progress, owned texels dropped for a degenerate world triangle)."""
        n, dr = C.c_uint32(0), C.c_uint32(0)
        self._ck(self._L.ptc_lightmap_texel_count(self._h, C.byref(n), C.byref(dr)))
        return int(n.value), int(dr.value)

    def lightmap_texels(self):
        """ptc_lightmap_read_texels: dict(atlas_index (n,) uint32, prim (n,) uint32, origin (n, 3) float32, normal (n, 3) float32) of the frame in progress."""
        n, _ = self.lightmap_texel_count()
        a, pr, o, nr = np.zeros(n, np.uint32), np.zeros(n, np.uint32), np.zeros((n, 3), np.float32), np.zeros((n, 3), np.float32)
        self._ck(self._L.ptc_lightmap_read_texels(self._h, _ptr(a), _ptr(pr), _ptr(o), _ptr(nr)))
        return dict(atlas_index=a, prim=pr, origin=o, normal=nr)

    def read_lightmap(self, dilate=2, backface_threshold=0.1, with_backface=False):
        """ptc_lightmap_read: the atlas (H, W, 4) float32 — RGB irradiance, alpha 1 baked / 0.5 filled by dilation / 0 empty; with_backface: and the back-face
        fraction per entry, (n,) float32."""
        h, w = getattr(self, "_lm_size", (1, 1))
        out = np.zeros((h, w, 4), np.float32)
        frac = np.zeros(max(self.lightmap_texel_count()[0], 1) if with_backface else 0, np.float32)
        self._ck(self._L.ptc_lightmap_read(self._h, int(dilate), float(backface_threshold), _ptr(out), _ptr(frac) if with_backface else None))
        return (out, frac[:self.lightmap_texel_count()[0]]) if with_backface else out

    def render_lightmap(self, instance, width, height, spp, uv=None, seed=0, max_bounces=8, index_base=0, dilate=2, backface_threshold=0.1):
        """ptc_render_lightmap: bake `instance` into a width x height atlas with spp samples per covered texel: (H, W, 4) float32 as read_lightmap returns it."""
        d, keep = self._lightmap_desc(instance, width, height, spp, uv, seed, max_bounces, index_base)
        out = np.zeros((int(height), int(width), 4), np.float32)
        self._ck(self._L.ptc_render_lightmap(self._h, C.byref(d), int(dilate), float(backface_threshold), _ptr(out)))
        n = C.c_uint32(0)
        self._ck(self._L.ptc_lightmap_texel_count(self._h, C.byref(n), None))
        self._w, self._h_px, self._lm_size = int(n.value), 1, (int(height), int(width))
        return out

    def debug_lightmap_cover(self, indices, uv, width, height):
        """ptc_debug_lightmap_cover: the owner image (H, W) uint32 of the triangles `indices` (n, 3) with the UVs `uv` (n_verts, 2); 0xffffffff: nobody."""
        idx = np.ascontiguousarray(indices, np.uint32).reshape(-1, 3)
        t = np.ascontiguousarray(uv, np.float32).reshape(-1, 2)
        out = np.zeros((int(height), int(width)), np.uint32)
        self._ck(self._L.ptc_debug_lightmap_cover(self._h, _ptr(idx), idx.shape[0], _ptr(t), t.shape[0], int(width), int(height), _ptr(out)))
        return out

    def debug_lightmap_rays(self, instance, width, height, seed, first_sample, n_samples, uv=None, index_base=0, rays=True):
        """ptc_debug_lightmap_rays: dict(covered, dropped, atlas_index, prim, origin, normal) of the texel list, and with rays=True ray_o, ray_d (n_samples * n, 3)
        float32 and key (n_samples * n,) uint32 in path order p = sample_local * n + entry."""
        d, keep = self._lightmap_desc(instance, width, height, 1, uv, seed, 0, index_base)
        cap = int(width) * int(height)
        counts = np.zeros(2, np.uint32)
        a, pr, o, nr = np.zeros(cap, np.uint32), np.zeros(cap, np.uint32), np.zeros((cap, 3), np.float32), np.zeros((cap, 3), np.float32)
        od, key = (np.zeros((cap * int(n_samples), 6), np.float32), np.zeros(cap * int(n_samples), np.uint32)) if rays else (None, None)
        self._ck(self._L.ptc_debug_lightmap_rays(self._h, C.byref(d), int(first_sample), int(n_samples), _ptr(counts), _ptr(a), _ptr(pr), _ptr(o), _ptr(nr),
                                                 _ptr(od) if rays else None, _ptr(key) if rays else None))
        n = int(counts[0])
        out = dict(covered=n, dropped=int(counts[1]), atlas_index=a[:n].copy(), prim=pr[:n].copy(), origin=o[:n].copy(), normal=nr[:n].copy())
        if rays:
            m = n * int(n_samples)
            out.update(ray_o=od[:m, :3].copy(), ray_d=od[:m, 3:].copy(), key=key[:m].copy())
        return out

    def debug_lightmap_dilate(self, rgba, iters):
        """ptc_debug_lightmap_dilate: `iters` dilation iterations over the (H, W, 4) image; a new array."""
        img = np.array(rgba, np.float32, order="C")
        if img.ndim != 3 or img.shape[2] != 4:
            raise PtcError(f"the image must be (H, W, 4), got {img.shape}")
        self._ck(self._L.ptc_debug_lightmap_dilate(self._h, img.shape[1], img.shape[0], int(iters), _ptr(img)))
        return img

    def debug_probe_rays(self, positions, seed, first_sample, n_samples, index_base=0):
        """ptc_debug_probe_rays: (origins, dirs, keys) of the probe rays in path order p = sample_local * n + j: (n_samples * n, 3) float32 twice and uint32."""
        p = self._probe_positions(positions)
        n = p.shape[0] * int(n_samples)
        od, key = np.zeros((n, 6), np.float32), np.zeros(n, np.uint32)
        self._ck(self._L.ptc_debug_probe_rays(self._h, _ptr(p), p.shape[0], index_base, seed, first_sample, n_samples, _ptr(od), _ptr(key)))
        return od[:, :3].copy(), od[:, 3:].copy(), key

    def debug_probe_project(self, n_probes, seed, first_sample, n_samples, lpath, acc=None, index_base=0):
        """ptc_debug_probe_project: the running sums (n, 9, 3) after adding the projection of lpath (n_samples * n, 4) to acc (zeros when None)."""
        L = np.ascontiguousarray(lpath, np.float32).reshape(-1, 4)
        if L.shape[0] != int(n_probes) * int(n_samples):
            raise PtcError(f"debug_probe_project: lpath has {L.shape[0]} paths, expected {int(n_probes) * int(n_samples)}")
        a = np.zeros((n_probes, 9, 3), np.float32) if acc is None else np.array(acc, np.float32).reshape(n_probes, 9, 3)
        a = np.ascontiguousarray(a)
        self._ck(self._L.ptc_debug_probe_project(self._h, n_probes, index_base, seed, first_sample, n_samples, _ptr(L), _ptr(a)))
        return a

    def frame_checkpoint(self):
        """(per-pixel sums as an opaque (n_owned, 4) float32 array, samples in them) of the frame in progress (ptc_frame_checkpoint)."""
        n, k = C.c_uint64(0), C.c_uint32(0)
        self._ck(self._L.ptc_frame_checkpoint(self._h, None, C.byref(n), C.byref(k)))
        acc = np.zeros((n.value, 4), np.float32)
        self._ck(self._L.ptc_frame_checkpoint(self._h, _ptr(acc), C.byref(n), C.byref(k)))
        return acc, int(k.value)

    def frame_restore(self, accum, samples_done):
        a = np.ascontiguousarray(accum, np.float32)
        self._ck(self._L.ptc_frame_restore(self._h, _ptr(a), a.shape[0], samples_done))

    def frame_set_sample_range(self, first_sample, resolve_divisor=0):
        self._ck(self._L.ptc_frame_set_sample_range(self._h, first_sample, resolve_divisor))

    def frame_add_samples(self, n):
        self._ck(self._L.ptc_frame_add_samples(self._h, n))

    def frame_reserve(self):
        """Allocate the frame's queues for full batches now (offline renders; see ptc_frame_reserve)."""
        self._ck(self._L.ptc_frame_reserve(self._h))

    def frame_resolve(self):
        self._ck(self._L.ptc_frame_resolve(self._h))

    def sync(self):
        self._ck(self._L.ptc_sync(self._h))

    def read_radiance(self):
        return self._read(self._L.ptc_read_radiance_rgba32f, (self._h_px, self._w, 4), np.float32)

    def write_radiance(self, img):
        a, p = _f(img)
        assert a.size == self._w * self._h_px * 4
        self._ck(self._L.ptc_write_radiance_rgba32f(self._h, p))

    def radiance_device_ptr(self) -> int:
        return int(self._L.ptc_radiance_device_ptr(self._h) or 0)

    def read_radiance_f16(self):
        """The radiance buffer as the reference's RGBA16F HdrImage holds it: (h, w, 4) float16."""
        return self._read(self._L.ptc_read_radiance_rgba16f, (self._h_px, self._w, 4), np.uint16).view(np.float16)

    def radiance_f16_device_ptr(self) -> int:
        return int(self._L.ptc_radiance_rgba16f_device_ptr(self._h) or 0)

    # ---- guide buffers, denoiser, output selection ---------------------------------------------------
    def frame_guides(self):
        """ptc_frame_guides: trace the first-hit guides (albedo, normal, depth, class, hit) of every pixel of the frame in progress."""
        self._ck(self._L.ptc_frame_guides(self._h))

    def read_guide(self, which):
        """(h, w, 4) float32: GUIDE_ALBEDO = (albedo rgb, class), GUIDE_NORMAL_DEPTH = (normal, depth)."""
        return self._read(self._L.ptc_read_guide_rgba32f, (self._h_px, self._w, 4), np.float32, int(which))

    def read_guide_hit(self):
        """(prim (h, w) int32 with -1 = miss, uv (h, w, 2) float32) of the guide rays' hits."""
        prim = np.empty((self._h_px, self._w), np.int32)
        uv = np.empty((self._h_px, self._w, 2), np.float32)
        self._ck(self._L.ptc_read_guide_hit(self._h, _ptr(prim), _ptr(uv)))
        return prim, uv

    @staticmethod
    def denoise_default_params():
        return PtcDenoiseParams.defaults().as_dict()

    def denoise(self, **params):
        """ptc_denoise: radiance buffer + guides -> the denoised buffer.  Keywords (iterations, sigma_l, sigma_n, sigma_p, demodulate) replace the defaults."""
        self._ck(self._L.ptc_denoise(self._h, C.byref(PtcDenoiseParams.defaults(**params))))

    def select_output(self, which):
        """ptc_select_output: OUTPUT_RADIANCE or OUTPUT_DENOISED is what read_radiance / read_radiance_f16 / tonemap serve."""
        self._ck(self._L.ptc_select_output(self._h, int(which)))

    def denoise_seconds(self):
        """(guide pass, denoise): HIP-event seconds of the last frame_guides() and the last denoise()."""
        g, d = C.c_double(0), C.c_double(0)
        self._ck(self._L.ptc_get_denoise_seconds(self._h, C.byref(g), C.byref(d)))
        return g.value, d.value

    # ---- temporal accumulation ----------------------------------------------------------------------------
    @staticmethod
    def temporal_default_params():
        return PtcTemporalParams.defaults().as_dict()

    def temporal_accumulate(self, **params):
        """ptc_temporal_accumulate: reproject the history through the frame's guides and blend the radiance buffer in; the accumulated image is
        OUTPUT_ACCUMULATED.  Keywords (max_history, sigma_z, demodulate) replace the defaults."""
        self._ck(self._L.ptc_temporal_accumulate(self._h, C.byref(PtcTemporalParams.defaults(**params))))

    def temporal_reset(self):
        """ptc_temporal_reset: drop the history; the next temporal_accumulate() starts from nothing."""
        self._ck(self._L.ptc_temporal_reset(self._h))

    def read_temporal(self, which):
        """(h, w, 4) float32 of the last temporal_accumulate(): TEMPORAL_HISTORY (D rgb, n), TEMPORAL_MOMENTS (m1, m2, Var_t, a), TEMPORAL_MOTION
        (x_prev, y_prev, W, reprojected n), and the history's copies of its frame's guides, TEMPORAL_NORMAL_DEPTH (N, Z) and TEMPORAL_POSITION_CLASS (P, K).
        (h, w) is the current frame's, which the library holds the history's size to: after a frame_begin with another size it raises (ptc error -2) until
        the next temporal_accumulate()."""
        return self._read(self._L.ptc_read_temporal_rgba32f, (self._h_px, self._w, 4), np.float32, int(which))

    def denoise_accumulated(self, **params):
        """ptc_denoise_accumulated: the denoiser's iterations over the accumulated image, with the temporal variance where the history is long enough."""
        self._ck(self._L.ptc_denoise_accumulated(self._h, C.byref(PtcDenoiseParams.defaults(**params))))

    def temporal_seconds(self):
        """HIP-event seconds of the last temporal_accumulate()."""
        t = C.c_double(0)
        self._ck(self._L.ptc_get_temporal_seconds(self._h, C.byref(t)))
        return t.value

    # ---- adaptive sampling ------------------------------------------------------------------------------
    @staticmethod
    def adaptive_default_params():
        return PtcAdaptiveParams.defaults().as_dict()

    def frame_set_adaptive(self, **params):
        """ptc_frame_set_adaptive, right after frame_begin: add_samples then feeds the active pixels only.  Keywords (threshold, radius, min_samples,
        step_samples) replace the defaults."""
        self._ck(self._L.ptc_frame_set_adaptive(self._h, C.byref(PtcAdaptiveParams.defaults(**params))))

    def frame_adapt(self):
        """ptc_frame_adapt: one decision step; returns the number of pixels still active."""
        n = C.c_uint64(0)
        self._ck(self._L.ptc_frame_adapt(self._h, C.byref(n)))
        return int(n.value)

    def read_sample_counts(self):
        """(h, w) uint32: samples every pixel of the adaptive frame has received, 0 where this context does not own the pixel."""
        return self._read(self._L.ptc_read_sample_counts, (self._h_px, self._w), np.uint32, alloc=np.zeros)

    def render_adaptive(self, w, h, max_spp, seed=1, max_bounces=8, **params):
        """ptc_render_adaptive: at most max_spp samples per pixel, fewer where the estimate has converged; returns the image (read_sample_counts has the counts)."""
        self._ck(self._L.ptc_render_adaptive(self._h, w, h, max_spp, seed, max_bounces, C.byref(PtcAdaptiveParams.defaults(**params))))
        self._w, self._h_px = w, h
        return self.read_radiance()

    def adaptive_stats(self):
        return self._get(self._L.ptc_get_adaptive_stats, PtcAdaptiveStats)

    # ---- denoising from per-sample statistics ----------------------------------------------
    def set_sample_covariance(self, on):
        """ptc_set_sample_covariance: every adaptive frame begun (frame_set_adaptive, render_adaptive) while it is on keeps the per-pixel RGB covariance sums."""
        self._ck(self._L.ptc_set_sample_covariance(self._h, int(on)))
        return self

    def read_sample_covariance(self):
        """(h, w, 6) float32: the raw sums (rr, gg, bb, rg, rb, gb) of the current frame's samples, 0 where this context does not own the pixel."""
        return self._read(self._L.ptc_read_sample_covariance, (self._h_px, self._w, 6), np.float32, alloc=np.zeros)

    def denoise_sampled(self, **params):
        """ptc_denoise_sampled: the denoiser's iterations over the resolved radiance with the variance of the frame's own samples where a pixel has four or
        more (after frame_resolve and frame_guides).  Keywords as denoise()."""
        self._ck(self._L.ptc_denoise_sampled(self._h, C.byref(PtcDenoiseParams.defaults(**params))))

    def read_sampled_variance(self):
        """(h, w, 2) float32: (Var_s, 1 / n) as the frame's last denoise_sampled() computed them, (0, 0) where the count is 0."""
        return self._read(self._L.ptc_read_sampled_variance, (self._h_px, self._w, 2), np.float32, alloc=np.zeros)

    # ---- multi-GPU (RCCL through the C-ABI) ---------------------------------------------------------
    def comm_init(self, unique_id: bytes, rank: int, n_ranks: int):
        buf = (C.c_uint8 * COMM_ID_BYTES).from_buffer_copy(unique_id)
        self._ck(self._L.ptc_comm_init(self._h, buf, rank, n_ranks))

    def comm_reduce_radiance(self, root: int = 0):
        self._ck(self._L.ptc_comm_reduce_radiance(self._h, root))

    def comm_destroy(self):
        self._ck(self._L.ptc_comm_destroy(self._h))

    def tonemap(self):
        return self._read(self._L.ptc_tonemap_rgba8, (self._h_px, self._w, 4), np.uint8)

    # ---- display transform (csrc/pt_display.h) -----------------------------------------------
    def set_display(self, **fields):
        """ptc_set_display: the current display parameters with `fields` replaced (gain, auto_exposure, key, percentile_lo, percentile_hi, adapt_rate,
        min_luminance, max_luminance, tonemap, white, oetf); no field: the defaults.  A context setting, kept across load_scene."""
        if fields:
            p = PtcDisplayParams()
            self._ck(self._L.ptc_get_display(self._h, C.byref(p)))
            self._ck(self._L.ptc_set_display(self._h, C.byref(p.update(**fields))))
        else:
            self._ck(self._L.ptc_set_display(self._h, None))
        return self

    def get_display(self):
        return self._get(self._L.ptc_get_display, PtcDisplayParams)

    def meter_exposure(self):
        """ptc_meter_exposure: meter the image select_output serves and move the adaptation state; queued, does not wait."""
        self._ck(self._L.ptc_meter_exposure(self._h))
        return self

    def exposure_reset(self):
        self._ck(self._L.ptc_exposure_reset(self._h))
        return self

    def exposure(self):
        """ptc_get_exposure (waits): the scale E a display call would use now, the adapted and the last metered luminance, the metered and rejected pixels."""
        e, a, m = C.c_float(0), C.c_float(0), C.c_float(0)
        n, r = C.c_uint64(0), C.c_uint64(0)
        self._ck(self._L.ptc_get_exposure(self._h, C.byref(e), C.byref(a), C.byref(m), C.byref(n), C.byref(r)))
        return {"scale": e.value, "adapted_luminance": a.value, "metered_luminance": m.value, "metered": n.value, "rejected": r.value}

    def exposure_state(self):
        """ptc_debug_display_state (waits): the integers of the state record, A (adaptation state), Q (last metering), N, M, rejected."""
        return dict(zip(("A", "Q", "N", "M", "rejected"), self._read(self._L.ptc_debug_display_state, 8, np.uint32, alloc=np.zeros).tolist()))

    def luminance_histogram(self):
        return self._read(self._L.ptc_read_luminance_histogram, LUMINANCE_BINS, np.uint32, alloc=np.zeros)

    def display(self):
        """ptc_display_rgba8: the served image through exposure, operator and transfer function: (h, w, 4) uint8."""
        return self._read(self._L.ptc_display_rgba8, (self._h_px, self._w, 4), np.uint8)

    def display_f16(self):
        """ptc_display_rgba16f: the served image times the exposure scale as RGBA16F: (h, w, 4) float16."""
        return self._read(self._L.ptc_display_rgba16f, (self._h_px, self._w, 4), np.uint16).view(np.float16)

    def display_f16_device_ptr(self) -> int:
        return int(self._L.ptc_display_rgba16f_device_ptr(self._h) or 0)

    def display_seconds(self):
        """(metering, display): HIP-event seconds of the last meter_exposure() and the last display() / display_f16()."""
        m, d = C.c_double(0), C.c_double(0)
        self._ck(self._L.ptc_get_display_seconds(self._h, C.byref(m), C.byref(d)))
        return m.value, d.value

    def display_internals(self):
        return self._read(self._L.ptc_debug_display_internals, 4, np.uint64, alloc=np.zeros).tolist()

    def stats(self):
        return self._get(self._L.ptc_get_stats, PtcStats)

    # ---- test hooks -------------------------------------------------------------------------------
    def trace_closest(self, origins, dirs):
        o, op = _f(origins)
        d, dp = _f(dirs)
        n = o.shape[0]
        t = np.zeros(n, np.float32)
        prim = np.zeros(n, np.int32)
        uv = np.zeros((n, 2), np.float32)
        self._ck(self._L.ptc_debug_trace_closest(self._h, op, dp, n, _ptr(t), _ptr(prim), _ptr(uv)))
        return t, prim, uv

    def trace_any(self, origins, dirs, tmax):
        o, op = _f(origins)
        d, dp = _f(dirs)
        tm, tp = _f(tmax)
        return self._read(self._L.ptc_debug_trace_any, o.shape[0], np.uint8, op, dp, tp, o.shape[0], alloc=np.zeros)

    def debug_camera_rays(self, w, h, seed, first_sample, n_samples, pixels=None):
        """ptc_debug_camera_rays: (origins, dirs), each (n_samples * n_pixels, 3) float32 in path order p = sample_local * n_pixels + j, of the path integrator's
        camera rays for `pixels` (indices y * w + x; None: every pixel in order) with the context's camera and lens."""
        px = np.arange(w * h, dtype=np.uint32) if pixels is None else np.ascontiguousarray(pixels, np.uint32).reshape(-1)
        n = px.size * int(n_samples)
        o, d = np.zeros((n, 3), np.float32), np.zeros((n, 3), np.float32)
        self._ck(self._L.ptc_debug_camera_rays(self._h, w, h, seed, first_sample, n_samples, _ptr(px), px.size, _ptr(o), _ptr(d)))
        return o, d

    def flat_scene(self):
        nv, nt = C.c_uint32(), C.c_uint32()
        self._ck(self._L.ptc_debug_get_flat_scene(self._h, C.byref(nv), C.byref(nt), None, None, None))
        verts = np.zeros((nv.value, 12), np.float32)
        idx = np.zeros((nt.value, 3), np.uint32)
        tm = np.zeros(nt.value, np.int32)
        self._ck(self._L.ptc_debug_get_flat_scene(self._h, None, None, verts.ctypes.data, _ptr(idx), _ptr(tm)))
        return verts, idx, tm

    def description(self):
        """Materials and textures as the context received them: ([(factors9, (tex_color, tex_normal, tex_mr))], [rgba arrays])."""
        nm, nt = C.c_int(0), C.c_int(0)
        self._ck(self._L.ptc_debug_get_description(self._h, C.byref(nm), C.byref(nt)))
        mats, texs = [], []
        for i in range(nm.value):
            f = np.zeros(9, np.float32)
            t = (C.c_int * 3)()
            self._ck(self._L.ptc_debug_get_material(self._h, i, _ptr(f), t))
            mats.append((f, tuple(t)))
        for i in range(nt.value):
            w, h = C.c_int(0), C.c_int(0)
            self._ck(self._L.ptc_debug_get_texture(self._h, i, C.byref(w), C.byref(h), None))
            px = np.zeros((h.value, w.value, 4), np.uint8)
            self._ck(self._L.ptc_debug_get_texture(self._h, i, C.byref(w), C.byref(h), px.ctypes.data))
            texs.append(px)
        return mats, texs

    def bvh(self):
        """(units, n_nodes, n_tris, grid): the BVH's unit array as (n_units, 4) float32 (see include/ptc.h), node / triangle-record
        counts and the origin grid (scene_lo.xyz, step.xyz)."""
        nn, nt, nu = C.c_uint32(), C.c_uint32(), C.c_uint32()
        self._ck(self._L.ptc_debug_get_bvh(self._h, C.byref(nn), C.byref(nt), C.byref(nu), None, None))
        units = np.zeros((nu.value, 4), np.float32)
        grid = np.zeros(6, np.float32)
        self._ck(self._L.ptc_debug_get_bvh(self._h, None, None, None, _ptr(units), _ptr(grid)))
        return units, nn.value, nt.value, grid

    def internals(self):
        buf = self._read(self._L.ptc_debug_get_internals, 8, np.uint64, alloc=np.zeros)
        keys = ("events_created", "spans_waiting", "queue_cap", "per_batch", "pending", "trace_blocks_per_cu", "stack_lds", "refit_on_device")
        d = {k: int(buf[i]) for i, k in enumerate(keys)}
        d["commit_on_device"] = (d["refit_on_device"] >> 1) & 1
        d["device_build_sah"] = (d["refit_on_device"] >> 2) & 1
        d["mesh_vertices_from_device"] = (d["refit_on_device"] >> 3) & 1
        d["refit_on_device"] &= 1
        return d

    def commit_host_parts(self):
        """The host's share of a commit on the device, checked against the host build (ptc_debug_commit_host_parts)."""
        buf = self._read(self._L.ptc_debug_commit_host_parts, 8, np.uint64, alloc=np.zeros)
        keys = ("n_tris", "n_lights", "indices_ok", "emitters_ok", "materials_ok", "tables_ok", "sizes_ok")
        return {k: int(buf[i]) for i, k in enumerate(keys)}

    def refit_host_parts(self):
        """The host's share of a refit on the device, checked against the host build (ptc_debug_refit_host_parts)."""
        buf = self._read(self._L.ptc_debug_refit_host_parts, 8, np.uint64, alloc=np.zeros)
        keys = ("n_verts", "n_tris", "nodes_listed", "levels", "emissive_prims", "levels_ok", "emitters_equal", "transforms_finite")
        return {k: int(buf[i]) for i, k in enumerate(keys)}

    def shading_tables(self):
        """(shade, lights, cdf): the per-primitive shading records as (n_tris, 4 * stride) float32, the emitter table (n, 20) and its cdf,
        as they lie in HBM (after a refit on the device they are read back first)."""
        stride, nl = C.c_uint32(), C.c_uint32()
        self._ck(self._L.ptc_debug_get_shading_tables(self._h, C.byref(stride), None, C.byref(nl), None, None))
        n = self.stats()["n_triangles"]
        shade = np.zeros((n, 4 * stride.value), np.float32)
        lights = np.zeros((max(nl.value, 1), 20), np.float32)
        cdf = np.zeros(max(nl.value, 1), np.float32)
        self._ck(self._L.ptc_debug_get_shading_tables(self._h, None, _ptr(shade), None, _ptr(lights), _ptr(cdf)))
        return shade, lights[:max(nl.value, 1)], cdf

    def shade_step(self, origins, dirs, throughput, prev_pdf, keys, bounce=0, max_bounces=8, variant=0):
        """ptc_debug_shade_step: explicit rays (path id = index) through k_trace_closest and one k_shade launch at `bounce`.  A dict of arrays per ray: t, word
        (the hit word, int32), uv, lpath (n, 3), alive, o / d / T (n, 3) and pdf of the continuation, shadow, so / sd (n, 3), tmax and contrib (n, 3) of the
        shadow record; rows without a record are zero.  variant: 0 the launch policy's kernel, 1 k_shade<SORT>, 2 k_shade<TABLES_LDS>."""
        o, op = _f(origins)
        d, dp = _f(dirs)
        T, Tp = _f(throughput)
        pp, ppp = _f(prev_pdf)
        k = np.ascontiguousarray(keys, np.uint32)
        n = o.shape[0]
        assert o.shape == d.shape == T.shape == (n, 3) and pp.shape == (n,) and k.shape == (n,)
        hit, lp = np.zeros((n, 4), np.float32), np.zeros((n, 3), np.float32)
        alive, sh = np.zeros(n, np.uint8), np.zeros(n, np.uint8)
        cont, srec = np.zeros((n, 10), np.float32), np.zeros((n, 10), np.float32)
        self._ck(self._L.ptc_debug_shade_step(self._h, op, dp, Tp, ppp, _ptr(k), n, int(bounce), int(max_bounces), int(variant), _ptr(hit), _ptr(lp), _ptr(alive),
                                              _ptr(cont), _ptr(sh), _ptr(srec)))
        return dict(t=hit[:, 0].copy(), word=hit[:, 1].copy().view(np.int32), uv=hit[:, 2:4].copy(), lpath=lp, alive=alive.astype(bool), o=cont[:, 0:3].copy(),
                    d=cont[:, 3:6].copy(), T=cont[:, 6:9].copy(), pdf=cont[:, 9].copy(), shadow=sh.astype(bool), so=srec[:, 0:3].copy(), sd=srec[:, 3:6].copy(),
                    tmax=srec[:, 6].copy(), contrib=srec[:, 7:10].copy())

    def env_tables(self):
        """ptc_debug_get_env_tables: (env (h, w, 4) float32 = radiance rgb and texel pmf, marg (h,), cond (h, w), ok) of the committed scene; empty arrays
        where the scene has no environment.  Works on a description-only context."""
        w, h, ok = C.c_int(0), C.c_int(0), C.c_int(0)
        self._ck(self._L.ptc_debug_get_env_tables(self._h, C.byref(w), C.byref(h), C.byref(ok), None, None, None))
        env, marg, cond = np.zeros((h.value, w.value, 4), np.float32), np.zeros(h.value, np.float32), np.zeros((h.value, w.value), np.float32)
        if env.size:
            self._ck(self._L.ptc_debug_get_env_tables(self._h, None, None, None, _ptr(env), _ptr(marg), _ptr(cond)))
        return env, marg, cond, bool(ok.value)

    def exact_arith(self, op, a=None, b=None, n=None, first=0, cross=False):
        """ptc_debug_exact_arith: fast path `op` (0 rcp, 1 sqrt, 2 rnorm, 3 div, 4 div3) of csrc/pt_exact.h against the compiler's / and sqrtf on the device.
        Explicit operands a (and b), or with a = None the n bit patterns from `first` on (hashed pairs for div and div3); cross: every a[i] with every b[j].
        Returns (mismatches, offenders): offenders (k, 4) uint32 = bits of a, b, the fast path's result and the reference's, k <= 16."""
        out = np.zeros(1 + 4 * 16, np.uint64)
        if a is None:
            ap = bp = None
        else:
            a = np.ascontiguousarray(a, np.float32)
            ap, n = _ptr(a), a.shape[0]
            b = None if b is None else np.ascontiguousarray(b, np.float32)
            assert b is None or b.shape == a.shape
            bp = None if b is None else _ptr(b)
        self._ck(self._L.ptc_debug_exact_arith(self._h, int(op), ap, bp, int(n), int(first) & 0xffffffff, int(bool(cross)), _ptr(out)))
        k = int(min(out[0], 16))
        return int(out[0]), out[1:1 + 4 * k].reshape(k, 4).astype(np.uint32)

    def raw_counters(self):
        buf = (C.c_uint64 * 32)()
        n = self._ck(self._L.ptc_debug_get_counters(self._h, buf, 32))
        return [int(buf[i]) for i in range(n)]


class Group:
    """ptc_group: one process driving several GPUs (n contexts + ncclCommInitAll).  `ctx(i)` is a PathTracer view of
    device i's context; load the same scene into each, then `render` (tiles sharded, RCCL reduce onto device 0)."""

    def __init__(self, device_ids):
        self._L = load_library()
        ids = (C.c_int * len(device_ids))(*[int(d) for d in device_ids])
        self._g = self._L.ptc_group_create(ids, len(device_ids))
        if not self._g:
            raise PtcError(self._L.ptc_group_last_error(None).decode())
        self.device_ids = [int(d) for d in device_ids]
        self._ctx = [PathTracer(d, _handle=self._L.ptc_group_ctx(self._g, i)) for i, d in enumerate(self.device_ids)]

    def __len__(self):
        return int(self._L.ptc_group_size(self._g))

    def _ck(self, rc):
        if rc < 0:
            raise PtcError(f"ptc error {rc}: {self._L.ptc_group_last_error(self._g).decode()}")
        return rc

    def ctx(self, i) -> PathTracer:
        return self._ctx[i]

    def load_scene(self, desc):
        """Describe the scene on device 0 and commit it to every device with ONE host build (ptc_group_scene_commit)."""
        self._ctx[0].load_scene(desc)
        self._ck(self._L.ptc_group_scene_commit(self._g))
        return self

    def scene_refit(self):
        """After ctx(0).update_instance(...): one host refit, uploaded to every device (ptc_group_scene_refit)."""
        self._ck(self._L.ptc_group_scene_refit(self._g))
        return self

    def render(self, w, h, spp, seed=1, max_bounces=8, integrator=INTEGRATOR_PATH):
        self._ck(self._L.ptc_group_render(self._g, w, h, spp, seed, max_bounces, integrator))
        for c in self._ctx:
            c._w, c._h_px = w, h
        return self._ctx[0].read_radiance()

    def close(self):
        if getattr(self, "_g", None):
            for c in self._ctx:
                c._h = None
            self._L.ptc_group_destroy(self._g)
            self._g = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
