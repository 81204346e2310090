/* ptc_alpha.h - alpha coverage over the C-ABI: glTF alphaMode MASK and BLEND in the path integrator (csrc/pt_alpha.h).
 *
 * ptc.h includes this header; include ptc.h.  The modes (PTC_ALPHA_OPAQUE / _MASK / _BLEND) are ptc.h's.
 *
 * An extension of the core interface, kept apart from it: the list of functions ptc.h declares and libptc.so exports under the prefix ptc_ is a fixed contract
 * of ABI version 4, held symbol for symbol, so what is added without a new ABI version has a header and a symbol prefix of its own.  In C and C++ the functions
 * have the names below; libptc.so exports them as ptcx_<name without its ptc_>, which the macros map.  A binding that looks symbols up by name (dlsym, ctypes)
 * asks for the ptcx_ name. */
#ifndef PTC_ALPHA_H
#define PTC_ALPHA_H
#ifndef PTC_H
#error "include ptc.h, which includes this header"
#endif

#define ptc_set_material_alpha ptcx_set_material_alpha
#define ptc_get_material_alpha ptcx_get_material_alpha
#define ptc_set_alpha_max_layers ptcx_set_alpha_max_layers
#define ptc_get_alpha_stats ptcx_get_alpha_stats
#define ptc_debug_alpha_closest ptcx_debug_alpha_closest
#define ptc_debug_alpha_any ptcx_debug_alpha_any
#define ptc_debug_alpha_decide ptcx_debug_alpha_decide
#define ptc_debug_get_alpha_tables ptcx_debug_get_alpha_tables

#ifdef __cplusplus
extern "C" {
#endif

/* Alpha coverage: glTF alphaMode (csrc/pt_alpha.h).  A material is OPAQUE (the default: every hit counts), MASK (a hit counts where the surface's
 * alpha reaches the cutoff) or BLEND (a hit counts with probability alpha; a shadow ray is attenuated by 1 - alpha).  The alpha of a hit is the base colour's
 * alpha times the colour texel's alpha, in the scene's filter mode.  The path integrator, the guides (ptc_frame_guides: deterministic, BLEND decides as MASK with
 * cutoff 0.5) and the probes honour it; the raster integrators, ptc_debug_trace_closest, ptc_debug_trace_any and ptc_debug_punctual_nee ignore it.
 * ptc_set_material_alpha belongs to the description: after ptc_add_material, before ptc_scene_commit (PTC_E_STATE once committed); it needs no device.
 *   PTC_E_ARG, nothing changed: an unknown mode, a material out of range, a cutoff that is not finite or outside [0, 1], a material whose emissive factor has a
 *   non-zero component (emitters are sampled by area without regard to coverage, so they stay opaque).  ptc_scene_begin drops all alpha state; a context that
 *   never calls this computes what it always did.
 * ptc_set_alpha_max_layers: how many surfaces one ray may pass through per trace (1 .. 16, default 8); a closest-hit ray that would pass one more stops at
 *   that surface, a shadow ray that would is occluded, both counted as exhausted.  A context setting: kept across ptc_scene_begin; a frame renders with the value it was begun with.
 * ptc_get_alpha_stats: the passes of the current frame (or of the last ptc_debug_alpha_* call): closest-hit rays passed on, shadow records walked through their
 *   occluders, surfaces shadow rays passed, exhausted rays, and the seconds of the resolutions (their trace launches included).  Waits. */
typedef struct ptc_alpha_stats {
  uint64_t closest_passes, shadow_walked, shadow_passes, exhausted;
  double seconds_alpha;
} ptc_alpha_stats;
int ptc_set_material_alpha(ptc_ctx*, int material, int mode, float cutoff);
int ptc_get_material_alpha(const ptc_ctx*, int material, int* mode, float* cutoff);
int ptc_set_alpha_max_layers(ptc_ctx*, int n);
int ptc_get_alpha_stats(ptc_ctx*, ptc_alpha_stats* out);

/* Test hooks.
 * ptc_debug_alpha_closest: n explicit rays in identity layout with the given RNG keys through k_trace_closest and the closest-hit resolution of `bounce`
 *   (deterministic != 0: the guides' form).  Per ray the final hit record — t (-1: miss), primitive id, barycentrics — and the layers it passed.
 * ptc_debug_alpha_any: n explicit shadow rays through the shadow resolution: the transmittance per ray, 0 when occluded.
 *   Both: preconditions and side effects as ptc_debug_trace_closest; they clear the alpha counters first.  A scene without alpha materials gives the plain trace results.
 * ptc_debug_alpha_decide: pt_alpha_accept and pt_alpha_transmit evaluated on the host; needs no context.  PTC_E_ARG for an unknown mode.
 * ptc_debug_get_alpha_tables: the tables of the committed scene as the pass reads them: one bit per primitive id ((n_prims + 31) / 32 words), set when the
 *   material is not OPAQUE, and (mode as int bits, cutoff) per material.  Sizes come back through the pointers; arrays may be null.  Works on a description-only
 *   context.  Returns 1 when an alpha queue is allocated on one of the context's lanes, else 0 (or an error). */
int ptc_debug_alpha_closest(ptc_ctx*, const float* origins, const float* dirs, const uint32_t* keys, uint32_t n, uint32_t bounce, int deterministic,
                            float* out_t, int32_t* out_prim, float* out_uv, uint32_t* out_layers);
int ptc_debug_alpha_any(ptc_ctx*, const float* origins, const float* dirs, const float* tmax, uint32_t n, float* out_transmittance);
int ptc_debug_alpha_decide(int mode, float cutoff, float a, float u, int* accept, float* transmit);
int ptc_debug_get_alpha_tables(ptc_ctx*, uint32_t* n_prims, uint32_t* bits, uint32_t* n_mats, float* mode_cutoff);

#ifdef __cplusplus
}
#endif
#endif /* PTC_ALPHA_H */
