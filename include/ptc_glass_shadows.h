/* ptc_glass_shadows.h - transparent shadows over the C-ABI: next-event light through thin-walled glass (csrc/pt_glass_shadow.h).
 *
 * ptc.h includes this header; include ptc.h.
 *
 * An extension of the core interface like ptc_glass.h, which it follows: in C and C++ the functions have the names below; libptc.so exports them as
 * ptcx_<name without its ptc_>, which the macros map.  A binding that looks symbols up by name (dlsym, ctypes) asks for the ptcx_ name. */
#ifndef PTC_GLASS_SHADOWS_H
#define PTC_GLASS_SHADOWS_H
#ifndef PTC_H
#error "include ptc.h, which includes this header"
#endif

#define ptc_set_glass_shadows ptcx_set_glass_shadows
#define ptc_get_glass_shadows ptcx_get_glass_shadows
#define ptc_get_glass_shadow_stats ptcx_get_glass_shadow_stats
#define ptc_debug_glass_any ptcx_debug_glass_any
#define ptc_debug_glass_shadow_transmit ptcx_debug_glass_shadow_transmit

#ifdef __cplusplus
extern "C" {
#endif

/* A thin-walled pane does not bend light, so a shadow ray may pass it with the pane's expected transmittance W = transmission x (1 - metallic) x (1 - F) x base
 * colour, F the reflectance of the pane's two faces: the probability with which a sampled path is transmitted, times the tint it receives.  With the feature
 * on, the shadow rays of the emitter, environment and punctual samples are walked through thin panes (and alpha surfaces, in the same walk), so a point, spot
 * or directional light lights what lies behind a window, and an emitter behind one is sampled directly.  A sampled path that only went straight through thin
 * panes then keeps its pdf for the MIS weight against those samples; a path that was reflected, or refracted by a solid, stays a delta path.  Solid glass
 * bends light and stays an occluder for shadow rays.
 * ptc_set_glass_shadows: on is 0 or 1 (default 0; PTC_E_ARG otherwise).  A context setting: kept across ptc_scene_begin; a frame renders with the value it was
 *   begun with; ptc_group_scene_commit hands context 0's value to the members.  With it off, or in a scene without a thin-walled transmissive material, a frame
 *   launches and computes what it did without this header.  It needs no device.
 * ptc_get_glass_shadows: the setting.
 * ptc_get_glass_shadow_stats: the shadow walk of the current frame (or of the last ptc_debug_glass_any call): `walked`: shadow records with something in their
 *   way, which entered the walk; `passes`: surfaces passed (thin panes and alpha surfaces); `visible`: walked records that reached their light; `exhausted`:
 *   records dropped because they would have passed more than max(ptc_set_glass_max_interactions, ptc_set_alpha_max_layers when the scene has alpha materials)
 *   surfaces.  Waits.  All zero on a context without a device.  The walk's time is part of ptc_glass_stats' seconds_glass; while it runs, ptc_alpha_stats'
 *   shadow counters stay 0: the alpha surfaces are passed by this walk. */
typedef struct ptc_glass_shadow_stats {
  uint64_t walked, passes, visible, exhausted;
} ptc_glass_shadow_stats;
int ptc_set_glass_shadows(ptc_ctx*, int on);
int ptc_get_glass_shadows(const ptc_ctx*, int* on);
int ptc_get_glass_shadow_stats(ptc_ctx*, ptc_glass_shadow_stats* out);

/* Test hooks.
 * ptc_debug_glass_any: n explicit shadow records (origin, direction, tmax) through the shadow resolution, as ptc_debug_alpha_any: per record the RGB
 *   transmittance instead of the addition to the path radiance (0 0 0: occluded) and the number of surfaces a visible record passed.  With the feature off, or
 *   in a scene without a thin-walled transmissive material, the transmittance is 0 or 1 from k_trace_any's flags and the layers are 0.  Preconditions and side
 *   effects as ptc_debug_trace_any; it clears the counters first.
 * ptc_debug_glass_shadow_transmit: csrc/pt_glass_shadow.h's pt_glass_shadow_transmit evaluated on the host for one hit; needs no context.  In: the material, the
 *   surface as orient_normals leaves it for wo = -d (ng, ns), the ray's direction d, base colour and metallic.  Out: W and the reflectance F_t it used.
 *   PTC_E_ARG for a null pointer. */
typedef struct ptc_glass_shadow_hit {
  float ng[3], ns[3], d[3];
  float base[3], metallic;
  float W[3], F_t;
} ptc_glass_shadow_hit;
int ptc_debug_glass_any(ptc_ctx*, const float* origins, const float* dirs, const float* tmax, uint32_t n, float* out_tr3, uint32_t* out_layers);
int ptc_debug_glass_shadow_transmit(const ptc_transmission_params*, ptc_glass_shadow_hit* io);

#ifdef __cplusplus
}
#endif
#endif /* PTC_GLASS_SHADOWS_H */
