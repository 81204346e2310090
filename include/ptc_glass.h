/* ptc_glass.h - dielectric transmission over the C-ABI: glass and thin-walled glTF materials in the path integrator (csrc/pt_glass.h).
 *
 * ptc.h includes this header; include ptc.h.
 *
 * An extension of the core interface, kept apart from it as ptc_alpha.h is: the list of functions ptc.h declares and libptc.so exports under the prefix ptc_ is a
 * fixed contract of ABI version 4, so what is added without a new ABI version has a header and a symbol prefix of its own.  In C and C++ the functions have the
 * names below; libptc.so exports them as ptcx_<name without its ptc_>, which the macros map.  A binding that looks symbols up by name (dlsym, ctypes) asks for
 * the ptcx_ name. */
#ifndef PTC_GLASS_H
#define PTC_GLASS_H
#ifndef PTC_H
#error "include ptc.h, which includes this header"
#endif

#define ptc_transmission_default_params ptcx_transmission_default_params
#define ptc_set_material_transmission ptcx_set_material_transmission
#define ptc_get_material_transmission ptcx_get_material_transmission
#define ptc_set_glass_max_interactions ptcx_set_glass_max_interactions
#define ptc_get_glass_stats ptcx_get_glass_stats
#define ptc_debug_glass_closest ptcx_debug_glass_closest
#define ptc_debug_glass_interact ptcx_debug_glass_interact
#define ptc_debug_get_glass_tables ptcx_debug_get_glass_tables

#ifdef __cplusplus
extern "C" {
#endif

/* Transmission of a material (KHR_materials_transmission, KHR_materials_ior, KHR_materials_volume).  With probability transmission x (1 - metallic) a path that
 * hits the surface meets a smooth dielectric interface of the given index of refraction, tinted by the base colour on the way in, instead of the surface
 * k_shade shades: it is reflected or refracted (a thin-walled material: passes straight on, with the reflectance of the pane's two faces) and traced again.
 * A solid (thin_walled = 0) attenuates what travels inside it: attenuation_color is what is left of white after attenuation_distance (0: no attenuation).
 *   transmission in [0, 1], default 0.  ior >= 1 and finite, default 1.5.  thin_walled 0 | 1, default 1 (glTF's meaning of "no volume").
 *   attenuation_color[3] in (0, 1], default 1.  attenuation_distance >= 0 and finite, default 0 = none.
 * ptc_set_material_transmission belongs to the description: after ptc_add_material, before ptc_scene_commit (PTC_E_STATE once committed); it needs no device.
 *   PTC_E_ARG, nothing changed: a null pointer, a material out of range, a value out of range, an emissive material, a material whose alpha mode is not OPAQUE.
 *   ptc_set_material_alpha likewise refuses a material whose transmission is above 0.  ptc_scene_begin drops all of it; a context that never calls this, or
 *   whose materials all have transmission 0, launches and computes what it always did.
 * ptc_set_glass_max_interactions: how many interface events one ray may have between two shaded hits (1 .. 32, default 8); a ray that would have one more ends
 *   without a contribution, counted as exhausted.  A context setting: kept across ptc_scene_begin; a frame renders with the value it was begun with.
 * ptc_get_glass_stats: the events of the current frame (or of the last ptc_debug_glass_closest call): reflections, refractions, `standing`: rays that ended
 *   the pass after at least one event with a result for k_shade, a hit that stood or a miss alike, exhausted rays (not in `standing`), and the seconds of the
 *   resolutions (their trace launches included).  Waits.  The segments the pass traces keep statistics of their own that nobody reads: ptc_stats' segments,
 *   hits, node visits, triangle tests and launches_trace_closest count the batch's own trace per bounce and leave out the continuation segments of the glass
 *   pass, as they leave out those of the alpha pass.  Where the scene also has alpha materials, the alpha resolutions of the continuations run inside this
 *   pass and their time is part of seconds_glass AND of ptc_alpha_stats' seconds_alpha: the two are not to be added.
 * Limits: no eta^2 radiance scaling; roughness is ignored for the interface; shadow rays of every kind see a transmissive surface as an occluder unless
 * ptc_set_glass_shadows (ptc_glass_shadows.h) lets them pass thin panes, so light otherwise reaches things behind glass only along sampled paths that hit an emitter or the environment; ptc_frame_guides, the denoisers, the temporal reprojection and
 * ptc_focus_distance_at_pixel see glass as the surface; the raster integrators and the other debug hooks ignore transmission. */
typedef struct ptc_transmission_params {
  float transmission, ior;
  int thin_walled;
  float attenuation_color[3];
  float attenuation_distance;
} ptc_transmission_params;
typedef struct ptc_glass_stats {
  uint64_t reflections, refractions, standing, exhausted;
  double seconds_glass;
} ptc_glass_stats;
void ptc_transmission_default_params(ptc_transmission_params* out);
int ptc_set_material_transmission(ptc_ctx*, int material, const ptc_transmission_params*);
int ptc_get_material_transmission(const ptc_ctx*, int material, ptc_transmission_params* out);
int ptc_set_glass_max_interactions(ptc_ctx*, int n);
int ptc_get_glass_stats(ptc_ctx*, ptc_glass_stats* out);

/* Test hooks.
 * ptc_debug_glass_closest: n explicit rays in identity layout with throughput 1 and the given RNG keys through k_trace_closest, the alpha resolution when the
 *   scene has one, and the glass resolution of `bounce`.  Per ray the final hit record - t (-1: miss), primitive id (-1: miss), barycentrics - the final ray
 *   record as ten floats (o, d, T, and the pdf word, which is 1 where the ray had no event) and the number of events j.  Preconditions and side effects as
 *   ptc_debug_trace_closest; it clears the glass counters first.  A scene without transmissive materials gives the plain trace results.
 * ptc_debug_glass_interact: steps 2 to 4 of csrc/pt_glass.h evaluated on the host for one hit; needs no context.  In: the material, the surface as
 *   orient_normals leaves it (P, ng, ns, front), the ray's direction d, throughput T and the hit's t, base colour and metallic, the two random numbers, j,
 *   max_interactions and the ray epsilon.  Out: outcome (0 the hit stands, 1 exhausted, 2 reflected, 3 transmitted), o, d, T after it and the reflectance F
 *   the event used.  PTC_E_ARG for a null pointer or a t that is not finite.
 * ptc_debug_get_glass_tables: the tables of the committed scene as the pass reads them: one bit per primitive id ((n_prims + 31) / 32 words), set when the
 *   material's transmission is above 0, and eight floats per material (transmission, ior, thin as int bits, 0, sigma2 x y z, 0).  Sizes come back through the
 *   pointers; arrays may be null.  Works on a description-only context.  Returns 1 when a glass queue is allocated on one of the context's lanes, else 0. */
typedef struct ptc_glass_interaction {
  float P[3], ng[3], ns[3];
  int front;
  float d[3], T[3], t;
  float base[3], metallic;
  float u_s, u_e;
  uint32_t j, max_interactions;
  float ray_eps;
  int outcome;
  float o_out[3], d_out[3], T_out[3], F;
} ptc_glass_interaction;
int ptc_debug_glass_closest(ptc_ctx*, const float* origins, const float* dirs, const uint32_t* keys, uint32_t n, uint32_t bounce,
                            float* out_t, int32_t* out_prim, float* out_uv, float* out_ray10, uint32_t* out_j);
int ptc_debug_glass_interact(const ptc_transmission_params*, ptc_glass_interaction* io);
int ptc_debug_get_glass_tables(ptc_ctx*, uint32_t* n_prims, uint32_t* bits, uint32_t* n_mats, float* mats8);

#ifdef __cplusplus
}
#endif
#endif /* PTC_GLASS_H */
