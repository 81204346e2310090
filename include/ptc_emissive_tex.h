/* ptc_emissive_tex.h - textured emission over the C-ABI: glTF emissiveTexture as a light set of its own in the path integrator (csrc/pt_emissive_tex.h,
 * DESIGN.md 2h).
 *
 * ptc.h includes this header; include ptc.h.
 *
 * An extension of the core interface, kept apart from it as ptc_glass.h is: in C and C++ the functions have the names below; libptc.so exports them as
 * ptcx_<name without its ptc_>, which the macros map.  A binding that looks symbols up by name (dlsym, ctypes) asks for the ptcx_ name. */
#ifndef PTC_EMISSIVE_TEX_H
#define PTC_EMISSIVE_TEX_H
#ifndef PTC_H
#error "include ptc.h, which includes this header"
#endif

#define ptc_set_material_emission_texture ptcx_set_material_emission_texture
#define ptc_get_material_emission_texture ptcx_get_material_emission_texture
#define ptc_get_emissive_tex_stats ptcx_get_emissive_tex_stats
#define ptc_debug_get_emissive_tex_table ptcx_debug_get_emissive_tex_table
#define ptc_debug_emissive_tex_sample ptcx_debug_emissive_tex_sample
#define ptc_debug_emissive_tex_step ptcx_debug_emissive_tex_step

#ifdef __cplusplus
extern "C" {
#endif

/* Emission texture of a material.  The radiance leaving a front-facing point of the material's surfaces is factor x texel(u, v): the texel is fetched with the
 * scene's filter mode and REPEAT from the texture `texture` (an id of ptc_add_texture_rgba8) at the vertices' texture coordinates, as texel / 255 without an
 * sRGB decode; emission is one-sided.  The path integrator samples these surfaces as a light set of its own, once per bounce, behind the emitter / environment
 * sample and the punctual sample; what it finds adds to theirs.
 *   ptc_set_material_emission_texture belongs to the description: after ptc_add_material, before ptc_scene_commit (PTC_E_STATE once committed); it needs no
 *   device.  texture = -1 removes the material's emission texture (factor is not read).  PTC_E_ARG, nothing changed: a null pointer, a material or texture out of
 *   range, a factor that is not finite and >= 0, a material whose emissive factor has a non-zero component (its base emission stays 0: give the colour as
 *   `factor`), a material whose alpha mode is not OPAQUE or whose transmission is above 0.  ptc_set_material_alpha and ptc_set_material_transmission likewise
 *   refuse a material that has an emission texture: an emitter stays opaque.  ptc_scene_begin drops all of it; a context that never calls this, or has removed
 *   every emission texture again, launches and computes what it always did.
 *   ptc_frame_begin refuses (PTC_E_STATE) a path-integrator frame with a medium (ptc_medium.h) over a committed scene that has an emission texture: a scatter
 *   point has no sampler for this set.
 * ptc_get_emissive_tex_stats: entries of the committed scene's table (one per primitive of such a material), and of the current frame (or the last
 *   ptc_debug_emissive_tex_step call) the hit-side additions, the shadow records written and the seconds of the pass's own kernel.  Its shadow traces count in
 *   ptc_stats' seconds_trace_any, launches_trace_any and shadow_rays.  Waits.
 * Limits: no sRGB decode of the texture, no KHR_texture_transform, texture coordinate set 0 only; ptc_frame_guides and the denoisers see the surface under the
 * emission; the raster integrators and the oracle ignore the texture; entries are weighted per triangle, not per texel; not inside a medium. */
typedef struct ptc_emissive_tex_stats {
  uint64_t entries, hit_additions, shadow_records;
  double seconds_emissive_tex;
} ptc_emissive_tex_stats;
int ptc_set_material_emission_texture(ptc_ctx*, int material, int texture, const float factor[3]);
int ptc_get_material_emission_texture(const ptc_ctx*, int material, int* texture, float factor[3]);
int ptc_get_emissive_tex_stats(ptc_ctx*, ptc_emissive_tex_stats* out);

/* Test hooks.
 * ptc_debug_get_emissive_tex_table: the table of the committed scene as the pass reads it: 28 floats per entry - (p0, area) (e1, pmf) (e2, texture id as int
 *   bits) (n, 0) (factor, 0) (uv of a, uv of b) (uv of c, 0, 0) -, the cdf, the entry of every primitive (-1: none) and the sum of the weights (0: the sample side
 *   is off).  Sizes come back through the pointers; arrays may be null.  Works on a description-only context.
 * ptc_debug_emissive_tex_sample: csrc/pt_emissive_tex.h evaluated on the host for one entry (28 floats as above, its texture id ignored) over one RGBA8 texture
 *   of w x h texels with the filter PTC_FILTER_*; needs no context.  In: the shading point P and the numbers (r1, r2) of the sample; the hit's barycentrics
 *   (hit_u, hit_v), bounce, pdf word, distance and cosine of the hit side.  Out: ok (the sample exists), y, wi, pl, Le of the sample; hit_Le and hit_weight.
 *   PTC_E_ARG for a null pointer or a bad size or filter.
 * ptc_debug_emissive_tex_step: n explicit rays in identity layout with the given throughput, pdf word and RNG keys through k_trace_closest and ONE launch of
 *   k_shade_emissive_tex at `bounce` of `max_bounces`.  lpath (rgb per ray) is in and out: in, the radiance each path carries so far; out, the same with what the
 *   hit side added.  The shadow record a ray wrote, by path id: valid, then ten floats (origin, direction, tmax, contribution).  Where the committed
 *   scene has alpha materials the hits are resolved by the alpha pass of `bounce` first, as a frame resolves them (ptc_debug_alpha_closest's launches; it clears the
 *   alpha counters); transmission is ignored.  Preconditions and side effects as ptc_debug_punctual_nee; it clears the pass's counters first.
 *   PTC_E_STATE when the committed scene has no emission texture. */
typedef struct ptc_emissive_tex_sample {
  float P[3], r1, r2;
  float hit_u, hit_v;
  uint32_t bounce;
  float prev_pdf, hit_t, hit_cos;
  int ok;
  float y[3], wi[3], pl, Le[3];
  float hit_Le[3], hit_weight;
} ptc_emissive_tex_sample;
int ptc_debug_get_emissive_tex_table(ptc_ctx*, uint32_t* n_entries, float* records28, float* cdf, uint32_t* n_prims, int32_t* prim_map, float* total);
int ptc_debug_emissive_tex_sample(const float entry28[28], const uint8_t* rgba, int w, int h, int filter, ptc_emissive_tex_sample* io);
int ptc_debug_emissive_tex_step(ptc_ctx*, const float* origins, const float* dirs, const float* throughput, const float* prev_pdf, const uint32_t* keys, uint32_t n,
                                uint32_t bounce, uint32_t max_bounces, float* lpath, uint8_t* out_shadow_valid, float* out_shadow10);

#ifdef __cplusplus
}
#endif
#endif /* PTC_EMISSIVE_TEX_H */
