/* ptc_medium.h - a homogeneous participating medium over the C-ABI: fog that scatters and absorbs inside an axis-aligned box, in the path integrator
 * (csrc/pt_medium.h).
 *
 * ptc.h includes this header; include ptc.h.
 *
 * An extension of the core interface, kept apart from it as ptc_glass.h is: the list of functions ptc.h declares and libptc.so exports under the prefix ptc_ is a
 * fixed contract of ABI version 4, so what is added without a new ABI version has a header and a symbol prefix of its own.  In C and C++ the functions have the
 * names below; libptc.so exports them as ptcx_<name without its ptc_>, which the macros map.  A binding that looks symbols up by name (dlsym, ctypes) asks for
 * the ptcx_ name. */
#ifndef PTC_MEDIUM_H
#define PTC_MEDIUM_H
#ifndef PTC_H
#error "include ptc.h, which includes this header"
#endif

#define ptc_set_medium ptcx_set_medium
#define ptc_get_medium ptcx_get_medium
#define ptc_clear_medium ptcx_clear_medium
#define ptc_get_medium_stats ptcx_get_medium_stats
#define ptc_debug_medium_sample ptcx_debug_medium_sample
#define ptc_debug_medium_step ptcx_debug_medium_step
#define ptc_debug_medium_env ptcx_debug_medium_env

#ifdef __cplusplus
extern "C" {
#endif

/* One homogeneous medium per context, inside the box [box_lo, box_hi].  A path segment that crosses the box may be scattered there (Henyey-Greenstein phase
 * function of anisotropy g, g > 0 scatters forward) with the single-scattering albedo as its weight; every scatter point samples the scene's lights - emissive
 * triangles, the environment, punctual lights - by next-event estimation, with MIS between that and the phase function's own sample; every shadow segment is
 * attenuated by exp(-sigma_t x its length inside the box).  sigma_t is one number for all channels: colour comes from albedo alone.
 *   box_lo, box_hi finite, lo < hi on every axis.  sigma_t finite and >= 0.  albedo each in [0, 1].  |g| <= 0.99.
 * ptc_set_medium / ptc_clear_medium only record; they need no device, no commit and no refit, and have the lifetime of the punctual lights: ptc_scene_begin drops
 *   the medium, a commit, a refit and a rebuild keep it.  A frame uses what was set when it began.  ptc_group_scene_commit and ptc_group_render hand context 0's
 *   medium to the members.  PTC_E_ARG, nothing changed: a null pointer or a value out of range.  sigma_t == 0, or no medium set, is "off": the context then
 *   launches, allocates and computes exactly what it did before this header existed.
 * ptc_get_medium: returns 1 and the parameters when a medium is set, else 0 and zeros.
 * ptc_get_medium_stats: of the current frame (or the last ptc_debug_medium_step): ray segments that crossed the box, scatter events, shadow records attenuated,
 *   and the seconds of the pass's kernels.  Waits.
 * A frame of PTC_INTEGRATOR_PATH with a medium on and a committed scene that has primitives with alpha coverage or transmissive materials is refused by
 * ptc_frame_begin with PTC_E_STATE: those passes walk several segments per bounce, which the medium does not follow yet.  Render such a scene without its alpha
 * modes or its transmission (ptc_render: --no-alpha, --no-transmission), or without the medium.  This is decided from the description and the host build before
 * the call looks for its device, so a description-only context reports PTC_E_STATE here and not PTC_E_DEVICE.
 * Limits: the raster integrators, ptc_frame_guides, the denoisers, the temporal history and ptc_focus_distance_at_pixel ignore the medium; probe frames honour
 * it.  No chromatic or heterogeneous extinction, no emission inside the medium, one medium. */
typedef struct ptc_medium_params {
  float box_lo[3], box_hi[3];
  float sigma_t;
  float albedo[3];
  float g;
} ptc_medium_params;
typedef struct ptc_medium_stats {
  uint64_t crossed, scattered, attenuated;
  double seconds_medium;
} ptc_medium_stats;
int ptc_set_medium(ptc_ctx*, const ptc_medium_params*);
int ptc_get_medium(const ptc_ctx*, ptc_medium_params* out);
int ptc_clear_medium(ptc_ctx*);
int ptc_get_medium_stats(ptc_ctx*, ptc_medium_stats* out);

/* Test hooks.
 * ptc_debug_medium_sample: the host's evaluation of csrc/pt_medium.h for one ray; needs no context.  In: the ray (o, d), the end of its segment t_end (a hit's
 *   t, or 3e38 for a miss), the three random numbers u0 (free flight), u1 (cosine), u2 (azimuth), and a shadow segment (so, sd, stmax).  Out: crosses (the span
 *   is not empty), t0, t1, the free-flight distance s (0 when the span is empty), scatters (s < t1), P, the sampled cosine, the direction wi and its pdf - the
 *   last three for (u1, u2) whether or not the ray scatters - and the transmittance of the shadow segment (1 where it misses the box).  PTC_E_ARG for a null
 *   pointer or parameters ptc_set_medium would refuse.
 * ptc_debug_medium_step: n explicit rays (origin, direction, throughput, previous pdf, key; path id = index) through k_set_counts, k_trace_closest and the medium
 *   pass of bounce `bounce` of a frame of `max_bounces`: k_medium_decide, k_shade, k_medium_append<0> and, when the context has punctual lights,
 *   k_shade_punctual and k_medium_append<1>, as run_batch launches them.  By path id: the hit record as k_shade saw it (4 floats), the continuation record as
 *   ten floats (o, d, T, pdf) and the two shadow records - emitter or environment, and punctual - as ten floats each (o, d, tmax, contribution), after
 *   attenuation; rows without a record are zero and their flag 0.  Preconditions and side effects as ptc_debug_shade_step; PTC_E_STATE without a medium.
 * ptc_debug_medium_env: the pass's own text of k_shade's environment sampler and lookup, on their own, for n items: out_dir = the direction sampled from
 *   (r1, r2), out_Le and out_pdf = the radiance and the solid-angle pdf the lookup gives for dir_in (unit vectors).  Needs a device and a committed scene with an
 *   environment of non-zero power (PTC_E_STATE otherwise); no medium needed.  A test holds out_dir to the shadow record k_shade writes for the same numbers. */
typedef struct ptc_medium_sample {
  float o[3], d[3], t_end;
  float u0, u1, u2;
  float so[3], sd[3], stmax;
  int crosses;
  float t0, t1, s;
  int scatters;
  float P[3], cos_theta, wi[3], pdf;
  float transmittance;
} ptc_medium_sample;
int ptc_debug_medium_sample(const ptc_medium_params*, ptc_medium_sample* io);
int ptc_debug_medium_step(ptc_ctx*, const float* origins, const float* dirs, const float* throughput, const float* prev_pdf, const uint32_t* keys, uint32_t n,
                          uint32_t bounce, uint32_t max_bounces, float* out_hit, uint8_t* out_alive, float* out_cont, uint8_t* out_shadow_valid, float* out_shadow,
                          uint8_t* out_punctual_valid, float* out_punctual);
int ptc_debug_medium_env(ptc_ctx*, const float* r1, const float* r2, const float* dir_in, uint32_t n, float* out_dir, float* out_Le, float* out_pdf);

#ifdef __cplusplus
}
#endif
#endif /* PTC_MEDIUM_H */
