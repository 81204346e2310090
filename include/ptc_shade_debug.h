/* ptc_shade_debug.h - test hooks around k_shade over the C-ABI: one shading step of explicit rays, and the environment tables (csrc/pt_kernels.hip P5-P8,
 * DESIGN.md 1b).
 *
 * ptc.h includes this header; include ptc.h.
 *
 * An extension of the core interface like ptc_alpha.h, which it follows: in C and C++ the functions have the names below; libptc.so exports them as
 * ptcx_<name without its ptc_>, which the macros map.  A binding that looks symbols up by name (dlsym, ctypes) asks for the ptcx_ name. */
#ifndef PTC_SHADE_DEBUG_H
#define PTC_SHADE_DEBUG_H
#ifndef PTC_H
#error "include ptc.h, which includes this header"
#endif

#define ptc_debug_shade_step ptcx_debug_shade_step
#define ptc_debug_get_env_tables ptcx_debug_get_env_tables

#ifdef __cplusplus
extern "C" {
#endif

/* Test hooks.
 * ptc_debug_shade_step: n explicit rays in identity layout (path id = index) with the given throughputs, previous pdfs and RNG keys through k_set_counts,
 *   k_trace_closest and ONE launch of k_shade at `bounce` of a frame of `max_bounces`; the path radiance of the n paths is zeroed first.  variant: 0 = the
 *   kernel the launch policy picks for the committed scene, 1 = k_shade<SORT>, 2 = k_shade<TABLES_LDS>.  Results per ray, de-compacted by the path id each record
 *   carries:
 *     out_hit[n][4]       t (-1: miss), the hit word (primitive | class << 28, -1: miss) as int bits, u, v
 *     out_lpath[n][3]     what the step added to the path radiance (emission, environment)
 *     out_alive[n]        1: the path goes on, with out_cont[n][10] = origin, direction, throughput, pdf
 *     out_shadow_valid[n] 1: the step produced a shadow record, with out_shadow[n][10] = origin, direction, tmax, contribution
 *   Rows of paths without a record are zero.  Preconditions and side effects as ptc_debug_trace_closest.
 *   PTC_E_ARG before anything is launched: a null pointer, n = 0, bounce or max_bounces out of [0, 2^20], a variant that is not 0, 1 or 2, a direction that is
 *   not finite or whose length differs from 1 by more than 1e-3, an origin, throughput or pdf that is not finite.
 *   PTC_E_STATE: the scene has a material with alpha coverage or transmission (those passes sit between the trace and the shading); variant 2 for a scene
 *   whose tables do not fit k_shade's copies in LDS.
 *   PTC_E_DEVICE: a record whose path id is out of range or taken twice, a segment with more records than slots.
 * ptc_debug_get_env_tables: the environment tables of the committed scene as k_shade reads them: env[h][w][4] = radiance rgb and the texel's pmf, marg[h] the
 *   row cdf, cond[h][w] the column cdf of every row; ok = the map has power (it is importance-sampled).  Sizes come back through the pointers; arrays may be
 *   null.  A scene without environment has w = h = 0.  Works on a description-only context. */
int ptc_debug_shade_step(ptc_ctx*, const float* origins, const float* dirs, const float* throughput, const float* prev_pdf, const uint32_t* keys, uint32_t n,
                         uint32_t bounce, uint32_t max_bounces, int variant, float* out_hit, float* out_lpath, uint8_t* out_alive, float* out_cont,
                         uint8_t* out_shadow_valid, float* out_shadow);
int ptc_debug_get_env_tables(ptc_ctx*, int* w, int* h, int* ok, float* env, float* marg, float* cond);

#ifdef __cplusplus
}
#endif
#endif /* PTC_SHADE_DEBUG_H */
