/* ptc_lightmap.h - lightmaps over the C-ABI: path-traced irradiance on the surfaces of one instance, stored over the texels of its UV atlas
 * (csrc/pt_lightmap.h).  The other half of baked diffuse illumination beside the light probes of ptc.h: a texture a rasterizer samples with a
 * second UV set.
 *
 * ptc.h includes this header; include ptc.h.
 *
 * An extension of the core interface, kept apart from it as ptc_medium.h is: the list of functions ptc.h declares and libptc.so exports under the prefix ptc_ is a
 * fixed contract of ABI version 4, so what is added without a new ABI version has a header and a symbol prefix of its own.  In C and C++ the functions have the
 * names below; libptc.so exports them as ptcx_<name without its ptc_>, which the macros map.  A binding that looks symbols up by name (dlsym, ctypes) asks for
 * the ptcx_ name. */
#ifndef PTC_LIGHTMAP_H
#define PTC_LIGHTMAP_H
#ifndef PTC_H
#error "include ptc.h, which includes this header"
#endif

#define ptc_lightmap_begin ptcx_lightmap_begin
#define ptc_lightmap_texel_count ptcx_lightmap_texel_count
#define ptc_lightmap_read_texels ptcx_lightmap_read_texels
#define ptc_lightmap_read ptcx_lightmap_read
#define ptc_render_lightmap ptcx_render_lightmap
#define ptc_debug_lightmap_cover ptcx_debug_lightmap_cover
#define ptc_debug_lightmap_rays ptcx_debug_lightmap_rays
#define ptc_debug_lightmap_dilate ptcx_debug_lightmap_dilate

#ifdef __cplusplus
extern "C" {
#endif

/* A lightmap frame bakes ONE instance of the committed scene into an atlas of width x height texels.
 *
 * Coverage.  uv holds 2 floats per vertex of the instance's mesh (NULL: the mesh's own texcoord).  Each is clamped to [0, 1] and goes to fixed point with 8
 *   sub-texel bits; texel (x, y) has its centre at (x + 1/2, y + 1/2) / (width, height), row 0 at v = 0.  A triangle covers every centre inside it or on its
 *   edges (exactly: integer arithmetic), a triangle of zero UV area covers nothing, and where triangles overlap the one with the lowest index inside the mesh
 *   owns the texel.  A texel whose owner has zero area in the world is dropped (counted by ptc_lightmap_texel_count).  The covered texels, in ascending atlas
 *   index y * width + x, are the entries of the frame.
 * Rays.  An entry's position and shading normal are interpolated from the owner's world vertices - as the last commit, refit or rebuild left them, deformation
 *   included - and its origin is lifted off the surface by the scene's ray epsilon.  Every sample draws a cosine-weighted direction about the shading normal, so
 *   the irradiance is pi x the mean radiance; an emitter seen directly counts in full.  No next-event estimation at the texel and no direct term of punctual
 *   lights (the engine evaluates that itself, as with probes); from the first hit on the path is any other path: punctual lights, fog, alpha and glass behave as
 *   in a camera frame.  The random numbers of a texel depend on texel_index_base + its atlas index alone: shards of an atlas (the same atlas with other
 *   triangles, or rows of a larger one through the base) concatenate bit for bit.
 * ptc_lightmap_begin: begins the frame; ptc_frame_add_samples / ptc_frame_set_sample_range / ptc_sync work as in any frame, within spp_total.  PTC_E_ARG, and
 *   nothing changed, for a NULL pointer, an unknown instance, a width or height outside 1..8192, a non-finite uv, spp_total < 1, max_bounces < 0 or texel indices
 *   beyond 32 bits; PTC_E_STATE without a committed scene; then PTC_E_DEVICE on a description-only context.  No covered texel is no error.
 * ptc_lightmap_texel_count: the entries of the frame, and the owned texels dropped.  Either pointer may be NULL.
 * ptc_lightmap_read_texels: per entry the atlas index, the owning triangle's index inside the mesh, the ray origin (3 floats) and the normal (3 floats).  Any
 *   pointer may be NULL.
 * ptc_lightmap_read: the atlas as width * height RGBA floats, row 0 first: RGB the irradiance E = sum * (pi / N), N the samples accumulated or the resolve divisor
 *   of ptc_frame_set_sample_range; alpha 1 baked, 0.5 filled by dilation, 0 empty.  An entry whose first hit was a back face in more than backface_threshold
 *   of its N samples lies inside geometry: it is invalid and enters the dilation as empty (a threshold >= 1 switches the test off; 0.1 is a usual choice).  Each
 *   of the dilate_iters iterations gives every empty texel with a non-empty neighbour among its 8 the mean of those neighbours.  out_backface (or NULL): the
 *   back-face fraction per entry.  Waits.  PTC_E_ARG for a NULL out_rgba, dilate_iters outside 0..64, a negative or non-finite threshold.
 * ptc_render_lightmap: begin, spp_total samples, read.
 * PTC_E_STATE outside a lightmap frame for the three readers, and in a lightmap frame for everything a probe frame refuses and for ptc_probes_read_sh. */
typedef struct ptc_lightmap_desc {
  int instance;
  int width, height;
  const float* uv;
  uint32_t texel_index_base;
  int spp_total;
  uint64_t seed;
  int max_bounces;
} ptc_lightmap_desc;
int ptc_lightmap_begin(ptc_ctx*, const ptc_lightmap_desc*);
int ptc_lightmap_texel_count(ptc_ctx*, uint32_t* covered, uint32_t* dropped);
int ptc_lightmap_read_texels(ptc_ctx*, uint32_t* atlas_index, uint32_t* prim, float* origin_xyz, float* normal_xyz);
int ptc_lightmap_read(ptc_ctx*, int dilate_iters, float backface_threshold, float* out_rgba, float* out_backface);
int ptc_render_lightmap(ptc_ctx*, const ptc_lightmap_desc*, int dilate_iters, float backface_threshold, float* out_rgba);

/* Test hooks.  Each runs the definition (csrc/pt_lightmap.h) on the host for a description-only context and the kernels on a device context, where it ends the
 * frame in progress.
 * ptc_debug_lightmap_cover: the owner image of n_tris triangles (3 vertex indices each, below n_verts) with the UVs uv (2 floats per vertex) over a width x height
 *   atlas: per texel the lowest covering triangle, or 0xffffffff.  Needs no scene.
 * ptc_debug_lightmap_rays: the texel list of the description as ptc_lightmap_begin would make it (out_counts: entries, dropped; the four arrays of
 *   ptc_lightmap_read_texels, each sized for width * height entries), and the rays of n_samples samples from first_sample on in path order
 *   p = sample_local * entries + entry: 6 floats (origin, direction) and the key per path, sized for width * height * n_samples paths.  Any output but out_counts
 *   may be NULL.  The description's spp_total and max_bounces are not read.  PTC_E_STATE without a committed scene.
 * ptc_debug_lightmap_dilate: `iters` dilation iterations over a width x height RGBA image, in place.
 * PTC_E_ARG for a NULL pointer, sizes outside 1..8192, an index >= n_verts, n_samples = 0, more than 2^31 - 1 paths, sample or texel indices beyond 32 bits,
 * iters outside 0..64. */
int ptc_debug_lightmap_cover(ptc_ctx*, const uint32_t* indices, uint32_t n_tris, const float* uv, uint32_t n_verts, int width, int height, uint32_t* out_owner);
int ptc_debug_lightmap_rays(ptc_ctx*, const ptc_lightmap_desc*, uint32_t first_sample, uint32_t n_samples, uint32_t* out_counts, uint32_t* atlas_index, uint32_t* prim,
                            float* origin_xyz, float* normal_xyz, float* out_o_d, uint32_t* out_key);
int ptc_debug_lightmap_dilate(ptc_ctx*, int width, int height, int iters, float* rgba_inout);

#ifdef __cplusplus
}
#endif
#endif /* PTC_LIGHTMAP_H */
