/* ptc_camera.h - camera models over the C-ABI: a camera given by its camera-to-world matrix (any orientation, roll included) with a perspective, an
 * orthographic or a 360-degree equirectangular projection (csrc/pt_camera.h).
 *
 * ptc.h includes this header; include ptc.h.
 *
 * An extension of the core interface, kept apart from it as ptc_medium.h is: the list of functions ptc.h declares and libptc.so exports under the prefix ptc_ is a
 * fixed contract of ABI version 4, so what is added without a new ABI version has a header and a symbol prefix of its own.  In C and C++ the functions have the
 * names below; libptc.so exports them as ptcx_<name without its ptc_>, which the macros map.  A binding that looks symbols up by name (dlsym, ctypes) asks for
 * the ptcx_ name. */
#ifndef PTC_CAMERA_H
#define PTC_CAMERA_H
#ifndef PTC_H
#error "include ptc.h, which includes this header"
#endif

#define ptc_camera_default_params ptcx_camera_default_params
#define ptc_set_camera_ex ptcx_set_camera_ex
#define ptc_get_camera_ex ptcx_get_camera_ex
#define ptc_debug_read_guide_positions ptcx_debug_read_guide_positions

#ifdef __cplusplus
extern "C" {
#endif

/* The camera of ptc_set_camera is the reference viewer's: a look-at basis with the up vector fixed at (0, -1, 0) and a perspective projection.  The extended
 * camera is glTF's: camera_to_world maps camera space - the camera looks along -Z, +Y is up, +X is right - to the world, and the image is upright and not
 * mirrored: row 0 is the top (+Y), column 0 the left (-X).
 *   The basis, in binary32: X, Y, Z = the normalised columns 0, 1, 2 of the matrix, pos = column 3; image right s = X, image down u = -Y, forward f = -Z.
 *   PTC_PROJ_PERSPECTIVE    yfov in (0, pi) radians, aspect > 0: the pinhole (or, with ptc_set_camera_lens, the thin lens) of ptc_set_camera on that basis.
 *   PTC_PROJ_ORTHOGRAPHIC   xmag, ymag > 0, glTF's half extents: parallel rays along f from the rectangle [-xmag, xmag] x [-ymag, ymag] of the plane through pos.
 *   PTC_PROJ_EQUIRECT       every direction around pos, as a latitude-longitude image: with the identity rotation, pixel (x, y) of a w x h frame looks where
 *                           texel (x, y) of a w x h environment of ptc_set_env_latlong_rgb32f lies (row 0 = +y, u = atan2(d.z, d.x) / 2 pi + 1/2), so a panorama
 *                           is an environment map of the point it was taken from.  yfov, aspect and the mags are ignored; a caller wants w = 2 h.
 * ptc_camera_default_params: perspective, the identity matrix, yfov pi / 2, aspect 1, xmag = ymag = 1.
 * ptc_set_camera_ex only records; it needs no device.  It and ptc_set_camera replace one another: the last call wins.  ptc_scene_begin drops the extended camera; a
 *   commit, a refit and a rebuild keep it; ptc_group_scene_commit copies it wherever it copies the camera.  During a frame it applies to the batches queued
 *   afterwards and invalidates the guides, as ptc_set_camera does.
 *   PTC_E_ARG, nothing changed: a null pointer; an unknown projection; a matrix entry that is not finite; a column 0..2 of zero length; columns that are not
 *   orthogonal (a pairwise |dot| of the normalised columns above 1e-4); a left-handed frame (dot(cross(X, Y), Z) <= 0); yfov, aspect (PERSPECTIVE) or xmag, ymag
 *   (ORTHOGRAPHIC) outside their ranges.  The columns are normalised, so a uniform scale inherited from parent nodes is accepted; nothing is re-orthogonalised.
 *   PTC_E_STATE, nothing changed: ORTHOGRAPHIC or EQUIRECT while a raster frame is in progress (ptc_frame_begin would have refused that frame).
 * ptc_get_camera_ex: returns 1 and the parameters as they were set when an extended camera is in force, else 0 and zeros.
 * An extended PERSPECTIVE camera is served by everything that serves ptc_set_camera's.  Under ORTHOGRAPHIC and EQUIRECT: PTC_INTEGRATOR_PATH frames, adaptive
 *   frames, tile shares, ptc_frame_guides, ptc_denoise, ptc_denoise_sampled and ptc_debug_camera_rays work; a raster integrator is refused by ptc_frame_begin,
 *   and ptc_temporal_accumulate, ptc_denoise_accumulated and ptc_focus_distance_at_pixel are refused, each with PTC_E_STATE and a message that names the
 *   projection, decided before the call looks for its device.  The thin lens applies to PERSPECTIVE alone; the other two ignore it (it is still recorded).
 * Limits: no fisheye and no cube-face projection; no prefiltering of a panorama into roughness mips; no temporal reprojection and no pixel focusing under
 *   ORTHOGRAPHIC / EQUIRECT, and no lens for them; no near / far clipping (glTF's znear and zfar are not applied: the path integrator clips nowhere, and
 *   orthographic rays start on the plane through pos); no motion blur. */
enum { PTC_PROJ_PERSPECTIVE = 0, PTC_PROJ_ORTHOGRAPHIC = 1, PTC_PROJ_EQUIRECT = 2 };
typedef struct ptc_camera_params {
  int   projection;
  float camera_to_world[16]; /* column-major; glTF camera space: looks along -Z, +Y up, +X right */
  float yfov, aspect;        /* PERSPECTIVE: radians in (0, pi); aspect > 0 */
  float xmag, ymag;          /* ORTHOGRAPHIC: half extents, > 0 (glTF xmag / ymag) */
} ptc_camera_params;
void ptc_camera_default_params(ptc_camera_params*);
int  ptc_set_camera_ex(ptc_ctx*, const ptc_camera_params*);
int  ptc_get_camera_ex(const ptc_ctx*, ptc_camera_params* out);

/* Test hook.
 * ptc_debug_read_guide_positions: the third guide buffer of the current frame's ptc_frame_guides, which ptc_read_guide_rgba32f does not serve: (P.xyz, K) per pixel,
 *   P = origin + Z direction of the pixel-centre ray of the camera in force (0 + the origin on a miss), K the class.  w x h x 4 floats.  Needs a device; PTC_E_STATE
 *   without valid guides.  Waits. */
int  ptc_debug_read_guide_positions(ptc_ctx*, float* out_rgba32f);

#ifdef __cplusplus
}
#endif
#endif /* PTC_CAMERA_H */
