// pt_camera.h — camera models: the orthographic and the equirectangular (360-degree panoramic) projection of an extended camera (include/ptc_camera.h,
// DESIGN.md §2j).
//
// A camera model lives in ray generation alone, as the thin lens does (pt_lens.h): a projection decides the origin and the direction written into the first
// ray queue, and nothing behind it.  The functions below are the definition — IEEE binary32, no contraction (-ffp-contract=off), in the order written, pt_fma =
// one rounding; the host evaluation (ptc_debug_camera_rays on a description-only context) and the kernels (pt_camera.hip) both call them, so the device writes
// the bytes the host computes.  tests/camera_reference.py restates them in numpy.
//
// The basis is DevCamera's: ptc_set_camera_ex fills pos = column 3 of the matrix and s = X, u = -Y, f = -Z from its normalised columns X, Y, Z (image right, image
// down — row 0 is the top —, forward).  PERSPECTIVE has no function here: with sy = (float)tan((double)yfov / 2), sx = aspect sy in that DevCamera it is k_raygen /
// pt_lens_ray, and every kernel that reads a DevCamera serves it as it is.  What DevCamera has no room for, the projection and its parameters, travels beside it
// in PtCamProj, as ptc_lens_params travels beside it.
//
// For (pixel, sample) of a w x h frame, key, jx, jy, fx, fy are exactly k_raygen's: key = path_key(seed_hash, pixel, sample), (jx, jy) = rng_f(key, 0, 0 / 1),
// fx = (px + jx) / w, fy = (py + jy) / h.
//   ORTHOGRAPHIC   ox = (2 fx - 1) xmag, oy = (2 fy - 1) ymag; o = vfma(s, ox, vfma(u, oy, pos)); d = f.
//   EQUIRECT       t = fx + 0.5; t = t - floor(t); (sp, cp) = sincos2pi(t); (st, ct) = sincos2pi(0.5 fy); the camera-space direction is (st cp, ct, st sp);
//                  d = normalize3(vfma(X, st cp, vfma(Y, ct, Z * (st sp)))) with X = s, Y = -u, Z = -f (a negation is exact); o = pos.
//                  With the identity rotation this inverts the environment lookup of ptc_set_env_latlong_rgb32f: row 0 = +y, u = atan2(d.z, d.x) / 2 pi + 1/2.
// The pixel-centre guide ray is the same arithmetic with the jitter (0.5, 0.5).
// Limits: no fisheye, no cube faces; the thin lens, the temporal reprojection and ptc_focus_distance_at_pixel are PERSPECTIVE's alone; no near / far clipping
// (orthographic rays start on the plane through pos); no motion blur.
#pragma once
#include "../../include/ptc.h"
#include "ptc_internal.h"
#include "pt_device.h"

struct PtCamProj { int projection; float xmag, ymag; };      // PTC_PROJ_*, and ORTHOGRAPHIC's half extents

// origin and unit direction of the image point (fx, fy) in [0, 1)^2 under ORTHOGRAPHIC or EQUIRECT
PT_HD void pt_proj_point(const DevCamera& cam, const PtCamProj& P, float fx, float fy, float o[3], float d[3]) {
  const v3 s = V3(cam.s), u = V3(cam.u), f = V3(cam.f), pos = V3(cam.pos);
  v3 ro, rd;
  if (P.projection == PTC_PROJ_ORTHOGRAPHIC) {
    const float ox = (2.0f * fx - 1.0f) * P.xmag, oy = (2.0f * fy - 1.0f) * P.ymag;
    ro = vfma(s, ox, vfma(u, oy, pos));
    rd = f;
  } else {
    float t = fx + 0.5f;
    t = t - __builtin_floorf(t);
    float sp, cp, st, ct;
    sincos2pi(t, sp, cp);
    sincos2pi(0.5f * fy, st, ct);
    const v3 X = s, Y = -u, Z = -f;
    ro = pos;
    rd = normalize3(vfma(X, st * cp, vfma(Y, ct, Z * (st * sp))));
  }
  o[0] = ro.x; o[1] = ro.y; o[2] = ro.z;
  d[0] = rd.x; d[1] = rd.y; d[2] = rd.z;
}

// The camera ray of (pixel, sample) of a w x h frame and the path's RNG key.
PT_HD void pt_proj_ray(const DevCamera& cam, const PtCamProj& P, int w, int h, uint32_t seed_hash, uint32_t pixel, uint32_t sample, float o[3], float d[3],
                       uint32_t& key_out) {
  const uint32_t px = pixel % (uint32_t)w, py = pixel / (uint32_t)w;
  const uint32_t key = path_key(seed_hash, pixel, sample);
  const float jx = rng_f(key, 0, 0), jy = rng_f(key, 0, 1);
  const float fx = ((float)px + jx) / (float)w, fy = ((float)py + jy) / (float)h;
  pt_proj_point(cam, P, fx, fy, o, d);
  key_out = key;
}

// The pixel-centre ray the guides are traced along: the jitter is (0.5, 0.5).
PT_HD void pt_proj_guide_ray(const DevCamera& cam, const PtCamProj& P, int w, int h, uint32_t pixel, float o[3], float d[3]) {
  const uint32_t px = pixel % (uint32_t)w, py = pixel / (uint32_t)w;
  const float fx = ((float)px + 0.5f) / (float)w, fy = ((float)py + 0.5f) / (float)h;
  pt_proj_point(cam, P, fx, fy, o, d);
}

// The pixel footprint of the denoiser's plane-distance weight (pt_denoise.hip): the world size of a pixel, at unit distance along the ray where it grows with
// the distance (`flat` = 0: PERSPECTIVE 2 tan(yfov / 2) / h, EQUIRECT pi / h), or at every depth (`flat` = 1: ORTHOGRAPHIC 2 ymag / h).
inline float pt_proj_footprint(const DevCamera& cam, const PtCamProj& P, int h, int& flat) {
  flat = P.projection == PTC_PROJ_ORTHOGRAPHIC ? 1 : 0;
  if (P.projection == PTC_PROJ_ORTHOGRAPHIC) return (2.0f * P.ymag) / (float)h;
  if (P.projection == PTC_PROJ_EQUIRECT) return PT_PI / (float)h;
  return (2.0f * cam.sy) / (float)h;
}

// ---- the kernels (pt_camera.hip) ----------------------------------------------------------------------------------------------------------
// k_raygen_proj: pt_launch_raygen's job (RASTER = false) under ORTHOGRAPHIC / EQUIRECT — the same path id -> (owned pixel, sample) mapping, the same queue record.
void pt_launch_raygen_proj(hipStream_t, const DevCamera&, const PtCamProj&, const DevFrame&, const DevQueues&, uint32_t first_sample, uint32_t n_samples);
// k_raygen_guides_proj: pt_launch_raygen_guides' job — the pixel-centre rays of the pixels [first_pixel, first_pixel + n) at the slots [0, n) of ray[0].
void pt_launch_raygen_guides_proj(hipStream_t, const DevCamera&, const PtCamProj&, int w, int h, uint32_t first_pixel, uint32_t n, const DevQueues&);
// k_guides_pos_proj: behind k_guides, which took the rays for perspective ones from cam.pos in this one field: pos_class.xyz = o + Z d of the projection's own ray.
void pt_launch_guides_pos_proj(hipStream_t, const DevCamera&, const PtCamProj&, int w, int h, uint32_t first_pixel, uint32_t n, const float4* normal_depth,
                               float4* pos_class);
