// pt_lens.h — the thin-lens camera: depth of field with a circular or a bladed aperture.
//
// The lens lives in ray generation alone: a lens sample changes the origin and the direction written into the first ray queue, and nothing behind it.
// pt_lens_point and pt_lens_ray below are the definition — IEEE binary32, no contraction (-ffp-contract=off), in the order written, pt_fma = one
// rounding; the host evaluation (ptc_debug_camera_rays on a description-only context, ptc_debug_lens_sample) and the kernel (pt_lens.hip) both call them, so
// the device writes the bytes the host computes.  tests/lens_reference.py restates them in numpy.
//
// path_key, rng_f, sincos2pi and pt_fma are pt_device.h's host + device functions, the ones k_raygen calls (tests/test_lens_host.py holds the host evaluation to
// the numpy restatement, tests/test_gpu_lens.py holds the rays to k_raygen's).
//
// RNG dimensions: bounce index 0 draws dimensions 0 and 1 (the pixel jitter); k_shade at bounce b draws from index b + 1, so the dimensions 2..7 of index 0
// are free.  The lens takes 2 and 3.
#pragma once
#include "../../include/ptc.h"
#include "ptc_internal.h"
#include "pt_device.h"

// The point (lx, ly) of the aperture that the pair (u1, u2) in [0,1)^2 selects, uniform over the aperture's area.
//   disk (blades = 0)   r = sqrt(u1), angle 2 pi u2.
//   n blades            the regular n-gon with circumradius R and a vertex at `rotation` turns: u1 picks the fan triangle k = min((int)(u1 n), n - 1) — centre,
//                       vertex k, vertex k + 1 — and its remainder a with u2 a uniform point of that triangle, (1 - sqrt a) centre + sqrt a ((1 - u2) V_k + u2 V_k+1).
PT_HD void pt_lens_point(const ptc_lens_params& L, float u1, float u2, float& lx, float& ly) {
  const float R = L.aperture_radius;
  if (L.blades == 0) {
    const float r = __builtin_sqrtf(u1);
    float sn, co; sincos2pi(u2, sn, co);
    const float rr = R * r;
    lx = rr * co; ly = rr * sn;
    return;
  }
  const int n = L.blades;
  const float x = u1 * (float)n;
  int k = (int)x;
  if (k > n - 1) k = n - 1;
  const float a = x - (float)k;
  const float su = __builtin_sqrtf(a);
  float t0 = L.rotation + (float)k / (float)n;
  t0 = t0 - __builtin_floorf(t0);
  float t1 = L.rotation + (float)(k + 1) / (float)n;
  t1 = t1 - __builtin_floorf(t1);
  float s0, c0, s1, c1;
  sincos2pi(t0, s0, c0);
  sincos2pi(t1, s1, c1);
  const float b0 = su * (1.0f - u2), b1 = su * u2;
  const float px = pt_fma(b1, c1, b0 * c0), py = pt_fma(b1, s1, b0 * s0);
  lx = R * px; ly = R * py;
}

// The camera ray of (pixel, sample) of a w x h frame: origin o, unit direction d, and the path's RNG key.  key, jitter, fx, fy, dvx, dvy are k_raygen's
// (pt_kernels.hip, RASTER = false).  R = 0 is the pinhole, k_raygen's ray restated; R > 0: the lens point l = (lx, ly) in the camera's (s, u) plane is the
// origin, and the ray goes through the point the pinhole ray meets at view depth F: o = pos + lx s + ly u, d = normalize((F dvx - lx) s + (F dvy - ly) u + F f).
PT_HD void pt_lens_ray(const DevCamera& cam, const ptc_lens_params& L, int w, int h, uint32_t seed_hash, uint32_t pixel, uint32_t sample,
                            float o[3], float d[3], uint32_t& key_out) {
  const uint32_t px = pixel % (uint32_t)w, py = pixel / (uint32_t)w;
  const uint32_t key = path_key(seed_hash, pixel, sample);
  const float jx = rng_f(key, 0, 0), jy = rng_f(key, 0, 1);
  const float fx = ((float)px + jx) / (float)w, fy = ((float)py + jy) / (float)h;
  const float dvx = (2.0f * fx - 1.0f) * cam.sx, dvy = (2.0f * fy - 1.0f) * cam.sy;
  float v[3];
  if (L.aperture_radius > 0.0f) {
    float lx, ly;
    pt_lens_point(L, rng_f(key, 0, 2), rng_f(key, 0, 3), lx, ly);
    const float F = L.focus_distance;
    const float qx = pt_fma(F, dvx, -lx), qy = pt_fma(F, dvy, -ly);
    for (int c = 0; c < 3; ++c) {
      o[c] = pt_fma(cam.s[c], lx, pt_fma(cam.u[c], ly, cam.pos[c]));
      v[c] = pt_fma(cam.s[c], qx, pt_fma(cam.u[c], qy, cam.f[c] * F));
    }
  } else {
    for (int c = 0; c < 3; ++c) {
      o[c] = cam.pos[c];
      v[c] = pt_fma(cam.s[c], dvx, pt_fma(cam.u[c], dvy, cam.f[c]));
    }
  }
  const float inv = 1.0f / __builtin_sqrtf(pt_fma(v[2], v[2], pt_fma(v[1], v[1], v[0] * v[0])));
  for (int c = 0; c < 3; ++c) d[c] = v[c] * inv;
  key_out = key;
}

// ---- the kernel (pt_lens.hip) -------------------------------------------------------------------------------------------------------------
// k_raygen_lens: pt_launch_raygen's job (RASTER = false) for a lens with R > 0 — the same path id -> (owned pixel, sample) mapping, the same queue record.
void pt_launch_raygen_lens(hipStream_t, const DevCamera&, const ptc_lens_params&, const DevFrame&, const DevQueues&, uint32_t first_sample, uint32_t n_samples);
