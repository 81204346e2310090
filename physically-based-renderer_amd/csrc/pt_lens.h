// pt_lens.h — the thin-lens camera: depth of field with a circular or a bladed aperture.
//
// The lens lives in ray generation alone: a lens sample changes the origin and the direction written into the first ray queue, and nothing behind it.
// pt_lens_point and pt_lens_ray below are the definition — IEEE binary32, no contraction (-ffp-contract=off), in the order written, pt_lens_fma = one
// rounding; the host evaluation (ptc_debug_camera_rays on a description-only context, ptc_debug_lens_sample) and the kernel (pt_lens.hip) both call them, so
// the device writes the bytes the host computes.  tests/lens_reference.py restates them in numpy.
//
// pt_device.h is device-only, so the four functions of it that a camera ray needs — pcg, path_key, rng_f, sincos2pi — are restated here in host + device
// form, operation for operation (tests/test_lens_host.py holds them to the numpy restatement, tests/test_gpu_lens.py holds the rays to k_raygen's).
//
// RNG dimensions: bounce index 0 draws dimensions 0 and 1 (the pixel jitter); k_shade at bounce b draws from index b + 1, so the dimensions 2..7 of index 0
// are free.  The lens takes 2 and 3.
#pragma once
#include "../../include/ptc.h"
#include "ptc_internal.h"

#define PT_LENS_HD __host__ __device__ inline

PT_LENS_HD float pt_lens_fma(float a, float b, float c) { return __builtin_fmaf(a, b, c); }
PT_LENS_HD uint32_t pt_lens_pcg(uint32_t v) {
  uint32_t s = v * 747796405u + 2891336453u;
  uint32_t w = ((s >> ((s >> 28) + 4u)) ^ s) * 277803737u;
  return (w >> 22) ^ w;
}
PT_LENS_HD uint32_t pt_lens_path_key(uint32_t seed_hash, uint32_t pixel, uint32_t sample) { return pt_lens_pcg(pixel + pt_lens_pcg(sample + seed_hash)); }
PT_LENS_HD float pt_lens_rng_f(uint32_t key, uint32_t bounce, uint32_t dim) {
  uint32_t x = pt_lens_pcg(pt_lens_pcg(bounce * 8u + dim) ^ key);
  return (float)(x >> 8) * (1.0f / 16777216.0f);
}
// sin(2 pi u), cos(2 pi u), u in [0,1): quadrant + octant reduction, Taylor on [0, pi/4] (pt_device.h: sincos2pi)
PT_LENS_HD void pt_lens_sincos2pi(float u, float& so, float& co) {
  float x4 = u * 4.0f;
  int q = (int)x4;
  if (q > 3) q = 3;
  float r = x4 - (float)q;
  bool swap = r > 0.5f;
  float rr = swap ? 1.0f - r : r;
  float x = rr * 1.57079632679489661923f;
  float x2 = x * x;
  float ps = pt_lens_fma(x2, pt_lens_fma(x2, pt_lens_fma(x2, pt_lens_fma(x2, 2.7557319e-6f, -1.9841270e-4f), 8.3333333e-3f), -1.6666667e-1f), 1.0f);
  float s = x * ps;
  float c = pt_lens_fma(x2, pt_lens_fma(x2, pt_lens_fma(x2, pt_lens_fma(x2, 2.4801587e-5f, -1.3888889e-3f), 4.1666667e-2f), -0.5f), 1.0f);
  if (swap) { float t = s; s = c; c = t; }
  float S, C;
  if (q == 0) { S = s; C = c; }
  else if (q == 1) { S = c; C = -s; }
  else if (q == 2) { S = -s; C = -c; }
  else { S = -c; C = s; }
  so = S; co = C;
}

// The point (lx, ly) of the aperture that the pair (u1, u2) in [0,1)^2 selects, uniform over the aperture's area.
//   disk (blades = 0)   r = sqrt(u1), angle 2 pi u2.
//   n blades            the regular n-gon with circumradius R and a vertex at `rotation` turns: u1 picks the fan triangle k = min((int)(u1 n), n - 1) — centre,
//                       vertex k, vertex k + 1 — and its remainder a with u2 a uniform point of that triangle, (1 - sqrt a) centre + sqrt a ((1 - u2) V_k + u2 V_k+1).
PT_LENS_HD void pt_lens_point(const ptc_lens_params& L, float u1, float u2, float& lx, float& ly) {
  const float R = L.aperture_radius;
  if (L.blades == 0) {
    const float r = __builtin_sqrtf(u1);
    float sn, co; pt_lens_sincos2pi(u2, sn, co);
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
  pt_lens_sincos2pi(t0, s0, c0);
  pt_lens_sincos2pi(t1, s1, c1);
  const float b0 = su * (1.0f - u2), b1 = su * u2;
  const float px = pt_lens_fma(b1, c1, b0 * c0), py = pt_lens_fma(b1, s1, b0 * s0);
  lx = R * px; ly = R * py;
}

// The camera ray of (pixel, sample) of a w x h frame: origin o, unit direction d, and the path's RNG key.  key, jitter, fx, fy, dvx, dvy are k_raygen's
// (pt_kernels.hip, RASTER = false).  R = 0 is the pinhole, k_raygen's ray restated; R > 0: the lens point l = (lx, ly) in the camera's (s, u) plane is the
// origin, and the ray goes through the point the pinhole ray meets at view depth F: o = pos + lx s + ly u, d = normalize((F dvx - lx) s + (F dvy - ly) u + F f).
PT_LENS_HD void pt_lens_ray(const DevCamera& cam, const ptc_lens_params& L, int w, int h, uint32_t seed_hash, uint32_t pixel, uint32_t sample,
                            float o[3], float d[3], uint32_t& key_out) {
  const uint32_t px = pixel % (uint32_t)w, py = pixel / (uint32_t)w;
  const uint32_t key = pt_lens_path_key(seed_hash, pixel, sample);
  const float jx = pt_lens_rng_f(key, 0, 0), jy = pt_lens_rng_f(key, 0, 1);
  const float fx = ((float)px + jx) / (float)w, fy = ((float)py + jy) / (float)h;
  const float dvx = (2.0f * fx - 1.0f) * cam.sx, dvy = (2.0f * fy - 1.0f) * cam.sy;
  float v[3];
  if (L.aperture_radius > 0.0f) {
    float lx, ly;
    pt_lens_point(L, pt_lens_rng_f(key, 0, 2), pt_lens_rng_f(key, 0, 3), lx, ly);
    const float F = L.focus_distance;
    const float qx = pt_lens_fma(F, dvx, -lx), qy = pt_lens_fma(F, dvy, -ly);
    for (int c = 0; c < 3; ++c) {
      o[c] = pt_lens_fma(cam.s[c], lx, pt_lens_fma(cam.u[c], ly, cam.pos[c]));
      v[c] = pt_lens_fma(cam.s[c], qx, pt_lens_fma(cam.u[c], qy, cam.f[c] * F));
    }
  } else {
    for (int c = 0; c < 3; ++c) {
      o[c] = cam.pos[c];
      v[c] = pt_lens_fma(cam.s[c], dvx, pt_lens_fma(cam.u[c], dvy, cam.f[c]));
    }
  }
  const float inv = 1.0f / __builtin_sqrtf(pt_lens_fma(v[2], v[2], pt_lens_fma(v[1], v[1], v[0] * v[0])));
  for (int c = 0; c < 3; ++c) d[c] = v[c] * inv;
  key_out = key;
}

// ---- the kernel (pt_lens.hip) -------------------------------------------------------------------------------------------------------------
// k_raygen_lens: pt_launch_raygen's job (RASTER = false) for a lens with R > 0 — the same path id -> (owned pixel, sample) mapping, the same queue record.
void pt_launch_raygen_lens(hipStream_t, const DevCamera&, const ptc_lens_params&, const DevFrame&, const DevQueues&, uint32_t first_sample, uint32_t n_samples);
