// pt_probes.h — light probes: path-traced radiance arriving at a point from every direction, projected onto real spherical harmonics up to band 2.
//
// A probe frame is a frame of the path integrator whose "pixels" are the probes: it has a ray generator of its own (uniform directions over the sphere from
// the probe's position) and, beside k_accumulate, an accumulator of its own (the SH projection of every path's radiance); nothing between the two knows that a
// path did not come from a camera.  The functions below are the definition — IEEE binary32, no contraction (-ffp-contract=off), in the order written,
// pt_fma = one rounding; the host evaluation (ptc_debug_probe_rays / ptc_debug_probe_project on a description-only context, ptc_sh9_*) and the kernels
// (pt_probes.hip) both call them, so the device computes the bytes the host computes.  tests/probes_reference.py restates them in numpy.
//
// path_key, rng_f and sincos2pi are pt_device.h's host + device functions.
//
// RNG dimensions: a probe has no pixel, so the jitter dimensions 0 and 1 of the path's RNG index 0 are free; the direction takes them.  k_shade at bounce b
// draws from index b + 1, as for a camera path.  The key of probe j, sample s is path_key(seed_hash, base + j, s): `base` shifts the index, so that shards of
// one probe set ([0, 40) with base 0 and [40, 65) with base 40) draw what the whole set draws.
#pragma once
#include "ptc_internal.h"
#include "pt_device.h"

#define PT_SH9 9                      // coefficients per colour channel
#define PT_SH9_FLOATS 27              // per probe, laid out [k][rgb]
#define PT_PROBE_FOUR_PI 12.566371f

// The ray of (probe index `idx` = base + j, sample): unit direction d, uniform over the sphere, and the path's RNG key.  The origin is the probe's position.
PT_HD void pt_probe_dir(uint32_t seed_hash, uint32_t idx, uint32_t sample, float d[3], uint32_t& key_out) {
  const uint32_t key = path_key(seed_hash, idx, sample);
  const float u1 = rng_f(key, 0, 0), u2 = rng_f(key, 0, 1);
  const float z = pt_fma(-2.0f, u1, 1.0f);
  const float r = __builtin_sqrtf(__builtin_fmaxf(pt_fma(-z, z, 1.0f), 0.0f));
  float sn, co; sincos2pi(u2, sn, co);
  const float vx = r * co, vy = r * sn, vz = z;
  const float inv = 1.0f / __builtin_sqrtf(pt_fma(vz, vz, pt_fma(vy, vy, vx * vx)));      // the camera ray's normalisation
  d[0] = vx * inv; d[1] = vy * inv; d[2] = vz * inv;
  key_out = key;
}

// Real SH basis function k of 0..8 at the unit direction (x, y, z): world axes, no Condon-Shortley sign.  k: 0 | y z x | xy yz (3z^2-1) xz (x^2-y^2).
PT_HD float pt_sh9_basis(int k, float x, float y, float z) {
  switch (k) {
    case 0: return 0.2820948f;
    case 1: return 0.4886025f * y;
    case 2: return 0.4886025f * z;
    case 3: return 0.4886025f * x;
    case 4: return 1.0925484f * (x * y);
    case 5: return 1.0925484f * (y * z);
    case 6: return pt_fma(0.9461747f, z * z, -0.3153916f);
    case 7: return 1.0925484f * (x * z);
    default: return 0.5462742f * (x * x - y * y);
  }
}

// resolve: coef = acc * (4 pi / N), N the samples accumulated (or the resolve divisor of a sample-range shard)
PT_HD float pt_sh9_resolve_scale(uint32_t n_samples) { return PT_PROBE_FOUR_PI / (float)n_samples; }

// Radiance from the unit direction dir: out_c = sum_k sh[k][c] b_k(dir), k ascending, product then sum.
PT_HD void pt_sh9_eval(const float sh[PT_SH9_FLOATS], const float dir[3], float out[3]) {
  float o[3] = {0.0f, 0.0f, 0.0f};
  for (int k = 0; k < PT_SH9; ++k) {
    const float b = pt_sh9_basis(k, dir[0], dir[1], dir[2]);
    for (int c = 0; c < 3; ++c) o[c] = o[c] + sh[k * 3 + c] * b;
  }
  for (int c = 0; c < 3; ++c) out[c] = o[c];
}

// Irradiance on a surface with the unit normal n: the radiance convolved with the clamped cosine (Ramamoorthi-Hanrahan), E = sum A_l coef_lm Y_lm(n) with
// A_0 = pi, A_1 = 2 pi / 3, A_2 = pi / 4: out_c = sum_k (A_k sh[k][c]) b_k(n), k ascending.
PT_HD void pt_sh9_irradiance(const float sh[PT_SH9_FLOATS], const float n[3], float out[3]) {
  float o[3] = {0.0f, 0.0f, 0.0f};
  for (int k = 0; k < PT_SH9; ++k) {
    const float A = k == 0 ? 3.1415927f : k < 4 ? 2.0943952f : 0.7853982f;
    const float b = pt_sh9_basis(k, n[0], n[1], n[2]);
    for (int c = 0; c < 3; ++c) o[c] = o[c] + (A * sh[k * 3 + c]) * b;
  }
  for (int c = 0; c < 3; ++c) out[c] = o[c];
}

// ---- the kernels (pt_probes.hip) ----------------------------------------------------------------------------------------------------------
// k_raygen_probe: pt_launch_raygen's job for a probe frame — path p is probe j = p % n_probes, sample first_sample + p / n_probes; k_raygen's queue record.
// positions: one float4 (x, y, z, -) per probe.
void pt_launch_raygen_probe(hipStream_t, const float4* positions, uint32_t n_probes, uint32_t index_base, uint32_t seed_hash, const DevQueues&, uint32_t first_sample,
                            uint32_t n_samples);
// k_accumulate_sh: acc[j][k][c] += lpath[s n + j].c * b_k(d(base + j, first_sample + s)) for s = 0 .. n_samples - 1 in that order; acc holds 27 n_probes floats.
void pt_launch_accumulate_sh(hipStream_t, uint32_t n_probes, uint32_t index_base, uint32_t seed_hash, const float4* lpath, float* acc, uint32_t first_sample, uint32_t n_samples);
