// pt_medium.h — a homogeneous participating medium inside an axis-aligned box (include/ptc_medium.h).
//
// The path integrator has surfaces only; this is the pass that puts a medium on the segments between them.  It runs between k_trace_closest(b) and k_shade(b)
// (pt_medium.hip: k_medium_decide) and behind k_shade(b) and k_shade_punctual(b) (k_medium_append<0>, <1>); a frame without a medium launches none of it.
// The functions below are the definition — IEEE binary32, no contraction (-ffp-contract=off), in the order written, pt_fma = one rounding, / and pt_sqrt correctly
// rounded, no libm; the kernels and the host evaluation (ptc_debug_medium_sample) call this one text.  tests/medium_reference.py restates it in numpy.
//
//  1 Span         pt_medium_span: the slab test of (o, d) against the box, per axis n = (lo - o) / d, f = (hi - o) / d (swapped so that n <= f), an axis with d == +-0
//                 decided by lo <= o <= hi alone; t0 = max(0, nearest), t1 = min(t_end, farthest); t_end is the hit record's t, PT_T_INF for a miss, tmax for a
//                 shadow record.  Empty unless t0 < t1; a ray with an empty span is untouched.
//  2 Free flight  u0 = rng_f(key, PT_MEDIUM_RNG_BASE + b + 1, 0);  s = t0 - pt_log2(1 - u0) * (ln 2 / sigma_t).  !(s < t1): the surface (or the miss) STANDS and
//                 nothing is written — with one extinction for all channels such a ray has weight transmittance / probability = 1.  Else a SCATTER EVENT at
//                 P = vfma(d, s, o) with T' = T * albedo.
//  3 The ray      of a scatter event leaves k_shade alone: its hit record becomes the miss record (-1, -1, 0, 0) and its T in ray[qi] becomes 0 — an exhausted glass
//                 ray's rule — so k_shade(b), unchanged, adds nothing for it and writes no record.  A scatter event with max(T') == 0 ends there.
//  4 Phase        ph(c) = (1 - g^2) / (4 pi x sqrt(x)), x = 1 + g^2 - 2 g c, c = dot3(d, wi) (pt_hg_phase).  pt_hg_cos inverts the cdf from u1 (|g| < 1e-3:
//                 c = 1 - 2 u1), clamped to [-1, 1]; the azimuth is sincos2pi(u2) in onb(d).  The continuation's pdf word is pt_hg_phase at the sampled c, its
//                 throughput T' (value / pdf = 1), its origin P itself: no surface, no epsilon.  Russian roulette is k_shade's P8 from the same bounce index,
//                 u = rng_f(.., 3).  Layout k_shade's: A = (P, wi.x) B = (wi.yz, T.xy) C = (T.z, pdf, path, key).  At b == max_bounces the ray simply ends.
//  5 NEE at P     k_shade's conventions, so that k_shade(b + 1)'s unchanged MIS weights are the complement: the light kind by p_env / p_area (u = rng_f(.., 4)),
//                 emitters by cdf_search (u = rng_f(.., 5)) and the sqrt(r1) mapping (r1, r2 = rng_f(.., 6), rng_f(.., 7)), pl = ((pmf dist^2) / (A cosl)) p_area with
//                 dist from P, wgt = pl^2 / fma(ph, ph, pl^2), contrib = T' Le ((ph wgt) / pl); the segment runs from P to the point minus its last 0.1 %.  The
//                 environment likewise with (r1, r2), pl = pe p_env, tmax = PT_T_INF.  Punctual lights, when the frame has any: one light by the table's cdf
//                 (u = rng_f(key, PT_MEDIUM_RNG_PUNCTUAL + b + 1, 0)), pt_light_sample(light, P), contrib = T' Li (ph / pmf), no MIS, §2b's segment from P.
//  6 Attenuation  of EVERY shadow record of a bounce, surface-born and medium-born: the span of (o, dir, tmax); a non-empty one multiplies the contribution by
//                 pt_exp2(-(sigma_t log2 e) (t1 - t0)) in place, before any shadow resolution reads the record; an empty one keeps the record's bits.
//
// RNG.  rng_f hashes the word index * 8 + dim in uint32.  k_shade's words are 8 (b + 1) + dim (alpha's PT_ALPHA_RNG_BASE * 8 wraps to the same small words), the
// glass pass's 0x40000000 + 512 (b + 1) + 8 j + dim, the punctual pass's 0x80000000 + 8 (b + 1) + dim.  The medium takes 0xC0000000 + 8 (b + 1) + dim and, for its
// punctual choice, 0xE0000000 + 8 (b + 1): for every bounce below 2^20 — the hooks' limit — each family stays inside the words between its start and the next family's (2^30 for glass, 2^29 for the rest).
#pragma once
#include "../../include/ptc.h"
#include "ptc_internal.h"
#include "pt_device.h"
#include "pt_lights.h"
#include "pt_alpha.h"
#include "pt_glass.h"

#define PT_MEDIUM_RNG_BASE 0x18000000u
#define PT_MEDIUM_RNG_PUNCTUAL 0x1c000000u
#define PT_MEDIUM_BOUNCE_LIMIT (1u << 20)
static_assert(PT_MEDIUM_RNG_BASE * 8u == 0xC0000000u && PT_MEDIUM_RNG_PUNCTUAL * 8u == 0xE0000000u && PT_LIGHTS_RNG_BASE * 8u == 0x80000000u &&
              PT_GLASS_RNG_BASE * 8u == 0x40000000u && PT_ALPHA_RNG_BASE * 8u == 0u,
              "the words each pass hashes start 2^29 or more apart");
static_assert((PT_MEDIUM_BOUNCE_LIMIT + 1u) * 512u + 8u * 64u <= 0x40000000u && (PT_MEDIUM_BOUNCE_LIMIT + 2u) * 8u <= 0x20000000u,
              "below the bounce limit the glass family (512 words per bounce) stays inside its 2^30 words, every other family (8 per bounce) inside 2^29");

#define PT_MEDIUM_G_MAX 0.99f
#define PT_MEDIUM_G_ISO 1e-3f
#define PT_LN2 0.693147180559945309f
#define PT_LOG2E 1.44269504088896341f
#define PT_4PI 12.5663706143591730f

enum { PT_MEDIUM_CROSSED = 0, PT_MEDIUM_SCATTERED, PT_MEDIUM_ATTENUATED, PT_MEDIUM_COUNTERS };

// the medium as the kernels read it
struct pt_medium {
  float lo[3], hi[3];
  float sigma_t;
  float ff;              // ln 2 / sigma_t
  float sl;              // sigma_t * log2 e
  float albedo[3];
  float g;
};

inline const char* pt_medium_params_error(const ptc_medium_params& p) {
  auto fin = [](float v) { return v - v == 0.0f; };
  for (int k = 0; k < 3; ++k) {
    if (!fin(p.box_lo[k]) || !fin(p.box_hi[k])) return "non-finite box";
    if (!(p.box_lo[k] < p.box_hi[k])) return "box_lo is not below box_hi on every axis";
    if (!(p.albedo[k] >= 0.0f && p.albedo[k] <= 1.0f)) return "albedo is not in [0, 1]";
  }
  if (!fin(p.sigma_t) || !(p.sigma_t >= 0.0f)) return "sigma_t is not finite and >= 0";
  if (!(p.g >= -PT_MEDIUM_G_MAX && p.g <= PT_MEDIUM_G_MAX)) return "|g| is not a number <= 0.99";
  return nullptr;
}
inline pt_medium pt_medium_make(const ptc_medium_params& p) {
  pt_medium m{};
  for (int k = 0; k < 3; ++k) { m.lo[k] = p.box_lo[k]; m.hi[k] = p.box_hi[k]; m.albedo[k] = p.albedo[k]; }
  m.sigma_t = p.sigma_t;
  m.ff = PT_LN2 / p.sigma_t;
  m.sl = p.sigma_t * PT_LOG2E;
  m.g = p.g;
  return m;
}

// ---- 1 ----
PT_HD bool pt_medium_axis(float lo, float hi, float o, float d, float& tn, float& tf) {
  if (d == 0.0f) return o >= lo && o <= hi;
  const float a = (lo - o) / d, b = (hi - o) / d;
  const float n = fmin2(a, b), f = fmax2(a, b);
  tn = fmax2(tn, n);
  tf = fmin2(tf, f);
  return true;
}
PT_HD bool pt_medium_span(const pt_medium& m, v3 o, v3 d, float t_end, float& t0, float& t1) {
  float tn = 0.0f, tf = t_end;
  t0 = t1 = 0.0f;
  if (!pt_medium_axis(m.lo[0], m.hi[0], o.x, d.x, tn, tf)) return false;
  if (!pt_medium_axis(m.lo[1], m.hi[1], o.y, d.y, tn, tf)) return false;
  if (!pt_medium_axis(m.lo[2], m.hi[2], o.z, d.z, tn, tf)) return false;
  t0 = tn; t1 = tf;
  return t0 < t1;
}
// ---- 2 ----
PT_HD float pt_medium_free_flight(const pt_medium& m, float t0, float u0) {
  const float l = pt_log2(1.0f - u0);
  const float w = l * m.ff;
  return t0 - w;
}
// ---- 4 ----
PT_HD float pt_hg_phase(float g, float c) {
  const float g2 = g * g;
  const float x = (1.0f + g2) - ((2.0f * g) * c);
  const float den = (PT_4PI * x) * pt_sqrt(x);
  return (1.0f - g2) / den;
}
PT_HD float pt_hg_cos(float g, float u1) {
  float c;
  if (__builtin_fabsf(g) < PT_MEDIUM_G_ISO) c = 1.0f - 2.0f * u1;
  else {
    const float g2 = g * g;
    const float q = (1.0f - g2) / ((1.0f - g) + ((2.0f * g) * u1));
    c = ((1.0f + g2) - q * q) / (2.0f * g);
  }
  return fmin2(fmax2(c, -1.0f), 1.0f);
}
// pt_device.h's onb (Duff et al. 2017), host and device: the same text
PT_HD void pt_medium_onb(v3 n, v3& t, v3& b) {
  float sg = __builtin_copysignf(1.0f, n.z);
  float a = -1.0f / (sg + n.z);
  float bb = n.x * n.y * a;
  t = V3(pt_fma(sg * n.x, n.x * a, 1.0f), sg * bb, -sg * n.x);
  b = V3(bb, pt_fma(n.y, n.y * a, sg), -n.y);
}
PT_HD v3 pt_hg_direction(v3 d, float c, float u2) {
  const float sn = pt_sqrt(fmax2(0.0f, 1.0f - c * c));
  float sp, cp;
  sincos2pi(u2, sp, cp);
  v3 tx, ty;
  pt_medium_onb(d, tx, ty);
  return vfma(tx, sn * cp, vfma(ty, sn * sp, d * c));
}
// P8 on T' (k_shade's rule): false, the path ends
PT_HD bool pt_medium_roulette(uint32_t rb, float ur, v3& T) {
  if (rb < PT_RR_START) return true;
  const float qq = max3c(T);
  if (!(qq > 0.0f)) return false;
  const float pr = fmin2(fmax2(qq, PT_RR_PMIN), 1.0f);
  if (ur >= pr) return false;
  pt_div3(T.x, T.y, T.z, pr);
  return true;
}
// ---- 6 ----
PT_HD float pt_medium_transmittance(const pt_medium& m, float t0, float t1) { return pt_exp2(-m.sl * (t1 - t0)); }

// ---- the kernels (pt_medium.hip) ---------------------------------------------------------------------------------------------------------------------
// The lane's medium queue: per segment of the batch's layout the parked continuation records, the parked emitter / environment shadow records and the parked
// punctual shadow records of its scatter events, each packed at the front of the segment's slots, and the three counts.
struct DevMediumQ {
  RayQ cont;
  ShadowQ sh, pl;
  uint32_t* n_cont; uint32_t* n_sh; uint32_t* n_pl;      // [PTC_MAX_SEGMENTS] each
  unsigned long long* counters;                         // PT_MEDIUM_COUNTERS
};
// k_medium_decide(b): between closest(b) and shade(b), over the live slots of ray[qi] and their hit records.  lights / cdf / n_punctual: the frame's punctual table (0: none)
void pt_launch_medium_decide(hipStream_t, const DevScene&, const DevQueues&, const DevMediumQ&, const pt_medium&, int qi, uint32_t bounce, uint32_t max_bounces,
                             const pt_light_rec* lights, const float* cdf, uint32_t n_punctual);
// k_medium_append<0>(b): behind shade(b), before the scan — the parked continuations behind ray[qi ^ 1]'s records, the parked emitter / environment shadow records behind
// seg_sh's, both counts raised, then every shadow record of the segment attenuated.  punctual: k_medium_append<1>(b), behind k_shade_punctual(b), before its scan — the same
// for the parked punctual records and the punctual pass's own
void pt_launch_medium_append(hipStream_t, const DevQueues&, const DevMediumQ&, const pt_medium&, int qi, bool punctual);
// the pass's own texts of k_shade's environment sampler and lookup (pt_medium.hip) on n items: out7 = (wi of (r1, r2), Le and pdf of dir_in) each; the scene has an environment
void pt_launch_medium_env(hipStream_t, const DevScene&, const float* r1, const float* r2, const float* dir_in, uint32_t n, float* out7);
