// pt_lights.h — punctual lights: point, spot and directional (glTF KHR_lights_punctual).
//
// A punctual light has no area: a BSDF sample can never hit it, so it is sampled by next-event estimation alone, without an MIS weight, and its term ADDS to
// what k_shade computes.  It is a pass of its own (pt_lights.hip: k_shade_punctual) behind k_shade's; a scene without such lights never launches it.
// pt_light_sample below is the definition — IEEE binary32, no contraction (-ffp-contract=off), in the order written, pt_fma = one rounding; the host
// evaluation (ptc_debug_light_sample) and the kernel both call it.  tests/lights_reference.py restates it in numpy.
//
// The cone of a spot is given by cosines, so nothing on the render path needs a trigonometric function.
//
// RNG: the light of a hit at bounce b is chosen by u = rng_f(key, PT_LIGHTS_RNG_BASE + b + 1, 0).  k_shade only ever uses the indices 0 .. max_bounces + 1, so
// nothing it draws changes.
//
// pt_fma, dot3, fmin2 / fmax2 and PT_T_INF are pt_device.h's; the pass rebuilds the surface with the helpers k_shade uses (pt_shading.h).
#pragma once
#include "../../include/ptc.h"
#include "ptc_internal.h"
#include "pt_device.h"

#define PT_LIGHTS_MAX 256u                  // hard cap: the table (16 KiB) and its cdf (1 KiB) always fit the kernel's LDS copies — one variant, no global fallback
#define PT_LIGHTS_RNG_BASE 0x10000000u

// one light as the kernel reads it: 64 bytes = 4 x float4
struct pt_light_rec {
  float pos[3]; int32_t type;        // PTC_LIGHT_*
  float dir[3]; float range;         // unit: the axis a spot points along / the way a directional light travels; range 0 = none
  float I[3]; float pmf;             // intensity (W/sr) or irradiance; probability of choosing this light
  float scale, offset;               // spot: s = clamp(fma(cd, scale, offset), 0, 1), scale = 1 / max(cos_inner - cos_outer, 0.001), offset = -cos_outer * scale
  float cos_inner, cos_outer;
};
static_assert(sizeof(pt_light_rec) == 64, "pt_light_rec is 64 bytes");

// The sample of light L seen from P: unit direction wi towards the light, the radiance Li arriving along it, the distance (PT_T_INF for a
// directional light).  false: no sample (P lies on the light).  Li may be 0 in every channel (outside the cone, beyond the range): the caller tests it.
PT_HD bool pt_light_sample(const pt_light_rec& L, v3 P, v3& wi, float& dist_out, v3& Li) {
  if (L.type == PTC_LIGHT_DIRECTIONAL) {
    wi = -V3(L.dir);
    Li = V3(L.I);
    dist_out = PT_T_INF;
    return true;
  }
  const v3 dv = V3(L.pos) - P;
  const float dist2 = dot3(dv, dv);
  if (!(dist2 > 0.0f)) return false;
  const float dist = pt_sqrt(dist2);
  const float inv = 1.0f / dist;
  wi = dv * inv;
  float att = 1.0f / dist2;
  if (L.range > 0.0f) {       // the window KHR_lights_punctual recommends
    const float q = dist2 / (L.range * L.range);
    const float w = fmin2(fmax2(1.0f - q * q, 0.0f), 1.0f);
    att = att * w;
  }
  if (L.type == PTC_LIGHT_SPOT) {
    const float cd = dot3(V3(L.dir), -wi);
    const float s = fmin2(fmax2(pt_fma(cd, L.scale, L.offset), 0.0f), 1.0f);
    att = att * (s * s);
  }
  Li = V3(L.I) * att;
  dist_out = dist;
  return true;
}

// ---- host: parameters -> records + cdf ----------------------------------------------------------------------------------------------------------
// nullptr when ptc_add_light would accept p
inline const char* pt_light_params_error(const ptc_light_params& p) {
  auto fin = [](float v) { return v - v == 0.0f; };
  if (p.type != PTC_LIGHT_POINT && p.type != PTC_LIGHT_SPOT && p.type != PTC_LIGHT_DIRECTIONAL) return "unknown light type";
  for (int k = 0; k < 3; ++k) if (!fin(p.position[k]) || !fin(p.direction[k]) || !fin(p.intensity[k])) return "non-finite position, direction or intensity";
  if (!fin(p.range) || !fin(p.cos_inner) || !fin(p.cos_outer)) return "non-finite range or cone cosine";
  for (int k = 0; k < 3; ++k) if (p.intensity[k] < 0.0f) return "negative intensity";
  if (p.range < 0.0f) return "negative range";
  if (p.type != PTC_LIGHT_POINT) {
    const float d2 = dot3(V3(p.direction), V3(p.direction));
    if (!(d2 > 0.0f) || !fin(1.0f / __builtin_sqrtf(d2))) return "zero direction";
  }
  if (p.type == PTC_LIGHT_SPOT && !(1.0f >= p.cos_inner && p.cos_inner > p.cos_outer && p.cos_outer >= -1.0f)) return "cone cosines out of order (1 >= cos_inner > cos_outer >= -1)";
  if (!(fin(p.sampling_weight) && p.sampling_weight > 0.0f)) return "sampling_weight is not finite and > 0";
  return nullptr;
}
// the direction normalised with normalize3's expression (a point light keeps what it was given)
inline void pt_light_normalise(ptc_light_params& p) {
  if (p.type == PTC_LIGHT_POINT) return;
  const float inv = 1.0f / __builtin_sqrtf(dot3(V3(p.direction), V3(p.direction)));
  for (int k = 0; k < 3; ++k) p.direction[k] = p.direction[k] * inv;
}
inline pt_light_rec pt_light_make_rec(const ptc_light_params& p, float pmf) {
  pt_light_rec r{};
  for (int k = 0; k < 3; ++k) { r.pos[k] = p.position[k]; r.dir[k] = p.direction[k]; r.I[k] = p.intensity[k]; }
  r.type = p.type; r.range = p.range; r.pmf = pmf;
  r.cos_inner = p.cos_inner; r.cos_outer = p.cos_outer;
  if (p.type == PTC_LIGHT_SPOT) {
    r.scale = 1.0f / fmax2(p.cos_inner - p.cos_outer, 0.001f);
    r.offset = -p.cos_outer * r.scale;
  }
  return r;
}
// the table as it is uploaded: pmf and cdf over sampling_weight as ptc_scene.cpp builds the emitter cdf (binary32 running sums, cdf[i] = run / total, last entry 1)
inline void pt_light_table(const std::vector<ptc_light_params>& lights, std::vector<pt_light_rec>& recs, std::vector<float>& cdf) {
  float total = 0.0f;
  for (const ptc_light_params& p : lights) total += p.sampling_weight;
  float run = 0.0f;
  recs.resize(lights.size()); cdf.resize(lights.size());
  for (size_t i = 0; i < lights.size(); ++i) {
    run += lights[i].sampling_weight;
    cdf[i] = run / total;
    recs[i] = pt_light_make_rec(lights[i], lights[i].sampling_weight / total);
  }
  if (!cdf.empty()) cdf.back() = 1.0f;
}

// ---- the kernel (pt_lights.hip) -----------------------------------------------------------------------------------------------------------------
// k_shade_punctual: the punctual next-event pass of bounce b over the rays of ray[qi] and their hit records, as k_shade(b) read them.  It writes shadow records to the
// front of each segment of q.shadow and their number to q.seg_sh; nothing else.  lights: n_lights (1 .. PT_LIGHTS_MAX) records, cdf: n_lights floats, both in device memory.
void pt_launch_shade_punctual(hipStream_t, const DevScene&, const DevQueues&, int qi, uint32_t bounce, const pt_light_rec* lights, const float* cdf, uint32_t n_lights);
