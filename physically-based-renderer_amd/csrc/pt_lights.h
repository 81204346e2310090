// pt_lights.h — punctual lights: point, spot and directional (glTF KHR_lights_punctual).
//
// A punctual light has no area: a BSDF sample can never hit it, so it is sampled by next-event estimation alone, without an MIS weight, and its term ADDS to
// what k_shade computes.  It is a pass of its own (pt_lights.hip: k_shade_punctual) behind k_shade's; a scene without such lights never launches it.
// pt_light_sample below is the definition — IEEE binary32, no contraction (-ffp-contract=off), in the order written, pt_lights_fma = one rounding; the host
// evaluation (ptc_debug_light_sample) and the kernel both call it.  tests/lights_reference.py restates it in numpy.
//
// The cone of a spot is given by cosines, so nothing on the render path needs a trigonometric function.
//
// RNG: the light of a hit at bounce b is chosen by u = rng_f(key, PT_LIGHTS_RNG_BASE + b + 1, 0).  k_shade only ever uses the indices 0 .. max_bounces + 1, so
// nothing it draws changes.
//
// pt_device.h is device-only and k_shade's surface reconstruction lives in pt_kernels.hip alone, so the second half of this file (PT_LIGHTS_DEVICE_PART, for
// pt_lights.hip, behind pt_device.h) restates what the pass needs of it operation for operation: the texture fetch over the plain texels / tex_info arrays
// (they hold the same texel values as the interleaved sets), apply_textures' arithmetic and the hit word's class shift.
#pragma once
#include "../../include/ptc.h"
#include "ptc_internal.h"

#define PT_LIGHTS_HD __host__ __device__ inline
#define PT_LIGHTS_MAX 256u                  // hard cap: the table (16 KiB) and its cdf (1 KiB) always fit the kernel's LDS copies — one variant, no global fallback
#define PT_LIGHTS_RNG_BASE 0x10000000u
#define PT_LIGHTS_T_INF 3.0e38f             // PT_T_INF
#define PT_LIGHTS_HIT_CLASS_SHIFT 28        // HIT_CLASS_SHIFT (pt_kernels.hip): the hit word is prim | class << 28

// one light as the kernel reads it: 64 bytes = 4 x float4
struct pt_light_rec {
  float pos[3]; int32_t type;        // PTC_LIGHT_*
  float dir[3]; float range;         // unit: the axis a spot points along / the way a directional light travels; range 0 = none
  float I[3]; float pmf;             // intensity (W/sr) or irradiance; probability of choosing this light
  float scale, offset;               // spot: s = clamp(fma(cd, scale, offset), 0, 1), scale = 1 / max(cos_inner - cos_outer, 0.001), offset = -cos_outer * scale
  float cos_inner, cos_outer;
};
static_assert(sizeof(pt_light_rec) == 64, "pt_light_rec is 64 bytes");

PT_LIGHTS_HD float pt_lights_fma(float a, float b, float c) { return __builtin_fmaf(a, b, c); }
PT_LIGHTS_HD float pt_lights_dot3(const float a[3], const float b[3]) { return pt_lights_fma(a[2], b[2], pt_lights_fma(a[1], b[1], a[0] * b[0])); }   // dot3
PT_LIGHTS_HD float pt_lights_min(float a, float b) { return a < b ? a : b; }      // fmin2
PT_LIGHTS_HD float pt_lights_max(float a, float b) { return a > b ? a : b; }      // fmax2

// The sample of light L seen from P: unit direction wi towards the light, the radiance Li arriving along it, the distance (PT_LIGHTS_T_INF for a
// directional light).  false: no sample (P lies on the light).  Li may be 0 in every channel (outside the cone, beyond the range): the caller tests it.
PT_LIGHTS_HD bool pt_light_sample(const pt_light_rec& L, const float P[3], float wi[3], float& dist_out, float Li[3]) {
  if (L.type == PTC_LIGHT_DIRECTIONAL) {
    wi[0] = -L.dir[0]; wi[1] = -L.dir[1]; wi[2] = -L.dir[2];
    Li[0] = L.I[0]; Li[1] = L.I[1]; Li[2] = L.I[2];
    dist_out = PT_LIGHTS_T_INF;
    return true;
  }
  const float dv[3] = {L.pos[0] - P[0], L.pos[1] - P[1], L.pos[2] - P[2]};
  const float dist2 = pt_lights_dot3(dv, dv);
  if (!(dist2 > 0.0f)) return false;
  const float dist = __builtin_sqrtf(dist2);
  const float inv = 1.0f / dist;
  wi[0] = dv[0] * inv; wi[1] = dv[1] * inv; wi[2] = dv[2] * inv;
  float att = 1.0f / dist2;
  if (L.range > 0.0f) {       // the window KHR_lights_punctual recommends
    const float q = dist2 / (L.range * L.range);
    const float w = pt_lights_min(pt_lights_max(1.0f - q * q, 0.0f), 1.0f);
    att = att * w;
  }
  if (L.type == PTC_LIGHT_SPOT) {
    const float mwi[3] = {-wi[0], -wi[1], -wi[2]};
    const float cd = pt_lights_dot3(L.dir, mwi);
    const float s = pt_lights_min(pt_lights_max(pt_lights_fma(cd, L.scale, L.offset), 0.0f), 1.0f);
    att = att * (s * s);
  }
  Li[0] = L.I[0] * att; Li[1] = L.I[1] * att; Li[2] = L.I[2] * att;
  dist_out = dist;
  return true;
}

// cdf_search's rule (pt_kernels.hip): the first index whose cdf entry exceeds r; the last entry is 1 > r
template <class P> PT_LIGHTS_HD uint32_t pt_lights_cdf_search(const P& cdf, uint32_t n, float r) {
  uint32_t lo = 0, hi = n - 1u;
  while (lo < hi) { const uint32_t mid = (lo + hi) >> 1; if (cdf[mid] > r) hi = mid; else lo = mid + 1u; }
  return lo;
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
    const float d2 = pt_lights_dot3(p.direction, p.direction);
    if (!(d2 > 0.0f) || !fin(1.0f / __builtin_sqrtf(d2))) return "zero direction";
  }
  if (p.type == PTC_LIGHT_SPOT && !(1.0f >= p.cos_inner && p.cos_inner > p.cos_outer && p.cos_outer >= -1.0f)) return "cone cosines out of order (1 >= cos_inner > cos_outer >= -1)";
  if (!(fin(p.sampling_weight) && p.sampling_weight > 0.0f)) return "sampling_weight is not finite and > 0";
  return nullptr;
}
// the direction normalised with normalize3's expression (a point light keeps what it was given)
inline void pt_light_normalise(ptc_light_params& p) {
  if (p.type == PTC_LIGHT_POINT) return;
  const float inv = 1.0f / __builtin_sqrtf(pt_lights_dot3(p.direction, p.direction));
  for (int k = 0; k < 3; ++k) p.direction[k] = p.direction[k] * inv;
}
inline pt_light_rec pt_light_make_rec(const ptc_light_params& p, float pmf) {
  pt_light_rec r{};
  for (int k = 0; k < 3; ++k) { r.pos[k] = p.position[k]; r.dir[k] = p.direction[k]; r.I[k] = p.intensity[k]; }
  r.type = p.type; r.range = p.range; r.pmf = pmf;
  r.cos_inner = p.cos_inner; r.cos_outer = p.cos_outer;
  if (p.type == PTC_LIGHT_SPOT) {
    r.scale = 1.0f / pt_lights_max(p.cos_inner - p.cos_outer, 0.001f);
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

#ifdef PT_LIGHTS_DEVICE_PART      // behind pt_device.h: restatements of pt_kernels.hip (texel_rgba, tex_fetch, apply_textures)
PT_DEV float4 pt_lights_texel_rgba(const DevScene& sc, size_t at) {
  const uint32_t p = sc.texels[at];
  return make_float4((float)(p & 255u) / 255.0f, (float)((p >> 8) & 255u) / 255.0f, (float)((p >> 16) & 255u) / 255.0f, (float)(p >> 24) / 255.0f);
}
PT_DEV float4 pt_lights_tex_fetch(const DevScene& sc, int tex, float u, float v) {
  const int4 ti = sc.tex_info[(size_t)tex];
  const float fu = u - __builtin_floorf(u), fv = v - __builtin_floorf(v);
  if (!sc.tex_linear) {
    int x = (int)(fu * (float)ti.y), y = (int)(fv * (float)ti.z);
    if (x > ti.y - 1) x = ti.y - 1;
    if (y > ti.z - 1) y = ti.z - 1;
    return pt_lights_texel_rgba(sc, (size_t)ti.x + (size_t)y * (size_t)ti.y + (size_t)x);
  }
  // PTC_FILTER_LINEAR: texel centres at i + 0.5, REPEAT wrap, lerp(a, b, t) = fma(t, b - a, a), x then y
  const float x = pt_fma(fu, (float)ti.y, -0.5f), y = pt_fma(fv, (float)ti.z, -0.5f);
  const float x0f = __builtin_floorf(x), y0f = __builtin_floorf(y);
  const float tx = x - x0f, ty = y - y0f;
  int x0 = (int)x0f, y0 = (int)y0f;
  int x1 = x0 + 1, y1 = y0 + 1;
  if (x0 < 0) x0 += ti.y;
  if (y0 < 0) y0 += ti.z;
  if (x1 > ti.y - 1) x1 -= ti.y;
  if (y1 > ti.z - 1) y1 -= ti.z;
  const size_t r0 = (size_t)ti.x + (size_t)y0 * (size_t)ti.y, r1 = (size_t)ti.x + (size_t)y1 * (size_t)ti.y;
  const float4 c00 = pt_lights_texel_rgba(sc, r0 + (size_t)x0), c10 = pt_lights_texel_rgba(sc, r0 + (size_t)x1), c01 = pt_lights_texel_rgba(sc, r1 + (size_t)x0),
               c11 = pt_lights_texel_rgba(sc, r1 + (size_t)x1);
  const float ax = pt_fma(tx, c10.x - c00.x, c00.x), ay = pt_fma(tx, c10.y - c00.y, c00.y), az = pt_fma(tx, c10.z - c00.z, c00.z), aw = pt_fma(tx, c10.w - c00.w, c00.w);
  const float bx = pt_fma(tx, c11.x - c01.x, c01.x), by = pt_fma(tx, c11.y - c01.y, c01.y), bz = pt_fma(tx, c11.z - c01.z, c01.z), bw = pt_fma(tx, c11.w - c01.w, c01.w);
  return make_float4(pt_fma(ty, bx - ax, ax), pt_fma(ty, by - ay, ay), pt_fma(ty, bz - az, az), pt_fma(ty, bw - aw, aw));
}
// apply_textures: t0..t5 are the units 5..10 of the primitive's shading record (uv x3, world tangent x3, world bitangent x3), M2 = (base.a, tex_color, tex_normal, tex_mr)
PT_DEV void pt_lights_apply_textures(const DevScene& sc, float4 t0, float4 t1, float4 t2, float4 t3, float4 t4, float4 t5, float hu, float hv, float hw, float4 M2, v3 ni, float base[4],
                                     float& metallic, float& roughness, v3& ns) {
  const int tex_color = __float_as_int(M2.y), tex_normal = __float_as_int(M2.z), tex_mr = __float_as_int(M2.w);
  const float tu = pt_fma(t1.x, hv, pt_fma(t0.z, hu, t0.x * hw)), tv = pt_fma(t1.y, hv, pt_fma(t0.w, hu, t0.y * hw));
  float4 cc = make_float4(1, 1, 1, 1), cn = make_float4(0.5f, 0.5f, 1.0f, 1.0f), cm = make_float4(1, 1, 1, 1);
  if (tex_color >= 0) cc = pt_lights_tex_fetch(sc, tex_color, tu, tv);
  if (tex_mr >= 0) cm = pt_lights_tex_fetch(sc, tex_mr, tu, tv);
  if (tex_normal >= 0) cn = pt_lights_tex_fetch(sc, tex_normal, tu, tv);
  if (tex_color >= 0) { base[0] = base[0] * cc.x; base[1] = base[1] * cc.y; base[2] = base[2] * cc.z; base[3] = base[3] * cc.w; }
  if (tex_mr >= 0) { roughness = roughness * cm.y; metallic = metallic * cm.z; }
  if (tex_normal >= 0) {
    const float nx = 2.0f * cn.x - 1.0f, ny = 2.0f * cn.y - 1.0f, nz = 2.0f * cn.z - 1.0f;
    const v3 ti = V3(pt_fma(t3.x, hv, pt_fma(t2.y, hu, t1.z * hw)), pt_fma(t3.y, hv, pt_fma(t2.z, hu, t1.w * hw)), pt_fma(t3.z, hv, pt_fma(t2.w, hu, t2.x * hw)));
    const v3 bi = V3(pt_fma(t5.y, hv, pt_fma(t4.z, hu, t3.w * hw)), pt_fma(t5.z, hv, pt_fma(t4.w, hu, t4.x * hw)), pt_fma(t5.w, hv, pt_fma(t5.x, hu, t4.y * hw)));
    ns = normalize3(vfma(ti, nx, vfma(bi, ny, ni * nz)));
  }
}
#endif
