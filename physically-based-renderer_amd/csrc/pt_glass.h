// pt_glass.h — dielectric transmission: glass and thin-walled glTF materials in the path integrator.
//
// A material has a transmission tau in [0, 1] (KHR_materials_transmission), an index of refraction (KHR_materials_ior) and is thin-walled (a pane: glTF's "no
// volume") or solid (KHR_materials_volume, with Beer attenuation sigma2 per unit of distance inside).  The trace kernels and k_shade know nothing of this.  A smooth
// dielectric interface is a delta event, so it is resolved in a pass of its own (pt_glass.hip: k_glass_filter) between k_trace_closest(b) — and the alpha
// resolution, when the scene has one — and k_shade(b): the pass follows a ray through its reflections and refractions and hands k_shade an ordinary hit or miss
// with the ray record rewritten.  A scene without a transmissive material never launches it.
//
// The BSDF this estimates is  p_t x (smooth tinted dielectric) + (1 - p_t) x (what k_shade shades),  p_t = tau x (1 - metallic).
//
// pt_glass_beer / pt_glass_event / pt_glass_interact below are the definition — IEEE binary32, no contraction, in the order written; the host evaluation
// (ptc_debug_glass_interact) and the kernel both call them.  tests/glass_reference.py restates them in numpy.
//
// A batch ray at bounce b has had j interface events so far, j = 0 at first.  While its hit record is a hit on a primitive whose material has tau > 0:
//  1 Surface   as k_shade rebuilds it (pt_shading.h): P, ng, ns after record_material (textures, normal map), base, metallic; wo = -d; front = orient_normals(wo, ng, ns).
//  2 Beer      a solid material, a back-face hit and a non-zero sigma2: T_c = T_c * pt_exp2(-(sigma2_c * t)), t the hit record's t — whether or not the hit then
//              stands; skipped altogether when all sigma2 are 0, so that T keeps its bits.
//  3 Choice    u_s = rng_f(key, PT_GLASS_RNG_BASE + (b + 1) * 64 + j, 0).  !(u_s < p_t): the hit STANDS and k_shade shades it as always.  Else j == max_interactions:
//              the ray is EXHAUSTED (counted): its hit record becomes the miss record (-1, -1, 0, 0) and T = 0, so the path ends in k_shade without a contribution.
//  4 Event     pt_glass_event with n = ns, u_e = rng_f(key, same index, 1).  Reflection must leave on ng's side (dot3(ng, d') > 0), transmission on the other
//              (dot3(ng, d') < 0); a d' that does not is discarded and the event evaluated again with n = ng (F and s2 anew from ng, the same u_e; total internal
//              reflection there reflects), and that result is taken as it is.  Reflect: o' = vfma(ng, ray_eps, P), T unchanged.  Transmit:
//              o' = vfma(ng, -ray_eps, P), T_c = T_c * base_c when thin or front (leaving a solid does not tint).  j = j + 1, and (o', d') is traced again by the
//              unchanged k_trace_closest (and resolved by the alpha pass, when the scene has one, with the bounce argument 0x01000000 + (b + 1) * 64 + r of round r).
// Results: a ray that never met a transmissive primitive keeps its ray and hit records bit for bit.  A ray with j >= 1 gets the standing hit at its own slot of
// q.hit — (t of the last segment, prim | class << 28, u, v), or the trace's miss record — and its own slot of ray[qi] becomes A = (o', d'.x), B = (d'.yz, T.xy),
// C = (T.z, PT_GLASS_DELTA_PDF, path, key).  A j = 0 ray whose T step 2 attenuated gets T rewritten in ray[qi] only.
// PT_GLASS_DELTA_PDF: its square is finite, and in k_shade's pb2 / fma(pl, pl, pb2) it gives the weight 1 for any realistic pl — the correct MIS weight, because
// next-event estimation cannot reach a light through a delta interface.  In a frame with transparent shadows (pt_glass_shadow.h) it can, through thin panes: there a
// ray all of whose events were thin transmissions keeps the pdf word, o and d of its source record instead, and its hit's t counts from the source origin.
//
// RNG: rng_f forms index * 8 + dim in uint32, so the pass draws at the counters 0x40000000 + ..: disjoint from k_shade (small), the punctual pass (0x80000000 + ..)
// and alpha.
//
// Limits.  No eta^2 radiance scaling; roughness is ignored for the interface.  Shadow rays (k_trace_any, alpha's shadow walk, the punctual pass) see a transmissive
// surface as an occluder unless ptc_set_glass_shadows lets them pass thin panes (pt_glass_shadow.h; solid glass bends light and stays an occluder): otherwise
// light reaches things behind glass only along sampled paths that hit an emitter or the environment.  ptc_frame_guides, the denoisers, the temporal reprojection and ptc_focus_distance_at_pixel see glass as the surface.  The raster
// integrators and the existing debug hooks ignore transmission.  Probe frames go through run_batch and honour it.  An emissive material and a material whose alpha
// mode is not OPAQUE are never transmissive.
#pragma once
#include "../../include/ptc.h"
#include "ptc_internal.h"
#include "pt_device.h"

#define PT_GLASS_RNG_BASE 0x08000000u
#define PT_GLASS_DELTA_PDF 1.0e18f
#define PT_GLASS_MAX_INTERACTIONS 32
#define PT_GLASS_DEFAULT_INTERACTIONS 8

enum { PT_GLASS_STANDS = 0, PT_GLASS_EXHAUSTED = 1, PT_GLASS_REFLECT = 2, PT_GLASS_TRANSMIT = 3 };

// what the pass reads of a material: 32 bytes
struct pt_glass_mat { float tau, ior; int thin; float pad0; float sigma2[3]; float pad1; };

// the stored attenuation coefficient of one channel: sigma2 = -log2(clamp(colour, 2^-20, 1)) / distance, 0 where there is none
PT_HD float pt_glass_sigma2(float color, float distance) {
  if (!(distance > 0.0f)) return 0.0f;
  const float c = fmin2(fmax2(color, 9.5367431640625e-7f), 1.0f);
  return -pt_log2(c) / distance;
}
inline pt_glass_mat pt_glass_make_mat(const ptc_transmission_params& p) {
  pt_glass_mat m{};
  m.tau = p.transmission; m.ior = p.ior; m.thin = p.thin_walled ? 1 : 0;
  for (int k = 0; k < 3; ++k) m.sigma2[k] = pt_glass_sigma2(p.attenuation_color[k], p.attenuation_distance);
  return m;
}

// step 2.  Returns whether T changed
PT_HD bool pt_glass_beer(const pt_glass_mat& m, bool front, float t, v3& T) {
  if (m.thin || front) return false;
  if (m.sigma2[0] == 0.0f && m.sigma2[1] == 0.0f && m.sigma2[2] == 0.0f) return false;
  T.x = T.x * pt_exp2(-(m.sigma2[0] * t)); T.y = T.y * pt_exp2(-(m.sigma2[1] * t)); T.z = T.z * pt_exp2(-(m.sigma2[2] * t));
  return true;
}

// one interface event about the normal n (on wo's side): the Fresnel reflectance F of the interface (a thin pane: of its two faces), the choice by u_e, the new direction
PT_HD bool pt_glass_event(v3 n, v3 d, v3 wo, float eta, bool thin, float u_e, v3& dn, float& F) {
  const float cos_i = fmin2(dot3(n, wo), 1.0f);
  const float s2 = eta * eta * (1.0f - cos_i * cos_i);
  float cos_t = 0.0f;
  if (s2 >= 1.0f) F = 1.0f;
  else {
    cos_t = pt_sqrt(1.0f - s2);
    const float rs = (eta * cos_i - cos_t) / (eta * cos_i + cos_t);
    const float rp = (cos_i - eta * cos_t) / (cos_i + eta * cos_t);
    F = 0.5f * (rs * rs + rp * rp);
  }
  if (thin) F = (2.0f * F) / (1.0f + F);
  const bool reflect = u_e < F;
  if (reflect) dn = vfma(n, 2.0f * cos_i, d);
  else if (thin) dn = d;
  else dn = normalize3(d * eta + n * (eta * cos_i - cos_t));
  return reflect;
}

// steps 3 and 4 for a hit whose surface is (P, ng, ns, front) as orient_normals left it.  o, d, T are updated by an event; F_out: the reflectance the event used
PT_HD int pt_glass_interact(const pt_glass_mat& m, v3 P, v3 ng, v3 ns, bool front, v3 base, float metallic, float ray_eps, float u_s, float u_e, uint32_t j, uint32_t max_interactions,
                            v3& o, v3& d, v3& T, float& F_out) {
  const float p_t = m.tau * (1.0f - metallic);
  F_out = 0.0f;
  if (!(u_s < p_t)) return PT_GLASS_STANDS;
  if (j == max_interactions) return PT_GLASS_EXHAUSTED;
  const v3 wo = -d;
  const bool thin = m.thin != 0;
  const float eta = (thin || front) ? 1.0f / m.ior : m.ior;
  v3 dn; float F;
  bool reflect = pt_glass_event(ns, d, wo, eta, thin, u_e, dn, F);
  const float side = dot3(ng, dn);
  if (reflect ? !(side > 0.0f) : !(side < 0.0f)) reflect = pt_glass_event(ng, d, wo, eta, thin, u_e, dn, F);
  F_out = F;
  d = dn;
  if (reflect) { o = vfma(ng, ray_eps, P); return PT_GLASS_REFLECT; }
  o = vfma(ng, -ray_eps, P);
  if (thin || front) { T.x = T.x * base.x; T.y = T.y * base.y; T.z = T.z * base.z; }
  return PT_GLASS_TRANSMIT;
}

// ---- the tables the pass reads --------------------------------------------------------------------------------------------------------------------
enum { PT_GLASS_REFLECTIONS = 0, PT_GLASS_REFRACTIONS, PT_GLASS_STANDING, PT_GLASS_EXHAUSTED_N, PT_GLASS_COUNTERS };
struct DevGlass {
  const uint32_t* bits;          // one bit per original primitive id, set when its material has tau > 0
  const float4* mats;            // two units per material: (tau, ior, thin as int bits, -) (sigma2.xyz, -)
  uint32_t max_interactions;     // 1 .. PT_GLASS_MAX_INTERACTIONS
  unsigned long long* counters;  // [PT_GLASS_COUNTERS]: a wave adds its totals once, when it ends
};

// host: the two tables from the per-primitive material ids (HostBuilt::tri_mat; primitive ids survive refit and rebuild, so the tables do).  params may be shorter
// than the material list: the rest is not transmissive.  Returns the number of primitives with a bit set.
inline uint32_t pt_glass_tables(const std::vector<int32_t>& tri_mat, size_t n_mats, const std::vector<ptc_transmission_params>& params, std::vector<uint32_t>& bits,
                                std::vector<pt_glass_mat>& mats) {
  bits.assign((tri_mat.size() + 31u) / 32u, 0u);
  mats.assign(n_mats, pt_glass_mat{0.0f, 1.5f, 1, 0.0f, {0.0f, 0.0f, 0.0f}, 0.0f});
  for (size_t m = 0; m < n_mats && m < params.size(); ++m) mats[m] = pt_glass_make_mat(params[m]);
  uint32_t n = 0;
  for (size_t p = 0; p < tri_mat.size(); ++p) {
    const int32_t m = tri_mat[p];
    if (m >= 0 && (size_t)m < n_mats && mats[(size_t)m].tau > 0.0f) { bits[p >> 5] |= 1u << (p & 31u); ++n; }
  }
  return n;
}

// ---- the kernel (pt_glass.hip) ---------------------------------------------------------------------------------------------------------------------
// `gq` is the lane's glass queue as a DevQueues view (ray[0] = the continuation records, hit, cnt, seg_ray[0], pre_ray of its own; seg_sh all zero): the unchanged
// pt_launch_scan, pt_launch_trace_closest and the alpha resolution take it as they take the batch's queues.  A continuation record keeps the batch ray's layout:
// A = (o', d'.x), B = (d'.yz, T.xy), C = (T.z, j, source slot, key).
// first = true: the batch's rays ray[qi] and their hit records -> the rays with an event, compacted to the front of each segment of gq.
// first = false: gq's records and THEIR hit records -> standing results scattered to the source slots of q.hit and q.ray[qi], the rays with an event compacted in place.
// shadows: the frame's shadow records pass thin panes (pt_glass_shadow.h), so a ray that only went straight through thin panes keeps its pdf word, o and d.
// j_out (or null): per source slot, the events of a ray whose result was written (debug hook).
void pt_launch_glass_filter(hipStream_t, const DevScene&, const DevQueues& q, const DevQueues& gq, int qi, uint32_t bounce, const DevGlass&, bool first, bool shadows, uint32_t* j_out);
