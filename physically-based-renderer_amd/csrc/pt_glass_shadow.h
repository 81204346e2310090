// pt_glass_shadow.h — transparent shadows: next-event light through thin-walled glass ("Transparent shadows").
//
// A thin-walled pane does not bend light, so a shadow ray passes it deterministically with the pane's expected transmittance: the probability with which steps
// 3 and 4 of pt_glass_interact transmit a ray of the same direction, times the tint a transmitted ray receives.  That is unbiased, and it is what alpha's BLEND
// attenuation (pt_alpha.h) does for coverage.  Off by default (ptc_set_glass_shadows); a frame with it off, or a scene without a thin transmissive primitive,
// launches what it always launched.
//
// pt_glass_shadow_transmit below is the definition — IEEE binary32, no contraction, in the order written; the host evaluation (ptc_debug_glass_shadow_transmit)
// and the kernel both call it.  tests/glass_shadow_reference.py restates it in numpy.
//
// The walk (pt_glass_shadow.hip: k_glass_filter_shadow), one for the alpha and the glass surfaces of a scene.  The shadow queue is first traced by k_trace_any in its
// flag-writing form.  A record flagged free adds its contribution as AnyRay::publish does.  A flagged record is walked through its occluders by the closest-hit
// kernel: Tr = (1, 1, 1), rem = tmax, k = 0; a miss or a hit with !(t < rem) ends the walk as visible; a hit on an alpha primitive multiplies every Tr_c by
// pt_alpha_transmit and goes on from alpha's onward point; a hit on a transmissive primitive multiplies Tr_c by W_c and goes on from vfma(ng, -ray_eps, P), ng on
// the ray's side; a hit on anything else: occluded; Tr == (0, 0, 0): occluded; k == L: occluded (exhaustion, counted); otherwise on with rem = rem - t, k = k + 1.
// L = max(max_interactions, max_layers when the scene has alpha materials) of the frame; alpha's own walk (pt_alpha.h: no transparent shadows) is the same walk
// without a glass table and with L = max_layers.  Visible: lpath[path].c = lpath[path].c + Tr_c * contrib.c, the products
// skipped when Tr == (1, 1, 1): an unobstructed record adds the bits it always added, and a record that met alpha surfaces only adds what alpha's own walk adds.
//
// MIS.  Next-event estimation now reaches a light through thin panes, so a BSDF-sampled ray whose events were ALL thin transmissions (it went straight on) is no
// delta path any more: k_glass_filter<.., true> (pt_glass.hip) leaves such a ray the pdf word, o and d of its source record, rewrites T, and gives it the standing
// hit with t measured from the source origin, t_out = dot3(o' - o_src, d) + t — k_shade converts the emitter's area pdf with the hit's t squared.  A ray with a
// reflection or a solid refraction keeps PT_GLASS_DELTA_PDF, the last segment's t and the rewritten o and d.
#pragma once
#include "pt_alpha.h"
#include "pt_glass.h"

// the thin two-face reflectance about n (on wo's side) and cos_i: pt_glass_event's arithmetic
PT_HD float pt_glass_thin_reflectance(v3 n, v3 wo, float eta, float& cos_i) {
  cos_i = fmin2(dot3(n, wo), 1.0f);
  const float s2 = eta * eta * (1.0f - cos_i * cos_i);
  float F;
  if (s2 >= 1.0f) F = 1.0f;
  else {
    const float cos_t = pt_sqrt(1.0f - s2);
    const float rs = (eta * cos_i - cos_t) / (eta * cos_i + cos_t);
    const float rp = (cos_i - eta * cos_t) / (cos_i + eta * cos_t);
    F = 0.5f * (rs * rs + rp * rp);
  }
  return (2.0f * F) / (1.0f + F);
}

// the RGB share W of a shadow ray's contribution that a hit on the material lets through: the surface (ng, ns) as orient_normals(-d, ..) left it.  F_t: the
// reflectance used.  0 for a solid material and for a ray that does not arrive against ng
PT_HD v3 pt_glass_shadow_transmit(const pt_glass_mat& m, v3 ng, v3 ns, v3 d, v3 base, float metallic, float& F_t) {
  F_t = 0.0f;
  if (m.thin == 0) return V3(0.0f, 0.0f, 0.0f);
  if (!(dot3(ng, d) < 0.0f)) return V3(0.0f, 0.0f, 0.0f);
  const float p_t = m.tau * (1.0f - metallic);
  const v3 wo = -d;
  const float eta = 1.0f / m.ior;
  float cos_i;
  F_t = pt_glass_thin_reflectance(ns, wo, eta, cos_i);
  const v3 d_r = vfma(ns, 2.0f * cos_i, d);
  if (!(dot3(ng, d_r) > 0.0f)) F_t = fmin2(F_t, pt_glass_thin_reflectance(ng, wo, eta, cos_i));
  const float s = p_t * (1.0f - F_t);
  return V3(s * base.x, s * base.y, s * base.z);
}

// counters of the walk, one 64-bit word each: a wave adds its totals once, when it ends
enum { PT_GLASS_SHADOW_WALKED = 0, PT_GLASS_SHADOW_PASSES, PT_GLASS_SHADOW_VISIBLE, PT_GLASS_SHADOW_EXHAUSTED, PT_GLASS_SHADOW_COUNTERS };

// where a walk counts: a frame with transparent shadows into the four words above, alpha's own walk (pt_alpha.h) into PT_ALPHA_SHADOW_WALKED / _PASSES and
// PT_ALPHA_EXHAUSTED of DevAlpha::counters, with no word for `visible` (null)
struct ShadowWalkCounters { unsigned long long *walked, *passes, *visible, *exhausted; };

// ---- the kernel (pt_glass_shadow.hip) ---------------------------------------------------------------------------------------------------------------
// `sq` is the lane's glass queue (pt_glass.h), or its alpha queue for alpha's own walk.  Continuation records: A = (o', d.x), B = (d.y, d.z, rem, source slot), C = (Tr.xyz, k).
// first = true: the shadow queue and k_trace_any's flags -> free records published, flagged ones to sq with Tr = 1, rem = tmax, k = 0.
// a later round: sq's records and their hit records -> visible ones published with Tr, occluded ones dropped, the rest compacted in place.
// al.bits == nullptr: the scene has no alpha material.  gl.bits == nullptr: alpha's own walk, every other hit is an opaque occluder.  max_rounds is L above.
// tr_out / layers_out (or null): per source slot, the RGB transmittance of a visible record INSTEAD of the addition to lpath, and the surfaces it passed (debug hook).
void pt_launch_glass_filter_shadow(hipStream_t, const DevScene&, const DevQueues& q, const DevQueues& sq, const DevAlpha& al, const DevGlass& gl, uint32_t max_rounds,
                                   const ShadowWalkCounters& ctr, const uint8_t* flags, bool first, float* tr_out, uint32_t* layers_out);
