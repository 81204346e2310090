// pt_alpha.h — alpha coverage: glTF alphaMode MASK and BLEND in the path integrator.
//
// A material is OPAQUE (every hit counts), MASK (a hit counts where its alpha reaches the cutoff) or BLEND (a hit counts with probability alpha).  The trace kernels
// know nothing of this: they report the nearest triangle.  Coverage is a pass of its own (pt_alpha.hip: k_alpha_filter) between the trace kernels and what
// consumes their results; a scene without such a material never launches it.  The alpha of a hit is base[3] as record_material (pt_shading.h) leaves it: the base
// colour's alpha, times the colour texel's alpha when the material has a colour texture, in the scene's filter mode.
//
// pt_alpha_accept / pt_alpha_transmit below are the definition — IEEE binary32, no contraction, in the order written; the host evaluation
// (ptc_debug_alpha_decide) and the kernel both call them.  tests/alpha_reference.py restates them in numpy.
//
// Closest hit (a path ray at bounce b, behind k_trace_closest(b), before k_shade(b)): layer k = 0, t_base = 0; while the ray's hit record is a hit on a
// primitive whose material is not OPAQUE:  u = rng_f(key, PT_ALPHA_RNG_BASE + b + 1, k), key = the ray record's C.w;  pt_alpha_accept: the hit stands;
// not accepted and k == max_layers: the hit stands as well (exhaustion, counted);  otherwise the ray passes: P = record_position, ng = record_face_normal,
// n = dot3(ng, d) > 0 ? ng : -ng, o' = vfma(n, ray_eps, P), t_base = t_base + t, k = k + 1, and (o', d) is traced again by the unchanged k_trace_closest.
// A ray that never passed keeps its record bit for bit; otherwise the record at its own slot of q.hit becomes (t_base + t, prim | class << 28, u, v) of the
// standing hit, or the miss record as the trace kernel wrote it.  ray[qi] is not touched: k_shade and k_shade_punctual see an ordinary hit.
// The deterministic form (the guides) decides BLEND as MASK with cutoff 0.5 and draws nothing.
//
// Shadow rays (no random numbers): the shadow queue is first traced by k_trace_any in its flag-writing form.  A record flagged free adds its contribution
// as AnyRay::publish does.  A flagged record is walked through its occluders by the closest-hit kernel: Tr = 1, rem = tmax; a miss or a hit with t >= rem ends
// the walk as visible; a hit with t < rem multiplies Tr by pt_alpha_transmit; Tr == 0: occluded; k == max_layers: occluded (exhaustion, counted); otherwise on
// from o' with rem = rem - t, k = k + 1.  Visible: lpath[path].c = lpath[path].c + Tr * contrib.c, the product skipped when Tr == 1.  The kernel is the shadow
// walk of pt_glass_shadow.h (k_glass_filter_shadow) without a glass table: it carries Tr in three equal channels.
//
// RNG: k_shade draws at the indices 0 .. max_bounces + 1 and the punctual pass at PT_LIGHTS_RNG_BASE + ..; PT_ALPHA_RNG_BASE + .. is disjoint from both.
//
// What ignores alpha: the raster integrators, ptc_debug_trace_closest, ptc_debug_trace_any and ptc_debug_punctual_nee.  Emitters are sampled by area without
// regard to coverage, so an emissive material is always OPAQUE (ptc_set_material_alpha refuses it).
#pragma once
#include "../../include/ptc.h"
#include "ptc_internal.h"
#include "pt_device.h"

#define PT_ALPHA_RNG_BASE 0x20000000u
#define PT_ALPHA_MAX_LAYERS 16
#define PT_ALPHA_DEFAULT_LAYERS 8

// does a hit of coverage `a` on a material of (mode, cutoff) count?  u: the layer's random number (BLEND only)
PT_HD bool pt_alpha_accept(int mode, float cutoff, float a, float u) {
  if (mode == PTC_ALPHA_MASK) return a >= cutoff;
  if (mode == PTC_ALPHA_BLEND) return u < a;
  return true;
}
// the share of a shadow ray's contribution that such a hit lets through
PT_HD float pt_alpha_transmit(int mode, float cutoff, float a) {
  if (mode == PTC_ALPHA_MASK) return a >= cutoff ? 0.0f : 1.0f;
  if (mode == PTC_ALPHA_BLEND) return 1.0f - fmin2(fmax2(a, 0.0f), 1.0f);
  return 0.0f;
}
// the deterministic form: BLEND decides as MASK with cutoff 0.5
PT_HD bool pt_alpha_accept_deterministic(int mode, float cutoff, float a) {
  return pt_alpha_accept(mode == PTC_ALPHA_BLEND ? PTC_ALPHA_MASK : mode, mode == PTC_ALPHA_BLEND ? 0.5f : cutoff, a, 0.0f);
}

// ---- the tables the pass reads --------------------------------------------------------------------------------------------------------------------
// counters of the pass (DevAlpha::counters), one 64-bit word each: a wave adds its totals once, when it ends
enum { PT_ALPHA_CLOSEST_PASSES = 0, PT_ALPHA_SHADOW_WALKED, PT_ALPHA_SHADOW_PASSES, PT_ALPHA_EXHAUSTED, PT_ALPHA_COUNTERS };
struct DevAlpha {
  const uint32_t* bits;          // one bit per original primitive id, set when its material is not OPAQUE: an opaque hit costs one 4-byte load from a table that stays in L2
  const float2* mode_cutoff;     // per material: (mode as int bits, cutoff)
  uint32_t max_layers;           // 1 .. PT_ALPHA_MAX_LAYERS
  unsigned long long* counters;  // [PT_ALPHA_COUNTERS]
};

// host: the two tables from the per-primitive material ids (HostBuilt::tri_mat: the host commit and the device commit both hold it; primitive ids survive refit and
// rebuild, so the tables do).  mode / cutoff may be shorter than the material list: the rest is OPAQUE.  Returns the number of primitives with a bit set.
inline uint32_t pt_alpha_tables(const std::vector<int32_t>& tri_mat, size_t n_mats, const std::vector<int32_t>& mode, const std::vector<float>& cutoff, std::vector<uint32_t>& bits,
                                std::vector<float>& mode_cutoff) {
  bits.assign((tri_mat.size() + 31u) / 32u, 0u);
  mode_cutoff.assign(n_mats * 2u, 0.0f);
  for (size_t m = 0; m < n_mats; ++m) {
    const int32_t md = m < mode.size() ? mode[m] : (int32_t)PTC_ALPHA_OPAQUE;
    mode_cutoff[m * 2u] = __builtin_bit_cast(float, md);
    mode_cutoff[m * 2u + 1u] = m < cutoff.size() ? cutoff[m] : 0.5f;
  }
  uint32_t n = 0;
  for (size_t p = 0; p < tri_mat.size(); ++p) {
    const int32_t m = tri_mat[p];
    if (m >= 0 && (size_t)m < mode.size() && mode[(size_t)m] != PTC_ALPHA_OPAQUE) { bits[p >> 5] |= 1u << (p & 31u); ++n; }
  }
  return n;
}

// ---- the kernel (pt_alpha.hip) ---------------------------------------------------------------------------------------------------------------------
// `aq` is the lane's alpha queue as a DevQueues view (ray[0] = the continuation records, hit, cnt, seg_ray[0], pre_ray of its own; seg_sh all zero): the unchanged
// pt_launch_scan and pt_launch_trace_closest take it as they take the batch's queues.  Continuation records: A = (o', d.x), B = (d.y, d.z, t_base, source slot) —
// the B.zw words the non-culling trace ignores —, C = (key, k, -, -); the shadow walk's own: pt_glass_shadow.h.
enum { PT_ALPHA_FORM_CLOSEST = 0, PT_ALPHA_FORM_GUIDE = 1, PT_ALPHA_FORM_SHADOW = 2 };
// round 0 of a closest-hit resolution (first = true): the batch's rays ray[qi] and their hit records -> the rays that pass, compacted to the front of each segment of aq.
// a later round (first = false): aq's records and THEIR hit records -> standing results scattered to the source slots of q.hit, the rays that pass compacted in place.
// form: PT_ALPHA_FORM_CLOSEST (stochastic) or PT_ALPHA_FORM_GUIDE (deterministic).  layers_out (or null): per source slot, the layers a ray passed (debug hook).
void pt_launch_alpha_filter_closest(hipStream_t, const DevScene&, const DevQueues& q, const DevQueues& aq, int qi, uint32_t bounce, const DevAlpha&, int form, bool first, uint32_t* layers_out);
