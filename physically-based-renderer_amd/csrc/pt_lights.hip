// pt_lights.hip — the punctual next-event pass (see pt_lights.h).
//
//   k_shade_punctual   runs behind k_shade(b), scan and any(b) of a bounce b < max_bounces, over the SAME input: the live slots of ray[qi] and their hit records,
//                      which k_shade leaves as it found them (it writes ray[qi ^ 1]).  Per hit it rebuilds the surface exactly as k_shade does (same shading record,
//                      same material, same arithmetic), picks ONE light by the weight cdf, evaluates pt_light_sample and the BSDF, and writes a shadow record
//                      (origin, direction, tmax, path, contribution) that k_trace_any then adds to the path's radiance if the light is visible.
// Layout: the per-segment pass of pt_pass_common.h, into q.shadow.  It writes q.seg_sh[seg]; nothing goes to lpath or to the ray queues.
// The light table (at most 256 x 64 B) and its cdf are staged in LDS once per block: 17 KiB, the one variant of the kernel.
// Memory per hit: 64 B of ray + hit record, the 80-byte shading record (176 B when the material is textured, plus its texel taps) and 48 B of material, all gathers —
// k_shade's traffic without its emitter and environment tables — and at most 48 B written.
#include "pt_pass_common.h"

namespace {
__global__ __launch_bounds__(WALK_BLOCK) void k_shade_punctual(DevScene sc, DevQueues q, int qi, uint32_t b, const float4* __restrict__ lights, const float* __restrict__ cdf,
                                                              uint32_t n_lights) {
  __shared__ float4 s_light[PT_LIGHTS_MAX * 4];
  __shared__ float s_cdf[PT_LIGHTS_MAX];
  stage_light_table(s_light, s_cdf, lights, cdf, n_lights);
  const uint32_t lane = lane_id();
  const WaveSegment w = wave_segment(q);
  if (!w.owned) return;
  const RayQ rin = q.ray[qi];
  const uint32_t base = w.base(q), n = w.count(q.seg_ray[qi]);
  uint32_t out_s = 0;                                          // wave cursor: shadow records written so far
  for (uint32_t i0 = 0; i0 < n; i0 += 64u) {
    const uint32_t slot = base + i0 + lane;
    ShadowRecord r{};
    if (i0 + lane < n) {
      const float4 A = rin.A[slot], Bq = rin.B[slot], Cq = rin.C[slot], H = q.hit[slot];
      if (__float_as_int(H.y) >= 0) {
        const v3 d = V3(A.w, Bq.x, Bq.y);
        const v3 T = V3(Bq.z, Bq.w, Cq.x);
        const uint32_t path = __float_as_uint(Cq.z), key = __float_as_uint(Cq.w);
        const HitSurface s = hit_surface(sc, H, d);
        // ---- one light by the weight cdf, its sample at P ----
        const float u = rng_f(key, PT_LIGHTS_RNG_BASE + b + 1u, 0);
        const pt_light_rec L = load_light_rec(s_light, cdf_search(s_cdf, n_lights, u));
        v3 wi, Li;
        float dist;
        if (pt_light_sample(L, s.P, wi, dist, Li))
          r = bsdf_shadow_record(s, sc.ray_eps, -d, wi, T, Li, path, [&](float cos_i, float) { return cos_i / L.pmf; },
                                 [&](v3 porg, v3& sdir, float& tmax) { punctual_segment(L, porg, wi, sdir, tmax); });
      }
    }
    out_s += (uint32_t)__popcll(put_compacted(q.shadow, base + out_s, r.has, r.A, r.B, r.C));
  }
  if (lane == 0) q.seg_sh[w.seg] = out_s;
}
}  // namespace

void pt_launch_shade_punctual(hipStream_t s, const DevScene& sc, const DevQueues& q, int qi, uint32_t bounce, const pt_light_rec* lights, const float* cdf, uint32_t n_lights) {
  if (!n_lights || n_lights > PT_LIGHTS_MAX) return;
  hipLaunchKernelGGL(k_shade_punctual, walk_grid(q), dim3(WALK_BLOCK), 0, s, sc, q, qi, bounce, (const float4*)lights, cdf, n_lights);
}
