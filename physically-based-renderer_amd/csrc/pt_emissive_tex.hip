// pt_emissive_tex.hip — the textured-emission pass (see pt_emissive_tex.h).
//
//   k_shade_emissive_tex   runs behind k_shade(b), scan, any(b) and the punctual pass of a bounce b, over the SAME input: the live slots of ray[qi] and their hit
//                          records, which k_shade leaves as it found them (it writes ray[qi ^ 1]).
//                          Hit side (every b <= max_bounces): a front-facing hit on a primitive with an entry adds T * Le(hit uv) * wgt to the path's radiance.  Each
//                          path occurs once in the queue and any(b) has committed, so the write to q.lpath has a single owner: no float atomic.
//                          Sample side (b < max_bounces, a table with weight): per hit it rebuilds the surface exactly as k_shade_punctual does (same shading record,
//                          same material, same arithmetic), picks ONE entry by the weight cdf, evaluates pt_emtex_sample and the BSDF, and writes a shadow record
//                          (origin, direction, tmax, path, contribution) that k_trace_any then adds to the path's radiance if the point is visible.
// Layout: the per-segment pass of pt_pass_common.h, into q.shadow.  It writes q.seg_sh[seg] when the sample side runs.  Table and cdf are read from global memory
// (an entry is 112 bytes; the scenes that use the feature have hundreds to thousands of them).  The two statistics are one atomic per wave and counter, on lines
// of their own.
#include "pt_pass_common.h"
#include "pt_emissive_tex.h"

namespace {
__device__ __forceinline__ pt_emtex_rec load_entry(const float4* __restrict__ recs, uint32_t e) {
  const float4* p = recs + (size_t)e * PT_EMTEX_UNITS;
  const float4 a0 = p[0], a1 = p[1], a2 = p[2], a3 = p[3], a4 = p[4], a5 = p[5], a6 = p[6];
  pt_emtex_rec E;
  E.p0[0] = a0.x; E.p0[1] = a0.y; E.p0[2] = a0.z; E.area = a0.w;
  E.e1[0] = a1.x; E.e1[1] = a1.y; E.e1[2] = a1.z; E.pmf = a1.w;
  E.e2[0] = a2.x; E.e2[1] = a2.y; E.e2[2] = a2.z; E.tex = __float_as_int(a2.w);
  E.n[0] = a3.x; E.n[1] = a3.y; E.n[2] = a3.z; E.pad0 = 0.0f;
  E.factor[0] = a4.x; E.factor[1] = a4.y; E.factor[2] = a4.z; E.pad1 = 0.0f;
  E.uv0[0] = a5.x; E.uv0[1] = a5.y; E.uv1[0] = a5.z; E.uv1[1] = a5.w;
  E.uv2[0] = a6.x; E.uv2[1] = a6.y; E.pad2[0] = E.pad2[1] = 0.0f;
  return E;
}

__global__ __launch_bounds__(WALK_BLOCK) void k_shade_emissive_tex(DevScene sc, DevQueues q, int qi, uint32_t b, uint32_t max_bounces, DevEmTex et) {
  const uint32_t lane = lane_id();
  const WaveSegment w = wave_segment(q);
  if (!w.owned) return;
  const bool sample_side = b < max_bounces && et.sample != 0;
  const pt_emtex_textures tex{sc.texels, (const int32_t*)sc.tex_info, sc.tex_linear};
  const RayQ rin = q.ray[qi];
  const uint32_t base = w.base(q), n = w.count(q.seg_ray[qi]);
  uint32_t out_s = 0;                                          // wave cursor: shadow records written so far
  uint32_t n_hits = 0;
  for (uint32_t i0 = 0; i0 < n; i0 += 64u) {
    const uint32_t slot = base + i0 + lane;
    bool added = false;
    ShadowRecord r{};
    if (i0 + lane < n) {
      const float4 A = rin.A[slot], Bq = rin.B[slot], Cq = rin.C[slot], H = q.hit[slot];
      if (__float_as_int(H.y) >= 0) {
        const v3 d = V3(A.w, Bq.x, Bq.y);
        const v3 T = V3(Bq.z, Bq.w, Cq.x);
        const float prev_pdf = Cq.y;
        const uint32_t path = __float_as_uint(Cq.z), key = __float_as_uint(Cq.w);
        const uint32_t prim = (uint32_t)__float_as_int(H.y) & ((1u << HIT_CLASS_SHIFT) - 1u);
        const int entry = et.prim_map[prim];
        if (entry >= 0 || sample_side) {
          const HitUnits u = load_hit_units(sc, H);      // the hit side needs no more than units 0..2
          const v3 wo = -d;
          // ---- hit side: emission (one-sided), MIS against this set's sample ----
          const v3 ng = hit_face_normal(u);
          const float cos_o = dot3(ng, wo);
          if (entry >= 0 && cos_o > 0.0f) {
            const pt_emtex_rec E = load_entry(et.recs, (uint32_t)entry);
            const v3 Le = pt_emtex_radiance(E, tex, u.hu, u.hv);
            const float wgt = pt_emtex_hit_weight(E, b, prev_pdf, H.x, cos_o);
            float4 L = q.lpath[path];
            L.x = pt_fma(T.x * Le.x, wgt, L.x); L.y = pt_fma(T.y * Le.y, wgt, L.y); L.z = pt_fma(T.z * Le.z, wgt, L.z);
            q.lpath[path] = L;
            added = true;
          }
          if (sample_side) {
            const HitSurface s = hit_surface(sc, d, u, load_hit_units_rest(sc, H, u), ng);
            // ---- one entry by the weight cdf, its sample at P ----
            const uint32_t rb = PT_EMTEX_RNG_BASE + b + 1u;
            const float u0 = rng_f(key, rb, 0), s1 = rng_f(key, rb, 1), s2 = rng_f(key, rb, 2);
            const pt_emtex_rec E = load_entry(et.recs, cdf_search(et.cdf, et.n, u0));
            v3 y, wi, Le;
            float pl;
            if (pt_emtex_sample(E, tex, s.P, s1, s2, y, wi, pl, Le))
              r = bsdf_shadow_record(s, sc.ray_eps, wo, wi, T, Le, path, [&](float cos_i, float pb) { return (cos_i * pt_emtex_sample_weight(pl, pb)) / pl; },
                                     [&](v3 porg, v3& sdir, float& tmax) {      // to the sampled point, minus the last 0.1 %
                                       const v3 sv = y - porg;
                                       float sd;
                                       sdir = sv * pt_rnorm(dot3(sv, sv), sd);
                                       tmax = sd * 0.999f;
                                     });
          }
        }
      }
    }
    n_hits += (uint32_t)__popcll(__ballot(added));
    if (sample_side) out_s += (uint32_t)__popcll(put_compacted(q.shadow, base + out_s, r.has, r.A, r.B, r.C));
  }
  if (lane == 0) {
    if (sample_side) q.seg_sh[w.seg] = out_s;
    if (n_hits) atomicAdd(et.counters + PT_EMTEX_HITS, (unsigned long long)n_hits);
    if (out_s) atomicAdd(et.counters + PT_EMTEX_SHADOW, (unsigned long long)out_s);
  }
}
}  // namespace

void pt_launch_shade_emissive_tex(hipStream_t s, const DevScene& sc, const DevQueues& q, int qi, uint32_t bounce, uint32_t max_bounces, const DevEmTex& et) {
  if (!et.n) return;
  hipLaunchKernelGGL(k_shade_emissive_tex, walk_grid(q), dim3(WALK_BLOCK), 0, s, sc, q, qi, bounce, max_bounces, et);
}
