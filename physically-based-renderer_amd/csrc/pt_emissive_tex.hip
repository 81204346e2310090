// pt_emissive_tex.hip — the textured-emission pass (see pt_emissive_tex.h).
//
//   k_shade_emissive_tex   runs behind k_shade(b), scan, any(b) and the punctual pass of a bounce b, over the SAME input: the live slots of ray[qi] and their hit
//                          records, which k_shade leaves as it found them (it writes ray[qi ^ 1]).
//                          Hit side (every b <= max_bounces): a front-facing hit on a primitive with an entry adds T * Le(hit uv) * wgt to the path's radiance.  Each
//                          path occurs once in the queue and any(b) has committed, so the write to q.lpath has a single owner: no float atomic.
//                          Sample side (b < max_bounces, a table with weight): per hit it rebuilds the surface exactly as k_shade_punctual does (same shading record,
//                          same material, same arithmetic), picks ONE entry by the weight cdf, evaluates pt_emtex_sample and the BSDF, and writes a shadow record
//                          (origin, direction, tmax, path, contribution) that k_trace_any then adds to the path's radiance if the point is visible.
// Layout: k_shade_punctual's.  Blocks of 256 threads, one WAVE owns one queue segment (seg = blockIdx.x * 4 + wave), takes its slots 64 at a time in queue order, and
// compacts the records it produces to the front of the same segment of q.shadow with a ballot and mbcnt64: no atomic, no block barrier, and a wave never writes more
// records than it read.  It writes q.seg_sh[seg] when the sample side runs.  Table and cdf are read from global memory (an entry is 112 bytes; the scenes that use
// the feature have hundreds to thousands of them).  The two statistics are one atomic per wave and counter, on lines of their own.
#include "pt_shading.h"
#include "pt_emissive_tex.h"

#define EMTEX_BLOCK 256
#define EMTEX_WAVES (EMTEX_BLOCK / 64)

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

__global__ __launch_bounds__(EMTEX_BLOCK) void k_shade_emissive_tex(DevScene sc, DevQueues q, int qi, uint32_t b, uint32_t max_bounces, DevEmTex et) {
  const uint32_t lane = lane_id();
  const uint32_t wave = threadIdx.x >> 6;
  const uint32_t seg = blockIdx.x * EMTEX_WAVES + wave;
  if (seg >= q.n_seg) return;
  const bool sample_side = b < max_bounces && et.sample != 0;
  const pt_emtex_textures tex{sc.texels, (const int32_t*)sc.tex_info, sc.tex_linear};
  const RayQ rin = q.ray[qi];
  const uint32_t base = seg * q.seg_len;                       // first slot of the segment, in every queue array
  const uint32_t n = (uint32_t)__builtin_amdgcn_readfirstlane((int)q.seg_ray[qi][seg]);
  uint32_t out_s = 0;                                          // wave cursor: shadow records written so far
  uint32_t n_hits = 0;
  for (uint32_t i0 = 0; i0 < n; i0 += 64u) {
    const bool valid = i0 + lane < n;
    const uint32_t slot = base + i0 + lane;
    bool has_shadow = false, added = false;
    float4 sA, sB, sC;
    sA = sB = sC = make_float4(0, 0, 0, 0);
    if (valid) {
      const float4 A = rin.A[slot], Bq = rin.B[slot], Cq = rin.C[slot], H = q.hit[slot];
      if (__float_as_int(H.y) >= 0) {
        const v3 d = V3(A.w, Bq.x, Bq.y);
        const v3 T = V3(Bq.z, Bq.w, Cq.x);
        const float prev_pdf = Cq.y;
        const uint32_t path = __float_as_uint(Cq.z), key = __float_as_uint(Cq.w);
        const float ht = H.x, hu = H.z, hv = H.w;
        const uint32_t prim = (uint32_t)__float_as_int(H.y) & ((1u << HIT_CLASS_SHIFT) - 1u);
        const int entry = et.prim_map[prim];
        if (entry >= 0 || sample_side) {
          // ---- the surface: k_shade's loads and its P5 (pt_shading.h) ----
          const size_t rec = (size_t)prim * sc.shade_stride;
          const float4 r0 = sc.shade[rec], r1 = sc.shade[rec + 1], r2 = sc.shade[rec + 2];
          const float hw = 1.0f - hu - hv;
          const v3 P = record_position(r0, r1, r2, hu, hv, hw);
          v3 ng = record_face_normal(r0, r1, r2);
          const v3 wo = -d;
          // ---- hit side: emission (one-sided), MIS against this set's sample ----
          if (entry >= 0 && dot3(ng, wo) > 0.0f) {
            const pt_emtex_rec E = load_entry(et.recs, (uint32_t)entry);
            const v3 Le = pt_emtex_radiance(E, tex, hu, hv);
            const float wgt = pt_emtex_hit_weight(E, b, prev_pdf, ht, dot3(ng, wo));
            float4 L = q.lpath[path];
            L.x = pt_fma(T.x * Le.x, wgt, L.x); L.y = pt_fma(T.y * Le.y, wgt, L.y); L.z = pt_fma(T.z * Le.z, wgt, L.z);
            q.lpath[path] = L;
            added = true;
          }
          if (sample_side) {
            const float4 r3 = sc.shade[rec + 3], r4 = sc.shade[rec + 4];
            const bool tex_cls = ((uint32_t)__float_as_int(H.y) >> HIT_CLASS_SHIFT) >= 2u;      // a textured class: the record has the six further units
            float4 x0, x1, x2, x3, x4, x5;
            x0 = x1 = x2 = x3 = x4 = x5 = make_float4(0, 0, 0, 0);
            if (tex_cls) { x0 = sc.shade[rec + 5]; x1 = sc.shade[rec + 6]; x2 = sc.shade[rec + 7]; x3 = sc.shade[rec + 8]; x4 = sc.shade[rec + 9]; x5 = sc.shade[rec + 10]; }
            const v3 ni = record_normal(r2, r3, r4, hu, hv, hw);
            v3 ns = normalize3(ni);
            float base_c[4], metallic, roughness;
            bool lambert;
            record_material(sc, sc.mats, __float_as_int(r0.w), x0, x1, x2, x3, x4, x5, hu, hv, hw, ni, base_c, metallic, roughness, lambert, ns);
            orient_normals(wo, ng, ns);
            // ---- one entry by the weight cdf, its sample at P ----
            const uint32_t rb = PT_EMTEX_RNG_BASE + b + 1u;
            const float u0 = rng_f(key, rb, 0), s1 = rng_f(key, rb, 1), s2 = rng_f(key, rb, 2);
            const uint32_t ei = cdf_search(et.cdf, et.n, u0);
            const pt_emtex_rec E = load_entry(et.recs, ei);
            v3 y, wi, Le;
            float pl;
            if (pt_emtex_sample(E, tex, P, s1, s2, y, wi, pl, Le)) {
              v3 tx, ty; onb(ns, tx, ty);
              const v3 wil = V3(dot3(tx, wi), dot3(ty, wi), dot3(ns, wi));
              if (wil.z > 0.0f && dot3(ng, wi) > 0.0f && (Le.x > 0.0f || Le.y > 0.0f || Le.z > 0.0f)) {
                const bsdf_t bs = make_bsdf(V3(base_c[0], base_c[1], base_c[2]), metallic, roughness, lambert);
                const v3 wol = V3(dot3(tx, wo), dot3(ty, wo), dot3(ns, wo));
                const float ps = spec_prob(bs, fmax2(wol.z, 1e-4f));
                const v3 porg = vfma(ng, sc.ray_eps, P);
                v3 f; float pb; bsdf_eval(bs, wol, wil, ps, f, pb);
                const float wgt = pt_emtex_sample_weight(pl, pb);
                const float k = (wil.z * wgt) / pl;
                // visibility: the segment from the offset origin porg to the sampled point, minus its last 0.1 %
                const v3 sv = y - porg;
                float sd;
                const v3 sdir = sv * pt_rnorm(dot3(sv, sv), sd);
                has_shadow = true;
                sA = make_float4(porg.x, porg.y, porg.z, sdir.x);
                sB = make_float4(sdir.y, sdir.z, sd * 0.999f, __uint_as_float(path));
                sC = make_float4(T.x * f.x * Le.x * k, T.y * f.y * Le.y * k, T.z * f.z * Le.z * k, 0.0f);
              }
            }
          }
        }
      }
    }
    n_hits += (uint32_t)__popcll(__ballot(added));
    if (sample_side) {
      // ---- compaction into the wave's own segment of the shadow queue ----
      const uint64_t ms = __ballot(has_shadow);
      if (has_shadow) { const uint32_t o = base + out_s + mbcnt64(ms); q.shadow.A[o] = sA; q.shadow.B[o] = sB; q.shadow.C[o] = sC; }
      out_s += (uint32_t)__popcll(ms);
    }
  }
  if (lane == 0) {
    if (sample_side) q.seg_sh[seg] = out_s;
    if (n_hits) atomicAdd(et.counters + PT_EMTEX_HITS, (unsigned long long)n_hits);
    if (out_s) atomicAdd(et.counters + PT_EMTEX_SHADOW, (unsigned long long)out_s);
  }
}
}  // namespace

void pt_launch_shade_emissive_tex(hipStream_t s, const DevScene& sc, const DevQueues& q, int qi, uint32_t bounce, uint32_t max_bounces, const DevEmTex& et) {
  if (!et.n) return;
  const dim3 grid((q.n_seg + EMTEX_WAVES - 1u) / EMTEX_WAVES);      // one wave per segment
  hipLaunchKernelGGL(k_shade_emissive_tex, grid, dim3(EMTEX_BLOCK), 0, s, sc, q, qi, bounce, max_bounces, et);
}
