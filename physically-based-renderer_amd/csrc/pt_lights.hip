// pt_lights.hip — the punctual next-event pass (see pt_lights.h).
//
//   k_shade_punctual   runs behind k_shade(b), scan and any(b) of a bounce b < max_bounces, over the SAME input: the live slots of ray[qi] and their hit records,
//                      which k_shade leaves as it found them (it writes ray[qi ^ 1]).  Per hit it rebuilds the surface exactly as k_shade does (same shading record,
//                      same material, same arithmetic), picks ONE light by the weight cdf, evaluates pt_light_sample and the BSDF, and writes a shadow record
//                      (origin, direction, tmax, path, contribution) that k_trace_any then adds to the path's radiance if the light is visible.
// Layout: k_shade's.  Blocks of 256 threads, one WAVE owns one queue segment (seg = blockIdx.x * 4 + wave), takes its slots 64 at a time in queue order, and compacts
// the records it produces to the front of the same segment of q.shadow with a ballot and mbcnt64: no atomic, no block barrier after the staging, and a wave never
// writes more records than it read.  It writes q.seg_sh[seg]; nothing goes to lpath or to the ray queues.
// The light table (at most 256 x 64 B) and its cdf are staged in LDS once per block: 17 KiB, the one variant of the kernel.
// Memory per hit: 64 B of ray + hit record, the 80-byte shading record (176 B when the material is textured, plus its texel taps) and 48 B of material, all gathers —
// k_shade's traffic without its emitter and environment tables — and at most 48 B written.
#include "pt_shading.h"
#include "pt_lights.h"

#define PUNCTUAL_BLOCK 256
#define PUNCTUAL_WAVES (PUNCTUAL_BLOCK / 64)

namespace {
__global__ __launch_bounds__(PUNCTUAL_BLOCK) void k_shade_punctual(DevScene sc, DevQueues q, int qi, uint32_t b, const float4* __restrict__ lights, const float* __restrict__ cdf,
                                                                  uint32_t n_lights) {
  __shared__ float4 s_light[PT_LIGHTS_MAX * 4];
  __shared__ float s_cdf[PT_LIGHTS_MAX];
  for (uint32_t i = threadIdx.x; i < n_lights * 4u; i += PUNCTUAL_BLOCK) s_light[i] = lights[i];
  for (uint32_t i = threadIdx.x; i < n_lights; i += PUNCTUAL_BLOCK) s_cdf[i] = cdf[i];
  __syncthreads();
  const uint32_t lane = lane_id();
  const uint32_t wave = threadIdx.x >> 6;
  const uint32_t seg = blockIdx.x * PUNCTUAL_WAVES + wave;
  if (seg >= q.n_seg) return;
  const RayQ rin = q.ray[qi];
  const uint32_t base = seg * q.seg_len;                       // first slot of the segment, in every queue array
  const uint32_t n = (uint32_t)__builtin_amdgcn_readfirstlane((int)q.seg_ray[qi][seg]);
  uint32_t out_s = 0;                                          // wave cursor: shadow records written so far
  for (uint32_t i0 = 0; i0 < n; i0 += 64u) {
    const bool valid = i0 + lane < n;
    const uint32_t slot = base + i0 + lane;
    bool has_shadow = false;
    float4 sA, sB, sC;
    sA = sB = sC = make_float4(0, 0, 0, 0);
    if (valid) {
      const float4 A = rin.A[slot], Bq = rin.B[slot], Cq = rin.C[slot], H = q.hit[slot];
      if (__float_as_int(H.y) >= 0) {
        const v3 d = V3(A.w, Bq.x, Bq.y);
        const v3 T = V3(Bq.z, Bq.w, Cq.x);
        const uint32_t path = __float_as_uint(Cq.z), key = __float_as_uint(Cq.w);
        const float hu = H.z, hv = H.w;
        const uint32_t prim = (uint32_t)__float_as_int(H.y) & ((1u << HIT_CLASS_SHIFT) - 1u);
        // ---- the surface: k_shade's loads and its P5 (pt_shading.h) ----
        const size_t rec = (size_t)prim * sc.shade_stride;
        const float4 r0 = sc.shade[rec], r1 = sc.shade[rec + 1], r2 = sc.shade[rec + 2], r3 = sc.shade[rec + 3], r4 = sc.shade[rec + 4];
        const bool tex_cls = ((uint32_t)__float_as_int(H.y) >> HIT_CLASS_SHIFT) >= 2u;      // a textured class: the record has the six further units
        float4 x0, x1, x2, x3, x4, x5;
        x0 = x1 = x2 = x3 = x4 = x5 = make_float4(0, 0, 0, 0);
        if (tex_cls) { x0 = sc.shade[rec + 5]; x1 = sc.shade[rec + 6]; x2 = sc.shade[rec + 7]; x3 = sc.shade[rec + 8]; x4 = sc.shade[rec + 9]; x5 = sc.shade[rec + 10]; }
        const float hw = 1.0f - hu - hv;
        const v3 P = record_position(r0, r1, r2, hu, hv, hw);
        v3 ng = record_face_normal(r0, r1, r2);
        const v3 ni = record_normal(r2, r3, r4, hu, hv, hw);
        v3 ns = normalize3(ni);
        float base_c[4], metallic, roughness;
        bool lambert;
        record_material(sc, sc.mats, __float_as_int(r0.w), x0, x1, x2, x3, x4, x5, hu, hv, hw, ni, base_c, metallic, roughness, lambert, ns);
        const v3 wo = -d;
        orient_normals(wo, ng, ns);
        // ---- one light by the weight cdf, its sample at P ----
        const float u = rng_f(key, PT_LIGHTS_RNG_BASE + b + 1u, 0);
        const uint32_t li = cdf_search(s_cdf, n_lights, u);
        const float4 l0 = s_light[li * 4u], l1 = s_light[li * 4u + 1u], l2 = s_light[li * 4u + 2u], l3 = s_light[li * 4u + 3u];
        pt_light_rec L;
        L.pos[0] = l0.x; L.pos[1] = l0.y; L.pos[2] = l0.z; L.type = __float_as_int(l0.w);
        L.dir[0] = l1.x; L.dir[1] = l1.y; L.dir[2] = l1.z; L.range = l1.w;
        L.I[0] = l2.x; L.I[1] = l2.y; L.I[2] = l2.z; L.pmf = l2.w;
        L.scale = l3.x; L.offset = l3.y; L.cos_inner = l3.z; L.cos_outer = l3.w;
        v3 wi, Li;
        float dist;
        if (pt_light_sample(L, P, wi, dist, Li)) {
          v3 tx, ty; onb(ns, tx, ty);
          const v3 wil = V3(dot3(tx, wi), dot3(ty, wi), dot3(ns, wi));
          if (wil.z > 0.0f && dot3(ng, wi) > 0.0f && (Li.x > 0.0f || Li.y > 0.0f || Li.z > 0.0f)) {
            const bsdf_t bs = make_bsdf(V3(base_c[0], base_c[1], base_c[2]), metallic, roughness, lambert);
            const v3 wol = V3(dot3(tx, wo), dot3(ty, wo), dot3(ns, wo));
            const float ps = spec_prob(bs, fmax2(wol.z, 1e-4f));
            const v3 porg = vfma(ng, sc.ray_eps, P);
            v3 f; float pb; bsdf_eval(bs, wol, wil, ps, f, pb);
            const float k = wil.z / L.pmf;
            v3 sdir = wi;
            float tmax = PT_T_INF;
            if (L.type != PTC_LIGHT_DIRECTIONAL) {      // the segment from the offset origin to the light, minus its last 0.1 %: the emitter sample's convention
              const v3 sv = V3(L.pos) - porg;
              const float sd = pt_sqrt(dot3(sv, sv));
              sdir = sv * (1.0f / sd);
              tmax = sd * 0.999f;
            }
            has_shadow = true;
            sA = make_float4(porg.x, porg.y, porg.z, sdir.x);
            sB = make_float4(sdir.y, sdir.z, tmax, __uint_as_float(path));
            sC = make_float4(T.x * f.x * Li.x * k, T.y * f.y * Li.y * k, T.z * f.z * Li.z * k, 0.0f);
          }
        }
      }
    }
    // ---- compaction into the wave's own segment of the shadow queue ----
    const uint64_t ms = __ballot(has_shadow);
    if (has_shadow) { const uint32_t o = base + out_s + mbcnt64(ms); q.shadow.A[o] = sA; q.shadow.B[o] = sB; q.shadow.C[o] = sC; }
    out_s += (uint32_t)__popcll(ms);
  }
  if (lane == 0) q.seg_sh[seg] = out_s;
}
}  // namespace

void pt_launch_shade_punctual(hipStream_t s, const DevScene& sc, const DevQueues& q, int qi, uint32_t bounce, const pt_light_rec* lights, const float* cdf, uint32_t n_lights) {
  if (!n_lights || n_lights > PT_LIGHTS_MAX) return;
  const dim3 grid((q.n_seg + PUNCTUAL_WAVES - 1u) / PUNCTUAL_WAVES);      // one wave per segment
  hipLaunchKernelGGL(k_shade_punctual, grid, dim3(PUNCTUAL_BLOCK), 0, s, sc, q, qi, bounce, (const float4*)lights, cdf, n_lights);
}
