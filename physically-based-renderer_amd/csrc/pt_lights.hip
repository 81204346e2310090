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
#include "pt_device.h"
#define PT_LIGHTS_DEVICE_PART
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
        const uint32_t prim = (uint32_t)__float_as_int(H.y) & ((1u << PT_LIGHTS_HIT_CLASS_SHIFT) - 1u);
        // ---- the surface, as k_shade's P5 rebuilds it ----
        const size_t rec = (size_t)prim * sc.shade_stride;
        const float4 r0 = sc.shade[rec], r1 = sc.shade[rec + 1], r2 = sc.shade[rec + 2], r3 = sc.shade[rec + 3], r4 = sc.shade[rec + 4];
        const v3 Pa = V3(r0.x, r0.y, r0.z), Pb = V3(r1.x, r1.y, r1.z), Pc = V3(r2.x, r2.y, r2.z);
        const v3 Na = V3(r2.w, r3.x, r3.y), Nb = V3(r3.z, r3.w, r4.x), Nc = V3(r4.y, r4.z, r4.w);
        const float hw = 1.0f - hu - hv;
        const v3 P = V3(pt_fma(Pc.x, hv, pt_fma(Pb.x, hu, Pa.x * hw)), pt_fma(Pc.y, hv, pt_fma(Pb.y, hu, Pa.y * hw)), pt_fma(Pc.z, hv, pt_fma(Pb.z, hu, Pa.z * hw)));
        v3 ng = normalize3(cross3(Pb - Pa, Pc - Pa));
        const v3 ni = V3(pt_fma(Nc.x, hv, pt_fma(Nb.x, hu, Na.x * hw)), pt_fma(Nc.y, hv, pt_fma(Nb.y, hu, Na.y * hw)), pt_fma(Nc.z, hv, pt_fma(Nb.z, hu, Na.z * hw)));
        v3 ns = normalize3(ni);
        const int mat = __float_as_int(r0.w);
        const float4 M0 = sc.mats[(size_t)(mat * 4 + 0)], M1 = sc.mats[(size_t)(mat * 4 + 1)], M2 = sc.mats[(size_t)(mat * 4 + 2)];
        float base_c[4] = {M0.x, M0.y, M0.z, M2.x};
        float metallic = M0.w, roughness = M1.w;
        const bool lambert = metallic == 0.0f && roughness >= 1.0f && __float_as_int(M2.w) < 0;
        if (__float_as_int(M2.y) >= 0 || __float_as_int(M2.z) >= 0 || __float_as_int(M2.w) >= 0) {     // a textured material: the record has the six further units
          const float4 x0 = sc.shade[rec + 5], x1 = sc.shade[rec + 6], x2 = sc.shade[rec + 7], x3 = sc.shade[rec + 8], x4 = sc.shade[rec + 9], x5 = sc.shade[rec + 10];
          pt_lights_apply_textures(sc, x0, x1, x2, x3, x4, x5, hu, hv, hw, M2, ni, base_c, metallic, roughness, ns);
        }
        const v3 wo = -d;
        const bool front = dot3(ng, wo) > 0.0f;
        if (dot3(ns, ng) < 0.0f) ns = -ns;
        if (!front) { ng = -ng; ns = -ns; }
        if (!(dot3(ns, wo) > 0.0f)) ns = ng;
        // ---- one light by the weight cdf, its sample at P ----
        const float u = rng_f(key, PT_LIGHTS_RNG_BASE + b + 1u, 0);
        const uint32_t li = pt_lights_cdf_search(s_cdf, n_lights, u);
        const float4 l0 = s_light[li * 4u], l1 = s_light[li * 4u + 1u], l2 = s_light[li * 4u + 2u], l3 = s_light[li * 4u + 3u];
        pt_light_rec L;
        L.pos[0] = l0.x; L.pos[1] = l0.y; L.pos[2] = l0.z; L.type = __float_as_int(l0.w);
        L.dir[0] = l1.x; L.dir[1] = l1.y; L.dir[2] = l1.z; L.range = l1.w;
        L.I[0] = l2.x; L.I[1] = l2.y; L.I[2] = l2.z; L.pmf = l2.w;
        L.scale = l3.x; L.offset = l3.y; L.cos_inner = l3.z; L.cos_outer = l3.w;
        const float Pf[3] = {P.x, P.y, P.z};
        float wif[3], Lif[3], dist;
        if (pt_light_sample(L, Pf, wif, dist, Lif)) {
          const v3 wi = V3(wif[0], wif[1], wif[2]);
          v3 tx, ty; onb(ns, tx, ty);
          const v3 wil = V3(dot3(tx, wi), dot3(ty, wi), dot3(ns, wi));
          if (wil.z > 0.0f && dot3(ng, wi) > 0.0f && (Lif[0] > 0.0f || Lif[1] > 0.0f || Lif[2] > 0.0f)) {
            const bsdf_t bs = make_bsdf(V3(base_c[0], base_c[1], base_c[2]), metallic, roughness, lambert);
            const v3 wol = V3(dot3(tx, wo), dot3(ty, wo), dot3(ns, wo));
            const float ps = spec_prob(bs, fmax2(wol.z, 1e-4f));
            const v3 porg = vfma(ng, sc.ray_eps, P);
            v3 f; float pb; bsdf_eval(bs, wol, wil, ps, f, pb);
            const float k = wil.z / L.pmf;
            v3 sdir = wi;
            float tmax = PT_T_INF;
            if (L.type != PTC_LIGHT_DIRECTIONAL) {      // the segment from the offset origin to the light, minus its last 0.1 %: the emitter sample's convention
              const v3 sv = V3(L.pos[0], L.pos[1], L.pos[2]) - porg;
              const float sd = pt_sqrt(dot3(sv, sv));
              sdir = sv * (1.0f / sd);
              tmax = sd * 0.999f;
            }
            has_shadow = true;
            sA = make_float4(porg.x, porg.y, porg.z, sdir.x);
            sB = make_float4(sdir.y, sdir.z, tmax, __uint_as_float(path));
            sC = make_float4(T.x * f.x * Lif[0] * k, T.y * f.y * Lif[1] * k, T.z * f.z * Lif[2] * k, 0.0f);
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
