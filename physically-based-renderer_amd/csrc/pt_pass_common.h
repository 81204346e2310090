// pt_pass_common.h — what the passes beside k_shade share (device only): the segment a wave owns and its compaction cursor, the surface of a hit, the
// BSDF-weighted shadow record, the punctual light and the primary ray record.  One definition each; DESIGN.md §2d names the users.
//
// The layout of every per-segment pass (k_shade_punctual, k_shade_emissive_tex, k_medium_decide, k_medium_append, k_lm_first_hit and, through walk_segments,
// the three filter kernels): blocks of WALK_BLOCK threads, one WAVE owns one queue segment (seg = blockIdx.x * WALK_WAVES + wave), takes its slots 64 at a
// time in queue order, and compacts the records it produces to the front of the same segment of the destination queue with a ballot and mbcnt64: no atomic
// on the data path, no block barrier behind the staging of a light table, and a wave never writes more records than it read.
//
// pt_shading.h's helpers are used by k_shade, k_shade_raster and k_guides (pt_kernels.hip), by load_hit_units / hit_surface below — and through them by
// k_shade_punctual, k_shade_emissive_tex, k_glass_filter and k_glass_filter_shadow — by alpha_surface (pt_walk_surfaces.h) and by k_lm_first_hit.
// k_shade, k_raygen and k_raygen_guides (pt_kernels.hip) keep their own text of all of this: that file and pt_shading.h are hashed into kernels-sha256, which
// the committed kernel models are calibrated against, so nothing here is included there.
#pragma once
#include "pt_shading.h"
#include "pt_lights.h"

// ---- the segment of a wave and its compaction ------------------------------------------------------------------------------------------------------------
#define WALK_BLOCK 256
#define WALK_WAVES (WALK_BLOCK / 64)
inline dim3 walk_grid(const DevQueues& q) { return dim3((q.n_seg + WALK_WAVES - 1u) / WALK_WAVES); }      // one wave per segment

// which segment is this wave's, its first slot (in every queue array) and, per count array, how many slots it has.  A wave past the last segment owns none:
// it returns before it asks for either (so a count is read by whole waves only and stays in a scalar register).
struct WaveSegment {
  uint32_t seg;
  bool owned;
  PT_DEV uint32_t base(const DevQueues& q) const { return seg * q.seg_len; }
  PT_DEV uint32_t count(const uint32_t* seg_count) const { return (uint32_t)__builtin_amdgcn_readfirstlane((int)seg_count[seg]); }
};
PT_DEV WaveSegment wave_segment(const DevQueues& q) {
  WaveSegment w;
  w.seg = blockIdx.x * WALK_WAVES + (threadIdx.x >> 6);
  w.owned = w.seg < q.n_seg;
  return w;
}
// Compaction, whole wave: the lanes with `has` store (A, B, C) to the slots of dst from `at` on, in lane order; returns the ballot of those lanes.  `at` is the
// segment's first slot plus the wave's cursor — the records it has put there so far, a plain counter of the kernel's that advances by the ballot's popcount
// (a cursor object advanced through a member function compiles to other register numbers than the text it replaces: profiles/pass_common.txt).
template <class Q> PT_DEV uint64_t put_compacted(const Q& dst, uint32_t at, bool has, float4 A, float4 B, float4 C) {
  const uint64_t m = __ballot(has);
  if (has) { const uint32_t o = at + mbcnt64(m); dst.A[o] = A; dst.B[o] = B; dst.C[o] = C; }
  return m;
}

// ---- the surface of a hit: k_shade's loads and its P5 (pt_shading.h) --------------------------------------------------------------------------------------
// The units of the hit primitive's shading record, loaded in two steps so that a kernel keeps its own load order (as the P5 helpers ask) and no load waits
// behind arithmetic: units 0..2 — the positions, so P and the face normal, and the material — with the hit's barycentrics; then units 3..4 (the vertex
// normals) and, on a textured class, the six further units 5..10.
struct HitUnits { size_t rec; float hu, hv, hw; float4 r0, r1, r2; };
struct HitUnitsRest { float4 r3, r4, x0, x1, x2, x3, x4, x5; };
PT_DEV HitUnits load_hit_units(const DevScene& sc, float4 H) {
  HitUnits u;
  u.rec = (size_t)((uint32_t)__float_as_int(H.y) & ((1u << HIT_CLASS_SHIFT) - 1u)) * sc.shade_stride;
  u.hu = H.z; u.hv = H.w; u.hw = 1.0f - u.hu - u.hv;
  u.r0 = sc.shade[u.rec]; u.r1 = sc.shade[u.rec + 1]; u.r2 = sc.shade[u.rec + 2];
  return u;
}
PT_DEV HitUnitsRest load_hit_units_rest(const DevScene& sc, float4 H, const HitUnits& u) {
  HitUnitsRest x;
  x.r3 = sc.shade[u.rec + 3]; x.r4 = sc.shade[u.rec + 4];
  x.x0 = x.x1 = x.x2 = x.x3 = x.x4 = x.x5 = make_float4(0, 0, 0, 0);
  if (((uint32_t)__float_as_int(H.y) >> HIT_CLASS_SHIFT) >= 2u) {
    x.x0 = sc.shade[u.rec + 5]; x.x1 = sc.shade[u.rec + 6]; x.x2 = sc.shade[u.rec + 7]; x.x3 = sc.shade[u.rec + 8]; x.x4 = sc.shade[u.rec + 9]; x.x5 = sc.shade[u.rec + 10];
  }
  return x;
}
PT_DEV v3 hit_face_normal(const HitUnits& u) { return record_face_normal(u.r0, u.r1, u.r2); }      // as stored: not yet turned towards the ray
// the surface a ray of direction d sees at a hit: P, ng and ns after record_material and orient_normals(-d, ..), and the material's values.  The first form
// takes the loaded units and the stored face normal (k_shade_emissive_tex's hit side has it from units 0..2 alone; glass_surface loads its glass record
// between), the second loads and computes all of it.
struct HitSurface { v3 P, ng, ns, base; float metallic, roughness; bool lambert, front; int mat; };
PT_DEV HitSurface hit_surface(const DevScene& sc, v3 d, const HitUnits& u, const HitUnitsRest& x, v3 ng_stored) {
  HitSurface s;
  s.mat = __float_as_int(u.r0.w);
  s.P = record_position(u.r0, u.r1, u.r2, u.hu, u.hv, u.hw);
  s.ng = ng_stored;
  const v3 ni = record_normal(u.r2, x.r3, x.r4, u.hu, u.hv, u.hw);
  s.ns = normalize3(ni);
  float base_c[4];
  record_material(sc, sc.mats, s.mat, x.x0, x.x1, x.x2, x.x3, x.x4, x.x5, u.hu, u.hv, u.hw, ni, base_c, s.metallic, s.roughness, s.lambert, s.ns);
  s.front = orient_normals(-d, s.ng, s.ns);
  s.base = V3(base_c[0], base_c[1], base_c[2]);
  return s;
}
PT_DEV HitSurface hit_surface(const DevScene& sc, float4 H, v3 d) {
  const HitUnits u = load_hit_units(sc, H);
  const HitUnitsRest x = load_hit_units_rest(sc, H, u);
  return hit_surface(sc, d, u, x, hit_face_normal(u));
}

// ---- the BSDF-weighted shadow record ------------------------------------------------------------------------------------------------------------------------
// Next-event estimation at surface s for the direction wi (unit, towards the light) along which L arrives, seen from wo: the two-sided test, the BSDF value f
// and its pdf pb, the origin porg = ng * eps + P, and the record (porg, sdir, tmax, path, T * f * L * k).  What differs between the passes stays with them:
// k_of(wil.z, pb) is the caller's factor, segment(porg, sdir, tmax) its visibility segment from porg.
struct ShadowRecord { bool has; float4 A, B, C; };
template <class K, class Seg>
PT_DEV ShadowRecord bsdf_shadow_record(const HitSurface& s, float eps, v3 wo, v3 wi, v3 T, v3 L, uint32_t path, K k_of, Seg segment) {
  ShadowRecord r;
  r.has = false;
  r.A = r.B = r.C = make_float4(0, 0, 0, 0);
  v3 tx, ty; onb(s.ns, tx, ty);
  const v3 wil = V3(dot3(tx, wi), dot3(ty, wi), dot3(s.ns, wi));
  if (wil.z > 0.0f && dot3(s.ng, wi) > 0.0f && (L.x > 0.0f || L.y > 0.0f || L.z > 0.0f)) {
    const bsdf_t bs = make_bsdf(s.base, s.metallic, s.roughness, s.lambert);
    const v3 wol = V3(dot3(tx, wo), dot3(ty, wo), dot3(s.ns, wo));
    const float ps = spec_prob(bs, fmax2(wol.z, 1e-4f));
    const v3 porg = vfma(s.ng, eps, s.P);
    v3 f; float pb; bsdf_eval(bs, wol, wil, ps, f, pb);
    const float k = k_of(wil.z, pb);
    v3 sdir; float tmax;
    segment(porg, sdir, tmax);
    r.has = true;
    r.A = make_float4(porg.x, porg.y, porg.z, sdir.x);
    r.B = make_float4(sdir.y, sdir.z, tmax, __uint_as_float(path));
    r.C = make_float4(T.x * f.x * L.x * k, T.y * f.y * L.y * k, T.z * f.z * L.z * k, 0.0f);
  }
  return r;
}

// ---- the punctual light (pt_lights.h) -------------------------------------------------------------------------------------------------------------------------
PT_DEV pt_light_rec load_light_rec(const float4* table, uint32_t i) {
  const float4 l0 = table[i * 4u], l1 = table[i * 4u + 1u], l2 = table[i * 4u + 2u], l3 = table[i * 4u + 3u];
  pt_light_rec L;
  L.pos[0] = l0.x; L.pos[1] = l0.y; L.pos[2] = l0.z; L.type = __float_as_int(l0.w);
  L.dir[0] = l1.x; L.dir[1] = l1.y; L.dir[2] = l1.z; L.range = l1.w;
  L.I[0] = l2.x; L.I[1] = l2.y; L.I[2] = l2.z; L.pmf = l2.w;
  L.scale = l3.x; L.offset = l3.y; L.cos_inner = l3.z; L.cos_outer = l3.w;
  return L;
}
// the table (at most PT_LIGHTS_MAX x 64 B) and its cdf into a block's LDS copies — 17 KiB — and the barrier behind them: whole block
PT_DEV void stage_light_table(float4* s_light, float* s_cdf, const float4* lights, const float* cdf, uint32_t n_lights) {
  for (uint32_t i = threadIdx.x; i < n_lights * 4u; i += WALK_BLOCK) s_light[i] = lights[i];
  for (uint32_t i = threadIdx.x; i < n_lights; i += WALK_BLOCK) s_cdf[i] = cdf[i];
  __syncthreads();
}
// the visibility segment from `origin` to light L sampled in direction wi: to the light minus its last 0.1 % (the emitter sample's convention), without end
// for a directional light
PT_DEV void punctual_segment(const pt_light_rec& L, v3 origin, v3 wi, v3& sdir, float& tmax) {
  sdir = wi;
  tmax = PT_T_INF;
  if (L.type != PTC_LIGHT_DIRECTIONAL) {
    const v3 sv = V3(L.pos) - origin;
    const float sd = pt_sqrt(dot3(sv, sv));
    sdir = sv * (1.0f / sd);
    tmax = sd * 0.999f;
  }
}

// ---- the primary ray record -------------------------------------------------------------------------------------------------------------------------------------
// path p of a batch starts at o along d with throughput 1, no pdf and its RNG key: A = (o, d.x), B = (d.y, d.z, 1, 1), C = (1, 0, p, key) in ray[0], four
// coalesced 16-byte stores with the cleared path radiance
PT_DEV void store_primary_ray(const DevQueues& q, uint32_t p, v3 o, v3 d, uint32_t key, bool clear_lpath) {
  const RayQ& r = q.ray[0];
  r.A[p] = make_float4(o.x, o.y, o.z, d.x);
  r.B[p] = make_float4(d.y, d.z, 1.0f, 1.0f);
  r.C[p] = make_float4(1.0f, 0.0f, __uint_as_float(p), __uint_as_float(key));
  if (clear_lpath) q.lpath[p] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
}
