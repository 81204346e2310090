// pt_walk_surfaces.h — what the alpha pass, the glass pass and the shadow walk through thin glass need of a hit (device only): the bit of a primitive, the
// alpha-mapped surface and the transmissive surface, each from the pt_shading.h helpers — k_shade's loads, texels and arithmetic.
#pragma once
#include "pt_pass_common.h"
#include "pt_alpha.h"
#include "pt_glass.h"

PT_DEV bool alpha_bit(const DevAlpha& al, uint32_t prim) { return (al.bits[prim >> 5] >> (prim & 31u)) & 1u; }
PT_DEV bool glass_bit(const DevGlass& gl, uint32_t prim) { return (gl.bits[prim >> 5] >> (prim & 31u)) & 1u; }
PT_DEV void wave_count(unsigned long long* ctr, unsigned long long v, uint32_t lane) { if (lane == 0 && v) atomicAdd(ctr, v); }

// ---- the segment walk: the loop of every filter kernel (pt_alpha.hip, pt_glass.hip, pt_glass_shadow.hip), on pt_pass_common.h's segment and cursor ---------------
// The records that go on are compacted to the front of the same segment of the side queue `sq`, which is also why a later round can compact IN PLACE
// (seg_count == sq.seg_ray[0]): a batch of 64 is loaded whole before anything is stored, and what it stores lies at or before its own slots.  An empty round
// (every segment count 0) is a launch whose waves read one word each.
//   record(slot) -> WalkNext   one lane's record: whether it goes on, and then its continuation (A, B, C); a result that stands it stores itself, to its SOURCE slot
//                              (single owner, one continuation per source record); what the kernel counts it leaves in the kernel's own flags
//   tally(mp)                  once per batch, whole wave: mp is the ballot of the lanes that go on; the kernel adds its flags' ballots to its sums and clears the
//                              flags (a lane past the segment's end never ran record).  The sums go to wave_count when the walk returns (a wave without a
//                              segment returns with every sum 0)
struct WalkNext { bool go_on; float4 A, B, C; };

template <class Record, class Tally>
PT_DEV void walk_segments(const DevQueues& q, const DevQueues& sq, const uint32_t* seg_count, Record record, Tally tally) {
  const uint32_t lane = lane_id();
  const WaveSegment w = wave_segment(q);
  if (!w.owned) return;
  const RayQ rout = sq.ray[0];
  const uint32_t base = w.base(q), n = w.count(seg_count);
  uint32_t out = 0;
  for (uint32_t i0 = 0; i0 < n; i0 += 64u) {
    WalkNext c{};
    if (i0 + lane < n) c = record(base + i0 + lane);
    const uint64_t mp = put_compacted(rout, base + out, c.go_on, c.A, c.B, c.C);
    out += (uint32_t)__popcll(mp);
    tally(mp);
  }
  if (lane == 0) sq.seg_ray[0][w.seg] = out;
}

// the alpha-mapped surface of a hit: its material's (mode, cutoff), its coverage a, and where a ray (.., d) that passes through it goes on from
PT_DEV void alpha_surface(const DevScene& sc, const DevAlpha& al, float4 H, v3 d, int& mode, float& cutoff, float& a, v3& onward) {
  const uint32_t hw_word = (uint32_t)__float_as_int(H.y);
  const uint32_t prim = hw_word & ((1u << HIT_CLASS_SHIFT) - 1u);
  const float hu = H.z, hv = H.w, hw = 1.0f - hu - hv;
  const size_t rec = (size_t)prim * sc.shade_stride;
  const float4 r0 = sc.shade[rec], r1 = sc.shade[rec + 1], r2 = sc.shade[rec + 2];
  float4 x0, x1;
  const float4 z = make_float4(0, 0, 0, 0);
  x0 = x1 = z;
  if ((hw_word >> HIT_CLASS_SHIFT) >= 2u) { x0 = sc.shade[rec + 5]; x1 = sc.shade[rec + 6]; }      // a textured class: the uv units (the tangent units only feed the normal map)
  const int mat = __float_as_int(r0.w);
  float base[4], metallic, roughness;
  bool lambert;
  v3 ns = V3(0.0f, 0.0f, 1.0f);
  record_material(sc, sc.mats, mat, x0, x1, z, z, z, z, hu, hv, hw, V3(0.0f, 0.0f, 1.0f), base, metallic, roughness, lambert, ns);
  a = base[3];
  const float2 mc = al.mode_cutoff[mat];
  mode = __float_as_int(mc.x); cutoff = mc.y;
  const v3 P = record_position(r0, r1, r2, hu, hv, hw);
  const v3 ng = record_face_normal(r0, r1, r2);
  const v3 n = dot3(ng, d) > 0.0f ? ng : -ng;
  onward = vfma(n, sc.ray_eps, P);
}

// the transmissive surface of a hit H of a ray of direction d: hit_surface and the glass record of its material
struct GlassSurface : HitSurface { pt_glass_mat m; };
PT_DEV GlassSurface glass_surface(const DevScene& sc, const DevGlass& gl, float4 H, v3 d) {
  const HitUnits u = load_hit_units(sc, H);
  const HitUnitsRest x = load_hit_units_rest(sc, H, u);
  const int mat = __float_as_int(u.r0.w);
  const float4 g0 = gl.mats[(size_t)mat * 2u], g1 = gl.mats[(size_t)mat * 2u + 1u];
  GlassSurface s{hit_surface(sc, d, u, x, hit_face_normal(u)), {}};
  s.m.tau = g0.x; s.m.ior = g0.y; s.m.thin = __float_as_int(g0.z); s.m.pad0 = 0.0f; s.m.sigma2[0] = g1.x; s.m.sigma2[1] = g1.y; s.m.sigma2[2] = g1.z; s.m.pad1 = 0.0f;
  return s;
}
