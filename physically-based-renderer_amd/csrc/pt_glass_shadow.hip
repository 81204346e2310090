// pt_glass_shadow.hip — the shadow walk through alpha surfaces and thin glass (see pt_glass_shadow.h).
//
//   k_glass_filter_shadow   one round of a shadow resolution.  Round 0 reads the batch's shadow queue and k_trace_any's flags; a later round reads the side queue and
//                           the hit records k_trace_closest wrote for it.  A visible record adds Tr x its contribution to its path's radiance at its SOURCE slot's
//                           path; a record that passes a surface goes on in the side queue, to be traced again by the unchanged k_trace_closest.
// One kernel for both walks: a scene with alpha materials and no transparent shadows runs it on the alpha queue without a glass table (gl.bits == nullptr), a frame
// with transparent shadows on the glass queue, without an alpha table when the scene has no alpha material (al.bits == nullptr).  The walk without a glass table is
// an instantiation of its own (GLASS = false), so that it does not carry the registers of the glass surface: 7 waves per SIMD instead of 4.
// Layout: walk_segments (pt_walk_surfaces.h).
// Memory per hit: the 4-byte bit loads; an alpha hit costs what it costs k_alpha_filter_closest, a glass hit what it costs k_glass_filter.
#include "pt_walk_surfaces.h"
#include "pt_glass_shadow.h"

namespace {
// the visible record `src` of the shadow queue adds Tr x its contribution to its path's radiance: AnyRay::publish's addition, the products skipped for Tr == (1, 1, 1)
PT_DEV void publish_shadow(const DevQueues& q, uint32_t src, v3 Tr, uint32_t k, float* tr_out, uint32_t* layers_out) {
  if (tr_out) {
    tr_out[(size_t)src * 3u] = Tr.x; tr_out[(size_t)src * 3u + 1u] = Tr.y; tr_out[(size_t)src * 3u + 2u] = Tr.z;
    if (layers_out) layers_out[src] = k;
    return;
  }
  const uint32_t path = __float_as_uint(q.shadow.B[src].w);
  float4 Cq = q.shadow.C[src];
  if (!(Tr.x == 1.0f && Tr.y == 1.0f && Tr.z == 1.0f)) { Cq.x = Tr.x * Cq.x; Cq.y = Tr.y * Cq.y; Cq.z = Tr.z * Cq.z; }
  float4 L = q.lpath[path];
  L.x = L.x + Cq.x; L.y = L.y + Cq.y; L.z = L.z + Cq.z;
  q.lpath[path] = L;
}

template <bool FIRST, bool GLASS>
__global__ __launch_bounds__(WALK_BLOCK) void k_glass_filter_shadow(DevScene sc, DevQueues q, DevQueues sq, DevAlpha al, DevGlass gl, uint32_t max_rounds, ShadowWalkCounters ctr,
                                                                    const uint8_t* flags, float* tr_out, uint32_t* layers_out) {
  const RayQ rin = sq.ray[0];
  unsigned long long n_walk = 0, n_pass = 0, n_vis = 0, n_exh = 0;
  bool exhausted = false, visible = false;
  walk_segments(q, sq, FIRST ? q.seg_sh : sq.seg_ray[0], [&](uint32_t slot) __attribute__((always_inline)) {
    WalkNext c{};
    bool pass = false;
    if (FIRST) {
      if (!flags[slot]) publish_shadow(q, slot, V3(1.0f, 1.0f, 1.0f), 0u, tr_out, layers_out);
      else {      // something lies in the way: the walk starts with the record's own ray
        const float4 A = q.shadow.A[slot], Bq = q.shadow.B[slot];
        pass = true;
        c.A = A;
        c.B = make_float4(Bq.x, Bq.y, Bq.z, __uint_as_float(slot));
        c.C = make_float4(1.0f, 1.0f, 1.0f, __uint_as_float(0u));
      }
    } else {
      const float4 A = rin.A[slot], Bq = rin.B[slot], Cq = rin.C[slot], H = sq.hit[slot];
      const uint32_t src = __float_as_uint(Bq.w), k = __float_as_uint(Cq.w);
      const float rem = Bq.z;
      v3 Tr = V3(Cq.x, Cq.y, Cq.z);
      const int pw = __float_as_int(H.y);
      const uint32_t prim = (uint32_t)pw & ((1u << HIT_CLASS_SHIFT) - 1u);
      if (pw < 0 || !(H.x < rem)) { publish_shadow(q, src, Tr, k, tr_out, layers_out); visible = true; }
      else {
        const v3 d = V3(A.w, Bq.x, Bq.y);
        v3 onward = V3(0.0f, 0.0f, 0.0f);
        if (al.bits && alpha_bit(al, prim)) {
          int mode; float cutoff, a;
          alpha_surface(sc, al, H, d, mode, cutoff, a, onward);
          const float w = pt_alpha_transmit(mode, cutoff, a);
          Tr = V3(Tr.x * w, Tr.y * w, Tr.z * w);
        } else if (GLASS && glass_bit(gl, prim)) {
          const GlassSurface s = glass_surface(sc, gl, H, d);
          float F_t;
          const v3 W = pt_glass_shadow_transmit(s.m, s.ng, s.ns, d, s.base, s.metallic, F_t);
          Tr = V3(Tr.x * W.x, Tr.y * W.y, Tr.z * W.z);
          onward = vfma(s.ng, -sc.ray_eps, s.P);
        } else Tr = V3(0.0f, 0.0f, 0.0f);      // an opaque occluder
        if (Tr.x == 0.0f && Tr.y == 0.0f && Tr.z == 0.0f) {}      // occluded
        else if (k == max_rounds) exhausted = true;               // occluded
        else {
          pass = true;
          c.A = make_float4(onward.x, onward.y, onward.z, d.x);
          c.B = make_float4(d.y, d.z, rem - H.x, __uint_as_float(src));
          c.C = make_float4(Tr.x, Tr.y, Tr.z, __uint_as_float(k + 1u));
        }
      }
    }
    c.go_on = pass;
    return c;
  }, [&](uint64_t mp) __attribute__((always_inline)) {
    if (FIRST) n_walk += (unsigned long long)__popcll(mp); else n_pass += (unsigned long long)__popcll(mp);
    n_vis += (unsigned long long)__popcll(__ballot(visible));
    n_exh += (unsigned long long)__popcll(__ballot(exhausted));
    exhausted = visible = false;
  });
  const uint32_t lane = lane_id();
  wave_count(ctr.walked, n_walk, lane);
  wave_count(ctr.passes, n_pass, lane);
  if (ctr.visible) wave_count(ctr.visible, n_vis, lane);
  wave_count(ctr.exhausted, n_exh, lane);
}
}  // namespace

void pt_launch_glass_filter_shadow(hipStream_t s, const DevScene& sc, const DevQueues& q, const DevQueues& sq, const DevAlpha& al, const DevGlass& gl, uint32_t max_rounds,
                                   const ShadowWalkCounters& ctr, const uint8_t* flags, bool first, float* tr_out, uint32_t* layers_out) {
  const dim3 grid = walk_grid(q), block(WALK_BLOCK);
  if (first) hipLaunchKernelGGL((k_glass_filter_shadow<true, false>), grid, block, 0, s, sc, q, sq, al, gl, max_rounds, ctr, flags, tr_out, layers_out);      // round 0 meets no surface
  else if (gl.bits) hipLaunchKernelGGL((k_glass_filter_shadow<false, true>), grid, block, 0, s, sc, q, sq, al, gl, max_rounds, ctr, flags, tr_out, layers_out);
  else hipLaunchKernelGGL((k_glass_filter_shadow<false, false>), grid, block, 0, s, sc, q, sq, al, gl, max_rounds, ctr, flags, tr_out, layers_out);
}
