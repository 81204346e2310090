// pt_glass_shadow.hip — the shadow walk through thin glass and alpha surfaces (see pt_glass_shadow.h).
//
//   k_glass_filter_shadow   one round of a shadow resolution.  Round 0 reads the batch's shadow queue and k_trace_any's flags; a later round reads the glass queue and
//                           the hit records k_trace_closest wrote for it.  A visible record adds Tr x its contribution to its path's radiance at its SOURCE slot's
//                           path (single owner, one continuation per source record); a record that passes a surface is compacted to the front of the same segment
//                           of the glass queue, to be traced again by the unchanged k_trace_closest.
// Layout: k_alpha_filter_shadow's.  Blocks of 256 threads, one WAVE owns one queue segment (seg = blockIdx.x * 4 + wave), takes its slots 64 at a time in queue order,
// and compacts what it produces with a ballot and mbcnt64: no atomic on the data path, no block barrier, and a wave never writes more records than it read — which is
// also why a later round can compact IN PLACE: a batch of 64 is loaded whole before anything is stored, and what it stores lies at or before its own slots.
// An empty round (every segment count 0) is a launch whose waves read one word each.
// Memory per hit: the 4-byte bit loads; an alpha hit costs what it costs k_alpha_filter_shadow, a glass hit what it costs k_glass_filter.
#include "pt_walk_surfaces.h"
#include "pt_glass_shadow.h"

#define GSH_BLOCK 256
#define GSH_WAVES (GSH_BLOCK / 64)

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

template <bool FIRST>
__global__ __launch_bounds__(GSH_BLOCK) void k_glass_filter_shadow(DevScene sc, DevQueues q, DevQueues gq, DevAlpha al, DevGlass gl, uint32_t max_rounds, unsigned long long* counters,
                                                                   const uint8_t* flags, float* tr_out, uint32_t* layers_out) {
  const uint32_t lane = lane_id();
  const uint32_t seg = blockIdx.x * GSH_WAVES + (threadIdx.x >> 6);
  if (seg >= q.n_seg) return;
  const RayQ rout = gq.ray[0];
  const uint32_t base = seg * q.seg_len;
  const uint32_t n = (uint32_t)__builtin_amdgcn_readfirstlane((int)(FIRST ? q.seg_sh[seg] : gq.seg_ray[0][seg]));
  uint32_t out = 0;
  unsigned long long n_walk = 0, n_pass = 0, n_vis = 0, n_exh = 0;
  for (uint32_t i0 = 0; i0 < n; i0 += 64u) {
    const uint32_t slot = base + i0 + lane;
    bool pass = false, exhausted = false, visible = false;
    float4 cA, cB, cC;
    cA = cB = cC = make_float4(0, 0, 0, 0);
    if (i0 + lane < n) {
      if (FIRST) {
        if (!flags[slot]) publish_shadow(q, slot, V3(1.0f, 1.0f, 1.0f), 0u, tr_out, layers_out);
        else {      // something lies in the way: the walk starts with the record's own ray
          const float4 A = q.shadow.A[slot], Bq = q.shadow.B[slot];
          pass = true;
          cA = A;
          cB = make_float4(Bq.x, Bq.y, Bq.z, __uint_as_float(slot));
          cC = make_float4(1.0f, 1.0f, 1.0f, __uint_as_float(0u));
        }
      } else {
        const float4 A = rout.A[slot], Bq = rout.B[slot], Cq = rout.C[slot], H = gq.hit[slot];
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
          } else if (glass_bit(gl, prim)) {
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
            cA = make_float4(onward.x, onward.y, onward.z, d.x);
            cB = make_float4(d.y, d.z, rem - H.x, __uint_as_float(src));
            cC = make_float4(Tr.x, Tr.y, Tr.z, __uint_as_float(k + 1u));
          }
        }
      }
    }
    const uint64_t mp = __ballot(pass);
    if (pass) { const uint32_t o = base + out + mbcnt64(mp); rout.A[o] = cA; rout.B[o] = cB; rout.C[o] = cC; }
    out += (uint32_t)__popcll(mp);
    if (FIRST) n_walk += (unsigned long long)__popcll(mp); else n_pass += (unsigned long long)__popcll(mp);
    n_vis += (unsigned long long)__popcll(__ballot(visible));
    n_exh += (unsigned long long)__popcll(__ballot(exhausted));
  }
  if (lane == 0) gq.seg_ray[0][seg] = out;
  wave_count(&counters[PT_GLASS_SHADOW_WALKED], n_walk, lane);
  wave_count(&counters[PT_GLASS_SHADOW_PASSES], n_pass, lane);
  wave_count(&counters[PT_GLASS_SHADOW_VISIBLE], n_vis, lane);
  wave_count(&counters[PT_GLASS_SHADOW_EXHAUSTED], n_exh, lane);
}
}  // namespace

void pt_launch_glass_filter_shadow(hipStream_t s, const DevScene& sc, const DevQueues& q, const DevQueues& gq, const DevAlpha& al, const DevGlass& gl, uint32_t max_rounds,
                                   unsigned long long* counters, const uint8_t* flags, bool first, float* tr_out, uint32_t* layers_out) {
  const dim3 grid((q.n_seg + GSH_WAVES - 1u) / GSH_WAVES), block(GSH_BLOCK);      // one wave per segment
  if (first) hipLaunchKernelGGL((k_glass_filter_shadow<true>), grid, block, 0, s, sc, q, gq, al, gl, max_rounds, counters, flags, tr_out, layers_out);
  else hipLaunchKernelGGL((k_glass_filter_shadow<false>), grid, block, 0, s, sc, q, gq, al, gl, max_rounds, counters, flags, tr_out, layers_out);
}
