// pt_glass.hip — the dielectric-transmission pass (see pt_glass.h).
//
//   k_glass_filter   one round of a resolution.  Round 0 reads the batch's own queue (the rays of ray[qi] and their hit records); a later round reads the glass queue
//                    and the hit records k_trace_closest wrote for it.  A ray whose hit stands (or that is exhausted) after at least one event is written to its
//                    SOURCE slot (the hit record and the ray record: single owner, one continuation per source ray); a ray with an event is compacted to the front
//                    of the same segment of the glass queue, to be traced again by the unchanged k_trace_closest.
// Layout: walk_segments (pt_walk_surfaces.h).
// The kernel is templated on transparent shadows (pt_glass_shadow.h): in such a frame a ray that only went straight through thin panes leaves the pass as a ray
// next-event estimation could have sampled — one more 16-byte load of the source origin at stand time.  The other instantiation does none of it.
// Memory per hit that needs a decision: the 80 B (192 B in a textured scene) of the shading record, the texel taps, 48 B of material and 32 B of glass record; a hit on
// anything else costs the 4-byte load of its bit from a table that stays in L2.  The surface comes from the pt_shading.h helpers: k_shade's texels and arithmetic.
#include "pt_walk_surfaces.h"

#define GLASS_BENT (1u << 16)      // SHADOWS: beside j in a continuation's C.y, set once the ray was reflected or refracted by a solid (j <= PT_GLASS_MAX_INTERACTIONS)

namespace {
// SHADOWS: the frame walks its shadow records through thin panes (pt_glass_shadow.h), so a ray all of whose events were thin transmissions leaves the pass as
// the straight ray it is: the pdf word, o and d of its source record, T rewritten, the standing hit's t measured from the source origin.  false: none of that.
template <bool FIRST, bool SHADOWS>
__global__ __launch_bounds__(WALK_BLOCK) void k_glass_filter(DevScene sc, DevQueues q, DevQueues gq, int qi, uint32_t b, DevGlass gl, uint32_t* j_out) {
  const RayQ rsrc = q.ray[qi];
  const RayQ rin = FIRST ? q.ray[qi] : gq.ray[0];
  const float4* hin = FIRST ? q.hit : gq.hit;
  unsigned long long n_refl = 0, n_refr = 0, n_stand = 0, n_exh = 0;
  bool reflected = false, exhausted = false, stood = false;
  walk_segments(q, gq, FIRST ? q.seg_ray[qi] : gq.seg_ray[0], [&](uint32_t slot) __attribute__((always_inline)) {
    WalkNext c{};
    bool go_on = false;
    float4 H = hin[slot];
    const int pw = __float_as_int(H.y);
    const bool decide = pw >= 0 && glass_bit(gl, (uint32_t)pw & ((1u << HIT_CLASS_SHIFT) - 1u));
    if (!FIRST || decide) {
      const float4 A = rin.A[slot], Bq = rin.B[slot], Cq = rin.C[slot];
      v3 o = V3(A.x, A.y, A.z), d = V3(A.w, Bq.x, Bq.y), T = V3(Bq.z, Bq.w, Cq.x);
      const uint32_t key = __float_as_uint(Cq.w);
      const uint32_t jw = FIRST ? 0u : __float_as_uint(Cq.y), src = FIRST ? slot : __float_as_uint(Cq.z);
      const uint32_t j = SHADOWS ? jw & (GLASS_BENT - 1u) : jw;
      bool bent = SHADOWS && (jw & GLASS_BENT) != 0u;
      int outcome = PT_GLASS_STANDS;
      bool beer = false;
      if (decide) {
        const GlassSurface s = glass_surface(sc, gl, H, d);
        beer = pt_glass_beer(s.m, s.front, H.x, T);
        const uint32_t idx = PT_GLASS_RNG_BASE + (b + 1u) * 64u + j;
        float F;
        outcome = pt_glass_interact(s.m, s.P, s.ng, s.ns, s.front, s.base, s.metallic, sc.ray_eps, rng_f(key, idx, 0), rng_f(key, idx, 1), j, gl.max_interactions, o, d, T, F);
        if (SHADOWS && (outcome == PT_GLASS_REFLECT || (outcome == PT_GLASS_TRANSMIT && s.m.thin == 0))) bent = true;
      }
      if (outcome >= PT_GLASS_REFLECT) {
        go_on = true; reflected = outcome == PT_GLASS_REFLECT;
        c.A = make_float4(o.x, o.y, o.z, d.x);
        c.B = make_float4(d.y, d.z, T.x, T.y);
        c.C = make_float4(T.z, __uint_as_float((j + 1u) | (bent ? GLASS_BENT : 0u)), __uint_as_float(src), __uint_as_float(key));
      } else if (!FIRST) {      // j >= 1: the standing hit (or the miss record) and the rewritten ray, at the source ray's own slot
        if (outcome == PT_GLASS_EXHAUSTED) { exhausted = true; H = make_float4(-1.0f, __int_as_float(-1), 0.0f, 0.0f); T = V3(0.0f, 0.0f, 0.0f); }
        else stood = true;      // counted as standing: the ray leaves the pass with a result for k_shade, a hit that stood or the trace's miss (pw < 0) alike
        if (SHADOWS && !bent) {      // it went straight on: d is the source record's, bit for bit; o and the pdf word stay, t counts from the source origin
          if (__float_as_int(H.y) >= 0) {
            const float4 As = rsrc.A[src];
            H.x = dot3(o - V3(As.x, As.y, As.z), d) + H.x;
          }
          q.hit[src] = H;
          *reinterpret_cast<float2*>(&rsrc.B[src].z) = make_float2(T.x, T.y);
          rsrc.C[src].x = T.z;
        } else {
          q.hit[src] = H;
          rsrc.A[src] = make_float4(o.x, o.y, o.z, d.x);
          rsrc.B[src] = make_float4(d.y, d.z, T.x, T.y);
          *reinterpret_cast<float2*>(&rsrc.C[src]) = make_float2(T.z, PT_GLASS_DELTA_PDF);      // path and key stay
        }
        if (j_out) j_out[src] = j;
      } else if (beer) {        // j = 0 and the hit stands: T alone
        rsrc.B[slot] = make_float4(Bq.x, Bq.y, T.x, T.y);
        rsrc.C[slot] = make_float4(T.z, Cq.y, Cq.z, Cq.w);
      }
    }
    c.go_on = go_on;
    return c;
  }, [&](uint64_t mp) __attribute__((always_inline)) {
    const unsigned long long nr = (unsigned long long)__popcll(__ballot(reflected));
    n_refl += nr; n_refr += (unsigned long long)__popcll(mp) - nr;
    n_stand += (unsigned long long)__popcll(__ballot(stood));
    n_exh += (unsigned long long)__popcll(__ballot(exhausted));
    reflected = exhausted = stood = false;
  });
  const uint32_t lane = lane_id();
  wave_count(&gl.counters[PT_GLASS_REFLECTIONS], n_refl, lane);
  wave_count(&gl.counters[PT_GLASS_REFRACTIONS], n_refr, lane);
  wave_count(&gl.counters[PT_GLASS_STANDING], n_stand, lane);
  wave_count(&gl.counters[PT_GLASS_EXHAUSTED_N], n_exh, lane);
}
}  // namespace

void pt_launch_glass_filter(hipStream_t s, const DevScene& sc, const DevQueues& q, const DevQueues& gq, int qi, uint32_t bounce, const DevGlass& gl, bool first, bool shadows, uint32_t* j_out) {
  const dim3 grid = walk_grid(q), block(WALK_BLOCK);
  if (first && shadows) hipLaunchKernelGGL((k_glass_filter<true, true>), grid, block, 0, s, sc, q, gq, qi, bounce, gl, j_out);
  else if (shadows) hipLaunchKernelGGL((k_glass_filter<false, true>), grid, block, 0, s, sc, q, gq, qi, bounce, gl, j_out);
  else if (first) hipLaunchKernelGGL((k_glass_filter<true, false>), grid, block, 0, s, sc, q, gq, qi, bounce, gl, j_out);
  else hipLaunchKernelGGL((k_glass_filter<false, false>), grid, block, 0, s, sc, q, gq, qi, bounce, gl, j_out);
}
