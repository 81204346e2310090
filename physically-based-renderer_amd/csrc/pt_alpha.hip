// pt_alpha.hip — the alpha-coverage pass (see pt_alpha.h).
//
//   k_alpha_filter_closest   one round of a closest-hit resolution.  Round 0 reads the batch's own queue (the rays of ray[qi] and their hit records); a later round
//                            reads the alpha queue and the hit records k_trace_closest wrote for it.  Rays whose result stands are written to their SOURCE slot's hit
//                            record; rays that pass through a surface go on in the alpha queue, to be traced again by the unchanged k_trace_closest.
// The shadow records of a scene with alpha materials are walked by k_glass_filter_shadow (pt_glass_shadow.hip), without a glass table.
// Layout: walk_segments (pt_walk_surfaces.h).
// Memory per hit that needs a decision: 48 B of shading record (positions, material), 32 B more (the uv units) and the texel taps when the class is textured,
// 8 B of (mode, cutoff); an opaque hit costs the 4-byte load of its bit.  The surface's alpha comes from record_material itself (pt_shading.h): the same texels and
// the same arithmetic as k_shade's base[3] (alpha_surface: pt_walk_surfaces.h, which the shadow walk through thin glass shares).
#include "pt_walk_surfaces.h"

namespace {
template <bool DET, bool FIRST>
__global__ __launch_bounds__(WALK_BLOCK) void k_alpha_filter_closest(DevScene sc, DevQueues q, DevQueues aq, int qi, uint32_t b, DevAlpha al, uint32_t* layers_out) {
  const RayQ rin = FIRST ? q.ray[qi] : aq.ray[0];
  const float4* hin = FIRST ? q.hit : aq.hit;
  unsigned long long n_pass = 0, n_exh = 0;
  bool exhausted = false;
  walk_segments(q, aq, FIRST ? q.seg_ray[qi] : aq.seg_ray[0], [&](uint32_t slot) __attribute__((always_inline)) {
    WalkNext c{};
    bool pass = false;
    const float4 H = hin[slot];
    const int pw = __float_as_int(H.y);
    // a continuation carries where it came from; a ray of round 0 is its own source
    uint32_t src = slot, k = 0, key = 0;
    float t_base = 0.0f;
    float4 A = make_float4(0, 0, 0, 0), Bq = A;
    bool decide = pw >= 0 && alpha_bit(al, (uint32_t)pw & ((1u << HIT_CLASS_SHIFT) - 1u));
    if (!FIRST || decide) {
      A = rin.A[slot]; Bq = rin.B[slot];
      const float4 Cq = rin.C[slot];
      if (FIRST) key = __float_as_uint(Cq.w);
      else { t_base = Bq.z; src = __float_as_uint(Bq.w); key = __float_as_uint(Cq.x); k = __float_as_uint(Cq.y); }
    }
    if (decide) {
      const v3 d = V3(A.w, Bq.x, Bq.y);
      int mode; float cutoff, a; v3 onward;
      alpha_surface(sc, al, H, d, mode, cutoff, a, onward);
      const bool accept = DET ? pt_alpha_accept_deterministic(mode, cutoff, a) : pt_alpha_accept(mode, cutoff, a, rng_f(key, PT_ALPHA_RNG_BASE + b + 1u, k));
      if (!accept) {
        if (k == al.max_layers) exhausted = true;
        else {
          pass = true;
          c.A = make_float4(onward.x, onward.y, onward.z, d.x);
          c.B = make_float4(d.y, d.z, t_base + H.x, __uint_as_float(src));
          c.C = make_float4(__uint_as_float(key), __uint_as_float(k + 1u), 0.0f, 0.0f);
        }
      }
    }
    if (!FIRST && !pass) {      // the result stands: to the source ray's own hit record (a ray of round 0 that stands keeps its record untouched)
      q.hit[src] = pw < 0 ? H : make_float4(t_base + H.x, H.y, H.z, H.w);
      if (layers_out) layers_out[src] = k;
    }
    c.go_on = pass;
    return c;
  }, [&](uint64_t mp) __attribute__((always_inline)) {
    n_pass += (unsigned long long)__popcll(mp);
    n_exh += (unsigned long long)__popcll(__ballot(exhausted));
    exhausted = false;
  });
  const uint32_t lane = lane_id();
  wave_count(&al.counters[PT_ALPHA_CLOSEST_PASSES], n_pass, lane);
  wave_count(&al.counters[PT_ALPHA_EXHAUSTED], n_exh, lane);
}
}  // namespace

void pt_launch_alpha_filter_closest(hipStream_t s, const DevScene& sc, const DevQueues& q, const DevQueues& aq, int qi, uint32_t bounce, const DevAlpha& al, int form, bool first,
                                    uint32_t* layers_out) {
  const dim3 grid = walk_grid(q), block(WALK_BLOCK);
  const bool det = form == PT_ALPHA_FORM_GUIDE;
  if (det && first) hipLaunchKernelGGL((k_alpha_filter_closest<true, true>), grid, block, 0, s, sc, q, aq, qi, bounce, al, layers_out);
  else if (det) hipLaunchKernelGGL((k_alpha_filter_closest<true, false>), grid, block, 0, s, sc, q, aq, qi, bounce, al, layers_out);
  else if (first) hipLaunchKernelGGL((k_alpha_filter_closest<false, true>), grid, block, 0, s, sc, q, aq, qi, bounce, al, layers_out);
  else hipLaunchKernelGGL((k_alpha_filter_closest<false, false>), grid, block, 0, s, sc, q, aq, qi, bounce, al, layers_out);
}
