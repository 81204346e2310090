// pt_alpha.hip — the alpha-coverage pass (see pt_alpha.h).
//
//   k_alpha_filter   one round of a resolution.  Round 0 reads the batch's own queue (the rays of ray[qi] and their hit records, or the shadow records and
//                    k_trace_any's flags); a later round reads the alpha queue and the hit records k_trace_closest wrote for it.  Rays whose result stands are
//                    written to their SOURCE slot (the hit record, or the addition to lpath: single owner, one continuation per source ray); rays that pass
//                    through a surface are compacted to the front of the same segment of the alpha queue, to be traced again by the unchanged k_trace_closest.
// Layout: k_shade_punctual's.  Blocks of 256 threads, one WAVE owns one queue segment (seg = blockIdx.x * 4 + wave), takes its slots 64 at a time in queue order, and
// compacts what it produces with a ballot and mbcnt64: no atomic on the data path, no block barrier, and a wave never writes more records than it read — which is
// also why a later round can compact IN PLACE: a batch of 64 is loaded whole before anything is stored, and what it stores lies at or before its own slots.
// An empty round (every segment count 0) is a launch whose waves read one word each.
// Memory per hit that needs a decision: 48 B of shading record (positions, material), 32 B more (the uv units) and the texel taps when the class is textured,
// 8 B of (mode, cutoff); an opaque hit costs the 4-byte load of its bit.  The surface's alpha comes from record_material itself (pt_shading.h): the same texels and
// the same arithmetic as k_shade's base[3] (alpha_surface: pt_walk_surfaces.h, which the shadow walk through thin glass shares).
#include "pt_walk_surfaces.h"

#define ALPHA_BLOCK 256
#define ALPHA_WAVES (ALPHA_BLOCK / 64)

namespace {
// ---- closest hit ------------------------------------------------------------------------------------------------------------------------------------
template <bool DET, bool FIRST>
__global__ __launch_bounds__(ALPHA_BLOCK) void k_alpha_filter_closest(DevScene sc, DevQueues q, DevQueues aq, int qi, uint32_t b, DevAlpha al, uint32_t* layers_out) {
  const uint32_t lane = lane_id();
  const uint32_t seg = blockIdx.x * ALPHA_WAVES + (threadIdx.x >> 6);
  if (seg >= q.n_seg) return;
  const RayQ rin = FIRST ? q.ray[qi] : aq.ray[0];
  const float4* hin = FIRST ? q.hit : aq.hit;
  const RayQ rout = aq.ray[0];
  const uint32_t base = seg * q.seg_len;
  const uint32_t n = (uint32_t)__builtin_amdgcn_readfirstlane((int)(FIRST ? q.seg_ray[qi][seg] : aq.seg_ray[0][seg]));
  uint32_t out = 0;
  unsigned long long n_pass = 0, n_exh = 0;
  for (uint32_t i0 = 0; i0 < n; i0 += 64u) {
    const uint32_t slot = base + i0 + lane;
    bool pass = false, exhausted = false;
    float4 cA, cB, cC;
    cA = cB = cC = make_float4(0, 0, 0, 0);
    if (i0 + lane < n) {
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
            cA = make_float4(onward.x, onward.y, onward.z, d.x);
            cB = make_float4(d.y, d.z, t_base + H.x, __uint_as_float(src));
            cC = make_float4(__uint_as_float(key), __uint_as_float(k + 1u), 0.0f, 0.0f);
          }
        }
      }
      if (!FIRST && !pass) {      // the result stands: to the source ray's own hit record (a ray of round 0 that stands keeps its record untouched)
        q.hit[src] = pw < 0 ? H : make_float4(t_base + H.x, H.y, H.z, H.w);
        if (layers_out) layers_out[src] = k;
      }
    }
    const uint64_t mp = __ballot(pass);
    if (pass) { const uint32_t o = base + out + mbcnt64(mp); rout.A[o] = cA; rout.B[o] = cB; rout.C[o] = cC; }
    out += (uint32_t)__popcll(mp);
    n_pass += (unsigned long long)__popcll(mp);
    n_exh += (unsigned long long)__popcll(__ballot(exhausted));
  }
  if (lane == 0) aq.seg_ray[0][seg] = out;
  wave_count(&al.counters[PT_ALPHA_CLOSEST_PASSES], n_pass, lane);
  wave_count(&al.counters[PT_ALPHA_EXHAUSTED], n_exh, lane);
}

// ---- shadow rays -------------------------------------------------------------------------------------------------------------------------------------
// the visible record `src` of the shadow queue adds Tr x its contribution to its path's radiance: AnyRay::publish's addition, the product skipped for Tr == 1
PT_DEV void publish_shadow(const DevQueues& q, uint32_t src, float Tr, float* tr_out) {
  if (tr_out) { tr_out[src] = Tr; return; }
  const uint32_t path = __float_as_uint(q.shadow.B[src].w);
  float4 Cq = q.shadow.C[src];
  if (Tr != 1.0f) { Cq.x = Tr * Cq.x; Cq.y = Tr * Cq.y; Cq.z = Tr * Cq.z; }
  float4 L = q.lpath[path];
  L.x = L.x + Cq.x; L.y = L.y + Cq.y; L.z = L.z + Cq.z;
  q.lpath[path] = L;
}

template <bool FIRST>
__global__ __launch_bounds__(ALPHA_BLOCK) void k_alpha_filter_shadow(DevScene sc, DevQueues q, DevQueues aq, DevAlpha al, const uint8_t* flags, float* tr_out) {
  const uint32_t lane = lane_id();
  const uint32_t seg = blockIdx.x * ALPHA_WAVES + (threadIdx.x >> 6);
  if (seg >= q.n_seg) return;
  const RayQ rout = aq.ray[0];
  const uint32_t base = seg * q.seg_len;
  const uint32_t n = (uint32_t)__builtin_amdgcn_readfirstlane((int)(FIRST ? q.seg_sh[seg] : aq.seg_ray[0][seg]));
  uint32_t out = 0;
  unsigned long long n_walk = 0, n_pass = 0, n_exh = 0;
  for (uint32_t i0 = 0; i0 < n; i0 += 64u) {
    const uint32_t slot = base + i0 + lane;
    bool pass = false, exhausted = false;
    float4 cA, cB, cC;
    cA = cB = cC = make_float4(0, 0, 0, 0);
    if (i0 + lane < n) {
      if (FIRST) {
        if (!flags[slot]) publish_shadow(q, slot, 1.0f, tr_out);
        else {      // something lies in the way: the walk starts with the record's own ray
          const float4 A = q.shadow.A[slot], Bq = q.shadow.B[slot];
          pass = true;
          cA = A;
          cB = make_float4(Bq.x, Bq.y, Bq.z, __uint_as_float(slot));
          cC = make_float4(0.0f, __uint_as_float(0u), 1.0f, 0.0f);
        }
      } else {
        const float4 A = rout.A[slot], Bq = rout.B[slot], Cq = rout.C[slot], H = aq.hit[slot];
        const uint32_t src = __float_as_uint(Bq.w), k = __float_as_uint(Cq.y);
        const float rem = Bq.z;
        float Tr = Cq.z;
        const int pw = __float_as_int(H.y);
        if (pw < 0 || !(H.x < rem)) publish_shadow(q, src, Tr, tr_out);
        else if (alpha_bit(al, (uint32_t)pw & ((1u << HIT_CLASS_SHIFT) - 1u))) {
          const v3 d = V3(A.w, Bq.x, Bq.y);
          int mode; float cutoff, a; v3 onward;
          alpha_surface(sc, al, H, d, mode, cutoff, a, onward);
          Tr = Tr * pt_alpha_transmit(mode, cutoff, a);
          if (Tr == 0.0f) {}      // occluded
          else if (k == al.max_layers) exhausted = true;      // occluded
          else {
            pass = true;
            cA = make_float4(onward.x, onward.y, onward.z, d.x);
            cB = make_float4(d.y, d.z, rem - H.x, __uint_as_float(src));
            cC = make_float4(0.0f, __uint_as_float(k + 1u), Tr, 0.0f);
          }
        }      // an opaque occluder: Tr = 0
      }
    }
    const uint64_t mp = __ballot(pass);
    if (pass) { const uint32_t o = base + out + mbcnt64(mp); rout.A[o] = cA; rout.B[o] = cB; rout.C[o] = cC; }
    out += (uint32_t)__popcll(mp);
    if (FIRST) n_walk += (unsigned long long)__popcll(mp); else n_pass += (unsigned long long)__popcll(mp);
    n_exh += (unsigned long long)__popcll(__ballot(exhausted));
  }
  if (lane == 0) aq.seg_ray[0][seg] = out;
  wave_count(&al.counters[PT_ALPHA_SHADOW_WALKED], n_walk, lane);
  wave_count(&al.counters[PT_ALPHA_SHADOW_PASSES], n_pass, lane);
  wave_count(&al.counters[PT_ALPHA_EXHAUSTED], n_exh, lane);
}

dim3 alpha_grid(const DevQueues& q) { return dim3((q.n_seg + ALPHA_WAVES - 1u) / ALPHA_WAVES); }      // one wave per segment
}  // namespace

void pt_launch_alpha_filter_closest(hipStream_t s, const DevScene& sc, const DevQueues& q, const DevQueues& aq, int qi, uint32_t bounce, const DevAlpha& al, int form, bool first,
                                    uint32_t* layers_out) {
  const dim3 grid = alpha_grid(q), block(ALPHA_BLOCK);
  const bool det = form == PT_ALPHA_FORM_GUIDE;
  if (det && first) hipLaunchKernelGGL((k_alpha_filter_closest<true, true>), grid, block, 0, s, sc, q, aq, qi, bounce, al, layers_out);
  else if (det) hipLaunchKernelGGL((k_alpha_filter_closest<true, false>), grid, block, 0, s, sc, q, aq, qi, bounce, al, layers_out);
  else if (first) hipLaunchKernelGGL((k_alpha_filter_closest<false, true>), grid, block, 0, s, sc, q, aq, qi, bounce, al, layers_out);
  else hipLaunchKernelGGL((k_alpha_filter_closest<false, false>), grid, block, 0, s, sc, q, aq, qi, bounce, al, layers_out);
}

void pt_launch_alpha_filter_shadow(hipStream_t s, const DevScene& sc, const DevQueues& q, const DevQueues& aq, const DevAlpha& al, const uint8_t* flags, bool first, float* tr_out) {
  const dim3 grid = alpha_grid(q), block(ALPHA_BLOCK);
  if (first) hipLaunchKernelGGL((k_alpha_filter_shadow<true>), grid, block, 0, s, sc, q, aq, al, flags, tr_out);
  else hipLaunchKernelGGL((k_alpha_filter_shadow<false>), grid, block, 0, s, sc, q, aq, al, flags, tr_out);
}
