// pt_medium.hip — the participating-medium pass (see pt_medium.h).
//
//   k_medium_decide(b)      between closest(b) and shade(b), over the live slots of ray[qi] and their hit records.  Per ray: the span and the free flight; for a scatter
//                           event the phase sample, Russian roulette and next-event estimation — an emitter or environment record and, when the frame has punctual lights,
//                           a punctual record — all parked at the front of the ray's own segment of the medium queue; the ray's hit record becomes the miss record and
//                           its T zero, so k_shade(b) does nothing for it.  A ray that stands costs the load of its ray and hit records and nothing else.
//   k_medium_append<0>(b)   behind shade(b), before the scan: per segment the parked continuations go behind the records k_shade wrote to ray[qi ^ 1], the parked emitter /
//                           environment shadow records behind k_shade's in q.shadow, both counts are raised, and then EVERY shadow record of the segment is attenuated.
//                           A segment cannot overflow: k_shade wrote nothing for the rays the medium took (the copies are bounded by seg_len all the same).
//   k_medium_append<1>(b)   behind k_shade_punctual(b), before its scan: the same for the parked punctual records and the punctual pass's own.
// Layout: the per-segment pass of pt_pass_common.h, into the three medium queues; counters added once per wave.
#include "pt_walk_surfaces.h"
#include "pt_medium.h"

namespace {
// ---- the environment: k_shade's env_lookup, cdf_search_guided and env_sample (pt_kernels.hip, whose text is hashed and so cannot be shared), line for line,
// over the scene's arrays in global memory ----
PT_DEV void medium_env_lookup(const DevScene& sc, v3 d, v3& Le, float& pdf) {
  const float u = pt_atan2(d.z, d.x) * (0.5f * PT_INV_PI) + 0.5f;
  const float dy = fmin2(fmax2(d.y, -1.0f), 1.0f);
  const float st = pt_sqrt(fmax2(0.0f, 1.0f - dy * dy));
  const float vv = pt_atan2(st, dy) * PT_INV_PI;
  int x = (int)(u * (float)sc.env_w), y = (int)(vv * (float)sc.env_h);
  if (x > sc.env_w - 1) x = sc.env_w - 1;
  if (x < 0) x = 0;
  if (y > sc.env_h - 1) y = sc.env_h - 1;
  if (y < 0) y = 0;
  const float4 t = ld4(sc.env, (size_t)y * (size_t)sc.env_w + (size_t)x);
  Le = V3(t.x, t.y, t.z);
  pdf = sc.env_ok ? (t.w * (float)sc.env_w * (float)sc.env_h) / (2.0f * PT_PI * PT_PI * fmax2(st, 1e-6f)) : 0.0f;
}
template <class P, class G> PT_DEV uint32_t medium_cdf_search_guided(const P& cdf, const G& guide, float r) {
  const uint32_t b = (uint32_t)(r * (float)PTC_ENV_GUIDE);
  uint32_t lo = guide[b], hi = guide[b + 1u];
  while (lo < hi) { const uint32_t mid = (lo + hi) >> 1; if (cdf[mid] > r) hi = mid; else lo = mid + 1u; }
  return lo;
}
PT_DEV v3 medium_env_sample(const DevScene& sc, float r1, float r2) {
  const float* marg = sc.env_marg;
  const uint32_t y = medium_cdf_search_guided(marg, sc.env_marg_guide, r1);
  const float m0 = y ? marg[y - 1u] : 0.0f, m1 = marg[y];
  float xi_v = m1 > m0 ? (r1 - m0) / (m1 - m0) : 0.5f;
  const auto cc = sc.env_cond + (size_t)y * (size_t)sc.env_w;
  const uint32_t x = medium_cdf_search_guided(cc, sc.env_cond_guide + (size_t)y * (PTC_ENV_GUIDE + 1u), r2);
  const float c0 = x ? cc[x - 1u] : 0.0f, c1 = cc[x];
  float xi_u = c1 > c0 ? (r2 - c0) / (c1 - c0) : 0.5f;
  xi_u = fmin2(fmax2(xi_u, 0.0f), 0.999999f); xi_v = fmin2(fmax2(xi_v, 0.0f), 0.999999f);
  const float u = ((float)x + xi_u) / (float)sc.env_w, vv = ((float)y + xi_v) / (float)sc.env_h;
  float s2, c2, st, ct;
  sincos2pi(u, s2, c2);             // phi = 2 pi u - pi: cos phi = -cos(2 pi u), sin phi = -sin(2 pi u)
  sincos2pi(0.5f * vv, st, ct);     // theta = pi v
  return V3(st * -c2, ct, st * -s2);
}

__global__ __launch_bounds__(WALK_BLOCK) void k_medium_decide(DevScene sc, DevQueues q, DevMediumQ mq, pt_medium med, int qi, uint32_t b, uint32_t max_bounces,
                                                            const float4* __restrict__ lights, const float* __restrict__ cdf, uint32_t n_punctual) {
  __shared__ float4 s_light[PT_LIGHTS_MAX * 4];
  __shared__ float s_cdf[PT_LIGHTS_MAX];
  if (n_punctual) stage_light_table(s_light, s_cdf, lights, cdf, n_punctual);      // uniform over the grid
  const uint32_t lane = lane_id();
  const WaveSegment w = wave_segment(q);
  if (!w.owned) return;
  const RayQ rin = q.ray[qi];
  const uint32_t base = w.base(q), n = w.count(q.seg_ray[qi]);
  // light-kind selection probabilities for NEE: k_shade's
  const bool has_env = sc.env_w > 0, env_nee = has_env && sc.env_ok != 0;
  const float p_env = env_nee ? (sc.n_lights > 0u ? 0.5f : 1.0f) : 0.0f, p_area = 1.0f - p_env;
  const uint32_t idx = PT_MEDIUM_RNG_BASE + b + 1u;
  uint32_t out_c = 0, out_s = 0, out_p = 0;                    // wave cursors: parked continuations / shadow records / punctual records
  unsigned long long n_cross = 0, n_scat = 0;
  for (uint32_t i0 = 0; i0 < n; i0 += 64u) {
    const bool valid = i0 + lane < n;
    const uint32_t slot = base + i0 + lane;
    bool crossed = false, scattered = false, alive = false, has_s = false, has_p = false;
    float4 oA, oB, oC, sA, sB, sC, pA, pB, pC;
    oA = oB = oC = sA = sB = sC = pA = pB = pC = make_float4(0, 0, 0, 0);
    if (valid) {
      const float4 A = rin.A[slot], Bq = rin.B[slot], Cq = rin.C[slot], H = q.hit[slot];
      const v3 o = V3(A.x, A.y, A.z), d = V3(A.w, Bq.x, Bq.y);
      const float t_end = __float_as_int(H.y) < 0 ? PT_T_INF : H.x;
      float t0, t1;
      crossed = pt_medium_span(med, o, d, t_end, t0, t1);
      if (crossed) {
        const uint32_t path = __float_as_uint(Cq.z), key = __float_as_uint(Cq.w);
        const float s = pt_medium_free_flight(med, t0, rng_f(key, idx, 0));
        scattered = s < t1;
        if (scattered) {
          // ---- 3: the ray leaves k_shade alone ----
          q.hit[slot] = make_float4(-1.0f, __int_as_float(-1), 0.0f, 0.0f);
          rin.B[slot] = make_float4(Bq.x, Bq.y, 0.0f, 0.0f);
          rin.C[slot] = make_float4(0.0f, Cq.y, Cq.z, Cq.w);
          const v3 P = vfma(d, s, o);
          v3 T = V3(Bq.z * med.albedo[0], Bq.w * med.albedo[1], Cq.x * med.albedo[2]);
          if (b < max_bounces && max3c(T) > 0.0f) {
            // ---- 5: next-event estimation at P, with the throughput before roulette ----
            const bool use_env = env_nee && (sc.n_lights == 0u || rng_f(key, idx, 4) < p_env);
            if (use_env) {
              const v3 wi = medium_env_sample(sc, rng_f(key, idx, 6), rng_f(key, idx, 7));
              v3 Le; float pe; medium_env_lookup(sc, wi, Le, pe);
              const float pl = pe * p_env;
              if (pl > 0.0f) {
                const float ph = pt_hg_phase(med.g, dot3(d, wi));
                const float pl2 = pl * pl;
                const float wgt = pl2 / pt_fma(ph, ph, pl2);
                const float k = (ph * wgt) / pl;
                has_s = true;
                sA = make_float4(P.x, P.y, P.z, wi.x);
                sB = make_float4(wi.y, wi.z, PT_T_INF, __uint_as_float(path));
                sC = make_float4(T.x * Le.x * k, T.y * Le.y * k, T.z * Le.z * k, 0.0f);
              }
            } else if (sc.n_lights > 0u) {
              const float u = rng_f(key, idx, 5), r1 = rng_f(key, idx, 6), r2 = rng_f(key, idx, 7);
              const uint32_t lo = cdf_search(sc.cdf, sc.n_lights, u);
              const float4 l0 = sc.lights[lo * 5u], l1 = sc.lights[lo * 5u + 1u], l2 = sc.lights[lo * 5u + 2u], l3 = sc.lights[lo * 5u + 3u], l4 = sc.lights[lo * 5u + 4u];
              const float su = pt_sqrt(r1);
              const float bu = su * (1.0f - r2), bv = su * r2;
              const v3 y = vfma(V3(l2.x, l2.y, l2.z), bv, vfma(V3(l1.x, l1.y, l1.z), bu, V3(l0.x, l0.y, l0.z)));
              const v3 dv = y - P;
              const float dist2 = dot3(dv, dv);
              if (dist2 > 0.0f) {
                float dist;
                const v3 wi = dv * pt_rnorm(dist2, dist);
                const float cosl = -dot3(V3(l3.x, l3.y, l3.z), wi);
                if (cosl > 0.0f) {
                  const float pl = ((l1.w * dist2) / (l0.w * cosl)) * p_area;
                  const float ph = pt_hg_phase(med.g, dot3(d, wi));
                  const float pl2 = pl * pl;
                  const float wgt = pl2 / pt_fma(ph, ph, pl2);
                  const float k = (ph * wgt) / pl;
                  has_s = true;
                  sA = make_float4(P.x, P.y, P.z, wi.x);
                  sB = make_float4(wi.y, wi.z, dist * 0.999f, __uint_as_float(path));
                  sC = make_float4(T.x * l4.x * k, T.y * l4.y * k, T.z * l4.z * k, 0.0f);
                }
              }
            }
            if (n_punctual) {
              const uint32_t li = cdf_search(s_cdf, n_punctual, rng_f(key, PT_MEDIUM_RNG_PUNCTUAL + b + 1u, 0));
              const float4 l0 = s_light[li * 4u], l1 = s_light[li * 4u + 1u], l2 = s_light[li * 4u + 2u], l3 = s_light[li * 4u + 3u];
              pt_light_rec L;      // load_light_rec's text (pt_pass_common.h), kept here: through the helper the index arithmetic compiles differently
              L.pos[0] = l0.x; L.pos[1] = l0.y; L.pos[2] = l0.z; L.type = __float_as_int(l0.w);
              L.dir[0] = l1.x; L.dir[1] = l1.y; L.dir[2] = l1.z; L.range = l1.w;
              L.I[0] = l2.x; L.I[1] = l2.y; L.I[2] = l2.z; L.pmf = l2.w;
              L.scale = l3.x; L.offset = l3.y; L.cos_inner = l3.z; L.cos_outer = l3.w;
              v3 wi, Li;
              float dist;
              if (pt_light_sample(L, P, wi, dist, Li) && (Li.x > 0.0f || Li.y > 0.0f || Li.z > 0.0f)) {
                const float k = pt_hg_phase(med.g, dot3(d, wi)) / L.pmf;
                v3 sdir; float tmax;
                punctual_segment(L, P, wi, sdir, tmax);
                has_p = true;
                pA = make_float4(P.x, P.y, P.z, sdir.x);
                pB = make_float4(sdir.y, sdir.z, tmax, __uint_as_float(path));
                pC = make_float4(T.x * Li.x * k, T.y * Li.y * k, T.z * Li.z * k, 0.0f);
              }
            }
            // ---- 4: the phase sample and roulette ----
            const float c = pt_hg_cos(med.g, rng_f(key, idx, 1));
            const v3 wi = pt_hg_direction(d, c, rng_f(key, idx, 2));
            const float pdf = pt_hg_phase(med.g, c);
            alive = pt_medium_roulette(b + 1u, rng_f(key, idx, 3), T);
            if (alive) {
              oA = make_float4(P.x, P.y, P.z, wi.x);
              oB = make_float4(wi.y, wi.z, T.x, T.y);
              oC = make_float4(T.z, pdf, __uint_as_float(path), __uint_as_float(key));
            }
          }
        }
      }
    }
    // ---- compaction into the wave's own segment of the medium queue ----
    // the kernel's own text, not three put_compacted: the three ballots are taken first, then the stores, then the advances.  One compaction after the other is
    // other machine code, and the fog frame at 64 spp came out above the parent's range with it (profiles/pass_common.txt)
    const uint64_t mc = __ballot(alive), ms = __ballot(has_s), mp = __ballot(has_p);
    if (alive) { const uint32_t at = base + out_c + mbcnt64(mc); mq.cont.A[at] = oA; mq.cont.B[at] = oB; mq.cont.C[at] = oC; }
    if (has_s) { const uint32_t at = base + out_s + mbcnt64(ms); mq.sh.A[at] = sA; mq.sh.B[at] = sB; mq.sh.C[at] = sC; }
    if (has_p) { const uint32_t at = base + out_p + mbcnt64(mp); mq.pl.A[at] = pA; mq.pl.B[at] = pB; mq.pl.C[at] = pC; }
    out_c += (uint32_t)__popcll(mc); out_s += (uint32_t)__popcll(ms); out_p += (uint32_t)__popcll(mp);
    n_cross += (unsigned long long)__popcll(__ballot(crossed));
    n_scat += (unsigned long long)__popcll(__ballot(scattered));
  }
  if (lane == 0) { mq.n_cont[w.seg] = out_c; mq.n_sh[w.seg] = out_s; mq.n_pl[w.seg] = out_p; }
  wave_count(&mq.counters[PT_MEDIUM_CROSSED], n_cross, lane);
  wave_count(&mq.counters[PT_MEDIUM_SCATTERED], n_scat, lane);
}

// ptc_debug_medium_env: the two texts above on their own — per item the sample of (r1, r2) and the lookup of dir_in, seven floats (wi, Le, pdf)
__global__ __launch_bounds__(256) void k_medium_env(DevScene sc, const float* __restrict__ r1, const float* __restrict__ r2, const float* __restrict__ din, uint32_t n,
                                                   float* __restrict__ out) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  const v3 wi = medium_env_sample(sc, r1[i], r2[i]);
  v3 Le; float pdf;
  medium_env_lookup(sc, V3(din[i * 3u], din[i * 3u + 1u], din[i * 3u + 2u]), Le, pdf);
  float* o = out + (size_t)i * 7u;
  o[0] = wi.x; o[1] = wi.y; o[2] = wi.z; o[3] = Le.x; o[4] = Le.y; o[5] = Le.z; o[6] = pdf;
}

// `n_src` records from the front of the segment of src go behind the `have` records of dst; returns the new count (never above seg_len)
PT_DEV uint32_t append_records(const float4* sA, const float4* sB, const float4* sC, float4* dA, float4* dB, float4* dC, uint32_t base, uint32_t have, uint32_t n_src,
                               uint32_t seg_len, uint32_t lane) {
  if (have > seg_len) have = seg_len;
  if (n_src > seg_len - have) n_src = seg_len - have;
  for (uint32_t i0 = 0; i0 < n_src; i0 += 64u) {
    const uint32_t i = i0 + lane;
    if (i < n_src) { dA[base + have + i] = sA[base + i]; dB[base + have + i] = sB[base + i]; dC[base + have + i] = sC[base + i]; }
  }
  return have + n_src;
}

template <int PUNCTUAL>
__global__ __launch_bounds__(WALK_BLOCK) void k_medium_append(DevQueues q, DevMediumQ mq, pt_medium med, int qi) {
  const uint32_t lane = lane_id();
  const WaveSegment w = wave_segment(q);
  if (!w.owned) return;
  const uint32_t seg = w.seg, base = w.base(q);
  if (!PUNCTUAL) {
    const RayQ rout = q.ray[qi ^ 1];
    const uint32_t have = w.count(q.seg_ray[qi ^ 1]), parked = w.count(mq.n_cont);
    const uint32_t total = append_records(mq.cont.A, mq.cont.B, mq.cont.C, rout.A, rout.B, rout.C, base, have, parked, q.seg_len, lane);
    if (lane == 0 && parked) q.seg_ray[qi ^ 1][seg] = total;
  }
  // ---- 6 and the shadow records: every lane reads only what an earlier kernel wrote and writes each word once — the pass's own records (k_shade's, or
  // k_shade_punctual's) are attenuated in place, the parked ones on their way behind them ----
  const ShadowQ src = PUNCTUAL ? mq.pl : mq.sh;
  uint32_t have = w.count(q.seg_sh), parked = w.count(PUNCTUAL ? mq.n_pl : mq.n_sh);
  if (have > q.seg_len) have = q.seg_len;
  if (parked > q.seg_len - have) parked = q.seg_len - have;
  unsigned long long n_att = 0;
  for (uint32_t i0 = 0; i0 < have; i0 += 64u) {
    const uint32_t at = base + i0 + lane;
    bool att = false;
    if (i0 + lane < have) {
      const float4 A = q.shadow.A[at], Bq = q.shadow.B[at];
      float t0, t1;
      att = pt_medium_span(med, V3(A.x, A.y, A.z), V3(A.w, Bq.x, Bq.y), Bq.z, t0, t1);
      if (att) {
        const float4 Cq = q.shadow.C[at];
        const float tr = pt_medium_transmittance(med, t0, t1);
        q.shadow.C[at] = make_float4(Cq.x * tr, Cq.y * tr, Cq.z * tr, Cq.w);
      }
    }
    n_att += (unsigned long long)__popcll(__ballot(att));
  }
  for (uint32_t i0 = 0; i0 < parked; i0 += 64u) {
    const uint32_t i = i0 + lane;
    bool att = false;
    if (i < parked) {
      const float4 A = src.A[base + i], Bq = src.B[base + i];
      float4 Cq = src.C[base + i];
      float t0, t1;
      att = pt_medium_span(med, V3(A.x, A.y, A.z), V3(A.w, Bq.x, Bq.y), Bq.z, t0, t1);
      if (att) {
        const float tr = pt_medium_transmittance(med, t0, t1);
        Cq = make_float4(Cq.x * tr, Cq.y * tr, Cq.z * tr, Cq.w);
      }
      const uint32_t at = base + have + i;
      q.shadow.A[at] = A; q.shadow.B[at] = Bq; q.shadow.C[at] = Cq;
    }
    n_att += (unsigned long long)__popcll(__ballot(att));
  }
  if (lane == 0 && parked) q.seg_sh[seg] = have + parked;
  wave_count(&mq.counters[PT_MEDIUM_ATTENUATED], n_att, lane);
}
}  // namespace

void pt_launch_medium_decide(hipStream_t s, const DevScene& sc, const DevQueues& q, const DevMediumQ& mq, const pt_medium& med, int qi, uint32_t bounce, uint32_t max_bounces,
                             const pt_light_rec* lights, const float* cdf, uint32_t n_punctual) {
  if (n_punctual > PT_LIGHTS_MAX) return;
  hipLaunchKernelGGL(k_medium_decide, walk_grid(q), dim3(WALK_BLOCK), 0, s, sc, q, mq, med, qi, bounce, max_bounces, (const float4*)lights, cdf, n_punctual);
}

void pt_launch_medium_append(hipStream_t s, const DevQueues& q, const DevMediumQ& mq, const pt_medium& med, int qi, bool punctual) {
  if (punctual) hipLaunchKernelGGL(k_medium_append<1>, walk_grid(q), dim3(WALK_BLOCK), 0, s, q, mq, med, qi);
  else hipLaunchKernelGGL(k_medium_append<0>, walk_grid(q), dim3(WALK_BLOCK), 0, s, q, mq, med, qi);
}

void pt_launch_medium_env(hipStream_t s, const DevScene& sc, const float* r1, const float* r2, const float* dir_in, uint32_t n, float* out7) {
  hipLaunchKernelGGL(k_medium_env, dim3((n + 255u) / 256u), dim3(256), 0, s, sc, r1, r2, dir_in, n, out7);
}
