// ptc_api_medium.cpp — the participating medium over the C-ABI (pt_medium.h, include/ptc_medium.h): the calls that record it, the frame's copy, the
// lanes' medium queues, the statistics and the ptc_debug_medium_* hooks.
#include "ptc_ctx.h"

#include <cmath>

using namespace ptc_detail;

namespace {
uint32_t ray_path(const float4&, const float4& C) { return __builtin_bit_cast(uint32_t, C.z); }
uint32_t shadow_path(const float4& B, const float4&) { return __builtin_bit_cast(uint32_t, B.w); }
}  // namespace

namespace ptc_detail {
const char* medium_conflict(const ptc_ctx* c, int integrator) {
  if (integrator != PTC_INTEGRATOR_PATH || !c->committed || !c->medium.set || !(c->medium.params.sigma_t > 0.0f)) return nullptr;
  // materials first (a handful): only a description that has such a material at all pays for the walk over the primitives that says whether one uses it
  bool any = false;
  for (size_t m = 0; m < c->mats.size() && !any; ++m) any = ((m < c->alpha.mode.size() && c->alpha.mode[m] != PTC_ALPHA_OPAQUE) || glass_tau(c, (int)m) > 0.0f);
  if (!any) return nullptr;
  for (const int32_t m : c->built->tri_mat) {
    if (m < 0) continue;
    if ((size_t)m < c->alpha.mode.size() && c->alpha.mode[(size_t)m] != PTC_ALPHA_OPAQUE)
      return "frame_begin: a medium is set and the committed scene has a material with alpha coverage: that pass walks several segments per bounce, which the medium "
             "does not follow yet — render without the alpha modes (ptc_render: --no-alpha) or clear the medium";
    if (glass_tau(c, m) > 0.0f)
      return "frame_begin: a medium is set and the committed scene has a transmissive material: that pass walks several segments per bounce, which the medium does "
             "not follow yet — render without transmission (ptc_render: --no-transmission) or clear the medium";
  }
  return nullptr;
}

int medium_frame_begin(ptc_ctx* c, bool on) {
  c->medium.frame_on = on && c->medium.set && c->medium.params.sigma_t > 0.0f;
  if (!c->medium.frame_on) {
    if (c->medium.counters.p) HIP_TRY(c, hipMemset(c->medium.counters.p, 0, PT_MEDIUM_COUNTERS * sizeof(unsigned long long)));
    return PTC_OK;
  }
  c->medium.frame = pt_medium_make(c->medium.params);
  { int rc = ensure_buf(c, c->medium.counters, (size_t)PT_MEDIUM_COUNTERS); if (rc) return rc; }
  HIP_TRY(c, hipMemset(c->medium.counters.p, 0, PT_MEDIUM_COUNTERS * sizeof(unsigned long long)));
  return PTC_OK;
}

int ensure_medium_queues(ptc_ctx* c) {
  bool grow = false;
  for (auto& ln : c->lanes) grow = grow || ln.medium.cap < ln.q.cap;
  if (!grow) return PTC_OK;
  { int rs = sync_all_lanes(c); if (rs) return rs; }
  for (auto& ln : c->lanes) {
    if (ln.medium.cap >= ln.q.cap) continue;
    MediumQueue& md = ln.medium;
    free_all(md.allocs);
    md.q = DevMediumQ{}; md.cap = 0;
    DevMediumQ mq{};
    const size_t slots = ptc_seg_slots(ln.q.cap, (uint32_t)c->cfg.shade_waves);      // the lane's own slot count: a segment of the batch's layout owns the same slots here
    uint32_t* segs = nullptr;
    int rc = 0;
    for (float4** a : {&mq.cont.A, &mq.cont.B, &mq.cont.C, &mq.sh.A, &mq.sh.B, &mq.sh.C, &mq.pl.A, &mq.pl.B, &mq.pl.C})
      if (!rc) rc = dev_alloc(c, md.allocs, a, slots);
    if (!rc) rc = dev_alloc(c, md.allocs, &segs, (size_t)3 * PTC_MAX_SEGMENTS);
    if (rc) { free_all(md.allocs); return rc; }
    HIP_TRY(c, hipMemset(segs, 0, (size_t)3 * PTC_MAX_SEGMENTS * sizeof(uint32_t)));
    mq.n_cont = segs; mq.n_sh = segs + PTC_MAX_SEGMENTS; mq.n_pl = segs + 2 * PTC_MAX_SEGMENTS;
    md.q = mq; md.cap = ln.q.cap;
  }
  return PTC_OK;
}
}  // namespace ptc_detail

extern "C" {
int ptc_set_medium(ptc_ctx* c, const ptc_medium_params* p) {
  if (!c) return PTC_E_ARG;
  if (!p) return fail(c, PTC_E_ARG, "set_medium: null pointer");
  if (const char* why = pt_medium_params_error(*p)) return fail(c, PTC_E_ARG, std::string("set_medium: ") + why);
  c->medium.params = *p;
  c->medium.set = true;
  return PTC_OK;
}

int ptc_get_medium(const ptc_ctx* c, ptc_medium_params* out) {
  if (!c || !out) return PTC_E_ARG;
  if (!c->medium.set) { std::memset(out, 0, sizeof *out); return 0; }
  *out = c->medium.params;
  return 1;
}

int ptc_clear_medium(ptc_ctx* c) {
  if (!c) return PTC_E_ARG;
  c->medium.set = false;
  c->medium.params = ptc_medium_params{};
  return PTC_OK;
}

int ptc_get_medium_stats(ptc_ctx* c, ptc_medium_stats* out) {
  if (!c) return PTC_E_ARG;
  if (!out) return fail(c, PTC_E_ARG, "get_medium_stats: null pointer");
  std::memset(out, 0, sizeof *out);
  if (c->device < 0) return PTC_OK;
  ptc_stats unused;
  { int rc = ptc_get_stats(c, &unused); if (rc) return rc; }      // flushes, waits and collects the timing spans
  if (c->medium.counters.p) {
    unsigned long long v[PT_MEDIUM_COUNTERS];
    HIP_TRY(c, hipMemcpy(v, c->medium.counters.p, sizeof v, hipMemcpyDeviceToHost));
    out->crossed = v[PT_MEDIUM_CROSSED]; out->scattered = v[PT_MEDIUM_SCATTERED]; out->attenuated = v[PT_MEDIUM_ATTENUATED];
  }
  out->seconds_medium = c->medium.seconds;
  return PTC_OK;
}

// ---- test hooks -------------------------------------------------------------------------------------------------------------------------------------
int ptc_debug_medium_sample(const ptc_medium_params* p, ptc_medium_sample* io) {
  if (!p || !io || pt_medium_params_error(*p)) return PTC_E_ARG;
  const pt_medium m = pt_medium_make(*p);
  const v3 o = V3(io->o), d = V3(io->d);
  float t0, t1;
  io->crosses = pt_medium_span(m, o, d, io->t_end, t0, t1) ? 1 : 0;
  io->t0 = t0; io->t1 = t1;
  io->s = 0.0f; io->scatters = 0;
  io->P[0] = io->P[1] = io->P[2] = 0.0f;
  if (io->crosses && m.sigma_t > 0.0f) {
    io->s = pt_medium_free_flight(m, t0, io->u0);
    io->scatters = io->s < t1 ? 1 : 0;
    const v3 P = vfma(d, io->s, o);
    io->P[0] = P.x; io->P[1] = P.y; io->P[2] = P.z;
  }
  const float c = pt_hg_cos(m.g, io->u1);
  const v3 wi = pt_hg_direction(d, c, io->u2);
  io->cos_theta = c;
  io->wi[0] = wi.x; io->wi[1] = wi.y; io->wi[2] = wi.z;
  io->pdf = pt_hg_phase(m.g, c);
  float s0, s1;
  io->transmittance = pt_medium_span(m, V3(io->so), V3(io->sd), io->stmax, s0, s1) ? pt_medium_transmittance(m, s0, s1) : 1.0f;
  return PTC_OK;
}

int ptc_debug_medium_env(ptc_ctx* c, const float* r1, const float* r2, const float* dir_in, uint32_t n, float* out_dir, float* out_Le, float* out_pdf) {
  if (!c) return PTC_E_ARG;
  if (!r1 || !r2 || !dir_in || !out_dir || !out_Le || !out_pdf || n == 0 || n > (1u << 24)) return fail(c, PTC_E_ARG, "debug_medium_env: bad argument");
  for (uint32_t i = 0; i < n; ++i)
    if (!(r1[i] >= 0.0f && r1[i] < 1.0f) || !(r2[i] >= 0.0f && r2[i] < 1.0f)) return fail(c, PTC_E_ARG, "debug_medium_env: a random number outside [0, 1)");
  { int rc = debug_prepare(c, 1, "debug_medium_env"); if (rc) return rc; }
  if (!c->scene.dsc.env_ok || c->scene.dsc.env_w <= 0) return fail(c, PTC_E_STATE, "debug_medium_env: the scene has no environment that can be sampled");
  DevBuf<float> in, out;
  { int rc = ensure_buf(c, in, (size_t)n * 5u); if (!rc) rc = ensure_buf(c, out, (size_t)n * 7u); if (rc) return rc; }
  HIP_TRY(c, hipMemcpy(in.p, r1, (size_t)n * 4, hipMemcpyHostToDevice));
  HIP_TRY(c, hipMemcpy(in.p + n, r2, (size_t)n * 4, hipMemcpyHostToDevice));
  HIP_TRY(c, hipMemcpy(in.p + 2 * (size_t)n, dir_in, (size_t)n * 12, hipMemcpyHostToDevice));
  const Lane& ln = c->lanes[0];
  pt_launch_medium_env(ln.stream, lane_scene(c, 0), in.p, in.p + n, in.p + 2 * (size_t)n, n, out.p);
  HIP_TRY(c, hipGetLastError());
  HIP_TRY(c, hipStreamSynchronize(ln.stream));
  std::vector<float> o((size_t)n * 7u);
  HIP_TRY(c, hipMemcpy(o.data(), out.p, o.size() * 4, hipMemcpyDeviceToHost));
  for (uint32_t i = 0; i < n; ++i) {
    std::memcpy(out_dir + (size_t)i * 3, &o[(size_t)i * 7], 12);
    std::memcpy(out_Le + (size_t)i * 3, &o[(size_t)i * 7 + 3], 12);
    out_pdf[i] = o[(size_t)i * 7 + 6];
  }
  return PTC_OK;
}

int ptc_debug_medium_step(ptc_ctx* c, const float* origins, const float* dirs, const float* throughput, const float* prev_pdf, const uint32_t* keys, uint32_t n,
                          uint32_t bounce, uint32_t max_bounces, float* out_hit, uint8_t* out_alive, float* out_cont, uint8_t* out_shadow_valid, float* out_shadow,
                          uint8_t* out_punctual_valid, float* out_punctual) {
  if (!c) return PTC_E_ARG;
  if (!origins || !dirs || !throughput || !prev_pdf || !keys || !out_hit || !out_alive || !out_cont || !out_shadow_valid || !out_shadow || !out_punctual_valid ||
      !out_punctual || n == 0 || bounce >= PT_MEDIUM_BOUNCE_LIMIT || max_bounces >= PT_MEDIUM_BOUNCE_LIMIT || bounce > max_bounces)
    return fail(c, PTC_E_ARG, "debug_medium_step: bad argument");
  for (uint32_t i = 0; i < n; ++i) {
    const float* d = dirs + (size_t)i * 3;
    bool ok = std::isfinite(prev_pdf[i]);
    for (int k = 0; k < 3; ++k) ok = ok && std::isfinite(origins[(size_t)i * 3 + k]) && std::isfinite(d[k]) && std::isfinite(throughput[(size_t)i * 3 + k]);
    const double len2 = (double)d[0] * d[0] + (double)d[1] * d[1] + (double)d[2] * d[2];
    if (!ok || !(std::fabs(std::sqrt(len2) - 1.0) <= 1e-3)) return fail(c, PTC_E_ARG, "debug_medium_step: a ray is not finite or its direction not of unit length");
  }
  if (const char* why = medium_conflict(c, PTC_INTEGRATOR_PATH)) return fail(c, PTC_E_STATE, why);
  { int rc = debug_prepare(c, n, "debug_medium_step"); if (rc) return rc; }
  if (!c->medium.set || !(c->medium.params.sigma_t > 0.0f)) return fail(c, PTC_E_STATE, "debug_medium_step: no medium (ptc_set_medium with sigma_t > 0)");
  { int rc = upload_lights(c); if (!rc) rc = medium_frame_begin(c, true); if (!rc) rc = ensure_medium_queues(c); if (rc) return rc; }
  c->medium.seconds = 0.0;
  const Lane& ln = c->lanes[0];
  { int rc = stage_rays(c, ln.q.ray[0], n, origins, dirs, [&](uint32_t i, float4& B, float4& C) {
      B.z = throughput[i * 3]; B.w = throughput[i * 3 + 1];
      C = make_float4(throughput[i * 3 + 2], prev_pdf[i], __builtin_bit_cast(float, i), __builtin_bit_cast(float, keys[i]));
    }); if (rc) return rc; }
  HIP_TRY(c, hipMemset(ln.q.lpath, 0, (size_t)n * sizeof(float4)));
  const DevQueues q = batch_queues(c, 0, n);
  const DevScene sc = lane_scene(c, 0);
  const DevMediumQ mq = dev_medium_q(c, 0);
  const LaunchCfg cfg = c->cfg;
  DevFrame fr{};
  fr.max_bounces = (int)max_bounces;
  const bool punctual = c->lights.n_dev > 0;
  pt_launch_set_counts(ln.stream, cfg, q, n, 0);
  pt_launch_trace_closest(ln.stream, cfg, sc, q, 0, false);
  pt_launch_medium_decide(ln.stream, sc, q, mq, c->medium.frame, 0, bounce, max_bounces, c->lights.recs.p, c->lights.cdf.p, c->lights.n_dev);
  pt_launch_shade(ln.stream, cfg, ln.d_scene, fr, q, 0, bounce);
  if (bounce < max_bounces) pt_launch_medium_append(ln.stream, q, mq, c->medium.frame, 0, false);
  HIP_TRY(c, hipGetLastError());
  HIP_TRY(c, hipStreamSynchronize(ln.stream));
  std::vector<float4> H(n);
  HIP_TRY(c, hipMemcpy(H.data(), ln.q.hit, n * sizeof(float4), hipMemcpyDeviceToHost));
  for (uint32_t i = 0; i < n; ++i) std::memcpy(out_hit + (size_t)i * 4, &H[i], 16);
  std::memset(out_alive, 0, n); std::memset(out_shadow_valid, 0, n); std::memset(out_punctual_valid, 0, n);
  std::memset(out_cont, 0, (size_t)n * 40); std::memset(out_shadow, 0, (size_t)n * 40); std::memset(out_punctual, 0, (size_t)n * 40);
  if (bounce == max_bounces) return PTC_OK;      // the last bounce: k_shade's counts are not meant to be read, nothing was appended
  { int rc = scatter_segment_records(c, q, q.seg_ray[1], q.ray[1], ray_path, n, "debug_medium_step", "continuation", [&](uint32_t path, const float4& A, const float4& B, const float4& C) {
      out_alive[path] = 1;
      const float r[10] = {A.x, A.y, A.z, A.w, B.x, B.y, B.z, B.w, C.x, C.y};
      std::memcpy(out_cont + (size_t)path * 10, r, sizeof r);
    }); if (rc) return rc; }
  { int rc = scatter_segment_records(c, q, q.seg_sh, as_rays(q.shadow), shadow_path, n, "debug_medium_step", "shadow", [&](uint32_t path, const float4& A, const float4& B, const float4& C) {
      out_shadow_valid[path] = 1;
      const float r[10] = {A.x, A.y, A.z, A.w, B.x, B.y, B.z, C.x, C.y, C.z};
      std::memcpy(out_shadow + (size_t)path * 10, r, sizeof r);
    }); if (rc) return rc; }
  if (!punctual) return PTC_OK;
  pt_launch_shade_punctual(ln.stream, sc, q, 0, bounce, c->lights.recs.p, c->lights.cdf.p, c->lights.n_dev);
  pt_launch_medium_append(ln.stream, q, mq, c->medium.frame, 0, true);
  HIP_TRY(c, hipGetLastError());
  HIP_TRY(c, hipStreamSynchronize(ln.stream));
  return scatter_segment_records(c, q, q.seg_sh, as_rays(q.shadow), shadow_path, n, "debug_medium_step", "punctual shadow", [&](uint32_t path, const float4& A, const float4& B, const float4& C) {
    out_punctual_valid[path] = 1;
    const float r[10] = {A.x, A.y, A.z, A.w, B.x, B.y, B.z, C.x, C.y, C.z};
    std::memcpy(out_punctual + (size_t)path * 10, r, sizeof r);
  });
}
}  // extern "C"
