// ptc_api_debug.cpp — the ptc_debug_* hooks: what the tests use to look inside the library (single rays, tables, the host build, the host halves of the device paths).
#include "ptc_ctx.h"
#include "pt_exact_debug.h"

using namespace ptc_detail;

namespace {
// what the two probe hooks need of debug_prepare: a device, idle lanes, the frame ended, lane 0's queues for n paths.  No scene: neither kernel reads one.
int probe_debug_prepare(ptc_ctx* c, uint32_t n) {
  { int rd = need_device(c); if (rd) return rd; }
  { int rf = flush(c); if (rf) return rf; }
  { int rs = sync_all_lanes(c); if (rs) return rs; }
  c->in_frame = false; c->pending = 0; drop_guides(c);
  return ensure_lane_queues(c, n);
}
// which path a record belongs to: a shadow record says so in B.w, a ray record in C.z
uint32_t shadow_path(const float4& B, const float4&) { return __builtin_bit_cast(uint32_t, B.w); }
uint32_t ray_path(const float4&, const float4& C) { return __builtin_bit_cast(uint32_t, C.z); }
bool probe_debug_args_bad(int n, uint32_t base, uint32_t first_sample, uint32_t n_samples) {
  return n < 1 || n > PTC_MAX_PROBES || n_samples == 0 || (uint64_t)n * (uint64_t)n_samples > 0x7fffffffull || (uint64_t)first_sample + n_samples > 0x100000000ull ||
         (uint64_t)base + (uint64_t)n > 0x100000000ull;
}

}  // namespace

namespace ptc_detail {
// The debug getters read the host build: after a refit on the device its vertex-dependent arrays come back from HBM first.
int refresh_host_copy(ptc_ctx* c) {
  if (!c->scene.host_stale || c->device < 0) return PTC_OK;
  HIP_TRY(c, hipSetDevice(c->device));
  { int rs = sync_all_lanes(c); if (rs) return rs; }
  HostBuilt& B = *c->built;
  B.recs.resize((size_t)B.n_units * 4);                                     // a tree or a commit made on the device left the host arrays unsized
  B.shade.resize((size_t)B.n_tris * B.shade_stride * 4);
  B.wverts.resize(B.n_wverts);
  HIP_TRY(c, hipMemcpy(B.recs.data(), c->scene.dsc.recs, B.recs.size() * 4, hipMemcpyDeviceToHost));
  HIP_TRY(c, hipMemcpy(B.shade.data(), c->scene.dsc.shade, B.shade.size() * 4, hipMemcpyDeviceToHost));
  HIP_TRY(c, hipMemcpy(B.wverts.data(), c->scene.drf.wverts, B.wverts.size() * sizeof(HostVertex), hipMemcpyDeviceToHost));
  c->scene.host_stale = false;
  return PTC_OK;
}

int debug_prepare(ptc_ctx* c, uint32_t n, const char* who, DebugFeatures features) {
  { int rd = need_device(c); if (rd) return rd; }
  if (!c->committed) return fail(c, PTC_E_STATE, std::string(who) + ": scene not committed");
  { int rf = flush(c); if (rf) return rf; }
  { int rs = sync_all_lanes(c); if (rs) return rs; }
  c->in_frame = false; c->pending = 0; drop_guides(c);
  int rc = ensure_lane_queues(c, n);
  if (rc) return rc;
  for (auto& ln : c->lanes) HIP_TRY(c, hipMemset(ln.q.stats, 0, ST_N * ST_STRIDE * sizeof(unsigned long long)));
  if (features == DebugPlain) return PTC_OK;
  const bool glass = features == DebugAlphaGlass;
  if ((rc = alpha_upload(c))) return rc;
  if (glass && (rc = glass_upload(c))) return rc;
  c->alpha.seconds = 0.0; c->alpha.frame_layers = c->alpha.max_layers;
  if (glass) { c->glass.seconds = 0.0; c->glass.frame_interactions = c->glass.max_interactions; c->glass.frame_shadows = c->glass.shadows; }
  if (alpha_on(c)) {
    if ((rc = ensure_alpha_queues(c))) return rc;
    HIP_TRY(c, hipMemset(c->alpha.counters.p, 0, PT_ALPHA_COUNTERS * sizeof(unsigned long long)));
  }
  if (glass && glass_on(c)) {
    if ((rc = ensure_glass_queues(c))) return rc;
    HIP_TRY(c, hipMemset(c->glass.counters.p, 0, PT_GLASS_COUNTERS * sizeof(unsigned long long)));
    HIP_TRY(c, hipMemset(c->glass.shadow_counters.p, 0, PT_GLASS_SHADOW_COUNTERS * sizeof(unsigned long long)));
  }
  return PTC_OK;
}

int stage_rays(ptc_ctx* c, const RayQ& rq, uint32_t n, const float* origins, const float* dirs, const RayFill& fill) {
  std::vector<float4> A(n), B(n), C(n, make_float4(0, 0, 0, 0));
  for (uint32_t i = 0; i < n; ++i) {
    A[i] = make_float4(origins[i * 3], origins[i * 3 + 1], origins[i * 3 + 2], dirs[i * 3]);
    B[i] = make_float4(dirs[i * 3 + 1], dirs[i * 3 + 2], 0.0f, 0.0f);
    fill(i, B[i], C[i]);
  }
  HIP_TRY(c, hipMemcpy(rq.A, A.data(), n * sizeof(float4), hipMemcpyHostToDevice));
  HIP_TRY(c, hipMemcpy(rq.B, B.data(), n * sizeof(float4), hipMemcpyHostToDevice));
  HIP_TRY(c, hipMemcpy(rq.C, C.data(), n * sizeof(float4), hipMemcpyHostToDevice));
  return PTC_OK;
}

int read_hits(ptc_ctx* c, uint32_t n, float* out_t, int32_t* out_prim, float* out_uv) {
  std::vector<float4> H(n);
  HIP_TRY(c, hipMemcpy(H.data(), c->lanes[0].q.hit, n * sizeof(float4), hipMemcpyDeviceToHost));
  for (uint32_t i = 0; i < n; ++i) {
    int32_t pc; std::memcpy(&pc, &H[i].y, 4);   // prim | class<<28, or -1
    out_t[i] = H[i].x; out_prim[i] = pc < 0 ? -1 : (pc & 0x0fffffff); out_uv[i * 2] = H[i].z; out_uv[i * 2 + 1] = H[i].w;
  }
  return PTC_OK;
}

int scatter_segment_records(ptc_ctx* c, const DevQueues& q, const uint32_t* seg_counts, const RayQ& rq, uint32_t (*path_of)(const float4& B, const float4& C), uint32_t n,
                            const char* who, const char* what, const RecordSink& sink) {
  std::vector<uint32_t> count(q.n_seg);
  HIP_TRY(c, hipMemcpy(count.data(), seg_counts, (size_t)q.n_seg * 4, hipMemcpyDeviceToHost));
  const size_t slots = (size_t)q.n_seg * q.seg_len;
  std::vector<float4> A(slots), B(slots), C(slots);
  HIP_TRY(c, hipMemcpy(A.data(), rq.A, slots * sizeof(float4), hipMemcpyDeviceToHost));
  HIP_TRY(c, hipMemcpy(B.data(), rq.B, slots * sizeof(float4), hipMemcpyDeviceToHost));
  HIP_TRY(c, hipMemcpy(C.data(), rq.C, slots * sizeof(float4), hipMemcpyDeviceToHost));
  std::vector<uint8_t> taken(n, 0);
  for (uint32_t sg = 0; sg < q.n_seg; ++sg) {
    if (count[sg] > q.seg_len) return fail(c, PTC_E_DEVICE, std::string(who) + ": a segment holds more " + what + " records than slots");
    for (uint32_t k = 0; k < count[sg]; ++k) {
      const size_t at = (size_t)sg * q.seg_len + k;
      const uint32_t path = path_of(B[at], C[at]);
      if (path >= n || taken[path]) return fail(c, PTC_E_DEVICE, std::string(who) + ": a " + what + " record carries a path id that is out of range or taken");
      taken[path] = 1;
      sink(path, A[at], B[at], C[at]);
    }
  }
  return PTC_OK;
}
}  // namespace ptc_detail

extern "C" {
// ---- test hooks -----------------------------------------------------------------------------------
int ptc_debug_trace_closest(ptc_ctx* c, const float* origins, const float* dirs, uint32_t n, float* out_t, int32_t* out_prim, float* out_uv) {
  if (!c) return PTC_E_ARG;
  if (c->device >= 0 && (!origins || !dirs || !out_t || !out_prim || !out_uv || n == 0)) return fail(c, PTC_E_ARG, "debug_trace_closest: bad argument");
  { int rc = debug_prepare(c, n, "debug_trace_closest"); if (rc) return rc; }
  const Lane& ln = c->lanes[0];
  { int rc = stage_rays(c, ln.q.ray[0], n, origins, dirs, [](uint32_t, float4&, float4&) {}); if (rc) return rc; }
  const DevQueues q = batch_queues(c, 0, n);
  pt_launch_set_counts(ln.stream, c->cfg, q, n, 0);
  pt_launch_trace_closest(ln.stream, c->cfg, lane_scene(c, 0), q, 0, false);
  HIP_TRY(c, hipGetLastError());
  HIP_TRY(c, hipStreamSynchronize(ln.stream));
  return read_hits(c, n, out_t, out_prim, out_uv);
}

int ptc_debug_trace_any(ptc_ctx* c, const float* origins, const float* dirs, const float* tmax, uint32_t n, uint8_t* out_occluded) {
  if (!c) return PTC_E_ARG;
  if (c->device >= 0 && (!origins || !dirs || !tmax || !out_occluded || n == 0)) return fail(c, PTC_E_ARG, "debug_trace_any: bad argument");
  { int rc = debug_prepare(c, n, "debug_trace_any"); if (rc) return rc; }
  const Lane& ln = c->lanes[0];
  { int rc = stage_rays(c, as_rays(ln.q.shadow), n, origins, dirs, [&](uint32_t i, float4& B, float4&) { B.z = tmax[i]; }); if (rc) return rc; }
  DevBuf<uint8_t> occ;
  { int rc = ensure_buf(c, occ, n); if (rc) return rc; }
  const DevQueues q = batch_queues(c, 0, n);
  pt_launch_set_counts(ln.stream, c->cfg, q, 0, n);
  pt_launch_trace_any(ln.stream, c->cfg, lane_scene(c, 0), q, occ.p);
  HIP_TRY(c, hipGetLastError());
  HIP_TRY(c, hipStreamSynchronize(ln.stream));
  HIP_TRY(c, hipMemcpy(out_occluded, occ.p, n, hipMemcpyDeviceToHost));
  return PTC_OK;
}

int ptc_debug_lens_sample(const ptc_lens_params* lens, float u1, float u2, float out_xy[2]) {
  if (!lens || !out_xy || lens_params_error(*lens) || !(u1 >= 0.0f && u1 < 1.0f) || !(u2 >= 0.0f && u2 < 1.0f)) return PTC_E_ARG;
  pt_lens_point(*lens, u1, u2, out_xy[0], out_xy[1]);
  return PTC_OK;
}

int ptc_debug_light_sample(const ptc_light_params* params, const float P[3], float out_wi[3], float* out_dist, float out_Li[3]) {
  if (!params || !P || !out_wi || !out_dist || !out_Li || pt_light_params_error(*params)) return PTC_E_ARG;
  ptc_light_params p = *params;
  pt_light_normalise(p);
  const pt_light_rec L = pt_light_make_rec(p, 1.0f);
  v3 wi, Li;
  if (!pt_light_sample(L, V3(P), wi, *out_dist, Li)) return 0;
  out_wi[0] = wi.x; out_wi[1] = wi.y; out_wi[2] = wi.z;
  out_Li[0] = Li.x; out_Li[1] = Li.y; out_Li[2] = Li.z;
  return 1;
}

int ptc_debug_get_light_table(ptc_ctx* c, uint32_t* n_lights, float* records, float* cdf) {
  if (!c) return PTC_E_ARG;
  std::vector<pt_light_rec> recs; std::vector<float> cd;
  pt_light_table(c->lights.list, recs, cd);
  if (n_lights) *n_lights = (uint32_t)recs.size();
  if (records && !recs.empty()) std::memcpy(records, recs.data(), recs.size() * sizeof(pt_light_rec));
  if (cdf && !cd.empty()) std::memcpy(cdf, cd.data(), cd.size() * sizeof(float));
  return PTC_OK;
}

int ptc_debug_punctual_nee(ptc_ctx* c, const float* origins, const float* dirs, const uint32_t* keys, uint32_t n, uint32_t bounce,
                           uint8_t* out_valid, float* out_origin, float* out_dir, float* out_tmax, float* out_contrib) {
  if (!c) return PTC_E_ARG;
  if (c->device >= 0 && (!origins || !dirs || !keys || !out_valid || !out_origin || !out_dir || !out_tmax || !out_contrib || n == 0 || bounce > 0x0fffffffu))
    return fail(c, PTC_E_ARG, "debug_punctual_nee: bad argument");
  { int rc = debug_prepare(c, n, "debug_punctual_nee"); if (rc) return rc; }
  if (c->lights.list.empty()) return fail(c, PTC_E_STATE, "debug_punctual_nee: no punctual light (ptc_add_light)");
  { int rc = upload_lights(c); if (rc) return rc; }
  const Lane& ln = c->lanes[0];
  { int rc = stage_rays(c, ln.q.ray[0], n, origins, dirs, [&](uint32_t i, float4& B, float4& C) {
      B.z = B.w = 1.0f; C = make_float4(1.0f, 0.0f, __builtin_bit_cast(float, i), __builtin_bit_cast(float, keys[i]));
    }); if (rc) return rc; }
  const DevQueues q = batch_queues(c, 0, n);
  const DevScene sc = lane_scene(c, 0);
  pt_launch_set_counts(ln.stream, c->cfg, q, n, 0);
  pt_launch_trace_closest(ln.stream, c->cfg, sc, q, 0, false);
  pt_launch_shade_punctual(ln.stream, sc, q, 0, bounce, c->lights.recs.p, c->lights.cdf.p, c->lights.n_dev);
  HIP_TRY(c, hipGetLastError());
  HIP_TRY(c, hipStreamSynchronize(ln.stream));
  std::memset(out_valid, 0, n);
  std::memset(out_origin, 0, (size_t)n * 12); std::memset(out_dir, 0, (size_t)n * 12); std::memset(out_tmax, 0, (size_t)n * 4); std::memset(out_contrib, 0, (size_t)n * 12);
  return scatter_segment_records(c, q, q.seg_sh, as_rays(q.shadow), shadow_path, n, "debug_punctual_nee", "shadow", [&](uint32_t path, const float4& A, const float4& B, const float4& C) {
    out_valid[path] = 1;
    out_origin[path * 3] = A.x; out_origin[path * 3 + 1] = A.y; out_origin[path * 3 + 2] = A.z;
    out_dir[path * 3] = A.w; out_dir[path * 3 + 1] = B.x; out_dir[path * 3 + 2] = B.y;
    out_tmax[path] = B.z;
    out_contrib[path * 3] = C.x; out_contrib[path * 3 + 1] = C.y; out_contrib[path * 3 + 2] = C.z;
  });
}

// One k_shade step of explicit rays (include/ptc_shade_debug.h).  The kernel variant is chosen through a copy of the launch configuration, so the launcher and
// the kernels are the frame's.
int ptc_debug_shade_step(ptc_ctx* c, const float* origins, const float* dirs, const float* throughput, const float* prev_pdf, const uint32_t* keys, uint32_t n,
                         uint32_t bounce, uint32_t max_bounces, int variant, float* out_hit, float* out_lpath, uint8_t* out_alive, float* out_cont,
                         uint8_t* out_shadow_valid, float* out_shadow) {
  if (!c) return PTC_E_ARG;
  if (!origins || !dirs || !throughput || !prev_pdf || !keys || !out_hit || !out_lpath || !out_alive || !out_cont || !out_shadow_valid || !out_shadow || n == 0 ||
      bounce > (1u << 20) || max_bounces > (1u << 20) || variant < 0 || variant > 2)
    return fail(c, PTC_E_ARG, "debug_shade_step: bad argument");
  for (uint32_t i = 0; i < n; ++i) {
    const float* d = dirs + (size_t)i * 3;
    bool ok = std::isfinite(prev_pdf[i]);
    for (int k = 0; k < 3; ++k) ok = ok && std::isfinite(origins[(size_t)i * 3 + k]) && std::isfinite(d[k]) && std::isfinite(throughput[(size_t)i * 3 + k]);
    const double len2 = (double)d[0] * d[0] + (double)d[1] * d[1] + (double)d[2] * d[2];
    if (!ok || !(std::fabs(std::sqrt(len2) - 1.0) <= 1e-3)) return fail(c, PTC_E_ARG, "debug_shade_step: a ray is not finite or its direction not of unit length");
  }
  { int rc = debug_prepare(c, n, "debug_shade_step"); if (rc) return rc; }
  for (int32_t m : c->alpha.mode)
    if (m != PTC_ALPHA_OPAQUE) return fail(c, PTC_E_STATE, "debug_shade_step: the scene has a material with alpha coverage (that pass sits between trace and shade)");
  for (size_t m = 0; m < c->mats.size(); ++m)
    if (glass_tau(c, (int)m) > 0.0f) return fail(c, PTC_E_STATE, "debug_shade_step: the scene has a transmissive material (that pass sits between trace and shade)");
  LaunchCfg cfg = c->cfg;
  if (variant == 1) cfg.shade_sort = 1;
  if (variant == 2) {
    if (!pt_shade_tables_fit(c->scene.dsc)) return fail(c, PTC_E_STATE, "debug_shade_step: the scene's tables do not fit k_shade's copies in LDS (variant 2)");
    cfg.shade_sort = 0; cfg.shade_tables_lds = 1;
  }
  const Lane& ln = c->lanes[0];
  { int rc = stage_rays(c, ln.q.ray[0], n, origins, dirs, [&](uint32_t i, float4& B, float4& C) {
      B.z = throughput[i * 3]; B.w = throughput[i * 3 + 1];
      C = make_float4(throughput[i * 3 + 2], prev_pdf[i], __builtin_bit_cast(float, i), __builtin_bit_cast(float, keys[i]));
    }); if (rc) return rc; }
  HIP_TRY(c, hipMemset(ln.q.lpath, 0, (size_t)n * sizeof(float4)));
  const DevQueues q = batch_queues(c, 0, n);
  const DevScene sc = lane_scene(c, 0);
  DevFrame fr{};
  fr.max_bounces = (int)max_bounces;
  pt_launch_set_counts(ln.stream, cfg, q, n, 0);
  pt_launch_trace_closest(ln.stream, cfg, sc, q, 0, false);
  pt_launch_shade(ln.stream, cfg, ln.d_scene, fr, q, 0, bounce);
  HIP_TRY(c, hipGetLastError());
  HIP_TRY(c, hipStreamSynchronize(ln.stream));
  std::vector<float4> H(n), L(n);
  HIP_TRY(c, hipMemcpy(H.data(), ln.q.hit, n * sizeof(float4), hipMemcpyDeviceToHost));
  HIP_TRY(c, hipMemcpy(L.data(), ln.q.lpath, n * sizeof(float4), hipMemcpyDeviceToHost));
  for (uint32_t i = 0; i < n; ++i) {
    std::memcpy(out_hit + (size_t)i * 4, &H[i], 16);
    out_lpath[i * 3] = L[i].x; out_lpath[i * 3 + 1] = L[i].y; out_lpath[i * 3 + 2] = L[i].z;
  }
  std::memset(out_alive, 0, n); std::memset(out_shadow_valid, 0, n);
  std::memset(out_cont, 0, (size_t)n * 40); std::memset(out_shadow, 0, (size_t)n * 40);
  { int rc = scatter_segment_records(c, q, q.seg_ray[1], q.ray[1], ray_path, n, "debug_shade_step", "continuation", [&](uint32_t path, const float4& A, const float4& B, const float4& C) {
      out_alive[path] = 1;
      const float r[10] = {A.x, A.y, A.z, A.w, B.x, B.y, B.z, B.w, C.x, C.y};
      std::memcpy(out_cont + (size_t)path * 10, r, sizeof r);
    }); if (rc) return rc; }
  return scatter_segment_records(c, q, q.seg_sh, as_rays(q.shadow), shadow_path, n, "debug_shade_step", "shadow", [&](uint32_t path, const float4& A, const float4& B, const float4& C) {
    out_shadow_valid[path] = 1;
    const float r[10] = {A.x, A.y, A.z, A.w, B.x, B.y, B.z, C.x, C.y, C.z};
    std::memcpy(out_shadow + (size_t)path * 10, r, sizeof r);
  });
}

int ptc_debug_get_env_tables(ptc_ctx* c, int* w, int* h, int* ok, float* env, float* marg, float* cond) {
  if (!c) return PTC_E_ARG;
  if (!c->committed) return fail(c, PTC_E_STATE, "debug_get_env_tables: scene not committed");
  const HostBuilt& B = *c->built;
  if (w) *w = B.env_w;
  if (h) *h = B.env_h;
  if (ok) *ok = B.env_ok;
  if (B.env_w <= 0 || B.env_h <= 0) return PTC_OK;
  if (env) std::memcpy(env, B.env.data(), B.env.size() * 4);
  if (marg) std::memcpy(marg, B.env_marg.data(), B.env_marg.size() * 4);
  if (cond) std::memcpy(cond, B.env_cond.data(), B.env_cond.size() * 4);
  return PTC_OK;
}

int ptc_debug_camera_rays(ptc_ctx* c, int w, int h, uint64_t seed, uint32_t first_sample, uint32_t n_samples, const uint32_t* pixels, uint32_t n_pixels,
                          float* origins, float* dirs) {
  if (!c) return PTC_E_ARG;
  if (!pixels || !origins || !dirs || w <= 0 || h <= 0 || (uint64_t)w * (uint64_t)h > 0x7fffffffull || n_samples == 0 || n_pixels == 0 ||
      (uint64_t)n_pixels * (uint64_t)n_samples > 0x7fffffffull || (uint64_t)first_sample + n_samples > 0xffffffffull)
    return fail(c, PTC_E_ARG, "debug_camera_rays: bad argument");
  for (uint32_t j = 0; j < n_pixels; ++j)
    if (pixels[j] >= (uint32_t)w * (uint32_t)h) return fail(c, PTC_E_ARG, "debug_camera_rays: pixel index outside the frame");
  if (entry_frame(c)) return fail(c, PTC_E_STATE, "debug_camera_rays: a probe or lightmap frame is in progress (its rays: ptc_debug_probe_rays, ptc_debug_lightmap_rays)");
  const uint32_t n = n_pixels * n_samples;
  const uint32_t seed_hash = ::seed_hash(seed);
  if (c->device < 0) {      // the host evaluation of pt_lens.h
    if (!c->have_cam) return fail(c, PTC_E_STATE, "debug_camera_rays: no camera (ptc_set_camera)");
    DevCamera cam;
    make_camera_in_force(c, cam);
    const PtCamProj proj = cam_proj(c);
    for (uint32_t p = 0; p < n; ++p) {
      uint32_t key, j, s;
      pt_path_entry(PT_ORDER_SAMPLE, p, n_pixels, n_samples, j, s);      // the output's order, whatever order the context's frames use
      if (proj.projection != PTC_PROJ_PERSPECTIVE) pt_proj_ray(cam, proj, w, h, seed_hash, pixels[j], first_sample + s, origins + (size_t)p * 3, dirs + (size_t)p * 3, key);      // pt_camera.h
      else pt_lens_ray(cam, c->lens, w, h, seed_hash, pixels[j], first_sample + s, origins + (size_t)p * 3, dirs + (size_t)p * 3, key);
    }
    return PTC_OK;
  }
  { int rc = debug_prepare(c, n, "debug_camera_rays"); if (rc) return rc; }
  const Lane& ln = c->lanes[0];
  DevBuf<uint32_t> list;
  { int rc = ensure_buf(c, list, n_pixels); if (rc) return rc; }
  std::vector<float4> A(n), B(n);
  hipError_t e = hipMemcpy(list.p, pixels, (size_t)n_pixels * 4, hipMemcpyHostToDevice);
  if (e == hipSuccess) {
    DevFrame fr{};
    fr.w = w; fr.h = h; fr.seed_hash = seed_hash; fr.max_bounces = 0; fr.n_owned = n_pixels; fr.owned = list.p;
    fr.path_order = c->path_order;      // the kernels run as a camera frame runs them; the read-back below re-maps the slots to the output's sample-major order
    const DevQueues q = batch_queues(c, 0, n);
    if (cam_projection(c) != PTC_PROJ_PERSPECTIVE) pt_launch_raygen_proj(ln.stream, c->cam, cam_proj(c), fr, q, first_sample, n_samples);      // run_batch's choice
    else if (c->lens.aperture_radius > 0.0f) pt_launch_raygen_lens(ln.stream, c->cam, c->lens, fr, q, first_sample, n_samples);
    else pt_launch_raygen(ln.stream, c->cam, fr, q, first_sample, n_samples, false);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipStreamSynchronize(ln.stream);
  if (e == hipSuccess) e = hipMemcpy(A.data(), ln.q.ray[0].A, (size_t)n * sizeof(float4), hipMemcpyDeviceToHost);
  if (e == hipSuccess) e = hipMemcpy(B.data(), ln.q.ray[0].B, (size_t)n * sizeof(float4), hipMemcpyDeviceToHost);
  list.release();      // the pixel list lives for this call only
  if (e != hipSuccess) return fail(c, PTC_E_DEVICE, std::string("debug_camera_rays: ") + hipGetErrorString(e));
  for (uint32_t p = 0; p < n; ++p) {      // output ray p = sample p / n_pixels of pixels[p % n_pixels]; the device wrote it to the slot of the context's path order
    uint32_t j, s;
    pt_path_entry(PT_ORDER_SAMPLE, p, n_pixels, n_samples, j, s);
    const size_t d = pt_path_id(c->path_order, j, s, n_pixels, n_samples), o = (size_t)p * 3;
    origins[o] = A[d].x; origins[o + 1] = A[d].y; origins[o + 2] = A[d].z;
    dirs[o] = A[d].w; dirs[o + 1] = B[d].x; dirs[o + 2] = B[d].y;
  }
  return PTC_OK;
}

int ptc_debug_probe_rays(ptc_ctx* c, const float* positions_xyz, int n_probes, uint32_t probe_index_base, uint64_t seed, uint32_t first_sample, uint32_t n_samples,
                         float* out_o_d, uint32_t* out_key) {
  if (!c) return PTC_E_ARG;
  if (!positions_xyz || !out_o_d || !out_key || probe_debug_args_bad(n_probes, probe_index_base, first_sample, n_samples)) return fail(c, PTC_E_ARG, "debug_probe_rays: bad argument");
  const uint32_t np = (uint32_t)n_probes, n = np * n_samples;
  const uint32_t seed_hash = ::seed_hash(seed);
  if (c->device < 0) {      // the host evaluation of pt_probes.h
    for (uint32_t p = 0; p < n; ++p) {
      const uint32_t j = p % np;
      float* o = out_o_d + (size_t)p * 6;
      for (int k = 0; k < 3; ++k) o[k] = positions_xyz[(size_t)j * 3 + k];
      pt_probe_dir(seed_hash, probe_index_base + j, first_sample + p / np, o + 3, out_key[p]);
    }
    return PTC_OK;
  }
  { int rc = probe_debug_prepare(c, n); if (rc) return rc; }
  const Lane& ln = c->lanes[0];
  DevBuf<float4> pos;
  { int rc = ensure_buf(c, pos, np); if (rc) return rc; }
  std::vector<float4> P(np), A(n), B(n), C(n);
  for (uint32_t j = 0; j < np; ++j) P[j] = make_float4(positions_xyz[(size_t)j * 3], positions_xyz[(size_t)j * 3 + 1], positions_xyz[(size_t)j * 3 + 2], 0.0f);
  hipError_t e = hipMemcpy(pos.p, P.data(), (size_t)np * sizeof(float4), hipMemcpyHostToDevice);
  if (e == hipSuccess) {
    pt_launch_raygen_probe(ln.stream, pos.p, np, probe_index_base, seed_hash, batch_queues(c, 0, n), first_sample, n_samples);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipStreamSynchronize(ln.stream);
  if (e == hipSuccess) e = hipMemcpy(A.data(), ln.q.ray[0].A, (size_t)n * sizeof(float4), hipMemcpyDeviceToHost);
  if (e == hipSuccess) e = hipMemcpy(B.data(), ln.q.ray[0].B, (size_t)n * sizeof(float4), hipMemcpyDeviceToHost);
  if (e == hipSuccess) e = hipMemcpy(C.data(), ln.q.ray[0].C, (size_t)n * sizeof(float4), hipMemcpyDeviceToHost);
  pos.release();      // the positions live for this call only
  if (e != hipSuccess) return fail(c, PTC_E_DEVICE, std::string("debug_probe_rays: ") + hipGetErrorString(e));
  for (size_t p = 0; p < n; ++p) {
    float* o = out_o_d + p * 6;
    o[0] = A[p].x; o[1] = A[p].y; o[2] = A[p].z; o[3] = A[p].w; o[4] = B[p].x; o[5] = B[p].y;
    std::memcpy(&out_key[p], &C[p].w, 4);
  }
  return PTC_OK;
}

int ptc_debug_probe_project(ptc_ctx* c, int n_probes, uint32_t probe_index_base, uint64_t seed, uint32_t first_sample, uint32_t n_samples, const float* lpath_rgba,
                            float* acc_inout) {
  if (!c) return PTC_E_ARG;
  if (!lpath_rgba || !acc_inout || probe_debug_args_bad(n_probes, probe_index_base, first_sample, n_samples)) return fail(c, PTC_E_ARG, "debug_probe_project: bad argument");
  const uint32_t np = (uint32_t)n_probes, n = np * n_samples;
  const uint32_t seed_hash = ::seed_hash(seed);
  if (c->device < 0) {      // the host evaluation of pt_probes.h: k_accumulate_sh's sums, sample by sample
    for (uint32_t j = 0; j < np; ++j)
      for (uint32_t s = 0; s < n_samples; ++s) {
        const float* L = lpath_rgba + ((size_t)s * np + j) * 4;
        float d[3]; uint32_t key;
        pt_probe_dir(seed_hash, probe_index_base + j, first_sample + s, d, key);
        for (int k = 0; k < PT_SH9; ++k) {
          const float b = pt_sh9_basis(k, d[0], d[1], d[2]);
          float* a = acc_inout + (size_t)j * PT_SH9_FLOATS + (size_t)k * 3;
          for (int ch = 0; ch < 3; ++ch) a[ch] = a[ch] + L[ch] * b;
        }
      }
    return PTC_OK;
  }
  { int rc = probe_debug_prepare(c, n); if (rc) return rc; }
  const Lane& ln = c->lanes[0];
  DevBuf<float> acc;
  const size_t na = (size_t)np * PT_SH9_FLOATS;
  { int rc = ensure_buf(c, acc, na); if (rc) return rc; }
  hipError_t e = hipMemcpy(acc.p, acc_inout, na * sizeof(float), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(ln.q.lpath, lpath_rgba, (size_t)n * sizeof(float4), hipMemcpyHostToDevice);
  if (e == hipSuccess) {
    pt_launch_accumulate_sh(ln.stream, np, probe_index_base, seed_hash, ln.q.lpath, acc.p, first_sample, n_samples);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipStreamSynchronize(ln.stream);
  if (e == hipSuccess) e = hipMemcpy(acc_inout, acc.p, na * sizeof(float), hipMemcpyDeviceToHost);
  acc.release();
  if (e != hipSuccess) return fail(c, PTC_E_DEVICE, std::string("debug_probe_project: ") + hipGetErrorString(e));
  return PTC_OK;
}

int ptc_debug_probe_resolve(const float* acc, int n_probes, uint32_t n_samples, float* out) {
  if (!acc || !out || n_probes < 1 || n_probes > PTC_MAX_PROBES || n_samples == 0) return PTC_E_ARG;
  const float scale = pt_sh9_resolve_scale(n_samples);
  for (size_t i = 0; i < (size_t)n_probes * PT_SH9_FLOATS; ++i) out[i] = acc[i] * scale;
  return PTC_OK;
}

int ptc_debug_get_flat_scene(ptc_ctx* c, uint32_t* n_verts, uint32_t* n_tris, ptc_vertex* verts, uint32_t* indices, int32_t* tri_material) {
  if (!c) return PTC_E_ARG;
  if (!c->committed) return fail(c, PTC_E_STATE, "debug_get_flat_scene: scene not committed");
  { int rr = refresh_host_copy(c); if (rr) return rr; }
  const HostBuilt& B = *c->built;
  if (n_verts) *n_verts = (uint32_t)B.wverts.size();
  if (n_tris) *n_tris = B.n_tris;
  if (verts) std::memcpy(verts, B.wverts.data(), B.wverts.size() * sizeof(ptc_vertex));
  if (indices) std::memcpy(indices, B.widx.data(), B.widx.size() * 4);
  if (tri_material) std::memcpy(tri_material, B.tri_mat.data(), B.tri_mat.size() * 4);
  return PTC_OK;
}

int ptc_debug_get_description(ptc_ctx* c, int* n_materials, int* n_textures) {
  if (!c) return PTC_E_ARG;
  if (n_materials) *n_materials = (int)c->mats.size();
  if (n_textures) *n_textures = (int)c->texs.size();
  return PTC_OK;
}

int ptc_debug_get_material(ptc_ctx* c, int index, float out_factors[9], int out_textures[3]) {
  if (!c) return PTC_E_ARG;
  if (index < 0 || (size_t)index >= c->mats.size() || !out_factors || !out_textures) return fail(c, PTC_E_ARG, "debug_get_material: bad argument");
  const HostMaterial& m = c->mats[(size_t)index];
  std::memcpy(out_factors, m.base, 16); out_factors[4] = m.metallic; out_factors[5] = m.roughness; std::memcpy(out_factors + 6, m.emissive, 12);
  out_textures[0] = m.tex_color; out_textures[1] = m.tex_normal; out_textures[2] = m.tex_mr;
  return PTC_OK;
}

int ptc_debug_get_texture(ptc_ctx* c, int index, int* w, int* h, uint8_t* rgba) {
  if (!c) return PTC_E_ARG;
  if (index < 0 || (size_t)index >= c->texs.size()) return fail(c, PTC_E_ARG, "debug_get_texture: bad argument");
  const HostTexture& t = c->texs[(size_t)index];
  if (w) *w = t.w;
  if (h) *h = t.h;
  if (rgba) std::memcpy(rgba, t.px.data(), t.px.size());
  return PTC_OK;
}

int ptc_debug_get_counters(ptc_ctx* c, uint64_t* out, int n) {
  { int rd = need_device(c); if (rd) return rd; }
  if (!out || n <= 0) return fail(c, PTC_E_ARG, "debug_get_counters: bad argument");
  { int rf = flush(c); if (rf) return rf; }
  { int rs = sync_all_lanes(c); if (rs) return rs; }
  unsigned long long st[ST_N];
  { int rc = sum_lane_stats(c, st); if (rc) return rc; }
  for (int i = 0; i < n; ++i) out[i] = i < ST_N ? st[i] : 0;
  return ST_N;
}

int ptc_debug_get_bvh(ptc_ctx* c, uint32_t* n_nodes, uint32_t* n_tris, uint32_t* n_units, float* units, float grid[6]) {
  if (!c) return PTC_E_ARG;
  if (!c->committed) return fail(c, PTC_E_STATE, "debug_get_bvh: scene not committed");
  { int rr = refresh_host_copy(c); if (rr) return rr; }
  const HostBuilt& B = *c->built;
  if (n_nodes) *n_nodes = B.n_nodes;
  if (n_tris) *n_tris = B.n_tri_records;
  if (n_units) *n_units = B.n_units;
  if (units) std::memcpy(units, B.recs.data(), B.recs.size() * 4);
  if (grid) for (int k = 0; k < 3; ++k) { grid[k] = B.grid_lo[k]; grid[3 + k] = B.grid_step[k]; }
  return PTC_OK;
}

// Context internals for tests of the host logic: [0] HIP events created so far, [1] timing spans waiting to be collected,
// [2] queue capacity (paths) of lane 0, [3] samples of one full batch, [4] samples accepted but not yet issued,
// [5] trace blocks per CU, [6] stack entries per lane kept in LDS.
// identity of the host build a context renders from (the contexts of a group share one: ptc_group_scene_commit): tests compare the values
uint64_t ptc_debug_host_build_id(const ptc_ctx* c) { return c ? (uint64_t)(uintptr_t)c->built.get() : 0u; }

int ptc_debug_get_internals(ptc_ctx* c, uint64_t out[8]) {
  if (!c || !out) return PTC_E_ARG;
  for (int i = 0; i < 8; ++i) out[i] = 0;
  out[0] = c->events_created; out[1] = c->spans.size(); out[2] = c->lanes.empty() ? 0 : c->lanes[0].q.cap; out[3] = c->per_batch; out[4] = c->pending;
  out[5] = (uint64_t)c->cfg.trace_blocks_per_cu; out[6] = (uint64_t)c->cfg.stack_lds;
  out[7] = (c->scene.last_refit_on_device ? 1u : 0u) | (c->scene.commit_on_device ? 2u : 0u) | (c->scene.tree_device_sah ? 4u : 0u) | (c->debug_verts_from_device ? 8u : 0u);
  return PTC_OK;
}

// The host's share of a refit on the device, run without a device (CPU tests, sanitizer builds): builds the plan of the committed scene and the
// emitter table of the CURRENT transforms from the emissive primitives alone, and checks them against the host build — call it after
// ptc_scene_refit on a description-only context.  out: [0] world vertices, [1] primitives, [2] 8-wide nodes in the level lists, [3] levels,
// [4] emissive-material primitives, [5] 1 if the level lists hold every node address of the tree exactly once with children after parents,
// [6] 1 if the emitter table and cdf equal the host refit's bit for bit (0 also when the set of emitters changed), [7] 1 if all transforms are finite.
int ptc_debug_refit_host_parts(ptc_ctx* c, uint64_t out[8]) {
  if (!c || !out) return PTC_E_ARG;
  if (!c->committed) return fail(c, PTC_E_STATE, "debug_refit_host_parts: scene not committed");
  { int rr = refresh_host_copy(c); if (rr) return rr; }
  const HostBuilt& B = *c->built;
  RefitPlan P;
  ptc_refit_plan(c->mats, c->meshes, c->insts, B, P);
  std::vector<float> xf, lights, cdf;
  const bool finite = ptc_refit_instance_transforms(c->insts, xf);
  const bool same_set = ptc_refit_emitters(c->mats, c->meshes, c->insts, P, B, lights, cdf);
  out[0] = P.n_verts; out[1] = P.n_tris; out[2] = P.level_nodes.size(); out[3] = P.level_first.empty() ? 0 : P.level_first.size() - 1; out[4] = P.emit_prims.size() / 5;
  // every node once, and a node's children (its block's interior records) in an earlier level than the node itself
  bool ok = P.level_nodes.size() == B.n_nodes && !P.level_first.empty() && P.level_first.back() == P.level_nodes.size() && P.vert_inst.size() == B.wverts.size();
  std::vector<int32_t> level_of((size_t)B.n_units / 4 + 1, -1);
  for (size_t l = 0; ok && l + 1 < P.level_first.size(); ++l)
    for (uint32_t i = P.level_first[l]; i < P.level_first[l + 1]; ++i) {
      const uint32_t a = P.level_nodes[i];
      if ((a & 3u) || a >= B.n_units || level_of[a >> 2] >= 0) { ok = false; break; }
      level_of[a >> 2] = (int32_t)l;
    }
  for (size_t i = 0; ok && i < P.level_nodes.size(); ++i) {
    const uint32_t a = P.level_nodes[i];
    uint32_t w2, w3; std::memcpy(&w2, &B.recs[(size_t)a * 4 + 2], 4); std::memcpy(&w3, &B.recs[(size_t)a * 4 + 3], 4);
    const uint32_t imask = (w2 >> 8) & 255u;
    for (uint32_t k = 0; k < (uint32_t)__builtin_popcount(imask); ++k) {
      const uint32_t ch = w3 + 4u * k;
      if (ch >= B.n_units || level_of[ch >> 2] < 0 || level_of[ch >> 2] >= level_of[a >> 2]) { ok = false; break; }
    }
  }
  out[5] = ok ? 1u : 0u;
  out[6] = (same_set && lights.size() == B.lights.size() && cdf.size() == B.cdf.size() && std::memcmp(lights.data(), B.lights.data(), lights.size() * 4) == 0 &&
            std::memcmp(cdf.data(), B.cdf.data(), cdf.size() * 4) == 0) ? 1u : 0u;
  out[7] = finite ? 1u : 0u;
  return PTC_OK;
}

// The host's share of a COMMIT on the device (ptc_build_skeleton), run without a device (CPU tests, sanitizer builds): describes the committed description again the way
// device_commit does — no flatten, the emitter table from the emissive primitives alone — and holds it against the host build the context was committed with.
// out: [0] primitives, [1] emitters, [2] 1 if world vertex indices and material per primitive agree, [3] 1 if the emitter index per primitive, the emitter table and its cdf
// agree bit for bit, [4] 1 if the material table agrees, [5] 1 if textures, texture sets and environment tables agree, [6] 1 if shading-record stride and vertex count agree.
int ptc_debug_commit_host_parts(ptc_ctx* c, uint64_t out[8]) {
  if (!c || !out) return PTC_E_ARG;
  if (!c->committed) return fail(c, PTC_E_STATE, "debug_commit_host_parts: scene not committed");
  { int rr = refresh_host_copy(c); if (rr) return rr; }
  if (!description_matches_commit(c)) return fail(c, PTC_E_STATE, kDescriptionChanged);
  const HostBuilt& B = *c->built;
  HostBuilt S;
  const std::string e = ptc_build_skeleton(c->mats, c->meshes, c->insts, c->texs, c->env, c->toplet_budget, S);
  if (!e.empty()) return fail(c, PTC_E_STATE, e);
  for (int i = 0; i < 8; ++i) out[i] = 0;
  auto same = [](const auto& a, const auto& b) { return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), a.size() * sizeof(a[0])) == 0); };
  out[0] = S.n_tris; out[1] = S.n_lights;
  out[2] = (S.n_tris == B.n_tris && same(S.widx, B.widx) && same(S.tri_mat, B.tri_mat)) ? 1u : 0u;
  out[3] = (S.n_lights == B.n_lights && same(S.prim_light, B.prim_light) && same(S.lights, B.lights) && same(S.cdf, B.cdf)) ? 1u : 0u;
  out[4] = same(S.mats, B.mats) ? 1u : 0u;
  out[5] = (same(S.texels, B.texels) && same(S.tex_info, B.tex_info) && same(S.set_texels, B.set_texels) && same(S.set_info, B.set_info) && same(S.env, B.env) && same(S.env_marg, B.env_marg) &&
            same(S.env_cond, B.env_cond) && same(S.env_marg_guide, B.env_marg_guide) && same(S.env_cond_guide, B.env_cond_guide) && S.env_w == B.env_w && S.env_h == B.env_h && S.env_ok == B.env_ok) ? 1u : 0u;
  out[6] = (S.shade_stride == B.shade_stride && S.n_wverts == B.n_wverts && B.n_wverts == B.wverts.size()) ? 1u : 0u;
  return PTC_OK;
}

// The tables k_shade reads besides the BVH: shading records (4 * stride floats per primitive), emitters (20 floats each), their power cdf.
// Sizes come back through the pointers; arrays may be null.
int ptc_debug_get_shading_tables(ptc_ctx* c, uint32_t* stride, float* shade, uint32_t* n_lights, float* lights, float* cdf) {
  if (!c) return PTC_E_ARG;
  if (!c->committed) return fail(c, PTC_E_STATE, "debug_get_shading_tables: scene not committed");
  { int rr = refresh_host_copy(c); if (rr) return rr; }
  const HostBuilt& B = *c->built;
  if (stride) *stride = B.shade_stride;
  if (n_lights) *n_lights = B.n_lights;
  if (shade) std::memcpy(shade, B.shade.data(), B.shade.size() * 4);
  if (lights) std::memcpy(lights, B.lights.data(), B.lights.size() * 4);
  if (cdf) std::memcpy(cdf, B.cdf.data(), B.cdf.size() * 4);
  return PTC_OK;
}

int ptc_debug_get_mesh_vertices(ptc_ctx* c, int mesh, ptc_vertex* out) {
  if (!c) return PTC_E_ARG;
  if (mesh < 0 || mesh >= (int)c->meshes.size() || !out) return fail(c, PTC_E_ARG, "debug_get_mesh_vertices: bad argument");
  const size_t m = (size_t)mesh;
  const size_t bytes = c->meshes[m].v.size() * sizeof(ptc_vertex);
  c->debug_verts_from_device = false;
  if (m < c->poses.size() && c->poses[m].active()) {
    const MeshPose& P = c->poses[m];
    const CommittedScene& s = c->scene;
    if (c->device >= 0 && s.refit_ready && P.on_device && m < s.deform.size() && s.deform[m].n_verts) {      // evaluated in HBM: from there
      HIP_TRY(c, hipSetDevice(c->device));
      { int rs = sync_all_lanes(c); if (rs) return rs; }
      HIP_TRY(c, hipMemcpy(out, s.deform[m].out, bytes, hipMemcpyDeviceToHost));
      c->debug_verts_from_device = true;
      return PTC_OK;
    }
    // not evaluated in HBM: the host's evaluation of the LIVE pose, into `out` alone — a pending pose is only recorded, and one that a refit refused never shows
    const size_t want = pt_deform_pose_floats(P.data->n_targets, P.data->skin.empty() ? 0u : P.data->n_joints);
    if (c->committed && P.base_live && P.base_live->size() == c->meshes[m].v.size() && P.pose_live.size() == want) {
      pt_deform_eval_mesh(*P.data, P.base_live->data(), P.pose_live.data(), reinterpret_cast<HostVertex*>(out));
      return PTC_OK;
    }
    deform_host_all(c);      // before the first commit there is no live pose: the pending one
  }
  std::memcpy(out, c->meshes[m].v.data(), bytes);
  return PTC_OK;
}

int ptc_debug_display_state(ptc_ctx* c, uint32_t out[8]) {
  { int rd = need_device(c); if (rd) return rd; }
  if (!out) return fail(c, PTC_E_ARG, "debug_display_state: null pointer");
  std::memset(out, 0, 8 * sizeof(uint32_t));
  if (!c->display.state.p) return PTC_OK;
  HIP_TRY(c, hipStreamSynchronize(c->lanes[0].stream));
  HIP_TRY(c, hipMemcpy(out, c->display.state.p, sizeof(pt_display_state), hipMemcpyDeviceToHost));
  return PTC_OK;
}

int ptc_debug_display_internals(ptc_ctx* c, uint64_t out[4]) {
  if (!c || !out) return PTC_E_ARG;
  out[0] = pt_display_meter_grid_pixels(); out[1] = 0; out[2] = 0; out[3] = 0;
  return PTC_OK;
}

int ptc_debug_display_pixel(const ptc_display_params* params, float E, const float rgba_in[4], uint8_t out8[4], uint16_t out16[4]) {
  const ptc_display_params p = with_defaults(params, ptc_display_default_params);
  if (!rgba_in || pt_display_params_error(p)) return PTC_E_ARG;
  if (out8) {
    const uint32_t v = pt_display_host_pixel8(p, E, rgba_in);
    for (int k = 0; k < 4; ++k) out8[k] = (uint8_t)(v >> (8 * k));
  }
  if (out16) {
    uint32_t lo, hi;
    pt_display_pixel16(rgba_in[0], rgba_in[1], rgba_in[2], rgba_in[3], E, lo, hi);
    out16[0] = (uint16_t)lo; out16[1] = (uint16_t)(lo >> 16); out16[2] = (uint16_t)hi; out16[3] = (uint16_t)(hi >> 16);
  }
  return PTC_OK;
}

int ptc_debug_meter(const ptc_display_params* params, const float* rgba, uint64_t n_pixels, uint32_t state_in, uint32_t* state_out, uint32_t* Q_out, uint64_t* N_out,
                    uint64_t* M_out, uint64_t* rejected_out, uint32_t hist_out[4096]) {
  const ptc_display_params p = with_defaults(params, ptc_display_default_params);
  if ((!rgba && n_pixels) || n_pixels > PT_DISPLAY_MAX_PIXELS || pt_display_params_error(p)) return PTC_E_ARG;
  std::vector<uint32_t> hist(PT_DISPLAY_BINS, 0u);
  uint64_t N = 0, rejected = 0;
  for (uint64_t i = 0; i < n_pixels; ++i) {
    uint32_t key = 0;
    const int cls = pt_meter_classify(rgba[4 * i], rgba[4 * i + 1], rgba[4 * i + 2], rgba[4 * i + 3], key);
    if (cls == 1) { hist[key]++; N++; } else if (cls == 2) rejected++;
  }
  uint64_t n_lo, n_hi, before = 0, S = 0, M = 0;
  pt_meter_bounds((uint32_t)N, p.percentile_lo, p.percentile_hi, n_lo, n_hi);
  for (uint32_t k = 0; k < PT_DISPLAY_BINS; ++k) {
    const uint64_t kept = pt_meter_kept(before, hist[k], n_lo, n_hi);
    S += kept * (uint64_t)(2u * k + 1u); M += kept; before += hist[k];
  }
  const uint32_t Q = pt_meter_mean(S, M);
  if (state_out) *state_out = pt_meter_adapt(state_in, Q, M, p.adapt_rate);
  if (Q_out) *Q_out = Q;
  if (N_out) *N_out = N;
  if (M_out) *M_out = M;
  if (rejected_out) *rejected_out = rejected;
  if (hist_out) std::memcpy(hist_out, hist.data(), PT_DISPLAY_BINS * sizeof(uint32_t));
  return PTC_OK;
}

// The fast paths of csrc/pt_exact.h against the compiler's / and sqrtf, on the device (include/ptc_exact_debug.h).  Needs a device, no scene; touches nothing
// of the context but its error string.
int ptc_debug_exact_arith(ptc_ctx* c, int op, const float* a, const float* b, uint64_t n, uint32_t first, int cross, uint64_t* out) {
  if (!c) return PTC_E_ARG;
  if (!out || op < PTC_EXACT_RCP || op > PTC_EXACT_DIV3 || n == 0 || n > (1ull << 32) || (b && !a) || (a && n > (1ull << 28)) ||
      (cross && (!a || !b || n > (1ull << 16) || (op != PTC_EXACT_DIV && op != PTC_EXACT_DIV3))))
    return fail(c, PTC_E_ARG, "debug_exact_arith: bad argument");
  { int rd = need_device(c); if (rd) return rd; }
  DevBuf<float> da, db;
  DevBuf<unsigned long long> dout;
  const size_t words = 1 + 4 * PTC_EXACT_OFFENDERS;
  { int rc = ensure_buf(c, dout, words); if (rc) return rc; }
  HIP_TRY(c, hipMemset(dout.p, 0, words * sizeof(unsigned long long)));
  if (a) {
    { int rc = ensure_buf(c, da, (size_t)n); if (rc) return rc; }
    HIP_TRY(c, hipMemcpy(da.p, a, (size_t)n * sizeof(float), hipMemcpyHostToDevice));
  }
  if (b) {
    { int rc = ensure_buf(c, db, (size_t)n); if (rc) return rc; }
    HIP_TRY(c, hipMemcpy(db.p, b, (size_t)n * sizeof(float), hipMemcpyHostToDevice));
  }
  pt_launch_exact_arith(nullptr, op, da.p, db.p, n, first, cross, dout.p);
  HIP_TRY(c, hipGetLastError());
  static_assert(sizeof(unsigned long long) == sizeof(uint64_t), "the counters are copied out as they are");
  HIP_TRY(c, hipMemcpy(out, dout.p, words * sizeof(uint64_t), hipMemcpyDeviceToHost));
  return PTC_OK;
}
}  // extern "C"

