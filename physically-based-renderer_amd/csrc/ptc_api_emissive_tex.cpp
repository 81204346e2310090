// ptc_api_emissive_tex.cpp — textured emission over the C-ABI (pt_emissive_tex.h): the material calls, the table of the committed scene and its
// placement after a refit or rebuild, the upload, the statistics and the ptc_debug_emissive_tex_* hooks.
#include "ptc_ctx.h"

#include <cmath>

using namespace ptc_detail;

namespace {
uint32_t shadow_path(const float4& B, const float4&) { return __builtin_bit_cast(uint32_t, B.w); }

pt_emtex_textures built_textures(const ptc_ctx* c) { return pt_emtex_textures{c->built->texels.data(), c->built->tex_info.data(), c->tex_linear}; }
}  // namespace

namespace ptc_detail {
void emtex_commit(ptc_ctx* c) {
  EmTex& e = c->emtex;
  const bool had = !e.table.fixed.empty() || e.n_dev > 0;
  pt_emtex_describe(e.mats, c->meshes, c->insts, c->texs, built_textures(c), e.table);
  pt_emtex_place(c->meshes, c->insts, e.table);
  e.dirty = had || !e.table.fixed.empty();
}

void emtex_place(ptc_ctx* c) {
  EmTex& e = c->emtex;
  if (e.table.fixed.empty()) return;
  // a posed mesh whose copy in the description is not the pending pose (a refit on the device): the host evaluates the entries' own vertices, as deform_host_emissive
  // does for the emitter table's — pt_deform_eval_vertex writes the posed vertex where a whole-mesh evaluation would
  std::vector<std::vector<float>> pose(c->poses.size());
  for (const pt_emtex_static& s : e.table.fixed) {
    const size_t m = (size_t)c->insts[s.inst].mesh;
    if (m >= c->poses.size() || !c->poses[m].active() || c->poses[m].host_fresh) continue;
    const MeshPose& P = c->poses[m];
    if (pose[m].empty()) pose[m] = P.pose();
    for (int k = 0; k < 3; ++k) pt_deform_eval_vertex(*P.data, P.base->data(), pose[m].data(), s.v[k], c->meshes[m].v[s.v[k]]);
  }
  pt_emtex_place(c->meshes, c->insts, e.table);
  e.dirty = true;
}

int emtex_upload(ptc_ctx* c) {
  EmTex& e = c->emtex;
  if (e.dirty) {
    const size_t n = e.table.recs.size();
    if (n) {
      int rc = ensure_buf(c, e.recs, n);
      if (!rc) rc = ensure_buf(c, e.cdf, n);
      if (!rc) rc = ensure_buf(c, e.prim_map, e.table.prim_map.size());
      if (!rc) rc = ensure_buf(c, e.counters, (size_t)PT_EMTEX_COUNTERS);
      if (rc) return rc;
      HIP_TRY(c, hipMemcpy(e.recs.p, e.table.recs.data(), n * sizeof(pt_emtex_rec), hipMemcpyHostToDevice));
      HIP_TRY(c, hipMemcpy(e.cdf.p, e.table.cdf.data(), n * sizeof(float), hipMemcpyHostToDevice));
      HIP_TRY(c, hipMemcpy(e.prim_map.p, e.table.prim_map.data(), e.table.prim_map.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    }
    e.n_dev = (uint32_t)n;
    e.dirty = false;
  }
  if (e.n_dev) HIP_TRY(c, hipMemset(e.counters.p, 0, PT_EMTEX_COUNTERS * sizeof(unsigned long long)));
  e.seconds = 0.0;
  return PTC_OK;
}

const char* emtex_medium_conflict(const ptc_ctx* c, int integrator) {
  if (integrator != PTC_INTEGRATOR_PATH || !c->committed || !c->medium.set || !(c->medium.params.sigma_t > 0.0f) || c->emtex.table.fixed.empty()) return nullptr;
  return "frame_begin: a medium is set and the committed scene has a material with an emission texture: a scatter point has no sampler for that light set — remove "
         "the emission textures (ptc_render: --no-emissive-textures) or clear the medium";
}
}  // namespace ptc_detail

extern "C" {
int ptc_set_material_emission_texture(ptc_ctx* c, int material, int texture, const float factor[3]) {
  if (!c) return PTC_E_ARG;
  if (c->committed) return fail(c, PTC_E_STATE, "set_material_emission_texture: the scene is committed (an emission texture belongs to the description: before ptc_scene_commit)");
  if (material < 0 || (size_t)material >= c->mats.size()) return fail(c, PTC_E_ARG, "set_material_emission_texture: material out of range");
  if (texture < 0) {      // removal
    if ((size_t)material < c->emtex.mats.size()) c->emtex.mats[(size_t)material] = pt_emtex_material{};
    return PTC_OK;
  }
  if (!factor) return fail(c, PTC_E_ARG, "set_material_emission_texture: null pointer");
  if ((size_t)texture >= c->texs.size()) return fail(c, PTC_E_ARG, "set_material_emission_texture: texture id out of range");
  for (int k = 0; k < 3; ++k)
    if (!std::isfinite(factor[k]) || !(factor[k] >= 0.0f)) return fail(c, PTC_E_ARG, "set_material_emission_texture: factor is not finite and >= 0");
  const HostMaterial& m = c->mats[(size_t)material];
  if (m.emissive[0] != 0.0f || m.emissive[1] != 0.0f || m.emissive[2] != 0.0f)
    return fail(c, PTC_E_ARG, "set_material_emission_texture: the material's emissive factor is not zero (the base emission of a textured emitter stays 0: pass the colour as `factor`)");
  if ((size_t)material < c->alpha.mode.size() && c->alpha.mode[(size_t)material] != PTC_ALPHA_OPAQUE)
    return fail(c, PTC_E_ARG, "set_material_emission_texture: the material's alpha mode is not OPAQUE (an emitter stays opaque)");
  if (glass_tau(c, material) > 0.0f) return fail(c, PTC_E_ARG, "set_material_emission_texture: the material is transmissive (an emitter stays opaque)");
  if (c->emtex.mats.size() < c->mats.size()) c->emtex.mats.resize(c->mats.size());
  pt_emtex_material& e = c->emtex.mats[(size_t)material];
  e.tex = texture;
  for (int k = 0; k < 3; ++k) e.factor[k] = factor[k];
  return PTC_OK;
}

int ptc_get_material_emission_texture(const ptc_ctx* c, int material, int* texture, float factor[3]) {
  if (!c || material < 0 || (size_t)material >= c->mats.size()) return PTC_E_ARG;
  const pt_emtex_material e = (size_t)material < c->emtex.mats.size() ? c->emtex.mats[(size_t)material] : pt_emtex_material{};
  if (texture) *texture = e.tex;
  if (factor) for (int k = 0; k < 3; ++k) factor[k] = e.factor[k];
  return PTC_OK;
}

int ptc_get_emissive_tex_stats(ptc_ctx* c, ptc_emissive_tex_stats* out) {
  if (!c) return PTC_E_ARG;
  if (!out) return fail(c, PTC_E_ARG, "get_emissive_tex_stats: null pointer");
  *out = ptc_emissive_tex_stats{};
  out->entries = c->committed ? c->emtex.table.fixed.size() : 0u;
  if (c->device < 0) return PTC_OK;
  ptc_stats st;      // flushes, waits and harvests the timing spans
  { int rc = ptc_get_stats(c, &st); if (rc) return rc; }
  if (c->emtex.n_dev && c->emtex.counters.p) {
    unsigned long long ctr[PT_EMTEX_COUNTERS];
    HIP_TRY(c, hipMemcpy(ctr, c->emtex.counters.p, sizeof ctr, hipMemcpyDeviceToHost));
    out->hit_additions = ctr[PT_EMTEX_HITS]; out->shadow_records = ctr[PT_EMTEX_SHADOW];
  }
  out->seconds_emissive_tex = c->emtex.seconds;
  return PTC_OK;
}

int ptc_debug_get_emissive_tex_table(ptc_ctx* c, uint32_t* n_entries, float* records28, float* cdf, uint32_t* n_prims, int32_t* prim_map, float* total) {
  if (!c) return PTC_E_ARG;
  if (!c->committed) return fail(c, PTC_E_STATE, "debug_get_emissive_tex_table: scene not committed");
  const pt_emtex_table& T = c->emtex.table;
  if (n_entries) *n_entries = (uint32_t)T.recs.size();
  if (n_prims) *n_prims = (uint32_t)T.prim_map.size();
  if (total) *total = T.total;
  if (records28 && !T.recs.empty()) std::memcpy(records28, T.recs.data(), T.recs.size() * sizeof(pt_emtex_rec));
  if (cdf && !T.cdf.empty()) std::memcpy(cdf, T.cdf.data(), T.cdf.size() * sizeof(float));
  if (prim_map && !T.prim_map.empty()) std::memcpy(prim_map, T.prim_map.data(), T.prim_map.size() * sizeof(int32_t));
  return PTC_OK;
}

int ptc_debug_emissive_tex_sample(const float entry28[28], const uint8_t* rgba, int w, int h, int filter, ptc_emissive_tex_sample* io) {
  if (!entry28 || !rgba || !io || w <= 0 || h <= 0 || (filter != PTC_FILTER_NEAREST && filter != PTC_FILTER_LINEAR)) return PTC_E_ARG;
  pt_emtex_rec E;
  std::memcpy(&E, entry28, sizeof E);
  E.tex = 0;
  std::vector<uint32_t> texels((size_t)w * (size_t)h);
  std::memcpy(texels.data(), rgba, texels.size() * 4);
  const int32_t info[4] = {0, w, h, 0};
  const pt_emtex_textures t{texels.data(), info, filter};
  v3 y = V3(0, 0, 0), wi = V3(0, 0, 0), Le = V3(0, 0, 0);
  float pl = 0.0f;
  io->ok = pt_emtex_sample(E, t, V3(io->P), io->r1, io->r2, y, wi, pl, Le) ? 1 : 0;
  if (!io->ok) { y = wi = Le = V3(0, 0, 0); pl = 0.0f; }
  scene_rules::store3(io->y, y); scene_rules::store3(io->wi, wi); scene_rules::store3(io->Le, Le);
  io->pl = pl;
  scene_rules::store3(io->hit_Le, pt_emtex_radiance(E, t, io->hit_u, io->hit_v));
  io->hit_weight = pt_emtex_hit_weight(E, io->bounce, io->prev_pdf, io->hit_t, io->hit_cos);
  return PTC_OK;
}

int ptc_debug_emissive_tex_step(ptc_ctx* c, const float* origins, const float* dirs, const float* throughput, const float* prev_pdf, const uint32_t* keys, uint32_t n,
                                uint32_t bounce, uint32_t max_bounces, float* lpath, uint8_t* out_shadow_valid, float* out_shadow10) {
  if (!c) return PTC_E_ARG;
  if (c->device >= 0 && (!origins || !dirs || !throughput || !prev_pdf || !keys || !lpath || !out_shadow_valid || !out_shadow10 || n == 0 || bounce > (1u << 20) ||
                         max_bounces > (1u << 20) || bounce > max_bounces))
    return fail(c, PTC_E_ARG, "debug_emissive_tex_step: bad argument");
  { int rc = debug_prepare(c, n, "debug_emissive_tex_step", DebugAlpha); if (rc) return rc; }      // the frame's alpha resolution of the hits, where the scene has alpha materials
  if (c->emtex.table.fixed.empty()) return fail(c, PTC_E_STATE, "debug_emissive_tex_step: the committed scene has no emission texture (ptc_set_material_emission_texture)");
  { int rc = emtex_upload(c); if (rc) return rc; }
  const Lane& ln = c->lanes[0];
  { int rc = stage_rays(c, ln.q.ray[0], n, origins, dirs, [&](uint32_t i, float4& B, float4& C) {
      B.z = throughput[i * 3]; B.w = throughput[i * 3 + 1];
      C = make_float4(throughput[i * 3 + 2], prev_pdf[i], __builtin_bit_cast(float, i), __builtin_bit_cast(float, keys[i]));
    }); if (rc) return rc; }
  std::vector<float4> L(n);
  for (uint32_t i = 0; i < n; ++i) L[i] = make_float4(lpath[i * 3], lpath[i * 3 + 1], lpath[i * 3 + 2], 0.0f);
  HIP_TRY(c, hipMemcpy(ln.q.lpath, L.data(), n * sizeof(float4), hipMemcpyHostToDevice));
  const DevQueues q = batch_queues(c, 0, n);
  const DevScene sc = lane_scene(c, 0);
  pt_launch_set_counts(ln.stream, c->cfg, q, n, 0);      // no shadow record: a launch without the sample side leaves the counts at zero
  pt_launch_trace_closest(ln.stream, c->cfg, sc, q, 0, false);
  if (alpha_on(c)) alpha_resolve_closest(c, 0, ln.stream, c->cfg, sc, q, 0, bounce, PT_ALPHA_FORM_CLOSEST, nullptr);      // as run_batch has it between closest(b) and shade(b)
  { ScopedSpan t(c, ln.stream, 8); pt_launch_shade_emissive_tex(ln.stream, sc, q, 0, bounce, max_bounces, dev_emtex(c)); }
  HIP_TRY(c, hipGetLastError());
  HIP_TRY(c, hipStreamSynchronize(ln.stream));
  HIP_TRY(c, hipMemcpy(L.data(), ln.q.lpath, n * sizeof(float4), hipMemcpyDeviceToHost));
  for (uint32_t i = 0; i < n; ++i) { lpath[i * 3] = L[i].x; lpath[i * 3 + 1] = L[i].y; lpath[i * 3 + 2] = L[i].z; }
  std::memset(out_shadow_valid, 0, n);
  std::memset(out_shadow10, 0, (size_t)n * 40);
  if (!(bounce < max_bounces && c->emtex.table.total > 0.0f)) return PTC_OK;
  return scatter_segment_records(c, q, q.seg_sh, as_rays(q.shadow), shadow_path, n, "debug_emissive_tex_step", "shadow", [&](uint32_t path, const float4& A, const float4& B, const float4& C) {
    out_shadow_valid[path] = 1;
    const float r[10] = {A.x, A.y, A.z, A.w, B.x, B.y, B.z, C.x, C.y, C.z};
    std::memcpy(out_shadow10 + (size_t)path * 10, r, sizeof r);
  });
}
}  // extern "C"
