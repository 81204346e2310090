// ptc_api_glass.cpp — dielectric transmission over the C-ABI (pt_glass.h): the material calls, the tables of the committed scene, the lanes' glass
// queues, the rounds of a resolution as run_batch and the debug hooks queue them, the statistics and the ptc_debug_glass_* hooks; and transparent shadows
// (pt_glass_shadow.h, include/ptc_glass_shadows.h): the setting, the rounds of the shadow walk, its statistics and hooks.
#include "ptc_ctx.h"

#include <cmath>

using namespace ptc_detail;

namespace {
DevGlass dev_glass(const ptc_ctx* c) { return DevGlass{c->glass.bits.p, c->glass.mats.p, (uint32_t)c->glass.frame_interactions, c->glass.counters.p}; }

void glass_tables(const ptc_ctx* c, std::vector<uint32_t>& bits, std::vector<pt_glass_mat>& mats, uint32_t& n) {
  n = pt_glass_tables(c->built->tri_mat, c->mats.size(), c->glass.params, bits, mats);
}
}  // namespace

namespace ptc_detail {
int glass_upload(ptc_ctx* c) {
  if (!c->glass.dirty) return PTC_OK;
  std::vector<uint32_t> bits; std::vector<pt_glass_mat> mats;
  uint32_t n = 0;
  glass_tables(c, bits, mats, n);
  if (n) {
    static_assert(sizeof(pt_glass_mat) == 32, "two 16-byte units per material");
    int rc = ensure_buf(c, c->glass.bits, bits.size());
    if (!rc) rc = ensure_buf(c, c->glass.mats, mats.size() * 2u);
    if (!rc) rc = ensure_buf(c, c->glass.counters, (size_t)PT_GLASS_COUNTERS);
    if (!rc) rc = ensure_buf(c, c->glass.shadow_counters, (size_t)PT_GLASS_SHADOW_COUNTERS);
    if (rc) return rc;
    HIP_TRY(c, hipMemcpy(c->glass.bits.p, bits.data(), bits.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    HIP_TRY(c, hipMemcpy(c->glass.mats.p, mats.data(), mats.size() * sizeof(pt_glass_mat), hipMemcpyHostToDevice));
    HIP_TRY(c, hipMemset(c->glass.counters.p, 0, PT_GLASS_COUNTERS * sizeof(unsigned long long)));
    HIP_TRY(c, hipMemset(c->glass.shadow_counters.p, 0, PT_GLASS_SHADOW_COUNTERS * sizeof(unsigned long long)));
  }
  uint32_t n_thin = 0;
  for (const int32_t m : c->built->tri_mat) n_thin += m >= 0 && (size_t)m < mats.size() && mats[(size_t)m].tau > 0.0f && mats[(size_t)m].thin != 0;
  c->glass.n_thin = n_thin;
  c->glass.n_prims = n;
  c->glass.dirty = false;
  return PTC_OK;
}

// flag bytes only for a frame (or ray hook) that walks its shadow records through thin panes: turning the feature on after frames have run allocates the queue anew
int ensure_glass_queues(ptc_ctx* c) { return ensure_side_queues(c, &Lane::glass, glass_shadows_on(c)); }

// filter, then max_interactions x (scan, trace, [alpha], filter).  In round r the continuations' hits are first resolved by the alpha pass on the glass view; its
// bounce argument only enters alpha's RNG index, and the value gives fresh numbers per interaction.
void glass_resolve_closest(ptc_ctx* c, int l, hipStream_t st, const LaunchCfg& cfg, const DevScene& sc, const DevQueues& q, int qi, uint32_t bounce, uint32_t* j_out) {
  ScopedSpan t(c, st, 6);
  const DevQueues gq = side_view(c->lanes[(size_t)l].glass, q);
  const DevGlass gl = dev_glass(c);
  const bool alpha = alpha_on(c), shadows = glass_shadows_on(c);
  resolve_rounds(st, cfg, sc, gq, gl.max_interactions, [&](bool first) { pt_launch_glass_filter(st, sc, q, gq, qi, bounce, gl, first, shadows, j_out); },
                 [&](uint32_t r) { if (alpha) alpha_resolve_closest(c, l, st, cfg, sc, gq, 0, 0x01000000u + (bounce + 1u) * 64u + r, PT_ALPHA_FORM_CLOSEST, nullptr); });
}

// a record that starts at k = 0 may be traced L + 1 times before it is exhausted: L is the frame's max_layers for alpha's own walk; through glass, the larger of its
// max_interactions and, in a scene with alpha materials, its max_layers
void resolve_shadow(ptc_ctx* c, int l, hipStream_t st, const LaunchCfg& cfg, const DevScene& sc, const DevQueues& q, bool through_glass, float* tr3_out, uint32_t* layers_out) {
  ScopedSpan t(c, st, through_glass ? 6 : 5);
  const SideQueue& side = through_glass ? c->lanes[(size_t)l].glass : c->lanes[(size_t)l].alpha;
  const DevQueues sq = side_view(side, q);
  const DevAlpha al = alpha_on(c) ? dev_alpha(c) : DevAlpha{nullptr, nullptr, 0u, nullptr};
  const DevGlass gl = through_glass ? dev_glass(c) : DevGlass{nullptr, nullptr, 0u, nullptr};
  const uint32_t L = al.max_layers > gl.max_interactions ? al.max_layers : gl.max_interactions;
  unsigned long long *a = c->alpha.counters.p, *g = c->glass.shadow_counters.p;
  const ShadowWalkCounters ctr = through_glass ? ShadowWalkCounters{g + PT_GLASS_SHADOW_WALKED, g + PT_GLASS_SHADOW_PASSES, g + PT_GLASS_SHADOW_VISIBLE, g + PT_GLASS_SHADOW_EXHAUSTED}
                                               : ShadowWalkCounters{a + PT_ALPHA_SHADOW_WALKED, a + PT_ALPHA_SHADOW_PASSES, nullptr, a + PT_ALPHA_EXHAUSTED};
  pt_launch_trace_any(st, cfg, sc, q, side.flags);
  resolve_rounds(st, cfg, sc, sq, L + 1u, [&](bool first) { pt_launch_glass_filter_shadow(st, sc, q, sq, al, gl, L, ctr, side.flags, first, tr3_out, layers_out); }, [](uint32_t) {});
}
}  // namespace ptc_detail

extern "C" {
void ptc_transmission_default_params(ptc_transmission_params* out) {
  if (!out) return;
  out->transmission = 0.0f; out->ior = 1.5f; out->thin_walled = 1;
  out->attenuation_color[0] = out->attenuation_color[1] = out->attenuation_color[2] = 1.0f;
  out->attenuation_distance = 0.0f;
}

int ptc_set_material_transmission(ptc_ctx* c, int material, const ptc_transmission_params* p) {
  if (!c) return PTC_E_ARG;
  if (c->committed) return fail(c, PTC_E_STATE, "set_material_transmission: the scene is committed (transmission belongs to the description: before ptc_scene_commit)");
  if (!p) return fail(c, PTC_E_ARG, "set_material_transmission: null pointer");
  if (material < 0 || (size_t)material >= c->mats.size()) return fail(c, PTC_E_ARG, "set_material_transmission: material out of range");
  if (!(p->transmission >= 0.0f && p->transmission <= 1.0f)) return fail(c, PTC_E_ARG, "set_material_transmission: transmission is not a number in [0, 1]");
  if (!(p->ior >= 1.0f) || !std::isfinite(p->ior)) return fail(c, PTC_E_ARG, "set_material_transmission: ior is not a finite number >= 1");
  if (p->thin_walled != 0 && p->thin_walled != 1) return fail(c, PTC_E_ARG, "set_material_transmission: thin_walled is 0 or 1");
  for (int k = 0; k < 3; ++k)
    if (!(p->attenuation_color[k] > 0.0f && p->attenuation_color[k] <= 1.0f)) return fail(c, PTC_E_ARG, "set_material_transmission: attenuation_color is not in (0, 1]");
  if (!(p->attenuation_distance >= 0.0f) || !std::isfinite(p->attenuation_distance)) return fail(c, PTC_E_ARG, "set_material_transmission: attenuation_distance is not a finite number >= 0");
  const HostMaterial& m = c->mats[(size_t)material];
  if (m.emissive[0] != 0.0f || m.emissive[1] != 0.0f || m.emissive[2] != 0.0f)
    return fail(c, PTC_E_ARG, "set_material_transmission: the material is emissive (emitters are sampled by area as opaque surfaces)");
  if ((size_t)material < c->alpha.mode.size() && c->alpha.mode[(size_t)material] != PTC_ALPHA_OPAQUE)
    return fail(c, PTC_E_ARG, "set_material_transmission: the material's alpha mode is not OPAQUE");
  if (p->transmission > 0.0f && emtex_has(c, material))
    return fail(c, PTC_E_ARG, "set_material_transmission: the material has an emission texture (ptc_set_material_emission_texture: an emitter stays opaque)");
  if (c->glass.params.size() < c->mats.size()) {
    ptc_transmission_params def;
    ptc_transmission_default_params(&def);
    c->glass.params.resize(c->mats.size(), def);
  }
  c->glass.params[(size_t)material] = *p;
  return PTC_OK;
}

int ptc_get_material_transmission(const ptc_ctx* c, int material, ptc_transmission_params* out) {
  if (!c || !out || material < 0 || (size_t)material >= c->mats.size()) return PTC_E_ARG;
  if ((size_t)material < c->glass.params.size()) *out = c->glass.params[(size_t)material];
  else ptc_transmission_default_params(out);
  return PTC_OK;
}

int ptc_set_glass_max_interactions(ptc_ctx* c, int n) {
  if (!c) return PTC_E_ARG;
  if (n < 1 || n > PT_GLASS_MAX_INTERACTIONS) return fail(c, PTC_E_ARG, "set_glass_max_interactions: 1 .. 32");
  c->glass.max_interactions = n;
  return PTC_OK;
}

int ptc_set_glass_shadows(ptc_ctx* c, int on) {
  if (!c) return PTC_E_ARG;
  if (on != 0 && on != 1) return fail(c, PTC_E_ARG, "set_glass_shadows: 0 or 1");
  c->glass.shadows = on;
  return PTC_OK;
}

int ptc_get_glass_shadows(const ptc_ctx* c, int* on) {
  if (!c || !on) return PTC_E_ARG;
  *on = c->glass.shadows;
  return PTC_OK;
}

int ptc_get_glass_shadow_stats(ptc_ctx* c, ptc_glass_shadow_stats* out) {
  if (!c) return PTC_E_ARG;
  if (!out) return fail(c, PTC_E_ARG, "get_glass_shadow_stats: null pointer");
  std::memset(out, 0, sizeof *out);
  if (c->device < 0) return PTC_OK;
  ptc_stats unused;
  { int rc = ptc_get_stats(c, &unused); if (rc) return rc; }      // flushes and waits
  if (c->glass.shadow_counters.p) {
    unsigned long long v[PT_GLASS_SHADOW_COUNTERS];
    HIP_TRY(c, hipMemcpy(v, c->glass.shadow_counters.p, sizeof v, hipMemcpyDeviceToHost));
    out->walked = v[PT_GLASS_SHADOW_WALKED]; out->passes = v[PT_GLASS_SHADOW_PASSES]; out->visible = v[PT_GLASS_SHADOW_VISIBLE]; out->exhausted = v[PT_GLASS_SHADOW_EXHAUSTED];
  }
  return PTC_OK;
}

int ptc_get_glass_stats(ptc_ctx* c, ptc_glass_stats* out) {
  if (!c) return PTC_E_ARG;
  if (!out) return fail(c, PTC_E_ARG, "get_glass_stats: null pointer");
  std::memset(out, 0, sizeof *out);
  if (c->device < 0) return PTC_OK;
  ptc_stats unused;
  { int rc = ptc_get_stats(c, &unused); if (rc) return rc; }      // flushes, waits and collects the timing spans
  if (c->glass.counters.p) {
    unsigned long long v[PT_GLASS_COUNTERS];
    HIP_TRY(c, hipMemcpy(v, c->glass.counters.p, sizeof v, hipMemcpyDeviceToHost));
    out->reflections = v[PT_GLASS_REFLECTIONS]; out->refractions = v[PT_GLASS_REFRACTIONS]; out->standing = v[PT_GLASS_STANDING]; out->exhausted = v[PT_GLASS_EXHAUSTED_N];
  }
  out->seconds_glass = c->glass.seconds;
  return PTC_OK;
}

// ---- test hooks -------------------------------------------------------------------------------------------------------------------------------------
int ptc_debug_glass_closest(ptc_ctx* c, const float* origins, const float* dirs, const uint32_t* keys, uint32_t n, uint32_t bounce,
                            float* out_t, int32_t* out_prim, float* out_uv, float* out_ray10, uint32_t* out_j) {
  if (!c) return PTC_E_ARG;
  if (c->device >= 0 && (!origins || !dirs || !keys || !out_t || !out_prim || !out_uv || !out_ray10 || !out_j || n == 0 || bounce > 0x0000ffffu)) return fail(c, PTC_E_ARG, "debug_glass_closest: bad argument");
  int rc = debug_prepare(c, n, "debug_glass_closest", DebugAlphaGlass);
  if (rc) return rc;
  const Lane& ln = c->lanes[0];
  if ((rc = stage_rays(c, ln.q.ray[0], n, origins, dirs, [&](uint32_t i, float4& B, float4& C) {
         B.z = B.w = 1.0f; C = make_float4(1.0f, 1.0f, __builtin_bit_cast(float, i), __builtin_bit_cast(float, keys[i]));
       }))) return rc;
  DevBuf<uint32_t> jn;
  if ((rc = ensure_buf(c, jn, n))) return rc;
  HIP_TRY(c, hipMemset(jn.p, 0, (size_t)n * 4));
  const DevQueues q = batch_queues(c, 0, n);
  const DevScene sc = lane_scene(c, 0);
  pt_launch_set_counts(ln.stream, c->cfg, q, n, 0);
  pt_launch_trace_closest(ln.stream, c->cfg, sc, q, 0, false);
  if (alpha_on(c)) alpha_resolve_closest(c, 0, ln.stream, c->cfg, sc, q, 0, bounce, PT_ALPHA_FORM_CLOSEST, nullptr);
  if (glass_on(c)) glass_resolve_closest(c, 0, ln.stream, c->cfg, sc, q, 0, bounce, jn.p);
  HIP_TRY(c, hipGetLastError());
  HIP_TRY(c, hipStreamSynchronize(ln.stream));
  std::vector<float4> A(n), B(n), C(n);
  HIP_TRY(c, hipMemcpy(A.data(), ln.q.ray[0].A, n * sizeof(float4), hipMemcpyDeviceToHost));
  HIP_TRY(c, hipMemcpy(B.data(), ln.q.ray[0].B, n * sizeof(float4), hipMemcpyDeviceToHost));
  HIP_TRY(c, hipMemcpy(C.data(), ln.q.ray[0].C, n * sizeof(float4), hipMemcpyDeviceToHost));
  HIP_TRY(c, hipMemcpy(out_j, jn.p, (size_t)n * 4, hipMemcpyDeviceToHost));
  for (uint32_t i = 0; i < n; ++i) {
    float* r = out_ray10 + (size_t)i * 10;
    r[0] = A[i].x; r[1] = A[i].y; r[2] = A[i].z; r[3] = A[i].w; r[4] = B[i].x; r[5] = B[i].y; r[6] = B[i].z; r[7] = B[i].w; r[8] = C[i].x; r[9] = C[i].y;
  }
  return read_hits(c, n, out_t, out_prim, out_uv);
}

int ptc_debug_glass_any(ptc_ctx* c, const float* origins, const float* dirs, const float* tmax, uint32_t n, float* out_tr3, uint32_t* out_layers) {
  if (!c) return PTC_E_ARG;
  if (c->device >= 0 && (!origins || !dirs || !tmax || !out_tr3 || !out_layers || n == 0)) return fail(c, PTC_E_ARG, "debug_glass_any: bad argument");
  { int rc = debug_prepare(c, n, "debug_glass_any", DebugAlphaGlass); if (rc) return rc; }
  const Lane& ln = c->lanes[0];
  { int rc = stage_rays(c, as_rays(ln.q.shadow), n, origins, dirs, [&](uint32_t i, float4& B, float4&) { B.z = tmax[i]; B.w = __builtin_bit_cast(float, i); }); if (rc) return rc; }
  DevBuf<float> tr;
  DevBuf<uint32_t> layers;
  DevBuf<uint8_t> occ;
  { int rc = ensure_buf(c, tr, (size_t)n * 3u); if (!rc) rc = ensure_buf(c, layers, n); if (!rc) rc = ensure_buf(c, occ, n); if (rc) return rc; }
  HIP_TRY(c, hipMemset(tr.p, 0, (size_t)n * 12));
  HIP_TRY(c, hipMemset(layers.p, 0, (size_t)n * 4));
  const DevQueues q = batch_queues(c, 0, n);
  const DevScene sc = lane_scene(c, 0);
  const bool walk = glass_shadows_on(c);
  pt_launch_set_counts(ln.stream, c->cfg, q, 0, n);
  if (walk) resolve_shadow(c, 0, ln.stream, c->cfg, sc, q, /*through_glass=*/true, tr.p, layers.p);
  else pt_launch_trace_any(ln.stream, c->cfg, sc, q, occ.p);
  HIP_TRY(c, hipGetLastError());
  HIP_TRY(c, hipStreamSynchronize(ln.stream));
  HIP_TRY(c, hipMemcpy(out_layers, layers.p, (size_t)n * 4, hipMemcpyDeviceToHost));
  if (walk) HIP_TRY(c, hipMemcpy(out_tr3, tr.p, (size_t)n * 12, hipMemcpyDeviceToHost));
  else {
    std::vector<uint8_t> o(n);
    HIP_TRY(c, hipMemcpy(o.data(), occ.p, n, hipMemcpyDeviceToHost));
    for (uint32_t i = 0; i < n * 3u; ++i) out_tr3[i] = o[i / 3u] ? 0.0f : 1.0f;
  }
  return PTC_OK;
}

int ptc_debug_glass_shadow_transmit(const ptc_transmission_params* p, ptc_glass_shadow_hit* io) {
  if (!p || !io) return PTC_E_ARG;
  const pt_glass_mat m = pt_glass_make_mat(*p);
  float F_t = 0.0f;
  const v3 W = pt_glass_shadow_transmit(m, V3(io->ng), V3(io->ns), V3(io->d), V3(io->base), io->metallic, F_t);
  io->W[0] = W.x; io->W[1] = W.y; io->W[2] = W.z;
  io->F_t = F_t;
  return PTC_OK;
}

int ptc_debug_glass_interact(const ptc_transmission_params* p, ptc_glass_interaction* io) {
  if (!p || !io || !std::isfinite(io->t)) return PTC_E_ARG;      // a hit record's t is finite
  const pt_glass_mat m = pt_glass_make_mat(*p);
  v3 o = V3(0.0f, 0.0f, 0.0f), d = V3(io->d), T = V3(io->T);
  const bool front = io->front != 0;
  pt_glass_beer(m, front, io->t, T);
  float F = 0.0f;
  io->outcome = pt_glass_interact(m, V3(io->P), V3(io->ng), V3(io->ns), front, V3(io->base), io->metallic, io->ray_eps, io->u_s, io->u_e, io->j, io->max_interactions, o, d, T, F);
  io->o_out[0] = o.x; io->o_out[1] = o.y; io->o_out[2] = o.z;
  io->d_out[0] = d.x; io->d_out[1] = d.y; io->d_out[2] = d.z;
  io->T_out[0] = T.x; io->T_out[1] = T.y; io->T_out[2] = T.z;
  io->F = F;
  return PTC_OK;
}

int ptc_debug_get_glass_tables(ptc_ctx* c, uint32_t* n_prims, uint32_t* bits, uint32_t* n_mats, float* mats8) {
  if (!c) return PTC_E_ARG;
  if (!c->committed) return fail(c, PTC_E_STATE, "debug_get_glass_tables: scene not committed");
  std::vector<uint32_t> b; std::vector<pt_glass_mat> m;
  uint32_t n = 0;
  glass_tables(c, b, m, n);
  if (n_prims) *n_prims = (uint32_t)c->built->tri_mat.size();
  if (n_mats) *n_mats = (uint32_t)c->mats.size();
  if (bits && !b.empty()) std::memcpy(bits, b.data(), b.size() * sizeof(uint32_t));
  if (mats8 && !m.empty()) std::memcpy(mats8, m.data(), m.size() * sizeof(pt_glass_mat));
  for (const Lane& ln : c->lanes) if (ln.glass.q.cap) return 1;
  return PTC_OK;
}
}  // extern "C"
