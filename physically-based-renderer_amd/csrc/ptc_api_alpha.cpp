// ptc_api_alpha.cpp — alpha coverage over the C-ABI (pt_alpha.h): the material calls, the tables of the committed scene, the lanes' alpha queues, the
// rounds of a resolution as run_batch, ptc_frame_guides and the debug hooks queue them, the statistics and the ptc_debug_alpha_* hooks.
#include "ptc_ctx.h"

using namespace ptc_detail;

namespace ptc_detail {
int alpha_upload(ptc_ctx* c) {
  if (!c->alpha.dirty) return PTC_OK;
  std::vector<uint32_t> bits; std::vector<float> mc;
  const uint32_t n = pt_alpha_tables(c->built->tri_mat, c->mats.size(), c->alpha.mode, c->alpha.cutoff, bits, mc);
  if (n) {
    int rc = ensure_buf(c, c->alpha.bits, bits.size());
    if (!rc) rc = ensure_buf(c, c->alpha.mode_cutoff, mc.size() / 2u);
    if (!rc) rc = ensure_buf(c, c->alpha.counters, (size_t)PT_ALPHA_COUNTERS);
    if (rc) return rc;
    HIP_TRY(c, hipMemcpy(c->alpha.bits.p, bits.data(), bits.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    HIP_TRY(c, hipMemcpy(c->alpha.mode_cutoff.p, mc.data(), mc.size() * sizeof(float), hipMemcpyHostToDevice));
    HIP_TRY(c, hipMemset(c->alpha.counters.p, 0, PT_ALPHA_COUNTERS * sizeof(unsigned long long)));
  }
  c->alpha.n_prims = n;
  c->alpha.dirty = false;
  return PTC_OK;
}

// A side queue per lane, as large as the lane's queues (grow only; waits for the work in flight first): 64 B of continuation and hit record per slot and, where
// `with_flags` says so, one flag byte per slot (a queue that lacks them is allocated anew); the small arrays (header words, per-segment counts, statistics) once.
// The alpha and the glass pass each keep one.
int ensure_side_queues(ptc_ctx* c, SideQueue Lane::*side, bool with_flags) {
  bool grow = false;
  auto enough = [&](const Lane& ln) { return (ln.*side).q.cap >= ln.q.cap && !(with_flags && ln.q.cap && !(ln.*side).flags); };      // flag bytes may be asked for later than the queue
  for (auto& ln : c->lanes) grow = grow || !enough(ln);
  if (!grow) return PTC_OK;
  { int rs = sync_all_lanes(c); if (rs) return rs; }
  for (auto& ln : c->lanes) {
    if (enough(ln)) continue;
    SideQueue& sd = ln.*side;
    free_all(sd.allocs);
    sd.q = DevQueues{};
    sd.flags = nullptr;
    DevQueues sq{};
    const size_t slots = ptc_seg_slots(ln.q.cap, (uint32_t)c->cfg.shade_waves);
    const size_t per = PTC_MAX_SEGMENTS + 64;
    uint32_t* segs = nullptr;
    int rc = dev_alloc(c, sd.allocs, &sq.ray[0].A, slots);
    if (!rc) rc = dev_alloc(c, sd.allocs, &sq.ray[0].B, slots);
    if (!rc) rc = dev_alloc(c, sd.allocs, &sq.ray[0].C, slots);
    if (!rc) rc = dev_alloc(c, sd.allocs, &sq.hit, slots);
    if (!rc && with_flags) rc = dev_alloc(c, sd.allocs, &sd.flags, slots);
    if (!rc) rc = dev_alloc(c, sd.allocs, &sq.cnt, (size_t)CNT_N);
    if (!rc) rc = dev_alloc(c, sd.allocs, &sq.stats, (size_t)ST_N * ST_STRIDE);
    if (!rc) rc = dev_alloc(c, sd.allocs, &segs, 5 * per);
    if (rc) { free_all(sd.allocs); sd.flags = nullptr; return rc; }
    HIP_TRY(c, hipMemset(sq.cnt, 0, CNT_N * sizeof(uint32_t)));
    HIP_TRY(c, hipMemset(sq.stats, 0, ST_N * ST_STRIDE * sizeof(unsigned long long)));
    HIP_TRY(c, hipMemset(segs, 0, 5 * per * sizeof(uint32_t)));
    sq.ray[1] = sq.ray[0];
    sq.seg_ray[0] = segs; sq.seg_ray[1] = segs + per; sq.seg_sh = segs + 2 * per; sq.pre_ray = segs + 3 * per; sq.pre_sh = segs + 4 * per;      // seg_sh stays zero: the view has no shadow queue
    sq.cap = ln.q.cap;
    sd.q = sq;
  }
  return PTC_OK;
}

int ensure_alpha_queues(ptc_ctx* c) { return ensure_side_queues(c, &Lane::alpha, /*with_flags=*/true); }

// filter, then max_layers x (scan, trace, filter)
void alpha_resolve_closest(ptc_ctx* c, int l, hipStream_t st, const LaunchCfg& cfg, const DevScene& sc, const DevQueues& q, int qi, uint32_t bounce, int form, uint32_t* layers_out) {
  ScopedSpan t(c, st, 5);
  const DevQueues aq = side_view(c->lanes[(size_t)l].alpha, q);
  const DevAlpha al = dev_alpha(c);
  resolve_rounds(st, cfg, sc, aq, al.max_layers, [&](bool first) { pt_launch_alpha_filter_closest(st, sc, q, aq, qi, bounce, al, form, first, layers_out); }, [](uint32_t) {});
}
}  // namespace ptc_detail

extern "C" {
int ptc_set_material_alpha(ptc_ctx* c, int material, int mode, float cutoff) {
  if (!c) return PTC_E_ARG;
  if (c->committed) return fail(c, PTC_E_STATE, "set_material_alpha: the scene is committed (alpha modes belong to the description: before ptc_scene_commit)");
  if (mode != PTC_ALPHA_OPAQUE && mode != PTC_ALPHA_MASK && mode != PTC_ALPHA_BLEND) return fail(c, PTC_E_ARG, "set_material_alpha: unknown mode");
  if (material < 0 || (size_t)material >= c->mats.size()) return fail(c, PTC_E_ARG, "set_material_alpha: material out of range");
  if (!(cutoff >= 0.0f && cutoff <= 1.0f)) return fail(c, PTC_E_ARG, "set_material_alpha: cutoff is not a finite number in [0, 1]");
  const HostMaterial& m = c->mats[(size_t)material];
  if (m.emissive[0] != 0.0f || m.emissive[1] != 0.0f || m.emissive[2] != 0.0f)
    return fail(c, PTC_E_ARG, "set_material_alpha: the material is emissive (emitters are sampled by area without regard to coverage: they stay opaque)");
  if (glass_tau(c, material) > 0.0f) return fail(c, PTC_E_ARG, "set_material_alpha: the material is transmissive (ptc_set_material_transmission: such a material stays OPAQUE)");
  if (mode != PTC_ALPHA_OPAQUE && emtex_has(c, material)) return fail(c, PTC_E_ARG, "set_material_alpha: the material has an emission texture (ptc_set_material_emission_texture: an emitter stays opaque)");
  if (c->alpha.mode.size() < c->mats.size()) { c->alpha.mode.resize(c->mats.size(), PTC_ALPHA_OPAQUE); c->alpha.cutoff.resize(c->mats.size(), 0.5f); }
  c->alpha.mode[(size_t)material] = mode; c->alpha.cutoff[(size_t)material] = cutoff;
  return PTC_OK;
}

int ptc_get_material_alpha(const ptc_ctx* c, int material, int* mode, float* cutoff) {
  if (!c || material < 0 || (size_t)material >= c->mats.size()) return PTC_E_ARG;
  const bool has = (size_t)material < c->alpha.mode.size();
  if (mode) *mode = has ? c->alpha.mode[(size_t)material] : (int)PTC_ALPHA_OPAQUE;
  if (cutoff) *cutoff = has ? c->alpha.cutoff[(size_t)material] : 0.5f;
  return PTC_OK;
}

int ptc_set_alpha_max_layers(ptc_ctx* c, int n) {
  if (!c) return PTC_E_ARG;
  if (n < 1 || n > PT_ALPHA_MAX_LAYERS) return fail(c, PTC_E_ARG, "set_alpha_max_layers: 1 .. 16");
  c->alpha.max_layers = n;
  return PTC_OK;
}

int ptc_get_alpha_stats(ptc_ctx* c, ptc_alpha_stats* out) {
  if (!c) return PTC_E_ARG;
  if (!out) return fail(c, PTC_E_ARG, "get_alpha_stats: null pointer");
  std::memset(out, 0, sizeof *out);
  if (c->device < 0) return PTC_OK;
  ptc_stats unused;
  { int rc = ptc_get_stats(c, &unused); if (rc) return rc; }      // flushes, waits and collects the timing spans
  if (c->alpha.counters.p) {
    unsigned long long v[PT_ALPHA_COUNTERS];
    HIP_TRY(c, hipMemcpy(v, c->alpha.counters.p, sizeof v, hipMemcpyDeviceToHost));
    out->closest_passes = v[PT_ALPHA_CLOSEST_PASSES]; out->shadow_walked = v[PT_ALPHA_SHADOW_WALKED]; out->shadow_passes = v[PT_ALPHA_SHADOW_PASSES]; out->exhausted = v[PT_ALPHA_EXHAUSTED];
  }
  out->seconds_alpha = c->alpha.seconds;
  return PTC_OK;
}

// ---- test hooks -------------------------------------------------------------------------------------------------------------------------------------
int ptc_debug_alpha_closest(ptc_ctx* c, const float* origins, const float* dirs, const uint32_t* keys, uint32_t n, uint32_t bounce, int deterministic,
                            float* out_t, int32_t* out_prim, float* out_uv, uint32_t* out_layers) {
  if (!c) return PTC_E_ARG;
  if (c->device >= 0 && (!origins || !dirs || !keys || !out_t || !out_prim || !out_uv || !out_layers || n == 0 || bounce > 0x0fffffffu)) return fail(c, PTC_E_ARG, "debug_alpha_closest: bad argument");
  { int rc = debug_prepare(c, n, "debug_alpha_closest", DebugAlpha); if (rc) return rc; }
  const Lane& ln = c->lanes[0];
  { int rc = stage_rays(c, ln.q.ray[0], n, origins, dirs, [&](uint32_t i, float4& B, float4& C) {
      B.z = B.w = 1.0f; C = make_float4(1.0f, 0.0f, __builtin_bit_cast(float, i), __builtin_bit_cast(float, keys[i]));
    }); if (rc) return rc; }
  DevBuf<uint32_t> layers;
  { int rc = ensure_buf(c, layers, n); if (rc) return rc; }
  HIP_TRY(c, hipMemset(layers.p, 0, (size_t)n * 4));
  const DevQueues q = batch_queues(c, 0, n);
  const DevScene sc = lane_scene(c, 0);
  pt_launch_set_counts(ln.stream, c->cfg, q, n, 0);
  pt_launch_trace_closest(ln.stream, c->cfg, sc, q, 0, false);
  if (alpha_on(c)) alpha_resolve_closest(c, 0, ln.stream, c->cfg, sc, q, 0, bounce, deterministic ? PT_ALPHA_FORM_GUIDE : PT_ALPHA_FORM_CLOSEST, layers.p);
  HIP_TRY(c, hipGetLastError());
  HIP_TRY(c, hipStreamSynchronize(ln.stream));
  HIP_TRY(c, hipMemcpy(out_layers, layers.p, (size_t)n * 4, hipMemcpyDeviceToHost));
  return read_hits(c, n, out_t, out_prim, out_uv);
}

int ptc_debug_alpha_any(ptc_ctx* c, const float* origins, const float* dirs, const float* tmax, uint32_t n, float* out_transmittance) {
  if (!c) return PTC_E_ARG;
  if (c->device >= 0 && (!origins || !dirs || !tmax || !out_transmittance || n == 0)) return fail(c, PTC_E_ARG, "debug_alpha_any: bad argument");
  { int rc = debug_prepare(c, n, "debug_alpha_any", DebugAlpha); if (rc) return rc; }
  const Lane& ln = c->lanes[0];
  { int rc = stage_rays(c, as_rays(ln.q.shadow), n, origins, dirs, [&](uint32_t i, float4& B, float4&) { B.z = tmax[i]; B.w = __builtin_bit_cast(float, i); }); if (rc) return rc; }
  DevBuf<float> tr;
  DevBuf<uint8_t> occ;
  { int rc = ensure_buf(c, tr, (size_t)n * 3u); if (!rc) rc = ensure_buf(c, occ, n); if (rc) return rc; }
  HIP_TRY(c, hipMemset(tr.p, 0, (size_t)n * 12));
  const DevQueues q = batch_queues(c, 0, n);
  const DevScene sc = lane_scene(c, 0);
  pt_launch_set_counts(ln.stream, c->cfg, q, 0, n);
  if (alpha_on(c)) resolve_shadow(c, 0, ln.stream, c->cfg, sc, q, /*through_glass=*/false, tr.p, nullptr);
  else pt_launch_trace_any(ln.stream, c->cfg, sc, q, occ.p);
  HIP_TRY(c, hipGetLastError());
  HIP_TRY(c, hipStreamSynchronize(ln.stream));
  if (alpha_on(c)) {      // the walk's three channels are equal without glass: channel 0
    std::vector<float> t3((size_t)n * 3u);
    HIP_TRY(c, hipMemcpy(t3.data(), tr.p, (size_t)n * 12, hipMemcpyDeviceToHost));
    for (uint32_t i = 0; i < n; ++i) out_transmittance[i] = t3[(size_t)i * 3u];
  } else {
    std::vector<uint8_t> o(n);
    HIP_TRY(c, hipMemcpy(o.data(), occ.p, n, hipMemcpyDeviceToHost));
    for (uint32_t i = 0; i < n; ++i) out_transmittance[i] = o[i] ? 0.0f : 1.0f;
  }
  return PTC_OK;
}

int ptc_debug_alpha_decide(int mode, float cutoff, float a, float u, int* accept, float* transmit) {
  if (mode != PTC_ALPHA_OPAQUE && mode != PTC_ALPHA_MASK && mode != PTC_ALPHA_BLEND) return PTC_E_ARG;
  if (accept) *accept = pt_alpha_accept(mode, cutoff, a, u) ? 1 : 0;
  if (transmit) *transmit = pt_alpha_transmit(mode, cutoff, a);
  return PTC_OK;
}

int ptc_debug_get_alpha_tables(ptc_ctx* c, uint32_t* n_prims, uint32_t* bits, uint32_t* n_mats, float* mode_cutoff) {
  if (!c) return PTC_E_ARG;
  if (!c->committed) return fail(c, PTC_E_STATE, "debug_get_alpha_tables: scene not committed");
  std::vector<uint32_t> b; std::vector<float> mc;
  pt_alpha_tables(c->built->tri_mat, c->mats.size(), c->alpha.mode, c->alpha.cutoff, b, mc);
  if (n_prims) *n_prims = (uint32_t)c->built->tri_mat.size();
  if (n_mats) *n_mats = (uint32_t)c->mats.size();
  if (bits && !b.empty()) std::memcpy(bits, b.data(), b.size() * sizeof(uint32_t));
  if (mode_cutoff && !mc.empty()) std::memcpy(mode_cutoff, mc.data(), mc.size() * sizeof(float));
  for (const Lane& ln : c->lanes) if (ln.alpha.q.cap) return 1;
  return PTC_OK;
}
}  // extern "C"
