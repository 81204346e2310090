// ptc_api_alpha.cpp — alpha coverage over the C-ABI (pt_alpha.h): the material calls, the tables of the committed scene, the lanes' alpha queues, the
// rounds of a resolution as run_batch, ptc_frame_guides and the debug hooks queue them, the statistics and the ptc_debug_alpha_* hooks.
#include "ptc_ctx.h"

using namespace ptc_detail;

namespace {
DevAlpha dev_alpha(const ptc_ctx* c) { return DevAlpha{c->alpha.bits.p, c->alpha.mode_cutoff.p, (uint32_t)c->alpha.frame_layers, c->alpha.counters.p}; }

// the lane's alpha queue with the segment layout of the batch whose queues are q
DevQueues alpha_view(const ptc_ctx* c, int l, const DevQueues& q) {
  DevQueues aq = c->lanes[(size_t)l].aq;
  aq.lpath = q.lpath;
  aq.n_seg = q.n_seg; aq.seg_len = q.seg_len;
  return aq;
}

// ptc_debug_alpha_*: what ptc_api_debug.cpp's ray hooks need — a device, the committed scene, idle lanes, the frame ended, lane 0's queues for n paths, the counters
// cleared — and the alpha tables, queues and counters of the committed scene
int alpha_debug_prepare(ptc_ctx* c, uint32_t n, const char* who) {
  { int rd = need_device(c); if (rd) return rd; }
  if (!c->committed) return fail(c, PTC_E_STATE, std::string(who) + ": scene not committed");
  { int rf = flush(c); if (rf) return rf; }
  { int rs = sync_all_lanes(c); if (rs) return rs; }
  c->in_frame = false; c->pending = 0; drop_guides(c);
  int rc = ensure_lane_queues(c, n);
  if (rc) return rc;
  for (auto& ln : c->lanes) HIP_TRY(c, hipMemset(ln.q.stats, 0, ST_N * ST_STRIDE * sizeof(unsigned long long)));
  if ((rc = alpha_upload(c))) return rc;
  if (alpha_on(c)) {
    if ((rc = ensure_alpha_queues(c))) return rc;
    HIP_TRY(c, hipMemset(c->alpha.counters.p, 0, PT_ALPHA_COUNTERS * sizeof(unsigned long long)));
  }
  c->alpha.seconds = 0.0;
  c->alpha.frame_layers = c->alpha.max_layers;
  return PTC_OK;
}
}  // namespace

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
// `with_flags` says so, one flag byte per slot in the member `flags` (a queue that lacks them is allocated anew); the small arrays (header words, per-segment counts, statistics) once.  The alpha and the glass pass each keep one.
int ensure_side_queues(ptc_ctx* c, DevQueues Lane::*queue, std::vector<void*> Lane::*owner, uint8_t* Lane::*flags, bool with_flags) {
  with_flags = with_flags && flags;
  bool grow = false;
  auto enough = [&](const Lane& ln) { return (ln.*queue).cap >= ln.q.cap && !(with_flags && ln.q.cap && !(ln.*flags)); };      // flag bytes may be asked for later than the queue
  for (auto& ln : c->lanes) grow = grow || !enough(ln);
  if (!grow) return PTC_OK;
  { int rs = sync_all_lanes(c); if (rs) return rs; }
  for (auto& ln : c->lanes) {
    if (enough(ln)) continue;
    std::vector<void*>& allocs = ln.*owner;
    free_all(allocs);
    ln.*queue = DevQueues{};
    if (flags) ln.*flags = nullptr;
    DevQueues sq{};
    const size_t slots = ptc_seg_slots(ln.q.cap, (uint32_t)c->cfg.shade_waves);
    const size_t per = PTC_MAX_SEGMENTS + 64;
    uint32_t* segs = nullptr;
    int rc = dev_alloc(c, allocs, &sq.ray[0].A, slots);
    if (!rc) rc = dev_alloc(c, allocs, &sq.ray[0].B, slots);
    if (!rc) rc = dev_alloc(c, allocs, &sq.ray[0].C, slots);
    if (!rc) rc = dev_alloc(c, allocs, &sq.hit, slots);
    if (!rc && with_flags) rc = dev_alloc(c, allocs, &(ln.*flags), slots);
    if (!rc) rc = dev_alloc(c, allocs, &sq.cnt, (size_t)CNT_N);
    if (!rc) rc = dev_alloc(c, allocs, &sq.stats, (size_t)ST_N * ST_STRIDE);
    if (!rc) rc = dev_alloc(c, allocs, &segs, 5 * per);
    if (rc) { free_all(allocs); if (flags) ln.*flags = nullptr; return rc; }
    HIP_TRY(c, hipMemset(sq.cnt, 0, CNT_N * sizeof(uint32_t)));
    HIP_TRY(c, hipMemset(sq.stats, 0, ST_N * ST_STRIDE * sizeof(unsigned long long)));
    HIP_TRY(c, hipMemset(segs, 0, 5 * per * sizeof(uint32_t)));
    sq.ray[1] = sq.ray[0];
    sq.seg_ray[0] = segs; sq.seg_ray[1] = segs + per; sq.seg_sh = segs + 2 * per; sq.pre_ray = segs + 3 * per; sq.pre_sh = segs + 4 * per;      // seg_sh stays zero: the view has no shadow queue
    sq.cap = ln.q.cap;
    ln.*queue = sq;
  }
  return PTC_OK;
}

int ensure_alpha_queues(ptc_ctx* c) { return ensure_side_queues(c, &Lane::aq, &Lane::aq_allocs, &Lane::aq_flags); }

// The host cannot know how many rays pass without a read-back, so a resolution queues every round it may need: filter, then max_layers x (scan, trace, filter).  A round
// with nothing left is three launches that find their queue empty.
void alpha_resolve_closest(ptc_ctx* c, int l, hipStream_t st, const LaunchCfg& cfg, const DevScene& sc, const DevQueues& q, int qi, uint32_t bounce, int form, uint32_t* layers_out) {
  ScopedSpan t(c, st, 5);
  const DevQueues aq = alpha_view(c, l, q);
  const DevAlpha al = dev_alpha(c);
  pt_launch_alpha_filter_closest(st, sc, q, aq, qi, bounce, al, form, /*first=*/true, layers_out);
  for (uint32_t r = 0; r < al.max_layers; ++r) {
    pt_launch_scan(st, cfg, aq, 0);
    pt_launch_trace_closest(st, cfg, sc, aq, 0, false);
    pt_launch_alpha_filter_closest(st, sc, q, aq, qi, bounce, al, form, /*first=*/false, layers_out);
  }
}

// the shadow queue of q, counted and scanned (pt_launch_scan / pt_launch_set_counts), resolved to a transmittance per record: the coarse flags by k_trace_any, then the walk —
// a record that starts at k = 0 may be traced max_layers + 1 times before it is exhausted
void alpha_resolve_shadow(ptc_ctx* c, int l, hipStream_t st, const LaunchCfg& cfg, const DevScene& sc, const DevQueues& q, float* tr_out) {
  ScopedSpan t(c, st, 5);
  const DevQueues aq = alpha_view(c, l, q);
  const DevAlpha al = dev_alpha(c);
  const uint8_t* flags = c->lanes[(size_t)l].aq_flags;
  pt_launch_trace_any(st, cfg, sc, q, c->lanes[(size_t)l].aq_flags);
  pt_launch_alpha_filter_shadow(st, sc, q, aq, al, flags, /*first=*/true, tr_out);
  for (uint32_t r = 0; r <= al.max_layers; ++r) {
    pt_launch_scan(st, cfg, aq, 0);
    pt_launch_trace_closest(st, cfg, sc, aq, 0, false);
    pt_launch_alpha_filter_shadow(st, sc, q, aq, al, flags, /*first=*/false, tr_out);
  }
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
  { int rc = alpha_debug_prepare(c, n, "debug_alpha_closest"); if (rc) return rc; }
  const Lane& ln = c->lanes[0];
  std::vector<float4> A(n), B(n), C(n);
  for (uint32_t i = 0; i < n; ++i) {
    float fi, fk; std::memcpy(&fi, &i, 4); std::memcpy(&fk, &keys[i], 4);
    A[i] = make_float4(origins[i * 3], origins[i * 3 + 1], origins[i * 3 + 2], dirs[i * 3]);
    B[i] = make_float4(dirs[i * 3 + 1], dirs[i * 3 + 2], 1.0f, 1.0f);
    C[i] = make_float4(1.0f, 0.0f, fi, fk);
  }
  HIP_TRY(c, hipMemcpy(ln.q.ray[0].A, A.data(), n * sizeof(float4), hipMemcpyHostToDevice));
  HIP_TRY(c, hipMemcpy(ln.q.ray[0].B, B.data(), n * sizeof(float4), hipMemcpyHostToDevice));
  HIP_TRY(c, hipMemcpy(ln.q.ray[0].C, C.data(), n * sizeof(float4), hipMemcpyHostToDevice));
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
  std::vector<float4> H(n);
  HIP_TRY(c, hipMemcpy(H.data(), ln.q.hit, n * sizeof(float4), hipMemcpyDeviceToHost));
  HIP_TRY(c, hipMemcpy(out_layers, layers.p, (size_t)n * 4, hipMemcpyDeviceToHost));
  for (uint32_t i = 0; i < n; ++i) {
    int32_t pc; std::memcpy(&pc, &H[i].y, 4);
    out_t[i] = H[i].x; out_prim[i] = pc < 0 ? -1 : (pc & 0x0fffffff); out_uv[i * 2] = H[i].z; out_uv[i * 2 + 1] = H[i].w;
  }
  return PTC_OK;
}

int ptc_debug_alpha_any(ptc_ctx* c, const float* origins, const float* dirs, const float* tmax, uint32_t n, float* out_transmittance) {
  if (!c) return PTC_E_ARG;
  if (c->device >= 0 && (!origins || !dirs || !tmax || !out_transmittance || n == 0)) return fail(c, PTC_E_ARG, "debug_alpha_any: bad argument");
  { int rc = alpha_debug_prepare(c, n, "debug_alpha_any"); if (rc) return rc; }
  const Lane& ln = c->lanes[0];
  std::vector<float4> A(n), B(n), C(n, make_float4(0, 0, 0, 0));
  for (uint32_t i = 0; i < n; ++i) {
    float fi; std::memcpy(&fi, &i, 4);
    A[i] = make_float4(origins[i * 3], origins[i * 3 + 1], origins[i * 3 + 2], dirs[i * 3]);
    B[i] = make_float4(dirs[i * 3 + 1], dirs[i * 3 + 2], tmax[i], fi);
  }
  HIP_TRY(c, hipMemcpy(ln.q.shadow.A, A.data(), n * sizeof(float4), hipMemcpyHostToDevice));
  HIP_TRY(c, hipMemcpy(ln.q.shadow.B, B.data(), n * sizeof(float4), hipMemcpyHostToDevice));
  HIP_TRY(c, hipMemcpy(ln.q.shadow.C, C.data(), n * sizeof(float4), hipMemcpyHostToDevice));
  DevBuf<float> tr;
  DevBuf<uint8_t> occ;
  { int rc = ensure_buf(c, tr, n); if (!rc) rc = ensure_buf(c, occ, n); if (rc) return rc; }
  HIP_TRY(c, hipMemset(tr.p, 0, (size_t)n * 4));
  const DevQueues q = batch_queues(c, 0, n);
  const DevScene sc = lane_scene(c, 0);
  pt_launch_set_counts(ln.stream, c->cfg, q, 0, n);
  if (alpha_on(c)) alpha_resolve_shadow(c, 0, ln.stream, c->cfg, sc, q, tr.p);
  else pt_launch_trace_any(ln.stream, c->cfg, sc, q, occ.p);
  HIP_TRY(c, hipGetLastError());
  HIP_TRY(c, hipStreamSynchronize(ln.stream));
  if (alpha_on(c)) HIP_TRY(c, hipMemcpy(out_transmittance, tr.p, (size_t)n * 4, hipMemcpyDeviceToHost));
  else {
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
  for (const Lane& ln : c->lanes) if (ln.aq.cap) return 1;
  return PTC_OK;
}
}  // extern "C"
