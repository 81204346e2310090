// ptc_api_image.cpp — the image-space half of the C-ABI: first-hit guides, the three denoise entries, temporal accumulation, adaptive sampling and the sample
// covariance, the display transform, light probes.  Each feature keeps its state in its own member of ptc_ctx (ptc_ctx.h).
#include "ptc_ctx.h"

using namespace ptc_detail;

namespace ptc_detail {
DevAdaptive dev_adaptive(const ptc_ctx* c) {
  return DevAdaptive{c->adaptive.mom.p, c->adaptive.count.p, c->adaptive.flags.p, c->adaptive.keep.p, c->adaptive.block.p, c->adaptive.n.p, c->adaptive.cov_on ? c->adaptive.cov4.p : nullptr, c->adaptive.cov_on ? c->adaptive.cov2.p : nullptr};
}

// A refit or a rebuild is about to overwrite the shading records.  A live temporal history whose frame saw the records as they lie now keeps their positions: the
// next ptc_temporal_accumulate needs where every primitive WAS.  Queued on stream 0; the callers wait for the lanes before they touch the scene.  A static scene
// never comes here, and of several refits between two accumulates only the first copies.
int temporal_keep_positions(ptc_ctx* c) {
  if (!c->temporal.live || c->temporal.snap_current || c->device < 0) return PTC_OK;
  const uint32_t n_prims = c->built->n_tris;
  int rc = ensure_buf(c, c->temporal.snap, (size_t)3 * n_prims);
  if (rc) return rc;
  pt_launch_temporal_snapshot(c->lanes[0].stream, c->scene.dsc.shade, c->scene.dsc.shade_stride, n_prims, c->temporal.snap.p);
  HIP_TRY(c, hipGetLastError());
  c->temporal.snap_current = true;
  return PTC_OK;
}
}  // namespace ptc_detail

extern "C" {
// ---- first-hit guide buffers + the variance-guided à-trous denoiser (pt_denoise.hip) -----------------------------------------

int ptc_frame_guides(ptc_ctx* c) {
  { int rd = need_device(c); if (rd) return rd; }
  if (!c->in_frame) return fail(c, PTC_E_STATE, "frame_guides: no frame");
  if (entry_frame(c)) return fail(c, PTC_E_STATE, "frame_guides: a probe or lightmap frame has no camera image to guide");
  if (c->integrator != PTC_INTEGRATOR_PATH) return fail(c, PTC_E_STATE, "frame_guides: the frame is not a PTC_INTEGRATOR_PATH frame (the raster integrators are noise-free)");
  const uint32_t n = (uint32_t)c->fr.w * (uint32_t)c->fr.h;      // every pixel, whatever the frame's tile share: the root of a sharded frame denoises the whole image
  int rc;
  if ((rc = ensure_buf(c, c->guides.albedo, n)) || (rc = ensure_buf(c, c->guides.normal, n)) || (rc = ensure_buf(c, c->guides.pos, n)) || (rc = ensure_buf(c, c->guides.prim, n)) ||
      (rc = ensure_buf(c, c->guides.uv, n))) return rc;
  if (!c->guides.stats.p) {
    if ((rc = ensure_buf(c, c->guides.stats, (size_t)ST_N * ST_STRIDE))) return rc;
    HIP_TRY(c, hipMemset(c->guides.stats.p, 0, ST_N * ST_STRIDE * sizeof(unsigned long long)));
  }
  // The guide rays borrow lane 0's queues between two batches (a batch leaves nothing in them: its radiance is in the sums once k_accumulate ran) and are
  // traced in chunks of what the lane holds; a lane without queues yet gets them for one sample per pixel, at most 2 M paths.
  {
    const uint32_t want = n < (1u << 21) ? n : (1u << 21);
    if (c->lanes[0].q.cap < want && (rc = ensure_lane_queues(c, want))) return rc;
    if (alpha_on(c) && (rc = ensure_alpha_queues(c))) return rc;
  }
  Lane& ln = c->lanes[0];
  hipStream_t st = ln.stream;
  const DevScene sc = lane_scene(c, 0);
  const GuideBufs g = c->guides.dev();
  const PtCamProj proj = cam_proj(c);
  const uint32_t chunk = ln.q.cap < n ? ln.q.cap : n;
  if ((rc = c->guides.timer.begin(c, st))) return rc;
  for (uint32_t first = 0; first < n; first += chunk) {
    const uint32_t m = n - first < chunk ? n - first : chunk;
    DevQueues q = batch_queues(c, 0, m);
    q.stats = c->guides.stats.p;            // the frame's counters do not see the guide rays
    const LaunchCfg cfg = batch_cfg(c, m);
    pt_launch_set_counts(st, cfg, q, m, 0);
    if (proj.projection != PTC_PROJ_PERSPECTIVE) pt_launch_raygen_guides_proj(st, c->cam, proj, c->fr.w, c->fr.h, first, m, q);      // pt_camera.hip
    else pt_launch_raygen_guides(st, c->cam, c->fr.w, c->fr.h, first, m, q);
    pt_launch_trace_closest(st, cfg, sc, q, 0, false);
    if (alpha_on(c)) alpha_resolve_closest(c, 0, st, cfg, sc, q, 0, 0, PT_ALPHA_FORM_GUIDE, nullptr);      // the first COVERING surface, decided without random numbers
    pt_launch_guides(st, sc, c->cam, c->fr.w, c->fr.h, first, m, q, g);
    if (proj.projection != PTC_PROJ_PERSPECTIVE) pt_launch_guides_pos_proj(st, c->cam, proj, c->fr.w, c->fr.h, first, m, g.normal_depth, g.pos_class);      // k_guides took the ray for a perspective one in this field alone
  }
  if ((rc = c->guides.timer.end(c, st))) return rc;
  HIP_TRY(c, hipGetLastError());
  c->guides.valid = true;
  return PTC_OK;
}

int ptc_read_guide_rgba32f(ptc_ctx* c, int which, float* out) {
  return read_image(c, "read_guide", out, sizeof(float4), /*all_lanes=*/false, [&](const void*& src) -> int {
    if (which != PTC_GUIDE_ALBEDO && which != PTC_GUIDE_NORMAL_DEPTH) return fail(c, PTC_E_ARG, "read_guide: unknown guide");
    if (!c->guides.valid) return fail(c, PTC_E_STATE, "read_guide: no guides (ptc_frame_guides)");
    src = which == PTC_GUIDE_ALBEDO ? c->guides.albedo.p : c->guides.normal.p;
    return PTC_OK;
  });
}

int ptc_read_guide_hit(ptc_ctx* c, int32_t* prim, float* uv) {
  { int rd = need_device(c); if (rd) return rd; }
  if (!c->guides.valid) return fail(c, PTC_E_STATE, "read_guide_hit: no guides (ptc_frame_guides)");
  HIP_TRY(c, hipStreamSynchronize(c->lanes[0].stream));
  const size_t n = (size_t)c->rad_w * c->rad_h;
  if (prim) HIP_TRY(c, hipMemcpy(prim, c->guides.prim.p, n * sizeof(int32_t), hipMemcpyDeviceToHost));
  if (uv) HIP_TRY(c, hipMemcpy(uv, c->guides.uv.p, n * sizeof(float2), hipMemcpyDeviceToHost));
  return PTC_OK;
}

int ptc_focus_distance_at_pixel(ptc_ctx* c, int px, int py, float* out) {
  if (c) { const std::string why = projection_refusal(c, "focus_distance_at_pixel", "the view depth of a pixel"); if (!why.empty()) return fail(c, PTC_E_STATE, why); }      // before the device: a description-only context can tell
  { int rd = need_device(c); if (rd) return rd; }
  if (!out) return fail(c, PTC_E_ARG, "focus_distance_at_pixel: null pointer");
  if (entry_frame(c)) return fail(c, PTC_E_STATE, "focus_distance_at_pixel: a probe or lightmap frame has no camera image");
  if (!c->guides.valid) return fail(c, PTC_E_STATE, "focus_distance_at_pixel: no guides (ptc_frame_guides)");
  const int w = c->rad_w, h = c->rad_h;
  if (px < 0 || py < 0 || px >= w || py >= h) return fail(c, PTC_E_ARG, "focus_distance_at_pixel: pixel outside the frame");
  HIP_TRY(c, hipStreamSynchronize(c->lanes[0].stream));
  float4 nz;
  HIP_TRY(c, hipMemcpy(&nz, c->guides.normal.p + ((size_t)py * (size_t)w + (size_t)px), sizeof nz, hipMemcpyDeviceToHost));
  // the pixel-centre ray of k_raygen_guides: Z is t along the unit ray, the view depth is t over the length of (dvx, dvy, 1)
  const float fx = ((float)px + 0.5f) / (float)w, fy = ((float)py + 0.5f) / (float)h;
  const float dvx = (2.0f * fx - 1.0f) * c->cam.sx, dvy = (2.0f * fy - 1.0f) * c->cam.sy;
  *out = nz.w / std::sqrt(pt_fma(dvy, dvy, pt_fma(dvx, dvx, 1.0f)));
  return PTC_OK;
}

void ptc_denoise_default_params(ptc_denoise_params* p) {
  if (!p) return;
  p->iterations = 4; p->sigma_l = 4.0f; p->sigma_n = 128.0f; p->sigma_p = 1.0f; p->demodulate = 1;
}
}  // extern "C"

namespace {
// accumulated: the input is the accumulated image of the frame's ptc_temporal_accumulate, i.e. D_new of the new history (demodulated already) with the temporal variance
// sampled: the input is the radiance, demodulated by k_ad_sampled_variance, with the variance of the frame's own samples (§8d) where a pixel has four or more
int denoise_image(ptc_ctx* c, const ptc_denoise_params* params, bool accumulated, bool sampled = false) {
  if (c && accumulated) { const std::string why = projection_refusal(c, "denoise_accumulated", "the accumulated image"); if (!why.empty()) return fail(c, PTC_E_STATE, why); }      // follows ptc_temporal_accumulate's refusal
  { int rd = need_device(c); if (rd) return rd; }
  if (entry_frame(c)) return fail(c, PTC_E_STATE, "denoise: a probe or lightmap frame has no image to denoise");
  const ptc_denoise_params p = with_defaults(params, ptc_denoise_default_params);
  auto bad = [](float v) { return !(v >= 0.0f) || !(v <= 3.0e38f); };      // NaN, negative, infinite
  if (p.iterations < 0 || p.iterations > PTC_DENOISE_MAX_ITERATIONS) return fail(c, PTC_E_ARG, "denoise: iterations outside 0..8");
  if (bad(p.sigma_l) || bad(p.sigma_n) || bad(p.sigma_p)) return fail(c, PTC_E_ARG, "denoise: a sigma is negative or not finite");
  if (!c->guides.valid) return fail(c, PTC_E_STATE, "denoise: no valid guides (ptc_frame_guides after the frame's ptc_frame_begin)");
  if (!c->radiance.p || c->rad_w == 0) return fail(c, PTC_E_STATE, "denoise: no radiance buffer");
  if (accumulated && !c->temporal.accum_valid) return fail(c, PTC_E_STATE, "denoise_accumulated: the frame has no accumulated image (ptc_temporal_accumulate)");
  if (accumulated && (p.demodulate ? 1 : 0) != c->temporal.demodulate) return fail(c, PTC_E_ARG, "denoise_accumulated: demodulate differs from the accumulate's");
  if (sampled && !(c->in_frame && c->adaptive.on && c->adaptive.cov_on)) return fail(c, PTC_E_STATE, "denoise_sampled: the frame is not an adaptive frame that keeps the sample covariance (ptc_set_sample_covariance before ptc_frame_set_adaptive)");
  if (sampled && (!c->adaptive.cov_resolved || c->pending)) return fail(c, PTC_E_STATE, "denoise_sampled: samples were added since the last ptc_frame_resolve");
  const size_t n = (size_t)c->rad_w * c->rad_h;
  int rc;
  if ((rc = ensure_buf(c, c->denoise.denoised, n))) return rc;
  if (sampled && ((rc = ensure_buf(c, c->adaptive.sv_colour, n)) || (rc = ensure_buf(c, c->adaptive.sv_var, n)))) return rc;
  if (p.iterations > 0 && ((rc = ensure_buf(c, c->denoise.cv[0], n)) || (rc = ensure_buf(c, c->denoise.cv[1], n)))) return rc;
  hipStream_t s0 = c->lanes[0].stream;      // behind the resolve, the reduce and the guide pass
  if ((rc = c->denoise.timer.begin(c, s0))) return rc;
  if (sampled)      // also with iterations = 0: ptc_read_sampled_variance serves what this call computed
    pt_launch_ad_sampled_variance(s0, c->owned_n, c->owned.p, c->accum.p, dev_adaptive(c), c->guides.albedo.p, c->radiance.p, p.demodulate ? 1 : 0, c->adaptive.sv_colour.p, c->adaptive.sv_var.p,
                                  (uint32_t)n, (size_t)c->owned_n != n);
  if (p.iterations == 0) HIP_TRY(c, hipMemcpyAsync(c->denoise.denoised.p, accumulated ? c->temporal.accum.p : c->radiance.p, n * sizeof(float4), hipMemcpyDeviceToDevice, s0));
  else {
    DenoiseArgs a{};
    a.w = c->rad_w; a.h = c->rad_h; a.sigma_l = p.sigma_l; a.sigma_n = p.sigma_n; a.sigma_p = p.sigma_p; a.demodulate = p.demodulate ? 1 : 0;
    if (cam_projection(c) == PTC_PROJ_PERSPECTIVE) a.pix = (2.0f * c->cam.sy) / (float)c->rad_h;
    else a.pix = pt_proj_footprint(c->cam, cam_proj(c), c->rad_h, a.pix_flat);      // pt_camera.h: pi / h, or 2 ymag / h at every depth
    a.radiance = c->radiance.p;
    a.g = c->guides.dev();
    if (sampled) {
      DenoiseArgs ap = a;
      ap.demodulate = 0;
      pt_launch_denoise_prepare(s0, ap, c->adaptive.sv_colour.p, c->adaptive.sv_var.p, c->denoise.cv[0].p);
    } else if (accumulated) {      // D_new lies demodulated in the history; the iterations re-modulate it as they do ptc_denoise's, and pass the other classes' radiance through
      DenoiseArgs ap = a;
      ap.demodulate = 0;
      pt_launch_denoise_prepare(s0, ap, c->temporal.dn[c->temporal.cur].p, c->temporal.mom[c->temporal.cur].p, c->denoise.cv[0].p);
    } else pt_launch_denoise_prepare(s0, a, c->radiance.p, nullptr, c->denoise.cv[0].p);
    for (int i = 0; i < p.iterations; ++i) {
      const bool last = i == p.iterations - 1;
      pt_launch_denoise_iteration(s0, a, i, c->denoise.cv[i & 1].p, last ? c->denoise.denoised.p : c->denoise.cv[(i + 1) & 1].p, last);
    }
  }
  if ((rc = c->denoise.timer.end(c, s0))) return rc;
  HIP_TRY(c, hipGetLastError());
  c->denoise.valid = true;
  if (sampled) c->adaptive.sv_valid = true;
  return PTC_OK;
}
}  // namespace

extern "C" {
int ptc_denoise(ptc_ctx* c, const ptc_denoise_params* params) { return denoise_image(c, params, false); }
int ptc_denoise_accumulated(ptc_ctx* c, const ptc_denoise_params* params) { return denoise_image(c, params, true); }
int ptc_denoise_sampled(ptc_ctx* c, const ptc_denoise_params* params) { return denoise_image(c, params, false, true); }

int ptc_get_denoise_seconds(ptc_ctx* c, double* guides, double* denoise) {
  { int rd = need_device(c); if (rd) return rd; }
  { int rc = c->guides.timer.seconds(c, guides); if (rc) return rc; }
  return c->denoise.timer.seconds(c, denoise);
}

// ---- temporal accumulation (pt_temporal.hip): the history lives in the context, see ptc_ctx ---------------------------------------------------
void ptc_temporal_default_params(ptc_temporal_params* p) {
  if (!p) return;
  p->max_history = 32; p->sigma_z = 1.0f; p->demodulate = 1;
}

int ptc_temporal_accumulate(ptc_ctx* c, const ptc_temporal_params* params) {
  if (c) { const std::string why = projection_refusal(c, "temporal_accumulate", "the reprojection of the history"); if (!why.empty()) return fail(c, PTC_E_STATE, why); }      // it needs the inverse projection; before the device: a description-only context can tell
  { int rd = need_device(c); if (rd) return rd; }
  if (entry_frame(c)) return fail(c, PTC_E_STATE, "temporal_accumulate: a probe or lightmap frame has no image to accumulate");
  const ptc_temporal_params p = with_defaults(params, ptc_temporal_default_params);
  if (p.max_history < 1 || p.max_history > PTC_TEMPORAL_MAX_HISTORY) return fail(c, PTC_E_ARG, "temporal_accumulate: max_history outside 1..1024");
  if (!(p.sigma_z >= 0.0f) || !(p.sigma_z <= 3.0e38f)) return fail(c, PTC_E_ARG, "temporal_accumulate: sigma_z is negative or not finite");
  if (!c->guides.valid) return fail(c, PTC_E_STATE, "temporal_accumulate: no valid guides (ptc_frame_guides after the frame's ptc_frame_begin)");
  if (!c->radiance.p || c->rad_w == 0) return fail(c, PTC_E_STATE, "temporal_accumulate: no radiance buffer");
  const int w = c->rad_w, h = c->rad_h, demodulate = p.demodulate ? 1 : 0;
  const size_t n = (size_t)w * h;
  int rc;
  Temporal& t = c->temporal;
  for (int k = 0; k < 2; ++k)
    if ((rc = ensure_buf(c, t.dn[k], n)) || (rc = ensure_buf(c, t.mom[k], n)) || (rc = ensure_buf(c, t.nz[k], n)) || (rc = ensure_buf(c, t.pk[k], n))) { drop_history(c); return rc; }
  // a set may have been regrown above: a failure from here on leaves no history either
  if ((rc = ensure_buf(c, t.motion, n)) || (rc = ensure_buf(c, t.accum, n))) { drop_history(c); return rc; }
  if ((rc = t.timer.create(c))) { drop_history(c); return rc; }
  if (t.live && (t.w != w || t.h != h || t.demodulate != demodulate)) drop_history(c);      // another size or another quantity: not this frame's history
  TemporalArgs a{};
  a.w = w; a.h = h; a.have_history = t.live ? 1 : 0; a.demodulate = demodulate;
  a.max_history = (float)p.max_history; a.sigma_z = p.sigma_z;
  a.cam_prev = t.cam;
  a.pix_prev = (2.0f * t.cam.sy) / (float)h;
  a.radiance = c->radiance.p;
  a.g = c->guides.dev();
  if (t.snap_current) { a.pos = t.snap.p; a.pos_stride = 3; }
  else { a.pos = c->scene.dsc.shade; a.pos_stride = c->scene.dsc.shade_stride; }
  const int cur = t.cur, nxt = cur ^ 1;
  a.prev = TemporalSet{t.dn[cur].p, t.mom[cur].p, t.nz[cur].p, t.pk[cur].p};
  a.next = TemporalSet{t.dn[nxt].p, t.mom[nxt].p, t.nz[nxt].p, t.pk[nxt].p};
  a.accumulated = t.accum.p; a.motion = t.motion.p;
  hipStream_t s0 = c->lanes[0].stream;      // behind the resolve, the reduce and the guide pass
  if ((rc = t.timer.begin(c, s0))) return rc;
  pt_launch_temporal_accumulate(s0, a);
  if ((rc = t.timer.end(c, s0))) return rc;
  HIP_TRY(c, hipGetLastError());
  t.cur = nxt; t.live = true; t.w = w; t.h = h; t.demodulate = demodulate; t.cam = c->cam;
  t.snap_current = false;      // the new history's frame saw the shading records as they lie now
  t.accum_valid = true;
  return PTC_OK;
}

int ptc_temporal_reset(ptc_ctx* c) {
  { int rd = need_device(c); if (rd) return rd; }
  drop_history(c);
  return PTC_OK;
}

int ptc_read_temporal_rgba32f(ptc_ctx* c, int which, float* out) {
  return read_image(c, "read_temporal", out, sizeof(float4), /*all_lanes=*/false, [&](const void*& src) -> int {
    if (which < PTC_TEMPORAL_HISTORY || which > PTC_TEMPORAL_POSITION_CLASS) return fail(c, PTC_E_ARG, "read_temporal: unknown buffer");
    if (!c->temporal.live) return fail(c, PTC_E_STATE, "read_temporal: no history (ptc_temporal_accumulate)");
    // the caller sizes `out` by the frame it knows, the current one: a history of another size (a frame_begin with a new size, not accumulated yet) is not served
    if (c->temporal.w != c->rad_w || c->temporal.h != c->rad_h) return fail(c, PTC_E_STATE, "read_temporal: the history's size is not the current frame's (no ptc_temporal_accumulate since the size changed)");
    const Temporal& t = c->temporal;      // rad_w x rad_h is the history's size here
    const float4* const bufs[5] = {t.dn[t.cur].p, t.mom[t.cur].p, t.motion.p, t.nz[t.cur].p, t.pk[t.cur].p};
    src = bufs[which];
    return PTC_OK;
  });
}

int ptc_get_temporal_seconds(ptc_ctx* c, double* accumulate) {
  { int rd = need_device(c); if (rd) return rd; }
  return c->temporal.timer.seconds(c, accumulate);
}

int ptc_select_output(ptc_ctx* c, int output) {
  { int rd = need_device(c); if (rd) return rd; }
  if (output != PTC_OUTPUT_RADIANCE && output != PTC_OUTPUT_DENOISED && output != PTC_OUTPUT_ACCUMULATED) return fail(c, PTC_E_ARG, "select_output: unknown output");
  if (output == PTC_OUTPUT_ACCUMULATED && !c->temporal.accum_valid) return fail(c, PTC_E_STATE, "select_output: the frame has no accumulated image (ptc_temporal_accumulate)");
  if (output == PTC_OUTPUT_DENOISED && !c->denoise.valid) return fail(c, PTC_E_STATE, "select_output: the frame has no denoised image (ptc_denoise)");
  c->output = output;
  return PTC_OK;
}

// ---- adaptive sampling (pt_adaptive.hip): the active set lives in c->fr, see ptc_ctx ---------------------------------------------------
void ptc_adaptive_default_params(ptc_adaptive_params* p) {
  if (!p) return;
  p->threshold = 0.05f; p->radius = 1; p->min_samples = 16; p->step_samples = 16;
}
}  // extern "C"

namespace {
int adaptive_params_ok(ptc_ctx* c, const ptc_adaptive_params& p, const char* who) {
  if (!(p.threshold >= 0.0f) || !(p.threshold <= 3.4028235e38f)) return fail(c, PTC_E_ARG, std::string(who) + ": the threshold is negative or not finite");
  if (p.radius < 0 || p.radius > PTC_AD_MAX_RADIUS) return fail(c, PTC_E_ARG, std::string(who) + ": radius outside 0..2");
  if (p.min_samples < 1 || p.step_samples < 1) return fail(c, PTC_E_ARG, std::string(who) + ": min_samples / step_samples < 1");
  return PTC_OK;
}
int need_adaptive_frame(ptc_ctx* c, const char* who) {
  { int rd = need_device(c); if (rd) return rd; }
  if (!c->in_frame || !c->adaptive.on) return fail(c, PTC_E_STATE, std::string(who) + ": no adaptive frame (ptc_frame_set_adaptive right after ptc_frame_begin)");
  return PTC_OK;
}
}  // namespace

extern "C" {
int ptc_frame_set_adaptive(ptc_ctx* c, const ptc_adaptive_params* params) {
  { int rd = need_device(c); if (rd) return rd; }
  if (!c->in_frame) return fail(c, PTC_E_STATE, "frame_set_adaptive: no frame");
  if (entry_frame(c)) return fail(c, PTC_E_STATE, "frame_set_adaptive: not available in a probe or lightmap frame");
  if (c->integrator != PTC_INTEGRATOR_PATH) return fail(c, PTC_E_STATE, "frame_set_adaptive: the frame is not a PTC_INTEGRATOR_PATH frame");
  if (c->adaptive.on || c->samples_done || c->pending) return fail(c, PTC_E_STATE, "frame_set_adaptive: call it once, right after ptc_frame_begin, before any sample");
  if (c->resolve_divisor) return fail(c, PTC_E_STATE, "frame_set_adaptive: the frame has a resolve divisor (ptc_frame_set_sample_range)");
  const ptc_adaptive_params p = with_defaults(params, ptc_adaptive_default_params);
  { int ra = adaptive_params_ok(c, p, "frame_set_adaptive"); if (ra) return ra; }
  const size_t n = c->owned_n, wh = (size_t)c->fr.w * (size_t)c->fr.h;
  int rc;
  for (int k = 0; k < 2; ++k) if ((rc = ensure_buf(c, c->adaptive.pix[k], n)) || (rc = ensure_buf(c, c->adaptive.slot[k], n))) return rc;
  if ((rc = ensure_buf(c, c->adaptive.mom, n)) || (rc = ensure_buf(c, c->adaptive.count, n)) || (rc = ensure_buf(c, c->adaptive.keep, n)) || (rc = ensure_buf(c, c->adaptive.flags, wh)) ||
      (rc = ensure_buf(c, c->adaptive.block, (size_t)pt_ad_blocks((uint32_t)n) + 1)) || (rc = ensure_buf(c, c->adaptive.n, 1))) return rc;
  const bool cov = c->adaptive.cov_setting;
  if (cov && ((rc = ensure_buf(c, c->adaptive.cov4, n)) || (rc = ensure_buf(c, c->adaptive.cov2, n)))) return rc;
  hipStream_t s0 = c->lanes[0].stream;
  HIP_TRY(c, hipMemsetAsync(c->adaptive.mom.p, 0, (n ? n : 1) * sizeof(float2), s0));
  if (cov) {
    HIP_TRY(c, hipMemsetAsync(c->adaptive.cov4.p, 0, (n ? n : 1) * sizeof(float4), s0));
    HIP_TRY(c, hipMemsetAsync(c->adaptive.cov2.p, 0, (n ? n : 1) * sizeof(float2), s0));
  }
  HIP_TRY(c, hipMemsetAsync(c->adaptive.count.p, 0, (n ? n : 1) * sizeof(uint32_t), s0));
  HIP_TRY(c, hipMemsetAsync(c->adaptive.flags.p, 0, wh, s0));
  pt_launch_ad_init(s0, (uint32_t)n, c->owned.p, c->adaptive.pix[0].p, c->adaptive.slot[0].p);
  HIP_TRY(c, hipGetLastError());
  HIP_TRY(c, hipStreamSynchronize(s0));      // the other lanes read these arrays too
  c->adaptive.cur = 0; c->adaptive.passes = 0; c->adaptive.seconds = 0.0; c->adaptive.params = p;
  c->fr.owned = c->adaptive.pix[0].p;              // n_owned is the frame's: everything is active
  c->adaptive.on = true; c->adaptive.cov_on = cov; c->adaptive.cov_resolved = false; c->adaptive.sv_valid = false;
  return PTC_OK;
}

int ptc_frame_adapt(ptc_ctx* c, uint64_t* n_active) {
  { int ra = need_adaptive_frame(c, "frame_adapt"); if (ra) return ra; }
  { int rf = flush(c); if (rf) return rf; }
  const uint32_t n_in = c->fr.n_owned;
  if (n_in == 0) { if (n_active) *n_active = 0; return PTC_OK; }
  const uint32_t n = c->samples_done;
  if (n == 0) return fail(c, PTC_E_STATE, "frame_adapt: the frame has no samples yet");
  { int rj = join_lanes_on_stream0(c); if (rj) return rj; }
  hipStream_t s0 = c->lanes[0].stream;
  const DevAdaptive ad = dev_adaptive(c);
  const int cur = c->adaptive.cur;
  uint32_t n_out = 0;
  { int rt = c->adaptive.timer.begin(c, s0); if (rt) return rt; }
  if (n >= (uint32_t)c->spp_total) {          // the budget is spent: everything stops; no pixel is active, so no flag stays set
    HIP_TRY(c, hipMemsetAsync(c->adaptive.flags.p, 0, (size_t)c->fr.w * (size_t)c->fr.h, s0));
  } else {
    pt_launch_ad_error(s0, n_in, c->adaptive.pix[cur].p, c->adaptive.slot[cur].p, ad, n, c->adaptive.params.threshold);
    pt_launch_ad_compact(s0, n_in, c->adaptive.pix[cur].p, c->adaptive.slot[cur].p, c->adaptive.pix[cur ^ 1].p, c->adaptive.slot[cur ^ 1].p, ad, c->fr.w, c->fr.h, c->adaptive.params.radius);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpyAsync(&n_out, c->adaptive.n.p, sizeof n_out, hipMemcpyDeviceToHost, s0));   // the host sizes the next launches by it
  }
  { int rt = c->adaptive.timer.end(c, s0); if (rt) return rt; }
  HIP_TRY(c, hipStreamSynchronize(s0));
  { double sec = 0.0; if (c->adaptive.timer.elapsed(&sec)) c->adaptive.seconds += sec; }
  if (n_out > n_in) return fail(c, PTC_E_DEVICE, "frame_adapt: the compaction returned more entries than it was given");
  c->adaptive.cur = cur ^ 1;
  c->fr.n_owned = n_out; c->fr.owned = c->adaptive.pix[c->adaptive.cur].p;
  c->per_batch = batch_samples(c, n_out, c->frame_batch_paths);      // as the set shrinks a pass still goes out as the fewest, widest launches
  c->adaptive.passes++;
  if (n_active) *n_active = n_out;
  return PTC_OK;
}

int ptc_read_sample_counts(ptc_ctx* c, uint32_t* out) {
  { int ra = need_adaptive_frame(c, "read_sample_counts"); if (ra) return ra; }
  if (!out) return fail(c, PTC_E_ARG, "read_sample_counts: null pointer");
  { int rf = flush(c); if (rf) return rf; }
  { int rs = sync_all_lanes(c); if (rs) return rs; }
  const size_t n = c->owned_n;
  std::vector<uint32_t> pix(n), cnt(n);
  if (n) {
    HIP_TRY(c, hipMemcpy(pix.data(), c->owned.p, n * sizeof(uint32_t), hipMemcpyDeviceToHost));
    HIP_TRY(c, hipMemcpy(cnt.data(), c->adaptive.count.p, n * sizeof(uint32_t), hipMemcpyDeviceToHost));
  }
  std::memset(out, 0, (size_t)c->rad_w * (size_t)c->rad_h * sizeof(uint32_t));
  for (size_t i = 0; i < n; ++i) out[pix[i]] = cnt[i];
  return PTC_OK;
}

int ptc_get_adaptive_stats(ptc_ctx* c, ptc_adaptive_stats* out) {
  { int ra = need_adaptive_frame(c, "get_adaptive_stats"); if (ra) return ra; }
  if (!out) return fail(c, PTC_E_ARG, "get_adaptive_stats: null pointer");
  { int rf = flush(c); if (rf) return rf; }
  { int rs = sync_all_lanes(c); if (rs) return rs; }
  std::vector<uint32_t> cnt(c->owned_n);
  if (!cnt.empty()) HIP_TRY(c, hipMemcpy(cnt.data(), c->adaptive.count.p, cnt.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
  ptc_adaptive_stats s{};
  s.owned_pixels = c->owned_n; s.active_pixels = c->fr.n_owned; s.passes = c->adaptive.passes; s.seconds_adapt = c->adaptive.seconds;
  for (uint32_t v : cnt) { s.samples_total += v; if (v > s.max_count) s.max_count = v; }
  *out = s;
  return PTC_OK;
}

int ptc_set_sample_covariance(ptc_ctx* c, int on) {
  if (!c) return PTC_E_ARG;
  if (on != 0 && on != 1) return fail(c, PTC_E_ARG, "set_sample_covariance: 0 or 1");
  if (on == 1 && entry_frame(c)) return fail(c, PTC_E_STATE, "set_sample_covariance: a probe or lightmap frame keeps no per-sample covariance (the setting is unchanged)");
  c->adaptive.cov_setting = on == 1;
  return PTC_OK;
}

int ptc_read_sample_covariance(ptc_ctx* c, float* out) {
  { int rd = need_device(c); if (rd) return rd; }
  if (!out) return fail(c, PTC_E_ARG, "read_sample_covariance: null pointer");
  if (!c->in_frame || !c->adaptive.on || !c->adaptive.cov_on) return fail(c, PTC_E_STATE, "read_sample_covariance: the frame is not an adaptive frame that keeps the sample covariance");
  { int rf = flush(c); if (rf) return rf; }
  { int rs = sync_all_lanes(c); if (rs) return rs; }
  const size_t n = c->owned_n;
  std::vector<uint32_t> pix(n);
  std::vector<float4> q4(n);
  std::vector<float2> q2(n);
  if (n) {
    HIP_TRY(c, hipMemcpy(pix.data(), c->owned.p, n * sizeof(uint32_t), hipMemcpyDeviceToHost));
    HIP_TRY(c, hipMemcpy(q4.data(), c->adaptive.cov4.p, n * sizeof(float4), hipMemcpyDeviceToHost));
    HIP_TRY(c, hipMemcpy(q2.data(), c->adaptive.cov2.p, n * sizeof(float2), hipMemcpyDeviceToHost));
  }
  std::memset(out, 0, (size_t)c->rad_w * (size_t)c->rad_h * 6 * sizeof(float));
  for (size_t i = 0; i < n; ++i) {
    float* o = out + (size_t)pix[i] * 6;
    o[0] = q4[i].x; o[1] = q4[i].y; o[2] = q4[i].z; o[3] = q4[i].w; o[4] = q2[i].x; o[5] = q2[i].y;
  }
  return PTC_OK;
}

int ptc_read_sampled_variance(ptc_ctx* c, float* out) {
  { int rd = need_device(c); if (rd) return rd; }
  if (!out) return fail(c, PTC_E_ARG, "read_sampled_variance: null pointer");
  if (!c->adaptive.sv_valid) return fail(c, PTC_E_STATE, "read_sampled_variance: no ptc_denoise_sampled in this frame");
  HIP_TRY(c, hipStreamSynchronize(c->lanes[0].stream));
  const size_t n = (size_t)c->rad_w * (size_t)c->rad_h;
  std::vector<float4> v(n);
  HIP_TRY(c, hipMemcpy(v.data(), c->adaptive.sv_var.p, n * sizeof(float4), hipMemcpyDeviceToHost));
  for (size_t i = 0; i < n; ++i) { out[2 * i] = v[i].z; out[2 * i + 1] = v[i].w; }
  return PTC_OK;
}

int ptc_render_adaptive(ptc_ctx* c, int w, int h, int max_spp, uint64_t seed, int max_bounces, const ptc_adaptive_params* params) {
  { int rd = need_device(c); if (rd) return rd; }
  const ptc_adaptive_params p = with_defaults(params, ptc_adaptive_default_params);
  { int ra = adaptive_params_ok(c, p, "render_adaptive"); if (ra) return ra; }
  int rc = ptc_frame_begin(c, w, h, max_spp, seed, max_bounces, PTC_INTEGRATOR_PATH, 0, 1);
  if (rc) return rc;
  if ((rc = ptc_frame_set_adaptive(c, &p))) return rc;
  if ((rc = ptc_frame_add_samples(c, p.min_samples < max_spp ? p.min_samples : max_spp))) return rc;
  for (;;) {
    uint64_t active = 0;
    if ((rc = ptc_frame_adapt(c, &active))) return rc;
    if (!active) break;      // converged everywhere, or the budget is spent (the step at n = max_spp empties the set)
    const int left = max_spp - (int)c->samples_done;
    if ((rc = ptc_frame_add_samples(c, p.step_samples < left ? p.step_samples : left))) return rc;
  }
  if ((rc = ptc_frame_resolve(c))) return rc;
  return ptc_sync(c);
}

}  // extern "C"

// ---- display transform (pt_display.h, pt_display.hip) ----------------------------------------------------------------------------------------
namespace {
// the histogram and the state record (zeroed when it is made: no adaptation state); what the display calls need before they queue anything
int ensure_display(ptc_ctx* c, const char* who) {
  if (!c->radiance.p || c->rad_w == 0) return fail(c, PTC_E_STATE, std::string(who) + ": nothing rendered");
  if ((size_t)c->rad_w * c->rad_h > PT_DISPLAY_MAX_PIXELS) return fail(c, PTC_E_ARG, std::string(who) + ": more than 2^28 pixels");
  int rc;
  if ((rc = ensure_buf(c, c->display.hist, PT_DISPLAY_BINS + 4))) return rc;
  if (!c->display.state.p) {
    if ((rc = ensure_buf(c, c->display.state, 1))) return rc;
    HIP_TRY(c, hipMemsetAsync(c->display.state.p, 0, sizeof(pt_display_state), c->lanes[0].stream));
    HIP_TRY(c, hipMemsetAsync(c->display.hist.p, 0, (PT_DISPLAY_BINS + 4) * sizeof(uint32_t), c->lanes[0].stream));
  }
  return PTC_OK;
}
int queue_display_half(ptc_ctx* c, const char* who) {
  { int rd = need_device(c); if (rd) return rd; }
  int rc;
  if ((rc = ensure_display(c, who))) return rc;
  const size_t n = (size_t)c->rad_w * c->rad_h;
  if ((rc = ensure_buf(c, c->display.half, n))) return rc;
  hipStream_t s0 = c->lanes[0].stream;
  if ((rc = c->display.t_display.begin(c, s0))) return rc;
  pt_launch_display_half(s0, served_image(c), (uint32_t)n, c->display.state.p, c->display.params, c->display.half.p);
  HIP_TRY(c, hipGetLastError());
  if ((rc = c->display.t_display.end(c, s0))) return rc;
  return PTC_OK;
}
}  // namespace

extern "C" {
void ptc_display_default_params(ptc_display_params* p) { if (p) pt_display_defaults(*p); }

int ptc_set_display(ptc_ctx* c, const ptc_display_params* params) {
  if (!c) return PTC_E_ARG;
  const ptc_display_params p = with_defaults(params, ptc_display_default_params);
  if (const char* e = pt_display_params_error(p)) return fail(c, PTC_E_ARG, std::string("set_display: ") + e);
  c->display.params = p;
  return PTC_OK;
}

int ptc_get_display(const ptc_ctx* c, ptc_display_params* out) {
  if (!c || !out) return PTC_E_ARG;
  *out = c->display.params;
  return PTC_OK;
}

int ptc_meter_exposure(ptc_ctx* c) {
  { int rd = need_device(c); if (rd) return rd; }
  int rc;
  if ((rc = ensure_display(c, "meter_exposure"))) return rc;
  hipStream_t s0 = c->lanes[0].stream;
  if ((rc = c->display.t_meter.begin(c, s0))) return rc;
  pt_launch_meter(s0, served_image(c), (uint32_t)((size_t)c->rad_w * c->rad_h), c->display.hist.p, c->display.state.p, c->display.params);
  HIP_TRY(c, hipGetLastError());
  if ((rc = c->display.t_meter.end(c, s0))) return rc;
  return PTC_OK;
}

int ptc_exposure_reset(ptc_ctx* c) {
  { int rd = need_device(c); if (rd) return rd; }
  if (c->display.state.p) HIP_TRY(c, hipMemsetAsync(c->display.state.p, 0, sizeof(pt_display_state), c->lanes[0].stream));      // behind a metering still queued
  return PTC_OK;
}

int ptc_get_exposure(ptc_ctx* c, float* scale_E, float* adapted_luminance, float* metered_luminance, uint64_t* metered, uint64_t* rejected) {
  uint32_t w[8];
  { int rc = ptc_debug_display_state(c, w); if (rc) return rc; }
  pt_display_state st;
  std::memcpy(&st, w, sizeof st);
  if (scale_E) *scale_E = pt_display_scale(c->display.params, st.A);
  if (adapted_luminance) *adapted_luminance = pt_display_float(st.A);
  if (metered_luminance) *metered_luminance = pt_display_float(st.Q);
  if (metered) *metered = st.N;
  if (rejected) *rejected = st.rejected;
  return PTC_OK;
}

int ptc_read_luminance_histogram(ptc_ctx* c, uint32_t out[4096]) {
  { int rd = need_device(c); if (rd) return rd; }
  if (!out) return fail(c, PTC_E_ARG, "read_luminance_histogram: null pointer");
  if (!c->display.hist.p || !c->display.t_meter.recorded) return fail(c, PTC_E_STATE, "read_luminance_histogram: nothing metered (ptc_meter_exposure)");
  HIP_TRY(c, hipStreamSynchronize(c->lanes[0].stream));
  HIP_TRY(c, hipMemcpy(out, c->display.hist.p, PT_DISPLAY_BINS * sizeof(uint32_t), hipMemcpyDeviceToHost));
  return PTC_OK;
}

int ptc_display_rgba8(ptc_ctx* c, uint8_t* out) {
  { int rd = need_device(c); if (rd) return rd; }
  if (!out) return fail(c, PTC_E_ARG, "display_rgba8: null pointer");
  int rc;
  if ((rc = ensure_display(c, "display_rgba8"))) return rc;
  const size_t n = (size_t)c->rad_w * c->rad_h;
  if ((rc = ensure_buf(c, c->display.ldr, n))) return rc;
  hipStream_t s0 = c->lanes[0].stream;
  if ((rc = c->display.t_display.begin(c, s0))) return rc;
  pt_launch_display_rgba8(s0, served_image(c), (uint32_t)n, c->display.state.p, c->display.params, c->display.ldr.p);
  HIP_TRY(c, hipGetLastError());
  if ((rc = c->display.t_display.end(c, s0))) return rc;
  HIP_TRY(c, hipStreamSynchronize(s0));
  HIP_TRY(c, hipMemcpy(out, c->display.ldr.p, n * 4, hipMemcpyDeviceToHost));
  return PTC_OK;
}

int ptc_display_rgba16f(ptc_ctx* c, uint16_t* out) {
  if (c && c->device >= 0 && !out) return fail(c, PTC_E_ARG, "display_rgba16f: null pointer");
  { int rc = queue_display_half(c, "display_rgba16f"); if (rc) return rc; }
  HIP_TRY(c, hipStreamSynchronize(c->lanes[0].stream));
  HIP_TRY(c, hipMemcpy(out, c->display.half.p, (size_t)c->rad_w * c->rad_h * sizeof(uint2), hipMemcpyDeviceToHost));
  return PTC_OK;
}
void* ptc_display_rgba16f_device_ptr(ptc_ctx* c) {
  if (queue_display_half(c, "display_rgba16f_device_ptr")) return nullptr;
  if (hipStreamSynchronize(c->lanes[0].stream) != hipSuccess) return nullptr;
  return (void*)c->display.half.p;
}

int ptc_get_display_seconds(ptc_ctx* c, double* meter, double* display) {
  { int rd = need_device(c); if (rd) return rd; }
  { int rc = c->display.t_meter.seconds(c, meter); if (rc) return rc; }
  return c->display.t_display.seconds(c, display);
}

// ---- light probes (pt_probes.h) ------------------------------------------------------------------------------------------------

int ptc_probes_begin(ptc_ctx* c, const float* positions_xyz, int n_probes, uint32_t probe_index_base, int spp_total, uint64_t seed, int max_bounces) {
  if (!c) return PTC_E_ARG;
  if (!positions_xyz) return fail(c, PTC_E_ARG, "probes_begin: null pointer");
  if (n_probes < 1 || n_probes > PTC_MAX_PROBES) return fail(c, PTC_E_ARG, "probes_begin: n_probes outside 1..2^26");
  if (spp_total < 1 || max_bounces < 0) return fail(c, PTC_E_ARG, "probes_begin: spp_total < 1 or max_bounces < 0");
  if ((uint64_t)probe_index_base + (uint64_t)n_probes > 0x100000000ull) return fail(c, PTC_E_ARG, "probes_begin: probe indices exceed 32 bits");
  for (size_t i = 0; i < (size_t)n_probes * 3; ++i)
    if (!std::isfinite(positions_xyz[i])) return fail(c, PTC_E_ARG, "probes_begin: a position is not finite");
  const FrameEntries fe{"probes_begin", positions_xyz, probe_index_base};
  return frame_begin(c, n_probes, 1, spp_total, seed, max_bounces, PTC_INTEGRATOR_PATH, 0, 1, &fe);
}

int ptc_probes_read_sh(ptc_ctx* c, float* out) {
  { int rd = need_device(c); if (rd) return rd; }
  if (!out) return fail(c, PTC_E_ARG, "probes_read_sh: null pointer");
  if (!c->in_frame || !c->probes.on) return fail(c, PTC_E_STATE, "probes_read_sh: no probe frame (ptc_probes_begin)");
  { int rf = flush(c); if (rf) return rf; }
  { int rs = sync_all_lanes(c); if (rs) return rs; }
  const size_t n = (size_t)c->fr.n_owned * PT_SH9_FLOATS;
  HIP_TRY(c, hipMemcpy(out, c->probes.acc.p, n * sizeof(float), hipMemcpyDeviceToHost));
  const uint32_t N = c->resolve_divisor ? c->resolve_divisor : c->samples_done;
  if (N == 0) return PTC_OK;      // no sample yet: the sums are zero, and so are the coefficients
  const float scale = pt_sh9_resolve_scale(N);
  for (size_t i = 0; i < n; ++i) out[i] = out[i] * scale;
  return PTC_OK;
}

int ptc_render_probes(ptc_ctx* c, const float* positions_xyz, int n_probes, int spp, uint64_t seed, int max_bounces, float* out) {
  if (c && !out) return fail(c, PTC_E_ARG, "render_probes: null pointer");
  int rc = ptc_probes_begin(c, positions_xyz, n_probes, 0, spp, seed, max_bounces);
  if (rc) return rc;
  if ((rc = ptc_frame_add_samples(c, spp))) return rc;
  return ptc_probes_read_sh(c, out);
}

int ptc_sh9_eval(const float sh[27], const float dir[3], float out[3]) {
  if (!sh || !dir || !out) return PTC_E_ARG;
  pt_sh9_eval(sh, dir, out);
  return PTC_OK;
}
int ptc_sh9_irradiance(const float sh[27], const float normal[3], float out[3]) {
  if (!sh || !normal || !out) return PTC_E_ARG;
  pt_sh9_irradiance(sh, normal, out);
  return PTC_OK;
}
}  // extern "C"

