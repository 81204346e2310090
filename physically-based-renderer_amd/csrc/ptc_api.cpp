// ptc_api.cpp — the C-ABI of include/ptc.h over the HIP wavefront path tracer.
//
// One context = one HIP device + `n_lanes` streams ("lanes").  Everything a frame needs is enqueued without host
// synchronisation: queue sizes live in device memory and the persistent kernels read them there, so a whole batch
// (set_counts → raygen → [closest, shade, scan, any] × bounces → accumulate) is a single asynchronous burst.  With PTC_LANES > 1
// successive batches of a frame alternate between the lanes, so one batch's launch tails overlap another batch's
// full-occupancy phases (only the per-pixel accumulation is ordered, in sample order, by events); the default is one lane,
// which the round-2 kernels make the faster arrangement.  The host blocks only in ptc_sync / read-backs / ptc_get_stats.
//
// There is no CPU path in this library: without a usable HIP device ptc_create fails.
//
// This file: the context's lifetime, lanes and batches, frames, the radiance read-backs, ptc_get_stats.  The scene calls are in ptc_api_scene.cpp, the image-space
// features in ptc_api_image.cpp, lightmaps in ptc_api_lightmap.cpp, RCCL and groups in ptc_api_multi.cpp, the ptc_debug_* hooks in ptc_api_debug.cpp; what a context owns is in ptc_ctx.h.
#include "ptc_ctx.h"

#define PTC_STR2(x) #x
#define PTC_STR(x) PTC_STR2(x)

using namespace ptc_detail;

namespace {
constexpr size_t kQueueBytesPerPath = 176;   // ensure_lane_queues: 2 x 48 (ray ping-pong) + 48 (shadow) + 16 (hit) + 16 (path radiance)
constexpr size_t kAlphaBytesPerPath = 65;    // ensure_alpha_queues: 48 (continuation) + 16 (its hit record) + 1 (k_trace_any's flag)
constexpr size_t kGlassBytesPerPath = 64;    // ensure_glass_queues: 48 (continuation) + 16 (its hit record)
constexpr size_t kGlassFlagBytesPerPath = 1; // ... + 1 (k_trace_any's flag) in a frame with transparent shadows
constexpr size_t kMediumBytesPerPath = 144;  // ensure_medium_queues: 3 x 48 (parked continuation, emitter / environment shadow and punctual shadow records)
constexpr size_t kMaxSpans = 1024;   // timing spans (event pairs) kept at most; see run_batch

// the timing spans that have completed (all_done: every one) go into the statistics, their events back to the pool
void collect_times(ptc_ctx* c, bool all_done) {
  size_t keep = 0;
  for (size_t i = 0; i < c->spans.size(); ++i) {
    const Span s = c->spans[i];
    if (!all_done && hipEventQuery(s.b) != hipSuccess) { c->spans[keep++] = s; continue; }
    float ms = 0.0f;
    if (hipEventElapsedTime(&ms, s.a, s.b) == hipSuccess) {
      const double sec = 1e-3 * (double)ms;
      if (s.kind == 0) c->stats.seconds_trace_closest += sec;
      else if (s.kind == 1) c->stats.seconds_trace_any += sec;
      else if (s.kind == 2) c->stats.seconds_shade += sec;
      else if (s.kind == 4) c->stats.seconds_reduce += sec;
      else if (s.kind == 5) c->alpha.seconds += sec;
      else if (s.kind == 6) c->glass.seconds += sec;
      else if (s.kind == 7) c->medium.seconds += sec;
      else if (s.kind == 8) { c->stats.seconds_shade += sec; c->emtex.seconds += sec; }
      else c->stats.seconds_render += sec;
    }
    c->free_events.push_back(s.a); c->free_events.push_back(s.b);
  }
  c->spans.resize(keep);
}

bool is_raster(int integrator) { return integrator == PTC_INTEGRATOR_RASTER_COMPAT || integrator == PTC_INTEGRATOR_RASTER_GBUFFER16; }

// One wavefront batch of n samples per owned pixel (per active pixel of an adaptive frame) on lane `l`, fully asynchronous.
int run_batch(ptc_ctx* c, int l, uint32_t first_sample, uint32_t n_samples) {
  const uint32_t n_paths = c->fr.n_owned * n_samples;
  Lane& ln = c->lanes[(size_t)l];
  hipStream_t st = ln.stream;
  const DevQueues q = batch_queues(c, l, n_paths);
  const DevScene sc = lane_scene(c, l);
  // The persistent grid of the trace kernels follows the batch: a wave wants several refills' worth of rays (c->trace_rays_per_lane per lane) to run in its
  // steady state; 8192 waves over the 2 M rays of a 1080p x 1 spp frame are 4 refills each, most of the launch is start-up and drain (0.8 ms for bounce 0,
  // 0.25 ms for the last bounces: tools/viewer_loop.py).  Batches of the benchmark's size keep the full grid.
  const LaunchCfg cfg = batch_cfg(c, n_paths);
  if (c->spans.size() > kMaxSpans) {      // bounded event pool: harvest what has completed; if the host runs far ahead of
    collect_times(c, false);              // the device, wait for the oldest batch (back-pressure) instead of growing
    if (c->spans.size() > kMaxSpans) { (void)hipEventSynchronize(c->spans[c->spans.size() - kMaxSpans].b); collect_times(c, false); }
  }
  ScopedSpan whole(c, st, 3);
  pt_launch_set_counts(st, cfg, q, n_paths, 0);
  if (is_raster(c->integrator)) {
    pt_launch_raygen(st, c->cam, c->fr, q, 0, 1, true);
    { ScopedSpan t(c, st, 0); pt_launch_trace_closest(st, cfg, sc, q, 0, true); c->stats.launches_trace_closest++; }
    pt_launch_shade_raster(st, sc, c->cam, c->fr, q, c->accum.p, c->integrator == PTC_INTEGRATOR_RASTER_GBUFFER16);
  } else {
    if (c->lightmap.on) pt_launch_raygen_texel(st, c->lightmap.texels.p, c->fr.n_owned, c->lightmap.base, c->fr.seed_hash, q, first_sample, n_samples);      // a lightmap frame (pt_lightmap.hip): oriented rays from the texels
    else if (c->probes.on) pt_launch_raygen_probe(st, c->probes.pos.p, c->fr.n_owned, c->probes.base, c->fr.seed_hash, q, first_sample, n_samples);      // a probe frame (pt_probes.hip) has no camera and no lens
    else if (cam_projection(c) != PTC_PROJ_PERSPECTIVE) pt_launch_raygen_proj(st, c->cam, cam_proj(c), c->fr, q, first_sample, n_samples);      // an orthographic or equirectangular camera (pt_camera.hip); it has no lens
    else if (c->lens.aperture_radius > 0.0f) pt_launch_raygen_lens(st, c->cam, c->lens, c->fr, q, first_sample, n_samples);      // the thin lens (pt_lens.hip); the raster integrators above ignore it
    else pt_launch_raygen(st, c->cam, c->fr, q, first_sample, n_samples, false);
    const bool shadows = sc.n_lights > 0 || sc.env_ok;
    const bool small_batch = n_paths <= (1u << 26);
    // punctual lights (pt_lights.hip): a second next-event pass per bounce, on this stream alone — it needs hit and ray[b & 1] of bounce b intact and lpath to itself,
    // so any(b) does not run beside closest(b + 1) while lights exist
    const bool punctual = c->lights.n_dev > 0;
    // alpha coverage (pt_alpha.hip): the hit records of bounce b are resolved between closest(b) and shade(b), every shadow queue to a transmittance per record instead of
    // a flag — rounds of filter, scan and closest-hit launches on this stream alone, so any(b) does not run beside closest(b + 1) while alpha materials exist either
    const bool alpha = alpha_on(c);
    // dielectric transmission (pt_glass.hip): behind the alpha resolution of bounce b, before shade(b), rounds of launches on this stream alone as well
    const bool glass = glass_on(c);
    // transparent shadows (pt_glass_shadow.hip): every shadow queue to an RGB transmittance per record, one walk for alpha surfaces and thin panes
    const bool glass_shadows = glass_shadows_on(c);
    // the participating medium (pt_medium.hip): k_medium_decide between closest(b) and shade(b), k_medium_append behind shade(b) and behind the punctual pass, each before
    // the scan that follows — on this stream alone, so any(b) does not run beside closest(b + 1) while a medium is on either.  Off: none of these branches, nothing allocated
    const bool medium = medium_on(c);
    const DevMediumQ mq = medium ? dev_medium_q(c, l) : DevMediumQ{};
    // textured emission (pt_emissive_tex.hip): a third next-event pass per bounce behind the punctual one, with the hit side of its MIS pair — on this stream alone as
    // well: it needs hit and ray[b & 1] of bounce b intact and adds to lpath itself, so any(b) does not run beside closest(b + 1) while the table exists
    const bool emtex = emtex_on(c);
    const DevEmTex et = emtex ? dev_emtex(c) : DevEmTex{};
    auto trace_shadows = [&]() {
      ScopedSpan t(c, st, 1);
      if (glass_shadows || alpha) resolve_shadow(c, l, st, cfg, sc, q, glass_shadows, nullptr, nullptr);
      else pt_launch_trace_any(st, cfg, sc, q, nullptr);
      c->stats.launches_trace_any++;
    };
    // behind a further next-event pass of bounce b: the same ray prefix again, the new shadow counts, the work counters zeroed (nothing runs beside it), its records traced
    auto scan_and_trace_shadows = [&](int b) { pt_launch_scan(st, cfg, q, (b + 1) & 1); trace_shadows(); };
    auto medium_append = [&](int b, bool behind_punctual) { ScopedSpan t(c, st, 7); pt_launch_medium_append(st, q, mq, c->medium.frame, b & 1, behind_punctual); };
    const bool overlap = (c->trace_overlap == 2 || (c->trace_overlap == 1 && small_batch)) && shadows && ln.stream2 && ln.stack_ovf2 && !punctual && !alpha && !glass && !medium && !emtex;
    if (overlap) {
      const size_t need = (size_t)c->fr.max_bounces + 1;
      while (ln.ev_scan.size() < need) { hipEvent_t e = nullptr; HIP_TRY(c, hipEventCreateWithFlags(&e, hipEventDisableTiming)); ln.ev_scan.push_back(e); }
      while (ln.ev_any.size() < need) { hipEvent_t e = nullptr; HIP_TRY(c, hipEventCreateWithFlags(&e, hipEventDisableTiming)); ln.ev_any.push_back(e); }
    }
    DevScene sc_any = sc;
    if (overlap) sc_any.stack_ovf = ln.stack_ovf2;
    const bool per_kernel = !overlap || c->timing >= 2;       // overlapped launches: the batch's span only (ptc_stats.seconds_render); seconds_trace_* / seconds_shade stay 0
    for (int b = 0; b <= c->fr.max_bounces; ++b) {
      { ScopedSpan t(c, st, 0, per_kernel); pt_launch_trace_closest(st, cfg, sc, q, b & 1, false); c->stats.launches_trace_closest++; }
      if (alpha) alpha_resolve_closest(c, l, st, cfg, sc, q, b & 1, (uint32_t)b, PT_ALPHA_FORM_CLOSEST, nullptr);
      if (glass) glass_resolve_closest(c, l, st, cfg, sc, q, b & 1, (uint32_t)b, nullptr);
      // a lightmap frame counts the back-face first hits of its texels: the geometric hit of bounce 0, before the medium may turn it into a scatter event
      if (b == 0 && c->lightmap.on) pt_launch_lm_first_hit(st, sc, q, 0, c->fr.n_owned, c->lightmap.back.p);
      if (medium) { ScopedSpan t(c, st, 7); pt_launch_medium_decide(st, sc, q, mq, c->medium.frame, b & 1, (uint32_t)b, (uint32_t)c->fr.max_bounces, c->lights.recs.p, c->lights.cdf.p, c->lights.n_dev); }
      // k_shade(b) overwrites the shadow queue any(b - 1) reads and adds to the path radiance it adds to
      if (overlap && b > 0) HIP_TRY(c, hipStreamWaitEvent(st, ln.ev_any[(size_t)b - 1], 0));
      { ScopedSpan t(c, st, 2, per_kernel); pt_launch_shade(st, cfg, ln.d_scene, c->fr, q, b & 1, (uint32_t)b); }
      if (b == c->fr.max_bounces) {                              // the last bounce's shade produces no rays; a textured emitter it hit still counts, as k_shade's emission does
        if (emtex) { ScopedSpan t(c, st, 8); pt_launch_shade_emissive_tex(st, sc, q, b & 1, (uint32_t)b, (uint32_t)c->fr.max_bounces, et); }
        break;
      }
      if (medium) medium_append(b, false);
      pt_launch_scan(st, cfg, q, (b + 1) & 1);
      if (overlap) {      // any(b) on the second stream, beside closest(b + 1)
        HIP_TRY(c, hipEventRecord(ln.ev_scan[(size_t)b], st));
        HIP_TRY(c, hipStreamWaitEvent(ln.stream2, ln.ev_scan[(size_t)b], 0));
        { ScopedSpan t(c, ln.stream2, 1, per_kernel); pt_launch_trace_any(ln.stream2, cfg, sc_any, q, nullptr); c->stats.launches_trace_any++; }
        HIP_TRY(c, hipEventRecord(ln.ev_any[(size_t)b], ln.stream2));
      } else if (shadows) trace_shadows();
      if (punctual) {     // behind emission (k_shade) and the emitter / environment sample (any): the punctual sample, through the same shadow queue
        { ScopedSpan t(c, st, 2); pt_launch_shade_punctual(st, sc, q, b & 1, (uint32_t)b, c->lights.recs.p, c->lights.cdf.p, c->lights.n_dev); }
        if (medium) medium_append(b, true);
        scan_and_trace_shadows(b);
      }
      if (emtex) {        // behind the punctual sample: textured emission at the hit, then the textured sample through the same shadow queue
        { ScopedSpan t(c, st, 8); pt_launch_shade_emissive_tex(st, sc, q, b & 1, (uint32_t)b, (uint32_t)c->fr.max_bounces, et); }
        if (et.sample) scan_and_trace_shadows(b);
      }
    }
    // sample-order accumulation: wait for the previous batch's accumulate (it ran on the previous lane)
    if (c->n_lanes > 1 && c->batches_issued > 0) {
      const int prev = (int)((c->batches_issued - 1) % (uint64_t)c->n_lanes);
      if (prev != l) HIP_TRY(c, hipStreamWaitEvent(st, c->lanes[(size_t)prev].acc_done, 0));
    }
    if (c->adaptive.on) pt_launch_ad_accumulate(st, c->fr.n_owned, c->adaptive.slot[c->adaptive.cur].p, q.lpath, c->accum.p, dev_adaptive(c), n_samples, c->fr.path_order);
    else pt_launch_accumulate(st, c->fr, q, c->accum.p, n_samples);
    // a probe frame: the SH projection of the same path radiance, inside the same sample-order bracket (it has its own sums, so the two do not order each other)
    if (c->probes.on) pt_launch_accumulate_sh(st, c->fr.n_owned, c->probes.base, c->fr.seed_hash, q.lpath, c->probes.acc.p, first_sample, n_samples);
    if (c->n_lanes > 1) HIP_TRY(c, hipEventRecord(ln.acc_done, st));
  }
  c->batches_issued++;
  HIP_TRY(c, hipGetLastError());
  return PTC_OK;
}

// Issue `k` samples (k <= per_batch) as one batch on the next lane.
int issue(ptc_ctx* c, uint32_t k) {
  if (is_raster(c->integrator)) {
    if (c->samples_done == 0) {
      int rc = ensure_lane_queues(c, c->fr.n_owned);
      if (rc) return rc;
      if ((rc = run_batch(c, 0, 0, 1))) return rc;
      c->stats.paths = c->fr.n_owned;
    }
    c->samples_done += k;
    return PTC_OK;
  }
  const uint64_t cap = (uint64_t)c->fr.n_owned * k;
  int rc = ensure_lane_queues(c, (uint32_t)cap);
  if (rc) return rc;
  if (alpha_on(c) && (rc = ensure_alpha_queues(c))) return rc;
  if (glass_on(c) && (rc = ensure_glass_queues(c))) return rc;
  if (medium_on(c) && (rc = ensure_medium_queues(c))) return rc;
  if ((rc = run_batch(c, (int)(c->batches_issued % (uint64_t)c->n_lanes), c->sample_base + c->samples_done, k))) return rc;
  c->samples_done += k;
  c->stats.paths += cap;
  return PTC_OK;
}

// RGBA16F view of the radiance buffer, converted on stream 0 (after everything queued there: resolve, reduce, write).
int convert_half(ptc_ctx* c) {
  if (!c->radiance.p || c->rad_w == 0) return fail(c, PTC_E_STATE, "radiance_rgba16f: nothing rendered");
  const size_t n = (size_t)c->rad_w * c->rad_h;
  int rc = ensure_buf(c, c->half, n);
  if (rc) return rc;
  pt_launch_to_half(c->lanes[0].stream, served_image(c), c->half.p, (uint32_t)n);
  HIP_TRY(c, hipGetLastError());
  return PTC_OK;
}

// what the environment says about building scenes: every context reads it, a description-only one reads nothing else
void read_build_environment(ptc_ctx* c) {
  if (const char* s = std::getenv("PTC_NODELETS")) c->toplet_budget = (uint32_t)std::strtoul(s, nullptr, 10);
  if (const char* s = std::getenv("PTC_BVH")) { if (std::strcmp(s, "lbvh") == 0) c->bvh_default = c->bvh_builder = PTC_BVH_LBVH; }
  if (const char* s = std::getenv("PTC_DEVICE_BVH")) { if (std::strcmp(s, "sah") == 0) c->device_builder = PTC_BVH_SAH; }
}
}  // namespace

// ---- what the other ptc_api*.cpp files call of this file (ptc_ctx.h declares it) -----------------------------------------------------------------
namespace ptc_detail {
std::string g_create_error;

int sync_all_lanes(ptc_ctx* c) {
  for (auto& ln : c->lanes) HIP_TRY(c, hipStreamSynchronize(ln.stream));
  return PTC_OK;
}

// Every lane gets queues for at least `cap` paths (grow only; all lanes keep the same capacity, so a batch fits whichever
// lane it is routed to).  Growing waits for the work in flight first: the old arrays may still be in use.
int ensure_lane_queues(ptc_ctx* c, uint32_t cap) {
  bool grow = false;
  for (auto& ln : c->lanes) grow = grow || ln.q.cap < cap;
  if (!grow) return PTC_OK;
  { int rs = sync_all_lanes(c); if (rs) return rs; }
  for (auto& ln : c->lanes) {
    if (ln.q.cap >= cap) continue;
    free_all(ln.allocs);
    ln.q.cap = 0;
    DevQueues q = ln.q;   // keeps cnt / stats / the per-segment arrays
    int rc = 0;
    const size_t slots = ptc_seg_slots(cap, (uint32_t)c->cfg.shade_waves);   // segments are padded to multiples of 64 slots
    for (int k = 0; k < 2 && !rc; ++k) {
      rc = dev_alloc(c, ln.allocs, &q.ray[k].A, slots); if (!rc) rc = dev_alloc(c, ln.allocs, &q.ray[k].B, slots);
      if (!rc) rc = dev_alloc(c, ln.allocs, &q.ray[k].C, slots);
    }
    if (!rc) rc = dev_alloc(c, ln.allocs, &q.shadow.A, slots);
    if (!rc) rc = dev_alloc(c, ln.allocs, &q.shadow.B, slots);
    if (!rc) rc = dev_alloc(c, ln.allocs, &q.shadow.C, slots);
    if (!rc) rc = dev_alloc(c, ln.allocs, &q.hit, slots);
    if (!rc) rc = dev_alloc(c, ln.allocs, &q.lpath, cap);
    if (rc) { free_all(ln.allocs); return rc; }
    q.cap = cap;
    ln.q = q;
  }
  return PTC_OK;
}

// ---- timing spans: event pairs around the kernels of a batch; events are recycled as soon as they have completed, so a
// progressive loop that never asks for statistics does not grow the pool -----------------------------------------------
hipEvent_t next_event(ptc_ctx* c) {
  if (!c->free_events.empty()) { hipEvent_t e = c->free_events.back(); c->free_events.pop_back(); return e; }
  hipEvent_t e;
  if (hipEventCreate(&e) != hipSuccess) return nullptr;
  c->events_created++;
  return e;
}

DevScene lane_scene(ptc_ctx* c, int l) { DevScene d = c->scene.dsc; d.stack_ovf = c->lanes[(size_t)l].stack_ovf; return d; }

// the lane's queues with the segment layout of a batch of n slots (ptc_internal.h, "SEGMENTED queues")
DevQueues batch_queues(ptc_ctx* c, int l, uint32_t n) {
  DevQueues q = c->lanes[(size_t)l].q;
  ptc_seg_layout(n, (uint32_t)c->cfg.shade_waves, q.n_seg, q.seg_len);
  return q;
}

// the launch configuration of a batch of n_paths rays: the trace kernels' persistent grid follows the batch (see run_batch)
LaunchCfg batch_cfg(const ptc_ctx* c, uint32_t n_paths) {
  LaunchCfg cfg = c->cfg;
  const uint64_t per_block = (uint64_t)pt_trace_block_threads() * (uint64_t)c->trace_rays_per_lane;
  uint64_t per_cu = ((uint64_t)n_paths + per_block * (uint64_t)cfg.n_cu - 1u) / (per_block * (uint64_t)cfg.n_cu);
  if (per_cu < 1) per_cu = 1;
  if (per_cu < (uint64_t)cfg.trace_blocks_per_cu) cfg.trace_blocks_per_cu = (int)per_cu;
  return cfg;
}

// samples of one full batch of `n_pixels` pixels: as many as fit `batch_paths` split over the lanes, and 32-bit slot indices
uint32_t batch_samples(const ptc_ctx* c, size_t n_pixels, size_t batch_paths) {
  size_t per = !n_pixels ? 1 : batch_paths / n_pixels / (size_t)c->n_lanes;
  if (per < 1) per = 1;
  if (per > 0x7fffffffu) per = 0x7fffffffu;
  {   // slot indices are 32 bits, and the segmented layout pads a batch by up to 64 slots per segment
    const uint64_t max_slots = 0xfffffff0ull - 64ull * (uint64_t)c->cfg.shade_waves - 64ull;
    if (n_pixels && (uint64_t)n_pixels * per > max_slots) per = max_slots / n_pixels;
    if (per < 1) per = 1;
  }
  return (uint32_t)per;
}

// Issue everything frame_add_samples has accepted so far.
int flush(ptc_ctx* c) {
  if (!c->in_frame) return PTC_OK;
  while (c->pending) {
    const uint32_t k = c->pending < c->per_batch ? c->pending : c->per_batch;
    c->pending -= k;
    if (c->fr.n_owned == 0) { c->samples_done += k; continue; }
    int rc = issue(c, k);
    if (rc) return rc;
  }
  return PTC_OK;
}

// stream 0 waits for the accumulates of all lanes (the last batches may have run elsewhere)
int join_lanes_on_stream0(ptc_ctx* c) {
  if (c->n_lanes > 1 && !is_raster(c->integrator))
    for (int l = 1; l < c->n_lanes; ++l)
      if ((uint64_t)l < c->batches_issued) HIP_TRY(c, hipStreamWaitEvent(c->lanes[0].stream, c->lanes[(size_t)l].acc_done, 0));
  return PTC_OK;
}

int sum_lane_stats(ptc_ctx* c, unsigned long long st[ST_N]) {
  for (int i = 0; i < ST_N; ++i) st[i] = 0;
  for (auto& ln : c->lanes) {
    if (!ln.q.stats) continue;
    unsigned long long one[ST_N * ST_STRIDE];
    HIP_TRY(c, hipMemcpy(one, ln.q.stats, sizeof one, hipMemcpyDeviceToHost));
    for (int i = 0; i < ST_N; ++i) st[i] += one[i * ST_STRIDE];
  }
  return PTC_OK;
}

// ptc_destroy's share of a lane: the stream goes after everything that ran on it; the overflow slabs are the committed scene's (release_scene)
void Lane::teardown() {
  if (acc_done) (void)hipEventDestroy(acc_done);
  free_all(allocs);
  free_all(alpha.allocs);
  free_all(glass.allocs);
  free_all(medium.allocs);
  if (q.cnt) (void)hipFree(q.cnt);
  if (q.stats) (void)hipFree(q.stats);
  if (q.seg_ray[0]) (void)hipFree(q.seg_ray[0]);
  if (d_scene) (void)hipFree(d_scene);
  if (stream) (void)hipStreamDestroy(stream);
  if (stream2) (void)hipStreamDestroy(stream2);
  for (hipEvent_t e : ev_scan) (void)hipEventDestroy(e);
  for (hipEvent_t e : ev_any) (void)hipEventDestroy(e);
}


// ptc_frame_begin, and ptc_probes_begin's and ptc_lightmap_begin's share of it: `entries` begins a frame over a list of w entries (h = 1, the path integrator, no
// tiles) — the "owned pixels" are the entries in their own order.  Probes: the positions go to the device, the 27 w sums are cleared and the probe flag is set.
// A lightmap: the texel list is on the device already (lightmap_begin built it), the back-face counts are cleared and the lightmap flag is set
int frame_begin(ptc_ctx* c, int w, int h, int spp_total, uint64_t seed, int max_bounces, int integrator, int tile_rank, int tile_count, const FrameEntries* entries) {
  const float* probe_pos = entries ? entries->probe_pos : nullptr;
  const bool lightmap = entries && !probe_pos;
  if (c) { if (const char* why = medium_conflict(c, integrator)) { c->in_frame = false; return fail(c, PTC_E_STATE, why); } }
  if (c) { if (const char* why = emtex_medium_conflict(c, integrator)) { c->in_frame = false; return fail(c, PTC_E_STATE, why); } }      // before the device: a description-only context can tell
  if (c && !entries && is_raster(integrator)) { const std::string why = projection_refusal(c, "frame_begin", "a raster integrator"); if (!why.empty()) { c->in_frame = false; return fail(c, PTC_E_STATE, why); } }
  { int rd = need_device(c); if (rd) return rd; }
  c->in_frame = false; c->pending = 0; c->adaptive.on = false; c->adaptive.cov_on = false; c->adaptive.cov_resolved = false; c->adaptive.sv_valid = false; drop_guides(c);      // whatever happens below, the previous frame is over
  const std::string who = entries ? entries->who : "frame_begin";      // the entry the caller used, for ptc_last_error
  if (!c->committed) return fail(c, PTC_E_STATE, who + ": scene not committed");
  if ((w <= 0 && !(lightmap && w == 0)) || h <= 0 || spp_total <= 0 || max_bounces < 0 || (uint64_t)w * (uint64_t)h > 0x7fffffffull) return fail(c, PTC_E_ARG, who + ": bad size");
  if (integrator != PTC_INTEGRATOR_PATH && !is_raster(integrator)) return fail(c, PTC_E_ARG, who + ": unknown integrator");
  if (tile_count < 1 || tile_rank < 0 || tile_rank >= tile_count) return fail(c, PTC_E_ARG, who + ": bad tile rank/count");
  { int rs = sync_all_lanes(c); if (rs) return rs; }
  int rc;
  if ((rc = upload_lights(c))) return rc;      // a changed light table: nothing is queued any more that reads the old one
  if ((rc = alpha_upload(c))) return rc;       // the alpha tables of a scene committed since the last frame
  if (c->alpha.counters.p) HIP_TRY(c, hipMemset(c->alpha.counters.p, 0, PT_ALPHA_COUNTERS * sizeof(unsigned long long)));
  if ((rc = glass_upload(c))) return rc;       // the glass tables likewise
  if (c->glass.counters.p) HIP_TRY(c, hipMemset(c->glass.counters.p, 0, PT_GLASS_COUNTERS * sizeof(unsigned long long)));
  if (c->glass.shadow_counters.p) HIP_TRY(c, hipMemset(c->glass.shadow_counters.p, 0, PT_GLASS_SHADOW_COUNTERS * sizeof(unsigned long long)));
  if ((rc = emtex_upload(c))) return rc;       // the textured emitters' table likewise, and after a refit or rebuild; its counters cleared
  c->glass.frame_shadows = c->glass.shadows;      // before the queues are sized: a frame with transparent shadows keeps a flag byte per path
  if ((rc = medium_frame_begin(c, integrator == PTC_INTEGRATOR_PATH))) return rc;      // likewise: a frame with a medium keeps a medium queue
  // the list of owned pixels (tile-Morton order) depends on the image size and the tile assignment only: a viewer that renders frame after frame at
  // one size keeps the list it has on the device (2 M entries: 10 ms of host time and an 8 MB upload per frame otherwise — tools/viewer_loop.py)
  if (entries) {      // entry j is "pixel" j: the identity list (the next camera frame makes its own)
    std::vector<uint32_t> owned((size_t)w);
    for (int j = 0; j < w; ++j) owned[(size_t)j] = (uint32_t)j;
    c->owned_key_valid = false;
    if ((rc = ensure_buf(c, c->owned, owned.size()))) return rc;
    if (w) HIP_TRY(c, hipMemcpy(c->owned.p, owned.data(), owned.size() * 4, hipMemcpyHostToDevice));
    if (probe_pos) {
      std::vector<float4> pos((size_t)w);
      for (int j = 0; j < w; ++j) pos[(size_t)j] = make_float4(probe_pos[j * 3], probe_pos[j * 3 + 1], probe_pos[j * 3 + 2], 0.0f);
      if ((rc = ensure_buf(c, c->probes.pos, pos.size())) || (rc = ensure_buf(c, c->probes.acc, (size_t)PT_SH9_FLOATS * (size_t)w))) return rc;
      HIP_TRY(c, hipMemcpy(c->probes.pos.p, pos.data(), pos.size() * sizeof(float4), hipMemcpyHostToDevice));
      HIP_TRY(c, hipMemsetAsync(c->probes.acc.p, 0, (size_t)PT_SH9_FLOATS * (size_t)w * sizeof(float), c->lanes[0].stream));
    } else {
      if ((rc = ensure_buf(c, c->lightmap.back, (size_t)w))) return rc;
      HIP_TRY(c, hipMemsetAsync(c->lightmap.back.p, 0, (size_t)(w ? w : 1) * sizeof(uint32_t), c->lanes[0].stream));
    }
    c->owned_n = (uint32_t)w;
  } else if (!(c->owned_key_valid && c->owned_w == w && c->owned_h == h && c->owned_rank == tile_rank && c->owned_count == tile_count && c->owned.p)) {
    std::vector<uint32_t> owned;
    ptc_owned_pixels(w, h, tile_rank, tile_count, owned);
    c->owned_key_valid = false;
    if ((rc = ensure_buf(c, c->owned, owned.size()))) return rc;
    if (!owned.empty()) HIP_TRY(c, hipMemcpy(c->owned.p, owned.data(), owned.size() * 4, hipMemcpyHostToDevice));
    c->owned_n = (uint32_t)owned.size();
    c->owned_w = w; c->owned_h = h; c->owned_rank = tile_rank; c->owned_count = tile_count; c->owned_key_valid = true;
  }
  const size_t n_owned = c->owned_n;
  if ((rc = ensure_buf(c, c->accum, n_owned))) return rc;
  if ((rc = ensure_buf(c, c->radiance, (size_t)w * h))) return rc;
  hipStream_t s0 = c->lanes[0].stream;
  HIP_TRY(c, hipMemsetAsync(c->accum.p, 0, (n_owned ? n_owned : 1) * sizeof(float4), s0));
  HIP_TRY(c, hipMemsetAsync(c->radiance.p, 0, (size_t)w * h * sizeof(float4), s0));
  c->rad_w = w; c->rad_h = h;
  c->fr.w = w; c->fr.h = h; c->fr.max_bounces = max_bounces; c->fr.n_owned = (uint32_t)n_owned; c->fr.owned = c->owned.p;
  c->fr.seed_hash = seed_hash(seed);
  // the path integrator's camera frames number a batch's paths in the context's order; raster frames (one sample), probe frames (k_raygen_probe and
  // k_accumulate_sh, whose order ptc_debug_probe_project publishes) and lightmap frames (k_raygen_texel, k_lm_first_hit) stay sample-major
  c->fr.path_order = is_raster(integrator) || entries ? PT_ORDER_SAMPLE : c->path_order;
  c->spp_total = is_raster(integrator) ? 1 : spp_total;
  c->integrator = integrator; c->samples_done = 0; c->sample_base = 0; c->resolve_divisor = 0;
  // samples of one full batch: as many as fit max_batch_paths split over the lanes.  The queues themselves are sized by the
  // batches actually issued (frame_add_samples), not by spp_total: a progressive loop adding one sample at a time needs
  // queues for one sample per pixel only.
  size_t batch_paths = c->max_batch_paths;
  size_t min_cap = (size_t)-1;
  for (const auto& ln : c->lanes) min_cap = ln.q.cap < min_cap ? ln.q.cap : min_cap;
  if (n_owned && (uint64_t)n_owned * (uint64_t)c->spp_total <= (uint64_t)min_cap) {
    // the whole frame fits the queues every lane already has (frame_add_samples refuses more than spp_total): nothing will be allocated,
    // no need to ask the driver how much memory is free (a call of 0.1-0.2 ms, every frame of a viewer's loop)
  } else {   // no more than 60 % of the device memory that is free now (plus what the lanes' queues already hold) goes into queues
    size_t free_b = 0, total_b = 0, held = 0;
    const size_t per_path = kQueueBytesPerPath + (alpha_on(c) ? kAlphaBytesPerPath : 0) + (glass_on(c) ? kGlassBytesPerPath : 0) + (glass_shadows_on(c) ? kGlassFlagBytesPerPath : 0) +
                            (medium_on(c) ? kMediumBytesPerPath : 0);
    for (const auto& ln : c->lanes)
      held += (size_t)ln.q.cap * kQueueBytesPerPath + (size_t)ln.alpha.q.cap * kAlphaBytesPerPath + (size_t)ln.glass.q.cap * (kGlassBytesPerPath + (ln.glass.flags ? kGlassFlagBytesPerPath : 0)) +
              (size_t)ln.medium.cap * kMediumBytesPerPath;
    if (hipMemGetInfo(&free_b, &total_b) == hipSuccess) {
      const size_t fit = (size_t)(0.6 * (double)(free_b + held)) / per_path;
      if (fit < batch_paths) batch_paths = fit;
    }
  }
  c->frame_batch_paths = batch_paths;
  c->per_batch = batch_samples(c, n_owned, batch_paths);
  for (auto& ln : c->lanes) HIP_TRY(c, hipMemsetAsync(ln.q.stats, 0, ST_N * ST_STRIDE * sizeof(unsigned long long), ln.stream));
  { int rs = sync_all_lanes(c); if (rs) return rs; }     // accum/radiance/statistics are cleared before any lane starts
  c->batches_issued = 0;
  collect_times(c, true);      // all lanes are idle: every span is complete; the previous frame's times are dropped below
  ptc_stats keep = c->stats;
  std::memset(&c->stats, 0, sizeof c->stats);
  c->stats.seconds_commit = keep.seconds_commit; c->stats.seconds_refit = keep.seconds_refit; c->stats.n_triangles = keep.n_triangles; c->stats.n_bvh_nodes = keep.n_bvh_nodes;
  c->stats.n_emitters = keep.n_emitters; c->stats.bvh_max_depth = keep.bvh_max_depth;
  c->stats.bvh_sa_cost = keep.bvh_sa_cost; c->stats.bvh_sa_cost_built = keep.bvh_sa_cost_built; c->stats.seconds_rebuild = keep.seconds_rebuild;
  c->alpha.seconds = 0.0; c->alpha.frame_layers = c->alpha.max_layers;
  c->glass.seconds = 0.0; c->glass.frame_interactions = c->glass.max_interactions;
  c->medium.seconds = 0.0;
  c->in_frame = true;
  c->probes.on = probe_pos != nullptr; c->lightmap.on = lightmap;
  if (probe_pos) c->probes.base = entries->base;
  if (lightmap) c->lightmap.base = entries->base;
  return PTC_OK;
}
}  // namespace ptc_detail

// =================================================================================================

extern "C" {
int ptc_abi_version(void) { return PTC_ABI_VERSION; }

#ifndef PTC_KERNEL_SHA
#define PTC_KERNEL_SHA "unknown"
#endif
// How the library launches: the kernels' compile-time constants, then what the context (or, without one, a fresh context with an empty environment) uses.
// A roofline figure belongs to a launch policy as much as to a kernel source: tools/make_kernel_model.py records this string, bench.py compares.
const char* ptc_launch_policy(const ptc_ctx* c) {
  static thread_local std::string out;
  static const ptc_ctx defaults;                     // member initialisers = the built-in defaults (ptc_create then reads the environment)
  const ptc_ctx& x = c ? *c : defaults;
  char buf[512];
  std::snprintf(buf, sizeof buf, " | stack_lds_max=6 segments_per_cu_default=64 nodelets=%u lanes=%d batch_paths=%zu trace_overlap=%d(<=2^26 paths) rays_per_lane=%d shade_sort=%d refit=%s bvh=%s path_order=%s",
                x.toplet_budget, x.n_lanes, x.max_batch_paths, x.trace_overlap, x.trace_rays_per_lane, x.cfg.shade_sort, x.refit_on_device ? "device" : "host",
                x.bvh_builder == PTC_BVH_LBVH ? "lbvh" : "sah", x.path_order == PT_ORDER_PIXEL ? "pixel" : "sample");
  out = std::string(pt_kernel_policy()) + buf;
  if (c && c->committed && c->device >= 0) {
    std::snprintf(buf, sizeof buf, " | trace_blocks_per_cu=%d stack_lds=%d lds_units=%u ovf_depth=%u shade_segments=%d shade_tables_lds=%d", c->cfg.trace_blocks_per_cu, c->cfg.stack_lds,
                  c->scene.dsc.n_lds_units, c->scene.dsc.ovf_depth, c->cfg.shade_waves, c->cfg.shade_tables_lds);
    out += buf;
  }
  return out.c_str();
}

const char* ptc_build_info(void) { return "ptc abi " PTC_STR(PTC_ABI_VERSION) " gfx950 kernels-sha256 " PTC_KERNEL_SHA; }

ptc_ctx* ptc_create(int device_id) {
  if (device_id == PTC_DEVICE_NONE) {   // description-only context: host flatten + BVH build, no rendering
    ptc_ctx* c = new ptc_ctx();
    c->device = PTC_DEVICE_NONE;
    read_build_environment(c);
    return c;
  }
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess || n <= 0) { g_create_error = std::string("ptc_create: no HIP device (") + hipGetErrorString(e) + "); this library has no CPU path"; return nullptr; }
  if (device_id < 0 || device_id >= n) { g_create_error = "ptc_create: device id out of range"; return nullptr; }
  if ((e = hipSetDevice(device_id)) != hipSuccess) { g_create_error = std::string("ptc_create: hipSetDevice: ") + hipGetErrorString(e); return nullptr; }
  hipDeviceProp_t prop;
  if ((e = hipGetDeviceProperties(&prop, device_id)) != hipSuccess) { g_create_error = std::string("ptc_create: ") + hipGetErrorString(e); return nullptr; }
  if (std::string(prop.gcnArchName).rfind("gfx950", 0) != 0) { g_create_error = std::string("ptc_create: device is ") + prop.gcnArchName + ", this library is built for gfx950 only"; return nullptr; }
  ptc_ctx* c = new ptc_ctx();
  c->device = device_id;
  c->cfg.n_cu = prop.multiProcessorCount;
  c->cfg.trace_blocks_per_cu = 4;
  c->cfg.stack_lds = 6;
  {   // segments of a queue = waves of k_shade's grid; a CU holds 16 of them at a time (4 waves per SIMD).  Whole multiples of 16 only: 8 / 12 / 20 / 24 leave a
      // partial round and cost 4-20 %.  With the round-3b kernel (global instead of FLAT gathers) 16 / 32 / 48 / 64 per CU give k_shade 0.1296 / 0.1296 / 0.1245 / 0.1236 s
      // per 6 steps on the atrium and 0.1768 / 0.1973 / 0.1902 / 0.1851 on the textured atrium (profiles/r03_shade_segments.txt): four short rounds beat two,
      // one round is best where every segment costs the same and worst where they do not.  64 = PTC_MAX_SEGMENTS / 256 CUs.
    int per_cu = 64;
    if (const char* s = std::getenv("PTC_SEGMENTS_PER_CU")) { int v = std::atoi(s); if (v >= 1 && v <= 64) per_cu = v; }
    uint32_t n = (uint32_t)(c->cfg.n_cu * per_cu);
    c->cfg.shade_waves = (int)(n > PTC_MAX_SEGMENTS ? PTC_MAX_SEGMENTS : n);
  }
  // P9's material sort is built and bit-exact either way, and OFF by default: k_shade runs at the rate of the CUs' memory path, so class-uniform
  // waves buy nothing, while the sort reads the hit words a second time and turns the ray loads into gathers: -11 % k_shade time without it on the
  // atrium, -5 % on the textured atrium (profiles/r03_shade_variants.txt).  Output compaction (ballot + mbcnt prefix) is always on.
  if (const char* s = std::getenv("PTC_SHADE_SORT")) c->cfg.shade_sort = std::atoi(s) != 0 ? 1 : 0;
  if (const char* s = std::getenv("PTC_TRACE_RAYS_PER_LANE")) { int v = std::atoi(s); if (v >= 1 && v <= 4096) c->trace_rays_per_lane = v; }
  if (const char* s = std::getenv("PTC_TRACE_OVERLAP")) { int v = std::atoi(s); if (v >= 0 && v <= 2) c->trace_overlap = v; }
  read_build_environment(c);
  if (const char* s = std::getenv("PTC_BATCH_PATHS")) { size_t v = std::strtoull(s, nullptr, 10); if (v >= 1024) c->max_batch_paths = v; }
  if (const char* s = std::getenv("PTC_TIMING")) { const int v = std::atoi(s); c->timing = v < 0 ? 0 : (v > 2 ? 2 : v); }
  if (const char* s = std::getenv("PTC_LANES")) { int v = std::atoi(s); if (v >= 1 && v <= 8) c->n_lanes = v; }
  if (const char* s = std::getenv("PTC_PATH_ORDER")) { if (std::strcmp(s, "sample") == 0) c->path_order = PT_ORDER_SAMPLE; else if (std::strcmp(s, "pixel") == 0) c->path_order = PT_ORDER_PIXEL; }
  c->lanes.resize((size_t)c->n_lanes);
  bool ok = true;
  for (auto& ln : c->lanes) {
    ok = ok && hipStreamCreateWithFlags(&ln.stream, hipStreamNonBlocking) == hipSuccess && hipEventCreateWithFlags(&ln.acc_done, hipEventDisableTiming) == hipSuccess;
    ok = ok && hipMalloc((void**)&ln.q.cnt, CNT_N * sizeof(uint32_t)) == hipSuccess && hipMalloc((void**)&ln.q.stats, ST_N * ST_STRIDE * sizeof(unsigned long long)) == hipSuccess;
    ok = ok && hipMemset(ln.q.cnt, 0, CNT_N * sizeof(uint32_t)) == hipSuccess && hipMemset(ln.q.stats, 0, ST_N * ST_STRIDE * sizeof(unsigned long long)) == hipSuccess;
    uint32_t* segs = nullptr;                                     // seg_ray[2], seg_sh, pre_ray, pre_sh: one allocation
    const size_t per = PTC_MAX_SEGMENTS + 64;
    ok = ok && hipMalloc((void**)&segs, 5 * per * sizeof(uint32_t)) == hipSuccess && hipMemset(segs, 0, 5 * per * sizeof(uint32_t)) == hipSuccess;
    if (ok) { ln.q.seg_ray[0] = segs; ln.q.seg_ray[1] = segs + per; ln.q.seg_sh = segs + 2 * per; ln.q.pre_ray = segs + 3 * per; ln.q.pre_sh = segs + 4 * per; }
    ok = ok && hipMalloc((void**)&ln.d_scene, sizeof(DevScene)) == hipSuccess;
  }
  if (!ok) { g_create_error = "ptc_create: could not create the lane streams / events / counters"; ptc_destroy(c); return nullptr; }
  return c;
}

void ptc_destroy(ptc_ctx* c) {
  if (!c) return;
  if (c->device < 0) { delete c; return; }
  (void)hipSetDevice(c->device);
  for (auto& ln : c->lanes) if (ln.stream) (void)hipStreamSynchronize(ln.stream);
  if (c->comm.handle && c->comm.owned && g_rccl.so) (void)g_rccl.CommDestroy(c->comm.handle);
  for (const Span& s : c->spans) { (void)hipEventDestroy(s.a); (void)hipEventDestroy(s.b); }
  for (hipEvent_t e : c->free_events) (void)hipEventDestroy(e);
  for (auto& ln : c->lanes) ln.teardown();
  release_scene(c);
  if (c->bscratch.p) (void)hipFree(c->bscratch.p);
  delete c;      // the device is current and idle: every DevBuf and StageTimer of the frame and the features frees what it holds
}

const char* ptc_last_error(const ptc_ctx* c) { return c ? c->err.c_str() : g_create_error.c_str(); }

int ptc_frame_begin(ptc_ctx* c, int w, int h, int spp_total, uint64_t seed, int max_bounces, int integrator, int tile_rank, int tile_count) {
  return frame_begin(c, w, h, spp_total, seed, max_bounces, integrator, tile_rank, tile_count, nullptr);
}

int ptc_frame_reserve(ptc_ctx* c) {
  { int rd = need_device(c); if (rd) return rd; }
  if (!c->in_frame) return fail(c, PTC_E_STATE, "frame_reserve: no frame");
  if (c->fr.n_owned == 0) return PTC_OK;
  const uint32_t k = is_raster(c->integrator) ? 1u : (c->per_batch < (uint32_t)c->spp_total ? c->per_batch : (uint32_t)c->spp_total);
  { int rc = ensure_lane_queues(c, c->fr.n_owned * k); if (rc) return rc; }     // n_owned * per_batch fits 32 bits by construction (frame_begin)
  if (alpha_on(c)) { int rc = ensure_alpha_queues(c); if (rc) return rc; }
  return glass_on(c) ? ensure_glass_queues(c) : PTC_OK;
}

int ptc_frame_add_samples(ptc_ctx* c, int n_samples) {
  { int rd = need_device(c); if (rd) return rd; }
  if (!c->in_frame) return fail(c, PTC_E_STATE, "frame_add_samples: no frame");
  if (n_samples <= 0) return fail(c, PTC_E_ARG, "frame_add_samples: n_samples <= 0");
  if (c->adaptive.on && c->fr.n_owned == 0) return PTC_OK;      // nothing is active: accepted, nothing to do
  if (!is_raster(c->integrator) && (uint64_t)c->samples_done + c->pending + (uint64_t)n_samples > (uint64_t)c->spp_total)
    return fail(c, PTC_E_ARG, "frame_add_samples: more samples than the spp_total given to frame_begin");
  c->pending += (uint32_t)n_samples;
  c->adaptive.cov_resolved = false;          // the sums are about to hold samples the radiance buffer does not (ptc_denoise_sampled)
  // full batches go out at once; a remainder waits for more samples (or for resolve / sync / a read-back), so that many
  // small calls still produce full-width launches
  while (c->pending >= c->per_batch) {
    c->pending -= c->per_batch;
    if (c->fr.n_owned == 0) { c->samples_done += c->per_batch; continue; }
    int rc = issue(c, c->per_batch);
    if (rc) return rc;
  }
  return PTC_OK;
}

int ptc_frame_resolve(ptc_ctx* c) {
  { int rd = need_device(c); if (rd) return rd; }
  if (!c->in_frame) return fail(c, PTC_E_STATE, "frame_resolve: no frame");
  { int rf = flush(c); if (rf) return rf; }
  { int rj = join_lanes_on_stream0(c); if (rj) return rj; }
  // divisor: the samples accumulated so far, so a progressive viewer sees a correctly exposed image after every call
  if (c->adaptive.on) { if (c->samples_done) pt_launch_ad_resolve(c->lanes[0].stream, c->owned_n, c->owned.p, c->accum.p, c->adaptive.count.p, c->radiance.p); }
  else if (c->fr.n_owned && c->samples_done)
    pt_launch_resolve(c->lanes[0].stream, c->fr, c->accum.p, c->radiance.p, (float)(c->resolve_divisor ? c->resolve_divisor : c->samples_done), is_raster(c->integrator));
  HIP_TRY(c, hipGetLastError());
  c->adaptive.cov_resolved = true;
  return PTC_OK;
}

int ptc_frame_set_sample_range(ptc_ctx* c, uint32_t first_sample, uint32_t resolve_divisor) {
  { int rd = need_device(c); if (rd) return rd; }
  if (!c->in_frame) return fail(c, PTC_E_STATE, "frame_set_sample_range: no frame");
  if (c->samples_done || c->pending) return fail(c, PTC_E_STATE, "frame_set_sample_range: call it right after ptc_frame_begin, before any sample");
  if (is_raster(c->integrator)) return fail(c, PTC_E_ARG, "frame_set_sample_range: the raster integrators have one sample");
  if ((uint64_t)first_sample + (uint64_t)c->spp_total > 0xffffffffull) return fail(c, PTC_E_ARG, "frame_set_sample_range: sample indices exceed 32 bits");
  if (c->adaptive.on && resolve_divisor) return fail(c, PTC_E_STATE, "frame_set_sample_range: an adaptive frame resolves every pixel by its own count, not by a divisor");
  c->sample_base = first_sample; c->resolve_divisor = resolve_divisor;
  return PTC_OK;
}

int ptc_frame_checkpoint(ptc_ctx* c, float* accum_rgba, uint64_t* n_owned_pixels, uint32_t* samples_done) {
  { int rd = need_device(c); if (rd) return rd; }
  if (!c->in_frame) return fail(c, PTC_E_STATE, "frame_checkpoint: no frame");
  if (is_raster(c->integrator)) return fail(c, PTC_E_ARG, "frame_checkpoint: the raster integrators have nothing to resume");
  if (c->adaptive.on) return fail(c, PTC_E_STATE, "frame_checkpoint: not available in an adaptive frame");
  if (entry_frame(c)) return fail(c, PTC_E_STATE, "frame_checkpoint: not available in a probe or lightmap frame");
  { int rf = flush(c); if (rf) return rf; }
  { int rs = sync_all_lanes(c); if (rs) return rs; }
  if (n_owned_pixels) *n_owned_pixels = c->fr.n_owned;
  if (samples_done) *samples_done = c->samples_done;
  if (accum_rgba && c->fr.n_owned) HIP_TRY(c, hipMemcpy(accum_rgba, c->accum.p, (size_t)c->fr.n_owned * sizeof(float4), hipMemcpyDeviceToHost));
  return PTC_OK;
}

int ptc_frame_restore(ptc_ctx* c, const float* accum_rgba, uint64_t n_owned_pixels, uint32_t samples_done) {
  { int rd = need_device(c); if (rd) return rd; }
  if (!c->in_frame) return fail(c, PTC_E_STATE, "frame_restore: no frame (ptc_frame_begin with the checkpointed frame's parameters first)");
  if (entry_frame(c)) return fail(c, PTC_E_STATE, "frame_restore: not available in a probe or lightmap frame");
  if (!accum_rgba) return fail(c, PTC_E_ARG, "frame_restore: null pointer");
  if (c->adaptive.on) return fail(c, PTC_E_STATE, "frame_restore: not available in an adaptive frame");
  if (c->samples_done || c->pending) return fail(c, PTC_E_STATE, "frame_restore: call it right after ptc_frame_begin, before any sample");
  if (is_raster(c->integrator)) return fail(c, PTC_E_ARG, "frame_restore: the raster integrators have nothing to resume");
  if (n_owned_pixels != c->fr.n_owned) return fail(c, PTC_E_ARG, "frame_restore: the checkpoint is of another frame (size or tile share differ)");
  if (samples_done > (uint32_t)c->spp_total) return fail(c, PTC_E_ARG, "frame_restore: more samples than this frame's spp_total");
  { int rs = sync_all_lanes(c); if (rs) return rs; }
  if (c->fr.n_owned) HIP_TRY(c, hipMemcpy(c->accum.p, accum_rgba, (size_t)c->fr.n_owned * sizeof(float4), hipMemcpyHostToDevice));
  c->samples_done = samples_done;
  return PTC_OK;
}

int ptc_sync(ptc_ctx* c) {
  { int rd = need_device(c); if (rd) return rd; }
  { int rf = flush(c); if (rf) return rf; }
  return sync_all_lanes(c);
}

int ptc_render(ptc_ctx* c, int w, int h, int spp, uint64_t seed, int max_bounces, int integrator) {
  int rc = ptc_frame_begin(c, w, h, spp, seed, max_bounces, integrator, 0, 1);
  if (rc) return rc;
  if ((rc = ptc_frame_add_samples(c, spp))) return rc;
  if ((rc = ptc_frame_resolve(c))) return rc;
  return ptc_sync(c);
}

int ptc_read_radiance_rgba32f(ptc_ctx* c, float* out) {
  return read_image(c, "read_radiance", out, sizeof(float4), /*all_lanes=*/true, [&](const void*& src) -> int {
    if (!c->radiance.p || c->rad_w == 0) return fail(c, PTC_E_STATE, "read_radiance: nothing rendered");
    src = served_image(c);
    return PTC_OK;
  });
}

void* ptc_radiance_device_ptr(ptc_ctx* c) { return (c && c->device >= 0) ? (void*)c->radiance.p : nullptr; }

int ptc_read_radiance_rgba16f(ptc_ctx* c, uint16_t* out) {
  { int rd = need_device(c); if (rd) return rd; }
  if (!out) return fail(c, PTC_E_ARG, "read_radiance_rgba16f: null pointer");
  { int rc = convert_half(c); if (rc) return rc; }
  HIP_TRY(c, hipStreamSynchronize(c->lanes[0].stream));
  HIP_TRY(c, hipMemcpy(out, c->half.p, (size_t)c->rad_w * c->rad_h * sizeof(uint2), hipMemcpyDeviceToHost));
  return PTC_OK;
}
void* ptc_radiance_rgba16f_device_ptr(ptc_ctx* c) {
  if (need_device(c)) return nullptr;
  if (convert_half(c)) return nullptr;
  if (hipStreamSynchronize(c->lanes[0].stream) != hipSuccess) return nullptr;
  return (void*)c->half.p;
}

int ptc_write_radiance_rgba32f(ptc_ctx* c, const float* in) {
  { int rd = need_device(c); if (rd) return rd; }
  if (!in) return fail(c, PTC_E_ARG, "write_radiance: null pointer");
  if (!c->radiance.p || c->rad_w == 0) return fail(c, PTC_E_STATE, "write_radiance: no frame");
  { int rs = sync_all_lanes(c); if (rs) return rs; }     // every lane: a resolve or a reduce may still be writing the buffer
  HIP_TRY(c, hipMemcpy(c->radiance.p, in, (size_t)c->rad_w * c->rad_h * sizeof(float4), hipMemcpyHostToDevice));
  return PTC_OK;
}

int ptc_tonemap_rgba8(ptc_ctx* c, uint8_t* out) {
  { int rd = need_device(c); if (rd) return rd; }
  if (!out) return fail(c, PTC_E_ARG, "tonemap: null pointer");
  if (!c->radiance.p || c->rad_w == 0) return fail(c, PTC_E_STATE, "tonemap: nothing rendered");
  int rc;
  if ((rc = ensure_buf(c, c->ldr, (size_t)c->rad_w * c->rad_h))) return rc;
  hipStream_t s0 = c->lanes[0].stream;
  pt_launch_tonemap(s0, served_image(c), c->ldr.p, c->rad_w, c->rad_h);
  HIP_TRY(c, hipGetLastError());
  HIP_TRY(c, hipStreamSynchronize(s0));
  HIP_TRY(c, hipMemcpy(out, c->ldr.p, (size_t)c->rad_w * c->rad_h * 4, hipMemcpyDeviceToHost));
  return PTC_OK;
}

int ptc_get_stats(ptc_ctx* c, ptc_stats* out) {
  if (!c) return PTC_E_ARG;
  if (!out) return fail(c, PTC_E_ARG, "get_stats: null pointer");
  if (c->device < 0) { *out = c->stats; return PTC_OK; }
  HIP_TRY(c, hipSetDevice(c->device));
  { int rf = flush(c); if (rf) return rf; }
  { int rs = sync_all_lanes(c); if (rs) return rs; }
  unsigned long long st[ST_N];
  { int rc = sum_lane_stats(c, st); if (rc) return rc; }
  ptc_stats& s = c->stats;
  s.segments = st[ST_SEGMENTS]; s.shadow_rays = st[ST_SHADOW]; s.hits = st[ST_HITS];
  s.node_visits_closest = st[ST_NODES_C]; s.tri_tests_closest = st[ST_TRIS_C];
  s.node_visits_any = st[ST_NODES_A]; s.tri_tests_any = st[ST_TRIS_A];
  // SURVEY §8d byte model with this build's record sizes (DESIGN.md §"Algorithmic bytes")
  s.algorithmic_bytes = s.segments * (2u * 56u + 2u * 16u) + s.node_visits_closest * 64u + s.tri_tests_closest * 48u + s.hits * 176u +
                        s.shadow_rays * (2u * 44u) + s.node_visits_any * 64u + s.tri_tests_any * 48u + s.paths * (2u * 16u);
  collect_times(c, true);
  *out = c->stats;
  return PTC_OK;
}
}  // extern "C"

