// ptc_api_multi.cpp — multi-GPU: RCCL, loaded on first use; a context's communicator (ptc_comm_*); groups of contexts that share one host build (ptc_group_*).
#include "ptc_ctx.h"

#include <dlfcn.h>

using namespace ptc_detail;

namespace ptc_detail {
Rccl g_rccl;
}  // namespace ptc_detail

namespace {
bool rccl_load() {
  if (g_rccl.so) return true;
  void* so = dlopen("librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
  if (!so) so = dlopen("librccl.so", RTLD_NOW | RTLD_GLOBAL);
  if (!so) so = dlopen("/opt/rocm/lib/librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
  if (!so) { const char* e = dlerror(); g_rccl.err = std::string("librccl.so not loadable: ") + (e ? e : "?"); return false; }
  bool ok = true;
  auto sym = [&](const char* name) { void* p = dlsym(so, name); if (!p) { ok = false; g_rccl.err = std::string("librccl.so lacks ") + name; } return p; };
  g_rccl.GetUniqueId = (decltype(g_rccl.GetUniqueId))sym("ncclGetUniqueId");
  g_rccl.CommInitRank = (decltype(g_rccl.CommInitRank))sym("ncclCommInitRank");
  g_rccl.CommInitAll = (decltype(g_rccl.CommInitAll))sym("ncclCommInitAll");
  g_rccl.CommDestroy = (decltype(g_rccl.CommDestroy))sym("ncclCommDestroy");
  g_rccl.Reduce = (decltype(g_rccl.Reduce))sym("ncclReduce");
  g_rccl.GroupStart = (decltype(g_rccl.GroupStart))sym("ncclGroupStart");
  g_rccl.GroupEnd = (decltype(g_rccl.GroupEnd))sym("ncclGroupEnd");
  g_rccl.GetErrorString = (decltype(g_rccl.GetErrorString))sym("ncclGetErrorString");
  if (!ok) { dlclose(so); return false; }
  g_rccl.so = so;
  return true;
}
}  // namespace

extern "C" {
// ---- multi-GPU: RCCL reduce of the framebuffer ----------------------------------------------------------
int ptc_comm_unique_id(uint8_t out[PTC_COMM_ID_BYTES]) {
  static_assert(PTC_COMM_ID_BYTES == NCCL_UNIQUE_ID_BYTES, "ptc.h mirrors NCCL_UNIQUE_ID_BYTES");
  if (!out) return PTC_E_ARG;
  if (!rccl_load()) { g_create_error = g_rccl.err; return PTC_E_DEVICE; }
  ncclUniqueId id;
  const ncclResult_t r = g_rccl.GetUniqueId(&id);
  if (r != ncclSuccess) { g_create_error = std::string("ncclGetUniqueId: ") + g_rccl.GetErrorString(r); return PTC_E_DEVICE; }
  std::memcpy(out, id.internal, PTC_COMM_ID_BYTES);
  return PTC_OK;
}

int ptc_comm_init(ptc_ctx* c, const uint8_t id[PTC_COMM_ID_BYTES], int rank, int n_ranks) {
  { int rd = need_device(c); if (rd) return rd; }
  if (!id || n_ranks < 1 || rank < 0 || rank >= n_ranks) return fail(c, PTC_E_ARG, "comm_init: bad argument");
  if (c->comm.handle) return fail(c, PTC_E_STATE, "comm_init: this context already has a communicator");
  if (!rccl_load()) return fail(c, PTC_E_DEVICE, g_rccl.err);
  ncclUniqueId uid;
  std::memcpy(uid.internal, id, PTC_COMM_ID_BYTES);
  NCCL_TRY(c, g_rccl.CommInitRank(&c->comm.handle, n_ranks, uid, rank));
  c->comm.rank = rank; c->comm.size = n_ranks; c->comm.owned = true;
  return PTC_OK;
}

int ptc_comm_reduce_radiance(ptc_ctx* c, int root) {
  { int rd = need_device(c); if (rd) return rd; }
  if (entry_frame(c)) return fail(c, PTC_E_STATE, "comm_reduce_radiance: a probe or lightmap frame is not a tile share of an image (shard probes by probe_index_base, texels by texel_index_base)");
  if (!c->comm.handle) return fail(c, PTC_E_STATE, "comm_reduce_radiance: no communicator (ptc_comm_init / ptc_group_create)");
  if (root < 0 || root >= c->comm.size) return fail(c, PTC_E_ARG, "comm_reduce_radiance: bad root");
  if (!c->radiance.p || c->rad_w == 0) return fail(c, PTC_E_STATE, "comm_reduce_radiance: nothing rendered");
  // in place on stream 0, behind the resolve: ranks own disjoint tiles and hold zeros elsewhere, so the fp32 sum is x + 0
  ScopedSpan t(c, c->lanes[0].stream, 4);            // seconds_reduce: the collective as this rank's stream sees it (it includes waiting for the slowest rank)
  NCCL_TRY(c, g_rccl.Reduce(c->radiance.p, c->radiance.p, (size_t)c->rad_w * c->rad_h * 4, ncclFloat32, ncclSum, root, c->comm.handle, c->lanes[0].stream));
  return PTC_OK;
}

int ptc_comm_destroy(ptc_ctx* c) {
  { int rd = need_device(c); if (rd) return rd; }
  if (!c->comm.handle) return PTC_OK;
  if (!c->comm.owned) return fail(c, PTC_E_STATE, "comm_destroy: the communicator belongs to a ptc_group");
  { int rs = sync_all_lanes(c); if (rs) return rs; }
  NCCL_TRY(c, g_rccl.CommDestroy(c->comm.handle));
  c->comm.handle = nullptr; c->comm.size = 0;
  return PTC_OK;
}

ptc_group* ptc_group_create(const int* device_ids, int n_devices) {
  if (!device_ids || n_devices < 1 || n_devices > 64) { g_create_error = "ptc_group_create: bad argument"; return nullptr; }
  bool none = true;
  for (int i = 0; i < n_devices; ++i) none = none && device_ids[i] == PTC_DEVICE_NONE;
  if (none) {      // a description-only group (every id PTC_DEVICE_NONE): the host half of the group calls — one build shared by all contexts — without GPUs or RCCL
    ptc_group* g = new ptc_group();
    for (int i = 0; i < n_devices; ++i) g->ctx.push_back(ptc_create(PTC_DEVICE_NONE));
    return g;
  }
  if (!rccl_load()) { g_create_error = g_rccl.err; return nullptr; }
  ptc_group* g = new ptc_group();
  for (int i = 0; i < n_devices; ++i) {
    ptc_ctx* c = ptc_create(device_ids[i]);
    if (!c) { ptc_group_destroy(g); return nullptr; }
    g->ctx.push_back(c);
  }
  g->comms.resize((size_t)n_devices, nullptr);
  const ncclResult_t r = g_rccl.CommInitAll(g->comms.data(), n_devices, device_ids);
  if (r != ncclSuccess) { g_create_error = std::string("ncclCommInitAll: ") + g_rccl.GetErrorString(r); g->comms.clear(); ptc_group_destroy(g); return nullptr; }
  for (int i = 0; i < n_devices; ++i) {
    ptc_ctx* c = g->ctx[(size_t)i];
    c->comm.handle = g->comms[(size_t)i]; c->comm.rank = i; c->comm.size = n_devices; c->comm.owned = false;
  }
  return g;
}

int ptc_group_size(const ptc_group* g) { return g ? (int)g->ctx.size() : 0; }

int ptc_group_scene_commit(ptc_group* g) {
  if (!g || g->ctx.empty()) return PTC_E_ARG;
  ptc_ctx* c0 = g->ctx[0];
  // flatten + BVH build, once, on the host (a scene device 0 has committed already is taken as it is; with the SAH device builder, a commit device 0 made on the
  // device is made again on the host: the other devices share device 0's host arrays)
  const bool sah_dev = c0->device_builder == PTC_BVH_SAH;
  int rc = c0->committed && !(sah_dev && c0->scene.commit_on_device) ? PTC_OK : scene_commit(c0, /*device_ok=*/!sah_dev);
  if (rc) { g->err = std::string("device 0: ") + ptc_last_error(c0); return rc; }
  for (size_t i = 1; i < g->ctx.size(); ++i) {
    ptc_ctx* c = g->ctx[i];
    if (c->device >= 0) {
      if (hipSetDevice(c->device) != hipSuccess) { g->err = "ptc_group_scene_commit: hipSetDevice failed"; return PTC_E_DEVICE; }
      if ((rc = sync_all_lanes(c))) { g->err = "device " + std::to_string(i) + ": " + ptc_last_error(c); return rc; }
    }
    const auto t0 = std::chrono::steady_clock::now();
    copy_description(c, c0);
    c->built = c0->built;                             // shared, read-only from here on
    if ((rc = commit_upload(c, t0, Upload::NewScene))) { g->err = "device " + std::to_string(i) + ": " + ptc_last_error(c); return rc; }
  }
  return PTC_OK;
}
ptc_ctx* ptc_group_ctx(ptc_group* g, int i) { return (g && i >= 0 && (size_t)i < g->ctx.size()) ? g->ctx[(size_t)i] : nullptr; }
const char* ptc_group_last_error(const ptc_group* g) { return g ? g->err.c_str() : g_create_error.c_str(); }

int ptc_group_scene_refit(ptc_group* g) {
  if (!g || g->ctx.empty()) return PTC_E_ARG;
  ptc_ctx* c0 = g->ctx[0];
  if (!c0->committed) { g->err = "ptc_group_scene_refit: the group's scene is not committed"; return PTC_E_STATE; }
  if (!description_matches_commit(c0)) { g->err = kDescriptionChanged; return PTC_E_STATE; }
  // device 0's instances carry the new transforms (ptc_update_instance* on ptc_group_ctx(g, 0)): one refit on the host, the arrays go to every device
  for (ptc_ctx* c : g->ctx) {
    if (c->device < 0) continue;
    if (hipSetDevice(c->device) != hipSuccess) { g->err = "ptc_group_scene_refit: hipSetDevice failed"; return PTC_E_DEVICE; }
    int rc = flush(c); if (!rc) rc = temporal_keep_positions(c); if (!rc) rc = sync_all_lanes(c);
    if (rc) { g->err = std::string("ptc_group_scene_refit: ") + ptc_last_error(c); return rc; }
  }
  const auto t0 = std::chrono::steady_clock::now();
  if (c0->device >= 0 && refit_on_device(c0)) {       // every device refits its own copy in place: nothing but the 84 bytes per instance and the emitter table cross the bus
    bool host_way = false;
    auto mine = std::make_shared<HostBuilt>(*c0->built);
    for (size_t i = 0; i < g->ctx.size() && !host_way; ++i) {
      ptc_ctx* c = g->ctx[i];
      if (hipSetDevice(c->device) != hipSuccess) { g->err = "ptc_group_scene_refit: hipSetDevice failed"; return PTC_E_DEVICE; }
      if (i) { c->insts = c0->insts; deform_take(c, c0, /*with_verts=*/false); }
      c->built = mine;
      const int rc = device_refit(c, t0);
      if (rc > 0) { host_way = true; break; }      // decided from the description alone, before any kernel ran: all devices take the host path together
      if (rc) {
        g->err = "device " + std::to_string(i) + ": " + ptc_last_error(c);
        if (i == 0) return rc;                     // nothing has been refitted yet (a refused refit leaves the device's scene as it was)
        host_way = true; break;                    // devices 0..i-1 hold the new state: the host path below brings ALL of them to one state, or fails as a whole
      }
    }
    if (!host_way) return PTC_OK;
  }
  auto built = std::make_shared<HostBuilt>(*c0->built);                 // the devices keep rendering from the old arrays until theirs are overwritten
  const size_t n_recs = built->recs.size(), n_shade = built->shade.size(), n_lights = built->lights.size(), n_cdf = built->cdf.size();
  deform_host_all(c0);
  const std::string e = ptc_refit_scene(c0->mats, c0->meshes, c0->insts, c0->texs, c0->env, *built);
  if (!e.empty()) { g->err = e; return PTC_E_STATE; }
  const bool same = built->recs.size() == n_recs && built->shade.size() == n_shade && built->lights.size() == n_lights && built->cdf.size() == n_cdf;
  for (size_t i = 0; i < g->ctx.size(); ++i) {
    ptc_ctx* c = g->ctx[i];
    if (c->device >= 0 && hipSetDevice(c->device) != hipSuccess) { g->err = "ptc_group_scene_refit: hipSetDevice failed"; return PTC_E_DEVICE; }
    if (i) { c->insts = c0->insts; deform_take(c, c0, /*with_verts=*/true); }
    c->built = built;
    c->in_frame = false; c->pending = 0; drop_guides(c);
    int rc = c->device >= 0 ? refit_upload(c, same, t0) : PTC_OK;
    if (!rc) rc = deform_after_host_refit(c);
    if (rc) { g->err = "device " + std::to_string(i) + ": " + ptc_last_error(c); return rc; }
    c->stats.seconds_refit = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  }
  return PTC_OK;
}

int ptc_group_render(ptc_group* g, int w, int h, int spp, uint64_t seed, int max_bounces, int integrator) {
  if (!g || g->ctx.empty()) return PTC_E_ARG;
  const int n = (int)g->ctx.size();
  auto bail = [&](int i, int rc) { g->err = std::string("device ") + std::to_string(i) + ": " + ptc_last_error(g->ctx[(size_t)i]); return rc; };
  // every device traces all samples of its tiles; all of it is queued before anything is waited for
  for (int i = 1; i < n; ++i) { take_lights(g->ctx[(size_t)i], g->ctx[0]); take_medium(g->ctx[(size_t)i], g->ctx[0]); }
  for (int i = 0; i < n; ++i) { int rc = ptc_frame_begin(g->ctx[(size_t)i], w, h, spp, seed, max_bounces, integrator, i, n); if (rc) return bail(i, rc); }
  for (int i = 0; i < n; ++i) { int rc = ptc_frame_add_samples(g->ctx[(size_t)i], spp); if (rc) return bail(i, rc); }
  for (int i = 0; i < n; ++i) { int rc = ptc_frame_resolve(g->ctx[(size_t)i]); if (rc) return bail(i, rc); }
  if (n > 1) {
    ncclResult_t r = g_rccl.GroupStart();
    for (int i = 0; i < n && r == ncclSuccess; ++i) {
      ptc_ctx* c = g->ctx[(size_t)i];
      if (hipSetDevice(c->device) != hipSuccess) { g->err = "ptc_group_render: hipSetDevice failed"; (void)g_rccl.GroupEnd(); return PTC_E_DEVICE; }
      r = g_rccl.Reduce(c->radiance.p, c->radiance.p, (size_t)w * h * 4, ncclFloat32, ncclSum, 0, c->comm.handle, c->lanes[0].stream);
    }
    const ncclResult_t r2 = g_rccl.GroupEnd();
    if (r != ncclSuccess || r2 != ncclSuccess) { g->err = std::string("ptc_group_render: ncclReduce: ") + g_rccl.GetErrorString(r != ncclSuccess ? r : r2); return PTC_E_DEVICE; }
  }
  for (int i = 0; i < n; ++i) { int rc = ptc_sync(g->ctx[(size_t)i]); if (rc) return bail(i, rc); }
  return PTC_OK;
}

void ptc_group_destroy(ptc_group* g) {
  if (!g) return;
  for (ptc_ctx* c : g->ctx)
    if (c && c->device >= 0) { (void)hipSetDevice(c->device); for (auto& ln : c->lanes) if (ln.stream) (void)hipStreamSynchronize(ln.stream); }
  for (ncclComm_t cm : g->comms) if (cm && g_rccl.so) (void)g_rccl.CommDestroy(cm);
  for (ptc_ctx* c : g->ctx) { if (c) { c->comm.handle = nullptr; ptc_destroy(c); } }
  delete g;
}
}  // extern "C"

