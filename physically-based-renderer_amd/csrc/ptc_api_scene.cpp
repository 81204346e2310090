// ptc_api_scene.cpp — the scene half of the C-ABI: description calls, camera, lens and punctual lights, commit, refit and rebuild on host and device, mesh deformation.
//
// Three parts: the helpers of this file, what the other ptc_api*.cpp files call of it (declared in ptc_ctx.h), the C-ABI.
#include "ptc_ctx.h"
#include "pt_scene_rules.h"

#include <map>
#include <mutex>

using namespace ptc_detail;

namespace {
// pt_trace_blocks_per_cu asks the runtime four occupancy questions; the answer depends on the kernels and the LDS size alone (every device is a gfx950), so it is asked once per
// size and process (sizes above 64 KiB also set a function attribute per device and are asked every time)
int trace_blocks_per_cu_cached(size_t lds) {
  static std::mutex mu;
  static std::map<size_t, int> known;
  if (lds > 64u * 1024u) return pt_trace_blocks_per_cu(lds);
  { std::lock_guard<std::mutex> lock(mu); const auto it = known.find(lds); if (it != known.end()) return it->second; }
  const int v = pt_trace_blocks_per_cu(lds);
  if (v > 0) { std::lock_guard<std::mutex> lock(mu); known[lds] = v; }
  return v;
}

// Traversal-stack overflow slabs deep enough for the tree beyond the stack entries kept in LDS, allocated when the slabs there are shallower (a commit has none): one
// per lane, and with trace overlap the any-hit launches' own (concurrent kernels must not share one).  A lane's new slabs are allocated before its old ones are
// freed, so a failed allocation leaves the old, still valid, ones in place.
int ensure_overflow_slabs(ptc_ctx* c) {
  const int need = (int)c->built->max_depth + 2;
  const uint32_t ovf = (uint32_t)(need - c->cfg.stack_lds > 0 ? need - c->cfg.stack_lds : 1);
  if (ovf <= c->scene.dsc.ovf_depth) return PTC_OK;
  const size_t total_waves = (size_t)c->cfg.n_cu * (size_t)c->cfg.trace_blocks_per_cu * (size_t)(pt_trace_block_threads() / 64);   // the persistent grid
  for (auto& ln : c->lanes) {
    std::vector<void*> fresh;
    uint2 *a = nullptr, *b = nullptr;
    int rc = dev_alloc(c, fresh, &a, total_waves * ovf * 64);
    if (!rc && c->trace_overlap) rc = dev_alloc(c, fresh, &b, total_waves * ovf * 64);
    if (rc) { free_all(fresh); return rc; }
    ln.free_overflow_slabs();
    ln.stack_ovf = a; ln.stack_ovf2 = b;
  }
  c->scene.dsc.ovf_depth = ovf;
  return PTC_OK;
}

int configure_launch(ptc_ctx* c) {
  // Traversal stack: at most one group of pending children per tree level, so a ray needs at most depth+1 entries.
  // `stack_lds` of them live in LDS (8 B each, 512 B per level and wave), the rest in a global overflow slab.
  // LDS per block = staged top of the tree (1.2 KB) + waves·stack_lds·512 B + the 2-KiB slot-order table + the waves' prepared rays (5 KB) + 512 B static.
  // Default: the most stack entries (at most 6) with which the register limit of 8 blocks (32 waves) per CU still fits the 160 KiB of LDS — 5 since the
  // prepared rays of round 4 (19.1 KB per block).
  const int need = (int)c->built->max_depth + 2;
  int l = 6, per_cu = 0;
  bool l_forced = false;
  if (const char* e = std::getenv("PTC_STACK_LDS")) { int v = std::atoi(e); if (v >= 1 && v <= 64) { l = v; l_forced = true; } }
  if (l > need) l = need;
  size_t lds = 0;
  for (;; --l) {
    c->cfg.stack_lds = l;
    lds = pt_trace_lds_bytes(c->cfg, c->scene.dsc);
    if (lds > 160u * 1024u) { if (l > 1 && !l_forced) continue; return fail(c, PTC_E_ARG, "configure_launch: staged tree top + stack exceed the 160 KiB of LDS"); }
    per_cu = trace_blocks_per_cu_cached(lds);     // registers, static LDS and launch bounds included
    if (per_cu >= 8 || l <= 2 || l_forced) break;
  }
  if (per_cu < 1) return fail(c, PTC_E_DEVICE, "configure_launch: the trace kernels do not fit a CU with this LDS size");
  if (const char* e = std::getenv("PTC_TRACE_BLOCKS_PER_CU")) { int v = std::atoi(e); if (v >= 1 && v <= per_cu) per_cu = v; }
  c->cfg.trace_blocks_per_cu = per_cu;
  { int rc = ensure_overflow_slabs(c); if (rc) return rc; }
  if (c->trace_overlap)
    for (auto& ln : c->lanes)
      if (!ln.stream2 && hipStreamCreateWithFlags(&ln.stream2, hipStreamNonBlocking) != hipSuccess) return fail(c, PTC_E_DEVICE, "configure_launch: hipStreamCreate failed");
  return PTC_OK;
}

// Every lane's copy of the scene (k_shade reads it through a pointer), enqueued on `st`: the caller synchronises
int publish_lane_scenes(ptc_ctx* c, hipStream_t st) {
  for (int l = 0; l < c->n_lanes; ++l) {
    const DevScene ds = lane_scene(c, l);
    HIP_TRY(c, hipMemcpyAsync(c->lanes[(size_t)l].d_scene, &ds, sizeof ds, hipMemcpyHostToDevice, st));
  }
  return PTC_OK;
}

// ---- deforming meshes (pt_deform.h): the stage before the flatten ---------------------------------------------------------------------
// Gives mesh `mesh` deformation state: its base vertices are the vertices as described, and so far they are what every copy holds.
MeshPose* pose_make(ptc_ctx* c, int mesh) {
  if (c->poses.size() <= (size_t)mesh) c->poses.resize((size_t)mesh + 1);
  MeshPose& P = c->poses[(size_t)mesh];
  if (!P.active()) {
    P.base = std::make_shared<std::vector<HostVertex>>(c->meshes[(size_t)mesh].v);
    P.data = std::make_shared<DeformMesh>();
    P.data->n_verts = (uint32_t)P.base->size();
    P.base_live = P.base; P.pose_live.clear();
    P.host_fresh = P.emis_fresh = P.dev_fresh = true;      // a mesh without targets and skin evaluates to its base, bit for bit
  }
  return &P;
}
void pose_changed(MeshPose& P) { P.host_fresh = P.emis_fresh = P.dev_fresh = false; }
bool any_pose(const ptc_ctx* c) { for (const MeshPose& P : c->poses) if (P.active()) return true; return false; }

// The vertices of emissive primitives alone, for a refit on the device (the host evaluates whole meshes in deform_host_all): ptc_refit_emitters reads those from the description
void deform_host_emissive(ptc_ctx* c) {
  bool any = false;
  for (const MeshPose& P : c->poses) any = any || (P.active() && !P.emis_fresh);
  if (!any) return;
  std::vector<std::vector<float>> pose(c->poses.size());
  for (size_t m = 0; m < c->poses.size(); ++m) if (c->poses[m].active() && !c->poses[m].emis_fresh) pose[m] = c->poses[m].pose();
  const std::vector<int32_t>& E = c->scene.plan.emit_prims;
  for (size_t j = 0; j * 5 < E.size(); ++j) {
    const size_t m = (size_t)c->insts[(size_t)E[j * 5 + 1]].mesh;
    if (m >= c->poses.size() || !c->poses[m].active() || c->poses[m].emis_fresh) continue;
    const MeshPose& P = c->poses[m];
    for (int k = 0; k < 3; ++k) {
      const uint32_t v = (uint32_t)E[j * 5 + 2 + k];
      pt_deform_eval_vertex(*P.data, P.base->data(), pose[m].data(), v, c->meshes[m].v[v]);
    }
  }
  for (MeshPose& P : c->poses) if (P.active()) P.emis_fresh = true;
}
bool deform_pending_finite(const ptc_ctx* c) {
  for (const MeshPose& P : c->poses)
    if (P.active() && !P.dev_fresh && !(pt_deform_pose_finite(P.w.data(), P.w.size()) && pt_deform_pose_finite(P.J.data(), P.J.size()))) return false;
  return true;
}
// The scene in HBM was laid out from the description as it stands (a commit, a host refit or rebuild): what is pending is live now
void deform_all_live(ptc_ctx* c) {
  for (MeshPose& P : c->poses) if (P.active()) { P.pose_live = P.pose(); P.base_live = P.base; }
}

// Base vertices, deltas and skin records of every mesh with deformation state go to HBM with the refit plan and stay there
int deform_upload_mesh(ptc_ctx* c, size_t m) {
  CommittedScene& s = c->scene;
  if (s.deform.size() < s.mesh_first.size()) { s.deform.resize(s.mesh_first.size(), DevDeform{}); s.pose_stage.resize(s.mesh_first.size()); }
  {
    MeshPose& P = c->poses[m];
    const DeformMesh& D = *P.data;
    DevDeform d{};
    int rc = dev_upload(c, s.allocs, &d.base, *P.base);
    if (!rc && D.n_targets) rc = dev_upload(c, s.allocs, &d.dp, D.dp);
    if (!rc && !D.dn.empty()) rc = dev_upload(c, s.allocs, &d.dn, D.dn);
    if (!rc && !D.dt.empty()) rc = dev_upload(c, s.allocs, &d.dt, D.dt);
    if (!rc && !D.skin.empty()) rc = dev_upload(c, s.allocs, &d.skin, D.skin);
    float* pose = nullptr;
    if (!rc) rc = dev_alloc(c, s.allocs, &pose, pt_deform_pose_floats(D.n_targets, D.n_joints));
    if (rc) return rc;
    d.pose = pose; d.out = s.mesh_verts_rw + s.mesh_first[m];
    d.n_verts = D.n_verts; d.n_targets = D.n_targets; d.n_joints = D.skin.empty() ? 0u : D.n_joints;
    s.deform[m] = d;
    P.base_on_device = P.base.get();
    // the slice holds whatever the description's copy held when the plan was made: only a fully evaluated copy is the pending pose
    P.dev_fresh = P.dev_fresh && P.host_fresh;
    P.on_device = false;
  }
  return PTC_OK;
}
int deform_upload(ptc_ctx* c) {
  for (size_t m = 0; m < c->poses.size() && m < c->scene.mesh_first.size(); ++m)
    if (c->poses[m].active()) { int rc = deform_upload_mesh(c, m); if (rc) return rc; }
  return PTC_OK;
}
// Evaluates, in HBM, every mesh whose slice is not the pending pose: from the pending pose, or (live) back from the live one after a refused refit
int deform_device(ptc_ctx* c, hipStream_t st, bool live) {
  CommittedScene& s = c->scene;
  for (size_t m = 0; m < c->poses.size() && m < s.mesh_first.size(); ++m) {
    MeshPose& P = c->poses[m];
    if (!P.active() || P.dev_fresh) continue;
    if (m >= s.deform.size() || !s.deform[m].n_verts) {      // the mesh got its state after the plan was made (ptc_update_mesh_vertices on a plain mesh)
      int rc = deform_upload_mesh(c, m); if (rc) return rc;
      P.dev_fresh = false;
    }
    const DevDeform& d = s.deform[m];
    const std::shared_ptr<std::vector<HostVertex>>& base = live ? P.base_live : P.base;
    if (P.base_on_device != base.get()) {
      HIP_TRY(c, hipMemcpyAsync((void*)d.base, base->data(), base->size() * sizeof(HostVertex), hipMemcpyHostToDevice, st));
      HIP_TRY(c, hipStreamSynchronize(st));      // the source is pageable memory that may go
      P.base_on_device = base.get();
    }
    std::vector<float>& pose = s.pose_stage[m];      // the caller synchronises the stream before it returns
    pose = live ? P.pose_live : P.pose();
    if (pose.size() != pt_deform_pose_floats(d.n_targets, P.data->skin.empty() ? 0u : P.data->n_joints)) return fail(c, PTC_E_STATE, "deform: pose size does not match the mesh");
    if (!pose.empty()) HIP_TRY(c, hipMemcpyAsync((void*)d.pose, pose.data(), pose.size() * 4, hipMemcpyHostToDevice, st));
    pt_launch_deform(st, d);
    P.on_device = true;
  }
  HIP_TRY(c, hipGetLastError());
  return PTC_OK;
}
// the refit the device has completed used the pending poses: they are the live ones now
void deform_applied(ptc_ctx* c) {
  for (size_t m = 0; m < c->poses.size() && m < c->scene.deform.size(); ++m) {
    MeshPose& P = c->poses[m];
    if (!P.active() || P.dev_fresh || !c->scene.deform[m].n_verts) continue;
    P.pose_live = P.pose(); P.base_live = P.base; P.dev_fresh = true;
  }
}

void use_live_tree(ptc_ctx* c) {      // dsc and drf address the live tree set
  CommittedScene& s = c->scene;
  s.dsc.recs = s.live.recs; s.drf.recs = s.live.recs; s.drf.level_nodes = s.live.levels; s.drf.nbox = s.live.nbox;
}

// The plan of the committed scene in HBM + the scratch arrays of the refit kernels; once per commit.  The level list and the node boxes join the live tree set.
int ensure_refit_plan(ptc_ctx* c) {
  CommittedScene& s = c->scene;
  if (s.refit_ready) return PTC_OK;
  const HostBuilt& B = *c->built;
  ptc_refit_plan(c->mats, c->meshes, c->insts, B, s.plan);
  const RefitPlan& P = s.plan;
  const size_t nbox_cap = (size_t)(B.n_units / 4u + 1u) * 6;
  DevRefit d{};
  std::vector<void*> tree;
  int rc = dev_upload(c, s.allocs, &d.mesh_verts, P.mesh_verts);
  if (!rc) rc = dev_upload(c, s.allocs, &d.vert_inst, P.vert_inst);
  if (!rc) rc = dev_upload(c, s.allocs, &d.inst_first, P.inst_first);
  if (!rc) rc = dev_upload(c, s.allocs, &d.inst_src, P.inst_src);
  if (!rc) rc = dev_upload(c, s.allocs, &d.widx, B.widx);
  if (!rc) rc = dev_upload(c, tree, &d.level_nodes, P.level_nodes);
  if (!rc) rc = dev_alloc(c, s.allocs, &d.inst_xf, c->insts.size() * 21);
  if (!rc) rc = dev_alloc(c, s.allocs, &d.wverts, (size_t)P.n_verts);
  if (!rc) rc = dev_alloc(c, s.allocs, &d.wbt, (size_t)P.n_verts * 3);
  if (!rc) rc = dev_alloc(c, tree, &d.nbox, nbox_cap);
  if (!rc) rc = dev_alloc(c, s.allocs, &d.bounds, 8);
  if (!rc) rc = dev_alloc(c, s.allocs, &d.cost, 1);
  if (!rc) { std::vector<uint32_t> cls; ptc_prim_classes(c->mats, B.tri_mat, cls); rc = dev_upload(c, s.allocs, &d.prim_cls, cls); }
  if (!rc) {      // the deformation data of the posed meshes, before the tree arrays join the live set: a failure here leaves as little behind as one above
    s.mesh_verts_rw = const_cast<HostVertex*>(d.mesh_verts);
    s.mesh_first.resize(c->meshes.size());
    { uint32_t at = 0; for (size_t m = 0; m < c->meshes.size(); ++m) { s.mesh_first[m] = at; at += (uint32_t)c->meshes[m].v.size(); } }
    if (any_pose(c)) rc = deform_upload(c);
  }
  if (rc) { free_all(tree); s.deform.clear(); s.pose_stage.clear(); s.mesh_verts_rw = nullptr; return rc; }
  s.live.levels = const_cast<uint32_t*>(d.level_nodes); s.live.levels_cap = P.level_nodes.size(); s.live.nbox = d.nbox; s.live.nbox_cap = nbox_cap;
  d.shade = const_cast<float4*>(s.dsc.shade);
  d.n_verts = P.n_verts; d.n_tris = P.n_tris; d.shade_stride = B.shade_stride;
  s.drf = d;
  use_live_tree(c);
  s.refit_ready = true;
  return PTC_OK;
}

const char* const kNonFinite = "scene_commit: non-finite vertex position after the instance transform";

// What the geometry pass hands on: the instance transforms, the emitter table of the moved scene, the scene box
struct Moved { std::vector<float> xf, lights, cdf; float lo[3], hi[3]; };

// The geometry pass of a refit, a rebuild or a commit on the device: world vertices and shading records of the current transforms in HBM, the scene box.
// Returns PTC_OK, an error, or +1: "not this way" (the set of emitters changed), decided before anything is launched.
int geometry_pass(ptc_ctx* c, Moved& m) {
  CommittedScene& s = c->scene;
  if (!ptc_refit_instance_transforms(c->insts, m.xf)) return fail(c, PTC_E_STATE, kNonFinite);
  if (!deform_pending_finite(c)) return fail(c, PTC_E_STATE, kNonFinite);
  deform_host_emissive(c);
  if (!ptc_refit_emitters(c->mats, c->meshes, c->insts, s.plan, *c->built, m.lights, m.cdf)) return 1;
  hipStream_t st = c->lanes[0].stream;
  const DevRefit& d = s.drf;
  { int rc = deform_device(c, st, /*live=*/false); if (rc) return rc; }      // the posed meshes' object-space vertices, before the flatten reads them
  HIP_TRY(c, hipMemcpyAsync(d.inst_xf, m.xf.data(), m.xf.size() * 4, hipMemcpyHostToDevice, st));
  pt_launch_refit_geometry(st, d);
  uint32_t raw[8];
  HIP_TRY(c, hipMemcpyAsync(raw, d.bounds, sizeof raw, hipMemcpyDeviceToHost, st));
  HIP_TRY(c, hipStreamSynchronize(st));
  bool bad = false;
  pt_refit_decode_bounds(raw, m.lo, m.hi, &bad);
  if (bad) {     // nothing of the scene was written (k_refit_prims saw the flag); the scratch vertices go back to the state the scene in HBM was made from
    { int rc = deform_device(c, st, /*live=*/true); if (rc) return rc; }      // object-space vertices included: back to the live poses
    HIP_TRY(c, hipStreamSynchronize(st));
    if (!s.xf_live.empty()) {
      HIP_TRY(c, hipMemcpyAsync(d.inst_xf, s.xf_live.data(), s.xf_live.size() * 4, hipMemcpyHostToDevice, st));
      pt_launch_refit_geometry(st, d);
      HIP_TRY(c, hipStreamSynchronize(st));
    }
    return fail(c, PTC_E_STATE, kNonFinite);
  }
  return PTC_OK;
}

// The node pass over the live tree: the origin grid of the scene box, the nodes from the leaves up and their cost (in the unit of the build: comparable with
// bvh_sa_cost_built), the emitter table; with `publish` the lanes' copies of the scene follow (a commit publishes them after its launch configuration).
// The host's build then holds the grid, the emitters and the cost; its other vertex-dependent arrays are stale.
int node_pass(ptc_ctx* c, Moved& m, bool publish) {
  CommittedScene& s = c->scene;
  HostBuilt& B = *c->built;
  hipStream_t st = c->lanes[0].stream;
  ptc_refit_grid(m.lo, m.hi, B.grid_lo, B.grid_step, &B.ray_eps);
  pt_launch_refit_nodes(st, s.drf, s.plan.level_first, B.grid_lo, B.grid_step, B.sa_unit);
  HIP_TRY(c, hipGetLastError());
  unsigned long long cost_fixed = 0;
  HIP_TRY(c, hipMemcpyAsync(&cost_fixed, s.drf.cost, sizeof cost_fixed, hipMemcpyDeviceToHost, st));
  B.lights = m.lights; B.cdf = m.cdf;
  HIP_TRY(c, hipMemcpyAsync((void*)s.dsc.lights, B.lights.data(), B.lights.size() * 4, hipMemcpyHostToDevice, st));
  HIP_TRY(c, hipMemcpyAsync((void*)s.dsc.cdf, B.cdf.data(), B.cdf.size() * 4, hipMemcpyHostToDevice, st));
  s.dsc.ray_eps = B.ray_eps;
  for (int k = 0; k < 3; ++k) { s.dsc.grid_lo[k] = B.grid_lo[k]; s.dsc.grid_step[k] = B.grid_step[k]; }
  if (publish) { int rc = publish_lane_scenes(c, st); if (rc) return rc; }
  HIP_TRY(c, hipStreamSynchronize(st));
  B.sa_cost_fixed = cost_fixed;
  s.host_stale = true; s.last_refit_on_device = true;
  s.xf_live.swap(m.xf);
  deform_applied(c);
  return PTC_OK;
}

// A NEW tree for the vertices as they lie in HBM (pt_build.hip; builder: PTC_BVH_LBVH pt_build_lbvh, PTC_BVH_SAH pt_build_sah), written into the spare tree set, which
// becomes the live one: the replaced arrays are the next rebuild's spare set.  The host's picture of the build follows: sizes of the new tree, the arrays come back
// from HBM when somebody asks (refresh_host_copy), and the topology the host refit needs is gone — the next host-path refit builds from scratch.
int device_build(ptc_ctx* c, int builder, const Moved& m) {
  CommittedScene& s = c->scene;
  const DevRefit& d = s.drf;
  TreeBufs& t = s.spare;
  BuildOut out;      // the build owns the spare unit array and level list now (it may free them); what it hands back is the spare set's again, whatever happened
  out.recs = t.recs; out.recs_cap = t.recs_cap; out.level_nodes = t.levels; out.level_cap = t.levels_cap;
  const std::string e = builder == PTC_BVH_SAH ? pt_build_sah(c->lanes[0].stream, d.wverts, d.widx, d.prim_cls, d.n_tris, c->toplet_budget, c->bscratch, out)
                                                : pt_build_lbvh(c->lanes[0].stream, d.wverts, d.widx, d.prim_cls, d.n_tris, c->toplet_budget, c->bscratch, out);
  t.recs = out.recs; t.recs_cap = out.recs_cap; t.levels = out.level_nodes; t.levels_cap = out.level_cap;
  if (!e.empty()) return fail(c, PTC_E_DEVICE, e);
  const size_t nbox_need = (size_t)(out.n_units / 4u + 1u) * 6;
  if (t.nbox_cap < nbox_need) {
    if (t.nbox) (void)hipFree(t.nbox);
    t.nbox = nullptr; t.nbox_cap = nbox_need + nbox_need / 8u;
    if (hipMalloc((void**)&t.nbox, t.nbox_cap * sizeof(float)) != hipSuccess) { t.nbox = nullptr; t.nbox_cap = 0; return fail(c, PTC_E_NOMEM, "scene_rebuild: out of device memory"); }
  }
  std::swap(s.live, s.spare);
  use_live_tree(c);
  s.plan.level_first = out.level_first; s.plan.level_nodes.clear();
  HostBuilt& B = *c->built;
  B.sa_unit = scene_rules::half_area(m.lo, m.hi);                  // a new topology: a new unit of its cost
  B.n_nodes = out.n_nodes; B.n_units = out.n_units; B.max_depth = out.max_depth; B.n_tri_records = out.n_tri_records;
  B.n_lds_units = B.n_units < c->toplet_budget * 4u ? B.n_units : c->toplet_budget * 4u;
  B.recs.clear();                       // refresh_host_copy sizes and fills them when somebody asks
  B.topology.reset();
  s.dsc.n_lds_units = B.n_lds_units;
  return PTC_OK;
}

// ptc_scene_rebuild on the device: the geometry pass, a new tree, the node pass over it.  Returns PTC_OK, an error, or +1: "not this way" (the set of emitters changed,
// fewer than two triangles): the caller builds on the host.
int device_rebuild(ptc_ctx* c, int builder) {
  { int rc = ensure_refit_plan(c); if (rc) return rc; }
  if (c->built->n_tris < 2u) return 1;
  Moved m;
  int rc = geometry_pass(c, m);
  if (!rc) rc = device_build(c, builder, m);
  if (!rc) rc = ensure_overflow_slabs(c);      // a deeper tree needs deeper slabs
  if (!rc) rc = node_pass(c, m, /*publish=*/true);
  if (rc) return rc;
  const HostBuilt& B = *c->built;
  c->stats.bvh_sa_cost = c->stats.bvh_sa_cost_built = (double)B.sa_cost_fixed / (double)PTC_SA_COST_ONE;
  c->stats.n_bvh_nodes = B.n_nodes; c->stats.bvh_max_depth = B.max_depth;
  c->scene.tree_device_sah = builder == PTC_BVH_SAH;
  return PTC_OK;
}

// A full host build of the description as it stands + upload (what ptc_scene_commit does), keeping what a refit / rebuild keeps of the statistics.
// The tree: a rebuild's is the device builder's (the one device_rebuild would have made); a refit's is the scene's builder, or the SAH when the tree it replaces
// is a device SAH build.
int host_build_and_upload(ptc_ctx* c, std::chrono::steady_clock::time_point t0, bool as_refit) {
  deform_host_all(c);
  auto built = std::make_shared<HostBuilt>();
  const int builder = as_refit ? (c->scene.tree_device_sah ? PTC_BVH_SAH : c->bvh_builder) : c->device_builder;
  const std::string e = ptc_build_scene(c->mats, c->meshes, c->insts, c->texs, c->env, c->toplet_budget, builder, *built);
  if (!e.empty()) return fail(c, PTC_E_STATE, e);
  const ptc_stats keep = c->stats;
  c->built = built;
  const int rc = commit_upload(c, t0, Upload::SameScene);
  if (rc) return rc;
  c->scene.last_refit_on_device = false;
  const double dt = c->stats.seconds_commit;
  c->stats.seconds_commit = keep.seconds_commit; c->stats.seconds_refit = keep.seconds_refit; c->stats.seconds_rebuild = keep.seconds_rebuild;
  (as_refit ? c->stats.seconds_refit : c->stats.seconds_rebuild) = dt;
  return PTC_OK;
}

// the statistics of a commit: the figures of the build, everything else zero
void commit_stats(ptc_ctx* c, std::chrono::steady_clock::time_point t0) {
  const HostBuilt& B = *c->built;
  std::memset(&c->stats, 0, sizeof c->stats);
  c->stats.seconds_commit = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  c->stats.n_triangles = B.n_tris; c->stats.n_bvh_nodes = B.n_nodes; c->stats.n_emitters = B.n_lights; c->stats.bvh_max_depth = B.max_depth;
  c->stats.bvh_sa_cost = c->stats.bvh_sa_cost_built = (double)B.sa_cost_fixed / (double)PTC_SA_COST_ONE;
}
// the launches follow the tree (its depth, the staged top): configuration, the lanes' copies of the scene, the statistics of a commit
int commit_finish(ptc_ctx* c, std::chrono::steady_clock::time_point t0) {
  const bool timing = std::getenv("PTC_BUILD_TIMING") != nullptr;
  const auto tc0 = std::chrono::steady_clock::now();
  { int rc = configure_launch(c); if (rc) { release_scene(c); return rc; } }
  if (timing) std::fprintf(stderr, "    configure_launch            %7.2f ms\n", std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tc0).count());
  c->cfg.shade_tables_lds = pt_shade_tables_fit(c->scene.dsc) ? 1 : 0;
  { int rc = publish_lane_scenes(c, c->lanes[0].stream); if (rc) return rc; }
  HIP_TRY(c, hipStreamSynchronize(c->lanes[0].stream));
  c->committed = true;
  commit_stats(c, t0);
  return PTC_OK;
}

// ptc_scene_commit with the LBVH builder (or the SAH builder with the SAH device builder) on a device context: the host describes (ptc_build_skeleton: indices, materials, emitters, textures), the DEVICE flattens the
// vertices, writes the shading records and builds the tree (pt_refit.hip, pt_build.hip) — the arrays in HBM are byte for byte those of the host's LBVH commit
// (tests/test_gpu_parity.py, tests/test_gpu_device_sah.py).  Returns PTC_OK, an error, or +1: "not this way" (fewer than two triangles): the caller commits on the host.
int device_commit(ptc_ctx* c, std::chrono::steady_clock::time_point t0) {
  const bool timing = std::getenv("PTC_BUILD_TIMING") != nullptr;      // phase times on stderr, as the host build prints them
  auto tprev = std::chrono::steady_clock::now();
  auto lap = [&](const char* what) {
    if (!timing) return;
    const auto now = std::chrono::steady_clock::now();
    std::fprintf(stderr, "  %-28s %7.2f ms\n", what, std::chrono::duration<double, std::milli>(now - tprev).count());
    tprev = now;
  };
  auto built = std::make_shared<HostBuilt>();
  const std::string e = ptc_build_skeleton(c->mats, c->meshes, c->insts, c->texs, c->env, c->toplet_budget, *built);
  if (!e.empty()) return fail(c, PTC_E_STATE, e);
  if (built->n_tris < 2u) return 1;
  c->built = built;
  lap("describe (skeleton)");
  { int rc = commit_upload(c, t0, Upload::NewScene, /*skeleton=*/true); if (rc) return rc; }
  lap("free + tables upload");
  CommittedScene& s = c->scene;
  int rc = ensure_refit_plan(c);
  if (rc) { release_scene(c); return rc; }
  lap("plan + its upload");
  const int32_t *d_mat = nullptr, *d_light = nullptr;
  rc = dev_upload(c, s.allocs, &d_mat, built->tri_mat);
  if (!rc) rc = dev_upload(c, s.allocs, &d_light, built->prim_light);
  if (!rc) pt_launch_refit_seed(c->lanes[0].stream, s.drf, d_mat, d_light);
  Moved m;
  if (!rc) rc = geometry_pass(c, m);
  if (!rc) rc = device_build(c, c->bvh_builder, m);
  if (!rc) rc = node_pass(c, m, /*publish=*/false);
  if (rc) { release_scene(c); return rc; }
  s.tree_device_sah = c->bvh_builder == PTC_BVH_SAH;
  lap("flatten + build on the device");
  rc = commit_finish(c, t0);
  lap("launch configuration");
  s.commit_on_device = rc == PTC_OK;
  return rc;
}
}  // namespace

// ---- what ptc_api.cpp, the group calls and the debug hooks call of this file (ptc_ctx.h declares it) ----------------------------------------------
namespace ptc_detail {
// Frees every array of the committed scene, the lanes' overflow slabs included, and forgets its state; the flags of how the last calls went stay
void release_scene(ptc_ctx* c) {
  CommittedScene& s = c->scene;
  free_all(s.allocs);
  s.live.release(); s.spare.release();
  for (auto& ln : c->lanes) ln.free_overflow_slabs();
  CommittedScene fresh;
  fresh.last_refit_on_device = s.last_refit_on_device; fresh.commit_on_device = s.commit_on_device; fresh.tree_device_sah = s.tree_device_sah;
  s = std::move(fresh);
  for (MeshPose& P : c->poses) { P.base_on_device = nullptr; P.on_device = false; }
}

// The punctual lights' table as recorded -> device memory, when it changed (ptc_frame_begin, ptc_debug_punctual_nee: every lane is idle).  No light: nothing is allocated.
int upload_lights(ptc_ctx* c) {
  if (!c->lights.dirty) return PTC_OK;
  std::vector<pt_light_rec> recs; std::vector<float> cdf;
  pt_light_table(c->lights.list, recs, cdf);
  if (!recs.empty()) {
    int rc = ensure_buf(c, c->lights.recs, recs.size());
    if (!rc) rc = ensure_buf(c, c->lights.cdf, cdf.size());
    if (rc) return rc;
    HIP_TRY(c, hipMemcpy(c->lights.recs.p, recs.data(), recs.size() * sizeof(pt_light_rec), hipMemcpyHostToDevice));
    HIP_TRY(c, hipMemcpy(c->lights.cdf.p, cdf.data(), cdf.size() * sizeof(float), hipMemcpyHostToDevice));
  }
  c->lights.n_dev = (uint32_t)recs.size();
  c->lights.dirty = false;
  return PTC_OK;
}

// The host evaluates whole meshes whenever a host path needs the description (a host commit, refit or rebuild, a description-only context)
void deform_host_all(ptc_ctx* c) {
  for (size_t m = 0; m < c->poses.size(); ++m) {
    MeshPose& P = c->poses[m];
    if (!P.active() || P.host_fresh) continue;
    const std::vector<float> pose = P.pose();
    pt_deform_eval_mesh(*P.data, P.base->data(), pose.data(), c->meshes[m].v.data());
    P.host_fresh = P.emis_fresh = true;
  }
}

// A host refit rewrote the scene's arrays in place from the fully evaluated description: the object-space vertices in HBM follow, so that a later refit on the
// device starts from the same state
int deform_after_host_refit(ptc_ctx* c) {
  deform_all_live(c);
  CommittedScene& s = c->scene;
  if (c->device < 0 || !s.refit_ready) return PTC_OK;
  for (size_t m = 0; m < c->poses.size() && m < s.deform.size(); ++m) {
    MeshPose& P = c->poses[m];
    if (!P.active() || P.dev_fresh || !s.deform[m].n_verts || !P.host_fresh) continue;
    HIP_TRY(c, hipMemcpy(s.deform[m].out, c->meshes[m].v.data(), c->meshes[m].v.size() * sizeof(HostVertex), hipMemcpyHostToDevice));
    P.dev_fresh = true; P.on_device = false;
  }
  return PTC_OK;
}
// A group member takes context 0's deformation state (shared arrays, its own flags); with_verts: and the evaluated vertices, for a host path
void deform_take(ptc_ctx* c, const ptc_ctx* c0, bool with_verts) {
  if (c == c0) return;
  c->poses.resize(c0->poses.size());
  for (size_t m = 0; m < c0->poses.size(); ++m) {
    const MeshPose& Q = c0->poses[m];
    MeshPose& P = c->poses[m];
    if (!Q.active()) { P = MeshPose(); continue; }
    const bool same = P.active() && P.data == Q.data && P.base == Q.base && P.w == Q.w && P.J == Q.J;
    if (!P.active()) { P.pose_live = Q.pose_live; P.base_live = Q.base_live; }
    P.data = Q.data; P.base = Q.base; P.w = Q.w; P.J = Q.J;
    if (!same) pose_changed(P);
    if (with_verts && Q.host_fresh && m < c->meshes.size()) { c->meshes[m].v = c0->meshes[m].v; P.host_fresh = P.emis_fresh = true; }
  }
}
// Device half of a refit: c->built holds the refitted arrays.  same_sizes: overwrite in place what depends on the vertex positions (textures,
// environment and materials stay where they are); else (an emitter appeared or vanished under a degenerate scale) upload everything.
int refit_upload(ptc_ctx* c, bool same_sizes, std::chrono::steady_clock::time_point t0) {
  const HostBuilt& B = *c->built;
  DevScene& d = c->scene.dsc;
  c->scene.host_stale = false; c->scene.last_refit_on_device = false;
  if (!same_sizes) return commit_upload(c, t0, Upload::SameScene);
  HIP_TRY(c, hipMemcpy((void*)d.recs, B.recs.data(), B.recs.size() * 4, hipMemcpyHostToDevice));
  HIP_TRY(c, hipMemcpy((void*)d.shade, B.shade.data(), B.shade.size() * 4, hipMemcpyHostToDevice));
  HIP_TRY(c, hipMemcpy((void*)d.lights, B.lights.data(), B.lights.size() * 4, hipMemcpyHostToDevice));
  HIP_TRY(c, hipMemcpy((void*)d.cdf, B.cdf.data(), B.cdf.size() * 4, hipMemcpyHostToDevice));
  d.ray_eps = B.ray_eps; d.n_lights = B.n_lights;
  for (int k = 0; k < 3; ++k) { d.grid_lo[k] = B.grid_lo[k]; d.grid_step[k] = B.grid_step[k]; }
  { int rc = publish_lane_scenes(c, c->lanes[0].stream); if (rc) return rc; }
  HIP_TRY(c, hipStreamSynchronize(c->lanes[0].stream));
  return PTC_OK;
}

bool refit_on_device(ptc_ctx* c) {
  if (const char* s = std::getenv("PTC_REFIT")) return std::strcmp(s, "host") != 0;
  return c->refit_on_device != 0;
}

// A refit moves the committed scene: ptc_add_mesh / ptc_add_instance* are accepted after a commit (they describe the NEXT commit), and a refit of a
// description that has grown since would index the committed arrays out of bounds — on the device without anybody noticing.  Same test, same
// error as the host path (build_or_refit), made before anything is uploaded or launched.
bool description_matches_commit(const ptc_ctx* c) {
  if (c->insts.size() != c->scene.insts) return false;
  uint64_t nv = 0, nt = 0;
  for (const HostInstance& in : c->insts) {
    if (in.mesh < 0 || (size_t)in.mesh >= c->meshes.size()) return false;
    nv += c->meshes[(size_t)in.mesh].v.size(); nt += c->meshes[(size_t)in.mesh].idx.size() / 3;
  }
  return nv == c->built->n_wverts && nt == c->built->n_tris;
}
// a group member takes device 0's punctual lights (ptc_group_scene_commit, ptc_group_render)
void take_lights(ptc_ctx* c, const ptc_ctx* c0) {
  if (c == c0) return;
  const bool same = c->lights.list.size() == c0->lights.list.size() && (c->lights.list.empty() || std::memcmp(c->lights.list.data(), c0->lights.list.data(), c->lights.list.size() * sizeof(ptc_light_params)) == 0);
  if (!same) { c->lights.list = c0->lights.list; c->lights.dirty = true; }
}

// A group member takes device 0's description: materials are counted from it, a later ptc_scene_commit on this context rebuilds from it
void copy_description(ptc_ctx* c, const ptc_ctx* c0) {
  c->mats = c0->mats; c->meshes = c0->meshes; c->insts = c0->insts; c->texs = c0->texs; c->env = c0->env;
  c->poses.clear(); deform_take(c, c0, /*with_verts=*/false);
  for (size_t m = 0; m < c->poses.size(); ++m) if (c->poses[m].active()) c->poses[m].host_fresh = c->poses[m].emis_fresh = c0->poses[m].host_fresh;
  std::memcpy(c->cam_pos, c0->cam_pos, 12); std::memcpy(c->cam_target, c0->cam_target, 12); c->cam_fov = c0->cam_fov; c->cam_aspect = c0->cam_aspect;
  c->lens = c0->lens;
  take_camera_ex(c, c0);      // the extended camera goes wherever the camera goes
  c->alpha.mode = c0->alpha.mode; c->alpha.cutoff = c0->alpha.cutoff;      // every member builds context 0's alpha tables
  c->glass.params = c0->glass.params; c->glass.shadows = c0->glass.shadows;      // and its glass tables, with its choice of transparent shadows
  c->emtex.mats = c0->emtex.mats;      // and its emission textures
  take_lights(c, c0);
  take_medium(c, c0);
  c->have_cam = true; c->tex_linear = c0->tex_linear; c->bvh_builder = c0->bvh_builder; c->toplet_budget = c0->toplet_budget;
}

// Refit on the device (t0: the start of the call).  Returns PTC_OK, an error, or +1: "not this way" (the set of emitters changed) — the caller refits on the host.
int device_refit(ptc_ctx* c, std::chrono::steady_clock::time_point t0) {
  { int rc = ensure_refit_plan(c); if (rc) return rc; }
  Moved m;
  int rc = geometry_pass(c, m);
  if (!rc) rc = node_pass(c, m, /*publish=*/true);
  if (rc) return rc;
  c->stats.bvh_sa_cost = (double)c->built->sa_cost_fixed / (double)PTC_SA_COST_ONE;
  c->in_frame = false; c->pending = 0; drop_guides(c);
  c->stats.seconds_refit = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  return PTC_OK;
}

const char* lens_params_error(const ptc_lens_params& p) {
  if (!(p.aperture_radius >= 0.0f) || !std::isfinite(p.aperture_radius)) return "aperture_radius must be finite and >= 0";
  if (!(p.focus_distance > 0.0f) || !std::isfinite(p.focus_distance)) return "focus_distance must be finite and > 0";
  if (p.blades != 0 && (p.blades < 3 || p.blades > 16)) return "blades must be 0 (disk) or 3..16";
  if (!(p.rotation >= 0.0f && p.rotation < 1.0f)) return "rotation must be in [0, 1)";
  return nullptr;
}

// Device half of a commit: upload c->built, size the launches.  The caller has set c->built, the camera and seconds_commit's start.
// skeleton: c->built is ptc_build_skeleton's — the tables are uploaded, the shading records allocated and zeroed, there is no tree yet: device_commit goes on from here.
int commit_upload(ptc_ctx* c, std::chrono::steady_clock::time_point t0, Upload what, bool skeleton) {
  if (what == Upload::NewScene) drop_history(c);      // every commit passes here — ptc_scene_commit on the host or on the device, each context of ptc_group_scene_commit
  make_camera_in_force(c, c->cam);      // the stored look-at, or the extended camera (ptc_api_camera.cpp)
  c->in_frame = false; c->pending = 0; drop_guides(c);
  c->committed = false;
  release_scene(c);
  c->alpha.dirty = true; c->alpha.n_prims = 0;      // the alpha tables follow the primitive ids of the build being laid out: the next ptc_frame_begin uploads them (alpha_upload)
  c->glass.dirty = true; c->glass.n_prims = 0; c->glass.n_thin = 0;      // the glass tables likewise (glass_upload)
  CommittedScene& s = c->scene;
  s.insts = c->insts.size();
  deform_all_live(c);      // every caller lays the scene out from the fully evaluated description
  for (MeshPose& P : c->poses) if (P.active()) P.dev_fresh = P.host_fresh;
  emtex_commit(c);      // the textured emitters' table follows the description being laid out, on a description-only context too; the next ptc_frame_begin uploads it (emtex_upload)
  if (c->device < 0) {   // description-only context: nothing to upload
    c->committed = true;
    commit_stats(c, t0);
    return PTC_OK;
  }
  s.commit_on_device = false; s.tree_device_sah = false;
  const HostBuilt& B = *c->built;
  DevScene d{};
  int rc = 0;
  {
    const float* p = nullptr;
    if (!skeleton) {      // the unit array is the live tree set's
      std::vector<void*> tree;
      if ((rc = dev_upload(c, tree, &p, B.recs))) free_all(tree);
      s.live.recs = (float4*)p; s.live.recs_cap = B.n_units;
    }
    auto up = [&](const std::vector<float>& v, const float4** out) { if (!rc) { rc = dev_upload(c, s.allocs, &p, v); *out = (const float4*)p; } };
    up(B.mats, &d.mats); up(B.lights, &d.lights);
    if (!rc) rc = dev_upload(c, s.allocs, &d.cdf, B.cdf);
    if (!skeleton) up(B.shade, &d.shade);
    else if (!rc) {
      float4* sh = nullptr;
      const size_t units = (size_t)B.n_tris * B.shade_stride;
      rc = dev_alloc(c, s.allocs, &sh, units);
      if (!rc && hipMemsetAsync(sh, 0, units * sizeof(float4), c->lanes[0].stream) != hipSuccess) rc = fail(c, PTC_E_DEVICE, "scene_commit: hipMemset failed");
      d.shade = sh;
    }
    if (!rc) rc = dev_upload(c, s.allocs, &d.texels, B.texels);
    if (!rc) { const int32_t* ti = nullptr; rc = dev_upload(c, s.allocs, &ti, B.tex_info); d.tex_info = (const int4*)ti; }
    if (!rc) { const uint32_t* st = nullptr; rc = dev_upload(c, s.allocs, &st, B.set_texels); d.set_texels = (const uint4*)st; }
    if (!rc) { const int32_t* si = nullptr; rc = dev_upload(c, s.allocs, &si, B.set_info); d.set_info = (const int4*)si; }
    if (!rc) rc = dev_upload(c, s.allocs, &d.env_marg_guide, B.env_marg_guide);
    if (!rc) rc = dev_upload(c, s.allocs, &d.env_cond_guide, B.env_cond_guide);
    up(B.env, &d.env);
    if (!rc) rc = dev_upload(c, s.allocs, &d.env_marg, B.env_marg);
    if (!rc) rc = dev_upload(c, s.allocs, &d.env_cond, B.env_cond);
  }
  if (rc) { release_scene(c); return rc; }
  d.env_w = B.env_w; d.env_h = B.env_h; d.env_ok = B.env_ok;
  d.tex_linear = c->tex_linear;
  d.shade_stride = B.shade_stride;
  d.n_lights = B.n_lights; d.n_mats = (uint32_t)c->mats.size(); d.n_lds_units = B.n_lds_units; d.ray_eps = B.ray_eps;
  for (int k = 0; k < 3; ++k) { d.grid_lo[k] = B.grid_lo[k]; d.grid_step[k] = B.grid_step[k]; }
  s.dsc = d;
  use_live_tree(c);
  if (skeleton) return PTC_OK;
  return commit_finish(c, t0);
}

// device_ok: the commit may build on the device (not for device 0 of a group with the SAH device builder: the others share its host build)
int scene_commit(ptc_ctx* c, bool device_ok) {
  if (!c) return PTC_E_ARG;
  if (!c->have_cam) return fail(c, PTC_E_STATE, "scene_commit: no camera");
  if (c->device >= 0) {
    HIP_TRY(c, hipSetDevice(c->device));
    { int rs = sync_all_lanes(c); if (rs) return rs; }
  }
  const auto t0 = std::chrono::steady_clock::now();
  deform_host_all(c);      // a commit of a posed description is the commit of plain meshes that hold the posed vertices
  // north_star's tree builds on the device, and so does the SAH tree with the SAH device builder: PTC_COMMIT=host keeps the host's build (the cross-check path)
  if (device_ok && c->device >= 0 && (c->bvh_builder == PTC_BVH_LBVH || c->device_builder == PTC_BVH_SAH)) {
    const char* how = std::getenv("PTC_COMMIT");
    if (!(how && std::strcmp(how, "host") == 0)) {
      const int rd = device_commit(c, t0);
      if (rd <= 0) return rd;
    }
  }
  auto built = std::make_shared<HostBuilt>();
  const std::string e = ptc_build_scene(c->mats, c->meshes, c->insts, c->texs, c->env, c->toplet_budget, c->bvh_builder, *built);
  if (!e.empty()) return fail(c, PTC_E_STATE, e);
  c->built = built;
  return commit_upload(c, t0, Upload::NewScene);
}
}  // namespace ptc_detail

extern "C" {
int ptc_scene_begin(ptc_ctx* c) {
  if (!c) return PTC_E_ARG;
  if (c->device >= 0) {
    HIP_TRY(c, hipSetDevice(c->device));
    { int rs = sync_all_lanes(c); if (rs) return rs; }
  }
  c->mats.clear(); c->meshes.clear(); c->insts.clear(); c->texs.clear(); c->env = HostEnv{}; c->tex_linear = 0;
  c->bvh_builder = c->bvh_default;
  c->poses.clear();
  c->have_cam = false; c->committed = false; c->in_frame = false; c->pending = 0; drop_guides(c);
  ptc_lens_default_params(&c->lens);
  c->cam_ex_set = false; c->cam_ex = ptc_camera_params{};      // the extended camera goes with the camera
  c->lights.dirty = c->lights.dirty || !c->lights.list.empty(); c->lights.list.clear();
  c->alpha.mode.clear(); c->alpha.cutoff.clear(); c->alpha.dirty = true; c->alpha.n_prims = 0;      // every material of the next description starts OPAQUE; max_layers stays
  c->glass.params.clear(); c->glass.dirty = true; c->glass.n_prims = 0; c->glass.n_thin = 0;      // and without transmission; max_interactions and shadows stay
  c->medium.set = false; c->medium.params = ptc_medium_params{};      // the medium goes as the lights do
  c->emtex.mats.clear(); c->emtex.dirty = c->emtex.dirty || c->emtex.n_dev > 0; c->emtex.table.clear();      // and no material has an emission texture
  drop_history(c);        // the history is about the primitives of the scene that goes, and reads its shading records in place
  if (c->display.state.p) HIP_TRY(c, hipMemset(c->display.state.p, 0, sizeof(pt_display_state)));      // the adaptation state goes with the scene; the display parameters stay
  release_scene(c);
  return PTC_OK;
}

int ptc_add_material(ptc_ctx* c, const float base_color[4], float metallic, float roughness, const float emissive[3],
                     int tex_color, int tex_normal, int tex_mr) {
  if (!c) return PTC_E_ARG;
  if (!base_color || !emissive) return fail(c, PTC_E_ARG, "add_material: null pointer");
  const int nt = (int)c->texs.size();
  if (tex_color >= nt || tex_normal >= nt || tex_mr >= nt) return fail(c, PTC_E_ARG, "add_material: texture id out of range");
  HostMaterial m;
  std::memcpy(m.base, base_color, 16); m.metallic = metallic; m.roughness = roughness; std::memcpy(m.emissive, emissive, 12);
  m.tex_color = tex_color; m.tex_normal = tex_normal; m.tex_mr = tex_mr;
  c->mats.push_back(m);
  return (int)c->mats.size() - 1;
}

int ptc_add_texture_rgba8(ptc_ctx* c, const uint8_t* px, int w, int h) {
  if (!c) return PTC_E_ARG;
  if (!px || w <= 0 || h <= 0) return fail(c, PTC_E_ARG, "add_texture: bad argument");
  HostTexture t;
  t.px.assign(px, px + (size_t)w * h * 4); t.w = w; t.h = h;
  c->texs.push_back(std::move(t));
  return (int)c->texs.size() - 1;
}

int ptc_add_mesh(ptc_ctx* c, const ptc_vertex* verts, uint32_t n_verts, const uint32_t* indices, uint32_t n_indices, int material) {
  if (!c) return PTC_E_ARG;
  if (!verts || !indices || n_verts == 0 || n_indices == 0 || (n_indices % 3u)) return fail(c, PTC_E_ARG, "add_mesh: bad argument");
  if (material < 0 || material >= (int)c->mats.size()) return fail(c, PTC_E_ARG, "add_mesh: material out of range");
  for (uint32_t i = 0; i < n_indices; ++i) if (indices[i] >= n_verts) return fail(c, PTC_E_ARG, "add_mesh: index out of range");
  HostMesh m;
  m.v.resize(n_verts);
  static_assert(sizeof(HostVertex) == sizeof(ptc_vertex) && sizeof(ptc_vertex) == 48, "R1 vertex record is 48 bytes");
  std::memcpy(m.v.data(), verts, (size_t)n_verts * sizeof(ptc_vertex));
  m.idx.assign(indices, indices + n_indices);
  m.material = material;
  c->meshes.push_back(std::move(m));
  return (int)c->meshes.size() - 1;
}

int ptc_add_instance(ptc_ctx* c, int mesh, const float t[3], const float q_wxyz[4], const float s[3]) {
  if (!c) return PTC_E_ARG;
  if (!t || !q_wxyz || !s) return fail(c, PTC_E_ARG, "add_instance: null pointer");
  if (mesh < 0 || mesh >= (int)c->meshes.size()) return fail(c, PTC_E_ARG, "add_instance: mesh out of range");
  HostInstance in;
  in.mesh = mesh;
  ptc_trs_to_matrix(t, q_wxyz, s, in.m);
  c->insts.push_back(in);
  return (int)c->insts.size() - 1;
}

int ptc_add_instance_matrix(ptc_ctx* c, int mesh, const float model[16]) {
  if (!c) return PTC_E_ARG;
  if (!model) return fail(c, PTC_E_ARG, "add_instance_matrix: null pointer");
  if (mesh < 0 || mesh >= (int)c->meshes.size()) return fail(c, PTC_E_ARG, "add_instance_matrix: mesh out of range");
  HostInstance in;
  in.mesh = mesh;
  std::memcpy(in.m, model, 64);
  c->insts.push_back(in);
  return (int)c->insts.size() - 1;
}

int ptc_update_instance_matrix(ptc_ctx* c, int instance, const float model[16]) {
  if (!c) return PTC_E_ARG;
  if (!model) return fail(c, PTC_E_ARG, "update_instance_matrix: null pointer");
  if (instance < 0 || instance >= (int)c->insts.size()) return fail(c, PTC_E_ARG, "update_instance: instance out of range");
  std::memcpy(c->insts[(size_t)instance].m, model, 64);
  return PTC_OK;
}

int ptc_update_instance(ptc_ctx* c, int instance, const float t[3], const float q_wxyz[4], const float s[3]) {
  if (!c) return PTC_E_ARG;
  if (!t || !q_wxyz || !s) return fail(c, PTC_E_ARG, "update_instance: null pointer");
  if (instance < 0 || instance >= (int)c->insts.size()) return fail(c, PTC_E_ARG, "update_instance: instance out of range");
  ptc_trs_to_matrix(t, q_wxyz, s, c->insts[(size_t)instance].m);
  return PTC_OK;
}

// ---- deforming meshes: description (before the commit) and pose updates (any time); DESIGN.md §7a --------------------------------------
int ptc_mesh_set_morph_targets(ptc_ctx* c, int mesh, uint32_t n_targets, const float* dpos, const float* dnormal, const float* dtangent) {
  if (!c) return PTC_E_ARG;
  if (mesh < 0 || mesh >= (int)c->meshes.size()) return fail(c, PTC_E_ARG, "mesh_set_morph_targets: mesh out of range");
  if (n_targets > 0 && !dpos) return fail(c, PTC_E_ARG, "mesh_set_morph_targets: null pointer");
  if (n_targets > 65535u) return fail(c, PTC_E_ARG, "mesh_set_morph_targets: too many targets");
  if (c->committed) return fail(c, PTC_E_STATE, "mesh_set_morph_targets: the scene is committed (targets belong to the description: ptc_scene_begin)");
  MeshPose& P = *pose_make(c, mesh);
  auto D = std::make_shared<DeformMesh>(*P.data);
  const size_t n = (size_t)n_targets * D->n_verts * 3;
  D->n_targets = n_targets;
  D->dp.assign(dpos, dpos + (n_targets ? n : 0));
  if (dnormal && n_targets) D->dn.assign(dnormal, dnormal + n); else D->dn.clear();
  if (dtangent && n_targets) D->dt.assign(dtangent, dtangent + n); else D->dt.clear();
  P.data = D;
  P.w.assign(n_targets, 0.0f);      // the default pose
  pose_changed(P);
  return PTC_OK;
}

int ptc_mesh_set_skin(ptc_ctx* c, int mesh, uint32_t n_joints, const uint16_t* joints_u16x4, const float* weights_f32x4) {
  if (!c) return PTC_E_ARG;
  if (mesh < 0 || mesh >= (int)c->meshes.size()) return fail(c, PTC_E_ARG, "mesh_set_skin: mesh out of range");
  if (!joints_u16x4 || !weights_f32x4) return fail(c, PTC_E_ARG, "mesh_set_skin: null pointer");
  if (n_joints < 1u || n_joints > 65536u) return fail(c, PTC_E_ARG, "mesh_set_skin: n_joints out of range");
  if (c->committed) return fail(c, PTC_E_STATE, "mesh_set_skin: the scene is committed (a skin belongs to the description: ptc_scene_begin)");
  const size_t nv = c->meshes[(size_t)mesh].v.size();
  for (size_t i = 0; i < nv * 4; ++i) if (joints_u16x4[i] >= n_joints) return fail(c, PTC_E_ARG, "mesh_set_skin: joint index out of range");
  MeshPose& P = *pose_make(c, mesh);
  auto D = std::make_shared<DeformMesh>(*P.data);
  D->n_joints = n_joints;
  D->skin.resize(nv);
  for (size_t v = 0; v < nv; ++v)
    for (int k = 0; k < 4; ++k) { D->skin[v].j[k] = joints_u16x4[v * 4 + k]; D->skin[v].w[k] = weights_f32x4[v * 4 + k]; }
  P.data = D;
  P.J.assign((size_t)n_joints * 12, 0.0f);      // the default pose: identity matrices
  for (uint32_t j = 0; j < n_joints; ++j) P.J[(size_t)j * 12 + 0] = P.J[(size_t)j * 12 + 4] = P.J[(size_t)j * 12 + 8] = 1.0f;
  pose_changed(P);
  return PTC_OK;
}

int ptc_update_mesh_pose(ptc_ctx* c, int mesh, const float* morph_weights, uint32_t n_weights, const float* joint_matrices, uint32_t n_joints) {
  if (!c) return PTC_E_ARG;
  if (mesh < 0 || mesh >= (int)c->meshes.size()) return fail(c, PTC_E_ARG, "update_mesh_pose: mesh out of range");
  const MeshPose* Q = (size_t)mesh < c->poses.size() && c->poses[(size_t)mesh].active() ? &c->poses[(size_t)mesh] : nullptr;
  const uint32_t T = Q ? Q->data->n_targets : 0u, nj = Q && !Q->data->skin.empty() ? Q->data->n_joints : 0u;
  if (morph_weights && n_weights != T) return fail(c, PTC_E_ARG, "update_mesh_pose: the number of weights is not the mesh's number of morph targets");
  if (joint_matrices && n_joints != nj) return fail(c, PTC_E_ARG, "update_mesh_pose: the number of matrices is not the mesh's number of joints");
  if (!Q) return PTC_OK;
  MeshPose& P = c->poses[(size_t)mesh];
  if (morph_weights && T) P.w.assign(morph_weights, morph_weights + T);
  if (joint_matrices && nj) P.J.assign(joint_matrices, joint_matrices + (size_t)nj * 12);
  if ((morph_weights && T) || (joint_matrices && nj)) pose_changed(P);
  return PTC_OK;
}

int ptc_update_mesh_vertices(ptc_ctx* c, int mesh, const ptc_vertex* verts, uint32_t n_verts) {
  if (!c) return PTC_E_ARG;
  if (mesh < 0 || mesh >= (int)c->meshes.size()) return fail(c, PTC_E_ARG, "update_mesh_vertices: mesh out of range");
  if (!verts) return fail(c, PTC_E_ARG, "update_mesh_vertices: null pointer");
  if (n_verts != c->meshes[(size_t)mesh].v.size()) return fail(c, PTC_E_ARG, "update_mesh_vertices: the number of vertices is not the mesh's");
  MeshPose& P = *pose_make(c, mesh);
  auto base = std::make_shared<std::vector<HostVertex>>(n_verts);
  std::memcpy(base->data(), verts, (size_t)n_verts * sizeof(ptc_vertex));
  P.base = base;
  pose_changed(P);
  return PTC_OK;
}

int ptc_scene_refit(ptc_ctx* c) {
  if (!c) return PTC_E_ARG;
  if (!c->committed) return fail(c, PTC_E_STATE, "scene_refit: scene not committed");
  if (!description_matches_commit(c)) return fail(c, PTC_E_STATE, kDescriptionChanged);
  if (c->device >= 0) {
    HIP_TRY(c, hipSetDevice(c->device));
    { int rf = flush(c); if (rf) return rf; }
    { int rt = temporal_keep_positions(c); if (rt) return rt; }
    { int rs = sync_all_lanes(c); if (rs) return rs; }
  }
  const auto t0 = std::chrono::steady_clock::now();
  if (c->built.use_count() > 1) c->built = std::make_shared<HostBuilt>(*c->built);      // a group shares one build: this context now gets its own
  if (c->device >= 0 && refit_on_device(c)) {
    const int rd = device_refit(c, t0);
    if (rd == 0) emtex_place(c);
    if (rd <= 0) return rd;
  }
  if (!c->built->topology) return host_build_and_upload(c, t0, /*as_refit=*/true);      // the tree in HBM was built on the device (ptc_scene_rebuild): the host has no topology to refit
  HostBuilt& B = *c->built;
  const size_t n_recs = B.recs.size(), n_shade = B.shade.size(), n_lights = B.lights.size(), n_cdf = B.cdf.size();
  deform_host_all(c);
  const std::string e = ptc_refit_scene(c->mats, c->meshes, c->insts, c->texs, c->env, B);
  if (!e.empty()) return fail(c, PTC_E_STATE, e);
  c->in_frame = false; c->pending = 0; drop_guides(c);
  c->stats.n_emitters = B.n_lights;
  c->stats.bvh_sa_cost = (double)B.sa_cost_fixed / (double)PTC_SA_COST_ONE;
  if (c->device >= 0) {
    int rc = refit_upload(c, B.recs.size() == n_recs && B.shade.size() == n_shade && B.lights.size() == n_lights && B.cdf.size() == n_cdf, t0);
    if (rc) return rc;
  }
  { int rc = deform_after_host_refit(c); if (rc) return rc; }
  emtex_place(c);
  c->stats.seconds_refit = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  return PTC_OK;
}

int ptc_scene_rebuild(ptc_ctx* c) {
  { int rd = need_device(c); if (rd) return rd; }
  if (!c->committed) return fail(c, PTC_E_STATE, "scene_rebuild: scene not committed");
  if (!description_matches_commit(c)) return fail(c, PTC_E_STATE, kDescriptionChanged);
  { int rf = flush(c); if (rf) return rf; }
  { int rt = temporal_keep_positions(c); if (rt) return rt; }
  { int rs = sync_all_lanes(c); if (rs) return rs; }
  const auto t0 = std::chrono::steady_clock::now();
  if (c->built.use_count() > 1) c->built = std::make_shared<HostBuilt>(*c->built);      // a group shares one build: this context now gets its own
  const char* how = std::getenv("PTC_REBUILD");
  int rd = (how && std::strcmp(how, "host") == 0) ? 1 : device_rebuild(c, c->device_builder);
  if (rd < 0) return rd;
  if (rd > 0) { if ((rd = host_build_and_upload(c, t0, /*as_refit=*/false))) return rd; }      // PTC_REBUILD=host, an emitter appeared or vanished, a single triangle
  else { emtex_place(c); c->stats.seconds_rebuild = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(); }
  c->in_frame = false; c->pending = 0; drop_guides(c);
  return PTC_OK;
}

int ptc_set_camera(ptc_ctx* c, const float pos[3], const float target[3], float fov_y, float aspect) {
  if (!c) return PTC_E_ARG;
  if (!pos || !target) return fail(c, PTC_E_ARG, "set_camera: null pointer");
  std::memcpy(c->cam_pos, pos, 12); std::memcpy(c->cam_target, target, 12); c->cam_fov = fov_y; c->cam_aspect = aspect;
  c->have_cam = true;
  c->cam_ex_set = false; c->cam_ex = ptc_camera_params{};      // ptc_set_camera and ptc_set_camera_ex replace one another
  c->guides.valid = false;      // the guides are those of the camera they were traced from
  if (c->committed) ptc_make_camera(c->cam_pos, c->cam_target, c->cam_fov, c->cam_aspect, c->cam);
  return PTC_OK;
}

// ---- thin-lens camera (pt_lens.h) ---------------------------------------------------------------------------------------------------------
void ptc_lens_default_params(ptc_lens_params* p) {
  if (!p) return;
  p->aperture_radius = 0.0f; p->focus_distance = 1.0f; p->blades = 0; p->rotation = 0.0f;
}

int ptc_set_camera_lens(ptc_ctx* c, const ptc_lens_params* params) {
  if (!c) return PTC_E_ARG;
  const ptc_lens_params p = with_defaults(params, ptc_lens_default_params);
  if (const char* e = lens_params_error(p)) return fail(c, PTC_E_ARG, std::string("set_camera_lens: ") + e);
  c->lens = p;      // the guides are traced through the lens centre: they stay valid
  return PTC_OK;
}

int ptc_get_camera_lens(const ptc_ctx* c, ptc_lens_params* out) {
  if (!c || !out) return PTC_E_ARG;
  *out = c->lens;
  return PTC_OK;
}

// ---- punctual lights (pt_lights.h) ----------------------------------------------------------------------------------------------------------
void ptc_light_default_params(ptc_light_params* p) {
  if (!p) return;
  std::memset(p, 0, sizeof *p);
  p->type = PTC_LIGHT_POINT;
  p->direction[2] = -1.0f;
  p->intensity[0] = p->intensity[1] = p->intensity[2] = 1.0f;
  p->cos_inner = 1.0f; p->cos_outer = 0.70710678f;      // glTF's default cone: inner 0, outer pi / 4
  p->sampling_weight = 1.0f;
}

int ptc_add_light(ptc_ctx* c, const ptc_light_params* params) {
  if (!c) return PTC_E_ARG;
  if (!params) return fail(c, PTC_E_ARG, "add_light: null pointer");
  if (const char* e = pt_light_params_error(*params)) return fail(c, PTC_E_ARG, std::string("add_light: ") + e);
  if (c->lights.list.size() >= PTC_MAX_LIGHTS) return fail(c, PTC_E_ARG, "add_light: more than PTC_MAX_LIGHTS lights");
  ptc_light_params p = *params;
  pt_light_normalise(p);
  c->lights.list.push_back(p);
  c->lights.dirty = true;
  return (int)c->lights.list.size() - 1;
}

int ptc_update_light(ptc_ctx* c, int id, const ptc_light_params* params) {
  if (!c) return PTC_E_ARG;
  if (!params || id < 0 || (size_t)id >= c->lights.list.size()) return fail(c, PTC_E_ARG, "update_light: null pointer or light id out of range");
  if (const char* e = pt_light_params_error(*params)) return fail(c, PTC_E_ARG, std::string("update_light: ") + e);
  ptc_light_params p = *params;
  pt_light_normalise(p);
  c->lights.list[(size_t)id] = p;
  c->lights.dirty = true;
  return PTC_OK;
}

int ptc_get_light(const ptc_ctx* c, int id, ptc_light_params* out) {
  if (!c || !out || id < 0 || (size_t)id >= c->lights.list.size()) return PTC_E_ARG;
  *out = c->lights.list[(size_t)id];
  return PTC_OK;
}

int ptc_light_count(const ptc_ctx* c) { return c ? (int)c->lights.list.size() : PTC_E_ARG; }

int ptc_clear_lights(ptc_ctx* c) {
  if (!c) return PTC_E_ARG;
  if (!c->lights.list.empty()) { c->lights.list.clear(); c->lights.dirty = true; }
  return PTC_OK;
}

int ptc_set_texture_filter(ptc_ctx* c, int filter) {
  if (!c) return PTC_E_ARG;
  if (filter != PTC_FILTER_NEAREST && filter != PTC_FILTER_LINEAR) return fail(c, PTC_E_ARG, "set_texture_filter: unknown filter");
  c->tex_linear = filter;
  return PTC_OK;
}

int ptc_set_bvh_builder(ptc_ctx* c, int builder) {
  if (!c) return PTC_E_ARG;
  if (builder != PTC_BVH_SAH && builder != PTC_BVH_LBVH) return fail(c, PTC_E_ARG, "set_bvh_builder: unknown builder");
  c->bvh_builder = builder;
  return PTC_OK;
}

int ptc_set_device_builder(ptc_ctx* c, int builder) {
  if (!c) return PTC_E_ARG;
  if (builder != PTC_BVH_SAH && builder != PTC_BVH_LBVH) return fail(c, PTC_E_ARG, "set_device_builder: unknown builder");
  c->device_builder = builder;
  return PTC_OK;
}

int ptc_set_env_latlong_rgb32f(ptc_ctx* c, const float* rgb, int w, int h) {
  if (!c) return PTC_E_ARG;
  if (!rgb) { c->env = HostEnv{}; return PTC_OK; }
  if (w <= 0 || h <= 0 || w > 65536 || h > 65536 || (uint64_t)w * (uint64_t)h > (1u << 28)) return fail(c, PTC_E_ARG, "set_env: bad size");
  c->env.rgb.assign(rgb, rgb + (size_t)w * h * 3); c->env.w = w; c->env.h = h;
  return PTC_OK;
}

int ptc_scene_commit(ptc_ctx* c) { return scene_commit(c, true); }
}  // extern "C"

