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
#include "../../include/ptc.h"
#include "ptc_internal.h"
#include "pt_refit.h"
#include "pt_build.h"
#include "pt_denoise.h"
#include "pt_adaptive.h"
#include "pt_temporal.h"
#include "pt_deform.h"
#include "pt_lens.h"
#include "pt_lights.h"
#include "pt_display.h"
#include "pt_probes.h"

#include <dlfcn.h>
#include <rccl/rccl.h>

#include <chrono>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <memory>
#include <string>
#include <vector>

#define PTC_STR2(x) #x
#define PTC_STR(x) PTC_STR2(x)
namespace {
std::string g_create_error;

struct Span { hipEvent_t a, b; int kind; };   // kind: 0 trace_closest, 1 trace_any, 2 shade, 3 whole batch, 4 the RCCL reduce

template <class T> struct DevBuf {
  T* p = nullptr; size_t n = 0;
  void release() { if (p) (void)hipFree(p); p = nullptr; n = 0; }
};

// One lane: a stream with its own wavefront queues.  cnt/stats are allocated once; the large arrays grow on demand.
struct Lane {
  hipStream_t stream = nullptr;
  DevQueues q{};
  std::vector<void*> allocs;        // the large queue arrays (sized q.cap)
  uint2* stack_ovf = nullptr;       // traversal-stack overflow slab of the committed scene (ensure_overflow_slabs; freed by release_scene)
  DevScene* d_scene = nullptr;      // this lane's DevScene in device memory (k_shade reads it through a pointer instead of ~200 B of kernel arguments)
  hipEvent_t acc_done = nullptr;    // "this lane's last accumulate finished"
  // PTC_TRACE_OVERLAP=1: the shadow rays of bounce b are traced on a second stream beside the closest-hit launch of bounce b + 1
  hipStream_t stream2 = nullptr;
  uint2* stack_ovf2 = nullptr;      // the any-hit launches' own overflow slab (concurrent kernels must not share one)
  std::vector<hipEvent_t> ev_scan, ev_any;
  void free_overflow_slabs() { for (uint2* p : {stack_ovf, stack_ovf2}) if (p) (void)hipFree(p); stack_ovf = stack_ovf2 = nullptr; }
};

// The arrays of a tree in HBM: unit array, the refit's level list, the per-record node boxes, with their capacities (a rebuild writes into arrays large enough)
struct TreeBufs {
  float4* recs = nullptr; size_t recs_cap = 0; uint32_t* levels = nullptr; size_t levels_cap = 0; float* nbox = nullptr; size_t nbox_cap = 0;
  void release() { for (void* p : {(void*)recs, (void*)levels, (void*)nbox}) if (p) (void)hipFree(p); *this = TreeBufs(); }
};

// The committed scene on the device and what the refit, the rebuild and the commit on the device keep of it.  release_scene frees all of it.
struct CommittedScene {
  DevScene dsc{};
  std::vector<void*> allocs;        // every array of dsc and drf but the tree's
  size_t insts = 0;                 // instances the committed scene was built from (ptc_scene_refit refuses a description that has grown since)
  // refit on the device (pt_refit.h): the plan is built and uploaded by the first ptc_scene_refit after a commit
  RefitPlan plan;
  DevRefit drf{};
  bool refit_ready = false;
  bool host_stale = false;          // the device refitted in place: built's vertex-dependent arrays are those of an earlier state until refresh_host_copy
  TreeBufs live, spare;             // the tree in use; a rebuild writes the new tree into the spare set and the arrays it replaces become the spare: no
                                    // allocation in a viewer's steady state
  std::vector<float> xf_live;       // instance transforms of the last refit the device completed (a refused one re-flattens its scratch vertices from these)
  // how the last calls went (ptc_debug_get_internals); release_scene keeps them
  bool last_refit_on_device = false;
  bool commit_on_device = false;      // the last ptc_scene_commit flattened and built on the device (device_commit)
  bool tree_device_sah = false;       // the tree in HBM was built on the device by the SAH front end (pt_build_sah)
  // deforming meshes (pt_deform.h): what ensure_refit_plan puts into HBM for every mesh with deformation state, by mesh index (n_verts = 0: none)
  std::vector<DevDeform> deform;
  std::vector<std::vector<float>> pose_stage;   // host side of the pose uploads in flight (alive until the pass that queued them has synchronised)
  std::vector<uint32_t> mesh_first;   // first vertex of every mesh in the object-space vertex array
  HostVertex* mesh_verts_rw = nullptr;   // drf.mesh_verts is const for the flatten: the deform kernel writes through this alias
};

// Deformation state of one mesh of the description (index = mesh id; a mesh that never saw one of the new calls has none: base == nullptr).
// c->meshes[m].v holds the POSED vertices — that is what every host path reads — and is brought up to date lazily (deform_host_all / deform_host_emissive).
// The pending pose is what the update calls recorded; the live pose is the one the mesh's slice in HBM was evaluated from (a refused refit re-evaluates from it,
// as xf_live keeps the live transforms).  Vertex arrays and the fixed data are shared: the contexts of a group take context 0's.
struct MeshPose {
  std::shared_ptr<DeformMesh> data;
  std::shared_ptr<std::vector<HostVertex>> base;        // base vertices as described (ptc_update_mesh_vertices replaces the vector)
  std::vector<float> w, J;                              // pending: morph weights, joint matrices (12 floats each)
  std::vector<float> pose_live;                         // live: weights then matrices
  std::shared_ptr<std::vector<HostVertex>> base_live;   // live base
  const void* base_on_device = nullptr;                 // identity of the vector DevDeform::base was uploaded from
  bool host_fresh = false;      // meshes[m].v is the pending pose, every vertex
  bool emis_fresh = false;      // ... at least the vertices of emissive primitives
  bool dev_fresh = false;       // the slice in HBM is the pending pose (live == pending)
  bool on_device = false;       // the slice in HBM was written by the kernel (ptc_debug_get_mesh_vertices reads it from there)
  bool active() const { return base != nullptr; }
  std::vector<float> pose() const { std::vector<float> p(w); p.insert(p.end(), J.begin(), J.end()); return p; }
};

// ---- RCCL, loaded on first use (a renderer that never reduces does not need librccl at load time) -------------------
struct Rccl {
  void* so = nullptr;
  ncclResult_t (*GetUniqueId)(ncclUniqueId*) = nullptr;
  ncclResult_t (*CommInitRank)(ncclComm_t*, int, ncclUniqueId, int) = nullptr;
  ncclResult_t (*CommInitAll)(ncclComm_t*, int, const int*) = nullptr;
  ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
  ncclResult_t (*Reduce)(const void*, void*, size_t, ncclDataType_t, ncclRedOp_t, int, ncclComm_t, hipStream_t) = nullptr;
  ncclResult_t (*GroupStart)() = nullptr;
  ncclResult_t (*GroupEnd)() = nullptr;
  const char* (*GetErrorString)(ncclResult_t) = nullptr;
  std::string err;
};
Rccl g_rccl;
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

struct ptc_ctx {
  int device = 0;
  std::string err;
  LaunchCfg cfg{};
  uint32_t toplet_budget = 73;   // 64-byte records staged in LDS: the top three levels (1+8+64 nodes) of the tree = 4.6 KB
  size_t max_batch_paths = (size_t)7 << 27;   // paths in flight over all lanes (939,524,096).  Large batches amortise what a launch costs regardless of its size
                                              // (drain of the persistent waves, small late-bounce launches): round 2 measured 2^29 1.5 % faster than 2^28, 2^27 3 % and
                                              // 2^25 24 % slower; round 4 7 x 2^27 another 0.8 % faster than 2^29 (profiles/r04_trace_variants.txt).  176 B per path = 165 GB of
                                              // queues when a 1080p frame is rendered at >= 453 spp — sized for 288 GB of HBM; frame_begin lowers it to what 60 % of the free memory holds.
  int timing = 1;                     // PTC_TIMING: 0 no events at all; 1 (default) a span per batch, and a span per kernel where the kernels of a batch run one after the other
                                      // (a small batch runs its trace kernels beside each other: their spans would include each other, and 54 event records are 0.2 ms of a 3-ms frame); 2 a span per kernel always
  // description
  std::vector<HostMaterial> mats;
  std::vector<HostMesh> meshes;
  std::vector<HostInstance> insts;
  std::vector<HostTexture> texs;
  HostEnv env;
  float cam_pos[3]{}, cam_target[3]{}, cam_fov = 0, cam_aspect = 1;
  bool have_cam = false;
  ptc_lens_params lens{0.0f, 1.0f, 0, 0.0f};   // the camera's lens (ptc_set_camera_lens): kept across ptc_set_camera, reset by ptc_scene_begin; R = 0: the pinhole, k_raygen
  // punctual lights (pt_lights.h): `lights` is what the calls recorded; the device table is what the last ptc_frame_begin uploaded of it, and what the frame's batches use
  std::vector<ptc_light_params> lights;
  bool lights_dirty = false;             // `lights` changed since the upload
  DevBuf<pt_light_rec> d_lights;
  DevBuf<float> d_light_cdf;
  uint32_t n_lights_dev = 0;             // lights in the device table; 0: no punctual pass, nothing allocated
  // display transform (pt_display.h): the parameters are a context setting; the histogram (4096 bins + the rejected count) and the state record live in HBM,
  // allocated by the first call that needs them.  Nothing here is touched by a context that never calls the display functions
  ptc_display_params display{1.0f, 0, 0.18f, 0.1f, 0.9f, 1.0f, 1e-4f, 1e6f, PTC_TONEMAP_ACES, 4.0f, PTC_OETF_GAMMA22};
  DevBuf<uint32_t> dp_hist, dp_ldr;
  DevBuf<pt_display_state> dp_state;
  DevBuf<uint2> dp_half;
  hipEvent_t ev_dp[4] = {nullptr, nullptr, nullptr, nullptr};   // start / stop of the last metering, start / stop of the last display kernel
  bool ev_dp_recorded[2] = {false, false};
  int tex_linear = 0;                    // PTC_FILTER_*: texture filter of the scene being described
  int bvh_default = PTC_BVH_SAH;         // PTC_BVH_*: builder a new scene description starts with (PTC_BVH=lbvh in the environment changes it)
  int bvh_builder = PTC_BVH_SAH;         // builder of the scene being described
  int device_builder = PTC_BVH_LBVH;     // PTC_BVH_*: the tree a build ON THE DEVICE makes (ptc_set_device_builder; PTC_DEVICE_BVH=sah in the environment), kept across ptc_scene_begin
  // committed scene
  bool committed = false;
  std::shared_ptr<HostBuilt> built = std::make_shared<HostBuilt>();   // the host build; the contexts of a ptc_group share one (ptc_group_scene_commit)
  CommittedScene scene;
  std::vector<MeshPose> poses;      // deformation state by mesh id (may be shorter than meshes: plain meshes at the end have none)
  DevCamera cam{};
  bool debug_verts_from_device = false;      // the last ptc_debug_get_mesh_vertices read the mesh's slice in HBM (ptc_debug_get_internals[7] bit 3)
  int refit_on_device = 1;          // PTC_REFIT=host: ptc_scene_refit recomputes on the host and uploads (the round-3a path, kept as the cross-check)
  int trace_rays_per_lane = 8;      // PTC_TRACE_RAYS_PER_LANE: rays per lane of the trace kernels' grid a batch should offer before the grid is made smaller (run_batch)
  int trace_overlap = 1;            // PTC_TRACE_OVERLAP: the shadow rays of bounce b are traced on the lane's second stream beside the closest-hit launch of bounce b + 1 (they are
                                    // independent; k_shade(b + 1) waits for both).  1 (default) = batches of up to 2^26 paths, whose launches do not keep the chip full for long:
                                    // -5 % .. -17 % frame time from 16 spp down to 1 spp at 1080p (profiles/r03_viewer_loop.txt); 2 = every batch (+0.4 % at the benchmark's
                                    // batch size, but the two kernels' launch durations then include each other: not the default, so that what bench.py and rocprofv3 time
                                    // per kernel stays a kernel's own time); 0 = never
  BuildScratch bscratch;            // device scratch of ptc_scene_rebuild (pt_build.hip), grow-only
  // lanes: lane 0 is the context's primary stream (resolve, tonemap, conversions, the reduce)
  std::vector<Lane> lanes;
  int n_lanes = 1;                  // PTC_LANES: >1 runs successive batches on separate streams.  With the round-2 kernels one lane
                                    // is 3.7 % faster than two (co-scheduled launches slow each other down by more than the tails they fill)
  uint64_t batches_issued = 0;
  // frame
  bool in_frame = false;
  DevFrame fr{};
  int spp_total = 0, integrator = 0;
  uint32_t samples_done = 0;        // samples issued to the device
  uint32_t sample_base = 0;         // index of the frame's first sample (ptc_frame_set_sample_range / ptc_frame_restore): sample k of the frame has index sample_base + k
  uint32_t resolve_divisor = 0;     // 0: the resolve divides by the samples accumulated; else by this (sample-range sharding: partial means that sum to the mean)
  uint32_t pending = 0;             // samples accepted by frame_add_samples and not yet issued (deferred batching)
  uint32_t per_batch = 1;           // samples of one full batch = max_batch_paths / owned pixels / lanes
  DevBuf<uint32_t> owned;
  bool owned_key_valid = false;     // c->owned holds the list for (owned_w, owned_h, owned_rank, owned_count)
  int owned_w = 0, owned_h = 0, owned_rank = 0, owned_count = 0;
  uint32_t owned_n = 0;
  DevBuf<float4> accum, radiance;
  DevBuf<uint32_t> ldr;
  DevBuf<uint2> half;               // RGBA16F copy of the radiance buffer
  int rad_w = 0, rad_h = 0;
  // denoiser: the first-hit guides of the current frame (k_guides), the filter's two (colour, variance) buffers, the denoised image and which image the read-backs serve
  DevBuf<float4> g_albedo, g_normal, g_pos, dn_cv[2], denoised;
  DevBuf<int32_t> g_prim;
  DevBuf<float2> g_uv;
  DevBuf<unsigned long long> g_stats;   // the guide rays' traversal counters: kept apart from the frame's (ptc_stats counts samples only)
  bool guides_valid = false, denoised_valid = false;
  int output = PTC_OUTPUT_RADIANCE;
  hipEvent_t ev_dn[4] = {nullptr, nullptr, nullptr, nullptr};   // start / stop of the last guide pass, start / stop of the last denoise
  bool ev_dn_recorded[2] = {false, false};
  // adaptive sampling (pt_adaptive.hip).  In an adaptive frame `fr` describes the ACTIVE pixels (n_owned = their number, owned = ad_pix[ad_cur]): that is all the
  // path kernels see of a frame; the frame's own pixels stay in owned / owned_n, where the sums, the moments and the counts live.
  bool adaptive = false;
  ptc_adaptive_params ad_params{};
  DevBuf<uint32_t> ad_pix[2], ad_slot[2], ad_count, ad_block, ad_n;   // the active list (pixel, owned position), ping-pong: a decision step compacts one into the other
  DevBuf<float2> ad_mom;
  DevBuf<uint8_t> ad_flags, ad_keep;
  int ad_cur = 0;
  uint32_t ad_passes = 0;
  double ad_seconds = 0.0;
  hipEvent_t ev_ad[2] = {nullptr, nullptr};
  // the per-sample RGB covariance: cov_setting is the context's (ptc_set_sample_covariance), cov_on what the current adaptive frame was begun with
  bool cov_setting = false, cov_on = false;
  bool cov_resolved = false;        // the radiance buffer holds the resolve of every sample the frame's sums hold
  bool sv_valid = false;            // sv_var holds the current frame's last ptc_denoise_sampled variance
  DevBuf<float4> ad_cov4, sv_colour, sv_var;   // (rr, gg, bb, rg) per owned pixel; the filter's input (D, n) and (0, 0, Var_s, 1 / n) per pixel
  DevBuf<float2> ad_cov2;                      // (rb, gb) per owned pixel
  size_t frame_batch_paths = 0;     // the path budget of a batch as ptc_frame_begin settled it: per_batch follows the active set from it
  // temporal accumulation (pt_temporal.hip).  The history is the state the last ptc_temporal_accumulate left: set tp_cur of the two ping-pong sets, the camera and
  // the size of its frame.  It outlives frames, cameras, refits and rebuilds; the accumulated image is the current frame's (drop_guides ends its validity).
  DevBuf<float4> tp_dn[2], tp_mom[2], tp_nz[2], tp_pk[2], tp_motion, tp_accum;
  DevBuf<float4> tp_snap;           // the position snapshot: 3 x float4 per primitive as the shading records held them when the history was written
  bool tp_snap_current = false;     // false: the shading records in HBM still are those of the history's frame (nothing moved since), the snapshot is not needed;
                                    // true: a refit or rebuild came after the history, tp_snap holds the positions it was about to overwrite
  bool tp_live = false;             // there is a history
  int tp_cur = 0, tp_w = 0, tp_h = 0, tp_demodulate = 0;
  DevCamera tp_cam{};
  bool tp_accum_valid = false;      // the current frame has been accumulated: tp_accum holds its accumulated image
  hipEvent_t ev_tp[2] = {nullptr, nullptr};
  bool ev_tp_recorded = false;
  // light probes (pt_probes.h).  A probe frame is a frame of n x 1 "pixels" — `fr`, accum, radiance, the batching and the sample range are the frame's own — whose
  // batches start at k_raygen_probe and end with k_accumulate_sh beside k_accumulate.  The flag lives as long as the frame does (drop_guides ends it).
  bool probe = false;
  uint32_t probe_base = 0;          // index of probe 0 in the RNG key (ptc_probes_begin: probe_index_base)
  DevBuf<float4> probe_pos;         // (x, y, z, -) per probe
  DevBuf<float> probe_acc;          // 27 running sums per probe, [probe][k][rgb]
  // multi-GPU
  ncclComm_t comm = nullptr;
  int comm_rank = 0, comm_size = 0;
  bool comm_owned = true;           // false: the communicator belongs to a ptc_group
  // stats
  ptc_stats stats{};
  std::vector<Span> spans;
  std::vector<hipEvent_t> free_events;
  size_t events_created = 0;
};

struct ptc_group {
  std::vector<ptc_ctx*> ctx;
  std::vector<ncclComm_t> comms;
  std::string err;
};

namespace {

constexpr size_t kQueueBytesPerPath = 176;   // ensure_lane_queues: 2 x 48 (ray ping-pong) + 48 (shadow) + 16 (hit) + 16 (path radiance)
constexpr size_t kMaxSpans = 1024;   // timing spans (event pairs) kept at most; see run_batch
int fail(ptc_ctx* c, int code, const std::string& msg) { if (c) c->err = msg; return code; }
// the frame is over or the scene changed: its guides and its denoised image go with it, the read-backs serve the radiance again
// the temporal history is about the primitive ids of one committed scene: whatever brings another scene (ptc_scene_begin; every kind of commit, through
// commit_upload(Upload::NewScene)) ends it, and with it the position snapshot's claim to be current.  Refits and rebuilds keep the ids and the history.
void drop_history(ptc_ctx* c) { c->tp_live = false; c->tp_snap_current = false; }
void drop_guides(ptc_ctx* c) { c->probe = false; c->guides_valid = false; c->denoised_valid = false; c->tp_accum_valid = false; c->output = PTC_OUTPUT_RADIANCE; }
// the image ptc_read_radiance_rgba32f / _rgba16f / ptc_tonemap_rgba8 serve (ptc_select_output)
const float4* served_image(const ptc_ctx* c) { return c->output == PTC_OUTPUT_DENOISED ? c->denoised.p : c->output == PTC_OUTPUT_ACCUMULATED ? c->tp_accum.p : c->radiance.p; }
const char* const kNoDevice = "this context has no device (PTC_DEVICE_NONE): the call needs a gfx950 GPU; there is no CPU path";

#define HIP_TRY(c, expr)                                                                                 \
  do {                                                                                                   \
    hipError_t e_ = (expr);                                                                              \
    if (e_ != hipSuccess)                                                                                \
      return fail((c), e_ == hipErrorOutOfMemory ? PTC_E_NOMEM : PTC_E_DEVICE, std::string(#expr) + ": " + hipGetErrorString(e_)); \
  } while (0)
#define NCCL_TRY(c, expr)                                                                                \
  do {                                                                                                   \
    ncclResult_t r_ = (expr);                                                                            \
    if (r_ != ncclSuccess) return fail((c), PTC_E_DEVICE, std::string(#expr) + ": " + g_rccl.GetErrorString(r_)); \
  } while (0)

template <class T> int dev_alloc(ptc_ctx* c, std::vector<void*>& owner, T** out, size_t count) {
  void* p = nullptr;
  HIP_TRY(c, hipMalloc(&p, (count ? count : 1) * sizeof(T)));
  owner.push_back(p);
  *out = (T*)p;
  return PTC_OK;
}
template <class T> int dev_upload(ptc_ctx* c, std::vector<void*>& owner, const T** out, const std::vector<T>& v) {
  T* p = nullptr;
  int rc = dev_alloc(c, owner, &p, v.size());
  if (rc) return rc;
  if (!v.empty()) HIP_TRY(c, hipMemcpy(p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
  *out = p;
  return PTC_OK;
}
void free_all(std::vector<void*>& v) { for (void* p : v) (void)hipFree(p); v.clear(); }
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

template <class T> int ensure_buf(ptc_ctx* c, DevBuf<T>& b, size_t n) {
  if (b.n >= n && b.p) return PTC_OK;
  b.release();
  HIP_TRY(c, hipMalloc((void**)&b.p, (n ? n : 1) * sizeof(T)));
  b.n = n;
  return PTC_OK;
}

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
      else c->stats.seconds_render += sec;
    }
    c->free_events.push_back(s.a); c->free_events.push_back(s.b);
  }
  c->spans.resize(keep);
}
struct ScopedSpan {   // records a start/stop event pair around launches on one of the context's streams
  ptc_ctx* c; hipStream_t st; Span s{}; bool on;
  ScopedSpan(ptc_ctx* c_, hipStream_t st_, int kind, bool enable = true) : c(c_), st(st_), on(c_->timing != 0 && enable) {
    if (!on) return;
    s.kind = kind; s.a = next_event(c); s.b = next_event(c);
    if (!s.a || !s.b) { if (s.a) c->free_events.push_back(s.a); on = false; return; }
    (void)hipEventRecord(s.a, st);
  }
  ~ScopedSpan() { if (on) { (void)hipEventRecord(s.b, st); c->spans.push_back(s); } }
};

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

DevScene lane_scene(ptc_ctx* c, int l) { DevScene d = c->scene.dsc; d.stack_ovf = c->lanes[(size_t)l].stack_ovf; return d; }
// Every lane's copy of the scene (k_shade reads it through a pointer), enqueued on `st`: the caller synchronises
int publish_lane_scenes(ptc_ctx* c, hipStream_t st) {
  for (int l = 0; l < c->n_lanes; ++l) {
    const DevScene ds = lane_scene(c, l);
    HIP_TRY(c, hipMemcpyAsync(c->lanes[(size_t)l].d_scene, &ds, sizeof ds, hipMemcpyHostToDevice, st));
  }
  return PTC_OK;
}
// the lane's queues with the segment layout of a batch of n slots (ptc_internal.h, "SEGMENTED queues")
DevQueues batch_queues(ptc_ctx* c, int l, uint32_t n) {
  DevQueues q = c->lanes[(size_t)l].q;
  ptc_seg_layout(n, (uint32_t)c->cfg.shade_waves, q.n_seg, q.seg_len);
  return q;
}
bool is_raster(int integrator) { return integrator == PTC_INTEGRATOR_RASTER_COMPAT || integrator == PTC_INTEGRATOR_RASTER_GBUFFER16; }

// the launch configuration of a batch of n_paths rays: the trace kernels' persistent grid follows the batch (see run_batch)
LaunchCfg batch_cfg(const ptc_ctx* c, uint32_t n_paths) {
  LaunchCfg cfg = c->cfg;
  const uint64_t per_block = (uint64_t)pt_trace_block_threads() * (uint64_t)c->trace_rays_per_lane;
  uint64_t per_cu = ((uint64_t)n_paths + per_block * (uint64_t)cfg.n_cu - 1u) / (per_block * (uint64_t)cfg.n_cu);
  if (per_cu < 1) per_cu = 1;
  if (per_cu < (uint64_t)cfg.trace_blocks_per_cu) cfg.trace_blocks_per_cu = (int)per_cu;
  return cfg;
}

DevAdaptive dev_adaptive(const ptc_ctx* c) {
  return DevAdaptive{c->ad_mom.p, c->ad_count.p, c->ad_flags.p, c->ad_keep.p, c->ad_block.p, c->ad_n.p, c->cov_on ? c->ad_cov4.p : nullptr, c->cov_on ? c->ad_cov2.p : nullptr};
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

// The punctual lights' table as recorded -> device memory, when it changed (ptc_frame_begin, ptc_debug_punctual_nee: every lane is idle).  No light: nothing is allocated.
int upload_lights(ptc_ctx* c) {
  if (!c->lights_dirty) return PTC_OK;
  std::vector<pt_light_rec> recs; std::vector<float> cdf;
  pt_light_table(c->lights, recs, cdf);
  if (!recs.empty()) {
    int rc = ensure_buf(c, c->d_lights, recs.size());
    if (!rc) rc = ensure_buf(c, c->d_light_cdf, cdf.size());
    if (rc) return rc;
    HIP_TRY(c, hipMemcpy(c->d_lights.p, recs.data(), recs.size() * sizeof(pt_light_rec), hipMemcpyHostToDevice));
    HIP_TRY(c, hipMemcpy(c->d_light_cdf.p, cdf.data(), cdf.size() * sizeof(float), hipMemcpyHostToDevice));
  }
  c->n_lights_dev = (uint32_t)recs.size();
  c->lights_dirty = false;
  return PTC_OK;
}

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
    if (c->probe) pt_launch_raygen_probe(st, c->probe_pos.p, c->fr.n_owned, c->probe_base, c->fr.seed_hash, q, first_sample, n_samples);      // a probe frame (pt_probes.hip) has no camera and no lens
    else if (c->lens.aperture_radius > 0.0f) pt_launch_raygen_lens(st, c->cam, c->lens, c->fr, q, first_sample, n_samples);      // the thin lens (pt_lens.hip); the raster integrators above ignore it
    else pt_launch_raygen(st, c->cam, c->fr, q, first_sample, n_samples, false);
    const bool shadows = sc.n_lights > 0 || sc.env_ok;
    const bool small_batch = n_paths <= (1u << 26);
    // punctual lights (pt_lights.hip): a second next-event pass per bounce, on this stream alone — it needs hit and ray[b & 1] of bounce b intact and lpath to itself,
    // so any(b) does not run beside closest(b + 1) while lights exist
    const bool punctual = c->n_lights_dev > 0;
    const bool overlap = (c->trace_overlap == 2 || (c->trace_overlap == 1 && small_batch)) && shadows && ln.stream2 && ln.stack_ovf2 && !punctual;
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
      // k_shade(b) overwrites the shadow queue any(b - 1) reads and adds to the path radiance it adds to
      if (overlap && b > 0) HIP_TRY(c, hipStreamWaitEvent(st, ln.ev_any[(size_t)b - 1], 0));
      { ScopedSpan t(c, st, 2, per_kernel); pt_launch_shade(st, cfg, ln.d_scene, c->fr, q, b & 1, (uint32_t)b); }
      if (b == c->fr.max_bounces) break;                         // the last bounce's shade produces no rays
      pt_launch_scan(st, cfg, q, (b + 1) & 1);
      if (overlap) {      // any(b) on the second stream, beside closest(b + 1)
        HIP_TRY(c, hipEventRecord(ln.ev_scan[(size_t)b], st));
        HIP_TRY(c, hipStreamWaitEvent(ln.stream2, ln.ev_scan[(size_t)b], 0));
        { ScopedSpan t(c, ln.stream2, 1, per_kernel); pt_launch_trace_any(ln.stream2, cfg, sc_any, q, nullptr); c->stats.launches_trace_any++; }
        HIP_TRY(c, hipEventRecord(ln.ev_any[(size_t)b], ln.stream2));
      } else if (shadows) {
        ScopedSpan t(c, st, 1); pt_launch_trace_any(st, cfg, sc, q, nullptr); c->stats.launches_trace_any++;
      }
      if (punctual) {     // behind emission (k_shade) and the emitter / environment sample (any): the punctual sample, through the same shadow queue
        { ScopedSpan t(c, st, 2); pt_launch_shade_punctual(st, sc, q, b & 1, (uint32_t)b, c->d_lights.p, c->d_light_cdf.p, c->n_lights_dev); }
        pt_launch_scan(st, cfg, q, (b + 1) & 1);      // the same ray prefix again, the new shadow counts, the work counters zeroed: nothing runs beside it
        { ScopedSpan t(c, st, 1); pt_launch_trace_any(st, cfg, sc, q, nullptr); c->stats.launches_trace_any++; }
      }
    }
    // sample-order accumulation: wait for the previous batch's accumulate (it ran on the previous lane)
    if (c->n_lanes > 1 && c->batches_issued > 0) {
      const int prev = (int)((c->batches_issued - 1) % (uint64_t)c->n_lanes);
      if (prev != l) HIP_TRY(c, hipStreamWaitEvent(st, c->lanes[(size_t)prev].acc_done, 0));
    }
    if (c->adaptive) pt_launch_ad_accumulate(st, c->fr.n_owned, c->ad_slot[c->ad_cur].p, q.lpath, c->accum.p, dev_adaptive(c), n_samples);
    else pt_launch_accumulate(st, c->fr, q, c->accum.p, n_samples);
    // a probe frame: the SH projection of the same path radiance, inside the same sample-order bracket (it has its own sums, so the two do not order each other)
    if (c->probe) pt_launch_accumulate_sh(st, c->fr.n_owned, c->probe_base, c->fr.seed_hash, q.lpath, c->probe_acc.p, first_sample, n_samples);
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
  if ((rc = run_batch(c, (int)(c->batches_issued % (uint64_t)c->n_lanes), c->sample_base + c->samples_done, k))) return rc;
  c->samples_done += k;
  c->stats.paths += cap;
  return PTC_OK;
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

// A refit or a rebuild is about to overwrite the shading records.  A live temporal history whose frame saw the records as they lie now keeps their positions: the
// next ptc_temporal_accumulate needs where every primitive WAS.  Queued on stream 0; the callers wait for the lanes before they touch the scene.  A static scene
// never comes here, and of several refits between two accumulates only the first copies.
int temporal_keep_positions(ptc_ctx* c) {
  if (!c->tp_live || c->tp_snap_current || c->device < 0) return PTC_OK;
  const uint32_t n_prims = c->built->n_tris;
  int rc = ensure_buf(c, c->tp_snap, (size_t)3 * n_prims);
  if (rc) return rc;
  pt_launch_temporal_snapshot(c->lanes[0].stream, c->scene.dsc.shade, c->scene.dsc.shade_stride, n_prims, c->tp_snap.p);
  HIP_TRY(c, hipGetLastError());
  c->tp_snap_current = true;
  return PTC_OK;
}

int need_device(ptc_ctx* c) {
  if (!c) return PTC_E_ARG;
  if (c->device < 0) return fail(c, PTC_E_DEVICE, kNoDevice);
  HIP_TRY(c, hipSetDevice(c->device));
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

int debug_prepare(ptc_ctx* c, uint32_t n, const char* who) {
  { int rd = need_device(c); if (rd) return rd; }
  if (!c->committed) return fail(c, PTC_E_STATE, std::string(who) + ": scene not committed");
  { int rf = flush(c); if (rf) return rf; }
  { int rs = sync_all_lanes(c); if (rs) return rs; }
  c->in_frame = false; c->pending = 0; drop_guides(c);
  int rc = ensure_lane_queues(c, n);
  if (rc) return rc;
  for (auto& ln : c->lanes) HIP_TRY(c, hipMemset(ln.q.stats, 0, ST_N * ST_STRIDE * sizeof(unsigned long long)));
  return PTC_OK;
}

}  // namespace

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
  std::snprintf(buf, sizeof buf, " | stack_lds_max=6 segments_per_cu_default=64 nodelets=%u lanes=%d batch_paths=%zu trace_overlap=%d(<=2^26 paths) rays_per_lane=%d shade_sort=%d refit=%s bvh=%s",
                x.toplet_budget, x.n_lanes, x.max_batch_paths, x.trace_overlap, x.trace_rays_per_lane, x.cfg.shade_sort, x.refit_on_device ? "device" : "host",
                x.bvh_builder == PTC_BVH_LBVH ? "lbvh" : "sah");
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
    if (const char* s = std::getenv("PTC_NODELETS")) c->toplet_budget = (uint32_t)std::strtoul(s, nullptr, 10);
    if (const char* s = std::getenv("PTC_BVH")) { if (std::strcmp(s, "lbvh") == 0) c->bvh_default = c->bvh_builder = PTC_BVH_LBVH; }
    if (const char* s = std::getenv("PTC_DEVICE_BVH")) { if (std::strcmp(s, "sah") == 0) c->device_builder = PTC_BVH_SAH; }
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
  if (const char* s = std::getenv("PTC_NODELETS")) c->toplet_budget = (uint32_t)std::strtoul(s, nullptr, 10);
  if (const char* s = std::getenv("PTC_BATCH_PATHS")) { size_t v = std::strtoull(s, nullptr, 10); if (v >= 1024) c->max_batch_paths = v; }
  if (const char* s = std::getenv("PTC_TIMING")) { const int v = std::atoi(s); c->timing = v < 0 ? 0 : (v > 2 ? 2 : v); }
  if (const char* s = std::getenv("PTC_BVH")) { if (std::strcmp(s, "lbvh") == 0) c->bvh_default = c->bvh_builder = PTC_BVH_LBVH; }
  if (const char* s = std::getenv("PTC_DEVICE_BVH")) { if (std::strcmp(s, "sah") == 0) c->device_builder = PTC_BVH_SAH; }
  if (const char* s = std::getenv("PTC_LANES")) { int v = std::atoi(s); if (v >= 1 && v <= 8) c->n_lanes = v; }
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
  if (c->comm && c->comm_owned && g_rccl.so) (void)g_rccl.CommDestroy(c->comm);
  for (const Span& s : c->spans) { (void)hipEventDestroy(s.a); (void)hipEventDestroy(s.b); }
  for (hipEvent_t e : c->free_events) (void)hipEventDestroy(e);
  for (auto& ln : c->lanes) {
    if (ln.acc_done) (void)hipEventDestroy(ln.acc_done);
    free_all(ln.allocs);
    if (ln.q.cnt) (void)hipFree(ln.q.cnt);
    if (ln.q.stats) (void)hipFree(ln.q.stats);
    if (ln.q.seg_ray[0]) (void)hipFree(ln.q.seg_ray[0]);
    if (ln.d_scene) (void)hipFree(ln.d_scene);
    if (ln.stream) (void)hipStreamDestroy(ln.stream);
    if (ln.stream2) (void)hipStreamDestroy(ln.stream2);
    for (hipEvent_t e : ln.ev_scan) (void)hipEventDestroy(e);
    for (hipEvent_t e : ln.ev_any) (void)hipEventDestroy(e);
  }
  release_scene(c);
  if (c->bscratch.p) (void)hipFree(c->bscratch.p);
  c->owned.release(); c->accum.release(); c->radiance.release(); c->ldr.release(); c->half.release();
  c->g_albedo.release(); c->g_normal.release(); c->g_pos.release(); c->dn_cv[0].release(); c->dn_cv[1].release(); c->denoised.release();
  c->g_prim.release(); c->g_uv.release(); c->g_stats.release();
  c->d_lights.release(); c->d_light_cdf.release();
  c->probe_pos.release(); c->probe_acc.release();
  c->dp_hist.release(); c->dp_ldr.release(); c->dp_state.release(); c->dp_half.release();
  for (hipEvent_t e : c->ev_dp) if (e) (void)hipEventDestroy(e);
  for (hipEvent_t e : c->ev_dn) if (e) (void)hipEventDestroy(e);
  for (auto* b : {&c->ad_pix[0], &c->ad_pix[1], &c->ad_slot[0], &c->ad_slot[1], &c->ad_count, &c->ad_block, &c->ad_n}) b->release();
  c->ad_mom.release(); c->ad_flags.release(); c->ad_keep.release();
  c->ad_cov4.release(); c->ad_cov2.release(); c->sv_colour.release(); c->sv_var.release();
  for (hipEvent_t e : c->ev_ad) if (e) (void)hipEventDestroy(e);
  for (int k = 0; k < 2; ++k) { c->tp_dn[k].release(); c->tp_mom[k].release(); c->tp_nz[k].release(); c->tp_pk[k].release(); }
  c->tp_motion.release(); c->tp_accum.release(); c->tp_snap.release();
  for (hipEvent_t e : c->ev_tp) if (e) (void)hipEventDestroy(e);
  delete c;
}

const char* ptc_last_error(const ptc_ctx* c) { return c ? c->err.c_str() : g_create_error.c_str(); }

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
  c->lights_dirty = c->lights_dirty || !c->lights.empty(); c->lights.clear();
  drop_history(c);         // the history is about the primitives of the scene that goes, and reads its shading records in place
  if (c->dp_state.p) HIP_TRY(c, hipMemset(c->dp_state.p, 0, sizeof(pt_display_state)));      // the adaptation state goes with the scene; the display parameters stay
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

namespace {
// what a commit_upload is for: a commit brings new primitive ids (the temporal history goes), a refit or rebuild that has to lay the arrays out anew keeps them
enum class Upload { NewScene, SameScene };
int commit_upload(ptc_ctx* c, std::chrono::steady_clock::time_point t0, Upload what, bool skeleton = false);

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
// ... and the vertices of emissive primitives alone for a refit on the device: ptc_refit_emitters reads those from the description
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
  const bool same = c->lights.size() == c0->lights.size() && (c->lights.empty() || std::memcmp(c->lights.data(), c0->lights.data(), c->lights.size() * sizeof(ptc_light_params)) == 0);
  if (!same) { c->lights = c0->lights; c->lights_dirty = true; }
}
const char* const kDescriptionChanged = "scene_refit: the scene's meshes or instances changed since the commit (only transforms may)";
const char* const kNonFinite = "scene_commit: non-finite vertex position after the instance transform";
// A group member takes device 0's description: materials are counted from it, a later ptc_scene_commit on this context rebuilds from it
void copy_description(ptc_ctx* c, const ptc_ctx* c0) {
  c->mats = c0->mats; c->meshes = c0->meshes; c->insts = c0->insts; c->texs = c0->texs; c->env = c0->env;
  c->poses.clear(); deform_take(c, c0, /*with_verts=*/false);
  for (size_t m = 0; m < c->poses.size(); ++m) if (c->poses[m].active()) c->poses[m].host_fresh = c->poses[m].emis_fresh = c0->poses[m].host_fresh;
  std::memcpy(c->cam_pos, c0->cam_pos, 12); std::memcpy(c->cam_target, c0->cam_target, 12); c->cam_fov = c0->cam_fov; c->cam_aspect = c0->cam_aspect;
  c->lens = c0->lens;
  take_lights(c, c0);
  c->have_cam = true; c->tex_linear = c0->tex_linear; c->bvh_builder = c0->bvh_builder; c->toplet_budget = c0->toplet_budget;
}

float scene_half_area(const float lo[3], const float hi[3]) {      // the host's box_half_area of the scene box
  const float ex = hi[0] - lo[0], ey = hi[1] - lo[1], ez = hi[2] - lo[2];
  return ex * ey + ey * ez + ez * ex;
}

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
  B.sa_unit = scene_half_area(m.lo, m.hi);                  // a new topology: a new unit of its cost
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
}  // namespace

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
  else c->stats.seconds_rebuild = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  c->in_frame = false; c->pending = 0; drop_guides(c);
  return PTC_OK;
}

int ptc_set_camera(ptc_ctx* c, const float pos[3], const float target[3], float fov_y, float aspect) {
  if (!c) return PTC_E_ARG;
  if (!pos || !target) return fail(c, PTC_E_ARG, "set_camera: null pointer");
  std::memcpy(c->cam_pos, pos, 12); std::memcpy(c->cam_target, target, 12); c->cam_fov = fov_y; c->cam_aspect = aspect;
  c->have_cam = true;
  c->guides_valid = false;      // the guides are those of the camera they were traced from
  if (c->committed) ptc_make_camera(c->cam_pos, c->cam_target, c->cam_fov, c->cam_aspect, c->cam);
  return PTC_OK;
}

// ---- thin-lens camera (pt_lens.h) ---------------------------------------------------------------------------------------------------------
void ptc_lens_default_params(ptc_lens_params* p) {
  if (!p) return;
  p->aperture_radius = 0.0f; p->focus_distance = 1.0f; p->blades = 0; p->rotation = 0.0f;
}

namespace {
const char* lens_params_error(const ptc_lens_params& p) {
  if (!(p.aperture_radius >= 0.0f) || !std::isfinite(p.aperture_radius)) return "aperture_radius must be finite and >= 0";
  if (!(p.focus_distance > 0.0f) || !std::isfinite(p.focus_distance)) return "focus_distance must be finite and > 0";
  if (p.blades != 0 && (p.blades < 3 || p.blades > 16)) return "blades must be 0 (disk) or 3..16";
  if (!(p.rotation >= 0.0f && p.rotation < 1.0f)) return "rotation must be in [0, 1)";
  return nullptr;
}
uint32_t frame_seed_hash(uint64_t seed) { return pt_lens_pcg((uint32_t)seed + pt_lens_pcg((uint32_t)(seed >> 32))); }   // as ptc_frame_begin
}  // namespace

int ptc_set_camera_lens(ptc_ctx* c, const ptc_lens_params* params) {
  if (!c) return PTC_E_ARG;
  ptc_lens_params p;
  ptc_lens_default_params(&p);
  if (params) p = *params;
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
  if (c->lights.size() >= PTC_MAX_LIGHTS) return fail(c, PTC_E_ARG, "add_light: more than PTC_MAX_LIGHTS lights");
  ptc_light_params p = *params;
  pt_light_normalise(p);
  c->lights.push_back(p);
  c->lights_dirty = true;
  return (int)c->lights.size() - 1;
}

int ptc_update_light(ptc_ctx* c, int id, const ptc_light_params* params) {
  if (!c) return PTC_E_ARG;
  if (!params || id < 0 || (size_t)id >= c->lights.size()) return fail(c, PTC_E_ARG, "update_light: null pointer or light id out of range");
  if (const char* e = pt_light_params_error(*params)) return fail(c, PTC_E_ARG, std::string("update_light: ") + e);
  ptc_light_params p = *params;
  pt_light_normalise(p);
  c->lights[(size_t)id] = p;
  c->lights_dirty = true;
  return PTC_OK;
}

int ptc_get_light(const ptc_ctx* c, int id, ptc_light_params* out) {
  if (!c || !out || id < 0 || (size_t)id >= c->lights.size()) return PTC_E_ARG;
  *out = c->lights[(size_t)id];
  return PTC_OK;
}

int ptc_light_count(const ptc_ctx* c) { return c ? (int)c->lights.size() : PTC_E_ARG; }

int ptc_clear_lights(ptc_ctx* c) {
  if (!c) return PTC_E_ARG;
  if (!c->lights.empty()) { c->lights.clear(); c->lights_dirty = true; }
  return PTC_OK;
}

// ---- display transform (pt_display.h, pt_display.hip) ----------------------------------------------------------------------------------------
namespace {
// the histogram, the state record (zeroed when it is made: no adaptation state) and the events; what the display calls need before they queue anything
int ensure_display(ptc_ctx* c, const char* who) {
  if (!c->radiance.p || c->rad_w == 0) return fail(c, PTC_E_STATE, std::string(who) + ": nothing rendered");
  if ((size_t)c->rad_w * c->rad_h > PT_DISPLAY_MAX_PIXELS) return fail(c, PTC_E_ARG, std::string(who) + ": more than 2^28 pixels");
  int rc;
  if ((rc = ensure_buf(c, c->dp_hist, PT_DISPLAY_BINS + 4))) return rc;
  if (!c->dp_state.p) {
    if ((rc = ensure_buf(c, c->dp_state, 1))) return rc;
    HIP_TRY(c, hipMemsetAsync(c->dp_state.p, 0, sizeof(pt_display_state), c->lanes[0].stream));
    HIP_TRY(c, hipMemsetAsync(c->dp_hist.p, 0, (PT_DISPLAY_BINS + 4) * sizeof(uint32_t), c->lanes[0].stream));
  }
  for (hipEvent_t& e : c->ev_dp) if (!e) HIP_TRY(c, hipEventCreate(&e));
  return PTC_OK;
}
int queue_display_half(ptc_ctx* c, const char* who) {
  { int rd = need_device(c); if (rd) return rd; }
  int rc;
  if ((rc = ensure_display(c, who))) return rc;
  const size_t n = (size_t)c->rad_w * c->rad_h;
  if ((rc = ensure_buf(c, c->dp_half, n))) return rc;
  hipStream_t s0 = c->lanes[0].stream;
  HIP_TRY(c, hipEventRecord(c->ev_dp[2], s0));
  pt_launch_display_half(s0, served_image(c), (uint32_t)n, c->dp_state.p, c->display, c->dp_half.p);
  HIP_TRY(c, hipGetLastError());
  HIP_TRY(c, hipEventRecord(c->ev_dp[3], s0));
  c->ev_dp_recorded[1] = true;
  return PTC_OK;
}
}  // namespace

void ptc_display_default_params(ptc_display_params* p) { if (p) pt_display_defaults(*p); }

int ptc_set_display(ptc_ctx* c, const ptc_display_params* params) {
  if (!c) return PTC_E_ARG;
  ptc_display_params p;
  pt_display_defaults(p);
  if (params) p = *params;
  if (const char* e = pt_display_params_error(p)) return fail(c, PTC_E_ARG, std::string("set_display: ") + e);
  c->display = p;
  return PTC_OK;
}

int ptc_get_display(const ptc_ctx* c, ptc_display_params* out) {
  if (!c || !out) return PTC_E_ARG;
  *out = c->display;
  return PTC_OK;
}

int ptc_meter_exposure(ptc_ctx* c) {
  { int rd = need_device(c); if (rd) return rd; }
  int rc;
  if ((rc = ensure_display(c, "meter_exposure"))) return rc;
  hipStream_t s0 = c->lanes[0].stream;
  HIP_TRY(c, hipEventRecord(c->ev_dp[0], s0));
  pt_launch_meter(s0, served_image(c), (uint32_t)((size_t)c->rad_w * c->rad_h), c->dp_hist.p, c->dp_state.p, c->display);
  HIP_TRY(c, hipGetLastError());
  HIP_TRY(c, hipEventRecord(c->ev_dp[1], s0));
  c->ev_dp_recorded[0] = true;
  return PTC_OK;
}

int ptc_exposure_reset(ptc_ctx* c) {
  { int rd = need_device(c); if (rd) return rd; }
  if (c->dp_state.p) HIP_TRY(c, hipMemsetAsync(c->dp_state.p, 0, sizeof(pt_display_state), c->lanes[0].stream));      // behind a metering still queued
  return PTC_OK;
}

int ptc_debug_display_state(ptc_ctx* c, uint32_t out[8]) {
  { int rd = need_device(c); if (rd) return rd; }
  if (!out) return fail(c, PTC_E_ARG, "debug_display_state: null pointer");
  std::memset(out, 0, 8 * sizeof(uint32_t));
  if (!c->dp_state.p) return PTC_OK;
  HIP_TRY(c, hipStreamSynchronize(c->lanes[0].stream));
  HIP_TRY(c, hipMemcpy(out, c->dp_state.p, sizeof(pt_display_state), hipMemcpyDeviceToHost));
  return PTC_OK;
}

int ptc_get_exposure(ptc_ctx* c, float* scale_E, float* adapted_luminance, float* metered_luminance, uint64_t* metered, uint64_t* rejected) {
  uint32_t w[8];
  { int rc = ptc_debug_display_state(c, w); if (rc) return rc; }
  pt_display_state st;
  std::memcpy(&st, w, sizeof st);
  if (scale_E) *scale_E = pt_display_scale(c->display, st.A);
  if (adapted_luminance) *adapted_luminance = pt_display_float(st.A);
  if (metered_luminance) *metered_luminance = pt_display_float(st.Q);
  if (metered) *metered = st.N;
  if (rejected) *rejected = st.rejected;
  return PTC_OK;
}

int ptc_read_luminance_histogram(ptc_ctx* c, uint32_t out[4096]) {
  { int rd = need_device(c); if (rd) return rd; }
  if (!out) return fail(c, PTC_E_ARG, "read_luminance_histogram: null pointer");
  if (!c->dp_hist.p || !c->ev_dp_recorded[0]) return fail(c, PTC_E_STATE, "read_luminance_histogram: nothing metered (ptc_meter_exposure)");
  HIP_TRY(c, hipStreamSynchronize(c->lanes[0].stream));
  HIP_TRY(c, hipMemcpy(out, c->dp_hist.p, PT_DISPLAY_BINS * sizeof(uint32_t), hipMemcpyDeviceToHost));
  return PTC_OK;
}

int ptc_display_rgba8(ptc_ctx* c, uint8_t* out) {
  { int rd = need_device(c); if (rd) return rd; }
  if (!out) return fail(c, PTC_E_ARG, "display_rgba8: null pointer");
  int rc;
  if ((rc = ensure_display(c, "display_rgba8"))) return rc;
  const size_t n = (size_t)c->rad_w * c->rad_h;
  if ((rc = ensure_buf(c, c->dp_ldr, n))) return rc;
  hipStream_t s0 = c->lanes[0].stream;
  HIP_TRY(c, hipEventRecord(c->ev_dp[2], s0));
  pt_launch_display_rgba8(s0, served_image(c), (uint32_t)n, c->dp_state.p, c->display, c->dp_ldr.p);
  HIP_TRY(c, hipGetLastError());
  HIP_TRY(c, hipEventRecord(c->ev_dp[3], s0));
  c->ev_dp_recorded[1] = true;
  HIP_TRY(c, hipStreamSynchronize(s0));
  HIP_TRY(c, hipMemcpy(out, c->dp_ldr.p, n * 4, hipMemcpyDeviceToHost));
  return PTC_OK;
}

int ptc_display_rgba16f(ptc_ctx* c, uint16_t* out) {
  if (c && c->device >= 0 && !out) return fail(c, PTC_E_ARG, "display_rgba16f: null pointer");
  { int rc = queue_display_half(c, "display_rgba16f"); if (rc) return rc; }
  HIP_TRY(c, hipStreamSynchronize(c->lanes[0].stream));
  HIP_TRY(c, hipMemcpy(out, c->dp_half.p, (size_t)c->rad_w * c->rad_h * sizeof(uint2), hipMemcpyDeviceToHost));
  return PTC_OK;
}
void* ptc_display_rgba16f_device_ptr(ptc_ctx* c) {
  if (queue_display_half(c, "display_rgba16f_device_ptr")) return nullptr;
  if (hipStreamSynchronize(c->lanes[0].stream) != hipSuccess) return nullptr;
  return (void*)c->dp_half.p;
}

int ptc_get_display_seconds(ptc_ctx* c, double* meter, double* display) {
  { int rd = need_device(c); if (rd) return rd; }
  double* out[2] = {meter, display};
  for (int k = 0; k < 2; ++k) {
    if (!out[k]) continue;
    *out[k] = 0.0;
    if (!c->ev_dp_recorded[k]) continue;
    HIP_TRY(c, hipEventSynchronize(c->ev_dp[2 * k + 1]));
    float ms = 0.0f;
    HIP_TRY(c, hipEventElapsedTime(&ms, c->ev_dp[2 * k], c->ev_dp[2 * k + 1]));
    *out[k] = 1e-3 * (double)ms;
  }
  return PTC_OK;
}

int ptc_debug_display_internals(ptc_ctx* c, uint64_t out[4]) {
  if (!c || !out) return PTC_E_ARG;
  out[0] = pt_display_meter_grid_pixels(); out[1] = 0; out[2] = 0; out[3] = 0;
  return PTC_OK;
}

int ptc_debug_display_pixel(const ptc_display_params* params, float E, const float rgba_in[4], uint8_t out8[4], uint16_t out16[4]) {
  ptc_display_params p;
  pt_display_defaults(p);
  if (params) p = *params;
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
  ptc_display_params p;
  pt_display_defaults(p);
  if (params) p = *params;
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

int ptc_focus_distance_at_pixel(ptc_ctx* c, int px, int py, float* out) {
  { int rd = need_device(c); if (rd) return rd; }
  if (!out) return fail(c, PTC_E_ARG, "focus_distance_at_pixel: null pointer");
  if (c->probe) return fail(c, PTC_E_STATE, "focus_distance_at_pixel: a probe frame has no camera image");
  if (!c->guides_valid) return fail(c, PTC_E_STATE, "focus_distance_at_pixel: no guides (ptc_frame_guides)");
  const int w = c->rad_w, h = c->rad_h;
  if (px < 0 || py < 0 || px >= w || py >= h) return fail(c, PTC_E_ARG, "focus_distance_at_pixel: pixel outside the frame");
  HIP_TRY(c, hipStreamSynchronize(c->lanes[0].stream));
  float4 nz;
  HIP_TRY(c, hipMemcpy(&nz, c->g_normal.p + ((size_t)py * (size_t)w + (size_t)px), sizeof nz, hipMemcpyDeviceToHost));
  // the pixel-centre ray of k_raygen_guides: Z is t along the unit ray, the view depth is t over the length of (dvx, dvy, 1)
  const float fx = ((float)px + 0.5f) / (float)w, fy = ((float)py + 0.5f) / (float)h;
  const float dvx = (2.0f * fx - 1.0f) * c->cam.sx, dvy = (2.0f * fy - 1.0f) * c->cam.sy;
  *out = nz.w / std::sqrt(pt_lens_fma(dvy, dvy, pt_lens_fma(dvx, dvx, 1.0f)));
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

namespace {
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
// Device half of a commit: upload c->built, size the launches.  The caller has set c->built, the camera and seconds_commit's start.
// skeleton: c->built is ptc_build_skeleton's — the tables are uploaded, the shading records allocated and zeroed, there is no tree yet: device_commit goes on from here.
int commit_upload(ptc_ctx* c, std::chrono::steady_clock::time_point t0, Upload what, bool skeleton) {
  if (what == Upload::NewScene) drop_history(c);      // every commit passes here — ptc_scene_commit on the host or on the device, each context of ptc_group_scene_commit
  ptc_make_camera(c->cam_pos, c->cam_target, c->cam_fov, c->cam_aspect, c->cam);
  c->in_frame = false; c->pending = 0; drop_guides(c);
  c->committed = false;
  release_scene(c);
  CommittedScene& s = c->scene;
  s.insts = c->insts.size();
  deform_all_live(c);      // every caller lays the scene out from the fully evaluated description
  for (MeshPose& P : c->poses) if (P.active()) P.dev_fresh = P.host_fresh;
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
}  // namespace

int ptc_scene_commit(ptc_ctx* c) { return scene_commit(c, true); }

namespace {
// ptc_frame_begin, and ptc_probes_begin's share of it: probe_pos != nullptr begins a probe frame of w probes (h = 1, the path integrator, no tiles) — the "owned
// pixels" are the probes in their own order, the positions go to the device, the 27 w sums are cleared and the probe flag is set
int frame_begin(ptc_ctx* c, int w, int h, int spp_total, uint64_t seed, int max_bounces, int integrator, int tile_rank, int tile_count, const float* probe_pos,
                uint32_t probe_base) {
  { int rd = need_device(c); if (rd) return rd; }
  c->in_frame = false; c->pending = 0; c->adaptive = false; c->cov_on = false; c->cov_resolved = false; c->sv_valid = false; drop_guides(c);      // whatever happens below, the previous frame is over
  const std::string who = probe_pos ? "probes_begin" : "frame_begin";      // the entry the caller used, for ptc_last_error
  if (!c->committed) return fail(c, PTC_E_STATE, who + ": scene not committed");
  if (w <= 0 || h <= 0 || spp_total <= 0 || max_bounces < 0 || (uint64_t)w * (uint64_t)h > 0x7fffffffull) return fail(c, PTC_E_ARG, who + ": bad size");
  if (integrator != PTC_INTEGRATOR_PATH && !is_raster(integrator)) return fail(c, PTC_E_ARG, who + ": unknown integrator");
  if (tile_count < 1 || tile_rank < 0 || tile_rank >= tile_count) return fail(c, PTC_E_ARG, who + ": bad tile rank/count");
  { int rs = sync_all_lanes(c); if (rs) return rs; }
  int rc;
  if ((rc = upload_lights(c))) return rc;      // a changed light table: nothing is queued any more that reads the old one
  // the list of owned pixels (tile-Morton order) depends on the image size and the tile assignment only: a viewer that renders frame after frame at
  // one size keeps the list it has on the device (2 M entries: 10 ms of host time and an 8 MB upload per frame otherwise — tools/viewer_loop.py)
  if (probe_pos) {      // probe j is "pixel" j: the identity list (the next camera frame makes its own)
    std::vector<uint32_t> owned((size_t)w);
    std::vector<float4> pos((size_t)w);
    for (int j = 0; j < w; ++j) { owned[(size_t)j] = (uint32_t)j; pos[(size_t)j] = make_float4(probe_pos[j * 3], probe_pos[j * 3 + 1], probe_pos[j * 3 + 2], 0.0f); }
    c->owned_key_valid = false;
    if ((rc = ensure_buf(c, c->owned, owned.size())) || (rc = ensure_buf(c, c->probe_pos, pos.size())) || (rc = ensure_buf(c, c->probe_acc, (size_t)PT_SH9_FLOATS * (size_t)w))) return rc;
    HIP_TRY(c, hipMemcpy(c->owned.p, owned.data(), owned.size() * 4, hipMemcpyHostToDevice));
    HIP_TRY(c, hipMemcpy(c->probe_pos.p, pos.data(), pos.size() * sizeof(float4), hipMemcpyHostToDevice));
    HIP_TRY(c, hipMemsetAsync(c->probe_acc.p, 0, (size_t)PT_SH9_FLOATS * (size_t)w * sizeof(float), c->lanes[0].stream));
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
  {  // seed_hash = pcg(seed_lo + pcg(seed_hi)), same hash as pt_device.h
    auto pcg = [](uint32_t v) { uint32_t s = v * 747796405u + 2891336453u; uint32_t x = ((s >> ((s >> 28) + 4u)) ^ s) * 277803737u; return (x >> 22) ^ x; };
    c->fr.seed_hash = pcg((uint32_t)seed + pcg((uint32_t)(seed >> 32)));
  }
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
    for (const auto& ln : c->lanes) held += (size_t)ln.q.cap * kQueueBytesPerPath;
    if (hipMemGetInfo(&free_b, &total_b) == hipSuccess) {
      const size_t fit = (size_t)(0.6 * (double)(free_b + held)) / kQueueBytesPerPath;
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
  c->in_frame = true;
  c->probe = probe_pos != nullptr; c->probe_base = probe_base;
  return PTC_OK;
}
}  // namespace

int ptc_frame_begin(ptc_ctx* c, int w, int h, int spp_total, uint64_t seed, int max_bounces, int integrator, int tile_rank, int tile_count) {
  return frame_begin(c, w, h, spp_total, seed, max_bounces, integrator, tile_rank, tile_count, nullptr, 0);
}

// ---- light probes (pt_probes.h) ------------------------------------------------------------------------------------------------
#define PTC_MAX_PROBES (1 << 26)      // 9 lanes per probe and 27 sums per probe stay inside 32-bit indices
int ptc_probes_begin(ptc_ctx* c, const float* positions_xyz, int n_probes, uint32_t probe_index_base, int spp_total, uint64_t seed, int max_bounces) {
  if (!c) return PTC_E_ARG;
  if (!positions_xyz) return fail(c, PTC_E_ARG, "probes_begin: null pointer");
  if (n_probes < 1 || n_probes > PTC_MAX_PROBES) return fail(c, PTC_E_ARG, "probes_begin: n_probes outside 1..2^26");
  if (spp_total < 1 || max_bounces < 0) return fail(c, PTC_E_ARG, "probes_begin: spp_total < 1 or max_bounces < 0");
  if ((uint64_t)probe_index_base + (uint64_t)n_probes > 0x100000000ull) return fail(c, PTC_E_ARG, "probes_begin: probe indices exceed 32 bits");
  for (size_t i = 0; i < (size_t)n_probes * 3; ++i)
    if (!std::isfinite(positions_xyz[i])) return fail(c, PTC_E_ARG, "probes_begin: a position is not finite");
  return frame_begin(c, n_probes, 1, spp_total, seed, max_bounces, PTC_INTEGRATOR_PATH, 0, 1, positions_xyz, probe_index_base);
}

int ptc_probes_read_sh(ptc_ctx* c, float* out) {
  { int rd = need_device(c); if (rd) return rd; }
  if (!out) return fail(c, PTC_E_ARG, "probes_read_sh: null pointer");
  if (!c->in_frame || !c->probe) return fail(c, PTC_E_STATE, "probes_read_sh: no probe frame (ptc_probes_begin)");
  { int rf = flush(c); if (rf) return rf; }
  { int rs = sync_all_lanes(c); if (rs) return rs; }
  const size_t n = (size_t)c->fr.n_owned * PT_SH9_FLOATS;
  HIP_TRY(c, hipMemcpy(out, c->probe_acc.p, n * sizeof(float), hipMemcpyDeviceToHost));
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

int ptc_frame_reserve(ptc_ctx* c) {
  { int rd = need_device(c); if (rd) return rd; }
  if (!c->in_frame) return fail(c, PTC_E_STATE, "frame_reserve: no frame");
  if (c->fr.n_owned == 0) return PTC_OK;
  const uint32_t k = is_raster(c->integrator) ? 1u : (c->per_batch < (uint32_t)c->spp_total ? c->per_batch : (uint32_t)c->spp_total);
  return ensure_lane_queues(c, c->fr.n_owned * k);     // n_owned * per_batch fits 32 bits by construction (frame_begin)
}

int ptc_frame_add_samples(ptc_ctx* c, int n_samples) {
  { int rd = need_device(c); if (rd) return rd; }
  if (!c->in_frame) return fail(c, PTC_E_STATE, "frame_add_samples: no frame");
  if (n_samples <= 0) return fail(c, PTC_E_ARG, "frame_add_samples: n_samples <= 0");
  if (c->adaptive && c->fr.n_owned == 0) return PTC_OK;      // nothing is active: accepted, nothing to do
  if (!is_raster(c->integrator) && (uint64_t)c->samples_done + c->pending + (uint64_t)n_samples > (uint64_t)c->spp_total)
    return fail(c, PTC_E_ARG, "frame_add_samples: more samples than the spp_total given to frame_begin");
  c->pending += (uint32_t)n_samples;
  c->cov_resolved = false;          // the sums are about to hold samples the radiance buffer does not (ptc_denoise_sampled)
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
  if (c->adaptive) { if (c->samples_done) pt_launch_ad_resolve(c->lanes[0].stream, c->owned_n, c->owned.p, c->accum.p, c->ad_count.p, c->radiance.p); }
  else if (c->fr.n_owned && c->samples_done)
    pt_launch_resolve(c->lanes[0].stream, c->fr, c->accum.p, c->radiance.p, (float)(c->resolve_divisor ? c->resolve_divisor : c->samples_done), is_raster(c->integrator));
  HIP_TRY(c, hipGetLastError());
  c->cov_resolved = true;
  return PTC_OK;
}

int ptc_frame_set_sample_range(ptc_ctx* c, uint32_t first_sample, uint32_t resolve_divisor) {
  { int rd = need_device(c); if (rd) return rd; }
  if (!c->in_frame) return fail(c, PTC_E_STATE, "frame_set_sample_range: no frame");
  if (c->samples_done || c->pending) return fail(c, PTC_E_STATE, "frame_set_sample_range: call it right after ptc_frame_begin, before any sample");
  if (is_raster(c->integrator)) return fail(c, PTC_E_ARG, "frame_set_sample_range: the raster integrators have one sample");
  if ((uint64_t)first_sample + (uint64_t)c->spp_total > 0xffffffffull) return fail(c, PTC_E_ARG, "frame_set_sample_range: sample indices exceed 32 bits");
  if (c->adaptive && resolve_divisor) return fail(c, PTC_E_STATE, "frame_set_sample_range: an adaptive frame resolves every pixel by its own count, not by a divisor");
  c->sample_base = first_sample; c->resolve_divisor = resolve_divisor;
  return PTC_OK;
}

int ptc_frame_checkpoint(ptc_ctx* c, float* accum_rgba, uint64_t* n_owned_pixels, uint32_t* samples_done) {
  { int rd = need_device(c); if (rd) return rd; }
  if (!c->in_frame) return fail(c, PTC_E_STATE, "frame_checkpoint: no frame");
  if (is_raster(c->integrator)) return fail(c, PTC_E_ARG, "frame_checkpoint: the raster integrators have nothing to resume");
  if (c->adaptive) return fail(c, PTC_E_STATE, "frame_checkpoint: not available in an adaptive frame");
  if (c->probe) return fail(c, PTC_E_STATE, "frame_checkpoint: not available in a probe frame");
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
  if (c->probe) return fail(c, PTC_E_STATE, "frame_restore: not available in a probe frame");
  if (!accum_rgba) return fail(c, PTC_E_ARG, "frame_restore: null pointer");
  if (c->adaptive) return fail(c, PTC_E_STATE, "frame_restore: not available in an adaptive frame");
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
  { int rd = need_device(c); if (rd) return rd; }
  if (!out) return fail(c, PTC_E_ARG, "read_radiance: null pointer");
  if (!c->radiance.p || c->rad_w == 0) return fail(c, PTC_E_STATE, "read_radiance: nothing rendered");
  { int rs = sync_all_lanes(c); if (rs) return rs; }
  HIP_TRY(c, hipMemcpy(out, served_image(c), (size_t)c->rad_w * c->rad_h * sizeof(float4), hipMemcpyDeviceToHost));
  return PTC_OK;
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

// ---- first-hit guide buffers + the variance-guided à-trous denoiser (pt_denoise.hip) -----------------------------------------
namespace {
int ensure_dn_events(ptc_ctx* c) {
  for (hipEvent_t& e : c->ev_dn) if (!e) HIP_TRY(c, hipEventCreate(&e));
  return PTC_OK;
}
}  // namespace

int ptc_frame_guides(ptc_ctx* c) {
  { int rd = need_device(c); if (rd) return rd; }
  if (!c->in_frame) return fail(c, PTC_E_STATE, "frame_guides: no frame");
  if (c->probe) return fail(c, PTC_E_STATE, "frame_guides: a probe frame has no camera image to guide");
  if (c->integrator != PTC_INTEGRATOR_PATH) return fail(c, PTC_E_STATE, "frame_guides: the frame is not a PTC_INTEGRATOR_PATH frame (the raster integrators are noise-free)");
  const uint32_t n = (uint32_t)c->fr.w * (uint32_t)c->fr.h;      // every pixel, whatever the frame's tile share: the root of a sharded frame denoises the whole image
  int rc;
  if ((rc = ensure_buf(c, c->g_albedo, n)) || (rc = ensure_buf(c, c->g_normal, n)) || (rc = ensure_buf(c, c->g_pos, n)) || (rc = ensure_buf(c, c->g_prim, n)) ||
      (rc = ensure_buf(c, c->g_uv, n)) || (rc = ensure_dn_events(c))) return rc;
  if (!c->g_stats.p) {
    if ((rc = ensure_buf(c, c->g_stats, (size_t)ST_N * ST_STRIDE))) return rc;
    HIP_TRY(c, hipMemset(c->g_stats.p, 0, ST_N * ST_STRIDE * sizeof(unsigned long long)));
  }
  // The guide rays borrow lane 0's queues between two batches (a batch leaves nothing in them: its radiance is in the sums once k_accumulate ran) and are
  // traced in chunks of what the lane holds; a lane without queues yet gets them for one sample per pixel, at most 2 M paths.
  {
    const uint32_t want = n < (1u << 21) ? n : (1u << 21);
    if (c->lanes[0].q.cap < want && (rc = ensure_lane_queues(c, want))) return rc;
  }
  Lane& ln = c->lanes[0];
  hipStream_t st = ln.stream;
  const DevScene sc = lane_scene(c, 0);
  const GuideBufs g = {c->g_albedo.p, c->g_normal.p, c->g_pos.p, c->g_prim.p, c->g_uv.p};
  const uint32_t chunk = ln.q.cap < n ? ln.q.cap : n;
  HIP_TRY(c, hipEventRecord(c->ev_dn[0], st));
  for (uint32_t first = 0; first < n; first += chunk) {
    const uint32_t m = n - first < chunk ? n - first : chunk;
    DevQueues q = batch_queues(c, 0, m);
    q.stats = c->g_stats.p;            // the frame's counters do not see the guide rays
    const LaunchCfg cfg = batch_cfg(c, m);
    pt_launch_set_counts(st, cfg, q, m, 0);
    pt_launch_raygen_guides(st, c->cam, c->fr.w, c->fr.h, first, m, q);
    pt_launch_trace_closest(st, cfg, sc, q, 0, false);
    pt_launch_guides(st, sc, c->cam, c->fr.w, c->fr.h, first, m, q, g);
  }
  HIP_TRY(c, hipEventRecord(c->ev_dn[1], st));
  HIP_TRY(c, hipGetLastError());
  c->ev_dn_recorded[0] = true;
  c->guides_valid = true;
  return PTC_OK;
}

int ptc_read_guide_rgba32f(ptc_ctx* c, int which, float* out) {
  { int rd = need_device(c); if (rd) return rd; }
  if (!out) return fail(c, PTC_E_ARG, "read_guide: null pointer");
  if (which != PTC_GUIDE_ALBEDO && which != PTC_GUIDE_NORMAL_DEPTH) return fail(c, PTC_E_ARG, "read_guide: unknown guide");
  if (!c->guides_valid) return fail(c, PTC_E_STATE, "read_guide: no guides (ptc_frame_guides)");
  HIP_TRY(c, hipStreamSynchronize(c->lanes[0].stream));
  HIP_TRY(c, hipMemcpy(out, which == PTC_GUIDE_ALBEDO ? c->g_albedo.p : c->g_normal.p, (size_t)c->rad_w * c->rad_h * sizeof(float4), hipMemcpyDeviceToHost));
  return PTC_OK;
}

int ptc_read_guide_hit(ptc_ctx* c, int32_t* prim, float* uv) {
  { int rd = need_device(c); if (rd) return rd; }
  if (!c->guides_valid) return fail(c, PTC_E_STATE, "read_guide_hit: no guides (ptc_frame_guides)");
  HIP_TRY(c, hipStreamSynchronize(c->lanes[0].stream));
  const size_t n = (size_t)c->rad_w * c->rad_h;
  if (prim) HIP_TRY(c, hipMemcpy(prim, c->g_prim.p, n * sizeof(int32_t), hipMemcpyDeviceToHost));
  if (uv) HIP_TRY(c, hipMemcpy(uv, c->g_uv.p, n * sizeof(float2), hipMemcpyDeviceToHost));
  return PTC_OK;
}

void ptc_denoise_default_params(ptc_denoise_params* p) {
  if (!p) return;
  p->iterations = 4; p->sigma_l = 4.0f; p->sigma_n = 128.0f; p->sigma_p = 1.0f; p->demodulate = 1;
}

namespace {
int denoise_image(ptc_ctx* c, const ptc_denoise_params* params, bool accumulated, bool sampled = false);
}
int ptc_denoise(ptc_ctx* c, const ptc_denoise_params* params) { return denoise_image(c, params, false); }
int ptc_denoise_accumulated(ptc_ctx* c, const ptc_denoise_params* params) { return denoise_image(c, params, true); }
int ptc_denoise_sampled(ptc_ctx* c, const ptc_denoise_params* params) { return denoise_image(c, params, false, true); }

namespace {
// accumulated: the input is the accumulated image of the frame's ptc_temporal_accumulate, i.e. D_new of the new history (demodulated already) with the temporal variance
// sampled: the input is the radiance, demodulated by k_ad_sampled_variance, with the variance of the frame's own samples (§8d) where a pixel has four or more
int denoise_image(ptc_ctx* c, const ptc_denoise_params* params, bool accumulated, bool sampled) {
  { int rd = need_device(c); if (rd) return rd; }
  if (c->probe) return fail(c, PTC_E_STATE, "denoise: a probe frame has no image to denoise");
  ptc_denoise_params p;
  ptc_denoise_default_params(&p);
  if (params) p = *params;
  auto bad = [](float v) { return !(v >= 0.0f) || !(v <= 3.0e38f); };      // NaN, negative, infinite
  if (p.iterations < 0 || p.iterations > PTC_DENOISE_MAX_ITERATIONS) return fail(c, PTC_E_ARG, "denoise: iterations outside 0..8");
  if (bad(p.sigma_l) || bad(p.sigma_n) || bad(p.sigma_p)) return fail(c, PTC_E_ARG, "denoise: a sigma is negative or not finite");
  if (!c->guides_valid) return fail(c, PTC_E_STATE, "denoise: no valid guides (ptc_frame_guides after the frame's ptc_frame_begin)");
  if (!c->radiance.p || c->rad_w == 0) return fail(c, PTC_E_STATE, "denoise: no radiance buffer");
  if (accumulated && !c->tp_accum_valid) return fail(c, PTC_E_STATE, "denoise_accumulated: the frame has no accumulated image (ptc_temporal_accumulate)");
  if (accumulated && (p.demodulate ? 1 : 0) != c->tp_demodulate) return fail(c, PTC_E_ARG, "denoise_accumulated: demodulate differs from the accumulate's");
  if (sampled && !(c->in_frame && c->adaptive && c->cov_on)) return fail(c, PTC_E_STATE, "denoise_sampled: the frame is not an adaptive frame that keeps the sample covariance (ptc_set_sample_covariance before ptc_frame_set_adaptive)");
  if (sampled && (!c->cov_resolved || c->pending)) return fail(c, PTC_E_STATE, "denoise_sampled: samples were added since the last ptc_frame_resolve");
  const size_t n = (size_t)c->rad_w * c->rad_h;
  int rc;
  if ((rc = ensure_buf(c, c->denoised, n)) || (rc = ensure_dn_events(c))) return rc;
  if (sampled && ((rc = ensure_buf(c, c->sv_colour, n)) || (rc = ensure_buf(c, c->sv_var, n)))) return rc;
  if (p.iterations > 0 && ((rc = ensure_buf(c, c->dn_cv[0], n)) || (rc = ensure_buf(c, c->dn_cv[1], n)))) return rc;
  hipStream_t s0 = c->lanes[0].stream;      // behind the resolve, the reduce and the guide pass
  HIP_TRY(c, hipEventRecord(c->ev_dn[2], s0));
  if (sampled)      // also with iterations = 0: ptc_read_sampled_variance serves what this call computed
    pt_launch_ad_sampled_variance(s0, c->owned_n, c->owned.p, c->accum.p, dev_adaptive(c), c->g_albedo.p, c->radiance.p, p.demodulate ? 1 : 0, c->sv_colour.p, c->sv_var.p,
                                  (uint32_t)n, (size_t)c->owned_n != n);
  if (p.iterations == 0) HIP_TRY(c, hipMemcpyAsync(c->denoised.p, accumulated ? c->tp_accum.p : c->radiance.p, n * sizeof(float4), hipMemcpyDeviceToDevice, s0));
  else {
    DenoiseArgs a{};
    a.w = c->rad_w; a.h = c->rad_h; a.sigma_l = p.sigma_l; a.sigma_n = p.sigma_n; a.sigma_p = p.sigma_p; a.demodulate = p.demodulate ? 1 : 0;
    a.pix = (2.0f * c->cam.sy) / (float)c->rad_h;
    a.radiance = c->radiance.p;
    a.g = GuideBufs{c->g_albedo.p, c->g_normal.p, c->g_pos.p, c->g_prim.p, c->g_uv.p};
    if (sampled) {
      DenoiseArgs ap = a;
      ap.demodulate = 0;
      pt_launch_denoise_prepare(s0, ap, c->sv_colour.p, c->sv_var.p, c->dn_cv[0].p);
    } else if (accumulated) {      // D_new lies demodulated in the history; the iterations re-modulate it as they do ptc_denoise's, and pass the other classes' radiance through
      DenoiseArgs ap = a;
      ap.demodulate = 0;
      pt_launch_denoise_prepare(s0, ap, c->tp_dn[c->tp_cur].p, c->tp_mom[c->tp_cur].p, c->dn_cv[0].p);
    } else pt_launch_denoise_prepare(s0, a, c->radiance.p, nullptr, c->dn_cv[0].p);
    for (int i = 0; i < p.iterations; ++i) {
      const bool last = i == p.iterations - 1;
      pt_launch_denoise_iteration(s0, a, i, c->dn_cv[i & 1].p, last ? c->denoised.p : c->dn_cv[(i + 1) & 1].p, last);
    }
  }
  HIP_TRY(c, hipEventRecord(c->ev_dn[3], s0));
  HIP_TRY(c, hipGetLastError());
  c->ev_dn_recorded[1] = true;
  c->denoised_valid = true;
  if (sampled) c->sv_valid = true;
  return PTC_OK;
}
}  // namespace

// ---- temporal accumulation (pt_temporal.hip): the history lives in the context, see ptc_ctx ---------------------------------------------------
void ptc_temporal_default_params(ptc_temporal_params* p) {
  if (!p) return;
  p->max_history = 32; p->sigma_z = 1.0f; p->demodulate = 1;
}

int ptc_temporal_accumulate(ptc_ctx* c, const ptc_temporal_params* params) {
  { int rd = need_device(c); if (rd) return rd; }
  if (c->probe) return fail(c, PTC_E_STATE, "temporal_accumulate: a probe frame has no image to accumulate");
  ptc_temporal_params p;
  ptc_temporal_default_params(&p);
  if (params) p = *params;
  if (p.max_history < 1 || p.max_history > PTC_TEMPORAL_MAX_HISTORY) return fail(c, PTC_E_ARG, "temporal_accumulate: max_history outside 1..1024");
  if (!(p.sigma_z >= 0.0f) || !(p.sigma_z <= 3.0e38f)) return fail(c, PTC_E_ARG, "temporal_accumulate: sigma_z is negative or not finite");
  if (!c->guides_valid) return fail(c, PTC_E_STATE, "temporal_accumulate: no valid guides (ptc_frame_guides after the frame's ptc_frame_begin)");
  if (!c->radiance.p || c->rad_w == 0) return fail(c, PTC_E_STATE, "temporal_accumulate: no radiance buffer");
  const int w = c->rad_w, h = c->rad_h, demodulate = p.demodulate ? 1 : 0;
  const size_t n = (size_t)w * h;
  int rc;
  for (int k = 0; k < 2; ++k)
    if ((rc = ensure_buf(c, c->tp_dn[k], n)) || (rc = ensure_buf(c, c->tp_mom[k], n)) || (rc = ensure_buf(c, c->tp_nz[k], n)) || (rc = ensure_buf(c, c->tp_pk[k], n))) { drop_history(c); return rc; }
  // a set may have been regrown above: a failure from here on leaves no history either
  if ((rc = ensure_buf(c, c->tp_motion, n)) || (rc = ensure_buf(c, c->tp_accum, n))) { drop_history(c); return rc; }
  for (hipEvent_t& e : c->ev_tp) if (!e) { const hipError_t he = hipEventCreate(&e); if (he != hipSuccess) { drop_history(c); HIP_TRY(c, he); } }
  if (c->tp_live && (c->tp_w != w || c->tp_h != h || c->tp_demodulate != demodulate)) drop_history(c);      // another size or another quantity: not this frame's history
  TemporalArgs a{};
  a.w = w; a.h = h; a.have_history = c->tp_live ? 1 : 0; a.demodulate = demodulate;
  a.max_history = (float)p.max_history; a.sigma_z = p.sigma_z;
  a.cam_prev = c->tp_cam;
  a.pix_prev = (2.0f * c->tp_cam.sy) / (float)h;
  a.radiance = c->radiance.p;
  a.g = GuideBufs{c->g_albedo.p, c->g_normal.p, c->g_pos.p, c->g_prim.p, c->g_uv.p};
  if (c->tp_snap_current) { a.pos = c->tp_snap.p; a.pos_stride = 3; }
  else { a.pos = c->scene.dsc.shade; a.pos_stride = c->scene.dsc.shade_stride; }
  const int cur = c->tp_cur, nxt = cur ^ 1;
  a.prev = TemporalSet{c->tp_dn[cur].p, c->tp_mom[cur].p, c->tp_nz[cur].p, c->tp_pk[cur].p};
  a.next = TemporalSet{c->tp_dn[nxt].p, c->tp_mom[nxt].p, c->tp_nz[nxt].p, c->tp_pk[nxt].p};
  a.accumulated = c->tp_accum.p; a.motion = c->tp_motion.p;
  hipStream_t s0 = c->lanes[0].stream;      // behind the resolve, the reduce and the guide pass
  HIP_TRY(c, hipEventRecord(c->ev_tp[0], s0));
  pt_launch_temporal_accumulate(s0, a);
  HIP_TRY(c, hipEventRecord(c->ev_tp[1], s0));
  HIP_TRY(c, hipGetLastError());
  c->ev_tp_recorded = true;
  c->tp_cur = nxt; c->tp_live = true; c->tp_w = w; c->tp_h = h; c->tp_demodulate = demodulate; c->tp_cam = c->cam;
  c->tp_snap_current = false;      // the new history's frame saw the shading records as they lie now
  c->tp_accum_valid = true;
  return PTC_OK;
}

int ptc_temporal_reset(ptc_ctx* c) {
  { int rd = need_device(c); if (rd) return rd; }
  drop_history(c);
  return PTC_OK;
}

int ptc_read_temporal_rgba32f(ptc_ctx* c, int which, float* out) {
  { int rd = need_device(c); if (rd) return rd; }
  if (!out) return fail(c, PTC_E_ARG, "read_temporal: null pointer");
  if (which < PTC_TEMPORAL_HISTORY || which > PTC_TEMPORAL_POSITION_CLASS) return fail(c, PTC_E_ARG, "read_temporal: unknown buffer");
  if (!c->tp_live) return fail(c, PTC_E_STATE, "read_temporal: no history (ptc_temporal_accumulate)");
  // the caller sizes `out` by the frame it knows, the current one: a history of another size (a frame_begin with a new size, not accumulated yet) is not served
  if (c->tp_w != c->rad_w || c->tp_h != c->rad_h) return fail(c, PTC_E_STATE, "read_temporal: the history's size is not the current frame's (no ptc_temporal_accumulate since the size changed)");
  HIP_TRY(c, hipStreamSynchronize(c->lanes[0].stream));
  const float4* const bufs[5] = {c->tp_dn[c->tp_cur].p, c->tp_mom[c->tp_cur].p, c->tp_motion.p, c->tp_nz[c->tp_cur].p, c->tp_pk[c->tp_cur].p};
  const float4* src = bufs[which];
  HIP_TRY(c, hipMemcpy(out, src, (size_t)c->tp_w * c->tp_h * sizeof(float4), hipMemcpyDeviceToHost));
  return PTC_OK;
}

int ptc_get_temporal_seconds(ptc_ctx* c, double* accumulate) {
  { int rd = need_device(c); if (rd) return rd; }
  if (!accumulate) return PTC_OK;
  *accumulate = 0.0;
  if (!c->ev_tp_recorded) return PTC_OK;
  HIP_TRY(c, hipEventSynchronize(c->ev_tp[1]));
  float ms = 0.0f;
  HIP_TRY(c, hipEventElapsedTime(&ms, c->ev_tp[0], c->ev_tp[1]));
  *accumulate = 1e-3 * (double)ms;
  return PTC_OK;
}

int ptc_select_output(ptc_ctx* c, int output) {
  { int rd = need_device(c); if (rd) return rd; }
  if (output != PTC_OUTPUT_RADIANCE && output != PTC_OUTPUT_DENOISED && output != PTC_OUTPUT_ACCUMULATED) return fail(c, PTC_E_ARG, "select_output: unknown output");
  if (output == PTC_OUTPUT_ACCUMULATED && !c->tp_accum_valid) return fail(c, PTC_E_STATE, "select_output: the frame has no accumulated image (ptc_temporal_accumulate)");
  if (output == PTC_OUTPUT_DENOISED && !c->denoised_valid) return fail(c, PTC_E_STATE, "select_output: the frame has no denoised image (ptc_denoise)");
  c->output = output;
  return PTC_OK;
}

int ptc_get_denoise_seconds(ptc_ctx* c, double* guides, double* denoise) {
  { int rd = need_device(c); if (rd) return rd; }
  double* out[2] = {guides, denoise};
  for (int k = 0; k < 2; ++k) {
    if (!out[k]) continue;
    *out[k] = 0.0;
    if (!c->ev_dn_recorded[k]) continue;
    HIP_TRY(c, hipEventSynchronize(c->ev_dn[2 * k + 1]));
    float ms = 0.0f;
    HIP_TRY(c, hipEventElapsedTime(&ms, c->ev_dn[2 * k], c->ev_dn[2 * k + 1]));
    *out[k] = 1e-3 * (double)ms;
  }
  return PTC_OK;
}

// ---- adaptive sampling (pt_adaptive.hip): the active set lives in c->fr, see ptc_ctx ---------------------------------------------------
void ptc_adaptive_default_params(ptc_adaptive_params* p) {
  if (!p) return;
  p->threshold = 0.05f; p->radius = 1; p->min_samples = 16; p->step_samples = 16;
}

namespace {
int adaptive_params_ok(ptc_ctx* c, const ptc_adaptive_params& p, const char* who) {
  if (!(p.threshold >= 0.0f) || !(p.threshold <= 3.4028235e38f)) return fail(c, PTC_E_ARG, std::string(who) + ": the threshold is negative or not finite");
  if (p.radius < 0 || p.radius > PTC_AD_MAX_RADIUS) return fail(c, PTC_E_ARG, std::string(who) + ": radius outside 0..2");
  if (p.min_samples < 1 || p.step_samples < 1) return fail(c, PTC_E_ARG, std::string(who) + ": min_samples / step_samples < 1");
  return PTC_OK;
}
int need_adaptive_frame(ptc_ctx* c, const char* who) {
  { int rd = need_device(c); if (rd) return rd; }
  if (!c->in_frame || !c->adaptive) return fail(c, PTC_E_STATE, std::string(who) + ": no adaptive frame (ptc_frame_set_adaptive right after ptc_frame_begin)");
  return PTC_OK;
}
}  // namespace

int ptc_frame_set_adaptive(ptc_ctx* c, const ptc_adaptive_params* params) {
  { int rd = need_device(c); if (rd) return rd; }
  if (!c->in_frame) return fail(c, PTC_E_STATE, "frame_set_adaptive: no frame");
  if (c->probe) return fail(c, PTC_E_STATE, "frame_set_adaptive: not available in a probe frame");
  if (c->integrator != PTC_INTEGRATOR_PATH) return fail(c, PTC_E_STATE, "frame_set_adaptive: the frame is not a PTC_INTEGRATOR_PATH frame");
  if (c->adaptive || c->samples_done || c->pending) return fail(c, PTC_E_STATE, "frame_set_adaptive: call it once, right after ptc_frame_begin, before any sample");
  if (c->resolve_divisor) return fail(c, PTC_E_STATE, "frame_set_adaptive: the frame has a resolve divisor (ptc_frame_set_sample_range)");
  ptc_adaptive_params p;
  ptc_adaptive_default_params(&p);
  if (params) p = *params;
  { int ra = adaptive_params_ok(c, p, "frame_set_adaptive"); if (ra) return ra; }
  const size_t n = c->owned_n, wh = (size_t)c->fr.w * (size_t)c->fr.h;
  int rc;
  for (int k = 0; k < 2; ++k) if ((rc = ensure_buf(c, c->ad_pix[k], n)) || (rc = ensure_buf(c, c->ad_slot[k], n))) return rc;
  if ((rc = ensure_buf(c, c->ad_mom, n)) || (rc = ensure_buf(c, c->ad_count, n)) || (rc = ensure_buf(c, c->ad_keep, n)) || (rc = ensure_buf(c, c->ad_flags, wh)) ||
      (rc = ensure_buf(c, c->ad_block, (size_t)pt_ad_blocks((uint32_t)n) + 1)) || (rc = ensure_buf(c, c->ad_n, 1))) return rc;
  const bool cov = c->cov_setting;
  if (cov && ((rc = ensure_buf(c, c->ad_cov4, n)) || (rc = ensure_buf(c, c->ad_cov2, n)))) return rc;
  for (hipEvent_t& e : c->ev_ad) if (!e) HIP_TRY(c, hipEventCreate(&e));
  hipStream_t s0 = c->lanes[0].stream;
  HIP_TRY(c, hipMemsetAsync(c->ad_mom.p, 0, (n ? n : 1) * sizeof(float2), s0));
  if (cov) {
    HIP_TRY(c, hipMemsetAsync(c->ad_cov4.p, 0, (n ? n : 1) * sizeof(float4), s0));
    HIP_TRY(c, hipMemsetAsync(c->ad_cov2.p, 0, (n ? n : 1) * sizeof(float2), s0));
  }
  HIP_TRY(c, hipMemsetAsync(c->ad_count.p, 0, (n ? n : 1) * sizeof(uint32_t), s0));
  HIP_TRY(c, hipMemsetAsync(c->ad_flags.p, 0, wh, s0));
  pt_launch_ad_init(s0, (uint32_t)n, c->owned.p, c->ad_pix[0].p, c->ad_slot[0].p);
  HIP_TRY(c, hipGetLastError());
  HIP_TRY(c, hipStreamSynchronize(s0));      // the other lanes read these arrays too
  c->ad_cur = 0; c->ad_passes = 0; c->ad_seconds = 0.0; c->ad_params = p;
  c->fr.owned = c->ad_pix[0].p;              // n_owned is the frame's: everything is active
  c->adaptive = true; c->cov_on = cov; c->cov_resolved = false; c->sv_valid = false;
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
  const int cur = c->ad_cur;
  uint32_t n_out = 0;
  HIP_TRY(c, hipEventRecord(c->ev_ad[0], s0));
  if (n >= (uint32_t)c->spp_total) {          // the budget is spent: everything stops; no pixel is active, so no flag stays set
    HIP_TRY(c, hipMemsetAsync(c->ad_flags.p, 0, (size_t)c->fr.w * (size_t)c->fr.h, s0));
  } else {
    pt_launch_ad_error(s0, n_in, c->ad_pix[cur].p, c->ad_slot[cur].p, ad, n, c->ad_params.threshold);
    pt_launch_ad_compact(s0, n_in, c->ad_pix[cur].p, c->ad_slot[cur].p, c->ad_pix[cur ^ 1].p, c->ad_slot[cur ^ 1].p, ad, c->fr.w, c->fr.h, c->ad_params.radius);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpyAsync(&n_out, c->ad_n.p, sizeof n_out, hipMemcpyDeviceToHost, s0));   // the host sizes the next launches by it
  }
  HIP_TRY(c, hipEventRecord(c->ev_ad[1], s0));
  HIP_TRY(c, hipStreamSynchronize(s0));
  { float ms = 0.0f; if (hipEventElapsedTime(&ms, c->ev_ad[0], c->ev_ad[1]) == hipSuccess) c->ad_seconds += 1e-3 * (double)ms; }
  if (n_out > n_in) return fail(c, PTC_E_DEVICE, "frame_adapt: the compaction returned more entries than it was given");
  c->ad_cur = cur ^ 1;
  c->fr.n_owned = n_out; c->fr.owned = c->ad_pix[c->ad_cur].p;
  c->per_batch = batch_samples(c, n_out, c->frame_batch_paths);      // as the set shrinks a pass still goes out as the fewest, widest launches
  c->ad_passes++;
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
    HIP_TRY(c, hipMemcpy(cnt.data(), c->ad_count.p, n * sizeof(uint32_t), hipMemcpyDeviceToHost));
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
  if (!cnt.empty()) HIP_TRY(c, hipMemcpy(cnt.data(), c->ad_count.p, cnt.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
  ptc_adaptive_stats s{};
  s.owned_pixels = c->owned_n; s.active_pixels = c->fr.n_owned; s.passes = c->ad_passes; s.seconds_adapt = c->ad_seconds;
  for (uint32_t v : cnt) { s.samples_total += v; if (v > s.max_count) s.max_count = v; }
  *out = s;
  return PTC_OK;
}

int ptc_set_sample_covariance(ptc_ctx* c, int on) {
  if (!c) return PTC_E_ARG;
  if (on != 0 && on != 1) return fail(c, PTC_E_ARG, "set_sample_covariance: 0 or 1");
  if (on == 1 && c->probe) return fail(c, PTC_E_STATE, "set_sample_covariance: a probe frame keeps no per-sample covariance (the setting is unchanged)");
  c->cov_setting = on == 1;
  return PTC_OK;
}

int ptc_read_sample_covariance(ptc_ctx* c, float* out) {
  { int rd = need_device(c); if (rd) return rd; }
  if (!out) return fail(c, PTC_E_ARG, "read_sample_covariance: null pointer");
  if (!c->in_frame || !c->adaptive || !c->cov_on) return fail(c, PTC_E_STATE, "read_sample_covariance: the frame is not an adaptive frame that keeps the sample covariance");
  { int rf = flush(c); if (rf) return rf; }
  { int rs = sync_all_lanes(c); if (rs) return rs; }
  const size_t n = c->owned_n;
  std::vector<uint32_t> pix(n);
  std::vector<float4> q4(n);
  std::vector<float2> q2(n);
  if (n) {
    HIP_TRY(c, hipMemcpy(pix.data(), c->owned.p, n * sizeof(uint32_t), hipMemcpyDeviceToHost));
    HIP_TRY(c, hipMemcpy(q4.data(), c->ad_cov4.p, n * sizeof(float4), hipMemcpyDeviceToHost));
    HIP_TRY(c, hipMemcpy(q2.data(), c->ad_cov2.p, n * sizeof(float2), hipMemcpyDeviceToHost));
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
  if (!c->sv_valid) return fail(c, PTC_E_STATE, "read_sampled_variance: no ptc_denoise_sampled in this frame");
  HIP_TRY(c, hipStreamSynchronize(c->lanes[0].stream));
  const size_t n = (size_t)c->rad_w * (size_t)c->rad_h;
  std::vector<float4> v(n);
  HIP_TRY(c, hipMemcpy(v.data(), c->sv_var.p, n * sizeof(float4), hipMemcpyDeviceToHost));
  for (size_t i = 0; i < n; ++i) { out[2 * i] = v[i].z; out[2 * i + 1] = v[i].w; }
  return PTC_OK;
}

int ptc_render_adaptive(ptc_ctx* c, int w, int h, int max_spp, uint64_t seed, int max_bounces, const ptc_adaptive_params* params) {
  { int rd = need_device(c); if (rd) return rd; }
  ptc_adaptive_params p;
  ptc_adaptive_default_params(&p);
  if (params) p = *params;
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
  if (c->comm) return fail(c, PTC_E_STATE, "comm_init: this context already has a communicator");
  if (!rccl_load()) return fail(c, PTC_E_DEVICE, g_rccl.err);
  ncclUniqueId uid;
  std::memcpy(uid.internal, id, PTC_COMM_ID_BYTES);
  NCCL_TRY(c, g_rccl.CommInitRank(&c->comm, n_ranks, uid, rank));
  c->comm_rank = rank; c->comm_size = n_ranks; c->comm_owned = true;
  return PTC_OK;
}

int ptc_comm_reduce_radiance(ptc_ctx* c, int root) {
  { int rd = need_device(c); if (rd) return rd; }
  if (c->probe) return fail(c, PTC_E_STATE, "comm_reduce_radiance: a probe frame is not a tile share of an image (shard probes by probe_index_base)");
  if (!c->comm) return fail(c, PTC_E_STATE, "comm_reduce_radiance: no communicator (ptc_comm_init / ptc_group_create)");
  if (root < 0 || root >= c->comm_size) return fail(c, PTC_E_ARG, "comm_reduce_radiance: bad root");
  if (!c->radiance.p || c->rad_w == 0) return fail(c, PTC_E_STATE, "comm_reduce_radiance: nothing rendered");
  // in place on stream 0, behind the resolve: ranks own disjoint tiles and hold zeros elsewhere, so the fp32 sum is x + 0
  ScopedSpan t(c, c->lanes[0].stream, 4);            // seconds_reduce: the collective as this rank's stream sees it (it includes waiting for the slowest rank)
  NCCL_TRY(c, g_rccl.Reduce(c->radiance.p, c->radiance.p, (size_t)c->rad_w * c->rad_h * 4, ncclFloat32, ncclSum, root, c->comm, c->lanes[0].stream));
  return PTC_OK;
}

int ptc_comm_destroy(ptc_ctx* c) {
  { int rd = need_device(c); if (rd) return rd; }
  if (!c->comm) return PTC_OK;
  if (!c->comm_owned) return fail(c, PTC_E_STATE, "comm_destroy: the communicator belongs to a ptc_group");
  { int rs = sync_all_lanes(c); if (rs) return rs; }
  NCCL_TRY(c, g_rccl.CommDestroy(c->comm));
  c->comm = nullptr; c->comm_size = 0;
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
    c->comm = g->comms[(size_t)i]; c->comm_rank = i; c->comm_size = n_devices; c->comm_owned = false;
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
  for (int i = 1; i < n; ++i) take_lights(g->ctx[(size_t)i], g->ctx[0]);
  for (int i = 0; i < n; ++i) { int rc = ptc_frame_begin(g->ctx[(size_t)i], w, h, spp, seed, max_bounces, integrator, i, n); if (rc) return bail(i, rc); }
  for (int i = 0; i < n; ++i) { int rc = ptc_frame_add_samples(g->ctx[(size_t)i], spp); if (rc) return bail(i, rc); }
  for (int i = 0; i < n; ++i) { int rc = ptc_frame_resolve(g->ctx[(size_t)i]); if (rc) return bail(i, rc); }
  if (n > 1) {
    ncclResult_t r = g_rccl.GroupStart();
    for (int i = 0; i < n && r == ncclSuccess; ++i) {
      ptc_ctx* c = g->ctx[(size_t)i];
      if (hipSetDevice(c->device) != hipSuccess) { g->err = "ptc_group_render: hipSetDevice failed"; (void)g_rccl.GroupEnd(); return PTC_E_DEVICE; }
      r = g_rccl.Reduce(c->radiance.p, c->radiance.p, (size_t)w * h * 4, ncclFloat32, ncclSum, 0, c->comm, c->lanes[0].stream);
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
  for (ptc_ctx* c : g->ctx) { if (c) { c->comm = nullptr; ptc_destroy(c); } }
  delete g;
}

// ---- test hooks -----------------------------------------------------------------------------------
int ptc_debug_trace_closest(ptc_ctx* c, const float* origins, const float* dirs, uint32_t n, float* out_t, int32_t* out_prim, float* out_uv) {
  if (!c) return PTC_E_ARG;
  if (c->device >= 0 && (!origins || !dirs || !out_t || !out_prim || !out_uv || n == 0)) return fail(c, PTC_E_ARG, "debug_trace_closest: bad argument");
  { int rc = debug_prepare(c, n, "debug_trace_closest"); if (rc) return rc; }
  const Lane& ln = c->lanes[0];
  std::vector<float4> A(n), B(n);
  for (uint32_t i = 0; i < n; ++i) {
    A[i] = make_float4(origins[i * 3], origins[i * 3 + 1], origins[i * 3 + 2], dirs[i * 3]);
    B[i] = make_float4(dirs[i * 3 + 1], dirs[i * 3 + 2], 0.0f, 0.0f);
  }
  HIP_TRY(c, hipMemcpy(ln.q.ray[0].A, A.data(), n * sizeof(float4), hipMemcpyHostToDevice));
  HIP_TRY(c, hipMemcpy(ln.q.ray[0].B, B.data(), n * sizeof(float4), hipMemcpyHostToDevice));
  const DevQueues q = batch_queues(c, 0, n);
  pt_launch_set_counts(ln.stream, c->cfg, q, n, 0);
  pt_launch_trace_closest(ln.stream, c->cfg, lane_scene(c, 0), q, 0, false);
  HIP_TRY(c, hipGetLastError());
  HIP_TRY(c, hipStreamSynchronize(ln.stream));
  std::vector<float4> H(n);
  HIP_TRY(c, hipMemcpy(H.data(), ln.q.hit, n * sizeof(float4), hipMemcpyDeviceToHost));
  for (uint32_t i = 0; i < n; ++i) {
    int32_t pc; std::memcpy(&pc, &H[i].y, 4);   // prim | class<<28, or -1
    out_t[i] = H[i].x; out_prim[i] = pc < 0 ? -1 : (pc & 0x0fffffff); out_uv[i * 2] = H[i].z; out_uv[i * 2 + 1] = H[i].w;
  }
  return PTC_OK;
}

int ptc_debug_trace_any(ptc_ctx* c, const float* origins, const float* dirs, const float* tmax, uint32_t n, uint8_t* out_occluded) {
  if (!c) return PTC_E_ARG;
  if (c->device >= 0 && (!origins || !dirs || !tmax || !out_occluded || n == 0)) return fail(c, PTC_E_ARG, "debug_trace_any: bad argument");
  { int rc = debug_prepare(c, n, "debug_trace_any"); if (rc) return rc; }
  const Lane& ln = c->lanes[0];
  std::vector<float4> A(n), B(n);
  for (uint32_t i = 0; i < n; ++i) {
    A[i] = make_float4(origins[i * 3], origins[i * 3 + 1], origins[i * 3 + 2], dirs[i * 3]);
    B[i] = make_float4(dirs[i * 3 + 1], dirs[i * 3 + 2], tmax[i], 0.0f);
  }
  HIP_TRY(c, hipMemcpy(ln.q.shadow.A, A.data(), n * sizeof(float4), hipMemcpyHostToDevice));
  HIP_TRY(c, hipMemcpy(ln.q.shadow.B, B.data(), n * sizeof(float4), hipMemcpyHostToDevice));
  uint8_t* d_out = nullptr;
  HIP_TRY(c, hipMalloc((void**)&d_out, n));
  const DevQueues q = batch_queues(c, 0, n);
  pt_launch_set_counts(ln.stream, c->cfg, q, 0, n);
  pt_launch_trace_any(ln.stream, c->cfg, lane_scene(c, 0), q, d_out);
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) e = hipStreamSynchronize(ln.stream);
  if (e == hipSuccess) e = hipMemcpy(out_occluded, d_out, n, hipMemcpyDeviceToHost);
  (void)hipFree(d_out);
  if (e != hipSuccess) return fail(c, PTC_E_DEVICE, std::string("debug_trace_any: ") + hipGetErrorString(e));
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
  float wi[3], Li[3], dist;
  if (!pt_light_sample(L, P, wi, dist, Li)) return 0;
  for (int k = 0; k < 3; ++k) { out_wi[k] = wi[k]; out_Li[k] = Li[k]; }
  *out_dist = dist;
  return 1;
}

int ptc_debug_get_light_table(ptc_ctx* c, uint32_t* n_lights, float* records, float* cdf) {
  if (!c) return PTC_E_ARG;
  std::vector<pt_light_rec> recs; std::vector<float> cd;
  pt_light_table(c->lights, recs, cd);
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
  if (c->lights.empty()) return fail(c, PTC_E_STATE, "debug_punctual_nee: no punctual light (ptc_add_light)");
  { int rc = upload_lights(c); if (rc) return rc; }
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
  const DevQueues q = batch_queues(c, 0, n);
  const DevScene sc = lane_scene(c, 0);
  pt_launch_set_counts(ln.stream, c->cfg, q, n, 0);
  pt_launch_trace_closest(ln.stream, c->cfg, sc, q, 0, false);
  pt_launch_shade_punctual(ln.stream, sc, q, 0, bounce, c->d_lights.p, c->d_light_cdf.p, c->n_lights_dev);
  HIP_TRY(c, hipGetLastError());
  HIP_TRY(c, hipStreamSynchronize(ln.stream));
  // the records lie at the front of each segment; a record says which ray it belongs to
  std::vector<uint32_t> seg_sh(q.n_seg);
  HIP_TRY(c, hipMemcpy(seg_sh.data(), q.seg_sh, (size_t)q.n_seg * 4, hipMemcpyDeviceToHost));
  const size_t slots = (size_t)q.n_seg * q.seg_len;
  std::vector<float4> SA(slots), SB(slots), SC(slots);
  HIP_TRY(c, hipMemcpy(SA.data(), q.shadow.A, slots * sizeof(float4), hipMemcpyDeviceToHost));
  HIP_TRY(c, hipMemcpy(SB.data(), q.shadow.B, slots * sizeof(float4), hipMemcpyDeviceToHost));
  HIP_TRY(c, hipMemcpy(SC.data(), q.shadow.C, slots * sizeof(float4), hipMemcpyDeviceToHost));
  std::memset(out_valid, 0, n);
  std::memset(out_origin, 0, (size_t)n * 12); std::memset(out_dir, 0, (size_t)n * 12); std::memset(out_tmax, 0, (size_t)n * 4); std::memset(out_contrib, 0, (size_t)n * 12);
  for (uint32_t sg = 0; sg < q.n_seg; ++sg) {
    if (seg_sh[sg] > q.seg_len) return fail(c, PTC_E_DEVICE, "debug_punctual_nee: a segment holds more shadow records than slots");
    for (uint32_t k = 0; k < seg_sh[sg]; ++k) {
      const size_t at = (size_t)sg * q.seg_len + k;
      uint32_t path; std::memcpy(&path, &SB[at].w, 4);
      if (path >= n || out_valid[path]) return fail(c, PTC_E_DEVICE, "debug_punctual_nee: a shadow record carries a path id that is out of range or taken");
      out_valid[path] = 1;
      out_origin[path * 3] = SA[at].x; out_origin[path * 3 + 1] = SA[at].y; out_origin[path * 3 + 2] = SA[at].z;
      out_dir[path * 3] = SA[at].w; out_dir[path * 3 + 1] = SB[at].x; out_dir[path * 3 + 2] = SB[at].y;
      out_tmax[path] = SB[at].z;
      out_contrib[path * 3] = SC[at].x; out_contrib[path * 3 + 1] = SC[at].y; out_contrib[path * 3 + 2] = SC[at].z;
    }
  }
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
  if (c->probe) return fail(c, PTC_E_STATE, "debug_camera_rays: a probe frame is in progress (its rays: ptc_debug_probe_rays)");
  const uint32_t n = n_pixels * n_samples;
  const uint32_t seed_hash = frame_seed_hash(seed);
  if (c->device < 0) {      // the host evaluation of pt_lens.h
    if (!c->have_cam) return fail(c, PTC_E_STATE, "debug_camera_rays: no camera (ptc_set_camera)");
    DevCamera cam;
    ptc_make_camera(c->cam_pos, c->cam_target, c->cam_fov, c->cam_aspect, cam);
    for (uint32_t p = 0; p < n; ++p) {
      uint32_t key;
      pt_lens_ray(cam, c->lens, w, h, seed_hash, pixels[p % n_pixels], first_sample + p / n_pixels, origins + (size_t)p * 3, dirs + (size_t)p * 3, key);
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
    const DevQueues q = batch_queues(c, 0, n);
    if (c->lens.aperture_radius > 0.0f) pt_launch_raygen_lens(ln.stream, c->cam, c->lens, fr, q, first_sample, n_samples);      // run_batch's choice
    else pt_launch_raygen(ln.stream, c->cam, fr, q, first_sample, n_samples, false);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipStreamSynchronize(ln.stream);
  if (e == hipSuccess) e = hipMemcpy(A.data(), ln.q.ray[0].A, (size_t)n * sizeof(float4), hipMemcpyDeviceToHost);
  if (e == hipSuccess) e = hipMemcpy(B.data(), ln.q.ray[0].B, (size_t)n * sizeof(float4), hipMemcpyDeviceToHost);
  list.release();      // the pixel list lives for this call only
  if (e != hipSuccess) return fail(c, PTC_E_DEVICE, std::string("debug_camera_rays: ") + hipGetErrorString(e));
  for (size_t p = 0; p < n; ++p) {
    origins[p * 3] = A[p].x; origins[p * 3 + 1] = A[p].y; origins[p * 3 + 2] = A[p].z;
    dirs[p * 3] = A[p].w; dirs[p * 3 + 1] = B[p].x; dirs[p * 3 + 2] = B[p].y;
  }
  return PTC_OK;
}

namespace {
// what the two probe hooks need of debug_prepare: a device, idle lanes, the frame ended, lane 0's queues for n paths.  No scene: neither kernel reads one.
int probe_debug_prepare(ptc_ctx* c, uint32_t n) {
  { int rd = need_device(c); if (rd) return rd; }
  { int rf = flush(c); if (rf) return rf; }
  { int rs = sync_all_lanes(c); if (rs) return rs; }
  c->in_frame = false; c->pending = 0; drop_guides(c);
  return ensure_lane_queues(c, n);
}
bool probe_debug_args_bad(int n, uint32_t base, uint32_t first_sample, uint32_t n_samples) {
  return n < 1 || n > PTC_MAX_PROBES || n_samples == 0 || (uint64_t)n * (uint64_t)n_samples > 0x7fffffffull || (uint64_t)first_sample + n_samples > 0x100000000ull ||
         (uint64_t)base + (uint64_t)n > 0x100000000ull;
}
}  // namespace

int ptc_debug_probe_rays(ptc_ctx* c, const float* positions_xyz, int n_probes, uint32_t probe_index_base, uint64_t seed, uint32_t first_sample, uint32_t n_samples,
                         float* out_o_d, uint32_t* out_key) {
  if (!c) return PTC_E_ARG;
  if (!positions_xyz || !out_o_d || !out_key || probe_debug_args_bad(n_probes, probe_index_base, first_sample, n_samples)) return fail(c, PTC_E_ARG, "debug_probe_rays: bad argument");
  const uint32_t np = (uint32_t)n_probes, n = np * n_samples;
  const uint32_t seed_hash = frame_seed_hash(seed);
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
  const uint32_t seed_hash = frame_seed_hash(seed);
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

}  // extern "C"
