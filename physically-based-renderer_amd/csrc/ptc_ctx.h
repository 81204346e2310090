// ptc_ctx.h — the private state of the C-ABI: what a context owns, and the helpers the ptc_api*.cpp files share.
//
// Private to ptc_api.cpp (context, lanes, batches, frames), ptc_api_scene.cpp (description, commit, refit, rebuild, deformation), ptc_api_image.cpp (guides, denoisers,
// temporal, adaptive, display, probes), ptc_api_lightmap.cpp (lightmaps), ptc_api_multi.cpp (RCCL, groups) and ptc_api_debug.cpp (the ptc_debug_* hooks).  It is not one of the kernel sources
// whose hash the library reports (ptc_build_info).
//
// Ownership is in the types: a DevBuf, a TreeBufs and a StageTimer free what they hold when they go, so `delete c` releases every feature's device memory and
// events — ptc_destroy makes the context's device current and waits for its streams first.  One struct per feature, each a member of ptc_ctx: the type's name says
// who owns a field.  Everything shared between the files lives in ptc_detail, which is hidden: none of it reaches the library's dynamic symbol table.
#pragma once
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
#include "pt_alpha.h"
#include "pt_glass.h"
#include "pt_glass_shadow.h"
#include "pt_display.h"
#include "pt_probes.h"
#include "pt_medium.h"
#include "pt_lightmap.h"
#include "pt_emissive_tex.h"
#include "pt_camera.h"

#include <rccl/rccl.h>

#include <chrono>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <memory>
#include <string>
#include <utility>
#include <vector>

#define PTC_MAX_PROBES (1 << 26)      // 9 lanes per probe and 27 sums per probe stay inside 32-bit indices

namespace ptc_detail __attribute__((visibility("hidden"))) {

int fail(ptc_ctx* c, int code, const std::string& msg);

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

struct Span { hipEvent_t a, b; int kind; };   // kind: 0 trace_closest, 1 trace_any, 2 shade, 3 whole batch, 4 the RCCL reduce, 5 an alpha resolution (alpha's own shadow walk included), 6 a glass resolution (the shadow walk of a frame with transparent shadows included), 7 the medium pass's kernels, 8 the textured-emission pass's kernel

// An array in HBM and its owner: freed when the owner goes (with the context: after ptc_destroy made the device current), or early by release()
template <class T> struct DevBuf {
  T* p = nullptr; size_t n = 0;
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  DevBuf(DevBuf&& o) noexcept : p(o.p), n(o.n) { o.p = nullptr; o.n = 0; }
  DevBuf& operator=(DevBuf&& o) noexcept { if (this != &o) { release(); p = o.p; n = o.n; o.p = nullptr; o.n = 0; } return *this; }
  ~DevBuf() { release(); }
  void release() { if (p) (void)hipFree(p); p = nullptr; n = 0; }
};

// The time of one stage on a stream: an event pair, created by the first begin(), and whether a pair of records has been queued
struct StageTimer {
  hipEvent_t start = nullptr, stop = nullptr;
  bool recorded = false;
  StageTimer() = default;
  StageTimer(const StageTimer&) = delete;
  StageTimer& operator=(const StageTimer&) = delete;
  ~StageTimer() { for (hipEvent_t e : {start, stop}) if (e) (void)hipEventDestroy(e); }
  int create(ptc_ctx* c);                           // the events, when they do not exist yet (begin does this; a caller that must act on a failure calls it first)
  int begin(ptc_ctx* c, hipStream_t st);
  int end(ptc_ctx* c, hipStream_t st);
  bool elapsed(double* out) const;                  // start .. stop in seconds, for a caller that has waited for the stream itself
  int seconds(ptc_ctx* c, double* out);             // 0.0 when nothing was recorded; else waits for the stop event
};

// A lane's side queue as a DevQueues view — continuation records in ray[0], their hit records, header words, segment counts and statistics of its own — and the
// flags k_trace_any writes for the shadow queue when a shadow walk goes through it
struct SideQueue { DevQueues q{}; uint8_t* flags = nullptr; std::vector<void*> allocs; };
// A lane's medium queue (pt_medium.h): the parked records of the scatter events and their per-segment counts, for `cap` paths
struct MediumQueue { DevMediumQ q{}; uint32_t cap = 0; std::vector<void*> allocs; };

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
  // alpha coverage (pt_alpha.h) and dielectric transmission (pt_glass.h): a side queue each, allocated only while the committed scene has such a material
  // (ensure_alpha_queues, ensure_glass_queues).  glass.flags only once a frame began with ptc_set_glass_shadows on (pt_glass_shadow.h)
  SideQueue alpha, glass;
  // the participating medium (pt_medium.h): allocated only once a frame runs with a medium on (ensure_medium_queues)
  MediumQueue medium;
  void free_overflow_slabs() { for (uint2* p : {stack_ovf, stack_ovf2}) if (p) (void)hipFree(p); stack_ovf = stack_ovf2 = nullptr; }
  void teardown();                  // ptc_destroy: everything but the overflow slabs (release_scene's), the streams after what ran on them
};

// The arrays of a tree in HBM: unit array, the refit's level list, the per-record node boxes, with their capacities (a rebuild writes into arrays large enough)
struct TreeBufs {
  float4* recs = nullptr; size_t recs_cap = 0; uint32_t* levels = nullptr; size_t levels_cap = 0; float* nbox = nullptr; size_t nbox_cap = 0;
  TreeBufs() = default;
  TreeBufs(const TreeBufs&) = delete;
  TreeBufs& operator=(const TreeBufs&) = delete;
  TreeBufs(TreeBufs&& o) noexcept { take(o); }
  TreeBufs& operator=(TreeBufs&& o) noexcept { if (this != &o) { release(); take(o); } return *this; }
  ~TreeBufs() { release(); }
  void release() { for (void* p : {(void*)recs, (void*)levels, (void*)nbox}) if (p) (void)hipFree(p); forget(); }
 private:
  void forget() { recs = nullptr; levels = nullptr; nbox = nullptr; recs_cap = levels_cap = nbox_cap = 0; }
  void take(TreeBufs& o) { recs = o.recs; recs_cap = o.recs_cap; levels = o.levels; levels_cap = o.levels_cap; nbox = o.nbox; nbox_cap = o.nbox_cap; o.forget(); }
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

// ---- one struct per feature -------------------------------------------------------------------------------------------------------------------

// punctual lights (pt_lights.h): `list` is what the calls recorded; the device table is what the last ptc_frame_begin uploaded of it, and what the frame's batches use
struct Lights {
  std::vector<ptc_light_params> list;
  bool dirty = false;               // `list` changed since the upload
  DevBuf<pt_light_rec> recs;
  DevBuf<float> cdf;
  uint32_t n_dev = 0;               // lights in the device table; 0: no punctual pass, nothing allocated
};

// alpha coverage (pt_alpha.h): mode / cutoff are what the calls recorded, by material id (shorter than the material list: the rest is OPAQUE); the device tables are
// those of the committed scene, built from its per-primitive material ids and uploaded by the first ptc_frame_begin (or ray hook) after the commit
struct Alpha {
  std::vector<int32_t> mode;
  std::vector<float> cutoff;
  int max_layers = PT_ALPHA_DEFAULT_LAYERS;   // a context setting: kept across ptc_scene_begin
  int frame_layers = PT_ALPHA_DEFAULT_LAYERS; // what the frame in progress (or the last ray hook) was begun with: a frame's batches all queue the same rounds
  bool dirty = true;                // the committed scene's tables are not on the device yet
  uint32_t n_prims = 0;             // primitives of the committed scene whose material is not OPAQUE, as of the last upload; 0: no pass, no queue, nothing allocated
  DevBuf<uint32_t> bits;
  DevBuf<float2> mode_cutoff;
  DevBuf<unsigned long long> counters;
  double seconds = 0.0;             // the frame's alpha resolutions (spans of kind 5)
};

// dielectric transmission (pt_glass.h): params are what the calls recorded, by material id (shorter than the material list: the rest is not transmissive); the device
// tables are those of the committed scene, built from its per-primitive material ids and uploaded by the first ptc_frame_begin (or ray hook) after the commit
struct Glass {
  std::vector<ptc_transmission_params> params;
  int max_interactions = PT_GLASS_DEFAULT_INTERACTIONS;     // a context setting: kept across ptc_scene_begin
  int frame_interactions = PT_GLASS_DEFAULT_INTERACTIONS;   // what the frame in progress (or the last ray hook) was begun with
  bool dirty = true;                // the committed scene's tables are not on the device yet
  uint32_t n_prims = 0;             // primitives of the committed scene whose material has tau > 0, as of the last upload; 0: no pass, no queue, nothing allocated
  DevBuf<uint32_t> bits;
  DevBuf<float4> mats;
  DevBuf<unsigned long long> counters;
  double seconds = 0.0;             // the frame's glass resolutions (spans of kind 6)
  // transparent shadows (pt_glass_shadow.h)
  int shadows = 0;                  // ptc_set_glass_shadows: a context setting, kept across ptc_scene_begin
  int frame_shadows = 0;            // what the frame in progress (or the last ray hook) was begun with
  uint32_t n_thin = 0;              // primitives of the committed scene whose material is transmissive AND thin-walled, as of the last upload; 0: no shadow walk
  DevBuf<unsigned long long> shadow_counters;
};

// the participating medium (pt_medium.h): `params` is what the calls recorded (set: there is one), with the lifetime of the punctual lights; `frame` is what the
// frame in progress (or the last ptc_debug_medium_step) was begun with, frame_on whether its batches launch the pass.  Nothing is allocated before that
struct Medium {
  bool set = false;
  ptc_medium_params params{};
  bool frame_on = false;
  pt_medium frame{};
  DevBuf<unsigned long long> counters;
  double seconds = 0.0;             // the frame's medium kernels (spans of kind 7)
};

// textured emission (pt_emissive_tex.h): `mats` is what the calls recorded, by material id (shorter than the material list: the rest has none).  `table` is the
// committed scene's, built by the commit and placed anew by every refit and rebuild from these primitives' vertices alone — a description-only context has it too;
// the device copies follow it (emtex_upload: ptc_frame_begin or a ray hook, every lane idle).  Nothing is allocated while the table is empty
struct EmTex {
  std::vector<pt_emtex_material> mats;
  pt_emtex_table table;
  bool dirty = false;               // the table changed since the upload
  uint32_t n_dev = 0;               // entries in the device table; 0: no pass
  DevBuf<pt_emtex_rec> recs;
  DevBuf<float> cdf;
  DevBuf<int32_t> prim_map;
  DevBuf<unsigned long long> counters;
  double seconds = 0.0;             // the frame's launches of the pass (spans of kind 8)
};

// display transform (pt_display.h): the parameters are a context setting; the histogram (4096 bins + the rejected count) and the state record live in HBM,
// allocated by the first call that needs them.  Nothing here is touched by a context that never calls the display functions
struct Display {
  ptc_display_params params{1.0f, 0, 0.18f, 0.1f, 0.9f, 1.0f, 1e-4f, 1e6f, PTC_TONEMAP_ACES, 4.0f, PTC_OETF_GAMMA22};
  DevBuf<uint32_t> hist, ldr;
  DevBuf<pt_display_state> state;
  DevBuf<uint2> half;
  StageTimer t_meter, t_display;    // the last metering, the last display kernel
};

// the first-hit guides of the current frame (k_guides)
struct Guides {
  DevBuf<float4> albedo, normal, pos;
  DevBuf<int32_t> prim;
  DevBuf<float2> uv;
  DevBuf<unsigned long long> stats;   // the guide rays' traversal counters: kept apart from the frame's (ptc_stats counts samples only)
  bool valid = false;
  StageTimer timer;                   // the last guide pass
  GuideBufs dev() const { return GuideBufs{albedo.p, normal.p, pos.p, prim.p, uv.p}; }      // what the kernels take
};

// the à-trous filter's two (colour, variance) buffers and the denoised image
struct Denoise {
  DevBuf<float4> cv[2], denoised;
  bool valid = false;
  StageTimer timer;                   // the last denoise
};

// adaptive sampling (pt_adaptive.hip).  In an adaptive frame `fr` describes the ACTIVE pixels (n_owned = their number, owned = pix[cur]): that is all the
// path kernels see of a frame; the frame's own pixels stay in owned / owned_n, where the sums, the moments and the counts live.
struct Adaptive {
  bool on = false;
  ptc_adaptive_params params{};
  DevBuf<uint32_t> pix[2], slot[2], count, block, n;   // the active list (pixel, owned position), ping-pong: a decision step compacts one into the other
  DevBuf<float2> mom;
  DevBuf<uint8_t> flags, keep;
  int cur = 0;
  uint32_t passes = 0;
  double seconds = 0.0;
  StageTimer timer;                 // one decision step
  // the per-sample RGB covariance: cov_setting is the context's (ptc_set_sample_covariance), cov_on what the current adaptive frame was begun with
  bool cov_setting = false, cov_on = false;
  bool cov_resolved = false;        // the radiance buffer holds the resolve of every sample the frame's sums hold
  bool sv_valid = false;            // sv_var holds the current frame's last ptc_denoise_sampled variance
  DevBuf<float4> cov4, sv_colour, sv_var;   // (rr, gg, bb, rg) per owned pixel; the filter's input (D, n) and (0, 0, Var_s, 1 / n) per pixel
  DevBuf<float2> cov2;                      // (rb, gb) per owned pixel
};

// temporal accumulation (pt_temporal.hip).  The history is the state the last ptc_temporal_accumulate left: set `cur` of the two ping-pong sets, the camera and
// the size of its frame.  It outlives frames, cameras, refits and rebuilds; the accumulated image is the current frame's (drop_guides ends its validity).
struct Temporal {
  DevBuf<float4> dn[2], mom[2], nz[2], pk[2], motion, accum;
  DevBuf<float4> snap;              // the position snapshot: 3 x float4 per primitive as the shading records held them when the history was written
  bool snap_current = false;        // false: the shading records in HBM still are those of the history's frame (nothing moved since), the snapshot is not needed;
                                    // true: a refit or rebuild came after the history, snap holds the positions it was about to overwrite
  bool live = false;                // there is a history
  int cur = 0, w = 0, h = 0, demodulate = 0;
  DevCamera cam{};
  bool accum_valid = false;         // the current frame has been accumulated: accum holds its accumulated image
  StageTimer timer;                 // the last accumulate
};

// light probes (pt_probes.h).  A probe frame is a frame of n x 1 "pixels" — `fr`, accum, radiance, the batching and the sample range are the frame's own — whose
// batches start at k_raygen_probe and end with k_accumulate_sh beside k_accumulate.  The flag lives as long as the frame does (drop_guides ends it).
struct Probes {
  bool on = false;
  uint32_t base = 0;                // index of probe 0 in the RNG key (ptc_probes_begin: probe_index_base)
  DevBuf<float4> pos;               // (x, y, z, -) per probe
  DevBuf<float> acc;                // 27 running sums per probe, [probe][k][rgb]
};

// lightmaps (pt_lightmap.h).  A lightmap frame is a frame of n x 1 "pixels", the covered texels of the atlas in ascending atlas index — `fr`, accum, radiance, the
// batching and the sample range are the frame's own — whose batches start at k_raygen_texel, count back-face first hits at bounce 0 and end with k_accumulate
// alone.  The flag lives as long as the frame does (drop_guides ends it).  Nothing here is allocated by a context that never bakes
struct Lightmap {
  bool on = false;
  int w = 0, h = 0;
  uint32_t base = 0;                // index of texel 0 in the RNG key (ptc_lightmap_desc: texel_index_base)
  uint32_t n = 0, dropped = 0;      // entries of the list; owned texels dropped for a degenerate world triangle
  DevBuf<float4> texels;            // two per entry: (origin, atlas index bits) (normal, primitive bits)
  DevBuf<uint32_t> back;            // per entry: samples whose first hit was a back face
  DevBuf<float4> atlas[2];          // the resolve's target and the dilation's ping-pong
  DevBuf<float> fraction;           // ptc_lightmap_read's out_backface
  // the texel-list build: the owner image, the compaction's scratch, the list; the instance's geometry when it comes from the host build
  DevBuf<uint32_t> owner, block, counts, list, idx;
  DevBuf<uint8_t> flags;
  DevBuf<float> uv;
  DevBuf<HostVertex> verts;
};

// multi-GPU
struct Comm {
  ncclComm_t handle = nullptr;
  int rank = 0, size = 0;
  bool owned = true;                // false: the communicator belongs to a ptc_group
};

// RCCL, loaded on first use (a renderer that never reduces does not need librccl at load time)
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
extern Rccl g_rccl;                     // ptc_api_multi.cpp (rccl_load); ptc_destroy destroys a context's communicator through it
extern std::string g_create_error;      // ptc_api.cpp: what ptc_last_error(NULL) serves

}  // namespace ptc_detail

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
  bool cam_ex_set = false;            // the camera in force is ptc_set_camera_ex's (include/ptc_camera.h): its matrix and projection instead of the look-at above
  ptc_camera_params cam_ex{};         // as it was set; ptc_set_camera and ptc_scene_begin drop it
  ptc_lens_params lens{0.0f, 1.0f, 0, 0.0f};   // the camera's lens (ptc_set_camera_lens): kept across ptc_set_camera, reset by ptc_scene_begin; R = 0: the pinhole, k_raygen
  ptc_detail::Lights lights;
  ptc_detail::Alpha alpha;
  ptc_detail::Glass glass;
  ptc_detail::Medium medium;
  ptc_detail::EmTex emtex;
  int tex_linear = 0;                    // PTC_FILTER_*: texture filter of the scene being described
  int bvh_default = PTC_BVH_SAH;         // PTC_BVH_*: builder a new scene description starts with (PTC_BVH=lbvh in the environment changes it)
  int bvh_builder = PTC_BVH_SAH;         // builder of the scene being described
  int device_builder = PTC_BVH_LBVH;     // PTC_BVH_*: the tree a build ON THE DEVICE makes (ptc_set_device_builder; PTC_DEVICE_BVH=sah in the environment), kept across ptc_scene_begin
  // committed scene
  bool committed = false;
  std::shared_ptr<HostBuilt> built = std::make_shared<HostBuilt>();   // the host build; the contexts of a ptc_group share one (ptc_group_scene_commit)
  ptc_detail::CommittedScene scene;
  std::vector<ptc_detail::MeshPose> poses;      // deformation state by mesh id (may be shorter than meshes: plain meshes at the end have none)
  DevCamera cam{};
  bool debug_verts_from_device = false;      // the last ptc_debug_get_mesh_vertices read the mesh's slice in HBM (ptc_debug_get_internals[7] bit 3)
  int refit_on_device = 1;          // PTC_REFIT=host: ptc_scene_refit recomputes on the host and uploads (the round-3a path, kept as the cross-check)
  int trace_rays_per_lane = 8;      // PTC_TRACE_RAYS_PER_LANE: rays per lane of the trace kernels' grid a batch should offer before the grid is made smaller (run_batch)
  int trace_overlap = 1;            // PTC_TRACE_OVERLAP: the shadow rays of bounce b are traced on the lane's second stream beside the closest-hit launch of bounce b + 1 (they are
                                    // independent; k_shade(b + 1) waits for both).  1 (default) = batches of up to 2^26 paths, whose launches do not keep the chip full for long:
                                    // -5 % .. -17 % frame time from 16 spp down to 1 spp at 1080p (profiles/r03_viewer_loop.txt); 2 = every batch (+0.4 % at the benchmark's
                                    // batch size, but the two kernels' launch durations then include each other: not the default, so that what bench.py and rocprofv3 time
                                    // per kernel stays a kernel's own time); 0 = never
  BuildScratch bscratch;            // device scratch of ptc_scene_rebuild (pt_build.hip), grow-only; ptc_destroy frees it
  // lanes: lane 0 is the context's primary stream (resolve, tonemap, conversions, the reduce)
  std::vector<ptc_detail::Lane> lanes;
  int n_lanes = 1;                  // PTC_LANES: >1 runs successive batches on separate streams.  With the round-2 kernels one lane
                                    // is 3.7 % faster than two (co-scheduled launches slow each other down by more than the tails they fill)
  uint64_t batches_issued = 0;
  int path_order = PT_ORDER_PIXEL;  // PTC_PATH_ORDER=sample|pixel: how a camera frame of the path integrator numbers a batch's paths (pt_device.h, pt_path_id).  Pixel-major:
                                    // a wave of bounce 0 carries 64 samples of one pixel instead of one sample of 64 pixels; the image is the same bit for bit
                                    // (profiles/path_order.txt has the A/B that chose the default)
  // frame
  bool in_frame = false;
  DevFrame fr{};
  int spp_total = 0, integrator = 0;
  uint32_t samples_done = 0;        // samples issued to the device
  uint32_t sample_base = 0;         // index of the frame's first sample (ptc_frame_set_sample_range / ptc_frame_restore): sample k of the frame has index sample_base + k
  uint32_t resolve_divisor = 0;     // 0: the resolve divides by the samples accumulated; else by this (sample-range sharding: partial means that sum to the mean)
  uint32_t pending = 0;             // samples accepted by frame_add_samples and not yet issued (deferred batching)
  uint32_t per_batch = 1;           // samples of one full batch = max_batch_paths / owned pixels / lanes
  size_t frame_batch_paths = 0;     // the path budget of a batch as ptc_frame_begin settled it: per_batch follows the active set from it
  ptc_detail::DevBuf<uint32_t> owned;
  bool owned_key_valid = false;     // c->owned holds the list for (owned_w, owned_h, owned_rank, owned_count)
  int owned_w = 0, owned_h = 0, owned_rank = 0, owned_count = 0;
  uint32_t owned_n = 0;
  ptc_detail::DevBuf<float4> accum, radiance;
  ptc_detail::DevBuf<uint32_t> ldr;
  ptc_detail::DevBuf<uint2> half;   // RGBA16F copy of the radiance buffer
  int rad_w = 0, rad_h = 0;
  int output = PTC_OUTPUT_RADIANCE; // which image the read-backs serve (ptc_select_output, served_image)
  // what the image-space features keep (ptc_api_image.cpp); ptc_api_multi.cpp's communicator
  ptc_detail::Guides guides;
  ptc_detail::Denoise denoise;
  ptc_detail::Adaptive adaptive;
  ptc_detail::Temporal temporal;
  ptc_detail::Display display;
  ptc_detail::Probes probes;
  ptc_detail::Lightmap lightmap;
  ptc_detail::Comm comm;
  // stats
  ptc_stats stats{};
  std::vector<ptc_detail::Span> spans;
  std::vector<hipEvent_t> free_events;
  size_t events_created = 0;
};

struct ptc_group {
  std::vector<ptc_ctx*> ctx;
  std::vector<ncclComm_t> comms;
  std::string err;
};

namespace ptc_detail __attribute__((visibility("hidden"))) {

inline int fail(ptc_ctx* c, int code, const std::string& msg) { if (c) c->err = msg; return code; }
inline const char* const kNoDevice = "this context has no device (PTC_DEVICE_NONE): the call needs a gfx950 GPU; there is no CPU path";
inline const char* const kDescriptionChanged = "scene_refit: the scene's meshes or instances changed since the commit (only transforms may)";

// the temporal history is about the primitive ids of one committed scene: whatever brings another scene (ptc_scene_begin; every kind of commit, through
// commit_upload(Upload::NewScene)) ends it, and with it the position snapshot's claim to be current.  Refits and rebuilds keep the ids and the history.
inline void drop_history(ptc_ctx* c) { c->temporal.live = false; c->temporal.snap_current = false; }
// the frame is over or the scene changed: its guides and its denoised image go with it, the read-backs serve the radiance again
inline void drop_guides(ptc_ctx* c) { c->probes.on = false; c->lightmap.on = false; c->guides.valid = false; c->denoise.valid = false; c->temporal.accum_valid = false; c->output = PTC_OUTPUT_RADIANCE; }
// the image ptc_read_radiance_rgba32f / _rgba16f / ptc_tonemap_rgba8 serve (ptc_select_output)
// a frame whose "pixels" are a list of entries — probes, or the texels of a lightmap — and no image: what has no meaning without a camera image refuses it
inline bool entry_frame(const ptc_ctx* c) { return c->probes.on || c->lightmap.on; }
inline const float4* served_image(const ptc_ctx* c) {
  return c->output == PTC_OUTPUT_DENOISED ? c->denoise.denoised.p : c->output == PTC_OUTPUT_ACCUMULATED ? c->temporal.accum.p : c->radiance.p;
}

inline int need_device(ptc_ctx* c) {
  if (!c) return PTC_E_ARG;
  if (c->device < 0) return fail(c, PTC_E_DEVICE, kNoDevice);
  HIP_TRY(c, hipSetDevice(c->device));
  return PTC_OK;
}

template <class T> int ensure_buf(ptc_ctx* c, DevBuf<T>& b, size_t n) {
  if (b.n >= n && b.p) return PTC_OK;
  b.release();
  HIP_TRY(c, hipMalloc((void**)&b.p, (n ? n : 1) * sizeof(T)));
  b.n = n;
  return PTC_OK;
}

// arrays whose owner is a list of allocations (the committed scene's, a lane's queues)
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
inline void free_all(std::vector<void*>& v) { for (void* p : v) (void)hipFree(p); v.clear(); }

// the parameters of a call: the defaults, or what the caller passed
template <class P> P with_defaults(const P* params, void (*defaults_fn)(P*)) {
  P p;
  defaults_fn(&p);
  if (params) p = *params;
  return p;
}

inline int StageTimer::create(ptc_ctx* c) {
  for (hipEvent_t* ev : {&start, &stop}) { hipEvent_t& e = *ev; if (!e) HIP_TRY(c, hipEventCreate(&e)); }
  return PTC_OK;
}
inline int StageTimer::begin(ptc_ctx* c, hipStream_t st) {
  { int rc = create(c); if (rc) return rc; }
  HIP_TRY(c, hipEventRecord(start, st));
  return PTC_OK;
}
inline int StageTimer::end(ptc_ctx* c, hipStream_t st) {
  HIP_TRY(c, hipEventRecord(stop, st));
  recorded = true;
  return PTC_OK;
}
inline bool StageTimer::elapsed(double* out) const {
  float ms = 0.0f;
  if (hipEventElapsedTime(&ms, start, stop) != hipSuccess) return false;
  *out = 1e-3 * (double)ms;
  return true;
}
inline int StageTimer::seconds(ptc_ctx* c, double* out) {
  if (!out) return PTC_OK;
  *out = 0.0;
  if (!recorded) return PTC_OK;
  HIP_TRY(c, hipEventSynchronize(stop));
  float ms = 0.0f;
  HIP_TRY(c, hipEventElapsedTime(&ms, start, stop));
  *out = 1e-3 * (double)ms;
  return PTC_OK;
}

// ---- ptc_api.cpp: lanes, batches, frames -------------------------------------------------------------------------------------------------------
int sync_all_lanes(ptc_ctx* c);
int ensure_lane_queues(ptc_ctx* c, uint32_t cap);
hipEvent_t next_event(ptc_ctx* c);
DevScene lane_scene(ptc_ctx* c, int l);
DevQueues batch_queues(ptc_ctx* c, int l, uint32_t n);
LaunchCfg batch_cfg(const ptc_ctx* c, uint32_t n_paths);
uint32_t batch_samples(const ptc_ctx* c, size_t n_pixels, size_t batch_paths);
int flush(ptc_ctx* c);
int join_lanes_on_stream0(ptc_ctx* c);
int sum_lane_stats(ptc_ctx* c, unsigned long long st[ST_N]);
// a frame over a list of w entries instead of an image (h = 1, the path integrator, no tiles): probes at probe_pos (3 floats each), or — probe_pos == nullptr — the
// texel list the lightmap state holds (w may be 0: nothing is covered); base: the index of entry 0 in the RNG key; who: the entry the caller used, for ptc_last_error
struct FrameEntries { const char* who; const float* probe_pos; uint32_t base; };
int frame_begin(ptc_ctx* c, int w, int h, int spp_total, uint64_t seed, int max_bounces, int integrator, int tile_rank, int tile_count, const FrameEntries* entries);

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

// The read-backs of a whole image share this: the device, `out`, the call's own checks (`source` returns an error or sets the image in HBM), wait, copy
// rad_w x rad_h elements.  all_lanes: wait for every lane — else for lane 0, on which everything behind the resolve is queued.
template <class Source> int read_image(ptc_ctx* c, const char* who, void* out, size_t elem_bytes, bool all_lanes, Source source) {
  { int rd = need_device(c); if (rd) return rd; }
  if (!out) return fail(c, PTC_E_ARG, std::string(who) + ": null pointer");
  const void* src = nullptr;
  { int rc = source(src); if (rc) return rc; }
  if (all_lanes) { int rs = sync_all_lanes(c); if (rs) return rs; }
  else HIP_TRY(c, hipStreamSynchronize(c->lanes[0].stream));
  HIP_TRY(c, hipMemcpy(out, src, (size_t)c->rad_w * c->rad_h * elem_bytes, hipMemcpyDeviceToHost));
  return PTC_OK;
}

// ---- ptc_api_scene.cpp: what the group calls and the debug hooks use of the description, the commit and the refit ----------------------------------
// what a commit_upload is for: a commit brings new primitive ids (the temporal history goes), a refit or rebuild that has to lay the arrays out anew keeps them
enum class Upload { NewScene, SameScene };
void release_scene(ptc_ctx* c);
int upload_lights(ptc_ctx* c);
void take_lights(ptc_ctx* c, const ptc_ctx* c0);
const char* lens_params_error(const ptc_lens_params& p);
void deform_host_all(ptc_ctx* c);
int deform_after_host_refit(ptc_ctx* c);
void deform_take(ptc_ctx* c, const ptc_ctx* c0, bool with_verts);
bool description_matches_commit(const ptc_ctx* c);
void copy_description(ptc_ctx* c, const ptc_ctx* c0);
bool refit_on_device(ptc_ctx* c);
int refit_upload(ptc_ctx* c, bool same_sizes, std::chrono::steady_clock::time_point t0);
int device_refit(ptc_ctx* c, std::chrono::steady_clock::time_point t0);
int commit_upload(ptc_ctx* c, std::chrono::steady_clock::time_point t0, Upload what, bool skeleton = false);
int scene_commit(ptc_ctx* c, bool device_ok);

// ---- ptc_api_alpha.cpp: alpha coverage (pt_alpha.h) ------------------------------------------------------------------------------------------------
int alpha_upload(ptc_ctx* c);                          // the committed scene's tables -> device memory, when a commit came since (every lane idle)
inline bool alpha_on(const ptc_ctx* c) { return c->alpha.n_prims > 0; }
inline DevAlpha dev_alpha(const ptc_ctx* c) { return DevAlpha{c->alpha.bits.p, c->alpha.mode_cutoff.p, (uint32_t)c->alpha.frame_layers, c->alpha.counters.p}; }
int ensure_side_queues(ptc_ctx* c, SideQueue Lane::*side, bool with_flags);      // what the two ensure_*_queues share
int ensure_alpha_queues(ptc_ctx* c);                   // every lane: an alpha queue as large as its queues (grow only; waits for the work in flight first)
void alpha_resolve_closest(ptc_ctx* c, int l, hipStream_t st, const LaunchCfg& cfg, const DevScene& sc, const DevQueues& q, int qi, uint32_t bounce, int form, uint32_t* layers_out);

// the lane's side queue with the segment layout of the batch whose queues are q
inline DevQueues side_view(const SideQueue& side, const DevQueues& q) {
  DevQueues sq = side.q;
  sq.lpath = q.lpath;
  sq.n_seg = q.n_seg; sq.seg_len = q.seg_len;
  return sq;
}
// The host cannot know how many records go on without a read-back, so a resolution queues every round it may need: filter(first), then rounds x (scan, trace,
// between(r), filter(later)) on the side-queue view.  A round with nothing left is launches that find their queue empty.
template <class Filter, class Between>
void resolve_rounds(hipStream_t st, const LaunchCfg& cfg, const DevScene& sc, const DevQueues& view, uint32_t rounds, Filter filter, Between between) {
  filter(/*first=*/true);
  for (uint32_t r = 0; r < rounds; ++r) {
    pt_launch_scan(st, cfg, view, 0);
    pt_launch_trace_closest(st, cfg, sc, view, 0, false);
    between(r);
    filter(/*first=*/false);
  }
}

// ---- ptc_api_glass.cpp: dielectric transmission (pt_glass.h) ---------------------------------------------------------------------------------------
int glass_upload(ptc_ctx* c);                          // the committed scene's tables -> device memory, when a commit came since (every lane idle)
inline bool glass_on(const ptc_ctx* c) { return c->glass.n_prims > 0; }
inline float glass_tau(const ptc_ctx* c, int material) { return (size_t)material < c->glass.params.size() ? c->glass.params[(size_t)material].transmission : 0.0f; }
int ensure_glass_queues(ptc_ctx* c);                   // every lane: a glass queue as large as its queues, with flag bytes when the frame has transparent shadows (grow only; waits for the work in flight first)
void glass_resolve_closest(ptc_ctx* c, int l, hipStream_t st, const LaunchCfg& cfg, const DevScene& sc, const DevQueues& q, int qi, uint32_t bounce, uint32_t* j_out);
// transparent shadows (pt_glass_shadow.h): the frame walks its shadow records through thin panes — the feature is on and the scene has a thin transmissive primitive
inline bool glass_shadows_on(const ptc_ctx* c) { return c->glass.frame_shadows != 0 && c->glass.n_thin > 0; }
// the shadow queue of q, counted and scanned, resolved to an RGB transmittance per record: k_trace_any's flags, then the walk (pt_glass_shadow.h).  through_glass: a
// frame with transparent shadows — the glass queue, alpha and glass tables, a span of kind 6; else alpha's own walk — the alpha queue, no glass table, kind 5.
// tr3_out / layers_out (or null): the debug hooks' outputs instead of the additions to lpath
void resolve_shadow(ptc_ctx* c, int l, hipStream_t st, const LaunchCfg& cfg, const DevScene& sc, const DevQueues& q, bool through_glass, float* tr3_out, uint32_t* layers_out);

// ---- ptc_api_medium.cpp: the participating medium (pt_medium.h) ----------------------------------------------------------------------------------------
inline bool medium_on(const ptc_ctx* c) { return c->medium.frame_on; }
inline void take_medium(ptc_ctx* c, const ptc_ctx* c0) { c->medium.set = c0->medium.set; c->medium.params = c0->medium.params; }
// the frame about to begin would run the medium pass over a scene whose committed primitives have alpha coverage or transmission: the message, else nullptr.
// Decided from the description and the host build, so a description-only context can tell
const char* medium_conflict(const ptc_ctx* c, int integrator);
int medium_frame_begin(ptc_ctx* c, bool on);           // the frame's copy of the parameters, the counters allocated and cleared when it is on (every lane idle)
int ensure_medium_queues(ptc_ctx* c);                  // every lane: a medium queue as large as its queues (grow only; waits for the work in flight first)
inline DevMediumQ dev_medium_q(const ptc_ctx* c, int l) { DevMediumQ m = c->lanes[(size_t)l].medium.q; m.counters = c->medium.counters.p; return m; }

// ---- ptc_api_camera.cpp: camera models (pt_camera.h) ------------------------------------------------------------------------------------------------------
// the DevCamera of the camera in force: the extended camera's basis, or ptc_make_camera of the stored look-at.  Every place that (re)makes c->cam calls this
void make_camera_in_force(const ptc_ctx* c, DevCamera& cam);
inline int cam_projection(const ptc_ctx* c) { return c->cam_ex_set ? c->cam_ex.projection : PTC_PROJ_PERSPECTIVE; }
inline PtCamProj cam_proj(const ptc_ctx* c) { return PtCamProj{cam_projection(c), c->cam_ex.xmag, c->cam_ex.ymag}; }
inline void take_camera_ex(ptc_ctx* c, const ptc_ctx* c0) { c->cam_ex_set = c0->cam_ex_set; c->cam_ex = c0->cam_ex; }
// what serves the perspective projection alone, asked under another: "<who>: ... PTC_PROJ_<name> ...", else empty.  Needs no device
std::string projection_refusal(const ptc_ctx* c, const char* who, const char* what);

// ---- ptc_api_emissive_tex.cpp: textured emission (pt_emissive_tex.h) ------------------------------------------------------------------------------------
inline bool emtex_has(const ptc_ctx* c, int material) { return (size_t)material < c->emtex.mats.size() && c->emtex.mats[(size_t)material].tex >= 0; }
void emtex_commit(ptc_ctx* c);                         // the table of the scene just committed (fixed part and placement); c->built holds its textures
void emtex_place(ptc_ctx* c);                          // a refit or rebuild went through: geometry, areas, pmf and cdf of the description's current transforms and poses
int emtex_upload(ptc_ctx* c);                          // the table -> device memory, when it changed (every lane idle); the counters cleared
inline bool emtex_on(const ptc_ctx* c) { return c->emtex.n_dev > 0; }
inline DevEmTex dev_emtex(const ptc_ctx* c) {
  return DevEmTex{(const float4*)c->emtex.recs.p, c->emtex.cdf.p, c->emtex.prim_map.p, c->emtex.n_dev, c->emtex.table.total > 0.0f ? 1 : 0, c->emtex.counters.p};
}
const char* emtex_medium_conflict(const ptc_ctx* c, int integrator);      // a medium together with emission textures: the message, else nullptr

// ---- ptc_api_debug.cpp: what the ray hooks of the three files share ----------------------------------------------------------------------------------
// a device, the committed scene, idle lanes, the frame ended, lane 0's queues for n paths, the counters cleared; with DebugAlpha the alpha tables, queues and counters
// of the committed scene and the frame settings a ray hook runs with, with DebugAlphaGlass those of the glass pass and of transparent shadows as well
enum DebugFeatures { DebugPlain = 0, DebugAlpha = 1, DebugAlphaGlass = 2 };
int debug_prepare(ptc_ctx* c, uint32_t n, const char* who, DebugFeatures features = DebugPlain);
// n explicit rays into a queue of lane 0: A = (o, d.x), B = (d.y, d.z, ..), C; fill(i, B, C) supplies B.zw and C of ray i (C starts as zero)
typedef std::function<void(uint32_t i, float4& B, float4& C)> RayFill;
inline RayQ as_rays(const ShadowQ& s) { return RayQ{s.A, s.B, s.C}; }      // the shadow queue's three arrays, for the two helpers that take either queue
int stage_rays(ptc_ctx* c, const RayQ& rq, uint32_t n, const float* origins, const float* dirs, const RayFill& fill);
// lane 0's first n hit records as (t, prim or -1, uv)
int read_hits(ptc_ctx* c, uint32_t n, float* out_t, int32_t* out_prim, float* out_uv);
// the records of rq lie at the front of each segment of q (seg_counts: device, per segment) and say which of the n paths they belong to (path_of): sink(path, A, B, C) for
// each; a count above seg_len or a path id out of range or taken is an error about "<what> records"
typedef std::function<void(uint32_t path, const float4& A, const float4& B, const float4& C)> RecordSink;
int scatter_segment_records(ptc_ctx* c, const DevQueues& q, const uint32_t* seg_counts, const RayQ& rq, uint32_t (*path_of)(const float4& B, const float4& C), uint32_t n,
                            const char* who, const char* what, const RecordSink& sink);

// ---- ptc_api_debug.cpp: the host's copy of the vertex-dependent arrays, fetched from HBM when a refit on the device left it stale ----------------------------
int refresh_host_copy(ptc_ctx* c);

// ---- ptc_api_image.cpp ---------------------------------------------------------------------------------------------------------------------------
DevAdaptive dev_adaptive(const ptc_ctx* c);
int temporal_keep_positions(ptc_ctx* c);

}  // namespace ptc_detail

